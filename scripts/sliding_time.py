"""Sliding-window inference (csrc/sliding.hip, utils/sliding.py) against the forwards it feeds; one JSON line.

    timeout -k 10 600 python scripts/sliding_time.py --case 512
    timeout -k 10 600 python scripts/sliding_time.py --case 1024

Model: AttentionUNet, bf16 compute, eval mode.  Cases: 8 x 3 x 512^2 and 4 x 3 x 1024^2, tile 256, overlap 0.5, Gaussian weights,
chunks of 8 tiles (``--case all`` runs both in one process; one case per command keeps every GPU step under a time limit of its
own).  Per case: ``resized_forward_ms`` = one eval forward of the same images at 256^2 (what the tester does without the option);
``tiles_forward_ms`` = the chunked forwards alone (ceil(N P / 8) forwards of 8 x 3 x 256^2); ``sliding_ms`` = the whole
SlidingWindowSegmenter call; ``kernels_ms`` = the gather launches plus the blend alone, ``gather_ms`` / ``blend_ms`` each alone with
the bytes it moves at the least — gather: every tile in and out; blend: the tile maps in, mean + spread (4 B each) and the mask
(1 B) per pixel and one cover plane out — over its time; ``torch_ms`` = the same result by slicing the tiles out, accumulating
weight maps over slices and dividing, in torch.  Device times are CUDA-event medians over --iters calls after --warmup calls,
taken twice in alternation (both values are printed).  The yardstick is ``tiles_forward_ms`` on the same box in the same run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355.lib import lib  # noqa: E402
from utils import sliding  # noqa: E402
from utils.helpers import get_seg_model  # noqa: E402

TILE, OVERLAP, BATCH = 256, 0.5, 8
CASES = {"512": (8, 512), "1024": (4, 1024)}


def med_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def torch_route(x, z, ys, xs, w2d):
    """the tiles of x, then the blend of their logit maps z [N, Py, Px, T, T], with torch ops alone"""
    N, _, H, W = x.shape
    T = TILE
    tiles = torch.stack([x[:, :, y:y + T, c:c + T] for y in ys for c in xs], 1).reshape(-1, 3, T, T)
    num = torch.zeros(N, H, W, device=x.device)
    den = torch.zeros(H, W, device=x.device)
    lo = torch.full((N, H, W), float("inf"), device=x.device)
    hi = torch.full((N, H, W), float("-inf"), device=x.device)
    cover = torch.zeros(H, W, dtype=torch.uint8, device=x.device)
    for iy, y in enumerate(ys):
        for ix, c in enumerate(xs):
            v = z[:, iy, ix]
            num[:, y:y + T, c:c + T] += w2d * v
            den[y:y + T, c:c + T] += w2d
            lo[:, y:y + T, c:c + T] = torch.minimum(lo[:, y:y + T, c:c + T], v)
            hi[:, y:y + T, c:c + T] = torch.maximum(hi[:, y:y + T, c:c + T], v)
            cover[y:y + T, c:c + T] += 1
    mean = num / den
    return tiles, mean, hi - lo, cover, ((torch.sigmoid(mean) > 0.5) * 255).to(torch.uint8)


def run_case(model, N, size, warmup, iters):
    x = torch.randn(N, 3, size, size, device="cuda")
    small = F.interpolate(x, size=(TILE, TILE), mode="bilinear", align_corners=False).contiguous()
    seg = sliding.SlidingWindowSegmenter(model, TILE, OVERLAP, "gaussian", "logit", 0.5, BATCH)
    ys, xs = seg.grid(size, size)
    P = len(ys) * len(xs)
    total = N * P
    chunks = -(-total // BATCH)
    hy, hx = torch.tensor(ys, dtype=torch.int32), torch.tensor(xs, dtype=torch.int32)
    tiles = seg._tile_list(total, x.device)
    buf = torch.empty(BATCH, 3, TILE, TILE, device="cuda")
    z = torch.randn(total, TILE, TILE, device="cuda")
    w = torch.from_numpy(sliding.window_weights(TILE, "gaussian")).cuda()
    w2d = torch.outer(w, w)
    z5 = z.reshape(N, len(ys), len(xs), TILE, TILE)
    mean, spread = torch.empty(N, size, size, device="cuda"), torch.empty(N, size, size, device="cuda")
    cover, mask = torch.empty(size, size, dtype=torch.uint8, device="cuda"), torch.empty(N, size, size, dtype=torch.uint8, device="cuda")

    def gather():
        for k in range(0, total, BATCH):
            lib.mi355_tile_gather_f32(x, N, 3, size, size, TILE, hy, len(ys), hx, len(xs), tiles[k:k + BATCH], BATCH, buf)

    def blend():
        lib.mi355_tile_blend(z, N, size, size, TILE, hy, len(ys), hx, len(xs), w, w, 0, 0.5, None, mean, spread, cover, mask)

    def forwards():
        for _ in range(chunks):
            model(buf)

    fns = {"resized_forward_ms": lambda: model(small), "tiles_forward_ms": forwards, "sliding_ms": lambda: seg(x),
           "kernels_ms": lambda: (gather(), blend()), "gather_ms": gather, "blend_ms": blend,
           "torch_ms": lambda: torch_route(x, z5, ys, xs, w2d)}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    r = {"shape": [N, 3, size, size], "tile": TILE, "overlap": OVERLAP, "batch": BATCH, "tiles_per_image": P, "chunks": chunks,
         "gather_bytes": 2 * chunks * BATCH * 3 * TILE * TILE * 4, "blend_bytes": total * TILE * TILE * 4 + N * size * size * 9 + size * size}
    for _ in range(2):                                     # alternating, twice: the spread between the two rounds is in the output
        for k, fn in fns.items():
            r.setdefault(k, []).append(round(med_ms(fn, iters), 4))
    r["gather_gbs"] = [round(r["gather_bytes"] / t / 1e6, 1) for t in r["gather_ms"]]
    r["blend_gbs"] = [round(r["blend_bytes"] / t / 1e6, 1) for t in r["blend_ms"]]
    r["kernels_share_of_tiles_forward"] = [round(k / f, 4) for k, f in zip(r["kernels_ms"], r["tiles_forward_ms"])]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--case", choices=("512", "1024", "all"), default="all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sliding_time.py measures on the GPU: none found (there is no CPU fallback)")
    torch.manual_seed(0)
    model = get_seg_model("attentionunet")
    model.compute_dtype = torch.bfloat16
    model = model.cuda().eval()
    res = {"model": "AttentionUNet", "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cases": []}
    with torch.no_grad():
        for name in (("512", "1024") if a.case == "all" else (a.case,)):
            res["cases"].append(run_case(model, *CASES[name], a.warmup, a.iters))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
