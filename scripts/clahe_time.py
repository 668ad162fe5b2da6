"""CLAHE (csrc/clahe.hip, utils/gpu_transforms.py ``clahe=``) against the transforms it rides on; one JSON line.

    timeout -k 10 300 python scripts/clahe_time.py

Workloads: 32 x 256^2 x 3 and 16 x 512^2 x 3, clip 4, grid 8 (tiles of 32^2 and 64^2), on narrow-band images (a smooth field of
100 +- 30 grey levels plus noise: what a chest film's histogram looks like, and the hard case for the LDS atomics) and, for the LUT
kernel, on uniform random bytes as well.  Per workload: ``lut_ms`` / ``apply_ms`` = the two kernels alone, with the bytes each one
moves at the least (``lut``: the image once in, the LUTs out; ``apply``: the image in and out plus the LUTs once) over its time;
``transform_ms`` / ``transform_clahe_ms`` = SegBatchTransform(size, train=...) on a resident uint8 batch of 299 x 299 files without
(= the transform as it was before the option existed: ``clahe=None`` launches nothing) and with ``clahe=(4, 8)``, train and eval.
Device times are CUDA-event medians over --iters calls after --warmup calls, taken twice in alternation (both values are printed).
The yardstick is bench.py's train step on the same box.  No host route is timed: cv2 is not a dependency of this project."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from mi355.lib import lib  # noqa: E402
from utils import clahe  # noqa: E402
from utils.gpu_transforms import SegBatchTransform  # noqa: E402


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


def narrow_band(n, h, w, c, gen):
    """uint8 [n, h, w, c] on the device: 100 + 30 sin cos + N(0, 2), the channels alike but for the noise"""
    y = torch.linspace(0, 6.28, h, device="cuda")[None, :, None, None]
    x = torch.linspace(0, 6.28, w, device="cuda")[None, None, :, None]
    ph = torch.rand(n, 1, 1, 1, device="cuda", generator=gen) * 6.28
    field = 100 + 30 * torch.sin(1.3 * y + ph) * torch.cos(0.9 * x + ph)
    return (field + 2 * torch.randn(n, h, w, c, device="cuda", generator=gen)).round().clamp(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clahe_time.py measures on the GPU: none found (there is no CPU fallback)")
    clip, grid = 4.0, 8
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"clip": clip, "grid": grid, "workloads": []}
    for bs, size in ((32, 256), (16, 512)):
        img = narrow_band(bs, size, size, 3, gen)
        rnd = torch.empty_like(img).random_(0, 256)
        files = narrow_band(bs, 299, 299, 3, gen)
        msks = (torch.rand(bs, 256, 256, device="cuda", generator=gen) < 0.5).to(torch.uint8) * 255
        th, tw = clahe.tile_geometry(size, size, grid, grid)
        lim = clahe.clip_count(clip, th * tw)
        luts = torch.empty(bs, 3, grid, grid, 256, dtype=torch.uint8, device="cuda")
        out = torch.empty_like(img)
        fns = {"lut_ms": lambda: lib.mi355_clahe_lut_u8(img, bs, size, size, 3, grid, grid, lim, luts),
               "lut_uniform_ms": lambda: lib.mi355_clahe_lut_u8(rnd, bs, size, size, 3, grid, grid, lim, luts),
               "apply_ms": lambda: lib.mi355_clahe_apply_u8(img, bs, size, size, 3, grid, grid, luts, out)}
        for train in (True, False):
            plain = SegBatchTransform(size, train=train, seed=0, device="cuda")
            eq = SegBatchTransform(size, train=train, seed=0, device="cuda", clahe=(clip, grid))
            tag = "train" if train else "eval"
            fns[f"transform_{tag}_ms"] = lambda t=plain: t(files, msks)
            fns[f"transform_{tag}_clahe_ms"] = lambda t=eq: t(files, msks)
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        w = {"bs": bs, "size": size, "tile": [th, tw], "clip_count": lim}
        for _ in range(2):                                     # alternating, twice: the spread between the two rounds is in the output
            for k, fn in fns.items():
                w.setdefault(k, []).append(round(med_ms(fn, a.iters), 4))
        w["lut_bytes"] = img.numel() + luts.numel()
        w["apply_bytes"] = 2 * img.numel() + luts.numel()
        w["lut_gbs"] = [round(w["lut_bytes"] / t / 1e6, 1) for t in w["lut_ms"]]
        w["lut_uniform_gbs"] = [round(w["lut_bytes"] / t / 1e6, 1) for t in w["lut_uniform_ms"]]
        w["apply_gbs"] = [round(w["apply_bytes"] / t / 1e6, 1) for t in w["apply_ms"]]
        res["workloads"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
