"""Elastic deformation (csrc/elastic.hip, utils/gpu_transforms.py ``elastic=``) against the train transform it rides on and against
the usual host route; one JSON line.

    timeout -k 10 600 python scripts/elastic_time.py

Workload: 32 images of 299 x 299 x 3 with 256 x 256 masks (the COVID-19 Radiography files) -> 256^2, sigma 20.5 (R = 82, 165 taps),
alpha 512.  ``transform_ms`` / ``transform_elastic_ms`` = SegBatchTransform(256, train=True) on the resident uint8 batch without and
with ``elastic=(512, 20.5, 1.0)`` (every sample deformed: the upper end; the host-side parameter draws are inside both);
``blur_ms`` = mi355_sepblur_reflect_f32 alone on the batch's 64 planes of 256^2, with the LDS and FMA work it implies
(``blur_lds_read_gb``: 4 bytes per window element, H pass 1 per 16 outputs and tap, W pass 1 per output and tap);
``noise_ms`` = torch.rand on the device; ``warp_field_ms`` / ``warp_ms`` = image and mask warps with and without the field;
``host_ms`` = the route the stage replaces on the same box: per image numpy noise, scipy.ndimage.gaussian_filter per displacement
component, map_coordinates per channel (order 1) and for the mask (order 0), on the affine-warped uint8 batch, one image per task
on a pool of --host-threads threads (skipped, and said so, where scipy does not import).  Device times are CUDA-event medians
over --iters calls after --warmup calls, the host time a wall-clock median over --host-iters.  The yardstick is bench.py's train
step on the same box."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mi355.lib import lib  # noqa: E402
from utils import elastic  # noqa: E402
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


def host_route(imgs, msks, alpha, sigma, ndi, pool, seed):
    """what a trainer does without the kernels: per image noise, two Gaussian filters, map_coordinates per channel and for the mask"""
    h, w = imgs.shape[1:3]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)

    def one(i):
        g = np.random.default_rng(seed + i)
        dx = ndi.gaussian_filter(g.random((h, w), dtype=np.float32) * 2 - 1, sigma, mode="reflect") * alpha
        dy = ndi.gaussian_filter(g.random((h, w), dtype=np.float32) * 2 - 1, sigma, mode="reflect") * alpha
        co = [yy + dy, xx + dx]
        img = np.stack([ndi.map_coordinates(imgs[i, ..., c], co, order=1, mode="mirror") for c in range(imgs.shape[-1])], axis=-1)
        return img, ndi.map_coordinates(msks[i], co, order=0, mode="mirror")

    out = list(pool.map(one, range(imgs.shape[0])))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("elastic_time.py measures on the GPU: none found (there is no CPU fallback)")
    try:
        import scipy
        import scipy.ndimage as ndi
        scipy_version = scipy.__version__
    except ImportError:
        ndi, scipy_version = None, None
        print("scipy does not import here: the host route is not timed", file=sys.stderr)
    bs, size, sigma, alpha = 32, 256, 20.5, 512.0
    g = np.random.default_rng(0)
    imgs = torch.from_numpy(g.integers(0, 256, (bs, 299, 299, 3), dtype=np.uint8)).cuda()
    msks = torch.from_numpy((g.random((bs, 256, 256)) < 0.5).astype(np.uint8) * 255).cuda()
    taps, r = elastic.gaussian_taps(sigma)
    res = {"bs": bs, "size": size, "sigma": sigma, "alpha": alpha, "radius": r, "scipy": scipy_version}

    plain = SegBatchTransform(size, train=True, seed=0, device="cuda")
    el = SegBatchTransform(size, train=True, seed=0, device="cuda", elastic=(alpha, sigma, 1.0))
    noise = torch.rand(bs, 2, size, size, device="cuda") * 2 - 1
    tdev = torch.from_numpy(taps).cuda()
    tmp, field = torch.empty_like(noise), torch.empty_like(noise)
    img = torch.empty(bs, size, size, 3, dtype=torch.uint8, device="cuda").random_(0, 256)
    msk = torch.empty(bs, size, size, 1, dtype=torch.uint8, device="cuda").random_(0, 2) * 255
    img2, msk2 = torch.empty_like(img), torch.empty_like(msk)
    m1 = torch.tensor(plain.draw(bs)[0], dtype=torch.float32, device="cuda")
    al = torch.full((bs,), alpha, device="cuda")

    def blur():
        lib.mi355_sepblur_reflect_f32(noise, bs * 2, size, size, tdev, r, tmp, field)

    def warp_field():
        lib.mi355_warp_field_u8(img, bs, size, size, 3, m1, field, al, img2, size, size, 0, 1)
        lib.mi355_warp_field_u8(msk, bs, size, size, 1, m1, field, al, msk2, size, size, 1, 1)

    def warp():
        lib.mi355_warp_u8(img, bs, size, size, 3, m1, img2, size, size, 0, 1)
        lib.mi355_warp_u8(msk, bs, size, size, 1, m1, msk2, size, size, 1, 1)

    def draw_noise():
        return torch.rand(bs, 2, size, size, device="cuda") * 2 - 1

    fns = {"transform_ms": lambda: plain(imgs, msks), "transform_elastic_ms": lambda: el(imgs, msks), "blur_ms": blur,
           "noise_ms": draw_noise, "warp_field_ms": warp_field, "warp_ms": warp}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(2):                                     # alternating, twice: the spread between the two rounds is in the output
        for k, fn in fns.items():
            res.setdefault(k, []).append(round(med_ms(fn, a.iters), 4))
    outs, ntaps = bs * 2 * size * size, 2 * r + 1
    res["blur_fma"] = 2 * outs * ntaps
    res["blur_lds_read_gb"] = round((outs * ntaps / 16 + outs * ntaps) * 4 / 1e9, 3)
    res["blur_hbm_min_mb"] = round(4 * outs * 4 / 1e6, 1)  # each pass reads and writes the plane set once
    if ndi is not None:
        hi, hm = img.cpu().numpy(), msk.cpu().numpy()[..., 0]
        ts = []
        with ThreadPoolExecutor(a.host_threads) as pool:
            for it in range(a.host_iters):
                t0 = time.perf_counter()
                host_route(hi, hm, alpha, sigma, ndi, pool, it * bs)
                ts.append((time.perf_counter() - t0) * 1e3)
        res["host_ms"], res["host_threads"] = round(statistics.median(ts), 2), a.host_threads
    print(json.dumps(res))


if __name__ == "__main__":
    main()
