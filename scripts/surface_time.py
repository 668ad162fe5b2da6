"""Surface-distance metrics (csrc/surface.hip, utils.tester.surface_metrics_batch) against the eval forward they ride on and against
the usual host route, for the tester's batch (8 x 256^2) and a larger one (16 x 512^2); one JSON line.

    timeout -k 10 600 python scripts/surface_time.py

Per workload: ``forward_ms`` = AttentionUNet eval forward (bf16) of the batch; ``surface_ms`` = surface_metrics_batch on logits whose
contours are those of a trained model (the target ellipse of oracle.train.synthetic_batch, shifted, with a stray blob);
``surface_noise_ms`` = the same call on p = 0.5 noise, where nearly every pixel is a border pixel and the row pass does all of its
O(H W W) work; ``host_ms`` = the route it replaces on the same box: device-to-host copy of logits and masks, then per sample
scipy.ndimage binary_erosion + distance_transform_edt + numpy.percentile (skipped, and said so, where scipy does not import).
Device times are CUDA-event medians over --iters calls after --warmup calls, the host time a wall-clock median over --host-iters."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.segmentation_models.AttentionUNet import AttentionUNet  # noqa: E402
from oracle import train as otrain  # noqa: E402
from utils import tester  # noqa: E402


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


def host_route(logits, masks, ndi):
    """what an evaluation kit does without the kernel: copy, then scipy per sample -> [B, 4]"""
    z, t = logits.cpu().numpy()[:, 0], masks.cpu().numpy()[:, 0]
    st = ndi.generate_binary_structure(2, 1)
    out = []
    for p, m in zip(1.0 / (1.0 + np.exp(-z)) > 0.5, t > 0.5):
        bp, bt = p & ~ndi.binary_erosion(p, st, border_value=0), m & ~ndi.binary_erosion(m, st, border_value=0)
        if not (bp.any() and bt.any()):
            out.append([np.nan] * 4 if bp.any() != bt.any() else [0.0, 0.0, 0.0, 1.0])
            continue
        d_pt, d_tp = ndi.distance_transform_edt(~bt)[bp], ndi.distance_transform_edt(~bp)[bt]
        both = np.concatenate([d_pt, d_tp])
        out.append([both.max(), np.percentile(both, 95), 0.5 * (d_pt.mean() + d_tp.mean()), (both <= 2.0).mean()])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=5)
    a = ap.parse_args()
    try:
        import scipy
        import scipy.ndimage as ndi
        scipy_version = scipy.__version__
    except ImportError:
        ndi, scipy_version = None, None
        print("scipy does not import here: the host route is not timed", file=sys.stderr)
    model = AttentionUNet()
    model.compute_dtype = torch.bfloat16
    model = model.cuda().eval()
    res = {"model": "AttentionUNet", "dtype": "bf16", "scipy": scipy_version, "workloads": []}
    for bs, size in ((8, 256), (16, 512)):
        x, mask = otrain.synthetic_batch(bs, size, seed=size)
        x, mask = x.cuda(), mask.cuda()
        pred = torch.roll(mask, (size // 40, -size // 30), (2, 3))
        pred[:, :, size // 16:size // 16 + size // 32, -size // 8:-size // 8 + size // 32] = 1.0      # a stray blob far from the contour
        logits = (pred * 2 - 1) * 4.0
        noise_logits = torch.randn(bs, 1, size, size, generator=torch.Generator().manual_seed(1)).cuda()
        noise_mask = (torch.rand(bs, 1, size, size, generator=torch.Generator().manual_seed(2)) < 0.5).float().cuda()
        with torch.no_grad():
            for _ in range(a.warmup):
                model(x)
                tester.surface_metrics_batch(logits, mask, True)
                tester.surface_metrics_batch(noise_logits, noise_mask, True)
            torch.cuda.synchronize()
            fwd = med_ms(lambda: model(x), a.iters)
            surf = med_ms(lambda: tester.surface_metrics_batch(logits, mask, True), a.iters)
            worst = med_ms(lambda: tester.surface_metrics_batch(noise_logits, noise_mask, True), a.iters)
        w = {"bs": bs, "size": size, "forward_ms": round(fwd, 3), "surface_ms": round(surf, 3), "surface_noise_ms": round(worst, 3),
             "surface_over_forward": round(surf / fwd, 3)}
        dev = tester.surface_metrics_batch(logits, mask, True)
        got = np.stack([dev[k].cpu().numpy() for k in tester.SURFACE_KEYS], 1)
        w["hd95_mean_px"] = round(float(np.nanmean(got[:, 1])), 3)
        if ndi is not None:
            ts = []
            for _ in range(a.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = host_route(logits, mask, ndi)
                ts.append((time.perf_counter() - t0) * 1e3)
            w["host_ms"] = round(statistics.median(ts), 3)
            w["host_over_surface"] = round(w["host_ms"] / surf, 1)
            w["max_rel_diff_vs_host"] = float(np.nanmax(np.abs(got - host) / np.maximum(np.abs(host), 1e-300)))
        res["workloads"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
