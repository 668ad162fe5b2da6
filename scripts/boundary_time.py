"""Boundary loss (csrc/boundary.hip, mi355.nn.RegionBoundaryLoss) against the train step it rides on and against the usual host
route for its distance maps; one JSON line.

    timeout -k 10 600 python scripts/boundary_time.py

``step_combined_ms`` / ``step_region_boundary_ms`` = the Attention U-Net 256^2 bs 32 bf16 train step (zero_grad, forward, loss,
backward, clip, AdamW — the body of bench.py's step) with CombinedLoss and with RegionBoundaryLoss(boundary_weight=0.01) on the same
batch.  Per workload (32 x 256^2, 16 x 512^2): ``map_ms`` = mi355_signed_dist2 alone on the batch's ellipse targets,
``map_noise_ms`` = the same call on p = 0.5 noise, where nearly every wave of the row pass holds both classes and scans both rows
(the whole O(B H W W) work), ``loss_fwd_bwd_ms`` = the boundary term's three launches given the map, ``host_ms`` = the route the map
replaces on the same box: device-to-host copy of the targets, scipy.ndimage.distance_transform_edt twice per image, Kervadec's
expression, host-to-device copy of phi (skipped, and said so, where scipy does not import).  Device times are CUDA-event medians
over --iters calls after --warmup calls, the host time a wall-clock median over --host-iters."""
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

from mi355 import nn as mnn, optim as moptim  # noqa: E402
from mi355.lib import lib  # noqa: E402
from models.segmentation_models.AttentionUNet import AttentionUNet  # noqa: E402
from oracle import train as otrain  # noqa: E402
from utils import distance  # noqa: E402


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


def host_route(masks, ndi):
    """what a trainer does without the kernel: copy, scipy per image, copy back -> phi [B, H, W] on the device"""
    t = masks.cpu().numpy()[:, 0] > 0.5
    out = np.zeros(t.shape, dtype=np.float32)
    for b, pos in enumerate(t):
        if pos.any() and not pos.all():
            neg = ~pos
            out[b] = ndi.distance_transform_edt(neg) * neg - (ndi.distance_transform_edt(pos) - 1) * pos
    return torch.from_numpy(out).to(masks.device)


def step_ms(crit, x, y, warmup, iters):
    model = AttentionUNet()
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    model.engine._check_storage()
    opt = moptim.AdamW(model.parameters(), lr=1e-6, weight_decay=5e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(x), y)
        loss.backward()
        moptim.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
        return loss

    for _ in range(warmup):
        loss = step()
    torch.cuda.synchronize()
    return med_ms(step, iters), float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=3)
    a = ap.parse_args()
    try:
        import scipy
        import scipy.ndimage as ndi
        scipy_version = scipy.__version__
    except ImportError:
        ndi, scipy_version = None, None
        print("scipy does not import here: the host route is not timed", file=sys.stderr)
    res = {"model": "AttentionUNet", "dtype": "bf16", "scipy": scipy_version, "workloads": []}
    x, mask = otrain.synthetic_batch(32, 256, seed=256)
    x, mask = x.cuda(), mask.cuda()
    res["step_combined_ms"], res["loss_combined"] = (round(v, 4) for v in step_ms(mnn.CombinedLoss(), x, mask, a.warmup, a.iters))
    res["step_region_boundary_ms"], res["loss_region_boundary"] = (
        round(v, 4) for v in step_ms(mnn.RegionBoundaryLoss(boundary_weight=0.01), x, mask, a.warmup, a.iters))
    res["boundary_over_step"] = round(res["step_region_boundary_ms"] / res["step_combined_ms"] - 1.0, 4)
    for bs, size in ((32, 256), (16, 512)):
        _, mask = otrain.synthetic_batch(bs, size, seed=size)
        mask = mask.cuda()
        noise = (torch.rand(bs, 1, size, size, generator=torch.Generator().manual_seed(2)) < 0.5).float().cuda()
        z = torch.randn(bs, 1, size, size, generator=torch.Generator().manual_seed(1)).cuda()
        sd2 = distance.signed_distance2(mask)
        per = size * size
        rows = lib.mi355_boundary_loss_rows(bs, per)
        partial, loss, dz = torch.empty(rows, device="cuda"), torch.empty(1, device="cuda"), torch.empty_like(z)

        def term():
            lib.mi355_boundary_loss_fwd(z, sd2, bs, per, 0.01, None, partial, loss)
            lib.mi355_boundary_loss_bwd(z, sd2, bs, per, 0.01, None, 0, dz)

        for _ in range(a.warmup):
            distance.signed_distance2(mask)
            distance.signed_distance2(noise)
            term()
        torch.cuda.synchronize()
        w = {"bs": bs, "size": size,
             "map_ms": round(med_ms(lambda: distance.signed_distance2(mask), a.iters), 4),
             "map_noise_ms": round(med_ms(lambda: distance.signed_distance2(noise), a.iters), 4),
             "loss_fwd_bwd_ms": round(med_ms(term, a.iters), 4)}
        if ndi is not None:
            ts = []
            for _ in range(a.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = host_route(mask, ndi)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            w["host_ms"] = round(statistics.median(ts), 3)
            w["host_over_map"] = round(w["host_ms"] / w["map_ms"], 1)
            w["max_abs_diff_vs_host"] = float((distance.signed_distance_map(mask) - host).abs().max())
        res["workloads"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
