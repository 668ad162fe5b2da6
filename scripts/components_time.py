"""Connected-component clean-up (csrc/components.hip, utils.postprocess.label_components_batch) against the eval forward it rides on
and against the usual host route, for ellipse masks (8 x 256^2), p = 0.5 noise of the same shape (the worst case: tens of thousands
of components) and a larger batch (16 x 512^2); one JSON line, also written to profiles/components_time.json.

    timeout -k 10 600 python scripts/components_time.py

Per workload: ``forward_ms`` = AttentionUNet eval forward (bf16) of the batch; ``components_ms`` = label_components_batch on the logits
with hole filling, a minimum area and keep-largest on (the longest route through the launcher), ``components_plain_ms`` = labelling
alone; ``host_ms`` = the route it replaces on the same box: device-to-host copy of the logits, then per sample
scipy.ndimage binary_fill_holes + label + sum + find_objects + center_of_mass (skipped, and said so, where scipy does not import).
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
from utils import postprocess as pp  # noqa: E402

SETTINGS = dict(connectivity=8, fill_holes=4, min_area=20, keep_largest=5, max_report=8)


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


def host_route(logits, ndi):
    """what a serving loop does without the kernel: copy, then scipy per sample -> kept-component count per sample"""
    z = logits.cpu().numpy()[:, 0]
    s4, s8 = ndi.generate_binary_structure(2, 1), ndi.generate_binary_structure(2, 2)
    out = []
    for m in 1.0 / (1.0 + np.exp(-z)) > 0.5:
        m = ndi.binary_fill_holes(m, structure=s4)
        lab, n = ndi.label(m, structure=s8)
        idx = np.arange(1, n + 1)
        area = ndi.sum(m, lab, idx) if n else np.zeros(0)
        order = np.lexsort((idx, -area))[:SETTINGS["keep_largest"]]
        keep = [k for k in order if area[k] >= SETTINGS["min_area"]]
        boxes = ndi.find_objects(lab)
        ndi.center_of_mass(m, lab, [idx[k] for k in keep]) if keep else None
        _ = np.isin(lab, [idx[k] for k in keep]), [boxes[k] for k in keep]
        out.append(len(keep))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_time.json"))
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
    res = {"model": "AttentionUNet", "dtype": "bf16", "scipy": scipy_version, "settings": SETTINGS, "workloads": []}
    for name, bs, size in (("ellipses", 8, 256), ("noise", 8, 256), ("ellipses", 16, 512)):
        x, mask = otrain.synthetic_batch(bs, size, seed=size)
        x = x.cuda()
        if name == "noise":
            logits = torch.randn(bs, 1, size, size, generator=torch.Generator().manual_seed(1)).cuda()
        else:
            pred = mask.clone()
            pred[:, :, size // 16:size // 16 + size // 32, -size // 8:-size // 8 + size // 32] = 1.0      # a stray blob
            pred[:, :, size // 2, size // 2] = 0.0                                                        # and a pin-hole
            logits = ((pred * 2 - 1) * 4.0).cuda()
        full = lambda: pp.label_components_batch(logits, True, **SETTINGS)
        plain = lambda: pp.label_components_batch(logits, True)
        with torch.no_grad():
            for _ in range(a.warmup):
                model(x)
                full()
                plain()
            torch.cuda.synchronize()
            fwd = med_ms(lambda: model(x), a.iters)
            t_full, t_plain = med_ms(full, a.iters), med_ms(plain, a.iters)
        r = full()
        w = {"input": name, "bs": bs, "size": size, "forward_ms": round(fwd, 3), "components_ms": round(t_full, 3),
             "components_plain_ms": round(t_plain, 3), "components_over_forward": round(t_full / fwd, 3),
             "components_mean": round(float(r["n_components"].double().mean()), 1), "status_max": int(r["out_i"][:, 7].max())}
        if ndi is not None:
            ts = []
            for _ in range(a.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = host_route(logits, ndi)
                ts.append((time.perf_counter() - t0) * 1e3)
            w["host_ms"] = round(statistics.median(ts), 3)
            w["host_over_components"] = round(w["host_ms"] / t_full, 1)
            w["kept_equal_to_host"] = bool(np.array_equal(host, r["n_kept"].cpu().numpy()))
        res["workloads"].append(w)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
