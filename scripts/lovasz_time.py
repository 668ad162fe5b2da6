"""Lovasz hinge (csrc/lovasz.hip on csrc/segsort.hip, mi355.nn.RegionLovaszLoss) against the train step it rides on, and the
segmented sort against torch.sort on the device; one JSON line.

    timeout -k 10 600 python scripts/lovasz_time.py [--parent-lib <libmi355conv.so built from the parent commit>]

``step_*_ms`` = the Attention U-Net 256^2 bs 32 bf16 train step (zero_grad, forward, loss, backward, clip, AdamW — the body of
bench.py's step) on one batch with CombinedLoss(0.5, 0), RegionLovaszLoss(per_image=True) and RegionLovaszLoss(per_image=False):
median, minimum and maximum over --iters steps, so the criterion's cost can be read against the step's own run-to-run spread.
``--parent-lib``: the CombinedLoss step once more in a fresh process on that library (MI355_LIB), the parent commit on the same box.
Per sort shape (32 x 65536 = per image, 1 x 2097152 = the batch): ``segsort_ms`` = mi355_segsort_f32 alone, ``torch_sort_ms`` =
torch.sort(stable=True) of the same keys (values and indices), ``lovasz_fwd_ms`` / ``lovasz_bwd_ms`` = the two loss launches alone
(the forward includes its sort).  Device times are CUDA-event medians after --warmup calls."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from mi355 import nn as mnn, optim as moptim  # noqa: E402
from mi355.lib import lib  # noqa: E402
from models.segmentation_models.AttentionUNet import AttentionUNet  # noqa: E402
from oracle import train as otrain  # noqa: E402


def times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


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
    t = times_ms(step, iters)
    t["loss"] = round(float(loss.detach()), 6)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--only-combined", action="store_true", help="time the CombinedLoss step alone (what --parent-lib runs)")
    ap.add_argument("--parent-lib", default=None, help="a libmi355conv.so built from the parent commit")
    a = ap.parse_args()
    x, mask = otrain.synthetic_batch(32, 256, seed=256)
    x, mask = x.cuda(), mask.cuda()
    res = {"model": "AttentionUNet", "dtype": "bf16", "bs": 32, "size": 256}
    res["step_combined_ms"] = step_ms(mnn.CombinedLoss(0.5, 0.0), x, mask, a.warmup, a.iters)
    if a.only_combined:
        print(json.dumps(res))
        return
    res["step_region_lovasz_image_ms"] = step_ms(mnn.RegionLovaszLoss(per_image=True), x, mask, a.warmup, a.iters)
    res["step_region_lovasz_batch_ms"] = step_ms(mnn.RegionLovaszLoss(per_image=False), x, mask, a.warmup, a.iters)
    for k in ("image", "batch"):
        res[f"lovasz_{k}_over_step"] = round(res[f"step_region_lovasz_{k}_ms"]["median"] / res["step_combined_ms"]["median"] - 1.0, 4)
    if a.parent_lib:
        env = dict(os.environ, MI355_LIB=os.path.abspath(a.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-combined", "--warmup", str(a.warmup), "--iters",
                              str(a.iters)], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
        res["step_combined_parent_ms"] = json.loads(out.strip().splitlines()[-1])["step_combined_ms"]
    res["sort"] = []
    for S, n in ((32, 65536), (1, 2097152)):
        keys = torch.randn(S, n, generator=torch.Generator().manual_seed(1)).cuda()
        t = (torch.rand(S, n, generator=torch.Generator().manual_seed(2)) < 0.35).float().cuda()
        need = lib.raw("mi355_segsort_ws_ints")(S, n)
        ws, perm = torch.empty(need, dtype=torch.int32, device="cuda"), torch.empty(S, n, dtype=torch.int32, device="cuda")
        need_l = lib.raw("mi355_lovasz_ws_ints")(S, n)
        ws_l = torch.empty(need_l, dtype=torch.int32, device="cuda")
        coef, loss, dz = torch.empty(S * n, device="cuda"), torch.empty(1, device="cuda"), torch.zeros(S * n, device="cuda")
        calls = {"segsort_ms": lambda: lib.mi355_segsort_f32(keys, S, n, ws, need, perm),
                 "torch_sort_ms": lambda: torch.sort(keys, dim=1, stable=True),
                 "lovasz_fwd_ms": lambda: lib.mi355_lovasz_fwd(keys, t, S, n, 0.5, 0.5, None, ws_l, need_l, coef, loss),
                 "lovasz_bwd_ms": lambda: lib.mi355_lovasz_bwd(coef, S * n, None, 1, dz)}
        w = {"S": S, "len": n}
        for name, fn in calls.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            w[name] = times_ms(fn, a.iters)["median"]
        w["torch_over_segsort"] = round(w["torch_sort_ms"] / w["segsort_ms"], 2)
        res["sort"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
