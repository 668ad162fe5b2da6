"""FocalTverskyLoss / FocalLoss / TverskyLoss (csrc/focal_tversky.hip) next to CombinedLoss (csrc/seg_loss.hip), and
FocalCrossEntropyLoss next to MixCrossEntropyLoss: forward + backward of the loss alone; two JSON lines.

    timeout -k 10 300 python scripts/focal_time.py      # seg losses at [32, 1, 256, 256] fp32, classifier losses at [4096, 3]

One process.  Times are device-event windows of --calls calls each, --rounds windows per criterion, the criteria ALTERNATING round by
round after --warmup calls of each; reported: the median window per call and the spread (fastest / slowest window) of each, and the
ratio of each new loss to the existing one of the same run.  ``bytes_per_pass`` is what one pass over the logits and the target must
move (forward: read both; backward: read both, write dz): the same for every segmentation loss here."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from mi355 import nn as mnn  # noqa: E402


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns, warmup, rounds, calls):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(window_ms(fn, calls))
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)} for k, v in ts.items()}


def make(crit, z, t):
    zz = z.clone().requires_grad_(True)

    def fn():
        zz.grad = None
        crit(zz, t).backward()
    return fn


def seg_losses(a):
    shape = (a.bs, 1, a.size, a.size)
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(*shape, generator=g) * 2).cuda()
    t = (torch.rand(*shape, generator=g) < 0.35).float().cuda()
    crits = {"bce_dice": mnn.CombinedLoss(), "focal_tversky": mnn.FocalTverskyLoss(), "focal": mnn.FocalLoss(),
             "focal_plus_focal_tversky": mnn.FocalTverskyLoss(0.5, 0.5), "tversky": mnn.TverskyLoss()}
    res = alternate({k: make(c, z, t) for k, c in crits.items()}, a.warmup, a.rounds, a.calls)
    n = z.numel()
    base = res["bce_dice"]["median_ms"]
    print(json.dumps({"part": "seg loss fwd+bwd", "shape": list(shape), "dtype": "fp32", "calls_per_window": a.calls, "rounds": a.rounds,
                      "bytes_per_pass": {"forward": 8 * n, "backward": 12 * n}, **res,
                      "over_bce_dice": {k: round(v["median_ms"] / base, 3) for k, v in res.items() if k != "bce_dice"}}))


def cls_losses(a):
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(a.rows, 3, generator=g) * 3).cuda()
    y = torch.randint(0, 3, (a.rows,), generator=g).cuda()
    w = [0.5, 2.0, 1.25]
    crits = {"ce_mix": mnn.MixCrossEntropyLoss(0.0, w), "ce_focal": mnn.FocalCrossEntropyLoss(2.0, w)}
    res = alternate({k: make(c, z, y) for k, c in crits.items()}, a.warmup, a.rounds, a.calls)
    print(json.dumps({"part": "cls loss fwd+bwd", "shape": [a.rows, 3], "dtype": "fp32 in, fp64 arithmetic", "calls_per_window": a.calls,
                      "rounds": a.rounds, **res, "ce_focal_over_ce_mix": round(res["ce_focal"]["median_ms"] / res["ce_mix"]["median_ms"], 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is timed on the CPU")
    seg_losses(a)
    cls_losses(a)


if __name__ == "__main__":
    main()
