"""BCEWithLogitsLoss vs CombinedLoss (Dice + BCE, csrc/seg_loss.hip): the loss alone and inside the train step; one JSON line per part.

    timeout -k 10 300 python scripts/seg_loss_time.py --part loss      # forward + backward of the loss at [32, 1, 256, 256] fp32
    timeout -k 10 600 python scripts/seg_loss_time.py --part step      # AttentionUNet 256^2 bs 32 bf16 train step with each criterion

One process per part.  Times are device-event windows of --calls calls each, --rounds windows per criterion, the two criteria
ALTERNATING round by round after --warmup calls of both; reported: the median window per call and the spread (fastest / slowest
window) of each.  ``bytes_per_pass`` is what one pass over the logits and the target must move (forward: read both; backward: read
both, write dz)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from mi355 import amp as mamp, nn as mnn, optim as moptim  # noqa: E402


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


def part_loss(a):
    shape = (a.bs, 1, a.size, a.size)
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(*shape, generator=g) * 2).cuda()
    t = (torch.rand(*shape, generator=g) < 0.35).float().cuda()
    crits = {"bce": mnn.BCEWithLogitsLoss(), "bce_dice": mnn.CombinedLoss(), "bce_dice_per_sample": mnn.CombinedLoss(per_sample=True)}

    def make(crit):
        zz = z.clone().requires_grad_(True)

        def fn():
            zz.grad = None
            crit(zz, t).backward()
        return fn
    res = alternate({k: make(c) for k, c in crits.items()}, a.warmup, a.rounds, a.calls)
    n = z.numel()
    print(json.dumps({"part": "loss fwd+bwd", "shape": list(shape), "dtype": "fp32", "calls_per_window": a.calls, "rounds": a.rounds,
                      "bytes_per_pass": {"forward": 8 * n, "backward": 12 * n}, **res,
                      "bce_dice_over_bce": round(res["bce_dice"]["median_ms"] / res["bce"]["median_ms"], 3)}))


def part_step(a):
    from utils.helpers import get_seg_model
    torch.manual_seed(0)
    model = get_seg_model("attentionunet")
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    model.engine._check_storage()
    opt = moptim.AdamW(model.parameters(), lr=1e-6, weight_decay=5e-4)
    scaler = mamp.GradScaler(enabled=False)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.bs, 3, a.size, a.size, generator=g).cuda()
    y = (torch.rand(a.bs, 1, a.size, a.size, generator=g) < 0.35).float().cuda()

    def make(crit):
        def fn():
            opt.zero_grad(set_to_none=True)
            loss = crit(model(x), y)
            scaler.scale(loss).backward()
            scaler.unscale_(opt)
            moptim.clip_grad_norm_(model.parameters(), max_norm=1.0)
            scaler.step(opt)
            scaler.update()
        return fn
    res = alternate({"bce": make(mnn.BCEWithLogitsLoss()), "bce_dice": make(mnn.CombinedLoss())}, a.warmup, a.rounds, a.calls)
    print(json.dumps({"part": "AttentionUNet train step", "bs": a.bs, "size": a.size, "dtype": "bf16", "calls_per_window": a.calls,
                      "rounds": a.rounds, **res, "bce_dice_over_bce": round(res["bce_dice"]["median_ms"] / res["bce"]["median_ms"], 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("loss", "step"), required=True)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--calls", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is timed on the CPU")
    d = {"loss": (20, 15, 200), "step": (5, 7, 10)}[a.part]
    a.warmup, a.rounds, a.calls = (v if v is not None else dv for v, dv in zip((a.warmup, a.rounds, a.calls), d))
    (part_loss if a.part == "loss" else part_step)(a)


if __name__ == "__main__":
    main()
