"""Weight averaging (csrc/weight_avg.hip, mi355/averaging.py): what ``WeightAverage.update()`` adds to a train step, the update kernel
alone against the bytes it must move, and what a ``swap()`` costs; three JSON lines.

    timeout -k 10 300 python scripts/averaging_time.py      # Attention U-Net 256 x 256, batch 32, bf16: bench.py's step

One process.  Times are device-event windows of --calls calls each, --rounds windows per variant, the variants ALTERNATING round by
round after --warmup calls of each; reported: the median window per call and the spread (fastest / slowest window).  The update
reads the average and the parameters and writes the average: 12 bytes per parameter (padding included), which is what ``GB/s`` is
computed from.  The exchange reads and writes both: 16 bytes per parameter."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from mi355 import nn as mnn, optim as moptim  # noqa: E402
from mi355.averaging import WeightAverage  # noqa: E402
from mi355.lib import lib  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5, help="train steps per window (the kernel windows take 20 times as many calls)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing is timed on the CPU")
    from oracle import train as otrain
    from utils.helpers import get_seg_model
    torch.manual_seed(0)
    model = get_seg_model("attentionunet")
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    crit = mnn.BCEWithLogitsLoss()
    opt = moptim.AdamW(model.parameters(), lr=1e-6, weight_decay=5e-4)
    x, y = (t.cuda() for t in otrain.synthetic_batch(a.bs, a.size, seed=0))
    avg = WeightAverage(model, mode="ema", decay=0.999, warmup=10)

    def step(update):
        opt.zero_grad(set_to_none=True)
        crit(model(x), y).backward()
        moptim.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
        if update:
            avg.update(opt)

    res = alternate({"step": lambda: step(False), "step_with_update": lambda: step(True)}, a.warmup, a.rounds, a.calls)
    d = res["step_with_update"]["median_ms"] - res["step"]["median_ms"]
    print(json.dumps({"part": "train step", "model": "AttentionUNet", "shape": [a.bs, 3, a.size, a.size], "dtype": "bf16",
                      "calls_per_window": a.calls, "rounds": a.rounds, **res, "update_adds_ms": round(d, 5),
                      "update_adds_percent": round(100 * d / res["step"]["median_ms"], 3)}))

    n = avg.flat.numel()
    flat_p = model.engine.flat_p
    nbuf = sum(b.numel() for b in avg._fbuf.values())
    kern = {
        "avg_update_flat": lambda: lib.mi355_avg_update(avg.flat, flat_p, n, 0, 0.999, 10.0, avg.count, None),
        "avg_update_table_bn": lambda: lib.mi355_avg_update_table(avg._tab_update, avg._n_buf_rows, 0, 0.999, 10.0, avg.count, None),
        "update": lambda: avg.update(opt),
    }
    res = alternate(kern, a.warmup, a.rounds, 20 * a.calls)
    ms = res["avg_update_flat"]["median_ms"]
    print(json.dumps({"part": "update kernels", "parameters_with_padding": n, "bytes": 12 * n, "bn_rows": avg._n_buf_rows, "bn_floats": nbuf,
                      "calls_per_window": 20 * a.calls, "rounds": a.rounds, **res, "avg_update_flat_GBps": round(12 * n / ms / 1e6, 1)}))

    def swap():
        with avg.swap():
            pass

    def exchange_twice():                     # out and back: the live weights are in place again after every call
        lib.mi355_swap_table(avg._tab_swap, 1 + avg._n_buf_rows)
        lib.mi355_swap_table(avg._tab_swap, 1 + avg._n_buf_rows)

    live = model.engine.flat_p.clone()
    res = alternate({"swap_in_and_out": swap, "swap_table_twice": exchange_twice}, a.warmup, a.rounds, 2 * a.calls)
    assert torch.equal(model.engine.flat_p, live), "the live weights are not where they were"
    ms = res["swap_table_twice"]["median_ms"] / 2
    print(json.dumps({"part": "swap", "rows": 1 + avg._n_buf_rows, "bytes_per_exchange": 16 * (n + nbuf), "calls_per_window": 2 * a.calls,
                      "rounds": a.rounds, **res, "swap_table_once_ms": round(ms, 5), "swap_table_GBps": round(16 * (n + nbuf) / ms / 1e6, 1),
                      "note": "swap_in_and_out = two exchanges plus the host-side num_batches_tracked copies; the next forward re-packs the weights"}))


if __name__ == "__main__":
    main()
