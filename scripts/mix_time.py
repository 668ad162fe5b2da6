"""Mixup / CutMix (csrc/mix.hip, utils/mix.py) and the mixed-target cross-entropy (mi355_ce_mix) against what they ride on; one JSON
line.

    timeout -k 10 300 python scripts/mix_time.py

``step``: a ResNet18 train step as utils/helpers.py::train runs it (bs 16, 3 x 256^2, the model's default compute dtype, all layers
training) without a mixer + CrossEntropyLoss(0.1) and with BatchMix(0.2, 1.0) + MixCrossEntropyLoss(0.1): host wall time per
step with one synchronisation at the end of --iters steps, the loop's own regime.  ``mix``: BatchMix's call alone (host draw, one
upload, the kernel) and the kernel alone on a resident draw, with the bytes the kernel moves at the least (two reads and one write of
the batch) over its time; 16 x 3 x 256^2 and 32 x 3 x 512^2, mixup (an empty box) and CutMix (a quarter-area box).  ``ce``: mi355_ce_mix
against mi355_ce_smooth, loss + gradient, at 16 x 3 and 256 x 3 (both are one workgroup and bound by the launch).  Kernel times are
CUDA-event medians over --iters calls after --warmup calls, taken twice in alternation (both values are printed).  Nothing is gated on
these numbers."""
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
from utils.helpers import get_class_model  # noqa: E402
from utils.mix import BatchMix, kernel_lam  # noqa: E402


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


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(fns, measure, iters, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {}
    for _ in range(2):                                         # alternating, twice: the spread between the two rounds is in the output
        for k, fn in fns.items():
            out.setdefault(k, []).append(round(measure(fn, iters), 4))
    return out


def step_fn(model, opt, crit, x, y, mix):
    def step():
        xb, yb = (x, y) if mix is None else mix(x, y)
        opt.zero_grad(set_to_none=True)
        loss = crit(model(xb), yb)
        loss.backward()
        moptim.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_time.py measures on the GPU: none found (there is no CPU fallback)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"step": {}, "mix": [], "ce": []}

    bs, size = 16, 256
    x = torch.randn(bs, 3, size, size, device="cuda", generator=gen)
    y = torch.randint(0, 3, (bs,), device="cuda", generator=gen)
    fns = {}
    for tag, mix, crit in (("plain_ms", None, mnn.CrossEntropyLoss(label_smoothing=0.1)),
                           ("mixed_ms", BatchMix(0.2, 1.0, seed=0), mnn.MixCrossEntropyLoss(label_smoothing=0.1))):
        torch.manual_seed(0)
        model, _ = get_class_model("resnet18")
        model = model.to("cuda").train()
        fns[tag] = step_fn(model, moptim.AdamW(model.parameters(), lr=1e-6, weight_decay=5e-4), crit, x, y, mix)
    res["step"] = {"model": "resnet18", "bs": bs, "size": size, **alternate(fns, wall_ms, a.iters, a.warmup)}
    del fns

    for n, s in ((16, 256), (32, 512)):
        xb = torch.randn(n, 3, s, s, device="cuda", generator=gen)
        yb = torch.randint(0, 3, (n,), device="cuda", generator=gen)
        out = torch.empty_like(xb)
        perm = np.roll(np.arange(n), 1)
        draws = {"mixup": (perm, np.full(n, 0.3, np.float32), np.zeros((n, 4), np.int64)),
                 "cutmix": (perm, np.full(n, 0.75, np.float32), np.tile([s // 4, s // 4 + 1, 3 * s // 4, 3 * s // 4 + 1], (n, 1)))}
        fns = {}
        for kind, (p, l, b) in draws.items():
            pd, bd = torch.from_numpy(p.astype(np.int32)).cuda(), torch.from_numpy(b.astype(np.int32)).cuda()
            ld = torch.from_numpy(kernel_lam(l, b)).cuda()
            fns[f"kernel_{kind}_ms"] = lambda pd=pd, ld=ld, bd=bd: lib.mi355_mix_batch_f32(xb, pd, ld, bd, out, n, 3, s, s)
        mixer = BatchMix(0.2, 1.0, seed=0)
        fns["call_ms"] = lambda: mixer(xb, yb)
        w = {"bs": n, "size": s, "bytes": 3 * xb.numel() * 4, **alternate(fns, med_ms, a.iters, a.warmup)}
        w["call_wall_ms"] = [round(wall_ms(fns["call_ms"], a.iters), 4) for _ in range(2)]
        for kind in draws:
            w[f"kernel_{kind}_gbs"] = [round(w["bytes"] / t / 1e6, 1) for t in w[f"kernel_{kind}_ms"]]
        res["mix"].append(w)
        del fns, xb, out

    for B in (16, 256):
        z = torch.randn(B, 3, device="cuda", generator=gen)
        ya, yb = (torch.randint(0, 3, (B,), device="cuda", generator=gen) for _ in range(2))
        lam = torch.rand(B, device="cuda", generator=gen)
        wgt = torch.tensor([0.8, 1.0, 1.3], device="cuda")
        loss, dz = torch.empty(1, device="cuda"), torch.empty(B, 3, device="cuda")
        fns = {"ce_smooth_ms": lambda: lib.mi355_ce_smooth(z, ya, loss, dz, None, B, 3, 0.1),
               "ce_mix_hard_ms": lambda: lib.mi355_ce_mix(z, ya, None, None, None, loss, dz, None, B, 3, 0.1),
               "ce_mix_ms": lambda: lib.mi355_ce_mix(z, ya, yb, lam, wgt, loss, dz, None, B, 3, 0.1)}
        res["ce"].append({"B": B, "C": 3, **alternate(fns, med_ms, a.iters, a.warmup)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
