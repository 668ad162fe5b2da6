"""Multi-class segmentation (csrc/mcseg.hip, mi355.nn.MultiClassSegLoss, utils/multiclass.py) against the train step it rides on and
against the plain-torch route, in one process; one JSON line.

    timeout -k 10 600 python scripts/multiclass_time.py

``step_*_ms`` = the Attention U-Net 256^2 bs 32 bf16 train step (zero_grad, forward, loss, backward, clip, AdamW — the body of
bench.py's step) on one batch: ``step_binary_ms`` the one-channel model under CombinedLoss(0.5, 0.5), ``step_multiclass_ms`` the
``out_channel=4`` model under MultiClassSegLoss(4, 0.5, 0.5); median, minimum and maximum over --iters steps.
Per shape (32 x 4 x 256^2 and 16 x 4 x 512^2), device times as CUDA-event medians after --warmup calls:
``loss_fwd_ms`` / ``loss_bwd_ms`` = the two loss launches alone (the forward includes its one-workgroup fold), ``confusion_ms`` the
argmax / confusion pass with predictions; ``*_gbs`` = the bytes the pass has to move (forward: logits + labels; backward: logits +
labels + the gradient; confusion: logits + labels + predictions) over that time; ``torch_loss_ms`` = F.cross_entropy + a one-hot
soft Dice, forward and backward through autograd, ``torch_confusion_ms`` = argmax + bincount per image; ``torch_over_*`` the ratios."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mi355 import nn as mnn, optim as moptim  # noqa: E402
from mi355.lib import lib  # noqa: E402
from models.segmentation_models.AttentionUNet import AttentionUNet  # noqa: E402
from oracle import train as otrain  # noqa: E402

ROW = mnn.MCSEG_ROW


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


def step_ms(model, crit, x, y, warmup, iters):
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


def labels_from_mask(mask, classes):
    """class-index labels from the binary ellipse: k shifted copies stacked, 0 outside"""
    m = mask[:, 0] > 0.5
    lab = torch.zeros(m.shape, dtype=torch.uint8)
    for k in range(1, classes):
        lab[m & (mask.roll(12 * (k - 1), dims=3)[:, 0] > 0.5)] = k
    return lab


def torch_loss(z, y64, C, smooth=1.0):
    z = z.detach().requires_grad_(True)
    ce = F.cross_entropy(z, y64, ignore_index=255)
    v = y64 != 255
    oh = F.one_hot(torch.where(v, y64, torch.zeros_like(y64)), C).permute(0, 3, 1, 2).float() * v[:, None]
    p = torch.softmax(z, 1) * v[:, None]
    dice = (2 * (p * oh).sum((0, 2, 3)) + smooth) / (p.sum((0, 2, 3)) + oh.sum((0, 2, 3)) + smooth)
    (0.5 * ce + 0.5 * (1 - dice.mean())).backward()
    return z.grad


def torch_confusion(z, y64, C):
    pred = z.argmax(1)
    v = y64 < C
    idx = torch.where(v, y64 * C + pred, torch.full_like(y64, C * C)) + torch.arange(z.shape[0], device=z.device).view(-1, 1, 1) * (C * C + 1)
    return torch.bincount(idx.reshape(-1), minlength=z.shape[0] * (C * C + 1)).view(z.shape[0], C * C + 1)[:, : C * C]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-step", action="store_true", help="skip the two train steps (kernels and the torch route only)")
    a = ap.parse_args()
    C = 4
    res = {"model": "AttentionUNet", "dtype": "bf16", "bs": 32, "size": 256, "classes": C}
    if not a.no_step:
        x, mask = otrain.synthetic_batch(32, 256, seed=256)
        lab = labels_from_mask(mask, C)
        x, mask, lab = x.cuda(), mask.cuda(), lab.cuda()
        res["step_binary_ms"] = step_ms(AttentionUNet(), mnn.CombinedLoss(0.5, 0.5), x, mask, a.warmup, a.iters)
        res["step_multiclass_ms"] = step_ms(AttentionUNet(out_channel=C), mnn.MultiClassSegLoss(C, 0.5, 0.5), x, lab, a.warmup, a.iters)
        res["multiclass_over_binary_step"] = round(res["step_multiclass_ms"]["median"] / res["step_binary_ms"]["median"] - 1.0, 4)
    res["kernels"] = []
    for N, S in ((32, 256), (16, 512)):
        HW = S * S
        g = torch.Generator().manual_seed(N)
        z = (torch.randn(N, C, S, S, generator=g) * 3).cuda()
        y = torch.randint(0, C, (N, S, S), generator=g).to(torch.uint8)
        y[:, :4] = 255
        y = y.cuda()
        y64 = y.long()
        rows = lib.mi355_mcseg_rows(N, HW)
        partial = torch.empty(rows * ROW, dtype=torch.float64, device="cuda")
        state = torch.empty(2 + 2 * N * C, dtype=torch.float64, device="cuda")
        loss, dz = torch.empty(3, device="cuda"), torch.empty_like(z)
        conf = torch.empty(N, C, C, dtype=torch.int32, device="cuda")
        pred = torch.empty(N, HW, dtype=torch.uint8, device="cuda")
        calls = {"loss_fwd_ms": lambda: lib.mi355_mcseg_loss_fwd(z, y, N, C, HW, None, 255, 0.5, 0.5, 1.0, 0, 1, partial, state, loss),
                 "loss_bwd_ms": lambda: lib.mi355_mcseg_loss_bwd(z, y, N, C, HW, None, 255, 0.5, 0.5, state, None, dz),
                 "confusion_ms": lambda: lib.mi355_mcseg_confusion(z, y, N, C, HW, 255, conf, pred),
                 "torch_loss_ms": lambda: torch_loss(z, y64, C),
                 "torch_confusion_ms": lambda: torch_confusion(z, y64, C)}
        w = {"N": N, "C": C, "H": S, "W": S}
        for name, fn in calls.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            w[name] = times_ms(fn, a.iters)["median"]
        zb, yb = 4 * N * C * HW, N * HW
        w["loss_fwd_gbs"] = round((zb + yb) / w["loss_fwd_ms"] / 1e6, 1)
        w["loss_bwd_gbs"] = round((2 * zb + yb) / w["loss_bwd_ms"] / 1e6, 1)
        w["confusion_gbs"] = round((zb + 2 * yb) / w["confusion_ms"] / 1e6, 1)
        w["torch_over_loss"] = round(w["torch_loss_ms"] / (w["loss_fwd_ms"] + w["loss_bwd_ms"]), 2)
        w["torch_over_confusion"] = round(w["torch_confusion_ms"] / w["confusion_ms"], 2)
        # the two routes agree (the torch route is fp32: a loose check that the same thing was timed)
        gt = torch_loss(z, y64, C)
        assert float((gt - dz).abs().max()) <= 1e-3 * float(dz.abs().max()), "the torch route computes another gradient"
        assert torch.equal(torch_confusion(z, y64, C).view(N, C, C).to(torch.int32), conf), "the torch route counts differently"
        res["kernels"].append(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
