"""Loss modules backed by the HIP library (utils/helpers.py:244-246 call sites).

``criterion(out, y)`` keeps torch's call shape; when ``out`` comes from a mi355 ``Net`` the
gradient w.r.t. the logits is written by the backward launch straight into the plan's static
``dout`` buffer, so no torch kernel sits between the loss and the model's backward plan."""
from __future__ import annotations

import torch
import torch.nn as nn

from .lib import lib


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, plan):
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=out.device)
        lib.mi355_bce_logits(o, target, loss, None, None, o.numel())
        ctx.o, ctx.t, ctx.plan = o, target, plan
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        n = o.numel()
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        scratch = torch.empty(1, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_bce_logits(o, t, scratch, dz, gs, n)
        return dz[:n].view(o.shape), None, None


class BCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() (mean reduction) on the HIP library."""

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        return _BCEFn.apply(out, target, getattr(out, "_mi355_plan", None))


class _SegLossFn(torch.autograd.Function):
    """Dice / BCE + Dice (csrc/seg_loss.hip): the forward leaves the loss and one coefficient pair per sample on the device, the
    backward is one pass that reads them together with the upstream gradient and writes dL/dlogits."""

    @staticmethod
    def forward(ctx, out, target, plan, bce_weight, dice_weight, smooth, per_sample):
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        B = o.shape[0]
        per = o.numel() // B
        rows = lib.mi355_seg_loss_rows(B, per)
        if rows <= 0:
            raise RuntimeError(f"mi355_seg_loss_rows failed: {lib.raw('mi355_last_error')().decode()}")
        # one buffer: [rows x 4 partial sums | (a_b, c_b) per sample | loss]
        buf = torch.empty(rows * 4 + 2 * B + 1, dtype=torch.float32, device=out.device)
        partial, state, loss = buf[: rows * 4], buf[rows * 4: rows * 4 + 2 * B], buf[rows * 4 + 2 * B:]
        lib.mi355_seg_loss_fwd(o, target, B, per, bce_weight, dice_weight, smooth, 1 if per_sample else 0, partial, state, loss)
        ctx.o, ctx.t, ctx.plan, ctx.state, ctx.bw = o, target, plan, state, bce_weight
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        n = o.numel()
        B = o.shape[0]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_seg_loss_bwd(o, t, B, n // B, ctx.bw, ctx.state, gs, dz)
        return dz[:n].view(o.shape), None, None, None, None, None, None


class CombinedLoss(nn.Module):
    """bce_weight * BCEWithLogits + dice_weight * Dice on the HIP library — the reference's CombinedLoss
    (utils/clip_seg_finetuner.py:61-74; its Dice term sums over the whole batch).  ``per_sample=True`` computes the Dice term per
    image and averages the B terms instead.  Deterministic: the same input gives the same bits."""

    def __init__(self, bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=False):
        super().__init__()
        if bce_weight < 0 or dice_weight < 0 or smooth < 0:
            raise ValueError(f"bce_weight, dice_weight and smooth must not be negative ({bce_weight}, {dice_weight}, {smooth})")
        self.bce_weight, self.dice_weight, self.smooth, self.per_sample = float(bce_weight), float(dice_weight), float(smooth), bool(per_sample)

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        return _SegLossFn.apply(out, target, getattr(out, "_mi355_plan", None), self.bce_weight, self.dice_weight, self.smooth,
                                self.per_sample)

    def extra_repr(self):
        return f"bce_weight={self.bce_weight}, dice_weight={self.dice_weight}, smooth={self.smooth}, per_sample={self.per_sample}"


class DiceLoss(CombinedLoss):
    """1 - (2 sum(p t) + smooth) / (sum p + sum t + smooth), p = sigmoid(logits) — the reference's DiceLoss
    (utils/clip_seg_finetuner.py:40-58): CombinedLoss(0, 1) on the same kernels."""

    def __init__(self, smooth=1.0, per_sample=False):
        super().__init__(0.0, 1.0, smooth, per_sample)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, smoothing, plan):
        o = out.detach().contiguous()
        t = target.to(torch.int64).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=out.device)
        lib.mi355_ce_smooth(o, t, loss, None, None, o.shape[0], o.shape[1], float(smoothing))
        ctx.o, ctx.t, ctx.plan, ctx.s = o, t, plan, float(smoothing)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        n = o.numel()
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        scratch = torch.empty(1, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_ce_smooth(o, t, scratch, dz, gs, o.shape[0], o.shape[1], ctx.s)
        return dz[:n].view(o.shape), None, None, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(label_smoothing=s) (mean reduction) on the HIP library."""

    def __init__(self, label_smoothing=0.0):
        super().__init__()
        self.label_smoothing = label_smoothing

    def forward(self, out, target):
        return _CEFn.apply(out.float(), target, self.label_smoothing, getattr(out, "_mi355_plan", None))
