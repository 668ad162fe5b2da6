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


class _FocalTverskyFn(torch.autograd.Function):
    """Focal + (focal-)Tversky (csrc/focal_tversky.hip), the launches of _SegLossFn: the forward leaves the loss and one coefficient
    pair per sample on the device, the backward is one pass that reads them with the upstream gradient and writes dL/dlogits."""

    @staticmethod
    def forward(ctx, out, target, plan, cfg):
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        fw, fa, fg, tw, a, b, g, smooth, per_sample = cfg
        B = o.shape[0]
        per = o.numel() // B
        rows = lib.mi355_ftv_loss_rows(B, per)
        if rows <= 0:
            raise RuntimeError(f"mi355_ftv_loss_rows failed: {lib.raw('mi355_last_error')().decode()}")
        # one buffer: [rows x 4 partial sums | (A_b, C_b) per sample | loss]
        buf = torch.empty(rows * 4 + 2 * B + 1, dtype=torch.float32, device=out.device)
        partial, state, loss = buf[: rows * 4], buf[rows * 4: rows * 4 + 2 * B], buf[rows * 4 + 2 * B:]
        lib.mi355_ftv_loss_fwd(o, target, B, per, fw, fa, fg, tw, a, b, g, smooth, 1 if per_sample else 0, partial, state, loss)
        ctx.o, ctx.t, ctx.plan, ctx.state, ctx.cfg = o, target, plan, state, cfg
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        fw, fa, fg, _, a, b = ctx.cfg[:6]
        n = o.numel()
        B = o.shape[0]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_ftv_loss_bwd(o, t, B, n // B, fw, fa, fg, a, b, ctx.state, gs, dz)
        return dz[:n].view(o.shape), None, None, None


class FocalTverskyLoss(nn.Module):
    """focal_weight * focal + tversky_weight * (1 - TI)^exponent on the HIP library, one autograd node (mi355_ftv_loss_*).  The target
    is binarised at 0.5 inside the kernels.  With p = sigmoid(logits):

        focal = mean(alpha_t (1 - p_t)^focal_gamma BCEWithLogits)     torchvision.ops.sigmoid_focal_loss (Lin et al. 2017), mean;
                                                                      focal_alpha < 0: no alpha_t
        TI    = (TP + smooth) / (TP + alpha FP + beta FN + smooth)    Salehi et al. 2017; TP = sum p t, FP = sum p (1 - t), FN = sum (1 - p) t

    ``alpha`` weighs false positives and ``beta`` false negatives: beta > alpha trains for recall.  ``exponent`` = 1 is the Tversky
    loss, 0.75 the focal-Tversky loss of Abraham & Khan 2019 (their gamma = 4/3).  ``per_sample=True`` forms TI per image and averages
    the B terms.  Where the prediction is perfect and saturated (1 - TI = 0) the Tversky gradient is 0.  Deterministic: the same
    input gives the same bits."""

    def __init__(self, focal_weight=0.0, tversky_weight=1.0, alpha=0.7, beta=0.3, exponent=0.75, focal_alpha=0.25, focal_gamma=2.0,
                 smooth=1.0, per_sample=False):
        super().__init__()
        if not (focal_weight >= 0 and tversky_weight >= 0 and smooth >= 0):
            raise ValueError(f"focal_weight, tversky_weight and smooth must not be negative ({focal_weight}, {tversky_weight}, {smooth})")
        if not (alpha >= 0 and beta >= 0 and alpha + beta > 0):
            raise ValueError(f"alpha and beta must not be negative and not both 0 ({alpha}, {beta})")
        if not exponent > 0:
            raise ValueError(f"exponent must be positive ({exponent})")
        if not focal_gamma >= 0:
            raise ValueError(f"focal_gamma must not be negative ({focal_gamma})")
        if not focal_alpha <= 1:
            raise ValueError(f"focal_alpha must lie in [0, 1], or be negative for no class balance ({focal_alpha})")
        for name, v in (("focal_weight", focal_weight), ("tversky_weight", tversky_weight), ("alpha", alpha), ("beta", beta),
                        ("exponent", exponent), ("focal_alpha", focal_alpha), ("focal_gamma", focal_gamma), ("smooth", smooth)):
            if v in (float("inf"), float("-inf")):
                raise ValueError(f"{name} must be finite ({v})")
        self.focal_weight, self.tversky_weight, self.alpha, self.beta = float(focal_weight), float(tversky_weight), float(alpha), float(beta)
        self.exponent, self.focal_alpha, self.focal_gamma = float(exponent), float(focal_alpha), float(focal_gamma)
        self.smooth, self.per_sample = float(smooth), bool(per_sample)

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        cfg = (self.focal_weight, self.focal_alpha, self.focal_gamma, self.tversky_weight, self.alpha, self.beta, self.exponent,
               self.smooth, self.per_sample)
        return _FocalTverskyFn.apply(out, target, getattr(out, "_mi355_plan", None), cfg)

    def extra_repr(self):
        return (f"focal_weight={self.focal_weight}, tversky_weight={self.tversky_weight}, alpha={self.alpha}, beta={self.beta}, "
                f"exponent={self.exponent}, focal_alpha={self.focal_alpha}, focal_gamma={self.focal_gamma}, smooth={self.smooth}, "
                f"per_sample={self.per_sample}")


class FocalLoss(FocalTverskyLoss):
    """mean(alpha_t (1 - p_t)^gamma BCEWithLogits(logits, target)) — torchvision.ops.sigmoid_focal_loss(reduction="mean"); ``alpha`` < 0
    switches alpha_t off: FocalTverskyLoss(1, 0) on the same kernels."""

    def __init__(self, alpha=0.25, gamma=2.0):
        super().__init__(1.0, 0.0, focal_alpha=alpha, focal_gamma=gamma)


class TverskyLoss(FocalTverskyLoss):
    """1 - (TP + smooth) / (TP + alpha FP + beta FN + smooth) (Salehi et al. 2017): FocalTverskyLoss(0, 1, exponent=1) on the same
    kernels.  TverskyLoss(0.5, 0.5, smooth=s) is DiceLoss(smooth=2 s) on a binary target."""

    def __init__(self, alpha=0.5, beta=0.5, smooth=1.0, per_sample=False):
        super().__init__(0.0, 1.0, alpha, beta, 1.0, smooth=smooth, per_sample=per_sample)


def _signed_dist2(target, threshold=0.5):
    """mi355_signed_dist2 on a contiguous fp32 device tensor [B, H, W] -> int32 [B, H, W] (csrc/boundary.hip): the signed squared
    Euclidean distance map of ``target > threshold``.  No host round trip."""
    B, H, W = target.shape
    n = lib.raw("mi355_sdist_ws_ints")(B, H, W)
    if n <= 0:
        raise RuntimeError(f"mi355_sdist_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    ws = torch.empty(n, dtype=torch.int32, device=target.device)
    sd2 = torch.empty(B, H, W, dtype=torch.int32, device=target.device)
    lib.mi355_signed_dist2(target, B, H, W, float(threshold), ws, n, sd2)
    return sd2


class _RegionBoundaryFn(torch.autograd.Function):
    """region + boundary as ONE autograd node.  Every mi355 criterion's backward returns the plan's ``dout`` buffer, so two nodes
    would hand autograd two views of one buffer, the second launch having overwritten the first ("Boundary loss"): here
    the regional backward writes ``dz`` and the boundary backward accumulates into it.  ``region`` = (bce_weight, dice_weight,
    smooth, per_sample) or None for the boundary term alone; next to a regional loss a boundary weight of 0 launches nothing more
    than CombinedLoss does."""

    @staticmethod
    def forward(ctx, out, target, plan, region, boundary_weight, threshold):
        if out.dim() == 4 and out.shape[1] == 1:
            B, H, W = out.shape[0], out.shape[2], out.shape[3]
        elif out.dim() == 3:
            B, H, W = out.shape
        else:
            raise ValueError(f"the boundary loss is defined for one-channel logits [B,1,H,W] or [B,H,W], got {tuple(out.shape)}")
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        per = H * W
        rows_r = 0
        if region is not None:
            rows_r = lib.mi355_seg_loss_rows(B, per)
            if rows_r <= 0:
                raise RuntimeError(f"mi355_seg_loss_rows failed: {lib.raw('mi355_last_error')().decode()}")
        run_b = boundary_weight > 0 or region is None
        rows_b = 0
        if run_b:
            rows_b = lib.mi355_boundary_loss_rows(B, per)
            if rows_b <= 0:
                raise RuntimeError(f"mi355_boundary_loss_rows failed: {lib.raw('mi355_last_error')().decode()}")
        # one buffer: [rows_r x 4 regional partial sums | (a_b, c_b) per sample | regional loss, loss | boundary partial sums]
        buf = torch.empty(rows_r * 4 + 2 * B + 2 + rows_b, dtype=torch.float32, device=out.device)
        partial, state = buf[: rows_r * 4], buf[rows_r * 4: rows_r * 4 + 2 * B]
        base, loss, bpartial = buf[rows_r * 4 + 2 * B:][:1], buf[rows_r * 4 + 2 * B + 1:][:1], buf[rows_r * 4 + 2 * B + 2:]
        if region is not None:
            bw, dw, smooth, per_sample = region
            lib.mi355_seg_loss_fwd(o, target, B, per, bw, dw, smooth, 1 if per_sample else 0, partial, state,
                                   base if run_b else loss)
        sd2 = None
        if run_b:
            sd2 = _signed_dist2(target.view(B, H, W), threshold)
            lib.mi355_boundary_loss_fwd(o, sd2, B, per, boundary_weight, base if region is not None else None, bpartial, loss)
        ctx.o, ctx.t, ctx.plan, ctx.state, ctx.sd2 = o, target, plan, state, sd2
        ctx.region, ctx.w, ctx.run_b = region, boundary_weight, run_b
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        n = o.numel()
        B = o.shape[0]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        if ctx.region is not None:
            lib.mi355_seg_loss_bwd(o, t, B, n // B, ctx.region[0], ctx.state, gs, dz)
        if ctx.run_b:
            lib.mi355_boundary_loss_bwd(o, ctx.sd2, B, n // B, ctx.w, gs, 1 if ctx.region is not None else 0, dz)
        return dz[:n].view(o.shape), None, None, None, None, None


class BoundaryLoss(nn.Module):
    """weight * mean(sigmoid(logits) * phi), phi the signed Euclidean distance map of ``target > threshold`` (Kervadec et al., MIDL
    2019: negative inside the mask, positive outside, zero for a sample without a boundary), built on the device for every batch
    (csrc/boundary.hip).  Logits [B,1,H,W] or [B,H,W], H, W <= 1024.  Deterministic.  To add it to a regional loss use
    RegionBoundaryLoss: the sum of two mi355 criteria is not a valid loss (both write their gradient into the plan's ``dout``)."""

    def __init__(self, weight=1.0, threshold=0.5):
        super().__init__()
        if weight < 0:
            raise ValueError(f"weight must not be negative ({weight})")
        self.weight, self.threshold = float(weight), float(threshold)

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        return _RegionBoundaryFn.apply(out, target, getattr(out, "_mi355_plan", None), None, self.weight, self.threshold)

    def extra_repr(self):
        return f"weight={self.weight}, threshold={self.threshold}"


class RegionBoundaryLoss(nn.Module):
    """CombinedLoss(bce_weight, dice_weight, smooth, per_sample) plus the boundary loss, as one autograd node.

    ``schedule="constant"``: region + boundary_weight * boundary.  ``schedule="rebalance"`` (Kervadec): with
    a = min(boundary_weight + epoch * step, max_weight), (1 - a) * region + a * boundary; ``train()`` calls
    ``on_epoch(epoch_index, epochs)`` at the start of every epoch (epoch_index from 0).  The factor (1 - a) goes into the two regional
    weights handed to the kernels: no extra pass."""

    SCHEDULES = ("constant", "rebalance")

    def __init__(self, bce_weight=0.5, dice_weight=0.5, boundary_weight=0.01, smooth=1.0, per_sample=False, schedule="constant",
                 step=0.01, max_weight=0.99, threshold=0.5):
        super().__init__()
        if bce_weight < 0 or dice_weight < 0 or boundary_weight < 0 or smooth < 0:
            raise ValueError(f"bce_weight, dice_weight, boundary_weight and smooth must not be negative "
                             f"({bce_weight}, {dice_weight}, {boundary_weight}, {smooth})")
        if schedule not in self.SCHEDULES:
            raise ValueError(f"schedule must be one of {self.SCHEDULES}, got {schedule!r}")
        if step < 0 or not 0 <= max_weight <= 1:
            raise ValueError(f"step must not be negative and max_weight must lie in [0, 1] ({step}, {max_weight})")
        if schedule == "rebalance" and boundary_weight > 1:
            raise ValueError(f"schedule='rebalance' mixes (1 - a) * region + a * boundary: boundary_weight <= 1 expected ({boundary_weight})")
        self.bce_weight, self.dice_weight, self.boundary_weight = float(bce_weight), float(dice_weight), float(boundary_weight)
        self.smooth, self.per_sample, self.threshold = float(smooth), bool(per_sample), float(threshold)
        self.schedule, self.step, self.max_weight = schedule, float(step), float(max_weight)
        self.epoch = 0

    def on_epoch(self, epoch, epochs=None):
        self.epoch = int(epoch)

    def current_weights(self):
        """(factor of the regional loss, factor of the boundary loss) at the current epoch."""
        if self.schedule == "constant":
            return 1.0, self.boundary_weight
        a = min(self.boundary_weight + self.epoch * self.step, self.max_weight)
        return 1.0 - a, a

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        r, a = self.current_weights()
        region = (r * self.bce_weight, r * self.dice_weight, self.smooth, self.per_sample)
        return _RegionBoundaryFn.apply(out, target, getattr(out, "_mi355_plan", None), region, a, self.threshold)

    def extra_repr(self):
        return (f"bce_weight={self.bce_weight}, dice_weight={self.dice_weight}, boundary_weight={self.boundary_weight}, "
                f"smooth={self.smooth}, per_sample={self.per_sample}, schedule={self.schedule!r}, step={self.step}, "
                f"max_weight={self.max_weight}")


def _segmented_argsort(keys):
    """mi355_segsort_f32 on a contiguous fp32 device tensor [S, len] -> int32 [S, len] (csrc/segsort.hip): per segment the order of
    ``np.argsort(kind="stable")``.  No host round trip."""
    S, n = keys.shape
    need = lib.raw("mi355_segsort_ws_ints")(S, n)
    if need <= 0:
        raise RuntimeError(f"mi355_segsort_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    ws = torch.empty(need, dtype=torch.int32, device=keys.device)
    perm = torch.empty(S, n, dtype=torch.int32, device=keys.device)
    lib.mi355_segsort_f32(keys, S, n, ws, need, perm)
    return perm


def _lovasz_fwd(o, target, S, n, threshold, weight, base, loss):
    """mi355_lovasz_fwd on contiguous fp32 device tensors of S * n elements -> the per-pixel coefficients (fp32 [S * n])."""
    need = lib.raw("mi355_lovasz_ws_ints")(S, n)
    if need <= 0:
        raise RuntimeError(f"mi355_lovasz_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    ws = torch.empty(need, dtype=torch.int32, device=o.device)
    coef = torch.empty(S * n, dtype=torch.float32, device=o.device)
    lib.mi355_lovasz_fwd(o, target, S, n, float(threshold), float(weight), base, ws, need, coef, loss)
    return coef


def _rank_metrics(scores, target, labels, threshold, curve=False):
    """mi355_rank_metrics on a contiguous fp32 device tensor [S, len] with ``target`` (fp32 [S, len]) or ``labels`` (int32 [len]) ->
    (counts int64 [S, 4], ap float64 [S], None or (thresholds fp32 [S, len], tp int32 [S, len], fp int32 [S, len], npoints int32 [S]))
    (csrc/ranking.hip).  The curve rows are written up to npoints[s] only.  No host round trip."""
    S, n = scores.shape
    need = lib.raw("mi355_rank_ws_ints")(S, n)
    if need <= 0:
        raise RuntimeError(f"mi355_rank_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    dev = scores.device
    ws = torch.empty(need, dtype=torch.int32, device=dev)
    counts = torch.empty(S, 4, dtype=torch.int64, device=dev)
    ap = torch.empty(S, dtype=torch.float64, device=dev)
    pts = None
    if curve:
        pts = (torch.empty(S, n, dtype=torch.float32, device=dev), torch.empty(S, n, dtype=torch.int32, device=dev),
               torch.empty(S, n, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev))
    lib.mi355_rank_metrics(scores, target, labels, S, n, float(threshold), ws, need, counts, ap, *(pts or (None,) * 4))
    return counts, ap, pts


def _ws_ints(name, *shape):
    need = lib.raw(name)(*shape)
    if need <= 0:
        raise RuntimeError(f"{name} failed: {lib.raw('mi355_last_error')().decode()}")
    return need


def _boot_counts(n, replicates, seed, device):
    """mi355_boot_counts -> int32 [replicates + 1, n] multinomial resample weights, row 0 all ones (csrc/resample.hip)."""
    counts = torch.empty(replicates + 1, n, dtype=torch.int32, device=device)
    lib.mi355_boot_counts(int(seed) & 0xFFFFFFFFFFFFFFFF, replicates, n, counts)
    return counts


def _boot_rank(scores, target, labels, threshold, counts):
    """mi355_boot_rank on a contiguous fp32 device tensor [S, len] with ``target`` or ``labels`` as for _rank_metrics and int32 weights
    [R1, len] -> (int64 [R1, S, 3] = P, N, U2, float64 [R1, S] = ap).  No host round trip."""
    S, n = scores.shape
    R1 = counts.shape[0]
    need = _ws_ints("mi355_boot_rank_ws_ints", S, n)
    dev = scores.device
    ws = torch.empty(need, dtype=torch.int32, device=dev)
    pnu = torch.empty(R1, S, 3, dtype=torch.int64, device=dev)
    ap = torch.empty(R1, S, dtype=torch.float64, device=dev)
    lib.mi355_boot_rank(scores, target, labels, S, n, float(threshold), counts, R1, ws, need, pnu, ap)
    return pnu, ap


def _boot_confusion(pred, labels, classes, counts):
    """mi355_boot_confusion on int32 device tensors [n] and weights [R1, n] -> (int64 [R1, C, C], rows the truth; int64 [R1] = the
    weight of the samples skipped for a class id outside 0 .. C - 1)."""
    R1, n = counts.shape
    cm = torch.empty(R1, classes, classes, dtype=torch.int64, device=pred.device)
    bad = torch.empty(R1, dtype=torch.int64, device=pred.device)
    lib.mi355_boot_confusion(pred, labels, n, classes, counts, R1, cm, bad)
    return cm, bad


def _boot_sums(values, counts):
    """mi355_boot_sums on a contiguous float64 device tensor [M, n] and weights [R1, n] -> (float64 [R1, M] weighted sums, int64
    [R1, M] weights), both over the non-NaN values."""
    M, n = values.shape
    R1 = counts.shape[0]
    total = torch.empty(R1, M, dtype=torch.float64, device=values.device)
    weight = torch.empty(R1, M, dtype=torch.int64, device=values.device)
    lib.mi355_boot_sums(values, M, n, counts, R1, total, weight)
    return total, weight


def _boot_interval(reps, lo_q, hi_q):
    """mi355_boot_interval on a contiguous float64 device tensor [R1, K] -> float64 [K, 6] = point, mean, se, lo, hi, valid."""
    R1, K = reps.shape
    out = torch.empty(K, 6, dtype=torch.float64, device=reps.device)
    lib.mi355_boot_interval(reps, R1, K, float(lo_q), float(hi_q), out)
    return out


def _delong(scores, labels):
    """mi355_delong on a contiguous fp32 device tensor [M, C, n] and int32 labels [n] -> (v2 int64 [M, C, n], pnu int64 [M, C, 3],
    var float64 [M, C], cov float64 [C, M, M]).  No host round trip."""
    M, C, n = scores.shape
    need = _ws_ints("mi355_delong_ws_ints", M, C, n)
    dev = scores.device
    ws = torch.empty(need, dtype=torch.int32, device=dev)
    v2 = torch.empty(M, C, n, dtype=torch.int64, device=dev)
    pnu = torch.empty(M, C, 3, dtype=torch.int64, device=dev)
    var = torch.empty(M, C, dtype=torch.float64, device=dev)
    cov = torch.empty(C, M, M, dtype=torch.float64, device=dev)
    lib.mi355_delong(scores, labels, M, C, n, ws, need, v2, pnu, var, cov)
    return v2, pnu, var, cov


def _cls_calibration(x, labels, bins, is_prob):
    """mi355_cls_calibration on a contiguous fp32 device tensor [N, C] and int32 labels [N] -> (bin_count int64 [bins], bin_correct
    int64 [bins], bin_conf float64 [bins], out float64 [3] = NLL, Brier, ECE, scores_t fp32 [C, N]).  No host round trip."""
    N, C = x.shape
    need = lib.raw("mi355_cls_calibration_ws_ints")(N, C, bins)
    if need <= 0:
        raise RuntimeError(f"mi355_cls_calibration_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    dev = x.device
    ws = torch.empty(need, dtype=torch.int32, device=dev)
    bin_count = torch.empty(bins, dtype=torch.int64, device=dev)
    bin_correct = torch.empty(bins, dtype=torch.int64, device=dev)
    bin_conf = torch.empty(bins, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    scores_t = torch.empty(C, N, dtype=torch.float32, device=dev)
    lib.mi355_cls_calibration(x, N, C, 1 if is_prob else 0, labels, bins, ws, need, bin_count, bin_correct, bin_conf, out, scores_t)
    return bin_count, bin_correct, bin_conf, out, scores_t


def _temperature_fit(x, labels):
    """mi355_temperature_fit on a contiguous fp32 device tensor [N, C] and int32 labels [N] -> float64 [8] = beta, T, NLL at beta = 1,
    NLL at beta, g', g'', evaluations, status (csrc/calibrate.hip).  No host round trip."""
    N, C = x.shape
    need = _ws_ints("mi355_temperature_fit_ws_ints", N, C)
    ws = torch.empty(need, dtype=torch.int32, device=x.device)
    state = torch.empty(8, dtype=torch.float64, device=x.device)
    lib.mi355_temperature_fit(x, N, C, labels, ws, need, state)
    return state


def _temperature_eval(x, labels, beta_dev):
    """mi355_temperature_eval: the mean NLL and its first two derivatives in beta at ``beta_dev[0]`` (float64 device tensor) -> float64 [3]"""
    N, C = x.shape
    need = _ws_ints("mi355_temperature_fit_ws_ints", N, C)
    ws = torch.empty(need, dtype=torch.int32, device=x.device)
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    lib.mi355_temperature_eval(x, N, C, labels, beta_dev, ws, need, out)
    return out


def _logits_scale(x, beta_dev):
    """mi355_logits_scale: fp32 [N, C] times the double at ``beta_dev`` (a float64 device tensor, e.g. _temperature_fit's) -> fp32."""
    N, C = x.shape
    y = torch.empty_like(x)
    lib.mi355_logits_scale(x, N, C, beta_dev, y)
    return y


def _thr_sweep(scores, target, thr, is_logit, target_threshold):
    """mi355_thr_sweep on contiguous fp32 device tensors [B, len], [B, len] and ascending candidates [K] -> (tp int32 [B, K],
    fp int32 [B, K], pos int32 [B]).  No host round trip."""
    B, n = scores.shape
    K = thr.shape[0]
    need = _ws_ints("mi355_thr_sweep_ws_ints", B, n, K)
    dev = scores.device
    ws = torch.empty(need, dtype=torch.int32, device=dev)
    tp = torch.empty(B, K, dtype=torch.int32, device=dev)
    fp = torch.empty(B, K, dtype=torch.int32, device=dev)
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    lib.mi355_thr_sweep(scores, target, B, n, thr, K, 1 if is_logit else 0, float(target_threshold), ws, need, tp, fp, pos)
    return tp, fp, pos


def _thr_sweep_fold(tp, fp, pos, acc, n_images):
    """mi355_thr_sweep_fold: adds a batch's per-image Dice / IoU to ``acc`` (float64 [2, K]) and its size to ``n_images`` (int64 [1])."""
    B, K = tp.shape
    lib.mi355_thr_sweep_fold(tp, fp, pos, B, K, acc, n_images)


def _thr_sweep_pick(acc, n_images, k_ref):
    """mi355_thr_sweep_pick -> (float64 [4] = mean Dice, mean IoU at the pick, then at candidate k_ref; int32 [1] = the pick)."""
    out_d = torch.empty(4, dtype=torch.float64, device=acc.device)
    out_k = torch.empty(1, dtype=torch.int32, device=acc.device)
    lib.mi355_thr_sweep_pick(acc, n_images, acc.shape[1], int(k_ref), out_d, out_k)
    return out_d, out_k


class _RegionLovaszFn(torch.autograd.Function):
    """region + Lovasz hinge as ONE autograd node, for the reason documented on _RegionBoundaryFn: every mi355 criterion's backward
    returns the plan's ``dout`` buffer, so the regional backward writes ``dz`` and the Lovasz backward accumulates into it.
    ``region`` = (bce_weight, dice_weight, smooth, per_sample) or None for the Lovasz term alone; next to a regional loss a Lovasz
    weight of 0 launches nothing more than CombinedLoss does."""

    @staticmethod
    def forward(ctx, out, target, plan, region, lovasz_weight, per_image, threshold):
        if out.dim() == 4 and out.shape[1] == 1:
            B, per = out.shape[0], out.shape[2] * out.shape[3]
        elif out.dim() == 3:
            B, per = out.shape[0], out.shape[1] * out.shape[2]
        else:
            raise ValueError(f"the Lovasz hinge is defined for one-channel logits [B,1,H,W] or [B,H,W], got {tuple(out.shape)}")
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        rows_r = 0
        if region is not None:
            rows_r = lib.mi355_seg_loss_rows(B, per)
            if rows_r <= 0:
                raise RuntimeError(f"mi355_seg_loss_rows failed: {lib.raw('mi355_last_error')().decode()}")
        run_l = lovasz_weight > 0 or region is None
        # one buffer: [rows_r x 4 regional partial sums | (a_b, c_b) per sample | regional loss, loss]
        buf = torch.empty(rows_r * 4 + 2 * B + 2, dtype=torch.float32, device=out.device)
        partial, state = buf[: rows_r * 4], buf[rows_r * 4: rows_r * 4 + 2 * B]
        base, loss = buf[rows_r * 4 + 2 * B:][:1], buf[rows_r * 4 + 2 * B + 1:][:1]
        if region is not None:
            bw, dw, smooth, per_sample = region
            lib.mi355_seg_loss_fwd(o, target, B, per, bw, dw, smooth, 1 if per_sample else 0, partial, state,
                                   base if run_l else loss)
        coef = None
        if run_l:
            S, n = (B, per) if per_image else (1, B * per)
            coef = _lovasz_fwd(o, target, S, n, threshold, lovasz_weight, base if region is not None else None, loss)
        ctx.o, ctx.t, ctx.plan, ctx.state, ctx.coef = o, target, plan, state, coef
        ctx.region, ctx.run_l = region, run_l
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        n = o.numel()
        B = o.shape[0]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        if ctx.region is not None:
            lib.mi355_seg_loss_bwd(o, t, B, n // B, ctx.region[0], ctx.state, gs, dz)
        if ctx.run_l:
            lib.mi355_lovasz_bwd(ctx.coef, n, gs, 1 if ctx.region is not None else 0, dz)
        return dz[:n].view(o.shape), None, None, None, None, None, None


class LovaszHingeLoss(nn.Module):
    """weight * Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1): the convex surrogate of the Jaccard index of
    ``target > threshold``, on a deterministic segmented sort of the margins (csrc/segsort.hip, csrc/lovasz.hip).  ``per_image=True``
    evaluates it per image and averages the B terms (Berman's ``per_image``), ``per_image=False`` over the flattened batch.  Logits
    [B,1,H,W] or [B,H,W], B * H * W <= 2^26.  To add it to a regional loss use RegionLovaszLoss: the sum of two mi355 criteria is not
    a valid loss (both write their gradient into the plan's ``dout``)."""

    def __init__(self, weight=1.0, per_image=True, threshold=0.5):
        super().__init__()
        if weight < 0:
            raise ValueError(f"weight must not be negative ({weight})")
        self.weight, self.per_image, self.threshold = float(weight), bool(per_image), float(threshold)

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        return _RegionLovaszFn.apply(out, target, getattr(out, "_mi355_plan", None), None, self.weight, self.per_image, self.threshold)

    def extra_repr(self):
        return f"weight={self.weight}, per_image={self.per_image}, threshold={self.threshold}"


class RegionLovaszLoss(nn.Module):
    """CombinedLoss(bce_weight, dice_weight, smooth, per_sample) + lovasz_weight * Lovasz hinge(per_image, threshold), as one
    autograd node.  ``lovasz_weight=0`` is CombinedLoss bit for bit, with no further launch."""

    def __init__(self, bce_weight=0.5, dice_weight=0.0, lovasz_weight=0.5, smooth=1.0, per_sample=False, per_image=True, threshold=0.5):
        super().__init__()
        if bce_weight < 0 or dice_weight < 0 or lovasz_weight < 0 or smooth < 0:
            raise ValueError(f"bce_weight, dice_weight, lovasz_weight and smooth must not be negative "
                             f"({bce_weight}, {dice_weight}, {lovasz_weight}, {smooth})")
        self.bce_weight, self.dice_weight, self.lovasz_weight = float(bce_weight), float(dice_weight), float(lovasz_weight)
        self.smooth, self.per_sample, self.per_image, self.threshold = float(smooth), bool(per_sample), bool(per_image), float(threshold)

    def forward(self, out, target):
        if out.dtype != torch.float32:
            out = out.float()
        region = (self.bce_weight, self.dice_weight, self.smooth, self.per_sample)
        if self.bce_weight == 0 and self.dice_weight == 0 and self.lovasz_weight > 0:
            region = None                      # the Lovasz term alone: what LovaszHingeLoss(lovasz_weight) launches, bit for bit
        return _RegionLovaszFn.apply(out, target, getattr(out, "_mi355_plan", None), region, self.lovasz_weight, self.per_image,
                                     self.threshold)

    def extra_repr(self):
        return (f"bce_weight={self.bce_weight}, dice_weight={self.dice_weight}, lovasz_weight={self.lovasz_weight}, "
                f"smooth={self.smooth}, per_sample={self.per_sample}, per_image={self.per_image}, threshold={self.threshold}")


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


class _CEMixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, ya, yb, lam, weight, smoothing, plan):
        o = out.detach().contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=out.device)
        lib.mi355_ce_mix(o, ya, yb, lam, weight, loss, None, None, o.shape[0], o.shape[1], float(smoothing))
        ctx.o, ctx.t, ctx.plan, ctx.s = o, (ya, yb, lam, weight), plan, float(smoothing)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, plan = ctx.o, ctx.plan
        ya, yb, lam, weight = ctx.t
        n = o.numel()
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        scratch = torch.empty(1, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_ce_mix(o, ya, yb, lam, weight, scratch, dz, gs, o.shape[0], o.shape[1], ctx.s)
        return dz[:n].view(o.shape), None, None, None, None, None, None


class MixCrossEntropyLoss(nn.Module):
    """Cross-entropy against a distribution (mi355_ce_mix; mean reduction): ``target`` is an int64 label tensor [B] (hard labels) or a
    ``utils.mix.MixedTarget`` — classes ``ya`` / ``yb`` with weights ``lam`` / ``1 - lam`` per sample, what mixup and CutMix produce —
    with ``label_smoothing`` and optional per-class weights ``weight`` ([C]; kept as a float32 device buffer):

        t = (1 - s) (lam onehot(ya) + (1 - lam) onehot(yb)) + s / C,   loss = (1 / B) sum_b sum_c weight_c t_bc (-log_softmax(z_b)_c)

    = ``F.cross_entropy(z, t, weight=weight, label_smoothing=s)`` with PROBABILITY targets: the sum is divided by B.  With class-index
    targets and a weight torch divides by the sum of the picked weights instead; that normalisation is not built, so the weighted
    hard-label loss here differs from ``nn.CrossEntropyLoss(weight=w)(z, y)`` by that factor.  Without a weight the hard-label case is
    ``CrossEntropyLoss(label_smoothing=s)``, evaluated in double.  One autograd node; the gradient goes straight into the plan's
    ``dout`` when the logits come from a mi355 ``Net``.  Labels on the host are checked against [0, C); labels on the device only with
    ``check_labels=True`` (one synchronisation per call) — the kernel never indexes by a label, one outside [0, C) selects no class."""

    accepts_mixed_target = True

    def __init__(self, label_smoothing=0.0, weight=None, check_labels=False):
        super().__init__()
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1] ({label_smoothing})")
        self.label_smoothing, self.check_labels = float(label_smoothing), bool(check_labels)
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().reshape(-1).contiguous().clone()
            if weight.numel() == 0 or not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError(f"weight must hold finite values >= 0, one per class ({weight.tolist()})")
        self.register_buffer("weight", weight)

    def forward(self, out, target):
        plan = getattr(out, "_mi355_plan", None)
        out = out.float()
        if out.dim() != 2:
            raise ValueError(f"logits [B, C] expected, got {tuple(out.shape)}")
        B, C = out.shape
        if hasattr(target, "ya"):
            ya, yb, lam = target.ya, target.yb, target.lam
        else:
            ya, yb, lam = target, None, None
        labels = [ya] if yb is None else [ya, yb]
        for t in labels:
            if t.dim() != 1 or t.size(0) != B or t.dtype.is_floating_point:
                raise ValueError(f"an integer label tensor [{B}] expected, got {t.dtype} {tuple(t.shape)}")
            if (self.check_labels or not t.is_cuda) and (int(t.min()) < 0 or int(t.max()) >= C):
                raise ValueError(f"labels must lie in [0, {C}), got {t.tolist()}")
        dev = out.device
        ya = ya.to(dev, torch.int64).contiguous()
        if yb is not None:
            if lam.shape != ya.shape:
                raise ValueError(f"lam must hold one weight per sample, got {tuple(lam.shape)}")
            yb, lam = yb.to(dev, torch.int64).contiguous(), lam.to(dev, torch.float32).contiguous()
        w = self.weight
        if w is not None:
            if w.numel() != C:
                raise ValueError(f"weight holds {w.numel()} classes, the logits {C}")
            if w.device != dev:
                self.weight = w = w.to(dev)
        return _CEMixFn.apply(out, ya, yb, lam, w, self.label_smoothing, plan)

    def extra_repr(self):
        return f"label_smoothing={self.label_smoothing}, weight={None if self.weight is None else self.weight.tolist()}"


class _CEFocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, y, weight, gamma, plan):
        o = out.detach().contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=out.device)
        lib.mi355_ce_focal(o, y, weight, loss, None, None, o.shape[0], o.shape[1], float(gamma))
        ctx.o, ctx.t, ctx.plan, ctx.gamma = o, (y, weight), plan, float(gamma)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        o, plan = ctx.o, ctx.plan
        y, weight = ctx.t
        n = o.numel()
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        scratch = torch.empty(1, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_ce_focal(o, y, weight, scratch, dz, gs, o.shape[0], o.shape[1], ctx.gamma)
        return dz[:n].view(o.shape), None, None, None, None


class FocalCrossEntropyLoss(nn.Module):
    """Focal cross-entropy for classifiers (Lin et al. 2017 on a softmax; mi355_ce_focal): with p = softmax(z_b), hard labels y and
    optional per-class weights ``weight`` ([C]; kept as a float32 device buffer)

        loss = (1 / B) sum_b weight[y_b] (1 - p_b[y_b])^gamma (-log p_b[y_b])

    The sum is divided by B, as in MixCrossEntropyLoss (not by the sum of the picked weights); ``gamma`` = 0 is
    MixCrossEntropyLoss(0, weight) on hard labels.  No label smoothing and no mixed targets (the focal factor is defined for one true
    class): train() rejects it next to mixup / CutMix.  One autograd node, evaluated in double; the gradient goes straight into the
    plan's ``dout`` when the logits come from a mi355 ``Net``.  Labels on the host are checked against [0, C); labels on the device
    only with ``check_labels=True`` (one synchronisation per call) — a row whose label is outside contributes nothing."""

    def __init__(self, gamma=2.0, weight=None, check_labels=False):
        super().__init__()
        if not (gamma >= 0 and gamma != float("inf")):
            raise ValueError(f"gamma must be a finite number >= 0 ({gamma})")
        self.gamma, self.check_labels = float(gamma), bool(check_labels)
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).detach().reshape(-1).contiguous().clone()
            if weight.numel() == 0 or not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError(f"weight must hold finite values >= 0, one per class ({weight.tolist()})")
        self.register_buffer("weight", weight)

    def forward(self, out, target):
        plan = getattr(out, "_mi355_plan", None)
        out = out.float()
        if out.dim() != 2:
            raise ValueError(f"logits [B, C] expected, got {tuple(out.shape)}")
        B, C = out.shape
        if hasattr(target, "ya"):
            raise ValueError("FocalCrossEntropyLoss takes hard labels: a mixed target (mixup / CutMix) needs MixCrossEntropyLoss")
        if target.dim() != 1 or target.size(0) != B or target.dtype.is_floating_point:
            raise ValueError(f"an integer label tensor [{B}] expected, got {target.dtype} {tuple(target.shape)}")
        if (self.check_labels or not target.is_cuda) and (int(target.min()) < 0 or int(target.max()) >= C):
            raise ValueError(f"labels must lie in [0, {C}), got {target.tolist()}")
        dev = out.device
        y = target.to(dev, torch.int64).contiguous()
        w = self.weight
        if w is not None:
            if w.numel() != C:
                raise ValueError(f"weight holds {w.numel()} classes, the logits {C}")
            if w.device != dev:
                self.weight = w = w.to(dev)
        return _CEFocalFn.apply(out, y, w, self.gamma, plan)

    def extra_repr(self):
        return f"gamma={self.gamma}, weight={None if self.weight is None else self.weight.tolist()}"


# ---- knowledge distillation (csrc/distill.hip) ------------------------------------------------------------------------------------
def _check_kd(kd_weight, temperature):
    if isinstance(kd_weight, bool) or not 0.0 <= kd_weight <= 1.0:
        raise ValueError(f"kd_weight must lie in [0, 1] ({kd_weight})")
    if isinstance(temperature, bool) or not (temperature > 0 and temperature != float("inf")):
        raise ValueError(f"temperature must be a finite number > 0 ({temperature})")


def _teacher_like(out, target):
    """the teacher logits of a DistillTarget as a contiguous float32 tensor of the student's shape"""
    v = target.teacher_logits

    def core(shape):          # [N, 1, H, W] and [N, H, W] are the same map
        return tuple(shape[:1]) + tuple(shape[2:]) if len(shape) == 4 and shape[1] == 1 else tuple(shape)

    if core(v.shape) != core(out.shape):
        raise ValueError(f"teacher logits {tuple(v.shape)} must match the student's output {tuple(out.shape)}")
    if v.device != out.device:
        raise ValueError(f"teacher logits on {v.device}, the student's output on {out.device}")
    return v.detach().to(torch.float32).contiguous().view(out.shape)


class _SegDistillFn(torch.autograd.Function):
    """BCE + Dice + KD (csrc/distill.hip), the launches of _SegLossFn with the teacher's logits as a third operand: the forward leaves
    [total, hard, KD] and one coefficient pair per sample on the device, the backward is one pass that reads them with the upstream
    gradient and writes dL/dlogits."""

    @staticmethod
    def forward(ctx, out, target, teacher, plan, cfg, holder):
        if target.dtype != torch.float32 or not target.is_contiguous():
            target = target.float().contiguous()
        if target.numel() != out.numel():
            raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(out.shape)}")
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        bw, dw, smooth, per_sample, kw, temp = cfg
        B = o.shape[0]
        per = o.numel() // B
        rows = lib.mi355_kd_seg_rows(B, per)
        if rows <= 0:
            raise RuntimeError(f"mi355_kd_seg_rows failed: {lib.raw('mi355_last_error')().decode()}")
        # one buffer: [rows x 8 partial sums | (a_b, c_b) per sample | total, hard, KD]
        buf = torch.empty(rows * 8 + 2 * B + 3, dtype=torch.float32, device=out.device)
        partial, state, loss = buf[: rows * 8], buf[rows * 8: rows * 8 + 2 * B], buf[rows * 8 + 2 * B:]
        lib.mi355_kd_seg_fwd(o, target, teacher, B, per, bw, dw, smooth, 1 if per_sample else 0, kw, temp, partial, state, loss)
        ctx.o, ctx.t, ctx.v, ctx.plan, ctx.state, ctx.cfg = o, target, teacher, plan, state, cfg
        holder.last_terms = loss
        return loss[:1].view(())

    @staticmethod
    def backward(ctx, g):
        o, t, plan = ctx.o, ctx.t, ctx.plan
        bw, _, _, _, kw, temp = ctx.cfg
        n = o.numel()
        B = o.shape[0]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_kd_seg_bwd(o, t, ctx.v, B, n // B, bw, kw, temp, ctx.state, gs, dz)
        return dz[:n].view(o.shape), None, None, None, None, None


class SegDistillationLoss(nn.Module):
    """(1 - kd_weight) (bce_weight BCEWithLogits + dice_weight Dice) + kd_weight KD against a ``utils.distill.DistillTarget`` (the hard
    mask and a frozen teacher's logits v), one autograd node (mi355_kd_seg_*).  With a = z / T, b = v / T:

        KD = T^2 mean_i KL(Bernoulli(sigmoid(b_i)) || Bernoulli(sigmoid(a_i)))        Hinton et al. 2015, per pixel

    The hard terms are ``CombinedLoss``'s (the mask is used as it is).  With a plain mask tensor — the validation loop — the loss is
    the unscaled hard loss through ``CombinedLoss``'s own launches, bit for bit, so that validation losses stay comparable with an
    undistilled run.  ``last_terms``: the device tensor [total, hard, KD] of the last distilled call, as the kernel leaves it (no
    synchronisation): hard is the hard part as it enters the total, (1 - kd_weight) included, KD is unweighted,
    total = hard + kd_weight KD.  Deterministic: the same input gives the same bits."""

    accepts_mixed_target = False
    accepts_distill_target = True

    def __init__(self, bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=False, kd_weight=0.5, temperature=2.0):
        super().__init__()
        if not (bce_weight >= 0 and dice_weight >= 0 and smooth >= 0):
            raise ValueError(f"bce_weight, dice_weight and smooth must not be negative ({bce_weight}, {dice_weight}, {smooth})")
        for name, v in (("bce_weight", bce_weight), ("dice_weight", dice_weight), ("smooth", smooth)):
            if v == float("inf"):
                raise ValueError(f"{name} must be finite ({v})")
        _check_kd(kd_weight, temperature)
        self.bce_weight, self.dice_weight, self.smooth, self.per_sample = float(bce_weight), float(dice_weight), float(smooth), bool(per_sample)
        self.kd_weight, self.temperature = float(kd_weight), float(temperature)
        self.last_terms = None

    def forward(self, out, target):
        plan = getattr(out, "_mi355_plan", None)
        if out.dtype != torch.float32:
            out = out.float()
        if not hasattr(target, "teacher_logits"):
            return _SegLossFn.apply(out, target, plan, self.bce_weight, self.dice_weight, self.smooth, self.per_sample)
        v = _teacher_like(out, target)
        keep = 1.0 - self.kd_weight
        cfg = (keep * self.bce_weight, keep * self.dice_weight, self.smooth, self.per_sample, self.kd_weight, self.temperature)
        return _SegDistillFn.apply(out, target.hard, v, plan, cfg, self)

    def extra_repr(self):
        return (f"bce_weight={self.bce_weight}, dice_weight={self.dice_weight}, smooth={self.smooth}, per_sample={self.per_sample}, "
                f"kd_weight={self.kd_weight}, temperature={self.temperature}")


class _CEDistillFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, y, teacher, weight, cfg, plan, holder):
        o = out.detach().contiguous()
        smoothing, hw, kw, temp = cfg
        loss = torch.empty(3, dtype=torch.float32, device=out.device)
        lib.mi355_ce_distill(o, y, teacher, weight, loss, None, None, o.shape[0], o.shape[1], smoothing, hw, kw, temp)
        ctx.o, ctx.t, ctx.plan, ctx.cfg = o, (y, teacher, weight), plan, cfg
        holder.last_terms = loss
        return loss[:1].view(())

    @staticmethod
    def backward(ctx, g):
        o, plan = ctx.o, ctx.plan
        y, teacher, weight = ctx.t
        smoothing, hw, kw, temp = ctx.cfg
        n = o.numel()
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        scratch = torch.empty(3, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        lib.mi355_ce_distill(o, y, teacher, weight, scratch, dz, gs, o.shape[0], o.shape[1], smoothing, hw, kw, temp)
        return dz[:n].view(o.shape), None, None, None, None, None, None


class DistillCrossEntropyLoss(MixCrossEntropyLoss):
    """(1 - kd_weight) CE + kd_weight T^2 KL(softmax(v / T) || softmax(z / T)) (batch mean) against a ``utils.distill.DistillTarget`` —
    hard labels and a frozen teacher's logits v — one autograd node evaluated in double (mi355_ce_distill).  CE is
    ``MixCrossEntropyLoss(label_smoothing, weight)`` on hard labels, with its normalisation (the sum is divided by B).  With a plain
    label tensor — the validation loop — the loss is that unscaled hard loss through ``MixCrossEntropyLoss``'s own launch, bit for
    bit.  No mixed targets: train() rejects mixup / CutMix next to it.  ``last_terms``: the device tensor [total, hard, KD] of the
    last distilled call, as the kernel leaves it (no synchronisation): CE and KD unweighted, total = (1 - kd_weight) CE + kd_weight KD."""

    accepts_mixed_target = False
    accepts_distill_target = True

    def __init__(self, kd_weight=0.5, temperature=4.0, label_smoothing=0.0, weight=None, check_labels=False):
        super().__init__(label_smoothing, weight, check_labels)
        _check_kd(kd_weight, temperature)
        self.kd_weight, self.temperature = float(kd_weight), float(temperature)
        self.last_terms = None

    def forward(self, out, target):
        if hasattr(target, "ya"):
            raise ValueError("DistillCrossEntropyLoss takes hard labels: distillation on a mixed target (mixup / CutMix) is not built")
        if not hasattr(target, "teacher_logits"):
            return super().forward(out, target)
        plan = getattr(out, "_mi355_plan", None)
        out = out.float()
        if out.dim() != 2:
            raise ValueError(f"logits [B, C] expected, got {tuple(out.shape)}")
        B, C = out.shape
        y = target.hard
        if y.dim() != 1 or y.size(0) != B or y.dtype.is_floating_point:
            raise ValueError(f"an integer label tensor [{B}] expected, got {y.dtype} {tuple(y.shape)}")
        if (self.check_labels or not y.is_cuda) and (int(y.min()) < 0 or int(y.max()) >= C):
            raise ValueError(f"labels must lie in [0, {C}), got {y.tolist()}")
        v = _teacher_like(out, target)
        dev = out.device
        y = y.to(dev, torch.int64).contiguous()
        w = self.weight
        if w is not None:
            if w.numel() != C:
                raise ValueError(f"weight holds {w.numel()} classes, the logits {C}")
            if w.device != dev:
                self.weight = w = w.to(dev)
        cfg = (self.label_smoothing, 1.0 - self.kd_weight, self.kd_weight, self.temperature)
        return _CEDistillFn.apply(out, y, v, w, cfg, plan, self)

    def extra_repr(self):
        return f"kd_weight={self.kd_weight}, temperature={self.temperature}, " + super().extra_repr()


# ---- multi-class segmentation (csrc/mcseg.hip) ---------------------------------------------------------------------------------
MCSEG_ROW = 50      # MI355_MCSEG_ROW of include/mi355conv.h: doubles per partial row


def _mc_labels(target, N, HW):
    """-> contiguous uint8 [N, HW] labels from a uint8 / integer target [N, H, W] or [N, 1, H, W].  A uint8 target is used as it
    is; any other integer dtype is converted once, after a range check (one synchronisation: hand over uint8 to avoid it)."""
    if target.dtype.is_floating_point or target.dtype == torch.bool:
        raise ValueError(f"class-index labels (uint8 or an integer dtype) expected, got {target.dtype}")
    if target.numel() != N * HW or target.size(0) != N:
        raise ValueError(f"target size {tuple(target.shape)} must match the logits' [N, H, W] = {N} x {HW} pixels")
    if target.dtype != torch.uint8:
        if target.numel() and (int(target.min()) < 0 or int(target.max()) > 255):
            raise ValueError(f"labels must lie in [0, 255] (class indices and the ignore value), got [{int(target.min())}, {int(target.max())}]")
        target = target.to(torch.uint8)
    return target.contiguous().view(N, HW)


def _mc_confusion(out, labels, ignore_index=255, return_pred=False):
    """mi355_mcseg_confusion on logits [N, C, ...] and labels (see _mc_labels) -> int32 [N, C, C] (and uint8 pred [N, HW]); no sync."""
    o = out.detach()
    if o.dtype != torch.float32:
        o = o.float()
    if not o.is_contiguous():
        o = o.contiguous()
    if o.dim() < 3:
        raise ValueError(f"logits [N, C, ...] expected, got {tuple(o.shape)}")
    N, C = o.shape[:2]
    HW = o.numel() // max(N * C, 1)
    y = _mc_labels(labels.to(o.device), N, HW)
    conf = torch.empty(N, C, C, dtype=torch.int32, device=o.device)
    pred = torch.empty(N, HW, dtype=torch.uint8, device=o.device) if return_pred else None
    lib.mi355_mcseg_confusion(o, y, N, C, HW, int(ignore_index), conf, pred)
    return (conf, pred) if return_pred else conf


class _MultiClassSegFn(torch.autograd.Function):
    """Softmax cross-entropy + per-class Dice as ONE node (csrc/mcseg.hip): the forward leaves the three loss terms and the backward's
    coefficients on the device, the backward is one pass that writes dL/dlogits — into the plan's ``dout`` when there is one."""

    @staticmethod
    def forward(ctx, out, labels, plan, weight, cfg, terms):
        o = out.detach()
        if not o.is_contiguous():
            o = o.contiguous()
        N, C = o.shape[:2]
        HW = o.numel() // (N * C)
        rows = lib.mi355_mcseg_rows(N, HW)
        if rows <= 0:
            raise RuntimeError(f"mi355_mcseg_rows failed: {lib.raw('mi355_last_error')().decode()}")
        # one fp64 buffer: [rows x MCSEG_ROW partial sums | state 2 + 2 N C]
        buf = torch.empty(rows * MCSEG_ROW + 2 + 2 * N * C, dtype=torch.float64, device=o.device)
        partial, state = buf[: rows * MCSEG_ROW], buf[rows * MCSEG_ROW:]
        loss = torch.empty(3, dtype=torch.float32, device=o.device)
        ce_w, dice_w, smooth, per_sample, include_bg, ignore = cfg
        lib.mi355_mcseg_loss_fwd(o, labels, N, C, HW, weight, ignore, ce_w, dice_w, smooth, 1 if per_sample else 0,
                                 1 if include_bg else 0, partial, state, loss)
        ctx.o, ctx.y, ctx.plan, ctx.w, ctx.state, ctx.cfg = o, labels, plan, weight, state, cfg
        terms[:] = [loss[1], loss[2]]             # device views for logging (MultiClassSegLoss.last_terms); not part of the graph
        return loss[:1].view(())

    @staticmethod
    def backward(ctx, g):
        o, plan = ctx.o, ctx.plan
        n = o.numel()
        N, C = o.shape[:2]
        dz = plan.dout if (plan is not None and plan.dout is not None and plan.dout.numel() >= n) else \
            torch.empty(n, dtype=torch.float32, device=o.device)
        gs = g.detach().float().reshape(1).contiguous()
        ce_w, dice_w, _, _, _, ignore = ctx.cfg
        lib.mi355_mcseg_loss_bwd(o, ctx.y, N, C, n // (N * C), ctx.w, ignore, ce_w, dice_w, ctx.state, gs, dz)
        return dz[:n].view(o.shape), None, None, None, None, None


class MultiClassSegLoss(nn.Module):
    """ce_weight * softmax cross-entropy + dice_weight * (1 - mean per-class soft Dice) on K-channel logits [N, K, H, W] and a
    class-index target (uint8 [N, H, W] or [N, 1, H, W]; another integer dtype is range-checked and converted once), on the HIP
    library.  The cross-entropy is ``F.cross_entropy(out, target, class_weight, ignore_index)`` with its weighted-mean normalisation,
    except that a batch without a valid pixel gives 0 (and a zero gradient) where torch gives NaN.  The Dice sums run over the batch
    (``per_sample=False``, the reference DiceLoss rule per class: a class absent from the targets stays in the mean) or per image;
    ``include_background=False`` leaves class 0 out of the Dice mean.  Every label >= K is ignored, ``ignore_index`` among them.
    One autograd node: the gradient goes straight into the plan's ``dout`` when the logits come from a mi355 ``Net``.
    ``last_terms`` = device views (cross-entropy, Dice) of the last forward, for logging without a sync.  Deterministic."""

    def __init__(self, num_classes, ce_weight=1.0, dice_weight=0.0, class_weight=None, ignore_index=255, smooth=1.0, per_sample=False,
                 include_background=True):
        super().__init__()
        num_classes = int(num_classes)
        if num_classes < 2:
            raise ValueError(f"num_classes must be >= 2 (got {num_classes}): one foreground is the binary losses' case (CombinedLoss)")
        if num_classes > 16:
            raise ValueError(f"num_classes must be <= 16 (got {num_classes})")
        if ce_weight < 0 or dice_weight < 0 or smooth < 0:
            raise ValueError(f"ce_weight, dice_weight and smooth must not be negative ({ce_weight}, {dice_weight}, {smooth})")
        ignore_index = -1 if ignore_index is None else int(ignore_index)
        if ignore_index != -1 and not num_classes <= ignore_index <= 255:
            raise ValueError(f"ignore_index must be None / -1 or lie in [{num_classes}, 255] (got {ignore_index})")
        if class_weight is not None:
            class_weight = torch.as_tensor(class_weight, dtype=torch.float32).detach().reshape(-1).contiguous().clone()
            if class_weight.numel() != num_classes or not bool(torch.isfinite(class_weight).all()) or bool((class_weight < 0).any()):
                raise ValueError(f"class_weight must hold {num_classes} finite values >= 0 ({class_weight.tolist()})")
        self.register_buffer("class_weight", class_weight)
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.ce_weight, self.dice_weight, self.smooth = float(ce_weight), float(dice_weight), float(smooth)
        self.per_sample, self.include_background = bool(per_sample), bool(include_background)
        self.last_terms = None

    def _check(self, out):
        if out.dim() < 3 or out.shape[1] != self.num_classes:
            raise ValueError(f"logits [N, {self.num_classes}, H, W] expected, got {tuple(out.shape)}")

    def forward(self, out, target):
        self._check(out)
        plan = getattr(out, "_mi355_plan", None)
        if out.dtype != torch.float32:
            out = out.float()
        N, C = out.shape[:2]
        labels = _mc_labels(target.to(out.device), N, out.numel() // (N * C))
        w = self.class_weight
        if w is not None and w.device != out.device:
            self.class_weight = w = w.to(out.device)
        cfg = (self.ce_weight, self.dice_weight, self.smooth, self.per_sample, self.include_background, self.ignore_index)
        terms = []
        loss = _MultiClassSegFn.apply(out, labels, plan, w, cfg, terms)
        self.last_terms = tuple(terms)
        return loss

    def confusion(self, out, target, return_pred=False):
        """int32 [N, K, K] device tensor, conf[n, label, prediction] over the valid pixels (mi355_mcseg_confusion); no sync."""
        self._check(out)
        return _mc_confusion(out, target, self.ignore_index, return_pred)

    def val_metric(self, out, target):
        """Mean IoU of the batch as a 0-dim device tensor (no sync): tp / (row + col - tp) from the batch-summed confusion matrix,
        averaged over the classes with a non-zero union (0 when there is none)."""
        c = self.confusion(out, target).sum(0).to(torch.float32)
        tp = torch.diagonal(c)
        union = c.sum(1) + c.sum(0) - tp
        ok = union > 0
        iou = torch.where(ok, tp / torch.where(ok, union, torch.ones_like(union)), torch.zeros_like(union))
        return iou.sum() / ok.sum().clamp(min=1).to(torch.float32)

    def extra_repr(self):
        return (f"num_classes={self.num_classes}, ce_weight={self.ce_weight}, dice_weight={self.dice_weight}, "
                f"class_weight={None if self.class_weight is None else self.class_weight.tolist()}, ignore_index={self.ignore_index}, "
                f"smooth={self.smooth}, per_sample={self.per_sample}, include_background={self.include_background}")


class MultiClassDiceLoss(MultiClassSegLoss):
    """1 - mean per-class soft Dice of softmax(logits): MultiClassSegLoss(num_classes, 0, 1) on the same kernels."""

    def __init__(self, num_classes, class_weight=None, ignore_index=255, smooth=1.0, per_sample=False, include_background=True):
        super().__init__(num_classes, 0.0, 1.0, class_weight, ignore_index, smooth, per_sample, include_background)
