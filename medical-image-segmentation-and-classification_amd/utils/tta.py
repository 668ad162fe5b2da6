"""Test-time augmentation (nothing in the reference): predict on K mirrored / slightly rotated and rescaled views of a batch — the
perturbations the train transforms draw (``ShiftScaleRotate(0.05, 0.05, 15)``, ``HorizontalFlip``) — map the predictions back and
average them.  Besides the merged prediction this yields, per pixel, how stable the mask is under those perturbations: the variance
of the views and how many of them vote for the mask.

A view is ``(angle_deg, scale, hflip)`` about the image centre (no shift, no vertical flip: a chest film is not up-down symmetric).
``warp_views`` makes the views of a normalised fp32 NCHW batch (mi355_warp_f32), ``fold_views`` merges the views' logit maps
(mi355_tta_fold), ``TTASegmenter`` / ``TTAClassifier`` wrap a model (the classifier's merge is mi355_cls_tta_decide).  K views cost
K forward passes at the input's own batch shape, one warp launch per non-identity view and one fold launch; nothing goes back to the
host.  Definitions: include/mi355conv.h; DESIGN.md, "Test-time augmentation"."""
from __future__ import annotations

import math

import torch

from mi355.lib import lib

MAX_VIEWS = 16
IDENTITY = (0.0, 1.0, False)
_ROT = ((0.0, 1.0), (7.5, 1.05), (-7.5, 0.95))
PRESETS = {
    "hflip": [IDENTITY, (0.0, 1.0, True)],
    "rot": [IDENTITY, (7.5, 1.0, False), (-7.5, 1.0, False)],
    "full": [(a, s, f) for f in (False, True) for a, s in _ROT],
}
MERGES = ("prob", "logit")


def check_views(views):
    """A preset name or a list of (angle_deg, scale, hflip) -> list of (float, float, bool).  1 <= K <= 16, the first view is the
    identity (so every pixel has a valid view), |angle| <= 45, 0.5 <= scale <= 2; ValueError otherwise."""
    if isinstance(views, str):
        if views not in PRESETS:
            raise ValueError(f"tta: unknown preset {views!r} (one of {sorted(PRESETS)})")
        return list(PRESETS[views])
    try:
        out = [(float(a), float(s), bool(f)) for a, s, f in views]
    except (TypeError, ValueError):
        raise ValueError(f"tta: views must be a preset name or a list of (angle_deg, scale, hflip), got {views!r}") from None
    if not 1 <= len(out) <= MAX_VIEWS:
        raise ValueError(f"tta: 1 to {MAX_VIEWS} views, got {len(out)}")
    if out[0] != IDENTITY:
        raise ValueError(f"tta: the first view must be the identity (0, 1, False), got {out[0]}")
    for a, s, _ in out:
        if not (abs(a) <= 45.0 and 0.5 <= s <= 2.0):          # (also rejects NaN)
            raise ValueError(f"tta: |angle| <= 45 and 0.5 <= scale <= 2 required, got angle {a}, scale {s}")
    return out


def _similarity(h, w, angle_deg, scale):
    """2x3 of cv2.getRotationMatrix2D about (w / 2 - 0.5, h / 2 - 0.5): the convention of gpu_transforms.shift_scale_rotate_matrix"""
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    a = math.radians(angle_deg)
    al, be = scale * math.cos(a), scale * math.sin(a) + 0.0
    return [[al, be, (1 - al) * cx - be * cy], [-be + 0.0, al, be * cx + (1 - al) * cy]]


def view_matrices(views, H, W):
    """-> (d2s, s2d), float32 [K, 6] each (row-major 2x3), formed in float64 in closed form.  With M the similarity of
    shift_scale_rotate_matrix (no shift) and F the flip [[-1, 0, W - 1], [0, 1, 0]], the view is x warped by the forward map F M:
    s2d = F M takes a source pixel to its place in the view, d2s = M^-1 F takes a view pixel to the source location it shows
    (``view(p) = x(d2s p)``); M^-1 is the similarity of -angle and 1 / scale.  Identity and flip have exact integer entries."""
    d2s, s2d = [], []
    for a, s, f in check_views(views):
        m, mi = _similarity(H, W, a, s), _similarity(H, W, -a, 1.0 / s)
        if f:
            s2d.append([-m[0][0], -m[0][1], (W - 1) - m[0][2], m[1][0], m[1][1], m[1][2]])
            d2s.append([-mi[0][0], mi[0][1], mi[0][0] * (W - 1) + mi[0][2], -mi[1][0], mi[1][1], mi[1][0] * (W - 1) + mi[1][2]])
        else:
            s2d.append(m[0] + m[1])
            d2s.append(mi[0] + mi[1])
    t = lambda rows: torch.tensor(rows, dtype=torch.float64).add(0.0).to(torch.float32)       # (+ 0.0: no negative zeros)
    return t(d2s), t(s2d)


def _is_identity(view):
    return view == IDENTITY


def warp_views(x, views):
    """x: fp32 [N,C,H,W] on the GPU -> list of K tensors shaped like x.  The identity is x itself (no launch); every other view is
    one mi355_warp_f32 launch."""
    views = check_views(views)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"tta: a float32 [N,C,H,W] GPU tensor expected, got {x.dtype} {tuple(x.shape)} on {x.device}")
    x = x.contiguous()
    N, C, H, W = x.shape
    d2s = view_matrices(views, H, W)[0].to(x.device)
    out = []
    for k, v in enumerate(views):
        if _is_identity(v):
            out.append(x)
            continue
        dst = torch.empty_like(x)
        lib.mi355_warp_f32(x, N, C, H, W, d2s[k:k + 1].expand(N, 6).contiguous(), dst)
        out.append(dst)
    return out


def fold_views(z, views, merge="prob", thr=0.5, idx=None, mask_out=None):
    """z: fp32 [K,N,H,W], the logit maps of the K views -> dict of device tensors: ``mean`` fp32 [N,H,W] (of the probabilities for
    ``merge="prob"``, of the logits for ``"logit"``), ``var`` fp32 [N,H,W] (population variance of the same quantity), ``votes``
    uint8 [N,H,W] (valid views that call the pixel positive), ``valid`` uint8 [N,H,W] (views that see the pixel) and ``mask`` uint8
    0 / 255 (the decision on the mean).  ``idx`` (int32 [>= N]) and ``mask_out`` (uint8 [B,H,W]): the mask of sample n is written to
    row idx[n] of mask_out instead, the other rows are left alone."""
    views = check_views(views)
    if merge not in MERGES:
        raise ValueError(f"tta: merge must be one of {MERGES}, got {merge!r}")
    if z.dim() != 4 or z.shape[0] != len(views) or z.dtype != torch.float32 or not z.is_cuda:
        raise ValueError(f"tta: a float32 [K={len(views)},N,H,W] GPU tensor expected, got {z.dtype} {tuple(z.shape)} on {z.device}")
    if (idx is None) != (mask_out is None):
        raise ValueError("tta: idx and mask_out go together")
    z = z.contiguous()
    K, N, H, W = z.shape
    s2d = view_matrices(views, H, W)[1].to(z.device)
    mean = torch.empty(N, H, W, dtype=torch.float32, device=z.device)
    var = torch.empty_like(mean)
    votes = torch.empty(N, 2, H, W, dtype=torch.uint8, device=z.device)
    mask = torch.empty(N, H, W, dtype=torch.uint8, device=z.device) if mask_out is None else mask_out
    lib.mi355_tta_fold(z, K, N, H, W, s2d, 1 if merge == "prob" else 0, float(thr), idx, mean, var, votes, mask)
    return {"mean": mean, "var": var, "votes": votes[:, 0], "valid": votes[:, 1], "mask": mask}


def _eval_only(model):
    if model.training:
        raise ValueError("tta: the model must be in eval mode (model.eval()); its state is left as found")


def view_logits(model, x, views, rows=None):
    """K forward passes of a segmenter at x's own batch shape (no new launch plan) -> fp32 [K,rows,H,W], rows = the first ``rows``
    samples of every pass (default: all)."""
    N, _, H, W = x.shape
    rows = N if rows is None else rows
    z = torch.empty(len(views), rows, H, W, dtype=torch.float32, device=x.device)
    for k, xv in enumerate(warp_views(x, views)):
        z[k].copy_(model(xv).float().reshape(N, H, W)[:rows])
    return z


class TTASegmenter:
    """``TTASegmenter(model, views="hflip", merge="prob", thr=0.5)(x)``: x [N,3,H,W] -> fold_views' dict for the model's one-channel
    logit maps of the K views.  Runs under no_grad; the model must be in eval mode."""

    def __init__(self, model, views="hflip", merge="prob", thr=0.5):
        if merge not in MERGES:
            raise ValueError(f"tta: merge must be one of {MERGES}, got {merge!r}")
        self.model, self.views, self.merge, self.thr = model, check_views(views), merge, float(thr)

    def eval(self):
        """puts the wrapped model into eval mode (what an evaluation loop calls on the model it is given)"""
        self.model.eval()
        return self

    @torch.no_grad()
    def __call__(self, x, rows=None, idx=None, mask_out=None):
        _eval_only(self.model)
        x = x.to(dtype=torch.float32).contiguous()
        return fold_views(view_logits(self.model, x, self.views, rows), self.views, self.merge, self.thr, idx, mask_out)


class TTAClassifier:
    """``TTAClassifier(model, views)(x)``: x [B,3,H,W], B <= 1024 -> dict of device tensors: ``probs`` fp32 [B,C] (mean softmax of
    the views), ``pred`` int32 [B] (its argmax), ``confidence`` fp32 [B] (percent), ``agreement`` int32 [B] (views whose own argmax
    is ``pred``), and mi355_cls_decide's ``kept`` (int32 [B + pad]) / ``n_kept`` for ``keep_class``."""

    def __init__(self, model, views="hflip", keep_class=-1, pad=0):
        self.model, self.views, self.keep_class, self.pad = model, check_views(views), int(keep_class), int(pad)

    def eval(self):
        """puts the wrapped model into eval mode (what an evaluation loop calls on the model it is given)"""
        self.model.eval()
        return self

    @torch.no_grad()
    def __call__(self, x):
        _eval_only(self.model)
        x = x.to(dtype=torch.float32).contiguous()
        B, dev = x.shape[0], x.device
        logits = None
        for k, xv in enumerate(warp_views(x, self.views)):
            zk = self.model(xv).float()
            if logits is None:
                logits = torch.empty(len(self.views), B, zk.shape[1], dtype=torch.float32, device=dev)
            logits[k].copy_(zk)
        C = logits.shape[2]
        probs = torch.empty(B, C, dtype=torch.float32, device=dev)
        pred = torch.empty(B, dtype=torch.int32, device=dev)
        conf = torch.empty(B, dtype=torch.float32, device=dev)
        agree = torch.empty(B, dtype=torch.int32, device=dev)
        kept = torch.empty(B + self.pad, dtype=torch.int32, device=dev)
        n_kept = torch.empty(1, dtype=torch.int32, device=dev)
        lib.mi355_cls_tta_decide(logits, len(self.views), B, C, self.keep_class, probs, pred, conf, agree, kept, n_kept)
        return {"probs": probs, "pred": pred, "confidence": conf, "agreement": agree, "kept": kept, "n_kept": n_kept, "logits": logits}
