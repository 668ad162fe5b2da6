"""Signed Euclidean distance maps of binary masks on the device (csrc/boundary.hip) — what the boundary loss
(mi355.nn.BoundaryLoss / RegionBoundaryLoss) weighs the predicted probabilities with, exposed for inspection and for other uses.

The mask is ``target > threshold``.  Per sample, an outside pixel holds its distance to the nearest foreground pixel, an inside
pixel minus its distance to the nearest background pixel; a sample without foreground or without background has no boundary and
holds zeros (Kervadec's ``one_hot2dist``).  Pixels outside the image are not background.  Unit pixel spacing, H, W <= 1024.
Everything stays on the device: no host round trip, no synchronisation."""
import torch

from mi355 import nn as mnn


def _as_bhw(target):
    if target.dim() == 4 and target.shape[1] == 1:
        target = target[:, 0]
    elif target.dim() == 2:
        target = target[None]
    elif target.dim() != 3:
        raise ValueError(f"distance maps are defined for one-channel masks [B,1,H,W], [B,H,W] or [H,W], got {tuple(target.shape)}")
    if not target.is_cuda:
        raise ValueError("distance maps are computed on the GPU: the target must be a device tensor (there is no CPU fallback)")
    return target.float().contiguous()


def signed_distance2(target, threshold=0.5):
    """-> int32 [B, H, W]: the signed SQUARED distance, exact (+d^2 outside, -d^2 inside, 0 for a sample without a boundary)."""
    return mnn._signed_dist2(_as_bhw(target), threshold)


def signed_distance_map(target, threshold=0.5):
    """-> float32 [B, H, W] phi: sqrt(sd2) outside, -(sqrt(-sd2) - 1) inside, 0 where sd2 = 0 — Kervadec's
    ``distance(neg) * neg - (distance(pos) - 1) * pos``, the weights of the boundary loss.  The integers are exact and below 2^24, so phi is
    ``torch.sqrt`` of exact fp32 inputs: its only error is that square root's own rounding."""
    sd2 = signed_distance2(target, threshold)
    r = torch.sqrt(sd2.abs().float())
    return torch.where(sd2 > 0, r, torch.where(sd2 < 0, 1.0 - r, torch.zeros_like(r)))
