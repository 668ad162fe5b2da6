"""Connected-component clean-up of segmentation masks on the device (csrc/components.hip; DESIGN.md, "Connected components"):
hole filling, small-object removal, keep-largest-K, and the lesion statistics behind them (count, area, bounding box, centroid).
The reference overlays the thresholded mask as it is (pipeline.py:399-413); the host route this replaces is a copy plus
``scipy.ndimage.label`` / ``binary_fill_holes`` per image.  Every result is an integer and equals scipy's."""
from __future__ import annotations

import torch

from mi355.lib import lib

MAX_REPORT = 16


def label_components_batch(pred, is_logit=False, threshold=0.5, connectivity=8, fill_holes=0, min_area=0, keep_largest=0, max_report=8):
    """[B,1,H,W] / [B,H,W] probabilities (logits with ``is_logit``), H, W <= 1024 -> dict of device tensors:

    ``mask`` uint8 [B,H,W] (255 on the kept components), ``labels`` int32 [B,H,W] (1..n by increasing first pixel, as
    scipy.ndimage.label numbers them, whatever the filter keeps), ``out_i`` int32 [B,8] (foreground after thresholding, pixels added by
    the fill, components, kept, foreground of ``mask``, largest area, rows reported, status), ``out_c`` int32 [B,max_report,8] (the
    kept components by (area descending, first pixel ascending): area, first, y0, x0, y1, x1, sum_y, sum_x), and from them
    ``n_components`` / ``n_kept`` int32 [B], ``area_percent`` float64 [B] (100 * foreground of ``mask`` / (H W)) and ``centroids``
    float64 [B,max_report,2] (y, x; NaN on unused rows).  ``fill_holes``: 0, or the connectivity (4 / 8) of the background whose
    frame-less components are filled first.  A component is kept iff area >= ``min_area`` and (``keep_largest`` == 0 or it is
    among the ``keep_largest`` largest).  A dozen launches on the current stream; nothing synchronises with the host."""
    if pred.dim() == 4:
        if pred.shape[1] != 1:
            raise ValueError(f"connected components are defined for one-channel masks, got C={pred.shape[1]}")
        pred = pred[:, 0]
    if pred.dim() != 3:
        raise ValueError(f"connected components: [B,1,H,W] or [B,H,W] maps expected, got {tuple(pred.shape)}")
    if connectivity not in (4, 8):
        raise ValueError(f"connected components: connectivity must be 4 or 8, got {connectivity}")
    if fill_holes not in (0, 4, 8):
        raise ValueError(f"connected components: fill_holes must be 0, 4 or 8, got {fill_holes}")
    if not 0 <= int(max_report) <= MAX_REPORT or min_area < 0 or keep_largest < 0:
        raise ValueError(f"connected components: 0 <= max_report <= {MAX_REPORT}, min_area >= 0 and keep_largest >= 0 expected "
                         f"({max_report}, {min_area}, {keep_largest})")
    B, H, W = pred.shape
    n = lib.raw("mi355_components_ws_ints")(B, H, W)
    if n < 0:
        raise RuntimeError(f"mi355_components_ws_ints failed: {lib.raw('mi355_last_error')().decode()}")
    if not pred.is_cuda:
        pred = pred.cuda()
    dev = pred.device
    ws = torch.empty(n, dtype=torch.int32, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    out_i = torch.empty(B, 8, dtype=torch.int32, device=dev)
    out_c = torch.empty(B, int(max_report), 8, dtype=torch.int32, device=dev)
    lib.mi355_components(pred.float().contiguous(), B, H, W, 1 if is_logit else 0, float(threshold), int(connectivity), int(fill_holes),
                         int(min_area), int(keep_largest), int(max_report), ws, n, mask, labels, out_i, out_c if max_report else None)
    c = out_c.double()
    centroids = torch.where(c[..., :1] > 0, c[..., 6:8] / c[..., :1].clamp(min=1.0), torch.full_like(c[..., 6:8], float("nan")))
    return {"mask": mask, "labels": labels, "out_i": out_i, "out_c": out_c, "n_components": out_i[:, 2], "n_kept": out_i[:, 3],
            "area_percent": out_i[:, 4].double() * (100.0 / (H * W)), "centroids": centroids}


def clean_masks(pred, is_logit=False, threshold=0.5, connectivity=8, fill_holes=0, min_area=0, keep_largest=0):
    """The cleaned uint8 [B,H,W] mask (0 / 255) alone."""
    return label_components_batch(pred, is_logit, threshold, connectivity, fill_holes, min_area, keep_largest, 0)["mask"]


class MaskPostprocess:
    """The clean-up settings as a callable: ``MaskPostprocess(min_area=20)(pred)`` = ``label_components_batch(pred, ...)``."""

    def __init__(self, connectivity=8, fill_holes=0, min_area=0, keep_largest=0, max_report=8):
        if connectivity not in (4, 8):
            raise ValueError(f"connected components: connectivity must be 4 or 8, got {connectivity}")
        if fill_holes not in (0, 4, 8):
            raise ValueError(f"connected components: fill_holes must be 0, 4 or 8, got {fill_holes}")
        self.connectivity, self.fill_holes = int(connectivity), int(fill_holes)
        self.min_area, self.keep_largest, self.max_report = int(min_area), int(keep_largest), int(max_report)

    def __call__(self, pred, is_logit=False, threshold=0.5):
        return label_components_batch(pred, is_logit, threshold, self.connectivity, self.fill_holes, self.min_area, self.keep_largest,
                                      self.max_report)
