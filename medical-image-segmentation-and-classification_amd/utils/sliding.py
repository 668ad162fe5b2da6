"""Sliding-window inference (nothing in the reference): keep the image at a higher resolution than the segmenter was trained at, cut
it into overlapping ``tile`` x ``tile`` windows, run every window through the model at ONE input shape (one launch plan) and blend
the one-channel logit maps where the windows overlap — MONAI's ``sliding_window_inference``, nnU-Net's Gaussian importance map.

``tile_starts`` places the windows along one axis and ``window_weights`` is the 1-D importance window (the 2-D weight is the product
of a row and a column entry).  ``gather_tiles`` cuts the windows out of a normalised fp32 NCHW batch (mi355_tile_gather_f32),
``blend_tiles`` merges the windows' logit maps (mi355_tile_blend), ``SlidingWindowSegmenter`` wraps a model.  N images of P windows
cost ceil(N P / batch) forward passes of ``batch`` windows, one gather launch per pass and one blend launch; nothing goes back to
the host.  Besides the merged map the blend yields, per pixel, how far the windows that cover it disagree (``spread``) and how many
cover it (``cover``).  Definitions: include/mi355conv.h; DESIGN.md, "Sliding-window inference"."""
from __future__ import annotations

import numpy as np
import torch

from mi355.lib import lib

MAX_STARTS = 64
MAX_OVERLAP = 0.75
WEIGHTINGS = ("gaussian", "constant")
MERGES = ("prob", "logit")
MIN_WEIGHT = 1e-3


def tile_starts(extent, tile, overlap):
    """The window starts along an axis of ``extent`` pixels: a step of max(1, int(tile (1 - overlap))) from 0, the last window
    pulled back to end at the border (a pulled-back start that repeats an earlier one is dropped).  Strictly ascending, first 0,
    last extent - tile, no gap wider than the tile.  ValueError unless 0 <= overlap <= 0.75, 1 <= tile <= extent and at most 64
    starts result."""
    extent, tile, overlap = int(extent), int(tile), float(overlap)
    if not 0.0 <= overlap <= MAX_OVERLAP:                      # (also rejects NaN)
        raise ValueError(f"sliding: 0 <= overlap <= {MAX_OVERLAP} required, got {overlap}")
    if not 1 <= tile <= extent:
        raise ValueError(f"sliding: 1 <= tile <= extent required (an image smaller than a tile is not padded), got tile {tile}, extent {extent}")
    interval = max(1, int(tile * (1 - overlap)))
    n = -(-(extent - tile) // interval) + 1
    if n > MAX_STARTS:
        raise ValueError(f"sliding: at most {MAX_STARTS} windows per axis, got {n} (extent {extent}, tile {tile}, overlap {overlap})")
    starts = []
    for i in range(n):
        s = min(i * interval, extent - tile)
        if not starts or s != starts[-1]:
            starts.append(s)
    return starts


def window_weights(tile, weighting, sigma_scale=0.125):
    """-> float32 [tile] numpy: ones ("constant") or max(exp(-0.5 ((i - (tile - 1) / 2) / (sigma_scale tile))^2), 1e-3)
    ("gaussian"), formed in float64 and rounded once.  All entries are > 0."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"sliding: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    tile = int(tile)
    if tile < 1:
        raise ValueError(f"sliding: tile >= 1 required, got {tile}")
    if weighting == "constant":
        return np.ones(tile, np.float32)
    if not float(sigma_scale) > 0:
        raise ValueError(f"sliding: sigma_scale > 0 required, got {sigma_scale}")
    i = np.arange(tile, dtype=np.float64)
    w = np.exp(-0.5 * ((i - (tile - 1) / 2) / (float(sigma_scale) * tile)) ** 2)
    return np.maximum(w, MIN_WEIGHT).astype(np.float32)


def check_sliding(value):
    """(tile, overlap, weighting) -> (int, float, str); ValueError otherwise"""
    try:
        tile, overlap, weighting = value
        tile, overlap = int(tile), float(overlap)
    except (TypeError, ValueError):
        raise ValueError(f"sliding must be None or (tile, overlap, weighting), got {value!r}") from None
    if tile < 1:
        raise ValueError(f"sliding: tile >= 1 required, got {tile}")
    if not 0.0 <= overlap <= MAX_OVERLAP:
        raise ValueError(f"sliding: 0 <= overlap <= {MAX_OVERLAP} required, got {overlap}")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"sliding: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    return tile, overlap, weighting


def _grid(H, W, tile, overlap):
    """-> (ys, xs): CPU int32 tensors, the launchers' host arrays"""
    return (torch.tensor(tile_starts(H, tile, overlap), dtype=torch.int32), torch.tensor(tile_starts(W, tile, overlap), dtype=torch.int32))


def _check_batch(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"sliding: {what}: a contiguous float32 [N,C,H,W] GPU tensor expected, got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', 'the host')}")


def gather_tiles(x, tile, overlap, tiles=None):
    """x: contiguous fp32 [N,C,H,W] on the GPU -> fp32 [M,C,tile,tile]: the windows listed in ``tiles`` (an int32 device tensor or a
    list of tile numbers (n Py + iy) Px + ix; default: all N Py Px in order; entries may repeat)."""
    _check_batch(x, "gather_tiles")
    N, C, H, W = x.shape
    tile = int(tile)
    ys, xs = _grid(H, W, tile, overlap)
    total = N * len(ys) * len(xs)
    if tiles is None:
        tiles = torch.arange(total, dtype=torch.int32, device=x.device)
    elif not isinstance(tiles, torch.Tensor):
        tiles = [int(t) for t in tiles]
        if any(not 0 <= t < total for t in tiles):
            raise ValueError(f"sliding: tile numbers must lie in [0, {total})")
        tiles = torch.tensor(tiles, dtype=torch.int32, device=x.device)
    if tiles.dim() != 1 or tiles.dtype != torch.int32 or tiles.device != x.device or not tiles.is_contiguous() or tiles.numel() < 1:
        raise ValueError("sliding: tiles must be a non-empty contiguous int32 vector on x's device")
    M = tiles.numel()
    dst = torch.empty(M, C, tile, tile, dtype=torch.float32, device=x.device)
    lib.mi355_tile_gather_f32(x, N, C, H, W, tile, ys, len(ys), xs, len(xs), tiles, M, dst)
    return dst


def _device_weights(tile, weighting, device):
    return torch.from_numpy(window_weights(tile, weighting)).to(device)


def blend_tiles(z, shape, tile, overlap, weighting="gaussian", merge="logit", thr=0.5, idx=None, mask_out=None, _weights=None):
    """z: contiguous fp32 [N Py Px, tile, tile] on the GPU, the logit maps of the windows of ``shape`` = (N, H, W) (or the batch's
    (N, C, H, W)) in tile order -> dict of device tensors: ``mean`` fp32 [N,H,W] (the weighted mean of the logits for
    ``merge="logit"``, of the probabilities for ``"prob"``), ``spread`` fp32 [N,H,W] (max - min of the same quantity over the
    covering windows; 0 where one window covers), ``cover`` uint8 [H,W] (how many windows cover the pixel) and ``mask`` uint8
    0 / 255 (the decision on the mean).  ``idx`` (int32 [>= N]) and ``mask_out`` (uint8 [B,H,W]): the mask of sample n is written
    to row idx[n] of mask_out instead, the other rows are left alone."""
    if merge not in MERGES:
        raise ValueError(f"sliding: merge must be one of {MERGES}, got {merge!r}")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"sliding: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"sliding: shape must be (N, H, W) or (N, C, H, W), got {shape}")
    N, H, W = shape[0], shape[-2], shape[-1]
    tile = int(tile)
    ys, xs = _grid(H, W, tile, overlap)
    total = N * len(ys) * len(xs)
    if (not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or not z.is_cuda or not z.is_contiguous()
            or tuple(z.shape) != (total, tile, tile)):
        raise ValueError(f"sliding: blend_tiles: a contiguous float32 [{total},{tile},{tile}] GPU tensor expected, got "
                         f"{getattr(z, 'dtype', type(z))} {tuple(getattr(z, 'shape', ()))} on {getattr(z, 'device', 'the host')}")
    if (idx is None) != (mask_out is None):
        raise ValueError("sliding: idx and mask_out go together")
    if mask_out is not None and (mask_out.dtype != torch.uint8 or tuple(mask_out.shape[1:]) != (H, W) or not mask_out.is_contiguous()
                                 or idx.dtype != torch.int32 or idx.numel() < N):
        raise ValueError(f"sliding: mask_out must be contiguous uint8 [B,{H},{W}] and idx int32 [>= {N}]")
    w = _device_weights(tile, weighting, z.device) if _weights is None else _weights
    mean = torch.empty(N, H, W, dtype=torch.float32, device=z.device)
    spread = torch.empty_like(mean)
    cover = torch.empty(H, W, dtype=torch.uint8, device=z.device)
    mask = torch.empty(N, H, W, dtype=torch.uint8, device=z.device) if mask_out is None else mask_out
    lib.mi355_tile_blend(z, N, H, W, tile, ys, len(ys), xs, len(xs), w, w, 1 if merge == "prob" else 0, float(thr), idx, mean, spread,
                         cover, mask)
    return {"mean": mean, "spread": spread, "cover": cover, "mask": mask}


class SlidingWindowSegmenter:
    """``SlidingWindowSegmenter(model, tile=256, overlap=0.5, weighting="gaussian", merge="logit", thr=0.5, batch=8)(x)``:
    x [N,3,H,W] with H, W >= tile -> blend_tiles' dict for the model's one-channel logit maps of the N Py Px windows.  The windows go
    through the model in chunks of exactly ``batch`` (one launch plan); the last chunk is filled up with window 0, whose extra
    outputs are dropped.  Runs under no_grad; the model must be in eval mode."""

    def __init__(self, model, tile=256, overlap=0.5, weighting="gaussian", merge="logit", thr=0.5, batch=8):
        if merge not in MERGES:
            raise ValueError(f"sliding: merge must be one of {MERGES}, got {merge!r}")
        self.tile, self.overlap, self.weighting = check_sliding((tile, overlap, weighting))
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError(f"sliding: batch >= 1 required, got {batch}")
        self.model, self.merge, self.thr = model, merge, float(thr)
        self._weights, self._lists = {}, {}

    def eval(self):
        """puts the wrapped model into eval mode (what an evaluation loop calls on the model it is given)"""
        self.model.eval()
        return self

    def grid(self, H, W):
        """-> (ys, xs): the row and column starts of the windows on an H x W image, lists of ints"""
        return tile_starts(H, self.tile, self.overlap), tile_starts(W, self.tile, self.overlap)

    def _tile_list(self, total, device):
        """the tile numbers 0 .. total - 1 filled up with 0 to whole chunks, on the device (kept per size)"""
        key = (total, str(device))
        if key not in self._lists:
            chunks = -(-total // self.batch)
            host = torch.zeros(chunks * self.batch, dtype=torch.int32)
            host[:total] = torch.arange(total, dtype=torch.int32)
            self._lists[key] = host.to(device)
        return self._lists[key]

    def _w(self, device):
        key = str(device)
        if key not in self._weights:
            self._weights[key] = _device_weights(self.tile, self.weighting, device)
        return self._weights[key]

    def _logits(self, x):
        if self.model.training:
            raise ValueError("sliding: the model must be in eval mode (model.eval()); its state is left as found")
        x = x.to(dtype=torch.float32).contiguous()
        _check_batch(x, "SlidingWindowSegmenter")
        N, C, H, W = x.shape
        T, b = self.tile, self.batch
        ys, xs = _grid(H, W, T, self.overlap)
        total = N * len(ys) * len(xs)
        tiles = self._tile_list(total, x.device)
        z = torch.empty(total, T, T, dtype=torch.float32, device=x.device)
        buf = torch.empty(b, C, T, T, dtype=torch.float32, device=x.device)
        for k in range(0, total, b):
            lib.mi355_tile_gather_f32(x, N, C, H, W, T, ys, len(ys), xs, len(xs), tiles[k:k + b], b, buf)
            m = min(b, total - k)
            z[k:k + m].copy_(self.model(buf).float().reshape(b, T, T)[:m])
        return x, z

    @torch.no_grad()
    def tile_logits(self, x):
        """-> fp32 [N Py Px, tile, tile]: the model's logit map of every window, in tile order"""
        return self._logits(x)[1]

    @torch.no_grad()
    def __call__(self, x, idx=None, mask_out=None):
        x, z = self._logits(x)
        return blend_tiles(z, tuple(x.shape), self.tile, self.overlap, self.weighting, self.merge, self.thr, idx, mask_out,
                           _weights=self._w(x.device))
