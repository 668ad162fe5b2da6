"""CLAHE — contrast-limited adaptive histogram equalisation (``A.CLAHE`` / ``cv2.createCLAHE``), the usual preprocessing of chest
films — on the device (csrc/clahe.hip): one 256-entry look-up table per tile of a ``grid`` (histogram, clipped at ``clip`` times the
mean bin count, the excess redistributed, prefix sum), then every pixel through the bilinear blend of its four neighbouring tiles'
tables.  The rules are written out in include/mi355conv.h; they restate OpenCV's ``clahe.cpp`` (byte parity with cv2 itself has not
been checked: cv2 is not a dependency of this project).

Images with channels: every channel is equalised on its own.  For an X-ray decoded to R = G = B that is CLAHE of the grey image, and
the result stays grey.  Albumentations routes colour images through LAB and equalises L only; this module does not.

Everything stays on the device: no host round trip, no synchronisation."""
import torch

from mi355.lib import lib

MAX_GRID = 64                          # the cap of mi355_clahe_lut_u8 / mi355_clahe_apply_u8
MAX_AREA = 1 << 24


def check_clahe(clip, grid):
    """the (clip, grid) of the transforms' ``clahe=`` argument, validated up front -> (float clip, (gy, gx)); ``grid`` is one int or
    (gy, gx), each side in 1 .. 64; ``clip`` = 0 equalises without a limit."""
    if isinstance(clip, bool) or not clip >= 0 or clip == float("inf"):
        raise ValueError(f"clahe: clip must be a finite number >= 0 ({clip})")
    g = (grid, grid) if isinstance(grid, int) and not isinstance(grid, bool) else grid
    try:
        gy, gx = g
        ok = all(isinstance(v, int) and not isinstance(v, bool) and 1 <= v <= MAX_GRID for v in (gy, gx))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"clahe: grid must be an int or (gy, gx) with each side in 1 .. {MAX_GRID} ({grid!r})")
    return float(clip), (int(gy), int(gx))


def tile_geometry(h, w, gy, gx):
    """-> (th, tw) of an h x w plane: used as is when both sides divide evenly, else extended at the bottom by gy - h % gy rows and on
    the right by gx - w % gx columns (reflect-101), a side that divides evenly by a full gy / gx (OpenCV's quirk)."""
    ph = pw = 0
    if h % gy or w % gx:
        ph, pw = gy - h % gy, gx - w % gx
    if ph > h - 1 or pw > w - 1:
        raise ValueError(f"clahe: a {h} x {w} plane is too small for a {gy} x {gx} grid (padding {ph} x {pw})")
    th, tw = (h + ph) // gy, (w + pw) // gx
    if th * tw > MAX_AREA:
        raise ValueError(f"clahe: tiles of {th} x {tw} hold more than 2^24 pixels")
    return th, tw


def clip_count(clip, area):
    """the integer limit per bin the kernel takes: max(int(clip * area / 256), 1) in double; 0 = no clipping"""
    return max(int(float(clip) * area / 256), 1) if clip > 0 else 0


def _batch(images_u8):
    if not isinstance(images_u8, torch.Tensor) or not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise ValueError("clahe runs on the GPU: the images must be a uint8 device tensor (there is no CPU fallback)")
    if images_u8.dim() not in (3, 4):
        raise ValueError(f"clahe takes [N, H, W, C] or [N, H, W] images, got {tuple(images_u8.shape)}")
    src = (images_u8[..., None] if images_u8.dim() == 3 else images_u8).contiguous()
    if src.shape[3] not in (1, 3) or 0 in src.shape:
        raise ValueError(f"clahe takes non-empty images of 1 or 3 channels, got {tuple(images_u8.shape)}")
    return src


def _luts(src, clip, grid):
    n, h, w, c = src.shape
    gy, gx = grid
    th, tw = tile_geometry(h, w, gy, gx)
    luts = torch.empty(n, c, gy, gx, 256, dtype=torch.uint8, device=src.device)
    lib.mi355_clahe_lut_u8(src, n, h, w, c, gy, gx, clip_count(clip, th * tw), luts)
    return luts


def clahe_luts(images_u8, clip=4.0, grid=8):
    """``mi355_clahe_lut_u8``: images_u8 [N, H, W, C] (or [N, H, W] as C = 1) uint8 on the device -> uint8 [N, C, gy, gx, 256], the
    look-up table of every tile of every channel plane."""
    clip, grid = check_clahe(clip, grid)
    return _luts(_batch(images_u8), clip, grid)


def apply_luts(images_u8, luts):
    """``mi355_clahe_apply_u8``: the images through the bilinear blend of the tables ``luts`` [N, C, gy, gx, 256] (any bytes)."""
    src = _batch(images_u8)
    n, h, w, c = src.shape
    if luts.dim() != 5 or luts.shape[:2] != (n, c) or luts.shape[4] != 256 or luts.dtype != torch.uint8 or luts.device != src.device:
        raise ValueError(f"luts must be uint8 [{n}, {c}, gy, gx, 256] on {src.device}, got {luts.dtype} {tuple(luts.shape)}")
    gy, gx = int(luts.shape[2]), int(luts.shape[3])
    check_clahe(0.0, (gy, gx))
    tile_geometry(h, w, gy, gx)
    out = torch.empty_like(src)
    lib.mi355_clahe_apply_u8(src, n, h, w, c, gy, gx, luts.contiguous(), out)
    return out[..., 0] if images_u8.dim() == 3 else out


def clahe(images_u8, clip=4.0, grid=8):
    """images_u8 [N, H, W, C] (or [N, H, W]) uint8 on the device -> the equalised images, same shape: two launches."""
    clip, grid = check_clahe(clip, grid)
    src = _batch(images_u8)
    out = apply_luts(src, _luts(src, clip, grid))
    return out[..., 0] if images_u8.dim() == 3 else out
