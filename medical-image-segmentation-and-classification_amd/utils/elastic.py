"""Elastic deformation (Simard et al. 2003, the augmentation of the U-Net paper; ``A.ElasticTransform``) on the device
(csrc/elastic.hip): a uniform noise field in [-1, 1] per displacement component, smoothed by a Gaussian of ``sigma`` pixels, scaled
by ``alpha`` and added to the sampling coordinate of the affine warp, so that image and mask see one interpolation,
``out(p) = src(M (p + alpha d(p)))``.

The blur is ``scipy.ndimage.gaussian_filter(mode='reflect', truncate=4)`` as a separable correlation: the taps below ARE scipy's
kernel, the kernel on the device only correlates.  Everything stays on the device: no host round trip, no synchronisation."""
import numpy as np
import torch

from mi355.lib import lib

MAX_RADIUS = 1024                      # the cap of mi355_sepblur_reflect_f32


def gaussian_radius(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def gaussian_taps(sigma, truncate=4.0):
    """-> (taps float32 [2R + 1], R): scipy's ``_gaussian_kernel1d(sigma, 0, R)`` — ``exp(-0.5 k^2 / sigma^2)`` normalised in
    float64 — cast to fp32, with R = int(truncate * sigma + 0.5)."""
    if not sigma > 0:
        raise ValueError(f"sigma must be positive ({sigma})")
    r = gaussian_radius(sigma, truncate)
    if r > MAX_RADIUS:
        raise ValueError(f"sigma = {sigma} needs a radius of {r} taps, above the kernel's cap of {MAX_RADIUS}")
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * k ** 2)
    return (w / w.sum()).astype(np.float32), r


def check_elastic(alpha, sigma, p):
    """the (alpha, sigma, p) of the transforms' ``elastic=`` argument, validated up front"""
    if not alpha >= 0:
        raise ValueError(f"elastic: alpha must not be negative ({alpha})")
    if not sigma > 0:
        raise ValueError(f"elastic: sigma must be positive ({sigma})")
    if not 0 <= p <= 1:
        raise ValueError(f"elastic: p must lie in [0, 1] ({p})")
    r = gaussian_radius(sigma)
    if r > MAX_RADIUS:
        raise ValueError(f"elastic: sigma = {sigma} needs a radius of {r} taps, above the kernel's cap of {MAX_RADIUS}")
    return float(alpha), float(sigma), float(p)


_TAPS = {}


def _device_taps(sigma, truncate, device):
    key = (float(sigma), float(truncate), str(device))
    if key not in _TAPS:
        taps, r = gaussian_taps(sigma, truncate)
        _TAPS[key] = (torch.from_numpy(taps).to(device), r)
    return _TAPS[key]


def blur_reflect(planes, taps, radius):
    """``mi355_sepblur_reflect_f32`` on a device tensor [..., H, W] fp32 with a device tap vector of 2 radius + 1 values."""
    if not planes.is_cuda:
        raise ValueError("the blur runs on the GPU: the planes must be a device tensor (there is no CPU fallback)")
    if planes.dim() < 2 or planes.dtype != torch.float32:
        raise ValueError(f"the blur takes float32 planes [..., H, W], got {planes.dtype} {tuple(planes.shape)}")
    if taps.numel() != 2 * radius + 1 or taps.dtype != torch.float32 or taps.device != planes.device:
        raise ValueError(f"taps must be {2 * radius + 1} float32 values on {planes.device}")
    src = planes.contiguous()
    h, w = src.shape[-2:]
    tmp, dst = torch.empty_like(src), torch.empty_like(src)
    lib.mi355_sepblur_reflect_f32(src, src.numel() // (h * w), h, w, taps.contiguous(), radius, tmp, dst)
    return dst


def elastic_field(noise, sigma, truncate=4.0):
    """noise: device tensor [N, 2, H, W] float32 (dx, dy; Simard: uniform in [-1, 1]) -> the field smoothed by a Gaussian of
    ``sigma`` pixels, ``scipy.ndimage.gaussian_filter(noise[n, c], sigma, mode='reflect', truncate=truncate)`` per plane."""
    if noise.dim() != 4 or noise.shape[1] != 2:
        raise ValueError(f"noise must be [N, 2, H, W], got {tuple(noise.shape)}")
    taps, r = _device_taps(sigma, truncate, noise.device)
    return blur_reflect(noise, taps, r)


def elastic_warp(images_u8, field, alpha, mats=None, nearest=False, reflect=True):
    """``mi355_warp_field_u8``: images_u8 [N, Hs, Ws, C] (or [N, Hs, Ws]) uint8 on the device, field [N, 2, H, W] float32, alpha a
    number or [N] values, mats [N, 6] dst -> src affine maps (None: identity) -> uint8 [N, H, W, C] with
    ``out(p) = src(M (p + alpha d(p)))``, bilinear or nearest, border reflect-101 or replicate."""
    if not images_u8.is_cuda or images_u8.dtype != torch.uint8:
        raise ValueError("images must be a uint8 device tensor (there is no CPU fallback)")
    squeeze = images_u8.dim() == 3
    src = (images_u8[..., None] if squeeze else images_u8).contiguous()
    n, hs, ws, c = src.shape
    dev = src.device
    if field.dim() != 4 or field.shape[0] != n or field.shape[1] != 2 or field.dtype != torch.float32 or field.device != dev:
        raise ValueError(f"field must be float32 [{n}, 2, H, W] on {dev}, got {field.dtype} {tuple(field.shape)}")
    h, w = field.shape[2:]
    a = torch.as_tensor(alpha, dtype=torch.float32, device=dev).reshape(-1)
    a = (a.expand(n) if a.numel() == 1 else a).contiguous()
    if a.numel() != n:
        raise ValueError(f"alpha must be one number or {n} values")
    m = torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] * n, device=dev) if mats is None else \
        torch.as_tensor(mats, dtype=torch.float32, device=dev).reshape(n, 6).contiguous()
    out = torch.empty(n, h, w, c, dtype=torch.uint8, device=dev)
    lib.mi355_warp_field_u8(src, n, hs, ws, c, m, field.contiguous(), a, out, h, w, int(bool(nearest)), int(bool(reflect)))
    return out[..., 0] if squeeze else out
