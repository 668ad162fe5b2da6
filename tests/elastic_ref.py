"""numpy restatement of the elastic deformation (csrc/elastic.hip, utils/elastic.py), the reference of tests/test_elastic_cpu.py
(which pins it to scipy.ndimage) and tests/test_gpu_elastic.py, and the maker of tests/golden/elastic.npz:

    python tests/elastic_ref.py            # rewrites the fixture

blur64         the separable correlation with scipy's mode='reflect' (np.pad 'symmetric'), along H then along W, in float64
warp_field_ref the header's coordinate formula and warp_u8's sampling, op for op in one float type (float32 = what the kernel
               evaluates; float64 = the formula itself, for the comparison with scipy.ndimage.map_coordinates)"""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "elastic.npz")


def gaussian_taps64(sigma, truncate=4.0):
    """scipy's _gaussian_kernel1d in float64 -> (taps, R)"""
    r = int(truncate * float(sigma) + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum(), r


def _correlate_axis(a, taps, r, axis):
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    e = np.pad(a, pad, mode="symmetric")           # d c b a | a b c d | d c b a, repeated where r exceeds the extent
    out = np.zeros(a.shape, dtype=np.float64)
    for k in range(2 * r + 1):                     # out[i] = sum_k taps[k] * ext[i + k - r], ascending k
        out += taps[k] * np.take(e, np.arange(k, k + n), axis=axis)
    return out


def blur64(field, taps, r):
    """field [..., H, W] -> float64, correlated with taps (2r + 1 values, taken as float64) along H, then along W"""
    taps = np.asarray(taps, dtype=np.float64)
    assert taps.shape == (2 * r + 1,)
    a = np.asarray(field, dtype=np.float64)
    return _correlate_axis(_correlate_axis(a, taps, r, a.ndim - 2), taps, r, a.ndim - 1)


def blur_bound(r, src_max):
    """|gpu - blur64| for positive taps that sum to 1: two passes of 2r + 1 fp32 accumulations each, plus the taps' rounding"""
    return 2 * (2 * r + 3) * 2.0 ** -24 * src_max


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def warp_field_ref(img, m, field, alpha, nearest=False, reflect=True, dtype=np.float32):
    """img [Hs, Ws, C] (or [Hs, Ws]) uint8, m: 6 numbers (dst -> src, row-major 2x3), field [2, H, W] (dx, dy), alpha a number
    -> uint8 [H, W, C]:  px = x + alpha dx, py = y + alpha dy, sx = m0 px + m1 py + m2, sy = m3 px + m4 py + m5, then warp_u8's
    sampling; every operation rounded to `dtype`, in the kernel's order."""
    f = dtype
    squeeze = img.ndim == 2
    src = img[..., None] if squeeze else img
    hs, ws, _ = src.shape
    _, h, w = field.shape
    m = [f(v) for v in np.asarray(m, dtype=np.float32).reshape(6)]       # the kernel reads the matrix as fp32
    a = f(np.float32(alpha))
    dx, dy = np.asarray(field[0], dtype=np.float32).astype(f), np.asarray(field[1], dtype=np.float32).astype(f)
    x = np.arange(w).astype(f)[None, :]
    y = np.arange(h).astype(f)[:, None]
    px, py = x + a * dx, y + a * dy
    sx = (m[0] * px + m[1] * py) + m[2]
    sy = (m[3] * px + m[4] * py) + m[5]
    assert px.dtype == f and sx.dtype == f and sy.dtype == f

    def at(yy, xx):
        if reflect:
            yy, xx = _reflect101(yy, hs), _reflect101(xx, ws)
        else:
            yy, xx = np.clip(yy, 0, hs - 1), np.clip(xx, 0, ws - 1)
        return src[yy, xx]                                                # [H, W, C]

    if nearest:
        out = at(np.floor(sy + f(0.5)).astype(np.int64), np.floor(sx + f(0.5)).astype(np.int64))
    else:
        fx, fy = np.floor(sx), np.floor(sy)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        ax, ay = (sx - fx)[..., None], (sy - fy)[..., None]
        one = f(1)
        top = at(y0, x0).astype(f) * (one - ax) + at(y0, x0 + 1).astype(f) * ax
        bot = at(y0 + 1, x0).astype(f) * (one - ax) + at(y0 + 1, x0 + 1).astype(f) * ax
        v = top * (one - ay) + bot * ay
        assert v.dtype == f
        out = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out[..., 0] if squeeze else out


def image(hs, ws, c, seed):
    """smooth structure plus noise, so that interpolation matters"""
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:hs, 0:ws]
    base = 127 + 90 * np.sin(xx / 3.0 + seed) * np.cos(yy / 2.5)
    return np.clip(base[..., None] + g.normal(0, 12, (hs, ws, c)), 0, 255).astype(np.uint8)


def mask(hs, ws):
    yy, xx = np.mgrid[0:hs, 0:ws]
    return (((((xx - ws * 0.5) / (ws * 0.3 + 0.5)) ** 2 + ((yy - hs * 0.45) / (hs * 0.25 + 0.5)) ** 2) < 1) * 255).astype(np.uint8)


def noise(n, h, w, seed):
    return (np.random.RandomState(seed).rand(n, 2, h, w) * 2 - 1).astype(np.float32)


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
ROT = (0.9781476, 0.20791169, -1.75, -0.20791169, 0.9781476, 2.5)       # 12 degrees and a shift

# name, (H, W) of field and output, (Hs, Ws, C) of the image, sigma (None: asymmetric taps of radius 3), alpha, m, nearest, reflect
CASES = [
    ("pixel", (1, 1), (1, 1, 1), 0.1, 3.0, IDENTITY, False, True),                # R = 0
    ("row_9", (1, 9), (1, 9, 3), 1.0, 2.0, IDENTITY, False, True),
    ("column_9", (9, 1), (9, 1, 1), 1.0, 2.0, IDENTITY, True, True),
    ("2x3", (2, 3), (2, 3, 3), 0.6, 1.5, IDENTITY, False, False),
    ("5x7_far_outside", (5, 7), (5, 7, 3), 3.0, 400.0, IDENTITY, False, True),    # R = 12 > both extents; samples extents away
    ("5x7_far_outside_clamped", (5, 7), (5, 7, 1), 3.0, 400.0, ROT, True, False),
    ("asymmetric_taps_8x8", (8, 8), (8, 8, 3), None, 4.0, IDENTITY, False, True),
    ("17x33_sigma64", (17, 33), (17, 33, 1), 64.0, 3000.0, ROT, False, True),     # R = 256
    ("3x65", (3, 65), (3, 65, 3), 2.0, 6.0, IDENTITY, False, True),
    ("65x3_mask", (65, 3), (65, 3, 1), 2.0, 6.0, IDENTITY, True, True),
    ("12x20_from_9x14", (12, 20), (9, 14, 3), 1.5, 5.0, (0.7, 0.0, -0.15, 0.0, 0.75, -0.125), False, False),
    ("29x41", (29, 41), (29, 41, 3), 4.0, 58.0, ROT, False, True),
    ("16x24_mask", (16, 24), (16, 24, 1), 2.0, 30.0, ROT, True, True),
]
ASYM_TAPS = np.array([0.05, 0.3, 0.1, 0.25, -0.1, 0.2, 0.2], dtype=np.float32)


def fixture_cases():
    """-> [(name, noise [2,H,W] f32, taps f32, R, img u8, m, alpha, nearest, reflect)], a function of nothing but this file"""
    out = []
    for i, (name, (h, w), (hs, ws, c), sigma, alpha, m, nearest, reflect) in enumerate(CASES):
        if sigma is None:
            taps, r = ASYM_TAPS, 3
        else:
            t64, r = gaussian_taps64(sigma)
            taps = t64.astype(np.float32)
        img = mask(hs, ws)[..., None] if name.endswith("_mask") else image(hs, ws, c, 40 + i)
        out.append((name, noise(1, h, w, 7 + i)[0], taps, r, img, np.asarray(m, dtype=np.float32), np.float32(alpha), nearest, reflect))
    return out


def make_case(nz, taps, r, img, m, alpha, nearest, reflect):
    """-> (field float64 = blur64 of the noise under the fp32 taps, warped uint8 under that field rounded to fp32)"""
    field = blur64(nz, taps, r)
    return field, warp_field_ref(img, m, field.astype(np.float32), alpha, nearest, reflect)


def save_fixture(path=FIXTURE):
    d = {"names": np.array([c[0] for c in fixture_cases()])}
    for name, nz, taps, r, img, m, alpha, nearest, reflect in fixture_cases():
        field, warped = make_case(nz, taps, r, img, m, alpha, nearest, reflect)
        for k, v in (("noise", nz), ("taps", taps), ("radius", np.int32(r)), ("field", field), ("image", img), ("m", m),
                     ("alpha", alpha), ("nearest", np.bool_(nearest)), ("reflect", np.bool_(reflect)), ("warped", warped)):
            d[f"{name}/{k}"] = v
    np.savez_compressed(path, **d)


def load_fixture(path=FIXTURE):
    """-> [{name, noise, taps, radius, field, image, m, alpha, nearest, reflect, warped}]"""
    z = np.load(path)
    keys = ("noise", "taps", "radius", "field", "image", "m", "alpha", "nearest", "reflect", "warped")
    return [dict({k: z[f"{n}/{k}"] for k in keys}, name=str(n)) for n in z["names"]]


if __name__ == "__main__":
    save_fixture()
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(CASES), "cases")
