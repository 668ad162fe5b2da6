"""CLAHE (contrast-limited adaptive histogram equalisation) restated in numpy, rule by rule as include/mi355conv.h states them for
mi355_clahe_lut_u8 / mi355_clahe_apply_u8 (which restate OpenCV's clahe.cpp; cv2 is not available where these tests run, so byte
parity with cv2 itself is unchecked).  tests/test_clahe_cpu.py pins this file to facts that do not come from it (plain histogram
equalisation, hand-derived constant images, closed forms of the redistribution); tests/test_gpu_clahe.py compares the kernels with
it byte for byte.  Integer arithmetic up to the LUT's one fp32 multiply; the interpolation is float32, every operation rounded on
its own (numpy float32 arrays do exactly that)."""
import numpy as np

F = np.float32


def tile_geometry(h, w, gy, gx):
    """-> (pad_h, pad_w, th, tw): a plane that divides evenly on both sides is used as is; otherwise BOTH sides are extended, a side
    that divides evenly by a full gy / gx (OpenCV's quirk)."""
    ph = pw = 0
    if h % gy or w % gx:
        ph, pw = gy - h % gy, gx - w % gx
    if ph > h - 1 or pw > w - 1:
        raise ValueError(f"{h} x {w} under a {gy} x {gx} grid: the padding exceeds the plane")
    return ph, pw, (h + ph) // gy, (w + pw) // gx


def pad_reflect101(plane, ph, pw):
    """bottom / right extension, mirrored without repeating the edge pixel: index i >= n reads 2 (n - 1) - i"""
    h, w = plane.shape
    yi = np.arange(h + ph)
    xi = np.arange(w + pw)
    yi = np.where(yi >= h, 2 * (h - 1) - yi, yi)
    xi = np.where(xi >= w, 2 * (w - 1) - xi, xi)
    return plane[np.ix_(yi, xi)]


def clip_limit(clip, area):
    """lim of the header: 0 = no clipping"""
    return max(int(float(clip) * area / 256), 1) if clip > 0 else 0


def tile_lut(hist, lim, area):
    """256 counts (int64) -> 256 uint8"""
    h = hist.astype(np.int64).copy()
    if lim > 0:
        excess = int(np.maximum(h - lim, 0).sum())
        h = np.minimum(h, lim)
        h += excess // 256
        res = excess % 256
        if res:
            step = max(256 // res, 1)
            i = 0
            while i < 256 and res > 0:
                h[i] += 1
                i += step
                res -= 1
    scale = F(255.0) / F(area)
    return np.clip(np.rint(np.cumsum(h).astype(F) * scale), 0, 255).astype(np.uint8)


def clahe_luts_ref(plane, gy, gx, clip):
    """plane uint8 [H, W] -> (luts uint8 [gy, gx, 256], th, tw)"""
    h, w = plane.shape
    ph, pw, th, tw = tile_geometry(h, w, gy, gx)
    p = pad_reflect101(plane, ph, pw)
    area = th * tw
    lim = clip_limit(clip, area)
    luts = np.empty((gy, gx, 256), dtype=np.uint8)
    for ty in range(gy):
        for tx in range(gx):
            t = p[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = tile_lut(np.bincount(t.ravel(), minlength=256), lim, area)
    return luts, th, tw


def _axis(n, t, g):
    tf = np.arange(n, dtype=F) * (F(1.0) / F(t)) - F(0.5)
    fl = np.floor(tf)
    a = tf - fl
    a1 = F(1.0) - a
    t1 = fl.astype(np.int64)
    t2 = np.minimum(t1 + 1, g - 1)
    return np.maximum(t1, 0), t2, a, a1


def clahe_apply_ref(plane, luts, th, tw):
    """plane uint8 [H, W], luts uint8 [gy, gx, 256] (any bytes) -> uint8 [H, W]"""
    h, w = plane.shape
    gy, gx = luts.shape[:2]
    ty1, ty2, ya, ya1 = (v[:, None] for v in _axis(h, th, gy))
    tx1, tx2, xa, xa1 = (v[None, :] for v in _axis(w, tw, gx))
    lf = luts.astype(F)
    top = lf[ty1, tx1, plane] * xa1 + lf[ty1, tx2, plane] * xa
    bot = lf[ty2, tx1, plane] * xa1 + lf[ty2, tx2, plane] * xa
    res = top * ya1 + bot * ya
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe_ref(images, clip=4.0, grid=8):
    """images uint8 [N, H, W, C] or [N, H, W] -> the same shape, every channel plane equalised on its own"""
    gy, gx = (grid, grid) if isinstance(grid, int) else grid
    img = images[..., None] if images.ndim == 3 else images
    out = np.empty_like(img)
    for n in range(img.shape[0]):
        for c in range(img.shape[3]):
            plane = np.ascontiguousarray(img[n, :, :, c])
            luts, th, tw = clahe_luts_ref(plane, gy, gx, clip)
            out[n, :, :, c] = clahe_apply_ref(plane, luts, th, tw)
    return out[..., 0] if images.ndim == 3 else out


def luts_ref(images, clip, grid):
    """images uint8 [N, H, W, C] -> uint8 [N, C, gy, gx, 256]"""
    gy, gx = (grid, grid) if isinstance(grid, int) else grid
    n, _, _, c = images.shape
    return np.stack([np.stack([clahe_luts_ref(np.ascontiguousarray(images[i, :, :, j]), gy, gx, clip)[0] for j in range(c)]) for i in range(n)])


def xray_like(n, h, w, seed):
    """uint8 [n, h, w]: a smooth field of about 100 +- 30 grey levels plus a few levels of noise — a narrow band, as a chest film's
    lung fields; on such data clip = 4 does reach the limit (uniform random bytes on 32 x 32 tiles never do)."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, h)[:, None]
    x = np.linspace(0.0, 1.0, w)[None, :]
    out = np.empty((n, h, w), dtype=np.uint8)
    for i in range(n):
        fy, fx, p0, p1 = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(0, 6.28), rng.uniform(0, 6.28)
        field = 100.0 + 30.0 * np.sin(6.28 * fy * y + p0) * np.cos(6.28 * fx * x + p1)
        out[i] = np.clip(np.rint(field + rng.normal(0.0, 2.0, (h, w))), 0, 255).astype(np.uint8)
    return out


# ---- the cases tests/test_gpu_clahe.py runs and tests/test_clahe_cpu.py checks for substance -----------------------------------------
# (N, C, H, W, gy, gx, clip)
LUT_CASES = [(1, 1, 2, 2, 1, 1, 0.0), (1, 1, 16, 16, 8, 8, 4.0), (1, 1, 9, 9, 8, 8, 4.0), (2, 3, 17, 23, 4, 4, 2.0), (1, 1, 33, 64, 8, 8, 1.0),
             (1, 3, 64, 40, 1, 3, 0.5), (1, 1, 96, 80, 2, 2, 3.0), (1, 1, 8, 600, 1, 2, 2.0), (2, 3, 256, 256, 8, 8, 4.0)]
CONST_WIDTHS = (257, 258, 259, 386, 512)            # 1 x W planes, grid (1, 1), clip 0.5: residual 0, 1, 2, 129, 255


def case_input(n, c, h, w, seed=0):
    """uint8 [n, h, w, c] narrow-band data, the channels distinct"""
    planes = xray_like(n * c, h, w, 1000 * h + w + seed).reshape(n, c, h, w)
    return np.ascontiguousarray(planes.transpose(0, 2, 3, 1))


# excess = w - 1 = 256 q + res; every bin gains q = 1; the bins that gain one more, written out by hand:
#   257: res 0;  258: res 1, step 256: bin 0;  259: res 2, step 128: bins 0, 128;  386: res 129, step 1: bins 0 .. 128;
#   512: res 255, step 1: bins 0 .. 254
CONST_BUMPS = {257: [], 258: [0], 259: [0, 128], 386: list(range(129)), 512: list(range(255))}
CONST_VALUE = 77


def const_plane(w, value=CONST_VALUE):
    return np.full((1, w), value, dtype=np.uint8)


def const_lut_closed_form(w, value=CONST_VALUE):
    """the LUT of a constant 1 x w plane, grid (1, 1), clip 0.5 (lim = max(int(0.5 w / 256), 1) = 1, excess w - 1): after clipping
    bin `value` holds 1, every bin gains 1, the bins of CONST_BUMPS one more"""
    h = np.ones(256, dtype=np.int64)
    h[value] += 1
    h[CONST_BUMPS[w]] += 1
    assert h.sum() == w
    return np.clip(np.rint(np.cumsum(h).astype(F) * (F(255.0) / F(w))), 0, 255).astype(np.uint8)
