"""numpy restatement of the two sliding-window kernels (csrc/sliding.hip; definitions in include/mi355conv.h) and of the host
geometry of utils/sliding.py (tile_starts, window_weights).  Imports nothing from the package.  The float32 variant evaluates in the
kernel's order — tiles in order iy, then ix — with every operation rounded on its own (numpy float32 arrays: one rounding per
ufunc), so with ``prob == 0`` the blend (+ * / min max alone) is restated bit for bit.  The sigmoid goes through the device's expf,
which is accurate to 1 ulp but not correctly rounded, so with ``prob != 0`` the blend is restated in float64 from the exact float32
logits and weights and compared within the bound derived below.  tests/test_sliding_cpu.py pins this file to facts that need no
GPU."""
import math

import numpy as np

# ---- error bounds (derived, not measured) --------------------------------------------------------------------------------------
# u = 2^-24 is the relative error of one correctly rounded fp32 operation.  The device sigmoid is 1 / (1 + expf(-v)): expf is
# documented at 1 ulp (relative 2u), which reaches the result scaled by e / (1 + e) < 1; the add and the divide are correctly rounded
# (u each).  So sigmoid' = sigmoid (1 + d), |d| <= 4u, and sigmoid <= 1 (tests/tta_ref.py derives the same figure):
U = 2.0 ** -24
SIGMOID_ERR = 4 * U                                    # 2^-22 = 2.4e-7, absolute


def blend_prob_bound(cnt):
    """|mean' - mean| for mean = (sum_i w_i s_i) / (sum_i w_i) over the cnt tiles that cover a pixel, s_i sigmoids.  The weights
    w_i = fl(wy wx) are the same float32 numbers on both sides (the restatement forms them in float32 and sums them exactly in
    float64), D = sum_i w_i.  Device: each product fl(w_i s_i') is off by w_i (SIGMOID_ERR + u) (s_i <= 1); the cnt - 1 roundings of
    the partial sums of num (each <= D) add (cnt - 1) D u, so num' = num + e, |e| <= D (SIGMOID_ERR + cnt u).  den' = D (1 + g),
    |g| <= (cnt - 1) u, from its own cnt - 1 roundings.  With mean = num / D <= 1 and u for the division:
        |mean' - mean| <= |e| / D + mean (cnt - 1) u + u <= SIGMOID_ERR + 2 cnt u,
    plus one more u that covers the second-order terms (of order cnt^2 u^2).  cnt = 16: 2.2e-6."""
    return SIGMOID_ERR + (2 * cnt + 1) * U


def blend_logit_bound(cnt, vmax):
    """the same sum for logits (no sigmoid), float32 kernel order against float64: relative to the largest |v| that enters:
    (u + (cnt - 1) u) from num, (cnt - 1) u from den, u for the division, one u for the second order -> (2 cnt + 1) u vmax"""
    return (2 * cnt + 1) * U * vmax


SPREAD_PROB_BOUND = 2 * SIGMOID_ERR + U                # hi - lo: two sigmoids and the rounding of the difference


# ---- host geometry -------------------------------------------------------------------------------------------------------------------
def tile_starts(extent, tile, overlap):
    interval = max(1, int(tile * (1 - overlap)))
    n = int(math.ceil((extent - tile) / interval)) + 1
    out = []
    for i in range(n):
        s = min(i * interval, extent - tile)
        if s not in out:
            out.append(s)
    return out


def depth_bound(extent, tile, overlap):
    """at most this many tiles cover a pixel: the starts of the tiles over pixel x lie in (x - tile, x], a half-open range of tile
    pixels that holds at most ceil(tile / interval) multiples of the interval; the last start, pulled back to extent - tile, is
    one more unless it is such a multiple itself"""
    interval = max(1, int(tile * (1 - overlap)))
    return -(-tile // interval) + (1 if (extent - tile) % interval else 0)


def coverage(extent, starts, tile):
    c = np.zeros(extent, np.int64)
    for s in starts:
        c[s:s + tile] += 1
    return c


def window_weights(tile, weighting, sigma_scale=0.125):
    if weighting == "constant":
        return np.ones(tile, np.float32)
    assert weighting == "gaussian"
    i = np.arange(tile, dtype=np.float64)
    return np.maximum(np.exp(-0.5 * ((i - (tile - 1) / 2) / (sigma_scale * tile)) ** 2), 1e-3).astype(np.float32)


# ---- kernels -----------------------------------------------------------------------------------------------------------------------
def gather_ref(src, T, ys, xs, tiles):
    """mi355_tile_gather_f32: src [N, C, H, W] -> [M, C, T, T]"""
    src = np.asarray(src, np.float32)
    Py, Px = len(ys), len(xs)
    out = np.empty((len(tiles), src.shape[1], T, T), np.float32)
    for i, t in enumerate(tiles):
        n, iy, ix = t // (Py * Px), (t // Px) % Py, t % Px
        out[i] = src[n, :, ys[iy]:ys[iy] + T, xs[ix]:xs[ix] + T]
    return out


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def blend_ref(z, N, H, W, T, ys, xs, wy, wx, prob, thr=0.5, exact=False):
    """mi355_tile_blend on z [N Py Px, T, T] (float32) -> dict.
    prob == 0: mean, spread float32 in the kernel's order (bit for bit); mask from the float64 sigmoid of that float32 mean,
    ``near_mask`` [N, H, W] bool = the decision value lies within SIGMOID_ERR of thr (the device may decide either way).
    prob != 0: the float64 sigmoids of the float32 logits, the float32 weight products, everything else in float64; ``near_mask``
    uses blend_prob_bound(cnt of the pixel).  ``exact``: prob == 0 in float64 throughout (the fp64 variant the bounds refer to).
    Also ``cover`` uint8 [H, W] and ``vmax`` (the largest |value| that enters)."""
    z = np.asarray(z, np.float32)
    Py, Px = len(ys), len(xs)
    assert z.shape == (N * Py * Px, T, T)
    wy, wx = np.asarray(wy, np.float32), np.asarray(wx, np.float32)
    acc = np.float64 if (prob or exact) else np.float32
    num, den = np.zeros((N, H, W), acc), np.zeros((H, W), acc)
    lo, hi = np.full((N, H, W), np.inf, acc), np.full((N, H, W), -np.inf, acc)
    cover = np.zeros((H, W), np.int64)
    zz = z.reshape(N, Py, Px, T, T)
    for iy in range(Py):
        for ix in range(Px):
            ry, rx = slice(ys[iy], ys[iy] + T), slice(xs[ix], xs[ix] + T)
            v = zz[:, iy, ix]
            v = sigmoid64(v) if prob else v.astype(acc)
            w = (wy[:, None] * wx[None, :]).astype(acc)                   # the float32 product, rounded once
            num[:, ry, rx] = num[:, ry, rx] + (w[None] * v)
            den[ry, rx] = den[ry, rx] + w
            lo[:, ry, rx] = np.minimum(lo[:, ry, rx], v)
            hi[:, ry, rx] = np.maximum(hi[:, ry, rx], v)
            cover[ry, rx] += 1
    assert cover.min() >= 1
    mean = num / den[None]
    spread = hi - lo
    thr = float(np.float32(thr))
    pm = mean.astype(np.float64) if prob else sigmoid64(mean)
    bound = blend_prob_bound(cover)[None] if prob else SIGMOID_ERR
    return {"mean": mean, "spread": spread, "cover": cover.astype(np.uint8), "mask": np.where(pm > thr, 255, 0).astype(np.uint8),
            "near_mask": np.abs(pm - thr) < bound, "vmax": float(np.abs(z).max())}


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def normal_maps(shape, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)
