"""numpy restatement of the three test-time-augmentation kernels (csrc/tta.hip; definitions in include/mi355conv.h).  Imports nothing
from the package.  The float32 variants evaluate in the kernels' order with every operation rounded on its own (numpy float32
arrays: one rounding per ufunc), so the parts of the kernels that use only + - * / floor are restated bit for bit; the sigmoid and
the softmax go through the device's expf, which is accurate to 1 ulp but not correctly rounded, so those are restated in float64
from the exact float32 operands and compared within the bounds derived below.  tests/test_tta_cpu.py pins this file to facts that
need no GPU."""
import math

import numpy as np

IDENTITY = (0.0, 1.0, False)
PRESETS = {
    "hflip": [IDENTITY, (0.0, 1.0, True)],
    "rot": [IDENTITY, (7.5, 1.0, False), (-7.5, 1.0, False)],
    "full": [(0.0, 1.0, False), (7.5, 1.05, False), (-7.5, 0.95, False), (0.0, 1.0, True), (7.5, 1.05, True), (-7.5, 0.95, True)],
}
# "full" padded with further small angles to the cap of 16 views
VIEWS16 = PRESETS["full"] + [(a, s, f) for f in (False, True) for a, s in ((3.0, 1.0), (-3.0, 1.0), (5.0, 1.02), (-5.0, 0.98), (10.0, 1.0))]
assert len(VIEWS16) == 16

# ---- error bounds (derived, not measured) --------------------------------------------------------------------------------------
# u = 2^-24 is the relative error of one correctly rounded fp32 operation, 2u = 1 ulp.  The device sigmoid is
# 1 / (1 + expf(-v)): expf is documented at 1 ulp (relative 2u), which reaches the result scaled by e / (1 + e) < 1; the add and
# the divide are correctly rounded (u each).  So sigmoid' = sigmoid (1 + d), |d| <= 2u + u + u = 4u, and sigmoid <= 1:
U = 2.0 ** -24
SIGMOID_ERR = 4 * U                                    # 2^-22 = 2.4e-7, absolute


def mean_prob_bound(K):
    """|mean' - mean| for mean = (sum of cnt <= K sigmoids) / cnt: each term is off by SIGMOID_ERR; the cnt - 1 partial sums are at
    most cnt, so each rounding is at most cnt u; that is (cnt SIGMOID_ERR + (cnt - 1) cnt u) / cnt after the division, whose own
    rounding adds u (mean <= 1):  SIGMOID_ERR + cnt u <= SIGMOID_ERR + K u.  K = 16: 1.2e-6."""
    return SIGMOID_ERR + K * U


def var_prob_bound(K):
    """d = v - mean is off by e_d = SIGMOID_ERR + mean_prob_bound(K) + u (its rounding; |d| <= 1); d^2 by 2 |d| e_d + u <= 2 e_d + u;
    the sum of cnt of them and the division as above add cnt u:  2 e_d + (K + 1) u.  K = 16: 4.0e-6."""
    e_d = SIGMOID_ERR + mean_prob_bound(K) + U
    return 2 * e_d + (K + 1) * U


def softmax_bound(K, C):
    """probs: e_c = expf(d) is off by 2u relative (d = z - max is the same float32 on both sides); den = sum of C terms <= 1 with
    den >= 1: 2u from the terms plus (C - 1) roundings of partial sums <= C, each <= C u absolute; e / den adds u.  p <= 1, so
    |p' - p| <= (2 + 2 + (C - 1) C + 1) u, and the mean over K views adds (K + 1) u as in mean_prob_bound."""
    return (5 + (C - 1) * C) * U + (K + 1) * U


def conf_bound(K, C):
    """conf: the same terms with one more rounding (100 e) and everything scaled by 100"""
    return 100.0 * ((6 + (C - 1) * C) * U + (K + 1) * U)


# ---- matrices --------------------------------------------------------------------------------------------------------------------
def _similarity(h, w, angle_deg, scale):
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    a = math.radians(angle_deg)
    al, be = scale * math.cos(a), scale * math.sin(a)
    return [[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]]


def view_matrices(views, H, W, dtype=np.float32):
    """-> (d2s, s2d) [K, 6]: s2d = F M (source pixel -> its place in the view), d2s = M^-1 F (view pixel -> the source location it
    shows), M = cv2.getRotationMatrix2D((W / 2 - 0.5, H / 2 - 0.5), angle, scale), F = [[-1, 0, W - 1], [0, 1, 0]] when flipped; in
    closed form (M^-1 = the similarity of -angle, 1 / scale), formed in float64."""
    d2s, s2d = [], []
    for a, s, f in views:
        m, mi = _similarity(H, W, a, s), _similarity(H, W, -a, 1.0 / s)
        if f:
            s2d.append([-m[0][0], -m[0][1], (W - 1) - m[0][2], m[1][0], m[1][1], m[1][2]])
            d2s.append([-mi[0][0], mi[0][1], mi[0][0] * (W - 1) + mi[0][2], -mi[1][0], mi[1][1], mi[1][0] * (W - 1) + mi[1][2]])
        else:
            s2d.append(m[0] + m[1])
            d2s.append(mi[0] + mi[1])
    return (np.asarray(d2s, np.float64) + 0.0).astype(dtype), (np.asarray(s2d, np.float64) + 0.0).astype(dtype)


def as3x3(m6):
    return np.vstack([np.asarray(m6, np.float64).reshape(2, 3), [0.0, 0.0, 1.0]])


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    """index array -> BORDER_REFLECT_101 (d c b | a b c d | c b a), any distance"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _coords(m, H, W, dtype):
    """(m0 x + m1 y) + m2, (m3 x + m4 y) + m5 over the [H, W] grid, every operation rounded in dtype"""
    m = np.asarray(m, dtype)
    y, x = np.meshgrid(np.arange(H).astype(dtype), np.arange(W).astype(dtype), indexing="ij")
    return (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]


def _bilinear(plane, x0, x1, y0, y1, ax, ay):
    one = plane.dtype.type(1)
    top = plane[y0, x0] * (one - ax) + plane[y0, x1] * ax
    bot = plane[y1, x0] * (one - ax) + plane[y1, x1] * ax
    return top * (one - ay) + bot * ay


def warp_ref(src, m, dtype=np.float32):
    """mi355_warp_f32: src [N, C, H, W], m [N, 6] (dst -> src) -> [N, C, H, W] in dtype"""
    src = np.asarray(src, dtype)
    N, C, H, W = src.shape
    out = np.empty_like(src)
    for n in range(N):
        sx, sy = _coords(m[n], H, W, dtype)
        fx, fy = np.floor(sx), np.floor(sy)
        ax, ay = sx - fx, sy - fy
        xi, yi = fx.astype(np.int64), fy.astype(np.int64)
        x0, x1, y0, y1 = reflect101(xi, W), reflect101(xi + 1, W), reflect101(yi, H), reflect101(yi + 1, H)
        for c in range(C):
            out[n, c] = _bilinear(src[n, c], x0, x1, y0, y1, ax, ay)
    return out


def sample_views(z, s2d, dtype=np.float32):
    """the fold's sampling step: z [K, N, H, W], s2d [K, 6] -> (v [K, N, H, W] in dtype, 0 where invalid; valid bool [K, H, W])"""
    z = np.asarray(z, dtype)
    K, N, H, W = z.shape
    v = np.zeros_like(z)
    valid = np.zeros((K, H, W), bool)
    for k in range(K):
        px, py = _coords(s2d[k], H, W, dtype)
        ok = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        fx, fy = np.floor(px), np.floor(py)
        x0, y0 = np.clip(fx.astype(np.int64), 0, W - 1), np.clip(fy.astype(np.int64), 0, H - 1)      # (clipped where invalid only)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        for n in range(N):
            v[k, n] = np.where(ok, _bilinear(z[k, n], x0, x1, y0, y1, px - fx, py - fy), 0)
        valid[k] = ok
    return v, valid


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def _ordered_sum(terms, valid):
    """0 + the valid terms in order k, one rounding per addition in the terms' dtype"""
    acc = np.zeros(terms.shape[1:], terms.dtype)
    for k in range(terms.shape[0]):
        acc = np.where(valid[k][None], acc + terms[k], acc)
    return acc


def fold_ref(z, s2d, prob, thr=0.5, exact=False):
    """mi355_tta_fold on z [K, N, H, W] (float32) -> dict.
    prob == 0: mean, var float32 in the kernel's order (bit for bit); votes / mask from the float64 sigmoid of those float32 values,
    ``near_votes`` / ``near_mask`` [N, H, W] bool = some decision lies within SIGMOID_ERR of thr (the device may decide either way).
    prob != 0: the float32 sampled logits (exact), then everything in float64; ``near_*`` use SIGMOID_ERR (a view's own vote) and
    mean_prob_bound(K) (the mask).  ``exact``: sample and merge in float64 throughout (the fp64 variant)."""
    dtype = np.float64 if exact else np.float32
    K = z.shape[0]
    v, valid = sample_views(z, s2d, dtype)
    cnt = valid.sum(0)
    thr = float(np.float32(thr))
    if prob or exact:
        t = sigmoid64(v) if prob else v.astype(np.float64)
    else:
        t = v
    fcnt = cnt.astype(t.dtype)[None]
    mean = _ordered_sum(t, valid) / fcnt
    d = t - mean[None]
    var = _ordered_sum(d * d, valid) / fcnt
    p = t if prob else sigmoid64(t)                       # a view's own decision value
    pm = mean if prob else sigmoid64(mean)
    vm = valid[:, None]
    votes = ((p > thr) & vm).sum(0).astype(np.uint8)
    near_votes = ((np.abs(p - thr) < SIGMOID_ERR) & vm).any(0)
    near_mask = np.abs(pm - thr) < (mean_prob_bound(K) if prob else SIGMOID_ERR)
    return {"mean": mean, "var": var, "votes": votes, "valid": np.broadcast_to(cnt.astype(np.uint8), votes.shape).copy(),
            "mask": np.where(pm > thr, 255, 0).astype(np.uint8), "near_votes": near_votes, "near_mask": near_mask, "samples": v,
            "valid_k": valid}


# ---- classification ----------------------------------------------------------------------------------------------------------------
def cls_tta_ref(logits, keep_class):
    """mi355_cls_tta_decide on logits [K, B, C] float32 -> dict; float64 from the float32 differences z - max (exact operands)"""
    z = np.asarray(logits, np.float32)
    K, B, C = z.shape
    d = (z - z.max(2, keepdims=True)).astype(np.float64)          # float32 subtraction, as on the device
    e = np.exp(d)
    p_k = e / e.sum(2, keepdims=True)
    probs = p_k.sum(0) / K
    pred = probs.argmax(1)                                        # first maximum
    own = z.argmax(2)
    top2 = np.sort(probs, 1)[:, -2:]
    kept = np.flatnonzero(pred == keep_class)
    return {"probs": probs, "pred": pred.astype(np.int32), "conf": 100.0 * probs[np.arange(B), pred],
            "agree": (own == pred[None]).sum(0).astype(np.int32), "kept": kept.astype(np.int32), "n_kept": len(kept),
            "margin": top2[:, 1] - top2[:, 0]}


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def normal_maps(shape, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def mixed_matrices(N, H, W, which=0):
    """per-sample dst -> src matrices: the six "full" views dealt over the batch, starting at ``which``"""
    d2s = view_matrices(PRESETS["full"], H, W)[0]
    return np.stack([d2s[(which + n) % 6] for n in range(N)])
