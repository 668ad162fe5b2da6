"""The yardstick of the surface-distance metrics (csrc/surface.hip, utils/tester.py): numpy only, brute force, exact.

Definition, per sample, for binary H x W masks P (prediction) and T (target):

* border(M) = the pixels of M with at least one 4-neighbour outside M, pixels outside the image counting as background
  (= ``M & ~scipy.ndimage.binary_erosion(M, generate_binary_structure(2, 1), border_value=0)``, tests/test_surface_cpu.py);
* d2_PT(p) = min over q in border(T) of |p - q|^2 for p in border(P), d2_TP likewise: integers, found here by forming every pair;
* hausdorff = sqrt(max(max d2_PT, max d2_TP));
* hd95 = the q-th percentile (q = 95) of the concatenation of both distance sets with linear interpolation: with
  n = n_P + n_T, lo = q (n - 1) div 100, r = q (n - 1) mod 100: (1 - r / 100) d[lo] + (r / 100) d[lo + (r > 0)], d ascending;
* assd = (mean d_PT + mean d_TP) / 2;
* surface_dice = (#{d2_PT <= tol2} + #{d2_TP <= tol2}) / n with tol2 = floor((tolerance / spacing)^2);
* ``spacing`` multiplies the three distances;
* both borders empty: 0, 0, 0, 1; exactly one empty: NaN four times.

``raw`` gives what mi355_surface_distances writes (out_i [B, 8], out_d [B, 2]), ``values`` the final numbers from them, ``metrics``
both from the masks.  Run as a script it writes tests/golden/surface_metrics.npz."""
import math
import os

import numpy as np

NAMES = ("hausdorff", "hd95", "assd", "surface_dice")
_CHUNK = 1 << 22            # pairs formed at a time


def binarise(v, is_logit=False, threshold=0.5):
    v = np.asarray(v, dtype=np.float64)
    if is_logit:
        v = 1.0 / (1.0 + np.exp(-v))
    return v > threshold


def border(m):
    m = np.asarray(m, dtype=bool)
    p = np.pad(m, 1)          # background all around
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def directed_d2(a, b):
    """min over the rows of b of |a_i - b_j|^2 for every row of a ([n, 2] integer coordinates) -> int64 [len(a)]."""
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    out = np.empty(len(a), dtype=np.int64)
    step = max(1, _CHUNK // max(1, len(b)))
    for i in range(0, len(a), step):
        dy = a[i:i + step, 0, None] - b[None, :, 0]
        dx = a[i:i + step, 1, None] - b[None, :, 1]
        dy *= dy
        dx *= dx
        dy += dx
        out[i:i + step] = dy.min(axis=1)
    return out


def tol2_of(tolerance, spacing=1.0):
    """d * spacing <= tolerance on integers: d2 <= floor((tolerance / spacing)^2).  The relative 1e-12 keeps a ratio such as
    0.3 / 0.1, whose square lands one rounding error under 9, on the integer it means."""
    return int(math.floor((tolerance / spacing) ** 2 * (1.0 + 1e-12)))


def raw_one(P, T, q=95, tol2=4):
    cp, ct = np.argwhere(border(P)), np.argwhere(border(T))
    out_i, out_d = np.zeros(8, dtype=np.int64), np.zeros(2, dtype=np.float64)
    out_i[0], out_i[1] = len(cp), len(ct)
    if len(cp) == 0 or len(ct) == 0:
        return out_i, out_d
    d_pt, d_tp = directed_d2(cp, ct), directed_d2(ct, cp)
    both = np.sort(np.concatenate([d_pt, d_tp]))
    pos = q * (len(both) - 1)
    lo, r = pos // 100, pos % 100
    out_i[2:] = d_pt.max(), d_tp.max(), both[lo], both[lo + (r > 0)], (d_pt <= tol2).sum(), (d_tp <= tol2).sum()
    out_d[:] = math.fsum(np.sqrt(d_pt.astype(np.float64))), math.fsum(np.sqrt(d_tp.astype(np.float64)))
    return out_i, out_d


def values_one(out_i, out_d, spacing=1.0, q=95):
    n_p, n_t, m_pt, m_tp, lo2, hi2, w_pt, w_tp = (int(v) for v in out_i)
    if n_p == 0 and n_t == 0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    if n_p == 0 or n_t == 0:
        return np.full(4, np.nan)
    n = n_p + n_t
    r = (q * (n - 1)) % 100 / 100.0
    return np.array([spacing * math.sqrt(max(m_pt, m_tp)),
                     spacing * ((1.0 - r) * math.sqrt(lo2) + r * math.sqrt(hi2)),
                     spacing * 0.5 * (float(out_d[0]) / n_p + float(out_d[1]) / n_t),
                     (w_pt + w_tp) / n])


def raw(P, T, q=95, tol2=4):
    """[B, H, W] boolean masks -> out_i int32 [B, 8], out_d float64 [B, 2]"""
    rows = [raw_one(p, t, q, tol2) for p, t in zip(P, T)]
    return np.stack([r[0] for r in rows]).astype(np.int32), np.stack([r[1] for r in rows])


def values(out_i, out_d, spacing=1.0, q=95):
    v = np.stack([values_one(i, d, spacing, q) for i, d in zip(out_i, out_d)])
    return {k: v[:, j] for j, k in enumerate(NAMES)}


def metrics(pred, target, is_logit=False, threshold=0.5, spacing=1.0, percentile=95, tolerance=2.0):
    """[B, H, W] (or [B, 1, H, W]) maps -> the four per-sample arrays plus out_i, out_d"""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 4:
        pred, target = pred[:, 0], target[:, 0]
    P, T = binarise(pred, is_logit, threshold), binarise(target, False, threshold)
    out_i, out_d = raw(P, T, percentile, tol2_of(tolerance, spacing))
    res = values(out_i, out_d, spacing, percentile)
    res["out_i"], res["out_d"] = out_i, out_d
    return res


# ---- masks ---------------------------------------------------------------------------------------------------------------
def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def noise(H, W, p, seed):
    return np.random.RandomState(seed).rand(H, W) < p


def fixture_cases():
    """(name, P, T, percentile, tolerance, spacing): a few dozen small masks, the hand-computable ones first"""
    z = lambda H, W: np.zeros((H, W), dtype=bool)
    c = []

    def add(name, P, T, q=95, tol=2.0, sp=1.0):
        c.append((name, np.asarray(P, dtype=bool), np.asarray(T, dtype=bool), q, tol, sp))
    a, b = z(8, 9), z(8, 9)
    a[1, 2], b[4, 6] = True, True
    add("pixel_3_4", a, b)                                     # 5 / 5 / 5 / 0
    add("pixel_3_4_spacing", a, b, 95, 2.6, 0.5)               # 2.5 / 2.5 / 2.5, 5 * 0.5 <= 2.6
    e = ellipse(17, 13, 8, 6, 6, 4)
    add("identical", e, e)                                     # 0 / 0 / 0 / 1
    a, b = z(16, 20), z(16, 20)
    a[3:10, 4:13], b[3:10, 6:15] = True, True
    add("rect_shift2", a, b)                                   # hausdorff 2, surface Dice 1 at tolerance 2
    add("rect_shift2_tol1", a, b, 95, 1.0)
    full = ~z(7, 5)
    add("all_foreground_both", full, full)
    a = z(7, 5)
    a[2:5, 1:4] = True
    add("all_foreground_vs_rect", full, a)
    add("both_empty", z(7, 5), z(7, 5))
    add("pred_empty", z(7, 5), a)
    add("target_empty", a, z(7, 5))
    add("single_row_all", ~z(1, 9), noise(1, 9, 0.5, 1))
    add("single_col_all", noise(8, 1, 0.5, 2), ~z(8, 1))
    for H, W in ((5, 7), (17, 13), (1, 9), (8, 1), (33, 64)):
        for k, (p, q) in enumerate(((0.3, 95), (0.5, 95), (0.7, 50))):
            P, T = noise(H, W, p, 100 * H + k), noise(H, W, p, 100 * W + 50 + k)
            if k == 0:
                P[0, 0] = T[-1, -1] = True                     # never empty
            add(f"noise_{H}x{W}_p{int(p * 10)}_q{q}", P, T, q)
    for k, q in enumerate((95, 0, 100, 37)):
        P = ellipse(48, 40, 22 + k, 18, 12 + k, 9)
        T = ellipse(48, 40, 24, 20 + k, 11, 10 + k) | ellipse(48, 40, 5, 33, 3, 3)
        add(f"ellipses_{k}_q{q}", P, T, q, 2.0 + 0.5 * k)
    P, T = ellipse(24, 31, 3, 2, 8, 9), ellipse(24, 31, 20, 29, 7, 6)
    add("touching_the_edge", P, T)
    return c


def write_fixture(path):
    out = {"names": np.array([n for n, *_ in fixture_cases()])}
    for name, P, T, q, tol, sp in fixture_cases():
        out_i, out_d = raw_one(P, T, q, tol2_of(tol, sp))
        out["P__" + name], out["T__" + name] = P.astype(np.uint8), T.astype(np.uint8)
        out["par__" + name] = np.array([q, tol, sp], dtype=np.float64)
        out["out_i__" + name], out["out_d__" + name] = out_i.astype(np.int32), out_d
        out["val__" + name] = values_one(out_i, out_d, sp, q)
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface_metrics.npz")
    o = write_fixture(p)
    print(f"{p}: {len(o['names'])} cases, {os.path.getsize(p)} bytes")
