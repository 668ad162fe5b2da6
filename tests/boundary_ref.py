"""The yardstick of the boundary loss (csrc/boundary.hip, mi355.nn.BoundaryLoss / RegionBoundaryLoss, utils/distance.py): numpy
only, integers for the map, fp64 for the loss.

Map, per sample, for a binary H x W mask T (foreground = True):

* outside pixel:  sd2 = +min (dy^2 + dx^2) over the foreground pixels            (>= 1)
* inside pixel:   sd2 = -min (dy^2 + dx^2) over the background pixels            (<= -1)
* no foreground or no background: sd2 = 0 everywhere (no boundary; Kervadec's ``one_hot2dist`` returns zeros for an empty mask,
  and scipy's answer for an all-ones mask is an artefact that is deliberately not reproduced).  Pixels outside the image are not
  background.

= ``rint(distance_transform_edt(~T)**2) * ~T - rint(distance_transform_edt(T)**2) * T`` for a mask with both classes
(tests/test_boundary_cpu.py).  ``signed_dist2`` finds it by the exact integer two-pass min-plus (column pass, then row pass),
``signed_dist2_brute`` by forming every pair.

Loss: phi = sqrt(sd2) (sd2 > 0), -(sqrt(-sd2) - 1) (sd2 < 0), 0 (sd2 = 0) — Kervadec's distance(neg) * neg - (distance(pos) - 1) *
pos; with p = sigmoid(z), n = z.size:

    loss = weight / n * sum p phi          dloss/dz_i = weight / n * phi_i p_i (1 - p_i)

``region_boundary`` adds it to tests/seg_loss_ref.py's BCE + Dice with the schedules of RegionBoundaryLoss.  Run as a script it
writes tests/golden/boundary_loss.npz."""
import os

import numpy as np

import seg_loss_ref as S

NONE = 1 << 14              # "no such pixel in this column"; NONE^2 is above every real squared distance (<= 2 * 1023^2)
NONE2 = NONE * NONE


def _column_d2(on):
    """on: bool [H, W] -> int64 [H, W]: squared vertical distance to the nearest True pixel of the same column, NONE2 without one."""
    H, W = on.shape
    idx = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(on, idx, -NONE), axis=0)                      # nearest True row <= y
    below = np.minimum.accumulate(np.where(on, idx, 2 * NONE)[::-1], axis=0)[::-1]       # nearest True row >= y
    d = np.minimum(idx - above, below - idx)
    d = np.minimum(d, NONE)
    return d * d


def _row_pass(g2, need):
    """d2[y, x] = min_x' (x - x')^2 + g2[y, x'] at the pixels of ``need``; only the columns with a finite g2 can win."""
    H, W = g2.shape
    out = np.zeros((H, W), dtype=np.int64)
    xs_all = np.arange(W, dtype=np.int64)
    for y in range(H):
        xs = xs_all[need[y]]
        if len(xs) == 0:
            continue
        cs = xs_all[g2[y] < NONE2]
        if len(cs) == 0:
            out[y, xs] = NONE2
            continue
        d = xs[:, None] - cs[None, :]
        out[y, xs] = (d * d + g2[y, cs][None, :]).min(axis=1)
    return out


def signed_dist2_one(T):
    T = np.asarray(T, dtype=bool)
    if T.all() or not T.any():
        return np.zeros(T.shape, dtype=np.int32)
    out = _row_pass(_column_d2(T), ~T) - _row_pass(_column_d2(~T), T)
    return out.astype(np.int32)


def signed_dist2(T):
    """bool [B, H, W] (or [H, W]) -> int32 of the same shape, by the two-pass min-plus."""
    T = np.asarray(T, dtype=bool)
    if T.ndim == 2:
        return signed_dist2_one(T)
    return np.stack([signed_dist2_one(t) for t in T])


def signed_dist2_brute(T):
    """The same by forming every (pixel, pixel of the other class) pair: small masks only."""
    T = np.asarray(T, dtype=bool)
    if T.ndim == 3:
        return np.stack([signed_dist2_brute(t) for t in T])
    out = np.zeros(T.shape, dtype=np.int32)
    fg, bg = np.argwhere(T).astype(np.int64), np.argwhere(~T).astype(np.int64)
    if len(fg) == 0 or len(bg) == 0:
        return out
    for src, dst, sign in ((bg, fg, 1), (fg, bg, -1)):
        step = max(1, (1 << 22) // len(dst))
        for i in range(0, len(src), step):
            a = src[i:i + step]
            d = ((a[:, None, :] - dst[None, :, :]) ** 2).sum(axis=2).min(axis=1)
            out[a[:, 0], a[:, 1]] = sign * d
    return out


def phi(sd2):
    sd2 = np.asarray(sd2, dtype=np.float64)
    r = np.sqrt(np.abs(sd2))
    return np.where(sd2 > 0, r, np.where(sd2 < 0, -(r - 1.0), 0.0))


def boundary_loss(z, sd2, weight=1.0):
    """-> (loss: float, dloss/dz: float64 array of z's shape)."""
    z = np.asarray(z, dtype=np.float64)
    f = phi(sd2).reshape(z.shape)
    p = S.sigmoid(z)
    e = np.exp(-np.abs(z))
    q = e / (1.0 + e)
    pq = q * (1.0 - q)                                     # p (1 - p) without cancellation at saturated logits
    return float(weight * (p * f).sum() / z.size), weight * f * pq / z.size


def mean_abs_term(z, sd2, weight=1.0):
    """A = weight * mean |p phi|: the scale of the loss (a mean distance, not O(1)), for relative bounds."""
    z = np.asarray(z, dtype=np.float64)
    return float(weight * np.abs(S.sigmoid(z) * phi(sd2).reshape(z.shape)).sum() / z.size)


def schedule_weights(boundary_weight=0.01, schedule="constant", epoch=0, step=0.01, max_weight=0.99):
    """(factor of the regional loss, factor of the boundary loss)"""
    if schedule == "constant":
        return 1.0, boundary_weight
    a = min(boundary_weight + epoch * step, max_weight)
    return 1.0 - a, a


def region_boundary(z, t, bce_weight=0.5, dice_weight=0.5, boundary_weight=0.01, smooth=1.0, per_sample=False, schedule="constant",
                    epoch=0, step=0.01, max_weight=0.99, threshold=0.5, sd2=None):
    """-> (loss, dloss/dz, A): tests/seg_loss_ref.py's BCE + Dice times its factor plus the boundary term times its factor.
    ``sd2``: the map of ``t > threshold`` where the caller has formed it already (signed_dist2 of a large batch takes seconds)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(z.shape)
    r, a = schedule_weights(boundary_weight, schedule, epoch, step, max_weight)
    lr, gr = S.seg_loss(z, t, r * bce_weight, r * dice_weight, smooth, per_sample)
    if sd2 is None:
        sd2 = signed_dist2(t.reshape(z.shape[0], z.shape[-2], z.shape[-1]) > threshold)
    lb, gb = boundary_loss(z, sd2, a)
    return lr + lb, gr + gb, mean_abs_term(z, sd2, a)


# ---- masks and the fixture ---------------------------------------------------------------------------------------------------
def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def noise(H, W, p, seed):
    return np.random.RandomState(seed).rand(H, W) < p


SHAPES = [(5, 7), (17, 13), (1, 9), (8, 1), (33, 64), (65, 130)]
DENSITIES = [0.02, 0.3, 0.7, 0.98]


def fixture_cases():
    """(name, T bool [B, H, W], z float32 [B, H, W], weight): the hand-computable ones first.  Logits are multiples of 1 / 64 in
    (-8, 8): fp32 holds them exactly and they are regenerated here from the seed, so the fixture does not store them."""
    c = []

    def add(name, T, weight=1.0):
        T = np.asarray(T, dtype=bool)
        T = T[None] if T.ndim == 2 else T
        rng = np.random.RandomState(len(c) + 7)
        z = np.clip(np.rint(rng.randn(*T.shape) * 2.0 * 64.0), -511, 511) / 64.0
        c.append((name, T, z.astype(np.float32), float(weight)))
    a = np.zeros((8, 9), dtype=bool)
    a[3, 4] = True
    add("pixel_3_4", a)                                        # sd2[0, 0] = 9 + 16
    add("background_pixel_3_4", ~a)
    add("empty", np.zeros((7, 5), dtype=bool))
    add("full", np.ones((7, 5), dtype=bool))
    e = ellipse(17, 13, 8, 6, 6, 4)
    add("degenerate_and_normal", np.stack([np.zeros_like(e), e, np.ones_like(e), noise(17, 13, 0.5, 3)]), 0.3)
    add("checkerboard", (np.add.outer(np.arange(6), np.arange(11)) & 1).astype(bool))
    add("touching_the_edge", ellipse(24, 31, 3, 2, 8, 9) | ellipse(24, 31, 20, 29, 7, 6), 0.01)
    for H, W in SHAPES:
        for k, p in enumerate(DENSITIES):
            if H * W > 4000 and k not in (1, 3):               # the two big shapes: two densities each keep the file small
                continue
            if H * W > 8000 and k != 1:
                continue
            T = noise(H, W, p, 1000 * H + W + k)
            T.flat[(k * 7) % T.size] = True                    # never degenerate
            T.flat[(k * 7 + 3) % T.size] = False
            add(f"noise_{H}x{W}_p{int(round(p * 100)):02d}", T)
    return c


def write_fixture(path):
    cases = fixture_cases()
    out = {"names": np.array([n for n, *_ in cases])}
    for name, T, z, w in cases:
        sd2 = signed_dist2(T)
        loss, grad = boundary_loss(z, sd2, w)
        out["T__" + name], out["sd2__" + name] = np.packbits(T), sd2
        out["shape__" + name], out["weight__" + name] = np.array(T.shape, dtype=np.int32), np.float64(w)
        out["loss__" + name], out["grad__" + name] = np.float64(loss), grad
    np.savez_compressed(path, **out)
    return out


def load_fixture(path):
    """-> [(name, T, sd2, weight, loss, grad)]"""
    f = np.load(path)
    res = []
    for name in f["names"]:
        n = str(name)
        shape = tuple(int(v) for v in f["shape__" + n])
        T = np.unpackbits(f["T__" + n])[: int(np.prod(shape))].reshape(shape).astype(bool)
        res.append((n, T, f["sd2__" + n], float(f["weight__" + n]), float(f["loss__" + n]), f["grad__" + n]))
    return res


if __name__ == "__main__":
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundary_loss.npz")
    o = write_fixture(p)
    print(f"{p}: {len(o['names'])} cases, {os.path.getsize(p)} bytes")
