"""The yardstick of the connected-component clean-up (csrc/components.hip, utils/postprocess.py): numpy and plain Python only, exact.

Definition, per sample, for a binary H x W mask m (``binarise`` of the probabilities or logits):

* fill_holes in {0, 4, 8} (0 = off): the background components under that connectivity that do not touch the image frame become
  foreground (= ``scipy.ndimage.binary_fill_holes(m, generate_binary_structure(2, 1 or 2))``, tests/test_components_cpu.py);
* the components of the filled mask under ``connectivity`` in {4, 8}; ``first`` of a component is the smallest linear index y W + x
  among its pixels; components are numbered 1..n by increasing ``first`` (= ``scipy.ndimage.label``), 0 is background;
* rank = position in the order (area descending, first ascending); a component is kept iff area >= min_area and
  (keep_largest == 0 or rank < keep_largest);
* mask = 255 on kept components; out_i = [foreground after thresholding, pixels added by the fill, components, kept components,
  foreground of mask, largest area of any component, rows reported = min(kept, max_report), status = 0];
  out_c [max_report, 8] = the kept components in rank order, each [area, first, y0, x0, y1, x1, sum_y, sum_x], unused rows zero.

``analyse`` is the part that does not depend on the filter (one pass of plain union-find over the pixels), ``finish`` the filter on top
of it, ``run`` both for a batch.  Run as a script it writes tests/golden/components.npz."""
import os

import numpy as np


def binarise(v, is_logit=False, threshold=0.5):
    v = np.asarray(v, dtype=np.float64)
    if is_logit:
        v = 1.0 / (1.0 + np.exp(-v))
    return v > threshold


def roots(m, connectivity=8):
    """int64 [H, W]: the smallest linear index of the component of every set pixel, -1 on the background."""
    assert connectivity in (4, 8)
    m = np.asarray(m, dtype=bool)
    H, W = m.shape
    flat = m.ravel().tolist()
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])      # the neighbours already visited
    fg = np.flatnonzero(m).tolist()
    for i in fg:
        y, x = divmod(i, W)
        for dy, dx in back:
            yy, xx = y + dy, x + dx
            if yy >= 0 and 0 <= xx < W and flat[yy * W + xx]:
                a, b = find(i), find(yy * W + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)      # the smaller index stays the root
    out = np.full(H * W, -1, dtype=np.int64)
    for i in fg:
        out[i] = find(i)
    return out.reshape(H, W)


def label(m, connectivity=8):
    """-> (labels int32 [H, W], first int64 [n])"""
    r = roots(m, connectivity)
    first = np.unique(r[r >= 0])
    lab = np.zeros(r.shape, dtype=np.int32)
    lab[r >= 0] = np.searchsorted(first, r[r >= 0]) + 1
    return lab, first


def fill_holes(m, structure):
    """structure 4 / 8: the connectivity of the BACKGROUND whose frame-less components are filled"""
    m = np.asarray(m, dtype=bool)
    r = roots(~m, structure)
    frame = np.concatenate([r[0], r[-1], r[:, 0], r[:, -1]])
    return m | ((r >= 0) & ~np.isin(r, frame[frame >= 0]))


def analyse(m, connectivity=8, fill=0):
    """-> dict: mask0, filled (bool), labels (int32), table int64 [n, 8] in label order"""
    m = np.asarray(m, dtype=bool)
    f = fill_holes(m, fill) if fill else m.copy()
    lab, first = label(f, connectivity)
    n = len(first)
    ys, xs = np.nonzero(f)
    k = lab[ys, xs] - 1
    t = np.zeros((n, 8), dtype=np.int64)
    t[:, 0] = np.bincount(k, minlength=n)
    t[:, 1] = first
    t[:, 2], t[:, 3] = m.shape
    t[:, 4:6] = -1
    np.minimum.at(t[:, 2], k, ys)
    np.minimum.at(t[:, 3], k, xs)
    np.maximum.at(t[:, 4], k, ys)
    np.maximum.at(t[:, 5], k, xs)
    np.add.at(t[:, 6], k, ys)
    np.add.at(t[:, 7], k, xs)
    for a in (f, lab, t):
        a.setflags(write=False)
    return {"mask0": m, "filled": f, "labels": lab, "table": t}


def finish(a, min_area=0, keep_largest=0, max_report=8):
    """-> mask uint8 [H, W], out_i int32 [8], out_c int32 [max_report, 8]"""
    t, lab = a["table"], a["labels"]
    n = len(t)
    order = np.lexsort((t[:, 1], -t[:, 0]))                  # area descending, then first ascending
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    kept = (t[:, 0] >= min_area) & ((rank < keep_largest) if keep_largest else np.ones(n, dtype=bool))
    mask = np.zeros(lab.shape, dtype=np.uint8)
    mask[lab > 0] = np.where(kept[lab[lab > 0] - 1], 255, 0)
    rows = [i for i in order if kept[i]][:max_report]
    out_c = np.zeros((max_report, 8), dtype=np.int32)
    if rows:
        out_c[:len(rows)] = t[rows]
    out_i = np.array([a["mask0"].sum(), a["filled"].sum() - a["mask0"].sum(), n, kept.sum(), (mask > 0).sum(),
                      t[:, 0].max() if n else 0, len(rows), 0], dtype=np.int32)
    return mask, out_i, out_c


def run(M, connectivity=8, fill=0, min_area=0, keep_largest=0, max_report=8):
    """[B, H, W] boolean masks -> dict of stacked mask, labels, out_i, out_c"""
    res = [(a["labels"],) + finish(a, min_area, keep_largest, max_report) for a in (analyse(m, connectivity, fill) for m in M)]
    return {k: np.stack([r[j] for r in res]) for j, k in enumerate(("labels", "mask", "out_i", "out_c"))}


def centroids(out_c):
    """[..., 8] rows -> float64 [..., 2] (y, x), NaN on unused rows"""
    c = np.asarray(out_c, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c[..., :1] > 0, c[..., 6:8] / c[..., :1], np.nan)


# ---- masks ---------------------------------------------------------------------------------------------------------------
def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[:H, :W]
    return ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0


def u_and_ring(H, W, shift=0):
    """left half: a U open towards row 0 (its inside touches the frame: never filled); right half: a closed ring (filled) and, below
    it, a ring with one corner pixel missing (filled by the 4-structure only: the 8-connected background leaks through the corner)"""
    m = np.zeros((H, W), dtype=bool)
    h, w = max(H // 2, 1), max(W // 2 - 1, 1)
    s = min(shift % 2, W - 1)
    m[:h, s] = m[:h, min(w - 1 + s, W - 1)] = True
    m[h - 1, s:w + s] = True
    for y0, y1, cut in ((1, max(H // 2 - 1, 1), False), (H // 2 + 1, H - 2, True)):
        x0, x1 = W // 2 + 1, W - 2
        if y1 - y0 >= 2 and x1 - x0 >= 2:
            m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
            m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True
            if cut:
                m[y0, x0] = False
    return m


def squares(H, W, shift=0):
    """identical squares on a grid, at least one empty line between them"""
    s = max(1, min(H, W) // 6)
    m = np.zeros((H, W), dtype=bool)
    for y in range(shift % 2, H - s + 1, 2 * s + 1):
        for x in range(0, W - s + 1, 2 * s + 1):
            m[y:y + s, x:x + s] = True
    return m


def kinds(B, H, W, seed):
    """the mask kinds at one shape: {kind: bool [B, H, W]}"""
    rng = np.random.RandomState(seed)
    ell = lambda cy, cx, ry, rx: ellipse(H, W, cy * H, cx * W, max(ry * H, 0.6), max(rx * W, 0.6))
    z = lambda: np.zeros((B, H, W), dtype=bool)
    y, x = np.mgrid[:H, :W]
    out = {"noise": rng.rand(B, H, W) < 0.5}
    out["ellipses"] = np.stack([ell(0.5, 0.45 + 0.04 * b, 0.27, 0.3) | ell(0.1, 0.85, 0.05, 0.05) for b in range(B)])      # a stray blob
    out["edge"] = np.stack([ell(0.0, 0.1 * b, 0.4, 0.35) | ell(0.9, 1.0, 0.45, 0.3) for b in range(B)])
    out["all_foreground"] = ~z()
    out["all_background"] = z()
    m = z()
    for b in range(B):
        for _ in range(1 + 2 * b):
            m[b, rng.randint(H), rng.randint(W)] = True
    out["single_pixels"] = m
    out["checkerboard"] = np.stack([(y + x + b) % 2 == 0 for b in range(B)])
    m = z()
    m[:, :, ::2] = True
    m[:, :, 1::2] = np.arange(H)[None, :, None] == H - 1      # the teeth join only in the last row
    out["comb"] = m
    out["u_and_ring"] = np.stack([u_and_ring(H, W, b) for b in range(B)])
    out["diagonal"] = np.stack([(y == x) | ((y == x + 3 * b) if b else False) for b in range(B)])
    out["squares"] = np.stack([squares(H, W, b) for b in range(B)])
    return out


def noise(H, W, p, seed):
    return np.random.RandomState(seed).rand(H, W) < p


def fixture_cases():
    """(name, mask, connectivity, fill, min_area, keep_largest, max_report)"""
    c = []
    settings = ((4, 0, 0, 0, 8), (8, 4, 2, 2, 3), (8, 8, 0, 1, 16), (4, 8, 3, 5, 0), (8, 0, 0, 0, 16))
    for H, W in ((17, 13), (1, 9), (8, 1), (24, 70)):
        for k, (kind, M) in enumerate(kinds(1, H, W, 10 * H + W).items()):
            for conn, fill, mn, kl, mr in (settings[k % 5], settings[(k + H) % 5 - 1]):
                c.append((f"{kind}_{H}x{W}_c{conn}_f{fill}_a{mn}_k{kl}_r{mr}", M[0], conn, fill, mn, kl, mr))
    return c


def write_fixture(path):
    out = {"names": np.array([c[0] for c in fixture_cases()])}
    for name, m, conn, fill, mn, kl, mr in fixture_cases():
        a = analyse(m, conn, fill)
        mask, out_i, out_c = finish(a, mn, kl, mr)
        out["m__" + name] = np.packbits(m, axis=1)
        out["par__" + name] = np.array([m.shape[0], m.shape[1], conn, fill, mn, kl, mr], dtype=np.int32)
        out["mask__" + name] = np.packbits(mask > 0, axis=1)
        out["labels__" + name] = a["labels"].astype(np.int16)
        out["out_i__" + name], out["out_c__" + name] = out_i, out_c
    np.savez_compressed(path, **out)
    return out


if __name__ == "__main__":
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "components.npz")
    o = write_fixture(p)
    print(f"{p}: {len(o['names'])} cases, {os.path.getsize(p)} bytes")
