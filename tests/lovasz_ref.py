"""fp64 numpy restatement of the Lovasz hinge (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1) as csrc/lovasz.hip evaluates it, and
of the order csrc/segsort.hip produces.  The yardstick of tests/test_lovasz_cpu.py (pinned there to a torch-fp64 autograd
transcription of the paper, tests/golden/lovasz.npz) and of the GPU tests.

The margins m = y ? z : -z are formed in the logits' own precision (exact) and THEY are sorted, ascending and stable, so a yardstick
in fp64 sees the ties the fp32 kernel sees; errors e = 1 - m, weights and sums are fp64."""
import numpy as np


def argsort_ref(keys):
    """keys [S, len] -> int32 [S, len]: np.argsort(kind="stable") per row after -0 -> +0."""
    keys = np.asarray(keys)
    k = np.where(keys == 0, np.zeros_like(keys), keys)
    return np.argsort(k, axis=-1, kind="stable").astype(np.int32)


def jaccard_weights(y_sorted):
    """The increment w_k of the Jaccard loss along the ranks, in closed form from the integers; y_sorted = the labels in rank order."""
    y = np.asarray(y_sorted, dtype=bool)
    n = y.size
    P = int(y.sum())
    c = np.cumsum(y, dtype=np.int64)
    I = P - c
    U = P + np.arange(1, n + 1, dtype=np.int64) - c
    den = np.maximum((U - 1) * U, 1).astype(np.float64)
    return np.where(y, 1.0 / U, np.where(U > 1, I / den, 1.0))


def jaccard_weights_differenced(y_sorted):
    """The same increments the way the paper's lovasz_grad forms them: J_k - J_{k-1}, J = 1 - I / U, in fp64."""
    y = np.asarray(y_sorted, dtype=np.float64)
    P = y.sum()
    inter = P - np.cumsum(y)
    union = P + np.cumsum(1.0 - y)
    J = 1.0 - inter / union
    J[1:] = J[1:] - J[:-1]
    return J


def lovasz_segment(z, t, thr=0.5):
    """One segment: z, t 1-D -> (L, dL/dz) in fp64."""
    z = np.asarray(z).reshape(-1)
    y = np.asarray(t).reshape(-1) > thr
    m = np.where(y, z, -z)                                 # the logits' dtype: exact
    order = argsort_ref(m[None])[0]
    ys = y[order]
    w = jaccard_weights(ys)
    e = 1.0 - m[order].astype(np.float64)
    active = ~(e <= 0)
    L = float(np.sum(np.where(active, e * w, 0.0)))
    g = np.zeros(z.size, dtype=np.float64)
    g[order] = np.where(active, np.where(ys, -w, w), 0.0)
    return L, g


def lovasz_ref(z, t, weight=1.0, per_image=True, thr=0.5):
    """z, t [B, ...] -> (loss, dloss/dz [same shape]) in fp64: weight * the mean over the segments (images, or the one flattened batch)."""
    z = np.asarray(z)
    t = np.asarray(t)
    B = z.shape[0]
    zs, ts = (z.reshape(B, -1), t.reshape(B, -1)) if per_image else (z.reshape(1, -1), t.reshape(1, -1))
    S = zs.shape[0]
    loss, grads = 0.0, []
    for s in range(S):
        L, g = lovasz_segment(zs[s], ts[s], thr)
        loss += L
        grads.append(g)
    return float(weight) / S * loss, (float(weight) / S * np.stack(grads)).reshape(z.shape)
