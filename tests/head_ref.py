"""fp64 references, error bounds and checkers for the kernels between the last convolution and the weight update: the pooling
kernels of csrc/elementwise.hip, csrc/head.hip, csrc/loss_optim.hip and mi355_bn_fold_bias.  CPU only, plain torch / numpy.

Every reference is the exact value of the operation ON THE OPERANDS AS THE KERNEL SEES THEM: tensors rounded to their storage
type, scalars (beta1, beta2, lr, eps, wd, p, smoothing, thresholds, ...) rounded to float32 first (f32()).  Three kinds of check:

  exact     the case is built so that every intermediate is representable (dyadic data, ties on purpose): bit-equality;
  interval  one division is the only inexact step: the stored value must be one of the storage values next to the exact one;
  bounded   |y - Y| <= bound per element.  fp32 dot products use conv_bounds.bound(model "fp32") with conv_bounds.C; the AdamW,
            BCE and CE bounds are first-order propagations of the kernels' own chains (the roundings are counted in the comments
            of each *_ref), scaled by K_ADAMW / K_BCE / K_CE (the sums of the losses keep conv_bounds.C alone).  Those constants were fixed on the CPU against float32 restatements
            of the same chains (emu_* below, numpy float32), never against the kernels: tests/test_head_ref_cpu.py holds the
            restatements to HALF of each bound on the inputs the GPU cases use.

Every checker returns (worst error / bound, flat index of the worst element); a ratio above 1 fails."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_bounds as cb

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
U24 = cb.U24
TINY = 2.0 ** -126           # results below the smallest normal fp32 may be flushed to zero (v_exp_f32, 1 / (1 + inf))

# The constants of the three derived bounds.  measured = the worst error / (bound at K = 1) of the float32 restatement over every
# case of the GPU file (printed by tests/test_head_ref_cpu.py); each K leaves at least 2x over it.
K_ADAMW = 2.0                # measured: p 0.72, m 0.92, v 0.97 (two roundings of b * state, both near half an ulp)
K_BCE = 2.0                  # measured: loss 0.02, dz 0.74 (the sigmoid's sum and quotient, both near half an ulp)
K_CE = 1.0                   # measured: loss 0.04, dz 0.37
POW_U = 4.0                  # relative error of powf in units of 2^-24 (2 ulp; numpy's float32 power measured 1.69)
NORM_ULPS = 8.0              # gradient norm: about four fp32 roundings of a positive sum, 2x over that count


def f32(v):
    """a scalar as a launcher receives it through its `float` parameter"""
    return float(np.float32(v))


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * (i + 3) for i, k in enumerate(key)) % (2 ** 31))


# ---- checkers --------------------------------------------------------------------------------------------------------------------
def _ratio(err, bnd):
    r = torch.where(bnd > 0, err / bnd, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf).flatten()
    if r.numel() == 0:
        return 0.0, -1
    w = int(torch.argmax(r))
    return float(r[w]), w


def check_exact(got, ref):
    """bit-equality of values (fp64 tensors of storage values): 0 or inf, index of the first difference"""
    got, ref = got.double().flatten(), ref.double().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = ~(got == ref)                                   # NaN counts as different
    if not bool(bad.any()):
        return 0.0, -1
    return math.inf, int(torch.nonzero(bad)[0])


def check_bounded(got, ref, bnd):
    """|got - ref| <= bnd per element (bnd a tensor or a number)"""
    got, ref = got.double(), torch.as_tensor(ref, dtype=torch.float64)
    bnd = torch.as_tensor(bnd, dtype=torch.float64).expand_as(ref)
    return _ratio((got.reshape(ref.shape) - ref).abs(), bnd)


def _step(r, up):
    """the storage value next to r (a tensor of a storage type) above (up) or below it"""
    it = {2: torch.int16, 4: torch.int32}[r.element_size()]
    top = {2: 0x7FFF, 4: 0x7FFFFFFF}[r.element_size()]
    b = r.contiguous().view(it).to(torch.int64)
    mag = b & top
    o = torch.where(b < 0, -mag, mag) + torch.where(up, 1, -1)
    bits = torch.where(o < 0, (-o) | (top + 1), o)
    bits = torch.where(bits > top, bits - 2 * (top + 1), bits)          # back into the signed range of `it`
    return bits.to(it).view(r.dtype)


def storage_interval(exact, slack, dtype):
    """[largest storage value <= exact - slack, smallest storage value >= exact + slack], as fp64"""
    lo_t, hi_t = exact - slack, exact + slack
    lo, hi = lo_t.to(dtype), hi_t.to(dtype)
    lo = torch.where(lo.double() > lo_t, _step(lo, torch.zeros_like(lo_t, dtype=torch.bool)), lo)
    hi = torch.where(hi.double() < hi_t, _step(hi, torch.ones_like(hi_t, dtype=torch.bool)), hi)
    return lo.double(), hi.double()


def check_interval(got, exact, dtype, slack=0.0):
    """got must be a storage value of `dtype` next to the exact value (slack = 0: the two neighbours, or the value itself where
    it is representable).  ratio = distance from the exact value / distance of the interval's end on that side"""
    got, exact = got.double(), exact.double()
    slack = torch.as_tensor(slack, dtype=torch.float64).expand_as(exact)
    lo, hi = storage_interval(exact, slack, dtype)
    d = got.reshape(exact.shape) - exact
    return _ratio(d.abs(), torch.where(d > 0, hi - exact, exact - lo))


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def rows(t):
    """NCHW -> [N*H*W, C] (the kernels' NHWC rows)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def dyadic(gen, shape, step=0.25, lim=8):
    """multiples of `step` in [-lim * step, lim * step]: a coarse grid (ties abound), exact in bf16"""
    return torch.randint(-lim, lim + 1, shape, generator=gen).double() * step


# ---- pools -------------------------------------------------------------------------------------------------------------------------
MAXPOOL_CASES = [  # (k, s, p, H, W, kernel)
    (2, 2, 0, 5, 9, "generic"), (3, 1, 1, 6, 7, "generic"), (3, 2, 0, 7, 8, "generic"), (2, 1, 0, 4, 5, "generic"),
    (3, 2, 1, 7, 9, "3s2"), (3, 2, 1, 8, 6, "3s2"), (3, 2, 1, 1, 5, "3s2"), (2, 2, 0, 4, 6, "2x2")]
POOL_N, POOL_C = 2, 24


def maxpool_case(k, s, p, H, W):
    """x, dy, old (NCHW fp64): x on a coarse grid, gradients multiples of 0.25 in [-2, 2] (nine windows plus the old value stay
    below 32: exact in bf16)"""
    g = _gen(k, s, p, H, W, 11)
    x = dyadic(g, (POOL_N, POOL_C, H, W), 0.5, 3)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return x, dyadic(g, (POOL_N, POOL_C, ho, wo)), dyadic(g, (POOL_N, POOL_C, H, W))


def maxpool_ref(x, dy, k, s, p, old=None):
    """-> y, dx (+ old) of F.max_pool2d on fp64 data (the gradient goes to the first maximum in scan order)"""
    xr = x.double().clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s, p)
    y.backward(dy.double())
    return y.detach(), xr.grad if old is None else xr.grad + old.double()


GLOBAL_CASES = [(2, 1, 64), (3, 3, 96), (2, 5, 130), (2, 20, 96), (1, 49, 64)]      # (N, HW, C)
WAVE_PAIRS = [(a, b) for a in range(4) for b in range(4) if a != b]


def global_case(N, HW, C):
    """x [N, HW, C], dy [N, C] on coarse grids; plant_wave_ties puts the column maximum twice into most channels"""
    g = _gen(N, HW, C, 5)
    x = dyadic(g, (N, HW, C), 0.5, 3)
    return x, dyadic(g, (N, C))


def plant_wave_ties(x):
    """in channel c of every image: the maximum (4.0, above the grid) at a position of wave a = p % 4 and once more at a LATER
    position of wave b, (a, b) = WAVE_PAIRS[c % 12] (the kernel's four waves take p % 4; the fold must prefer the smaller p,
    not the smaller wave).  -> the set of pairs that fit into HW"""
    N, HW, C = x.shape
    done = set()
    for c in range(C):
        a, b = WAVE_PAIRS[c % 12]
        p2 = next((p for p in range(a + 1, HW) if p % 4 == b), None)
        if a < HW and p2 is not None:
            x[:, a, c] = 4.0
            x[:, p2, c] = 4.0
            done.add((a, b))
    return done


def global_pool_ref(x, dy, is_max):
    """x [N, HW, C] fp64, dy [N, C] -> y [N, C], arg-max position [N, C] (None for the mean), dx [N, HW, C]"""
    xr = x.double().permute(0, 2, 1).unsqueeze(-1).clone().requires_grad_(True)      # [N, C, HW, 1]
    if is_max:
        y, idx = F.adaptive_max_pool2d(xr, 1, return_indices=True)
        idx = idx.flatten(1)
    else:
        y, idx = F.adaptive_avg_pool2d(xr, 1), None
    y.flatten(1).backward(dy.double())
    return y.detach().flatten(1), idx, xr.grad.squeeze(-1).permute(0, 2, 1).contiguous()


ADAPTIVE_CASES = [(14, 14, 7, 7, True), (7, 7, 7, 7, True), (1, 2, 7, 7, True), (10, 9, 7, 7, False), (5, 3, 2, 2, False)]


def adaptive_windows(n_in, n_out):
    """[start, end) of every output cell: floor(o * n / N), ceil((o + 1) * n / N)"""
    return [((o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)) for o in range(n_out)]


def adaptive_case(H, W, OH, OW):
    """x NCHW, dy [N, C*OH*OW]: gradients multiples of 0.25 in [-0.5, 0.5] (28 cells of area 1 or 2 meet in one pixel of the
    1 x 2 input: multiples of 1/8 below 16)"""
    g = _gen(H, W, OH, OW, 7)
    return dyadic(g, (POOL_N, POOL_C, H, W), 0.5, 3), dyadic(g, (POOL_N, POOL_C * OH * OW), 0.25, 2)


def adaptive_avg_ref(x, dy, OH, OW):
    """-> y [N, C*OH*OW] (torch's NCHW flatten order), dx NCHW, and for the inexact cases the slack of dx: one fp32 ulp (at the
    magnitude sum |dy| / area of the pixel) per division, which covers the additions between them"""
    xr = x.double().clone().requires_grad_(True)
    y = F.adaptive_avg_pool2d(xr, (OH, OW)).flatten(1)
    y.backward(dy.double())
    dx = xr.grad
    H, W = x.shape[2:]
    area = torch.tensor([[(h1 - h0) * (w1 - w0) for (w0, w1) in adaptive_windows(W, OW)] for (h0, h1) in adaptive_windows(H, OH)],
                        dtype=torch.float64)

    def back(d):
        z = torch.zeros_like(x, dtype=torch.float64, requires_grad=True)
        F.adaptive_avg_pool2d(z, (OH, OW)).backward(d.reshape(x.shape[0], x.shape[1], OH, OW))
        return z.grad
    cnt = back(area.expand(x.shape[0], x.shape[1], OH, OW).contiguous())
    mag = back(dy.double().abs())
    return y.detach(), dx, cnt * cb.ulp(mag, F32)


def adaptive_avg_plain(x, OH, OW, shift=0):
    """the same pooling written out with adaptive_windows (shift = 1: every window's columns start one late, the off-by-one a
    checker must reject)"""
    N, C, H, W = x.shape
    y = torch.zeros(N, C, OH, OW, dtype=torch.float64)
    for oh, (h0, h1) in enumerate(adaptive_windows(H, OH)):
        for ow, (w0, w1) in enumerate(adaptive_windows(W, OW)):
            w0s = min(w0 + shift, w1 - 1)
            y[:, :, oh, ow] = x[:, :, h0:h1, w0s:w1].double().sum((2, 3)) / ((h1 - h0) * (w1 - w0))
    return y.flatten(1)


# ---- dropout -----------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def mix32(k):
    """the splitmix64 finaliser of head.hip on a numpy uint64 array -> the upper 32 bits"""
    with np.errstate(over="ignore"):
        k = k + np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (k ^ (k >> np.uint64(31))) >> np.uint64(32)


def dropout_ref(x, p, seed, counter=None):
    """-> mask (uint8), y (fp64), scale.  key = seed * 0x100000001B3 + i with seed ^= counter * 0xD1342543DE82EF95 first;
    u = (h >> 8) * 2^-24; keep = u >= float32(p); scale = float32(1 / (1 - float32(p))) (a per-launch scalar; 0 for p = 1)"""
    n = x.numel()
    seed = int(seed) & _M64
    if counter is not None:
        seed ^= ((int(counter) & 0xFFFFFFFF) * 0xD1342543DE82EF95) & _M64
    base = np.uint64((seed * 0x100000001B3) & _M64)
    with np.errstate(over="ignore"):
        h = mix32(base + np.arange(n, dtype=np.uint64))
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    keep = u >= p32
    scale = float(np.float32(1) / (np.float32(1) - p32)) if p32 < 1 else 0.0
    mask = torch.from_numpy(keep.astype(np.uint8))
    return mask, torch.where(mask.bool(), x.double() * scale, torch.zeros_like(x, dtype=torch.float64)), scale


# ---- seg_counts --------------------------------------------------------------------------------------------------------------------
def seg_counts_case(B, per, is_logit, thr):
    """predictions kept at least 1e-3 (in probability) away from the threshold, targets in {0, 1}"""
    g = _gen(B, per, is_logit, int(thr * 10))
    pr = torch.rand(B, per, generator=g).double()
    pr = torch.where((pr - f32(thr)).abs() < 2e-3, pr + 0.01, pr).clamp(1e-4, 1 - 1e-4)
    v = torch.log(pr / (1 - pr)) if is_logit else pr
    return v.float(), (torch.rand(B, per, generator=g) > 0.6).float()


def seg_counts_ref(v, t, is_logit, thr):
    """-> counts [B, 4] (tp, predicted, target, equal) and the smallest |probability - thr| of the inputs"""
    thr = f32(thr)
    pr = torch.sigmoid(v.double()) if is_logit else v.double()
    pb, tb = pr > thr, t.double() > thr
    c = torch.stack([(pb & tb).sum(1), pb.sum(1), tb.sum(1), (pb == tb).sum(1)], 1).double()
    return c, float((pr - thr).abs().min())


# ---- fp32 dot products: Linear -------------------------------------------------------------------------------------------------------
LINEAR_CASES = [  # (B, I, O, relu, kernel)
    (1, 1, 1, 0, "small"), (3, 70, 5, 1, "small"), (1, 1020, 1028, 0, "small"),
    (1, 1024, 1024, 0, "wide"), (17, 4100, 257, 1, "wide"), (2, 4096, 300, 0, "wide")]


def linear_case(B, I, O):
    g = _gen(B, I, O, 3)
    r = lambda *s: torch.randn(*s, generator=g).float()
    return dict(x=r(B, I), w=r(O, I) / math.sqrt(I), bias=r(O), dy=r(B, O), old_dw=r(O, I), old_db=r(O))


def linear_fwd_ref(x, w, bias, relu):
    """-> y, bound: |y - Y| <= C sqrt(I) 2^-24 (|x| |w|^T + |bias|) (a ReLU does not widen it)"""
    x, w = x.double(), w.double()
    z, a = x @ w.T, x.abs() @ w.abs().T
    if bias is not None:
        z, a = z + bias.double(), a + bias.double().abs()
    return (z.clamp(min=0) if relu else z), cb.bound("fp32", None, a, x.shape[1], F32)


def linear_bwd_ref(x, w, y_gpu, dy, relu, beta, old_dw, old_db):
    """-> {dx, dw, db: (value, bound)}; the ReLU mask is that of the y the forward stored; K = O, B, B"""
    x, w, g = x.double(), w.double(), dy.double()
    if relu:
        g = g * (y_gpu.double() > 0)
    beta = f32(beta)
    B, O = g.shape
    out = {"dx": (g @ w, cb.bound("fp32", None, g.abs() @ w.abs(), O, F32))}
    odw = None if beta == 0 else beta * old_dw.double()
    odb = None if beta == 0 else beta * old_db.double()
    dw, db = g.T @ x, g.sum(0)
    out["dw"] = (dw if odw is None else dw + odw, cb.bound("fp32", None, g.abs().T @ x.abs(), B, F32, old=odw))
    out["db"] = (db if odb is None else db + odb, cb.bound("fp32", None, g.abs().sum(0), B, F32, old=odb))
    return out


# ---- gradient norm -------------------------------------------------------------------------------------------------------------------
NORM_NS = [1, 3, 5, 1023, 100_003, 3_145_728 + 4 * 1000 + 3]
CLIP_NBLOCKS = [1, 64, 65, 1024]


def rowreduce_blocks(n):
    """mi355_rowreduce_blocks, for the CPU restatement only (the GPU file asks the library)"""
    return max(1, min((n + 63) // 64, 1024))


def clip_case(nblocks):
    """partial sums of squares as mi355_clip_coef takes them"""
    return (torch.rand(nblocks, generator=_gen(nblocks, 47)) * 100).float()


def norm_case(n):
    return torch.randn(n, generator=_gen(n, 17)).float() * 3


def norm_ref(sumsq, inv_scale=1.0, dev_scale=1.0):
    """sumsq: the exact sum (fp64) -> norm, bound (NORM_ULPS * 2^-24 relative)"""
    nrm = math.sqrt(float(sumsq)) * f32(inv_scale) * f32(dev_scale)
    return nrm, NORM_ULPS * U24 * nrm


def coef_ref(nrm, nrm_bound, max_norm):
    """min(1, max / (norm + 1e-6)): the norm's bound propagated, plus the roundings of the sum and the quotient; exactly 1 for
    max_norm <= 0"""
    mx = f32(max_norm)
    if not mx > 0:
        return 1.0, 0.0
    c = mx / (nrm + f32(1e-6))
    return min(1.0, c), c * (nrm_bound / (nrm + f32(1e-6)) + 2 * U24)


def emu_norm(g, nb, inv_scale=1.0, dev_scale=1.0):
    """the kernels' chain: double sums per workgroup, each rounded to fp32, folded in double, sqrt rounded, two fp32 scalings"""
    g = g.double().numpy()
    part = np.array([np.float32((g[b::nb] ** 2).sum()) for b in range(nb)], np.float64)
    nrm = np.float32(math.sqrt(part.sum()))
    return float(np.float32(np.float32(nrm * np.float32(inv_scale)) * np.float32(dev_scale)))


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------------
ADAMW_NS = [1, 255, 100_003, 524_288 + 259]
ADAMW_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4)
ADAMW_SCALE = (0.25, 1.0 / 1024)             # inv_scale (host), dev_scale (device): the stored gradients carry a factor 4096


def adamw_case(n):
    """p0 and the three stored gradients (scales 10, 1e-3, 1e-3 as in test_clip_and_adamw_match_torch, times 4096)"""
    g = _gen(n, 23)
    p0 = torch.randn(n, generator=g).float()
    return p0, [(torch.randn(n, generator=g) * (10 if it == 0 else 0.001) * 4096).float() for it in range(3)]


def adamw_ref(p, m, v, g, t, coef=1.0, inv_scale=1.0, dev_scale=1.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4):
    """one step of adamw_kernel in fp64 from the state (p, m, v) -> {p, m, v: (value, per-element bound)} and the update delta.
    u = 2^-24 is the relative error of one fp32 rounding.  The kernel's chain:
      gg = g * gs, gs = coef * inv_scale * dev_scale              3 roundings
      m' = b1 m + (1 - b1) gg                                     2 u |b1 m| + 6 u |(1 - b1) gg|     (1 - b1, gg, product, sum)
      v' = b2 v + ((1 - b2) gg) gg                                2 u |b2 v| + 10 u (1 - b2) gg^2
      bc = 1 - powf(b, t)                                         POW_U u b^t / (1 - b^t) + u: the cancellation amplifies powf
      delta = (lr / bc1) m' / (sqrtf(v') / sqrtf(bc2) + eps)      7 roundings, rel(bc1), rel(bc2) / 2, e_v / (2 v'); e_m / |m'|
      p' = p (1 - lr wd) - delta                                  2 u |p decay| (decay, product) + u |p'| + e_delta"""
    p, m, v, g = (a.double() for a in (p, m, v, g))
    lr, b1, b2, eps, wd, coef, inv, dev = (f32(a) for a in (lr, beta1, beta2, eps, wd, coef, inv_scale, dev_scale))
    u = U24
    gg = g * (coef * inv * dev)
    am, bm = b1 * m, (1 - b1) * gg
    mm, e_m = am + bm, u * (2 * am.abs() + 6 * bm.abs())
    av, bv = b2 * v, (1 - b2) * gg * gg
    vv, e_v = av + bv, u * (2 * av.abs() + 10 * bv)
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1 - pw1, 1 - pw2
    r1, r2 = POW_U * u * pw1 / bc1 + u, POW_U * u * pw2 / bc2 + u
    step = lr / bc1
    d = vv.sqrt() / math.sqrt(bc2) + eps
    delta = step * mm / d
    rel = 7 * u + r1 + 0.5 * r2 + torch.where(vv > 0, 0.5 * e_v / vv.clamp(min=1e-300), torch.zeros_like(vv))
    e_d = delta.abs() * rel + step * e_m / d
    pp = p * (1 - lr * wd)
    pn = pp - delta
    e_p = u * (2 * pp.abs() + pn.abs()) + e_d
    return {"p": (pn, K_ADAMW * e_p), "m": (mm, K_ADAMW * e_m), "v": (vv, K_ADAMW * e_v)}, delta


def emu_adamw(p, m, v, g, t, coef=1.0, inv_scale=1.0, dev_scale=1.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=5e-4):
    """adamw_kernel line by line in numpy float32 (every operation rounded, nothing fused)"""
    f = np.float32
    p, m, v, g = (a.float().numpy() for a in (p, m, v, g))
    lr, b1, b2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    gs = f(f(f(coef) * f(inv_scale)) * f(dev_scale))
    tt = f(t)
    bc1 = f(1) - np.power(b1, tt)
    bc2s = np.sqrt(f(1) - np.power(b2, tt))
    step, decay = lr / bc1, f(1) - lr * wd
    gg = g * gs
    pp = p * decay
    mm = b1 * m + (f(1) - b1) * gg
    vv = b2 * v + (f(1) - b2) * gg * gg
    pp = pp - step * mm / (np.sqrt(vv) / bc2s + eps)
    assert pp.dtype == mm.dtype == vv.dtype == np.float32
    return torch.from_numpy(pp), torch.from_numpy(mm), torch.from_numpy(vv)


# ---- BCE with logits -------------------------------------------------------------------------------------------------------------------
BCE_NS = [1, 1000, 5000, 1_048_576 + 1025]
BCE_EDGES = [0.0, -0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]


def bce_case(n):
    """logits N(0, 3) with the edge values spread over the front, targets in {0, 1} and a soft 0.3"""
    g = _gen(n, 29)
    z = torch.randn(n, generator=g).float() * 3
    t = (torch.rand(n, generator=g) > 0.5).float()
    e = torch.tensor(BCE_EDGES)
    k = min(n, 3 * len(e))
    z[:k] = e.repeat(3)[:k] if n > 1 else torch.tensor([-20.0])
    t[:k] = torch.tensor([0.0, 1.0, 0.3]).repeat_interleave(len(e))[:k]
    return z, t


def _exp_rel(a, arg_roundings=2):
    """relative error of __expf(a) = exp2(a * log2e): the scaled argument carries `arg_roundings` relative roundings, which the
    exponential turns into |a| u each (ln2 * log2e = 1); v_exp_f32 itself 1 ulp = 2 u"""
    return (arg_roundings * a.abs() + 2) * U24


def bce_ref(z, t, gscale=1.0):
    """-> (loss, bound), (dz, per-element bound).  Per element, e = __expf(-|x|):
      l = max(x, 0) - x y + log1pf(e)      log1pf: 2 ulp of its value + rel(e) e / (1 + e); the product, the difference and the
                                           sum one rounding each
      dz = (1 / (1 + __expf(-x)) - y) gs   sigmoid: sum and quotient 2 u + rel(E) E / (1 + E); the difference, gs = gscale / n
                                           and the product 3 u
    the loss sums n fp32 terms in some order: conv_bounds' C sqrt(n) 2^-24 sum |l|, and two roundings of the mean"""
    z, t = z.double(), t.double()
    n, u = z.numel(), U24
    a = z.abs()
    e = torch.exp(-a)
    l1p = torch.log1p(e)
    e_l1p = _exp_rel(a) * e / (1 + e) + 4 * u * l1p + TINY
    mx, xy = z.clamp(min=0), z * t
    l = mx - xy + l1p
    e_l = e_l1p + u * (xy.abs() + (mx - xy).abs() + l.abs())
    loss = float(l.sum()) / n
    e_loss = (K_BCE * float(e_l.sum()) + cb.C * math.sqrt(n) * u * float(l.abs().sum())) / n + 2 * u * abs(loss)
    E = torch.exp(-z)
    s = 1 / (1 + E)
    gs = f32(gscale) / n
    dz = (s - t) * gs
    e_dz = gs * (s * (2 * u + _exp_rel(a) * E / (1 + E)) + 3 * u * (s - t).abs()) + TINY
    return (loss, e_loss), (dz, K_BCE * e_dz)


def _expf32(a):
    """__expf in float32: the argument scaled by fp32 log2(e) (one rounding), exp2 in float32"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(a * np.float32(1.4426950408889634)).astype(np.float32)


def _sum32(terms, blocks):
    """a float32 sum in the kernels' shape: `blocks` * 256 strided per-thread chains, a pairwise fold per workgroup, the
    workgroups one after the other"""
    f = np.float32
    T = blocks * 256
    pad = (-terms.size) % T
    acc = np.zeros(T, f)
    for r in np.concatenate([terms.astype(f), np.zeros(pad, f)]).reshape(-1, T):
        acc = acc + r
    return acc.reshape(blocks, 256)


def emu_bce(z, t, gscale=1.0):
    """bce_logits_kernel in numpy float32"""
    f = np.float32
    z, t = z.float().numpy(), t.float().numpy()
    n = z.size
    gs = f(gscale) / f(n)
    with np.errstate(over="ignore"):
        l = np.maximum(z, f(0)) - z * t + np.log1p(_expf32(-np.abs(z)))
        dz = (f(1) / (f(1) + _expf32(-z)) - t) * gs
    blocks = min((n + 1023) // 1024, 1024)
    loss = f(0)
    for b in _sum32(l, blocks):
        w = b.reshape(4, 64)
        for sft in (32, 16, 8, 4, 2, 1):
            w = w[:, :sft] + w[:, sft:2 * sft]
        loss = loss + f(f(f(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]) / f(n)
    assert l.dtype == dz.dtype == np.float32
    return float(loss), torch.from_numpy(dz)


# ---- cross-entropy with label smoothing ------------------------------------------------------------------------------------------------
CE_CASES = [(1, 1), (6, 3), (257, 3), (5, 1000)]


def ce_case(B, C):
    """logits N(0, 2); every third row holds one logit 60 above the rest"""
    g = _gen(B, C, 31)
    z = torch.randn(B, C, generator=g).float() * 2
    y = torch.randint(0, C, (B,), generator=g)
    for b in range(0, B, 3):
        if C > 1:
            z[b, int(torch.randint(0, C, (1,), generator=g))] += 60.0
    return z, y


def ce_ref(z, y, sm, gscale=1.0):
    """-> (loss, bound), (dz [B, C], per-element bound).  Per row, a_c = x_c - max:
      se = sum __expf(a_c)                 rel(exp_c) = (3 |a_c| + 2) u (the difference is rounded, then scaled); the sum of C
                                           positive terms C sqrt(C) u
      lse = max + __logf(se)               rel(se) + 2 ulp of log(se) + one rounding
      logp_c = x_c - lse                   e_lse + u |logp_c|;  their sum over c: C sqrt(C) u sum |logp_c| on top
      l = -(1 - sm) logp_lab - sm sum / C  two roundings per term, one for the difference
      dz = (__expf(logp_c) - tgt_c) gs     the argument's error e_logp becomes relative, __expf 2 |logp| u + 2 u; tgt 3 u, the
                                           difference, gs = gscale / B and the product 3 u"""
    z = z.double()
    B, C = z.shape
    sm, u = f32(sm), U24
    mx = z.max(1).values
    a = z - mx[:, None]
    ex = torch.exp(a)
    se = ex.sum(1)
    rel_se = (ex * _exp_rel(a, 3)).sum(1) / se + cb.C * math.sqrt(C) * u
    lse = mx + se.log()
    e_lse = rel_se + 4 * u * se.log().abs() + u * lse.abs()
    logp = z - lse[:, None]
    e_logp = e_lse[:, None] + u * logp.abs()
    sl = logp.sum(1)
    e_sl = e_logp.sum(1) + cb.C * math.sqrt(C) * u * logp.abs().sum(1)
    ar = torch.arange(B)
    t1, t2 = (1 - sm) * logp[ar, y], sm * sl / C
    rowl = -t1 - t2
    e_row = (1 - sm) * e_logp[ar, y] + sm / C * e_sl + 3 * u * (t1.abs() + t2.abs())
    loss = float(rowl.sum()) / B
    e_loss = (K_CE * float(e_row.sum()) + cb.C * math.sqrt(B) * u * float(rowl.abs().sum())) / B + 2 * u * abs(loss)
    p = torch.exp(logp)
    tgt = torch.full_like(z, sm / C)
    tgt[ar, y] += 1 - sm
    gs = f32(gscale) / B
    dz = (p - tgt) * gs
    e_dz = gs * (p * (e_logp + _exp_rel(logp)) + 3 * u * tgt + 3 * u * (p - tgt).abs()) + TINY
    return (loss, e_loss), (dz, K_CE * e_dz)


def emu_ce(z, y, sm, gscale=1.0):
    """ce_smooth_kernel in numpy float32 (rows in parallel, the class loops sequential as in the kernel)"""
    f = np.float32
    z, y = z.float().numpy(), y.numpy()
    B, C = z.shape
    sm, gs = f(sm), f(gscale) / f(B)
    mx = z.max(1)
    se = np.zeros(B, f)
    for c in range(C):
        se = se + _expf32(z[:, c] - mx)
    lse = mx + np.log(se)
    sl = np.zeros(B, f)
    for c in range(C):
        sl = sl + (z[:, c] - lse)
    ar = np.arange(B)
    rowl = -(f(1) - sm) * (z[ar, y] - lse) - sm * sl / f(C)
    tgt = np.full((B, C), sm / f(C), f)
    tgt[ar, y] = (f(1) - sm) * f(1) + sm / f(C)
    dz = (_expf32(z - lse[:, None]) - tgt) * gs
    acc = np.zeros(256, f)
    for r in np.concatenate([rowl, np.zeros((-B) % 256, f)]).reshape(-1, 256):
        acc = acc + r
    w = acc.reshape(4, 64)
    for sft in (32, 16, 8, 4, 2, 1):
        w = w[:, :sft] + w[:, sft:2 * sft]
    loss = f(f(f(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]) / f(B)
    assert dz.dtype == rowl.dtype == np.float32
    return float(loss), torch.from_numpy(dz)
