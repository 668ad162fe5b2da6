"""Exact operands and fp64 references for the row-streaming BatchNorm passes (csrc/rowred.hpp, csrc/bn.hip).  CPU only.

The launchers take their per-channel constants as arguments, so a test can hand them operands for which every intermediate of
the kernel's formula is exactly representable in fp32 and every stored value in the storage type: small integers in the tensors,
powers of two and small integers in the constants.  Such a result does not depend on the summation order, on fma contraction or
on rounding, and a kernel must reproduce the fp64 reference BIT FOR BIT in fp32, bf16 and fp16 — a row that is dropped, read
twice or taken from the wrong place changes it.  The generators assert the exactness limits of the case they build.

The second half holds the derived bounds of the one real-data chain (reduce -> finalize -> apply) and a float32 restatement of
that chain in the kernels' own order, which tests/test_stream_exact_cpu.py holds to half of each bound."""
import math

import numpy as np
import torch

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
EPC = {F32: 4, BF: 8, FP: 8}
U24 = 2.0 ** -24


def geometry(dtype, C, B=1, cap=256):
    """(epc, cp, tpr, rp, rows per batch, rows per sweep of `cap` workgroups) as rowred_geom / rowred_grid / rowmap_launch
    compute them.  For choosing M and for printing only: no expected value comes from here."""
    epc = EPC[dtype]
    cp = C // epc
    tpr = min(cp, 256)
    rp = 256 // tpr
    return epc, cp, tpr, rp, rp * B, cap * rp * B


def fetch_grid(M, cap=256):
    """workgroups of a fetch-batched row reduction (for printing and for choosing M)"""
    return max(1, min((M + 63) // 64, 1024, cap))


# ---- generators ---------------------------------------------------------------------------------------------------------------
def ints(gen, shape, lim=4, pzero=0.3):
    """integers in [-lim, lim] as fp64, about `pzero` of them forced to zero (many zeros, many ties)"""
    t = torch.randint(-lim, lim + 1, shape, generator=gen).double()
    z = torch.rand(shape, generator=gen) < pzero
    return torch.where(z, torch.zeros_like(t), t)


def pow2(gen, C, lo, hi, signed=False):
    """powers of two 2^lo .. 2^hi per channel (fp64)"""
    t = torch.pow(2.0, torch.randint(lo, hi + 1, (C,), generator=gen).double())
    if signed:
        t = t * (torch.randint(0, 2, (C,), generator=gen).double() * 2 - 1)
    return t


class Consts:
    """per-channel constants of one case, fp64 [C]; .f(name) is the fp32 tensor a launcher takes"""

    def __init__(self, gen, C, small=False):
        self.C = C
        self.small = small
        self.xlim = 2 if small else 4                       # |x| <= xlim, |mean| <= xlim: |x - mean| <= 4 (small) / 8
        self.mean = ints(gen, (C,), self.xlim, 0.2)
        self.invstd = pow2(gen, C, -2, 0 if small else 2)
        self.gamma = pow2(gen, C, -1 if small else -2, 1 if small else 2, signed=True)
        self.mscale = pow2(gen, C, -2, 2, signed=True)
        self.mshift = ints(gen, (C,), 2, 0.3)
        self.scale = pow2(gen, C, -2, 2, signed=True)
        self.shift = ints(gen, (C,), 2, 0.3)
        self.scale2 = pow2(gen, C, -2, 2, signed=True)
        self.shift2 = ints(gen, (C,), 2, 0.3)
        for v in vars(self).values():
            if isinstance(v, torch.Tensor):
                assert torch.equal(v.float().double(), v)

    def f(self, name):
        return getattr(self, name).float()


def assert_storable(t, dtype, what=""):
    """every value of the fp64 tensor is exactly representable in `dtype`"""
    assert torch.equal(t.to(dtype).double(), t), f"{what}: not exactly representable in {dtype}"


def assert_f32_sum_exact(terms, quantum, what=""):
    """fp32 accumulation of the columns of `terms` (fp64 [M, C]) is exact in ANY order: every term is a multiple of `quantum` (a
    power of two) and sum |t| / quantum <= 2^24, so every partial sum of every order is an integer multiple of quantum below 2^24"""
    assert quantum > 0 and math.frexp(quantum)[0] == 0.5, quantum
    u = terms / quantum
    assert torch.equal(u, u.round()), f"{what}: terms are not multiples of {quantum}"
    top = float(u.abs().sum(0).max()) if terms.numel() else 0.0
    assert top <= 2.0 ** 24, f"{what}: sum |t| / quantum = {top:.0f} exceeds 2^24 (M = {terms.shape[0]})"


# ---- fp64 references of the launchers' contracts (include/mi355conv.h, the formulas of bn.hip) -----------------------------------
def ref_colsum(x):
    return x.sum(0)


def ref_stats(x):
    """mi355_bn_stats: (sum x, sum x^2) per channel"""
    return x.sum(0), (x * x).sum(0)


def ref_finalize(s, q, M, gamma, beta, rmean, rvar, momentum, eps):
    """mi355_bn_finalize in fp64, with the kernel's roundings of its INPUTS to the last two lines (invstd and mean are rounded to
    fp32 before scale / shift are formed): dict of fp64 tensors"""
    mean = s / M
    var = (q / M - mean * mean).clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    unb = var * M / (M - 1) if M > 1 else var
    mom = float(np.float32(momentum))
    out = {"mean": mean, "invstd": invstd, "rmean": (1.0 - mom) * rmean + mom * mean, "rvar": (1.0 - mom) * rvar + mom * unb}
    sc = gamma * invstd.float().double()
    out["scale"] = sc
    out["shift"] = beta - mean.float().double() * sc.float().double()
    return out


def relu_mask(act, y=None, x=None, mscale=None, mshift=None, fma=None):
    """the ReLU mask of the backward passes: y > 0 when the activated tensor is given, else fmaf(x, mscale, mshift) > 0 (`fma`:
    how to evaluate it on real data; exact data needs none); None when act == 0"""
    if not act:
        return None
    if y is not None:
        return y > 0
    if fma is not None:
        return fma(x.float(), mscale.float().view(1, -1), mshift.float().view(1, -1)) > 0
    return x * mscale + mshift > 0


def ref_bn_act(x, scale, shift, x2=None, scale2=None, shift2=None, res=None, act=0):
    """mi355_bn_act: act bit 0 = ReLU, bit 1 = the residual is added behind the activation"""
    v = x * scale + shift
    if x2 is not None:
        v = v + x2 * scale2 + shift2
    if res is not None and not act & 2:
        v = v + res
    if act & 1:
        v = v.clamp(min=0)
    if res is not None and act & 2:
        v = v + res
    return v


def windows(t, N, H, W):
    """[N*H*W, C] -> [N, H/2, W/2, C, 4] in window scan order (h, w), (h, w+1), (h+1, w), (h+1, w+1)"""
    C = t.shape[-1]
    v = t.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4)
    return v.reshape(N, H // 2, W // 2, C, 4)


def unwindows(v, N, H, W):
    C = v.shape[3]
    return v.reshape(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N * H * W, C)


def ref_pool2(y, N, H, W):
    """2 x 2 max of the stored activation: [N*H*W, C] -> [N*(H/2)*(W/2), C]"""
    return windows(y, N, H, W).max(-1)[0].reshape(-1, y.shape[-1])


def ref_pool_grad(x, mscale, mshift, dy, dp, N, H, W, dtype=None, fma=None):
    """the gradient reaching the BatchNorm output of a layer whose activation a = relu(fmaf(x, ms, mt)) (rounded to `dtype` when
    given, as the forward stored it) also feeds MaxPool2d(2, 2): g = [a > 0] * (dy + [first maximum of its window] * dp), torch's
    first-maximum rule in window scan order; dy None: the pooling is the only consumer"""
    if fma is not None:
        a = fma(x.float(), mscale.float().view(1, -1), mshift.float().view(1, -1)).double().clamp(min=0)
    else:
        a = (x * mscale + mshift).clamp(min=0)
    if dtype is not None:
        a = a.to(dtype).double()
    aw = windows(a, N, H, W)
    eq = aw == aw.max(-1, keepdim=True)[0]
    first = eq & (eq.cumsum(-1) == 1)
    routed = unwindows(first.double() * dp.reshape(N, H // 2, W // 2, -1, 1), N, H, W)
    t = routed if dy is None else dy + routed
    return torch.where(a > 0, t, torch.zeros_like(t))


def masked(dy, mask):
    return dy if mask is None else torch.where(mask, dy, torch.zeros_like(dy))


def bwd_terms(g, x, mean, invstd):
    """the two summands of the backward reduction per element: g and g * xhat"""
    return g, g * (x - mean) * invstd


def ref_bwd_sums(g, x, mean, invstd):
    t0, t1 = bwd_terms(g, x, mean, invstd)
    return t0.sum(0), t1.sum(0)


def ref_dx(g, x, gamma, mean, invstd, s0, s1, M):
    """dx = gamma * invstd * (g - s0 / M - xhat * s1 / M)"""
    xh = (x - mean) * invstd
    return gamma * invstd * (g - s0 / M - xh * (s1 / M))


def ref_dpost(dy, old=None, extras=()):
    """gradient of an operand added behind the activation: the unmasked dy (+ the old contents) (+ earlier gradients)"""
    v = dy.clone()
    if old is not None:
        v = v + old
    for e in extras:
        v = v + e
    return v


# ---- the real-data chain: derived bounds and the float32 restatement ----------------------------------------------------------------
def fma32(a, b, c):
    """fmaf of fp32 tensors (product exact in fp64, one rounding to fp64, one to fp32): the fused operation's sign"""
    return (a.double() * b.double() + c.double()).float()


def real_operands(shape, dtype, seed):
    """random real operands of a BatchNorm + ReLU backward at (N, C, H, W): dict with x, dy (fp64 [M, C], rounded to `dtype`) and
    the fp32 per-channel constants as the forward's finalize leaves them"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    M = n * h * w
    x = (torch.randn(M, c, generator=g) * (0.5 + torch.rand(c, generator=g)) + torch.randn(c, generator=g)).to(dtype).double()
    dy = torch.randn(M, c, generator=g).to(dtype).double()
    gamma = (0.5 + torch.rand(c, generator=g)).float()
    beta = (0.3 * torch.randn(c, generator=g)).float()
    mean = x.mean(0)
    var = (x * x).mean(0) - mean * mean
    invstd = (1.0 / torch.sqrt(var + 1e-5)).float()
    mean = mean.float()
    mscale = gamma * invstd
    mshift = beta - mean * mscale
    return dict(M=M, C=c, x=x, dy=dy, gamma=gamma, beta=beta, mean=mean, invstd=invstd, mscale=mscale, mshift=mshift)


def chain_terms(o, fma=fma32):
    """masked gradient g and the fp64 terms (g, g * xhat) of the chain's reduction"""
    g = masked(o["dy"], relu_mask(1, None, o["x"], o["mscale"], o["mshift"], fma))
    return (g,) + bwd_terms(g, o["x"], o["mean"].double(), o["invstd"].double())


def sums_chain_length(M, grid, rp):
    """K of the sums bound: the longest fp32 chain of one thread plus the levels of the fold tree (the folds behind are fp64)"""
    return -(-M // (grid * rp)) + (math.ceil(math.log2(rp)) if rp > 1 else 0)


def sums_bound(terms, K, c):
    """|s - s64| <= c * sqrt(K) * 2^-24 * sum |t| per channel"""
    return c * math.sqrt(K) * U24 * terms.abs().sum(0)


def dx_parts(o, g, s0, s1):
    """fp64 evaluation of dx from GIVEN fp32 sums (the apply pass judged alone) and the magnitude of its bound's fp32 part"""
    M = o["M"]
    mu, is_, gam = o["mean"].double(), o["invstd"].double(), o["gamma"].double()
    gi = gam * is_
    k0, k1 = s0.double() / M, s1.double() / M
    xh = (o["x"] - mu) * is_
    d64 = gi * (g - k0 - xh * k1)
    mag = gi.abs() * (g.abs() + k0.abs() + (xh * k1).abs())
    return d64, mag


def dx_bound(d64, dx, mag, dtype, ulp, c=16.0):
    """|dx - d64| <= 1/2 ulp_T(max(|d64|, |dx|)) + c * 2^-24 * |gi| (|g| + |k0| + |xhat k1|)"""
    return 0.5 * ulp(torch.maximum(d64.abs(), dx.double().abs()), dtype) + c * U24 * mag


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def sums32(terms, M, grid, rp, B, drop_row=None):
    """float32 restatement of a fetch-batched reduction of `terms` (fp64 [M, C], each rounded to fp32 first) in the kernel's order:
    workgroup b takes the batches b, b + grid, ... of rp * B rows, thread row ty the rows ty, ty + rp, ... of each (one fp32 chain),
    the rp chains are folded by the log-step tree, the workgroups' rows in fp64.  drop_row: leave that row out (a seeded fault)."""
    t = _f32(terms.numpy())
    if drop_row is not None:
        t = t.copy()
        t[drop_row] = 0
    C = t.shape[1]
    batch = rp * B
    trips = -(-M // (grid * batch))
    pad = np.zeros((trips * grid * batch, C), np.float32)
    pad[:M] = t
    v = pad.reshape(trips, grid, B, rp, C).transpose(1, 3, 0, 2, 4).reshape(grid, rp, trips * B, C)
    acc = np.cumsum(v, axis=2, dtype=np.float32)[:, :, -1]                      # sequential fp32 chain per (workgroup, ty)
    stride = 1
    while stride < rp:                                                          # rowred_kernel's tree over ty
        for ty in range(0, rp, 2 * stride):
            if ty + stride < rp:
                acc[:, ty] = acc[:, ty] + acc[:, ty + stride]
        stride *= 2
    return torch.from_numpy(acc[:, 0].astype(np.float64).sum(0)).float()


def dx32(o, g, s0, s1, dtype, fused=True, swap=False):
    """float32 restatement of bn_bwd_apply's arithmetic from fp32 sums, every step rounded; fused: the fmaf as one operation
    (exact product, one rounding) or as a rounded product and a rounded sum; swap: k0 and k1 exchanged (a seeded fault)"""
    M = o["M"]
    invM = np.float32(1.0 / M)
    x, gg = _f32(o["x"].numpy()), _f32(g.numpy())
    mu, is_, gam = _f32(o["mean"].numpy()), _f32(o["invstd"].numpy()), _f32(o["gamma"].numpy())
    k0, k1 = _f32(s0.numpy()) * invM, _f32(s1.numpy()) * invM
    if swap:
        k0, k1 = k1, k0
    gi = gam * is_
    xh = (x - mu) * is_
    t = gg - k0
    if fused:
        inner = (-xh.astype(np.float64) * k1.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
    else:
        inner = t - xh * k1
    d = gi * inner
    assert d.dtype == np.float32
    return torch.from_numpy(d).to(dtype)
