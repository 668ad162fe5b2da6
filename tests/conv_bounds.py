"""Per-element error bounds for the convolution kernels against an fp64 reference (plain torch, CPU only).

A kernel result y is judged against the exact value Y of the same operation on the operands as the kernel sees them (rounded to
the storage dtype), computed in fp64:

    |y - M(Y)| <= r_T + C * sqrt(K) * 2^-24 * A          for every element,

  - A = sum |a * b| (+ |bias| + |old|) of the element: the same operation on the absolute operands (mag64);
  - K = the reduction length of the element (fp32 accumulation of K products, any order);
  - M = the epilogue's rounding model (the table below: where the kernel rounds to the storage dtype T, in what order), emulated
    exactly in fp64; r_T = one ulp of T per rounding step of M (the fp32 error may move a value across a rounding boundary;
    0 for fp32 outputs).

2-byte outputs are also held to a statistical check on the larger half of the elements (|Y| >= median): the RMS error in ulps
may exceed that of the model's own roundings (0.289 ulp for one correct rounding) only by the CPU fp32 result's own error,
and the mean signed error (the bias a truncating or biased rounding leaves) must be within +-0.05 ulp.

C is fixed by tests/test_conv_bounds_cpu.py against two CORRECT fp32 summations (torch's blocked sums and a strictly sequential
chain in the kernels' (slab, tap) order), never fitted to the kernels under test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

C = 8.0                      # per-element constant: sequential fp32 chains pass with >= 2x margin (test_conv_bounds_cpu.py)
U24 = 2.0 ** -24             # unit round-off of fp32
RMS_ONE_ROUNDING = 0.289     # RMS of the error of one correct rounding, in ulps (1 / sqrt(12))
RMS_FACTOR = 1.25
MEAN_LIMIT = 0.05            # |mean signed error| in ulps

# mantissa bits (explicit) and smallest normal exponent of each output type
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}

# ---- epilogue rounding models -----------------------------------------------------------------------------------------------
# Read from the kernels' epilogues (csrc/); every 2-byte variant rounds the same way, the fp32 generic kernel keeps fp32 throughout:
#   "round"    y = R(relu?(acc + bias))                  one rounding.  conv3x3_halo.hpp:235 / conv3x3_halo_pp.hpp:297 /
#              conv3x3_ws.hpp:285 (bias = the first MFMA's C operand); conv3x3_halo_pp128.hpp:317-318, conv_gemm256.hpp:185-186,
#              conv1x1_stream.hpp:94-99 (bias = starting accumulator), conv_igemm.hip conv_igemm_kernel / conv_igemm_dma_kernel LDS
#              epilogues (acc + bias, then R)
#   "acc2"     y = R(R(relu?(acc + bias)) + old)          two roundings: the tile is rounded into the LDS staging tile first, the
#              destination added to the ROUNDED value (conv3x3_halo.hpp:316, _pp.hpp:376, _pp128.hpp:395, _ws.hpp:354,
#              conv1x1_stream.hpp:125, conv_gemm256.hpp:231, conv_igemm.hip (both 2-byte epilogues))
#   "pool2"    y = R(sum_2x2 R(acc))                     the four outputs of a 2x2 group are rounded, summed in fp32, rounded again
#              (conv3x3_halo.hpp:284-294, _pp.hpp:352-362, _pp128.hpp:371-381, _ws.hpp:326-336)
#   "pool2acc" y = R(sum_2x2 R(acc) + old)               ... with the destination added before the second rounding (:291 / :359 /
#              :378 / :333)
#   "fp32"     y = relu?(acc + bias) (+ old), all fp32    conv_igemm_kernel<float> (conv_igemm.hip, !LDS_EPI branch); the weight
#              gradients (fp32 partial slabs, fp32 split reduction with beta)
# variant (mi355_conv2d_igemm_variant_n) -> the models of the epilogues it serves (accumulate bit 0, ReLU bit 1, 2x2 sum bit 2)
VARIANT_EPILOGUES = {
    0: ("round", "acc2", "fp32"),                       # generic: 2-byte LDS epilogue, or fp32 in registers
    1: ("round", "acc2"),                               # LDS-DMA ring
    2: ("round", "acc2", "pool2", "pool2acc"),          # 4-wave halo 8x32
    3: ("round", "acc2", "pool2", "pool2acc"),          # 4-wave halo 16x16
    4: ("round", "acc2"),                               # 1x1 stream
    5: ("round", "acc2", "pool2", "pool2acc"),          # ping-pong halo (64 channels)
    6: ("round", "acc2", "pool2", "pool2acc"),          # ping-pong halo (128 channels)
    7: ("round", "acc2", "pool2", "pool2acc"),          # weight-stationary, Ci = 64
    8: ("round", "acc2", "pool2", "pool2acc"),          # weight-stationary, Ci = 128
    9: ("round", "acc2"),                               # padding-free GEMM (1x1, 2x2/s2, ConvTranspose2d phases)
}
VARIANT_NAMES = {0: "generic", 1: "dma", 2: "halo8x32", 3: "halo16x16", 4: "stream1x1", 5: "halo_pp", 6: "halo_pp128", 7: "ws64",
                 8: "ws128", 9: "gemm256"}
WGRAD_NAMES = {0: "wgrad_generic", 1: "wgrad_halo32", 2: "wgrad_halo16x2", 3: "wgrad_halo8_64", 4: "wgrad_halo8_32x2"}


def model_for(accumulate: int, dtype) -> str:
    """the epilogue model of an ABI `accumulate` bit set"""
    if dtype == torch.float32:
        return "fp32"
    acc, pool = accumulate & 1, (accumulate >> 2) & 1
    return ("pool2acc" if acc else "pool2") if pool else ("acc2" if acc else "round")


# ---- rounding helpers ---------------------------------------------------------------------------------------------------------
def rnd(x, dtype):
    """round-to-nearest-even to `dtype`, back in fp64 (fp64 -> fp32 -> 2-byte double-rounds only in exact ties of fp32, which
    never matter at the bounds used here; torch's fp64 -> bf16 cast goes through fp32 as well)"""
    return x.to(dtype).double()


def ulp(y, dtype):
    """one ulp of `dtype` at |y| (fp64 tensor); the subnormal floor for fp16 (2^-24) and bf16 / fp32 (2^-133 / 2^-149)"""
    mant, emin = _FMT[dtype]
    e = torch.frexp(y.double().abs())[1].double() - 1          # floor(log2 |y|); 0 for y == 0 -> clamped below
    e = torch.where(y == 0, torch.full_like(e, emin), torch.clamp(e, min=emin))
    return torch.pow(2.0, e - mant)


# ---- fp64 references ----------------------------------------------------------------------------------------------------------
def up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _fwd(x, w, b, stride, pad, up):
    return F.conv2d(up2(x) if up else x, w, b, stride=stride, padding=pad)


def ref64(op, x, w, b=None, dtype=torch.float32, hw=None):
    """fp64 result of `op` on the operands as the kernel sees them (x, w rounded to `dtype`; bias fp32), NCHW.
    op = dict(kind=fwd | dgrad | convT | wgrad, stride, pad, up):
      fwd   x [N,Ci,H,W], w [Co,Ci,k,k]             -> conv2d(up2?(x), w) + b
      dgrad x = dy [N,Co,Ho,Wo], w [Co,Ci,k,k]      -> input gradient on the (logical) input grid hw
      convT x [N,Ci,H,W], w [Ci,Co,k,k] (stride s)  -> conv_transpose2d(x, w, stride=s) + b
      wgrad x [N,Ci,H,W], w = dy [N,Co,Ho,Wo]       -> dW [Co,Ci,k,k] (k = op['k']), built image by image
    The same with every operand replaced by its absolute value is mag64."""
    return _op64(op, rnd(x, dtype), rnd(w, dtype), None if b is None else b.double(), hw)


def mag64(op, x, w, b=None, dtype=torch.float32, hw=None):
    """A = sum |a * b| (+ |bias|) per output element"""
    return _op64(op, rnd(x, dtype).abs(), rnd(w, dtype).abs(), None if b is None else b.double().abs(), hw)


def _op64(op, x, w, b, hw):
    kind, s, p, up = op["kind"], op.get("stride", 1), op.get("pad", 0), op.get("up", 0)
    if kind == "fwd":
        return _fwd(x, w, b, s, p, up)
    if kind == "dgrad":
        n = x.shape[0]
        y = torch.nn.grad.conv2d_input((n, w.shape[1]) + tuple(hw), w, x, stride=s, padding=p)
        return y if b is None else y + b.view(1, -1, 1, 1)
    if kind == "convT":
        return F.conv_transpose2d(x, w, b, stride=s)
    if kind == "wgrad":
        k = op["k"]
        shape = (w.shape[1], x.shape[1], k, k)
        out = torch.zeros(shape, dtype=torch.float64)
        for i in range(x.shape[0]):                     # image by image: bounded memory at K = N * Ho * Wo >= 2^18
            xi = up2(x[i:i + 1]) if up else x[i:i + 1]
            out += torch.nn.grad.conv2d_weight(xi, shape, w[i:i + 1], stride=s, padding=p)
        return out
    raise ValueError(kind)


def reduction_length(op, ci, co, k, npix=None, bias=False):
    """K of one output element: taps x input channels for forward / data gradient (ci is the channel count reduced over), the
    pixel count for weight gradients (over all splits)"""
    if op["kind"] == "wgrad":
        return npix
    return ci * k * k + (1 if bias else 0)


def sum2x2(t):
    n, c, h, w = t.shape
    return t.view(n, c, h // 2, 2, w // 2, 2).sum((3, 5))


# ---- the epilogue models, emulated ---------------------------------------------------------------------------------------------
def apply_model(model, z, dtype, old=None, relu=False):
    """M(Z): the kernel's rounding sequence applied to exact values.  z is the exact pre-epilogue value (conv + bias, fp64) at the
    RESOLUTION the kernel accumulates on (the up-sampled grid for the pool2 models); returns the exact model value (unrounded,
    for the statistical check) and the rounded one."""
    if relu:
        z = z.clamp(min=0)
    if model == "fp32":
        exact = z if old is None else z + old
        return exact, exact.float().double()
    if model == "round":
        return z, rnd(z, dtype)
    if model == "acc2":
        return z + old, rnd(rnd(z, dtype) + old, dtype)
    if model in ("pool2", "pool2acc"):
        s_exact, s_inner = sum2x2(z), sum2x2(rnd(z, dtype))
        if model == "pool2acc":
            s_exact, s_inner = s_exact + old, s_inner + old
        return s_exact, rnd(s_inner, dtype)
    raise ValueError(model)


def bound(model, z, a, k, dtype, old=None, c=C):
    """per-element allowed |y - M(Y)|: one ulp of T per rounding step (at the value that step rounds, widened by the fp32 error)
    plus c * sqrt(K) * 2^-24 * A.  z / a at the accumulation resolution (as in apply_model)."""
    delta = c * math.sqrt(k) * U24 * a
    if model == "fp32":
        if old is not None:
            delta = c * math.sqrt(k + 1) * U24 * (a + old.abs())
        return delta
    if model == "round":
        return ulp(z.abs() + delta, dtype) + delta
    if model == "acc2":
        inner = ulp(z.abs() + delta, dtype)
        d2 = delta + inner
        return inner + ulp((z + old).abs() + d2, dtype) + d2
    if model in ("pool2", "pool2acc"):
        inner = ulp(z.abs() + delta, dtype)
        d4 = sum2x2(delta + inner)
        s = sum2x2(z) + (old if model == "pool2acc" else 0)
        return ulp(s.abs() + d4, dtype) + d4
    raise ValueError(model)


# ---- checks --------------------------------------------------------------------------------------------------------------------
def _where(idx, shape):
    out = []
    for d in reversed(shape):
        out.append(idx % d)
        idx //= d
    return tuple(reversed(out))


def element_check(y, m_rounded, bnd):
    """-> (max |y - M| / bound, number of elements over the bound, NCHW index of the worst element)"""
    err = (y.double() - m_rounded).abs()
    bad = ~(err <= bnd)                                   # NaN counts as over the bound
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = int(torch.argmax(ratio.flatten()))
    return float(ratio.flatten()[worst]), int(bad.sum()), _where(worst, tuple(y.shape))


def stat_check(y, y_exact, dtype, rms_model, y_cpu32=None):
    """statistical check of 2-byte outputs on the elements with |Y| >= median |Y| (Y != 0): -> (rms_ulps, rms_limit, mean_ulps).
    rms_model: the RMS, in ulps, of the epilogue model's own roundings; y_cpu32: the CPU fp32 result (its own error against Y
    widens the limit)."""
    ya = y_exact.abs()
    nz = ya[ya > 0]
    if nz.numel() == 0:
        return 0.0, 0.0, 0.0
    sel = ya >= nz.median()
    Y = y_exact[sel]
    u = ulp(Y, dtype)
    e = (y.double()[sel] - Y) / u
    rms = float(e.pow(2).mean().sqrt())
    mean = float((e * Y.sign()).mean())
    s = float(((y_cpu32.double()[sel] - Y) / u).pow(2).mean().sqrt()) if y_cpu32 is not None else 0.0
    return rms, RMS_FACTOR * math.sqrt(rms_model ** 2 + s ** 2), mean


def model_rms(model, z, dtype, old=None, relu=False):
    """RMS in ulps (over |Y| >= median) of the model's own roundings against the exact value"""
    if model == "round":
        return RMS_ONE_ROUNDING
    exact, rounded = apply_model(model, z, dtype, old, relu)
    return stat_check(rounded, exact, dtype, 0.0)[0]


class Report:
    """outcome of one comparison; .ok, .msg, and the figures the GPU tests print per variant"""

    def __init__(self, name, ratio, nbad, worst, rms=None, rms_lim=None, mean=None, numel=0):
        self.name, self.ratio, self.nbad, self.worst = name, ratio, nbad, worst
        self.rms, self.rms_lim, self.mean, self.numel = rms, rms_lim, mean, numel

    @property
    def ok(self):
        if self.nbad:
            return False
        if self.rms is not None and (not self.rms <= self.rms_lim or not abs(self.mean) <= MEAN_LIMIT):
            return False
        return True

    @property
    def msg(self):
        s = f"{self.name}: max err/bound {self.ratio:.3g}, {self.nbad} of {self.numel} elements over the bound, worst at (n,c,h,w)={self.worst}"
        if self.rms is not None:
            s += f"; RMS {self.rms:.3f} ulp (limit {self.rms_lim:.3f}), mean signed {self.mean:+.4f} ulp (limit +-{MEAN_LIMIT})"
        return s


def check(name, y, z, a, k, dtype, model, old=None, relu=False, y_cpu32=None, c=C):
    """the combined check of one kernel output y (NCHW, any dtype) against the exact pre-epilogue value z (conv + bias, fp64) and
    its magnitude a, at the accumulation resolution; old = the destination's previous contents (fp64) for accumulating models.
    y_cpu32: the CPU fp32 result at the OUTPUT resolution, exact epilogue applied (for the statistical limit)."""
    exact, m = apply_model(model, z, dtype, old, relu)
    bnd = bound(model, z if not relu else z.clamp(min=0), a, k, dtype, old, c)
    ratio, nbad, worst = element_check(y, m, bnd)
    if dtype == torch.float32 or model == "fp32":
        return Report(name, ratio, nbad, worst, numel=y.numel())
    rms, lim, mean = stat_check(y, exact, dtype, model_rms(model, z, dtype, old, relu), y_cpu32)
    return Report(name, ratio, nbad, worst, rms, lim, mean, y.numel())


def stats_bound_check(partial, y, rows):
    """fused BatchNorm statistics: partial [rows, 2, C] (fp32) folded in fp64 against fp64 sums of the kernel's own rounded
    outputs y [M, C]; allowed (pixels per row + rows) * 2^-24 * sum|y| (and with y^2).  -> (max err/bound for sum, for sum sq)"""
    p = partial.double().view(rows, 2, -1).sum(0)
    yd = y.double()
    per = -(-yd.shape[0] // rows)
    out = []
    for q, (v, mag) in enumerate(((yd.sum(0), yd.abs().sum(0)), ((yd * yd).sum(0), (yd * yd).sum(0)))):
        b = (per + rows) * U24 * mag
        err = (p[q] - v).abs()
        r = torch.where(b > 0, err / b, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        out.append(float(torch.nan_to_num(r, nan=math.inf).max()))
    return tuple(out)


def old_criterion(y, ref, dtype):
    """today's op-level parity criterion of tests/test_gpu_conv.py: max|y - ref| / max|ref| < TOL"""
    tol = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 3e-3}[dtype]
    rel = float((y.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))
    return rel, rel < tol


# ---- a strictly sequential fp32 chain (the worst order a correct kernel can have) ----------------------------------------------
def seq_chain_fwd(x, w, b, stride, pad, up, slab=32):
    """conv2d of fp32-representable operands as ONE fp32 chain per output element in the kernels' (32-channel slab, tap, channel)
    order, starting from the bias; numpy float32 (every product and every sum rounded)."""
    x = (up2(x) if up else x).float()
    n, ci, h, wd = x.shape
    co, _, kh, kw = w.shape
    cols = F.unfold(x, (kh, kw), padding=pad, stride=stride)         # [N, ci*kh*kw, L], row index = c * kh*kw + tap
    L = cols.shape[2]
    ho = (h + 2 * pad - kh) // stride + 1
    wo = (wd + 2 * pad - kw) // stride + 1
    a = cols.permute(0, 2, 1).reshape(n * L, ci, kh * kw).numpy()
    wm = w.float().reshape(co, ci, kh * kw).numpy()
    acc = np.broadcast_to((b.float().numpy() if b is not None else np.zeros(co, np.float32))[None, :], (n * L, co)).copy()
    for s0 in range(0, ci, slab):
        for t in range(kh * kw):
            for c in range(s0, min(ci, s0 + slab)):
                acc = (acc + a[:, c, t][:, None] * wm[None, :, c, t]).astype(np.float32)
    return torch.from_numpy(acc).view(n, ho, wo, co).permute(0, 3, 1, 2).double()


def seq_chain_wgrad(x, dy, k, stride, pad, up):
    """weight gradient as ONE fp32 chain over the pixels (image, row, column) per (co, ci, tap)"""
    x = (up2(x) if up else x).float()
    n, ci = x.shape[:2]
    co = dy.shape[1]
    cols = F.unfold(x, (k, k), padding=pad, stride=stride)           # [N, ci*k*k, L]
    a = cols.permute(0, 2, 1).reshape(-1, ci * k * k).numpy()
    d = dy.float().permute(0, 2, 3, 1).reshape(-1, co).numpy()
    acc = np.zeros((co, ci * k * k), np.float32)
    for m in range(a.shape[0]):
        acc = (acc + d[m][:, None] * a[m][None, :]).astype(np.float32)
    return torch.from_numpy(acc).view(co, ci, k, k).double()
