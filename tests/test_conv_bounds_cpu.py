"""CPU: the per-element bounds of tests/conv_bounds.py pass correct fp32 summations with margin (this fixes the constant C) and
fail every seeded kernel fault — including the ones today's max-relative criterion of tests/test_gpu_conv.py lets through."""
import math

import pytest
import torch

import conv_bounds as cb

BF, FP = torch.bfloat16, torch.float16
FWD = {"kind": "fwd", "stride": 1, "pad": 1, "up": 0}


def _fwd_case(n, ci, h, w_, co, dtype, seed=0, up=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w_, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    b = torch.randn(co, generator=g)
    op = dict(FWD, up=up)
    z = cb.ref64(op, x, w, b, dtype)
    a = cb.mag64(op, x, w, b, dtype)
    k = cb.reduction_length(op, ci, co, 3, bias=True)
    xq, wq = cb.rnd(x, dtype), cb.rnd(w, dtype)
    z32 = cb._fwd(xq.float(), wq.float(), b, 1, 1, up).double()           # torch's own (blocked) fp32 computation
    return dict(x=xq, w=wq, b=b.double(), z=z, a=a, k=k, z32=z32, op=op, dtype=dtype)


def _wgrad_case(n, ci, h, w_, co, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w_, generator=g)
    dy = torch.randn(n, co, h, w_, generator=g)
    op = {"kind": "wgrad", "stride": 1, "pad": 1, "up": 0, "k": 3}
    dtype = BF
    z = cb.ref64(op, x, dy, None, dtype)
    a = cb.mag64(op, x, dy, None, dtype)
    xq, dyq = cb.rnd(x, dtype), cb.rnd(dy, dtype)
    z32 = cb._op64(op, xq.float(), dyq.float(), None, None).double()
    return dict(x=xq, dy=dyq, z=z, a=a, k=n * h * w_, z32=z32, op=op)


@pytest.fixture(scope="module")
def fwd_cases():
    # the issue's shapes: 128 -> 128 channels on 16 x 32 (bf16), 256 -> 128 (fp16); a fused-up-sampling case for the 2x2 models
    return {BF: _fwd_case(2, 128, 16, 32, 128, BF, 1), FP: _fwd_case(2, 256, 16, 32, 128, FP, 2)}


@pytest.fixture(scope="module")
def wgrad_case():
    return _wgrad_case(2, 32, 32, 128, 32)          # K = 2 * 32 * 128 = 8192 pixels


def _rounded(t, dtype):
    return cb.rnd(t, dtype)


def _ok_at_half_c(name, y, c, dtype, model, **kw):
    r = cb.check(name, y, c["z"], c["a"], c["k"], dtype, model, c=cb.C / 2, **kw)
    print(f"  at C / 2: {r.msg}")
    return r.ok


@pytest.mark.parametrize("dtype", [BF, FP])
def test_correct_forward_results_pass_with_margin(fwd_cases, dtype):
    """the correctly rounded fp64 result, torch's fp32 result rounded once, and a strictly sequential fp32 chain in the kernels'
    (slab, tap) order rounded once: all inside the bound at HALF the constant (2x margin on C; a value one fp32 error puts on the
    other side of a rounding boundary is one ulp off M(Y), which the ulp term allows), and inside the RMS / bias limits"""
    c = fwd_cases[dtype]
    seq = cb.seq_chain_fwd(c["x"], c["w"], c["b"], 1, 1, 0)
    for name, y in (("fp64", _rounded(c["z"], dtype)), ("torch fp32", _rounded(c["z32"], dtype)), ("sequential fp32", _rounded(seq, dtype))):
        r = cb.check(name, y, c["z"], c["a"], c["k"], dtype, "round", y_cpu32=c["z32"])
        print(r.msg)
        assert r.ok and _ok_at_half_c(name, y, c, dtype, "round", y_cpu32=c["z32"]), r.msg
    # the constant itself: the raw fp32 errors (before the output rounding) within half of C * sqrt(K) * 2^-24 * A
    for name, y in (("torch fp32", c["z32"]), ("sequential fp32", seq)):
        ratio = float(((y - c["z"]).abs() / (cb.C * math.sqrt(c["k"]) * cb.U24 * c["a"])).max())
        print(f"{name} raw fp32 error / fp32 term: {ratio:.3g}")
        assert ratio <= 0.5, (name, ratio)


@pytest.mark.parametrize("dtype", [BF, FP])
def test_correct_two_rounding_epilogues_pass(fwd_cases, dtype):
    """accumulate (R(R(acc) + old)), ReLU, 2x2 sums (R(sum R(acc)), plain and accumulating) emulated on torch's fp32 result"""
    c = fwd_cases[dtype]
    g = torch.Generator().manual_seed(5)
    old = _rounded(torch.randn(c["z"].shape, generator=g).double(), dtype)
    y = cb.rnd(cb.rnd(c["z32"], dtype) + old, dtype)
    r = cb.check("acc2", y, c["z"], c["a"], c["k"], dtype, "acc2", old=old)
    print(r.msg)
    assert r.ok and _ok_at_half_c("acc2", y, c, dtype, "acc2", old=old), r.msg
    y = cb.rnd(c["z32"].clamp(min=0), dtype)
    r = cb.check("relu", y, c["z"], c["a"], c["k"], dtype, "round", relu=True)
    print(r.msg)
    assert r.ok and _ok_at_half_c("relu", y, c, dtype, "round", relu=True), r.msg
    old2 = _rounded(torch.randn(cb.sum2x2(c["z"]).shape, generator=g).double(), dtype)
    for model, o in (("pool2", None), ("pool2acc", old2)):
        s = cb.sum2x2(cb.rnd(c["z32"], dtype)) + (o if o is not None else 0)
        r = cb.check(model, cb.rnd(s, dtype), c["z"], c["a"], c["k"], dtype, model, old=o)
        print(r.msg)
        assert r.ok and _ok_at_half_c(model, cb.rnd(s, dtype), c, dtype, model, old=o), r.msg


def test_correct_weight_gradients_pass_with_margin(wgrad_case):
    c = wgrad_case
    seq = cb.seq_chain_wgrad(c["x"], c["dy"], 3, 1, 1, 0)
    for name, y in (("fp64 as fp32", c["z"].float()), ("torch fp32", c["z32"]), ("sequential fp32", seq)):
        r = cb.check(name, y, c["z"], c["a"], c["k"], torch.float32, "fp32")
        print(r.msg)
        assert r.ok and r.ratio <= 0.5, r.msg


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------
def _conv_part(x, w, ci_lo, ci_hi, taps=None):
    """fp64 conv restricted to input channels [ci_lo, ci_hi) (and to the listed (kh, kw) taps)"""
    wm = torch.zeros_like(w)
    if taps is None:
        wm[:, ci_lo:ci_hi] = w[:, ci_lo:ci_hi]
    else:
        for kh, kw in taps:
            wm[:, ci_lo:ci_hi, kh, kw] = w[:, ci_lo:ci_hi, kh, kw]
    return torch.nn.functional.conv2d(x, wm, None, padding=1)


def _fwd_faults(c, dtype):
    """-> {name: (y, model, old)}: every forward / epilogue fault, as the kernel would have stored it"""
    x, w, b, z = c["x"], c["w"], c["b"], c["z"]
    n, ci, h, w_ = x.shape
    out = {}
    # 1. one whole tap (all input channels) missing at one border pixel: the tap below the top-row pixel (0, 0, 0, 3)
    y = z.clone()
    y[0, :, 0, 3] -= _conv_part(x, w, 0, ci, [(2, 1)])[0, :, 0, 3]
    out["tap missing at a border pixel"] = (cb.rnd(y, dtype), "round", None)
    # 2. one halo pixel (all channels) read from the neighbouring image instead of zero padding: image 1's row -1, column 3 taken
    #    from image 0's last row; it enters the outputs (1, :, 0, 4 - kw) through the taps (0, kw)
    y = z.clone()
    for kw in range(3):
        y[1, :, 0, 4 - kw] += w[:, :, 0, kw] @ x[0, :, h - 1, 3]
    out["halo pixel from the neighbouring image"] = (cb.rnd(y, dtype), "round", None)
    # 3. accumulator rounded to the storage dtype after every 32-channel slab (bias as the starting value, as in the halo kernels)
    acc = b.view(1, -1, 1, 1).expand_as(z).clone()
    for s0 in range(0, ci, 32):
        acc = cb.rnd(acc + _conv_part(x, w, s0, s0 + 32), dtype)
    out["accumulator rounded per 32-channel slab"] = (acc, "round", None)
    # 4. truncating conversion (round toward zero)
    r = z.to(dtype)
    over = r.double().abs() > z.abs()
    r = torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r)
    out["truncating conversion"] = (r.double(), "round", None)
    # 5. bias added after rounding (R(R(acc) + bias))
    out["bias added after rounding"] = (cb.rnd(cb.rnd(z - b.view(1, -1, 1, 1), dtype) + b.view(1, -1, 1, 1), dtype), "round", None)
    # 6. accumulate epilogue reading `old` as 0 for one channel
    g = torch.Generator().manual_seed(6)
    old = cb.rnd(torch.randn(z.shape, generator=g).double(), dtype)
    y = cb.rnd(cb.rnd(z, dtype) + old, dtype)
    y[:, 5] = cb.rnd(z[:, 5], dtype)
    out["accumulate reads old = 0 for one channel"] = (y, "acc2", old)
    return out


@pytest.mark.parametrize("dtype", [BF, FP])
def test_seeded_forward_faults_fail(fwd_cases, dtype):
    c = fwd_cases[dtype]
    missed_old = []
    for name, (y, model, old) in _fwd_faults(c, dtype).items():
        r = cb.check(name, y, c["z"], c["a"], c["k"], dtype, model, old=old, y_cpu32=c["z32"] if old is None else c["z32"] + old)
        ref = c["z"] if old is None else c["z"] + old
        rel, passes_old = cb.old_criterion(y, ref, dtype)
        if passes_old:
            missed_old.append(name)
        print(f"[{dtype}] {r.msg} | old criterion rel {rel:.3g}: {'MISSED' if passes_old else 'caught'}")
        assert not r.ok, f"seeded fault not caught: {r.msg}"
    print(f"[{dtype}] faults today's criterion lets through: {missed_old}")


def test_seeded_weight_gradient_faults_fail(wgrad_case):
    c = wgrad_case
    x, dy, z = c["x"], c["dy"], c["z"]
    n, co, h, w_ = dy.shape
    op = c["op"]

    def without(mask):                     # the weight gradient with the pixels in `mask` (N, 1, H, W) left out
        return z - cb._op64(op, x, dy * mask, None, None)

    faults = {}
    m = torch.zeros(n, 1, h, w_, dtype=torch.float64); m[1, 0, 17, 40] = 1
    faults["one pixel missing (K = 8192)"] = without(m)
    m = torch.zeros(n, 1, h, w_, dtype=torch.float64); m[0, 0, 9, 64:128] = 1
    faults["one 64-pixel segment missing"] = without(m)
    # split reduction skipping the last of 3 splits (the generic kernel's chunk: ceil(ceil(M / splits) / 32) * 32 pixels)
    M, splits = n * h * w_, 3
    chunk = -(-(-(-M // splits)) // 32) * 32
    m = torch.zeros(M, dtype=torch.float64); m[(splits - 1) * chunk:] = 1
    faults["split reduction skips the last split"] = without(m.view(n, h, w_).unsqueeze(1))
    missed_old = []
    for name, y in faults.items():
        r = cb.check(name, y.float(), z, c["a"], c["k"], torch.float32, "fp32")
        rel, passes_old = cb.old_criterion(y.float(), z, BF)          # bf16 operands: today's test allows 2e-2
        if passes_old:
            missed_old.append(name)
        print(f"{r.msg} | old criterion rel {rel:.3g}: {'MISSED' if passes_old else 'caught'}")
        assert not r.ok, f"seeded fault not caught: {r.msg}"
    print(f"weight-gradient faults today's criterion lets through: {missed_old}")


@pytest.mark.parametrize("dtype", [BF, FP])
def test_statistics_row_missing_fails(fwd_cases, dtype):
    """fused BatchNorm statistics: correct fp32 partial rows (256 pixels each) pass, a missing row fails"""
    c = fwd_cases[dtype]
    y = cb.rnd(c["z"], dtype).permute(0, 2, 3, 1).reshape(-1, c["z"].shape[1])
    rows = y.shape[0] // 256
    yf = y.float().view(rows, 256, -1)
    part = torch.stack([yf.sum(1), (yf * yf).sum(1)], 1)           # fp32 partial rows
    r1, r2 = cb.stats_bound_check(part, y, rows)
    assert r1 <= 0.5 and r2 <= 0.5, (r1, r2)
    part[rows // 2] = 0
    r1, r2 = cb.stats_bound_check(part, y, rows)
    print(f"[{dtype}] one partial row missing: sum err/bound {r1:.3g}, sum-of-squares err/bound {r2:.3g}")
    assert max(r1, r2) > 1


def test_messages_name_the_worst_element(fwd_cases):
    c = fwd_cases[BF]
    y = cb.rnd(c["z"], BF)
    y[1, 7, 3, 9] += 1.0
    r = cb.check("poke", y, c["z"], c["a"], c["k"], BF, "round")
    assert not r.ok and r.nbad == 1 and r.worst == (1, 7, 3, 9) and "(1, 7, 3, 9)" in r.msg
