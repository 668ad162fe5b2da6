"""The kernels between the last convolution and the weight update (csrc/head.hip, csrc/loss_optim.hip, the pooling kernels of
csrc/elementwise.hip, mi355_bn_fold_bias) against the fp64 references of tests/head_ref.py, at the shapes where their grids,
loops and tie rules change: bit-equality where the case makes the arithmetic exact, a per-element bound derived from the kernel's
own chain elsewhere.  Operands sit in guarded buffers (tests/exact_harness.py): NaN around inputs, a sentinel around outputs,
outputs pre-filled with NaN; guards unchanged after the launch, and a second launch gives the same bytes.

The last test asserts from the ledger that every launcher and case ran and prints the worst error / bound per launcher and dtype.

What tests/test_gpu_ops.py did not reach, and the test here that does:
  AdamW judged relative to max |p|                      test_adamw: p, m, v per element, the bound on p a few 1e-4 of the update
  adamw_kernel's grid-stride trip (n > 524 288)         test_adamw[524547]
  sumsq_kernel's unrolled loop (n > 3 145 728)          test_sumsq_counts_every_element_once[3149731], test_grad_norm[3149731]
  bce_logits_kernel's atomic fold over workgroups       test_bce_logits[5000], [1049601]
  seg_counts_kernel on several workgroups per image     test_seg_counts[2049], [131849]
  ce_smooth_kernel's second row trip (B > 256)          test_ce_smooth[b257_c3-*]
  gscale, dz == NULL                                    test_bce_logits, test_ce_smooth (modes "gscale", "no_dz")
  adaptive_avgpool_fwd / _bwd                           test_adaptive_avgpool
  bn_fold_bias, fill_f32                                test_bn_fold_bias, test_fill
  the generic maxpool_bwd_kernel, ld > C                test_maxpool[*generic*] (every case pools out of slices, ld = C + 16)
  global_pool: HW < 4, ties between waves, ld > C       test_global_pool (hw1, hw3; plant_wave_ties; ld = C + 16)
  wide Linear: B = 17, I / 4 = 1025, O = 257, beta,     test_linear[b17_i4100_o257_relu1_wide] and the beta / NULL loop of every case
  NULL dx / dw / db / bias
  dropout by keep-rate only                             test_dropout: the mask bit for bit against head_ref.mix32"""
import math

import pytest
import torch

import conv_bounds as cb
import head_ref as hr
from exact_harness import F32, BF, FP, DTYPES, G, SENT, NAN, Buf, Flat, Vec, Ledger, _run, _bits, _dn  # noqa: F401
from gpu_util import DEV
from mi355.lib import lib, DTYPE_CODE

pytestmark = pytest.mark.gpu

_LEDGER = Ledger("MI355_HEAD")
RATIOS = {}                    # (launcher, dtype name) -> worst error / bound (0 for the exact cases)


def _note(launcher, dtype, ratio, *cases):
    _LEDGER.mark(launcher, dtype, *cases)
    key = (launcher, _dn(dtype))
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


class Raw(Flat):
    """a contiguous integer buffer of n elements between two sentinel pads: an output pre-filled with `fill`, or state (body)"""

    def __init__(self, n, dtype, fill, body=None):
        self.M, self.C, self.input, self.n = 1, n, False, n
        w = torch.full((n + 2 * G,), int(SENT), dtype=dtype)
        w[G:G + n] = fill if body is None else body
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + G * w.element_size()

    def guards_ok(self):
        a = self.t.clone()
        a[G:G + self.n] = self.init[G:G + self.n]
        return torch.equal(a, self.init)


def _launch(what, fn, bufs, outs, same=None):
    """launch; guards of every buffer; no NaN in the outputs; a second launch from the same start gives the same bytes in `same`
    (default: every output; sums folded by atomics are left out).  -> the outputs' bodies (fp64)"""
    fn()
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.guards_ok(), f"{what}: guards of buffer {i} changed"
    got = [b.body() for b in outs]
    for g in got:
        assert not torch.isnan(g).any(), f"{what}: {int(torch.isnan(g).sum())} elements never written (or NaN read)"
    same = outs if same is None else same
    first = [b.t.clone() for b in same]
    for b in bufs:
        b.reset()
    fn()
    torch.cuda.synchronize()
    for b, f in zip(same, first):
        assert torch.equal(_raw(b.t), _raw(f)), f"{what}: a second launch gives other bytes"
    return got


def _raw(t):
    return t if not t.is_floating_point() else _bits(t)


def _ok(what, ratio, idx):
    print(f"{what}: err/bound {ratio:.4g}" + (f" at {idx}" if ratio > 0 else ""))
    assert ratio <= 1, f"{what}: error / bound = {ratio:.4g} at flat index {idx}"
    return ratio


def _vec(t):
    return Vec(t.double().flatten())


def _dev(v, dtype=torch.float32):
    return torch.tensor(v, dtype=dtype, device=DEV)


# ---- max pooling: the generic, the 3x3/s2/p1 and the 2x2 kernels out of channel slices ---------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", hr.MAXPOOL_CASES, ids=lambda c: "k%ds%dp%d_%dx%d_%s" % c)
def test_maxpool(case, dtype):
    k, s, p, H, W, kern = case
    N, C, code = hr.POOL_N, hr.POOL_C, DTYPE_CODE[dtype]
    x, dy, old = hr.maxpool_case(k, s, p, H, W)
    yref, _ = hr.maxpool_ref(x, dy, k, s, p)
    Ho, Wo = yref.shape[2:]
    xb, yb = Buf(N * H * W, C, dtype, 2, hr.rows(x)), Buf(N * Ho * Wo, C, dtype, 2)
    assert xb.ld == C + 16
    _run(f"maxpool_fwd {case}", lambda: lib.mi355_maxpool_fwd(xb.ptr, xb.ld, yb.ptr, yb.ld, N, H, W, C, k, s, p, code), [xb, yb],
         {yb: hr.rows(yref)})
    _note("maxpool_fwd", dtype, 0.0, "k%ds%dp%d_%dx%d" % case[:5])
    dyb = Buf(N * Ho * Wo, C, dtype, 2, hr.rows(dy))
    for acc in (0, 1):
        dxb = Buf(N * H * W, C, dtype, 2, hr.rows(old), inout=True) if acc else Buf(N * H * W, C, dtype, 2)
        _, dxref = hr.maxpool_ref(x, dy, k, s, p, old if acc else None)
        _run(f"maxpool_bwd {case} acc={acc}",
             lambda: lib.mi355_maxpool_bwd(xb.ptr, xb.ld, dyb.ptr, dyb.ld, dxb.ptr, dxb.ld, N, H, W, C, k, s, p, acc, code),
             [xb, dyb, dxb], {dxb: hr.rows(dxref)})
        _note("maxpool_bwd", dtype, 0.0, "k%ds%dp%d_%dx%d" % case[:5], kern, f"acc{acc}")


# ---- global max / average pooling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", hr.GLOBAL_CASES, ids=lambda c: "n%d_hw%d_c%d" % c)
def test_global_pool(case, dtype):
    N, HW, C = case
    code, label = DTYPE_CODE[dtype], "n%d_hw%d_c%d" % case
    x, dy = hr.global_case(N, HW, C)
    pairs = hr.plant_wave_ties(x)
    xb, dyv = Buf(N * HW, C, dtype, 2, x.reshape(N * HW, C)), _vec(dy.flatten())
    assert xb.ld == C + 16
    # maximum: the value and the position of the FIRST maximum, whichever wave holds it
    yref, idx, dxref = hr.global_pool_ref(x, dy, 1)
    y, am, dxb = Flat(N * C), Raw(N * C, torch.int32, -7), Buf(N * HW, C, dtype, 2)
    _run(f"global_pool_fwd max {case}", lambda: lib.mi355_global_pool_fwd(xb.ptr, xb.ld, y.ptr, am.ptr, N, HW, C, 1, code), [xb, y, am],
         {y: yref, am: idx.double()})
    _run(f"global_pool_bwd max {case}", lambda: lib.mi355_global_pool_bwd(dyv.ptr, am.ptr, dxb.ptr, dxb.ld, N, HW, C, 1, code),
         [dyv, am, dxb], {dxb: dxref.reshape(N * HW, C)}, twice=False)       # (am is an input here: a reset would wipe it)
    _note("global_pool_fwd", dtype, 0.0, label, "max", *(["ties_all_wave_pairs"] if pairs == set(hr.WAVE_PAIRS) else []),
          *(["hw<4"] if HW < 4 else []))
    _note("global_pool_bwd", dtype, 0.0, label, "max")
    # mean: the sum is exact; the division is the only rounding (none for HW a power of two)
    yref, _, dxref = hr.global_pool_ref(x, dy, 0)
    y, dxb = Flat(N * C), Buf(N * HW, C, dtype, 2)
    fwd = lambda: lib.mi355_global_pool_fwd(xb.ptr, xb.ld, y.ptr, None, N, HW, C, 0, code)       # noqa: E731
    bwd = lambda: lib.mi355_global_pool_bwd(dyv.ptr, None, dxb.ptr, dxb.ld, N, HW, C, 0, code)   # noqa: E731
    if HW & (HW - 1) == 0:
        _run(f"global_pool_fwd avg {case}", fwd, [xb, y], {y: yref})
        _run(f"global_pool_bwd avg {case}", bwd, [dyv, dxb], {dxb: dxref.reshape(N * HW, C)})
        r1 = r2 = 0.0
    else:
        got, = _launch(f"global_pool_fwd avg {case}", fwd, [xb, y], [y])
        r1 = _ok(f"global_pool_fwd avg {label} {_dn(dtype)}", *hr.check_bounded(got, yref.flatten(), cb.ulp(yref.flatten(), F32)))
        got, = _launch(f"global_pool_bwd avg {case}", bwd, [dyv, dxb], [dxb])
        r2 = _ok(f"global_pool_bwd avg {label} {_dn(dtype)}", *hr.check_interval(got, dxref.reshape(N * HW, C), dtype))
    _note("global_pool_fwd", dtype, r1, label, "avg")
    _note("global_pool_bwd", dtype, r2, label, "avg")


# ---- adaptive average pooling + flatten ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", hr.ADAPTIVE_CASES, ids=lambda c: "%dx%d_to_%dx%d" % c[:4])
def test_adaptive_avgpool(case, dtype):
    H, W, OH, OW, exact = case
    N, C, code, label = hr.POOL_N, hr.POOL_C, DTYPE_CODE[dtype], "%dx%d_to_%dx%d" % case[:4]
    x, dy = hr.adaptive_case(H, W, OH, OW)
    yref, dxref, slack = hr.adaptive_avg_ref(x, dy, OH, OW)
    xb, y = Buf(N * H * W, C, dtype, 2, hr.rows(x)), Flat(N * C * OH * OW)
    dyv, dxb = _vec(dy.flatten()), Buf(N * H * W, C, dtype, 2)
    fwd = lambda: lib.mi355_adaptive_avgpool_fwd(xb.ptr, xb.ld, y.ptr, N, H, W, C, OH, OW, code)        # noqa: E731
    bwd = lambda: lib.mi355_adaptive_avgpool_bwd(dyv.ptr, dxb.ptr, dxb.ld, N, H, W, C, OH, OW, code)    # noqa: E731
    if exact:
        _run(f"adaptive_avgpool_fwd {case}", fwd, [xb, y], {y: yref})
        _run(f"adaptive_avgpool_bwd {case}", bwd, [dyv, dxb], {dxb: hr.rows(dxref)})
        r1 = r2 = 0.0
    else:
        got, = _launch(f"adaptive_avgpool_fwd {case}", fwd, [xb, y], [y])
        r1 = _ok(f"adaptive_avgpool_fwd {label} {_dn(dtype)}", *hr.check_bounded(got, yref.flatten(), cb.ulp(yref.flatten(), F32)))
        got, = _launch(f"adaptive_avgpool_bwd {case}", bwd, [dyv, dxb], [dxb])
        r2 = _ok(f"adaptive_avgpool_bwd {label} {_dn(dtype)}", *hr.check_interval(got, hr.rows(dxref), dtype, hr.rows(slack)))
    _note("adaptive_avgpool_fwd", dtype, r1, label)
    _note("adaptive_avgpool_bwd", dtype, r2, label)


# ---- dropout: the mask is a pure integer hash ----------------------------------------------------------------------------------------------
def test_dropout():
    n, seed = 1003, 0x1234_5678_9ABC
    g = hr._gen(n, 41)
    x, dy = torch.randn(n, generator=g).float(), torch.randn(n, generator=g).float()
    xv, dyv = _vec(x), _vec(dy)
    masks = {}
    for counter in (None, 7):
        cnt = None if counter is None else _dev([counter], torch.int32)
        for p in (0.0, 0.5, 0.75, 1.0, 0.3):
            mref, yref, scale = hr.dropout_ref(x, p, seed, counter)
            dxref = torch.where(mref.bool(), dy.double() * scale, torch.zeros(n, dtype=torch.float64))
            mk, y, dx = Raw(n, torch.uint8, 9), Flat(n), Flat(n)
            fwd = lambda: lib.mi355_dropout_fwd(xv.ptr, y.ptr, mk.ptr, n, p, seed, cnt)       # noqa: E731
            bwd = lambda: lib.mi355_dropout_bwd(dyv.ptr, mk.ptr, dx.ptr, n, p)                # noqa: E731
            what = f"dropout p={p} counter={counter}"
            if p != 0.3:
                _run(what + " fwd", fwd, [xv, mk, y], {y: yref})
                _ok(what + " mask", *hr.check_exact(mk.body(), mref))
                _run(what + " bwd", bwd, [dyv, mk, dx], {dx: dxref}, twice=False)      # (mk is an input here: a reset would wipe it)
                r1 = r2 = 0.0
            else:                                  # 1 / (1 - p) is not exact: the mask bit for bit, y and dx within one fp32 ulp
                got, _ = _launch(what + " fwd", fwd, [xv, mk, y], [y, mk])
                _ok(what + " mask", *hr.check_exact(mk.body(), mref))
                r1 = _ok(what + " y", *hr.check_bounded(got, yref, cb.ulp(yref, F32)))
                got, = _launch(what + " bwd", bwd, [dyv, dx], [dx])
                r2 = _ok(what + " dx", *hr.check_bounded(got, dxref, cb.ulp(dxref, F32)))
            masks[(counter, p)] = mref
            _note("dropout_fwd", F32, r1, f"p{p}", "counter" if counter else "no_counter")
            _note("dropout_bwd", F32, r2, f"p{p}")
    assert not torch.equal(masks[(None, 0.5)], masks[(7, 0.5)]) and not torch.equal(masks[(None, 0.3)], masks[(7, 0.3)])


# ---- fill, BatchNorm bias folding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257, 2048 * 256 + 5])
def test_fill(n):
    out = Flat(n)
    _run(f"fill_f32 n={n}", lambda: lib.mi355_fill_f32(out.ptr, -2.5, n), [out], {out: torch.full((n,), -2.5, dtype=torch.float64)})
    _note("fill_f32", F32, 0.0, f"n{n}")


@pytest.mark.parametrize("with_bias", [1, 0])
@pytest.mark.parametrize("C", [1, 128, 129])
def test_bn_fold_bias(C, with_bias):
    g = hr._gen(C, with_bias, 43)
    bias, shift = hr.dyadic(g, (C,), 0.5, 6), hr.dyadic(g, (C,), 0.25, 8)
    scale = torch.pow(2.0, torch.randint(-2, 3, (C,), generator=g).double()) * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
    bv, sv, hv, out = _vec(bias), _vec(scale), _vec(shift), Flat(C)
    ref = scale * (bias if with_bias else 0) + shift              # dyadic: a fused and an unfused multiply-add agree
    _run(f"bn_fold_bias C={C} bias={with_bias}", lambda: lib.mi355_bn_fold_bias(bv.ptr if with_bias else None, sv.ptr, hv.ptr, out.ptr, C),
         [bv, sv, hv, out], {out: ref})
    _note("bn_fold_bias", F32, 0.0, f"C{C}", "bias" if with_bias else "no_bias")


# ---- segmentation counters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [561, 2049, 64 * 2048 + 777])
def test_seg_counts(per):
    B = 3
    for is_logit in (0, 1):
        for thr in (0.5, 0.3):
            v, t = hr.seg_counts_case(B, per, is_logit, thr)
            ref, margin = hr.seg_counts_ref(v, t, is_logit, thr)
            assert margin >= 1e-3, f"an input sits {margin:.2e} from the threshold: the reference alone must decide every element"
            vv, tv, cnt = _vec(v.flatten()), _vec(t.flatten()), Flat(4 * B)
            _run(f"seg_counts per={per} logit={is_logit} thr={thr}", lambda: lib.mi355_seg_counts(vv.ptr, tv.ptr, cnt.ptr, B, per, is_logit, thr),
                 [vv, tv, cnt], {cnt: ref})
            _note("seg_counts", F32, 0.0, f"per{per}", f"logit{is_logit}", f"thr{thr}")


# ---- gradient norm -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hr.NORM_NS)
def test_sumsq_counts_every_element_once(n):
    """all ones: the folded partials are n exactly (every partial is an integer below 2^24), whichever loop took which element"""
    nb = lib.mi355_rowreduce_blocks(n)
    gv, part = _vec(torch.ones(n, dtype=torch.float64)), Flat(nb)
    got, = _launch(f"sumsq ones n={n}", lambda: lib.mi355_sumsq_partial(gv.ptr, part.ptr, n), [gv, part], [part])
    assert float(got.max()) < 2 ** 24
    _ok(f"sumsq ones n={n}", *hr.check_exact(got.sum().reshape(1), torch.tensor([float(n)], dtype=torch.float64)))
    _note("sumsq_partial", F32, 0.0, f"ones_n{n}")


@pytest.mark.parametrize("n", hr.NORM_NS)
def test_grad_norm(n):
    g = hr.norm_case(n)
    ss = float((g.double() ** 2).sum())
    nb = lib.mi355_rowreduce_blocks(n)
    assert nb == hr.rowreduce_blocks(n)
    if n == hr.NORM_NS[-1]:                      # the unrolled loop runs for threads i < 1000 only, and a 3-element remainder
        assert n // 4 - 3 * 256 * nb == 1000 and n % 4 == 3
    gv = _vec(g)
    for inv, dev, mx in ((1.0, None, 1.0), (0.25, 1.0 / 1024, 0.01)):
        devt = None if dev is None else _dev([dev])
        part, norm, coef, finf, step = Flat(nb), Flat(1), Flat(1), Flat(1), Raw(1, torch.int32, 0, torch.tensor([5], dtype=torch.int32))

        def fn():
            lib.mi355_sumsq_partial(gv.ptr, part.ptr, n)
            lib.mi355_clip_coef(part.ptr, nb, mx, inv, devt, norm.ptr, coef.ptr, finf.ptr, step.ptr)
        gn, gc, gf, gs = _launch(f"grad norm n={n}", fn, [gv, part, norm, coef, finf, step], [norm, coef, finf, step])
        nrm, bnd = hr.norm_ref(ss, inv, 1.0 if dev is None else dev)
        c, cbnd = hr.coef_ref(nrm, bnd, mx)
        r1 = _ok(f"norm n={n} inv={inv}", *hr.check_bounded(gn, [nrm], [bnd]))
        r2 = _ok(f"coef n={n} inv={inv}", *hr.check_bounded(gc, [c], [cbnd]))
        assert float(gf) == 0.0 and int(gs) == 6
        _note("sumsq_partial", F32, r1, f"n{n}")
        _note("clip_coef", F32, max(r1, r2), f"chain_n{n}", "dev_scale" if dev else "no_dev_scale")


@pytest.mark.parametrize("nblocks", hr.CLIP_NBLOCKS)
def test_clip_coef(nblocks):
    partial = hr.clip_case(nblocks)
    ss = float(partial.double().sum())
    pv = _vec(partial)
    for inv, dev, mx, aux in ((1.0, None, 1.0, True), (1.0, None, 0.0, True), (0.5, 0.125, -1.0, False), (0.5, 0.125, 2.5, True)):
        devt = None if dev is None else _dev([dev])
        norm, coef, finf, step = Flat(1), Flat(1), Flat(1), Raw(1, torch.int32, 0, torch.tensor([2], dtype=torch.int32))
        bufs = [pv, norm, coef] + ([finf, step] if aux else [])
        gn, gc = _launch(f"clip_coef nblocks={nblocks} max={mx}", lambda: lib.mi355_clip_coef(
            pv.ptr, nblocks, mx, inv, devt, norm.ptr, coef.ptr, finf.ptr if aux else None, step.ptr if aux else None), bufs, [norm, coef])
        nrm, bnd = hr.norm_ref(ss, inv, 1.0 if dev is None else dev)
        c, cbnd = hr.coef_ref(nrm, bnd, mx)
        r1 = _ok(f"clip_coef norm nblocks={nblocks}", *hr.check_bounded(gn, [nrm], [bnd]))
        r2 = _ok(f"clip_coef coef nblocks={nblocks} max={mx}", *hr.check_bounded(gc, [c], [cbnd]))
        if not mx > 0:
            assert float(gc) == 1.0
        if aux:
            assert float(finf.body()) == 0.0 and int(step.body()) == 3
        _note("clip_coef", F32, max(r1, r2), f"nblocks{nblocks}", f"max{mx}", "dev_scale" if dev else "no_dev_scale")
    # a non-finite sum: flagged, the step counter stays
    bad = partial.clone()
    bad[nblocks // 2] = math.inf
    bv, norm, coef, finf, step = _vec(bad), Flat(1), Flat(1), Flat(1), Raw(1, torch.int32, 0, torch.tensor([2], dtype=torch.int32))
    lib.mi355_clip_coef(bv.ptr, nblocks, 1.0, 1.0, None, norm.ptr, coef.ptr, finf.ptr, step.ptr)
    torch.cuda.synchronize()
    assert float(finf.body()) == 1.0 and int(step.body()) == 2 and all(b.guards_ok() for b in (bv, norm, coef, finf, step))
    _note("clip_coef", F32, 0.0, f"nblocks{nblocks}", "found_inf")


# ---- AdamW: p, m, v per element after every step, in the size of that element's update ----------------------------------------------------------
@pytest.mark.parametrize("n", hr.ADAMW_NS)
def test_adamw(n):
    p0, grads = hr.adamw_case(n)
    inv, dev = hr.ADAMW_SCALE
    hp = hr.ADAMW_HP
    lr, devt = _dev([hp["lr"]]), _dev([dev])
    nb = lib.mi355_rowreduce_blocks(n)
    state = [p0, torch.zeros(n), torch.zeros(n)]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for it, g in enumerate(grads):
        gv, part, norm, coef, finf = _vec(g), Flat(nb), Flat(1), Flat(1), Flat(1)
        step = Raw(1, torch.int32, 0, torch.tensor([it], dtype=torch.int32))
        pf, mf, vf = (Flat(n, body=s) for s in state)

        def fn():
            lib.mi355_sumsq_partial(gv.ptr, part.ptr, n)
            lib.mi355_clip_coef(part.ptr, nb, 1.0, inv, devt, norm.ptr, coef.ptr, finf.ptr, step.ptr)
            lib.mi355_adamw(pf.ptr, gv.ptr, mf.ptr, vf.ptr, n, lr, hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], coef.ptr, inv, devt,
                            finf.ptr, step.ptr)
        gp, gm, gvv, gc, gs = _launch(f"adamw n={n} step {it + 1}", fn, [gv, part, norm, coef, finf, step, pf, mf, vf], [pf, mf, vf, coef, step])
        assert int(gs) == it + 1
        if it == 0 and n > 1:
            assert float(gc) < 1.0                                   # the clip coefficient is in play
        # the fp64 step from the state the GPU started this step with, with the coefficient the GPU computed
        out, delta = hr.adamw_ref(state[0], state[1], state[2], g, it + 1, float(gc), inv, dev, **hp)
        for k, got in (("p", gp), ("m", gm), ("v", gvv)):
            worst[k] = max(worst[k], _ok(f"adamw n={n} step {it + 1} {k}", *hr.check_bounded(got, *out[k])))
        rel_update = float((out["p"][1] / delta.abs().clamp(min=1e-300)).median())
        print(f"adamw n={n} step {it + 1}: median bound on p / |update| = {rel_update:.2e}")
        assert rel_update < 2e-3                                     # an update wrong by 0.4 % cannot pass
        state = [gp.float(), gm.float(), gvv.float()]
    _note("adamw", F32, max(worst.values()), f"n{n}", "coef+inv_scale+dev_scale", *(["grid_stride"] if n > 2048 * 256 else []))
    # found_inf = 1: nothing moves
    g = grads[0]
    gv, one, step = _vec(g), _vec(torch.ones(1, dtype=torch.float64)), Raw(1, torch.int32, 0, torch.tensor([3], dtype=torch.int32))
    pf, mf, vf = (Flat(n, body=s) for s in state)
    _run(f"adamw n={n} found_inf", lambda: lib.mi355_adamw(pf.ptr, gv.ptr, mf.ptr, vf.ptr, n, lr, hp["beta1"], hp["beta2"], hp["eps"],
                                                        hp["wd"], None, inv, devt, one.ptr, step.ptr),
         [gv, one, step, pf, mf, vf], {pf: state[0].double(), mf: state[1].double(), vf: state[2].double()})
    _note("adamw", F32, 0.0, f"n{n}", "found_inf")


# ---- Linear: the one-wave-per-output kernels and the wide streaming kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("case", hr.LINEAR_CASES, ids=lambda c: "b%d_i%d_o%d_relu%d_%s" % c)
def test_linear(case):
    B, I, O, relu, kern = case
    label = "b%d_i%d_o%d" % case[:3]
    d = hr.linear_case(B, I, O)
    need = lib.mi355_linear_bwd_scratch(B, I, O)
    assert (need > 0) == (kern == "wide") and (kern == "wide") == (I % 4 == 0 and I * O >= 2 ** 20)
    xv, wv, bv, dyv = _vec(d["x"].flatten()), _vec(d["w"].flatten()), _vec(d["bias"]), _vec(d["dy"].flatten())
    y_gpu = None
    for with_bias in (0, 1):
        y = Flat(B * O)
        got, = _launch(f"linear_fwd {case} bias={with_bias}",
                       lambda: lib.mi355_linear_fwd(xv.ptr, wv.ptr, bv.ptr if with_bias else None, y.ptr, B, I, O, relu), [xv, wv, bv, y], [y])
        ref, bnd = hr.linear_fwd_ref(d["x"], d["w"], d["bias"] if with_bias else None, relu)
        r = _ok(f"linear_fwd {label} bias={with_bias}", *hr.check_bounded(got.reshape(B, O), ref, bnd))
        _note("linear_fwd", F32, r, label, kern, "bias" if with_bias else "no_bias")
        y_gpu = got.reshape(B, O).float()
    yv = _vec(y_gpu.flatten())
    for beta, skip in ((0.0, ""), (0.5, ""), (1.0, ""), (0.0, "dx"), (0.0, "dw"), (0.0, "db")):
        dx = None if skip == "dx" else Flat(B * I)
        dw = None if skip == "dw" else Flat(O * I, body=d["old_dw"].flatten() if beta else None)
        db = None if skip in ("dw", "db") else Flat(O, body=d["old_db"] if beta else None)      # (db comes out of the dW pass)
        scratch = Flat(need) if need and dx is not None else None
        ptr = lambda b: None if b is None else b.ptr      # noqa: E731
        outs = [b for b in (dx, dw, db) if b is not None]
        got = _launch(f"linear_bwd {case} beta={beta} without {skip or 'nothing'}",
                      lambda: lib.mi355_linear_bwd(xv.ptr, wv.ptr, yv.ptr, dyv.ptr, ptr(dx), ptr(dw), ptr(db), B, I, O, relu, beta, ptr(scratch)),
                      [xv, wv, yv, dyv] + outs + ([scratch] if scratch is not None else []), outs)
        ref = hr.linear_bwd_ref(d["x"], d["w"], y_gpu, d["dy"], relu, beta, d["old_dw"], d["old_db"])
        r = 0.0
        for name, buf, shape in (("dx", dx, (B, I)), ("dw", dw, (O, I)), ("db", db, (O,))):
            if buf is not None:
                r = max(r, _ok(f"linear_bwd {label} beta={beta} -{skip} {name}",
                               *hr.check_bounded(got[outs.index(buf)].reshape(shape), *ref[name])))
        _note("linear_bwd", F32, r, label, kern, f"beta{beta}", *([f"no_{skip}"] if skip else []))


# ---- the losses ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hr.BCE_NS)
def test_bce_logits(n):
    z, t = hr.bce_case(n)
    zv, tv = _vec(z), _vec(t)
    one_wg = (n + 1023) // 1024 == 1
    for mode in ("plain", "no_dz", "gscale"):
        gscale = 1024.0 if mode == "gscale" else 1.0
        gst = _dev([gscale]) if mode == "gscale" else None
        loss, dz = Flat(1), (None if mode == "no_dz" else Flat(n))
        outs = [loss] + ([dz] if dz is not None else [])
        got = _launch(f"bce_logits n={n} {mode}", lambda: lib.mi355_bce_logits(zv.ptr, tv.ptr, loss.ptr, None if dz is None else dz.ptr, gst, n),
                      [zv, tv] + outs, outs, same=outs if one_wg else outs[1:])      # (the workgroups meet in an atomic sum)
        (lref, lbnd), (dref, dbnd) = hr.bce_ref(z, t, gscale)
        r = _ok(f"bce_logits n={n} {mode} loss", *hr.check_bounded(got[0], [lref], [lbnd]))
        if dz is not None:
            r = max(r, _ok(f"bce_logits n={n} {mode} dz", *hr.check_bounded(got[1], dref, dbnd)))
        _note("bce_logits", F32, r, f"n{n}", mode, "one_workgroup" if one_wg else "atomic_fold")


@pytest.mark.parametrize("sm", [0.0, 0.1])
@pytest.mark.parametrize("case", hr.CE_CASES, ids=lambda c: "b%d_c%d" % c)
def test_ce_smooth(case, sm):
    B, C = case
    z, y = hr.ce_case(B, C)
    zv, yd = _vec(z.flatten()), y.to(DEV)
    for mode in ("plain", "no_dz", "gscale"):
        gscale = 1024.0 if mode == "gscale" else 1.0
        gst = _dev([gscale]) if mode == "gscale" else None
        loss, dz = Flat(1), (None if mode == "no_dz" else Flat(B * C))
        outs = [loss] + ([dz] if dz is not None else [])
        got = _launch(f"ce_smooth {case} sm={sm} {mode}",
                      lambda: lib.mi355_ce_smooth(zv.ptr, yd, loss.ptr, None if dz is None else dz.ptr, gst, B, C, sm), [zv] + outs, outs)
        (lref, lbnd), (dref, dbnd) = hr.ce_ref(z, y, sm, gscale)
        r = _ok(f"ce_smooth {case} sm={sm} {mode} loss", *hr.check_bounded(got[0], [lref], [lbnd]))
        if dz is not None:
            r = max(r, _ok(f"ce_smooth {case} sm={sm} {mode} dz", *hr.check_bounded(got[1].reshape(B, C), dref, dbnd)))
        _note("ce_smooth", F32, r, "b%d_c%d" % case, f"sm{sm}", mode, *(["second_row_trip"] if B > 256 else []))


# ---- the ledger ---------------------------------------------------------------------------------------------------------------------------------
_MP = ["k%ds%dp%d_%dx%d" % c[:5] for c in hr.MAXPOOL_CASES]
_GP = ["n%d_hw%d_c%d" % c for c in hr.GLOBAL_CASES]
_AP = ["%dx%d_to_%dx%d" % c[:4] for c in hr.ADAPTIVE_CASES]
_LIN = ["b%d_i%d_o%d" % c[:3] for c in hr.LINEAR_CASES]
EXPECTED = {      # launcher -> (its dtypes, the cases and branches that must have run in each)
    "maxpool_fwd": (DTYPES, _MP),
    "maxpool_bwd": (DTYPES, _MP + ["generic", "3s2", "2x2", "acc0", "acc1"]),
    "global_pool_fwd": (DTYPES, _GP + ["max", "avg", "ties_all_wave_pairs", "hw<4"]),
    "global_pool_bwd": (DTYPES, _GP + ["max", "avg"]),
    "adaptive_avgpool_fwd": (DTYPES, _AP),
    "adaptive_avgpool_bwd": (DTYPES, _AP),
    "dropout_fwd": ([F32], ["p0.0", "p0.5", "p0.75", "p1.0", "p0.3", "counter", "no_counter"]),
    "dropout_bwd": ([F32], ["p0.0", "p0.5", "p0.75", "p1.0", "p0.3"]),
    "fill_f32": ([F32], ["n0", "n1", "n257", f"n{2048 * 256 + 5}"]),
    "bn_fold_bias": ([F32], ["C1", "C128", "C129", "bias", "no_bias"]),
    "seg_counts": ([F32], ["per561", "per2049", f"per{64 * 2048 + 777}", "logit0", "logit1", "thr0.5", "thr0.3"]),
    "sumsq_partial": ([F32], [f"ones_n{n}" for n in hr.NORM_NS] + [f"n{n}" for n in hr.NORM_NS]),
    "clip_coef": ([F32], [f"nblocks{n}" for n in hr.CLIP_NBLOCKS] + [f"chain_n{n}" for n in hr.NORM_NS]
                  + ["max1.0", "max0.0", "max-1.0", "max2.5", "dev_scale", "no_dev_scale", "found_inf"]),
    "adamw": ([F32], [f"n{n}" for n in hr.ADAMW_NS] + ["coef+inv_scale+dev_scale", "grid_stride", "found_inf"]),
    "linear_fwd": ([F32], _LIN + ["small", "wide", "bias", "no_bias"]),
    "linear_bwd": ([F32], _LIN + ["small", "wide", "beta0.0", "beta0.5", "beta1.0", "no_dx", "no_dw", "no_db"]),
    "bce_logits": ([F32], [f"n{n}" for n in hr.BCE_NS] + ["plain", "no_dz", "gscale", "one_workgroup", "atomic_fold"]),
    "ce_smooth": ([F32], ["b%d_c%d" % c for c in hr.CE_CASES] + ["sm0.0", "sm0.1", "plain", "no_dz", "gscale", "second_row_trip"]),
}


def test_every_launcher_and_case_ran():
    """(runs last) every launcher, dtype and case of the list above is in the ledger; prints the ratio table"""
    seen = {}
    for r in _LEDGER.results:
        seen.setdefault((r["launcher"], r["dtype"]), set()).update(r["branches"])
    print("\n| launcher | dtype | cases | worst error / bound |")
    print("|---|---|---|---|")
    for (l, dt), br in sorted(seen.items()):
        print(f"| {l} | {dt} | {len(br)} | {RATIOS[(l, dt)]:.3f} |")
    for l, (dts, cases) in EXPECTED.items():
        for dt in dts:
            assert (l, _dn(dt)) in seen, f"{l} never ran in {_dn(dt)}"
            missing = [c for c in cases if c not in seen[(l, _dn(dt))]]
            assert not missing, f"{l} ({_dn(dt)}): cases that never ran: {missing}"
    assert all(v <= 1 for v in RATIOS.values())
