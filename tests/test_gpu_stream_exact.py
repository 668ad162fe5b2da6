"""-m gpu: the row-streaming BatchNorm passes (csrc/rowred.hpp, csrc/bn.hip) on EXACT data (tests/stream_exact.py): operands for
which every intermediate is exact in fp32 and every stored value in the storage type, so each result must equal the fp64 reference
bit for bit in fp32, bf16 and fp16 — a dropped, repeated or misplaced row shows, whatever the summation order.

Every tensor is a channel slice of a wider buffer with guard channels on both sides and rp guard rows behind row M - 1 (NaN in
inputs, a sentinel in outputs); outputs are pre-filled with NaN.  After each launch: guards unchanged, no NaN, bit-equal to the
reference, and a second launch gives the same bytes.  Switches that are read once per process run in child pytest processes; the
last test asserts that every (launcher, dtype) pair and every branch of the two skeletons ran, and prints the table.

The real-data chain at the end (reduce -> finalize -> apply on random operands) is held to bounds derived in the issue and
checked on the CPU (tests/test_stream_exact_cpu.py); the test prints the measured err / bound per dtype and shape."""
import pytest
import torch

import conv_bounds as cb
import stream_exact as se
from exact_harness import F32, BF, FP, DTYPES, G, SENT, NAN, Buf, Flat, Ledger, _run, _bits, _dn, _gen, _f, _fold  # noqa: F401
from gpu_util import DEV, lib, DTYPE_CODE, _fma32

pytestmark = pytest.mark.gpu

SWITCHES = {
    "wgs3": {"MI355_RR_WGS": "3", "MI355_RM_WGS": "3"},
    "rev": {"MI355_BN_APPLY_REV": "1", "MI355_RR_WGS": "3"},
    "nt": {"MI355_BN_REDUCE_NT": "1", "MI355_BN_APPLY_NT": "1"},
}
_LEDGER = Ledger("MI355_STREAM")
HERE, RESULTS, _mark = _LEDGER.here, _LEDGER.results, _LEDGER.mark      # rows dict(launcher, dtype, branches, n, switch)
CAP = 3 if HERE in ("wgs3", "rev") else 256            # grid cap of the fetch-batched reductions in this process
CAP_MAP = 3 if HERE == "wgs3" else 1024                # ... and of the fetch-batched elementwise passes

# channel counts of the 2-byte types (fp32: half of each) and the state each reaches
CH2 = [8, 40, 96, 64, 1024, 2048, 2560]


def _chans(dtype):
    return [c // 2 for c in CH2] if dtype == F32 else list(CH2)


def _edge_rows(rp, B, extra=()):
    """row counts without a whole batch and just around one, plus the case's extras"""
    ms = {1, rp - 1, rp * B - 1, rp * B, rp * B + 1} | set(extra)
    return sorted(m for m in ms if m >= 1)


def _fetch_branches(M, rp, B, grid):
    br = ["rowred.fetch.ring" if M >= rp * B else "rowred.fetch.tail_only"]
    if M >= (grid + 1) * rp * B:
        br.append("rowred.fetch.second_trip")
    if M >= rp * B and M % (rp * B):
        br.append("rowred.fetch.ring+tail")
    return br


def _cb(dtype, C):
    return ["colblocks>1"] if C // se.EPC[dtype] > 256 else []


# ---- column sums and forward statistics -------------------------------------------------------------------------------------------
def _colsum_case(dtype, C, M, twice=True):
    g = _gen(1, C, M)
    x = se.ints(g, (M, C), 4)
    se.assert_f32_sum_exact(x, 1.0, "colsum")
    rp = se.geometry(dtype, C)[3]
    xb = Buf(M, C, dtype, rp, x)
    nb = lib.mi355_rowreduce_blocks(M)
    part, out = Flat(nb * C), Flat(C, se.ints(g, (C,), 4))
    old = out.body()
    for acc in (0.0, 1.0):
        def fn():
            lib.mi355_colsum(xb.ptr, xb.ld, part.ptr, M, C, DTYPE_CODE[dtype])
            lib.mi355_colsum_finalize(part.ptr, nb, 1, C, out.ptr, acc)
        ref = se.ref_colsum(x)
        _run(f"colsum {_dn(dtype)} C={C} M={M} acc={acc}", fn, [xb, part, out], {out: ref + acc * old}, twice)
        assert torch.equal(_fold(part.body(), nb, 1, C)[0], ref)
        for b in (xb, part, out):
            b.reset()
    _mark("colsum", dtype, "rowred.plain.f32", *_cb(dtype, C))
    _mark("colsum_finalize", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_colsum(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C)
        print(f"\ncolsum {_dn(dtype)} C={C}: (epc, cp, tpr, rp, batch, sweep) = {geo}")
        for M in _edge_rows(geo[3], 1, (64 * 3 + 5, 2 * geo[3] + 3)):
            _colsum_case(dtype, C, M)


def _ulps32(got, ref64):
    """|got - ref| in fp32 ulps of the reference"""
    ref32 = ref64.float()
    u = cb.ulp(ref32.double(), F32)
    return float(((got - ref64).abs() / u).max())


def _stats_case(dtype, C, M, check_finalize):
    g = _gen(2, C, M)
    x = se.ints(g, (M, C), 4)
    se.assert_f32_sum_exact(x * x, 1.0, "bn_stats")
    rp = se.geometry(dtype, C)[3]
    xb = Buf(M, C, dtype, rp, x)
    nb = lib.mi355_rowreduce_blocks(M)
    part = Flat(nb * 2 * C)
    s, q = se.ref_stats(x)
    _run(f"bn_stats {_dn(dtype)} C={C} M={M}", lambda: lib.mi355_bn_stats(xb.ptr, part.ptr, M, C, xb.ld, DTYPE_CODE[dtype]), [xb, part], {})
    p = part.body()
    assert not torch.isnan(p).any()
    f = _fold(p, nb, 2, C)
    assert torch.equal(f[0], s) and torch.equal(f[1], q), "partial sums are not exact"
    _mark("bn_stats", dtype, "rowred.plain.f64", *_cb(dtype, C))
    if not check_finalize:
        return
    gamma = se.pow2(g, C, -2, 2)
    mean = s / M
    beta = -torch.sign(mean) * (1 + se.ints(g, (C,), 2, 0).abs())     # no cancellation in shift = beta - mean * scale (2-ulp bound)
    rm0, rv0 = se.ints(g, (C,), 2), se.ints(g, (C,), 2).abs() + 1
    mom, eps = 0.125, 1e-5
    ref = se.ref_finalize(s, q, M, gamma, beta, rm0, rv0, mom, eps)
    outs = {k: Flat(C) for k in ("scale", "shift", "mean", "invstd")}
    rmb, rvb = Flat(C, rm0), Flat(C, rv0)
    nbt = torch.full((3,), 41, dtype=torch.int64, device=DEV)
    lib.mi355_bn_finalize(part.ptr, nb, M, C, _f(gamma), _f(beta), rmb.ptr, rvb.ptr, nbt.data_ptr() + 8, mom, eps,
                          outs["scale"].ptr, outs["shift"].ptr, outs["mean"].ptr, outs["invstd"].ptr)
    torch.cuda.synchronize()
    assert nbt.tolist() == [41, 42, 41], nbt.tolist()
    for b in list(outs.values()) + [rmb, rvb, part]:
        assert b.guards_ok()
    got_mean = outs["mean"].body()
    assert torch.equal(got_mean, mean.float().double()), "mean is not float(s / M)"
    worst = 0.0
    for k, b in list(outs.items()) + [("rmean", rmb), ("rvar", rvb)]:
        if k == "mean":
            continue
        got = b.body()
        assert not torch.isnan(got).any(), k
        u = _ulps32(got, ref[k])
        worst = max(worst, u)
        assert u <= 2.0, f"bn_finalize {k}: {u:.2f} fp32 ulp from the fp64 evaluation (C={C}, M={M})"
    print(f"  bn_finalize C={C} M={M} nblocks={nb}: worst {worst:.2f} ulp")
    _mark("bn_finalize", dtype, "finalize<4,256>" if nb > 128 else "finalize<32,32>")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_stats_and_finalize(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C)
        print(f"\nbn_stats {_dn(dtype)} C={C}: {geo}")
        for M in _edge_rows(geo[3], 1, (64 * 3 + 5,)):
            _stats_case(dtype, C, M, M > 1)
    _stats_case(dtype, _chans(dtype)[3], 8192 + 64 * 5 + 7, True)          # more than 128 partial rows: the <4, 256> fold


# ---- forward apply ------------------------------------------------------------------------------------------------------------------
def _act_case(dtype, C, M, forms, twice=True):
    g = _gen(3, C, M)
    k = se.Consts(g, C)
    x, x2, res = se.ints(g, (M, C), 4), se.ints(g, (M, C), 4), se.ints(g, (M, C), 4)
    rp = se.geometry(dtype, C, 8)[3]
    xb, x2b, rb, yb = Buf(M, C, dtype, rp, x), Buf(M, C, dtype, rp, x2), Buf(M, C, dtype, rp, res), Buf(M, C, dtype, rp)
    sc, sh, sc2, sh2 = _f(k.scale), _f(k.shift), _f(k.scale2), _f(k.shift2)
    for h2, hr, act in forms:
        ref = se.ref_bn_act(x, k.scale, k.shift, x2 if h2 else None, k.scale2, k.shift2, res if hr else None, act)
        se.assert_storable(ref, BF, "bn_act result")
        se.assert_storable(ref, FP, "bn_act result")

        def fn():
            lib.mi355_bn_act(xb.ptr, xb.ld, sc, sh, x2b.ptr if h2 else None, x2b.ld, sc2 if h2 else None, sh2 if h2 else None,
                             rb.ptr if hr else None, rb.ld, yb.ptr, yb.ld, M, C, act, DTYPE_CODE[dtype])
        _run(f"bn_act {_dn(dtype)} C={C} M={M} H2={h2} HR={hr} act={act}", fn, [xb, x2b, rb, yb], {yb: ref}, twice)
        yb.reset()
    br = ["rowmap.fetch.batch" if M >= rp * 8 else "rowmap.fetch.tail_only"]
    if M > CAP_MAP * rp * 8:
        br.append("rowmap.fetch.second_trip")
    _mark("bn_act", dtype, "rowmap.fetch", *br, *_cb(dtype, C), n=len(forms))


ALL_FORMS = [(h2, hr, act) for h2 in (0, 1) for hr in (0, 1) for act in range(4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_act(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C, 8, CAP_MAP)
        print(f"\nbn_act {_dn(dtype)} C={C}: {geo}")
        for M in _edge_rows(geo[3], 8):
            _act_case(dtype, C, M, ALL_FORMS if M == geo[4] + 1 else [(1, 1, 3), (0, 0, 1), (0, 1, 1)])
    C = _chans(dtype)[4]
    _act_case(dtype, C, 16384 + 16 + 1, [(1, 1, 1), (0, 0, 0)])              # one row past a whole sweep of the capped grid + a batch


def _relu_plain_case(dtype, C, M):
    g = _gen(4, C, M)
    x = se.ints(g, (M, C), 4)
    rp = se.geometry(dtype, C)[3]
    xb, yb = Buf(M, C, dtype, rp, x), Buf(M, C, dtype, rp)
    _run(f"relu_fwd {_dn(dtype)} C={C} M={M}", lambda: lib.mi355_relu_fwd(xb.ptr, xb.ld, yb.ptr, yb.ld, M, C, DTYPE_CODE[dtype]),
         [xb, yb], {yb: x.clamp(min=0)})
    _mark("relu_fwd", dtype, "rowmap.plain", *_cb(dtype, C))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_rowmap_plain_loop(dtype):
    """no bn.hip launcher reaches rowmap_kernel's loop without fetch batches: mi355_relu_fwd (elementwise.hip) does"""
    for C in _chans(dtype):
        rp = se.geometry(dtype, C)[3]
        for M in _edge_rows(rp, 1, (3 * rp + 2,)):
            _relu_plain_case(dtype, C, M)


def _pool_shapes(dtype, C):
    """(N, H, W) of the window-ordered passes for a power-of-two tpr: one batch, and an odd N over several batches"""
    _, cp, tpr, rp, _, _ = se.geometry(dtype, C)
    Wm = 2 * rp
    return [(1, 2, Wm), (3, 4, 2 * Wm)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_act_pool2_and_windows(dtype):
    for C in _chans(dtype):
        rp = se.geometry(dtype, C)[3]
        for (N, H, W) in [(1, 2, 2), (3, 6, 10), (1, 2, 2 * rp + 2)]:
            M = N * H * W
            g = _gen(5, C, M)
            k = se.Consts(g, C)
            x, res = se.ints(g, (M, C), 4), se.ints(g, (M, C), 4)
            xb, rb, yb, pb = Buf(M, C, dtype, rp, x), Buf(M, C, dtype, rp, res), Buf(M, C, dtype, rp), Buf(M // 4, C, dtype, rp)
            sc, sh = _f(k.scale), _f(k.shift)
            for act in (0, 1):
                y = se.ref_bn_act(x, k.scale, k.shift, act=act)
                for withp in (True, False):
                    def fn():
                        lib.mi355_bn_act_pool2(xb.ptr, xb.ld, sc, sh, yb.ptr, yb.ld, pb.ptr if withp else None, pb.ld, N, H, W, C, act,
                                               DTYPE_CODE[dtype])
                    want = {yb: y, pb: se.ref_pool2(y, N, H, W)} if withp else {yb: y}
                    _run(f"bn_act_pool2 {_dn(dtype)} C={C} {N}x{H}x{W} act={act} p={withp}", fn, [xb, yb, pb], want)
                    if not withp:
                        assert torch.equal(_bits(pb.t), _bits(pb.init)), "p written without being given"
                    yb.reset(); pb.reset()
            for act in range(4):
                for withr in (True, False):
                    def fn():
                        lib.mi355_bn_act_windows(xb.ptr, xb.ld, sc, sh, rb.ptr if withr else None, rb.ld, yb.ptr, yb.ld, N, H, W, C, act,
                                                 DTYPE_CODE[dtype])
                    y = se.ref_bn_act(x, k.scale, k.shift, res=res if withr else None, act=act)
                    _run(f"bn_act_windows {_dn(dtype)} C={C} {N}x{H}x{W} act={act} res={withr}", fn, [xb, rb, yb], {yb: y})
                    yb.reset()
        _mark("bn_act_pool2", dtype)
        _mark("bn_act_windows", dtype)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
class BwdCase:
    """operands of one BatchNorm backward on exact data: buffers, constants, references of both mask sources"""

    def __init__(self, dtype, C, M, small=False, seed=6):
        g = _gen(seed, C, M)
        self.dtype, self.C, self.M, self.code = dtype, C, M, DTYPE_CODE[dtype]
        self.k = k = se.Consts(g, C, small)
        self.rp = rp = se.geometry(dtype, C, 4)[3]
        self.x, self.dy, self.y = se.ints(g, (M, C), k.xlim), se.ints(g, (M, C), 4), se.ints(g, (M, C), 4, 0.4)
        self.xb, self.dyb, self.yb = Buf(M, C, dtype, rp, self.x), Buf(M, C, dtype, rp, self.dy), Buf(M, C, dtype, rp, self.y)
        self.dev = {n: _f(getattr(k, n)) for n in ("mean", "invstd", "gamma", "mscale", "mshift")}
        self.gen = g

    def g(self, act, from_y):
        return se.masked(self.dy, se.relu_mask(act, self.y if from_y else None, self.x, self.k.mscale, self.k.mshift))


def _reduce_case(dtype, C, M, small=False, twice=True, forms=((0, False), (1, True), (1, False))):
    c = BwdCase(dtype, C, M, small)
    nb, rows = lib.mi355_rowreduce_blocks(M), lib.mi355_bn_bwd_reduce_rows(M)
    assert 1 <= rows <= min(nb, CAP)
    part, sums, dgam, dbet = Flat(nb * 2 * C), Flat(2 * C), Flat(C, se.ints(c.gen, (C,), 4)), Flat(C, se.ints(c.gen, (C,), 4))
    old_g, old_b = dgam.body(), dbet.body()
    d = c.dev
    for act, from_y in forms:
        g = c.g(act, from_y)
        t0, t1 = se.bwd_terms(g, c.x, c.k.mean, c.k.invstd)
        se.assert_f32_sum_exact(t0, 1.0, "sum g")
        se.assert_f32_sum_exact(t1, float(c.k.invstd.min()), "sum g * xhat")
        s0, s1 = t0.sum(0), t1.sum(0)
        for fold_rows, acc in ((nb, 0.0), (rows, 1.0)):
            def fn():
                lib.mi355_bn_bwd_reduce(c.dyb.ptr, c.dyb.ld, c.yb.ptr if from_y else None, c.yb.ld, c.xb.ptr, c.xb.ld, d["mean"], d["invstd"],
                                        None if from_y else d["mscale"], None if from_y else d["mshift"], part.ptr, M, C, act, c.code)
                lib.mi355_bn_bwd_finalize(part.ptr, fold_rows, C, sums.ptr, dgam.ptr, dbet.ptr, acc)
            what = f"bn_bwd_reduce {_dn(dtype)} C={C} M={M} act={act} y={from_y} fold {fold_rows} of {nb} rows acc={acc}"
            _run(what, fn, [c.xb, c.dyb, c.yb, part, sums, dgam, dbet],
                 {sums: torch.cat([s0, s1]), dgam: s1 + acc * old_g, dbet: s0 + acc * old_b}, twice)
            p = part.body()
            assert not torch.isnan(p).any(), f"{what}: partial rows left unwritten"
            assert float(p.reshape(nb, 2 * C)[rows:].abs().sum()) == 0.0, f"{what}: partial rows {rows}.. of {nb} are not zero"
            for b in (part, sums, dgam, dbet):
                b.reset()
    grid = rows
    _mark("bn_bwd_reduce", dtype, *_fetch_branches(M, c.rp, 4, grid), *_cb(dtype, C), n=len(forms))
    _mark("bn_bwd_finalize", dtype, "finalize<4,256>" if nb > 128 else "finalize<32,32>")
    return c


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_bwd_reduce(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C, 4, CAP)
        print(f"\nbn_bwd_reduce {_dn(dtype)} C={C}: {geo}")
        for M in _edge_rows(geo[3], 4, (3 * geo[4] + geo[3] + 1,)):
            _reduce_case(dtype, C, M)


def _apply_case(dtype, C, M, small=False, pow2_sums=False, twice=True, forms=None):
    c = BwdCase(dtype, C, M, small or pow2_sums, seed=7)
    k, d = c.k, c.dev
    nb = lib.mi355_rowreduce_blocks(M)
    if pow2_sums:
        assert M & (M - 1) == 0
        a0, a1 = se.ints(c.gen, (C,), 1, 0.3), se.ints(c.gen, (C,), 1, 0.3)
        s0, s1 = a0 * M, a1 * M
    else:
        s0 = s1 = torch.zeros(C, dtype=torch.float64)
    sums = _f(torch.cat([s0, s1]))
    old = se.ints(c.gen, (M, C), 4)
    dxb, drb, dpb, part = Buf(M, C, dtype, c.rp), Buf(M, C, dtype, c.rp), Buf(M, C, dtype, c.rp, old, inout=True), Flat(nb * C)
    # (act, mask from y, dres, dpost, post_acc, dbias partial)
    forms = forms or [(0, False, 0, 0, 0, 0), (1, True, 1, 0, 0, 1), (1, False, 0, 1, 0, 0), (1, False, 1, 1, 1, 1), (1, True, 0, 1, 1, 0)]
    for act, from_y, dres, dpost, pacc, dbias in forms:
        g = c.g(act, from_y)
        dx = se.ref_dx(g, c.x, k.gamma, k.mean, k.invstd, s0, s1, M)
        for dt in DTYPES:
            se.assert_storable(dx, dt, "dx")
        want = {dxb: dx}
        if dres:
            want[drb] = g
        if dpost:
            want[dpb] = se.ref_dpost(c.dy, old if pacc else None)
        if dbias:
            gi = (k.gamma * k.invstd).abs().min()
            se.assert_f32_sum_exact(dx, float(gi * (k.invstd.min() if pow2_sums else 1.0)), "column sums of dx")

        def fn():
            lib.mi355_bn_bwd_apply(c.dyb.ptr, c.dyb.ld, c.yb.ptr if from_y else None, c.yb.ld, c.xb.ptr, c.xb.ld, d["gamma"], d["mean"],
                                   d["invstd"], None if from_y else d["mscale"], None if from_y else d["mshift"], sums, dxb.ptr, dxb.ld,
                                   drb.ptr if dres else None, drb.ld, dpb.ptr if dpost else None, dpb.ld, pacc,
                                   part.ptr if dbias else None, M, C, act, c.code)
        what = f"bn_bwd_apply {_dn(dtype)} C={C} M={M} act={act} y={from_y} dres={dres} dpost={dpost} acc={pacc} dbias={dbias} pow2={pow2_sums}"
        _run(what, fn, [c.xb, c.dyb, c.yb, dxb, drb, dpb, part], want, twice)
        if dbias:
            p = part.body()
            assert not torch.isnan(p).any(), f"{what}: bias-gradient partial rows left unwritten"
            assert torch.equal(_fold(p, nb, 1, C)[0], dx.sum(0)), f"{what}: bias-gradient partials"
        for b in (dxb, drb, dpb, part):
            assert b in want or (b is part and dbias) or torch.equal(_bits(b.t), _bits(b.init)), f"{what}: an output that was not given was written"
            b.reset()
    grid = lib.mi355_bn_bwd_reduce_rows(M)
    _mark("bn_bwd_apply", dtype, *_fetch_branches(M, c.rp, 4, grid), *_cb(dtype, C), n=len(forms))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_bwd_apply(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C, 4, CAP)
        print(f"\nbn_bwd_apply {_dn(dtype)} C={C}: {geo}")
        for M in _edge_rows(geo[3], 4, (3 * geo[4] + geo[3] + 1,)):
            _apply_case(dtype, C, M)
        _apply_case(dtype, C, 2048 if geo[3] > 2 else 4096, pow2_sums=True)       # M a power of two, sums = M * a: the whole formula


def _post4_case(dtype, C, M, small=False, twice=True, nexs=(1, 2, 3, 4)):
    c = BwdCase(dtype, C, M, small, seed=8)
    k, d = c.k, c.dev
    rp = se.geometry(dtype, C, 2)[3]
    sums = _f(torch.zeros(2 * C, dtype=torch.float64))
    old = se.ints(c.gen, (M, C), 4)
    exs = [se.ints(c.gen, (M, C), 4) for _ in range(4)]
    exb = [Buf(M, C, dtype, rp, e) for e in exs]
    dxb, dpb = Buf(M, C, dtype, rp), Buf(M, C, dtype, rp, old, inout=True)
    zero = torch.zeros(C, dtype=torch.float64)
    for nex in nexs:
        act, from_y, pacc = 1, nex % 2 == 0, int(nex >= 3)
        g = c.g(act, from_y)
        want = {dxb: se.ref_dx(g, c.x, k.gamma, k.mean, k.invstd, zero, zero, M), dpb: se.ref_dpost(c.dy, old if pacc else None, exs[:nex])}
        for dt in DTYPES:
            se.assert_storable(want[dpb], dt, "dpost")
        ptrs = [exb[j].ptr if j < nex else None for j in range(4)]

        def fn():
            lib.mi355_bn_bwd_apply_post4(c.dyb.ptr, c.dyb.ld, c.yb.ptr if from_y else None, c.yb.ld, c.xb.ptr, c.xb.ld, d["gamma"], d["mean"],
                                         d["invstd"], None if from_y else d["mscale"], None if from_y else d["mshift"], sums, dxb.ptr, dxb.ld,
                                         dpb.ptr, dpb.ld, pacc, *ptrs, exb[0].ld, M, C, act, c.code)
        _run(f"bn_bwd_apply_post4 {_dn(dtype)} C={C} M={M} extras={nex} y={from_y} acc={pacc}", fn, [c.xb, c.dyb, c.yb, dxb, dpb] + exb, want, twice)
        dxb.reset(); dpb.reset()
    grid = lib.mi355_bn_bwd_reduce_rows(M)
    _mark("bn_bwd_apply_post4", dtype, *_fetch_branches(M, rp, 2, grid), *_cb(dtype, C), n=len(nexs))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_bwd_apply_post4(dtype):
    for C in _chans(dtype):
        geo = se.geometry(dtype, C, 2, CAP)
        print(f"\nbn_bwd_apply_post4 {_dn(dtype)} C={C}: {geo}")
        for i, M in enumerate(_edge_rows(geo[3], 2, (3 * geo[4] + geo[3] + 1,))):
            _post4_case(dtype, C, M, nexs=(1, 2, 3, 4) if i >= 3 else (1 + i, 4 - i))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_bwd_finalize_kernels(dtype):
    """both fold kernels (nblocks on both sides of 128) of mi355_bn_bwd_finalize and _at, acc 0 and 1, on exact partial rows; the
    fold has no storage type: the dtype only names the partial rows' origin in the coverage table"""
    for C in (4, 48, 100):
        for nblocks in (1, 33, 128, 129, 1024):
            for nq, q0, q1 in ((2, 0, 1), (5, 0, 2), (5, 3, 1)):
                g = _gen(9, C, nblocks, nq, q0, q1)
                p = se.ints(g, (nblocks, nq, C), 1000)
                part = Flat(nblocks * nq * C, p.reshape(-1))
                sums, dgam, dbet = Flat(2 * C), Flat(C, se.ints(g, (C,), 4)), Flat(C, se.ints(g, (C,), 4))
                og, ob = dgam.body(), dbet.body()
                s0, s1 = p[:, q0].sum(0), p[:, q1].sum(0)
                assert float(p.abs().sum(0).max()) < 2 ** 24
                for acc in (0.0, 1.0):
                    def fn():
                        if nq == 2:
                            lib.mi355_bn_bwd_finalize(part.ptr, nblocks, C, sums.ptr, dgam.ptr, dbet.ptr, acc)
                        else:
                            lib.mi355_bn_bwd_finalize_at(part.ptr, nblocks, nq, q0, q1, C, sums.ptr, dgam.ptr, dbet.ptr, acc)
                    _run(f"bn_bwd_finalize C={C} nblocks={nblocks} nq={nq} ({q0},{q1}) acc={acc}", fn, [part, sums, dgam, dbet],
                         {sums: torch.cat([s0, s1]), dgam: s1 + acc * og, dbet: s0 + acc * ob, part: p})
                    for b in (sums, dgam, dbet):
                        b.reset()
                _mark("bn_bwd_finalize" if nq == 2 else "bn_bwd_finalize_at", dtype, "finalize<4,256>" if nblocks > 128 else "finalize<32,32>")


def _pool_bwd_case(dtype, C, N, H, W, small=False, twice=True):
    M = N * H * W
    code = DTYPE_CODE[dtype]
    assert lib.mi355_bn_bwd_pool2_ok(H, W, C, code) == 1, (H, W, C)
    g = _gen(10, C, M)
    k = se.Consts(g, C, small)
    rp = se.geometry(dtype, C, 4)[3]
    x, dy, dp = se.ints(g, (M, C), k.xlim), se.ints(g, (M, C), 4), se.ints(g, (M // 4, C), 4)
    xb, dyb, dpb, dxb = Buf(M, C, dtype, rp, x), Buf(M, C, dtype, rp, dy), Buf(M // 4, C, dtype, rp, dp), Buf(M, C, dtype, rp)
    nb, rows = lib.mi355_rowreduce_blocks(M), lib.mi355_bn_bwd_reduce_pool2_rows(M)
    part, sums = Flat(nb * 2 * C), Flat(2 * C)
    d = {n: _f(getattr(k, n)) for n in ("mean", "invstd", "gamma", "mscale", "mshift")}
    zsums = _f(torch.zeros(2 * C, dtype=torch.float64))
    zero = torch.zeros(C, dtype=torch.float64)
    for with_dy in (True, False):
        gg = se.ref_pool_grad(x, k.mscale, k.mshift, dy if with_dy else None, dp, N, H, W, dtype)
        t0, t1 = se.bwd_terms(gg, x, k.mean, k.invstd)
        se.assert_f32_sum_exact(t0, 1.0, "sum g")
        se.assert_f32_sum_exact(t1, float(k.invstd.min()), "sum g * xhat")
        for fold_rows in (nb, rows):
            def fn():
                lib.mi355_bn_bwd_reduce_pool2(dyb.ptr if with_dy else None, dyb.ld, dpb.ptr, dpb.ld, xb.ptr, xb.ld, d["mean"], d["invstd"],
                                              d["mscale"], d["mshift"], part.ptr, N, H, W, C, code)
                lib.mi355_bn_bwd_finalize(part.ptr, fold_rows, C, sums.ptr, None, None, 0.0)
            what = f"bn_bwd_reduce_pool2 {_dn(dtype)} C={C} {N}x{H}x{W} dy={with_dy} fold {fold_rows} of {nb}"
            _run(what, fn, [xb, dyb, dpb, part, sums], {sums: torch.cat([t0.sum(0), t1.sum(0)])}, twice)
            p = part.body()
            assert not torch.isnan(p).any(), f"{what}: partial rows left unwritten"
            assert float(p.reshape(nb, 2 * C)[rows:].abs().sum()) == 0.0, f"{what}: partial rows {rows}.. are not zero"
            part.reset(); sums.reset()
        dx = se.ref_dx(gg, x, k.gamma, k.mean, k.invstd, zero, zero, M)
        for dt in DTYPES:
            se.assert_storable(dx, dt, "dx")

        def fn2():
            lib.mi355_bn_bwd_apply_pool2(dyb.ptr if with_dy else None, dyb.ld, dpb.ptr, dpb.ld, xb.ptr, xb.ld, d["gamma"], d["mean"], d["invstd"],
                                         d["mscale"], d["mshift"], zsums, dxb.ptr, dxb.ld, N, H, W, C, code)
        _run(f"bn_bwd_apply_pool2 {_dn(dtype)} C={C} {N}x{H}x{W} dy={with_dy}", fn2, [xb, dyb, dpb, dxb], {dxb: dx}, twice)
        dxb.reset()
    br = ["rowred.batch"] + (["rowred.batch.second_trip"] if M > rows * rp * 4 else [])
    _mark("bn_bwd_reduce_pool2", dtype, *br, n=2)
    _mark("bn_bwd_apply_pool2", dtype, *br, n=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn_bwd_pool2(dtype):
    code = DTYPE_CODE[dtype]
    for C in _chans(dtype):
        epc, cp, tpr, rp, _, _ = se.geometry(dtype, C, 4)
        if tpr & (tpr - 1) or cp > 256:
            assert lib.mi355_bn_bwd_pool2_ok(64, 512, C, code) == 0, f"C={C}: tpr = {tpr}, cp = {cp} is no geometry of the window-ordered pass"
            continue
        print(f"\nbn_bwd_pool2 {_dn(dtype)} C={C}: {se.geometry(dtype, C, 4, CAP)}")
        assert lib.mi355_bn_bwd_pool2_ok(2, 2 * rp, C, code) == 1
        assert lib.mi355_bn_bwd_pool2_ok(2, 6 * rp, C, code) == 0 and lib.mi355_bn_bwd_pool2_ok(3, 2 * rp, C, code) == 0
        if rp > 1:
            assert lib.mi355_bn_bwd_pool2_ok(2, rp, C, code) == 0
        for (N, H, W) in _pool_shapes(dtype, C):
            _pool_bwd_case(dtype, C, N, H, W)


# ---- one sweep of the capped grid and a ragged tail ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_rows_past_a_whole_sweep(dtype):
    """default grid caps: bn_bwd_reduce / _apply / _post4 at rp = 2 (nine trips of 256 workgroups) and at the benchmark's channel
    count (two sweeps + a batch + 37 rows), the pool-aware passes with an odd N over more than one sweep"""
    c_wide, c_bench = _chans(dtype)[4], _chans(dtype)[3]
    for C, M in ((c_wide, 16405), (c_bench, 2 * 32768 + 128 + 37)):
        geo = se.geometry(dtype, C, 4)
        print(f"\n{_dn(dtype)} C={C} M={M}: {geo}, grid {lib.mi355_bn_bwd_reduce_rows(M)}")
        assert M > geo[5] + geo[4] and M % geo[4]
        _reduce_case(dtype, C, M, small=True, forms=((1, False),) if C == c_wide else ((1, True), (1, False)))
        _apply_case(dtype, C, M, small=True, forms=[(1, False, 1, 1, 1, 1)] if C == c_wide else [(1, True, 1, 0, 0, 1), (1, False, 0, 1, 1, 0)])
    _post4_case(dtype, c_bench, 2 * 32768 + 128 + 37, small=True, nexs=(2, 3))
    N, H, W = 3, 172, 64
    assert N * H * W > se.geometry(dtype, c_bench, 4)[5]
    _pool_bwd_case(dtype, c_bench, N, H, W, small=True)


# ---- the real-data chain ------------------------------------------------------------------------------------------------------------
CHAIN_SHAPES = [(3, 96, 37, 41), (2, 64, 181, 181)]
CHAIN_RATIOS = {}


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_real_data_chain(dtype, shape):
    """reduce -> finalize -> apply on random real operands, act = 1 with the recomputed mask, against the derived bounds:
    |s - s64| <= C sqrt(K) 2^-24 sum|t| and |dx - d64| <= 1/2 ulp_T + 16 * 2^-24 |gi| (|g| + |k0| + |xhat k1|), dx judged from the
    kernel's own fp32 sums.  The float32 restatement on the CPU (same operands) reaches sums 0.006, dx 0.53 (fp32) / 1.000 (bf16, fp16: the
    half ulp of the storage type is the result's own rounding); the figures of the kernels are printed here and by the coverage test."""
    o = se.real_operands(shape, dtype, seed=sum(shape))
    M, C, code = o["M"], o["C"], DTYPE_CODE[dtype]
    rp = se.geometry(dtype, C, 4)[3]
    nb, rows = lib.mi355_rowreduce_blocks(M), lib.mi355_bn_bwd_reduce_rows(M)
    K = se.sums_chain_length(M, rows, rp)
    g, t0, t1 = se.chain_terms(o, _fma32)
    xb, dyb, dxb = Buf(M, C, dtype, rp, o["x"]), Buf(M, C, dtype, rp, o["dy"]), Buf(M, C, dtype, rp)
    part, sums = Flat(nb * 2 * C), Flat(2 * C)
    d = {n: o[n].to(DEV) for n in ("mean", "invstd", "gamma", "mscale", "mshift")}
    lib.mi355_bn_bwd_reduce(dyb.ptr, dyb.ld, None, 0, xb.ptr, xb.ld, d["mean"], d["invstd"], d["mscale"], d["mshift"], part.ptr, M, C, 1, code)
    lib.mi355_bn_bwd_finalize(part.ptr, rows, C, sums.ptr, None, None, 0.0)
    lib.mi355_bn_bwd_apply(dyb.ptr, dyb.ld, None, 0, xb.ptr, xb.ld, d["gamma"], d["mean"], d["invstd"], d["mscale"], d["mshift"], sums.ptr,
                           dxb.ptr, dxb.ld, None, 0, None, 0, 0, None, M, C, 1, code)
    torch.cuda.synchronize()
    for b in (xb, dyb, dxb, part, sums):
        assert b.guards_ok()
    s = sums.body()
    assert not torch.isnan(s).any()
    rs = max(float(((s[q * C:(q + 1) * C] - t.sum(0)).abs() / se.sums_bound(t, K, cb.C)).max()) for q, t in enumerate((t0, t1)))
    dx = dxb.body()
    assert not torch.isnan(dx).any()
    d64, mag = se.dx_parts(o, g, s[:C].float(), s[C:].float())
    rd = float(((dx - d64).abs() / se.dx_bound(d64, dx, mag, dtype, cb.ulp)).max())
    print(f"\nchain {_dn(dtype)} {shape}: K = {K}, sums err/bound {rs:.4f}, dx err/bound {rd:.4f}")
    CHAIN_RATIOS[(_dn(dtype), shape)] = (rs, rd)
    _mark("chain", dtype)
    assert rs <= 1.0, f"sums exceed the bound: {rs}"
    assert rd <= 1.0, f"dx exceeds the bound: {rd}"


# ---- child processes: switches read once per process ---------------------------------------------------------------------------------
def _walk(dtype, C, launcher):
    """every M from 1 to two sweeps + two batches of a 3-workgroup grid: operands and references are built once for the largest
    M and cut to the first M rows on the device; the rows behind M are NaN in the inputs and the sentinel in the outputs"""
    B = {"bn_bwd_reduce": 4, "bn_bwd_apply": 4, "bn_bwd_apply_post4": 2, "bn_act": 8, "colsum": 1}[launcher]
    _, _, _, rp, batch, sweep = se.geometry(dtype, C, B, 3)
    top = 2 * sweep + 2 * batch
    Mx = top + rp
    code = DTYPE_CODE[dtype]
    g = _gen(12, C, B)
    k = se.Consts(g, C)
    x, dy, e0 = se.ints(g, (Mx, C), 4), se.ints(g, (Mx, C), 4), se.ints(g, (Mx, C), 4)
    dv = {n: _f(getattr(k, n)) for n in ("mean", "invstd", "gamma", "mscale", "mshift", "scale", "shift")}
    gm = se.masked(dy, se.relu_mask(1, None, x, k.mscale, k.mshift))
    zero = torch.zeros(C, dtype=torch.float64)
    zs = _f(torch.zeros(2 * C, dtype=torch.float64))
    if launcher == "bn_bwd_reduce":
        t0, t1 = se.bwd_terms(gm, x, k.mean, k.invstd)
        se.assert_f32_sum_exact(t1[:top], float(k.invstd.min()))
        ref = torch.cat([t0.cumsum(0), t1.cumsum(0)], 1)
    elif launcher == "colsum":
        ref = x.cumsum(0)
    elif launcher == "bn_act":
        ref = se.ref_bn_act(x, k.scale, k.shift, act=1)
    else:
        ref = se.ref_dx(gm, x, k.gamma, k.mean, k.invstd, zero, zero, 1)
        refp = se.ref_dpost(dy, None, [e0])
    if launcher not in ("bn_bwd_reduce", "colsum"):
        se.assert_storable(ref, dtype)
    refd = ref.to(DEV)
    ins = {n: Buf(Mx, C, dtype, 0, t) for n, t in (("x", x), ("dy", dy), ("e0", e0))}
    full = {n: b.init.clone() for n, b in ins.items()}
    out, outp = Buf(Mx, C, dtype, 0), Buf(Mx, C, dtype, 0)
    if launcher == "bn_bwd_apply_post4":
        se.assert_storable(refp, dtype)
        refpd = refp.to(dtype).to(DEV)
    refo = ref.to(dtype).to(DEV) if launcher not in ("bn_bwd_reduce", "colsum") else None
    nq = 2 if launcher == "bn_bwd_reduce" else 1
    sums = Flat(nq * C)
    n = 0
    for M in range(1, top + 1):
        for nme, b in ins.items():                              # rows M .. are NaN
            b.t[M:M + rp] = NAN
        nb = lib.mi355_rowreduce_blocks(M)
        part = torch.full((nb * nq * C,), NAN, device=DEV)
        X, DY, E0 = ins["x"], ins["dy"], ins["e0"]
        if launcher == "bn_bwd_reduce":
            lib.mi355_bn_bwd_reduce(DY.ptr, DY.ld, None, 0, X.ptr, X.ld, dv["mean"], dv["invstd"], dv["mscale"], dv["mshift"], part, M, C, 1, code)
            lib.mi355_bn_bwd_finalize(part, lib.mi355_bn_bwd_reduce_rows(M), C, sums.ptr, None, None, 0.0)
        elif launcher == "colsum":
            lib.mi355_colsum(X.ptr, X.ld, part, M, C, code)
            lib.mi355_colsum_finalize(part, nb, 1, C, sums.ptr, 0.0)
        elif launcher == "bn_act":
            lib.mi355_bn_act(X.ptr, X.ld, dv["scale"], dv["shift"], None, 0, None, None, None, 0, out.ptr, out.ld, M, C, 1, code)
        elif launcher == "bn_bwd_apply":
            lib.mi355_bn_bwd_apply(DY.ptr, DY.ld, None, 0, X.ptr, X.ld, dv["gamma"], dv["mean"], dv["invstd"], dv["mscale"], dv["mshift"], zs,
                                   out.ptr, out.ld, None, 0, None, 0, 0, None, M, C, 1, code)
        else:
            lib.mi355_bn_bwd_apply_post4(DY.ptr, DY.ld, None, 0, X.ptr, X.ld, dv["gamma"], dv["mean"], dv["invstd"], dv["mscale"], dv["mshift"],
                                         zs, out.ptr, out.ld, outp.ptr, outp.ld, 0, E0.ptr, None, None, None, E0.ld, M, C, 1, code)
        n += 1
        what = f"{launcher} {_dn(dtype)} C={C} M={M} (batch {batch}, sweep {sweep})"
        if refo is None:
            got = sums.t[G:G + nq * C].double()
            assert torch.equal(got, refd[M - 1]), f"{what}: sums differ: {(got - refd[M - 1]).abs().max().item()}"
            assert sums.guards_ok()
        else:
            for o_, r_ in ((out, refo),) + (((outp, refpd),) if launcher == "bn_bwd_apply_post4" else ()):
                body = o_.t[:M, G:G + C]
                assert torch.equal(body, r_[:M]), f"{what}: {int((body != r_[:M]).sum())} elements differ (NaN = never written)"
                o_.t[:M, G:G + C] = o_.init[:M, G:G + C]
                assert torch.equal(_bits(o_.t), _bits(o_.init)), f"{what}: rows behind M - 1 or guard channels written"
        for nme, b in ins.items():                              # restore
            b.t[M:M + rp] = full[nme][M:M + rp]
    grid = 3
    br = set()
    for M in (1, batch, top):
        br |= set(_fetch_branches(M, rp, B, grid)) if launcher not in ("colsum", "bn_act") else set()
    if launcher == "colsum":
        br = {"rowred.plain.f32"}
    if launcher == "bn_act":
        br = {"rowmap.fetch", "rowmap.fetch.batch", "rowmap.fetch.tail_only", "rowmap.fetch.second_trip"}
    _mark(launcher, dtype, *br, n=n)
    print(f"  walked {launcher} {_dn(dtype)} C={C}: M = 1 .. {top} ({n} launches)")


def _walk_params():
    if HERE == "wgs3":
        ls = ("bn_bwd_reduce", "bn_bwd_apply", "bn_act", "colsum")
    elif HERE == "rev":
        ls = ("bn_bwd_apply", "bn_bwd_apply_post4")
    else:
        return []
    return [pytest.param(l, d, i, id=f"{l}-{_dn(d)}-C{_chans(d)[i]}") for l in ls for d in DTYPES for i in (2, 3)]


@pytest.mark.parametrize("launcher,dtype,ci", _walk_params())
def test_walk_every_row_count_on_three_workgroups(launcher, dtype, ci):
    _walk(dtype, _chans(dtype)[ci], launcher)


def _nt_params():
    return [pytest.param(d, id=_dn(d)) for d in DTYPES] if HERE == "nt" else []


@pytest.mark.parametrize("dtype", _nt_params())
def test_streaming_load_instantiations(dtype):
    """MI355_BN_REDUCE_NT=1 MI355_BN_APPLY_NT=1: the KEEP = false instantiations of every backward launcher, ragged and multi-trip"""
    C, M = _chans(dtype)[3], 2 * 32768 + 128 + 37
    _reduce_case(dtype, C, M, small=True, twice=False, forms=((1, True), (1, False)))
    _apply_case(dtype, C, M, small=True, twice=False, forms=[(1, True, 1, 0, 0, 1), (1, False, 0, 1, 1, 0)])
    _post4_case(dtype, C, M, small=True, twice=False, nexs=(2, 3))
    _pool_bwd_case(dtype, C, 3, 172, 64, small=True, twice=False)


def _children():
    return [pytest.param(k, id=k) for k in SWITCHES] if not HERE else []


_CHILD_ROWS, _CHILD_TIME = _LEDGER.child_rows, _LEDGER.child_time


@pytest.mark.parametrize("switch", _children())
def test_switched_paths_in_a_child_process(switch):
    _LEDGER.run_child(__file__, switch, SWITCHES[switch])


def _coverage():
    return [pytest.param("all", id="all")] if not HERE else []


LAUNCHERS = ["colsum", "colsum_finalize", "bn_stats", "bn_finalize", "bn_act", "bn_act_pool2", "bn_act_windows", "bn_bwd_reduce",
             "bn_bwd_finalize", "bn_bwd_finalize_at", "bn_bwd_apply", "bn_bwd_apply_post4", "bn_bwd_reduce_pool2", "bn_bwd_apply_pool2",
             "relu_fwd", "chain"]
BRANCHES = ["rowred.batch", "rowred.batch.second_trip", "rowred.fetch.ring", "rowred.fetch.second_trip", "rowred.fetch.ring+tail",
            "rowred.fetch.tail_only", "rowred.plain.f32", "rowred.plain.f64", "rowmap.fetch", "rowmap.fetch.second_trip", "rowmap.plain",
            "colblocks>1", "finalize<32,32>", "finalize<4,256>"]


@pytest.mark.parametrize("scope", _coverage())
def test_every_launcher_and_branch_ran(scope):
    """(runs last) every launcher in three dtypes, every branch of the two skeletons per dtype, the three children; prints the table"""
    rows = RESULTS + _CHILD_ROWS
    table, branches = {}, {}
    for r in rows:
        key = (r["launcher"], r["dtype"])
        t = table.setdefault(key, {"n": 0, "switch": set(), "br": set()})
        t["n"] += r["n"]
        t["switch"].add(r["switch"] or "default")
        t["br"] |= set(r["branches"])
        branches.setdefault(r["dtype"], set()).update(r["branches"])
    print("\n| launcher | dtype | launches checked | processes | branches |")
    print("|---|---|---|---|---|")
    for (l, dt), t in sorted(table.items()):
        print(f"| {l} | {dt} | {t['n']} | {' '.join(sorted(t['switch']))} | {' '.join(sorted(t['br']))} |")
    print("child processes:", ", ".join(f"{k} {v:.1f} s" for k, v in _CHILD_TIME.items()))
    for k, v in sorted(CHAIN_RATIOS.items()):
        print(f"chain {k}: sums err/bound {v[0]:.4f}, dx err/bound {v[1]:.4f}")
    for dt in ("float32", "bfloat16", "float16"):
        for l in LAUNCHERS:
            assert (l, dt) in table, f"{l} never ran in {dt}"
        missing = [b for b in BRANCHES if b not in branches.get(dt, set())]
        assert not missing, f"{dt}: skeleton branches that never ran: {missing}"
        for l, sw in (("bn_bwd_reduce", "wgs3"), ("bn_act", "wgs3"), ("colsum", "wgs3"), ("bn_bwd_apply", "wgs3"), ("bn_bwd_apply", "rev"),
                      ("bn_bwd_apply_post4", "rev"), ("bn_bwd_reduce", "nt"), ("bn_bwd_apply", "nt"), ("bn_bwd_apply_post4", "nt"),
                      ("bn_bwd_reduce_pool2", "nt"), ("bn_bwd_apply_pool2", "nt")):
            assert sw in table[(l, dt)]["switch"], f"{l} never ran under the {sw} switches in {dt}"


# a process collects only its own cases (an empty parameter set would show up as a skipped test)
_PARENT = ("test_colsum", "test_bn_stats_and_finalize", "test_bn_act", "test_rowmap_plain_loop", "test_bn_act_pool2_and_windows",
           "test_bn_bwd_reduce", "test_bn_bwd_apply", "test_bn_bwd_apply_post4", "test_bn_bwd_finalize_kernels", "test_bn_bwd_pool2",
           "test_rows_past_a_whole_sweep", "test_real_data_chain", "test_switched_paths_in_a_child_process",
           "test_every_launcher_and_branch_ran")
if HERE:
    for _t in _PARENT:
        del globals()[_t]
if HERE not in ("wgs3", "rev"):
    del globals()["test_walk_every_row_count_on_three_workgroups"]
if HERE != "nt":
    del globals()["test_streaming_load_instantiations"]
