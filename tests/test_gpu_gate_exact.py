"""-m gpu: the attention-gate kernels (csrc/gate.hip) on EXACT data (tests/gate_exact.py): operands for which every intermediate
is exact in fp32 and every stored value in the storage type, so each result must equal the fp64 reference bit for bit in fp32,
bf16 and fp16 — a row taken from its neighbour, a chunk weighted by another channel's constant or a z row read one off shows,
whatever the summation order.  The sigmoid of the gate multiply runs on its three exact classes (psi = 0, 1/2, 1) only.

Buffers, guards and the launch-and-compare step are those of tests/exact_harness.py.  The sums of the kernels that accumulate
in fp64 and round once per workgroup (rowdot_fwd, gate_psi_fwd, gate_mul_bwd) are held to the one derived bound
|sum_b partial_b - ref| <= 2^-24 sum_b |partial_b| (one rounding per partial row); every other result is bit-equal.  Switches
that are read once per process run in child pytest processes; the last test asserts that every launcher ran in every dtype and
every branch ran, and prints the table with each child's wall time."""
import pytest
import torch

import gate_exact as ge
import stream_exact as se
from exact_harness import F32, BF, FP, DTYPES, G, NAN, Buf, Flat, Vec, Ledger, _run, _bits, _dn, _f, _fold  # noqa: F401
from gpu_util import DEV, lib, DTYPE_CODE

pytestmark = pytest.mark.gpu

SWITCHES = {
    "wgs3": {"MI355_ROWDOT_WGS": "3", "MI355_RR_WGS": "3", "MI355_RM_WGS": "3"},
    "nt": {"MI355_BN_REDUCE_NT": "1", "MI355_BN_APPLY_NT": "1"},
}
_LEDGER = Ledger("MI355_GATE")
HERE, _mark = _LEDGER.here, _LEDGER.mark
WCAP = 3 if HERE == "wgs3" else 1024                   # grid cap of the moving-window kernels in this process
RCAP = 3 if HERE == "wgs3" else 1024                   # ... of rowdot_bwd (the gate BatchNorm passes: mi355_gate_bn_bwd_reduce_rows)
GR = 16                                                # guard rows behind row M - 1
U24 = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    ge.clear_cases()                                   # (the cached operands of the large cases: not held for the rest of the session)


def _epc(dtype):
    return se.EPC[dtype]


def _dev(cons, *names):
    return [_f(cons[n].reshape(-1)) for n in names]


def _fetch_branches(M, rp, B, grid):
    br = ["rowred.fetch.ring" if M >= rp * B else "rowred.fetch.tail_only"]
    if M >= (grid + 1) * rp * B:
        br.append("rowred.fetch.second_trip")
    if M >= rp * B and M % (rp * B):
        br.append("rowred.fetch.ring+tail")
    return br


def _cb(dtype, C):
    return ["colblocks>1"] if C // _epc(dtype) > 256 else []


def _check_pair(what, p, grid, s0, s1):
    """partial rows [nb, 2] (fp64 of the fp32 rows) of a kernel that sums in fp64 and rounds once per workgroup"""
    assert not torch.isnan(p).any(), f"{what}: {int(torch.isnan(p).any(1).sum())} partial rows left unwritten"
    for q, ref in ((0, s0), (1, s1)):
        tot, mag = float(p[:, q].sum()), float(p[:, q].abs().sum())
        assert abs(tot - float(ref)) <= U24 * mag, f"{what}: partial sum {q}: {tot!r} against {float(ref)!r}, bound {U24 * mag!r}"
    assert float(p[grid:].abs().sum()) == 0.0, f"{what}: partial rows {grid}.. of {p.shape[0]} are not zero"


# ---- the moving-window kernels: rowdot_fwd, gate_psi_fwd ------------------------------------------------------------------------------
def _window_case(launcher, dtype, C, M, two=True, twice=True, salt=0):
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    c = ge.rowdot_fwd_case(C, epc, M, salt) if launcher == "rowdot_fwd" else ge.gate_psi_case(C, epc, M, two, salt)
    nb = lib.mi355_rowreduce_blocks(M)
    zb, part = Flat(M), Flat(nb * 2)
    w, b = _dev(c.cons, "w", "b")
    if launcher == "rowdot_fwd":
        xb = Buf(M, C, dtype, GR, c.rows["x"])
        ins = [xb]

        def launch(p):
            lib.mi355_rowdot_fwd(xb.ptr, xb.ld, w, b, zb.ptr, p, M, C, 0, 1, code)
    else:
        gb = Buf(M, C, dtype, GR, c.rows["g1"])
        x1b = Buf(M, C, dtype, GR, c.rows["x1"]) if two else None
        ins = [gb] + ([x1b] if two else [])
        sg, shg, sx, shx = _dev(c.cons, "sg", "shg", "sx", "shx")

        def launch(p):
            lib.mi355_gate_psi_fwd(gb.ptr, gb.ld, x1b.ptr if two else None, x1b.ld if two else 0, sg, shg, sx if two else None,
                                   shx if two else None, w, b, zb.ptr, p, M, C, code)
    what = f"{launcher} {_dn(dtype)} C={C} M={M} two={two}"
    _run(what, lambda: launch(part.ptr), ins + [zb, part], {zb: c.outs["z"]}, twice)
    s = c.sums()
    _check_pair(what, part.body().reshape(nb, 2), min(nb, WCAP), s["s0"], s["s1"])
    zb.reset(); part.reset()
    _run(what + " partial=NULL", lambda: launch(None), ins + [zb, part], {zb: c.outs["z"]}, False)
    assert torch.equal(_bits(part.t), _bits(part.init)), f"{what}: partial written without being given"
    _mark(launcher, dtype, *ge.window_branches(dtype, C, M, WCAP), n=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_rowdot_fwd(dtype):
    code = DTYPE_CODE[dtype]
    for c2, ms in ge.WINDOW_CASES + ge.ROWDOT_WIDE:
        C = ge.chans(dtype, c2)
        for M in ms:
            print(f"\nrowdot_fwd {_dn(dtype)} C={C} M={M}: (cp, tpr, step, grid, sweep, nb) = {ge.window_geometry(dtype, C, M, WCAP)}")
            _window_case("rowdot_fwd", dtype, C, M)
    C = ge.chans(dtype, ge.ROWDOT_REJECTED)
    xb, zb, part = Buf(4, C, dtype, GR, torch.zeros(4, C, dtype=torch.float64)), Flat(4), Flat(2)
    w = torch.zeros(C, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported C"):
        lib.mi355_rowdot_fwd(xb.ptr, xb.ld, w, None, zb.ptr, part.ptr, 4, C, 0, 1, code)
    torch.cuda.synchronize()
    assert torch.equal(_bits(zb.t), _bits(zb.init)) and torch.equal(_bits(part.t), _bits(part.init)), "a rejected launch wrote"


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_gate_psi_fwd(dtype):
    code = DTYPE_CODE[dtype]
    for c2, ms in ge.WINDOW_CASES:
        C = ge.chans(dtype, c2)
        assert lib.mi355_gate_psi_fwd_ok(C, code) == 1
        for M in ms:
            for two in (True, False):
                _window_case("gate_psi_fwd", dtype, C, M, two)
    C = ge.chans(dtype, ge.PSI_REJECTED)
    assert lib.mi355_gate_psi_fwd_ok(C, code) == 0
    _mark("gate_psi_fwd_ok", dtype)
    gb, zb, part = Buf(4, C, dtype, GR, torch.zeros(4, C, dtype=torch.float64)), Flat(4), Flat(2)
    k = torch.zeros(C, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported C"):
        lib.mi355_gate_psi_fwd(gb.ptr, gb.ld, gb.ptr, gb.ld, k, k, k, k, k, None, zb.ptr, part.ptr, 4, C, code)
    torch.cuda.synchronize()
    assert torch.equal(_bits(zb.t), _bits(zb.init)) and torch.equal(_bits(part.t), _bits(part.init)), "a rejected launch wrote"


# ---- K > 1: channel planes of an [N][K][hw] map ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_channel_planes(dtype):
    """each of K = 3 planes is written in turn into one [N][K][hw] map; after plane k the others hold what they held before;
    the backward reads dz through the same map"""
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    K, hw, N, C = ge.PLANES["K"], ge.PLANES["hw"], ge.PLANES["N"], ge.chans(dtype, ge.PLANES["C"])
    M = N * hw
    idx = ge.plane_index(M, hw, K).to(DEV)
    nb = lib.mi355_rowreduce_blocks(M)
    zmap = Flat(N * K * hw)
    want = zmap.init.clone()
    dzs = torch.zeros(N * K * hw, dtype=torch.float64)
    bwd = [ge.rowdot_bwd_case(C, epc, M, k % 2, int(k > 0), 10 + k) for k in range(K)]
    for k in range(K):
        dzs[idx.cpu() + k * hw] = bwd[k].rows["dz"]
    dzmap = Vec(dzs)
    for k in range(K):
        c = ge.rowdot_fwd_case(C, epc, M, 10 + k)
        xb, part = Buf(M, C, dtype, GR, c.rows["x"]), Flat(nb * 2)
        w, b = _dev(c.cons, "w", "b")
        lib.mi355_rowdot_fwd(xb.ptr, xb.ld, w, b, zmap.ptr + 4 * k * hw, part.ptr, M, C, hw, K, code)
        torch.cuda.synchronize()
        want[G + idx + k * hw] = c.outs["z"].float().to(DEV)
        assert torch.equal(_bits(zmap.t), _bits(want)), f"rowdot_fwd {_dn(dtype)} plane {k}: the map differs (another plane or a guard written, or a wrong place)"
        assert xb.guards_ok() and part.guards_ok()
        s = c.sums()
        _check_pair(f"rowdot_fwd plane {k}", part.body().reshape(nb, 2), min(nb, WCAP), s["s0"], s["s1"])
    _mark("rowdot_fwd", dtype, "planes.fwd", n=K)
    rp = se.geometry(dtype, C, 4)[3]
    for k in range(K):
        c = bwd[k]
        acc = int(k > 0)
        xb = Buf(M, C, dtype, rp, c.rows["x"])
        dxb = Buf(M, C, dtype, rp, c.rows["old"], inout=True) if acc else Buf(M, C, dtype, rp)
        part = Flat(nb * 2 * C)
        w, = _dev(c.cons, "w")
        _run(f"rowdot_bwd {_dn(dtype)} plane {k}",
             lambda: lib.mi355_rowdot_bwd(dzmap.ptr + 4 * k * hw, xb.ptr, xb.ld, w, dxb.ptr, dxb.ld, part.ptr, M, C, k % 2, hw, K, acc, code),
             [dzmap, xb, dxb, part], {dxb: c.outs["dx"]})
        f, s = _fold(part.body(), nb, 2, C), c.sums()
        assert torch.equal(f[0], s["q0"]) and torch.equal(f[1], s["q1"]), f"rowdot_bwd plane {k}: partial sums"
    _mark("rowdot_bwd", dtype, "planes.bwd", n=K)


# ---- the reductions on the rowred skeleton --------------------------------------------------------------------------------------------
def _rowdot_bwd_case(dtype, C, M, mask, acc, twice=True):
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    c = ge.rowdot_bwd_case(C, epc, M, mask, acc)
    rp = se.geometry(dtype, C, 4)[3]
    nb = lib.mi355_rowreduce_blocks(M)
    dzb, xb = Vec(c.rows["dz"]), Buf(M, C, dtype, rp, c.rows["x"])
    dxb = Buf(M, C, dtype, rp, c.rows["old"], inout=True) if acc else Buf(M, C, dtype, rp)
    part = Flat(nb * 2 * C)
    w, = _dev(c.cons, "w")
    s = c.sums()
    what = f"rowdot_bwd {_dn(dtype)} C={C} M={M} mask={mask} acc={acc}"
    for with_dx in (True, False):
        _run(what + f" dx={with_dx}",
             lambda: lib.mi355_rowdot_bwd(dzb.ptr, xb.ptr, xb.ld, w, dxb.ptr if with_dx else None, dxb.ld, part.ptr, M, C, mask, 0, 1, acc, code),
             [dzb, xb, dxb, part], {dxb: c.outs["dx"]} if with_dx else {}, twice)
        p = part.body()
        assert not torch.isnan(p).any(), f"{what}: partial rows left unwritten"
        f = _fold(p, nb, 2, C)
        assert torch.equal(f[0], s["q0"]) and torch.equal(f[1], s["q1"]), f"{what}: partial sums are not exact"
        assert float(p.reshape(nb, -1)[RCAP:].abs().sum()) == 0.0, f"{what}: partial rows past the grid are not zero"
        if not with_dx:
            assert torch.equal(_bits(dxb.t), _bits(dxb.init)), f"{what}: dx written without being given"
        dxb.reset(); part.reset()
    _mark("rowdot_bwd", dtype, *_fetch_branches(M, rp, 4, min(nb, RCAP)), *_cb(dtype, C), n=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_rowdot_bwd(dtype):
    for c2 in ge.CH2:
        C = ge.chans(dtype, c2)
        print(f"\nrowdot_bwd {_dn(dtype)} C={C}: {se.geometry(dtype, C, 4, RCAP)}")
        for M in ge.rowred_rows(dtype, C):
            for mask, acc in ge.ROWDOT_BWD_FORMS:
                _rowdot_bwd_case(dtype, C, M, mask, acc)


def _gate_bn_case(dtype, C, M, two, small=False, pow2=False, twice=True):
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    c = ge.gate_bn_case(C, epc, M, two, small, pow2)
    rp = se.geometry(dtype, C, 4)[3]
    nb, rows = lib.mi355_rowreduce_blocks(M), lib.mi355_gate_bn_bwd_reduce_rows(M)
    assert 1 <= rows <= nb
    dzb, gb = Vec(c.rows["dz"]), Buf(M, C, dtype, rp, c.rows["g1"])
    x1b = Buf(M, C, dtype, rp, c.rows["x1"]) if two else None
    dgb, dxb, part = Buf(M, C, dtype, rp), Buf(M, C, dtype, rp), Flat(nb * 5 * C)
    sg, shg, mg, ig, w, gg, sums_g = _dev(c.cons, "sg", "shg", "mg", "ig", "w", "gg", "sums_g")
    sx, shx, mx, ix, gx, sums_x = _dev(c.cons, "sx", "shx", "mx", "ix", "gx", "sums_x") if two else [None] * 6
    xp, xl = (x1b.ptr, x1b.ld) if two else (None, 0)
    ins = [dzb, gb] + ([x1b] if two else [])
    what = f"gate_bn_bwd {_dn(dtype)} C={C} M={M} two={two} small={small} pow2={pow2}"
    _run(what + " reduce", lambda: lib.mi355_gate_bn_bwd_reduce(dzb.ptr, gb.ptr, gb.ld, xp, xl, sg, shg, mg, ig, sx, shx, mx, ix, w, part.ptr, M, C, code),
         ins + [part], {}, twice)
    p = part.body()
    assert not torch.isnan(p).any(), f"{what}: partial rows left unwritten"
    s = c.sums()
    for fold_rows in (nb, rows):
        f = _fold(p, fold_rows, 5, C)
        for q in range(5):
            assert torch.equal(f[q], s[f"q{q}"]), f"{what}: quantity {q} folded over {fold_rows} rows: max |diff| {float((f[q] - s[f'q{q}']).abs().max())}"
    assert float(p.reshape(nb, -1)[rows:].abs().sum()) == 0.0, f"{what}: partial rows {rows}.. of {nb} are not zero"
    if not two:
        assert float(_fold(p, nb, 5, C)[2].abs().sum()) == 0.0
    _mark("gate_bn_bwd_reduce", dtype, *_fetch_branches(M, rp, 4, rows), *_cb(dtype, C), "two" if two else "one")
    _mark("gate_bn_bwd_reduce_rows", dtype)
    want = {dgb: c.outs["dg"]}
    if two:
        want[dxb] = c.outs["dx"]
    _run(what + " apply", lambda: lib.mi355_gate_bn_bwd_apply(dzb.ptr, gb.ptr, gb.ld, xp, xl, sg, shg, mg, ig, sx, shx, mx, ix, w, gg, gx, sums_g, sums_x,
                                                               dgb.ptr, dgb.ld, dxb.ptr, dxb.ld, M, C, code),
         ins + [dgb, dxb], want, twice)
    if not two:
        assert torch.equal(_bits(dxb.t), _bits(dxb.init)), f"{what}: dx1 written in the one-operand form"
    _mark("gate_bn_bwd_apply", dtype, *_fetch_branches(M, rp, 4, rows), *_cb(dtype, C), "two" if two else "one")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_gate_bn_bwd(dtype):
    for c2 in ge.CH2:
        C = ge.chans(dtype, c2)
        print(f"\ngate_bn_bwd {_dn(dtype)} C={C}: {se.geometry(dtype, C, 4, 3 if HERE == 'wgs3' else 512)}")
        for M in ge.rowred_rows(dtype, C):
            for two in (True, False):
                _gate_bn_case(dtype, C, M, two)
        for two in (True, False):
            _gate_bn_case(dtype, C, ge.pow2_rows(dtype, C), two, True, True)          # M a power of two, sums = M * k: the whole formula


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_reductions_past_a_whole_sweep(dtype):
    """default grid caps: several trips of the fetch ring of rowdot_bwd (1024 workgroups) and the gate BatchNorm passes (512)"""
    for i, M in ge.BIG_ROWS:
        C = ge.chans(dtype, ge.CH2[i])
        print(f"\n{_dn(dtype)} C={C} M={M}: {se.geometry(dtype, C, 4, 512)}, grid {lib.mi355_gate_bn_bwd_reduce_rows(M)}")
        _rowdot_bwd_case(dtype, C, M, 1, 1)
        for two in (True, False):
            _gate_bn_case(dtype, C, M, two, True)


# ---- x * sigmoid(bn1(z)) on the three exact classes -----------------------------------------------------------------------------------
def _mul_fwd_case(dtype, C, M):
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    c = ge.gate_mul_fwd_case(C, epc, M)
    rp = se.geometry(dtype, C)[3]
    xb, zb, yb = Buf(M, C, dtype, rp, c.rows["x"]), Vec(c.rows["z"]), Buf(M, C, dtype, rp)
    sc, sh = _dev(c.cons, "scale", "shift")
    _run(f"gate_mul_fwd {_dn(dtype)} C={C} M={M}", lambda: lib.mi355_gate_mul_fwd(xb.ptr, xb.ld, zb.ptr, sc, sh, yb.ptr, yb.ld, M, C, code),
         [xb, zb, yb], {yb: c.outs["y"]})
    _mark("gate_mul_fwd", dtype, "rowmap.plain", *_cb(dtype, C))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_gate_mul_fwd(dtype):
    for c2 in ge.CH2:
        C = ge.chans(dtype, c2)
        for M in ge.rowmap_rows(dtype, C):
            _mul_fwd_case(dtype, C, M)


def _mul_bwd_case(dtype, C, M, acc):
    code, epc = DTYPE_CODE[dtype], _epc(dtype)
    c = ge.gate_mul_bwd_case(C, epc, M, acc)
    nb = lib.mi355_rowreduce_blocks(M)
    dyb, xb, zb = Buf(M, C, dtype, GR, c.rows["dy"]), Buf(M, C, dtype, GR, c.rows["x"]), Vec(c.rows["z"])
    dxb = Buf(M, C, dtype, GR, c.rows["old"], inout=True) if acc else Buf(M, C, dtype, GR)
    dzn, part = Flat(M), Flat(nb * 2)
    sc, sh, mu, isd = _dev(c.cons, "scale", "shift", "mean", "invstd")
    what = f"gate_mul_bwd {_dn(dtype)} C={C} M={M} acc={acc}"
    _run(what, lambda: lib.mi355_gate_mul_bwd(dyb.ptr, dyb.ld, xb.ptr, xb.ld, zb.ptr, sc, sh, mu, isd, dxb.ptr, dxb.ld, acc, dzn.ptr, part.ptr, M, C, code),
         [dyb, xb, zb, dxb, dzn, part], {dxb: c.outs["dx"], dzn: c.outs["dzn"]})
    s = c.sums()
    _check_pair(what, part.body().reshape(nb, 2), nb, s["s0"], s["s1"])
    _mark("gate_mul_bwd", dtype, *ge.mul_bwd_branches(dtype, C, M, acc))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_gate_mul_bwd(dtype):
    for c2, ms in ge.MUL_BWD_CASES:
        for M in ms:
            for acc in (0, 1):
                _mul_bwd_case(dtype, ge.chans(dtype, c2), M, acc)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_bn1_bwd_apply(dtype):
    """fp32 only: the dtype names the coverage table's column"""
    for M, pow2 in [(m, False) for m in ge.BN1_ROWS] + [(2 ** 20, True)]:
        c = ge.bn1_case(M, pow2)
        dznb, zb, dzb = Vec(c.rows["dzn"]), Vec(c.rows["z"]), Flat(M)
        gam, mu, isd, sums = _dev(c.cons, "gamma", "mean", "invstd", "sums")
        _run(f"bn1_bwd_apply M={M} pow2={pow2}", lambda: lib.mi355_bn1_bwd_apply(dznb.ptr, zb.ptr, gam, mu, isd, sums, dzb.ptr, M),
             [dznb, zb, dzb], {dzb: c.outs["dz"]})
        _mark("bn1_bwd_apply", dtype, *(["bn1.second_trip"] if M > 4096 * 256 else []))


# ---- child processes: switches read once per process ---------------------------------------------------------------------------------
def _walk(dtype, C, launcher):
    """every M from 1 to ge.walk_top on three workgroups: operands and references are built once for the largest M and cut to the
    first M rows on the device; the rows behind M are NaN in the inputs and keep their sentinel in the outputs"""
    code = DTYPE_CODE[dtype]
    c = ge.walk_case(dtype, C, launcher)
    top = c.M
    window = launcher in ("rowdot_fwd", "gate_psi_fwd")
    bufs = {k: (Buf(top, C, dtype, GR, v) if v.dim() == 2 else Vec(v)) for k, v in c.rows.items()}
    d = {k: _f(v.reshape(-1)) for k, v in c.cons.items()}
    outs = {k: (Buf(top, C, dtype, GR) if v.dim() == 2 else Flat(top)) for k, v in c.outs.items()}
    if launcher == "gate_bn_bwd_reduce":
        outs = {}
    refs = {k: (v.to(dtype) if v.dim() == 2 else v.float()).to(DEV) for k, v in c.outs.items() if k in outs}
    pre = {k: v.to(DEV) for k, v in c.prefix_sums().items()}
    nq = {"rowdot_fwd": 2, "gate_psi_fwd": 2, "rowdot_bwd": 2, "gate_bn_bwd_reduce": 5}.get(launcher, 0)
    pc = 1 if window else C
    n = 0
    for M in range(1, top + 1):
        for b in bufs.values():                                 # rows M .. are NaN
            if isinstance(b, Vec):
                b.t[G + M:G + M + GR] = NAN
            else:
                b.t[M:M + GR] = NAN
        nb = lib.mi355_rowreduce_blocks(M)
        part = torch.full((max(nb * nq * pc, 1),), NAN, device=DEV)
        B = bufs
        if launcher == "rowdot_fwd":
            lib.mi355_rowdot_fwd(B["x"].ptr, B["x"].ld, d["w"], d["b"], outs["z"].ptr, part, M, C, 0, 1, code)
        elif launcher == "gate_psi_fwd":
            lib.mi355_gate_psi_fwd(B["g1"].ptr, B["g1"].ld, B["x1"].ptr, B["x1"].ld, d["sg"], d["shg"], d["sx"], d["shx"], d["w"], d["b"],
                                   outs["z"].ptr, part, M, C, code)
        elif launcher == "rowdot_bwd":
            lib.mi355_rowdot_bwd(B["dz"].ptr, B["x"].ptr, B["x"].ld, d["w"], outs["dx"].ptr, outs["dx"].ld, part, M, C, 1, 0, 1, 0, code)
        elif launcher == "gate_bn_bwd_reduce":
            lib.mi355_gate_bn_bwd_reduce(B["dz"].ptr, B["g1"].ptr, B["g1"].ld, B["x1"].ptr, B["x1"].ld, d["sg"], d["shg"], d["mg"], d["ig"],
                                         d["sx"], d["shx"], d["mx"], d["ix"], d["w"], part, M, C, code)
        elif launcher == "gate_bn_bwd_apply":
            lib.mi355_gate_bn_bwd_apply(B["dz"].ptr, B["g1"].ptr, B["g1"].ld, B["x1"].ptr, B["x1"].ld, d["sg"], d["shg"], d["mg"], d["ig"],
                                        d["sx"], d["shx"], d["mx"], d["ix"], d["w"], d["gg"], d["gx"], d["sums_g"], d["sums_x"],
                                        outs["dg"].ptr, outs["dg"].ld, outs["dx"].ptr, outs["dx"].ld, M, C, code)
        else:
            lib.mi355_gate_mul_fwd(B["x"].ptr, B["x"].ld, B["z"].ptr, d["scale"], d["shift"], outs["y"].ptr, outs["y"].ld, M, C, code)
        n += 1
        what = f"{launcher} {_dn(dtype)} C={C} M={M} of {top}"
        for k, o in outs.items():
            body = o.t[:M, G:G + C] if isinstance(o, Buf) and not isinstance(o, Flat) else o.t[G:G + M]
            assert torch.equal(body, refs[k][:M]), f"{what}: {k}: {int((body != refs[k][:M]).sum())} elements differ (NaN = never written)"
            if isinstance(o, Flat):
                o.t[G:G + M] = o.init[G:G + M]
            else:
                o.t[:M, G:G + C] = o.init[:M, G:G + C]
            assert torch.equal(_bits(o.t), _bits(o.init)), f"{what}: {k}: rows behind M - 1 or guard channels written"
        if nq:
            p = part.view(nb, nq, pc).double()
            assert not torch.isnan(p).any(), f"{what}: partial rows left unwritten"
            assert float(p[3:].abs().sum()) == 0.0, f"{what}: partial rows past the three workgroups are not zero"
            names = ("s0", "s1") if window else tuple(f"q{q}" for q in range(nq))
            for q, name in enumerate(names):
                ref = pre[name][M - 1].reshape(-1)
                if window:
                    tot, mag = p[:, q].sum(0), p[:, q].abs().sum(0)
                    assert bool(((tot - ref).abs() <= U24 * mag).all()), f"{what}: partial sum {q}: {tot.tolist()} against {ref.tolist()}"
                else:
                    assert torch.equal(p[:, q].sum(0), ref), f"{what}: quantity {q}: max |diff| {float((p[:, q].sum(0) - ref).abs().max())}"
        for b in bufs.values():                                 # restore
            b.reset()
    rp = se.geometry(dtype, C, 4)[3]
    br = set()
    for M in range(1, top + 1):
        if window:
            br |= set(ge.window_branches(dtype, C, M, 3))
        elif launcher == "gate_mul_fwd":
            br.add("rowmap.plain")
        else:
            br |= set(_fetch_branches(M, rp, 4, 3))
    _mark(launcher, dtype, *br, n=n)
    print(f"  walked {launcher} {_dn(dtype)} C={C}: M = 1 .. {top} ({n} launches)")


def _walk_params():
    if HERE != "wgs3":
        return []
    return [pytest.param(l, d, c2, id=f"{l}-{_dn(d)}-C{ge.chans(d, c2)}") for l in ge.WALK_LAUNCHERS for d in DTYPES for c2 in ge.WALK_C2]


@pytest.mark.parametrize("launcher,dtype,c2", _walk_params())
def test_walk_every_row_count_on_three_workgroups(launcher, dtype, c2):
    _walk(dtype, ge.chans(dtype, c2), launcher)


def _nt_params():
    return [pytest.param(d, id=_dn(d)) for d in DTYPES] if HERE == "nt" else []


@pytest.mark.parametrize("dtype", _nt_params())
def test_streaming_load_instantiations(dtype):
    """MI355_BN_REDUCE_NT=1 MI355_BN_APPLY_NT=1: the KEEP = false instantiations of both gate BatchNorm passes, both forms, ragged
    and multi-trip"""
    i, M = ge.BIG_ROWS[1]
    for two in (True, False):
        _gate_bn_case(dtype, ge.chans(dtype, ge.CH2[i]), M, two, True, twice=False)


def _children():
    return [pytest.param(k, id=k) for k in SWITCHES] if not HERE else []


@pytest.mark.parametrize("switch", _children())
def test_switched_paths_in_a_child_process(switch):
    _LEDGER.run_child(__file__, switch, SWITCHES[switch])


def _coverage():
    return [pytest.param("all", id="all")] if not HERE else []


LAUNCHERS = ["rowdot_fwd", "rowdot_bwd", "gate_psi_fwd", "gate_psi_fwd_ok", "gate_bn_bwd_reduce_rows", "gate_bn_bwd_reduce", "gate_bn_bwd_apply",
             "gate_mul_fwd", "gate_mul_bwd", "bn1_bwd_apply"]
BRANCHES = {
    "rowdot_fwd": ["window.one_sweep", "window.second_sweep", "window.clamped_tail", "window.idle_lanes", "window.extra_chunks",
                   "window.rows_past_grid", "planes.fwd"],
    "gate_psi_fwd": ["window.one_sweep", "window.second_sweep", "window.clamped_tail", "window.idle_lanes", "window.rows_past_grid"],
    "gate_mul_bwd": ["mul_bwd.one_chunk", "mul_bwd.strided", "mul_bwd.accumulate", "mul_bwd.empty_workgroup", "mul_bwd.boundary_off_64"],
    "rowdot_bwd": ["rowred.fetch.ring", "rowred.fetch.second_trip", "rowred.fetch.ring+tail", "rowred.fetch.tail_only", "colblocks>1", "planes.bwd"],
    "gate_bn_bwd_reduce": ["rowred.fetch.ring", "rowred.fetch.second_trip", "rowred.fetch.ring+tail", "rowred.fetch.tail_only", "colblocks>1", "one", "two"],
    "gate_bn_bwd_apply": ["rowred.fetch.ring", "rowred.fetch.second_trip", "rowred.fetch.ring+tail", "rowred.fetch.tail_only", "colblocks>1", "one", "two"],
    "gate_mul_fwd": ["rowmap.plain", "colblocks>1"],
    "bn1_bwd_apply": ["bn1.second_trip"],
}


@pytest.mark.parametrize("scope", _coverage())
def test_every_launcher_and_branch_ran(scope):
    """(runs last) every launcher of gate.hip and the two host queries in three dtypes, every branch per launcher and dtype, the two
    children; prints the table"""
    table = {}
    for r in _LEDGER.results + _LEDGER.child_rows:
        t = table.setdefault((r["launcher"], r["dtype"]), {"n": 0, "switch": set(), "br": set()})
        t["n"] += r["n"]
        t["switch"].add(r["switch"] or "default")
        t["br"] |= set(r["branches"])
    print("\n| launcher | dtype | launches checked | processes | branches |")
    print("|---|---|---|---|---|")
    for (l, dt), t in sorted(table.items()):
        print(f"| {l} | {dt} | {t['n']} | {' '.join(sorted(t['switch']))} | {' '.join(sorted(t['br']))} |")
    print("child processes:", ", ".join(f"{k} {v:.1f} s" for k, v in _LEDGER.child_time.items()))
    for dt in ("float32", "bfloat16", "float16"):
        for l in LAUNCHERS:
            assert (l, dt) in table, f"{l} never ran in {dt}"
            missing = [b for b in BRANCHES.get(l, []) if b not in table[(l, dt)]["br"]]
            assert not missing, f"{l} {dt}: branches that never ran: {missing}"
        for l in ge.WALK_LAUNCHERS:
            assert "wgs3" in table[(l, dt)]["switch"], f"{l} never ran on three workgroups in {dt}"
        for l in ("gate_bn_bwd_reduce", "gate_bn_bwd_apply"):
            assert "nt" in table[(l, dt)]["switch"], f"{l} never ran under the nt switches in {dt}"


# a process collects only its own cases (an empty parameter set would show up as a skipped test)
_PARENT = ("test_rowdot_fwd", "test_gate_psi_fwd", "test_channel_planes", "test_rowdot_bwd", "test_gate_bn_bwd", "test_reductions_past_a_whole_sweep",
           "test_gate_mul_fwd", "test_gate_mul_bwd", "test_bn1_bwd_apply", "test_switched_paths_in_a_child_process",
           "test_every_launcher_and_branch_ran")
if HERE:
    for _t in _PARENT:
        del globals()[_t]
if HERE != "wgs3":
    del globals()["test_walk_every_row_count_on_three_workgroups"]
if HERE != "nt":
    del globals()["test_streaming_load_instantiations"]
