"""The layout, weight-pack, up-sampling and add / ReLU kernels of csrc/elementwise.hip against the references of
tests/layout_ref.py, at the sizes where their grids, loops and tile paths change.  Every one of these operations is exact or
rounds exactly once, so every comparison is of BITS (-0.0, inf and subnormals count); there is no tolerance in this file.

NHWC tensors are channel slices with guard channels and guard rows (ld = C + 16 or wider), contiguous operands sit between guard
pads (tests/exact_harness.py: Slice, Pad): NaN around inputs, a sentinel around outputs, outputs pre-filled with NaN.  After each
launch: guards unchanged, no NaN, the bits of the reference, and a second launch gives the same bytes.  The last test asserts
from the ledger that every launcher ran in every dtype with every branch of the list at the end of this file.

What tests/test_gpu_ops.py did not reach, and the test here that does:
  pack / unpack: ld > C, C = 1, Cpad = C, a pad starting inside a chunk, grid-stride     test_pack_input_nchw, test_pack_unpack_nchw, test_*_sweep
  im2col3: the 128- and 256-wide workgroups, a second workgroup along x, H < 3,          test_im2col3, test_im2col3_many_rows
    N * H beyond 65 535
  weight packs: Co = 1, 2; tiles all or partly padding; element and vector paths; a      test_pack_conv_weights_batched, test_pack_conv_weight
    scale on a transposed descriptor; more tiles than workgroups; taps up to 256
  upsample2_bwd: accumulate, sliced ld, where and how often it rounds, a whole sweep     test_upsample2_bwd, test_upsample2_bwd_sweep
  add: the copy form, both in-place forms, three different ld, > 256 chunks per row      test_add_relu_bwd, test_add_relu_bwd_sweep
  relu_bwd: -0.0 in y, inf / -0.0 in dy, ld > C"""
import pytest
import torch

import layout_ref as lr
from exact_harness import F32, BF, FP, DTYPES, G, Slice, Pad, Vec, Ledger, _run_bits, _bits, _dn  # noqa: F401
from gpu_util import DEV
from mi355.lib import lib, DTYPE_CODE

pytestmark = pytest.mark.gpu

_LEDGER = Ledger("MI355_LAYOUT")
_mark = _LEDGER.mark
GR = 2                         # guard rows behind a slice


def _rows(t):
    """[N, H, W, C] -> [N*H*W, C]"""
    return t.reshape(-1, t.shape[-1])


def _refused(what, fn, bufs):
    """the launcher refuses its arguments on the host and writes nothing"""
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.untouched(), f"{what}: buffer {i} was written by a refused call"


# ---- NCHW fp32 -> padded NHWC (the network input) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", lr.PACK_INPUT_CASES, ids=lambda c: "n%d_c%d_%dx%d_pad%d" % c)
def test_pack_input_nchw(case, dtype):
    N, C, H, W, Cpad = case
    x = lr.nchw_case(N, C, H, W)
    xb, yb = Pad(x.numel(), F32, x), Pad(N * H * W * Cpad, dtype)
    _run_bits(f"pack_input_nchw {case}", lambda: lib.mi355_pack_input_nchw(xb.ptr, yb.ptr, N, C, H, W, Cpad, DTYPE_CODE[dtype]),
              [xb, yb], {yb: lr.pack_nchw_ref(x, Cpad, dtype)})
    _mark("pack_input_nchw", dtype, "c%d_pad%d" % (C, Cpad))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_pack_input_nchw_sweep(dtype):
    N, Cpad, H, W = lr.pack_sweep(dtype)
    C = 3
    x = lr.nchw_case(N, C, H, W, big=True)
    xb, yb = Pad(x.numel(), F32, x), Pad(N * H * W * Cpad, dtype)
    _run_bits("pack_input_nchw sweep", lambda: lib.mi355_pack_input_nchw(xb.ptr, yb.ptr, N, C, H, W, Cpad, DTYPE_CODE[dtype]),
              [xb, yb], {yb: lr.pack_nchw_ref(x, Cpad, dtype)})
    _mark("pack_input_nchw", dtype, *lr.flat_branches(N * H * W * (Cpad // lr.EPC[dtype])))


# ---- NCHW fp32 <-> a channel slice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("nhw", lr.PACK_HW, ids=lambda c: "n%d_%dx%d" % c)
def test_pack_unpack_nchw(nhw, dtype):
    N, H, W = nhw
    code = DTYPE_CODE[dtype]
    for C in lr.pack_chans(dtype):
        x = lr.nchw_case(N, C, H, W)
        xb, yb = Pad(x.numel(), F32, x), Slice(N * H * W, C, dtype, GR)
        assert yb.ld == C + 16
        _run_bits(f"pack_nchw {nhw} C={C}", lambda: lib.mi355_pack_nchw(xb.ptr, yb.ptr, N, C, H, W, yb.ld, code), [xb, yb],
                  {yb: _rows(lr.pack_nchw_ref(x, C, dtype))})
        _mark("pack_nchw", dtype, f"c{C}", "%dx%d" % (H, W))
        s = lr.storage_case(N * H * W, C, dtype)
        sb, ob = Slice(N * H * W, C, dtype, GR, s), Pad(N * C * H * W, F32)
        _run_bits(f"unpack_output_nchw {nhw} C={C}", lambda: lib.mi355_unpack_output_nchw(sb.ptr, ob.ptr, N, C, H, W, sb.ld, code),
                  [sb, ob], {ob: lr.unpack_ref(s, N, H, W)})
        _mark("unpack_output_nchw", dtype, f"c{C}", "%dx%d" % (H, W))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_pack_nchw_sweep(dtype):
    N, C, H, W = lr.pack_sweep(dtype)
    x = lr.nchw_case(N, C, H, W, big=True)
    xb, yb = Pad(x.numel(), F32, x), Slice(N * H * W, C, dtype, GR)
    _run_bits("pack_nchw sweep", lambda: lib.mi355_pack_nchw(xb.ptr, yb.ptr, N, C, H, W, yb.ld, DTYPE_CODE[dtype]), [xb, yb],
              {yb: _rows(lr.pack_nchw_ref(x, C, dtype))})
    _mark("pack_nchw", dtype, *lr.flat_branches(N * H * W * (C // lr.EPC[dtype])))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_unpack_output_nchw_sweep(dtype):
    N, C, H, W = lr.UNPACK_SWEEP
    s = lr.storage_case(N * H * W, C, dtype)
    sb, ob = Slice(N * H * W, C, dtype, GR, s), Pad(N * C * H * W, F32)
    _run_bits("unpack_output_nchw sweep", lambda: lib.mi355_unpack_output_nchw(sb.ptr, ob.ptr, N, C, H, W, sb.ld, DTYPE_CODE[dtype]),
              [sb, ob], {ob: lr.unpack_ref(s, N, H, W)})
    _mark("unpack_output_nchw", dtype, *lr.flat_branches(N * C * H * W))


# ---- the stem's 3 x 3 patches -----------------------------------------------------------------------------------------------------------
def _im2col(case, dtype):
    N, C, H, W = case
    x = lr.im2col_case(N, C, H, W)
    xb, yb = Pad(x.numel(), F32, x), Pad(N * H * W * 32, dtype)
    _run_bits(f"pack_input_im2col3 {case}", lambda: lib.mi355_pack_input_im2col3(xb.ptr, yb.ptr, N, C, H, W, DTYPE_CODE[dtype]),
              [xb, yb], {yb: lr.im2col3_ref(x, dtype)})


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", lr.IM2COL_CASES, ids=lambda c: "n%d_c%d_%dx%d" % c)
def test_im2col3(case, dtype):
    _im2col(case, dtype)
    _mark("pack_input_im2col3", dtype, "c%d_%dx%d" % case[1:], *lr.im2col_branches(case[3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_im2col3_many_rows(dtype):
    """N * H = 65 538 image rows: more than 65 535 workgroup rows"""
    N, C, H, W = lr.IM2COL_ROWS
    assert N * H > 65535
    _im2col(lr.IM2COL_ROWS, dtype)
    _mark("pack_input_im2col3", dtype, "rows>65535")


# ---- weight packs -------------------------------------------------------------------------------------------------------------------------
def _weight_operands(case, dtype, key):
    """device operands of one weight case and the references of its packs; the scale only where the launcher takes one"""
    Co, Ci, Cip, KH, KW, tr, has_wb, sc = case
    taps = KH * KW
    w, scale = lr.weight_case(case, key)
    wf_ref, wb_ref = lr.pack_weight_ref(w, Co, Ci, Cip, taps, tr, scale, dtype)
    wv = Pad(w.numel(), F32, w)
    wf = Pad(Co * taps * Cip, dtype)
    wb = Pad(Cip * taps * Co, dtype) if has_wb else None
    sv = Pad(Co, F32, scale) if scale is not None else None
    bufs = [b for b in (wv, wf, wb, sv) if b is not None]
    want = {wf: wf_ref}
    if wb is not None:
        want[wb] = wb_ref
    return wv, wf, wb, sv, bufs, want


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("table", list(lr.WEIGHT_TABLES), ids=str)
def test_pack_conv_weights_batched(table, dtype):
    idx = lr.WEIGHT_TABLES[table]
    rows, bufs, want, branches = [], [], {}, set()
    for i in idx:
        case = lr.WEIGHT_CASES[i]
        Co, Ci, Cip, KH, KW, tr, has_wb, sc = case
        wv, wf, wb, sv, b, w_ = _weight_operands(case, dtype, key=0)
        rows.append([wv.ptr, wf.ptr, wb.ptr if wb is not None else 0, Co, Ci, Cip, KH * KW, tr, sv.ptr if sv is not None else 0])
        bufs += b
        want.update(w_)
        branches.update(lr.weight_branches(case, dtype))
        branches.add("case%d" % i)
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    _run_bits(f"pack_conv_weights_batched {table}", lambda: lib.mi355_pack_conv_weights_batched(tab, len(rows), 9, DTYPE_CODE[dtype]),
              bufs, want)
    _mark("pack_conv_weights_batched", dtype, f"table_{table}", *branches, n=len(idx))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("i", range(len(lr.WEIGHT_CASES) + 1), ids=lambda i: "case%d" % i if i < len(lr.WEIGHT_CASES) else "sweep")
def test_pack_conv_weight(i, dtype):
    sweep = i == len(lr.WEIGHT_CASES)
    case = lr.WEIGHT_SWEEP if sweep else lr.WEIGHT_CASES[i]
    case = case[:7] + (0,)                                  # (this launcher takes no scale)
    Co, Ci, Cip, KH, KW, tr, has_wb, _ = case
    wv, wf, wb, _, bufs, want = _weight_operands(case, dtype, key=1)
    _run_bits(f"pack_conv_weight {case}", lambda: lib.mi355_pack_conv_weight(wv.ptr, wf.ptr, wb.ptr if wb is not None else None, Co, Ci, Cip,
                                                                           KH, KW, tr, DTYPE_CODE[dtype]), bufs, want)
    _mark("pack_conv_weight", dtype, "sweep" if sweep else "case%d" % i, f"taps{KH * KW}", *(["transposed"] if tr else []),
          *(["no_wb"] if not has_wb else []), *lr.flat_branches(Co * KH * KW * Cip, lr.WEIGHT_CAP))


# ---- gradient of nearest x2 up-sampling ---------------------------------------------------------------------------------------------------
def _upsample(what, N, H, W, C, dtype, dy, old):
    """both accumulate modes on the same operands"""
    dyb = Slice(N * 4 * H * W, C, dtype, GR, dy)
    assert dyb.ld == C + 16
    for acc in (0, 1):
        dxb = Slice(N * H * W, C, dtype, GR, old if acc else None, inout=bool(acc))
        ref = lr.upsample2_bwd_ref(dy, old if acc else None, dtype, (N, H, W))
        _run_bits(f"upsample2_bwd {what} acc={acc}",
                  lambda: lib.mi355_upsample2_bwd(dyb.ptr, dyb.ld, dxb.ptr, dxb.ld, N, H, W, C, acc, DTYPE_CODE[dtype]), [dyb, dxb], {dxb: ref})
        del dxb


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", lr.UPSAMPLE_SHAPES, ids=lambda c: "n%d_%dx%d" % c)
def test_upsample2_bwd(shape, dtype):
    N, H, W = shape
    for C in lr.upsample_chans(dtype):
        for kind in ("int",) + (("rounding",) if dtype != F32 else ()):
            dy, old = lr.upsample_case(N, H, W, C, dtype, kind)
            _upsample(f"{shape} C={C} {kind}", N, H, W, C, dtype, dy, old)
            _mark("upsample2_bwd", dtype, "n%d_%dx%d" % shape, f"c{C}", kind, "acc0", "acc1", n=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_upsample2_bwd_sweep(dtype):
    N, H, W, C = lr.upsample_sweep(dtype)
    assert H % 2 and W % 2
    g = lr._gen(N, H, W, C, 37)
    dy, old = lr.big_ints(g, (N * 4 * H * W, C), dtype), lr.big_ints(g, (N * H * W, C), dtype)
    _upsample("sweep", N, H, W, C, dtype, dy, old)
    _mark("upsample2_bwd", dtype, "acc0", "acc1", *lr.flat_branches(N * H * W * (C // lr.EPC[dtype])), n=2)


# ---- add (two operands, copy, in place) and the ReLU gradient: three independent ld --------------------------------------------------------
def _add_relu(M, C, dtype):
    code = DTYPE_CODE[dtype]
    rp = lr.rowmap_geom(dtype, C)[2]
    gr = min(rp, 4)
    a, b = lr.add_case(M, C, dtype)
    what = f"M={M} C={C}"
    # out of place, every ld its own
    ab, bb, yb = Slice(M, C, dtype, gr, a, g=8), Slice(M, C, dtype, gr, b, g=16), Slice(M, C, dtype, gr, g=24)
    assert len({ab.ld, bb.ld, yb.ld}) == 3 and ab.ld == C + 16
    _run_bits(f"add {what}", lambda: lib.mi355_add(ab.ptr, ab.ld, bb.ptr, bb.ld, yb.ptr, yb.ld, M, C, code), [ab, bb, yb],
              {yb: lr.add_ref(a, b, dtype)})
    # b == NULL: a strided copy, bits unchanged
    s = lr.storage_case(M, C, dtype, key=1)
    sb, cb = Slice(M, C, dtype, gr, s, g=16), Slice(M, C, dtype, gr, g=8)
    _run_bits(f"add copy {what}", lambda: lib.mi355_add(sb.ptr, sb.ld, None, 0, cb.ptr, cb.ld, M, C, code), [sb, cb], {cb: lr.add_ref(s, None, dtype)})
    # in place: y == a, then y == b
    ia = Slice(M, C, dtype, gr, a, inout=True, g=24)
    _run_bits(f"add y==a {what}", lambda: lib.mi355_add(ia.ptr, ia.ld, bb.ptr, bb.ld, ia.ptr, ia.ld, M, C, code), [ia, bb], {ia: lr.add_ref(a, b, dtype)})
    ib = Slice(M, C, dtype, gr, b, inout=True, g=24)
    _run_bits(f"add y==b {what}", lambda: lib.mi355_add(ab.ptr, ab.ld, ib.ptr, ib.ld, ib.ptr, ib.ld, M, C, code), [ab, ib], {ib: lr.add_ref(a, b, dtype)})
    br = lr.rowmap_branches(dtype, C, M)
    _mark("add", dtype, f"c{C}", "add.two", "add.copy", "add.inplace_a", "add.inplace_b", *br, n=4)
    # the ReLU gradient
    dy, y = lr.relu_case(M, C, dtype)
    db, yv, xb = Slice(M, C, dtype, gr, dy, g=8), Slice(M, C, dtype, gr, y, g=16), Slice(M, C, dtype, gr, g=24)
    _run_bits(f"relu_bwd {what}", lambda: lib.mi355_relu_bwd(db.ptr, db.ld, yv.ptr, yv.ld, xb.ptr, xb.ld, M, C, code), [db, yv, xb],
              {xb: lr.relu_bwd_ref(dy, y)})
    _mark("relu_bwd", dtype, f"c{C}", *br)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("k", range(len(lr.CH2)), ids=lambda k: "c%d" % lr.CH2[k])
def test_add_relu_bwd(k, dtype):
    from test_gpu_stream_exact import _chans, _edge_rows
    assert lr.chans(dtype) == _chans(dtype)
    C = lr.chans(dtype)[k]
    rp = lr.rowmap_geom(dtype, C)[2]
    assert lr.rowmap_rows(dtype, C) == _edge_rows(rp, 1, (3 * rp + 2,))
    for M in lr.rowmap_rows(dtype, C):
        _add_relu(M, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_add_relu_bwd_sweep(dtype):
    M, C = lr.rowmap_sweep(dtype)
    _add_relu(M, C, dtype)


# ---- arguments refused on the host ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_refused_arguments_write_nothing(dtype):
    code = DTYPE_CODE[dtype]
    N, H, W = 1, 2, 3
    x = Pad(16 * N * H * W, F32, torch.ones(16 * N * H * W))
    y = Pad(64 * N * H * W, dtype)
    _refused("pack_nchw C=6", lambda: lib.mi355_pack_nchw(x.ptr, y.ptr, N, 6, H, W, 16, code), [x, y])
    _refused("pack_input_nchw Cpad=12", lambda: lib.mi355_pack_input_nchw(x.ptr, y.ptr, N, 3, H, W, 12, code), [x, y])
    _refused("pack_input_nchw Cpad<C", lambda: lib.mi355_pack_input_nchw(x.ptr, y.ptr, N, 9, H, W, 8, code), [x, y])
    _refused("pack_input_im2col3 C=4", lambda: lib.mi355_pack_input_im2col3(x.ptr, y.ptr, N, 4, H, W, code), [x, y])
    w, wf, wb = Pad(8 * 5 * 9, F32, torch.ones(8 * 5 * 9)), Pad(8 * 9 * 8, dtype), Pad(8 * 9 * 8, dtype)
    _refused("pack_conv_weight Cip<Ci", lambda: lib.mi355_pack_conv_weight(w.ptr, wf.ptr, wb.ptr, 8, 5, 4, 3, 3, 0, code), [w, wf, wb])
    tab = torch.tensor([[w.ptr, wf.ptr, wb.ptr, 8, 5, 8, 9, 0, 0]], dtype=torch.int64).to(DEV)
    _refused("pack_conv_weights_batched fields=8", lambda: lib.mi355_pack_conv_weights_batched(tab, 1, 8, code), [w, wf, wb])
    a, o = Slice(4 * H * W, 6, dtype, GR, torch.ones(4 * H * W, 6, dtype=dtype)), Slice(4 * H * W, 6, dtype, GR)
    _refused("add C=6", lambda: lib.mi355_add(a.ptr, a.ld, a.ptr, a.ld, o.ptr, o.ld, 4 * H * W, 6, code), [a, o])
    _refused("upsample2_bwd C=6", lambda: lib.mi355_upsample2_bwd(a.ptr, a.ld, o.ptr, o.ld, N, H, W, 6, 0, code), [a, o])
    _mark("refused", dtype, "pack_nchw", "pack_input_nchw", "im2col3", "pack_conv_weight", "fields", "add", "upsample2_bwd")


# ---- the ledger -----------------------------------------------------------------------------------------------------------------------------------
_WCASES = ["case%d" % i for i in range(len(lr.WEIGHT_CASES))]
_ROWMAP = ["colblocks>1", "second_sweep"]


def _expected(dtype):
    two = dtype != F32
    return {
        "pack_input_nchw": ["c%d_pad%d" % (c[1], c[4]) for c in lr.PACK_INPUT_CASES] + ["grid_stride"],
        "pack_nchw": [f"c{c}" for c in lr.pack_chans(dtype)] + ["7x9", "1x1", "grid_stride"],
        "unpack_output_nchw": [f"c{c}" for c in lr.pack_chans(dtype)] + ["7x9", "1x1", "grid_stride"],
        "pack_input_im2col3": ["c%d_%dx%d" % c[1:] for c in lr.IM2COL_CASES] + ["bx64", "bx128", "bx256", "x_blocks>1", "rows>65535"],
        "pack_conv_weights_batched": _WCASES + [f"table_{t}" for t in lr.WEIGHT_TABLES] + sorted({f"TB{tb}" for tb in lr.TB_CLASSES.values()})
        + ["elem_a", "elem_b", "pad_tile", "part_tile", "ragged_a", "tiles>grid", "scale", "no_scale", "scale+transposed", "no_wb", "transposed"]
        + (["vec_a", "vec_b"] if two else []),
        "pack_conv_weight": _WCASES + [f"taps{t}" for t in lr.TB_CLASSES] + ["sweep", "grid_stride", "no_wb", "transposed"],
        "upsample2_bwd": ["n%d_%dx%d" % s for s in lr.UPSAMPLE_SHAPES] + [f"c{c}" for c in lr.upsample_chans(dtype)]
        + ["int", "acc0", "acc1", "grid_stride"] + (["rounding"] if two else []),
        "add": [f"c{c}" for c in lr.chans(dtype)] + ["add.two", "add.copy", "add.inplace_a", "add.inplace_b"] + _ROWMAP,
        "relu_bwd": [f"c{c}" for c in lr.chans(dtype)] + _ROWMAP,
        "refused": ["pack_nchw", "pack_input_nchw", "im2col3", "pack_conv_weight", "fields", "add", "upsample2_bwd"],
    }


def test_every_launcher_and_branch_ran():
    """(runs last) every launcher ran in every dtype with every case and branch of _expected; prints launcher x dtype x cases"""
    seen, count = {}, {}
    for r in _LEDGER.results:
        key = (r["launcher"], r["dtype"])
        seen.setdefault(key, set()).update(r["branches"])
        count[key] = count.get(key, 0) + r["n"]
    print("\n| launcher | dtype | compared launches (descriptors for the batched pack) | distinct case / branch names |")
    print("|---|---|---|---|")
    for (l, dt), br in sorted(seen.items()):
        print(f"| {l} | {dt} | {count[(l, dt)]} | {len(br)} |")
    for dtype in DTYPES:
        for l, cases in _expected(dtype).items():
            assert (l, _dn(dtype)) in seen, f"{l} never ran in {_dn(dtype)}"
            missing = [c for c in cases if c not in seen[(l, _dn(dtype))]]
            assert not missing, f"{l} ({_dn(dtype)}): cases / branches that never ran: {missing}"
