"""tests/layout_ref.py on the CPU: every reference agrees with an independent restatement on the very inputs of the cases of
tests/test_gpu_layout_exact.py, those inputs have the properties the GPU cases rely on (ties both ways, overflow, subnormals, -0.0
and inf in the rounding inputs; sums that are exact in fp32 but not storable in the up-sampling "rounding" case), and the restated
launch geometry reaches every branch the GPU file's ledger demands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layout_ref as lr
import stream_exact as se

F32, BF, FP = lr.F32, lr.BF, lr.FP
DTYPES = [F32, BF, FP]
TWO = [BF, FP]


def _dn(dtype):
    return str(dtype).split(".")[-1]


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- the rounding -------------------------------------------------------------------------------------------------------------------
def _bf16_rne_bits(x32):
    """fp32 -> bf16 round to nearest even, in integer arithmetic on the bit patterns (no NaN among the inputs)"""
    b = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    lsb = (b >> 16) & 1
    r = ((b + 0x7FFF + lsb) >> 16) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def _round_inputs():
    """every fp32 tensor a GPU case hands to a rounding kernel"""
    yield "specials", lr.specials()
    for N, C, H, W, _ in lr.PACK_INPUT_CASES:
        yield f"nchw {N, C, H, W}", lr.nchw_case(N, C, H, W)
    for dtype in DTYPES:
        for N, H, W in lr.PACK_HW:
            for C in lr.pack_chans(dtype):
                yield f"nchw {N, C, H, W}", lr.nchw_case(N, C, H, W)
    for case in lr.IM2COL_CASES:
        yield f"im2col {case}", lr.im2col_case(*case)
    for i, case in enumerate(lr.WEIGHT_CASES):
        for key in (0, 1):
            w, scale = lr.weight_case(case, key)
            yield f"weight {i}", w
            if scale is not None and not case[5]:
                yield f"scaled weight {i}", (w.reshape(case[0], -1) * scale.view(-1, 1)).reshape(-1)


def test_round_to_is_round_to_nearest_even():
    for what, x in _round_inputs():
        assert not torch.isnan(x).any(), what
        assert torch.equal(_bits(lr.round_to(x, BF)), _bf16_rne_bits(x).reshape(x.shape)), what
        with np.errstate(over="ignore"):
            want = torch.from_numpy(x.numpy().astype(np.float16))
        assert _same_bits(lr.round_to(x, FP), want), what
        assert _same_bits(lr.round_to(x, F32), x), what


def _tie_directions(x, dtype):
    """(ties rounded away from zero, ties rounded towards zero) among the finite results of rounding x to dtype"""
    x = x[torch.isfinite(x)].double()
    r = lr.round_to(x.float(), dtype)
    ok = torch.isfinite(r)
    x, r = x[ok], r[ok]
    # the storage neighbours on both sides of x: r and the value one step from r towards x
    step = torch.where(x > r.double(), 1, -1) * torch.where(r.double() >= 0, 1, -1)
    nb = (_bits(r).to(torch.int32) + step.to(torch.int32)).to(torch.int16).view(dtype).double()
    nb = torch.where(x == r.double(), r.double(), nb)
    tie = (x != r.double()) & ((x - r.double()).abs() == (nb - x).abs())
    away = tie & (r.double().abs() > x.abs())
    return int(away.sum()), int((tie & ~away).sum())


@pytest.mark.parametrize("dtype", TWO, ids=_dn)
def test_rounding_inputs_hold_every_special_value(dtype):
    """the conditions on the inputs: ties both ways, fp16 overflow, an fp16 subnormal result, -0.0, +-inf — in the specials, and
    therefore in every operand they are planted in (asserted for the operands of each rounding launcher)"""
    def check(what, x):
        r = lr.round_to(x, dtype)
        away, toward = _tie_directions(x, dtype)
        assert away > 0 and toward > 0, (what, away, toward)
        assert bool((torch.isinf(r) & torch.isfinite(x)).any()), f"{what}: nothing overflows to inf"
        assert bool(torch.isinf(x).any()) and bool((x == -lr.INF).any()), what
        assert bool(((x == 0) & torch.signbit(x)).any()), f"{what}: no -0.0"
        h = lr.round_to(x, FP)
        assert bool(((h != 0) & (h.abs().double() < 2.0 ** -14)).any()), f"{what}: no fp16 subnormal result"
        assert bool(((x.abs() > 65504) & torch.isfinite(x)).any()), f"{what}: nothing beyond fp16's range"
    check("specials", lr.specials())
    n_sp = len(lr.SPECIALS)
    for what, x in _round_inputs():
        if what.startswith("im2col") or what.startswith("scaled"):
            continue                       # (im2col inputs carry inf on the borders; their rounding is the same conversion)
        if x.numel() >= 2 * n_sp:
            check(what, x)


# ---- layout references against permute / unfold --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_pack_and_unpack_are_permutes(dtype):
    cases = [(N, C, H, W, Cp) for N, C, H, W, Cp in lr.PACK_INPUT_CASES] + [(N, C, H, W, C) for N, H, W in lr.PACK_HW for C in lr.pack_chans(dtype)]
    for N, C, H, W, Cp in cases:
        x = lr.nchw_case(N, C, H, W)
        y = lr.pack_nchw_ref(x, Cp, dtype)
        assert y.shape == (N, H, W, Cp)
        assert _same_bits(y[..., :C].permute(0, 3, 1, 2).contiguous(), x.to(dtype))
        assert torch.equal(_bits(y[..., C:]), torch.zeros_like(_bits(y[..., C:])))              # +0, not -0
        # the last real channel carries inf and the huge value; the padded channels sit next to it
        if (N, C, H, W, Cp) in lr.PACK_INPUT_CASES:
            last = x[:, C - 1]
            assert bool(torch.isinf(last).any()) and bool((last == lr.HUGE).any())
    for N, H, W in lr.PACK_HW:
        for C in lr.pack_chans(dtype):
            s = lr.storage_case(N * H * W, C, dtype)
            u = lr.unpack_ref(s, N, H, W)
            assert u.dtype == F32 and u.shape == (N, C, H, W)
            assert _same_bits(u.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), s.float())
            assert _same_bits(u.to(dtype).permute(0, 2, 3, 1).reshape(-1, C).contiguous(), s)
            tiny = {F32: 2.0 ** -126, BF: 2.0 ** -126, FP: 2.0 ** -14}[dtype]
            assert bool(((s != 0) & (s.double().abs() < tiny)).any()), "no subnormal"
            assert bool(torch.isinf(s).any()) and bool(((s == 0) & torch.signbit(s)).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("case", lr.IM2COL_CASES + [lr.IM2COL_ROWS], ids=str)
def test_im2col3_is_unfold(case, dtype):
    N, C, H, W = case
    x = lr.im2col_case(N, C, H, W)
    y = lr.im2col3_ref(x, dtype)
    assert y.shape == (N, H, W, 32)
    # unfold copies: an inf next to the zero padding stays an inf, the padding a +0
    ref = F.unfold(x, 3, padding=1).view(N, C * 9, H, W).permute(0, 2, 3, 1).contiguous()
    assert _same_bits(y[..., :9 * C].contiguous(), ref.to(dtype))
    assert torch.equal(_bits(y[..., 9 * C:]), torch.zeros_like(_bits(y[..., 9 * C:])))
    assert bool(torch.isinf(x[:, C - 1]).any())
    border = torch.cat([x[:, :, 0].flatten(), x[:, :, -1].flatten(), x[:, :, :, 0].flatten(), x[:, :, :, -1].flatten()])
    assert bool(torch.isinf(border).any())


# ---- weight packs against gpu_util.pack_w ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("i", range(len(lr.WEIGHT_CASES)), ids=lambda i: "case%d" % i)
def test_pack_weight_ref_is_pack_w(i, dtype):
    from gpu_util import pack_w
    case = lr.WEIGHT_CASES[i]
    Co, Ci, Cip, KH, KW, tr, has_wb, sc = case
    for key in (0, 1):
        w, scale = lr.weight_case(case, key)
        wf, wb = lr.pack_weight_ref(w, Co, Ci, Cip, KH * KW, tr, scale if key == 0 else None, dtype)
        w4 = w.reshape(Ci, Co, KH, KW) if tr else w.reshape(Co, Ci, KH, KW)
        if scale is not None and not tr and key == 0:
            w4 = w4 * scale.view(-1, 1, 1, 1)
        rf, rb = pack_w(w4, dtype, cip=Cip, transposed=bool(tr), dev="cpu")
        assert _same_bits(wf, rf) and _same_bits(wb, rb)
        if scale is not None and key == 0:
            # not a power of two: the product needs its own fp32 rounding, so folding it elsewhere would show
            m = torch.frexp(scale)[0]
            assert bool((m != 0.5).all())
            plain, _ = lr.pack_weight_ref(w, Co, Ci, Cip, KH * KW, tr, None, dtype)
            assert _same_bits(plain, wf) == bool(tr)            # ignored when transposed, folded otherwise


def test_weight_cases_cover_the_tap_classes_and_the_sweep():
    taps = {c[3] * c[4] for c in lr.WEIGHT_CASES}
    assert taps == set(lr.TB_CLASSES)
    for t, tb in lr.TB_CLASSES.items():
        assert lr.weight_tb(t) == tb
    Co, Ci, Cip, KH, KW = lr.WEIGHT_SWEEP[:5]
    assert Co * KH * KW * Cip > lr.WEIGHT_CAP
    assert sorted(set(sum(lr.WEIGHT_TABLES.values(), []))) == list(range(len(lr.WEIGHT_CASES)))
    assert lr.WEIGHT_TABLES["all"] == list(range(len(lr.WEIGHT_CASES)))
    for name, idx in lr.WEIGHT_TABLES.items():
        assert name == "all" or len(idx) < len(lr.WEIGHT_CASES)
    big = [i for i, c in enumerate(lr.WEIGHT_CASES) if "tiles>grid" in lr.weight_branches(c, BF)]
    assert big and len(big) < len(lr.WEIGHT_CASES)            # idle workgroups and the second trip in one table


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_weight_cases_reach_every_branch(dtype):
    seen = set()
    for c in lr.WEIGHT_CASES:
        seen.update(lr.weight_branches(c, dtype))
    need = {f"TB{tb}" for tb in lr.TB_CLASSES.values()} | {"elem_a", "elem_b", "pad_tile", "part_tile", "ragged_a", "tiles>grid", "scale",
                                                          "no_scale", "scale+transposed", "no_wb", "transposed"}
    if dtype != F32:
        need |= {"vec_a", "vec_b"}
    assert need <= seen, need - seen
    by = {i: set(lr.weight_branches(c, dtype)) for i, c in enumerate(lr.WEIGHT_CASES)}
    assert "pad_tile" in by[4] and "pad_tile" in by[5] and "part_tile" in by[7] and "tiles>grid" in by[15]
    if dtype != F32:
        assert "elem_b" in by[8] and "vec_b" in by[1] and "elem_a" in by[2]


# ---- the up-sampling gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", lr.UPSAMPLE_SHAPES, ids=str)
def test_upsample2_bwd_ref_is_autograd_of_nearest(shape, dtype):
    N, H, W = shape
    for C in lr.upsample_chans(dtype):
        for kind in ("int",) + (("rounding",) if dtype != F32 else ()):
            dy, old = lr.upsample_case(N, H, W, C, dtype, kind)
            x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
            up = F.interpolate(x, scale_factor=2.0, mode="nearest")
            up.backward(dy.double().reshape(N, 2 * H, 2 * W, C).permute(0, 3, 1, 2))
            g = x.grad.permute(0, 2, 3, 1).reshape(N * H * W, C)
            for o in (None, old):
                want = g if o is None else g + o.double()
                ref = lr.upsample2_bwd_ref(dy, o, dtype, shape)
                assert _same_bits(ref, want.to(dtype))
            terms = torch.cat([lr.groups2x2(dy, N, H, W), old.double().unsqueeze(0)]).reshape(5, -1)
            se.assert_f32_sum_exact(terms, 1.0, f"upsample {shape} {kind}")
            s4, s5 = terms[:4].sum(0), terms.sum(0)
            stor4, stor5 = s4.to(dtype).double() == s4, s5.to(dtype).double() == s5
            if kind == "int":
                assert bool(stor4.all()) and bool(stor5.all())
            elif s4.numel() >= 40:
                assert int((~stor4).sum()) > 0 and int((~stor5).sum()) > 0
                # a kernel that rounded the group sum before adding old, or that summed in the storage type, gives other bits
                twice = (s4.to(dtype).double() + terms[4]).to(dtype).double()
                assert int((twice != s5.to(dtype).double()).sum()) > 0
                chain = terms[0].to(dtype)
                for k in (1, 2, 3):
                    chain = (chain.double() + terms[k]).to(dtype)
                assert int((chain.double() != s4.to(dtype).double()).sum()) > 0


@pytest.mark.parametrize("dtype", TWO, ids=_dn)
def test_upsample_rounding_case_exists_at_every_shape_family(dtype):
    """summed over the cases of a dtype the rounding data hold unstorable sums at every C"""
    for C in lr.upsample_chans(dtype):
        n = 0
        for N, H, W in lr.UPSAMPLE_SHAPES:
            dy, old = lr.upsample_case(N, H, W, C, dtype, "rounding")
            s = lr.groups2x2(dy, N, H, W).sum(0)
            n += int((s.to(dtype).double() != s).sum())
        assert n > 0


# ---- add, ReLU gradient ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_add_and_relu_refs_and_their_data(dtype):
    unstorable = 0
    for C in lr.chans(dtype):
        for M in lr.rowmap_rows(dtype, C):
            a, b = lr.add_case(M, C, dtype)
            s = a.double() + b.double()
            assert _same_bits(lr.add_ref(a, b, dtype), s.to(dtype))
            unstorable += int((s.to(dtype).double() != s).sum())
            assert _same_bits(lr.add_ref(a, None, dtype), a)
            dy, y = lr.relu_case(M, C, dtype)
            ref = lr.relu_bwd_ref(dy, y)
            pos = y.double() > 0
            assert torch.equal(_bits(ref)[pos], _bits(dy)[pos]) and bool((_bits(ref)[~pos] == 0).all())
            if M * C >= 256:
                neg0 = (y == 0) & torch.signbit(y)
                assert bool(neg0.any()) and bool(((y == 0) & ~torch.signbit(y)).any()) and bool((y < 0).any())
                for m in (pos, ~pos):
                    assert bool(torch.isinf(dy[m]).any()) and bool(((dy[m] == 0) & torch.signbit(dy[m])).any())
    assert (unstorable > 0) == (dtype == BF)       # bf16: most sums need the one rounding; fp16 / fp32 store them all
    # the copy form carries subnormals, inf and -0.0
    s = lr.storage_case(7, 8, dtype, key=1)
    assert bool(torch.isinf(s).any()) and bool(((s == 0) & torch.signbit(s)).any())


# ---- the geometry restatement reaches every branch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_case_tables_reach_every_branch(dtype):
    epc = lr.EPC[dtype]
    # flat kernels: one case beyond a whole grid each
    N, C, H, W = lr.pack_sweep(dtype)
    assert lr.flat_branches(N * H * W * (C // epc)) == ["grid_stride"]
    N, C, H, W = lr.UNPACK_SWEEP
    assert lr.flat_branches(N * C * H * W) == ["grid_stride"] and C % epc == 0
    N, H, W, C = lr.upsample_sweep(dtype)
    assert lr.flat_branches(N * H * W * (C // epc)) == ["grid_stride"] and H % 2 and W % 2
    assert N * 4 * H * W * (C + 16) * (16 // epc) < 140e6                     # the largest operand of the file
    for N, C, H, W, Cp in lr.PACK_INPUT_CASES:
        assert not lr.flat_branches(N * H * W * (Cp // epc))
    # im2col: every workgroup width, with one and with two workgroups along x
    seen = set()
    for case in lr.IM2COL_CASES:
        seen.add(tuple(lr.im2col_branches(case[3])))
    assert seen == {("bx64",), ("bx64", "x_blocks>1"), ("bx128",), ("bx128", "x_blocks>1"), ("bx256",), ("bx256", "x_blocks>1")}
    assert lr.IM2COL_ROWS[0] * lr.IM2COL_ROWS[2] == 65538
    # rowmap: chunk counts that do not divide 256, more than 256 chunks, a second sweep
    cps = [lr.rowmap_geom(dtype, C)[0] for C in lr.chans(dtype)]
    assert any(256 % cp for cp in cps if cp <= 256) and any(cp > 256 for cp in cps)
    assert any("colblocks>1" in lr.rowmap_branches(dtype, C, 1) for C in lr.chans(dtype))
    for C in lr.chans(dtype):
        assert all("second_sweep" not in lr.rowmap_branches(dtype, C, M) for M in lr.rowmap_rows(dtype, C))
    M, C = lr.rowmap_sweep(dtype)
    cp, tpr, rp = lr.rowmap_geom(dtype, C)
    assert cp == 256 and rp == 1 and M == 4096 * rp + rp + 1 and lr.rowmap_branches(dtype, C, M) == ["second_sweep"]
