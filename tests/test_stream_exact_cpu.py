"""CPU checks of tests/stream_exact.py, the instrument of tests/test_gpu_stream_exact.py: its fp64 references against torch
autograd on random real data, the generators' exactness claim (float32 and fp64, forward and reversed row order: four bit-equal
runs), and the derived bounds of the real-data chain (a float32 restatement in the kernels' order stays within HALF of each bound
— for dx: half of the fp32 part, the half ulp of the storage type being the result's own rounding —, a chain with a seeded fault
exceeds it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import stream_exact as se

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
N, C, H, W = 3, 6, 4, 6
M = N * H * W
EPS, MOM = 1e-5, 0.125


def _nchw(t):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    err = float((a - b).abs().max())
    assert err <= tol * (1 + float(b.abs().max())), err


def _bn_setup(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 0.5
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    s, q = se.ref_stats(x)
    fin = se.ref_finalize(s, q, M, gamma, beta, torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), MOM, EPS)
    # (ref_finalize rounds invstd / mean to fp32 in front of scale / shift, as the kernel does: the fp64 checks here use them unrounded)
    scale = gamma * fin["invstd"]
    shift = beta - fin["mean"] * scale
    return g, x, gamma, beta, fin, scale, shift


@pytest.mark.parametrize("act,with_res", [(0, False), (1, False), (1, True), (3, True), (2, True), (0, True)])
def test_forward_and_backward_references_match_autograd(act, with_res):
    g, x, gamma, beta, fin, scale, shift = _bn_setup(11 + act)
    res = torch.randn(M, C, generator=g, dtype=torch.float64) if with_res else None
    wgt = torch.randn(M, C, generator=g, dtype=torch.float64)
    xt = _nchw(x).clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rt = _nchw(res).clone().requires_grad_(True) if with_res else None
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    v = F.batch_norm(xt, rm, rv, gt, bt, True, float(np.float32(MOM)), float(np.float32(EPS)))
    if with_res and not act & 2:
        v = v + rt
    if act & 1:
        v = F.relu(v)
    if with_res and act & 2:
        v = v + rt
    (v * _nchw(wgt)).sum().backward()
    # forward: statistics, finalize, apply
    _close(fin["rmean"], rm)
    _close(fin["rvar"], rv)
    y = se.ref_bn_act(x, scale, shift, res=res, act=act)
    _close(y, _rows(v.detach()))
    # backward: mask from the activated tensor (pre-activation residual) or recomputed from x
    if act & 1:
        pre = y - res if (with_res and act & 2) else y
        mask = se.relu_mask(1, y=pre)
        if not with_res:
            assert torch.equal(mask, se.relu_mask(1, x=x, mscale=scale, mshift=shift))
    else:
        mask = None
    gm = se.masked(wgt, mask)
    s0, s1 = se.ref_bwd_sums(gm, x, fin["mean"], fin["invstd"])
    _close(s0, bt.grad)
    _close(s1, gt.grad)
    _close(se.ref_dx(gm, x, gamma, fin["mean"], fin["invstd"], s0, s1, M), _rows(xt.grad))
    if with_res:
        want = se.ref_dpost(wgt) if act & 2 else gm            # dpost: the unmasked gradient; dres: the masked one
        _close(want, _rows(rt.grad))


def test_second_operand_and_post4_references_match_autograd():
    g, x, gamma, beta, fin, scale, shift = _bn_setup(5)
    x2 = torch.randn(M, C, generator=g, dtype=torch.float64)
    sc2, sh2 = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    y = se.ref_bn_act(x, scale, shift, x2, sc2, sh2, act=1)
    _close(y, F.relu(x * scale + shift + x2 * sc2 + sh2))
    # x + relu(bn(.)) applied to the same x four times: d x = the sum of the incoming gradients (+ what was there)
    r = torch.randn(M, C, generator=g, dtype=torch.float64, requires_grad=True)
    ws = [torch.randn(M, C, generator=g, dtype=torch.float64) for _ in range(4)]
    sum((F.relu(x * scale + shift) + r) * w_ for w_ in ws).sum().backward()
    _close(se.ref_dpost(ws[3], None, ws[:3]), r.grad)
    old = torch.randn(M, C, generator=g, dtype=torch.float64)
    _close(se.ref_dpost(ws[3], old, ws[:2]), old + ws[3] + ws[0] + ws[1])


@pytest.mark.parametrize("with_dy", [True, False])
def test_pool_aware_gradient_matches_autograd(with_dy):
    g, x, gamma, beta, fin, scale, shift = _bn_setup(7)
    xt = _nchw(x).clone().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    a = F.relu(F.batch_norm(xt, None, None, gt, bt, True, 0.0, float(np.float32(EPS))))
    p = F.max_pool2d(a, 2, 2)
    w1 = torch.randn(M, C, generator=g, dtype=torch.float64)
    w2 = torch.randn(M // 4, C, generator=g, dtype=torch.float64)
    loss = (p * w2.reshape(N, H // 2, W // 2, C).permute(0, 3, 1, 2)).sum()
    if with_dy:
        loss = loss + (a * _nchw(w1)).sum()
    loss.backward()
    _close(se.ref_pool2(_rows(a.detach()), N, H, W), _rows(p.detach()))
    gg = se.ref_pool_grad(x, scale, shift, w1 if with_dy else None, w2, N, H, W)
    s0, s1 = se.ref_bwd_sums(gg, x, fin["mean"], fin["invstd"])
    _close(s0, bt.grad)
    _close(s1, gt.grad)
    _close(se.ref_dx(gg, x, gamma, fin["mean"], fin["invstd"], s0, s1, M), _rows(xt.grad))


def test_pool_aware_gradient_routes_ties_to_the_first_maximum():
    """integer data: most windows hold ties (and all-zero windows); torch's CPU max_pool2d backward is the rule"""
    g = torch.Generator().manual_seed(3)
    k = se.Consts(g, C)
    x = se.ints(g, (M, C), 4)
    dp = se.ints(g, (M // 4, C), 4)
    a = (x * k.mscale + k.mshift).clamp(min=0)
    at = _nchw(a).clone().requires_grad_(True)
    (F.max_pool2d(at, 2, 2) * dp.reshape(N, H // 2, W // 2, C).permute(0, 3, 1, 2)).sum().backward()
    want = torch.where(a > 0, _rows(at.grad), torch.zeros_like(a))
    got = se.ref_pool_grad(x, k.mscale, k.mshift, None, dp, N, H, W, BF)
    assert torch.equal(got, want)
    aw = se.windows(a, N, H, W)
    assert int(((aw == aw.max(-1, keepdim=True)[0]).sum(-1) > 1).sum()) > 0, "no ties in the data"
    assert torch.equal(se.unwindows(se.windows(x, N, H, W), N, H, W), x)


# ---- the exactness claim --------------------------------------------------------------------------------------------------------
def _exact_chain(ops, np_t, reverse, Mrows, pow2_form):
    """the whole reference chain with separate multiplies and adds in `np_t`, rows summed sequentially in the given order"""
    k, x, x2, res, dy, yact, dp, n, h, w = ops
    f = lambda t: np.asarray(t.numpy(), dtype=np_t)                             # noqa: E731
    order = slice(None, None, -1) if reverse else slice(None)

    def seq(t):
        return np.cumsum(t[order], axis=0, dtype=np_t)[-1]

    out = {}
    X, DY = f(x), f(dy)
    out["s"], out["q"] = seq(X), seq(X * X)
    v = X * f(k.scale) + f(k.shift)
    v = v + f(x2) * f(k.scale2)
    v = v + f(k.shift2)
    v = np.maximum(v + f(res), np_t(0))
    out["y"] = v
    mask = (X * f(k.mscale) + f(k.mshift)) > 0
    g = np.where(mask, DY, np_t(0))
    g2 = np.where(f(yact) > 0, DY, np_t(0))
    xh = (X - f(k.mean)) * f(k.invstd)
    out["s0"], out["s1"], out["s0y"], out["s1y"] = seq(g), seq(g * xh), seq(g2), seq(g2 * xh)
    gi = f(k.gamma) * f(k.invstd)
    out["dx0"] = gi * g                                                         # the coverage form: sums = 0
    out["db0"] = seq(out["dx0"])
    if pow2_form is not None:
        a0, a1 = pow2_form
        invM = np_t(1.0 / Mrows)
        k0, k1 = f(a0 * Mrows) * invM, f(a1 * Mrows) * invM
        out["dx1"] = gi * ((g - k0) - xh * k1)
    a = np.maximum(X * f(k.mscale) + f(k.mshift), np_t(0))
    gp = f(se.ref_pool_grad(x, k.mscale, k.mshift, dy, dp, n, h, w))
    out["p0"], out["p1"] = seq(gp), seq(gp * xh)
    out["a"] = a
    return {kk: np.asarray(vv, dtype=np.float64) for kk, vv in out.items()}


@pytest.mark.parametrize("small,n,h,w", [(False, 2, 8, 16), (True, 8, 32, 32)])
def test_generated_operands_make_every_result_exact(small, n, h, w):
    """float32 and fp64, forward and reversed row order: all four runs bit-equal, equal to the references, storable in every type"""
    g = torch.Generator().manual_seed(17 + small)
    c, m = 16, n * h * w                                                        # (m a power of two for the sums = M * a form)
    k = se.Consts(g, c, small)
    x, x2, res, dy, yact = (se.ints(g, (m, c), lim) for lim in (k.xlim, 4, 4, 4, 4))
    dp = se.ints(g, (m // 4, c), 4)
    a0, a1 = (se.ints(g, (c,), 1, 0.3), se.ints(g, (c,), 1, 0.3)) if small else (None, None)
    ops = (k, x, x2, res, dy, yact, dp, n, h, w)
    runs = [_exact_chain(ops, t, rev, m, (a0, a1) if small else None) for t in (np.float32, np.float64) for rev in (False, True)]
    for r in runs[1:]:
        for key in runs[0]:
            assert np.array_equal(runs[0][key], r[key]), key
    r0 = {kk: torch.from_numpy(vv) for kk, vv in runs[0].items()}
    gm = se.masked(dy, se.relu_mask(1, None, x, k.mscale, k.mshift))
    s0, s1 = se.ref_bwd_sums(gm, x, k.mean, k.invstd)
    assert torch.equal(r0["s0"], s0) and torch.equal(r0["s1"], s1)
    assert torch.equal(r0["y"], se.ref_bn_act(x, k.scale, k.shift, x2, k.scale2, k.shift2, res, 1))
    zero = torch.zeros(c, dtype=torch.float64)
    assert torch.equal(r0["dx0"], se.ref_dx(gm, x, k.gamma, k.mean, k.invstd, zero, zero, m))
    if small:
        assert torch.equal(r0["dx1"], se.ref_dx(gm, x, k.gamma, k.mean, k.invstd, a0 * m, a1 * m, m))
    for dt in (F32, BF, FP):
        for key in ("y", "dx0", "a") + (("dx1",) if small else ()):
            se.assert_storable(r0[key], dt, key)
    t0, t1 = se.bwd_terms(gm, x, k.mean, k.invstd)
    se.assert_f32_sum_exact(t1, float(k.invstd.min()), "g * xhat")
    with pytest.raises(AssertionError):                                         # the helper refuses what it cannot promise
        se.assert_f32_sum_exact(t1 * 3e5, float(k.invstd.min()))
    with pytest.raises(AssertionError):
        se.assert_f32_sum_exact(t1 + 0.3, float(k.invstd.min()))
    with pytest.raises(AssertionError):
        se.assert_storable(torch.tensor([257.0], dtype=torch.float64), BF)


def test_geometry_restates_the_skeletons():
    assert se.geometry(BF, 1024, 4) == (8, 128, 128, 2, 8, 2048)
    assert se.geometry(F32, 48, 4) == (4, 12, 12, 21, 84, 256 * 84)
    assert se.geometry(BF, 2560, 8, 1024) == (8, 320, 256, 1, 8, 8192)
    assert se.geometry(FP, 8, 1, 3) == (8, 1, 1, 256, 256, 768)
    assert se.fetch_grid(16320) == 255 and se.fetch_grid(16321) == 256 and se.fetch_grid(10 ** 6, 3) == 3


# ---- the real-data chain's bounds -------------------------------------------------------------------------------------------------
CHAIN_SHAPES = [(3, 96, 37, 41), (2, 64, 181, 181)]


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [F32, BF, FP], ids=lambda d: str(d).split(".")[-1])
def test_chain_bounds_hold_for_a_float32_restatement_and_catch_seeded_faults(shape, dtype):
    o = se.real_operands(shape, dtype, seed=sum(shape))
    Mr, Cc = o["M"], o["C"]
    _, _, _, rp, _, _ = se.geometry(dtype, Cc, 4)
    grid = se.fetch_grid(Mr)
    K = se.sums_chain_length(Mr, grid, rp)
    g, t0, t1 = se.chain_terms(o)
    s64 = (t0.sum(0), t1.sum(0))
    bnd = (se.sums_bound(t0, K, cb.C), se.sums_bound(t1, K, cb.C))
    s32 = (se.sums32(t0, Mr, grid, rp, 4), se.sums32(t1, Mr, grid, rp, 4))
    for q in range(2):
        r = float(((s32[q].double() - s64[q]).abs() / bnd[q]).max())
        print(f"sums[{q}] K={K}: restatement err/bound {r:.3f}")
        assert r <= 0.5, (q, r)
        bad = se.sums32((t0, t1)[q], Mr, grid, rp, 4, drop_row=Mr // 2)
        assert float(((bad.double() - s64[q]).abs() / bnd[q]).max()) > 1, "a dropped row stays within the bound"
    d64, mag = se.dx_parts(o, g, s32[0], s32[1])
    # (the rounding to the storage type is the result's own: half an ulp of it can be used up by a correct chain, so the margin
    # of two is held on the fp32 part, c = 8 = the formula's eight roundings)
    for fused in (True, False):
        dx = se.dx32(o, g, s32[0], s32[1], dtype, fused)
        r = float(((dx.double() - d64).abs() / se.dx_bound(d64, dx, mag, dtype, cb.ulp, c=8.0)).max())
        print(f"dx fused={fused}: restatement err / bound at c = 8: {r:.3f}")
        assert r <= 1.0, (fused, r)
    dx = se.dx32(o, g, s32[0], s32[1], dtype, True, swap=True)
    assert float(((dx.double() - d64).abs() / se.dx_bound(d64, dx, mag, dtype, cb.ulp)).max()) > 1, "k0 / k1 swapped stays within the bound"
