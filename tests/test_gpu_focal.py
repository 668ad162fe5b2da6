"""-m gpu: the focal / Tversky / focal-Tversky segmentation loss (csrc/focal_tversky.hip: mi355_ftv_loss_*, mi355.nn.FocalTverskyLoss /
FocalLoss / TverskyLoss) and the focal cross-entropy (mi355_ce_focal, mi355.nn.FocalCrossEntropyLoss) on the device, against the fp64
restatement tests/focal_ref.py, which tests/test_focal_cpu.py pins to torch's fp64 autograd.

Bounds.  Segmentation kernels: those of this loss family in tests/test_gpu_seg_loss.py, |loss - ref| < 1e-5 and
rel_err(dz, ref) < 1e-5 (the difference at the largest magnitude over the reference's largest magnitude).  mi355_ce_focal computes in
double and rounds to float32 once on store: 2^-23 |ref| + 1e-12 for the loss and for every element of dz, as tests/test_gpu_mix.py
derives it for mi355_ce_mix.

Every call through the ABI writes into buffers pre-filled with a sentinel between guard bands and is checked for intact guards,
unchanged sources and two bit-identical runs (the harness of tests/test_gpu_mix.py)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import focal_ref as R
from gpu_util import gpu_kinks, rel_err
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A

# the grid gamma {0, .5, 2} x alpha {-1, .25} x (a, b) {(.5, .5), (.7, .3), (.3, .7)} x g {1, .75, 2} x weights, thinned: every value
# of every parameter occurs, the pure losses (focal alone, Tversky alone) and the mixtures
#        fw   tw   a    b    g     f_alpha gamma smooth
GRID = [(1.0, 0.0, 0.5, 0.5, 1.0, 0.25, 2.0, 1.0),
        (1.0, 0.0, 0.5, 0.5, 1.0, -1.0, 0.0, 1.0),
        (1.0, 0.0, 0.5, 0.5, 1.0, 0.25, 0.5, 1.0),
        (0.0, 1.0, 0.5, 0.5, 1.0, 0.25, 2.0, 1.0),
        (0.0, 1.0, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0),
        (0.0, 1.0, 0.3, 0.7, 2.0, 0.25, 2.0, 1e-3),
        (0.0, 1.0, 0.3, 0.7, 0.75, 0.25, 2.0, 1e-3),
        (0.5, 0.5, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0),
        (0.5, 0.5, 0.5, 0.5, 1.0, -1.0, 0.5, 1.0),
        (0.3, 0.7, 0.3, 0.7, 2.0, 0.25, 0.0, 1.0),
        (0.3, 0.7, 0.7, 0.3, 1.0, -1.0, 2.0, 1e-3),
        (2.0, 0.5, 0.3, 0.7, 0.75, 0.25, 0.5, 1.0)]


def _kw(cfg, ps=False):
    fw, tw, a, b, g, fa, fg, sm = cfg
    return dict(focal_weight=fw, tversky_weight=tw, alpha=a, beta=b, exponent=g, focal_alpha=fa, focal_gamma=fg, smooth=sm, per_sample=ps)


def _f32(cfg):
    """the parameters as the kernels receive them (float arguments)"""
    return tuple(float(np.float32(v)) for v in cfg)


class Guarded:
    """``count`` float32 elements filled with sentinel bytes between two guard bands; ``shift``: the view starts that many bytes off a
    16-byte boundary"""

    def __init__(self, count, shift=0):
        self.nbytes = count * 4
        self.whole = torch.full((self.nbytes + 2 * GUARD + shift,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        self.whole[self.lo:self.lo + self.nbytes] = SENTINEL
        self.t = self.whole[self.lo:self.lo + self.nbytes].view(torch.float32)
        assert self.t.data_ptr() % 16 == shift % 16

    def intact(self):
        return bool((self.whole[:self.lo] == GUARD_BYTE).all()) and bool((self.whole[self.lo + self.nbytes:] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.t.view(torch.uint8) == SENTINEL).all())


def _src(t, shift=0):
    g = Guarded(t.numel(), shift)
    g.t.copy_(t.reshape(-1))
    return g


def op(z, t, cfg, ps, gscale=None, shift=0, runs=2):
    """The C ABI as a caller sees it -> (loss tensor [1], dz tensor of z's shape), both on the host.  z, t: host tensors."""
    from mi355.lib import lib
    fw, tw, a, b, g, fa, fg, sm = cfg
    B, per = z.shape[0], z.numel() // z.shape[0]
    rows = lib.mi355_ftv_loss_rows(B, per)
    assert rows >= B and rows % B == 0
    zs, ts = _src(z, shift), _src(t, shift)
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    outs = []
    for _ in range(runs):
        partial, state, loss, dz = Guarded(rows * 4), Guarded(2 * B), Guarded(1), Guarded(z.numel(), shift)
        lib.mi355_ftv_loss_fwd(zs.t, ts.t, B, per, fw, fa, fg, tw, a, b, g, sm, 1 if ps else 0, partial.t, state.t, loss.t)
        torch.cuda.synchronize()
        assert dz.untouched() and dz.intact()
        lib.mi355_ftv_loss_bwd(zs.t, ts.t, B, per, fw, fa, fg, a, b, state.t, gs, dz.t)
        torch.cuda.synchronize()
        assert partial.intact() and state.intact() and loss.intact() and dz.intact()
        outs.append((loss.t.cpu().clone(), dz.t.cpu().clone().view(z.shape)))
    for l, d in outs[1:]:
        assert torch.equal(l, outs[0][0]) and torch.equal(d, outs[0][1])
    assert zs.intact() and ts.intact() and torch.equal(zs.t.cpu(), z.reshape(-1)) and torch.equal(ts.t.cpu(), t.reshape(-1))
    return outs[0]


def module(z, t, cfg, ps):
    from mi355 import nn as mnn
    crit = mnn.FocalTverskyLoss(**_kw(cfg, ps))
    zz = z.to(DEV).requires_grad_(True)
    loss = crit(zz, t.to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), zz.grad.cpu()


def check(tag, loss, dz, l64, g64):
    l, e = float(loss), rel_err(dz.reshape(-1), torch.from_numpy(np.ascontiguousarray(g64)).reshape(-1))
    print(f"{tag}: loss {l:.8f} ref {l64:.8f} |d| {abs(l - l64):.2e}  dz rel_err {e:.2e}")
    assert np.isfinite(l) and bool(torch.isfinite(dz).all()), tag
    assert abs(l - l64) < 1e-5, (tag, l, l64)
    assert e < 1e-5, (tag, e)


@functools.lru_cache(maxsize=None)
def _data(shape, seed=11):
    g = torch.Generator().manual_seed(seed + sum(shape))
    z = (torch.randn(*shape, generator=g) * 2.0).float()
    t = (torch.rand(*shape, generator=g) < 0.35).float()
    return z, t


SHAPES = [((3, 1, 17, 13), 0), ((1, 1, 64, 64), 0), ((2, 1, 96, 172), 0), ((2, 1, 96, 172), 4)]


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("shape,shift", SHAPES)
def test_parity_with_the_fp64_restatement(shape, shift, ps):
    """(3,1,17,13): per odd, scalar path, one workgroup per sample; (1,1,64,64): one exact four-vector trip; (2,1,96,172): per % 4 = 0,
    four workgroups per sample, some threads in the one-vector loop; the same at a 4-byte offset: the scalar path with per % 4 = 0"""
    from mi355.lib import lib
    z, t = _data(shape)
    B, per = shape[0], z.numel() // shape[0]
    assert lib.mi355_ftv_loss_rows(B, per) // B == {221: 1, 4096: 1, 16512: 4}[per]
    for i, cfg in enumerate(GRID):
        cfg = _f32(cfg)
        for gscale in (None, 3.0, 65536.0) if i == 0 else ((None, 3.0, 65536.0)[i % 3],):          # all three at the first, then rotating
            ref = R.ftv_loss(z.numpy(), t.numpy(), **_kw(cfg, ps), gscale=1.0 if gscale is None else gscale)
            check(f"abi {shape}+{shift} ps={ps} {cfg} gscale={gscale}", *op(z, t, cfg, ps, gscale, shift), *ref)


@pytest.mark.parametrize("ps", [False, True])
def test_parity_at_the_flagship_shape_and_the_module_is_the_abi(ps):
    shape = (32, 1, 256, 256)
    z, t = _data(shape)
    for cfg, gscale in ((GRID[7], None), (GRID[11], 3.0)):
        cfg = _f32(cfg)
        ref = R.ftv_loss(z.numpy(), t.numpy(), **_kw(cfg, ps), gscale=1.0 if gscale is None else gscale)
        loss, dz = op(z, t, cfg, ps, gscale)
        check(f"abi {shape} ps={ps} {cfg} gscale={gscale}", loss, dz, *ref)
        if gscale is None:
            lm, dm = module(z, t, cfg, ps)
            lm2, dm2 = module(z, t, cfg, ps)
            assert torch.equal(lm, lm2) and torch.equal(dm, dm2)
            assert torch.equal(lm.reshape(1), loss) and torch.equal(dm, dz)          # bit for bit


def test_target_is_binarised_in_the_kernels():
    z, t = _data((3, 1, 17, 13))
    g = torch.Generator().manual_seed(1)
    soft = torch.where(t > 0, 0.5 + 2.0 ** -20 + 0.4 * torch.rand(t.shape, generator=g), 0.5 * torch.rand(t.shape, generator=g))
    soft.view(-1)[:4] = torch.tensor([0.5, 0.5, 0.0, 1.0])
    hard = (soft > 0.5).float()
    for ps in (False, True):
        a, b = op(z, soft, _f32(GRID[7]), ps), op(z, hard, _f32(GRID[7]), ps)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("shape", [(4, 1, 32, 32), (3, 1, 17, 13)])
def test_saturated_logits_and_constant_targets_stay_finite_and_right(shape, ps):
    """|z| in {30, 100}, on the target's side everywhere and on either side at random; all-zero and all-one targets.  Everything is
    finite and the loss is within the bound everywhere.  The gradient is compared where fp32 sums can hold it: not at |z| = 100 (the
    fp64 gradient is 1e-44 or below), and not the Tversky term's where every logit is at +-30 on its target's side — there
    1 - TI = (a FP + b FN) / Den with FP + FN ~ 1e-13 n, which fp32 sums of p next to sums of 1 do not resolve: they give
    1 - TI = 0 exactly, the case with the sub-gradient 0 (test_perfect_saturated_prediction_and_gamma_zero_at_u_zero)."""
    g = torch.Generator().manual_seed(3)
    t = (torch.rand(*shape, generator=g) < 0.5).float()
    flip = torch.rand(*shape, generator=g) < 0.5
    z0 = torch.randn(*shape, generator=g) * 2
    cases = {"all-zero target": (z0, torch.zeros(shape)), "all-one target": (z0, torch.ones(shape))}
    for mag in (30.0, 100.0):
        cases[f"+-{mag:g} agreeing"] = (torch.where(t > 0, mag, -mag), t)
        cases[f"+-{mag:g} mixed"] = (torch.where(flip, mag, -mag), t)
    for tag, (z, t_) in cases.items():
        for cfg in GRID:
            cfg = _f32(cfg)
            ref = R.ftv_loss(z.numpy(), t_.numpy(), **_kw(cfg, ps))
            loss, dz = op(z, t_, cfg, ps, runs=1)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all()), (tag, cfg)
            print(f"{tag} {shape} ps={ps} {cfg}: loss {float(loss):.8f} ref {ref[0]:.8f} |d| {abs(float(loss) - ref[0]):.2e}")
            assert abs(float(loss) - ref[0]) < 1e-5, (tag, cfg, float(loss), ref[0])
            if "100" not in tag and not ("agreeing" in tag and cfg[1] > 0):
                check(f"{tag} {shape} ps={ps} {cfg}", loss, dz, *ref)


@pytest.mark.parametrize("ps", [False, True])
def test_perfect_saturated_prediction_and_gamma_zero_at_u_zero(ps):
    """|z| = 100 on the target's side: p = t exactly, u = 0.  Focal-Tversky (g = 0.75, where (1 - TI)^(g - 1) would be 0^-0.25): the
    loss is finite (0) and the Tversky gradient all zero.  gamma = 0 with u = 0: u^0 = 1, the focal term is BCE's, 0 here; and on the
    WRONG side (u = 1, ce = 100) the loss is 100 alpha_t and the gradient -+alpha_t / n, for every gamma."""
    shape = (3, 1, 17, 13)
    t = _data(shape)[1]
    z = torch.where(t > 0, 100.0, -100.0)
    loss, dz = op(z, t, _f32((0.0, 1.0, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0)), ps)
    assert float(loss) == 0.0 and not bool(dz.any())
    loss, dz = op(z, t, _f32((0.0, 1.0, 0.7, 0.3, 0.75, 0.25, 2.0, 0.0)), ps)          # smooth = 0 as well
    assert float(loss) == 0.0 and not bool(dz.any())
    for gamma in (0.0, 0.5, 2.0):
        loss, dz = op(z, t, _f32((1.0, 0.0, 0.5, 0.5, 1.0, -1.0, gamma, 1.0)), ps)
        assert float(loss) == 0.0 and not bool(dz.any()), gamma
        loss, dz = op(-z, t, _f32((1.0, 0.0, 0.5, 0.5, 1.0, -1.0, gamma, 1.0)), ps)
        want = torch.where(t > 0, -1.0, 1.0) / t.numel()
        assert abs(float(loss) - 100.0) < 1e-5 and rel_err(dz, want) < 1e-6, (gamma, float(loss))
    # mixed with the focal term: the Tversky part of the gradient is still exactly 0, what is left is the focal gradient alone
    both = op(z, t, _f32((0.5, 0.5, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0)), ps)
    alone = op(z, t, _f32((0.5, 0.0, 0.7, 0.3, 0.75, 0.25, 2.0, 1.0)), ps)
    assert torch.equal(both[0], alone[0]) and torch.equal(both[1], alone[1])


@pytest.mark.parametrize("shape", [(2, 1, 96, 172), (3, 1, 17, 13)])
def test_identities_on_the_device(shape):
    from mi355 import nn as mnn
    z, t = _data(shape)
    zd, td = z.to(DEV), t.to(DEV)

    def run(crit):
        a = zd.clone().requires_grad_(True)
        l = crit(a, td)
        l.backward()
        torch.cuda.synchronize()
        return float(l.detach()), a.grad

    for name, new, old in (("FocalLoss(-1, 0) vs BCEWithLogitsLoss", mnn.FocalLoss(alpha=-1, gamma=0), mnn.BCEWithLogitsLoss()),
                           ("TverskyLoss(.5, .5, .5) vs DiceLoss(1)", mnn.TverskyLoss(0.5, 0.5, smooth=0.5), mnn.DiceLoss(smooth=1.0)),
                           ("TverskyLoss(.5, .5, .5, per_sample) vs DiceLoss(1, per_sample)", mnn.TverskyLoss(0.5, 0.5, 0.5, True),
                            mnn.DiceLoss(1.0, True))):
        (la, ga), (lb, gb) = run(new), run(old)
        print(f"{name} {shape}: |dloss| {abs(la - lb):.2e}, dz rel_err {rel_err(ga, gb):.2e}")
        assert abs(la - lb) < 1e-5 and rel_err(ga, gb) < 1e-5


def test_module_surface():
    from mi355 import amp as mamp, nn as mnn
    z = torch.randn(2, 17, 13, device=DEV)
    t = (torch.rand(2, 17, 13, device=DEV) < 0.5).float()
    with pytest.raises(ValueError, match="must match input size"):
        mnn.FocalTverskyLoss()(z, t[:1])
    cfg = _f32(GRID[7])
    l3, g3 = module(z.cpu(), t.cpu(), cfg, True)
    l4, g4 = module(z.cpu()[:, None], t.cpu()[:, None], cfg, True)
    assert torch.equal(l3, l4) and torch.equal(g3.reshape(-1), g4.reshape(-1)) and g3.shape == z.shape
    lu, gu = module(z.cpu(), t.cpu().to(torch.uint8), cfg, False)            # targets of another dtype are converted, as for BCE
    lf, gf = module(z.cpu(), t.cpu(), cfg, False)
    assert torch.equal(lu, lf) and torch.equal(gu, gf)
    # the upstream gradient and the loss scale enter as one factor
    a = z.clone().requires_grad_(True)
    sc = mamp.GradScaler()
    assert sc.get_scale() == 65536.0
    sc.scale(mnn.FocalTverskyLoss(**_kw(cfg))(a, t)).backward()
    torch.cuda.synchronize()
    assert rel_err(a.grad.cpu(), gf * 65536.0) < 1e-6


# ---- mi355_ce_focal ------------------------------------------------------------------------------------------------------------------
def ce_bound(ref):
    """tests/mix_ref.py::ce_bound: one float32 rounding of a value computed in double"""
    return 2.0 ** -23 * np.abs(ref) + 1e-12


@functools.lru_cache(maxsize=None)
def _ce_inputs(B, C):
    rng = np.random.default_rng(100 * B + C)
    z = rng.normal(0, 3, (B, C)).astype(np.float32)
    y = rng.integers(0, C, B)
    z[0] = rng.normal(0, 1, C)
    z[0, 0] += 60.0                                      # one logit 60 above the rest: the true class of row 0 ...
    y[0] = 0
    if B > 1:
        z[B - 1] = z[0]                                  # ... and a wrong class of the last row
        y[B - 1] = C - 1
    w = (0.25 + 2 * rng.random(C)).astype(np.float32)
    return z, y, w


def _gpu_ce_focal(z, y, w, gamma, gscale, want_dz=True):
    from mi355.lib import lib
    B, C = z.shape
    zs = _src(torch.from_numpy(z.copy()))
    yt = torch.from_numpy(np.asarray(y, np.int64).copy()).to(DEV)
    ws = None if w is None else _src(torch.from_numpy(w.copy()))
    gs = None if gscale is None else torch.full((1,), gscale, device=DEV)
    outs = []
    for _ in range(2):
        loss, dz = Guarded(1), Guarded(B * C)
        lib.mi355_ce_focal(zs.t, yt, None if ws is None else ws.t, loss.t, dz.t if want_dz else None, gs, B, C, float(gamma))
        torch.cuda.synchronize()
        assert loss.intact() and dz.intact() and (want_dz or dz.untouched())
        outs.append((loss.t.cpu().clone(), dz.t.cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert zs.intact() and torch.equal(zs.t.cpu().view(B, C), torch.from_numpy(z)) and (ws is None or ws.intact())
    return outs[0][0], outs[0][1].double().numpy().reshape(B, C)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_ce_focal_is_within_one_float32_rounding_of_the_restatement(B, C, weighted):
    from mi355.lib import lib
    z, y, w = _ce_inputs(B, C)
    w = w if weighted else None
    for gamma, gscale in ((0.0, None), (0.5, 1024.0), (2.0, None)):
        ref_loss, ref_dz = R.ce_focal(z, y, w, gamma, 1.0 if gscale is None else gscale)
        loss, dz = _gpu_ce_focal(z, y, w, gamma, gscale)
        e_loss, e_dz = abs(float(loss.double()) - ref_loss), np.abs(dz - ref_dz)
        print(f"B={B} C={C} w={weighted} gamma={gamma} gscale={gscale}: loss {float(loss):.7g} |d| {e_loss:.2e} (bound {ce_bound(ref_loss):.2e}), "
              f"dz worst |d| / bound {(e_dz / ce_bound(ref_dz)).max():.3f}")
        assert e_loss <= ce_bound(ref_loss)
        assert (e_dz <= ce_bound(ref_dz)).all(), np.argwhere(e_dz > ce_bound(ref_dz))[:5].tolist()
        only, _ = _gpu_ce_focal(z, y, w, gamma, gscale, want_dz=False)          # dz = NULL: the loss alone, the same bits
        assert torch.equal(only, loss)
        if gamma == 0.0:                                 # = mi355_ce_mix on hard labels without smoothing
            zt, yt = torch.from_numpy(z.copy()).to(DEV), torch.from_numpy(np.asarray(y, np.int64).copy()).to(DEV)
            wt = None if w is None else torch.from_numpy(w.copy()).to(DEV)
            lm, dm = torch.empty(1, device=DEV), torch.empty(B * C, device=DEV)
            lib.mi355_ce_mix(zt, yt, None, None, wt, lm, dm, None, B, C, 0.0)
            torch.cuda.synchronize()
            assert abs(float(lm.double()) - ref_loss) <= ce_bound(ref_loss) and abs(float(lm.double()) - float(loss.double())) <= ce_bound(ref_loss)
            assert (np.abs(dm.cpu().double().numpy().reshape(B, C) - dz) <= ce_bound(ref_dz)).all()


def test_ce_focal_rows_without_weight_on_the_other_classes_and_the_module():
    from mi355 import nn as mnn
    z = np.array([[800.0, 0.0, -3.0], [0.5, -1.0, 2.0]], np.float32)           # row 0: u = 0 in double
    for gamma in (0.0, 0.5, 2.0):
        ref_loss, ref_dz = R.ce_focal(z, [0, 1], None, gamma)
        loss, dz = _gpu_ce_focal(z, np.array([0, 1]), None, gamma, None)
        assert np.isfinite(float(loss)) and np.isfinite(dz).all() and not dz[0].any()
        assert abs(float(loss.double()) - ref_loss) <= ce_bound(ref_loss) and (np.abs(dz - ref_dz) <= ce_bound(ref_dz)).all()
    zf, y, w = _ce_inputs(257, 3)
    crit = mnn.FocalCrossEntropyLoss(0.5, w)
    a = torch.from_numpy(zf.copy()).to(DEV).requires_grad_(True)
    l = crit(a, torch.from_numpy(y.copy()).to(DEV))
    (3 * l).backward()
    torch.cuda.synchronize()
    lo, do = _gpu_ce_focal(zf, y, w, 0.5, 3.0)
    assert torch.equal(l.detach().cpu().reshape(1), lo) and np.array_equal(a.grad.cpu().double().numpy(), do)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        mnn.FocalCrossEntropyLoss(check_labels=True)(a.detach(), torch.full((257,), 3, device=DEV))


# ---- whole model ---------------------------------------------------------------------------------------------------------------------
FTV_MODEL = dict(focal_weight=0.5, tversky_weight=0.5)


def test_whole_model_gradients_match_fp64_oracle_on_the_same_masks():
    """tests/test_gpu_seg_loss.py's statement and bounds for AttentionUNet 64 x 64 in fp32, under FocalTverskyLoss(0.5, 0.5): logits
    1e-4, loss 1e-5, plan.dout 1e-3, parameter gradients median <= 5e-5, max <= 1e-3, >= 97 % of the tensors <= 3e-4 of their maximum.
    The gradients are right only if dloss/dlogits really landed in the plan's dout buffer."""
    from mi355 import nn as mnn
    from utils.helpers import get_seg_model
    name = "AttentionUNet"
    sd = nets.closed_form_state(name)
    m = get_seg_model("attentionunet")
    m.load_state_dict(sd)
    m.compute_dtype = torch.float32
    m = m.to(DEV).train()
    x, y = otrain.closed_form_input(2, 64)
    out = m(x.to(DEV))
    plan = out._mi355_plan
    loss = mnn.FocalTverskyLoss(**FTV_MODEL)(out, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    relu, pool = gpu_kinks(plan)
    assert len(pool) == 4
    # dloss/dlogits in the plan's own buffer, against the restatement on the GPU's logits
    n = out.numel()
    zg = out.detach().float().cpu().numpy()
    lg, dzg = R.ftv_loss(zg, y.numpy().reshape(zg.shape), **FTV_MODEL)
    check("plan.dout on the GPU's logits", loss.detach().cpu(), plan.dout[:n].cpu().view(zg.shape), lg, dzg)
    # the fp64 oracle replayed on the GPU's ReLU / max-pool decisions
    s64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    pk = nets.param_keys(s64)
    for k in pk:
        s64[k].requires_grad_(True)
    nets.Kinks.start("replay", relu, pool)
    try:
        o64 = nets.NETS[name](s64, x.double(), True)
        if o64.dim() == 3:
            o64 = o64.unsqueeze(1)
        l64, dz64 = R.ftv_loss(o64.detach().numpy(), y.double().numpy(), **FTV_MODEL)
        o64.backward(torch.from_numpy(dz64))
    finally:
        _, _, used = nets.Kinks.stop()
    assert used == (len(relu), len(pool)), (used, len(relu), len(pool))
    o64 = o64.detach()
    g64 = {k: s64[k].grad for k in pk if s64[k].grad is not None}
    e_dout = rel_err(plan.dout[:n].cpu(), torch.from_numpy(dz64).reshape(-1))
    e_out = float((out.detach().cpu().double().reshape(o64.shape) - o64).abs().max() / o64.abs().max())
    print(f"FocalTverskyLoss(0.5, 0.5) AttentionUNet 64: logits {e_out:.2e}, loss |d| {abs(float(loss.detach()) - l64):.2e}, plan.dout {e_dout:.2e}")
    assert e_dout < 1e-3
    assert e_out < 1e-4
    assert abs(float(loss.detach()) - l64) < 1e-5
    gmax = max(float(v.abs().max()) for v in g64.values())
    errs = {}
    for k, p in m.named_parameters():
        ref = g64[k]
        sc = float(ref.abs().max())
        if sc < 1e-6 * gmax:
            assert float(p.grad.abs().max()) <= 1e-5 * gmax, k          # conv bias in front of a train-mode BN: exactly zero
            continue
        errs[k] = float((p.grad.cpu().double() - ref).abs().max()) / sc
    e = np.array(list(errs.values()))
    worst = max(errs, key=errs.get)
    print(f"  parameter gradients: median {np.median(e):.2e}, max {e.max():.2e} ({worst}), {100 * np.mean(e <= 3e-4):.1f} % <= 3e-4")
    assert np.median(e) <= 5e-5, np.median(e)
    assert e.max() <= 1e-3, (worst, errs[worst])
    assert np.mean(e <= 3e-4) >= 0.97, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


# ---- train() -------------------------------------------------------------------------------------------------------------------------
LOG = r"Ep(\d+): TrainLoss ([\d.]+) \| ValLoss ([\d.]+) \| IoU ([\d.]+)"


def test_train_with_focal_tversky_loss_follows_the_cpu_protocol(tmp_path, capsys):
    """helpers.train(criterion=FocalTverskyLoss(0.5, 0.5)) on the fixed synthetic loader of tests/test_gpu_seg_loss.py against a CPU
    fp64 loop built from oracle.nets, oracle.train.AdamW / clip_grad_norm / cosine_lr and tests/focal_ref.py, with the bounds of
    test_train_with_combined_loss_follows_the_cpu_protocol: both sides three-decimal numbers as the log prints them, training loss
    2e-3, validation loss 2e-3 (relative above 1), IoU 5e-3, best validation loss 2e-3 relative."""
    from torch.utils.data import DataLoader, TensorDataset
    from mi355 import nn as mnn
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils import helpers
    name = "AttentionUNet"
    zf = np.load(os.path.join(G, "train_traj_AttentionUNet.npz"))
    hw, epochs, lr = int(zf["hw"]), int(zf["epochs"]), float(zf["lr"])
    b = [otrain.synthetic_batch(4, hw, seed=s) for s in (0, 1, 2)]
    tr = DataLoader(TensorDataset(torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(b[2][0], b[2][1]), batch_size=4, shuffle=False)
    m = AttentionUNet()
    m.load_state_dict(nets.closed_form_state(name))
    m.compute_dtype = torch.float32
    best = helpers.train(m.to(DEV), tr, va, torch.device(DEV), epochs, lr, name, str(tmp_path), seg=True, criterion=mnn.FocalTverskyLoss(**FTV_MODEL))
    rows = re.findall(LOG, capsys.readouterr().out)
    assert len(rows) == epochs
    assert os.path.exists(os.path.join(str(tmp_path), f"{name}_best_loss.pt"))

    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in nets.closed_form_state(name).items()}
    fn = nets.NETS[name]
    pk = nets.param_keys(sd)
    opt = otrain.AdamW(pk, lr)
    b = [(x.double(), y.double()) for x, y in b]
    train_b, val_b = b[:2], b[2:]
    n_train, n_val = sum(x.shape[0] for x, _ in train_b), sum(x.shape[0] for x, _ in val_b)
    hist, ref_best = [], float("inf")
    for ep in range(1, epochs + 1):
        run = 0.0
        for x, y in train_b:
            for k in pk:
                sd[k].requires_grad_(True)
                sd[k].grad = None
            out = fn(sd, x, True)
            if out.dim() == 3:
                out = out.unsqueeze(1)
            l, dz = R.ftv_loss(out.detach().numpy(), y.numpy(), **FTV_MODEL)
            out.backward(torch.from_numpy(dz).to(out.dtype))
            grads = {k: sd[k].grad.detach().clone() for k in pk if sd[k].grad is not None}
            for k in pk:
                sd[k].requires_grad_(False)
                sd[k].grad = None
            otrain.clip_grad_norm(list(grads.values()), 1.0)
            with torch.no_grad():
                opt.step(sd, grads)
            run += l * x.shape[0]
        vl = vm = 0.0
        with torch.no_grad():
            for x, y in val_b:
                out = fn(sd, x, False)
                vl += R.ftv_loss(out.numpy().reshape(y.shape), y.numpy(), **FTV_MODEL)[0] * x.shape[0]
                vm += otrain.iou_train(torch.sigmoid(out).reshape(y.shape), y)
        vl /= n_val
        hist.append((run / n_train, vl, vm / len(val_b)))
        opt.lr = otrain.cosine_lr(lr, ep, epochs)
        ref_best = min(ref_best, vl)
    for row, ref in zip(rows, hist):
        got = [float(v) for v in row]
        ref = tuple(float(f"{v:.3f}") for v in ref)            # what the CPU loop's own log line would print
        print(f"Ep{int(got[0])}: GPU train {got[1]:.3f} val {got[2]:.3f} IoU {got[3]:.3f} | CPU train {ref[0]:.4f} val {ref[1]:.4f} IoU {ref[2]:.4f}")
        assert abs(got[1] - ref[0]) <= 2e-3 + 1e-9 and abs(got[2] - ref[1]) <= 2e-3 * max(1, ref[1]) + 1e-9 and \
            abs(got[3] - ref[2]) <= 5e-3 + 1e-9, (got, ref)
    assert abs(best - ref_best) < 2e-3 * ref_best


def test_train_one_classifier_epoch_with_focal_cross_entropy(tmp_path, capsys):
    """One epoch of helpers.train on ResNet18 (a plain Linear head: no dropout draw to match), 8 synthetic 64 x 64 samples in two
    batches, under FocalCrossEntropyLoss(2, weight): stage 1 trains the head alone with AdamW(1e-4).  The CPU loop is the same protocol
    in fp64 from oracle.nets / oracle.train and tests/focal_ref.py; the printed training loss is within 2e-3 of it."""
    from torch.utils.data import DataLoader, TensorDataset
    from mi355 import nn as mnn
    from models.classification_models.ResNet import ResNet18
    from utils import helpers
    name = "ResNet18"
    w = np.array([0.5, 2.0, 1.25], np.float32)
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(12, 3, 64, 64, generator=gen), torch.randint(0, 3, (12,), generator=gen)
    tr = DataLoader(TensorDataset(x[:8], y[:8]), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(x[8:], y[8:]), batch_size=4, shuffle=False)
    state = nets.closed_form_state(name)
    m = ResNet18(num_classes=3)
    m.load_state_dict(state)
    m.compute_dtype = torch.float32
    helpers.train(m, tr, va, torch.device(DEV), 1, 1e-4, name, str(tmp_path), seg=False, cls_head_name="fc",
                  criterion=mnn.FocalCrossEntropyLoss(2.0, w))
    rows = re.findall(r"Ep1: TrainLoss ([\d.]+) \(Acc ([\d.]+)%\) \| ValLoss ([\d.]+) \|", capsys.readouterr().out)
    assert len(rows) == 1
    got_train, got_val = float(rows[0][0]), float(rows[0][2])

    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    head = ["fc.weight", "fc.bias"]
    opt = otrain.AdamW(head, 1e-4)
    run = 0.0
    for lo in (0, 4):
        xb, yb = x[lo:lo + 4].double(), y[lo:lo + 4]
        for k in head:
            sd[k].requires_grad_(True)
            sd[k].grad = None
        out = nets.NETS[name](sd, xb, True)
        l, dz = R.ce_focal(out.detach().numpy(), yb.numpy(), w, 2.0)
        out.backward(torch.from_numpy(dz))
        grads = {k: sd[k].grad.detach().clone() for k in head}
        for k in head:
            sd[k].requires_grad_(False)
            sd[k].grad = None
        otrain.clip_grad_norm(list(grads.values()), 1.0)
        with torch.no_grad():
            opt.step(sd, grads)
        run += l * 4
    print(f"GPU train {got_train:.3f} val {got_val:.3f} | CPU train {run / 8:.4f}")
    assert abs(got_train - float(f"{run / 8:.3f}")) <= 2e-3 + 1e-9, (got_train, run / 8)
    assert np.isfinite(got_val)
