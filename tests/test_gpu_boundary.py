"""-m gpu: the boundary loss on the device — the signed squared distance map (csrc/boundary.hip, utils/distance.py), the loss and
its gradient (mi355.nn.BoundaryLoss / RegionBoundaryLoss), and the way through train().

Yardsticks: tests/boundary_ref.py (integers for the map, fp64 for the loss; pinned to scipy and to tests/golden/boundary_loss.npz
on the CPU, tests/test_boundary_cpu.py) and tests/seg_loss_ref.py for the regional part.  The map is compared bit for bit.  Loss
bounds follow tests/test_gpu_seg_loss.py: rel_err(dz, ref) < 1e-5 and |loss - ref| < 1e-5 * max(1, A) with A = weight * mean |p phi|
in fp64 — relative, because this loss is a mean distance and not O(1) (torch's own fp32 evaluation of the restatement sits at
5e-8 * A on the CPU at (4, 64, 64))."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import boundary_ref as R
import seg_loss_ref as S
from gpu_util import gpu_kinks, rel_err
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")


# ---- the C ABI as a caller sees it -------------------------------------------------------------------------------------------
def op_map(t, thr=0.5):
    """float [B, H, W] device tensor -> int32 [B, H, W]"""
    B, H, W = t.shape
    n = lib.raw("mi355_sdist_ws_ints")(B, H, W)
    assert n >= B * H * W
    ws = torch.full((n + 16,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)      # 16 guard words behind the workspace
    sd2 = torch.full((B * H * W + 16,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    lib.mi355_signed_dist2(t, B, H, W, thr, ws, n, sd2)
    torch.cuda.synchronize()
    assert bool((ws[n:] == 0x5a5a5a5a).all()) and bool((sd2[B * H * W:] == 0x5a5a5a5a).all()), "wrote behind its buffers"
    return sd2[: B * H * W].view(B, H, W)


def op_fwd(z, sd2, weight, base=None):
    B, per = z.shape[0], z.numel() // z.shape[0]
    rows = lib.mi355_boundary_loss_rows(B, per)
    assert rows >= B
    partial = torch.empty(rows, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    lib.mi355_boundary_loss_fwd(z, sd2, B, per, weight, base, partial, loss)
    torch.cuda.synchronize()
    return loss


def op_bwd(z, sd2, weight, gscale=None, accumulate=0, dz=None):
    B, per = z.shape[0], z.numel() // z.shape[0]
    dz = torch.empty_like(z) if dz is None else dz
    lib.mi355_boundary_loss_bwd(z, sd2, B, per, weight, gscale, accumulate, dz)
    torch.cuda.synchronize()
    return dz


def op_seg(z, t, bw, dw, sm, ps, gscale=None):
    B, per = z.shape[0], z.numel() // z.shape[0]
    rows = lib.mi355_seg_loss_rows(B, per)
    partial = torch.empty(rows * 4, dtype=torch.float32, device=DEV)
    state = torch.empty(2 * B, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    lib.mi355_seg_loss_fwd(z, t, B, per, bw, dw, sm, 1 if ps else 0, partial, state, loss)
    dz = torch.empty_like(z)
    lib.mi355_seg_loss_bwd(z, t, B, per, bw, state, gscale, dz)
    torch.cuda.synchronize()
    return loss, dz


def module(crit, z, t, factor=None):
    zz = z.clone().requires_grad_(True)
    loss = crit(zz, t)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (loss if factor is None else factor * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), zz.grad


def check(tag, loss, dz, l64, g64, A):
    l, e = float(loss), rel_err(dz.cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(g64)).reshape(-1))
    print(f"{tag}: loss {l:.8f} ref {l64:.8f} |d| {abs(l - l64):.2e} = {abs(l - l64) / max(A, 1e-300):.2e} A (A = {A:.4f})  dz rel_err {e:.2e}")
    assert np.isfinite(l) and bool(torch.isfinite(dz).all()), tag
    assert abs(l - l64) < 1e-5 * max(1.0, A), (tag, l, l64, A)
    assert e < 1e-5, (tag, e)


# ---- 1. the map, exact ----------------------------------------------------------------------------------------------------------
def _mask_kinds(B, H, W, seed):
    rng = np.random.RandomState(seed)
    kinds = {f"p{p}": rng.rand(B, H, W) < p for p in (0.02, 0.5, 0.98)}
    kinds["empty"], kinds["full"] = np.zeros((B, H, W), dtype=bool), np.ones((B, H, W), dtype=bool)
    kinds["checkerboard"] = np.broadcast_to((np.add.outer(np.arange(H), np.arange(W)) & 1).astype(bool), (B, H, W)).copy()
    return kinds


def _ellipses():
    return np.stack([R.ellipse(256, 256, 120, 130, 60, 45) | R.ellipse(256, 256, 30, 200, 9, 14)])


@functools.lru_cache(maxsize=None)
def _map_cases(shape):
    """[(tag, mask bool [B, H, W], restatement int32 [B, H, W])], computed once per shape"""
    B, H, W = shape
    if (H, W) == (1024, 1024):
        a = np.zeros((1, H, W), dtype=bool)
        a[0, H - 1, 0] = True                                  # a corner: the farthest pixel is 2 * 1023^2 away
        kinds = {"corner_pixel": a, "corner_background_pixel": ~a, "empty": np.zeros_like(a), "full": np.ones_like(a)}
    else:
        kinds = _mask_kinds(B, H, W, 17 * H + W)
        if (H, W) == (256, 256):
            kinds["ellipses"] = _ellipses()
            kinds["ellipse_cut_by_the_frame"] = np.stack([R.ellipse(256, 256, 10, 250, 40, 30)])
    return [(k, m, R.signed_dist2(m)) for k, m in kinds.items()]


MAP_SHAPES = [(1, 1, 1), (3, 17, 13), (2, 1, 9), (2, 8, 1), (2, 65, 130), (1, 1023, 67), (1, 256, 256), (1, 1024, 1024)]


@pytest.mark.parametrize("shape", MAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_is_exact(shape):
    from utils import distance
    for tag, m, ref in _map_cases(shape):
        want = torch.from_numpy(ref)
        t = torch.from_numpy(m).float().to(DEV)
        got = op_map(t)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (shape, tag, int((got.cpu() != want).sum()))
        # the threshold is strict, as in surface_on: 0.5 is background
        soft = torch.where(t > 0, 0.75, 0.5)
        assert torch.equal(op_map(soft).cpu(), want), (shape, tag, "threshold")
        # the Python surface on the same input, in every accepted layout
        for view in (t, t[:, None]) + ((t[0],) if shape[0] == 1 else ()):
            d2 = distance.signed_distance2(view)
            assert d2.dtype == torch.int32 and d2.shape == t.shape and d2.is_cuda and torch.equal(d2.cpu(), want), (shape, tag)
        # phi = torch.sqrt of the exact integers in fp32, on the device it is computed on (torch's fp32 square root is not correctly
        # rounded everywhere — this build's CPU one differs from IEEE in 0.5 % of the integers below 2^21 — so "the same bits" names
        # the evaluator), and within two ulp of the fp64 restatement (one for the square root, half a one for 1 - r)
        phi = distance.signed_distance_map(t[:, None])
        wd = want.to(DEV)
        r = torch.sqrt(wd.abs().float())
        want_phi = torch.where(wd > 0, r, torch.where(wd < 0, -(r - 1.0), torch.zeros_like(r)))
        assert phi.dtype == torch.float32 and phi.is_cuda and phi.shape == t.shape and torch.equal(phi, want_phi), (shape, tag)
        p64 = torch.from_numpy(R.phi(ref))
        assert bool(((phi.cpu().double() - p64).abs() <= 2.0 ** -22 * p64.abs().clamp(min=1.0)).all()), (shape, tag)
    if shape == (1, 1024, 1024):
        assert int(_map_cases(shape)[0][2].max()) == 2 * 1023 ** 2 and int(_map_cases(shape)[1][2].min()) == -2 * 1023 ** 2


@pytest.mark.parametrize("hw", [(17, 13), (65, 130)])
def test_samples_of_a_batch_do_not_leak_into_each_other(hw):
    H, W = hw
    n1, n2 = R.noise(H, W, 0.3, 1), R.ellipse(H, W, H / 2, W / 3, H / 3, W / 4)
    batch = np.stack([np.zeros((H, W), dtype=bool), n1, np.ones((H, W), dtype=bool), n2])
    got = op_map(torch.from_numpy(batch).float().to(DEV)).cpu()
    assert not got[0].any() and not got[2].any()
    for i in range(4):
        alone = op_map(torch.from_numpy(batch[i:i + 1]).float().to(DEV)).cpu()
        assert torch.equal(got[i:i + 1], alone), i
        assert torch.equal(alone[0], torch.from_numpy(R.signed_dist2(batch[i]))), i


# ---- 2. loss and gradient against fp64 ------------------------------------------------------------------------------------------
def test_fixture_parity_through_the_abi_and_both_modules():
    from mi355 import nn as mnn
    stored = R.load_fixture(os.path.join(G, "boundary_loss.npz"))
    cases = {c[0]: c for c in R.fixture_cases()}
    assert len(stored) >= 24
    for name, T, sd2, w, l64, g64 in stored:
        z = torch.from_numpy(cases[name][2]).to(DEV)
        t = torch.from_numpy(T).float().to(DEV)
        A = R.mean_abs_term(cases[name][2], sd2, w)
        got = op_map(t)
        assert torch.equal(got.cpu(), torch.from_numpy(sd2)), name
        check(f"abi {name}", op_fwd(z, got, w), op_bwd(z, got, w), l64, g64, A)
        check(f"module {name}", *module(mnn.BoundaryLoss(w), z, t), l64, g64, A)
        lr, gr, Ar = R.region_boundary(cases[name][2], T, 0.5, 0.5, w, sd2=sd2)
        check(f"RegionBoundaryLoss(0.5, 0.5, {w}) {name}", *module(mnn.RegionBoundaryLoss(0.5, 0.5, w), z, t), lr, gr, Ar)


@functools.lru_cache(maxsize=None)
def _big(shape, seed=11):
    """-> (z fp32 [B,1,H,W], t fp32 [B,1,H,W], sd2 int32 [B,H,W]): logits 2 randn; targets are ellipses cut by the frame (what a
    trainer sees), every fourth sample noise, one sample empty where the batch has room for it"""
    B, _, H, W = shape
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(*shape, generator=g) * 2.0).float()
    rng = np.random.RandomState(seed)
    m = np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        if b % 4 == 3 or B < 4:
            m[b] = rng.rand(H, W) < 0.35
        else:
            m[b] = R.ellipse(H, W, rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 8, H / 3), rng.uniform(W / 8, W / 3))
    if B >= 8:
        m[5] = False
    return z, torch.from_numpy(m).float()[:, None], R.signed_dist2(m)


BIG = [(32, 1, 256, 256), (1, 1, 64, 64), (3, 1, 17, 13)]


@pytest.mark.parametrize("shape", BIG, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_fp64_restatement(shape):
    from mi355 import nn as mnn
    z, t, sd2 = _big(shape)
    zd, td = z.to(DEV), t.to(DEV)
    got = op_map(td[:, 0].contiguous())
    assert torch.equal(got.cpu(), torch.from_numpy(sd2))
    for w in (1.0, 0.01):
        ref = R.boundary_loss(z.numpy(), sd2, w)
        A = R.mean_abs_term(z.numpy(), sd2, w)
        check(f"abi {shape} w={w}", op_fwd(zd, got, w), op_bwd(zd, got, w), *ref, A)
        check(f"module {shape} w={w}", *module(mnn.BoundaryLoss(w), zd, td), *ref, A)
        # the regional + boundary node: the base-added forward and the accumulating backward at this grid
        check(f"RegionBoundaryLoss(0.5, 0.5, {w}) {shape}", *module(mnn.RegionBoundaryLoss(0.5, 0.5, w), zd, td),
              *R.region_boundary(z.numpy(), t.numpy(), 0.5, 0.5, w, sd2=sd2))
    # `base` is added on the device
    base = torch.tensor([0.625], device=DEV)
    ref = R.boundary_loss(z.numpy(), sd2, 1.0)
    l = float(op_fwd(zd, got, 1.0, base))
    assert abs(l - (0.625 + ref[0])) < 1e-5 * max(1.0, R.mean_abs_term(z.numpy(), sd2, 1.0)), (l, ref[0])


@pytest.mark.parametrize("shape", [(4, 1, 32, 32), (3, 1, 17, 13)], ids=lambda s: "x".join(map(str, s)))
def test_saturated_logits_stay_finite_and_right(shape):
    from mi355 import nn as mnn
    _, t, _ = _big(shape, 3)
    sd2 = R.signed_dist2(t.numpy()[:, 0] > 0.5)
    flip = torch.rand(*shape, generator=torch.Generator().manual_seed(4)) < 0.5
    for tag, z in (("+-30 agreeing", torch.where(t > 0, 30.0, -30.0)), ("+-30 opposing", torch.where(t > 0, -30.0, 30.0)),
                   ("+-30 mixed", torch.where(flip, 30.0, -30.0))):
        ref = R.boundary_loss(z.numpy(), sd2, 1.0)
        A = R.mean_abs_term(z.numpy(), sd2, 1.0)
        zd = z.to(DEV)
        check(f"abi {tag} {shape}", op_fwd(zd, torch.from_numpy(sd2).to(DEV), 1.0), op_bwd(zd, torch.from_numpy(sd2).to(DEV), 1.0), *ref, A)
        check(f"module {tag} {shape}", *module(mnn.BoundaryLoss(), zd, t.to(DEV)), *ref, A)
        check(f"RegionBoundaryLoss(0.5, 0.5, 1.0) {tag} {shape}", *module(mnn.RegionBoundaryLoss(0.5, 0.5, 1.0), zd, t.to(DEV)),
              *R.region_boundary(z.numpy(), t.numpy(), 0.5, 0.5, 1.0, sd2=sd2))


# ---- 3. one node, the right sum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 1, 64, 64), (3, 1, 17, 13)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ps", [False, True])
def test_region_boundary_is_the_sum_of_its_two_restatements(shape, ps):
    from mi355 import nn as mnn
    z, t, _ = _big(shape, 23)
    zd, td = z.to(DEV), t.to(DEV)
    for bw, dw, w in ((0.5, 0.5, 0.01), (1.0, 0.0, 0.3), (0.0, 1.0, 1.0)):
        for sched, epochs in (("constant", (0, 5, 200)), ("rebalance", (0, 5, 200))):
            for ep in epochs:
                crit = mnn.RegionBoundaryLoss(bw, dw, w, per_sample=ps, schedule=sched)
                crit.on_epoch(ep, 300)
                assert crit.current_weights() == pytest.approx(R.schedule_weights(w, sched, ep), abs=1e-15)
                l64, g64, A = R.region_boundary(z.numpy(), t.numpy(), bw, dw, w, 1.0, ps, sched, ep)
                check(f"RegionBoundaryLoss({bw}, {dw}, {w}, per_sample={ps}, {sched}) epoch {ep} {shape}", *module(crit, zd, td), l64, g64, A)


@pytest.mark.parametrize("shape", [(4, 1, 64, 64), (3, 1, 17, 13)], ids=lambda s: "x".join(map(str, s)))
def test_accumulate_adds_and_overwrite_overwrites(shape):
    z, t, sd2 = _big(shape, 29)
    zd, td, sd = z.to(DEV), t.to(DEV), torch.from_numpy(sd2).to(DEV)
    term = op_bwd(zd, sd, 0.3)
    poisoned = torch.full_like(zd, float("nan"))
    assert torch.equal(op_bwd(zd, sd, 0.3, dz=poisoned), term)                       # accumulate = 0 ignores what dz held
    known = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    acc = op_bwd(zd, sd, 0.3, accumulate=1, dz=known.clone())
    assert torch.equal(acc, known + term)                                            # one fp32 addition of the rounded term
    # the two launches of RegionBoundaryLoss's backward against the two gradients formed separately
    _, seg = op_seg(zd, td, 0.5, 0.5, 1.0, False)
    both = op_bwd(zd, sd, 0.3, accumulate=1, dz=seg.clone())
    e = rel_err(both, seg + term)
    print(f"seg bwd, then boundary bwd accumulating {shape}: rel_err {e:.2e}")
    assert e < 1e-6


# ---- 4. scale and reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 1, 64, 64), (3, 1, 17, 13)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("factor", [3.0, 65536.0])
def test_upstream_gradient_and_loss_scale_enter_as_one_factor(shape, factor):
    from mi355 import amp as mamp, nn as mnn
    z, t, sd2 = _big(shape, 41)
    zd, td, sd = z.to(DEV), t.to(DEV), torch.from_numpy(sd2).to(DEV)
    base = op_bwd(zd, sd, 0.3)
    assert torch.equal(base, op_bwd(zd, sd, 0.3, gscale=torch.ones(1, device=DEV)))
    e = rel_err(op_bwd(zd, sd, 0.3, gscale=torch.full((1,), factor, device=DEV)), base * factor)
    print(f"gscale {factor:g} at the op {shape}: rel_err {e:.2e}")
    assert e < 1e-6
    for crit in (mnn.BoundaryLoss(0.3), mnn.RegionBoundaryLoss(boundary_weight=0.3)):
        _, one = module(crit, zd, td)
        a = zd.clone().requires_grad_(True)
        loss = crit(a, td)
        if factor == 3.0:
            (3 * loss).backward()
        else:
            sc = mamp.GradScaler()
            assert sc.get_scale() == 65536.0
            sc.scale(loss).backward()
        torch.cuda.synchronize()
        e = rel_err(a.grad, one * factor)
        print(f"factor {factor:g} through autograd, {type(crit).__name__} {shape}: rel_err {e:.2e}")
        assert e < 1e-6


def test_loss_and_gradient_are_bit_reproducible():
    from mi355 import nn as mnn
    z, t, sd2 = _big((32, 1, 256, 256))
    zd, td = z.to(DEV), t.to(DEV)
    m0 = op_map(td[:, 0].contiguous())
    l0, d0 = op_fwd(zd, m0, 0.3), op_bwd(zd, m0, 0.3)
    for _ in range(2):
        m1 = op_map(td[:, 0].contiguous())
        assert torch.equal(m0, m1) and torch.equal(l0, op_fwd(zd, m1, 0.3)) and torch.equal(d0, op_bwd(zd, m1, 0.3))
    for crit in (mnn.BoundaryLoss(0.3), mnn.RegionBoundaryLoss(boundary_weight=0.3, per_sample=True)):
        runs = [module(crit, zd, td) for _ in range(3)]
        assert all(torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]) for r in runs[1:]), type(crit).__name__
    lb, db = module(mnn.BoundaryLoss(0.3), zd, td)
    assert torch.equal(lb.reshape(1), l0) and torch.equal(db, d0)


def test_layouts_dtypes_and_errors():
    from mi355 import nn as mnn
    z = torch.randn(2, 17, 13, device=DEV)
    t = (torch.rand(2, 17, 13, device=DEV) < 0.5).float()
    for crit in (mnn.BoundaryLoss(), mnn.RegionBoundaryLoss(boundary_weight=0.3)):
        with pytest.raises(ValueError, match="must match input size"):
            crit(z, t[:1])
        with pytest.raises(ValueError, match="one-channel"):
            crit(torch.zeros(2, 2, 17, 13, device=DEV), torch.zeros(2, 2, 17, 13, device=DEV))
        l3, g3 = module(crit, z, t)
        l4, g4 = module(crit, z[:, None], t[:, None])
        assert torch.equal(l3, l4) and torch.equal(g3.reshape(-1), g4.reshape(-1)) and g3.shape == z.shape
        lu, gu = module(crit, z, t.to(torch.uint8))            # targets of another dtype are converted, as for CombinedLoss
        assert torch.equal(lu, l3) and torch.equal(gu, g3)
    # a boundary weight of 0 is CombinedLoss, bit for bit
    l0, g0 = module(mnn.RegionBoundaryLoss(0.3, 0.7, 0.0), z, t)
    lc, gc = module(mnn.CombinedLoss(0.3, 0.7), z, t)
    assert torch.equal(l0, lc) and torch.equal(g0, gc)


# ---- 5. whole model ---------------------------------------------------------------------------------------------------------------
def _replayed_oracle_with_loss(name, sd, x, y, relu, pool, **kw):
    """fp64 oracle forward + backward on the GPU's own ReLU / max-pool decisions (tests/test_gpu_seg_loss.py), the loss and
    dloss/dlogits from tests/boundary_ref.py -> (loss, logits, dlogits, grads)."""
    s64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    pk = nets.param_keys(s64)
    for k in pk:
        s64[k].requires_grad_(True)
    nets.Kinks.start("replay", relu, pool)
    try:
        o64 = nets.NETS[name](s64, x.double(), True)
        if o64.dim() == 3:
            o64 = o64.unsqueeze(1)
        l64, dz, _ = R.region_boundary(o64.detach().numpy(), y.double().numpy(), **kw)
        o64.backward(torch.from_numpy(dz))
    finally:
        _, _, used = nets.Kinks.stop()
    assert used == (len(relu), len(pool)), (used, len(relu), len(pool))
    return l64, o64.detach(), dz, {k: s64[k].grad for k in pk if s64[k].grad is not None}


@pytest.mark.parametrize("ps", [False, True])
def test_whole_model_gradients_match_fp64_oracle_on_the_same_masks(ps):
    """tests/test_gpu_seg_loss.py's statement and bounds for AttentionUNet 64 x 64 with RegionBoundaryLoss(boundary_weight=0.3):
    logits 1e-4, loss 1e-5, parameter gradients median <= 5e-5, max <= 1e-3, >= 97 % of the tensors <= 3e-4 of their maximum.  The
    gradients are right only if BOTH backward launches landed in the plan's dout buffer, the second on top of the first."""
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
    loss = mnn.RegionBoundaryLoss(boundary_weight=0.3, per_sample=ps)(out, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    relu, pool = gpu_kinks(plan)
    kw = dict(bce_weight=0.5, dice_weight=0.5, boundary_weight=0.3, smooth=1.0, per_sample=ps)
    l64, o64, dz64, g64 = _replayed_oracle_with_loss(name, sd, x, y, relu, pool, **kw)
    assert len(pool) == 4
    n = out.numel()
    e_dout = rel_err(plan.dout[:n].cpu(), torch.from_numpy(dz64).reshape(-1))
    # neither term alone is what the buffer holds
    region_only = S.seg_loss(o64.numpy(), y.double().numpy(), 0.5, 0.5, 1.0, ps)[1]
    assert rel_err(torch.from_numpy(region_only).reshape(-1), torch.from_numpy(dz64).reshape(-1)) > 1e-2
    e_out = float((out.detach().cpu().double().reshape(o64.shape) - o64).abs().max() / o64.abs().max())
    print(f"RegionBoundaryLoss(0.3, per_sample={ps}) AttentionUNet 64: logits {e_out:.2e}, loss {float(loss.detach()):.6f} ref {l64:.6f} "
          f"|d| {abs(float(loss.detach()) - l64):.2e}, plan.dout {e_dout:.2e}")
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


# ---- 6. through train() -----------------------------------------------------------------------------------------------------------
LOG = r"Ep(\d+): TrainLoss ([\d.]+|nan|inf) \| ValLoss ([\d.]+|nan|inf) \| IoU ([\d.]+|nan)"


def _loaders():
    from torch.utils.data import DataLoader, TensorDataset
    b = [otrain.synthetic_batch(4, 64, seed=s) for s in (0, 1, 2)]
    tr = DataLoader(TensorDataset(torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(b[2][0], b[2][1]), batch_size=4, shuffle=False)
    return tr, va


def _fresh_model():
    from models.segmentation_models.AttentionUNet import AttentionUNet
    m = AttentionUNet()
    m.load_state_dict(nets.closed_form_state("AttentionUNet"))
    m.compute_dtype = torch.float32
    return m.to(DEV)


def _run(crit, path, capsys):
    from utils import helpers
    tr, va = _loaders()
    m = _fresh_model()
    best = helpers.train(m, tr, va, torch.device(DEV), 3, 1e-3, "AttentionUNet", str(path), seg=True, criterion=crit)
    text = re.sub(r"finished in [\d.]+ minutes", "finished", capsys.readouterr().out)
    return best, text, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_train_drives_the_schedule_and_leaves_other_criteria_alone(tmp_path, capsys):
    from mi355 import nn as mnn

    class Recording(mnn.RegionBoundaryLoss):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.used = [], []

        def on_epoch(self, epoch, epochs=None):
            super().on_epoch(epoch, epochs)
            self.calls.append((epoch, epochs))

        def forward(self, out, target):
            self.used.append((len(self.calls), self.current_weights()))
            return super().forward(out, target)

    crit = Recording(schedule="rebalance")
    best, text, _ = _run(crit, tmp_path / "rebalance", capsys)
    assert crit.calls == [(0, 3), (1, 3), (2, 3)]
    # two training batches and one validation batch per epoch, all under that epoch's factors
    assert [n for n, _ in crit.used] == [1] * 3 + [2] * 3 + [3] * 3
    for (n, got), want in zip(crit.used[::3], ((0.99, 0.01), (0.98, 0.02), (0.97, 0.03))):
        assert got == pytest.approx(want, abs=1e-12), (n, got)
    rows = re.findall(LOG, text)
    assert len(rows) == 3 and all(np.isfinite(float(v)) for r in rows for v in r[1:]), text
    assert np.isfinite(best)
    # a boundary weight of 0 is CombinedLoss (which has no on_epoch, and trains as before), bit for bit
    zero = Recording(boundary_weight=0.0, schedule="constant")
    b0, t0, s0 = _run(zero, tmp_path / "zero", capsys)
    assert not hasattr(mnn.CombinedLoss(), "on_epoch")
    b1, t1, s1 = _run(mnn.CombinedLoss(), tmp_path / "combined", capsys)
    assert zero.calls == [(0, 3), (1, 3), (2, 3)]
    assert len(re.findall(LOG, t1)) == 3
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert t0 == t1 and b0 == b1
    # and the boundary term does change the trajectory when it is on
    assert text != t1
