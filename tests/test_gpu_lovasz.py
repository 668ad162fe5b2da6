"""GPU: the Lovasz hinge (csrc/lovasz.hip on csrc/segsort.hip) through the C ABI, mi355.nn.LovaszHingeLoss / RegionLovaszLoss,
utils/lovasz.py, a whole model and train(), against the fp64 restatement tests/lovasz_ref.py on the same fp32 inputs.

Bounds.  loss: |loss - ref| < 1e-5 max(1, |ref|), the project's bound for its other losses.  Gradient, per ELEMENT:
|dz_i - ref_i| <= 4 * 2^-24 |ref_i| and dz_i == 0 exactly where ref_i == 0 — the coefficient is formed in double from exact integers,
rounded once to fp32 and multiplied once by gscale: two roundings, <= 2 * 2^-24; the test allows twice that."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import lovasz_ref as R
import seg_loss_ref as S
from gpu_util import gpu_kinks, rel_err
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
EPS = 2.0 ** -24
SHAPES = [(3, 1, 17, 13), (1, 1, 1, 1), (2, 1, 64, 64), (32, 1, 256, 256)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)      # noqa: E731


def f32(w):
    return float(np.float32(w))                            # the weight as the ABI's float argument holds it


# ---- the C ABI as a caller sees it -------------------------------------------------------------------------------------------
def op_fwd(z, t, per_image, weight, thr=0.5, base=None):
    """device fp32 tensors -> (loss [1], coef [n]); the workspace and coef sit between guard words."""
    B, n = z.shape[0], z.numel()
    Sg, ln = (B, n // B) if per_image else (1, n)
    need = lib.raw("mi355_lovasz_ws_ints")(Sg, ln)
    assert need > 0, lib.raw("mi355_last_error")()
    ws = torch.full((need + 16,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    coef = torch.full((n + 16,), 7.0, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    z0, t0 = z.clone(), t.clone()
    lib.mi355_lovasz_fwd(z, t, Sg, ln, thr, weight, base, ws, need, coef, loss)
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5a5a5a5a).all()) and bool((coef[n:] == 7.0).all()), "wrote behind its buffers"
    assert torch.equal(z.view(torch.int32), z0.view(torch.int32)) and torch.equal(t, t0)
    return loss, coef[:n]


def op_bwd(coef, gscale=None, accumulate=0, dz=None):
    n = coef.numel()
    dz = torch.empty(n, dtype=torch.float32, device=DEV) if dz is None else dz
    lib.mi355_lovasz_bwd(coef, n, gscale, accumulate, dz)
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


def check(tag, loss, dz, l64, g64, factor=1.0):
    l = float(loss)
    got = dz.detach().cpu().double().numpy().reshape(-1)
    ref = np.asarray(g64, dtype=np.float64).reshape(-1) * factor
    nz = ref != 0
    worst = float((np.abs(got - ref)[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0
    print(f"{tag}: loss {l:.8f} ref {l64:.8f} |d| {abs(l - l64):.2e}  dz worst element {worst / EPS:.2f} x 2^-24, "
          f"{int((~nz).sum())} zeros of {ref.size}")
    assert np.isfinite(l) and np.isfinite(got).all(), tag
    assert abs(l - l64) < 1e-5 * max(1.0, abs(l64)), (tag, l, l64)
    assert (got[~nz] == 0).all(), (tag, "non-zero where the reference is zero")
    assert (np.abs(got - ref) <= 4 * EPS * np.abs(ref)).all(), (tag, worst / EPS)


# ---- inputs and their references, computed once ----------------------------------------------------------------------------------
KINDS = ("random", "quantised", "all_zero_target", "all_one_target")


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    rng = np.random.RandomState(sum(shape) + len(kind))
    z = (rng.randn(*shape) * 2.0).astype(np.float32)
    if kind == "quantised":
        z = (np.round(rng.randn(*shape) * 4.0) / 4.0).astype(np.float32)
    t = (rng.rand(*shape) < 0.35).astype(np.float32)
    if kind == "all_zero_target":
        t[:] = 0
    if kind == "all_one_target":
        t[:] = 1
    z.setflags(write=False)
    t.setflags(write=False)
    return z, t


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, per_image):
    z, t = _case(shape, kind)
    l, g = R.lovasz_ref(z, t, 1.0, per_image)
    g.setflags(write=False)
    return l, g


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)            # (a copy: the cached inputs are read-only)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
def test_fixture_parity_through_the_abi_and_the_module():
    from mi355 import nn as mnn
    fx = np.load(os.path.join(G, "lovasz.npz"))
    for key in (str(k) for k in fx["cases"]):
        name, mode = key.rsplit("__", 1)
        z, t = fx["z__" + name], fx["t__" + name].astype(np.float32)
        per_image = mode == "image"
        l64, g64 = R.lovasz_ref(z, t, 1.0, per_image)
        assert abs(l64 - float(fx["loss__" + key])) <= 1e-12
        zd, td = _dev(z), _dev(t)
        loss, coef = op_fwd(zd, td, per_image, 1.0)
        check(f"fixture {key} ABI", loss, op_bwd(coef), l64, g64)
        check(f"fixture {key} vs the paper's transcription", loss, coef, float(fx["loss__" + key]), g64)
        lm, gm = module(mnn.LovaszHingeLoss(per_image=per_image), zd, td)
        check(f"fixture {key} module", lm, gm, l64, g64)


@pytest.mark.parametrize("weight", [1.0, 0.3])
@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_parity_with_the_fp64_restatement(shape, per_image, weight):
    from mi355 import nn as mnn
    from utils import lovasz as UL
    w = f32(weight)
    for kind in KINDS:
        z, t = _case(shape, kind)
        l1, g1 = _ref(shape, kind, per_image)
        zd, td = _dev(z), _dev(t)
        tag = f"{ids(shape)} {kind} {'image' if per_image else 'batch'} w={weight}"
        loss, coef = op_fwd(zd, td, per_image, weight)
        check(tag + " ABI", loss, op_bwd(coef), w * l1, w * g1)
        base = torch.full((1,), 0.625, device=DEV)
        lb, cb = op_fwd(zd, td, per_image, weight, base=base)
        assert torch.equal(cb, coef) and float(base) == 0.625
        check(tag + " ABI base", lb, cb, 0.625 + w * l1, w * g1)
        lm, gm = module(mnn.LovaszHingeLoss(weight, per_image), zd, td)
        assert torch.equal(lm.reshape(1), loss) and torch.equal(gm.reshape(-1), coef) and gm.shape == zd.shape
    z, t = _case(shape, "random")
    lu, gu = UL.lovasz_hinge(_dev(z), _dev(t), per_image)
    check(f"{ids(shape)} utils.lovasz_hinge", lu, gu, *_ref(shape, "random", per_image))


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("shape", [(3, 1, 17, 13), (2, 1, 64, 64)], ids=ids)
def test_saturated_logits_stay_finite_and_inactive_pixels_get_no_gradient(shape, per_image):
    rng = np.random.RandomState(7)
    t = (rng.rand(*shape) < 0.4).astype(np.float32)
    sign = 2 * t - 1
    z0 = (rng.randn(*shape) * 2).astype(np.float32)
    for mag in (30.0, 100.0):
        for name, z in (("agreeing", sign * mag), ("opposed", -sign * mag),
                        ("mixed", np.where(rng.rand(*shape) < 0.5, sign * mag, -sign * mag)),
                        ("among normal", np.where(rng.rand(*shape) < 0.5, np.where(rng.rand(*shape) < 0.5, mag, -mag), z0))):
            z = z.astype(np.float32)
            l64, g64 = R.lovasz_ref(z, t, 1.0, per_image)
            loss, coef = op_fwd(_dev(z), _dev(t), per_image, 1.0)
            check(f"{ids(shape)} +-{mag:g} {name}", loss, op_bwd(coef), l64, g64)
            margin = np.where(t > 0.5, z, -z)
            assert bool((coef.cpu().numpy().reshape(shape)[margin >= 1] == 0).all())
            if name == "agreeing":
                assert float(loss) == 0.0 and not bool(coef.any())


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_threshold_with_soft_targets(per_image):
    from mi355 import nn as mnn
    shape = (3, 1, 17, 13)
    rng = np.random.RandomState(11)
    z, t = rng.randn(*shape).astype(np.float32), rng.rand(*shape).astype(np.float32)
    for thr in (0.2, 0.75):
        l64, g64 = R.lovasz_ref(z, t, 1.0, per_image, f32(thr))
        loss, coef = op_fwd(_dev(z), _dev(t), per_image, 1.0, thr=thr)
        check(f"thr {thr}", loss, coef, l64, g64)
        lm, gm = module(mnn.LovaszHingeLoss(1.0, per_image, thr), _dev(z), _dev(t))
        assert torch.equal(lm.reshape(1), loss) and torch.equal(gm.reshape(-1), coef)
    assert not np.array_equal(R.lovasz_ref(z, t, 1.0, per_image, 0.2)[1], R.lovasz_ref(z, t, 1.0, per_image, 0.75)[1])


def test_a_nan_logit_gives_a_nan_loss():
    for shape in ((3, 1, 17, 13), (2, 1, 64, 64)):
        z, t = _case(shape, "random")
        z = z.copy()
        z[0, 0, 3, 5] = np.nan
        for per_image in (True, False):
            loss, coef = op_fwd(_dev(z), _dev(t), per_image, 1.0)
            assert bool(torch.isnan(loss).all()), (shape, per_image)


# ---- 2. the backward pass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (3, 1, 17, 13), (1, 1, 1, 1)], ids=ids)
def test_accumulate_adds_and_overwrite_overwrites(shape):
    z, t = _case(shape, "random")
    _, coef = op_fwd(_dev(z), _dev(t), True, 0.3)
    n = coef.numel()
    pre = torch.randn(n, device=DEV)
    for gs in (None, torch.full((1,), 3.0, device=DEV)):
        term = op_bwd(coef, gs, 0, pre.clone())
        assert torch.equal(term, coef if gs is None else coef * 3.0)
        acc = op_bwd(coef, gs, 1, pre.clone())
        assert torch.equal(acc, pre + term)                # the ROUNDED term is added
    # an unaligned view takes the element-wise kernel and gives the same bits; neighbours stay untouched
    if n > 8:
        big_c, big_d = torch.zeros(n + 8, device=DEV), torch.full((n + 8,), 5.0, device=DEV)
        big_c[1: n + 1] = coef
        out = op_bwd(big_c[1: n + 1], None, 1, big_d[3: n + 3])
        assert torch.equal(out, 5.0 + coef) and bool((big_d[:3] == 5).all()) and bool((big_d[n + 3:] == 5).all())


@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (3, 1, 17, 13)], ids=ids)
@pytest.mark.parametrize("factor", [3.0, 65536.0])
def test_upstream_gradient_and_loss_scale_enter_as_one_factor(shape, factor):
    from mi355 import amp as mamp, nn as mnn
    z, t = _case(shape, "random")
    zd, td = _dev(z), _dev(t)
    l1, g1 = _ref(shape, "random", True)
    _, coef = op_fwd(zd, td, True, 0.3)
    base = op_bwd(coef)
    assert torch.equal(base, op_bwd(coef, gscale=torch.ones(1, device=DEV)))
    scaled = op_bwd(coef, gscale=torch.full((1,), factor, device=DEV))
    check(f"gscale {factor:g} at the op {shape}", torch.zeros(()), scaled, 0.0, f32(0.3) * g1, factor)
    e = rel_err(scaled, base * factor)
    assert e < 1e-6
    for crit in (mnn.LovaszHingeLoss(0.3), mnn.RegionLovaszLoss(lovasz_weight=0.3)):
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


# ---- 3. the modules ----------------------------------------------------------------------------------------------------------
def test_layouts_dtypes_and_errors():
    from mi355 import nn as mnn
    z = torch.randn(2, 17, 13, device=DEV)
    t = (torch.rand(2, 17, 13, device=DEV) < 0.5).float()
    for crit in (mnn.LovaszHingeLoss(), mnn.LovaszHingeLoss(per_image=False), mnn.RegionLovaszLoss(lovasz_weight=0.3)):
        with pytest.raises(ValueError, match="must match input size"):
            crit(z, t[:1])
        with pytest.raises(ValueError, match="one-channel"):
            crit(torch.zeros(2, 2, 17, 13, device=DEV), torch.zeros(2, 2, 17, 13, device=DEV))
        l3, g3 = module(crit, z, t)
        l4, g4 = module(crit, z[:, None], t[:, None])
        assert torch.equal(l3, l4) and torch.equal(g3.reshape(-1), g4.reshape(-1)) and g3.shape == z.shape
        lu, gu = module(crit, z, t.to(torch.uint8))            # targets of another dtype are converted, as for BCE
        assert torch.equal(lu, l3) and torch.equal(gu, g3)


@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
@pytest.mark.parametrize("shape", [(2, 1, 64, 64), (3, 1, 17, 13)], ids=ids)
def test_region_lovasz_is_its_two_terms(shape, per_image):
    """A Lovasz weight of 0 is CombinedLoss, no regional weight is LovaszHingeLoss, bit for bit.  With both: the loss is within the
    loss bound of the two restatements' sum; the gradient is, bit for bit, the fp32 sum of what the two backward launches give alone
    (the second adds its rounded term to the first) — each of them is held to its own bound in its own test — and within the regional
    loss's bound (1e-5 of the largest element, tests/test_gpu_seg_loss.py) of the two restatements' sum."""
    from mi355 import nn as mnn
    z, t = _case(shape, "random")
    zd, td = _dev(z), _dev(t)
    for b, d in ((0.5, 0.5), (0.3, 0.0), (0.0, 1.0)):
        l0, g0 = module(mnn.RegionLovaszLoss(b, d, 0.0, per_image=per_image), zd, td)
        lc, gc = module(mnn.CombinedLoss(b, d), zd, td)
        assert torch.equal(l0, lc) and torch.equal(g0, gc)
    for w in (1.0, 0.3):
        lr, gr = module(mnn.RegionLovaszLoss(0.0, 0.0, w, per_image=per_image), zd, td)
        ll, gl = module(mnn.LovaszHingeLoss(w, per_image), zd, td)
        assert torch.equal(lr, ll) and torch.equal(gr, gl)
    for ps in (False, True):
        for b, d, w in ((0.5, 0.0, 0.5), (0.5, 0.5, 0.3), (0.0, 1.0, 1.0)):
            crit = mnn.RegionLovaszLoss(b, d, w, per_sample=ps, per_image=per_image)
            loss, dz = module(crit, zd, td)
            ls, gs = S.seg_loss(z.astype(np.float64), t.astype(np.float64), f32(b), f32(d), 1.0, ps)
            l1, g1 = _ref(shape, "random", per_image)
            l64, g64 = ls + f32(w) * l1, gs + f32(w) * g1
            _, seg_alone = op_seg(zd, td, b, d, 1.0, ps)
            _, coef = op_fwd(zd, td, per_image, w)
            assert torch.equal(dz.reshape(-1), seg_alone.reshape(-1) + coef)
            e = rel_err(dz.cpu().reshape(-1), torch.from_numpy(g64).reshape(-1))
            print(f"RegionLovaszLoss({b}, {d}, {w}, per_sample={ps}) {shape}: loss {float(loss):.8f} ref {l64:.8f}, dz rel_err {e:.2e}")
            assert abs(float(loss) - l64) < 1e-5 * max(1.0, abs(l64))
            assert e < 1e-5


def test_loss_and_gradient_are_bit_reproducible():
    from mi355 import nn as mnn
    shape = (32, 1, 256, 256)
    z, t = _case(shape, "quantised")
    zd, td = _dev(z), _dev(t)
    for per_image in (True, False):
        l0, c0 = op_fwd(zd, td, per_image, 0.3)
        for _ in range(2):
            l1, c1 = op_fwd(zd, td, per_image, 0.3)
            assert torch.equal(l0, l1) and torch.equal(c0, c1)
        for crit in (mnn.LovaszHingeLoss(0.3, per_image), mnn.RegionLovaszLoss(per_sample=True, per_image=per_image)):
            runs = [module(crit, zd, td) for _ in range(3)]
            assert all(torch.equal(runs[0][0], r[0]) and torch.equal(runs[0][1], r[1]) for r in runs[1:]), type(crit).__name__


# ---- 4. whole model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_image", [True, False], ids=["image", "batch"])
def test_whole_model_gradients_match_fp64_oracle_on_the_same_masks(per_image):
    """tests/test_gpu_seg_loss.py's statement and parameter-gradient bounds for AttentionUNet 64 x 64, with LovaszHingeLoss.  The loss
    is piecewise linear in the ORDER of the logits, so the yardstick's dloss/dlogits is taken at the GPU's own logits (copied to the
    host, tests/lovasz_ref.py in fp64): plan.dout is held to the per-element bound, and that gradient is pushed through the fp64
    oracle replayed on the GPU's ReLU / max-pool decisions."""
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
    loss = mnn.LovaszHingeLoss(per_image=per_image)(out, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    relu, pool = gpu_kinks(plan)
    assert len(pool) == 4
    logits = out.detach().cpu().numpy()
    l64, dz64 = R.lovasz_ref(logits, y.numpy().reshape(logits.shape), 1.0, per_image)
    n = out.numel()
    check(f"LovaszHingeLoss(per_image={per_image}) AttentionUNet 64, plan.dout", loss.detach(), plan.dout[:n], l64, dz64)

    s64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    pk = nets.param_keys(s64)
    for k in pk:
        s64[k].requires_grad_(True)
    nets.Kinks.start("replay", relu, pool)
    try:
        o64 = nets.NETS[name](s64, x.double(), True)
        if o64.dim() == 3:
            o64 = o64.unsqueeze(1)
        o64.backward(torch.from_numpy(dz64).reshape(o64.shape))
    finally:
        _, _, used = nets.Kinks.stop()
    assert used == (len(relu), len(pool)), (used, len(relu), len(pool))
    g64 = {k: s64[k].grad for k in pk if s64[k].grad is not None}
    e_out = float((out.detach().cpu().double().reshape(o64.shape) - o64.detach()).abs().max() / o64.detach().abs().max())
    print(f"  logits {e_out:.2e}")
    assert e_out < 1e-4
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


# ---- 5. through train() ----------------------------------------------------------------------------------------------------------
LOG = r"Ep(\d+): TrainLoss ([\d.]+) \| ValLoss ([\d.]+) \| IoU ([\d.]+)"
KW = dict(bce_weight=0.5, dice_weight=0.0, lovasz_weight=0.5, smooth=1.0, per_sample=False, per_image=True)      # RegionLovaszLoss()


def _traj_setup():
    from torch.utils.data import DataLoader, TensorDataset
    z = np.load(os.path.join(G, "train_traj_AttentionUNet.npz"))
    hw, epochs, lr = int(z["hw"]), int(z["epochs"]), float(z["lr"])
    b = [otrain.synthetic_batch(4, hw, seed=s) for s in (0, 1, 2)]
    tr = DataLoader(TensorDataset(torch.cat([b[0][0], b[1][0]]), torch.cat([b[0][1], b[1][1]])), batch_size=4, shuffle=False)
    va = DataLoader(TensorDataset(b[2][0], b[2][1]), batch_size=4, shuffle=False)
    return b, tr, va, epochs, lr


def _fresh_model():
    from models.segmentation_models.AttentionUNet import AttentionUNet
    m = AttentionUNet()
    m.load_state_dict(nets.closed_form_state("AttentionUNet"))
    m.compute_dtype = torch.float32
    return m.to(DEV)


def _region_lovasz_ref(z, t):
    """(loss, dloss/dz) of RegionLovaszLoss() in fp64 on logits of either precision: seg_loss_ref + lovasz_ref."""
    ls, gs = S.seg_loss(z.astype(np.float64), t.astype(np.float64), KW["bce_weight"], KW["dice_weight"], KW["smooth"], KW["per_sample"])
    ll, gl = R.lovasz_ref(z, t, KW["lovasz_weight"], KW["per_image"])
    return ls + ll, gs + gl.reshape(gs.shape)


def cpu_protocol(dtype=torch.float64):
    """The protocol of oracle.train.train_seg on the fixed synthetic loader with the loss swapped for _region_lovasz_ref (training and
    validation alike), the network in ``dtype`` -> [(train loss, val loss, IoU) per epoch], best val loss."""
    name = "AttentionUNet"
    b, _, _, epochs, lr = _traj_setup()
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in nets.closed_form_state(name).items()}
    fn = nets.NETS[name]
    pk = nets.param_keys(sd)
    opt = otrain.AdamW(pk, lr)
    b = [(x.to(dtype), y.to(dtype)) for x, y in b]
    train_b, val_b = b[:2], b[2:]
    n_train, n_val = sum(x.shape[0] for x, _ in train_b), sum(x.shape[0] for x, _ in val_b)
    hist, best = [], float("inf")
    for ep in range(1, epochs + 1):
        run = 0.0
        for x, y in train_b:
            for k in pk:
                sd[k].requires_grad_(True)
                sd[k].grad = None
            out = fn(sd, x, True)
            if out.dim() == 3:
                out = out.unsqueeze(1)
            l, dz = _region_lovasz_ref(out.detach().numpy(), y.numpy().reshape(out.shape))
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
                vl += _region_lovasz_ref(out.numpy().reshape(y.shape), y.numpy())[0] * x.shape[0]
                vm += otrain.iou_train(torch.sigmoid(out).reshape(y.shape), y)
        vl /= n_val
        hist.append((run / n_train, vl, float(vm) / len(val_b)))
        opt.lr = otrain.cosine_lr(lr, ep, epochs)
        best = min(best, vl)
    return hist, best


def test_train_with_region_lovasz_follows_the_cpu_protocol(tmp_path, capsys):
    """helpers.train(criterion=RegionLovaszLoss()) on the fixed synthetic loader against cpu_protocol() in fp64, the statement of
    tests/test_gpu_seg_loss.py::test_train_with_combined_loss_follows_the_cpu_protocol.  Bounds: what an fp32 and an fp64 evaluation
    of that CPU loop differ by for THIS loss, measured on the CPU (cpu_protocol(torch.float32) against cpu_protocol(torch.float64),
    16 threads), per epoch:
        training loss   1.495840 / 1.189162 / 1.020025  against  1.495813 / 1.188732 / 1.018694:  2.7e-5, 4.3e-4, 1.3e-3
        validation loss 0.981125 / 0.954512 / 0.963168  against  0.981150 / 0.954460 / 0.963149:  2.5e-5, 5.2e-5, 1.9e-5
        IoU             0.234043 / 0.277613 / 0.271964  against  0.234959 / 0.277340 / 0.272277:  9.2e-4, 2.7e-4, 3.1e-4
    That spread lies within the BCE test's bounds (2e-3 on the training loss, 2e-3 relative on the validation loss, 5e-3 on the
    IoU), so those are used.  Both sides of every comparison are three-decimal numbers, as the log prints them."""
    from mi355 import nn as mnn
    from utils import helpers
    name = "AttentionUNet"
    _, tr, va, epochs, lr = _traj_setup()
    m = _fresh_model()
    best = helpers.train(m, tr, va, torch.device(DEV), epochs, lr, name, str(tmp_path), seg=True, criterion=mnn.RegionLovaszLoss())
    text = capsys.readouterr().out
    rows = re.findall(LOG, text)
    assert len(rows) == epochs, text
    assert os.path.exists(os.path.join(str(tmp_path), f"{name}_best_loss.pt"))
    hist, ref_best = cpu_protocol(torch.float64)
    for row, ref in zip(rows, hist):
        got = [float(v) for v in row]
        ref = tuple(float(f"{v:.3f}") for v in ref)            # what the CPU loop's own log line would print
        print(f"Ep{int(got[0])}: GPU train {got[1]:.3f} val {got[2]:.3f} IoU {got[3]:.3f} | CPU train {ref[0]:.4f} val {ref[1]:.4f} IoU {ref[2]:.4f}")
        assert abs(got[1] - ref[0]) <= 2e-3 + 1e-9 and abs(got[2] - ref[1]) <= 2e-3 * max(1, ref[1]) + 1e-9 and \
            abs(got[3] - ref[2]) <= 5e-3 + 1e-9, (got, ref)
    assert abs(best - ref_best) < 2e-3 * ref_best


def test_train_default_criterion_is_unchanged(tmp_path, capsys):
    """The logic of tests/test_gpu_seg_loss.py::test_train_default_criterion_is_unchanged with this change in place: criterion=None
    twice and BCEWithLogitsLoss() once from the same initial state — the explicit run agrees with a default run as well as two
    default runs agree with each other, bit for bit where they do."""
    from mi355 import nn as mnn
    from utils import helpers
    _, tr, va, epochs, lr = _traj_setup()
    runs = []
    for i, crit in enumerate([None, None, mnn.BCEWithLogitsLoss()]):
        m = _fresh_model()
        kw = {} if crit is None else {"criterion": crit}
        best = helpers.train(m, tr, va, torch.device(DEV), epochs, lr, "AttentionUNet", str(tmp_path / f"run{i}"), seg=True, **kw)
        text = re.sub(r"finished in [\d.]+ minutes", "finished", capsys.readouterr().out)
        runs.append((best, text, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (b0, t0, s0), (b1, t1, s1), (b2, t2, s2) = runs
    defaults_equal = all(torch.equal(s0[k], s1[k]) for k in s0)
    print("two default runs bit-identical:", defaults_equal, "| log identical:", t0 == t1)
    assert len(re.findall(LOG, t2)) == epochs
    if defaults_equal:
        for k in s0:
            assert torch.equal(s0[k], s2[k]), k
    else:
        for k in s0:
            d01 = float((s0[k].double() - s1[k].double()).abs().max())
            d02 = float((s0[k].double() - s2[k].double()).abs().max())
            assert d02 <= d01, (k, d02, d01)
    if t0 == t1:
        assert t2 == t0
        assert b2 == b0
    else:
        assert abs(b2 - b0) <= abs(b1 - b0) + 1e-6
