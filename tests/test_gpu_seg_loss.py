"""-m gpu: the Dice / BCE + Dice segmentation loss (csrc/seg_loss.hip, mi355.nn.DiceLoss / CombinedLoss) on the device.

Yardsticks: tests/golden/seg_losses.npz (what the reference's own classes give in fp64) and tests/seg_loss_ref.py (the fp64
restatement pinned to that fixture on the CPU, tests/test_seg_loss_cpu.py) for shapes too big to commit.  Op bounds are those
tests/test_gpu_ops.py applies to mi355_bce_logits: |loss - ref| < 1e-5, rel_err(dz, ref) < 1e-5 (torch's own fp32 evaluation of the
reference classes sits at <= 2e-7 / <= 4e-7 from fp64 on these inputs)."""
import os
import re

import numpy as np
import pytest
import torch

import seg_loss_ref as R
from gpu_util import gpu_kinks, rel_err
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
WEIGHTS = [(0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, 0.7)]
SMOOTH = [1.0, 1e-3]


def op(z, t, bw, dw, sm, ps, gscale=None, dz=None):
    """The C ABI as a caller sees it -> (loss tensor [1], dz tensor of z's shape)."""
    B, per = z.shape[0], z.numel() // z.shape[0]
    rows = lib.mi355_seg_loss_rows(B, per)
    assert rows >= B
    partial = torch.empty(rows * 4, dtype=torch.float32, device=DEV)
    state = torch.empty(2 * B, dtype=torch.float32, device=DEV)
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    lib.mi355_seg_loss_fwd(z, t, B, per, bw, dw, sm, 1 if ps else 0, partial, state, loss)
    dz = torch.empty_like(z) if dz is None else dz
    lib.mi355_seg_loss_bwd(z, t, B, per, bw, state, gscale, dz)
    torch.cuda.synchronize()
    return loss, dz


def module(z, t, bw, dw, sm, ps):
    from mi355 import nn as mnn
    crit = mnn.DiceLoss(sm, ps) if (bw, dw) == (0.0, 1.0) else mnn.CombinedLoss(bw, dw, sm, ps)
    zz = z.clone().requires_grad_(True)
    loss = crit(zz, t)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), zz.grad


def check(tag, loss, dz, l64, g64):
    l, e = float(loss), rel_err(dz.cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(g64)).reshape(-1))
    print(f"{tag}: loss {l:.8f} ref {l64:.8f} |d| {abs(l - l64):.2e}  dz rel_err {e:.2e}")
    assert np.isfinite(l) and bool(torch.isfinite(dz).all()), tag
    assert abs(l - l64) < 1e-5, (tag, l, l64)
    assert e < 1e-5, (tag, e)


def test_fixture_parity_through_the_abi_and_the_modules():
    z = np.load(os.path.join(G, "seg_losses.npz"))
    n = 0
    for key in z["cases"]:
        name, bw, dw, sm = str(key).split("__")
        bw, dw, sm = float(bw[2:]), float(dw[2:]), float(sm[1:])
        zz, tt = torch.from_numpy(z["z__" + name]).float().to(DEV), torch.from_numpy(z["t__" + name]).float().to(DEV)
        l64, g64 = float(z["loss__" + key]), z["grad__" + key]
        check(f"abi {key}", *op(zz, tt, bw, dw, sm, False), l64, g64)
        check(f"module {key}", *module(zz, tt, bw, dw, sm, False), l64, g64)
        # per-image mode against the restatement (pinned to this fixture on the CPU)
        lp, gp = R.seg_loss(z["z__" + name], z["t__" + name], bw, dw, sm, per_sample=True)
        check(f"abi per-sample {key}", *op(zz, tt, bw, dw, sm, True), lp, gp)
        n += 1
    assert n >= 80


def _big(shape, seed, soft=False):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(*shape, generator=g) * 2.0).float()
    r = torch.rand(*shape, generator=g)
    t = r if soft else (r < 0.35).float()
    return z, t


@pytest.mark.parametrize("shape", [(32, 1, 256, 256), (1, 1, 64, 64), (3, 1, 17, 13)])
@pytest.mark.parametrize("ps", [False, True])
def test_parity_with_the_fp64_restatement(shape, ps):
    z, t = _big(shape, 11)
    zs, ts = _big(shape, 12, soft=True)
    zd, td, zsd, tsd = z.to(DEV), t.to(DEV), zs.to(DEV), ts.to(DEV)
    for bw, dw in WEIGHTS:
        for sm in SMOOTH:
            ref = R.seg_loss(z.numpy(), t.numpy(), bw, dw, sm, ps)
            check(f"abi {shape} ps={ps} ({bw},{dw}) s={sm}", *op(zd, td, bw, dw, sm, ps), *ref)
            check(f"module {shape} ps={ps} ({bw},{dw}) s={sm}", *module(zd, td, bw, dw, sm, ps), *ref)
    check(f"abi soft {shape} ps={ps}", *op(zsd, tsd, 0.5, 0.5, 1.0, ps), *R.seg_loss(zs.numpy(), ts.numpy(), 0.5, 0.5, 1.0, ps))


@pytest.mark.parametrize("shape", [(4, 1, 32, 32), (3, 1, 17, 13)])
@pytest.mark.parametrize("ps", [False, True])
def test_saturated_logits_and_constant_targets_stay_finite_and_right(shape, ps):
    g = torch.Generator().manual_seed(3)
    t = (torch.rand(*shape, generator=g) < 0.5).float()
    flip = torch.rand(*shape, generator=g) < 0.5
    z0 = torch.randn(*shape, generator=g) * 2
    cases = {"all-zero target": (z0, torch.zeros(shape)), "all-one target": (z0, torch.ones(shape))}
    for mag in (30.0, 100.0):
        cases[f"+-{mag:g} agreeing"] = (torch.where(t > 0, mag, -mag), t)
        cases[f"+-{mag:g} mixed"] = (torch.where(flip, mag, -mag), t)
    for tag, (z, t_) in cases.items():
        for bw, dw in WEIGHTS:
            for sm in SMOOTH:
                ref = R.seg_loss(z.numpy(), t_.numpy(), bw, dw, sm, ps)
                loss, dz = op(z.to(DEV), t_.to(DEV), bw, dw, sm, ps)
                assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all()), (tag, bw, dw, sm)
                assert abs(float(loss) - ref[0]) < 1e-5 * max(1.0, abs(ref[0])), (tag, bw, dw, sm, float(loss), ref[0])
                if "100" not in tag:                  # (at |z| = 100 the fp64 gradient is 1e-44: below fp32, the kernel gives 0)
                    check(f"{tag} {shape} ps={ps} ({bw},{dw}) s={sm}", loss, dz, *ref)


@pytest.mark.parametrize("shape", [(32, 1, 256, 256), (3, 1, 17, 13)])
def test_bce_only_weights_agree_with_bce_with_logits(shape):
    from mi355 import nn as mnn
    z, t = _big(shape, 21)
    zd, td = z.to(DEV), t.to(DEV)
    a = zd.clone().requires_grad_(True)
    la = mnn.CombinedLoss(1, 0)(a, td)
    la.backward()
    b = zd.clone().requires_grad_(True)
    lb = mnn.BCEWithLogitsLoss()(b, td)
    lb.backward()
    torch.cuda.synchronize()
    print(f"CombinedLoss(1, 0) vs BCEWithLogitsLoss {shape}: |dloss| {abs(float(la) - float(lb)):.2e}, dz rel_err {rel_err(a.grad, b.grad):.2e}")
    assert abs(float(la) - float(lb)) < 1e-5 and rel_err(a.grad, b.grad) < 1e-5


@pytest.mark.parametrize("ps", [False, True])
def test_loss_and_gradient_are_bit_reproducible(ps):
    z, t = _big((32, 1, 256, 256), 31)
    zd, td = z.to(DEV), t.to(DEV)
    l0, d0 = op(zd, td, 0.5, 0.5, 1.0, ps)
    for _ in range(2):
        l1, d1 = op(zd, td, 0.5, 0.5, 1.0, ps)
        assert torch.equal(l0, l1) and torch.equal(d0, d1)
    lm0, dm0 = module(zd, td, 0.5, 0.5, 1.0, ps)
    lm1, dm1 = module(zd, td, 0.5, 0.5, 1.0, ps)
    assert torch.equal(lm0, lm1) and torch.equal(dm0, dm1) and torch.equal(lm0.reshape(1), l0) and torch.equal(dm0, d0)


@pytest.mark.parametrize("shape", [(32, 1, 256, 256), (3, 1, 17, 13)])
@pytest.mark.parametrize("factor", [3.0, 65536.0])
def test_upstream_gradient_and_loss_scale_enter_as_one_factor(shape, factor):
    from mi355 import amp as mamp, nn as mnn
    z, t = _big(shape, 41)
    zd, td = z.to(DEV), t.to(DEV)
    _, base = op(zd, td, 0.5, 0.5, 1.0, False)
    _, one = op(zd, td, 0.5, 0.5, 1.0, False, gscale=torch.ones(1, device=DEV))
    assert torch.equal(base, one)
    _, scaled = op(zd, td, 0.5, 0.5, 1.0, False, gscale=torch.full((1,), factor, device=DEV))
    e = rel_err(scaled, base * factor)
    print(f"gscale {factor:g} at the op {shape}: rel_err {e:.2e}")
    assert e < 1e-6
    a = zd.clone().requires_grad_(True)
    loss = mnn.CombinedLoss()(a, td)
    if factor == 3.0:
        (3 * loss).backward()
    else:
        sc = mamp.GradScaler()
        assert sc.get_scale() == 65536.0
        sc.scale(loss).backward()
    torch.cuda.synchronize()
    e = rel_err(a.grad, base * factor)
    print(f"factor {factor:g} through autograd {shape}: rel_err {e:.2e}")
    assert e < 1e-6


def test_target_size_must_match_and_3d_logits_are_accepted():
    from mi355 import nn as mnn
    z = torch.randn(2, 17, 13, device=DEV)
    t = (torch.rand(2, 17, 13, device=DEV) < 0.5).float()
    with pytest.raises(ValueError, match="must match input size"):
        mnn.CombinedLoss()(z, t[:1])
    l3, g3 = module(z, t, 0.5, 0.5, 1.0, True)
    l4, g4 = module(z[:, None], t[:, None], 0.5, 0.5, 1.0, True)
    assert torch.equal(l3, l4) and torch.equal(g3.reshape(-1), g4.reshape(-1)) and g3.shape == z.shape
    lu, gu = module(z, t.to(torch.uint8), 0.5, 0.5, 1.0, False)            # targets of another dtype are converted, as for BCE
    lf, gf = module(z, t, 0.5, 0.5, 1.0, False)
    assert torch.equal(lu, lf) and torch.equal(gu, gf)


# ---- whole model ------------------------------------------------------------------------------------------------------------
def _replayed_oracle_with_loss(name, sd, x, y, relu, pool, **kw):
    """fp64 oracle forward + backward on the GPU's own ReLU / max-pool decisions (tests/test_gpu_models.py:264-291), the loss and
    dloss/dlogits from tests/seg_loss_ref.py -> (loss, logits, grads)."""
    s64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    pk = nets.param_keys(s64)
    for k in pk:
        s64[k].requires_grad_(True)
    nets.Kinks.start("replay", relu, pool)
    try:
        o64 = nets.NETS[name](s64, x.double(), True)
        if o64.dim() == 3:
            o64 = o64.unsqueeze(1)
        l64, dz = R.seg_loss(o64.detach().numpy(), y.double().numpy(), **kw)
        o64.backward(torch.from_numpy(dz))
    finally:
        _, _, used = nets.Kinks.stop()
    assert used == (len(relu), len(pool)), (used, len(relu), len(pool))
    return l64, o64.detach(), {k: s64[k].grad for k in pk if s64[k].grad is not None}


@pytest.mark.parametrize("ps", [False, True])
def test_whole_model_gradients_match_fp64_oracle_on_the_same_masks(ps):
    """tests/test_gpu_kinks.py's statement and bounds for AttentionUNet 64 x 64 under BCE, with CombinedLoss(): logits 1e-4, loss 1e-5,
    parameter gradients median <= 5e-5, max <= 1e-3, >= 97 % of the tensors <= 3e-4 of their maximum.  The gradients are right only
    if dloss/dlogits really landed in the plan's dout buffer."""
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
    loss = mnn.CombinedLoss(per_sample=ps)(out, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    relu, pool = gpu_kinks(plan)
    l64, o64, g64 = _replayed_oracle_with_loss(name, sd, x, y, relu, pool, bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=ps)
    assert len(pool) == 4
    # the loss wrote into the plan's own buffer
    dz64 = R.seg_loss(o64.numpy(), y.double().numpy(), 0.5, 0.5, 1.0, ps)[1]
    n = out.numel()
    e_dout = rel_err(plan.dout[:n].cpu(), torch.from_numpy(dz64).reshape(-1))
    e_out = float((out.detach().cpu().double().reshape(o64.shape) - o64).abs().max() / o64.abs().max())
    print(f"CombinedLoss(per_sample={ps}) AttentionUNet 64: logits {e_out:.2e}, loss |d| {abs(float(loss.detach()) - l64):.2e}, plan.dout {e_dout:.2e}")
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


# ---- train() ------------------------------------------------------------------------------------------------------------------
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


LOG = r"Ep(\d+): TrainLoss ([\d.]+) \| ValLoss ([\d.]+) \| IoU ([\d.]+)"


def _strip_time(text):
    return re.sub(r"finished in [\d.]+ minutes", "finished", text)


def test_train_default_criterion_is_unchanged(tmp_path, capsys):
    """criterion=None twice and criterion=BCEWithLogitsLoss() once, from the same initial state, on the fixed synthetic loader of
    test_fp32_train_loop_matches_reference_trajectory: the explicit run agrees with a default run as well as two default runs agree
    with each other — bit for bit in every state_dict entry (the step is bit-reproducible); the log text likewise, if the two
    default runs print the same (only the BCE loss VALUE is summed with atomics and may differ in its last bit)."""
    from mi355 import nn as mnn
    from utils import helpers
    _, tr, va, epochs, lr = _traj_setup()
    runs = []
    for i, crit in enumerate([None, None, mnn.BCEWithLogitsLoss()]):
        m = _fresh_model()
        kw = {} if crit is None else {"criterion": crit}
        best = helpers.train(m, tr, va, torch.device(DEV), epochs, lr, "AttentionUNet", str(tmp_path / f"run{i}"), seg=True, **kw)
        text = _strip_time(capsys.readouterr().out)
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


def test_train_with_combined_loss_follows_the_cpu_protocol(tmp_path, capsys):
    """helpers.train(criterion=CombinedLoss()) on the fixed synthetic loader against a CPU loop built here from oracle.nets,
    oracle.train.AdamW / clip_grad_norm / cosine_lr and tests/seg_loss_ref.py (the protocol of oracle.train.train_seg with the loss
    swapped, for the training and the validation loss alike).  Bounds: those test_fp32_train_loop_matches_reference_trajectory uses
    for BCE — what two CPU evaluations of the protocol differ by (tests/test_oracle_pins.py::test_train_trajectory_seg).  The CPU
    loop runs in fp64, so that none of that budget goes to the yardstick's own rounding: its fp32 evaluations on 16 threads / one
    thread / fp64 give an epoch-3 training loss of 0.54463 / 0.54454 / 0.54407 (the GPU prints 0.543).  Both sides of every
    comparison are three-decimal numbers, as the log prints them; the 1e-9 lets a difference of exactly 0.002 through, which
    binary floating point represents as 0.0020000000000000018."""
    from mi355 import nn as mnn
    from utils import helpers
    name = "AttentionUNet"
    b, tr, va, epochs, lr = _traj_setup()
    m = _fresh_model()
    best = helpers.train(m, tr, va, torch.device(DEV), epochs, lr, name, str(tmp_path), seg=True, criterion=mnn.CombinedLoss())
    text = capsys.readouterr().out
    rows = re.findall(LOG, text)
    assert len(rows) == epochs
    assert os.path.exists(os.path.join(str(tmp_path), f"{name}_best_loss.pt"))

    kw = dict(bce_weight=0.5, dice_weight=0.5, smooth=1.0, per_sample=False)
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
            l, dz = R.seg_loss(out.detach().numpy(), y.numpy(), **kw)
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
                vl += R.seg_loss(out.numpy().reshape(y.shape), y.numpy(), **kw)[0] * x.shape[0]
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
