"""-m gpu: the claims of tests/plan_verify.py on the device, with exact comparisons.

1. Poison invariance: a training step gives the same bits — output, every element of flat_g, the running statistics — whether
   the bytes the access table says the step writes (in plan.keep, plan.ws, flat_g) were zero, 0xFF (NaN in fp32 / bf16 / fp16;
   integer buffers get 0 so that a stale index stays in range) or whatever a step on another input left there.  A read of a byte
   that no launch of the step wrote cannot pass all three.
2. Declared writes are the real writes: the bound launches replayed one at a time, every byte that changes lies in a write
   region the table declares for that launch.  (This checks the WRITE half of the table against the kernels; the read half is
   covered by the poison runs only.)
3. Replay paths: gradients are bit-identical with MI355_PLAN_C=0 and with MI355_SIDE_STREAM=0 (child processes: both are read
   when a plan is made, the parent holds the defaults).

Every case first runs the static verifier on its plan and launches nothing if the plan is not clean."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
THREE = ("AttentionUNet", "R2AttU_Net", "ResNet18")


def _case(name):
    from test_plan_dataflow_cpu import _ctor
    return _ctor(name)


def _make(name, dtype, seed=0):
    ctor, shape = _case(name)
    torch.manual_seed(seed)
    net = ctor()
    net.compute_dtype = DT[dtype]
    return net.to(DEV).train(), shape


def _batch(name, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if _is_seg(name):                                           # segmenters: a binary mask
        y = (torch.randn((shape[0], 1) + tuple(shape[2:]), generator=g) > 0).float()
    else:
        y = torch.randint(0, 3, (shape[0],), generator=g)
    return x.to(DEV), y.to(DEV)


def _is_seg(name):
    return name in ("AttentionUNet", "R2AttU_Net", "R2U_Net") or name.startswith("ResNetUnet")


def _criterion(name):
    from mi355 import nn as mnn
    return mnn.BCEWithLogitsLoss() if _is_seg(name) else mnn.CrossEntropyLoss(label_smoothing=0.1)


def _static_check(net, shape, dtype):
    import plan_verify as pv
    net.engine._check_storage()
    plan = net.engine.plan_for(tuple(shape), True, True, DT[dtype])
    view = pv.PlanView(plan)
    bad = pv.verify(view)
    assert not bad, "the plan is not clean, nothing was launched:\n" + "\n".join(map(repr, bad[:20]))
    return plan, view


def _bits(t):
    t = t.contiguous().view(-1)
    return t.view(torch.uint8)


# ---- 1. poison invariance --------------------------------------------------------------------------------------------------------
POISON_CASES = [("AttentionUNet", "fp16"), ("R2AttU_Net", "bf16"), ("R2U_Net", "fp32"), ("ResNet18", "bf16"), ("resnet18_tv", "fp32"),
                ("ResNet50", "fp16"), ("VGG16", "fp16"), ("ResNetUnet_frozen", "bf16"), ("ResNetUnet_unfrozen", "fp32")]


@pytest.mark.parametrize("name,dtype", POISON_CASES, ids=lambda v: str(v))
def test_step_does_not_depend_on_what_its_buffers_held(name, dtype):
    import plan_verify as pv
    from mi355 import amp as mamp
    net, shape = _make(name, dtype)
    x, y = _batch(name, shape, 1)
    x2, y2 = _batch(name, shape, 2)
    plan, view = _static_check(net, shape, dtype)
    crit = _criterion(name)
    # fp16 runs through the loss scaler.  Randomly initialised weights, no step taken: the default scale of 65536 overflows fp16
    # gradients here (which training answers by skipping the step and backing off); 256 keeps mean-reduced losses' gradients
    # well inside fp16's range, and the test is about finite values being the same bits
    scaler = mamp.GradScaler(init_scale=256.0) if dtype == "fp16" else None
    eng = net.engine

    def step(x, y):
        net.zero_grad(set_to_none=True)
        out = net(x)
        assert out._mi355_plan is plan
        loss = crit(out, y)
        (scaler.scale(loss) if scaler is not None else loss).backward()
        torch.cuda.synchronize()
        return [out.detach().clone(), eng.flat_g.clone()] + [b.detach().clone() for b in net.buffers()]

    step(x2, y2)                                                   # warm-up: the plan is bound, every buffer has been used once
    state = [b.detach().clone() for b in net.buffers()]
    counter = None if eng._drop_counter is None else eng._drop_counter.clone()

    def restore():
        with torch.no_grad():
            for b, s in zip(net.buffers(), state):
                b.copy_(s)
            if counter is not None:
                eng._drop_counter.copy_(counter)

    # the step-written bytes of keep, ws and flat_g, by the access table (the frozen-weight packs are written on refresh only)
    regions = pv.write_regions(view, plan.pre + plan.fwd + plan.bwd)
    masks = []
    for key, t in pv.plan_buffers(view):
        if key in regions:
            nbytes = t.numel() * t.element_size()
            m = torch.from_numpy(pv.byte_mask(regions[key], nbytes)).to(DEV)
            integer = t.dtype in (torch.int32, torch.int64)
            masks.append((_bits(t), m, integer))
    assert len(masks) > 10 and any(bool(m.all()) for _, m, _ in masks)

    def fill(poison):
        for b, m, integer in masks:
            b.masked_fill_(m, 0xFF if (poison and not integer) else 0)

    runs = {}
    for tag in ("zero", "zero2", "poison"):
        restore()
        fill(tag == "poison")
        if tag == "poison":                        # (the poison is there: a fully step-written floating-point buffer is all NaN bytes)
            assert any(not integer and bool(m.all()) and bool((b == 0xFF).all()) for b, m, integer in masks)
        runs[tag] = step(x, y)
    restore()
    step(x2, y2)
    restore()
    runs["untouched"] = step(x, y)
    for tag, r in runs.items():
        for i, t in enumerate(r):
            assert bool(torch.isfinite(t.float()).all()), (tag, ("output", "flat_g")[i] if i < 2 else f"buffer {i - 2}")
    what = lambda i: ("output", "flat_g")[i] if i < 2 else f"buffer {i - 2}"
    for i, (a, b) in enumerate(zip(runs["zero"], runs["zero2"])):
        assert torch.equal(_bits(a), _bits(b)), f"two zero-filled runs differ in {what(i)}: the plan is not reproducible"
    for tag in ("poison", "untouched"):
        for i, (a, b) in enumerate(zip(runs["zero"], runs[tag])):
            if not torch.equal(_bits(a), _bits(b)):
                d = (a.reshape(-1) != b.reshape(-1)).nonzero()
                raise AssertionError(f"{tag} run differs from the zero-filled one in {what(i)}: {d.numel()} elements, first at {int(d[0])}")
    assert float(runs["zero"][1].abs().max()) > 0


# ---- 2. declared writes are the real writes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE)
def test_every_changed_byte_lies_in_a_declared_write_region(name):
    import plan_verify as pv
    net, shape = _make(name, "bf16")
    plan, view = _static_check(net, shape, "bf16")
    plan.side_stream_enabled = False                                 # one stream: every launch is bound to the current one
    x, _ = _batch(name, shape, 1)
    plan.input[0][: x.numel()].copy_(x.reshape(-1))
    plan.dout.copy_(torch.randn(plan.dout.numel(), generator=torch.Generator().manual_seed(3)).to(DEV) * 1e-3)
    stream = torch.cuda.current_stream().cuda_stream
    plan.refresh_static_packs(stream)
    fwd, bwd = plan.bind(stream)
    bufs = pv.plan_buffers(view)
    base, total = {}, 0
    for key, t in bufs:
        base[key] = total
        total += t.numel() * t.element_size()
    views = [_bits(t) for _, t in bufs]
    snap = torch.cat(views)
    decl = torch.zeros(total, dtype=torch.bool, device=DEV)
    n_changed = 0
    for k, (fn, args, lname, l) in enumerate(fwd + bwd):
        rc = fn(*args)
        assert rc == 0, (k, lname, rc)
        torch.cuda.synchronize()
        spans = []
        for ac in view.res.accesses(l):
            r = ac.region
            if ac.writes and r.key in base:
                v = decl[base[r.key] + r.start:].as_strided((r.rows, r.width), (r.pitch, 1))
                v.fill_(True)
                spans.append(v)
        cur = torch.cat(views)
        diff = cur != snap
        n_changed += int(diff.any())
        stray = diff & ~decl
        if bool(stray.any()):
            at = int(stray.nonzero()[0])
            key = max((b, kk) for kk, b in base.items() if b <= at)
            raise AssertionError(f"launch {k} {lname} changed {int(stray.sum())} bytes outside its declared write regions, first at byte "
                                 f"{at - key[0]} of {key[1]}")
        for v in spans:
            v.fill_(False)
        snap = cur
    assert n_changed > 0.9 * len(fwd + bwd)                          # (the snapshots do see the launches)


# ---- 3. replay paths -----------------------------------------------------------------------------------------------------------------
def _gradients(names):
    """{model: flat_g after the second of two training steps (bf16)} under this process's MI355_PLAN_C / MI355_SIDE_STREAM"""
    out = {}
    for name in names:
        net, shape = _make(name, "bf16")
        plan, _ = _static_check(net, shape, "bf16")
        x, y = _batch(name, shape, 1)
        crit = _criterion(name)
        for _ in range(2):
            net.zero_grad(set_to_none=True)
            o = net(x)
            assert o._mi355_plan is plan
            crit(o, y).backward()
        torch.cuda.synchronize()
        assert plan.replay_in_c == (os.environ.get("MI355_PLAN_C", "1") != "0")
        assert (plan._side is not None) == (os.environ.get("MI355_SIDE_STREAM", "1") != "0")
        out[name] = net.engine.flat_g.cpu()
    return out


_BASE = {}


@pytest.mark.parametrize("switch", ["MI355_PLAN_C", "MI355_SIDE_STREAM"])
def test_replay_paths_give_the_same_gradient_bits(switch):
    assert os.environ.get("MI355_PLAN_C", "1") != "0" and os.environ.get("MI355_SIDE_STREAM", "1") != "0"
    if not _BASE:
        _BASE.update(_gradients(THREE))
    fd, path = tempfile.mkstemp(suffix=".pt")
    os.close(fd)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **{switch: "0"}),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        other = torch.load(path)
    finally:
        os.unlink(path)
    for name in THREE:
        a, b = _BASE[name], other[name]
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: {int((a != b).sum())} gradient elements differ with {switch}=0"


if __name__ == "__main__":          # the child: the same three models under the environment it was started with
    import conftest  # noqa: F401  (the paths)
    torch.save(_gradients(THREE), sys.argv[1])
