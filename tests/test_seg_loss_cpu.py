"""CPU: the Dice / BCE + Dice segmentation loss below the GPU — the fp64 restatement (tests/seg_loss_ref.py) against what the
reference's own ``DiceLoss`` / ``CombinedLoss`` recorded (tests/golden/seg_losses.npz, scripts/make_seg_loss_golden.py), the C ABI
(declared, exported, known to the plan engine, arguments validated before the device is touched) and the Python surface
(``mi355.nn``, ``utils.helpers.train``, the trainer's command line)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import seg_loss_ref as R
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
EPS = 1e-12


def _cases():
    z = np.load(os.path.join(G, "seg_losses.npz"))
    for key in z["cases"]:
        name, bw, dw, sm = str(key).split("__")
        yield str(key), z["z__" + name], z["t__" + name], float(bw[2:]), float(dw[2:]), float(sm[1:]), float(z["loss__" + key]), z["grad__" + key]


def test_fixture_covers_what_it_should():
    cases = list(_cases())
    assert {(c[3], c[4]) for c in cases} == {(0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, 0.7)}
    assert {c[5] for c in cases} == {1.0, 1e-3}
    shapes = {c[1].shape for c in cases}
    assert (2, 17, 13) in shapes and (2, 1, 16, 16) in shapes and all(max(s[-2:]) <= 17 for s in shapes)
    assert any(not np.all((c[2] == 0) | (c[2] == 1)) for c in cases), "soft targets"
    assert any(np.all(c[2] == 0) for c in cases) and any(np.all(c[2] == 1) for c in cases)
    assert any(np.any(c[1] == 30.0) and np.any(c[1] == -30.0) for c in cases)
    assert os.path.getsize(os.path.join(G, "seg_losses.npz")) < 512 * 1024


def test_restatement_reproduces_the_reference_classes():
    """Both are fp64 evaluations of the same expression: 1e-12 of the loss, 1e-12 of the gradient tensor's maximum."""
    n = 0
    for key, z, t, bw, dw, sm, loss, grad in _cases():
        l, g = R.seg_loss(z, t, bw, dw, sm)
        assert abs(l - loss) <= EPS * abs(loss), (key, l, loss)
        assert g.shape == grad.shape and np.abs(g - grad).max() <= EPS * np.abs(grad).max(), (key, np.abs(g - grad).max())
        assert np.isfinite(l) and np.all(np.isfinite(g))
        n += 1
    assert n >= 80


@pytest.mark.parametrize("bw,dw,sm", [(0.5, 0.5, 1.0), (0.0, 1.0, 1e-3), (0.3, 0.7, 1.0)])
def test_per_sample_mode_is_the_mean_of_single_image_calls(bw, dw, sm):
    rng = np.random.RandomState(5)
    z, t = rng.randn(3, 1, 9, 11) * 2, (rng.rand(3, 1, 9, 11) < 0.4).astype(np.float64)
    l, g = R.seg_loss(z, t, bw, dw, sm, per_sample=True)
    singles = [R.seg_loss(z[b:b + 1], t[b:b + 1], bw, dw, sm) for b in range(3)]
    assert abs(l - np.mean([s[0] for s in singles])) <= EPS * max(1.0, abs(l))
    g1 = np.concatenate([s[1] for s in singles]) / 3
    assert np.abs(g - g1).max() <= EPS * np.abs(g1).max()
    # and a batch of one image is the same in both modes
    a, b = R.seg_loss(z[:1], t[:1], bw, dw, sm, per_sample=True), R.seg_loss(z[:1], t[:1], bw, dw, sm)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_restatement_gradient_is_the_derivative_of_its_loss():
    rng = np.random.RandomState(7)
    z, t = rng.randn(2, 1, 4, 5), rng.rand(2, 1, 4, 5)
    for ps in (False, True):
        _, g = R.seg_loss(z, t, 0.3, 0.7, 1.0, ps)
        for idx in [(0, 0, 0, 0), (1, 0, 3, 4), (0, 0, 2, 1)]:
            h = 1e-6
            zp, zm = z.copy(), z.copy()
            zp[idx] += h
            zm[idx] -= h
            fd = (R.seg_loss(zp, t, 0.3, 0.7, 1.0, ps)[0] - R.seg_loss(zm, t, 0.3, 0.7, 1.0, ps)[0]) / (2 * h)
            assert abs(fd - g[idx]) < 1e-8, (ps, idx, fd, g[idx])


NEW = ("mi355_seg_loss_rows", "mi355_seg_loss_fwd", "mi355_seg_loss_bwd")


def test_abi_declares_exports_and_replays_the_new_entry_points():
    protos = L.parse_header()
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name in NEW:
        assert name in protos and protos[name][0] is ctypes.c_int, name
        assert hasattr(dll, name), name
        assert arity(name.encode()) == len(protos[name][1]), name
    assert [n for _, n in protos["mi355_seg_loss_fwd"][1]][-1] == "s" and [n for _, n in protos["mi355_seg_loss_bwd"][1]][-1] == "s"
    rows = L.lib.raw("mi355_seg_loss_rows")
    assert rows(32, 256 * 256) >= 32 and rows(2, 17 * 13) >= 2 and rows(1, 1) == 1
    assert rows(32, 256 * 256) <= 4096


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    fwd, bwd, rows = lib.raw("mi355_seg_loss_fwd"), lib.raw("mi355_seg_loss_bwd"), lib.raw("mi355_seg_loss_rows")
    buf = (ctypes.c_float * 64)()                       # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(z=p, t=p, B=2, per=8, bw=0.5, dw=0.5, sm=1.0, ps=0, partial=p, state=p, loss=p)

    def call_fwd(**kw):
        a = dict(ok, **kw)
        return fwd(a["z"], a["t"], a["B"], a["per"], a["bw"], a["dw"], a["sm"], a["ps"], a["partial"], a["state"], a["loss"], None)

    for bad, word in (({"z": None}, b"null"), ({"t": None}, b"null"), ({"partial": None}, b"null"), ({"state": None}, b"null"),
                      ({"loss": None}, b"null"), ({"B": 0}, b"B"), ({"B": -3}, b"B"), ({"per": 0}, b"per"), ({"bw": -0.5}, b"negative"),
                      ({"dw": -1.0}, b"negative"), ({"sm": -1e-3}, b"negative"), ({"bw": float("nan")}, b"negative")):
        assert call_fwd(**bad) == -1, bad
        assert word in err(), (bad, err())
    assert bwd(None, p, 2, 8, 0.5, p, None, p, None) == -1 and b"null" in err()
    assert bwd(p, p, 2, 8, 0.5, None, None, p, None) == -1 and b"null" in err()
    assert bwd(p, p, 2, 8, 0.5, p, None, None, None) == -1 and b"null" in err()
    assert bwd(p, p, 0, 8, 0.5, p, None, p, None) == -1 and b"B" in err()
    assert bwd(p, p, 2, 0, 0.5, p, None, p, None) == -1 and b"per" in err()
    assert bwd(p, p, 2, 8, -0.5, p, None, p, None) == -1 and b"negative" in err()
    assert rows(0, 8) == -1 and rows(2, 0) == -1 and err()


def test_loss_modules_have_the_reference_constructors():
    from mi355 import nn as mnn
    sig = inspect.signature(mnn.DiceLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [("smooth", 1.0), ("per_sample", False)]
    sig = inspect.signature(mnn.CombinedLoss.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == \
        [("bce_weight", 0.5), ("dice_weight", 0.5), ("smooth", 1.0), ("per_sample", False)]
    c = mnn.CombinedLoss()
    assert (c.bce_weight, c.dice_weight, c.smooth, c.per_sample) == (0.5, 0.5, 1.0, False)
    c = mnn.CombinedLoss(0.3, 0.7)
    assert (c.bce_weight, c.dice_weight) == (0.3, 0.7)
    d = mnn.DiceLoss()
    assert isinstance(d, mnn.CombinedLoss) and (d.bce_weight, d.dice_weight, d.smooth, d.per_sample) == (0.0, 1.0, 1.0, False)
    assert mnn.DiceLoss(1e-3, True).smooth == 1e-3 and mnn.DiceLoss(1e-3, True).per_sample is True
    with pytest.raises(ValueError):
        mnn.CombinedLoss(-0.1, 0.5)
    with pytest.raises(ValueError):
        mnn.DiceLoss(smooth=-1.0)


def test_train_takes_a_criterion_behind_the_reference_signature():
    from utils.helpers import train
    params = list(inspect.signature(train).parameters.values())
    assert [p.name for p in params] == ["model", "train_dl", "val_dl", "device", "epochs", "lr", "name", "save_dir", "seg", "cls_head_name",
                                        "criterion"]
    assert params[-1].default is None and params[-2].default is None and params[-3].default is False


def test_trainer_command_line():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    a = ap.parse_args([])
    assert a.seg_loss == "bce" and a.bce_weight == 0.5 and a.dice_weight == 0.5 and a.dice_per_sample is False
    assert trainer.seg_criterion(a) is None                       # the default run takes train()'s own BCEWithLogits
    a = ap.parse_args(["--seg-loss", "bce_dice", "--bce-weight", "0.3", "--dice-weight", "0.7", "--dice-per-sample"])
    c = trainer.seg_criterion(a)
    assert type(c) is mnn.CombinedLoss and (c.bce_weight, c.dice_weight, c.smooth, c.per_sample) == (0.3, 0.7, 1.0, True)
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice"]))
    assert type(c) is mnn.DiceLoss and (c.bce_weight, c.dice_weight, c.per_sample) == (0.0, 1.0, False)
    with pytest.raises(SystemExit):
        ap.parse_args(["--seg-loss", "focal"])


def test_new_kernels_use_no_scratch_and_keep_their_loads_in_flight(tmp_path):
    """Read as tests/test_code_objects.py reads them: no private segment, no spilled register, and at most two loads followed within
    two instructions by a full wait (the remainder loop's single vector) in the two streaming kernels."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed here")
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built"
    so = shutil.copy(L.SO_PATH, tmp_path)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp_path)
    found, traps = {}, {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp_path, f)], check=True, capture_output=True,
                               text=True).stdout
        if "seg_loss" not in notes:
            continue
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "seg_loss" in name:
                found[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count")}
        dis = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", os.path.join(tmp_path, f)], check=True, capture_output=True,
                             text=True).stdout
        cur, last, idx = None, -10, 0
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur, last, idx = m.group(1), -10, 0
                if "seg_loss" in cur:
                    traps[cur] = [0, 0]
                continue
            t = line.strip().split()
            if cur is None or "seg_loss" not in cur or not line.startswith("\t") or not t:
                continue
            idx += 1
            if t[0].startswith(("global_load", "buffer_load")):
                traps[cur][1] += 1
                last = idx
            elif t[0] == "s_waitcnt" and "vmcnt(0)" in line and idx - last <= 2:
                traps[cur][0] += 1
    # forward and backward in their 16-byte and scalar forms, and the finalize
    assert len(found) == 5 and sum("fwd" in k for k in found) == 2 and sum("bwd" in k for k in found) == 2, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)                  # two 256-thread workgroups per SIMD-quad and more
    for name, (n_trap, n_load) in traps.items():
        assert n_trap <= 2, (name, n_trap, n_load)
        if "fwd" in name or "bwd" in name:
            assert n_load >= 10, (name, n_load)                   # eight in flight in the main loop, two in the remainder loop
