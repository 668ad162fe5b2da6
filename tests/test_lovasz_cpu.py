"""CPU: the Lovasz hinge and the segmented sort below the GPU — the fp64 restatement (tests/lovasz_ref.py) against its committed
fixture (tests/golden/lovasz.npz: a torch-fp64 autograd transcription of the paper's Algorithm 1), the closed-form Jaccard increment
against the differenced one, the constructors and their errors, the trainer's flags, the C ABI's argument checks (which run before
anything touches the device) and the new kernels' code-object notes."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import lovasz_ref as R
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "lovasz.npz")


def test_restatement_reproduces_the_papers_algorithm():
    z = np.load(FIXTURE)
    cases = [str(k) for k in z["cases"]]
    assert os.path.getsize(FIXTURE) <= 100 * 1024 and len(cases) >= 16
    shapes, kinds, modes = set(), set(), set()
    for key in cases:
        name, mode = key.rsplit("__", 1)
        logits, target = z["z__" + name], z["t__" + name].astype(np.float32)
        assert logits.dtype == np.float32
        shapes.add(logits.shape)
        kinds.add(name.split("_", 1)[1])
        modes.add(mode)
        loss, grad = R.lovasz_ref(logits, target, 1.0, mode == "image")
        assert abs(loss - float(z["loss__" + key])) <= 1e-12, key
        assert np.abs(grad - z["grad__" + key]).max() <= 1e-12, key
    assert shapes == {(3, 1, 17, 13), (1, 1, 1, 1), (2, 1, 32, 32)} and modes == {"image", "batch"}
    assert kinds == {"random", "quantised", "all_zero_target", "all_one_target"}
    q = z["z__3x1x17x13_quantised"]
    assert np.array_equal(q * 4, np.round(q * 4)) and np.unique(q).size < q.size // 4      # multiples of 0.25: ties
    assert not z["t__3x1x17x13_all_zero_target"].any() and z["t__3x1x17x13_all_one_target"].all()


def test_weight_and_threshold_enter_the_restatement_as_stated():
    rng = np.random.RandomState(2)
    z = rng.randn(3, 1, 5, 7).astype(np.float32)
    t = rng.rand(3, 1, 5, 7).astype(np.float32)
    for per_image in (True, False):
        l1, g1 = R.lovasz_ref(z, t, 1.0, per_image, 0.7)
        l2, g2 = R.lovasz_ref(z, (t > 0.7).astype(np.float32), 0.3, per_image)
        assert abs(l2 - 0.3 * l1) < 1e-15 and np.abs(g2 - 0.3 * g1).max() < 1e-16
    # a margin >= 1 contributes nothing; a NaN logit makes the loss NaN
    l, g = R.lovasz_ref(np.array([[30.0, -30.0, 1.0, 0.5]], dtype=np.float32), np.array([[1, 0, 1, 1]], dtype=np.float32))
    assert g[0, :3].tolist() == [0.0, 0.0, 0.0] and g[0, 3] == -1.0 / 3 and abs(l - 0.5 / 3) < 1e-16
    assert np.isnan(R.lovasz_ref(np.array([[np.nan, 1.0]], dtype=np.float32), np.array([[1, 0]], dtype=np.float32))[0])


@pytest.mark.parametrize("n", [1, 7, 221, 4096, 65536])
def test_closed_form_increment_equals_the_differenced_jaccard(n):
    rng = np.random.RandomState(n)
    for y in (rng.rand(n) < 0.3, rng.rand(n) < 0.01, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)):
        w, d = R.jaccard_weights(y), R.jaccard_weights_differenced(y)
        # the difference of two numbers near 1 carries their rounding: a few ulps of 1, not of w
        assert np.abs(w - d).max() <= 8 * np.finfo(np.float64).eps, (n, y.sum())
        assert abs(w.sum() - 1.0) < 1e-12                  # the increments add up to the Jaccard loss of the full set
        assert (w >= 0).all()


def test_argsort_ref_is_stable_and_merges_the_zeros():
    k = np.array([[0.0, -0.0, 1.0, -1.0, 0.0, np.inf, -np.inf, 1.0]], dtype=np.float32)
    assert R.argsort_ref(k).tolist() == [[6, 3, 0, 1, 4, 2, 7, 5]] and R.argsort_ref(k).dtype == np.int32


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_constructors_defaults_and_errors():
    import torch
    from mi355 import nn as mnn
    sig = inspect.signature(mnn.LovaszHingeLoss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("weight", 1.0), ("per_image", True), ("threshold", 0.5)]
    sig = inspect.signature(mnn.RegionLovaszLoss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("bce_weight", 0.5), ("dice_weight", 0.0), ("lovasz_weight", 0.5), ("smooth", 1.0), ("per_sample", False), ("per_image", True),
        ("threshold", 0.5)]
    c = mnn.LovaszHingeLoss()
    assert (c.weight, c.per_image, c.threshold) == (1.0, True, 0.5)
    r = mnn.RegionLovaszLoss()
    assert (r.bce_weight, r.dice_weight, r.lovasz_weight, r.smooth, r.per_sample, r.per_image, r.threshold) == \
        (0.5, 0.0, 0.5, 1.0, False, True, 0.5)
    with pytest.raises(ValueError):
        mnn.LovaszHingeLoss(weight=-1.0)
    for kw in ({"bce_weight": -1}, {"dice_weight": -0.1}, {"lovasz_weight": -0.01}, {"smooth": -1}):
        with pytest.raises(ValueError):
            mnn.RegionLovaszLoss(**kw)
    for crit in (c, r):
        for shape in ((2, 2, 4, 4), (2, 16), (2, 1, 1, 4, 4)):          # raised before anything touches a device
            with pytest.raises(ValueError, match="one-channel"):
                crit(torch.zeros(shape), torch.zeros(shape))
        with pytest.raises(ValueError, match="must match input size"):
            crit(torch.zeros(2, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    from utils import lovasz as UL
    with pytest.raises(ValueError, match="device tensor"):
        UL.segmented_argsort(torch.zeros(2, 8))
    with pytest.raises(ValueError, match="device tensor"):
        UL.lovasz_hinge(torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError, match="one-channel"):
        UL.lovasz_hinge(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))


def test_trainer_flags():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.lovasz_weight, d.lovasz_batch, d.seg_loss) == (0.0, False, "bce")
    assert trainer.seg_criterion(d) is None
    assert trainer.seg_criterion(ap.parse_args(["--lovasz-weight", "0"])) is None
    assert trainer.seg_criterion(ap.parse_args(["--lovasz-batch"])) is None
    assert type(trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice", "--lovasz-weight", "0"]))) is mnn.DiceLoss
    assert type(trainer.seg_criterion(ap.parse_args(["--seg-loss", "bce_dice"]))) is mnn.CombinedLoss
    assert type(trainer.seg_criterion(ap.parse_args(["--seg-loss", "bce", "--boundary-weight", "0.1"]))) is mnn.RegionBoundaryLoss
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "lovasz"]))
    assert type(c) is mnn.LovaszHingeLoss and (c.weight, c.per_image, c.threshold) == (1.0, True, 0.5)
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "lovasz", "--lovasz-batch"]))
    assert type(c) is mnn.LovaszHingeLoss and not c.per_image
    for loss, extra, want in (("bce", [], (1.0, 0.0)), ("dice", [], (0.0, 1.0)), ("bce_dice", [], (0.5, 0.5)),
                              ("bce_dice", ["--bce-weight", "0.3", "--dice-weight", "0.7"], (0.3, 0.7))):
        c = trainer.seg_criterion(ap.parse_args(["--seg-loss", loss, "--lovasz-weight", "0.25"] + extra))
        assert type(c) is mnn.RegionLovaszLoss and (c.bce_weight, c.dice_weight) == want and c.lovasz_weight == 0.25
        assert c.per_image and not c.per_sample
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice", "--lovasz-weight", "0.5", "--lovasz-batch", "--dice-per-sample"]))
    assert (c.per_image, c.per_sample, c.lovasz_weight) == (False, True, 0.5)
    for bad in (["--lovasz-weight", "-1"], ["--lovasz-weight", "0.5", "--boundary-weight", "0.1"],
                ["--seg-loss", "lovasz", "--lovasz-weight", "0.5"]):
        with pytest.raises(ValueError):
            trainer.seg_criterion(ap.parse_args(bad))
    with pytest.raises(SystemExit):
        ap.parse_args(["--seg-loss", "focal"])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = {"mi355_segsort_tile": [],
         "mi355_segsort_ws_ints": ["S", "len"],
         "mi355_segsort_f32": ["keys", "S", "len", "ws", "ws_ints", "perm", "s"],
         "mi355_lovasz_ws_ints": ["S", "len"],
         "mi355_lovasz_fwd": ["z", "t", "S", "len", "thr", "weight", "base", "ws", "ws_ints", "coef", "loss", "s"],
         "mi355_lovasz_bwd": ["coef", "n", "gscale", "accumulate", "dz", "s"]}


def test_abi_declares_exports_and_replays_the_new_entry_points():
    protos = L.parse_header()
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, args in NAMES.items():
        assert name in protos and protos[name][0] is ctypes.c_int, name
        assert [n for _, n in protos[name][1]] == args, name
        assert hasattr(dll, name), name
        assert arity(name.encode()) == len(args), name
    T = L.lib.raw("mi355_segsort_tile")()
    assert T > 0 and T % 64 == 0
    sort_ws, lov_ws = L.lib.raw("mi355_segsort_ws_ints"), L.lib.raw("mi355_lovasz_ws_ints")
    for S, n in ((1, 1), (3, 221), (32, 65536), (1, 1 << 21), (65535, 4), (1, 1 << 26), (65535, 1024)):
        assert 2 * S * n <= sort_ws(S, n) <= 4 * S * n + 512 * S, (S, n)
        assert sort_ws(S, n) + 2 * S * n <= lov_ws(S, n) <= sort_ws(S, n) + 3 * S * n + 8 * S, (S, n)


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    sort_ws, lov_ws = lib.raw("mi355_segsort_ws_ints"), lib.raw("mi355_lovasz_ws_ints")
    for bad in ((0, 16), (-1, 16), (65536, 16), (2, 0), (2, -4), (2, (1 << 25) + 1), (1, (1 << 26) + 1), (65535, 1025)):
        assert sort_ws(*bad) == -1 and b"segsort_ws_ints" in err() and b"2^26" in err(), (bad, err())
        assert lov_ws(*bad) == -1 and b"lovasz_ws_ints" in err() and b"2^26" in err(), (bad, err())
    buf = (ctypes.c_double * 4096)()                    # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)

    need = sort_ws(2, 64)
    assert need > 0
    run = lib.raw("mi355_segsort_f32")
    ok = dict(keys=p, S=2, len=64, ws=p, ws_ints=need, perm=p)

    def call(**kw):
        a = dict(ok, **kw)
        return run(a["keys"], a["S"], a["len"], a["ws"], a["ws_ints"], a["perm"], None)

    for bad, word in (({"keys": None}, b"null pointer (keys)"), ({"ws": None}, b"null pointer (ws)"), ({"perm": None}, b"null pointer (perm)"),
                      ({"S": 0}, b"S"), ({"S": 65536}, b"65535"), ({"len": 0}, b"len"), ({"len": -3}, b"len"),
                      ({"len": (1 << 25) + 1}, b"2^26"), ({"ws_ints": need - 1}, b"too short"), ({"ws_ints": 0}, b"too short")):
        assert call(**bad) == -1, bad
        assert word in err() and b"segsort_f32" in err(), (bad, err())

    need = lov_ws(2, 64)
    assert need > 0
    fwd, bwd = lib.raw("mi355_lovasz_fwd"), lib.raw("mi355_lovasz_bwd")
    okf = dict(z=p, t=p, S=2, len=64, thr=0.5, weight=1.0, base=None, ws=p, ws_ints=need, coef=p, loss=p)
    okb = dict(coef=p, n=128, gscale=None, accumulate=0, dz=p)

    def call_f(**kw):
        a = dict(okf, **kw)
        return fwd(a["z"], a["t"], a["S"], a["len"], a["thr"], a["weight"], a["base"], a["ws"], a["ws_ints"], a["coef"], a["loss"], None)

    def call_b(**kw):
        a = dict(okb, **kw)
        return bwd(a["coef"], a["n"], a["gscale"], a["accumulate"], a["dz"], None)

    for bad, word in (({"z": None}, b"null pointer (z)"), ({"t": None}, b"null pointer (t)"), ({"ws": None}, b"null pointer (ws)"),
                      ({"coef": None}, b"null pointer (coef)"), ({"loss": None}, b"null pointer (loss)"), ({"S": 0}, b"S"),
                      ({"S": 65536}, b"65535"), ({"len": 0}, b"len"), ({"len": (1 << 25) + 1}, b"2^26"), ({"weight": -0.5}, b"weight"),
                      ({"weight": float("nan")}, b"weight"), ({"ws_ints": need - 1}, b"too short"), ({"ws_ints": 0}, b"too short")):
        assert call_f(**bad) == -1, bad
        assert word in err() and b"lovasz_fwd" in err(), (bad, err())
    for bad, word in (({"coef": None}, b"null pointer (coef)"), ({"dz": None}, b"null pointer (dz)"), ({"n": 0}, b"n"), ({"n": -1}, b"n"),
                      ({"n": (1 << 26) + 1}, b"2^26")):
        assert call_b(**bad) == -1, bad
        assert word in err() and b"lovasz_bwd" in err(), (bad, err())


def test_new_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    """Read as tests/test_seg_loss_cpu.py reads its own: no private segment, no spilled register."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(os.path.join(llvm, "llvm-objdump")) and os.path.exists(os.path.join(llvm, "llvm-readelf"))):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed here")
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built"
    so = shutil.copy(L.SO_PATH, tmp_path)
    subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(tmp_path, f)], check=True, capture_output=True,
                               text=True).stdout
        if "segsort" not in notes and "lovasz" not in notes:
            continue
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "segsort" in name or "lovasz" in name:
                assert "seg_loss" not in name, name
                found[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                               for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count",
                                         "group_segment_fixed_size")}
    # the sort: histogram (fp32 / integer keys), row scan, scatter (first / middle / last pass); the loss: margin, count, weight,
    # finalize, backward (16-byte / scalar x overwrite / accumulate)
    assert sum("segsort_hist" in k for k in found) == 2 and sum("segsort_rowscan" in k for k in found) == 1, sorted(found)
    assert sum("segsort_scatter" in k for k in found) == 3, sorted(found)
    assert sum("lovasz_bwd" in k for k in found) == 4 and sum("lovasz" in k for k in found) == 8, sorted(found)
    for name, k in found.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)                  # two 256-thread workgroups per SIMD-quad and more
        assert k["group_segment_fixed_size"] <= 40 * 1024, (name, k)      # four workgroups per CU keep their LDS
