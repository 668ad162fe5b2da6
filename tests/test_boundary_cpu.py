"""CPU: the boundary loss below the GPU — the integer / fp64 restatement (tests/boundary_ref.py) against brute force, scipy.ndimage
and its committed fixture (tests/golden/boundary_loss.npz), the schedule arithmetic and the argument checks of
mi355.nn.RegionBoundaryLoss / BoundaryLoss, the trainer's flags, and the C ABI's argument checks, which run before anything
touches the device."""
import ctypes
import os

import numpy as np
import pytest

import boundary_ref as R
import seg_loss_ref as S
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(G, "boundary_loss.npz")


def _against_scipy(T):
    ndi = pytest.importorskip("scipy.ndimage")
    d_out, d_in = ndi.distance_transform_edt(~T), ndi.distance_transform_edt(T)
    o2, i2 = np.rint(d_out ** 2), np.rint(d_in ** 2)
    assert np.abs(d_out ** 2 - o2).max() < 1e-9 and np.abs(d_in ** 2 - i2).max() < 1e-9      # squared distances ARE integers
    sd2 = R.signed_dist2(T)
    assert sd2.dtype == np.int32 and np.array_equal(sd2, (o2 * ~T - i2 * T).astype(np.int32))
    # Kervadec's expression, from scipy's own distances
    want = d_out * ~T - (d_in - 1.0) * T
    assert np.abs(R.phi(sd2) - want).max() == 0.0
    return sd2


@pytest.mark.parametrize("shape", R.SHAPES)
def test_restatement_equals_brute_force_and_scipy_on_random_masks(shape):
    for k, p in enumerate(R.DENSITIES):
        T = R.noise(*shape, p, 100 * shape[0] + shape[1] + k)
        T.flat[0], T.flat[-1] = True, False                # both classes present: scipy's all-ones artefact never enters
        sd2 = R.signed_dist2(T)
        assert np.array_equal(sd2, R.signed_dist2_brute(T)), (shape, p)
        assert (sd2[T] <= -1).all() and (sd2[~T] >= 1).all()
        _against_scipy(T)


def test_restatement_equals_scipy_on_256_ellipses_cut_by_the_frame():
    for T in (R.ellipse(256, 256, 120, 130, 60, 45) | R.ellipse(256, 256, 30, 200, 9, 14), R.ellipse(256, 256, 10, 250, 40, 30),
              R.ellipse(256, 256, 200, 20, 70, 35), R.ellipse(256, 256, 128, 128, 300, 90)):
        _against_scipy(T)
    # cut by the frame: the frame is not background, a pixel of the mask on the frame is not at distance 1 because of it
    T = R.ellipse(256, 256, 128, 128, 300, 90)             # a band from top to bottom; row 0 holds columns 47 .. 209 of it
    assert T[0, 47] and T[0, 209] and not T[0, 46] and not T[0, 210] and R.signed_dist2(T)[0, 128] == -(82 ** 2)


def test_hand_computable_cases():
    a = np.zeros((8, 9), dtype=bool)
    a[3, 4] = True
    sd2 = R.signed_dist2(a)
    yy, xx = np.mgrid[:8, :9]
    want = (yy - 3) ** 2 + (xx - 4) ** 2
    want[3, 4] = -1
    assert sd2[0, 0] == 25 and np.array_equal(sd2, want)
    assert np.array_equal(R.signed_dist2(~a), np.where(a, 1, -want)) and R.signed_dist2(~a)[0, 0] == -25
    for T in (np.zeros((7, 5), dtype=bool), np.ones((7, 5), dtype=bool), np.ones((1, 1), dtype=bool)):
        assert not R.signed_dist2(T).any() and not R.signed_dist2_brute(T).any()
    e = R.ellipse(17, 13, 8, 6, 6, 4)
    batch = np.stack([np.zeros_like(e), e, np.ones_like(e), ~e])
    got = R.signed_dist2(batch)
    assert not got[0].any() and not got[2].any() and np.array_equal(got[1], R.signed_dist2(e)) and np.array_equal(got[3], -got[1])
    assert R.phi(np.array([25, 1, 0, -1, -4, -25])).tolist() == [5.0, 1.0, 0.0, 0.0, -1.0, -4.0]


def test_loss_restatement_is_its_own_derivative():
    rng = np.random.RandomState(5)
    T = R.noise(6, 7, 0.4, 1)[None]
    sd2, z = R.signed_dist2(T), rng.randn(1, 6, 7) * 2
    loss, grad = R.boundary_loss(z, sd2, 0.7)
    assert abs(loss - 0.7 * np.mean(S.sigmoid(z) * R.phi(sd2))) < 1e-15
    h = 1e-6
    for i in ((0, 0, 0), (0, 3, 4), (0, 5, 6)):
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        num = (R.boundary_loss(zp, sd2, 0.7)[0] - R.boundary_loss(zm, sd2, 0.7)[0]) / (2 * h)
        assert abs(num - grad[i]) < 1e-8 * max(1.0, abs(grad[i]))
    # region_boundary = the two restatements with the schedule's factors
    t = T.astype(np.float64)
    for sched, ep, r, a in (("constant", 9, 1.0, 0.3), ("rebalance", 0, 0.7, 0.3), ("rebalance", 5, 0.65, 0.35), ("rebalance", 200, 0.01, 0.99)):
        l, g, A = R.region_boundary(z, t, 0.5, 0.5, 0.3, 1.0, False, sched, ep)
        lr, gr = S.seg_loss(z, t, r * 0.5, r * 0.5, 1.0, False)
        lb, gb = R.boundary_loss(z, sd2, a)
        assert abs(l - (lr + lb)) < 1e-14 and np.abs(g - (gr + gb)).max() < 1e-16 and A > 0


def test_fixture_covers_what_it_should_and_is_reproduced():
    stored = R.load_fixture(FIXTURE)
    cases = R.fixture_cases()
    assert 24 <= len(stored) <= 64 and os.path.getsize(FIXTURE) < 256 * 1024
    assert [c[0] for c in cases] == [s[0] for s in stored]
    for (name, T, z, w), (_, T_s, sd2, w_s, loss, grad) in zip(cases, stored):
        assert np.array_equal(T, T_s) and w == w_s and z.dtype == np.float32 and sd2.dtype == np.int32, name
        assert np.array_equal(R.signed_dist2(T), sd2), name
        if T.size <= 2500:
            assert np.array_equal(R.signed_dist2_brute(T), sd2), name
        l, g = R.boundary_loss(z, sd2, w)
        np.testing.assert_allclose(l, loss, rtol=1e-14, atol=1e-300, err_msg=name)
        np.testing.assert_allclose(g, grad, rtol=1e-14, atol=1e-300, err_msg=name)
    by = {s[0]: s for s in stored}
    assert by["pixel_3_4"][2][0, 0, 0] == 25 and by["background_pixel_3_4"][2][0, 0, 0] == -25
    assert not by["empty"][2].any() and not by["full"][2].any() and by["empty"][4] == 0.0 and not by["full"][5].any()
    mixed = by["degenerate_and_normal"]
    assert not mixed[2][0].any() and not mixed[2][2].any() and mixed[2][1].any() and mixed[2][3].any()
    assert {s[1].shape[1:] for s in stored} >= set(R.SHAPES)


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_schedule_arithmetic():
    from mi355 import nn as mnn
    c = mnn.RegionBoundaryLoss()
    assert c.current_weights() == (1.0, 0.01)
    c.on_epoch(7, 20)
    assert c.current_weights() == (1.0, 0.01)              # constant: the epoch does not matter
    r = mnn.RegionBoundaryLoss(schedule="rebalance")
    assert r.current_weights() == pytest.approx((0.99, 0.01), abs=1e-12)
    for ep, want in ((0, (0.99, 0.01)), (1, (0.98, 0.02)), (2, (0.97, 0.03)), (50, (0.49, 0.51)), (98, (0.01, 0.99)), (99, (0.01, 0.99)),
                     (200, (0.01, 0.99))):
        r.on_epoch(ep, 300)
        assert r.current_weights() == pytest.approx(want, abs=1e-12), ep
        assert r.current_weights() == pytest.approx(R.schedule_weights(0.01, "rebalance", ep), abs=1e-15)
    q = mnn.RegionBoundaryLoss(boundary_weight=0.3, schedule="rebalance", step=0.1, max_weight=0.5)
    for ep, want in ((0, (0.7, 0.3)), (1, (0.6, 0.4)), (2, (0.5, 0.5)), (3, (0.5, 0.5)), (1000, (0.5, 0.5))):
        q.on_epoch(ep, 1001)
        assert q.current_weights() == pytest.approx(want, abs=1e-12), ep


def test_constructor_checks_and_one_channel_error():
    import torch
    from mi355 import nn as mnn
    for kw in ({"bce_weight": -1}, {"dice_weight": -0.1}, {"boundary_weight": -0.01}, {"smooth": -1}, {"step": -0.5},
               {"schedule": "linear"}, {"max_weight": 1.5}):
        with pytest.raises(ValueError):
            mnn.RegionBoundaryLoss(**kw)
    with pytest.raises(ValueError):
        mnn.BoundaryLoss(weight=-1.0)
    c = mnn.RegionBoundaryLoss()
    assert (c.bce_weight, c.dice_weight, c.boundary_weight, c.smooth, c.per_sample, c.schedule, c.step, c.max_weight) == \
        (0.5, 0.5, 0.01, 1.0, False, "constant", 0.01, 0.99)
    b = mnn.BoundaryLoss()
    assert (b.weight, b.threshold) == (1.0, 0.5)
    for crit in (c, b):
        for shape in ((2, 2, 4, 4), (2, 16), (2, 1, 1, 4, 4)):          # raised before anything touches a device
            with pytest.raises(ValueError, match="one-channel"):
                crit(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match="must match input size"):
        c(torch.zeros(2, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_trainer_flags_keep_todays_criteria_by_default():
    from mi355 import nn as mnn
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.boundary_weight, d.boundary_schedule, d.boundary_step) == (0.0, "constant", 0.01)
    assert trainer.seg_criterion(d) is None
    assert trainer.seg_criterion(ap.parse_args(["--boundary-weight", "0"])) is None
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice", "--boundary-weight", "0"]))
    assert type(c) is mnn.DiceLoss
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "bce_dice", "--bce-weight", "0.3", "--dice-weight", "0.7"]))
    assert type(c) is mnn.CombinedLoss and (c.bce_weight, c.dice_weight) == (0.3, 0.7)
    for loss, extra, want in (("bce", [], (1.0, 0.0)), ("dice", [], (0.0, 1.0)), ("bce_dice", [], (0.5, 0.5)),
                              ("bce_dice", ["--bce-weight", "0.3", "--dice-weight", "0.7"], (0.3, 0.7))):
        c = trainer.seg_criterion(ap.parse_args(["--seg-loss", loss, "--boundary-weight", "0.05"] + extra))
        assert type(c) is mnn.RegionBoundaryLoss and (c.bce_weight, c.dice_weight) == want and c.boundary_weight == 0.05
        assert c.schedule == "constant" and not c.per_sample
    c = trainer.seg_criterion(ap.parse_args(["--seg-loss", "dice", "--boundary-weight", "0.02", "--boundary-schedule", "rebalance",
                                             "--boundary-step", "0.005", "--dice-per-sample"]))
    assert (c.schedule, c.step, c.per_sample, c.boundary_weight) == ("rebalance", 0.005, True, 0.02)
    with pytest.raises(ValueError):
        trainer.seg_criterion(ap.parse_args(["--boundary-weight", "-1"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--boundary-schedule", "cosine"])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = {"mi355_sdist_ws_ints": ["B", "H", "W"],
         "mi355_signed_dist2": ["target", "B", "H", "W", "thr", "ws", "ws_ints", "sd2", "s"],
         "mi355_boundary_loss_rows": ["B", "per"],
         "mi355_boundary_loss_fwd": ["z", "sd2", "B", "per", "weight", "base", "partial", "loss", "s"],
         "mi355_boundary_loss_bwd": ["z", "sd2", "B", "per", "weight", "gscale", "accumulate", "dz", "s"]}


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
    ws = L.lib.raw("mi355_sdist_ws_ints")
    for B, H, W in ((1, 1, 1), (3, 17, 13), (32, 256, 256), (1, 1024, 1024)):
        assert B * H * W <= ws(B, H, W) <= B * H * W * 2 + 64, (B, H, W)
    rows = L.lib.raw("mi355_boundary_loss_rows")
    for B, per in ((1, 1), (3, 221), (32, 65536), (1, 1 << 20), (65535, 4)):
        assert B <= rows(B, per) <= 256 * B and rows(B, per) % B == 0, (B, per)


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    ws_ints, run = lib.raw("mi355_sdist_ws_ints"), lib.raw("mi355_signed_dist2")
    for bad in ((1, 0, 5), (1, 1025, 8), (1, 8, 1025), (1, 5, 0), (0, 8, 8), (-1, 8, 8), (65536, 8, 8)):
        assert ws_ints(*bad) == -1 and b"1024" in err(), (bad, err())
    assert ws_ints(60000, 1024, 1024) == -1 and b"2^31" in err()          # the count would not fit its return type
    need = ws_ints(2, 8, 8)
    assert need > 0
    buf = (ctypes.c_double * 1024)()                    # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(target=p, B=2, H=8, W=8, thr=0.5, ws=p, ws_ints=need, sd2=p)

    def call(**kw):
        a = dict(ok, **kw)
        return run(a["target"], a["B"], a["H"], a["W"], a["thr"], a["ws"], a["ws_ints"], a["sd2"], None)

    for bad, word in (({"target": None}, b"null pointer (target)"), ({"ws": None}, b"null pointer (ws)"),
                      ({"sd2": None}, b"null pointer (sd2)"), ({"B": 0}, b"B"), ({"B": 65536}, b"65535"), ({"H": 0}, b"1024"),
                      ({"H": 1025}, b"1024"), ({"W": 1025}, b"1024"), ({"W": 0}, b"1024"), ({"ws_ints": need - 1}, b"too short"),
                      ({"ws_ints": 0}, b"too short")):
        assert call(**bad) == -1, bad
        assert word in err() and b"signed_dist2" in err(), (bad, err())

    rows, fwd, bwd = lib.raw("mi355_boundary_loss_rows"), lib.raw("mi355_boundary_loss_fwd"), lib.raw("mi355_boundary_loss_bwd")
    for bad in ((0, 16), (-1, 16), (65536, 16), (2, 0), (2, -4)):
        assert rows(*bad) == -1 and b"boundary_loss_rows" in err() and b"per" in err(), (bad, err())
    okf = dict(z=p, sd2=p, B=2, per=64, weight=1.0, base=None, partial=p, loss=p)
    okb = dict(z=p, sd2=p, B=2, per=64, weight=1.0, gscale=None, accumulate=0, dz=p)

    def call_f(**kw):
        a = dict(okf, **kw)
        return fwd(a["z"], a["sd2"], a["B"], a["per"], a["weight"], a["base"], a["partial"], a["loss"], None)

    def call_b(**kw):
        a = dict(okb, **kw)
        return bwd(a["z"], a["sd2"], a["B"], a["per"], a["weight"], a["gscale"], a["accumulate"], a["dz"], None)

    for bad, word in (({"z": None}, b"null pointer (z)"), ({"sd2": None}, b"null pointer (sd2)"), ({"partial": None}, b"null pointer (partial)"),
                      ({"loss": None}, b"null pointer (loss)"), ({"B": 0}, b"B"), ({"B": 65536}, b"65535"), ({"per": 0}, b"per"),
                      ({"per": -1}, b"per"), ({"weight": -0.5}, b"weight")):
        assert call_f(**bad) == -1, bad
        assert word in err() and b"boundary_loss_fwd" in err(), (bad, err())
    for bad, word in (({"z": None}, b"null pointer (z)"), ({"sd2": None}, b"null pointer (sd2)"), ({"dz": None}, b"null pointer (dz)"),
                      ({"B": 0}, b"B"), ({"per": 0}, b"per"), ({"weight": -0.5}, b"weight"), ({"weight": float("nan")}, b"weight")):
        assert call_b(**bad) == -1, bad
        assert word in err() and b"boundary_loss_bwd" in err(), (bad, err())
