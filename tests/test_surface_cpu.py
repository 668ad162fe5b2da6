"""CPU: the surface-distance metrics below the GPU — the brute-force restatement (tests/surface_ref.py) against scipy.ndimage and
against its committed fixture (tests/golden/surface_metrics.npz), utils.tester._surface_from_raw against the restatement, and the
C ABI's argument checks, which run before anything touches the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import surface_ref as R
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = [(5, 7), (17, 13), (1, 9), (8, 1), (33, 64)]


def _fixture():
    z = np.load(os.path.join(G, "surface_metrics.npz"))
    for name in z["names"]:
        n = str(name)
        q, tol, sp = z["par__" + n]
        yield n, z["P__" + n].astype(bool), z["T__" + n].astype(bool), int(q), float(tol), float(sp), z["out_i__" + n], z["out_d__" + n], z["val__" + n]


def _scipy_metrics(P, T, q, tolerance):
    """The usual host route: binary_erosion for the border, distance_transform_edt for the distances, numpy.percentile."""
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(2, 1)
    bp, bt = P & ~ndi.binary_erosion(P, st, border_value=0), T & ~ndi.binary_erosion(T, st, border_value=0)
    d_pt, d_tp = ndi.distance_transform_edt(~bt)[bp], ndi.distance_transform_edt(~bp)[bt]
    both = np.concatenate([d_pt, d_tp])
    vals = np.array([both.max(), np.percentile(both, q), 0.5 * (d_pt.mean() + d_tp.mean()), (both <= tolerance).mean()])
    return bp, bt, d_pt, d_tp, vals


def _against_scipy(P, T, q=95, tolerance=2.0):
    bp, bt, d_pt, d_tp, vals = _scipy_metrics(P, T, q, tolerance)
    assert np.array_equal(R.border(P), bp) and np.array_equal(R.border(T), bt)
    out_i, out_d = R.raw_one(P, T, q, R.tol2_of(tolerance))
    i_pt, i_tp = np.rint(d_pt ** 2).astype(np.int64), np.rint(d_tp ** 2).astype(np.int64)
    assert np.array_equal(R.directed_d2(np.argwhere(bp), np.argwhere(bt)), i_pt)
    assert np.array_equal(R.directed_d2(np.argwhere(bt), np.argwhere(bp)), i_tp)
    both = np.sort(np.concatenate([i_pt, i_tp]))
    lo, r = (q * (len(both) - 1)) // 100, (q * (len(both) - 1)) % 100
    assert out_i.tolist() == [len(i_pt), len(i_tp), i_pt.max(), i_tp.max(), both[lo], both[lo + (r > 0)], (i_pt <= tolerance ** 2).sum(),
                              (i_tp <= tolerance ** 2).sum()]
    np.testing.assert_allclose(out_d, [d_pt.sum(), d_tp.sum()], rtol=1e-12)
    np.testing.assert_allclose(R.values_one(out_i, out_d, 1.0, q), vals, rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_scipy_on_random_masks(shape):
    for seed, p, q in ((0, 0.5, 95), (1, 0.3, 95), (2, 0.7, 50), (3, 0.5, 0), (4, 0.5, 100)):
        rng = np.random.RandomState(1000 * shape[0] + shape[1] + seed)
        P, T = rng.rand(*shape) < p, rng.rand(*shape) < p
        P.flat[0] = T.flat[-1] = True
        _against_scipy(P, T, q)


def test_restatement_equals_scipy_on_256_ellipses():
    P = R.ellipse(256, 256, 120, 130, 60, 45) | R.ellipse(256, 256, 30, 200, 9, 14)
    T = R.ellipse(256, 256, 126, 124, 55, 50)
    _against_scipy(P, T)
    _against_scipy(R.ellipse(256, 256, 10, 250, 40, 30), R.ellipse(256, 256, 200, 20, 70, 35), 95, 3.0)       # both cut by the frame


def test_border_rule_at_the_frame():
    full = np.ones((6, 9), dtype=bool)
    b = R.border(full)
    assert b[0].all() and b[-1].all() and b[:, 0].all() and b[:, -1].all() and not b[1:-1, 1:-1].any()
    assert R.border(np.ones((1, 9), dtype=bool)).all() and R.border(np.ones((8, 1), dtype=bool)).all()


def test_fixture_covers_what_it_should_and_is_reproduced():
    cases = {c[0]: c for c in _fixture()}
    assert 24 <= len(cases) <= 64 and os.path.getsize(os.path.join(G, "surface_metrics.npz")) < 256 * 1024
    assert [c[0] for c in R.fixture_cases()] == list(cases)
    for name, P, T, q, tol, sp, out_i, out_d, val in cases.values():
        i, d = R.raw_one(P, T, q, R.tol2_of(tol, sp))
        assert np.array_equal(i, out_i) and out_i.dtype == np.int32, name
        np.testing.assert_allclose(d, out_d, rtol=1e-15, atol=0, err_msg=name)
        np.testing.assert_allclose(R.values_one(i, d, sp, q), val, rtol=1e-15, atol=0, err_msg=name)
    # the hand-computable ones
    assert cases["pixel_3_4"][8].tolist() == [5.0, 5.0, 5.0, 0.0] and cases["pixel_3_4"][6].tolist() == [1, 1, 25, 25, 25, 25, 0, 0]
    assert cases["pixel_3_4_spacing"][8].tolist() == [2.5, 2.5, 2.5, 1.0]
    assert cases["identical"][8].tolist() == [0.0, 0.0, 0.0, 1.0] and cases["identical"][6][0] > 0
    assert cases["all_foreground_both"][8].tolist() == [0.0, 0.0, 0.0, 1.0] and cases["all_foreground_both"][6][0] == 2 * 7 + 2 * 5 - 4
    h, hd, assd, sd = cases["rect_shift2"][8]
    assert h == 2.0 and hd == 2.0 and 0.0 < assd < 2.0 and sd == 1.0 and cases["rect_shift2_tol1"][8][3] < 1.0
    assert cases["both_empty"][8].tolist() == [0.0, 0.0, 0.0, 1.0] and not cases["both_empty"][6].any()
    for name, k in (("pred_empty", 1), ("target_empty", 0)):
        assert np.isnan(cases[name][8]).all() and cases[name][6][k] > 0 and not np.delete(cases[name][6], k).any()
        assert not cases[name][7].any()
    assert {c[1].shape for c in cases.values()} >= set(SHAPES)
    assert {c[3] for c in cases.values()} >= {0, 50, 95, 100}


def test_surface_from_raw_reproduces_the_restatement():
    from utils import tester
    cases = list(_fixture())
    out_i, out_d = np.stack([c[6] for c in cases]), np.stack([c[7] for c in cases])
    for sp, q in ((1.0, 95), (0.7, 95), (2.0, 50)):
        got = tester._surface_from_raw(out_i, out_d, sp, q)
        want = R.values(out_i, out_d, sp, q)
        assert list(got) == list(R.NAMES)
        for k in R.NAMES:
            assert got[k].dtype == np.float64 and got[k].shape == (len(cases),)
            np.testing.assert_allclose(got[k], want[k], rtol=1e-14, atol=0, err_msg=f"{k} spacing {sp} q {q}")      # NaN == NaN here
    names = [c[0] for c in cases]
    one = tester._surface_from_raw(out_i, out_d, 1.0, 95)
    for name, nan in (("both_empty", False), ("pred_empty", True), ("target_empty", True)):
        v = [one[k][names.index(name)] for k in R.NAMES]
        assert np.isnan(v).all() if nan else v == [0.0, 0.0, 0.0, 1.0], (name, v)
    # each case with its own parameters gives the recorded values
    for n, P, T, q, tol, sp, i, d, val in cases:
        got = tester._surface_from_raw(i, d, sp, q)
        np.testing.assert_allclose([got[k][0] for k in R.NAMES], val, rtol=1e-14, atol=0, err_msg=n)
    assert tester._surface_tol2(2.0, 1.0) == 4 and tester._surface_tol2(0.3, 0.1) == 9 and tester._surface_tol2(2.6, 0.5) == 27
    assert tester._surface_tol2(2.0, 1.0) == R.tol2_of(2.0) and tester._surface_tol2(0.0, 1.0) == 0


def test_python_surface_keeps_the_existing_signatures():
    from utils import tester
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(tester.surface_metrics_batch) == [("pred", E), ("target", E), ("is_logit", False), ("threshold", 0.5), ("spacing", 1.0),
                                                 ("percentile", 95), ("tolerance", 2.0)]
    assert sig(tester.calculate_surface_metrics) == [("pred", E), ("target", E), ("threshold", 0.5), ("spacing", 1.0), ("percentile", 95),
                                                     ("tolerance", 2.0)]
    assert sig(tester.test_segmentation_model) == [("model", E), ("test_loader", E), ("device", E), ("model_name", E), ("surface", False)]
    assert sig(tester.test_all_models)[-1] == ("surface", False) and sig(tester.test_all_models)[:2] == [("device", "cuda"), ("batch_size", 16)]
    assert sig(tester.calculate_segmentation_metrics) == [("pred", E), ("target", E), ("threshold", 0.5)]
    import torch
    with pytest.raises(ValueError, match="one-channel"):
        tester.surface_metrics_batch(torch.zeros(2, 2, 4, 4), torch.zeros(2, 2, 4, 4))


def test_summary_prints_the_second_table_only_with_surface_results(capsys):
    from utils import tester
    base = {"iou": 80.0, "dice": 88.0, "pixel_accuracy": 97.0, "precision": 90.0, "recall": 87.0, "f1": 88.4}
    tester.print_summary({"AttentionUNet": dict(base)})
    plain = capsys.readouterr().out
    assert "SURFACE" not in plain and "Hausdorff" not in plain
    tester.print_summary({"AttentionUNet": dict(base, hausdorff=12.5, hd95=7.25, assd=1.5, surface_dice=91.0, surface_samples=8)})
    out = capsys.readouterr().out
    assert out.startswith(plain[:plain.index("\U0001F3C6 Best Segmentation")]) and "SURFACE DISTANCES" in out
    row = [l for l in out.splitlines() if l.startswith("AttentionUNet")][1]
    assert row.split() == ["AttentionUNet", "12.50", "7.25", "1.50", "91.00%", "8"]


def test_abi_declares_exports_and_replays_the_new_entry_points():
    protos = L.parse_header()
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, n in (("mi355_surface_ws_ints", 3), ("mi355_surface_distances", 14)):
        assert name in protos and protos[name][0] is ctypes.c_int and len(protos[name][1]) == n, name
        assert hasattr(dll, name), name
        assert arity(name.encode()) == n, name
    assert [n for _, n in protos["mi355_surface_distances"][1]] == ["pred", "target", "B", "H", "W", "is_logit", "thr", "q", "tol2", "ws",
                                                                   "ws_ints", "out_i", "out_d", "s"]
    ws = L.lib.raw("mi355_surface_ws_ints")
    for B, H, W in ((1, 1, 1), (3, 17, 13), (8, 256, 256), (1, 1024, 1024)):
        assert B * H * W * 2 <= ws(B, H, W) <= B * H * W * 4 + 64, (B, H, W)


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    ws_ints, run = lib.raw("mi355_surface_ws_ints"), lib.raw("mi355_surface_distances")
    for bad in ((1, 0, 5), (1, 1025, 8), (1, 8, 1025), (1, 5, 0), (0, 8, 8), (-1, 8, 8)):
        assert ws_ints(*bad) == -1 and b"1024" in err(), (bad, err())
    assert ws_ints(60000, 1024, 1024) == -1 and b"2^31" in err()          # the count would not fit its return type
    need = ws_ints(2, 8, 8)
    assert need > 0
    buf = (ctypes.c_double * 1024)()                    # host memory: never dereferenced, the checks come first
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(pred=p, target=p, B=2, H=8, W=8, is_logit=0, thr=0.5, q=95, tol2=4, ws=p, ws_ints=need, out_i=p, out_d=p)

    def call(**kw):
        a = dict(ok, **kw)
        return run(a["pred"], a["target"], a["B"], a["H"], a["W"], a["is_logit"], a["thr"], a["q"], a["tol2"], a["ws"], a["ws_ints"],
                   a["out_i"], a["out_d"], None)

    for bad, word in (({"pred": None}, b"null"), ({"target": None}, b"null"), ({"ws": None}, b"null"), ({"out_i": None}, b"null"),
                      ({"out_d": None}, b"null"), ({"B": 0}, b"B"), ({"H": 0}, b"1024"), ({"H": 1025}, b"1024"), ({"W": 1025}, b"1024"),
                      ({"q": 101}, b"0..100"), ({"q": -1}, b"0..100"), ({"tol2": -1}, b"negative"), ({"ws_ints": need - 1}, b"too short"),
                      ({"ws_ints": 0}, b"too short")):
        assert call(**bad) == -1, bad
        assert word in err(), (bad, err())
