"""CPU: the numpy restatement tests/sliding_ref.py pinned to hand-derived facts, the host side of utils/sliding.py (window starts,
weights, validation), the tester's flags, the pipeline's options, and what the built library says about the two new entry points
without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sliding_ref as R
from mi355 import lib as L

BUILT = pytest.mark.skipif(not os.path.exists(L.SO_PATH), reason="libmi355conv.so not built (run __graft_entry__.build())")

STARTS = [((37, 16, 0.25), [0, 12, 21]), ((45, 16, 0.25), [0, 12, 24, 29]), ((17, 16, 0.5), [0, 1]), ((112, 64, 0.5), [0, 32, 48]),
          ((33, 16, 0), [0, 16, 17]), ((512, 256, 0.5), [0, 128, 256])]


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,want", STARTS)
def test_tile_starts_quoted_cases(args, want):
    from utils.sliding import tile_starts
    got = tile_starts(*args)
    assert got == want == R.tile_starts(*args) and all(isinstance(s, int) for s in got)


def test_tile_starts_at_the_largest_overlap_is_seven_starts_four_deep():
    from utils.sliding import tile_starts
    got = tile_starts(40, 16, 0.75)
    assert got == [0, 4, 8, 12, 16, 20, 24] == R.tile_starts(40, 16, 0.75)
    assert R.coverage(40, got, 16).max() == 4 == R.depth_bound(40, 16, 0.75)


def test_every_pixel_is_covered_and_no_deeper_than_derived():
    from utils.sliding import tile_starts
    rng = np.random.default_rng(0)
    cases = [a for a, _ in STARTS] + [(43, 16, 0.25), (64, 64, 0.5), (7, 5, 0.5), (9, 5, 0.5), (96, 64, 0.5), (1, 1, 0.0)]
    for _ in range(300):
        tile = int(rng.integers(1, 40))
        cases.append((tile + int(rng.integers(0, 60)), tile, float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.6, 0.75]))))
    deepest = 0
    for extent, tile, overlap in cases:
        s = tile_starts(extent, tile, overlap)
        assert s == R.tile_starts(extent, tile, overlap), (extent, tile, overlap)
        assert s[0] == 0 and s[-1] == extent - tile and all(0 < b - a <= tile for a, b in zip(s, s[1:])) and len(s) <= 64
        cov = R.coverage(extent, s, tile)
        depth = R.depth_bound(extent, tile, overlap)
        assert cov.min() >= 1 and cov.max() <= depth, (extent, tile, overlap, cov.max(), depth)
        deepest = max(deepest, cov.max())
    assert R.coverage(43, tile_starts(43, 16, 0.25), 16).max() == 3 == R.depth_bound(43, 16, 0.25)      # the pulled-back start is one more
    assert deepest >= 4


def test_window_weights():
    from utils.sliding import window_weights
    g = window_weights(16, "gaussian")
    assert g.dtype == np.float32 and g.shape == (16,) and np.array_equal(g, R.window_weights(16, "gaussian"))
    assert np.allclose(g[:4], [1e-3, 0.00508607, 0.02279418, 0.07955951], rtol=2e-6, atol=0)
    assert g[0] == np.float32(1e-3) and np.array_equal(g, g[::-1]) and g.min() > 0 and g.argmax() in (7, 8)
    want = np.exp(-0.5 * ((np.arange(16) - 7.5) / 2.0) ** 2)
    assert np.array_equal(g, np.maximum(want, 1e-3).astype(np.float32))                        # float64, rounded once
    c = window_weights(5, "constant")
    assert c.dtype == np.float32 and np.array_equal(c, np.ones(5, np.float32))
    g256 = window_weights(256, "gaussian")
    assert np.array_equal(g256, R.window_weights(256, "gaussian")) and g256.min() == np.float32(1e-3) and g256.max() > 0.999
    two = np.outer(g, g)                                                                       # the 2-D weight: the separable Gaussian
    yy, xx = np.mgrid[0:16, 0:16]
    inner = (want[:, None] >= 1e-3) & (want[None, :] >= 1e-3)
    assert np.allclose(two[inner], np.exp(-0.5 * (((yy - 7.5) / 2.0) ** 2 + ((xx - 7.5) / 2.0) ** 2))[inner], rtol=1e-6)


def test_bad_options():
    from utils.sliding import SlidingWindowSegmenter, blend_tiles, check_sliding, gather_tiles, tile_starts, window_weights
    for args in ((64, 16, 0.8), (64, 16, -0.1), (64, 16, float("nan")), (15, 16, 0.5), (64, 0, 0.5), (1000, 4, 0.75)):
        with pytest.raises(ValueError, match="sliding"):
            tile_starts(*args)
    assert len(tile_starts(67, 4, 0.75)) == 64                                                 # the cap itself is allowed
    with pytest.raises(ValueError, match="weighting"):
        window_weights(16, "hann")
    for bad in ((16, 0.8, "gaussian"), (16, 0.5, "hann"), (0, 0.5, "gaussian"), (16, 0.5), "gaussian", 16):
        with pytest.raises(ValueError):
            check_sliding(bad)
    assert check_sliding([64, 0, "constant"]) == (64, 0.0, "constant")
    model = torch.nn.Identity()
    for kw in ({"overlap": 0.8}, {"weighting": "hann"}, {"merge": "mean"}, {"batch": 0}, {"tile": 0}):
        with pytest.raises(ValueError):
            SlidingWindowSegmenter(model, **kw)
    seg = SlidingWindowSegmenter(model.train(), tile=16, batch=2)
    assert seg.eval() is seg and not model.training and seg.grid(37, 45) == ([0, 8, 16, 21], [0, 8, 16, 24, 29])
    with pytest.raises(ValueError, match="GPU"):
        gather_tiles(torch.zeros(1, 1, 8, 8), 4, 0.5)
    with pytest.raises(ValueError, match="GPU"):
        blend_tiles(torch.zeros(9, 4, 4), (1, 8, 8), 4, 0.5)
    with pytest.raises(ValueError, match="merge"):
        blend_tiles(torch.zeros(9, 4, 4), (1, 8, 8), 4, 0.5, merge="mean")
    with pytest.raises(ValueError, match="GPU"):
        seg(torch.zeros(1, 3, 32, 32))


def test_tta_together_with_sliding_is_refused():
    from utils import tester
    from utils.pipeline import JointPipeline
    with pytest.raises(ValueError, match="sliding together with tta"):
        tester.test_all_models(tta="hflip", sliding=(64, 0.5, "gaussian"))
    with pytest.raises(ValueError, match="at least the tile"):
        tester.test_all_models(sliding=(64, 0.5, "gaussian"), size=32)
    with pytest.raises(ValueError):
        tester.test_all_models(sliding=(64, 0.8, "gaussian"))
    ident = torch.nn.Identity()
    with pytest.raises(ValueError, match="together with tta"):
        JointPipeline(ident, None, "cpu", tta="hflip", sliding=(64, 0.5, "gaussian"))
    p = JointPipeline(ident, None, "cpu", sliding=[64, 0.5, "constant"], seg_size=128)
    assert p.sliding == (64, 0.5, "constant") and p.seg_size == 128 and p.tta is None
    with pytest.raises(ValueError, match="together with sliding"):
        p.tta = "hflip"
    p.sliding = None
    p.tta = "hflip"
    with pytest.raises(ValueError, match="together with tta"):
        p.sliding = (64, 0.5, "gaussian")
    for bad in ((64, 0.8, "gaussian"), (64, 0.5, "hann"), 64):
        with pytest.raises(ValueError):
            JointPipeline(ident, None, "cpu", sliding=bad)
    for bad in (0, -4, 1.5, True):
        with pytest.raises(ValueError, match="seg_size"):
            JointPipeline(ident, None, "cpu", seg_size=bad)
    seg_model = torch.nn.Identity()
    q = JointPipeline(ident, seg_model, "cpu", sliding=(64, 0.5, "constant"), bucket=2)
    w = q._window_segmenter()                                                                  # one wrapper, kept between calls ...
    assert q._window_segmenter() is w and w.model is seg_model and (w.tile, w.overlap, w.weighting, w.merge, w.batch) == (64, 0.5, "constant", "logit", 2)
    q.sliding = (32, 0.25, "gaussian")                                                         # ... until what it was built from changes
    w2 = q._window_segmenter()
    assert w2 is not w and (w2.tile, w2.overlap, w2.weighting) == (32, 0.25, "gaussian") and q._window_segmenter() is w2
    q.bucket = 4
    assert q._window_segmenter().batch == 4
    off = JointPipeline(ident, None, "cpu")
    assert off.sliding is None and off.seg_size is None                                        # off by default
    with pytest.raises(ValueError, match="x_seg"):
        off.predict(torch.zeros(1, 3, 8, 8), x_seg=torch.zeros(1, 3, 16, 16))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_one_constant_tile_returns_the_bits_of_z():
    z = R.normal_maps((2, 8, 8), 1)
    z[0, 0, 0], z[1, 3, 3] = -0.0, 0.0
    one = np.ones(8, np.float32)
    r = R.blend_ref(z, 2, 8, 8, 8, [0], [0], one, one, 0)
    want = z + np.float32(0)                                                                   # (0 + -0 = +0, as on the device)
    assert r["mean"].dtype == np.float32 and np.array_equal(_bits(r["mean"]), _bits(want))
    assert (r["spread"] == 0).all() and (r["cover"] == 1).all()
    assert np.array_equal(r["mask"], np.where(z > 0, 255, 0))                                  # sigmoid(v) > 0.5 iff v > 0


def test_two_half_overlapping_constant_tiles():
    T, W = 8, 12
    z = R.normal_maps((2, T, T), 2)                                                            # N = 1, Py = 1, Px = 2: xs = [0, 4]
    one = np.ones(T, np.float32)
    r = R.blend_ref(z, 1, T, W, T, [0], [0, 4], one, one, 0)
    assert np.array_equal(r["cover"], np.tile([1] * 4 + [2] * 4 + [1] * 4, (T, 1)))
    assert np.array_equal(_bits(r["mean"][0, :, :4]), _bits(z[0][:, :4] + np.float32(0)))
    assert np.array_equal(_bits(r["mean"][0, :, 8:]), _bits(z[1][:, 4:] + np.float32(0)))
    seam = (z[0][:, 4:] + z[1][:, :4]) / np.float32(2)                                         # the plain mean, float32
    assert np.array_equal(_bits(r["mean"][0, :, 4:8]), _bits(seam))
    assert np.array_equal(r["spread"][0, :, 4:8], np.abs(z[0][:, 4:] - z[1][:, :4]))
    assert (r["spread"][0][r["cover"] == 1] == 0).all() and (r["spread"][0][r["cover"] == 2] > 0).all()


def test_weighted_blend_by_hand_and_the_float64_variant():
    T, H, W = 4, 6, 7
    ys, xs = [0, 2], [0, 3]
    assert ys == R.tile_starts(H, T, 0.5) and xs == R.tile_starts(W, T, 0.25)
    z = R.normal_maps((2 * 4, T, T), 3)
    w = np.array([0.25, 1.0, 0.75, 0.125], np.float32)
    r = R.blend_ref(z, 2, H, W, T, ys, xs, w, w, 0)
    # pixel (y, x) = (3, 3) of sample 1: tiles (0,0) at (3,3), (0,1) at (3,0), (1,0) at (1,3), (1,1) at (1,0), in that order
    f = np.float32
    terms = [(f(w[3] * w[3]), z[4][3, 3]), (f(w[3] * w[0]), z[5][3, 0]), (f(w[1] * w[3]), z[6][1, 3]), (f(w[1] * w[0]), z[7][1, 0])]
    num = den = f(0)
    for wt, v in terms:
        num, den = f(num + f(wt * v)), f(den + wt)
    assert r["cover"][3, 3] == 4 and r["mean"][1, 3, 3] == f(num / den)
    assert r["spread"][1, 3, 3] == f(max(v for _, v in terms) - min(v for _, v in terms))
    e = R.blend_ref(z, 2, H, W, T, ys, xs, w, w, 0, exact=True)
    assert e["mean"].dtype == np.float64
    assert np.abs(r["mean"] - e["mean"]).max() <= R.blend_logit_bound(4, r["vmax"])
    p = R.blend_ref(z, 2, H, W, T, ys, xs, w, w, 1)
    assert p["mean"].dtype == np.float64 and 0 < p["mean"].min() and p["mean"].max() < 1 and (p["spread"] >= 0).all()
    assert np.array_equal(p["cover"], r["cover"]) and (p["spread"][:, p["cover"] == 1] == 0).all()
    assert R.blend_prob_bound(16) < 2.3e-6 and R.blend_prob_bound(1) == R.SIGMOID_ERR + 3 * R.U


def test_gather_ref_is_slicing():
    x = R.normal_maps((2, 3, 7, 9), 4)
    ys, xs = R.tile_starts(7, 5, 0.5), R.tile_starts(9, 5, 0.5)
    assert (ys, xs) == ([0, 2], [0, 2, 4])
    g = R.gather_ref(x, 5, ys, xs, [0, 11, 4, 4])
    assert g.shape == (4, 3, 5, 5)
    assert np.array_equal(g[0], x[0, :, 0:5, 0:5]) and np.array_equal(g[1], x[1, :, 2:7, 4:9]) and np.array_equal(g[2], x[0, :, 2:7, 2:7])
    assert np.array_equal(g[2], g[3])


# ---- parser ---------------------------------------------------------------------------------------------------------------------------
def test_tester_flags():
    from utils import tester
    ap = tester.build_parser()
    d = ap.parse_args([])
    assert (d.sw_tile, d.sw_overlap, d.sw_weight, d.size) == (0, 0.5, "gaussian", tester.IMG_SIZE)      # sliding is off by default
    a = ap.parse_args("--sw-tile 256 --sw-overlap 0.25 --sw-weight constant --size 512".split())
    assert (a.sw_tile, a.sw_overlap, a.sw_weight, a.size) == (256, 0.25, "constant", 512)
    with pytest.raises(SystemExit):
        ap.parse_args(["--sw-weight", "hann"])
    import inspect
    sig = inspect.signature(tester.test_all_models).parameters
    assert sig["sliding"].default is None and sig["size"].default is None


# ---- the library, without a GPU -------------------------------------------------------------------------------------------------------
@BUILT
def test_library_exports_both_symbols_and_the_plan_table_knows_them():
    protos = L.parse_header()
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, n in (("mi355_tile_gather_f32", 14), ("mi355_tile_blend", 19)):
        assert name in protos and len(protos[name][1]) == n and protos[name][1][-1][1] == "s"
        assert hasattr(dll, name) and arity(name.encode()) == n


@BUILT
def test_launchers_refuse_bad_calls_before_touching_the_device():
    """bad sizes, null pointers and invalid starts are all refused from the arguments alone (the device addresses are never
    dereferenced, and the host arrays only once the sizes are known to be good)"""
    L.lib.load()
    gather, blend, err = L.lib.raw("mi355_tile_gather_f32"), L.lib.raw("mi355_tile_blend"), L.lib.raw("mi355_last_error")
    buf = (ctypes.c_float * 1024)()
    p = ctypes.addressof(buf)
    I3, I = ctypes.c_int32 * 3, ctypes.c_int32 * 4
    ys, xs = I3(0, 12, 21), I(0, 12, 24, 29)                                                   # 37 x 45, T = 16, overlap 0.25
    ay, ax = ctypes.addressof(ys), ctypes.addressof(xs)

    def g(**kw):
        a = dict(src=p, N=2, C=3, H=37, W=45, T=16, ys=ay, Py=3, xs=ax, Px=4, tiles=p, M=5, dst=p + 2048)
        a.update(kw)
        return gather(a["src"], a["N"], a["C"], a["H"], a["W"], a["T"], a["ys"], a["Py"], a["xs"], a["Px"], a["tiles"], a["M"], a["dst"], None)

    def b(**kw):
        a = dict(z=p, N=2, H=37, W=45, T=16, ys=ay, Py=3, xs=ax, Px=4, wy=p, wx=p, mean=p + 2048)
        a.update(kw)
        return blend(a["z"], a["N"], a["H"], a["W"], a["T"], a["ys"], a["Py"], a["xs"], a["Px"], a["wy"], a["wx"], 0, ctypes.c_float(0.5), None,
                     a["mean"], None, None, None, None)

    for kw in ({"T": 0}, {"T": 38}, {"T": 46, "H": 64}, {"M": 0}, {"N": 0}, {"C": 0}, {"src": None}, {"tiles": None}, {"dst": None},
               {"ys": None}, {"xs": None}, {"dst": p}, {"Py": 0}, {"Px": 65}):
        assert g(**kw) != 0, kw
        assert b"tile_gather_f32" in err(), (kw, err())
    for kw in ({"T": 0}, {"T": 38}, {"N": 0}, {"z": None}, {"wy": None}, {"wx": None}, {"mean": None}, {"ys": None}, {"xs": None}, {"Py": 65}):
        assert b(**kw) != 0, kw
        assert b"tile_blend" in err(), (kw, err())
    for bad, what in ((I(0, 8, 12, 29), b"gap"), (I(0, 12, 24, 28), b"last"), (I(0, 12, 12, 29), b"ascending"), (I(0, 24, 12, 29), b"gap"),
                      (I(1, 12, 24, 29), b"first"), (I(0, 13, 13, 29), b"ascending")):
        for fn in (g, b):
            assert fn(xs=ctypes.addressof(bad)) != 0
            assert b"xs" in err() and what in err(), (list(bad), err())
    assert g(ys=ctypes.addressof(I3(0, 4, 21))) != 0 and b"ys" in err() and b"gap" in err()
    # cover is a uint8 plane: a grid on which 16 x 16 = 256 tiles cover one pixel is refused
    I16 = ctypes.c_int32 * 16
    dense = I16(*range(16))                                                                    # T = 16 on 31 pixels
    for fn in (g, b):
        assert fn(H=31, W=31, ys=ctypes.addressof(dense), Py=16, xs=ctypes.addressof(dense), Px=16) != 0
        assert b"256 tiles cover one pixel" in err(), err()
