"""CPU: the connected-component clean-up below the GPU — the restatement (tests/components_ref.py) against scipy.ndimage and against
its committed fixture (tests/golden/components.npz), the rank and tie rule, the C ABI's prototypes and argument checks (which run
before anything touches the device) and the Python argument errors of utils.postprocess."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import components_ref as R
from mi355 import lib as L

G = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = [(17, 13), (1, 9), (8, 1), (64, 64), (40, 300)]
NAMES = ("mi355_components_ws_ints", "mi355_components")


def _against_scipy(m, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(2, 1 if conn == 4 else 2)
    lab, n = ndi.label(m, structure=st)
    a = R.analyse(m, conn, 0)
    assert np.array_equal(a["labels"], lab) and len(a["table"]) == n
    for fill in (4, 8):
        want = ndi.binary_fill_holes(m, structure=ndi.generate_binary_structure(2, 1 if fill == 4 else 2))
        assert np.array_equal(R.fill_holes(m, fill), want), (conn, fill)
        assert np.array_equal(R.analyse(m, conn, fill)["labels"], ndi.label(want, structure=st)[0])
    t = a["table"]
    for k, sl in enumerate(ndi.find_objects(lab)):
        assert (t[k, 2], t[k, 4] + 1, t[k, 3], t[k, 5] + 1) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
    if n:
        com = np.array(ndi.center_of_mass(m, lab, np.arange(1, n + 1)))
        np.testing.assert_allclose(R.centroids(t), com, rtol=1e-12, atol=1e-12)
        assert np.array_equal(t[:, 0], ndi.sum(m, lab, np.arange(1, n + 1)).astype(np.int64))
        assert np.array_equal(t[:, 1], [np.flatnonzero(lab == k + 1)[0] for k in range(n)]) and (np.diff(t[:, 1]) > 0).all()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_scipy(shape, conn):
    for k, p in enumerate((0.3, 0.5, 0.6)):
        _against_scipy(R.noise(*shape, p, 1000 * shape[0] + shape[1] + k), conn)
    for kind, M in R.kinds(2, *shape, seed=sum(shape)).items():
        for m in M:
            _against_scipy(m, conn)


def test_structured_cases_are_what_they_claim():
    k = R.kinds(1, 16, 20, 0)
    count = lambda m, c, f=0: len(R.analyse(m, c, f)["table"])
    assert count(k["checkerboard"][0], 4) == 160 and count(k["checkerboard"][0], 8) == 1
    assert count(k["comb"][0], 4) == 1 and count(k["comb"][0][:-1], 4) == 10
    assert count(k["diagonal"][0], 8) == 1 and count(k["diagonal"][0], 4) == 16
    u = k["u_and_ring"][0]
    added = lambda f: int(R.fill_holes(u, f).sum() - u.sum())
    assert added(4) > added(8) > 0                               # the cut ring fills under the 4-structure only, the U never
    inside_u = (slice(0, 7), slice(1, 8))
    assert not R.fill_holes(u, 4)[inside_u].all() and not u[inside_u].any()
    assert count(k["squares"][0], 8) >= 6 and len(set(R.analyse(k["squares"][0], 8)["table"][:, 0])) == 1


def test_rank_and_tie_rule_on_equal_areas():
    m = np.zeros((12, 20), dtype=bool)
    for y, x in ((0, 0), (0, 8), (5, 3), (8, 12)):
        m[y:y + 2, x:x + 2] = True                               # four blobs of area 4 ...
    m[4:7, 14:18] = True                                         # ... one of 12 that comes third in raster order
    m[11, 19] = True
    a = R.analyse(m, 8)
    assert a["table"][:, 0].tolist() == [4, 4, 12, 4, 4, 1]
    mask, out_i, out_c = R.finish(a, 0, 3, 8)
    assert out_i.tolist() == [29, 0, 6, 3, 20, 12, 3, 0]
    assert out_c[:3, 1].tolist() == [4 * 20 + 14, 0, 8] and not out_c[3:].any()      # the largest, then the ties by first pixel
    assert mask[0, 0] == 255 and mask[0, 8] == 255 and mask[5, 3] == 0 and mask[8, 12] == 0 and mask[4, 14] == 255
    mask, out_i, out_c = R.finish(a, 2, 0, 2)
    assert out_i.tolist() == [29, 0, 6, 5, 28, 12, 2, 0] and mask[11, 19] == 0 and out_c[:, 0].tolist() == [12, 4]
    mask, out_i, out_c = R.finish(a, 5, 4, 16)                   # both filters: rank < 4 and area >= 5
    assert out_i.tolist() == [29, 0, 6, 1, 12, 12, 1, 0] and out_c.shape == (16, 8)
    assert np.isnan(R.centroids(out_c)[1:]).all() and R.centroids(out_c)[0].tolist() == [5.0, 15.5]


def _fixture():
    z = np.load(os.path.join(G, "components.npz"))
    for name in z["names"]:
        n = str(name)
        H, W, conn, fill, mn, kl, mr = (int(v) for v in z["par__" + n])
        m = np.unpackbits(z["m__" + n], axis=1)[:, :W].astype(bool)
        mask = np.unpackbits(z["mask__" + n], axis=1)[:, :W].astype(np.uint8) * 255
        yield n, m, conn, fill, mn, kl, mr, mask, z["labels__" + n], z["out_i__" + n], z["out_c__" + n]


def test_fixture_is_reproduced():
    cases = list(_fixture())
    assert len(cases) >= 64 and os.path.getsize(os.path.join(G, "components.npz")) < 256 * 1024
    assert [c[0] for c in cases] == [c[0] for c in R.fixture_cases()]
    for n, m, conn, fill, mn, kl, mr, mask, labels, out_i, out_c in cases:
        a = R.analyse(m, conn, fill)
        got = R.finish(a, mn, kl, mr)
        assert np.array_equal(a["labels"], labels) and np.array_equal(got[0], mask), n
        assert np.array_equal(got[1], out_i) and np.array_equal(got[2], out_c) and out_i.dtype == np.int32 and out_c.dtype == np.int32, n
    assert {c[1].shape for c in cases} >= {(17, 13), (1, 9), (8, 1)} and any(c[9][1] > 0 for c in cases)


def test_header_has_exactly_the_two_prototypes():
    protos = L.parse_header()
    assert sorted(n for n in protos if "components" in n) == sorted(NAMES)
    assert all(protos[n][0] is ctypes.c_int for n in NAMES)
    assert [n for _, n in protos["mi355_components_ws_ints"][1]] == ["B", "H", "W"]
    assert [n for _, n in protos["mi355_components"][1]] == ["src", "B", "H", "W", "is_logit", "thr", "connectivity", "fill_holes", "min_area",
                                                            "keep_largest", "max_report", "ws", "ws_ints", "mask_out", "labels_out", "out_i",
                                                            "out_c", "s"]
    src = open(L.HEADER).read()
    assert src.count("\nint mi355_components_ws_ints(") == 1 and src.count("\nint mi355_components(") == 1      # column 0: the plan table
    assert os.path.exists(L.SO_PATH), "libmi355conv.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    dll = ctypes.CDLL(L.SO_PATH)
    arity = L.lib.raw("mi355_plan_arity")
    for name, n in zip(NAMES, (3, 18)):
        assert hasattr(dll, name) and arity(name.encode()) == n, name


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    ws_ints, run = lib.raw("mi355_components_ws_ints"), lib.raw("mi355_components")
    for bad in ((1, 0, 5), (1, 1025, 8), (1, 8, 1025), (1, 5, 0), (0, 8, 8), (-1, 8, 8), (65536, 8, 8)):
        assert ws_ints(*bad) == -1 and b"1024" in err(), (bad, err())
    assert ws_ints(60000, 1024, 1024) == -1 and b"2^31" in err()          # the count would not fit its return type
    for B, H, W in ((1, 1, 1), (3, 17, 13), (8, 256, 256), (1, 1024, 1024)):
        assert B * H * W <= ws_ints(B, H, W) <= 8 * B * H * W + 256, (B, H, W)
    need = ws_ints(2, 8, 8)
    buf = (ctypes.c_double * 4096)()                    # host memory: never dereferenced, the checks come first
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    ok = dict(src=p, B=2, H=8, W=8, is_logit=0, thr=0.5, connectivity=8, fill_holes=0, min_area=0, keep_largest=0, max_report=8, ws=p,
              ws_ints=need, mask_out=p, labels_out=p, out_i=p, out_c=p)

    def call(**kw):
        a = dict(ok, **kw)
        return run(*[a[k] for k in ok], None)

    for bad, word in (({"src": None}, b"null"), ({"ws": None}, b"null"), ({"mask_out": None}, b"null"), ({"out_i": None}, b"null"),
                      ({"out_c": None}, b"null"), ({"B": 0}, b"B"), ({"H": 0}, b"1024"), ({"H": 1025}, b"1024"), ({"W": 1025}, b"1024"),
                      ({"connectivity": 6}, b"connectivity"), ({"connectivity": 0}, b"connectivity"), ({"fill_holes": 1}, b"fill_holes"),
                      ({"max_report": 17}, b"max_report"), ({"max_report": -1}, b"max_report"), ({"min_area": -1}, b"negative"),
                      ({"keep_largest": -1}, b"negative"), ({"ws_ints": need - 1}, b"too short"), ({"ws_ints": 0}, b"too short"),
                      ({"ws": ctypes.c_void_p(base + 4)}, b"aligned")):
        assert call(**bad) == -1, bad
        assert word in err(), (bad, err())


def test_python_argument_errors_on_cpu_tensors():
    import torch
    from utils import postprocess as pp
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(pp.label_components_batch) == [("pred", E), ("is_logit", False), ("threshold", 0.5), ("connectivity", 8), ("fill_holes", 0),
                                              ("min_area", 0), ("keep_largest", 0), ("max_report", 8)]
    assert sig(pp.MaskPostprocess.__init__)[1:] == [("connectivity", 8), ("fill_holes", 0), ("min_area", 0), ("keep_largest", 0),
                                                    ("max_report", 8)]
    with pytest.raises(ValueError, match="one-channel"):
        pp.label_components_batch(torch.zeros(2, 2, 8, 8))
    with pytest.raises(ValueError, match="connectivity"):
        pp.label_components_batch(torch.zeros(2, 8, 8), connectivity=6)
    with pytest.raises(ValueError, match="connectivity"):
        pp.MaskPostprocess(connectivity=6)
    with pytest.raises(ValueError, match="fill_holes"):
        pp.clean_masks(torch.zeros(2, 8, 8), fill_holes=3)
    with pytest.raises(ValueError, match="max_report"):
        pp.label_components_batch(torch.zeros(2, 8, 8), max_report=17)
    with pytest.raises(RuntimeError, match="1024"):
        pp.label_components_batch(torch.zeros(1, 1, 1025, 8))
    with pytest.raises(RuntimeError, match="1024"):
        pp.MaskPostprocess()(torch.zeros(1, 8, 1025))


def test_joint_pipeline_constructor_keeps_todays_arguments():
    import torch
    from utils.pipeline import CLASSES, JointPipeline
    sig = [(p.name, p.default) for p in inspect.signature(JointPipeline.__init__).parameters.values()]
    E = inspect.Parameter.empty
    assert sig == [("self", E), ("classification_model", E), ("segmentation_model", E), ("device", "cuda"), ("classes", CLASSES),
                   ("positive", "COVID"), ("bucket", 4), ("postprocess", None)]
    p = JointPipeline(torch.nn.Identity(), None, "cpu", ["a", "b"], "b", 2)
    assert p.bucket == 2 and p.keep == 1 and p.postprocess is None
