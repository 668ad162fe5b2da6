"""CPU: CLAHE below the GPU — the numpy restatement (tests/clahe_ref.py) pinned to facts that do not come from it (plain histogram
equalisation written inline, constant images derived by hand, the closed forms of every redistribution branch, the padding quirk),
the substance of the inputs the GPU tests use, utils/clahe.py's argument checks, the trainer's flags, and the C ABI's argument
checks, which run before anything touches the device."""
import ctypes
import os

import numpy as np
import pytest

import clahe_ref as R
from mi355 import lib as L


# ---- the restatement against facts from outside it --------------------------------------------------------------------------------
def test_grid_one_without_clipping_is_plain_histogram_equalisation():
    p = np.random.default_rng(1).integers(0, 256, (37, 53), dtype=np.uint8)
    area = 37 * 53
    lut = np.rint(np.cumsum(np.bincount(p.ravel(), minlength=256)).astype(np.float32) * (np.float32(255) / np.float32(area)))
    want = lut.astype(np.uint8)[p]
    assert np.array_equal(R.clahe_ref(p[None], clip=0.0, grid=(1, 1))[0], want)
    luts, th, tw = R.clahe_luts_ref(p, 1, 1, 0.0)
    assert (th, tw) == (37, 53) and np.array_equal(luts[0, 0], lut.astype(np.uint8))


@pytest.mark.parametrize("value,want", [(0, 8), (7, 12), (255, 255)])
def test_constant_images_by_hand(value, want):
    """64 x 64, grid 8, clip 4: tiles of 64 pixels, lim = max(int(4 * 64 / 256), 1) = 1.  The one occupied bin keeps 1, excess 63:
    63 // 256 = 0 to every bin, residual 63, step 256 // 63 = 4: bins 0, 4, ..., 248 get one more.
      input 0:   lut[0] = rint((1 + 1) * 255 / 64) = rint(7.97) = 8
      input 7:   bins 0 and 4 hold 1 each, bin 7 holds 1: lut[7] = rint(3 * 255 / 64) = rint(11.95) = 12
      input 255: the whole histogram lies at or below 255: lut[255] = rint(64 * 255 / 64) = 255
    Every tile has the same LUT, so the blend returns that value everywhere."""
    img = np.full((1, 64, 64), value, dtype=np.uint8)
    out = R.clahe_ref(img, clip=4.0, grid=8)
    assert out.shape == img.shape and (out == want).all(), np.unique(out)


@pytest.mark.parametrize("w", R.CONST_WIDTHS)
def test_every_redistribution_branch_against_its_closed_form(w):
    """constant 1 x W planes, grid (1, 1), clip 0.5: lim = 1, excess W - 1.  W = 257, 258, 259, 386, 512: residual 0, 1 (step 256),
    2 (step 128), 129 (step 1) and 255 (step 1, stops after 255 bins)"""
    assert (w - 1) % 256 == {257: 0, 258: 1, 259: 2, 386: 129, 512: 255}[w] and R.clip_limit(0.5, w) == 1
    h = np.ones(256, dtype=np.int64)                     # 1 from excess // 256 (bin 77: its own clipped 1 comes below)
    h[77] += 1
    for b in {257: [], 258: [0], 259: [0, 128], 386: range(0, 129), 512: range(0, 255)}[w]:
        h[b] += 1
    assert h.sum() == w                                  # redistribution loses no pixel in these cases
    want = np.rint(np.cumsum(h).astype(np.float32) * (np.float32(255) / np.float32(w))).astype(np.uint8)
    luts, th, tw = R.clahe_luts_ref(R.const_plane(w), 1, 1, 0.5)
    assert (th, tw) == (1, w) and np.array_equal(luts[0, 0], want)
    assert np.array_equal(R.const_lut_closed_form(w), want)


def test_padding_quirk_and_mirror():
    assert R.tile_geometry(33, 64, 8, 8) == (7, 8, 5, 9)          # 64 divides by 8 and still gets a full 8 columns
    assert R.tile_geometry(17, 23, 4, 4) == (3, 1, 5, 6)
    assert R.tile_geometry(64, 64, 8, 8) == (0, 0, 8, 8)
    assert R.tile_geometry(9, 9, 8, 8) == (7, 7, 2, 2)
    from utils import clahe as C
    for h, w, gy, gx in ((33, 64, 8, 8), (17, 23, 4, 4), (64, 64, 8, 8), (9, 9, 8, 8), (8, 600, 1, 2), (64, 40, 1, 3)):
        assert C.tile_geometry(h, w, gy, gx) == R.tile_geometry(h, w, gy, gx)[2:]
    p = np.arange(12, dtype=np.uint8).reshape(3, 4)
    q = R.pad_reflect101(p, 2, 3)
    assert q.shape == (5, 7) and np.array_equal(q[:3, :4], p)
    assert q[0].tolist() == [0, 1, 2, 3, 2, 1, 0] and q[:, 0].tolist() == [0, 4, 8, 4, 0]      # d c b a | b c d: the edge is not repeated
    with pytest.raises(ValueError, match="padding"):
        R.tile_geometry(3, 64, 8, 8)


def _inputs_with_clipping():
    for n, c, h, w, gy, gx, clip in R.LUT_CASES:
        if clip > 0:
            yield f"{(n, c, h, w, gy, gx, clip)}", R.case_input(n, c, h, w), clip, (gy, gx)
    for w in R.CONST_WIDTHS:
        yield f"const {w}", R.const_plane(w)[None, :, :, None], 0.5, (1, 1)


def test_luts_are_monotone_and_end_at_255():
    for name, img, clip, grid in _inputs_with_clipping():
        for cl in (clip, 0.0):
            luts = R.luts_ref(img, cl, grid).astype(np.int32)
            assert (np.diff(luts, axis=-1) >= 0).all() and (luts[..., 255] == 255).all(), (name, cl)


def test_the_gpu_tests_inputs_are_not_vacuous():
    """clipping must matter on every input the GPU tests equalise with clip > 0: at least 5 % of the output bytes differ from
    clip = 0.  (The all-255 plane cannot: lut[255] is 255 under every rule.  Its case is about the LUT, and there the bytes differ.)"""
    for name, img, clip, grid in _inputs_with_clipping():
        a, b = R.clahe_ref(img, clip, grid), R.clahe_ref(img, 0.0, grid)
        share = float((a != b).mean())
        assert share >= 0.05, (name, share)
    top = np.full((1, 32, 32, 1), 255, dtype=np.uint8)
    assert float((R.luts_ref(top, 4.0, (2, 2)) != R.luts_ref(top, 0.0, (2, 2))).mean()) >= 0.05
    assert (R.clahe_ref(top, 4.0, (2, 2)) == 255).all()


def test_xray_like_is_narrow_band():
    x = R.xray_like(2, 64, 64, 3)
    assert x.dtype == np.uint8 and x.shape == (2, 64, 64) and 50 <= x.min() and x.max() <= 150 and x.std() > 5
    assert np.array_equal(x, R.xray_like(2, 64, 64, 3)) and not np.array_equal(x[0], x[1])


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_check_clahe_validates_and_normalises():
    from utils import clahe as C
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    assert C.check_clahe(4, 8) == (4.0, (8, 8)) and C.check_clahe(0, (1, 64)) == (0.0, (1, 64)) and C.check_clahe(2.5, [3, 5]) == (2.5, (3, 5))
    for bad, word in (((-1, 8), "clip"), ((float("nan"), 8), "clip"), ((float("inf"), 8), "clip"), ((4, 0), "grid"), ((4, 65), "grid"),
                      ((4, (8, 0)), "grid"), ((4, (65, 8)), "grid"), ((4, 8.0), "grid"), ((4, (8, 8, 8)), "grid"), ((4, None), "grid")):
        for make in (lambda a: C.check_clahe(*a), lambda a: SegBatchTransform(64, device="cpu", clahe=a),
                     lambda a: ClsBatchTransform(64, train=True, device="cpu", clahe=a)):
            with pytest.raises(ValueError, match=word):
                make(bad)
    with pytest.raises(ValueError, match="clip, grid"):
        SegBatchTransform(64, device="cpu", clahe=(4.0,))
    with pytest.raises(ValueError, match="too small"):
        SegBatchTransform(30, device="cpu", clahe=(4.0, 64))              # 30 x 30 under 64 x 64: pad 34 > 29
    t = SegBatchTransform(64, device="cpu", clahe=(4, 8))
    assert t.clahe == (4.0, (8, 8)) and SegBatchTransform(64, device="cpu").clahe is None
    assert C.clip_count(4.0, 1024) == 16 and C.clip_count(0.0, 1024) == 0 and C.clip_count(0.01, 4) == 1 and C.clip_count(40.0, 1024) == 160
    import torch
    for f in (C.clahe, C.clahe_luts):
        with pytest.raises(ValueError, match="device tensor"):
            f(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


def test_clahe_consumes_no_random_draw():
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    for T in (SegBatchTransform, ClsBatchTransform):
        plain = T(64, train=True, seed=11, device="cpu")
        eq = T(64, train=True, seed=11, device="cpu", clahe=(4.0, 8))
        for n in (5, 3):
            assert eq.draw(n) == plain.draw(n)


def test_trainer_flags_keep_todays_transforms_by_default():
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.clahe_clip, d.clahe_grid) == (0.0, 8) and trainer.clahe_arg(d) is None
    assert trainer.clahe_arg(ap.parse_args(["--clahe-clip", "0", "--clahe-grid", "4"])) is None
    assert trainer.clahe_arg(ap.parse_args(["--clahe-clip", "4"])) == (4.0, (8, 8))
    assert trainer.clahe_arg(ap.parse_args(["--clahe-clip", "2.5", "--clahe-grid", "16", "--size", "64"])) == (2.5, (16, 16))
    for bad in (["--clahe-clip", "-1"], ["--clahe-clip", "4", "--clahe-grid", "0"], ["--clahe-clip", "4", "--clahe-grid", "65"],
                ["--clahe-clip", "4", "--clahe-grid", "64", "--size", "30"]):
        with pytest.raises(ValueError):
            trainer.clahe_arg(ap.parse_args(bad))
    import inspect
    from utils.pipeline import JointPipeline
    from utils.tester import test_all_models
    assert inspect.signature(test_all_models).parameters["clahe"].default is None
    import torch
    pipe = JointPipeline(torch.nn.Identity(), None, "cpu")
    assert pipe.clahe is None
    pipe.clahe = (4, 8)
    assert pipe.clahe == (4.0, (8, 8))
    for bad in ((-1, 8), (4, 65), (4.0,)):
        with pytest.raises(ValueError):
            pipe.clahe = bad
    pipe.clahe = None
    assert pipe.clahe is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = {"mi355_clahe_lut_u8": ["src", "N", "H", "W", "C", "gy", "gx", "clip_count", "luts", "s"],
         "mi355_clahe_apply_u8": ["src", "N", "H", "W", "C", "gy", "gx", "luts", "dst", "s"]}


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


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.lib
    err = lib.raw("mi355_last_error")
    bufs = [(ctypes.c_double * 64)() for _ in range(3)]                   # host memory: never dereferenced, the checks come first
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    lut = lib.raw("mi355_clahe_lut_u8")
    ok = dict(src=p[0], N=1, H=16, W=16, C=3, gy=4, gx=4, clip=2, luts=p[1])

    def call(**kw):
        a = dict(ok, **kw)
        return lut(a["src"], a["N"], a["H"], a["W"], a["C"], a["gy"], a["gx"], a["clip"], a["luts"], None)

    shared = (({"N": 0}, b"positive"), ({"H": 0}, b"positive"), ({"W": -3}, b"positive"), ({"C": 2}, b"C = 2"), ({"C": 0}, b"C = 0"),
              ({"C": 4}, b"C = 4"), ({"gy": 0}, b"grid"), ({"gx": 0}, b"grid"), ({"gy": 65}, b"grid"), ({"gx": 65}, b"grid"),
              ({"gy": -1}, b"grid"), ({"H": 3, "gy": 8}, b"padding"), ({"W": 7, "gx": 16}, b"padding"),
              ({"H": 1, "W": 9, "gy": 1, "gx": 2}, b"padding"),           # W pads by 1, so H gets a full gy = 1 > H - 1 = 0
              ({"H": 1 << 28, "W": 1 << 28, "gy": 1, "gx": 1}, b"2^24"), ({"N": 1 << 20, "gy": 64, "gx": 64, "H": 64, "W": 64}, b"LUTs"))
    for bad, word in (({"src": None}, b"null pointer (src)"), ({"luts": None}, b"null pointer (luts)"), ({"luts": p[0]}, b"alias"),
                      ({"clip": -1}, b"negative")) + shared:
        assert call(**bad) == -1, bad
        assert word in err() and b"clahe_lut_u8" in err(), (bad, err())

    app = lib.raw("mi355_clahe_apply_u8")
    oka = dict(src=p[0], N=1, H=16, W=16, C=3, gy=4, gx=4, luts=p[1], dst=p[2])

    def call_a(**kw):
        a = dict(oka, **kw)
        return app(a["src"], a["N"], a["H"], a["W"], a["C"], a["gy"], a["gx"], a["luts"], a["dst"], None)

    for bad, word in (({"src": None}, b"null pointer (src)"), ({"luts": None}, b"null pointer (luts)"), ({"dst": None}, b"null pointer (dst)"),
                      ({"dst": p[0]}, b"alias"), ({"dst": p[1]}, b"alias")) + shared:
        assert call_a(**bad) == -1, bad
        assert word in err() and b"clahe_apply_u8" in err(), (bad, err())
