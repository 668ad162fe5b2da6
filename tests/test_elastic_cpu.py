"""CPU: the elastic deformation below the GPU — the numpy restatement (tests/elastic_ref.py) pinned to scipy.ndimage
(gaussian_filter, correlate1d, map_coordinates) and to its committed fixture (tests/golden/elastic.npz), the float32 evaluation of
the warp against the same formula in float64, utils/elastic.py's taps and argument checks, the transforms' and the trainer's
options, and the C ABI's argument checks, which run before anything touches the device."""
import ctypes
import os

import numpy as np
import pytest

import elastic_ref as R
from mi355 import lib as L


# ---- the restatement against scipy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sigma", [((1, 1), 0.1), ((1, 9), 1.0), ((9, 1), 1.0), ((5, 7), 3.0), ((17, 33), 64.0), ((64, 64), 1.0),
                                         ((40, 56), 20.0), ((3, 129), 2.5), ((65, 3), 2.5)])
def test_blur64_equals_scipy_gaussian_filter(shape, sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    nz = R.noise(1, *shape, 3)[0].astype(np.float64)
    taps, r = R.gaussian_taps64(sigma)
    assert r == int(4.0 * sigma + 0.5) and abs(taps.sum() - 1) < 1e-15 and (taps > 0).all()
    want = np.stack([ndi.gaussian_filter(p, sigma, mode="reflect", truncate=4.0) for p in nz])
    assert np.abs(R.blur64(nz, taps, r) - want).max() <= 1e-12


def test_blur64_with_asymmetric_taps_equals_correlate1d():
    """a flipped kernel (convolution in place of correlation) or swapped axes would show here"""
    ndi = pytest.importorskip("scipy.ndimage")
    nz = R.noise(1, 11, 6, 4)[0, 0].astype(np.float64)
    t = R.ASYM_TAPS.astype(np.float64)
    want = ndi.correlate1d(ndi.correlate1d(nz, t, axis=0, mode="reflect"), t, axis=1, mode="reflect")
    assert np.abs(R.blur64(nz, t, 3) - want).max() <= 1e-15
    flipped = ndi.correlate1d(ndi.correlate1d(nz, t[::-1], axis=0, mode="reflect"), t[::-1], axis=1, mode="reflect")
    assert np.abs(R.blur64(nz, t, 3) - flipped).max() > 1e-3
    # radius several times the extent: the reflection repeats
    t9 = np.linspace(-1, 2, 19)
    row = np.array([[1.0, -2.0, 5.0]])
    want = ndi.correlate1d(ndi.correlate1d(row, t9, axis=0, mode="reflect"), t9, axis=1, mode="reflect")
    assert np.abs(R.blur64(row, t9, 9) - want).max() <= 1e-12


@pytest.mark.parametrize("sigma", [0.1, 0.6, 1.0, 3.0, 20.0, 20.48, 64.0, 255.9])
def test_gaussian_taps_are_scipys_impulse_response(sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    from utils.elastic import gaussian_radius, gaussian_taps
    taps, r = gaussian_taps(sigma)
    assert taps.dtype == np.float32 and taps.shape == (2 * r + 1,) and r == gaussian_radius(sigma) == int(4.0 * sigma + 0.5)
    imp = np.zeros(2 * r + 1 + 2 * 8)
    imp[r + 8] = 1.0
    resp = ndi.gaussian_filter1d(imp, sigma, mode="constant", truncate=4.0)
    assert not resp[:8].any() and not resp[-8:].any()                        # scipy's support is exactly R on either side
    assert np.array_equal(taps, resp[8:-8].astype(np.float32))
    assert np.array_equal(taps, R.gaussian_taps64(sigma)[0].astype(np.float32))


@pytest.mark.parametrize("shape", [(64, 64), (256, 256), (37, 53)])
def test_warp_formula_equals_map_coordinates_and_float32_stays_within_a_grey_level(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = shape
    sigma = 0.08 * max(h, w)
    taps, r = R.gaussian_taps64(sigma)
    field = R.blur64(R.noise(1, h, w, 11)[0], taps, r).astype(np.float32)
    alpha = np.float32(2 * max(h, w))
    img, msk = R.image(h, w, 3, 5), R.mask(h, w)
    got64 = R.warp_field_ref(img, R.IDENTITY, field, alpha, dtype=np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    coords = [yy + np.float64(alpha) * field[1], xx + np.float64(alpha) * field[0]]
    assert np.abs(coords[0] - yy).max() > 1.0                                 # the field does move pixels
    for c in range(3):
        want = ndi.map_coordinates(img[..., c].astype(np.float64), coords, order=1, mode="mirror")
        assert np.array_equal(got64[..., c], np.clip(np.rint(want), 0, 255).astype(np.uint8))
    # what the kernel evaluates (float32) against the formula (float64): a value that sits on .5 may round the other way
    got32 = R.warp_field_ref(img, R.IDENTITY, field, alpha, dtype=np.float32)
    d = np.abs(got32.astype(np.int32) - got64.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() <= 5e-3, (d.max(), (d > 0).mean())
    m32, m64 = (R.warp_field_ref(msk, R.IDENTITY, field, alpha, nearest=True, dtype=t) for t in (np.float32, np.float64))
    assert np.array_equal(m32, m64) and set(np.unique(m32)) <= {0, 255}
    near = ndi.map_coordinates(msk, coords, order=0, mode="mirror")
    assert (near != m64).mean() <= 1e-3                                       # scipy rounds half to even, the kernel half up
    # alpha = 0 is the plain affine warp: with the identity map, the image itself
    assert np.array_equal(R.warp_field_ref(img, R.IDENTITY, field, 0.0), img)


def test_fixture_covers_what_it_should_and_is_reproduced():
    stored = R.load_fixture()
    cases = R.fixture_cases()
    assert 10 <= len(stored) <= 16 and os.path.getsize(R.FIXTURE) < 118948       # below tests/golden/boundary_loss.npz
    assert [c[0] for c in cases] == [s["name"] for s in stored]
    for (name, nz, taps, r, img, m, alpha, nearest, reflect), s in zip(cases, stored):
        assert np.array_equal(nz, s["noise"]) and np.array_equal(img, s["image"]) and np.array_equal(m, s["m"]), name
        assert int(s["radius"]) == r and s["taps"].dtype == np.float32 and s["field"].dtype == np.float64, name
        assert np.abs(taps - s["taps"]).max() <= 2.0 ** -24 and (bool(s["nearest"]), bool(s["reflect"])) == (nearest, reflect), name
        assert float(s["alpha"]) == float(alpha), name
        field, warped = R.make_case(s["noise"], s["taps"], r, img, m, alpha, nearest, reflect)
        assert np.abs(field - s["field"]).max() <= 1e-15, name
        assert np.array_equal(R.warp_field_ref(img, m, s["field"].astype(np.float32), alpha, nearest, reflect), s["warped"]), name
    by = {s["name"]: s for s in stored}
    assert int(by["pixel"]["radius"]) == 0 and np.array_equal(by["pixel"]["field"], by["pixel"]["noise"])
    assert int(by["5x7_far_outside"]["radius"]) == 12 and int(by["17x33_sigma64"]["radius"]) == 256
    far = by["5x7_far_outside"]
    assert np.abs(far["alpha"] * far["field"]).max() > 3 * 7                    # samples land several extents outside the source
    assert by["12x20_from_9x14"]["image"].shape[:2] != by["12x20_from_9x14"]["warped"].shape[:2]
    assert (by["asymmetric_taps_8x8"]["taps"] != by["asymmetric_taps_8x8"]["taps"][::-1]).any()
    assert set(np.unique(by["65x3_mask"]["warped"])) <= {0, 255}


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_bad_values_raise_and_name_the_argument():
    from utils import elastic as E
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    assert E.check_elastic(512, 20.48, 0.5) == (512.0, 20.48, 0.5) and E.check_elastic(0, 0.1, 0) == (0.0, 0.1, 0.0)
    for bad, word in (((-1, 20, 0.5), "alpha"), ((float("nan"), 20, 0.5), "alpha"), ((10, 0, 0.5), "sigma"), ((10, -3, 0.5), "sigma"),
                      ((10, 20, -0.1), "p must"), ((10, 20, 1.5), "p must"), ((10, 256.2, 0.5), "1024"), ((10, 1e6, 0.5), "radius")):
        for make in (lambda e: E.check_elastic(*e), lambda e: SegBatchTransform(64, train=True, device="cpu", elastic=e),
                     lambda e: ClsBatchTransform(64, train=True, device="cpu", elastic=e)):
            with pytest.raises(ValueError, match=word):
                make(bad)
    assert E.check_elastic(10, 256.1, 0.5)[1] == 256.1 and E.gaussian_radius(256.1) == 1024       # the cap itself is allowed
    with pytest.raises(ValueError, match="alpha, sigma, p"):
        SegBatchTransform(64, train=True, device="cpu", elastic=(1.0, 2.0))
    with pytest.raises(ValueError, match="sigma"):
        E.gaussian_taps(0.0)
    with pytest.raises(ValueError, match="1024"):
        E.gaussian_taps(300.0)
    import torch
    with pytest.raises(ValueError, match="device tensor"):
        E.blur_reflect(torch.zeros(1, 2, 4, 4), torch.ones(1), 0)
    with pytest.raises(ValueError, match="device tensor"):
        E.elastic_warp(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 2, 4, 4), 1.0)


def test_elastic_leaves_the_affine_draws_of_a_seed_alone():
    import torch
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    for T in (SegBatchTransform, ClsBatchTransform):
        plain = T(64, train=True, seed=11, device="cpu")
        el = T(64, train=True, seed=11, device="cpu", elastic=(128.0, 5.0, 0.5))
        assert plain.elastic is None and el.elastic == (128.0, 5.0, 0.5)
        assert T(64, train=True, seed=11, device="cpu", elastic=None).draw(5) == plain.draw(5)
        plain = T(64, train=True, seed=11, device="cpu")
        for n in (5, 3):
            want = plain.draw(n)
            noise, alphas = el.draw_elastic(n)                                 # interleaved: the elastic draws use generators of their own
            assert el.draw(n) == want
            assert tuple(noise.shape) == (n, 2, 64, 64) and noise.dtype == torch.float32 and float(noise.abs().max()) <= 1.0
            assert len(alphas) == n and set(alphas) <= {0.0, 128.0}
    a = SegBatchTransform(64, train=True, seed=3, device="cpu", elastic=(9.0, 5.0, 0.5))
    b = SegBatchTransform(64, train=True, seed=3, device="cpu", elastic=(9.0, 5.0, 0.5))
    (na, aa), (nb, ab) = a.draw_elastic(16), b.draw_elastic(16)
    assert torch.equal(na, nb) and aa == ab and 0.0 in aa and 9.0 in aa           # same seed, same draw; p = 0.5 picks some of 16
    assert set(SegBatchTransform(64, train=True, device="cpu", elastic=(9.0, 5.0, 0.0)).draw_elastic(8)[1]) == {0.0}
    assert set(SegBatchTransform(64, train=True, device="cpu", elastic=(9.0, 5.0, 1.0)).draw_elastic(8)[1]) == {9.0}


def test_trainer_flags_keep_todays_transforms_by_default():
    from utils import trainer
    ap = trainer.build_parser()
    d = ap.parse_args([])
    assert (d.elastic_alpha, d.elastic_sigma, d.elastic_p) == (0.0, None, 0.5)
    assert trainer.elastic_arg(d) is None
    assert trainer.elastic_arg(ap.parse_args(["--elastic-alpha", "0", "--elastic-sigma", "7"])) is None
    assert trainer.elastic_arg(ap.parse_args(["--elastic-alpha", "512"])) == (512.0, 0.08 * 256, 0.5)
    assert trainer.elastic_arg(ap.parse_args(["--elastic-alpha", "128", "--size", "64"])) == (128.0, 0.08 * 64, 0.5)
    assert trainer.elastic_arg(ap.parse_args(["--elastic-alpha", "300", "--elastic-sigma", "12.5", "--elastic-p", "1"])) == (300.0, 12.5, 1.0)
    for bad in (["--elastic-alpha", "-1"], ["--elastic-alpha", "10", "--elastic-sigma", "0"], ["--elastic-alpha", "10", "--elastic-p", "2"],
                ["--elastic-alpha", "10", "--elastic-sigma", "400"]):
        with pytest.raises(ValueError):
            trainer.elastic_arg(ap.parse_args(bad))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NAMES = {"mi355_sepblur_reflect_f32": ["src", "planes", "H", "W", "taps", "radius", "tmp", "dst", "s"],
         "mi355_warp_field_u8": ["src", "N", "Hs", "Ws", "C", "m", "field", "alpha", "dst", "H", "W", "nearest", "reflect", "s"]}


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
    bufs = [(ctypes.c_double * 64)() for _ in range(6)]                   # host memory: never dereferenced, the checks come first
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    blur = lib.raw("mi355_sepblur_reflect_f32")
    ok = dict(src=p[0], planes=2, H=4, W=4, taps=p[1], radius=3, tmp=p[2], dst=p[3])

    def call(**kw):
        a = dict(ok, **kw)
        return blur(a["src"], a["planes"], a["H"], a["W"], a["taps"], a["radius"], a["tmp"], a["dst"], None)

    for bad, word in (({"src": None}, b"null pointer (src)"), ({"taps": None}, b"null pointer (taps)"), ({"tmp": None}, b"null pointer (tmp)"),
                      ({"dst": None}, b"null pointer (dst)"), ({"planes": 0}, b"positive"), ({"planes": -2}, b"positive"),
                      ({"H": 0}, b"positive"), ({"W": 0}, b"positive"), ({"W": -5}, b"positive"), ({"radius": -1}, b"radius -1"),
                      ({"radius": 1025}, b"1024"), ({"radius": 1 << 30}, b"1024"), ({"tmp": p[0]}, b"alias"), ({"dst": p[0]}, b"alias"),
                      ({"dst": p[2]}, b"alias")):
        assert call(**bad) == -1, bad
        assert word in err() and b"sepblur_reflect_f32" in err(), (bad, err())

    warp = lib.raw("mi355_warp_field_u8")
    okw = dict(src=p[0], N=1, Hs=4, Ws=4, C=3, m=p[1], field=p[2], alpha=p[3], dst=p[4], H=4, W=4, nearest=0, reflect=1)

    def call_w(**kw):
        a = dict(okw, **kw)
        return warp(a["src"], a["N"], a["Hs"], a["Ws"], a["C"], a["m"], a["field"], a["alpha"], a["dst"], a["H"], a["W"], a["nearest"],
                    a["reflect"], None)

    for bad, word in (({"src": None}, b"null pointer (src)"), ({"m": None}, b"null pointer (m)"), ({"field": None}, b"null pointer (field)"),
                      ({"alpha": None}, b"null pointer (alpha)"), ({"dst": None}, b"null pointer (dst)"), ({"N": 0}, b"positive"),
                      ({"Hs": 0}, b"positive"), ({"Ws": -1}, b"positive"), ({"H": 0}, b"positive"), ({"W": 0}, b"positive"),
                      ({"C": 0}, b"C = 0"), ({"C": 5}, b"C = 5"), ({"dst": p[0]}, b"alias")):
        assert call_w(**bad) == -1, bad
        assert word in err() and b"warp_field_u8" in err(), (bad, err())
