"""-m gpu: the elastic deformation on the device (csrc/elastic.hip, utils/elastic.py, the ``elastic=`` option of
utils/gpu_transforms.py) against the numpy restatement tests/elastic_ref.py, which tests/test_elastic_cpu.py pins to scipy.ndimage.

Blur: |gpu - blur64| <= 2 (2R + 3) 2^-24 max|src| per element, blur64 being the float64 correlation with the UNROUNDED float64 taps.
Where the bound comes from: positive taps that sum to 1; per pass one fp32 FMA chain of 2R + 1 terms (error <= (2R + 1) 2^-24 of
sum |t| |x| <= max|x|) plus the taps' rounding to fp32 (<= 2^-24 max|x|), < (2R + 3) 2^-24 max|x|; the second pass sees values
bounded by the same maximum and passes the first pass's error on with weights that sum to 1: twice that.  For a tap vector that
is not a probability vector (the asymmetric one) both passes scale with its l1 norm: the bound times max(1, sum |t|)^2.
Warp: byte-identical to the float32 restatement, and with alpha = 0 to mi355_warp_u8."""
import os

import numpy as np
import pytest
import torch

import elastic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = 12345.0


def _guarded(n):
    """a NaN-filled buffer of n floats between two guard bands -> (whole, view)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    whole[GUARD:GUARD + n] = float("nan")
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _gpu_blur(src, taps32, r):
    """mi355_sepblur_reflect_f32 through the ABI on src [P, H, W] (numpy float32), dst and tmp pre-filled with NaN between guard
    bands; asserts what holds for every call (finite, guards, two runs bit-identical) -> dst as numpy"""
    from mi355.lib import lib
    p, h, w = src.shape
    s = torch.from_numpy(np.ascontiguousarray(src)).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(taps32)).to(DEV)
    assert t.numel() == 2 * r + 1
    outs = []
    for _ in range(2):
        tmp_all, tmp = _guarded(s.numel())
        dst_all, dst = _guarded(s.numel())
        lib.mi355_sepblur_reflect_f32(s, p, h, w, t, r, tmp, dst)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tmp).all()) and bool(torch.isfinite(dst).all())
        assert _guards_intact(tmp_all) and _guards_intact(dst_all)
        outs.append(dst.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(s.cpu(), torch.from_numpy(src))                          # the source is read only
    return outs[0].cpu().numpy().reshape(p, h, w)


def _check_blur(src, taps64, r):
    got = _gpu_blur(src, taps64.astype(np.float32), r)
    ref = R.blur64(src, taps64, r)
    bound = R.blur_bound(r, float(np.abs(src).max())) * max(1.0, float(np.abs(taps64).sum())) ** 2
    err = float(np.abs(got - ref).max())
    print(f"blur {src.shape} R={r}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (src.shape, r, err, bound)
    return got


# (planes, H, W, sigma): R = int(4 sigma + 0.5)
BLUR_SHAPES = [(1, 1, 1, 0.1), (1, 1, 9, 1.0), (1, 9, 1, 1.0), (2, 5, 7, 3.0), (1, 17, 33, 64.0), (1, 64, 64, 1.0), (1, 40, 56, 20.0),
               (1, 3, 63, 2.5), (1, 3, 64, 2.5), (1, 3, 65, 2.5), (1, 3, 127, 2.5), (1, 3, 129, 2.5), (1, 63, 3, 2.5), (1, 65, 3, 2.5),
               (1, 9, 257, 2.5),                      # past the W pass's 256-column tile and its 8-row tile
               (4, 256, 256, 20.5)]


@pytest.mark.parametrize("p,h,w,sigma", BLUR_SHAPES)
def test_blur_within_bound_of_float64(p, h, w, sigma):
    taps, r = R.gaussian_taps64(sigma)
    src = R.noise(p, h, w, 100 + h + w).reshape(2 * p, h, w)[:p]
    _check_blur(src, taps, r)


@pytest.mark.parametrize("r", [7, 8, 95, 96, 127, 128, 200, 1024])
def test_blur_radii_around_the_tap_chunks(r):
    """16-tap groups and their tail (15 = 0 groups + 15, 17 = 1 + 1), the H pass's 192-tap chunk (191 / 193 taps), the W pass's
    256-tap chunk (255 / 257), several chunks in both (401), and the cap (2049 taps on a 3 x 5 plane)"""
    taps, rr = R.gaussian_taps64(r / 4.0)
    assert rr == r
    h, w = (3, 5) if r == 1024 else (70, 300)
    _check_blur(R.noise(1, h, w, r)[0, :1], taps, r)


def test_blur_asymmetric_taps_constant_plane_and_fixture():
    nz = R.noise(1, 23, 70, 5)[0]
    got = _check_blur(nz, R.ASYM_TAPS.astype(np.float64), 3)
    flipped = R.blur64(nz, R.ASYM_TAPS[::-1].astype(np.float64), 3)
    assert np.abs(got - flipped).max() > 1e-2                                     # correlation, not convolution
    # a constant plane stays constant within the bound, at a radius far past the extents
    taps, r = R.gaussian_taps64(20.5)
    const = np.full((1, 19, 70), 0.8125, dtype=np.float32)
    assert np.abs(_check_blur(const, taps, r) - 0.8125).max() <= R.blur_bound(r, 0.8125)
    for s in R.load_fixture():
        got = _gpu_blur(s["noise"], s["taps"], int(s["radius"]))
        l1 = max(1.0, float(np.abs(s["taps"].astype(np.float64)).sum()))
        assert np.abs(got - s["field"]).max() <= R.blur_bound(int(s["radius"]), float(np.abs(s["noise"]).max())) * l1 ** 2, s["name"]


# ---- warp ----------------------------------------------------------------------------------------------------------------------
def _warp_u8(img, m, h, w, nearest, reflect):
    from mi355.lib import lib
    n, hs, ws, c = img.shape
    out = torch.empty(n, h, w, c, dtype=torch.uint8, device=DEV)
    lib.mi355_warp_u8(img, n, hs, ws, c, m, out, h, w, int(nearest), int(reflect))
    return out


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("reflect", [False, True])
def test_alpha_zero_is_warp_u8_byte_for_byte(c, nearest, reflect):
    from utils.elastic import elastic_warp
    n, hs, ws, h, w = 3, 37, 53, 29, 61
    img = torch.from_numpy(np.stack([R.image(hs, ws, c, 60 + i) for i in range(n)])).to(DEV)
    mats = torch.tensor([R.ROT, (1.3, 0.0, -4.5, 0.0, 1.25, 3.25), (0.87, 0.0, 0.4, 0.0, 1.27, 0.1)], dtype=torch.float32, device=DEV)
    field = torch.from_numpy(R.noise(n, h, w, 9) * 50).to(DEV)                 # large and never used: alpha = 0
    want = _warp_u8(img, mats, h, w, nearest, reflect)
    got = elastic_warp(img, field, 0.0, mats, nearest=nearest, reflect=reflect)
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.equal(elastic_warp(img, field, 0.05, mats, nearest=nearest, reflect=reflect), want)     # and the field is read


# (N, H, W, C, sigma, alpha): the field is the GPU's own blur of seeded noise, downloaded for the restatement
WARP_SHAPES = [(1, 1, 1, 3, 0.5, 2.0), (1, 2, 3, 3, 0.6, 3.0), (1, 5, 7, 3, 3.0, 400.0), (1, 37, 53, 3, 4.0, 74.0), (1, 64, 64, 3, 5.12, 128.0),
               (2, 256, 256, 3, 20.48, 512.0)]


@pytest.mark.parametrize("n,h,w,c,sigma,alpha", WARP_SHAPES)
def test_warp_with_the_gpus_own_field_is_the_float32_restatement(n, h, w, c, sigma, alpha):
    from utils.elastic import elastic_field, elastic_warp
    field = elastic_field(torch.from_numpy(R.noise(n, h, w, 21)).to(DEV), sigma)
    fh = field.cpu().numpy()
    if (h, w) == (5, 7):
        assert np.abs(alpha * fh).max() > 3 * 7                                  # several extents outside the source
    imgs = np.stack([R.image(h, w, c, 70 + i) for i in range(n)])
    msks = np.stack([R.mask(h, w) for _ in range(n)])
    mats = [R.ROT if i % 2 == 0 else (1.02, -0.05, 1.5, 0.05, 0.97, -2.25) for i in range(n)]
    for reflect in (True, False):
        got = elastic_warp(torch.from_numpy(imgs).to(DEV), field, alpha, mats, reflect=reflect).cpu().numpy()
        gotm = elastic_warp(torch.from_numpy(msks).to(DEV), field, alpha, mats, nearest=True, reflect=reflect).cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], R.warp_field_ref(imgs[i], mats[i], fh[i], alpha, False, reflect)), (i, reflect)
            assert np.array_equal(gotm[i], R.warp_field_ref(msks[i], mats[i], fh[i], alpha, True, reflect)), (i, reflect)
    ident = elastic_warp(torch.from_numpy(imgs).to(DEV), field, alpha).cpu().numpy()       # mats=None: the identity map
    assert np.array_equal(ident[0], R.warp_field_ref(imgs[0], R.IDENTITY, fh[0], alpha))


def test_per_sample_alphas_zero_and_non_zero_in_one_batch():
    from utils.elastic import elastic_field, elastic_warp
    n, h, w = 4, 40, 56
    alphas = [0.0, 80.0, 0.0, 33.5]
    field = elastic_field(torch.from_numpy(R.noise(n, h, w, 31)).to(DEV), 4.0)
    fh = field.cpu().numpy()
    imgs = np.stack([R.image(h, w, 3, 80 + i) for i in range(n)])
    mats = [R.ROT] * n
    g = torch.from_numpy(imgs).to(DEV)
    got = elastic_warp(g, field, alphas, mats)
    plain = _warp_u8(g, torch.tensor(mats, dtype=torch.float32, device=DEV), h, w, False, True)
    for i, a in enumerate(alphas):
        assert np.array_equal(got[i].cpu().numpy(), R.warp_field_ref(imgs[i], mats[i], fh[i], a)), i
        assert torch.equal(got[i], plain[i]) == (a == 0.0), i


def test_warp_fixture_cases():
    from utils.elastic import elastic_warp
    for s in R.load_fixture():
        field = torch.from_numpy(s["field"].astype(np.float32))[None].to(DEV)
        img = torch.from_numpy(s["image"])[None].to(DEV)
        got = elastic_warp(img, field, float(s["alpha"]), [s["m"].tolist()], nearest=bool(s["nearest"]), reflect=bool(s["reflect"]))
        assert np.array_equal(got[0].cpu().numpy(), s["warped"]), s["name"]


# ---- transforms and train() ------------------------------------------------------------------------------------------------------
def _batch(n, hs, ws, seed):
    imgs = np.stack([R.image(hs, ws, 3, seed + i) for i in range(n)])
    msks = np.stack([R.mask(hs, ws) for _ in range(n)])
    return torch.from_numpy(imgs), torch.from_numpy(msks)


def test_elastic_none_and_p_zero_are_todays_batches():
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    imgs, msks = _batch(5, 90, 75, 3)
    x0, y0 = SegBatchTransform(64, train=True, seed=4, device=DEV)(imgs, msks)
    for el in (None, (128.0, 5.12, 0.0)):
        x, y = SegBatchTransform(64, train=True, seed=4, device=DEV, elastic=el)(imgs, msks)
        assert torch.equal(x, x0) and torch.equal(y, y0), el
    x1, y1 = SegBatchTransform(64, train=True, seed=4, device=DEV, elastic=(128.0, 5.12, 1.0))(imgs, msks)
    assert not torch.equal(x1, x0) and not torch.equal(y1, y0)                      # and p = 1 does deform
    # the validation transform ignores the option
    v0 = SegBatchTransform(64, train=False, device=DEV)(imgs, msks)
    v1 = SegBatchTransform(64, train=False, device=DEV, elastic=(128.0, 5.12, 1.0))(imgs, msks)
    assert torch.equal(v0[0], v1[0]) and torch.equal(v0[1], v1[1])
    c0 = ClsBatchTransform(64, train=True, seed=4, device=DEV)(imgs)
    assert torch.equal(ClsBatchTransform(64, train=True, seed=4, device=DEV, elastic=None)(imgs), c0)
    assert torch.equal(ClsBatchTransform(64, train=True, seed=4, device=DEV, elastic=(128.0, 5.12, 0.0))(imgs), c0)


def test_fixed_params_reproduce_the_restatement():
    """64 x 64 sources: A.Resize is then the identity, and the batch is the restatement's warp of the sources, normalised"""
    from mi355.lib import lib
    from utils.elastic import elastic_field
    from utils.gpu_transforms import SegBatchTransform, shift_scale_rotate_matrix
    n, s, sigma = 4, 64, 5.12
    imgs, msks = _batch(n, s, s, 9)
    mats = [shift_scale_rotate_matrix(s, s, a, sc, dx, dy, f) for a, sc, dx, dy, f in
            ((12.5, 1.04, 0.03, -0.05, True), (-15.0, 0.95, -0.05, 0.05, False), (0.0, 1.0, 0.0, 0.0, False), (7.0, 1.0, 0.02, 0.0, True))]
    bcs = [[1.0, 0.0]] * n
    noise = torch.from_numpy(R.noise(n, s, s, 13))
    alphas = [128.0, 0.0, 64.0, 128.0]
    t = SegBatchTransform(s, train=True, seed=1, device=DEV, elastic=(128.0, sigma, 0.5))
    x, y = t(imgs, msks, params=(mats, bcs, (noise, alphas)))
    fh = elastic_field(noise.to(DEV), sigma).cpu().numpy()
    m32 = np.asarray(mats, dtype=np.float32)
    want_img = np.stack([R.warp_field_ref(imgs[i].numpy(), m32[i], fh[i], alphas[i], False, True) for i in range(n)])
    want_msk = np.stack([R.warp_field_ref(msks[i].numpy(), m32[i], fh[i], alphas[i], True, True) for i in range(n)])
    wx = torch.empty(n, 3, s, s, dtype=torch.float32, device=DEV)
    lib.mi355_normalize_u8(torch.from_numpy(want_img).to(DEV), n, s, s, 3, None, t.mean, t.std, wx)
    assert torch.equal(x, wx)
    assert np.array_equal(y.cpu().numpy()[:, 0], (want_msk == 255).astype(np.float32))
    assert set(np.unique(y.cpu().numpy())) <= {0.0, 1.0}
    with pytest.raises(ValueError, match="elastic=None"):
        SegBatchTransform(s, train=True, device=DEV)(imgs, msks, params=(mats, bcs, (noise, alphas)))


def test_same_seed_same_batches_masks_binary_and_cls_with_padding():
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    imgs, msks = _batch(6, 90, 75, 5)
    el = (128.0, 5.12, 0.5)
    a, b = (SegBatchTransform(64, train=True, seed=9, device=DEV, elastic=el) for _ in range(2))
    for _ in range(2):                                                                  # two batches: the generators advance alike
        (xa, ya), (xb, yb) = a(imgs, msks), b(imgs, msks)
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert tuple(xa.shape) == (6, 3, 64, 64) and tuple(ya.shape) == (6, 1, 64, 64) and bool(torch.isfinite(xa).all())
        assert set(np.unique(ya.cpu().numpy())) <= {0.0, 1.0}
    xc, _ = SegBatchTransform(64, train=True, seed=10, device=DEV, elastic=el)(imgs, msks)
    assert not torch.equal(xc, xb)
    # 90 x 75 -> LongestMaxSize 64 x 53 -> padded to 64 x 64
    ca = ClsBatchTransform(64, train=True, seed=9, device=DEV, elastic=(128.0, 5.12, 1.0))(imgs)
    cb = ClsBatchTransform(64, train=True, seed=9, device=DEV, elastic=(128.0, 5.12, 1.0))(imgs)
    plain = ClsBatchTransform(64, train=True, seed=9, device=DEV)(imgs)
    assert tuple(ca.shape) == (6, 3, 64, 64) and bool(torch.isfinite(ca).all()) and torch.equal(ca, cb) and not torch.equal(ca, plain)


def test_train_runs_from_png_files_with_elastic_on(tmp_path, capsys):
    """tests/test_gpu_transforms.py::test_train_runs_from_png_files_end_to_end with the elastic stage in the train transform"""
    pytest.importorskip("PIL.Image")
    from test_dataset_cpu import make_tree
    from utils.dataset import GpuBatchLoader, SegmentationDataset
    from utils.gpu_transforms import SegBatchTransform
    from utils.helpers import get_seg_model, train
    root = str(tmp_path / "dataset")
    make_tree(root, n=13)
    ds_tr = SegmentationDataset(root, SegBatchTransform(64, train=True, device=DEV, elastic=(128.0, 5.12, 0.5)), "train")
    ds_va = SegmentationDataset(root, SegBatchTransform(64, train=False, device=DEV), "train")
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(0)).tolist()
    tr = GpuBatchLoader(ds_tr, 4, shuffle=True, device=DEV, indices=perm[:9])
    va = GpuBatchLoader(ds_va, 4, shuffle=False, device=DEV, indices=perm[9:])
    best = train(get_seg_model("attentionunet"), tr, va, torch.device(DEV), 2, 1e-3, "AttentionUNet", str(tmp_path / "w"), seg=True)
    out = capsys.readouterr().out
    assert np.isfinite(best) and "Ep2" in out and os.path.exists(tmp_path / "w" / "AttentionUNet_best_loss.pt")
