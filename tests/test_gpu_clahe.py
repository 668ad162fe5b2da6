"""-m gpu: CLAHE on the device (csrc/clahe.hip, utils/clahe.py, the ``clahe=`` option of utils/gpu_transforms.py, utils/tester.py and
utils/pipeline.py) against the numpy restatement tests/clahe_ref.py, which tests/test_clahe_cpu.py pins to hand-derived facts.

Every comparison is byte-exact: the LUTs are integer arithmetic up to one fp32 multiply, the interpolation is fp32 with every
operation rounded on its own, and numpy's float32 does the same.  Every call through the ABI writes into buffers pre-filled with a
sentinel between guard bands and is checked for intact guards, an unchanged source and two bit-identical runs."""
import functools
import os

import numpy as np
import pytest
import torch

import clahe_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A


def _guarded(n, shift=0):
    """n sentinel bytes between two guard bands (``shift``: the view starts that many bytes off a 4-byte boundary) -> (whole, view)"""
    whole = torch.full((n + 2 * GUARD + shift,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    whole[GUARD + shift:GUARD + shift + n] = SENTINEL
    return whole, whole[GUARD + shift:GUARD + shift + n]


def _guards_intact(whole, n, shift=0):
    return bool((whole[:GUARD + shift] == GUARD_BYTE).all()) and bool((whole[GUARD + shift + n:] == GUARD_BYTE).all())


def _gpu_luts(img, gy, gx, lim):
    """mi355_clahe_lut_u8 through the ABI on img [N, H, W, C] (numpy uint8) -> uint8 [N, C, gy, gx, 256] as numpy"""
    from mi355.lib import lib
    n, h, w, c = img.shape
    s = torch.from_numpy(np.ascontiguousarray(img)).to(DEV)
    size = n * c * gy * gx * 256
    outs = []
    for _ in range(2):
        whole, luts = _guarded(size)
        lib.mi355_clahe_lut_u8(s, n, h, w, c, gy, gx, lim, luts)
        torch.cuda.synchronize()
        assert _guards_intact(whole, size)
        outs.append(luts.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(s.cpu(), torch.from_numpy(img))                              # the source is read only
    return outs[0].cpu().numpy().reshape(n, c, gy, gx, 256)


def _gpu_apply(img, luts, shift=0):
    """mi355_clahe_apply_u8 through the ABI on img [N, H, W, C] and luts [N, C, gy, gx, 256] (numpy uint8) -> numpy like img"""
    from mi355.lib import lib
    n, h, w, c = img.shape
    gy, gx = luts.shape[2:4]
    src_whole, s = _guarded(img.size, shift)
    s.copy_(torch.from_numpy(np.ascontiguousarray(img)).reshape(-1))
    l = torch.from_numpy(np.ascontiguousarray(luts)).to(DEV)
    outs = []
    for _ in range(2):
        whole, dst = _guarded(img.size, shift)
        lib.mi355_clahe_apply_u8(s, n, h, w, c, gy, gx, l, dst)
        torch.cuda.synchronize()
        assert _guards_intact(whole, img.size, shift)
        outs.append(dst.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(s.cpu(), torch.from_numpy(img).reshape(-1)) and _guards_intact(src_whole, img.size, shift)
    assert torch.equal(l.cpu(), torch.from_numpy(luts))
    return outs[0].cpu().numpy().reshape(img.shape)


@functools.lru_cache(maxsize=None)
def _case(n, c, h, w, gy, gx, clip):
    """-> (input, reference LUTs, reference output, lim), computed once per case and shared"""
    img = R.case_input(n, c, h, w)
    luts = R.luts_ref(img, clip, (gy, gx))
    _, _, th, tw = R.tile_geometry(h, w, gy, gx)
    out = np.stack([np.stack([R.clahe_apply_ref(np.ascontiguousarray(img[i, :, :, j]), luts[i, j], th, tw) for j in range(c)], axis=-1)
                    for i in range(n)])
    for a in (img, luts, out):
        a.setflags(write=False)
    return img, luts, out, R.clip_limit(clip, th * tw)


# ---- the LUT kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LUT_CASES)
def test_luts_are_the_restatement(case):
    n, c, h, w, gy, gx, clip = case
    img, want, _, lim = _case(*case)
    got = _gpu_luts(img, gy, gx, lim)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("w", R.CONST_WIDTHS)
def test_luts_of_constant_planes_take_every_redistribution_branch(w):
    got = _gpu_luts(R.const_plane(w)[None, :, :, None], 1, 1, 1)
    assert np.array_equal(got[0, 0, 0, 0], R.const_lut_closed_form(w))


def test_luts_of_an_all_255_plane():
    """the top bin: everything below it comes from the redistribution alone"""
    img = np.full((1, 32, 32, 1), 255, dtype=np.uint8)
    for clip in (4.0, 0.0):
        lim = R.clip_limit(clip, 256)
        got = _gpu_luts(img, 2, 2, lim)
        assert np.array_equal(got, R.luts_ref(img, clip, (2, 2))) and (got[..., 255] == 255).all()
    assert (_gpu_luts(img, 2, 2, 0)[..., :255] == 0).all()


# ---- the apply kernel ---------------------------------------------------------------------------------------------------------------
# (N, C, H, W, gy, gx): tiles 1, 2, 3, 5 x 9, 5, 32; planes smaller than the padded extent; a row shorter than a thread's four bytes
APPLY_SHAPES = [(1, 3, 8, 8, 8, 8), (1, 1, 16, 16, 8, 8), (2, 3, 17, 23, 6, 8), (1, 3, 33, 64, 8, 8), (1, 1, 10, 15, 2, 3), (1, 3, 64, 64, 2, 2),
                (3, 1, 5, 1, 5, 1), (1, 1, 7, 3, 1, 1), (2, 3, 256, 256, 8, 8)]


def _random_luts(n, c, gy, gx, seed):
    """any bytes, not histogram-made: neighbouring tiles far apart, so that the blend takes many exact .5 ties (round half to even)
    and a fused multiply-add would show"""
    return np.random.default_rng(seed).integers(0, 256, (n, c, gy, gx, 256), dtype=np.uint8)


def _apply_ref(img, luts):
    n, h, w, c = img.shape
    _, _, th, tw = R.tile_geometry(h, w, *luts.shape[2:4])
    return np.stack([np.stack([R.clahe_apply_ref(np.ascontiguousarray(img[i, :, :, j]), luts[i, j], th, tw) for j in range(c)], axis=-1)
                     for i in range(n)])


@pytest.mark.parametrize("shape", APPLY_SHAPES)
def test_apply_with_random_luts_is_the_restatement(shape):
    n, c, h, w, gy, gx = shape
    img = np.random.default_rng(h * w).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    luts = _random_luts(n, c, gy, gx, 7)
    want = _apply_ref(img, luts)
    for shift in ((0, 1) if h <= 64 else (0,)):                                 # 1: pointers off a 4-byte boundary, the byte-wise path
        got = _gpu_apply(img, luts, shift)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (shape, shift, len(bad), bad[:5].tolist())


def test_apply_takes_exact_ties_and_grid_one_is_the_lut_itself():
    # tile 1: every interior weight is exactly 0.5, so odd sums of two LUT entries land on .5
    img = np.random.default_rng(3).integers(0, 256, (1, 8, 8, 1), dtype=np.uint8)
    luts = _random_luts(1, 1, 8, 8, 11)
    _, _, th, tw = R.tile_geometry(8, 8, 8, 8)
    assert (th, tw) == (1, 1)
    lf = luts[0, 0].astype(np.float64)
    y, x = np.mgrid[1:8, 1:8]
    v = img[0, 1:8, 1:8, 0]
    exact = 0.25 * (lf[y - 1, x - 1, v] + lf[y - 1, x, v] + lf[y, x - 1, v] + lf[y, x, v])
    ties = np.abs(exact - np.floor(exact) - 0.5) < 1e-9
    assert ties.sum() >= 5
    got = _gpu_apply(img, luts)[0, 1:8, 1:8, 0]
    assert np.array_equal(got[ties], np.rint(exact[ties]).astype(np.uint8))      # numpy's rint rounds half to even; halves are exact in fp32
    assert np.array_equal(got, np.rint(exact).astype(np.uint8))
    # grid (1, 1): the blend of one LUT with itself, weights that sum to 1
    img = np.random.default_rng(4).integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    luts = _random_luts(2, 3, 1, 1, 12)
    got = _gpu_apply(img, luts)
    for i in range(2):
        for j in range(3):
            assert np.array_equal(got[i, :, :, j], luts[i, j, 0, 0][img[i, :, :, j]])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LUT_CASES)
def test_clahe_end_to_end_is_the_restatement(case):
    from utils.clahe import clahe, clahe_luts
    n, c, h, w, gy, gx, clip = case
    img, luts, want, _ = _case(*case)
    g = torch.from_numpy(img).to(DEV)
    got = clahe(g, clip, (gy, gx))
    assert got.shape == g.shape and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(clahe_luts(g, clip, (gy, gx)).cpu().numpy(), luts)
    assert np.array_equal(g.cpu().numpy(), img)
    if c == 1:                                                                  # [N, H, W] is C = 1
        got3 = clahe(g[..., 0], clip, (gy, gx))
        assert got3.shape == g.shape[:3] and torch.equal(got3, got[..., 0])


def test_clahe_constant_images_and_defaults():
    from utils.clahe import clahe
    for w in R.CONST_WIDTHS:
        img = R.const_plane(w)[None]
        got = clahe(torch.from_numpy(img).to(DEV), 0.5, 1).cpu().numpy()
        assert np.array_equal(got, R.clahe_ref(img, 0.5, 1)) and (got == R.const_lut_closed_form(w)[R.CONST_VALUE]).all()
    for value, want in ((0, 8), (7, 12), (255, 255)):                           # tests/test_clahe_cpu.py derives these by hand
        got = clahe(torch.full((1, 64, 64, 3), value, dtype=torch.uint8, device=DEV))        # defaults: clip 4, grid 8
        assert bool((got == want).all()), (value, got.unique().tolist())
    grey = torch.from_numpy(R.xray_like(1, 64, 64, 5)).to(DEV)
    rgb = clahe(grey[..., None].expand(1, 64, 64, 3).contiguous())
    assert torch.equal(rgb[..., 0], rgb[..., 1]) and torch.equal(rgb[..., 0], rgb[..., 2]) and torch.equal(rgb[..., 0], clahe(grey))


# ---- transforms ---------------------------------------------------------------------------------------------------------------------
def _batch(n, hs, ws, seed):
    imgs = R.case_input(n, 3, hs, ws, seed)
    yy, xx = np.mgrid[0:hs, 0:ws]
    msks = np.stack([(((yy - hs // 2 - i) ** 2 + (xx - ws // 2) ** 2) < (min(hs, ws) // 3) ** 2).astype(np.uint8) * 255 for i in range(n)])
    return torch.from_numpy(imgs), torch.from_numpy(msks)


def test_eval_transform_is_its_stages_by_hand():
    from mi355.lib import lib
    from utils.clahe import clahe
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    n, s = 5, 64
    imgs, msks = _batch(n, 90, 75, 3)
    for T, m in ((SegBatchTransform, msks), (ClsBatchTransform, None)):        # Cls: 90 x 75 -> 64 x 53, padded with black to 64 x 64
        t = T(s, train=False, device=DEV, clahe=(4.0, 8))
        out = t(imgs, m) if m is not None else (t(imgs), None)
        sq, _ = t._to_square(imgs.to(DEV).contiguous(), m, n, 90, 75)
        eq = clahe(sq, 4.0, 8)
        assert np.array_equal(eq.cpu().numpy(), R.clahe_ref(sq.cpu().numpy(), 4.0, 8))
        want = torch.empty(n, 3, s, s, dtype=torch.float32, device=DEV)
        lib.mi355_normalize_u8(eq, n, s, s, 3, None, t.mean, t.std, want)
        assert torch.equal(out[0], want)
        plain = T(s, train=False, device=DEV)
        ref = plain(imgs, m) if m is not None else (plain(imgs), None)
        assert not torch.equal(out[0], ref[0])
        if m is not None:
            assert torch.equal(out[1], ref[1]) and set(np.unique(out[1].cpu().numpy())) <= {0.0, 1.0}
        else:
            assert bool((sq[:, :, :5] == 0).all()) and not bool((eq[:, :, :5] == 0).all())      # the padding takes part, as in A.CLAHE


def test_train_mode_same_seed_same_masks_other_images():
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    imgs, msks = _batch(6, 90, 75, 5)
    a = SegBatchTransform(64, train=True, seed=9, device=DEV)
    b = SegBatchTransform(64, train=True, seed=9, device=DEV, clahe=(4.0, 8))
    for _ in range(2):                                                          # two batches: CLAHE consumes no draw
        (xa, ya), (xb, yb) = a(imgs, msks), b(imgs, msks)
        assert torch.equal(ya, yb) and not torch.equal(xa, xb) and bool(torch.isfinite(xb).all())
    ca = ClsBatchTransform(64, train=True, seed=9, device=DEV)(imgs)
    cb = ClsBatchTransform(64, train=True, seed=9, device=DEV, clahe=(4.0, 8))(imgs)
    cc = ClsBatchTransform(64, train=True, seed=9, device=DEV, clahe=(4.0, 8))(imgs)
    assert tuple(cb.shape) == (6, 3, 64, 64) and torch.equal(cb, cc) and not torch.equal(ca, cb)
    # with elastic as well: both options in one transform
    e0 = SegBatchTransform(64, train=True, seed=9, device=DEV, elastic=(128.0, 5.12, 1.0))(imgs, msks)
    e1 = SegBatchTransform(64, train=True, seed=9, device=DEV, elastic=(128.0, 5.12, 1.0), clahe=(4.0, 8))(imgs, msks)
    assert torch.equal(e0[1], e1[1]) and not torch.equal(e0[0], e1[0])


def test_clahe_none_is_todays_batches():
    from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
    imgs, msks = _batch(5, 90, 75, 3)
    for train in (False, True):
        x0, y0 = SegBatchTransform(64, train=train, seed=4, device=DEV)(imgs, msks)
        x1, y1 = SegBatchTransform(64, train=train, seed=4, device=DEV, clahe=None)(imgs, msks)
        assert torch.equal(x0, x1) and torch.equal(y0, y1)
        c0 = ClsBatchTransform(64, train=train, seed=4, device=DEV)(imgs)
        assert torch.equal(ClsBatchTransform(64, train=train, seed=4, device=DEV, clahe=None)(imgs), c0)


# ---- through train() and the pipeline ---------------------------------------------------------------------------------------------------
def test_train_runs_from_png_files_with_clahe_on(tmp_path, capsys):
    """tests/test_gpu_transforms.py::test_train_runs_from_png_files_end_to_end with CLAHE in the train and the validation transform"""
    pytest.importorskip("PIL.Image")
    from test_dataset_cpu import make_tree
    from utils.dataset import GpuBatchLoader, SegmentationDataset
    from utils.gpu_transforms import SegBatchTransform
    from utils.helpers import get_seg_model, train
    root = str(tmp_path / "dataset")
    make_tree(root, n=13)
    ds_tr = SegmentationDataset(root, SegBatchTransform(64, train=True, device=DEV, clahe=(4.0, 8)), "train")
    ds_va = SegmentationDataset(root, SegBatchTransform(64, train=False, device=DEV, clahe=(4.0, 8)), "train")
    perm = torch.randperm(12, generator=torch.Generator().manual_seed(0)).tolist()
    tr = GpuBatchLoader(ds_tr, 4, shuffle=True, device=DEV, indices=perm[:9])
    va = GpuBatchLoader(ds_va, 4, shuffle=False, device=DEV, indices=perm[9:])
    best = train(get_seg_model("attentionunet"), tr, va, torch.device(DEV), 2, 1e-3, "AttentionUNet", str(tmp_path / "w"), seg=True)
    out = capsys.readouterr().out
    assert np.isfinite(best) and "Ep2" in out and os.path.exists(tmp_path / "w" / "AttentionUNet_best_loss.pt")


def test_pipeline_process_files_with_clahe(tmp_path):
    pytest.importorskip("PIL.Image")
    import glob
    import test_gpu_pipeline as P
    from mi355.lib import lib
    from test_dataset_cpu import make_tree
    from utils.clahe import clahe
    from utils.dataset import decode_batch, read_files
    from utils.gpu_transforms import SegBatchTransform
    from utils.pipeline import JointPipeline
    root = str(tmp_path / "dataset")
    make_tree(root, n=6)
    paths = sorted(glob.glob(os.path.join(root, "*", "images", "*.png")))
    assert len(paths) == 6
    cls_sd, seg_sd, _, _ = P._fixture("ResNet18")
    cm, sm = P._models(torch.float32, cls_sd, seg_sd, "ResNet18")
    pipe = JointPipeline(cm, sm, device=DEV, bucket=4)
    assert pipe.clahe is None
    plain = pipe.process_files(paths, size=64)
    pipe.clahe = (4.0, 8)
    assert pipe.clahe == (4.0, (8, 8))
    got = pipe.process_files(paths, size=64)
    assert [r[1] for r in got] != [r[1] for r in plain]                           # the option reaches the models
    assert len(got) == 6 and all(len(r) == 3 and r[0] in pipe.classes and isinstance(r[1], float) for r in got)
    assert all(r[2] is None or (r[2].dtype == torch.uint8 and tuple(r[2].shape) == (64, 64)) for r in got)
    # the batch equalised by hand
    imgs = decode_batch(read_files(paths), 3, 8, names=paths).to(DEV)
    t = SegBatchTransform(64, train=False, device=DEV)
    sq, _ = t._to_square(imgs.contiguous(), None, 6, imgs.shape[1], imgs.shape[2])
    x = torch.empty(6, 3, 64, 64, dtype=torch.float32, device=DEV)
    lib.mi355_normalize_u8(clahe(sq, 4.0, 8), 6, 64, 64, 3, None, t.mean, t.std, x)
    want = pipe.process_batch(x)
    for (p1, c1, m1), (p2, c2, m2) in zip(got, want):
        assert p1 == p2 and c1 == c2 and (m1 is None) == (m2 is None)
        assert m1 is None or torch.equal(m1, m2)
    res = pipe.process_images(paths, size=64)                                   # the overlays: at the file's own size, on its own pixels
    assert [r[0] for r in res] == [r[0] for r in got]
    assert all(r[2] is None or r[2].shape == (299, 299, 3) for r in res)
