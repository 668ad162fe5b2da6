"""No GPU: pins tests/tta_ref.py — the numpy restatement tests/test_gpu_tta.py holds the kernels to — to facts that can be checked by
hand or against scipy, and utils/tta.py's host side (views, presets, matrices) to the restatement."""
import numpy as np
import pytest

import tta_ref as R

H, W = 13, 19
FULL = R.PRESETS["full"]


def test_identity_and_flip_matrices_are_exact_integers():
    d2s, s2d = R.view_matrices(R.PRESETS["hflip"], H, W)
    want = np.array([[1, 0, 0, 0, 1, 0], [-1, 0, W - 1, 0, 1, 0]], np.float32)
    assert d2s.dtype == np.float32 and np.array_equal(d2s, want) and np.array_equal(s2d, want)
    assert not np.signbit(d2s).any() or np.array_equal(np.signbit(d2s), want < 0)


def test_flip_view_is_np_flip_and_folds_back_bit_for_bit():
    x = R.normal_maps((2, 3, H, W), 1)
    d2s, s2d = R.view_matrices(R.PRESETS["hflip"], H, W)
    view = R.warp_ref(x, np.repeat(d2s[1:2], 2, 0))
    assert np.array_equal(view, np.flip(x, 3))
    assert np.array_equal(R.warp_ref(x, np.repeat(d2s[0:1], 2, 0)), x)
    z = np.stack([x[:, 0], view[:, 0]])                      # a "model" that returns its input's first channel
    f = R.fold_ref(z, s2d, 0)
    assert f["valid_k"].all() and (f["valid"] == 2).all()
    assert np.array_equal(f["mean"], x[:, 0]) and (f["var"] == 0).all()      # (a + a) / 2 is exact


def test_d2s_times_s2d_is_the_identity():
    d2s, s2d = R.view_matrices(R.VIEWS16, H, W, np.float64)
    for a, b in zip(d2s, s2d):
        assert np.abs(R.as3x3(a) @ R.as3x3(b) - np.eye(3)).max() < 1e-12


def test_matrices_follow_shift_scale_rotate_matrix():
    """the convention the train transform uses: its dst -> src matrix (formed there by a numeric inverse) is d2s"""
    from utils.gpu_transforms import shift_scale_rotate_matrix
    d2s, _ = R.view_matrices(R.VIEWS16, H, W, np.float64)
    for (a, s, f), m in zip(R.VIEWS16, d2s):
        assert np.abs(np.array(shift_scale_rotate_matrix(H, W, a, s, 0.0, 0.0, f)) - m).max() < 1e-12


def test_package_views_and_matrices_are_the_restatement():
    from utils import tta
    assert {k: tta.check_views(k) for k in tta.PRESETS} == R.PRESETS
    assert [len(tta.PRESETS[k]) for k in ("hflip", "rot", "full")] == [2, 3, 6]
    for hw in ((H, W), (64, 64), (2, 2)):
        got, want = tta.view_matrices(R.VIEWS16, *hw), R.view_matrices(R.VIEWS16, *hw)
        for g, w_ in zip(got, want):
            assert g.dtype.is_floating_point and g.numpy().dtype == np.float32 and np.array_equal(g.numpy(), w_)


def _interior(valid, margin=2):
    inner = np.zeros_like(valid)
    inner[margin:-margin, margin:-margin] = True
    return valid & inner


@pytest.mark.parametrize("k", range(6))
def test_unwarping_a_warped_ramp_returns_the_ramp(k):
    """bilinear interpolation reproduces linear functions: view = ramp(d2s p) wherever the taps are inside, and sampling the view at
    s2d q gives ramp(q) back; checked at every valid pixel at least 2 px from the border"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ramp = 0.3 * x - 0.2 * y + 1
    d2s, s2d = R.view_matrices(FULL, H, W, np.float64)
    view = R.warp_ref(ramp[None, None], d2s[k:k + 1], np.float64)
    back, valid = R.sample_views(view, s2d[k:k + 1], np.float64)
    at = _interior(valid[0])
    assert at.sum() >= 100                                   # of the 9 x 15 = 135 pixels that far inside
    assert np.abs(back[0, 0] - ramp)[at].max() < 1e-9
    d32, s32 = R.view_matrices(FULL, H, W)
    v32 = R.warp_ref(ramp[None, None].astype(np.float32), d32[k:k + 1])
    b32, ok32 = R.sample_views(v32, s32[k:k + 1])
    # float32: a coordinate <= 19 carries three roundings of <= 2^-20 (3e-6, times the ramp's slope 0.36), a sample of |ramp| <= 8 six
    # of <= 4.8e-7, both once per direction: below 1e-5
    assert np.abs(b32[0, 0].astype(np.float64) - ramp)[_interior(ok32[0])].max() < 1e-5


def test_fp64_bilinear_reflect101_is_scipy_mirror():
    from scipy.ndimage import map_coordinates
    src = R.normal_maps((1, 2, H, W), 2).astype(np.float64)
    d2s, _ = R.view_matrices(FULL, H, W, np.float64)
    for k in range(6):
        got = R.warp_ref(src, d2s[k:k + 1], np.float64)
        sx, sy = R._coords(d2s[k], H, W, np.float64)
        for c in range(2):
            want = map_coordinates(src[0, c], [sy, sx], order=1, mode="mirror")
            assert np.abs(got[0, c] - want).max() < 1e-12


def test_valid_shares():
    _, s2d = R.view_matrices(FULL, H, W)
    _, valid = R.sample_views(np.zeros((6, 1, H, W), np.float32), s2d)
    count = valid.reshape(6, -1).sum(1)
    assert count.tolist() == [247, 195, 229, 247, 195, 229]          # of 247: identity and flip everywhere, the rotated views 0.79 and 0.93
    assert [round(c / 247, 2) for c in count[[1, 2]]] == [0.79, 0.93]
    _, s16 = R.view_matrices(R.VIEWS16, 64, 64)
    assert R.sample_views(np.zeros((16, 1, 64, 64), np.float32), s16)[1][0].all()


def test_fold_counts_votes_and_population_variance_by_hand():
    """two views of a 1 x 2 map, identity and flip: the pixel pairs are (a, b) and (b, a)"""
    z = np.array([[[[2.0, -1.0]]], [[[3.0, 0.5]]]], np.float32)         # view 1 holds the flipped prediction: un-flipped (0.5, 3)
    _, s2d = R.view_matrices(R.PRESETS["hflip"], 1, 2)
    f = R.fold_ref(z, s2d, 0)
    assert np.array_equal(f["mean"], np.float32([[[1.25, 1.0]]])) and np.array_equal(f["var"], np.float32([[[0.5625, 4.0]]]))
    assert f["votes"].tolist() == [[[2, 1]]] and f["valid"].tolist() == [[[2, 2]]] and f["mask"].tolist() == [[[255, 255]]]
    p = R.fold_ref(z, s2d, 1)
    s = R.sigmoid64(np.array([[2.0, 0.5], [-1.0, 3.0]]))
    assert np.allclose(p["mean"][0, 0], s.mean(1), atol=1e-15) and np.allclose(p["var"][0, 0], s.var(1), atol=1e-15)


@pytest.mark.parametrize("bad", [[], [R.IDENTITY] * 17, [(0.0, 1.0, True)], [R.IDENTITY, (45.5, 1.0, False)], [R.IDENTITY, (0.0, 0.4, False)],
                                 [R.IDENTITY, (0.0, 2.5, True)], [R.IDENTITY, (-50.0, 1.0, False)], "diagonal", [R.IDENTITY, (1.0, 1.0)], None])
def test_check_views_rejects(bad):
    from utils.tta import check_views
    with pytest.raises(ValueError):
        check_views(bad)


def test_check_views_accepts_the_limits():
    from utils.tta import check_views
    assert len(check_views([R.IDENTITY] + [(45, 2, True), (-45, 0.5, False)] * 7 + [(0, 1, True)])) == 16
    assert check_views([(0, 1, 0)]) == [R.IDENTITY]


def test_cls_restatement_with_one_view_is_softmax_argmax():
    import torch
    z = R.normal_maps((1, 9, 3), 3)
    r = R.cls_tta_ref(z, 0)
    sm = torch.softmax(torch.from_numpy(z[0]).double(), 1).numpy()
    tol = 2 * np.abs(z).max() * R.U              # the restatement subtracts the maximum in float32, as the device does: |z - max| u
    assert np.abs(r["probs"] - sm).max() < tol and np.array_equal(r["pred"], sm.argmax(1))
    assert np.allclose(r["conf"], 100 * sm.max(1), rtol=tol) and (r["agree"] == 1).all()
    assert np.array_equal(r["kept"], np.flatnonzero(sm.argmax(1) == 0)) and r["n_kept"] == len(r["kept"])


def test_cls_restatement_counts_agreement():
    z = np.float32([[[2, 0, 0]], [[0, 1, 0]], [[3, 0, 0]]])                 # views vote 0, 1, 0; the mean favours 0
    r = R.cls_tta_ref(z, 0)
    assert r["pred"].tolist() == [0] and r["agree"].tolist() == [2] and r["kept"].tolist() == [0]


def test_bounds_are_the_documented_figures():
    assert R.mean_prob_bound(16) < 2e-6 and R.SIGMOID_ERR == 2.0 ** -22
    assert R.var_prob_bound(16) < 5e-6 and R.softmax_bound(6, 3) < 2e-6
