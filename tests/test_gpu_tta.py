"""-m gpu: test-time augmentation (csrc/tta.hip, utils/tta.py, the ``tta=`` option of utils/tester.py and utils/pipeline.py) against the
numpy restatement tests/tta_ref.py, which tests/test_tta_cpu.py pins to hand-derived facts.

What is + - * / floor alone is compared byte for byte (the warp; the fold's mean, variance and valid count with ``prob == 0``).  What
goes through the device's expf is compared within bounds derived in tta_ref.py from its documented accuracy (1 ulp):

  sigmoid' = 1 / (1 + expf(-v)): 1 ulp = 2u relative from expf (u = 2^-24), which reaches the result scaled by e / (1 + e) < 1, plus
  u for the add and u for the divide -> SIGMOID_ERR = 4u = 2^-22 absolute (the value is <= 1);
  mean of cnt <= K sigmoids: cnt SIGMOID_ERR from the terms, cnt - 1 roundings of partial sums <= cnt (<= cnt u each), all divided
  by cnt, plus u for the division -> mean_prob_bound(K) = SIGMOID_ERR + K u (K = 16: 1.2e-6);
  variance: d = v - mean is off by e_d = SIGMOID_ERR + mean_prob_bound(K) + u, d^2 (|d| <= 1) by 2 e_d + u, the mean of them adds
  K u -> var_prob_bound(K) = 2 e_d + (K + 1) u (K = 16: 4.0e-6).

A thresholded output (a view's vote, the mask) may differ from the restatement only where the restatement's float64 value lies
within that bound of the threshold, and at most 1 pixel in 10 000 (at least 1) may be such a pixel — asserted on the restatement.
Every call through the ABI writes into buffers pre-filled with a sentinel between guard bands and is checked for intact guards, an
unchanged source and two bit-identical runs."""
import functools

import numpy as np
import pytest
import torch

import tta_ref as R
from oracle import nets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A
_NP = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int32: np.int32}


class Guarded:
    """``count`` elements of ``dtype`` filled with sentinel bytes between two guard bands; ``shift``: the view starts that many bytes
    off a 16-byte boundary"""

    def __init__(self, count, dtype=torch.float32, shift=0, fill=SENTINEL):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((self.nbytes + 2 * GUARD + shift,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.lo = GUARD + shift
        self.whole[self.lo:self.lo + self.nbytes] = fill
        self.t = self.whole[self.lo:self.lo + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == shift % 16

    def intact(self):
        return bool((self.whole[:self.lo] == GUARD_BYTE).all()) and bool((self.whole[self.lo + self.nbytes:] == GUARD_BYTE).all())

    def numpy(self, shape):
        return self.t.cpu().numpy().reshape(shape)


def _src(arr, shift=0):
    g = Guarded(arr.size, torch.float32, shift)
    g.t.copy_(torch.from_numpy(np.array(arr, np.float32)).reshape(-1))
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _cap(npix):
    return max(1, npix // 10000)


# ---- mi355_warp_f32 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shift", [((2, 3, 13, 19), 0), ((1, 1, 2, 2), 0), ((3, 3, 64, 64), 0), ((2, 3, 13, 19), 4), ((3, 3, 64, 64), 4)])
def test_warp_f32_is_the_restatement(shape, shift):
    from mi355.lib import lib
    N, C, H, W = shape
    x = R.normal_maps(shape, 10)
    m = R.mixed_matrices(N, H, W, which=(3 if shift else 0) + (N < 3))      # between them the cases of a shape take all six views
    want = R.warp_ref(x, m)
    src, md = _src(x, shift), torch.from_numpy(m).to(DEV)
    outs = []
    for _ in range(2):
        dst = Guarded(x.size, torch.float32, shift)
        lib.mi355_warp_f32(src.t, N, C, H, W, md, dst.t)
        torch.cuda.synchronize()
        assert dst.intact()
        outs.append(dst.numpy(shape))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    assert src.intact() and np.array_equal(_bits(src.numpy(shape)), _bits(x)) and np.array_equal(md.cpu().numpy(), m)
    bad = np.argwhere(_bits(outs[0]) != _bits(want))
    assert bad.size == 0, (len(bad), bad[:5].tolist())


def test_warp_f32_all_six_views_on_one_batch():
    from mi355.lib import lib
    x = R.normal_maps((6, 2, 13, 19), 11)
    m = R.mixed_matrices(6, 13, 19)
    dst = Guarded(x.size)
    lib.mi355_warp_f32(_src(x).t, 6, 2, 13, 19, torch.from_numpy(m).to(DEV), dst.t)
    torch.cuda.synchronize()
    assert dst.intact() and np.array_equal(_bits(dst.numpy(x.shape)), _bits(R.warp_ref(x, m)))
    assert np.array_equal(dst.numpy(x.shape)[0], x[0]) and np.array_equal(dst.numpy(x.shape)[3], np.flip(x[3], 2))


def test_warp_f32_bad_arguments():
    from mi355.lib import lib
    x = torch.zeros(1, 1, 4, 4, device=DEV)
    m = torch.zeros(1, 6, device=DEV)
    for args in ((None, 1, 1, 4, 4, m, x), (x, 0, 1, 4, 4, m, torch.empty_like(x)), (x, 1, 1, 4, 4, None, torch.empty_like(x)),
                 (x, 1, 1, 4, 4, m, x)):
        with pytest.raises(RuntimeError, match="warp_f32"):
            lib.mi355_warp_f32(*args)


# ---- mi355_tta_fold --------------------------------------------------------------------------------------------------------------
VIEWS = {1: [R.IDENTITY], 2: R.PRESETS["hflip"], 6: R.PRESETS["full"], 16: R.VIEWS16}


@functools.lru_cache(maxsize=None)
def _fold_case(K, N, H, W):
    """-> (z, s2d, restatement with prob = 0, restatement with prob = 1), computed once per case and shared, read-only"""
    z = R.normal_maps((K, N, H, W), 100 + K + N + H)
    s2d = R.view_matrices(VIEWS[K], H, W)[1]
    refs = [R.fold_ref(z, s2d, prob) for prob in (0, 1)]
    for a in [z, s2d] + [v for r in refs for v in r.values()]:
        a.setflags(write=False)
    return z, s2d, refs[0], refs[1]


def _gpu_fold(z, s2d, prob, thr=0.5, shift=0, skip=(), idx=None, rows=None, runs=2):
    """mi355_tta_fold through the ABI -> dict of numpy arrays (None for the outputs in ``skip``)"""
    from mi355.lib import lib
    K, N, H, W = z.shape
    src, sd = _src(z), torch.from_numpy(np.array(s2d, np.float32)).to(DEV)
    idx_d = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=DEV)
    rows = N if rows is None else rows
    outs = []
    for _ in range(runs):
        g = {"mean": Guarded(N * H * W, torch.float32, shift), "var": Guarded(N * H * W, torch.float32, shift),
             "votes": Guarded(N * 2 * H * W, torch.uint8), "mask": Guarded(rows * H * W, torch.uint8)}
        ptr = {k: (None if k in skip else v.t) for k, v in g.items()}
        lib.mi355_tta_fold(src.t, K, N, H, W, sd, prob, thr, idx_d, ptr["mean"], ptr["var"], ptr["votes"], ptr["mask"])
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values())
        for k in skip:                                  # a skipped output is not touched at all
            assert bool((g[k].t.view(torch.uint8) == SENTINEL).all())
        outs.append({"mean": g["mean"].numpy((N, H, W)), "var": g["var"].numpy((N, H, W)), "votes": g["votes"].numpy((N, 2, H, W)),
                     "mask": g["mask"].numpy((rows, H, W))})
    for o in outs[1:]:
        assert all(np.array_equal(o[k].view(np.uint8), outs[0][k].view(np.uint8)) for k in o)
    assert src.intact() and np.array_equal(_bits(src.numpy(z.shape)), _bits(z))
    return outs[0]


def _check_decisions(got, ref, npix):
    """votes and mask against the restatement, except where it is within the device's error of the threshold"""
    for near in (ref["near_votes"], ref["near_mask"]):
        assert int(near.sum()) <= _cap(npix), "the seeded input itself has too many pixels at the threshold"
    assert np.array_equal(got["votes"][:, 1], ref["valid"])
    assert np.array_equal(got["votes"][:, 0][~ref["near_votes"]], ref["votes"][~ref["near_votes"]])
    assert np.abs(got["votes"][:, 0].astype(int) - ref["votes"].astype(int)).max() <= int(ref["near_votes"].any()) * ref["valid"].max()
    assert np.array_equal(got["mask"][~ref["near_mask"]], ref["mask"][~ref["near_mask"]])
    assert set(np.unique(got["mask"])) <= {0, 255}


@pytest.mark.parametrize("hw", [(13, 19), (64, 64)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 6, 16])
def test_fold_of_logits_is_the_restatement_byte_for_byte(K, N, hw):
    z, s2d, ref, _ = _fold_case(K, N, *hw)
    got = _gpu_fold(z, s2d, 0)
    for k in ("mean", "var"):
        bad = np.argwhere(_bits(got[k]) != _bits(ref[k]))
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())
    _check_decisions(got, ref, N * hw[0] * hw[1])
    if K > 2:                                           # rotated views leave the frame somewhere, the identity never does
        assert ref["valid"].min() >= 1 and ref["valid"].min() < K and ref["valid"].max() == K


@pytest.mark.parametrize("hw", [(13, 19), (64, 64)])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 6, 16])
def test_fold_of_probabilities_is_within_the_derived_bound(K, N, hw):
    """bounds: this module's docstring; the restatement is fed the exact float32 sampled logits and evaluated in float64"""
    z, s2d, _, ref = _fold_case(K, N, *hw)
    got = _gpu_fold(z, s2d, 1)
    err_mean = np.abs(got["mean"].astype(np.float64) - ref["mean"]).max()
    err_var = np.abs(got["var"].astype(np.float64) - ref["var"]).max()
    print(f"K={K} N={N} {hw}: |mean - ref| {err_mean:.3e} (bound {R.mean_prob_bound(K):.3e}), |var - ref| {err_var:.3e} (bound {R.var_prob_bound(K):.3e})")
    assert err_mean <= R.mean_prob_bound(K)
    assert err_var <= R.var_prob_bound(K)
    _check_decisions(got, ref, N * hw[0] * hw[1])


@pytest.mark.parametrize("prob", [0, 1])
@pytest.mark.parametrize("skip", ["var", "votes", "mask"])
def test_fold_skips_a_null_output_and_leaves_the_others_alone(skip, prob):
    z, s2d, _, _ = _fold_case(6, 3, 13, 19)
    full = _gpu_fold(z, s2d, prob, runs=1)
    part = _gpu_fold(z, s2d, prob, skip=(skip,), runs=1)
    for k in ("mean", "var", "votes", "mask"):
        if k != skip:
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k


def test_fold_scatters_the_mask_rows_through_idx():
    z, s2d, ref, _ = _fold_case(6, 3, 13, 19)
    idx = [5, 0, 3]
    got = _gpu_fold(z, s2d, 0, idx=idx, rows=7)
    plain = _gpu_fold(z, s2d, 0, runs=1)
    for n, r in enumerate(idx):
        assert np.array_equal(got["mask"][r], plain["mask"][n])
    for r in set(range(7)) - set(idx):
        assert (got["mask"][r] == SENTINEL).all()
    assert np.array_equal(_bits(got["mean"]), _bits(ref["mean"]))


@pytest.mark.parametrize("N,hw", [(3, (13, 19)), (2, (64, 64))])
def test_fold_of_one_identity_view_is_the_logits_and_mask_scatter(N, hw):
    from mi355.lib import lib
    z, s2d, _, _ = _fold_case(1, 3, *hw)
    z = z[:, :N]
    got = _gpu_fold(z, s2d, 0)
    assert np.array_equal(_bits(got["mean"]), _bits(z[0])) and (got["var"] == 0).all()
    assert (got["votes"][:, 1] == 1).all() and np.array_equal(got["votes"][:, 0] * 255, got["mask"])
    out = torch.zeros(N, hw[0] * hw[1], dtype=torch.uint8, device=DEV)
    lib.mi355_mask_scatter(torch.from_numpy(z[0].copy()).to(DEV), torch.arange(N, dtype=torch.int32, device=DEV), N, hw[0] * hw[1], 0.5, out)
    assert np.array_equal(out.cpu().numpy().reshape(got["mask"].shape), got["mask"])


@pytest.mark.parametrize("prob", [0, 1])
def test_fold_into_misaligned_outputs(prob):
    z, s2d, _, _ = _fold_case(6, 3, 13, 19)
    a, b = _gpu_fold(z, s2d, prob, runs=1), _gpu_fold(z, s2d, prob, shift=4)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_fold_threshold_other_than_one_half():
    z, s2d, _, _ = _fold_case(2, 1, 13, 19)
    ref = R.fold_ref(z, s2d, 0, thr=0.8)
    got = _gpu_fold(z, s2d, 0, thr=0.8)
    _check_decisions(got, ref, 13 * 19)
    assert 0 < (got["mask"] == 255).mean() < 0.4


def test_fold_bad_arguments():
    from mi355.lib import lib
    z = torch.zeros(17, 1, 4, 4, device=DEV)
    s2d = torch.zeros(17, 6, device=DEV)
    mean = torch.empty(1, 4, 4, device=DEV)
    for K, zz, mm in ((0, z, mean), (17, z, mean), (2, None, mean), (2, z, None)):
        with pytest.raises(RuntimeError, match="tta_fold"):
            lib.mi355_tta_fold(zz, K, 1, 4, 4, s2d, 0, 0.5, None, mm, None, None, None)
    lib.load()
    raw = lib.raw("mi355_tta_fold")
    assert raw(z.data_ptr(), 0, 1, 4, 4, s2d.data_ptr(), 0, 0.5, None, mean.data_ptr(), None, None, None, None) != 0
    assert raw(z.data_ptr(), 17, 1, 4, 4, s2d.data_ptr(), 0, 0.5, None, mean.data_ptr(), None, None, None, None) != 0
    assert raw(None, 2, 1, 4, 4, s2d.data_ptr(), 0, 0.5, None, mean.data_ptr(), None, None, None, None) != 0


# ---- mi355_cls_tta_decide --------------------------------------------------------------------------------------------------------
def _gpu_cls(logits, keep):
    from mi355.lib import lib
    K, B, C = logits.shape
    src = _src(logits)
    outs = []
    for _ in range(2):
        g = {"probs": Guarded(B * C), "pred": Guarded(B, torch.int32), "conf": Guarded(B), "agree": Guarded(B, torch.int32),
             "kept": Guarded(B, torch.int32), "n_kept": Guarded(1, torch.int32)}
        lib.mi355_cls_tta_decide(src.t, K, B, C, keep, *(g[k].t for k in ("probs", "pred", "conf", "agree", "kept", "n_kept")))
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values())
        o = {k: v.numpy(-1) for k, v in g.items()}
        n = int(o["n_kept"][0])
        assert (o["kept"][n:].view(np.uint8) == SENTINEL).all()          # nothing is written behind the kept indices
        o["kept"] = o["kept"][:n]
        outs.append(o)
    assert all(np.array_equal(outs[0][k].view(np.uint8), outs[1][k].view(np.uint8)) for k in outs[0])
    assert src.intact() and np.array_equal(_bits(src.numpy(logits.shape)), _bits(logits))
    return outs[0]


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("K", [1, 2, 6])
def test_cls_tta_decide_is_the_restatement(K, B):
    """probs within softmax_bound(K, C) = (5 + (C - 1) C) u + (K + 1) u, conf within conf_bound(K, C) (tta_ref.py: expf at 1 ulp, the
    sum of C terms, one division, the mean over K views); everything integer exact where the top two mean probabilities are at
    least 1e-3 apart, which the seeded logits are"""
    from mi355.lib import lib
    C = 3
    logits = R.normal_maps((K, B, C), 47 + K + B, scale=2.0)          # (seeds whose nine cases all keep the margin)
    for keep in (0, 2):
        ref = R.cls_tta_ref(logits, keep)
        assert ref["margin"].min() >= 1e-3
        got = _gpu_cls(logits, keep)
        assert np.array_equal(got["pred"], ref["pred"]) and np.array_equal(got["agree"], ref["agree"])
        assert np.array_equal(got["kept"], ref["kept"]) and int(got["n_kept"][0]) == ref["n_kept"]
        assert np.abs(got["probs"].reshape(B, C).astype(np.float64) - ref["probs"]).max() <= R.softmax_bound(K, C)
        assert np.abs(got["conf"].astype(np.float64) - ref["conf"]).max() <= R.conf_bound(K, C)
    if K == 1:                                          # one view: mi355_cls_decide bit for bit
        z = torch.from_numpy(logits[0].copy()).to(DEV)
        pred, conf = torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, device=DEV)
        kept, n_kept = torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
        lib.mi355_cls_decide(z, B, C, 2, pred, conf, kept, n_kept)
        assert np.array_equal(pred.cpu().numpy(), got["pred"]) and np.array_equal(_bits(conf.cpu().numpy()), _bits(got["conf"]))
        assert int(n_kept) == int(got["n_kept"][0]) and np.array_equal(kept.cpu().numpy()[:int(n_kept)], got["kept"])


def test_cls_tta_decide_bad_arguments():
    from mi355.lib import lib
    z = torch.zeros(17, 2, 3, device=DEV)
    f, i = torch.empty(6, device=DEV), torch.empty(6, dtype=torch.int32, device=DEV)
    for K, zz in ((0, z), (17, z), (1, None)):
        with pytest.raises(RuntimeError, match="cls_tta_decide"):
            lib.mi355_cls_tta_decide(zz, K, 2, 3, 0, f, i, f, i, i, i)


# ---- end to end at 64 x 64 (the models and weights tests/test_gpu_pipeline.py builds; its helpers, copied) ------------------------
def _he(sd):
    """default init has gain 1/sqrt(3); eval-mode BN with fresh running statistics is the identity, so rescale the convolutions to He
    gain to keep activations O(1) through the depth"""
    for v in sd.values():
        if v.dim() == 4:
            v.mul_(6 ** 0.5)
    return sd


@functools.lru_cache(maxsize=None)
def _models():
    """ResNet18 + AttentionUNet, fp32 compute, on the device in eval mode, and the 16 x 3 x 64 x 64 batch they were centred on"""
    from models.segmentation_models.AttentionUNet import AttentionUNet
    cls_sd = _he(nets.default_init_state("ResNet18", seed=3, num_classes=3, head_dropout=True))
    seg_sd = _he(nets.default_init_state("AttentionUNet", seed=4))
    x = torch.randn(16, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():        # centre the logits over the batch: the three classes all occur
        cls_sd["fc.1.bias"] = cls_sd["fc.1.bias"] - nets.NETS["ResNet18"]({k: v.clone() for k, v in cls_sd.items()}, x, False).mean(0)
    sm = AttentionUNet()
    sm.load_state_dict(seg_sd)
    sm.compute_dtype = torch.float32
    return _classifier(cls_sd), sm.to(DEV).eval(), x.to(DEV)


_CLS_SD = {}


def _classifier(cls_sd=None):
    """a fresh ResNet18 on the device from the state _models() made"""
    from models.classification_models.ResNet import ResNet18
    from utils.helpers import add_dropout_to_fc
    if cls_sd is not None:
        _CLS_SD.update(cls_sd)
    elif not _CLS_SD:
        _models()
    cm = ResNet18(num_classes=3)
    add_dropout_to_fc(cm)
    cm.load_state_dict(_CLS_SD)
    cm.compute_dtype = torch.float32
    return cm.to(DEV).eval()


def test_segmenter_with_the_identity_view_is_the_model():
    from utils.tta import TTASegmenter
    _, sm, x = _models()
    x = x[:4].contiguous()
    with torch.no_grad():
        want = sm(x).float().reshape(4, 64, 64)
    r = TTASegmenter(sm, [R.IDENTITY], merge="logit")(x)
    assert torch.equal(r["mean"].view(torch.int32), want.view(torch.int32))
    assert not sm.training and bool((r["valid"] == 1).all()) and bool((r["var"] == 0).all())
    sm.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            TTASegmenter(sm, "hflip")(x)
        assert sm.training                               # left as found
    finally:
        sm.eval()


def test_segmenter_hflip_is_the_mean_of_the_two_torch_flip_passes():
    from utils.tta import TTASegmenter
    _, sm, x = _models()
    x = x[:4].contiguous()
    with torch.no_grad():
        a = sm(x).float()
        b = torch.flip(sm(torch.flip(x, [3]).contiguous()).float(), [3])
        want = ((a + b) / 2).reshape(4, 64, 64)
    r = TTASegmenter(sm, "hflip", merge="logit")(x)
    assert torch.equal(r["mean"].view(torch.int32), want.view(torch.int32))
    assert bool((r["valid"] == 2).all())


def test_pipeline_with_the_identity_view_is_the_plain_pipeline():
    from utils.pipeline import JointPipeline
    cm, sm, x = _models()
    plain = JointPipeline(cm, sm, device=DEV, bucket=4).predict(x)
    one = JointPipeline(cm, sm, device=DEV, bucket=4, tta=[R.IDENTITY], tta_merge="logit").predict(x)
    assert 2 <= int(plain["segmented"].sum()) <= 14
    assert set(plain) == {"pred", "confidence", "masks", "segmented"}           # tta=None: today's outputs
    for k in ("pred", "masks", "segmented"):
        assert torch.equal(plain[k], one[k]), k
    assert torch.equal(plain["confidence"].view(torch.int32), one["confidence"].view(torch.int32))
    assert bool((one["agreement"] == 1).all()) and bool((one["uncertainty"] == 0).all())


def test_pipeline_full_tta_masks_are_the_restatements_fold():
    from utils.pipeline import CLASSES, JointPipeline
    from utils.tta import TTAClassifier, view_logits
    _, sm, x = _models()
    cm = _classifier()                                   # a classifier of its own: its head is re-centred on the merged views
    with torch.no_grad():                                # so that the mean softmax of the six views gives every class to some samples
        cm.fc[1].bias -= TTAClassifier(cm, "full")(x)["logits"].mean((0, 1))
    count = torch.bincount(TTAClassifier(cm, "full")(x)["pred"].long(), minlength=3).tolist()
    mixed = [c for c in range(3) if 2 <= count[c] <= 14]
    assert mixed, count
    positive = mixed[0]
    pipe = JointPipeline(cm, sm, device=DEV, bucket=4, tta="full", positive=CLASSES[positive])
    r = pipe.predict(x)
    assert torch.equal(r["segmented"], r["pred"] == positive)
    seg = r["segmented"].cpu().numpy()
    n = int(seg.sum())
    assert 2 <= n <= 14 and r["uncertainty"].shape == (16, 64, 64) and r["agreement"].dtype == torch.int32
    assert float(r["uncertainty"][~r["segmented"]].abs().sum()) == 0 and float(r["masks"][~r["segmented"]].sum()) == 0
    assert float(r["uncertainty"][r["segmented"]].sum()) > 0
    assert bool(((r["agreement"] >= 1) & (r["agreement"] <= 6)).all())
    kept = np.flatnonzero(seg)
    rows = np.concatenate([kept, np.repeat(kept[:1], -n % 4)])                  # the pipeline's padded batch: the same launch shapes
    with torch.no_grad():
        z = view_logits(sm, x[torch.from_numpy(rows).to(DEV)].contiguous(), R.PRESETS["full"], rows=n).cpu().numpy()
    ref = R.fold_ref(z, R.view_matrices(R.PRESETS["full"], 64, 64)[1], 1)
    assert int(ref["near_mask"].sum()) <= _cap(n * 64 * 64)
    got = r["masks"].cpu().numpy()[kept]
    assert np.array_equal(got[~ref["near_mask"]], ref["mask"][~ref["near_mask"]])
    assert np.abs(r["uncertainty"].cpu().numpy()[kept].astype(np.float64) - ref["var"]).max() <= R.var_prob_bound(6)
    on = ref["mask"] == 255
    same = (ref["votes"] == 0) | (ref["votes"] == ref["valid"])
    want = (on & same).reshape(n, -1).sum(1) / np.maximum(on.reshape(n, -1).sum(1), 1) * 100
    near = int(ref["near_mask"].sum() + ref["near_votes"].sum())                 # each such pixel may enter or leave either count
    assert np.abs(r["stable_percent"].cpu().numpy()[kept] - want).max() <= 1e-3 + 100.0 * 2 * near / max(on.reshape(n, -1).sum(1).min(), 1)
    with pytest.raises(ValueError, match="explain"):
        pipe.predict(x, explain=True)


def _counts_np(p, t):
    P, T = p > 0.5, t > 0.5
    f = lambda a: a.reshape(a.shape[0], -1).sum(1).astype(np.float64)
    return np.stack([f(P & T), f(P), f(T), f(P == T)], 1)


def test_tester_segmentation_with_hflip(capsys):
    from utils import tester
    from utils.tta import TTASegmenter, view_logits
    _, sm, x = _models()
    g = torch.Generator().manual_seed(9)
    loader = [(x[0:4].contiguous(), (torch.rand(4, 1, 64, 64, generator=g) < 0.4).float()),
              (x[4:6].contiguous(), (torch.rand(2, 1, 64, 64, generator=g) < 0.4).float())]
    got = tester.test_segmentation_model(TTASegmenter(sm, "hflip"), loader, DEV, "AttentionUNet")
    text = capsys.readouterr().out
    s2d = R.view_matrices(R.PRESETS["hflip"], 64, 64)[1]
    per_sample, unanimous = [], []
    for images, masks in loader:
        with torch.no_grad():
            z = view_logits(sm, images, R.PRESETS["hflip"]).cpu().numpy()
        ref = R.fold_ref(z, s2d, 1)
        assert not ref["near_mask"].any() and not ref["near_votes"].any()
        for c in _counts_np(ref["mean"], masks.numpy()[:, 0]):
            per_sample.append(tester._metrics_from_counts(c, 64 * 64))
        unanimous.extend(((ref["votes"] == 0) | (ref["votes"] == ref["valid"])).reshape(len(z[0]), -1).mean(1))
    keys = ("iou", "dice", "pixel_accuracy", "precision", "recall", "f1")
    for k in keys:
        assert abs(got[k] - np.mean([m[k] for m in per_sample])) <= 1e-4, k
    assert abs(got["tta_unanimous"] - 100 * np.mean(unanimous)) <= 1e-4 and got["tta_views"] == 2
    assert set(got) == set(keys) | {"tta_unanimous", "tta_views"}
    assert text.count("TTA unanimous:") == 1
    plain = tester.test_segmentation_model(sm, loader, DEV, "AttentionUNet")
    assert set(plain) == set(keys) and "TTA" not in capsys.readouterr().out       # tta=None: today's keys and lines
    logit = tester.test_segmentation_model(TTASegmenter(sm, "hflip", merge="logit"), loader, DEV, "AttentionUNet", surface=True)
    assert set(logit) == set(keys) | set(tester.SURFACE_KEYS) | {"surface_samples", "tta_unanimous", "tta_views"}


def test_tester_classification_with_hflip(capsys):
    from utils import tester
    cm, _, x = _models()
    with torch.no_grad():                                # the samples whose two views leave no doubt: a top-two margin of the mean
        z = torch.stack([cm(x).float(), cm(torch.flip(x, [3]).contiguous()).float()]).cpu().numpy()      # softmax of at least 1e-2
    sure = torch.from_numpy(np.flatnonzero(R.cls_tta_ref(z, 0)["margin"] >= 1e-2)).to(DEV)
    assert len(sure) >= 8
    xs, labels, h = x[sure].contiguous(), torch.arange(len(sure)) % 3, len(sure) // 2
    loader = [(xs[:h].contiguous(), labels[:h]), (xs[h:].contiguous(), labels[h:])]
    got = tester.test_classification_model(cm, loader, DEV, "ResNet18", tta="hflip")
    preds, agree = [], []
    for images, _ in loader:
        with torch.no_grad():
            z = torch.stack([cm(images).float(), cm(torch.flip(images, [3]).contiguous()).float()]).cpu().numpy()
        ref = R.cls_tta_ref(z, 0)
        assert ref["margin"].min() >= 1e-3
        preds.append(ref["pred"])
        agree.append(ref["agree"])
    want = tester.calculate_classification_metrics(np.concatenate(preds), labels.numpy())
    assert np.array_equal(got["confusion_matrix"], want["confusion_matrix"]) and got["accuracy"] == want["accuracy"]
    assert abs(got["tta_agreement"] - np.concatenate(agree).mean() / 2 * 100) <= 1e-9 and got["tta_views"] == 2
    assert "TTA agreement:" in capsys.readouterr().out
    plain = tester.test_classification_model(cm, loader, DEV, "ResNet18")
    assert set(plain) == {"accuracy", "precision", "recall", "f1", "precision_per_class", "recall_per_class", "f1_per_class", "confusion_matrix"}
    assert "TTA" not in capsys.readouterr().out


def test_process_images_says_how_stable_the_highlighted_area_is(tmp_path):
    import re
    from PIL import Image
    from utils.pipeline import CLASSES, JointPipeline
    cm, sm, _ = _models()
    rng = np.random.RandomState(2)
    paths = []
    for i in range(6):
        yy, xx = np.mgrid[0:80, 0:96]
        img = (127 + 80 * np.sin(xx / (9.0 + i)) * np.cos(yy / (6.0 + i)))[..., None] + rng.randint(-10, 10, (80, 96, 3))
        paths.append(str(tmp_path / f"x{i}.png"))
        Image.fromarray(img.clip(0, 255).astype(np.uint8), "RGB").save(paths[-1])
    line = re.compile(r"\nStable under test-time augmentation: (\d+\.\d\d)% of the highlighted pixels \(2 views\)\.")
    segmented = 0
    for positive in CLASSES:                             # whichever class the files get: each sample is segmented under one of the three
        pipe = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive, tta="hflip")
        plain = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive)
        for (pred, conf, img, text), base in zip(pipe.process_images(paths, size=64), plain.process_images(paths, size=64)):
            found = line.findall(text)
            assert "test-time" not in base[3]
            if pred == positive:
                assert len(found) == 1 and 0.0 <= float(found[0]) <= 100.0 and img.shape == (80, 96, 3)
                segmented += 1
            else:
                assert not found and img is None
    assert segmented == 6


def test_stability_is_taken_over_the_masks_that_are_returned():
    """with a postprocess the overlay shows the cleaned masks, so the stable share is theirs: a filter that drops every component
    leaves nothing highlighted and a share of 0, whatever the raw masks held"""
    from utils.pipeline import CLASSES, JointPipeline
    from utils.postprocess import MaskPostprocess
    cm, sm, x = _models()
    raw_pixels = 0
    for positive in CLASSES:
        r = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive, tta="hflip").predict(x)
        none = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive, tta="hflip",
                             postprocess=MaskPostprocess(min_area=64 * 64 + 1)).predict(x)
        assert torch.equal(none["masks_raw"], r["masks"]) and not bool(none["masks"].any())
        assert bool((none["stable_percent"] == 0).all())
        has = (r["masks"] != 0).flatten(1).any(1)
        assert bool((r["stable_percent"][~has] == 0).all()) and bool((r["stable_percent"] <= 100).all())
        raw_pixels += int((r["masks"] != 0).sum())
    assert raw_pixels > 0
