"""-m gpu: sliding-window inference (csrc/sliding.hip, utils/sliding.py, the ``sliding=`` option of utils/tester.py and
utils/pipeline.py) against the numpy restatement tests/sliding_ref.py, which tests/test_sliding_cpu.py pins to hand-derived facts.

What is + * / min max alone is compared byte for byte (the gather; the blend's mean, spread and cover with ``prob == 0``, for both
weightings).  What goes through the device's expf is compared within the bound derived in sliding_ref.py from its documented
accuracy (1 ulp):

  sigmoid' = 1 / (1 + expf(-v)) is within SIGMOID_ERR = 4u = 2^-22 of sigmoid (u = 2^-24; tests/tta_ref.py derives the same figure);
  mean = (sum_i w_i s_i) / (sum_i w_i) over the cnt tiles that cover a pixel, the float32 weights w_i = fl(wy wx) being the same
  numbers on both sides: the products are off by w_i (SIGMOID_ERR + u), the cnt - 1 roundings of num's partial sums (<= D = sum w_i)
  by (cnt - 1) D u, den by a factor within (cnt - 1) u of 1, the division by u -> blend_prob_bound(cnt) = SIGMOID_ERR + (2 cnt + 1) u,
  the last u covering the second-order terms (cnt = 16: 2.2e-6);
  spread = hi - lo of two such sigmoids -> 2 SIGMOID_ERR + u.

The mask may differ from the restatement only where the restatement's float64 decision value lies within that bound (SIGMOID_ERR
for ``prob == 0``) of the threshold, and at most 1 pixel in 10 000 (at least 1) may be such a pixel — asserted on the restatement.
Every call through the ABI writes into buffers pre-filled with a sentinel between guard bands and is checked for intact guards, an
unchanged source and two bit-identical runs."""
import functools

import numpy as np
import pytest
import torch

import sliding_ref as R
from oracle import nets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A


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

    def untouched(self):
        return bool((self.t.view(torch.uint8) == SENTINEL).all())

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


def _host(starts):
    return torch.tensor(starts, dtype=torch.int32)


# the geometries of the issue: (N, C, H, W), T, overlap
GEOMS = [((2, 3, 37, 45), 16, 0.25), ((1, 1, 7, 9), 5, 0.5), ((2, 3, 64, 64), 64, 0.5), ((3, 3, 96, 112), 64, 0.5)]
BLEND_GEOMS = [(s[0], s[2], s[3], T, ov) for s, T, ov in GEOMS] + [(1, 40, 40, 16, 0.75)]


# ---- mi355_tile_gather_f32 -------------------------------------------------------------------------------------------------------
def _gpu_gather(x, T, ys, xs, tiles, shift=0, runs=2):
    from mi355.lib import lib
    N, C, H, W = x.shape
    M = len(tiles)
    src, td = _src(x, shift), torch.tensor(tiles, dtype=torch.int32, device=DEV)
    hy, hx = _host(ys), _host(xs)
    outs = []
    for _ in range(runs):
        dst = Guarded(M * C * T * T, torch.float32, shift)
        lib.mi355_tile_gather_f32(src.t, N, C, H, W, T, hy, len(ys), hx, len(xs), td, M, dst.t)
        torch.cuda.synchronize()
        assert dst.intact()
        outs.append(dst.numpy((M, C, T, T)))
    assert all(np.array_equal(_bits(o), _bits(outs[0])) for o in outs[1:])
    assert src.intact() and np.array_equal(_bits(src.numpy(x.shape)), _bits(x)) and td.cpu().tolist() == list(tiles)
    assert hy.tolist() == list(ys) and hx.tolist() == list(xs)
    return outs[0]


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("shape,T,overlap", GEOMS)
def test_gather_is_the_restatement_byte_for_byte(shape, T, overlap, shift):
    N, C, H, W = shape
    x = R.normal_maps(shape, 20 + H)
    ys, xs = R.tile_starts(H, T, overlap), R.tile_starts(W, T, overlap)
    total = N * len(ys) * len(xs)
    rng = np.random.default_rng(H + shift)
    lists = {"natural": list(range(total)), "reversed": list(range(total))[::-1][:max(1, total - 1)],
             "repeats": [0, 0, total - 1] + rng.integers(0, total, 4).tolist()}                # M = total, total - 1, 7
    for name, tiles in lists.items():
        got = _gpu_gather(x, T, ys, xs, tiles, shift)
        bad = np.argwhere(_bits(got) != _bits(R.gather_ref(x, T, ys, xs, tiles)))
        assert bad.size == 0, (name, len(bad), bad[:5].tolist())
    if len(ys) * len(xs) == 1:
        assert np.array_equal(_bits(_gpu_gather(x, T, ys, xs, lists["natural"], shift, runs=1)), _bits(x))      # one tile: the image


def test_gather_leaves_the_tiles_of_entries_outside_the_grid_alone():
    x = R.normal_maps((2, 3, 37, 45), 5)
    ys, xs = R.tile_starts(37, 16, 0.25), R.tile_starts(45, 16, 0.25)
    tiles = [3, -1, 24, 23, 2 ** 31 - 1, -2 ** 31]                                          # 24 tiles: 0 .. 23 exist
    got = _gpu_gather(x, 16, ys, xs, tiles)
    want = R.gather_ref(x, 16, ys, xs, [3, 0, 0, 23, 0, 0])
    sentinel = np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]
    for i, t in enumerate(tiles):
        if 0 <= t < 24:
            assert np.array_equal(_bits(got[i]), _bits(want[i])), i
        else:
            assert (_bits(got[i]) == sentinel).all(), i


def test_gather_python_wrapper():
    from utils.sliding import gather_tiles
    x = R.normal_maps((2, 3, 37, 45), 3)
    ys, xs = R.tile_starts(37, 16, 0.25), R.tile_starts(45, 16, 0.25)
    xd = torch.from_numpy(x).to(DEV)
    assert np.array_equal(_bits(gather_tiles(xd, 16, 0.25).cpu().numpy()), _bits(R.gather_ref(x, 16, ys, xs, list(range(24)))))
    assert np.array_equal(_bits(gather_tiles(xd, 16, 0.25, [23, 5, 5]).cpu().numpy()), _bits(R.gather_ref(x, 16, ys, xs, [23, 5, 5])))
    with pytest.raises(ValueError, match="tile numbers"):
        gather_tiles(xd, 16, 0.25, [24])
    with pytest.raises(ValueError, match="tile"):
        gather_tiles(xd, 38, 0.25)
    with pytest.raises(ValueError, match="float32"):
        gather_tiles(xd.double(), 16, 0.25)
    with pytest.raises(ValueError, match="contiguous"):
        gather_tiles(xd[:, :, :, ::2], 16, 0.25)


# ---- mi355_tile_blend ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blend_case(N, H, W, T, overlap, weighting):
    """-> (z, ys, xs, w, restatement with prob = 0, restatement with prob = 1), computed once per case and shared, read-only"""
    ys, xs = R.tile_starts(H, T, overlap), R.tile_starts(W, T, overlap)
    z = R.normal_maps((N * len(ys) * len(xs), T, T), 100 + N + H + T)
    w = R.window_weights(T, weighting)
    refs = [R.blend_ref(z, N, H, W, T, ys, xs, w, w, prob) for prob in (0, 1)]
    for a in [z, w] + [v for r in refs for v in r.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return z, ys, xs, w, refs[0], refs[1]


def _gpu_blend(z, N, H, W, T, ys, xs, wy, wx, prob, thr=0.5, shift=0, skip=(), idx=None, rows=None, runs=2):
    """mi355_tile_blend through the ABI -> dict of numpy arrays"""
    from mi355.lib import lib
    src = _src(z, shift)
    wyd, wxd = torch.from_numpy(np.array(wy, np.float32)).to(DEV), torch.from_numpy(np.array(wx, np.float32)).to(DEV)
    hy, hx = _host(ys), _host(xs)
    idx_d = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=DEV)
    rows = N if rows is None else rows
    outs = []
    for _ in range(runs):
        g = {"mean": Guarded(N * H * W, torch.float32, shift), "spread": Guarded(N * H * W, torch.float32, shift),
             "cover": Guarded(H * W, torch.uint8, shift and 1), "mask": Guarded(rows * H * W, torch.uint8, shift and 1)}
        ptr = {k: (None if k in skip else v.t) for k, v in g.items()}
        lib.mi355_tile_blend(src.t, N, H, W, T, hy, len(ys), hx, len(xs), wyd, wxd, prob, thr, idx_d, ptr["mean"], ptr["spread"], ptr["cover"],
                             ptr["mask"])
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values())
        for k in skip:                                  # a skipped output is not touched at all
            assert g[k].untouched()
        outs.append({"mean": g["mean"].numpy((N, H, W)), "spread": g["spread"].numpy((N, H, W)), "cover": g["cover"].numpy((H, W)),
                     "mask": g["mask"].numpy((rows, H, W))})
    for o in outs[1:]:
        assert all(np.array_equal(o[k].view(np.uint8), outs[0][k].view(np.uint8)) for k in o)
    assert src.intact() and np.array_equal(_bits(src.numpy(z.shape)), _bits(z))
    assert np.array_equal(wyd.cpu().numpy(), np.array(wy, np.float32)) and hy.tolist() == list(ys) and hx.tolist() == list(xs)
    return outs[0]


def _check_mask(got, ref, npix):
    """the mask against the restatement, except where it is within the device's error of the threshold"""
    assert int(ref["near_mask"].sum()) <= _cap(npix), "the seeded input itself has too many pixels at the threshold"
    assert np.array_equal(got["mask"][~ref["near_mask"]], ref["mask"][~ref["near_mask"]])
    assert set(np.unique(got["mask"])) <= {0, 255}


@pytest.mark.parametrize("weighting", ["gaussian", "constant"])
@pytest.mark.parametrize("N,H,W,T,overlap", BLEND_GEOMS)
def test_blend_of_logits_is_the_restatement_byte_for_byte(N, H, W, T, overlap, weighting):
    z, ys, xs, w, ref, _ = _blend_case(N, H, W, T, overlap, weighting)
    got = _gpu_blend(z, N, H, W, T, ys, xs, w, w, 0)
    for k in ("mean", "spread"):
        bad = np.argwhere(_bits(got[k]) != _bits(ref[k]))
        assert bad.size == 0, (k, len(bad), bad[:5].tolist())
    assert np.array_equal(got["cover"], ref["cover"])
    _check_mask(got, ref, N * H * W)
    depth = R.depth_bound(H, T, overlap) * R.depth_bound(W, T, overlap)
    assert 1 <= ref["cover"].min() and ref["cover"].max() <= depth
    if overlap == 0.75:
        assert ref["cover"].max() == 16
    assert (got["spread"][:, ref["cover"] == 1] == 0).all()


@pytest.mark.parametrize("weighting", ["gaussian", "constant"])
@pytest.mark.parametrize("N,H,W,T,overlap", BLEND_GEOMS)
def test_blend_of_probabilities_is_within_the_derived_bound(N, H, W, T, overlap, weighting):
    """bounds: this module's docstring; the restatement is fed the exact float32 logits and weights and evaluated in float64"""
    z, ys, xs, w, _, ref = _blend_case(N, H, W, T, overlap, weighting)
    got = _gpu_blend(z, N, H, W, T, ys, xs, w, w, 1)
    bound = R.blend_prob_bound(ref["cover"].astype(np.float64))[None]
    err = np.abs(got["mean"].astype(np.float64) - ref["mean"])
    err_spread = np.abs(got["spread"].astype(np.float64) - ref["spread"]).max()
    print(f"N={N} {H}x{W} T={T} {weighting}: |mean - ref| {err.max():.3e} (bound {bound.max():.3e}), max err / bound {(err / bound).max():.3f}, "
          f"|spread - ref| {err_spread:.3e} (bound {R.SPREAD_PROB_BOUND:.3e})")
    assert (err <= bound).all()
    assert err_spread <= R.SPREAD_PROB_BOUND
    assert np.array_equal(got["cover"], ref["cover"]) and (got["spread"][:, ref["cover"] == 1] == 0).all()
    _check_mask(got, ref, N * H * W)


@pytest.mark.parametrize("N,T", [(3, 13), (2, 64)])
def test_one_constant_tile_is_the_logits_and_mask_scatter(N, T):
    from mi355.lib import lib
    z = R.normal_maps((N, T, T), 7 + T)
    one = np.ones(T, np.float32)
    got = _gpu_blend(z, N, T, T, T, [0], [0], one, one, 0)
    assert np.array_equal(_bits(got["mean"]), _bits(z)) and (got["spread"] == 0).all() and (got["cover"] == 1).all()
    out = torch.zeros(N, T * T, dtype=torch.uint8, device=DEV)
    lib.mi355_mask_scatter(torch.from_numpy(z.copy()).to(DEV), torch.arange(N, dtype=torch.int32, device=DEV), N, T * T, 0.5, out)
    assert np.array_equal(out.cpu().numpy().reshape(got["mask"].shape), got["mask"])


@pytest.mark.parametrize("prob", [0, 1])
@pytest.mark.parametrize("skip", ["spread", "cover", "mask"])
def test_blend_skips_a_null_output_and_leaves_the_others_alone(skip, prob):
    z, ys, xs, w, _, _ = _blend_case(2, 37, 45, 16, 0.25, "gaussian")
    full = _gpu_blend(z, 2, 37, 45, 16, ys, xs, w, w, prob, runs=1)
    part = _gpu_blend(z, 2, 37, 45, 16, ys, xs, w, w, prob, skip=(skip,), runs=1)
    for k in ("mean", "spread", "cover", "mask"):
        if k != skip:
            assert np.array_equal(part[k].view(np.uint8), full[k].view(np.uint8)), k
    none = _gpu_blend(z, 2, 37, 45, 16, ys, xs, w, w, prob, skip=("spread", "cover", "mask"), runs=1)
    assert np.array_equal(_bits(none["mean"]), _bits(full["mean"]))


@pytest.mark.parametrize("N,H,W,T,overlap", [(2, 37, 45, 16, 0.25), (3, 96, 112, 64, 0.5)])
def test_blend_scatters_the_mask_rows_through_idx(N, H, W, T, overlap):
    z, ys, xs, w, ref, _ = _blend_case(N, H, W, T, overlap, "gaussian")
    idx = [5, 0, 3][:N]
    got = _gpu_blend(z, N, H, W, T, ys, xs, w, w, 0, idx=idx, rows=7)
    plain = _gpu_blend(z, N, H, W, T, ys, xs, w, w, 0, runs=1)
    for n, r in enumerate(idx):
        assert np.array_equal(got["mask"][r], plain["mask"][n])
    for r in set(range(7)) - set(idx):
        assert (got["mask"][r] == SENTINEL).all()
    assert np.array_equal(_bits(got["mean"]), _bits(ref["mean"]))


@pytest.mark.parametrize("prob", [0, 1])
def test_blend_into_misaligned_buffers_takes_the_scalar_path_to_the_same_bytes(prob):
    z, ys, xs, w, _, _ = _blend_case(3, 96, 112, 64, 0.5, "gaussian")                    # T, W and the starts are multiples of 4
    a, b = _gpu_blend(z, 3, 96, 112, 64, ys, xs, w, w, prob, runs=1), _gpu_blend(z, 3, 96, 112, 64, ys, xs, w, w, prob, shift=4)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_blend_threshold_other_than_one_half():
    z, ys, xs, w, _, _ = _blend_case(2, 37, 45, 16, 0.25, "gaussian")
    for prob in (0, 1):
        ref = R.blend_ref(z, 2, 37, 45, 16, ys, xs, w, w, prob, thr=0.8)
        got = _gpu_blend(z, 2, 37, 45, 16, ys, xs, w, w, prob, thr=0.8)
        _check_mask(got, ref, 2 * 37 * 45)
        assert 0 < (got["mask"] == 255).mean() < 0.45
        assert (got["mask"] == 255).sum() < (_gpu_blend(z, 2, 37, 45, 16, ys, xs, w, w, prob, runs=1)["mask"] == 255).sum()


def test_bad_arguments_are_refused_and_touch_nothing():
    from mi355.lib import lib
    N, C, H, W, T = 2, 3, 37, 45, 16
    ys, xs = _host(R.tile_starts(H, T, 0.25)), _host(R.tile_starts(W, T, 0.25))
    x, tiles = torch.zeros(N, C, H, W, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV)
    z, w = torch.zeros(N * 12, T, T, device=DEV), torch.ones(T, device=DEV)
    dst = Guarded(5 * C * T * T)
    outs = {"mean": Guarded(N * H * W), "spread": Guarded(N * H * W), "cover": Guarded(H * W, torch.uint8), "mask": Guarded(N * H * W, torch.uint8)}
    good_g = dict(src=x, N=N, C=C, H=H, W=W, T=T, ys=ys, Py=3, xs=xs, Px=4, tiles=tiles, M=5, dst=dst.t)
    good_b = dict(z=z, N=N, H=H, W=W, T=T, ys=ys, Py=3, xs=xs, Px=4, wy=w, wx=w, prob=0, thr=0.5, idx=None, mean=outs["mean"].t,
                  spread=outs["spread"].t, cover=outs["cover"].t, mask=outs["mask"].t)
    bad_starts = [{"xs": _host([0, 8, 12, 29])}, {"xs": _host([0, 12, 24, 28])}, {"xs": _host([0, 12, 12, 29])}, {"ys": _host([0, 4, 21])},
                  {"ys": _host([0, 12, 20])}, {"ys": _host([0, 21, 12])}, {"ys": _host([1, 12, 21])}, {"ys": None}, {"xs": None},
                  {"Py": 0}, {"Px": 65}]
    for kw in [{"T": 0}, {"T": -1}, {"T": 38}, {"T": 46, "H": 64}, {"M": 0}, {"N": 0}, {"C": 0}, {"src": None}, {"tiles": None}, {"dst": None},
               {"dst": x}] + bad_starts:
        with pytest.raises(RuntimeError, match="tile_gather_f32"):
            lib.mi355_tile_gather_f32(*{**good_g, **kw}.values())
    for kw in [{"T": 0}, {"T": 38}, {"T": 46, "H": 64}, {"N": 0}, {"z": None}, {"wy": None}, {"wx": None}, {"mean": None}] + bad_starts:
        with pytest.raises(RuntimeError, match="tile_blend"):
            lib.mi355_tile_blend(*{**good_b, **kw}.values())
    torch.cuda.synchronize()
    assert dst.intact() and dst.untouched() and all(g.intact() and g.untouched() for g in outs.values())
    assert not bool(x.any()) and not bool(z.any())
    lib.mi355_tile_gather_f32(*good_g.values())                  # and the calls they were derived from are good
    lib.mi355_tile_blend(*good_b.values())
    torch.cuda.synchronize()
    assert dst.intact() and bool((dst.t == 0).all()) and all(g.intact() for g in outs.values()) and bool((outs["cover"].t >= 1).all())


# ---- end to end (the models and weights tests/test_gpu_tta.py builds; its helpers, copied) ---------------------------------------
def _he(sd):
    """default init has gain 1/sqrt(3); eval-mode BN with fresh running statistics is the identity, so rescale the convolutions to He
    gain to keep activations O(1) through the depth"""
    for v in sd.values():
        if v.dim() == 4:
            v.mul_(6 ** 0.5)
    return sd


@functools.lru_cache(maxsize=None)
def _models():
    """ResNet18 + AttentionUNet, fp32 compute, on the device in eval mode, the 16 x 3 x 64 x 64 batch they were centred on and a
    16 x 3 x 96 x 112 batch of the same kind"""
    from models.classification_models.ResNet import ResNet18
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils.helpers import add_dropout_to_fc
    cls_sd = _he(nets.default_init_state("ResNet18", seed=3, num_classes=3, head_dropout=True))
    seg_sd = _he(nets.default_init_state("AttentionUNet", seed=4))
    x = torch.randn(16, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():        # centre the logits over the batch: the three classes all occur
        cls_sd["fc.1.bias"] = cls_sd["fc.1.bias"] - nets.NETS["ResNet18"]({k: v.clone() for k, v in cls_sd.items()}, x, False).mean(0)
    sm = AttentionUNet()
    sm.load_state_dict(seg_sd)
    sm.compute_dtype = torch.float32
    cm = ResNet18(num_classes=3)
    add_dropout_to_fc(cm)
    cm.load_state_dict(cls_sd)
    cm.compute_dtype = torch.float32
    big = torch.randn(16, 3, 96, 112, generator=torch.Generator().manual_seed(6))
    return cm.to(DEV).eval(), sm.to(DEV).eval(), x.to(DEV), big.to(DEV)


def test_segmenter_with_one_tile_is_the_model():
    from utils.sliding import SlidingWindowSegmenter
    _, sm, x, _ = _models()
    x = x[:4].contiguous()
    with torch.no_grad():
        want = sm(x).float().reshape(4, 64, 64)
    seg = SlidingWindowSegmenter(sm, tile=64, overlap=0.5, weighting="constant", merge="logit", batch=4)
    r = seg(x)
    assert torch.equal(r["mean"].view(torch.int32), (want + 0.0).view(torch.int32))
    assert torch.equal(seg.tile_logits(x).view(torch.int32), want.view(torch.int32))
    assert not sm.training and bool((r["cover"] == 1).all()) and bool((r["spread"] == 0).all())


@functools.lru_cache(maxsize=None)
def _tile_logits():
    """the 30 tile logit maps of the first five 96 x 112 images (tile 64, overlap 0.5, chunks of 4), computed once, read-only"""
    from utils.sliding import SlidingWindowSegmenter
    _, sm, _, big = _models()
    x = big[:5].contiguous()
    z = SlidingWindowSegmenter(sm, tile=64, overlap=0.5, batch=4).tile_logits(x)
    return x, z


@pytest.mark.parametrize("weighting", ["constant", "gaussian"])
def test_segmenter_on_a_padded_last_chunk_is_the_restatement_of_its_tile_logits(weighting):
    from utils.sliding import SlidingWindowSegmenter, blend_tiles, gather_tiles
    _, sm, _, _ = _models()
    x, z = _tile_logits()
    seg = SlidingWindowSegmenter(sm, tile=64, overlap=0.5, weighting=weighting, merge="logit", batch=4)
    assert seg.grid(96, 112) == ([0, 32], [0, 32, 48]) and tuple(z.shape) == (30, 64, 64)      # 2 x 3 tiles, 30 tiles: 8 chunks
    assert torch.equal(seg.tile_logits(x).view(torch.int32), z.view(torch.int32))
    with torch.no_grad():                                                                     # a full chunk and the padded last one
        first = sm(gather_tiles(x, 64, 0.5, [0, 1, 2, 3])).float().reshape(4, 64, 64)
        last = sm(gather_tiles(x, 64, 0.5, [28, 29, 0, 0])).float().reshape(4, 64, 64)
    assert torch.equal(first.view(torch.int32), z[:4].view(torch.int32)) and torch.equal(last[:2].view(torch.int32), z[28:].view(torch.int32))
    r, b = seg(x), blend_tiles(z, x.shape, 64, 0.5, weighting, "logit")
    for k in ("mean", "spread", "cover", "mask"):
        assert torch.equal(r[k].view(torch.uint8), b[k].view(torch.uint8)), k
    zn = z.cpu().numpy()
    w = R.window_weights(64, weighting)
    ref = R.blend_ref(zn, 5, 96, 112, 64, [0, 32], [0, 32, 48], w, w, 0)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    exact = R.blend_ref(zn, 5, 96, 112, 64, [0, 32], [0, 32, 48], w, w, 0, exact=True)
    err = np.abs(got["mean"].astype(np.float64) - exact["mean"]).max()
    print(f"{weighting}: |mean - fp64| {err:.3e} (bound {R.blend_logit_bound(6, ref['vmax']):.3e}, max |z| {ref['vmax']:.3f})")
    assert err <= R.blend_logit_bound(6, ref["vmax"])                                          # the stated bound (Gaussian weighting) ...
    for k in ("mean", "spread"):                                                              # ... and in fact the bits, both weightings
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    assert np.array_equal(got["cover"], ref["cover"]) and ref["cover"].max() == 6          # two rows of tiles, three columns
    _check_mask(got, ref, 5 * 96 * 112)
    p = SlidingWindowSegmenter(sm, tile=64, overlap=0.5, weighting=weighting, merge="prob", batch=4)(x)
    refp = R.blend_ref(zn, 5, 96, 112, 64, [0, 32], [0, 32, 48], w, w, 1)
    assert (np.abs(p["mean"].cpu().numpy().astype(np.float64) - refp["mean"]) <= R.blend_prob_bound(refp["cover"].astype(np.float64))[None]).all()


def test_segmenter_refuses_train_mode_and_small_images():
    from utils.sliding import SlidingWindowSegmenter
    _, sm, x, _ = _models()
    seg = SlidingWindowSegmenter(sm, tile=64, batch=4)
    sm.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            seg(x[:1])
        with pytest.raises(ValueError, match="eval"):
            seg.tile_logits(x[:1])
        assert sm.training                               # left as found
    finally:
        sm.eval()
    with pytest.raises(ValueError, match="tile"):
        SlidingWindowSegmenter(sm, tile=128, batch=4)(x[:1])
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="together"):
        seg(x[:1], idx=idx)


def _counts_np(p, t):
    P, T = p > 0.5, t > 0.5
    f = lambda a: a.reshape(a.shape[0], -1).sum(1).astype(np.float64)
    return np.stack([f(P & T), f(P), f(T), f(P == T)], 1)


def test_tester_segmentation_with_the_wrapper(capsys):
    from utils import tester
    from utils.sliding import SlidingWindowSegmenter
    _, sm, _, big = _models()
    g = torch.Generator().manual_seed(9)
    loader = [(big[0:3].contiguous(), (torch.rand(3, 1, 96, 112, generator=g) < 0.4).float()),
              (big[3:5].contiguous(), (torch.rand(2, 1, 96, 112, generator=g) < 0.4).float())]
    seg = SlidingWindowSegmenter(sm, tile=64, overlap=0.5, weighting="gaussian", merge="logit", batch=4)
    got = tester.evaluate_segmentation_model(seg, loader, DEV, "AttentionUNet")
    text = capsys.readouterr().out
    per_sample, seam = [], []
    for images, masks in loader:
        r = {k: v.cpu().numpy() for k, v in seg(images).items()}
        prob = R.sigmoid64(r["mean"])
        assert not (np.abs(prob - 0.5) < R.SIGMOID_ERR).any()
        for c in _counts_np(prob, masks.numpy()[:, 0]):
            per_sample.append(tester._metrics_from_counts(c, 96 * 112))
        over = r["cover"] > 1
        assert 0 < over.sum() < 96 * 112
        seam.extend(r["spread"][:, over].astype(np.float64).mean(1))
    keys = ("iou", "dice", "pixel_accuracy", "precision", "recall", "f1")
    for k in keys:
        assert abs(got[k] - np.mean([m[k] for m in per_sample])) <= 1e-4, k
    assert got["sw_tiles"] == 6 and len(seam) == 5 and np.mean(seam) > 0
    assert abs(got["sw_seam_spread"] - np.mean(seam)) <= 1e-9 * np.mean(seam)
    assert set(got) == set(keys) | {"sw_tiles", "sw_seam_spread"}
    assert text.count("Sliding window:") == 1 and "6 tiles of 64 px" in text
    plain = tester.evaluate_segmentation_model(sm, loader, DEV, "AttentionUNet")
    assert set(plain) == set(keys) and "Sliding" not in capsys.readouterr().out               # no wrapper: today's keys and lines
    both = tester.evaluate_segmentation_model(SlidingWindowSegmenter(sm, tile=64, merge="prob", batch=4), loader, DEV, "AttentionUNet",
                                              surface=True, auc=True)
    assert set(both) == set(keys) | set(tester.SURFACE_KEYS) | {"surface_samples", "pixel_auroc", "pixel_ap", "auc_samples", "sw_tiles",
                                                                "sw_seam_spread"}
    assert 0 < both["sw_seam_spread"] < 1                                                      # probabilities


def test_all_models_hands_the_segmenters_on_wrapped_and_only_then(tmp_path, capsys):
    """test_all_models through the segmentation path with a loader and a weights directory: ``auc`` alone, ``sliding`` alone, both,
    neither — each adds its own keys and lines and nothing else"""
    from torch.utils.data import DataLoader, TensorDataset
    from utils import tester
    from utils.sliding import SlidingWindowSegmenter
    _, sm, _, big = _models()
    seg_dir, cls_dir = tmp_path / "seg", tmp_path / "cls"
    seg_dir.mkdir()
    cls_dir.mkdir()
    torch.save(sm.state_dict(), seg_dir / "AttentionUNet_best_loss.pt")
    g = torch.Generator().manual_seed(10)
    dl = DataLoader(TensorDataset(big[:4].cpu(), (torch.rand(4, 1, 96, 112, generator=g) < 0.4).float()), batch_size=2)
    keys = {"iou", "dice", "pixel_accuracy", "precision", "recall", "f1"}
    auc_keys, sw_keys = {"pixel_auroc", "pixel_ap", "auc_samples"}, {"sw_tiles", "sw_seam_spread"}
    run = lambda **kw: tester.test_all_models("cuda", 8, seg_loader=dl, cls_weights_dir=str(cls_dir), seg_weights_dir=str(seg_dir), **kw)
    sliding = (64, 0.5, "gaussian")
    for kw, extra in (({}, set()), ({"auc": True}, auc_keys), ({"sliding": sliding}, sw_keys), ({"sliding": sliding, "auc": True}, auc_keys | sw_keys),
                      ({"sliding": sliding, "surface": True}, sw_keys | set(tester.SURFACE_KEYS) | {"surface_samples"})):
        res = run(**kw)
        out = capsys.readouterr().out
        assert set(res) == {"AttentionUNet"} and set(res["AttentionUNet"]) == keys | extra, kw
        assert ("Pixel AUROC / AP:" in out) == ("auc" in kw) and ("Sliding window:" in out) == ("sliding" in kw), kw
        if kw == {"sliding": sliding}:
            windowed = res["AttentionUNet"]
    from utils.helpers import get_seg_model
    fresh = get_seg_model("AttentionUNet")                                                   # what test_all_models builds: the default compute type
    fresh.load_state_dict(sm.state_dict())
    direct = tester.evaluate_segmentation_model(SlidingWindowSegmenter(fresh.to(DEV), 64, 0.5, "gaussian", batch=4), dl, torch.device(DEV), "x")
    assert direct["sw_tiles"] == windowed["sw_tiles"] == 6 and all(abs(direct[k] - windowed[k]) < 1e-9 for k in direct)
    with pytest.raises(ValueError, match="sliding together with tta"):
        run(sliding=sliding, tta="hflip")


def test_pipeline_with_one_tile_is_the_plain_pipeline():
    from utils.pipeline import JointPipeline
    cm, sm, x, _ = _models()
    plain = JointPipeline(cm, sm, device=DEV, bucket=16).predict(x)                            # one padded launch of 16 on both sides
    one = JointPipeline(cm, sm, device=DEV, bucket=16, sliding=(64, 0.5, "constant")).predict(x, x_seg=x)
    assert 2 <= int(plain["segmented"].sum()) <= 14
    assert set(plain) == {"pred", "confidence", "masks", "segmented"}                         # sliding=None: today's outputs
    assert set(one) == set(plain) | {"seam_spread"}
    for k in ("pred", "masks", "segmented"):
        assert torch.equal(plain[k], one[k]), k
    assert torch.equal(plain["confidence"].view(torch.int32), one["confidence"].view(torch.int32))
    assert bool(one["masks"].any()) and bool((one["seam_spread"] == 0).all())
    same = JointPipeline(cm, sm, device=DEV, bucket=16, sliding=(64, 0.5, "constant")).predict(x)          # x_seg defaults to x
    assert torch.equal(same["masks"], one["masks"])


def test_pipeline_masks_at_the_segmenters_resolution_are_the_wrappers():
    from utils.pipeline import JointPipeline
    from utils.postprocess import MaskPostprocess
    from utils.sliding import SlidingWindowSegmenter
    cm, sm, x, big = _models()
    pipe = JointPipeline(cm, sm, device=DEV, bucket=4, sliding=(64, 0.5, "gaussian"))
    r = pipe.predict(x, x_seg=big)
    plain = JointPipeline(cm, sm, device=DEV, bucket=4).predict(x)
    assert torch.equal(r["pred"], plain["pred"]) and torch.equal(r["segmented"], plain["segmented"])      # the classifier's path
    assert torch.equal(r["confidence"].view(torch.int32), plain["confidence"].view(torch.int32))
    assert r["masks"].shape == (16, 96, 112) and r["masks"].dtype == torch.uint8 and r["seam_spread"].shape == (16, 96, 112)
    rows = torch.nonzero(r["segmented"]).flatten()
    assert 2 <= len(rows) <= 14
    w = SlidingWindowSegmenter(sm, 64, 0.5, "gaussian", "logit", 0.5, batch=4)(big[rows].contiguous())
    assert torch.equal(r["masks"][rows], w["mask"]) and torch.equal(r["seam_spread"][rows].view(torch.int32), w["spread"].view(torch.int32))
    assert not bool(r["masks"][~r["segmented"]].any()) and bool((r["seam_spread"][~r["segmented"]] == 0).all())
    assert bool(r["masks"][rows].any()) and float(r["seam_spread"][rows].sum()) > 0
    clean = JointPipeline(cm, sm, device=DEV, bucket=4, sliding=(64, 0.5, "gaussian"), postprocess=MaskPostprocess(min_area=4)).predict(x, x_seg=big)
    assert torch.equal(clean["masks_raw"], r["masks"]) and clean["masks"].shape == (16, 96, 112)
    with pytest.raises(ValueError, match="at least the tile"):
        JointPipeline(cm, sm, device=DEV, bucket=4, sliding=(128, 0.5, "gaussian")).predict(x, x_seg=big)
    with pytest.raises(ValueError, match="x_seg"):
        pipe.predict(x, x_seg=big[:3])


def test_process_images_overlays_at_the_file_size_and_names_the_tile_grid(tmp_path):
    from PIL import Image
    from utils.pipeline import CLASSES, JointPipeline
    cm, sm, _, _ = _models()
    rng = np.random.RandomState(2)
    paths = []
    for i in range(6):
        yy, xx = np.mgrid[0:80, 0:96]
        img = (127 + 80 * np.sin(xx / (9.0 + i)) * np.cos(yy / (6.0 + i)))[..., None] + rng.randint(-10, 10, (80, 96, 3))
        paths.append(str(tmp_path / f"x{i}.png"))
        Image.fromarray(img.clip(0, 255).astype(np.uint8), "RGB").save(paths[-1])
    line = "\nSliding window: 2 x 2 tiles of 64 px on 96 x 96 (overlap 0.5, gaussian weights)."
    segmented = masks = 0
    for positive in CLASSES:                             # whichever class the files get: each sample is segmented under one of the three
        pipe = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive, sliding=(64, 0.5, "gaussian"), seg_size=96)
        plain = JointPipeline(cm, sm, device=DEV, bucket=4, positive=positive)
        for (pred, conf, img, text), base in zip(pipe.process_images(paths, size=64), plain.process_images(paths, size=64)):
            assert "Sliding" not in base[3] and (pred, conf) == base[:2]
            if pred == positive:
                assert text.count(line) == 1 and img.shape == (80, 96, 3) and img.dtype == np.uint8
                assert text.replace(line, "") == base[3]
                segmented += 1
            else:
                assert "Sliding" not in text and img is None and text == base[3]
        masks += sum(1 for _, _, m in pipe.process_files(paths, size=64) if m is not None and tuple(m.shape) == (96, 96))
    assert segmented == 6 == masks
    with pytest.raises(ValueError, match="seg_size"):
        JointPipeline(cm, sm, device=DEV, seg_size=96).process_images(paths, size=64)
    with pytest.raises(ValueError, match="at least the tile"):
        JointPipeline(cm, sm, device=DEV, sliding=(64, 0.5, "gaussian"), seg_size=48).process_images(paths, size=64)
