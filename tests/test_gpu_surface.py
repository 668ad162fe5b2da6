"""-m gpu: the surface-distance metrics (csrc/surface.hip, utils.tester.surface_metrics_batch, test_segmentation_model(surface=True))
on the device against the brute-force restatement tests/surface_ref.py (pinned to scipy.ndimage and to its fixture on the CPU,
tests/test_surface_cpu.py).

Every input is judged through the C ABI and through surface_metrics_batch.  The eight integers per sample must EQUAL the
restatement's.  The two fp64 sums and the final distances must be within 1e-9 relative: a sum of n <= 2 H W non-negative terms
in fp64 is off by at most n 2^-53 relative whatever the order (<= 1.5e-11 at 256^2, <= 2.4e-10 at 1024^2), each term is one correctly
rounded square root, and the percentile's interpolation differs from the restatement's by roundings only."""
import numpy as np
import pytest
import torch

import surface_ref as R
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-9
_REF = {}


def ref(key, P, T, q=95, tol2=4):
    """restatement of one batch of boolean masks, computed once per key and never modified"""
    if key not in _REF:
        out_i, out_d = R.raw(P, T, q, tol2)
        out_i.setflags(write=False)
        out_d.setflags(write=False)
        _REF[key] = (out_i, out_d)
    return _REF[key]


def abi(pred, target, is_logit=False, thr=0.5, q=95, tol2=4):
    B, H, W = pred.shape
    n = lib.raw("mi355_surface_ws_ints")(B, H, W)
    assert n > 0, lib.raw("mi355_last_error")()
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    out_i = torch.full((B, 8), -7, dtype=torch.int32, device=DEV)
    out_d = torch.full((B, 2), -7.0, dtype=torch.float64, device=DEV)
    lib.mi355_surface_distances(pred, target, B, H, W, 1 if is_logit else 0, thr, q, tol2, ws, n, out_i, out_d)
    torch.cuda.synchronize()
    return out_i, out_d


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(DEV)


def check(key, P, T, q=95, tolerance=2.0, spacing=1.0):
    from utils import tester
    tol2 = R.tol2_of(tolerance, spacing)
    want_i, want_d = ref((key, q, tol2), P, T, q, tol2)
    got_i, got_d = abi(dev(P), dev(T), False, 0.5, q, tol2)
    gi, gd = got_i.cpu().numpy(), got_d.cpu().numpy()
    err = np.abs(gd - want_d).max() / max(want_d.max(), 1e-300)
    print(f"{key} q={q} tol2={tol2}: out_i {'==' if np.array_equal(gi, want_i) else '!='} ref, out_d rel err {err:.2e}, n_P {want_i[:, 0].tolist()}")
    assert np.array_equal(gi, want_i), (key, gi.tolist(), want_i.tolist())
    np.testing.assert_allclose(gd, want_d, rtol=RTOL, atol=0, err_msg=str(key))
    res = tester.surface_metrics_batch(dev(P)[:, None], dev(T)[:, None], False, 0.5, spacing, q, tolerance)
    assert torch.equal(res["out_i"], got_i) and torch.equal(res["out_d"], got_d), key
    want = R.values(want_i, want_d, spacing, q)
    for k in R.NAMES:
        assert res[k].is_cuda and res[k].dtype == torch.float64 and res[k].shape == (len(P),)
        np.testing.assert_allclose(res[k].cpu().numpy(), want[k], rtol=RTOL, atol=0, err_msg=f"{key} {k}")      # NaN == NaN here
    return got_i, got_d


def kinds(B, H, W, seed):
    """the mask kinds at one shape: {kind: (P, T)} boolean [B, H, W]"""
    rng = np.random.RandomState(seed)
    ell = lambda cy, cx, ry, rx: R.ellipse(H, W, cy * H, cx * W, max(ry * H, 0.6), max(rx * W, 0.6))
    out = {"noise": (rng.rand(B, H, W) < 0.5, rng.rand(B, H, W) < 0.5)}
    P = np.stack([ell(0.45 + 0.03 * b, 0.5, 0.3, 0.25) for b in range(B)])
    T = np.stack([ell(0.5, 0.45 + 0.04 * b, 0.27, 0.3) | ell(0.1, 0.85, 0.05, 0.05) for b in range(B)])      # with a stray blob
    out["ellipses"] = (P, T)
    out["edge"] = (np.stack([ell(0.0, 0.1 * b, 0.4, 0.35) for b in range(B)]), np.stack([ell(0.9, 1.0, 0.45, 0.3) for b in range(B)]))
    out["all_foreground"] = (np.ones((B, H, W), dtype=bool), np.stack([np.ones((H, W), dtype=bool) if b % 2 else ell(0.5, 0.5, 0.3, 0.3)
                                                                       for b in range(B)]))
    P, T = np.zeros((B, H, W), dtype=bool), np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        P[b, rng.randint(H), rng.randint(W)] = True
        T[b, rng.randint(H), rng.randint(W)] = True
    out["single_pixel"] = (P, T)
    same = rng.rand(B, H, W) < 0.6
    same[:, 0, 0] = True
    out["same"] = (same, same.copy())
    return out


# odd and narrower than a wavefront; one row; one column; two samples; wider / taller than one 256-thread block, no multiple of 64
SHAPES = [(3, 17, 13), (1, 1, 9), (1, 8, 1), (2, 64, 64), (1, 40, 300), (1, 300, 40)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_mask_kind_at_the_small_shapes(shape):
    for kind, (P, T) in kinds(*shape, seed=sum(shape)).items():
        check((shape, kind), P, T)
    P, T = kinds(*shape, seed=sum(shape))["noise"]
    for q, tol in ((0, 0.0), (100, 1.0), (50, 3.0), (37, 2.0)):
        check((shape, "noise"), P, T, q, tol)
    check((shape, "noise", "spacing"), P, T, 95, 1.5, 0.7)


def _tester_batch():
    """(8, 256, 256), every kind in one batch: noise (a 128 x 128 window of it: the restatement forms every pair), the ellipses of
    oracle.train.synthetic_batch against shifted ones, masks cut by the frame, all-foreground, single pixels, P == T, a stray blob"""
    H = W = 256
    rng = np.random.RandomState(256)
    P, T = np.zeros((8, H, W), dtype=bool), np.zeros((8, H, W), dtype=bool)
    P[0, 60:188, 100:228], T[0, 60:188, 100:228] = rng.rand(128, 128) < 0.5, rng.rand(128, 128) < 0.5
    m = otrain.synthetic_batch(4, 256, seed=3)[1][:, 0].numpy() > 0.5
    P[1], T[1], P[2], T[2] = m[0], m[1], m[2], np.roll(m[2], (5, -9), (0, 1))
    P[3], T[3] = R.ellipse(H, W, 0, 30, 90, 70), R.ellipse(H, W, 255, 255, 60, 120)
    P[4], T[4] = True, m[3]
    P[5, 3, 250], T[5, 200, 7] = True, True
    P[6] = T[6] = m[3]
    P[7], T[7] = m[0] | R.ellipse(H, W, 20, 230, 4, 6), m[0]
    return P, T


def test_the_testers_batch_and_reproducibility():
    P, T = _tester_batch()
    got_i, got_d = check("tester_batch", P, T)
    p, t = dev(P), dev(T)
    for _ in range(3):
        i, d = abi(p, t)
        assert torch.equal(i, got_i) and torch.equal(d, got_d)


def test_logits_and_probabilities_of_the_same_masks_agree():
    """every value at least 0.5 away from the threshold (0 in logits, 0.5 in probabilities)"""
    P, T = _tester_batch()
    want_i, want_d = ref(("tester_batch", 95, 4), P, T)
    g = torch.Generator().manual_seed(9)
    sign = torch.from_numpy(np.where(P, 1.0, -1.0).astype(np.float32))
    logits = (sign * (0.5 + 4.0 * torch.rand(P.shape, generator=g))).to(DEV)
    li, ld = abi(logits, dev(T), True)
    pi, pd = abi(dev(P), dev(T), False)
    assert torch.equal(li, pi) and torch.equal(ld, pd)
    assert np.array_equal(li.cpu().numpy(), want_i)
    soft = torch.sigmoid(logits)                       # 0.62 .. 0.99 inside, 0.01 .. 0.38 outside
    si, sd = abi(soft, dev(T), False)
    assert torch.equal(si, pi) and torch.equal(sd, pd)
    hi, hd = abi(dev(P) * 0.4 + 0.45, dev(T), False, 0.65)      # 0.85 / 0.45 around another threshold: the target is cut by it too
    assert torch.equal(hi, pi) and torch.equal(hd, pd)


@pytest.mark.parametrize("side,d2", [(256, 130050), (1024, 2093058)])
def test_opposite_corners_reach_the_largest_distance(side, d2):
    P, T = np.zeros((1, side, side), dtype=bool), np.zeros((1, side, side), dtype=bool)
    P[0, 0, 0], T[0, -1, -1] = True, True
    got_i, got_d = check(("corners", side), P, T)
    assert got_i.cpu().tolist() == [[1, 1, d2, d2, d2, d2, 0, 0]]
    assert abs(float(got_d[0, 0]) - np.sqrt(d2)) <= RTOL * np.sqrt(d2)
    check(("corners", side), P, T, 50, float(side) * 1.5)          # r = 50: the interpolation between two equal values; all within


def test_the_largest_image_with_real_contours():
    """1024 x 1024: 64-row column segments, four 256-pixel spans per row, every one of the 16 segments crossed"""
    H = W = 1024
    P = (R.ellipse(H, W, 500, 520, 420, 300) | R.ellipse(H, W, 40, 980, 12, 20))[None]
    T = (R.ellipse(H, W, 530, 500, 400, 330) & ~R.ellipse(H, W, 530, 500, 100, 80))[None]      # a ring: two contours
    check("largest", P, T)


def test_empty_masks_in_a_batch_and_in_the_loop(capsys):
    from torch.utils.data import DataLoader, TensorDataset
    from utils import tester
    H, W = 20, 24
    e = R.ellipse(H, W, 9, 11, 5, 7)
    z = np.zeros((H, W), dtype=bool)
    P = np.stack([z, z, e, e, np.roll(e, 3, 1), z])
    T = np.stack([z, e, z, np.roll(e, 2, 0), e, z])
    got_i, got_d = check("empties", P, T)
    gi = got_i.cpu().numpy()
    n = int(e.sum() - (e & ~R.border(e)).sum())
    assert gi[0].tolist() == [0] * 8 and gi[1].tolist() == [0, n] + [0] * 6 and gi[2].tolist() == [n] + [0] * 7 and gi[3, 0] == n
    assert not got_d[:3].any()
    res = tester.surface_metrics_batch(dev(P), dev(T))
    assert res["surface_dice"].cpu().tolist()[0] == 1.0 and torch.isnan(res["hd95"]).cpu().tolist() == [False, True, True, False, False, False]

    class Logits(torch.nn.Module):          # the "images" are the logits
        def forward(self, x):
            return x

    logit = torch.from_numpy(np.where(P, 3.0, -3.0).astype(np.float32))[:, None]
    dl = DataLoader(TensorDataset(logit, torch.from_numpy(T.astype(np.float32))[:, None]), batch_size=4)
    avg = tester.test_segmentation_model(Logits(), dl, torch.device(DEV), "Logits", surface=True)
    out = capsys.readouterr().out
    want = R.metrics(P, T)
    ok = ~np.isnan(want["hausdorff"])
    assert avg["surface_samples"] == 4 == int(ok.sum()) and "(4 of 6 samples)" in out
    for k in R.NAMES:
        w = want[k][ok].mean() * (100.0 if k == "surface_dice" else 1.0)
        assert np.isfinite(avg[k]) and abs(avg[k] - w) <= RTOL * abs(w), (k, avg[k], w)
    # nothing defined at all: NaN averages, zero samples
    dl = DataLoader(TensorDataset(logit[1:3], torch.from_numpy(T.astype(np.float32))[1:3, None]), batch_size=2)
    avg = tester.test_segmentation_model(Logits(), dl, torch.device(DEV), "Logits", surface=True)
    capsys.readouterr()
    assert avg["surface_samples"] == 0 and all(np.isnan(avg[k]) for k in R.NAMES)


def test_single_sample_helper_and_error_paths():
    from utils import tester
    P, T = kinds(1, 17, 13, seed=5)["ellipses"]
    want = R.metrics(P, T, spacing=0.5, percentile=90, tolerance=1.0)
    for p, t in ((dev(P)[0], dev(T)[0]), (dev(P), dev(T)), (dev(P)[0].cpu(), dev(T)[0].cpu())):      # [H,W], [1,H,W], CPU tensors
        got = tester.calculate_surface_metrics(p, t, 0.5, 0.5, 90, 1.0)
        assert list(got) == list(R.NAMES)
        for k in R.NAMES:
            assert isinstance(got[k], float) and abs(got[k] - want[k][0]) <= RTOL * abs(want[k][0]), (k, got[k], want[k][0])
    with pytest.raises(ValueError, match="one-channel"):
        tester.surface_metrics_batch(torch.zeros(2, 2, 8, 8, device=DEV), torch.zeros(2, 2, 8, 8, device=DEV))
    with pytest.raises(RuntimeError, match="1024"):
        tester.surface_metrics_batch(torch.zeros(1, 1, 1025, 8, device=DEV), torch.zeros(1, 1, 1025, 8, device=DEV))
    with pytest.raises(ValueError, match="percentile"):
        tester.surface_metrics_batch(torch.zeros(1, 8, 8, device=DEV), torch.zeros(1, 8, 8, device=DEV), percentile=101)


def test_through_the_evaluation_loop(tmp_path, capsys):
    """AttentionUNet at the closed-form weights, fp32, two batches of four 64 x 64 ellipses: surface=True leaves the six overlap metrics
    and the text up to "F1 Score" as they are, the new keys are the restatement of that model's own logits, the CSV gains the columns."""
    from torch.utils.data import DataLoader, TensorDataset
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils import tester
    m = AttentionUNet()
    m.load_state_dict(nets.closed_form_state("AttentionUNet"))
    m.compute_dtype = torch.float32
    m = m.to(DEV)
    xs, ms = zip(*[otrain.synthetic_batch(4, 64, seed=s) for s in (31, 32)])
    x, mask = torch.cat(xs), torch.cat(ms)
    dl = DataLoader(TensorDataset(x, mask), batch_size=4)
    plain = tester.test_segmentation_model(m, dl, torch.device(DEV), "AttentionUNet")
    plain_text = capsys.readouterr().out
    surf = tester.test_segmentation_model(m, dl, torch.device(DEV), "AttentionUNet", surface=True)
    surf_text = capsys.readouterr().out
    keys = ["iou", "dice", "pixel_accuracy", "precision", "recall", "f1"]
    assert list(plain) == keys and list(surf) == keys + ["hausdorff", "hd95", "assd", "surface_dice", "surface_samples"]
    assert all(plain[k] == surf[k] for k in keys)
    cut = plain_text.index("F1 Score")
    end = plain_text.index("\n", cut)
    assert surf_text[:end] == plain_text[:end]
    extra = surf_text[end:].strip("\n").splitlines()
    assert [l.split(":")[0] for l in extra[:4]] == ["Hausdorff", "HD95", "ASSD", "Surface Dice @2px"] and extra[4] == "=" * 60 and len(extra) == 5
    m.eval()
    with torch.no_grad():
        logits = torch.cat([m(x[i:i + 4].to(DEV)) for i in (0, 4)]).float().cpu().numpy()
    assert np.abs(logits).min() > 1e-6, "a logit on the threshold: fp32 and fp64 sigmoids may cut it differently"
    want = R.metrics(logits, mask.numpy(), is_logit=True)
    ok = ~np.isnan(want["hausdorff"])
    assert surf["surface_samples"] == int(ok.sum())
    print("loop:", {k: surf[k] for k in R.NAMES}, "samples", surf["surface_samples"], "n_P", want["out_i"][:, 0].tolist())
    for k in R.NAMES:
        w = want[k][ok].mean() * (100.0 if k == "surface_dice" else 1.0) if ok.any() else float("nan")
        assert (np.isnan(w) and np.isnan(surf[k])) or abs(surf[k] - w) <= RTOL * abs(w), (k, surf[k], w)
    tester.save_results_to_csv({"AttentionUNet": plain}, str(tmp_path / "c.csv"), str(tmp_path / "s0.csv"))
    tester.save_results_to_csv({"AttentionUNet": surf}, str(tmp_path / "c.csv"), str(tmp_path / "s1.csv"))
    h0, h1 = (tmp_path / "s0.csv").read_text().splitlines()[0], (tmp_path / "s1.csv").read_text().splitlines()[0]
    assert h0 == "Model,iou,dice,pixel_accuracy,precision,recall,f1" and h1 == h0 + ",hausdorff,hd95,assd,surface_dice,surface_samples"
