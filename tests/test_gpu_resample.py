"""-m gpu: csrc/resample.hip through utils/resample.py and the ABI against the numpy restatement tests/resample_ref.py, which
tests/test_resample_cpu.py pins to the Random123 vectors, scikit-learn, scipy and a Fraction evaluation of DeLong's definition.  Every
integer is compared for equality, every double against the bound derived in resample_ref.py's docstring; the bootstrap weights used as
inputs are the restatement's own (uploaded), so a kernel is never checked with another kernel's output.  Shapes sit around the Philox
block (n = 5, 7), the wave and the scan step (257), the LDS histogram's limit and the tile of the sort."""
import math

import numpy as np
import pytest
import torch

import ranking_ref
import resample_ref as RR
from mi355.lib import lib
from utils import ranking, resample
from utils.tester import calculate_classification_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
T = lib.raw("mi355_segsort_tile")()
LDS_MAX = lib.raw("mi355_boot_counts_lds_max")()
GUARD, GUARD_BYTE, SENTINEL = 64, 0xA5, 0x5A


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def ulps(got, want):
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(np.asarray(want, dtype=np.float64)))


# ---- counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, R", [(n, R) for n in (1, 5, 7, 257) for R in (1, 3, 64)] + [(LDS_MAX, 2), (LDS_MAX + 1, 2)])
def test_counts_equal_the_restatement(n, R):
    seed = 0x1234567 << 20 | n                     # both halves of the key in use
    nbytes = (R + 1) * n * 4
    whole = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    whole[GUARD:GUARD + nbytes] = SENTINEL
    out = whole[GUARD:GUARD + nbytes].view(torch.int32)
    lib.mi355_boot_counts(seed, R, n, out)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == GUARD_BYTE).all()) and bool((whole[GUARD + nbytes:] == GUARD_BYTE).all()), "a guard band was written"
    got = out.cpu().numpy().reshape(R + 1, n)
    assert np.array_equal(got, RR.counts_ref(seed, R, n))
    assert (got[0] == 1).all() and (got.sum(1) == n).all()
    again = resample.bootstrap_counts(n, R, seed=seed, device=DEV)
    assert again.dtype == torch.int32 and np.array_equal(again.cpu().numpy(), got), "the same seed gave other bits"


@pytest.mark.parametrize("n", [7, 257, LDS_MAX + 1])
def test_counts_seeds_differ(n):
    a = resample.bootstrap_counts(n, 2, seed=1, device=DEV).cpu().numpy()
    b = resample.bootstrap_counts(n, 2, seed=2, device=DEV).cpu().numpy()
    c = resample.bootstrap_counts(n, 2, seed=1 << 32, device=DEV).cpu().numpy()      # the high half of the seed is the second key word
    assert not np.array_equal(a[1:], b[1:]) and not np.array_equal(a[1:], c[1:])
    assert np.array_equal(c, RR.counts_ref(1 << 32, 2, n))


# ---- rank --------------------------------------------------------------------------------------------------------------------------
def rank_case(kind, mode, seed):
    """-> (scores fp32 [S, n], target or None, labels or None, R)"""
    rng = np.random.RandomState(seed)
    S = 3 if mode == "labels" else 2
    n, R = {"continuous": (257, 3), "quantised": (257, 3), "constant": (2 * T + 3, 2), "single": (5, 64)}[kind]
    if kind == "continuous":
        scores = rng.rand(S, n).astype(np.float32)
    elif kind == "quantised":
        scores = (rng.randint(0, 4, (S, n)) / 4.0).astype(np.float32)
    elif kind == "constant":
        scores = np.full((S, n), 0.25, dtype=np.float32)
    else:
        scores = rng.rand(S, n).astype(np.float32)
    if mode == "labels":
        labels = rng.randint(0, S, n).astype(np.int32)
        if kind == "single":
            labels = np.array([0, 1, 1, 2, 2], dtype=np.int32)[rng.permutation(5)]      # class 0: a single positive
        return scores, None, labels, R
    target = (rng.rand(S, n) < 0.4).astype(np.float32)
    if kind == "single":
        target[:] = 0
        target[0, 3] = 1                           # segment 0: a single positive;
        target[1] = 1
        target[1, 1] = 0                           # segment 1: a single negative
    return scores, target, None, R


@pytest.mark.parametrize("mode", ["labels", "target"])
@pytest.mark.parametrize("kind", ["continuous", "quantised", "constant", "single"])
def test_rank_equals_the_restatement(kind, mode):
    scores, target, labels, R = rank_case(kind, mode, 11)
    S, n = scores.shape
    counts = RR.counts_ref(5, R, n)
    ref = RR.boot_rank_ref(scores, counts, target=target, labels=labels)
    if kind == "single":                           # asserted of the input: the seed gives both kinds of replicate for segment 0
        assert any(ref[r][0]["P"] == 0 for r in range(1, R + 1)) and any(ref[r][0]["P"] > 0 and ref[r][0]["N"] > 0 for r in range(1, R + 1))
    z = dev(scores)
    kw = {"target": dev(target)} if target is not None else {"labels": dev(labels)}
    runs = [resample.boot_rank_metrics(z, dev(counts), **kw) for _ in range(2)]
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in runs[0].items()}
    for k, v in runs[1].items():
        assert np.array_equal(v.cpu().numpy().view(np.uint8), got[k].view(np.uint8)), f"second run differs in {k}"
    assert got["pos"].shape == (R + 1, S)
    for r in range(R + 1):
        for s in range(S):
            e = ref[r][s]
            assert (int(got["pos"][r, s]), int(got["neg"][r, s]), int(got["u2"][r, s])) == (e["P"], e["N"], e["U2"]), (r, s)
            if e["P"] == 0:
                assert np.isnan(got["average_precision"][r, s]) and np.isnan(got["auroc"][r, s]), (r, s)
            else:
                assert abs(got["average_precision"][r, s] - e["ap"]) <= RR.ap_bound(n), (r, s, got["average_precision"][r, s], e["ap"])
                if e["N"] == 0:
                    assert np.isnan(got["auroc"][r, s]), (r, s)
                else:
                    assert got["auroc"][r, s] == e["auroc"], (r, s)
    plain = ranking.rank_metrics(z, **kw)          # row 0 is the point estimate of the existing kernel, to the bit
    for k in ("pos", "neg", "u2", "auroc", "average_precision"):
        assert np.array_equal(plain[k].cpu().numpy().view(np.uint8), got[k][0].view(np.uint8)), k


# ---- confusion ---------------------------------------------------------------------------------------------------------------------
def check_confusion(pred, labels, C, counts):
    cm, bad = resample.boot_confusion(dev(pred), dev(labels), C, dev(counts))
    want, want_bad = RR.confusion_ref(pred, labels, C, counts)
    cm_h = cm.cpu().numpy()
    assert cm.dtype == torch.int64 and np.array_equal(cm_h, want) and np.array_equal(bad.cpu().numpy(), want_bad)
    m = {k: v.cpu().numpy() for k, v in resample.classification_from_confusion(cm).items()}
    ok = (pred >= 0) & (pred < C) & (labels >= 0) & (labels < C)
    for r, w in enumerate(counts):
        p, y = RR.expand(w[ok], pred[ok], labels[ok])
        e = calculate_classification_metrics(p, y)
        for k in ("accuracy", "precision", "recall", "f1"):
            assert ulps(m[k][r], e[k]) <= 4 or m[k][r] == e[k], (r, k, m[k][r], e[k])
    return cm_h


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("n", [1, 257])
def test_confusion_exact(C, n):
    rng = np.random.RandomState(100 * C + n)
    labels = rng.randint(0, C, n).astype(np.int32)
    pred = np.where(rng.rand(n) < 0.7, labels, rng.randint(0, C, n)).astype(np.int32)
    check_confusion(pred, labels, C, RR.counts_ref(9, 3, n))


def test_confusion_with_a_lost_class_and_bad_ids():
    labels = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 2], dtype=np.int32)
    pred = np.array([0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 2], dtype=np.int32)
    counts = RR.counts_ref(3, 16, 12)
    assert (counts[1:, 11] == 0).any() and (counts[1:, 11] > 0).any()      # asserted of the input: class 2 is lost by some replicates
    cm = check_confusion(pred, labels, 3, counts)
    assert (cm[counts[:, 11] == 0][:, 2, :] == 0).all() and (cm[counts[:, 11] == 0][:, :, 2] == 0).all()
    pred[2], labels[5] = 3, -1                     # outside 0 .. C - 1: skipped and counted
    check_confusion(pred, labels, 3, counts)


def test_mcnemar():
    rng = np.random.RandomState(8)
    a, b = rng.rand(257) < 0.8, rng.rand(257) < 0.7
    m = resample.mcnemar(dev(a), dev(b))
    assert m["b"] == int((a & ~b).sum()) and m["c"] == int((~a & b).sum()) and m["p"] == RR.mcnemar_ref(m["b"], m["c"])
    assert m["table"] == [[int((~a & ~b).sum()), m["c"]], [m["b"], int((a & b).sum())]]
    same = resample.mcnemar(dev(a), dev(a))
    assert same["b"] == same["c"] == 0 and same["p"] == 1.0


# ---- sums --------------------------------------------------------------------------------------------------------------------------
def test_sums():
    rng = np.random.RandomState(21)
    M, n, R = 4, 257, 3
    v = np.empty((M, n))
    v[0] = rng.randint(0, 1024, n) / 1024.0        # dyadic: every product and every partial sum is exact
    v[1] = rng.randint(0, 1024, n) / 1024.0
    v[1, ::5] = np.nan
    v[2] = rng.randn(n)
    v[3] = rng.randn(n) * 1e3
    v[3, 7:40] = np.nan
    counts = RR.counts_ref(13, R, n)
    want, wt, mag = RR.sums_ref(v, counts)
    runs = [resample._boot_sums(dev(v), dev(counts)) for _ in range(2)]
    got, got_w = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert np.array_equal(got.view(np.int64), runs[1][0].cpu().numpy().view(np.int64)), "second run differs"
    assert np.array_equal(got_w, wt)
    assert np.array_equal(got[:, :2], want[:, :2]), "dyadic sums are exact"
    assert (np.abs(got - want) <= (n + 4) * U * mag).all(), np.abs(got - want) / mag
    means = resample.boot_means(dev(v), dev(counts)).cpu().numpy()
    assert np.array_equal(means, got / got_w)
    one = resample.boot_means(dev(np.full(5, np.nan)), dev(RR.counts_ref(0, 2, 5))).cpu().numpy()
    assert one.shape == (3, 1) and np.isnan(one).all()


# ---- interval ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 64, 8192])
def test_interval(R):
    rng = np.random.RandomState(R)
    reps = 0.5 + rng.rand(R + 1, 3)                # column 0: no NaN, 1: some, 2: all
    if R == 2:
        reps[1:, 0] = (0.6, 1.4)
    reps[1::3, 1] = np.nan
    reps[1:, 2] = np.nan
    lo_q, hi_q = (1.0 - 0.95) / 2.0, 1.0 - (1.0 - 0.95) / 2.0
    want = RR.interval_ref(reps, lo_q, hi_q)
    runs = [resample.interval(dev(reps), level=0.95) for _ in range(2)]
    got = {k: v.cpu().numpy() for k, v in runs[0].items()}
    for k, v in runs[1].items():
        assert np.array_equal(v.cpu().numpy().view(np.int64), got[k].view(np.int64)), f"second run differs in {k}"
    assert np.array_equal(got["point"].view(np.int64), reps[0].view(np.int64))
    assert np.array_equal(got["valid"], want[:, 5]) and want[2, 5] == 0 and want[0, 5] == R
    for k in range(3):
        v = reps[1:, k][~np.isnan(reps[1:, k])]
        if v.size == 0:
            assert all(np.isnan(got[name][k]) for name in ("mean", "se", "lo", "hi")), k
            continue
        assert ulps(got["lo"][k], np.nanquantile(reps[1:, k], lo_q, method="linear")) <= 1, k
        assert ulps(got["hi"][k], np.nanquantile(reps[1:, k], hi_q, method="linear")) <= 1, k
        assert abs(got["mean"][k] - want[k, 1]) <= (R + 4) * U * np.abs(v).mean(), k
        if v.size == 1:
            assert np.isnan(got["se"][k]) and got["lo"][k] == got["hi"][k] == v[0], k
        else:
            assert want[k, 2] >= 0.1 * abs(want[k, 1]), "asserted of the input: the spread is at least a tenth of the mean"
            assert abs(got["se"][k] - want[k, 2]) <= 8 * (R + 4) * U * want[k, 2], (k, got["se"][k], want[k, 2])


# ---- DeLong ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 257])
def test_delong(n):
    rng = np.random.RandomState(n)
    M, C = 2, 3
    labels = np.array([0, 0, 0, 1, 1, 1, 2], dtype=np.int32) if n == 7 else rng.randint(0, C, n).astype(np.int32)
    scores = (rng.randint(0, 8, (M, C, n)) / 8.0).astype(np.float32)       # ties
    scores[1] = np.where(rng.rand(C, n) < 0.5, scores[0], scores[1])      # the two models agree on half the samples
    want = RR.delong_ref(scores, labels)
    runs = [resample.delong(dev(scores), dev(labels)) for _ in range(2)]
    got = {k: v.cpu().numpy() for k, v in runs[0].items()}
    for k, v in runs[1].items():
        assert np.array_equal(v.cpu().numpy().view(np.uint8), got[k].view(np.uint8)), f"second run differs in {k}"
    assert np.array_equal(got["v2"], want["v2"])
    assert np.array_equal(np.stack([got["pos"], got["neg"], got["u2"]], -1), want["pnu"])
    undefined = np.isnan(want["cov"])
    assert np.array_equal(np.isnan(got["cov"]), undefined) and np.array_equal(np.isnan(got["var"]), np.isnan(want["var"]))
    assert undefined[2].all() if n == 7 else not undefined.any()           # n = 7: class 2 has a single member
    ok = ~undefined
    # asserted of the input: the two models agree on half the samples, so no covariance is a small remainder of cancelling products
    # (resample_ref.py: a sum errs relative to the sum of its terms' magnitudes; a quarter of that keeps it inside the bound)
    assert (np.abs(want["cov"])[ok] >= 0.25 * want["mag"][ok]).all(), np.abs(want["cov"]) / want["mag"]
    assert (np.abs(got["cov"] - want["cov"])[ok] <= 8 * (n + 4) * U * np.abs(want["cov"])[ok]).all(), (got["cov"], want["cov"])
    okv = ~np.isnan(want["var"])
    assert (np.abs(got["var"] - want["var"])[okv] <= 8 * (n + 4) * U * want["var"][okv]).all()
    for m in range(M):
        assert np.array_equal(got["var"][m].view(np.int64), np.array([got["cov"][c, m, m] for c in range(C)]).view(np.int64))
    auc = want["pnu"][..., 2] / (2.0 * want["pnu"][..., 0] * want["pnu"][..., 1])
    assert np.array_equal(got["auroc"], auc)
    t = resample.delong_test(dev(scores[0]), dev(scores[1]), dev(labels))
    for c in range(C):
        v = want["cov"][c, 0, 0] + want["cov"][c, 1, 1] - 2 * want["cov"][c, 0, 1]
        assert t[c]["auc_a"] == auc[0, c] and t[c]["auc_b"] == auc[1, c]
        if np.isnan(v):
            assert math.isnan(t[c]["z"]) and math.isnan(t[c]["p"])
        else:
            z = (auc[0, c] - auc[1, c]) / math.sqrt(v)
            assert abs(t[c]["z"] - z) <= 1e-9 * max(1.0, abs(z)) and abs(t[c]["p"] - math.erfc(abs(z) / math.sqrt(2))) <= 1e-9
    same = resample.delong_test(dev(scores[0]), dev(scores[0]), dev(labels))
    assert all(math.isnan(r["z"]) and r["auc_a"] == r["auc_b"] or math.isnan(r["auc_a"]) for r in same)


def test_delong_spans_tiles():
    """one tie group over more than two tiles of the sort and a second group behind it: the carried prefixes cross every tile border"""
    n = 2 * T + 3
    rng = np.random.RandomState(2)
    labels = rng.randint(0, 2, n).astype(np.int32)
    scores = np.full((1, 2, n), 0.5, dtype=np.float32)
    scores[0, :, -40:] = 0.75
    scores[0, 1] = scores[0, 1][rng.permutation(n)]
    want = RR.delong_ref(scores, labels)
    got = resample.delong(dev(scores), dev(labels))
    assert np.array_equal(got["v2"].cpu().numpy(), want["v2"])
    assert np.array_equal(torch.stack([got["pos"], got["neg"], got["u2"]], -1).cpu().numpy(), want["pnu"])
    assert (np.abs(got["var"].cpu().numpy() - want["var"]) <= 8 * (n + 4) * U * want["var"]).all()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def refused(name, *args):
    """the launcher returns MI355_ERR_ARG and leaves a message"""
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args] + [torch.cuda.current_stream().cuda_stream]
    rc = lib.raw(name)(*conv)
    msg = lib.raw("mi355_last_error")().decode()
    assert rc == -1 and name[len("mi355_"):] in msg, (name, rc, msg)


def test_argument_errors():
    n = 8
    buf = torch.full((4 * n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    keep = buf.clone()
    f32 = torch.zeros(2, n, dtype=torch.float32, device=DEV)
    f64 = torch.zeros(4, n, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(n, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(64, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    big = (1 << 26) // n                           # R1 = big + 1 rows of n: one row too many
    refused("mi355_boot_counts", 0, 0, n, buf)
    refused("mi355_boot_counts", 0, 3, 0, buf)
    refused("mi355_boot_counts", 0, big, n, buf)
    refused("mi355_boot_counts", 0, 3, n, None)
    refused("mi355_boot_rank", f32, None, i32, 2, n, 0.5, buf, 1, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, None, i32, 2, 0, 0.5, buf, 4, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, None, i32, 2, n, 0.5, buf, big + 1, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, None, None, 2, n, 0.5, buf, 4, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, f32, i32, 2, n, 0.5, buf, 4, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", None, None, i32, 2, n, 0.5, buf, 4, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, None, i32, 2, n, 0.5, None, 4, ws, ws.numel(), i64, f64)
    refused("mi355_boot_rank", f32, None, i32, 2, n, 0.5, buf, 4, ws, 3, i64, f64)
    refused("mi355_boot_confusion", i32, i32, n, 2, buf, 1, i64, i64)
    refused("mi355_boot_confusion", i32, i32, 0, 2, buf, 4, i64, i64)
    refused("mi355_boot_confusion", i32, i32, n, 65, buf, 4, i64, i64)
    refused("mi355_boot_confusion", i32, i32, n, 2, buf, big + 1, i64, i64)
    refused("mi355_boot_confusion", None, i32, n, 2, buf, 4, i64, i64)
    refused("mi355_boot_confusion", i32, i32, n, 2, buf, 4, None, i64)
    refused("mi355_boot_sums", f64, 4, n, buf, 1, f64, i64)
    refused("mi355_boot_sums", f64, 4, 0, buf, 4, f64, i64)
    refused("mi355_boot_sums", f64, 4, n, buf, big + 1, f64, i64)
    refused("mi355_boot_sums", None, 4, n, buf, 4, f64, i64)
    refused("mi355_boot_sums", f64, 4, n, buf, 4, f64, None)
    refused("mi355_boot_interval", f64, 1, 2, 0.025, 0.975, f64)
    refused("mi355_boot_interval", f64, 8192 + 2, 2, 0.025, 0.975, f64)
    refused("mi355_boot_interval", f64, 4, 0, 0.025, 0.975, f64)
    refused("mi355_boot_interval", f64, 4, 2, 0.975, 0.025, f64)
    refused("mi355_boot_interval", None, 4, 2, 0.025, 0.975, f64)
    refused("mi355_boot_interval", f64, 4, 2, 0.025, 0.975, None)
    refused("mi355_delong", f32, i32, 1, 2, 0, ws, ws.numel(), i64, i64, f64, f64)
    refused("mi355_delong", f32, i32, 0, 2, n, ws, ws.numel(), i64, i64, f64, f64)
    refused("mi355_delong", f32, i32, 1, 2, n, ws, 3, i64, i64, f64, f64)
    refused("mi355_delong", None, i32, 1, 2, n, ws, ws.numel(), i64, i64, f64, f64)
    refused("mi355_delong", f32, None, 1, 2, n, ws, ws.numel(), i64, i64, f64, f64)
    refused("mi355_delong", f32, i32, 1, 2, n, ws, ws.numel(), i64, i64, None, f64)
    assert lib.raw("mi355_boot_rank_ws_ints")(0, n) == -1 and lib.raw("mi355_delong_ws_ints")(1, 2, 1 << 26) == -1
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and not f64.any() and not i64.any(), "a refused call wrote to its buffers"
    for call in (lambda: resample.bootstrap_counts(0, 4, device=DEV), lambda: resample.bootstrap_counts(4, 0, device=DEV),
                 lambda: resample.interval(torch.zeros(8194, 1, dtype=torch.float64, device=DEV)),
                 lambda: resample.boot_means(f64, buf.view(4, n)[:, :4]), lambda: resample.boot_confusion(i32, i32, 65, buf.view(4, n))):
        with pytest.raises(ValueError):
            call()
