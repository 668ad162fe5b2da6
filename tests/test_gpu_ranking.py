"""-m gpu: mi355_rank_metrics (csrc/ranking.hip) against the numpy restatement tests/ranking_ref.py, which tests/test_ranking_cpu.py
pins to scikit-learn.  Every integer — P, N, U2, T, the number of operating points, tp, fp — and the bit patterns of the thresholds are
compared for equality; ``ap`` within ranking_ref.ap_bound(len) = (len + 4) 2^-53 (derived there), NaN exactly where P = 0.  Lengths sit
around the wave, the scan block and the tile of the sort; the score sets put tie groups inside a wave, across waves, across a tile
border and over whole tiles; the label sets include the empty classes and a single positive at either end of the ranking.  Every call
through the ABI writes into sentinel-filled buffers between guard bands: guards intact, nothing written behind the operating points,
two runs bit-identical."""
import functools

import numpy as np
import pytest
import torch

import ranking_ref as R
from mi355.lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lib.raw("mi355_segsort_tile")()
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A


class Guarded:
    """``count`` elements of ``dtype`` filled with sentinel bytes between two guard bands (8-byte aligned)"""

    def __init__(self, count, dtype):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((self.nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.whole[GUARD:GUARD + self.nbytes] = SENTINEL
        self.t = self.whole[GUARD:GUARD + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.whole[:GUARD] == GUARD_BYTE).all()) and bool((self.whole[GUARD + self.nbytes:] == GUARD_BYTE).all())


def op_rank(scores, target=None, labels=None, thr=0.5, curve=True, runs=1):
    """host arrays -> dict of numpy outputs of mi355_rank_metrics through the ABI (curve rows as written: sentinel behind npoints)"""
    S, n = scores.shape
    need = lib.raw("mi355_rank_ws_ints")(S, n)
    assert need > 0, lib.raw("mi355_last_error")()
    z = torch.from_numpy(scores).to(DEV).contiguous()
    z0 = z.clone()
    t = None if target is None else torch.from_numpy(np.ascontiguousarray(target, np.float32)).to(DEV)
    y = None if labels is None else torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(DEV)
    outs = []
    for _ in range(runs):
        g = {"ws": Guarded(need, torch.int32), "counts": Guarded(S * 4, torch.int64), "ap": Guarded(S, torch.float64)}
        if curve:
            g.update(thresholds=Guarded(S * n, torch.float32), tp=Guarded(S * n, torch.int32), fp=Guarded(S * n, torch.int32),
                     npoints=Guarded(S, torch.int32))
        ptr = [g[k].t if curve else None for k in ("thresholds", "tp", "fp", "npoints")] if curve else [None] * 4
        lib.mi355_rank_metrics(z, t, y, S, n, float(thr), g["ws"].t, need, g["counts"].t, g["ap"].t, *ptr)
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values()), "a guard region next to ws or an output was written"
        o = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
        o["counts"] = o["counts"].reshape(S, 4)
        for k in ("thresholds", "tp", "fp"):
            if curve:
                o[k] = o[k].reshape(S, n)
        outs.append(o)
    for o in outs[1:]:
        assert all(np.array_equal(o[k].view(np.uint8), outs[0][k].view(np.uint8)) for k in o), "second run differs"
    assert torch.equal(z.view(torch.int32), z0.view(torch.int32)), "scores were modified"
    return outs[0]


def check(got, refs, n, what):
    """the ABI's outputs against the restatement's list of segments"""
    sent32 = np.frombuffer(bytes([SENTINEL] * 4), dtype=np.int32)[0]
    for s, r in enumerate(refs):
        assert got["counts"][s].tolist() == [r["P"], r["N"], r["U2"], r["T"]], (what, s, got["counts"][s].tolist(), [r["P"], r["N"], r["U2"], r["T"]])
        if r["P"] == 0:
            assert np.isnan(got["ap"][s]), (what, s)
        else:
            assert abs(got["ap"][s] - r["ap"]) <= R.ap_bound(n), (what, s, got["ap"][s], r["ap"])
        if "npoints" in got:
            k = r["T"]
            assert int(got["npoints"][s]) == k, (what, s)
            assert np.array_equal(got["thresholds"][s, :k].view(np.int32), r["thresholds"].view(np.int32)), (what, s)
            assert np.array_equal(got["tp"][s, :k], r["tp"]) and np.array_equal(got["fp"][s, :k], r["fp"]), (what, s)
            for name in ("thresholds", "tp", "fp"):          # nothing is written behind the operating points
                assert (got[name][s, k:].view(np.int32) == sent32).all(), (what, s, name)


def shuffled(sorted_vals, rng):
    return np.ascontiguousarray(sorted_vals[rng.permutation(sorted_vals.size)], dtype=np.float32)


def score_sets(S, n, seed):
    rng = np.random.RandomState(seed)
    ramp = np.arange(n, dtype=np.float32) - n // 2
    across = ramp.copy()
    across[max(0, min(n, T - 5)):min(n, T + 6)] = ramp[max(0, min(n - 1, T - 5))]          # one group over ranks T-5 .. T+5
    tiles = ramp.copy()
    tiles[max(0, min(n, T - 3)):min(n, 3 * T + 2)] = ramp[max(0, min(n - 1, T - 3))]         # one group over tiles 1 and 2 and beyond
    return {"randn": rng.randn(S, n).astype(np.float32),
            "quantised": (np.round(rng.randn(S, n) * 4) / 4).astype(np.float32),            # multiples of 0.25, -0.0 among them
            "equal": np.full((S, n), 1.5, dtype=np.float32),
            "ascending": np.tile(ramp, (S, 1)),
            "descending": np.tile(ramp[::-1].copy(), (S, 1)),
            "two_valued": np.where(rng.rand(S, n) < 0.5, np.float32(-1.5), np.float32(2.0)).astype(np.float32),
            "run_across_the_tile_border": np.stack([shuffled(across, rng) for _ in range(S)]),
            "run_over_two_tiles": np.stack([shuffled(tiles, rng) for _ in range(S)])}


def target_sets(scores, seed):
    S, n = scores.shape
    rng = np.random.RandomState(seed)
    order = np.argsort(scores + np.float32(0), axis=1, kind="stable")
    lowest, highest = np.zeros((S, n), np.float32), np.zeros((S, n), np.float32)
    lowest[np.arange(S), order[:, 0]] = 1
    highest[np.arange(S), order[:, -1]] = 1
    return {"half": (rng.rand(S, n) < 0.5).astype(np.float32), "one_percent": (rng.rand(S, n) < 0.01).astype(np.float32),
            "all_negative": np.zeros((S, n), np.float32), "all_positive": np.ones((S, n), np.float32),
            "one_at_the_lowest_rank": lowest, "one_at_the_highest_rank": highest}


LENGTHS = sorted({1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 4 * T + 1, 65536})


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("S", [1, 3])
def test_rank_metrics_are_the_restatement(S, n):
    for name, scores in score_sets(S, n, 1000 * S + n).items():
        assert not np.isnan(scores).any()
        first = True
        for tname, target in target_sets(scores, n + len(name)).items():
            got = op_rank(scores, target=target, runs=2 if first else 1)
            check(got, R.rank_ref(scores, target=target), n, (name, tname, S, n))
            first = False
        labels = np.random.RandomState(n).randint(0, 3, n).astype(np.int32)          # one-vs-rest over C = 3 classes (S = 1: class 0)
        got = op_rank(scores, labels=labels, runs=2)
        check(got, R.rank_ref(scores, labels=labels), n, (name, "labels", S, n))


def test_threshold_and_skipped_curve():
    S, n = 3, 2 * T + 1
    scores = score_sets(S, n, 7)["quantised"]
    target = np.random.RandomState(8).rand(S, n).astype(np.float32)
    refs = R.rank_ref(scores, target=target, thr=0.7)
    assert 0 < refs[0]["P"] < 0.4 * n
    full = op_rank(scores, target=target, thr=0.7)
    check(full, refs, n, "thr=0.7")
    bare = op_rank(scores, target=target, thr=0.7, curve=False)
    assert set(bare) == {"counts", "ap"}
    assert np.array_equal(bare["counts"], full["counts"]) and np.array_equal(bare["ap"].view(np.int64), full["ap"].view(np.int64))


@pytest.mark.parametrize("S,n", [(32, 65536), (1, 2097152)])
def test_benchmark_shapes(S, n):
    sets = score_sets(S, n, 5)
    for name in ("randn", "quantised"):
        scores = sets[name]
        target = (np.random.RandomState(6).rand(S, n) < (0.5 if name == "randn" else 0.01)).astype(np.float32)
        check(op_rank(scores, target=target), R.rank_ref(scores, target=target), n, (name, S, n))


@pytest.mark.parametrize("S,n", [(3, 257), (2, 2 * T + 1)])
def test_nan_scores_keep_every_write_in_bounds(S, n):
    rng = np.random.RandomState(3)
    scores = rng.randn(S, n).astype(np.float32)
    scores[:, ::7] = np.nan
    scores[0, 1] = -np.nan
    target = (rng.rand(S, n) < 0.3).astype(np.float32)
    got = op_rank(scores, target=target)              # the guards are checked inside
    assert np.array_equal(got["counts"][:, 0], target.sum(1).astype(np.int64))
    assert (got["counts"][:, 0] + got["counts"][:, 1] == n).all()
    assert (got["npoints"] >= 1).all() and (got["npoints"] <= n).all() and np.array_equal(got["npoints"], got["counts"][:, 3])


@functools.lru_cache(maxsize=None)
def _surface_case():
    S, n = 3, 2 * T + 1
    scores = score_sets(S, n, 9)["quantised"]
    target = (np.random.RandomState(10).rand(S, n) < 0.3).astype(np.float32)
    labels = np.random.RandomState(11).randint(0, 3, n).astype(np.int32)
    return scores, target, labels


def test_python_surface_matches_the_abi():
    from utils import ranking as UR
    scores, target, labels = _surface_case()
    S, n = scores.shape
    z = torch.from_numpy(scores).to(DEV)
    for kw_np, kw in (({"target": target}, {"target": torch.from_numpy(target).to(DEV)}),
                      ({"labels": labels}, {"labels": torch.from_numpy(labels).to(DEV).long()})):
        want = op_rank(scores, **kw_np)
        refs = R.rank_ref(scores, **kw_np)
        m = UR.rank_metrics(z, **kw)
        assert set(m) == {"pos", "neg", "u2", "thresholds_n", "auroc", "average_precision"}
        assert all(v.is_cuda and v.shape == (S,) for v in m.values())
        assert m["auroc"].dtype == torch.float64 and m["average_precision"].dtype == torch.float64 and m["u2"].dtype == torch.int64
        got = torch.stack([m["pos"], m["neg"], m["u2"], m["thresholds_n"]], 1).cpu().numpy()
        assert np.array_equal(got, want["counts"])
        assert np.array_equal(m["average_precision"].cpu().numpy().view(np.int64), want["ap"].view(np.int64))
        assert np.array_equal(m["auroc"].cpu().numpy(), np.array([r["auroc"] for r in refs]))          # one division of exact integers
        curves = UR.binary_curve(z, **kw)
        rocs, prs = UR.roc_curve(z, **kw), UR.precision_recall_curve(z, **kw)
        assert len(curves) == S
        for s, r in enumerate(refs):
            thr, tp, fp = curves[s]
            assert thr.dtype == np.float32 and tp.dtype == np.int32 and thr.shape == (r["T"],)
            assert np.array_equal(thr.view(np.int32), r["thresholds"].view(np.int32)) and np.array_equal(tp, r["tp"]) and np.array_equal(fp, r["fp"])
            for a, b in zip(rocs[s], R.roc_ref(r)):
                assert np.array_equal(a, b)
            for a, b in zip(prs[s], R.pr_ref(r)):
                assert np.array_equal(a, b)
    # [B, 1, H, W] maps are flattened per sample; a 1-D score vector is one segment; undefined figures are NaN
    m4 = UR.rank_metrics(z[:, :2048].reshape(3, 1, 32, 64), target=torch.from_numpy(target[:, :2048]).to(DEV).reshape(3, 1, 32, 64))
    assert np.array_equal(m4["u2"].cpu().numpy(), [r["U2"] for r in R.rank_ref(scores[:, :2048], target=target[:, :2048])])
    m1 = UR.rank_metrics(z[0], target=torch.zeros(n, device=DEV))
    assert m1["auroc"].shape == (1,) and bool(torch.isnan(m1["auroc"]).all()) and bool(torch.isnan(m1["average_precision"]).all())
    ones = UR.rank_metrics(z[0], target=torch.ones(n, device=DEV))
    assert bool(torch.isnan(ones["auroc"]).all()) and abs(float(ones["average_precision"][0]) - 1.0) <= R.ap_bound(n)
    with pytest.raises(ValueError, match="must match"):
        UR.rank_metrics(z, target=torch.zeros(3, 5, device=DEV))
    with pytest.raises(ValueError, match="shared by the segments"):
        UR.rank_metrics(z, labels=torch.zeros(5, dtype=torch.int32, device=DEV))


def test_bad_arguments_raise():
    z = torch.zeros(2, 8, device=DEV)
    c, a = torch.empty(2, 4, dtype=torch.int64, device=DEV), torch.empty(2, dtype=torch.float64, device=DEV)
    ws = torch.empty(lib.raw("mi355_rank_ws_ints")(2, 8), dtype=torch.int32, device=DEV)
    y = torch.zeros(8, dtype=torch.int32, device=DEV)
    for args in ((z, z, y, 2, 8, 0.5, ws, ws.numel(), c, a, None, None, None, None), (z, None, None, 2, 8, 0.5, ws, ws.numel(), c, a, None, None, None, None),
                 (z, z, None, 2, 8, 0.5, ws, ws.numel() - 1, c, a, None, None, None, None), (z, z, None, 2, 8, 0.5, ws, ws.numel(), c, a, z, None, None, None)):
        with pytest.raises(RuntimeError, match="rank_metrics"):
            lib.mi355_rank_metrics(*args)
