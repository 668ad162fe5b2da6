"""-m gpu: csrc/calibrate.hip through the ABI against the numpy restatement tests/calibrate_ref.py (pinned on the CPU by
tests/test_calibrate_cpu.py), which derives every bound used here.

Temperature: status and — in the clamp and flat cases — beta exactly; in the converged cases the restated fp64 g' has to change sign
across [beta_gpu (1 - 2^-30), beta_gpu (1 + 2^-30)] and both NLLs lie within temp_nll_bound of the restatement at beta_gpu, on inputs
asserted to have an interior optimum with g'' >= 1e-3.  mi355_logits_scale to the bit.  Sweep: tp, fp, pos for equality; the fold within
fold_bound; the pick by the restatement's argmax rule.  Every call writes into sentinel-filled buffers between guard bands: guards
intact, inputs unmodified, two runs bit-identical."""
import numpy as np
import pytest
import torch

import calibrate_ref as CR
from mi355.lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BYTE, SENTINEL = 0xA5, 0x5A
CHUNK = lib.raw("mi355_thr_sweep_chunk")()


class Guarded:
    """``count`` elements of ``dtype`` filled with sentinel bytes between two guard bands (8-byte aligned)"""

    def __init__(self, count, dtype, fill=None):
        self.nbytes = count * torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((self.nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.whole[GUARD:GUARD + self.nbytes] = SENTINEL
        self.t = self.whole[GUARD:GUARD + self.nbytes].view(dtype)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.whole[:GUARD] == GUARD_BYTE).all()) and bool((self.whole[GUARD + self.nbytes:] == GUARD_BYTE).all())


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def ws_ints(name, *shape):
    need = lib.raw(name)(*shape)
    assert need > 0, lib.raw("mi355_last_error")()
    return need


# ---- temperature -----------------------------------------------------------------------------------------------------------------
def op_fit(x, labels, runs=2):
    """-> state float64 [8] of mi355_temperature_fit; also checks mi355_temperature_eval at the fitted beta against state[3..5]"""
    N, C = x.shape
    need = ws_ints("mi355_temperature_fit_ws_ints", N, C)
    xd, yd = dev(x, np.float32), dev(labels, np.int32)
    x0, y0 = xd.clone(), yd.clone()
    outs = []
    for _ in range(runs):
        g = {"ws": Guarded(need, torch.int32), "state": Guarded(8, torch.float64), "out": Guarded(3, torch.float64)}
        lib.mi355_temperature_fit(xd, N, C, yd, g["ws"].t, need, g["state"].t)
        lib.mi355_temperature_eval(xd, N, C, yd, g["state"].t, g["ws"].t, need, g["out"].t)
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values()), "a guard region next to ws, state or out was written"
        outs.append((g["state"].t.cpu().numpy(), g["out"].t.cpu().numpy()))
    assert all(same_bits(o[0], outs[0][0]) and same_bits(o[1], outs[0][1]) for o in outs[1:]), "second run differs"
    assert torch.equal(xd.view(torch.int32), x0.view(torch.int32)) and torch.equal(yd, y0), "inputs were modified"
    state, out = outs[0]
    assert same_bits(out, state[3:6]), ("one evaluation at the fitted beta is not the fit's last one", out, state[3:6])
    return state


CONVERGED = [(63, 2), (64, 3), (65, 32), (65, 33), (257, 64), (257, 65), (63, 1000), (4096, 3), (4096, 64), (257, 1000)]


@pytest.mark.parametrize("T0", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("N,C", CONVERGED)
def test_temperature_converges_to_the_root_of_the_gradient(N, C, T0):
    x, labels = CR.temperature_inputs(N, C, T0, seed=100 * N + C)
    s = op_fit(x, labels)
    beta, status = float(s[0]), int(s[7])
    at = CR.nll_terms(x, labels, beta)
    print(f"N={N} C={C} T0={T0}: beta={beta!r} evals={int(s[6])} g'={s[4]:.3e} g''={s[5]:.4f} (restated {at['g1']:.3e}, {at['g2']:.4f})")
    # the test's own inputs: an interior optimum with curvature
    assert CR.BETA_LO < beta < CR.BETA_HI and at["g2"] >= 1e-3, (beta, at["g2"])
    assert status == 0 and 3 <= int(s[6]) <= CR.MAX_EVALS, s
    ok, below, above = CR.sign_change(x, labels, beta)
    assert ok, ("the restated g' does not change sign around beta_gpu", beta, below, above)
    assert s[1] == 1.0 / beta
    one = CR.nll_terms(x, labels, 1.0)
    for got, ref in ((s[2], one), (s[3], at)):
        bound = CR.temp_nll_bound(N, C, ref["nll_max"], ref["zmax"])
        print(f"  NLL {got!r} restated {ref['nll']!r} diff {abs(got - ref['nll']):.3e} bound {bound:.3e}")
        assert bound < 1e-9 and abs(got - ref["nll"]) <= bound, (got, ref["nll"], bound)
    assert abs(s[5] - at["g2"]) <= 1e-9 * at["g2"], (s[5], at["g2"])


def margin_logits(N, C, seed, margin, pick):
    """randn logits whose label — ``pick`` of argmax / argmin — is ``margin`` away from the rest"""
    rng = np.random.RandomState(seed)
    x = rng.randn(N, C).astype(np.float32)
    labels = pick(x, 1).astype(np.int32)
    x[np.arange(N), labels] += np.float32(margin)
    return x, labels


@pytest.mark.parametrize("N,C", [(1, 2), (1, 65), (65, 3), (257, 33)])
def test_temperature_clamps_and_flat_rows(N, C):
    # separable: the correct logit larger by 50 -> g' < 0 up to 2^6 (where it underflows to 0)
    x, labels = margin_logits(N, C, N + C, 50.0, np.argmax)
    ref = CR.temperature_ref(x, labels)
    s = op_fit(x, labels)
    assert ref["status"] == 2 and (int(s[7]), s[0], s[1], int(s[6])) == (2, 64.0, 1.0 / 64, 2), (s, ref)
    # the label always the smallest logit, by a margin: g' > 0 down to 2^-6
    x, labels = margin_logits(N, C, N + C + 1, -50.0, np.argmin)
    ref = CR.temperature_ref(x, labels)
    assert CR.nll_terms(x, labels, CR.BETA_LO)["g1"] > 1.0
    s = op_fit(x, labels)
    assert ref["status"] == 1 and (int(s[7]), s[0], s[1], int(s[6])) == (1, 2.0 ** -6, 64.0, 2), (s, ref)
    # every row constant: g'' = 0 at beta = 1
    x = np.repeat(np.random.RandomState(N).randn(N, 1).astype(np.float32), C, axis=1)
    labels = np.random.RandomState(C).randint(0, C, N).astype(np.int32)
    ref = CR.temperature_ref(x, labels)
    s = op_fit(x, labels)
    assert ref["status"] == 3 and (int(s[7]), s[0], s[1], int(s[6])) == (3, 1.0, 1.0, 1), (s, ref)
    assert abs(s[2] - np.log(C)) <= CR.temp_nll_bound(N, C, np.log(C), float(np.abs(x).max())), s
    assert same_bits(s[2], s[3]) and s[4] == 0.0 and s[5] == 0.0, s


def test_temperature_of_a_single_row():
    # N = 1 with the label on the middle logit: E_p[x] crosses x_y inside the bracket
    x = np.array([[2.0, 0.5, -1.0, -1.5]], dtype=np.float32)
    labels = np.array([1], dtype=np.int32)
    ref = CR.temperature_ref(x, labels)
    s = op_fit(x, labels)
    assert ref["status"] == 0 and int(s[7]) == 0 and CR.nll_terms(x, labels, float(s[0]))["g2"] >= 1e-3
    assert CR.sign_change(x, labels, float(s[0]))[0] and abs(s[0] - ref["beta"]) <= 1e-9 * ref["beta"]
    at = CR.nll_terms(x, labels, float(s[0]))
    assert abs(s[3] - at["nll"]) <= CR.temp_nll_bound(1, 4, at["nll_max"], at["zmax"])


def test_temperature_nan_and_bad_labels_stop_at_once():
    x, labels = CR.temperature_inputs(65, 3, 1.0, seed=5)
    bad = labels.copy()
    bad[7] = 3                                     # outside 0 .. C - 1: read as a NaN, nothing out of bounds
    s = op_fit(x, bad)
    assert int(s[7]) == 4 and int(s[6]) == 1 and s[0] == 1.0 and np.isnan(s[4])
    xn = x.copy()
    xn[3, 1] = np.nan
    s = op_fit(xn, labels)
    assert int(s[7]) == 4 and int(s[6]) == 1 and s[0] == 1.0


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4099])
def test_logits_scale_is_one_rounding(n):
    rng = np.random.RandomState(n)
    x = (rng.randn(n) * 5).astype(np.float32)
    beta = np.array([0.7310585786300049, -1.0], dtype=np.float64)          # only beta_dev[0] is read
    shapes = [(1, n)] + ([(n // 3, 3)] if n % 3 == 0 else [])
    for N, C in shapes:
        for off in (0, 1):                          # a 16-byte aligned pair of buffers, and one 4 bytes off it
            xg = Guarded(n + off, torch.float32, fill=dev(np.r_[np.zeros(off, np.float32), x], np.float32))
            yg = Guarded(n + off, torch.float32)
            bd = dev(beta, np.float64)
            runs = []
            for _ in range(2):
                lib.mi355_logits_scale(xg.t[off:], N, C, bd, yg.t[off:])
                torch.cuda.synchronize()
                runs.append(yg.t.cpu().numpy())
            assert xg.intact() and yg.intact()
            assert same_bits(runs[0], runs[1]) and same_bits(xg.t[off:].cpu().numpy(), x)
            assert same_bits(runs[0][off:], (x.astype(np.float64) * beta[0]).astype(np.float32)), (N, C, off)
            assert (runs[0][:off].view(np.int32) == np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]).all()


# ---- sweep -----------------------------------------------------------------------------------------------------------------------
def op_sweep(scores, target, thr, is_logit=False, tthr=0.5, runs=1):
    B, n = scores.shape
    K = len(thr)
    need = ws_ints("mi355_thr_sweep_ws_ints", B, n, K)
    sd, td, hd = dev(scores, np.float32), dev(target, np.float32), dev(thr, np.float32)
    keep = [t.clone() for t in (sd, td, hd)]
    outs = []
    for _ in range(runs):
        g = {"ws": Guarded(need, torch.int32), "tp": Guarded(B * K, torch.int32), "fp": Guarded(B * K, torch.int32),
             "pos": Guarded(B, torch.int32)}
        lib.mi355_thr_sweep(sd, td, B, n, hd, K, 1 if is_logit else 0, float(tthr), g["ws"].t, need, g["tp"].t, g["fp"].t, g["pos"].t)
        torch.cuda.synchronize()
        assert all(v.intact() for v in g.values()), "a guard region next to ws or an output was written"
        outs.append((g["tp"].t.cpu().numpy().reshape(B, K), g["fp"].t.cpu().numpy().reshape(B, K), g["pos"].t.cpu().numpy()))
    assert all(all(np.array_equal(a, b) for a, b in zip(o, outs[0])) for o in outs[1:]), "second run differs"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((sd, td, hd), keep)), "inputs were modified"
    return outs[0]


def threshold_lists(K):
    grid = (np.arange(1, K + 1, dtype=np.float32) / np.float32(K + 1)).astype(np.float32)
    zero = ((np.arange(K, dtype=np.float32) - np.float32(K // 2)) / np.float32(2048)).astype(np.float32)          # holds 0.0 exactly
    assert (np.diff(grid) > 0).all() and (np.diff(zero) > 0).all() and zero[K // 2] == 0.0
    return {"grid": grid, "around_zero": zero}


def score_sets(B, n, thr, rng):
    lo, hi = float(thr[0]), float(thr[-1])
    uniform = (lo - 0.1 + rng.rand(B, n) * (hi - lo + 0.2)).astype(np.float32)
    nan = uniform.copy()
    nan[:, ::5] = np.nan
    nan[0, 0] = -np.nan
    tiny = np.float32(1e-45)
    return {"uniform": uniform,
            "on_the_candidates": thr[rng.randint(0, len(thr), (B, n))],
            "signed_zeros": np.array([0.0, -0.0, tiny, -tiny], dtype=np.float32)[rng.randint(0, 4, (B, n))],
            "all_below": np.full((B, n), lo - 1, dtype=np.float32), "all_above": np.full((B, n), hi + 1, dtype=np.float32),
            "nan": nan}


LENGTHS = [1, 63, 64, 65, 255, 256, 257, 2 * CHUNK + 77]
KS = [1, 2, 63, 64, 65, 255, 1024]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("B", [1, 3])
def test_sweep_counts_are_the_restatement(B, n):
    rng = np.random.RandomState(1000 * B + n)
    targets = {"mixed": (rng.rand(B, n) < 0.4).astype(np.float32), "all_positive": np.ones((B, n), np.float32),
               "none_positive": np.zeros((B, n), np.float32)}
    for K in KS:
        for lname, thr in threshold_lists(K).items():
            first = True
            for sname, scores in score_sets(B, n, thr, rng).items():
                for tname, target in targets.items():
                    if n > CHUNK and tname != "mixed" and sname not in ("uniform", "nan"):
                        continue                  # (the long image: every score set once, the target sets on two of them)
                    got = op_sweep(scores, target, thr, runs=2 if first else 1)
                    first = False
                    for name, a, b in zip(("tp", "fp", "pos"), got, CR.sweep_ref(scores, target, thr)):
                        assert np.array_equal(a, b), (name, B, n, K, lname, sname, tname)


def test_sweep_target_threshold_and_nan_bin():
    rng = np.random.RandomState(3)
    thr = threshold_lists(65)["grid"]
    scores = np.full((2, 300), np.nan, dtype=np.float32)
    target = rng.rand(2, 300).astype(np.float32)
    tp, fp, pos = op_sweep(scores, target, thr, tthr=0.7)
    assert not tp.any() and not fp.any() and np.array_equal(pos, (target > np.float32(0.7)).sum(1))          # NaN: bin 0, above no candidate
    scores = rng.rand(2, 300).astype(np.float32)
    for a, b in zip(op_sweep(scores, target, thr, tthr=0.7), CR.sweep_ref(scores, target, thr, tthr=0.7)):
        assert np.array_equal(a, b)


def safe_logits(B, n, thr, rng):
    """logits whose fp64 sigmoid is at least 2^-20 from every candidate"""
    z = (rng.randn(B, n) * 3).astype(np.float32)
    near = np.abs(CR.sigmoid64(z)[..., None] - thr.astype(np.float64)).min(-1) < 2.0 ** -19
    z[near] = np.float32(0.3)
    return z


@pytest.mark.parametrize("B,n", [(1, 257), (3, 4099), (2, 2 * CHUNK + 77)])
def test_sweep_of_logits(B, n):
    rng = np.random.RandomState(n)
    thr = CR.DEFAULT_THRESHOLDS
    assert thr[127] == 0.5 and len(thr) == 255
    z = safe_logits(B, n, thr, rng)
    assert CR.logit_margin(z, thr) >= 2.0 ** -20
    target = (rng.rand(B, n) < 0.3).astype(np.float32)
    got = op_sweep(z, target, thr, is_logit=True, runs=2)
    for name, a, b in zip(("tp", "fp", "pos"), got, CR.sweep_ref(z, target, thr, is_logit=True)):
        assert np.array_equal(a, b), name
    # the same buffers through mi355_seg_counts at three of the candidates
    zd, td = dev(z, np.float32), dev(target, np.float32)
    for k in (0, 127, 254):
        cnt = torch.empty(B, 4, dtype=torch.float32, device=DEV)
        lib.mi355_seg_counts(zd, td, cnt, B, n, 1, float(thr[k]))
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:, 0], got[0][:, k]) and np.array_equal(c[:, 1], got[0][:, k] + got[1][:, k]) and np.array_equal(c[:, 2], got[2])


# ---- fold and pick ---------------------------------------------------------------------------------------------------------------
def op_fold_pick(batches, K, k_ref):
    """[(tp, fp, pos), ...] -> (acc float64 [2, K], n_images, out_d float64 [4], out_k) through the ABI"""
    runs = []
    for _ in range(2):
        acc, n = Guarded(2 * K, torch.float64), Guarded(1, torch.int64)
        acc.t.zero_()
        n.t.zero_()
        for tp, fp, pos in batches:
            lib.mi355_thr_sweep_fold(dev(tp, np.int32), dev(fp, np.int32), dev(pos, np.int32), tp.shape[0], K, acc.t, n.t)
        out_d, out_k = Guarded(4, torch.float64), Guarded(1, torch.int32)
        lib.mi355_thr_sweep_pick(acc.t, n.t, K, k_ref, out_d.t, out_k.t)
        torch.cuda.synchronize()
        assert acc.intact() and n.intact() and out_d.intact() and out_k.intact()
        runs.append((acc.t.cpu().numpy().reshape(2, K), int(n.t.cpu()), out_d.t.cpu().numpy(), int(out_k.t.cpu())))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][2], runs[1][2]) and runs[0][1::2] == runs[1][1::2]
    return runs[0]


def check_fold_pick(batches, K, k_ref, what):
    acc, n, out_d, out_k = op_fold_pick(batches, K, k_ref)
    racc, rn = CR.fold_ref(batches, K)
    bound = CR.fold_bound(rn)
    assert n == rn
    worst = float(np.abs(acc - racc).max())
    print(f"{what}: n={n} largest |sum - restated| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound, (what, worst, bound)
    k, dice, iou, dice_ref, iou_ref, gap = CR.pick_ref(racc, rn, k_ref)
    mean = racc / rn
    assert mean[0][k] - mean[0][out_k] <= 2 * bound, (what, out_k, k)
    if gap > 2 * bound:
        assert out_k == k, (what, out_k, k)
    for got, ref in zip(out_d, (mean[0][out_k], mean[1][out_k], dice_ref, iou_ref)):
        assert (np.isnan(got) and np.isnan(ref)) or abs(got - ref) <= 2 * bound, (what, got, ref)
    return out_k, out_d


def test_fold_two_batches_and_pick():
    rng = np.random.RandomState(11)
    thr = CR.DEFAULT_THRESHOLDS
    batches = []
    for B in (3, 2):
        target = (rng.rand(B, 700) < 0.35).astype(np.float32)
        scores = np.clip(0.35 * target + 0.2 + 0.25 * rng.randn(B, 700), 0, 1).astype(np.float32)
        batches.append(CR.sweep_ref(scores, target, thr))
    out_k, out_d = check_fold_pick(batches, len(thr), 127, "two batches")
    assert out_d[0] >= out_d[2] > 0.3
    check_fold_pick(batches, len(thr), -1, "no reference candidate")
    check_fold_pick(batches[:1], len(thr), 0, "one batch")


def test_pick_takes_the_lowest_index_of_a_plateau():
    thr = CR.DEFAULT_THRESHOLDS
    target = np.zeros((2, 64), np.float32)
    target[:, :20] = 1
    scores = np.where(target > 0, np.float32(0.8), np.float32(0.2)).astype(np.float32)
    scores[:, 20:24] = 0.45                         # four false positives below 0.45: the plateau of Dice = 1 starts at 0.45
    out_k, out_d = check_fold_pick([CR.sweep_ref(scores, target, thr)], len(thr), 127, "plateau")
    assert thr[out_k] == np.float32(116 / 256) and out_k == 115 and out_d[0] == 1.0 and out_d[2] == 1.0


def test_pick_on_empty_images():
    thr = CR.DEFAULT_THRESHOLDS
    empty = CR.sweep_ref(np.zeros((3, 50), np.float32), np.zeros((3, 50), np.float32), thr)
    out_k, out_d = check_fold_pick([empty, empty], len(thr), 127, "all empty")
    assert out_k == 0 and out_d[0] == 1.0 and out_d[1] == 1.0 and out_d[2] == 1.0


def test_python_surface():
    from utils import calibrate as UC
    x, labels = CR.temperature_inputs(257, 3, 3.0, seed=21)
    xd, yd = dev(x, np.float32), dev(labels, np.int64)
    fit = UC.fit_temperature(xd, yd)
    assert all(v.is_cuda for v in fit.values()) and fit["state"].dtype == torch.float64
    state = op_fit(x, labels, runs=1)
    assert same_bits(fit["state"].cpu().numpy(), state)
    y = UC.apply_temperature(xd, fit)
    assert same_bits(y.cpu().numpy(), (x.astype(np.float64) * state[0]).astype(np.float32))
    assert same_bits(UC.apply_temperature(xd, 4.0).cpu().numpy(), (x.astype(np.float64) * 0.25).astype(np.float32))
    assert same_bits(UC.nll_at(xd, yd, fit).cpu().numpy(), state[3])
    rng = np.random.RandomState(22)
    target = (rng.rand(5, 1, 16, 24) < 0.4).astype(np.float32)
    z = safe_logits(5, 16 * 24, CR.DEFAULT_THRESHOLDS, rng).reshape(5, 1, 16, 24)
    acc = UC.dice_sweep(dev(z[:3], np.float32), dev(target[:3], np.float32), is_logit=True)
    acc = UC.dice_sweep(dev(z[3:], np.float32), dev(target[3:], np.float32), is_logit=True, acc=acc)
    refs = [CR.sweep_ref(z[a:b].reshape(b - a, -1), target[a:b].reshape(b - a, -1), CR.DEFAULT_THRESHOLDS, is_logit=True) for a, b in ((0, 3), (3, 5))]
    racc, rn = CR.fold_ref(refs, 255)
    assert int(acc["n_images"]) == 5 and np.array_equal(acc["tp"].cpu().numpy(), refs[1][0])
    assert np.abs(acc["sums"].cpu().numpy() - racc).max() <= CR.fold_bound(5)
    p = UC.pick_threshold(acc)
    k = CR.pick_ref(racc, rn, 127)
    assert abs(float(p["dice_ref"]) - k[3]) <= 2 * CR.fold_bound(5) and float(p["threshold"]) == float(CR.DEFAULT_THRESHOLDS[int(p["index"])])
    with pytest.raises(ValueError, match="ascending"):
        UC.dice_sweep(dev(z, np.float32), dev(target, np.float32), thresholds=[0.5, 0.5])


def test_bad_arguments_raise():
    x = torch.zeros(4, 3, device=DEV)
    y = torch.zeros(4, dtype=torch.int32, device=DEV)
    st = torch.empty(8, dtype=torch.float64, device=DEV)
    ws = torch.empty(64, dtype=torch.int32, device=DEV)
    for args in ((x, 4, 1, y, ws, 64, st), (x, 4, 3, y, ws, 8, st), (x, 4, 3, None, ws, 64, st), (x, 0, 3, y, ws, 64, st)):
        with pytest.raises(RuntimeError, match="temperature_fit"):
            lib.mi355_temperature_fit(*args)
    assert lib.raw("mi355_temperature_fit_ws_ints")(4, 4097) < 0 and lib.raw("mi355_thr_sweep_ws_ints")(1, 1 << 25, 4) < 0
    s = torch.zeros(2, 8, device=DEV)
    thr = torch.tensor([0.5], device=DEV)
    o = torch.empty(2, 1, dtype=torch.int32, device=DEV)
    big = torch.empty(4096, dtype=torch.int32, device=DEV)
    for args in ((s, s, 2, 8, thr, 0, 0, 0.5, big, 4096, o, o, o), (s, s, 2, 8, thr, 1025, 0, 0.5, big, 4096, o, o, o),
                 (s, s, 2, 8, thr, 1, 0, 0.5, big, 7, o, o, o), (s, s, 2, 8, None, 1, 0, 0.5, big, 4096, o, o, o)):
        with pytest.raises(RuntimeError, match="thr_sweep"):
            lib.mi355_thr_sweep(*args)
    acc = torch.zeros(2, 1, dtype=torch.float64, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="thr_sweep_pick"):
        lib.mi355_thr_sweep_pick(acc, n, 1, 1, torch.empty(4, dtype=torch.float64, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV))
