"""tests/head_ref.py on the CPU: every reference agrees with torch's own operator (forward and autograd) at the case shapes of
tests/test_gpu_head_exact.py; the float32 restatement of each bounded chain stays within HALF of its bound on the very inputs
the GPU cases use (the figures behind K_ADAMW / K_BCE / K_CE / POW_U are printed); every checker rejects a wrong result of the
kind it exists to catch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_bounds as cb
import head_ref as hr

F32, BF, FP = hr.F32, hr.BF, hr.FP
MARGIN = 0.5                 # a correct float32 chain may use half of a bound


# ---- references against torch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hr.MAXPOOL_CASES)
def test_maxpool_reference_is_torchs_operator_and_its_data_stay_exact(case):
    k, s, p, H, W, _ = case
    x, dy, old = hr.maxpool_case(k, s, p, H, W)
    y, dx = hr.maxpool_ref(x, dy, k, s, p, old)
    xr = x.float().requires_grad_(True)
    yt = F.max_pool2d(xr, k, s, p)
    yt.backward(dy.float())
    assert torch.equal(yt.detach().double(), y) and torch.equal((xr.grad + old.float()).double(), dx)
    for t in (x, dy, old, y, dx):                                         # exact in every storage type, sums included
        for dt in (BF, FP, F32):
            assert torch.equal(t.to(dt).double(), t)
    # the first maximum written out: window by window, scan order, strict >
    N, C = x.shape[:2]
    ho, wo = y.shape[2:]
    want = old.clone()
    for i in range(ho):
        for j in range(wo):
            best = torch.full((N, C), -math.inf, dtype=torch.float64)
            bh = torch.zeros(N, C, dtype=torch.long)
            bw = torch.zeros(N, C, dtype=torch.long)
            for kh in range(k):
                for kw in range(k):
                    h, w = i * s + kh - p, j * s + kw - p
                    if 0 <= h < H and 0 <= w < W:
                        gt = x[:, :, h, w] > best
                        best = torch.where(gt, x[:, :, h, w], best)
                        bh, bw = torch.where(gt, h, bh), torch.where(gt, w, bw)
            n_i, c_i = torch.meshgrid(torch.arange(N), torch.arange(C), indexing="ij")
            want.index_put_((n_i, c_i, bh, bw), dy[:, :, i, j], accumulate=True)
    assert torch.equal(want, dx)
    if (k, s, p, H, W) == (2, 2, 0, 5, 9):                                # the last row and column lie in no window
        assert torch.equal(dx[:, :, 4, :], old[:, :, 4, :]) and torch.equal(dx[:, :, :, 8], old[:, :, :, 8])


@pytest.mark.parametrize("case", hr.GLOBAL_CASES)
def test_global_pool_reference(case):
    N, HW, C = case
    x, dy = hr.global_case(N, HW, C)
    pairs = hr.plant_wave_ties(x)
    if HW >= 8:
        assert pairs == set(hr.WAVE_PAIRS)
    y, idx, dx = hr.global_pool_ref(x, dy, 1)
    first = torch.from_numpy(np.argmax(x.numpy(), axis=1))                # numpy: the first occurrence
    assert torch.equal(idx, first) and torch.equal(y, x.amax(1))
    want = torch.zeros_like(x)
    want.scatter_(1, first.unsqueeze(1), dy.unsqueeze(1))
    assert torch.equal(dx, want)
    if HW > 1:
        assert int((x == y.unsqueeze(1)).sum(1).max()) >= 2               # the maximum really occurs twice somewhere
    y, idx, dx = hr.global_pool_ref(x, dy, 0)
    assert idx is None and torch.allclose(y, x.mean(1), rtol=1e-15, atol=0)
    assert torch.allclose(dx, (dy / HW).unsqueeze(1).expand_as(x), rtol=1e-15, atol=0)
    assert torch.equal(x.sum(1).float().double(), x.sum(1))               # the sum is exact in fp32 in any order (multiples of 1/2)


@pytest.mark.parametrize("case", hr.ADAPTIVE_CASES)
def test_adaptive_avgpool_reference(case):
    H, W, OH, OW, exact = case
    x, dy = hr.adaptive_case(H, W, OH, OW)
    y, dx, slack = hr.adaptive_avg_ref(x, dy, OH, OW)
    assert torch.allclose(hr.adaptive_avg_plain(x, OH, OW), y, rtol=1e-15, atol=1e-300)
    xr = x.float().requires_grad_(True)
    yt = F.adaptive_avg_pool2d(xr, (OH, OW)).flatten(1)
    yt.backward(dy.float())
    assert hr.check_bounded(yt.detach(), y, cb.ulp(y, F32))[0] <= 1 and hr.check_interval(xr.grad, dx, F32, slack)[0] <= 1
    if exact:
        assert torch.equal(yt.detach().double(), y)
        for dt in (BF, FP, F32):
            assert torch.equal(dx.to(dt).double(), dx), "the exact cases' dx must be storable"
    else:
        assert not torch.equal(dx.float().double(), dx)


def _mix32_int(k):
    M = (1 << 64) - 1
    k = (k + 0x9E3779B97F4A7C15) & M
    k = ((k ^ (k >> 30)) * 0xBF58476D1CE4E5B9) & M
    k = ((k ^ (k >> 27)) * 0x94D049BB133111EB) & M
    return (k ^ (k >> 31)) >> 32


@pytest.mark.parametrize("counter", [None, 7])
def test_dropout_reference_against_python_integers(counter):
    n, seed = 1003, 1234
    x = torch.arange(1, n + 1).float()
    masks = {}
    for p in (0.0, 0.3, 0.5, 0.75, 1.0):
        mask, y, scale = hr.dropout_ref(x, p, seed, counter)
        s = seed if counter is None else seed ^ ((counter * 0xD1342543DE82EF95) & ((1 << 64) - 1))
        want = [(_mix32_int((s * 0x100000001B3 + i) & ((1 << 64) - 1)) >> 8) * 2.0 ** -24 >= float(np.float32(p)) for i in range(n)]
        assert mask.tolist() == [int(w) for w in want]
        assert abs(float(mask.float().mean()) - (1 - p)) < 0.05
        assert torch.equal(y, x.double() * scale * mask)
        masks[p] = mask
    assert masks[0.0].all() and not masks[1.0].any()
    assert not torch.equal(hr.dropout_ref(x, 0.5, seed, None)[0], hr.dropout_ref(x, 0.5, seed, 7)[0])


@pytest.mark.parametrize("case", hr.LINEAR_CASES)
def test_linear_reference_and_fp32_sums_within_half_the_bound(case):
    B, I, O, relu, _ = case
    d = hr.linear_case(B, I, O)
    x, w, b = (d[k].clone().requires_grad_(True) for k in ("x", "w", "bias"))
    z = F.linear(x, w, b)
    y = F.relu(z) if relu else z
    y.backward(d["dy"])
    ref, bnd = hr.linear_fwd_ref(d["x"], d["w"], d["bias"], relu)
    worst = [hr.check_bounded(y.detach(), ref, bnd)[0]]
    for beta in (0.0, 0.5, 1.0):
        out = hr.linear_bwd_ref(d["x"], d["w"], y.detach(), d["dy"], relu, beta, d["old_dw"], d["old_db"])
        worst.append(hr.check_bounded(x.grad, *out["dx"])[0])
        worst.append(hr.check_bounded(w.grad + np.float32(beta) * d["old_dw"], *out["dw"])[0])
        worst.append(hr.check_bounded(b.grad + np.float32(beta) * d["old_db"], *out["db"])[0])
    print(f"linear {case}: torch fp32 err/bound {max(worst):.3f}")
    assert max(worst) <= MARGIN


@pytest.mark.parametrize("n", hr.NORM_NS)
def test_norm_reference_and_restatement(n):
    g = hr.norm_case(n)
    ss = float((g.double() ** 2).sum())
    nrm, bnd = hr.norm_ref(ss, 0.25, 1 / 1024)
    assert abs(nrm - float(torch.linalg.vector_norm(g.double())) * 0.25 / 1024) <= 1e-12 * nrm
    emu = hr.emu_norm(g, hr.rowreduce_blocks(n), 0.25, 1 / 1024)
    r = abs(emu - nrm) / bnd
    c, cbnd = hr.coef_ref(nrm, bnd, 1.0)
    ce = float(np.minimum(np.float32(1), np.float32(1) / (np.float32(emu) + np.float32(1e-6))))
    rc = abs(ce - c) / cbnd if cbnd else float(ce != c)
    print(f"norm n={n}: restatement err/bound {r:.3f}, coef {rc:.3f}")
    assert r <= MARGIN and rc <= MARGIN
    assert hr.coef_ref(nrm, bnd, 0.0) == (1.0, 0.0) and hr.coef_ref(nrm, bnd, -1.0) == (1.0, 0.0)


@pytest.mark.parametrize("nblocks", hr.CLIP_NBLOCKS)
def test_clip_coef_restatement(nblocks):
    partial = hr.clip_case(nblocks)
    f = np.float32
    for inv, dev, mx in ((1.0, 1.0, 1.0), (0.5, 0.125, 2.5), (0.5, 0.125, -1.0)):
        nrm, bnd = hr.norm_ref(float(partial.double().sum()), inv, dev)
        c, cbnd = hr.coef_ref(nrm, bnd, mx)
        n32 = f(f(f(math.sqrt(float(partial.double().sum()))) * f(inv)) * f(dev))
        c32 = float(np.minimum(f(1), f(mx) / (n32 + f(1e-6)))) if mx > 0 else 1.0
        assert abs(float(n32) - nrm) <= MARGIN * bnd and abs(c32 - c) <= MARGIN * cbnd
        assert (cbnd > 0) == (mx > 0)


def test_pow_restatement():
    """numpy's float32 power against fp64, in units of 2^-24 relative: what POW_U leaves room for"""
    worst = 0.0
    for b in (0.9, 0.999):
        for t in range(1, 2000):
            got = float(np.power(np.float32(b), np.float32(t)))
            ref = float(np.float32(b)) ** t
            if ref < 1e-30:
                break
            worst = max(worst, abs(got - ref) / ref / hr.U24)
    print(f"float32 power: worst relative error {worst:.2f} x 2^-24 (POW_U = {hr.POW_U})")
    assert worst <= MARGIN * hr.POW_U


@pytest.mark.parametrize("n", hr.ADAMW_NS)
def test_adamw_reference_is_torch_adamw_and_restatement_within_half(n):
    p0, grads = hr.adamw_case(n)
    inv, dev = hr.ADAMW_SCALE
    hp = {k: hr.f32(v) for k, v in hr.ADAMW_HP.items()}
    # the reference, carried forward by itself, is torch.optim.AdamW in fp64 with the same float32-rounded scalars
    pt = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([pt], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pe, me, ve = p0.clone(), torch.zeros(n), torch.zeros(n)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for it, g in enumerate(grads):
        nrm, nb = hr.norm_ref(float((g.double() ** 2).sum()), inv, dev)
        coef = float(np.float32(hr.coef_ref(nrm, nb, 1.0)[0]))
        pt.grad = g.double() * (coef * hr.f32(inv) * hr.f32(dev))
        opt.step()
        out, delta = hr.adamw_ref(p, m, v, g, it + 1, coef, inv, dev, **hr.ADAMW_HP)
        p, m, v = out["p"][0], out["m"][0], out["v"][0]
        assert torch.allclose(p, pt.detach(), rtol=1e-12, atol=1e-15)
        # the float32 chain from ITS OWN previous state, against the fp64 step from that same state
        oe, _ = hr.adamw_ref(pe, me, ve, g, it + 1, coef, inv, dev, **hr.ADAMW_HP)
        pe, me, ve = hr.emu_adamw(pe, me, ve, g, it + 1, coef, inv, dev, **hr.ADAMW_HP)
        for k, got in (("p", pe), ("m", me), ("v", ve)):
            worst[k] = max(worst[k], hr.check_bounded(got, *oe[k])[0])
    print(f"adamw n={n}: restatement err/bound p {worst['p']:.3f}, m {worst['m']:.3f}, v {worst['v']:.3f}")
    assert max(worst.values()) <= MARGIN


@pytest.mark.parametrize("n", hr.BCE_NS)
def test_bce_reference_and_restatement(n):
    z, t = hr.bce_case(n)
    if n >= 1000:
        assert {hr.f32(e) for e in hr.BCE_EDGES} <= set(z.tolist()) and {0.0, 1.0, hr.f32(0.3)} <= set(t.tolist())
    zr = z.double().requires_grad_(True)
    lt = F.binary_cross_entropy_with_logits(zr, t.double())
    lt.backward()
    for gscale in (1.0, 1024.0):
        (loss, e_loss), (dz, e_dz) = hr.bce_ref(z, t, gscale)
        assert abs(loss - float(lt.detach())) <= 1e-12 * abs(loss) + 1e-15 and torch.allclose(dz, zr.grad * gscale, rtol=1e-12, atol=1e-300)
        l32, dz32 = hr.emu_bce(z, t, gscale)
        rl, rd = abs(l32 - loss) / e_loss, hr.check_bounded(dz32, dz, e_dz)[0]
        print(f"bce n={n} gscale={gscale:g}: restatement err/bound loss {rl:.3f}, dz {rd:.3f}")
        assert rl <= MARGIN and rd <= MARGIN


@pytest.mark.parametrize("sm", [0.0, 0.1])
@pytest.mark.parametrize("case", hr.CE_CASES)
def test_ce_reference_and_restatement(case, sm):
    B, C = case
    z, y = hr.ce_case(B, C)
    if C > 1:
        assert float((z.max(1).values - z.median(1).values).max()) > 50          # some rows hold one logit 60 above the rest
    zr = z.double().requires_grad_(True)
    lt = F.cross_entropy(zr, y, label_smoothing=hr.f32(sm))
    lt.backward()
    for gscale in (1.0, 1024.0):
        (loss, e_loss), (dz, e_dz) = hr.ce_ref(z, y, sm, gscale)
        assert abs(loss - float(lt.detach())) <= 1e-12 * abs(loss) + 1e-14 and torch.allclose(dz, zr.grad * gscale, rtol=1e-11, atol=1e-15 * gscale)
        l32, dz32 = hr.emu_ce(z, y, sm, gscale)
        rl, rd = abs(l32 - loss) / e_loss, hr.check_bounded(dz32, dz, e_dz)[0]
        print(f"ce {case} sm={sm} gscale={gscale:g}: restatement err/bound loss {rl:.3f}, dz {rd:.3f}")
        assert rl <= MARGIN and rd <= MARGIN


@pytest.mark.parametrize("B,per,is_logit,thr", [(3, 561, 1, 0.5), (3, 2049, 0, 0.3), (3, 2049, 1, 0.3)])
def test_seg_counts_reference(B, per, is_logit, thr):
    v, t = hr.seg_counts_case(B, per, is_logit, thr)
    c, margin = hr.seg_counts_ref(v, t, is_logit, thr)
    assert margin >= 1e-3
    pr = torch.sigmoid(v) if is_logit else v
    pb, tb = pr > thr, t > thr
    assert torch.equal(c[:, 1], pb.sum(1).double()) and torch.equal(c[:, 0], (pb & tb).sum(1).double())
    assert 0 < int(c[:, 1].sum()) < B * per and 0 < int(c[:, 2].sum()) < B * per


# ---- the checkers reject what they exist to catch ------------------------------------------------------------------------------------
def test_interval_checker():
    for dt in (BF, FP, F32):
        exact = torch.tensor([1.0 / 3, -1.0 / 3, 0.5, 3.0, -2.0 / 3, 1e-3], dtype=torch.float64)
        lo, hi = hr.storage_interval(exact, torch.zeros_like(exact), dt)
        assert torch.equal(lo.to(dt).double(), lo) and torch.equal(hi.to(dt).double(), hi)
        assert bool((lo <= exact).all()) and bool((hi >= exact).all())
        inexact = exact.to(dt).double() != exact
        assert torch.equal(lo == hi, ~inexact)
        assert bool(((hi - lo)[inexact] == cb.ulp(exact, dt)[inexact]).all())
        assert hr.check_interval(lo, exact, dt)[0] <= 1 and hr.check_interval(hi, exact, dt)[0] <= 1
        assert hr.check_interval(hi + cb.ulp(exact, dt), exact, dt)[0] > 1
        assert hr.check_interval(lo - cb.ulp(exact, dt), exact, dt)[0] > 1


def test_rejects_the_last_maximum_on_tied_data():
    k, s, p, H, W, _ = hr.MAXPOOL_CASES[1]
    x, dy, old = hr.maxpool_case(k, s, p, H, W)
    _, dx = hr.maxpool_ref(x, dy, k, s, p)
    _, last = hr.maxpool_ref(x.flip(2, 3), dy.flip(2, 3), k, s, p)              # the first maximum of the mirrored image
    assert hr.check_exact(dx, dx)[0] == 0 and hr.check_exact(last.flip(2, 3), dx)[0] == math.inf
    N, HW, C = 2, 20, 96
    x, dy = hr.global_case(N, HW, C)
    hr.plant_wave_ties(x)
    _, idx, _ = hr.global_pool_ref(x, dy, 1)
    _, idx_last, _ = hr.global_pool_ref(x.flip(1), dy, 1)
    assert hr.check_exact(HW - 1 - idx_last, idx)[0] == math.inf
    # the smaller WAVE instead of the smaller position (what a fold without the `vi < ri` rule gives)
    by_wave = torch.from_numpy(np.argmax(np.concatenate([x.numpy()[:, w::4] for w in range(4)], 1), 1))
    order = torch.cat([torch.arange(w, HW, 4) for w in range(4)])
    assert hr.check_exact(order[by_wave], idx)[0] == math.inf


def test_rejects_a_dropped_element_in_the_sum_of_squares():
    """the norm's bound sees one typical element missing up to n ~ 10^6 (its share of the norm is 1 / 2n against 8 * 2^-24); the
    all-ones count sees any single element at every n"""
    for n in hr.NORM_NS:
        g = hr.norm_case(n)
        sq = g.double() ** 2
        nrm, bnd = hr.norm_ref(float(sq.sum()))
        without = math.sqrt(float(sq.sum()) - float(sq.median()))
        assert hr.check_bounded(torch.tensor(nrm, dtype=torch.float64), nrm, bnd)[0] == 0
        if n <= 100_003:
            assert hr.check_bounded(torch.tensor(without, dtype=torch.float64), nrm, bnd)[0] > 1
        assert hr.check_exact(torch.tensor(float(n - 1)), torch.tensor(float(n)))[0] == math.inf
        assert float(np.float32(n)) == n                                           # the count itself is exact in fp32


def test_rejects_an_adamw_update_scaled_by_1_004():
    n = hr.ADAMW_NS[2]
    p0, grads = hr.adamw_case(n)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for it, g in enumerate(grads):
        out, delta = hr.adamw_ref(p, m, v, g, it + 1, 0.5, *hr.ADAMW_SCALE, **hr.ADAMW_HP)
        wrong = (p * (1 - hr.f32(1e-3) * hr.f32(5e-4)) - 1.004 * delta).float()
        ratio, _ = hr.check_bounded(wrong, *out["p"])
        over = ((wrong.double() - out["p"][0]).abs() > out["p"][1]).double().mean()
        assert ratio > 1 and over > 0.9, (it, ratio, float(over))                 # nearly every element, not one outlier
        assert gpu_util_rel_err(wrong, out["p"][0]) < 1e-6                        # ... which the old max-relative criterion passes
        p, m, v = out["p"][0], out["m"][0], out["v"][0]


def gpu_util_rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def test_rejects_a_bce_loss_missing_one_workgroup():
    n = hr.BCE_NS[-1]
    z, t = hr.bce_case(n)
    (loss, e_loss), _ = hr.bce_ref(z, t)
    zd, td = z.double(), t.double()
    l = zd.clamp(min=0) - zd * td + torch.log1p(torch.exp(-zd.abs()))
    blocks = 1024
    share = l[torch.arange(n) // 256 % blocks == 1023].sum() / n                  # the last workgroup's grid-stride share
    assert abs(float(share)) / e_loss > 1


def test_rejects_an_adaptive_window_off_by_one():
    for H, W, OH, OW, exact in hr.ADAPTIVE_CASES:
        if W == 1 or (H, W) == (7, 7) or (H, W) == (1, 2):
            continue
        x, dy = hr.adaptive_case(H, W, OH, OW)
        y, _, _ = hr.adaptive_avg_ref(x, dy, OH, OW)
        wrong = hr.adaptive_avg_plain(x, OH, OW, shift=1)
        assert hr.check_bounded(wrong, y, cb.ulp(y, F32))[0] > 1
        assert hr.check_bounded(hr.adaptive_avg_plain(x, OH, OW), y, cb.ulp(y, F32))[0] <= 1


def test_rejects_a_dropout_mask_from_another_seed():
    x = torch.ones(1003)
    m0, y0, _ = hr.dropout_ref(x, 0.5, 1234)
    m1, y1, _ = hr.dropout_ref(x, 0.5, 1235)
    assert hr.check_exact(m0, m0)[0] == 0 and hr.check_exact(m1, m0)[0] == math.inf and hr.check_exact(y1, y0)[0] == math.inf
