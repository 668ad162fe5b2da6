"""-m gpu: weight averaging (csrc/weight_avg.hip, mi355/averaging.py) through the C ABI, ``WeightAverage`` / ``update_bn`` on real models,
``train(model, WithAveraging(train_dl, ...), ...)`` and the tester's ``weights_variant``, against the numpy restatement tests/averaging_ref.py (pinned by
tests/test_averaging_cpu.py).

The update and the exchange are +, -, * and moves, every operation rounded on its own: they are compared BYTE FOR BYTE.  The bias
correction divides in double and rounds once: one float32 ulp against the fp64 restatement.  Every buffer a kernel writes lies between
guard bands of a NaN bit pattern inside one allocation, and the WHOLE allocation is compared with what the restatement expects."""
import os
import re

import numpy as np
import pytest
import torch

import averaging_ref as R
from mi355.lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 8                                   # guard words on either side of a row (a multiple of 4: the shift alone sets the alignment)
NANW = 0x7FC5A5A5                       # a quiet NaN with a payload no arithmetic produces
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def _values(n, seed):
    """random float32 with the awkward ones mixed in: zeros of both signs, denormals, a large and a tiny normal"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(f32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, 1.5e30, 1.2e-38], f32)
    idx = rng.permutation(n)[: min(n // 3, 3 * len(special))]
    v[idx] = special[np.arange(len(idx)) % len(special)]
    return v


class Arena:
    """rows of float32 inside ONE device allocation, each behind G guard words and ``shift`` floats off a 16-byte boundary"""

    def __init__(self, rows, shifts):
        self.off, pos = [], 0
        for v, sh in zip(rows, shifts):
            pos = (pos + G + 3) // 4 * 4 + sh
            self.off.append(pos)
            pos += len(v)
        self.host = np.full((pos + 3) // 4 * 4 + G, NANW, np.int32)
        self.put(self.host, rows)
        self.dev = torch.from_numpy(self.host.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.n = [len(v) for v in rows]

    def put(self, whole, rows):
        for o, v in zip(self.off, rows):
            whole[o:o + len(v)] = _bits(v)
        return whole

    def ptr(self, i):
        return self.dev.data_ptr() + 4 * self.off[i]

    def row(self, i):
        return self.dev[self.off[i]:self.off[i] + self.n[i]].view(torch.float32)

    def holds(self, rows):
        """the whole allocation — rows AND guard bands — is what ``rows`` say"""
        return np.array_equal(self.dev.cpu().numpy(), self.put(self.host.copy(), rows))


def _i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _finf(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


# ---- mi355_avg_update -----------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 255, 256, 257, 4 * 1023 + 1]
CASES = [(R.EMA, 1), (R.EMA, 5), (R.EMA, 10 ** 4), (R.EQUAL, 1), (R.EQUAL, 7)]      # warm-up active twice, decay-limited; copy, 1 / 7
SHIFTS = [(0, 0), (1, 0), (0, 1), (1, 1)]                                            # (avg, p) floats off a 16-byte boundary


def _update_once(n, sa, sp, mode, t, finf=None, seed=0):
    avg, p = _values(n, seed), _values(n, seed + 1)
    A, P = Arena([avg], [sa]), Arena([p], [sp])
    count = _i32(t)
    lib.mi355_avg_update(A.row(0), P.row(0), n, mode, 0.999, 10.0, count, _finf(finf))
    torch.cuda.synchronize()
    want = R.update(avg, p, mode, t, 0.999, 10.0, found_inf=finf or 0.0)
    return A.holds([want]), P.holds([p]), int(count.item())


@pytest.mark.parametrize("sa,sp", SHIFTS)
@pytest.mark.parametrize("mode,t", CASES)
def test_avg_update_is_the_restatement_byte_for_byte(mode, t, sa, sp):
    for n in SIZES:
        ok, src_ok, cnt = _update_once(n, sa, sp, mode, t, seed=n)
        assert ok and src_ok and cnt == t, (n, mode, t, sa, sp)


@pytest.mark.parametrize("sa,sp", [(0, 0), (1, 1), (1, 0)])
def test_avg_update_past_one_full_sweep_of_the_grid(sa, sp):
    """the launcher caps its grid: a range a few elements longer than one sweep sends the first threads round the stride loop"""
    n = lib.mi355_avg_update_grid_elems() + 4 * 3 + 1
    for mode, t in ((R.EMA, 5), (R.EQUAL, 1)):
        assert _update_once(n, sa, sp, mode, t, seed=3) == (True, True, t)


@pytest.mark.parametrize("mode", [R.EMA, R.EQUAL])
def test_found_inf_leaves_every_byte_and_the_count(mode):
    for n, sa, sp in ((257, 0, 0), (5, 1, 0), (4093, 1, 1)):
        avg, p = _values(n, 5), _values(n, 6)
        A, P = Arena([avg], [sa]), Arena([p], [sp])
        count, finf = _i32(3), _finf(1.0)
        lib.mi355_step_tick(count, finf)
        lib.mi355_avg_update(A.row(0), P.row(0), n, mode, 0.999, 10.0, count, finf)
        assert A.holds([avg]) and P.holds([p]) and int(count.item()) == 3
        finf.zero_()                                                   # the same launches with found_inf = 0 do count and write
        lib.mi355_step_tick(count, finf)
        lib.mi355_avg_update(A.row(0), P.row(0), n, mode, 0.999, 10.0, count, finf)
        assert int(count.item()) == 4 and A.holds([R.update(avg, p, mode, 4, 0.999, 10.0)])
    A = Arena([_values(8, 1)], [0])
    lib.mi355_avg_update(A.row(0), A.row(0), 0, mode, 0.999, 10.0, _i32(2), None)         # n == 0: OK, nothing happens
    assert A.holds([_values(8, 1)])


@pytest.mark.parametrize("mode,sa,sp", [(R.EMA, 0, 0), (R.EMA, 1, 0), (R.EQUAL, 1, 1)])
def test_a_chain_of_twenty_updates(mode, sa, sp):
    n = 4 * 1023 + 1
    avg = _values(n, 40)
    A = Arena([avg], [sa])
    count = _i32(0)
    for t in range(1, 21):
        p = _values(n, 40 + t)
        P = Arena([p], [sp])
        lib.mi355_step_tick(count, None)
        lib.mi355_avg_update(A.row(0), P.row(0), n, mode, 0.9, 4.0, count, None)
        avg = R.update(avg, p, mode, R.tick(t - 1), 0.9, 4.0)
        torch.cuda.synchronize()
    assert int(count.item()) == 20 and A.holds([avg])


@pytest.mark.parametrize("mode,t", [(R.EMA, 5), (R.EMA, 10 ** 4), (R.EQUAL, 7)])
def test_equal_inputs_keep_their_bits(mode, t):
    """p == avg bit for bit (padding, frozen parameters): -0.0, +0.0 and denormals included — avg + a * 0 alone would turn -0 into +0"""
    v = np.tile(np.array([-0.0, 0.0, 1e-42, -1e-45, 1.0, -3.5e-39, 7e37, 1.17549435e-38], f32), 33)[:259]
    for sa, sp in SHIFTS:
        A, P = Arena([v], [sa]), Arena([v], [sp])
        lib.mi355_avg_update(A.row(0), P.row(0), len(v), mode, 0.999, 10.0, _i32(t), None)
        assert A.holds([v]) and P.holds([v])


# ---- the table launchers --------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 3, 64, 2048]


def _table_case(rows):
    """-> (dst arena, src arena, their rows, the device table): lengths cycle through LENGTHS, every third row starts one float off
    on both sides (head / tail path), every fifth on the destination alone (scalar path)"""
    ns = [LENGTHS[(i + i // 4 + 3) % 4] for i in range(rows)]          # (the one-row case is the longest)
    d = [_values(n, 100 + i) for i, n in enumerate(ns)]
    s = [_values(n, 900 + i) for i, n in enumerate(ns)]
    sd = [1 if (i % 3 == 1 or i % 5 == 2) else 0 for i in range(rows)]
    ss = [1 if i % 3 == 1 and i % 5 != 2 else 0 for i in range(rows)]
    D, S = Arena(d, sd), Arena(s, ss)
    table = torch.tensor([[D.ptr(i), S.ptr(i), ns[i]] for i in range(rows)], dtype=torch.int64).to(DEV)
    return D, S, d, s, table


@pytest.mark.parametrize("rows", [1, 130])
def test_avg_update_table_is_the_restatement_byte_for_byte(rows):
    for mode, t, finf in ((R.EMA, 5, None), (R.EQUAL, 1, 0.0), (R.EQUAL, 7, None), (R.EMA, 3, 1.0)):
        D, S, d, s, table = _table_case(rows)
        lib.mi355_avg_update_table(table, rows, mode, 0.999, 10.0, _i32(t), _finf(finf))
        want = [R.update(a, b, mode, t, 0.999, 10.0, found_inf=finf or 0.0) for a, b in zip(d, s)]
        assert D.holds(want) and S.holds(s), (rows, mode, t, finf)
        if finf:
            assert D.holds(d)


@pytest.mark.parametrize("rows", [1, 130])
def test_swap_table_exchanges_and_twice_is_the_identity(rows):
    D, S, d, s, table = _table_case(rows)
    lib.mi355_swap_table(table, rows)
    assert D.holds(s) and S.holds(d)
    lib.mi355_swap_table(table, rows)
    assert D.holds(d) and S.holds(s)


def test_swap_table_on_a_row_longer_than_its_grid():
    """the flat parameter buffer is one row: longer than one sweep of the row's workgroups, one float off on both sides"""
    n = 512 * 256 * 4 + 4 * 7 + 2
    d, s = _values(n, 1), _values(n, 2)
    D, S = Arena([d], [1]), Arena([s], [1])
    table = torch.tensor([[D.ptr(0), S.ptr(0), n]], dtype=torch.int64).to(DEV)
    lib.mi355_swap_table(table, 1)
    assert D.holds([s]) and S.holds([d])


def test_bn_debias_table_within_one_ulp_and_k_zero_untouched():
    ks = [0, 1, 2, 50, 4000]
    Cs = [1, 3, 64, 600]                                        # 600: more channels than one sweep of the row's workgroups
    rows = [(k, C) for k in ks for C in Cs]
    run = [_values(C, 7 * i) for i, (k, C) in enumerate(rows)]
    run = [np.where(np.abs(r) > 1e20, f32(1.0), r).astype(f32) for r in run]          # (1.5e30 / 0.1 is still finite; keep it tame)
    A = Arena(run, [i % 2 for i in range(len(rows))])
    nbt = torch.tensor([k for k, _ in rows], dtype=torch.int64).to(DEV)
    table = torch.tensor([[A.ptr(i), nbt.data_ptr() + 8 * i, C] for i, (_, C) in enumerate(rows)], dtype=torch.int64).to(DEV)
    lib.mi355_bn_debias_table(table, len(rows), 0.1)
    whole = A.dev.cpu().numpy()
    got = [whole[o:o + n].view(f32) for o, n in zip(A.off, A.n)]
    assert A.holds(got)                                         # the guard bands
    assert nbt.cpu().tolist() == [k for k, _ in rows]
    for (k, C), r, g in zip(rows, run, got):
        want32, exact = R.bn_debias(r, k, 0.1)
        if k == 0:
            assert np.array_equal(_bits(g), _bits(r)), (k, C)
        else:
            assert np.all(np.abs(g.astype(np.float64) - exact) <= np.spacing(np.abs(want32)).astype(np.float64)), (k, C)


# ---- WeightAverage on real models ---------------------------------------------------------------------------------------------------
def _model(name, seed=0):
    from utils.helpers import get_seg_model
    torch.manual_seed(seed)
    m = get_seg_model(name)
    if name == "r2unet":
        m.compute_dtype = torch.float32          # (the Attention U-Net runs in the default bf16: its eval plans cache packed weights)
    return m


def _batches(k, bs=2, hw=32):
    from oracle import train as otrain
    return [otrain.synthetic_batch(bs, hw, seed=s) for s in range(k)]


def _state_bits(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def _same_state(a, b):
    return set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", ["attentionunet", "r2unet"])
def test_weight_average_follows_the_restatement_and_swaps_exactly(name):
    from mi355 import nn as mnn, optim as moptim
    from mi355.averaging import WeightAverage
    m = _model(name).to(DEV).train()
    eng = m.engine
    opt = moptim.AdamW(m.parameters(), lr=1e-3, weight_decay=5e-4)
    avg = WeightAverage(m, mode="ema", decay=0.9, warmup=2)
    ref = eng.flat_p.cpu().numpy().copy()
    assert np.array_equal(_bits(avg.flat.cpu().numpy()), _bits(ref))
    fnames = [k for k, b in m.named_buffers() if b.is_floating_point()]
    ref_buf = {k: dict(m.named_buffers())[k].cpu().numpy().copy() for k in fnames}
    crit = mnn.BCEWithLogitsLoss()
    for t, (x, y) in enumerate(_batches(3), 1):
        opt.zero_grad(set_to_none=True)
        out = m(x.to(DEV))
        crit(out if out.dim() == 4 else out.unsqueeze(1), y.to(DEV)).backward()
        moptim.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()
        avg.update(opt)
        ref = R.update(ref, eng.flat_p.cpu().numpy(), R.EMA, t, 0.9, 2.0)
        live = dict(m.named_buffers())
        ref_buf = {k: R.update(ref_buf[k], live[k].cpu().numpy(), R.EMA, t, 0.9, 2.0) for k in fnames}
    assert int(avg.count.item()) == 3
    assert np.array_equal(_bits(avg.flat.cpu().numpy()), _bits(ref))
    assert not np.array_equal(_bits(ref), _bits(eng.flat_p.cpu().numpy()))
    sd = avg.state_dict()
    assert sd["count"] == 3 and sd["mode"] == "ema" and all(np.array_equal(_bits(sd["buffers"][k].cpu().numpy()), _bits(ref_buf[k])) for k in fnames)
    for k, p in m.named_parameters():
        o, n = eng.offsets[id(p)]
        assert np.array_equal(_bits(sd["params"][k].cpu().numpy()).ravel(), _bits(ref[o:o + n])), k

    # swap(): the model IS the averaged model — the same launches on the same packed weights as a fresh model loaded from the checkpoint
    x = _batches(4)[3][0].to(DEV)
    m.eval()
    with torch.no_grad():
        out_live = m(x).clone()                  # (also fills the eval plan's weight packs with the LIVE weights)
    before = _state_bits(m)
    asd = avg.averaged_state_dict()
    assert list(asd) == list(m.state_dict())
    fresh = _model(name, seed=1)
    fresh.load_state_dict(asd)
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        out_fresh = fresh(x).clone()
        with avg.swap():
            out_swapped = m(x).clone()
            assert _same_state(_state_bits(m), {k: v.cpu().numpy() for k, v in asd.items()})
        out_after = m(x).clone()
    assert torch.equal(out_swapped, out_fresh) and not torch.equal(out_swapped, out_live)
    assert _same_state(_state_bits(m), before) and torch.equal(out_after, out_live)
    # a second average resumes from the checkpoint
    other = WeightAverage(m, mode="ema", decay=0.5, warmup=0)
    other.load_state_dict(sd)
    assert int(other.count.item()) == 3 and other.decay == 0.9 and torch.equal(other.flat, avg.flat)


# ---- update_bn ----------------------------------------------------------------------------------------------------------------------------
def _bns(m):
    return [(k, b) for k, b in m.named_modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]


def test_update_bn_is_the_bias_corrected_weighted_mean_of_the_batch_statistics():
    """Single-firing model, K = 3 batches of 2 x 3 x 32^2.  Each batch's statistics b_k come from the GPU itself (reset, one train-mode
    forward, running / momentum: one float32 rounding each); their fp64 combination with the bias-corrected weights is compared with
    update_bn's result under |diff| <= (K + 2) 2^-24 max_k |b_k| per channel: the finalize rounds to float32 once per update (K), the
    correction once, the measured b_k once."""
    from mi355.averaging import update_bn
    K = 3
    m = _model("attentionunet").to(DEV)
    xs = [x for x, _ in _batches(K)]
    mom = float(f32(0.1))
    per_batch = []
    for x in xs:
        for _, b in _bns(m):
            b.running_mean.zero_()
            b.running_var.zero_()
            b.num_batches_tracked.zero_()
        m.train()
        with torch.no_grad():
            m(x.to(DEV))
        assert all(b.momentum == 0.1 for _, b in _bns(m))
        per_batch.append({k: (b.running_mean.cpu().numpy().astype(np.float64) / mom, b.running_var.cpu().numpy().astype(np.float64) / mom,
                              int(b.num_batches_tracked.item())) for k, b in _bns(m)})
    m.eval()
    assert update_bn(m, [(x, None) for x in xs], DEV) == K and not m.training
    checked = 0
    for k, b in _bns(m):
        assert int(b.num_batches_tracked.item()) == K and all(v[k][2] == 1 for v in per_batch)
        for j, r in ((0, b.running_mean), (1, b.running_var)):
            bk = np.stack([v[k][j] for v in per_batch])
            want = R.bn_weighted_mean(bk, 0.1)
            diff = np.abs(r.cpu().numpy().astype(np.float64) - want)
            bound = (K + 2) * 2.0 ** -24 * np.abs(bk).max(0)
            assert np.all(diff <= bound), (k, j, float((diff / np.maximum(bound, 1e-300)).max()))
            checked += r.numel()
        assert float(b.running_var.min()) >= 0
    assert checked > 1000


def test_update_bn_counts_every_firing_of_the_recurrent_blocks():
    from mi355.averaging import update_bn
    K = 3
    m = _model("r2unet").to(DEV)
    xs = [x for x, _ in _batches(K)]
    update_bn(m, xs[:1], DEV)
    firings = {k: int(b.num_batches_tracked.item()) for k, b in _bns(m)}
    assert max(firings.values()) > 1 and min(firings.values()) >= 1
    assert update_bn(m, xs, DEV, max_batches=K) == K
    first = _state_bits(m)
    for k, b in _bns(m):
        assert int(b.num_batches_tracked.item()) == firings[k] * K, k
        assert bool(torch.isfinite(b.running_mean).all()) and bool(torch.isfinite(b.running_var).all())
    update_bn(m, xs, DEV)
    assert _same_state(_state_bits(m), first)


# ---- train(), the checkpoints, the tester ---------------------------------------------------------------------------------------------
NAME = "AttentionUNet"


def _strip_time(text):
    return re.sub(r"finished in [\d.]+ minutes", "finished", text)


def _seg_loaders():
    from torch.utils.data import DataLoader, TensorDataset
    from oracle import train as otrain
    b = [otrain.synthetic_batch(4, 32, seed=s) for s in (0, 1, 2)]
    x, y = torch.cat([v[0] for v in b]), torch.cat([v[1] for v in b])
    return (DataLoader(TensorDataset(x[:8], y[:8]), batch_size=4, shuffle=True), DataLoader(TensorDataset(x[8:], y[8:]), batch_size=4, shuffle=False))


def _train_model():
    from utils.helpers import get_seg_model
    torch.manual_seed(5)
    m = get_seg_model("attentionunet")
    m.compute_dtype = torch.float32
    return m


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """two epochs of train() at the shape of tests/test_gpu_mix.py's segmentation run (AttentionUNet fp32, 8 + 4 synthetic samples of
    32 x 32, batches of 4, a SHUFFLING training loader): twice without averaging, once with an EMA, once with SWA from epoch 1"""
    import contextlib
    import io
    from mi355.averaging import WithAveraging
    from utils import helpers
    out = {}
    for tag, averaging in (("plain", None), ("again", None), ("ema", {"mode": "ema", "decay": 0.9, "warmup": 2}),
                           ("swa", {"mode": "swa", "swa_start": 1})):
        d = str(tmp_path_factory.mktemp(tag))
        tr, va = _seg_loaders()
        model = _train_model()
        torch.manual_seed(7)                      # the training loader shuffles from the host generator
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            best = helpers.train(model, tr if averaging is None else WithAveraging(tr, averaging), va, torch.device(DEV), 2, 1e-4, NAME, d, seg=True)
        out[tag] = (d, _strip_time(buf.getvalue()), best)
    return out


def _load(d, fname):
    return torch.load(os.path.join(d, fname), map_location="cpu")


def _same_sd(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_train_with_ema_leaves_the_raw_run_alone(runs):
    """Two runs of train() without averaging at this shape print identical lines and save identical tensors (established here, on
    an MI355X: the engine's kernels sum in a fixed order) — asserted first, so that a loss of determinism fails this test instead
    of weakening it.  The run with an EMA must then print the same raw lines, return the same best score and save the same
    {name}_best_loss.pt, bit for bit, although the training loader shuffles from the host generator."""
    (d0, t0, b0), (d1, t1, b1), (de, te, be) = runs["plain"], runs["again"], runs["ema"]
    raw = "\n".join(l for l in te.splitlines() if "EMA" not in l) + "\n"
    deterministic = t0 == t1 and b0 == b1 and _same_sd(_load(d0, f"{NAME}_best_loss.pt"), _load(d1, f"{NAME}_best_loss.pt"))
    assert deterministic
    assert raw == t0 and be == b0
    assert _same_sd(_load(de, f"{NAME}_best_loss.pt"), _load(d0, f"{NAME}_best_loss.pt"))
    assert sorted(os.listdir(d0)) == [f"{NAME}_best_loss.pt"]


def test_train_with_ema_logs_and_saves_the_averaged_model(runs):
    from mi355 import nn as mnn
    d, text, _ = runs["ema"]
    lines = re.findall(rf"^\[{NAME}\] Ep(\d+): EMA ValLoss ([\d.]+) \| IoU ([\d.]+)$", text, flags=re.M)
    assert [e for e, _, _ in lines] == ["1", "2"]
    assert len(re.findall(r"Ep\d+: TrainLoss", text)) == 2
    assert sorted(os.listdir(d)) == [f"{NAME}_best_loss.pt", f"{NAME}_ema_best_loss.pt"]
    best = min(lines, key=lambda l: (float(l[1]), int(l[0])))               # the first epoch with the lowest averaged loss was saved
    m = _train_model()
    m.load_state_dict(_load(d, f"{NAME}_ema_best_loss.pt"))
    m = m.to(DEV).eval()
    _, va = _seg_loaders()
    crit, tot = mnn.BCEWithLogitsLoss(), torch.zeros((), device=DEV)
    with torch.no_grad():
        for x, y in va:
            out = m(x.to(DEV))
            tot += crit(out if out.dim() == 4 else out.unsqueeze(1), y.to(DEV)) * x.size(0)
    assert f"{tot.item() / len(va.dataset):.3f}" == best[1]
    assert not _same_sd(_load(d, f"{NAME}_ema_best_loss.pt"), _load(d, f"{NAME}_best_loss.pt"))


def test_train_with_swa_saves_re_estimated_statistics(runs):
    d, text, _ = runs["swa"]
    assert len(re.findall(rf"^\[{NAME}\] SWA \(2 epochs\): ValLoss [\d.]+ \| IoU [\d.]+$", text, flags=re.M)) == 1
    assert "EMA" not in text and sorted(os.listdir(d)) == [f"{NAME}_best_loss.pt", f"{NAME}_swa.pt"]
    swa, raw = _load(d, f"{NAME}_swa.pt"), _load(d, f"{NAME}_best_loss.pt")
    assert list(swa) == list(raw)
    stats = [k for k in swa if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(stats) > 20 and all(bool(torch.isfinite(swa[k]).all()) for k in stats)
    assert all(not torch.equal(swa[k], raw[k]) for k in stats)
    assert all(int(swa[k]) == 2 for k in swa if k.endswith("num_batches_tracked"))         # two training batches re-estimated them
    m = _train_model()
    m.load_state_dict(swa)


def test_tester_reads_the_variant_it_is_asked_for(runs, tmp_path, capsys):
    import shutil
    from torch.utils.data import DataLoader, TensorDataset
    from oracle import train as otrain
    from utils import tester

    def _same(a, b):
        if isinstance(a, dict):
            return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
        if isinstance(a, (np.ndarray, float, tuple, list)):
            return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
        return a == b
    d = runs["ema"][0]
    xs, ms = zip(*[otrain.synthetic_batch(4, 32, seed=s) for s in (1, 2)])
    seg_dl = DataLoader(TensorDataset(torch.cat(xs), torch.cat(ms)), batch_size=4)
    cls_dl = DataLoader(TensorDataset(torch.cat(xs), torch.tensor([0, 1, 2, 1, 0, 2, 1, 0])), batch_size=4)
    empty, only_ema = tmp_path / "cls", tmp_path / "only_ema"
    empty.mkdir()
    only_ema.mkdir()
    shutil.copy(os.path.join(d, f"{NAME}_ema_best_loss.pt"), only_ema / f"{NAME}_ema_best_loss.pt")
    kw = dict(cls_loader=cls_dl, seg_loader=seg_dl, cls_weights_dir=str(empty))
    capsys.readouterr()
    plain = tester.test_all_models("cuda", 4, seg_weights_dir=d, **kw)
    plain_text = capsys.readouterr().out
    raw = tester.test_all_models("cuda", 4, seg_weights_dir=d, weights_variant="raw", **kw)
    raw_text = capsys.readouterr().out
    assert set(plain) == {NAME} and _same(raw, plain) and raw_text == plain_text                 # the default is what it was
    # a directory that holds the averaged checkpoint alone: found under "ema", missing (the usual message) under the default
    ema = tester.test_all_models("cuda", 4, seg_weights_dir=str(only_ema), weights_variant="ema", **kw)
    ema_text = capsys.readouterr().out
    assert set(ema) == {NAME} and "Weights not found for " + NAME + ":" not in ema_text
    none = tester.test_all_models("cuda", 4, seg_weights_dir=str(only_ema), **kw)
    none_text = capsys.readouterr().out
    assert none == {} and f"[WARNING] Weights not found for {NAME}: {only_ema / (NAME + '_best_loss.pt')}" in none_text
    assert _same(tester.test_all_models("cuda", 4, seg_weights_dir=d, weights_variant="ema", **kw), ema)
    swa_text = (tester.test_all_models("cuda", 4, seg_weights_dir=d, weights_variant="swa", **kw), capsys.readouterr().out)
    assert swa_text[0] == {} and f"{NAME}_swa.pt" in swa_text[1]
    with pytest.raises(ValueError, match="weights_variant"):
        tester.test_all_models("cuda", 4, seg_weights_dir=d, weights_variant="best", **kw)


@pytest.mark.parametrize("flags,variant", [(["--ema-decay", "0.9", "--ema-warmup", "2"], "ema"), (["--swa-start", "1"], "swa")])
def test_trainer_command_line_trains_saves_and_calibrates_the_averaged_model(flags, variant, tmp_path, capsys, monkeypatch):
    from utils import trainer
    monkeypatch.setattr("sys.argv", ["trainer.py", "--task", "seg", "--model", "attentionunet", "--epochs", "2", "--samples", "15", "--size", "32",
                                     "--lr", "1e-4", "--save-dir", str(tmp_path), "--calibrate"] + flags)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    trainer.main()
    text = capsys.readouterr().out
    d = tmp_path / "segmentation_models"
    ckpt = "attentionunet_ema_best_loss.pt" if variant == "ema" else "attentionunet_swa.pt"
    assert sorted(os.listdir(d)) == sorted(["attentionunet_best_loss.pt", "attentionunet_calibration.json", ckpt,
                                            f"attentionunet_{variant}_calibration.json"])
    assert len(re.findall(r"Ep\d+: EMA ValLoss", text)) == (2 if variant == "ema" else 0)
    assert len(re.findall(r"SWA \(2 epochs\): ValLoss", text)) == (0 if variant == "ema" else 1)
    assert text.count("[calibration] attentionunet: ") == 1 and text.count(f"[calibration] attentionunet_{variant}: ") == 1


def test_a_replaced_buffer_is_seen_and_the_tables_are_rebuilt():
    """``Module._apply`` (``.to()``, ``.float()``) and a re-registered buffer put NEW tensors into the modules: the next update must
    not write through the old pointers"""
    from mi355.averaging import WeightAverage
    m = _model("attentionunet").to(DEV)
    avg = WeightAverage(m, mode="ema", decay=0.5, warmup=0)
    name, first = next((k, b) for k, b in m.named_buffers() if b.is_floating_point())
    mod = m.get_submodule(name.rsplit(".", 1)[0])
    old_ptr, old_table = first.data_ptr(), avg._tab_update
    assert int(old_table[0, 1]) == old_ptr
    setattr(mod, name.rsplit(".", 1)[1], torch.full_like(first, 3.0))                     # a new tensor under the same name
    new = dict(m.named_buffers())[name]
    assert new.data_ptr() != old_ptr
    keep = first.clone()
    avg.update()
    assert avg._tab_update is not old_table and int(avg._tab_update[0, 1]) == new.data_ptr()
    want = R.update(keep.cpu().numpy(), new.cpu().numpy(), R.EMA, 1, 0.5, 0.0)              # avg copy (the old values) towards 3.0
    assert np.array_equal(_bits(avg._fbuf[name].cpu().numpy()), _bits(want)) and torch.equal(first, keep)
    with avg.swap():
        assert np.array_equal(_bits(dict(m.named_buffers())[name].cpu().numpy()), _bits(want))
    assert bool((dict(m.named_buffers())[name] == 3.0).all())
