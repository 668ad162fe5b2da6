"""CPU checks of tests/gate_exact.py, the instrument of tests/test_gpu_gate_exact.py: every case the GPU file builds passes the
generators' exactness assertions and carries its sensitivity witness; float32 accumulation in three orders reproduces the fp64
references bit for bit; the sigmoid classes hold; the references agree with torch autograd on random real data; and the host
queries the GPU file relies on answer as include/mi355conv.h says."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gate_exact as ge
import stream_exact as se
from mi355 import lib as L

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF, FP]
_dn = lambda d: str(d).split(".")[-1]                                           # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    ge.clear_cases()


def _orders(n, seed):
    return [np.arange(n), np.arange(n)[::-1], np.random.default_rng(seed).permutation(n)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_every_case_is_exact_order_independent_and_sensitive(dtype):
    """builds every case of the GPU file (the factories assert exactness and search for a full witness), then re-checks the witness
    and accumulates in float32 in three orders — the channel dot products of the window kernels, the row sums of the reductions"""
    n = 0
    for factory, args in ge.case_specs(dtype):
        c = factory(*args)
        assert c.epc == se.EPC[dtype] or c.op == "bn1_bwd_apply"
        if c.M * c.C <= 1 << 16:
            assert c.blind_spots() == [], (c.op, args)                         # (the factory searched for it: re-checked where it is cheap)
        for name, r in c.rows.items():
            se.assert_storable(r, dtype if r.dim() == 2 else F32, name)
        for o in c.outs.values():
            se.assert_storable(o, dtype if o.dim() == 2 else F32, c.op)
        n += 1
        if c.M * c.C > 1 << 20:
            continue
        if c.acc == "f32":
            want = c.sums()
            for k, t in c.terms.items():
                for order in _orders(c.M, n):
                    assert torch.equal(ge.f32_sums_in_order(t, order), want[k]), (c.op, args, k)
        if c.op in ("rowdot_fwd", "gate_psi_fwd"):
            p = c.rows["x"] if c.op == "rowdot_fwd" else ge.psi_in(c.rows, c.cons, "x1" in c.rows)
            prod = (p * c.cons["w"]).t().contiguous()
            for order in _orders(c.C, n):
                z = ge.f32_sums_in_order(prod, order) + c.cons["b"]
                assert torch.equal(z, c.outs["z"]), (c.op, args)
        if c.op == "gate_mul_bwd":
            prod = (c.rows["dy"] * c.rows["x"]).t().contiguous()
            psi = ge._psi_of(c.rows["z"], c.cons)
            for order in _orders(c.C, n):
                assert torch.equal(ge.f32_sums_in_order(prod, order) * psi * (1 - psi), c.outs["dzn"])
    print(f"{_dn(dtype)}: {n} cases")
    assert n > 200


def test_witness_refuses_blind_operands():
    """a last row of zeros, equal first rows, a weight that is zero on the last chunk: each is reported"""
    c = ge.rowdot_fwd_case(16, 8, 9)
    rows, cons = {k: v.clone() for k, v in c.rows.items()}, {k: v.clone() for k, v in c.cons.items()}
    cons["w"][8:] = 0
    blind = ge.Case("rowdot_fwd", 9, 16, 8, rows, cons, c.fn, c.check, "f64").blind_spots()
    assert ("zero_last_chunk", "z") in blind and ("zero_last_chunk", "s0") in blind
    rows["x"][1] = rows["x"][0]
    assert ("dup_row0", "z") in ge.Case("rowdot_fwd", 9, 16, 8, rows, c.cons, c.fn, c.check, "f64").blind_spots()
    rows = {"x": c.rows["x"].clone()}
    rows["x"][8] = 0
    cons = dict(c.cons, b=torch.zeros(1, dtype=torch.float64))
    assert ("drop_last_row", "s0") in ge.Case("rowdot_fwd", 9, 16, 8, rows, cons, c.fn, c.check, "f64").blind_spots()
    with pytest.raises(AssertionError):
        ge.assert_f64_sum_exact(torch.full((4, 1), 2.0 ** 52, dtype=torch.float64), 1.0)
    with pytest.raises(AssertionError):
        ge.assert_f64_sum_exact(torch.full((4, 1), 0.3, dtype=torch.float64), 0.25)


def test_sigmoid_classes():
    for a, want in zip(ge.PSI_ARGS, ge.PSI_CLASS):
        assert float(np.float32(1.0 / (1.0 + math.exp(-a)))) == want
        # ... and in float32 arithmetic with an exponential that saturates: exp(128) = inf, exp(-128) = 0 in fp32
        with np.errstate(over="ignore"):
            e = np.exp(np.float32(-a), dtype=np.float32)
        assert float(np.float32(1) / (np.float32(1) + e)) == want
    assert ge.sigmoid_classes_hold()
    g = torch.Generator().manual_seed(1)
    for M in (1, 2, 3, 50):
        cls = ge.class_rows(g, M)
        assert bool((cls[1:] != cls[:-1]).all())
    assert set(ge.class_rows(g, 50).tolist()) == {0, 1, 2}
    for i in range(len(ge.GATE_AFFINE)):
        z, scale, shift = ge._gate_z(g, 40, i)
        assert set((z * scale + shift).tolist()) == set(ge.PSI_ARGS)


def test_plane_index_is_the_header_contract():
    K, hw, N = 3, 37, 5
    idx = ge.plane_index(N * hw, hw, K)
    full = torch.arange(N * K * hw).reshape(N, K, hw)
    for k in range(K):
        assert torch.equal(full[:, k].reshape(-1), idx + k * hw)


def _close(a, b, tol=1e-10):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * (1 + float(b.abs().max()))


def test_references_match_autograd_on_real_data():
    """the gate's tail in fp64 torch: psi_in = relu(bn_g + bn_x), z = conv1x1, zn = bn1(z), y = x * sigmoid(zn) — against the
    references fed with the same constants (real data: _psi_of is replaced by the sigmoid itself)"""
    g = torch.Generator().manual_seed(5)
    M, C = 60, 12
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)              # noqa: E731
    g1, x1, xs = rn(M, C).requires_grad_(True), rn(M, C).requires_grad_(True), rn(M, C).requires_grad_(True)
    gam = {k: (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) for k in "gx"}
    bet = {k: rn(C) for k in "gx"}
    w, b = rn(C).requires_grad_(True), rn(1).requires_grad_(True)
    g1n = F.batch_norm(g1.t().unsqueeze(0), None, None, gam["g"], bet["g"], True, 0.0, 1e-5).squeeze(0).t()
    x1n = F.batch_norm(x1.t().unsqueeze(0), None, None, gam["x"], bet["x"], True, 0.0, 1e-5).squeeze(0).t()
    p = F.relu(g1n + x1n)
    z = p @ w + b
    z.retain_grad()
    p.retain_grad()
    g1n.retain_grad()
    gamma1, beta1 = torch.tensor([1.3], dtype=torch.float64), torch.tensor([-0.2], dtype=torch.float64)
    mu, var = z.mean(), z.var(unbiased=False)
    is1 = 1 / torch.sqrt(var + 1e-5)
    zn = (z - mu) * is1 * gamma1 + beta1
    zn.retain_grad()
    y = xs * torch.sigmoid(zn).unsqueeze(1)
    dy = rn(M, C)
    (y * dy).sum().backward()

    def stats(t):
        m = t.mean(0)
        return m, 1 / torch.sqrt((t * t).mean(0) - m * m + 1e-5)
    cons = {}
    for k, t in (("g", g1.detach()), ("x", x1.detach())):
        m, i = stats(t)
        cons["m" + k], cons["i" + k], cons["s" + k], cons["sh" + k] = m, i, gam[k] * i, bet[k] - m * gam[k] * i
        cons["g" + k] = gam[k]
    cons["w"], cons["b"] = w.detach(), b.detach()
    rows = {"g1": g1.detach(), "x1": x1.detach(), "dz": z.grad}
    _close(ge.psi_in(rows, cons, True), p.detach())
    _close(ge._psi_fn(True)(rows, cons)[0]["z"], z.detach())
    # the two-branch BatchNorm backward: reduce, then apply with the reduced sums
    cons["sums_g"] = cons["sums_x"] = torch.zeros(2, C, dtype=torch.float64)
    _, terms = ge._gate_bn_fn(True, M)(rows, cons)
    s = {k: t.sum(0) for k, t in terms.items()}
    _close(s["q0"], g1n.grad.sum(0))
    _close(s["q3"], w.grad)
    _close(s["q4"][0], b.grad[0])
    cons["sums_g"], cons["sums_x"] = torch.stack([s["q0"], s["q1"]]), torch.stack([s["q0"], s["q2"]])
    outs, _ = ge._gate_bn_fn(True, M)(rows, cons)
    _close(outs["dg"], g1.grad)
    _close(outs["dx"], x1.grad)
    # rowdot_bwd on the stored psi_in
    o, t = ge._rowdot_bwd_fn(0, 0)({"dz": z.grad, "x": p.detach()}, {"w": w.detach()})
    _close(o["dx"], p.grad)
    _close(ge._rowdot_bwd_fn(1, 0)({"dz": z.grad, "x": p.detach()}, {"w": w.detach()})[0]["dx"], g1n.grad)
    _close(t["q0"].sum(0), w.grad)
    # bn1 backward and the gate multiply (sigmoid in place of its classes)
    psi = torch.sigmoid(zn.detach())
    dzn = (dy * xs.detach()).sum(1) * psi * (1 - psi)
    _close(dzn, zn.grad)
    zh = (z.detach() - mu.detach()) * is1.detach()
    c1 = {"gamma": gamma1, "mean": mu.detach().reshape(1), "invstd": is1.detach().reshape(1), "sums": torch.stack([dzn.sum(), (dzn * zh).sum()])}
    _close(ge._bn1_fn(M)({"dzn": dzn, "z": z.detach()}, c1)[0]["dz"], z.grad)
    _close(dy * psi.unsqueeze(1), xs.grad)


def test_geometry_restates_the_kernels():
    assert ge.window_geometry(BF, 512, 16405) == (64, 64, 16, 257, 4112, 257)
    assert ge.window_geometry(F32, 48, 4133) == (12, 16, 64, 65, 4160, 65)
    assert ge.window_geometry(BF, 8, 70001) == (1, 1, 1024, 1024, 1 << 20, 1024)
    assert ge.window_geometry(BF, 96, 449, 3) == (12, 16, 64, 3, 192, 8)
    assert "window.second_sweep" in ge.window_branches(BF, 512, 17) and "window.second_sweep" not in ge.window_branches(BF, 96, 4133)
    assert "window.second_sweep" in ge.window_branches(BF, 96, 65605) and "window.idle_lanes" in ge.window_branches(BF, 40, 63)
    assert "window.extra_chunks" in ge.window_branches(FP, 520, 1) and "window.rows_past_grid" in ge.window_branches(BF, 96, 449, 3)
    assert ge.mul_bwd_branches(BF, 64, 65537, 0) == ["mul_bwd.one_chunk", "mul_bwd.empty_workgroup", "mul_bwd.boundary_off_64"]
    assert ge.mul_bwd_branches(BF, 64, 65, 1) == ["mul_bwd.one_chunk", "mul_bwd.accumulate", "mul_bwd.boundary_off_64"]
    assert ge.mul_bwd_branches(F32, 260, 1, 0) == ["mul_bwd.strided"]
    assert ge.walk_top(BF, 96, "rowdot_fwd") == 449 and ge.walk_top(BF, 512, "gate_psi_fwd") == 113


@pytest.mark.skipif(not os.path.exists(L.SO_PATH), reason="libmi355conv.so not built (run __graft_entry__.build())")
def test_host_queries_the_gpu_file_relies_on():
    lib = L.lib
    for dtype in DTYPES:
        code, epc = L.DTYPE_CODE[dtype], se.EPC[dtype]
        assert lib.mi355_gate_psi_fwd_ok(64 * epc, code) == 1
        assert lib.mi355_gate_psi_fwd_ok(65 * epc, code) == 0
        assert lib.mi355_gate_psi_fwd_ok(64 * epc - 1, code) == 0 and lib.mi355_gate_psi_fwd_ok(epc // 2, code) == 0
        assert lib.mi355_gate_psi_fwd_ok(ge.chans(dtype, ge.PSI_REJECTED), code) == 0
        for c2, _ in ge.WINDOW_CASES:
            assert lib.mi355_gate_psi_fwd_ok(ge.chans(dtype, c2), code) == 1
    for M in (1, 63, 64, 65, 449, 4133, 32704, 32705, 65701, 2 ** 20, 10 ** 9):
        assert 1 <= lib.mi355_gate_bn_bwd_reduce_rows(M) <= lib.mi355_rowreduce_blocks(M) <= 1024
    assert lib.mi355_gate_bn_bwd_reduce_rows(10 ** 9) == 512
