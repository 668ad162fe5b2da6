"""Exact operands and fp64 references for the attention-gate kernels (csrc/gate.hip).  CPU only.

The method is that of tests/stream_exact.py: small integers in the tensors, powers of two and small integers in the constants,
so that every intermediate of a kernel's formula is exact in fp32 and every stored value in the storage type.  The result then
does not depend on the summation order or on fma contraction and must equal the fp64 reference BIT FOR BIT in fp32, bf16 and fp16.
The references are written from the contracts of include/mi355conv.h and the formulas of gate.hip, never from kernel geometry;
the geometry helpers at the end choose row counts and name branches only.

The sigmoid of gate_mul_fwd / gate_mul_bwd is the one inexact step of the file, so the operands avoid it: z, scale and shift are
chosen with z * scale + shift in {-128, 0, +128}, where psi = 1 / (1 + exp(-a)) is 0, 1/2 or 1 in fp32 (exp(128) = 2^184.7 and
exp(-128) are past both ends of fp32); the generator asserts that the fp64 sigmoid rounds to that class value.

Every case carries its SENSITIVITY WITNESS: each checked output of the reference changes when row M - 1 is dropped, when row 0
is duplicated onto row 1, and when the last 16-byte chunk of channels is zeroed — operands that would hide such an error (a last
row of zeros, a weight that is zero on the last chunk) are not handed out: the factory moves on to the next seed."""
import functools
import math

import torch

import stream_exact as se
from stream_exact import F32, BF, FP, EPC, ints, pow2, assert_storable, assert_f32_sum_exact

DTYPES = (F32, BF, FP)
F64 = torch.float64


def assert_f64_sum_exact(terms, quantum, what=""):
    """fp64 accumulation of `terms` along dim 0 is exact in any order: multiples of `quantum` with sum |t| / quantum < 2^53"""
    assert quantum > 0 and math.frexp(quantum)[0] == 0.5, quantum
    u = terms / quantum
    assert torch.equal(u, u.round()), f"{what}: terms are not multiples of {quantum}"
    top = float(u.abs().sum(0).max()) if terms.numel() else 0.0
    assert top < 2.0 ** 53, f"{what}: sum |t| / quantum = {top:.3g} reaches 2^53"


def _storable_everywhere(t, what):
    for dt in DTYPES:
        assert_storable(t, dt, what)


class Case:
    """operands of one launch (fp64): rows {name: [M] or [M, C]}, cons {name: [C] or [1]}, and the reference
    fn(rows, cons) -> (outs {name: per-row result}, terms {name: per-row summand of a reduced quantity}).
    `check(outs, terms, cons)` holds the exactness assertions of the op; `acc` names the accumulator of the sums ("f32" / "f64")."""

    def __init__(self, op, M, C, epc, rows, cons, fn, check, acc=None):
        self.op, self.M, self.C, self.epc, self.rows, self.cons, self.fn, self.check, self.acc = op, M, C, epc, rows, cons, fn, check, acc
        self.outs, self.terms = fn(rows, cons)
        check(self.outs, self.terms, cons)
        self.term_names = tuple(self.terms)
        self._sums = {k: t.sum(0) for k, t in self.terms.items()}
        if M * C > 1 << 21:
            self.terms = None                                   # (the summands of a large case are not kept: five tensors of the operands' size)

    def sums(self):
        return dict(self._sums)

    def prefix_sums(self):
        """sums of the first m rows for every m: [M, ...]"""
        return {k: t.cumsum(0) for k, t in self.terms.items()}

    def ref(self, rows=None, cons=None):
        return self.fn(self.rows if rows is None else rows, self.cons if cons is None else cons)

    # ---- the sensitivity witness ----
    def perturbed(self, kind):
        """the reference of the perturbed operands, row outputs padded with zeros to M rows (a row never computed): (outs, sums)"""
        M, C, epc = self.M, self.C, self.epc
        rows = {k: v.clone() for k, v in self.rows.items()}
        cons = {k: v.clone() for k, v in self.cons.items()}
        if kind == "drop_last_row":
            rows = {k: v[:M - 1] for k, v in rows.items()}
        elif kind == "dup_row0":
            for v in rows.values():
                v[1] = v[0]
        elif kind == "zero_last_chunk":
            for d in (rows, cons):
                for k, v in d.items():
                    if v.shape[-1] == C and (v.dim() == 2 or d is cons):
                        v[..., C - epc:] = 0
        else:
            raise ValueError(kind)
        outs, terms = self.fn(rows, cons)
        pad = {}
        for k, v in outs.items():
            full = torch.zeros_like(self.outs[k])
            full[:v.shape[0]] = v
            pad[k] = full
        return pad, {k: t.sum(0) for k, t in terms.items()}

    def witness_kinds(self):
        kinds = ["drop_last_row"]
        if self.M >= 2:
            kinds.append("dup_row0")
        if any(v.dim() == 2 for v in self.rows.values()):
            kinds.append("zero_last_chunk")
        return kinds

    def blind_spots(self):
        """[(perturbation, output)] the reference does NOT react to: empty for a case the factory hands out"""
        if self.acc == "f32" and self.M * self.C > 1 << 21:
            return self._blind_spots_sampled()
        blind = []
        base_s = self.sums()
        for kind in self.witness_kinds():
            outs, sums = self.perturbed(kind)
            for k, v in outs.items():
                if torch.equal(v, self.outs[k]):
                    blind.append((kind, k))
            for k, v in sums.items():
                if k in self.quiet or (kind == "zero_last_chunk" and k in self.chanfree):
                    continue
                if torch.equal(v, base_s[k]):
                    blind.append((kind, k))
        return blind

    def _blind_spots_sampled(self, n=256):
        """large reductions: every reference here treats each row on its own (asserted on the sample), so the first and last n
        rows decide the two row witnesses — the sums move by the same term as those of the whole —, and a sum over the whole
        reacts to the zeroed chunk iff it is non-zero there while the sample's perturbed terms are zero there"""
        M, C, epc = self.M, self.C, self.epc
        idx = torch.cat([torch.arange(n), torch.arange(M - n, M)])
        sub = Case(self.op, 2 * n, C, epc, {k: v[idx] for k, v in self.rows.items()}, self.cons, self.fn, lambda *a: None, self.acc)
        sub.quiet, sub.chanfree = self.quiet, self.chanfree
        for k, v in sub.outs.items():
            assert torch.equal(v, self.outs[k][idx]), "the reference does not treat rows independently"
        blind = [b for b in sub.blind_spots() if not (b[0] == "zero_last_chunk" and b[1] in self.term_names)]
        full, (_, zeroed) = self.sums(), sub.perturbed("zero_last_chunk")
        for k, v in full.items():
            if k in self.quiet or k in self.chanfree:
                continue
            if bool(zeroed[k][..., C - epc:].any()) or not bool(v[..., C - epc:].any()):
                blind.append(("zero_last_chunk", k))
        return blind

    quiet = ()              # sums that stay zero by contract
    chanfree = ()           # sums that do not depend on the channel (sum dz): a dropped chunk shows as NaN left in the partial row


def loud(dz, lim):
    """rows 0, 1 and M - 1 of a per-row operand carry different non-zero values: no row witness fails on a zero of the draw"""
    dz[0] = lim
    if dz.numel() > 1:
        dz[1] = -1
    if dz.numel() > 2:
        dz[-1] = 1
    return dz


def _searched(build, key, tries=64):
    """the first seed whose case has no blind spot (the generator's own assertions hold for every seed)"""
    last = None
    for t in range(tries):
        c = build(torch.Generator().manual_seed((hash_key(key) + 7919 * t) % (2 ** 31)))
        last = c.blind_spots()
        if not last:
            return c
    raise AssertionError(f"{key}: no operands with a full sensitivity witness in {tries} seeds: {last}")


def hash_key(key):
    h = 17
    for i, k in enumerate(key):
        h = (h * 1000003 + (int(k) if not isinstance(k, str) else sum(map(ord, k))) * (i + 3)) % (2 ** 31)
    return h


# ---- rowdot_fwd: z[m] = b + sum_c w[c] x[m][c]; partial (sum z, sum z^2) ---------------------------------------------------------
def _rowdot_fwd_fn(rows, cons):
    z = cons["b"] + rows["x"] @ cons["w"]
    return {"z": z}, {"s0": z, "s1": z * z}


def _rowdot_fwd_check(outs, terms, cons):
    assert_storable(outs["z"], F32, "z")
    assert_f64_sum_exact(terms["s1"], 1.0, "sum z^2")


@functools.lru_cache(maxsize=128)
def rowdot_fwd_case(C, epc, M, salt=0):
    def build(g):
        x = ints(g, (M, C), 4)
        w, b = ints(g, (C,), 3, 0.2), ints(g, (1,), 3, 0.0) + 5
        assert_f32_sum_exact((x * w).t(), 1.0, "w . x")
        return Case("rowdot_fwd", M, C, epc, {"x": x}, {"w": w, "b": b}, _rowdot_fwd_fn, _rowdot_fwd_check, "f64")
    return _searched(build, ("rowdot_fwd", C, epc, M, salt))


def plane_index(M, hw, K):
    """where pixel m = n * hw + p of channel plane 0 lands in an [N][K][hw] map: n * K * hw + p (include/mi355conv.h)"""
    m = torch.arange(M)
    return (m // hw) * (K * hw) + m % hw


# ---- rowdot_bwd: dx = dz w (masked by x > 0) (+ old); partial q0[c] = sum dz x, q1 = sum dz ---------------------------------------
def _rowdot_bwd_fn(mask, acc):
    def fn(rows, cons):
        dz, x = rows["dz"].unsqueeze(1), rows["x"]
        d = dz * cons["w"]
        if mask:
            d = torch.where(x > 0, d, torch.zeros_like(d))
        dx = d + rows["old"] if acc else d
        return {"dx": dx}, {"q0": dz * x, "q1": dz.expand_as(x).clone()}
    return fn


def _rowdot_bwd_check(outs, terms, cons):
    _storable_everywhere(outs["dx"], "dx")
    assert_f32_sum_exact(terms["q0"], 1.0, "sum dz x")
    assert_f32_sum_exact(terms["q1"], 1.0, "sum dz")


@functools.lru_cache(maxsize=128)
def rowdot_bwd_case(C, epc, M, mask, acc, salt=0):
    def build(g):
        rows = {"dz": loud(ints(g, (M,), 4), 4), "x": ints(g, (M, C), 4)}
        if acc:
            rows["old"] = ints(g, (M, C), 4)
        c = Case("rowdot_bwd", M, C, epc, rows, {"w": ints(g, (C,), 3, 0.2)}, _rowdot_bwd_fn(mask, acc), _rowdot_bwd_check, "f32")
        c.chanfree = ("q1",)
        return c
    return _searched(build, ("rowdot_bwd", C, epc, M, mask, acc, salt))


# ---- gate_psi_fwd: p = store(relu(fma(x1, sx, fma(g1, sg, shg + shx)))), z = b + sum w p ------------------------------------------
def psi_in(rows, cons, two):
    v = rows["g1"] * cons["sg"] + (cons["shg"] + cons["shx"] if two else cons["shg"])
    if two:
        v = rows["x1"] * cons["sx"] + v
    return v.clamp(min=0)


def _psi_fn(two):
    def fn(rows, cons):
        p = psi_in(rows, cons, two)
        z = cons["b"] + p @ cons["w"]
        return {"z": z}, {"s0": z, "s1": z * z}
    return fn


def _psi_check(outs, terms, cons):
    assert_storable(outs["z"], F32, "z")
    assert_f64_sum_exact(terms["s0"], 0.25, "sum z")
    assert_f64_sum_exact(terms["s1"], 0.0625, "sum z^2")


def _branch_consts(g, C, small=False):
    k = se.Consts(g, C, small)
    return {"sg": k.scale, "shg": k.shift, "sx": k.scale2, "shx": k.shift2, "mg": k.mean, "ig": k.invstd,
            "mx": ints(g, (C,), k.xlim, 0.2), "ix": pow2(g, C, -2, 0 if small else 2)}, k


@functools.lru_cache(maxsize=128)
def gate_psi_case(C, epc, M, two, salt=0):
    def build(g):
        cons, _ = _branch_consts(g, C)
        cons = {k: cons[k] for k in ("sg", "shg", "sx", "shx")}
        cons["w"], cons["b"] = ints(g, (C,), 3, 0.2), ints(g, (1,), 3, 0.0) + 5
        rows = {"g1": ints(g, (M, C), 4)}
        if two:
            rows["x1"] = ints(g, (M, C), 4)
        p = psi_in(rows, cons, two)
        _storable_everywhere(p, "psi_in")
        assert_f32_sum_exact((p * cons["w"]).t(), 0.25, "w . psi_in")
        return Case("gate_psi_fwd", M, C, epc, rows, cons, _psi_fn(two), _psi_check, "f64")
    return _searched(build, ("gate_psi_fwd", C, epc, M, two, salt))


# ---- gate_bn_bwd_reduce / _apply ----------------------------------------------------------------------------------------------------
def _gate_bn_fn(two, M):
    def fn(rows, cons):
        dz = rows["dz"].unsqueeze(1)
        p = psi_in(rows, cons, two)
        dp = torch.where(p > 0, dz * cons["w"], torch.zeros_like(p))                  # store(dz w) where p > 0
        hg = (rows["g1"] - cons["mg"]) * cons["ig"]
        terms = {"q0": dp, "q1": dp * hg, "q2": torch.zeros_like(dp), "q3": dz * p, "q4": dz.expand_as(p).clone()}
        outs = {"dg": cons["gg"] * cons["ig"] * (dp - cons["sums_g"][0] / M - hg * (cons["sums_g"][1] / M))}
        if two:
            hx = (rows["x1"] - cons["mx"]) * cons["ix"]
            terms["q2"] = dp * hx
            outs["dx"] = cons["gx"] * cons["ix"] * (dp - cons["sums_x"][0] / M - hx * (cons["sums_x"][1] / M))
        return outs, terms
    return fn


def _gate_bn_check(outs, terms, cons):
    for k, v in outs.items():
        _storable_everywhere(v, k)
    _storable_everywhere(terms["q0"], "dp")
    assert_f32_sum_exact(terms["q0"], 1.0, "q0")
    assert_f32_sum_exact(terms["q1"], float(cons["ig"].min()), "q1")
    assert_f32_sum_exact(terms["q2"], float(cons["ix"].min()), "q2")
    assert_f32_sum_exact(terms["q3"], 0.25, "q3")
    assert_f32_sum_exact(terms["q4"], 1.0, "q4")


@functools.lru_cache(maxsize=128)
def gate_bn_case(C, epc, M, two, small=False, pow2_sums=False, salt=0):
    """pow2_sums: M a power of two and sums = k * M (k in {-1, 0, 1}), so that sums * (float)(1 / M) is exact; else zero sums"""
    def build(g):
        sm = small or pow2_sums
        cons, k = _branch_consts(g, C, sm)
        lim = 2 if sm else 4
        cons["w"] = ints(g, (C,), 2 if sm else 3, 0.2)
        cons["gg"], cons["gx"] = k.gamma, pow2(g, C, -1 if sm else -2, 1 if sm else 2, signed=True)
        if pow2_sums:
            assert M & (M - 1) == 0
            cons["sums_g"], cons["sums_x"] = ints(g, (2, C), 1, 0.3) * M, ints(g, (2, C), 1, 0.3) * M
        else:
            cons["sums_g"], cons["sums_x"] = torch.zeros(2, C, dtype=F64), torch.zeros(2, C, dtype=F64)
        rows = {"dz": loud(ints(g, (M,), lim), lim), "g1": ints(g, (M, C), lim)}
        if two:
            rows["x1"] = ints(g, (M, C), lim)
        _storable_everywhere(psi_in(rows, cons, two), "psi_in")
        c = Case("gate_bn_bwd", M, C, epc, rows, cons, _gate_bn_fn(two, M), _gate_bn_check, "f32")
        c.chanfree = ("q4",)
        c.quiet = () if two else ("q2",)                                           # one operand: quantity 2 stays zero
        return c
    return _searched(build, ("gate_bn_bwd", C, epc, M, two, small, pow2_sums, salt))


# ---- gate_mul_fwd / gate_mul_bwd: the sigmoid on its three exact classes -------------------------------------------------------------
PSI_ARGS = (-128.0, 0.0, 128.0)
PSI_CLASS = (0.0, 0.5, 1.0)
GATE_AFFINE = ((32.0, -64.0), (-64.0, 128.0), (128.0, 0.0), (16.0, 48.0))           # (scale, shift): z = (a - shift) / scale is an integer


def sigmoid_classes_hold():
    for a, c in zip(PSI_ARGS, PSI_CLASS):
        s = 1.0 / (1.0 + math.exp(-a)) if a > -700 else 0.0
        assert float(torch.tensor(s, dtype=F64).float()) == c, (a, s)
    return True


def class_rows(g, M):
    """a class index per row, no two neighbouring rows alike, all three present from M = 3 on"""
    step = torch.randint(1, 3, (M,), generator=g)
    step[0] = int(torch.randint(0, 3, (1,), generator=g))
    return torch.cumsum(step, 0) % 3


def _psi_of(z, cons):
    """psi per row from the CLASS of its argument; the generator asserted that the argument is one of the three"""
    a = z * cons["scale"] + cons["shift"]
    psi = torch.full_like(a, float("nan"))
    for arg, c in zip(PSI_ARGS, PSI_CLASS):
        psi = torch.where(a == arg, torch.full_like(a, c), psi)
    assert not torch.isnan(psi).any(), "an argument of the sigmoid outside {-128, 0, 128}"
    return psi


def _gate_z(g, M, which):
    sigmoid_classes_hold()
    scale, shift = GATE_AFFINE[which % len(GATE_AFFINE)]
    cls = class_rows(g, M)
    z = (torch.tensor(PSI_ARGS, dtype=F64)[cls] - shift) / scale
    assert torch.equal(z, z.round()) and float(z.abs().max()) <= 16
    return z, torch.tensor([scale], dtype=F64), torch.tensor([shift], dtype=F64)


def _mul_fwd_fn(rows, cons):
    return {"y": rows["x"] * _psi_of(rows["z"], cons).unsqueeze(1)}, {}


@functools.lru_cache(maxsize=128)
def gate_mul_fwd_case(C, epc, M, salt=0):
    def build(g):
        z, scale, shift = _gate_z(g, M, C + M + salt)
        x = ints(g, (M, C), 4, 0.1)
        return Case("gate_mul_fwd", M, C, epc, {"x": x, "z": z}, {"scale": scale, "shift": shift}, _mul_fwd_fn,
                    lambda o, t, c: _storable_everywhere(o["y"], "y"))
    return _searched(build, ("gate_mul_fwd", C, epc, M, salt))


def _mul_bwd_fn(acc):
    def fn(rows, cons):
        psi = _psi_of(rows["z"], cons)
        d = rows["dy"] * psi.unsqueeze(1)
        dzn = (rows["dy"] * rows["x"]).sum(1) * psi * (1 - psi)
        zh = (rows["z"] - cons["mean"]) * cons["invstd"]
        return {"dx": d + rows["old"] if acc else d, "dzn": dzn}, {"s0": dzn, "s1": dzn * zh}
    return fn


def _mul_bwd_check(outs, terms, cons):
    _storable_everywhere(outs["dx"], "dx")
    assert_storable(outs["dzn"], F32, "dzn")
    q = 0.25 * float(cons["invstd"])
    assert_f64_sum_exact(terms["s0"], 0.25, "sum dzn")
    assert_f64_sum_exact(terms["s1"], q, "sum dzn zhat")


@functools.lru_cache(maxsize=128)
def gate_mul_bwd_case(C, epc, M, acc, salt=0):
    def build(g):
        z, scale, shift = _gate_z(g, M, C + M + acc + salt)
        rows = {"dy": ints(g, (M, C), 4, 0.1), "x": ints(g, (M, C), 4, 0.1), "z": z}
        if acc:
            rows["old"] = ints(g, (M, C), 4)
        assert_f32_sum_exact((rows["dy"] * rows["x"]).t(), 1.0, "dy . x")
        cons = {"scale": scale, "shift": shift, "mean": ints(g, (1,), 3, 0.0), "invstd": pow2(g, 1, -2, 2)}
        c = Case("gate_mul_bwd", M, C, epc, rows, cons, _mul_bwd_fn(acc), _mul_bwd_check, "f64")
        return c
    return _searched(build, ("gate_mul_bwd", C, epc, M, acc, salt))


# ---- bn1_bwd_apply: dz = gamma is (dzn - s0 / M - (z - mu) is s1 / M) -----------------------------------------------------------------
def _bn1_fn(M):
    def fn(rows, cons):
        zh = (rows["z"] - cons["mean"]) * cons["invstd"]
        return {"dz": cons["gamma"] * cons["invstd"] * (rows["dzn"] - cons["sums"][0] / M - zh * (cons["sums"][1] / M))}, {}
    return fn


@functools.lru_cache(maxsize=128)
def bn1_case(M, pow2_sums, salt=0):
    def build(g):
        rows = {"dzn": ints(g, (M,), 16) / 4, "z": ints(g, (M,), 8)}
        cons = {"gamma": pow2(g, 1, -2, 2, signed=True), "mean": ints(g, (1,), 3, 0.0), "invstd": pow2(g, 1, -2, 2)}
        if pow2_sums:
            assert M & (M - 1) == 0
            cons["sums"] = (ints(g, (2,), 1, 0.0) + 2) * M
        else:
            cons["sums"] = torch.zeros(2, dtype=F64)
        return Case("bn1_bwd_apply", M, 1, 1, rows, cons, _bn1_fn(M), lambda o, t, c: assert_storable(o["dz"], F32, "dz"))
    return _searched(build, ("bn1_bwd_apply", M, pow2_sums, salt))


# ---- order independence (tests/test_gate_exact_cpu.py) -------------------------------------------------------------------------------
def f32_sums_in_order(terms, order):
    """sequential numpy float32 accumulation of the rows of `terms` (fp64) in the given order"""
    import numpy as np
    t = np.asarray(terms.numpy(), dtype=np.float32)[order]
    return torch.from_numpy(np.cumsum(t, axis=0, dtype=np.float32)[-1].astype(np.float64))


# ---- geometry: for choosing M and naming branches only — no expected value comes from here ------------------------------------------
def window_geometry(dtype, C, M, cap=1024):
    """(cp, tpr, rows per workgroup step, workgroups, rows per sweep, partial rows) of rowdot_fwd_kernel / gate_psi_fwd_kernel"""
    cp = C // EPC[dtype]
    tpr = 1
    while tpr < cp and tpr < 64:
        tpr *= 2
    chunk = 16 * (64 // tpr)
    nb = max(1, min((M + 63) // 64, 1024))
    grid = min(nb, cap)
    return cp, tpr, chunk, grid, grid * chunk, nb


def window_branches(dtype, C, M, cap=1024):
    cp, tpr, chunk, grid, sweep, nb = window_geometry(dtype, C, M, cap)
    br = ["window.one_sweep"]
    if M > sweep:
        br.append("window.second_sweep")
    if M % chunk:
        br.append("window.clamped_tail")
    if cp < tpr:
        br.append("window.idle_lanes")
    if cp > tpr:
        br.append("window.extra_chunks")
    if nb > grid:
        br.append("window.rows_past_grid")
    return br


def mul_bwd_branches(dtype, C, M, acc):
    cp = C // EPC[dtype]
    nb = max(1, min((M + 63) // 64, 1024))
    rpb = -(-M // nb)
    br = ["mul_bwd.one_chunk" if cp <= 64 else "mul_bwd.strided"]
    if acc:
        br.append("mul_bwd.accumulate")
    if (nb - 1) * rpb >= M:
        br.append("mul_bwd.empty_workgroup")
    if nb > 1 and rpb % 64:
        br.append("mul_bwd.boundary_off_64")
    return br


# (C of the 2-byte types, [M]) of the moving-window cases; fp32 runs C / 2: the same chunk count
WINDOW_CASES = [(512, [1, 15, 16, 17, 197, 1024 * 16 + 16 + 5]), (96, [63, 64, 65, 4133, 65536 + 64 + 5]), (40, [63, 64, 65, 4133]),
                (8, [1, 1023, 1025, 70001])]
ROWDOT_WIDE = [(520, [1, 65, 197]), (1600, [65, 197]), (2048, [17, 197])]      # more than one chunk per lane: rowdot_fwd only
ROWDOT_REJECTED, PSI_REJECTED = 2056, 520
PLANES = dict(K=3, hw=37, N=5, C=96)
MUL_BWD_CASES = [(64, [1, 65, 1025, 65537]), (96, [1, 65, 1025]), (512, [1, 65, 1025]), (520, [1, 65, 1025]), (1024, [1, 65, 1025])]
BN1_ROWS = [1, 255, 257, 2 ** 20, 2 ** 20 + 300]
CH2 = [8, 40, 96, 64, 1024, 2048, 2560]                                       # the channel list of tests/test_gpu_stream_exact.py


def chans(dtype, c2):
    return c2 // 2 if dtype == F32 else c2


def edge_rows(rp, B, extra=()):
    ms = {1, rp - 1, rp * B - 1, rp * B, rp * B + 1} | set(extra)
    return sorted(m for m in ms if m >= 1)


def rowred_rows(dtype, C):
    """the row counts of the fetch-batched reductions (FETCH_ROWS = 4), as the BatchNorm file chooses them"""
    geo = se.geometry(dtype, C, 4)
    return edge_rows(geo[3], 4, (3 * geo[4] + geo[3] + 1,))


def rowmap_rows(dtype, C):
    """the row counts of the plain elementwise loop"""
    rp = se.geometry(dtype, C)[3]
    return edge_rows(rp, 1, (3 * rp + 2,))


BIG_ROWS = [(4, 16405), (3, 2 * 32768 + 128 + 37)]                              # (index into CH2, M): several trips of the capped grids


def walk_top(dtype, C, launcher):
    """the last M of the three-workgroup walks: two sweeps of the window plus one workgroup step plus one (window kernels and
    the plain elementwise loop), two sweeps and two batches of the fetch ring (the reductions)"""
    if launcher in ("rowdot_bwd", "gate_bn_bwd_reduce", "gate_bn_bwd_apply"):
        _, _, _, _, batch, sweep = se.geometry(dtype, C, 4, 3)
        return 2 * sweep + 2 * batch
    chunk = window_geometry(dtype, C, 1)[2]
    return 2 * 3 * chunk + chunk + 1


WALK_C2 = (96, 512)
WALK_LAUNCHERS = ("rowdot_fwd", "gate_psi_fwd", "rowdot_bwd", "gate_bn_bwd_reduce", "gate_bn_bwd_apply", "gate_mul_fwd")
ROWDOT_BWD_FORMS = ((0, 0), (1, 0), (0, 1), (1, 1))                              # (mask, accumulate)


def pow2_rows(dtype, C):
    """a power-of-two M of several fetch batches (rp * 4 rows each)"""
    return 2048 if se.geometry(dtype, C, 4)[3] > 2 else 512


def walk_case(dtype, C, launcher):
    epc, M = EPC[dtype], walk_top(dtype, C, launcher)
    if launcher == "rowdot_fwd":
        return rowdot_fwd_case(C, epc, M, 1)
    if launcher == "gate_psi_fwd":
        return gate_psi_case(C, epc, M, True, 1)
    if launcher == "rowdot_bwd":
        return rowdot_bwd_case(C, epc, M, 1, 0, 1)
    if launcher == "gate_mul_fwd":
        return gate_mul_fwd_case(C, epc, M, 1)
    return gate_bn_case(C, epc, M, True, False, False, 1)


def clear_cases():
    """drop the cached cases (the large ones hold hundreds of megabytes)"""
    for f in (rowdot_fwd_case, rowdot_bwd_case, gate_psi_case, gate_bn_case, gate_mul_fwd_case, gate_mul_bwd_case, bn1_case):
        f.cache_clear()


def case_specs(dtype):
    """every case tests/test_gpu_gate_exact.py builds for `dtype`: [(factory, args)] (tests/test_gate_exact_cpu.py builds them all)"""
    epc, out = EPC[dtype], []
    for c2, ms in WINDOW_CASES:
        for M in ms:
            C = chans(dtype, c2)
            out += [(rowdot_fwd_case, (C, epc, M)), (gate_psi_case, (C, epc, M, True)), (gate_psi_case, (C, epc, M, False))]
    for c2, ms in ROWDOT_WIDE:
        out += [(rowdot_fwd_case, (chans(dtype, c2), epc, M)) for M in ms]
    P, C = PLANES, chans(dtype, PLANES["C"])
    for k in range(P["K"]):
        out += [(rowdot_fwd_case, (C, epc, P["N"] * P["hw"], 10 + k)), (rowdot_bwd_case, (C, epc, P["N"] * P["hw"], k % 2, int(k > 0), 10 + k))]
    for c2 in CH2:
        C = chans(dtype, c2)
        for M in rowred_rows(dtype, C):
            out += [(rowdot_bwd_case, (C, epc, M, m, a)) for m, a in ROWDOT_BWD_FORMS]
            out += [(gate_bn_case, (C, epc, M, two)) for two in (True, False)]
        out += [(gate_bn_case, (C, epc, pow2_rows(dtype, C), two, True, True)) for two in (True, False)]
        out += [(gate_mul_fwd_case, (C, epc, M)) for M in rowmap_rows(dtype, C)]
    for i, M in BIG_ROWS:
        C = chans(dtype, CH2[i])
        out += [(rowdot_bwd_case, (C, epc, M, 1, 1)), (gate_bn_case, (C, epc, M, True, True)), (gate_bn_case, (C, epc, M, False, True))]
    for c2, ms in MUL_BWD_CASES:
        out += [(gate_mul_bwd_case, (chans(dtype, c2), epc, M, a)) for M in ms for a in (0, 1)]
    out += [(bn1_case, (M, False)) for M in BN1_ROWS] + [(bn1_case, (2 ** 20, True))]
    for c2 in WALK_C2:
        out += [(walk_case, (dtype, chans(dtype, c2), l)) for l in WALK_LAUNCHERS if l != "gate_bn_bwd_apply"]
    return out
