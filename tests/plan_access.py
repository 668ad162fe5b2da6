"""What every launcher of a launch plan touches: the access table behind tests/plan_verify.py.

One entry per launcher name that mi355/graph.py emits.  For every POINTER slot of the prototype in include/mi355conv.h the
entry says

  mode      read or write, taken from the header's own ``const`` (parsed here: mi355.lib.parse_header drops it); ``rmw`` names
            the scalar slot that turns a write into a read-modify-write (`accumulate`, `acc`, `beta`, `post_acc`), ``state``
            marks persistent state that is read-modify-write by design (PERSISTENT_STATE lists every such slot);
  nullable  whether the slot may be NULL;
  extent    rows x row length x pitch as an expression of the launch's own scalar arguments, as the header documents them.

`accesses()` resolves the un-bound ``Launch.args`` objects (T, V, GRef, Ws, Builder._WsOff, (tensor, byte offset),
torch.Tensor) into regions (storage, first byte, rows, row bytes, pitch bytes) and checks, for a ``T`` / ``V`` handle, that the
scalar slots beside it (ld, M or N H W, C) agree with the handle.  A launcher without a complete entry is an AccessError: there
is no default."""
import re
from types import SimpleNamespace

import torch

from mi355 import graph
from mi355.lib import lib, HEADER


class AccessError(AssertionError):
    """the table, not the plan, cannot describe a launch (missing entry, missing slot, a handle that disagrees with its scalars)"""


# ---- the header's own prototypes, with const ------------------------------------------------------------------------------
def parse_slots(path=HEADER):
    """-> {launcher: [(slot name, kind)]} with kind 'in' (const T*), 'out' (T*) or 'scalar', in prototype order (the trailing
    stream included, as 'scalar')."""
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|const char\*|void\*)\s+(mi355_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        slots = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                name = a.split("*")[-1].strip() if "*" in a else a.rsplit(" ", 1)[1]
                kind = ("in" if a.startswith("const ") else "out") if "*" in a else "scalar"
                slots.append((name, kind))
        out[m.group(2)] = slots
    return out


SLOTS = parse_slots()
ESZ = {0: 4, 1: 2, 2: 2}          # MI355_F32, MI355_BF16, MI355_F16


# ---- extents ------------------------------------------------------------------------------------------------------------------
def rows(M, C, ld, esz):
    """M rows of C elements of esz bytes, row pitch ld elements"""
    return (int(M), int(C), int(ld), int(esz))


def flat(n, esz=4):
    return (1, int(n), int(n), int(esz))


def nb(M):
    return lib.mi355_rowreduce_blocks(int(M))


class S:
    """one pointer slot: extent(a) over the namespace of the launch's arguments; rmw(a) -> the write also reads"""
    __slots__ = ("extent", "null", "rmw", "state")

    def __init__(self, extent, null=False, rmw=None, state=False):
        self.extent, self.null, self.rmw, self.state = extent, null, rmw, state


def _act(M, C, ld, null=False, rmw=None):       # an activation operand: M rows of C elements of the launch's dtype at pitch ld
    return S(lambda a, M=M, C=C, ld=ld: rows(getattr(a, M) if isinstance(M, str) else M(a), getattr(a, C), getattr(a, ld), a.e), null=null, rmw=rmw)


def _f(n, null=False, rmw=None, state=False, esz=4):      # n fp32 (or esz-byte) elements, n a slot name or a function
    return S(lambda a, n=n: flat(getattr(a, n) if isinstance(n, str) else n(a), esz), null=null, rmw=rmw, state=state)


_NHW = lambda a: a.N * a.H * a.W
_bit0 = lambda name: (lambda a: bool(int(getattr(a, name)) & 1))
_nz = lambda name: (lambda a: getattr(a, name) != 0)


def _igemm_out_rows(a):      # bit 2: the 2x2 sums go to a half-resolution out [N][Ho/2][Wo/2] (mi355conv.h, mi355_conv2d_igemm)
    return a.N * (a.Ho // 2) * (a.Wo // 2) if a.accumulate & 4 else a.N * a.Ho * a.Wo


def _igemm_stats(a):         # stats[(b*2+q)*Co + c], b < mi355_conv2d_igemm_stat_rows(...)
    r = lib.mi355_conv2d_igemm_stat_rows(a.N, a.Hi, a.Wi, a.Ci, a.Ho, a.Wo, a.Co, a.KH, a.KW, a.mul, a.kmul, a.off, a.div, a.up, a.dtype)
    return max(r, 0) * 2 * a.Co


def _zplane(a):              # one channel plane of an NCHW fp32 map [N][K][HW] (mi355_rowdot_fwd): pixel n*HW + p at z[n*K*HW + p]
    return flat(a.M) if a.K == 1 else rows(a.M // a.HW, a.HW, a.K * a.HW, 4)


def _pool_out(a):
    return (a.H + 2 * a.pad - a.k) // a.stride + 1, (a.W + 2 * a.pad - a.k) // a.stride + 1


_bn_coef = {k: _f("C") for k in ("mean", "invstd", "mscale", "mshift")}
_gate_coef = {k + s: _f("C", null=(s == "_x")) for k in ("scale", "shift", "mean", "invstd") for s in ("_g", "_x")}
_bn_bwd_ops = dict(dy=_act("M", "C", "lddy"), y=_act("M", "C", "ldy", null=True), x=_act("M", "C", "ldx"), gamma=_f("C"), **_bn_coef,
                   sums=_f(lambda a: 2 * a.C), dx=_act("M", "C", "lddx"))
_pool2_ops = dict(dy=_act(_NHW, "C", "lddy", null=True), dp=_act(lambda a: a.N * (a.H // 2) * (a.W // 2), "C", "lddp"),
                  x=_act(_NHW, "C", "ldx"), **_bn_coef)
_wgrad_pair = lambda i: {f"x{i}": S(lambda a: rows(a.N * a.Hi * a.Wi, a.Ci, a.ldx, a.e), null=True),
                         f"dy{i}": S(lambda a: rows(a.N * a.Ho * a.Wo, a.Co, a.ldy, a.e), null=True)}

TABLE = {
    # ---- layout staging
    "mi355_pack_input_nchw": dict(x=_f(lambda a: a.N * a.C * a.H * a.W), y=_act(_NHW, "Cpad", "Cpad")),
    "mi355_pack_input_im2col3": dict(x=_f(lambda a: a.N * a.C * a.H * a.W), y=S(lambda a: rows(_NHW(a), 32, 32, a.e))),
    "mi355_unpack_output_nchw": dict(x=_act(_NHW, "C", "ld"), y=_f(lambda a: a.N * a.C * a.H * a.W)),
    "mi355_pack_nchw": dict(x=_f(lambda a: a.N * a.C * a.H * a.W), y=_act(_NHW, "C", "ld")),
    # the table's rows are further reads and writes: indirect_accesses()
    "mi355_pack_conv_weights_batched": dict(table=_f(lambda a: a.n * a.fields, esz=8)),
    # ---- convolutions
    "mi355_conv2d_igemm": dict(**{"in": S(lambda a: rows(a.N * a.Hi * a.Wi, a.Ci, a.ldi, a.e))},
                               wk=S(lambda a: flat(a.Co * a.KH * a.KW * a.Ci, a.e)), bias=_f("Co", null=True),
                               out=S(lambda a: rows(_igemm_out_rows(a), a.Co, a.ldo, a.e), rmw=_bit0("accumulate")),     # epilogue codes 1 and 5
                               stats=_f(_igemm_stats, null=True)),
    "mi355_conv2d_wgrad": dict(x=S(lambda a: rows(a.N * a.Hi * a.Wi, a.Ci, a.ldx, a.e)), dy=S(lambda a: rows(a.N * a.Ho * a.Wo, a.Co, a.ldy, a.e)),
                               ws=_f(lambda a: a.splits * a.Co * a.KH * a.KW * a.Ci)),
    "mi355_conv2d_wgrad_multi": dict(**{k: v for i in range(6) for k, v in _wgrad_pair(i).items()},
                                     ws=_f(lambda a: a.splits * a.Co * 9 * a.Ci)),
    "mi355_conv2d_wgrad_reduce": dict(ws=_f(lambda a: a.splits * a.Co * a.KH * a.KW * a.Ci),
                                      dw=_f(lambda a: a.Co * a.Ci_real * a.KH * a.KW, rmw=_nz("beta"))),
    # ---- BatchNorm / per-channel reductions
    "mi355_bn_stats": dict(x=_act("M", "C", "ld"), partial=_f(lambda a: nb(a.M) * 2 * a.C)),
    "mi355_bn_finalize": dict(partial=_f(lambda a: a.nblocks * 2 * a.C), gamma=_f("C"), beta=_f("C"),
                              running_mean=_f("C", null=True, state=True), running_var=_f("C", null=True, state=True),
                              nbt=_f(lambda a: 1, null=True, state=True, esz=8),
                              scale=_f("C"), shift=_f("C"), mean=_f("C"), invstd=_f("C")),
    "mi355_fold_rows": dict(partial=_f(lambda a: a.rows * a.rowlen), out=_f(lambda a: a.nsplit * a.rowlen)),
    "mi355_bn_fold_bias": dict(bias=_f("C", null=True), scale=_f("C"), shift=_f("C"), out=_f("C")),
    "mi355_bn_eval_coeffs": dict(gamma=_f("C"), beta=_f("C"), running_mean=_f("C"), running_var=_f("C"), scale=_f("C"), shift=_f("C")),
    "mi355_bn_act": dict(x=_act("M", "C", "ldx"), scale=_f("C"), shift=_f("C"), x2=_act("M", "C", "ldx2", null=True),
                         scale2=_f("C", null=True), shift2=_f("C", null=True), res=_act("M", "C", "ldr", null=True), y=_act("M", "C", "ldy")),
    "mi355_bn_act_pool2": dict(x=_act(_NHW, "C", "ldx"), scale=_f("C"), shift=_f("C"), y=_act(_NHW, "C", "ldy"),
                               p=_act(lambda a: a.N * (a.H // 2) * (a.W // 2), "C", "ldp", null=True)),
    "mi355_bn_act_windows": dict(x=_act(_NHW, "C", "ldx"), scale=_f("C"), shift=_f("C"), res=_act(_NHW, "C", "ldr"), y=_act(_NHW, "C", "ldy")),
    "mi355_bn_bwd_reduce": dict(dy=_act("M", "C", "lddy"), y=_act("M", "C", "ldy", null=True), x=_act("M", "C", "ldx"), **_bn_coef,
                                partial=_f(lambda a: nb(a.M) * 2 * a.C)),       # rows beyond the grid are written as zeros
    "mi355_bn_bwd_finalize": dict(partial=_f(lambda a: a.nblocks * 2 * a.C), sums=_f(lambda a: 2 * a.C),
                                  dgamma=_f("C", null=True, rmw=_nz("acc")), dbeta=_f("C", null=True, rmw=_nz("acc"))),
    "mi355_bn_bwd_finalize_at": dict(partial=_f(lambda a: a.nblocks * a.nq * a.C), sums=_f(lambda a: 2 * a.C),
                                     dgamma=_f("C", null=True, rmw=_nz("acc")), dbeta=_f("C", null=True, rmw=_nz("acc"))),
    "mi355_bn_bwd_apply": dict(**_bn_bwd_ops, dres=_act("M", "C", "lddres", null=True),
                               dpost=_act("M", "C", "lddpost", null=True, rmw=_nz("post_acc")),
                               dbias_partial=_f(lambda a: nb(a.M) * a.C, null=True)),
    "mi355_bn_bwd_apply_post4": dict(**_bn_bwd_ops, dpost=_act("M", "C", "lddpost", rmw=_nz("post_acc")),
                                     ex0=_act("M", "C", "ldex"), ex1=_act("M", "C", "ldex", null=True),
                                     ex2=_act("M", "C", "ldex", null=True), ex3=_act("M", "C", "ldex", null=True)),
    "mi355_bn_bwd_reduce_pool2": dict(**_pool2_ops, partial=_f(lambda a: nb(_NHW(a)) * 2 * a.C)),
    "mi355_bn_bwd_apply_pool2": dict(**_pool2_ops, gamma=_f("C"), sums=_f(lambda a: 2 * a.C), dx=_act(_NHW, "C", "lddx")),
    "mi355_colsum_finalize": dict(partial=S(lambda a: rows(a.nblocks, a.C, a.stride * a.C, 4)), out=_f("C", rmw=_nz("acc"))),
    "mi355_colsum": dict(x=_act("M", "C", "ld"), partial=_f(lambda a: nb(a.M) * a.C)),
    # ---- pooling / elementwise
    "mi355_maxpool_fwd": dict(x=_act(_NHW, "C", "ldx"), y=S(lambda a: rows(a.N * _pool_out(a)[0] * _pool_out(a)[1], a.C, a.ldy, a.e))),
    "mi355_maxpool_bwd": dict(x=_act(_NHW, "C", "ldx"), dy=S(lambda a: rows(a.N * _pool_out(a)[0] * _pool_out(a)[1], a.C, a.lddy, a.e)),
                              dx=_act(_NHW, "C", "lddx", rmw=_nz("accumulate"))),
    "mi355_upsample2_bwd": dict(dy=_act(lambda a: 4 * _NHW(a), "C", "lddy"), dx=_act(_NHW, "C", "lddx", rmw=_nz("accumulate"))),
    "mi355_add": dict(a=_act("M", "C", "lda"), b=_act("M", "C", "ldb", null=True), y=_act("M", "C", "ldy")),
    "mi355_relu_bwd": dict(dy=_act("M", "C", "lddy"), y=_act("M", "C", "ldy"), dx=_act("M", "C", "lddx")),
    # ---- attention gate / one-channel 1x1
    "mi355_rowdot_fwd": dict(x=_act("M", "C", "ldx"), w=_f("C"), b=_f(lambda a: 1, null=True), z=S(_zplane),
                             partial=_f(lambda a: nb(a.M) * 2, null=True)),
    "mi355_rowdot_bwd": dict(dz=S(_zplane), x=_act("M", "C", "ldx"), w=_f("C"), dx=_act("M", "C", "lddx", null=True, rmw=_nz("accumulate")),
                             partial=_f(lambda a: nb(a.M) * 2 * a.C)),
    "mi355_gate_mul_fwd": dict(x=_act("M", "C", "ldx"), z=_f("M"), scale=_f(lambda a: 1), shift=_f(lambda a: 1), y=_act("M", "C", "ldy")),
    "mi355_gate_mul_bwd": dict(dy=_act("M", "C", "lddy"), x=_act("M", "C", "ldx"), z=_f("M"), **{k: _f(lambda a: 1) for k in ("scale", "shift", "mean", "invstd")},
                               dx=_act("M", "C", "lddx", rmw=_nz("accumulate")), dzn=_f("M"), partial=_f(lambda a: nb(a.M) * 2)),
    "mi355_bn1_bwd_apply": dict(dzn=_f("M"), z=_f("M"), gamma=_f(lambda a: 1), mean=_f(lambda a: 1), invstd=_f(lambda a: 1),
                                sums=_f(lambda a: 2), dz=_f("M")),
    "mi355_gate_psi_fwd": dict(g1=_act("M", "C", "ldg"), x1=_act("M", "C", "ldx", null=True), scale_g=_f("C"), shift_g=_f("C"),
                               scale_x=_f("C", null=True), shift_x=_f("C", null=True), w=_f("C"), b=_f(lambda a: 1, null=True), z=_f("M"),
                               partial=_f(lambda a: nb(a.M) * 2, null=True)),
    "mi355_gate_bn_bwd_reduce": dict(dz=_f("M"), g1=_act("M", "C", "ldg"), x1=_act("M", "C", "ldx", null=True), **_gate_coef, w=_f("C"),
                                     partial=_f(lambda a: nb(a.M) * 5 * a.C)),
    "mi355_gate_bn_bwd_apply": dict(dz=_f("M"), g1=_act("M", "C", "ldg"), x1=_act("M", "C", "ldx", null=True), **_gate_coef, w=_f("C"),
                                    gamma_g=_f("C"), gamma_x=_f("C", null=True), sums_g=_f(lambda a: 2 * a.C), sums_x=_f(lambda a: 2 * a.C, null=True),
                                    dg1=_act("M", "C", "lddg"), dx1=_act("M", "C", "lddx", null=True)),
    # ---- classifier heads
    "mi355_global_pool_fwd": dict(x=_act(lambda a: a.N * a.HW, "C", "ldx"), y=_f(lambda a: a.N * a.C), argmax=_f(lambda a: a.N * a.C, null=True)),
    "mi355_global_pool_bwd": dict(dy=_f(lambda a: a.N * a.C), argmax=_f(lambda a: a.N * a.C, null=True), dx=_act(lambda a: a.N * a.HW, "C", "lddx")),
    "mi355_adaptive_avgpool_fwd": dict(x=_act(_NHW, "C", "ldx"), y=_f(lambda a: a.N * a.C * a.OH * a.OW)),
    "mi355_adaptive_avgpool_bwd": dict(dy=_f(lambda a: a.N * a.C * a.OH * a.OW), dx=_act(_NHW, "C", "lddx")),
    "mi355_linear_fwd": dict(x=_f(lambda a: a.B * a.I), w=_f(lambda a: a.O * a.I), bias=_f("O", null=True), y=_f(lambda a: a.B * a.O)),
    "mi355_linear_bwd": dict(x=_f(lambda a: a.B * a.I), w=_f(lambda a: a.O * a.I), y=_f(lambda a: a.B * a.O), dy=_f(lambda a: a.B * a.O),
                             dx=_f(lambda a: a.B * a.I, null=True), dw=_f(lambda a: a.O * a.I, null=True, rmw=_nz("beta")),
                             db=_f("O", null=True, rmw=_nz("beta")),
                             scratch=_f(lambda a: lib.mi355_linear_bwd_scratch(a.B, a.I, a.O), null=True)),
    "mi355_dropout_fwd": dict(x=_f("n"), y=_f("n"), mask=_f("n", esz=1), counter=_f(lambda a: 1)),
    "mi355_dropout_bwd": dict(dy=_f("n"), mask=_f("n", esz=1), dx=_f("n")),
    # ---- Grad-CAM
    "mi355_cam_seed": dict(logits=_f(lambda a: a.B * a.K), target=_f("B", null=True), dout=_f(lambda a: a.B * a.K), target_out=_f("B")),
    "mi355_gradcam": dict(A=_act(lambda a: a.N * a.HW, "C", "ldA"), dA=_act(lambda a: a.N * a.HW, "C", "lddA"), cam_lowres=_f(lambda a: a.N * a.HW)),
}

# Persistent state, read-modify-write by design: (launcher, slot) and the words of mi355conv.h that say so.  The first three are
# the only ones a plan emits; the optimiser's and the loss scaler's launches are issued by mi355/optim.py and mi355/amp.py.
PERSISTENT_STATE = [
    ("mi355_bn_finalize", "running_mean", "updates running stats (momentum, unbiased var)"),
    ("mi355_bn_finalize", "running_var", "updates running stats (momentum, unbiased var)"),
    ("mi355_bn_finalize", "nbt", "and num_batches_tracked"),
    ("mi355_step_tick", "step", "step[0] += 1 unless found_inf[0] != 0"),
    ("mi355_amp_update", "scale", "scale *= backoff"),
    ("mi355_amp_update", "inv_scale", "inv_scale = 1/scale"),
    ("mi355_amp_update", "growth_tracker", "tracker = 0"),
]


# Scratch a launcher writes and reads within itself (mi355conv.h, mi355_linear_bwd_scratch: "fold 16 deterministic output-range
# partials"): no other launch has to read it.
SCRATCH = {("mi355_linear_bwd", "scratch")}


# ---- regions --------------------------------------------------------------------------------------------------------------------
class Region:
    """`rows` rows of `width` bytes, `pitch` bytes apart, from byte `start` of storage `key`"""
    __slots__ = ("key", "start", "rows", "width", "pitch")

    def __init__(self, key, start, rows_, width, pitch):
        self.key, self.start, self.rows, self.width, self.pitch = key, int(start), int(rows_), int(width), int(pitch)
        if self.rows == 1 or self.pitch == self.width:          # contiguous: one row
            self.width, self.pitch, self.rows = self.width * self.rows, self.width * self.rows, 1

    @property
    def end(self):
        return self.start + (self.rows - 1) * self.pitch + self.width if self.rows and self.width else self.start

    def __repr__(self):
        return f"{self.key}[{self.start}:{self.end}] ({self.rows} x {self.width} B @ {self.pitch} B)"


class Access:
    __slots__ = ("slot", "mode", "state", "region", "via")

    def __init__(self, slot, mode, region, state=False, via=None):
        self.slot, self.mode, self.region, self.state, self.via = slot, mode, region, state, via

    @property
    def reads(self):
        return self.mode in ("r", "rw")

    @property
    def writes(self):
        return self.mode in ("w", "rw")


def storage_key(t):
    s = t.untyped_storage()
    return ("mem", s.data_ptr()), t.data_ptr() - s.data_ptr(), s.nbytes()


class Resolver:
    """regions of one plan's launches.  Storages are told apart by their base address; the two shared workspaces are the keys
    ('ws', 'bytes') and ('ws', 'f32'), sized as Plan sizes them (``ws_size``, in bytes: the seeded-fault tests shrink it)."""

    def __init__(self, plan):
        self.plan = plan
        self.size = {}                 # key -> bytes
        self.ws_size = {k: t.numel() * t.element_size() for k, t in plan.ws.items()}
        self._ws_ptr = {t.data_ptr(): k for k, t in plan.ws.items()}
        self._bases = []               # (base address, bytes, key) of every storage met, for the pack table's raw pointers
        for t in [plan.flat_p, plan.engine.flat_g] + list(plan.keep) + list(plan.engine.net.buffers()):
            self._tensor(t)

    def _tensor(self, t, off=0):
        if t.data_ptr() in self._ws_ptr and t is self.plan.ws[self._ws_ptr[t.data_ptr()]]:
            return ("ws", self._ws_ptr[t.data_ptr()]), off
        key, o, n = storage_key(t)
        if key not in self.size:
            self.size[key] = n
            self._bases.append((key[1], n, key))
        return key, o + off

    def nbytes(self, key):
        return self.ws_size[key[1]] if key[0] == "ws" else self.size[key]

    def _pointer(self, ptr):
        for base, n, key in self._bases:
            if base <= ptr < base + n:
                return key, ptr - base
        raise AccessError(f"pack table: pointer {ptr:#x} lies in no storage of the plan")

    def _where(self, l, slot, arg, ext):
        """(key, byte offset) of a pointer argument; a T / V handle must agree with the extent its scalars give"""
        M, C, ld, esz = ext
        if isinstance(arg, graph.T):
            if (M, C, ld, esz) != (arg.M, arg.C, arg.ld, arg.buf.element_size()):
                raise AccessError(f"{l.name}.{slot}: scalars say {M} rows x {C} @ {ld} of {esz} B, the handle is "
                                  f"{arg.M} x {arg.C} @ {arg.ld} of {arg.buf.element_size()} B")
            return self._tensor(arg.buf, arg.off * esz)
        if isinstance(arg, graph.V):
            if M != 1 or C != arg.B * arg.F or esz != 4:
                raise AccessError(f"{l.name}.{slot}: scalars say {M} x {C} of {esz} B, the handle is [{arg.B}, {arg.F}] fp32")
            return self._tensor(arg.buf)
        if isinstance(arg, graph.GRef):
            return self._tensor(arg.tensor, arg.off)
        if isinstance(arg, graph.Ws):
            return ("ws", arg.kind), 0
        if isinstance(arg, graph.Builder._WsOff):
            return ("ws", arg.ws.kind), arg.off
        if isinstance(arg, tuple) and len(arg) == 2 and isinstance(arg[0], torch.Tensor):
            return self._tensor(arg[0], int(arg[1]))
        if isinstance(arg, torch.Tensor):
            return self._tensor(arg)
        raise AccessError(f"{l.name}.{slot}: cannot resolve an argument of type {type(arg).__name__}")

    def namespace(self, l):
        slots = SLOTS.get(l.name)
        if slots is None:
            raise AccessError(f"{l.name} is not a prototype of include/mi355conv.h")
        if len(slots) != len(l.args) + 1 or slots[-1][0] != "s":
            raise AccessError(f"{l.name}: {len(l.args)} arguments built, the prototype takes {len(slots) - 1} and the stream")
        a = SimpleNamespace(**{("in_" if n == "in" else n): v for (n, _), v in zip(slots, l.args)})
        if hasattr(a, "dtype"):
            a.e = ESZ[a.dtype]
        return a, slots[:-1]

    def accesses(self, l):
        entry = TABLE.get(l.name)
        if entry is None:
            raise AccessError(f"{l.name}: no entry in the access table")
        a, slots = self.namespace(l)
        ptr_slots = [n for n, k in slots if k != "scalar"]
        if set(entry) != set(ptr_slots):
            raise AccessError(f"{l.name}: the entry describes {sorted(entry)}, the prototype's pointers are {sorted(ptr_slots)}")
        if l.name == "mi355_conv2d_wgrad_multi":
            for i in range(6):
                if (getattr(a, f"x{i}") is not None, getattr(a, f"dy{i}") is not None) != (i < a.napp, i < a.napp):
                    raise AccessError(f"mi355_conv2d_wgrad_multi: pair {i} of napp = {a.napp}")
        out = []
        for (name, kind), arg in zip(slots, l.args):
            if kind == "scalar":
                if isinstance(arg, (graph.T, graph.V, graph.GRef, graph.Ws, torch.Tensor, tuple, graph.Builder._WsOff)):
                    raise AccessError(f"{l.name}.{name}: a buffer in a scalar slot")
                continue
            spec = entry[name]
            if arg is None:
                if not spec.null:
                    raise AccessError(f"{l.name}.{name} is NULL and the table says it may not be")
                continue
            ext = spec.extent(a)
            key, off = self._where(l, name, arg, ext)
            M, C, ld, esz = ext
            mode = "r" if kind == "in" else ("rw" if (spec.state or (spec.rmw is not None and spec.rmw(a))) else "w")
            if kind == "in" and (spec.rmw is not None or spec.state):
                raise AccessError(f"{l.name}.{name}: a const slot cannot be read-modify-write")
            out.append(Access(name, mode, Region(key, off, M, C * esz, ld * esz), spec.state))
        if l.name == "mi355_pack_conv_weights_batched":
            out += self.indirect_accesses(l, a)
        return out

    def indirect_accesses(self, l, a):
        """the rows of the pack table {w, wf, wb, Co, Ci, Cip, KH*KW, transposed, scale} (mi355conv.h, mi355_pack_conv_weights_batched)"""
        table = l.args[0]
        assert a.fields == 9 and tuple(table.shape) == (a.n, 9) and table.dtype == torch.int64
        out = []
        for r, (w, wf, wb, co, ci, cip, taps, tr, sc) in enumerate(table.cpu().tolist()):
            def acc(slot, mode, ptr, n, esz):
                key, off = self._pointer(ptr)
                out.append(Access(f"table[{r}].{slot}", mode, Region(key, off, 1, n * esz, n * esz), via="table"))
            acc("w", "r", w, co * ci * taps, 4)
            acc("wf", "w", wf, co * taps * cip, a.e)
            if wb:
                acc("wb", "w", wb, cip * taps * co, a.e)
            if sc:
                acc("scale", "r", sc, co, 4)
        return out
