"""Static checks over a whole launch plan (tests/test_plan_dataflow_cpu.py, tests/test_gpu_plan_dataflow.py): bounds, defined before
use, side-stream hazards, data-parallel buckets, live results.  Nothing is launched: the walk reads the un-bound ``Launch`` objects
through the access table of tests/plan_access.py.

One walk over ``pre + fwd`` and then ``bwd``, in order, with per-unit state in numpy arrays per storage (a unit is the storage's
element: every region is a whole number of them).  The stream rule is the one of csrc/plan.cpp and Plan.run_calls_two_streams:
main launches are ordered, side launches are ordered; a side group that starts at position f happens after the main launches below
f; main never happens after a side launch before the join at the end of the list."""
import copy

import numpy as np

import plan_access as pa


class Violation:
    __slots__ = ("kind", "phase", "index", "launcher", "slot", "key", "lo", "hi", "what")

    def __init__(self, kind, phase, index, launcher, slot, key, lo, hi, what):
        self.kind, self.phase, self.index, self.launcher, self.slot = kind, phase, index, launcher, slot
        self.key, self.lo, self.hi, self.what = key, lo, hi, what

    def ident(self):
        return (self.kind, self.phase, self.index, self.slot)

    def __repr__(self):
        return f"{self.kind}: {self.phase}[{self.index}] {self.launcher}.{self.slot} bytes [{self.lo}, {self.hi}) of {self.key}: {self.what}"


class PlanView:
    """the launch lists of a plan as copies that a test may edit (seeded faults), with the sizes the bounds check holds them to"""

    def __init__(self, plan):
        self.plan = plan
        self.pre, self.fwd, self.bwd = ([copy.copy(l) for l in lst] for lst in (plan.pre, plan.fwd, plan.bwd))
        self.res = pa.Resolver(plan)
        self.size_override = {}            # storage key -> bytes (a buffer made smaller)

    def nbytes(self, key):
        return self.size_override.get(key, self.res.nbytes(key))

    def launches(self):
        """[(phase, index in its list, launch)]: 'fwd' counts pre + fwd, as Plan.bind does"""
        return [("fwd", i, l) for i, l in enumerate(self.pre + self.fwd)] + [("bwd", i, l) for i, l in enumerate(self.bwd)]

    def tensor_key(self, t, off=0):
        return self.res._tensor(t, off)


class _State:
    __slots__ = ("unit", "written", "main_w", "main_r", "side_r", "side_w", "lastw")

    def __init__(self, nbytes, unit, ws):
        n = -(-nbytes // unit)
        self.unit = unit
        self.written = np.zeros(n, np.bool_)
        self.main_w = np.zeros(n, np.uint16)       # position + 1 of the last main-stream writer / reader, 0 = none
        self.main_r = np.zeros(n, np.uint16)
        self.side_r = np.zeros(n, np.bool_)
        self.side_w = np.zeros(n, np.bool_)
        self.lastw = np.zeros(n, np.uint16) if ws else None     # workspaces: last writer on either stream


def _select(arr, reg, unit, nbytes):
    """the units of `reg` inside [0, nbytes): (writable view of `arr`, None), or (None, unit indices) for a region that sticks out"""
    if reg.rows == 0 or reg.width == 0:
        return arr[:0], None
    if reg.start >= 0 and reg.end <= nbytes:
        if reg.rows == 1:
            return arr[reg.start // unit: reg.end // unit], None
        return np.lib.stride_tricks.as_strided(arr[reg.start // unit:], shape=(reg.rows, reg.width // unit),
                                               strides=(reg.pitch // unit * arr.itemsize, arr.itemsize)), None
    idx = (reg.start + np.arange(reg.rows, dtype=np.int64)[:, None] * reg.pitch + np.arange(0, reg.width, unit, dtype=np.int64)[None, :]).ravel()
    return None, idx[(idx >= 0) & (idx + unit <= nbytes)] // unit


def _pick(arr, reg, unit, nbytes):
    v, idx = _select(arr, reg, unit, nbytes)
    return v if idx is None else arr[idx]


def _put(arr, reg, unit, nbytes, value):
    v, idx = _select(arr, reg, unit, nbytes)
    if idx is None:
        v[...] = value
    else:
        arr[idx] = value


def external_keys(view):
    """storages a step may read without having written them: the flat parameters, the module's buffers (persistent state among
    them), the dropout counter, the network input, the loss's seed into dout (training plans), the pack tables"""
    plan = view.plan
    ext = {view.tensor_key(plan.flat_p)[0]}
    ext |= {view.tensor_key(b)[0] for b in plan.engine.net.buffers()}
    ext.add(view.tensor_key(plan.input[0])[0])
    if plan.engine._drop_counter is not None:
        ext.add(view.tensor_key(plan.engine._drop_counter)[0])
    if plan.dout is not None and plan.cam is None:
        ext.add(view.tensor_key(plan.dout)[0])
    for l in plan.pre + ([plan.static_pack] if plan.static_pack is not None else []):
        if l.name == "mi355_pack_conv_weights_batched":
            ext.add(view.tensor_key(l.args[0])[0])
    return ext


def resolve(view):
    """[(phase, i, launch, [Access])] of the whole step; AccessError when the table cannot describe a launch"""
    return [(ph, i, l, view.res.accesses(l)) for ph, i, l in view.launches()]


def verify(view, cuts=(), side_stream=True, stats=None):
    """Checks 1 (bounds), 2 (defined before use; a workspace read sees the workspace's LATEST writer on every byte: produce, then
    consume before anything else uses the workspace, which is how every builder rule uses it; and every workspace write is read by
    some launch), 3 (side-stream hazards; ``cuts``: backward positions at
    which a new range starts and its first side group re-forks) and 5 (live results).  -> [Violation]"""
    plan = view.plan
    out = []
    steps = resolve(view)
    assert len(steps) < 65535
    if plan.static_pack is not None:       # frozen-weight packs: written by Plan.refresh_static_packs in front of the step
        steps = [("static", 0, plan.static_pack, view.res.accesses(plan.static_pack))] + steps
    ext = external_keys(view)
    unit_of, written_keys = {}, set()
    for _, _, l, accs in steps:
        for ac in accs:
            r = ac.region
            u = unit_of.get(r.key, 8)
            for v in (r.start, r.width, r.pitch):
                while v % u:
                    u //= 2
            unit_of[r.key] = u
            if ac.writes:
                written_keys.add(r.key)
    state = {k: _State(view.nbytes(k), unit_of[k], k[0] == "ws") for k in written_keys}
    last_ws = {}                           # workspace -> position + 1 of the launch that wrote into it last
    unread = {}                            # position + 1 of a workspace writer nothing has read from yet -> its launch
    cuts = set(cuts)
    fork, prev_side = 0, False
    n_side = n_forks = 0
    for pos, (ph, i, l, accs) in enumerate(steps):
        side = bool(side_stream and ph == "bwd" and l.side)
        if ph == "bwd" and i in cuts:
            prev_side = False
        if side and not prev_side:
            fork, n_forks = pos, n_forks + 1
        prev_side = side
        n_side += side
        tag = pos + 1

        def bad(kind, ac, what):
            out.append(Violation(kind, ph, i, l.name, ac.slot, ac.region.key, ac.region.start, ac.region.end, what))
        sels = []
        for ac in accs:                    # all checks against the state BEFORE this launch, then the updates
            r = ac.region
            size = view.nbytes(r.key)
            if r.start < 0 or r.end > size:
                bad("bounds", ac, f"the storage has {size} bytes")
            st = state.get(r.key)
            if st is None:
                if r.key not in ext:
                    bad("undefined", ac, "read of a buffer that no launch writes")
                sels.append(None)
                continue
            pick = lambda arr, r=r, st=st, size=size: _pick(arr, r, st.unit, size)
            sels.append(pick)
            if ac.reads and r.key not in ext and not pick(st.written).all():
                bad("undefined", ac, "reads bytes that no earlier launch of the step wrote")
            if not side:
                if ac.reads and pick(st.side_w).any():
                    bad("hazard", ac, "main-stream read of bytes a side-stream launch wrote (no join in between)")
                if ac.writes and (pick(st.side_w).any() or pick(st.side_r).any()):
                    bad("hazard", ac, "main-stream write of bytes a side-stream launch read or wrote (no join in between)")
            else:
                if pick(st.main_w).max(initial=0) > fork:
                    bad("hazard", ac, f"side-stream access to bytes a main-stream launch at or behind its fork wrote")
                if ac.writes and pick(st.main_r).max(initial=0) > fork:
                    bad("hazard", ac, f"side-stream write of bytes a main-stream launch at or behind its fork read")
            if ac.reads and st.lastw is not None:
                lw = pick(st.lastw)
                for w in ([lw.max()] if lw.size and lw.min() == lw.max() else np.unique(lw)):
                    if int(w) in unread:
                        del unread[int(w)]
                if lw.size and (lw.min() != last_ws[r.key] or lw.max() != last_ws[r.key]) and pick(st.written).all():
                    bad("stale", ac, f"workspace bytes whose writer is not the workspace's latest (position {last_ws[r.key] - 1}): "
                                     "another launch has used the workspace since they were produced")
        for ac, pick in zip(accs, sels):
            if pick is None:
                continue
            st = state[ac.region.key]
            if ac.reads:
                _put(st.side_r if side else st.main_r, ac.region, st.unit, view.nbytes(ac.region.key), True if side else tag)
            if ac.writes:
                size = view.nbytes(ac.region.key)
                _put(st.written, ac.region, st.unit, size, True)
                _put(st.side_w if side else st.main_w, ac.region, st.unit, size, True if side else tag)
                if st.lastw is not None:
                    _put(st.lastw, ac.region, st.unit, size, tag)
                    last_ws[ac.region.key] = tag
                    if (l.name, ac.slot) not in pa.SCRATCH:
                        unread[tag] = (ph, i, l, ac)
    for ph, i, l, ac in unread.values():
        out.append(Violation("dead", ph, i, l.name, ac.slot, ac.region.key, ac.region.start, ac.region.end,
                             "workspace bytes that no launch reads: overwritten, or left at the end of the step, unread"))
    # 5. live results: the output, every gradient the plan promises (and the Grad-CAM map of an explain plan)
    def live(t, nbytes, what, off=0):
        key, o = view.tensor_key(t, off)
        st = state.get(key)
        reg = pa.Region(key, o, 1, nbytes, nbytes)
        if st is None or not _pick(st.written, reg, st.unit, view.nbytes(key)).all():
            out.append(Violation("live", "-", -1, "-", what, key, o, o + nbytes, "never (or not completely) written"))
    kind, buf, shape = plan.output
    live(buf if kind == "z" else buf.buf, int(np.prod(shape)) * 4, "output")
    zero = {id(p) for p in plan.zero_grad_params}
    if plan.bwd:
        for p in plan.grad_params:
            if id(p) not in zero:
                o, n = plan.engine.offsets[id(p)]
                live(plan.engine.flat_g, n * 4, f"grad[{o}:{o + n}]", o * 4)
    if plan.cam is not None:
        live(plan.cam_lowres, plan.cam.N * plan.cam.H * plan.cam.W * 4, "cam_lowres")
        live(plan.cam_target, plan.cam.N * 4, "cam_target")
    if stats is not None:
        stats.update(launches=len(steps), side=n_side, forks=n_forks, bytes=sum(view.nbytes(k) for k in unit_of))
    return out


# ---- 4. data-parallel buckets ----------------------------------------------------------------------------------------------------
def grad_touch(view):
    """per fp32 element of flat_g: index of the last backward launch that touches it, and of the last that writes it (-1: none),
    recomputed from the access table"""
    plan = view.plan
    gkey, _ = view.tensor_key(plan.engine.flat_g)
    n = plan.engine.flat_g.numel()
    touch, write = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for i, l in enumerate(view.bwd):
        for ac in view.res.accesses(l):
            if ac.region.key == gkey:
                _put(touch, ac.region, 4, n * 4, i)
                if ac.writes:
                    _put(write, ac.region, 4, n * 4, i)
    return touch, write


def check_buckets(view, buckets):
    """buckets: [(ready, lo, hi)] of DataParallel.schedule, in fp32 elements of flat_g"""
    plan = view.plan
    eng = plan.engine
    gkey, _ = view.tensor_key(eng.flat_g)
    touch, write = grad_touch(view)
    out = []

    def bad(b, what, index=-1, launcher="-"):
        ready, lo, hi = buckets[b]
        out.append(Violation("bucket", "bwd", index, launcher, f"bucket[{b}]", gkey, lo * 4, hi * 4, what))
    covered = np.zeros(eng.flat_g.numel(), np.int32)
    for b, (ready, lo, hi) in enumerate(buckets):
        if not (0 <= lo < hi <= eng.flat_g.numel()):
            bad(b, f"[{lo}, {hi}) is not a range of flat_g")
            continue
        covered[lo:hi] += 1
        late = int(touch[lo:hi].max())
        if late > ready:
            bad(b, f"touched by a launch behind ready = {ready}: the collective is already enqueued", late, view.bwd[late].name)
        last = int(write[lo:hi].max())
        if last != ready:
            bad(b, f"ready = {ready}, the last writer by the access table is launch {last}")
    if covered.max(initial=0) > 1:
        bad(0, "buckets overlap")
    seen = set()
    for p in list(plan.grad_params) + list(plan.zero_grad_params):
        if id(p) in seen:
            continue
        seen.add(id(p))
        o, n = eng.offsets[id(p)]
        if not (covered[o:o + n] == 1).all():
            bad(0, f"parameter at [{o}, {o + n}) is not covered exactly once")
    return out


# ---- the same table on the device (tests/test_gpu_plan_dataflow.py) ----------------------------------------------------------------
def plan_buffers(view):
    """[(storage key, tensor)] of the buffers a step may write: plan.keep, the two workspaces, flat_g"""
    plan = view.plan
    out, seen = [], set()
    for t in list(plan.keep) + list(plan.ws.values()) + [plan.engine.flat_g]:
        key, off = view.tensor_key(t)
        assert off == 0 and key not in seen
        seen.add(key)
        out.append((key, t))
    return out


def write_regions(view, launches):
    """{storage key: [Region]} of everything `launches` write, by the access table"""
    out = {}
    for l in launches:
        for ac in view.res.accesses(l):
            if ac.writes:
                out.setdefault(ac.region.key, []).append(ac.region)
    return out


def byte_mask(regions, nbytes):
    m = np.zeros(nbytes, np.bool_)
    for r in regions:
        _put(m, r, 1, nbytes, True)
    return m
