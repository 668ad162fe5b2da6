"""CPU: dataflow and stream-hazard verifier over whole launch plans (no kernels run).

tests/plan_access.py says what every launcher touches; tests/plan_verify.py walks a plan once and checks bounds, defined before
use, side-stream hazards, the data-parallel bucket schedule and live results.  Here: every model's training plans (fp32, bf16,
fp16), eval plans and the classifiers' explain plans are clean; the builder's A/B switches are checked in child processes (they
are read at import); and six faults seeded into copies of a real plan are each reported, with nothing else."""
import json
import os
import re
import subprocess
import sys
import tempfile
import zlib

import pytest
import torch

import plan_access as pa
import plan_verify as pv
from mi355 import dp, graph
from mi355.lib import available
from test_plan_cpu import _models

pytestmark = pytest.mark.skipif(not available(), reason="libmi355conv.so not built")

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CLASSIFIERS = [n for n in _models() if "resnet" in n.lower() or "VGG" in n]
BUCKET_MB = 0.25          # small buckets: several per plan, so that the schedule and the range cuts are exercised


def _ctor(name):
    if name.startswith("ResNetUnet"):
        from models.segmentation_models.ResnetUnet import ResNetUnet
        return (lambda: ResNetUnet(freeze=name.endswith("frozen"))), (2, 3, 64, 64)
    return _models()[name]


MODELS = list(_models()) + ["ResNetUnet_frozen", "ResNetUnet_unfrozen"]
CASES = [(m, d, "train") for m in MODELS for d in DTYPES] + [(m, d, "eval") for m in MODELS for d in ("fp32", "bf16")] + \
        [(m, d, "explain") for m in CLASSIFIERS for d in ("fp32", "bf16")]


def build_plan(name, dtype, kind):
    ctor, shape = _ctor(name)
    net = ctor()
    net.train() if kind == "train" else net.eval()
    net.engine.flatten()
    plan = net.engine.plan_for(shape, kind == "train", kind == "train", DTYPES[dtype], explain=kind == "explain")
    return net, plan


def check_plan(net, plan):
    """every check over one plan -> (row of the report, violations)"""
    view = pv.PlanView(plan)
    stats = {}
    bad = pv.verify(view, stats=stats)
    buckets = []
    if plan.bwd and plan.grad_params:
        buckets = dp.DataParallel(net, bucket_mb=BUCKET_MB).schedule(plan)
        assert len(buckets) > 1 or sum(p.numel() for p in plan.grad_params) * 4 <= BUCKET_MB * 2 ** 20
        bad += pv.check_buckets(view, buckets)
        cuts = sorted({ready + 1 for ready, _, _ in buckets})
        bad += pv.verify(view, cuts=cuts)          # each range re-forks, as both replay paths do
    names = sorted(l.name for l in plan.pre + plan.fwd + plan.bwd)
    row = dict(launches=stats["launches"], side=stats["side"], forks=stats["forks"], buckets=len(buckets), bytes=stats["bytes"],
               violations=len(bad), digest=zlib.crc32(" ".join(names).encode()))
    return row, bad


_ROWS = {}


def _row(case):
    if case not in _ROWS:
        net, plan = build_plan(*case)
        row, bad = check_plan(net, plan)
        _ROWS[case] = (row, [repr(v) for v in bad[:20]])
    return _ROWS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))
def test_plan_is_clean(case):
    row, bad = _row(case)
    assert not bad, "\n".join(bad)
    assert row["launches"] > 0 and (case[2] != "train" or row["side"] > 0)


# ---- the access table ---------------------------------------------------------------------------------------------------------
def test_access_table_is_complete_and_takes_its_modes_from_the_header():
    src = open(graph.__file__).read()
    emitted = set(re.findall(r'Launch\(\s*"(mi355_\w+)"', src)) | set(re.findall(r'"(mi355_\w+)" if at else "(mi355_\w+)"', src)[0])
    assert len(emitted) > 40 and emitted <= set(pa.TABLE), sorted(emitted - set(pa.TABLE))
    for name, entry in pa.TABLE.items():
        ptrs = {n: k for n, k in pa.SLOTS[name] if k != "scalar"}
        assert set(entry) == set(ptrs), name
        for slot, spec in entry.items():           # read-modify-write and state only on slots the header leaves non-const
            assert ptrs[slot] == "out" or (spec.rmw is None and not spec.state), (name, slot)
    # mi355.lib's parser and this one see the same prototypes in the same order
    from mi355.lib import lib
    assert {n: [s for s, _ in v] for n, v in pa.SLOTS.items()} == {n: [s for _, s in v[1]] for n, v in lib.protos.items()}
    # the header's own const: a few anchors
    k = dict(pa.SLOTS["mi355_conv2d_igemm"])
    assert (k["in"], k["wk"], k["bias"], k["out"], k["stats"], k["N"]) == ("in", "in", "in", "out", "out", "scalar")
    assert dict(pa.SLOTS["mi355_dropout_fwd"])["counter"] == "in" and dict(pa.SLOTS["mi355_bn_finalize"])["nbt"] == "out"


def test_persistent_state_is_the_explicit_list():
    listed = {(n, s) for n, s, _ in pa.PERSISTENT_STATE}
    assert {(n, s) for n, e in pa.TABLE.items() for s, spec in e.items() if spec.state} <= listed
    for name, slot, words in pa.PERSISTENT_STATE:
        assert dict(pa.SLOTS[name])[slot] == "out", (name, slot)
        assert words in " ".join(open(pa.HEADER).read().split()), (name, slot, words)       # the header describes it as state


def test_a_launcher_without_an_entry_is_an_error(monkeypatch):
    net, plan = build_plan("ResNet18", "bf16", "train")
    entry = dict(pa.TABLE["mi355_bn_finalize"])
    monkeypatch.delitem(pa.TABLE, "mi355_maxpool_fwd")
    with pytest.raises(pa.AccessError, match="no entry"):
        pv.verify(pv.PlanView(plan))
    monkeypatch.undo()
    del entry["nbt"]
    monkeypatch.setitem(pa.TABLE, "mi355_bn_finalize", entry)
    with pytest.raises(pa.AccessError, match="nbt"):
        pv.verify(pv.PlanView(plan))
    monkeypatch.undo()
    view = pv.PlanView(plan)                      # a handle that disagrees with the scalars beside it
    i = next(i for i, l in enumerate(view.fwd) if l.name == "mi355_conv2d_igemm")
    a = list(view.fwd[i].args)
    a[8] += 8                                     # ldi
    view.fwd[i].args = tuple(a)
    with pytest.raises(pa.AccessError, match="the handle is"):
        pv.verify(view)


# ---- the verifier bites: one seeded fault at a time ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet():
    net, plan = build_plan("AttentionUNet", "bf16", "train")
    assert not pv.verify(pv.PlanView(plan))
    return net, plan


def _idents(vs):
    return sorted({v.ident() for v in vs})


def _uses_ws(l, kind):
    return any((isinstance(a, graph.Ws) and a.kind == kind) for a in l.args)


def test_fault_a_slab_workspace_user_on_the_main_stream(unet):
    """the historical race: a weight-gradient launch on the main stream writes the slab the side stream is still folding"""
    view = pv.PlanView(unet[1])
    users = [i for i, l in enumerate(view.bwd) if l.name == "mi355_conv2d_wgrad" and l.side and _uses_ws(l, "bytes")]
    i = users[3]
    view.bwd[i].side = False
    got = pv.verify(view)
    assert _idents(got) == [("hazard", "bwd", i, "ws")], got
    assert "main-stream write" in got[0].what


def test_fault_b_producer_moved_to_the_side_stream(unet):
    view = pv.PlanView(unet[1])
    cand = [i for i, l in enumerate(view.bwd) if l.name == "mi355_conv2d_igemm" and not l.side and l.arg("accumulate") == 0]
    res = view.res
    j = next(j for j in cand[len(cand) // 2:] if [ac.region.rows for ac in res.accesses(view.bwd[j]) if ac.writes] == [1])
    mine = [ac.region for ac in res.accesses(view.bwd[j]) if ac.writes]
    lo, hi, key = mine[0].start, mine[0].end, mine[0].key
    want = set()                                  # every later main-stream launch that touches those bytes (one contiguous range)
    for i in range(j + 1, len(view.bwd)):
        if not view.bwd[i].side:
            for ac in res.accesses(view.bwd[i]):
                r = ac.region
                if r.key == key and r.start < hi and r.end > lo:
                    assert r.rows == 1 or r.pitch >= r.width
                    want.add(("hazard", "bwd", i, ac.slot))
    assert want
    view.bwd[j].side = True
    got = pv.verify(view)
    assert set(_idents(got)) == want, got
    assert min(v.index for v in got) > j and all(v.key == key for v in got)


def test_fault_c_first_write_of_an_activation_gradient_deleted():
    """ResNet18: a block's input feeds the block and its downsample branch; the first data gradient overwrites, the second accumulates"""
    net, plan = build_plan("ResNet18", "bf16", "train")
    view = pv.PlanView(plan)
    res = view.res
    acc = [res.accesses(l) for l in view.bwd]
    gkey = view.tensor_key(plan.engine.flat_g)[0]
    pick = None
    for f, l in enumerate(view.bwd):
        w = [ac for ac in acc[f] if ac.writes]
        if len(w) != 1 or w[0].mode != "w" or w[0].region.key[0] == "ws" or w[0].region.key == gkey:
            continue
        r = w[0].region
        for i in range(f + 1, len(view.bwd)):         # the next launch that touches the region: an accumulate onto exactly it?
            hit = [ac for ac in acc[i] if ac.region.key == r.key and ac.region.start < r.end and ac.region.end > r.start]
            if hit:
                if len(hit) == 1 and hit[0].mode == "rw" and (hit[0].region.start, hit[0].region.end, hit[0].region.rows) == (r.start, r.end, r.rows):
                    pick = (f, i, hit[0].slot)
                break
        if pick:
            break
    assert pick, "no first-write / accumulate pair in this plan"
    f, i, slot = pick
    del view.bwd[f]
    got = pv.verify(view)
    assert _idents(got) == [("undefined", "bwd", i - 1, slot)], got


def test_fault_d_workspace_and_partial_rows_one_element_short(unet):
    view = pv.PlanView(unet[1])
    steps = pv.resolve(view)
    full = view.res.ws_size["bytes"]
    assert full > 64
    want = sorted({("bounds", ph, i, ac.slot) for ph, i, l, accs in steps for ac in accs if ac.region.key == ("ws", "bytes") and ac.region.end == full})
    assert want                                    # (the largest request: its weight-gradient launch and its reduce)
    view.res.ws_size["bytes"] = full - 4
    assert _idents(pv.verify(view)) == want
    # one partial-row buffer of its own: the attention gate's five quantities per channel and row
    view = pv.PlanView(unet[1])
    l = next(l for l in view.bwd if l.name == "mi355_gate_bn_bwd_reduce")
    part = l.arg("partial")
    assert isinstance(part, torch.Tensor)
    key, _ = view.tensor_key(part)
    full = view.nbytes(key)
    assert full == part.numel() * 4 > 32
    want = sorted({("bounds", ph, i, ac.slot) for ph, i, l, accs in steps for ac in accs if ac.region.key == key and ac.region.end == full})
    assert ("bounds", "bwd", view.bwd.index(l), "partial") in want
    view.size_override[key] = full - 4
    assert _idents(pv.verify(view)) == want


def test_fault_e_bucket_ready_one_launch_early(unet):
    net, plan = unet
    view = pv.PlanView(plan)
    buckets = list(dp.DataParallel(net, bucket_mb=BUCKET_MB).schedule(plan))
    assert not pv.check_buckets(view, buckets)
    b = next(b for b, (ready, _, _) in enumerate(buckets) if ready > 0 and b > 0)
    ready, lo, hi = buckets[b]
    buckets[b] = (ready - 1, lo, hi)
    got = pv.check_buckets(view, buckets)
    assert _idents(got) == [("bucket", "bwd", -1, f"bucket[{b}]"), ("bucket", "bwd", ready, f"bucket[{b}]")], got


def test_fault_f_workspace_producer_behind_its_consumer(unet):
    view = pv.PlanView(unet[1])
    res = view.res
    p = [i for i, l in enumerate(view.bwd) if l.name == "mi355_bn_bwd_reduce" and _uses_ws(l, "f32")][-1]
    c = next(i for i in range(p + 1, len(view.bwd)) if any(ac.reads and ac.region.key == ("ws", "f32") for ac in res.accesses(view.bwd[i])))
    assert c == p + 1 and view.bwd[c].name == "mi355_bn_bwd_finalize"
    moved = view.bwd[c + 1]
    made = {ac.region.key for ac in res.accesses(view.bwd[c]) if ac.writes and ac.region.key[0] != "ws"}
    gkey = view.tensor_key(unet[1].engine.flat_g)[0]
    # the consumer now folds what another layer left in the workspace; the launch that changed places with the producer reads
    # what the consumer has not written yet (the layer's sums)
    # (workspace regions start at byte 0: what earlier launches of the step wrote there is one range)
    prior = max(ac.region.end for l in view.pre + view.fwd + view.bwd[:p] for ac in res.accesses(l) if ac.writes and ac.region.key == ("ws", "f32"))
    need = next(ac.region.end for ac in res.accesses(view.bwd[c]) if ac.slot == "partial")
    latest = [ac.region.end for l in view.pre + view.fwd + view.bwd[:p] for ac in res.accesses(l) if ac.writes and ac.region.key == ("ws", "f32")][-1]
    # ... unless the workspace's latest writer left at least as many rows there: then only the producer's own write, which nothing reads
    # any more, gives the swap away
    want = [("dead", "bwd", c + 1, "partial")] + ([("undefined", "bwd", c, "partial")] if prior < need else
                                                   [("stale", "bwd", c, "partial")] if latest < need else []) + [("undefined", "bwd", p, ac.slot) for ac in res.accesses(moved)
                                                if ac.reads and ac.region.key in made and ac.region.key != gkey]
    assert len(want) >= 2
    view.bwd[p], view.bwd[c + 1] = view.bwd[c + 1], view.bwd[p]
    assert _idents(pv.verify(view)) == sorted(want)


# ---- the builder's A/B switches: read at import, so one child process per switch ------------------------------------------------
SWITCHES = {"fuse_pool": ("MI355_FUSE_POOL", "FUSE_POOL"), "fuse_pool_bwd": ("MI355_FUSE_POOL_BWD", "FUSE_POOL_BWD"),
            "side_colsum": ("MI355_SIDE_COLSUM", "SIDE_COLSUM"), "bn_act_windows": ("MI355_BN_ACT_WINDOWS", "BN_ACT_WINDOWS"),
            "fuse_residual": ("MI355_FUSE_RESIDUAL", "FUSE_RESIDUAL"), "wgrad_multi": ("MI355_WGRAD_MULTI", None),
            "defer_post": ("MI355_DEFER_POST", "DEFER_POST")}
SWITCH_MODELS = ("AttentionUNet", "R2AttU_Net", "ResNet18")
HERE = os.environ.get("PLANFLOW_SWITCH", "")
REPORT = os.environ.get("PLANFLOW_REPORT", "")


def test_switch_models_in_this_process():
    """the three models under the switch set of THIS process (the parent: the defaults; a child: one switch at its other value)"""
    for key, (env, attr) in SWITCHES.items():
        want = key != HERE
        assert (os.environ.get(env, "1") != "0") == want, env
        if attr is not None:
            assert getattr(graph, attr) is want, attr
    for m in SWITCH_MODELS:
        for d in ("bf16", "fp32"):
            row, bad = _row((m, d, "train"))
            assert not bad, "\n".join(bad)
            if REPORT:
                with open(REPORT, "a") as f:
                    f.write(json.dumps(dict(row, model=m, dtype=d, kind="train", switch=HERE)) + "\n")


_CHILD_ROWS = []


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_plans_are_clean_under_switch(switch):
    fd, path = tempfile.mkstemp(suffix=".jsonl")
    os.close(fd)
    try:
        env = dict(os.environ, PLANFLOW_SWITCH=switch, PLANFLOW_REPORT=path, **{SWITCHES[switch][0]: "0"})
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-p", "no:cacheprovider",
                            "-k", "test_switch_models_in_this_process"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        with open(path) as f:
            rows = [json.loads(line) for line in f if line.strip()]
    finally:
        os.unlink(path)
    assert len(rows) == 2 * len(SWITCH_MODELS) and all(r["violations"] == 0 and r["switch"] == switch for r in rows)
    # the switch changed at least one of the plans (else the child checked what the parent had checked already)
    assert any(r["digest"] != _row((r["model"], r["dtype"], "train"))[0]["digest"] or
               r["bytes"] != _row((r["model"], r["dtype"], "train"))[0]["bytes"] for r in rows), switch
    _CHILD_ROWS.extend(rows)


def test_report_every_plan_has_zero_violations():
    rows = [dict(_row(c)[0], model=c[0], dtype=c[1], kind=c[2], switch="") for c in CASES] + _CHILD_ROWS
    print("\n%-20s %-5s %-8s %-15s %9s %6s %6s %8s %13s %10s" % ("model", "dtype", "kind", "switch=0", "launches", "side", "forks", "buckets", "bytes", "violations"))
    for r in rows:
        print("%-20s %-5s %-8s %-15s %9d %6d %6d %8d %13d %10d" % (r["model"], r["dtype"], r["kind"], r["switch"], r["launches"], r["side"],
                                                                 r["forks"], r["buckets"], r["bytes"], r["violations"]))
    assert len(rows) >= len(CASES) and all(r["violations"] == 0 for r in rows)
