"""CPU: scripts/plan_dump.py, the canonical text form of a launch plan (nothing is launched): two independent builds of a
configuration dump identically, every plan entry is a real Launch of the right arity, and Launch.arg(name) finds the slot the C
prototype gives that name."""
import os
import sys

import pytest
import torch

from mi355 import graph
from mi355.lib import lib, available

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import plan_dump  # noqa: E402

pytestmark = pytest.mark.skipif(not available(), reason="libmi355conv.so not built")


@pytest.mark.parametrize("name,shape", [("AttentionUNet", (2, 3, 64, 64)), ("R2AttU_Net", (1, 3, 32, 32))])
def test_plan_dump(name, shape):
    (net, plan), (net2, plan2) = (plan_dump.build_plan(name, shape, "bf16", "train") for _ in range(2))
    assert net is not net2 and plan is not plan2
    text = plan_dump.dump_plan(net, plan)
    assert text == plan_dump.dump_plan(net2, plan2)
    launches = plan.pre + plan.fwd + plan.bwd
    assert text.count("\n") > len(launches) > 100 and all(type(l) is graph.Launch for l in launches)      # no placeholder survives finish()
    fwd, bwd = plan.bind(0)                     # resolves every pointer and checks ABI arity; launches nothing
    assert len(fwd) + len(bwd) == len(launches)
    for l in launches:
        names = [n for _, n in lib.protos[l.name][1]][:-1]      # (the last parameter is the stream, bound later)
        assert len(names) == len(l.args) == len(set(names)), l.name
        for i, n in enumerate(names):
            assert l.arg(n) is l.args[i], (l.name, n)
