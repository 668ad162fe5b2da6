"""bench.py's plain run, its --full extras and --dump-outputs.
  * CPU: dump_outputs writes float32 .npy files, whole logits up to the sample size, the same seeded parameter / gradient sample
    in every call, under 64 MB at the headline shape; the per-kernel table is refused without --full;
  * -m gpu: a plain run and a --full run with the same arguments print the headline keys, only the --full line carries the extras,
    and both dump the same outputs (the inputs are seeded, and --full measures only after the dump)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_float32_fixed_sample_and_bounded(tmp_path):
    bench = _bench()
    n = bench.DUMP_SAMPLE + 5
    params = [torch.nn.Parameter(torch.arange(n, dtype=torch.float32)), torch.nn.Parameter(torch.full((7,), float(n)))]
    params[0].grad = -params[0].detach()                                 # params[1] has no gradient: dumped as zeros
    logits = torch.randn(32, 1, 256, 256, generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(0.25), logits, params)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(a) == {"loss", "logits", "params_sample", "grads_sample"}
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].tolist() == [0.25] and np.array_equal(a["logits"], logits.numpy())
    ps, gs = a["params_sample"], a["grads_sample"]
    assert ps.shape == gs.shape == (bench.DUMP_SAMPLE,) and len(np.unique(ps)) > bench.DUMP_SAMPLE // 2
    # parameter i of the flattened list holds the value i (the 7 of params[1] hold n): the gradient sample is taken at the same places
    assert np.array_equal(gs, np.where(ps < n, -ps, 0))
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "b" / f), a[f[:-4]]), f


def test_kernel_table_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--kernel-table"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and r.stdout.strip() == "" and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--size", "64"]
    lines, dumps = {}, {}
    for mode, extra in (("plain", []), ("full", ["--full", "--kernel-table"])):
        d = tmp_path / mode
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra + ["--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines[mode] = json.loads(out[0])
        dumps[mode] = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    for mode, res in lines.items():
        assert all(k in res for k in HEADLINE) and res["steps"] == 3 and res["ms_per_step"] > 0, res
        assert res["unit"] == "images/s" and res["dtype"] == "bf16" and res["higher_is_better"] is True
    assert not {"roofline", "cpu_baseline"} & set(lines["plain"]) and "host_issue_ms_per_step" not in lines["plain"]["config"]
    assert {"roofline", "cpu_baseline"} <= set(lines["full"]) and "host_issue_ms_per_step" in lines["full"]["config"]
    p, f = dumps["plain"], dumps["full"]
    assert set(p) == set(f) == {"loss", "logits", "params_sample", "grads_sample"}
    assert p["logits"].shape == (4, 1, 64, 64) and all(np.isfinite(v).all() for v in p.values())
    assert abs(float(p["loss"][0]) - lines["plain"]["config"]["final_loss"]) <= 1e-5
    for k in p:
        scale = float(np.abs(p[k]).max()) or 1.0
        assert float(np.abs(p[k] - f[k]).max()) <= 1e-3 * scale, k
