"""-m gpu: ``train(model, WithAveraging(train_dl, ...), ...)`` under data parallelism, world_size 2 (both ranks on the box's one GPU over
gloo, the harness of tests/test_gpu_dp_train.py).  BatchNorm statistics are per GPU, so the averaged ones differ between the ranks
until ``train()`` syncs them inside ``swap()``: every rank must validate ONE averaged model, the one rank 0 saves.
  * after train() both ranks hold bit-identical averaged parameters AND averaged buffers;
  * the printed EMA / SWA line is the validation loss of the checkpoint rank 0 wrote, recomputed in one process over the whole
    validation set: to half a unit of the last printed digit plus 1e-4 for the other order of the fp32 sums over the batches;
  * rank 1 prints nothing and only rank 0 writes."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_dp_train import DEV, EPOCHS, LR, _free_port, _loaders, _model, _paths

pytestmark = pytest.mark.gpu
SPECS = {"ema": {"mode": "ema", "decay": 0.9, "warmup": 2}, "swa": {"mode": "swa", "swa_start": 1}}


def _avg_worker(rank, world, port, save_dir, mode, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    _paths()
    m = _model()                                           # imports the package before the first CUDA call
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mi355 import averaging
        from utils.helpers import train
        made, init = [], averaging.WeightAverage.__init__

        def recording_init(self, *a, **kw):                # keep the WeightAverage train() builds from the dict (the trainer's path)
            init(self, *a, **kw)
            made.append(self)
        averaging.WeightAverage.__init__ = recording_init
        if rank == 1:                                      # a rank-dependent start: the average must begin from rank 0's state too
            with torch.no_grad():
                for p in m.parameters():
                    p.mul_(1.5)
        tr, va = _loaders()
        buf = io.StringIO()
        with redirect_stdout(buf):
            train(m, averaging.WithAveraging(tr, dict(SPECS[mode])), va, DEV, EPOCHS, LR, "AttentionUNet", save_dir, seg=True)
        torch.cuda.synchronize()
        assert len(made) == 1
        sd = made[0].state_dict()
        flat = {**{"p." + k: v.cpu().numpy() for k, v in sd["params"].items()}, **{"b." + k: v.cpu().numpy() for k, v in sd["buffers"].items()}}
        q.put((rank, "ok", sd["count"], buf.getvalue(), flat))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "fail", traceback.format_exc(), "", None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_train_world2_validates_and_saves_one_averaged_model(mode, tmp_path):
    from mi355 import nn as mnn
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    save_dir = str(tmp_path / "w")
    procs = [ctx.Process(target=_avg_worker, args=(r, 2, port, save_dir, mode, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for rank, status, info, _, _ in res:
        assert status == "ok", f"rank {rank}: {info}"
    (_, _, n0, log0, sd0), (_, _, n1, log1, sd1) = res
    assert n0 == n1 == (3 * EPOCHS if mode == "ema" else EPOCHS)                      # 3 optimiser steps per epoch and rank
    assert set(sd0) == set(sd1) and all(np.array_equal(sd0[k], sd1[k]) and sd0[k].dtype == sd1[k].dtype for k in sd0)
    assert any(k.endswith("running_var") for k in sd0) and log1 == ""
    fname = "AttentionUNet_ema_best_loss.pt" if mode == "ema" else "AttentionUNet_swa.pt"
    assert sorted(os.listdir(save_dir)) == sorted(["AttentionUNet_best_loss.pt", fname])
    if mode == "ema":
        lines = re.findall(r"^\[AttentionUNet\] Ep(\d+): EMA ValLoss ([\d.]+) \| IoU [\d.]+$", log0, flags=re.M)
        assert [e for e, _ in lines] == [str(e) for e in range(1, EPOCHS + 1)]
        printed = min(lines, key=lambda l: (float(l[1]), int(l[0])))[1]
    else:
        lines = re.findall(rf"^\[AttentionUNet\] SWA \({EPOCHS} epochs\): ValLoss ([\d.]+) \| IoU [\d.]+$", log0, flags=re.M)
        assert len(lines) == 1
        printed = lines[0]
    m = _model()
    m.load_state_dict(torch.load(os.path.join(save_dir, fname), map_location="cpu"))
    m = m.to(DEV).eval()
    _, va = _loaders()
    crit, tot = mnn.BCEWithLogitsLoss(), 0.0
    with torch.no_grad():
        for x, y in va:
            out = m(x.to(DEV))
            tot += float(crit(out if out.dim() == 4 else out.unsqueeze(1), y.to(DEV))) * x.size(0)
    got = tot / len(va.dataset)
    print(f"{mode}: printed {printed}, the saved checkpoint validates at {got:.6f}")
    assert abs(float(printed) - got) <= 5e-4 + 1e-4
