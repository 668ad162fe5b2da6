"""Weight averaging along the optimiser trajectory: EMA (Mean Teacher; timm's ModelEmaV2 with its decay warm-up) and the
equal-weight average of SWA (Izmailov et al. 2018), with a BatchNorm re-estimation for the latter.  Nothing in the reference.

The engine keeps every parameter in one flat fp32 buffer, so an update is ONE streaming launch (csrc/weight_avg.hip,
mi355_avg_update) plus one table launch for the BatchNorm running statistics; the update count and the skip decision of a loss
scaler live in device memory like AdamW's, so ``update()`` never waits for the host, allocates nothing and can be captured.

    avg = WeightAverage(model, mode="ema", decay=0.999)
    ... scaler.step(optimizer); avg.update(optimizer) ...
    with avg.swap():                      # the model IS the averaged model in here (same plans, same launches)
        validate(model)
    torch.save(avg.averaged_state_dict(), path)      # loads into a fresh model

    train(model, WithAveraging(train_dl, {"mode": "ema", "decay": 0.999}), val_dl, ...)      # utils/helpers.py does all of that

There is no torch fall-back: the model must be a mi355 Net on the GPU."""
from __future__ import annotations

import contextlib
from collections import OrderedDict

import torch
from torch.nn.modules.batchnorm import _BatchNorm

from .lib import lib

MODES = {"ema": 0, "swa": 1}


def _table(rows, device):
    """rows of three integers -> the int64 device table the *_table launchers read"""
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(device)


class WithAveraging:
    """``train(model, WithAveraging(train_dl, averaging), val_dl, ...)``: how utils/helpers.py::train is told to keep an average of
    the weights — like ``utils.mix.MixedBatches`` a wrapper of the training loader, because ``train()`` keeps the reference's
    parameter list.  ``averaging``: None (off), a dict ``{"mode": "ema" | "swa", "decay", "warmup", "buffers", "swa_start"}`` or a
    ``WeightAverage`` of the model.  ``loader`` may itself be a ``MixedBatches``."""

    def __init__(self, loader, averaging):
        self.loader, self.averaging = loader, averaging

    def __iter__(self):
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)


class WeightAverage:
    """``mode``: "ema" (avg += (1 - d) (p - avg), d = min(decay, (1 + t) / (warmup + t)); ``warmup`` <= 0: d = decay) or "swa"
    (the equal-weight mean of the iterates ``update()`` was called on).  ``buffers``: keep an averaged copy of the float buffers
    (BatchNorm running statistics) as well — averaged with the same coefficient in EMA mode, exchanged as they are in SWA mode,
    where ``update_bn`` re-estimates them inside ``swap()``; False: the averaged weights run with the live buffers."""

    def __init__(self, model, mode="ema", decay=0.999, warmup=10, buffers=True):
        if mode not in MODES:
            raise ValueError(f"WeightAverage: mode must be 'ema' or 'swa' (got {mode!r})")
        if not 0.0 <= float(decay) <= 1.0 or float(warmup) < 0:
            raise ValueError(f"WeightAverage: decay {decay} outside [0, 1] or warmup {warmup} < 0")
        if not hasattr(model, "engine"):
            raise TypeError("WeightAverage needs a mi355 Net (flat parameter storage); there is no torch fallback on this path")
        self.model, self.mode, self.decay, self.warmup, self.buffers = model, mode, float(decay), float(warmup), bool(buffers)
        eng = model.engine
        eng._check_storage()
        if eng.flat_p is None or eng.flat_p.device.type != "cuda":
            raise RuntimeError("WeightAverage: move the model to the GPU first (model.to(device))")
        self.flat = eng.flat_p.clone()
        self.count = torch.zeros(1, dtype=torch.int32, device=self.flat.device)
        named = list(model.named_buffers()) if self.buffers else []
        self._fbuf = OrderedDict((n, b.detach().clone()) for n, b in named if b.is_floating_point())
        self._ibuf = OrderedDict((n, b.detach().clone()) for n, b in named if not b.is_floating_point())
        for n, b in self._fbuf.items():
            if b.dtype != torch.float32 or not b.is_contiguous():
                raise RuntimeError(f"WeightAverage: buffer {n} is not contiguous fp32")
        self._built_for = None
        self._sync_tables()

    # ---- device pointer tables ------------------------------------------------------------------------------------------
    def _live_buffers(self):
        live = dict(self.model.named_buffers())
        return [live[n] for n in self._fbuf], [live[n] for n in self._ibuf]

    def _probe_key(self):
        """where the flat buffer and the first and the last float buffer live NOW: the buffers are looked up in their modules'
        ``_buffers`` (two dictionary reads, not a walk over the model), so one that was replaced there is seen"""
        return (self.model.engine.flat_p.data_ptr(),) + tuple(mod._buffers[key].data_ptr() for mod, key in self._probe_at)

    def _sync_tables(self):
        """(Re)build the pointer tables when the engine re-flattened or the buffers were re-created: ``.to()`` / ``Module._apply``
        replace every buffer, which the first and the last one show.  A single buffer in the middle re-registered on its own is
        NOT detected (checking all of them would walk about a hundred tensors per step): build a new WeightAverage after that."""
        eng = self.model.engine
        eng._check_storage()
        if self._built_for is not None and self._probe_key() == self._built_for:
            return
        if eng.flat_p.numel() != self.flat.numel():
            raise RuntimeError("WeightAverage: the model's flat parameter buffer changed its layout")
        dev = eng.flat_p.device
        if self.flat.device != dev:
            self.flat, self.count = self.flat.to(dev), self.count.to(dev)
            self._fbuf = OrderedDict((n, b.to(dev)) for n, b in self._fbuf.items())
            self._ibuf = OrderedDict((n, b.to(dev)) for n, b in self._ibuf.items())
        fl, il = self._live_buffers()
        for b in fl:
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != dev:
                raise RuntimeError("WeightAverage: a live buffer is not contiguous fp32 on the model's device")
        rows = [(a.data_ptr(), b.data_ptr(), b.numel()) for a, b in zip(self._fbuf.values(), fl) if b.numel()]
        self._live_f, self._live_i = fl, il
        self._n_buf_rows = len(rows)
        self._tab_update = _table(rows, dev) if rows else None                                   # {avg, live, n}
        self._tab_swap = _table([(eng.flat_p.data_ptr(), self.flat.data_ptr(), self.flat.numel())] + [(b, a, n) for a, b, n in rows], dev)
        owners = {}
        for mname, mod in self.model.named_modules():
            for key in mod._buffers:
                owners.setdefault((mname + "." if mname else "") + key, (mod, key))
        names = list(self._fbuf)
        self._probe_at = [owners[n] for n in (names[0], names[-1])] if names else []
        self._built_for = self._probe_key()

    # ---- the per-step update ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, optimizer=None):
        """Fold the live weights into the average.  ``optimizer``: the mi355.optim.AdamW that has just stepped — when a loss
        scaler made it skip the step (inf / nan gradients), the average skips it too and does not count it."""
        self._sync_tables()
        finf = None
        if optimizer is not None:
            for st in getattr(optimizer, "_st", ()):
                f = st.get("finf")
                if f is not None:
                    finf = f
        mode = MODES[self.mode]
        lib.mi355_step_tick(self.count, finf)
        lib.mi355_avg_update(self.flat, self.model.engine.flat_p, self.flat.numel(), mode, self.decay, self.warmup, self.count, finf)
        if self.mode == "ema" and self._tab_update is not None:
            lib.mi355_avg_update_table(self._tab_update, self._n_buf_rows, mode, self.decay, self.warmup, self.count, finf)

    # ---- exchange with the live model ---------------------------------------------------------------------------------------
    def _exchange(self):
        self._sync_tables()
        lib.mi355_swap_table(self._tab_swap, 1 + self._n_buf_rows)
        # the int64 num_batches_tracked counters are exchanged here with torch, not by the kernel (which moves fp32 words): there
        # are few of them, they are eight bytes each, and nothing on the hot path reads them
        for mine, live in zip(self._ibuf.values(), self._live_i):
            tmp = live.clone()
            live.copy_(mine)
            mine.copy_(tmp)
        self.model.engine.invalidate_packs()          # eval plans cache their packed bf16 weights by pack_epoch

    @contextlib.contextmanager
    def swap(self):
        """Inside the block the model holds the averaged parameters (and buffers) and this object holds the live ones: an in-place
        exchange, so every plan, pointer and optimiser view stays valid.  On exit every live byte is what it was, and what the
        block wrote into the model (``update_bn``) belongs to the average."""
        with torch.no_grad():
            if self.mode == "ema":                    # the averaged statistics have seen what the live ones have
                for mine, live in zip(self._ibuf.values(), self._live_buffers()[1]):
                    mine.copy_(live)
            self._exchange()
        try:
            yield self.model
        finally:
            with torch.no_grad():
                self._exchange()

    # ---- checkpoints ------------------------------------------------------------------------------------------------------
    def _param_views(self):
        eng = self.model.engine
        out = OrderedDict()
        for name, p in self.model.named_parameters():
            o, n = eng.offsets[id(p)]
            out[name] = self.flat[o:o + n].view(p.shape)
        return out

    def state_dict(self):
        """The averaged tensors by parameter / buffer name, the update count, the mode and its constants."""
        return {"mode": self.mode, "decay": self.decay, "warmup": self.warmup, "count": int(self.count.item()),
                "params": OrderedDict((k, v.clone()) for k, v in self._param_views().items()),
                "buffers": OrderedDict((k, v.clone()) for k, v in list(self._fbuf.items()) + list(self._ibuf.items()))}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if sd["mode"] != self.mode:
            raise ValueError(f"WeightAverage: the checkpoint averages in mode {sd['mode']!r}, this object in {self.mode!r}")
        views, bufs = self._param_views(), {**self._fbuf, **self._ibuf}
        if set(sd["params"]) != set(views) or set(sd["buffers"]) != set(bufs):
            raise ValueError("WeightAverage: the checkpoint names other parameters / buffers than the model")
        self.decay, self.warmup = float(sd["decay"]), float(sd["warmup"])
        self.count.fill_(int(sd["count"]))
        for k, v in views.items():
            v.copy_(sd["params"][k])
        for k, v in bufs.items():
            v.copy_(sd["buffers"][k])

    def averaged_state_dict(self):
        """A checkpoint of the averaged model in the model's own ``state_dict`` format (loads into a fresh model).  Buffers this
        object does not average (``buffers=False``) are the live ones."""
        mine = {**self._param_views(), **self._fbuf, **self._ibuf}
        live_i = dict(zip(self._ibuf, self._live_buffers()[1])) if self.mode == "ema" else {}
        out = OrderedDict()
        for k, v in self.model.state_dict().items():
            src = live_i.get(k, mine.get(k, v))
            out[k] = src.detach().clone()
        return out


@torch.no_grad()
def update_bn(model, loader, device, max_batches=None):
    """Re-estimate every BatchNorm's running statistics under the model's CURRENT weights (after ``WeightAverage.swap()`` for
    SWA; on films from another scanner for AdaBN-style adaptation).

    running_mean, running_var and num_batches_tracked are reset to 0, the loader runs through the model in train mode without
    gradients (the engine's own train-mode plans: their BatchNorm launches accumulate r = (1 - m) r + m b with the momentum m the
    plan bakes in), and one mi355_bn_debias_table launch divides by 1 - (1 - m)^k, k being the device's own
    num_batches_tracked — exact however often a block fires one BatchNorm per forward (the recurrent R2 blocks).  The result is

        sum_j w_j b_j,   w_j = m (1 - m)^(k - 1 - j) / (1 - (1 - m)^k)      (weights sum to 1, the last batch weighs most)

    the bias-corrected exponentially weighted mean of the batch statistics.  ``torch.optim.swa_utils.update_bn`` weights the
    batches EQUALLY instead (momentum = None, a cumulative average): that needs a momentum of 1 / num_batches_tracked read and
    counted inside the BatchNorm launch itself, which the engine's launches (one constant momentum per plan) do not take.  With
    m = 0.1 the last ~20 batches carry 88 % of the weight; shuffle the loader as for training.

    Returns the number of batches that ran.  The model's train / eval mode is restored."""
    bns = [m for m in model.modules() if isinstance(m, _BatchNorm) and m.track_running_stats]
    if not bns:
        return 0
    device = torch.device(device)
    for bn in bns:
        bn.running_mean.zero_()
        bn.running_var.zero_()
        bn.num_batches_tracked.zero_()
    was_training = model.training
    model.train()
    ran = 0
    try:
        for batch in loader:
            if max_batches is not None and ran >= max_batches:
                break
            x = batch[0] if isinstance(batch, (tuple, list)) else batch
            model(x.to(device, non_blocking=True))
            ran += 1
    finally:
        model.train(was_training)
    by_momentum = {}
    for bn in bns:                                    # (None: the engine's plans run such a BatchNorm with 0.1 too)
        by_momentum.setdefault(float(bn.momentum if bn.momentum is not None else 0.1), []).append(bn)
    for mom, group in by_momentum.items():            # one launch: every BatchNorm of these models shares one momentum
        rows = [(r.data_ptr(), bn.num_batches_tracked.data_ptr(), r.numel()) for bn in group for r in (bn.running_mean, bn.running_var)]
        lib.mi355_bn_debias_table(_table(rows, device), len(rows), mom)
    if hasattr(model, "engine"):
        model.engine.invalidate_packs()               # eval plans that fold BatchNorm into frozen packs see the new statistics
    return ran
