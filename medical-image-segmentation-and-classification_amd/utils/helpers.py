"""Training driver and factories of the MI355X path — same public names, signatures and
printed lines as the reference's utils/helpers.py (acc/iou :219-227, factories :124-213,
train :231-412), executing on the HIP launch-plan engine.

Differences that do not change results: the compute dtype is a property of the model (bf16 default, fp32,
or fp16 with the device-side ``mi355.amp.GradScaler`` in the place of ``torch.amp.GradScaler``,
helpers.py:285,323-336) instead of autocast, the per-step ``loss.item()`` host syncs (helpers.py:337,341) are replaced
by device-side accumulation read back once per epoch, and model factories construct the local
classes directly (the reference first tries a torch.hub download, helpers.py:158-166, which has
no network here).

Additions the reference does not have, all off by default: ``criterion=`` (a loss module of ``mi355.nn`` for the training and the
validation loss) and a ``utils.mix.MixedBatches(train_dl, batch_mix)`` in the place of ``train_dl`` (the parameter list stays the
reference's plus ``criterion``): mixup / CutMix of every training batch on the device by that ``utils.mix.BatchMix``; classifiers then
train against a ``MixedTarget`` with ``mi355.nn.MixCrossEntropyLoss``, validation stays on hard labels and unmixed batches.
A ``mi355.averaging.WithAveraging(train_dl, averaging)`` in the place of ``train_dl`` (outside a ``MixedBatches``, if both are used;
the parameter list stays as it is here too), ``averaging`` a dict such as ``{"mode": "ema", "decay": 0.999, "warmup": 10}`` or
``{"mode": "swa", "swa_start": E}``, or a ``mi355.averaging.WeightAverage``: an average of the weights along the trajectory, validated
and saved beside the raw model (``{name}_ema_best_loss.pt`` / ``{name}_ema_best_acc.pt``, ``{name}_swa.pt``); the raw model's lines,
schedule and files do not change.
A ``utils.distill.Distilled(train_dl, teacher)`` in the place of ``train_dl`` (inside a ``WithAveraging``, outside a ``MixedBatches``):
knowledge distillation — the frozen teacher's eval forward on every training batch, the target a ``DistillTarget`` for
``mi355.nn.SegDistillationLoss`` / ``DistillCrossEntropyLoss``, one more line per epoch (``Distill hard … | KD …``); validation stays
on the hard target alone.

Data parallel: when ``torch.distributed`` is initialised with more than one rank (``torchrun --nproc-per-node N
utils/trainer.py ...``), ``train()`` shards the loaders' batches by rank (utils/distributed.py), wraps the model in
``mi355.dp.DataParallel`` (bucketed RCCL all-reduce of the flat gradient buffer overlapped with backward, 1/world folded
into clip / AdamW), sums the epoch's loss / metric accumulators over ranks with one collective per pass, and lets rank 0
alone print and write checkpoints; every rank returns the same ``best_score`` and stops early at the same epoch."""
import math
import os
import time

import torch
import torch.nn as nn

from mi355 import amp as mamp
from mi355 import nn as mnn
from mi355 import optim as moptim
from mi355.lib import lib
from utils.distributed import RankShard, all_reduce_sums, dist_info

CLASSES = ["COVID", "Healthy", "Non-COVID"]


# ---- model factories ---------------------------------------------------------------------------
def add_dropout_to_fc(model, p=0.5, classes=CLASSES):
    """Swap the classification layer for Dropout(p) + Linear(in, len(classes)); returns the name of
    the head attribute ("fc" / "classifier") that stage 1 trains (helpers.py:124-144)."""
    n_out = len(classes)
    if hasattr(model, "fc"):
        model.fc = nn.Sequential(nn.Dropout(p=p), nn.Linear(model.fc.in_features, n_out))
        return "fc"
    head = getattr(model, "classifier", None)
    if isinstance(head, nn.Sequential):
        kept = list(head.children())
        last = kept.pop()
        model.classifier = nn.Sequential(*kept, nn.Dropout(p=p), nn.Linear(last.in_features, n_out))
        return "classifier"
    return None


def get_class_model(name, hub=None):
    """name -> (model, head attribute name); random init.  The reference first asks torch.hub for the torchvision
    model (`resnet18` / `resnet50`; `vgg16` -> `vgg16_bn`, helpers.py:158-166) and falls back to its local classes when
    that fails (:170-192).  There is no network here, so by default "vgg16" / "vgg19" / "resnet*" are the local classes
    (the reference's offline behaviour); ``hub=True`` (or MI355_HUB_LAYOUT=1) selects the torchvision layouts the online
    reference trains — `TorchvisionResNet.resnet18/50`, `VGG.VGG16_BN/VGG19_BN` — into which hub checkpoints load
    unchanged.  The hub layouts are also reachable by their own names "vgg16_bn" / "vgg19_bn" / "resnet18_tv" / "resnet50_tv"."""
    from models.classification_models import ResNet, TorchvisionResNet, VGG
    local = {"resnet18": ResNet.ResNet18, "resnet50": ResNet.ResNet50, "vgg16": VGG.VGG16, "vgg19": VGG.VGG19}
    tv = {"resnet18": TorchvisionResNet.resnet18, "resnet50": TorchvisionResNet.resnet50, "vgg16": VGG.VGG16_BN, "vgg19": VGG.VGG19_BN}
    named = {"vgg16_bn": VGG.VGG16_BN, "vgg19_bn": VGG.VGG19_BN, "resnet18_tv": TorchvisionResNet.resnet18,
             "resnet50_tv": TorchvisionResNet.resnet50}
    if hub is None:
        hub = os.environ.get("MI355_HUB_LAYOUT", "0") == "1"
    key = name.lower()
    table = {**(tv if hub else local), **named}
    if key not in table:
        raise ValueError(f"Unknown classification model: {name}")
    model = table[key](num_classes=1000)
    return model, add_dropout_to_fc(model, p=0.5)


def get_seg_model(name, classes=1):
    """name -> segmentation model instance (helpers.py:195-213).  ``classes`` > 1: a K-channel logit head for the multi-class
    path (mi355.nn.MultiClassSegLoss, utils/multiclass.py); 1 = the reference's single-foreground model, built as before."""
    key = name.lower()
    classes = int(classes)
    if classes < 1:
        raise ValueError(f"classes must be >= 1 (got {classes})")
    if key == "attentionunet":
        from models.segmentation_models.AttentionUNet import AttentionUNet
        return AttentionUNet() if classes == 1 else AttentionUNet(out_channel=classes)
    if key == "r2unet":
        from models.segmentation_models.R2U_Net import R2U_Net
        return R2U_Net() if classes == 1 else R2U_Net(out_channels=classes)
    if key == "r2attunet":
        from models.segmentation_models.R2AttU_Net import R2AttU_Net
        return R2AttU_Net() if classes == 1 else R2AttU_Net(out_channels=classes)
    if key == "resnetunet":
        from models.segmentation_models.ResnetUnet import ResNetUnet
        return ResNetUnet() if classes == 1 else ResNetUnet(n_classes=classes)
    raise ValueError(f"Unknown segmentation model: {name}")


# ---- metrics --------------------------------------------------------------------------------------
def acc(logits, y):
    return (torch.argmax(logits, 1) == y).sum().item(), y.size(0)


def _iou_device(pred, mask, t=0.5, is_logit=False):
    """Whole-batch IoU of helpers.py:223-227 as a 0-dim device tensor (no sync)."""
    cnt = torch.empty(4, dtype=torch.float32, device=pred.device)
    lib.mi355_seg_counts(pred.contiguous(), mask.contiguous(), cnt, 1, pred.numel(), 1 if is_logit else 0, float(t))
    inter, union = cnt[0], cnt[1] + cnt[2] - cnt[0]
    return inter / (union + 1e-7)


def iou(pred, mask, t=0.5):
    if pred.is_cuda:
        return _iou_device(pred.float(), mask.float(), t).item()
    p = (pred > t).float()
    inter = (p * mask).sum()
    union = ((p + mask) > 0).float().sum()
    return (inter / (union + 1e-7)).item()


# ---- training ----------------------------------------------------------------------------------------
def _make_optimizer(params, lr):
    return moptim.AdamW(params, lr=lr, weight_decay=5e-4)


def _averaging_spec(averaging, epochs):
    """WithAveraging(train_dl, averaging).averaging -> (WeightAverage or its constructor arguments, mode, first SWA epoch); validated before any work"""
    from mi355.averaging import WeightAverage
    if isinstance(averaging, WeightAverage):
        return averaging, averaging.mode, max(1, int(math.ceil(0.75 * epochs)))
    if not isinstance(averaging, dict):
        raise TypeError(f"averaging must be None, a dict or a mi355.averaging.WeightAverage (got {type(averaging).__name__})")
    spec = dict(averaging)
    mode = spec.setdefault("mode", "ema")
    swa_start = spec.pop("swa_start", None)
    unknown = set(spec) - {"mode", "decay", "warmup", "buffers"}
    if unknown or mode not in ("ema", "swa"):
        raise ValueError(f"averaging: mode 'ema' or 'swa' with decay / warmup / buffers / swa_start (got {averaging})")
    if swa_start is None:
        swa_start = max(1, int(math.ceil(0.75 * epochs)))          # an epoch, 1-based: the last quarter of the run
    if mode == "swa" and not 1 <= int(swa_start) <= epochs:
        raise ValueError(f"averaging: swa_start {swa_start} outside the epochs 1..{epochs}")
    return spec, mode, int(swa_start)


def train(model, train_dl, val_dl, device, epochs, lr, name, save_dir, seg=False, cls_head_name=None, criterion=None):
    # a utils.distill.Distilled among the wrappers of train_dl: its teacher runs in eval mode and gets its previous mode back, however
    # the run ends
    teacher, dl = None, train_dl
    while dl is not None and teacher is None:
        teacher, dl = getattr(dl, "teacher", None), getattr(dl, "loader", None)
    was_training = bool(getattr(teacher, "training", False))
    try:
        return _train(model, train_dl, val_dl, device, epochs, lr, name, save_dir, seg, cls_head_name, criterion)
    finally:
        if was_training:
            teacher.train()


def _train(model, train_dl, val_dl, device, epochs, lr, name, save_dir, seg, cls_head_name, criterion):
    device = torch.device(device)
    # train_dl may be a mi355.averaging.WithAveraging(loader, averaging): the loader is used as it would be without the wrapper and
    # an average of the weights is kept beside the raw model (below); a plain loader = today's loop
    averaging = None
    if hasattr(train_dl, "averaging"):
        train_dl, averaging = train_dl.loader, train_dl.averaging
        if averaging is not None:
            averaging, avg_mode, swa_start = _averaging_spec(averaging, epochs)
    # train_dl may be a utils.distill.Distilled(loader, teacher): the loader is used as it would be without the wrapper and every
    # TRAINING batch's target becomes a DistillTarget(y, teacher's logits on x); a plain loader = today's loop
    teacher = None
    if hasattr(train_dl, "teacher"):
        train_dl, teacher = train_dl.loader, train_dl.teacher
    _ORDER = "WithAveraging(Distilled(MixedBatches(loader, batch_mix), teacher), averaging)"
    if teacher is not None and hasattr(train_dl, "averaging"):
        raise TypeError(f"WithAveraging goes OUTSIDE Distilled: train(model, {_ORDER}, ...)")
    if hasattr(train_dl, "batch_mix") and hasattr(train_dl.loader, "teacher"):
        raise TypeError(f"Distilled goes OUTSIDE MixedBatches (the teacher sees the mixed batch): train(model, {_ORDER}, ...)")
    model = model.to(device)
    if hasattr(model, "engine"):
        model.engine._check_storage()                 # flat fp32 parameter / gradient buffers
    # criterion: a loss module of mi355.nn (mnn.DiceLoss(), mnn.CombinedLoss(), ...) for the training AND the validation loss;
    # None = the reference's choice
    # train_dl may be a utils.mix.MixedBatches(loader, batch_mix): the loader is used as it would be without the wrapper and the
    # utils.mix.BatchMix (mixup / CutMix) is applied to every TRAINING batch on the device; a plain loader = today's loop
    batch_mix = None
    if hasattr(train_dl, "batch_mix"):
        train_dl, batch_mix = train_dl.loader, train_dl.batch_mix
    if hasattr(train_dl, "averaging"):
        raise TypeError("WithAveraging goes OUTSIDE MixedBatches: train(model, WithAveraging(MixedBatches(loader, batch_mix), averaging), ...)")
    if teacher is not None:
        if batch_mix is not None and not seg:
            raise ValueError("Distilled next to a classifier batch_mix: distillation on a MixedTarget (mixup / CutMix labels) is not built; "
                             "use one of the two")
        if criterion is None:
            criterion = mnn.SegDistillationLoss(1.0, 0.0) if seg else mnn.DistillCrossEntropyLoss(label_smoothing=0.1)
        elif not getattr(criterion, "accepts_distill_target", False):
            raise TypeError(f"Distilled turns the target into a DistillTarget, which {type(criterion).__name__} cannot take: use "
                            f"mi355.nn.{'SegDistillationLoss' if seg else 'DistillCrossEntropyLoss'}")
    if batch_mix is not None:
        if bool(getattr(batch_mix, "seg", seg)) != bool(seg):
            raise ValueError(f"batch_mix was built with seg={batch_mix.seg} but train() runs with seg={seg}")
        if not seg:
            if criterion is None:
                criterion = mnn.MixCrossEntropyLoss(label_smoothing=0.1)
            elif not getattr(criterion, "accepts_mixed_target", False):
                raise TypeError(f"batch_mix turns the labels into a MixedTarget, which {type(criterion).__name__} cannot take: "
                                "use mi355.nn.MixCrossEntropyLoss")
    if criterion is None:
        criterion = mnn.BCEWithLogitsLoss() if seg else mnn.CrossEntropyLoss(label_smoothing=0.1)
    STAGE1 = 5

    # data parallel (module docstring): the reference's loop on this rank's batches, gradients averaged over ranks
    rank, world = dist_info()
    dp, inv_scale = None, 1.0
    say = print if rank == 0 else (lambda *a, **k: None)
    n_train, n_val, n_val_batches = len(train_dl.dataset), len(val_dl.dataset), len(val_dl)
    if world > 1:
        from mi355.dp import DataParallel
        dp = DataParallel(model)                      # replicas start from rank 0's parameters and buffers
        inv_scale = dp.inv_scale
        train_dl, val_dl = RankShard(train_dl, rank, world, pad=True), RankShard(val_dl, rank, world, pad=False)

    def make_optimizer(params, lr_):
        opt = _make_optimizer(params, lr_)
        opt.inv_scale = inv_scale                     # gradient averaging over ranks is folded into clip + AdamW
        return opt

    if seg:
        optimizer = make_optimizer(model.parameters(), lr)
        say(f"Training Segmentation model (all layers unfrozen) with LR: {lr}")
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=epochs)
    else:
        say(f"--- STAGE 1: Feature Extraction (Epochs 1-{STAGE1}) ---")
        for p in model.parameters():
            p.requires_grad = False
        head_params = []
        if cls_head_name:
            for p in getattr(model, cls_head_name).parameters():
                p.requires_grad = True
                head_params.append(p)
        optimizer = make_optimizer(head_params, 1e-4)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=STAGE1)

    # helpers.py:285 — scaling is enabled exactly where the reference's autocast would compute in fp16
    from mi355 import engine as _engine
    scaler = mamp.GradScaler(enabled=(getattr(model, "compute_dtype", None) or _engine._DEFAULT_DTYPE) == torch.float16)
    best_score = float("inf") if seg else 0.0
    patience, stale = 10, 0
    t0 = time.time()

    # averaging (None = off): an EMA of the weights updated after every optimiser step, or the equal-weight SWA average of the
    # epoch ends from swa_start on (mi355/averaging.py).  The raw model is trained, validated, logged, scheduled and saved exactly
    # as without it; the averaged model gets one more validation pass and files of its own.  It is created behind the
    # data-parallel wrapper, so that every rank averages the PARAMETERS of the replica it shares with rank 0 (the averaged buffers
    # are per rank between validations: validate_averaged syncs them).
    avg = None
    if averaging is not None:
        from mi355.averaging import WeightAverage, update_bn
        avg = averaging if isinstance(averaging, WeightAverage) else WeightAverage(model, **averaging)
        avg_best = float("inf") if seg else 0.0

    # distillation (None = off): the frozen teacher runs forward only, in eval mode for the whole run (its previous mode is put back
    # at the end); data parallel: every rank runs its own replica, nothing of it is communicated
    if teacher is not None:
        from utils.distill import DistillTarget, teacher_logits
        if getattr(teacher, "training", False):
            teacher.eval()

    def validate():
        """one pass over val_dl in eval mode -> (loss sum, metric sum) on the device"""
        model.eval()
        vloss = torch.zeros((), device=device)
        vmetric = torch.zeros((), device=device)
        with torch.no_grad():
            for x, y in val_dl:
                x, y = x.to(device), y.to(device)
                out = model(x)
                if seg and out.dim() == 3:
                    out = out.unsqueeze(1)
                vloss += criterion(out, y) * x.size(0)
                if seg and hasattr(criterion, "val_metric"):
                    vmetric += criterion.val_metric(out, y)      # multi-class criteria: mean IoU from the confusion matrix
                elif seg:
                    vmetric += _iou_device(out.float(), y.float(), 0.5, is_logit=True)
                else:
                    vmetric += (torch.argmax(out, 1) == y).sum()
        return vloss, vmetric

    def validate_averaged(refresh_bn):
        """validate() of the averaged model, inside swap() -> (val loss, metric as printed, its state_dict on rank 0).  The host
        random state is put back afterwards: a DataLoader draws its base seed from it whenever it is iterated, and the next
        epoch's shuffle must be the one a run without averaging sees."""
        rng = torch.get_rng_state()
        with avg.swap():
            if refresh_bn:
                update_bn(model, train_dl, device)               # the plain training loader: no batch_mix
            if dp is not None:
                # BatchNorm statistics are per GPU: the averaged ones were folded from (EMA) or re-estimated on (SWA: train_dl is
                # this rank's shard) each rank's own.  The live buffers ARE the averaged ones in here, so rank 0's go to every
                # rank, as before the raw validation: all ranks validate, and rank 0 saves, ONE averaged model.  The synced
                # statistics stay with the average on exit.
                dp.sync_buffers()
            vl, vm = validate()
            if dp is not None:
                vl, vm = all_reduce_sums(vl, vm)
            sd = model.state_dict() if rank == 0 else None
            sd = {k: v.detach().clone() for k, v in sd.items()} if sd is not None else None
        torch.set_rng_state(rng)
        return vl.item() / n_val, (vm.item() / n_val_batches if seg else 100 * vm.item() / n_val), sd

    for epoch in range(1, epochs + 1):
        if hasattr(criterion, "on_epoch"):
            criterion.on_epoch(epoch - 1, epochs)     # epoch-dependent loss weights (mnn.RegionBoundaryLoss), index from 0
        if not seg and epoch == STAGE1 + 1:
            say(f"\n--- STAGE 2: Full Fine-Tuning (Epochs {epoch}-{epochs}) ---")
            for p in model.parameters():
                p.requires_grad = True
            optimizer = make_optimizer(model.parameters(), lr)
            scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="max", factor=0.1, patience=3)
            say(f"Full fine-tuning (all layers unfrozen) with very low LR: {lr}. Using ReduceLROnPlateau scheduler.")

        model.train()
        loss_sum = torch.zeros((), device=device)
        hit_sum = torch.zeros((), device=device)
        seen = 0
        seen_all = 0                                  # samples this rank trained on (padding batches of the last step included)
        kd_sums = torch.zeros(2, device=device) if teacher is not None else None      # hard and KD term, sample-weighted
        for x, y in train_dl:
            x, y = x.to(device, non_blocking=True), y.to(device, non_blocking=True)
            if batch_mix is not None:
                x, y = batch_mix(x, y)
            if teacher is not None:
                y = DistillTarget(y, teacher_logits(teacher, x))      # (segmentation CutMix: the teacher sees the mixed image)
            optimizer.zero_grad(set_to_none=True)
            out = model(x)
            if seg and out.dim() == 3:
                out = out.unsqueeze(1)
            loss = criterion(out, y)
            scaler.scale(loss).backward()
            scaler.unscale_(optimizer)
            moptim.clip_grad_norm_(model.parameters(), max_norm=1.0, inv_scale=inv_scale)
            scaler.step(optimizer)
            if avg is not None and avg_mode == "ema":
                avg.update(optimizer)                 # one streaming launch; skips with the optimiser on inf / nan gradients
            scaler.update()
            loss_sum += loss.detach() * x.size(0)
            seen_all += x.size(0)
            if teacher is not None:
                kd_sums += criterion.last_terms[1:3] * x.size(0)
            if not seg:
                hit_sum += (torch.argmax(out.detach(), 1) == (y if batch_mix is None and teacher is None else getattr(y, "hard", y))).sum()
                seen += y.size(0)

        if dp is not None:
            dp.sync_buffers()                         # rank 0's BatchNorm statistics everywhere: one model is validated and saved
        vloss, vmetric = validate()

        # one host read-back per epoch (data parallel: one collective over the five accumulators first; the padded last
        # optimiser step makes the number of samples trained on larger than the dataset, so the mean divides by what was seen)
        if dp is not None:
            cnt = torch.tensor([float(seen_all), float(seen)], device=device, dtype=torch.float64)
            if teacher is None:
                loss_sum, hit_sum, vloss, vmetric, seen_all_t, seen_t = all_reduce_sums(loss_sum, hit_sum, vloss, vmetric, cnt[0], cnt[1])
            else:
                loss_sum, hit_sum, vloss, vmetric, seen_all_t, seen_t, kd_h, kd_k = all_reduce_sums(
                    loss_sum, hit_sum, vloss, vmetric, cnt[0], cnt[1], kd_sums[0], kd_sums[1])
                kd_sums = torch.stack([kd_h, kd_k])
            n_train_seen, seen = int(seen_all_t.item()), int(seen_t.item())
        else:
            n_train_seen = n_train
        train_loss = loss_sum.item() / n_train_seen
        val_loss = vloss.item() / n_val
        if seg:
            val_iou = vmetric.item() / n_val_batches
            score = val_loss
            say(f"[{name}] Ep{epoch}: TrainLoss {train_loss:.3f} | ValLoss {val_loss:.3f} | IoU {val_iou:.3f}")
            improved = val_loss < best_score
        else:
            train_acc = 100 * hit_sum.item() / max(seen, 1)
            val_acc = 100 * vmetric.item() / n_val
            score = val_acc
            say(f"[{name}] Ep{epoch}: TrainLoss {train_loss:.3f} (Acc {train_acc:.2f}%) | ValLoss {val_loss:.3f} | ValAcc {val_acc:.2f}%")
            improved = val_acc > best_score
        if teacher is not None:
            kd_h, kd_k = (kd_sums / n_train_seen).tolist()      # the epoch's means of the two terms as the kernels report them (criterion.last_terms)
            say(f"[{name}] Ep{epoch}: Distill hard {kd_h:.3f} | KD {kd_k:.3f}")

        if seg or epoch <= STAGE1:
            scheduler.step()
        else:
            scheduler.step(score)

        if improved:
            best_score, stale = score, 0
            if rank == 0:
                os.makedirs(save_dir, exist_ok=True)
                fname = f"{name}_best_loss.pt" if seg else f"{name}_best_acc.pt"
                torch.save(model.state_dict(), os.path.join(save_dir, fname))
        else:
            stale += 1

        if avg is not None and avg_mode == "ema":
            # the averaged model of this epoch: validated inside swap(), logged on a line of its own, saved on its own best score
            a_loss, a_metric, a_sd = validate_averaged(False)
            if seg:
                say(f"[{name}] Ep{epoch}: EMA ValLoss {a_loss:.3f} | IoU {a_metric:.3f}")
            else:
                say(f"[{name}] Ep{epoch}: EMA ValLoss {a_loss:.3f} | ValAcc {a_metric:.2f}%")
            if (a_loss < avg_best) if seg else (a_metric > avg_best):
                avg_best = a_loss if seg else a_metric
                if rank == 0:
                    os.makedirs(save_dir, exist_ok=True)
                    torch.save(a_sd, os.path.join(save_dir, f"{name}_ema_best_loss.pt" if seg else f"{name}_ema_best_acc.pt"))
        elif avg is not None and epoch >= swa_start:
            avg.update()                              # SWA: the iterate at the end of this epoch joins the equal-weight average

        if stale >= patience:
            say(f"Early stopping at epoch {epoch}. Best score: {best_score:.2f}")
            break

    if avg is not None and avg_mode == "swa":
        n_avg = int(avg.count.item())
        if n_avg == 0:
            say(f"[{name}] SWA: training stopped before epoch {swa_start}, nothing was averaged")
        else:
            # BatchNorm statistics of the averaged weights do not exist yet: re-estimate them on the training loader, then validate
            a_loss, a_metric, a_sd = validate_averaged(True)
            if seg:
                say(f"[{name}] SWA ({n_avg} epochs): ValLoss {a_loss:.3f} | IoU {a_metric:.3f}")
            else:
                say(f"[{name}] SWA ({n_avg} epochs): ValLoss {a_loss:.3f} | ValAcc {a_metric:.2f}%")
            if rank == 0:
                os.makedirs(save_dir, exist_ok=True)
                torch.save(a_sd, os.path.join(save_dir, f"{name}_swa.pt"))

    say(f"Training for {name} finished in {(time.time() - t0) / 60:.2f} minutes.")
    return best_score
