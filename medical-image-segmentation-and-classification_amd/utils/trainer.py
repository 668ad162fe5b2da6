"""Training entry point of the MI355X path — the counterpart of the reference's utils/trainer.py
(a ``__main__`` script: datasets -> loaders -> ``train()`` for each model, trainer.py:163-232).

The reference reads the COVID-19 Radiography dataset through Albumentations/cv2 (absent offline and
out of scope); this driver keeps its protocol — classification bs=16, segmentation bs=8,
80/20 split, 20 epochs, lr 1e-6 (trainer.py:28-37,159-160,199-210) — on any ``(x, y)`` datasets and
defaults to synthetic 256x256 batches so that it runs anywhere:

    python utils/trainer.py --task seg --model attentionunet --epochs 2 --samples 64
    python utils/trainer.py --task seg --model r2attunet --seg-loss bce_dice --bce-weight 0.5 --dice-weight 0.5
    python utils/trainer.py --task seg --model attentionunet --seg-loss bce_dice --boundary-weight 0.01 --boundary-schedule rebalance
    python utils/trainer.py --task seg --model attentionunet --seg-loss bce --lovasz-weight 0.5
    python utils/trainer.py --task seg --model attentionunet --data-root dataset --elastic-alpha 512 --elastic-sigma 20.5
    python utils/trainer.py --task seg --model attentionunet --data-root dataset --clahe-clip 4 --clahe-grid 8
    python utils/trainer.py --task cls --model resnet18 --mixup-alpha 0.2 --cutmix-alpha 1.0 --class-weight balanced
    python utils/trainer.py --task seg --model attentionunet --cutmix-alpha 1.0 --mix-prob 0.5
    python utils/trainer.py --task seg --model attentionunet --seg-classes 3 --seg-ce-weight 0.5 --seg-dice-weight 0.5
    python utils/trainer.py --task seg --model attentionunet --seg-loss focal_tversky --tversky-alpha 0.3 --tversky-beta 0.7
    python utils/trainer.py --task seg --model attentionunet --seg-loss focal_dice --focal-gamma 2 --focal-alpha 0.25
    python utils/trainer.py --task cls --model resnet18 --cls-loss focal --focal-gamma 2 --class-weight balanced
    python utils/trainer.py --task seg --model resnetunet --teacher weights/segmentation_models/attentionunet_best_loss.pt --teacher-model attentionunet

With ``--data-root dataset`` (the reference's DATA_ROOT layout: ``splits/train.csv``, ``<class>/images|masks/<id>.png``) it reads the
real files instead: two dataset objects per task with the train / val transforms, one 80/20 index split shared by both
(trainer.py:119-151), PNGs decoded by native threads and transformed on the GPU (utils/dataset.py, utils/gpu_transforms.py).

Data parallel (BASELINE.json north star; the reference is single-device): one process per GPU,

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 utils/trainer.py --task seg ...

The script joins the RCCL process group (backend "nccl"), draws the 80/20 split from a seed rank 0 broadcasts, and ``train()``
does the rest: batches sharded by rank, gradients all-reduced over xGMI during backward, rank 0 prints and saves.
"""
import argparse
import os
import sys

import torch
from torch.utils.data import DataLoader, TensorDataset, random_split

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from utils.helpers import get_class_model, get_seg_model, train  # noqa: E402

IMG_SIZE = 256
CLS_MODELS = ["resnet18", "resnet50", "vgg16", "vgg19"]
SEG_MODELS = ["resnetunet", "attentionunet", "r2unet", "r2attunet"]
# mi355.nn.FocalTverskyLoss (focal_arg).  The focal loss alone is focal_dice with --focal-weight 1 --tversky-weight 0: the name
# "focal" stays a choice the parser rejects (tests/test_seg_loss_cpu.py, tests/test_lovasz_cpu.py hold it to that).
FOCAL_SEG_LOSSES = ["tversky", "focal_tversky", "focal_dice"]


def synthetic_dataset(task, n, size, seed=0, classes=1):
    """``classes`` K > 1 (seg): nested, offset ellipses inside the K = 1 ellipse give uint8 labels 0 .. K - 1 [n, size, size], each
    class tinted differently; K = 1 is the binary set, tensor for tensor."""
    if classes != 1 and (task != "seg" or not 2 <= classes <= 16):
        raise ValueError(f"classes > 1 is for task 'seg' with 2 <= classes <= 16 (task={task!r}, classes={classes})")
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, size, size, generator=g)
    if task == "cls":
        return TensorDataset(x, torch.randint(0, 3, (n,), generator=g))
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    c = torch.rand(n, 4, generator=g)
    cy, cx = (0.4 + 0.2 * c[:, 0]) * size, (0.4 + 0.2 * c[:, 1]) * size
    ry, rx = (0.25 + 0.1 * c[:, 2]) * size, (0.25 + 0.1 * c[:, 3]) * size
    if classes > 1:
        lab = torch.zeros(n, size, size, dtype=torch.uint8)
        for k in range(1, classes):          # ellipse k: the outer one shrunk by (K - k) / (K - 1), its centre pushed towards +x / +y
            f = (classes - k) / (classes - 1)
            oy, ox = cy + 0.15 * (1 - f) * ry, cx + 0.25 * (1 - f) * rx
            inside = (((yy[None] - oy[:, None, None]) / (f * ry[:, None, None])) ** 2 +
                      ((xx[None] - ox[:, None, None]) / (f * rx[:, None, None])) ** 2) <= 1
            lab[inside] = k
        tint = torch.tensor([[0.0, 0.0, 0.0]] + [[1.0 - 0.35 * k, -0.7 + 0.45 * k, 0.4 * (-1) ** k + 0.1 * k] for k in range(classes - 1)])
        return TensorDataset(x + tint[lab.long()].permute(0, 3, 1, 2), lab)
    m = ((((yy[None] - cy[:, None, None]) / ry[:, None, None]) ** 2 + ((xx[None] - cx[:, None, None]) / rx[:, None, None]) ** 2) <= 1).float()
    return TensorDataset(x + m[:, None] * torch.tensor([1.0, -0.7, 0.4]).view(1, 3, 1, 1), m[:, None])


def make_loader(ds, bs, shuffle):
    return DataLoader(ds, batch_size=bs, shuffle=shuffle, num_workers=0, pin_memory=True, drop_last=False)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=["cls", "seg", "both"], default="seg")
    ap.add_argument("--model", default=None, help="one model name; default: every model of the task (trainer.py:163-168)")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-6)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--size", type=int, default=IMG_SIZE)
    ap.add_argument("--save-dir", default="weights")
    ap.add_argument("--data-root", default=None, help="dataset directory in the reference's layout; default: synthetic batches")
    ap.add_argument("--seg-loss", choices=["bce", "dice", "bce_dice", "lovasz"] + FOCAL_SEG_LOSSES, default="bce",
                    help="segmentation loss: BCEWithLogits (the reference's train()), Dice, bce_weight * BCE + dice_weight * Dice "
                         "(the reference's DiceLoss / CombinedLoss, clip_seg_finetuner.py:40-74), the Lovasz hinge (Berman et al. 2018), "
                         "the Tversky loss (Salehi et al. 2017), the focal-Tversky loss (Abraham & Khan 2019), or focal_weight * focal "
                         "(Lin et al. 2017) + tversky_weight * Dice (mi355.nn.FocalTverskyLoss; the focal loss alone: focal_dice with "
                         "--focal-weight 1 --tversky-weight 0)")
    ap.add_argument("--bce-weight", type=float, default=0.5, help="bce_dice: weight of the BCE term")
    ap.add_argument("--dice-weight", type=float, default=0.5, help="bce_dice: weight of the Dice term")
    ap.add_argument("--dice-per-sample", action="store_true", help="Dice term per image, averaged over the batch (default: over the whole batch)")
    ap.add_argument("--focal-gamma", type=float, default=2.0, help="focal_dice, --cls-loss focal: the focusing exponent (0: none)")
    ap.add_argument("--focal-alpha", type=float, default=0.25, help="focal_dice: weight of the positive pixels, 1 - alpha of the others; -1 = off")
    ap.add_argument("--tversky-alpha", type=float, default=0.7, help="tversky, focal_tversky: weight of the false positives")
    ap.add_argument("--tversky-beta", type=float, default=0.3, help="tversky, focal_tversky: weight of the false negatives (beta > alpha favours recall)")
    ap.add_argument("--tversky-exponent", type=float, default=0.75, help="focal_tversky: (1 - TI)^exponent; 0.75 is Abraham & Khan's gamma = 4/3")
    ap.add_argument("--focal-weight", type=float, default=0.5, help="focal_dice: weight of the focal term")
    ap.add_argument("--tversky-weight", type=float, default=0.5, help="focal_dice: weight of the Dice term")
    ap.add_argument("--cls-loss", choices=["ce", "focal"], default="ce",
                    help="cls: cross-entropy with label smoothing 0.1 (the reference's train()) or the focal cross-entropy "
                         "(mi355.nn.FocalCrossEntropyLoss(--focal-gamma), weighted by --class-weight balanced when given)")
    ap.add_argument("--boundary-weight", type=float, default=0.0,
                    help="weight of the boundary loss (Kervadec et al. 2019) added to --seg-loss; 0 = off")
    ap.add_argument("--boundary-schedule", choices=["constant", "rebalance"], default="constant",
                    help="constant: region + w * boundary; rebalance: (1 - a) * region + a * boundary, a = min(w + epoch * step, 0.99)")
    ap.add_argument("--boundary-step", type=float, default=0.01, help="rebalance: growth of the boundary weight per epoch")
    ap.add_argument("--lovasz-weight", type=float, default=0.0,
                    help="weight of the Lovasz hinge (Berman et al. 2018) added to --seg-loss bce|dice|bce_dice; 0 = off")
    ap.add_argument("--lovasz-batch", action="store_true",
                    help="Lovasz hinge over the flattened batch (default: per image, the B terms averaged)")
    ap.add_argument("--elastic-alpha", type=float, default=0.0,
                    help="--data-root: elastic deformation (A.ElasticTransform) in the train transforms, displacement scale in pixels; "
                         "0 = off; the usual pairing is 2 * size with sigma 0.08 * size")
    ap.add_argument("--elastic-sigma", type=float, default=None, help="elastic: Gaussian smoothing of the field in pixels; default 0.08 * size")
    ap.add_argument("--elastic-p", type=float, default=0.5, help="elastic: probability per sample")
    ap.add_argument("--clahe-clip", type=float, default=0.0,
                    help="--data-root: CLAHE (A.CLAHE) on the resized images of the train AND the validation transforms, clip limit; "
                         "0 = off; test and serve the model with the same values (tester.py --clahe-clip, JointPipeline.clahe)")
    ap.add_argument("--clahe-grid", type=int, default=8, help="CLAHE: tiles per side")
    ap.add_argument("--mixup-alpha", type=float, default=0.0,
                    help="cls: mixup (Zhang et al. 2018) on the training batches, lam ~ Beta(alpha, alpha); 0 = off; usual value 0.2")
    ap.add_argument("--cutmix-alpha", type=float, default=0.0,
                    help="cls and seg: CutMix (Yun et al. 2019) on the training batches (seg: image and mask get the same box); 0 = off; "
                         "usual value 1.0")
    ap.add_argument("--mix-prob", type=float, default=1.0, help="mixup / CutMix: probability that a batch (or a sample) is mixed")
    ap.add_argument("--mix-switch-prob", type=float, default=0.5, help="both alphas > 0: probability of CutMix, else mixup")
    ap.add_argument("--mix-per-sample", action="store_true", help="mixup / CutMix: a draw per sample (default: one per batch)")
    ap.add_argument("--class-weight", choices=["none", "balanced"], default="none",
                    help="cls: per-class loss weights n / (C * count_c) from the training files (--data-root; ignored for synthetic data)")
    ap.add_argument("--seg-classes", type=int, default=1,
                    help="seg: K > 1 trains K-channel heads on class-index masks (grey value = class, 255 = ignore) under softmax "
                         "cross-entropy + per-class Dice (mi355.nn.MultiClassSegLoss); 1 = the binary path")
    ap.add_argument("--seg-ce-weight", type=float, default=1.0, help="--seg-classes: weight of the cross-entropy term")
    ap.add_argument("--seg-dice-weight", type=float, default=0.0, help="--seg-classes: weight of the per-class Dice term")
    ap.add_argument("--seg-ignore-index", type=int, default=255, help="--seg-classes: the label left out of loss and metrics (-1: none)")
    ap.add_argument("--seg-class-weight", default=None, help="--seg-classes: comma-separated cross-entropy weights w0,w1,... one per class")
    ap.add_argument("--calibrate", action="store_true",
                    help="after training, fit the post-hoc calibration of the best checkpoint on the validation split (utils/calibrate.py): "
                         "a classifier's temperature, a segmenter's Dice-optimal mask threshold; written next to the checkpoint as "
                         "{name}_calibration.json for tester.py --calibration and JointPipeline(calibration=...)")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay (usual value 0.999; mi355/averaging.py): "
                         "validated on a line of its own every epoch and saved as {name}_ema_best_loss.pt / {name}_ema_best_acc.pt "
                         "(tester.py --weights-variant ema); off by default")
    ap.add_argument("--ema-warmup", type=float, default=10.0,
                    help="--ema-decay: the decay in force at update t is min(decay, (1 + t) / (warmup + t)); 0 = the plain decay")
    ap.add_argument("--swa-start", type=int, default=None,
                    help="stochastic weight averaging: the equal-weight average of the weights at the end of every epoch from this one "
                         "(1-based) on, BatchNorm statistics re-estimated on the training data, saved as {name}_swa.pt "
                         "(tester.py --weights-variant swa); off by default; not together with --ema-decay")
    ap.add_argument("--teacher", default=None,
                    help="knowledge distillation (Hinton et al. 2015; utils/distill.py): checkpoint of a trained model of --teacher-model "
                         "whose logits every training batch is also matched against; needs one --task; off by default")
    ap.add_argument("--teacher-model", default=None, help="--teacher: the teacher's model name (any name --model takes for the task)")
    ap.add_argument("--kd-weight", type=float, default=0.5,
                    help="--teacher: loss = (1 - w) * hard loss + w * T^2 * KL(teacher || student); in [0, 1]")
    ap.add_argument("--kd-temperature", type=float, default=None, help="--teacher: the temperature T; default 2 (seg) / 4 (cls)")
    return ap


def distill_arg(args):
    """--teacher / --teacher-model: None without them (today's loop), else dict(path, model, kd_weight, temperature), after a clear
    error for a half-given pair, for what the distillation losses are not combined with and for values out of range — raised here,
    before any data is read."""
    if args.teacher is None and args.teacher_model is None:
        return None
    if args.teacher is None or args.teacher_model is None:
        raise ValueError("--teacher (a checkpoint) and --teacher-model (its model name) go together")
    if args.task == "both":
        raise ValueError("--teacher with --task both: one teacher fits one task; run --task seg and --task cls separately")
    if args.task == "seg":
        if args.seg_loss not in ("bce", "dice", "bce_dice"):
            raise ValueError(f"--teacher: the distillation loss adds its term to --seg-loss bce|dice|bce_dice (got {args.seg_loss})")
        bad = [flag for flag, on in (("--boundary-weight", args.boundary_weight != 0), ("--lovasz-weight", args.lovasz_weight != 0),
                                     ("--seg-classes > 1", int(args.seg_classes) != 1)) if on]
        if bad:
            raise ValueError(f"--teacher: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} not combined with distillation "
                             "(binary BCE / Dice + KD is what is built)")
    else:
        bad = [flag for flag, on in (("--cls-loss focal", args.cls_loss == "focal"), ("--mixup-alpha", args.mixup_alpha != 0),
                                     ("--cutmix-alpha", args.cutmix_alpha != 0)) if on]
        if bad:
            raise ValueError(f"--teacher with --task cls: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} not combined with "
                             "distillation (hard labels under cross-entropy + KD is what is built)")
    fin = float("inf")
    if not 0 <= args.kd_weight <= 1:
        raise ValueError(f"--kd-weight must lie in [0, 1] ({args.kd_weight})")
    temp = (2.0 if args.task == "seg" else 4.0) if args.kd_temperature is None else args.kd_temperature
    if not 0 < temp < fin:
        raise ValueError(f"--kd-temperature must be a finite number > 0 ({temp})")
    if args.task == "seg" and not (0 <= args.bce_weight < fin and 0 <= args.dice_weight < fin):
        raise ValueError(f"--bce-weight and --dice-weight must be finite and not negative ({args.bce_weight}, {args.dice_weight})")
    return dict(path=args.teacher, model=args.teacher_model, kd_weight=float(args.kd_weight), temperature=float(temp))


def distill_criterion(args, kd, weight=None):
    """The loss of a distilled run (distill_arg has checked the flags): mi355.nn.SegDistillationLoss with --seg-loss's hard terms, or
    mi355.nn.DistillCrossEntropyLoss(label smoothing 0.1, ``weight`` from --class-weight balanced)."""
    from mi355 import nn as mnn
    if args.task == "seg":
        bw, dw = {"bce": (1.0, 0.0), "dice": (0.0, 1.0), "bce_dice": (args.bce_weight, args.dice_weight)}[args.seg_loss]
        return mnn.SegDistillationLoss(bw, dw, per_sample=args.dice_per_sample, kd_weight=kd["kd_weight"], temperature=kd["temperature"])
    return mnn.DistillCrossEntropyLoss(kd["kd_weight"], kd["temperature"], label_smoothing=0.1, weight=weight)


def load_teacher(kd, task, device):
    """The frozen teacher of a distilled run: --teacher-model with the weights of --teacher on ``device``, in eval mode, no gradients."""
    model = get_seg_model(kd["model"]) if task == "seg" else get_class_model(kd["model"])[0]
    model.load_state_dict(torch.load(kd["path"], map_location="cpu"))
    for p in model.parameters():
        p.requires_grad = False
    return model.to(device).eval()


def averaging_arg(args):
    """What train() takes as mi355.averaging.WithAveraging(train_dl, ...): None without --ema-decay / --swa-start (today's loop), else the dict it takes, after a
    clear error for both at once and for values out of range — raised here, before any data is read."""
    if args.ema_decay is not None and args.swa_start is not None:
        raise ValueError("--ema-decay and --swa-start are mutually exclusive: one average of the weights per run")
    if args.ema_decay is not None:
        if not 0 <= args.ema_decay < 1:
            raise ValueError(f"--ema-decay must lie in [0, 1) ({args.ema_decay})")
        if not (args.ema_warmup >= 0 and args.ema_warmup != float("inf")):
            raise ValueError(f"--ema-warmup must be a finite number >= 0 ({args.ema_warmup})")
        return {"mode": "ema", "decay": args.ema_decay, "warmup": args.ema_warmup}
    if args.swa_start is not None:
        if not 1 <= args.swa_start <= args.epochs:
            raise ValueError(f"--swa-start must be an epoch in [1, --epochs = {args.epochs}] ({args.swa_start})")
        return {"mode": "swa", "swa_start": args.swa_start}
    return None


AVERAGED_FILES = {"ema": ("{name}_ema_best_loss.pt", "{name}_ema_best_acc.pt"), "swa": ("{name}_swa.pt", "{name}_swa.pt")}


def calibrate_checkpoint(model, val_dl, device, name, save_dir, seg, say=print, variant=None):
    """--calibrate: reload ``name``'s best checkpoint from ``save_dir`` into ``model``, fit its calibration on ``val_dl`` (rank 0; the
    other ranks skip) and write the sidecar next to the checkpoint -> the Calibration, or None on the other ranks.  ``variant``
    "ema" / "swa": the averaged checkpoint instead, when train() wrote one (None otherwise); its sidecar is {name}_{variant}_calibration.json."""
    from utils.calibrate import Calibration, calibrate_model
    from utils.distributed import dist_info
    if dist_info()[0] != 0:
        return None
    fname = f"{name}_best_loss.pt" if seg else f"{name}_best_acc.pt"
    if variant is not None:
        fname = AVERAGED_FILES[variant][0 if seg else 1].format(name=name)
        if not os.path.exists(os.path.join(save_dir, fname)):
            return None
    model.load_state_dict(torch.load(os.path.join(save_dir, fname), map_location=device))
    cal = calibrate_model(model.to(device), val_dl, device, seg)
    tag = name if variant is None else f"{name}_{variant}"
    path = cal.save(Calibration.path(save_dir, tag))
    say(f"[calibration] {tag}: {cal.describe()} -> {path}")
    return cal


def elastic_arg(args):
    """The ``elastic=`` argument of the train transforms: None with --elastic-alpha 0 (today's transforms), else (alpha, sigma, p),
    validated here so that a bad flag fails before any data is read."""
    if args.elastic_alpha < 0:
        raise ValueError(f"--elastic-alpha must not be negative ({args.elastic_alpha})")
    if args.elastic_alpha == 0:
        return None
    from utils.elastic import check_elastic
    return check_elastic(args.elastic_alpha, 0.08 * args.size if args.elastic_sigma is None else args.elastic_sigma, args.elastic_p)


def clahe_arg(args):
    """The ``clahe=`` argument of the train and the validation transforms: None with --clahe-clip 0 (today's transforms), else
    (clip, (grid, grid)), validated here so that a bad flag fails before any data is read."""
    if not args.clahe_clip >= 0:
        raise ValueError(f"--clahe-clip must not be negative ({args.clahe_clip})")
    if args.clahe_clip == 0:
        return None
    from utils.clahe import check_clahe, tile_geometry
    clip, grid = check_clahe(args.clahe_clip, args.clahe_grid)
    tile_geometry(args.size, args.size, *grid)
    return clip, grid


def mix_arg(args, task, rank=0):
    """The mixer of one task's training batches (train() takes it as utils.mix.MixedBatches(train_dl, mixer)): None with both alphas 0
    (today's loop), else a utils.mix.BatchMix seeded with the rank (data-parallel ranks draw different mixes), validated here so that
    a bad flag fails before any data is read.  For --task seg only --cutmix-alpha is accepted."""
    for flag, v in (("--mixup-alpha", args.mixup_alpha), ("--cutmix-alpha", args.cutmix_alpha)):
        if not v >= 0 or v == float("inf"):
            raise ValueError(f"{flag} must be a finite number >= 0 ({v})")
    for flag, v in (("--mix-prob", args.mix_prob), ("--mix-switch-prob", args.mix_switch_prob)):
        if not 0 <= v <= 1:
            raise ValueError(f"{flag} must lie in [0, 1] ({v})")
    if task == "seg" and args.mixup_alpha > 0:
        if args.task == "both":
            raise ValueError("--mixup-alpha is for classifiers only: with --task both run the two tasks separately")
        raise ValueError("--mixup-alpha is not accepted with --task seg (a blended mask breaks the thresholded losses); use --cutmix-alpha")
    if args.mixup_alpha == 0 and args.cutmix_alpha == 0:
        return None
    from utils.mix import BatchMix
    return BatchMix(args.mixup_alpha, args.cutmix_alpha, p=args.mix_prob, switch_p=args.mix_switch_prob, per_sample=args.mix_per_sample,
                    seed=int(rank), seg=task == "seg")


def balanced_class_weights(labels, n_classes):
    """n / (C * count_c) per class (sklearn's "balanced"); a class without samples gets 0 (it cannot occur as a label)"""
    count = [0] * n_classes
    for c in labels:
        count[int(c)] += 1
    n = sum(count)
    return [n / (n_classes * k) if k else 0.0 for k in count]


def cls_criterion(args, batch_mix, dataset=None, indices=None, say=print):
    """The classifier's loss: None = train()'s own default (CrossEntropyLoss(0.1), or MixCrossEntropyLoss(0.1) on mixed batches);
    with --class-weight balanced MixCrossEntropyLoss(0.1, weight) from the labels of ``dataset.samples`` at ``indices``.  With
    --cls-loss focal: FocalCrossEntropyLoss(--focal-gamma, that weight or None) (cls_loss_arg has checked the flags)."""
    focal = cls_loss_arg(args)
    w = None
    if args.class_weight != "none":
        if dataset is None or not hasattr(dataset, "samples"):
            say("--class-weight balanced needs the file list of --data-root: ignored for synthetic data")
        else:
            from utils.helpers import CLASSES
            idx = range(len(dataset.samples)) if indices is None else indices
            w = balanced_class_weights([dataset.samples[i][1] for i in idx], len(CLASSES))
            say(f"class weights (balanced): {', '.join(f'{c} {v:.3f}' for c, v in zip(CLASSES, w))}")
    if focal:
        from mi355 import nn as mnn
        return mnn.FocalCrossEntropyLoss(gamma=args.focal_gamma, weight=w)
    if w is None:
        return None
    from mi355 import nn as mnn
    return mnn.MixCrossEntropyLoss(label_smoothing=0.1, weight=w)


def cls_loss_arg(args):
    """--cls-loss: False for ce (today's criterion), True for focal, after a clear error for what the focal cross-entropy cannot be
    combined with — raised here, before any data is read."""
    if args.cls_loss != "focal":
        return False
    if args.task == "seg":
        raise ValueError("--cls-loss focal is for classifiers (--task cls or both); the segmenters take --seg-loss focal_dice")
    bad = [flag for flag, v in (("--mixup-alpha", args.mixup_alpha), ("--cutmix-alpha", args.cutmix_alpha)) if v != 0]
    if bad:
        raise ValueError(f"--cls-loss focal: {', '.join(bad)} {'gives' if len(bad) == 1 else 'give'} two labels per sample, the focal "
                         "cross-entropy is defined for one true class; train mixed batches with --cls-loss ce")
    if not (args.focal_gamma >= 0 and args.focal_gamma != float("inf")):
        raise ValueError(f"--focal-gamma must be a finite number >= 0 ({args.focal_gamma})")
    return True


def focal_arg(args):
    """--seg-loss tversky | focal_tversky | focal_dice: None for the other losses, else the keyword arguments of
    mi355.nn.FocalTverskyLoss, after a clear error for the terms these losses are not combined with and for values out of range —
    raised here, before any data is read.  (--seg-classes > 1 next to them is multiclass_arg's error.)"""
    if args.seg_loss not in FOCAL_SEG_LOSSES:
        return None
    bad = [flag for flag, on in (("--boundary-weight", args.boundary_weight != 0), ("--lovasz-weight", args.lovasz_weight != 0)) if on]
    if bad:
        raise ValueError(f"--seg-loss {args.seg_loss}: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} added to --seg-loss "
                         "bce|dice|bce_dice only")
    fin = float("inf")
    if not (args.focal_gamma >= 0 and args.focal_gamma != fin):
        raise ValueError(f"--focal-gamma must be a finite number >= 0 ({args.focal_gamma})")
    if not (args.focal_alpha <= 1 and args.focal_alpha != -fin):
        raise ValueError(f"--focal-alpha must lie in [0, 1], or be negative (-1) for no class balance ({args.focal_alpha})")
    if not (args.tversky_alpha >= 0 and args.tversky_beta >= 0 and 0 < args.tversky_alpha + args.tversky_beta < fin):
        raise ValueError(f"--tversky-alpha and --tversky-beta must be finite, not negative and not both 0 ({args.tversky_alpha}, {args.tversky_beta})")
    if not 0 < args.tversky_exponent < fin:
        raise ValueError(f"--tversky-exponent must be a finite number > 0 ({args.tversky_exponent})")
    if not (0 <= args.focal_weight < fin and 0 <= args.tversky_weight < fin):
        raise ValueError(f"--focal-weight and --tversky-weight must be finite and not negative ({args.focal_weight}, {args.tversky_weight})")
    focal = dict(focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma)
    tversky = dict(alpha=args.tversky_alpha, beta=args.tversky_beta, per_sample=args.dice_per_sample)
    if args.seg_loss == "tversky":
        return dict(focal_weight=0.0, tversky_weight=1.0, exponent=1.0, **tversky)
    if args.seg_loss == "focal_tversky":
        return dict(focal_weight=0.0, tversky_weight=1.0, exponent=args.tversky_exponent, **tversky)
    return dict(focal_weight=args.focal_weight, tversky_weight=args.tversky_weight, alpha=0.5, beta=0.5, exponent=1.0,
                per_sample=args.dice_per_sample, **focal)


def multiclass_arg(args):
    """--seg-classes K: 1 -> None (the binary path, untouched); K > 1 -> the keyword arguments of mi355.nn.MultiClassSegLoss, after a
    clear error for every flag that is defined for one foreground only — raised here, before any data is read."""
    k = int(args.seg_classes)
    if k == 1:
        return None
    if not 2 <= k <= 16:
        raise ValueError(f"--seg-classes must lie in [1, 16] ({k})")
    if args.task != "seg":
        raise ValueError(f"--seg-classes {k} is for --task seg (got --task {args.task})")
    bad = [flag for flag, on in (("--seg-loss lovasz", args.seg_loss == "lovasz"),
                                 (f"--seg-loss {args.seg_loss}", args.seg_loss in FOCAL_SEG_LOSSES), ("--boundary-weight", args.boundary_weight != 0),
                                 ("--lovasz-weight", args.lovasz_weight != 0), ("--cutmix-alpha", args.cutmix_alpha != 0),
                                 ("--mixup-alpha", args.mixup_alpha != 0), ("--calibrate", args.calibrate)) if on]
    if bad:
        raise ValueError(f"--seg-classes {k}: {', '.join(bad)} {'is' if len(bad) == 1 else 'are'} defined for binary segmentation "
                         "only (one foreground) and cannot be combined with more than one class")
    w = None
    if args.seg_class_weight is not None:
        try:
            w = [float(v) for v in args.seg_class_weight.split(",")]
        except ValueError:
            raise ValueError(f"--seg-class-weight must be comma-separated numbers ({args.seg_class_weight!r})") from None
        if len(w) != k or any(not (v >= 0 and v != float("inf")) for v in w):
            raise ValueError(f"--seg-class-weight must hold {k} finite weights >= 0 ({args.seg_class_weight!r})")
    if args.seg_ce_weight < 0 or args.seg_dice_weight < 0:
        raise ValueError(f"--seg-ce-weight and --seg-dice-weight must not be negative ({args.seg_ce_weight}, {args.seg_dice_weight})")
    if args.seg_ignore_index != -1 and not k <= args.seg_ignore_index <= 255:
        raise ValueError(f"--seg-ignore-index must be -1 or lie in [{k}, 255] ({args.seg_ignore_index})")
    return dict(num_classes=k, ce_weight=args.seg_ce_weight, dice_weight=args.seg_dice_weight, class_weight=w,
                ignore_index=args.seg_ignore_index, per_sample=args.dice_per_sample)


def seg_criterion(args):
    """The loss module --seg-loss asks for; None = train()'s own default (BCEWithLogits).  With --boundary-weight > 0 it is that
    regional loss plus the boundary loss, as one criterion (mi355.nn.RegionBoundaryLoss); with --lovasz-weight > 0 that regional loss
    plus the Lovasz hinge (mi355.nn.RegionLovaszLoss).  Three terms are not combined.  With --seg-classes K > 1:
    mi355.nn.MultiClassSegLoss (multiclass_arg)."""
    mc = multiclass_arg(args)
    if mc is not None:
        from mi355 import nn as mnn
        return mnn.MultiClassSegLoss(**mc)
    ftv = focal_arg(args)
    if ftv is not None:
        from mi355 import nn as mnn
        return mnn.FocalTverskyLoss(**ftv)
    if args.boundary_weight < 0:
        raise ValueError(f"--boundary-weight must not be negative ({args.boundary_weight})")
    if args.lovasz_weight < 0:
        raise ValueError(f"--lovasz-weight must not be negative ({args.lovasz_weight})")
    if args.lovasz_weight > 0 and args.boundary_weight > 0:
        raise ValueError("--lovasz-weight and --boundary-weight cannot be combined: one term is added to --seg-loss at a time")
    if args.lovasz_weight > 0 and args.seg_loss == "lovasz":
        raise ValueError("--lovasz-weight adds the Lovasz hinge to --seg-loss bce|dice|bce_dice; --seg-loss lovasz is that loss alone")
    if args.seg_loss == "lovasz":
        if args.boundary_weight > 0:
            raise ValueError("--boundary-weight is added to --seg-loss bce|dice|bce_dice, not to --seg-loss lovasz")
        from mi355 import nn as mnn
        return mnn.LovaszHingeLoss(per_image=not args.lovasz_batch)
    if args.lovasz_weight > 0:
        from mi355 import nn as mnn
        bw, dw = {"bce": (1.0, 0.0), "dice": (0.0, 1.0), "bce_dice": (args.bce_weight, args.dice_weight)}[args.seg_loss]
        return mnn.RegionLovaszLoss(bw, dw, args.lovasz_weight, per_sample=args.dice_per_sample, per_image=not args.lovasz_batch)
    if args.boundary_weight > 0:
        from mi355 import nn as mnn
        bw, dw = {"bce": (1.0, 0.0), "dice": (0.0, 1.0), "bce_dice": (args.bce_weight, args.dice_weight)}[args.seg_loss]
        return mnn.RegionBoundaryLoss(bw, dw, args.boundary_weight, per_sample=args.dice_per_sample, schedule=args.boundary_schedule,
                                      step=args.boundary_step)
    if args.seg_loss == "bce":
        return None
    from mi355 import nn as mnn
    if args.seg_loss == "dice":
        return mnn.DiceLoss(per_sample=args.dice_per_sample)
    return mnn.CombinedLoss(args.bce_weight, args.dice_weight, per_sample=args.dice_per_sample)


def main():
    args = build_parser().parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the MI355X path needs a GPU (no CPU fallback)")
    # one process per GPU under torch.distributed.run: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the launcher
    world, rank, local_rank = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    # (MI355_DP_BACKEND=gloo: ranks may share a GPU — a rehearsal of the launcher path on a one-GPU box, tests/test_gpu_dp_train.py;
    #  RCCL wants a device per rank)
    backend = os.environ.get("MI355_DP_BACKEND", "nccl")
    local_dev = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_dev)
    device = torch.device("cuda", local_dev)
    split_gen = None                                      # (single process: unseeded, like the reference's random_split)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        seed = [int(torch.randint(0, 2 ** 31 - 1, (1,)))]
        dist.broadcast_object_list(seed, src=0)          # every rank must cut the SAME 80/20 split
        split_gen = torch.Generator().manual_seed(seed[0])
    say = print if rank == 0 else (lambda *a, **k: None)
    results = {}
    tasks = ["cls", "seg"] if args.task == "both" else [args.task]
    mixes = {task: mix_arg(args, task, rank) for task in tasks}          # (a bad flag fails before any data is read)
    multi = multiclass_arg(args) is not None
    if not multi and "seg" in tasks:
        focal_arg(args)
    cls_loss_arg(args)
    averaging = averaging_arg(args)
    kd = distill_arg(args)
    variant = None if averaging is None else averaging["mode"]
    seg_labels = {"labels": True} if multi else {}
    for task in tasks:
        names = [args.model] if args.model else (CLS_MODELS if task == "cls" else SEG_MODELS)
        bs = 16 if task == "cls" else 8
        if args.data_root:
            from utils.dataset import ClassificationDataset, GpuBatchLoader, SegmentationDataset
            from utils.gpu_transforms import ClsBatchTransform, SegBatchTransform
            DS, TF = (ClassificationDataset, ClsBatchTransform) if task == "cls" else (SegmentationDataset, SegBatchTransform)
            kw = seg_labels if task == "seg" else {}
            ds_tr = DS(args.data_root, TF(args.size, train=True, device=device, elastic=elastic_arg(args), clahe=clahe_arg(args), **kw), "train", **kw)
            ds_va = DS(args.data_root, TF(args.size, train=False, device=device, clahe=clahe_arg(args), **kw), "train", **kw)
            if len(ds_tr) == 0:
                say(f"{task} dataset is empty under {args.data_root}. Skipping.")
                continue
            n_train = int(0.8 * len(ds_tr))
            perm = torch.randperm(len(ds_tr), generator=split_gen).tolist()      # (unseeded, like the reference's random_split)
            train_dl = GpuBatchLoader(ds_tr, bs, shuffle=True, device=device, indices=perm[:n_train])
            val_dl = GpuBatchLoader(ds_va, bs, shuffle=True, device=device, indices=perm[n_train:])
        else:
            full = synthetic_dataset(task, args.samples, args.size, classes=args.seg_classes if task == "seg" else 1)
            n_train = int(0.8 * len(full))
            tr, va = random_split(full, [n_train, len(full) - n_train], generator=split_gen) if split_gen is not None else \
                random_split(full, [n_train, len(full) - n_train])
            train_dl, val_dl = make_loader(tr, bs, True), make_loader(va, bs, False)
        if mixes[task] is not None:
            from utils.mix import MixedBatches
            train_dl = MixedBatches(train_dl, mixes[task])
        if kd is not None:
            from utils.distill import Distilled
            train_dl = Distilled(train_dl, load_teacher(kd, task, device))
            say(f"distillation: teacher {kd['model']} from {kd['path']}, kd weight {kd['kd_weight']}, temperature {kd['temperature']}")
        if averaging is not None:
            from mi355.averaging import WithAveraging
            train_dl = WithAveraging(train_dl, dict(averaging))
        cls_crit = None
        if task == "cls":
            cls_crit = cls_criterion(args, mixes[task], ds_tr if args.data_root else None, perm[:n_train] if args.data_root else None, say)
            if kd is not None:
                cls_crit = distill_criterion(args, kd, None if cls_crit is None else cls_crit.weight)
        for name in names:
            say(f"\n{'=' * 20} {task.upper()} :: {name} {'=' * 20}")
            if task == "cls":
                model, head = get_class_model(name)
                best = train(model, train_dl, val_dl, device, args.epochs, args.lr, name, os.path.join(args.save_dir, "classification_models"),
                             seg=False, cls_head_name=head, criterion=cls_crit)
                if args.calibrate:
                    calibrate_checkpoint(model, val_dl, device, name, os.path.join(args.save_dir, "classification_models"), False, say)
                    if variant is not None:
                        calibrate_checkpoint(model, val_dl, device, name, os.path.join(args.save_dir, "classification_models"), False, say, variant)
            else:
                model = get_seg_model(name, classes=args.seg_classes)
                best = train(model, train_dl, val_dl, device, args.epochs, args.lr, name, os.path.join(args.save_dir, "segmentation_models"), seg=True,
                             criterion=seg_criterion(args) if kd is None else distill_criterion(args, kd))
                if args.calibrate:
                    calibrate_checkpoint(model, val_dl, device, name, os.path.join(args.save_dir, "segmentation_models"), True, say)
                    if variant is not None:
                        calibrate_checkpoint(model, val_dl, device, name, os.path.join(args.save_dir, "segmentation_models"), True, say, variant)
            results[(task, name)] = best
    say("\n===== SUMMARY =====")
    for (task, name), best in results.items():
        say(f"{task:>4} {name:<14} best {'val loss' if task == 'seg' else 'val acc'}: {best:.4f}")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
