"""Knowledge distillation (Hinton et al. 2015; nothing in the reference): a frozen teacher's logits as a second target of the
student's loss.

    teacher = get_seg_model("AttentionUNet"); teacher.load_state_dict(torch.load("AttentionUNet_best_loss.pt"))
    train(student, Distilled(train_dl, teacher), val_dl, device, ..., seg=True,
          criterion=mnn.SegDistillationLoss(1, 0, kd_weight=0.5, temperature=2))

``train()`` takes the wrapper apart as it does ``utils.mix.MixedBatches`` and ``mi355.averaging.WithAveraging`` (the nesting is
``WithAveraging(Distilled(MixedBatches(loader, batch_mix), teacher), averaging)``), runs the teacher forward only, in eval mode, on
every TRAINING batch behind ``batch_mix``, and hands the criterion a ``DistillTarget``.  The losses are ``mi355.nn.SegDistillationLoss``
and ``mi355.nn.DistillCrossEntropyLoss`` (csrc/distill.hip); validation stays on the hard target alone."""
import torch


class DistillTarget:
    """The target of a distilled batch: the hard target ``hard`` (a mask batch or an integer label tensor) and the teacher's logits
    ``teacher_logits`` (float32, of the student's output shape; the loss checks the shape).  ``hard`` is what training accuracy counts."""

    def __init__(self, hard, teacher_logits):
        if not torch.is_tensor(hard) or not torch.is_tensor(teacher_logits):
            raise TypeError(f"DistillTarget: two tensors expected, got {type(hard).__name__} and {type(teacher_logits).__name__}")
        if not teacher_logits.dtype.is_floating_point:
            raise ValueError(f"DistillTarget: teacher_logits must be floating point (got {teacher_logits.dtype})")
        if hard.size(0) != teacher_logits.size(0):
            raise ValueError(f"DistillTarget: {hard.size(0)} hard targets but {teacher_logits.size(0)} rows of teacher logits")
        self.hard, self.teacher_logits = hard, teacher_logits

    def to(self, *args, **kwargs):
        """Moves both tensors; a dtype among the arguments applies to the (floating-point) teacher logits only."""
        device_only = [a for a in args if not isinstance(a, torch.dtype)]
        hard_kwargs = {k: v for k, v in kwargs.items() if k != "dtype"}
        return DistillTarget(self.hard.to(*device_only, **hard_kwargs), self.teacher_logits.to(*args, **kwargs))

    def size(self, dim=None):
        return self.hard.size() if dim is None else self.hard.size(dim)

    def __len__(self):
        return self.hard.size(0)

    def __repr__(self):
        return f"DistillTarget(hard={tuple(self.hard.shape)}, teacher_logits={tuple(self.teacher_logits.shape)})"


def teacher_logits(teacher, x):
    """The teacher's logits on ``x``: no graph, eval mode (its previous mode is put back), a 3-d segmenter output [N,H,W] unsqueezed
    to [N,1,H,W], float32.  The tensor is a copy: a mi355 ``Net`` may hand out a buffer that its next forward overwrites."""
    was_training = getattr(teacher, "training", False)
    if was_training:
        teacher.eval()
    try:
        with torch.no_grad():
            v = teacher(x)
    finally:
        if was_training:
            teacher.train()
    if not torch.is_tensor(v):
        raise TypeError(f"the teacher must return a logit tensor (got {type(v).__name__})")
    if v.dim() == 3:
        v = v.unsqueeze(1)
    return v.detach().to(torch.float32, copy=True).contiguous()


class Distilled:
    """A training loader with the teacher that goes with it: ``train(model, Distilled(train_dl, teacher), val_dl, ...)``.  ``teacher``:
    any callable that returns logits of the student's output shape on the device, normally a mi355 ``Net`` on that device with its
    trained weights.  ``train()`` never writes its parameters or buffers.  ``loader`` may itself be a ``MixedBatches`` (segmentation
    CutMix: the teacher sees the mixed image).  In a hand-written loop, iterating the wrapper yields ``(x, DistillTarget)``; the loader
    must then deliver batches on the teacher's device (``GpuBatchLoader``), or ``device`` says where to move them first."""

    def __init__(self, loader, teacher, device=None):
        if not callable(teacher):
            raise TypeError(f"Distilled: teacher must be a callable that returns logits, got {type(teacher).__name__}")
        self.loader, self.teacher, self.device = loader, teacher, device
        self.dataset = getattr(loader, "dataset", None)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for x, y in self.loader:
            if self.device is not None:
                x, y = x.to(self.device, non_blocking=True), y.to(self.device, non_blocking=True)
            yield x, DistillTarget(y, teacher_logits(self.teacher, x))
