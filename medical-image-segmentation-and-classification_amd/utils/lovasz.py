"""The segmented stable argsort and the Lovasz hinge on the device (csrc/segsort.hip, csrc/lovasz.hip), for callers outside autograd —
what mi355.nn.LovaszHingeLoss / RegionLovaszLoss run, exposed for inspection and for other uses of the sort.

``segmented_argsort`` orders every row like ``np.argsort(kind="stable")`` (-0.0 == +0.0, equal keys in ascending index); NaN keys are
not supported as an order.  Everything stays on the device: no host round trip, no synchronisation, the same bits on every run."""
import torch

from mi355 import nn as mnn


def _device_f32(x, what):
    if not x.is_cuda:
        raise ValueError(f"{what} is computed on the GPU: a device tensor is expected (there is no CPU fallback)")
    return x.float().contiguous()


def segmented_argsort(keys):
    """device fp32 [S, len] (or [len]) -> int32 of the same shape: perm[s, k] = index within row s of its k-th smallest key."""
    if keys.dim() not in (1, 2):
        raise ValueError(f"segmented_argsort expects keys [S, len] or [len], got {tuple(keys.shape)}")
    k = _device_f32(keys, "the segmented sort")
    perm = mnn._segmented_argsort(k.view(-1, k.shape[-1]))
    return perm.view(keys.shape)


def lovasz_hinge(logits, target, per_image=True, threshold=0.5):
    """-> (loss, dloss/dlogits): the Lovasz hinge of one-channel logits [B,1,H,W] or [B,H,W] against ``target > threshold``, per image
    and averaged (``per_image=True``) or over the flattened batch.  loss is a 0-d fp32 tensor, the gradient has the logits' shape."""
    if not ((logits.dim() == 4 and logits.shape[1] == 1) or logits.dim() == 3):
        raise ValueError(f"the Lovasz hinge is defined for one-channel logits [B,1,H,W] or [B,H,W], got {tuple(logits.shape)}")
    z = _device_f32(logits, "the Lovasz hinge")
    t = _device_f32(target, "the Lovasz hinge")
    if t.numel() != z.numel():
        raise ValueError(f"target size {tuple(target.shape)} must match input size {tuple(logits.shape)}")
    B = z.shape[0]
    S, n = (B, z.numel() // B) if per_image else (1, z.numel())
    loss = torch.empty(1, dtype=torch.float32, device=z.device)
    coef = mnn._lovasz_fwd(z, t, S, n, threshold, 1.0, None, loss)
    return loss.view(()), coef.view(logits.shape)
