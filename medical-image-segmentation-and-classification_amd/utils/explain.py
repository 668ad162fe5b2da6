"""Grad-CAM for the classifiers and the GPU-rendered overlays of the joint pipeline.

``GradCAM(model)(x)`` explains each sample's class at the feature map the classifier's head consumes (the layer every
ResNet / VGG Grad-CAM targets by default: layer4's output, the output of ``features``).  It runs the model's explain plan
(mi355/graph.py ``Builder.cam_tap``): the eval forward, a one-hot seed of the explained class, the head's backward down to the
tapped map, and the map itself (csrc/explain.hip ``mi355_gradcam``):

    alpha[c] = mean_hw dA[hw, c],   raw = relu(sum_c alpha[c] A[., c]),   cam = (raw - min) / (1e-7 + max(raw - min))

(pytorch-grad-cam's order: normalise at the feature-map size, then resize).  No parameter gradient is formed, so a CAM can be
taken between two training steps; ``model.training`` is left as it is.  Everything is enqueued on the current stream.

``overlay_mask`` is the reference's red blend of a segmentation mask (pipeline.py:399-407), ``overlay_heatmap`` the usual
jet-coloured Grad-CAM overlay; both work on device uint8 RGB images [B, H, W, 3]."""
from __future__ import annotations

import torch

from mi355.lib import lib


def resize_bilinear(maps, size):
    """fp32 [B, h, w] -> [B, H, W]: F.interpolate(mode="bilinear", align_corners=False) (mi355_resize_bilinear_f32)."""
    B, h, w = maps.shape
    H, W = int(size[0]), int(size[1])
    if maps.dtype != torch.float32 or not maps.is_contiguous():
        raise TypeError("resize_bilinear: contiguous float32 maps expected")
    out = torch.empty(B, H, W, dtype=torch.float32, device=maps.device)
    lib.mi355_resize_bilinear_f32(maps, B, h, w, out, H, W)
    return out


class GradCAM:
    """``GradCAM(model)(x, target=None, size=None)`` -> dict of device tensors:

    ``logits``      float32 [B, K]: what ``model.eval()(x)`` returns in the same compute dtype, bit for bit;
    ``target``      int32 [B]: the explained class (``target``, else each sample's first maximum logit);
    ``cam_lowres``  float32 [B, h, w] in [0, 1] at the feature-map size;
    ``cam``         float32 [B, H, W] in [0, 1], resized bilinearly to ``size`` (default: the input's H, W).

    ``model``: any classifier of models/classification_models; a model without a CAM tap (the segmenters) raises
    NotImplementedError.  ``target``: None, an int, a sequence of B ints, or an integer tensor of B classes."""

    def __init__(self, model):
        self.model = model

    def _target(self, target, B, K, device):
        if target is None:
            return None
        if isinstance(target, torch.Tensor):
            t = target.reshape(-1)
            if t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
                raise TypeError("GradCAM: target must hold integer classes")
            if t.device.type == "cpu" and (t.numel() and (int(t.min()) < 0 or int(t.max()) >= K)):
                raise ValueError(f"GradCAM: target classes must lie in [0, {K})")
            t = t.to(device=device, dtype=torch.int32).contiguous()
        else:
            vals = [int(target)] * B if isinstance(target, int) else [int(v) for v in target]
            if any(v < 0 or v >= K for v in vals):
                raise ValueError(f"GradCAM: target classes must lie in [0, {K})")
            t = torch.tensor(vals, dtype=torch.int32).to(device)
        if t.numel() != B:
            raise ValueError(f"GradCAM: {t.numel()} targets for a batch of {B}")
        return t

    def __call__(self, x, target=None, size=None):
        if x.dim() != 4:
            raise ValueError("GradCAM: x must be [B, 3, H, W]")
        B, _, H, W = x.shape
        K = self._num_classes()
        logits, tgt, cam_lowres = self.model.explain(x, self._target(target, B, K, x.device))
        cam = resize_bilinear(cam_lowres, size if size is not None else (H, W))
        return {"logits": logits, "target": tgt, "cam_lowres": cam_lowres, "cam": cam}

    def _num_classes(self):
        last = None
        for m in self.model.modules():
            if isinstance(m, torch.nn.Linear):
                last = m
        if last is None:
            raise NotImplementedError(f"Grad-CAM: {type(self.model).__name__} has no classifier head")
        return last.out_features


def _check_images(images, who):
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_contiguous():
        raise TypeError(f"{who}: images must be contiguous uint8 [B, H, W, 3] (RGB)")
    if images.device.type != "cuda":
        raise RuntimeError(f"{who}: the images must be on the GPU")


def overlay_mask(images, masks, opacity=0.5):
    """The reference's segmentation overlay (pipeline.py:399-407): masks uint8 [B, h, w] (0 / 255, at the model's resolution) are
    resized nearest to the image size; where a mask is 255, R += 255 * opacity (rounded half to even, saturated).  -> uint8 [B, H, W, 3]."""
    _check_images(images, "overlay_mask")
    B, H, W, _ = images.shape
    if masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != B or masks.device != images.device:
        raise TypeError("overlay_mask: masks must be uint8 [B, h, w] on the images' device")
    masks = masks.contiguous()
    out = torch.empty_like(images)
    lib.mi355_overlay_mask(images, B, H, W, masks, masks.shape[1], masks.shape[2], float(opacity), out)
    return out


def overlay_heatmap(images, cam, alpha=0.4):
    """Grad-CAM overlay: out = (1 - alpha) * image + alpha * 255 * jet(cam) per channel, rounded half to even and saturated;
    ``cam`` float32 [B, H, W] in [0, 1] at the image size (resize it first: ``GradCAM(..., size=(H, W))``)."""
    _check_images(images, "overlay_heatmap")
    B, H, W, _ = images.shape
    if cam.dtype != torch.float32 or tuple(cam.shape) != (B, H, W) or cam.device != images.device:
        raise TypeError(f"overlay_heatmap: cam must be float32 [{B}, {H}, {W}] on the images' device")
    cam = cam.contiguous()
    out = torch.empty_like(images)
    lib.mi355_overlay_heatmap(images, B, H, W, cam, float(alpha), out)
    return out
