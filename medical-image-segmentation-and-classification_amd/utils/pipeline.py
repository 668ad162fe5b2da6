"""Joint inference path of the reference (utils/pipeline.py:324-357 ``_predict_classification`` /
``_predict_segmentation``, decision logic of ``process_image`` :359-418) as ONE batched pass on the GPU:

    classify the batch -> softmax / argmax / confidence on the device -> compact the samples predicted
    "COVID" -> segment only those -> sigmoid > 0.5 -> uint8 masks scattered back to their batch slots.

The reference handles one PIL image per call and synchronises after every model; here the only host
round-trip is the number of kept samples (it sizes the segmentation launch).  The compacted batch is
padded to a multiple of ``bucket`` so that at most B / bucket launch plans ever exist per image size.
``predict`` takes the already normalised tensor (``val_transform`` output) and returns the masks (with ``explain=True``
also the Grad-CAM map of every sample's predicted class, utils/explain.py).  ``process_images`` is ``process_image``'s
per-file result — the red overlay at the file's own size (:399-413, mi355_overlay_mask) and the analysis text (:391-417) —
for a list of PNG files, run as one batch.  ``postprocess`` (a utils.postprocess.MaskPostprocess; nothing in the reference) cleans
the masks by connected components on the device before they are overlaid and adds the lesion count and area to the text.
``pipeline.clahe = (clip, grid)`` equalises the resized images in ``process_files`` / ``process_images`` (utils/clahe.py) — the
values the models were trained with (trainer.py --clahe-clip / --clahe-grid); the overlays are still drawn on the file's own pixels.
``tta`` (a preset name or a list of views, utils/tta.py): both models predict on every view and the merged predictions decide; the
result gains a per-pixel uncertainty map and the views' agreement, and the analysis text says how stable the highlighted area is.
``sliding=(tile, overlap, weighting)`` (utils/sliding.py): the kept samples are segmented at the resolution of ``predict``'s ``x_seg``
(``seg_size`` in ``process_files`` / ``process_images``) by overlapping windows of ``tile`` pixels blended on the GPU; the masks come
back at that resolution, with a map of how far overlapping windows disagree.  The classifier's path is unchanged.
``calibration=(cls_cal, seg_cal)`` (utils/calibrate.py, fitted by trainer.py --calibrate): the confidence comes from the
temperature-scaled logits and every mask is cut at the fitted threshold instead of 0.5; the analysis text says so in one sentence."""
from __future__ import annotations

import numpy as np
import torch

from mi355 import nn as mnn
from mi355.lib import lib

CLASSES = ["COVID", "Healthy", "Non-COVID"]          # pipeline.py:22


class _KeywordOptions(type):
    """``JointPipeline(..., tta=None, tta_merge="prob", sliding=None, seg_size=None, calibration=None)``: the options are keywords of the call, set
    through their properties once ``__init__`` has run, so ``__init__`` keeps the positional parameter list its callers rely on."""

    def __call__(cls, *args, tta=None, tta_merge="prob", sliding=None, seg_size=None, calibration=None, **kwargs):
        self = super().__call__(*args, **kwargs)
        self.calibration = calibration
        self.tta_merge = tta_merge
        self.tta = tta
        self.sliding = sliding
        self.seg_size = seg_size
        return self


class _TemperatureScaled:
    """a classifier whose logits are multiplied by the double at ``beta`` on the device (mi355_logits_scale): what TTAClassifier is
    handed when the pipeline is calibrated"""

    def __init__(self, model, beta):
        self.model, self.beta = model, beta

    @property
    def training(self):
        return self.model.training

    def __call__(self, x):
        return mnn._logits_scale(self.model(x).float().contiguous(), self.beta)


class JointPipeline(metaclass=_KeywordOptions):
    def __init__(self, classification_model, segmentation_model, device="cuda", classes=CLASSES, positive="COVID", bucket=4, postprocess=None):
        self.device = torch.device(device)
        self._tta, self._tta_merge = None, "prob"
        self._sliding, self._seg_size, self._sw = None, None, None
        self.classes = list(classes)
        self.keep = self.classes.index(positive)
        self.bucket = int(bucket)
        self.postprocess = postprocess
        self._clahe = None
        self._calibration, self._beta, self._thr = None, None, 0.5
        self.classification_model = classification_model.to(self.device).eval()
        self.segmentation_model = None if segmentation_model is None else segmentation_model.to(self.device).eval()

    @property
    def clahe(self):
        """None (default: the transforms as they were) or (clip, (gy, gx)): CLAHE on the resized images of ``process_files`` /
        ``process_images``.  Set it to the (clip, grid) the models were trained with; validated on assignment."""
        return self._clahe

    @clahe.setter
    def clahe(self, value):
        if value is None:
            self._clahe = None
            return
        from utils.clahe import check_clahe
        if len(value) != 2:
            raise ValueError(f"clahe must be None or (clip, grid), got {value!r}")
        self._clahe = check_clahe(*value)

    @property
    def calibration(self):
        """None (default: the softmax as it is, masks cut at 0.5) or (cls_cal, seg_cal), two ``utils.calibrate.Calibration`` — either
        may be None: the classifier's logits are divided by cls_cal's temperature before the decision, so ``confidence`` is the
        calibrated one (the class is the same), and seg_cal's threshold takes the place of 0.5 wherever a mask is cut."""
        return self._calibration

    @calibration.setter
    def calibration(self, value):
        if value is None:
            self._calibration, self._beta, self._thr = None, None, 0.5
            return
        if len(value) != 2:
            raise ValueError(f"calibration must be None or (cls_cal, seg_cal), got {value!r}")
        cls_cal, seg_cal = value
        if (cls_cal is not None and cls_cal.kind != "classification") or (seg_cal is not None and seg_cal.kind != "segmentation"):
            raise ValueError("calibration: (a classification Calibration or None, a segmentation Calibration or None) expected")
        if cls_cal is not None and not cls_cal.temperature > 0:
            raise ValueError(f"calibration: temperature > 0 required, got {cls_cal.temperature}")
        self._beta = None if cls_cal is None else torch.tensor([1.0 / cls_cal.temperature], dtype=torch.float64, device=self.device)
        self._thr = 0.5 if seg_cal is None else float(np.float32(seg_cal.threshold))
        self._calibration = (cls_cal, seg_cal)
        self._sw = None                            # (the window segmenter holds the threshold)

    def _clean(self, masks):
        """the postprocess on 0 / 255 masks: against the calibrated threshold when there is one (the same cut for any value in (0, 255))"""
        return self.postprocess(masks) if self._calibration is None else self.postprocess(masks, threshold=self._thr)

    @property
    def tta(self):
        """None (default: one forward pass per model) or the views of test-time augmentation (utils/tta.py): a preset name or a list
        of (angle_deg, scale, hflip), validated on assignment and kept as that list."""
        return self._tta

    @tta.setter
    def tta(self, value):
        if value is None:
            self._tta = None
            return
        from utils.tta import check_views
        if self._sliding is not None:
            raise ValueError("JointPipeline: tta together with sliding is not supported: set one of the two")
        self._tta = check_views(value)

    @property
    def sliding(self):
        """None (default: the segmenter sees the batch ``predict`` is given) or (tile, overlap, weighting): sliding-window
        segmentation (utils/sliding.py), validated on assignment.  Not together with ``tta``."""
        return self._sliding

    @sliding.setter
    def sliding(self, value):
        if value is None:
            self._sliding = None
            return
        from utils.sliding import check_sliding
        value = check_sliding(value)
        if self._tta is not None:
            raise ValueError("JointPipeline: sliding together with tta is not supported: set one of the two")
        self._sliding = value

    @property
    def seg_size(self):
        """None (default) or the side ``process_files`` / ``process_images`` resize the images to for the sliding-window segmenter
        (the classifier keeps ``size``); at least the tile, checked when used together with ``sliding``."""
        return self._seg_size

    @seg_size.setter
    def seg_size(self, value):
        if value is None:
            self._seg_size = None
            return
        if isinstance(value, bool) or int(value) != value or int(value) < 1:
            raise ValueError(f"seg_size must be None or a positive integer, got {value!r}")
        self._seg_size = int(value)

    @property
    def tta_merge(self):
        """"prob" (default) or "logit": what the segmenter's views are averaged as"""
        return self._tta_merge

    @tta_merge.setter
    def tta_merge(self, value):
        from utils.tta import MERGES
        if value not in MERGES:
            raise ValueError(f"tta_merge must be one of {MERGES}, got {value!r}")
        self._tta_merge = value

    @torch.no_grad()
    def predict(self, x, explain=False, x_seg=None):
        """x: [B,3,H,W] normalised float (B <= 1024).  Returns a dict of device tensors:
        ``pred`` int32 [B] class index, ``confidence`` float [B] in percent, ``masks`` uint8 [B,H,W] (0 / 255; all zero
        where no segmentation ran), ``segmented`` bool [B].  ``explain``: also ``cam`` float32 [B,H,W] (and ``cam_lowres`` at
        the feature-map size), the Grad-CAM of each sample's predicted class; the logits then come from the classifier's explain
        plan, whose forward is the eval forward: every other output is the same, bit for bit.  With a ``postprocess``: ``masks`` are
        the cleaned masks, ``masks_raw`` the thresholded ones, ``n_lesions`` int32 [B] and ``area_percent`` float64 [B] the kept
        components and their share of the image, ``lesions`` int32 [B,max_report,8] their rows (utils/postprocess.py).  With ``tta``:
        ``pred`` / ``confidence`` come from the views' mean softmax and the masks from their merged maps (before any postprocess);
        also ``agreement`` int32 [B] (views whose own class is ``pred``), ``uncertainty`` fp32 [B,H,W] (the variance of the views'
        probabilities, or logits for tta_merge="logit"; zero where nothing was segmented) and ``stable_percent`` fp32 [B] (the share
        of the pixels of ``masks`` — the cleaned masks with a postprocess — on which every view that sees them votes alike; 0 without a mask).  ``explain`` with ``tta``: ValueError.
        With ``sliding``: the kept samples are taken from ``x_seg`` ([B,3,Hs,Ws], the same images at the segmenter's resolution;
        default x; Hs, Ws >= tile) and segmented window by window in chunks of ``bucket`` windows; ``masks`` are uint8 [B,Hs,Ws] and
        ``seam_spread`` fp32 [B,Hs,Ws] is, per pixel, the largest minus the smallest logit the windows covering it give (zero where
        one window covers and where nothing was segmented).  ``x_seg`` without ``sliding``: ValueError."""
        x = x.to(self.device, dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        if x_seg is not None and self.sliding is None:
            raise ValueError("JointPipeline: x_seg is the sliding-window segmenter's input: set sliding=(tile, overlap, weighting)")
        seam = None
        if self.sliding is not None:
            x_seg = x if x_seg is None else x_seg.to(self.device, dtype=torch.float32).contiguous()
            if x_seg.dim() != 4 or x_seg.shape[0] != B or x_seg.shape[1] != 3:
                raise ValueError(f"JointPipeline: x_seg must be [{B},3,Hs,Ws], got {tuple(x_seg.shape)}")
            H, W = x_seg.shape[2:]                    # the masks' size from here on
            if min(H, W) < self.sliding[0]:
                raise ValueError(f"JointPipeline: sliding: the segmenter's input ({H} x {W}) must be at least the tile ({self.sliding[0]})")
        if self.tta is not None:
            if explain:
                raise ValueError("JointPipeline: explain=True is not defined with tta (Grad-CAM of an averaged prediction)")
            return self._predict_tta(x)
        cams = None
        if explain:
            from utils.explain import GradCAM
            cams = GradCAM(self.classification_model)(x)
            logits = cams["logits"].float().contiguous()
        else:
            logits = self.classification_model(x).float().contiguous()
        if self._beta is not None:
            logits = mnn._logits_scale(logits, self._beta)
        pred = torch.empty(B, dtype=torch.int32, device=self.device)
        conf = torch.empty(B, dtype=torch.float32, device=self.device)
        kept = torch.empty(B + self.bucket, dtype=torch.int32, device=self.device)
        n_kept = torch.empty(1, dtype=torch.int32, device=self.device)
        lib.mi355_cls_decide(logits, B, logits.shape[1], self.keep, pred, conf, kept, n_kept)
        masks = torch.zeros(B, H, W, dtype=torch.uint8, device=self.device)
        segmented = pred == self.keep
        n = int(n_kept)                               # the one host sync: sizes the segmentation launch
        if self.sliding is not None:
            seam = torch.zeros(B, H, W, dtype=torch.float32, device=self.device)
        if n and self.segmentation_model is not None and self.sliding is not None:
            xs = torch.empty(n, 3, H, W, dtype=torch.float32, device=self.device)
            lib.mi355_gather_rows(x_seg, kept, n, 3 * H * W, xs)
            f = self._window_segmenter()(xs, kept, masks)
            seam[kept[:n].long()] = f["spread"]
        elif n and self.segmentation_model is not None:
            npad = -(-n // self.bucket) * self.bucket
            if npad > n:
                kept[n:npad] = kept[0]                 # padding rows repeat a kept sample; their output is dropped
            xs = torch.empty(npad, 3, H, W, dtype=torch.float32, device=self.device)
            lib.mi355_gather_rows(x, kept, npad, 3 * H * W, xs)
            z = self.segmentation_model(xs)
            if z.dim() == 3:
                z = z.unsqueeze(1)
            lib.mi355_mask_scatter(z.float().contiguous(), kept, n, H * W, self._thr, masks)
        elif self.segmentation_model is None:
            segmented = torch.zeros_like(segmented)
        out = {"pred": pred, "confidence": conf, "masks": masks, "segmented": segmented}
        if seam is not None:
            out["seam_spread"] = seam
        if self.postprocess is not None:
            clean = self._clean(masks)                 # 0 / 255 against 0.5; rows without a segmentation are empty and stay so
            out.update(masks=clean["mask"], masks_raw=masks, n_lesions=clean["n_kept"], area_percent=clean["area_percent"],
                       lesions=clean["out_c"])
        if cams is not None:
            out["cam"], out["cam_lowres"] = cams["cam"], cams["cam_lowres"]
        return out

    def _window_segmenter(self):
        """the SlidingWindowSegmenter of the current (sliding, bucket, segmentation_model), kept between calls: it holds the tile
        lists and the window weights on the device"""
        from utils.sliding import SlidingWindowSegmenter
        key = (self.sliding, self.bucket, self.segmentation_model)
        if self._sw is None or self._sw[0] != key[:2] or self._sw[1] is not key[2]:
            tile, overlap, weighting = self.sliding
            self._sw = (key[:2], key[2], SlidingWindowSegmenter(key[2], tile, overlap, weighting, "logit", self._thr, self.bucket))
        return self._sw[2]

    def _predict_tta(self, x):
        """predict() with test-time augmentation: the same steps, every model call replaced by its K views and their merge"""
        from utils.tta import TTAClassifier, fold_views, view_logits
        B, _, H, W = x.shape
        classifier = self.classification_model if self._beta is None else _TemperatureScaled(self.classification_model, self._beta)
        c = TTAClassifier(classifier, self.tta, keep_class=self.keep, pad=self.bucket)(x)
        pred, kept = c["pred"], c["kept"]
        masks = torch.zeros(B, H, W, dtype=torch.uint8, device=self.device)
        uncertainty = torch.zeros(B, H, W, dtype=torch.float32, device=self.device)
        stable = torch.zeros(B, dtype=torch.float32, device=self.device)
        segmented = pred == self.keep
        same = None
        n = int(c["n_kept"])                          # the one host sync: sizes the segmentation launches
        if n and self.segmentation_model is not None:
            npad = -(-n // self.bucket) * self.bucket
            if npad > n:
                kept[n:npad] = kept[0]                 # padding rows repeat a kept sample; their output is dropped
            xs = torch.empty(npad, 3, H, W, dtype=torch.float32, device=self.device)
            lib.mi355_gather_rows(x, kept, npad, 3 * H * W, xs)
            f = fold_views(view_logits(self.segmentation_model, xs, self.tta, rows=n), self.tta, self.tta_merge, self._thr, kept, masks)
            rows = kept[:n].long()
            uncertainty[rows] = f["var"]
            same = (f["votes"] == 0) | (f["votes"] == f["valid"])
        elif self.segmentation_model is None:
            segmented = torch.zeros_like(segmented)
        out = {"pred": pred, "confidence": c["confidence"], "masks": masks, "segmented": segmented, "agreement": c["agreement"],
               "uncertainty": uncertainty, "stable_percent": stable}
        if self.postprocess is not None:
            clean = self._clean(masks)
            out.update(masks=clean["mask"], masks_raw=masks, n_lesions=clean["n_kept"], area_percent=clean["area_percent"],
                       lesions=clean["out_c"])
        if same is not None:                          # over the masks that are returned and overlaid: the cleaned ones with a postprocess
            on = out["masks"][rows] != 0
            stable[rows] = ((on & same).flatten(1).sum(1).float() / on.flatten(1).sum(1).clamp(min=1).float()) * 100
        return out

    def process_files(self, paths, size=256, threads=8):
        """PNG files -> the reference's per-image results.  The reference opens each file with PIL, applies ``A.Resize(256, 256)`` +
        ``A.Normalize`` + ``ToTensorV2`` (pipeline.py:186-193, 381-390) and runs the two models; here the files of one size are
        decoded by native threads (utils/dataset.py) and resized / normalised on the GPU (utils/gpu_transforms.py) as ONE batch."""
        from utils.dataset import decode_batch, read_files
        from utils.gpu_transforms import SegBatchTransform
        imgs = decode_batch(read_files(paths), 3, threads, names=list(paths))
        imgs = imgs.to(self.device, non_blocking=True)
        x = SegBatchTransform(size, train=False, device=self.device, clahe=self.clahe)(imgs)
        return self.process_batch(x, self._seg_input(imgs, size))

    def _seg_input(self, imgs, size):
        """the decoded images resized to ``seg_size`` by the same transform (same CLAHE), or None: the segmenter sees the
        classifier's batch"""
        if self.seg_size is None:
            return None
        if self.sliding is None:
            raise ValueError("JointPipeline: seg_size is the sliding-window segmenter's input size: set sliding=(tile, overlap, weighting)")
        if self.seg_size < self.sliding[0]:
            raise ValueError(f"JointPipeline: seg_size ({self.seg_size}) must be at least the tile ({self.sliding[0]})")
        from utils.gpu_transforms import SegBatchTransform
        if self.seg_size == size:
            return None
        return SegBatchTransform(self.seg_size, train=False, device=self.device, clahe=self.clahe)(imgs)

    def process_batch(self, x, x_seg=None):
        """The reference's per-image result shape: list of (prediction, confidence_percent, mask uint8 [H,W] or None).  ``x_seg``:
        predict's."""
        r = self.predict(x, x_seg=x_seg)
        pred, conf, seg = r["pred"].cpu(), r["confidence"].cpu(), r["segmented"].cpu()
        masks = r["masks"].cpu()
        return [(self.classes[int(pred[i])], float(conf[i]), masks[i] if bool(seg[i]) else None) for i in range(len(pred))]

    def process_images(self, paths, overlay_opacity=0.5, explain=False, size=256, threads=8, heatmap_alpha=0.4):
        """PNG files -> one ``process_image`` result per file (pipeline.py:359-418): ``(prediction, confidence, output_img,
        analysis_text)``.  ``output_img`` is a numpy uint8 RGB image at the file's own size — the red overlay of the segmentation
        mask — for a "COVID" call with a segmentation model, else None, as in the reference.  ``explain``: a fifth element, the
        Grad-CAM overlay (utils/explain.py overlay_heatmap, weight ``heatmap_alpha``) of the predicted class at the file's size.
        Files of several sizes are decoded per size; all of them are classified / segmented as one batch."""
        from utils.dataset import decode_batch, png_size, read_files
        from utils.explain import overlay_heatmap, overlay_mask, resize_bilinear
        from utils.gpu_transforms import SegBatchTransform
        paths = list(paths)
        bufs = read_files(paths)
        groups = {}
        for i, b in enumerate(bufs):
            groups.setdefault(png_size(b), []).append(i)
        tf = SegBatchTransform(size, train=False, device=self.device, clahe=self.clahe)
        order, imgs, xs, xsegs = [], [], [], []
        for idx in groups.values():
            im = decode_batch([bufs[i] for i in idx], 3, threads, names=[paths[i] for i in idx]).to(self.device, non_blocking=True)
            order.append(idx)
            imgs.append(im)
            xs.append(tf(im))
            xsegs.append(self._seg_input(im, size))
        x_seg = None if xsegs[0] is None else (torch.cat(xsegs) if len(xsegs) > 1 else xsegs[0])
        r = self.predict(torch.cat(xs) if len(xs) > 1 else xs[0], explain=explain, x_seg=x_seg)
        grid_line = None
        if self.sliding is not None:
            from utils.sliding import tile_starts
            Hs, Ws = r["masks"].shape[1:]
            tile, overlap, weighting = self.sliding
            grid_line = (f"\nSliding window: {len(tile_starts(Hs, tile, overlap))} x {len(tile_starts(Ws, tile, overlap))} tiles of {tile} px "
                         f"on {Hs} x {Ws} (overlap {overlap:g}, {weighting} weights).")
        pred, conf = r["pred"].cpu(), r["confidence"].cpu()
        lesions = (r["n_lesions"].cpu(), r["area_percent"].cpu()) if "n_lesions" in r else None
        stable = r["stable_percent"].cpu() if "stable_percent" in r else None
        positive = self.classes[self.keep]
        cal_line = ""
        if self._calibration is not None:
            cls_cal, seg_cal = self._calibration
            parts = ([f"confidence at temperature {cls_cal.temperature:.3f}"] if cls_cal is not None else []) \
                + ([f"mask threshold {self._thr:.4f}"] if seg_cal is not None else [])
            cal_line = "Calibrated on the validation set: " + " and ".join(parts) + ".\n" if parts else ""
        results = [None] * len(paths)
        row = 0
        for idx, im in zip(order, imgs):
            n, H0, W0, _ = im.shape
            red = overlay_mask(im, r["masks"][row:row + n], overlay_opacity).cpu().numpy() if self.segmentation_model is not None else None
            heat = None
            if explain:
                heat = overlay_heatmap(im, resize_bilinear(r["cam_lowres"][row:row + n].contiguous(), (H0, W0)), heatmap_alpha).cpu().numpy()
            for j, i in enumerate(idx):
                prediction, confidence = self.classes[int(pred[row + j])], float(conf[row + j])
                output_img = None
                text = f"Diagnosis: {prediction}\nConfidence: {confidence:.2f}%\n"
                text += cal_line
                if prediction != positive:
                    text += ("\nRecommendation: Consult a medical professional for final diagnosis. The model suggests no severe "
                             "COVID-19 pathology.")
                elif red is not None:
                    output_img = red[j]
                    text += "\nInfection areas have been highlighted in red (segmentation model)."
                    if lesions is not None:
                        text += f"\nLesions: {int(lesions[0][row + j])} (area {float(lesions[1][row + j]):.2f}% of the image)."
                    if grid_line is not None:
                        text += grid_line
                    if stable is not None:
                        text += (f"\nStable under test-time augmentation: {float(stable[row + j]):.2f}% of the highlighted pixels "
                                 f"({len(self.tta)} views).")
                else:
                    text += "\nWARNING: Segmentation model failed to load. Cannot highlight infection areas."
                results[i] = (prediction, confidence, output_img, text) + ((heat[j],) if explain else ())
            row += n
        return results
