"""numpy restatements of the Grad-CAM overlays (csrc/explain.hip) and of the reference's ``process_image`` output
(utils/pipeline.py:391-417 of the reference), used by tests/test_explain_cpu.py and tests/test_gpu_explain.py.

PARITY UNPINNED at this boundary: the reference draws the overlay with OpenCV (``cv2.resize(INTER_NEAREST)``,
``cv2.addWeighted``) and the usual Grad-CAM overlay uses matplotlib's ``jet``; neither cv2 nor (here) matplotlib is
installed, so what they compute is restated from their documented behaviour instead of being run:
  - nearest resize: source index ``(dst * src_size) // dst_size``;
  - ``addWeighted(img, 1, overlay, opacity, 0)`` on uint8: ``saturate_cast<uchar>(img + overlay * opacity)`` in float32,
    rounded half to even;
  - ``jet``: matplotlib's LinearSegmentedColormap lookup table (``_create_lookup_table``) of the jet segment data, 256
    entries, looked up at ``min(int(v * 256), 255)``.
The ``jet`` table is cross-checked against matplotlib where it is installed (tests/test_explain_cpu.py)."""
import numpy as np

JET_DATA = {
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}

COVID_TEXT = "\nInfection areas have been highlighted in red (segmentation model)."
NO_SEG_TEXT = "\nWARNING: Segmentation model failed to load. Cannot highlight infection areas."
OTHER_TEXT = "\nRecommendation: Consult a medical professional for final diagnosis. The model suggests no severe COVID-19 pathology."


def _lut(points, n=256):
    xs = np.array([p[0] for p in points], dtype=np.float64)
    ys = np.array([p[1] for p in points], dtype=np.float64)
    x = np.linspace(0.0, 1.0, n)
    ind = np.searchsorted(xs, x)[1:-1]
    dist = (x[1:-1] - xs[ind - 1]) / (xs[ind] - xs[ind - 1])
    lut = np.concatenate([[ys[0]], dist * (ys[ind] - ys[ind - 1]) + ys[ind - 1], [ys[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_lut():
    """float32 [256, 3] RGB in [0, 1]."""
    return np.stack([_lut(JET_DATA[c]) for c in ("red", "green", "blue")], 1).astype(np.float32)


def jet(v):
    """RGB float32 [..., 3] of values v in [0, 1]."""
    idx = np.minimum((np.asarray(v, dtype=np.float32) * np.float32(256)).astype(np.int64), 255)
    return jet_lut()[np.maximum(idx, 0)]


def _round_sat(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)      # np.rint: half to even


def nearest_resize(mask, H, W):
    """mask [h, w] -> [H, W], source index (dst * h) // H."""
    h, w = mask.shape
    ys = (np.arange(H, dtype=np.int64) * h) // H
    xs = (np.arange(W, dtype=np.int64) * w) // W
    return mask[ys[:, None], xs[None, :]]


def overlay_mask(img, mask, opacity):
    """img uint8 [H, W, 3] RGB, mask uint8 [h, w] -> the reference's red blend (pipeline.py:399-407)."""
    H, W, _ = img.shape
    on = nearest_resize(mask, H, W) == 255
    out = img.copy()
    red = img[..., 0].astype(np.float32) + np.float32(255) * np.float32(opacity)
    out[..., 0] = np.where(on, _round_sat(red), img[..., 0])
    return out


def overlay_heatmap(img, cam, alpha):
    """img uint8 [H, W, 3], cam float32 [H, W] in [0, 1] -> (1 - alpha) img + alpha 255 jet(cam), float32, half to even."""
    a = np.float32(alpha)
    keep, a255 = np.float32(1) - a, a * np.float32(255)
    return _round_sat(keep * img.astype(np.float32) + a255 * jet(cam))


def analysis_text(prediction, confidence, positive="COVID", segmented=True):
    """The reference's analysis_text (pipeline.py:391-417) for a known prediction."""
    text = f"Diagnosis: {prediction}\nConfidence: {confidence:.2f}%\n"
    if prediction != positive:
        return text + OTHER_TEXT
    return text + (COVID_TEXT if segmented else NO_SEG_TEXT)
