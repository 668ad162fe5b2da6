"""CPU: the Grad-CAM explain plan (host-side only, nothing launched) and the numpy restatements the GPU tests
(tests/test_gpu_explain.py) compare the overlay kernels against (tests/explain_ref.py: restated from the reference's cv2 calls
and matplotlib's jet, which are not installed here — see that module)."""
import numpy as np
import pytest
import torch

import explain_ref as ref
from mi355 import graph
from mi355.lib import available
from test_plan_cpu import _models

CLASSIFIERS = [n for n in _models() if n.startswith(("ResNet", "resnet", "VGG"))]
SEGMENTERS = [n for n in _models() if n not in CLASSIFIERS]
HEAD_LAUNCHES = {"mi355_linear_bwd", "mi355_global_pool_bwd", "mi355_adaptive_avgpool_bwd"}

needs_lib = pytest.mark.skipif(not available(), reason="libmi355conv.so not built")


def _flat_range(eng):
    base = eng.flat_g.data_ptr()
    return base, base + eng.flat_g.numel() * 4


@needs_lib
@pytest.mark.parametrize("name", CLASSIFIERS)
def test_explain_plan(name):
    ctor, shape = _models()[name]
    net = ctor()
    eng = net.engine
    eng.flatten()
    plan = eng.plan_for(shape, False, False, torch.float32, explain=True)
    fwd, bwd = plan.bind(0)                     # resolves every pointer and checks ABI arity; launches nothing
    assert plan.grad_params == [] and plan.zero_grad_params == []
    lo, hi = _flat_range(eng)
    for _, args, lname, _ in fwd + bwd:
        for a in args[:-1]:
            assert not (isinstance(a, int) and lo <= a < hi), (lname, "points into flat_g")
    names = [l.name for l in plan.bwd]
    assert names[0] == "mi355_cam_seed" and names[-1] == "mi355_gradcam"
    assert set(names[1:-1]) <= HEAD_LAUNCHES and names[1] == "mi355_linear_bwd"
    assert not any(l.side for l in plan.bwd)
    # the tap: the head's input, the only tensor upstream of the head that needs a gradient
    t, g = plan.cam, plan.cam_grad
    assert t.needs_grad and g.ld == t.ld and g.buf.dtype == torch.float32
    assert plan.bwd[-1].args[:4] == (t, t.ld, g, g.ld)
    assert plan.cam_lowres.numel() >= t.N * t.H * t.W and plan.cam_target.dtype == torch.int32
    # the forward is the eval plan's, launch for launch
    ev = eng.plan_for(shape, False, False, torch.float32)
    assert [l.name for l in plan.pre + plan.fwd] == [l.name for l in ev.pre + ev.fwd]
    assert ev is not plan and not ev.bwd


@needs_lib
@pytest.mark.parametrize("name", CLASSIFIERS)
def test_cam_tap_leaves_train_and_eval_plans_alone(name, monkeypatch):
    ctor, shape = _models()[name]

    def summary(training):
        net = ctor().train(training)
        net.engine.flatten()
        p = net.engine.plan_for(shape, training, training, torch.bfloat16)
        return [l.name for l in p.pre + p.fwd], [l.name for l in p.bwd], len(p.grad_params)
    got = {tr: summary(tr) for tr in (True, False)}
    monkeypatch.setattr(graph.Builder, "cam_tap", lambda self, t: t)
    want = {tr: summary(tr) for tr in (True, False)}
    assert got == want


@needs_lib
@pytest.mark.parametrize("name", SEGMENTERS)
def test_segmenters_cannot_be_explained(name):
    ctor, shape = _models()[name]
    net = ctor()
    net.engine.flatten()
    with pytest.raises(NotImplementedError, match=name):
        net.engine.plan_for(shape, False, False, torch.float32, explain=True)


def test_explain_needs_a_gpu():
    from utils.explain import GradCAM
    from models.classification_models.ResNet import ResNet18
    with pytest.raises(RuntimeError, match="GPU"):
        GradCAM(ResNet18(3))(torch.zeros(1, 3, 32, 32))


# ---- the numpy restatements ----------------------------------------------------------------------------------------------
def test_jet_lut_against_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    lut = mpl.colormaps["jet"](np.arange(256))[:, :3].astype(np.float32)
    assert np.array_equal(lut, ref.jet_lut())
    v = np.linspace(0, 1, 1001)
    assert np.array_equal(mpl.colormaps["jet"](v)[:, :3].astype(np.float32), ref.jet(v))


def test_jet_lut_segments():
    lut = ref.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.float32
    assert lut[0].tolist() == [0.0, 0.0, 0.5] and lut[255].tolist() == [0.5, 0.0, 0.0]
    # green ramps up over [0.125, 0.375]: entry i sits at x = i / 255
    i = 64
    assert abs(float(lut[i, 1]) - (i / 255 - 0.125) / 0.25) < 1e-7
    assert ref.jet(np.float32(1.0)).tolist() == lut[255].tolist() and ref.jet(np.float32(255 / 256)).tolist() == lut[255].tolist()
    assert ref.jet(np.float32(0.0)).tolist() == lut[0].tolist()


def test_overlay_mask_restatement():
    img = np.full((4, 6, 3), 100, np.uint8)
    img[0, 0] = (250, 1, 2)
    mask = np.zeros((2, 3), np.uint8)
    mask[0, 0] = 255
    mask[1, 2] = 254                                              # not 255: untouched
    out = ref.overlay_mask(img, mask, 0.5)
    on = np.zeros((4, 6), bool)
    on[:2, :2] = True                                             # nearest: rows (y * 2) // 4, columns (x * 3) // 6
    assert np.array_equal(out[..., 1:], img[..., 1:])
    assert out[0, 0, 0] == 255                                    # saturated
    assert (out[on][1:, 0] == 228).all()                          # 100 + 127.5 -> 228 (half to even)
    assert (out[~on] == img[~on]).all()
    assert ref.overlay_mask(np.full((1, 1, 3), 101, np.uint8), np.full((1, 1), 255, np.uint8), 0.5)[0, 0, 0] == 228   # 228.5 -> 228


def test_overlay_heatmap_restatement():
    img = np.zeros((1, 3, 3), np.uint8)
    img[0, :, 0] = 200
    cam = np.array([[0.0, 0.5, 1.0]], np.float32)
    out = ref.overlay_heatmap(img, cam, 0.5)
    lut = ref.jet_lut()
    for j, k in enumerate((0, 128, 255)):
        want = np.rint(np.float32(0.5) * img[0, j].astype(np.float32) + np.float32(127.5) * lut[k])
        assert out[0, j].tolist() == want.astype(np.uint8).tolist()
    assert ref.overlay_heatmap(img, cam, 0.0).tolist() == img.tolist()


def test_analysis_texts():
    assert ref.analysis_text("Healthy", 91.234) == ("Diagnosis: Healthy\nConfidence: 91.23%\n\nRecommendation: Consult a medical "
                                                    "professional for final diagnosis. The model suggests no severe COVID-19 pathology.")
    assert ref.analysis_text("COVID", 50.0) == "Diagnosis: COVID\nConfidence: 50.00%\n\nInfection areas have been highlighted in red (segmentation model)."
    assert ref.analysis_text("COVID", 50.0, segmented=False).endswith("WARNING: Segmentation model failed to load. Cannot highlight infection areas.")
