"""-m gpu: the connected-component clean-up (csrc/components.hip, utils.postprocess, JointPipeline(postprocess=...)) on the device
against the restatement tests/components_ref.py (pinned to scipy.ndimage and to its fixture on the CPU, tests/test_components_cpu.py).

Every comparison is exact equality: the masks, the labels, the eight integers per sample and the component rows are integers.  Every
input is judged through the C ABI and through label_components_batch.  At 1024 x 1024 the inputs have closed forms."""
import itertools
import struct
import zlib

import numpy as np
import pytest
import torch

import components_ref as R
from mi355.lib import lib
from oracle import nets
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_AN = {}


def analysis(key, M, conn, fill):
    """restatement of one batch of boolean masks up to the filter, computed once per key and never modified"""
    k = (key, conn, fill)
    if k not in _AN:
        _AN[k] = [R.analyse(m, conn, fill) for m in M]
    return _AN[k]


def abi(src, is_logit=False, thr=0.5, conn=8, fill=0, min_area=0, keep=0, report=8, labels=True):
    B, H, W = src.shape
    n = lib.raw("mi355_components_ws_ints")(B, H, W)
    assert n > 0, lib.raw("mi355_last_error")()
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    mask = torch.full((B, H, W), 7, dtype=torch.uint8, device=DEV)
    lab = torch.full((B, H, W), -7, dtype=torch.int32, device=DEV) if labels else None
    out_i = torch.full((B, 8), -7, dtype=torch.int32, device=DEV)
    out_c = torch.full((B, report, 8), -7, dtype=torch.int32, device=DEV)
    lib.mi355_components(src, B, H, W, 1 if is_logit else 0, thr, conn, fill, min_area, keep, report, ws, n, mask, lab, out_i,
                         out_c if report else None)
    torch.cuda.synchronize()
    return mask, lab, out_i, out_c


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).to(DEV)


def check(key, M, src, conn, fill, min_area, keep, report, labels=True, python=True):
    from utils import postprocess as pp
    an = analysis(key, M, conn, fill)
    fin = [R.finish(a, min_area, keep, report) for a in an]
    want = {"labels": np.stack([a["labels"] for a in an]), "mask": np.stack([f[0] for f in fin]), "out_i": np.stack([f[1] for f in fin]),
            "out_c": np.stack([f[2] for f in fin])}
    mask, lab, out_i, out_c = abi(src, False, 0.5, conn, fill, min_area, keep, report, labels)
    what = (key, conn, fill, min_area, keep, report, labels)
    assert np.array_equal(out_i.cpu().numpy(), want["out_i"]), (what, out_i.cpu().tolist(), want["out_i"].tolist())
    assert np.array_equal(out_c.cpu().numpy(), want["out_c"]), (what, out_c.cpu().tolist(), want["out_c"].tolist())
    assert np.array_equal(mask.cpu().numpy(), want["mask"]), what
    if labels:
        assert np.array_equal(lab.cpu().numpy(), want["labels"]), what
    if python:
        res = pp.label_components_batch(src[:, None], False, 0.5, conn, fill, min_area, keep, report)
        assert torch.equal(res["mask"], mask) and torch.equal(res["out_i"], out_i) and torch.equal(res["out_c"], out_c), what
        if labels:
            assert torch.equal(res["labels"], lab), what
        assert torch.equal(res["n_components"], out_i[:, 2]) and torch.equal(res["n_kept"], out_i[:, 3])
        assert res["area_percent"].dtype == torch.float64 and res["centroids"].shape == (len(M), report, 2)
        assert np.array_equal(res["area_percent"].cpu().numpy(), want["out_i"][:, 4] * (100.0 / (M.shape[1] * M.shape[2])))
        np.testing.assert_array_equal(res["centroids"].cpu().numpy(), R.centroids(want["out_c"]))      # NaN == NaN here
    return mask, lab, out_i, out_c


# odd and narrower than a wavefront; one row; one column; two samples; wider / taller than one block, no multiple of 64
SHAPES = [(3, 17, 13), (1, 1, 9), (1, 8, 1), (2, 64, 64), (1, 40, 300), (1, 300, 40)]
GRID = list(itertools.product((0, 4, 8), (0, 2, 50), (0, 1, 2, 5), (0, 3, 16), (True, False)))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_mask_kind_and_setting_at_the_small_shapes(shape, conn):
    """every kind of mask of components_ref.kinds, stacked into one batch, under the whole grid of settings"""
    kinds = R.kinds(*shape, seed=sum(shape))
    assert list(kinds) == ["noise", "ellipses", "edge", "all_foreground", "all_background", "single_pixels", "checkerboard", "comb",
                           "u_and_ring", "diagonal", "squares"]
    M = np.concatenate(list(kinds.values()))
    src = dev(M)
    for fill, min_area, keep, report, labels in GRID:
        check(shape, M, src, conn, fill, min_area, keep, report, labels)
    n = [len(a["table"]) for a in analysis(shape, M, conn, 0)]
    print(f"{shape} conn {conn}: components per sample {n}")


def _mixed_batch():
    """(8, 256, 256): noise, the ellipses of oracle.train.synthetic_batch (one with a stray blob and a pin-hole), masks cut by the
    frame, a checkerboard window, a comb, rings, single pixels, nothing"""
    H = W = 256
    rng = np.random.RandomState(256)
    M = np.zeros((8, H, W), dtype=bool)
    M[0] = rng.rand(H, W) < 0.5
    m = otrain.synthetic_batch(4, 256, seed=3)[1][:, 0].numpy() > 0.5
    M[1] = m[0] | R.ellipse(H, W, 20, 230, 4, 6)
    M[1, 128, 128] = False
    M[2] = m[1] | m[2]
    M[3] = R.ellipse(H, W, 0, 30, 90, 70) | R.ellipse(H, W, 255, 255, 60, 120)
    big = R.kinds(1, H, W, 7)
    M[4] = big["comb"][0]
    M[4, 60:190, 70:200] = big["checkerboard"][0, 60:190, 70:200]
    M[5] = big["u_and_ring"][0] | R.ellipse(H, W, 64, 192, 30, 30) & ~R.ellipse(H, W, 64, 192, 20, 20)
    M[6, 3, 250] = M[6, 200, 7] = M[6, 201, 8] = True
    return M


def test_the_mixed_batch_reproducibility_and_logits():
    M = _mixed_batch()
    src = dev(M)
    for conn, fill, min_area, keep, report in ((8, 0, 0, 0, 8), (4, 8, 20, 3, 16), (8, 4, 2, 0, 3)):
        got = check("mixed", M, src, conn, fill, min_area, keep, report)
        for _ in range(3):
            again = abi(src, False, 0.5, conn, fill, min_area, keep, report)
            assert all(torch.equal(a, g) for a, g in zip(again, got))
        # every value at least 0.5 away from the threshold (0 in logits, 0.5 in probabilities)
        g = torch.Generator().manual_seed(9)
        sign = torch.from_numpy(np.where(M, 1.0, -1.0).astype(np.float32))
        logits = (sign * (0.5 + 4.0 * torch.rand(M.shape, generator=g))).to(DEV)
        assert all(torch.equal(a, b) for a, b in zip(abi(logits, True, 0.5, conn, fill, min_area, keep, report), got))
        assert all(torch.equal(a, b) for a, b in zip(abi(torch.sigmoid(logits), False, 0.5, conn, fill, min_area, keep, report), got))
        assert all(torch.equal(a, b) for a, b in zip(abi(src * 0.4 + 0.45, False, 0.65, conn, fill, min_area, keep, report), got))


def _spiral(S):
    """a rectangular spiral, one pixel wide with one-pixel gaps, wound inwards from (0, 0)"""
    m = np.zeros((S, S), dtype=bool)
    y0, x0, y1, x1 = 0, 0, S - 1, S - 1
    m[0, :] = True
    while True:
        m[y0:y1 + 1, x1] = True            # down the right side
        m[y1, x0:x1 + 1] = True            # along the bottom, leftwards
        y0 += 2
        if y1 - y0 < 2:
            break
        m[y0:y1 + 1, x0] = True            # up the left side, to two rows under the previous turn
        x1 -= 2
        if x1 - x0 < 2:
            break
        m[y0, x0:x1 + 1] = True            # along the top, rightwards
        y1 -= 2
        x0 += 2
        if y1 - y0 < 2 or x1 - x0 < 2:
            break
    return m


def test_the_largest_shape_by_closed_form():
    S = 1024
    y, x = np.mgrid[:S, :S]
    serp = (y % 2 == 0) & (y < S - 1) | (y % 4 == 1) & (x == S - 1) & (y < S - 2) | (y % 4 == 3) & (x == 0) & (y < S - 2)
    spiral = _spiral(S)
    for name, m in (("serpentine", serp), ("spiral", spiral)):
        ys, xs = np.nonzero(m)
        area = len(ys)
        if name == "serpentine":
            assert area == 512 * 1024 + 511
        else:
            assert area > S * S // 2 - 4 * S and not (m[1:] & m[:-1] & np.roll(m, 1, 1)[1:] & np.roll(m, 1, 1)[:-1])[:, 1:].any()
        row = [area, 0, 0, 0, int(ys.max()), int(xs.max()), int(ys.sum()), int(xs.sum())]
        for conn in (4, 8):
            mask, lab, out_i, out_c = abi(dev(m[None]), conn=conn, report=2)
            print(name, conn, out_i.cpu().tolist())
            assert out_i.cpu().tolist() == [[area, 0, 1, 1, area, area, 1, 0]], (name, conn)
            assert out_c.cpu().tolist() == [[row, [0] * 8]], (name, conn)
            assert torch.equal(mask[0] == 255, torch.from_numpy(m).to(DEV)) and torch.equal(lab[0] == 1, torch.from_numpy(m).to(DEV))
    # the holes of the serpentine all reach the frame; the spiral's corridor does too
    _, _, out_i, _ = abi(dev(serp[None]), conn=8, fill=4, report=0)
    assert out_i.cpu().tolist() == [[512 * 1024 + 511, 0, 1, 1, 512 * 1024 + 511, 512 * 1024 + 511, 0, 0]]
    checker = (y + x) % 2 == 0
    mask, lab, out_i, out_c = abi(dev(checker[None]), conn=4, report=16)
    assert out_i.cpu().tolist() == [[S * S // 2, 0, S * S // 2, S * S // 2, S * S // 2, 1, 16, 0]]
    assert out_c[0, :, 0].cpu().tolist() == [1] * 16 and out_c[0, :, 1].cpu().tolist() == [2 * k for k in range(16)]      # ties: by first pixel
    assert int(lab.max()) == S * S // 2 and lab[0, S - 1, S - 1] == S * S // 2
    mask, lab, out_i, out_c = abi(dev(checker[None]), conn=8, keep=1, min_area=3, report=1)
    assert out_i.cpu().tolist() == [[S * S // 2, 0, 1, 1, S * S // 2, S * S // 2, 1, 0]]
    mask, lab, out_i, out_c = abi(dev(checker[None]), conn=4, fill=4, keep=5, report=3)      # every white square inside the frame is a hole
    filled = (S - 2) * (S - 2) // 2
    assert out_i.cpu().tolist() == [[S * S // 2, filled, 3, 3, S * S // 2 + filled, S * S // 2 + filled - 2, 3, 0]]


def _png(path, img):
    """8-bit RGB PNG, filter 0 on every row"""
    h, w, _ = img.shape
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
                + chunk(b"IEND", b""))


def _pipeline_models():
    """the closed-form weights at 64 x 64; the classifier's head bias is centred over the batch so that all classes occur"""
    from models.classification_models.ResNet import ResNet18
    from models.segmentation_models.AttentionUNet import AttentionUNet
    from utils.helpers import add_dropout_to_fc
    cls_sd = nets.closed_form_state("ResNet18", head_dropout=True)
    x = torch.randn(16, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        cls_sd["fc.1.bias"] = cls_sd["fc.1.bias"] - nets.NETS["ResNet18"]({k: v.clone() for k, v in cls_sd.items()}, x, False).mean(0)
    cm = ResNet18(num_classes=3)
    add_dropout_to_fc(cm)
    cm.load_state_dict(cls_sd)
    sm = AttentionUNet()
    sm.load_state_dict(nets.closed_form_state("AttentionUNet"))
    cm.compute_dtype = sm.compute_dtype = torch.float32
    return cm, sm, x


def test_joint_pipeline_with_and_without_postprocess(tmp_path):
    import explain_ref
    from utils.pipeline import JointPipeline
    from utils.postprocess import MaskPostprocess
    cm, sm, x = _pipeline_models()
    plain = JointPipeline(cm, sm, device=DEV, bucket=4)
    a = plain.predict(x)
    assert list(a) == ["pred", "confidence", "masks", "segmented"]
    seg = a["segmented"].cpu().numpy()
    assert 2 <= seg.sum() <= len(seg) - 2, "degenerate fixture: the batch must mix COVID and non-COVID predictions"
    again = JointPipeline(cm, sm, device=DEV, bucket=4, postprocess=None).predict(x)
    assert all(torch.equal(a[k], again[k]) for k in a)
    post = MaskPostprocess(connectivity=8, fill_holes=4, min_area=6, keep_largest=4, max_report=5)
    pipe = JointPipeline(cm, sm, device=DEV, bucket=4, postprocess=post)
    b = pipe.predict(x)
    assert list(b) == ["pred", "confidence", "masks", "segmented", "masks_raw", "n_lesions", "area_percent", "lesions"]
    assert all(torch.equal(a[k], b[k]) for k in ("pred", "confidence", "segmented")) and torch.equal(a["masks"], b["masks_raw"])
    raw = b["masks_raw"].cpu().numpy()
    want = R.run(raw > 0, 8, 4, 6, 4, 5)
    assert np.array_equal(b["masks"].cpu().numpy(), want["mask"]) and np.array_equal(b["lesions"].cpu().numpy(), want["out_c"])
    assert np.array_equal(b["n_lesions"].cpu().numpy(), want["out_i"][:, 3])
    assert np.array_equal(b["area_percent"].cpu().numpy(), want["out_i"][:, 4] * (100.0 / (64 * 64)))
    assert (want["out_i"][seg, 2] > want["out_i"][seg, 3]).any(), "the filter removes nothing: the test would not see it"
    assert not b["masks"][~b["segmented"]].any() and not b["n_lesions"][~b["segmented"]].any() and not raw[~seg].any()
    # two PNG files, one of each kind
    imgs = {}
    for name, i in (("covid", int(np.flatnonzero(seg)[0])), ("other", int(np.flatnonzero(~seg)[0]))):
        v = x[i].permute(1, 2, 0).numpy() * np.array([0.229, 0.224, 0.225]) + np.array([0.485, 0.456, 0.406])
        imgs[name] = np.ascontiguousarray((v * 255).round().clip(0, 255).astype(np.uint8))
        _png(str(tmp_path / f"{name}.png"), imgs[name])
    paths = [str(tmp_path / "covid.png"), str(tmp_path / "other.png")]
    got, base = pipe.process_images(paths, size=64), plain.process_images(paths, size=64)
    from utils.dataset import decode_batch, read_files
    from utils.gpu_transforms import SegBatchTransform
    r = pipe.predict(SegBatchTransform(64, train=False, device=DEV)(decode_batch(read_files(paths), 3).to(DEV)))
    for g, p0, row, name in zip(got, base, range(2), ("covid", "other")):
        assert g[:2] == p0[:2] and len(g) == 4
        if bool(r["segmented"][row]):
            line = f"\nLesions: {int(r['n_lesions'][row])} (area {float(r['area_percent'][row]):.2f}% of the image)."
            assert g[3] == p0[3] + line and p0[3].endswith("(segmentation model).")
            assert np.array_equal(g[2], explain_ref.overlay_mask(imgs[name], r["masks"][row].cpu().numpy(), 0.5))
            assert np.array_equal(p0[2], explain_ref.overlay_mask(imgs[name], r["masks_raw"][row].cpu().numpy(), 0.5))
        else:
            assert g[3] == p0[3] and g[2] is None and "Lesions" not in g[3]
    assert any("Lesions: " in g[3] for g in got)
