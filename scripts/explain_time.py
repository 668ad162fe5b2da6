"""Eval forward vs GradCAM (utils/explain.py) of one classifier: bs 32, 256^2, bf16 by default; one JSON line.

    timeout -k 10 300 python scripts/explain_time.py --model ResNet50
    timeout -k 10 300 python scripts/explain_time.py --model VGG16_BN

Times are CUDA-event medians over --iters calls after --warmup calls (one call = one forward, or one forward + seed + head
backward + Grad-CAM + the resize to 256^2); ``extra`` is what the explanation adds to the eval forward."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import torch  # noqa: E402

from models.classification_models.ResNet import ResNet50  # noqa: E402
from models.classification_models.VGG import VGG16_BN  # noqa: E402
from utils.explain import GradCAM  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def med_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("ResNet50", "VGG16_BN"), default="ResNet50")
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=tuple(DTYPES), default="bf16")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    m = {"ResNet50": ResNet50, "VGG16_BN": VGG16_BN}[a.model](num_classes=3)
    m.compute_dtype = DTYPES[a.dtype]
    m = m.cuda().eval()
    x = torch.randn(a.bs, 3, a.size, a.size, generator=torch.Generator().manual_seed(0)).cuda()
    cam = GradCAM(m)
    with torch.no_grad():
        for _ in range(a.warmup):
            m(x)
            cam(x)
        torch.cuda.synchronize()
        fwd = med_ms(lambda: m(x), a.iters)
        exp = med_ms(lambda: cam(x), a.iters)
    print(json.dumps({"model": a.model, "bs": a.bs, "size": a.size, "dtype": a.dtype, "eval_forward_ms": round(fwd, 3),
                      "gradcam_ms": round(exp, 3), "extra_ms": round(exp - fwd, 3), "extra_pct": round(100 * (exp - fwd) / fwd, 2)}))


if __name__ == "__main__":
    main()
