"""Bootstrap intervals and DeLong's components (csrc/resample.hip, utils/resample.py) against the eval forward they follow and against
the host route an evaluation kit takes without them; one JSON line.

    timeout -k 10 600 python scripts/resample_time.py

Classifier workload (4096 x 3 scores, R = 2000 replicates): ``forward_bs32_256_ms`` = ResNet18 eval forward (bf16) of 32 256^2 images
for scale; ``counts_ms`` / ``confusion_ms`` / ``rank_ms`` / ``interval_ms`` / ``delong_ms`` = the calls the tester makes under ``ci``
(weights, weighted confusion matrices and the four figures formed from them, the weighted ranking metrics of the three classes, the
percentile intervals of 4 + 2 + 3 statistics, DeLong's components), ``ci_total_ms`` = all of them in one timed region; ``host_ms`` =
the same replicates on the host: the weights copied back, a numpy loop over sklearn.metrics.roc_auc_score(sample_weight=...) per
class and np.nanquantile (wall clock, --host-iters runs).  Segmenter workload (12 per-image values of 256 images, R = 2000):
``means_ms`` + ``interval_ms`` against a numpy loop of weighted nan-means.  Device times are CUDA-event medians (min .. max) after
--warmup calls; ``max_diff_vs_host`` = the largest difference between the two routes' interval ends."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "medical-image-segmentation-and-classification_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.classification_models.ResNet import ResNet18  # noqa: E402
from utils import ranking, resample  # noqa: E402


def times_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def host_ms(fn, iters):
    ts, out = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--replicates", type=int, default=2000)
    a = ap.parse_args()
    try:
        import sklearn
        from sklearn import metrics
        sk_version = sklearn.__version__
    except ImportError:
        metrics, sk_version = None, None
        print("scikit-learn does not import here: the host route is not timed", file=sys.stderr)
    R, lo_q, hi_q = a.replicates, 0.025, 0.975
    res = {"replicates": R, "sklearn": sk_version}
    with torch.no_grad():
        cls = ResNet18(num_classes=3)
        cls.compute_dtype = torch.bfloat16
        cls = cls.cuda().eval()
        xc = torch.randn(32, 3, 256, 256, generator=torch.Generator().manual_seed(3)).cuda()
        N, C = 4096, 3
        z = (torch.randn(N, C, generator=torch.Generator().manual_seed(4)) * 2).cuda()
        y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(5)).to(torch.int32).cuda()
        z[torch.arange(N), y.long()] += 1.5                                   # a classifier that is right more often than not
        scores_t = ranking.calibration(z, y)["scores_t"]
        pred = z.argmax(1).to(torch.int32)

        def device_route():
            counts = resample.bootstrap_counts(N, R, 0, device=z.device)
            cm, _ = resample.boot_confusion(pred, y, C, counts)
            m = resample.classification_from_confusion(cm)
            rk = resample.boot_rank_metrics(scores_t, counts, labels=y)
            reps = torch.stack([m["accuracy"], m["precision"], m["recall"], m["f1"], rk["auroc"].mean(1), rk["average_precision"].mean(1)]
                               + list(rk["auroc"].unbind(1)), 1)
            return resample.interval(reps, 0.95), resample.delong(scores_t, y)

        counts = resample.bootstrap_counts(N, R, 0, device=z.device)
        cm, _ = resample.boot_confusion(pred, y, C, counts)
        reps = torch.rand(R + 1, 9, dtype=torch.float64, device=z.device)
        for _ in range(a.warmup):
            cls(xc)
            device_route()
        torch.cuda.synchronize()
        w = {"N": N, "C": C, "forward_bs32_256_ms": times_ms(lambda: cls(xc), a.iters),
             "counts_ms": times_ms(lambda: resample.bootstrap_counts(N, R, 0, device=z.device), a.iters),
             "confusion_ms": times_ms(lambda: resample.classification_from_confusion(resample.boot_confusion(pred, y, C, counts)[0]), a.iters),
             "rank_ms": times_ms(lambda: resample.boot_rank_metrics(scores_t, counts, labels=y), a.iters),
             "interval_ms": times_ms(lambda: resample.interval(reps, 0.95), a.iters),
             "delong_ms": times_ms(lambda: resample.delong(scores_t, y), a.iters),
             "ci_total_ms": times_ms(device_route, a.iters)}
        iv, _ = device_route()
        got = torch.stack([iv["lo"][6:], iv["hi"][6:]], 1).cpu().numpy()       # the per-class ROC-AUC intervals
        w["auroc_class0_ci"] = [round(float(v), 6) for v in got[0]]
        if metrics is not None:
            def host_cls():
                cw, p, yy = counts.cpu().numpy(), scores_t.cpu().numpy(), y.cpu().numpy()
                auc = np.array([[metrics.roc_auc_score(yy == c, p[c], sample_weight=cw[r]) for c in range(C)] for r in range(1, R + 1)])
                return np.stack([np.nanquantile(auc, lo_q, axis=0), np.nanquantile(auc, hi_q, axis=0)], 1)
            w["host_ms"], ref = host_ms(host_cls, a.host_iters)
            w["host_over_device"] = round(w["host_ms"] / (w["counts_ms"]["median"] + w["rank_ms"]["median"] + w["interval_ms"]["median"]), 1)
            w["max_diff_vs_host"] = float(np.abs(got - ref).max())
        res["classifier"] = w

        M, n = 12, 256
        v = torch.rand(M, n, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
        v[6:, ::17] = float("nan")                                            # samples without surface distances
        v = v.cuda()
        cs = resample.bootstrap_counts(n, R, 0, device=v.device)
        seg_route = lambda: resample.interval(resample.boot_means(v, cs), 0.95)      # noqa: E731
        for _ in range(a.warmup):
            seg_route()
        torch.cuda.synchronize()
        s = {"M": M, "n": n, "means_ms": times_ms(lambda: resample.boot_means(v, cs), a.iters),
             "ci_total_ms": times_ms(lambda: (resample.bootstrap_counts(n, R, 0, device=v.device), seg_route()), a.iters)}
        iv = seg_route()
        got = torch.stack([iv["lo"], iv["hi"]], 1).cpu().numpy()

        def host_seg():
            cw, vv = cs.cpu().numpy().astype(np.float64), v.cpu().numpy()
            ok = ~np.isnan(vv)
            means = np.array([[(cw[r][ok[m]] * vv[m][ok[m]]).sum() / cw[r][ok[m]].sum() for m in range(M)] for r in range(1, R + 1)])
            return np.stack([np.nanquantile(means, lo_q, axis=0), np.nanquantile(means, hi_q, axis=0)], 1)
        s["host_ms"], ref = host_ms(host_seg, max(a.host_iters, 3))
        s["host_over_device"] = round(s["host_ms"] / s["ci_total_ms"]["median"], 1)
        s["max_diff_vs_host"] = float(np.abs(got - ref).max())
        res["segmenter"] = s
    print(json.dumps(res))


if __name__ == "__main__":
    main()
