"""Generate tests/golden/lovasz.npz: the Lovasz hinge of Berman, Triki, Blaschko (CVPR 2018), a literal torch-fp64 transcription of
the paper's Algorithm 1 with autograd for dloss/dlogits — errors = 1 - logits * signs, a stable descending sort, the gradient of the
Jaccard loss along it by differencing, dot(relu(errors), grad) — on fp32 inputs.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_lovasz_golden.py

The fixture holds data only: logits, targets, the recorded loss and gradient of every case.  The restatement the tests use
(tests/lovasz_ref.py: closed-form increments, ascending sort of the margins) is written differently on purpose; tests/
test_lovasz_cpu.py pins it to this file.  No test, smoke() or bench.py imports this script."""
import argparse
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 1, 17, 13), (1, 1, 1, 1), (2, 1, 32, 32)]


def lovasz_grad(gt_sorted):
    """Algorithm 1: the gradient of the Jaccard loss with respect to the sorted errors."""
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def lovasz_hinge_flat(logits, labels):
    signs = 2.0 * labels - 1.0
    errors = 1.0 - logits * signs
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
    grad = lovasz_grad(labels[perm])
    return torch.dot(torch.relu(errors_sorted), grad)


def lovasz_hinge(logits, labels, per_image):
    if per_image:
        terms = [lovasz_hinge_flat(z.reshape(-1), t.reshape(-1)) for z, t in zip(logits, labels)]
        return sum(terms) / len(terms)
    return lovasz_hinge_flat(logits.reshape(-1), labels.reshape(-1))


def inputs():
    """name -> (logits fp32, target fp32 in {0, 1})."""
    rng = np.random.RandomState(20181218)
    out = {}
    for shape in SHAPES:
        tag = "x".join(map(str, shape))
        z = (rng.randn(*shape) * 2.0).astype(np.float32)
        t = (rng.rand(*shape) < 0.35).astype(np.float32)
        out[f"{tag}_random"] = (z, t)
        out[f"{tag}_quantised"] = ((np.round(rng.randn(*shape) * 4.0) / 4.0).astype(np.float32), t)      # multiples of 0.25: ties
        if z.size < 1024:                                   # (the fixture stays below 100 KB)
            out[f"{tag}_all_zero_target"] = (z, np.zeros(shape, dtype=np.float32))
            out[f"{tag}_all_one_target"] = (z, np.ones(shape, dtype=np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "lovasz.npz"))
    args = ap.parse_args()
    store, names = {}, []
    for name, (z, t) in inputs().items():
        store[f"z__{name}"], store[f"t__{name}"] = z, t.astype(np.uint8)
        for per_image in (True, False):
            zz = torch.from_numpy(z).double().requires_grad_(True)
            loss = lovasz_hinge(zz, torch.from_numpy(t).double(), per_image)
            loss.backward()
            assert loss.dtype == torch.float64 and zz.grad.dtype == torch.float64
            key = f"{name}__{'image' if per_image else 'batch'}"
            names.append(key)
            store[f"loss__{key}"] = np.float64(loss.item())
            store[f"grad__{key}"] = zz.grad.numpy().copy()
    store["cases"] = np.array(names)
    np.savez_compressed(args.out, **store)
    print(f"{args.out}: {len(names)} cases, {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
