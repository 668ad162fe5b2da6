"""Generate tests/golden/seg_losses.npz by running the REFERENCE's own ``DiceLoss`` / ``CombinedLoss``
(utils/clip_seg_finetuner.py:40-74 of the reference) in fp64 on the CPU, with autograd for dloss/dlogits.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_seg_loss_golden.py --reference <checkout of the reference>

The reference module imports ``transformers`` at its top, which is not needed by the two loss classes: the file is parsed and
only those two class definitions are compiled and run (with ``torch`` and ``torch.nn`` in scope, as in the file).  The fixture
holds data only — inputs, weights, the recorded loss and gradient of every case — and no text of the reference.  Needs the
reference checkout, so it runs where that exists; no test, smoke() or bench.py imports this script."""
import argparse
import ast
import os

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [(0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.3, 0.7)]
SMOOTH = [1.0, 1e-3]


def reference_classes(ref_root):
    path = os.path.join(ref_root, "utils", "clip_seg_finetuner.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("DiceLoss", "CombinedLoss")]
    assert [n.name for n in keep] == ["DiceLoss", "CombinedLoss"], [n.name for n in keep]
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["DiceLoss"], ns["CombinedLoss"]


def inputs():
    """name -> (logits, target), fp64."""
    rng = np.random.RandomState(20240611)
    out = {}
    for name, shape in (("b1_8x8", (1, 1, 8, 8)), ("b2_16x16", (2, 1, 16, 16)), ("b3_5x7", (3, 1, 5, 7)), ("b2_17x13_3d", (2, 17, 13))):
        z = rng.randn(*shape) * 2.0
        out[name + "_binary"] = (z, (rng.rand(*shape) < 0.35).astype(np.float64))
        out[name + "_soft"] = (z, rng.rand(*shape))
    shape = (2, 1, 8, 8)
    z = rng.randn(*shape) * 2.0
    out["all_zero_target"] = (z, np.zeros(shape))
    out["all_one_target"] = (z, np.ones(shape))
    t = (rng.rand(*shape) < 0.5).astype(np.float64)
    # logits at +-30 (either side of the target) among ordinary ones.  With EVERY logit saturated the gradient is made of
    # sigmoid(30) - 1 = -9.4e-14 and p (1 - p), which fp64 autograd forms as differences of numbers next to 1: the recorded values
    # would carry 1.1e-16 / 9.4e-14 = 1e-3 of rounding and pin nothing.  Next to gradients of ordinary size that is invisible.
    sat = rng.rand(*shape) < 0.5
    out["logits_pm30_among_normal"] = (np.where(sat, np.where(rng.rand(*shape) < 0.5, 30.0, -30.0), z), t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "seg_losses.npz"))
    args = ap.parse_args()
    DiceLoss, CombinedLoss = reference_classes(args.reference)
    store, names = {}, []
    for name, (z, t) in inputs().items():
        store[f"z__{name}"], store[f"t__{name}"] = z, t
        for bw, dw in WEIGHTS:
            for sm in SMOOTH:
                if (bw, dw) == (0.0, 1.0):
                    crit = DiceLoss(smooth=sm)                  # the plain Dice loss is the reference's DiceLoss itself
                else:
                    crit = CombinedLoss(bw, dw)
                    crit.dice.smooth = sm                       # (CombinedLoss builds its DiceLoss with the default)
                zz = torch.from_numpy(z).clone().requires_grad_(True)
                loss = crit(zz, torch.from_numpy(t))
                loss.backward()
                assert loss.dtype == torch.float64 and zz.grad.dtype == torch.float64
                key = f"{name}__bw{bw}__dw{dw}__s{sm}"
                names.append(key)
                store[f"loss__{key}"] = np.float64(loss.item())
                store[f"grad__{key}"] = zz.grad.numpy().copy()
    store["cases"] = np.array(names)
    np.savez_compressed(args.out, **store)
    print(f"{args.out}: {len(names)} cases, {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
