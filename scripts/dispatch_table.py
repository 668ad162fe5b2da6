#!/usr/bin/env python3
"""Table of the host-side convolution dispatch: which kernel, tile and statistics-row count mi355_conv2d_igemm and
mi355_conv2d_wgrad choose over a fixed grid of shapes (no device needed: the queries assume 256 CUs without one).

    MI355_LIB=/path/to/libmi355conv.so python scripts/dispatch_table.py tests/golden/conv_dispatch.npz

writes the fixture tests/test_dispatch_cpu.py pins the library against (arrays of [column][row]: IN_COLS for rows_*, OUT_COLS
for the tables); generate it from the build whose decisions are to be kept.  The MI355_* switches are read once per process,
so the default table and one thinned table per switch are each computed in a fresh child of this script.  Plain ctypes, no
torch: a child starts in a fraction of a second."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "medical-image-segmentation-and-classification_amd", "mi355", "libmi355conv.so")
SWITCHES = ("MI355_IGEMM_VARIANT=0", "MI355_HALO_PP=1", "MI355_HALO_PP128=0", "MI355_WS64=0", "MI355_WS128=0", "MI355_GEMM256=0",
            "MI355_DMA_SMALLGRID=0", "MI355_WGRAD_HALO=0")
F32, BF16, F16 = 0, 1, 2
# columns of a row: the 15 arguments of mi355_conv2d_igemm_variant_n, then the layer the weight gradient is asked about
IN_COLS = ("N", "Hi", "Wi", "Ci", "Ho", "Wo", "Co", "KH", "KW", "mul", "kmul", "off", "div", "up", "dtype", "wHo", "wWo", "stride", "pad")
OUT_COLS = ("variant", "variant_n", "stat_rows", "dma_tile", "generic_tile", "wgrad_variant", "wgrad_multi_ok", "wgrad_splits")


def geometries(H, W):
    """(Hi, Wi, Ho, Wo, k, mul, kmul, off, div, up, wHo, wWo, stride, pad) of every launch form mi355/graph.py emits."""
    h2, w2 = H // 2, W // 2
    return [
        (H, W, H, W, 3, 1, 1, -1, 1, 0, H, W, 1, 1),                # 3x3 s1 p1 forward
        (H, W, H, W, 3, 1, -1, 1, 1, 0, H, W, 1, 1),                # ... its data gradient
        (H, W, 2 * H, 2 * W, 3, 1, 1, -1, 1, 1, 2 * H, 2 * W, 1, 1),  # 3x3 on a nearest-x2 up-sampled input
        (H, W, h2, w2, 3, 2, 1, -1, 1, 0, h2, w2, 2, 1),            # 3x3 s2 p1 forward
        (h2, w2, H, W, 3, 1, -1, 1, 2, 0, h2, w2, 2, 1),            # ... its data gradient
        (H, W, H, W, 1, 1, 1, 0, 1, 0, H, W, 1, 0),                 # 1x1 s1
        (H, W, h2, w2, 1, 2, 1, 0, 1, 0, h2, w2, 2, 0),             # 1x1 s2
        (H, W, h2, w2, 2, 2, 1, 0, 1, 0, h2, w2, 2, 0),             # 2x2 s2
        (H, W, 2 * H, 2 * W, 2, 1, -1, 0, 2, 0, H, W, 2, 0),        # ConvTranspose2d(2, 2) forward (data-gradient form)
        (H, W, h2, w2, 7, 2, 1, -3, 1, 0, h2, w2, 2, 3),            # 7x7 s2 p3 stem
    ]


def grid(thin=False):
    batches = (2, 32) if thin else (1, 2, 16, 32)
    chans = (64, 128, 256, 512) if thin else (32, 64, 96, 128, 256, 512, 1024)
    extents = [(e, e) for e in (8, 16, 32, 64, 128, 256)] + [(32, 64), (24, 40)]
    rows = []
    for N in batches:
        for H, W in extents:
            for g in geometries(H, W):
                Hi, Wi, Ho, Wo, k, mul, kmul, off, div, up, *wg = g
                for Ci in chans:
                    for Co in chans:
                        for dt in (F32, BF16, F16):
                            rows.append((N, Hi, Wi, Ci, Ho, Wo, Co, k, k, mul, kmul, off, div, up, dt, *wg))
    # an image of 2 GiB: the buffer-descriptor kernels hand over to the LDS-DMA ring kernel
    rows.append((1, 4096, 4096, 64, 4096, 4096, 64, 3, 3, 1, 1, -1, 1, 0, BF16, 4096, 4096, 1, 1))
    return np.asarray(rows, dtype=np.int32)


def table(dll, rows):
    out = np.empty((len(rows), len(OUT_COLS)), dtype=np.int32)
    for i, r in enumerate(rows.tolist()):
        N, Hi, Wi, Ci, Ho, Wo, Co, KH, KW, mul, kmul, off, div, up, dt, wHo, wWo, stride, pad = r
        geom = r[1:15]
        out[i] = (dll.mi355_conv2d_igemm_variant(*geom), dll.mi355_conv2d_igemm_variant_n(N, *geom),
                  dll.mi355_conv2d_igemm_stat_rows(N, *geom), dll.mi355_conv2d_igemm_dma_tile(N, Ho, Wo, Ci, Co),
                  dll.mi355_conv2d_igemm_generic_tile(N, Ho, Wo, Co), dll.mi355_conv2d_wgrad_variant(N, wHo, wWo, KH, KW, stride, pad, dt),
                  dll.mi355_conv2d_wgrad_multi_ok(N, wHo, wWo, dt), dll.mi355_conv2d_wgrad_splits(N, wHo, wWo, Ci, Co, KH, KW))
    return out


def key_of(switch):
    return switch.replace("=", "_") if switch else "default"


def child(switch, path):
    dll = ctypes.CDLL(os.environ.get("MI355_LIB") or DEFAULT_LIB)
    np.save(path, table(dll, grid(thin=bool(switch))))


def generate(out_path):
    arrays = {"rows_default": grid(False), "rows_thin": grid(True)}
    base = {k: v for k, v in os.environ.items() if not k.startswith("MI355_") or k == "MI355_LIB"}
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for sw in ("",) + SWITCHES:
            path = os.path.join(tmp, key_of(sw) + ".npy")
            env = dict(base, **dict([sw.split("=")])) if sw else base
            jobs.append((sw, path, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", sw, path], env=env)))
        for sw, path, proc in jobs:
            if proc.wait() != 0:
                raise SystemExit(f"child for {key_of(sw)} failed")
            arrays[key_of(sw)] = np.load(path)
    d = arrays["default"]
    variants = set(np.unique(np.concatenate([arrays[key_of(sw)][:, 1] for sw in ("",) + SWITCHES])).tolist())
    modes = set(np.unique(d[:, 5]).tolist())
    assert variants == set(range(10)), f"igemm variants in the tables: {sorted(variants)}"
    assert modes == set(range(5)), f"wgrad modes in the default table: {sorted(modes)}"
    assert d[-1, 0] >= 2 and d[-1, 1] == 1, "the 2 GiB image must fall back from a halo kernel to the LDS-DMA ring kernel"
    # one row of the file per column of the table: runs of equal values, a fifth of the size of the row-major layout
    np.savez_compressed(out_path, **{k: np.ascontiguousarray(v.T) for k, v in arrays.items()})
    print(f"{out_path}: {len(d)} default rows, {len(arrays['rows_thin'])} rows per switch, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 2:
        generate(sys.argv[1])
    else:
        raise SystemExit(__doc__)
