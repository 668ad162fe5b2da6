"""CPU: the host-side convolution dispatch (csrc/conv_igemm.hip choose, csrc/conv_wgrad.hip wgrad3_mode) pinned against
tests/golden/conv_dispatch.npz, the table scripts/dispatch_table.py recorded before the decision became one function: variant,
tile and statistics-row answers over a grid of shapes, under the default switches and under each A/B switch.  Without a device
the queries assume 256 CUs.  The kernel-name queries are checked against the rules bench.py's per-kernel table was built on,
kept here as their specification."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mi355.lib import lib, available, SO_PATH, REPO_ROOT

pytestmark = pytest.mark.skipif(not available(), reason="libmi355conv.so not built")

GOLDEN = os.path.join(REPO_ROOT, "tests", "golden", "conv_dispatch.npz")
SCRIPT = os.path.join(REPO_ROOT, "scripts", "dispatch_table.py")
HALO_FAMILY = {2, 3, 5, 6, 7, 8}
F32 = 0


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_library_reproduces_every_recorded_table(golden, tmp_path):
    """The switches are read once per process: the generator computes each table in a fresh child of its own."""
    out = str(tmp_path / "now.npz")
    subprocess.run([sys.executable, SCRIPT, out], check=True, env=dict(os.environ, MI355_LIB=SO_PATH))
    now = np.load(out)
    assert sorted(now.files) == sorted(golden) and len(golden) == 11
    for key in sorted(golden):
        diff = np.flatnonzero((now[key] != golden[key]).any(axis=0)) if now[key].shape == golden[key].shape else None
        assert diff is not None and diff.size == 0, (key, now[key].shape, golden[key].shape, None if diff is None else
                                                     [(golden["rows_default" if key == "default" else "rows_thin"][:, i].tolist(),
                                                       golden[key][:, i].tolist(), now[key][:, i].tolist()) for i in diff[:3]])


def igemm_name_spec(N, Hi, Wi, ci, Ho, Wo, co, k, mul, kmul, off, div, up, code):
    """The kernel names as mi355/graph.py derived them from the queries before the library named its kernels itself."""
    if code == F32:
        return f"conv_igemm_kernel<f32,{lib.mi355_conv2d_igemm_generic_tile(N, Ho, Wo, co)},16>"
    v = lib.mi355_conv2d_igemm_variant_n(N, Hi, Wi, ci, Ho, Wo, co, k, k, mul, kmul, off, div, up, code)
    k64 = ci % 64 == 0
    if v == 0:
        return f"conv_igemm_kernel<bf16,{lib.mi355_conv2d_igemm_generic_tile(N, Ho, Wo, co)},{64 if k64 else 32}>"
    if v == 1:
        bn = lib.mi355_conv2d_igemm_dma_tile(N, Ho, Wo, ci, co)
        if bn == 128:
            return "conv_igemm_dma_kernel<128,64,2>" if k64 else "conv_igemm_dma_kernel<128,32,3>"
        return "conv_igemm_dma_kernel<64,32,3>" if bn == 64 else "conv_igemm_dma_kernel<32,64,3>"
    return {2: "conv3x3_halo_rw_kernel<8,32>", 3: "conv3x3_halo_rw_kernel<16,16>", 4: f"conv1x1_stream_kernel<{ci},{co}>",
            5: "conv3x3_halo_pp_kernel", 6: "conv3x3_halo_pp128_kernel", 7: "conv3x3_ws_kernel<64,8>", 8: "conv3x3_ws_kernel<128,4>",
            9: "conv_gemm256_kernel"}[v]


def wgrad_name_spec(N, Ho, Wo, ci, co, k, s, p, code):
    t = "f32" if code == F32 else "bf16"       # (the fp16 build runs the same variants as bf16)
    v = lib.mi355_conv2d_wgrad_variant(N, Ho, Wo, k, k, s, p, code) if t == "bf16" else 0
    if v:
        return "wgrad3x3_halo8_kernel" if v >= 3 else "wgrad3x3_halo_kernel"
    return f"conv_wgrad_kernel<{t},{128 if co % 128 == 0 else 64},{128 if ci % 128 == 0 else 64}>"


def test_pool2_and_kernel_names_follow_the_launcher(golden):
    """On every row of the default grid: the 2x2-sum epilogue exists exactly for the halo family (never for fp32), and the two
    name queries give the names the per-kernel table has always used."""
    seen = set()
    for r in golden["rows_default"].T.tolist():
        N, Hi, Wi, Ci, Ho, Wo, Co, KH, KW, mul, kmul, off, div, up, dt, wHo, wWo, stride, pad = r
        geom = r[:15]
        v = lib.mi355_conv2d_igemm_variant_n(*geom)
        assert lib.mi355_conv2d_igemm_pool2_ok(*geom) == (1 if v in HALO_FAMILY else 0), geom
        assert dt != F32 or lib.mi355_conv2d_igemm_pool2_ok(*geom) == 0, geom
        name = lib.mi355_conv2d_igemm_kernel_name(*geom).decode()
        assert name == igemm_name_spec(N, Hi, Wi, Ci, Ho, Wo, Co, KH, mul, kmul, off, div, up, dt), geom
        wname = lib.mi355_conv2d_wgrad_kernel_name(N, wHo, wWo, Ci, Co, KH, KW, stride, pad, dt).decode()
        assert wname == wgrad_name_spec(N, wHo, wWo, Ci, Co, KH, stride, pad, dt), r
        seen.update((name.split("<")[0], wname.split("<")[0]))
    assert {"conv_igemm_kernel", "conv_igemm_dma_kernel", "conv3x3_halo_rw_kernel", "conv1x1_stream_kernel", "conv3x3_halo_pp128_kernel",
            "conv3x3_ws_kernel", "conv_gemm256_kernel", "wgrad3x3_halo_kernel", "wgrad3x3_halo8_kernel", "conv_wgrad_kernel"} <= seen
