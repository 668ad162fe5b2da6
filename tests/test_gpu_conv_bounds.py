"""-m gpu: every convolution kernel variant against an fp64 reference with PER-ELEMENT error bounds (tests/conv_bounds.py):
|y - M(Y)| <= r_T + C * sqrt(K) * 2^-24 * sum|a * b|, plus an RMS / mean-signed-error check in ulps for 2-byte outputs and an
fp32-summation bound on the fused BatchNorm statistics.  Every case asserts the variant that serves it before it launches;
variants reachable only under a dispatch switch run in a child pytest process (the switches are read once per process), and the
last test asserts that every forward variant and every weight-gradient mode ran, and prints the per-variant table."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import conv_bounds as cb
from gpu_util import DEV, lib, to_nhwc, from_nhwc, pack_w, DTYPE_CODE

pytestmark = pytest.mark.gpu
BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32

# the child run this process is ("" = the parent, default dispatch); its switch and the JSON-lines file results go to
SWITCHES = {
    "pp": {"MI355_HALO_PP": "1"},
    "pp128": {"MI355_HALO_PP128_MINCI": "64", "MI355_PP128_FILL": "0"},      # (FILL=0: no fall-back on a grid short of a round)
    "ws": {"MI355_WS64_MIN_TILES": "1"},
    "smallgrid0": {"MI355_DMA_SMALLGRID": "0"},
    "gemm256": {"MI355_GEMM256_MIN_TILES": "1"},
    "generic": {"MI355_IGEMM_VARIANT": "0"},
    "wgrad8off": {"MI355_WGRAD8": "0"},
    "wgradhalo0": {"MI355_WGRAD_HALO": "0"},
}
HERE = os.environ.get("MI355_BOUNDS_SWITCH", "")
REPORT = os.environ.get("MI355_BOUNDS_REPORT", "")
RESULTS = []          # this process's rows: dict(kind, variant, dtype, epi, ratio, rms, mean)


def _record(kind, variant, dtype, epi, rep):
    row = dict(kind=kind, variant=int(variant), dtype=str(dtype).split(".")[-1], epi=epi, ratio=rep.ratio,
               rms=rep.rms, mean=rep.mean, switch=HERE)
    RESULTS.append(row)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(row) + "\n")
    extra = f", RMS {rep.rms:.3f} ulp (limit {rep.rms_lim:.3f}), mean {rep.mean:+.4f}" if rep.rms is not None else ""
    print(f"  [{kind} v{variant} {row['dtype']} {epi}] max err/bound {rep.ratio:.3f}{extra}")


# ---- forward / data gradient / ConvTranspose2d / 2x2-sum cases --------------------------------------------------------------------
# (name, kind, N, ci, H, W, co, k, stride, pad, up, switch, variant of the 2-byte types, images checked (None = all))
# kind: fwd = conv(ci -> co) on H x W; dgrad = its data gradient (co-channel gradient in, ci-channel gradient out); convT =
# ConvTranspose2d(ci -> co, 2, 2) of an H x W input; pool2 = the data gradient of conv(up2(x)) summed over 2 x 2 groups (x is H x W)
FCASES = [
    # generic register-staged kernel (2-byte: Co % 64 and Ci % 64 both non-zero; fp32 serves everything)
    ("gen_9x7", "fwd", 1, 32, 9, 7, 32, 3, 1, 1, 0, "", 0, None),
    ("gen_tail", "fwd", 2, 96, 10, 10, 160, 3, 1, 1, 0, "", 0, None),
    # LDS-DMA ring: stride 2, 7x7 stem, images off the halo tiles, data gradients of stride 2
    ("dma_s2", "fwd", 2, 32, 16, 16, 64, 3, 2, 1, 0, "", 1, None),
    ("dma_7x7", "fwd", 2, 32, 20, 20, 64, 7, 2, 3, 0, "", 1, None),
    ("dma_12x20", "fwd", 1, 128, 12, 20, 64, 3, 1, 1, 0, "", 1, None),
    ("dma_dgrad_s2", "dgrad", 2, 32, 16, 16, 64, 3, 2, 1, 0, "", 1, None),
    # four-wave halo kernels: 8 x 32 (odd / even slab counts, several tiles per image, up = 1) and 16 x 16
    ("halo8_odd", "fwd", 2, 96, 16, 64, 64, 3, 1, 1, 0, "", 2, None),
    ("halo8_up", "fwd", 2, 64, 8, 16, 128, 3, 1, 1, 1, "", 2, None),
    ("halo8_dgrad", "dgrad", 2, 128, 16, 32, 64, 3, 1, 1, 0, "", 2, None),
    ("halo8_pool2", "pool2", 2, 64, 8, 16, 128, 3, 1, 1, 0, "", 2, None),
    ("halo16", "fwd", 2, 64, 16, 16, 64, 3, 1, 1, 0, "", 3, None),
    ("halo16_dgrad", "dgrad", 2, 64, 16, 16, 128, 3, 1, 1, 0, "", 3, None),
    ("halo16_pool2", "pool2", 1, 64, 8, 8, 64, 3, 1, 1, 0, "", 3, None),
    # streaming pointwise kernel: ragged pixel counts
    ("stream_189", "fwd", 3, 64, 9, 7, 128, 1, 1, 0, 0, "", 4, None),
    ("stream_1480", "fwd", 1, 128, 40, 37, 64, 1, 1, 0, 0, "", 4, None),
    ("stream_dgrad", "dgrad", 3, 128, 9, 7, 64, 1, 1, 0, 0, "", 4, None),
    # weight-stationary Ci = 64 at its default threshold: 288 tiles x 4 channel tiles over 512 persistent workgroups (uneven ranges)
    ("ws64_default", "fwd", 36, 64, 32, 64, 256, 3, 1, 1, 0, "", 7, None),
    # padding-free GEMM kernel at its default threshold (>= 128 tiles of 256 rows)
    ("gemm_1x1", "fwd", 8, 128, 32, 32, 512, 1, 1, 0, 0, "", 9, None),
    ("gemm_convT", "convT", 16, 64, 32, 32, 128, 2, 2, 0, 0, "", 9, None),
    # benchmark shapes (images 0, 15 and 31 checked)
    ("bench_ws64", "fwd", 32, 64, 256, 256, 64, 3, 1, 1, 0, "", 7, (0, 15, 31)),
    ("bench_pp128", "fwd", 32, 512, 32, 32, 512, 3, 1, 1, 0, "", 6, (0, 15, 31)),
    # --- MI355_HALO_PP=1: the 64-channel ping-pong halo kernel (one / three slabs, several tiles, up = 1, 2x2 sums)
    ("pp_1slab", "fwd", 1, 32, 16, 32, 64, 3, 1, 1, 0, "pp", 5, None),
    ("pp_3slab", "fwd", 2, 96, 32, 64, 64, 3, 1, 1, 0, "pp", 5, None),
    ("pp_up", "fwd", 2, 64, 8, 16, 64, 3, 1, 1, 1, "pp", 5, None),
    ("pp_dgrad", "dgrad", 1, 64, 16, 32, 128, 3, 1, 1, 0, "pp", 5, None),
    ("pp_pool2", "pool2", 1, 128, 8, 16, 64, 3, 1, 1, 0, "pp", 5, None),
    # --- MI355_HALO_PP128_MINCI=64: the 128-channel ping-pong kernel on small shapes (two / four slabs, two channel tiles)
    ("pp128_2slab", "fwd", 2, 64, 16, 32, 256, 3, 1, 1, 0, "pp128", 6, None),
    ("pp128_4slab", "fwd", 1, 128, 32, 64, 128, 3, 1, 1, 0, "pp128", 6, None),
    ("pp128_up", "fwd", 2, 64, 8, 16, 128, 3, 1, 1, 1, "pp128", 6, None),
    ("pp128_dgrad", "dgrad", 1, 128, 16, 32, 128, 3, 1, 1, 0, "pp128", 6, None),
    ("pp128_pool2", "pool2", 1, 128, 8, 16, 128, 3, 1, 1, 0, "pp128", 6, None),
    # --- MI355_WS64_MIN_TILES=1: weight-stationary kernels on small shapes (at least 8 spatial tiles: the launcher's floor; one tile
    #     per workgroup, uneven ranges, 2x2 sums)
    ("ws64_small", "fwd", 2, 64, 32, 32, 64, 3, 1, 1, 0, "ws", 7, None),
    ("ws64_uneven", "fwd", 3, 64, 8, 96, 128, 3, 1, 1, 0, "ws", 7, None),
    ("ws64_up", "fwd", 2, 64, 16, 16, 64, 3, 1, 1, 1, "ws", 7, None),
    ("ws64_pool2", "pool2", 2, 64, 16, 16, 64, 3, 1, 1, 0, "ws", 7, None),
    ("ws128_small", "fwd", 2, 128, 16, 32, 128, 3, 1, 1, 0, "ws", 8, None),
    ("ws128_3ct", "fwd", 1, 128, 16, 64, 192, 3, 1, 1, 0, "ws", 8, None),
    ("ws128_dgrad", "dgrad", 2, 64, 16, 32, 128, 3, 1, 1, 0, "ws", 8, None),
    ("ws128_pool2", "pool2", 2, 128, 8, 16, 128, 3, 1, 1, 0, "ws", 8, None),
    # --- MI355_DMA_SMALLGRID=0: the ring kernel's 128- / 64-wide tiles on small grids
    ("dma_wide128", "fwd", 2, 64, 12, 20, 128, 3, 1, 1, 0, "smallgrid0", 1, None),
    ("dma_wide_1x1", "fwd", 2, 128, 8, 8, 256, 1, 1, 0, 0, "smallgrid0", 1, None),
    ("dma_wide64_s2", "fwd", 2, 96, 16, 16, 64, 3, 2, 1, 0, "smallgrid0", 1, None),
    # --- MI355_GEMM256_MIN_TILES=1: the GEMM kernel's 1x1 / stride 2, 2x2 / stride 2 and ConvTranspose2d phases on few tiles
    ("gemm_1x1s2", "fwd", 2, 64, 32, 32, 128, 1, 2, 0, 0, "gemm256", 9, None),
    ("gemm_2x2s2", "fwd", 2, 64, 32, 32, 128, 2, 2, 0, 0, "gemm256", 9, None),
    ("gemm_convT_small", "convT", 2, 64, 8, 16, 128, 2, 2, 0, 0, "gemm256", 9, None),
    ("gemm_dgrad_2x2", "dgrad", 2, 128, 32, 32, 64, 2, 2, 0, 0, "gemm256", 9, None),
    # --- MI355_IGEMM_VARIANT=0: the generic kernel for 2-byte types on shapes the other kernels own
    ("gen_forced_halo", "fwd", 2, 64, 16, 32, 128, 3, 1, 1, 0, "generic", 0, None),
    ("gen_forced_s2", "fwd", 2, 64, 12, 12, 64, 3, 2, 1, 0, "generic", 0, None),
    ("gen_forced_dgrad", "dgrad", 2, 64, 16, 16, 128, 3, 1, 1, 0, "generic", 0, None),
]


def _geometry(case):
    """-> ABI arguments of the igemm call: (Hi, Wi, Cin, Ho, Wo, Cout, KH, KW, mul, kmul, off, div, up, pool)"""
    _, kind, n, ci, h, w_, co, k, s, p, up, *_ = case
    if kind == "fwd":
        hl, wl = (2 * h, 2 * w_) if up else (h, w_)
        return h, w_, ci, (hl + 2 * p - k) // s + 1, (wl + 2 * p - k) // s + 1, co, k, k, s, 1, -p, 1, up, 0
    if kind == "dgrad":
        ho, wo = (h + 2 * p - k) // s + 1, (w_ + 2 * p - k) // s + 1
        return ho, wo, co, h, w_, ci, k, k, 1, -1, p, s, 0, 0
    if kind == "convT":
        return h, w_, ci, 2 * h, 2 * w_, co, 2, 2, 1, -1, 0, 2, 0, 0
    if kind == "pool2":
        return 2 * h, 2 * w_, co, 2 * h, 2 * w_, ci, 3, 3, 1, -1, 1, 1, 0, 1
    raise ValueError(kind)


def _operands(case, dtype):
    """CPU fp32 operands, the fp64 pre-epilogue result z (conv + bias) and its magnitude a at the accumulation resolution (NCHW,
    restricted to the checked images), K, the device input (NHWC) and packed weights"""
    name, kind, n, ci, h, w_, co, k, s, p, up, _, _, imgs = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    sel = list(imgs) if imgs else list(range(n))
    if kind in ("fwd", "convT"):
        x = torch.randn(n, ci, h, w_, generator=g)
        if kind == "fwd":
            w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
            op = {"kind": "fwd", "stride": s, "pad": p, "up": up}
            wk, _ = pack_w(w, dtype)
            kk = ci * k * k + 1
        else:
            w = torch.randn(ci, co, 2, 2, generator=g) / ci ** 0.5
            op = {"kind": "convT", "stride": 2}
            wk, _ = pack_w(w, dtype, transposed=True)
            kk = ci + 1
        b = torch.randn(co, generator=g)
        z = cb.ref64(op, x[sel], w, b, dtype)
        a = cb.mag64(op, x[sel], w, b, dtype)
        z32 = cb._op64(op, cb.rnd(x[sel], dtype).float(), cb.rnd(w, dtype).float(), b, None).double()
        return x, wk, b, z, a, kk, z32
    # data gradients: dy on the layer's output grid, weights [co][ci][k][k] in the Wb pack
    hl, wl = (2 * h, 2 * w_) if kind == "pool2" else (h, w_)
    ho, wo = (hl + 2 * p - k) // s + 1, (wl + 2 * p - k) // s + 1
    dy = torch.randn(n, co, ho, wo, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (co * k * k) ** 0.5
    _, wk = pack_w(w, dtype)
    op = {"kind": "dgrad", "stride": s, "pad": p}
    z = cb.ref64(op, dy[sel], w, None, dtype, hw=(hl, wl))
    a = cb.mag64(op, dy[sel], w, None, dtype, hw=(hl, wl))
    z32 = cb._op64(op, cb.rnd(dy[sel], dtype).float(), cb.rnd(w, dtype).float(), None, (hl, wl)).double()
    return dy, wk, None, z, a, co * k * k, z32


def _fcases():
    out = []
    for c in FCASES:
        if c[11] != HERE:
            continue
        dts = [BF, FP] if (HERE or c[13] or c[1] == "pool2") else [F32, BF, FP]
        out += [pytest.param(c, d, id=f"{c[0]}-{str(d).split('.')[-1]}") for d in dts]
    return out


def _igemm(xd, wk, b, out, case, dtype, ldi, ldo, acc, stats=None, xoff=0, ooff=0):
    Hi, Wi, cin, Ho, Wo, cout, KH, KW, mul, kmul, off, div, up, _ = _geometry(case)
    n = case[2]
    es = out.element_size()
    lib.mi355_conv2d_igemm(xd.data_ptr() + xoff * es, wk, None if b is None else b.to(DEV), out.data_ptr() + ooff * es, n, Hi, Wi,
                           cin, ldi, Ho, Wo, cout, ldo, KH, KW, mul, kmul, off, div, up, acc, stats, DTYPE_CODE[dtype])


def _nchw(y, sel, c0=0, c=None):
    """device NHWC -> CPU fp64 NCHW of the checked images and channel window"""
    t = y[sel].float().cpu()[..., c0:(c0 + c) if c else None]
    return t.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("case,dtype", _fcases())
def test_igemm_bounds(case, dtype):
    name, kind, n, ci, h, w_, co, k, s, p, up, switch, var, imgs = case
    code = DTYPE_CODE[dtype]
    Hi, Wi, cin, Ho, Wo, cout, KH, KW, mul, kmul, off, div, gup, pool = _geometry(case)
    want = 0 if dtype == F32 else var
    got_v = lib.mi355_conv2d_igemm_variant_n(n, Hi, Wi, cin, Ho, Wo, cout, KH, KW, mul, kmul, off, div, gup, code)
    assert got_v == want, f"{name}: served by variant {got_v}, expected {want}"
    rows = lib.mi355_conv2d_igemm_stat_rows(n, Hi, Wi, cin, Ho, Wo, cout, KH, KW, mul, kmul, off, div, gup, code)
    xin, wk, b, z, a, kk, z32 = _operands(case, dtype)
    sel = list(imgs) if imgs else list(range(n))
    ho_out, wo_out = (Ho // 2, Wo // 2) if pool else (Ho, Wo)
    print(f"\n{name} [{kind}] variant {got_v} {dtype}, stat rows {rows}")

    def judge(epi, y, model, old=None, relu=False):
        cpu = z32.clamp(min=0) if relu else z32
        if model in ("pool2", "pool2acc"):
            cpu = cb.sum2x2(cpu)
        if old is not None:
            cpu = cpu + old
        rep = cb.check(f"{name} {epi}", y, z, a, kk, dtype, model, old=old, relu=relu, y_cpu32=cpu)
        _record("igemm", got_v, dtype, epi, rep)
        assert model in cb.VARIANT_EPILOGUES[got_v], (got_v, model)
        assert rep.ok, rep.msg

    xd = to_nhwc(xin, dtype)
    if pool:
        # the 2x2-sum epilogue: plain, then accumulating onto random contents
        y = torch.full((n, ho_out, wo_out, cout), float("nan"), dtype=dtype, device=DEV)
        _igemm(xd, wk, None, y, case, dtype, cin, cout, 4)
        torch.cuda.synchronize()
        judge("pool2", _nchw(y, sel), "pool2")
        old = torch.randn(n, ho_out, wo_out, cout, generator=torch.Generator().manual_seed(3)).to(dtype)
        y = old.clone().to(DEV)
        _igemm(xd, wk, None, y, case, dtype, cin, cout, 5)
        torch.cuda.synchronize()
        judge("pool2acc", _nchw(y, sel), "pool2acc", old=old[sel].double().permute(0, 3, 1, 2))
        return
    # 1. plain, with the bias where the layer has one
    y = torch.full((n, Ho, Wo, cout), float("nan"), dtype=dtype, device=DEV)
    _igemm(xd, wk, b, y, case, dtype, cin, cout, 0)
    torch.cuda.synchronize()
    judge("plain", _nchw(y, sel), cb.model_for(0, dtype))
    if imgs:
        return                                      # (benchmark shapes: the plain epilogue only)
    # 2. bias + ReLU, input read from and output written into channel slices of wider buffers, fused statistics where the launcher
    #    has them; the neighbouring channels stay untouched
    xw = torch.zeros(n, Hi, Wi, cin + 32, dtype=dtype, device=DEV); xw[..., 32:] = xd
    base = torch.randn(n, Ho, Wo, cout + 64, generator=torch.Generator().manual_seed(4)).to(dtype)
    yw = base.clone().to(DEV)
    part = torch.full((max(rows, 1) * 2 * cout,), float("nan"), device=DEV) if rows and dtype != F32 else None
    _igemm(xw, wk, b, yw, case, dtype, cin + 32, cout + 64, 2, part, xoff=32, ooff=32)
    torch.cuda.synchronize()
    got = yw.cpu()
    assert torch.equal(got[..., :32], base[..., :32]) and torch.equal(got[..., 32 + cout:], base[..., 32 + cout:]), "neighbours written"
    judge("relu_slice", _nchw(yw, sel, 32, cout), cb.model_for(0, dtype), relu=True)
    if part is not None:
        r1, r2 = cb.stats_bound_check(part.cpu(), got[..., 32:32 + cout].reshape(-1, cout), rows)
        print(f"  [igemm v{got_v} stats] sum err/bound {r1:.3f}, sum-of-squares err/bound {r2:.3f}")
        assert r1 <= 1 and r2 <= 1, (r1, r2)
    # 3. accumulate into a channel slice of a wider buffer
    yw = base.clone().to(DEV)
    _igemm(xw, wk, b, yw, case, dtype, cin + 32, cout + 64, 1, xoff=32, ooff=32)
    torch.cuda.synchronize()
    got = yw.cpu()
    assert torch.equal(got[..., :32], base[..., :32]) and torch.equal(got[..., 32 + cout:], base[..., 32 + cout:]), "neighbours written"
    old = base[..., 32:32 + cout].double().permute(0, 3, 1, 2)
    judge("acc_slice", _nchw(yw, sel, 32, cout), cb.model_for(1, dtype), old=old)
    # 4. the statistics guard: a stats buffer is accepted exactly when the row query says the variant has the epilogue
    if rows == 0:
        M = n * Ho * Wo
        big = torch.zeros(((M + 63) // 64 + 2) * 2 * 4 * cout, device=DEV)      # (room for any partial layout, should it launch)
        with pytest.raises(RuntimeError, match="statistics"):
            _igemm(xd, wk, b, y, case, dtype, cin, cout, 0, big)
        torch.cuda.synchronize()
        assert float(big.abs().sum()) == 0.0
    if rows:
        with pytest.raises(RuntimeError, match="statistics"):                  # (never with the accumulate epilogue)
            _igemm(xd, wk, b, y, case, dtype, cin, cout, 1, part)


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------
# (name, N, ci, H, W, co, k, stride, pad, up, cip, switch, mode of the 2-byte types)
WCASES = [
    ("wg_pad_cip", 2, 32, 12, 12, 64, 3, 1, 1, 0, 64, "", 0),
    ("wg_s2", 2, 32, 16, 16, 64, 3, 2, 1, 0, 32, "", 0),
    ("wg_1x1", 3, 64, 8, 8, 64, 1, 1, 0, 0, 64, "", 0),
    ("wg_halo32", 3, 64, 16, 32, 96, 3, 1, 1, 0, 64, "", 1),
    ("wg_halo32_w96", 2, 64, 8, 96, 64, 3, 1, 1, 0, 64, "", 1),
    ("wg_halo16x2", 6, 64, 16, 16, 64, 3, 1, 1, 0, 64, "", 2),
    ("wg_halo16x2_up", 2, 64, 8, 8, 64, 3, 1, 1, 1, 64, "", 2),
    ("wg_halo8_64", 2, 64, 32, 128, 64, 3, 1, 1, 0, 64, "", 3),
    ("wg_halo8_64_up", 2, 64, 16, 32, 64, 3, 1, 1, 1, 64, "", 3),
    ("wg_halo8_big", 4, 64, 256, 256, 64, 3, 1, 1, 0, 64, "", 3),              # K = 4 * 256 * 256 = 2^18
    ("wg_halo8_32x2", 4, 96, 24, 32, 64, 3, 1, 1, 0, 96, "", 4),
    ("wg_halo8_32x2_up", 4, 64, 8, 16, 128, 3, 1, 1, 1, 64, "", 4),
    ("wg8off_64", 2, 64, 32, 128, 64, 3, 1, 1, 0, 64, "wgrad8off", 1),
    ("wg8off_32_up", 4, 64, 8, 16, 64, 3, 1, 1, 1, 64, "wgrad8off", 1),
    ("wghalo0", 2, 64, 16, 32, 64, 3, 1, 1, 0, 64, "wgradhalo0", 0),
]


def _wcases():
    out = []
    for c in WCASES:
        if c[11] != HERE:
            continue
        dts = [BF, FP] if (HERE or c[0] == "wg_halo8_big") else [F32, BF, FP]
        out += [pytest.param(c, d, id=f"{c[0]}-{str(d).split('.')[-1]}") for d in dts]
    return out


def _check_reduce(name, ws, sp, co, cip, ci, k, z, a, kk, mode, dtype, tag):
    """mi355_conv2d_wgrad_reduce at beta = 0 and beta = 1 against the fp64 weight gradient"""
    dw = torch.full((co, ci, k, k), float("nan"), device=DEV)
    lib.mi355_conv2d_wgrad_reduce(ws, sp, dw, co, cip, ci, k, k, 0, 0.0)
    torch.cuda.synchronize()
    rep = cb.check(f"{name} splits={sp} beta=0", dw.cpu(), z, a, kk, F32, "fp32")
    _record(tag, mode, dtype, f"splits={sp},beta=0", rep)
    assert rep.ok, rep.msg
    old = torch.randn(co, ci, k, k, generator=torch.Generator().manual_seed(sp))
    dw = old.to(DEV)
    lib.mi355_conv2d_wgrad_reduce(ws, sp, dw, co, cip, ci, k, k, 0, 1.0)
    torch.cuda.synchronize()
    rep = cb.check(f"{name} splits={sp} beta=1", dw.cpu(), z, a, kk, F32, "fp32", old=old.double())
    _record(tag, mode, dtype, f"splits={sp},beta=1", rep)
    assert rep.ok, rep.msg


@pytest.mark.parametrize("case,dtype", _wcases())
def test_wgrad_bounds(case, dtype):
    name, n, ci, h, w_, co, k, s, p, up, cip, switch, mode = case
    code = DTYPE_CODE[dtype]
    hl, wl = (2 * h, 2 * w_) if up else (h, w_)
    ho, wo = (hl + 2 * p - k) // s + 1, (wl + 2 * p - k) // s + 1
    want = 0 if dtype == F32 else mode
    got_m = lib.mi355_conv2d_wgrad_variant(n, ho, wo, k, k, s, p, code)
    assert got_m == want, f"{name}: weight-gradient mode {got_m}, expected {want}"
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(n, ci, h, w_, generator=g)
    dy = torch.randn(n, co, ho, wo, generator=g)
    op = {"kind": "wgrad", "stride": s, "pad": p, "up": up, "k": k}
    z = cb.ref64(op, x, dy, None, dtype)
    a = cb.mag64(op, x, dy, None, dtype)
    kk = n * ho * wo                                   # every pixel, over all splits
    print(f"\n{name} mode {got_m} {dtype}, K = {kk}")
    xd = to_nhwc(x, dtype, cpad=cip)
    dyd = to_nhwc(dy, dtype)
    default = lib.mi355_conv2d_wgrad_splits(n, ho, wo, cip, co, k, k)
    for sp in sorted({1, 3, default}):
        ws = torch.full((sp, co, k * k, cip), float("nan"), device=DEV)
        lib.mi355_conv2d_wgrad(xd, dyd, ws, sp, n, h, w_, cip, cip, ho, wo, co, co, k, k, s, p, up, code)
        _check_reduce(name, ws, sp, co, cip, ci, k, z, a, kk, got_m, dtype, "wgrad")


# (name, N, ci, H, W, co, up, extra input channels (ldx = ci + extra), napp, switch, mode)
MCASES = [
    ("wm_n1_halo8_32x2", 6, 64, 16, 32, 64, 0, 0, 1, "", 4),          # (3 work items: splits = 3 fits)
    ("wm_n2_halo8_64_ldx", 2, 64, 8, 64, 64, 0, 32, 2, "", 3),
    ("wm_n3_halo32", 3, 64, 16, 32, 96, 0, 0, 3, "", 1),
    ("wm_n6_up", 2, 32, 8, 16, 64, 1, 0, 6, "", 4),
    ("wm_n6_halo16x2_ldx", 4, 64, 16, 16, 64, 0, 32, 6, "", 2),
    ("wm8off_n2_ldx", 2, 64, 16, 64, 64, 0, 32, 2, "wgrad8off", 1),
    ("wm8off_n3_16x2", 2, 64, 8, 16, 64, 0, 0, 3, "wgrad8off", 2),
]


def _mcases():
    return [pytest.param(c, d, id=f"{c[0]}-{str(d).split('.')[-1]}") for c in MCASES if c[9] == HERE for d in (BF, FP)]


@pytest.mark.parametrize("case,dtype", _mcases())
def test_wgrad_multi_bounds(case, dtype):
    """mi355_conv2d_wgrad_multi: the recurrent block's shared-weight gradient over napp distinct operand pairs in one launch; the
    reference is the fp64 sum over the pairs, K = napp * N * Ho * Wo"""
    name, n, ci, h, w_, co, up, extra, napp, switch, mode = case
    code = DTYPE_CODE[dtype]
    ho, wo = (2 * h, 2 * w_) if up else (h, w_)
    assert lib.mi355_conv2d_wgrad_multi_ok(n, ho, wo, code) == 1
    assert lib.mi355_conv2d_wgrad_variant(n, ho, wo, 3, 3, 1, 1, code) == mode
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    op = {"kind": "wgrad", "stride": 1, "pad": 1, "up": up, "k": 3}
    xs, dys, z, a = [], [], 0, 0
    for i in range(napp):
        x = torch.randn(n, ci, h, w_, generator=g)
        dy = torch.randn(n, co, ho, wo, generator=g)
        z = z + cb.ref64(op, x, dy, None, dtype)
        a = a + cb.mag64(op, x, dy, None, dtype)
        xw = torch.zeros(n, h, w_, ci + extra, dtype=dtype)
        xw[..., extra:] = x.permute(0, 2, 3, 1).to(dtype)
        xs.append(xw.to(DEV))
        dys.append(to_nhwc(dy, dtype))
    kk = napp * n * ho * wo
    print(f"\n{name} mode {mode} {dtype}, napp {napp}, K = {kk}")
    es = 2
    ptrs = []
    for i in range(6):
        ptrs += [xs[i].data_ptr() + extra * es, dys[i].data_ptr()] if i < napp else [None, None]
    default = lib.mi355_conv2d_wgrad_splits(n * napp, ho, wo, ci, co, 3, 3)
    for sp in sorted({1, 3, default}):
        ws = torch.full((sp, co, 9, ci), float("nan"), device=DEV)       # splits * Co * 9 * Ci floats (include/mi355conv.h)
        lib.mi355_conv2d_wgrad_multi(*ptrs, napp, ws, sp, n, h, w_, ci, ci + extra, ho, wo, co, co, up, code)
        _check_reduce(name, ws, sp, co, ci, ci, 3, z, a, kk, mode, dtype, "wgrad_multi")


# ---- child processes (switches read once per process) and the coverage check -----------------------------------------------------
def _children():
    return [pytest.param(k, id=k) for k in SWITCHES] if not HERE else []


_CHILD_ROWS = []


@pytest.mark.parametrize("switch", _children())
def test_switched_variants_in_a_child_process(switch):
    fd, path = tempfile.mkstemp(suffix=".jsonl")
    os.close(fd)
    try:
        env = dict(os.environ, MI355_BOUNDS_SWITCH=switch, MI355_BOUNDS_REPORT=path, **SWITCHES[switch])
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider"],
                           env=env, capture_output=True, text=True, timeout=420)
        print(r.stdout[-6000:])
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
        with open(path) as f:
            rows = [json.loads(line) for line in f if line.strip()]
        assert rows, f"child {switch} ran no case"
        _CHILD_ROWS.extend(rows)
    finally:
        os.unlink(path)


def _all_rows():
    return RESULTS + _CHILD_ROWS


def _coverage():
    return [pytest.param("all", id="all")] if not HERE else []       # (the parent process only)


@pytest.mark.parametrize("scope", _coverage())
def test_every_variant_and_mode_ran(scope):
    """(runs last: after the cases of this process and the child processes) every forward variant 0-9 per 2-byte dtype (fp32: the
    generic kernel), every weight-gradient mode 0-4 per 2-byte dtype, mode 0 for fp32, and wgrad_multi; prints the table"""
    rows = _all_rows()
    table = {}
    for r in rows:
        key = (r["kind"], r["variant"], r["dtype"])
        t = table.setdefault(key, {"epi": set(), "ratio": 0.0, "rms": None, "mean": 0.0, "n": 0})
        t["epi"].add(r["epi"].split(",")[0] if r["kind"] != "igemm" else r["epi"])
        t["ratio"] = max(t["ratio"], r["ratio"])
        if r["rms"] is not None:
            t["rms"] = max(t["rms"] or 0.0, r["rms"])
            t["mean"] = max(t["mean"], abs(r["mean"]), key=abs)
        t["n"] += 1
    print("\n| kernel | variant | dtype | checks | max err/bound | max RMS (ulp) | max abs mean (ulp) | epilogues |")
    print("|---|---|---|---|---|---|---|---|")
    for (kind, v, dt), t in sorted(table.items()):
        nm = cb.VARIANT_NAMES[v] if kind == "igemm" else cb.WGRAD_NAMES[v]
        rms = f"{t['rms']:.3f}" if t["rms"] is not None else "-"
        mean = f"{t['mean']:.4f}" if t["rms"] is not None else "-"
        print(f"| {kind} | {v} {nm} | {dt} | {t['n']} | {t['ratio']:.3f} | {rms} | {mean} | {' '.join(sorted(t['epi']))} |")
    for dt in ("bfloat16", "float16"):
        fv = {v for (kind, v, d) in table if kind == "igemm" and d == dt}
        assert fv == set(range(10)), f"{dt}: forward variants that never ran: {sorted(set(range(10)) - fv)}"
        wm = {v for (kind, v, d) in table if kind == "wgrad" and d == dt}
        assert wm == set(range(5)), f"{dt}: weight-gradient modes that never ran: {sorted(set(range(5)) - wm)}"
        assert any(kind == "wgrad_multi" and d == dt for (kind, v, d) in table)
        epis = {e for (kind, v, d), t in table.items() if kind == "igemm" and d == dt for e in t["epi"]}
        assert {"plain", "relu_slice", "acc_slice", "pool2", "pool2acc"} <= epis
    assert {v for (kind, v, d) in table if d == "float32"} == {0}


# a child process collects only its own switch's cases: drop the tests that have none there (an empty parameter set would show up
# as a skipped test)
for _test, _params in (("test_igemm_bounds", _fcases()), ("test_wgrad_bounds", _wcases()), ("test_wgrad_multi_bounds", _mcases()),
                       ("test_switched_variants_in_a_child_process", _children()), ("test_every_variant_and_mode_ran", _coverage())):
    if not _params:
        del globals()[_test]
