"""References and case tables for the layout, weight-pack, up-sampling and add / ReLU kernels of csrc/elementwise.hip.  CPU only,
plain torch / numpy.

Every reference is written from the semantics documented in include/mi355conv.h and returns a tensor of the STORAGE type: these
operations are exact or round exactly once (fp32 -> storage type, round to nearest even), so tests/test_gpu_layout_exact.py
compares bits — -0.0, inf and subnormals count.  tests/test_layout_ref_cpu.py holds each reference against an independent
restatement on the inputs of the GPU cases and asserts the properties of those inputs the GPU cases rely on.

The second half restates the launch geometry (grid caps, the rowmap split, the weight tiles, the im2col workgroup widths) FOR
CHOOSING SIZES AND NAMING BRANCHES ONLY: no expected value comes from it."""
import math

import torch

import stream_exact as se

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
EPC = se.EPC
INF = math.inf


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * (i + 3) for i, k in enumerate(key)) % (2 ** 31))


# ---- the one rounding -----------------------------------------------------------------------------------------------------------
def round_to(x32, dtype):
    """fp32 -> storage type, round to nearest even (overflow to inf, gradual underflow); the identity for fp32"""
    assert x32.dtype == F32, x32.dtype
    return x32.to(dtype)


# fp32 values at which a conversion can go wrong, planted into every operand that a kernel rounds
SPECIALS = [
    1.0 + 2.0 ** -8,            # bf16 tie, down to 1 (even)
    1.0 + 3 * 2.0 ** -8,        # bf16 tie, up to 1 + 2^-6
    -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),
    1.0 + 2.0 ** -11,           # fp16 tie, down to 1
    1.0 + 3 * 2.0 ** -11,       # fp16 tie, up to 1 + 2^-9
    -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -11),
    1.0 + 2.0 ** -8 + 2.0 ** -20,   # just above a bf16 tie: up
    1.0 + 2.0 ** -11 - 2.0 ** -23,  # just below an fp16 tie: down
    70000.0, -70000.0,          # beyond fp16: inf
    65520.0,                    # the fp16 tie between 65504 and 2^16: inf
    65519.0,                    # just below it: 65504
    3.0 * 2.0 ** -24,           # an fp16 subnormal, exact
    2.0 ** -25,                 # tie between 0 and the smallest fp16 subnormal: +0
    3.0 * 2.0 ** -25,           # tie between 2^-24 and 2^-23: up to 2^-23
    -5.0 * 2.0 ** -26,          # between two fp16 subnormals: -2^-24
    2.0 ** -130,                # an fp32 (and bf16) subnormal
    3.4e38, -3.4e38,            # beyond bf16's largest finite value: inf
    -0.0, INF, -INF,
]


def specials():
    return torch.tensor(SPECIALS, dtype=F32)


def plant(x, values, start=0, step=1):
    """values written into the flattened x at start, start + step, ... (x is changed and returned)"""
    f = x.reshape(-1)
    n = min(len(values), (f.numel() - start + step - 1) // step)
    f[start:start + n * step:step] = values[:n]
    return x


# ---- NCHW fp32 <-> NHWC ----------------------------------------------------------------------------------------------------------
def pack_nchw_ref(x, cwrite, dtype):
    """NCHW fp32 -> [N, H, W, cwrite] of dtype: channel c of pixel (n, h, w) is x[n][c][h][w] rounded, channels >= C are +0"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, cwrite, dtype=dtype)
    y[..., :C] = round_to(x.permute(0, 2, 3, 1).contiguous(), dtype)
    return y


def unpack_ref(x, N, H, W):
    """[N*H*W, C] of a storage type -> NCHW fp32 (every storage value is an fp32 value)"""
    C = x.shape[-1]
    return x.reshape(N, H, W, C).permute(0, 3, 1, 2).float().contiguous()


def im2col3_ref(x, dtype):
    """NCHW fp32, C <= 3 -> [N, H, W, 32]: channel c * 9 + kh * 3 + kw = x[n][c][h + kh - 1][w + kw - 1], +0 outside the image and
    for k >= 9 C"""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, 32, dtype=dtype)
    for c in range(C):
        for kh in range(3):
            for kw in range(3):
                for h in range(H):
                    hh = h + kh - 1
                    if not 0 <= hh < H:
                        continue
                    w_lo, w_hi = max(0, 1 - kw), min(W, W + 1 - kw)          # output columns whose tap lies inside the image
                    if w_lo < w_hi:
                        y[:, h, w_lo:w_hi, c * 9 + kh * 3 + kw] = round_to(x[:, c, hh, w_lo + kw - 1:w_hi + kw - 1].contiguous(), dtype)
    return y


def pack_weight_ref(w, Co, Ci, Cip, taps, transposed, scale, dtype):
    """fp32 parameter [Co][Ci][taps] ([Ci][Co][taps] when transposed) -> (Wf [Co][taps][Cip], Wb [Cip][taps][Co]) of dtype, ci >= Ci
    zero.  scale[Co] (fp32 or None) multiplies output channel co as ONE fp32 product before the single rounding; it is ignored
    when transposed."""
    assert w.dtype == F32 and w.numel() == Co * Ci * taps
    w3 = w.reshape(Ci, Co, taps).permute(1, 0, 2) if transposed else w.reshape(Co, Ci, taps)
    if scale is not None and not transposed:
        assert scale.dtype == F32
        w3 = w3 * scale.view(Co, 1, 1)
        assert w3.dtype == F32
    wf = torch.zeros(Co, taps, Cip, dtype=dtype)
    wf[..., :Ci] = round_to(w3.permute(0, 2, 1).contiguous(), dtype)
    wb = torch.zeros(Cip, taps, Co, dtype=dtype)
    wb[:Ci] = round_to(w3.permute(1, 2, 0).contiguous(), dtype)
    return wf, wb


# ---- up-sampling gradient, add, ReLU gradient -------------------------------------------------------------------------------------
def groups2x2(dy, N, H, W):
    """[N*2H*2W, C] -> the four terms of every coarse pixel, fp64 [4, N*H*W, C]"""
    C = dy.shape[-1]
    v = dy.double().reshape(N, H, 2, W, 2, C).permute(2, 4, 0, 1, 3, 5)
    return v.reshape(4, N * H * W, C)


def upsample2_bwd_ref(dy, old, dtype, shape):
    """gradient of nearest x2 up-sampling: the fp64 sum of the 2 x 2 group of dy (+ old when accumulating), rounded ONCE to dtype.
    The sums must be exact in fp32 (asserted): the one rounding is then the same whichever way fp32 partial sums were formed."""
    N, H, W = shape
    s = groups2x2(dy, N, H, W).sum(0)
    if old is not None:
        s = s + old.double()
    assert torch.equal(s.float().double(), s), "the case's sums are not exact in fp32"
    return round_to(s.float(), dtype)


def add_ref(a, b, dtype):
    """y = a + b rounded once (the fp64 sum must be exact in fp32: asserted); b None: the bits of a"""
    if b is None:
        return a.clone()
    s = a.double() + b.double()
    assert torch.equal(s.float().double(), s), "the case's sums are not exact in fp32"
    return round_to(s.float(), dtype)


def relu_bwd_ref(dy, y):
    """dx = y > 0 ? dy : +0 — the bits of dy pass unchanged"""
    return torch.where(y.double() > 0, dy, torch.zeros_like(dy))


# ---- data ---------------------------------------------------------------------------------------------------------------------------
HUGE = 3.0e38


def nchw_case(N, C, H, W, big=False):
    """fp32 NCHW input of the pack cases: random values, the last real channel carrying inf and a huge value, SPECIALS planted"""
    g = _gen(N, C, H, W, 11)
    if big:                                   # (a few million elements: cheap to make, every value needs rounding in bf16 / fp16)
        x = torch.randint(-2 ** 20, 2 ** 20, (N, C, H, W), generator=g).float() * 2.0 ** -12
    else:
        x = torch.randn(N, C, H, W, generator=g) * 3
    hw = torch.arange(H * W).reshape(H, W)
    last = x[:, C - 1]
    last[:, hw % 3 == 0] = INF
    last[:, hw % 3 == 1] = HUGE
    return plant(x, specials())


def storage_case(M, C, dtype, key=0):
    """[M, C] of dtype for the unpack / copy cases: random storage values with subnormals, inf and -0.0 among them"""
    g = _gen(M, C, key, 13)
    x = (torch.randn(M, C, generator=g) * 3).to(dtype)
    tiny = {F32: 2.0 ** -149, BF: 2.0 ** -133, FP: 2.0 ** -24}[dtype]
    vals = torch.tensor([tiny, -tiny, 3 * tiny, INF, -INF, -0.0, 0.0, 2.0 ** -126 if dtype != FP else 2.0 ** -14], dtype=torch.float64).to(dtype)
    return plant(x, vals, start=min(1, x.numel() - 1), step=max(1, x.numel() // 9))


def im2col_case(N, C, H, W):
    """fp32 NCHW: random values; every other border pixel and every third pixel of channel C - 1 carry +-inf"""
    g = _gen(N, C, H, W, 17)
    x = torch.randn(N, C, H, W, generator=g) * 3
    h, w = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    border = ((h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)) & ((h + w) % 2 == 0)
    x[:, :, border] = INF
    x[:, C - 1, (h * W + w) % 3 == 1] = -INF
    return x


def ints_t(gen, shape, lim, dtype, pzero=0.3):
    """se.ints in the storage type (every |value| <= lim must be storable)"""
    t = se.ints(gen, shape, lim, pzero)
    se.assert_storable(t, dtype, "integer operand")
    return t.to(dtype)


ROUND_LIM = {BF: 255, FP: 2047}      # integers the type stores exactly whose four- and five-term sums it does not


def upsample_case(N, H, W, C, dtype, kind):
    """(dy [N*2H*2W, C], old [N*H*W, C]) of dtype.  kind "int": small integers, every sum storable.  kind "rounding" (2-byte
    types): integers up to ROUND_LIM, so that the sums are exact in fp32 but mostly NOT storable — the result shows where and how
    often the kernel rounds."""
    g = _gen(N, H, W, C, {"int": 1, "rounding": 2}[kind], 19)
    lim = 4 if kind == "int" else ROUND_LIM[dtype]
    pz = 0.3 if kind == "int" else 0.05
    return ints_t(g, (N * 4 * H * W, C), lim, dtype, pz), ints_t(g, (N * H * W, C), lim, dtype, pz)


def big_ints(gen, shape, dtype):
    """integers in [-4, 4] of dtype without an fp64 detour (operands of a hundred MB)"""
    return torch.randint(-4, 5, shape, generator=gen, dtype=torch.int8).to(dtype)


def add_case(M, C, dtype, key=0):
    """(a, b) [M, C] of dtype: integers up to 255 (every sum exact in fp32; in bf16 most sums need the one rounding)"""
    g = _gen(M, C, key, 23)
    return ints_t(g, (M, C), 255, dtype, 0.1), ints_t(g, (M, C), 255, dtype, 0.1)


def relu_case(M, C, dtype):
    """(dy, y) [M, C] of dtype.  y: small integers with 0, -0.0 and negative values; dy: integers, with inf, -inf and -0.0 planted
    both where y > 0 (their bits must pass) and where y <= 0 (the result must be +0: a product with a 0 / 1 mask would be NaN)"""
    g = _gen(M, C, 29)
    y = ints_t(g, (M, C), 3, dtype, 0.3)
    y = torch.where(torch.rand(M, C, generator=g) < 0.1, torch.tensor(-0.0, dtype=dtype), y)
    dy = ints_t(g, (M, C), 100, dtype, 0.1)
    sp = torch.tensor([INF, -INF, -0.0], dtype=dtype)[torch.randint(0, 3, (M, C), generator=g)]
    dy = torch.where(torch.rand(M, C, generator=g) < 0.3, sp, dy)
    return dy, y


def weight_case(case, key=0):
    """(w fp32 flat, scale fp32 [Co] or None) of a weight case; SPECIALS planted into w"""
    Co, Ci, Cip, KH, KW, tr, has_wb, sc = case
    g = _gen(Co, Ci, Cip, KH * KW, tr, key, 31)
    w = plant(torch.randn(Co * Ci * KH * KW, generator=g), specials(), start=KH * KW - 1, step=max(1, (Co * Ci * KH * KW) // 29))
    scale = (torch.rand(Co, generator=g) + 0.5).float() if sc else None
    return w, scale


# ---- the launch geometry, restated for choosing sizes and naming branches only ------------------------------------------------------
FLAT_CAP = 8192 * 256          # threads of a whole flat grid: pack / unpack / upsample2_bwd (8192 workgroups of 256)
WEIGHT_CAP = 4096 * 256        # ... of mi355_pack_conv_weight
ROWMAP_CAP = 4096              # workgroups of a plain rowmap launch (add, relu_bwd)
BATCHED_GRID = 256             # workgroups per descriptor of the batched weight pack
TA, ROWMAX = 32, 288


def flat_branches(threads, cap=FLAT_CAP):
    return ["grid_stride"] if threads > cap else []


def rowmap_geom(dtype, C):
    """(cp, tpr, rp) of rowmap_kernel"""
    _, cp, tpr, rp, _, _ = se.geometry(dtype, C)
    return cp, tpr, rp


def rowmap_branches(dtype, C, M):
    cp, _, rp = rowmap_geom(dtype, C)
    return (["colblocks>1"] if cp > 256 else []) + (["second_sweep"] if M > ROWMAP_CAP * rp else [])


def edge_rows(rp, B, extra=()):
    """row counts without a whole batch and just around one, plus the case's extras (as tests/test_gpu_stream_exact.py)"""
    ms = {1, rp - 1, rp * B - 1, rp * B, rp * B + 1} | set(extra)
    return sorted(m for m in ms if m >= 1)


def im2col_bx(W):
    return 256 if W >= 256 else (128 if W >= 128 else 64)


def im2col_branches(W):
    bx = im2col_bx(W)
    return [f"bx{bx}"] + (["x_blocks>1"] if W > bx else [])


def weight_tb(taps):
    return max(1, min(32, ROWMAX // taps))


def weight_branches(case, dtype):
    """the branches of pack_weight_batched_kernel a descriptor reaches"""
    Co, Ci, Cip, KH, KW, tr, has_wb, sc = case
    taps = KH * KW
    TB = weight_tb(taps)
    A, B = (Ci, Co) if tr else (Co, Ci)
    Ap, Bp = (Cip, Co) if tr else (Co, Cip)
    V = 16 // torch.tensor([], dtype=dtype).element_size()
    br = {f"TB{TB}"}
    tiles_b = -(-Bp // TB)
    for a0 in range(0, Ap, TA):
        na = min(TA, Ap - a0)
        vec_a = dtype != F32 and na % V == 0 and Ap % V == 0 and a0 % V == 0
        if na < TA or a0 + na > A:
            br.add("ragged_a")
        for b0 in range(0, Bp, TB):
            nb = min(TB, Bp - b0)
            vec_b = dtype != F32 and nb % V == 0 and Bp % V == 0 and b0 % V == 0
            out_b, out_a = (has_wb, True) if tr else (True, has_wb)
            if out_b:
                br.add("vec_b" if vec_b else "elem_b")
            if out_a:
                br.add("vec_a" if vec_a else "elem_a")
            if b0 >= B:
                br.add("pad_tile")
            elif b0 + nb > B:
                br.add("part_tile")
    if -(-Ap // TA) * tiles_b > BATCHED_GRID:
        br.add("tiles>grid")
    br.add("scale+transposed" if sc and tr else ("scale" if sc else "no_scale"))
    if not has_wb:
        br.add("no_wb")
    if tr:
        br.add("transposed")
    return sorted(br)


# ---- case tables --------------------------------------------------------------------------------------------------------------------
PACK_INPUT_CASES = [(3, c, 5, 7, 32) for c in (1, 2, 3, 5)] + [(3, 9, 5, 7, 16), (3, 8, 5, 7, 8)]        # (N, C, H, W, Cpad)
PACK_HW = [(2, 7, 9), (2, 1, 1)]                                                                          # (N, H, W) of pack_nchw / unpack


def pack_chans(dtype):
    return [4, 12] if dtype == F32 else [8, 24]


def pack_sweep(dtype):
    """(N, C, H, W) whose N*H*W*chunks exceeds a whole flat grid of pack_nchw_kernel"""
    return (2, 64 if dtype == F32 else 128, 257, 257)


UNPACK_SWEEP = (2, 16, 257, 257)               # N*C*H*W beyond a whole flat grid of unpack_nchw_kernel

IM2COL_CASES = ([(2, 3, 3, w) for w in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)] + [(2, 3, 1, 5), (2, 3, 2, 5)]
                + [(2, 1, 3, 65), (2, 2, 3, 65)])                                                      # (N, C, H, W)
IM2COL_ROWS = (21846, 1, 3, 3)                 # N * H = 65 538 workgroup rows

# (Co, Ci, Cip, KH, KW, transposed, has_wb, scale)
WEIGHT_CASES = [
    (1, 64, 64, 1, 1, 0, 1, 0),          # the logit head
    (2, 40, 40, 1, 1, 0, 1, 1),          # the gate's psi; last b tile nb = 8 (vector path); scale
    (37, 16, 16, 3, 3, 0, 1, 1),         # ragged a tile, element path in a
    (40, 3, 32, 3, 3, 0, 1, 0),          # the stem: one b tile, 3 real + 29 padded
    (40, 3, 64, 3, 3, 0, 1, 1),          # ... and a whole padded b tile at 3 x 3
    (64, 3, 32, 7, 7, 0, 1, 0),          # TB = 5: the tiles b0 = 5 .. 30 are all padding
    (64, 3, 32, 7, 7, 0, 0, 1),          # the same without wb, scaled
    (32, 130, 136, 3, 3, 0, 1, 0),       # a tile partly real, partly padding
    (40, 36, 36, 3, 3, 0, 1, 1),         # Cip % 8 != 0: element path in b
    (40, 3, 32, 2, 2, 1, 1, 0),          # transposed, Ci = 3
    (36, 32, 32, 2, 2, 1, 1, 1),         # transposed, Co = 36, a scale pointer that must be ignored
    (8, 20, 24, 4, 4, 0, 1, 0),          # taps 16
    (8, 12, 16, 5, 5, 0, 1, 1),          # taps 25
    (3, 5, 8, 12, 12, 0, 1, 0),          # taps 144
    (2, 3, 8, 16, 16, 0, 1, 1),          # taps 256
    (32, 264, 264, 16, 16, 0, 1, 0),     # 264 tiles for 256 workgroups: the second trip through LDS
]
WEIGHT_TABLES = {"all": list(range(len(WEIGHT_CASES))), "small_a": [0, 1, 2, 9], "small_b": [5, 10, 7, 14, 3]}
WEIGHT_SWEEP = (128, 1024, 1024, 3, 3, 0, 1, 0)      # Co*taps*Cip beyond a whole grid of pack_weight_kernel
TB_CLASSES = {1: 32, 4: 32, 9: 32, 16: 18, 25: 11, 49: 5, 144: 2, 256: 1}

UPSAMPLE_SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 5, 7)]                                            # (N, H, W)


def upsample_chans(dtype):
    return [4, 20, 48] if dtype == F32 else [8, 40, 96]


def upsample_sweep(dtype):
    """(N, H, W, C): N*H*W*chunks beyond a whole flat grid, H and W odd, few pixels"""
    return (1, 91, 91, 1024 if dtype == F32 else 2048)


CH2 = [8, 40, 96, 64, 1024, 2048, 2560]         # the channel counts of tests/test_gpu_stream_exact.py (2-byte types; fp32: half)


def chans(dtype):
    return [c // 2 for c in CH2] if dtype == F32 else list(CH2)


def rowmap_rows(dtype, C):
    rp = rowmap_geom(dtype, C)[2]
    return edge_rows(rp, 1, (3 * rp + 2,))


def rowmap_sweep(dtype):
    """(M, C): 256 chunks per row (rp = 1), one row more than a whole sweep and a batch"""
    C = 256 * EPC[dtype]
    rp = rowmap_geom(dtype, C)[2]
    return ROWMAP_CAP * rp + rp + 1, C
