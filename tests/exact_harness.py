"""What the exact-data GPU files (tests/test_gpu_stream_exact.py, tests/test_gpu_gate_exact.py, tests/test_gpu_head_exact.py,
tests/test_gpu_layout_exact.py) share: guarded device buffers, the launch-and-compare step, the coverage ledger and the runner of
child pytest processes.

Every tensor is a channel slice of a wider buffer with guard channels on both sides and guard rows behind row M - 1 (NaN in
inputs, a sentinel in outputs); outputs are pre-filled with NaN.  After each launch: guards unchanged, no NaN, bit-equal to the
reference, and a second launch gives the same bytes."""
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

import stream_exact as se
from gpu_util import DEV

F32, BF, FP = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF, FP]
G = 8                 # guard channels on each side (16 / 32 bytes: the slices stay 16-byte aligned)
SENT = 77.0
NAN = float("nan")


def _dn(dtype):
    return str(dtype).split(".")[-1]


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Buf:
    """[M + guard rows][G + C + G] of `dtype` on the device.  body given: an input (guards NaN; the launch must leave every byte
    alone) or, with inout, an accumulated output (guards = sentinel); body None: an output (body NaN, guards = sentinel)."""

    def __init__(self, M, C, dtype, gr, body=None, inout=False):
        self.M, self.C, self.input = M, C, body is not None and not inout
        w = torch.full((M + gr, C + 2 * G), NAN if self.input else SENT, dtype=dtype)
        if body is None:
            w[:M, G:G + C] = NAN
        else:
            se.assert_storable(body, dtype, "operand")
            w[:M, G:G + C] = body.to(dtype)
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + G * self.t.element_size()
        self.ld = C + 2 * G

    def reset(self):
        self.t.copy_(self.init)

    def body(self):
        return self.t[:self.M, G:G + self.C].cpu().double()

    def guards_ok(self):
        if self.input:
            return torch.equal(_bits(self.t), _bits(self.init))
        a = self.t.clone()
        a[:self.M, G:G + self.C] = self.init[:self.M, G:G + self.C]
        return torch.equal(_bits(a), _bits(self.init))


class Flat(Buf):
    """a contiguous fp32 output of n floats (partial rows, per-channel results) between two sentinel pads"""

    def __init__(self, n, body=None):
        self.M, self.C, self.input, self.n = 1, n, False, n
        w = torch.full((n + 2 * G,), SENT, dtype=F32)
        w[G:G + n] = NAN if body is None else body.float()
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + 4 * G

    def body(self):
        return self.t[G:G + self.n].cpu().double()

    def guards_ok(self):
        a = self.t.clone()
        a[G:G + self.n] = self.init[G:G + self.n]
        return torch.equal(_bits(a), _bits(self.init))


class Vec(Flat):
    """a contiguous fp32 INPUT of n floats (one value per row) between two NaN pads: the launch must leave every byte alone"""

    def __init__(self, body):
        se.assert_storable(body, F32, "operand")
        n = body.numel()
        self.M, self.C, self.input, self.n = 1, n, True, n
        w = torch.full((n + 2 * G,), NAN, dtype=F32)
        w[G:G + n] = body.float()
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + 4 * G

    def guards_ok(self):
        return torch.equal(_bits(self.t), _bits(self.init))


def _run(what, fn, bufs, want, twice=True):
    """launch; guards, NaN, bit-equality against want {Buf: fp64 reference of its body}; a second launch gives the same bytes"""
    fn()
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.guards_ok(), f"{what}: guard rows / channels of buffer {i} changed"
    first = {}
    for b, ref in want.items():
        got = b.body()
        assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} elements never written (or NaN read)"
        ref = ref.reshape(got.shape)
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {got.numel()} elements differ, max |diff| {float((got - ref).abs().max())}"
        first[b] = _bits(b.t).clone()
    if twice:
        for b in bufs:
            b.reset()
        fn()
        torch.cuda.synchronize()
        for b in want:
            assert torch.equal(_bits(b.t), first[b]), f"{what}: a second launch gives other bytes"


# ---- operands given in the storage type itself, compared by their BITS (-0.0, inf and subnormals count) ---------------------------
class Slice:
    """[M + guard rows][g + C + g] of `dtype` on the device, the body a channel slice (ld = C + 2 g).  `body` is a tensor of `dtype`
    itself (its bits are kept).  body given: an input (guards NaN; the launch must leave every byte alone) or, with inout, an
    output that is also read (guards = sentinel); body None: an output (body NaN, guards = sentinel)."""

    def __init__(self, M, C, dtype, gr, body=None, inout=False, g=G):
        assert g % 8 == 0                                  # the slice stays 16-byte aligned
        self.M, self.C, self.g, self.input = M, C, g, body is not None and not inout
        w = torch.full((M + gr, C + 2 * g), NAN if self.input else SENT, dtype=dtype)
        if body is None:
            w[:M, g:g + C] = NAN
        else:
            assert body.dtype == dtype and tuple(body.shape) == (M, C), (body.dtype, tuple(body.shape), M, C)
            w[:M, g:g + C] = body
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + g * self.t.element_size()
        self.ld = C + 2 * g

    def reset(self):
        self.t.copy_(self.init)

    def raw(self):
        return self.t[:self.M, self.g:self.g + self.C].cpu().contiguous()

    def untouched(self):
        return torch.equal(_bits(self.t), _bits(self.init))

    def guards_ok(self):
        if self.input:
            return self.untouched()
        a = self.t.clone()
        a[:self.M, self.g:self.g + self.C] = self.init[:self.M, self.g:self.g + self.C]
        return torch.equal(_bits(a), _bits(self.init))


class Pad(Slice):
    """a contiguous buffer of n elements of any float `dtype` between two pads of PADW elements (fp32 NCHW tensors, weight packs,
    the fixed-ld outputs of the input packs): input, output or inout as in Slice"""
    PADW = 64

    def __init__(self, n, dtype, body=None, inout=False):
        p = self.PADW
        self.M, self.C, self.g, self.n, self.input = 1, n, p, n, body is not None and not inout
        w = torch.full((n + 2 * p,), NAN if self.input else SENT, dtype=dtype)
        if body is None:
            w[p:p + n] = NAN
        else:
            assert body.dtype == dtype and body.numel() == n, (body.dtype, body.numel(), n)
            w[p:p + n] = body.reshape(-1)
        self.init = w.to(DEV)
        self.t = self.init.clone()
        self.ptr = self.t.data_ptr() + p * self.t.element_size()

    def raw(self):
        return self.t[self.g:self.g + self.n].cpu()

    def guards_ok(self):
        if self.input:
            return self.untouched()
        a = self.t.clone()
        a[self.g:self.g + self.n] = self.init[self.g:self.g + self.n]
        return torch.equal(_bits(a), _bits(self.init))


def _run_bits(what, fn, bufs, want, twice=True):
    """launch; guards of every Slice / Pad in `bufs`; no NaN; the BITS of each output equal those of want {buffer: reference in the
    storage type}; a second launch from the same start gives the same bytes"""
    fn()
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.guards_ok(), f"{what}: guards of buffer {i} changed"
    first = {}
    for b, ref in want.items():
        got = b.raw()
        assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} elements never written (or NaN read)"
        assert ref.dtype == got.dtype, (ref.dtype, got.dtype)
        ref = ref.reshape(got.shape)
        bad = _bits(got) != _bits(ref.contiguous())
        if bool(bad.any()):
            k = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ in their bits, first at {k}: "
                                 f"got {float(got[tuple(k)])!r}, want {float(ref[tuple(k)])!r}")
        first[b] = _bits(b.t).clone()
    if twice:
        for b in bufs:
            b.reset()
        fn()
        torch.cuda.synchronize()
        for b in want:
            assert torch.equal(_bits(b.t), first[b]), f"{what}: a second launch gives other bytes"


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * (i + 3) for i, k in enumerate(key)) % (2 ** 31))


def _f(t):
    return t.float().to(DEV)


def _fold(partial, rows, nq, C):
    """fp64 fold of the first `rows` partial rows: [nq, C]"""
    return partial.reshape(-1, nq, C)[:rows].sum(0)


class Ledger:
    """the coverage report of one test file: rows dict(launcher, dtype, branches, n, switch), appended to the file named by
    <prefix>_REPORT when the process is a child; <prefix>_SWITCH names the switch set the process runs under ('' = the parent)"""

    def __init__(self, prefix):
        self.prefix = prefix
        self.here = os.environ.get(prefix + "_SWITCH", "")
        self.report = os.environ.get(prefix + "_REPORT", "")
        self.results = []
        self.child_rows = []
        self.child_time = {}

    def mark(self, launcher, dtype, *branches, n=1):
        row = dict(launcher=launcher, dtype=_dn(dtype), branches=sorted(set(branches)), n=n, switch=self.here)
        self.results.append(row)
        if self.report:
            with open(self.report, "a") as f:
                f.write(json.dumps(row) + "\n")

    def run_child(self, test_file, switch, switch_env):
        """the same file in a fresh pytest process under `switch_env` (switches that are read once per process)"""
        fd, path = tempfile.mkstemp(suffix=".jsonl")
        os.close(fd)
        try:
            env = dict(os.environ, **{self.prefix + "_SWITCH": switch, self.prefix + "_REPORT": path}, **switch_env)
            t0 = time.time()
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(test_file), "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider"],
                               env=env, capture_output=True, text=True, timeout=300)
            self.child_time[switch] = time.time() - t0
            print(r.stdout[-3000:])
            assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
            with open(path) as f:
                rows = [json.loads(line) for line in f if line.strip()]
            assert rows, f"child {switch} ran no case"
            self.child_rows.extend(rows)
        finally:
            os.unlink(path)
