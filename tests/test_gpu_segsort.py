"""GPU: mi355_segsort_f32 (csrc/segsort.hip) against np.argsort(kind="stable") — integer equality, no tolerance — at every length
around the wave, the scan block and the tile, on key sets where every radix digit decides an order; bit-reproducible; writes nothing
outside perm and ws; a NaN-bearing input still gives a permutation."""
import numpy as np
import pytest
import torch

import lovasz_ref as R
from mi355.lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lib.raw("mi355_segsort_tile")()
GUARD = 64


def op_sort(keys):
    """keys: host fp32 [S, len] -> (perm tensor, keys-on-device-after, guards intact).  ws and perm sit between guard regions."""
    S, n = keys.shape
    need = lib.raw("mi355_segsort_ws_ints")(S, n)
    assert need > 0, lib.raw("mi355_last_error")()
    k = torch.from_numpy(keys).to(DEV).contiguous()
    k0 = k.clone()
    arena = torch.full((GUARD + need + GUARD + S * n + GUARD,), -7, dtype=torch.int32, device=DEV)
    ws = arena[GUARD: GUARD + need]
    perm = arena[GUARD + need + GUARD: GUARD + need + GUARD + S * n]
    lib.mi355_segsort_f32(k, S, n, ws, need, perm)
    torch.cuda.synchronize()
    guards = torch.cat([arena[:GUARD], arena[GUARD + need: GUARD + need + GUARD], arena[-GUARD:]])
    assert bool((guards == -7).all()), "a guard region next to ws / perm was written"
    assert torch.equal(k.view(torch.int32), k0.view(torch.int32)), "keys were modified"
    return perm.clone().view(S, n)


def key_sets(S, n, seed):
    rng = np.random.RandomState(seed)
    out = {"randn": rng.randn(S, n).astype(np.float32),
           "equal": np.full((S, n), 1.5, dtype=np.float32),
           "ascending": np.tile(np.arange(n, dtype=np.float32) - n // 2, (S, 1)),
           "descending": np.tile(np.arange(n, 0, -1, dtype=np.float32) - n // 2, (S, 1)),
           "quantised": (np.round(rng.randn(S, n) * 4) / 4).astype(np.float32)}      # multiples of 0.25, -0.0 among them
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, 3e38, -3e38, 1.0, -1.0, 1.1754944e-38, -1.1754944e-38],
                       dtype=np.float32)
    out["special"] = special[rng.randint(0, special.size, (S, n))]
    # keys that differ in ONE byte only: that radix digit alone decides.  Byte 3 holds the sign and seven exponent bits over a mantissa
    # whose top bit is clear: denormals of both signs among them, never an infinity or a NaN
    for byte in range(4):
        base = np.uint32(0x3f800000) if byte < 3 else np.uint32(0x00345678)
        bits = (base & ~np.uint32(0xff << (8 * byte))) | (rng.randint(0, 256, (S, n)).astype(np.uint32) << np.uint32(8 * byte))
        out[f"byte{byte}"] = bits.astype(np.uint32).view(np.float32)
    return out


LENGTHS = sorted({1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 4096, 65536})


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("S", [1, 3])
def test_order_is_numpys_stable_argsort(S, n):
    for name, keys in key_sets(S, n, 1000 * S + n).items():
        assert not np.isnan(keys).any(), name
        want = torch.from_numpy(R.argsort_ref(keys))
        got = op_sort(keys)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (name, S, n)
        assert torch.equal(op_sort(keys), got), ("second run differs", name, S, n)


@pytest.mark.parametrize("S,n", [(32, 65536), (1, 2097152)])
def test_benchmark_shapes(S, n):
    sets = key_sets(S, n, 5)
    for name in ("randn", "quantised"):
        keys = sets[name]
        want = torch.from_numpy(R.argsort_ref(keys))
        got = op_sort(keys)
        assert torch.equal(got.cpu(), want), (name, S, n)
        assert torch.equal(op_sort(keys), got), ("second run differs", name, S, n)


def test_python_surface_matches_the_abi():
    from utils import lovasz as UL
    keys = key_sets(3, 2 * T + 1, 9)["quantised"]
    want = torch.from_numpy(R.argsort_ref(keys))
    assert torch.equal(UL.segmented_argsort(torch.from_numpy(keys).to(DEV)).cpu(), want)
    assert torch.equal(UL.segmented_argsort(torch.from_numpy(keys[0]).to(DEV)).cpu(), want[0])
    with pytest.raises(ValueError):
        UL.segmented_argsort(torch.zeros(2, 3))


@pytest.mark.parametrize("S,n", [(3, 257), (2, 2 * T + 1)])
def test_nan_keys_still_give_a_permutation(S, n):
    keys = np.random.RandomState(3).randn(S, n).astype(np.float32)
    keys[:, ::7] = np.nan
    keys[0, 1] = -np.nan
    got = op_sort(keys).cpu().numpy()
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(n, dtype=np.int32), (S, 1)))
