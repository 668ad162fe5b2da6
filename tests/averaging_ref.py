"""numpy restatement of csrc/weight_avg.hip (include/mi355conv.h, "weight averaging"): the coefficient schedule, the float32
update with every operation rounded on its own, the exchange, and the bias correction behind mi355.averaging.update_bn.
The GPU tests require the kernels' bytes to equal these."""
import numpy as np

EMA, EQUAL = 0, 1
f32 = np.float32


def ema_decay(t, decay, warmup):
    """the decay in force at update t (1-based), in double from the float32 arguments: timm.ModelEmaV3's warm-up
    min(decay, (1 + t) / (warmup + t)), the plain decay for warmup <= 0"""
    d = float(f32(decay))
    w = float(f32(warmup))
    if w > 0:
        d = min(d, (1.0 + t) / (w + t))
    return d


def coefficient(mode, t, decay=0.999, warmup=10.0):
    """-> (what, a): what = 'skip' (t < 1), 'copy' (equal average, t == 1) or 'update'; a float32, rounded once from double"""
    t = int(t)
    if t < 1:
        return "skip", f32(0)
    if mode == EQUAL:
        return ("copy" if t == 1 else "update"), f32(1.0 / t)
    return "update", f32(1.0 - ema_decay(t, decay, warmup))


def update(avg, p, mode, t, decay=0.999, warmup=10.0, found_inf=0.0):
    """one mi355_avg_update: a new float32 array (avg itself is not written)"""
    avg = np.asarray(avg, f32)
    p = np.asarray(p, f32)
    what, a = coefficient(mode, t, decay, warmup)
    if found_inf != 0 or what == "skip":
        return avg.copy()
    if what == "copy":
        return p.copy()
    with np.errstate(all="ignore"):
        diff = (p - avg).astype(f32)
        step = (a * diff).astype(f32)
        r = (avg + step).astype(f32)
    return np.where(diff == 0, avg, r).astype(f32)


def tick(count, found_inf=0.0):
    """mi355_step_tick"""
    return count if found_inf != 0 else count + 1


def bn_correction(k, momentum):
    """1 - (1 - momentum)^k in double, momentum widened from float32 as mi355_bn_finalize widens it"""
    return 1.0 - (1.0 - float(f32(momentum))) ** int(k)


def bn_debias(running, k, momentum):
    """mi355_bn_debias_table on one row -> (float32 result, the unrounded fp64 value)"""
    running = np.asarray(running, f32)
    if int(k) == 0:
        return running.copy(), running.astype(np.float64)
    exact = running.astype(np.float64) / bn_correction(k, momentum)
    return exact.astype(f32), exact


def bn_recurrence(batches, momentum, start=0.0):
    """mi355_bn_finalize's running-statistics recurrence from `start`: r = (float)((1 - m) r + m b) per batch statistic b"""
    m = float(f32(momentum))
    r = f32(start)
    for b in batches:
        r = f32((1.0 - m) * float(r) + m * float(b))
    return r


def bn_weighted_mean(batches, momentum):
    """what update_bn converges to, in fp64: sum_k w_k b_k with w_k = m (1 - m)^(K - 1 - k) / (1 - (1 - m)^K), k = 0 .. K - 1"""
    b = np.asarray(batches, np.float64)
    K = b.shape[0]
    m = float(f32(momentum))
    w = m * (1.0 - m) ** np.arange(K - 1, -1, -1, dtype=np.float64) / bn_correction(K, momentum)
    return np.tensordot(w, b, axes=(0, 0))
