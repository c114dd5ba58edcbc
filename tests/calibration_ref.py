"""float64 restatements behind the thresholds calibrated on leave-one-out validation Z-maps: the brute force (row i
deleted, the others' mean and ddof-1 std recomputed), the closed form from (n, mean, M2), the formula of ``ops.map_zscore_loo``
in fp32 numpy, the quantile rule on a histogram, and the inputs the tests share.  numpy (and scipy for the smoothing) only."""

import numpy as np


def case_values(n, n_t=3, H=7, W=9, seed=0):
    """float32 [n, n_t, 2, H, W]: gamma-distributed values (as squared errors are), a scale per (t, channel), and one outlier
    column: pixel (0, 0) of every (t, channel) is 40 x larger in row 1, so that its leave-one-out Z is large there."""
    rng = np.random.default_rng(1000 * n + 10 * H + W + seed)
    v = rng.gamma(2.0, 1.0, size=(n, n_t, 2, H, W)) * rng.uniform(0.01, 1.0, size=(1, n_t, 2, 1, 1))
    v[1, :, :, 0, 0] *= 40.0
    return v.astype(np.float32)


def stats(values):
    """(n, mean, m2) in float64 over axis 0."""
    v = np.asarray(values, dtype=np.float64)
    mean = v.mean(axis=0)
    return v.shape[0], mean, ((v - mean) ** 2).sum(axis=0)


def floor_table(values, rel_floor=0.01):
    """floor[t, c] = rel_floor x the largest full-set std (ddof = 1) of that (t, c), float64 [n_t, 2]."""
    v = np.asarray(values, dtype=np.float64)
    return rel_floor * v.std(axis=0, ddof=1).max(axis=(2, 3))


def loo_brute(values, floor, rows=None):
    """Z-maps [len(rows), 2, H, W] in float64 by deleting row i: z_i = mean over t of (v_i - mean of the others) / max(std of the
    others (ddof = 1), floor[t, c])."""
    v = np.asarray(values, dtype=np.float64)
    floor = np.asarray(floor, dtype=np.float64)[:, :, None, None]
    out = []
    for i in (range(v.shape[0]) if rows is None else rows):
        others = np.delete(v, i, axis=0)
        z = (v[i] - others.mean(axis=0)) / np.maximum(others.std(axis=0, ddof=1), floor)
        out.append(z.mean(axis=0))
    return np.stack(out)


def loo_closed(values_rows, n, mean, m2, floor, weight=None):
    """The closed form in float64: rows [B, n_t, 2, H, W] that were counted in (n, mean, m2)."""
    v = np.asarray(values_rows, dtype=np.float64)
    d = v - np.asarray(mean, dtype=np.float64)[None]
    dl = d * (n / (n - 1.0))
    q = np.maximum(np.asarray(m2, dtype=np.float64)[None] - d * dl, 0.0)
    s = np.sqrt(q / (n - 2.0))
    z = dl / np.maximum(s, np.asarray(floor, dtype=np.float64)[None, :, :, None, None])
    return z.sum(axis=1) * (1.0 / v.shape[1] if weight is None else weight)


def loo_fp32(values_rows, n, mean32, m232, floor32, weight=None):
    """The kernel's formula, operation by operation, in fp32 numpy (every operation rounds once; t ascending)."""
    f = np.float32
    v, mean, m2 = (np.asarray(a, dtype=f) for a in (values_rows, mean32, m232))
    fl = np.asarray(floor32, dtype=f)[:, :, None, None]
    r1, r2 = f(n / (n - 1.0)), f(1.0 / (n - 2.0))
    acc = None
    for t in range(v.shape[1]):
        d = v[:, t] - mean[t]
        dl = d * r1
        q = np.maximum(m2[t] - d * dl, f(0))
        s = np.sqrt(q * r2)
        z = dl / np.maximum(s, fl[t])
        acc = z if acc is None else acc + z
    out = acc * f(1.0 / v.shape[1] if weight is None else weight)
    assert out.dtype == f
    return out


def quantile_bins(hist_negatives, fprs):
    """k* per target by the definition, one k at a time: the smallest k with (pixels of bins >= k) / N <= f."""
    h = np.asarray(hist_negatives)[:-1].astype(np.int64)
    N = int(h.sum())
    out = []
    for f in fprs:
        k = 0
        while int(h[k:].sum()) / N > f:
            k += 1
        out.append(k)
    return out


def blur(maps, sigma):
    """scipy's gaussian_filter over the last two axes of [..., H, W] float64 maps (mode="reflect", truncate 4)."""
    from scipy.ndimage import gaussian_filter

    m = np.asarray(maps, dtype=np.float64)
    flat = m.reshape((-1,) + m.shape[-2:])
    return np.stack([gaussian_filter(p, sigma, mode="reflect", truncate=4.0) for p in flat]).reshape(m.shape)


def bin_of(z, lo, hi, nbins):
    """The bin of ``ops.map_mask_hist`` in fp32: (v - lo) * inv_step, clamped; NaN -> nbins."""
    f = np.float32
    b = (np.asarray(z, dtype=f) - f(lo)) * f(nbins / (hi - lo))
    out = np.clip(np.nan_to_num(b, nan=0.0, posinf=nbins, neginf=-1), 0, nbins - 1).astype(np.int64)
    out[np.isnan(b)] = nbins
    return out
