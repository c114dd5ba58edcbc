"""Float64 numpy restatement of the three formulas behind the per-pixel Z-maps, written as the header states them: the
chunked Chan update of a running mean / sum of squared deviations, the Z-map of a row averaged over the t-starts, and the separable
smoothing with the reflect boundary.  No import from the product.  tests/test_anomaly_z_maps_host.py holds THIS against numpy's
mean / var, ``np.pad(mode="symmetric")`` and ``scipy.ndimage.gaussian_filter``; the tests of the kernels compare with it.
"""

import numpy as np


def chan_update(values, n_prev=0, mean=None, m2=None):
    """One batch [B, ...] merged into (n, mean, m2): mb = sum / B, Mb = sum (v - mb)^2 in a second pass; the first batch sets the
    tables, a later one: delta = mb - mean, mean += delta B / n, m2 += Mb + delta^2 n_prev B / n with n = n_prev + B."""
    v = np.asarray(values, dtype=np.float64)
    B = v.shape[0]
    mb = v.sum(axis=0) / B
    Mb = ((v - mb) ** 2).sum(axis=0)
    if n_prev == 0:
        return B, mb, Mb
    n = n_prev + B
    delta = mb - np.asarray(mean, dtype=np.float64)
    return n, mean + delta * (B / n), np.asarray(m2, dtype=np.float64) + Mb + delta * delta * (n_prev * B / n)


def chan_chunks(values, splits):
    """The rows of `values` merged batch by batch, the batches `splits` rows long."""
    assert sum(splits) == len(values)
    n, mean, m2, at = 0, None, None, 0
    for b in splits:
        n, mean, m2 = chan_update(values[at:at + b], n, mean, m2)
        at += b
    return n, mean, m2


def floor_inv_std(std, rel_floor):
    """1 / max(std, rel_floor * the largest std of each (t, c) over the pixels) for std [n_t, C, H, W]."""
    std = np.asarray(std, dtype=np.float64)
    return 1.0 / np.maximum(std, rel_floor * std.max(axis=(2, 3), keepdims=True))


def zscore(values, mean, inv_std, weight=None):
    """out[b, ...] = weight * sum_t (values[b, t] - mean[t]) * inv_std[t]; weight defaults to 1 / n_t."""
    v = np.asarray(values, dtype=np.float64)
    w = 1.0 / v.shape[1] if weight is None else float(weight)
    return w * ((v - np.asarray(mean, dtype=np.float64)[None]) * np.asarray(inv_std, dtype=np.float64)[None]).sum(axis=1)


def refl(i, L):
    """scipy's mode="reflect" index (d c b a | a b c d | d c b a) for any integer i: m = i mod 2L, m < L ? m : 2L - 1 - m."""
    m = int(i) % (2 * L)
    return m if m < L else 2 * L - 1 - m


def gaussian_taps(sigma, truncate=4.0):
    """exp(-k^2 / 2 sigma^2), |k| <= radius = int(truncate * sigma + 0.5), normalised to sum 1 (float64)."""
    radius = int(truncate * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(k ** 2) / (2.0 * float(sigma) ** 2)) if radius else np.ones(1)
    return w / w.sum()


def blur(maps, taps):
    """[N, H, W]: tmp[y, x] = sum_k taps[k] in[refl(y + k - r, H), x], then out[y, x] = sum_k taps[k] tmp[y, refl(x + k - r, W)]."""
    x = np.asarray(maps, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    r = len(taps) // 2
    N, H, W = x.shape
    rows = np.array([[refl(y + k - r, H) for k in range(len(taps))] for y in range(H)])  # [H, K]
    cols = np.array([[refl(c + k - r, W) for k in range(len(taps))] for c in range(W)])  # [W, K]
    tmp = np.einsum("nykx,k->nyx", x[:, rows, :], taps)
    return np.einsum("nyxk,k->nyx", tmp[:, :, cols], taps)
