"""numpy restatements of the pixel-metrics kernels (csrc/pixel_metrics.hip), for the tests.

``bin_index`` is the kernels' bin rule in float32, one rounding per operation: b = (v - lo) * inv_step with inv_step =
float32(nbins / (hi - lo)) formed in float64; NaN -> nbins; b < 0 -> 0; b >= nbins -> nbins - 1; else the truncation.  The
comparisons come before the conversion, as in the kernel."""

import numpy as np


def inv_step(lo, hi, nbins):
    return np.float32(nbins / (float(hi) - float(lo)))


def bin_index(values, lo, hi, nbins):
    v = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        b = (v - np.float32(lo)).astype(np.float32) * inv_step(lo, hi, nbins)
    b = b.astype(np.float32)
    out = np.empty(b.shape, dtype=np.int64)
    nan = np.isnan(b)
    low = ~nan & (b < np.float32(0))
    high = ~nan & (b >= np.float32(nbins))
    mid = ~(nan | low | high)
    out[nan], out[low], out[high] = nbins, 0, nbins - 1
    out[mid] = b[mid].astype(np.int64)  # (0 <= b < nbins: the truncation is exact)
    return out


def hist(maps, masks, lo, hi, nbins):
    """int64 [2, nbins + 1]: row = (mask != 0), column = bin_index."""
    k = bin_index(np.asarray(maps).reshape(-1), lo, hi, nbins)
    cls = (np.asarray(masks).reshape(-1) != 0).astype(np.int64)
    return np.bincount(cls * (nbins + 1) + k, minlength=2 * (nbins + 1)).reshape(2, nbins + 1).astype(np.int64)


def counts(maps, masks, thresholds):
    """int32 [N, K, 3]: TP, FP, FN of v > thr (float32 comparison; NaN predicted negative) against mask != 0, per row."""
    v = np.asarray(maps, dtype=np.float32)
    v = v.reshape(v.shape[0], -1)
    m = np.asarray(masks).reshape(v.shape[0], -1) != 0
    out = np.zeros((v.shape[0], len(thresholds), 3), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(np.asarray(thresholds, dtype=np.float32)):
            pred = v > t
            out[:, k, 0] = (pred & m).sum(axis=1)
            out[:, k, 1] = (pred & ~m).sum(axis=1)
            out[:, k, 2] = (~pred & m).sum(axis=1)
    return out


def case_values(N, P, lo, hi, nbins, seed):
    """float32 [N, P] maps and uint8 masks that visit every branch of the bin rule: normal values reaching beyond both ends of
    the range, exact bin edges (lo, hi and interior ones), +-inf, NaN; mask bytes 0 / 1 / 255."""
    rng = np.random.default_rng(seed)
    span = float(hi) - float(lo)
    v = (float(lo) - 0.1 * span + 1.2 * span * rng.random((N, P))).astype(np.float32)
    flat = v.reshape(-1)
    edges = (float(lo) + span * np.arange(nbins + 1) / nbins).astype(np.float32)
    special = np.concatenate([edges[rng.integers(0, nbins + 1, size=max(1, flat.size // 8))],
                              np.asarray([lo, hi, np.inf, -np.inf, np.nan], dtype=np.float32)])
    where = rng.permutation(flat.size)[:min(len(special), flat.size)]
    flat[where] = special[:len(where)]
    masks = rng.choice(np.asarray([0, 0, 1, 255], dtype=np.uint8), size=(N, P))
    return v, masks
