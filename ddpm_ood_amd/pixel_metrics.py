"""Pixel-level metrics of the Z-maps against ground-truth masks (``reconstruct.py --pixel_metrics 1``).

The device side (``ops.map_mask_hist`` / ``ops.map_mask_counts``) leaves two integer tables: the two-class histogram of every
pixel's Z-value over a fixed range, and per image and fixed threshold the TP / FP / FN pixel counts.  This module turns them into
numbers, in float64 numpy and nothing else.  A histogram is int [2, nbins + 1]: row 0 the pixels outside the mask, row 1 those
inside; column b < nbins the bin, column nbins the NaN pixels, which are reported (``nan_pixels``) and never scored.  The score
of a pixel is its bin index, so "predicted positive at k" means bin >= k, k = 0 .. nbins (k = nbins: nothing is predicted).

Degenerate histograms: without a positive pixel every function raises ValueError (no recall, no Dice).  Without a negative pixel
``auroc`` returns NaN (no false-positive rate); ``average_precision`` and ``best_dice`` need no negatives and are computed.
"""

from __future__ import annotations

import numpy as np

FLAG = "--pixel_metrics 1"
CHANNELS = ("lpips", "mse")  # (zmaps.CHANNELS: the first axis of the [2, 2, nbins + 1] table of a run)
KEYS = ("z_lpips_map", "z_mse_map")
DEFAULT_BINS, DEFAULT_RANGE, DEFAULT_THRESHOLDS = 4096, (-16.0, 48.0), (2.0, 3.0, 4.0)
MAX_BINS, MAX_THRESHOLDS = 8191, 8  # (ops.MAP_HIST_MAX_BINS, ops.MAP_COUNTS_MAX_K; this module imports no device code)


def _scored(hist):
    h = np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != 2 or h.shape[1] < 2:
        raise ValueError(f"a histogram is [2, nbins + 1] (negatives, positives; the last column the NaN pixels), got {h.shape}")
    if (h < 0).any():
        raise ValueError("a histogram holds counts: negative entry")
    return h[:, :-1].astype(np.float64)


def nan_pixels(hist):
    """(negatives, positives) among the NaN pixels: the last column."""
    h = np.asarray(hist)
    return int(h[0, -1]), int(h[1, -1])


def curves(hist):
    """Cumulated from the top bin: dict of tp, fp (float64 [nbins + 1], entry k = the pixels of bins >= k inside / outside the
    mask; entry nbins = 0), fn = P - tp, and the totals ``positives`` / ``negatives`` (NaN pixels left out)."""
    h = _scored(hist)
    pos, neg = h[1].sum(), h[0].sum()
    if pos == 0:
        raise ValueError("pixel metrics: the histogram holds no positive (masked) pixel")
    tp = np.concatenate([np.cumsum(h[1][::-1])[::-1], [0.0]])
    fp = np.concatenate([np.cumsum(h[0][::-1])[::-1], [0.0]])
    return {"tp": tp, "fp": fp, "fn": pos - tp, "positives": float(pos), "negatives": float(neg)}


def auroc(hist) -> float:
    """The trapezoid under (FPR, TPR) over k = nbins .. 0: ``roc_auc_score`` of the bin indices.  NaN without a negative pixel."""
    c = curves(hist)
    if c["negatives"] == 0:
        return float("nan")
    tpr, fpr = c["tp"][::-1] / c["positives"], c["fp"][::-1] / c["negatives"]
    return float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1])) * 0.5)


def average_precision(hist) -> float:
    """sum_k (R_k - R_{k+1}) P_k from the top bin down (R_nbins = 0): ``average_precision_score`` of the bin indices.  A k at
    which nothing is predicted adds no recall, so its (undefined) precision never counts."""
    c = curves(hist)
    tp, fp = c["tp"], c["fp"]
    pred = tp + fp
    precision = np.where(pred > 0, tp / np.where(pred > 0, pred, 1.0), 1.0)
    recall = tp / c["positives"]
    return float(np.sum((recall[:-1] - recall[1:]) * precision[:-1]))


def best_dice(hist, lo: float, step: float):
    """(the largest Dice 2 TP / (2 TP + FP + FN) over k = 0 .. nbins, its threshold lo + k * step); of equal ones the lowest k."""
    c = curves(hist)
    dice = 2.0 * c["tp"] / (2.0 * c["tp"] + c["fp"] + c["fn"])  # (the denominator is at least P > 0)
    k = int(np.argmax(dice))
    return float(dice[k]), float(lo) + k * float(step)


def dice_from_counts(counts):
    """Dice per entry of integer counts [..., 3] = (TP, FP, FN); an image with an empty mask and no predicted pixel has Dice 1."""
    c = np.asarray(counts, dtype=np.float64)
    if c.shape[-1] != 3:
        raise ValueError(f"counts are [..., 3] (TP, FP, FN), got {c.shape}")
    den = 2.0 * c[..., 0] + c[..., 1] + c[..., 2]
    return np.where(den > 0, 2.0 * c[..., 0] / np.where(den > 0, den, 1.0), 1.0)


def merge(*hists):
    """The sum of histograms of one shape ([2, nbins + 1] or a run's [2, 2, nbins + 1]) in int64: batches, ranks or sets pooled."""
    hs = [np.asarray(h) for h in hists]
    if not hs or any(h.shape != hs[0].shape or h.ndim < 2 or h.shape[-2] != 2 for h in hs):
        raise ValueError(f"merge wants histograms of one shape [..., 2, nbins + 1], got {[h.shape for h in hs]}")
    return np.sum([h.astype(np.int64) for h in hs], axis=0)


def pool_negatives(hist, in_hist):
    """``hist`` with every pixel of ``in_hist`` (an in-distribution set: no anomaly, whatever its class row says) added to the
    negatives."""
    h, g = np.asarray(hist).astype(np.int64), np.asarray(in_hist).astype(np.int64)
    if h.shape != g.shape or h.shape[-2] != 2:
        raise ValueError(f"pool_negatives wants two histograms of one shape [..., 2, nbins + 1], got {h.shape} and {g.shape}")
    out = h.copy()
    out[..., 0, :] += g[..., 0, :] + g[..., 1, :]
    return out


def parse_thresholds(text):
    """"2,3,4" (or a sequence of numbers) -> [2.0, 3.0, 4.0]."""
    if isinstance(text, str):
        text = [s for s in text.split(",") if s.strip()]
    try:
        return [float(v) for v in text]
    except (TypeError, ValueError):
        raise ValueError(f"{FLAG}: --pixel_thresholds must be a comma list of numbers, got {text!r}") from None


def check_flags(anomaly_z_maps, out_ids, out_masks=None, bins=DEFAULT_BINS, value_range=DEFAULT_RANGE,
                thresholds=DEFAULT_THRESHOLDS):
    """What ``Reconstruct`` refuses at construction when the flag is on (no device needed).  Returns (lo, hi, nbins, thresholds,
    masks): ``masks`` parallel to the entries of ``out_ids``, each "auto", a path, or None for a set without masks."""
    if not anomaly_z_maps:
        raise ValueError(f"{FLAG} evaluates the Z-maps: it needs --anomaly_z_maps 1 (the raw maps have no fixed scale)")
    try:
        nbins = int(bins)
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError(f"{FLAG}: --pixel_bins is an integer and --pixel_range two numbers, got {bins!r} and {value_range!r}") from None
    if nbins != float(bins) or not 1 <= nbins <= MAX_BINS:
        raise ValueError(f"{FLAG}: --pixel_bins must be an integer in 1 .. {MAX_BINS}, got {bins}")
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi) or not np.isfinite(np.float32(nbins / (hi - lo))) \
            or not np.isfinite(np.float32(lo)):
        raise ValueError(f"{FLAG}: --pixel_range must be two finite numbers LO < HI, got {lo} {hi}")
    thr = parse_thresholds(thresholds)
    if not 1 <= len(thr) <= MAX_THRESHOLDS or not all(np.isfinite(thr)):
        raise ValueError(f"{FLAG}: --pixel_thresholds takes 1 .. {MAX_THRESHOLDS} finite numbers, got {thr}")
    ids = [s for s in str(out_ids).split(",")] if out_ids else []
    if out_masks is None:  # (no flag: no set has masks)
        masks = [None] * len(ids)
    else:
        masks = [s.strip() or None for s in str(out_masks).split(",")]
    if len(masks) != len(ids):
        raise ValueError(f"{FLAG}: --out_masks lists {len(masks)} entries for the {len(ids)} of --out_ids (an empty entry stands "
                         f"for a set without masks)")
    return lo, hi, nbins, thr, masks


def summarize(hist, lo: float, hi: float, counts=None, thresholds=None):
    """The numbers ``ood.score_pixels`` prints for one [2, nbins + 1] histogram (and the per-image counts [N, K, 3])."""
    nbins = np.asarray(hist).shape[1] - 1
    dice, at = best_dice(hist, lo, (float(hi) - float(lo)) / nbins)
    out = {"auroc": auroc(hist), "ap": average_precision(hist), "best_dice": dice, "best_dice_threshold": at,
           "nan_pixels": sum(nan_pixels(hist))}
    if counts is not None:
        out["mean_dice"] = dict(zip([float(t) for t in thresholds], dice_from_counts(counts).mean(axis=0).tolist()))
    return out
