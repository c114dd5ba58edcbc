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


# ---- thresholds calibrated on the validation set (``--pixel_calibrate_fpr``) -------------------------
# The validation set's leave-one-out Z-maps (``ops.map_zscore_loo``) are binned like every other set's; a threshold is the bin edge
# above which at most a fraction f of those healthy pixels falls.  Bin edges on purpose: the pooled TP / FP / FN at a calibrated
# threshold, and its realised false-positive rate on the in set, are sums over the histograms pixels_<name>.npz already holds.

CALIBRATE_FLAG = "--pixel_calibrate_fpr"
BUDGET_FLAG = "--pixel_calibrate_budget_gb"
CALIBRATION_FILE = "calibration.npz"
DEFAULT_BUDGET_GB = 8.0


def thresholds_from_hist(hist_negatives, lo: float, hi: float, fprs):
    """(bin indices int64 [F], thresholds float64 [F]) from the histogram [nbins + 1] of healthy pixels (the last column, the NaN
    pixels, is left out): with c_k the pixels of bins >= k and N the scored pixels, k* is the smallest k with c_k / N <= f and the
    threshold lo + k* step.  k* = nbins (more than f of the pixels lie in the last bin, which takes everything from hi on) is a
    ValueError that names --pixel_range, as are an empty histogram, a target outside (0, 1) and other than 1 .. 8 targets."""
    h = np.asarray(hist_negatives)
    if h.ndim != 1 or h.shape[0] < 2:
        raise ValueError(f"thresholds_from_hist wants one histogram [nbins + 1] (the last column the NaN pixels), got {h.shape}")
    if (h < 0).any():
        raise ValueError("a histogram holds counts: negative entry")
    f = np.asarray(fprs, dtype=np.float64).reshape(-1)
    if not 1 <= len(f) <= MAX_THRESHOLDS:
        raise ValueError(f"{CALIBRATE_FLAG} takes 1 .. {MAX_THRESHOLDS} target rates, got {len(f)}")
    if not all(0.0 < v < 1.0 for v in f):
        raise ValueError(f"{CALIBRATE_FLAG}: every target false-positive rate must lie in (0, 1), got {f.tolist()}")
    nbins = h.shape[0] - 1
    scored = h[:-1].astype(np.int64)
    N = int(scored.sum())
    if N == 0:
        raise ValueError(f"{CALIBRATE_FLAG}: the validation histogram holds no scored pixel: nothing to calibrate on")
    above = np.concatenate([np.cumsum(scored[::-1])[::-1], [0]]).astype(np.float64) / N  # c_k / N, k = 0 .. nbins (not increasing)
    ks = np.asarray([int(np.argmax(above <= v)) for v in f], dtype=np.int64)
    if (ks >= nbins).any():
        worst = float(f[ks >= nbins].min())
        raise ValueError(f"{CALIBRATE_FLAG}: more than {worst:g} of the validation pixels lie in the last bin (Z >= "
                         f"{float(lo) + (nbins - 1) * (float(hi) - float(lo)) / nbins:g}): no bin edge reaches that rate; widen "
                         f"--pixel_range beyond {hi:g}")
    return ks, float(lo) + ks * ((float(hi) - float(lo)) / nbins)


def reached_fpr(hist_negatives, ks):
    """c_k / N of ``thresholds_from_hist`` at the bin indices ``ks``: the rate a calibrated threshold reaches on that histogram."""
    scored = np.asarray(hist_negatives)[..., :-1].astype(np.float64)
    return np.asarray([scored[..., int(k):].sum() for k in np.asarray(ks).reshape(-1)]) / scored.sum()


def parse_fprs(text):
    """"0.05,0.01" (or a sequence of numbers) -> [0.05, 0.01]; 1 .. 8 targets, each in (0, 1)."""
    if isinstance(text, str):
        text = [s for s in text.split(",") if s.strip()]
    try:
        f = [float(v) for v in text]
    except (TypeError, ValueError):
        raise ValueError(f"{CALIBRATE_FLAG} must be a comma list of numbers, got {text!r}") from None
    if not 1 <= len(f) <= MAX_THRESHOLDS:
        raise ValueError(f"{CALIBRATE_FLAG} takes 1 .. {MAX_THRESHOLDS} target rates, got {len(f)}")
    if not all(0.0 < v < 1.0 for v in f):
        raise ValueError(f"{CALIBRATE_FLAG}: every target false-positive rate must lie in (0, 1), got {f}")
    return f


def check_calibration_flags(anomaly_z_maps, fprs, budget_gb=DEFAULT_BUDGET_GB):
    """What ``Reconstruct`` refuses at construction when ``--pixel_calibrate_fpr`` is given (no device needed).  Returns (the
    target rates, the budget in bytes)."""
    if not anomaly_z_maps:
        raise ValueError(f"{CALIBRATE_FLAG} calibrates thresholds of the Z-maps: it needs --anomaly_z_maps 1")
    try:
        budget = float(budget_gb)
    except (TypeError, ValueError):
        raise ValueError(f"{BUDGET_FLAG} is a number of GiB, got {budget_gb!r}") from None
    if not budget > 0 or not np.isfinite(budget):
        raise ValueError(f"{BUDGET_FLAG} must be a positive number of GiB, got {budget_gb}")
    return parse_fprs(fprs), int(budget * (1 << 30))


def check_budget(rows: int, n_t: int, *extent_and_budget, flags=(CALIBRATE_FLAG, BUDGET_FLAG)):
    """``check_budget(rows, n_t, H, W, budget_bytes)``, or ``(rows, n_t, D, H, W, budget_bytes)`` for volumes: the bytes of the
    validation rows a rank keeps on the device for the leave-one-out pass (rows x n_t x 2 x the extent, fp32), or ValueError when
    they exceed the budget.  ``flags``: the calibration flag and its budget flag the message names."""
    *extent, budget_bytes = extent_and_budget
    if len(extent) < 2:
        raise TypeError("check_budget(rows, n_t, *extent, budget_bytes): an extent of two or three numbers")
    need = int(rows) * int(n_t) * 2 * int(np.prod([int(e) for e in extent], dtype=object)) * 4
    if need > int(budget_bytes):
        shape = " x ".join(str(int(e)) for e in extent)
        raise ValueError(f"{flags[0]}: keeping the per-t maps of {rows} validation images ({rows} x {n_t} x 2 x {shape} fp32 "
                         f"= {need / (1 << 30):.3f} GiB on this rank) exceeds the budget of {budget_bytes / (1 << 30):.3f} GiB: raise "
                         f"{flags[1]}, use more ranks or truncate the set with --first_n_val")
    return need


CALIBRATION_KEYS = ("t", "n", "fpr", "bin", "thresholds", "hist", "lo", "hi", "nbins", "sigma", "rel_floor", "channels")


def calibration_tables(hist, t_values, n, fprs, lo, hi, nbins, sigma, rel_floor):
    """The contents of ood/calibration.npz from the validation set's histogram int64 [2, nbins + 1] (one row per channel)."""
    hist = np.asarray(hist).astype(np.int64)
    if hist.shape != (2, int(nbins) + 1):
        raise ValueError(f"a calibration histogram is [2, nbins + 1] (one row per channel), got {hist.shape} for nbins = {nbins}")
    got = [thresholds_from_hist(hist[c], lo, hi, fprs) for c in range(2)]
    return {"t": np.asarray([int(t) for t in t_values], dtype=np.int64), "n": np.int64(n), "fpr": np.asarray(fprs, dtype=np.float64),
            "bin": np.stack([g[0] for g in got]).astype(np.int64), "thresholds": np.stack([g[1] for g in got]).astype(np.float32),
            "hist": hist, "lo": np.float64(lo), "hi": np.float64(hi), "nbins": np.int64(nbins), "sigma": np.float64(sigma),
            "rel_floor": np.float64(rel_floor), "channels": np.asarray(CHANNELS)}


def load_calibration(path, t_values=None, lo=None, hi=None, nbins=None, sigma=None, rel_floor=None, fprs=None):
    """The dict of a ``calibration.npz``.  Each of the run's settings that is given must equal the file's, else ValueError; a
    missing file is a FileNotFoundError that names the flag that writes it."""
    from pathlib import Path

    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"no {path}: reconstruct.py {CALIBRATE_FLAG} (with --run_val 1) writes it")
    with np.load(path) as z:
        missing = [k for k in CALIBRATION_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path} lacks {missing}: no calibration file")
        cal = {k: z[k] for k in CALIBRATION_KEYS}
    F = len(cal["fpr"])
    if cal["bin"].shape != (2, F) or cal["thresholds"].shape != (2, F) or cal["hist"].shape != (2, int(cal["nbins"]) + 1):
        raise ValueError(f"{path}: tables of {cal['bin'].shape}, {cal['thresholds'].shape} and {cal['hist'].shape} for {F} targets "
                         f"and {int(cal['nbins'])} bins are no calibration")
    if t_values is not None and [int(t) for t in t_values] != [int(t) for t in cal["t"]]:
        raise ValueError(f"{path} was calibrated on the t-starts {[int(t) for t in cal['t']]}, this run has {[int(t) for t in t_values]}")
    if (lo is not None and float(lo) != float(cal["lo"])) or (hi is not None and float(hi) != float(cal["hi"])):
        raise ValueError(f"{path} holds the range [{float(cal['lo'])}, {float(cal['hi'])}), this run's --pixel_range is [{lo}, {hi})")
    if nbins is not None and int(nbins) != int(cal["nbins"]):
        raise ValueError(f"{path} holds {int(cal['nbins'])} bins, this run's --pixel_bins is {nbins}")
    if sigma is not None and float(sigma) != float(cal["sigma"]):
        raise ValueError(f"{path} was calibrated with --anomaly_z_sigma {float(cal['sigma'])}, this run has {sigma}")
    if rel_floor is not None and float(rel_floor) != float(cal["rel_floor"]):
        raise ValueError(f"{path} was calibrated with --anomaly_z_std_floor {float(cal['rel_floor'])}, this run has {rel_floor}")
    if fprs is not None and [float(v) for v in fprs] != [float(v) for v in cal["fpr"]]:
        raise ValueError(f"{path} holds the target rates {[float(v) for v in cal['fpr']]}, this run's {CALIBRATE_FLAG} is "
                         f"{[float(v) for v in fprs]}")
    return cal


# ---- region-level metrics (``--pixel_regions 1``) ----------------------------------------------------
# The device side (``ops.map_label`` / ``map_region_overlap`` / ``map_component_counts``) leaves the number of ground-truth
# regions per image, the overlap table float64 [nbins + 1] = sum over the regions of (the region's pixels in the bin) / (its
# pixels) with the NaN pixels in the last column, and per image and threshold (hit, pred, false_pred).

REGION_FLAG = "--pixel_regions 1"
DEFAULT_CONNECTIVITY, DEFAULT_PRO_FPR = 8, 0.3
MAX_REGION_PIXELS = 16384  # (ops.MAP_LABEL_MAX_PIXELS)


def pro_curve(overlap, regions_total, hist):
    """(fpr, pro), float64 [nbins + 1], entry j for k = nbins - j (from (0, 0) at k = nbins: nothing predicted) with "predicted at
    k" = bin >= k:
    PRO_k = (1 / R) sum_{k <= b < nbins} overlap[b], the mean over the R regions of the fraction of a region predicted, and
    FPR_k = fp_k / negatives from row 0 of the [2, nbins + 1] histogram.  R == 0: ValueError; no negative pixel: fpr is NaN."""
    w = np.asarray(overlap, dtype=np.float64)
    h = _scored(hist)
    if w.ndim != 1 or w.shape[0] != h.shape[1] + 1:
        raise ValueError(f"an overlap table is [nbins + 1] beside a histogram [2, nbins + 1], got {w.shape} and {np.asarray(hist).shape}")
    R = int(regions_total)
    if R <= 0:
        raise ValueError("region metrics: no ground-truth region")
    pro = np.concatenate([[0.0], np.cumsum(w[:-1][::-1])]) / R  # entry j: k = nbins - j
    neg = h[0].sum()
    fp = np.concatenate([[0.0], np.cumsum(h[0][::-1])])
    fpr = fp / neg if neg > 0 else np.full_like(fp, np.nan)
    return fpr, pro


def aupro(overlap, regions_total, hist, fpr_limit: float = DEFAULT_PRO_FPR) -> float:
    """The trapezoid of PRO over FPR on [0, fpr_limit], the segment that crosses the limit cut there by linear interpolation,
    divided by fpr_limit: 1 for a perfect map.  NaN without a negative pixel."""
    fpr_limit = float(fpr_limit)
    if not 0.0 < fpr_limit <= 1.0:
        raise ValueError(f"aupro: fpr_limit must lie in (0, 1], got {fpr_limit}")
    fpr, pro = pro_curve(overlap, regions_total, hist)
    if np.isnan(fpr).any():
        return float("nan")
    area = 0.0
    for j in range(1, len(fpr)):
        x0, x1, y0, y1 = fpr[j - 1], fpr[j], pro[j - 1], pro[j]
        if x1 <= fpr_limit:
            area += (x1 - x0) * (y0 + y1) * 0.5
        else:
            if x0 < fpr_limit:
                y_cut = y0 + (y1 - y0) * (fpr_limit - x0) / (x1 - x0)
                area += (fpr_limit - x0) * (y0 + y_cut) * 0.5
            break
    return float(area / fpr_limit)


def component_scores(components, regions):
    """From integer ``components`` [N, K, 3] = (hit, pred, false_pred) and ``regions`` [N]: dict of float64 [K] arrays --
    ``region_recall`` = sum hit / sum regions (NaN without a region), ``component_precision`` = 1 - sum false_pred / sum pred
    (1 when nothing is predicted), ``component_f1`` of the two (0 when both are 0) and ``false_per_image`` = sum false_pred / N."""
    c = np.asarray(components, dtype=np.float64)
    r = np.asarray(regions, dtype=np.float64).reshape(-1)
    if c.ndim != 3 or c.shape[2] != 3 or c.shape[0] != r.shape[0] or c.shape[0] == 0:
        raise ValueError(f"components are [N, K, 3] (hit, pred, false_pred) beside regions [N], got {c.shape} and {r.shape}")
    hit, pred, false_pred = c[..., 0].sum(axis=0), c[..., 1].sum(axis=0), c[..., 2].sum(axis=0)
    total = r.sum()
    recall = hit / total if total > 0 else np.full_like(hit, np.nan)
    precision = np.where(pred > 0, 1.0 - false_pred / np.where(pred > 0, pred, 1.0), 1.0)
    den = recall + precision
    f1 = np.where(den > 0, 2.0 * recall * precision / np.where(den > 0, den, 1.0), 0.0)
    return {"region_recall": recall, "component_precision": precision, "component_f1": f1, "false_per_image": false_pred / c.shape[0]}


def check_region_flags(pixel_metrics, connectivity=DEFAULT_CONNECTIVITY, pro_fpr=DEFAULT_PRO_FPR):
    """What ``Reconstruct`` refuses at construction when ``--pixel_regions 1`` is given (no device needed).  Returns
    (connectivity, pro_fpr)."""
    if not pixel_metrics:
        raise ValueError(f"{REGION_FLAG} adds to the pixel metrics: it needs {FLAG}")
    try:
        conn = int(connectivity)
        fpr = float(pro_fpr)
    except (TypeError, ValueError):
        raise ValueError(f"{REGION_FLAG}: --pixel_connectivity is 4 or 8 and --pixel_pro_fpr a number, got {connectivity!r} and "
                         f"{pro_fpr!r}") from None
    if conn != float(connectivity) or conn not in (4, 8):
        raise ValueError(f"{REGION_FLAG}: --pixel_connectivity must be 4 or 8, got {connectivity}")
    if not 0.0 < fpr <= 1.0:
        raise ValueError(f"{REGION_FLAG}: --pixel_pro_fpr must lie in (0, 1], got {pro_fpr}")
    return conn, fpr


def summarize_regions(overlap, regions, hist, components, fpr_limit: float = DEFAULT_PRO_FPR):
    """The numbers ``ood.score_pixels`` adds for one channel: aupro and ``component_scores`` as lists per threshold."""
    out = {"aupro": aupro(overlap, int(np.asarray(regions).sum()), hist, fpr_limit)}
    out.update({k: v.tolist() for k, v in component_scores(components, regions).items()})
    return out


def summarize(hist, lo: float, hi: float, counts=None, thresholds=None):
    """The numbers ``ood.score_pixels`` prints for one [2, nbins + 1] histogram (and the per-image counts [N, K, 3])."""
    nbins = np.asarray(hist).shape[1] - 1
    dice, at = best_dice(hist, lo, (float(hi) - float(lo)) / nbins)
    out = {"auroc": auroc(hist), "ap": average_precision(hist), "best_dice": dice, "best_dice_threshold": at,
           "nan_pixels": sum(nan_pixels(hist))}
    if counts is not None:
        out["mean_dice"] = dict(zip([float(t) for t in thresholds], dice_from_counts(counts).mean(axis=0).tolist()))
    return out


# ---- predicted segmentations (``--pixel_segment 1``) --------------------------------------------------
# The device side (``ops.map_median`` / ``map_segment``) leaves per image, channel and threshold the binary segmentation after
# the median filter and the removal of components below a minimum size, its (TP, FP, FN), (hit, pred, false_pred) and what the
# size filter dropped (components, pixels).

SEGMENT_FLAG = "--pixel_segment 1"
DEFAULT_MEDIAN, DEFAULT_MIN_COMPONENT = 3, 4
MEDIAN_SIZES = (1, 3, 5)


def check_segment_flags(args):
    """What ``Reconstruct`` refuses at construction when ``--pixel_segment 1`` is given, from the Namespace alone (no device needed).
    Returns (median, min_component, thresholds, connectivity)."""
    if not bool(getattr(args, "anomaly_z_maps", 0)):
        raise ValueError(f"{SEGMENT_FLAG} thresholds the Z-maps: it needs --anomaly_z_maps 1 (the raw maps have no fixed scale)")
    median, small = getattr(args, "pixel_median", DEFAULT_MEDIAN), getattr(args, "pixel_min_component", DEFAULT_MIN_COMPONENT)
    try:
        m, n = int(median), int(small)
        if m != float(median) or n != float(small):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{SEGMENT_FLAG}: --pixel_median and --pixel_min_component are integers, got {median!r} and {small!r}") from None
    if m not in MEDIAN_SIZES:
        raise ValueError(f"{SEGMENT_FLAG}: --pixel_median must be 1 (no filter), 3 or 5, got {median}")
    if not 1 <= n <= MAX_REGION_PIXELS:
        raise ValueError(f"{SEGMENT_FLAG}: --pixel_min_component must lie in 1 .. {MAX_REGION_PIXELS}, got {small}")
    thr = parse_thresholds(getattr(args, "pixel_thresholds", None) or DEFAULT_THRESHOLDS)
    if not 1 <= len(thr) <= MAX_THRESHOLDS or not all(np.isfinite(thr)):
        raise ValueError(f"{SEGMENT_FLAG}: --pixel_thresholds takes 1 .. {MAX_THRESHOLDS} finite numbers, got {thr}")
    conn = getattr(args, "pixel_connectivity", DEFAULT_CONNECTIVITY)
    if conn not in (4, 8):
        raise ValueError(f"{SEGMENT_FLAG}: --pixel_connectivity must be 4 or 8, got {conn}")
    return m, n, thr, int(conn)
