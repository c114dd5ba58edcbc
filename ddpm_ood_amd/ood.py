"""Scoring stage: results_*.csv -> per-t Z-scores -> AUROC.

Mirror of /root/reference/ood_detection.py:40-223 minus the plotting (:177-192) and the
MONAI imports it only uses for a step count (:65-71, restated with this package's
scheduler).  pandas / scikit-learn semantics are the reference's: drop_duplicates keep-first
(:54,144-145), strict MIN_T < t < MAX_T (:59-61), pandas std ddof=1 (:152-161), groupby mean
over t (:174), roc_auc_score(in=0, out=1) on the MSE Z-score (:195-206).
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pandas as pd
from sklearn.metrics import roc_auc_score

MEDNIST = ["AbdomenCT", "BreastMRI", "ChestCT", "CXR", "Hand", "HeadCT"]


def out_datasets_for(model: str):
    """/root/reference/ood_detection.py:91-135."""
    if "fashionmnist" in model:
        return ("MNIST", "FashionMNIST_vflip", "FashionMNIST_hflip")
    if "mnist" in model:
        return ("FashionMNIST", "MNIST_vflip", "MNIST_hflip")
    if "cifar10" in model:
        return ("SVHN", "CelebA", "CIFAR10_vflip", "CIFAR10_hflip")
    if "celeba" in model.lower():
        return ("CIFAR10", "SVHN", "CelebA_vflip", "CelebA_hflip")
    if "svhn" in model:
        return ("CIFAR10", "CelebA", "SVHN_vflip", "SVHN_hflip")
    for key, name in (("abdomenct", "AbdomenCT"), ("breastmri", "BreastMRI"), ("cxr", "CXR"),
                      ("chestct", "ChestCT"), ("hand", "Hand"), ("headct", "HeadCT")):
        if key in model:
            return tuple(d for d in MEDNIST if d != name)
    if "decathlon" in model or "Task01" in model:
        return tuple(f"Task{i:02d}" for i in range(2, 11))
    raise ValueError(f"Unknown dataset to select for run_dir {model}")


def count_model_evaluations(t_values, num_inference_steps: int = 100) -> int:
    """ood_detection.py:63-71: UNet evaluations needed for a set of start points."""
    ts = np.arange(0, num_inference_steps)[::-1] * (1000 // num_inference_steps)
    return int(sum((ts <= t).sum() for t in t_values))


TARGETS = ("perceptual_difference", "mse")


def _rows(df: pd.DataFrame, keep_t=None) -> pd.DataFrame:
    """One row per (image, t-start) -- a padded DDP shard repeats images, the first copy counts -- inside the t window."""
    rows = df[~df.duplicated(subset=["filename", "t"])]
    return rows if keep_t is None else rows[rows["t"].isin(keep_t)]


def score(val: pd.DataFrame, ind: pd.DataFrame, ood: pd.DataFrame, max_t: int = 1000, min_t: int = 0, plot_target: str = "mse"):
    """Z-scores and AUROC of one in- / out-of-distribution pair of result tables against the validation table
    (what /root/reference/ood_detection.py:141-206 computes per out-dataset).

    For every t-start inside the open window (min_t, max_t): the validation set's mean and sample standard deviation of each
    similarity column; every in / out row gets z = (x - mean_t) / std_t; an image's score is the mean of its z over the
    t-starts; AUROC with in = 0, out = 1.  Returns (rows with `val_mean_*`, `val_std_*`, `z_score_*` columns,
    per-image means, AUROC).  NaN rows (a genuine overflow, written as the reference would) are skipped by the per-t
    statistics and by an image's mean; an image with no finite row makes roc_auc_score raise, as it does for the reference."""
    val_rows = _rows(val)
    window = val_rows["t"][(val_rows["t"] > min_t) & (val_rows["t"] < max_t)].unique()
    stats = val_rows[val_rows["t"].isin(window)].groupby("t")[list(TARGETS)].agg(["mean", "std"])  # NaN-skipping, ddof = 1
    table = pd.concat((_rows(ind, window), _rows(ood, window)), ignore_index=True)
    for col in TARGETS:
        mu, sigma = table["t"].map(stats[(col, "mean")]), table["t"].map(stats[(col, "std")])
        table[f"val_mean_{col}"], table[f"val_std_{col}"] = mu.to_numpy(), sigma.to_numpy()
        table[f"z_score_{col}"] = ((table[col] - mu) / sigma).to_numpy()
    if plot_target == "mse+perceptual":
        table["z_score_mse+perceptual"] = table["z_score_mse"] + table["z_score_perceptual_difference"]
    per_image = table.groupby(["filename", "type"]).mean(numeric_only=True).reset_index()
    z = per_image[f"z_score_{plot_target}"].to_numpy()
    is_ood = (per_image["type"] == "out").to_numpy()
    known = is_ood | (per_image["type"] == "in").to_numpy()
    return table, per_image, roc_auc_score(is_ood[known].astype(int), z[known])


def score_likelihood(ind: pd.DataFrame, ood: pd.DataFrame, column: str = "nll"):
    """AUROC of the likelihood baseline (likelihood_*.csv of likelihood.py): one row per image -- a repeated filename counts
    once, the first copy, as in ``_rows`` -- in = 0, out = 1, and the score is the column itself: a higher NLL means more
    out-of-distribution.  Returns (the table of both sets, AUROC)."""
    table = pd.concat((ind[~ind.duplicated(subset=["filename"])].assign(type="in"),
                       ood[~ood.duplicated(subset=["filename"])].assign(type="out")), ignore_index=True)
    return table, roc_auc_score((table["type"] == "out").to_numpy().astype(int), table[column].to_numpy())


def main_likelihood(args, out_data=None):
    """``ood_detection.py --score likelihood``: the AUROC lines of ``main`` from likelihood_in.csv / likelihood_<name>.csv."""
    model = args.model_name
    run_dir = Path(args.output_dir) / model
    print(f"Run directory: {str(run_dir)}")
    out_dir = run_dir / "ood"
    print("Score is the likelihood column nll")
    if out_data is None:
        out_data = out_datasets_for(model)
    ind = pd.read_csv(out_dir / "likelihood_in.csv")
    scores = []
    for out_dataset in out_data:
        df, auc = score_likelihood(ind, pd.read_csv(out_dir / f"likelihood_{out_dataset}.csv"))
        print(f"n_in={(df['type'] == 'in').sum()} n_out={(df['type'] == 'out').sum()}")
        scores.append(auc)
    for o, s in zip(out_data, scores):
        print(f"AUC for {model} vs {o}: {s * 100:.1f}")
    print(f"Average AUC: {np.mean(scores) * 100:.1f}")
    return dict(zip(out_data, scores))


ZMAP_KEYS = ("z_mse_map", "z_lpips_map")
ZMAP_REDUCTIONS = ("mean", "max")


def score_zmaps(ind_npz, ood_npz, key: str = "z_mse_map", reduce: str = "mean"):
    """AUROC of the per-pixel Z-maps (zmaps_*.npz of ``reconstruct.py --anomaly_z_maps 1``): an image's score is the mean, or
    the maximum, of its Z-map ``key``; a repeated filename counts once, the first copy; in = 0, out = 1.  ``ind_npz`` /
    ``ood_npz``: a path or the loaded mapping.  Returns (the table of both sets, AUROC)."""
    if key not in ZMAP_KEYS:
        raise ValueError(f"score_zmaps: key must be one of {ZMAP_KEYS}, got {key!r}")
    if reduce not in ZMAP_REDUCTIONS:
        raise ValueError(f"score_zmaps: reduce must be one of {ZMAP_REDUCTIONS}, got {reduce!r}")
    frames = []
    for src, kind in ((ind_npz, "in"), (ood_npz, "out")):
        z = np.load(src) if isinstance(src, (str, Path)) else src
        maps = np.asarray(z[key], dtype=np.float64)
        flat = maps.reshape(maps.shape[0], -1)
        df = pd.DataFrame({"filename": [str(f) for f in z["filename"]], "type": kind,
                           "score": flat.mean(axis=1) if reduce == "mean" else flat.max(axis=1)})
        frames.append(df[~df.duplicated(subset=["filename"])])
    table = pd.concat(frames, ignore_index=True)
    return table, roc_auc_score((table["type"] == "out").to_numpy().astype(int), table["score"].to_numpy())


def main_zmaps(args, out_data=None):
    """``ood_detection.py --score zmap``: the AUROC lines of ``main`` from zmaps_in.npz / zmaps_<name>.npz."""
    model = args.model_name
    run_dir = Path(args.output_dir) / model
    print(f"Run directory: {str(run_dir)}")
    out_dir = run_dir / "ood"
    key, reduce = getattr(args, "zmap_key", "z_mse_map"), getattr(args, "zmap_reduce", "mean")
    print(f"Score is the {reduce} of the per-pixel Z-map {key}")
    if out_data is None:
        out_data = out_datasets_for(model)
    scores = []
    for out_dataset in out_data:
        df, auc = score_zmaps(out_dir / "zmaps_in.npz", out_dir / f"zmaps_{out_dataset}.npz", key, reduce)
        print(f"n_in={(df['type'] == 'in').sum()} n_out={(df['type'] == 'out').sum()}")
        scores.append(auc)
    for o, s in zip(out_data, scores):
        print(f"AUC for {model} vs {o}: {s * 100:.1f}")
    print(f"Average AUC: {np.mean(scores) * 100:.1f}")
    return dict(zip(out_data, scores))


def score_pixels(out_npz, in_npz=None, key: str = "z_mse_map", regions_npz=None, pro_fpr: float = 0.3):
    """Pixel-level metrics of one out set (pixels_<name>.npz of ``reconstruct.py --pixel_metrics 1``) for the Z-map ``key``: a dict
    of auroc, ap, best_dice, best_dice_threshold, nan_pixels and mean_dice {threshold: the mean per-image Dice}
    (``pixel_metrics.summarize``).  ``in_npz`` given: the in set's pixels are pooled in as negatives of the histogram (the
    per-image Dice stays the out set's).  ``regions_npz`` given (regions_<name>.npz of ``--pixel_regions 1``): also aupro (the
    region-overlap curve up to the false-positive rate ``pro_fpr``; the in set's pixels, when pooled, enter that rate only) and
    region_recall, component_precision, component_f1 {threshold: value}.  A path or the loaded mapping each."""
    from . import pixel_metrics as pm

    if key not in pm.KEYS:
        raise ValueError(f"score_pixels: key must be one of {pm.KEYS}, got {key!r}")
    c = pm.KEYS.index(key)
    z = np.load(out_npz) if isinstance(out_npz, (str, Path)) else out_npz
    hist = np.asarray(z["hist"])
    if hist.ndim != 3 or hist.shape[:2] != (2, 2) or hist.shape[2] != int(z["nbins"]) + 1:
        raise ValueError(f"score_pixels: hist of {hist.shape} for nbins = {int(z['nbins'])} is no [2, 2, nbins + 1] table")
    if in_npz is not None:
        zi = np.load(in_npz) if isinstance(in_npz, (str, Path)) else in_npz
        if (float(zi["lo"]), float(zi["hi"]), int(zi["nbins"])) != (float(z["lo"]), float(z["hi"]), int(z["nbins"])):
            raise ValueError("score_pixels: the in set's histogram has another range or another number of bins")
        hist = pm.pool_negatives(hist, np.asarray(zi["hist"]))
    out = pm.summarize(hist[c], float(z["lo"]), float(z["hi"]), np.asarray(z["counts"])[:, c], np.asarray(z["thresholds"]))
    if regions_npz is not None:
        zr = np.load(regions_npz) if isinstance(regions_npz, (str, Path)) else regions_npz
        if (float(zr["lo"]), float(zr["hi"]), int(zr["nbins"])) != (float(z["lo"]), float(z["hi"]), int(z["nbins"])) \
                or np.asarray(zr["overlap"]).shape != hist.shape[1:]:
            raise ValueError("score_pixels: the regions file has another range or another number of bins than the pixels file")
        r = pm.summarize_regions(np.asarray(zr["overlap"])[c], np.asarray(zr["regions"]), hist[c], np.asarray(zr["components"])[:, c],
                                 pro_fpr)
        thr = [float(t) for t in np.asarray(zr["thresholds"])]
        out["aupro"] = r["aupro"]
        for name in ("region_recall", "component_precision", "component_f1"):
            out[name] = dict(zip(thr, r[name]))
    return out


# the flags of reconstruct.py that write the same files for volumes: a missing file names both
VOXEL_FLAGS = {"--pixel_metrics 1": "--voxel_metrics 1", "--pixel_regions 1": "--voxel_regions 1",
               "--pixel_calibrate_fpr": "--voxel_calibrate_fpr", "--pixel_segment 1": "--voxel_segment 1"}


def _need(path, flag):
    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"no {path}: reconstruct.py {flag} writes it")
    return np.load(path)


def score_pixels_calibrated(out_dir, out_name, key: str = "z_mse_map", regions: bool = False):
    """The operating points calibrated on the validation set (``reconstruct.py --pixel_calibrate_fpr``) for one out
    set and the Z-map ``key``: a list, one dict per target rate, of ``fpr`` (the target), ``threshold``, ``val_fpr`` (the rate the
    threshold reaches on the validation set's leave-one-out Z-maps, from calibration.npz), ``in_fpr`` (the rate on the in set) and
    ``pooled_dice`` (both exact sums over the histograms of pixels_in.npz / pixels_<name>.npz from the threshold's bin on),
    ``mean_dice`` (the mean per-image Dice, calibrated_<name>.npz) and with ``regions`` region_recall, component_precision and
    component_f1 (calibrated_<name>.npz beside the region counts of regions_<name>.npz).  A missing file is a
    FileNotFoundError that names the reconstruct flag that writes it."""
    from . import pixel_metrics as pm

    if key not in pm.KEYS:
        raise ValueError(f"score_pixels_calibrated: key must be one of {pm.KEYS}, got {key!r}")
    c = pm.KEYS.index(key)
    out_dir = Path(out_dir)
    cal = pm.load_calibration(out_dir / pm.CALIBRATION_FILE)
    both = lambda flag: f"{flag} (volumes: {VOXEL_FLAGS[flag]})"  # noqa: E731
    px_out = _need(out_dir / f"pixels_{out_name}.npz", both(pm.FLAG))
    px_in = _need(out_dir / "pixels_in.npz", both(pm.FLAG))
    done = _need(out_dir / f"calibrated_{out_name}.npz", f"{both(pm.CALIBRATE_FLAG)} with {both(pm.FLAG)}")
    grid = (float(cal["lo"]), float(cal["hi"]), int(cal["nbins"]))
    for name, z in ((f"pixels_{out_name}.npz", px_out), ("pixels_in.npz", px_in)):
        if (float(z["lo"]), float(z["hi"]), int(z["nbins"])) != grid:
            raise ValueError(f"score_pixels_calibrated: {name} has another range or another number of bins than {pm.CALIBRATION_FILE}")
    if not np.array_equal(np.asarray(done["thresholds"]), np.asarray(cal["thresholds"])):
        raise ValueError(f"score_pixels_calibrated: calibrated_{out_name}.npz was counted at other thresholds than {pm.CALIBRATION_FILE} holds")
    ks = [int(k) for k in cal["bin"][c]]
    h_out = np.asarray(px_out["hist"])[c][:, :-1].astype(np.float64)
    h_in = np.asarray(px_in["hist"])[c][:, :-1].astype(np.float64).sum(axis=0)  # (an in set has no anomaly: every pixel a negative)
    val_fpr = pm.reached_fpr(cal["hist"][c], ks)
    mean_dice = pm.dice_from_counts(np.asarray(done["counts"])[:, c]).mean(axis=0)
    comp = None
    if regions:
        if "components" not in done.files:
            raise FileNotFoundError(f"calibrated_{out_name}.npz holds no component counts: reconstruct.py {pm.REGION_FLAG} with "
                                    f"{pm.CALIBRATE_FLAG} writes them")
        reg = _need(out_dir / f"regions_{out_name}.npz", pm.REGION_FLAG)
        comp = pm.component_scores(np.asarray(done["components"])[:, c], np.asarray(reg["regions"]))
    rows = []
    for j, k in enumerate(ks):
        tp, fp = h_out[1, k:].sum(), h_out[0, k:].sum()
        fn = h_out[1].sum() - tp
        den = 2.0 * tp + fp + fn
        row = {"fpr": float(cal["fpr"][j]), "threshold": float(cal["thresholds"][c, j]), "val_fpr": float(val_fpr[j]),
               "in_fpr": float(h_in[k:].sum() / h_in.sum()) if h_in.sum() > 0 else float("nan"),
               "pooled_dice": float(2.0 * tp / den) if den > 0 else 1.0, "mean_dice": float(mean_dice[j])}
        if comp is not None:
            row.update({name: float(comp[name][j]) for name in ("region_recall", "component_precision", "component_f1")})
        rows.append(row)
    return rows


def score_segments(out_npz, in_npz=None, key: str = "z_mse_map"):
    """The predicted segmentations of one out set (segments_<name>.npz of ``reconstruct.py --pixel_segment 1``) for the
    Z-map ``key``: a list, one dict per threshold, of ``threshold``, ``fpr`` (the target rate of a calibrated threshold, NaN for a
    fixed one), ``mean_dice`` (the mean per-image Dice), ``pooled_dice`` (of the summed TP, FP, FN), ``region_recall``,
    ``component_precision``, ``component_f1`` (``pixel_metrics.component_scores``), ``removed_components`` and ``removed_pixels``
    (what the size filter dropped, summed over the images).  ``in_npz`` given: also ``in_fpr``, the predicted pixels of the in
    set's segmentations over all its pixels.  A path or the loaded mapping each."""
    from . import pixel_metrics as pm

    if key not in pm.KEYS:
        raise ValueError(f"score_segments: key must be one of {pm.KEYS}, got {key!r}")
    c = pm.KEYS.index(key)
    z = np.load(out_npz) if isinstance(out_npz, (str, Path)) else out_npz
    pixels, components, removed = (np.asarray(z[k])[:, c].astype(np.int64) for k in ("pixels", "components", "removed"))
    if pixels.ndim != 3 or pixels.shape[2] != 3 or components.shape != pixels.shape or removed.shape != pixels.shape[:2] + (2,):
        raise ValueError(f"score_segments: pixels / components [N, 2, T, 3] and removed [N, 2, T, 2] expected, got "
                         f"{np.asarray(z['pixels']).shape}, {np.asarray(z['components']).shape} and {np.asarray(z['removed']).shape}")
    thresholds, fpr = np.asarray(z["thresholds"])[c], np.asarray(z["fpr"], dtype=np.float64)
    mean_dice = pm.dice_from_counts(pixels).mean(axis=0)
    pooled_dice = pm.dice_from_counts(pixels.sum(axis=0))
    comp = pm.component_scores(components, np.asarray(z["regions"]))
    in_fpr = None
    if in_npz is not None:
        zi = np.load(in_npz) if isinstance(in_npz, (str, Path)) else in_npz
        if not np.array_equal(np.asarray(zi["thresholds"]), np.asarray(z["thresholds"])) \
                or any(int(zi[k]) != int(z[k]) for k in ("median", "min_component", "connectivity")):
            raise ValueError("score_segments: the in set was segmented at other thresholds or with another filter")
        seg = np.asarray(zi["segmentation"])[:, c]
        # (seg: [N, T, H, W], or [N, T, D, H, W] of volumes: every pixel or voxel of the N items)
        in_fpr = np.asarray(zi["pixels"])[:, c, :, 1].astype(np.float64).sum(axis=0) / float(seg.shape[0] * np.prod(seg.shape[2:], dtype=np.int64))
    rows = []
    for j in range(pixels.shape[1]):
        row = {"threshold": float(thresholds[j]), "fpr": float(fpr[j]), "mean_dice": float(mean_dice[j]), "pooled_dice": float(pooled_dice[j]),
               **{name: float(comp[name][j]) for name in ("region_recall", "component_precision", "component_f1")},
               "removed_components": int(removed[:, j, 0].sum()), "removed_pixels": int(removed[:, j, 1].sum())}
        if in_fpr is not None:
            row["in_fpr"] = float(in_fpr[j])
        rows.append(row)
    return rows


def print_segments(model, o, out_dir, key):
    """``--pixel_segmented 1``: one line per threshold of ``score_segments`` for the out set ``o``."""
    from . import pixel_metrics as pm

    flag = f"{pm.SEGMENT_FLAG} (volumes: {VOXEL_FLAGS[pm.SEGMENT_FLAG]})"
    out = _need(out_dir / f"segments_{o}.npz", flag)
    rows = score_segments(out, _need(out_dir / "segments_in.npz", flag), key)
    print(f"Segmentations for {model} vs {o}: median {int(out['median'])}, components below {int(out['min_component'])} pixels removed "
          f"(connectivity {int(out['connectivity'])})")
    for r in rows:
        at = f"Z > {r['threshold']:.4g}" + ("" if np.isnan(r["fpr"]) else f" (validation FPR <= {r['fpr']:g})")
        print(f"Segmented for {model} vs {o} at {at}: mean image Dice {r['mean_dice']:.4f}, pooled Dice {r['pooled_dice']:.4f}, "
              f"recall {r['region_recall']:.4f}, component precision {r['component_precision']:.4f}, F1 {r['component_f1']:.4f}, "
              f"in-set FPR {r['in_fpr']:.5f}, removed {r['removed_components']} components / {r['removed_pixels']} pixels")
    return rows


def main_pixels(args, out_data=None):
    """``ood_detection.py --score pixel``: per out set the pixel AUROC, AP, best Dice and the mean per-image Dice at the fixed
    thresholds, from pixels_<name>.npz (and pixels_in.npz with --pixel_include_in 1).  --pixel_calibrated 1: also the operating
    points of ``score_pixels_calibrated``.  --pixel_segmented 1: also the lines of ``print_segments``."""
    model = args.model_name
    run_dir = Path(args.output_dir) / model
    print(f"Run directory: {str(run_dir)}")
    out_dir = run_dir / "ood"
    key = getattr(args, "zmap_key", "z_mse_map")
    include_in = bool(getattr(args, "pixel_include_in", 0))
    regions, pro_fpr = bool(getattr(args, "pixel_regions", 0)), float(getattr(args, "pixel_pro_fpr", 0.3))
    print(f"Pixel metrics of the Z-map {key}" + (", the in set's pixels pooled in as negatives" if include_in else ""))
    if out_data is None:
        out_data = out_datasets_for(model)
    got = {}
    for o in out_data:
        s = got[o] = score_pixels(out_dir / f"pixels_{o}.npz", out_dir / "pixels_in.npz" if include_in else None, key,
                                  out_dir / f"regions_{o}.npz" if regions else None, pro_fpr)
        print(f"Pixel AUC for {model} vs {o}: {s['auroc'] * 100:.2f}")
        print(f"Pixel AP for {model} vs {o}: {s['ap'] * 100:.2f}")
        print(f"Best Dice for {model} vs {o}: {s['best_dice']:.4f} at Z >= {s['best_dice_threshold']:.4f}")
        for t, d in s["mean_dice"].items():
            print(f"Mean image Dice for {model} vs {o} at Z > {t:g}: {d:.4f}")
        if s["nan_pixels"]:
            print(f"NaN pixels of {o} (not scored): {s['nan_pixels']}")
        if regions:
            print(f"AUPRO (FPR <= {pro_fpr:g}) for {model} vs {o}: {s['aupro'] * 100:.2f}")
            for t in s["region_recall"]:
                print(f"Regions for {model} vs {o} at Z > {t:g}: recall {s['region_recall'][t]:.4f}, component precision "
                      f"{s['component_precision'][t]:.4f}, F1 {s['component_f1'][t]:.4f}")
        if bool(getattr(args, "pixel_segmented", 0)):
            s["segmented"] = print_segments(model, o, out_dir, key)
        if bool(getattr(args, "pixel_calibrated", 0)):
            s["calibrated"] = score_pixels_calibrated(out_dir, o, key, regions)
            for r in s["calibrated"]:
                print(f"Calibrated for {model} vs {o} at validation FPR <= {r['fpr']:g}: Z > {r['threshold']:.4f} (validation FPR "
                      f"{r['val_fpr']:.5f}, in-set FPR {r['in_fpr']:.5f}), pooled Dice {r['pooled_dice']:.4f}, mean image Dice "
                      f"{r['mean_dice']:.4f}")
                if regions:
                    print(f"Calibrated regions for {model} vs {o} at validation FPR <= {r['fpr']:g}: recall {r['region_recall']:.4f}, "
                          f"component precision {r['component_precision']:.4f}, F1 {r['component_f1']:.4f}")
    return got


def main(args, out_data=None):
    model = args.model_name
    run_dir = Path(args.output_dir) / model
    print(f"Run directory: {str(run_dir)}")
    out_dir = run_dir / "ood"
    out_dir.mkdir(exist_ok=True)
    results_df_val = pd.read_csv(out_dir / "results_val.csv")
    t_all = results_df_val.drop_duplicates(subset=["filename", "t"], keep="first")["t"].unique()
    t_values = t_all[(t_all < args.max_t) & (args.min_t < t_all)]
    plot_target = getattr(args, "plot_target", "mse")
    print(f"SETTING MAX_T to {args.max_t} and T_SKIP to 1 with a total of {len(t_values)} starting points "
          f"{count_model_evaluations(t_values)} model evaluations")
    print(f"Plot target is {plot_target}")
    if out_data is None:
        out_data = out_datasets_for(model)
    scores = []
    for out_dataset in out_data:
        results_df_in = pd.read_csv(out_dir / "results_in.csv")
        results_df_out = pd.read_csv(out_dir / f"results_{out_dataset}.csv")
        df, df_mean, auc = score(results_df_val, results_df_in, results_df_out, args.max_t, args.min_t, plot_target)
        n_val = results_df_val["filename"].nunique()
        print(f"n_val={n_val} n_in={df.loc[df['type'] == 'in']['filename'].nunique()} "
              f"n_out={df.loc[df['type'] == 'out']['filename'].nunique()}")
        scores.append(auc)
    for o, s in zip(out_data, scores):
        print(f"AUC for {model} vs {o}: {s * 100:.1f}")
    print(f"Average AUC: {np.mean(scores) * 100:.1f}")
    return dict(zip(out_data, scores))
