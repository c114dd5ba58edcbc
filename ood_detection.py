"""CLI of the scoring stage: results_*.csv -> per-t Z-scores -> AUROC.

Flag names / defaults follow /root/reference/ood_detection.py:15-37 (--t_skip is dead there
too, Q12).  The work is in ddpm_ood_amd/ood.py.
"""

import argparse
import warnings


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    for name, typ, default in (("seed", int, 2), ("output_dir", str, None), ("model_name", str, None),
                               ("max_t", int, 1000), ("min_t", int, 0), ("t_skip", int, 1)):
        p.add_argument(f"--{name}", type=typ, default=default)
    p.add_argument("--plot_target", default="mse", choices=["mse", "perceptual_difference", "mse+perceptual"],
                   help="extension: which Z-score feeds the AUROC (the reference hard-codes mse)")
    p.add_argument("--out_data", default=None,
                   help="extension: comma list of OOD set names (default: picked from --model_name)")
    p.add_argument("--score", default="reconstruction", choices=["reconstruction", "likelihood", "zmap", "pixel"],
                   help="extension: likelihood reads the likelihood_*.csv files of likelihood.py and ranks by NLL; zmap reads the "
                        "zmaps_*.npz files of reconstruct.py --anomaly_z_maps 1 and ranks by a reduction of the per-pixel Z-map; "
                        "pixel reads the pixels_*.npz files of reconstruct.py --pixel_metrics 1 and prints the pixel-level AUROC, "
                        "AP and Dice of the Z-map against the ground-truth masks")
    p.add_argument("--zmap_key", default="z_mse_map", choices=["z_mse_map", "z_lpips_map"],
                   help="--score zmap / pixel: which Z-map")
    p.add_argument("--pixel_include_in", type=int, default=0,
                   help="--score pixel: 1 pools the in set's pixels (pixels_in.npz) into the negatives")
    p.add_argument("--pixel_regions", type=int, default=0,
                   help="--score pixel: 1 also reads the regions_*.npz files of reconstruct.py --pixel_regions 1 and prints the "
                        "region-overlap score (AUPRO) and, per fixed threshold, region recall, component precision and their F1")
    p.add_argument("--pixel_pro_fpr", type=float, default=0.3,
                   help="--score pixel --pixel_regions 1: the false-positive rate up to which the region-overlap curve is integrated")
    p.add_argument("--pixel_calibrated", type=int, default=0,
                   help="--score pixel: 1 also reads calibration.npz and the calibrated_*.npz files of reconstruct.py "
                        "--pixel_calibrate_fpr and prints, per target rate, the threshold calibrated on the validation set, the rate "
                        "it reaches there and on the in set (pixels_in.npz), the pooled and the mean per-image Dice and, with "
                        "--pixel_regions 1, the component scores")
    p.add_argument("--pixel_segmented", type=int, default=0,
                   help="--score pixel: 1 also reads the segments_*.npz files of reconstruct.py --pixel_segment 1 (the out set's and "
                        "segments_in.npz) and prints, per threshold, the Dice, the component scores and the in-set false-positive "
                        "rate of the post-processed segmentations and what the size filter removed")
    p.add_argument("--zmap_reduce", default="mean", choices=["mean", "max"], help="--score zmap: mean or maximum over the pixels")
    return p.parse_args(argv)


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    args = parse_args()
    from ddpm_ood_amd import ood

    for model in args.model_name.split(","):
        args.model_name = model
        run = {"likelihood": ood.main_likelihood, "zmap": ood.main_zmaps, "pixel": ood.main_pixels}.get(args.score, ood.main)
        run(args, out_data=args.out_data.split(",") if args.out_data else None)
