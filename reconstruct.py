"""CLI of the multi-t reconstruction path.

Flag names, types and defaults are the reference's (/root/reference/reconstruct.py:7-141) so
existing launch scripts keep working; the flags the reference parses but never reads
(--eval_checkpoint, --augmentation, --cache_data, --num_workers, --num_inference_steps;
SURVEY Q1/Q12) are accepted and ignored in the same way.  Extensions default to the
reference's behaviour.

    python reconstruct.py --output_dir=... --model_name=fashionmnist --validation_ids=... \
        --in_ids=... --out_ids=a.csv,b_vflip.csv --is_grayscale=1 \
        --beta_schedule=scaled_linear_beta --beta_start=0.0015 --beta_end=0.0195 \
        --inference_skip_factor=4
    torchrun --nproc_per_node=8 --master-addr 127.0.0.1 reconstruct.py ...   # one rank per MI355X
"""

import argparse
import ast

# (flag, type, default, help)
_FLAGS = [
    ("seed", int, 2, "seed of the per-image noise inputs"),
    ("output_dir", str, None, "root directory holding <model_name>/checkpoint.pth"),
    ("model_name", str, None, "run directory name"),
    ("validation_ids", str, None, "id file (or synthetic: spec) of the validation set"),
    ("in_ids", str, None, "id file of the in-distribution test set"),
    ("out_ids", str, None, "comma list of OOD id files; a _vflip / _hflip suffix adds the flip"),
    ("spatial_dimension", int, 2, "2 or 3"),
    ("image_size", None, None, "resize to this extent"),
    ("image_roi", ast.literal_eval, None, "central crop, tuple, -1 keeps a dimension"),
    ("latent_pad", ast.literal_eval, None, "F.pad-style padding of the latent"),
    ("vqvae_checkpoint", None, None, "VQ-VAE checkpoint for latent diffusion"),
    ("ddpm_checkpoint_epoch", None, None, "use checkpoint_<epoch>.pth instead of checkpoint.pth"),
    ("prediction_type", None, "epsilon", "epsilon or v_prediction"),
    ("model_type", None, "small", "small or big"),
    ("beta_schedule", None, "linear", "linear[_beta] | scaled_linear[_beta] | sigmoid[_beta] | cosine"),
    ("beta_start", float, 1e-4, "first beta"),
    ("beta_end", float, 2e-2, "last beta"),
    ("b_scale", float, 1, "data scale applied before noising"),
    ("snr_shift", float, 1, "SNR shift factor of the schedule"),
    ("simplex_noise", int, 0, "1: AnoDDPM simplex noise instead of Gaussian (score a model trained with it)"),
    ("batch_size", int, 256, "images per batch"),
    ("augmentation", int, 0, "ignored (as in the reference)"),
    ("cache_data", int, 1, "ignored: data is always cached"),
    ("num_workers", int, 8, "ignored: ingest is in-process"),
    ("first_n_val", None, None, "truncate the validation set"),
    ("first_n", None, None, "truncate every other set"),
    ("eval_checkpoint", None, None, "ignored (as in the reference)"),
    ("drop_last", None, False, "drop a ragged last batch"),
    ("is_grayscale", int, 0, "1-channel data"),
    ("run_val", int, 1, "score the validation set"),
    ("run_in", int, 1, "score the in-distribution set"),
    ("run_out", int, 1, "score the OOD sets"),
    ("num_inference_steps", int, 100, "ignored unless --honour_num_inference_steps=1 (reference hard-codes 100)"),
    ("inference_skip_factor", int, 1, "use every k-th timestep as a reconstruction start"),
]

_EXTENSIONS = [
    ("honour_num_inference_steps", int, 0, "1: really use --num_inference_steps (Q1)"),
    ("reset_scheduler_per_t", int, 0, "1: clear the PLMS history before each t-start (deviation, Q3)"),
    ("use_proj_attn", int, 0, "1: apply AttentionBlock.proj_attn (SURVEY A.3 open point)"),
    ("lpips_weights", None, None, "state_dict file with LPIPS-AlexNet weights"),
    ("anomaly_maps", int, 0, "1: also write ood/maps_<name>.npz, the per-pixel LPIPS and squared-error maps averaged over the "
                             "t-starts (2-D pixel-space models)"),
    ("anomaly_z_maps", int, 0, "1: also write ood/map_stats.npz (per-pixel mean and std of every t-start's maps over the "
                               "validation set) and ood/zmaps_<name>.npz, the in / out sets' maps as Z-scores against them, "
                               "averaged over the t-starts (2-D pixel-space models)"),
    ("anomaly_z_sigma", float, 0.0, "Gaussian smoothing of the Z-maps in pixels (0: none; below 4.125)"),
    ("anomaly_z_std_floor", float, 0.01, "a pixel's std is floored at this fraction of the largest std of its (t, channel)"),
    ("pixel_metrics", int, 0, "1 (with --anomaly_z_maps 1): also write ood/pixels_<name>.npz, the in / out sets' Z-maps against "
                              "ground-truth masks: a two-class histogram and per-image TP / FP / FN counts (ood_detection.py --score pixel)"),
    ("out_masks", str, None, "--pixel_metrics 1: comma list parallel to --out_ids; an entry is auto (a synthetic: spec), an .npz "
                             "with 'masks', a one-row CSV of mask files, or empty for a set without masks (all zero)"),
    ("pixel_bins", int, 4096, "--pixel_metrics 1: bins of the histogram (1 .. 8191)"),
    ("pixel_thresholds", str, "2,3,4", "--pixel_metrics 1: comma list of 1 .. 8 fixed Z thresholds of the per-image Dice"),
    ("pixel_regions", int, 0, "1 (with --pixel_metrics 1): also write ood/regions_<name>.npz, the masks' connected components "
                              "against the Z-maps: the per-region overlap table (AUPRO) and per-image component counts at the "
                              "fixed thresholds (ood_detection.py --score pixel --pixel_regions 1); planes up to 128 x 128"),
    ("pixel_pro_fpr", float, 0.3, "--pixel_regions 1: the false-positive rate up to which the region-overlap curve is integrated"),
    ("pixel_calibrate_fpr", str, None, "comma list of 1 .. 8 target false-positive rates in (0, 1), e.g. 0.05,0.01,0.001 (with "
                                       "--anomaly_z_maps 1): also write ood/calibration.npz, the Z thresholds above which those "
                                       "fractions of the validation set's leave-one-out Z-map pixels fall (bins of --pixel_range / "
                                       "--pixel_bins), and with --pixel_metrics 1 ood/calibrated_<name>.npz, the per-image counts "
                                       "at them (ood_detection.py --score pixel --pixel_calibrated 1); --run_val 0 reads the file"),
    ("pixel_calibrate_budget_gb", float, 8.0, "--pixel_calibrate_fpr: the most device memory (GiB per rank) the validation set's "
                                              "per-t maps may take while they wait for the leave-one-out pass"),
    ("pixel_segment", int, 0, "1 (with --anomaly_z_maps 1): also write ood/segments_<name>.npz, a predicted segmentation per image, "
                              "channel and threshold (--pixel_thresholds, then those of --pixel_calibrate_fpr): the Z-map median-"
                              "filtered, thresholded, its components below a minimum size removed (--pixel_connectivity), with its "
                              "pixel and component counts against the masks if there are any (ood_detection.py --score pixel "
                              "--pixel_segmented 1); planes up to 128 x 128"),
    ("pixel_median", int, 3, "--pixel_segment 1: the side of the median filter, 1 (none), 3 or 5"),
    ("pixel_min_component", int, 4, "--pixel_segment 1: predicted components of fewer pixels are removed (1 .. 16384; 1: none)"),
    ("anomaly_volume_maps", int, 0, "1 (--spatial_dimension 3, with or without --vqvae_checkpoint): also write ood/maps_<name>.npz, "
                                    "the per-voxel 2.5-D LPIPS and squared-error maps [N, D, H, W] of the decoded volume against "
                                    "the input, averaged over the t-starts"),
    ("anomaly_volume_z_maps", int, 0, "1 (--spatial_dimension 3): also write ood/map_stats.npz and ood/zmaps_<name>.npz for volumes, "
                                      "as --anomaly_z_maps 1 does for images; --anomaly_z_sigma smooths in 3-D, "
                                      "--anomaly_z_std_floor keeps its meaning (ood_detection.py --score zmap reads the files)"),
    ("anomaly_volume_views", str, "last", "the slice directions the LPIPS map of a volume is taken over: last (the view whose "
                                          "value is the perceptual_difference column) or all (the mean of the three views' maps)"),
    ("anomaly_volume_budget_gb", float, 8.0, "the most device memory (GiB) a batch's maps of volumes may take (batch x t-starts x 2 x "
                                             "D x H x W fp32 with --anomaly_volume_z_maps 1, plus the masks, labels, forests and "
                                             "tables of --voxel_metrics 1 / --voxel_regions 1 / --voxel_segment 1); a larger batch is refused"),
    ("voxel_metrics", int, 0, "1 (with --spatial_dimension 3 --anomaly_volume_z_maps 1): also write ood/pixels_<name>.npz for volumes, "
                              "the in / out sets' Z-maps against ground-truth masks voxel by voxel (--out_masks, --pixel_bins, "
                              "--pixel_range and --pixel_thresholds keep their meaning; ood_detection.py --score pixel reads the file)"),
    ("voxel_regions", int, 0, "1 (with --voxel_metrics 1): also write ood/regions_<name>.npz for volumes, the masks' 3-D connected "
                              "components against the Z-maps: the per-region overlap table (AUPRO) and per-volume component counts "
                              "(ood_detection.py --score pixel --pixel_regions 1)"),
    ("voxel_connectivity", int, 26, "--voxel_regions 1, --voxel_segment 1: the neighbours that join two voxels: 26, 18 or 6 "
                                    "(scipy.ndimage.generate_binary_structure(3, 3 | 2 | 1))"),
    ("voxel_pro_fpr", float, 0.3, "--voxel_regions 1: the false-positive rate up to which the region-overlap curve is integrated"),
    ("voxel_calibrate_fpr", str, None, "--pixel_calibrate_fpr for volumes (with --spatial_dimension 3 --anomaly_volume_z_maps 1): comma list "
                                       "of 1 .. 8 target false-positive rates in (0, 1); writes ood/calibration.npz from the validation "
                                       "volumes' leave-one-out Z-maps and, with --voxel_metrics 1, ood/calibrated_<name>.npz "
                                       "(ood_detection.py --score pixel --pixel_calibrated 1); --run_val 0 reads the file"),
    ("voxel_calibrate_budget_gb", float, 8.0, "--voxel_calibrate_fpr: the most device memory (GiB per rank) the validation volumes' "
                                              "per-t maps may take while they wait for the leave-one-out pass"),
    ("voxel_segment", int, 0, "1 (with --spatial_dimension 3 --anomaly_volume_z_maps 1): also write ood/segments_<name>.npz for volumes, a "
                              "predicted segmentation per volume, channel and threshold (--pixel_thresholds, then those of "
                              "--voxel_calibrate_fpr): the Z-map median-filtered, thresholded, its 3-D components below a minimum size "
                              "removed (--voxel_connectivity), with its voxel and component counts against the masks of "
                              "--voxel_metrics 1 --out_masks if there are any (ood_detection.py --score pixel --pixel_segmented 1)"),
    ("voxel_median", int, 3, "--voxel_segment 1: the side of the 3-D median filter, 1 (none) or 3"),
    ("voxel_min_component", int, 8, "--voxel_segment 1: predicted components of fewer voxels are removed (1 .. 2^31 - 1; 1: none)"),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default, text in _FLAGS:
        kw = {"default": default, "help": text}
        if typ not in (None, str):
            kw["type"] = typ
        parser.add_argument(f"--{name}", **kw)
    ext = parser.add_argument_group("extensions (defaults reproduce the reference)")
    for name, typ, default, text in _EXTENSIONS:
        kw = {"default": default, "help": text}
        if typ is not None:
            kw["type"] = typ
        ext.add_argument(f"--{name}", **kw)
    ext.add_argument("--pixel_range", type=float, nargs=2, default=[-16.0, 48.0], metavar=("LO", "HI"),
                     help="--pixel_metrics 1: the Z range the bins divide; values outside fall into the first / last bin")
    ext.add_argument("--pixel_connectivity", type=int, default=8, choices=[8, 4],
                     help="--pixel_regions 1: the neighbours that join two pixels (8: the 3 x 3 structure, 4: the cross)")
    ext.add_argument("--timestep_list", default="monai", choices=["monai", "diffusers"],
                     help="100-entry or 101-entry PLMS timestep list (Q9)")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    from ddpm_ood_amd.trainer import Reconstruct

    recon = Reconstruct(args)
    recon.reconstruct(args)
    import torch.distributed as dist

    if dist.is_initialized():
        dist.destroy_process_group()
