"""Measurements behind DESIGN 3.23 (development / evidence tool; summary kept under profiles/pixel_metrics.md).

Kernels: ``ops.map_mask_hist`` (4 096 bins over [-16, 48)) and ``ops.map_mask_counts`` (3 thresholds) by themselves at the bench's
batch (1 024 maps of 32 x 32) and at 16 maps of 256 x 256, timed by the library's ProfScope (hipEvent-bracketed launches; the
histogram's figure covers both of its launches), the histogram with the wrapper's default ``parts`` and with 256 and 16.
Passes: ``Reconstruct.get_scores`` on ``synthetic.write_checkpoint``'s `small` model over 32 x 32 x 1 images at ``--batch``, one
validation pass for the statistics, then --runs alternating in-set passes (blobs, no masks) and out-set passes (lesion, masks
"auto") of two trainers, --anomaly_z_maps 1 alone and with --pixel_metrics 1.  --trained EPOCHS: tools/train_synthetic.py's
model scored on a lesion set (``trained_leg``).  Prints one JSON line.

    python tools/pixel_metrics_bench.py [--batch 1024] [--skip 4] [--runs 2] [--no_passes] [--trained 40]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from tools.anomaly_map_bench import make_args  # noqa: E402

LO, HI, BINS, THRESHOLDS = -16.0, 48.0, 4096, [2.0, 3.0, 4.0]


def kernel_times(lib, ops, dev):
    out = {}
    for N, H in ((1024, 32), (16, 256)):
        g = torch.Generator().manual_seed(N)
        z = (torch.randn(N, H * H, generator=g) * 2).to(dev)
        m = (torch.rand(N, H * H, generator=g) < 0.05).to(torch.uint8).to(dev)
        thr = torch.tensor(THRESHOLDS, device=dev)
        total = torch.zeros(2, BINS + 1, dtype=torch.int64, device=dev)
        for parts in (None, 256, 16):
            def once():
                ops.map_mask_hist(z, m, LO, HI, BINS, total=total, parts=parts)
                ops.map_mask_counts(z, m, thr)

            for _ in range(5):
                once()
            torch.cuda.synchronize()
            lib.ddpm_prof_enable(1)
            for _ in range(50):
                once()
            lib.ddpm_prof_enable(0)
            torch.cuda.synchronize()
            buf = ctypes.create_string_buffer(1 << 16)
            lib.ddpm_prof_report(buf, len(buf))
            prof = json.loads(buf.value.decode())
            n_parts = parts or ops.map_hist_parts(N * H * H)
            for k in ("map_mask_hist", "map_mask_counts"):
                v = prof[k]
                out[f"{k}_{N}x{H}x{H}_parts{n_parts}"] = {
                    "launches": v["launches"], "us_per_call": round(v["ms"] / v["launches"] * 1e3, 2),
                    "GBps": round(v["bytes"] / v["ms"] / 1e6, 1), "input_MB": round(5 * N * H * H / 1e6, 3),
                    "slab_MB": round(n_parts * 2 * (BINS + 1) * 4 / 1e6, 3) if k == "map_mask_hist" else 0.0}
    return out


def trained_leg(epochs, root):
    """tools/train_synthetic.py's model (`small`, 2 048 blobs, `epochs` epochs) on a lesion set of 64 images (mix = 25: discs 8 px
    across): pixel AUROC / AP / best Dice of both Z-maps without and with --anomaly_z_sigma 1.5, and the AUROC of the
    unquantised Z-values beside the 4 096-bin one."""
    import numpy as np
    from sklearn.metrics import roc_auc_score

    import reconstruct as rcli
    import train_ddpm
    from ddpm_ood_amd import data, ood
    from ddpm_ood_amd.train import DDPMTrainer
    from ddpm_ood_amd.trainer import Reconstruct

    sched = ["--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195"]
    common = ["--output_dir", str(root), "--model_name", "pixel_metrics_trained", "--is_grayscale", "1"]
    targs = train_ddpm.parse_args(common + sched + [
        "--training_ids", "synthetic:blobs:n=2048:seed=1", "--validation_ids", "synthetic:blobs:n=64:seed=10",
        "--n_epochs", str(epochs), "--batch_size", "64", "--eval_freq", "20", "--checkpoint_every", "0"])
    t0 = time.time()
    tr = DDPMTrainer(targs)
    tr.train(targs)
    out = {"epochs": epochs, "train_seconds": round(time.time() - t0, 1), "loss_first": round(float(tr.history[0][1]), 5),
           "loss_last": round(float(tr.history[-1][1]), 5), "sets": {}}
    del tr
    torch.cuda.empty_cache()
    masks = data.synthetic_masks("lesion", 64, 1, 32, seed=15, mix=25).numpy().reshape(-1)
    for k, sigma in enumerate((0.0, 1.5)):
        rargs = rcli.parse_args(common + sched + [
            "--validation_ids", "synthetic:blobs:n=64:seed=10", "--in_ids", "synthetic:blobs:n=64:seed=11",
            "--out_ids", "synthetic:lesion:n=64:seed=15:mix=25:name=LES", "--inference_skip_factor", "16", "--batch_size", "64",
            "--anomaly_z_maps", "1", "--pixel_metrics", "1", "--out_masks", "auto", "--anomaly_z_sigma", str(sigma),
            "--run_val", "0" if k else "1"])
        Reconstruct(rargs).reconstruct(rargs)
        ood_dir = Path(root) / "pixel_metrics_trained" / "ood"
        z = np.load(ood_dir / "zmaps_LES.npz")
        for key in ("z_mse_map", "z_lpips_map"):
            s = ood.score_pixels(ood_dir / "pixels_LES.npz", key=key)
            pooled = ood.score_pixels(ood_dir / "pixels_LES.npz", ood_dir / "pixels_in.npz", key=key)
            s["auroc_unquantised"] = float(roc_auc_score(masks, z[key].reshape(-1).astype(np.float64)))
            s["auroc_with_in_set"], s["ap_with_in_set"] = pooled["auroc"], pooled["ap"]
            s["mean_dice"] = {str(t): d for t, d in s["mean_dice"].items()}
            out["sets"][f"{key}_sigma{sigma}"] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trained", type=int, default=0, metavar="EPOCHS",
                    help="also train tools/train_synthetic.py's model for EPOCHS epochs and score a lesion set with it")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip", type=int, default=4, help="inference_skip_factor (4: the bench's 25 t-starts)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no_passes", action="store_true")
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops, synthetic
    from ddpm_ood_amd.data import get_data_loader
    from ddpm_ood_amd.trainer import Reconstruct

    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "inference_skip_factor": a.skip,
           "kernels": kernel_times(_lib.load(), ops, dev), "runs": []}
    if not a.no_passes:
        stdout = sys.stdout
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_checkpoint(Path(root) / "anomaly_map_bench", "small", 1, seed=1)
            sys.stdout = open(os.devnull, "w")  # the trainer prints like the reference; keep stdout to ONE JSON line
            try:
                lesion = f"synthetic:lesion:n={a.batch}:size=32:channels=1:seed=1:mix=25"
                trainers = {}
                for px in (0, 1):
                    args = make_args(root, a.batch, a.batch, a.skip, 0, 1, 0.0)
                    args.pixel_metrics, args.run_out, args.out_ids, args.out_masks = px, 1, lesion, "auto"
                    trainers[px] = Reconstruct(args)
                    trainers[px].quiet = True
                loaders = {"val": get_data_loader(args.validation_ids, batch_size=a.batch, is_grayscale=True),
                           "in": get_data_loader(args.in_ids, batch_size=a.batch, is_grayscale=True),
                           "out": get_data_loader(lesion, batch_size=a.batch, is_grayscale=True, mask_ids="auto")}
                for ld in loaders.values():
                    ld.images = ld.images.to(dev)  # inputs resident in HBM before timing starts
                for px in (0, 1):
                    trainers[px].get_scores(loaders["val"], "val", a.skip)  # the statistics, and the warm-up of every shape
                for run in range(a.runs):
                    for name in ("in", "out"):
                        for px in (0, 1):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            rows = trainers[px].get_scores(loaders[name], name, a.skip)
                            torch.cuda.synchronize()
                            dt = time.perf_counter() - t0
                            assert (trainers[px].last_pixels is not None) == bool(px)
                            out["runs"].append({"pixel_metrics": px, "pass": name, "run": run, "reconstructions": len(rows),
                                                "seconds": round(dt, 4), "reconstructions_per_s": round(len(rows) / dt, 2)})
            finally:
                sys.stdout = stdout
        for name in ("in", "out"):
            best = {px: max(r["reconstructions_per_s"] for r in out["runs"] if r["pass"] == name and r["pixel_metrics"] == px)
                    for px in (0, 1)}
            out[f"value_{name}_off"], out[f"value_{name}_on"] = best[0], best[1]
            out[f"ratio_{name}_on_over_off"] = round(best[1] / best[0], 4)
        out["unit"] = "reconstructions/s"
    if a.trained:
        stdout = sys.stdout
        with tempfile.TemporaryDirectory() as root:
            sys.stdout = open(os.devnull, "w")
            try:
                out["trained"] = trained_leg(a.trained, root)
            finally:
                sys.stdout = stdout
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
