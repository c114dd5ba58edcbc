"""Measurements behind DESIGN 3.21, 3.22 and 3.25 (development / evidence tool; summaries kept under profiles/anomaly_maps.md,
profiles/anomaly_z_maps.md and profiles/pixel_calibration.md).

``Reconstruct.get_scores`` on ``synthetic.write_checkpoint``'s `small` model over 32x32x1 blobs at the bench's batch, with
--anomaly_maps off and on and with --anomaly_z_maps 1 in ONE process (three trainers on one checkpoint), --runs timed passes of
each, alternating, after one short warm-up pass of each (2 t-starts: allocations, the engine's workspace).  The Z-map trainer is
timed twice per run: a validation pass (the statistics are accumulated) and an in-set pass (the Z-maps are formed, smoothed with
--z_sigma, and copied to the host).  With --calibrate a fourth trainer runs the validation pass with --pixel_calibrate_fpr
0.05,0.01,0.001 (the counted rows kept on the device, then the leave-one-out Z-maps and their histograms) beside the plain
validation pass.  With --kernels the map kernels are also timed by themselves at that batch (the library's
ProfScope: hipEvent-bracketed launches).  Prints one JSON line.

    python tools/anomaly_map_bench.py [--batch 1024] [--skip 4] [--runs 1] [--z_sigma 1.5] [--kernels] [--calibrate]
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

SCHED = dict(beta_schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)


def make_args(root, n_images, batch, skip, maps, z_maps=0, z_sigma=0.0, calibrate=None):
    ids = f"synthetic:blobs:n={n_images}:size=32:channels=1:seed=0"
    return argparse.Namespace(
        seed=2, output_dir=str(root), model_name="anomaly_map_bench", validation_ids=ids, in_ids=ids, out_ids=ids,
        spatial_dimension=2, image_size=None, image_roi=None, latent_pad=None, vqvae_checkpoint=None,
        ddpm_checkpoint_epoch=None, prediction_type="epsilon", model_type="small", b_scale=1.0, snr_shift=1, simplex_noise=0,
        batch_size=batch, augmentation=0, cache_data=1, num_workers=0, first_n_val=None, first_n=None, eval_checkpoint=None,
        drop_last=False, is_grayscale=1, run_val=1, run_in=0, run_out=0, num_inference_steps=100, inference_skip_factor=skip,
        anomaly_maps=int(maps), anomaly_z_maps=int(z_maps), anomaly_z_sigma=float(z_sigma), anomaly_z_std_floor=0.01,
        pixel_calibrate_fpr=calibrate, **SCHED)


def kernel_times(lib, ops, batch, dev):
    """us per launch and achieved GB/s (algorithmic bytes) of the three map kernels at `batch` pairs of 32x32x1."""
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(batch, 1, 32, 32, generator=g).to(dev), torch.rand(batch, 1, 32, 32, generator=g).to(dev)
    sizes, chns = [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)], (64, 192, 384, 256, 256)
    feats = [(torch.rand(batch, c, h, w, generator=g).to(dev), torch.rand(batch, c, h, w, generator=g).to(dev),
              (torch.rand(c, generator=g) / c).to(dev)) for c, (h, w) in zip(chns, sizes)]
    se, lp = torch.zeros(batch, 32, 32, device=dev), torch.zeros(batch, 32, 32, device=dev)
    packed = torch.empty(batch, sum(h * w for h, w in sizes), device=dev)

    def once():
        ops.sqerr_map(a, b, 0.04, out=se)
        off = 0
        for (f0, f1, lin), (h, w) in zip(feats, sizes):
            ops.lpips_layer_map(f0, f1, lin, packed, off)
            off += h * w
        ops.lpips_map_upsample(packed, sizes, (32, 32), weight=0.04, out=lp)

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
    return {k: {"launches": v["launches"], "us_per_launch": round(v["ms"] / v["launches"] * 1e3, 2),
                "GBps": round(v["bytes"] / v["ms"] / 1e6, 1)}
            for k, v in prof.items() if k in ("sqerr_map", "lpips_layer_map", "lpips_map_upsample")}


def z_kernel_times(lib, ops, batch, n_t, sigma, dev):
    """The same for the four Z-map kernels: the statistics update, the Z-score and the leave-one-out Z-score over `batch` rows of
    n_t x 2 x 32 x 32, the smoothing of the batch's 2 x `batch` maps."""
    g = torch.Generator().manual_seed(1)
    per_t = torch.rand(batch, n_t, 2, 32, 32, generator=g).to(dev)
    mean, m2 = torch.empty(n_t, 2, 32, 32, device=dev), torch.empty(n_t, 2, 32, 32, device=dev)
    ops.map_stats_update(per_t, 0, mean, m2)
    inv = 1.0 / torch.sqrt(m2 / (batch - 1))
    taps = torch.from_numpy(ops.gaussian_taps(sigma).astype("float32")).to(dev)
    z, zb = torch.empty(batch, 2, 32, 32, device=dev), torch.empty(2 * batch, 32, 32, device=dev)
    floor = (0.01 * torch.sqrt(m2 / (batch - 1)).amax(dim=(2, 3))).contiguous()
    zl = torch.empty_like(z)

    def once():
        ops.map_stats_update(per_t, batch, mean, m2)
        ops.map_zscore(per_t, mean, inv, out=z)
        ops.map_zscore_loo(per_t, mean, m2, 2 * batch, floor, out=zl)
        ops.map_blur(z.view(2 * batch, 32, 32), taps=taps, out=zb)

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
    return {k: {"launches": v["launches"], "us_per_launch": round(v["ms"] / v["launches"] * 1e3, 2),
                "GBps": round(v["bytes"] / v["ms"] / 1e6, 1)}
            for k, v in prof.items() if k in ("map_stats_update", "map_zscore", "map_zscore_loo", "map_blur")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip", type=int, default=4, help="inference_skip_factor (4: the bench's 25 t-starts)")
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--z_sigma", type=float, default=1.5, help="--anomaly_z_sigma of the Z-map leg (0: no smoothing launch)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--calibrate", action="store_true", help="also time the validation pass with --pixel_calibrate_fpr 0.05,0.01,0.001")
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops, synthetic
    from ddpm_ood_amd.data import get_data_loader
    from ddpm_ood_amd.trainer import Reconstruct

    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "inference_skip_factor": a.skip, "runs": []}
    stdout = sys.stdout
    with tempfile.TemporaryDirectory() as root:
        synthetic.write_checkpoint(Path(root) / "anomaly_map_bench", "small", 1, seed=1)
        sys.stdout = open(os.devnull, "w")  # the trainer prints like the reference; keep stdout to ONE JSON line
        try:
            trainers = {}
            for maps in (0, 1, "z"):
                args = make_args(root, a.batch, a.batch, a.skip, maps == 1, maps == "z", a.z_sigma)
                rec = trainers[maps] = Reconstruct(args)
                rec.quiet = True
            if a.calibrate:
                trainers["cal"] = Reconstruct(make_args(root, a.batch, a.batch, a.skip, False, True, a.z_sigma, "0.05,0.01,0.001"))
                trainers["cal"].quiet = True
            loader = get_data_loader(args.validation_ids, batch_size=a.batch, is_grayscale=True)
            loader.images = loader.images.to(trainers[0].device)  # inputs resident in HBM before timing starts
            for maps in (0, 1, "z"):
                trainers[maps].get_scores(loader, "val", 64)  # warm-up
            trainers["z"].get_scores(loader, "in", 64)
            if a.calibrate:
                trainers["cal"].get_scores(loader, "val", 64)
            for run in range(a.runs):
                for maps in (0, 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = trainers[maps].get_scores(loader, "val", a.skip)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    got = trainers[maps].last_maps
                    assert (got is not None) == bool(maps) and (not maps or got["lpips_map"].shape == (a.batch, 32, 32))
                    out["runs"].append({"anomaly_maps": maps, "run": run, "reconstructions": len(rows), "seconds": round(dt, 4),
                                        "reconstructions_per_s": round(len(rows) / dt, 2)})
                if a.calibrate:  # the validation pass again, with the rows kept and the leave-one-out pass behind it
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = trainers["cal"].get_scores(loader, "val", a.skip)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    cal = trainers["cal"].last_calibration
                    assert cal is not None and int(cal["n"]) == a.batch
                    out["runs"].append({"pixel_calibrate_fpr": "0.05,0.01,0.001", "pass": "val_calibrate", "z_sigma": a.z_sigma, "run": run,
                                        "reconstructions": len(rows), "seconds": round(dt, 4),
                                        "thresholds": cal["thresholds"].tolist(), "kept_bytes": a.batch * len(cal["t"]) * 2 * 32 * 32 * 4})
                for name in ("val", "in"):  # --anomaly_z_maps 1: the statistics pass, then a pass normalised by them
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rows = trainers["z"].get_scores(loader, name, a.skip)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    got = trainers["z"].last_zmaps
                    assert (got is not None) == (name == "in") and (got is None or got["z_mse_map"].shape == (a.batch, 32, 32))
                    out["runs"].append({"anomaly_z_maps": 1, "pass": name, "z_sigma": a.z_sigma, "run": run,
                                        "reconstructions": len(rows), "seconds": round(dt, 4),
                                        "reconstructions_per_s": round(len(rows) / dt, 2)})
        finally:
            sys.stdout = stdout
    best = {m: max(r["reconstructions_per_s"] for r in out["runs"] if r.get("anomaly_maps") == m) for m in (0, 1)}
    for name in ("val", "in"):
        out[f"value_z_maps_{name}"] = max(r["reconstructions_per_s"] for r in out["runs"] if r.get("pass") == name)
        out[f"ratio_z_{name}_over_off"] = round(out[f"value_z_maps_{name}"] / best[0], 4)
    if a.calibrate:
        plain = min(r["seconds"] for r in out["runs"] if r.get("pass") == "val")
        with_cal = min(r["seconds"] for r in out["runs"] if r.get("pass") == "val_calibrate")
        out["calibrate_added_seconds"], out["calibrate_over_plain_val"] = round(with_cal - plain, 4), round(with_cal / plain, 4)
    out["value_maps_off"], out["value_maps_on"] = best[0], best[1]
    out["ratio_on_over_off"] = round(best[1] / best[0], 4)
    out["unit"] = "reconstructions/s"
    if a.kernels:
        out["kernels"] = kernel_times(_lib.load(), ops, a.batch, torch.device("cuda:0"))
        n_t = len(range(1, 100, a.skip))
        out["kernels"].update(z_kernel_times(_lib.load(), ops, a.batch, n_t, a.z_sigma, torch.device("cuda:0")))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
