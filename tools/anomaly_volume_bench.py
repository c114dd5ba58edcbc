"""Measurements behind DESIGN 3.29 (development / evidence tool; summary kept under profiles/anomaly_volume_maps.md).

--kernels: the kernels of the volume maps by themselves at the cfg5 extent (one 128^3 volume, 25 t-starts, sigma 1.5), timed by
the library's ProfScope (hipEvent-bracketed launches), with the bytes each must move over its time: ``sqerr_map`` (the yardstick:
it streams the volume), ``lpips_map_upsample_view`` per axis (accumulating, as the trainer calls it, and fresh), the in-plane and
the depth pass of ``map_blur3d``, ``map_stats_update`` and ``map_zscore`` over [1, 25, 2, 128^3].

Without --kernels: ``Reconstruct.get_scores`` over one batch (a "step": every t-start of every volume of the batch) with the
volume flags off and on in ONE process, alternating, --runs timed passes each after a warm-up pass of each: the toy latent model
of tests/test_gpu_volume_maps_cli.py (32^3 volumes, README VQ-VAE shape, latents padded to 4^3) and, with --cfg5, bench.py's cfg5
(128^3 volumes).  The flags-off leg is the code path of a run without the flags.  With the flags on a validation pass (statistics)
and an in-set pass (Z-maps, smoothed, copied to the host) are timed.  Prints one JSON line.

    python tools/anomaly_volume_bench.py --kernels [--size 128] [--n_t 25] [--sigma 1.5]
    python tools/anomaly_volume_bench.py [--cfg5] [--batch 4] [--skip 4] [--runs 3] [--sigma 1.5] [--views last|all]
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
VQ_README = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(256, 256, 256, 256), num_res_layers=3,
                 num_res_channels=(256, 256, 256, 256), downsample_parameters=((2, 4, 1, 1),) * 4,
                 upsample_parameters=((2, 4, 1, 1, 0),) * 4, num_embeddings=2048, embedding_dim=128)


def _profiled(lib, once, reps=20, warm=3):
    """{kernel: (us per launch, GB/s of the launcher's own byte count)} of `reps` calls of once() after `warm` unrecorded ones."""
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    lib.ddpm_prof_enable(1)
    for _ in range(reps):
        once()
    lib.ddpm_prof_enable(0)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.ddpm_prof_report(buf, len(buf))
    return {k: {"launches": v["launches"], "us_per_launch": round(v["ms"] / v["launches"] * 1e3, 2),
                "MB_per_launch": round(v["bytes"] / v["launches"] / 1e6, 2), "GBps": round(v["bytes"] / v["ms"] / 1e6, 1)}
            for k, v in json.loads(buf.value.decode()).items()}


def kernel_times(lib, ops, size, n_t, sigma, dev):
    from ddpm_ood_amd.perceptual import LPIPS

    g = torch.Generator().manual_seed(0)
    vol = (size, size, size)
    a, b = torch.rand((1, 1) + vol, generator=g).to(dev), torch.rand((1, 1) + vol, generator=g).to(dev)
    acc = torch.zeros((1,) + vol, device=dev)
    out = {"sqerr_map": _profiled(lib, lambda: ops.sqerr_map(a, b, 1.0 / n_t, out=acc))["sqerr_map"]}
    sizes = LPIPS.pyramid_sizes(size, size)
    rows = torch.rand(size, sum(h * w for h, w in sizes), generator=g).to(dev)
    for axis in (2, 3, 4):
        out[f"lpips_map_upsample_view axis {axis} accumulate"] = _profiled(
            lib, lambda: ops.lpips_map_upsample_view(rows, sizes, vol, axis, 1.0 / n_t, out=acc))["lpips_map_upsample_view"]
        out[f"lpips_map_upsample_view axis {axis} fresh"] = _profiled(
            lib, lambda: ops.lpips_map_upsample_view(rows, sizes, vol, axis))["lpips_map_upsample_view"]
    z, zb = torch.rand((2,) + vol, generator=g).to(dev), torch.empty((2,) + vol, device=dev)
    taps = torch.from_numpy(ops.gaussian_taps(sigma).astype("float32")).to(dev)
    blur = _profiled(lib, lambda: ops.map_blur3d(z, taps=taps, out=zb))
    out["map_blur3d in-plane passes (H, W)"], out["map_blur3d depth pass"] = blur["map_blur"], blur["map_blur_depth"]
    per_t = torch.rand((1, n_t, 2) + vol, generator=g).to(dev)
    mean, m2 = torch.empty((n_t, 2) + vol, device=dev), torch.empty((n_t, 2) + vol, device=dev)
    ops.map_stats_update(per_t, 0, mean, m2)
    out["map_stats_update"] = _profiled(lib, lambda: ops.map_stats_update(per_t, 4, mean, m2), reps=10)["map_stats_update"]
    inv = torch.rand((n_t, 2) + vol, generator=g).to(dev)
    zo = torch.empty((1, 2) + vol, device=dev)
    out["map_zscore"] = _profiled(lib, lambda: ops.map_zscore(per_t, mean, inv, out=zo), reps=10)["map_zscore"]
    return out


def make_args(root, model, size, n, batch, skip, on, sigma, views, latent_pad):
    ids = f"synthetic:blobs3d:n={n}:size={size}:channels=1:seed=0"
    return argparse.Namespace(
        seed=2, output_dir=str(root), model_name=model, validation_ids=ids, in_ids=ids, out_ids=ids, spatial_dimension=3,
        image_size=None, image_roi=None, latent_pad=latent_pad, vqvae_checkpoint=str(Path(root) / "vqvae" / "checkpoint.pth"),
        ddpm_checkpoint_epoch=None, prediction_type="epsilon", model_type="small", b_scale=1.0, snr_shift=1, simplex_noise=0,
        batch_size=batch, augmentation=0, cache_data=1, num_workers=0, first_n_val=None, first_n=None, eval_checkpoint=None,
        drop_last=False, is_grayscale=1, run_val=1, run_in=0, run_out=0, num_inference_steps=100, inference_skip_factor=skip,
        anomaly_volume_maps=int(on), anomaly_volume_z_maps=int(on), anomaly_z_sigma=float(sigma) if on else 0.0,
        anomaly_volume_views=views, **SCHED)


def step_times(root, name, size, latent_pad, a):
    """One entry of the report: the timed passes of a configuration, flags off and on alternating."""
    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.data import get_data_loader
    from ddpm_ood_amd.trainer import Reconstruct

    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    (Path(root) / name).mkdir()
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               Path(root) / name / "checkpoint.pth")
    trainers = {}
    for on in (0, 1):
        args = make_args(root, name, size, a.batch, a.batch, a.skip, on, a.sigma, a.views, latent_pad)
        trainers[on] = Reconstruct(args)
        trainers[on].quiet = True
    loader = get_data_loader(args.validation_ids, batch_size=a.batch, is_grayscale=True, spatial_dimension=3)
    loader.images = loader.images.to(trainers[0].device)  # inputs resident in HBM before timing starts
    legs = [(0, "val"), (1, "val"), (1, "in")]
    for on, which in legs:  # warm-up: every shape of the timed window (allocations, the engine's workspace, code objects)
        trainers[on].get_scores(loader, which, a.skip)
    runs = []
    for run in range(a.runs):
        for on, which in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = trainers[on].get_scores(loader, which, a.skip)
            torch.cuda.synchronize()
            runs.append({"flags": on, "pass": which, "run": run, "reconstructions": len(rows), "seconds": round(time.perf_counter() - t0, 4)})
    best = {leg: min(r["seconds"] for r in runs if (r["flags"], r["pass"]) == leg) for leg in legs}
    spread = {f"{on}-{which}": round(max(r["seconds"] for r in runs if (r["flags"], r["pass"]) == (on, which)) / best[on, which] - 1, 4)
              for on, which in legs}
    return {"volume": size, "batch": a.batch, "t_starts": len(range(1, 100, a.skip)), "views": a.views, "sigma": a.sigma, "runs": runs,
            "seconds_off": best[0, "val"], "seconds_on_val": best[1, "val"], "seconds_on_in": best[1, "in"], "spread": spread,
            "overhead_val": round(best[1, "val"] / best[0, "val"] - 1, 4), "overhead_in": round(best[1, "in"] / best[0, "val"] - 1, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--size", type=int, default=128, help="--kernels: the volume's side")
    ap.add_argument("--n_t", type=int, default=25, help="--kernels: t-starts of the statistics and the Z-score")
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--cfg5", action="store_true", help="also time the README cfg5 configuration (128^3 volumes)")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--skip", type=int, default=4, help="inference_skip_factor (4: 25 t-starts)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--views", default="last", choices=["last", "all"])
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops
    from ddpm_ood_amd.vqvae import VQVAE

    out = {"device": torch.cuda.get_device_name(0)}
    if a.kernels:
        out["kernels"] = kernel_times(_lib.load(), ops, a.size, a.n_t, a.sigma, torch.device("cuda:0"))
        print(json.dumps(out), flush=True)
        return
    stdout = sys.stdout
    with tempfile.TemporaryDirectory() as root:
        torch.manual_seed(3)
        vq = VQVAE(**VQ_README).eval()  # random init, the codebook spread so that codes are used (as bench.py's cfg5)
        with torch.no_grad():
            vq.quantizer.quantizer.embedding.weight.mul_(3.0)
        (Path(root) / "vqvae").mkdir()
        torch.save({"model_state_dict": vq.state_dict()}, Path(root) / "vqvae" / "checkpoint.pth")
        json.dump(VQ_README, open(Path(root) / "vqvae" / "vqvae_config.json", "w"))
        sys.stdout = open(os.devnull, "w")  # the trainer prints like the reference; keep stdout to ONE JSON line
        try:
            out["toy"] = step_times(root, "toy_ldm", 32, (1, 1, 1, 1, 1, 1), a)
            if a.cfg5:
                out["cfg5"] = step_times(root, "cfg5", 128, None, a)
        finally:
            sys.stdout = stdout
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
