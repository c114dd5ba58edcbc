"""Measurements behind DESIGN 3.24 (development / evidence tool; summary kept under profiles/region_metrics.md).

Kernels: ``ops.map_label`` (both predicates), ``ops.map_region_overlap`` (4 096 bins over [-16, 48)) and
``ops.map_component_counts`` (3 thresholds) by themselves at [256, 32, 32] and [256, 64, 64], on masks of 1, 4 and 16 discs per
image, connectivity 8, timed by the library's ProfScope (hipEvent-bracketed launches; the overlap's figure covers both of its
launches).  --worst adds the labelling of the longest chains (serpentine, comb, checkerboard at connectivity 4, random masks of
density 0.6) at [256, 128, 128].
Passes: ``Reconstruct.get_scores`` on ``synthetic.write_checkpoint``'s `small` model over 32 x 32 x 1 images at ``--batch``, one
validation pass for the statistics, then --runs alternating in-set passes (blobs, no masks) and out-set passes (lesion, masks
"auto") of two trainers, --pixel_metrics 1 alone and with --pixel_regions 1.  Prints one JSON line.

    python tools/region_metrics_bench.py [--batch 1024] [--skip 4] [--runs 2] [--no_passes] [--worst]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.anomaly_map_bench import make_args  # noqa: E402

LO, HI, BINS, THRESHOLDS = -16.0, 48.0, 4096, [2.0, 3.0, 4.0]
OPS = ("map_label_u8", "map_label_f32", "map_region_overlap", "map_component_counts")


def disc_masks(N, H, discs, seed):
    """uint8 [N, H, H]: `discs` discs per image, H / 10 pixels in radius, centres drawn uniformly (discs may merge)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :H]
    m = np.zeros((N, H, H), dtype=np.uint8)
    for n in range(N):
        for cy, cx in rng.uniform(0, H, (discs, 2)):
            m[n] |= ((y - cy) ** 2 + (x - cx) ** 2 <= (H / 10) ** 2).astype(np.uint8)
    return m


def profiled(lib, once, warmup=5, launches=50):
    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    lib.ddpm_prof_enable(1)
    for _ in range(launches):
        once()
    lib.ddpm_prof_enable(0)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.ddpm_prof_report(buf, len(buf))
    prof = json.loads(buf.value.decode())
    return {k: round(prof[k]["ms"] / prof[k]["launches"] * 1e3, 2) for k in OPS if k in prof}


def kernel_times(lib, ops, dev):
    out = {}
    for N, H in ((256, 32), (256, 64)):
        for discs in (1, 4, 16):
            m = torch.from_numpy(disc_masks(N, H, discs, seed=H + discs)).to(dev)
            g = torch.Generator().manual_seed(H + discs)
            z = (torch.randn(N, H, H, generator=g) * 2).to(dev) + 3.0 * m
            thr = torch.tensor(THRESHOLDS, device=dev)
            total = torch.zeros(BINS + 1, dtype=torch.float64, device=dev)
            labels, regions = ops.map_label(m, 8)

            def once():
                ops.map_label(m, 8)
                ops.map_label(z, 8, threshold=2.0)
                ops.map_region_overlap(z, labels, regions, LO, HI, BINS, total=total)
                ops.map_component_counts(z, m, labels, regions, thr, 8)

            us = profiled(lib, once)
            us["regions_per_image"] = round(float(regions.float().mean()), 2)
            us["components_per_image_at_2"] = round(float(ops.map_label(z, 8, threshold=2.0)[1].float().mean()), 1)
            out[f"{N}x{H}x{H}_discs{discs}"] = us
    return out


def worst_labelling(lib, ops, dev):
    """The labelling alone at [256, 128, 128] on the shapes with the longest merge chains (tests/region_ref.py's shapes, restated)."""
    H = W = 128
    serp = np.zeros((H, W), dtype=np.uint8)
    serp[0::2] = 1
    for k, yy in enumerate(range(1, H, 2)):
        serp[yy, W - 1 if k % 2 == 0 else 0] = 1
    y, x = np.mgrid[:H, :W]
    comb = np.zeros((H, W), dtype=np.uint8)  # teeth that join only in the last row
    comb[:, 0::2] = 1
    comb[H - 1] = 1
    cases = {"serpentine": (serp, 8), "comb": (comb, 8), "checkerboard_conn4": (((y + x) % 2 == 0).astype(np.uint8), 4),
             "ones": (np.ones((H, W), dtype=np.uint8), 8),
             "random0.6": ((np.random.default_rng(0).random((H, W)) < 0.6).astype(np.uint8), 8)}
    out = {}
    for name, (plane, conn) in cases.items():
        m = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(plane, (256, H, W)))).to(dev)
        us = profiled(lib, lambda: ops.map_label(m, conn))
        out[name] = {"us_per_call": us["map_label_u8"], "regions": int(ops.map_label(m, conn)[1][0])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip", type=int, default=4, help="inference_skip_factor (4: the bench's 25 t-starts)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--no_passes", action="store_true")
    ap.add_argument("--worst", action="store_true")
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops, synthetic
    from ddpm_ood_amd.data import get_data_loader
    from ddpm_ood_amd.trainer import Reconstruct

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "inference_skip_factor": a.skip,
           "kernels_us": kernel_times(lib, ops, dev), "runs": []}
    if a.worst:
        out["worst_labelling"] = worst_labelling(lib, ops, dev)
    if not a.no_passes:
        stdout = sys.stdout
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_checkpoint(Path(root) / "anomaly_map_bench", "small", 1, seed=1)
            sys.stdout = open(os.devnull, "w")  # the trainer prints like the reference; keep stdout to ONE JSON line
            try:
                lesion = f"synthetic:lesion:n={a.batch}:size=32:channels=1:seed=1:mix=25"
                trainers = {}
                for rg in (0, 1):
                    args = make_args(root, a.batch, a.batch, a.skip, 0, 1, 0.0)
                    args.pixel_metrics, args.pixel_regions, args.run_out, args.out_ids, args.out_masks = 1, rg, 1, lesion, "auto"
                    trainers[rg] = Reconstruct(args)
                    trainers[rg].quiet = True
                loaders = {"val": get_data_loader(args.validation_ids, batch_size=a.batch, is_grayscale=True),
                           "in": get_data_loader(args.in_ids, batch_size=a.batch, is_grayscale=True),
                           "out": get_data_loader(lesion, batch_size=a.batch, is_grayscale=True, mask_ids="auto")}
                for ld in loaders.values():
                    ld.images = ld.images.to(dev)  # inputs resident in HBM before timing starts
                for rg in (0, 1):
                    trainers[rg].get_scores(loaders["val"], "val", a.skip)  # the statistics, and the warm-up of every shape
                for run in range(a.runs):
                    for name in ("in", "out"):
                        for rg in (0, 1):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            rows = trainers[rg].get_scores(loaders[name], name, a.skip)
                            torch.cuda.synchronize()
                            dt = time.perf_counter() - t0
                            assert (trainers[rg].last_regions is not None) == bool(rg) and trainers[rg].last_pixels is not None
                            out["runs"].append({"pixel_regions": rg, "pass": name, "run": run, "reconstructions": len(rows),
                                                "seconds": round(dt, 4), "reconstructions_per_s": round(len(rows) / dt, 2)})
                # the per-batch cost of the region calls by themselves, on the out set's last batch shape
                m = loaders["out"].masks
                m = (torch.stack(list(m)) if isinstance(m, list) else m)[:a.batch].reshape(-1, 32, 32).contiguous().to(dev)
                z = torch.randn(m.shape[0], 2, 32 * 32, device=dev)
                region_pass = trainers[1].map_pipeline.begin("out", loaders["out"], [])
                us = profiled(lib, lambda: region_pass.region_step(z, m, 32, 32), launches=20)
                out["per_batch_us"] = {**us, "sum": round(us["map_label_u8"] + 2 * us["map_region_overlap"] + 2 * us["map_component_counts"], 2)}
            finally:
                sys.stdout = stdout
        for name in ("in", "out"):
            best = {rg: max(r["reconstructions_per_s"] for r in out["runs"] if r["pass"] == name and r["pixel_regions"] == rg)
                    for rg in (0, 1)}
            out[f"value_{name}_off"], out[f"value_{name}_on"] = best[0], best[1]
            out[f"ratio_{name}_on_over_off"] = round(best[1] / best[0], 4)
        out["unit"] = "reconstructions/s"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
