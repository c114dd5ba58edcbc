"""Measurements behind DESIGN 3.27 (development / evidence tool; summary kept under profiles/segmentation.md).

Kernels: ``ops.map_median`` (3 x 3 and 5 x 5; us and achieved GB/s at 8 bytes per pixel) and ``ops.map_segment`` (3 thresholds,
min_size 4, connectivity 8) beside ``ops.map_component_counts`` on the same inputs (the same labelling without the size table and
the mask store), at the bench's map shapes [2 x 256, 32, 32] and [2 x 16, 64, 64] and at [1, 128, 128], timed by the library's
ProfScope (hipEvent-bracketed launches).  Maps: N(0, 2^2) + 3 inside four discs per image.  --worst adds the all-ones plane, the
checkerboard at connectivity 4 and the serpentine at [256, 128, 128].
Passes: ``Reconstruct.get_scores`` on ``synthetic.write_checkpoint``'s `small` model over 32 x 32 x 1 images at ``--batch``, one
validation pass for the statistics, then --runs alternating in-set passes of two trainers, --anomaly_z_maps 1 alone and with
--pixel_segment 1.  Prints one JSON line.

    python tools/segment_bench.py [--batch 1024] [--skip 4] [--runs 3] [--no_passes] [--worst]
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

import tools.region_metrics_bench as rb  # noqa: E402
from tools.anomaly_map_bench import make_args  # noqa: E402

THRESHOLDS, MIN_SIZE = [2.0, 3.0, 4.0], 4
SHAPES = ((512, 32, 32), (32, 64, 64), (1, 128, 128))
OPS = ("map_median", "map_segment", "map_component_counts")


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
    for N, H, W in SHAPES:
        m = torch.from_numpy(rb.disc_masks(N, H, 4, seed=H)).to(dev)
        g = torch.Generator().manual_seed(H)
        z = (torch.randn(N, H, W, generator=g) * 2).to(dev) + 3.0 * m
        thr = torch.tensor(THRESHOLDS, device=dev)
        labels, regions = ops.map_label(m, 8)
        buf = torch.empty_like(z)
        row = {}
        for size in (3, 5):
            us = profiled(lib, lambda: ops.map_median(z, size, out=buf))["map_median"]
            row[f"map_median{size}"] = {"us": us, "GB_per_s": round(8.0 * N * H * W / us * 1e-3, 1)}
        zf = ops.map_median(z, 3)

        def once():
            ops.map_segment(zf, m, labels, regions, thr, MIN_SIZE, 8)
            ops.map_component_counts(zf, m, labels, regions, thr, 8)

        us = profiled(lib, once)
        removed = ops.map_segment(zf, m, labels, regions, thr, MIN_SIZE, 8)[3]
        row.update(map_segment_us=us["map_segment"], map_component_counts_us=us["map_component_counts"],
                   removed_components_per_image_at_2=round(float(removed[:, 0, 0].float().mean()), 1))
        out[f"{N}x{H}x{W}"] = row
    return out


def worst_planes(lib, ops, dev):
    H = W = 128
    serp = np.zeros((H, W), dtype=np.uint8)
    serp[0::2] = 1
    for k, yy in enumerate(range(1, H, 2)):
        serp[yy, W - 1 if k % 2 == 0 else 0] = 1
    y, x = np.mgrid[:H, :W]
    cases = {"ones": (np.ones((H, W), dtype=np.uint8), 8), "checkerboard_conn4": (((y + x) % 2 == 0).astype(np.uint8), 4),
             "serpentine": (serp, 8)}
    out = {}
    for name, (plane, conn) in cases.items():
        z = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(plane, (256, H, W))).astype(np.float32) * 9.0).to(dev)
        m = torch.zeros((256, H, W), dtype=torch.uint8, device=dev)
        labels, regions = ops.map_label(m, conn)
        thr = torch.tensor(THRESHOLDS, device=dev)

        def once():
            ops.map_segment(z, m, labels, regions, thr, MIN_SIZE, conn)
            ops.map_component_counts(z, m, labels, regions, thr, conn)

        us = profiled(lib, once)
        out[name] = {"map_segment_us": us["map_segment"], "map_component_counts_us": us["map_component_counts"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip", type=int, default=4, help="inference_skip_factor (4: the bench's 25 t-starts)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no_passes", action="store_true")
    ap.add_argument("--worst", action="store_true")
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops, synthetic
    from ddpm_ood_amd.data import get_data_loader
    from ddpm_ood_amd.trainer import Reconstruct

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "inference_skip_factor": a.skip,
           "kernels": kernel_times(lib, ops, dev), "runs": []}
    if a.worst:
        out["worst_256x128x128"] = worst_planes(lib, ops, dev)
    if not a.no_passes:
        stdout = sys.stdout
        with tempfile.TemporaryDirectory() as root:
            synthetic.write_checkpoint(Path(root) / "anomaly_map_bench", "small", 1, seed=1)
            sys.stdout = open(os.devnull, "w")  # the trainer prints like the reference; keep stdout to ONE JSON line
            try:
                trainers = {}
                for sg in (0, 1):
                    args = make_args(root, a.batch, a.batch, a.skip, 0, 1, 0.0)
                    args.pixel_segment = sg
                    trainers[sg] = Reconstruct(args)
                    trainers[sg].quiet = True
                loaders = {"val": get_data_loader(args.validation_ids, batch_size=a.batch, is_grayscale=True),
                           "in": get_data_loader(args.in_ids, batch_size=a.batch, is_grayscale=True)}
                for ld in loaders.values():
                    ld.images = ld.images.to(dev)  # inputs resident in HBM before timing starts
                for sg in (0, 1):
                    trainers[sg].get_scores(loaders["val"], "val", a.skip)  # the statistics, and the warm-up of every shape
                    trainers[sg].get_scores(loaders["in"], "in", a.skip)
                for run in range(a.runs):
                    for sg in (0, 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rows = trainers[sg].get_scores(loaders["in"], "in", a.skip)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        assert (trainers[sg].last_segments is not None) == bool(sg) and trainers[sg].last_zmaps is not None
                        out["runs"].append({"pixel_segment": sg, "run": run, "reconstructions": len(rows), "seconds": round(dt, 4)})
            finally:
                sys.stdout = stdout
        for sg in (0, 1):
            secs = [r["seconds"] for r in out["runs"] if r["pixel_segment"] == sg]
            out["seconds_on" if sg else "seconds_off"] = {"min": min(secs), "max": max(secs), "mean": round(sum(secs) / len(secs), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
