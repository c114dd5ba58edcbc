"""Measurements behind DESIGN 3.30 (development / evidence tool; summary kept under profiles/voxel_metrics.md).

Kernels: ``ops.map_label3d`` (both predicates), ``ops.map_region_overlap3d`` (4 096 bins over [-16, 48)) and
``ops.map_component_counts3d`` (3 thresholds) on ONE volume at the cfg5 extent 128^3 and at 160 x 160 x 128, connectivity 26 (and 6
for the labelling), on four masks: empty, one ball, the 3-D serpentine (one voxel wide: the worst chain) and random voxels of
density 0.3.  Timed by the library's ProfScope (hipEvent-bracketed: an op's figure covers all of its launches); bytes are the
launcher's own count.  ``sqerr_map`` on the same volume is the yardstick of DESIGN 3.29.
Pass: the device work of one in-set batch of ``--batch`` volumes as ``voxel_passes.count_batch`` issues it (zero mask; per channel
histogram, counts, overlap, component counts; one labelling), hipEvent-timed around the whole batch, with and without regions.
Prints one JSON line.

    python tools/voxel_metrics_bench.py [--batch 4] [--launches 20]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

LO, HI, BINS, THRESHOLDS = -16.0, 48.0, 4096, [2.0, 3.0, 4.0]
OPS = ("map_label3d_u8", "map_label3d_f32", "map_region_overlap3d", "map_component_counts3d", "map_mask_hist", "map_mask_counts", "sqerr_map")
EXTENTS = ((128, 128, 128), (160, 160, 128))


def serpentine3d(D, H, W):
    """One voxel wide: every other row of every other plane full, rows joined alternately at their ends, planes at the path's ends."""
    plane = np.zeros((H, W), dtype=np.uint8)
    plane[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        plane[y, W - 1 if k % 2 == 0 else 0] = 1
    rows = len(range(0, H, 2))
    end = (2 * (rows - 1), W - 1 if (rows - 1) % 2 == 0 else 0)
    m = np.zeros((D, H, W), dtype=np.uint8)
    for j, z in enumerate(range(0, D, 2)):
        m[z] = plane
        if z + 2 < D:
            y, x = end if j % 2 == 0 else (0, 0)
            m[z + 1, y, x] = 1
    return m


def masks_of(D, H, W):
    z, y, x = np.mgrid[:D, :H, :W]
    ball = (((z - D / 2) ** 2 + (y - H / 2) ** 2 + (x - W / 2) ** 2) <= (0.125 * D) ** 2).astype(np.uint8)  # 25 % of the extent across
    return {"empty": np.zeros((D, H, W), dtype=np.uint8), "ball": ball, "serpentine": serpentine3d(D, H, W),
            "random0.3": (np.random.default_rng(0).random((D, H, W)) < 0.3).astype(np.uint8)}


def profiled(lib, once, warmup=3, launches=20):
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
    return {k: {"us": round(prof[k]["ms"] / prof[k]["launches"] * 1e3, 2), "MB": round(prof[k]["bytes"] / prof[k]["launches"] / 1e6, 2)}
            for k in OPS if k in prof}


def kernel_times(lib, ops, dev, launches):
    out = {}
    for D, H, W in EXTENTS:
        g = torch.Generator().manual_seed(D + W)
        noise = torch.randn(1, D, H, W, generator=g)
        a, b = torch.rand(1, 1, D, H, W, generator=g).to(dev), torch.rand(1, 1, D, H, W, generator=g).to(dev)
        acc = torch.zeros((1, D, H, W), device=dev)
        out[f"{D}x{H}x{W}"] = per = {"sqerr_map": profiled(lib, lambda: ops.sqerr_map(a, b, 0.04, out=acc), launches=launches)["sqerr_map"]}
        thr = torch.tensor(THRESHOLDS, device=dev)
        for name, mask in masks_of(D, H, W).items():
            m = torch.from_numpy(mask[None]).to(dev)
            z = (noise * 1.0 + 3.0 * torch.from_numpy(mask[None]).float()).to(dev)  # Z-like: N(0, 1) outside, shifted by 3 inside
            total = torch.zeros(BINS + 1, dtype=torch.float64, device=dev)
            hist = torch.zeros((2, BINS + 1), dtype=torch.int64, device=dev)
            labels, regions = ops.map_label3d(m, 26)

            def once():
                ops.map_label3d(m, 26)
                ops.map_label3d(z, 26, threshold=2.0)
                ops.map_region_overlap3d(z, labels, regions, LO, HI, BINS, total=total)
                ops.map_component_counts3d(z, m, labels, regions, thr, 26)
                ops.map_mask_hist(z, m, LO, HI, BINS, total=hist)
                ops.map_mask_counts(z, m, thr)

            row = profiled(lib, once, launches=launches)
            row["label_u8_conn6"] = profiled(lib, lambda: ops.map_label3d(m, 6), launches=launches)["map_label3d_u8"]
            row["regions"] = int(regions[0])
            row["mask_voxels"] = int(mask.sum())
            row["components_at_2"] = int(ops.map_label3d(z, 26, threshold=2.0)[1][0])
            per[name] = row
    return out


def in_set_pass(ops, dev, B, launches):
    """ms per in-set batch of B cfg5 volumes: what ``voxel_passes.count_batch`` launches on the zero mask, metrics alone and with regions."""
    D = H = W = 128
    P = D * H * W
    z = torch.randn(B, 2, P, device=dev)
    m = torch.zeros((B, P), dtype=torch.uint8, device=dev)
    thr = torch.tensor(THRESHOLDS, device=dev)
    hist = torch.zeros((2, 2, BINS + 1), dtype=torch.int64, device=dev)
    overlap = torch.zeros((2, BINS + 1), dtype=torch.float64, device=dev)
    out = {}
    for regions_on in (False, True):
        def once():
            if regions_on:
                labels, regions = ops.map_label3d(m.reshape(B, D, H, W), 26)
            for c in range(2):
                zc = z[:, c].contiguous()
                ops.map_mask_hist(zc, m, LO, HI, BINS, total=hist[c])
                ops.map_mask_counts(zc, m, thr)
                if regions_on:
                    zv = zc.reshape(B, D, H, W)
                    ops.map_region_overlap3d(zv, labels, regions, LO, HI, BINS, total=overlap[c])
                    ops.map_component_counts3d(zv, m.reshape(B, D, H, W), labels, regions, thr, 26)

        for _ in range(3):
            once()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            once()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1))
        out["regions" if regions_on else "metrics"] = round(best, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(lib, ops, dev, a.launches),
           "in_set_batch_ms": in_set_pass(ops, dev, a.batch, a.launches), "batch": a.batch}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
