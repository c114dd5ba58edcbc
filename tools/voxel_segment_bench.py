"""Measurements behind DESIGN 3.31 (development / evidence tool; summary kept under profiles/voxel_segmentation.md).

Kernels: ``ops.map_median3d`` on ONE volume of 64^3 and 128^3 (us and achieved GB/s at 8 bytes per voxel), beside ``ops.map_blur3d``
(sigma 1) and ``ops.sqerr_map`` on the same volume in the same call; ``ops.map_segment3d`` (3 thresholds, min_size 8, connectivity
26) beside ``ops.map_component_counts3d``, the op it extends, on the four inputs of tools/voxel_metrics_bench.py: empty, one
ball, the 3-D serpentine and random voxels of density 0.3.  Timed by the library's ProfScope (hipEvent-bracketed: an op's figure
covers all of its launches), warm.
Pass: the device work of one in-set batch of ``--batch`` cfg5 volumes (128^3) as ``voxel_passes`` issues it on the zero mask: the
voxel metrics with regions alone, and with the segmentation (median, 3 + 2 thresholds) and the calibrated counts on top,
hipEvent-timed around the whole batch.  Validation: the leave-one-out pass of ``--batch`` retained rows (map_zscore_loo, the 3-D blur,
two histogram launches), the whole of what --voxel_calibrate_fpr adds to a validation pass beside keeping the rows.
Prints one JSON line.

    python tools/voxel_segment_bench.py [--batch 4] [--launches 20]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from voxel_metrics_bench import BINS, HI, LO, THRESHOLDS, masks_of  # noqa: E402

OPS = ("map_median3d", "map_blur", "map_blur_depth", "sqerr_map", "map_segment3d", "map_component_counts3d")  # (map_blur3d: its two launches)
MIN_SIZE, CONN = 8, 26


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
    return {k: round(prof[k]["ms"] / prof[k]["launches"] * 1e3, 2) for k in OPS if k in prof}


def kernel_times(lib, ops, dev, launches):
    out = {}
    taps = torch.from_numpy(ops.gaussian_taps(1.0).astype(np.float32)).to(dev)
    for side in (64, 128):
        D = H = W = side
        g = torch.Generator().manual_seed(side)
        noise = torch.randn(1, D, H, W, generator=g)
        z0 = noise.to(dev)
        a, b = torch.rand(1, 1, D, H, W, generator=g).to(dev), torch.rand(1, 1, D, H, W, generator=g).to(dev)
        acc, med = torch.zeros((1, D, H, W), device=dev), torch.empty((1, D, H, W), device=dev)

        def flat():
            ops.map_median3d(z0, 3, out=med)
            ops.map_blur3d(z0, taps=taps)
            ops.sqerr_map(a, b, 0.04, out=acc)

        us = profiled(lib, flat, launches=launches)
        us["map_blur3d"] = round(us.pop("map_blur", 0.0) + us.pop("map_blur_depth", 0.0), 2)
        per = out[f"{side}^3"] = {k: {"us": v, "GB_per_s": round(8.0 * D * H * W / v * 1e-3, 1)} for k, v in us.items()}
        thr = torch.tensor(THRESHOLDS, device=dev)
        for name, mask in masks_of(D, H, W).items():
            m = torch.from_numpy(mask[None]).to(dev)
            z = (noise * 1.0 + 3.0 * torch.from_numpy(mask[None]).float()).to(dev)  # Z-like: N(0, 1) outside, shifted by 3 inside
            labels, regions = ops.map_label3d(m, CONN)

            def once():
                ops.map_segment3d(z, m, labels, regions, thr, MIN_SIZE, CONN)
                ops.map_component_counts3d(z, m, labels, regions, thr, CONN)

            row = profiled(lib, once, launches=launches)
            removed = ops.map_segment3d(z, m, labels, regions, thr, MIN_SIZE, CONN)[3]
            per[name] = {"map_segment3d_us": row["map_segment3d"], "map_component_counts3d_us": row["map_component_counts3d"],
                         "removed_components_at_2": int(removed[0, 0, 0]), "removed_voxels_at_2": int(removed[0, 0, 1])}
    return out


def timed(once, launches):
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
    return round(best, 3)


def in_set_pass(ops, dev, B, launches):
    """ms per in-set batch of B cfg5 volumes on the zero mask: metrics with regions; the same with calibrated counts and segmentation."""
    D = H = W = 128
    P = D * H * W
    z = torch.randn(B, 2, P, device=dev)
    m = torch.zeros((B, P), dtype=torch.uint8, device=dev)
    mv = m.reshape(B, D, H, W)
    thr = torch.tensor(THRESHOLDS, device=dev)
    cal = torch.tensor([[2.5, 3.5], [2.5, 3.5]], device=dev)
    hist = torch.zeros((2, 2, BINS + 1), dtype=torch.int64, device=dev)
    overlap = torch.zeros((2, BINS + 1), dtype=torch.float64, device=dev)
    weights = torch.tensor([1 << b for b in range(16)], dtype=torch.int32, device=dev)
    out = {}
    for new in (False, True):
        def once():
            labels, regions = ops.map_label3d(mv, CONN)
            for c in range(2):
                zc = z[:, c].contiguous()
                zv = zc.reshape(B, D, H, W)
                ops.map_mask_hist(zc, m, LO, HI, BINS, total=hist[c])
                ops.map_mask_counts(zc, m, thr)
                ops.map_region_overlap3d(zv, labels, regions, LO, HI, BINS, total=overlap[c])
                ops.map_component_counts3d(zv, mv, labels, regions, thr, CONN)
                if new:
                    ops.map_mask_counts(zc, m, cal[c].contiguous())
                    ops.map_component_counts3d(zv, mv, labels, regions, cal[c].contiguous(), CONN)
            if new:
                vols = ops.map_median3d(z.reshape(2 * B, D, H, W), 3).reshape(B, 2, D, H, W)
                segs = []
                for c in range(2):
                    zc = vols[:, c].contiguous()
                    segs.append(torch.cat([ops.map_segment3d(zc, mv, labels, regions, thr, MIN_SIZE, CONN)[0],
                                           ops.map_segment3d(zc, mv, labels, regions, cal[c].contiguous(), MIN_SIZE, CONN)[0]], dim=1))
                bits = torch.stack(segs, dim=1).reshape(B, -1, 16)
                (bits.to(torch.int32) * weights).sum(dim=2).to(torch.float32).cpu()

        out["with_calibration_and_segmentation" if new else "metrics_and_regions"] = timed(once, launches)
    return out


def validation_extra(ops, dev, B, launches):
    """ms of the leave-one-out pass over B retained rows of one t-start at 128^3: what the calibration adds behind the validation pass."""
    D = H = W = 128
    P = D * H * W
    rows = torch.rand(B, 1, 2, D, H, W, device=dev)
    mean, m2 = rows.mean(dim=0).contiguous(), (rows.var(dim=0, unbiased=False) * max(B, 3)).contiguous()
    floor = torch.full((1, 2), 1e-3, device=dev)
    taps = torch.from_numpy(ops.gaussian_taps(1.0).astype(np.float32)).to(dev)
    no_mask = torch.zeros((B, P), dtype=torch.uint8, device=dev)
    hist = torch.zeros((2, 2, BINS + 1), dtype=torch.int64, device=dev)

    def once():
        zz = ops.map_blur3d(ops.map_zscore_loo(rows, mean, m2, max(B, 3), floor).reshape(-1, D, H, W), taps=taps).reshape(B, 2, P)
        for c in range(2):
            ops.map_mask_hist(zz[:, c].contiguous(), no_mask, LO, HI, BINS, total=hist[c])

    return timed(once, launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    from ddpm_ood_amd import _lib, ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(lib, ops, dev, a.launches),
           "in_set_batch_ms": in_set_pass(ops, dev, a.batch, a.launches), "validation_leave_one_out_ms": validation_extra(ops, dev, a.batch, a.launches),
           "batch": a.batch}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
