"""Voxel-level metrics of the Z-maps of volumes against ground-truth masks (``reconstruct.py --voxel_metrics 1``, with
``--voxel_regions 1`` the masks' 3-D connected components): what ``--pixel_metrics 1`` / ``--pixel_regions 1`` do for
images, on top of ``--spatial_dimension 3 --anomaly_volume_z_maps 1``.  The files are the 2-D ones (``pixels_<name>.npz``,
``regions_<name>.npz``: the same keys, ``connectivity`` in {26, 18, 6}), so ``ood_detection.py --score pixel`` reads them as they are.

``VoxelSettings`` is the flags, checked from the Namespace alone; ``MapPipeline`` takes it by keyword.  ``count_batch`` is one
batch's device work -- the histogram and counts kernels are flat over the voxels, the three region ops are those of
csrc/regions3d.hip -- and ``collect`` the pass's collectives and files.  With the flags off nothing here is called.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from . import ops, pixel_metrics, zmaps

FLAG = "--voxel_metrics 1"
REGION_FLAG = "--voxel_regions 1"
CONNECTIVITIES = (26, 18, 6)  # scipy.ndimage.generate_binary_structure(3, 3 | 2 | 1)
DEFAULT_CONNECTIVITY, DEFAULT_PRO_FPR = 26, 0.3
PIXEL_FLAGS = ("pixel_metrics", "pixel_regions", "pixel_calibrate_fpr", "pixel_segment")
MAX_VOXELS = 2 ** 31 - 1


@dataclass(frozen=True)
class VoxelSettings:
    metrics: bool = False  # pixels_<name>.npz of volumes: the in / out sets' Z-maps against --out_masks, voxel by voxel
    lo: float = None
    hi: float = None
    bins: int = None
    thresholds: list = None
    masks: list = None
    regions: bool = False  # regions_<name>.npz of volumes: 3-D components, overlap table, component counts
    connectivity: int = None
    pro_fpr: float = None

    @classmethod
    def from_args(cls, args):
        """Every refusal the voxel flags can earn, as ValueError naming the flag, from the Namespace alone."""
        metrics, regions = bool(getattr(args, "voxel_metrics", 0)), bool(getattr(args, "voxel_regions", 0))
        if not metrics and not regions:
            return cls()
        flag = FLAG if metrics else REGION_FLAG
        if regions and not metrics:
            raise ValueError(f"{REGION_FLAG} adds to the voxel metrics: it needs {FLAG}")
        for name in PIXEL_FLAGS:
            if getattr(args, name, None):
                raise ValueError(f"{flag}: not together with --{name} (the --pixel_* flags evaluate 2-D maps, the --voxel_* flags volumes; "
                                 f"calibration and segmentation of volumes are not built)")
        if int(args.spatial_dimension) != 3:
            raise ValueError(f"{flag}: voxel metrics evaluate volumes, they need --spatial_dimension 3 (2-D images: --pixel_metrics 1)")
        if not bool(getattr(args, "anomaly_volume_z_maps", 0)):
            raise ValueError(f"{flag} evaluates the Z-maps of volumes: it needs {zmaps.VOLUME_FLAG} (the raw maps have no fixed scale)")
        voxels = namespace_voxels(args)
        if voxels is not None and voxels > MAX_VOXELS:
            raise ValueError(f"{flag}: volumes of {voxels} voxels (--image_size / --image_roi) do not fit the 32-bit voxel indices and "
                             f"counts: D H W must stay below 2^31")
        try:
            lo, hi, bins, thresholds, masks = pixel_metrics.check_flags(
                True, args.out_ids if bool(getattr(args, "run_out", 1)) else None, getattr(args, "out_masks", None),
                getattr(args, "pixel_bins", pixel_metrics.DEFAULT_BINS), getattr(args, "pixel_range", None) or pixel_metrics.DEFAULT_RANGE,
                getattr(args, "pixel_thresholds", None) or pixel_metrics.DEFAULT_THRESHOLDS)
        except ValueError as e:  # (the shared flags keep their names; the message leads with this flag)
            raise ValueError(str(e).replace(pixel_metrics.FLAG, FLAG)) from None
        s = dict(metrics=True, lo=lo, hi=hi, bins=bins, thresholds=thresholds, masks=masks)
        if regions:
            connectivity = getattr(args, "voxel_connectivity", DEFAULT_CONNECTIVITY)
            pro_fpr = getattr(args, "voxel_pro_fpr", DEFAULT_PRO_FPR)
            try:
                conn, fpr = int(connectivity), float(pro_fpr)
            except (TypeError, ValueError):
                raise ValueError(f"{REGION_FLAG}: --voxel_connectivity is 26, 18 or 6 and --voxel_pro_fpr a number, got {connectivity!r} "
                                 f"and {pro_fpr!r}") from None
            if conn != float(connectivity) or conn not in CONNECTIVITIES:
                raise ValueError(f"{REGION_FLAG}: --voxel_connectivity must be 26, 18 or 6, got {connectivity}")
            if not 0.0 < fpr <= 1.0:
                raise ValueError(f"{REGION_FLAG}: --voxel_pro_fpr must lie in (0, 1], got {pro_fpr}")
            s.update(regions=True, connectivity=conn, pro_fpr=fpr)
        return cls(**s)


def namespace_voxels(args):
    """D H W of the volumes a Namespace asks for, where it says: --image_size cubed, else the product of a --image_roi without a
    kept (-1) axis; None when the extent comes from the files."""
    size, roi = getattr(args, "image_size", None), getattr(args, "image_roi", None)
    if size:
        return int(size) ** 3
    if roi and all(int(r) > 0 for r in roi):
        return int(np.prod([int(r) for r in roi], dtype=object))
    return None


# ---- the bytes a batch's voxel steps take on the device ---------------------------------------------------------------------
# The formulas of the library's size functions (csrc/regions3d.hip), restated so that a batch is refused before anything is
# allocated; tests/test_voxel_metrics_host.py holds them against the library.

def label_scratch_bytes(B: int, P: int) -> int:
    return 4 * (B * P + B * -(-P // 256) + B)


def overlap_scratch_bytes(B: int, bins: int, chunk: int) -> int:
    return 8 * B * (bins + 1) + 4 * chunk * (bins + 2)


def counts_scratch_bytes(B: int, K: int, P: int) -> int:
    items = B * K
    return 4 * (items * P + items * 2 * (P // 32 + 1) + items * -(-P // 256) * 3 + items)


def batch_bytes(B: int, extent, s: VoxelSettings) -> int:
    """What ``count_batch`` allocates for a batch of B volumes: the mask, one channel's Z-map, the histogram slabs and counts; with
    regions the labels, the three scratch buffers (the forests of the mask and of the K thresholded maps, the overlap tables) and
    the component counts.  The two channels run one after the other through the same sizes."""
    P, K = int(np.prod([int(e) for e in extent], dtype=object)), len(s.thresholds)
    need = B * P + 4 * B * P + ops.map_hist_parts(B * P) * 2 * (s.bins + 1) * 4 + 2 * 12 * B * K
    if s.regions:
        need += 4 * B * P + 4 * B + label_scratch_bytes(B, P) + overlap_scratch_bytes(B, s.bins, ops.map_region_overlap3d_chunk(s.bins)) \
            + counts_scratch_bytes(B, K, P) + 2 * 12 * B * K
    return int(need)


def check_budget(B: int, n_t: int, extent, s: VoxelSettings, budget_bytes: int) -> int:
    """The bytes of a batch's per-t maps plus those of its voxel steps, or ValueError when they exceed
    --anomaly_volume_budget_gb (before the voxel steps allocate anything)."""
    P = int(np.prod([int(e) for e in extent], dtype=object))
    if P > MAX_VOXELS:
        raise ValueError(f"{FLAG}: volumes of {P} voxels do not fit the 32-bit voxel indices and counts: D H W must stay below 2^31")
    maps, mine = int(B) * int(n_t) * 2 * P * 4, batch_bytes(B, extent, s)
    if maps + mine > int(budget_bytes):
        shape = " x ".join(str(int(e)) for e in extent)
        raise ValueError(f"{REGION_FLAG if s.regions else FLAG}: a batch of {B} volumes of {shape} takes {maps / (1 << 30):.3f} GiB of per-t "
                         f"maps and {mine / (1 << 30):.3f} GiB of masks, labels, forests and tables, over the budget of "
                         f"{budget_bytes / (1 << 30):.3f} GiB: lower --batch_size or raise --anomaly_volume_budget_gb")
    return maps + mine


# ---- one batch, one pass -------------------------------------------------------------------------------------------------------

def count_batch(mp, z, mask, extent, n_t: int):
    """``z`` [B, 2, D H W] on the device, the final Z-maps of a batch, against ``mask`` (uint8 [B, 1, D, H, W]; None: all zero).  Per
    channel one histogram launch into the pass's [2, 2, nbins + 1] table and one counts launch; with regions the mask labelled
    once, then per channel one overlap call into the pass's float64 [2, nbins + 1] table and one component-counts call.  Mask,
    labels and regions are arguments between the steps.  Returns (the device's columns of the row by name, the masks' voxel counts
    [B] on the host)."""
    p, s = mp.p, mp.p.voxel
    B, _, P = z.shape
    check_budget(B, n_t, extent, s, p.s.volume_budget)
    m, mask_voxels = mp.device_mask(mask, B, P, FLAG)
    if mp.hist is None:
        mp.hist = torch.zeros((2, 2, s.bins + 1), dtype=torch.int64, device=p.device)
    if s.regions and mp.overlap is None:
        mp.overlap = torch.zeros((2, s.bins + 1), dtype=torch.float64, device=p.device)
    labels = regions = None
    if s.regions:
        labels, regions = ops.map_label3d(m.reshape((B,) + tuple(extent)), s.connectivity)
    counts, components = [], []
    for c in range(2):
        zc = z[:, c].contiguous()
        ops.map_mask_hist(zc, m, s.lo, s.hi, s.bins, total=mp.hist[c])
        counts.append(ops.map_mask_counts(zc, m, p.thresholds))
        if s.regions:
            zv = zc.reshape((B,) + tuple(extent))
            ops.map_region_overlap3d(zv, labels, regions, s.lo, s.hi, s.bins, total=mp.overlap[c])
            components.append(ops.map_component_counts3d(zv, m.reshape(zv.shape), labels, regions, p.thresholds, s.connectivity))
    parts = {"counts": torch.stack(counts, dim=1)}
    if s.regions:
        parts["components"], parts["regions"] = torch.stack(components, dim=1), regions
    return parts, mask_voxels


def collect(mp, files, t, results, *ids):
    """The histogram (and the overlap table) summed over the ranks, ONE all_reduce each, and every rank's integer rows in the CSV's
    order (the gather's payload is fp32, so a count must stay below 2^24 with more than one rank): ``files`` gains PIXELS and,
    with regions, REGIONS -- the keys of the 2-D files."""
    from .map_passes import PIXELS, REGIONS, host_if_gloo

    p, s = mp.p, mp.p.voxel
    hist, overlap = mp.hist, mp.overlap
    if p.ddp:
        voxels = int(np.prod(mp.zmaps[0].shape[2:], dtype=np.int64))
        if voxels >= 1 << 24:
            raise ValueError(f"{FLAG}: a count of up to {voxels} voxels is not exact in the fp32 payload of the gather (D H W must "
                             f"stay below 2^24 with more than one rank)")
        hist = host_if_gloo(hist)
        dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        if s.regions:
            overlap = host_if_gloo(overlap)
            dist.all_reduce(overlap, op=dist.ReduceOp.SUM)
    got = mp._gather(FLAG, mp.rows, results, *ids)
    if got is None:
        return files
    stems, row = np.asarray(got[0]), p.layout.unpack(np.rint(got[1]).astype(np.int64))
    head = {"filename": stems, "t": t, "channels": np.asarray(zmaps.CHANNELS), "lo": np.float64(s.lo), "hi": np.float64(s.hi),
            "nbins": np.int64(s.bins)}
    thresholds = np.asarray(s.thresholds, dtype=np.float32)
    if s.regions:
        files[REGIONS] = {**head, "connectivity": np.int64(s.connectivity), "regions": row["regions"].astype(np.int32),
                          "overlap": overlap.cpu().numpy().astype(np.float64), "thresholds": thresholds,
                          "components": row["components"].astype(np.int32), "sigma": np.float64(p.s.z_sigma)}
    files[PIXELS] = {**head, "hist": hist.cpu().numpy().astype(np.int64), "thresholds": thresholds,
                     "counts": row["counts"].astype(np.int32), "mask_pixels": row["mask_pixels"], "sigma": np.float64(p.s.z_sigma)}
    return files
