"""Voxel-level metrics of the Z-maps of volumes against ground-truth masks (``reconstruct.py --voxel_metrics 1``, with
``--voxel_regions 1`` the masks' 3-D connected components): what ``--pixel_metrics 1`` / ``--pixel_regions 1`` do for
images, on top of ``--spatial_dimension 3 --anomaly_volume_z_maps 1``.  The files are the 2-D ones (``pixels_<name>.npz``,
``regions_<name>.npz``: the same keys, ``connectivity`` in {26, 18, 6}), so ``ood_detection.py --score pixel`` reads them as they are.

``--voxel_calibrate_fpr`` and ``--voxel_segment 1`` are ``--pixel_calibrate_fpr`` and ``--pixel_segment 1`` for volumes:
``calibration.npz`` / ``calibrated_<name>.npz`` and ``segments_<name>.npz`` with the 2-D keys (``segmentation`` [N, 2, T, D, H, W]).

``VoxelSettings`` is the flags, checked from the Namespace alone; ``MapPipeline`` takes it by keyword.  ``count_batch`` is one
batch's device work -- the histogram and counts kernels are flat over the voxels, the three region ops are those of
csrc/regions3d.hip --, ``segment_batch`` its segmentations (csrc/segment3d.hip) and ``collect`` / ``collect_segments`` the pass's
collectives and files.  With the flags off nothing here is called.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist

from . import ops, pixel_metrics, zmaps

FLAG = "--voxel_metrics 1"
REGION_FLAG = "--voxel_regions 1"
CALIBRATE_FLAG, BUDGET_FLAG = "--voxel_calibrate_fpr", "--voxel_calibrate_budget_gb"
SEGMENT_FLAG = "--voxel_segment 1"
DEFAULT_MEDIAN, DEFAULT_MIN_COMPONENT = 3, 8
MEDIAN_SIZES = (1, 3)
MAX_MIN_COMPONENT = 2 ** 31 - 1
SEG_MAX_VOXELS = 1 << 24  # the segmentations' integer rows travel as fp32: a count of voxels must stay exact
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
    calibrate: bool = False  # calibration.npz (and calibrated_<name>.npz with metrics) of volumes: thresholds at target rates
    cal_fprs: list = None
    cal_budget: int = None
    segment: bool = False  # segments_<name>.npz of volumes: 3 x 3 x 3 median, components below a minimum size removed
    median: int = None
    min_component: int = None

    @property
    def active(self) -> bool:
        return self.metrics or self.calibrate or self.segment

    @classmethod
    def from_args(cls, args):
        """Every refusal the voxel flags can earn, as ValueError naming the flag, from the Namespace alone."""
        metrics, regions = bool(getattr(args, "voxel_metrics", 0)), bool(getattr(args, "voxel_regions", 0))
        calibrate, segment = bool(getattr(args, "voxel_calibrate_fpr", None)), bool(getattr(args, "voxel_segment", 0))
        if not (metrics or regions or calibrate or segment):
            return cls()
        flag = FLAG if metrics else REGION_FLAG if regions else CALIBRATE_FLAG if calibrate else SEGMENT_FLAG
        if regions and not metrics:
            raise ValueError(f"{REGION_FLAG} adds to the voxel metrics: it needs {FLAG}")
        for name in PIXEL_FLAGS:
            if getattr(args, name, None):
                raise ValueError(f"{flag}: not together with --{name} (the --pixel_* flags evaluate 2-D maps, the --voxel_* flags volumes: "
                                 f"--voxel_{name[len('pixel_'):]} is its counterpart for volumes)")
        if int(args.spatial_dimension) != 3:
            raise ValueError(f"{flag}: the voxel flags evaluate volumes, they need --spatial_dimension 3 (2-D images: --pixel_metrics 1, "
                             f"--pixel_calibrate_fpr, --pixel_segment 1)")
        if not bool(getattr(args, "anomaly_volume_z_maps", 0)):
            raise ValueError(f"{flag} evaluates the Z-maps of volumes: it needs {zmaps.VOLUME_FLAG} (the raw maps have no fixed scale)")
        voxels = namespace_voxels(args)
        if voxels is not None and voxels > MAX_VOXELS:
            raise ValueError(f"{flag}: volumes of {voxels} voxels (--image_size / --image_roi) do not fit the 32-bit voxel indices and "
                             f"counts: D H W must stay below 2^31")
        bins = getattr(args, "pixel_bins", pixel_metrics.DEFAULT_BINS), getattr(args, "pixel_range", None) or pixel_metrics.DEFAULT_RANGE
        thresholds = getattr(args, "pixel_thresholds", None) or pixel_metrics.DEFAULT_THRESHOLDS
        s = {}
        try:
            if metrics:
                lo, hi, nbins, thr, masks = pixel_metrics.check_flags(
                    True, args.out_ids if bool(getattr(args, "run_out", 1)) else None, getattr(args, "out_masks", None), *bins, thresholds)
                s.update(metrics=True, lo=lo, hi=hi, bins=nbins, thresholds=thr, masks=masks)
            if calibrate:
                s["cal_fprs"], s["cal_budget"] = pixel_metrics.check_calibration_flags(
                    True, args.voxel_calibrate_fpr, getattr(args, "voxel_calibrate_budget_gb", pixel_metrics.DEFAULT_BUDGET_GB))
                s["calibrate"] = True
                if not metrics:  # (the bins of the validation histogram are those of --pixel_range / --pixel_bins)
                    s["lo"], s["hi"], s["bins"] = pixel_metrics.check_flags(True, None, None, *bins)[:3]
        except ValueError as e:  # (the shared flags keep their names; the message leads with this flag)
            raise ValueError(str(e).replace(pixel_metrics.FLAG, FLAG).replace(pixel_metrics.CALIBRATE_FLAG, CALIBRATE_FLAG)
                             .replace(pixel_metrics.BUDGET_FLAG, BUDGET_FLAG)) from None
        if segment:
            median, small = getattr(args, "voxel_median", DEFAULT_MEDIAN), getattr(args, "voxel_min_component", DEFAULT_MIN_COMPONENT)
            try:
                m, n = int(median), int(small)
                if m != float(median) or n != float(small):
                    raise ValueError
            except (TypeError, ValueError):
                raise ValueError(f"{SEGMENT_FLAG}: --voxel_median and --voxel_min_component are integers, got {median!r} and {small!r}") from None
            if m not in MEDIAN_SIZES:
                raise ValueError(f"{SEGMENT_FLAG}: --voxel_median must be 1 (no filter) or 3, got {median} (a 5 x 5 x 5 median is not built)")
            if not 1 <= n <= MAX_MIN_COMPONENT:
                raise ValueError(f"{SEGMENT_FLAG}: --voxel_min_component must lie in 1 .. {MAX_MIN_COMPONENT}, got {small}")
            try:
                thr = pixel_metrics.parse_thresholds(thresholds)
            except ValueError as e:
                raise ValueError(str(e).replace(pixel_metrics.FLAG, SEGMENT_FLAG)) from None
            if not 1 <= len(thr) <= pixel_metrics.MAX_THRESHOLDS or not all(np.isfinite(thr)):
                raise ValueError(f"{SEGMENT_FLAG}: --pixel_thresholds takes 1 .. {pixel_metrics.MAX_THRESHOLDS} finite numbers, got {thr}")
            s.update(segment=True, median=m, min_component=n, thresholds=thr)
        if regions or segment:
            connectivity = getattr(args, "voxel_connectivity", DEFAULT_CONNECTIVITY)
            pro_fpr = getattr(args, "voxel_pro_fpr", DEFAULT_PRO_FPR)
            which = REGION_FLAG if regions else SEGMENT_FLAG
            try:
                conn, fpr = int(connectivity), float(pro_fpr)
            except (TypeError, ValueError):
                raise ValueError(f"{which}: --voxel_connectivity is 26, 18 or 6 and --voxel_pro_fpr a number, got {connectivity!r} "
                                 f"and {pro_fpr!r}") from None
            if conn != float(connectivity) or conn not in CONNECTIVITIES:
                raise ValueError(f"{which}: --voxel_connectivity must be 26, 18 or 6, got {connectivity}")
            if regions and not 0.0 < fpr <= 1.0:
                raise ValueError(f"{REGION_FLAG}: --voxel_pro_fpr must lie in (0, 1], got {pro_fpr}")
            s.update(connectivity=conn)
            if regions:
                s.update(regions=True, pro_fpr=fpr)
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


def segment_scratch_bytes(B: int, K: int, P: int) -> int:
    items = B * K
    return 4 * (items * 2 * P + items * 2 * (P // 32 + 1) + items * -(-P // 256) * 6 + items)


def segment_words(T: int, P: int) -> int:
    """fp32 values of a volume's packed segmentations: 16 voxels to a value (map_passes.SEG_BITS)."""
    return -(-2 * T * P // 16)


def segment_bytes(B: int, P: int, s: VoxelSettings, labelled: bool) -> int:
    """What ``segment_batch`` allocates: the median's buffer over the 2 B volumes, per call of ``map_segment3d`` (K thresholds, then
    the F calibrated ones; the larger stands for both) seg, the integers and the scratch, the two channels' seg kept until they are
    packed, and the transport (16 voxels to an fp32, as in 2-D); without ``labelled`` (the labels of
    ``count_batch``) the mask, its labels and the labelling's scratch."""
    K, F = len(s.thresholds), len(s.cal_fprs) if s.calibrate else 0
    T, most = K + F, max(K, F)
    need = (2 * B * P * 4 if s.median > 1 else 0) + 4 * B * P + segment_scratch_bytes(B, most, P) + 32 * B * most
    # seg per channel, stacked and padded: 3 x 2 B T P bytes; the bits as int32 and their products: 2 x 4 x 2 B T P; packed int32 and fp32
    need += 22 * B * T * P + 2 * 4 * B * segment_words(T, P)
    if not labelled:
        need += B * P + 4 * B * P + 4 * B + label_scratch_bytes(B, P)
    return int(need)


def batch_bytes(B: int, extent, s: VoxelSettings) -> int:
    """What ``count_batch`` allocates for a batch of B volumes: the mask, one channel's Z-map, the histogram slabs and counts; with
    regions the labels, the three scratch buffers (the forests of the mask and of the K thresholded maps, the overlap tables) and
    the component counts.  The two channels run one after the other through the same sizes."""
    P = int(np.prod([int(e) for e in extent], dtype=object))
    need = 0
    if s.metrics:
        K = len(s.thresholds)
        need += B * P + 4 * B * P + ops.map_hist_parts(B * P) * 2 * (s.bins + 1) * 4 + 2 * 12 * B * K
        if s.regions:
            need += 4 * B * P + 4 * B + label_scratch_bytes(B, P) + overlap_scratch_bytes(B, s.bins, ops.map_region_overlap3d_chunk(s.bins)) \
                + counts_scratch_bytes(B, K, P) + 2 * 12 * B * K
        if s.calibrate:  # one more counts call (with regions: and one more component-counts call) per channel at the F thresholds
            F = len(s.cal_fprs)
            need += 2 * 12 * B * F + ((counts_scratch_bytes(B, F, P) + 2 * 12 * B * F) if s.regions else 0)
    if s.segment:
        need += segment_bytes(B, P, s, labelled=s.metrics and s.regions)
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
        flag = REGION_FLAG if s.regions else FLAG if s.metrics else SEGMENT_FLAG
        raise ValueError(f"{flag}: a batch of {B} volumes of {shape} takes {maps / (1 << 30):.3f} GiB of per-t "
                         f"maps and {mine / (1 << 30):.3f} GiB of masks, labels, forests and tables, over the budget of "
                         f"{budget_bytes / (1 << 30):.3f} GiB: lower --batch_size or raise --anomaly_volume_budget_gb")
    return maps + mine


# ---- one batch, one pass -------------------------------------------------------------------------------------------------------

def count_batch(mp, z, mask, extent, n_t: int):
    """``z`` [B, 2, D H W] on the device, the final Z-maps of a batch, against ``mask`` (uint8 [B, 1, D, H, W]; None: all zero).  Per
    channel one histogram launch into the pass's [2, 2, nbins + 1] table and one counts launch; with regions the mask labelled
    once, then per channel one overlap call into the pass's float64 [2, nbins + 1] table and one component-counts call.  With
    --voxel_calibrate_fpr per channel one more counts call (with regions: and one more component-counts call) at its calibrated
    thresholds.  Mask, labels and regions are arguments between the steps.  Returns (the device's columns of the row by name, the
    masks' voxel counts [B] on the host, (mask, labels, regions) for ``segment_batch``)."""
    p, s = mp.p, mp.p.voxel
    B, _, P = z.shape
    m, mask_voxels = mp.device_mask(mask, B, P, FLAG)
    if mp.hist is None:
        mp.hist = torch.zeros((2, 2, s.bins + 1), dtype=torch.int64, device=p.device)
    if s.regions and mp.overlap is None:
        mp.overlap = torch.zeros((2, s.bins + 1), dtype=torch.float64, device=p.device)
    labels = regions = None
    if s.regions:
        labels, regions = ops.map_label3d(m.reshape((B,) + tuple(extent)), s.connectivity)
    cal = p.calibration(mp.t_values)["thr"] if s.calibrate else None
    counts, components, cal_counts, cal_components = [], [], [], []
    for c in range(2):
        zc = z[:, c].contiguous()
        ops.map_mask_hist(zc, m, s.lo, s.hi, s.bins, total=mp.hist[c])
        counts.append(ops.map_mask_counts(zc, m, p.thresholds))
        if cal is not None:
            cal_counts.append(ops.map_mask_counts(zc, m, cal[c].contiguous()))
        if s.regions:
            zv = zc.reshape((B,) + tuple(extent))
            ops.map_region_overlap3d(zv, labels, regions, s.lo, s.hi, s.bins, total=mp.overlap[c])
            components.append(ops.map_component_counts3d(zv, m.reshape(zv.shape), labels, regions, p.thresholds, s.connectivity))
            if cal is not None:
                cal_components.append(ops.map_component_counts3d(zv, m.reshape(zv.shape), labels, regions, cal[c].contiguous(), s.connectivity))
    parts = {"counts": torch.stack(counts, dim=1)}
    if s.regions:
        parts["components"], parts["regions"] = torch.stack(components, dim=1), regions
    if cal is not None:  # [B, R 2 F 3]: the counts, then with regions the components (RowLayout's "calibrated")
        parts["calibrated"] = torch.cat([torch.stack(kind, dim=1).reshape(B, -1) for kind in (cal_counts, cal_components) if kind], dim=1)
    return parts, mask_voxels, (m, labels, regions)


def segment_batch(mp, z, mask, extent, truth=None):
    """--voxel_segment 1: ``z`` [B, 2, D H W] on the device, the final Z-maps.  One median launch over the 2 B volumes (none at
    --voxel_median 1), the mask labelled once (``truth``: the mask, labels and regions of ``count_batch``, reused when it labelled),
    per channel one ``map_segment3d`` call at the fixed thresholds and, with --voxel_calibrate_fpr, one at the channel's calibrated
    ones.  The segmentations, 16 voxels to an fp32, and the integer row behind them reach the host in ONE copy."""
    from .map_passes import SEG_BITS

    p, s = mp.p, mp.p.voxel
    B, _, P = z.shape
    if P >= SEG_MAX_VOXELS:
        raise ValueError(f"{SEGMENT_FLAG}: a count of up to {P} voxels is not exact in the fp32 rows the segmentations travel in (D H W "
                         f"must stay below 2^24)")
    shape = (B,) + tuple(extent)
    m, labels, regions = truth if truth is not None else (None, None, None)
    if m is None:
        m, _ = mp.device_mask(mask, B, P, SEGMENT_FLAG)
    mask_voxels = torch.zeros(B, dtype=torch.int64) if mask is None else (mask.reshape(B, P) != 0).sum(dim=1).cpu()
    m = m.reshape(shape)
    if labels is None:
        labels, regions = ops.map_label3d(m, s.connectivity)
    vols = z.reshape((2 * B,) + tuple(extent))
    if s.median > 1:
        vols = ops.map_median3d(vols.contiguous(), s.median)
    vols = vols.reshape((B, 2) + tuple(extent))
    cal = p.calibration(mp.t_values)["thr"] if s.calibrate else None
    per_channel = []
    for c in range(2):
        zc = vols[:, c].contiguous()
        got = [ops.map_segment3d(zc, m, labels, regions, p.seg_thresholds, s.min_component, s.connectivity)]
        if cal is not None:
            got.append(ops.map_segment3d(zc, m, labels, regions, cal[c].contiguous(), s.min_component, s.connectivity))
        per_channel.append([torch.cat(kind, dim=1) for kind in zip(*got)])  # (seg, pixels, components, removed), each [B, T, ...]
    seg, pixels, components, removed = (torch.stack(kind, dim=1) for kind in zip(*per_channel))  # [B, 2, T, ...]
    bits = seg.reshape(B, -1)
    pad = -bits.shape[1] % SEG_BITS
    if pad:
        bits = torch.nn.functional.pad(bits, (0, pad))
    packed = (bits.reshape(B, -1, SEG_BITS).to(torch.int32) * p.seg_bit_weights).sum(dim=2)
    ints = p.seg_layout.without("mask_pixels").pack({"pixels": pixels, "components": components, "removed": removed, "regions": regions[:, None]})
    row = torch.cat([packed, ints], dim=1).to(torch.float32).cpu()  # (every entry is an integer below 2^24: exact)
    mp.seg_plane = tuple(extent)
    mp.seg_rows.append(torch.cat([row, mask_voxels.to(torch.float32)[:, None]], dim=1))


def collect_segments(mp, files, t, results, *ids):
    """--voxel_segment 1: ONE gather of the rows (packed segmentation, integers); the file, saved compressed, has the keys of the 2-D
    one, ``segmentation`` uint8 [N, 2, T, D, H, W]."""
    from .map_passes import SEGMENTS, unpack_segmentation

    p, s = mp.p, mp.p.voxel
    got = mp._gather(SEGMENT_FLAG, mp.seg_rows, results, *ids)
    if got is None:
        return
    extent = tuple(mp.seg_plane)
    T, K = p.seg_T, len(s.thresholds)
    words = segment_words(T, int(np.prod(extent, dtype=np.int64)))
    row = p.seg_layout.unpack(np.rint(got[1][:, words:]).astype(np.int64))
    thresholds = np.repeat(np.asarray(s.thresholds, dtype=np.float32)[None], 2, axis=0)
    fpr = np.full(K, np.nan, dtype=np.float64)
    if s.calibrate:
        cal = p.calibration(mp.t_values)
        thresholds = np.concatenate([thresholds, np.asarray(cal["thresholds"], dtype=np.float32)], axis=1)
        fpr = np.concatenate([fpr, np.asarray(cal["fpr"], dtype=np.float64)])
    arrays = {"filename": np.asarray(got[0]), "t": t, "channels": np.asarray(zmaps.CHANNELS), "thresholds": thresholds, "fpr": fpr,
              "median": np.int64(s.median), "min_component": np.int64(s.min_component), "connectivity": np.int64(s.connectivity),
              "sigma": np.float64(p.s.z_sigma), "segmentation": unpack_segmentation(got[1][:, :words], (2, T) + extent),
              "pixels": row["pixels"].astype(np.int32), "components": row["components"].astype(np.int32),
              "removed": row["removed"].astype(np.int32), "mask_pixels": row["mask_pixels"], "regions": row["regions"].astype(np.int32)}
    files[SEGMENTS] = lambda path, arrays=arrays: np.savez_compressed(path, **arrays)


def collect(mp, files, t, results, *ids):
    """The histogram (and the overlap table) summed over the ranks, ONE all_reduce each, and every rank's integer rows in the CSV's
    order (the gather's payload is fp32, so a count must stay below 2^24 with more than one rank): ``files`` gains PIXELS and,
    with regions, REGIONS -- the keys of the 2-D files."""
    from .map_passes import CALIBRATED, PIXELS, REGIONS, host_if_gloo

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
    if s.calibrate:  # counts int32 [N, 2, F, 3] = (TP, FP, FN), with --voxel_regions 1 components = (hit, pred, false_pred)
        cal, at = p.calibration(mp.t_values), row["calibrated"].astype(np.int32)
        files[CALIBRATED] = {"filename": stems, "fpr": np.asarray(cal["fpr"], dtype=np.float64),
                             "thresholds": np.asarray(cal["thresholds"], dtype=np.float32), "counts": at[:, 0]}
        if s.regions:
            files[CALIBRATED]["components"] = at[:, 1]
    if s.regions:
        files[REGIONS] = {**head, "connectivity": np.int64(s.connectivity), "regions": row["regions"].astype(np.int32),
                          "overlap": overlap.cpu().numpy().astype(np.float64), "thresholds": thresholds,
                          "components": row["components"].astype(np.int32), "sigma": np.float64(p.s.z_sigma)}
    files[PIXELS] = {**head, "hist": hist.cpu().numpy().astype(np.int64), "thresholds": thresholds,
                     "counts": row["counts"].astype(np.int32), "mask_pixels": row["mask_pixels"], "sigma": np.float64(p.s.z_sigma)}
    return files
