"""The anomaly-map stack of ``reconstruct.py``: what ``Reconstruct`` does with a batch's maps once its scores
are final.  ``MapSettings`` is the six opt-in flags, checked before any device is touched; ``MapPipeline`` holds what outlives a
pass, ``MapPass`` what one ``get_scores`` call accumulates, and ``RowLayout`` names the columns of the per-image integer row that
rides behind the Z-map bits in a batch's one device->host copy.  Everything is built lazily: with every flag off nothing is
allocated, launched, gathered or written.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from . import ops, pixel_metrics, voxel_passes, zmaps

# what ``MapPass.collect`` returns on rank 0: {file name with the set's name left open: the arrays of the .npz, in key order}
MAPS, ZMAPS, PIXELS, REGIONS, CALIBRATED, SEGMENTS = (f"{kind}_{{name}}.npz" for kind in ("maps", "zmaps", "pixels", "regions", "calibrated",
                                                                                         "segments"))
SEG_BITS = 16  # pixels of a segmentation per fp32 of a row: a sum of 16 distinct powers of two below 2^16 is exact


@dataclass(frozen=True)
class MapSettings:
    """The extension flags of the stack.  bench.py and the tests build their Namespace by hand without the attributes: off."""
    anomaly_maps: bool = False  # maps_<name>.npz: per-pixel LPIPS and squared error, the mean over the t-starts
    anomaly_z_maps: bool = False  # map_stats.npz, zmaps_<name>.npz: the per-t maps normalised per pixel
    z_sigma: float = 0.0
    z_std_floor: float = 0.01
    pixel_metrics: bool = False  # pixels_<name>.npz: the in / out sets' Z-maps against --out_masks
    px_lo: float = None
    px_hi: float = None
    px_bins: int = None
    px_thresholds: list = None
    px_masks: list = None
    pixel_regions: bool = False  # regions_<name>.npz: connected components, overlap table, component counts
    px_connectivity: int = None
    px_calibrate: bool = False  # calibration.npz, calibrated_<name>.npz: thresholds at target false-positive rates
    cal_fprs: list = None
    cal_budget: int = None
    keep_calibration_rows: bool = False  # test hook (not a CLI flag): see ``MapPipeline.calibration_rows``
    pixel_segment: bool = False  # segments_<name>.npz: the Z-maps thresholded, median-filtered, small components removed
    sg_median: int = None
    sg_min_component: int = None
    sg_thresholds: list = None
    sg_connectivity: int = None
    volume_maps: bool = False  # maps_<name>.npz of volumes [N, D, H, W]: 2.5-D LPIPS and squared error per voxel
    volume_z_maps: bool = False  # map_stats.npz, zmaps_<name>.npz of volumes; --anomaly_z_sigma smooths in 3-D
    volume_views: str = "last"  # the slice directions of the LPIPS map: the view whose value is the score, or all three
    volume_budget: int = None  # bytes a batch's maps may take on the device

    @property
    def want_maps(self) -> bool:
        return self.anomaly_maps or self.volume_maps

    @property
    def want_z_maps(self) -> bool:
        return self.anomaly_z_maps or self.volume_z_maps

    @property
    def volume(self) -> bool:
        return self.volume_maps or self.volume_z_maps

    @classmethod
    def from_args(cls, args):
        """Every refusal the flags can earn, as ValueError, from the Namespace alone (no device, library or checkpoint)."""
        s = dict(anomaly_maps=bool(getattr(args, "anomaly_maps", 0)), anomaly_z_maps=bool(getattr(args, "anomaly_z_maps", 0)),
                 z_sigma=float(getattr(args, "anomaly_z_sigma", 0.0) or 0.0), z_std_floor=float(getattr(args, "anomaly_z_std_floor", 0.01)),
                 pixel_metrics=bool(getattr(args, "pixel_metrics", 0)), pixel_regions=bool(getattr(args, "pixel_regions", 0)),
                 px_calibrate=bool(getattr(args, "pixel_calibrate_fpr", None)), pixel_segment=bool(getattr(args, "pixel_segment", 0)),
                 keep_calibration_rows=bool(getattr(args, "keep_calibration_rows", False)))
        if s["anomaly_maps"] and (int(args.spatial_dimension) != 2 or args.vqvae_checkpoint):
            raise ValueError("--anomaly_maps 1: anomaly maps cover 2-D pixel-space models only (no --spatial_dimension 3, no "
                             "--vqvae_checkpoint): 2.5-D and latent maps are not built")
        if s["anomaly_z_maps"]:
            zmaps.check_flags(args.spatial_dimension, args.vqvae_checkpoint, s["z_sigma"], s["z_std_floor"])
        s.update(check_volume_flags(args, s))
        bins = getattr(args, "pixel_bins", pixel_metrics.DEFAULT_BINS), getattr(args, "pixel_range", None) or pixel_metrics.DEFAULT_RANGE
        if s["pixel_metrics"]:
            s["px_lo"], s["px_hi"], s["px_bins"], s["px_thresholds"], s["px_masks"] = pixel_metrics.check_flags(
                s["anomaly_z_maps"], args.out_ids if bool(args.run_out) else None, getattr(args, "out_masks", None), *bins,
                getattr(args, "pixel_thresholds", None) or pixel_metrics.DEFAULT_THRESHOLDS)
        if s["pixel_regions"]:
            s["px_connectivity"] = pixel_metrics.check_region_flags(  # (--pixel_pro_fpr: checked here, used by ood_detection.py)
                s["pixel_metrics"], getattr(args, "pixel_connectivity", pixel_metrics.DEFAULT_CONNECTIVITY),
                getattr(args, "pixel_pro_fpr", pixel_metrics.DEFAULT_PRO_FPR))[0]
        if s["px_calibrate"]:
            s["cal_fprs"], s["cal_budget"] = pixel_metrics.check_calibration_flags(
                s["anomaly_z_maps"], args.pixel_calibrate_fpr, getattr(args, "pixel_calibrate_budget_gb", pixel_metrics.DEFAULT_BUDGET_GB))
            if not s["pixel_metrics"]:  # (the bins of the validation histogram are those of --pixel_range / --pixel_bins)
                s["px_lo"], s["px_hi"], s["px_bins"] = pixel_metrics.check_flags(True, None, None, *bins)[:3]
        if s["pixel_segment"]:
            s["sg_median"], s["sg_min_component"], s["sg_thresholds"], s["sg_connectivity"] = pixel_metrics.check_segment_flags(args)
        return cls(**s)


VOLUME_VIEWS = ("last", "all")
DEFAULT_VOLUME_BUDGET_GB = 8.0


def check_volume_flags(args, s) -> dict:
    """The volume flags' fields of ``MapSettings`` ({} with both off), or the refusals they earn, from the Namespace alone."""
    on = {"volume_maps": bool(getattr(args, "anomaly_volume_maps", 0)), "volume_z_maps": bool(getattr(args, "anomaly_volume_z_maps", 0))}
    if not any(on.values()):
        return {}
    flag = "--anomaly_volume_maps 1" if on["volume_maps"] else zmaps.VOLUME_FLAG
    if int(args.spatial_dimension) != 3:
        raise ValueError(f"{flag}: the maps of volumes need --spatial_dimension 3 (2-D images: --anomaly_maps 1 / --anomaly_z_maps 1)")
    if (on["volume_maps"] and s["anomaly_maps"]) or (on["volume_z_maps"] and s["anomaly_z_maps"]):
        raise ValueError(f"{flag}: not together with its 2-D counterpart (--anomaly_maps 1 / --anomaly_z_maps 1): they write the same files")
    for name in ("pixel_metrics", "pixel_regions", "pixel_calibrate_fpr", "pixel_segment"):
        if getattr(args, name, None):
            raise ValueError(f"{flag}: --{name} is not built for volumes (the --pixel_* flags cover 2-D maps only: its counterpart for "
                             f"volumes is --voxel_{name[len('pixel_'):]})")
    if on["volume_z_maps"]:
        zmaps.check_volume_flags(args.spatial_dimension, s["z_sigma"], s["z_std_floor"])
    views = getattr(args, "anomaly_volume_views", "last")
    if views not in VOLUME_VIEWS:
        raise ValueError(f"{flag}: --anomaly_volume_views must be one of {VOLUME_VIEWS}, got {views!r}")
    budget_gb = float(getattr(args, "anomaly_volume_budget_gb", DEFAULT_VOLUME_BUDGET_GB))
    if not budget_gb > 0:
        raise ValueError(f"{flag}: --anomaly_volume_budget_gb must be positive, got {budget_gb}")
    return dict(on, volume_views=views, volume_budget=int(budget_gb * (1 << 30)))


def check_volume_budget(B: int, n_t: int, extent, per_t: bool, budget_bytes: int) -> int:
    """The bytes of a batch's maps on the device -- B x 2 x D H W fp32 accumulated, with the Z-maps B x n_t x 2 x D H W for the
    per-t stack -- or ValueError when they exceed the budget (before anything is allocated)."""
    voxels = int(np.prod([int(e) for e in extent], dtype=np.int64))
    need = int(B) * (int(n_t) if per_t else 1) * 2 * voxels * 4
    if need > int(budget_bytes):
        shape = " x ".join(str(int(e)) for e in extent)
        raise ValueError(f"--anomaly_volume_{'z_' if per_t else ''}maps 1: the maps of a batch of {B} volumes ({B} x {n_t if per_t else 1} x 2 x "
                         f"{shape} fp32 = {need / (1 << 30):.3f} GiB) exceed the budget of {budget_bytes / (1 << 30):.3f} GiB: lower "
                         f"--batch_size or raise --anomaly_volume_budget_gb")
    return need


class RowLayout:
    """The per-image integer row of --pixel_metrics 1, as named segments: ``counts`` [2, K, 3], ``mask_pixels`` []; with regions
    ``components`` [2, K, 3], ``regions`` []; with F calibrated thresholds ``calibrated`` [R, 2, F, 3] (R = 1: the counts; with regions
    R = 2: then the components).  One object packs the row and takes the host copy and the gathered rows apart."""
    def __init__(self, K: int, F: int = 0, regions: bool = False, segments=None):
        self.segments = segments if segments is not None else (
            [("counts", (2, K, 3)), ("mask_pixels", ())] + ([("components", (2, K, 3)), ("regions", ())] if regions else [])
            + ([("calibrated", (2 if regions else 1, 2, F, 3))] if F else []))
        self.width = sum(int(np.prod(shape, dtype=np.int64)) for _, shape in self.segments)

    def without(self, *names):
        """The layout of the same row with these columns left out (what the device fills in: all but ``mask_pixels``)."""
        return RowLayout(0, segments=[seg for seg in self.segments if seg[0] not in names])

    def pack(self, parts: dict, lead=()) -> torch.Tensor:
        """int32 [B, (lead) + width]: every segment's tensor in the row's order, behind the int32 [B, n] tensors of ``lead``."""
        return torch.cat(list(lead) + [parts[name].reshape(parts[name].shape[0], -1).to(torch.int32) for name, _ in self.segments], dim=1)

    def unpack(self, rows) -> dict:
        """{name: [n, *shape]} of rows [n, width] (a torch tensor or a numpy array, of any dtype)."""
        if rows.ndim != 2 or rows.shape[1] != self.width:
            raise ValueError(f"rows of {tuple(rows.shape)} for a layout of {self.width} columns {[n for n, _ in self.segments]}")
        out, at = {}, 0
        for name, shape in self.segments:
            size = int(np.prod(shape, dtype=np.int64))
            out[name] = rows[:, at:at + size].reshape((rows.shape[0],) + tuple(shape))
            at += size
        return out


def host_if_gloo(t: torch.Tensor) -> torch.Tensor:
    """Before a collective.  Test hook (two ranks on one GPU): gloo moves host memory, so a device tensor goes through the host."""
    return t.cpu() if dist.get_backend() == "gloo" and t.is_cuda else t


def gather_rows(ids: torch.Tensor, rows: torch.Tensor, n_max: int = None, who: str = "gather_rows"):
    """ONE all_gather of dense per-image rows of any trailing shape (RCCL over xGMI; gloo in the CPU tests).  ids: int32 [n_local]
    global image indices; rows: fp32 [n_local, ...]; n_max: the static shard capacity ceil(n_images / world), which every rank
    can compute from the id list, so no size exchange is needed.  Each rank sends a dense [n_max, 1 + row size] fp32 payload, ids
    in column 0 (exact below 2^24: one collective, not two), short shards padded with id = -1; the padding is dropped after the
    gather and ``counts`` (rows per rank) read off the ids.  Returns (ids, rows, counts) rank-major on every rank."""
    if not dist.is_initialized():
        return ids, rows, [int(ids.shape[0])]
    world = dist.get_world_size()  # a 1-rank group still goes through the collective (same code path as N ranks)
    if n_max is None:
        n_max = int(ids.shape[0]) if world == 1 else None
    if n_max is None or ids.shape[0] > n_max:
        raise ValueError(f"{who}: shard of {ids.shape[0]} rows does not fit the static capacity {n_max}")
    if rows.shape[0] != ids.shape[0]:
        raise ValueError(f"{who}: {rows.shape[0]} rows for {ids.shape[0]} ids")
    if ids.numel() and int(ids.max()) >= 1 << 24:
        raise ValueError(f"{who}: image id {int(ids.max())} is not exact in the fp32 payload (ids must be < 2^24)")
    trailing = tuple(rows.shape[1:])
    width = int(np.prod(trailing, dtype=np.int64))
    payload = torch.full((n_max, width + 1), -1.0, dtype=torch.float32, device=rows.device)
    payload[: ids.shape[0], 0] = ids.to(device=rows.device, dtype=torch.float32)
    payload[: ids.shape[0], 1:] = rows.reshape(ids.shape[0], width)  # (an empty shard has 0 rows)
    payload = host_if_gloo(payload)
    out = torch.empty((world * n_max, width + 1), dtype=torch.float32, device=payload.device)
    dist.all_gather_into_tensor(out, payload)
    out = out.to(rows.device)
    valid = out[:, 0] >= 0
    counts = valid.reshape(world, n_max).sum(dim=1).tolist()
    out = out[valid]
    return out[:, 0].to(torch.int32), out[:, 1:].reshape((-1,) + trailing), [int(c) for c in counts]


def check_plane(flag: str, H: int, W: int):
    """The labelling holds a plane's 16-bit parents in LDS."""
    if H * W > ops.MAP_LABEL_MAX_PIXELS:
        raise ValueError(f"{flag}: maps of {H} x {W} pixels are above the {ops.MAP_LABEL_MAX_PIXELS} pixels "
                         f"(128 x 128) a labelled plane may have")


def unpack_segmentation(packed, shape):
    """uint8 [n, *shape] from the rows' fp32 [n, ceil(prod(shape) / SEG_BITS)] (numpy), SEG_BITS pixels to a value, lowest bit first."""
    v = np.rint(packed).astype(np.int64)
    bits = ((v[:, :, None] >> np.arange(SEG_BITS)) & 1).astype(np.uint8).reshape(v.shape[0], -1)
    return np.ascontiguousarray(bits[:, :int(np.prod(shape, dtype=np.int64))]).reshape((v.shape[0],) + tuple(shape))


def file_stem(filename) -> str:
    """The ``filename`` column of the CSV (reconstruct.py:192-204 of the reference strips .nii / .gz as well)."""
    return Path(filename).stem.replace(".nii", "").replace(".gz", "")


def map_rows_in_csv_order(results, ids, name_of):
    """Which gathered row belongs to which line of ``maps_<name>.npz``: (stems, picks) with ``stems`` the CSV's filenames in
    their order of first appearance in ``results`` (the row dicts of ``rows_from_scores``) and ``picks[k]`` the position in
    ``ids`` (the gathered image ids, rank-major) of the first row whose image carries the name ``stems[k]``."""
    first = {}
    for k, i in enumerate(ids):
        first.setdefault(file_stem(name_of.get(int(i), str(int(i)))), k)
    stems = list(dict.fromkeys(r["filename"] for r in results))
    return stems, [first[s] for s in stems]


class MapPipeline:
    """What outlives a pass, each built at its first use: the Z tables the in / out sets are normalised by, the smoothing taps,
    the fixed thresholds and an all-zero mask on the device, the calibration in force, and the two results of a validation pass."""
    def __init__(self, s: MapSettings, device, out_dir, rank: int = 0, world: int = 1, ddp: bool = False, voxel=None):
        self.s, self.device, self.out_dir, self.rank, self.world, self.ddp = s, device, Path(out_dir), rank, world, ddp
        self.voxel = voxel if voxel is not None and voxel.active else None  # voxel_passes.VoxelSettings; None: off
        self.layout = RowLayout(len(s.px_thresholds), len(s.cal_fprs) if s.px_calibrate else 0, s.pixel_regions) if s.pixel_metrics else None
        if self.voxel and self.voxel.metrics:  # (never beside --pixel_metrics 1: refused) the same row, with the voxel flags' thresholds
            self.layout = RowLayout(len(self.voxel.thresholds), len(self.voxel.cal_fprs) if self.voxel.calibrate else 0, self.voxel.regions)
        self.device_layout = self.layout.without("mask_pixels") if self.layout else None  # (the masks' pixel counts are taken on the host)
        self.last_map_stats = None  # (MapStats, t values) of the last validation pass, merged over the ranks
        self.last_calibration = None  # the contents of ood/calibration.npz after a validation pass with --pixel_calibrate_fpr
        # ``keep_calibration_rows``: this rank's retained validation rows [n, n_t, 2, H, W] and their leave-one-out Z-maps, on the host
        self.calibration_rows = self.calibration_zmaps = None
        self._tables = self._taps = self._no_mask = self._cal = None
        # --pixel_segment 1: T thresholds per channel (the fixed ones, then the calibrated ones); the integer row of an image
        self.seg_T = (len(s.sg_thresholds) + (len(s.cal_fprs) if s.px_calibrate else 0)) if s.pixel_segment else 0
        if self.voxel and self.voxel.segment:  # --voxel_segment 1 (never beside --pixel_segment 1: refused): the same row
            self.seg_T = len(self.voxel.thresholds) + (len(self.voxel.cal_fprs) if self.voxel.calibrate else 0)
        self.seg_layout = RowLayout(0, segments=[("pixels", (2, self.seg_T, 3)), ("components", (2, self.seg_T, 3)),
                                                 ("removed", (2, self.seg_T, 2)), ("regions", ()), ("mask_pixels", ())]) if self.seg_T else None

    @property
    def calibrating(self) -> bool:
        return self.s.px_calibrate or bool(self.voxel and self.voxel.calibrate)

    @property
    def cal_grid(self):
        """(flag, budget flag, lo, hi, bins, target rates, budget in bytes) of the calibration in force: the voxel flags' or the 2-D ones'."""
        v, s = self.voxel, self.s
        if v and v.calibrate:
            return voxel_passes.CALIBRATE_FLAG, voxel_passes.BUDGET_FLAG, v.lo, v.hi, v.bins, v.cal_fprs, v.cal_budget
        return pixel_metrics.CALIBRATE_FLAG, pixel_metrics.BUDGET_FLAG, s.px_lo, s.px_hi, s.px_bins, s.cal_fprs, s.cal_budget

    def begin(self, dataset_name: str, loader, t_values) -> "MapPass":
        return MapPass(self, dataset_name, loader, t_values)

    def smooth(self, z, extent):
        """--anomaly_z_sigma > 0: the Z-maps [..., *extent] blurred plane by plane (H, W: one launch) or volume by volume (D, H, W: the
        in-plane launch and the depth pass), else ``z`` itself."""
        if not self.s.z_sigma > 0:
            return z
        if self._taps is None:
            self._taps = torch.from_numpy(ops.gaussian_taps(self.s.z_sigma).astype(np.float32)).to(self.device)
        blur = ops.map_blur if len(extent) == 2 else ops.map_blur3d
        return blur(z.reshape((-1,) + tuple(extent)), taps=self._taps)

    def zero_mask(self, B: int, P: int):
        """uint8 [B, P] of zeros (the in set, an out set without masks, the validation set: every pixel is a negative)."""
        if self._no_mask is None or self._no_mask.shape[0] < B or self._no_mask.shape[1] != P:
            self._no_mask = torch.zeros((B, P), dtype=torch.uint8, device=self.device)
        return self._no_mask[:B]

    @functools.cached_property
    def thresholds(self):
        return torch.tensor(self.voxel.thresholds if self.voxel else self.s.px_thresholds, dtype=torch.float32, device=self.device)

    @functools.cached_property
    def seg_thresholds(self):
        return torch.tensor(self.voxel.thresholds if self.voxel and self.voxel.segment else self.s.sg_thresholds, dtype=torch.float32,
                            device=self.device)

    @functools.cached_property
    def seg_bit_weights(self):
        return torch.tensor([1 << b for b in range(SEG_BITS)], dtype=torch.int32, device=self.device)

    def tables(self, t_values, shape, fresh=False):
        """(mean, inv_std) [n_t, 2, *extent] on the device: the statistics of this process's validation pass (``fresh``: it just
        ended), else those of ood/map_stats.npz (--run_val 0), which must have been written for these t-starts and this extent."""
        if fresh or self._tables is None or self._tables[0] != list(t_values) or self._tables[1].shape != shape:
            extent = tuple(shape[2:])
            if self.last_map_stats is not None:
                stats, t_val = self.last_map_stats
                if [int(t) for t in t_val] != [int(t) for t in t_values] or tuple(stats.tables()[1].shape[2:]) != extent:
                    raise ValueError(f"--anomaly_z_maps 1: the validation pass gave statistics for t = {t_val} and maps of "
                                     f"{tuple(stats.tables()[1].shape[2:])}, this set has t = {list(t_values)} and {extent}")
            else:
                stats = zmaps.MapStats.load(self.out_dir / zmaps.STATS_FILE, t_values, extent)
            mean, inv_std = stats.finalize(self.s.z_std_floor)
            self._tables = ([int(t) for t in t_values], torch.from_numpy(mean).to(self.device), torch.from_numpy(inv_std).to(self.device))
        return self._tables[1:]

    def calibration(self, t_values, fresh=False):
        """The file's dict and "thr", the thresholds [2, F] on the device: of this process's validation pass (``fresh``: it just ended),
        else of ood/calibration.npz (--run_val 0), written with this run's t-starts, range, bins, smoothing, floor and target rates."""
        s, cal = self.s, self.last_calibration
        if fresh or self._cal is None or [int(t) for t in self._cal["t"]] != [int(t) for t in t_values]:
            flag, _, lo, hi, bins, fprs, _ = self.cal_grid
            if cal is not None and [int(t) for t in cal["t"]] != [int(t) for t in t_values]:
                raise ValueError(f"{flag}: the validation pass calibrated on t = {[int(t) for t in cal['t']]}"
                                 f", this set has t = {list(t_values)}")
            if cal is None:
                try:
                    cal = pixel_metrics.load_calibration(self.out_dir / pixel_metrics.CALIBRATION_FILE, t_values, lo, hi,
                                                         bins, s.z_sigma, s.z_std_floor, fprs)
                except (ValueError, FileNotFoundError) as e:  # (the file and its checks are shared; the message names the flag in force)
                    raise type(e)(str(e).replace(pixel_metrics.CALIBRATE_FLAG, flag)) from None
            self._cal = dict(cal, thr=torch.from_numpy(np.ascontiguousarray(cal["thresholds"], dtype=np.float32)).to(self.device))
        return self._cal


class MapPass:
    """One ``get_scores`` call's share of the stack.  Validation pass: the running statistics and, for the calibration, the counted
    rows on the device.  Any other pass: the histogram and overlap tables on the device and, per batch, the maps, Z-maps and
    integer rows on the host.  The batch's mask, labels and regions are arguments between the steps, never state."""
    def __init__(self, pipeline: MapPipeline, dataset_name: str, loader, t_values):
        self.p, self.loader, self.t_values = pipeline, loader, [int(t) for t in t_values]
        s = pipeline.s
        self.stats = zmaps.MapStats() if s.want_z_maps and dataset_name == "val" else None
        self.z_maps = s.want_z_maps and dataset_name != "val"  # (the validation set gets no Z-maps)
        self.counting = s.pixel_metrics and dataset_name != "val"
        self.voxel_counting = pipeline.voxel is not None and pipeline.voxel.metrics and dataset_name != "val"  # --voxel_metrics 1 (voxel_passes.py)
        self.voxel_segmenting = pipeline.voxel is not None and pipeline.voxel.segment and dataset_name != "val"  # --voxel_segment 1
        self.segmenting = s.pixel_segment and dataset_name != "val"  # (the validation pass does nothing for it)
        self.seg_rows, self.seg_plane = [], None  # fp32 host rows [B, packed segmentation + integer row], one entry per batch; (H, W)
        self.cal_rows = None  # --pixel_calibrate_fpr, validation: the counted rows' per-t maps, one device tensor per batch
        if pipeline.calibrating and self.stats is not None:  # they stay on the device for the leave-one-out pass: refuse first
            dims = 3 if s.volume else 2
            shape = tuple(loader.images[0].shape) if len(loader.names) else (0,) * dims
            flag, budget_flag, *_, budget = pipeline.cal_grid
            pixel_metrics.check_budget(len(loader.names), len(self.t_values), *shape[-dims:], budget, flags=(flag, budget_flag))
            self.cal_rows = []
        self.hist = self.overlap = None  # int64 [2, 2, nbins + 1] / float64 [2, nbins + 1], on the device
        self.maps, self.zmaps, self.rows = [], [], []  # host tensors, one entry per batch
        self.rows_skipped = 0  # validation images left out of the statistics (a non-finite score)

    def add_batch(self, scores, maps, per_t_maps, mask=None):
        """One batch after the numeric guard ([.., H, W] below: [.., D, H, W] for volumes): ``maps`` [B, 2, H, W] goes to the host.  ``per_t_maps`` [B, n_t, 2, H, W], validation:
        the rows whose scores are all finite go into the running statistics.  Any other pass: the batch's Z-maps and, with --pixel_metrics
        1, their counts against ``mask`` (uint8 [B, 1, H, W]; None: all zero) reach the host in ONE copy, the Z-maps as their int32 bits."""
        if maps is not None:
            self.maps.append(maps.cpu())
        if per_t_maps is None:
            return
        p = self.p
        B, n_t = per_t_maps.shape[:2]
        extent = tuple(per_t_maps.shape[3:])
        P1 = 2 * int(np.prod(extent, dtype=np.int64))
        if self.stats is not None:
            finite = torch.isfinite(scores).all(dim=2).all(dim=1)
            keep = int(finite.sum())
            counted = per_t_maps if keep == B else per_t_maps[finite].contiguous() if keep else None
            if counted is not None:
                self.stats.update(counted)
                if self.cal_rows is not None:  # the very tensor the statistics received
                    self.cal_rows.append(counted)
            self.rows_skipped += B - keep
            return
        mean, inv_std = p.tables(self.t_values, per_t_maps.shape[1:])
        z = ops.map_zscore(per_t_maps.reshape(B, n_t, P1), mean.reshape(n_t, P1), inv_std.reshape(n_t, P1))
        z = p.smooth(z, extent)
        if self.voxel_counting or self.voxel_segmenting:  # volumes: the Z-maps go to the host as they do without the flags, the integer rows in copies of their own
            voxel_passes.check_budget(B, n_t, extent, p.voxel, p.s.volume_budget)
            truth = None
            if self.voxel_counting:
                parts, mask_voxels, truth = voxel_passes.count_batch(self, z.reshape(B, 2, P1 // 2), mask, extent, n_t)
                self.rows.append(p.layout.pack(dict(p.device_layout.unpack(p.device_layout.pack(parts).cpu()), mask_pixels=mask_voxels)))
            if self.voxel_segmenting:
                voxel_passes.segment_batch(self, z.reshape(B, 2, P1 // 2), mask if self.voxel_counting else None, extent, truth)
            self.zmaps.append(z.reshape((B, 2) + extent).cpu())
            return
        if not (self.segmenting or self.counting):
            self.zmaps.append(z.reshape((B, 2) + extent).cpu())
            return
        H, W = extent  # (the steps against masks are 2-D only: refused with the volume flags)
        if self.segmenting:
            self.segment_batch(z.reshape(B, 2, H * W), mask if self.counting else None, H, W)
        if not self.counting:
            self.zmaps.append(z.reshape(B, 2, H, W).cpu())
            return
        parts, mask_pixels = self.count_batch(z.reshape(B, 2, H * W), mask, H, W)
        both = p.device_layout.pack(parts, lead=[z.reshape(B, 2 * H * W).view(torch.int32)]).cpu()
        self.zmaps.append(both[:, :2 * H * W].contiguous().view(torch.float32).reshape(B, 2, H, W))
        self.rows.append(p.layout.pack(dict(p.device_layout.unpack(both[:, 2 * H * W:]), mask_pixels=mask_pixels)))

    def device_mask(self, mask, B: int, P: int, flag: str = "--pixel_metrics 1"):
        """(uint8 [B, P] on the device, the masks' pixel counts [B] on the host) of a batch's ``mask`` (None: all zero)."""
        if mask is None:
            return self.p.zero_mask(B, P), torch.zeros(B, dtype=torch.int64)
        if mask.shape[0] != B or mask.numel() != B * P:
            raise ValueError(f"{flag}: masks of {tuple(mask.shape)} for maps of {B} x {P} pixels")
        return mask.reshape(B, P).to(device=self.p.device, dtype=torch.uint8).contiguous(), (mask.reshape(B, P) != 0).sum(dim=1).cpu()

    def segment_batch(self, z, mask, H: int, W: int):
        """--pixel_segment 1: ``z`` [B, 2, H W] on the device, the final Z-maps.  One median launch over the 2 B planes (none at
        --pixel_median 1), one labelling of the mask, per channel one ``map_segment`` call at the fixed thresholds and, with
        --pixel_calibrate_fpr, one at the channel's calibrated ones.  The segmentations, 16 pixels to an fp32, and the integer row
        behind them reach the host in ONE copy."""
        p, s = self.p, self.p.s
        B, _, P = z.shape
        check_plane(pixel_metrics.SEGMENT_FLAG, H, W)
        m, mask_pixels = self.device_mask(mask, B, P, pixel_metrics.SEGMENT_FLAG)
        m = m.reshape(B, H, W)
        planes = z.reshape(2 * B, H, W)
        if s.sg_median > 1:
            planes = ops.map_median(planes.contiguous(), s.sg_median)
        planes = planes.reshape(B, 2, H, W)
        labels, regions = ops.map_label(m, s.sg_connectivity)
        cal = p.calibration(self.t_values)["thr"] if s.px_calibrate else None
        per_channel = []
        for c in range(2):
            zc = planes[:, c].contiguous()
            got = [ops.map_segment(zc, m, labels, regions, p.seg_thresholds, s.sg_min_component, s.sg_connectivity)]
            if cal is not None:
                got.append(ops.map_segment(zc, m, labels, regions, cal[c].contiguous(), s.sg_min_component, s.sg_connectivity))
            per_channel.append([torch.cat(kind, dim=1) for kind in zip(*got)])  # (seg, pixels, components, removed), each [B, T, ...]
        seg, pixels, components, removed = (torch.stack(kind, dim=1) for kind in zip(*per_channel))  # [B, 2, T, ...]
        bits = seg.reshape(B, -1)
        pad = -bits.shape[1] % SEG_BITS
        if pad:
            bits = torch.nn.functional.pad(bits, (0, pad))
        packed = (bits.reshape(B, -1, SEG_BITS).to(torch.int32) * p.seg_bit_weights).sum(dim=2)
        device_layout = p.seg_layout.without("mask_pixels")
        ints = device_layout.pack({"pixels": pixels, "components": components, "removed": removed, "regions": regions[:, None]})
        row = torch.cat([packed, ints], dim=1).to(torch.float32).cpu()  # (every entry is an integer below 2^24: exact)
        self.seg_plane = (H, W)
        self.seg_rows.append(torch.cat([row, mask_pixels.to(torch.float32)[:, None]], dim=1))

    def count_batch(self, z, mask, H: int, W: int):
        """--pixel_metrics 1: ``z`` [B, 2, H W] on the device against ``mask``; the pixel, region and calibrated steps in the order
        the tables are pinned to.  Returns (the device's columns of the row by name, the masks' pixel counts [B] on the host)."""
        s = self.p.s
        B, _, P = z.shape
        if P >= 1 << 31:
            raise ValueError(f"--pixel_metrics 1: maps of {P} pixels do not fit the 32-bit counts")
        m, mask_pixels = self.device_mask(mask, B, P)
        if self.hist is None:
            self.hist = torch.zeros((2, 2, s.px_bins + 1), dtype=torch.int64, device=self.p.device)
        counts = []
        for c in range(2):  # the pixel step: one histogram launch into the pass's [2, 2, nbins + 1] table and one counts launch
            zc = z[:, c].contiguous()
            ops.map_mask_hist(zc, m, s.px_lo, s.px_hi, s.px_bins, total=self.hist[c])
            counts.append(ops.map_mask_counts(zc, m, self.p.thresholds))
        parts, labels = {"counts": torch.stack(counts, dim=1)}, None
        if s.pixel_regions:
            parts["components"], labels, parts["regions"] = self.region_step(z, m, H, W)
        if s.px_calibrate:
            parts["calibrated"] = self.calibrated_step(z, m, H, W, labels, parts.get("regions"))
        return parts, mask_pixels

    def region_step(self, z, m, H: int, W: int):
        """--pixel_regions 1: the mask's components are labelled once; per channel one overlap call into the pass's [2, nbins + 1] float64
        table and one component-counts call.  Returns (components int32 [B, 2, K, 3], labels, regions int32 [B]); an all-zero mask: 0."""
        s = self.p.s
        B, _, P = z.shape
        check_plane("--pixel_regions 1", H, W)
        m = m.reshape(B, H, W)
        labels, regions = ops.map_label(m, s.px_connectivity)
        if self.overlap is None:
            self.overlap = torch.zeros((2, s.px_bins + 1), dtype=torch.float64, device=self.p.device)
        components = []
        for c in range(2):
            zc = z[:, c].contiguous().reshape(B, H, W)
            ops.map_region_overlap(zc, labels, regions, s.px_lo, s.px_hi, s.px_bins, total=self.overlap[c])
            components.append(ops.map_component_counts(zc, m, labels, regions, self.p.thresholds, s.px_connectivity))
        return torch.stack(components, dim=1), labels, regions

    def calibrated_step(self, z, m, H: int, W: int, labels=None, regions=None):
        """--pixel_calibrate_fpr: per channel one more counts call at its calibrated thresholds (with regions: and one more
        component-counts call).  Returns int32 [B, 2 F 3] (with regions [B, 2 F 3 + 2 F 3]) on the device."""
        B = z.shape[0]
        thr = self.p.calibration(self.t_values)["thr"]
        counts = [ops.map_mask_counts(z[:, c].contiguous(), m, thr[c]) for c in range(2)]
        parts = [torch.stack(counts, dim=1).reshape(B, -1)]
        if self.p.s.pixel_regions:
            comps = [ops.map_component_counts(z[:, c].contiguous().reshape(B, H, W), m.reshape(B, H, W), labels, regions, thr[c],
                                              self.p.s.px_connectivity) for c in range(2)]
            parts.append(torch.stack(comps, dim=1).reshape(B, -1))
        return torch.cat(parts, dim=1)

    def finish_validation(self):
        """--anomaly_z_maps 1, after the validation pass: with N ranks ONE all_gather of (n, mean, m2) and the same float64 merge
        on every rank, so that every rank finalises the same tables; then the calibration."""
        if self.stats is None:
            return
        p = self.p
        n, mean, m2 = self.stats.tables()
        if p.ddp:
            if hasattr(self.loader, "all_names") and len(self.loader.all_names) < p.world:
                raise ValueError(f"--anomaly_z_maps 1: {len(self.loader.all_names)} images over {p.world} ranks leave a rank "
                                 f"without an image, and the maps' extent comes from the images")
            if mean is None:
                raise ValueError("--anomaly_z_maps 1: this rank counted no validation image: no statistics to gather")
            if n >= 1 << 24:
                raise ValueError(f"--anomaly_z_maps 1: a row count of {n} is not exact in the fp32 payload")
            payload = host_if_gloo(torch.cat([torch.tensor([float(n)], dtype=torch.float32, device=p.device),
                                              self.stats.mean.reshape(-1), self.stats.m2.reshape(-1)])[None])  # [1, 1 + 2 P]
            out = torch.empty((p.world, payload.numel()), dtype=torch.float32, device=payload.device)
            dist.all_gather_into_tensor(out, payload)
            out = out.cpu().double().numpy()
            P = mean.size
            n, mean, m2 = zmaps.MapStats.merge([(int(r[0]), r[1:1 + P].reshape(mean.shape), r[1 + P:].reshape(mean.shape)) for r in out])
        if mean is None:
            raise ValueError("--anomaly_z_maps 1: the validation pass counted no image: no statistics")
        stats = zmaps.MapStats.from_tables(n, mean, m2, self.t_values)
        p.last_map_stats = (stats, self.t_values)
        p.tables(self.t_values, mean.shape, fresh=True)  # (n < 2 or a channel that never varies: refused here, on every rank alike)
        if p.calibrating:
            self._calibrate(stats)

    def _calibrate(self, stats):
        """Every rank uploads the merged mean and M2 (float64 rounded once to fp32) and the floor, bins the leave-one-out Z-maps of the
        rows it kept (smoothed like every other set's) per channel; ONE all_reduce of the int64 table: the same thresholds everywhere."""
        p, s = self.p, self.p.s
        flag, _, lo, hi, bins, fprs, _ = p.cal_grid
        rows, self.cal_rows = self.cal_rows, None
        n, mean, m2 = stats.tables()
        if n < 3:
            raise ValueError(f"{flag}: leaving one of {n} validation image(s) out leaves fewer than 2: at least 3 are needed")
        mean_d = torch.from_numpy(mean.astype(np.float32)).to(p.device)
        m2_d = torch.from_numpy(m2.astype(np.float32)).to(p.device)
        floor_d = torch.from_numpy(stats.floor(s.z_std_floor)).to(p.device)
        hist = torch.zeros((2, 2, bins + 1), dtype=torch.int64, device=p.device)  # [channel, class, bin]: class 1 stays 0
        kept = []
        for per_t in rows:
            extent = tuple(per_t.shape[3:])
            P = int(np.prod(extent, dtype=np.int64))
            # planes: the batch in one call.  Volumes: slices of rows whose Z-maps, the blur's intermediate and result and one channel's
            # copy (3.5 x 2 D H W fp32 a row) stay inside --anomaly_volume_budget_gb, one row at the least
            step = per_t.shape[0] if len(extent) == 2 else max(1, int(s.volume_budget // (28 * P)))
            for r0 in range(0, per_t.shape[0], step):
                part = per_t[r0:r0 + step]
                B = part.shape[0]
                z = p.smooth(ops.map_zscore_loo(part, mean_d, m2_d, n, floor_d), extent).reshape(B, 2, P)
                no_mask = p.zero_mask(B, P)
                for c in range(2):
                    ops.map_mask_hist(z[:, c].contiguous(), no_mask, lo, hi, bins, total=hist[c])
                if s.keep_calibration_rows:
                    kept.append((part.cpu(), z.reshape((B, 2) + extent).cpu()))
        hist = hist[:, 0].contiguous()
        if p.ddp:
            hist = host_if_gloo(hist)
            dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        if s.keep_calibration_rows:
            p.calibration_rows = torch.cat([k[0] for k in kept]).numpy() if kept else None
            p.calibration_zmaps = torch.cat([k[1] for k in kept]).numpy() if kept else None
        try:
            p.last_calibration = pixel_metrics.calibration_tables(hist.cpu().numpy(), self.t_values, n, fprs, lo, hi, bins, s.z_sigma, s.z_std_floor)
        except ValueError as e:  # (--pixel_range is shared; the message leads with the flag in force)
            raise ValueError(str(e).replace(pixel_metrics.CALIBRATE_FLAG, flag)) from None
        p.calibration(self.t_values, fresh=True)

    def collect(self, results, local_ids, gathered_ids, name_of) -> dict:
        """The pass's collectives: one ``gather_rows`` per kind of per-image rows, one all_reduce per table.  Returns {file name: its
        arrays, or a callable that saves to a path} on rank 0, {} elsewhere.  ``local_ids`` / ``gathered_ids``: this / every rank's."""
        p, s = self.p, self.p.s
        ids, files = (local_ids, gathered_ids, name_of), {}
        t = np.asarray(self.t_values, dtype=np.int64)
        if s.want_maps:
            got = self._gather("--anomaly_volume_maps 1" if s.volume_maps else "--anomaly_maps 1", self.maps, results, *ids)
            if got is not None:
                files[MAPS] = {"filename": np.asarray(got[0]), "t": t, "lpips_map": np.ascontiguousarray(got[1][:, 0]),
                               "mse_map": np.ascontiguousarray(got[1][:, 1])}
        if self.stats is not None and p.rank == 0:  # t [n_t], n, mean / std fp32 [n_t, 2, H, W] (the un-floored std), channels, rel_floor
            files[zmaps.STATS_FILE] = lambda path, stats=p.last_map_stats[0]: stats.save(path, self.t_values, s.z_std_floor)
            if p.calibrating:
                files[pixel_metrics.CALIBRATION_FILE] = p.last_calibration
        if self.z_maps:
            got = self._gather(zmaps.VOLUME_FLAG if s.volume_z_maps else zmaps.FLAG, self.zmaps, results, *ids)
            if got is not None:
                files[ZMAPS] = {"filename": np.asarray(got[0]), "t": t, "z_lpips_map": np.ascontiguousarray(got[1][:, 0]),
                                "z_mse_map": np.ascontiguousarray(got[1][:, 1]), "sigma": np.float64(s.z_sigma),
                                "rel_floor": np.float64(s.z_std_floor)}
        if self.segmenting:
            self._collect_segments(files, t, results, *ids)
        if self.voxel_segmenting:
            voxel_passes.collect_segments(self, files, t, results, *ids)
        if self.voxel_counting:
            return voxel_passes.collect(self, files, t, results, *ids)
        if not self.counting:
            return files
        # --pixel_metrics 1: the histogram (and the overlap table) summed over the ranks, ONE all_reduce each, and every rank's integer
        # rows in the CSV's order (the gather's payload is fp32, so a count must stay below 2^24)
        hist, overlap = self.hist, self.overlap
        if p.ddp:
            pixels = int(self.zmaps[0].shape[2] * self.zmaps[0].shape[3])
            if pixels >= 1 << 24:
                raise ValueError(f"--pixel_metrics 1: a count of up to {pixels} pixels is not exact in the fp32 payload of the "
                                 f"gather (H W must stay below 2^24 with more than one rank)")
            hist = host_if_gloo(hist)
            dist.all_reduce(hist, op=dist.ReduceOp.SUM)
            if s.pixel_regions:
                overlap = host_if_gloo(overlap)
                dist.all_reduce(overlap, op=dist.ReduceOp.SUM)
        got = self._gather("--pixel_metrics 1", self.rows, results, *ids)
        if got is None:
            return files
        stems, row = np.asarray(got[0]), p.layout.unpack(np.rint(got[1]).astype(np.int64))
        head = {"filename": stems, "t": t, "channels": np.asarray(zmaps.CHANNELS), "lo": np.float64(s.px_lo), "hi": np.float64(s.px_hi),
                "nbins": np.int64(s.px_bins)}
        thresholds = np.asarray(s.px_thresholds, dtype=np.float32)
        if s.px_calibrate:  # counts int32 [N, 2, F, 3] = (TP, FP, FN), with --pixel_regions 1 components = (hit, pred, false_pred)
            cal, at = p.calibration(self.t_values), row["calibrated"].astype(np.int32)
            files[CALIBRATED] = {"filename": stems, "fpr": np.asarray(cal["fpr"], dtype=np.float64),
                                 "thresholds": np.asarray(cal["thresholds"], dtype=np.float32), "counts": at[:, 0]}
            if s.pixel_regions:
                files[CALIBRATED]["components"] = at[:, 1]
        if s.pixel_regions:  # regions int32 [N], overlap float64 [2, nbins + 1], components int32 [N, 2, K, 3] = (hit, pred, false_pred)
            files[REGIONS] = {**head, "connectivity": np.int64(s.px_connectivity), "regions": row["regions"].astype(np.int32),
                              "overlap": overlap.cpu().numpy().astype(np.float64), "thresholds": thresholds,
                              "components": row["components"].astype(np.int32), "sigma": np.float64(s.z_sigma)}
        # hist int64 [2, 2, nbins + 1], thresholds [K], counts int32 [N, 2, K, 3] = (TP, FP, FN), mask_pixels [N]
        files[PIXELS] = {**head, "hist": hist.cpu().numpy().astype(np.int64), "thresholds": thresholds,
                         "counts": row["counts"].astype(np.int32), "mask_pixels": row["mask_pixels"], "sigma": np.float64(s.z_sigma)}
        return files

    def _collect_segments(self, files, t, results, *ids):
        """--pixel_segment 1: ONE gather of the rows (packed segmentation, integers); the file is saved compressed."""
        p, s = self.p, self.p.s
        got = self._gather(pixel_metrics.SEGMENT_FLAG, self.seg_rows, results, *ids)
        if got is None:
            return
        H, W = self.seg_plane
        T, K = p.seg_T, len(s.sg_thresholds)
        words = -(-2 * T * H * W // SEG_BITS)
        row = p.seg_layout.unpack(np.rint(got[1][:, words:]).astype(np.int64))
        thresholds = np.repeat(np.asarray(s.sg_thresholds, dtype=np.float32)[None], 2, axis=0)
        fpr = np.full(K, np.nan, dtype=np.float64)
        if s.px_calibrate:
            cal = p.calibration(self.t_values)
            thresholds = np.concatenate([thresholds, np.asarray(cal["thresholds"], dtype=np.float32)], axis=1)
            fpr = np.concatenate([fpr, np.asarray(cal["fpr"], dtype=np.float64)])
        arrays = {"filename": np.asarray(got[0]), "t": t, "channels": np.asarray(zmaps.CHANNELS), "thresholds": thresholds, "fpr": fpr,
                  "median": np.int64(s.sg_median), "min_component": np.int64(s.sg_min_component),
                  "connectivity": np.int64(s.sg_connectivity), "sigma": np.float64(s.z_sigma),
                  "segmentation": unpack_segmentation(got[1][:, :words], (2, T, H, W)), "pixels": row["pixels"].astype(np.int32),
                  "components": row["components"].astype(np.int32), "removed": row["removed"].astype(np.int32),
                  "mask_pixels": row["mask_pixels"], "regions": row["regions"].astype(np.int32)}
        files[SEGMENTS] = lambda path, arrays=arrays: np.savez_compressed(path, **arrays)

    def _gather(self, flag, batches, results, local_ids, gathered_ids, name_of):
        """(filenames, rows) on rank 0, None elsewhere: every rank's per-image rows (``batches``: this rank's) in the CSV's order."""
        p = self.p
        n_total = len(self.loader.all_names) if hasattr(self.loader, "all_names") else None
        if p.ddp and n_total is not None and n_total < p.world:  # (every rank sees the same list and raises alike)
            raise ValueError(f"{flag}: {n_total} images over {p.world} ranks leave a rank without "
                             f"an image, and the maps' extent comes from the images")
        if not batches:
            raise ValueError(f"{flag}: this rank scored no batch (--drop_last on a short shard?): no maps to gather")
        rows = torch.cat(list(batches), dim=0)
        if p.ddp:
            n_max = -(-n_total // p.world) if n_total is not None else None
            gids, rows, _ = gather_rows(local_ids.to(p.device), rows.to(p.device), n_max)
            gathered_ids, rows = gids.cpu().tolist(), rows.cpu()
        if p.rank != 0:
            return None
        stems, picks = map_rows_in_csv_order(results, gathered_ids, name_of)
        return stems, rows[torch.as_tensor(picks, dtype=torch.long)].numpy()
