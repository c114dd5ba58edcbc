"""``Reconstruct``: the multi-t reconstruction trainer with the reference's surface.

Mirrors /root/reference/src/trainers/base.py:19-164 (setup half: device / process group,
stage-1 model, ``small`` / ``big`` UNet constructor arguments, schedule parameters, checkpoint
load with the reference's exceptions) and /root/reference/src/trainers/reconstruct.py:29-330
(``get_scores`` hot loops, CSV files, ``_vflip`` / ``_hflip`` out-set variants).

What is MI355X-native here (and differs in mechanism, not in results, from the reference):
  * the UNet forward is one native call (ddpm_unet_forward), the PLMS update / add_noise /
    clamp+MSE are single fused HIP kernels; there is no autocast (fp32 throughout, Q5);
  * timesteps live on the device (one cached int64 tensor per step value, Q18) and scores
    come back with ONE device->host copy per batch instead of 2*B ``.item()`` syncs per t;
  * noise is an explicit, host-generated, per-image seeded input (``--seed`` finally has an
    effect, Q2), so results do not depend on batch composition or rank count;
  * images are sharded round-robin over ranks and scores return through a single RCCL
    all_gather of a dense [ceil(n / world), n_t * 2 + 1] fp32 tensor per rank (ids ride in column 0; the
    shard capacity is static, so no size exchange precedes it) instead of all_gather_object of pickled
    dict rows; only rank 0 writes the CSV (Q6).
"""

from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import pandas as pd
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib, ops, pixel_metrics, zmaps
from .data import get_data_loader
from .perceptual import PerceptualLoss
from .scheduler import DDPMScheduler, PNDMScheduler
from .unet import DiffusionModelUNet
from .vqvae import VQVAE, PassthroughVQVAE

MODEL_CONFIGS = {  # /root/reference/src/trainers/base.py:65-86
    "small": dict(num_channels=(128, 256, 256), attention_levels=(False, False, True), num_res_blocks=1,
                  num_head_channels=256),
    "big": dict(num_channels=(256, 512, 768), attention_levels=(True, True, True), num_res_blocks=2,
                num_head_channels=256),
}


def image_noise(seed: int, index: int, t_start: int, shape) -> torch.Tensor:
    """The noise input of one (image, t_start) reconstruction: host fp32 N(0, 1), a pure
    function of (seed, global image index, t_start)."""
    g = torch.Generator().manual_seed((int(seed) * 1_000_003 + int(index)) * 1_009 + int(t_start))
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32)


def batch_noise(seed: int, indices, t_start: int, shape) -> torch.Tensor:
    return torch.stack([image_noise(seed, i, t_start, shape[1:]) for i in indices])


SIMPLEX_SEED_RANGE = 10**10  # Simplex_CLASS.newSeed draws np.random.randint(-10**10, 10**10)
_U64 = (1 << 64) - 1


def _splitmix64(x: np.ndarray) -> np.ndarray:
    """SplitMix64's finaliser over a uint64 array (wrapping arithmetic)."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def simplex_seeds(seed: int, indices, t_start: int, channels: int) -> torch.Tensor:
    """The permutation seeds of --simplex_noise: int64 [len(indices), channels] in the reference's range [-10^10, 10^10), a pure
    function of (seed, global image index, t_start, channel) -- like image_noise, independent of batch composition and rank
    count.  (The reference draws them from numpy's global generator in the order its loops meet them.)"""
    idx = np.asarray([int(i) & _U64 for i in indices], dtype=np.uint64)
    h = _splitmix64(np.full(idx.shape, int(seed) & _U64, dtype=np.uint64))
    h = _splitmix64(h ^ idx)
    h = _splitmix64(h ^ np.uint64(int(t_start) & _U64))
    h = _splitmix64(h[:, None] ^ np.arange(channels, dtype=np.uint64)[None, :])
    return torch.from_numpy((h % np.uint64(2 * SIMPLEX_SEED_RANGE)).astype(np.int64) - SIMPLEX_SEED_RANGE)


def snr_shift_tables(scheduler, snr_shift: float) -> None:
    """/root/reference/src/trainers/reconstruct.py:106-117 (same code at base.py:104-116)."""
    snr = scheduler.alphas_cumprod / (1 - scheduler.alphas_cumprod)
    target_snr = snr * snr_shift
    new_alphas_cumprod = 1 / (torch.pow(target_snr, -1) + 1)
    new_alphas = torch.zeros_like(new_alphas_cumprod)
    new_alphas[0] = new_alphas_cumprod[0]
    for i in range(1, len(new_alphas)):
        new_alphas[i] = new_alphas_cumprod[i] / new_alphas_cumprod[i - 1]
    scheduler.betas = 1 - new_alphas
    scheduler.alphas = new_alphas
    scheduler.alphas_cumprod = new_alphas_cumprod


def gather_scores(ids: torch.Tensor, scores: torch.Tensor, n_max: int = None):
    """ONE all_gather of dense per-image scores (RCCL over xGMI; gloo in the CPU tests).

    ids: int32 [n_local] global image indices; scores: fp32 [n_local, n_t, 2]; n_max: the static shard capacity
    ceil(n_images / world) -- every rank can compute it from the id list, so no size exchange is needed.
    Returns (ids, scores, counts) concatenated rank-major on every rank (the reference's all_gather_object
    semantics, reconstruct.py:238-242, in 2 MB instead of 30 MB of pickles).  Short shards are padded with
    id = -1; the padding is dropped after the gather and ``counts`` (rows per rank) is read off the ids."""
    if not dist.is_initialized():
        return ids, scores, [int(ids.shape[0])]
    world = dist.get_world_size()  # a 1-rank group still goes through the collective (same code path as N ranks)
    if n_max is None:
        n_max = int(ids.shape[0]) if world == 1 else None
    if n_max is None or ids.shape[0] > n_max:
        raise ValueError(f"gather_scores: shard of {ids.shape[0]} rows does not fit the static capacity {n_max}")
    n_t = scores.shape[1]
    # ids travel inside the same fp32 payload (exact for ids < 2^24): one collective, not two
    if ids.numel() and int(ids.max()) >= 1 << 24:
        raise ValueError(f"gather_scores: image id {int(ids.max())} is not exact in the fp32 payload (ids must be < 2^24)")
    payload = torch.full((n_max, n_t * 2 + 1), -1.0, dtype=torch.float32, device=scores.device)
    payload[: ids.shape[0], 0] = ids.to(torch.float32)
    payload[: ids.shape[0], 1:] = scores.reshape(ids.shape[0], n_t * 2)  # (an empty shard has 0 rows)
    dev = scores.device
    if dist.get_backend() == "gloo" and payload.is_cuda:  # test hook (2 ranks on one GPU): gloo moves host memory
        payload = payload.cpu()
    out = torch.empty((world * n_max, n_t * 2 + 1), dtype=torch.float32, device=payload.device)
    dist.all_gather_into_tensor(out, payload)
    out = out.to(dev)
    valid = out[:, 0] >= 0
    counts = valid.reshape(world, n_max).sum(dim=1).tolist()
    out = out[valid]
    return out[:, 0].to(torch.int32), out[:, 1:].reshape(-1, n_t, 2), [int(c) for c in counts]


def gather_rows(ids: torch.Tensor, rows: torch.Tensor, n_max: int = None):
    """``gather_scores`` for rows of any trailing shape (the anomaly maps: fp32 [n_local, 2, H, W]): ONE all_gather of a dense
    [n_max, 1 + row size] fp32 payload per rank, ids in column 0, short shards padded with id = -1 and the padding dropped
    after the gather.  Returns (ids, rows, counts) concatenated rank-major on every rank."""
    if not dist.is_initialized():
        return ids, rows, [int(ids.shape[0])]
    world = dist.get_world_size()
    if n_max is None:
        n_max = int(ids.shape[0]) if world == 1 else None
    if n_max is None or ids.shape[0] > n_max:
        raise ValueError(f"gather_rows: shard of {ids.shape[0]} rows does not fit the static capacity {n_max}")
    if rows.shape[0] != ids.shape[0]:
        raise ValueError(f"gather_rows: {rows.shape[0]} rows for {ids.shape[0]} ids")
    if ids.numel() and int(ids.max()) >= 1 << 24:
        raise ValueError(f"gather_rows: image id {int(ids.max())} is not exact in the fp32 payload (ids must be < 2^24)")
    trailing = tuple(rows.shape[1:])
    width = 1
    for d in trailing:
        width *= int(d)
    payload = torch.full((n_max, width + 1), -1.0, dtype=torch.float32, device=rows.device)
    payload[: ids.shape[0], 0] = ids.to(device=rows.device, dtype=torch.float32)
    payload[: ids.shape[0], 1:] = rows.reshape(ids.shape[0], width)
    dev = rows.device
    if dist.get_backend() == "gloo" and payload.is_cuda:  # (the test hook of gather_scores)
        payload = payload.cpu()
    out = torch.empty((world * n_max, width + 1), dtype=torch.float32, device=payload.device)
    dist.all_gather_into_tensor(out, payload)
    out = out.to(dev)
    valid = out[:, 0] >= 0
    counts = valid.reshape(world, n_max).sum(dim=1).tolist()
    out = out[valid]
    return out[:, 0].to(torch.int32), out[:, 1:].reshape((-1,) + trailing), [int(c) for c in counts]


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


def sub_batch(batch: dict, keep):
    """The loader batch restricted to the items `keep` (the numeric guard re-runs only the images that overflowed)."""
    img = batch["image"]
    sel = torch.as_tensor(keep, dtype=torch.long)
    image = img[sel.to(img.device)] if torch.is_tensor(img) else torch.stack([img[int(i)] for i in keep])
    names = batch["image_meta_dict"]["filename_or_obj"]
    return {"image": image, "index": [batch["index"][i] for i in keep],
            "image_meta_dict": {"filename_or_obj": [names[i] for i in keep]}}


def rows_from_scores(ids, scores, counts, t_values, name_of, batch_size: int, dataset_name: str):
    """Dense gathered scores -> the reference's row dicts, in the reference's order: rank-major
    (all_gather_object, reconstruct.py:238-242), and inside a rank per batch, per t_start, per image
    (reconstruct.py:128,192-204)."""
    ids = [int(i) for i in ids]
    results = []
    start = 0
    for n_rank in counts:
        for s in range(start, start + n_rank, batch_size):
            e = min(start + n_rank, s + batch_size)
            for j, t in enumerate(t_values):
                for b in range(s, e):
                    filename = name_of.get(ids[b], str(ids[b]))
                    stem = Path(filename).stem.replace(".nii", "").replace(".gz", "")
                    results.append({"filename": stem, "type": dataset_name, "t": int(t),
                                    "perceptual_difference": float(scores[b, j, 0]), "mse": float(scores[b, j, 1])})
        start += n_rank
    return results


class BaseTrainer:
    def __init__(self, args):
        # every rank reports a missing device / library BEFORE the non-zero ranks' output is silenced
        if not torch.cuda.is_available():
            raise RuntimeError("No ROCm device visible: the HIP reconstruction path has no CPU fallback "
                               "(the CPU oracle under oracle/ is test infrastructure only)")
        _lib.load()  # fail before any work if the native library is missing
        # initialise the process group if launched with torchrun (base.py:22-33)
        if "LOCAL_RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            print("Setting up DDP.")
            self.ddp = True
            local_rank = int(os.environ["LOCAL_RANK"])
            if local_rank != 0:
                sys.stdout = sys.stderr = open(os.devnull, "w")
            if not dist.is_initialized():
                # backend "nccl" IS RCCL on ROCm: one process per GPU, xGMI underneath.  DDPM_DIST_BACKEND=gloo is the
                # test hook for boxes with fewer GPUs than ranks (RCCL refuses two ranks on one device); with
                # DDPM_DIST_SHARED_DEVICE=1 every rank then computes on cuda:0 (tests/test_gpu_dist.py)
                dist.init_process_group(backend=os.environ.get("DDPM_DIST_BACKEND", "nccl"), init_method="env://")
            shared = os.environ.get("DDPM_DIST_SHARED_DEVICE", "0") == "1"
            self.device = torch.device("cuda:0" if shared else f"cuda:{local_rank}")
        else:
            self.ddp = False
            self.device = torch.device("cuda:0")
        torch.cuda.set_device(self.device)
        self.rank = dist.get_rank() if self.ddp else 0
        self.world = dist.get_world_size() if self.ddp else 1

        print(f"Arguments: {str(args)}")
        for k, v in vars(args).items():
            print(f"  {k}: {v}")

        self._setup_stage1(args)
        self._setup_unet(args)
        self._setup_schedule(args)
        self._setup_geometry(args)
        self._restore_checkpoint(args)
        # no optimizer, no GradScaler, no DDP wrap: inference only, every rank reads the same
        # checkpoint file instead of the reference's DDP parameter broadcast (Q15)


    # ---- the pieces of the reference's BaseTrainer.__init__ (base.py:44-158) the reconstruction path needs, one loader each.
    # Attribute names, printed messages and exception types are the reference's (row a2 of SURVEY 8: a caller that catches
    # FileNotFoundError / ValueError or reads trainer.vqvae_config keeps working); the structure is not.
    @staticmethod
    def _require(path: Path, what: str) -> Path:
        if not path.exists():
            raise FileNotFoundError(f"Cannot find {what} {path}")
        return path

    def _setup_stage1(self, args):
        """Stage-1 model (base.py:44-64): a VQ-VAE checkpoint + its vqvae_config.json next to it, or the identity."""
        self.ddpm_channels = 1 if args.is_grayscale else 3
        if not args.vqvae_checkpoint:
            self.vqvae_model = PassthroughVQVAE()
            return
        ckpt = self._require(Path(args.vqvae_checkpoint), "VQ-VAE checkpoint")
        cfg = self._require(ckpt.parent / "vqvae_config.json", "VQ-VAE config")
        self.vqvae_config = json.loads(cfg.read_text())
        self.vqvae_model = VQVAE(**self.vqvae_config)
        state = torch.load(ckpt, map_location="cpu", weights_only=False)["model_state_dict"]
        self.vqvae_model.load_state_dict(state)
        self.vqvae_model.to(self.device).eval()
        print("Loaded vqvae model with config:")
        for k, v in self.vqvae_config.items():
            print(f"  {k}: {v}")
        self.ddpm_channels = self.vqvae_config["embedding_dim"]

    def _setup_unet(self, args):
        """The denoiser (base.py:65-86): `small` / `big` channel tables, one channel count on both sides."""
        if args.model_type not in MODEL_CONFIGS:
            raise ValueError(f"Do not recognise model type {args.model_type}")
        self.model = DiffusionModelUNet(spatial_dims=args.spatial_dimension, in_channels=self.ddpm_channels,
                                        out_channels=self.ddpm_channels, with_conditioning=False,
                                        use_proj_attn=bool(getattr(args, "use_proj_attn", 0)),
                                        **MODEL_CONFIGS[args.model_type]).to(self.device)
        print(f"{sum(p.numel() for p in self.model.parameters()):,} model parameters")

    def _setup_schedule(self, args):
        """Noise schedule attributes + the training scheduler (base.py:88-117); --snr_shift rewrites its tables."""
        for name in ("prediction_type", "beta_schedule", "beta_start", "beta_end", "b_scale", "snr_shift"):
            setattr(self, name, getattr(args, name))
        self.scheduler = DDPMScheduler(num_train_timesteps=1000, prediction_type=self.prediction_type,
                                       schedule=self.beta_schedule, beta_start=self.beta_start, beta_end=self.beta_end)
        if self.snr_shift != 1:
            print("Changing scheduler parameters to shift SNR")
            snr_shift_tables(self.scheduler, self.snr_shift)
        self.simplex_noise = bool(args.simplex_noise)  # AnoDDPM simplex noise instead of Gaussian (ops.simplex_noise)

    def _setup_geometry(self, args):
        """Spatial bookkeeping (base.py:118-131): dimension, resize target, latent padding and its inverse."""
        self.spatial_dimension = args.spatial_dimension
        self.image_size = int(args.image_size) if args.image_size else args.image_size
        self.do_latent_pad = bool(args.latent_pad)
        if self.do_latent_pad:
            self.latent_pad = args.latent_pad
            self.inverse_latent_pad = [-x for x in self.latent_pad]

    def _restore_checkpoint(self, args):
        """DDPM checkpoint (base.py:133-158; map_location added so a CPU-saved file loads, Q4): counters default to a fresh run."""
        self.run_dir = Path(args.output_dir) / args.model_name
        stem = f"checkpoint_{int(args.ddpm_checkpoint_epoch)}" if args.ddpm_checkpoint_epoch else "checkpoint"
        checkpoint_path = self.run_dir / f"{stem}.pth"
        self.start_epoch, self.best_loss, self.global_step, self.optimizer_state = 0, 1000, 0, None
        self.found_checkpoint = checkpoint_path.exists()
        if not self.found_checkpoint:
            return
        checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(checkpoint["model_state_dict"])
        self.start_epoch = checkpoint["epoch"] + 1
        self.global_step = checkpoint["global_step"]
        self.best_loss = checkpoint["best_loss"]
        self.optimizer_state = checkpoint.get("optimizer_state_dict")  # used by DDPMTrainer only
        print(f"Resuming training using checkpoint {checkpoint_path} at epoch {self.start_epoch}")


class Reconstruct(BaseTrainer):
    def __init__(self, args):
        # --anomaly_maps 1 (extension): per-pixel LPIPS and squared-error maps averaged over the t-starts, written next to the CSV
        # (maps_<name>.npz).  bench.py and the tests build their Namespace by hand without the attribute: off.
        self.anomaly_maps = bool(getattr(args, "anomaly_maps", 0))
        if self.anomaly_maps and (int(args.spatial_dimension) != 2 or args.vqvae_checkpoint):
            raise ValueError("--anomaly_maps 1: anomaly maps cover 2-D pixel-space models only (no --spatial_dimension 3, no "
                             "--vqvae_checkpoint): 2.5-D and latent maps are not built")
        # --anomaly_z_maps 1 (extension): the per-t maps normalised per pixel by the validation set's mean and
        # standard deviation, averaged over the t-starts (ood/map_stats.npz, ood/zmaps_<name>.npz).  Off without the attribute.
        self.anomaly_z_maps = bool(getattr(args, "anomaly_z_maps", 0))
        self.z_sigma = float(getattr(args, "anomaly_z_sigma", 0.0) or 0.0)
        self.z_std_floor = float(getattr(args, "anomaly_z_std_floor", 0.01))
        if self.anomaly_z_maps:
            zmaps.check_flags(args.spatial_dimension, args.vqvae_checkpoint, self.z_sigma, self.z_std_floor)
        # --pixel_metrics 1 (extension): the in / out sets' Z-maps against ground-truth masks (--out_masks), as a
        # two-class histogram and per-image TP / FP / FN counts (ood/pixels_<name>.npz).  Off without the attribute.
        self.pixel_metrics = bool(getattr(args, "pixel_metrics", 0))
        if self.pixel_metrics:
            self.px_lo, self.px_hi, self.px_bins, self.px_thresholds, self.px_masks = pixel_metrics.check_flags(
                self.anomaly_z_maps, args.out_ids if bool(args.run_out) else None, getattr(args, "out_masks", None),
                getattr(args, "pixel_bins", pixel_metrics.DEFAULT_BINS), getattr(args, "pixel_range", None) or pixel_metrics.DEFAULT_RANGE,
                getattr(args, "pixel_thresholds", None) or pixel_metrics.DEFAULT_THRESHOLDS)
        # --pixel_regions 1 (extension): on top of --pixel_metrics 1 the masks' connected components, the per-region
        # overlap table and per-image component counts (ood/regions_<name>.npz).  Off without the attribute.
        self.pixel_regions = bool(getattr(args, "pixel_regions", 0))
        if self.pixel_regions:
            self.px_connectivity, self.px_pro_fpr = pixel_metrics.check_region_flags(
                self.pixel_metrics, getattr(args, "pixel_connectivity", pixel_metrics.DEFAULT_CONNECTIVITY),
                getattr(args, "pixel_pro_fpr", pixel_metrics.DEFAULT_PRO_FPR))
        # --pixel_calibrate_fpr F1,F2,... (extension): thresholds above which those fractions of the validation set's
        # leave-one-out Z-map pixels fall (ood/calibration.npz), and the in / out sets' counts at them (ood/calibrated_<name>.npz).
        # Off without the attribute.
        self.px_calibrate = bool(getattr(args, "pixel_calibrate_fpr", None))
        if self.px_calibrate:
            self.cal_fprs, self.cal_budget = pixel_metrics.check_calibration_flags(
                self.anomaly_z_maps, args.pixel_calibrate_fpr, getattr(args, "pixel_calibrate_budget_gb", pixel_metrics.DEFAULT_BUDGET_GB))
            if not self.pixel_metrics:  # (the bins of the validation histogram are those of --pixel_range / --pixel_bins)
                self.px_lo, self.px_hi, self.px_bins = pixel_metrics.check_flags(
                    True, None, None, getattr(args, "pixel_bins", pixel_metrics.DEFAULT_BINS),
                    getattr(args, "pixel_range", None) or pixel_metrics.DEFAULT_RANGE)[:3]
        super().__init__(args)
        if not self.found_checkpoint:
            raise FileNotFoundError("Failed to find a saved model checkpoint.")
        self.last_calibration = None  # the contents of ood/calibration.npz after a validation pass with --pixel_calibrate_fpr
        self.last_calibrated = None  # the same for ood/calibrated_<name>.npz (the in / out sets)
        self._cal = None  # the calibration in force: the file's dict and "thr", the thresholds [2, F] on the device
        self._cal_rows = None  # the validation pass under way: the counted rows' per-t maps, one device tensor per batch
        # test hook (not a CLI flag): keep the retained validation rows and their leave-one-out Z-maps on the host after the
        # pass (``calibration_rows`` [n, n_t, 2, H, W], ``calibration_zmaps`` [n, 2, H, W]; this rank's rows in the pass's order)
        self.keep_calibration_rows = bool(getattr(args, "keep_calibration_rows", False))
        self.calibration_rows = self.calibration_zmaps = None
        self.last_regions = None  # the same for --pixel_regions 1
        self.last_pixels = None  # the same for --pixel_metrics 1 (the in / out sets)
        self._px = None  # the running tables of the pass under way: hist (device), rows (host, one entry per batch)
        self._px_thr = self._px_no_mask = None  # the thresholds / an all-zero mask batch on the device
        self.last_maps = None  # the maps of the last get_scores call (rank 0, --anomaly_maps 1), what _write puts into the .npz
        self.last_zmaps = None  # the same for --anomaly_z_maps 1 (the in / out sets)
        self.last_map_stats = None  # (MapStats, t values) of the last validation pass, merged over the ranks
        self._z_tables = None  # (t values, mean, inv_std on the device) the in / out passes normalise by
        self._z_taps = None  # the smoothing weights on the device (--anomaly_z_sigma > 0)
        self.out_dir = self.run_dir / "ood"
        if self.rank == 0:
            self.out_dir.mkdir(exist_ok=True)
        self.seed = int(args.seed)
        self.num_inference_steps = int(getattr(args, "honour_num_inference_steps", 0)
                                       and args.num_inference_steps) or 100  # Q1: 100 is hard-coded
        self.reset_scheduler_per_t = bool(getattr(args, "reset_scheduler_per_t", 0))
        self.timestep_list = getattr(args, "timestep_list", "monai")
        # test hook (not a CLI flag): only the t-starts <= max_t_start of the reference's list are run -- a PREFIX of the
        # chained list, so the trajectories that do run are exactly the reference's (tests price the CPU oracle per forward)
        self.max_t_start = getattr(args, "max_t_start", None)
        # test hook: keep only these members of the chained t-start list (in the list's order): long chains at a few start points
        self.t_start_subset = getattr(args, "t_start_subset", None)
        self.lpips_weights = getattr(args, "lpips_weights", None)
        self._loader_args = dict(batch_size=args.batch_size, is_grayscale=bool(args.is_grayscale),
                                 image_size=self.image_size, drop_last=bool(args.drop_last),
                                 spatial_dimension=args.spatial_dimension, image_roi=args.image_roi,
                                 rank=self.rank, world=self.world)
        self.val_loader = get_data_loader(args.validation_ids,
                                          first_n=int(args.first_n_val) if args.first_n_val else args.first_n_val,
                                          **self._loader_args)
        self.in_loader = get_data_loader(args.in_ids, first_n=int(args.first_n) if args.first_n else args.first_n,
                                         **self._loader_args)
        self._ts_cache = {}
        self._pl = None
        self.last_stats = {}
        self.profile_first_steps = False  # bench.py: hipEvent-bracket the first UNet step of each t-start

    # ---- helpers -------------------------------------------------------------------------------------
    def _timesteps_tensor(self, step: int, batch: int) -> torch.Tensor:
        key = (int(step), batch)
        t = self._ts_cache.get(key)
        if t is None:
            t = torch.full((batch,), int(step), dtype=torch.int64, device=self.device)
            self._ts_cache[key] = t
        return t

    def _perceptual(self) -> PerceptualLoss:
        if self._pl is None:
            pl = PerceptualLoss(dimensions=self.spatial_dimension, include_pixel_loss=False,
                                is_fake_3d=True if self.spatial_dimension == 3 else False, lpips_normalize=True,
                                spatial=False)
            if self.lpips_weights:
                pl.perceptual_function.load_pretrained_state_dict(
                    torch.load(self.lpips_weights, map_location="cpu", weights_only=False))
            elif self.rank == 0:
                # the reference builds lpips.LPIPS(pretrained=True) (perceptual_loss.py:68-84); those weights
                # cannot be fetched here, so say loudly that this column is not LPIPS
                print("WARNING: no --lpips_weights given: LPIPS-AlexNet runs with SEEDED RANDOM weights, so the "
                      "'perceptual_difference' column (and plot_target=perceptual_difference / mse+perceptual) is "
                      "NOT an LPIPS value. Only 'mse' is comparable with the reference. Export weights on a "
                      "machine with the lpips package: torch.save(lpips.LPIPS(net='alex').state_dict(), path).",
                      file=sys.__stderr__, flush=True)
            self._pl = pl.to(self.device)
        return self._pl

    def make_scheduler(self) -> PNDMScheduler:
        s = PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, prediction_type=self.prediction_type,
                          schedule=self.beta_schedule, beta_start=self.beta_start, beta_end=self.beta_end,
                          timestep_list=self.timestep_list)
        if self.snr_shift != 1:
            snr_shift_tables(s, self.snr_shift)
        s.set_timesteps(self.num_inference_steps)
        return s

    # ---- the hot loops (reconstruct.py:72-250) ---------------------------------------------------
    @torch.no_grad()
    def get_scores(self, loader, dataset_name, inference_skip_factor):
        quiet = getattr(self, "quiet", False)
        if self.ddp and not quiet:
            sys.stdout, sys.stderr = sys.__stdout__, sys.__stderr__
            print(f"{self.rank}: {dataset_name}")
        elif not quiet:
            print(f"{dataset_name}")
        pl = self._perceptual()
        self.model.eval()
        ids_all, names_all, scores_all, maps_all, zmaps_all = [], [], [], [], []
        self.last_maps = self.last_zmaps = self.last_calibrated = None
        # --anomaly_z_maps 1: the validation pass accumulates the per-pixel statistics, every other pass is normalised by them
        z_stats = zmaps.MapStats() if self.anomaly_z_maps and dataset_name == "val" else None
        self.last_pixels = None
        self._px = {"hist": None, "rows": []} if self.pixel_metrics and dataset_name != "val" else None
        self.last_regions = None
        z_skipped = 0
        t_values = [int(t) for t in reversed(self.make_scheduler().timesteps)[1::inference_skip_factor]
                    if (self.max_t_start is None or int(t) <= int(self.max_t_start))
                    and (self.t_start_subset is None or int(t) in set(self.t_start_subset))]
        self._cal_rows = None
        if self.px_calibrate and z_stats is not None:  # the counted rows stay on the device for the leave-one-out pass: refuse first
            shape = tuple(loader.images[0].shape) if len(loader.names) else (0, 0)
            pixel_metrics.check_budget(len(loader.names), len(t_values), shape[-2], shape[-1], self.cal_budget)
            self._cal_rows = []
        n_recon = n_fwd = 0
        guard = {"batches_rerun_fp32": 0, "batches_nonfinite": 0}
        _lib.status_read(clear=True)  # whatever an earlier caller left behind is not this run's
        quantises = not isinstance(self.vqvae_model, PassthroughVQVAE)
        if quantises:
            guard["vq_near_ties"] = 0  # latent positions whose two nearest codes were within 1e-5: candidates for a code flip
            _lib.vq_near_ties_read(clear=True)
        for batch in loader:
            scores, t_values, n_r, n_f, B, dt, maps, per_t_maps = self._score_batch(batch, pl, inference_skip_factor)
            # numeric guard (include/ddpm_ood_hip.h): a non-finite eps / reconstruction / latent set the device status word.
            # With the split-f16 kernels on, that may be an operand beyond the f16 range rather than a genuine fp32
            # overflow: run the affected IMAGES again on the fp32-MFMA kernels; what is still non-finite then is written as
            # NaN, like the reference would (reconstruct.py:188-204 has no check).
            word = _lib.status_read(clear=True)
            if word and _lib.split_f16_active():
                # only the images that came out non-finite ride again (clamp + MSE keeps a NaN: a non-finite eps, latent or
                # reconstruction ends as a non-finite score of ITS image; a per-image result does not depend on the batch it
                # rides in -- noise is a function of the image index, the PLMS history is per element)
                bad = (~torch.isfinite(scores).all(dim=2).all(dim=1)).nonzero().flatten().cpu().tolist()
                if not bad:
                    bad = list(range(B))
                print(f"WARNING: {_lib.status_text(word)} in a batch of {B} on the split-f16 kernels: running {len(bad)} image(s) "
                      f"again with fp32 MFMA products (ddpm_set_split_f16(0); permanently: DDPM_WINO44_F16X3=0 "
                      f"DDPM_CONV1X1_F16X3=0 DDPM_ATTN_F16X3=0 DDPM_DOWN_S2H=0)", file=sys.__stderr__, flush=True)
                if quantises:  # the counter must match the scores that are KEPT: a wholly discarded pass contributes nothing
                    first_pass = _lib.vq_near_ties_read(clear=True)
                    if len(bad) < B:  # (includes the re-run images' share of the first pass: an upper bound)
                        guard["vq_near_ties"] += first_pass
                prev = _lib.set_split_f16(False)
                try:
                    sub = sub_batch(batch, bad)
                    scores_b, t_values, _, n_f2, _, dt2, maps_b, per_t_b = self._score_batch(sub, pl, inference_skip_factor)
                    scores[torch.as_tensor(bad, device=scores.device)] = scores_b
                    if maps is not None:  # the maps follow the scores that are kept
                        maps[torch.as_tensor(bad, device=maps.device)] = maps_b
                    if per_t_maps is not None:
                        per_t_maps[torch.as_tensor(bad, device=per_t_maps.device)] = per_t_b
                    n_f += n_f2
                    dt += dt2
                    word = _lib.status_read(clear=True)
                finally:
                    _lib.set_split_f16(prev)
                guard["batches_rerun_fp32"] += 1
                guard["images_rerun_fp32"] = guard.get("images_rerun_fp32", 0) + len(bad)
            if quantises:
                guard["vq_near_ties"] += _lib.vq_near_ties_read(clear=True)
            if word:
                guard["batches_nonfinite"] += 1
                print(f"WARNING: {_lib.status_text(word)} with fp32 products too: a genuine overflow of this checkpoint on "
                      f"these inputs; the affected scores are NaN / inf in the CSV, as the reference would write them",
                      file=sys.__stderr__, flush=True)
            n_recon += n_r
            n_fwd += n_f
            scores_all.append(scores)
            if maps is not None:
                maps_all.append(maps.cpu())  # one device->host copy per batch, after the batch's synchronisation
            if per_t_maps is not None:  # after the guard: the statistics see the per-t maps of the scores that are kept
                z_skipped += self._z_batch(z_stats, scores, per_t_maps, t_values, zmaps_all, batch.get("mask"))
            ids_all.append(torch.tensor(batch["index"], dtype=torch.int32))
            names_all.extend(batch["image_meta_dict"]["filename_or_obj"])
            if quiet:
                pass
            elif self.ddp:
                print(f"{self.rank}: Took {dt}s for a batch size of {B}")
            else:
                print(f"Took {dt}s for a batch size of {B}")
        self.last_stats = {"reconstructions": n_recon, "unet_forwards": n_fwd,
                           "lpips_pretrained": bool(pl.perceptual_function.pretrained), **guard}
        if self.anomaly_z_maps:
            self.last_stats["zmap_rows_skipped"] = z_skipped
            if z_stats is not None:
                self._z_finish_validation(loader, z_stats, t_values)
                if self.px_calibrate:
                    self._cal_finish_validation(self.last_map_stats[0], t_values)
        return self._collect(loader, dataset_name, t_values, ids_all, names_all, scores_all, quiet, maps_all, zmaps_all)

    def _score_batch(self, batch, pl, inference_skip_factor):
        """One batch through reconstruct.py:97-204: every t-start's noise, PLMS trajectory, decode, MSE and LPIPS.
        Returns (scores [B, n_t, 2] on the device, t values, reconstructions, UNet image-forwards, B, seconds, maps, per-t
        maps): maps is None, or with --anomaly_maps 1 the device tensor [B, 2, H, W] of the per-pixel LPIPS (channel 0) and
        squared error (channel 1), each the mean over the t-starts; per-t maps is None, or with --anomaly_z_maps 1 the same two
        channels of every t-start by itself, [B, n_t, 2, H, W] (B * n_t * 2 * H * W * 4 bytes)."""
        n_recon = n_fwd = 0
        sched = self.make_scheduler()  # one per batch: PLMS history leaks across t-starts (Q3)
        timesteps = sched.timesteps
        start_points = reversed(timesteps)[1::inference_skip_factor]
        if self.max_t_start is not None:
            start_points = start_points[start_points <= int(self.max_t_start)]
        if self.t_start_subset is not None:
            start_points = start_points[torch.isin(start_points, torch.as_tensor(list(self.t_start_subset), dtype=start_points.dtype))]
        t_values = [int(t) for t in start_points]

        t1 = time.time()
        images_original = batch["image"].to(self.device, non_blocking=True).float().contiguous()
        images = self.vqvae_model.encode_stage_2_inputs(images_original).float().contiguous()
        if self.do_latent_pad:
            images = F.pad(input=images, pad=self.latent_pad, mode="constant", value=0)
        B = images.shape[0]
        idx = batch["index"]
        per_t = []
        lp_map = se_map = None
        if self.anomaly_maps:  # accumulated into once per t-start with weight 1 / n_t; no synchronisation inside the loop
            lp_map = torch.zeros((B,) + tuple(images_original.shape[2:]), dtype=torch.float32, device=self.device)
            se_map = torch.zeros_like(lp_map)
            w_t = 1.0 / max(len(t_values), 1)
        per_t_maps = [] if self.anomaly_z_maps else None  # fresh maps of every t-start at weight 1 (2-D only)
        for t_start in start_points:
            if self.reset_scheduler_per_t:
                sched.set_timesteps(self.num_inference_steps)
            start_timesteps = torch.Tensor([t_start] * B).long()
            if self.simplex_noise:  # reconstruct.py:133-139: T = t_start for every row; the (padded) latent's shape
                noise = ops.simplex_noise(images.shape, simplex_seeds(self.seed, idx, int(t_start), images.shape[1]),
                                          start_timesteps, device=self.device)
            else:
                noise = batch_noise(self.seed, idx, int(t_start), images.shape).to(self.device, non_blocking=True)
            x = sched.add_noise(original_samples=images, noise=noise, timesteps=start_timesteps,
                                b_scale=self.b_scale)
            first = self.profile_first_steps
            for step in timesteps[timesteps <= t_start]:
                if first:
                    _lib.load().ddpm_prof_enable(1)
                eps = self.model(x, timesteps=self._timesteps_tensor(int(step), B))
                x, _ = sched.step(eps, step, x)
                if first:
                    _lib.load().ddpm_prof_enable(0)
                    first = False
                n_fwd += B
            if self.do_latent_pad:
                x = F.pad(input=x, pad=self.inverse_latent_pad, mode="constant", value=0).contiguous()
            prof_decode = self.profile_first_steps and not isinstance(self.vqvae_model, PassthroughVQVAE)
            if prof_decode:
                _lib.load().ddpm_prof_enable(1)
            x = self.vqvae_model.decode_stage_2_outputs(x).contiguous()
            if prof_decode:
                _lib.load().ddpm_prof_enable(0)
            mse = ops.clamp_mse_(images_original, x, self.b_scale)  # x / b_scale, clamp_(0, 1), MSE
            if self.anomaly_maps:  # (2-D only) the same value from the same launches, and the map from the same features
                ops.sqerr_map(images_original, x, w_t, out=se_map)
                # --anomaly_z_maps 1 beside it: the resampling kernel runs a second time on the same packed layer maps
                second = {"second_weight": 1.0} if self.anomaly_z_maps else {}
                if images_original.shape[3] == 28:
                    pd_, *lp_t = pl.forward_with_map(F.pad(images_original, (2, 2, 2, 2)), F.pad(x, (2, 2, 2, 2)),
                                                     window=(2, 2) + tuple(images_original.shape[2:]), weight=w_t, out=lp_map,
                                                     **second)
                else:
                    pd_, *lp_t = pl.forward_with_map(images_original, x, weight=w_t, out=lp_map, **second)
                pd_ = pd_.reshape(B)
                if self.anomaly_z_maps:
                    per_t_maps.append(torch.stack([lp_t[1][:, 0], ops.sqerr_map(images_original, x)], dim=1))
            elif self.anomaly_z_maps:  # (2-D only) the score from the launches ``pl(...)`` makes, and this t-start's two maps
                if images_original.shape[3] == 28:
                    pd_, lp_t = pl.forward_with_map(F.pad(images_original, (2, 2, 2, 2)), F.pad(x, (2, 2, 2, 2)),
                                                    window=(2, 2) + tuple(images_original.shape[2:]))
                else:
                    pd_, lp_t = pl.forward_with_map(images_original, x)
                pd_ = pd_.reshape(B)
                per_t_maps.append(torch.stack([lp_t[:, 0], ops.sqerr_map(images_original, x)], dim=1))
            elif self.spatial_dimension == 2:
                if images_original.shape[3] == 28:
                    pd_ = pl(F.pad(images_original, (2, 2, 2, 2)), F.pad(x, (2, 2, 2, 2)))
                else:
                    pd_ = pl(images_original, x)
                pd_ = pd_.reshape(B)
            else:
                pd_ = torch.stack([pl(images_original[b, None, ...], x[b, None, ...]).reshape(())
                                   for b in range(B)])
            per_t.append(torch.stack([pd_, mse], dim=1))
            n_recon += B
        scores = torch.stack(per_t, dim=1)  # [B, n_t, 2] on the device
        maps = torch.stack([lp_map, se_map], dim=1) if self.anomaly_maps else None  # [B, 2, H, W]
        if per_t_maps is not None:
            per_t_maps = torch.stack(per_t_maps, dim=1) if per_t_maps else None  # [B, n_t, 2, H, W] (no t-start: nothing)
        torch.cuda.current_stream().synchronize()
        t2 = time.time()
        return scores, t_values, n_recon, n_fwd, B, t2 - t1, maps, per_t_maps

    def _z_batch(self, z_stats, scores, per_t_maps, t_values, zmaps_all, mask=None):
        """--anomaly_z_maps 1, one batch after the numeric guard.  Validation pass (``z_stats`` given): the per-t maps of the
        images whose scores are all finite go into the running statistics (one launch); returns how many images were left out.
        Any other pass: the batch's Z-maps [B, 2, H, W] -- one launch, one more per batch when smoothing -- are appended to
        ``zmaps_all`` on the host (one device->host copy per batch, after the batch's synchronisation).  --pixel_metrics 1: the
        batch's Z-maps, still on the device, are also counted against ``mask`` (uint8 [B, 1, H, W]; None: all zero), per channel
        one histogram launch into the pass's table and one counts launch; the counts ride to the host inside the same copy."""
        B, n_t = per_t_maps.shape[:2]
        if z_stats is not None:
            finite = torch.isfinite(scores).all(dim=2).all(dim=1)
            keep = int(finite.sum())
            counted = per_t_maps if keep == B else per_t_maps[finite].contiguous() if keep else None
            if counted is not None:
                z_stats.update(counted)
                if self._cal_rows is not None:  # --pixel_calibrate_fpr: the very tensor the statistics received stays on the device
                    self._cal_rows.append(counted)
            return B - keep
        if self._z_tables is None or self._z_tables[0] != list(t_values) or self._z_tables[1].shape != per_t_maps.shape[1:]:
            self._z_tables = self._z_load_tables(t_values, tuple(per_t_maps.shape[3:]))
        _, mean, inv_std = self._z_tables
        H, W = per_t_maps.shape[3:]
        z = ops.map_zscore(per_t_maps.reshape(B, n_t, 2 * H * W), mean.reshape(n_t, 2 * H * W), inv_std.reshape(n_t, 2 * H * W))
        if self.z_sigma > 0:
            if self._z_taps is None:
                self._z_taps = torch.from_numpy(ops.gaussian_taps(self.z_sigma).astype(np.float32)).to(self.device)
            z = ops.map_blur(z.reshape(B * 2, H, W), taps=self._z_taps)
        if self._px is None:
            zmaps_all.append(z.reshape(B, 2, H, W).cpu())
            return 0
        counts, mask_pixels = self._px_batch(z.reshape(B, 2, H * W), mask)
        # one copy: each image's Z-maps travel as their int32 bit patterns with the int32 counts behind them (every bit is kept)
        parts = [z.reshape(B, 2 * H * W).view(torch.int32), counts.reshape(B, -1)]
        if self.pixel_regions:  # (the component counts and the regions per image ride in the same copy)
            components, regions = self._px_regions_batch(z.reshape(B, 2, H * W), H, W)
            parts += [components.reshape(B, -1), regions[:, None]]
        n_cal = 0
        if self.px_calibrate:  # (the counts at the calibrated thresholds ride behind everything else in the same copy)
            cal = self._px_calibrated_batch(z.reshape(B, 2, H * W), H, W, t_values)
            n_cal = cal.shape[1]
            parts.append(cal)
        self._px.pop("mask", None)
        self._px.pop("labels", None)
        both = torch.cat(parts, dim=1).cpu()
        cal_host = both[:, both.shape[1] - n_cal:]
        both = both[:, :both.shape[1] - n_cal]
        zmaps_all.append(both[:, :2 * H * W].contiguous().view(torch.float32).reshape(B, 2, H, W))
        n_counts = counts[0].numel()
        rows = [both[:, 2 * H * W:2 * H * W + n_counts], mask_pixels.to(torch.int32)[:, None], both[:, 2 * H * W + n_counts:]]
        # [counts | mask_pixels | with --pixel_regions 1: components | regions | with --pixel_calibrate_fpr: the calibrated counts]
        self._px["rows"].append(torch.cat(rows + [cal_host], dim=1))
        return 0

    def _px_batch(self, z, mask):
        """--pixel_metrics 1, one batch: ``z`` [B, 2, H W] on the device against ``mask``.  Returns (counts int32 [B, 2, K, 3] on
        the device, the masks' pixel counts [B] on the host); the histograms are added into the pass's [2, 2, nbins + 1] table."""
        B, _, P = z.shape
        if P >= 1 << 31:
            raise ValueError(f"--pixel_metrics 1: maps of {P} pixels do not fit the 32-bit counts")
        if mask is None:  # (the in set, an out set without masks: every pixel is a negative)
            if self._px_no_mask is None or self._px_no_mask.shape[0] < B or self._px_no_mask.shape[1] != P:
                self._px_no_mask = torch.zeros((B, P), dtype=torch.uint8, device=self.device)
            m, mask_pixels = self._px_no_mask[:B], torch.zeros(B, dtype=torch.int64)
        else:
            if mask.shape[0] != B or mask.numel() != B * P:
                raise ValueError(f"--pixel_metrics 1: masks of {tuple(mask.shape)} for maps of {B} x {P} pixels")
            mask_pixels = (mask.reshape(B, P) != 0).sum(dim=1).cpu()
            m = mask.reshape(B, P).to(device=self.device, dtype=torch.uint8).contiguous()
        if self._px["hist"] is None:
            self._px["hist"] = torch.zeros((2, 2, self.px_bins + 1), dtype=torch.int64, device=self.device)
        if self._px_thr is None:
            self._px_thr = torch.tensor(self.px_thresholds, dtype=torch.float32, device=self.device)
        counts = []
        for c in range(2):
            zc = z[:, c].contiguous()
            ops.map_mask_hist(zc, m, self.px_lo, self.px_hi, self.px_bins, total=self._px["hist"][c])
            counts.append(ops.map_mask_counts(zc, m, self._px_thr))
        if self.pixel_regions or self.px_calibrate:
            self._px["mask"] = m  # (for _px_regions_batch / _px_calibrated_batch)
        return torch.stack(counts, dim=1), mask_pixels

    def _px_regions_batch(self, z, H, W):
        """--pixel_regions 1, one batch, after ``_px_batch`` (which left the batch's mask on the device): the mask's connected
        components are labelled once; per channel one overlap call into the pass's [2, nbins + 1] float64 table and one
        component-counts call.  Returns (components int32 [B, 2, K, 3], regions int32 [B]) on the device.  A set without masks
        runs on the all-zero mask: 0 regions, nothing added to the table, hit = 0."""
        B, _, P = z.shape
        if P > ops.MAP_LABEL_MAX_PIXELS:
            raise ValueError(f"--pixel_regions 1: maps of {H} x {W} pixels are above the {ops.MAP_LABEL_MAX_PIXELS} pixels "
                             f"(128 x 128) a labelled plane may have")
        m = self._px["mask"].reshape(B, H, W)
        labels, regions = ops.map_label(m, self.px_connectivity)
        self._px["labels"] = (labels, regions)  # (for _px_calibrated_batch)
        if self._px.get("overlap") is None:
            self._px["overlap"] = torch.zeros((2, self.px_bins + 1), dtype=torch.float64, device=self.device)
        components = []
        for c in range(2):
            zc = z[:, c].contiguous().reshape(B, H, W)
            ops.map_region_overlap(zc, labels, regions, self.px_lo, self.px_hi, self.px_bins, total=self._px["overlap"][c])
            components.append(ops.map_component_counts(zc, m, labels, regions, self._px_thr, self.px_connectivity))
        return torch.stack(components, dim=1), regions

    def _px_calibrated_batch(self, z, H, W, t_values):
        """--pixel_calibrate_fpr with --pixel_metrics 1, one batch, after ``_px_batch`` (and ``_px_regions_batch``): per channel one
        more counts call at that channel's calibrated thresholds, with --pixel_regions 1 one more component-counts call.  Returns
        int32 [B, 2 F 3] (with regions [B, 2 F 3 + 2 F 3]) on the device: the counts of both channels, then the components."""
        B = z.shape[0]
        thr = self._cal_load(t_values)["thr"]
        m = self._px["mask"]
        counts = [ops.map_mask_counts(z[:, c].contiguous(), m, thr[c]) for c in range(2)]
        parts = [torch.stack(counts, dim=1).reshape(B, -1)]
        if self.pixel_regions:
            labels, regions = self._px["labels"]
            comps = [ops.map_component_counts(z[:, c].contiguous().reshape(B, H, W), m.reshape(B, H, W), labels, regions, thr[c],
                                              self.px_connectivity) for c in range(2)]
            parts.append(torch.stack(comps, dim=1).reshape(B, -1))
        return torch.cat(parts, dim=1)

    def _cal_set(self, cal):
        self._cal = dict(cal, thr=torch.from_numpy(np.ascontiguousarray(cal["thresholds"], dtype=np.float32)).to(self.device))
        return self._cal

    def _cal_load(self, t_values):
        """The calibration of this process's validation pass, else that of ood/calibration.npz (--run_val 0), which must have
        been written with this run's t-starts, range, bins, smoothing, floor and target rates."""
        if self._cal is None or [int(t) for t in self._cal["t"]] != [int(t) for t in t_values]:
            if self.last_calibration is not None:
                raise ValueError(f"--pixel_calibrate_fpr: the validation pass calibrated on t = {[int(t) for t in self.last_calibration['t']]}"
                                 f", this set has t = {list(t_values)}")
            self._cal_set(pixel_metrics.load_calibration(self.out_dir / pixel_metrics.CALIBRATION_FILE, t_values, self.px_lo,
                                                         self.px_hi, self.px_bins, self.z_sigma, self.z_std_floor, self.cal_fprs))
        return self._cal

    def _cal_finish_validation(self, stats, t_values):
        """--pixel_calibrate_fpr, after ``_z_finish_validation``: every rank uploads the merged mean and M2 (float64 rounded once to
        fp32; the same tables on every rank) and the floor, forms the leave-one-out Z-maps of the rows it kept batch by batch
        (smoothed like every other set's) and bins them per channel; with N ranks ONE all_reduce of the int64 table.  Every rank
        derives the same thresholds; rank 0 keeps the file's contents for ``_write``."""
        rows, self._cal_rows = self._cal_rows, None
        n, mean, m2 = stats.tables()
        if n < 3:
            raise ValueError(f"--pixel_calibrate_fpr: leaving one of {n} validation image(s) out leaves fewer than 2: at least 3 are needed")
        mean_d = torch.from_numpy(mean.astype(np.float32)).to(self.device)
        m2_d = torch.from_numpy(m2.astype(np.float32)).to(self.device)
        floor_d = torch.from_numpy(stats.floor(self.z_std_floor)).to(self.device)
        hist = torch.zeros((2, 2, self.px_bins + 1), dtype=torch.int64, device=self.device)  # [channel, class, bin]: class 1 stays 0
        kept = []
        for per_t in rows:
            B, _, _, H, W = per_t.shape
            z = ops.map_zscore_loo(per_t, mean_d, m2_d, n, floor_d)
            if self.z_sigma > 0:
                if self._z_taps is None:
                    self._z_taps = torch.from_numpy(ops.gaussian_taps(self.z_sigma).astype(np.float32)).to(self.device)
                z = ops.map_blur(z.reshape(B * 2, H, W), taps=self._z_taps)
            z = z.reshape(B, 2, H * W)
            if self._px_no_mask is None or self._px_no_mask.shape[0] < B or self._px_no_mask.shape[1] != H * W:
                self._px_no_mask = torch.zeros((B, H * W), dtype=torch.uint8, device=self.device)
            for c in range(2):
                ops.map_mask_hist(z[:, c].contiguous(), self._px_no_mask[:B], self.px_lo, self.px_hi, self.px_bins, total=hist[c])
            if self.keep_calibration_rows:
                kept.append((per_t.cpu(), z.reshape(B, 2, H, W).cpu()))
        hist = hist[:, 0].contiguous()
        if self.ddp:
            if dist.get_backend() == "gloo" and hist.is_cuda:  # (the test hook of gather_scores)
                hist = hist.cpu()
            dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        if self.keep_calibration_rows:
            self.calibration_rows = torch.cat([k[0] for k in kept]).numpy() if kept else None
            self.calibration_zmaps = torch.cat([k[1] for k in kept]).numpy() if kept else None
        cal = pixel_metrics.calibration_tables(hist.cpu().numpy(), t_values, n, self.cal_fprs, self.px_lo, self.px_hi, self.px_bins,
                                               self.z_sigma, self.z_std_floor)
        self.last_calibration = cal
        self._cal_set(cal)

    def _z_set_tables(self, stats, t_values):
        mean, inv_std = stats.finalize(self.z_std_floor)
        self._z_tables = ([int(t) for t in t_values], torch.from_numpy(mean).to(self.device), torch.from_numpy(inv_std).to(self.device))
        return self._z_tables

    def _z_load_tables(self, t_values, extent):
        """The statistics of this process's validation pass, else those of ood/map_stats.npz (--run_val 0)."""
        if self.last_map_stats is not None:
            stats, t_val = self.last_map_stats
            if [int(t) for t in t_val] != [int(t) for t in t_values] or tuple(stats.tables()[1].shape[2:]) != tuple(extent):
                raise ValueError(f"--anomaly_z_maps 1: the validation pass gave statistics for t = {t_val} and maps of "
                                 f"{tuple(stats.tables()[1].shape[2:])}, this set has t = {list(t_values)} and {tuple(extent)}")
            return self._z_set_tables(stats, t_values)
        return self._z_set_tables(zmaps.MapStats.load(self.out_dir / zmaps.STATS_FILE, t_values, extent), t_values)

    def _z_finish_validation(self, loader, z_stats, t_values):
        """After the validation pass: with N ranks ONE all_gather of (n, mean, m2) and the same float64 merge on every rank,
        so that every rank finalises the same tables; rank 0 keeps them for ``_write`` (ood/map_stats.npz)."""
        n, mean, m2 = z_stats.tables()
        if self.ddp:
            if hasattr(loader, "all_names") and len(loader.all_names) < self.world:
                raise ValueError(f"--anomaly_z_maps 1: {len(loader.all_names)} images over {self.world} ranks leave a rank "
                                 f"without an image, and the maps' extent comes from the images")
            if mean is None:
                raise ValueError("--anomaly_z_maps 1: this rank counted no validation image: no statistics to gather")
            if n >= 1 << 24:
                raise ValueError(f"--anomaly_z_maps 1: a row count of {n} is not exact in the fp32 payload")
            payload = torch.cat([torch.tensor([float(n)], dtype=torch.float32, device=self.device),
                                 z_stats.mean.reshape(-1), z_stats.m2.reshape(-1)])[None]  # [1, 1 + 2 P]: stacked rank by rank
            if dist.get_backend() == "gloo" and payload.is_cuda:  # (the test hook of gather_scores)
                payload = payload.cpu()
            out = torch.empty((self.world, payload.numel()), dtype=torch.float32, device=payload.device)
            dist.all_gather_into_tensor(out, payload)
            out = out.cpu().double().numpy()
            P = mean.size
            n, mean, m2 = zmaps.MapStats.merge([(int(r[0]), r[1:1 + P].reshape(mean.shape), r[1 + P:].reshape(mean.shape))
                                                for r in out])
        if mean is None:
            raise ValueError("--anomaly_z_maps 1: the validation pass counted no image: no statistics")
        stats = zmaps.MapStats.from_tables(n, mean, m2, t_values)
        self.last_map_stats = (stats, [int(t) for t in t_values])
        self._z_set_tables(stats, t_values)  # (n < 2 or a channel that never varies: refused here, on every rank alike)

    def _collect(self, loader, dataset_name, t_values, ids_all, names_all, scores_all, quiet, maps_all=(), zmaps_all=()):
        """reconstruct.py:238-250: everyone's rows on every rank, through ONE collective (with --anomaly_maps 1 a second one
        of the same scheme carries the maps; rank 0 keeps them in ``last_maps`` for ``_write``; --anomaly_z_maps 1: a further
        one for the Z-maps of an in / out set, ``last_zmaps``)."""
        if not scores_all and not self.ddp:
            return []
        local_ids = torch.cat(ids_all) if ids_all else torch.zeros((0,), dtype=torch.int32)
        if scores_all:
            scores = torch.cat(scores_all, dim=0)
            ids = torch.cat(ids_all).to(self.device)
        else:  # a rank whose shard is empty still takes part in the collective
            scores = torch.zeros((0, len(t_values), 2), dtype=torch.float32, device=self.device)
            ids = torch.zeros((0,), dtype=torch.int32, device=self.device)
        name_of = dict(zip((int(i) for i in ids.cpu()), names_all))
        counts = [int(ids.shape[0])]
        if self.ddp:
            n_total = len(loader.all_names) if hasattr(loader, "all_names") else None
            n_max = -(-n_total // self.world) if n_total is not None else None
            if scores.is_cuda:
                torch.cuda.synchronize()  # (the batch loop already synchronised at its last status read: this prices the collective alone)
            t_g = time.perf_counter()
            ids, scores, counts = gather_scores(ids, scores, n_max)
            if scores.is_cuda:
                torch.cuda.synchronize()
            self.last_stats["gather_ms"] = round((time.perf_counter() - t_g) * 1e3, 3)  # wait for the slowest rank included
            # every rank can name every image: the id list is the same file on every rank
            name_of = {i: n for i, n in enumerate(loader.all_names)} if hasattr(loader, "all_names") else name_of
            if int(os.environ["LOCAL_RANK"]) != 0 and not quiet:
                sys.stdout = sys.stderr = open(os.devnull, "w")
        # the one device->host copy of the scores
        results = rows_from_scores(ids.cpu().tolist(), scores.cpu().numpy(), counts, t_values, name_of,
                                   loader.batch_size, dataset_name)
        if self.anomaly_maps:
            self._collect_maps(loader, results, t_values, local_ids, ids.cpu().tolist(), name_of, maps_all)
        if self.anomaly_z_maps and dataset_name != "val":  # (the validation set gets no Z-maps)
            got = self._gather_map_rows("--anomaly_z_maps 1", loader, results, local_ids, ids.cpu().tolist(), name_of, zmaps_all)
            if got is not None:
                stems, z = got
                self.last_zmaps = {"filename": np.asarray(stems), "t": np.asarray(t_values, dtype=np.int64),
                                   "z_lpips_map": np.ascontiguousarray(z[:, 0]), "z_mse_map": np.ascontiguousarray(z[:, 1]),
                                   "sigma": np.float64(self.z_sigma), "rel_floor": np.float64(self.z_std_floor)}
            if self._px is not None:
                self._collect_pixels(loader, results, t_values, local_ids, ids.cpu().tolist(), name_of, zmaps_all)
        self._px = None
        return results

    def _collect_pixels(self, loader, results, t_values, local_ids, gathered_ids, name_of, zmaps_all):
        """--pixel_metrics 1: the histogram summed over the ranks (ONE all_reduce of the int64 table) and every rank's count rows
        in the CSV's order of first appearance (the collective of the maps; its payload is fp32, so a count must stay below
        2^24).  Rank 0 keeps both in ``last_pixels`` for ``_write``."""
        hist = self._px["hist"]
        K = len(self.px_thresholds)
        pixels = int(zmaps_all[0].shape[2] * zmaps_all[0].shape[3])
        if self.ddp:
            if pixels >= 1 << 24:
                raise ValueError(f"--pixel_metrics 1: a count of up to {pixels} pixels is not exact in the fp32 payload of the "
                                 f"gather (H W must stay below 2^24 with more than one rank)")
            if dist.get_backend() == "gloo" and hist.is_cuda:  # (the test hook of gather_scores)
                hist = hist.cpu()
            dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        overlap = self._px.get("overlap")
        if self.pixel_regions and self.ddp:  # (one more all_reduce: the float64 overlap table)
            if dist.get_backend() == "gloo" and overlap.is_cuda:
                overlap = overlap.cpu()
            dist.all_reduce(overlap, op=dist.ReduceOp.SUM)
        got = self._gather_map_rows("--pixel_metrics 1", loader, results, local_ids, gathered_ids, name_of, self._px["rows"])
        if got is not None:
            stems, rows = got
            rows = np.rint(rows).astype(np.int64)
            if self.px_calibrate:  # the trailing columns: counts [2, F, 3] at the calibrated thresholds, with regions components [2, F, 3]
                F = len(self.cal_fprs)
                n_cal = 2 * F * 3 * (2 if self.pixel_regions else 1)
                rows, cal_rows = rows[:, :-n_cal], rows[:, -n_cal:].astype(np.int32)
                self.last_calibrated = {"filename": np.asarray(stems), "fpr": np.asarray(self._cal["fpr"], dtype=np.float64),
                                        "thresholds": np.asarray(self._cal["thresholds"], dtype=np.float32),
                                        "counts": cal_rows[:, :2 * F * 3].reshape(-1, 2, F, 3)}
                if self.pixel_regions:
                    self.last_calibrated["components"] = cal_rows[:, 2 * F * 3:].reshape(-1, 2, F, 3)
            if self.pixel_regions:  # the columns behind mask_pixels: components [2, K, 3], regions
                rows, extra = rows[:, :2 * K * 3 + 1], rows[:, 2 * K * 3 + 1:]
                self.last_regions = {"filename": np.asarray(stems), "t": np.asarray(t_values, dtype=np.int64),
                                     "channels": np.asarray(zmaps.CHANNELS), "lo": np.float64(self.px_lo),
                                     "hi": np.float64(self.px_hi), "nbins": np.int64(self.px_bins),
                                     "connectivity": np.int64(self.px_connectivity), "regions": extra[:, -1].astype(np.int32),
                                     "overlap": overlap.cpu().numpy().astype(np.float64),
                                     "thresholds": np.asarray(self.px_thresholds, dtype=np.float32),
                                     "components": extra[:, :-1].reshape(-1, 2, K, 3).astype(np.int32),
                                     "sigma": np.float64(self.z_sigma)}
            self.last_pixels = {"filename": np.asarray(stems), "t": np.asarray(t_values, dtype=np.int64),
                                "channels": np.asarray(zmaps.CHANNELS), "lo": np.float64(self.px_lo), "hi": np.float64(self.px_hi),
                                "nbins": np.int64(self.px_bins), "hist": hist.cpu().numpy().astype(np.int64),
                                "thresholds": np.asarray(self.px_thresholds, dtype=np.float32),
                                "counts": rows[:, :-1].reshape(-1, 2, K, 3).astype(np.int32), "mask_pixels": rows[:, -1],
                                "sigma": np.float64(self.z_sigma)}

    def _collect_maps(self, loader, results, t_values, local_ids, gathered_ids, name_of, maps_all):
        """The maps of every rank's images in the CSV's order of first appearance (rank 0 keeps them: ``last_maps``)."""
        got = self._gather_map_rows("--anomaly_maps 1", loader, results, local_ids, gathered_ids, name_of, maps_all)
        if got is not None:
            stems, maps = got
            self.last_maps = {"filename": np.asarray(stems), "t": np.asarray(t_values, dtype=np.int64),
                              "lpips_map": np.ascontiguousarray(maps[:, 0]), "mse_map": np.ascontiguousarray(maps[:, 1])}

    def _gather_map_rows(self, flag, loader, results, local_ids, gathered_ids, name_of, maps_all):
        """Per-image rows [n, 2, H, W] of every rank, in the CSV's order of first appearance: (filenames, rows) on rank 0,
        None on the others."""
        if self.ddp and hasattr(loader, "all_names") and len(loader.all_names) < self.world:
            # (every rank sees the same list and raises alike: a rank without an image does not know the maps' extent)
            raise ValueError(f"{flag}: {len(loader.all_names)} images over {self.world} ranks leave a rank without "
                             f"an image, and the maps' extent comes from the images")
        if not maps_all:
            raise ValueError(f"{flag}: this rank scored no batch (--drop_last on a short shard?): no maps to gather")
        maps = torch.cat(list(maps_all), dim=0)
        map_ids = gathered_ids
        if self.ddp:
            n_total = len(loader.all_names) if hasattr(loader, "all_names") else None
            n_max = -(-n_total // self.world) if n_total is not None else None
            gids, maps, _ = gather_rows(local_ids.to(self.device), maps.to(self.device), n_max)
            map_ids, maps = gids.cpu().tolist(), maps.cpu()
        if self.rank != 0:
            return None
        stems, picks = map_rows_in_csv_order(results, map_ids, name_of)
        return stems, maps[torch.as_tensor(picks, dtype=torch.long)].numpy()

    def _write(self, results_list, name):
        if self.rank == 0:
            pd.DataFrame(results_list).to_csv(self.out_dir / f"results_{name}.csv")
            if self.anomaly_maps and self.last_maps is not None:  # filename [N], t [n_t], lpips_map / mse_map fp32 [N, H, W]
                np.savez(self.out_dir / f"maps_{name}.npz", **self.last_maps)
            if self.anomaly_z_maps and name == "val" and self.last_map_stats is not None:
                # t [n_t], n, mean / std fp32 [n_t, 2, H, W] (the un-floored std), channels, rel_floor
                self.last_map_stats[0].save(self.out_dir / zmaps.STATS_FILE, self.last_map_stats[1], self.z_std_floor)
            if self.anomaly_z_maps and self.last_zmaps is not None:
                # filename [N], t [n_t], z_lpips_map / z_mse_map fp32 [N, H, W], sigma, rel_floor
                np.savez(self.out_dir / f"zmaps_{name}.npz", **self.last_zmaps)
            if self.pixel_metrics and self.last_pixels is not None:
                # filename [N], t, channels, lo, hi, nbins, hist int64 [2, 2, nbins + 1], thresholds [K], counts int32 [N, 2, K, 3],
                # mask_pixels [N], sigma
                np.savez(self.out_dir / f"pixels_{name}.npz", **self.last_pixels)
            if self.pixel_regions and self.last_regions is not None:
                # filename [N], t, channels, lo, hi, nbins, connectivity, regions int32 [N], overlap float64 [2, nbins + 1],
                # thresholds [K], components int32 [N, 2, K, 3] = (hit, pred, false_pred), sigma
                np.savez(self.out_dir / f"regions_{name}.npz", **self.last_regions)
            if self.px_calibrate and name == "val" and self.last_calibration is not None:
                # t [n_t], n, fpr [F], bin int64 [2, F], thresholds fp32 [2, F], hist int64 [2, nbins + 1], lo, hi, nbins, sigma,
                # rel_floor, channels
                np.savez(self.out_dir / pixel_metrics.CALIBRATION_FILE, **self.last_calibration)
            if self.px_calibrate and self.last_calibrated is not None:
                # filename [N], fpr [F], thresholds fp32 [2, F], counts int32 [N, 2, F, 3] = (TP, FP, FN), with --pixel_regions 1
                # components int32 [N, 2, F, 3] = (hit, pred, false_pred)
                np.savez(self.out_dir / f"calibrated_{name}.npz", **self.last_calibrated)
        self.last_maps = self.last_zmaps = self.last_pixels = self.last_regions = self.last_calibrated = None

    def reconstruct(self, args):
        if bool(args.run_val):
            self._write(self.get_scores(self.val_loader, "val", args.inference_skip_factor), "val")
        if bool(args.run_in):
            self._write(self.get_scores(self.in_loader, "in", args.inference_skip_factor), "in")
        if bool(args.run_out):
            for k, out in enumerate(args.out_ids.split(",")):
                print(out)
                masks = {"mask_ids": self.px_masks[k]} if self.pixel_metrics and self.px_masks[k] else {}
                flips = {}
                if "vflip" in out:
                    out = out.replace("_vflip", "")
                    flips, suffix = {"add_vflip": True}, "_vflip"
                elif "hflip" in out:
                    out = out.replace("_hflip", "")
                    flips, suffix = {"add_hflip": True}, "_hflip"
                else:
                    suffix = ""
                out_loader = get_data_loader(out, first_n=int(args.first_n) if args.first_n else args.first_n,
                                             **flips, **masks, **self._loader_args)
                dataset_name = dataset_stem(out) + suffix
                self._write(self.get_scores(out_loader, "out", args.inference_skip_factor), dataset_name)


def dataset_stem(ids: str) -> str:
    """Path(out).stem.split("_")[0] of the reference (reconstruct.py:287,308,327); synthetic
    specs are named by their kind."""
    if str(ids).startswith("synthetic:"):
        parts = str(ids).split(":")
        name = parts[1]
        for p in parts[2:]:
            if p.startswith("name="):
                name = p[5:]
        return name
    return Path(ids).stem.split("_")[0]
