"""Drawing samples from a trained model: ``Sampler`` (the trainer behind ``sample.py``) and the pieces the validation grids of
``train.DDPMTrainer.val_epoch`` share with it.

The reference draws a grid from pure noise at the end of every validation epoch (src/trainers/ddpm_trainer.py:177-216:
``inferer.sample`` over the 1000-step ``DDPMScheduler``, inverse latent pad, VQ-VAE decode, matplotlib figure to TensorBoard).
Here the loop is ``DiffusionInferer.sample`` over the native UNet and ONE fused scheduler kernel per step, the noise is addressed
per sample (sample i is a function of (checkpoint, seed, i): not of the batch size or the rank count, as ``trainer.image_noise``
is for reconstruction), and the figure is a PNG written with zlib next to the raw ``.npy``.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib, ops
from .data import write_png
from .inferer import DiffusionInferer
from .scheduler import DDPMScheduler, PNDMScheduler, sampling_key, sampling_streams
from .trainer import BaseTrainer, snr_shift_tables


def make_sampling_scheduler(kind: str, *, prediction_type: str, beta_schedule: str, beta_start: float, beta_end: float,
                            snr_shift: float = 1, num_inference_steps=None):
    """``ddpm``: the 1000-step ancestral sampler (``num_inference_steps`` shortens it, quirk Q22 applies);
    ``pndm``: PLMS, 100 steps unless told otherwise -- deterministic given x_T."""
    kw = dict(num_train_timesteps=1000, prediction_type=prediction_type, schedule=beta_schedule, beta_start=beta_start,
              beta_end=beta_end)
    if kind == "ddpm":
        s = DDPMScheduler(**kw)
    elif kind == "pndm":
        s = PNDMScheduler(skip_prk_steps=True, **kw)
    else:
        raise ValueError(f"unknown scheduler {kind} (ddpm or pndm)")
    if snr_shift != 1:
        snr_shift_tables(s, snr_shift)
    if num_inference_steps is None:
        num_inference_steps = 1000 if kind == "ddpm" else 100
    s.set_timesteps(int(num_inference_steps))
    return s


def draw_latents(model, scheduler, inferer: DiffusionInferer, indices, row_shape, seed: int, device, verbose: bool = False):
    """Latent samples of the global sample indices ``indices``: x_T of row b is the Philox stream
    ``indices[b] * 65536 + num_train_timesteps`` under ``sampling_key(seed)``, every later draw stream ``indices[b] * 65536 + t``."""
    indices = [int(i) for i in indices]
    streams = sampling_streams(indices, scheduler.num_train_timesteps)
    x = ops.randn_rows((len(indices),) + tuple(row_shape), sampling_key(seed), streams, device=device)
    if hasattr(scheduler, "reset"):  # PLMS history belongs to one trajectory
        scheduler.reset()
    return inferer.sample(x, model, scheduler, seed=seed, row_ids=indices, verbose=verbose)


def decode_latents(latents, vqvae_model, inverse_latent_pad=None, b_scale: float = 1.0):
    """Inverse latent pad, stage-1 decode, / b_scale, clamp to [0, 1] (what the reconstruction path does before it scores)."""
    if inverse_latent_pad is not None:
        latents = F.pad(input=latents, pad=inverse_latent_pad, mode="constant", value=0).contiguous()
    x = vqvae_model.decode_stage_2_outputs(latents.contiguous()).float()
    return (x / b_scale).clamp_(0, 1)


def sample_grid(samples: np.ndarray) -> np.ndarray:
    """uint8 picture of [N, C, H, W] samples (a near-square tiling, row-major: 2 x 4 for the 8 validation samples, 2 x 2 for 4) or
    of [N, C, H, W, D] volumes (one row per volume, the slices at 0.25 / 0.5 / 0.75 of the last axis: the reference's figure).
    C = 1 gives a greyscale picture [rows, cols], C = 3 an RGB one; other channel counts show channel 0."""
    a = np.asarray(samples, dtype=np.float32)
    if a.ndim == 5:
        cuts = [int(r * a.shape[4]) for r in (0.25, 0.5, 0.75)]
        tiles = [[a[i, :, :, :, c] for c in cuts] for i in range(a.shape[0])]
    elif a.ndim == 4:
        n = a.shape[0]
        rows = max(1, int(math.floor(math.sqrt(n))))
        cols = -(-n // rows)  # (a ragged last row is padded with black tiles)
        blank = np.zeros_like(a[0])
        tiles = [[a[r * cols + c] if r * cols + c < n else blank for c in range(cols)] for r in range(rows)]
    else:
        raise ValueError(f"sample_grid: expected [N, C, H, W] or [N, C, H, W, D], got {a.shape}")
    pic = np.concatenate([np.concatenate(row, axis=2) for row in tiles], axis=1)  # [C, rows * H, cols * W]
    pic = np.clip(np.rint(pic * 255.0), 0, 255).astype(np.uint8)
    return np.transpose(pic, (1, 2, 0)) if pic.shape[0] == 3 else pic[0]


def write_samples(out_dir, stem: str, samples: np.ndarray) -> None:
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    np.save(out_dir / f"{stem}.npy", np.ascontiguousarray(samples, dtype=np.float32))
    write_png(out_dir / f"{stem}.png", sample_grid(samples))


def gather_samples(ids: torch.Tensor, samples: torch.Tensor, n_max: int):
    """ONE all_gather of every rank's samples, the pattern of ``trainer.gather_scores``: a dense [n_max, 1 + numel] fp32 payload
    per rank with the sample index in column 0 (-1 on the padding rows; exact below 2^24), static capacity n_max =
    ceil(N / world).  Returns (ids, samples) of all ranks ordered by sample index."""
    if not dist.is_initialized():
        order = torch.argsort(ids)
        return ids[order], samples[order]
    world = dist.get_world_size()
    if ids.shape[0] > n_max:
        raise ValueError(f"gather_samples: shard of {ids.shape[0]} rows does not fit the static capacity {n_max}")
    if ids.numel() and int(ids.max()) >= 1 << 24:
        raise ValueError("gather_samples: sample index is not exact in the fp32 payload (must be < 2^24)")
    row_shape = tuple(samples.shape[1:])
    numel = int(np.prod(row_shape))
    dev = samples.device
    payload = torch.full((n_max, 1 + numel), -1.0, dtype=torch.float32, device=dev)
    payload[: ids.shape[0], 0] = ids.to(torch.float32)
    payload[: ids.shape[0], 1:] = samples.reshape(ids.shape[0], numel)
    if dist.get_backend() == "gloo" and payload.is_cuda:  # test hook (2 ranks on one GPU): gloo moves host memory
        payload = payload.cpu()
    out = torch.empty((world * n_max, 1 + numel), dtype=torch.float32, device=payload.device)
    dist.all_gather_into_tensor(out, payload)
    out = out.to(dev)
    out = out[out[:, 0] >= 0]
    out = out[torch.argsort(out[:, 0])]
    return out[:, 0].to(torch.int64), out[:, 1:].reshape((-1,) + row_shape)


class Sampler(BaseTrainer):
    """``sample.py``: loads the run's checkpoint like the other trainers and draws ``--num_samples`` images from pure noise."""

    def __init__(self, args):
        args.simplex_noise = 0  # (BaseTrainer reads it; sampling draws Gaussian noise)
        super().__init__(args)
        if not self.found_checkpoint:
            raise FileNotFoundError(f"Failed to find a saved model checkpoint in {self.run_dir}.")
        if not self.image_size:
            raise ValueError("--image_size is required: sampling reads no dataset to take the shape from")
        self.seed = int(args.seed)
        self.num_samples = int(args.num_samples)
        self.batch_size = int(args.batch_size)
        if self.num_samples < 1 or self.batch_size < 1:
            raise ValueError("--num_samples and --batch_size must be positive")
        self.scheduler_kind = args.scheduler
        self.num_inference_steps = args.num_inference_steps
        self.out_dir = Path(args.out) if args.out else self.run_dir / "samples"
        self.image_channels = 1 if args.is_grayscale else 3
        self.verbose = bool(getattr(args, "verbose", 0))
        self.inferer = DiffusionInferer()
        self.last_stats = {}

    def latent_shape(self):
        """Shape of one latent: what stage 1 makes of a zero image of the run's size, plus the latent pad."""
        z = torch.zeros((1, self.image_channels) + (self.image_size,) * self.spatial_dimension, device=self.device)
        lat = self.vqvae_model.encode_stage_2_inputs(z).float()
        if self.do_latent_pad:
            lat = F.pad(input=lat, pad=self.latent_pad, mode="constant", value=0)
        return tuple(lat.shape[1:])

    def make_scheduler(self):
        return make_sampling_scheduler(self.scheduler_kind, prediction_type=self.prediction_type,
                                       beta_schedule=self.beta_schedule, beta_start=self.beta_start, beta_end=self.beta_end,
                                       snr_shift=self.snr_shift, num_inference_steps=self.num_inference_steps)

    @torch.no_grad()
    def sample_indices(self, indices):
        """Decoded samples [len(indices), C, ...] in [0, 1] of the given global sample indices, in batches of --batch_size."""
        self.model.eval()
        row_shape = self.latent_shape()
        sched = self.make_scheduler()
        inv = self.inverse_latent_pad if self.do_latent_pad else None
        out = []
        _lib.status_read(clear=True)
        for s in range(0, len(indices), self.batch_size):
            idx = indices[s: s + self.batch_size]
            lat = draw_latents(self.model, sched, self.inferer, idx, row_shape, self.seed, self.device, verbose=self.verbose)
            out.append(decode_latents(lat, self.vqvae_model, inv, self.b_scale))
            word = _lib.status_read(clear=True)
            if word:
                print(f"WARNING: {_lib.status_text(word)} while sampling indices {idx[0]} .. {idx[-1]}: these samples are not "
                      f"finite", file=sys.__stderr__, flush=True)
                self.last_stats["batches_nonfinite"] = self.last_stats.get("batches_nonfinite", 0) + 1
        if not out:
            shape = decode_latents(torch.zeros((1,) + row_shape, device=self.device), self.vqvae_model, inv, self.b_scale).shape
            return torch.zeros((0,) + tuple(shape[1:]), dtype=torch.float32, device=self.device)
        return torch.cat(out, dim=0)

    def sample(self):
        """Sample index i goes to rank i % world; one gather; rank 0 writes samples.npy / samples.png.  Returns the samples
        (every rank holds all of them after the gather)."""
        mine = list(range(self.rank, self.num_samples, self.world))
        x = self.sample_indices(mine)
        ids = torch.tensor(mine, dtype=torch.int64, device=self.device)
        ids, x = gather_samples(ids, x, -(-self.num_samples // self.world))
        assert ids.cpu().tolist() == list(range(self.num_samples))
        samples = x.cpu().numpy()
        if self.rank == 0:
            write_samples(self.out_dir, "samples", samples)
            print(f"Wrote {samples.shape[0]} samples of shape {samples.shape[1:]} to {self.out_dir}")
        return samples
