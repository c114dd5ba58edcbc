"""``DiffusionInferer``: the sampling loop of ``generative.inferers.DiffusionInferer.sample`` (the reference calls it at the
end of every validation epoch, src/trainers/ddpm_trainer.py:177-216).

The loop is host code; what it launches per step is one native UNet forward (``DiffusionModelUNet``: the engine, its small-batch
kernels and, under ``DDPM_UNET_GRAPH=1``, its graph replay) and ONE fused scheduler kernel: ``DDPMScheduler.step`` (ancestral,
noise drawn inside the kernel) or ``PNDMScheduler.step`` (PLMS, deterministic).  Timesteps live on the device, one cached
[B] int64 tensor per step value.
"""

from __future__ import annotations

import inspect

import numpy as np
import torch

from . import ops
from .scheduler import DDPMScheduler, likelihood_streams, sampling_key


def plan_rows(n_images: int, timesteps, rows_per_forward: int):
    """The (image, timestep) rows of a variational bound, packed into forwards of at most ``rows_per_forward`` rows.

    Pair (timesteps[i], image b) has the flat index i * n_images + b -- timestep-major, in the scheduler's order -- and forward
    k takes the flat indices [k * rows_per_forward, (k + 1) * rows_per_forward): every pair exactly once, every forward but
    the last full.  ``rows_per_forward == n_images`` is the package's loop: one timestep per forward.  Returns a list of
    (offset, row_src, row_t) with ``offset`` the flat index of the forward's first row."""
    n, rows = int(n_images), int(rows_per_forward)
    ts = [int(t) for t in timesteps]
    if n < 1 or rows < 1 or not ts:
        raise ValueError(f"plan_rows: n_images {n}, rows_per_forward {rows} and the timestep list must be non-empty")
    src = np.tile(np.arange(n, dtype=np.int64), len(ts))
    t = np.repeat(np.asarray(ts, dtype=np.int64), n)
    return [(k, src[k: k + rows].tolist(), t[k: k + rows].tolist()) for k in range(0, n * len(ts), rows)]


class DiffusionInferer:
    def __init__(self, scheduler=None):
        self.scheduler = scheduler
        self._ts_cache = {}

    def _timesteps_tensor(self, step: int, batch: int, device) -> torch.Tensor:
        key = (int(step), int(batch), str(device))
        t = self._ts_cache.get(key)
        if t is None:
            if len(self._ts_cache) > 4096:
                self._ts_cache.clear()
            t = torch.full((batch,), int(step), dtype=torch.int64, device=device)
            self._ts_cache[key] = t
        return t

    @torch.no_grad()
    def sample(self, input_noise: torch.Tensor, diffusion_model, scheduler=None, save_intermediates: bool = False,
               intermediate_steps: int = 100, verbose: bool = False, seed: int = 0, row_ids=None):
        """x_T -> x_0 over ``scheduler.timesteps``.  ``seed`` / ``row_ids`` address the noise of a stochastic scheduler
        (``DDPMScheduler.step``: row b of step t reads Philox stream ``row_ids[b] * 65536 + t``); a scheduler whose ``step``
        takes no seed (``PNDMScheduler``) is called without them.  Returns the sample, or (sample, intermediates) with
        ``save_intermediates`` -- an intermediate is kept after every step whose ``t % intermediate_steps == 0``."""
        scheduler = scheduler or self.scheduler
        if scheduler is None:
            raise ValueError("DiffusionInferer.sample: no scheduler")
        params = inspect.signature(scheduler.step).parameters
        kw = {}
        if "seed" in params:
            kw["seed"] = seed
        if "row_ids" in params:
            kw["row_ids"] = list(range(input_noise.shape[0])) if row_ids is None else list(row_ids)
        image = input_noise
        B = image.shape[0]
        intermediates = []
        steps = [int(t) for t in scheduler.timesteps]
        for i, t in enumerate(steps):
            model_output = diffusion_model(image, timesteps=self._timesteps_tensor(t, B, image.device))
            image, _ = scheduler.step(model_output, t, image, **kw)
            if verbose and (i % 100 == 0 or i == len(steps) - 1):
                print(f"sampling: step {i + 1} / {len(steps)} (t = {t})", flush=True)
            if save_intermediates and t % intermediate_steps == 0:
                intermediates.append(image)
        return (image, intermediates) if save_intermediates else image

    @torch.no_grad()
    def get_likelihood(self, inputs: torch.Tensor, diffusion_model, scheduler=None, save_intermediates: bool = False,
                       original_input_range=(0, 255), scaled_input_range=(0, 1), verbose: bool = False, *, seed: int = 0,
                       row_ids=None, rows_per_forward=None):
        """The DDPM variational bound of every image (``generative.inferers.DiffusionInferer.get_likelihood``):
        ``total_kl`` [N] -- the sum over ``scheduler.timesteps`` of the per-image mean of the KL between posterior and predicted
        step (t > 0) and of the discretised-Gaussian decoder NLL (t = 0) -- or (total_kl, terms [len(timesteps), N]) with
        ``save_intermediates``.  Both are float64 host tensors; the sum over t is taken on the host.

        One noise per image, shared by all timesteps: the normals of Philox stream ``row_ids[b] * 65536 + 65535`` under
        ``sampling_key(seed)`` (``row_ids`` defaults to 0 .. N - 1), so an image's terms depend on (model, seed, its id) alone.
        The T terms do not depend on each other, so ``rows_per_forward`` (default N: one timestep per forward, the package's
        loop) may pack several timesteps into one UNet forward (``plan_rows``).  Per forward: one noising launch, the model
        call ``diffusion_model(x_t, timesteps=int64[R])``, one term launch; one device-to-host copy at the end."""
        scheduler = scheduler or self.scheduler
        if scheduler is None:
            raise ValueError("DiffusionInferer.get_likelihood: no scheduler")
        if not isinstance(scheduler, DDPMScheduler):
            raise NotImplementedError(f"Likelihood computation is only compatible with DDPMScheduler, you are using "
                                      f"{scheduler.__class__.__name__}")
        if scheduler.num_train_timesteps >= 65535:
            raise ValueError("get_likelihood: num_train_timesteps must be below 65535 (stream 65535 of a row is its noise)")
        x0 = ops.require_device_f32(inputs, "inputs")
        N = int(x0.shape[0])
        ids = list(range(N)) if row_ids is None else [int(r) for r in row_ids]
        if len(ids) != N or any(r < 0 or r >= (1 << 47) for r in ids):
            raise ValueError("get_likelihood: row_ids must be N ids in [0, 2^47)")
        steps = [int(t) for t in scheduler.timesteps]
        rows = N if rows_per_forward is None else int(rows_per_forward)
        plan = plan_rows(N, steps, rows)
        bin_width = (float(scaled_input_range[1]) - float(scaled_input_range[0])) / (
            float(original_input_range[1]) - float(original_input_range[0]))
        dev = x0.device
        coef = scheduler.likelihood_coefficients_device(dev)
        noise = ops.randn_rows(tuple(x0.shape), sampling_key(seed), likelihood_streams(ids), device=dev)
        all_rows = ops.VlbRows(np.concatenate([p[1] for p in plan]), np.concatenate([p[2] for p in plan]), N,
                               scheduler.num_train_timesteps, dev)
        t_model = all_rows.t.to(torch.int64)  # the timesteps argument of every forward is a slice of this
        terms = torch.empty((len(steps) * N,), dtype=torch.float32, device=dev)
        x_t = {}
        for i, (k, src, _) in enumerate(plan):
            R = len(src)
            part = all_rows[k: k + R]
            buf = x_t.get(R)
            if buf is None:
                buf = x_t[R] = torch.empty((R,) + tuple(x0.shape[1:]), dtype=torch.float32, device=dev)
            ops.vlb_noise_rows(x0, noise, part, None, coef, out=buf)
            model_output = diffusion_model(buf, timesteps=t_model[k: k + R])
            ops.vlb_term_rows(x0, buf, model_output, part, None, coef, prediction_type=scheduler.prediction_type,
                              clip_sample=scheduler.clip_sample, bin_width=bin_width, out=terms[k: k + R])
            if verbose and (i % 100 == 0 or i == len(plan) - 1):
                print(f"likelihood: forward {i + 1} / {len(plan)}", flush=True)
        terms64 = terms.reshape(len(steps), N).cpu().double()  # the one device-to-host copy
        total_kl = terms64.sum(dim=0)
        return (total_kl, terms64) if save_intermediates else total_kl
