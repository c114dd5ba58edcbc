"""``DiffusionInferer``: the sampling loop of ``generative.inferers.DiffusionInferer.sample`` (the reference calls it at the
end of every validation epoch, src/trainers/ddpm_trainer.py:177-216).

The loop is host code; what it launches per step is one native UNet forward (``DiffusionModelUNet``: the engine, its small-batch
kernels and, under ``DDPM_UNET_GRAPH=1``, its graph replay) and ONE fused scheduler kernel: ``DDPMScheduler.step`` (ancestral,
noise drawn inside the kernel) or ``PNDMScheduler.step`` (PLMS, deterministic).  Timesteps live on the device, one cached
[B] int64 tensor per step value.
"""

from __future__ import annotations

import inspect

import torch


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
