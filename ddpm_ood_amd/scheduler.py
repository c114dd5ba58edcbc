"""``PNDMScheduler`` / ``DDPMScheduler`` with the MONAI-Generative call surface.

Drop-in for ``generative.networks.schedulers.PNDMScheduler`` as exercised by the reference:
  ctor kwargs                          /root/reference/src/trainers/reconstruct.py:98-105
  readable + assignable tables         /root/reference/src/trainers/reconstruct.py:106-117
  set_timesteps / timesteps            /root/reference/src/trainers/reconstruct.py:118-120,149
  add_noise(original_samples=, noise=, timesteps=)   :143-147
  step(model_output, timestep, sample) -> (prev_sample, None)   :155-157
Host side: the schedule tables and the ~15 scalar operations of a PLMS step stay on the
host as fp32 torch CPU scalars (bit-identical to what the reference computes with 0-d
tensors); device side: ONE fused kernel per step (ddpm_plms_step_f32) instead of 2-6
full-tensor ATen launches, and one for add_noise.  PLMS state (ets, counter, cur_sample)
persists across calls until set_timesteps, exactly like the reference (quirk Q3).
``DDPMScheduler.set_timesteps`` / ``.step`` are the ancestral sampler of the same package (one fused kernel per step as well,
noise drawn inside it); the reference reaches it through ``DiffusionInferer.sample`` in its validation epoch.
"""

from __future__ import annotations

import numpy as np
import torch

from . import ops

_ALIASES = {
    "linear": "linear_beta", "linear_beta": "linear_beta",
    "scaled_linear": "scaled_linear_beta", "scaled_linear_beta": "scaled_linear_beta",
    "sigmoid": "sigmoid_beta", "sigmoid_beta": "sigmoid_beta",
    "cosine": "cosine",
}


def noise_schedule(schedule: str, num_train_timesteps: int, beta_start: float = 1e-4, beta_end: float = 2e-2,
                   sig_range: float = 6.0, s: float = 8e-3) -> torch.Tensor:
    name = _ALIASES.get(schedule)
    if name is None:
        raise ValueError(f"Unknown beta schedule {schedule}")
    T = num_train_timesteps
    if name == "linear_beta":
        return torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
    if name == "scaled_linear_beta":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    if name == "sigmoid_beta":
        return torch.sigmoid(torch.linspace(-sig_range, sig_range, T)) * (beta_end - beta_start) + beta_start
    x = torch.linspace(0, T, T + 1)
    ac = torch.cos(((x / T) + s) / (1 + s) * torch.pi * 0.5) ** 2
    ac = ac / ac[0].item()
    return 1.0 - torch.clip(ac[1:] / ac[:-1], 0.0001, 0.9999)


class Scheduler:
    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", **schedule_args):
        self.num_train_timesteps = num_train_timesteps
        self.betas = noise_schedule(schedule, num_train_timesteps, **schedule_args)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor,
                  b_scale: float = 1.0) -> torch.Tensor:
        """sqrt(abar_t) * x0 + sqrt(1 - abar_t) * noise.  ``b_scale`` lets the trainer fold the
        reference's ``images * self.b_scale`` (reconstruct.py:144) into the same kernel."""
        ac = self.alphas_cumprod.to(dtype=torch.float32, device="cpu")
        t = timesteps.to("cpu").long()
        sa = (ac[t] ** 0.5).numpy()
        sb = ((1 - ac[t]) ** 0.5).numpy()
        return ops.add_noise(original_samples, noise, sa, sb, b_scale)


SAMPLING_KEY_TAG = 1 << 63
STREAMS_PER_ROW = 65536


def sampling_key(seed: int) -> int:
    """Philox key of the sampling noise: bit 63 set over the low 63 bits of ``seed``.  The training step keys its noise with
    ``seed * 7919 + rank`` (train.py), which stays below 2^63 for every seed below 1.1e15, so no (key, stream) pair of a sampling
    run can coincide with one of a training run, whatever the two seeds are."""
    return SAMPLING_KEY_TAG | (int(seed) & (SAMPLING_KEY_TAG - 1))


def sampling_streams(row_ids, timestep: int):
    """Philox stream id of row b at step t: ``row_ids[b] * 65536 + t`` (x_T: t = num_train_timesteps).  A row's noise depends on
    its own id and the step only -- not on the batch it rides in, its position in it, or the rank that draws it."""
    t = int(timestep)
    if not 0 <= t < STREAMS_PER_ROW:
        raise ValueError(f"timestep {t} outside [0, {STREAMS_PER_ROW})")
    return [int(r) * STREAMS_PER_ROW + t for r in row_ids]


LIKELIHOOD_STREAM = STREAMS_PER_ROW - 1


def likelihood_streams(row_ids):
    """Philox stream id of image b's noise in the variational bound: ``row_ids[b] * 65536 + 65535`` under ``sampling_key(seed)``
    -- ONE noise per image, shared by every timestep.  ``sampling_streams`` uses t <= num_train_timesteps (x_T: t = T) and the
    bound rejects num_train_timesteps >= 65535, so no sampling step, x_T draw or (by the key's bit 63) training step reads the
    same (key, stream) pair."""
    return [int(r) * STREAMS_PER_ROW + LIKELIHOOD_STREAM for r in row_ids]


class DDPMScheduler(Scheduler):
    """``generative.networks.schedulers.DDPMScheduler``: constructor, ``add_noise``, ``set_timesteps`` and the ancestral
    ``step`` (Ho et al. 2020, eq. 7 and algorithm 2), the latter as ONE fused launch (ops.ancestral_step) with the noise drawn
    inside the kernel.

    Quirk Q22 (kept, it is the package's behaviour): ``step`` takes abar_{t-1} from ``alphas_cumprod[t - 1]`` (1 at t = 0)
    WHATEVER ``set_timesteps`` chose -- with 25 inference steps the update at t = 960 still uses abar_959, not abar_920, so a
    shortened schedule is not the DDPM posterior of the strided chain.
    """

    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", variance_type: str = "fixed_small",
                 clip_sample: bool = True, prediction_type: str = "epsilon", **schedule_args):
        super().__init__(num_train_timesteps, schedule, **schedule_args)
        if variance_type in ("learned", "learned_range"):
            raise NotImplementedError(f"variance_type {variance_type}: learned variances are not built (the UNets here "
                                      f"predict one tensor)")
        if variance_type not in ("fixed_small", "fixed_large"):
            raise ValueError("Argument `variance_type` must be a member of `DDPMVarianceType`")
        if prediction_type not in ops.PREDICTION_TYPES:
            raise ValueError("Argument `prediction_type` must be a member of `DDPMPredictionType`")
        self.prediction_type = prediction_type
        self.variance_type = variance_type
        self.clip_sample = bool(clip_sample)
        self.num_inference_steps = None
        self._coef_cache = {}
        self._coef_tables = (None, None, None)
        self._vlb_cache = None  # (tables, (variance type, device), fp32 [T, 8] device table of the bound's coefficients)
        self._stream_table = None  # (row ids, device, int64 [T + 1, B] device tensor of stream ids)

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(
                f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.num_train_timesteps`:"
                f" {self.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.num_train_timesteps // self.num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].astype(np.int64)
        self.timesteps = torch.from_numpy(ts.copy())  # host tensor, as PNDMScheduler's

    def step_coefficients(self, timestep: int):
        """(sqrt(abar_t), sqrt(1 - abar_t), c0, ct, sigma) of one reverse step, evaluated in float64 from the tables as they are
        AT CALL TIME (snr_shift_tables reassigns them) and memoised per (t, table):
          c0 = sqrt(abar_{t-1}) beta_t / (1 - abar_t),  ct = sqrt(alpha_t) (1 - abar_{t-1}) / (1 - abar_t),
          sigma^2 = (1 - abar_{t-1}) / (1 - abar_t) beta_t floored at 1e-20 (fixed_small) or beta_t (fixed_large); sigma = 0 at
          t = 0 (the last step adds no noise).  abar_{t-1} = alphas_cumprod[t - 1], 1 at t = 0 (quirk Q22)."""
        t = int(timestep)
        tables = (self.alphas_cumprod, self.betas, self.alphas)
        if not all(a is b for a, b in zip(tables, self._coef_tables)):
            # the tables were reassigned: drop what was computed from the old ones, and hold the new ones so that no id() in a
            # live key can be reused by a later tensor
            self._coef_cache.clear()
            self._coef_tables = tables
        key = (t, id(self.alphas_cumprod), id(self.betas), id(self.alphas), self.variance_type)
        hit = self._coef_cache.get(key)
        if hit is not None:
            return hit
        if not 0 <= t < self.num_train_timesteps:
            raise ValueError(f"timestep {t} outside [0, {self.num_train_timesteps})")
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[t - 1]) if t > 0 else 1.0
        beta, alpha = float(self.betas[t]), float(self.alphas[t])
        c0 = a_p ** 0.5 * beta / (1.0 - a_t)
        ct = alpha ** 0.5 * (1.0 - a_p) / (1.0 - a_t)
        if t == 0:
            sigma = 0.0
        elif self.variance_type == "fixed_small":
            sigma = max((1.0 - a_p) / (1.0 - a_t) * beta, 1e-20) ** 0.5
        else:
            sigma = beta ** 0.5
        out = (a_t ** 0.5, (1.0 - a_t) ** 0.5, c0, ct, sigma)
        self._coef_cache[key] = out
        return out

    def _tables64(self):
        """(abar_t, abar_{t-1}, beta_t, alpha_t) as float64 arrays of the tables as they are now; abar_{t-1} = 1 at t = 0 (Q22)."""
        a_t = self.alphas_cumprod.double().numpy()
        a_p = np.concatenate([np.ones(1), a_t[:-1]])
        return a_t, a_p, self.betas.double().numpy(), self.alphas.double().numpy()

    def _get_variance(self, timestep: int) -> float:
        """The variance of p(x_{t-1} | x_t) (float64): (1 - abar_{t-1}) / (1 - abar_t) beta_t floored at 1e-20 (fixed_small, so
        1e-20 at t = 0) or beta_t (fixed_large)."""
        t = int(timestep)
        if not 0 <= t < self.num_train_timesteps:
            raise ValueError(f"timestep {t} outside [0, {self.num_train_timesteps})")
        return float(self.likelihood_coefficients(raw=True)[t, 4])

    def _get_mean(self, timestep: int, x_0: torch.Tensor, x_t: torch.Tensor) -> torch.Tensor:
        """c0 x_0 + ct x_t: the mean of q(x_{t-1} | x_t, x_0) for the true x_0, of p(x_{t-1} | x_t) for the predicted one.
        Plain tensor arithmetic in the inputs' dtype (a helper for callers and tests; the bound itself runs in
        ops.vlb_term_rows)."""
        _, _, c0, ct, _ = self.step_coefficients(int(timestep))
        return c0 * x_0 + ct * x_t

    def likelihood_coefficients(self, raw: bool = False) -> np.ndarray:
        """float64 [T, 6]: sqrt(abar_t), sqrt(1 - abar_t), c0, ct, 0.5 / var, var^-1/2 of every train timestep, from the tables
        as they are AT CALL TIME (snr_shift_tables reassigns them), with c0, ct, abar_{t-1} as in ``step_coefficients`` and var
        as in ``_get_variance``.  ``raw``: column 4 holds var itself and column 5 its logarithm."""
        a_t, a_p, beta, alpha = self._tables64()
        c0 = np.sqrt(a_p) * beta / (1.0 - a_t)
        ct = np.sqrt(alpha) * (1.0 - a_p) / (1.0 - a_t)
        var = np.maximum((1.0 - a_p) / (1.0 - a_t) * beta, 1e-20) if self.variance_type == "fixed_small" else beta.copy()
        last = (var, np.log(var)) if raw else (0.5 / var, np.exp(-0.5 * np.log(var)))
        return np.stack([np.sqrt(a_t), np.sqrt(1.0 - a_t), c0, ct, *last], axis=1)

    def likelihood_coefficients_device(self, device) -> torch.Tensor:
        """The fp32 [T, 8] device copy of ``likelihood_coefficients`` (ops.vlb_coef_table), cached per (tables, variance type,
        device); the held tables keep their id() from being reused."""
        tables = (self.alphas_cumprod, self.betas, self.alphas)
        key = (self.variance_type, str(torch.device(device)))
        hit = self._vlb_cache
        if hit is not None and hit[1] == key and all(a is b for a, b in zip(tables, hit[0])):
            return hit[2]
        dev = ops.vlb_coef_table(self.likelihood_coefficients(), device)
        self._vlb_cache = (tables, key, dev)
        return dev

    def _streams(self, row_ids, timestep: int, device) -> torch.Tensor:
        """The [B] device array of stream ids of this step: a row of a [T + 1, B] table uploaded once per (row ids, device),
        so that a step launches nothing besides its kernel."""
        ids = tuple(int(r) for r in row_ids)
        tab = self._stream_table
        if tab is None or tab[0] != ids or tab[1] != device:
            T = self.num_train_timesteps
            if any(r < 0 or r >= (1 << 47) for r in ids) or T >= STREAMS_PER_ROW:
                raise ValueError("row ids must lie in [0, 2^47) and num_train_timesteps below 65536")
            host = (torch.tensor(ids, dtype=torch.int64)[None, :] * STREAMS_PER_ROW
                    + torch.arange(T + 1, dtype=torch.int64)[:, None])
            tab = (ids, device, host.to(device))
            self._stream_table = tab
        return tab[2][int(timestep)]

    def initial_noise(self, shape, *, seed: int = 0, row_ids=None, device=None) -> torch.Tensor:
        """x_T: row b = the normals of stream ``row_ids[b] * 65536 + num_train_timesteps`` under ``sampling_key(seed)``."""
        ids = range(int(shape[0])) if row_ids is None else row_ids
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return ops.randn_rows(shape, sampling_key(seed), self._streams(ids, self.num_train_timesteps, device))

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, *, seed: int = 0, row_ids=None):
        """x_{t-1} ~ p(x_{t-1} | x_t): returns (prev_sample, pred_original_sample).

        The noise of row b is drawn in the kernel from Philox stream ``row_ids[b] * 65536 + t`` (``row_ids`` defaults to
        0 .. B - 1) under the key ``sampling_key(seed)`` = 2^63 | seed: disjoint from the training step's keys
        ``seed * 7919 + rank`` < 2^63, so sampling never replays training noise.  ``ops.randn_rows`` with the same key and
        stream ids returns exactly the z this call adds."""
        t = int(timestep)
        sa, sb, c0, ct, sigma = self.step_coefficients(t)
        ids = range(sample.shape[0]) if row_ids is None else row_ids
        streams = self._streams(ids, t, sample.device) if sigma != 0.0 else None
        return ops.ancestral_step(sample, model_output, sqrt_ac=sa, sqrt_1m_ac=sb, c0=c0, ct=ct, sigma=sigma,
                                  seed=sampling_key(seed), row_streams=streams, prediction_type=self.prediction_type,
                                  clip_sample=self.clip_sample)


class PNDMScheduler(Scheduler):
    def __init__(self, num_train_timesteps: int = 1000, schedule: str = "linear_beta", skip_prk_steps: bool = False,
                 set_alpha_to_one: bool = False, prediction_type: str = "epsilon", steps_offset: int = 0,
                 timestep_list: str = "monai", **schedule_args):
        super().__init__(num_train_timesteps, schedule, **schedule_args)
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError("Argument `prediction_type` must be a member of PNDMPredictionType")
        if not skip_prk_steps:
            raise NotImplementedError("the reconstruction path constructs PNDMScheduler(skip_prk_steps=True) only")
        if timestep_list not in ("monai", "diffusers"):
            raise ValueError("timestep_list must be 'monai' or 'diffusers'")
        self.prediction_type = prediction_type
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        self.skip_prk_steps = skip_prk_steps
        self.steps_offset = steps_offset
        self.timestep_list = timestep_list  # 100-entry (default) vs 101-entry list
        self._coef_cache = {}
        self._coef_table = None
        self.cur_model_output = 0
        self.counter = 0
        self.cur_sample = None
        self.ets: list = []
        self.set_timesteps(num_train_timesteps)

    def set_timesteps(self, num_inference_steps: int, device=None) -> None:
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError(
                f"`num_inference_steps`: {num_inference_steps} cannot be larger than `self.num_train_timesteps`:"
                f" {self.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.num_train_timesteps // self.num_inference_steps
        ts = (np.arange(0, num_inference_steps) * step_ratio).round().astype(np.int64)
        ts += self.steps_offset
        if self.timestep_list == "diffusers":
            plms = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].copy()
        else:
            plms = ts[::-1].copy()
        self.timesteps = torch.from_numpy(plms.astype(np.int64))  # host tensor: supports reversed(), masks, iteration
        # the PLMS update steps by num_train_timesteps // (requested steps): the 101-entry diffusers list repeats
        # one timestep, it does not change the ratio (diffusers keeps the requested count for it)
        self._step_ratio = step_ratio
        self.num_inference_steps = len(self.timesteps)
        self.reset()

    def reset(self) -> None:
        """Forget the PLMS history (it belongs to one trajectory); the timestep list stays as set_timesteps left it."""
        self.ets = []
        self.counter = 0
        self.cur_sample = None

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor):
        return self.step_plms(model_output, int(timestep), sample), None

    def plms_coefficients(self, timestep: int, prev_timestep: int):
        """fp32 scalars of _get_prev_sample, computed with the same 0-d torch CPU ops as the reference (memoised per
        (timestep, prev_timestep, table): ~70 us of 0-d tensor arithmetic otherwise, on every PLMS step)."""
        if self.alphas_cumprod is not self._coef_table:  # reassigned (snr_shift_tables): the old entries are stale, and the
            self._coef_cache.clear()                     # held table keeps its id() from being reused
            self._coef_table = self.alphas_cumprod
        key = (timestep, prev_timestep, id(self.alphas_cumprod))
        hit = self._coef_cache.get(key)
        if hit is not None:
            return hit
        a_t = self.alphas_cumprod[timestep]
        a_p = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        b_p = 1 - a_p
        sample_coeff = (a_p / a_t) ** 0.5
        denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
        out = (float(sample_coeff), float(a_p - a_t), float(denom), float(a_t ** 0.5), float(b_t ** 0.5))
        self._coef_cache[key] = out
        return out

    def step_plms(self, model_output: torch.Tensor, timestep: int, sample: torch.Tensor) -> torch.Tensor:
        ratio = self._step_ratio
        prev_timestep = timestep - ratio
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + ratio

        if len(self.ets) == 1 and self.counter == 0:
            kind, es = 0, [model_output]
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            kind, es = 1, [model_output, self.ets[-1]]
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            kind, es = 2, [self.ets[-1], self.ets[-2]]
        elif len(self.ets) == 3:
            kind, es = 3, [self.ets[-1], self.ets[-2], self.ets[-3]]
        else:
            kind, es = 4, [self.ets[-1], self.ets[-2], self.ets[-3], self.ets[-4]]

        sc, ce, dn, va, vb = self.plms_coefficients(timestep, prev_timestep)
        prev = ops.plms_step(sample, es, kind, sc, ce, dn, v_prediction=self.prediction_type == "v_prediction",
                             v_a=va, v_b=vb)
        self.counter += 1
        return prev
