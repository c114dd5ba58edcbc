"""Float64 restatement of ``generative.inferers.DiffusionInferer.get_likelihood`` for one timestep, written
literally: both means through ``get_mean``, both log-variances, the KL of two Gaussians with its ``-1 + 0 + exp(0)``, and the
discretised-Gaussian decoder.  The tests of the likelihood path compare the kernels and the scheduler with THIS, not with a
rearranged form.  Everything is torch float64 on the CPU; the tables are the scheduler's fp32 tables widened to float64, which is
what ``DDPMScheduler.likelihood_coefficients`` reads.
"""

import math

import torch


class Tables:
    def __init__(self, scheduler):
        self.betas = scheduler.betas.double()
        self.alphas = scheduler.alphas.double()
        self.alphas_cumprod = scheduler.alphas_cumprod.double()
        self.variance_type = scheduler.variance_type
        self.prediction_type = scheduler.prediction_type
        self.clip_sample = scheduler.clip_sample


def _alpha_prods(tab, t):
    a_t = tab.alphas_cumprod[t]
    a_p = tab.alphas_cumprod[t - 1] if t > 0 else torch.tensor(1.0, dtype=torch.float64)
    return a_t, a_p


def get_mean(tab, t, x_0, x_t):
    a_t, a_p = _alpha_prods(tab, t)
    c0 = a_p.sqrt() * tab.betas[t] / (1 - a_t)
    ct = tab.alphas[t].sqrt() * (1 - a_p) / (1 - a_t)
    return c0 * x_0 + ct * x_t


def get_variance(tab, t):
    a_t, a_p = _alpha_prods(tab, t)
    variance = (1 - a_p) / (1 - a_t) * tab.betas[t]
    if tab.variance_type == "fixed_small":
        return torch.clamp(variance, min=1e-20)
    assert tab.variance_type == "fixed_large"
    return tab.betas[t]


def add_noise(tab, t, x0, noise):
    a_t = tab.alphas_cumprod[t]
    return a_t.sqrt() * x0.double() + (1 - a_t).sqrt() * noise.double()


def predict_x0(tab, t, x_t, out):
    a_t = tab.alphas_cumprod[t]
    if tab.prediction_type == "epsilon":
        p = (x_t - (1 - a_t).sqrt() * out) / a_t.sqrt()
    elif tab.prediction_type == "v_prediction":
        p = a_t.sqrt() * x_t - (1 - a_t).sqrt() * out
    else:
        p = out
    return torch.clamp(p, -1, 1) if tab.clip_sample else p


def _approx_standard_normal_cdf(x):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3))))


def discretised_gaussian_log_likelihood(inputs, means, log_scales, bin_width):
    centered_x = inputs - means
    inv_stdv = torch.exp(-log_scales)
    cdf_plus = _approx_standard_normal_cdf(inv_stdv * (centered_x + bin_width / 2))
    cdf_min = _approx_standard_normal_cdf(inv_stdv * (centered_x - bin_width / 2))
    log_cdf_plus = torch.log(cdf_plus.clamp(min=1e-12))
    log_one_minus_cdf_min = torch.log((1.0 - cdf_min).clamp(min=1e-12))
    cdf_delta = cdf_plus - cdf_min
    return torch.where(inputs < -0.999, log_cdf_plus,
                       torch.where(inputs > 0.999, log_one_minus_cdf_min, torch.log(cdf_delta.clamp(min=1e-12))))


def kl_map(tab, t, x0, x_t, out, bin_width=1.0 / 255.0):
    """The per-element term of timestep t; returns (kl, x0 - pred_mean)."""
    x0, x_t, out = x0.double(), x_t.double(), out.double()
    pred_mean = get_mean(tab, t, predict_x0(tab, t, x_t, out), x_t)
    post_mean = get_mean(tab, t, x0, x_t)
    pred_log_variance = torch.log(get_variance(tab, t))
    post_log_variance = torch.log(get_variance(tab, t))
    if t > 0:
        kl = 0.5 * (-1.0 + pred_log_variance - post_log_variance + torch.exp(post_log_variance - pred_log_variance)
                    + (post_mean - pred_mean) ** 2 * torch.exp(-pred_log_variance))
    else:
        kl = -discretised_gaussian_log_likelihood(x0, pred_mean, 0.5 * pred_log_variance, bin_width)
    return kl, x0 - pred_mean


def term(tab, t, x0, x_t, out, bin_width=1.0 / 255.0):
    """mean over the non-batch dimensions of the per-element term: [B]."""
    kl, _ = kl_map(tab, t, x0, x_t, out, bin_width)
    return kl.reshape(kl.shape[0], -1).mean(dim=1)
