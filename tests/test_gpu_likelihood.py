"""-m gpu: the likelihood baseline -- the two row kernels against the float64 restatement of the package's
``get_likelihood`` (tests/likelihood_ref.py), answers that do not depend on the recalled spec, row independence bit for bit, a
float64 replay through the real UNet, the status word, memory bounds and likelihood.py end to end.

How the smooth branches are judged (t > 0, and t = 0 under fixed_large): the SAME formula is evaluated with fp32 torch
operations on the CPU (``_eval32``), and the kernel's error against float64 may be at most 4 times that evaluation's error plus
2^-20 relative.  The factor covers the summation order and the library's tanh / log against torch's; a wrong coefficient or
branch is off by O(1).  An error is max over the rows of [max over the row's elements of |got - ref|] / [max |ref| of the row]
(kl_map) or of |got - ref| / |ref| (term).  t = 0 under fixed_small is a step function (inv_s = 1e10: kl is 0 or -log 1e-12):
compared elementwise outside a band of 1e-5 around |x0 - pred_mean| = bin_width / 2, 40 times the 2.4e-7 fp32 rounding of x0hat;
at most 1 % of the elements may lie in the band.
"""

import json
import math
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import likelihood_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SCHED = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
SCHED_CLI = ["--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195"]
T = 1000
BIN = 1.0 / 255.0
BAND = 1e-5
FLOOR = 2.0 ** -20
ROW_SHAPES = [(1, 28, 28), (1, 32, 32), (3, 7, 7, 5), (128, 4, 4, 4)]
# bound of likelihood.py's terms between batch sizes and rank counts: 4 x the largest relative difference measured on the
# MI355X (7.13e-7, profiles/likelihood.md), for box-to-box spread; a permutation of images or a wrong noise stream differs by O(1)
LIK_REL = 2.9e-6


def _scheduler(variance_type="fixed_small", prediction_type="epsilon", clip_sample=True):
    from ddpm_ood_amd import DDPMScheduler

    return DDPMScheduler(T, variance_type=variance_type, prediction_type=prediction_type, clip_sample=clip_sample, **SCHED)


def _coef32(s):
    from ddpm_ood_amd import ops

    return ops.vlb_coef_table(s.likelihood_coefficients(), "cpu")


def make_rows(seed=0, R=37, N=3):
    """R rows over N images: repeated row_src, row_t from {0, 1, 2, T / 2, T - 1}, every value several times."""
    g = torch.Generator().manual_seed(seed)
    ts = [0, 1, 2, T // 2, T - 1]
    row_t = [ts[i % 5] for i in range(R)]
    row_t = [row_t[i] for i in torch.randperm(R, generator=g).tolist()]
    row_src = torch.randint(0, N, (R,), generator=g).tolist()
    return row_src, row_t


def make_images(shape, seed=0, N=3):
    """x0 in [-1, 1] with about 5 % of the elements at each end (the decoder's two edge branches), and the noise."""
    g = torch.Generator().manual_seed(1000 + seed)
    x0 = torch.rand((N,) + tuple(shape), generator=g) * 2 - 1
    edge = torch.rand(x0.shape, generator=g)
    x0 = torch.where(edge < 0.05, torch.full_like(x0, -1.0), torch.where(edge > 0.95, torch.full_like(x0, 1.0), x0))
    return x0.contiguous(), torch.randn(x0.shape, generator=g)


def make_outputs(s, x0, x_t, row_src, row_t, seed=0):
    """Model outputs [R, ...] (fp32) whose x0hat lies x0 + U(-3, 3) bin widths away on the t = 0 rows and x0 + 0.1 N(0, 1) on
    the others: the inverse of the prediction type's x0hat formula, in float64."""
    g = torch.Generator().manual_seed(2000 + seed)
    tab = ref.Tables(s)
    out = torch.empty_like(x_t)
    for r, (b, t) in enumerate(zip(row_src, row_t)):
        shape = x0[b].shape
        delta = (torch.rand(shape, generator=g, dtype=torch.float64) * 6 - 3) * BIN if t == 0 else \
            0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
        target = x0[b].double() + delta
        a_t = tab.alphas_cumprod[t]
        if s.prediction_type == "epsilon":
            o = (x_t[r].double() - a_t.sqrt() * target) / (1 - a_t).sqrt()
        elif s.prediction_type == "v_prediction":
            o = (a_t.sqrt() * x_t[r].double() - target) / (1 - a_t).sqrt()
        else:
            o = target
        out[r] = o.float()
    return out


def _eval32(c, t, x0, xt, o, prediction_type, clip, bin_width=BIN):
    """The kernel's formula in fp32 torch operations: c is the fp32 [T, 8] table."""
    sa, sb, c0, ct, half_inv_var, inv_s = (c[t, i] for i in range(6))
    if prediction_type == "epsilon":
        p = (xt - sb * o) / sa
    elif prediction_type == "v_prediction":
        p = sa * xt - sb * o
    else:
        p = o
    if clip:
        p = p.clamp(-1, 1)
    if t > 0:
        dm = c0 * (x0 - p)
        return half_inv_var * (dm * dm)
    half_bin = torch.tensor(0.5, dtype=torch.float32) * torch.tensor(bin_width, dtype=torch.float32)
    d = x0 - (c0 * p + ct * xt)

    def cdf(z):
        return 0.5 * (1.0 + torch.tanh(0.7978845608028654 * (z + 0.044715 * (z * z * z))))

    cp, cm = cdf(inv_s * (d + half_bin)), cdf(inv_s * (d - half_bin))
    pr = torch.where(x0 < -0.999, cp, torch.where(x0 > 0.999, 1.0 - cm, cp - cm))
    return -torch.log(pr.clamp(min=1e-12))


def _map_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


class _Judge:
    """Collects, per class of rows, the kernel's and the fp32 evaluation's errors against float64."""

    def __init__(self, what):
        self.what, self.k_map, self.e_map, self.k_term, self.e_term = what, 0.0, 0.0, 0.0, 0.0
        self.rows = 0

    def add(self, kl_k, kl_e, kl_ref, term_k, term_e, term_ref):
        self.rows += 1
        self.k_map, self.e_map = max(self.k_map, _map_err(kl_k, kl_ref)), max(self.e_map, _map_err(kl_e, kl_ref))
        self.k_term = max(self.k_term, abs(float(term_k) - term_ref) / abs(term_ref))
        self.e_term = max(self.e_term, abs(float(term_e) - term_ref) / abs(term_ref))

    def check(self):
        if not self.rows:
            return
        print(f"{self.what}: {self.rows} rows, kl_map error kernel {self.k_map:.3e} / fp32 torch {self.e_map:.3e}, "
              f"term error kernel {self.k_term:.3e} / fp32 torch {self.e_term:.3e}")
        assert self.k_map <= 4 * self.e_map + FLOOR, (self.what, self.k_map, self.e_map)
        assert self.k_term <= 4 * self.e_term + FLOOR, (self.what, self.k_term, self.e_term)


def judge_rows(s, what, x0, x_t, out, row_src, row_t, term_k, kl_k, bin_width=BIN):
    """Every row of one launch against the restatement, by the rules of the module docstring.  All tensors on the CPU; term_k /
    kl_k are the kernel's.  Returns the fraction of the fixed_small t = 0 elements inside the exclusion band."""
    tab, c = ref.Tables(s), _coef32(s)
    smooth, smooth0 = _Judge(f"{what} t > 0"), _Judge(f"{what} t = 0 smooth")
    band = total = 0
    for r, (b, t) in enumerate(zip(row_src, row_t)):
        kl_ref, d = ref.kl_map(tab, t, x0[b][None], x_t[r][None], out[r][None], bin_width)
        kl_ref, d = kl_ref[0], d[0]
        kl_e = _eval32(c, t, x0[b], x_t[r], out[r], s.prediction_type, s.clip_sample, bin_width)
        if t > 0 or s.variance_type == "fixed_large":
            (smooth if t > 0 else smooth0).add(kl_k[r], kl_e, kl_ref, term_k[r], kl_e.mean(), float(kl_ref.mean()))
            continue
        # the step function: elementwise outside the band, the term over the hybrid of restatement and kernel inside it
        inside = ((d.abs() - bin_width / 2).abs() <= BAND)
        band, total = band + int(inside.sum()), total + inside.numel()
        keep = ~inside
        assert set(torch.unique(kl_ref[keep]).tolist()) <= {0.0, -math.log(1e-12)}
        assert bool(((kl_k[r].double() - kl_ref).abs()[keep] <= FLOOR * kl_ref.abs()[keep]).all()), (what, r)
        hybrid = torch.where(inside, kl_k[r].double(), kl_ref)
        hybrid32 = torch.where(inside, kl_k[r], kl_ref.float())
        want = float(hybrid.mean())
        err_k, err_e = abs(float(term_k[r]) - want), abs(float(hybrid32.mean()) - want)
        assert err_k <= 4 * err_e + FLOOR * abs(want), (what, r, err_k, err_e)
    smooth.check()
    smooth0.check()
    return band / total if total else 0.0


# ---- 1. the kernels against float64 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64(device, shape, prediction_type):
    from ddpm_ood_amd import ops

    row_src, row_t = make_rows()
    x0, noise = make_images(shape)
    assert len(row_src) == 37 and set(row_t) == {0, 1, 2, T // 2, T - 1} and len(set(row_src)) == 3
    assert bool((x0 < -0.999).any()) and bool((x0 > 0.999).any())
    for variance_type in ("fixed_small", "fixed_large"):
        for clip in (False, True):
            s = _scheduler(variance_type, prediction_type, clip)
            coef = s.likelihood_coefficients_device(device)
            tab = ref.Tables(s)
            x_t = ops.vlb_noise_rows(x0.to(device), noise.to(device), row_src, row_t, coef).cpu()
            assert x_t.shape == (37,) + tuple(shape)
            for r, (b, t) in enumerate(zip(row_src, row_t)):
                a_t = tab.alphas_cumprod[t]
                a, n = a_t.sqrt() * x0[b].double(), (1 - a_t).sqrt() * noise[b].double()
                # three roundings plus the fp32 rounding of the two coefficients
                assert bool(((x_t[r].double() - (a + n)).abs() <= 4 * 2.0 ** -24 * (a.abs() + n.abs())).all()), (r, b, t)
            out = make_outputs(s, x0, x_t, row_src, row_t)
            term, kl = ops.vlb_term_rows(x0.to(device), x_t.to(device), out.to(device), row_src, row_t, coef,
                                         prediction_type=prediction_type, clip_sample=clip, bin_width=BIN, return_kl_map=True)
            alone = ops.vlb_term_rows(x0.to(device), x_t.to(device), out.to(device), row_src, row_t, coef,
                                      prediction_type=prediction_type, clip_sample=clip, bin_width=BIN)
            assert torch.equal(alone, term)  # kl_map changes nothing in term
            what = f"{shape} {prediction_type} {variance_type} clip={int(clip)}"
            frac = judge_rows(s, what, x0, x_t, out, row_src, row_t, term.cpu(), kl.cpu())
            if variance_type == "fixed_small":
                print(f"{what}: {frac * 100:.3f} % of the t = 0 elements inside the exclusion band")
                assert frac <= 0.01


# ---- 2. answers that do not depend on the recalled spec -------------------------------------------------------------------------

def test_known_answers_for_a_perfect_and_a_zero_model(device):
    from ddpm_ood_amd import DiffusionInferer, ops
    from ddpm_ood_amd.scheduler import likelihood_streams, sampling_key

    s = _scheduler(clip_sample=False)
    s.set_timesteps(20)
    steps = [int(t) for t in s.timesteps]
    x0, _ = make_images((1, 28, 28), seed=3, N=4)
    ids = [5, 6, 40, 41]
    noise = ops.randn_rows(tuple(x0.shape), sampling_key(7), likelihood_streams(ids), device=device)
    inf = DiffusionInferer(s)
    # a model that returns exactly the noise of each row (rows_per_forward = N: every forward holds the N images in order)
    total, terms = inf.get_likelihood(x0.to(device), lambda x, timesteps: noise, save_intermediates=True, seed=7, row_ids=ids)
    assert terms.shape == (20, 4) and steps[-1] == 0
    print(f"perfect model: largest t > 0 term {float(terms[:-1].max()):.3e}")
    assert float(terms[:-1].max()) <= 1e-10 and float(terms[:-1].min()) >= 0
    assert bool((terms[-1] == 0).all())  # the decoder term under fixed_small: every element inside its own bin
    # a model that returns zeros: x0 - x0hat = -(sb / sa) n
    total, terms = inf.get_likelihood(x0.to(device), lambda x, timesteps: torch.zeros_like(x), save_intermediates=True, seed=7,
                                      row_ids=ids)
    tab = s.likelihood_coefficients()
    c = _coef32(s)
    n64, n32, x32 = noise.cpu().double(), noise.cpu(), x0
    k_err = e_err = 0.0
    for i, t in enumerate(steps[:-1]):
        sa, sb, c0, _, half_inv_var, _ = tab[t]
        want = half_inv_var * c0 ** 2 * (sb / sa) ** 2 * (n64 ** 2).reshape(4, -1).mean(dim=1)
        x_t32 = c[t, 0] * x32 + c[t, 1] * n32
        got32 = _eval32(c, t, x32, x_t32, torch.zeros_like(x32), "epsilon", False).reshape(4, -1).mean(dim=1)
        k_err = max(k_err, float(((terms[i] - want).abs() / want).max()))
        e_err = max(e_err, float(((got32.double() - want).abs() / want).max()))
    print(f"zero model: term error kernel {k_err:.3e} / fp32 torch {e_err:.3e}")
    assert k_err <= 4 * e_err + FLOOR
    assert torch.allclose(total, terms.sum(dim=0), rtol=1e-14, atol=0)


# ---- 3. row independence ----------------------------------------------------------------------------------------------------------

def _elementwise_model(x, timesteps):
    return torch.tanh(0.7 * x) + 1e-3 * timesteps.to(torch.float32).reshape((-1,) + (1,) * (x.dim() - 1)) * x


def test_terms_do_not_depend_on_the_packing(device):
    from ddpm_ood_amd import DiffusionInferer

    s = _scheduler()
    s.set_timesteps(20)
    x0, _ = make_images((1, 16, 16), seed=4, N=8)
    x0 = x0.to(device)
    inf = DiffusionInferer(s)
    _, want = inf.get_likelihood(x0, _elementwise_model, save_intermediates=True, seed=2)
    assert want.shape == (20, 8) and want.dtype == torch.float64 and bool(torch.isfinite(want).all())
    for rows in (8, 16, 3, 160):
        total, got = inf.get_likelihood(x0, _elementwise_model, save_intermediates=True, seed=2, rows_per_forward=rows)
        assert torch.equal(got, want), rows
        assert torch.equal(total, want.sum(dim=0))
    halves = [inf.get_likelihood(x0[i: i + 4], _elementwise_model, save_intermediates=True, seed=2, row_ids=range(i, i + 4),
                                 rows_per_forward=16)[1] for i in (0, 4)]
    assert torch.equal(torch.cat(halves, dim=1), want)
    _, other = inf.get_likelihood(x0, _elementwise_model, save_intermediates=True, seed=3)
    assert not torch.equal(other, want) and float((other - want).abs().max()) > 1e-3
    assert torch.equal(inf.get_likelihood(x0, _elementwise_model, seed=2), want.sum(dim=0))  # without intermediates: total_kl


# ---- 4. float64 replay through the real UNet ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_unet(device):
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    hip = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    hip.load_state_dict(random_state_dict("small", 1, seed=1))
    return hip.to(device).eval()


@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
def test_real_unet_terms_match_a_float64_replay(device, small_unet, variance_type):
    from ddpm_ood_amd import DiffusionInferer, ops
    from ddpm_ood_amd.inferer import plan_rows
    from ddpm_ood_amd.scheduler import likelihood_streams, sampling_key

    s = _scheduler(variance_type)
    s.set_timesteps(20)
    steps = [int(t) for t in s.timesteps]
    x0, _ = make_images((1, 16, 16), seed=5, N=4)
    seen = []

    def recording(x, timesteps):
        out = small_unet(x, timesteps=timesteps)
        seen.append((x.clone(), timesteps.clone(), out.clone()))
        return out

    total, terms = DiffusionInferer(s).get_likelihood(x0.to(device), recording, save_intermediates=True, seed=9,
                                                      rows_per_forward=16)
    plan = plan_rows(4, steps, 16)
    assert len(seen) == len(plan) == 5 and terms.shape == (20, 4)
    noise = ops.randn_rows(tuple(x0.shape), sampling_key(9), likelihood_streams(range(4)), device=device).cpu()
    tab = ref.Tables(s)
    coef = s.likelihood_coefficients_device(device)
    flat = terms.reshape(-1)
    for (k, row_src, row_t), (x_t, ts, out) in zip(plan, seen):
        assert ts.dtype == torch.int64 and ts.cpu().tolist() == row_t
        x_t, out = x_t.cpu(), out.cpu()
        for r, (b, t) in enumerate(zip(row_src, row_t)):
            a_t = tab.alphas_cumprod[t]
            a, n = a_t.sqrt() * x0[b].double(), (1 - a_t).sqrt() * noise[b].double()
            assert bool(((x_t[r].double() - (a + n)).abs() <= 4 * 2.0 ** -24 * (a.abs() + n.abs())).all()), (k, r)
        # the same rows through the op, for the per-element values: its terms are the loop's, bit for bit
        term, kl = ops.vlb_term_rows(x0.to(device), x_t.to(device), out.to(device), row_src, row_t, coef,
                                     prediction_type="epsilon", clip_sample=True, bin_width=BIN, return_kl_map=True)
        assert torch.equal(term.cpu().double(), flat[k: k + len(row_src)])
        judge_rows(s, f"real UNet {variance_type} forward at {k}", x0, x_t, out, row_src, row_t, term.cpu(), kl.cpu())
    assert torch.allclose(total, terms.sum(dim=0), rtol=1e-14, atol=0) and bool(torch.isfinite(total).all())


# ---- 5. status word ---------------------------------------------------------------------------------------------------------------

def test_nan_model_output_sets_the_status_word_and_leaves_the_other_rows(device):
    from ddpm_ood_amd import _lib, ops

    s = _scheduler()
    coef = s.likelihood_coefficients_device(device)
    row_src, row_t = make_rows()
    x0, noise = make_images((1, 28, 28))
    x_t = ops.vlb_noise_rows(x0.to(device), noise.to(device), row_src, row_t, coef)
    out = make_outputs(s, x0, x_t.cpu(), row_src, row_t).to(device)
    _lib.status_read(clear=True)
    clean = ops.vlb_term_rows(x0.to(device), x_t, out, row_src, row_t, coef, bin_width=BIN)
    assert _lib.status_read(clear=True) == 0 and bool(torch.isfinite(clean).all())
    out[11, 0, 27, 27] = float("nan")
    dirty = ops.vlb_term_rows(x0.to(device), x_t, out, row_src, row_t, coef, bin_width=BIN)
    assert _lib.status_read(clear=True) == 1  # DDPM_STATUS_NONFINITE_EPS
    assert _lib.status_read(clear=True) == 0
    keep = [r for r in range(37) if r != 11]
    assert torch.equal(dirty[keep], clean[keep]) and not bool(torch.isfinite(dirty[11]))


def test_ops_refuse_rows_out_of_range(device):
    from ddpm_ood_amd import ops

    s = _scheduler()
    coef = s.likelihood_coefficients_device(device)
    x0 = torch.zeros(3, 1, 4, 4, device=device)
    for src, t in (([3], [0]), ([0], [T]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(ValueError):
            ops.vlb_noise_rows(x0, x0, src, t, coef)
        with pytest.raises(ValueError):
            ops.vlb_term_rows(x0, x0[:1], x0[:1], src, t, coef)


# ---- 6. memory bounds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_ops_stay_inside_their_buffers(device, shape, R):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    s = _scheduler()
    coef = _coef32(s)
    row_src, row_t = make_rows(R=R)
    x0, noise = make_images(shape)
    tab = ref.Tables(s)
    x_t = torch.stack([ref.add_noise(tab, t, x0[b], noise[b]).float() for b, t in zip(row_src, row_t)])
    out = make_outputs(s, x0, x_t, row_src, row_t)
    _bounds(device, dict(x0=(x0, True), noise=(noise, True), coef=(coef, True)),
            lambda t: ops.vlb_noise_rows(t["x0"], t["noise"], row_src, row_t, t["coef"]))
    for with_map in (False, True):
        _bounds(device, dict(x0=(x0, True), x_t=(x_t, True), out=(out, True), coef=(coef, True)),
                lambda t: ops.vlb_term_rows(t["x0"], t["x_t"], t["out"], row_src, row_t, t["coef"], bin_width=BIN,
                                            return_kl_map=with_map))  # noqa: B023
    if R == 37:
        # x0 four bytes off a 16-byte boundary: the scalar path, the bits of the aligned call
        padded = torch.cat([torch.zeros(1), x0.reshape(-1)])
        aligned = ops.vlb_term_rows(x0.to(device), x_t.to(device), out.to(device), row_src, row_t, coef.to(device), bin_width=BIN,
                                    return_kl_map=True)
        plain, _ = _bounds(device, dict(x0=(padded, True), x_t=(x_t, True), out=(out, True), coef=(coef, True)),
                           lambda t: ops.vlb_term_rows(t["x0"][1:].view(x0.shape), t["x_t"], t["out"], row_src, row_t, t["coef"],
                                                       bin_width=BIN, return_kl_map=True))
        assert torch.equal(plain.res[0], aligned[0]) and torch.equal(plain.res[1], aligned[1])
        _bounds(device, dict(x0=(padded, True), noise=(noise, True), coef=(coef, True)),
                lambda t: ops.vlb_noise_rows(t["x0"][1:].view(x0.shape), t["noise"], row_src, row_t, t["coef"]))


# ---- 7. likelihood.py -------------------------------------------------------------------------------------------------------------
# One baseline run (--batch_size 64, one rank) is shared by the cases below.  The runs of one process go through the CLI's parser
# and the trainer in this process (no interpreter start and no second GPU context per run); the two-rank case starts the script.

MODEL = "fashionmnist_lik"
FILES = {"val": 5, "in": 7, "noise": 6}


def _cli_argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1",
            "--validation_ids", "synthetic:blobs:n=5:seed=10", "--in_ids", "synthetic:blobs:n=7:seed=11",
            "--out_ids", "synthetic:noise:n=6:seed=12", *SCHED_CLI, "--num_inference_steps", "20", "--save_terms", "1",
            "--seed", "3", *extra]


def _cli_run(root, tag, *extra):
    """likelihood.py's parser and trainer on the checkpoint under `root`; the ood directory is kept as ood_<tag>."""
    import likelihood as cli
    from ddpm_ood_amd.likelihood import Likelihood

    args = cli.parse_args(_cli_argv(root, *extra))
    Likelihood(args).likelihood(args)
    return (root / MODEL / "ood").rename(root / MODEL / f"ood_{tag}")


@pytest.fixture(scope="module")
def cli_baseline(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("likelihood_cli")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    return root, _cli_run(root, "a", "--batch_size", "64")


def _rel_diff(a, b):
    """Largest relative difference of the t >= 1 terms ([N, n_t], the scheduler's order: t = 0 is the last column)."""
    a, b = a[:, :-1].astype(np.float64), b[:, :-1].astype(np.float64)
    return float(np.max(np.abs(a - b) / np.abs(a)))


def _compare_terms(a, other, what):
    """Same images in the same order, the t >= 1 terms within LIK_REL of the baseline's."""
    worst = 0.0
    for name in FILES:
        assert list(pd.read_csv(other / f"likelihood_{name}.csv")["filename"]) == list(pd.read_csv(a / f"likelihood_{name}.csv")["filename"])
        diff = _rel_diff(np.load(a / f"likelihood_terms_{name}.npy"), np.load(other / f"likelihood_terms_{name}.npy"))
        print(f"likelihood.py {name}: {what} vs --batch_size 64 on one rank: largest relative difference of a term {diff:.3e}")
        worst = max(worst, diff)
    print(f"{what}: largest relative difference {worst:.3e} (LIK_REL {LIK_REL})")
    assert LIK_REL <= 1e-3 and worst <= LIK_REL


def test_likelihood_cli(cli_baseline):
    import argparse

    from ddpm_ood_amd import ood

    root, a = cli_baseline
    for name, n in FILES.items():
        df = pd.read_csv(a / f"likelihood_{name}.csv")
        assert list(df.columns) == ["filename", "type", "nll", "bpd"] and len(df) == n
        assert set(df["type"]) == {"out" if name == "noise" else name} and df["filename"].nunique() == n
        assert np.isfinite(df["nll"]).all() and np.allclose(df["bpd"], df["nll"] / math.log(2.0), rtol=1e-12, atol=0)
        terms = np.load(a / f"likelihood_terms_{name}.npy")
        assert terms.shape == (n, 20) and terms.dtype == np.float32 and np.isfinite(terms).all()
        assert np.allclose(terms.astype(np.float64).sum(axis=1), df["nll"], rtol=1e-12, atol=0)
    assert not list(a.glob("results_*.csv"))
    b = _cli_run(root, "b", "--batch_size", "64")
    assert sorted(p.name for p in b.iterdir()) == sorted(p.name for p in a.iterdir()) and len(list(a.iterdir())) == 6
    for p in sorted(a.iterdir()):
        assert p.read_bytes() == (b / p.name).read_bytes(), p.name
    # another batch size: other forwards (the UNet dispatches by batch), the same images in the same order
    _compare_terms(a, _cli_run(root, "c", "--batch_size", "3"), "--batch_size 3")
    # the scoring stage reads the files (its command line: tests/test_likelihood_host.py)
    (root / MODEL / "ood").symlink_to(a, target_is_directory=True)
    try:
        res = ood.main_likelihood(argparse.Namespace(output_dir=str(root), model_name=MODEL), out_data=["noise"])
    finally:
        (root / MODEL / "ood").unlink()
    assert set(res) == {"noise"} and 0.0 <= res["noise"] <= 1.0


def test_two_ranks_on_one_gpu_write_the_same_likelihoods(cli_baseline):
    """likelihood.py started as 2 ranks (gloo rendezvous, both on cuda:0: tests/test_gpu_dist.py's hook): image i on rank i % 2,
    one gather, rank 0 writes in image order."""
    from test_gpu_dist import _launch_ranks

    root, a = cli_baseline
    _launch_ranks(2, [str(ROOT / "likelihood.py"), *_cli_argv(root, "--batch_size", "64")], root)
    _compare_terms(a, (root / MODEL / "ood").rename(root / MODEL / "ood_2ranks"), "2 ranks")


def test_likelihood_cli_missing_checkpoint(device, tmp_path):
    import likelihood as cli
    from ddpm_ood_amd.likelihood import Likelihood

    (tmp_path / "m").mkdir()
    args = cli.parse_args(["--output_dir", str(tmp_path), "--model_name", "m", "--is_grayscale", "1",
                           "--validation_ids", "synthetic:blobs:n=2", "--in_ids", "synthetic:blobs:n=2"])
    with pytest.raises(FileNotFoundError, match="Failed to find a saved model checkpoint"):
        Likelihood(args)


def test_latent_likelihood_through_a_vqvae_with_latent_pad(device, tmp_path):
    """48^3 volumes through a conditioned synthetic VQ-VAE: [128, 3, 3, 3] latents padded to 4^3, times b_scale, four timesteps."""
    import likelihood as cli
    from oracle.vqvae import VQVAE as OracleVQVAE
    from parity_util import VQ_README

    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.likelihood import Likelihood

    torch.manual_seed(3)
    vq = OracleVQVAE(**VQ_README).eval()
    vq_dir = tmp_path / "vqvae"
    vq_dir.mkdir()
    torch.save({"model_state_dict": synthetic.condition_vqvae_state_dict(vq.state_dict())}, vq_dir / "checkpoint.pth")
    json.dump(VQ_README, open(vq_dir / "vqvae_config.json", "w"))
    model = "decathlon_lik"
    (tmp_path / model).mkdir()
    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               tmp_path / model / "checkpoint.pth")
    ids = "synthetic:blobs3d:n=2:size=48:seed=5"
    args = cli.parse_args(["--output_dir", str(tmp_path), "--model_name", model, "--is_grayscale", "1", "--spatial_dimension", "3",
                           "--vqvae_checkpoint", str(vq_dir / "checkpoint.pth"), "--latent_pad", "(0,1,0,1,0,1)", "--b_scale", "0.5",
                           *SCHED_CLI, "--validation_ids", ids, "--in_ids", ids, "--run_val", "0", "--run_out", "0",
                           "--num_inference_steps", "4", "--batch_size", "8", "--save_terms", "1"])
    Likelihood(args).likelihood(args)
    df = pd.read_csv(tmp_path / model / "ood" / "likelihood_in.csv")
    terms = np.load(tmp_path / model / "ood" / "likelihood_terms_in.npy")
    assert len(df) == 2 and terms.shape == (2, 4) and np.isfinite(terms).all() and np.isfinite(df["nll"]).all()
    assert (terms[:, :-1] > 0).all()
