"""-m gpu: sampling -- the fused ancestral step against a float64 evaluation of its closed form, the row-addressed noise, the
inferer end to end against the CPU oracle (deterministic PLMS and a float64 replay of the stochastic chain), sample.py, two ranks
on one GPU, and the opt-in validation grids of the training loop."""

import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SCHED = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
SCHED_CLI = ["--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195"]
# the bound of the B = 128 25-chain test of tests/test_gpu_dispatch.py (raw results <= 2e-4 relative), for chains of 10 - 25 forwards
CHAIN_REL = 2e-4
EPS32 = 2.0 ** -23


def _rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| relative to the largest |ref| (a sample is an image around 0: an element-wise ratio has no meaning)"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- the kernel ---------------------------------------------------------------------------------------------------------

def _reference_step(x, out, z, coeffs, prediction_type, clip):
    """float64 closed form on the fp32 scalars the kernel receives.  Returns (prev, pred_original, L) where L is, per element,
    the largest magnitude among the addends and the partial sums of the formula at the scale of the result."""
    sa, sb, c0, ct, sigma = (float(np.float32(c)) for c in coeffs)
    x, out, z = x.double(), out.double(), z.double()
    if prediction_type == "epsilon":
        x0 = (x - sb * out) / sa
        parts = [c0 * x / sa, c0 * sb * out / sa]
    elif prediction_type == "v_prediction":
        x0 = sa * x - sb * out
        parts = [c0 * sa * x, c0 * sb * out]
    else:
        x0 = out
        parts = [c0 * out]
    parts.append(c0 * x0)  # (before the clamp: the largest the partial sum gets)
    if clip:
        x0 = x0.clamp(-1, 1)
    mean = c0 * x0 + ct * x
    prev = mean + sigma * z
    parts += [ct * x, mean, sigma * z, prev]
    L = torch.stack([p.abs() for p in parts]).max(dim=0).values
    return prev, x0, L


@pytest.mark.parametrize("row_shape", [(1, 28, 28), (1, 32, 32), (3, 64, 64), (3, 7, 7, 5)])
@pytest.mark.parametrize("prediction_type", ["epsilon", "v_prediction", "sample"])
def test_ancestral_step_against_float64(device, row_shape, prediction_type):
    """ops.ancestral_step on random x / model output, the noise replayed through ops.randn_rows, for clip on / off and
    t in {0, 1, 500, 999}; row lengths 784, 1024, 3*64*64 (16-byte path) and 3*7*7*5 = 735 (scalar path).

    Bound, per element: |err| <= 4 ulp(L), ulp(L) = 2^-23 L, L = the largest magnitude among the addends and partial sums of
    the formula.  Derivation: the longest form (epsilon) is eight fp32 operations -- sb*out, x - ., . / sa, c0 * ., ct * x, the
    sum of the two, sigma * z, the final sum (the library is built without FMA contraction, so each rounds once); the scalars and
    z are the SAME fp32 numbers on both sides; every operation is correctly rounded, so it adds at most half an ulp of its own
    result, i.e. <= 2^-24 |result| <= 0.5 ulp(L) once carried to the scale of the output (the factors c0 / sa etc. scale result
    and error alike).  8 x 0.5 = 4.  The clamp is monotone and 1-Lipschitz: it never enlarges an error.
    At t = 0 (sigma = 0) the output must be BIT-equal to the mean c0 * x0 + ct * x formed from the kernel's own x0: nothing was
    added to it.  (This cannot tell a skipped Philox block from an added 0 * z; that the block is skipped is the kernel's `noisy`
    branch, and what it saves is time, not bits.)"""
    from ddpm_ood_amd import DDPMScheduler, ops
    from ddpm_ood_amd.scheduler import sampling_key, sampling_streams

    B = 5
    g = torch.Generator().manual_seed(7 * sum(row_shape) + len(prediction_type))
    x = torch.randn((B,) + row_shape, generator=g)
    out = torch.randn((B,) + row_shape, generator=g)
    if prediction_type == "sample":
        out = out * 0.8  # an x0 prediction: on both sides of the clamp edges
    xd, od = x.to(device), out.to(device)
    row_ids = [3, 0, 11, 2 ** 20, 7]
    worst = 0.0
    for clip in (True, False):
        s = DDPMScheduler(num_train_timesteps=1000, prediction_type=prediction_type, clip_sample=clip, **SCHED)
        for t in (0, 1, 500, 999):
            prev, pred = s.step(od, t, xd, seed=5, row_ids=row_ids)
            coeffs = s.step_coefficients(t)
            z = ops.randn_rows(x.shape, sampling_key(5), sampling_streams(row_ids, t), device=device)
            ref_prev, ref_pred, L = _reference_step(x, out, z.cpu(), coeffs, prediction_type, clip)
            err = (prev.cpu().double() - ref_prev).abs()
            ratio = float((err / (EPS32 * L + 1e-300)).max())
            worst = max(worst, ratio)
            assert ratio <= 4.0, (clip, t, ratio)
            assert float(((pred.cpu().double() - ref_pred).abs() / (EPS32 * L / abs(coeffs[2]) + 1e-300)).max()) <= 4.0
            if t == 0:
                assert coeffs[4] == 0.0
                c0, ct = np.float32(coeffs[2]), np.float32(coeffs[3])
                mean = torch.from_numpy(c0 * pred.cpu().numpy() + ct * x.numpy())
                assert torch.equal(prev.cpu(), mean)
            else:
                assert float((prev.cpu().double() - (ref_prev - coeffs[4] * z.cpu().double())).abs().max()) > 1e-3  # noise went in
            # pred_original is optional: the same prev without it
            prev2, none = ops.ancestral_step(xd, od, sqrt_ac=coeffs[0], sqrt_1m_ac=coeffs[1], c0=coeffs[2], ct=coeffs[3],
                                             sigma=coeffs[4], seed=sampling_key(5),
                                             row_streams=sampling_streams(row_ids, t) if t else None,
                                             prediction_type=prediction_type, clip_sample=clip, return_pred=False)
            assert none is None and torch.equal(prev2, prev)
    print(f"ancestral_step {prediction_type} {row_shape}: worst error {worst:.2f} ulp of the largest term (bound 4)")


def test_unaligned_pointers_take_the_scalar_path(device):
    """row_numel % 4 == 0 but a base pointer 4 bytes off a 16-byte boundary: same numbers as the aligned call."""
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(3)
    n = 2 * 1024
    buf_x, buf_o = torch.randn(n + 1, generator=g).to(device), torch.randn(n + 1, generator=g).to(device)
    kw = dict(sqrt_ac=0.5, sqrt_1m_ac=0.75 ** 0.5, c0=0.3, ct=0.6, sigma=0.2, seed=9, row_streams=[4, 5])
    x_off, o_off = buf_x[1:].view(2, 1024), buf_o[1:].view(2, 1024)
    assert x_off.data_ptr() % 16 == 4
    a, pa = ops.ancestral_step(x_off, o_off, **kw)
    b, pb = ops.ancestral_step(x_off.clone(), o_off.clone(), **kw)
    assert torch.equal(a, b) and torch.equal(pa, pb)


# ---- the noise -------------------------------------------------------------------------------------------------------------

def test_randn_rows_is_the_training_generator(device):
    """One generator, not two: a single row with stream s is bit-equal to train_ops.randn(seed, s) of the same length."""
    from ddpm_ood_amd import ops, train_ops

    for n, seed, s in ((1024, 7, 3), (735, 2 ** 63 | 5, 65536 * 9 + 412), (3 * 64 * 64, 0, 2 ** 40 + 1)):
        a = ops.randn_rows((1, n), seed, [s], device=device)
        b = train_ops.randn((n,), device, seed, s)
        assert torch.equal(a[0], b), (n, seed, s)
    many = ops.randn_rows((3, 735), 7, [10, 11, 12], device=device)
    for r, s in enumerate((10, 11, 12)):
        assert torch.equal(many[r], train_ops.randn((735,), device, 7, s))


def test_rows_do_not_depend_on_the_batch_they_ride_in(device):
    from ddpm_ood_amd import DDPMScheduler

    g = torch.Generator().manual_seed(8)
    x, e = torch.randn(4, 1, 28, 28, generator=g).to(device), torch.randn(4, 1, 28, 28, generator=g).to(device)
    s = DDPMScheduler(**SCHED)
    full, _ = s.step(e, 500, x, seed=3, row_ids=[5, 6, 7, 8])
    alone, _ = s.step(e[2:3].contiguous(), 500, x[2:3].contiguous(), seed=3, row_ids=[7])
    assert torch.equal(full[2:3], alone)
    other, _ = s.step(e[2:3].contiguous(), 500, x[2:3].contiguous(), seed=3, row_ids=[6])
    assert not torch.equal(other, alone)
    reseed, _ = s.step(e[2:3].contiguous(), 500, x[2:3].contiguous(), seed=4, row_ids=[7])
    assert not torch.equal(reseed, alone)
    x_t = s.initial_noise((4, 1, 28, 28), seed=3, row_ids=[5, 6, 7, 8], device=device)
    assert torch.equal(x_t[2:3], s.initial_noise((1, 1, 28, 28), seed=3, row_ids=[7], device=device))


def test_noise_moments(device):
    """2^22 values as 2^14 rows (consecutive stream ids) of 256: mean, variance, lag-1 correlation of the flattened sequence and
    of the pairs that straddle a row boundary, each within 5 sigma of its sampling error under the N(0, 1) i.i.d. hypothesis
    (derived, not measured): sd(mean) = 1 / sqrt(N); sd(s^2) = sqrt(2 / N); sd(r) = 1 / sqrt(pairs)."""
    from ddpm_ood_amd import ops

    rows, cols = 2 ** 14, 256
    N = rows * cols
    z = ops.randn_rows((rows, cols), 2 ** 63 | 1, [7 * 65536 + i for i in range(rows)], device=device).double().cpu()
    assert torch.isfinite(z).all()
    mean, var = float(z.mean()), float(z.var())
    flat = z.flatten()
    r_all = float((flat[:-1] * flat[1:]).mean())
    r_edge = float((z[:-1, -1] * z[1:, 0]).mean())
    print(f"noise: mean {mean:.2e}, var - 1 {var - 1:.2e}, lag-1 r {r_all:.2e}, across the row boundary {r_edge:.2e}")
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1) <= 5 * math.sqrt(2 / N)
    assert abs(r_all) <= 5 / math.sqrt(N - 1)
    assert abs(r_edge) <= 5 / math.sqrt(rows - 1)


def test_nan_model_output_sets_the_status_word(device):
    from ddpm_ood_amd import DDPMScheduler, _lib

    s = DDPMScheduler(**SCHED)
    x = torch.zeros(2, 1, 28, 28, device=device)
    e = torch.zeros(2, 1, 28, 28, device=device)
    _lib.status_read(clear=True)
    s.step(e, 500, x)
    assert _lib.status_read(clear=True) == 0
    e[1, 0, 27, 27] = float("nan")
    s.step(e, 500, x)
    assert _lib.status_read(clear=True) == 1  # DDPM_STATUS_NONFINITE_EPS
    assert _lib.status_read(clear=True) == 0


# ---- the loop, end to end ---------------------------------------------------------------------------------------------

def _models(device, double=False):
    import oracle
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    sd = random_state_dict("small", 1, seed=1)
    ref = oracle.DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"]).eval()
    ref.load_state_dict(sd)
    if double:
        ref = ref.double()
    hip = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    hip.load_state_dict(sd)
    return ref, hip.to(device).eval()


def test_pndm_sampling_matches_the_oracle_loop(device):
    """inferer.sample over PNDMScheduler.set_timesteps(10), seeded `small` UNet, 32x32x1, B = 4, against the oracle UNet + the
    oracle PNDM loop on the CPU from the same x_T.  Measured: see DESIGN 3.16."""
    import oracle
    from ddpm_ood_amd import DiffusionInferer, PNDMScheduler, ops
    from ddpm_ood_amd.scheduler import sampling_key, sampling_streams

    ref, hip = _models(device)
    x_t = ops.randn_rows((4, 1, 32, 32), sampling_key(1), sampling_streams(range(4), 1000), device=device)
    s = PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, **SCHED)
    s.set_timesteps(10)
    got, inter = DiffusionInferer().sample(x_t, hip, s, save_intermediates=True, intermediate_steps=500)
    assert len(inter) == 2 and torch.equal(inter[-1], got)  # t = 500 and t = 0
    so = oracle.PNDMScheduler(num_train_timesteps=1000, skip_prk_steps=True, **SCHED)
    so.set_timesteps(10)
    x = x_t.cpu()
    with torch.no_grad():
        for t in so.timesteps:
            x, _ = so.step(ref(x, timesteps=torch.full((4,), int(t))), t, x)
    err = _rel_err(got.cpu(), x)
    print(f"PNDM 10-step sampling, B = 4: max error {err:.3e} of max |x_0| = {float(x.abs().max()):.3f} (bound {CHAIN_REL})")
    assert math.isfinite(err) and err <= CHAIN_REL, err
    again = DiffusionInferer().sample(x_t, hip, s)  # set_timesteps was not called again: PLMS history persists (Q3) ...
    s.set_timesteps(10)
    assert torch.equal(DiffusionInferer().sample(x_t, hip, s), got) and again.shape == got.shape  # ... a fresh one is deterministic


# The stochastic chain runs at 16x16: the replay must keep every x0 of every step at least 1e-4 away from the clamp edges, and how
# many seeds do is a matter of how many x0 values there are.  Under random weights x0 is about N(0, 1) wide at every step
# (density 0.24 at +-1), so a step of n elements puts n * 2 edges * 2e-4 * 0.24 ~ 1e-4 n values inside the band: 25 steps of
# 4 x 32 x 32 expect ~10 (a seed passes with probability e^-10; none of the first 141 did), 25 steps of 4 x 16 x 16 expect ~2.5
# (seeds 0 and 4 of the first five pass, with 1.32e-4 and 2.04e-4).  The seed is the smallest that passes, found from the replay
# alone, and asserted below.
ANCESTRAL_SHAPE = (4, 1, 16, 16)
ANCESTRAL_SEED = 0


def ancestral_replay(device, seed, steps=25):
    """(x_T on the device, float64 CPU replay of `steps` ancestral steps, distance of the closest x0 to a clamp edge)."""
    from ddpm_ood_amd import DDPMScheduler, ops
    from ddpm_ood_amd.scheduler import sampling_key, sampling_streams

    ref, _ = _models(device, double=True)
    s = DDPMScheduler(num_train_timesteps=1000, **SCHED)
    s.set_timesteps(steps)
    x_t = s.initial_noise(ANCESTRAL_SHAPE, seed=seed, device=device)
    assert torch.equal(x_t, ops.randn_rows(ANCESTRAL_SHAPE, sampling_key(seed), sampling_streams(range(4), 1000), device=device))
    x = x_t.cpu().double()
    margin = float("inf")
    with torch.no_grad():
        for t in s.timesteps:
            t = int(t)
            sa, sb, c0, ct, sigma = (float(np.float32(c)) for c in s.step_coefficients(t))
            eps = ref(x, timesteps=torch.full((4,), t))
            x0 = (x - sb * eps) / sa
            margin = min(margin, float((x0.abs() - 1).abs().min()))
            mean = c0 * x0.clamp(-1, 1) + ct * x
            if sigma:
                z = ops.randn_rows(ANCESTRAL_SHAPE, sampling_key(seed), sampling_streams(range(4), t), device=device)
                mean = mean + sigma * z.cpu().double()
            x = mean
    return x_t, x, margin


def test_ancestral_sampling_matches_a_float64_replay(device):
    """25 ancestral steps (set_timesteps(25)), B = 4, 16x16x1, against a CPU replay in float64: the oracle UNet + the closed form, x_T and
    every z_t fetched through ops.randn_rows for the same streams.  The seed keeps every x0 of the replay >= 1e-4 from the clamp
    edges (the clamp's kink would otherwise turn a rounding difference into a different branch)."""
    from ddpm_ood_amd import DDPMScheduler, DiffusionInferer

    _, hip = _models(device)
    x_t, ref_x, margin = ancestral_replay(device, ANCESTRAL_SEED)
    print(f"ancestral replay, seed {ANCESTRAL_SEED}: closest x0 to a clamp edge {margin:.3e}")
    assert margin >= 1e-4, margin
    s = DDPMScheduler(num_train_timesteps=1000, **SCHED)
    s.set_timesteps(25)
    got = DiffusionInferer().sample(x_t, hip, s, seed=ANCESTRAL_SEED)
    err = _rel_err(got.cpu(), ref_x)
    print(f"ancestral 25-step sampling, B = 4: max error {err:.3e} of max |x_0| = {float(ref_x.abs().max()):.3f} (bound {CHAIN_REL})")
    assert math.isfinite(err) and err <= CHAIN_REL, err
    assert torch.equal(DiffusionInferer().sample(x_t, hip, s, seed=ANCESTRAL_SEED), got)
    assert not torch.equal(DiffusionInferer().sample(x_t, hip, s, seed=ANCESTRAL_SEED + 1), got)


# ---- sample.py -------------------------------------------------------------------------------------------------------------

def _run_cli(tmp_path, model, out, *extra, timeout=900):
    cmd = [sys.executable, str(ROOT / "sample.py"), "--output_dir", str(tmp_path), "--model_name", model, "--is_grayscale", "1",
           "--image_size", "32", *SCHED_CLI, "--out", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return np.load(Path(out) / "samples.npy")


@pytest.mark.parametrize("sched", [("--scheduler", "ddpm"), ("--scheduler", "pndm", "--num_inference_steps", "100")])
def test_sample_cli(device, tmp_path, sched):
    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.data import read_png

    model = "fashionmnist_sample"
    synthetic.write_checkpoint(tmp_path / model, "small", 1, seed=1)
    n = ["--num_samples", "8"]
    a = _run_cli(tmp_path, model, tmp_path / "a", *sched, *n, "--seed", "3", "--batch_size", "8")
    assert a.shape == (8, 1, 32, 32) and a.dtype == np.float32 and a.min() >= 0 and a.max() <= 1 and a.std() > 1e-3
    png = read_png(str(tmp_path / "a" / "samples.png"))
    assert png.shape == (64, 128) and np.array_equal(png, np.rint(a.reshape(2, 4, 32, 32).transpose(0, 2, 1, 3).reshape(64, 128) * 255))
    b = _run_cli(tmp_path, model, tmp_path / "b", *sched, *n, "--seed", "3", "--batch_size", "8")
    assert (tmp_path / "a" / "samples.npy").read_bytes() == (tmp_path / "b" / "samples.npy").read_bytes()
    assert (tmp_path / "a" / "samples.png").read_bytes() == (tmp_path / "b" / "samples.png").read_bytes()
    c = _run_cli(tmp_path, model, tmp_path / "c", *sched, *n, "--seed", "4", "--batch_size", "8")
    assert np.abs(c - a).max() > 1e-2
    # batches of 3 (3 + 3 + 2): the engine dispatches by batch, so equal within the chain bound, not bit for bit
    d = _run_cli(tmp_path, model, tmp_path / "d", *sched, *n, "--seed", "3", "--batch_size", "3")
    err = float(np.abs(d - a).max() / np.abs(a).max())
    print(f"sample.py {sched[1]}: --batch_size 3 vs 8: max difference {err:.3e} of max |x| (bound {CHAIN_REL})")
    assert err <= CHAIN_REL, err


def test_sample_cli_missing_checkpoint(device, tmp_path):
    import sample
    from ddpm_ood_amd.sampling import Sampler

    (tmp_path / "m").mkdir()
    args = sample.parse_args(["--output_dir", str(tmp_path), "--model_name", "m", "--is_grayscale", "1", "--image_size", "32"])
    with pytest.raises(FileNotFoundError, match="Failed to find a saved model checkpoint"):
        Sampler(args)


def test_latent_sample_through_a_vqvae_with_latent_pad(device, tmp_path):
    """One latent through a conditioned synthetic VQ-VAE: 48^3 volumes -> [128, 3, 3, 3] latents (27 elements per channel: the
    scalar path), padded to 4^3 for the UNet, cropped back, decoded to the image shape."""
    import sample
    from oracle.vqvae import VQVAE as OracleVQVAE
    from parity_util import VQ_README
    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.sampling import Sampler

    torch.manual_seed(3)
    vq = OracleVQVAE(**VQ_README).eval()
    vq_dir = tmp_path / "vqvae"
    vq_dir.mkdir()
    torch.save({"model_state_dict": synthetic.condition_vqvae_state_dict(vq.state_dict())}, vq_dir / "checkpoint.pth")
    json.dump(VQ_README, open(vq_dir / "vqvae_config.json", "w"))
    model = "decathlon_sample"
    (tmp_path / model).mkdir()
    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               tmp_path / model / "checkpoint.pth")
    args = sample.parse_args(["--output_dir", str(tmp_path), "--model_name", model, "--is_grayscale", "1", "--image_size", "48",
                              "--spatial_dimension", "3", "--vqvae_checkpoint", str(vq_dir / "checkpoint.pth"),
                              "--latent_pad", "(0,1,0,1,0,1)", *SCHED_CLI, "--num_samples", "1", "--batch_size", "1",
                              "--num_inference_steps", "20"])
    smp = Sampler(args)
    assert smp.latent_shape() == (128, 4, 4, 4)
    x = smp.sample()
    assert x.shape == (1, 1, 48, 48, 48) and np.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
    from ddpm_ood_amd.data import read_png

    assert read_png(str(tmp_path / model / "samples" / "samples.png")).shape == (48, 3 * 48)


def test_two_ranks_on_one_gpu_draw_the_same_samples(device, tmp_path):
    """sample.py as 1 rank and as 2 ranks (gloo rendezvous, both on cuda:0: tests/test_gpu_dist.py's hook): sample i goes to rank
    i % 2, one gather, rank 0 writes, in index order -- the union equals the single-process run within the chain bound."""
    from test_gpu_dist import _launch_ranks
    from ddpm_ood_amd import synthetic

    model = "fashionmnist_sample2"
    synthetic.write_checkpoint(tmp_path / model, "small", 1, seed=1)
    flags = ["--scheduler", "pndm", "--num_inference_steps", "20", "--num_samples", "7", "--seed", "3", "--batch_size", "4"]
    one = _run_cli(tmp_path, model, tmp_path / "w1", *flags)
    argv = [str(ROOT / "sample.py"), "--output_dir", str(tmp_path), "--model_name", model, "--is_grayscale", "1",
            "--image_size", "32", *SCHED_CLI, "--out", str(tmp_path / "w2"), *flags]
    _launch_ranks(2, argv, tmp_path)
    two = np.load(tmp_path / "w2" / "samples.npy")
    assert two.shape == one.shape == (7, 1, 32, 32)
    err = float(np.abs(two - one).max() / np.abs(one).max())
    print(f"2 ranks vs 1 rank: max difference {err:.3e} of max |x| (bound {CHAIN_REL})")
    assert err <= CHAIN_REL, err  # in index order: a permutation would differ by O(1)


# ---- validation grids ------------------------------------------------------------------------------------------------------

def _train_args(tmp_path, **kw):
    import argparse

    d = dict(seed=2, output_dir=str(tmp_path), model_name="val_grids", training_ids="synthetic:blobs:n=8:seed=1",
             validation_ids="synthetic:blobs:n=4:seed=10", spatial_dimension=2, image_size=None, image_roi=None, latent_pad=None,
             vqvae_checkpoint=None, prediction_type="epsilon", model_type="small", beta_schedule="scaled_linear_beta",
             beta_start=0.0015, beta_end=0.0195, b_scale=1.0, snr_shift=1, simplex_noise=0, batch_size=4, n_epochs=2, eval_freq=1,
             augmentation=1, num_workers=0, cache_data=1, checkpoint_every=0, ddpm_checkpoint_epoch=None, is_grayscale=1,
             quick_test=0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_validation_grids_are_drawn_from_the_updated_parameters(device, tmp_path, monkeypatch):
    """DDPM_VAL_SAMPLES=1, two epochs with eval_freq = 1: two grids.  The sampler's forwards are the inference engine's, which
    packs its own copy of the weights: after the optimiser moved the parameters (in place, by a kernel torch does not see) the
    engine must have re-packed them -- its output on a probe equals unet_forward_torch on the holders as they are NOW, and is far
    from the output under the initial parameters.  No tape is left behind."""
    from ddpm_ood_amd.data import read_png
    from ddpm_ood_amd.train import DDPMTrainer, unet_forward_torch

    monkeypatch.setenv("DDPM_VAL_SAMPLES", "1")
    args = _train_args(tmp_path)
    tr = DDPMTrainer(args)
    assert tr.native
    tr.stepper.lr = 1e-3  # (the probe below must see the parameters move)
    g = torch.Generator().manual_seed(5)
    probe, t = torch.randn(8, 1, 32, 32, generator=g).to(device), torch.full((8,), 400, device=device)
    before = tr.model(probe, timesteps=t).clone()
    tr.train(args)
    val = tmp_path / "val_grids" / "val"
    for e in (0, 1):
        a = np.load(val / f"samples_epoch{e}.npy")
        assert a.shape == (8, 1, 32, 32) and np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
        assert read_png(str(val / f"samples_epoch{e}.png")).shape == (64, 128)
    assert not np.array_equal(np.load(val / "samples_epoch0.npy"), np.load(val / "samples_epoch1.npy"))
    assert tr.stepper._tape is None
    # the engine state the second grid was drawn with: nothing touched the parameters since
    assert tr.model._synced_key is not None
    now = tr.model(probe, timesteps=t)
    with torch.no_grad():
        want = unet_forward_torch(tr.model, probe, t)
    scale = float(want.abs().max())
    assert float((now - want).abs().max()) <= 2e-5 * (1 + scale)  # the single-forward bound of tests/test_gpu_dispatch.py
    assert float((now - before).abs().max()) > 100 * 2e-5 * (1 + scale)


def test_no_validation_grids_by_default(device, tmp_path, monkeypatch):
    from ddpm_ood_amd.train import DDPMTrainer

    monkeypatch.delenv("DDPM_VAL_SAMPLES", raising=False)
    args = _train_args(tmp_path, n_epochs=1)
    tr = DDPMTrainer(args)
    tr.train(args)
    assert not (tmp_path / "val_grids" / "val").exists()
    assert tr.stepper._tape is None
