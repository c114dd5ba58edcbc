"""-m gpu: --simplex_noise -- the HIP kernel (simplex.hip) against the noise recorded from the reference's own function
(tests/golden/simplex_noise.npz), and the flag through reconstruction (against the CPU oracle), training (native step against
ATen autograd) and both CLIs."""

import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
G = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def fixture():
    return np.load(G / "simplex_noise.npz")


def test_kernel_matches_every_recorded_slice(device, fixture):
    from ddpm_ood_amd import ops

    d = fixture
    worst = {}
    for k in range(len(d["slice_seed"])):
        h, w = (int(v) for v in d["slice_hw"][k])
        octaves, persistence, frequency = (float(v) for v in d["slice_params"][k])
        seeds = torch.tensor([[int(d["slice_seed"][k])]], dtype=torch.int64)
        t = torch.tensor([int(d["slice_t"][k])], dtype=torch.int64)
        got = ops.simplex_noise((1, 1, h, w), seeds, t, int(octaves), persistence, frequency).cpu()[0, 0].double()
        err = float((got - torch.from_numpy(d[f"slice_{k}"])).abs().max())
        key = "default" if (octaves, persistence, frequency) == (6, 0.8, 64) else "(2, 0.6, 16)"
        worst[key] = max(worst.get(key, 0.0), err)
        assert err <= 1e-6, (k, h, w, int(d["slice_t"][k]), err)
    print(f"simplex slices: max |kernel - reference| = {worst}")
    assert set(worst) == {"default", "(2, 0.6, 16)"}


@pytest.mark.parametrize("call", ["call2d", "call3d"])
def test_kernel_matches_whole_reference_calls(device, fixture, call):
    """generate_simplex_noise(x, t, in_channels = C): seeds drawn channel-major (for each channel, for each row), slice (row,
    channel) at noise[row, channel], and for a 3-D x the same slice on every depth plane."""
    from ddpm_ood_amd import ops

    shape = tuple(int(v) for v in fixture[f"{call}_shape"])
    B, C = shape[:2]
    seeds = torch.from_numpy(fixture[f"{call}_seeds"]).reshape(C, B).t().contiguous()  # -> [row, channel]
    t = torch.from_numpy(fixture[f"{call}_t"])
    got = ops.simplex_noise(shape, seeds.to(device), t.to(device)).cpu()
    err = float((got - torch.from_numpy(fixture[f"{call}_noise"])).abs().max())
    print(f"{call} {shape}: max |kernel - reference| = {err:.2e}")
    assert err <= 1e-6


def _sets():
    return {"val": "synthetic:blobs:n=3:seed=10", "in": "synthetic:blobs:n=3:seed=11",
            "out": "synthetic:noise:n=3:seed=12:name=MNIST"}


def _simplex_fn(seed):
    from ddpm_ood_amd import ops
    from ddpm_ood_amd.trainer import simplex_seeds

    def noise(batch, t, shape):
        return ops.simplex_noise(shape, simplex_seeds(seed, batch["index"], t, shape[1]), torch.full((shape[0],), int(t))).cpu()

    return noise


def test_reconstruction_with_simplex_noise_matches_oracle(device, tmp_path):
    """k = 64 (t in {10, 650}, stale PLMS history) on the bench dispatch: HIP rows against the CPU oracle given the product's
    simplex noise; with the flag off the rows change (the noise is wired in)."""
    import oracle
    from ddpm_ood_amd import synthetic
    from ddpm_ood_amd.trainer import MODEL_CONFIGS, Reconstruct
    from parity_util import assert_rows_close, assert_z_close, hip_scores, loader_for, make_args

    args = make_args(tmp_path, simplex_noise=1, batch_size=2, validation_ids=_sets()["val"], in_ids=_sets()["in"])
    sd = synthetic.write_checkpoint(tmp_path / args.model_name, "small", 1, seed=1)
    rec = Reconstruct(args)
    rows_h = {name: hip_scores(args, rec, ids, name) for name, ids in _sets().items()}

    ref = oracle.DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"]).eval()
    ref.load_state_dict(sd)
    pl = oracle.PerceptualLoss(dimensions=2, include_pixel_loss=False, is_fake_3d=False, lpips_normalize=True)
    pl.perceptual_function.load_state_dict(rec._perceptual().perceptual_function.state_dict())
    rows_o = {}
    for name, ids in _sets().items():
        rows_o[name] = pd.DataFrame(oracle.get_scores(
            loader_for(args, ids), name, 64, model=ref, vqvae=oracle.PassthroughVQVAE(), perceptual=pl,
            noise_fn=_simplex_fn(args.seed), beta_schedule=args.beta_schedule, beta_start=args.beta_start,
            beta_end=args.beta_end))
        assert sorted(set(rows_o[name]["t"])) == [10, 650]
        assert_rows_close(rows_h[name], rows_o[name], 2e-4, name)
    worst, auc_h, auc_o = assert_z_close(rows_h, rows_o, tol=1e-4)
    print(f"simplex reconstruction: worst |dZ| {worst:.2e}, AUROC {auc_h:.4f} / {auc_o:.4f}")

    gauss = Reconstruct(make_args(tmp_path, simplex_noise=0, batch_size=2, validation_ids=_sets()["val"], in_ids=_sets()["in"]))
    rows_g = hip_scores(args, gauss, _sets()["in"], "in")
    assert (rows_g["mse"] - rows_h["in"]["mse"]).abs().max() > 1e-4


def test_simplex_noise_and_rows_do_not_depend_on_the_batch(device, tmp_path):
    from ddpm_ood_amd import ops, synthetic
    from ddpm_ood_amd.trainer import Reconstruct, simplex_seeds
    from parity_util import hip_scores, make_args

    t = torch.full((16,), 650)
    whole = ops.simplex_noise((16, 1, 32, 32), simplex_seeds(2, range(16), 650, 1), t)
    parts = torch.cat([ops.simplex_noise((4, 1, 32, 32), simplex_seeds(2, range(s, s + 4), 650, 1), t[:4]) for s in range(0, 16, 4)])
    assert torch.equal(whole, parts)

    synthetic.write_checkpoint(tmp_path / "synth", "small", 1, seed=1)
    ids = "synthetic:blobs:n=16:seed=11"
    rows = {}
    for bs in (4, 16):
        args = make_args(tmp_path, simplex_noise=1, batch_size=bs, validation_ids=ids, in_ids=ids)
        rows[bs] = hip_scores(args, Reconstruct(args), ids, "in")
    # (rows come per batch, per t, per image -- the reference's order -- so the two batchings list them differently)
    a, b = (rows[bs].sort_values(["filename", "t"]).reset_index(drop=True) for bs in (4, 16))
    assert list(a["filename"]) == list(b["filename"]) and list(a["t"]) == list(b["t"]) and len(a) == 16 * 2
    for col in ("mse", "perceptual_difference"):
        rel = float(((a[col] - b[col]).abs() / (b[col].abs() + 1e-6)).max())
        assert rel <= 1e-5, (col, rel)


def test_native_step_and_aten_autograd_agree_on_simplex_noise(device):
    """One training step from identical weights, images, timesteps and simplex noise: the native HIP step against PyTorch-ROCm
    autograd over the same parameter holders -- loss and every gradient (max-norm relative error <= 1e-4)."""
    from ddpm_ood_amd import DiffusionModelUNet, ops
    from ddpm_ood_amd.scheduler import DDPMScheduler
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.train import unet_forward_torch
    from ddpm_ood_amd.train_native import NativeUNetStep
    from ddpm_ood_amd.trainer import MODEL_CONFIGS, simplex_seeds

    sd = random_state_dict("small", 1, seed=1)
    x0 = torch.rand(4, 1, 32, 32, generator=torch.Generator().manual_seed(11)).to(device)
    t = torch.tensor([10, 330, 650, 970])
    noise = ops.simplex_noise((4, 1, 32, 32), simplex_seeds(2, range(4), 1, 1), t)
    assert 0.05 < float(noise.std()) < 1.0
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    noisy = sched.add_noise(original_samples=x0, noise=noise, timesteps=t).contiguous()
    t_dev = t.to(device)

    models = []
    for _ in range(2):
        m = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
        m.load_state_dict(sd)
        models.append(m.to(device).train())
    nat, aten = models
    with torch.no_grad():
        step = NativeUNetStep(nat, lr=2.5e-5)
        loss_n = step.loss_and_grads(noisy, t_dev, noise)
    for p in aten.parameters():
        p.requires_grad_(True)
    loss_a = torch.nn.functional.mse_loss(unet_forward_torch(aten, noisy, t_dev), noise)
    loss_a.backward()
    assert abs(loss_n.item() - loss_a.item()) <= 1e-5 * abs(loss_a.item())
    pn, pa = dict(nat.named_parameters()), dict(aten.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in pa.values() if p.grad is not None)
    worst = 0.0
    for k, p in pa.items():
        if p.grad is None:
            continue
        rel = float((pn[k].grad - p.grad).abs().max() / max(float(p.grad.abs().max()), 1e-5 * gmax))
        worst = max(worst, rel)
        assert rel <= 1e-4, (k, rel)
    print(f"simplex training step: loss {loss_a.item():.6f}, worst gradient max-norm relative error {worst:.2e}")


def _train_args(tmp_path, **kw):
    import argparse

    d = dict(seed=2, output_dir=str(tmp_path), model_name="simplex_trained",
             training_ids="synthetic:blobs:n=64:seed=1", validation_ids="synthetic:blobs:n=8:seed=10",
             spatial_dimension=2, image_size=None, image_roi=None, latent_pad=None, vqvae_checkpoint=None,
             prediction_type="epsilon", model_type="small", beta_schedule="scaled_linear_beta", beta_start=0.0015,
             beta_end=0.0195, b_scale=1.0, snr_shift=1, simplex_noise=1, batch_size=32, n_epochs=2, eval_freq=1,
             augmentation=1, num_workers=0, cache_data=1, checkpoint_every=100, ddpm_checkpoint_epoch=None,
             is_grayscale=1, quick_test=0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_train_with_simplex_noise_then_reconstruct_cli(device, tmp_path, monkeypatch):
    from ddpm_ood_amd import ops
    from ddpm_ood_amd.train import DDPMTrainer

    calls = []
    real = ops.simplex_noise

    def spy(shape, *a, **kw):
        calls.append(tuple(shape))
        return real(shape, *a, **kw)

    monkeypatch.setattr(ops, "simplex_noise", spy)
    args = _train_args(tmp_path)
    tr = DDPMTrainer(args)
    tr.train(args)
    losses = [l for _, l in tr.history]
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert (tmp_path / args.model_name / "checkpoint.pth").exists()
    # 2 epochs x 2 training batches of 32, and one validation pass per epoch (one batch of 8): all simplex
    assert calls.count((32, 1, 32, 32)) == 4 and calls.count((8, 1, 32, 32)) == 2, calls
    assert tr.noise_calls == 6

    cmd = [sys.executable, str(ROOT / "reconstruct.py"), "--output_dir", str(tmp_path), "--model_name", args.model_name,
           "--is_grayscale", "1", "--simplex_noise", "1", "--validation_ids", "synthetic:blobs:n=2:seed=10",
           "--in_ids", "synthetic:blobs:n=2:seed=11", "--run_out", "0", "--beta_schedule", "scaled_linear_beta",
           "--beta_start", "0.0015", "--beta_end", "0.0195", "--batch_size", "2", "--inference_skip_factor", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    for n in ("val", "in"):
        df = pd.read_csv(tmp_path / args.model_name / "ood" / f"results_{n}.csv")
        assert len(df) == 2 * 2 and df["mse"].between(0, 1).all()


def test_native_simplex_step_launches_no_aten_or_library_kernels(device):
    """The --simplex_noise form of test_native_training_step_launches_no_aten_or_library_kernels: noise, forward, MSE, backward
    and Adam of one native step launch kernels of libddpm_ood_hip.so only."""
    from torch.profiler import ProfilerActivity, profile

    from ddpm_ood_amd import DiffusionModelUNet, ops
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.train_native import NativeUNetStep
    from ddpm_ood_amd.trainer import MODEL_CONFIGS, simplex_seeds

    hip = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    hip.load_state_dict(random_state_dict("small", 1, seed=1))
    hip = hip.to(device).train()
    B = 32
    x = torch.rand(B, 1, 32, 32, device=device)
    t_host = torch.randint(0, 1000, (B,))
    t = t_host.to(device)
    with torch.no_grad():
        step = NativeUNetStep(hip, lr=2.5e-5)
        noise = ops.simplex_noise((B, 1, 32, 32), simplex_seeds(1, range(B), 1, 1), t_host)
        step.loss_and_grads(x, t, noise)  # warm-up: code objects, allocator
        step.adam_step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            noise = ops.simplex_noise((B, 1, 32, 32), simplex_seeds(1, range(B), 2, 1), t_host)
            loss = step.loss_and_grads(x, t, noise)
            step.adam_step()
            torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    if not names:
        pytest.skip("torch.profiler recorded no device kernels on this box")
    foreign = [n for n in names if any(k in n for k in ("at::native", "at_cuda", "miopen", "MIOpen", "rocblas", "Cijk_", "hipblas"))]
    assert not foreign, foreign
    assert any("simplex_noise_kernel" in n for n in names), names
    print(f"native simplex step: {len(names)} distinct device kernels; loss {float(loss.cpu()):.5f}")
