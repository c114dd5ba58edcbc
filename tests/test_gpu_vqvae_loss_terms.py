"""-m gpu: the perceptual and spectral terms of VQ-VAE training (ddpm_ood_amd/loss_terms.py, csrc/lpips_train.hip, csrc/spectral.hip)
-- every new kernel against float64 autograd on the host, the two terms against float64 autograd over torch.fft and the oracle's
LPIPS, the trainer with DDPM_VQVAE_LOSS_TERMS=perceptual,spectral against float64 autograd over the oracle's VQ-VAE, and the CLI.

Bars (the project's own): gradients 1e-4 max-norm relative, floored at 1e-5 of the largest gradient (the measure of
tests/test_gpu_vqvae_train.py::test_parameter_gradients_match_float64_autograd_over_the_oracle); loss values 2e-5 relative (the
LPIPS score tests).  Reconstructions are 0.8 x + 0.1 + 0.05 randn, seeded, so that |R| - |X| is not degenerate."""

import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GRAD_BAR, LOSS_BAR = 1e-4, 2e-5

CFG = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(8, 16), num_res_layers=1, num_res_channels=(8, 16),
           downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1)), upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0)),
           num_embeddings=16, embedding_dim=8, decay=0.99, commitment_cost=0.25, epsilon=1e-5)


def _cli(size):
    return ["--spatial_dimension", "2", "--is_grayscale", "1", "--vqvae_num_channels", "(8, 16)", "--vqvae_num_res_channels",
            "(8, 16)", "--vqvae_num_res_layers", "1", "--vqvae_downsample_parameters", "((2, 4, 1, 1), (2, 4, 1, 1))",
            "--vqvae_upsample_parameters", "((2, 4, 1, 1, 0), (2, 4, 1, 1, 0))", "--vqvae_num_embeddings", "16",
            "--vqvae_embedding_dim", "8", "--training_ids", f"synthetic:blobs:n=16:size={size}:seed=1",
            "--validation_ids", f"synthetic:blobs:n=16:size={size}:seed=2", "--batch_size", "16"]


def _pair_of(shape, seed, blobs=False):
    """(image, reconstruction) float32 on the host: blobs or uniform noise, reconstruction = 0.8 x + 0.1 + 0.05 randn."""
    from ddpm_ood_amd.data import synthetic_images

    g = torch.Generator().manual_seed(seed)
    x = synthetic_images("blobs", shape[0], shape[1], shape[2], seed=1) if blobs else torch.rand(shape, generator=g)
    assert tuple(x.shape) == tuple(shape)
    return x.float(), (0.8 * x + 0.1 + 0.05 * torch.randn(shape, generator=g)).float()


def _rel(got, ref, floor=0.0):
    ref = ref.detach().double()
    return float((got.detach().cpu().double() - ref).abs().max() / max(float(ref.abs().max()), floor))


# ---- spectral term ------------------------------------------------------------------------------------------------------------

def _spectral64(r, x):
    dims = tuple(range(1, x.ndim))
    r = r.double().requires_grad_(True)
    a = lambda t: torch.fft.fftn(t, dim=dims, norm="ortho").abs()  # noqa: E731
    loss = ((a(r) - a(x.double())) ** 2).mean()
    loss.backward()
    return float(loss.detach()), r.grad


@pytest.mark.parametrize("shape,blobs", [((4, 1, 16, 16), True), ((2, 3, 12, 20), False), ((2, 1, 8, 12, 16), False)])
def test_spectral_value_and_gradient(device, shape, blobs):
    from ddpm_ood_amd.loss_terms import spectral_term

    x, r = _pair_of(shape, 5, blobs)
    want, gwant = _spectral64(r, x)
    rd = r.to(device).requires_grad_(True)
    loss = spectral_term(rd, x.to(device))
    (3.0 * loss).backward()  # an upstream factor: dloss reaches the kernel
    lrel, grel = abs(loss.item() - want) / want, _rel(rd.grad / 3.0, gwant)
    print(f"spectral {shape}: loss {loss.item():.6e} (rel {lrel:.2e}), gradient rel {grel:.2e}")
    assert loss.shape == () and lrel <= LOSS_BAR and grel <= GRAD_BAR


def test_spectral_edge_cases_and_reproducibility(device):
    from ddpm_ood_amd.loss_terms import spectral_term

    x, r = _pair_of((2, 3, 12, 20), 6)
    xd = x.to(device)
    same = xd.clone().requires_grad_(True)
    loss = spectral_term(same, xd)
    loss.backward()
    assert loss.item() == 0.0 and torch.isfinite(same.grad).all() and not same.grad.any()
    zero = torch.zeros_like(xd).requires_grad_(True)
    loss = spectral_term(zero, xd)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(zero.grad).all() and not zero.grad.any()  # G = 0 where |R| = 0
    want = float((x.double() ** 2).mean())  # Parseval: the transform is unitary
    assert abs(loss.item() - want) <= LOSS_BAR * want
    runs = []
    for _ in range(2):
        rd = r.to(device).requires_grad_(True)
        loss = spectral_term(rd, xd)
        loss.backward()
        runs.append((loss.detach().clone(), rd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- LPIPS backward kernels ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(7, 9), (15, 15)])
def test_maxpool3s2_backward(device, hw):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(hw[0])
    x = torch.randn((2, 3) + hw, generator=g)  # tie-free
    ho, wo = (hw[0] - 3) // 2 + 1, (hw[1] - 3) // 2 + 1
    dy = torch.randn(2, 3, ho, wo, generator=g)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2).backward(dy.double())
    got = ops.maxpool3s2_backward(x.to(device), dy.to(device))
    assert _rel(got, x64.grad) <= 1e-6
    base = torch.randn(x.shape, generator=g)
    got = ops.maxpool3s2_backward(x.to(device), dy.to(device), out=base.to(device))
    assert _rel(got, x64.grad + base.double()) <= 1e-6
    # a ReLU-ed input with zero plateaus: equal after the mask (ties at 0 carry no gradient either way)
    z = torch.randn((2, 3) + hw, generator=g)
    z[:, :, : hw[0] // 2] = -z[:, :, : hw[0] // 2].abs()  # whole windows of zeros after the ReLU
    z64 = z.double().requires_grad_(True)
    F.max_pool2d(F.relu(z64), 3, 2).backward(dy.double())
    got = ops.maxpool3s2_backward(F.relu(z).to(device), dy.to(device), relu_mask=True)
    assert _rel(got, z64.grad) <= 1e-6 and not got.cpu()[z <= 0].any()


@pytest.mark.parametrize("cx,h,w", [(1, 32, 40), (3, 32, 40), (1, 34, 33)])
def test_lpips_conv1_dgrad(device, cx, h, w):
    """Against float64 F.conv2d autograd through the affine and the 1 -> 3 broadcast; 34 rows: the last one is under no window."""
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(cx * 100 + h)
    wt = (torch.rand(64, 3, 11, 11, generator=g) * 2 - 1) / 19.0
    a = 1.0 / torch.tensor([0.458, 0.448, 0.450])
    b = torch.tensor([0.030, 0.088, 0.188]) * a
    x = torch.rand(2, cx, h, w, generator=g).double().requires_grad_(True)
    y = F.conv2d(x.expand(-1, 3, -1, -1) * a.double()[None, :, None, None] + b.double()[None, :, None, None], wt.double(), None, 4, 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.double())
    got = ops.lpips_conv1_dgrad(gy.to(device), wt.to(device), cx, h, w, 4, 2, in_scale=a.to(device))
    assert tuple(got.shape) == (2, cx, h, w) and _rel(got, x.grad) <= 1e-5
    if h == 34:
        assert not x.grad[:, :, 33].any() and not got[:, :, 33].any()  # exact zeros


@pytest.mark.parametrize("c,hw", [(64, (7, 9)), (256, (1, 1))])
def test_lpips_layer_backward(device, c, hw):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(c)
    n = 3
    f0, f1 = F.relu(torch.randn((n, c) + hw, generator=g)), F.relu(torch.randn((n, c) + hw, generator=g))
    lin, up = torch.rand(c, generator=g) / c, torch.randn(n, generator=g)
    a = f0.double().requires_grad_(True)
    norm = lambda f: f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + 1e-10)  # noqa: E731
    score = (lin.double()[None, :, None, None] * (norm(a) - norm(f1.double())) ** 2).sum(1).mean((1, 2))
    (score * up.double()).sum().backward()
    dev = [t.to(device) for t in (f0, f1, lin, up)]
    want = ops.lpips_layer(dev[0], dev[1], dev[2])
    assert _rel(want, score) <= LOSS_BAR
    got = ops.lpips_layer_backward(*dev, relu_mask=False)
    assert _rel(got, a.grad) <= GRAD_BAR
    base = torch.randn(f0.shape, generator=g)
    got = ops.lpips_layer_backward(*dev, out=base.to(device), relu_mask=True)  # accumulate, then the mask of f0's ReLU
    assert _rel(got, (a.grad + base.double()) * (f0 > 0), floor=1e-30) <= GRAD_BAR and not got.cpu()[f0 <= 0].any()


# ---- perceptual term ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lpips_pair(device):
    """(the product's PerceptualLoss on the device, the oracle's LPIPS in float64 on the host), same weights."""
    from oracle.lpips import LPIPSAlex
    from ddpm_ood_amd.perceptual import PerceptualLoss

    pl = PerceptualLoss(dimensions=2).to(device)
    o = LPIPSAlex()
    o.load_state_dict(pl.perceptual_function.state_dict())
    return pl, o.double()


def _lpips64(o, r, x):
    r = r.double().requires_grad_(True)
    v = o(r, x.double(), normalize=False).reshape(-1)
    return r, v


@pytest.mark.parametrize("shape,blobs", [((4, 1, 32, 32), True), ((2, 3, 32, 40), False), ((3, 1, 48, 32), False)])
def test_perceptual_2d_value_and_gradient(device, lpips_pair, shape, blobs):
    from ddpm_ood_amd.loss_terms import LPIPSGradFunction, perceptual_term

    pl, o = lpips_pair
    x, r = _pair_of(shape, 7, blobs)
    r64, v = _lpips64(o, r, x)
    v.mean().backward()
    rd = r.to(device).requires_grad_(True)
    LPIPSGradFunction.last_paths = {}
    loss = perceptual_term(pl.perceptual_function, rd, x.to(device), 2)
    loss.backward()
    want = float(v.mean().detach())
    lrel, grel = abs(loss.item() - want) / want, _rel(rd.grad, r64.grad)
    print(f"perceptual {shape}: loss {loss.item():.6e} (rel {lrel:.2e}), gradient rel {grel:.2e}, paths {LPIPSGradFunction.last_paths}")
    assert lrel <= LOSS_BAR and grel <= GRAD_BAR
    # input gradients of the stride-1 layers (index = AlexNet convolution): the two 256-wide 3x3 layers on the MFMA convolution
    # over the packed rotated weight, the 384 <- 192 3x3 layer and the 5x5 layer on the generic kernel
    assert LPIPSGradFunction.last_paths == {4: "mfma", 3: "mfma", 2: "generic", 1: "generic"}


def test_perceptual_3d_with_supplied_indices(device, lpips_pair):
    from ddpm_ood_amd.loss_terms import _VIEWS, fake3d_slice_indices, perceptual_term

    pl, o = lpips_pair
    shape = (1, 1, 32, 40, 32)
    x, r = _pair_of(shape, 8)
    idx = [i[:5] for i in fake3d_slice_indices(shape, 3, 0, 0)]  # five slices per axis keep the float64 reference quick
    r64 = r.double().requires_grad_(True)
    want = 0
    for perm, i in zip(_VIEWS, idx):
        rs, xs = r64.permute(*perm), x.double().permute(*perm)
        want = want + o(rs.reshape(-1, *rs.shape[2:])[i], xs.reshape(-1, *xs.shape[2:])[i], normalize=False).mean()
    want.backward()
    rd = r.to(device).requires_grad_(True)
    loss = perceptual_term(pl.perceptual_function, rd, x.to(device), 3, slice_indices=idx)
    loss.backward()
    lrel, grel = abs(loss.item() - float(want.detach())) / float(want.detach()), _rel(rd.grad, r64.grad)
    print(f"perceptual 3-D {shape}: loss {loss.item():.6e} (rel {lrel:.2e}), gradient rel {grel:.2e}")
    assert lrel <= LOSS_BAR and grel <= GRAD_BAR
    with pytest.raises(ValueError, match="slice-index"):
        perceptual_term(pl.perceptual_function, rd, x.to(device), 3)


def test_scoring_path_bits_are_unchanged_by_a_training_call(device, lpips_pair):
    from ddpm_ood_amd.loss_terms import perceptual_term

    pl, _ = lpips_pair
    x, r = _pair_of((2, 3, 32, 40), 9)
    xd, rd = x.to(device), r.to(device)
    before = (pl(xd, rd).clone(), pl.perceptual_function(xd, rd, normalize=False).clone())
    t = rd.clone().requires_grad_(True)
    perceptual_term(pl.perceptual_function, t, xd, 2).backward()
    assert t.grad is not None and all(not p.requires_grad and p.grad is None for p in pl.parameters())
    after = (pl(xd, rd), pl.perceptual_function(xd, rd, normalize=False))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_perceptual_term_rejects_small_images(device, lpips_pair):
    from ddpm_ood_amd.loss_terms import perceptual_term

    x = torch.rand(2, 1, 16, 16, device=device)
    with pytest.raises(ValueError, match=">= 32"):
        perceptual_term(lpips_pair[0].perceptual_function, x.clone().requires_grad_(True), x, 2)


# ---- trainer ------------------------------------------------------------------------------------------------------------------

def _args(tmp_path, name, size=32):
    import train_vqvae

    return train_vqvae.parse_args(_cli(size) + ["--output_dir", str(tmp_path), "--model_name", name])


def test_trainer_parameter_gradients_of_the_total_loss(device, tmp_path, monkeypatch):
    """Every encoder / decoder parameter gradient of L1 + quantisation + 0.001 perceptual + spectral against float64 autograd over
    the oracle's VQ-VAE and LPIPS and torch.fft; update_codebook=False, the oracle is fed the HIP indices."""
    from oracle.lpips import LPIPSAlex
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.data import synthetic_images
    from ddpm_ood_amd.vqvae_train import VQTrainFunction, VQVAETrainer, decode_train, encode_train

    monkeypatch.setenv("DDPM_VQVAE_LOSS_TERMS", "perceptual,spectral")
    tr = VQVAETrainer(_args(tmp_path, "grads"))
    assert tr.loss_terms == ("perceptual", "spectral") and tr.last_stats["lpips_pretrained"] is False
    x = synthetic_images("blobs", 16, 1, 32, seed=1)
    m, q = tr.model, tr.model.quantizer.quantizer
    with torch.no_grad():  # spread the codebook over the latents' range: more than one code in use
        z = encode_train(m, x.to(device))
        q.embedding.weight.mul_(z.std()).add_(z.mean(dim=(0, 2, 3))[None])
    o = OV(**CFG).eval()
    o.load_state_dict(m.state_dict())
    o = o.double()
    lp = LPIPSAlex()
    lp.load_state_dict(tr.lpips.state_dict())
    lp = lp.double()

    for p in tr.params:
        p.grad = None
    z = encode_train(m, x.to(device))
    qz, qloss, idx, _ = VQTrainFunction.apply(z, q, False)
    r = decode_train(m, qz)
    extra, values = tr.extra_terms(r, x.to(device))
    total = F.l1_loss(r, x.to(device)) + qloss + extra
    total.backward()
    assert len(torch.unique(idx)) > 1

    x64 = x.double()
    zo = o.encode(x64)
    e = o.quantizer.quantizer.embedding.weight.detach()[idx.long().cpu()].movedim(-1, 1)
    ro = o.decode(zo + (e - zo).detach())
    a = lambda t: torch.fft.fftn(t, dim=(1, 2, 3), norm="ortho").abs()  # noqa: E731
    perc = lp(ro, x64, normalize=False).mean()
    spec = ((a(ro) - a(x64)) ** 2).mean()
    lo = F.l1_loss(ro, x64) + CFG["commitment_cost"] * F.mse_loss(e, zo) + 0.001 * perc + spec
    lo.backward()
    print(f"total {total.item():.6f} vs {lo.item():.6f}; perceptual {values['perceptual'].item():.6e} vs {perc.item():.6e}; "
          f"spectral {values['spectral'].item():.6e} vs {spec.item():.6e}")
    assert abs(values["perceptual"].item() - perc.item()) <= LOSS_BAR * perc.item()
    assert abs(values["spectral"].item() - spec.item()) <= LOSS_BAR * spec.item()
    ref = dict(o.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in ref.values() if p.grad is not None)
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        if "embedding" in n:
            assert p.grad is None
            continue
        gr = ref[n].grad
        rel = float((p.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5 * gmax))
        worst = max(worst, (n, rel), key=lambda kv: kv[1])
        assert rel <= GRAD_BAR, (n, rel)
    print(f"worst parameter-gradient error: {worst[1]:.2e} ({worst[0]})")


def test_trainer_warning_stats_and_small_images(device, tmp_path, monkeypatch, capsys):
    from ddpm_ood_amd import vqvae_train

    monkeypatch.setenv("DDPM_VQVAE_LOSS_TERMS", "perceptual,spectral")
    vqvae_train._WARNED.clear()
    capsys.readouterr()
    a = vqvae_train.VQVAETrainer(_args(tmp_path, "w1"))
    b = vqvae_train.VQVAETrainer(_args(tmp_path, "w2"))
    err = capsys.readouterr().err
    assert err.count("NOT built") == 1
    line = next(ln for ln in err.splitlines() if "NOT built" in ln)
    assert "adversarial" in line and "LPIPS" not in line and "Jukebox" not in line
    assert err.count("DDPM_LPIPS_WEIGHTS is not set") == 1
    for t in (a, b):
        assert len(t.last_stats["missing_loss_terms"]) == 1 and "adversarial" in t.last_stats["missing_loss_terms"][0]
        assert t.last_stats["optimised_loss"] == "l1 + quantization + 0.001 perceptual + spectral"
    out = a.train_step(a.train_loader.images[:8].to(device))
    assert len(out) == 3 and set(a.last_terms) == {"perceptual", "spectral"}
    assert all(torch.isfinite(v) and v.item() > 0 for v in a.last_terms.values())
    with pytest.raises(ValueError, match=">= 32"):
        vqvae_train.VQVAETrainer(_args(tmp_path, "w3", size=16))
    monkeypatch.setenv("DDPM_VQVAE_LOSS_TERMS", "perceptual,adversarial")
    with pytest.raises(ValueError, match="unknown term"):
        vqvae_train.VQVAETrainer(_args(tmp_path, "w4"))
    monkeypatch.setenv("DDPM_VQVAE_LOSS_TERMS", "spectral")  # the spectral term alone has no size limit
    vqvae_train._WARNED.clear()
    c = vqvae_train.VQVAETrainer(_args(tmp_path, "w5", size=16))
    assert len(c.last_stats["missing_loss_terms"]) == 2 and c.lpips is None and "lpips_pretrained" not in c.last_stats
    c.train_step(c.train_loader.images[:8].to(device))
    assert set(c.last_terms) == {"spectral"}


def test_cli_quick_test_with_both_terms(device, tmp_path):
    import os

    argv = [sys.executable, str(ROOT / "train_vqvae.py"), *_cli(32), "--output_dir", str(tmp_path), "--model_name", "cli",
            "--quick_test", "1", "--n_epochs", "1", "--eval_freq", "1"]
    env = dict(os.environ, DDPM_VQVAE_LOSS_TERMS="perceptual,spectral")
    out = subprocess.run(argv, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr.count("NOT built") == 1
    epoch = next(ln for ln in out.stdout.splitlines() if ln.startswith("Epoch 0:"))
    assert ", perceptual " in epoch and ", spectral " in epoch and "Validation 0" in out.stdout
    ck = torch.load(tmp_path / "cli" / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "best_loss"}
