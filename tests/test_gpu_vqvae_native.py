"""-m gpu: the VQ-VAE's encoder / decoder training step on the library's kernels (DDPM_VQVAE_NATIVE=1, ddpm_ood_amd/vqvae_native.py):
the gradient range of the input-gradient convolutions, the native forward against the eval path, every parameter gradient against
float64 autograd over the oracle, training progress and the device-kernel trace of a step.  The 2-D model is the CFG of
tests/test_gpu_vqvae_train.py (generic kernels); the 3-D one has 128 channels (MFMA tilings), one down-level, 8 x 12 x 16 inputs."""

import copy

import pytest
import torch
import torch.nn.functional as F

from test_gpu_vqvae_train import CFG, PROGRESS_STEPS, _args, _images

pytestmark = pytest.mark.gpu
GRAD_BAR = 1e-4

CFG3 = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(128,), num_res_layers=1, num_res_channels=(128,),
            downsample_parameters=((2, 4, 1, 1),), upsample_parameters=((2, 4, 1, 1, 0),), num_embeddings=16, embedding_dim=8,
            decay=0.99, commitment_cost=0.25, epsilon=1e-5)


def _volumes(n):
    return torch.rand((n, 1, 8, 12, 16), generator=torch.Generator().manual_seed(21))


def _pair(cfg, images, device):
    """(oracle VQ-VAE on the host, product VQ-VAE on the device), same weights, the codebook spread over the latents' range."""
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.vqvae import VQVAE

    torch.manual_seed(11)
    o = OV(**cfg).eval()
    with torch.no_grad():
        z = o.encode(images)
        dims = (0,) + tuple(range(2, z.ndim))
        o.quantizer.quantizer.embedding.weight.mul_(z.std()).add_(z.mean(dim=dims)[None])
        o.quantizer.quantizer.ema_w.copy_(o.quantizer.quantizer.embedding.weight)
    m = VQVAE(**cfg)
    m.load_state_dict(o.state_dict())
    return o, m.to(device)


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- gradient range ---------------------------------------------------------------------------------------------------------

def _families(fn):
    """fn() with a spy on ddpm_conv_f32 -> (result, the family ddpm_conv_kernel_name reports for every launched descriptor)"""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    real, names = lib.ddpm_conv_f32, []

    def spy(desc, stream):
        names.append(lib.ddpm_conv_kernel_name(desc).decode())
        return real(desc, stream)

    lib.ddpm_conv_f32 = spy
    try:
        return fn(), names
    finally:
        lib.ddpm_conv_f32 = real


@pytest.mark.parametrize("which", ["k3_wino44h", "convT_parity"])
def test_small_upstream_gradients_keep_their_precision(device, monkeypatch, which):
    """A backward whose upstream gradient is 2^-20 times smaller (an L1 loss over a 64^3 volume hands the layers ~4e-6), rescaled by
    2^20, agrees with the unscaled backward to 1e-4 max-norm relative on dx and dw; the unscaled one agrees with PyTorch-ROCm
    autograd on the same device to 1e-4.  The layers' FORWARD kernels are the split-f16 ones, the input-gradient launches of the
    backward are not (both asserted through ddpm_conv_kernel_name).  The ATen reference
    multiplies its pre-activation by the ReLU mask of the native output: the two forwards differ by ~1e-5, so a handful of the
    outputs nearest 0 would otherwise take a gradient on one side only (relu_backward itself is tested bit for bit)."""
    from ddpm_ood_amd import vqvae_native
    from ddpm_ood_amd.vqvae import _Convolution

    monkeypatch.setenv("DDPM_CONV_WINO44", "2")  # lifts the launch-size gate of the F(4x4) kernels (B = 1 of 128 channels is below it)
    torch.manual_seed(5)
    if which == "k3_wino44h":
        layer = _Convolution(3, 128, 128).to(device)
        x = torch.randn((1, 128, 32, 32, 32), device=device)
        aten = lambda t, w, b: F.conv3d(t, w, b, padding=1)  # noqa: E731
    else:
        layer = _Convolution(3, 128, 128, strides=2, kernel_size=4, padding=1, is_transposed=True).to(device)
        x = torch.randn((1, 128, 4, 32, 32), device=device)
        aten = lambda t, w, b: F.conv_transpose3d(t, w, b, stride=2, padding=1)  # noqa: E731
        assert layer._hip_kind(x) == "convT_parity"
    x.requires_grad_(True)
    w, b = layer.conv.weight, layer.conv.bias
    y, names = _families(lambda: vqvae_native.conv_layer(layer, x))
    assert names and set(names) == {"wino44h"}, names  # (the parity form: eight launches of the same family)
    u = torch.randn(y.shape, device=device, generator=torch.Generator(device=device).manual_seed(6))
    full, back = _families(lambda: torch.autograd.grad(y, (x, w, b), u, retain_graph=True))
    split = {"wino44h", "d3s", "d3s2", "s2h", "d1s", "conv1x1_dma"}  # the families that multiply on the f16 MFMA
    assert back and not split & set(back), back  # the input gradient ran, on an fp32 family
    small = torch.autograd.grad(y, (x, w, b), u * 2.0 ** -20)
    ref = torch.autograd.grad(aten(x, w, b) * (y.detach() > 0), (x, w, b), u)
    for name, f, s, r in zip(("dx", "dw", "db"), full, small, ref):
        e_scale, e_ref = _rel(s * 2.0 ** 20, f), _rel(f, r)
        print(f"{which} {name}: scaled vs unscaled {e_scale:.2e}, native vs ATen {e_ref:.2e}")
        assert e_scale <= 1e-4 and e_ref <= 1e-4, (name, e_scale, e_ref)


# ---- the native forward is the eval path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [2, 3])
def test_native_forward_is_the_eval_path(device, monkeypatch, dims):
    from ddpm_ood_amd.vqvae_train import encode_train, vqvae_forward_train

    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    images = _images() if dims == 2 else _volumes(1)
    _, m = _pair(CFG if dims == 2 else CFG3, images, device)
    x = images.to(device)
    with torch.no_grad():
        assert torch.equal(encode_train(m, x), m.encode(x))
        assert torch.equal(vqvae_forward_train(m, x, update_codebook=False)[0], m(x)[0])


# ---- parameter gradients ----------------------------------------------------------------------------------------------------------

def _check_parameter_gradients(o, m, cfg, x, device, extra=None, extra64=None):
    from ddpm_ood_amd.vqvae_train import VQTrainFunction, decode_train, encode_train

    o = copy.deepcopy(o).double()
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(True)
    xd = x.to(device)
    z = encode_train(m, xd)
    qz, qloss, idx, _ = VQTrainFunction.apply(z, m.quantizer.quantizer, False)
    r = decode_train(m, qz)
    total = F.l1_loss(r, xd) + qloss
    if extra is not None:
        total = total + extra(r, xd)
    total.backward()
    assert len(torch.unique(idx)) > 1

    x64 = x.double()
    zo = o.encode(x64)
    e = o.quantizer.quantizer.embedding.weight.detach()[idx.long().cpu()].movedim(-1, 1)
    ro = o.decode(zo + (e - zo).detach())
    lo = F.l1_loss(ro, x64) + cfg["commitment_cost"] * F.mse_loss(e, zo)
    if extra64 is not None:
        lo = lo + extra64(ro, x64)
    lo.backward()
    assert abs(qloss.item() - (cfg["commitment_cost"] * F.mse_loss(e, zo)).item()) <= 2e-6 * lo.item()
    ref = dict(o.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in ref.values() if p.grad is not None)
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        if "embedding" in n:
            assert p.grad is None  # the codebook moves by EMA only
            continue
        gr = ref[n].grad
        rel = float((p.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5 * gmax))
        worst = max(worst, (n, rel), key=lambda kv: kv[1])
        assert rel <= GRAD_BAR, (n, rel)
    print(f"worst parameter-gradient error: {worst[1]:.2e} ({worst[0]})")
    for p in m.parameters():
        p.grad = None


@pytest.mark.parametrize("dims", [2, 3])
def test_parameter_gradients_match_float64_autograd_over_the_oracle(device, monkeypatch, dims):
    """tests/test_gpu_vqvae_train.py's method with the switch on: L1 + quantisation loss, the oracle fed the HIP indices, every
    parameter within 1e-4 max-norm relative, floored at 1e-5 of the model's largest gradient."""
    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    images = _images() if dims == 2 else _volumes(2)
    cfg = CFG if dims == 2 else CFG3
    o, m = _pair(cfg, images, device)
    _check_parameter_gradients(o, m, cfg, images, device)


def test_parameter_gradients_with_the_perceptual_and_spectral_terms(device, tmp_path, monkeypatch):
    """The 2-D CFG at 32 x 32 with DDPM_VQVAE_LOSS_TERMS=perceptual,spectral and the switch on (the method of
    tests/test_gpu_vqvae_loss_terms.py::test_trainer_parameter_gradients_of_the_total_loss)."""
    from oracle.lpips import LPIPSAlex
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.data import synthetic_images
    from ddpm_ood_amd.vqvae_train import VQVAETrainer, encode_train
    from test_gpu_vqvae_loss_terms import _args as _args32

    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    monkeypatch.setenv("DDPM_VQVAE_LOSS_TERMS", "perceptual,spectral")
    tr = VQVAETrainer(_args32(tmp_path, "native_terms"))
    assert tr.loss_terms == ("perceptual", "spectral") and tr.last_stats["conv_gradients"] == "native"
    x = synthetic_images("blobs", 16, 1, 32, seed=1)
    m, q = tr.model, tr.model.quantizer.quantizer
    with torch.no_grad():
        z = encode_train(m, x.to(device))
        q.embedding.weight.mul_(z.std()).add_(z.mean(dim=(0, 2, 3))[None])
    o = OV(**CFG).eval()
    o.load_state_dict(m.state_dict())
    lp = LPIPSAlex()
    lp.load_state_dict(tr.lpips.state_dict())
    lp = lp.double()
    amp = lambda t: torch.fft.fftn(t, dim=(1, 2, 3), norm="ortho").abs()  # noqa: E731
    _check_parameter_gradients(
        o, m, CFG, x, device, extra=lambda r, xd: tr.extra_terms(r, xd)[0],
        extra64=lambda ro, x64: 0.001 * lp(ro, x64, normalize=False).mean() + ((amp(ro) - amp(x64)) ** 2).mean())


# ---- training and trace -------------------------------------------------------------------------------------------------------------

def test_training_makes_progress_and_reports_its_route(device, tmp_path, monkeypatch):
    from ddpm_ood_amd.vqvae_train import VQVAETrainer

    x = _images().to(device)
    tr = VQVAETrainer(_args(tmp_path, "aten", n_epochs=1, checkpoint_every=0))
    tr.train_step(x)
    assert tr.last_stats["conv_gradients"] == "aten"
    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    tr = VQVAETrainer(_args(tmp_path, "native", n_epochs=1, checkpoint_every=0))
    l1 = [float(tr.train_step(x)[1]) for _ in range(PROGRESS_STEPS + 1)]
    print(f"native route, L1 on the fixed batch: step 0 {l1[0]:.6f} -> step {PROGRESS_STEPS} {l1[-1]:.6f}")
    assert tr.last_stats["conv_gradients"] == "native"
    assert l1[-1] < l1[0]
    assert all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_native_step_launches_no_library_convolution(device, tmp_path, monkeypatch):
    """torch.profiler's device-kernel trace of one native step: no MIOpen kernel, no ATen convolution kernel."""
    from torch.profiler import ProfilerActivity, profile

    from ddpm_ood_amd.vqvae_train import VQVAETrainer

    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    tr = VQVAETrainer(_args(tmp_path, "trace", n_epochs=1, checkpoint_every=0))
    x = _images().to(device)
    tr.train_step(x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tr.train_step(x)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
    if not names:
        pytest.skip("torch.profiler recorded no device kernels on this box")
    foreign = [n for n in names if "ddpm" not in n and any(k in n.lower() for k in ("conv", "igemm", "cijk", "im2col", "col2im",
                                                                                    "vol2col", "col2vol"))]
    ours = [n for n in names if "ddpm" in n]
    print(f"native VQ-VAE step: {len(names)} distinct device kernels, {len(ours)} of this library")
    assert not foreign, foreign
    assert any("k4s2_wgrad" in n for n in ours) and any("relu_bwd" in n for n in ours), ours
