"""GPU: DDPM_TRAIN_ATTN=recompute through train_native.NativeUNetStep: gradient parity with ATen autograd at the
bar of tests/test_gpu_train.py, which blocks took which route, what the tape holds, the peak memory of a step beside the GEMM
route, the no-tape forward, and the default."""

import pytest
import torch

pytestmark = pytest.mark.gpu

MiB = 1 << 20


def _model(device, dims, channels, cfg, sd):
    from ddpm_ood_amd import DiffusionModelUNet

    m = DiffusionModelUNet(dims, channels, channels, **cfg)
    m.load_state_dict(sd)
    return m.to(device).train()


def _batch(device, B, channels, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    shape = (B, channels, H, W)
    return (torch.rand(shape, generator=g).to(device), torch.randint(0, 1000, (B,), generator=g).to(device),
            torch.randn(shape, generator=g).to(device))


def _big(device):
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    return _model(device, 2, 3, MODEL_CONFIGS["big"], random_state_dict("big", 3, spatial_dims=2, seed=1))


def _two_level(device):
    """256 / 512 channels, attention on both levels, one ResnetBlock each, head channels 256: on 16 x 24 images the blocks see
    N = 384 (one head) and N = 96 (two heads: not a multiple of 64)."""
    from ddpm_ood_amd.synthetic import random_state_dict

    cfg = dict(num_channels=(256, 512), attention_levels=(True, True), num_res_blocks=1, num_head_channels=256)
    sd = random_state_dict(channels=1, spatial_dims=2, seed=11, config=cfg)
    return _model(device, 2, 1, cfg, sd), lambda: _model(device, 2, 1, cfg, sd)


def _parity(ref, step, x, t, noise, deterministic_ref=False):
    """test_native_step_matches_aten_autograd_on_other_unets' comparison."""
    from ddpm_ood_amd.train import unet_forward_torch

    for p in ref.parameters():
        p.requires_grad_(True)
    # The autograd reference sums some of its gradients with atomics.  to_k.bias has an analytically zero gradient, so there the
    # comparison is between two roundings, and on the 16 x 24 images the reference's own one moves between 3e-5 and 9e-5 of the
    # norm below from run to run (either attention route then lands between 4e-5 and 1.1e-4).  With its deterministic kernels the
    # same reference gives the same bits every time; the native step is deterministic anyway.  (`big` on 64 x 64 sums seven
    # times the pixels: 1.5e-5 either way, and its deterministic reference takes 10 s longer.)
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    if deterministic_ref:
        torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        loss_r = torch.nn.functional.mse_loss(unet_forward_torch(ref, x, t), noise)
        loss_r.backward()
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])
    with torch.no_grad():
        loss_h = step.loss_and_grads(x, t, noise)
    assert abs(loss_h.item() - loss_r.item()) <= 2e-5 * abs(loss_r.item())
    pr, ph = dict(ref.named_parameters()), dict(step.model.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in pr.values() if p.grad is not None)
    worst = ("", 0.0)
    for k in pr:
        if pr[k].grad is None:
            assert float(ph[k].grad.abs().max()) == 0.0, k
            continue
        rel = float((ph[k].grad - pr[k].grad).abs().max() / max(float(pr[k].grad.abs().max()), 1e-5 * gmax))
        worst = max(worst, (k, rel), key=lambda kv: kv[1])
        assert rel <= 1e-4, (k, rel)
    print(f"loss {loss_r.item():.6f}, worst gradient error {worst[1]:.2e} ({worst[0]})")


def test_two_level_unet_gradients_match_autograd_and_routes_are_per_block(device, monkeypatch):
    from ddpm_ood_amd.train_native import NativeUNetStep

    monkeypatch.setenv("DDPM_TRAIN_ATTN", "recompute")
    ref, again = _two_level(device)
    x, t, noise = _batch(device, 3, 1, 16, 24)
    with torch.no_grad():
        step = NativeUNetStep(again())
    _parity(ref, step, x, t, noise, deterministic_ref=True)
    # down level 0, down level 1, middle, up level 1 (two blocks), up level 0 (two blocks)
    assert step.attn_routes == [("recompute", 1, 384), ("gemm", 2, 96), ("gemm", 2, 96), ("gemm", 2, 96), ("gemm", 2, 96),
                                ("recompute", 1, 384), ("recompute", 1, 384)]


def _tensors(obj, seen):
    """Every tensor reachable from a tape entry."""
    if isinstance(obj, torch.Tensor):
        seen.append(obj)
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _tensors(o, seen)


def test_big_unet_gradients_match_autograd_and_the_tape_holds_no_n_by_n_tensor(device, monkeypatch):
    from ddpm_ood_amd.train_native import NativeUNetStep

    monkeypatch.setenv("DDPM_TRAIN_ATTN", "recompute")
    B = 2
    x, t, noise = _batch(device, B, 3, 64, 64)
    with torch.no_grad():
        step = NativeUNetStep(_big(device))
        step.forward(x, t)
        routes = list(step.attn_routes)
        assert routes and all(r == "recompute" for r, _, _ in routes)
        assert {(h, n) for _, h, n in routes} == {(1, 4096), (2, 1024), (3, 256)}
        # (An attention entry's own tensors are the measure: q at N = 256 has heads * 256 * N = heads * N^2 elements itself, and
        # a level-0 concatenation outgrows the N^2 tensor of level 2, so the bound is taken per block against what the block put
        # on the tape, and the level-0 size against everything reachable.)
        entries = [ctx for kind, ctx in step._tape if kind == "attn"]
        assert len(entries) == len(routes)
        for ctx, (_, h, n) in zip(entries, routes):
            own = []
            _tensors(ctx, own)
            assert len(own) >= 6  # xn, q, k, v, o, lse and the GroupNorm context
            for a in own:
                assert a.numel() <= B * h * 256 * n, (tuple(a.shape), h, n)  # nothing larger than an activation of the block
                assert not (a.ndim >= 2 and a.shape[-1] == n and a.shape[-2] == n), tuple(a.shape)
            assert any(a.shape == (B, h, n) for a in own)  # the row statistic
        held = []
        _tensors(step._tape, held)
        assert len(held) > 100 and max(a.numel() for a in held) < B * 4096 * 4096
        step._tape = None
    _parity(_big(device), step, x, t, noise)


def test_a_step_of_big_peaks_at_least_512_mib_lower(device, monkeypatch):
    """The GEMM route holds five level-0 P tensors and one dP of 64 MiB per image at the start of the backward; the new route
    holds five o tensors of 4 MiB per image and the row statistics instead: at B = 2 at least 4 B 64 MiB less."""
    from ddpm_ood_amd.train_native import NativeUNetStep

    B = 2
    x, t, noise = _batch(device, B, 3, 64, 64)
    peaks = {}
    for route in ("gemm", "recompute"):
        monkeypatch.setenv("DDPM_TRAIN_ATTN", route)
        with torch.no_grad():
            step = NativeUNetStep(_big(device))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step.loss_and_grads(x, t, noise)
            torch.cuda.synchronize()
            peaks[route] = torch.cuda.max_memory_allocated()
        assert all(r == route for r, _, _ in step.attn_routes)
        del step
        torch.cuda.empty_cache()
    print(f"peak of one step of big at B = {B}: gemm {peaks['gemm'] / MiB:.0f} MiB, recompute {peaks['recompute'] / MiB:.0f} MiB")
    assert peaks["gemm"] - peaks["recompute"] >= 4 * B * 64 * MiB, peaks


@pytest.mark.parametrize("route", ["gemm", "recompute"])
def test_no_tape_forward_returns_the_taped_bits_and_keeps_nothing(device, monkeypatch, route):
    from ddpm_ood_amd.train_native import NativeUNetStep

    monkeypatch.setenv("DDPM_TRAIN_ATTN", route)
    _, again = _two_level(device)
    x, t, _ = _batch(device, 3, 1, 16, 24)
    with torch.no_grad():
        step = NativeUNetStep(again())
        taped = step.forward(x, t).clone()
        assert step._tape
        free = step.forward(x, t, keep_tape=False)
        assert not step._tape  # also the earlier forward's tape is gone
        assert torch.equal(taped, free)
        assert {r for r, _, _ in step.attn_routes} == ({"gemm"} if route == "gemm" else {"gemm", "recompute"})


def test_default_is_the_gemm_route(device, monkeypatch):
    from ddpm_ood_amd.train_native import NativeUNetStep

    monkeypatch.delenv("DDPM_TRAIN_ATTN", raising=False)
    _, again = _two_level(device)
    x, t, _ = _batch(device, 3, 1, 16, 24)
    with torch.no_grad():
        step = NativeUNetStep(again())
        assert step.attn_route == "gemm"
        step.forward(x, t, keep_tape=False)
    assert len(step.attn_routes) == 7 and all(r == "gemm" for r, _, _ in step.attn_routes)
    monkeypatch.setenv("DDPM_TRAIN_ATTN", "flash")
    with pytest.raises(ValueError, match="DDPM_TRAIN_ATTN"):
        NativeUNetStep(again())
