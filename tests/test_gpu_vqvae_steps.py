"""-m gpu: VQ-VAE training (DDPM_VQVAE_NATIVE=1) over CONSECUTIVE optimiser steps -- tests/test_gpu_vqvae_native.py checks the
native forward and the parameter gradients on freshly loaded weights only.  After two real Adam steps (the trainer's loss, L1 +
quantisation, and its learning rate) the eval path's packed weights must have followed the update (the native forward IS the eval
path, bit for bit), the parameter gradients are held to the same 1e-4 against a float64 oracle loaded from the updated
state_dict, and the EMA codebook state is carried from step to step and follows the float64 restatement of
tests/test_gpu_vq_train.py at that test's bounds.

The case proves that it can see a stale weight form: on the float64 oracle alone, the gradient at the parameters after step 1
differs from the one after step 2 (same batch) by >= 1e-2 -- 100 x the bar -- in more than half of the parameter tensors
(measured on the host without the codebook's EMA movement: 96 % of the tensors, median 0.17, for the 2-D model; 100 %, median
0.96, for the 3-D one)."""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_vq_train import DECAY, _flat, _restate, _ulp
from test_gpu_vqvae_native import CFG, CFG3, _check_parameter_gradients, _images, _pair, _volumes

pytestmark = pytest.mark.gpu

LR = 3e-4  # train_vqvae.py's --vqvae_learning_rate default: the trainer's
SENSITIVITY = 1e-2
STEPS = 2


def _oracle_gradients(cfg, sd, x64):
    """float64 autograd over the oracle's layers from a state_dict, the nearest code chosen in float64 -> {name: gradient}."""
    from oracle.vqvae import VQVAE as OV

    o = OV(**cfg).double()
    o.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu() for k, v in sd.items()})
    zo = o.encode(x64)
    E = o.quantizer.quantizer.embedding.weight.detach()
    flat = zo.detach().movedim(1, -1).reshape(-1, zo.shape[1])
    d = (flat * flat).sum(1, keepdim=True) - 2.0 * flat @ E.t() + (E * E).sum(1)[None]
    e = E[d.argmin(1).reshape(zo.shape[0], *zo.shape[2:])].movedim(-1, 1)
    ro = o.decode(zo + (e - zo).detach())
    (F.l1_loss(ro, x64) + cfg["commitment_cost"] * F.mse_loss(e, zo)).backward()
    return {n: p.grad for n, p in o.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("dims", [2, 3])
def test_two_optimiser_steps_then_the_eval_path_the_gradients_and_the_codebook(device, monkeypatch, dims):
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd import ops
    from ddpm_ood_amd.vqvae_train import encode_train, vqvae_forward_train

    monkeypatch.setenv("DDPM_VQVAE_NATIVE", "1")
    images = _images() if dims == 2 else _volumes(2)
    cfg = CFG if dims == 2 else CFG3
    _, m = _pair(cfg, images, device)
    x = images.to(device)
    q = m.quantizer.quantizer
    K = cfg["num_embeddings"]
    assert float(q.decay) == pytest.approx(DECAY) and float(q.commitment_cost) == 0.25
    codebook = q.embedding.weight
    codebook.requires_grad_(False)  # moved by the EMA update only (vqvae_train.VQVAETrainer)
    params = [p for p in m.parameters() if p is not codebook]
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=LR)
    with torch.no_grad():  # packs the eval path's weight forms BEFORE the first update: they have to follow it
        z0 = m.encode(x)
        m(x)
        # the EMA state of a run under way: every code carries an equal share of the batch's positions (a fresh module's zero
        # cluster sizes divide the first update by epsilon -- the codes scatter and one of them takes every position afterwards,
        # which leaves the straight-through gradient nothing to tell apart)
        share = z0.numel() / z0.shape[1] / K
        q.ema_cluster_size.fill_(share)
        q.ema_w.copy_(codebook.data * share)

    seen = []
    real = ops.vq_train_assign

    def spy(z, e, cc):
        out = real(z, e, cc)
        seen.append((z.detach().clone(), out[0].detach().clone()))
        return out

    monkeypatch.setattr(ops, "vq_train_assign", spy)
    state = lambda: [t.detach().clone() for t in (codebook.data, q.ema_cluster_size, q.ema_w)]  # noqa: E731
    snaps, carried = [], None
    for step in range(STEPS):
        before = state()
        if carried is not None:  # what step k left is what step k + 1 starts from
            assert all(torch.equal(a, b) for a, b in zip(carried, before))
        opt.zero_grad(set_to_none=True)
        r, qloss = vqvae_forward_train(m, x, update_codebook=True)
        (F.l1_loss(r.float(), x.float()) + qloss).backward()
        opt.step()
        carried = state()
        snaps.append({k: v.detach().clone() for k, v in m.state_dict().items()})
        # the EMA state against the float64 restatement fed the HIP indices, from the fp32 state the device carried into the step
        assert len(seen) == step + 1
        z, idx = seen[step]
        flat_idx = idx.reshape(-1).long().cpu()
        ref = _restate(_flat(z), flat_idx, *(t.cpu().double() for t in before), K)
        E, cs, emaw = (t.cpu().double() for t in carried)
        assert bool(((cs - ref["cs"]).abs() <= 4 * _ulp(ref["cs"])).all()), step
        b_emaw = (1 - DECAY) * ref["dw_bound"]
        assert bool(((emaw - ref["ema_w"]).abs() <= b_emaw + 4 * _ulp(ref["ema_w"])).all()), step
        e_err, e_bound = (E - ref["codebook"]).abs(), b_emaw / ref["w"][:, None] + 4 * _ulp(ref["codebook"])
        assert bool((e_err <= e_bound).all()), f"step {step}: codebook off by up to {(e_err / e_bound).max():.2f} x the bound"
        assert not torch.equal(carried[0], before[0]) and len(torch.unique(flat_idx)) > 1
    monkeypatch.setattr(ops, "vq_train_assign", real)
    assert all(not torch.equal(snaps[0][k], snaps[1][k]) for k, _ in m.named_parameters())  # every tensor moved in step 2

    # the sensitivity condition, on the oracle alone
    x64 = images.double()
    cur, stale = _oracle_gradients(cfg, snaps[1], x64), _oracle_gradients(cfg, snaps[0], x64)
    gmax = max(float(g.abs().max()) for g in cur.values())
    d = sorted(float((stale[k] - g).abs().max() / max(float(g.abs().max()), 1e-5 * gmax)) for k, g in cur.items())
    share = sum(v >= SENSITIVITY for v in d) / len(d)
    print(f"dims {dims}: the oracle's gradient after step 1 differs from the one after step 2 by >= {SENSITIVITY} in {share:.0%} of "
          f"the tensors (median {d[len(d) // 2]:.3g})")
    assert share > 0.5, f"the case cannot tell updated from stale parameters: {share:.0%} of the tensors, median {d[len(d) // 2]:.3g}"

    # the eval path's packed weights followed the updates
    with torch.no_grad():
        assert torch.equal(encode_train(m, x), m.encode(x))
        assert torch.equal(vqvae_forward_train(m, x, update_codebook=False)[0], m(x)[0])
    # and so did everything the native backward reads
    o = OV(**cfg).eval()
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    _check_parameter_gradients(o, m, cfg, images, device)
