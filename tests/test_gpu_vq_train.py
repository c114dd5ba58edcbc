"""-m gpu: the training step of the EMA quantiser on its HIP kernels (vq.hip: ddpm_vq_train_{assign,update,backward}_f32)
against a float64 restatement of the formulas in include/ddpm_ood_hip.h (MONAI-Generative's EMAQuantizer in training mode).

The restatement is fed the indices the HIP kernel returned (they are checked separately, bit for bit, against
``ops.vq_nearest``), so a near-tie cannot flip a comparison.  Bounds are per entry and derived from the data inside the test:
  * dw[k, d]: recursive summation in fp32, count_k * 2^-24 * sum |x[p, d]| over the positions assigned to k;
  * ema_w / codebook: that bound through ``ema_w <- decay ema_w + (1 - decay) dw`` and the division by w_k, plus 4 ulp (fp32
    spacing) of the float64 result;
  * loss: 2e-6 relative (what tests/test_gpu_train_ops.py holds mse_loss_grad to); dx: 4 ulp of its largest term.
The state of the quantiser IS three fp32 buffers, so in the chained run every step's restatement starts from the fp32 state the
device carries into that step (read back exactly), and each of the three steps is held to the one-step bound.  The constants
are the fp32 values the kernels receive."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CC = 0.25
DECAY = float(np.float32(0.99))
EPS = float(np.float32(1e-5))


def _ulp(v: torch.Tensor) -> torch.Tensor:
    """fp32 spacing at |v| (float64 in, float64 out)."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def _flat(x: torch.Tensor) -> torch.Tensor:
    """[B, D, *S] -> [B S, D] float64 on the host"""
    return x.detach().cpu().double().movedim(1, -1).reshape(-1, x.shape[1])


def _restate(x64, idx, E, cs, emaw, K):
    """One training step in float64 -> dict of everything the kernels produce (+ the per-entry dw bound)."""
    q = E[idx]
    counts = torch.bincount(idx, minlength=K).double()
    dw = torch.zeros_like(E).index_add_(0, idx, x64)
    absx = torch.zeros_like(E).index_add_(0, idx, x64.abs())
    cs1 = DECAY * cs + (1 - DECAY) * counts
    n = cs1.sum()
    w = (cs1 + EPS) / (n + K * EPS) * n
    emaw1 = DECAY * emaw + (1 - DECAY) * dw
    return dict(q=q, counts=counts, dw=dw, dw_bound=counts[:, None] * U * absx, cs=cs1, w=w, ema_w=emaw1,
                codebook=emaw1 / w[:, None], loss=CC * ((q - x64) ** 2).mean())


def _codebook(case, K, D, g):
    E = torch.randn(K, D, generator=g)
    if case == "far":        # rows 2 and 3 far from the data: dead codes
        E[2:] += 100.0
    elif case == "one":      # every position nearest to row 0
        E[0] = 0.0
        E[1:] += 50.0
    elif case == "copy":     # row 1 a copy of row 0: row 0 wins every tie
        E[1] = E[0]
    return E


CASES = [
    (2, 8, (5, 7), 5, "random"),          # templated D; K not a multiple of the four-wave split; 70 positions: ragged last workgroup
    (3, 3, (3, 3, 3), 7, "random"),       # generic D; odd everything
    (1, 128, (4, 4, 4), 2048, "random"),  # the README codebook; 64 positions; most codes dead
    (2, 16, (8, 8), 4, "far"),
    (2, 16, (8, 8), 4, "one"),
    (2, 16, (8, 8), 4, "copy"),
]


@pytest.mark.parametrize("B,D,spatial,K,case", CASES, ids=[f"{c[0]}x{c[1]}x{'x'.join(map(str, c[2]))}-K{c[3]}-{c[4]}" for c in CASES])
def test_vq_train_step_matches_float64(device, B, D, spatial, K, case):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(1000 * K + D)
    E0 = _codebook(case, K, D, g)
    # the module's initial state has zero cluster sizes (README case: the epsilon path); the others start from non-zero sizes so
    # that "a dead code only decays" compares against something
    cs0 = torch.zeros(K) if K == 2048 else torch.rand(K, generator=g) + 0.5
    E, cs, emaw = E0.clone().to(device), cs0.clone().to(device), E0.clone().to(device)
    N = B * int(np.prod(spatial))
    scale = 0.1 if case == "one" else 1.0
    for step in range(3):
        x = (torch.randn(B, D, *spatial, generator=g) * scale).to(device)
        before = dict(E=E.clone(), cs=cs.clone(), emaw=emaw.clone())
        idx_n, out_n = ops.vq_nearest(x, E)
        idx, out, counts, dw, loss, sums = ops.vq_train_assign(x, E, CC)
        # the search is the eval path's, bit for bit
        assert idx.dtype == torch.int32 and idx.shape == idx_n.shape
        assert torch.equal(idx.long(), idx_n) and torch.equal(out, out_n)
        # counts and dw share one allocation (one all_reduce between assign and update)
        assert sums.numel() == K * (D + 1) and counts.data_ptr() == sums.data_ptr() and dw.data_ptr() == sums[K:].data_ptr()
        flat_idx = idx.reshape(-1).long().cpu()
        assert torch.equal(counts.cpu(), torch.bincount(flat_idx, minlength=K).float()) and float(counts.sum()) == N
        # a second call from identical state: bit-identical sums and loss
        idx2, out2, counts2, dw2, loss2, _ = ops.vq_train_assign(x, E, CC)
        assert torch.equal(dw, dw2) and torch.equal(loss, loss2) and torch.equal(counts, counts2) and torch.equal(idx, idx2)
        x64 = _flat(x)
        ref = _restate(x64, flat_idx, before["E"].cpu().double(), before["cs"].cpu().double(), before["emaw"].cpu().double(), K)
        assert torch.isfinite(dw).all() and torch.isfinite(loss)
        err = (dw.cpu().double() - ref["dw"]).abs()
        assert bool((err <= ref["dw_bound"]).all()), f"step {step}: dw off by up to {(err - ref['dw_bound']).max():.3e} over the bound"
        rel = abs(float(loss) - float(ref["loss"])) / float(ref["loss"])
        print(f"step {step}: loss {float(loss):.7g} (float64 {float(ref['loss']):.7g}, rel {rel:.2e}); worst dw error / bound "
              f"{(err / ref['dw_bound'].clamp_min(1e-300))[ref['dw_bound'] > 0].max().item() if (ref['dw_bound'] > 0).any() else 0:.3f}")
        assert rel < 2e-6
        # backward against float64 autograd through the restatement (straight-through + commitment wired by hand)
        dout, dloss = torch.randn(x.shape, generator=g), torch.randn((), generator=g)
        xa = x.detach().cpu().double().requires_grad_(True)
        qa = ref["q"].reshape(B, *spatial, D).movedim(-1, 1)
        total = ((xa + (qa - xa).detach()) * dout.double()).sum() + CC * ((qa.detach() - xa) ** 2).mean() * dloss.double()
        (dx_ref,) = torch.autograd.grad(total, xa)
        dx = ops.vq_train_backward(dout.to(device), x, before["E"], idx, dloss.to(device), CC)
        term = torch.maximum(dout.double().abs(), (dx_ref - dout.double()).abs())
        assert bool(((dx.cpu().double() - dx_ref).abs() <= 4 * _ulp(term)).all())
        # the update: in place, one launch; twice from identical state -> identical bits
        twin = dict(E=E.clone(), cs=cs.clone(), emaw=emaw.clone())
        ops.vq_train_update(cs, emaw, E, counts, dw, DECAY, EPS)
        ops.vq_train_update(twin["cs"], twin["emaw"], twin["E"], counts, dw, DECAY, EPS)
        assert torch.equal(E, twin["E"]) and torch.equal(cs, twin["cs"]) and torch.equal(emaw, twin["emaw"])
        for t in (E, cs, emaw):
            assert torch.isfinite(t).all()
        dead = (counts == 0).cpu()
        if case in ("far", "one") or K == 2048:
            assert bool(dead.any())
        if case == "copy" and step == 0:  # (the first update moves the two rows apart: their cluster sizes differ)
            assert float(counts[1]) == 0 and float(counts[0]) > 0
        if case == "one":
            assert float(counts[0]) == N
        # dead codes only decay
        assert torch.equal(cs.cpu()[dead], (torch.tensor(DECAY, dtype=torch.float32) * before["cs"].cpu())[dead])
        assert bool(((cs.cpu().double() - ref["cs"]).abs() <= 4 * _ulp(ref["cs"])).all())
        b_emaw = (1 - DECAY) * ref["dw_bound"]
        assert bool(((emaw.cpu().double() - ref["ema_w"]).abs() <= b_emaw + 4 * _ulp(ref["ema_w"])).all())
        e_err = (E.cpu().double() - ref["codebook"]).abs()
        e_bound = b_emaw / ref["w"][:, None] + 4 * _ulp(ref["codebook"])
        assert bool((e_err <= e_bound).all()), f"step {step}: codebook off by up to {(e_err / e_bound).max():.2f} x the bound"
        assert not torch.equal(E, before["E"])
        # the eval search sees the updated codebook (code norms are recomputed per call, not cached): its choice is the nearest
        # code of the NEW codebook in float64, up to a near-tie
        idx_new, _ = ops.vq_nearest(x, E)
        d = ((x64 ** 2).sum(1, keepdim=True) - 2.0 * x64 @ E.cpu().double().t() + (E.cpu().double() ** 2).sum(1)[None])
        chosen = d.gather(1, idx_new.reshape(-1, 1).cpu()).squeeze(1)
        assert bool((chosen - d.min(1).values <= 1e-5 * d.min(1).values.abs().clamp_min(1e-12)).all())


def test_update_codebook_false_leaves_the_state_untouched(device):
    from ddpm_ood_amd.vqvae import _EMAQuantizer
    from ddpm_ood_amd.vqvae_train import VQTrainFunction

    torch.manual_seed(3)
    q = _EMAQuantizer(16, 8, commitment_cost=CC, decay=DECAY, epsilon=EPS).to(device)
    q.ema_cluster_size.add_(1.0)
    state = [t.clone() for t in (q.embedding.weight.data, q.ema_cluster_size, q.ema_w)]
    x = torch.randn(2, 8, 6, 6, device=device, requires_grad=True)
    out, loss, idx, counts = VQTrainFunction.apply(x, q, False)
    (out.sum() + loss).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    for a, b in zip(state, (q.embedding.weight.data, q.ema_cluster_size, q.ema_w)):
        assert torch.equal(a, b)
    out2, loss2, _, _ = VQTrainFunction.apply(x.detach(), q, True)
    assert torch.equal(out, out2) and torch.equal(loss, loss2)  # outputs and loss belong to the codebook as it was
    assert not torch.equal(state[0], q.embedding.weight.data) and not torch.equal(state[1], q.ema_cluster_size)
