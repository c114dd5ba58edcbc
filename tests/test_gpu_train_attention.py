"""GPU: train_ops.attention_fwd / attention_bwd (csrc/attention_train.hip) against float64 CPU torch -- softmax over
einsum with autograd -- and beside the GEMM route they stand in for (the five T.gemm calls, softmax_rows_ and
softmax_backward_rows_ exactly as train_native._attn_fwd / _attn_bwd issue them) on the same inputs.

Condition per output (o, dq, dk, dv): err_new <= 4 err_old, err = max |x - ref| / max |ref|.  The 4 is the margin for one more
rescale rounding per key block of the online softmax; it is not a measured number.  lse: absolute error <= 4 fp32 ulp of the
largest |logit| of the case.  Measured figures: profiles/train_attention.md."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 16.0
SHAPES = [(2, 1, 64), (2, 3, 192), (1, 2, 1024)]  # one query tile, two 32-key blocks / N no power of two, head strides / many blocks
FAMILIES = ["plain", "ramp", "shift"]


@functools.lru_cache(maxsize=None)
def _case(B, heads, N, family):
    """(q, k, v, do) fp32 on the CPU and the float64 reference (o, lse, dq, dk, dv, logits); computed once, never modified."""
    g = torch.Generator().manual_seed(N)
    C = heads * 256
    q, k, v, do = (torch.randn(B, C, N, generator=g) for _ in range(4))
    if family == "ramp":  # the running row maximum moves in nearly every key block
        k = k * torch.linspace(0.25, 2, N)
    elif family == "shift":  # a per-row logit offset that only a max-subtracting softmax survives
        k = k + 64 * torch.randn(B, C, 1, generator=g)
    q64, k64, v64 = (t.double().view(B, heads, 256, N).requires_grad_(True) for t in (q, k, v))
    s = SCALE * torch.einsum("bhci,bhcj->bhij", q64, k64)
    o = torch.einsum("bhij,bhcj->bhci", torch.softmax(s, dim=-1), v64)
    o.backward(do.double().view(B, heads, 256, N))
    ref = dict(o=o.detach().reshape(B, C, N), lse=torch.logsumexp(s.detach(), dim=-1), dq=q64.grad.reshape(B, C, N),
               dk=k64.grad.reshape(B, C, N), dv=v64.grad.reshape(B, C, N), s=s.detach())
    return (q, k, v, do), ref


def _gemm_route(q, k, v, do, heads, scale):
    """train_native._attn_fwd / _attn_bwd's core, call for call."""
    from ddpm_ood_amd import train_ops as T

    B, Cc, n = q.shape
    d = Cc // heads
    P = torch.empty((B * heads, n, n), dtype=torch.float32, device=q.device)
    zb = dict(batch=B * heads, batch_inner=heads, a_batch=d * n, a_batch_outer=Cc * n, b_batch=d * n, b_batch_outer=Cc * n)
    T.gemm(q, k, P, n, n, d, a_m=1, a_k=n, b_k=n, b_n=1, c_m=n, c_n=1, c_batch=n * n, c_batch_outer=heads * n * n, alpha=scale, **zb)
    T.softmax_rows_(P, B * heads * n, n)
    o = torch.empty_like(q)
    T.gemm(v, P, o, d, n, n, a_m=n, a_k=1, b_k=1, b_n=n, c_m=n, c_n=1, batch=B * heads, batch_inner=heads, a_batch=d * n,
           a_batch_outer=Cc * n, b_batch=n * n, b_batch_outer=heads * n * n, c_batch=d * n, c_batch_outer=Cc * n)
    zq = dict(batch=B * heads, batch_inner=heads)
    cn = dict(c_m=n, c_n=1)
    dv, dq, dk = torch.empty_like(v), torch.empty_like(q), torch.empty_like(k)
    dP = torch.empty_like(P)
    T.gemm(do, P, dv, d, n, n, a_m=n, a_k=1, b_k=n, b_n=1, a_batch=d * n, a_batch_outer=Cc * n, b_batch=n * n,
           b_batch_outer=heads * n * n, c_batch=d * n, c_batch_outer=Cc * n, **cn, **zq)
    T.gemm(do, v, dP, n, n, d, a_m=1, a_k=n, b_k=n, b_n=1, a_batch=d * n, a_batch_outer=Cc * n, b_batch=d * n,
           b_batch_outer=Cc * n, c_batch=n * n, c_batch_outer=heads * n * n, **cn, **zq)
    T.softmax_backward_rows_(P, dP, B * heads * n, n)
    T.gemm(k, dP, dq, d, n, n, a_m=n, a_k=1, b_k=1, b_n=n, a_batch=d * n, a_batch_outer=Cc * n, b_batch=n * n,
           b_batch_outer=heads * n * n, c_batch=d * n, c_batch_outer=Cc * n, alpha=scale, **cn, **zq)
    T.gemm(q, dP, dk, d, n, n, a_m=n, a_k=1, b_k=n, b_n=1, a_batch=d * n, a_batch_outer=Cc * n, b_batch=n * n,
           b_batch_outer=heads * n * n, c_batch=d * n, c_batch_outer=Cc * n, alpha=scale, **cn, **zq)
    return dict(o=o, dq=dq, dk=dk, dv=dv)


def _err(x, ref):
    return float((x.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ops_are_as_accurate_as_the_gemm_route_and_lse_is_the_logsumexp(device, shape, family):
    from ddpm_ood_amd import train_ops as T

    B, heads, N = shape
    (q, k, v, do), ref = _case(B, heads, N, family)
    row_max = ref["s"].amax(dim=-1).reshape(-1)
    if family == "shift":  # the case is what it claims to be: exp(s) itself would overflow / underflow fp32 in many rows
        assert float((row_max > 88.7).float().mean()) >= 0.05 and float((row_max < -88.7).float().mean()) >= 0.05
    qd, kd, vd, dod = (t.to(device) for t in (q, k, v, do))
    o, lse = T.attention_fwd(qd, kd, vd, heads, SCALE)
    dq, dk, dv = T.attention_bwd(qd, kd, vd, o, dod, lse, heads, SCALE)
    new = dict(o=o, dq=dq, dk=dk, dv=dv)
    # the GEMM route's backward starts from ITS OWN forward, as in the training step
    old = _gemm_route(qd, kd, vd, dod, heads, SCALE)
    torch.cuda.synchronize()
    assert o.shape == (B, heads * 256, N) and lse.shape == (B, heads, N) and lse.dtype == torch.float32
    max_logit = float(ref["s"].abs().max())
    lse_err = float((lse.double().cpu() - ref["lse"]).abs().max())
    lse_bound = 4 * float(np.spacing(np.float32(max_logit)))
    errs = {name: (_err(new[name], ref[name]), _err(old[name], ref[name])) for name in ("o", "dq", "dk", "dv")}
    print(f"\n{B}x{heads}x{N} {family}: " + ", ".join(f"{n_} new {a:.2e} old {b:.2e}" for n_, (a, b) in errs.items())
          + f"; lse {lse_err:.2e} (bound {lse_bound:.2e}, max |logit| {max_logit:.1f})")
    for name, (e_new, e_old) in errs.items():
        assert e_new <= 4 * e_old, (name, e_new, e_old)
    assert lse_err <= lse_bound, (lse_err, lse_bound)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(device, shape):
    from ddpm_ood_amd import train_ops as T

    B, heads, N = shape
    q, k, v, do = (t.to(device) for t in _case(B, heads, N, "ramp")[0])
    o1, l1 = T.attention_fwd(q, k, v, heads, SCALE)
    o2, l2 = T.attention_fwd(q, k, v, heads, SCALE)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1 = T.attention_bwd(q, k, v, o1, do, l1, heads, SCALE)
    g2 = T.attention_bwd(q, k, v, o1, do, l1, heads, SCALE)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_shapes_and_tensors_the_kernels_do_not_take_are_refused(device):
    from ddpm_ood_amd import train_ops as T

    def both(q, k, v, heads):
        with pytest.raises(ValueError):
            T.attention_fwd(q, k, v, heads, SCALE)
        o, lse = torch.zeros_like(q), torch.zeros(q.shape[0], heads, q.shape[-1], device=q.device)
        with pytest.raises(ValueError):
            T.attention_bwd(q, k, v, o, torch.zeros_like(q), lse, heads, SCALE)

    z = lambda *s, dev=device: torch.zeros(*s, device=dev)  # noqa: E731
    both(z(1, 256, 96), z(1, 256, 96), z(1, 256, 96), 1)        # N = 96
    both(z(1, 256, 64), z(1, 256, 64), z(1, 256, 64), 2)        # head dim 128
    both(z(1, 256, 64, dev="cpu"), z(1, 256, 64), z(1, 256, 64), 1)  # a CPU tensor
    both(z(1, 256, 64), z(1, 64, 256).transpose(1, 2), z(1, 256, 64), 1)  # a non-contiguous tensor
    assert not T.attention_takes(256, 96, 1) and not T.attention_takes(256, 64, 2) and T.attention_takes(768, 192, 3)
