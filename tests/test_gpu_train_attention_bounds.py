"""GPU: train_ops.attention_fwd / attention_bwd (csrc/attention_train.hip) on the guard-band arena of tests/guard_util.py: inputs
frozen, every buffer the wrappers allocate poisoned (then zeroed), every pointer inside the arena -- nothing is written outside
the outputs, no result depends on what a buffer held, and the allocations are exactly the closed forms of the header
(q-sized tensors of B C N floats, row statistics of B heads N floats; no workspace)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 16.0


@pytest.mark.parametrize("shape", [(2, 1, 64), (1, 3, 192)], ids=lambda s: "x".join(map(str, s)))
def test_the_two_ops_stay_inside_their_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import train_ops as T

    B, heads, N = shape
    C = heads * 256
    g = torch.Generator().manual_seed(B * 1000 + N)
    q, k, v, do = (torch.randn(B, C, N, generator=g) for _ in range(4))
    big, row = B * C * N, B * heads * N

    inputs = dict(q=(q, True), k=(k, True), v=(v, True))
    plain, poison = _bounds(device, inputs, lambda t: T.attention_fwd(t["q"], t["k"], t["v"], heads, SCALE))
    assert [a.numel() for a in poison.allocated] == [big, row]  # o, lse
    assert [name for name, _ in poison.called] == ["ddpm_attention_train_fwd_f32"]
    o, lse = (x.cpu() for x in plain.res)
    s = SCALE * torch.einsum("bhci,bhcj->bhij", q.double().view(B, heads, 256, N), k.double().view(B, heads, 256, N))
    want = torch.einsum("bhij,bhcj->bhci", torch.softmax(s, -1), v.double().view(B, heads, 256, N)).reshape(B, C, N)
    assert float((o.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())

    inputs = dict(q=(q, True), k=(k, True), v=(v, True), o=(o, True), do=(do, True), lse=(lse, True))
    plain, poison = _bounds(device, inputs,
                            lambda t: T.attention_bwd(t["q"], t["k"], t["v"], t["o"], t["do"], t["lse"], heads, SCALE))
    assert [a.numel() for a in poison.allocated] == [big, big, big, row]  # dq, dk, dv, delta
    assert [name for name, _ in poison.called] == ["ddpm_attention_train_bwd_f32"]
    assert all(x.shape == (B, C, N) for x in plain.res)
