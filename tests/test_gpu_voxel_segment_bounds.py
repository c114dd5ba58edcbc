"""GPU: the two ops of csrc/segment3d.hip on the guard-band arena of tests/guard_util.py: inputs frozen, every buffer the wrappers
allocate -- outputs and scratch -- poisoned (then zeroed), every pointer inside the arena: nothing is written outside the buffers,
no result depends on what a buffer held, and the scratch is exactly what the size function answers."""

import numpy as np
import pytest
import torch

import pixel_ref
import voxel_ref
import voxel_segment_ref as ref

pytestmark = pytest.mark.gpu

LO, HI, NBINS = -16.0, 48.0, 4096
THRESHOLDS = [2.0, 3.0, 40.0, float("nan"), -20.0]


def _words(nbytes):
    return (nbytes + 7) // 8  # the wrappers take the scratch as int64 words


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 2, 3, 130), (1, 9, 17, 65)], ids=lambda s: "x".join(map(str, s)))
def test_the_two_ops_stay_inside_their_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    N, D, H, W = shape
    P = D * H * W
    v, _ = pixel_ref.case_values(N, P, LO, HI, NBINS, seed=H)  # (NaN and +-inf among them)
    v = v.reshape(N, D, H, W)
    m = voxel_ref.random_masks(N, D, H, W, 0.25, seed=W)
    m[:, :, H // 2:] = 0

    finite = np.nan_to_num(v, nan=0.5, posinf=60.0, neginf=-60.0)  # (a poison that leaked would show as the one NaN of the result)
    plain, poison = _bounds(device, dict(v=(torch.from_numpy(finite), True)), lambda t: ops.map_median3d(t["v"], 3))
    assert ref.same_values(plain.res[0].cpu().numpy(), ref.median(finite))
    assert [a.numel() for a in poison.allocated] == [N * P]  # out
    assert [name for name, _ in poison.called] == ["ddpm_map_median3d_f32"]

    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    K = len(THRESHOLDS)
    scratch_words = _words(ops.map_segment3d_scratch_bytes(N, D, H, W, K))
    for min_size, conn in ((1, 26), (4, 6)):
        labels, regions = ref.label(m, conn)
        inputs = dict(v=(torch.from_numpy(v), True), m=(torch.from_numpy(m), True), l=(torch.from_numpy(labels), True),
                      r=(torch.from_numpy(regions), True), thr=(thr, True))
        plain, poison = _bounds(device, inputs, lambda t: ops.map_segment3d(t["v"], t["m"], t["l"], t["r"], t["thr"], min_size, conn),
                                size_fns=["ddpm_regions3d_segment_scratch_bytes"], size_of=_words)
        for got, want in zip(plain.res, ref.segment(v, m, labels, regions, THRESHOLDS, min_size, conn)):
            assert np.array_equal(got.cpu().numpy(), want)
        assert sorted(a.numel() for a in poison.allocated) == sorted([N * K * P, N * K * 3, N * K * 3, N * K * 2, scratch_words])
        assert [name for name, _ in poison.called] == ["ddpm_regions3d_segment_scratch_bytes", "ddpm_map_segment3d_f32"]


def test_every_refusal_returns_minus_one_without_a_launch(device):
    """With real buffers, between two reads of the outputs: a refused call leaves them as they were."""
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    N, D, H, W, K = 1, 4, 5, 6, 2
    m = torch.ones((N, D, H, W), dtype=torch.uint8, device=device)
    v = torch.ones((N, D, H, W), dtype=torch.float32, device=device)
    labels = torch.ones((N, D, H, W), dtype=torch.int32, device=device)
    regions = torch.ones((N,), dtype=torch.int32, device=device)
    thr = torch.zeros((K,), dtype=torch.float32, device=device)
    out = torch.full((N, D, H, W), -3.0, dtype=torch.float32, device=device)
    seg = torch.full((N, K, D, H, W), 7, dtype=torch.uint8, device=device)
    pixels = torch.full((N, K, 3), -3, dtype=torch.int32, device=device)
    components = torch.full((N, K, 3), -3, dtype=torch.int32, device=device)
    removed = torch.full((N, K, 2), -3, dtype=torch.int32, device=device)
    scratch = torch.full((1 << 12,), -3, dtype=torch.int64, device=device)
    assert 0 < ops.map_segment3d_scratch_bytes(N, D, H, W, K) <= 8 * scratch.numel()
    s = _lib.stream_ptr()
    p = lambda t: t.data_ptr()  # noqa: E731

    def segment(maps=p(v), n=N, d=D, k=K, min_size=1, conn=26, seg_=p(seg), pixels_=p(pixels), removed_=p(removed), scratch_=p(scratch)):
        return lib.ddpm_map_segment3d_f32(maps, p(m), p(labels), p(regions), n, d, H, W, p(thr), k, min_size, conn, seg_, pixels_,
                                          p(components), removed_, scratch_, s)

    refused = [
        lib.ddpm_map_median3d_f32(p(v), p(out), 5, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), p(out), 1, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), p(v), 3, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), p(v) + 16, 3, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), p(out) + 2, 3, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), None, 3, N, D, H, W, s),
        lib.ddpm_map_median3d_f32(p(v), p(out), 3, N, 0, H, W, s),
        segment(min_size=0), segment(min_size=-5), segment(conn=8), segment(k=0), segment(k=9), segment(d=0), segment(n=65535),
        segment(scratch_=None), segment(scratch_=p(scratch) + 2), segment(seg_=p(v)), segment(pixels_=p(components) + 4),
        segment(scratch_=p(labels)), segment(removed_=p(scratch) + 64), segment(seg_=p(scratch)),
    ]
    assert refused == [-1] * len(refused)
    assert ops.map_segment3d_scratch_bytes(N, 0, H, W, K) == 0 and ops.map_segment3d_scratch_bytes(N, D, H, W, 9) == 0
    torch.cuda.synchronize()
    for t, fill in ((out, -3.0), (seg, 7), (pixels, -3), (components, -3), (removed, -3), (scratch, -3), (v, 1.0), (labels, 1)):
        assert bool((t == fill).all())
    for call in (lambda: ops.map_median3d(v, 5), lambda: ops.map_median3d(v, True), lambda: ops.map_median3d(v[0], 3),
                 lambda: ops.map_median3d(v, 3, out=v), lambda: ops.map_median3d(v.cpu(), 3),
                 lambda: ops.map_segment3d(v, m, labels, regions, [2.0], 0), lambda: ops.map_segment3d(v, m, labels, regions, [2.0], 2 ** 31),
                 lambda: ops.map_segment3d(v, m, labels, regions, [2.0], 1.5), lambda: ops.map_segment3d(v, m, labels, regions, [2.0], 1, 8),
                 lambda: ops.map_segment3d(v, m, labels, regions, [1.0] * 9, 1), lambda: ops.map_segment3d(v, m[0], labels, regions, [2.0], 1),
                 lambda: ops.map_segment3d(v, m, labels.to(torch.int64), regions, [2.0], 1)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
