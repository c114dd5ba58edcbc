"""GPU: the ops of csrc/regions3d.hip on the guard-band arena of tests/guard_util.py: inputs frozen, every buffer the wrappers
allocate -- outputs and scratch -- poisoned (then zeroed), every pointer inside the arena: nothing is written outside the buffers,
no result depends on what a buffer held, and the scratch is exactly what the size functions answer."""

import numpy as np
import pytest
import torch

import pixel_ref
import voxel_ref as ref

pytestmark = pytest.mark.gpu

LO, HI, NBINS = -16.0, 48.0, 4096
THRESHOLDS = [2.0, 3.0, 40.0, float("nan"), -20.0]


def _words(nbytes):
    return (nbytes + 7) // 8  # the wrappers take the scratch as int64 words


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 2, 3, 130), (1, 17, 33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_the_three_ops_stay_inside_their_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    N, D, H, W = shape
    P = D * H * W
    v, _ = pixel_ref.case_values(N, P, LO, HI, NBINS, seed=H)
    v = v.reshape(N, D, H, W)
    m = ref.random_masks(N, D, H, W, 0.25, seed=W)
    m[:, :, H // 2:] = 0  # (regions of every size in one half, none in the other)
    labels, regions = ref.label(m, 18)
    tv, tm, tl, tr = (torch.from_numpy(a) for a in (v, m, labels, regions))
    label_words = _words(ops.map_label3d_scratch_bytes(N, D, H, W))

    plain, poison = _bounds(device, dict(m=(tm, True)), lambda t: ops.map_label3d(t["m"], 18), size_fns=["ddpm_regions3d_label_scratch_bytes"],
                            size_of=_words)
    assert np.array_equal(plain.res[0].cpu().numpy(), labels) and np.array_equal(plain.res[1].cpu().numpy(), regions)
    assert sorted(a.numel() for a in poison.allocated) == sorted([N * P, N, label_words])  # labels, regions, scratch
    assert [name for name, _ in poison.called] == ["ddpm_regions3d_label_scratch_bytes", "ddpm_map_label3d_u8"]

    want_l, want_r = ref.label(v, 6, threshold=20.0)
    plain, poison = _bounds(device, dict(v=(tv, True)), lambda t: ops.map_label3d(t["v"], 6, threshold=20.0),
                            size_fns=["ddpm_regions3d_label_scratch_bytes"], size_of=_words)
    assert np.array_equal(plain.res[0].cpu().numpy(), want_l) and np.array_equal(plain.res[1].cpu().numpy(), want_r)
    assert [name for name, _ in poison.called] == ["ddpm_regions3d_label_scratch_bytes", "ddpm_map_label3d_f32"]

    want = ref.overlap(v, labels, regions, LO, HI, NBINS)
    inputs = dict(v=(tv, True), l=(tl, True), r=(tr, True))
    for chunk in (None, 3):  # (3: several chunks per volume)
        plain, poison = _bounds(device, inputs, lambda t: ops.map_region_overlap3d(t["v"], t["l"], t["r"], LO, HI, NBINS, chunk_regions=chunk),
                                size_fns=["ddpm_regions3d_overlap_scratch_bytes"], size_of=_words)
        assert np.array_equal(plain.res[0].cpu().numpy().view(np.int64), want.view(np.int64))
        scratch_words = _words(ops.map_region_overlap3d_scratch_bytes(N, NBINS, chunk))
        assert sorted(a.numel() for a in poison.allocated) == sorted([NBINS + 1, scratch_words])  # total, scratch
        assert [name for name, _ in poison.called] == ["ddpm_regions3d_overlap_scratch_bytes", "ddpm_map_region_overlap3d_f32"]
    first = torch.from_numpy(want)
    plain, poison = _bounds(device, dict(total=(first, False), **inputs),
                            lambda t: ops.map_region_overlap3d(t["v"], t["l"], t["r"], LO, HI, NBINS, total=t["total"]))
    twice = ref.overlap(v, labels, regions, LO, HI, NBINS, total=want)
    assert np.array_equal(plain.res[0].cpu().numpy().view(np.int64), twice.view(np.int64))
    assert len(poison.allocated) == 1  # scratch alone

    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    plain, poison = _bounds(device, dict(m=(tm, True), thr=(thr, True), **inputs),
                            lambda t: ops.map_component_counts3d(t["v"], t["m"], t["l"], t["r"], t["thr"], 18),
                            size_fns=["ddpm_regions3d_counts_scratch_bytes"], size_of=_words)
    assert np.array_equal(plain.res[0].cpu().numpy(), ref.component_counts(v, m, labels, regions, THRESHOLDS, 18))
    counts_words = _words(ops.map_component_counts3d_scratch_bytes(N, D, H, W, len(THRESHOLDS)))
    assert sorted(a.numel() for a in poison.allocated) == sorted([N * len(THRESHOLDS) * 3, counts_words])  # counts, scratch
    assert [name for name, _ in poison.called] == ["ddpm_regions3d_counts_scratch_bytes", "ddpm_map_component_counts3d_f32"]


def test_every_refusal_returns_minus_one_without_a_launch(device):
    """With real buffers, between two reads of the outputs: a refused call leaves them as they were."""
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    N, D, H, W = 1, 4, 5, 6
    m = torch.ones((N, D, H, W), dtype=torch.uint8, device=device)
    v = torch.ones((N, D, H, W), dtype=torch.float32, device=device)
    labels = torch.full((N, D, H, W), -3, dtype=torch.int32, device=device)
    regions = torch.full((N,), -3, dtype=torch.int32, device=device)
    scratch = torch.full((1 << 16,), -3, dtype=torch.int64, device=device)
    total = torch.full((65,), -3.0, dtype=torch.float64, device=device)
    counts = torch.full((N, 2, 3), -3, dtype=torch.int32, device=device)
    thr = torch.ones((2,), dtype=torch.float32, device=device)
    s = _lib.stream_ptr()
    p = lambda t: t.data_ptr()  # noqa: E731
    refused = [
        lib.ddpm_map_label3d_u8(p(m), N, D, H, W, 8, p(labels), p(regions), p(scratch), s),
        lib.ddpm_map_label3d_u8(p(m), N, D, H, W, 26, p(labels), p(regions), None, s),
        lib.ddpm_map_label3d_u8(p(m), N, D, H, W, 26, p(labels), p(labels) + 16, p(scratch), s),
        lib.ddpm_map_label3d_f32(p(v), 0.0, N, D, H, W, 26, p(v), p(regions), p(scratch), s),
        lib.ddpm_map_label3d_f32(p(v), 0.0, N, D, H, W, 26, p(labels), p(regions), p(labels), s),
        lib.ddpm_map_label3d_f32(p(v), 0.0, N, 0, H, W, 26, p(labels), p(regions), p(scratch), s),
        lib.ddpm_map_label3d_u8(p(m), N, D, H, W, 26, p(labels) + 2, p(regions), p(scratch), s),
        lib.ddpm_map_region_overlap3d_f32(p(v), p(labels), p(regions), N, D * H * W, LO, 1.0, 64, 4, p(scratch), p(scratch) + 64, 0, s),
        lib.ddpm_map_region_overlap3d_f32(p(v), p(labels), p(regions), N, D * H * W, LO, 1.0, 64, 0, p(scratch), p(total), 0, s),
        lib.ddpm_map_region_overlap3d_f32(p(v), p(labels), p(regions), N, 1 << 31, LO, 1.0, 64, 4, p(scratch), p(total), 0, s),
        lib.ddpm_map_component_counts3d_f32(p(v), p(m), p(labels), p(regions), N, D, H, W, p(thr), 9, 26, p(counts), p(scratch), s),
        lib.ddpm_map_component_counts3d_f32(p(v), p(m), p(labels), p(regions), N, D, H, W, p(thr), 2, 18, p(counts), p(counts), s),
        lib.ddpm_map_component_counts3d_f32(p(v), p(m), p(labels), p(regions), N, D, H, W, p(thr), 2, 7, p(counts), p(scratch), s),
    ]
    assert refused == [-1] * len(refused)
    torch.cuda.synchronize()
    for t, fill in ((labels, -3), (regions, -3), (scratch, -3), (counts, -3)):
        assert bool((t == fill).all())
    assert bool((total == -3.0).all())
    for call in (lambda: ops.map_label3d(m, 8), lambda: ops.map_label3d(v, 4, threshold=0.0), lambda: ops.map_label3d(m, True),
                 lambda: ops.map_component_counts3d(v, m, labels, regions, [2.0], connectivity=8),
                 lambda: ops.map_label3d(m[0], 26), lambda: ops.map_label3d(m.to(torch.int32), 26),
                 lambda: ops.map_region_overlap3d(v, labels, regions, LO, HI, 64, chunk_regions=0),
                 lambda: ops.map_region_overlap3d(v, labels.to(torch.int64), regions, LO, HI, 64),
                 lambda: ops.map_component_counts3d(v, m, labels, regions, [1.0] * 9)):
        with pytest.raises(ValueError):
            call()
