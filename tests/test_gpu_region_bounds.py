"""GPU: the three ops of csrc/regions.hip on the guard-band arena of tests/guard_util.py: inputs frozen, every buffer the wrappers
allocate poisoned (then zeroed), every pointer inside the arena -- nothing is written outside the outputs, and no result depends
on what a buffer held."""

import numpy as np
import pytest
import torch

import pixel_ref
import region_ref as ref

pytestmark = pytest.mark.gpu

LO, HI, NBINS = -16.0, 48.0, 4096
THRESHOLDS = [2.0, 3.0, 40.0, float("nan"), -20.0]


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31), (1, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_the_three_ops_stay_inside_their_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    N, H, W = shape
    v, _ = pixel_ref.case_values(N, H * W, LO, HI, NBINS, seed=H)
    v = v.reshape(N, H, W)
    m = ref.random_masks(N, H, W, 0.45, seed=W)
    m[:, H // 2:] = 0  # (regions of every size in one half, none in the other)
    labels, regions = ref.label(m, 8)
    tv, tm, tl, tr = (torch.from_numpy(a) for a in (v, m, labels, regions))

    plain, poison = _bounds(device, dict(m=(tm, True)), lambda t: ops.map_label(t["m"], 8))
    assert np.array_equal(plain.res[0].cpu().numpy(), labels) and np.array_equal(plain.res[1].cpu().numpy(), regions)
    assert sorted(a.numel() for a in poison.allocated) == sorted([N * H * W, N])  # labels, regions
    assert [name for name, _ in poison.called] == ["ddpm_map_label_u8"]

    want_l, want_r = ref.label(v, 4, threshold=20.0)
    plain, poison = _bounds(device, dict(v=(tv, True)), lambda t: ops.map_label(t["v"], 4, threshold=20.0))
    assert np.array_equal(plain.res[0].cpu().numpy(), want_l) and np.array_equal(plain.res[1].cpu().numpy(), want_r)
    assert sorted(a.numel() for a in poison.allocated) == sorted([N * H * W, N])
    assert [name for name, _ in poison.called] == ["ddpm_map_label_f32"]

    R = int(regions.sum())
    want = ref.overlap(v, labels, regions, LO, HI, NBINS)
    inputs = dict(v=(tv, True), l=(tl, True), r=(tr, True))
    plain, poison = _bounds(device, inputs, lambda t: ops.map_region_overlap(t["v"], t["l"], t["r"], LO, HI, NBINS))
    assert (np.abs(plain.res[0].cpu().numpy() - want) <= ref.overlap_bound(want, R)).all()
    assert sorted(a.numel() for a in poison.allocated) == sorted([NBINS + 1, N * (NBINS + 1)])  # total, scratch
    assert [name for name, _ in poison.called] == ["ddpm_map_region_overlap_f32"]
    first = torch.from_numpy(want)
    plain, poison = _bounds(device, dict(total=(first, False), **inputs),
                            lambda t: ops.map_region_overlap(t["v"], t["l"], t["r"], LO, HI, NBINS, total=t["total"]))
    twice = ref.overlap(v, labels, regions, LO, HI, NBINS, total=want)
    assert (np.abs(plain.res[0].cpu().numpy() - twice) <= ref.overlap_bound(twice, 2 * R)).all()
    assert [a.numel() for a in poison.allocated] == [N * (NBINS + 1)]  # scratch alone

    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    plain, poison = _bounds(device, dict(m=(tm, True), thr=(thr, True), **inputs),
                            lambda t: ops.map_component_counts(t["v"], t["m"], t["l"], t["r"], t["thr"], 8))
    assert np.array_equal(plain.res[0].cpu().numpy(), ref.component_counts(v, m, labels, regions, THRESHOLDS, 8))
    assert [a.numel() for a in poison.allocated] == [N * len(THRESHOLDS) * 3]  # counts
    assert [name for name, _ in poison.called] == ["ddpm_map_component_counts_f32"]
