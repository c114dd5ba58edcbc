"""GPU: the two ops of csrc/segment.hip on the guard-band arena of tests/guard_util.py: inputs frozen, every buffer the wrappers
allocate poisoned (then zeroed), every pointer inside the arena -- nothing is written outside the outputs, and no result depends
on what a buffer held."""

import numpy as np
import pytest
import torch

import pixel_ref
import region_ref
import segment_ref as ref

pytestmark = pytest.mark.gpu

LO, HI, NBINS = -16.0, 48.0, 4096
THRESHOLDS = [2.0, 3.0, 40.0, float("nan"), -20.0]


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31), (1, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_the_two_ops_stay_inside_their_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    N, H, W = shape
    v, _ = pixel_ref.case_values(N, H * W, LO, HI, NBINS, seed=H)  # (NaN and +-inf among them)
    v = v.reshape(N, H, W)
    m = region_ref.random_masks(N, H, W, 0.45, seed=W)
    m[:, H // 2:] = 0
    labels, regions = ref.label(m, 8)
    tv, tm, tl, tr = (torch.from_numpy(a) for a in (v, m, labels, regions))

    finite = np.nan_to_num(v, nan=0.5, posinf=60.0, neginf=-60.0)  # (a poison that leaked would show as the one NaN of the result)
    for size in (3, 5):
        plain, poison = _bounds(device, dict(v=(torch.from_numpy(finite), True)), lambda t: ops.map_median(t["v"], size))
        assert ref.same_values(plain.res[0].cpu().numpy(), ref.median(finite, size))
        assert [a.numel() for a in poison.allocated] == [N * H * W]  # out
        assert [name for name, _ in poison.called] == ["ddpm_map_median_f32"]

    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    K = len(THRESHOLDS)
    inputs = dict(v=(tv, True), m=(tm, True), l=(tl, True), r=(tr, True), thr=(thr, True))
    for min_size, conn in ((1, 8), (4, 4)):
        truth = (labels, regions) if conn == 8 else ref.label(m, 4)
        inputs["l"], inputs["r"] = (torch.from_numpy(truth[0]), True), (torch.from_numpy(truth[1]), True)
        plain, poison = _bounds(device, inputs, lambda t: ops.map_segment(t["v"], t["m"], t["l"], t["r"], t["thr"], min_size, conn))
        for got, want in zip(plain.res, ref.segment(v, m, *truth, THRESHOLDS, min_size, conn)):
            assert np.array_equal(got.cpu().numpy(), want)
        assert sorted(a.numel() for a in poison.allocated) == sorted([N * K * H * W, N * K * 3, N * K * 3, N * K * 2])
        assert [name for name, _ in poison.called] == ["ddpm_map_segment_f32"]

