"""CPU: the host side of ddpm_ood_amd/map_passes.py: the named row layout through the fp32 payload of the gather,
``MapSettings.from_args`` on hand-built Namespaces (what the other host tests do not reach), and the two gathers without a group."""

import argparse
import itertools
import re

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("regions,calibrated,K,F,B", [(r, c, K, F, B) for r, c in itertools.product((False, True), repeat=2)
                                                     for K, F, B in ((1, 1, 1), (3, 2, 3), (3, 1, 1), (1, 2, 3))])
def test_layout_round_trip_through_the_fp32_payload(regions, calibrated, K, F, B):
    from ddpm_ood_amd.map_passes import RowLayout

    layout = RowLayout(K, F if calibrated else 0, regions)
    shapes = {"counts": (2, K, 3), "mask_pixels": ()}
    if regions:
        shapes.update(components=(2, K, 3), regions=())
    if calibrated:
        shapes["calibrated"] = (2 if regions else 1, 2, F, 3)
    assert dict(layout.segments) == shapes and [n for n, _ in layout.segments] == list(shapes)
    width = 2 * K * 3 + 1 + (2 * K * 3 + 1 if regions else 0) + ((2 * F * 3 + (2 * F * 3 if regions else 0)) if calibrated else 0)
    assert layout.width == width
    # distinct integers in every cell; the largest count the fp32 payload carries exactly, and an image without a region
    values = torch.arange(1, B * width + 1, dtype=torch.int32) * 7
    values[0] = (1 << 24) - 1
    parts, at = {}, 0
    for name, shape in shapes.items():
        n = B * int(np.prod(shape, dtype=np.int64))
        parts[name] = values[at:at + n].reshape((B,) + shape).clone()
        at += n
    if regions:
        parts["regions"][B - 1] = 0
    parts["mask_pixels"] = parts["mask_pixels"].to(torch.int64)  # (taken on the host as int64)
    rows = layout.pack(parts)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (B, width)
    for back in (layout.unpack(rows), layout.unpack(np.rint(rows.to(torch.float32).numpy()).astype(np.int64))):
        assert list(back) == list(shapes)
        for name, shape in shapes.items():
            assert tuple(back[name].shape) == (B,) + shape, name
            assert np.array_equal(np.asarray(back[name]), parts[name].numpy()), name
    # the device's share: the same row without the column the host fills in, behind the leading Z-map bits
    device = layout.without("mask_pixels")
    assert device.width == width - 1 and "mask_pixels" not in dict(device.segments)
    lead = torch.full((B, 5), -3, dtype=torch.int32)
    both = device.pack({k: v for k, v in parts.items() if k != "mask_pixels"}, lead=[lead])
    assert torch.equal(both[:, :5], lead)
    assert torch.equal(layout.pack(dict(device.unpack(both[:, 5:]), mask_pixels=parts["mask_pixels"])), rows)
    with pytest.raises(ValueError, match="columns"):
        layout.unpack(rows[:, 1:])


def test_settings_from_a_namespace_without_the_extension_attributes():
    from ddpm_ood_amd.map_passes import MapPipeline, MapSettings

    s = MapSettings.from_args(argparse.Namespace())
    assert (s.anomaly_maps, s.anomaly_z_maps, s.pixel_metrics, s.pixel_regions, s.px_calibrate, s.keep_calibration_rows) == (False,) * 6
    assert s.z_sigma == 0.0 and s.z_std_floor == 0.01  # (test_scope_missing_attributes_and_the_counter)
    assert (s.px_lo, s.px_hi, s.px_bins, s.px_thresholds, s.px_masks, s.px_connectivity, s.cal_fprs, s.cal_budget) == (None,) * 8
    with pytest.raises(Exception):
        s.anomaly_maps = True  # frozen
    p = MapPipeline(s, torch.device("cpu"), "nowhere")  # nothing is built until a flag asks for it
    assert p.layout is None and p.last_map_stats is None and p.last_calibration is None
    mp = p.begin("in", None, [10, 30])
    mp.add_batch(torch.zeros(2, 2, 2), None, None)
    mp.finish_validation()
    assert mp.collect([], torch.zeros(0, dtype=torch.int32), [], {}) == {} and mp.rows_skipped == 0


def test_anomaly_maps_scope_is_refused_from_the_constructor_without_a_device():
    from ddpm_ood_amd.trainer import Reconstruct

    for kw in (dict(spatial_dimension=3, vqvae_checkpoint=None), dict(spatial_dimension=2, vqvae_checkpoint="vqvae.pth")):
        with pytest.raises(ValueError, match=re.escape("--anomaly_maps 1: anomaly maps cover 2-D pixel-space models only")):
            Reconstruct(argparse.Namespace(anomaly_maps=1, **kw))


def test_calibration_without_pixel_metrics_takes_the_bins_of_the_range_flags():
    from ddpm_ood_amd import pixel_metrics as pm
    from ddpm_ood_amd.map_passes import MapSettings

    base = dict(anomaly_z_maps=1, spatial_dimension=2, vqvae_checkpoint=None, pixel_calibrate_fpr="0.05,0.01")
    s = MapSettings.from_args(argparse.Namespace(**base))
    assert s.px_calibrate and not s.pixel_metrics and s.cal_fprs == [0.05, 0.01] and s.cal_budget == int(pm.DEFAULT_BUDGET_GB * (1 << 30))
    assert (s.px_lo, s.px_hi, s.px_bins) == (*pm.DEFAULT_RANGE, pm.DEFAULT_BINS) and s.px_thresholds is None and s.px_masks is None
    s = MapSettings.from_args(argparse.Namespace(**base, pixel_bins=64, pixel_range=[-4.0, 12.0]))
    assert (s.px_lo, s.px_hi, s.px_bins) == (-4.0, 12.0, 64)
    with pytest.raises(ValueError, match="--pixel_bins"):
        MapSettings.from_args(argparse.Namespace(**base, pixel_bins=9000))


def test_gathers_without_a_group_are_the_identity():
    from ddpm_ood_amd.trainer import gather_rows, gather_scores

    ids = torch.arange(4, dtype=torch.int32)
    scores = torch.arange(4 * 3 * 2, dtype=torch.float32).reshape(4, 3, 2)
    for gather in (gather_scores, gather_rows):
        a, b, c = gather(ids, scores)
        assert a is ids and b is scores and c == [4]
