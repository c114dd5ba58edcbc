"""CPU: the host side of the anomaly maps of volumes -- every refusal of the four new flags from the Namespace
alone, the 2-D refusals as they were, the extent-generic map statistics (a 5-D table through save / load), the batch budget, and
that the 2-D settings and the row layout did not move."""

import argparse
import dataclasses
import re

import numpy as np
import pytest
import torch

VOLUME = dict(spatial_dimension=3, vqvae_checkpoint=None)


def _settings(**kw):
    from ddpm_ood_amd.map_passes import MapSettings

    return MapSettings.from_args(argparse.Namespace(**kw))


def test_volume_flags_parse_and_default():
    import reconstruct as cli
    from ddpm_ood_amd.map_passes import MapSettings

    args = cli.parse_args([])
    assert (args.anomaly_volume_maps, args.anomaly_volume_z_maps, args.anomaly_volume_views, args.anomaly_volume_budget_gb) == (0, 0, "last", 8.0)
    off = MapSettings.from_args(args)
    assert not off.volume and not off.want_maps and not off.want_z_maps and off.volume_budget is None and off.volume_views == "last"
    args = cli.parse_args(["--spatial_dimension", "3", "--anomaly_volume_maps", "1", "--anomaly_volume_z_maps", "1", "--anomaly_z_sigma",
                           "1.5", "--anomaly_z_std_floor", "0.05", "--anomaly_volume_views", "all", "--anomaly_volume_budget_gb", "0.5"])
    s = MapSettings.from_args(args)
    assert s.volume_maps and s.volume_z_maps and s.volume and s.want_maps and s.want_z_maps
    assert not s.anomaly_maps and not s.anomaly_z_maps  # the 2-D flags stay what the command line said
    assert (s.z_sigma, s.z_std_floor, s.volume_views, s.volume_budget) == (1.5, 0.05, "all", 1 << 29)
    for vq in (None, "vqvae/checkpoint.pth"):  # with or without a VQ-VAE
        one = _settings(anomaly_volume_z_maps=1, spatial_dimension=3, vqvae_checkpoint=vq)
        assert one.volume_z_maps and not one.volume_maps and one.want_z_maps and not one.want_maps
        assert one.volume_budget == 8 << 30 and one.volume_views == "last"


@pytest.mark.parametrize("flag", ["anomaly_volume_maps", "anomaly_volume_z_maps"])
def test_every_refusal_of_the_volume_flags_comes_from_the_namespace_alone(flag):
    from ddpm_ood_amd.trainer import Reconstruct

    cli_flag = f"--{flag} 1"
    twin = flag.replace("_volume", "")
    cases = [
        (dict(spatial_dimension=2, vqvae_checkpoint=None), "--spatial_dimension 3"),
        (dict(spatial_dimension=2, vqvae_checkpoint=None, **{twin: 1}), "."),  # both: refused either way
        (dict(VOLUME, pixel_metrics=1), "--pixel_metrics"),
        (dict(VOLUME, pixel_regions=1), "--pixel_regions"),
        (dict(VOLUME, pixel_calibrate_fpr="0.05"), "--pixel_calibrate_fpr"),
        (dict(VOLUME, pixel_segment=1), "--pixel_segment"),
        (dict(VOLUME, anomaly_volume_views="first"), "--anomaly_volume_views"),
        (dict(VOLUME, anomaly_volume_budget_gb=0.0), "--anomaly_volume_budget_gb"),
    ]
    if flag == "anomaly_volume_z_maps":
        cases += [(dict(VOLUME, anomaly_z_sigma=4.2), "--anomaly_z_sigma"),  # radius 17 > 16
                  (dict(VOLUME, anomaly_z_sigma=-1.0), "--anomaly_z_sigma"),
                  (dict(VOLUME, anomaly_z_std_floor=0.0), "--anomaly_z_std_floor")]
    for kw, match in cases:
        with pytest.raises(ValueError, match=re.escape(match) if match != "." else match):
            _settings(**{flag: 1}, **kw)
        with pytest.raises(ValueError):  # the constructor runs the check before any device, library or checkpoint
            Reconstruct(argparse.Namespace(**{flag: 1}, **kw))
    with pytest.raises(ValueError, match=re.escape(cli_flag)):
        _settings(**{flag: 1}, spatial_dimension=2, vqvae_checkpoint=None)
    # the 2-D counterpart beside it: the 2-D flag's own message on a volume, the pair's message never reached on an image
    with pytest.raises(ValueError, match="2-D pixel-space models only"):
        _settings(**{flag: 1, twin: 1}, **VOLUME)
    assert _settings(**{flag: 1}, **VOLUME, anomaly_z_sigma=4.1).volume  # radius 16: the largest


def test_the_pair_of_a_volume_flag_and_its_2d_counterpart_is_refused_by_name():
    from ddpm_ood_amd import map_passes

    for flag, twin in (("volume_maps", "anomaly_maps"), ("volume_z_maps", "anomaly_z_maps")):
        args = argparse.Namespace(spatial_dimension=3, vqvae_checkpoint=None, **{f"anomaly_{flag}": 1})
        with pytest.raises(ValueError, match="2-D counterpart"):
            map_passes.check_volume_flags(args, {"anomaly_maps": twin == "anomaly_maps", "anomaly_z_maps": twin == "anomaly_z_maps",
                                                 "z_sigma": 0.0, "z_std_floor": 0.01})


def test_the_2d_refusals_still_raise_with_their_messages():
    from ddpm_ood_amd import zmaps
    from ddpm_ood_amd.perceptual import PerceptualLoss

    for kw in (dict(spatial_dimension=3, vqvae_checkpoint=None), dict(spatial_dimension=2, vqvae_checkpoint="vqvae.pth")):
        with pytest.raises(ValueError, match=re.escape("--anomaly_maps 1: anomaly maps cover 2-D pixel-space models only (no --spatial_dimension 3, "
                                                       "no --vqvae_checkpoint): 2.5-D and latent maps are not built")):
            _settings(anomaly_maps=1, **kw)
        with pytest.raises(ValueError, match=re.escape("--anomaly_z_maps 1: Z-maps cover 2-D pixel-space models only (no --spatial_dimension 3, "
                                                       "no --vqvae_checkpoint): 2.5-D and latent maps are not built")):
            _settings(anomaly_z_maps=1, **kw)
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        zmaps.check_flags(3, None)
    with pytest.raises(NotImplementedError, match="2.5-D maps"):
        PerceptualLoss(3, spatial=True)
    with pytest.raises(NotImplementedError, match="2D inputs only"):
        PerceptualLoss(3).forward_with_map(torch.zeros(1, 1, 32, 32, 32), torch.zeros(1, 1, 32, 32, 32))
    with pytest.raises(NotImplementedError):
        PerceptualLoss(2).forward_with_volume_map(torch.zeros(1, 1, 32, 32, 32), torch.zeros(1, 1, 32, 32, 32))


def test_2d_settings_and_the_row_layout_are_untouched():
    from ddpm_ood_amd.map_passes import MapSettings, RowLayout

    names = [f.name for f in dataclasses.fields(MapSettings)]
    assert names[:21] == ["anomaly_maps", "anomaly_z_maps", "z_sigma", "z_std_floor", "pixel_metrics", "px_lo", "px_hi", "px_bins",
                          "px_thresholds", "px_masks", "pixel_regions", "px_connectivity", "px_calibrate", "cal_fprs", "cal_budget",
                          "keep_calibration_rows", "pixel_segment", "sg_median", "sg_min_component", "sg_thresholds", "sg_connectivity"]
    assert names[21:] == ["volume_maps", "volume_z_maps", "volume_views", "volume_budget"]
    s = _settings(anomaly_maps=1, anomaly_z_maps=1, anomaly_z_sigma=1.5, spatial_dimension=2, vqvae_checkpoint=None)
    assert s == MapSettings(anomaly_maps=True, anomaly_z_maps=True, z_sigma=1.5)  # every volume field at its default
    assert s.want_maps is True and s.want_z_maps is True and s.volume is False
    assert MapSettings().want_maps is False and MapSettings().want_z_maps is False
    layout = RowLayout(3, 2, True)
    assert [n for n, _ in layout.segments] == ["counts", "mask_pixels", "components", "regions", "calibrated"] and layout.width == 2 * (18 + 1) + 24
    assert RowLayout(2).width == 13 and RowLayout(2).without("mask_pixels").width == 12


def test_map_statistics_take_an_extent(tmp_path):
    from ddpm_ood_amd import zmaps
    from ddpm_ood_amd.zmaps import MapStats

    rng = np.random.default_rng(3)
    rows = rng.random((5, 2, 2, 3, 4, 6))  # [rows, n_t, 2, D, H, W]
    n, mean, m2 = MapStats.merge([(3, rows[:3].mean(0), ((rows[:3] - rows[:3].mean(0)) ** 2).sum(0)),
                                  (2, rows[3:].mean(0), ((rows[3:] - rows[3:].mean(0)) ** 2).sum(0))])
    assert n == 5 and np.allclose(mean, rows.mean(0), atol=1e-14) and np.allclose(m2 / 4, rows.var(0, ddof=1), atol=1e-14)
    stats = MapStats.from_tables(n, mean, m2)
    std = stats.std()
    assert std.shape == (2, 2, 3, 4, 6) and std.dtype == np.float32
    floor = zmaps.std_floor(std, 0.25)
    assert floor.shape == (2, 2, 1, 1, 1)
    assert np.array_equal(floor[:, :, 0, 0, 0], 0.25 * std.astype(np.float64).reshape(2, 2, -1).max(axis=2))  # over every voxel of a (t, c)
    assert np.array_equal(stats.floor(0.25), floor[:, :, 0, 0, 0].astype(np.float32))
    m32, inv = stats.finalize(0.25)
    assert m32.shape == inv.shape == std.shape and inv.dtype == np.float32
    assert np.array_equal(inv, (1.0 / np.maximum(std.astype(np.float64), floor)).astype(np.float32))
    path = tmp_path / "map_stats.npz"
    stats.save(path, [10, 970], 0.25)
    z = np.load(path)
    assert z["mean"].shape == z["std"].shape == (2, 2, 3, 4, 6) and z["t"].tolist() == [10, 970] and int(z["n"]) == 5
    back = MapStats.load(path, [10, 970], (3, 4, 6))
    for a, b in zip(back.finalize(0.25), (m32, inv)):
        assert np.array_equal(a, b)  # a run that reads the file divides by the writer's bits
    with pytest.raises(ValueError, match="maps of"):
        MapStats.load(path, [10, 970], (4, 6))  # a 2-D run on a volume's file
    with pytest.raises(ValueError, match="maps of"):
        MapStats.load(path, [10, 970], (3, 6, 4))
    with pytest.raises(ValueError, match="t-starts"):
        MapStats.load(path, [10], (3, 4, 6))
    with pytest.raises(ValueError, match="std table"):
        zmaps.std_floor(std[None], 0.25)
    flat = np.ones((1, 2, 2, 2, 2))
    with pytest.raises(ValueError, match="varies"):
        m0 = flat.copy()
        m0[0, 1] = 0
        MapStats.from_tables(4, flat, m0).finalize(0.01)


def test_the_batch_budget_names_batch_size():
    from ddpm_ood_amd.map_passes import check_volume_budget

    per_volume = 25 * 2 * 128 ** 3 * 4  # 128^3, 25 t-starts: 420 MB of per-t maps per volume
    assert check_volume_budget(1, 25, (128, 128, 128), True, 8 << 30) == per_volume == 419430400
    assert check_volume_budget(20, 25, (128, 128, 128), True, 8 << 30) == 20 * per_volume  # 7.8 GiB
    with pytest.raises(ValueError, match=re.escape("--batch_size")) as e:
        check_volume_budget(21, 25, (128, 128, 128), True, 8 << 30)
    assert "--anomaly_volume_budget_gb" in str(e.value) and "21 x 25 x 2 x 128 x 128 x 128" in str(e.value)
    assert check_volume_budget(21, 25, (128, 128, 128), False, 8 << 30) == 21 * 2 * 128 ** 3 * 4  # the accumulated maps alone
