"""-m gpu: ``reconstruct.py --voxel_metrics 1 --voxel_regions 1`` through the trainer on the toy latent model of
tests/test_gpu_volume_maps_cli.py (a conditioned synthetic VQ-VAE, 32^3 volumes -> [128, 2, 2, 2] latents padded to 4^3; the 3-D
engine takes no 1-channel input, so a volume run goes through a VQ-VAE; maps, Z-maps and masks live in the volume's own space
either way): 32^3 volumes (the smallest extent the LPIPS map accepts), 4 / 2 / 4 volumes in batches of 2, the t-start 10 alone, the
out set of kind lesion3d with ``--out_masks auto``.  The CSVs and the map files are those of the run without the voxel flags, byte for byte;
pixels_<name>.npz and regions_<name>.npz are held against tests/voxel_ref.py applied to the Z-maps the run wrote."""

import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pixel_ref
import voxel_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MODEL = "decathlon_voxels"
SIZE, MIX = 32, 40
SETS = {"val": f"synthetic:blobs3d:n=4:size={SIZE}:seed=10", "in": f"synthetic:blobs3d:n=2:size={SIZE}:seed=11",
        "LES": f"synthetic:lesion3d:n=4:size={SIZE}:seed=12:mix={MIX}:name=LES"}
Z_FLAGS = ("--anomaly_volume_maps", "1", "--anomaly_volume_z_maps", "1", "--anomaly_z_sigma", "1.0")
VOXEL = Z_FLAGS + ("--voxel_metrics", "1", "--voxel_regions", "1")
FLAGS = VOXEL + ("--out_masks", "auto")
LO, HI, BINS, THRESHOLDS = -16.0, 48.0, 4096, (2.0, 3.0, 4.0)


def _argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1", "--spatial_dimension", "3", "--vqvae_checkpoint",
            str(root / "vqvae" / "checkpoint.pth"), "--latent_pad", "(1,1,1,1,1,1)", "--b_scale", "0.5", "--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195", "--validation_ids", SETS["val"], "--in_ids", SETS["in"],
            "--out_ids", SETS["LES"], "--batch_size", "2", *extra]


def _run(root, tag, *extra):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    args.max_t_start = 10  # (the test hook: a prefix of the chained list)
    Reconstruct(args).reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from oracle.vqvae import VQVAE as OracleVQVAE
    from parity_util import VQ_README

    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("voxel_metrics")
    torch.manual_seed(3)
    vq = OracleVQVAE(**VQ_README).eval()
    (root / "vqvae").mkdir()
    torch.save({"model_state_dict": synthetic.condition_vqvae_state_dict(vq.state_dict())}, root / "vqvae" / "checkpoint.pth")
    json.dump(VQ_README, open(root / "vqvae" / "vqvae_config.json", "w"))
    (root / MODEL).mkdir()
    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               root / MODEL / "checkpoint.pth")
    return root, _run(root, "z", *Z_FLAGS), _run(root, "vx", *FLAGS)


def _masks():
    from ddpm_ood_amd import data

    m = data.synthetic_masks("lesion3d", 4, 1, SIZE, seed=12, mix=MIX).numpy()
    assert m.any(axis=(1, 2, 3, 4)).all()
    return m[:, 0]


def test_every_other_file_is_byte_identical(runs):
    _, off, on = runs
    names = sorted(p.name for p in off.iterdir())
    assert names == sorted([f"results_{n}.csv" for n in SETS] + [f"maps_{n}.npz" for n in SETS] + ["map_stats.npz", "zmaps_in.npz", "zmaps_LES.npz"])
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["pixels_in.npz", "pixels_LES.npz", "regions_in.npz", "regions_LES.npz"])
    for n in names:
        assert (off / n).read_bytes() == (on / n).read_bytes(), n


def _check(on, name, masks, conn=26):
    z = np.load(on / f"zmaps_{name}.npz")
    px, rg = np.load(on / f"pixels_{name}.npz"), np.load(on / f"regions_{name}.npz")
    head = ["filename", "t", "channels", "lo", "hi", "nbins"]
    assert sorted(px.files) == sorted(head + ["hist", "thresholds", "counts", "mask_pixels", "sigma"])  # the keys of the 2-D files
    assert sorted(rg.files) == sorted(head + ["connectivity", "regions", "overlap", "thresholds", "components", "sigma"])
    n = len(masks)
    assert z["z_mse_map"].shape == (n, SIZE, SIZE, SIZE)
    labels, regions = ref.label(masks, conn)
    for c, key in enumerate(("z_lpips_map", "z_mse_map")):
        v = z[key]
        assert np.array_equal(px["hist"][c], pixel_ref.hist(v, masks, LO, HI, BINS)), key
        assert np.array_equal(px["counts"][:, c], pixel_ref.counts(v, masks, THRESHOLDS)), key
        assert np.array_equal(rg["overlap"][c].view(np.int64), ref.overlap(v, labels, regions, LO, HI, BINS).view(np.int64)), key
        assert np.array_equal(rg["components"][:, c], ref.component_counts(v, masks, labels, regions, THRESHOLDS, conn)), key
    assert px["hist"].dtype == np.int64 and px["counts"].dtype == np.int32 and rg["components"].dtype == np.int32 and rg["overlap"].dtype == np.float64
    assert np.array_equal(px["mask_pixels"], masks.reshape(n, -1).astype(bool).sum(axis=1)) and np.array_equal(rg["regions"], regions)
    assert int(rg["connectivity"]) == conn and float(px["sigma"]) == 1.0 == float(rg["sigma"]) and list(px["t"]) == [10]
    assert (float(px["lo"]), float(px["hi"]), int(px["nbins"])) == (LO, HI, BINS) and [str(s) for s in px["filename"]] == [str(s) for s in z["filename"]]
    assert px["hist"].sum() == 2 * n * SIZE ** 3
    return px, rg


def test_the_files_equal_the_reference_on_the_written_z_maps(runs):
    _, _, on = runs
    masks = _masks()
    px, rg = _check(on, "LES", masks)
    assert rg["regions"].tolist() == [1, 1, 1, 1] and px["hist"][:, 1].sum() == 2 * masks.sum()
    pin, rin = _check(on, "in", np.zeros((2, SIZE, SIZE, SIZE), dtype=np.uint8))  # no masks: the zero mask
    assert pin["hist"][:, 1].sum() == 0 and rin["regions"].tolist() == [0, 0] and not rin["overlap"].any() and (rin["components"][..., 0] == 0).all()
    assert (rin["components"][..., 1] == rin["components"][..., 2]).all()  # every predicted component is off every region


def test_other_connectivity_from_the_statistics_file(runs):
    root, _, on = runs
    (root / MODEL / "ood").mkdir(exist_ok=True)
    shutil.copy(on / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")
    other = _run(root, "vx6", *FLAGS, "--run_val", "0", "--run_in", "0", "--voxel_connectivity", "6")
    assert (other / "zmaps_LES.npz").read_bytes() == (on / "zmaps_LES.npz").read_bytes()  # the statistics from the file: the same bits
    px, rg = _check(other, "LES", _masks(), conn=6)
    a = np.load(on / "pixels_LES.npz")
    for key in a.files:  # the voxel step does not see the connectivity
        assert np.array_equal(a[key], px[key]), key


def test_command_line_prints_finite_voxel_metrics(runs):
    from ddpm_ood_amd import pixel_metrics as pm

    root, _, on = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL, "--out_data",
                              "LES", "--score", "pixel", "--pixel_regions", "1"], capture_output=True, text=True, check=True).stdout
        print(got)
        px, rg = np.load(on / "pixels_LES.npz"), np.load(on / "regions_LES.npz")
        auroc, ap = pm.auroc(px["hist"][1]), pm.average_precision(px["hist"][1])
        aupro = pm.aupro(rg["overlap"][1], int(rg["regions"].sum()), px["hist"][1], 0.3)
        assert all(np.isfinite(x) and 0.0 <= x <= 1.0 for x in (auroc, ap, aupro))
        assert abs(aupro - ref.aupro_direct(np.load(on / "zmaps_LES.npz")["z_mse_map"], _masks(), LO, HI, BINS, 26, 0.3)) <= 1e-12
        assert f"Pixel AUC for {MODEL} vs LES: {auroc * 100:.2f}" in got and f"Pixel AP for {MODEL} vs LES: {ap * 100:.2f}" in got
        assert "Best Dice" in got and "Mean image Dice" in got and f"AUPRO (FPR <= 0.3) for {MODEL} vs LES: {aupro * 100:.2f}" in got
        assert "nan" not in got.lower()
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_a_batch_over_the_budget_is_refused(runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, _, on = runs
    (root / MODEL / "ood").mkdir(exist_ok=True)
    shutil.copy(on / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")
    try:
        # 2 volumes x 1 t-start x 2 x 32^3 fp32 = 0.5 MiB of maps fit 0.001 GiB (1 MiB); the forests of the voxel steps do not
        args = cli.parse_args(_argv(root, *VOXEL, "--run_val", "0", "--run_out", "0", "--anomaly_volume_budget_gb", "0.001"))
        args.max_t_start = 10
        with pytest.raises(ValueError, match="--anomaly_volume_budget_gb"):
            Reconstruct(args).reconstruct(args)
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_on_one_gpu_reproduce_the_single_rank_files(device, runs):
    """Two ranks (gloo rendezvous, both on cuda:0) on the single-rank run's map_stats.npz: the Z-maps are its bits, so the
    all-reduced histogram is its histogram and every volume's integers are its integers, rows rank-major (0 2, 1 3) as in the CSV;
    the all-reduced overlap table adds the same four terms in another order (bound: region_ref.overlap_bound)."""
    import region_ref
    from test_gpu_dist import _launch_ranks

    root, _, on = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    (root / MODEL / "ood").mkdir()
    shutil.copy(on / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")
    try:
        _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *FLAGS, "--run_val", "0", "--run_in", "0", "--inference_skip_factor", "99")],
                      root, timeout=600)
        out = root / MODEL / "ood"
        assert sorted(p.name for p in out.iterdir()) == ["map_stats.npz", "maps_LES.npz", "pixels_LES.npz", "regions_LES.npz",
                                                         "results_LES.csv", "zmaps_LES.npz"]
        order = [0, 2, 1, 3]
        for n in ("pixels_LES.npz", "regions_LES.npz", "zmaps_LES.npz"):
            one, two = np.load(on / n), np.load(out / n)
            assert sorted(one.files) == sorted(two.files)
            for key in one.files:
                if key == "overlap":
                    assert (np.abs(two[key] - one[key]) <= region_ref.overlap_bound(one[key], 4)).all()
                elif one[key].ndim and one[key].shape[0] == 4 and key not in ("thresholds",):
                    assert np.array_equal(two[key], one[key][order]), (n, key)
                else:
                    assert np.array_equal(one[key], two[key]), (n, key)
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
