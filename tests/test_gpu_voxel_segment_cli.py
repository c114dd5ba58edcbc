"""-m gpu: ``reconstruct.py --voxel_calibrate_fpr ... --voxel_segment 1`` through the trainer on the toy latent run of
tests/test_gpu_voxel_cli.py (32^3 volumes, 4 validation volumes so that the leave-one-out pass has its n >= 3, batches of 2, the
t-start 10 alone).  Every file of the run without the two flags is there byte for byte; calibration.npz is held against the float64
brute-force leave-one-out of the retained rows smoothed by scipy in 3-D; calibrated_<name>.npz and segments_<name>.npz are held
against tests/voxel_segment_ref.py applied to the Z-maps the run wrote, integer for integer.

The range is [-16, 112) in 4096 bins (step 1 / 32): with three other rows a leave-one-out Z has the tails of a t-distribution with
two degrees of freedom (|Z| up to 181 on this data before the smoothing), and the thresholds of the target rates 0.1 and 0.02 lie
between Z = 1 and 2.5, well inside."""

import json
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import calibration_ref
import pixel_ref
import voxel_ref
import voxel_segment_ref as ref
from test_gpu_voxel_cli import MIX, MODEL, ROOT, SETS, SIZE, Z_FLAGS, _argv

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SIGMA = 1.0
LO, HI, BINS = -16.0, 112.0, 4096
STEP = (HI - LO) / BINS
FPRS = [0.1, 0.02]
THRESHOLDS = (2.0, 3.0, 4.0)
MIN_COMPONENT = 8
RANGE = ("--pixel_range", str(LO), str(HI))
OFF = Z_FLAGS + RANGE + ("--voxel_metrics", "1", "--voxel_regions", "1", "--out_masks", "auto")
NEW = ("--voxel_calibrate_fpr", "0.1,0.02", "--voxel_segment", "1")
ON = OFF + NEW


def _run(root, tag, *extra):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    args.max_t_start = 10  # (the test hook: a prefix of the chained list)
    args.keep_calibration_rows = True
    rec = Reconstruct(args)
    rec.reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept, rec


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from oracle.vqvae import VQVAE as OracleVQVAE
    from parity_util import VQ_README

    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("voxel_segment")
    torch.manual_seed(3)
    vq = OracleVQVAE(**VQ_README).eval()
    (root / "vqvae").mkdir()
    torch.save({"model_state_dict": synthetic.condition_vqvae_state_dict(vq.state_dict())}, root / "vqvae" / "checkpoint.pth")
    json.dump(VQ_README, open(root / "vqvae" / "vqvae_config.json", "w"))
    (root / MODEL).mkdir()
    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               root / MODEL / "checkpoint.pth")
    off, _ = _run(root, "off", *OFF)
    on, rec = _run(root, "on", *ON)
    return root, off, on, rec


def _masks():
    from ddpm_ood_amd import data

    return {"LES": data.synthetic_masks("lesion3d", 4, 1, SIZE, seed=12, mix=MIX).numpy()[:, 0], "in": np.zeros((2, SIZE, SIZE, SIZE), dtype=np.uint8)}


def _with_files_of(root, src, names=("map_stats.npz", "calibration.npz")):
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    (root / MODEL / "ood").mkdir()
    for n in names:
        shutil.copy(src / n, root / MODEL / "ood" / n)


def test_every_other_file_is_byte_identical(runs):
    _, off, on, _ = runs
    names = sorted(p.name for p in off.iterdir())
    new = ["calibration.npz"] + [f"{kind}_{n}.npz" for kind in ("calibrated", "segments") for n in ("in", "LES")]
    assert sorted(p.name for p in on.iterdir()) == sorted(names + new)
    for n in names:
        assert (off / n).read_bytes() == (on / n).read_bytes(), n


def test_calibration_matches_the_float64_leave_one_out_recomputation(runs):
    """From the rows the trainer retained, the voxels flattened to one row of a plane for tests/calibration_ref.py: the float64
    brute force, then scipy's gaussian_filter over (D, H, W).  Tolerance: 4 x the error of the fp32 restatement evaluated with the
    run's own fp32 tables (the bound of tests/test_gpu_pixel_calibration.py) plus the blur's: a pass of 2 r + 1 non-negative taps
    that sum to 1 errs by at most (2 r + 1) u (1 + (2 r + 1) u) max |Z|; that test allows twice that per pass for its two passes,
    here there are three.  The recomputed thresholds lie within one bin step of the file's.  (Measured on an MI355X:
    profiles/voxel_segmentation.md.)"""
    from scipy.ndimage import gaussian_filter

    from ddpm_ood_amd import pixel_metrics as pm

    _, _, on, rec = runs
    rows, got = rec.calibration_rows, rec.calibration_zmaps
    extent = (SIZE, SIZE, SIZE)
    assert rows.shape == (4, 1, 2) + extent and got.shape == (4, 2) + extent and rows.dtype == np.float32 == got.dtype
    stats = rec.last_map_stats[0]
    n, mean, m2 = stats.tables()
    floor32 = stats.floor(0.01).reshape(1, 2)
    assert n == 4
    flat = lambda a: np.asarray(a).reshape(a.shape[:-3] + (1, -1))  # noqa: E731
    want_raw = calibration_ref.loo_brute(flat(rows), floor32).reshape((4, 2) + extent)
    own = np.abs(calibration_ref.loo_fp32(flat(rows), 4, flat(mean.astype(np.float32)), flat(m2.astype(np.float32)), floor32)
                 .astype(np.float64).reshape(want_raw.shape) - want_raw).max()
    radius = int(4 * SIGMA + 0.5)
    tol = 4 * own + 6 * (2 * radius + 1) * U * (1 + (2 * radius + 1) * U) * np.abs(want_raw).max()
    want = np.stack([[gaussian_filter(v, SIGMA, mode="reflect", truncate=4.0) for v in row] for row in want_raw])
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"validation Z-maps of volumes: err {err:.3e} (bound {tol:.3e}: restatement {own:.3e}), max |Z| raw {np.abs(want_raw).max():.2f} "
          f"smoothed {np.abs(want).max():.2f}")
    assert own > 0 and err <= tol and np.abs(want).max() > 1.0
    cal = np.load(on / "calibration.npz")
    assert sorted(cal.files) == sorted(pm.CALIBRATION_KEYS)
    assert cal["t"].tolist() == [10] and int(cal["n"]) == 4 and cal["fpr"].tolist() == FPRS and cal["channels"].tolist() == ["lpips", "mse"]
    assert (float(cal["lo"]), float(cal["hi"]), int(cal["nbins"]), float(cal["sigma"]), float(cal["rel_floor"])) == (LO, HI, BINS, SIGMA, 0.01)
    assert cal["hist"].shape == (2, BINS + 1) and (cal["hist"][:, :-1].sum(axis=1) == 4 * SIZE ** 3).all() and (cal["hist"][:, -1] == 0).all()
    for c in range(2):
        hist = np.bincount(calibration_ref.bin_of(want[:, c], LO, HI, BINS).reshape(-1), minlength=BINS + 1)
        ks, thr = pm.thresholds_from_hist(hist, LO, HI, FPRS)  # (inside the range: else this raises)
        print(f"channel {c}: thresholds {cal['thresholds'][c].tolist()} recomputed {thr.tolist()}")
        assert np.abs(thr - cal["thresholds"][c]).max() <= STEP
        assert np.array_equal(cal["hist"][c], np.bincount(calibration_ref.bin_of(got[:, c], LO, HI, BINS).reshape(-1), minlength=BINS + 1))
        N = cal["hist"][c, :-1].sum()
        for j, f in enumerate(FPRS):
            k = int(cal["bin"][c, j])
            assert cal["hist"][c, k:-1].sum() / N <= f < cal["hist"][c, k - 1:-1].sum() / N and cal["thresholds"][c, j] == np.float32(LO + k * STEP)


def test_the_new_files_equal_the_reference_on_the_written_z_maps(runs):
    _, _, on, _ = runs
    cal = np.load(on / "calibration.npz")
    found = 0
    for name, m in _masks().items():
        n = len(m)
        z, done, sg = np.load(on / f"zmaps_{name}.npz"), np.load(on / f"calibrated_{name}.npz"), np.load(on / f"segments_{name}.npz")
        assert sorted(done.files) == ["components", "counts", "filename", "fpr", "thresholds"]
        assert sorted(sg.files) == sorted(["filename", "t", "channels", "thresholds", "fpr", "median", "min_component", "connectivity", "sigma",
                                           "segmentation", "pixels", "components", "removed", "mask_pixels", "regions"])
        assert np.array_equal(done["thresholds"], cal["thresholds"]) and done["fpr"].tolist() == FPRS
        assert [str(s) for s in done["filename"]] == [str(s) for s in z["filename"]] == [str(s) for s in sg["filename"]]
        assert (int(sg["median"]), int(sg["min_component"]), int(sg["connectivity"]), float(sg["sigma"])) == (3, MIN_COMPONENT, 26, SIGMA)
        assert sg["segmentation"].shape == (n, 2, 5, SIZE, SIZE, SIZE) and sg["segmentation"].dtype == np.uint8
        assert np.array_equal(sg["fpr"], np.asarray([np.nan] * 3 + FPRS), equal_nan=True)
        labels, regions = ref.label(m, 26)
        assert np.array_equal(sg["regions"], regions) and np.array_equal(sg["mask_pixels"], m.reshape(n, -1).astype(bool).sum(axis=1))
        for c, key in enumerate(("z_lpips_map", "z_mse_map")):
            v = z[key]
            thr = cal["thresholds"][c]
            assert np.array_equal(done["counts"][:, c], pixel_ref.counts(v.reshape(n, -1), m.reshape(n, -1), thr)), (name, key)
            assert np.array_equal(done["components"][:, c], voxel_ref.component_counts(v, m, labels, regions, thr, 26)), (name, key)
            every = np.concatenate([np.asarray(THRESHOLDS, dtype=np.float32), thr])
            assert np.array_equal(sg["thresholds"][c], every)
            want = ref.segment(ref.median(v), m, labels, regions, every, MIN_COMPONENT, 26)
            for kind, a in zip(("segmentation", "pixels", "components", "removed"), want):
                assert np.array_equal(sg[kind][:, c], a), (name, key, kind)
            found += int(sg["pixels"][:, c, :, 0].sum())
    assert found > 0  # (something of the lesions is found)


def test_stored_calibration_reproduces_the_files_and_a_foreign_range_is_refused(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, _, on, _ = runs
    try:
        _with_files_of(root, on)
        again, _ = _run(root, "from_file", *ON, "--run_val", "0", "--run_in", "0")
        assert (again / "calibration.npz").read_bytes() == (on / "calibration.npz").read_bytes()  # read, not rewritten
        for n in ("calibrated_LES.npz", "segments_LES.npz", "pixels_LES.npz", "regions_LES.npz", "zmaps_LES.npz"):
            assert (again / n).read_bytes() == (on / n).read_bytes(), n
        for extra, text in ((("--pixel_range", "-8", "112"), "--pixel_range"), (("--voxel_calibrate_fpr", "0.1"), "--voxel_calibrate_fpr")):
            _with_files_of(root, on)
            args = cli.parse_args(_argv(root, *ON, "--run_val", "0", "--run_in", "0", *extra))
            args.max_t_start = 10
            with pytest.raises(ValueError, match=text):
                Reconstruct(args).reconstruct(args)
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_both_budgets_refuse(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, _, on, _ = runs
    try:
        # the retained rows: 4 volumes x 1 t-start x 2 x 32^3 fp32 = 1 MiB on this rank: refused before the validation pass
        args = cli.parse_args(_argv(root, *ON, "--voxel_calibrate_budget_gb", str((2 ** 20 - 1) / 2 ** 30)))
        args.max_t_start = 10
        with pytest.raises(ValueError, match=r"4 x 1 x 2 x 32 x 32 x 32 fp32.*--voxel_calibrate_budget_gb"):
            Reconstruct(args).reconstruct(args)
        # a batch: 2 volumes' maps (0.5 MiB) fit 0.001 GiB, the median's buffer, seg and the forests of --voxel_segment 1 do not
        _with_files_of(root, on)
        args = cli.parse_args(_argv(root, *Z_FLAGS, *RANGE, *NEW, "--run_val", "0", "--run_out", "0", "--anomaly_volume_budget_gb", "0.001"))
        args.max_t_start = 10
        with pytest.raises(ValueError, match=r"--voxel_segment 1.*--anomaly_volume_budget_gb"):
            Reconstruct(args).reconstruct(args)
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_command_line_prints_finite_calibrated_and_segmented_lines(runs):
    root, _, on, _ = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL, "--out_data",
                              "LES", "--score", "pixel", "--pixel_regions", "1", "--pixel_calibrated", "1", "--pixel_segmented", "1"],
                             capture_output=True, text=True, check=True).stdout
        print(got)
        assert got.count("Calibrated for ") == 2 and got.count("Calibrated regions for ") == 2 and got.count("Segmented for ") == 5
        assert "median 3, components below 8 pixels removed (connectivity 26)" in got and "nan" not in got.lower()
        from ddpm_ood_amd import ood

        rows = ood.score_segments(on / "segments_LES.npz", on / "segments_in.npz", "z_mse_map")
        sg = np.load(on / "segments_in.npz")
        for j, r in enumerate(rows):
            assert r["in_fpr"] == float(sg["segmentation"][:, 1, j].mean()) and 0.0 <= r["in_fpr"] < 1.0  # over every voxel of the in set
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_on_one_gpu_reproduce_the_single_rank_files(device, runs):
    """Two ranks (gloo rendezvous, both on cuda:0) on the single-rank run's map_stats.npz and calibration.npz: the Z-maps are its bits,
    so every volume's integers and segmentations are the single rank's, rows rank-major (0 2, 1 3) as in the CSV."""
    from test_gpu_dist import _launch_ranks

    root, _, on, _ = runs
    _with_files_of(root, on)
    try:
        _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *ON, "--run_val", "0", "--run_in", "0", "--inference_skip_factor", "99")],
                      root, timeout=600)
        out = root / MODEL / "ood"
        assert sorted(p.name for p in out.iterdir()) == sorted(["map_stats.npz", "calibration.npz", "maps_LES.npz", "pixels_LES.npz", "regions_LES.npz",
                                                                "results_LES.csv", "zmaps_LES.npz", "calibrated_LES.npz", "segments_LES.npz"])
        order = [0, 2, 1, 3]
        for n in ("calibrated_LES.npz", "segments_LES.npz"):
            one, two = np.load(on / n), np.load(out / n)
            assert sorted(one.files) == sorted(two.files)
            for key in one.files:
                if one[key].ndim and one[key].shape[0] == 4 and key not in ("thresholds", "fpr"):
                    assert np.array_equal(two[key], one[key][order]), (n, key)
                else:
                    assert np.array_equal(one[key], two[key], equal_nan=one[key].dtype.kind == "f"), (n, key)
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
