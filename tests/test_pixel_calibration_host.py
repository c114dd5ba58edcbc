"""CPU: thresholds calibrated on leave-one-out validation Z-maps -- the closed form against the brute force, the
quantile rule on hand-made histograms, the flags and their refusals, the budget, ``calibration.npz`` and its mismatch errors, the
entry point's host-side refusals, and the lines ``ood_detection.py --score pixel --pixel_calibrated 1`` prints."""

import argparse
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import calibration_ref as ref

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. the closed form ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 8, 33])
def test_closed_form_equals_deleting_the_row(n):
    """Row i deleted, mean and ddof-1 std of the others recomputed, the floor applied, the mean over t: the closed form from
    (n, mean, M2) agrees to 1e-9 (gamma-distributed values with one outlier column; |Z| up to about 50)."""
    v = ref.case_values(n)
    assert v.shape == (n, 3, 2, 7, 9)
    floor = ref.floor_table(v)
    want = ref.loo_brute(v, floor)
    got = ref.loo_closed(v, *ref.stats(v), floor)
    err = np.abs(got - want).max()
    print(f"n={n}: closed form vs brute force {err:.2e}, max |Z| {np.abs(want).max():.1f}")
    assert got.shape == want.shape == (n, 2, 7, 9) and err <= 1e-9
    assert np.abs(want).max() > 1.0
    if n >= 8:
        assert want[1, :, 0, 0].min() > 10.0  # the outlier column stands out against the others' statistics


def test_floor_is_the_one_finalize_tables_divides_by():
    """``MapStats.floor`` is fp32 of rel_floor x the largest fp32 std of the (t, c): the number behind ``finalize``'s inv_std
    wherever the floor holds."""
    from ddpm_ood_amd import zmaps

    v = ref.case_values(8, H=8, W=8)
    v[:, :, :, 3, 3] = 0.5  # a pixel that never varies: floored
    n, mean, m2 = ref.stats(v)
    stats = zmaps.MapStats.from_tables(n, mean, m2, [10, 20, 30])
    floor = stats.floor(0.01)
    assert floor.shape == (3, 2) and floor.dtype == np.float32
    std32 = stats.std()
    assert np.array_equal(floor, (0.01 * std32.astype(np.float64).max(axis=(2, 3))).astype(np.float32))
    _, inv = stats.finalize(0.01)
    assert np.array_equal(inv[:, :, 3, 3], (1.0 / (0.01 * std32.astype(np.float64).max(axis=(2, 3)))).astype(np.float32))
    assert np.abs(floor - ref.floor_table(v)).max() <= 1e-6 * floor.max()
    with pytest.raises(ValueError, match="varies"):
        zmaps.MapStats.from_tables(4, np.zeros((1, 2, 2, 2)), np.zeros((1, 2, 2, 2))).floor(0.01)


# ---- 2. the quantile rule ------------------------------------------------------------------------------------------------------------------

def test_thresholds_from_hist_on_hand_made_histograms():
    from ddpm_ood_amd import pixel_metrics as pm

    # 100 pixels over 10 bins of [0, 10): c_k = 100 90 80 ... 10, 0
    flat = np.asarray([10] * 10 + [7])  # (7 NaN pixels: left out of N)
    # exact ties: c_5 / N = 0.5 <= 0.5 -> k* = 5; c_9 / N = 0.1 <= 0.1 -> 9; 0.45 falls between c_5 and c_6 -> 6
    ks, thr = pm.thresholds_from_hist(flat, 0.0, 10.0, [0.5, 0.1, 0.45])
    assert ks.tolist() == [5, 9, 6] and thr.tolist() == [5.0, 9.0, 6.0] and ks.dtype == np.int64 and thr.dtype == np.float64
    assert ks.tolist() == ref.quantile_bins(flat, [0.5, 0.1, 0.45])
    assert pm.reached_fpr(flat, ks).tolist() == [0.5, 0.1, 0.4]
    # a target below the last bin's share: no bin edge reaches it
    with pytest.raises(ValueError, match="--pixel_range"):
        pm.thresholds_from_hist(flat, 0.0, 10.0, [0.5, 0.05])
    # everything in one bin: the edge above it, for any target
    one = np.zeros(9, dtype=np.int64)
    one[3] = 1000
    ks, thr = pm.thresholds_from_hist(one, -4.0, 12.0, [0.9, 0.001])
    assert ks.tolist() == [4, 4] and thr.tolist() == [4.0, 4.0]
    one[:] = 0
    one[7] = 5  # ... unless it is the last bin
    with pytest.raises(ValueError, match="--pixel_range"):
        pm.thresholds_from_hist(one, -4.0, 12.0, [0.9])
    # mass below the range sits in bin 0 and counts in N
    low = np.asarray([90, 0, 0, 5, 5, 0])
    ks, thr = pm.thresholds_from_hist(low, 1.0, 6.0, [0.1, 0.05, 0.5])
    assert ks.tolist() == [1, 4, 1] and thr.tolist() == [2.0, 5.0, 2.0]
    assert ks.tolist() == ref.quantile_bins(low, [0.1, 0.05, 0.5])
    with pytest.raises(ValueError, match="--pixel_range"):
        pm.thresholds_from_hist(low, 1.0, 6.0, [0.04])
    # random histograms against the one-k-at-a-time definition, both sides of every threshold
    rng = np.random.default_rng(0)
    for _ in range(20):
        h = rng.integers(0, 1000, 65)
        h[-2] = 0
        f = rng.uniform(0.001, 0.9, 8)
        ks, thr = pm.thresholds_from_hist(h, -4.0, 12.0, f)
        assert ks.tolist() == ref.quantile_bins(h, f)
        N = h[:-1].sum()
        for k, t in zip(ks, f):
            assert h[k:-1].sum() / N <= t < h[k - 1:-1].sum() / N
        assert np.array_equal(thr, -4.0 + ks * 0.25)


def test_thresholds_from_hist_refusals():
    from ddpm_ood_amd import pixel_metrics as pm

    h = np.asarray([10] * 10 + [0])
    with pytest.raises(ValueError, match="no scored pixel"):
        pm.thresholds_from_hist(np.asarray([0, 0, 0, 12]), 0.0, 3.0, [0.1])  # only NaN pixels
    for bad in ([0.0], [1.0], [-0.1], [0.5, 1.5], [float("nan")]):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            pm.thresholds_from_hist(h, 0.0, 10.0, bad)
    with pytest.raises(ValueError, match="1 .. 8"):
        pm.thresholds_from_hist(h, 0.0, 10.0, [])
    with pytest.raises(ValueError, match="1 .. 8"):
        pm.thresholds_from_hist(h, 0.0, 10.0, [0.5] * 9)
    assert len(pm.thresholds_from_hist(h, 0.0, 10.0, [0.5] * 8)[0]) == 8
    with pytest.raises(ValueError, match="nbins"):
        pm.thresholds_from_hist(np.zeros((2, 11)), 0.0, 10.0, [0.5])
    with pytest.raises(ValueError, match="negative"):
        pm.thresholds_from_hist(np.asarray([5, -1, 0]), 0.0, 2.0, [0.5])


# ---- 3. flags, budget -----------------------------------------------------------------------------------------------------------------------

def test_flags_parse_with_their_defaults():
    import ood_detection as det
    import reconstruct as cli

    a = cli.parse_args([])
    assert a.pixel_calibrate_fpr is None and a.pixel_calibrate_budget_gb == 8.0
    a = cli.parse_args(["--pixel_calibrate_fpr", "0.05,0.01,0.001", "--pixel_calibrate_budget_gb", "0.5"])
    assert a.pixel_calibrate_fpr == "0.05,0.01,0.001" and a.pixel_calibrate_budget_gb == 0.5
    assert det.parse_args([]).pixel_calibrated == 0 and det.parse_args(["--pixel_calibrated", "1"]).pixel_calibrated == 1


def test_reconstruct_refuses_at_construction_before_anything_is_loaded():
    from ddpm_ood_amd import pixel_metrics as pm
    from ddpm_ood_amd.trainer import Reconstruct

    def ns(**kw):
        base = dict(anomaly_z_maps=1, anomaly_maps=0, spatial_dimension=2, vqvae_checkpoint=None, run_out=0, out_ids=None,
                    pixel_calibrate_fpr="0.05,0.01")
        base.update(kw)
        return argparse.Namespace(**base)

    with pytest.raises(ValueError, match=r"--pixel_calibrate_fpr.*--anomaly_z_maps 1"):
        Reconstruct(ns(anomaly_z_maps=0))
    for kw, text in ((dict(pixel_calibrate_fpr="0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9"), "1 .. 8"), (dict(pixel_calibrate_fpr="0.5,1.0"), "(0, 1)"),
                     (dict(pixel_calibrate_fpr="0"), "(0, 1)"), (dict(pixel_calibrate_fpr="-0.01"), "(0, 1)"),
                     (dict(pixel_calibrate_fpr="five"), "--pixel_calibrate_fpr"), (dict(pixel_calibrate_budget_gb=0), "--pixel_calibrate_budget_gb"),
                     (dict(pixel_calibrate_budget_gb="much"), "--pixel_calibrate_budget_gb"), (dict(pixel_bins=9000), "--pixel_bins"),
                     (dict(pixel_range=[3.0, 3.0]), "--pixel_range")):
        with pytest.raises(ValueError, match=re.escape(text)):
            Reconstruct(ns(**kw))
    assert pm.check_calibration_flags(1, "0.05, 0.01") == ([0.05, 0.01], 8 << 30)
    assert pm.check_calibration_flags(1, [0.5], 0.25) == ([0.5], 1 << 28)


def test_budget_refusal_states_the_size_and_names_the_flag():
    from ddpm_ood_amd import pixel_metrics as pm

    assert pm.check_budget(1024, 25, 32, 32, 8 << 30) == 1024 * 25 * 2 * 32 * 32 * 4
    assert pm.check_budget(8, 2, 32, 32, 8 * 2 * 2 * 32 * 32 * 4) == 131072  # exactly the budget: fine
    with pytest.raises(ValueError, match=r"10000 x 100 x 2 x 64 x 64 fp32 = 30\.518 GiB.*--pixel_calibrate_budget_gb"):
        pm.check_budget(10000, 100, 64, 64, 8 << 30)
    with pytest.raises(ValueError, match="--pixel_calibrate_budget_gb"):
        pm.check_budget(8, 2, 32, 32, 131071)


# ---- 4. calibration.npz --------------------------------------------------------------------------------------------------------------------

def _calibration(seed=0, nbins=64, lo=-4.0, hi=12.0, fprs=(0.05, 0.01)):
    from ddpm_ood_amd import pixel_metrics as pm

    rng = np.random.default_rng(seed)
    z = rng.normal(0, 1, (2, 20000)) * np.asarray([[1.0], [1.5]])
    hist = np.stack([np.bincount(ref.bin_of(zc, lo, hi, nbins), minlength=nbins + 1) for zc in z])
    return pm.calibration_tables(hist, [10, 30], 8, list(fprs), lo, hi, nbins, 1.0, 0.01), hist


def test_calibration_file_round_trip_and_every_mismatch(tmp_path):
    from ddpm_ood_amd import pixel_metrics as pm

    cal, hist = _calibration()
    assert sorted(cal) == sorted(pm.CALIBRATION_KEYS)
    assert cal["bin"].shape == (2, 2) and cal["bin"].dtype == np.int64 and cal["thresholds"].dtype == np.float32
    assert cal["hist"].dtype == np.int64 and cal["hist"].shape == (2, 65) and cal["fpr"].tolist() == [0.05, 0.01]
    for c in range(2):
        assert cal["bin"][c].tolist() == ref.quantile_bins(hist[c], [0.05, 0.01])
        assert np.array_equal(cal["thresholds"][c], (-4.0 + cal["bin"][c] * 0.25).astype(np.float32))
    assert (cal["thresholds"][1] > cal["thresholds"][0]).all()  # the wider channel needs the higher thresholds
    path = tmp_path / pm.CALIBRATION_FILE
    np.savez(path, **cal)
    same = dict(t_values=[10, 30], lo=-4.0, hi=12.0, nbins=64, sigma=1.0, rel_floor=0.01, fprs=[0.05, 0.01])
    back = pm.load_calibration(path, **same)
    assert sorted(back) == sorted(pm.CALIBRATION_KEYS)
    for k in pm.CALIBRATION_KEYS:
        assert np.array_equal(back[k], cal[k]) and back[k].dtype == np.asarray(cal[k]).dtype, k
    assert np.array_equal(pm.load_calibration(path)["bin"], cal["bin"])  # nothing given: nothing compared
    for kw, text in ((dict(t_values=[10, 50]), "t-starts"), (dict(t_values=[10]), "t-starts"), (dict(lo=-8.0), "--pixel_range"),
                     (dict(hi=16.0), "--pixel_range"), (dict(nbins=128), "--pixel_bins"), (dict(sigma=0.0), "--anomaly_z_sigma"),
                     (dict(rel_floor=0.02), "--anomaly_z_std_floor"), (dict(fprs=[0.05]), "--pixel_calibrate_fpr")):
        with pytest.raises(ValueError, match=re.escape(text)):
            pm.load_calibration(path, **{**same, **kw})
    with pytest.raises(FileNotFoundError, match="--pixel_calibrate_fpr"):
        pm.load_calibration(tmp_path / "nowhere" / pm.CALIBRATION_FILE)
    np.savez(tmp_path / "short.npz", **{k: v for k, v in cal.items() if k != "hist"})
    with pytest.raises(ValueError, match="hist"):
        pm.load_calibration(tmp_path / "short.npz")
    with pytest.raises(ValueError, match=r"\[2, nbins \+ 1\]"):
        pm.calibration_tables(hist[0], [10], 8, [0.05], -4.0, 12.0, 64, 0.0, 0.01)


# ---- 5. the C ABI and the wrapper ----------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_exported_bound_and_refuses_on_the_host():
    from ddpm_ood_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ddpm_ood_hip.h").read_text(), flags=re.S)
    assert "#define DDPM_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    lib = _lib.load()
    name = "ddpm_map_zscore_loo_f32"
    argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_float, C.c_void_p]
    assert re.search(rf"\bint\s+{name}\s*\(", header)
    assert _lib.SIGNATURES[name] == (C.c_int, argtypes)
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and fn.argtypes == argtypes
    v, mean, m2, fl, out = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28  # (never touched: every refusal comes before the launch)
    assert fn(None, mean, m2, fl, out, 2, 3, 64, 8, 1.0, None) == -1 and b"map_zscore_loo" in lib.ddpm_last_error()
    for n in (2, 1, 0, -5):
        assert fn(v, mean, m2, fl, out, 2, 3, 64, n, 1.0, None) == -1 and b"n >= 3" in lib.ddpm_last_error()
    assert fn(v, mean, m2, fl, out, 0, 3, 64, 8, 1.0, None) == -1 and b"B must" in lib.ddpm_last_error()
    assert fn(v, mean, m2, fl, out, 2, 0, 64, 8, 1.0, None) == -1 and b"n_t must" in lib.ddpm_last_error()
    assert fn(v, mean, m2, fl, out, 2, 3, 0, 8, 1.0, None) == -1 and b"plane must" in lib.ddpm_last_error()
    # out inside values, the mean, m2 and the floor table: B = 2, n_t = 3, plane = 64 -> values 3072, tables 1536, floor 24, out 1024 bytes
    for alias in (v + 3068, v - 1020, mean + 1532, m2, fl + 20, fl - 1020):
        assert fn(v, mean, m2, fl, alias, 2, 3, 64, 8, 1.0, None) == -1 and b"alias" in lib.ddpm_last_error(), alias


def test_wrapper_validates_before_the_library_is_asked():
    from ddpm_ood_amd import ops

    v, tab, fl = torch.zeros(2, 3, 2, 8), torch.zeros(3, 2, 8), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.map_zscore_loo(v, tab, tab, 8, fl)  # (no CPU fallback)


# ---- 6. the report -------------------------------------------------------------------------------------------------------------------------------

def _run_files(ood_dir, regions=True):
    """Hand-written files of one run: 4 in images, 4 out images with masks, 256 pixels each, 64 bins of [-4, 12)."""
    from ddpm_ood_amd import pixel_metrics as pm

    ood_dir.mkdir(parents=True)
    cal, _ = _calibration(fprs=(0.05, 0.01))
    np.savez(ood_dir / pm.CALIBRATION_FILE, **cal)
    rng = np.random.default_rng(7)
    sets = {}
    for name, masked in (("in", False), ("LES", True)):
        m = (rng.random((4, 256)) < 0.2).astype(np.uint8) if masked else np.zeros((4, 256), dtype=np.uint8)
        z = [(rng.normal(0, 1.0 + 0.5 * c, (4, 256)) + 5.0 * m).astype(np.float32) for c in range(2)]
        hist = np.zeros((2, 2, 65), dtype=np.int64)
        for c in range(2):
            for cls in range(2):
                hist[c, cls] = np.bincount(ref.bin_of(z[c][m == cls], -4.0, 12.0, 64), minlength=65)
        np.savez(ood_dir / f"pixels_{name}.npz", filename=np.asarray([f"{name}{i}" for i in range(4)]), t=np.asarray([10, 30]),
                 channels=np.asarray(["lpips", "mse"]), lo=np.float64(-4.0), hi=np.float64(12.0), nbins=np.int64(64), hist=hist,
                 thresholds=np.asarray([2.0], dtype=np.float32), counts=np.zeros((4, 2, 1, 3), dtype=np.int32), mask_pixels=m.sum(axis=1),
                 sigma=np.float64(1.0))
        counts = np.zeros((4, 2, 2, 3), dtype=np.int32)
        for c in range(2):
            for j, t in enumerate(cal["thresholds"][c]):
                pred = z[c] > t
                counts[:, c, j] = np.stack([(pred & (m == 1)).sum(axis=1), (pred & (m == 0)).sum(axis=1), (~pred & (m == 1)).sum(axis=1)], axis=1)
        extra = {}
        if regions:  # 3 regions per image: (hit, pred, false_pred) made up, the same for every image
            extra["components"] = np.tile(np.asarray([[[2, 4, 1], [1, 2, 0]], [[3, 3, 0], [2, 5, 3]]], dtype=np.int32), (4, 1, 1, 1))
            np.savez(ood_dir / f"regions_{name}.npz", regions=np.full(4, 3, dtype=np.int32))
        np.savez(ood_dir / f"calibrated_{name}.npz", filename=np.asarray([f"{name}{i}" for i in range(4)]), fpr=cal["fpr"],
                 thresholds=cal["thresholds"], counts=counts, **extra)
        sets[name] = (z, m, hist, counts)
    return cal, sets


def test_calibrated_report_lines_from_hand_written_files(tmp_path, capsys):
    from ddpm_ood_amd import ood
    from ddpm_ood_amd import pixel_metrics as pm

    ood_dir = tmp_path / "model" / "ood"
    cal, sets = _run_files(ood_dir)
    z_in, _, _, _ = sets["in"]
    z, m, hist, counts = sets["LES"]
    for c, key in enumerate(("z_lpips_map", "z_mse_map")):
        rows = ood.score_pixels_calibrated(ood_dir, "LES", key, regions=True)
        assert [r["fpr"] for r in rows] == [0.05, 0.01]
        for j, r in enumerate(rows):
            k, t = int(cal["bin"][c, j]), float(cal["thresholds"][c, j])
            assert r["threshold"] == t
            assert r["val_fpr"] == cal["hist"][c, k:-1].sum() / cal["hist"][c, :-1].sum() <= r["fpr"]
            # the two rates and the pooled Dice are exact sums over the histograms from the threshold's bin on
            b_in, b_out = ref.bin_of(z_in[c], -4.0, 12.0, 64), ref.bin_of(z[c], -4.0, 12.0, 64)
            assert r["in_fpr"] == (b_in >= k).sum() / b_in.size
            tp, fp, fn = ((b_out >= k) & (m == 1)).sum(), ((b_out >= k) & (m == 0)).sum(), ((b_out < k) & (m == 1)).sum()
            assert r["pooled_dice"] == 2.0 * tp / (2.0 * tp + fp + fn)
            assert abs(r["mean_dice"] - pm.dice_from_counts(counts[:, c, j]).mean()) <= 1e-15
        # the made-up component counts: recall = hit / 3, precision = 1 - false / pred
        hit, pred, false = ([[2, 1], [3, 2]][c], [[4, 2], [3, 5]][c], [[1, 0], [0, 3]][c])
        for j, r in enumerate(rows):
            assert abs(r["region_recall"] - hit[j] / 3) <= 1e-15 and abs(r["component_precision"] - (1 - false[j] / pred[j])) <= 1e-15
        assert "region_recall" not in ood.score_pixels_calibrated(ood_dir, "LES", key)[0]
    args = argparse.Namespace(output_dir=str(tmp_path), model_name="model", zmap_key="z_mse_map", pixel_include_in=0, pixel_calibrated=1)
    got = ood.main_pixels(args, out_data=["LES"])
    out = capsys.readouterr().out
    rows = ood.score_pixels_calibrated(ood_dir, "LES", "z_mse_map")
    assert got["LES"]["calibrated"] == rows
    for r in rows:
        assert (f"Calibrated for model vs LES at validation FPR <= {r['fpr']:g}: Z > {r['threshold']:.4f} (validation FPR "
                f"{r['val_fpr']:.5f}, in-set FPR {r['in_fpr']:.5f}), pooled Dice {r['pooled_dice']:.4f}, mean image Dice "
                f"{r['mean_dice']:.4f}") in out
    assert "Calibrated regions" not in out
    # without the flag: the lines of before and nothing else
    args.pixel_calibrated = 0
    assert "calibrated" not in ood.main_pixels(args, out_data=["LES"])["LES"] and "Calibrated" not in capsys.readouterr().out


def test_calibrated_report_names_the_flag_behind_a_missing_file(tmp_path):
    from ddpm_ood_amd import ood

    ood_dir = tmp_path / "model" / "ood"
    _run_files(ood_dir, regions=False)
    with pytest.raises(FileNotFoundError, match="--pixel_regions 1"):
        ood.score_pixels_calibrated(ood_dir, "LES", regions=True)
    for name, flag in (("calibrated_LES.npz", "--pixel_calibrate_fpr"), ("pixels_in.npz", "--pixel_metrics 1"),
                       ("pixels_LES.npz", "--pixel_metrics 1"), ("calibration.npz", "--pixel_calibrate_fpr")):
        (ood_dir / name).unlink()
        with pytest.raises(FileNotFoundError, match=re.escape(flag)):
            ood.score_pixels_calibrated(ood_dir, "LES")
    with pytest.raises(ValueError, match="key"):
        ood.score_pixels_calibrated(ood_dir, "LES", key="mse_map")
