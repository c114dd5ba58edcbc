"""CPU: the host side of the per-pixel Z-maps -- the float64 restatement of tests/zmap_ref.py against numpy and scipy,
the C ABI of the three kernels and their argument checks (no device is reached), ``MapStats``, the CLI flags and
``ood.score_zmaps`` / ``ood_detection.py --score zmap`` (tests/test_gpu_anomaly_z_maps.py runs the kernels)."""

import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import zmap_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("ddpm_map_stats_update_f32", "ddpm_map_zscore_f32", "ddpm_map_blur_f32")


# ---- 1. the restatement against independent ground truth ---------------------------------------------------------------------------

@pytest.mark.parametrize("splits", [[4, 2], [1, 1, 1, 5], [8]], ids=lambda s: "+".join(map(str, s)))
def test_chunked_chan_update_equals_mean_and_var_of_all_rows(splits):
    rng = np.random.default_rng(sum(splits) * 10 + len(splits))
    v = 1.0 + 1e-3 * rng.standard_normal((sum(splits), 3, 2, 5, 4))
    n, mean, m2 = ref.chan_chunks(v, splits)
    assert n == sum(splits)
    assert np.abs(mean - v.mean(axis=0)).max() <= 1e-12
    assert np.abs(m2 / (n - 1) - v.var(axis=0, ddof=1)).max() <= 1e-12
    assert np.abs(m2 / (n - 1) / v.var(axis=0, ddof=1) - 1).max() <= 1e-9  # (values near 1, deviations 1e-3: relative too)


@pytest.mark.parametrize("L", [1, 2, 5])
def test_refl_is_the_index_pattern_of_symmetric_padding(L):
    want = np.pad(np.arange(L), (3 * L, 3 * L), mode="symmetric")
    got = [ref.refl(i, L) for i in range(-3 * L, 4 * L)]
    assert got == want.tolist()
    assert ref.refl(-3 * L - 1, L) == ref.refl(3 * L, L) and all(0 <= ref.refl(i, L) < L for i in range(-50, 50))


@pytest.mark.parametrize("H,W,sigma", [(5, 5, 2.0), (7, 12, 1.0), (1, 9, 1.5), (33, 31, 4.0)])
def test_restated_blur_equals_scipy_gaussian_filter(H, W, sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((2, H, W))
    taps = ref.gaussian_taps(sigma)
    assert len(taps) == 2 * int(4 * sigma + 0.5) + 1 and abs(taps.sum() - 1) <= 1e-15
    got = ref.blur(x, taps)
    want = np.stack([ndimage.gaussian_filter(m, sigma, mode="reflect", truncate=4.0) for m in x])
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_product_taps_are_the_restated_ones():
    from ddpm_ood_amd import ops

    for sigma in (0.3, 1.0, 1.5, 2.0, 4.0):
        assert np.array_equal(ops.gaussian_taps(sigma), ref.gaussian_taps(sigma)) or \
            np.abs(ops.gaussian_taps(sigma) - ref.gaussian_taps(sigma)).max() <= 1e-16
    assert ops.gaussian_taps(0.0).tolist() == [1.0] == ops.gaussian_taps(0.1).tolist()  # radius 0: the single weight 1


# ---- 2. entry points -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    return _lib.load()


def test_entry_points_are_declared_exported_bound_and_return_int(lib):
    from ddpm_ood_amd import _lib

    header = (ROOT / "include" / "ddpm_ood_hip.h").read_text()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int  # no workspace, no size function
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is C.c_int
        assert args[-1] is C.c_void_p  # the stream; every other void * is a device buffer
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and "map" in n]
    assert lib.ddpm_abi_version() == 10 == _lib.ABI_VERSION  # additive entries: the ABI version stays
    assert "#define DDPM_ABI_VERSION 10" in header


FAKE = 0x10000  # never dereferenced: the argument checks come first
FAR, FAR2 = FAKE + (1 << 20), FAKE + (2 << 20)


def test_map_stats_update_refuses_bad_arguments(lib):
    f = lib.ddpm_map_stats_update_f32
    for v, m, q in ((None, FAR, FAR2), (FAKE, None, FAR2), (FAKE, FAR, None)):
        assert f(v, 2, 8, 0, m, q, None) == -1 and b"null" in lib.ddpm_last_error()
    for B in (0, -1):
        assert f(FAKE, B, 8, 0, FAR, FAR2, None) == -1 and b"B must be positive" in lib.ddpm_last_error()
    for P in (0, -8):
        assert f(FAKE, 2, P, 0, FAR, FAR2, None) == -1 and b"P must be positive" in lib.ddpm_last_error()
    assert f(FAKE, 2, 8, -1, FAR, FAR2, None) == -1 and b"n_prev" in lib.ddpm_last_error()
    # a table on the values ([2, 8] floats = 64 bytes), inside them, the values inside a table, and the two tables on each other
    for m, q in ((FAKE, FAR), (FAKE + 60, FAR), (FAR, FAKE - 28), (FAR, FAR + 16)):
        assert f(FAKE, 2, 8, 0, m, q, None) == -1 and b"aliases" in lib.ddpm_last_error()


def test_map_zscore_refuses_bad_arguments(lib):
    f = lib.ddpm_map_zscore_f32
    ok = [FAKE, FAR, FAR2, FAKE + (3 << 20)]
    for k in range(4):
        ptrs = list(ok)
        ptrs[k] = None
        assert f(*ptrs, 2, 3, 8, 1.0, None) == -1 and b"null" in lib.ddpm_last_error()
    for B in (0, -2):
        assert f(*ok, B, 3, 8, 1.0, None) == -1 and b"B must be positive" in lib.ddpm_last_error()
    for n_t in (0, -1):
        assert f(*ok, 2, n_t, 8, 1.0, None) == -1 and b"n_t must be positive" in lib.ddpm_last_error()
    for P1 in (0, -8):
        assert f(*ok, 2, 3, P1, 1.0, None) == -1 and b"P1 must be positive" in lib.ddpm_last_error()
    # out [2, 8] on / inside the values [2, 3, 8] (192 bytes), on the mean, on inv_std [3, 8] (96 bytes)
    for out in (FAKE, FAKE + 188, FAKE - 60, FAR, FAR + 92, FAR2, FAR2 - 60):
        assert f(FAKE, FAR, FAR2, out, 2, 3, 8, 1.0, None) == -1 and b"aliases" in lib.ddpm_last_error()


def test_map_blur_refuses_bad_arguments(lib):
    f = lib.ddpm_map_blur_f32
    for i, o, t in ((None, FAR, FAR2), (FAKE, None, FAR2), (FAKE, FAR, None)):
        assert f(i, o, t, 2, 1, 8, 8, None) == -1 and b"null" in lib.ddpm_last_error()
    assert f(FAKE, FAR, FAR2, -1, 1, 8, 8, None) == -1 and b"radius must not be negative" in lib.ddpm_last_error()
    assert f(FAKE, FAR, FAR2, 17, 1, 8, 8, None) == -1 and b"above the maximum of 16" in lib.ddpm_last_error()
    for N, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert f(FAKE, FAR, FAR2, 2, N, H, W, None) == -1 and b"must be positive" in lib.ddpm_last_error()
    # in place, out inside in ([1, 8, 8] floats = 256 bytes), in inside out, out on the taps (5 floats)
    for out in (FAKE, FAKE + 252, FAKE - 252, FAR2 + 16, FAR2 - 252):
        assert f(FAKE, out, FAR2, 2, 1, 8, 8, None) == -1 and b"aliases" in lib.ddpm_last_error()


def test_wrappers_refuse_host_tensors_and_bad_shapes_before_any_launch():
    import torch

    from ddpm_ood_amd import ops

    x = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.map_stats_update(x, 0, torch.zeros(3, 8), torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.map_zscore(x, x[0], x[0])
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.map_blur(x, 1.0)
    assert ops.MAP_BLUR_MAX_RADIUS == 16


# ---- 3. MapStats -----------------------------------------------------------------------------------------------------------------------

def _partial(rows):
    return ref.chan_update(rows)


def test_merge_of_two_partials_is_the_table_of_all_rows():
    from ddpm_ood_amd.zmaps import MapStats

    rng = np.random.default_rng(5)
    v = rng.standard_normal((6, 3, 2, 4, 5)) ** 2
    a, b = _partial(v[:3]), _partial(v[3:])
    before = [x.copy() for x in a[1:] + b[1:]]
    n, mean, m2 = MapStats.merge([a, b])
    assert n == 6
    assert np.abs(mean - v.mean(axis=0)).max() <= 1e-12 and np.abs(m2 / 5 - v.var(axis=0, ddof=1)).max() <= 1e-12
    assert all(np.array_equal(x, y) for x, y in zip(before, a[1:] + b[1:]))  # pure: the partials are untouched
    whole = _partial(v)
    assert np.abs(mean - whole[1]).max() <= 1e-12 and np.abs(m2 - whole[2]).max() <= 1e-12
    n0, mean0, m20 = MapStats.merge([(0, None, None), a, (0, None, None)])  # a rank without a row is passed over
    assert n0 == 3 and np.array_equal(mean0, a[1]) and np.array_equal(m20, a[2])
    assert MapStats.merge([]) == (0, None, None)
    with pytest.raises(ValueError):
        MapStats.merge([a, (3, b[1][:, :1], b[2][:, :1])])


def test_finalize_floors_the_std_per_t_and_channel():
    from ddpm_ood_amd.zmaps import MapStats

    n = 5
    std = np.zeros((2, 2, 1, 3))
    std[0, 0, 0] = [0.0, 0.004, 2.0]      # a pixel that never varies, one below the floor 0.02, one above
    std[0, 1, 0] = [10.0, 0.05, 0.2]      # the other channel has its own floor: 0.1
    std[1, 0, 0] = [1.0, 1.0, 1.0]
    std[1, 1, 0] = [0.5, 0.25, 1e-9]
    mean = np.arange(12, dtype=np.float64).reshape(2, 2, 1, 3) / 7
    s = MapStats.from_tables(n, mean, std ** 2 * (n - 1))
    got_mean, inv = s.finalize(0.01)
    assert got_mean.dtype == np.float32 == inv.dtype and inv.shape == (2, 2, 1, 3)
    assert np.array_equal(got_mean, mean.astype(np.float32))
    want = np.array([[[1 / 0.02, 1 / 0.02, 1 / 2.0]], [[1 / 10.0, 1 / 0.1, 1 / 0.2]]])
    assert np.abs(inv[0] / want - 1).max() <= 2e-7  # (float64 arithmetic on the fp32 std, rounded once)
    assert np.abs(inv[1, 1, 0] / np.array([2.0, 4.0, 1 / 0.005]) - 1).max() <= 2e-7
    assert np.array_equal(inv, ref.floor_inv_std(s.std(), 0.01).astype(np.float32))
    assert np.isfinite(inv).all()
    _, inv50 = s.finalize(0.5)
    assert np.abs(inv50[0, 0, 0] / np.array([1.0, 1.0, 0.5]) - 1).max() <= 2e-7


def test_finalize_refuses_too_few_rows_and_a_channel_that_never_varies():
    from ddpm_ood_amd.zmaps import MapStats

    ones = np.ones((1, 2, 2, 2))
    for n in (0, 1):
        with pytest.raises(ValueError, match="at least 2"):
            MapStats.from_tables(n, ones, ones).finalize(0.01)
    m2 = ones.copy()
    m2[0, 1] = 0  # the mse channel of the only t-start: every pixel's std is 0
    with pytest.raises(ValueError, match="varies"):
        MapStats.from_tables(4, ones, m2).finalize(0.01)
    assert MapStats.from_tables(2, ones, ones).finalize(0.01)[1].shape == (1, 2, 2, 2)


def test_save_and_load_round_trip_and_a_foreign_file_is_refused(tmp_path):
    from ddpm_ood_amd.zmaps import MapStats

    rng = np.random.default_rng(8)
    v = rng.random((4, 3, 2, 5, 6)).astype(np.float32)
    n, mean, m2 = _partial(v)
    s = MapStats.from_tables(n, mean, m2)
    path = tmp_path / "map_stats.npz"
    s.save(path, [10, 330, 650], 0.02)
    z = np.load(path)
    assert sorted(z.files) == ["channels", "mean", "n", "rel_floor", "std", "t"]
    assert z["t"].tolist() == [10, 330, 650] and int(z["n"]) == 4 and z["channels"].tolist() == ["lpips", "mse"]
    assert float(z["rel_floor"]) == 0.02
    assert z["mean"].dtype == np.float32 == z["std"].dtype and z["std"].shape == (3, 2, 5, 6)
    assert np.abs(z["std"] - v.astype(np.float64).std(axis=0, ddof=1)).max() <= 1e-7  # the un-floored std
    back = MapStats.load(path, [10, 330, 650], (5, 6))
    assert back.n == 4 and back.t_values == [10, 330, 650]
    for a, b in zip(s.finalize(0.02), back.finalize(0.02)):
        assert np.array_equal(a, b)  # the loaded tables divide by the same bits
    assert np.abs(back.tables()[2] - m2).max() <= 1e-6
    assert MapStats.load(path).n == 4  # nothing to compare with: accepted
    with pytest.raises(ValueError, match="t-starts"):
        MapStats.load(path, [10, 330, 970], (5, 6))
    with pytest.raises(ValueError, match="t-starts"):
        MapStats.load(path, [10, 330], (5, 6))
    with pytest.raises(ValueError, match="maps of"):
        MapStats.load(path, [10, 330, 650], (6, 5))
    with pytest.raises(FileNotFoundError, match="map_stats.npz"):
        MapStats.load(tmp_path / "elsewhere" / "map_stats.npz")


# ---- 4. flags ---------------------------------------------------------------------------------------------------------------------------

def test_cli_flags_default_to_off_and_likelihood_accepts_them():
    import likelihood as lcli
    import reconstruct as cli

    a = cli.parse_args([])
    assert a.anomaly_z_maps == 0 and a.anomaly_z_sigma == 0.0 and a.anomaly_z_std_floor == 0.01
    a = cli.parse_args(["--anomaly_z_maps", "1", "--anomaly_z_sigma", "1.5", "--anomaly_z_std_floor", "0.05"])
    assert a.anomaly_z_maps == 1 and a.anomaly_z_sigma == 1.5 and a.anomaly_z_std_floor == 0.05 and a.anomaly_maps == 0
    b = lcli.parse_args(["--anomaly_z_maps", "1", "--anomaly_z_sigma", "2"])  # inherited with the parser; the bound has no maps
    assert b.anomaly_z_maps == 1 and b.anomaly_z_sigma == 2.0


def test_scope_is_checked_without_a_device_and_names_the_flag():
    from ddpm_ood_amd import zmaps

    zmaps.check_flags(2, None)
    zmaps.check_flags(2, None, 4.0, 0.01)  # radius 16: the largest
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        zmaps.check_flags(3, None)
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        zmaps.check_flags(2, "vqvae.pth")
    with pytest.raises(ValueError, match="--anomaly_z_sigma"):
        zmaps.check_flags(2, None, 4.2)  # radius 17
    with pytest.raises(ValueError, match="--anomaly_z_sigma"):
        zmaps.check_flags(2, None, -1.0)
    with pytest.raises(ValueError, match="--anomaly_z_std_floor"):
        zmaps.check_flags(2, None, 0.0, 0.0)
    # Reconstruct runs this check first thing in its constructor (before any device or checkpoint is touched)
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        Reconstruct(cli.parse_args(["--anomaly_z_maps", "1", "--spatial_dimension", "3"]))
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        Reconstruct(cli.parse_args(["--anomaly_z_maps", "1", "--vqvae_checkpoint", "vqvae.pth"]))


# ---- 5. scoring ------------------------------------------------------------------------------------------------------------------------

def _write_zmaps(path, names, lp, se):
    np.savez(path, filename=np.asarray(names), t=np.asarray([10, 330]), z_lpips_map=lp.astype(np.float32),
             z_mse_map=se.astype(np.float32), sigma=np.float64(0.0), rel_floor=np.float64(0.01))


def test_score_zmaps_and_the_command_line(tmp_path):
    from sklearn.metrics import roc_auc_score

    from ddpm_ood_amd import ood

    rng = np.random.default_rng(3)
    n_in, n_out = 5, 4
    in_se, out_se = rng.standard_normal((n_in, 4, 6)), rng.standard_normal((n_out, 4, 6)) + 0.4
    in_lp, out_lp = rng.standard_normal((n_in, 4, 6)), rng.standard_normal((n_out, 4, 6)) - 0.2
    out_se[1, 2, 3] = 9.0  # one hot pixel: the maximum sees it, the mean hardly
    run = tmp_path / "fashionmnist_z" / "ood"
    run.mkdir(parents=True)
    names_in, names_out = [f"in{i}" for i in range(n_in)], [f"out{i}" for i in range(n_out)]
    # a padded shard repeats an image: the first copy counts, the second (with a wild map) does not
    _write_zmaps(run / "zmaps_in.npz", names_in + ["in0"], np.concatenate([in_lp, in_lp[:1] + 50]), np.concatenate([in_se, in_se[:1] + 50]))
    sets = ood.out_datasets_for("fashionmnist_z")
    for name in sets:
        _write_zmaps(run / f"zmaps_{name}.npz", names_out + ["out2"], np.concatenate([out_lp, out_lp[2:3] - 50]),
                     np.concatenate([out_se, out_se[2:3] - 50]))
    y = [0] * n_in + [1] * n_out
    f32 = lambda a: a.astype(np.float32).astype(np.float64).reshape(len(a), -1)  # noqa: E731
    want = {("z_mse_map", "mean"): roc_auc_score(y, np.concatenate([f32(in_se).mean(1), f32(out_se).mean(1)])),
            ("z_mse_map", "max"): roc_auc_score(y, np.concatenate([f32(in_se).max(1), f32(out_se).max(1)])),
            ("z_lpips_map", "mean"): roc_auc_score(y, np.concatenate([f32(in_lp).mean(1), f32(out_lp).mean(1)])),
            ("z_lpips_map", "max"): roc_auc_score(y, np.concatenate([f32(in_lp).max(1), f32(out_lp).max(1)]))}
    assert len({round(v, 6) for v in want.values()}) >= 3  # (the four choices are told apart)
    for (key, reduce), auc in want.items():
        table, got = ood.score_zmaps(run / "zmaps_in.npz", run / f"zmaps_{sets[0]}.npz", key, reduce)
        assert got == auc and len(table) == n_in + n_out and list(table["type"]) == ["in"] * n_in + ["out"] * n_out
    assert ood.score_zmaps(np.load(run / "zmaps_in.npz"), np.load(run / f"zmaps_{sets[0]}.npz"))[1] == want[("z_mse_map", "mean")]
    with pytest.raises(ValueError):
        ood.score_zmaps(run / "zmaps_in.npz", run / f"zmaps_{sets[0]}.npz", "mse_map")
    with pytest.raises(ValueError):
        ood.score_zmaps(run / "zmaps_in.npz", run / f"zmaps_{sets[0]}.npz", "z_mse_map", "median")

    base = [sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(tmp_path), "--model_name", "fashionmnist_z",
            "--score", "zmap"]
    for extra, auc in (([], want[("z_mse_map", "mean")]),
                       (["--zmap_key", "z_lpips_map", "--zmap_reduce", "max"], want[("z_lpips_map", "max")]),
                       (["--zmap_reduce", "max"], want[("z_mse_map", "max")])):
        got = subprocess.run(base + extra, capture_output=True, text=True, check=True).stdout
        for name in sets:
            assert f"AUC for fashionmnist_z vs {name}: {auc * 100:.1f}" in got
        assert f"Average AUC: {auc * 100:.1f}" in got and f"n_in={n_in} n_out={n_out}" in got
    import ood_detection

    assert ood_detection.parse_args([]).score == "reconstruction"  # the default and the other choices are what they were
    assert ood_detection.parse_args(["--score", "likelihood"]).score == "likelihood"
