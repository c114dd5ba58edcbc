"""-m gpu: ``reconstruct.py --anomaly_volume_maps 1 --anomaly_volume_z_maps 1`` through the trainer on a toy latent model (a
conditioned synthetic VQ-VAE, 32^3 volumes -> [128, 2, 2, 2] latents padded to 4^3; the set-up of
tests/test_gpu_likelihood.py::test_latent_likelihood_through_a_vqvae_with_latent_pad): 3 sets x 4 volumes, t = 10 and 650.

What is held against what (u = 2^-24; ``_close``: err <= tol (1 + max |ref|)):
  maps_<name>.npz   the float64 restatement (tests/anomaly_ref.py + the CPU oracle's AlexNet per slice, tests/volume_ref.py) of the very
                    tensors the run handed to ``clamp_mse_``, at the 2-D maps' tolerances: squared error 2e-6, LPIPS 2e-5;
  the per-t maps    the fp32 tensors the run handed to ``MapPass.add_batch``, against the same restatement, same tolerances;
  map_stats.npz     float64 mean / std (ddof 1) of those per-t maps.  One update of B = 4 rows: mean within B u L (L = max |value|;
                    tests/test_gpu_anomaly_z_maps.py).  std: a deviation d = v - mb carries u |v| + B u L, so the sum of squares is
                    off by 2 (B + 1) u L sum |d| and, with sum |d| <= sqrt(n (n - 1)) std, the std by (B + 1) sqrt(n / (n - 1)) u L
                    < 6 u L; the B + 2 roundings of the squares and their sum add (B + 2) u std / 2 <= 3 u L: bound 16 u L, a
                    margin below 2 for the second-order terms;
  zmaps_<name>.npz  ``zmap_ref.zscore`` of those per-t maps with the tables ``finalize_tables`` makes of the FILE's fp32 mean and
                    std (restated here; float64 rounded once, so the same bits), then ``volume_ref.blur3d`` with the fp32 weights:
                    (2 n_t + 1) u L_z through three passes, plus the blur's own 6 (2 r + 1) u (1 + (2 r + 1) u)^2 max |z|.
"""

import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import anomaly_ref
import volume_ref as vref
import zmap_ref
from test_gpu_ops import _close

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MODEL = "decathlon_volume_maps"
SIZE = 32
SETS = {"val": f"synthetic:blobs3d:n=4:size={SIZE}:seed=10", "in": f"synthetic:blobs3d:n=4:size={SIZE}:seed=11",
        "NOISE": f"synthetic:noise3d:n=4:size={SIZE}:seed=12:name=NOISE"}
T_STARTS = [10, 650]
SIGMA = 1.0
FLAGS = ("--anomaly_volume_maps", "1", "--anomaly_volume_z_maps", "1", "--anomaly_z_sigma", str(SIGMA))
U = 2.0 ** -24


def _argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1", "--spatial_dimension", "3",
            "--vqvae_checkpoint", str(root / "vqvae" / "checkpoint.pth"), "--latent_pad", "(1,1,1,1,1,1)", "--b_scale", "0.5",
            "--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195", "--validation_ids", SETS["val"],
            "--in_ids", SETS["in"], "--out_ids", SETS["NOISE"], "--batch_size", "4", "--inference_skip_factor", "64", *extra]


def _run(root, tag, *extra):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    Reconstruct(args).reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept


class _Capture:
    """``ops.clamp_mse_`` as the trainer calls it (a copy of the originals and the clamped reconstruction per t-start) and
    ``MapPass.add_batch`` (a copy of the per-t maps per batch)."""

    def __init__(self, ops, map_pass_cls):
        self.ops, self.cls, self.real, self.real_add = ops, map_pass_cls, ops.clamp_mse_, map_pass_cls.add_batch
        self.calls, self.per_t = [], []

    def __enter__(self):
        def spy(orig, recon, b_scale=1.0):
            mse = self.real(orig, recon, b_scale)
            self.calls.append((orig.detach().cpu().clone(), recon.detach().cpu().clone()))
            return mse

        def add(mp, scores, maps, per_t_maps, mask=None):
            self.per_t.append(per_t_maps.detach().cpu().clone())
            return self.real_add(mp, scores, maps, per_t_maps, mask)

        self.ops.clamp_mse_, self.cls.add_batch = spy, add
        return self

    def __exit__(self, *exc):
        self.ops.clamp_mse_, self.cls.add_batch = self.real, self.real_add


def _restate(calls):
    """float64 [N, n_t, 2, D, H, W] of one data set (one batch) from the captured pairs: channel 0 the LPIPS map of the slices along
    the last axis, 1 the squared error, every t-start by itself."""
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS

    cpu = oracle.LPIPSAlex()
    cpu.load_state_dict(LPIPS().state_dict())  # the trainer's LPIPS without --lpips_weights: the seeded default
    assert len(calls) == len(T_STARTS) and all(torch.equal(o, calls[0][0]) for o, _ in calls)
    per_t = []
    for o, r in calls:
        lp = anomaly_ref.spatial_lpips(cpu, vref.volume_to_slices(o, 4), vref.volume_to_slices(r, 4), normalize=True)[:, 0]
        per_t.append(torch.stack([vref.slices_to_volume(lp, o.shape[0], 4), anomaly_ref.sqerr_map(o, r)], dim=1))
    return torch.stack(per_t, dim=1)


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from oracle.vqvae import VQVAE as OracleVQVAE
    from parity_util import VQ_README

    from ddpm_ood_amd import map_passes, synthetic, trainer

    root = tmp_path_factory.mktemp("volume_maps")
    torch.manual_seed(3)
    vq = OracleVQVAE(**VQ_README).eval()
    (root / "vqvae").mkdir()
    torch.save({"model_state_dict": synthetic.condition_vqvae_state_dict(vq.state_dict())}, root / "vqvae" / "checkpoint.pth")
    json.dump(VQ_README, open(root / "vqvae" / "vqvae_config.json", "w"))
    (root / MODEL).mkdir()
    sd = synthetic.random_state_dict("small", 128, spatial_dims=3, seed=1)
    torch.save({"epoch": 0, "global_step": 0, "model_state_dict": sd, "optimizer_state_dict": {}, "best_loss": 1000},
               root / MODEL / "checkpoint.pth")
    off = _run(root, "off")
    with _Capture(trainer.ops, map_passes.MapPass) as cap:
        on = _run(root, "on", *FLAGS)
    n_t = len(T_STARTS)
    assert len(cap.calls) == n_t * len(SETS) and len(cap.per_t) == len(SETS)  # one batch of 4 per set
    want = {name: _restate(cap.calls[k * n_t:(k + 1) * n_t]) for k, name in enumerate(SETS)}  # the run's order: val, in, out
    return root, off, on, dict(zip(SETS, cap.per_t)), want


def test_the_flags_leave_every_csv_as_it_was(runs):
    _, off, on, _, _ = runs
    names = sorted(f"results_{n}.csv" for n in SETS)
    assert sorted(p.name for p in off.iterdir()) == names  # flags off: nothing new
    assert sorted(p.name for p in on.iterdir()) == sorted(names + [f"maps_{n}.npz" for n in SETS] + ["map_stats.npz", "zmaps_in.npz",
                                                                                                       "zmaps_NOISE.npz"])
    for n in names:
        assert len(pd.read_csv(off / n)) == 4 * len(T_STARTS)
        assert (off / n).read_bytes() == (on / n).read_bytes(), n


def test_maps_file_matches_the_csv_and_the_float64_restatement(runs):
    _, _, on, per_t, want = runs
    for name in SETS:
        df = pd.read_csv(on / f"results_{name}.csv")
        z = np.load(on / f"maps_{name}.npz")
        assert sorted(z.files) == ["filename", "lpips_map", "mse_map", "t"]  # the keys of the 2-D file
        stems = list(dict.fromkeys(df["filename"].astype(str)))
        assert len(stems) == 4 and [str(s) for s in z["filename"]] == stems and z["t"].tolist() == T_STARTS == sorted(df["t"].unique())
        for key in ("lpips_map", "mse_map"):
            assert z[key].shape == (4, SIZE, SIZE, SIZE) and z[key].dtype == np.float32 and np.isfinite(z[key]).all() and (z[key] >= 0).all()
        csv_mse = np.array([df[df["filename"].astype(str) == s]["mse"].mean() for s in stems])
        got_mse = z["mse_map"].astype(np.float64).mean(axis=(1, 2, 3))
        rel = np.abs(got_mse - csv_mse) / csv_mse
        print(f"{name}: mse_map mean vs the CSV, worst relative difference {rel.max():.2e} (bound 1e-5)")
        assert (rel <= 1e-5).all()
        mean_t = want[name].mean(dim=1)
        _close(torch.from_numpy(z["lpips_map"]), mean_t[:, 0], tol=2e-5)
        _close(torch.from_numpy(z["mse_map"]), mean_t[:, 1], tol=2e-6)
        assert float(mean_t[:, 0].max()) > 1e-3 and float(mean_t[:, 1].max()) > 1e-3  # (maps with something in them)
        # every t-start by itself, as the statistics and the Z-maps receive it
        assert per_t[name].shape == (4, len(T_STARTS), 2, SIZE, SIZE, SIZE) and per_t[name].dtype == torch.float32
        _close(per_t[name][:, :, 0], want[name][:, :, 0], tol=2e-5)
        _close(per_t[name][:, :, 1], want[name][:, :, 1], tol=2e-6)


def _tables_of(path):
    """(mean32, inv_std32, rel_floor) as ``zmaps.finalize_tables`` makes them of the file's fp32 arrays, restated."""
    z = np.load(path)
    rel_floor = float(z["rel_floor"])
    return z["mean"], vref.floor_inv_std(z["std"], rel_floor).astype(np.float32), rel_floor


def test_statistics_and_z_maps_match_the_float64_restatement(runs):
    from ddpm_ood_amd import ops

    _, _, on, per_t, _ = runs
    n_t, B, radius = len(T_STARTS), 4, int(4 * SIGMA + 0.5)
    z = np.load(on / "map_stats.npz")
    assert sorted(z.files) == ["channels", "mean", "n", "rel_floor", "std", "t"]
    assert int(z["n"]) == 4 and z["t"].tolist() == T_STARTS and z["channels"].tolist() == ["lpips", "mse"] and float(z["rel_floor"]) == 0.01
    assert z["mean"].shape == (n_t, 2, SIZE, SIZE, SIZE) == z["std"].shape and z["mean"].dtype == np.float32 == z["std"].dtype
    val = per_t["val"].double().numpy()
    for c, name in enumerate(("lpips", "mse")):
        L = np.abs(val[:, :, c]).max()
        em = np.abs(z["mean"][:, c] - val[:, :, c].mean(axis=0)).max() / (U * L)
        es = np.abs(z["std"][:, c] - val[:, :, c].std(axis=0, ddof=1)).max() / (U * L)
        print(f"map_stats {name}: mean err {em:.2f} u L (bound {B} + 0.5 for the file's rounding), std err {es:.2f} u L (bound 16 + 0.5)")
        assert em <= B + 0.5 and es <= 16 + 0.5
        assert float(z["std"][:, c].max()) > 1e-4  # (statistics with something in them)
    mean32, inv32, rel_floor = _tables_of(on / "map_stats.npz")
    taps32 = ops.gaussian_taps(SIGMA).astype(np.float32)
    w = float(np.float32(1.0 / n_t))
    for name in ("in", "NOISE"):
        f = np.load(on / f"zmaps_{name}.npz")
        assert sorted(f.files) == ["filename", "rel_floor", "sigma", "t", "z_lpips_map", "z_mse_map"]  # the keys of the 2-D file
        df = pd.read_csv(on / f"results_{name}.csv")
        assert [str(s) for s in f["filename"]] == list(dict.fromkeys(df["filename"].astype(str)))
        assert f["t"].tolist() == T_STARTS and float(f["sigma"]) == SIGMA and float(f["rel_floor"]) == rel_floor
        v = per_t[name].double().numpy()
        addends = (v - mean32.astype(np.float64)[None]) * inv32.astype(np.float64)[None]
        Lz = (w * np.maximum(np.abs(addends).max(axis=1), np.abs(np.cumsum(addends, axis=1)).max(axis=1))).max()
        z64 = zmap_ref.zscore(v, mean32, inv32, weight=w)
        want = vref.blur3d(z64.reshape((-1, SIZE, SIZE, SIZE)), taps32).reshape(z64.shape)
        for c, key in enumerate(("z_lpips_map", "z_mse_map")):
            assert f[key].shape == (4, SIZE, SIZE, SIZE) and f[key].dtype == np.float32 and np.isfinite(f[key]).all()
            top = np.abs(z64[:, c]).max()
            bound = (2 * n_t + 1) * U * Lz * (1 + (2 * radius + 1) * U) ** 3 + 6 * (2 * radius + 1) * U * (1 + (2 * radius + 1) * U) ** 2 * top * (1 + 1e-6)
            err = np.abs(f[key] - want[:, c]).max()
            print(f"zmaps {name} {key}: err {err:.3e} (bound {bound:.3e}), max |z| {np.abs(want[:, c]).max():.3f}")
            assert err <= bound
            if name == "NOISE":
                assert np.abs(want[:, c]).max() > 1.0 and bound < 1e-3 * np.abs(want[:, c]).max()  # (a bound that means something)


def test_statistics_from_the_file_reproduce_the_z_maps_bit_for_bit(runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, _, on, _, _ = runs
    (root / MODEL / "ood").mkdir(exist_ok=True)
    shutil.copy(on / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")
    again = _run(root, "from_file", *FLAGS, "--run_val", "0")
    assert (again / "map_stats.npz").read_bytes() == (on / "map_stats.npz").read_bytes()  # read, not rewritten
    for n in ("zmaps_in.npz", "zmaps_NOISE.npz", "maps_in.npz", "maps_NOISE.npz"):
        a, b = np.load(on / n), np.load(again / n)
        assert sorted(a.files) == sorted(b.files)
        for key in a.files:
            assert np.array_equal(a[key], b[key]), (n, key)
    # the file's extent is checked: statistics of 32^3 volumes against a set of 48^3 ones
    (root / MODEL / "ood").mkdir(exist_ok=True)
    shutil.copy(on / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")
    args = cli.parse_args(_argv(root, *FLAGS, "--run_val", "0", "--run_out", "0", "--in_ids", "synthetic:blobs3d:n=1:size=48:seed=11",
                                "--latent_pad", "(0,1,0,1,0,1)"))
    with pytest.raises(ValueError, match="maps of"):
        Reconstruct(args).reconstruct(args)
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_ood_detection_scores_the_volume_files_unchanged(runs):
    root, _, on, _, _ = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL, "--out_data",
                              "NOISE", "--score", "zmap", "--zmap_key", "z_mse_map"], capture_output=True, text=True, check=True).stdout
        print(got)
        assert f"AUC for {MODEL} vs NOISE: " in got and "n_in=4 n_out=4" in got
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_all_views_change_the_lpips_maps_and_nothing_else(runs):
    root, _, on, _, _ = runs
    every = _run(root, "all_views", *FLAGS, "--anomaly_volume_views", "all")
    assert sorted(p.name for p in every.iterdir()) == sorted(p.name for p in on.iterdir())
    for p in sorted(on.iterdir()):
        if p.suffix == ".csv":
            assert p.read_bytes() == (every / p.name).read_bytes(), p.name
            continue
        a, b = np.load(p), np.load(every / p.name)
        assert sorted(a.files) == sorted(b.files)
        for key in a.files:
            if key in ("lpips_map", "z_lpips_map"):
                assert a[key].shape == b[key].shape and np.abs(a[key] - b[key]).max() > 1e-3, (p.name, key)
            elif key in ("mean", "std"):  # map_stats.npz: channel 0 is the LPIPS map's, channel 1 the squared error's
                assert np.array_equal(a[key][:, 1], b[key][:, 1]) and not np.array_equal(a[key][:, 0], b[key][:, 0]), (p.name, key)
            else:
                assert np.array_equal(a[key], b[key]), (p.name, key)
