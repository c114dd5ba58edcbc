"""CPU: the host side of the likelihood baseline -- the coefficient table and the scheduler's mean / variance
against the float64 restatement (tests/likelihood_ref.py), the packing of (image, timestep) rows into forwards, the noise
addressing, the AUROC of the NLL column with its command line, and the C ABI of the two kernels
(tests/test_gpu_likelihood.py runs them)."""

import argparse
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import likelihood_ref as ref

ROOT = Path(__file__).resolve().parents[1]
G = Path(__file__).resolve().parent / "golden"
SCHED = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
T = 1000


def _closed_forms():
    """float64 tables of scaled_linear_beta 0.0015 .. 0.0195, from the closed form of the schedule."""
    beta = np.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, T, dtype=np.float64) ** 2
    alpha = 1.0 - beta
    abar = np.cumprod(alpha)
    abar_prev = np.concatenate([[1.0], abar[:-1]])
    return beta, alpha, abar, abar_prev


def test_coefficient_table_against_float64_closed_forms():
    from ddpm_ood_amd.scheduler import DDPMScheduler
    from ddpm_ood_amd.trainer import snr_shift_tables

    beta, alpha, abar, abar_prev = _closed_forms()
    c0 = np.sqrt(abar_prev) * beta / (1.0 - abar)
    ct = np.sqrt(alpha) * (1.0 - abar_prev) / (1.0 - abar)
    # The scheduler's tables are fp32: beta_t and alpha_t carry a relative 2^-24 each and abar_t, a product of t + 1 factors, at
    # most (t + 1) 2^-24 <= 6e-5.  1 - abar_t amplifies abar's ABSOLUTE error by 1 / (1 - abar_t) <= 1 / beta_0 = 667 at t = 0
    # (4e-5 relative) and less later, so every entry agrees with the closed form to 2e-4 relative.
    rtol = 2e-4
    for variance_type in ("fixed_small", "fixed_large"):
        s = DDPMScheduler(T, variance_type=variance_type, **SCHED)
        tab = s.likelihood_coefficients()
        assert tab.shape == (T, 6) and tab.dtype == np.float64
        var = np.maximum((1.0 - abar_prev) / (1.0 - abar) * beta, 1e-20) if variance_type == "fixed_small" else beta
        want = np.stack([np.sqrt(abar), np.sqrt(1.0 - abar), c0, ct, 0.5 / var, var ** -0.5], axis=1)
        assert np.allclose(tab[1:], want[1:], rtol=rtol, atol=0)
        assert np.allclose(tab[0, :3], want[0, :3], rtol=rtol, atol=0)
        # t = 0: abar_{-1} = 1, so ct is exactly 0 and c0 = beta_0 / (1 - abar_0) = 1 up to the fp32 rounding of the two tables
        assert tab[0, 3] == 0.0 and abs(tab[0, 2] - 1.0) <= 2.0 ** -23 / beta[0]
        raw = s.likelihood_coefficients(raw=True)
        if variance_type == "fixed_small":
            assert raw[0, 4] == 1e-20 == s._get_variance(0)  # (1 - 1) beta_0 / (1 - abar_0) = 0, floored
            assert tab[0, 4] == 0.5 / 1e-20 and np.isclose(tab[0, 5], 1e10, rtol=1e-12)
        else:
            assert np.array_equal(raw[:, 4], s.betas.double().numpy())  # var = beta_t, every t
            assert s._get_variance(0) == float(s.betas[0])
        # the table is read from the tables as they are at call time
        before = s.likelihood_coefficients()
        snr_shift_tables(s, 0.5)
        after = s.likelihood_coefficients()
        assert not np.allclose(before[:, 0], after[:, 0], rtol=1e-3, atol=0)
        a = s.alphas_cumprod.double().numpy()
        assert np.array_equal(after[:, 0], np.sqrt(a)) and np.array_equal(after[:, 1], np.sqrt(1.0 - a))


@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
def test_get_mean_and_get_variance_equal_the_restatement(variance_type):
    from ddpm_ood_amd.scheduler import DDPMScheduler
    from ddpm_ood_amd.trainer import snr_shift_tables

    s = DDPMScheduler(T, variance_type=variance_type, **SCHED)
    g = torch.Generator().manual_seed(5)
    x0, xt = torch.randn(2, 3, 5, generator=g, dtype=torch.float64), torch.randn(2, 3, 5, generator=g, dtype=torch.float64)
    for shifted in (False, True):
        if shifted:
            snr_shift_tables(s, 2.0)
        tab = ref.Tables(s)
        for t in (0, 1, 2, 500, 999):
            assert torch.allclose(s._get_mean(t, x0, xt), ref.get_mean(tab, t, x0, xt), rtol=1e-14, atol=1e-15)
            assert np.isclose(s._get_variance(t), float(ref.get_variance(tab, t)), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        s._get_variance(T)


@pytest.mark.parametrize("n,n_t,rows", [(1, 7, 4), (5, 20, 8), (3, 1000, 1024), (8, 20, 8), (9, 20, 8)])
def test_plan_rows_packs_every_pair_exactly_once(n, n_t, rows):
    from ddpm_ood_amd.inferer import plan_rows
    from ddpm_ood_amd.scheduler import DDPMScheduler

    s = DDPMScheduler(T, **SCHED)
    s.set_timesteps(n_t)
    steps = [int(t) for t in s.timesteps]
    plan = plan_rows(n, steps, rows)
    pairs, offset = [], 0
    for k, src, ts in plan:
        assert k == offset and len(src) == len(ts) and 1 <= len(src) <= rows
        offset += len(src)
        pairs += list(zip(src, ts))
    assert len(pairs) == n * n_t == len(set(pairs))
    assert set(pairs) == {(b, t) for b in range(n) for t in steps}
    assert all(len(src) == rows for _, src, _ in plan[:-1])  # packed: only the last forward may be short
    # rows_per_forward = n is the package's loop: one timestep per forward, in the scheduler's order
    one = plan_rows(n, steps, n)
    assert [p[2] for p in one] == [[t] * n for t in steps] and all(p[1] == list(range(n)) for p in one)
    with pytest.raises(ValueError):
        plan_rows(n, steps, 0)


def test_noise_addressing_is_a_function_of_seed_and_row_id_and_disjoint_from_sampling():
    from ddpm_ood_amd.scheduler import (LIKELIHOOD_STREAM, STREAMS_PER_ROW, likelihood_streams, sampling_key,
                                        sampling_streams)

    ids = [0, 1, 7, 12345, (1 << 47) - 1]
    streams = likelihood_streams(ids)
    assert streams == [i * 65536 + 65535 for i in ids] and LIKELIHOOD_STREAM == STREAMS_PER_ROW - 1
    assert likelihood_streams([7]) == [streams[2]]  # of the id alone: not of the batch or the position in it
    assert len(set(streams)) == len(ids)
    assert sampling_key(3) != sampling_key(4) and sampling_key(3) >> 63 == 1  # never a training key (those are < 2^63)
    # every stream a sampling run of ANY row id can read under the same key: row * 65536 + t, t <= T (x_T: t = T), T < 65535
    for t_max in (1000, 65534):
        used = {s % STREAMS_PER_ROW for s in sampling_streams(ids, t_max)} | {s % STREAMS_PER_ROW for s in sampling_streams(ids, 0)}
        assert max(used) <= t_max < LIKELIHOOD_STREAM
    all_sampling = {s for t in range(0, T + 1) for s in sampling_streams(ids, t)}
    assert not all_sampling & set(streams)


def test_get_likelihood_rejects_other_schedulers_and_long_schedules():
    from ddpm_ood_amd.inferer import DiffusionInferer
    from ddpm_ood_amd.scheduler import DDPMScheduler, PNDMScheduler

    inf = DiffusionInferer()
    with pytest.raises(NotImplementedError):
        inf.get_likelihood(torch.zeros(1, 1, 4, 4), None, PNDMScheduler(T, skip_prk_steps=True, **SCHED))
    with pytest.raises(ValueError, match="65535"):
        inf.get_likelihood(torch.zeros(1, 1, 4, 4), None, DDPMScheduler(65535, **SCHED))


def test_score_likelihood_matches_sklearn_and_drops_duplicates(tmp_path, capsys):
    from sklearn.metrics import roc_auc_score

    from ddpm_ood_amd import ood

    inn = pd.DataFrame({"filename": ["a", "b", "c", "d"], "type": "in", "nll": [1.0, 2.5, 0.5, 3.0]})
    out = pd.DataFrame({"filename": ["p", "q", "r"], "type": "out", "nll": [2.0, 4.0, 2.75]})
    for frame in (inn, out):
        frame["bpd"] = frame["nll"] / np.log(2.0)
    want = roc_auc_score([0, 0, 0, 0, 1, 1, 1], list(inn["nll"]) + list(out["nll"]))
    assert 0.5 < want < 1.0  # (a table that separates imperfectly: a flipped label or sign would show)
    # a padded shard repeats images: the first copy counts, the later ones (with values that would change the AUROC) do not
    inn_dup = pd.concat([inn, inn.iloc[:2].assign(nll=99.0)], ignore_index=True)
    out_dup = pd.concat([out, out.iloc[:1].assign(nll=-99.0)], ignore_index=True)
    table, auc = ood.score_likelihood(inn_dup, out_dup)
    assert auc == want and len(table) == 7 and list(table["type"]) == ["in"] * 4 + ["out"] * 3
    assert ood.score_likelihood(inn, out, column="bpd")[1] == want
    assert roc_auc_score([0] * 6 + [1] * 4, list(inn_dup["nll"]) + list(out_dup["nll"])) != want

    # the command line: ood_detection.py --score likelihood on CSVs written here
    run = tmp_path / "fashionmnist_x" / "ood"
    run.mkdir(parents=True)
    inn_dup.to_csv(run / "likelihood_in.csv", index=False)
    names = ood.out_datasets_for("fashionmnist_x")
    for name in names:
        out_dup.to_csv(run / f"likelihood_{name}.csv", index=False)
    base = [sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(tmp_path), "--model_name", "fashionmnist_x"]
    got = subprocess.run(base + ["--score", "likelihood"], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert f"AUC for fashionmnist_x vs {name}: {want * 100:.1f}" in got
    assert f"Average AUC: {want * 100:.1f}" in got

    # without the option: the reconstruction scoring, its output what ood.main prints for the same files
    df = pd.read_csv(G / "trajectory_rows.csv", index_col=0)
    val, inn_r, out_r = (df[df["type"] == t] for t in ("val", "in", "out"))
    val.to_csv(run / "results_val.csv")
    inn_r.to_csv(run / "results_in.csv")
    for name in names:
        out_r.to_csv(run / f"results_{name}.csv")
    capsys.readouterr()
    res = ood.main(argparse.Namespace(output_dir=str(tmp_path), model_name="fashionmnist_x", max_t=1000, min_t=0))
    want_stdout = capsys.readouterr().out
    plain = subprocess.run(base, capture_output=True, text=True, check=True).stdout
    assert plain == want_stdout and "Plot target is mse" in plain and "Score is the likelihood column" not in plain
    assert len(re.findall(r"^AUC for fashionmnist_x vs ", plain, flags=re.M)) == len(names) == len(res)


def test_likelihood_cli_reuses_the_reconstruction_flags():
    import likelihood as cli
    import reconstruct

    a, r = cli.parse_args([]), reconstruct.parse_args([])
    changed = {"num_inference_steps"}
    assert all(getattr(a, k) == v for k, v in vars(r).items() if k not in changed)  # same names, same defaults
    assert a.num_inference_steps is None and a.save_terms == 0 and a.batch_size == 256 and a.seed == 2
    b = cli.parse_args(["--num_inference_steps", "20", "--save_terms", "1", "--latent_pad", "(1,1,1,1)", "--b_scale", "0.5"])
    assert (b.num_inference_steps, b.save_terms, b.latent_pad, b.b_scale) == (20, 1, (1, 1, 1, 1), 0.5)


def test_exclusion_band_of_the_gpu_cases_holds_under_one_percent():
    """The fixed_small t = 0 comparison of tests/test_gpu_likelihood.py leaves out the elements whose float64 |x0 - pred_mean| lies
    within 1e-5 of bin_width / 2.  With x0 - x0hat uniform over +-3 bin widths the band holds 4 * 1e-5 / (6 / 255) = 0.17 % of
    the unclipped elements (more where the clamp folds x0hat onto +-1, never near the cap): the restatement alone, on the
    cases and seeds the GPU test uses, with x_t rounded to fp32 as the noising kernel leaves it."""
    import test_gpu_likelihood as cases
    from ddpm_ood_amd.scheduler import DDPMScheduler

    row_src, row_t = cases.make_rows()
    for shape in cases.ROW_SHAPES:
        x0, noise = cases.make_images(shape)
        for prediction_type in ("epsilon", "v_prediction", "sample"):
            for clip in (False, True):
                s = DDPMScheduler(T, prediction_type=prediction_type, clip_sample=clip, **SCHED)
                tab = ref.Tables(s)
                x_t = torch.stack([ref.add_noise(tab, t, x0[b], noise[b]).float() for b, t in zip(row_src, row_t)])
                out = cases.make_outputs(s, x0, x_t, row_src, row_t)
                inside = total = 0
                for r, (b, t) in enumerate(zip(row_src, row_t)):
                    if t == 0:
                        kl, d = ref.kl_map(tab, 0, x0[b][None], x_t[r][None], out[r][None], cases.BIN)
                        band = (d.abs() - cases.BIN / 2).abs() <= cases.BAND
                        inside += int(band.sum())
                        total += d.numel()
                        assert set(torch.unique(kl[~band]).tolist()) == {0.0, -np.log(1e-12)}  # a step function outside the band
                assert total >= 7 * x0[0].numel() and inside / total <= 0.01, (shape, prediction_type, clip, inside / total)


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    return _lib.load()


def test_entry_points_are_declared_exported_bound_and_return_int(lib):
    import ctypes as C

    from ddpm_ood_amd import _lib

    header = (ROOT / "include" / "ddpm_ood_hip.h").read_text()
    before = {n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t}
    for name in ("ddpm_vlb_noise_rows_f32", "ddpm_vlb_term_rows_f32"):
        assert re.search(rf"\bint {name}\(", header)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int  # no workspace, no size function
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is C.c_int
    assert not [n for n in before if "vlb" in n]
    assert lib.ddpm_abi_version() == 10 == _lib.ABI_VERSION  # additive entries: the ABI version stays
    assert "#define DDPM_ABI_VERSION 10" in header
    fake = 0x1000  # never dereferenced: the argument checks come first
    noise, term = lib.ddpm_vlb_noise_rows_f32, lib.ddpm_vlb_term_rows_f32
    assert noise(None, fake, fake, fake, fake, 10, fake + 64, 1, 4, None) == -1
    assert noise(fake, fake, fake, fake, fake, 0, fake + 64, 1, 4, None) == -1
    assert noise(fake, fake, fake, fake, fake, 10, fake, 1, 4, None) == -1 and b"aliases" in lib.ddpm_last_error()
    ok = (fake, fake, fake, fake, fake, fake, 10)
    assert term(*ok, 3, 0, 0.01, fake, None, 1, 4, None) == -1 and b"prediction_type" in lib.ddpm_last_error()
    assert term(*ok, 0, 0, 0.0, fake, None, 1, 4, None) == -1 and b"bin_width" in lib.ddpm_last_error()
    assert term(*ok, 0, 0, 0.01, None, None, 1, 4, None) == -1
    assert term(*ok, 0, 0, 0.01, fake + 64, fake, 1, 4, None) == -1 and b"aliases" in lib.ddpm_last_error()
    assert term(*ok, 0, 0, 0.01, fake + 64, None, 0, 4, None) == -1


def test_row_indices_are_range_checked_before_the_upload():
    from ddpm_ood_amd import ops

    for src, t in (([0, 3], [1, 1]), ([-1], [0]), ([0], [10]), ([0], [-1]), ([0, 1], [0]), ([], [])):
        with pytest.raises(ValueError):
            ops.VlbRows(src, t, 3, 10, "cpu")
    rows = ops.VlbRows([0, 2, 1], [9, 0, 5], 3, 10, "cpu")
    assert len(rows) == 3 and rows.src.dtype == torch.int32 and rows[1:3].t.tolist() == [0, 5]
    tab = ops.vlb_coef_table(np.arange(12, dtype=np.float64).reshape(2, 6) / 7.0, "cpu")
    assert tab.shape == (2, 8) and tab.dtype == torch.float32 and tab[:, 6:].abs().sum() == 0
    assert np.array_equal(tab[:, :6].numpy(), (np.arange(12).reshape(2, 6) / 7.0).astype(np.float32))
