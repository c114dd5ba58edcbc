"""-m gpu: thresholds calibrated on leave-one-out validation Z-maps -- ``ops.map_zscore_loo`` against the float64
brute force of tests/calibration_ref.py (row i deleted, the others' statistics recomputed), its two paths bit for bit, its edges,
refusals and memory bounds, and ``reconstruct.py --pixel_calibrate_fpr`` through the trainer, ``--run_val 0`` and two ranks.

The accuracy bound is not a number: the test evaluates the kernel's formula in fp32 numpy on the same inputs and asks the
kernel's largest error to stay within 4 x that restatement's largest error (operation order in ``weight``, sqrt / divide
rounding).  The figures measured on an MI355X are in profiles/pixel_calibration.md."""

import shutil
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import calibration_ref as ref
import pixel_ref
import region_ref
from guard_util import Arena, bits, need_bytes
from test_gpu_pixel_metrics import HI, LO, MODEL, _argv

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24
B = 5


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _off_boundary(t, device):
    """The same values on the device, 4 bytes behind a 16-byte boundary."""
    out = torch.cat([torch.zeros(1), t.reshape(-1)]).to(device)[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.fixture(scope="module")
def cases():
    """Per (n, H, W): the fp32 values, the tables the kernel reads (float64 statistics rounded once), the float64 brute force of
    the first B rows and the fp32 restatement on the same inputs -- computed once, shared, never changed."""
    out = {}
    for n in (8, 33):
        for H, W in ((7, 9), (8, 8)):
            v = ref.case_values(n, 3, H, W)
            _, mean, m2 = ref.stats(v)
            mean32, m232 = mean.astype(np.float32), m2.astype(np.float32)
            floor32 = ref.floor_table(v).astype(np.float32)
            want = ref.loo_brute(v, floor32, rows=range(B))
            out[n, H, W] = dict(v=v, mean=mean32, m2=m232, floor=floor32, want=want, fp32=ref.loo_fp32(v[:B], n, mean32, m232, floor32))
    return out


def _dev(case, device, rows=slice(0, B)):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (case["v"][rows], case["mean"], case["m2"], case["floor"])]


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(7, 9), (8, 8)], ids=["scalar", "vector"])
@pytest.mark.parametrize("n", [8, 33])
def test_map_zscore_loo_against_the_float64_brute_force(device, cases, n, H, W):
    """The kernel's largest absolute error against the brute force is at most 4 x the largest error of the fp32 numpy
    restatement of its formula on the same inputs (both include the rounding of the tables to fp32)."""
    from ddpm_ood_amd import ops

    c = cases[n, H, W]
    v, mean, m2, floor = _dev(c, device)
    got = ops.map_zscore_loo(v, mean, m2, n, floor)
    assert got.shape == (B, 2, H, W) and got.dtype == torch.float32
    got = got.cpu().double().numpy()
    err, own = np.abs(got - c["want"]).max(), np.abs(c["fp32"].astype(np.float64) - c["want"]).max()
    print(f"map_zscore_loo n={n} plane {H}x{W}: kernel err {err:.3e}, fp32 restatement err {own:.3e} (bound {4 * own:.3e}), "
          f"max |Z| {np.abs(c['want']).max():.1f}")
    assert own > 0 and err <= 4 * own
    assert np.abs(c["want"]).max() > 10.0 and c["want"][1, :, 0, 0].min() > 10.0  # (the outlier column is among the rows)
    # an explicit weight: the sum over t instead of the mean
    total = ops.map_zscore_loo(v, mean, m2, n, floor, weight=1.0).cpu().double().numpy()
    assert np.abs(total - 3.0 * c["want"]).max() <= 3.0 * 4 * own


def test_three_rows_finite_signed_and_floored(device):
    """n = 3: m2 - d dl cancels, so no accuracy is asked.  Finite everywhere; the sign of v - mean (one t-start); and the floor
    branch: where the other two rows are equal q clamps to 0 and the divisor is the floor -- 1, 1, 4 gives mean 2, d = 2,
    dl = 3, m2 = 6 = d dl exactly, so Z = 3 / floor; three equal rows give 0 / floor = 0, not 0 / 0."""
    from ddpm_ood_amd import ops

    for H, W in ((7, 9), (8, 8)):
        v = ref.case_values(3, 1, H, W)
        v[:, 0, :, 2, 3] = np.asarray([1.0, 1.0, 4.0], dtype=np.float32)[:, None]
        v[:, 0, :, 4, 5] = 0.25
        _, mean, m2 = ref.stats(v)
        assert (m2[0, :, 2, 3] == 6.0).all() and (m2[0, :, 4, 5] == 0.0).all()
        floor = ref.floor_table(v).astype(np.float32)
        ins = [torch.from_numpy(a).to(device) for a in (v, mean.astype(np.float32), m2.astype(np.float32), floor)]
        got = ops.map_zscore_loo(ins[0], ins[1], ins[2], 3, ins[3]).cpu().numpy()
        assert got.shape == (3, 2, H, W) and np.isfinite(got).all()
        d = v.astype(np.float64)[:, 0] - mean[0]
        clear = np.abs(d) > 1e-3 * np.abs(mean[0])
        assert clear.mean() > 0.9 and (np.sign(got[clear]) == np.sign(d[clear])).all()
        assert np.array_equal(got[2, :, 2, 3], np.float32(3.0) / floor[0])  # the floor branch, exactly
        assert (got[:, :, 4, 5] == 0).all()
        # n = 4 as well: finite (the same cancellation, one more row)
        v4 = ref.case_values(4, 3, H, W)
        _, mean, m2 = ref.stats(v4)
        ins = [torch.from_numpy(a).to(device) for a in (v4, mean.astype(np.float32), m2.astype(np.float32), ref.floor_table(v4).astype(np.float32))]
        assert bool(torch.isfinite(ops.map_zscore_loo(ins[0], ins[1], ins[2], 4, ins[3])).all())


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------------

def test_both_paths_split_batches_and_a_given_out_give_the_same_bits(device, cases):
    from ddpm_ood_amd import ops

    c = cases[33, 8, 8]
    v, mean, m2, floor = _dev(c, device)
    want = ops.map_zscore_loo(v, mean, m2, 33, floor)
    assert all(t.data_ptr() % 16 == 0 for t in (v, mean, m2, want))  # the 16-byte path
    for who in ("values", "mean", "m2", "out", "all"):  # a base 4 bytes off: the scalar path, on the same data
        ins = [(_off_boundary(t.cpu(), device) if who in (name, "all") else t) for name, t in (("values", v), ("mean", mean), ("m2", m2))]
        out = _off_boundary(torch.zeros(B, 2, 8, 8), device) if who in ("out", "all") else None
        got = ops.map_zscore_loo(*ins, 33, floor, out=out)
        assert (out is None or got is out) and _bits(got, want), who
    # one call with B = 5 equals calls of 2 + 3; a row alone; a row in another place
    two, three = ops.map_zscore_loo(v[:2].contiguous(), mean, m2, 33, floor), ops.map_zscore_loo(v[2:].contiguous(), mean, m2, 33, floor)
    assert _bits(torch.cat([two, three]), want)
    assert _bits(ops.map_zscore_loo(v[3:4].contiguous(), mean, m2, 33, floor), want[3:4])
    assert _bits(ops.map_zscore_loo(v[[4, 3, 0]].contiguous(), mean, m2, 33, floor)[1:2], want[3:4])
    # out= given equals a fresh out, whatever it held
    out = torch.full((B, 2, 8, 8), float("nan"), device=device)
    assert ops.map_zscore_loo(v, mean, m2, 33, floor, out=out) is out and _bits(out, want)
    # the scalar plane (7 x 9) the same three ways
    c = cases[8, 7, 9]
    v, mean, m2, floor = _dev(c, device)
    want = ops.map_zscore_loo(v, mean, m2, 8, floor)
    assert _bits(torch.cat([ops.map_zscore_loo(v[:2].contiguous(), mean, m2, 8, floor), ops.map_zscore_loo(v[2:].contiguous(), mean, m2, 8, floor)]), want)
    assert _bits(ops.map_zscore_loo(_off_boundary(v.cpu(), device), mean, m2, 8, floor), want)


# ---- 3. edges and errors ----------------------------------------------------------------------------------------------------------------------------

def test_a_nan_stays_at_its_own_pixel(device, cases):
    from ddpm_ood_amd import ops

    for key, at in (((8, 8, 8), (1, 2, 1, 5, 6)), ((8, 7, 9), (4, 0, 0, 6, 8))):
        c = cases[key]
        v, mean, m2, floor = _dev(c, device)
        clean = ops.map_zscore_loo(v, mean, m2, 8, floor).cpu()
        v[at] = float("nan")
        dirty = ops.map_zscore_loo(v, mean, m2, 8, floor).cpu()
        bad = torch.isnan(dirty)
        assert int(bad.sum()) == 1 and bool(bad[at[0], at[2], at[3], at[4]])
        assert torch.equal(dirty[~bad], clean[~bad])


def test_what_the_op_refuses(device, cases):
    from ddpm_ood_amd import ops

    v, mean, m2, floor = _dev(cases[8, 8, 8], device)
    for n in (2, 1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="n >= 3"):
            ops.map_zscore_loo(v, mean, m2, n, floor)
    for bad in ((v, mean[:2], m2, floor), (v, mean, m2[:, :1], floor), (v, mean, m2, floor[:2]), (v, mean, m2, floor.reshape(-1)),
                (v[:, :, :1], mean[:, :1], m2[:, :1], floor[:, :1]), (v.reshape(B, 3, 2 * 64), mean.reshape(3, 128), m2.reshape(3, 128), floor),
                (v.double(), mean, m2, floor), (v.transpose(3, 4), mean.transpose(2, 3), m2.transpose(2, 3), floor),
                (v.cpu(), mean, m2, floor), (v, mean.cpu(), m2, floor), (v, mean, m2, floor.cpu()), (v[:0], mean, m2, floor)):
        with pytest.raises(ValueError):
            ops.map_zscore_loo(*bad[:3], 8, bad[3])
    for out in (torch.empty(B, 2, 8, 9, device=device), torch.empty(B, 2, 8, 8), torch.empty(B, 2, 8, 8, dtype=torch.float64, device=device)):
        with pytest.raises(ValueError, match="out"):
            ops.map_zscore_loo(v, mean, m2, 8, floor, out=out)
    tables = torch.rand(4, 3, 2, 8, 8, device=device)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_zscore_loo(v, mean, m2, 8, floor, out=v.view(-1)[64:64 + B * 128].view(B, 2, 8, 8))
    with pytest.raises(ValueError, match="aliases"):
        ops.map_zscore_loo(tables[:2].contiguous(), tables[2], tables[3], 8, floor, out=tables.view(-1)[2 * 384 + 128:2 * 384 + 384].view(2, 2, 8, 8))
    with pytest.raises(ValueError, match="aliases"):
        ops.map_zscore_loo(tables[:2].contiguous(), tables[2], tables[3], 8, floor, out=tables.view(-1)[3 * 384:3 * 384 + 256].view(2, 2, 8, 8))


@pytest.mark.parametrize("H,W", [(8, 8), (7, 9)], ids=["V4", "V1"])
def test_the_entry_point_stays_inside_its_buffers(device, cases, H, W):
    """The C entry point on the guard-band arena: the inputs frozen, ``out`` left poisoned, then zeroed -- no guard word and no
    input changes, and the result is the ordinary call's bits both times (``out``'s contents are not read)."""
    from ddpm_ood_amd import _lib, ops

    c = cases[8, H, W]
    lib = _lib.load()
    want = ops.map_zscore_loo(*_dev(c, device)[:3], 8, _dev(c, device)[3])
    shapes = [a.shape for a in (c["v"][:B], c["mean"], c["m2"], c["floor"])] + [(B, 2, H, W)]
    for zero in (False, True):
        arena = Arena(device, need_bytes([4 * int(np.prod(s)) for s in shapes]))
        ins = [arena.alloc(a.shape, torch.float32, fill=torch.from_numpy(np.ascontiguousarray(a)), name=name, input_only=True)
               for name, a in (("values", c["v"][:B]), ("mean", c["mean"]), ("m2", c["m2"]), ("floor", c["floor"]))]
        out = arena.alloc((B, 2, H, W), torch.float32, name="out")
        if zero:
            out.zero_()
        arena.freeze()
        _lib.check(lib.ddpm_map_zscore_loo_f32(*(t.data_ptr() for t in ins), out.data_ptr(), B, 3, H * W, 8, float(np.float32(1.0 / 3)),
                                               _lib.stream_ptr()), "map_zscore_loo")
        arena.check()
        assert torch.equal(bits(out), bits(want)), "zeroed" if zero else "poisoned"


# ---- 4. through the trainer ---------------------------------------------------------------------------------------------------------------------
# The fixture of tests/test_gpu_pixel_metrics.py: 8 / 8 / 8 synthetic 32 x 32 images in batches of 4, the t-starts 10 and 30 only.

SIGMA = 1.0
BASE = ("--anomaly_z_maps", "1", "--pixel_metrics", "1", "--out_masks", "auto", "--pixel_regions", "1", "--anomaly_z_sigma", str(SIGMA))
CAL = ("--pixel_calibrate_fpr", "0.05,0.01")
FPRS = [0.05, 0.01]
NBINS, STEP = 4096, (HI - LO) / 4096


def _run(root, tag, *extra, hooks=True):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    if hooks:
        args.max_t_start, args.t_start_subset = 30, [10, 30]
    args.keep_calibration_rows = True
    rec = Reconstruct(args)
    rec.reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept, rec


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("pixel_calibration")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    off, _ = _run(root, "off", *BASE)
    on, rec = _run(root, "on", *BASE, *CAL)
    return root, off, on, rec


def test_nothing_that_was_written_before_moves(runs):
    root, off, on, _ = runs
    names = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["calibration.npz", "calibrated_in.npz", "calibrated_LES.npz"])
    for n in names:
        assert (off / n).read_bytes() == (on / n).read_bytes(), n


def test_files_hold_the_stated_keys_and_the_quantile_rule(runs):
    from ddpm_ood_amd import pixel_metrics as pm

    root, off, on, _ = runs
    cal = np.load(on / "calibration.npz")
    assert sorted(cal.files) == sorted(pm.CALIBRATION_KEYS)
    assert cal["t"].tolist() == [10, 30] and int(cal["n"]) == 8 and cal["fpr"].tolist() == FPRS and cal["channels"].tolist() == ["lpips", "mse"]
    assert (float(cal["lo"]), float(cal["hi"]), int(cal["nbins"]), float(cal["sigma"]), float(cal["rel_floor"])) == (LO, HI, NBINS, SIGMA, 0.01)
    assert cal["bin"].shape == (2, 2) and cal["bin"].dtype.kind == "i" and cal["thresholds"].shape == (2, 2) and cal["thresholds"].dtype == np.float32
    assert cal["hist"].shape == (2, NBINS + 1) and cal["hist"].dtype == np.int64
    assert (cal["hist"][:, :-1].sum(axis=1) == 8 * 32 * 32).all() and (cal["hist"][:, -1] == 0).all()
    for c in range(2):
        N = cal["hist"][c, :-1].sum()
        for j, f in enumerate(FPRS):
            k = int(cal["bin"][c, j])
            above, one_lower = cal["hist"][c, k:-1].sum() / N, cal["hist"][c, k - 1:-1].sum() / N
            print(f"channel {c} f={f}: k*={k} threshold {cal['thresholds'][c, j]:.4f} reaches {above:.5f} (one bin lower {one_lower:.5f})")
            assert above <= f < one_lower and cal["thresholds"][c, j] == np.float32(LO + k * STEP)
    for name in ("in", "LES"):
        z = np.load(on / f"calibrated_{name}.npz")
        assert sorted(z.files) == ["components", "counts", "filename", "fpr", "thresholds"]
        assert z["counts"].shape == (8, 2, 2, 3) == z["components"].shape and z["counts"].dtype == np.int32 == z["components"].dtype
        assert np.array_equal(z["thresholds"], cal["thresholds"]) and z["fpr"].tolist() == FPRS
        assert [str(s) for s in z["filename"]] == [str(s) for s in np.load(on / f"zmaps_{name}.npz")["filename"]]


def test_validation_z_maps_and_thresholds_match_the_float64_recomputation(runs):
    """From the rows the trainer retained: the float64 brute force, then scipy's gaussian_filter.  Tolerance: 4 x the error of the
    fp32 restatement evaluated with the run's own fp32 tables (the kernel's bound) plus what ``map_blur``'s test allows,
    4 (2 r + 1) u (1 + (2 r + 1) u) max |Z| at radius 4.  The recomputed thresholds lie within one bin step of the file's."""
    from ddpm_ood_amd import pixel_metrics as pm

    root, off, on, rec = runs
    rows, got = rec.calibration_rows, rec.calibration_zmaps
    assert rows.shape == (8, 2, 2, 32, 32) and got.shape == (8, 2, 32, 32) and rows.dtype == np.float32 == got.dtype
    stats = rec.last_map_stats[0]
    n, mean, m2 = stats.tables()
    floor32 = stats.floor(0.01)
    assert n == 8
    want_raw = ref.loo_brute(rows, floor32)
    own = np.abs(ref.loo_fp32(rows, 8, mean.astype(np.float32), m2.astype(np.float32), floor32).astype(np.float64) - want_raw).max()
    radius = int(4 * SIGMA + 0.5)
    tol = 4 * own + 4 * (2 * radius + 1) * U * (1 + (2 * radius + 1) * U) * np.abs(want_raw).max()
    want = ref.blur(want_raw, SIGMA)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"validation Z-maps: err {err:.3e} (bound {tol:.3e}: restatement {own:.3e}), max |Z| raw {np.abs(want_raw).max():.2f} smoothed {np.abs(want).max():.2f}")
    assert err <= tol and np.abs(want).max() > 1.0
    cal = np.load(on / "calibration.npz")
    for c in range(2):
        hist = np.bincount(ref.bin_of(want[:, c], LO, HI, NBINS).reshape(-1), minlength=NBINS + 1)
        _, thr = pm.thresholds_from_hist(hist, LO, HI, FPRS)
        print(f"channel {c}: thresholds {cal['thresholds'][c].tolist()} recomputed {thr.tolist()}")
        assert np.abs(thr - cal["thresholds"][c]).max() <= STEP
        assert np.array_equal(cal["hist"][c], np.bincount(ref.bin_of(got[:, c], LO, HI, NBINS).reshape(-1), minlength=NBINS + 1))


def test_counts_equal_numpy_on_the_written_z_maps(runs):
    from ddpm_ood_amd import data

    root, off, on, _ = runs
    cal = np.load(on / "calibration.npz")
    masks = {"LES": data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy().reshape(8, 32, 32), "in": np.zeros((8, 32, 32), dtype=np.uint8)}
    for name, m in masks.items():
        z, done = np.load(on / f"zmaps_{name}.npz"), np.load(on / f"calibrated_{name}.npz")
        for c, key in enumerate(("z_lpips_map", "z_mse_map")):
            thr = cal["thresholds"][c]
            assert np.array_equal(done["counts"][:, c], pixel_ref.counts(z[key].reshape(8, -1), m.reshape(8, -1), thr)), (name, key)
            for j, t in enumerate(thr):
                pred = z[key] > t
                want = np.stack([(pred & (m != 0)).sum(axis=(1, 2)), (pred & (m == 0)).sum(axis=(1, 2)), (~pred & (m != 0)).sum(axis=(1, 2))], axis=1)
                assert np.array_equal(done["counts"][:, c, j], want), (name, key, j)
            labels, regions = region_ref.label(m, 8)
            assert np.array_equal(done["components"][:, c], region_ref.component_counts(z[key], m, labels, regions, thr, 8)), (name, key)
    assert np.load(on / "calibrated_LES.npz")["counts"][..., 0].sum() > 0  # (something is found)


def test_stored_calibration_reproduces_the_files_and_foreign_settings_are_refused(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, off, on, _ = runs

    def with_files_of(src):
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
        (root / MODEL / "ood").mkdir()
        for n in ("map_stats.npz", "calibration.npz"):
            shutil.copy(src / n, root / MODEL / "ood" / n)

    with_files_of(on)
    again, _ = _run(root, "from_file", *BASE, *CAL, "--run_val", "0")
    assert (again / "calibration.npz").read_bytes() == (on / "calibration.npz").read_bytes()  # read, not rewritten
    for n in ("calibrated_in.npz", "calibrated_LES.npz", "pixels_LES.npz", "regions_LES.npz"):
        assert (again / n).read_bytes() == (on / n).read_bytes(), n
    for extra, text in ((("--anomaly_z_sigma", "1.5"), "--anomaly_z_sigma"), (("--pixel_bins", "1024"), "--pixel_bins"),
                        (("--pixel_range", "-8", "48"), "--pixel_range"), (("--anomaly_z_std_floor", "0.02"), "--anomaly_z_std_floor")):
        with_files_of(on)
        args = cli.parse_args(_argv(root, *BASE, *CAL, "--run_val", "0", "--run_in", "0", *extra))
        args.max_t_start, args.t_start_subset = 30, [10, 30]
        with pytest.raises(ValueError, match=text):
            Reconstruct(args).reconstruct(args)
    with_files_of(on)
    args = cli.parse_args(_argv(root, *BASE, *CAL, "--run_val", "0", "--run_in", "0"))
    args.max_t_start, args.t_start_subset = 30, [10]  # another list of t-starts: the statistics file refuses first
    with pytest.raises(ValueError, match="t-starts"):
        Reconstruct(args).reconstruct(args)
    (root / MODEL / "ood" / "calibration.npz").unlink()
    args.t_start_subset = [10, 30]
    with pytest.raises(FileNotFoundError, match="--pixel_calibrate_fpr"):
        Reconstruct(args).reconstruct(args)
    # the budget: 8 rows x 2 t-starts x 2 x 32 x 32 fp32 = 131 072 bytes on this rank
    args = cli.parse_args(_argv(root, *BASE, *CAL, "--pixel_calibrate_budget_gb", str(131071 / 2 ** 30)))  # (refused before the pass)
    args.max_t_start, args.t_start_subset = 30, [10, 30]
    with pytest.raises(ValueError, match=r"8 x 2 x 2 x 32 x 32 fp32.*--pixel_calibrate_budget_gb"):
        Reconstruct(args).reconstruct(args)
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_command_line_prints_the_calibrated_lines(runs, capsys):
    import argparse

    from ddpm_ood_amd import ood

    root, off, on, _ = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        args = argparse.Namespace(output_dir=str(root), model_name=MODEL, zmap_key="z_mse_map", pixel_include_in=0, pixel_regions=1,
                                  pixel_pro_fpr=0.3, pixel_calibrated=1)
        got = ood.main_pixels(args, out_data=["LES"])["LES"]["calibrated"]
        out = capsys.readouterr().out
        print(out)
        cal = np.load(on / "calibration.npz")
        assert [r["threshold"] for r in got] == [float(t) for t in cal["thresholds"][1]]
        assert all(r["val_fpr"] <= r["fpr"] and 0.0 <= r["in_fpr"] <= 1.0 and 0.0 <= r["pooled_dice"] <= 1.0 for r in got)
        assert out.count("Calibrated for ") == 2 and out.count("Calibrated regions for ") == 2
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_calibrate_within_one_bin_step_of_one_rank(device, runs):
    """reconstruct.py --pixel_calibrate_fpr as two ranks (t = 10 alone, --inference_skip_factor 99): each rank keeps its 4 validation
    rows, both upload the merged tables, ONE all_reduce sums the histograms.  The merged statistics differ from the single rank's
    in their last bits, so the thresholds may move by a bin; the rows of calibrated_LES.npz are in the CSV's order."""
    if torch.cuda.device_count() < 2:
        pytest.skip("no second device")
    from test_gpu_dist import _launch_ranks

    root = runs[0]
    extra = (*BASE, *CAL, "--run_in", "0", "--inference_skip_factor", "99")
    single, _ = _run(root, "single_t10", *extra, hooks=False)
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    try:
        _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *extra)], root, timeout=600)
        out = root / MODEL / "ood"
        one, two = np.load(single / "calibration.npz"), np.load(out / "calibration.npz")
        assert two["t"].tolist() == [10] and int(two["n"]) == 8 and two["hist"][:, :-1].sum() == 2 * 8 * 32 * 32
        print(f"thresholds one rank {one['thresholds'].tolist()} two ranks {two['thresholds'].tolist()}")
        assert np.abs(two["thresholds"].astype(np.float64) - one["thresholds"]).max() <= STEP
        done = np.load(out / "calibrated_LES.npz")
        df = pd.read_csv(out / "results_LES.csv")
        assert [str(s) for s in done["filename"]] == list(dict.fromkeys(df["filename"].astype(str)))
        names = [str(s) for s in np.load(single / "calibrated_LES.npz")["filename"]]
        assert [str(s) for s in done["filename"]] == [names[i] for i in (0, 2, 4, 6, 1, 3, 5, 7)]
        z = np.load(out / "zmaps_LES.npz")
        assert [str(s) for s in z["filename"]] == [str(s) for s in done["filename"]]
        from ddpm_ood_amd import data

        m = data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy().reshape(8, -1)[[0, 2, 4, 6, 1, 3, 5, 7]]
        for c, key in enumerate(("z_lpips_map", "z_mse_map")):
            assert np.array_equal(done["counts"][:, c], pixel_ref.counts(z[key].reshape(8, -1), m, two["thresholds"][c]))
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
