"""GPU: the two kernels of csrc/pixel_metrics.hip against the numpy restatement of tests/pixel_ref.py (exact integer equality),
their memory bounds on the guard-band arena, and --pixel_metrics 1 through the trainer, the command line and two ranks
(DESIGN 3.23)."""

import argparse
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pixel_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# (1, 1, 1): one element, no chunk; (3, 5, 2): 15 elements, ragged tail; (2, 1024, 64): whole chunks; (5, 1023, 4096): rows that
# are no multiple of 4 (the counts' scalar path); (7, 4100, 8191): the largest histogram, several workgroups at the default parts;
# (64, 1024, 4096): four default parts
SHAPES = [(1, 1, 1), (3, 5, 2), (2, 1024, 64), (5, 1023, 4096), (7, 4100, 8191), (64, 1024, 4096)]
LO, HI = -16.0, 48.0
THRESHOLDS = [2.0, 3.0, 4.0, -20.0, 1e30]


@pytest.fixture(scope="module")
def cases():
    """Per shape: (maps, masks, the restatement's histogram), computed once."""
    out = {}
    for k, (N, P, nbins) in enumerate(SHAPES):
        v, m = ref.case_values(N, P, LO, HI, nbins, seed=k)
        out[N, P, nbins] = (v, m, ref.hist(v, m, LO, HI, nbins))
    return out


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _off_boundary(a, device, offset_bytes):
    """The array at `offset_bytes` behind a 256-byte aligned base: a contiguous view of a larger device buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    item = t.element_size()
    assert offset_bytes % item == 0
    buf = torch.zeros(t.numel() + 64, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 256 == 0
    view = buf[offset_bytes // item: offset_bytes // item + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == offset_bytes % 16 and view.is_contiguous()
    return view


# ---- 1. the histogram -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts", [1, 3, None], ids=["parts1", "parts3", "default"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_mask_hist_equals_the_restatement(device, cases, shape, parts):
    from ddpm_ood_amd import ops

    N, P, nbins = shape
    v, m, want = cases[shape]
    got = ops.map_mask_hist(_dev(v, device), _dev(m, device), LO, HI, nbins, parts=parts)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, nbins + 1)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(got.sum()) == N * P
    if N * P >= 15:  # the inputs do visit the special columns
        assert want[:, nbins].sum() >= 1 and want[:, 0].sum() >= 1 and want[:, nbins - 1].sum() >= 1 and (want[1] > 0).any()


def test_map_mask_hist_accumulates_and_a_rows_share_does_not_depend_on_the_batch(device, cases):
    from ddpm_ood_amd import ops

    N, P, nbins = 5, 1023, 4096
    v, m, want = cases[N, P, nbins]
    dv, dm = _dev(v, device), _dev(m, device)
    total = ops.map_mask_hist(dv[:2].contiguous(), dm[:2].contiguous(), LO, HI, nbins)
    again = ops.map_mask_hist(dv[2:].contiguous(), dm[2:].contiguous(), LO, HI, nbins, total=total)
    assert again is total and np.array_equal(total.cpu().numpy(), want)  # two calls = one call on the concatenation
    # row 3 alone, and as the difference of the batch with and without it
    alone = ops.map_mask_hist(dv[3:4].contiguous(), dm[3:4].contiguous(), LO, HI, nbins).cpu().numpy()
    rest = np.delete(np.arange(N), 3)
    without = ops.map_mask_hist(dv[rest].contiguous(), dm[rest].contiguous(), LO, HI, nbins).cpu().numpy()
    assert np.array_equal(alone, ref.hist(v[3:4], m[3:4], LO, HI, nbins)) and np.array_equal(want - without, alone)
    # a poisoned total is fine without accumulation: it is written, not read
    junk = torch.full((2, nbins + 1), -(1 << 40), dtype=torch.int64, device=device)
    lib_total = ops.map_mask_hist(dv, dm, LO, HI, nbins)
    from ddpm_ood_amd import _lib

    slabs = torch.full((2, 2, nbins + 1), -1, dtype=torch.int32, device=device)
    _lib.check(_lib.load().ddpm_map_mask_hist_f32(dv.data_ptr(), dm.data_ptr(), N, P, LO, float(ref.inv_step(LO, HI, nbins)), nbins, 2,
                                                  slabs.data_ptr(), junk.data_ptr(), 0, _lib.stream_ptr()), "map_mask_hist")
    assert torch.equal(junk, lib_total)


@pytest.mark.parametrize("map_off,mask_off", [(4, 0), (8, 1), (12, 2), (0, 3), (4, 3)])
def test_map_mask_hist_and_counts_off_a_16_byte_boundary(device, cases, map_off, mask_off):
    """Maps 4 / 8 / 12 bytes and masks 1 - 3 bytes off a 16-byte boundary: the head in front of the first 16-byte boundary, the
    byte loads of the masks, and the counts' scalar path give the aligned call's numbers."""
    from ddpm_ood_amd import ops

    for shape in ((2, 1024, 64), (7, 4100, 8191), (3, 5, 2)):
        N, P, nbins = shape
        v, m, want = cases[shape]
        dv, dm = _off_boundary(v, device, map_off), _off_boundary(m, device, mask_off)
        assert np.array_equal(ops.map_mask_hist(dv, dm, LO, HI, nbins).cpu().numpy(), want), shape
        assert np.array_equal(ops.map_mask_counts(dv, dm, THRESHOLDS).cpu().numpy(), ref.counts(v, m, THRESHOLDS)), shape


def test_what_the_two_ops_refuse(device):
    from ddpm_ood_amd import ops

    v = torch.zeros(4, 64, device=device)
    m = torch.zeros(4, 64, dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match="nbins"):
        ops.map_mask_hist(v, m, LO, HI, 8192)
    with pytest.raises(ValueError, match="nbins"):
        ops.map_mask_hist(v, m, LO, HI, 0)
    with pytest.raises(ValueError, match="thresholds"):
        ops.map_mask_counts(v, m, [float(k) for k in range(9)])
    with pytest.raises(ValueError, match="thresholds"):
        ops.map_mask_counts(v, m, [])
    with pytest.raises(ValueError, match="parts"):
        ops.map_mask_hist(v, m, LO, HI, 8, parts=0)
    with pytest.raises(ValueError, match="range"):
        ops.map_mask_hist(v, m, 1.0, 1.0, 8)
    # a total that overlaps an input: the library refuses (8 int64 counters x 2 classes... inside the maps' own bytes)
    inside = v.view(torch.int64)[0:1, :].reshape(-1)[:18].view(2, 9)
    with pytest.raises(ValueError, match="alias"):
        ops.map_mask_hist(v, m, LO, HI, 8, total=inside)
    for bad_v, bad_m in ((v.double(), m), (v, m.int()), (v.t(), m.t()), (v, m[:2]), (v.cpu(), m.cpu()), (v.reshape(-1), m.reshape(-1))):
        with pytest.raises(ValueError):
            ops.map_mask_hist(bad_v, bad_m, LO, HI, 8)
        with pytest.raises(ValueError):
            ops.map_mask_counts(bad_v, bad_m, [1.0])
    for total in (torch.zeros(2, 9, device=device), torch.zeros(2, 8, dtype=torch.int64, device=device), torch.zeros(2, 9, dtype=torch.int64)):
        with pytest.raises(ValueError, match="total"):
            ops.map_mask_hist(v, m, LO, HI, 8, total=total)


# ---- 2. the counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_mask_counts_equals_the_restatement(device, cases, shape):
    from ddpm_ood_amd import ops

    N, P, _ = shape
    v, m, _ = cases[shape]
    v = v.copy()
    if N >= 2:
        v[1] = np.nan  # a NaN row: nothing predicted, every masked pixel a false negative
    thr = [float(v[0, 0]) if np.isfinite(v[0, 0]) else 2.0, 3.0, -20.0]  # an exact map value: the comparison is strict
    got = ops.map_mask_counts(_dev(v, device), _dev(m, device), thr)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, 3, 3)
    want = ref.counts(v, m, thr)
    assert np.array_equal(got.cpu().numpy(), want)
    if N >= 2:
        assert (want[1, :, :2] == 0).all() and (want[1, :, 2] == (m[1] != 0).sum()).all()
    one = ops.map_mask_counts(_dev(v, device), _dev(m, device), torch.tensor(thr[:1], device=device))
    assert np.array_equal(one.cpu().numpy(), want[:, :1])
    eight = ops.map_mask_counts(_dev(v, device), _dev(m, device), thr + [0.0, 1.0, 5.0, 7.5, 47.0])
    assert np.array_equal(eight.cpu().numpy(), ref.counts(v, m, thr + [0.0, 1.0, 5.0, 7.5, 47.0]))


def test_map_mask_counts_of_a_row_alone(device):
    from ddpm_ood_amd import ops

    v, m = ref.case_values(6, 1023, LO, HI, 64, seed=40)
    batch = ops.map_mask_counts(_dev(v, device), _dev(m, device), THRESHOLDS)
    alone = ops.map_mask_counts(_dev(v[3:4], device), _dev(m[3:4], device), THRESHOLDS)
    assert torch.equal(batch[3:4], alone) and np.array_equal(batch.cpu().numpy(), ref.counts(v, m, THRESHOLDS))


# ---- 3. memory bounds ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 5, 2), (5, 1023, 4096), (7, 4100, 8191)], ids=lambda s: "x".join(map(str, s)))
def test_the_two_ops_stay_inside_their_buffers(device, cases, shape):
    """Inputs frozen, the outputs and the slabs poisoned (then zeroed), every pointer inside the arena; the ordinary call's result."""
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    N, P, nbins = shape
    v, m, want = cases[shape]
    tv, tm = torch.from_numpy(v), torch.from_numpy(m)
    for parts in (None, 3):
        plain, poison = _bounds(device, dict(v=(tv, True), m=(tm, True)), lambda t: ops.map_mask_hist(t["v"], t["m"], LO, HI, nbins, parts=parts))
        assert np.array_equal(plain.res[0].cpu().numpy(), want)
        n_parts = parts or ops.map_hist_parts(N * P)
        assert sorted(a.numel() for a in poison.allocated) == sorted([2 * (nbins + 1), n_parts * 2 * (nbins + 1)])
        assert [name for name, _ in poison.called] == ["ddpm_map_mask_hist_f32"]
    first = torch.from_numpy(ref.hist(v, m, LO, HI, nbins))

    def accumulate(t):
        return ops.map_mask_hist(t["v"], t["m"], LO, HI, nbins, total=t["total"])

    plain, _ = _bounds(device, dict(v=(tv, True), m=(tm, True), total=(first, False)), accumulate)
    assert np.array_equal(plain.res[0].cpu().numpy(), 2 * want)
    thr = torch.tensor(THRESHOLDS, dtype=torch.float32)
    plain, poison = _bounds(device, dict(v=(tv, True), m=(tm, True), thr=(thr, True)), lambda t: ops.map_mask_counts(t["v"], t["m"], t["thr"]))
    assert np.array_equal(plain.res[0].cpu().numpy(), ref.counts(v, m, THRESHOLDS))
    assert [a.numel() for a in poison.allocated] == [N * len(THRESHOLDS) * 3]
    plain, poison = _bounds(device, dict(v=(tv, True), m=(tm, True)), lambda t: ops.map_mask_counts(t["v"], t["m"], THRESHOLDS))
    assert sorted(a.numel() for a in poison.allocated) == sorted([len(THRESHOLDS), N * len(THRESHOLDS) * 3])  # the wrapper's upload too


# ---- 4. through the trainer -------------------------------------------------------------------------------------------------------------------
# 8 / 8 / 8 synthetic 32 x 32 images in batches of 4, the t-starts 10 and 30 only (1 + 3 UNet forwards per batch).

MODEL = "fashionmnist_pixels"
SETS = {"val": "synthetic:blobs:n=8:seed=10", "in": "synthetic:blobs:n=8:seed=11", "LES": "synthetic:lesion:n=8:mix=25:name=LES"}
FLAGS = ("--anomaly_z_maps", "1", "--pixel_metrics", "1", "--out_masks", "auto")


def _argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1", "--validation_ids", SETS["val"],
            "--in_ids", SETS["in"], "--out_ids", SETS["LES"], "--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015",
            "--beta_end", "0.0195", "--batch_size", "4", *extra]


def _run(root, tag, *extra):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    args.max_t_start, args.t_start_subset = 30, [10, 30]  # (the test hooks: a prefix of the chained list, two of its members)
    Reconstruct(args).reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("pixel_metrics")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    return root, _run(root, "z", "--anomaly_z_maps", "1"), _run(root, "px", *FLAGS)


def _with_stats_of(root, src):
    """A fresh ood/ holding only the statistics of the run kept in `src` (for --run_val 0)."""
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    (root / MODEL / "ood").mkdir()
    shutil.copy(src / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")


def _expected(zfile, masks, bins=4096, value_range=(LO, HI), thresholds=(2.0, 3.0, 4.0)):
    z = np.load(zfile)
    hist = np.stack([ref.hist(z[key], masks, *value_range, bins) for key in ("z_lpips_map", "z_mse_map")])
    counts = np.stack([ref.counts(z[key], masks, thresholds) for key in ("z_lpips_map", "z_mse_map")], axis=1)
    return hist, counts


def _check_file(path, zfile, masks, **kw):
    px = np.load(path)
    assert sorted(px.files) == sorted(["filename", "t", "channels", "lo", "hi", "nbins", "hist", "thresholds", "counts", "mask_pixels", "sigma"])
    hist, counts = _expected(zfile, masks, **kw)
    assert px["hist"].dtype == np.int64 and px["counts"].dtype == np.int32
    assert np.array_equal(px["hist"], hist) and np.array_equal(px["counts"], counts)
    assert np.array_equal(px["mask_pixels"], np.asarray(masks).reshape(len(masks), -1).astype(bool).sum(axis=1))
    assert [str(s) for s in px["filename"]] == [str(s) for s in np.load(zfile)["filename"]] and list(px["channels"]) == ["lpips", "mse"]
    return px


def test_pixels_file_equals_the_histogram_of_the_written_z_maps(runs):
    from ddpm_ood_amd import data

    root, off, on = runs
    masks = data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy()
    assert masks.any(axis=(1, 2, 3)).all()
    px = _check_file(on / "pixels_LES.npz", on / "zmaps_LES.npz", masks)
    assert px["hist"].sum() == 2 * 8 * 32 * 32 and px["hist"][:, 1].sum() == 2 * masks.sum() and list(px["t"]) == [10, 30]
    assert (float(px["lo"]), float(px["hi"]), int(px["nbins"]), float(px["sigma"])) == (LO, HI, 4096, 0.0)
    pin = _check_file(on / "pixels_in.npz", on / "zmaps_in.npz", np.zeros((8, 1, 32, 32), dtype=np.uint8))  # no masks: all negative
    assert pin["hist"][:, 1].sum() == 0 and (pin["counts"][..., 0] == 0).all() and (pin["counts"][..., 2] == 0).all()


def test_nothing_else_moves(runs):
    root, off, on = runs
    names = sorted(p.name for p in off.iterdir())
    assert names == sorted(["map_stats.npz", "results_LES.csv", "results_in.csv", "results_val.csv", "zmaps_LES.npz", "zmaps_in.npz"])
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["pixels_LES.npz", "pixels_in.npz"])
    for n in names:
        if n.endswith(".csv"):
            assert (off / n).read_bytes() == (on / n).read_bytes(), n
        else:
            a, b = np.load(off / n), np.load(on / n)
            assert sorted(a.files) == sorted(b.files)
            for key in a.files:
                assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f"), (n, key)


def test_two_batches_equal_one_and_other_settings(runs):
    from ddpm_ood_amd import data

    root, off, on = runs
    masks = data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy()
    _with_stats_of(root, on)
    one = _run(root, "px8", *FLAGS, "--batch_size", "8", "--run_val", "0", "--run_in", "0")
    _check_file(one / "pixels_LES.npz", one / "zmaps_LES.npz", masks)
    a, b = np.load(on / "pixels_LES.npz"), np.load(one / "pixels_LES.npz")
    for key in a.files:  # two batches of 4 accumulated = one batch of 8
        assert np.array_equal(a[key], b[key]), key
    _with_stats_of(root, on)
    other = _run(root, "px_other", *FLAGS, "--run_val", "0", "--run_in", "0", "--pixel_bins", "64", "--pixel_range", "-4", "12",
                 "--pixel_thresholds", "1.5", "--anomaly_z_sigma", "1.5")
    px = _check_file(other / "pixels_LES.npz", other / "zmaps_LES.npz", masks, bins=64, value_range=(-4.0, 12.0), thresholds=(1.5,))
    assert px["counts"].shape == (8, 2, 1, 3) and float(px["sigma"]) == 1.5


def test_command_line_prints_the_files_auroc(runs):
    from sklearn.metrics import roc_auc_score

    from ddpm_ood_amd import data
    from ddpm_ood_amd import pixel_metrics as pm

    root, off, on = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        px = np.load(on / "pixels_LES.npz")
        want = pm.auroc(px["hist"][1])
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL,
                              "--out_data", "LES", "--score", "pixel"], capture_output=True, text=True, check=True).stdout
        assert f"Pixel AUC for {MODEL} vs LES: {want * 100:.2f}" in got and "Best Dice" in got and "Mean image Dice" in got
        masks = data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy().reshape(-1)
        exact = roc_auc_score(masks, np.load(on / "zmaps_LES.npz")["z_mse_map"].reshape(-1).astype(np.float64))
        print(f"pixel AUROC of z_mse_map, random weights: 4096 bins {want:.6f}, unquantised {exact:.6f}, difference {want - exact:+.2e}")
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_on_one_gpu_reproduce_the_single_rank_file(device, runs):
    """reconstruct.py --pixel_metrics 1 as two ranks (gloo rendezvous, both on cuda:0) on the single-rank run's map_stats.npz: the
    Z-maps are the single-rank run's bits, so the all-reduced histogram is its histogram and every image's counts are its counts,
    rows rank-major (0 2 4 6, 1 3 5 7) as in the CSV.  The t-starts are those of --inference_skip_factor 99: t = 10 alone."""
    from test_gpu_dist import _launch_ranks

    root, off, on = runs
    extra = ("--run_val", "0", "--run_in", "0", "--inference_skip_factor", "99")
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    args = cli.parse_args(_argv(root, *FLAGS, "--run_in", "0", "--inference_skip_factor", "99"))
    Reconstruct(args).reconstruct(args)  # one rank: validation (the statistics at t = 10) and the out set
    single = root / MODEL / "ood_single_t10"
    shutil.copytree(root / MODEL / "ood", single)
    for p in (root / MODEL / "ood").iterdir():
        if p.name != "map_stats.npz":
            p.unlink()
    try:
        _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *FLAGS, *extra)], root, timeout=600)
        out = root / MODEL / "ood"
        assert sorted(p.name for p in out.iterdir()) == ["map_stats.npz", "pixels_LES.npz", "results_LES.csv", "zmaps_LES.npz"]
        one, two = np.load(single / "pixels_LES.npz"), np.load(out / "pixels_LES.npz")
        names = [str(s) for s in one["filename"]]
        order = [0, 2, 4, 6, 1, 3, 5, 7]
        assert [str(s) for s in two["filename"]] == [names[i] for i in order]
        assert np.array_equal(two["hist"], one["hist"]) and two["hist"].sum() == 2 * 8 * 32 * 32
        assert np.array_equal(two["counts"], one["counts"][order]) and np.array_equal(two["mask_pixels"], one["mask_pixels"][order])
        assert two["counts"].dtype == np.int32 and list(two["t"]) == [10]
        for key in ("lo", "hi", "nbins", "thresholds", "sigma", "channels"):
            assert np.array_equal(one[key], two[key]), key
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
