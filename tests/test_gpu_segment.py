"""GPU: the kernels of csrc/segment.hip against the numpy restatements of tests/segment_ref.py (values and integers exactly), and
--pixel_segment 1 through the trainer, the command line and two ranks."""

import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import region_ref
import segment_ref as ref
from test_gpu_region_metrics import MODEL, ROOT, SHAPES, _argv, _dev, _flags, _hand_masks, _inputs, _masks_of, _run, _with_stats_of

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD
# the first four: a radius above the plane; odd sizes; more than one tile in x (64) and y (16); 130 x 257: five tiles in x, nine in y
MEDIAN_SHAPES = [(1, 1, 1), (2, 1, 9), (2, 9, 1), (1, 2, 2), (3, 5, 7), (2, 33, 31), (1, 64, 64), (1, 128, 128), (1, 130, 257)]


def _ids(s):
    return "x".join(map(str, s))


# ---- 1. median --------------------------------------------------------------------------------------------------------------------

def _median_inputs(shape):
    """name -> fp32 [N, H, W]: few distinct values (ties in every window), +-inf and both zeros, NaN (of either sign) at 10 % and at
    60 % of the pixels (most windows hold more NaN than numbers)."""
    rng = np.random.default_rng(shape[1] * 1000 + shape[2])
    ties = rng.integers(-3, 4, size=shape).astype(np.float32)
    wide = rng.standard_normal(shape).astype(np.float32)
    special = np.asarray([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e38], dtype=np.float32)
    infs = np.where(rng.random(shape) < 0.3, rng.choice(special, size=shape), wide).astype(np.float32)
    out = {"ties": ties, "normal": wide, "inf": infs}
    nans = np.asarray([np.nan, -np.nan], dtype=np.float32)
    nans.view(np.uint32)[1] |= 0x80000000  # (a NaN with the sign bit set, whatever the line above gave)
    for frac in (0.1, 0.6):
        out[f"nan{frac}"] = np.where(rng.random(shape) < frac, rng.choice(nans, size=shape), infs).astype(np.float32)
    return out


@pytest.mark.parametrize("size", [3, 5])
@pytest.mark.parametrize("shape", MEDIAN_SHAPES, ids=_ids)
def test_map_median_equals_the_restatement(device, shape, size):
    from ddpm_ood_amd import ops

    for name, v in _median_inputs(shape).items():
        want = ref.median(v, size)
        got = ops.map_median(_dev(v, device), size)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        assert ref.same_values(got.cpu().numpy(), want), (name, shape, size)


@pytest.mark.parametrize("size", [3, 5])
def test_map_median_depends_on_nothing_but_the_image(device, size):
    """An image alone equals its row in a batch; the caller's ``out``, poisoned or all ones, is overwritten everywhere."""
    from ddpm_ood_amd import ops

    v = _median_inputs((5, 33, 31))["nan0.1"]
    want = ref.median(v, size)
    x = _dev(v, device)
    batch = ops.map_median(x, size)
    for n in (0, 2, 4):
        assert torch.equal(ops.map_median(x[n:n + 1].contiguous(), size).view(torch.int32), batch[n:n + 1].view(torch.int32))
    for fill in (POISON, 0x3F800000):
        out = torch.full((5, 33, 31), fill, dtype=torch.int32, device=device).view(torch.float32)
        assert ops.map_median(x, size, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(out.view(torch.int32), batch.view(torch.int32)) and ref.same_values(out.cpu().numpy(), want)


# ---- 2. segment -------------------------------------------------------------------------------------------------------------------

THRESHOLDS = [2.0, np.nan, 3.0, -np.inf, np.inf, 1e30, 2.5, -20.0]  # (NaN, +inf and 1e30 predict nothing, -inf and -20 everything finite)


def _values(m, seed):
    """fp32 maps whose {v > 2} is the mask ``m``: inside 2.25, 2.75 (gone at 2.5), 3.5 or +inf, outside 0.5, the threshold itself,
    -inf or NaN."""
    rng = np.random.default_rng(seed)
    return np.where(m != 0, rng.choice(np.asarray([2.25, 2.75, 3.5, np.inf], dtype=np.float32), size=m.shape),
                    rng.choice(np.asarray([0.5, 2.0, -np.inf, np.nan], dtype=np.float32), size=m.shape)).astype(np.float32)


def _truth(shape, seed):
    """Ground-truth masks of a few rectangles per image (image 0: none), with their labels."""
    N, H, W = shape
    rng = np.random.default_rng(seed)
    g = np.zeros(shape, dtype=np.uint8)
    for n in range(1, N):
        for _ in range(int(rng.integers(1, 4))):
            y, x = rng.integers(0, H), rng.integers(0, W)
            g[n, y:y + rng.integers(1, max(2, H // 2)), x:x + rng.integers(1, max(2, W // 2))] = 1
    return g


def _check(device, v, g, thresholds, min_size, conn, truth=None):
    """``truth``: (labels, regions) of ``g`` at ``conn``, for a caller that labels once."""
    from ddpm_ood_amd import ops

    labels, regions = truth if truth is not None else ref.label(g, conn)
    want = ref.segment(v, g, labels, regions, thresholds, min_size, conn)
    tv, tg, tl, tr = (_dev(a, device) for a in (v, g, labels, regions))
    got = ops.map_segment(tv, tg, tl, tr, thresholds, min_size, conn)
    N, H, W = v.shape
    K = len(thresholds)
    assert [tuple(t.shape) for t in got] == [(N, K, H, W), (N, K, 3), (N, K, 3), (N, K, 2)]
    assert [t.dtype for t in got] == [torch.uint8, torch.int32, torch.int32, torch.int32]
    for name, a, b in zip(("seg", "pixels", "components", "removed"), got, want):
        assert np.array_equal(a.cpu().numpy(), b), (name, v.shape, min_size, conn)
    if min_size == 1:  # the three existing ops, integer for integer
        assert torch.equal(got[1], ops.map_mask_counts(tv, tg, thresholds))
        assert torch.equal(got[2], ops.map_component_counts(tv, tg, tl, tr, thresholds, conn))
        assert not got[3].any()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got[0].cpu().numpy(), (v[:, None] > np.asarray(thresholds, dtype=np.float32)[None, :, None, None]))
    return want


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_map_segment_equals_the_restatement(device, shape, conn):
    """The named shapes and random densities of the labelling tests as {v > 2}, K = 3, min_size 1, 2, 5 and the whole plane."""
    N, H, W = shape
    g = _truth(shape, seed=H + W)
    truth = ref.label(g, conn)
    for name, m in _inputs(shape).items():
        v = _values(m, seed=H * W + conn)
        for min_size in (1, 2, 5, H * W):
            _check(device, v, g, [2.0, 2.5, 3.0], min_size, conn, truth)


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_map_segment_every_number_of_thresholds_and_the_largest_min_size(device, K):
    shape = (3, 33, 31)
    g = _truth(shape, seed=K)
    m = region_ref.random_masks(*shape, 0.5, seed=K)
    v = _values(m, seed=K)
    thr = THRESHOLDS[:K]
    want = _check(device, v, g, thr, 1, 8)
    if K >= 5:
        assert not want[0][:, [1, 4]].any() and want[0][:, 3].sum() == np.isfinite(v).sum() + (v == np.inf).sum()
    _check(device, v, g, thr, 3, 4)
    _check(device, v, g, thr, 16384, 8)
    thr_dev = torch.tensor(thr, dtype=torch.float32, device=device)  # a device tensor of thresholds: the same results
    from ddpm_ood_amd import ops

    labels, regions = ref.label(g, 8)
    a = ops.map_segment(_dev(v, device), _dev(g, device), _dev(labels, device), _dev(regions, device), thr_dev, 3, 8)
    b = ops.map_segment(_dev(v, device), _dev(g, device), _dev(labels, device), _dev(regions, device), thr, 3, 8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_map_segment_keeps_a_component_of_exactly_min_size(device):
    """Components of 1, 5, 6 and 7 pixels (an L of 6 whose corner joins only at connectivity 8): min_size at the exact size, one above."""
    v = np.zeros((1, 16, 16), dtype=np.float32)
    v[0, 1, 1] = 9.0
    v[0, 3, 2:7] = 9.0  # 5
    v[0, 6, 2:7] = v[0, 7, 7] = 9.0  # 5 + 1 through a corner
    v[0, 10, 2:9] = 9.0  # 7
    g = np.zeros((1, 16, 16), dtype=np.uint8)
    g[0, 10, :] = g[0, 1, 1] = 1
    for conn, sizes in ((8, [1, 5, 6, 7]), (4, [1, 5, 5, 1, 7])):
        for min_size in (1, 5, 6, 7, 8):
            seg, pixels, components, removed = _check(device, v, g, [2.0], min_size, conn)
            kept = [s for s in sizes if s >= min_size]
            assert components[0, 0, 1] == len(kept) and seg.sum() == sum(kept)
            assert list(removed[0, 0]) == [len(sizes) - len(kept), sum(sizes) - sum(kept)]


def test_map_segment_longest_chains_and_most_roots(device):
    """128 x 128: the checkerboard at connectivity 4 (8 192 components of one pixel), the all-ones plane (one size counter takes
    16 384 pixels) and the serpentine (one component of 8 256 pixels)."""
    H = W = 128
    g = _truth((1, H, W), seed=5)
    g[0, 40:60, 40:60] = 1
    for name, m in (("checkerboard", region_ref.checkerboard(H, W)), ("one", np.ones((H, W), dtype=np.uint8)),
                    ("serpentine", region_ref.serpentine(H, W))):
        v = np.where(m[None] != 0, 9.0, 0.0).astype(np.float32)
        for conn, min_size in ((4, 1), (4, 2), (8, 8192), (8, 16384)):
            seg, pixels, components, removed = _check(device, v, g, [2.0], min_size, conn)
            if name == "checkerboard" and conn == 4:
                assert components[0, 0, 1] + removed[0, 0, 0] == 8192 and removed[0, 0, 0] == (8192 if min_size == 2 else 0)
            if name == "one":
                assert components[0, 0, 1] == 1 and seg.all() and not removed.any()
            if name == "serpentine":
                assert int(m.sum()) == 8256 and list(removed[0, 0]) == ([1, 8256] if min_size == 16384 else [0, 0])


def test_map_segment_depends_on_nothing_but_the_image(device):
    """An image alone equals its rows in a batch; the entry point on poisoned and on all-ones outputs."""
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    shape = (4, 32, 32)
    g = _truth(shape, seed=2)
    v = _values(region_ref.random_masks(*shape, 0.55, seed=9), seed=9)
    labels, regions = ref.label(g, 8)
    want = ref.segment(v, g, labels, regions, [2.0, 3.0], 4, 8)
    tv, tg, tl, tr = (_dev(a, device) for a in (v, g, labels, regions))
    batch = ops.map_segment(tv, tg, tl, tr, [2.0, 3.0], 4, 8)
    for n in (0, 3):
        one = ops.map_segment(*(t[n:n + 1].contiguous() for t in (tv, tg, tl, tr)), [2.0, 3.0], 4, 8)
        assert all(torch.equal(a[0], b[n]) for a, b in zip(one, batch))
    thr = torch.tensor([2.0, 3.0], dtype=torch.float32, device=device)
    for fill in (POISON, -1):
        seg = torch.full((4, 2, 32, 32), fill & 0xFF, dtype=torch.uint8, device=device)
        ints = [torch.full((4, 2, w), fill, dtype=torch.int32, device=device) for w in (3, 3, 2)]
        assert lib.ddpm_map_segment_f32(tv.data_ptr(), tg.data_ptr(), tl.data_ptr(), tr.data_ptr(), 4, 32, 32, thr.data_ptr(), 2, 4, 8,
                                        seg.data_ptr(), *(t.data_ptr() for t in ints), _lib.stream_ptr()) == 0
        for a, b in zip([seg] + ints, want):
            assert np.array_equal(a.cpu().numpy(), b)


def test_what_the_two_ops_refuse(device):
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    v = torch.zeros((1, 8, 8), dtype=torch.float32, device=device)
    for size in (1, 4, 7, 0, -3, 3.5, None, True):
        with pytest.raises(ValueError, match="size must be 3 or 5"):
            ops.map_median(v, size)
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        ops.map_median(v[0], 3)
    with pytest.raises(ValueError, match="out must be"):
        ops.map_median(v, 3, out=torch.zeros((1, 8, 9), dtype=torch.float32, device=device))
    out = torch.zeros((1, 8, 8), dtype=torch.float32, device=device)
    assert lib.ddpm_map_median_f32(v.data_ptr(), out.data_ptr(), 4, 1, 8, 8, _lib.stream_ptr()) == -1 and b"size" in lib.ddpm_last_error()
    assert lib.ddpm_map_median_f32(v.data_ptr(), v.data_ptr(), 3, 1, 8, 8, _lib.stream_ptr()) == -1 and b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_median_f32(v.data_ptr(), v.data_ptr() + 128, 3, 1, 8, 8, _lib.stream_ptr()) == -1 and b"alias" in lib.ddpm_last_error()
    m = torch.zeros((1, 8, 8), dtype=torch.uint8, device=device)
    labels, regions = ops.map_label(m, 8)
    for bad in (0, -1, 16385, 2.5, None, True):
        with pytest.raises(ValueError, match="min_size"):
            ops.map_segment(v, m, labels, regions, [2.0], bad)
    with pytest.raises(ValueError, match="connectivity"):
        ops.map_segment(v, m, labels, regions, [2.0], 4, connectivity=6)
    with pytest.raises(ValueError, match="1 .. 8 thresholds"):
        ops.map_segment(v, m, labels, regions, [1.0] * 9, 4)
    with pytest.raises(ValueError, match="1 .. 8 thresholds"):
        ops.map_segment(v, m, labels, regions, [], 4)
    with pytest.raises(ValueError, match="regions"):
        ops.map_segment(v, m, labels, regions[:0], [2.0], 4)
    big_v, big_m = torch.zeros((1, 129, 128), dtype=torch.float32, device=device), torch.zeros((1, 129, 128), dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match="128 x 128"):
        ops.map_segment(big_v, big_m, torch.zeros((1, 129, 128), dtype=torch.int32, device=device), regions, [2.0], 4)
    thr = torch.zeros((1,), dtype=torch.float32, device=device)
    seg = torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device=device)
    ints = [torch.zeros((1, 1, w), dtype=torch.int32, device=device) for w in (3, 3, 2)]

    def call(min_size=4, conn=8, seg_ptr=seg.data_ptr(), pixels_ptr=ints[0].data_ptr()):
        return lib.ddpm_map_segment_f32(v.data_ptr(), m.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 8, 8, thr.data_ptr(), 1,
                                        min_size, conn, seg_ptr, pixels_ptr, ints[1].data_ptr(), ints[2].data_ptr(), _lib.stream_ptr())

    assert call() == 0
    assert call(min_size=0) == -1 and b"min_size" in lib.ddpm_last_error()
    assert call(min_size=16385) == -1 and b"min_size" in lib.ddpm_last_error()
    assert call(conn=6) == -1 and b"connectivity" in lib.ddpm_last_error()
    assert call(seg_ptr=m.data_ptr()) == -1 and b"alias" in lib.ddpm_last_error()  # the segmentation over the mask
    assert call(pixels_ptr=ints[1].data_ptr() + 4) == -1 and b"alias" in lib.ddpm_last_error()  # two outputs over each other


# ---- 3. through the trainer -------------------------------------------------------------------------------------------------------
# The sets of test_gpu_region_metrics.py: 8 / 8 / 8 + 8 synthetic 32 x 32 images in batches of 4, the t-starts 10 and 30.

KEYS = ("z_lpips_map", "z_mse_map")
SEGMENT_KEYS = ["filename", "t", "channels", "thresholds", "fpr", "median", "min_component", "connectivity", "sigma", "segmentation", "pixels",
                "components", "removed", "mask_pixels", "regions"]
SEG = ("--pixel_segment", "1")


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic

    root = tmp_path_factory.mktemp("segment")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    np.savez(root / "mul_masks.npz", masks=_hand_masks())
    flags = (*_flags(root), "--pixel_regions", "1", "--pixel_calibrate_fpr", "0.05,0.01")
    return root, _run(root, "off", *flags), _run(root, "on", *flags, *SEG)


def _check_file(path, zfile, masks, median=3, min_component=4, conn=8, thresholds=(2.0, 3.0, 4.0), calibration=None, sigma=0.0):
    """segments_<name>.npz against the restatement applied to the written Z-maps and the masks: every integer and every pixel."""
    sg, z = np.load(path), np.load(zfile)
    assert sorted(sg.files) == sorted(SEGMENT_KEYS)
    N, K = len(masks), len(thresholds)
    thr = np.repeat(np.asarray(thresholds, dtype=np.float32)[None], 2, axis=0)
    fpr = np.full(K, np.nan)
    if calibration is not None:
        thr = np.concatenate([thr, calibration["thresholds"].astype(np.float32)], axis=1)
        fpr = np.concatenate([fpr, calibration["fpr"]])
    T = thr.shape[1]
    assert sg["thresholds"].dtype == np.float32 and np.array_equal(sg["thresholds"], thr)
    assert sg["fpr"].dtype == np.float64 and np.array_equal(sg["fpr"], fpr, equal_nan=True)
    assert (int(sg["median"]), int(sg["min_component"]), int(sg["connectivity"]), float(sg["sigma"])) == (median, min_component, conn, sigma)
    assert sg["segmentation"].dtype == np.uint8 and sg["segmentation"].shape == (N, 2, T) + masks.shape[1:]
    assert all(sg[k].dtype == np.int32 for k in ("pixels", "components", "removed", "regions"))
    assert sg["pixels"].shape == (N, 2, T, 3) and sg["components"].shape == (N, 2, T, 3) and sg["removed"].shape == (N, 2, T, 2)
    labels, regions = ref.label(masks, conn)
    assert np.array_equal(sg["regions"], regions) and np.array_equal(sg["mask_pixels"], (masks != 0).reshape(N, -1).sum(axis=1))
    for c, key in enumerate(KEYS):
        zc = z[key] if median == 1 else ref.median(z[key], median)
        want = ref.segment(zc, masks, labels, regions, thr[c], min_component, conn)
        for name, w in zip(("segmentation", "pixels", "components", "removed"), want):
            assert np.array_equal(sg[name][:, c], w), (path.name, key, name)
    assert [str(s) for s in sg["filename"]] == [str(s) for s in z["filename"]] and list(sg["channels"]) == ["lpips", "mse"]
    assert list(sg["t"]) == list(z["t"])
    return sg


def test_segments_file_equals_the_restatement_on_the_written_z_maps(runs):
    root, off, on = runs
    cal = np.load(on / "calibration.npz")
    les = _check_file(on / "segments_LES.npz", on / "zmaps_LES.npz", _masks_of("LES"), calibration=cal)
    assert list(les["t"]) == [10, 30] and les["segmentation"].any()
    _check_file(on / "segments_MUL.npz", on / "zmaps_MUL.npz", _masks_of("MUL"), calibration=cal)
    sin = _check_file(on / "segments_in.npz", on / "zmaps_in.npz", _masks_of("in"), calibration=cal)  # no masks: every kept pixel a false one
    assert not sin["pixels"][..., [0, 2]].any() and np.array_equal(sin["pixels"][..., 1], sin["segmentation"].reshape(8, 2, 5, -1).sum(axis=3))


def test_nothing_else_moves(runs):
    root, off, on = runs
    names = sorted(p.name for p in off.iterdir())
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["segments_LES.npz", "segments_MUL.npz", "segments_in.npz"])
    assert {"calibration.npz", "calibrated_LES.npz", "regions_MUL.npz", "pixels_in.npz", "zmaps_in.npz", "map_stats.npz"} <= set(names)
    for n in names:
        if n.endswith(".csv"):
            assert (off / n).read_bytes() == (on / n).read_bytes(), n
        else:  # (an archive carries its members' time stamps: the members are compared, bit for bit)
            a, b = np.load(off / n), np.load(on / n)
            assert a.files == b.files
            for key in a.files:
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (n, key)


def test_two_batches_equal_one_and_other_settings(runs):
    root, off, on = runs
    _with_stats_of(root, on)
    shutil.copy(on / "calibration.npz", root / MODEL / "ood" / "calibration.npz")
    flags = (*_flags(root), "--pixel_regions", "1", "--pixel_calibrate_fpr", "0.05,0.01", *SEG)
    one = _run(root, "sg8", *flags, "--batch_size", "8", "--run_val", "0", "--run_in", "0")
    for name in ("LES", "MUL"):
        a, b = np.load(on / f"segments_{name}.npz"), np.load(one / f"segments_{name}.npz")
        for key in SEGMENT_KEYS:
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
    # no median, connectivity 4, another minimum size and smoothing, one threshold, no calibration
    _with_stats_of(root, on)
    other = _run(root, "sg_other", *_flags(root), *SEG, "--run_val", "0", "--run_in", "0", "--pixel_median", "1", "--pixel_min_component", "2",
                 "--pixel_thresholds", "1.5", "--anomaly_z_sigma", "1.5", "--pixel_connectivity", "4")
    _check_file(other / "segments_MUL.npz", other / "zmaps_MUL.npz", _masks_of("MUL"), median=1, min_component=2, conn=4, thresholds=(1.5,),
                sigma=1.5)
    _with_stats_of(root, on)
    five = _run(root, "sg_five", *_flags(root), *SEG, "--run_val", "0", "--run_in", "0", "--pixel_median", "5", "--pixel_min_component", "1")
    sg = _check_file(five / "segments_LES.npz", five / "zmaps_LES.npz", _masks_of("LES"), median=5, min_component=1)
    assert not sg["removed"].any()


def test_without_pixel_metrics_the_masks_are_all_zero(runs):
    """The deployment case: no ground truth, no --pixel_metrics; the out sets are segmented against all-zero masks."""
    root, off, on = runs
    _with_stats_of(root, on)
    plain = _run(root, "sg_plain", "--anomaly_z_maps", "1", *SEG, "--run_val", "0")
    assert sorted(p.name for p in plain.iterdir()) == sorted(
        ["map_stats.npz"] + [f"{kind}_{o}.{ext}" for o in ("in", "LES", "MUL") for kind, ext in (("results", "csv"), ("zmaps", "npz"),
                                                                                                ("segments", "npz"))])
    for name in ("in", "LES", "MUL"):
        sg = _check_file(plain / f"segments_{name}.npz", plain / f"zmaps_{name}.npz", np.zeros((8, 32, 32), dtype=np.uint8))
        assert not sg["pixels"][..., [0, 2]].any() and not sg["mask_pixels"].any() and not sg["regions"].any()
        assert np.array_equal(np.load(plain / f"zmaps_{name}.npz")["z_mse_map"], np.load(on / f"zmaps_{name}.npz")["z_mse_map"])
    # and with the masks: the same segmentations
    assert np.array_equal(np.load(plain / "segments_LES.npz")["segmentation"], np.load(on / "segments_LES.npz")["segmentation"][:, :, :3])


def test_what_the_constructor_refuses(runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root = runs[0]
    for extra, text in ((("--pixel_segment", "1"), "--anomaly_z_maps 1"),
                        (("--anomaly_z_maps", "1", *SEG, "--pixel_median", "4"), "--pixel_median"),
                        (("--anomaly_z_maps", "1", *SEG, "--pixel_min_component", "0"), "--pixel_min_component"),
                        (("--anomaly_z_maps", "1", *SEG, "--pixel_min_component", "16385"), "--pixel_min_component")):
        with pytest.raises(ValueError, match=text):
            Reconstruct(cli.parse_args(_argv(root, *extra)))


def test_command_line_prints_the_segment_scores(runs):
    from ddpm_ood_amd import ood

    root, off, on = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL, "--out_data",
                              "LES,MUL", "--score", "pixel", "--pixel_segmented", "1"], capture_output=True, text=True, check=True).stdout
        assert f"Pixel AUC for {MODEL} vs LES" in got
        for name in ("LES", "MUL"):
            rows = ood.score_segments(on / f"segments_{name}.npz", on / "segments_in.npz")
            assert len(rows) == 5 and f"Segmentations for {MODEL} vs {name}: median 3, components below 4 pixels removed" in got
            for r in rows:
                assert 0.0 <= r["mean_dice"] <= 1.0 and 0.0 <= r["in_fpr"] <= 1.0
                assert (f"mean image Dice {r['mean_dice']:.4f}, pooled Dice {r['pooled_dice']:.4f}, recall {r['region_recall']:.4f}, "
                        f"component precision {r['component_precision']:.4f}, F1 {r['component_f1']:.4f}, in-set FPR {r['in_fpr']:.5f}, "
                        f"removed {r['removed_components']} components / {r['removed_pixels']} pixels") in got
            assert "(validation FPR <= 0.05)" in got and "(validation FPR <= 0.01)" in got
        (root / MODEL / "ood" / "segments_in.npz").unlink()
        with pytest.raises(FileNotFoundError, match="--pixel_segment 1"):
            ood.print_segments(MODEL, "LES", root / MODEL / "ood", "z_mse_map")
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_on_one_gpu_reproduce_the_single_rank_file(device, runs):
    """reconstruct.py --pixel_segment 1 as two ranks (gloo rendezvous, both on cuda:0) on the single-rank run's map_stats.npz: the
    Z-maps are the single-rank run's bits, so every image's segmentation and integers are too, rows rank-major (0 2 4 6, 1 3 5 7) as
    in the CSV.  t = 10 alone (--inference_skip_factor 99)."""
    from test_gpu_dist import _launch_ranks

    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, off, on = runs
    flags = (*_flags(root), *SEG)
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    args = cli.parse_args(_argv(root, *flags, "--run_in", "0", "--inference_skip_factor", "99"))
    Reconstruct(args).reconstruct(args)  # one rank: validation (the statistics at t = 10) and the out sets
    single = root / MODEL / "ood_single_t10"
    shutil.copytree(root / MODEL / "ood", single)
    for p in (root / MODEL / "ood").iterdir():
        if p.name != "map_stats.npz":
            p.unlink()
    try:
        _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *flags, "--run_val", "0", "--run_in", "0", "--inference_skip_factor", "99")],
                      root, timeout=600)
        out = root / MODEL / "ood"
        order = [0, 2, 4, 6, 1, 3, 5, 7]
        for name in ("LES", "MUL"):
            one, two = np.load(single / f"segments_{name}.npz"), np.load(out / f"segments_{name}.npz")
            names = [str(s) for s in one["filename"]]
            assert [str(s) for s in two["filename"]] == [names[i] for i in order] and list(two["t"]) == [10]
            for key in ("segmentation", "pixels", "components", "removed", "mask_pixels", "regions"):
                assert two[key].dtype == one[key].dtype and np.array_equal(two[key], one[key][order]), (name, key)
            for key in ("thresholds", "fpr", "median", "min_component", "connectivity", "sigma", "channels"):
                assert np.array_equal(one[key], two[key], equal_nan=key == "fpr"), key
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
