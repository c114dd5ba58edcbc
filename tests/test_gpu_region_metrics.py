"""GPU: the kernels of csrc/regions.hip against the numpy restatement of tests/region_ref.py (labels and counts exactly, the
overlap table to the rounding of its R_total terms), and --pixel_regions 1 through the trainer, the command line and two ranks
(DESIGN 3.24)."""

import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pixel_ref
import region_ref as ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# one pixel; one row; one column; odd sizes below one pixel per thread; exactly one pixel per thread; more, odd; 4 and 16 pixels per
# thread (the largest plane)
SHAPES = [(1, 1, 1), (2, 1, 9), (2, 9, 1), (3, 5, 7), (4, 32, 32), (2, 33, 31), (1, 64, 64), (1, 128, 128)]
LO, HI = -16.0, 48.0
POISON = 0x7FC0DEAD


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _inputs(shape):
    """name -> uint8 [N, H, W]: the named shapes (image n of a batch transposed / flipped so that the images differ) and random
    masks at three densities."""
    N, H, W = shape
    out = {}
    for name, m in ref.named_shapes(H, W).items():
        out[name] = np.stack([m if n % 2 == 0 else m[::-1, ::-1] for n in range(N)])
    for d in (0.3, 0.5, 0.6):
        out[f"random{d}"] = ref.random_masks(N, H, W, d, seed=int(d * 10) + H * W)
    return out


@pytest.fixture(scope="module")
def label_cases():
    """(shape, name, connectivity) -> (mask, labels, regions) of the restatement, computed once."""
    out = {}
    for shape in SHAPES:
        for name, m in _inputs(shape).items():
            for conn in (4, 8):
                out[shape, name, conn] = (m,) + ref.label(m, conn)
    return out


# ---- 1. labelling -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_label_equals_the_restatement(device, label_cases, shape, conn):
    """Both predicates, every named shape and density, into the wrapper's uninitialised outputs."""
    from ddpm_ood_amd import ops

    N, H, W = shape
    for name in _inputs(shape):
        m, want_l, want_r = label_cases[shape, name, conn]
        labels, regions = ops.map_label(_dev(m, device), conn)
        assert labels.dtype == torch.int32 and regions.dtype == torch.int32 and labels.shape == (N, H, W) and regions.shape == (N,)
        assert np.array_equal(regions.cpu().numpy(), want_r), (name, regions.cpu().numpy(), want_r)
        assert np.array_equal(labels.cpu().numpy(), want_l), name
        # the fp32 predicate v > thr: inside 1.5 or +inf, outside 0.5, the threshold itself, -inf or NaN
        rng = np.random.default_rng(H * W + conn)
        v = np.where(m != 0, rng.choice(np.asarray([1.5, np.inf], dtype=np.float32), size=m.shape),
                     rng.choice(np.asarray([0.5, 1.0, -np.inf, np.nan], dtype=np.float32), size=m.shape)).astype(np.float32)
        labels, regions = ops.map_label(_dev(v, device), conn, threshold=1.0)
        assert np.array_equal(regions.cpu().numpy(), want_r) and np.array_equal(labels.cpu().numpy(), want_l), name
    if H * W > 1:  # the known counts of the named shapes
        assert label_cases[shape, "checkerboard", 4][2][0] == (H * W + 1) // 2
        assert label_cases[shape, "checkerboard", 8][2][0] == (1 if min(H, W) > 1 else (H * W + 1) // 2)
        assert label_cases[shape, "one", conn][2][0] == 1 and label_cases[shape, "zero", conn][2][0] == 0
    if min(H, W) >= 5:
        assert label_cases[shape, "serpentine", conn][2][0] == 1 and label_cases[shape, "comb", conn][2][0] == 1
        assert label_cases[shape, "diagonals", 4][2][0] > label_cases[shape, "diagonals", 8][2][0]


def test_map_label_depends_on_nothing_but_the_image(device, label_cases):
    """An image labelled alone equals its rows in a batch, whatever the output buffers held (the entry point on poisoned and on
    all-ones buffers)."""
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    shape = (4, 32, 32)
    m, want_l, want_r = label_cases[shape, "random0.6", 8]
    batch = np.concatenate([m, label_cases[shape, "serpentine", 8][0], label_cases[shape, "random0.5", 8][0]])
    lb, rb = ops.map_label(_dev(batch, device), 8)
    for n in (0, 3, 5, 11):
        l1, r1 = ops.map_label(_dev(batch[n:n + 1], device), 8)
        assert torch.equal(l1[0], lb[n]) and int(r1[0]) == int(rb[n])
    assert np.array_equal(lb[:4].cpu().numpy(), want_l)
    x = _dev(m, device)
    for fill in (POISON, -1):
        labels = torch.full((4, 32, 32), fill, dtype=torch.int32, device=device)
        regions = torch.full((4,), fill, dtype=torch.int32, device=device)
        assert lib.ddpm_map_label_u8(x.data_ptr(), 4, 32, 32, 8, labels.data_ptr(), regions.data_ptr(), _lib.stream_ptr()) == 0
        assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(regions.cpu().numpy(), want_r)


# ---- 2. region overlap ------------------------------------------------------------------------------------------------------------

def _overlap_case(N, H, W, nbins, seed):
    """Maps that visit every branch of the bin rule (pixel_ref.case_values) against a few blobs per image."""
    v, _ = pixel_ref.case_values(N, H * W, LO, HI, nbins, seed=seed)
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        for _ in range(max(int(rng.integers(0, 5)), 1 if n == N - 1 else 0)):  # (some images without a region, never all)
            y, x, h, w = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, H // 3)), rng.integers(1, max(2, W // 3))
            m[n, y:y + h, x:x + w] = 1
    return v.reshape(N, H, W), m


@pytest.mark.parametrize("nbins", [2, 4096, 8191])
@pytest.mark.parametrize("shape", [(3, 5, 7), (6, 32, 32), (2, 33, 31), (1, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_map_region_overlap_equals_the_restatement(device, shape, nbins):
    from ddpm_ood_amd import ops

    N, H, W = shape
    v, m = _overlap_case(N, H, W, nbins, seed=H + nbins)
    labels, regions = ref.label(m, 8)
    R = int(regions.sum())
    want = ref.overlap(v, labels, regions, LO, HI, nbins)
    tv, tl, tr = _dev(v, device), _dev(labels, device), _dev(regions, device)
    got = ops.map_region_overlap(tv, tl, tr, LO, HI, nbins)
    assert got.dtype == torch.float64 and got.shape == (nbins + 1,)
    g = got.cpu().numpy()
    err = np.abs(g - want)
    print(f"overlap {shape} nbins {nbins}: R_total {R}, largest error {err.max():.3e}, bound {ref.overlap_bound(want, R).min():.3e}")
    assert (err <= ref.overlap_bound(want, R)).all()
    assert abs(g.sum() - R) <= (R + 1) * (nbins + 1) * 2.0 ** -52 * max(1, R)  # every region's fractions sum to one
    again = ops.map_region_overlap(tv, tl, tr, LO, HI, nbins)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))  # repeated launches: the same bits
    # two accumulating half-batches: the bits of one batch
    if N >= 2:
        h = N // 2
        total = ops.map_region_overlap(tv[:h].contiguous(), tl[:h].contiguous(), tr[:h].contiguous(), LO, HI, nbins)
        out = ops.map_region_overlap(tv[h:].contiguous(), tl[h:].contiguous(), tr[h:].contiguous(), LO, HI, nbins, total=total)
        assert out.data_ptr() == total.data_ptr() and torch.equal(out.view(torch.int64), got.view(torch.int64))


def test_map_region_overlap_nan_column_range_ends_and_checkerboard(device):
    from ddpm_ood_amd import ops

    # one region of four pixels: NaN, below the range, above it (+inf), inside
    m = np.zeros((1, 4, 4), dtype=np.uint8)
    m[0, 1, :] = 1
    v = np.zeros((1, 4, 4), dtype=np.float32)
    v[0, 1] = [np.nan, -100.0, np.inf, 0.0]
    v[0, 0, 0] = np.nan  # (a NaN outside every region counts nowhere)
    labels, regions = ops.map_label(_dev(m, device), 8)
    got = ops.map_region_overlap(_dev(v, device), labels, regions, LO, HI, 64).cpu().numpy()
    want = np.zeros(65)
    want[64] = want[0] = want[63] = want[16] = 0.25
    assert np.array_equal(got, want)
    # a 16 x 16 checkerboard at connectivity 4: 128 regions of area 1, every one in the bin of its own pixel
    cb = ref.checkerboard(16, 16)[None]
    labels, regions = ops.map_label(_dev(cb, device), 4)
    assert int(regions[0]) == 128
    v = (LO + (HI - LO) * np.random.default_rng(3).random((1, 16, 16))).astype(np.float32)
    got = ops.map_region_overlap(_dev(v, device), labels, regions, LO, HI, 4096).cpu().numpy()
    assert np.array_equal(got, np.bincount(pixel_ref.bin_index(v[cb != 0], LO, HI, 4096), minlength=4097).astype(np.float64))
    assert np.array_equal(got, ref.overlap(v, labels.cpu().numpy(), regions.cpu().numpy(), LO, HI, 4096))


# ---- 3. component counts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_map_component_counts_equal_the_restatement(device, K, conn):
    from ddpm_ood_amd import ops

    thresholds = [2.0, np.nan, 3.0, -20.0, 1e30, 0.5, 2.5, 4.0][:K] if K > 1 else [2.0]
    for N, H, W in [(3, 5, 7), (5, 32, 32), (2, 33, 31), (2, 128, 128)]:
        v, m = _overlap_case(N, H, W, 64, seed=H + K)
        v = (v / 8).astype(np.float32)  # (many components at the thresholds 2 .. 4)
        m[0] = 0  # an image with an empty mask
        if H >= 32:
            m[1], v[1] = 0, 0.0
            m[1, 4:8, 4:8] = 1
            m[1, 4:8, 12:16] = 1
            v[1, 5, 5:14] = 9.0  # one predicted component touching two regions
            m[1, 20:28, 4:12] = 1
            v[1, 21, 5] = v[1, 26, 10] = 9.0  # one region touched by two components
            v[1, 30, 30] = 9.0  # and a false one
        labels, regions = ref.label(m, conn)
        want = ref.component_counts(v, m, labels, regions, thresholds, conn)
        got = ops.map_component_counts(_dev(v, device), _dev(m, device), _dev(labels, device), _dev(regions, device), thresholds, conn)
        assert got.dtype == torch.int32 and got.shape == (N, K, 3)
        assert np.array_equal(got.cpu().numpy(), want), (N, H, W)
        if H >= 32:
            assert list(want[1, 0]) == [3, 4, 1]
        if K > 1:
            assert (want[:, 1] == 0).all()  # a NaN threshold predicts nothing


def test_what_the_three_ops_refuse(device):
    from ddpm_ood_amd import _lib, ops

    lib = _lib.load()
    m = torch.zeros((1, 129, 128), dtype=torch.uint8, device=device)
    v = torch.zeros((1, 129, 128), dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match="128 x 128"):
        ops.map_label(m, 8)
    with pytest.raises(ValueError, match="128 x 128"):
        ops.map_label(v, 8, threshold=0.0)
    labels = torch.zeros((1, 129, 128), dtype=torch.int32, device=device)
    regions = torch.zeros((1,), dtype=torch.int32, device=device)
    for rc in (lib.ddpm_map_label_u8(m.data_ptr(), 1, 129, 128, 8, labels.data_ptr(), regions.data_ptr(), _lib.stream_ptr()),
               lib.ddpm_map_label_f32(v.data_ptr(), 0.0, 1, 129, 128, 8, labels.data_ptr(), regions.data_ptr(), _lib.stream_ptr())):
        assert rc == -1 and b"map_label" in lib.ddpm_last_error() and b"129 x 128" in lib.ddpm_last_error()
    total = torch.zeros((65,), dtype=torch.float64, device=device)
    scratch = torch.zeros((1, 65), dtype=torch.float64, device=device)
    assert lib.ddpm_map_region_overlap_f32(v.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 129 * 128, LO, 1.0, 64,
                                           scratch.data_ptr(), total.data_ptr(), 0, _lib.stream_ptr()) == -1
    assert b"map_region_overlap" in lib.ddpm_last_error()
    with pytest.raises(ValueError, match="128 x 128"):
        ops.map_region_overlap(v, labels, regions, LO, HI, 64)
    with pytest.raises(ValueError, match="128 x 128"):
        ops.map_component_counts(v, m, labels, regions, [2.0])
    m, v, labels = m[:, :8, :8].contiguous(), v[:, :8, :8].contiguous(), labels[:, :8, :8].contiguous()
    with pytest.raises(ValueError, match="1 .. 8 thresholds"):
        ops.map_component_counts(v, m, labels, regions, [1.0] * 9)
    thr = torch.zeros((9,), dtype=torch.float32, device=device)
    counts = torch.zeros((1, 9, 3), dtype=torch.int32, device=device)
    assert lib.ddpm_map_component_counts_f32(v.data_ptr(), m.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 8, 8, thr.data_ptr(),
                                             9, 8, counts.data_ptr(), _lib.stream_ptr()) == -1
    assert b"map_component_counts" in lib.ddpm_last_error() and b"K" in lib.ddpm_last_error()
    for call in (lambda: ops.map_label(m, 6), lambda: ops.map_label(v, 6, threshold=0.0),
                 lambda: ops.map_component_counts(v, m, labels, regions, [2.0], connectivity=6)):
        with pytest.raises(ValueError, match="connectivity"):
            call()
    assert lib.ddpm_map_label_u8(m.data_ptr(), 1, 8, 8, 6, labels.data_ptr(), regions.data_ptr(), _lib.stream_ptr()) == -1
    assert b"connectivity" in lib.ddpm_last_error()
    assert lib.ddpm_map_component_counts_f32(v.data_ptr(), m.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 8, 8, thr.data_ptr(),
                                             1, 6, counts.data_ptr(), _lib.stream_ptr()) == -1
    # overlapping outputs: labels inside the maps it is computed from, total inside scratch, counts inside the labels
    assert lib.ddpm_map_label_f32(v.data_ptr(), 0.0, 1, 8, 8, 8, v.data_ptr(), regions.data_ptr(), _lib.stream_ptr()) == -1
    assert b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_label_u8(m.data_ptr(), 1, 8, 8, 8, labels.data_ptr(), labels.data_ptr() + 16, _lib.stream_ptr()) == -1
    assert lib.ddpm_map_region_overlap_f32(v.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 64, LO, 1.0, 64, scratch.data_ptr(),
                                           scratch.data_ptr() + 64, 0, _lib.stream_ptr()) == -1
    assert b"map_region_overlap" in lib.ddpm_last_error() and b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_component_counts_f32(v.data_ptr(), m.data_ptr(), labels.data_ptr(), regions.data_ptr(), 1, 8, 8, thr.data_ptr(),
                                             1, 8, labels.data_ptr() + 32, _lib.stream_ptr()) == -1
    assert b"map_component_counts" in lib.ddpm_last_error() and b"alias" in lib.ddpm_last_error()
    # wrong dtypes, shapes and strides never reach the library
    with pytest.raises(ValueError, match="contiguous"):
        ops.map_label(m.to(torch.int32), 8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.map_label(torch.zeros((1, 8, 16), dtype=torch.uint8, device=device)[:, :, ::2], 8)
    with pytest.raises(ValueError, match=r"\[N, H, W\]"):
        ops.map_label(m[0], 8)
    with pytest.raises(ValueError, match="labels"):
        ops.map_region_overlap(v, labels.to(torch.int64), regions, LO, HI, 64)
    with pytest.raises(ValueError, match="regions"):
        ops.map_component_counts(v, m, labels, regions[:0], [2.0])
    with pytest.raises(ValueError, match="total"):
        ops.map_region_overlap(v, labels, regions, LO, HI, 64, total=torch.zeros((65,), dtype=torch.float32, device=device))


# ---- 4. through the trainer -------------------------------------------------------------------------------------------------------
# 8 / 8 / 8 + 8 synthetic 32 x 32 images in batches of 4, the t-starts 10 and 30 only.  LES: lesions with their own (auto) masks,
# one disc each; MUL: blobs against hand-made masks of several regions from an .npz.

MODEL = "fashionmnist_pixels"
SETS = {"val": "synthetic:blobs:n=8:seed=10", "in": "synthetic:blobs:n=8:seed=11",
        "out": "synthetic:lesion:n=8:mix=25:name=LES,synthetic:blobs:n=8:seed=12:name=MUL"}
KEYS = ("z_lpips_map", "z_mse_map")
REGION_KEYS = ["filename", "t", "channels", "lo", "hi", "nbins", "connectivity", "regions", "overlap", "thresholds", "components", "sigma"]


def _hand_masks():
    m = np.zeros((8, 32, 32), dtype=np.uint8)  # image 0: no region
    m[1, 2:8, 2:8] = m[1, 20:30, 12:28] = 1  # two squares, one larger
    m[2, 4:10, 4:10] = m[2, 10:16, 10:16] = 1  # two squares that touch at a corner: one region at 8, two at 4
    m[3, 8:24, 8:24], m[3, 12:20, 12:20] = 1, 0  # a ring
    m[3, 15:17, 15:17] = 1  # and an island inside it
    m[4] = ref.random_masks(1, 32, 32, 0.05, seed=4)[0]  # many single pixels
    m[5, :, 0] = m[5, 31, :] = m[5, 0, 31] = 1  # along the border
    m[6, 3, 3] = m[6, 28, 28] = m[6, 3, 28] = 1
    m[7, 10:22, 10:22] = 1
    return m


def _flags(root):
    return ("--anomaly_z_maps", "1", "--pixel_metrics", "1", "--out_masks", f"auto,{root / 'mul_masks.npz'}")


def _argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1", "--validation_ids", SETS["val"],
            "--in_ids", SETS["in"], "--out_ids", SETS["out"], "--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015",
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

    root = tmp_path_factory.mktemp("region_metrics")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    np.savez(root / "mul_masks.npz", masks=_hand_masks())
    return root, _run(root, "px", *_flags(root)), _run(root, "rg", *_flags(root), "--pixel_regions", "1")


def _masks_of(name):
    from ddpm_ood_amd import data

    if name == "LES":
        return data.synthetic_masks("lesion", 8, 1, 32, seed=0, mix=25).numpy().reshape(8, 32, 32)
    return _hand_masks() if name == "MUL" else np.zeros((8, 32, 32), dtype=np.uint8)


def _with_stats_of(root, src):
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    (root / MODEL / "ood").mkdir()
    shutil.copy(src / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")


def _check_file(path, zfile, masks, conn=8, bins=4096, value_range=(LO, HI), thresholds=(2.0, 3.0, 4.0)):
    """regions_<name>.npz against region_ref applied to the written Z-maps and the masks: integers exactly, the overlap to the bound."""
    rg, z = np.load(path), np.load(zfile)
    assert sorted(rg.files) == sorted(REGION_KEYS)
    labels, regions = ref.label(masks, conn)
    R = int(regions.sum())
    assert rg["regions"].dtype == np.int32 and rg["components"].dtype == np.int32 and rg["overlap"].dtype == np.float64
    assert np.array_equal(rg["regions"], regions) and int(rg["connectivity"]) == conn
    assert rg["overlap"].shape == (2, bins + 1) and rg["components"].shape == (len(masks), 2, len(thresholds), 3)
    for c, key in enumerate(KEYS):
        want = ref.overlap(z[key], labels, regions, *value_range, bins)
        err = np.abs(rg["overlap"][c] - want)
        print(f"{path.name} {key}: R_total {R}, largest overlap error {err.max():.3e}")
        assert (err <= ref.overlap_bound(want, R)).all()
        assert np.array_equal(rg["components"][:, c], ref.component_counts(z[key], masks, labels, regions, thresholds, conn)), key
    assert [str(s) for s in rg["filename"]] == [str(s) for s in z["filename"]] and list(rg["channels"]) == ["lpips", "mse"]
    assert np.array_equal(rg["thresholds"], np.asarray(thresholds, dtype=np.float32))
    return rg


def test_regions_file_equals_the_restatement_on_the_written_z_maps(runs):
    root, off, on = runs
    les = _check_file(on / "regions_LES.npz", on / "zmaps_LES.npz", _masks_of("LES"))
    assert list(les["regions"]) == [1] * 8 and list(les["t"]) == [10, 30]
    assert (float(les["lo"]), float(les["hi"]), int(les["nbins"]), float(les["sigma"])) == (LO, HI, 4096, 0.0)
    mul = _check_file(on / "regions_MUL.npz", on / "zmaps_MUL.npz", _masks_of("MUL"))
    assert list(mul["regions"][:4]) == [0, 2, 1, 2] and mul["regions"][4] > 5 and list(mul["regions"][5:]) == [2, 3, 1]
    rin = _check_file(on / "regions_in.npz", on / "zmaps_in.npz", _masks_of("in"))  # no masks: no region
    assert not rin["regions"].any() and not rin["overlap"].any() and not rin["components"][..., 0].any()
    assert np.array_equal(rin["components"][..., 1], rin["components"][..., 2])  # every predicted component is a false one


def test_nothing_else_moves(runs):
    root, off, on = runs
    names = sorted(p.name for p in off.iterdir())
    assert names == sorted(["map_stats.npz", "results_val.csv", "results_in.csv", "zmaps_in.npz", "pixels_in.npz"]
                           + [f"{kind}_{o}.{ext}" for o in ("LES", "MUL") for kind, ext in (("results", "csv"), ("zmaps", "npz"), ("pixels", "npz"))])
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["regions_LES.npz", "regions_MUL.npz", "regions_in.npz"])
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
    one = _run(root, "rg8", *_flags(root), "--pixel_regions", "1", "--batch_size", "8", "--run_val", "0", "--run_in", "0")
    for name in ("LES", "MUL"):
        a, b = np.load(on / f"regions_{name}.npz"), np.load(one / f"regions_{name}.npz")
        for key in REGION_KEYS:  # two batches of 4 accumulated = one batch of 8, the float64 table included
            assert a[key].tobytes() == b[key].tobytes(), (name, key)
    _with_stats_of(root, on)
    other = _run(root, "rg_other", *_flags(root), "--pixel_regions", "1", "--run_val", "0", "--run_in", "0", "--pixel_bins", "64",
                 "--pixel_range", "-4", "12", "--pixel_thresholds", "1.5", "--anomaly_z_sigma", "1.5", "--pixel_connectivity", "4")
    rg = _check_file(other / "regions_MUL.npz", other / "zmaps_MUL.npz", _masks_of("MUL"), conn=4, bins=64, value_range=(-4.0, 12.0),
                     thresholds=(1.5,))
    assert rg["regions"][2] == 2 and float(rg["sigma"]) == 1.5


def test_what_the_constructor_refuses(runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root = runs[0]
    with pytest.raises(ValueError, match="--pixel_metrics 1"):
        Reconstruct(cli.parse_args(_argv(root, "--anomaly_z_maps", "1", "--pixel_regions", "1")))
    with pytest.raises(SystemExit):
        cli.parse_args(_argv(root, *_flags(root), "--pixel_regions", "1", "--pixel_connectivity", "6"))
    with pytest.raises(ValueError, match="--pixel_pro_fpr"):
        Reconstruct(cli.parse_args(_argv(root, *_flags(root), "--pixel_regions", "1", "--pixel_pro_fpr", "0")))


def test_command_line_prints_the_files_aupro(runs, capsys):
    """One run of the command line itself; the pooled variant through the function behind it (the lines without the flag:
    tests/test_region_metrics_host.py)."""
    import argparse

    from ddpm_ood_amd import ood
    from ddpm_ood_amd import pixel_metrics as pm

    root, off, on = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        got = subprocess.run([sys.executable, str(ROOT / "ood_detection.py"), "--output_dir", str(root), "--model_name", MODEL, "--out_data",
                              "LES,MUL", "--score", "pixel", "--pixel_regions", "1"], capture_output=True, text=True, check=True).stdout
        capsys.readouterr()
        ood.main_pixels(argparse.Namespace(output_dir=str(root), model_name=MODEL, zmap_key="z_mse_map", pixel_include_in=1, pixel_regions=1,
                                           pixel_pro_fpr=0.1), out_data=["LES", "MUL"])
        pooled = capsys.readouterr().out
        assert f"Pixel AUC for {MODEL} vs LES" in got and "Mean image Dice" in got
        for name in ("LES", "MUL"):
            px, rg = np.load(on / f"pixels_{name}.npz"), np.load(on / f"regions_{name}.npz")
            want = pm.aupro(rg["overlap"][1], int(rg["regions"].sum()), px["hist"][1], 0.3)
            assert 0.0 <= want <= 1.0
            assert f"AUPRO (FPR <= 0.3) for {MODEL} vs {name}: {want * 100:.2f}" in got
            scores = pm.component_scores(rg["components"][:, 1], rg["regions"])
            assert (f"Regions for {MODEL} vs {name} at Z > 2: recall {scores['region_recall'][0]:.4f}, component precision "
                    f"{scores['component_precision'][0]:.4f}, F1 {scores['component_f1'][0]:.4f}") in got
            hist = pm.pool_negatives(px["hist"], np.load(on / "pixels_in.npz")["hist"])  # the in set's pixels enter the FPR only
            want = pm.aupro(rg["overlap"][1], int(rg["regions"].sum()), hist[1], 0.1)
            assert f"AUPRO (FPR <= 0.1) for {MODEL} vs {name}: {want * 100:.2f}" in pooled
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_two_ranks_on_one_gpu_reproduce_the_single_rank_file(device, runs):
    """reconstruct.py --pixel_regions 1 as two ranks (gloo rendezvous, both on cuda:0) on the single-rank run's map_stats.npz: the
    Z-maps are the single-rank run's bits, so every image's integers are the single-rank run's, rows rank-major (0 2 4 6, 1 3 5 7)
    as in the CSV; the all-reduced overlap table adds the same terms in another order.  t = 10 alone (--inference_skip_factor 99)."""
    from test_gpu_dist import _launch_ranks

    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, off, on = runs
    flags = (*_flags(root), "--pixel_regions", "1")
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
            one, two = np.load(single / f"regions_{name}.npz"), np.load(out / f"regions_{name}.npz")
            names = [str(s) for s in one["filename"]]
            assert [str(s) for s in two["filename"]] == [names[i] for i in order]
            assert np.array_equal(two["regions"], one["regions"][order]) and np.array_equal(two["components"], one["components"][order])
            assert two["regions"].dtype == np.int32 and two["components"].dtype == np.int32 and list(two["t"]) == [10]
            R = int(one["regions"].sum())
            err = np.abs(two["overlap"] - one["overlap"])
            print(f"two ranks, {name}: R_total {R}, largest overlap difference {err.max():.3e}")
            assert (err <= ref.overlap_bound(one["overlap"], R)).all()
            for key in ("lo", "hi", "nbins", "thresholds", "sigma", "channels", "connectivity"):
                assert np.array_equal(one[key], two[key]), key
            a, b = np.load(single / f"pixels_{name}.npz"), np.load(out / f"pixels_{name}.npz")
            assert np.array_equal(a["hist"], b["hist"]) and np.array_equal(b["counts"], a["counts"][order])
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
