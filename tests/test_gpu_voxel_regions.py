"""GPU: the kernels of csrc/regions3d.hip against tests/voxel_ref.py (scipy.ndimage.label with the three 3-D structures; the
float64 overlap, the counts and aupro_direct restated flat): labels, regions and counts as integers, the overlap table bit for
bit, D = 1 volumes against the 2-D ops' bits."""

import numpy as np
import pytest
import torch

import pixel_ref
import voxel_ref as ref

pytestmark = pytest.mark.gpu

# one voxel; odd extents on every axis; W past a wave and a row of a workgroup; odd and past a wave; numbering and unions across
# workgroups (64 000 voxels = 250 workgroups)
EXTENTS = [(1, 1, 1), (3, 5, 7), (2, 3, 130), (17, 33, 65), (40, 40, 40)]
CONNS = [26, 18, 6]
LO, HI = -16.0, 48.0


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _ids(e):
    return "x".join(map(str, e))


def _inputs(extent):
    """name -> uint8 [2, D, H, W]: the named shapes (the second volume flipped, so that the two differ), the touching cubes and
    random masks at three densities (0.3: near the 6-connected percolation threshold, large ragged clusters)."""
    D, H, W = extent
    out = {name: np.stack([m, m[::-1, ::-1, ::-1]]) for name, m in ref.named_shapes(D, H, W).items()}
    for d in (0.05, 0.3, 0.6):
        out[f"random{d}"] = ref.random_masks(2, D, H, W, d, seed=int(d * 100) + D * H * W)
    return out


@pytest.fixture(scope="module")
def label_cases():
    """(extent, name, connectivity) -> (mask, labels, regions) of the reference, computed once."""
    out = {}
    for extent in EXTENTS:
        for name, m in _inputs(extent).items():
            for conn in CONNS:
                out[extent, name, conn] = (m,) + ref.label(m, conn)
    return out


# ---- 1. labelling -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("extent", EXTENTS, ids=_ids)
def test_map_label3d_equals_scipy(device, label_cases, extent, conn):
    """Both predicates, every named shape and density, as integers."""
    from ddpm_ood_amd import ops

    for name in _inputs(extent):
        m, want_l, want_r = label_cases[extent, name, conn]
        labels, regions = ops.map_label3d(_dev(m, device), conn)
        assert labels.dtype == regions.dtype == torch.int32 and tuple(labels.shape) == m.shape
        assert np.array_equal(regions.cpu().numpy(), want_r), (name, regions.cpu().tolist(), want_r.tolist())
        assert np.array_equal(labels.cpu().numpy(), want_l), name
        v = np.where(m != 0, np.float32(1.5), np.float32(0.5)).astype(np.float32)
        labels, regions = ops.map_label3d(_dev(v, device), conn, threshold=1.0)
        assert np.array_equal(regions.cpu().numpy(), want_r) and np.array_equal(labels.cpu().numpy(), want_l), name


@pytest.mark.parametrize("kind,joined_from", [("face", 6), ("edge", 18), ("corner", 26)])
def test_touching_cubes_separate_the_three_connectivities(device, kind, joined_from):
    from ddpm_ood_amd import ops

    m = ref.two_cubes(kind)[None]
    for conn in CONNS:
        want_l, want_r = ref.label(m, conn)
        assert int(want_r[0]) == (1 if conn >= joined_from else 2)
        labels, regions = ops.map_label3d(_dev(m, device), conn)
        assert np.array_equal(regions.cpu().numpy(), want_r) and np.array_equal(labels.cpu().numpy(), want_l), (kind, conn)


def test_map_label3d_f32_nan_voxel_and_nan_threshold(device):
    from ddpm_ood_amd import ops

    rng = np.random.default_rng(5)
    v = rng.normal(1.0, 1.0, (2, 5, 9, 70)).astype(np.float32)
    v[0, 2, 4, 30:40] = np.nan
    v[1, 0, 0, 0] = np.nan
    v[1, 3] = np.inf
    for conn in CONNS:
        want_l, want_r = ref.label(v, conn, threshold=1.0)
        labels, regions = ops.map_label3d(_dev(v, device), conn, threshold=1.0)
        assert np.array_equal(regions.cpu().numpy(), want_r) and np.array_equal(labels.cpu().numpy(), want_l)
        assert (labels.cpu().numpy()[np.isnan(v)] == 0).all()
    labels, regions = ops.map_label3d(_dev(v, device), 26, threshold=float("nan"))
    assert int(regions.abs().sum()) == 0 and int(labels.abs().sum()) == 0


def test_map_label3d_depends_on_nothing_but_the_volume(device, label_cases):
    """A volume's labels do not depend on its place in a batch, on a second run, or on what outputs and scratch held."""
    from ddpm_ood_amd import _lib, ops

    extent = (17, 33, 65)
    D, H, W = extent
    batch = np.concatenate([label_cases[extent, name, 26][0] for name in ("random0.3", "serpentine", "checkerboard")])
    t = _dev(batch, device)
    lb, rb = ops.map_label3d(t, 26)
    again_l, again_r = ops.map_label3d(t, 26)
    assert torch.equal(lb, again_l) and torch.equal(rb, again_r)
    for n in range(batch.shape[0]):
        l1, r1 = ops.map_label3d(t[n:n + 1].contiguous(), 26)
        assert torch.equal(l1[0], lb[n]) and int(r1[0]) == int(rb[n])
    lib = _lib.load()
    N = batch.shape[0]
    nbytes = ops.map_label3d_scratch_bytes(N, D, H, W)
    assert nbytes >= 4 * N * D * H * W
    for fill in (0xFF, 0x00):
        labels = torch.full((N, D, H, W), -1 if fill else 0, dtype=torch.int32, device=device)
        regions = torch.full((N,), -1 if fill else 0, dtype=torch.int32, device=device)
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=device)
        assert lib.ddpm_map_label3d_u8(t.data_ptr(), N, D, H, W, 26, labels.data_ptr(), regions.data_ptr(), scratch.data_ptr(),
                                       _lib.stream_ptr()) == 0
        assert torch.equal(labels, lb) and torch.equal(regions, rb)


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31), (1, 128, 128)], ids=_ids)
def test_d1_volumes_give_the_bits_of_the_2d_ops(device, shape):
    """26 -> 8 and 6 -> 4 on planes the 2-D kernels hold: labels, overlap table and counts."""
    from ddpm_ood_amd import ops

    N, H, W = shape
    m = ref.random_masks(N, 1, H, W, 0.45, seed=H)[:, 0]
    v, _ = pixel_ref.case_values(N, H * W, LO, HI, 512, seed=W)
    v = v.reshape(N, H, W)
    tm, tv = _dev(m, device), _dev(v, device)
    thr = [2.0, 20.0, float("nan")]
    for c3, c2 in ((26, 8), (6, 4)):
        l2, r2 = ops.map_label(tm, c2)
        l3, r3 = ops.map_label3d(tm[:, None].contiguous(), c3)
        assert torch.equal(l3[:, 0], l2) and torch.equal(r3, r2)
        a2, b2 = ops.map_label(tv, c2, threshold=20.0)
        a3, b3 = ops.map_label3d(tv[:, None].contiguous(), c3, threshold=20.0)
        assert torch.equal(a3[:, 0], a2) and torch.equal(b3, b2)
        o2 = ops.map_region_overlap(tv, l2, r2, LO, HI, 512)
        o3 = ops.map_region_overlap3d(tv[:, None].contiguous(), l3, r3, LO, HI, 512)
        assert torch.equal(o3.view(torch.int64), o2.view(torch.int64))
        c2d = ops.map_component_counts(tv, tm, l2, r2, thr, c2)
        c3d = ops.map_component_counts3d(tv[:, None].contiguous(), tm[:, None].contiguous(), l3, r3, thr, c3)
        assert torch.equal(c3d, c2d)


# ---- 2. region overlap ------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_overlap_table_is_bit_equal_to_the_float64_restatement(device):
    """The checkerboard at 6 neighbours on 8 x 8 x 8 (256 one-voxel regions) beside a ragged random mask; more regions than a
    chunk holds (chunk_regions 1, 7, 100 through the wrapper); two half-batches with accumulate; NaN voxels in column nbins."""
    from ddpm_ood_amd import ops

    nbins = 64
    m = np.stack([ref.checkerboard(8, 8, 8), ref.random_masks(1, 8, 8, 8, 0.3, seed=3)[0], ref.ball(8, 8, 8, (4, 4, 4), 2.5),
                  np.zeros((8, 8, 8), dtype=np.uint8)])
    v, _ = pixel_ref.case_values(4, 512, LO, HI, nbins, seed=11)
    v = v.reshape(4, 8, 8, 8)
    v[2, 4, 4, 3:6] = np.nan
    labels, regions = ref.label(m, 6)
    assert int(regions[0]) == 256 and int(regions[3]) == 0
    want = ref.overlap(v, labels, regions, LO, HI, nbins)
    assert want[nbins] > 0.0
    tv, tl, tr = _dev(v, device), _dev(labels, device), _dev(regions, device)
    got = ops.map_region_overlap3d(tv, tl, tr, LO, HI, nbins)
    assert got.dtype == torch.float64 and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    for chunk in (1, 7, 100):
        again = ops.map_region_overlap3d(tv, tl, tr, LO, HI, nbins, chunk_regions=chunk)
        assert np.array_equal(_bits(again.cpu().numpy()), _bits(want)), chunk
    total = ops.map_region_overlap3d(tv[:2].contiguous(), tl[:2].contiguous(), tr[:2].contiguous(), LO, HI, nbins, chunk_regions=100)
    out = ops.map_region_overlap3d(tv[2:].contiguous(), tl[2:].contiguous(), tr[2:].contiguous(), LO, HI, nbins, total=total)
    assert out is total and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    lg, rg = ops.map_label3d(_dev(m, device), 6)
    assert np.array_equal(_bits(ops.map_region_overlap3d(tv, lg, rg, LO, HI, nbins).cpu().numpy()), _bits(want))


def test_aupro_from_the_device_tables(device):
    """aupro from the device's overlap table and histogram within 1e-12 of aupro_direct, as in 2-D."""
    from ddpm_ood_amd import ops
    from ddpm_ood_amd import pixel_metrics as pm

    nbins = 64
    D, H, W = 9, 12, 20
    m = np.stack([ref.ball(D, H, W, (4, 5, 6), 3.0) | ref.ball(D, H, W, (6, 9, 15), 2.0), ref.random_masks(1, D, H, W, 0.02, seed=1)[0]])
    rng = np.random.default_rng(2)
    v = (rng.normal(0.0, 1.5, m.shape) + 3.0 * m).astype(np.float32)
    v[0, 0, 0, :3] = np.nan
    for conn in CONNS:
        tm, tv = _dev(m, device), _dev(v, device)
        labels, regions = ops.map_label3d(tm, conn)
        overlap = ops.map_region_overlap3d(tv, labels, regions, LO, HI, nbins).cpu().numpy()
        hist = ops.map_mask_hist(tv, tm, LO, HI, nbins).cpu().numpy()
        R = int(regions.sum())
        for limit in (0.3, 0.05, 1.0):
            assert abs(pm.aupro(overlap, R, hist, limit) - ref.aupro_direct(v, m, LO, HI, nbins, conn, limit)) <= 1e-12, (conn, limit)


# ---- 3. component counts ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("conn", CONNS)
def test_component_counts_equal_the_restatement(device, K, conn):
    """A lesion mask, the zero mask, a mask with no prediction and a prediction with no mask in one batch; twice the same bytes;
    a poisoned scratch changes nothing."""
    from ddpm_ood_amd import _lib, ops

    D, H, W = 10, 19, 67
    rng = np.random.default_rng(conn + K)
    m = np.zeros((4, D, H, W), dtype=np.uint8)
    m[0] = ref.ball(D, H, W, (4, 8, 20), 3.0) | ref.ball(D, H, W, (7, 12, 50), 2.0)
    m[2] = ref.ball(D, H, W, (5, 9, 30), 3.0)
    v = rng.normal(0.0, 1.0, m.shape).astype(np.float32)
    v[0] += 2.5 * m[0]
    v[2] = -5.0                     # a mask, no prediction at the thresholds above -5
    v[3, 2:5, 3:9, 10:40] = 9.0     # a prediction, no mask
    v[1, 0, 0, 0] = np.nan
    thresholds = [2.0] if K == 1 else [2.0, 1.0, 0.0, 3.5, float("nan"), 100.0, -4.0, 8.0]
    labels, regions = ref.label(m, conn)
    want = ref.component_counts(v, m, labels, regions, thresholds, conn)
    assert want[2, 0, 0] == 0 and want[2, 0, 1] == 0 and want[3, 0, 1] >= 1 and want[3, 0, 2] == want[3, 0, 1]
    args = (_dev(v, device), _dev(m, device), _dev(labels, device), _dev(regions, device))
    got = ops.map_component_counts3d(*args, thresholds, conn)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() - want)
    assert torch.equal(ops.map_component_counts3d(*args, thresholds, conn), got)
    lib = _lib.load()
    nbytes = ops.map_component_counts3d_scratch_bytes(4, D, H, W, K)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
    counts = torch.full((4, K, 3), -7, dtype=torch.int32, device=device)
    thr = _dev(np.asarray(thresholds, dtype=np.float32), device)
    assert lib.ddpm_map_component_counts3d_f32(*(a.data_ptr() for a in args), 4, D, H, W, thr.data_ptr(), K, conn, counts.data_ptr(),
                                               scratch.data_ptr(), _lib.stream_ptr()) == 0
    assert torch.equal(counts, got)
