"""GPU: the kernels of csrc/segment3d.hip against the restatements of tests/voxel_segment_ref.py, values and integers exactly
(DESIGN 3.31)."""

import numpy as np
import pytest
import torch

import voxel_ref
import voxel_segment_ref as ref

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD
# extents 1 and 2 (the reflection repeats); odd; N > 1; 33^3: nine tiles in h and d; 9 x 9 x 65: the 8 x 8 x 64 tile plus one voxel
# in every axis
MEDIAN_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 5), (2, 2, 3, 4), (1, 5, 1, 7), (3, 5, 6, 7), (1, 33, 33, 33), (2, 9, 9, 65)]


def _ids(s):
    return "x".join(map(str, s))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- 1. median --------------------------------------------------------------------------------------------------------------------

def _median_inputs(shape):
    """name -> fp32 [N, D, H, W]: few distinct values (ties in every window), normal values, +-inf and both zeros, NaN (of either
    sign) at 10 % and at 60 % of the voxels (most windows hold more NaN than numbers)."""
    rng = np.random.default_rng(shape[1] * 10000 + shape[2] * 100 + shape[3])
    ties = rng.integers(-3, 4, size=shape).astype(np.float32)
    wide = rng.standard_normal(shape).astype(np.float32)
    special = np.asarray([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e38], dtype=np.float32)
    infs = np.where(rng.random(shape) < 0.3, rng.choice(special, size=shape), wide).astype(np.float32)
    out = {"ties": ties, "normal": wide, "inf": infs}
    nans = np.asarray([np.nan, np.nan], dtype=np.float32)
    nans.view(np.uint32)[1] |= 0x80000000  # (a NaN with the sign bit set)
    for frac in (0.1, 0.6):
        out[f"nan{frac}"] = np.where(rng.random(shape) < frac, rng.choice(nans, size=shape), infs).astype(np.float32)
    return out


@pytest.mark.parametrize("shape", MEDIAN_SHAPES, ids=_ids)
def test_map_median3d_equals_the_restatement(device, shape):
    from ddpm_ood_amd import ops

    for name, v in _median_inputs(shape).items():
        want = ref.median(v)
        got = ops.map_median3d(_dev(v, device), 3)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        assert ref.same_values(got.cpu().numpy(), want), (name, shape)
        if name in ("ties", "normal"):  # (no NaN and no zero of either sign among equal zeros: the bits themselves)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, shape)


@pytest.mark.parametrize("shape", [(2, 1, 33, 31), (1, 1, 17, 130), (3, 1, 1, 9), (1, 1, 2, 2)], ids=_ids)
def test_map_median3d_of_one_plane_has_the_bits_of_map_median(device, shape):
    """The reflected depth triples every value: the median of the 27 is the median of the 9."""
    from ddpm_ood_amd import ops

    for name, v in _median_inputs(shape).items():
        x = _dev(v, device)
        flat = ops.map_median(x.reshape(shape[0], shape[2], shape[3]).contiguous(), 3)
        assert torch.equal(ops.map_median3d(x, 3).view(torch.int32).reshape(flat.shape), flat.view(torch.int32)), (name, shape)


def test_map_median3d_depends_on_nothing_but_the_volume(device):
    """A volume alone equals its row in a batch; the caller's ``out``, poisoned or all ones, is overwritten everywhere; twice the
    same bytes."""
    from ddpm_ood_amd import ops

    shape = (3, 9, 10, 66)
    v = _median_inputs(shape)["nan0.1"]
    want = ref.median(v)
    x = _dev(v, device)
    batch = ops.map_median3d(x, 3)
    assert torch.equal(ops.map_median3d(x, 3).view(torch.int32), batch.view(torch.int32))
    for n in range(3):
        assert torch.equal(ops.map_median3d(x[n:n + 1].contiguous(), 3).view(torch.int32), batch[n:n + 1].view(torch.int32))
    for fill in (POISON, 0x3F800000):
        out = torch.full(shape, fill, dtype=torch.int32, device=device).view(torch.float32)
        assert ops.map_median3d(x, 3, out=out).data_ptr() == out.data_ptr()
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
    """Ground-truth masks of a few boxes per volume (volume 0: none)."""
    N, D, H, W = shape
    rng = np.random.default_rng(seed)
    g = np.zeros(shape, dtype=np.uint8)
    for n in range(1, N):
        for _ in range(int(rng.integers(1, 4))):
            z, y, x = rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)
            g[n, z:z + rng.integers(1, max(2, D // 2)), y:y + rng.integers(1, max(2, H // 2)), x:x + rng.integers(1, max(2, W // 2))] = 1
    return g


def _check(device, v, g, thresholds, min_size, conn, truth=None):
    from ddpm_ood_amd import ops

    labels, regions = truth if truth is not None else ref.label(g, conn)
    want = ref.segment(v, g, labels, regions, thresholds, min_size, conn)
    tv, tg, tl, tr = (_dev(a, device) for a in (v, g, labels, regions))
    got = ops.map_segment3d(tv, tg, tl, tr, thresholds, min_size, conn)
    N, D, H, W = v.shape
    K = len(thresholds)
    assert [tuple(t.shape) for t in got] == [(N, K, D, H, W), (N, K, 3), (N, K, 3), (N, K, 2)]
    assert [t.dtype for t in got] == [torch.uint8, torch.int32, torch.int32, torch.int32]
    for name, a, b in zip(("seg", "pixels", "components", "removed"), got, want):
        assert np.array_equal(a.cpu().numpy(), b), (name, v.shape, min_size, conn)
    if min_size == 1:  # the three existing ops, integer for integer
        assert torch.equal(got[1], ops.map_mask_counts(tv, tg, thresholds))
        assert torch.equal(got[2], ops.map_component_counts3d(tv, tg, tl, tr, thresholds, conn))
        assert not got[3].any()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got[0].cpu().numpy(), (v[:, None] > np.asarray(thresholds, dtype=np.float32)[None, :, None, None, None]))
    return got


def _inputs(shape):
    """name -> uint8 [N, D, H, W]: voxel_ref's named shapes (volume n of a batch flipped so that the volumes differ) and random
    masks at three densities."""
    N, D, H, W = shape
    out = {}
    for name, m in voxel_ref.named_shapes(D, H, W).items():
        out[name] = np.stack([m if n % 2 == 0 else m[::-1, ::-1, ::-1] for n in range(N)])
    for d in (0.05, 0.3, 0.7):
        out[f"random{d}"] = voxel_ref.random_masks(N, D, H, W, d, seed=int(d * 100) + D * H * W)
    return out


# (2, 5, 6, 7): less than one workgroup; (1, 9, 10, 70): rows that straddle waves, 25 workgroups, P no multiple of 64;
# (2, 3, 16, 64): every wave one whole row
@pytest.mark.parametrize("conn", [6, 18, 26])
@pytest.mark.parametrize("shape", [(2, 5, 6, 7), (1, 9, 10, 70), (2, 3, 16, 64)], ids=_ids)
def test_map_segment3d_equals_the_restatement(device, shape, conn):
    """The named shapes (the serpentine among them: one component through every workgroup) and random densities as {v > 2}, K = 3,
    min_size 1, 2, 5 and the whole volume."""
    N, D, H, W = shape
    g = _truth(shape, seed=D + H + W)
    truth = ref.label(g, conn)
    for name, m in _inputs(shape).items():
        v = _values(m, seed=D * H * W + conn)
        for min_size in (1, 2, 5, D * H * W):
            _check(device, v, g, [2.0, 2.5, 3.0], min_size, conn, truth)


@pytest.mark.parametrize("K", [1, 8])
def test_map_segment3d_one_and_eight_thresholds_nan_among_them(device, K):
    shape = (3, 6, 9, 11)
    g = _truth(shape, seed=K)
    m = voxel_ref.random_masks(*shape, 0.4, seed=K)
    v = _values(m, seed=K)  # (NaN voxels outside)
    for min_size in (1, 3, 2 ** 31 - 1):
        got = _check(device, v, g, THRESHOLDS[:K] if K > 1 else [np.nan], min_size, 18)
        if K == 1:  # a NaN threshold predicts nothing
            assert not got[0].any() and not got[1][..., :2].any() and not got[2].any() and not got[3].any()
    _check(device, v, g, [2.0], 2, 26)


def test_map_segment3d_keeps_min_size_and_drops_one_less(device):
    """Bars of 4 and of 5 voxels along each axis at min_size 5; diagonal pairs that are one component only at 18 / 26."""
    m = np.zeros((1, 12, 12, 12), dtype=np.uint8)
    m[0, 0, 0, 0:4] = m[0, 2, 0, 0:5] = 1
    m[0, 4, 0:4, 11] = m[0, 6, 0:5, 11] = 1
    m[0, 7:11, 5, 5] = m[0, 7:12, 9, 9] = 1
    m[0, 0, 6, 0:3] = m[0, 0, 7, 3:5] = 1  # 3 + 2 voxels joined by an edge: 5 at 18 and 26, two small ones at 6
    m[0, 3, 6, 0:3] = m[0, 4, 7, 3:5] = 1  # joined by a corner: 5 at 26 only
    g = np.zeros_like(m)
    g[0, 2] = 1
    g[0, 0] = 1
    v = _values(m, seed=3)
    for conn, kept in ((6, 3), (18, 4), (26, 5)):
        got = _check(device, v, g, [2.0], 5, conn)
        assert int(got[2][0, 0, 1]) == kept and int(got[3][0, 0, 0]) == {6: 7, 18: 5, 26: 3}[conn]
        _check(device, v, g, [2.0], 4, conn)


def test_map_segment3d_a_component_of_more_than_65536_voxels(device):
    """24 x 48 x 64 = 73 728 voxels (the smallest count above 2^16 with whole waves per row): the full volume is one component
    whose size no 16-bit counter holds, counted by 1 152 additions; with a slab removed, two components, one below min_size."""
    shape = (1, 24, 48, 64)
    P = 24 * 48 * 64
    m = np.ones(shape, dtype=np.uint8)
    g = _truth((2,) + shape[1:], seed=5)[1:]
    v = np.where(m != 0, np.float32(3.5), np.float32(0.5)).astype(np.float32)
    for min_size in (1, P, P + 1):
        got = _check(device, v, g, [2.0], min_size, 6)
        assert int(got[3][0, 0, 1]) == (P if min_size > P else 0)
    v[0, 1] = 0.5  # one plane of 3 072 voxels in front, 22 planes behind
    got = _check(device, v, g, [2.0], 3073, 26)
    assert got[3].cpu().tolist() == [[[1, 3072]]]


@pytest.mark.parametrize("shape", [(2, 1, 33, 31), (1, 1, 128, 128), (3, 1, 1, 70)], ids=_ids)
def test_map_segment3d_of_one_plane_equals_map_segment(device, shape):
    """Connectivity 26 <-> 8 and 6 <-> 4: every output of the 2-D op."""
    from ddpm_ood_amd import ops

    N, _, H, W = shape
    g = _truth(shape, seed=H)
    for d in (0.3, 0.6):
        v = _values(voxel_ref.random_masks(*shape, d, seed=W), seed=H + W)
        tv, tg = _dev(v, device), _dev(g, device)
        for c3, c2 in ((26, 8), (6, 4)):
            labels, regions = ops.map_label3d(tg, c3)
            for min_size in (1, 4):
                got = ops.map_segment3d(tv, tg, labels, regions, THRESHOLDS, min_size, c3)
                flat = ops.map_segment(tv.reshape(N, H, W), tg.reshape(N, H, W), labels.reshape(N, H, W), regions, THRESHOLDS, min_size, c2)
                for name, a, b in zip(("seg", "pixels", "components", "removed"), got, flat):
                    assert torch.equal(a.reshape(b.shape), b), (name, shape, d, c3, min_size)


def test_map_segment3d_twice_the_same_bytes(device):
    from ddpm_ood_amd import ops

    shape = (2, 9, 10, 70)
    g = _truth(shape, seed=1)
    v = _values(voxel_ref.random_masks(*shape, 0.3, seed=2), seed=3)
    tv, tg = _dev(v, device), _dev(g, device)
    labels, regions = ops.map_label3d(tg, 26)
    first = ops.map_segment3d(tv, tg, labels, regions, THRESHOLDS, 3, 26)
    second = ops.map_segment3d(tv, tg, labels, regions, THRESHOLDS, 3, 26)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
