"""-m gpu: the anomaly maps of volumes -- ``ops.lpips_map_upsample_view`` and ``ops.map_blur3d`` against the float64
restatements of tests/volume_ref.py (the 2-D ones of anomaly_ref.py / zmap_ref.py applied per slice / in the library's pass
order), ``PerceptualLoss.forward_with_volume_map`` against the 2-D method on the slices and the CPU oracle's features, the
extent-generic statistics through ``MapPass``, and both new kernels inside guard bands.

Tolerances (``test_gpu_ops._close``: err <= tol (1 + max |ref|); u = 2^-24):
  view upsample   1e-5, the project's bound for ``lpips_map_upsample`` (tests/test_gpu_anomaly_maps.py): the same expressions per
                  slice; it holds for source coordinates below 16, so every plane here stays <= 64.  Three accumulated calls: 1e-5.
  volume LPIPS    2e-5, the project's bound for the whole LPIPS; the mean of three views is a convex combination of maps that
                  each hold it, and three more roundings of values below 1 (3 u) vanish beside it.
  map_blur3d      the 2-D test's per-pass term, 2 (2 r + 1) u (1 + (2 r + 1) u) max |in|, over three passes: every pass's
                  weights are positive and sum to 1 within (2 r + 1) u, so an earlier pass's error goes through the later
                  ones amplified by at most that factor: 6 (2 r + 1) u (1 + (2 r + 1) u)^2 max |in|.
  statistics      those of tests/test_gpu_anomaly_z_maps.py: mean (B + 4 (k - 1)) u L after k updates, variance VAR_TOL["sq"] of
                  the mean variance, Z (2 n_t + 1) u L per element; the smoothed Z-maps add the blur's bound at max |z|.
"""

import types

import numpy as np
import pytest
import torch

import anomaly_ref
import volume_ref as vref
import zmap_ref
from test_gpu_ops import _close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. lpips_map_upsample_view -----------------------------------------------------------------------------------------------------
# odd W (unaligned stores); rectangular planes; planes [D, W]; more slices than a wavefront
VIEW_CASES = [((2, 32, 32, 5), 4), ((1, 5, 35, 40), 2), ((1, 32, 3, 47), 3), ((1, 64, 48, 70), 4)]
VIEW_IDS = ["2x32x32x5-axis4", "1x5x35x40-axis2", "1x32x3x47-axis3", "1x64x48x70-axis4"]


def _view_case(shape, axis, seed=0):
    """(packed rows [N * S, row + 5], the plane's layer sizes, (D, H, W))."""
    vol = tuple(shape[1:])
    sizes = anomaly_ref.pyramid_sizes(*vref.plane_of(vol, axis))
    assert min(min(s) for s in sizes) >= 1 and max(max(s) for s in sizes) < 16
    rows = shape[0] * vol[axis - 2]
    return torch.rand(rows, sum(h * w for h, w in sizes) + 5, generator=_g(seed + axis + rows)), sizes, vol


@pytest.mark.parametrize("shape,axis", VIEW_CASES, ids=VIEW_IDS)
def test_view_upsample_against_float64_and_the_2d_kernel(device, shape, axis):
    from ddpm_ood_amd import ops

    maps, sizes, vol = _view_case(shape, axis)
    got = ops.lpips_map_upsample_view(maps.to(device), sizes, vol, axis)
    assert got.shape == shape and got.dtype == torch.float32
    _close(got, vref.upsample_view(maps, sizes, vol, axis), tol=1e-5)
    _close(ops.lpips_map_upsample_view(maps.to(device), sizes, vol, axis, weight=0.25), vref.upsample_view(maps, sizes, vol, axis, 0.25),
           tol=1e-5)
    # the existing 2-D kernel on the same slices, moved into the volume's layout by torch
    flat = ops.lpips_map_upsample(maps.to(device), sizes, vref.plane_of(vol, axis))
    moved = vref.slices_to_volume(flat, shape[0], axis).contiguous()
    print(f"view upsample {shape} axis {axis}: bits equal to lpips_map_upsample per slice: {_bits(got, moved)}; "
          f"max |diff| {float((got - moved).abs().max()):.3e}")
    _close(got, moved.double(), tol=1e-5)
    # three calls with weight 1 / 3 into one buffer, against the same sequence in float64
    acc, want = torch.zeros_like(got), torch.zeros(shape, dtype=torch.float64)
    for k in range(3):
        mk = _view_case(shape, axis, seed=10 + k)[0]
        assert ops.lpips_map_upsample_view(mk.to(device), sizes, vol, axis, weight=1.0 / 3.0, out=acc) is acc
        want = vref.upsample_view(mk, sizes, vol, axis, weight=1.0 / 3.0, out=want)
    _close(acc, want, tol=1e-5)


def test_view_upsample_refuses_what_it_cannot_do(device):
    from ddpm_ood_amd import ops

    maps, sizes, vol = _view_case((2, 32, 32, 5), 4)
    maps = maps.to(device)
    for axis in (1, 5, 0, -1, 2.5):
        with pytest.raises(ValueError, match="axis"):
            ops.lpips_map_upsample_view(maps, sizes, vol, axis)
    with pytest.raises(ValueError, match="empty AlexNet layer"):
        ops.lpips_map_upsample_view(maps, [(7, 7), (3, 3), (1, 0), (1, 0), (1, 0)], vol, 4)
    for bad_sizes in ([], sizes + [(1, 1)], [(9, 8)]):  # no layer, six, more than the row of 66 holds
        with pytest.raises(ValueError):
            ops.lpips_map_upsample_view(maps, bad_sizes, vol, 4)
    with pytest.raises(ValueError, match="whole number of volumes"):
        ops.lpips_map_upsample_view(maps, sizes, (32, 32, 4), 4)  # 10 rows, 4 slices per volume
    with pytest.raises(ValueError, match="whole number of volumes"):
        ops.lpips_map_upsample_view(maps[:3], sizes, vol, 4)  # fewer rows than one volume has slices
    with pytest.raises(ValueError):
        ops.lpips_map_upsample_view(maps, sizes, (32, 32), 4)
    with pytest.raises(ValueError):
        ops.lpips_map_upsample_view(maps, sizes, vol, 4, out=torch.zeros(2, 32, 32, 6, device=device))
    with pytest.raises(ValueError):
        ops.lpips_map_upsample_view(maps, sizes, vol, 4, out=torch.zeros(2, 32, 32, 10, device=device)[..., ::2])
    with pytest.raises(ValueError, match="aliases"):
        big = torch.zeros(2 * 32 * 32 * 5 + maps.numel(), device=device)
        ops.lpips_map_upsample_view(big[-maps.numel():].view(maps.shape), sizes, vol, 4, out=big[maps.numel() // 2:][:2 * 32 * 32 * 5].view(2, 32, 32, 5))
    with pytest.raises(RuntimeError):
        ops.lpips_map_upsample_view(maps.cpu(), sizes, vol, 4)


# ---- 2. PerceptualLoss.forward_with_volume_map --------------------------------------------------------------------------------------
# (D, H, W): 8 slices along the last axis, 16 images per feature pass (the general first layer); 40 slices, 80 images (>= 64: the
# bulk grey fold)
ITEMS = {"general": (32, 32, 8), "bulk": (32, 32, 40)}


@pytest.fixture(scope="module")
def losses(device):
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS, PerceptualLoss

    cpu = oracle.LPIPSAlex()
    cpu.load_state_dict(LPIPS().state_dict())  # the seeded default: what both PerceptualLoss instances below hold
    return PerceptualLoss(3).to(device), PerceptualLoss(2).to(device), cpu


def _volumes(vol, device, seed=0):
    g = _g(seed + sum(vol))
    return torch.rand((1, 1) + vol, generator=g).to(device), torch.rand((1, 1) + vol, generator=g).to(device)


def _view_map_2d(pl2, y, p, axis):
    """[1, D, H, W]: the 2-D ``forward_with_map`` of the slices along ``axis``, back in the volume's layout."""
    _, m = pl2.forward_with_map(vref.volume_to_slices(y, axis), vref.volume_to_slices(p, axis))
    return vref.slices_to_volume(m[:, 0], y.shape[0], axis)


@pytest.mark.parametrize("item", list(ITEMS))
def test_volume_map_value_and_the_last_view(device, losses, item):
    pl3, pl2, cpu = losses
    vol = ITEMS[item]
    y, p = _volumes(vol, device)
    assert (2 * vol[2] >= 64) == (item == "bulk")
    plain = pl3(y, p)
    val, vmap = pl3.forward_with_volume_map(y, p)
    assert val.shape == plain.shape == () and torch.equal(val, plain)  # the score's own launches: the same bits
    assert vmap.shape == (1, 1) + vol and vmap.dtype == torch.float32
    want2d = _view_map_2d(pl2, y, p, 4)
    print(f"volume map {item}: bits equal to forward_with_map on the slices: {_bits(vmap[:, 0], want2d.contiguous())}")
    _close(vmap[:, 0], want2d.double(), tol=2e-5)
    oracle_map = anomaly_ref.spatial_lpips(cpu, vref.volume_to_slices(y.cpu(), 4), vref.volume_to_slices(p.cpu(), 4), normalize=True)
    _close(vmap[:, 0], vref.slices_to_volume(oracle_map[:, 0], 1, 4), tol=2e-5)
    assert float(vmap.max()) > 1e-3
    # the accumulated map and a fresh second one from the same feature pass
    acc = torch.zeros((1,) + vol, device=device)
    val2, first, second = pl3.forward_with_volume_map(y, p, weight=0.5, out=acc, second_weight=1.0)
    assert torch.equal(val2, plain) and first.data_ptr() == acc.data_ptr() and second.shape == vmap.shape
    assert _bits(second, vmap) and _bits(acc, 0.5 * vmap[:, 0])  # (0 + 0.5 x is 0.5 x, exactly)
    val3, again = pl3.forward_with_volume_map(y, p, weight=0.5, out=acc)
    assert torch.equal(val3, plain) and again.data_ptr() == acc.data_ptr()
    _close(acc, vmap[:, 0].double(), tol=2e-5)


def test_volume_map_over_all_views_is_the_mean_of_the_three(device, losses):
    pl3, pl2, _ = losses
    vol = ITEMS["bulk"]
    y, p = _volumes(vol, device, seed=1)
    plain = pl3(y, p)
    val, vmap = pl3.forward_with_volume_map(y, p, views="all")
    assert torch.equal(val, plain) and vmap.shape == (1, 1) + vol
    views = [_view_map_2d(pl2, y, p, axis).double() for axis in (2, 3, 4)]
    _close(vmap[:, 0], sum(views) / 3.0, tol=2e-5)
    last = pl3.forward_with_volume_map(y, p)[1]
    assert float((vmap - last).abs().max()) > 1e-3  # (the other two views do change the map)
    val2, acc, second = pl3.forward_with_volume_map(y, p, views="all", weight=0.25, out=torch.zeros((1,) + vol, device=device),
                                                    second_weight=1.0)
    assert torch.equal(val2, plain) and _bits(second, vmap)
    _close(acc[:, 0], 0.25 * vmap[:, 0].double(), tol=2e-5)


def test_volume_map_refusals(device, losses):
    pl3, pl2, _ = losses
    y, p = _volumes(ITEMS["general"], device)
    with pytest.raises(ValueError, match="empty AlexNet layer"):
        pl3.forward_with_volume_map(y, p, views="all")  # the [32, 8] planes of the other two views
    with pytest.raises(ValueError, match="views"):
        pl3.forward_with_volume_map(y, p, views="first")
    with pytest.raises(NotImplementedError):
        pl2.forward_with_volume_map(y, p)
    with pytest.raises(ValueError):
        pl3.forward_with_volume_map(y[0], p[0])
    with pytest.raises(NotImplementedError):  # the 2-D method stays 2-D, the constructor's spatial flag stays refused
        pl3.forward_with_map(y, p)


# ---- 3. map_blur3d ------------------------------------------------------------------------------------------------------------------
# radius above every extent; D = 1; the largest radius across tile edges; W beyond 64 lanes; radius 1
BLUR_CASES = [(1, 5, 5, 5, 2.0), (2, 1, 9, 7, 1.5), (1, 33, 6, 35, 4.0), (1, 20, 17, 66, 1.0), (2, 8, 8, 8, 0.3)]


def _blur_bound(radius):
    return 6 * (2 * radius + 1) * U * (1 + (2 * radius + 1) * U) ** 2


@pytest.mark.parametrize("N,D,H,W,sigma", BLUR_CASES, ids=lambda v: str(v))
def test_map_blur3d_against_float64_and_scipy(device, N, D, H, W, sigma):
    from scipy.ndimage import gaussian_filter

    from ddpm_ood_amd import ops

    radius = int(4 * sigma + 0.5)
    x = torch.randn(N, D, H, W, generator=_g(D * 10000 + H * 100 + W))
    taps32 = ops.gaussian_taps(sigma).astype(np.float32)
    assert len(taps32) == 2 * radius + 1
    got = ops.map_blur3d(x.to(device), sigma)
    assert got.shape == (N, D, H, W) and got.dtype == torch.float32
    want = vref.blur3d(x.numpy(), taps32)
    err = np.abs(got.cpu().double().numpy() - want).max() / float(x.abs().max())
    print(f"blur3d {N}x{D}x{H}x{W} sigma={sigma}: worst err {err / U:.2f} u max|in| (bound {_blur_bound(radius) / U:.0f})")
    assert err <= _blur_bound(radius)
    assert _bits(ops.map_blur3d(x.to(device), taps=torch.from_numpy(taps32).to(device)), got)  # the weights handed over: the same bits
    scipy64 = np.stack([gaussian_filter(v, sigma, mode="reflect", truncate=4.0) for v in x.double().numpy()])
    assert np.abs(vref.blur3d(x.numpy(), zmap_ref.gaussian_taps(sigma)) - scipy64).max() <= 1e-6  # the restatement is scipy's filter
    assert np.abs(want - scipy64).max() <= 1e-6  # (and the fp32 weights are scipy's, rounded)
    const = ops.map_blur3d(torch.full((N, D, H, W), 0.75, device=device), sigma).cpu().double().numpy()
    assert np.abs(const - 0.75).max() <= _blur_bound(radius) * 0.75 + 3 * (2 * radius + 1) * U * 0.75  # (x the fp32 weights' sum, thrice)


def test_map_blur3d_radius_zero_is_a_copy_and_what_it_refuses(device):
    from ddpm_ood_amd import ops

    x = torch.randn(2, 5, 9, 7, generator=_g(5))
    x[0, 0, 0, 0], x[1, 2, 5, 6], x[1, 4, 8, 6] = -0.0, float("inf"), 1e-42  # (a signed zero, an infinity, a subnormal)
    assert _bits(ops.map_blur3d(x.to(device), 0.1).cpu(), x)  # radius int(0.9) = 0: the single weight 1
    assert _bits(ops.map_blur3d(x.to(device), 0.0).cpu(), x)
    xd = x.to(device)
    out = torch.empty_like(xd)
    assert ops.map_blur3d(xd, 1.0, out=out) is out and _bits(out, ops.map_blur3d(xd, 1.0))
    with pytest.raises(ValueError, match="aliases"):
        ops.map_blur3d(xd, 1.0, out=xd)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_blur3d(xd[:1], 1.0, out=xd.view(-1)[7:7 + 5 * 9 * 7].view(1, 5, 9, 7))
    with pytest.raises(ValueError, match="radius"):
        ops.map_blur3d(xd, 4.2)  # radius 17
    with pytest.raises(ValueError, match="radius"):
        ops.map_blur3d(xd, taps=torch.ones(35, device=device))
    with pytest.raises(ValueError):
        ops.map_blur3d(xd, taps=torch.ones(4, device=device))
    with pytest.raises(ValueError):
        ops.map_blur3d(xd, 1.0, taps=torch.ones(3, device=device))
    with pytest.raises(ValueError):
        ops.map_blur3d(xd, -1.0)
    with pytest.raises(ValueError):
        ops.map_blur3d(xd[0], 1.0)
    with pytest.raises(ValueError):
        ops.map_blur3d(xd, 1.0, out=torch.empty(2, 5, 9, 8, device=device))
    with pytest.raises(RuntimeError):
        ops.map_blur3d(x, 1.0)


# ---- 4. statistics and Z-maps of volumes through MapPass -----------------------------------------------------------------------------

def test_statistics_and_z_maps_of_volumes(device):
    """Two validation batches of [3, 2, 2, 4, 6, 5] through ``MapPass`` (one ``map_stats_update`` each), then the smoothed Z-maps
    of a third against the statistics: every step against the float64 restatement, at the bounds of the 2-D kernels' tests."""
    from test_gpu_anomaly_z_maps import VAR_TOL

    from ddpm_ood_amd import ops
    from ddpm_ood_amd.map_passes import MapPipeline, MapSettings

    B, n_t, sigma, rel_floor = 3, 2, 1.0, 0.01
    extent = (4, 6, 5)
    rng = np.random.default_rng(7)
    v = ((rng.standard_normal((3 * B, n_t, 2) + extent) ** 2) * 1e-2).astype(np.float32)
    pipe = MapPipeline(MapSettings(volume_z_maps=True, z_sigma=sigma, z_std_floor=rel_floor), device, ".")
    loader, scores = types.SimpleNamespace(names=[]), torch.zeros(B, n_t, 2, device=device)
    val = pipe.begin("val", loader, [10, 970])
    for k in range(2):
        val.add_batch(scores, None, torch.from_numpy(v[k * B:(k + 1) * B]).to(device))
        rows = v[:(k + 1) * B].astype(np.float64)
        L = np.abs(rows).max()
        n, mean, m2 = val.stats.tables()
        assert n == (k + 1) * B and mean.shape == (n_t, 2) + extent == m2.shape
        err = np.abs(mean - rows.mean(axis=0)).max()
        var = rows.var(axis=0, ddof=1)
        verr = np.abs(m2 / (n - 1) - var).max() / var.mean()
        print(f"volume stats k={k + 1}: mean err {err / (U * L):.2f} u L (bound {B + 4 * k}); var err {verr:.2e} (bound {VAR_TOL['sq']:.0e})")
        assert err <= (B + 4 * k) * U * L and verr <= VAR_TOL["sq"]
    _, want_mean, want_m2 = zmap_ref.chan_chunks(v[:2 * B].astype(np.float64), [B, B])
    assert np.abs(mean - want_mean).max() <= (B + 4) * U * L and np.abs(m2 - want_m2).max() <= VAR_TOL["sq"] * want_m2.mean()
    val.finish_validation()
    stats = pipe.last_map_stats[0]
    mean32, inv32 = stats.finalize(rel_floor)
    std32 = stats.std()
    assert mean32.shape == inv32.shape == std32.shape == (n_t, 2) + extent and stats.floor(rel_floor).shape == (n_t, 2)
    want_inv = vref.floor_inv_std(std32, rel_floor)  # the floor over every voxel of a (t, c), from the same fp32 std
    assert np.abs(inv32 - want_inv).max() <= U * want_inv.max()  # float64, rounded once
    assert np.array_equal(stats.floor(rel_floor), (rel_floor * std32.astype(np.float64).max(axis=(2, 3, 4))).astype(np.float32))
    # the third batch: Z against the fp32 tables, the mean over t, smoothed in 3-D
    run = pipe.begin("in", loader, [10, 970])
    run.add_batch(scores, None, torch.from_numpy(v[2 * B:]).to(device))
    got = run.zmaps[0].double().numpy()
    assert got.shape == (B, 2) + extent
    w = float(np.float32(1.0 / n_t))
    addends = (v[2 * B:].astype(np.float64) - mean32[None]) * inv32.astype(np.float64)[None]
    Lz = w * np.maximum(np.abs(addends).max(axis=1), np.abs(np.cumsum(addends, axis=1)).max(axis=1))
    z64 = zmap_ref.zscore(v[2 * B:], mean32, inv32, weight=w)
    raw = ops.map_zscore(torch.from_numpy(v[2 * B:]).to(device), torch.from_numpy(mean32).to(device), torch.from_numpy(inv32).to(device))
    ratio = (np.abs(raw.cpu().double().numpy() - z64) / (U * Lz + 1e-300)).max()
    print(f"volume zscore: worst err {ratio:.2f} u L (bound {2 * n_t + 1})")
    assert ratio <= 2 * n_t + 1 and float(np.abs(z64).max()) > 1.0
    radius = int(4 * sigma + 0.5)
    taps32 = ops.gaussian_taps(sigma).astype(np.float32)
    want = vref.blur3d(z64.reshape((2 * B,) + extent), taps32).reshape(got.shape)
    # the Z error goes through three passes whose weights sum to at most 1 + (2 r + 1) u each; the blur's own bound at max |z|
    bound = (2 * n_t + 1) * U * Lz.max() * (1 + (2 * radius + 1) * U) ** 3 + _blur_bound(radius) * np.abs(z64).max() * (1 + 1e-6)
    err = np.abs(got - want).max()
    print(f"volume z-maps sigma={sigma}: err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert _bits(run.zmaps[0], ops.map_blur3d(raw.reshape((2 * B,) + extent), sigma).reshape(got.shape).cpu())  # (what smooth launches)


# ---- 5. memory bounds ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,axis", VIEW_CASES[:3], ids=VIEW_IDS[:3])
def test_view_upsample_stays_inside_its_buffers(device, shape, axis):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    maps, sizes, vol = _view_case(shape, axis)
    _bounds(device, dict(maps=(maps, True)), lambda t: ops.lpips_map_upsample_view(t["maps"], sizes, vol, axis))
    acc = torch.rand(shape, generator=_g(13))
    _bounds(device, dict(maps=(maps, True), acc=(acc, False)),
            lambda t: ops.lpips_map_upsample_view(t["maps"], sizes, vol, axis, weight=0.5, out=t["acc"]))


@pytest.mark.parametrize("N,D,H,W,sigma", BLUR_CASES[:3], ids=lambda v: str(v))
def test_map_blur3d_stays_inside_its_buffers(device, N, D, H, W, sigma):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    x = torch.randn(N, D, H, W, generator=_g(D))
    taps = torch.from_numpy(ops.gaussian_taps(sigma).astype(np.float32))
    _bounds(device, dict(x=(x, True)), lambda t: ops.map_blur3d(t["x"], sigma))  # the wrapper uploads the weights itself
    _bounds(device, dict(x=(x, True), taps=(taps, True)), lambda t: ops.map_blur3d(t["x"], taps=t["taps"]))
