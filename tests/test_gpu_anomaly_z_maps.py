"""-m gpu: the per-pixel Z-maps -- ``ops.map_stats_update``, ``ops.map_zscore`` and ``ops.map_blur`` against the
float64 restatement of tests/zmap_ref.py, the three kernels inside guard bands (tests/test_gpu_memory_bounds.py::_bounds), and
``reconstruct.py --anomaly_z_maps 1`` through the trainer: nothing that was written before moves, and ``map_stats.npz`` /
``zmaps_<name>.npz`` hold what the float64 restatement makes of the very tensors the run handed to ``clamp_mse_``.

Bounds.  u = 2^-24, the relative error of one correctly rounded fp32 operation (the library is built without FMA contraction, so
every operation rounds once); the inputs and the scalars are the same fp32 numbers on both sides.  Each test's docstring derives
its own; the three that are measurements (4 x the worst error seen on an MI355X, rounded up to one digit; profiles/anomaly_z_maps.md)
are VAR_TOL, STD_TOL and Z_TOL below.
"""

import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import anomaly_ref
import zmap_ref as ref
from test_gpu_anomaly_maps import MODEL, SETS, T_STARTS, _argv, _Capture, _run

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# measured (profiles/anomaly_z_maps.md): worst |var - var64| / mean_j var64 over the cases of test_map_stats_update_against_float64
# 1.59e-4 on the 1 + 1e-3 N values (B = 6, P = 1023, after the second update), 3.34e-6 on the 1e-2 N^2 values -> 4 x, one digit up.
# The error on the values near 1 is the fp32 means' own (3e-7 of a deviation of 1e-3, squared into the merge term); over twenty
# other seeds of the same cases, replayed on the host in numpy fp32, it stayed below 2.4e-4.  A sum-of-squares form is off by 1e-1.
VAR_TOL = {"near1": 7e-4, "sq": 2e-5}
# measured through the trainer (the fixture's sets; batch 4, batch 3 and two ranks), err = max |got - f64| / (1 + max |f64|):
# std 3.79e-9 (lpips), 4.35e-8 (mse); z 1.86e-6 without smoothing, 1.14e-6 with sigma = 1.5 -> 4 x, one digit up.
STD_TOL = {"lpips": 2e-8, "mse": 2e-7}
Z_TOL = {0.0: 8e-6, 1.5: 5e-6}


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _off_boundary(t, device):
    """The same values on the device, 4 bytes behind a 16-byte boundary."""
    out = torch.cat([torch.zeros(1), t.reshape(-1)]).to(device)[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


# ---- 1. map_stats_update ------------------------------------------------------------------------------------------------------------

STATS_SHAPES = [(1, 5), (3, 7), (6, 1023), (4, 2 * 4 * 32 * 32)]  # B = 1 (Mb is 0); the scalar path; odd; the 16-byte path


def stats_values(B, P, kind):
    rng = np.random.default_rng(B * 10 + P + (kind == "sq"))
    z = rng.standard_normal((4 * B, P))
    return (1.0 + 1e-3 * z if kind == "near1" else z * z * 1e-2).astype(np.float32)


@pytest.mark.parametrize("kind", ["near1", "sq"])
@pytest.mark.parametrize("B,P", STATS_SHAPES, ids=lambda v: str(v))
def test_map_stats_update_against_float64(device, B, P, kind):
    """Four updates of B rows each, the first into NaN-poisoned tables; after every one the mean and m2 / (n - 1) are held against
    np.mean / np.var(ddof=1) of all rows so far.  Values 1 + 1e-3 N(0, 1) (where a sum and a sum of squares cancel) and
    1e-2 N(0, 1)^2.

    Mean, per column: |err| <= (B + 4 (k - 1)) u L after k updates, L = the largest |value|.  Derivation: mb is B - 1 additions
    whose partial sums are below B L and one division, B roundings worth u L each once carried to the scale of the mean.  A merge
    forms mean + (mb - mean) r = (1 - r) mean + r mb, a convex combination, so the errors the two means carry do not add up: the
    larger one survives; on top come the rounding of the difference (u |delta|; the values are positive, so |delta| <= L), of
    r itself (fp32 of a float64 ratio: u |delta r|), of the product and of the sum (u L): 4 u L per merge.
    Variance: measured, VAR_TOL x the mean variance over the columns (see the constant); on the values near 1 that bound has to be
    below 1e-3 of the variance itself."""
    from ddpm_ood_amd import ops

    v = stats_values(B, P, kind)
    mean = torch.full((P,), float("nan"), device=device)
    m2 = torch.full((P,), float("nan"), device=device)
    assert VAR_TOL["near1"] < 1e-3
    n = 0
    for k in range(4):
        n = ops.map_stats_update(torch.from_numpy(v[k * B:(k + 1) * B]).to(device), n, mean, m2)
        assert n == (k + 1) * B
        rows = v[:n].astype(np.float64)
        L = np.abs(rows).max()
        got_mean, got_m2 = mean.cpu().double().numpy(), m2.cpu().double().numpy()
        assert np.isfinite(got_mean).all() and np.isfinite(got_m2).all() and (got_m2 >= 0).all()  # the poison was not read
        err = np.abs(got_mean - rows.mean(axis=0)).max()
        print(f"stats B={B} P={P} {kind} k={k + 1}: mean err {err / (U * L):.2f} u L (bound {B + 4 * k})", end="")
        assert err <= (B + 4 * k) * U * L
        if n == 1:
            assert (got_m2 == 0).all()
            print()
            continue
        var = rows.var(axis=0, ddof=1)
        verr = np.abs(got_m2 / (n - 1) - var).max() / var.mean()
        print(f"; var err {verr:.2e} of the mean variance (bound {VAR_TOL[kind]:.0e})")
        assert verr <= VAR_TOL[kind]
    # the reference's chunked form agrees with the kernel as closely as with numpy's one-shot form
    _, want_mean, want_m2 = ref.chan_chunks(v.astype(np.float64), [B] * 4)
    assert np.abs(got_mean - want_mean).max() <= (B + 12) * U * L and np.abs(got_m2 - want_m2).max() <= VAR_TOL[kind] * want_m2.mean()


def test_map_stats_update_refuses_what_it_cannot_do(device):
    from ddpm_ood_amd import ops

    v = torch.rand(3, 2, 8, device=device)
    mean, m2 = torch.zeros(2, 8, device=device), torch.zeros(2, 8, device=device)
    with pytest.raises(RuntimeError):
        ops.map_stats_update(v.cpu(), 0, mean, m2)
    with pytest.raises(ValueError):
        ops.map_stats_update(v, 0, mean[:1], m2)
    with pytest.raises(ValueError):
        ops.map_stats_update(v, 0, mean, torch.zeros(2, 16, device=device)[:, ::2])
    with pytest.raises(ValueError):
        ops.map_stats_update(v, -1, mean, m2)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_stats_update(v, 0, mean, mean)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_stats_update(v, 0, v[0], m2)


# ---- 2. alignment and row independence -----------------------------------------------------------------------------------------------

def test_map_stats_update_off_a_16_byte_boundary_gives_the_aligned_bits(device):
    from ddpm_ood_amd import ops

    B, P = 4, 2 * 4 * 32 * 32
    v = stats_values(B, P, "near1")
    a, b = torch.from_numpy(v[:B]), torch.from_numpy(v[B:2 * B])

    def two_updates(first, second, mean, m2):
        n = ops.map_stats_update(first, 0, mean, m2)
        ops.map_stats_update(second, n, mean, m2)
        return mean.clone(), m2.clone()

    want = two_updates(a.to(device), b.to(device), torch.empty(P, device=device), torch.empty(P, device=device))
    assert want[0].data_ptr() % 16 == 0
    for who in ("values", "mean", "m2", "all"):
        first, second = (_off_boundary(t, device) if who in ("values", "all") else t.to(device) for t in (a, b))
        mean = _off_boundary(torch.zeros(P), device) if who in ("mean", "all") else torch.empty(P, device=device)
        m2 = _off_boundary(torch.zeros(P), device) if who in ("m2", "all") else torch.empty(P, device=device)
        got = two_updates(first, second, mean, m2)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), who


def test_map_zscore_off_a_16_byte_boundary_and_alone_gives_the_same_bits(device):
    from ddpm_ood_amd import ops

    B, n_t, P1 = 6, 4, 2 * 28 * 28
    g = _g(21)
    v, mean, inv = torch.rand(B, n_t, P1, generator=g), torch.rand(n_t, P1, generator=g), torch.rand(n_t, P1, generator=g) * 40
    want = ops.map_zscore(v.to(device), mean.to(device), inv.to(device))
    assert want.shape == (B, P1) and want.data_ptr() % 16 == 0
    for who in ("values", "mean", "inv_std", "out", "all"):
        ops_in = [(_off_boundary(t, device) if who in (name, "all") else t.to(device))
                  for name, t in (("values", v), ("mean", mean), ("inv_std", inv))]
        out = _off_boundary(torch.zeros(B, P1), device) if who in ("out", "all") else None
        got = ops.map_zscore(*ops_in, out=out)
        assert (out is None or got is out) and _bits(got, want), who
    # a row's bits depend neither on B nor on its place in the batch
    assert _bits(ops.map_zscore(v[3:4].to(device), mean.to(device), inv.to(device)), want[3:4])
    assert _bits(ops.map_zscore(v[2:5].to(device), mean.to(device), inv.to(device))[1:2], want[3:4])


# ---- 3. map_zscore ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P1", [5, 2 * 28 * 28, 2 * 32 * 24])
@pytest.mark.parametrize("n_t", [1, 4])
def test_map_zscore_against_float64(device, n_t, P1):
    """out = w sum_t (v - mean) inv_std, w = fp32(1 / n_t) on both sides.  Per element |err| <= (2 n_t + 1) u L, L = w x the largest
    magnitude among the addends and the partial sums of that element: per t-start the difference (u |v - mean|, carried by inv_std
    to the addend's scale) and the product round, the n_t - 1 additions round at the scale of their partial sums, and the
    weight's product once more."""
    from ddpm_ood_amd import ops

    B = 3
    g = _g(n_t * 10000 + P1)
    v = torch.rand(B, n_t, P1, generator=g)
    mean = torch.rand(n_t, P1, generator=g)
    inv = 1.0 / (0.01 + torch.rand(n_t, P1, generator=g))
    got = ops.map_zscore(v.to(device), mean.to(device), inv.to(device))
    assert got.shape == (B, P1) and got.dtype == torch.float32
    w = float(np.float32(1.0 / n_t))
    addends = (v.double().numpy() - mean.double().numpy()[None]) * inv.double().numpy()[None]
    partial = np.cumsum(addends, axis=1)
    L = w * np.maximum(np.abs(addends).max(axis=1), np.abs(partial).max(axis=1))
    want = ref.zscore(v.numpy(), mean.numpy(), inv.numpy(), weight=w)
    ratio = (np.abs(got.cpu().double().numpy() - want) / (U * L + 1e-300)).max()
    print(f"zscore n_t={n_t} P1={P1}: worst err {ratio:.2f} u L (bound {2 * n_t + 1})")
    assert ratio <= 2 * n_t + 1
    assert float(np.abs(want).max()) > 1.0
    # an explicit weight, into the caller's buffer
    out = torch.empty(B, P1, device=device)
    assert ops.map_zscore(v.to(device), mean.to(device), inv.to(device), weight=1.0, out=out) is out
    assert (np.abs(out.cpu().double().numpy() - want / w) / (U * L / w + 1e-300)).max() <= 2 * n_t + 1


def test_map_zscore_keeps_a_nan_at_its_own_pixel_and_refuses_overlap(device):
    from ddpm_ood_amd import ops

    for P1, at in ((2 * 28 * 28, (1, 2, 777)), (5, (2, 0, 4))):
        g = _g(P1)
        v, mean, inv = torch.rand(3, 4, P1, generator=g), torch.rand(4, P1, generator=g), torch.rand(4, P1, generator=g) + 0.5
        clean = ops.map_zscore(v.to(device), mean.to(device), inv.to(device)).cpu()
        v[at] = float("nan")
        dirty = ops.map_zscore(v.to(device), mean.to(device), inv.to(device)).cpu()
        bad = torch.isnan(dirty)
        assert int(bad.sum()) == 1 and bool(bad[at[0], at[2]])
        assert torch.equal(dirty[~bad], clean[~bad])
    v = torch.rand(2, 3, 8, device=device)
    tables = torch.rand(2, 3, 8, device=device)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_zscore(v, tables[0], tables[1], out=v.view(-1)[:16].view(2, 8))
    with pytest.raises(ValueError, match="aliases"):
        ops.map_zscore(v, tables.view(-1)[:24].view(3, 8), tables[1], out=tables.view(-1)[8:24].view(2, 8))
    with pytest.raises(ValueError):
        ops.map_zscore(v, tables[0][:2], tables[1])
    with pytest.raises(ValueError):
        ops.map_zscore(v, tables[0], tables[1], out=torch.empty(2, 9, device=device))
    with pytest.raises(RuntimeError):
        ops.map_zscore(v.cpu(), tables[0], tables[1])


# ---- 4. map_blur -----------------------------------------------------------------------------------------------------------------------

# radius 8 > H; a ragged tile; H = 1; 28 x 28 at the largest radius; across a tile edge on both axes; radius 1
BLUR_CASES = [(2, 5, 5, 2.0), (1, 7, 12, 1.0), (1, 1, 9, 1.5), (3, 28, 28, 4.0), (2, 33, 31, 4.0), (2, 32, 32, 0.3)]


@pytest.mark.parametrize("N,H,W,sigma", BLUR_CASES, ids=lambda v: str(v))
def test_map_blur_against_float64(device, N, H, W, sigma):
    """The float64 restatement with the SAME fp32 weights.  Per pass 2 r + 1 products and 2 r additions round, below 2 (2 r + 1)
    roundings at the scale of max |in| (the weights are positive and sum to 1 within (2 r + 1) u, so no partial sum exceeds it by
    more); the H pass's error goes through the W pass's weights unamplified: |err| <= 2 x 2 (2 r + 1) u (1 + (2 r + 1) u) max |in|.
    A constant map comes back constant within the same bound (its value times the sum of the fp32 weights)."""
    from ddpm_ood_amd import ops

    radius = int(4 * sigma + 0.5)
    x = torch.randn(N, H, W, generator=_g(H * 100 + W))
    taps32 = ops.gaussian_taps(sigma).astype(np.float32)
    assert len(taps32) == 2 * radius + 1
    got = ops.map_blur(x.to(device), sigma)
    assert got.shape == (N, H, W) and got.dtype == torch.float32
    bound = 4 * (2 * radius + 1) * U * (1 + (2 * radius + 1) * U)
    want = ref.blur(x.numpy(), taps32)
    err = np.abs(got.cpu().double().numpy() - want).max() / float(x.abs().max())
    print(f"blur {N}x{H}x{W} sigma={sigma}: worst err {err / U:.2f} u max|in| (bound {bound / U:.0f})")
    assert err <= bound
    assert _bits(ops.map_blur(x.to(device), taps=torch.from_numpy(taps32).to(device)), got)  # the weights handed over: the same launch
    assert np.abs(want - ref.blur(x.numpy(), ref.gaussian_taps(sigma))).max() <= 1e-6  # (the fp32 weights are scipy's, rounded)
    const = ops.map_blur(torch.full((N, H, W), 0.75, device=device), sigma).cpu().double().numpy()
    assert np.abs(const - 0.75).max() <= bound * 0.75 + (2 * radius + 1) * U * 2 * 0.75


def test_map_blur_radius_zero_is_a_copy_and_what_it_refuses(device):
    from ddpm_ood_amd import ops

    x = torch.randn(3, 33, 31, generator=_g(5))
    x[0, 0, 0], x[1, 5, 7], x[2, 32, 30] = -0.0, float("inf"), 1e-42  # (a signed zero, an infinity, a subnormal)
    got = ops.map_blur(x.to(device), 0.1)  # radius int(0.9) = 0: the single weight 1
    assert _bits(got.cpu(), x)
    assert _bits(ops.map_blur(x.to(device), 0.0).cpu(), x)
    xd = x.to(device)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_blur(xd, 1.0, out=xd)
    with pytest.raises(ValueError, match="aliases"):
        ops.map_blur(xd[:2], 1.0, out=xd.view(-1)[31:31 + 2 * 33 * 31].view(2, 33, 31))
    with pytest.raises(ValueError, match="radius"):
        ops.map_blur(xd, 4.2)  # radius 17
    with pytest.raises(ValueError, match="radius"):
        ops.map_blur(xd, taps=torch.ones(35, device=device))
    with pytest.raises(ValueError):
        ops.map_blur(xd, taps=torch.ones(4, device=device))
    with pytest.raises(ValueError):
        ops.map_blur(xd, 1.0, taps=torch.ones(3, device=device))
    with pytest.raises(ValueError):
        ops.map_blur(xd[0], 1.0)
    with pytest.raises(RuntimeError):
        ops.map_blur(x, 1.0)


# ---- 5. memory bounds ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,P", [(4, 2 * 4 * 32 * 32), (3, 7)], ids=["V4", "V1"])
def test_map_stats_update_stays_inside_its_buffers(device, B, P):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    v = torch.from_numpy(stats_values(B, P, "sq"))

    def first(t):  # n_prev = 0: the tables come from the wrapper's caller as fresh (poisoned, then zeroed) buffers
        mean, m2 = ops.torch.empty((P,), dtype=torch.float32, device=device), ops.torch.empty((P,), dtype=torch.float32, device=device)
        ops.map_stats_update(t["v"][:B], 0, mean, m2)
        return mean, m2

    _bounds(device, dict(v=(v, True)), first)  # same bits from poisoned and zeroed tables: their contents are not read
    mean0, m20 = torch.rand(P, generator=_g(1)), torch.rand(P, generator=_g(2))

    def later(t):
        ops.map_stats_update(t["v"][B:2 * B], B, t["mean"], t["m2"])
        return t["mean"], t["m2"]

    _bounds(device, dict(v=(v, True), mean=(mean0, False), m2=(m20, False)), later)


@pytest.mark.parametrize("P1", [2 * 32 * 32, 5], ids=["V4", "V1"])
def test_map_zscore_stays_inside_its_buffers(device, P1):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    g = _g(31)
    v, mean, inv = torch.rand(3, 4, P1, generator=g), torch.rand(4, P1, generator=g), torch.rand(4, P1, generator=g) + 0.5
    _bounds(device, dict(v=(v, True), mean=(mean, True), inv=(inv, True)), lambda t: ops.map_zscore(t["v"], t["mean"], t["inv"]))


@pytest.mark.parametrize("N,H,W,sigma", [(2, 96, 96, 2.0), (2, 33, 31, 4.0), (1, 1, 9, 1.5)], ids=["interior", "edge", "row"])
def test_map_blur_stays_inside_its_buffers(device, N, H, W, sigma):
    """96 x 96 at radius 8: the middle tile's halo lies wholly inside the image; 33 x 31: every tile is ragged and reflects."""
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    x = torch.randn(N, H, W, generator=_g(H))
    taps = torch.from_numpy(ops.gaussian_taps(sigma).astype(np.float32))
    _bounds(device, dict(x=(x, True)), lambda t: ops.map_blur(t["x"], sigma))  # the wrapper uploads the weights itself
    _bounds(device, dict(x=(x, True), taps=(taps, True)), lambda t: ops.map_blur(t["x"], taps=t["taps"]))


# ---- 6. through the trainer ------------------------------------------------------------------------------------------------------------
# The fixture of tests/test_gpu_anomaly_maps.py section 6: 6 / 6 / 6 synthetic images, batches of 4, t = 10, 330, 650, 970.

FLAG = ("--anomaly_z_maps", "1")
PER_SET = 2 * len(T_STARTS)  # two batches (4 + 2 images), one clamp_mse_ per t-start


def _per_t_maps(calls):
    """float64 [N, n_t, 2, H, W] of one data set from the captured (original, reconstruction) pairs: channel 0 LPIPS, 1 squared
    error, every t-start by itself (tests/anomaly_ref.py + the CPU oracle's features, as ``_expected_maps`` of the maps' tests)."""
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS

    cpu = oracle.LPIPSAlex()
    cpu.load_state_dict(LPIPS().state_dict())
    rows = []
    for s in range(0, len(calls), len(T_STARTS)):
        batch = calls[s:s + len(T_STARTS)]
        assert all(torch.equal(o, batch[0][0]) for o, _ in batch)
        rows.append(torch.stack([torch.stack([anomaly_ref.spatial_lpips(cpu, o, r, normalize=True)[:, 0], anomaly_ref.sqerr_map(o, r)],
                                             dim=1) for o, r in batch], dim=1))
    return torch.cat(rows).numpy()


def _expected(per_t, rel_floor=0.01):
    """The float64 restatement from the three sets' per-t maps: statistics over the validation rows, floor, Z, mean over t."""
    val = per_t["val"]
    mean, std = val.mean(axis=0), val.std(axis=0, ddof=1)
    inv = ref.floor_inv_std(std, rel_floor)
    return mean, std, {name: ref.zscore(per_t[name], mean, inv) for name in per_t if name != "val"}


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic, trainer

    root = tmp_path_factory.mktemp("anomaly_z_maps")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    off = _run(root, "off")
    with _Capture(trainer.ops) as cap:
        on = _run(root, "z", *FLAG)
    assert len(cap.calls) == PER_SET * len(SETS)
    per_t = {name: _per_t_maps(cap.calls[k * PER_SET:(k + 1) * PER_SET]) for k, name in enumerate(SETS)}  # the run's order
    return root, off, on, per_t, _expected(per_t)


def test_nothing_else_moves(runs):
    root, off, on, _, _ = runs
    names = sorted(f"results_{n}.csv" for n in SETS)
    assert sorted(p.name for p in off.iterdir()) == names  # flag off: nothing new
    assert sorted(p.name for p in on.iterdir()) == sorted(names + ["map_stats.npz", "zmaps_in.npz", "zmaps_MNIST.npz"])
    for n in names:
        assert (off / n).read_bytes() == (on / n).read_bytes(), n
    maps = _run(root, "maps", "--anomaly_maps", "1")
    both = _run(root, "maps_z", "--anomaly_maps", "1", *FLAG)
    assert sorted(p.name for p in maps.glob("maps_*")) == sorted(f"maps_{n}.npz" for n in SETS) == sorted(p.name for p in both.glob("maps_*"))
    for n in names:
        assert (off / n).read_bytes() == (both / n).read_bytes() == (maps / n).read_bytes(), n
    for n in SETS:
        a, b = np.load(maps / f"maps_{n}.npz"), np.load(both / f"maps_{n}.npz")
        assert sorted(a.files) == sorted(b.files) == ["filename", "lpips_map", "mse_map", "t"]
        for key in a.files:
            assert np.array_equal(a[key], b[key]), (n, key)
    # the Z-maps do not depend on whether the plain maps are written beside them: the same launches feed them
    for n in ("map_stats.npz", "zmaps_in.npz", "zmaps_MNIST.npz"):
        a, b = np.load(on / n), np.load(both / n)
        for key in a.files:
            assert np.array_equal(a[key], b[key]), (n, key)


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (1.0 + np.abs(want).max()))


def _check_stats(path, want_mean, want_std, what):
    z = np.load(path)
    assert sorted(z.files) == ["channels", "mean", "n", "rel_floor", "std", "t"]
    assert int(z["n"]) == 6 and z["t"].tolist() == T_STARTS and z["channels"].tolist() == ["lpips", "mse"]
    assert float(z["rel_floor"]) == 0.01
    assert z["mean"].shape == (4, 2, 32, 32) == z["std"].shape and z["mean"].dtype == np.float32 == z["std"].dtype
    for c, (name, mean_tol) in enumerate((("lpips", 2e-5), ("mse", 2e-6))):  # the maps' own tolerances (``_close``)
        em, es = _rel(z["mean"][:, c], want_mean[:, c]), _rel(z["std"][:, c], want_std[:, c])
        print(f"{what}: {name} mean err {em:.2e} (bound {mean_tol:.0e}), std err {es:.2e} (bound {STD_TOL[name]:.0e}), "
              f"max std {want_std[:, c].max():.3e}")
        assert em <= mean_tol and es <= STD_TOL[name]
        assert float(want_std[:, c].max()) > 1e-4  # (statistics with something in them)


def _check_zmaps(ood_dir, want_z, sigma, what):
    from ddpm_ood_amd import ops

    taps32 = ops.gaussian_taps(sigma).astype(np.float32)
    for name in ("in", "MNIST"):
        z = np.load(ood_dir / f"zmaps_{name}.npz")
        assert sorted(z.files) == ["filename", "rel_floor", "sigma", "t", "z_lpips_map", "z_mse_map"]
        df = pd.read_csv(ood_dir / f"results_{name}.csv")
        assert [str(s) for s in z["filename"]] == list(dict.fromkeys(df["filename"].astype(str)))  # the CSV's order
        assert z["t"].tolist() == T_STARTS and float(z["sigma"]) == sigma and float(z["rel_floor"]) == 0.01
        for c, key in enumerate(("z_lpips_map", "z_mse_map")):
            assert z[key].shape == (6, 32, 32) and z[key].dtype == np.float32 and np.isfinite(z[key]).all()
            want = want_z[name][:, c]
            if sigma > 0:
                want = ref.blur(want, taps32)
            err, top = _rel(z[key], want), float(np.abs(want).max())
            print(f"{what}: {name} {key} sigma={sigma}: err {err:.2e} (bound {Z_TOL[sigma]:.0e}) max|z| {top:.3f}")
            assert err <= Z_TOL[sigma]
            if name == "MNIST":  # the noise set: the bound means something only on maps with something in them
                assert top > 1.0 and Z_TOL[sigma] * (1.0 + top) < 1e-2 * top


def test_statistics_file_matches_the_float64_restatement(runs):
    _, _, on, _, (want_mean, want_std, _) = runs
    _check_stats(on / "map_stats.npz", want_mean, want_std, "batch 4")


def test_z_maps_match_the_float64_restatement(runs):
    _, _, on, _, (_, _, want_z) = runs
    _check_zmaps(on, want_z, 0.0, "batch 4")


def _with_stats_of(root, src):
    """A fresh ood/ holding only the statistics of an earlier run: what --run_val 0 reads."""
    (root / MODEL / "ood").mkdir(exist_ok=True)
    shutil.copy(src / "map_stats.npz", root / MODEL / "ood" / "map_stats.npz")


def test_statistics_from_the_file_and_smoothing(runs):
    root, _, on, _, (_, _, want_z) = runs
    _with_stats_of(root, on)
    again = _run(root, "from_file", *FLAG, "--run_val", "0")
    assert sorted(p.name for p in again.iterdir()) == sorted(["map_stats.npz", "results_in.csv", "results_MNIST.csv", "zmaps_in.npz",
                                                              "zmaps_MNIST.npz"])
    assert (again / "map_stats.npz").read_bytes() == (on / "map_stats.npz").read_bytes()  # read, not rewritten
    for n in ("zmaps_in.npz", "zmaps_MNIST.npz"):
        a, b = np.load(on / n), np.load(again / n)
        for key in a.files:
            assert np.array_equal(a[key], b[key]), (n, key)
    _with_stats_of(root, on)
    smooth = _run(root, "smooth", *FLAG, "--run_val", "0", "--anomaly_z_sigma", "1.5")
    _check_zmaps(smooth, want_z, 1.5, "batch 4")


def test_missing_or_foreign_statistics_are_refused(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root, _, on, _, _ = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    args = cli.parse_args(_argv(root, *FLAG, "--run_val", "0", "--run_out", "0"))
    with pytest.raises(FileNotFoundError, match="map_stats.npz"):
        Reconstruct(args).reconstruct(args)
    _with_stats_of(root, on)
    args = cli.parse_args(_argv(root, *FLAG, "--run_val", "0", "--run_out", "0", "--inference_skip_factor", "48"))  # t = 10, 490, 970
    with pytest.raises(ValueError, match="t-starts"):
        Reconstruct(args).reconstruct(args)
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_another_batch_size_agrees_within_the_bounds(runs):
    root, _, on, _, (want_mean, want_std, want_z) = runs
    three = _run(root, "batch3", *FLAG, "--batch_size", "3")
    _check_stats(three / "map_stats.npz", want_mean, want_std, "batch 3")
    _check_zmaps(three, want_z, 0.0, "batch 3")
    for n in SETS:  # (the scores do not depend on the batch an image rides in; the CSV's rows are ordered batch by batch)
        a, b = pd.read_csv(on / f"results_{n}.csv"), pd.read_csv(three / f"results_{n}.csv")
        assert sorted(a["filename"].astype(str).unique()) == sorted(b["filename"].astype(str).unique())


def test_two_ranks_on_one_gpu_merge_the_statistics_and_gather_every_z_map(device, runs):
    """reconstruct.py --anomaly_z_maps 1 as two ranks (gloo rendezvous, both on cuda:0): rank 0 holds images 0 2 4, rank 1 images
    1 3 5.  Each rank's validation statistics (3 rows) travel in ONE all_gather and are merged on every rank; the Z-maps of the
    in-set return through gather_rows, and rank 0 alone writes."""
    from test_gpu_dist import ROOT, _launch_ranks

    root, _, on, _, (want_mean, want_std, want_z) = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    _launch_ranks(2, [str(ROOT / "reconstruct.py"), *_argv(root, *FLAG, "--run_out", "0")], root, timeout=600)
    out = root / MODEL / "ood_two_ranks"
    shutil.move(str(root / MODEL / "ood"), str(out))
    assert sorted(p.name for p in out.iterdir()) == ["map_stats.npz", "results_in.csv", "results_val.csv", "zmaps_in.npz"]
    _check_stats(out / "map_stats.npz", want_mean, want_std, "two ranks")
    one, two = np.load(on / "zmaps_in.npz"), np.load(out / "zmaps_in.npz")
    names = [str(s) for s in one["filename"]]
    assert [str(s) for s in two["filename"]] == [names[i] for i in (0, 2, 4, 1, 3, 5)]  # rank-major, as the CSV
    df = pd.read_csv(out / "results_in.csv")
    assert [str(s) for s in two["filename"]] == list(dict.fromkeys(df["filename"].astype(str)))
    for c, key in enumerate(("z_lpips_map", "z_mse_map")):
        for row, name in enumerate(str(s) for s in two["filename"]):  # every row on its image's line
            want = want_z["in"][names.index(name), c]
            err = np.abs(two[key][row] - want).max() / (1.0 + np.abs(want_z["in"][:, c]).max())
            print(f"two ranks: {key} of {name}: err {err:.2e} (bound {Z_TOL[0.0]:.0e})")
            assert err <= Z_TOL[0.0]
            others = [np.abs(two[key][row] - one[key][k]).max() for k in range(6) if names[k] != name]
            assert np.abs(two[key][row] - one[key][names.index(name)]).max() < 0.1 * min(others)  # and on no other image's


def test_command_line_scores_the_runs_files(runs):
    from sklearn.metrics import roc_auc_score

    root, _, on, _, _ = runs
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
    shutil.copytree(on, root / MODEL / "ood")
    try:
        a, b = np.load(on / "zmaps_in.npz"), np.load(on / "zmaps_MNIST.npz")
        base = [sys.executable, str(Path(__file__).resolve().parents[1] / "ood_detection.py"), "--output_dir", str(root),
                "--model_name", MODEL, "--out_data", "MNIST", "--score", "zmap"]
        from ddpm_ood_amd import ood

        want = {}
        for key, reduce in (("z_mse_map", "mean"), ("z_lpips_map", "max"), ("z_lpips_map", "mean"), ("z_mse_map", "max")):
            red = (lambda m: m.reshape(6, -1).astype(np.float64).mean(axis=1)) if reduce == "mean" else \
                (lambda m: m.reshape(6, -1).astype(np.float64).max(axis=1))
            want[key, reduce] = roc_auc_score([0] * 6 + [1] * 6, np.concatenate([red(a[key]), red(b[key])]))
            assert ood.score_zmaps(on / "zmaps_in.npz", on / "zmaps_MNIST.npz", key, reduce)[1] == want[key, reduce]
            print(f"--score zmap {key} {reduce}: AUC {want[key, reduce] * 100:.1f}")
        got = subprocess.run(base + ["--zmap_key", "z_lpips_map", "--zmap_reduce", "max"], capture_output=True, text=True,
                             check=True).stdout  # (one interpreter start: the other choices are checked in process above)
        assert f"AUC for {MODEL} vs MNIST: {want['z_lpips_map', 'max'] * 100:.1f}" in got and "n_in=6 n_out=6" in got
    finally:
        shutil.rmtree(root / MODEL / "ood", ignore_errors=True)


def test_scope_missing_attributes_and_the_counter(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root = runs[0]
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        Reconstruct(cli.parse_args(_argv(root, *FLAG, "--spatial_dimension", "3")))
    with pytest.raises(ValueError, match="--anomaly_z_maps"):
        Reconstruct(cli.parse_args(_argv(root, *FLAG, "--vqvae_checkpoint", str(root / "vqvae.pth"))))
    with pytest.raises(ValueError, match="--anomaly_z_sigma"):
        Reconstruct(cli.parse_args(_argv(root, *FLAG, "--anomaly_z_sigma", "5")))
    args = cli.parse_args(_argv(root))
    for name in ("anomaly_z_maps", "anomaly_z_sigma", "anomaly_z_std_floor"):
        delattr(args, name)  # bench.py and many tests build their Namespace by hand
    rec = Reconstruct(args)
    assert rec.anomaly_z_maps is False and rec.z_sigma == 0.0 and rec.z_std_floor == 0.01
    rec.quiet = True
    rec.get_scores(rec.val_loader, "val", 96)
    assert "zmap_rows_skipped" not in rec.last_stats and rec.last_map_stats is None
    on = Reconstruct(cli.parse_args(_argv(root, *FLAG)))
    on.quiet = True
    on.get_scores(on.val_loader, "val", 96)  # t = 10, 970
    assert on.last_stats["zmap_rows_skipped"] == 0 and on.last_map_stats[0].n == 6 and on.last_map_stats[1] == [10, 970]
    shutil.rmtree(root / MODEL / "ood", ignore_errors=True)
