"""-m gpu: the anomaly maps -- ``ops.sqerr_map``, ``ops.lpips_layer_map`` and ``ops.lpips_map_upsample`` against the
float64 restatement of tests/anomaly_ref.py, the whole spatial LPIPS against the CPU oracle's features, the three kernels inside
guard bands (tests/test_gpu_memory_bounds.py::_bounds), and ``reconstruct.py --anomaly_maps 1`` through the trainer: the CSVs of a
run with the flag are those of a run without it, and ``maps_<name>.npz`` holds what the float64 restatement makes of the very
tensors the run handed to ``clamp_mse_``.

Tolerances (``test_gpu_ops._close``: err <= tol (1 + max |ref|)):
  sqerr_map     2e-6: inputs in [0, 1], C <= 4: the fp32 error of C squared differences and their sum is below (C + 2) 2^-24;
                1e-5 for three accumulated calls (three more roundings of values below 1)
  layer map     1e-5, the project's bound for ``lpips_layer`` (test_gpu_ops.py::test_lpips_layer), whose per-position value it is
  upsample      1e-5: four products and three sums of values below 1 per layer, five layers; the fp32 source coordinate (below
                16, error 2^-20) moves a weight by 1e-6
  whole LPIPS   2e-5, the project's bound for the whole score (test_gpu_ops.py::test_lpips_score_vs_oracle)
"""

import shutil
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import anomaly_ref as ref
from test_gpu_ops import _close

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. sqerr_map -----------------------------------------------------------------------------------------------------------------

SQ_SHAPES = [(3, 1, 32, 32), (2, 3, 5, 7), (1, 2, 4, 6, 5)]  # aligned; odd (the scalar path); 3-D


@pytest.mark.parametrize("shape", SQ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sqerr_map_against_float64(device, shape):
    from ddpm_ood_amd import ops

    g = _g(sum(shape))
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    got = ops.sqerr_map(a.to(device), b.to(device))
    assert got.shape == (shape[0],) + shape[2:] and got.dtype == torch.float32
    _close(got, ref.sqerr_map(a, b), tol=2e-6)
    _close(ops.sqerr_map(a.to(device), b.to(device), 0.25), ref.sqerr_map(a, b, 0.25), tol=2e-6)
    # three t-starts into one buffer with weight 1 / 3, against the same sequence in float64
    acc, want = torch.zeros_like(got), torch.zeros(got.shape, dtype=torch.float64)
    for k in range(3):
        bk = torch.rand(shape, generator=g)
        assert ops.sqerr_map(a.to(device), bk.to(device), 1.0 / 3.0, out=acc) is acc
        want = ref.sqerr_map(a, bk, 1.0 / 3.0, out=want)
    _close(acc, want, tol=1e-5)


def test_sqerr_map_off_a_16_byte_boundary_gives_the_aligned_bits(device):
    from ddpm_ood_amd import ops

    shape = (2, 3, 32, 32)
    g = _g(9)
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    aligned = ops.sqerr_map(a.to(device), b.to(device), 0.5)
    for who in ("a", "b", "both"):
        pa = torch.cat([torch.zeros(1), a.reshape(-1)]).to(device)[1:].view(shape) if who != "b" else a.to(device)
        pb = torch.cat([torch.zeros(1), b.reshape(-1)]).to(device)[1:].view(shape) if who != "a" else b.to(device)
        assert (pa.data_ptr() % 16 == 4) == (who != "b") and (pb.data_ptr() % 16 == 4) == (who != "a")
        assert _bits(ops.sqerr_map(pa, pb, 0.5), aligned), who
    base = torch.rand(2 * 32 * 32 + 1, generator=g).to(device)
    out = base[1:].view(2, 32, 32)  # the map off the boundary, accumulated into
    want = base[1:].view(2, 32, 32).clone()
    ops.sqerr_map(a.to(device), b.to(device), 0.5, out=want)
    ops.sqerr_map(a.to(device), b.to(device), 0.5, out=out)
    assert out.data_ptr() % 16 == 4 and want.data_ptr() % 16 == 0 and _bits(out, want)


def test_sqerr_map_keeps_a_nan_at_its_own_pixel(device):
    from ddpm_ood_amd import ops

    for shape, at in (((2, 3, 5, 7), (1, 2, 3, 4)), ((2, 3, 8, 8), (0, 0, 7, 7))):
        g = _g(3)
        a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
        clean = ops.sqerr_map(a.to(device), b.to(device))
        a[at] = float("nan")
        dirty = ops.sqerr_map(a.to(device), b.to(device)).cpu()
        bad = torch.isnan(dirty)
        assert int(bad.sum()) == 1 and bool(bad[at[0], at[2], at[3]])
        assert torch.equal(dirty[~bad], clean.cpu()[~bad])


def test_sqerr_map_refuses_what_it_cannot_do(device):
    from ddpm_ood_amd import ops

    a = torch.rand(2, 3, 8, 8, device=device)
    with pytest.raises(RuntimeError):
        ops.sqerr_map(a.cpu(), a)
    with pytest.raises(ValueError):
        ops.sqerr_map(a, a[:, :2])
    with pytest.raises(ValueError):
        ops.sqerr_map(a, a, out=torch.zeros(2, 8, 8, 2, device=device)[..., 0])  # not contiguous
    with pytest.raises(ValueError):
        ops.sqerr_map(a, a, out=torch.zeros(2, 8, 9, device=device))
    with pytest.raises(ValueError, match="aliases"):
        ops.sqerr_map(a, a, out=a.view(-1)[: 2 * 64].view(2, 8, 8))


# ---- 2. lpips_layer_map -----------------------------------------------------------------------------------------------------------
# test_lpips_layer's shapes and a rectangular one, then the two sides of the threshold between the kernel's forms (HW = 16 | 17)
LAYER_SHAPES = [(64, 7, 7), (192, 3, 3), (256, 1, 1), (32, 31, 31), (5, 5, 3), (8, 4, 4), (8, 17, 1)]
N_PAIRS = 6


@pytest.fixture(scope="module")
def layer_case(device):
    """The layers' features, their maps in ONE packed buffer (first layer at offset 5, a row longer than the layers need) and
    ops.lpips_layer's accumulated value."""
    from ddpm_ood_amd import ops

    g = _g(6)
    used = sum(h * w for _, h, w in LAYER_SHAPES)
    packed = torch.full((N_PAIRS, used + 16), -7.0, device=device)
    feats, offsets, val, offset = [], [], None, 5
    for C, H, W in LAYER_SHAPES:
        f0, f1 = torch.rand(N_PAIRS, C, H, W, generator=g), torch.rand(N_PAIRS, C, H, W, generator=g)
        f0[1] = 0  # an all-zero feature vector: the 1e-10 guard
        lin = torch.rand(C, generator=g) / C
        feats.append((f0, f1, lin))
        offsets.append(offset)
        assert ops.lpips_layer_map(f0.to(device), f1.to(device), lin.to(device), packed, offset) is packed
        val = ops.lpips_layer(f0.to(device), f1.to(device), lin.to(device), val)
        offset += H * W
    torch.cuda.synchronize()
    return feats, offsets, packed.cpu(), val.cpu(), used


def test_lpips_layer_map_against_float64(layer_case):
    feats, offsets, packed, val, used = layer_case
    means = torch.zeros(N_PAIRS, dtype=torch.float64)
    for (f0, f1, lin), off, (C, H, W) in zip(feats, offsets, LAYER_SHAPES):
        got = packed[:, off:off + H * W].reshape(N_PAIRS, H, W)
        want = ref.lpips_layer_map(f0, f1, lin)
        _close(got, want, tol=1e-5)
        assert float(got[1].min()) > 0  # (the zeroed image: its distance is the other image's own norm)
        means += got.double().mean(dim=(1, 2))
    _close(means, val, tol=1e-5)  # the row means, summed over the layers: what lpips_layer accumulates
    assert torch.all(packed[:, :5] == -7.0) and torch.all(packed[:, 5 + used:] == -7.0)  # nothing outside the layers' slots


def test_lpips_layer_map_of_a_row_does_not_depend_on_its_batch(device, layer_case):
    from ddpm_ood_amd import ops

    feats, offsets, packed, _, _ = layer_case
    for (f0, f1, lin), off, (C, H, W) in zip(feats, offsets, LAYER_SHAPES):
        alone = ops.lpips_layer_map(f0[3:4].to(device), f1[3:4].to(device), lin.to(device))
        assert alone.shape == (1, H * W) and _bits(alone.cpu(), packed[3:4, off:off + H * W]), (C, H, W)


def test_lpips_layer_map_refuses_what_it_cannot_do(device):
    from ddpm_ood_amd import ops

    f = torch.rand(2, 8, 3, 3, device=device)
    lin = torch.rand(8, device=device)
    with pytest.raises(ValueError):
        ops.lpips_layer_map(f, f[:, :4], lin)
    with pytest.raises(ValueError):
        ops.lpips_layer_map(f, f, lin[:4])
    with pytest.raises(ValueError):
        ops.lpips_layer_map(f, f, lin, torch.zeros(2, 12, device=device), 4)  # 4 + 9 > 12
    with pytest.raises(ValueError):
        ops.lpips_layer_map(f, f, lin, torch.zeros(3, 12, device=device), 0)  # rows of another batch
    with pytest.raises(ValueError):
        ops.lpips_layer_map(f, f, lin, torch.zeros(2, 24, device=device)[:, ::2], 0)


# ---- 3. lpips_map_upsample ----------------------------------------------------------------------------------------------------------

UP_CASES = [([(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)], (32, 32)),
            ([(15, 11), (7, 5), (3, 2), (3, 2), (3, 2)], (64, 48)),
            ([(8, 8)], (8, 8)),
            ([(5, 3), (1, 1)], (9, 7))]


def _packed_maps(sizes, n=3, seed=0):
    return torch.rand(n, sum(h * w for h, w in sizes) + 5, generator=_g(seed + len(sizes)))


@pytest.mark.parametrize("sizes,full", UP_CASES, ids=lambda v: "-".join("x".join(map(str, s)) for s in v) if isinstance(v, list) else None)
def test_lpips_map_upsample_against_float64(device, sizes, full):
    from ddpm_ood_amd import ops

    maps = _packed_maps(sizes)
    got = ops.lpips_map_upsample(maps.to(device), sizes, full)
    assert got.shape == (3,) + full and got.dtype == torch.float32
    _close(got, ref.upsample_sum(maps, sizes, full), tol=1e-5)
    if sizes == [(8, 8)]:
        assert torch.equal(got.cpu(), maps[:, :64].reshape(3, 8, 8))  # the identity is an exact copy
    # weight and accumulate: three calls with weight 1 / 3 into one buffer, against the same sequence in float64
    acc, want = torch.zeros_like(got), torch.zeros(got.shape, dtype=torch.float64)
    for k in range(3):
        mk = _packed_maps(sizes, seed=10 + k)
        assert ops.lpips_map_upsample(mk.to(device), sizes, full, weight=1.0 / 3.0, out=acc) is acc
        want = ref.upsample_sum(mk, sizes, full, weight=1.0 / 3.0, out=want)
    _close(acc, want, tol=1e-5)


def test_lpips_map_upsample_window_is_a_slice_of_the_full_result(device):
    from ddpm_ood_amd import ops

    sizes, full = UP_CASES[0]
    maps = _packed_maps(sizes).to(device)
    whole = ops.lpips_map_upsample(maps, sizes, full, weight=0.25)
    crop = ops.lpips_map_upsample(maps, sizes, full, window=(2, 2, 28, 28), weight=0.25)
    assert crop.shape == (3, 28, 28) and _bits(crop, whole[:, 2:30, 2:30])
    sizes, full = UP_CASES[3]
    maps = _packed_maps(sizes).to(device)
    whole = ops.lpips_map_upsample(maps, sizes, full)
    assert _bits(ops.lpips_map_upsample(maps, sizes, full, window=(4, 1, 5, 6)), whole[:, 4:9, 1:7])  # up to the far corner
    _close(whole[:, 4:9, 1:7], ref.upsample_sum(maps.cpu(), sizes, full, window=(4, 1, 5, 6)), tol=1e-5)


def test_a_one_by_one_layer_alone_is_a_constant_map_of_its_value(device):
    from ddpm_ood_amd import ops

    maps = torch.rand(4, 3, generator=_g(1))
    for full in ((32, 32), (9, 7)):
        got = ops.lpips_map_upsample(maps.to(device), [(1, 1)], full).cpu()
        assert torch.equal(got, maps[:, :1, None].expand(4, *full))


def test_lpips_map_upsample_refuses_what_it_cannot_do(device):
    from ddpm_ood_amd import ops

    maps = torch.rand(2, 61, device=device)
    sizes = UP_CASES[0][0]
    for bad_sizes in ([], sizes + [(1, 1)], [(7, 7), (0, 3)], [(8, 8)]):  # no layer, six, an empty one, more than the row holds
        with pytest.raises(ValueError):
            ops.lpips_map_upsample(maps, bad_sizes, (32, 32))
    for window in ((0, 0, 33, 32), (5, 5, 28, 28), (-1, 0, 8, 8), (0, 0, 0, 8)):
        with pytest.raises(ValueError):
            ops.lpips_map_upsample(maps, sizes, (32, 32), window=window)
    with pytest.raises(ValueError):
        ops.lpips_map_upsample(maps, sizes, (32, 32), out=torch.zeros(2, 32, 31, device=device))
    with pytest.raises(ValueError):
        ops.lpips_map_upsample(maps, sizes, (32, 32), out=torch.zeros(2, 32, 64, device=device)[..., ::2])


# ---- 4. the whole spatial LPIPS -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(7, 1, 32, 32), (3, 3, 64, 48)], ids=lambda s: "x".join(map(str, s)))
def test_spatial_lpips_vs_oracle_features(device, shape):
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS

    g = _g(shape[2])
    x, y = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)
    hip = LPIPS(seed=3, spatial=True)
    cpu = oracle.LPIPSAlex()
    cpu.load_state_dict(hip.state_dict())
    want = ref.spatial_lpips(cpu, x, y, normalize=True)
    hip = hip.to(device)
    got = hip(x.to(device), y.to(device), normalize=True)
    assert got.shape == (shape[0], 1) + shape[2:]  # [N, 1, H, W]: the parent commit returned [N, 1, 1, 1] here
    _close(got, want, tol=2e-5)
    plain = LPIPS(seed=3).to(device)(x.to(device), y.to(device), normalize=True)
    val, amap = hip.forward_with_map(x.to(device), y.to(device), normalize=True)
    assert val.shape == (shape[0], 1, 1, 1) and torch.equal(val, plain)  # the score's own launches: the same bits
    assert _bits(amap, got)
    # a window of the map, weighted into a caller's buffer (how the trainer averages the t-starts)
    acc = torch.ones(shape[0], shape[2] - 4, shape[3] - 4, device=device)
    _, part = hip.forward_with_map(x.to(device), y.to(device), normalize=True, weight=0.5, out=acc,
                                   window=(2, 2, shape[2] - 4, shape[3] - 4))
    assert part.shape == (shape[0], 1, shape[2] - 4, shape[3] - 4) and part.data_ptr() == acc.data_ptr()
    _close(acc, 1.0 + 0.5 * want[:, 0, 2:-2, 2:-2], tol=2e-5)


def test_perceptual_loss_forwards_spatial(device):
    from ddpm_ood_amd.perceptual import LPIPS, PerceptualLoss

    g = _g(2)
    x, y = torch.rand(2, 1, 32, 32, generator=g).to(device), torch.rand(2, 1, 32, 32, generator=g).to(device)
    pl = PerceptualLoss(2, spatial=True).to(device)
    got = pl(x, y)
    assert got.shape == (2, 1, 32, 32)
    assert _bits(got, LPIPS(spatial=True).to(device)(x, y, normalize=True))
    plain = PerceptualLoss(2).to(device)
    assert plain(x, y).shape == (2, 1, 1, 1)  # spatial=False: what it always was
    val, amap = plain.forward_with_map(x, y)
    assert torch.equal(val, plain(x, y)) and _bits(amap, got)


def test_constructor_and_empty_pyramid_are_refused(device):
    from ddpm_ood_amd.perceptual import LPIPS, PerceptualLoss

    with pytest.raises(NotImplementedError, match="2.5-D maps"):
        PerceptualLoss(3, spatial=True)
    x = torch.rand(1, 1, 32, 24, device=device)
    with pytest.raises(ValueError, match="empty AlexNet layer"):
        LPIPS(spatial=True).to(device)(x, x)
    with pytest.raises(ValueError, match="empty AlexNet layer"):
        LPIPS().to(device).forward_with_map(x, x)


# ---- 5. memory bounds -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 1, 32, 32), (2, 3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_sqerr_map_stays_inside_its_buffers(device, shape):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    g = _g(11)
    a, b = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    _bounds(device, dict(a=(a, True), b=(b, True)), lambda t: ops.sqerr_map(t["a"], t["b"], 0.5))
    acc = torch.rand((shape[0],) + shape[2:], generator=g)
    _bounds(device, dict(a=(a, True), b=(b, True), acc=(acc, False)), lambda t: ops.sqerr_map(t["a"], t["b"], 0.5, out=t["acc"]))


@pytest.mark.parametrize("C,H,W", [(64, 8, 8), (64, 7, 9), (256, 1, 1), (5, 5, 3)])
def test_lpips_layer_map_stays_inside_its_buffers(device, C, H, W):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    g = _g(12)
    f0, f1 = torch.rand(3, C, H, W, generator=g), torch.rand(3, C, H, W, generator=g)
    f0[1] = 0
    lin = torch.rand(C, generator=g) / C
    feats = dict(f0=(f0, True), f1=(f1, True), lin=(lin, True))
    _bounds(device, feats, lambda t: ops.lpips_layer_map(t["f0"], t["f1"], t["lin"]))
    row = torch.rand(3, H * W + 7, generator=g)  # a pre-filled packed row, the layer at offset 3
    _bounds(device, dict(row=(row, False), **feats), lambda t: ops.lpips_layer_map(t["f0"], t["f1"], t["lin"], t["row"], 3))


@pytest.mark.parametrize("case", [0, 3])
def test_lpips_map_upsample_stays_inside_its_buffers(device, case):
    from test_gpu_memory_bounds import _bounds

    from ddpm_ood_amd import ops

    sizes, full = UP_CASES[case]
    window = (2, 2, 28, 28) if case == 0 else (4, 1, 5, 6)
    maps = _packed_maps(sizes)
    _bounds(device, dict(maps=(maps, True)), lambda t: ops.lpips_map_upsample(t["maps"], sizes, full))
    _bounds(device, dict(maps=(maps, True)), lambda t: ops.lpips_map_upsample(t["maps"], sizes, full, window=window, weight=0.5))
    acc = torch.rand((3,) + window[2:], generator=_g(13))
    _bounds(device, dict(maps=(maps, True), acc=(acc, False)),
            lambda t: ops.lpips_map_upsample(t["maps"], sizes, full, window=window, weight=0.5, out=t["acc"]))


# ---- 6. through the trainer ---------------------------------------------------------------------------------------------------------------
# reconstruct.py's parser and trainer in this process (no interpreter start, no second GPU context per run): the set-up of
# tests/test_gpu_cli.py, 6 images in batches of 4 and every 32nd of the 100 timesteps as a start -> t = 10, 330, 650, 970.

MODEL = "fashionmnist_maps"
SETS = {"val": "synthetic:blobs:n=6:seed=10", "in": "synthetic:blobs:n=6:seed=11", "MNIST": "synthetic:noise:n=6:seed=12:name=MNIST"}
T_STARTS = [10, 330, 650, 970]


def _argv(root, *extra):
    return ["--output_dir", str(root), "--model_name", MODEL, "--is_grayscale", "1", "--validation_ids", SETS["val"],
            "--in_ids", SETS["in"], "--out_ids", SETS["MNIST"], "--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015",
            "--beta_end", "0.0195", "--batch_size", "4", "--inference_skip_factor", "32", *extra]


def _run(root, tag, *extra):
    """One reconstruct.py run on the checkpoint under `root`; its ood directory is kept as ood_<tag>."""
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    args = cli.parse_args(_argv(root, *extra))
    Reconstruct(args).reconstruct(args)
    kept = root / MODEL / f"ood_{tag}"
    shutil.move(str(root / MODEL / "ood"), str(kept))
    return kept


class _Capture:
    """ops.clamp_mse_ as the trainer calls it, keeping a copy of (images_original, the clamped reconstruction) per t-start."""

    def __init__(self, ops):
        self.ops, self.real, self.calls = ops, ops.clamp_mse_, []

    def __enter__(self):
        def spy(orig, recon, b_scale=1.0):
            mse = self.real(orig, recon, b_scale)
            self.calls.append((orig.detach().cpu().clone(), recon.detach().cpu().clone()))
            return mse

        self.ops.clamp_mse_ = spy
        return self

    def __exit__(self, *exc):
        self.ops.clamp_mse_ = self.real


@pytest.fixture(scope="module")
def runs(device, tmp_path_factory):
    from ddpm_ood_amd import synthetic, trainer

    root = tmp_path_factory.mktemp("anomaly_maps")
    synthetic.write_checkpoint(root / MODEL, "small", 1, seed=1)
    off = _run(root, "off", "--anomaly_maps", "0")
    with _Capture(trainer.ops) as cap:
        on = _run(root, "on", "--anomaly_maps", "1")
    return root, off, on, cap.calls


def test_the_flag_leaves_every_csv_as_it_was(runs):
    _, off, on, _ = runs
    names = sorted(p.name for p in off.glob("results_*.csv"))
    assert names == sorted(f"results_{n}.csv" for n in SETS) == sorted(p.name for p in on.glob("results_*.csv"))
    for n in names:
        a, b = pd.read_csv(off / n), pd.read_csv(on / n)
        assert len(a) == 6 * 4 and a.equals(b), n
        assert (off / n).read_bytes() == (on / n).read_bytes(), n
    assert not list(off.glob("maps_*"))  # flag off: no file
    assert sorted(p.name for p in on.glob("maps_*")) == sorted(f"maps_{n}.npz" for n in SETS)


def _expected_maps(calls, pad=0):
    """float64 maps of one data set from the captured (original, reconstruction) pairs: per batch the mean over its t-starts."""
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS

    cpu = oracle.LPIPSAlex()
    cpu.load_state_dict(LPIPS().state_dict())  # the trainer's LPIPS without --lpips_weights: the seeded default
    lp, se = [], []
    for s in range(0, len(calls), len(T_STARTS)):
        batch = calls[s:s + len(T_STARTS)]
        assert all(torch.equal(o, batch[0][0]) for o, _ in batch)  # one batch: the same originals at every t-start
        se.append(sum(ref.sqerr_map(o, r) for o, r in batch) / len(batch))
        full = [ref.spatial_lpips(cpu, F.pad(o, (pad,) * 4), F.pad(r, (pad,) * 4), normalize=True)[:, 0] for o, r in batch]
        full = sum(full) / len(batch)
        lp.append(full[:, pad:full.shape[1] - pad, pad:full.shape[2] - pad])
    return torch.cat(lp), torch.cat(se)


def test_maps_file_matches_the_csv_and_the_float64_restatement(runs):
    _, _, on, calls = runs
    per_set = 2 * len(T_STARTS)  # two batches (4 + 2 images), one clamp_mse_ per t-start
    assert len(calls) == per_set * len(SETS)
    for k, name in enumerate(SETS):  # the run's order: val, in, out
        df = pd.read_csv(on / f"results_{name}.csv")
        z = np.load(on / f"maps_{name}.npz")
        assert sorted(z.files) == ["filename", "lpips_map", "mse_map", "t"]
        stems = list(dict.fromkeys(df["filename"].astype(str)))
        assert len(stems) == 6 and [str(s) for s in z["filename"]] == stems  # the CSV's order of first appearance
        assert z["t"].tolist() == T_STARTS == sorted(df["t"].unique())
        for key in ("lpips_map", "mse_map"):
            assert z[key].shape == (6, 32, 32) and z[key].dtype == np.float32
            assert np.isfinite(z[key]).all() and (z[key] >= 0).all()
        # each image's map averages to the mean over t of its CSV rows: file order, t-weighting and CSV agree
        csv_mse = torch.tensor([df[df["filename"].astype(str) == s]["mse"].mean() for s in stems], dtype=torch.float64)
        _close(torch.from_numpy(z["mse_map"]).double().mean(dim=(1, 2)), csv_mse, tol=1e-6)
        want_lp, want_se = _expected_maps(calls[k * per_set:(k + 1) * per_set])
        _close(torch.from_numpy(z["mse_map"]), want_se, tol=2e-6)
        _close(torch.from_numpy(z["lpips_map"]), want_lp, tol=2e-5)
        assert float(want_se.max()) > 1e-3 and float(want_lp.max()) > 1e-3  # (maps with something in them)


def test_28_pixel_images_are_padded_for_lpips_and_cropped_back(device, runs):
    from ddpm_ood_amd import trainer

    root = runs[0]
    with _Capture(trainer.ops) as cap:
        out = _run(root, "28", "--anomaly_maps", "1", "--validation_ids", "synthetic:blobs:n=3:size=28:seed=4", "--run_in", "0",
                   "--run_out", "0")
    assert len(cap.calls) == len(T_STARTS) and cap.calls[0][0].shape == (3, 1, 28, 28)
    z = np.load(out / "maps_val.npz")
    assert z["lpips_map"].shape == (3, 28, 28) == z["mse_map"].shape and z["t"].tolist() == T_STARTS
    want_lp, want_se = _expected_maps(cap.calls, pad=2)
    _close(torch.from_numpy(z["mse_map"]), want_se, tol=2e-6)
    _close(torch.from_numpy(z["lpips_map"]), want_lp, tol=2e-5)
    df = pd.read_csv(out / "results_val.csv")
    csv_mse = torch.tensor([df[df["filename"].astype(str) == str(s)]["mse"].mean() for s in z["filename"]], dtype=torch.float64)
    _close(torch.from_numpy(z["mse_map"]).double().mean(dim=(1, 2)), csv_mse, tol=1e-6)


def test_two_ranks_on_one_gpu_gather_every_map_to_its_image(device, runs):
    """reconstruct.py --anomaly_maps 1 as two ranks (gloo rendezvous, both on cuda:0: tests/test_gpu_dist.py): rank 0 holds images
    0 2 4, rank 1 images 1 3 5; the maps return through gather_rows and rank 0 writes them in the CSV's rank-major order.  Every
    image has its own MSE, so a map that averages to its CSV rows sits on the right line."""
    from test_gpu_dist import ROOT, _launch_ranks

    root = runs[0]
    argv = [str(ROOT / "reconstruct.py"), *_argv(root, "--anomaly_maps", "1", "--run_in", "0", "--run_out", "0")]
    _launch_ranks(2, argv, root, timeout=600)
    out = root / MODEL / "ood_two_ranks"
    shutil.move(str(root / MODEL / "ood"), str(out))
    assert sorted(p.name for p in out.iterdir()) == ["maps_val.npz", "results_val.csv"]  # rank 0 alone writes
    df = pd.read_csv(out / "results_val.csv")
    z = np.load(out / "maps_val.npz")
    stems = list(dict.fromkeys(df["filename"].astype(str)))
    one_rank = [str(s) for s in np.load(runs[2] / "maps_val.npz")["filename"]]
    assert stems == [one_rank[i] for i in (0, 2, 4, 1, 3, 5)] and [str(s) for s in z["filename"]] == stems
    assert z["lpips_map"].shape == (6, 32, 32) == z["mse_map"].shape and z["t"].tolist() == T_STARTS
    csv_mse = torch.tensor([df[df["filename"].astype(str) == s]["mse"].mean() for s in stems], dtype=torch.float64)
    assert float((csv_mse[:, None] - csv_mse[None, :]).abs().add(torch.eye(6)).min()) > 1e-5  # (distinct images, distinct MSEs)
    _close(torch.from_numpy(z["mse_map"]).double().mean(dim=(1, 2)), csv_mse, tol=1e-6)
    csv_lp = torch.tensor([df[df["filename"].astype(str) == s]["perceptual_difference"].mean() for s in stems], dtype=torch.float64)
    assert float(csv_lp.min()) > 0 and np.isfinite(z["lpips_map"]).all() and (z["lpips_map"] >= 0).all()


def test_scope_and_the_missing_attribute(device, runs):
    import reconstruct as cli
    from ddpm_ood_amd.trainer import Reconstruct

    root = runs[0]
    with pytest.raises(ValueError, match="2-D pixel-space models"):
        Reconstruct(cli.parse_args(_argv(root, "--anomaly_maps", "1", "--spatial_dimension", "3")))
    with pytest.raises(ValueError, match="2-D pixel-space models"):
        Reconstruct(cli.parse_args(_argv(root, "--anomaly_maps", "1", "--vqvae_checkpoint", str(root / "vqvae.pth"))))
    args = cli.parse_args(_argv(root))
    assert args.anomaly_maps == 0
    delattr(args, "anomaly_maps")  # bench.py and many tests build their Namespace by hand
    assert Reconstruct(args).anomaly_maps is False
