"""CPU: the host side of calibration and segmentation of volumes -- the flags, their defaults and every refusal from
the Namespace alone, the budget formulas against the library's size function, the median's selection network on all 2^27 zero-one
inputs, ``score_segments`` on a file of volumes, the restatement of the GPU tests against scipy, and the refusals of the new entry
points (a refusal launches nothing, so it needs no device)."""

import argparse
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import scipy.ndimage

import voxel_segment_ref as ref

ROOT = Path(__file__).resolve().parents[1]
BASE = dict(spatial_dimension=3, vqvae_checkpoint=None, anomaly_volume_z_maps=1, out_ids="a.csv,b.csv", run_out=1)
SEG = dict(BASE, voxel_segment=1)
CAL = dict(BASE, voxel_calibrate_fpr="0.05,0.01")


def _settings(**kw):
    from ddpm_ood_amd.voxel_passes import VoxelSettings

    return VoxelSettings.from_args(argparse.Namespace(**kw))


# ---- flags ------------------------------------------------------------------------------------------------------------------------

def test_flags_parse_with_their_defaults():
    import reconstruct as cli
    from ddpm_ood_amd.map_passes import MapPipeline, MapSettings
    from ddpm_ood_amd.voxel_passes import VoxelSettings

    args = cli.parse_args([])
    assert (args.voxel_calibrate_fpr, args.voxel_calibrate_budget_gb, args.voxel_segment, args.voxel_median, args.voxel_min_component) \
        == (None, 8.0, 0, 3, 8)
    assert VoxelSettings.from_args(args) == VoxelSettings() and not VoxelSettings().active
    args = cli.parse_args(["--spatial_dimension", "3", "--anomaly_volume_z_maps", "1", "--voxel_calibrate_fpr", "0.05,0.01,0.001",
                           "--voxel_calibrate_budget_gb", "2", "--voxel_segment", "1", "--voxel_median", "1", "--voxel_min_component", "20",
                           "--voxel_connectivity", "6", "--pixel_thresholds", "1.5,2", "--pixel_bins", "64", "--pixel_range", "-4", "12"])
    s = VoxelSettings.from_args(args)
    assert s.active and s.calibrate and s.segment and not s.metrics and not s.regions and s.masks is None
    assert (s.cal_fprs, s.cal_budget, s.median, s.min_component, s.connectivity) == ([0.05, 0.01, 0.001], 2 << 30, 1, 20, 6)
    assert (s.lo, s.hi, s.bins, s.thresholds) == (-4.0, 12.0, 64, [1.5, 2.0]) and s.pro_fpr is None
    settings = MapSettings.from_args(args)
    assert not settings.px_calibrate and not settings.pixel_segment  # the 2-D settings stay what the command line said
    pipeline = MapPipeline(settings, "cpu", ".", voxel=s)
    assert pipeline.voxel is s and pipeline.layout is None and pipeline.calibrating and pipeline.seg_T == 2 + 3
    assert [n for n, _ in pipeline.seg_layout.segments] == ["pixels", "components", "removed", "regions", "mask_pixels"]
    assert pipeline.cal_grid == ("--voxel_calibrate_fpr", "--voxel_calibrate_budget_gb", -4.0, 12.0, 64, [0.05, 0.01, 0.001], 2 << 30)
    seg = _settings(**SEG)
    assert (seg.median, seg.min_component, seg.connectivity, seg.thresholds) == (3, 8, 26, [2.0, 3.0, 4.0]) and not seg.calibrate
    assert seg.lo is None and seg.bins is None
    cal = _settings(**CAL)
    assert (cal.lo, cal.hi, cal.bins, cal.cal_budget) == (-16.0, 48.0, 4096, 8 << 30) and cal.thresholds is None and cal.connectivity is None
    # with the metrics: the calibrated counts ride in the row RowLayout describes
    full = _settings(**dict(CAL, voxel_metrics=1, voxel_regions=1, voxel_segment=1))
    pipeline = MapPipeline(MapSettings(), "cpu", ".", voxel=full)
    assert [n for n, _ in pipeline.layout.segments] == ["counts", "mask_pixels", "components", "regions", "calibrated"]
    assert dict(pipeline.layout.segments)["calibrated"] == (2, 2, 2, 3) and pipeline.seg_T == 3 + 2
    plain = MapPipeline(MapSettings(), "cpu", ".", voxel=_settings(**dict(CAL, voxel_metrics=1)))
    assert dict(plain.layout.segments)["calibrated"] == (1, 2, 2, 3)


def test_every_refusal_comes_from_the_namespace_alone():
    from ddpm_ood_amd.trainer import Reconstruct

    cases = [
        (dict(SEG, spatial_dimension=2), "--spatial_dimension 3"),                       # 2-D
        (dict(CAL, spatial_dimension=2), "--spatial_dimension 3"),
        (dict(SEG, anomaly_volume_z_maps=0), "--anomaly_volume_z_maps 1"),               # no Z-maps
        (dict(CAL, anomaly_volume_z_maps=0), "--anomaly_volume_z_maps 1"),
        (dict(SEG, voxel_median=5), "--voxel_median"),                                   # a median other than 1 / 3
        (dict(SEG, voxel_median=2), "--voxel_median"),
        (dict(SEG, voxel_median="3.5"), "--voxel_median"),
        (dict(SEG, voxel_min_component=0), "--voxel_min_component"),                     # a minimum size out of range
        (dict(SEG, voxel_min_component=2 ** 31), "--voxel_min_component"),
        (dict(SEG, voxel_min_component=-3), "--voxel_min_component"),
        (dict(SEG, voxel_connectivity=8), "--voxel_connectivity"),
        (dict(SEG, pixel_thresholds="1,2,3,4,5,6,7,8,9"), "--pixel_thresholds"),
        (dict(SEG, pixel_thresholds="1,inf"), "--pixel_thresholds"),
        (dict(BASE, voxel_calibrate_fpr="0.0"), "--voxel_calibrate_fpr"),                # rates outside (0, 1)
        (dict(BASE, voxel_calibrate_fpr="0.5,1.0"), "--voxel_calibrate_fpr"),
        (dict(BASE, voxel_calibrate_fpr="0.1,a"), "--voxel_calibrate_fpr"),
        (dict(BASE, voxel_calibrate_fpr=",".join(["0.1"] * 9)), "--voxel_calibrate_fpr"),  # more than 8
        (dict(CAL, voxel_calibrate_budget_gb=0), "--voxel_calibrate_budget_gb"),         # a non-positive budget
        (dict(CAL, voxel_calibrate_budget_gb=-1.0), "--voxel_calibrate_budget_gb"),
        (dict(CAL, pixel_bins=9000), "--pixel_bins"),
        (dict(SEG, image_size=1291), "2^31"),                                            # 1291^3 >= 2^31
        (dict(CAL, image_roi=(2048, 1024, 1024)), "2^31"),
        (dict(SEG, pixel_metrics=1), "--pixel_metrics"),                                 # beside a 2-D pixel flag
        (dict(SEG, pixel_segment=1), "--pixel_segment"),
        (dict(CAL, pixel_calibrate_fpr="0.05"), "--pixel_calibrate_fpr"),
        (dict(CAL, pixel_regions=1), "--pixel_regions"),
    ]
    for kw, match in cases:
        with pytest.raises(ValueError, match=re.escape(match)) as e:
            _settings(**kw)
        assert "--voxel_" in str(e.value), str(e.value)  # named by a voxel flag
        with pytest.raises(ValueError):  # the constructor runs the check before any device, library or checkpoint
            Reconstruct(argparse.Namespace(**kw))
    assert _settings(**dict(SEG, voxel_min_component=2 ** 31 - 1)).min_component == 2 ** 31 - 1
    assert _settings(**dict(SEG, voxel_median=1)).median == 1 and _settings(**dict(SEG, image_size=1290)).segment
    # the two existing messages now point to the counterpart
    from ddpm_ood_amd.map_passes import MapSettings

    with pytest.raises(ValueError, match="is not built for volumes") as e:
        MapSettings.from_args(argparse.Namespace(**dict(SEG, pixel_segment=1)))
    assert "--pixel_segment" in str(e.value) and "--voxel_segment" in str(e.value)
    with pytest.raises(ValueError, match="--voxel_calibrate_fpr") as e:
        _settings(**dict(SEG, pixel_calibrate_fpr="0.05"))
    assert "--pixel_calibrate_fpr" in str(e.value) and "not built" not in str(e.value)


# ---- budgets ----------------------------------------------------------------------------------------------------------------------

def test_the_budgets_cover_the_new_steps():
    from ddpm_ood_amd import ops, pixel_metrics as pm, voxel_passes as vp

    for (b, d, h, w, k) in ((1, 1, 1, 1, 1), (2, 3, 5, 7, 3), (3, 17, 33, 65, 8), (1, 128, 128, 128, 3), (4, 1, 128, 128, 5)):
        assert vp.segment_scratch_bytes(b, k, d * h * w) == ops.map_segment3d_scratch_bytes(b, d, h, w, k) > 0
    assert ops.map_segment3d_scratch_bytes(1, 2048, 1024, 1024, 3) == 0 and ops.map_segment3d_scratch_bytes(1, 4, 4, 4, 9) == 0
    assert ops.map_segment3d_scratch_bytes(0, 4, 4, 4, 1) == 0
    B, n_t, extent, P = 2, 25, (128, 128, 128), 128 ** 3
    seg = _settings(**SEG)
    mine = vp.batch_bytes(B, extent, seg)
    # the median's buffer, a channel's copy, the scratch of three thresholded maps (forest and sizes), seg, the mask and its labels
    assert mine >= 2 * B * P * 4 + 4 * B * P + vp.segment_scratch_bytes(B, 3, P) + 2 * B * 3 * P + B * P * 5 + vp.label_scratch_bytes(B, P)
    assert mine >= 4 * B * vp.segment_words(3, P) and vp.segment_words(3, P) == 2 * 3 * P // 16 and vp.segment_words(1, 9) == 2
    assert vp.batch_bytes(B, extent, _settings(**dict(SEG, voxel_median=1))) == mine - 2 * B * P * 4
    both = _settings(**dict(SEG, voxel_metrics=1, voxel_regions=1))
    assert vp.batch_bytes(B, extent, both) == vp.batch_bytes(B, extent, _settings(**dict(BASE, voxel_metrics=1, voxel_regions=1))) \
        + mine - (B * P * 5 + 4 * B + vp.label_scratch_bytes(B, P))  # the labels of count_batch are reused
    cal = _settings(**dict(CAL, voxel_metrics=1, voxel_regions=1))
    assert vp.batch_bytes(B, extent, cal) == vp.batch_bytes(B, extent, _settings(**dict(BASE, voxel_metrics=1, voxel_regions=1))) \
        + 2 * 2 * 12 * B * 2 + vp.counts_scratch_bytes(B, 2, P)
    assert vp.batch_bytes(B, extent, _settings(**CAL)) == 0  # the calibration alone adds nothing to a batch of another pass
    maps = B * n_t * 2 * P * 4
    assert vp.check_budget(B, n_t, extent, seg, 16 << 30) == maps + mine
    with pytest.raises(ValueError, match=re.escape("--anomaly_volume_budget_gb")) as e:
        vp.check_budget(B, n_t, extent, seg, maps + mine - 1)
    assert "--voxel_segment 1" in str(e.value) and "128 x 128 x 128" in str(e.value)
    # the retained validation rows: any extent, the 2-D result and message unchanged
    assert pm.check_budget(8, 2, 32, 32, 8 << 30) == 8 * 2 * 2 * 32 * 32 * 4
    assert pm.check_budget(4, 25, 128, 128, 128, 8 << 30) == 4 * 25 * 2 * P * 4
    with pytest.raises(ValueError, match=re.escape("8 x 2 x 2 x 32 x 32 fp32")) as e:
        pm.check_budget(8, 2, 32, 32, 131071)
    assert "--pixel_calibrate_fpr" in str(e.value) and "--pixel_calibrate_budget_gb" in str(e.value)
    with pytest.raises(ValueError, match=re.escape("100 x 25 x 2 x 128 x 128 x 128 fp32")) as e:
        pm.check_budget(100, 25, 128, 128, 128, 8 << 30, flags=(vp.CALIBRATE_FLAG, vp.BUDGET_FLAG))
    assert "--voxel_calibrate_fpr" in str(e.value) and "--voxel_calibrate_budget_gb" in str(e.value) and "--pixel_" not in str(e.value)


# ---- the median's selection network -------------------------------------------------------------------------------------------------

def test_the_selection_network_selects_the_median_of_all_zero_one_inputs(tmp_path):
    """tools/median_zero_one.cpp instantiates the kernels' own template (csrc/median_common.h) on bit-sliced words: 2^9 inputs of
    the 2-D window, 2^27 of the 3-D one."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None and Path("/opt/rocm/llvm/bin/clang++").exists():
        cxx = "/opt/rocm/llvm/bin/clang++"
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "median_zero_one"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", str(ROOT / "ddpm_ood_amd" / "csrc"), str(ROOT / "tools" / "median_zero_one.cpp"), "-o",
                    str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert got.returncode == 0 and got.stdout.split() == ["ok", "512", "ok", str(2 ** 27)], got.stdout
    # the kernels use that very template, and the shared pieces are shared, not copied
    csrc = ROOT / "ddpm_ood_amd" / "csrc"
    for name in ("segment.hip", "segment3d.hip"):
        text = (csrc / name).read_text()
        assert '#include "median_common.h"' in text and "select_median<" in text and "uint32_t med_key" not in text
    for name in ("regions3d.hip", "segment3d.hip"):
        text = (csrc / name).read_text()
        assert '#include "regions3d_common.h"' in text and "void g3_union" not in text and "cc3_union_kernel(Src src" not in text
    common = (csrc / "regions3d_common.h").read_text()
    assert all(k in common for k in ("g3_find", "g3_union", "r3_block_sum", "r3_block_scan", "struct SrcThr", "cc3_init_kernel",
                                     "cc3_union_kernel", "cc3_flatten_kernel", "launch_cc3_link", "check_volume"))


# ---- the reference of the GPU tests -------------------------------------------------------------------------------------------------

def test_the_sorted_windows_equal_scipy_on_nan_free_volumes():
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 1), (1, 1, 5), (2, 3, 4), (5, 1, 7), (9, 10, 11)):
        for v in (rng.standard_normal(shape).astype(np.float32), rng.integers(-2, 3, size=shape).astype(np.float32)):
            assert np.array_equal(ref.median_sorted(v), scipy.ndimage.median_filter(v, size=3, mode="reflect")), shape
    v = rng.standard_normal((3, 4, 5)).astype(np.float32)
    v[1, 2, 3] = np.nan
    got = ref.median(v[None])[0]
    assert not np.isnan(got).any()  # one NaN of 27 never reaches the middle
    v[0:2, 1:3, 2:5] = np.nan
    assert np.isnan(ref.median(v[None])[0]).any()
    # a plane: the median of the 27 is the median of the 9
    import segment_ref

    p = rng.standard_normal((7, 9)).astype(np.float32)
    assert np.array_equal(ref.median_sorted(p[None])[0], segment_ref.median_plane(p, 3))


def test_the_segment_restatement_on_a_hand_made_volume():
    m = np.zeros((1, 3, 4, 5), dtype=np.uint8)
    m[0, 0, 0, 0:3] = 1  # a bar of 3
    m[0, 2, 3, 4] = 1    # a single voxel
    m[0, 1, 1, 3] = 1    # touches the bar's end (0, 0, 2) by a corner only
    v = np.where(m != 0, np.float32(3.0), np.float32(0.0)).astype(np.float32)
    g = np.zeros_like(m)
    g[0, 0, 0, 0] = g[0, 2, 3, 4] = 1
    labels, regions = ref.label(g, 26)
    seg, pixels, components, removed = ref.segment(v, g, labels, regions, [2.0], 2, 26)
    assert seg.sum() == 4 and pixels.tolist() == [[[1, 3, 1]]] and components.tolist() == [[[1, 1, 0]]] and removed.tolist() == [[[1, 1]]]
    seg, pixels, components, removed = ref.segment(v, g, labels, regions, [2.0], 2, 6)
    assert seg.sum() == 3 and pixels.tolist() == [[[1, 2, 1]]] and components.tolist() == [[[1, 1, 0]]] and removed.tolist() == [[[2, 2]]]
    seg, pixels, components, removed = ref.segment(v, g, labels, regions, [2.0, np.nan], 1, 6)
    assert pixels.tolist() == [[[2, 3, 0], [0, 0, 2]]] and components.tolist() == [[[2, 3, 1], [0, 0, 0]]] and not removed.any()


# ---- scoring ----------------------------------------------------------------------------------------------------------------------

def _segments_file(extent, n=3, T=2, seed=0):
    """A hand-made segments file of ``n`` items of ``extent``: random segmentations, no masks, FP = the predicted voxels."""
    rng = np.random.default_rng(seed)
    seg = (rng.random((n, 2, T) + tuple(extent)) < 0.2).astype(np.uint8)
    fp = seg.reshape(n, 2, T, -1).sum(axis=3).astype(np.int32)
    pixels = np.stack([np.zeros_like(fp), fp, np.zeros_like(fp)], axis=-1)
    components = np.zeros((n, 2, T, 3), dtype=np.int32)
    return {"filename": np.asarray([f"v{k}" for k in range(n)]), "t": np.asarray([10]), "channels": np.asarray(["lpips", "mse"]),
            "thresholds": np.tile(np.asarray([2.0, 3.0], dtype=np.float32)[:T], (2, 1)), "fpr": np.full(T, np.nan), "median": np.int64(3),
            "min_component": np.int64(8), "connectivity": np.int64(26 if len(extent) == 3 else 8), "sigma": np.float64(1.0), "segmentation": seg,
            "pixels": pixels, "components": components, "removed": np.zeros((n, 2, T, 2), dtype=np.int32),
            "mask_pixels": np.zeros(n, dtype=np.int64), "regions": np.zeros(n, dtype=np.int32)}


def test_score_segments_counts_every_voxel_of_a_volume_file():
    """in_fpr = FP / (N D H W): on the parent the divisor was N D H."""
    from ddpm_ood_amd import ood

    z = _segments_file((4, 5, 6))
    rows = ood.score_segments(z, z, "z_mse_map")
    for j, r in enumerate(rows):
        assert r["in_fpr"] == float(z["pixels"][:, 1, j, 1].sum()) / (3 * 4 * 5 * 6)
        assert r["in_fpr"] == float(z["segmentation"][:, 1, j].mean()) and 0.0 < r["in_fpr"] < 1.0


def test_score_segments_of_planes_is_unchanged():
    from ddpm_ood_amd import ood

    z = _segments_file((7, 9))
    rows = ood.score_segments(z, z, "z_lpips_map")
    for j, r in enumerate(rows):
        assert r["in_fpr"] == float(z["pixels"][:, 0, j, 1].sum()) / float(3 * 7 * 9)


def test_missing_files_name_both_flags(tmp_path):
    from ddpm_ood_amd import ood

    with pytest.raises(FileNotFoundError, match="--voxel_segment 1") as e:
        ood.print_segments("m", "X", tmp_path, "z_mse_map")
    assert "--pixel_segment 1" in str(e.value)


# ---- entry points -----------------------------------------------------------------------------------------------------------------

def test_every_refusal_of_the_entry_points_returns_minus_one():
    """Argument checks come before any launch: no device is needed to see them."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    A, B_, C_, D_, E_, F_, G_, H_, I_, J_ = (1 << k for k in (20, 24, 26, 28, 30, 32, 34, 36, 38, 40))  # disjoint fake device addresses

    def median(maps=A, out=B_, size=3, N=1, D=4, H=4, W=4):
        return lib.ddpm_map_median3d_f32(maps, out, size, N, D, H, W, None)

    for kw, what in ((dict(maps=None), b"null"), (dict(out=None), b"null"), (dict(size=1), b"size"), (dict(size=5), b"size"), (dict(size=27), b"size"),
                     (dict(D=0), b"positive"), (dict(N=0), b"positive"), (dict(W=-2), b"positive"), (dict(D=2048, H=1024, W=1024), b"2^31"),
                     (dict(out=B_ + 2), b"aligned"), (dict(maps=A + 1), b"aligned"), (dict(out=A), b"in place"), (dict(out=A + 64), b"in place"),
                     (dict(out=A - 64), b"in place")):
        assert median(**kw) == -1, kw
        assert b"map_median3d" in lib.ddpm_last_error() and what in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())

    def segment(maps=A, masks=B_, labels=C_, regions=D_, N=1, D=4, H=4, W=4, thr=E_, K=2, min_size=1, conn=26, seg=F_, pixels=G_,
                components=H_, removed=I_, scratch=J_):
        return lib.ddpm_map_segment3d_f32(maps, masks, labels, regions, N, D, H, W, thr, K, min_size, conn, seg, pixels, components, removed,
                                          scratch, None)

    for kw, what in ((dict(maps=None), b"null"), (dict(thr=None), b"null"), (dict(seg=None), b"null"), (dict(removed=None), b"null"),
                     (dict(scratch=None), b"null"), (dict(K=0), b"K must"), (dict(K=9), b"K must"), (dict(conn=8), b"connectivity"),
                     (dict(conn=4), b"connectivity"), (dict(H=0), b"positive"), (dict(D=2048, H=1024, W=1024), b"2^31"),
                     (dict(N=8192, K=8), b"65535"), (dict(min_size=0), b"min_size"), (dict(min_size=-1), b"min_size"),
                     (dict(pixels=G_ + 2), b"aligned"), (dict(scratch=J_ + 2), b"aligned"), (dict(maps=A + 1), b"aligned"),
                     (dict(seg=A + 8), b"alias"), (dict(pixels=E_), b"alias"), (dict(scratch=C_), b"alias"), (dict(scratch=F_ - 16), b"alias"),
                     (dict(removed=J_ + 32), b"alias"), (dict(components=G_ + 4), b"alias"), (dict(seg=J_ + 1), b"alias")):
        assert segment(**kw) == -1, kw
        assert b"map_segment3d" in lib.ddpm_last_error() and what in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ddpm_ood_hip.h").read_text(), flags=re.S)
    assert "#define DDPM_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    for name in ("ddpm_map_median3d_f32", "ddpm_map_segment3d_f32"):
        assert re.search(rf"\bint\s+{name}\s*\(", header) and _lib.SIGNATURES[name][0] is C.c_int
    assert re.search(r"\bint64_t\s+ddpm_regions3d_segment_scratch_bytes\s*\(", header)
    assert _lib.SIGNATURES["ddpm_regions3d_segment_scratch_bytes"] == (C.c_int64, [C.c_int] * 5)
    assert _lib.SIGNATURES["ddpm_map_segment3d_f32"][1].count(C.c_void_p) == 11
