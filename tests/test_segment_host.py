"""CPU: the restatements of tests/segment_ref.py against scipy, the flags of --pixel_segment 1, ``ood.score_segments`` on a hand-made
file, the C ABI of csrc/segment.hip and the packing of the segmentation rows."""

import argparse
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.ndimage
import torch

import region_ref
import segment_ref as ref

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. the restatements ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [3, 5])
def test_median_restatement_equals_scipy_on_nan_free_input(size):
    rng = np.random.default_rng(size)
    for H, W in [(1, 1), (1, 9), (9, 1), (2, 2), (5, 7), (33, 31), (128, 128)]:
        ties = rng.integers(-2, 3, size=(H, W)).astype(np.float32)
        special = np.asarray([np.inf, -np.inf, 0.0, 1e-45, -1e38, 3.0], dtype=np.float32)
        infs = np.where(rng.random((H, W)) < 0.4, rng.choice(special, size=(H, W)), rng.standard_normal((H, W))).astype(np.float32)
        for v in (ties, infs):
            want = scipy.ndimage.median_filter(v, size=size, mode="reflect")
            got = ref.median_plane(v, size)
            assert got.dtype == np.float32 and np.array_equal(got, want), (H, W)
    # NaN sorts above +inf: a window of 5 NaN among 9 values has a NaN median, one of 4 has not
    v = np.zeros((3, 3), dtype=np.float32)
    v[0, :] = v[1, 0] = np.nan
    v[1, 1] = np.inf
    assert np.isinf(ref.median_plane(v, 3)[1, 1])  # centre window: 4 NaN, then +inf is element 4 of 0 0 0 0 inf nan nan nan nan
    v[1, 2] = np.nan
    assert np.isnan(ref.median_plane(v, 3)[1, 1])
    assert ref.same_values(np.asarray([np.nan, -0.0, 1.0]), np.asarray([np.nan, 0.0, 1.0]))
    assert not ref.same_values(np.asarray([np.nan, 1.0]), np.asarray([1.0, np.nan]))


@pytest.mark.parametrize("conn", [4, 8])
def test_segment_restatement_numbers_components_as_the_labelling_restatement(conn):
    for H, W in [(1, 1), (5, 7), (33, 31)]:
        for name, m in region_ref.named_shapes(H, W).items():
            a, b = ref.label_plane(m != 0, conn), region_ref.label_plane(m != 0, conn)
            assert a[1] == b[1] and np.array_equal(a[0], b[0]), (name, H, W)
    m = region_ref.random_masks(2, 33, 31, 0.5, seed=conn)
    assert all(np.array_equal(x, y) for x, y in zip(ref.label(m, conn), region_ref.label(m, conn)))


def test_segment_restatement_on_a_hand_case():
    v = np.zeros((1, 6, 8), dtype=np.float32)
    v[0, 0, 0:3] = 5.0  # 3 pixels, on the mask
    v[0, 2, 5] = 5.0  # 1 pixel, off it
    v[0, 4, 0:4] = v[0, 5, 0] = 5.0  # 5 pixels, off it
    v[0, 5, 7] = np.nan
    g = np.zeros((1, 6, 8), dtype=np.uint8)
    g[0, 0, 1:6] = 1
    labels, regions = ref.label(g, 8)
    seg, pixels, components, removed = ref.segment(v, g, labels, regions, [2.0, np.nan], 3, 8)
    assert seg[0, 0].sum() == 8 and not seg[0, 1].any() and seg[0, 0, 2, 5] == 0
    assert pixels.tolist() == [[[2, 6, 3], [0, 0, 5]]] and components.tolist() == [[[1, 2, 1], [0, 0, 0]]]
    assert removed.tolist() == [[[1, 1], [0, 0]]]
    assert ref.segment(v, g, labels, regions, [2.0], 6, 8)[3].tolist() == [[[3, 9]]]


# ---- 2. flags -----------------------------------------------------------------------------------------------------------------------

def test_flags_parse_with_their_defaults_and_refusals():
    import ood_detection as det
    import reconstruct as cli
    from ddpm_ood_amd import pixel_metrics as pm
    from ddpm_ood_amd.map_passes import MapSettings

    a = cli.parse_args([])
    assert (a.pixel_segment, a.pixel_median, a.pixel_min_component) == (0, 3, 4)
    a = cli.parse_args(["--anomaly_z_maps", "1", "--pixel_segment", "1", "--pixel_median", "5", "--pixel_min_component", "9",
                        "--pixel_connectivity", "4", "--pixel_thresholds", "1.5,2"])
    assert pm.check_segment_flags(a) == (5, 9, [1.5, 2.0], 4)
    assert det.parse_args([]).pixel_segmented == 0 and det.parse_args(["--score", "pixel", "--pixel_segmented", "1"]).pixel_segmented == 1
    s = MapSettings.from_args(a)
    assert (s.pixel_segment, s.sg_median, s.sg_min_component, s.sg_thresholds, s.sg_connectivity) == (True, 5, 9, [1.5, 2.0], 4)
    assert not s.pixel_metrics and s.px_thresholds is None
    off = MapSettings.from_args(cli.parse_args(["--anomaly_z_maps", "1"]))
    assert not off.pixel_segment and off.sg_median is None
    assert pm.check_segment_flags(argparse.Namespace(anomaly_z_maps=1)) == (3, 4, [2.0, 3.0, 4.0], 8)  # a hand-made Namespace: the defaults

    def ns(**kw):
        return argparse.Namespace(**dict(dict(anomaly_z_maps=1, pixel_segment=1, anomaly_maps=0, pixel_metrics=0, spatial_dimension=2,
                                              vqvae_checkpoint=None, run_out=0, out_ids=None), **kw))

    for kw, text in ((dict(anomaly_z_maps=0), "--anomaly_z_maps 1"), (dict(pixel_median=2), "--pixel_median"), (dict(pixel_median=7), "--pixel_median"),
                     (dict(pixel_median=0), "--pixel_median"), (dict(pixel_median=3.5), "--pixel_median"), (dict(pixel_median="x"), "--pixel_median"),
                     (dict(pixel_min_component=0), "--pixel_min_component"), (dict(pixel_min_component=16385), "--pixel_min_component"),
                     (dict(pixel_min_component=-4), "--pixel_min_component"), (dict(pixel_min_component=None), "--pixel_min_component"),
                     (dict(pixel_thresholds="1,x"), "--pixel_thresholds"), (dict(pixel_thresholds="1,2,3,4,5,6,7,8,9"), "--pixel_thresholds"),
                     (dict(pixel_connectivity=6), "--pixel_connectivity")):
        with pytest.raises(ValueError, match=re.escape(text)):
            pm.check_segment_flags(ns(**kw))
        with pytest.raises(ValueError, match=re.escape(text)):
            MapSettings.from_args(ns(**kw))
    assert MapSettings.from_args(ns(pixel_median=1, pixel_min_component=16384)).sg_median == 1


def test_reconstruct_refuses_at_construction_before_anything_is_loaded():
    from ddpm_ood_amd.trainer import Reconstruct

    for kw, text in ((dict(anomaly_z_maps=0), "--anomaly_z_maps 1"), (dict(pixel_median=4), "--pixel_median"),
                     (dict(pixel_min_component=0), "--pixel_min_component")):
        base = dict(pixel_segment=1, anomaly_z_maps=1, anomaly_maps=0, pixel_metrics=0, spatial_dimension=2, vqvae_checkpoint=None, run_out=0,
                    out_ids=None)
        base.update(kw)
        with pytest.raises(ValueError, match=re.escape(text)):
            Reconstruct(argparse.Namespace(**base))


# ---- 3. scoring ---------------------------------------------------------------------------------------------------------------------

def _hand_file(N=2, T=2, H=4, W=4):
    pixels = np.zeros((N, 2, T, 3), dtype=np.int32)
    pixels[0, 1, 0] = (3, 1, 2)  # Dice 6 / 9
    pixels[1, 1, 0] = (0, 0, 0)  # an empty mask, nothing predicted: Dice 1
    pixels[0, 1, 1] = (1, 0, 4)  # Dice 2 / 6
    pixels[1, 1, 1] = (0, 2, 0)  # Dice 0
    components = np.zeros((N, 2, T, 3), dtype=np.int32)
    components[0, 1, 0], components[1, 1, 0] = (2, 3, 1), (0, 0, 0)
    components[0, 1, 1], components[1, 1, 1] = (1, 1, 0), (0, 1, 1)
    removed = np.zeros((N, 2, T, 2), dtype=np.int32)
    removed[0, 1, 0], removed[1, 1, 0], removed[1, 1, 1] = (4, 6), (1, 1), (2, 5)
    return {"filename": np.asarray(["a", "b"]), "t": np.asarray([10]), "channels": np.asarray(["lpips", "mse"]),
            "thresholds": np.asarray([[2.0, 3.5], [2.0, 4.5]], dtype=np.float32), "fpr": np.asarray([np.nan, 0.01]),
            "median": np.int64(3), "min_component": np.int64(4), "connectivity": np.int64(8), "sigma": np.float64(0.0),
            "segmentation": np.zeros((N, 2, T, H, W), dtype=np.uint8), "pixels": pixels, "components": components, "removed": removed,
            "mask_pixels": np.asarray([5, 0]), "regions": np.asarray([2, 0], dtype=np.int32)}


def test_score_segments_on_a_hand_made_file(tmp_path, capsys):
    from ddpm_ood_amd import ood

    out = _hand_file()
    rows = ood.score_segments(out)
    assert [r["threshold"] for r in rows] == [2.0, 4.5] and np.isnan(rows[0]["fpr"]) and rows[1]["fpr"] == 0.01
    assert rows[0]["mean_dice"] == pytest.approx((6 / 9 + 1.0) / 2) and rows[0]["pooled_dice"] == pytest.approx(6 / 9)
    assert rows[1]["mean_dice"] == pytest.approx((2 / 6 + 0.0) / 2) and rows[1]["pooled_dice"] == pytest.approx(2 / 8)
    assert (rows[0]["region_recall"], rows[0]["component_precision"]) == (1.0, pytest.approx(2 / 3))
    assert rows[0]["component_f1"] == pytest.approx(2 * (2 / 3) / (1 + 2 / 3))
    assert (rows[1]["region_recall"], rows[1]["component_precision"]) == (0.5, 0.5)
    assert [(r["removed_components"], r["removed_pixels"]) for r in rows] == [(5, 7), (2, 5)] and "in_fpr" not in rows[0]
    assert [r["threshold"] for r in ood.score_segments(out, key="z_lpips_map")] == [2.0, 3.5]
    ins = _hand_file()
    ins["pixels"][:] = 0
    ins["pixels"][0, 1, 0, 1], ins["pixels"][1, 1, 0, 1], ins["pixels"][1, 1, 1, 1] = 3, 5, 1
    rows = ood.score_segments(out, ins)
    assert [r["in_fpr"] for r in rows] == [8 / 32, 1 / 32]
    with pytest.raises(ValueError, match="another filter"):
        ood.score_segments(out, dict(ins, median=np.int64(5)))
    with pytest.raises(ValueError, match="key"):
        ood.score_segments(out, key="mse_map")
    # through the files and the printed lines
    (tmp_path / "m" / "ood").mkdir(parents=True)
    np.savez_compressed(tmp_path / "m" / "ood" / "segments_X.npz", **out)
    with pytest.raises(FileNotFoundError, match=re.escape("--pixel_segment 1")):
        ood.print_segments("m", "X", tmp_path / "m" / "ood", "z_mse_map")
    np.savez_compressed(tmp_path / "m" / "ood" / "segments_in.npz", **ins)
    assert repr(ood.print_segments("m", "X", tmp_path / "m" / "ood", "z_mse_map")) == repr(rows)  # (repr: a NaN equals no NaN)
    text = capsys.readouterr().out
    assert "Segmentations for m vs X: median 3, components below 4 pixels removed (connectivity 8)" in text
    assert "Segmented for m vs X at Z > 2: mean image Dice 0.8333, pooled Dice 0.6667, recall 1.0000, component precision 0.6667" in text
    assert "at Z > 4.5 (validation FPR <= 0.01): mean image Dice 0.1667" in text and "in-set FPR 0.03125, removed 2 components / 5 pixels" in text
    with pytest.raises(FileNotFoundError, match=re.escape("--pixel_segment 1")):
        ood.print_segments("m", "Y", tmp_path / "m" / "ood", "z_mse_map")


# ---- 4. the C ABI -------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_bound_and_return_int():
    from ddpm_ood_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ddpm_ood_hip.h").read_text(), flags=re.S)
    assert "#define DDPM_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.ddpm_abi_version() == 10
    p, i = C.c_void_p, C.c_int
    want = {"ddpm_map_median_f32": [p, p, i, i, i, i, p], "ddpm_map_segment_f32": [p, p, p, p, i, i, i, p, i, i, i, p, p, p, p, p]}
    for name, argtypes in want.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == argtypes
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == argtypes
    csrc = ROOT / "ddpm_ood_amd" / "csrc"
    build = (csrc / "build.sh").read_text()
    assert re.search(r"\bsegment\)", build) and "flags_segment=(-fno-strict-aliasing)" in build and "flags_regions=(-fno-strict-aliasing)" in build
    # the labelling is shared through a header, not copied
    assert "cc_link(CcShared" in (csrc / "regions_common.h").read_text() and "cc_compact(CcShared" in (csrc / "regions_common.h").read_text()
    for name in ("regions.hip", "segment.hip"):
        text = (csrc / name).read_text()
        assert '#include "regions_common.h"' in text and "__device__ void cc_link" not in text and "struct CcShared" not in text
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and ("map" in n or "pixel" in n or "region" in n or "segment" in n)]
    # host-side refusals need no device: they come before any launch
    assert lib.ddpm_map_median_f32(None, None, 3, 1, 1, 1, None) == -1 and b"map_median" in lib.ddpm_last_error() and b"null" in lib.ddpm_last_error()
    a, b, c, d, e, f, g, h, k = (j << 24 for j in range(1, 10))  # far apart: no overlap
    for size in (1, 2, 4, 7, 0, -3):
        assert lib.ddpm_map_median_f32(a, b, size, 1, 4, 4, None) == -1 and b"size must be 3 or 5" in lib.ddpm_last_error()
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.ddpm_map_median_f32(a, b, 3, N, H, W, None) == -1 and b"positive" in lib.ddpm_last_error()
    assert lib.ddpm_map_median_f32(a, b, 3, 1, 65536, 65536, None) == -1 and b"2^31" in lib.ddpm_last_error()
    assert lib.ddpm_map_median_f32(a, b + 2, 3, 1, 4, 4, None) == -1 and b"aligned" in lib.ddpm_last_error()
    for out in (a, a + 60, a - 60):
        assert lib.ddpm_map_median_f32(a, out, 5, 1, 4, 4, None) == -1 and b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_segment_f32(None, None, None, None, 1, 1, 1, None, 1, 1, 8, None, None, None, None, None) == -1
    assert b"map_segment" in lib.ddpm_last_error() and b"null" in lib.ddpm_last_error()

    def seg(N=2, H=4, W=4, K=1, min_size=4, conn=8, ptrs=(a, b, c, d, e, f, g, h, k)):
        return lib.ddpm_map_segment_f32(*ptrs[:4], N, H, W, ptrs[4], K, min_size, conn, *ptrs[5:], None)

    for kw, text in ((dict(H=129, W=128), b"129 x 128"), (dict(H=1, W=16385), b"1 x 16385"), (dict(H=0), b"positive"), (dict(conn=6), b"connectivity"),
                     (dict(H=65536, W=65536), b"65536 x 65536"), (dict(K=0), b"K must"), (dict(K=9), b"K must"), (dict(min_size=0), b"min_size"),
                     (dict(min_size=16385), b"min_size"), (dict(min_size=-1), b"min_size"),
                     (dict(ptrs=(a + 2, b, c, d, e, f, g, h, k)), b"aligned"), (dict(ptrs=(a, b, c, d, e, f, g + 1, h, k)), b"aligned")):
        assert seg(**kw) == -1 and b"map_segment" in lib.ddpm_last_error() and text in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())
    # an output over an input or over another output is refused before any launch
    for ptrs in ((a, b, c, d, e, b + 8, g, h, k), (a, b, c, d, e, f, a + 64, h, k), (a, b, c, d, e, f, g, c + 4, k), (a, b, c, d, e, f, g, h, d),
                 (a, b, c, d, e, f, g, h, e), (a, b, c, d, e, f, g, g + 12, k), (a, b, c, d, e, f, g, h, f + 16), (a, b, c, d, e, f, g, h, h + 20)):
        assert seg(ptrs=ptrs) == -1 and b"alias" in lib.ddpm_last_error(), ptrs


def test_wrappers_validate_before_the_library_is_asked():
    from ddpm_ood_amd import ops

    x = torch.zeros((1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.map_median(x, 3)  # a host tensor
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.map_segment(x, x.to(torch.uint8), x.to(torch.int32), torch.zeros(1, dtype=torch.int32), [2.0], 4)
    assert ops.MAP_MEDIAN_SIZES == (3, 5)


# ---- 5. the rows --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 1, 1, 1), (2, 5, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_segmentation_rows_pack_sixteen_pixels_to_a_float_exactly(shape):
    """The packing ``MapPass.segment_batch`` does on the device, here on the host, and ``unpack_segmentation``; the row layout."""
    from ddpm_ood_amd.map_passes import SEG_BITS, MapPipeline, MapSettings, unpack_segmentation

    rng = np.random.default_rng(shape[2])
    seg = (rng.random((3,) + shape) < 0.5).astype(np.uint8)
    seg[0] = 1  # (all sixteen bits set: 65 535)
    bits = torch.from_numpy(seg).reshape(3, -1)
    pad = -bits.shape[1] % SEG_BITS
    bits = torch.nn.functional.pad(bits, (0, pad))
    weights = torch.tensor([1 << b for b in range(SEG_BITS)], dtype=torch.int32)
    packed = (bits.reshape(3, -1, SEG_BITS).to(torch.int32) * weights).sum(dim=2).to(torch.float32)
    assert packed.shape[1] == -(-int(np.prod(shape)) // SEG_BITS) and float(packed.max()) <= 65535.0
    got = unpack_segmentation(packed.numpy(), shape)
    assert got.dtype == np.uint8 and np.array_equal(got, seg)
    s = MapSettings(anomaly_z_maps=True, pixel_segment=True, sg_median=3, sg_min_component=4, sg_thresholds=[2.0, 3.0, 4.0], sg_connectivity=8,
                    px_calibrate=True, cal_fprs=[0.05, 0.01])
    p = MapPipeline(s, torch.device("cpu"), ".")
    assert p.seg_T == 5 and p.layout is None
    assert p.seg_layout.segments == [("pixels", (2, 5, 3)), ("components", (2, 5, 3)), ("removed", (2, 5, 2)), ("regions", ()), ("mask_pixels", ())]
    assert p.seg_layout.width == 82 and p.seg_layout.without("mask_pixels").width == 81
    off = MapPipeline(MapSettings(), torch.device("cpu"), ".")
    assert off.seg_T == 0 and off.seg_layout is None
