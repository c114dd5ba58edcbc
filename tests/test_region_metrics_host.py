"""CPU: the numpy restatement of the labelling against scipy, pixel_metrics.pro_curve / aupro / component_scores against brute force
and hand cases, the flags of --pixel_regions 1 and their refusals, and the C ABI of csrc/regions.hip."""

import argparse
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pixel_ref
import region_ref as ref

ROOT = Path(__file__).resolve().parents[1]
LO, HI = -4.0, 12.0


# ---- 1. the restatement's labelling -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_labels_as_scipy_does(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
    planes = []
    for k, d in enumerate((0.3, 0.5, 0.6)):
        planes += list(ref.random_masks(6, 19, 17, d, seed=k)) + list(ref.random_masks(2, 1, 23, d, seed=10 + k))
        planes += list(ref.random_masks(2, 23, 1, d, seed=20 + k))
    for H, W in ((1, 1), (5, 7), (12, 12), (33, 31)):
        planes += list(ref.named_shapes(H, W).values())
    late = np.zeros((9, 9), dtype=np.uint8)  # a U whose arms meet only in the last row
    late[:, 1] = late[:, 7] = late[8, 1:8] = 1
    planes.append(late)
    for m in planes:
        want, n = ndimage.label(m, structure=structure)
        got, R = ref.label_plane(m, conn)
        assert R == n and np.array_equal(got, want)
    labels, regions = ref.label(np.stack([late, late.T]), conn)
    assert list(regions) == [1, 1] and labels.dtype == np.int32 and regions.dtype == np.int32
    v = np.where(late != 0, 2.0, np.nan).astype(np.float32)
    assert np.array_equal(ref.label(v[None], conn, threshold=1.0)[0][0], ref.label_plane(late, conn)[0])  # NaN is outside


# ---- 2. the curve and its area ----------------------------------------------------------------------------------------------------

def _case(seed, N=4, H=16, W=16, nbins=64, nan=True):
    """Random maps, raised inside a few rectangles per image; some NaN pixels inside and outside the regions."""
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), dtype=np.uint8)
    for n in range(N):
        for _ in range(int(rng.integers(1, 4))):
            y, x, h, w = rng.integers(0, H - 2), rng.integers(0, W - 2), rng.integers(1, 6), rng.integers(1, 6)
            m[n, y:y + h, x:x + w] = 1
    v = (rng.normal(0, 1.5, (N, H, W)) + 3.0 * m * rng.random((N, H, W))).astype(np.float32)
    if nan:
        v.reshape(-1)[rng.permutation(v.size)[:12]] = np.nan
    return v, m


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pro_curve_and_aupro_equal_the_brute_force(seed, conn):
    from ddpm_ood_amd import pixel_metrics as pm

    v, m = _case(seed)
    labels, regions = ref.label(m, conn)
    R = int(regions.sum())
    overlap = ref.overlap(v, labels, regions, LO, HI, 64)
    hist = pixel_ref.hist(v, m, LO, HI, 64)
    fpr, pro = pm.pro_curve(overlap, R, hist)
    want_fpr, want_pro = ref.pro_curve_direct(v, m, LO, HI, 64, conn)
    assert fpr.shape == pro.shape == (65,) and fpr[0] == 0.0 and pro[0] == 0.0
    assert np.abs(fpr - want_fpr).max() <= 1e-12 and np.abs(pro - want_pro).max() <= 1e-12
    assert (np.diff(fpr) >= 0).all() and (np.diff(pro) >= 0).all() and fpr[-1] == 1.0
    for limit in (0.3, 0.05, 0.731, 1.0):
        assert abs(pm.aupro(overlap, R, hist, limit) - ref.aupro_direct(v, m, LO, HI, 64, conn, limit)) <= 1e-12


def _tables(v, m, nbins, conn=8):
    labels, regions = ref.label(m, conn)
    return ref.overlap(v, labels, regions, LO, HI, nbins), int(regions.sum()), pixel_ref.hist(v, m, LO, HI, nbins)


def test_aupro_hand_cases():
    from ddpm_ood_amd import pixel_metrics as pm

    # a perfect map: every region above every pixel outside
    v, m = _case(5, nan=False)
    perfect = np.where(m != 0, 10.0, -2.0).astype(np.float32)
    assert pm.aupro(*_tables(perfect, m, 64)) == 1.0 and pm.aupro(*_tables(perfect, m, 64), fpr_limit=1.0) == 1.0
    # two regions of 30 and 3 pixels, the map graded inside the larger one and blind to the smaller one (its pixels lie below every
    # other pixel): each region weighs one half, so the score is half of what the larger region's pixels reach on their own --
    # pooled over the pixels the 30 of 33 would count for 10 / 11 instead
    m = np.zeros((1, 16, 16), dtype=np.uint8)
    m[0, 2:7, 2:8] = m[0, 12, 10:13] = 1
    rng = np.random.default_rng(6)
    v = rng.normal(0, 1, (1, 16, 16)).astype(np.float32)
    v[0, 2:7, 2:8] += rng.normal(2, 1, (5, 6)).astype(np.float32)
    v[0, 12, 10:13] = -3.9
    both = pm.aupro(*_tables(v, m, 64))
    alone = m.copy()
    alone[0, 12, 10:13] = 0
    overlap, R, _ = _tables(v, alone, 64)
    hist = pixel_ref.hist(v, m, LO, HI, 64)  # (the same negatives)
    assert R == 1 and abs(both - 0.5 * pm.aupro(overlap, 1, hist)) <= 1e-12
    pooled = hist[1][:-1].astype(np.float64)  # one pooled "region": the fraction of all 33 masked pixels per bin
    assert abs(both - 0.5 * (33 / 30) * pm.aupro(np.append(pooled / 33, 0.0), 1, hist)) <= 1e-12
    found = np.where(alone != 0, 10.0, np.where(m != 0, -3.9, 0.0)).astype(np.float32)  # the larger one found perfectly
    assert pm.aupro(*_tables(found, m, 64)) == 0.5
    # a limit that falls between two curve points.  Two bins; outside: 6 pixels in bin 0, 4 in bin 1; one region of 4 pixels, 1 in
    # bin 0 and 3 in bin 1: the curve is (0, 0), (0.4, 0.75), (1, 1)
    hist = np.asarray([[6, 4, 0], [1, 3, 0]])
    overlap = np.asarray([0.25, 0.75, 0.0])
    fpr, pro = pm.pro_curve(overlap, 1, hist)
    assert np.array_equal(fpr, [0.0, 0.4, 1.0]) and np.array_equal(pro, [0.0, 0.75, 1.0])
    assert abs(pm.aupro(overlap, 1, hist, 0.3) - 0.28125) <= 1e-15  # the triangle up to (0.3, 0.5625), over 0.3
    assert abs(pm.aupro(overlap, 1, hist, 0.7) - 0.5625) <= 1e-15  # 0.15 + 0.3 (0.75 + 0.875) / 2, over 0.7
    assert abs(pm.aupro(overlap, 1, hist, 0.4) - 0.375) <= 1e-15 and abs(pm.aupro(overlap, 1, hist, 1.0) - 0.675) <= 1e-15
    # NaN pixels inside a region count for its area and are never predicted: the curve ends below 1
    assert pm.pro_curve(np.asarray([0.25, 0.5, 0.25]), 1, hist)[1][-1] == 0.75
    # the conventions of auroc
    with pytest.raises(ValueError, match="no ground-truth region"):
        pm.aupro(overlap, 0, hist)
    assert np.isnan(pm.aupro(overlap, 1, np.asarray([[0, 0, 2], [1, 3, 0]])))
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="fpr_limit"):
            pm.aupro(overlap, 1, hist, bad)
    with pytest.raises(ValueError, match="overlap table"):
        pm.pro_curve(overlap[:2], 1, hist)


def test_component_scores_on_hand_counts():
    from ddpm_ood_amd import pixel_metrics as pm

    # three images with 2, 0 and 3 regions; two thresholds.  (hit, pred, false_pred)
    comp = np.asarray([[[2, 3, 1], [1, 1, 0]], [[0, 2, 2], [0, 0, 0]], [[1, 1, 0], [0, 0, 0]]])
    s = pm.component_scores(comp, [2, 0, 3])
    assert np.allclose(s["region_recall"], [3 / 5, 1 / 5], rtol=0, atol=1e-15)
    assert np.allclose(s["component_precision"], [1 - 3 / 6, 1.0], rtol=0, atol=1e-15)
    assert np.allclose(s["component_f1"], [2 * 0.6 * 0.5 / 1.1, 2 * 0.2 / 1.2], rtol=0, atol=1e-15)
    assert np.allclose(s["false_per_image"], [1.0, 0.0], rtol=0, atol=1e-15)
    nothing = pm.component_scores(np.zeros((2, 1, 3), dtype=np.int32), [1, 1])  # nothing predicted: precision 1, recall 0, F1 0
    assert (nothing["region_recall"][0], nothing["component_precision"][0], nothing["component_f1"][0]) == (0.0, 1.0, 0.0)
    assert np.isnan(pm.component_scores(np.zeros((2, 1, 3)), [0, 0])["region_recall"][0])
    for bad in ((np.zeros((2, 3)), [1, 1]), (np.zeros((2, 1, 3)), [1]), (np.zeros((0, 1, 3)), [])):
        with pytest.raises(ValueError, match="components"):
            pm.component_scores(*bad)


# ---- 3. flags ---------------------------------------------------------------------------------------------------------------------

def test_flags_parse_with_their_defaults_and_refusals():
    import ood_detection as det
    import reconstruct as cli
    from ddpm_ood_amd import pixel_metrics as pm

    a = cli.parse_args([])
    assert (a.pixel_regions, a.pixel_connectivity, a.pixel_pro_fpr) == (0, 8, 0.3)
    a = cli.parse_args(["--pixel_regions", "1", "--pixel_connectivity", "4", "--pixel_pro_fpr", "0.1"])
    assert (a.pixel_regions, a.pixel_connectivity, a.pixel_pro_fpr) == (1, 4, 0.1)
    with pytest.raises(SystemExit):
        cli.parse_args(["--pixel_connectivity", "6"])
    d = det.parse_args(["--score", "pixel", "--pixel_regions", "1", "--pixel_pro_fpr", "0.2"])
    assert (d.pixel_regions, d.pixel_pro_fpr) == (1, 0.2) and (det.parse_args([]).pixel_regions, det.parse_args([]).pixel_pro_fpr) == (0, 0.3)
    assert pm.check_region_flags(1) == (8, 0.3) and pm.check_region_flags(True, "4", "1") == (4, 1.0)
    for args, text in (((0,), "--pixel_metrics 1"), ((1, 6), "--pixel_connectivity"), ((1, 4.5), "--pixel_connectivity"),
                       ((1, "x"), "--pixel_connectivity"), ((1, 8, 0.0), "--pixel_pro_fpr"), ((1, 8, 1.5), "--pixel_pro_fpr"),
                       ((1, 8, float("nan")), "--pixel_pro_fpr"), ((1, 8, None), "--pixel_pro_fpr")):
        with pytest.raises(ValueError, match=re.escape(text)):
            pm.check_region_flags(*args)
    # check_flags is what it was
    assert pm.check_flags(1, "a.csv", None) == (-16.0, 48.0, 4096, [2.0, 3.0, 4.0], [None])


def test_reconstruct_refuses_at_construction_before_anything_is_loaded():
    from ddpm_ood_amd.trainer import Reconstruct

    def ns(**kw):
        base = dict(pixel_regions=1, pixel_metrics=1, anomaly_z_maps=1, anomaly_maps=0, spatial_dimension=2, vqvae_checkpoint=None,
                    run_out=1, out_ids="a.csv", out_masks=None)
        base.update(kw)
        return argparse.Namespace(**base)

    for kw, text in ((dict(pixel_metrics=0), "--pixel_metrics 1"), (dict(pixel_connectivity=6), "--pixel_connectivity"),
                     (dict(pixel_pro_fpr=2.0), "--pixel_pro_fpr")):
        with pytest.raises(ValueError, match=re.escape(text)):
            Reconstruct(ns(**kw))


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_bound_and_return_int():
    from ddpm_ood_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ddpm_ood_hip.h").read_text(), flags=re.S)
    assert "#define DDPM_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    lib = _lib.load()
    assert lib.ddpm_abi_version() == 10
    p, i, f = C.c_void_p, C.c_int, C.c_float
    want = {"ddpm_map_label_u8": [p, i, i, i, i, p, p, p],
            "ddpm_map_label_f32": [p, f, i, i, i, i, p, p, p],
            "ddpm_map_region_overlap_f32": [p, p, p, i, i, f, f, i, p, p, i, p],
            "ddpm_map_component_counts_f32": [p, p, p, p, i, i, i, p, i, i, p, p]}
    for name, argtypes in want.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == argtypes
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == argtypes
    build = (ROOT / "ddpm_ood_amd" / "csrc" / "build.sh").read_text()
    assert re.search(r"\bregions\b", build) and "pixel_metrics" in build
    # the bin rule is shared through a header, not copied
    csrc = ROOT / "ddpm_ood_amd" / "csrc"
    assert "pm_bin(float" in (csrc / "pixel_common.h").read_text()
    for name in ("regions.hip", "pixel_metrics.hip"):
        text = (csrc / name).read_text()
        assert '#include "pixel_common.h"' in text and "pm_bin(float" not in text
    # no size function came with them
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and ("map" in n or "pixel" in n or "region" in n)]
    # host-side refusals need no device: they come before any launch
    assert lib.ddpm_map_label_u8(None, 1, 1, 1, 8, None, None, None) == -1 and b"map_label_u8" in lib.ddpm_last_error()
    assert lib.ddpm_map_label_f32(None, 0.0, 1, 1, 1, 8, None, None, None) == -1 and b"map_label_f32" in lib.ddpm_last_error()
    assert lib.ddpm_map_region_overlap_f32(None, None, None, 1, 1, 0.0, 1.0, 1, None, None, 0, None) == -1
    assert b"map_region_overlap" in lib.ddpm_last_error() and b"null" in lib.ddpm_last_error()
    assert lib.ddpm_map_component_counts_f32(None, None, None, None, 1, 1, 1, None, 1, 8, None, None) == -1
    assert b"map_component_counts" in lib.ddpm_last_error() and b"null" in lib.ddpm_last_error()
    a, b, c, d, e, g = (k << 22 for k in range(1, 7))  # far apart: no overlap
    for H, W, conn, text in ((129, 128, 8, b"129 x 128"), (1, 16385, 8, b"1 x 16385"), (0, 4, 8, b"positive"), (4, 4, 6, b"connectivity"),
                             (4, 4, 0, b"connectivity"), (65536, 65536, 8, b"65536 x 65536")):
        assert lib.ddpm_map_label_u8(a, 1, H, W, conn, b, c, None) == -1 and b"map_label_u8" in lib.ddpm_last_error()
        assert text in lib.ddpm_last_error(), lib.ddpm_last_error()
        assert lib.ddpm_map_label_f32(a, 0.0, 1, H, W, conn, b, c, None) == -1 and b"map_label_f32" in lib.ddpm_last_error()
        assert lib.ddpm_map_component_counts_f32(a, b, c, d, 1, H, W, e, 1, conn, g, None) == -1
        assert b"map_component_counts" in lib.ddpm_last_error() and text in lib.ddpm_last_error()
    for K in (0, 9):
        assert lib.ddpm_map_component_counts_f32(a, b, c, d, 1, 4, 4, e, K, 8, g, None) == -1 and b"K must" in lib.ddpm_last_error()
    for P, lo, inv, nbins, text in ((16385, 0.0, 1.0, 8, b"16385"), (0, 0.0, 1.0, 8, b"positive"), (16, 0.0, 1.0, 8192, b"nbins"),
                                    (16, 0.0, 1.0, 0, b"nbins"), (16, 0.0, 0.0, 8, b"inv_step"), (16, float("nan"), 1.0, 8, b"lo")):
        assert lib.ddpm_map_region_overlap_f32(a, b, c, 1, P, lo, inv, nbins, d, e, 0, None) == -1
        assert b"map_region_overlap" in lib.ddpm_last_error() and text in lib.ddpm_last_error(), lib.ddpm_last_error()
    # an output that overlaps another operand is refused before any launch
    assert lib.ddpm_map_label_u8(a, 2, 4, 4, 8, a + 16, c, None) == -1 and b"alias" in lib.ddpm_last_error()  # labels inside masks
    assert lib.ddpm_map_label_u8(a, 2, 4, 4, 8, b, b + 64, None) == -1 and b"alias" in lib.ddpm_last_error()  # regions inside labels
    assert lib.ddpm_map_label_f32(a, 0.0, 2, 4, 4, 8, b, a + 124, None) == -1 and b"alias" in lib.ddpm_last_error()  # regions inside maps
    assert lib.ddpm_map_region_overlap_f32(a, b, c, 2, 16, 0.0, 1.0, 8, d, d + 72, 0, None) == -1 and b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_region_overlap_f32(a, b, c, 2, 16, 0.0, 1.0, 8, b + 64, e, 0, None) == -1 and b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_region_overlap_f32(a, b, c, 2, 16, 0.0, 1.0, 8, d, c, 0, None) == -1 and b"alias" in lib.ddpm_last_error()
    for where in (a + 8, b + 8, c + 8, d, e):
        assert lib.ddpm_map_component_counts_f32(a, b, c, d, 2, 4, 4, e, 1, 8, where, None) == -1 and b"alias" in lib.ddpm_last_error()


def test_wrappers_validate_before_the_library_is_asked():
    from ddpm_ood_amd import ops

    assert ops.MAP_LABEL_MAX_PIXELS == 16384
    maps, masks = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8)
    labels, regions = torch.zeros(2, 4, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for fn in (lambda: ops.map_label(masks), lambda: ops.map_label(maps, threshold=0.0),
               lambda: ops.map_region_overlap(maps, labels, regions, 0.0, 1.0, 8),
               lambda: ops.map_component_counts(maps, masks, labels, regions, [1.0])):
        with pytest.raises(ValueError, match="ROCm device"):
            fn()
    with pytest.raises(ValueError, match="connectivity"):
        ops.map_label(masks, 6)


# ---- 5. scoring -------------------------------------------------------------------------------------------------------------------

def _files(tmp, name, seed, masks=True, nbins=64):
    """Hand-made pixels_<name>.npz and regions_<name>.npz from random maps with the restatements."""
    v0, m = _case(seed, nan=False)
    v1, _ = _case(seed + 100, nan=False)
    if not masks:
        m = np.zeros_like(m)
    z = [v0, (v1 + 2.0 * m).astype(np.float32)]
    thr = [2.0, 3.0]
    labels, regions = ref.label(m, 8)
    common = dict(filename=np.asarray([f"im{i}" for i in range(len(m))]), t=np.asarray([10]), channels=np.asarray(["lpips", "mse"]),
                  lo=np.float64(LO), hi=np.float64(HI), nbins=np.int64(nbins), thresholds=np.asarray(thr, dtype=np.float32),
                  sigma=np.float64(0.0))
    hist = np.stack([pixel_ref.hist(zc, m, LO, HI, nbins) for zc in z])
    np.savez(tmp / f"pixels_{name}.npz", hist=hist, counts=np.stack([pixel_ref.counts(zc, m, thr) for zc in z], axis=1).astype(np.int32),
             mask_pixels=m.reshape(len(m), -1).sum(axis=1), **common)
    overlap = np.stack([ref.overlap(zc, labels, regions, LO, HI, nbins) for zc in z])
    comps = np.stack([ref.component_counts(zc, m, labels, regions, thr, 8) for zc in z], axis=1)
    np.savez(tmp / f"regions_{name}.npz", connectivity=np.int64(8), regions=regions, overlap=overlap, components=comps, **common)
    return z, m, hist, overlap, regions, comps


def test_score_pixels_with_a_regions_file(tmp_path, capsys):
    from ddpm_ood_amd import ood
    from ddpm_ood_amd import pixel_metrics as pm

    run = tmp_path / "run" / "model" / "ood"
    run.mkdir(parents=True)
    z, m, hist, overlap, regions, comps = _files(run, "LES", 3)
    zi, mi, hist_in, *_ = _files(run, "in", 4, masks=False)
    plain = ood.score_pixels(run / "pixels_LES.npz")
    assert "aupro" not in plain and "region_recall" not in plain  # without the file: what it was
    for c, key in enumerate(("z_lpips_map", "z_mse_map")):
        s = ood.score_pixels(run / "pixels_LES.npz", key=key, regions_npz=run / "regions_LES.npz")
        assert s["aupro"] == pm.aupro(overlap[c], int(regions.sum()), hist[c], 0.3)
        assert abs(s["aupro"] - ref.aupro_direct(z[c], m, LO, HI, 64, 8, 0.3)) <= 1e-12
        want = pm.component_scores(comps[:, c], regions)
        for name in ("region_recall", "component_precision", "component_f1"):
            assert list(s[name]) == [2.0, 3.0] and list(s[name].values()) == want[name].tolist()
        assert {k: s[k] for k in plain} == ood.score_pixels(run / "pixels_LES.npz", key=key)
        # the in set's pixels enter the false-positive rate only
        pooled = ood.score_pixels(run / "pixels_LES.npz", run / "pixels_in.npz", key, run / "regions_LES.npz", 0.2)
        both, mask = np.concatenate([z[c], zi[c]]), np.concatenate([m, mi])
        assert abs(pooled["aupro"] - ref.aupro_direct(both, mask, LO, HI, 64, 8, 0.2)) <= 1e-12
        assert pooled["region_recall"] == s["region_recall"] and pooled["component_precision"] == s["component_precision"]
    _files(tmp_path, "other", 5, nbins=32)
    with pytest.raises(ValueError, match="regions file"):
        ood.score_pixels(run / "pixels_LES.npz", regions_npz=tmp_path / "regions_other.npz")
    # the command line's lines
    args = argparse.Namespace(output_dir=str(tmp_path / "run"), model_name="model", zmap_key="z_mse_map", pixel_include_in=0)
    ood.main_pixels(args, out_data=["LES"])
    before = capsys.readouterr().out
    assert "AUPRO" not in before
    args.pixel_regions, args.pixel_pro_fpr = 1, 0.3
    got = ood.main_pixels(args, out_data=["LES"])
    out = capsys.readouterr().out
    s = ood.score_pixels(run / "pixels_LES.npz", regions_npz=run / "regions_LES.npz")
    assert got == {"LES": s} and out.startswith(before)  # the new lines come after the existing ones
    assert f"AUPRO (FPR <= 0.3) for model vs LES: {s['aupro'] * 100:.2f}" in out
    assert f"Regions for model vs LES at Z > 2: recall {s['region_recall'][2.0]:.4f}" in out and "at Z > 3: recall" in out
