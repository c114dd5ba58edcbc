"""CPU: the host side of --pixel_metrics 1: the metrics of ddpm_ood_amd/pixel_metrics.py against scikit-learn on
the bin indices, the float32 bin rule of tests/pixel_ref.py at its edges, the ``lesion`` kind and the masks of the data layer,
the flags and their refusals, the C ABI, and the scoring of a hand-made pixels_*.npz."""

import argparse
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pixel_ref as ref

ROOT = Path(__file__).resolve().parents[1]


def _hist_of(scores, labels, nbins):
    h = np.zeros((2, nbins + 1), dtype=np.int64)
    np.add.at(h, (labels, scores), 1)
    return h


@pytest.fixture(scope="module")
def pixels():
    """6 x 1 024 pixels at 64 bins: bin indices of overlapping classes, every bin index possible, some bins empty."""
    rng = np.random.default_rng(5)
    labels = (rng.random(6 * 1024) < 0.2).astype(np.int64)
    scores = np.clip(np.rint(rng.normal(24 + 10 * labels, 7)), 0, 63).astype(np.int64)
    return scores, labels, _hist_of(scores, labels, 64)


# ---- 1. metrics -----------------------------------------------------------------------------------------------------------------------

def test_auroc_and_average_precision_equal_sklearn_on_the_bin_indices(pixels):
    from sklearn.metrics import average_precision_score, roc_auc_score

    from ddpm_ood_amd import pixel_metrics as pm

    scores, labels, hist = pixels
    a, ap = pm.auroc(hist), pm.average_precision(hist)
    want_a, want_ap = roc_auc_score(labels, scores), average_precision_score(labels, scores)
    print(f"auroc {a:.12f} (sklearn {want_a:.12f}, diff {abs(a - want_a):.1e}); ap {ap:.12f} (sklearn {want_ap:.12f}, "
          f"diff {abs(ap - want_ap):.1e})")
    assert abs(a - want_a) <= 1e-12 and abs(ap - want_ap) <= 1e-12
    # NaN pixels are reported and change nothing
    with_nan = hist.copy()
    with_nan[:, -1] = (7, 3)
    assert pm.auroc(with_nan) == a and pm.average_precision(with_nan) == ap and pm.nan_pixels(with_nan) == (7, 3)


def test_curves_cumulate_from_the_top_bin(pixels):
    from ddpm_ood_amd import pixel_metrics as pm

    scores, labels, hist = pixels
    c = pm.curves(hist)
    assert len(c["tp"]) == len(c["fp"]) == 65 and c["tp"][64] == c["fp"][64] == 0
    for k in (0, 1, 17, 40, 63):
        assert c["tp"][k] == ((scores >= k) & (labels == 1)).sum() and c["fp"][k] == ((scores >= k) & (labels == 0)).sum()
        assert c["fn"][k] == ((scores < k) & (labels == 1)).sum()
    assert c["positives"] == labels.sum() and c["negatives"] == (1 - labels).sum()


def test_best_dice_equals_a_loop_over_the_bins(pixels):
    from ddpm_ood_amd import pixel_metrics as pm

    scores, labels, hist = pixels
    lo, step = -16.0, 0.5
    best, at = -1.0, None
    for k in range(65):
        pred = scores >= k
        tp, fp, fn = (pred & (labels == 1)).sum(), (pred & (labels == 0)).sum(), (~pred & (labels == 1)).sum()
        d = 2.0 * tp / (2.0 * tp + fp + fn)
        if d > best:
            best, at = d, lo + k * step
    got = pm.best_dice(hist, lo, step)
    assert got == (best, at) and 0 < best < 1


def test_dice_from_counts_and_the_empty_image():
    from ddpm_ood_amd import pixel_metrics as pm

    counts = np.asarray([[[3, 1, 2], [0, 0, 0]], [[0, 5, 0], [0, 0, 4]]])
    assert np.array_equal(pm.dice_from_counts(counts), [[6 / 9, 1.0], [0.0, 0.0]])
    with pytest.raises(ValueError):
        pm.dice_from_counts(np.zeros((2, 2)))


def test_degenerate_histograms():
    """No positive pixel: every metric raises.  No negative pixel: auroc is NaN, AP and Dice are computed (both 1 here)."""
    from ddpm_ood_amd import pixel_metrics as pm

    none = np.zeros((2, 9), dtype=np.int64)
    none[0, 2:5] = 4
    none[1, 8] = 3  # (NaN pixels inside the mask are no positives)
    for fn in (pm.curves, pm.auroc, pm.average_precision, lambda h: pm.best_dice(h, 0.0, 1.0)):
        with pytest.raises(ValueError, match="no positive"):
            fn(none)
    only = np.zeros((2, 9), dtype=np.int64)
    only[1, 2:5] = 4
    assert np.isnan(pm.auroc(only)) and pm.average_precision(only) == 1.0 and pm.best_dice(only, 0.0, 1.0) == (1.0, 0.0)
    for bad in (np.zeros((3, 9)), np.zeros(9), -np.ones((2, 9))):
        with pytest.raises(ValueError):
            pm.curves(bad)


# ---- 2. the bin rule --------------------------------------------------------------------------------------------------------------------

def test_bin_rule_at_the_edges():
    lo, hi, nbins = -16.0, 48.0, 4096
    step = (hi - lo) / nbins  # 1 / 64: every edge is a float32, and (edge - lo) * 64 is exact
    f = np.float32
    up, down = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
    assert ref.inv_step(lo, hi, nbins) == f(64.0)
    cases = [(lo, 0), (down(lo), 0), (up(lo), 0), (-1e30, 0), (-np.inf, 0), (hi, nbins - 1), (down(hi), nbins - 1), (up(hi), nbins - 1),
             (np.inf, nbins - 1), (3e38, nbins - 1), (np.nan, nbins)]
    # one ulp below an edge falls into the bin below only where the float32 subtraction keeps that ulp: v - lo is rounded once,
    # and with lo = -16 a value below 32 loses its last bit in it.  From 32 on, v and v - lo share the binade [32, 64) and the
    # difference is exact.  -0.375 - 1 ulp gives 15.625 again: bin 1000, not 999.
    for k in (3073, 3500, 4095):
        edge = f(lo + k * step)
        assert float(edge) > 32.0
        cases += [(edge, k), (down(edge), k - 1), (up(edge), k)]
    for k in (1, 2):  # next to lo the difference is small against both operands and exact too
        edge = f(lo + k * step)
        cases += [(edge, k), (down(edge), k - 1), (up(edge), k)]
    for k in (1000, 1024):
        edge = f(lo + k * step)
        cases += [(edge, k), (down(edge), k), (up(edge), k)]
    cases += [(0.0, 1024), (-0.0, 1024), (3.0, 19 * 64)]
    values = np.asarray([c[0] for c in cases], dtype=np.float32)
    got = ref.bin_index(values, lo, hi, nbins)
    assert got.tolist() == [c[1] for c in cases]
    # the same through float64: the difference of two float32 values of these magnitudes is exact there, rounded once to
    # float32 it is the float32 subtraction; the product with 64 is exact
    finite = np.isfinite(values)
    d = (values[finite].astype(np.float64) - lo).astype(np.float32).astype(np.float64) * 64.0
    assert got[finite].tolist() == np.clip(np.floor(np.maximum(d, 0.0)), 0, nbins - 1).astype(np.int64).tolist()
    # one bin: everything finite lands in it
    assert ref.bin_index(np.asarray([-5, 0, 0.999, 1, 7, np.nan], dtype=np.float32), 0.0, 1.0, 1).tolist() == [0, 0, 0, 0, 0, 1]
    # a range whose step is no float32: the rule is the float32 product's, rounding included
    v = np.asarray([0.1, 0.2, 0.3, 0.7], dtype=np.float32)
    want = [int(np.float32(np.float32(x - np.float32(0.0)) * np.float32(10 / 0.7))) for x in v[:3]] + [9]
    assert ref.bin_index(v, 0.0, 0.7, 10).tolist() == want
    h = ref.hist(np.asarray([[0.0, np.nan, 50.0, -20.0]], dtype=np.float32), np.asarray([[0, 255, 1, 0]], dtype=np.uint8), lo, hi, nbins)
    assert h.sum() == 4 and h[0, 1024] == 1 and h[1, nbins] == 1 and h[1, nbins - 1] == 1 and h[0, 0] == 1
    c = ref.counts(np.asarray([[1.0, 2.0, np.nan, 3.0]], dtype=np.float32), np.asarray([[1, 1, 1, 0]], dtype=np.uint8), [2.0])
    assert c.tolist() == [[[0, 1, 3]]]  # 2.0 > 2.0 is false; the NaN is predicted negative


# ---- 3. the lesion kind and the masks ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,mix,channels", [(32, 25, 1), (28, 10, 1), (32, 50, 3), (16, 5, 1)])
def test_lesion_kind(size, mix, channels):
    from ddpm_ood_amd import data

    x = data.synthetic_images("lesion", 5, channels, size, seed=3, mix=mix)
    m = data.synthetic_masks("lesion", 5, channels, size, seed=3, mix=mix)
    assert x.shape == (5, channels, size, size) and m.shape == (5, 1, size, size) and m.dtype == torch.uint8
    assert torch.equal(x, data.synthetic_images("lesion", 5, channels, size, seed=3, mix=mix))  # deterministic per seed
    assert torch.equal(m, data.synthetic_masks("lesion", 5, channels, size, seed=3, mix=mix))
    assert not torch.equal(m, data.synthetic_masks("lesion", 5, channels, size, seed=4, mix=mix))
    blobs = data.scale_intensity(data._blobs(5, channels, size, torch.Generator().manual_seed(3)))
    outside = (m == 0).expand_as(x)
    assert torch.equal(x[outside], blobs[outside])  # bit for bit: no second rescale
    assert not torch.equal(x, blobs) and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
    r = max(2.0, mix / 100.0 * size / 2.0)
    assert data.lesion_radius(size, mix) == r
    ys, xs = np.mgrid[:size, :size]
    for i in range(5):
        inside = m[i, 0].numpy().astype(bool)
        cy, cx = ys[inside].mean(), xs[inside].mean()  # a disc's centroid is its centre, up to the pixel grid
        d = np.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)
        assert inside[d <= r - 1].all() and not inside[d > r + 1].any()
        assert abs(inside.sum() - np.pi * r * r) <= 2 * np.pi * r + 4  # the area, within a ring of one pixel
        assert r - 1 <= cy <= size - r and r - 1 <= cx <= size - r  # inside the image: no row or column of the border is cut
        assert ys[inside].min() >= 0 and ys[inside].max() - ys[inside].min() + 1 >= 2 * int(r) - 1
    for kind in ("blobs", "speckle", "noise"):
        z = data.synthetic_masks(kind, 3, 1, size)
        assert z.shape == (3, 1, size, size) and z.dtype == torch.uint8 and not z.any()
    with pytest.raises(ValueError):
        data.synthetic_masks("nothing", 1)


def _batches(loader):
    return list(loader)


def test_loader_carries_no_mask_by_default_and_the_synthetic_masks_on_request():
    from ddpm_ood_amd import data

    spec = "synthetic:lesion:n=7:mix=25:seed=2"
    plain = _batches(data.get_data_loader(spec, 3, is_grayscale=True))
    assert all(sorted(b) == ["image", "image_meta_dict", "index"] for b in plain)
    masked = _batches(data.get_data_loader(spec, 3, is_grayscale=True, mask_ids="auto"))
    want = data.synthetic_masks("lesion", 7, 1, 32, seed=2, mix=25)
    assert [b["mask"].shape[0] for b in masked] == [3, 3, 1]
    for a, b in zip(plain, masked):
        assert torch.equal(a["image"], b["image"]) and a["index"] == b["index"]
        assert b["mask"].dtype == torch.uint8 and b["mask"].shape == (len(b["index"]), 1, 32, 32)
        assert torch.equal(b["mask"], want[b["index"]])
    # first_n and the rank partition, exactly as the images
    part = _batches(data.get_data_loader(spec, 8, is_grayscale=True, first_n=5, rank=1, world=2, mask_ids="auto"))
    assert part[0]["index"] == [1, 3] and torch.equal(part[0]["mask"], want[[1, 3]])
    with pytest.raises(ValueError, match="synthetic"):
        data.load_masks("auto", "some.csv", [], [])


def test_masks_follow_the_geometry_of_the_images(tmp_path):
    """--image_roi 32 24, --image_size and both flips: a marker pixel pattern takes the same way through both pipelines."""
    from ddpm_ood_amd import data

    rng = np.random.default_rng(0)
    images = rng.random((3, 1, 40, 36)).astype(np.float32)
    masks = np.zeros((3, 40, 36), dtype=np.uint8)
    masks[:, 10:22, 8:20] = 255  # any non-zero byte is inside
    masks[1, 0:4, :] = 1         # cropped away
    np.savez(tmp_path / "img.npz", images=images, names=np.asarray(["a.npy", "b.npy", "c.npy"]))
    np.savez(tmp_path / "msk.npz", masks=masks, names=np.asarray(["a.npy", "b.npy", "c.npy"]))
    for kw in ({}, {"image_roi": (32, 24)}, {"image_roi": (32, 24), "image_size": 16}, {"add_vflip": True}, {"add_hflip": True},
               {"image_roi": (32, 24), "image_size": 16, "add_vflip": True, "add_hflip": True}):
        b = _batches(data.get_data_loader(str(tmp_path / "img.npz"), 3, is_grayscale=True, mask_ids=str(tmp_path / "msk.npz"), **kw))[0]
        # the same geometry applied to the mask as an image (no intensity scaling): crop, area resize, >= 0.5, flips
        m = torch.from_numpy((masks != 0).astype(np.float32))[:, None]
        want = []
        for a in m:
            if kw.get("image_roi"):
                a = data.center_crop(a, kw["image_roi"])
            if kw.get("image_size"):
                a = torch.nn.functional.interpolate(a[None], size=(16, 16), mode="area")[0]
            a = (a >= 0.5).to(torch.uint8)
            if kw.get("add_vflip"):
                a = torch.flip(a, dims=(1,))
            if kw.get("add_hflip"):
                a = torch.flip(a, dims=(2,))
            want.append(a)
        assert torch.equal(b["mask"], torch.stack(want)), kw
        assert b["mask"].shape[2:] == b["image"].shape[2:] and set(b["mask"].unique().tolist()) <= {0, 1}
    # the crop start is the images': rows 4 .. 35 of 40, columns 6 .. 29 of 36
    b = _batches(data.get_data_loader(str(tmp_path / "img.npz"), 3, is_grayscale=True, mask_ids=str(tmp_path / "msk.npz"),
                                      image_roi=(32, 24)))[0]
    assert torch.equal(b["mask"][1, 0], torch.from_numpy((masks[1, 4:36, 6:30] != 0).astype(np.uint8)))
    # a flip moves the mask with the image: flipping back gives the unflipped loader's mask
    v = _batches(data.get_data_loader(str(tmp_path / "img.npz"), 3, is_grayscale=True, mask_ids=str(tmp_path / "msk.npz"), add_vflip=True))[0]
    p = _batches(data.get_data_loader(str(tmp_path / "img.npz"), 3, is_grayscale=True, mask_ids=str(tmp_path / "msk.npz")))[0]
    assert torch.equal(torch.flip(v["mask"], dims=(2,)), p["mask"]) and torch.equal(torch.flip(v["image"], dims=(2,)), p["image"])


def test_mask_files_and_their_refusals(tmp_path):
    from ddpm_ood_amd import data

    rng = np.random.default_rng(1)
    names = []
    for i in range(3):
        np.save(tmp_path / f"im{i}.npy", rng.random((20, 20)).astype(np.float32))
        np.save(tmp_path / f"mk{i}.npy", (rng.random((20, 20)) < 0.3).astype(np.float32) * (i + 1))
        names.append(str(tmp_path / f"im{i}.npy"))
    (tmp_path / "ids.csv").write_text(",".join(names) + "\n")
    (tmp_path / "masks.csv").write_text(",".join(str(tmp_path / f"mk{i}.npy") for i in range(3)) + "\n")
    b = _batches(data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "masks.csv")))[0]
    for i in range(3):
        assert torch.equal(b["mask"][i, 0], torch.from_numpy((np.load(tmp_path / f"mk{i}.npy") != 0).astype(np.uint8)))
    two = _batches(data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, first_n=2, mask_ids=str(tmp_path / "masks.csv")))[0]
    assert two["mask"].shape == (2, 1, 20, 20) and torch.equal(two["mask"], b["mask"][:2])
    # a count that differs
    (tmp_path / "short.csv").write_text(",".join(str(tmp_path / f"mk{i}.npy") for i in range(2)) + "\n")
    with pytest.raises(ValueError, match="2 masks for 3 images"):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "short.csv"))
    # an extent that differs
    np.savez(tmp_path / "wide.npz", masks=np.zeros((3, 20, 24), dtype=np.uint8))
    with pytest.raises(ValueError, match="after the transforms"):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "wide.npz"))
    np.savez(tmp_path / "count.npz", masks=np.zeros((4, 20, 20), dtype=np.uint8))
    with pytest.raises(ValueError, match="4 masks for 3 images"):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "count.npz"))
    # names that are not the images'
    np.savez(tmp_path / "named.npz", masks=np.zeros((3, 20, 20), dtype=np.uint8), names=np.asarray(["x", "y", "z"]))
    with pytest.raises(ValueError, match="names"):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "named.npz"))
    np.savez(tmp_path / "nokey.npz", images=np.zeros((3, 20, 20), dtype=np.uint8))
    with pytest.raises(ValueError, match="'masks'"):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "nokey.npz"))
    with pytest.raises(FileNotFoundError):
        data.get_data_loader(str(tmp_path / "ids.csv"), 4, is_grayscale=True, mask_ids=str(tmp_path / "none.npz"))


# ---- 4. flags ----------------------------------------------------------------------------------------------------------------------------

def test_flags_parse_with_their_defaults():
    import reconstruct as cli

    a = cli.parse_args([])
    assert (a.pixel_metrics, a.out_masks, a.pixel_bins, list(a.pixel_range), a.pixel_thresholds) == (0, None, 4096, [-16.0, 48.0], "2,3,4")
    a = cli.parse_args(["--pixel_metrics", "1", "--out_masks", "auto,,m.npz", "--pixel_bins", "64", "--pixel_range", "-4", "12.5",
                        "--pixel_thresholds", "1.5,3"])
    assert (a.pixel_metrics, a.out_masks, a.pixel_bins, list(a.pixel_range), a.pixel_thresholds) == (1, "auto,,m.npz", 64, [-4.0, 12.5], "1.5,3")
    import ood_detection as det

    d = det.parse_args(["--score", "pixel", "--pixel_include_in", "1", "--zmap_key", "z_lpips_map"])
    assert (d.score, d.pixel_include_in, d.zmap_key) == ("pixel", 1, "z_lpips_map") and det.parse_args([]).pixel_include_in == 0


def test_check_flags_and_every_refusal():
    from ddpm_ood_amd import pixel_metrics as pm

    assert pm.check_flags(1, "a.csv,b.csv,c.csv", "auto,,m.npz") == (-16.0, 48.0, 4096, [2.0, 3.0, 4.0], ["auto", None, "m.npz"])
    assert pm.check_flags(True, "a.csv", None, 64, [-4, 12], "1.5, 3")[:4] == (-4.0, 12.0, 64, [1.5, 3.0])
    assert pm.check_flags(1, "a.csv,b.csv", None)[4] == [None, None] and pm.check_flags(1, "a.csv", "")[4] == [None]
    assert pm.check_flags(1, None, None)[4] == []  # --run_out 0
    for kw, text in ((dict(anomaly_z_maps=0), "--anomaly_z_maps 1"), (dict(bins=0), "--pixel_bins"), (dict(bins=8192), "--pixel_bins"),
                     (dict(bins=2.5), "--pixel_bins"), (dict(bins="many"), "--pixel_bins"), (dict(value_range=(3, 3)), "--pixel_range"),
                     (dict(value_range=(5, -5)), "--pixel_range"), (dict(value_range=(0, float("inf"))), "--pixel_range"),
                     (dict(value_range=(float("nan"), 1)), "--pixel_range"), (dict(value_range=(1,)), "--pixel_range"),
                     (dict(thresholds=""), "--pixel_thresholds"), (dict(thresholds="1,2,3,4,5,6,7,8,9"), "--pixel_thresholds"),
                     (dict(thresholds="2,x"), "--pixel_thresholds"), (dict(thresholds="2,nan"), "--pixel_thresholds"),
                     (dict(out_masks="auto"), "--out_masks"), (dict(out_masks="auto,auto,auto"), "--out_masks")):
        args = dict(anomaly_z_maps=1, out_ids="a.csv,b.csv", out_masks=None)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(text)):
            pm.check_flags(**args)


def test_reconstruct_refuses_at_construction_before_anything_is_loaded():
    """The refusals come before the checkpoint is looked for: no run directory is needed to see them."""
    from ddpm_ood_amd.trainer import Reconstruct

    def ns(**kw):
        base = dict(pixel_metrics=1, anomaly_z_maps=1, anomaly_maps=0, spatial_dimension=2, vqvae_checkpoint=None, run_out=1,
                    out_ids="a.csv,b.csv", out_masks=None)
        base.update(kw)
        return argparse.Namespace(**base)

    for kw, text in ((dict(anomaly_z_maps=0), "--anomaly_z_maps 1"), (dict(pixel_bins=9000), "--pixel_bins"),
                     (dict(pixel_range=[2.0, 1.0]), "--pixel_range"), (dict(pixel_thresholds="a"), "--pixel_thresholds"),
                     (dict(out_masks="auto"), "--out_masks")):
        with pytest.raises(ValueError, match=re.escape(text)):
            Reconstruct(ns(**kw))


# ---- 5. the C ABI --------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_bound_and_return_int():
    from ddpm_ood_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ddpm_ood_hip.h").read_text(), flags=re.S)
    assert "#define DDPM_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10
    lib = _lib.load()
    want = {"ddpm_map_mask_hist_f32": [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p],
            "ddpm_map_mask_counts_f32": [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]}
    for name, argtypes in want.items():
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == argtypes
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == argtypes
    assert "pixel_metrics" in (ROOT / "ddpm_ood_amd" / "csrc" / "build.sh").read_text()
    # no size function came with them: the caller chooses `parts`
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and ("map" in n or "pixel" in n)]
    # host-side refusals of the entry points themselves need no device: they come before any launch
    assert lib.ddpm_map_mask_hist_f32(None, None, 1, 1, 0.0, 1.0, 1, 1, None, None, 0, None) == -1
    assert b"map_mask_hist" in lib.ddpm_last_error()
    assert lib.ddpm_map_mask_counts_f32(None, None, 1, 1, None, 1, None, None) == -1 and b"map_mask_counts" in lib.ddpm_last_error()
    for args, text in (((1, 1, 0.0, 1.0, 8192, 1), b"nbins"), ((1, 1, 0.0, 1.0, 0, 1), b"nbins"), ((65536, 65536, 0.0, 1.0, 8, 1), b"2^32"),
                       ((1, 1, 0.0, 1.0, 8, 0), b"parts"), ((1, 1, 0.0, 0.0, 8, 1), b"inv_step"), ((1, 1, float("nan"), 1.0, 8, 1), b"lo")):
        N, P, lo, inv, nbins, parts = args
        assert lib.ddpm_map_mask_hist_f32(1 << 20, 1 << 22, N, P, lo, inv, nbins, parts, 1 << 24, 1 << 26, 0, None) == -1, args
        assert text in lib.ddpm_last_error(), (args, lib.ddpm_last_error())
    assert lib.ddpm_map_mask_counts_f32(1 << 20, 1 << 22, 1, 16, 1 << 24, 9, 1 << 26, None) == -1 and b"K must" in lib.ddpm_last_error()
    assert lib.ddpm_map_mask_counts_f32(1 << 20, 1 << 22, 1, 16, 1 << 24, 0, 1 << 26, None) == -1
    assert lib.ddpm_map_mask_counts_f32(1 << 20, 1 << 20, 1, 16, 1 << 24, 2, (1 << 20) + 8, None) == -1 and b"alias" in lib.ddpm_last_error()
    # an output inside an input is refused before any launch: total inside maps, slabs inside masks
    assert lib.ddpm_map_mask_hist_f32(1 << 20, 1 << 22, 4, 16, 0.0, 1.0, 8, 1, 1 << 24, (1 << 20) + 64, 0, None) == -1
    assert b"alias" in lib.ddpm_last_error()
    assert lib.ddpm_map_mask_hist_f32(1 << 20, 1 << 22, 4, 16, 0.0, 1.0, 8, 1, (1 << 22) + 32, 1 << 26, 0, None) == -1
    assert lib.ddpm_map_mask_hist_f32(1 << 20, 1 << 22, 4, 16, 0.0, 1.0, 8, 2, 1 << 24, (1 << 24) + 72, 0, None) == -1  # total inside slabs


def test_wrappers_validate_before_the_library_is_asked():
    from ddpm_ood_amd import ops

    maps, masks = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8)
    for fn in (lambda: ops.map_mask_hist(maps, masks, 0.0, 1.0, 8), lambda: ops.map_mask_counts(maps, masks, [1.0])):
        with pytest.raises(ValueError, match="ROCm device"):
            fn()
    assert ops.map_hist_parts(1) == 1 and ops.map_hist_parts(16384) == 1 and ops.map_hist_parts(16385) == 2
    assert ops.map_hist_parts(1024 * 32 * 32) == 64 and ops.map_hist_parts(1 << 31) == ops.MAP_HIST_MAX_PARTS == 256


# ---- 6. merge and scoring -------------------------------------------------------------------------------------------------------------------

def _pixels_file(path, seed, nbins=64, n=4, masks=True):
    """A hand-made pixels_<name>.npz: both channels' histograms and counts computed from random maps with the restatement."""
    rng = np.random.default_rng(seed)
    lo, hi, thr = -4.0, 12.0, [2.0, 3.0]
    m = (rng.random((n, 256)) < 0.25).astype(np.uint8) if masks else np.zeros((n, 256), dtype=np.uint8)
    z = [(rng.normal(0, 1, (n, 256)) + (3.0 + c) * m).astype(np.float32) for c in range(2)]
    hist = np.stack([ref.hist(zc, m, lo, hi, nbins) for zc in z])
    counts = np.stack([ref.counts(zc, m, thr) for zc in z], axis=1)
    np.savez(path, filename=np.asarray([f"im{i}" for i in range(n)]), t=np.asarray([10]), channels=np.asarray(["lpips", "mse"]),
             lo=np.float64(lo), hi=np.float64(hi), nbins=np.int64(nbins), hist=hist, thresholds=np.asarray(thr, dtype=np.float32),
             counts=counts.astype(np.int32), mask_pixels=m.sum(axis=1), sigma=np.float64(0.0))
    return z, m, hist, counts


def test_merge_and_pooling():
    from ddpm_ood_amd import pixel_metrics as pm

    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 50, (2, 2, 9)), rng.integers(0, 50, (2, 2, 9))
    assert np.array_equal(pm.merge(a, b), a + b) and pm.merge(a, b).dtype == np.int64 and np.array_equal(pm.merge(a), a)
    big = np.full((2, 2, 9), 2 ** 40)
    assert (pm.merge(big, big, big) == 3 * 2 ** 40).all()
    pooled = pm.pool_negatives(a, b)
    assert np.array_equal(pooled[:, 1], a[:, 1]) and np.array_equal(pooled[:, 0], a[:, 0] + b[:, 0] + b[:, 1])
    for bad in ((a, b[:, :, :8]), (a[0, 0], a[0, 0])):
        with pytest.raises(ValueError):
            pm.merge(*bad)
    with pytest.raises(ValueError):
        pm.pool_negatives(a, b[:1])


def test_score_pixels_on_a_hand_made_file(tmp_path, capsys):
    from sklearn.metrics import roc_auc_score

    from ddpm_ood_amd import ood
    from ddpm_ood_amd import pixel_metrics as pm

    z, m, hist, counts = _pixels_file(tmp_path / "pixels_LES.npz", 3)
    zi, mi, hist_in, _ = _pixels_file(tmp_path / "pixels_in.npz", 4, masks=False)
    for c, key in enumerate(("z_lpips_map", "z_mse_map")):
        s = ood.score_pixels(tmp_path / "pixels_LES.npz", key=key)
        assert s["auroc"] == pm.auroc(hist[c]) and s["ap"] == pm.average_precision(hist[c])
        assert (s["best_dice"], s["best_dice_threshold"]) == pm.best_dice(hist[c], -4.0, 0.25) and s["nan_pixels"] == 0
        assert abs(s["auroc"] - roc_auc_score(m.reshape(-1), ref.bin_index(z[c].reshape(-1), -4.0, 12.0, 64))) <= 1e-12
        assert list(s["mean_dice"]) == [2.0, 3.0]
        assert np.allclose(list(s["mean_dice"].values()), pm.dice_from_counts(counts[:, c]).mean(axis=0), rtol=0, atol=1e-15)
        pooled = ood.score_pixels(tmp_path / "pixels_LES.npz", tmp_path / "pixels_in.npz", key=key)
        both = np.concatenate([z[c].reshape(-1), zi[c].reshape(-1)])
        labels = np.concatenate([m.reshape(-1), mi.reshape(-1)])
        assert abs(pooled["auroc"] - roc_auc_score(labels, ref.bin_index(both, -4.0, 12.0, 64))) <= 1e-12
        assert pooled["mean_dice"] == s["mean_dice"] and pooled["ap"] < s["ap"]
    with pytest.raises(ValueError, match="key"):
        ood.score_pixels(tmp_path / "pixels_LES.npz", key="mse_map")
    _pixels_file(tmp_path / "pixels_other.npz", 5, nbins=32)
    with pytest.raises(ValueError, match="another range"):
        ood.score_pixels(tmp_path / "pixels_LES.npz", tmp_path / "pixels_other.npz")
    # the command line's lines
    run = tmp_path / "run" / "model" / "ood"
    run.mkdir(parents=True)
    for n in ("pixels_LES.npz", "pixels_in.npz"):
        (run / n).write_bytes((tmp_path / n).read_bytes())
    args = argparse.Namespace(output_dir=str(tmp_path / "run"), model_name="model", zmap_key="z_mse_map", pixel_include_in=0)
    got = ood.main_pixels(args, out_data=["LES"])
    out = capsys.readouterr().out
    s = ood.score_pixels(tmp_path / "pixels_LES.npz")
    assert got == {"LES": s}
    assert f"Pixel AUC for model vs LES: {s['auroc'] * 100:.2f}" in out and f"Pixel AP for model vs LES: {s['ap'] * 100:.2f}" in out
    assert f"Best Dice for model vs LES: {s['best_dice']:.4f} at Z >= {s['best_dice_threshold']:.4f}" in out
    assert "Mean image Dice for model vs LES at Z > 2:" in out and "Mean image Dice for model vs LES at Z > 3:" in out
    args.pixel_include_in = 1
    assert ood.main_pixels(args, out_data=["LES"])["LES"]["auroc"] == ood.score_pixels(run / "pixels_LES.npz", run / "pixels_in.npz")["auroc"]
    assert "pooled in as negatives" in capsys.readouterr().out
