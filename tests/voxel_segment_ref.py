"""Restatements of the kernels of csrc/segment3d.hip, for the tests.

``median``: ``scipy.ndimage.median_filter(v, size=3, mode="reflect")`` for NaN-free volumes; with NaN, element 13 of ``np.sort`` of
every 27-value window of ``np.pad(v, 1, mode="symmetric")`` (np.sort puts NaN above +inf; on NaN-free input the two agree:
tests/test_voxel_segment_host.py).  ``segment``: the components of ``v > thr`` by ``scipy.ndimage.label`` with
``generate_binary_structure(3, k)``, their sizes by ``np.bincount``, the counts restated flat."""

import numpy as np
import scipy.ndimage

import voxel_ref

label = voxel_ref.label  # (labels int32 [N, D, H, W], regions int32 [N]) of masks != 0


def median_sorted(vol):
    """One fp32 [D, H, W] volume, by sorting the windows."""
    vol = np.asarray(vol, dtype=np.float32)
    padded = np.pad(vol, 1, mode="symmetric")  # (repeats the reflection where an extent is 1)
    D, H, W = vol.shape
    windows = np.stack([padded[dz:dz + D, dy:dy + H, dx:dx + W] for dz in range(3) for dy in range(3) for dx in range(3)], axis=-1)
    return np.sort(windows, axis=-1)[..., 13]


def median(vols):
    """fp32 [N, D, H, W]: scipy's filter where a volume holds no NaN, the sorted windows where it does."""
    vols = np.asarray(vols, dtype=np.float32)
    return np.stack([median_sorted(v) if np.isnan(v).any() else scipy.ndimage.median_filter(v, size=3, mode="reflect") for v in vols])


def same_values(got, want):
    """Value equality with NaN exactly where the restatement has NaN (the sign of a zero and a NaN's payload are not pinned)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and bool((got[~np.isnan(want)] == want[~np.isnan(want)]).all())


def segment(maps, masks, labels, regions, thresholds, min_size, connectivity=26):
    """(seg uint8 [N, K, D, H, W], pixels int32 [N, K, 3], components int32 [N, K, 3], removed int32 [N, K, 2])."""
    maps = np.asarray(maps, dtype=np.float32)
    N = maps.shape[0]
    flat_mask = (np.asarray(masks) != 0).reshape(N, -1)
    flat_labels = np.asarray(labels).reshape(N, -1)
    K = len(thresholds)
    seg = np.zeros((N, K) + maps.shape[1:], dtype=np.uint8)
    pixels, components, removed = (np.zeros((N, K, w), dtype=np.int32) for w in (3, 3, 2))
    for k, t in enumerate(np.asarray(thresholds, dtype=np.float32)):
        with np.errstate(invalid="ignore"):
            pred = maps > t
        for n in range(N):
            comp, R = voxel_ref.label_volume(pred[n], connectivity)
            comp = comp.reshape(-1)
            sizes = np.bincount(comp, minlength=R + 1)
            keep = sizes >= min_size
            keep[0] = False
            kept, m = keep[comp], flat_mask[n]
            seg[n, k] = kept.reshape(maps.shape[1:])
            pixels[n, k] = (kept & m).sum(), (kept & ~m).sum(), (~kept & m).sum()
            hit = np.unique(flat_labels[n][kept])
            touched = np.zeros(R + 1, dtype=bool)
            touched[np.unique(comp[m])] = True
            components[n, k] = ((hit >= 1) & (hit <= int(regions[n]))).sum(), keep.sum(), (keep & ~touched).sum()
            removed[n, k] = (~keep[1:]).sum(), sizes[1:][~keep[1:]].sum()
    return seg, pixels, components, removed
