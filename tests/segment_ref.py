"""numpy restatements of the kernels of csrc/segment.hip, for the tests.

``median``: element (size^2 - 1) / 2 of ``np.sort`` of every window of ``np.pad(plane, size // 2, mode="symmetric")`` (what
``scipy.ndimage.median_filter(mode="reflect")`` gives on NaN-free input; np.sort puts NaN above +inf).  ``segment``: the components of
``v > thr`` (``scipy.ndimage.label``, which numbers them as ``region_ref.label_plane`` does: tests/test_segment_host.py) with their
sizes by ``np.bincount``."""

import numpy as np
import scipy.ndimage

STRUCTURES = {4: np.asarray([[0, 1, 0], [1, 1, 1], [0, 1, 0]]), 8: np.ones((3, 3), dtype=int)}


def label_plane(inside, connectivity=8):
    """(labels int32 [H, W], R) of one boolean plane."""
    labels, R = scipy.ndimage.label(np.asarray(inside, dtype=bool), structure=STRUCTURES[connectivity])
    return labels.astype(np.int32), int(R)


def median_plane(plane, size):
    plane = np.asarray(plane, dtype=np.float32)
    r = size // 2
    padded = np.pad(plane, r, mode="symmetric")  # (repeats the reflection when r exceeds the plane)
    H, W = plane.shape
    windows = np.stack([padded[dy:dy + H, dx:dx + W] for dy in range(size) for dx in range(size)], axis=-1)
    return np.sort(windows, axis=-1)[..., (size * size - 1) // 2]


def median(maps, size):
    """fp32 [N, H, W]."""
    return np.stack([median_plane(p, size) for p in np.asarray(maps, dtype=np.float32)])


def same_values(got, want):
    """Value equality with NaN exactly where the restatement has NaN (the sign of a zero and a NaN's payload are not pinned)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and bool((got[~np.isnan(want)] == want[~np.isnan(want)]).all())


def segment(maps, masks, labels, regions, thresholds, min_size, connectivity=8):
    """(seg uint8 [N, K, H, W], pixels int32 [N, K, 3], components int32 [N, K, 3], removed int32 [N, K, 2])."""
    maps = np.asarray(maps, dtype=np.float32)
    masks, labels = np.asarray(masks) != 0, np.asarray(labels)
    N, H, W = maps.shape
    K = len(thresholds)
    seg = np.zeros((N, K, H, W), dtype=np.uint8)
    pixels, components, removed = (np.zeros((N, K, w), dtype=np.int32) for w in (3, 3, 2))
    for k, t in enumerate(np.asarray(thresholds, dtype=np.float32)):
        with np.errstate(invalid="ignore"):
            pred = maps > t
        for n in range(N):
            comp, R = label_plane(pred[n], connectivity)
            sizes = np.bincount(comp.reshape(-1), minlength=R + 1)
            keep = sizes >= min_size
            keep[0] = False
            kept = keep[comp]
            seg[n, k] = kept
            pixels[n, k] = (kept & masks[n]).sum(), (kept & ~masks[n]).sum(), (~kept & masks[n]).sum()
            hit = np.unique(labels[n][kept])
            touched = np.zeros(R + 1, dtype=bool)
            touched[np.unique(comp[masks[n]])] = True
            components[n, k] = ((hit >= 1) & (hit <= int(regions[n]))).sum(), keep.sum(), (keep & ~touched).sum()
            removed[n, k] = (~keep[1:]).sum(), sizes[1:][~keep[1:]].sum()
    return seg, pixels, components, removed


def label(masks, connectivity=8):
    """(labels int32 [N, H, W], regions int32 [N]) of masks != 0."""
    got = [label_plane(np.asarray(p) != 0, connectivity) for p in masks]
    return np.stack([g[0] for g in got]), np.asarray([g[1] for g in got], dtype=np.int32)
