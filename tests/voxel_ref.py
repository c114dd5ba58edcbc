"""Restatements of the 3-D region kernels (csrc/regions3d.hip), for the tests.

``label``: ``scipy.ndimage.label`` with ``generate_binary_structure(3, k)`` (connectivity 6, 18, 26 for k = 1, 2, 3); label 0 is
the background and the components are numbered 1 .. R in ascending order of their smallest flat voxel index.  ``label_plain``: the
same by a plain union-find over the voxels, no scipy (the CPU tests hold the two against each other).  ``overlap``,
``component_counts`` and ``aupro_direct`` are region_ref.py's flat float64 restatements with this labelling."""

import numpy as np
import scipy.ndimage

import pixel_ref
import region_ref

RANK = {6: 1, 18: 2, 26: 3}


def structure(connectivity):
    return scipy.ndimage.generate_binary_structure(3, RANK[connectivity])


def _inside(x, threshold):
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return x != 0 if threshold is None else x.astype(np.float32) > np.float32(threshold)


def label_volume(inside, connectivity=26):
    """(labels int32 [D, H, W], R) of one boolean volume."""
    lab, R = scipy.ndimage.label(np.asarray(inside, dtype=bool), structure=structure(connectivity))
    return lab.astype(np.int32), int(R)


def label(x, connectivity=26, threshold=None):
    """(labels int32 [N, D, H, W], regions int32 [N]): of x != 0, or of x > threshold in float32 (NaN outside)."""
    got = [label_volume(v, connectivity) for v in _inside(x, threshold)]
    return np.stack([g[0] for g in got]), np.asarray([g[1] for g in got], dtype=np.int32)


def label_plain(inside, connectivity=26):
    """``label_volume`` by a plain union-find: every voxel joined to the neighbours that precede it in flat order."""
    inside = np.asarray(inside, dtype=bool)
    D, H, W = inside.shape
    flat = inside.reshape(-1)
    parent = list(range(D * H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    limit = RANK[connectivity]
    steps = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if (dz, dy, dx) < (0, 0, 0) and abs(dz) + abs(dy) + abs(dx) <= limit]
    for i in np.flatnonzero(flat):
        z, y, x = i // (H * W), i // W % H, i % W
        for dz, dy, dx in steps:
            zz, yy, xx = z + dz, y + dy, x + dx
            if 0 <= zz < D and 0 <= yy < H and 0 <= xx < W and inside[zz, yy, xx]:
                a, b = find(int(i)), find((zz * H + yy) * W + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)  # (the root is the smallest flat index of its tree)
    labels = np.zeros(D * H * W, dtype=np.int32)
    number = {}
    for i in np.flatnonzero(flat):  # ascending: a component is first met at its smallest voxel, its root
        labels[i] = number.setdefault(find(int(i)), len(number) + 1)
    return labels.reshape(D, H, W), len(number)


overlap = region_ref.overlap            # flat over everything behind the batch axis
overlap_rows = region_ref.overlap_rows


def component_counts(maps, masks, labels, regions, thresholds, connectivity=26):
    """int32 [N, K, 3]: hit (regions with a voxel v > thr), pred (components of v > thr), false_pred (those without a masked voxel)."""
    maps = np.asarray(maps, dtype=np.float32)
    masks, labels = np.asarray(masks) != 0, np.asarray(labels)
    N = maps.shape[0]
    out = np.zeros((N, len(thresholds), 3), dtype=np.int32)
    for k, t in enumerate(np.asarray(thresholds, dtype=np.float32)):
        with np.errstate(invalid="ignore"):
            pred = maps > t
        for n in range(N):
            hit = np.unique(labels[n][pred[n]])
            out[n, k, 0] = int(((hit >= 1) & (hit <= int(regions[n]))).sum())
            comp, R = label_volume(pred[n], connectivity)
            out[n, k, 1] = R
            out[n, k, 2] = R - len(np.setdiff1d(np.unique(comp[masks[n]]), [0]))
    return out


def pro_curve_direct(maps, masks, lo, hi, nbins, connectivity=26):
    """region_ref.pro_curve_direct with the regions of ``label``: per threshold k the mean over all regions of the predicted
    fraction of the region, and the FPR over the scored voxels outside every mask."""
    maps = np.asarray(maps, dtype=np.float32)
    N = maps.shape[0]
    labels, regions = label(np.asarray(masks).reshape(maps.shape), connectivity)
    bins = pixel_ref.bin_index(maps, lo, hi, nbins)
    scored = bins < nbins
    negatives = (labels == 0) & scored
    region_sets = [(n, labels[n] == r) for n in range(N) for r in range(1, int(regions[n]) + 1)]
    areas = [sel.sum() for _, sel in region_sets]
    fpr, pro = [], []
    for k in range(nbins, -1, -1):
        pred = (bins >= k) & scored
        fpr.append((pred & negatives).sum() / negatives.sum())
        pro.append(np.mean([(pred[n] & sel).sum() / a for (n, sel), a in zip(region_sets, areas)]))
    return np.asarray(fpr), np.asarray(pro)


def aupro_direct(maps, masks, lo, hi, nbins, connectivity=26, fpr_limit=0.3):
    """The area under ``pro_curve_direct`` on [0, fpr_limit], the last segment cut by linear interpolation, over fpr_limit."""
    fpr, pro = pro_curve_direct(maps, masks, lo, hi, nbins, connectivity)
    area = 0.0
    for j in range(1, len(fpr)):
        x0, x1, y0, y1 = fpr[j - 1], fpr[j], pro[j - 1], pro[j]
        if x1 <= fpr_limit:
            area += (x1 - x0) * (y0 + y1) / 2
        else:
            if x0 < fpr_limit:
                area += (fpr_limit - x0) * (y0 + (y0 + (y1 - y0) * (fpr_limit - x0) / (x1 - x0))) / 2
            break
    return area / fpr_limit


# ---- named shapes -------------------------------------------------------------------------------------------------------------

def checkerboard(D, H, W):
    z, y, x = np.mgrid[:D, :H, :W]
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def serpentine(D, H, W):
    """One voxel wide: region_ref.serpentine in every other plane, the planes joined alternately at the last and the first voxel
    of the path (the worst chain: one component whose voxels are met in an order that keeps re-rooting it)."""
    m = np.zeros((D, H, W), dtype=np.uint8)
    plane = region_ref.serpentine(H, W)
    rows = list(range(0, H, 2))
    # the path of a plane runs from (0, 0) to the free end of its last full row
    k = len(rows) - 1
    end = (rows[-1], W - 1 if k % 2 == 0 else 0)
    for j, z in enumerate(range(0, D, 2)):
        m[z] = plane
        if z + 1 < D and z + 2 < D:
            y, x = end if j % 2 == 0 else (0, 0)
            m[z + 1, y, x] = 1
    return m


def spiral(D, H, W):
    """region_ref.spiral in every other plane, the planes joined at the outer corner."""
    m = np.zeros((D, H, W), dtype=np.uint8)
    m[0::2] = region_ref.spiral(H, W)
    m[1::2, 0, 0] = 1
    return m


def comb(D, H, W):
    """Teeth along d at every other (h, w) that join only in the last plane."""
    m = np.zeros((D, H, W), dtype=np.uint8)
    m[:, 0::2, 0::2] = 1
    m[D - 1] = 1
    return m


def two_cubes(kind, side=2):
    """Two cubes that touch by a face, an edge or a corner: one component for 6 / 18 / 26 neighbours and up, two below."""
    s = side
    m = np.zeros((2 * s + 1, 2 * s + 1, 2 * s + 1), dtype=np.uint8)
    m[:s, :s, :s] = 1
    off = {"face": (s, 0, 0), "edge": (s, s, 0), "corner": (s, s, s)}[kind]
    m[off[0]:off[0] + s, off[1]:off[1] + s, off[2]:off[2] + s] = 1
    return m


def named_shapes(D, H, W):
    single = np.zeros((D, H, W), dtype=np.uint8)
    single[D // 2, H // 2, W // 2] = 1
    return {"empty": np.zeros((D, H, W), dtype=np.uint8), "full": np.ones((D, H, W), dtype=np.uint8), "single": single,
            "checkerboard": checkerboard(D, H, W), "serpentine": serpentine(D, H, W), "spiral": spiral(D, H, W),
            "comb": comb(D, H, W)}


def random_masks(N, D, H, W, density, seed):
    return (np.random.default_rng(seed).random((N, D, H, W)) < density).astype(np.uint8)


def ball(D, H, W, centre, radius):
    z, y, x = np.mgrid[:D, :H, :W]
    return (((z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2) <= radius ** 2).astype(np.uint8)
