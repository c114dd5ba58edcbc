"""numpy restatements of the region-metrics kernels (csrc/regions.hip), for the tests.

``label``: a plain union-find over one plane; label 0 is the background and the components are numbered 1 .. R in ascending
order of their smallest flat pixel index (the numbering of ``scipy.ndimage.label`` with the cross for connectivity 4 and the
3 x 3 structure for 8).  ``overlap``: per region and bin by brute force from the float32 bin rule of pixel_ref.py, in float64,
in the contract's order (regions ascending within an image, then one addition per image).  ``component_counts``: hit / pred /
false_pred.  ``aupro_direct``: the maps thresholded at every bin edge and each region's overlap measured directly."""

import numpy as np

import pixel_ref


def label_plane(inside, connectivity=8):
    """(labels int32 [H, W], R) of one boolean plane."""
    inside = np.asarray(inside, dtype=bool)
    H, W = inside.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    steps = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for y in range(H):
        for x in range(W):
            if not inside[y, x]:
                continue
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and inside[yy, xx]:
                    a, b = find(y * W + x), find(yy * W + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)  # (the root is the smallest flat index of its tree)
    labels = np.zeros(H * W, dtype=np.int32)
    number = {}
    for i in range(H * W):  # ascending flat index: a component is first met at its smallest pixel, its root
        if inside.reshape(-1)[i]:
            labels[i] = number.setdefault(find(i), len(number) + 1)
    return labels.reshape(H, W), len(number)


def label(x, connectivity=8, threshold=None):
    """(labels int32 [N, H, W], regions int32 [N]): of x != 0, or of x > threshold in float32 (NaN outside)."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        inside = x != 0 if threshold is None else x.astype(np.float32) > np.float32(threshold)
    got = [label_plane(p, connectivity) for p in inside]
    return np.stack([g[0] for g in got]), np.asarray([g[1] for g in got], dtype=np.int32)


def overlap_rows(maps, labels, regions, lo, hi, nbins):
    """float64 [N, nbins + 1]: w_n[b] = sum over r = 1 .. R_n ascending of h_{n,r}[b] / area_{n,r}."""
    maps, labels = np.asarray(maps, dtype=np.float32), np.asarray(labels)
    N = maps.shape[0]
    bins = pixel_ref.bin_index(maps.reshape(N, -1), lo, hi, nbins)
    lab = labels.reshape(N, -1)
    out = np.zeros((N, nbins + 1), dtype=np.float64)
    for n in range(N):
        for r in range(1, int(regions[n]) + 1):
            sel = lab[n] == r
            area = int(sel.sum())
            if area:
                h = np.bincount(bins[n][sel], minlength=nbins + 1).astype(np.float64)
                out[n] = out[n] + h / np.float64(area)
    return out


def overlap(maps, labels, regions, lo, hi, nbins, total=None):
    """float64 [nbins + 1]: (total or 0) + w_0 + w_1 + ..., one addition per image in ascending order."""
    t = np.zeros(nbins + 1, dtype=np.float64) if total is None else np.asarray(total, dtype=np.float64).copy()
    for row in overlap_rows(maps, labels, regions, lo, hi, nbins):
        t = t + row
    return t


def overlap_bound(value, regions_total):
    """The issue's bound on one entry: at most R_total correctly rounded terms."""
    return (regions_total + 1) * 2.0 ** -52 * np.maximum(1.0, np.abs(value))


def component_counts(maps, masks, labels, regions, thresholds, connectivity=8):
    """int32 [N, K, 3]: hit (regions with a pixel v > thr), pred (components of v > thr), false_pred (those without a masked pixel)."""
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
            comp, R = label_plane(pred[n], connectivity)
            out[n, k, 1] = R
            out[n, k, 2] = R - len(np.setdiff1d(np.unique(comp[masks[n]]), [0]))
    return out


def pro_curve_direct(maps, masks, lo, hi, nbins, connectivity=8):
    """(fpr, pro) by thresholding, entry j for k = nbins - j: "predicted at k" = bin >= k (NaN pixels never predicted, and left
    out of the negatives); per k the mean over all regions of the predicted fraction of the region, and the FPR over the scored
    pixels outside every mask."""
    maps = np.asarray(maps, dtype=np.float32)
    N = maps.shape[0]
    labels, regions = label(np.asarray(masks).reshape(maps.shape), connectivity)
    bins = pixel_ref.bin_index(maps, lo, hi, nbins)
    scored = bins < nbins
    negatives = (labels == 0) & scored
    region_sets = [(n, labels[n] == r) for n in range(N) for r in range(1, int(regions[n]) + 1)]
    fpr, pro = [], []
    for k in range(nbins, -1, -1):
        pred = (bins >= k) & scored
        fpr.append((pred & negatives).sum() / negatives.sum())
        pro.append(np.mean([(pred[n] & sel).sum() / sel.sum() for n, sel in region_sets]))
    return np.asarray(fpr), np.asarray(pro)


def aupro_direct(maps, masks, lo, hi, nbins, connectivity=8, fpr_limit=0.3):
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


# ---- named shapes ---------------------------------------------------------------------------------------------------------------------

def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2 == 0).astype(np.uint8)


def diagonals(H, W, period=3):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % period == 0).astype(np.uint8)


def serpentine(H, W):
    """One-pixel-wide: every other row full, joined alternately at the right and the left end."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(H, W):
    """A one-pixel-wide spiral from the corner inwards, one free pixel between its turns."""
    m = np.zeros((H, W), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    for _ in range(4 * H * W):
        yy, xx = y + dy, x + dx
        ahead2 = (yy + dy, xx + dx)
        blocked = not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] or (
            0 <= ahead2[0] < H and 0 <= ahead2[1] < W and m[ahead2])
        if blocked:
            dy, dx = dx, -dy  # turn right
            yy, xx = y + dy, x + dx
            ahead2 = (yy + dy, xx + dx)
            if not (0 <= yy < H and 0 <= xx < W) or m[yy, xx] or (0 <= ahead2[0] < H and 0 <= ahead2[1] < W and m[ahead2]):
                break
        y, x = yy, xx
        m[y, x] = 1
    return m


def comb(H, W):
    """Teeth in every other column that join only in the last row."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[:, 0::2] = 1
    m[H - 1] = 1
    return m


def named_shapes(H, W):
    single = np.zeros((H, W), dtype=np.uint8)
    single[H // 2, W // 2] = 1
    return {"zero": np.zeros((H, W), dtype=np.uint8), "one": np.ones((H, W), dtype=np.uint8), "single": single,
            "checkerboard": checkerboard(H, W), "diagonals": diagonals(H, W), "serpentine": serpentine(H, W), "spiral": spiral(H, W),
            "comb": comb(H, W)}


def random_masks(N, H, W, density, seed):
    return (np.random.default_rng(seed).random((N, H, W)) < density).astype(np.uint8)
