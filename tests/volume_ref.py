"""Float64 restatements for the anomaly maps of volumes, built from the 2-D ones of tests/anomaly_ref.py and
tests/zmap_ref.py: the LPIPS map of a volume from its slices along one axis, and the separable 3-D smoothing in the library's pass
order (H, then W, then D).  No import from the product.
"""

import numpy as np
import torch

import anomaly_ref
import zmap_ref


def plane_of(volume_shape, axis):
    """The extent of a slice along ``axis`` (2, 3 or 4 of [N, C, D, H, W]) of a (D, H, W) volume: [H, W], [D, W] or [D, H]."""
    return tuple(e for i, e in enumerate(volume_shape) if i != axis - 2)


def slices_to_volume(per_slice, n, axis):
    """[N * S, p, q] (volume-major) -> [N, D, H, W]: the slice index goes back to its axis."""
    return per_slice.reshape((n, -1) + tuple(per_slice.shape[1:])).movedim(1, axis - 1)


def volume_to_slices(vol, axis):
    """[N, C, D, H, W] -> [N * S, C, p, q], the slices of ``_calculate_fake_3d_loss``: permute(0, axis, 1, rest), view."""
    rest = [d for d in (2, 3, 4) if d != axis]
    v = vol.permute(0, axis, 1, *rest).contiguous()
    return v.view(-1, *v.shape[2:])


def upsample_view(maps, layer_sizes, volume_shape, axis, weight=1.0, out=None):
    """out (+)= weight * the 2-D ``anomaly_ref.upsample_sum`` of every slice's packed row, permuted back into [N, D, H, W]."""
    per_slice = anomaly_ref.upsample_sum(maps, layer_sizes, plane_of(volume_shape, axis))
    n = maps.shape[0] // volume_shape[axis - 2]
    total = weight * slices_to_volume(per_slice, n, axis)
    return total if out is None else out.double() + total


def blur3d(vols, taps):
    """[N, D, H, W]: ``zmap_ref.blur`` (the H pass, then the W pass) over the N D planes, then out[d] = sum_k taps[k]
    tmp[refl(d + k - r, D)]."""
    x = np.asarray(vols, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    N, D, H, W = x.shape
    r = len(taps) // 2
    tmp = zmap_ref.blur(x.reshape(N * D, H, W), taps).reshape(N, D, H, W)
    rows = np.array([[zmap_ref.refl(d + k - r, D) for k in range(len(taps))] for d in range(D)])  # [D, K]
    return np.einsum("ndkyx,k->ndyx", tmp[:, rows], taps)


def floor_inv_std(std, rel_floor):
    """``zmap_ref.floor_inv_std`` for a table [n_t, 2, *extent]: the floor is taken over every pixel or voxel of a (t, c)."""
    std = np.asarray(std, dtype=np.float64)
    flat = std.reshape(std.shape[:2] + (1, -1))
    return zmap_ref.floor_inv_std(flat, rel_floor).reshape(std.shape)


def as_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a))
