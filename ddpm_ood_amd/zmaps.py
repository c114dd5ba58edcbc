"""Per-pixel Z-scores of the anomaly maps against the validation set (``reconstruct.py --anomaly_z_maps 1``).

The image-level score normalises every t-start's similarity by the validation set's mean and sample standard deviation at that
t before averaging over t (``ood.score``).  This module keeps the same statistics per (t, channel, pixel): ``MapStats`` is the
running mean / sum of squared deviations on the device (one ``ops.map_stats_update`` launch per validation batch), merged across
ranks on the host in float64 and finalised into the two fp32 tables ``ops.map_zscore`` reads.  Channels: 0 LPIPS, 1 squared error.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import ops

CHANNELS = ("lpips", "mse")
STATS_FILE = "map_stats.npz"
FLAG = "--anomaly_z_maps 1"
VOLUME_FLAG = "--anomaly_volume_z_maps 1"


def check_flags(spatial_dimension, vqvae_checkpoint, sigma: float = 0.0, rel_floor: float = 0.01):
    """What ``Reconstruct`` refuses at construction when the flag is on (no device needed)."""
    if int(spatial_dimension) != 2 or vqvae_checkpoint:
        raise ValueError(f"{FLAG}: Z-maps cover 2-D pixel-space models only (no --spatial_dimension 3, no --vqvae_checkpoint): "
                         f"2.5-D and latent maps are not built")
    if not float(sigma) >= 0.0:
        raise ValueError(f"{FLAG}: --anomaly_z_sigma must not be negative, got {sigma}")
    radius = int(4.0 * float(sigma) + 0.5)  # (ops.gaussian_taps: truncate 4)
    if radius > ops.MAP_BLUR_MAX_RADIUS:
        raise ValueError(f"{FLAG}: --anomaly_z_sigma {sigma} needs a radius of {radius} pixels, above the smoothing kernel's "
                         f"maximum of {ops.MAP_BLUR_MAX_RADIUS} (sigma < 4.125)")
    if not 0.0 < float(rel_floor) <= 1.0:
        raise ValueError(f"{FLAG}: --anomaly_z_std_floor must lie in (0, 1], got {rel_floor}")


def check_volume_flags(spatial_dimension, sigma: float = 0.0, rel_floor: float = 0.01):
    """The same for ``--anomaly_volume_z_maps 1``: volumes only, with or without a VQ-VAE; the smoothing is 3-D."""
    if int(spatial_dimension) != 3:
        raise ValueError(f"{VOLUME_FLAG}: Z-maps of volumes need --spatial_dimension 3 (2-D images: {FLAG})")
    if not float(sigma) >= 0.0:
        raise ValueError(f"{VOLUME_FLAG}: --anomaly_z_sigma must not be negative, got {sigma}")
    radius = int(4.0 * float(sigma) + 0.5)
    if radius > ops.MAP_BLUR_MAX_RADIUS:
        raise ValueError(f"{VOLUME_FLAG}: --anomaly_z_sigma {sigma} needs a radius of {radius} voxels, above the smoothing kernel's "
                         f"maximum of {ops.MAP_BLUR_MAX_RADIUS} (sigma < 4.125)")
    if not 0.0 < float(rel_floor) <= 1.0:
        raise ValueError(f"{VOLUME_FLAG}: --anomaly_z_std_floor must lie in (0, 1], got {rel_floor}")


def std_floor(std, rel_floor: float):
    """floor[t, c] = rel_floor * the largest std of that (t, c) over the pixels (voxels), float64 [n_t, 2, 1, 1(, 1)], from the fp32
    std table [n_t, 2, *extent] (an image's H, W or a volume's D, H, W):
    the absolute floor of the divisor.  ``finalize_tables`` (the in / out sets) and ``MapStats.floor`` (the leave-one-out Z-maps of
    the validation set) both take it from here."""
    std = np.asarray(std, dtype=np.float32)
    if std.ndim not in (4, 5):
        raise ValueError(f"map statistics want a [n_t, 2, H, W] std table, got {std.shape}")
    top = std.astype(np.float64).max(axis=tuple(range(2, std.ndim)), keepdims=True)
    if not np.isfinite(top).all() or (top <= 0).any():
        flat = top.reshape(top.shape[:2])
        bad = [(int(t), CHANNELS[int(c)]) for t, c in zip(*np.nonzero(~(flat > 0) | ~np.isfinite(flat)))]
        raise ValueError(f"map statistics: no pixel of (t index, channel) {bad} varies over the validation set (largest std 0 or "
                         f"not finite): nothing to normalise by")
    return float(rel_floor) * top


def finalize_tables(mean, std, rel_floor: float):
    """(mean fp32, inv_std fp32) from the fp32 tables ``map_stats.npz`` holds: inv_std = 1 / max(std, floor[t, c]) with
    floor[t, c] = rel_floor * the largest std of that (t, c) over the pixels, in float64, rounded once.  Both a run's own validation
    pass and a run that loads the file come through here with the same fp32 arrays, so they divide by the same bits."""
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    if mean.shape != std.shape or mean.ndim not in (4, 5):
        raise ValueError(f"map statistics want two [n_t, 2, H, W] tables, got {mean.shape} and {std.shape}")
    inv = 1.0 / np.maximum(std.astype(np.float64), std_floor(std, rel_floor))
    return mean, inv.astype(np.float32)


class MapStats:
    """n, mean and m2 (the sum of squared deviations) of the per-t maps [n_t, 2, H, W] over the validation rows seen so far
    (volumes: [n_t, 2, D, H, W] throughout; every formula is per column, only the floor looks at the extent).
    Running: the two tables are device tensors, ``update`` is one kernel call.  ``from_tables`` / ``load``: host tables."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, None, None
        self.t_values = None
        self._std32 = None  # (a loaded file: the fp32 std it holds, what ``finalize`` must use to reproduce the writer's bits)

    # ---- running, on the device
    def update(self, values):
        """values: [B, n_t, 2, H, W] on the device, the rows to be counted (the caller leaves non-finite images out)."""
        if values.ndim not in (5, 6) or values.shape[2] != 2:  # ([B, n_t, 2, D, H, W]: volumes)
            raise ValueError(f"MapStats.update wants [B, n_t, 2, H, W] values, got {tuple(values.shape)}")
        if self.mean is None:
            self.mean = torch.empty(tuple(values.shape[1:]), dtype=torch.float32, device=values.device)
            self.m2 = torch.empty_like(self.mean)
        elif not isinstance(self.mean, torch.Tensor):
            raise ValueError("MapStats.update: these statistics are host tables (loaded or merged), not a running accumulator")
        self.n = ops.map_stats_update(values, self.n, self.mean, self.m2)
        return self.n

    # ---- host tables
    def tables(self):
        """(n, mean, m2) with float64 numpy tables."""
        if self.mean is None:
            return 0, None, None
        as64 = (lambda a: a.detach().cpu().double().numpy()) if isinstance(self.mean, torch.Tensor) else np.asarray
        return int(self.n), as64(self.mean).astype(np.float64), as64(self.m2).astype(np.float64)

    @classmethod
    def from_tables(cls, n, mean, m2, t_values=None):
        s = cls()
        s.n, s.mean, s.m2 = int(n), np.asarray(mean, dtype=np.float64), np.asarray(m2, dtype=np.float64)
        s.t_values = None if t_values is None else [int(t) for t in t_values]
        return s

    @staticmethod
    def merge(parts):
        """Chan's merge of [(n, mean, m2), ...] in float64 on the host, in the list's order; parts with n = 0 are passed over.
        Pure: returns (n, mean, m2) and changes nothing."""
        n, mean, m2 = 0, None, None
        for nb, mb, qb in parts:
            nb = int(nb)
            if nb == 0:
                continue
            mb, qb = np.asarray(mb, dtype=np.float64), np.asarray(qb, dtype=np.float64)
            if n == 0:
                n, mean, m2 = nb, mb.copy(), qb.copy()
                continue
            if mb.shape != mean.shape:
                raise ValueError(f"MapStats.merge: tables of {mb.shape} and {mean.shape}")
            tot = n + nb
            delta = mb - mean
            mean = mean + delta * (nb / tot)
            m2 = m2 + qb + delta * delta * (n * nb / tot)
            n = tot
        return n, mean, m2

    def std(self):
        """The un-floored sample standard deviation (ddof = 1, as pandas' in ``ood.score``), float64 rounded once to fp32."""
        if self._std32 is not None:
            return self._std32
        n, _, m2 = self.tables()
        if n < 2:
            raise ValueError(f"map statistics of {n} validation image(s): a sample standard deviation needs at least 2")
        return np.sqrt(m2 / (n - 1)).astype(np.float32)

    def finalize(self, rel_floor: float = 0.01):
        """(mean, inv_std) as fp32 [n_t, 2, H, W]: ``finalize_tables`` of the fp32 mean and std."""
        std = self.std()
        return finalize_tables(self.tables()[1].astype(np.float32), std, rel_floor)

    def floor(self, rel_floor: float = 0.01):
        """The absolute floor of the divisor per (t, channel), fp32 [n_t, 2]: ``std_floor`` of the fp32 std, rounded once -- what
        ``ops.map_zscore_loo`` takes, and the number ``finalize`` floors the in / out sets' divisor at."""
        floor = std_floor(self.std(), rel_floor)
        return floor.reshape(floor.shape[:2]).astype(np.float32)

    def save(self, path, t_values, rel_floor: float = 0.01):
        n, mean, _ = self.tables()
        np.savez(path, t=np.asarray([int(t) for t in t_values], dtype=np.int64), n=np.int64(n), mean=mean.astype(np.float32),
                 std=self.std(), channels=np.asarray(CHANNELS), rel_floor=np.float64(rel_floor))

    @classmethod
    def load(cls, path, t_values=None, extent=None):
        """The statistics of a ``map_stats.npz``.  ``t_values`` / ``extent`` = (H, W) given: a file written for another list of
        t-starts or another image extent is a ValueError."""
        path = Path(path)
        if not path.exists():
            raise FileNotFoundError(f"{FLAG}: no validation pass in this run and no {path}: run with --run_val 1 first")
        with np.load(path) as z:
            t, n, mean, std = [int(v) for v in z["t"]], int(z["n"]), z["mean"].astype(np.float32), z["std"].astype(np.float32)
        if mean.ndim not in (4, 5) or mean.shape != std.shape or mean.shape[:2] != (len(t), 2):
            raise ValueError(f"{path}: tables of {mean.shape} / {std.shape} for {len(t)} t-starts are no map statistics")
        if t_values is not None and [int(v) for v in t_values] != t:
            raise ValueError(f"{path} holds the t-starts {t}, this run has {[int(v) for v in t_values]}")
        if extent is not None and tuple(int(e) for e in extent) != mean.shape[2:]:
            raise ValueError(f"{path} holds maps of {mean.shape[2:]}, this run's images are {tuple(int(e) for e in extent)}")
        s = cls.from_tables(n, mean, std.astype(np.float64) ** 2 * max(n - 1, 0), t)
        if n >= 2:
            s._std32 = std
        return s
