"""CPU: the host side of the voxel metrics of volumes -- the flags and every refusal from the Namespace alone, the
synthetic kind lesion3d and its masks, 3-D masks through ``load_masks``, the batch budget, the reference of the GPU tests held
against a plain union-find, and the refusals of the new entry points (a refusal launches nothing, so it needs no device)."""

import argparse
import ctypes as C
import re

import numpy as np
import pytest
import torch

import voxel_ref as ref

ON = dict(spatial_dimension=3, vqvae_checkpoint=None, anomaly_volume_z_maps=1, voxel_metrics=1, out_ids="a.csv,b.csv", run_out=1)


def _settings(**kw):
    from ddpm_ood_amd.voxel_passes import VoxelSettings

    return VoxelSettings.from_args(argparse.Namespace(**kw))


def test_voxel_flags_parse_and_default_off():
    import reconstruct as cli
    from ddpm_ood_amd.map_passes import MapPipeline, MapSettings
    from ddpm_ood_amd.voxel_passes import VoxelSettings

    args = cli.parse_args([])
    assert (args.voxel_metrics, args.voxel_regions, args.voxel_connectivity, args.voxel_pro_fpr) == (0, 0, 26, 0.3)
    off = VoxelSettings.from_args(args)
    assert off == VoxelSettings() and not off.metrics and not off.regions
    pipeline = MapPipeline(MapSettings.from_args(args), "cpu", ".", voxel=off)
    assert pipeline.voxel is None and pipeline.layout is None and MapPipeline(MapSettings(), "cpu", ".").voxel is None
    args = cli.parse_args(["--spatial_dimension", "3", "--anomaly_volume_z_maps", "1", "--voxel_metrics", "1", "--voxel_regions", "1",
                           "--voxel_connectivity", "18", "--voxel_pro_fpr", "0.1", "--out_ids", "a.csv,b.csv", "--out_masks", "auto,",
                           "--pixel_bins", "64", "--pixel_range", "-4", "12", "--pixel_thresholds", "1.5,2"])
    s = VoxelSettings.from_args(args)
    assert s.metrics and s.regions and (s.connectivity, s.pro_fpr, s.lo, s.hi, s.bins) == (18, 0.1, -4.0, 12.0, 64)
    assert s.thresholds == [1.5, 2.0] and s.masks == ["auto", None]
    assert not MapSettings.from_args(args).pixel_metrics  # the 2-D settings stay what the command line said
    pipeline = MapPipeline(MapSettings.from_args(args), "cpu", ".", voxel=s)
    assert [n for n, _ in pipeline.layout.segments] == ["counts", "mask_pixels", "components", "regions"] and pipeline.layout.width == 2 * 13
    plain = _settings(**ON)
    assert plain.metrics and not plain.regions and plain.connectivity is None and plain.masks == [None, None]
    assert (plain.lo, plain.hi, plain.bins, plain.thresholds) == (-16.0, 48.0, 4096, [2.0, 3.0, 4.0])
    assert _settings(**ON, voxel_regions=1).connectivity == 26


def test_every_refusal_comes_from_the_namespace_alone():
    from ddpm_ood_amd.trainer import Reconstruct

    cases = [
        (dict(ON, spatial_dimension=2), "--spatial_dimension 3"),                      # 2-D
        (dict(ON, anomaly_volume_z_maps=0), "--anomaly_volume_z_maps 1"),              # no Z-maps
        (dict(ON, voxel_metrics=0, voxel_regions=1), "--voxel_metrics 1"),             # regions without metrics
        (dict(ON, voxel_regions=1, voxel_connectivity=8), "--voxel_connectivity"),     # another connectivity
        (dict(ON, voxel_regions=1, voxel_connectivity=4), "--voxel_connectivity"),
        (dict(ON, voxel_regions=1, voxel_connectivity="many"), "--voxel_connectivity"),
        (dict(ON, voxel_regions=1, voxel_pro_fpr=0.0), "--voxel_pro_fpr"),
        (dict(ON, pixel_metrics=1), "--pixel_metrics"),                                # a voxel flag beside a 2-D pixel flag
        (dict(ON, pixel_regions=1), "--pixel_regions"),
        (dict(ON, pixel_calibrate_fpr="0.05"), "--pixel_calibrate_fpr"),
        (dict(ON, pixel_segment=1), "--pixel_segment"),
        (dict(ON, spatial_dimension=2, anomaly_volume_z_maps=0, anomaly_z_maps=1, pixel_metrics=1), "--pixel_metrics"),
        (dict(ON, image_size=1291), "2^31"),                                           # 1291^3 >= 2^31
        (dict(ON, image_roi=(2048, 1024, 1024)), "2^31"),
        (dict(ON, out_masks="auto"), "--out_masks"),                                   # one entry for two sets
        (dict(ON, pixel_bins=9000), "--pixel_bins"),
        (dict(ON, pixel_thresholds="1,2,3,4,5,6,7,8,9"), "--pixel_thresholds"),
    ]
    for kw, match in cases:
        with pytest.raises(ValueError, match=re.escape(match)) as e:
            _settings(**kw)
        assert "--voxel_" in str(e.value), str(e.value)  # named by the flag
        with pytest.raises(ValueError):  # the constructor runs the check before any device, library or checkpoint
            Reconstruct(argparse.Namespace(**kw))
    assert _settings(**dict(ON, image_size=1290)).metrics and _settings(**dict(ON, image_roi=(128, -1, 128))).metrics
    # the four 2-D flags stay refused beside a volume flag, with the message they have
    from ddpm_ood_amd.map_passes import MapSettings

    with pytest.raises(ValueError, match="is not built for volumes"):
        MapSettings.from_args(argparse.Namespace(**dict(ON, pixel_metrics=1)))


def test_lesion3d_follows_lesion():
    from ddpm_ood_amd import data

    n, size, seed, mix = 3, 24, 5, 30
    x = data.synthetic_images("lesion3d", n, 1, size, seed, mix)
    m = data.synthetic_masks("lesion3d", n, 1, size, seed, mix)
    base = data.synthetic_images("blobs3d", n, 1, size, seed, mix)
    assert x.shape == base.shape == (n, 1, size, size, size) and m.shape == x.shape and m.dtype == torch.uint8
    assert torch.equal(x[m == 0], base[m == 0])  # bit-equal to blobs3d outside the ball: nothing rescaled
    assert torch.equal((x != base).to(torch.uint8), m)  # the mask is the changed voxels (uniform noise never equals the blob value here)
    r = data.lesion_radius(size, mix)
    assert abs(r - 3.6) < 1e-12  # 30 % of 24 voxels across
    for k in range(n):
        idx = torch.nonzero(m[k, 0]).double()
        centre = idx.mean(dim=0)
        assert ((idx - centre).norm(dim=1) <= r + 1.0).all() and idx.min() >= 0 and idx.max() <= size - 1
        lo, hi = idx.min(dim=0).values, idx.max(dim=0).values
        assert (hi - lo + 1 >= 2 * int(r) - 1).all() and (lo >= 0).all() and (hi <= size - 1).all()
        assert ref.label_volume(m[k, 0].numpy(), 6)[1] == 1  # one ball
        assert abs(int(m[k].sum()) - 4.0 / 3.0 * np.pi * r ** 3) < 0.35 * 4.0 / 3.0 * np.pi * r ** 3  # whole: not cut by the border
    # the generator order of _lesion: blobs, centres, noise -- a second call repeats it, another seed moves the ball
    assert torch.equal(data.synthetic_images("lesion3d", n, 1, size, seed, mix), x)
    assert not torch.equal(data.synthetic_masks("lesion3d", n, 1, size, seed + 1, mix), m)
    assert data.lesion_radius(32, 1) == 2.0 and int(data.synthetic_masks("lesion3d", 1, 1, 32, 0, 1).sum()) > 0  # radius at least 2
    assert int(data.synthetic_masks("blobs3d", 2, 1, 8).sum()) == 0
    imgs, names = data.load_ids("synthetic:lesion3d:n=2:size=16:seed=3:mix=40:name=LES3", spatial_dimension=3)
    assert len(imgs) == 2 and tuple(imgs[0].shape) == (1, 16, 16, 16) and names[0].startswith("lesion3d_3_")


def test_load_masks_for_volumes(tmp_path):
    from ddpm_ood_amd import data

    spec = "synthetic:lesion3d:n=3:size=12:seed=4:mix=50"
    loader = data.get_data_loader(spec, batch_size=2, is_grayscale=True, spatial_dimension=3, mask_ids="auto")
    want = data.synthetic_masks("lesion3d", 3, 1, 12, 4, 50)
    got = torch.cat([b["mask"] for b in loader])
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # .npz of [N, D, H, W], through the images' crop and flip
    rng = np.random.default_rng(0)
    vols = rng.random((3, 12, 10, 8)).astype(np.float32)
    masks = (rng.random((3, 12, 10, 8)) < 0.3).astype(np.uint8)
    np.savez(tmp_path / "vols.npz", images=vols[:, None])
    np.savez(tmp_path / "masks.npz", masks=masks)
    kw = dict(batch_size=3, is_grayscale=True, spatial_dimension=3)
    b = next(iter(data.get_data_loader(str(tmp_path / "vols.npz"), mask_ids=str(tmp_path / "masks.npz"), **kw)))
    assert torch.equal(b["mask"], torch.from_numpy(masks)[:, None])
    b = next(iter(data.get_data_loader(str(tmp_path / "vols.npz"), mask_ids=str(tmp_path / "masks.npz"), image_roi=(8, -1, 4),
                                       add_vflip=True, **kw)))
    assert tuple(b["image"].shape) == (3, 1, 8, 10, 4) == tuple(b["mask"].shape)
    assert torch.equal(b["mask"], torch.from_numpy(masks[:, 2:10, :, 2:6][:, ::-1].copy())[:, None])
    # a CSV of .npy volumes
    files, mfiles = [], []
    for k in range(2):
        np.save(tmp_path / f"v{k}.npy", vols[k])
        np.save(tmp_path / f"m{k}.npy", masks[k] * 7)  # (anything != 0 is inside)
        files.append(str(tmp_path / f"v{k}.npy"))
        mfiles.append(str(tmp_path / f"m{k}.npy"))
    (tmp_path / "ids.csv").write_text(",".join(files) + "\n")
    (tmp_path / "mask_ids.csv").write_text(",".join(mfiles) + "\n")
    b = next(iter(data.get_data_loader(str(tmp_path / "ids.csv"), mask_ids=str(tmp_path / "mask_ids.csv"), add_hflip=True, **kw)))
    assert torch.equal(b["mask"], torch.from_numpy(masks[:2, :, ::-1].copy())[:, None])
    with pytest.raises(ValueError, match="after the transforms"):
        np.savez(tmp_path / "short.npz", masks=masks[:, :, :, :4])
        data.get_data_loader(str(tmp_path / "vols.npz"), mask_ids=str(tmp_path / "short.npz"), **kw)
    with pytest.raises(ValueError, match="are not"):  # planes handed to a volume run
        np.savez(tmp_path / "planes.npz", masks=masks[:, 0])
        data.get_data_loader(str(tmp_path / "vols.npz"), mask_ids=str(tmp_path / "planes.npz"), **kw)


def test_the_budget_covers_the_voxel_steps():
    from ddpm_ood_amd import ops, voxel_passes as vp

    s = _settings(**ON, voxel_regions=1)
    B, n_t, extent = 2, 25, (128, 128, 128)
    P = 128 ** 3
    maps = B * n_t * 2 * P * 4
    mine = vp.batch_bytes(B, extent, s)
    # the mask and a channel's Z-map; labels; the forests of the mask and of the three thresholded maps dominate
    assert mine >= B * P * (1 + 4 + 4 + 4 + 3 * 4) and mine < B * P * 32
    # without regions: the mask, one channel's Z-map, 256 histogram slabs, two channels' counts
    assert vp.batch_bytes(B, extent, _settings(**ON)) == B * P * 5 + 256 * 2 * 4097 * 4 + 2 * 12 * B * 3
    assert vp.check_budget(B, n_t, extent, s, 8 << 30) == maps + mine
    with pytest.raises(ValueError, match=re.escape("--anomaly_volume_budget_gb")) as e:
        vp.check_budget(B, n_t, extent, s, maps + mine - 1)
    assert "--voxel_regions 1" in str(e.value) and "--batch_size" in str(e.value) and "128 x 128 x 128" in str(e.value)
    with pytest.raises(ValueError, match=re.escape("--voxel_metrics 1")):
        vp.check_budget(B, n_t, extent, _settings(**ON), maps)
    with pytest.raises(ValueError, match="2\\^31"):
        vp.check_budget(1, 1, (2048, 1024, 1024), s, 1 << 60)
    # the restated sizes are the library's
    for (b, d, h, w, k) in ((1, 1, 1, 1, 1), (2, 3, 5, 7, 3), (3, 17, 33, 65, 8), (1, 128, 128, 128, 3)):
        p = d * h * w
        assert vp.label_scratch_bytes(b, p) == ops.map_label3d_scratch_bytes(b, d, h, w)
        assert vp.counts_scratch_bytes(b, k, p) == ops.map_component_counts3d_scratch_bytes(b, d, h, w, k)
        for bins, chunk in ((64, 7), (4096, None)):
            assert vp.overlap_scratch_bytes(b, bins, chunk or ops.map_region_overlap3d_chunk(bins)) == ops.map_region_overlap3d_scratch_bytes(b, bins, chunk)
    assert ops.map_label3d_scratch_bytes(1, 2048, 1024, 1024) == 0 and ops.map_component_counts3d_scratch_bytes(1, 4, 4, 4, 9) == 0


def test_scipy_reference_equals_the_plain_union_find():
    for extent in ((1, 1, 1), (3, 5, 7), (2, 3, 17), (6, 6, 6)):
        shapes = dict(ref.named_shapes(*extent))
        for d in (0.05, 0.3, 0.6):
            shapes[f"random{d}"] = ref.random_masks(1, *extent, d, seed=int(d * 100))[0]
        for name, m in shapes.items():
            for conn in (6, 18, 26):
                a, b = ref.label_volume(m, conn), ref.label_plain(m, conn)
                assert a[1] == b[1] and np.array_equal(a[0], b[0]), (extent, name, conn)
    for kind, joined_from in (("face", 6), ("edge", 18), ("corner", 26)):
        m = ref.two_cubes(kind)
        assert [ref.label_plain(m, c)[1] for c in (6, 18, 26)] == [1 if c >= joined_from else 2 for c in (6, 18, 26)]
    assert ref.label_volume(ref.serpentine(5, 6, 7), 6)[1] == 1 and ref.label_volume(ref.spiral(5, 9, 9), 6)[1] == 1
    assert ref.label_volume(ref.comb(4, 5, 5), 26)[1] == 1 and ref.label_volume(ref.comb(4, 5, 5)[:3], 26)[1] == 9
    assert ref.label_volume(ref.checkerboard(8, 8, 8), 6)[1] == 256 and ref.label_volume(ref.checkerboard(8, 8, 8), 18)[1] == 1


def test_every_refusal_of_the_entry_points_returns_minus_one():
    """Argument checks come before any launch: no device is needed to see them."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    A, B_, C_, D_, E_, F_, G_ = (1 << 20, 1 << 24, 1 << 26, 1 << 28, 1 << 30, 1 << 32, 1 << 34)  # disjoint fake device addresses

    def label(masks=A, N=1, D=4, H=4, W=4, conn=26, labels=B_, regions=C_, scratch=D_, f32=False):
        if f32:
            return lib.ddpm_map_label3d_f32(masks, 0.0, N, D, H, W, conn, labels, regions, scratch, None)
        return lib.ddpm_map_label3d_u8(masks, N, D, H, W, conn, labels, regions, scratch, None)

    for f32 in (False, True):
        name = b"map_label3d_f32" if f32 else b"map_label3d_u8"
        for kw, what in ((dict(masks=None), b"null"), (dict(labels=None), b"null"), (dict(regions=None), b"null"), (dict(scratch=None), b"null"),
                         (dict(conn=8), b"connectivity"), (dict(conn=4), b"connectivity"), (dict(conn=0), b"connectivity"),
                         (dict(D=0), b"positive"), (dict(W=-1), b"positive"), (dict(N=0), b"positive"), (dict(D=2048, H=1024, W=1024), b"2^31"),
                         (dict(N=65536), b"65535"), (dict(labels=B_ + 2), b"aligned"), (dict(scratch=D_ + 1), b"aligned"),
                         (dict(regions=C_ + 3), b"aligned"), (dict(labels=A), b"alias"), (dict(regions=B_ + 16), b"alias"),
                         (dict(scratch=B_ + 64), b"alias"), (dict(scratch=C_ - 64), b"alias"), (dict(scratch=A - 128), b"alias")):
            assert label(f32=f32, **kw) == -1, kw
            assert name in lib.ddpm_last_error() and what in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())
    assert lib.ddpm_map_label3d_f32(A + 2, 0.0, 1, 4, 4, 4, 26, B_, C_, D_, None) == -1 and b"aligned" in lib.ddpm_last_error()

    def overlap(maps=A, labels=B_, regions=C_, N=2, P=64, lo=-16.0, inv=1.0, nbins=64, chunk=4, scratch=D_, total=E_):
        return lib.ddpm_map_region_overlap3d_f32(maps, labels, regions, N, P, lo, inv, nbins, chunk, scratch, total, 0, None)

    for kw, what in ((dict(maps=None), b"null"), (dict(scratch=None), b"null"), (dict(total=None), b"null"), (dict(N=0), b"positive"),
                     (dict(P=0), b"2^31"), (dict(P=1 << 31), b"2^31"), (dict(nbins=0), b"nbins"), (dict(nbins=8192), b"nbins"),
                     (dict(chunk=0), b"chunk_regions"), (dict(chunk=65537), b"chunk_regions"), (dict(inv=0.0), b"inv_step"),
                     (dict(lo=float("nan")), b"lo must"), (dict(scratch=D_ + 4), b"aligned"), (dict(total=E_ + 4), b"aligned"),
                     (dict(labels=B_ + 1), b"aligned"), (dict(total=A + 8), b"alias"), (dict(scratch=B_), b"alias"),
                     (dict(total=D_ + 64), b"alias"), (dict(scratch=E_ - 8), b"alias")):
        assert overlap(**kw) == -1, kw
        assert b"map_region_overlap3d" in lib.ddpm_last_error() and what in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())

    def counts(maps=A, masks=B_, labels=C_, regions=D_, N=1, D=4, H=4, W=4, thr=E_, K=2, conn=26, out=F_, scratch=G_):
        return lib.ddpm_map_component_counts3d_f32(maps, masks, labels, regions, N, D, H, W, thr, K, conn, out, scratch, None)

    for kw, what in ((dict(maps=None), b"null"), (dict(thr=None), b"null"), (dict(out=None), b"null"), (dict(scratch=None), b"null"),
                     (dict(K=0), b"K must"), (dict(K=9), b"K must"), (dict(conn=8), b"connectivity"), (dict(H=0), b"positive"),
                     (dict(D=2048, H=1024, W=1024), b"2^31"), (dict(N=8192, K=8), b"65535"), (dict(out=F_ + 2), b"aligned"),
                     (dict(scratch=G_ + 2), b"aligned"), (dict(maps=A + 1), b"aligned"), (dict(out=A + 8), b"alias"), (dict(out=E_), b"alias"),
                     (dict(scratch=C_), b"alias"), (dict(scratch=F_ - 16), b"alias"), (dict(out=G_ + 32), b"alias")):
        assert counts(**kw) == -1, kw
        assert b"map_component_counts3d" in lib.ddpm_last_error() and what in lib.ddpm_last_error(), (kw, lib.ddpm_last_error())
    sigs = _lib.SIGNATURES
    assert sigs["ddpm_map_label3d_u8"][1].count(C.c_void_p) == 5 and sigs["ddpm_map_region_overlap3d_f32"][1][4] is C.c_int64
