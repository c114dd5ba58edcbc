"""CPU: the host side of the anomaly maps -- the C ABI of the three kernels and their argument checks, the CLI flag,
the float64 restatement's bilinear against ``F.interpolate``, ``gather_rows`` on a two-rank gloo group and the ordering of the
``.npz`` rows (tests/test_gpu_anomaly_maps.py runs the kernels)."""

import ctypes as C
import os
import re
import socket
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import anomaly_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("ddpm_sqerr_map_f32", "ddpm_lpips_layer_map_f32", "ddpm_lpips_map_upsample_f32")


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    return _lib.load()


def test_entry_points_are_declared_exported_bound_and_return_int(lib):
    from ddpm_ood_amd import _lib

    header = (ROOT / "include" / "ddpm_ood_hip.h").read_text()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int  # no workspace, no size function
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is C.c_int
        assert args[-1] is C.c_void_p  # the stream; every other void * is a device buffer
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and ("map" in n or "sqerr" in n)]
    assert lib.ddpm_abi_version() == 10 == _lib.ABI_VERSION  # additive entries: the ABI version stays
    assert "#define DDPM_ABI_VERSION 10" in header


FAKE = 0x10000  # never dereferenced: the argument checks come first


def test_sqerr_map_refuses_bad_arguments(lib):
    f = lib.ddpm_sqerr_map_f32
    far = FAKE + 4096
    for a, b, m in ((None, FAKE, far), (FAKE, None, far), (FAKE, FAKE, None)):
        assert f(a, b, m, 1, 1, 4, 1.0, 0, None) == -1 and b"null" in lib.ddpm_last_error()
    for B, Cc, S in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (-1, 1, 4), (1, -3, 4), (1, 1, -4)):
        assert f(FAKE, FAKE, far, B, Cc, S, 1.0, 0, None) == -1 and b"positive" in lib.ddpm_last_error()
    # map on an input, inside an input ([2, 3, 16] floats = 384 bytes), and an input inside the map
    for m in (FAKE, FAKE + 380, FAKE - 124):
        assert f(FAKE, FAKE + 8192, m, 2, 3, 16, 1.0, 0, None) == -1 and b"aliases" in lib.ddpm_last_error()
        assert f(FAKE + 8192, FAKE, m, 2, 3, 16, 1.0, 1, None) == -1 and b"aliases" in lib.ddpm_last_error()


def test_lpips_layer_map_refuses_bad_arguments(lib):
    f = lib.ddpm_lpips_layer_map_f32
    ok = [FAKE, FAKE + 4096, FAKE + 8192, FAKE + 12288]
    for k in range(4):
        ptrs = list(ok)
        ptrs[k] = None
        assert f(*ptrs, 2, 8, 9, 9, 0, None) == -1 and b"null" in lib.ddpm_last_error()
    for N, Cc, HW in ((0, 8, 9), (2, 0, 9), (2, 8, 0), (-2, 8, 9)):
        assert f(*ok, N, Cc, HW, 9, 0, None) == -1 and b"positive" in lib.ddpm_last_error()
    for stride, offset in ((8, 0), (9, 1), (20, -1), (20, 12)):  # the layer has to lie inside the row
        assert f(*ok, 2, 8, 9, stride, offset, None) == -1 and b"do not fit" in lib.ddpm_last_error()
    assert f(FAKE, FAKE + 4096, FAKE + 8192, FAKE + 16, 2, 8, 9, 9, 0, None) == -1 and b"aliases" in lib.ddpm_last_error()


def _upsample(lib, maps, out, n_layers=5, sizes=((7, 7), (3, 3), (1, 1), (1, 1), (1, 1)), full=(32, 32), window=(0, 0, 32, 32),
              N=2, row_stride=61):
    flat = [v for s in sizes for v in s]
    return lib.ddpm_lpips_map_upsample_f32(maps, out, N, row_stride, n_layers, *flat, *full, *window, 1.0, 0, None)


def test_lpips_map_upsample_refuses_bad_arguments(lib):
    far = FAKE + (1 << 20)
    assert _upsample(lib, None, far) == -1 and b"null" in lib.ddpm_last_error()
    assert _upsample(lib, FAKE, None) == -1 and b"null" in lib.ddpm_last_error()
    assert _upsample(lib, FAKE, far, N=0) == -1
    for n_layers in (0, 6, -1):
        assert _upsample(lib, FAKE, far, n_layers=n_layers) == -1 and b"n_layers" in lib.ddpm_last_error()
    for k in range(5):  # a zero extent in any layer that is used
        sizes = [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
        sizes[k] = (sizes[k][0], 0)
        assert _upsample(lib, FAKE, far, sizes=sizes) == -1 and f"layer {k}".encode() in lib.ddpm_last_error()
        sizes[k] = (0, 3)
        assert _upsample(lib, FAKE, far, sizes=sizes) == -1 and f"layer {k}".encode() in lib.ddpm_last_error()
    assert _upsample(lib, FAKE, far, row_stride=60) == -1 and b"do not fit" in lib.ddpm_last_error()  # 49 + 9 + 3 = 61
    for window in ((0, 0, 33, 32), (0, 0, 32, 33), (5, 0, 28, 28), (0, 5, 28, 28), (-1, 0, 28, 28), (0, -1, 28, 28),
                   (0, 0, 0, 28), (0, 0, 28, 0)):
        assert _upsample(lib, FAKE, far, window=window) == -1 and b"outside the full grid" in lib.ddpm_last_error()
    assert _upsample(lib, FAKE, far, full=(0, 32), window=(0, 0, 1, 1)) == -1
    assert _upsample(lib, FAKE, FAKE + 64) == -1 and b"aliases" in lib.ddpm_last_error()


def test_cli_flag_defaults_to_off_and_likelihood_accepts_it():
    import likelihood as lcli
    import reconstruct as cli

    assert cli.parse_args([]).anomaly_maps == 0
    assert cli.parse_args(["--anomaly_maps", "1"]).anomaly_maps == 1
    assert lcli.parse_args(["--anomaly_maps", "1"]).anomaly_maps == 1  # inherited with the parser; the bound has no maps


def test_perceptual_loss_spatial_in_3d_is_refused_not_ignored():
    from ddpm_ood_amd.perceptual import LPIPS, PerceptualLoss

    with pytest.raises(NotImplementedError, match="2.5-D maps"):
        PerceptualLoss(3, spatial=True)
    assert PerceptualLoss(2, spatial=True).perceptual_function.spatial is True
    assert PerceptualLoss(2).perceptual_function.spatial is False and PerceptualLoss(3).perceptual_function.spatial is False
    assert LPIPS.pyramid_sizes(32, 32) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)] == ref.pyramid_sizes(32, 32)
    assert LPIPS.pyramid_sizes(64, 48) == [(15, 11), (7, 5), (3, 2), (3, 2), (3, 2)] == ref.pyramid_sizes(64, 48)
    assert LPIPS.pyramid_sizes(32, 24)[2] == (1, 0) and LPIPS.pyramid_sizes(32, 24) == ref.pyramid_sizes(32, 24)  # 5 -> 2 -> 0


@pytest.mark.parametrize("src,dst", [((7, 7), (32, 32)), ((3, 3), (32, 32)), ((1, 1), (32, 32)), ((15, 11), (64, 48)),
                                     ((7, 5), (64, 48)), ((3, 2), (64, 48)), ((5, 3), (9, 7)), ((8, 8), (8, 8))])
def test_restated_bilinear_equals_interpolate(src, dst):
    g = torch.Generator().manual_seed(src[0] * 100 + dst[0])
    m = torch.rand(3, *src, generator=g, dtype=torch.float64)
    want = F.interpolate(m[:, None], size=dst, mode="bilinear", align_corners=False)[:, 0]
    got = ref.bilinear(m, dst)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 2e-15
    if src == dst:
        assert torch.equal(got, m)  # the identity comes out exact
    if src == (1, 1):
        assert float((got - m.expand(-1, *dst)).abs().max()) <= 2e-16  # a 1 x 1 layer: a constant map of its value


def test_restated_upsample_sum_windows_weights_and_accumulates():
    g = torch.Generator().manual_seed(4)
    sizes = [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    maps = torch.rand(2, 70, generator=g, dtype=torch.float64)  # (a row_stride larger than the 61 the layers use)
    full = ref.upsample_sum(maps, sizes, (32, 32))
    want = sum(F.interpolate(m[:, None], size=(32, 32), mode="bilinear", align_corners=False)[:, 0]
               for m in ref.unpack(maps, sizes))
    assert float((full - want).abs().max()) <= 1e-14
    base = torch.rand(2, 28, 28, generator=g, dtype=torch.float64)
    got = ref.upsample_sum(maps, sizes, (32, 32), window=(2, 2, 28, 28), weight=0.25, out=base)
    assert torch.equal(got, base + 0.25 * full[:, 2:30, 2:30])


def test_map_rows_follow_the_csv_order_of_first_appearance():
    """Two ranks, batches of two: rank 0 holds images 0 2 4 (batches [0, 2], [4]), rank 1 images 1 3 ([1, 3]).  The CSV goes rank
    by rank, batch by batch, t by t, image by image; the .npz rows follow the filenames' first appearance there."""
    from ddpm_ood_amd.trainer import map_rows_in_csv_order, rows_from_scores

    ids = [0, 2, 4, 1, 3]  # gathered rank-major
    name_of = {0: "/d/zero.png", 1: "/d/one.nii.gz", 2: "/d/two.npy", 3: "/d/three.png", 4: "/d/four.png"}
    scores = torch.zeros(5, 2, 2).numpy()
    results = rows_from_scores(ids, scores, [3, 2], [10, 50], name_of, 2, "in")
    assert [r["filename"] for r in results] == (["zero", "two"] * 2 + ["four"] * 2 + ["one", "three"] * 2)
    stems, picks = map_rows_in_csv_order(results, ids, name_of)
    assert stems == ["zero", "two", "four", "one", "three"] and picks == [0, 1, 2, 3, 4]
    # the gathered maps in another order than the rows (and one image twice): every stem picks its first row
    stems, picks = map_rows_in_csv_order(results, [3, 1, 4, 4, 2, 0], name_of)
    assert stems == ["zero", "two", "four", "one", "three"] and picks == [5, 4, 2, 1, 0]
    assert map_rows_in_csv_order([], ids, name_of) == ([], [])
    # an image the name table does not know is called by its id, as rows_from_scores calls it
    results = rows_from_scores([7], scores[:1], [1], [10, 50], {}, 2, "in")
    assert map_rows_in_csv_order(results, [7], {}) == (["7"], [0])


def _fake_rows(ids, trailing=(2, 5, 7)):
    i = torch.tensor(ids, dtype=torch.float32).reshape(-1, *([1] * len(trailing)))
    n = 1
    for d in trailing:
        n *= d
    return i * 1000.0 + torch.arange(n, dtype=torch.float32).reshape(1, *trailing)


def _worker(rank, world, port, n_images, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ddpm_ood_amd.data import partition
    from ddpm_ood_amd.trainer import gather_rows

    ids = partition(n_images, rank, world)
    calls = []
    for name in ("all_gather", "all_gather_into_tensor", "all_gather_object", "all_reduce", "broadcast", "gather"):
        orig = getattr(dist, name)
        setattr(dist, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    gids, rows, counts = gather_rows(torch.tensor(ids, dtype=torch.int32), _fake_rows(ids), -(-n_images // world))
    assert calls == ["all_gather_into_tensor"], calls  # ONE collective, the static-capacity scheme of gather_scores
    refused = False
    try:
        gather_rows(torch.tensor(ids, dtype=torch.int32), _fake_rows(ids), len(ids) - 1)
    except ValueError:
        refused = True
    q.put((rank, gids.tolist(), rows.numpy(), counts, refused or not ids))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n_images", [7, 1])
def test_gather_rows_two_ranks_rank_major_padding_dropped(n_images):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_images, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    order = [i for r in range(2) for i in range(r, n_images, 2)]  # unequal shards, rank-major
    for rank, ids, rows, counts, refused in got:
        assert ids == order and counts == [len(range(r, n_images, 2)) for r in range(2)]
        assert rows.shape == (n_images, 2, 5, 7) and rows.dtype.name == "float32"
        assert torch.equal(torch.from_numpy(rows), _fake_rows(order))  # every row with its id, no padding left
        assert refused  # a shard beyond the static capacity is refused (before the collective)


def test_gather_rows_without_a_group_is_the_identity():
    from ddpm_ood_amd.trainer import gather_rows

    ids, rows = torch.arange(3, dtype=torch.int32), _fake_rows([0, 1, 2])
    a, b, c = gather_rows(ids, rows)
    assert a is ids and b is rows and c == [3]
