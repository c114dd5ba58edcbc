"""CPU: --simplex_noise on the host side -- the fixture recorded from the reference's simplex noise, the C-ABI entry point of the
kernel (exported, bound, argument checks), and the per-image seed derivation (tests/test_gpu_simplex.py runs the kernel)."""

from pathlib import Path

import numpy as np
import pytest
import torch

G = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    if not _lib.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_fixture_holds_the_recorded_cases():
    d = np.load(G / "simplex_noise.npz")
    n = len(d["slice_seed"])
    assert n == 5 * 7 + 2
    hw = {tuple(int(v) for v in r) for r in d["slice_hw"]}
    assert hw == {(32, 32), (28, 28), (64, 64), (8, 8), (16, 40)}
    assert set(int(t) for t in d["slice_t"]) >= {0, 1, 10, 499, 500, 970, 999}
    seeds = [int(s) for s in d["slice_seed"]]
    assert -10**10 in seeds and 10**10 - 1 in seeds and -(2**63) in seeds and 2**63 - 1 in seeds
    params = {tuple(float(v) for v in p) for p in d["slice_params"]}
    assert params == {(6.0, 0.8, 64.0), (2.0, 0.6, 16.0)}
    for k in range(n):
        s = d[f"slice_{k}"]
        assert s.dtype == np.float64 and s.shape == tuple(int(v) for v in d["slice_hw"][k])
        assert 0.05 < s.std() < 1.0  # not normalised (the reference does not rescale)
    for call, shape in (("call2d", (3, 3, 16, 16)), ("call3d", (2, 2, 4, 8, 8))):
        assert tuple(d[f"{call}_shape"]) == shape and d[f"{call}_noise"].shape == shape
        assert len(d[f"{call}_seeds"]) == shape[0] * shape[1] and len(d[f"{call}_t"]) == shape[0]
    # the reference's 3-D quirk: the (1, H, W) slice is broadcast along depth
    v = d["call3d_noise"]
    assert (v == v[:, :, :1]).all()


def test_kernel_entry_point_is_exported_bound_and_checks_its_arguments(lib):
    from ddpm_ood_amd import _lib

    assert "ddpm_simplex_noise_f32" in _lib.SIGNATURES
    fn = lib.ddpm_simplex_noise_f32
    assert fn.argtypes == _lib.SIGNATURES["ddpm_simplex_noise_f32"][1]
    assert lib.ddpm_abi_version() == 10 == _lib.ABI_VERSION  # an additive entry point: the ABI version stays
    assert fn(None, None, None, 1, 1, 1, 8, 8, 6, 0.8, 64.0, None) == -1
    assert b"NULL" in lib.ddpm_last_error()
    fake = 0x1000  # never dereferenced: the shape checks come first
    assert fn(fake, fake, fake, 1, 1, 1, 0, 8, 6, 0.8, 64.0, None) == -1
    assert b"shape" in lib.ddpm_last_error()
    assert fn(fake, fake, fake, 1, 1, 1, 8, 8, 0, 0.8, 64.0, None) == -1
    assert fn(fake, fake, fake, 1, 1, 1, 8, 8, 6, 0.8, 0.0, None) == -1
    assert b"octave" in lib.ddpm_last_error()


def test_simplex_seeds_are_a_pure_function_of_seed_index_t_and_channel():
    from ddpm_ood_amd.trainer import SIMPLEX_SEED_RANGE, simplex_seeds

    a = simplex_seeds(2, range(64), 500, 3)
    assert a.dtype == torch.int64 and a.shape == (64, 3)
    assert torch.equal(a, simplex_seeds(2, range(64), 500, 3))  # pure
    big = simplex_seeds(2, range(4096), 10, 4)
    assert int(big.min()) >= -SIMPLEX_SEED_RANGE and int(big.max()) < SIMPLEX_SEED_RANGE
    assert int(big.min()) < -SIMPLEX_SEED_RANGE // 2 and int(big.max()) > SIMPLEX_SEED_RANGE // 2  # spread over the range
    assert big.unique().numel() == big.numel()  # image index x channel: all distinct
    assert not torch.equal(a, simplex_seeds(2, range(64), 499, 3))  # t_start
    assert not torch.equal(a, simplex_seeds(3, range(64), 500, 3))  # seed
    assert (a[:, 0] != a[:, 1]).all() and (a[:, 1] != a[:, 2]).all()  # channel
    # a row's seeds depend on its image index, not on the batch it rides in
    assert torch.equal(simplex_seeds(2, [17, 3, 40], 500, 3), a[[17, 3, 40]])
    assert torch.equal(torch.cat([simplex_seeds(2, range(s, s + 16), 500, 3) for s in range(0, 64, 16)]), a)
    # negative and huge seeds (rank mixing: seed * 7919 + rank) are accepted
    assert simplex_seeds(-5, [0], 0, 1).shape == (1, 1) and simplex_seeds(2**70, [0], 2**40, 1).shape == (1, 1)


def test_simplex_flag_is_accepted_by_both_clis():
    import reconstruct
    import train_ddpm

    assert reconstruct.parse_args(["--simplex_noise", "1"]).simplex_noise == 1
    assert train_ddpm.parse_args(["--simplex_noise", "1"]).simplex_noise == 1
    assert reconstruct.parse_args([]).simplex_noise == 0 and train_ddpm.parse_args([]).simplex_noise == 0
