"""CPU: the host-side half of ddpm_conv_k4s2_wgrad_f32 -- which shapes have the matrix-pipe tiling, what the scratch query answers,
and that bad arguments are refused before anything is launched (no compute calls without a GPU)."""

import pytest


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    if not _lib.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_tiling_rule_and_scratch_query(lib):
    split, scratch = lib.ddpm_conv_k4s2_wgrad_split, lib.ddpm_conv_k4s2_wgrad_scratch_floats
    for B, cin, cout, ext, dims in ((2, 128, 64, (8, 12, 16), 3), (2, 64, 128, (8, 12, 16), 3), (3, 64, 64, (1, 12, 20), 2),
                                    (1, 256, 256, (32, 32, 32), 3), (1, 128, 128, (8, 64, 64), 3)):
        s = split(B, cin, cout, *ext, dims)
        assert s >= 1, (cin, cout, ext)
        assert scratch(B, cin, cout, *ext, dims) >= s * 16 * cout * cin
    # no tiling: channel counts that are no multiple of 64, an odd or too wide W / 2
    assert split(2, 1, 8, 8, 12, 16, 3) == 0 and split(2, 8, 16, 1, 16, 12, 2) == 0 and split(1, 64, 96, 1, 8, 8, 2) == 0
    assert split(1, 64, 64, 1, 8, 6, 2) == 0 and split(1, 64, 64, 1, 8, 260, 2) == 0
    # the pixel stream is split once a slice has at least four pixel tiles: one image of 12 x 20 is not, some batch <= 64 is
    assert split(1, 64, 64, 1, 12, 20, 2) == 1
    assert any(split(B, 64, 64, 1, 12, 20, 2) > 1 for B in range(2, 65))
    # the 1-channel first layer of the README VQ-VAE takes the generic form, sliced over its 32^3 output positions
    assert scratch(1, 1, 256, 64, 64, 64, 3) >= 2 * 64 * 256
    # odd or missing extents, unknown dims: nothing to query
    for bad in ((1, 64, 64, 8, 7, 8, 3), (1, 64, 64, 3, 8, 8, 3), (1, 64, 64, 8, 8, 8, 4), (0, 64, 64, 8, 8, 8, 3)):
        assert split(*bad) == 0 and scratch(*bad) == 0


def test_bad_arguments_are_refused(lib):
    f = lib.ddpm_conv_k4s2_wgrad_f32
    assert f(None, None, None, 1, 64, 64, 8, 8, 8, 3, None, 0, 0, None) == -1
    assert b"null operand" in lib.ddpm_last_error()
    # non-null dummies with extents the argument check refuses (odd; unknown dims): nothing is planned or launched
    assert f(8, 8, 8, 1, 64, 64, 8, 7, 8, 3, None, 0, 0, None) == -1
    assert b"even" in lib.ddpm_last_error()
    assert f(8, 8, 8, 1, 64, 64, 8, 8, 8, 4, None, 0, 1, None) == -1
    assert b"dims 4" in lib.ddpm_last_error()
    assert lib.ddpm_relu_backward_f32(None, None, None, 4, None) == -1
