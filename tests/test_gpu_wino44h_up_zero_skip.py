"""-m gpu: the Upsample form of the split-f16 F(4x4, 3x3) kernel (conv_wino44r.hip, UP instantiations) after it stopped
computing the 11 transform positions that are exact zeros on a nearest-x2 image: 25 live positions on a
7 / 6 / 6 / 6 wave table, V from the four distinct source values per axis.

Reference: F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1) in float64 on the CPU, bar
max|err| < 2e-4 (1 + max|ref|) (the existing Upsample tests' bar, tests/test_gpu_wino44h.py).  Shapes: the smallest that reach
every branch -- two images per item (8^2 -> 16^2, ragged with B = 3) and one image per item in two parts (16^2 -> 32^2),
Cin 16 (one chunk pair) and 48 (three), Cout 64 and 128 (two cout tiles), one rectangular image (4 x 16 -> 8 x 32), and
eight images per item (4^2 -> 8^2, ragged with B = 9: the <8, 1> instantiation).  The fourth UP instantiation, <10, 0>, is
not reachable in 2-D: with Wo <= 32 a one-image item is 18 x 32, 34 x 16, 66 x 8 or 130 x 4 pixels, nine staging rounds each.
"""

import ctypes
import functools
import json
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [
    # B, Cin, Cout, low-res H, low-res W
    (3, 16, 64, 8, 8),      # two images per item, ragged last item, one chunk pair
    (3, 48, 128, 8, 8),     # ... three chunk pairs, two cout tiles
    (2, 16, 128, 16, 16),   # one image per item in two parts, one chunk pair, two cout tiles
    (2, 48, 64, 16, 16),    # ... three chunk pairs
    (2, 16, 64, 4, 16),     # rectangular: 4 x 16 -> 8 x 32
    (9, 16, 64, 4, 4),      # eight images per item, ragged last item
]


def _border_scaled(x):
    """Border rows and columns x 8: a wrong padding pixel (or a neighbour read in its place) shows."""
    x = x.clone()
    x[..., 0, :] *= 8
    x[..., -1, :] *= 8
    x[..., :, 0] *= 8
    x[..., :, -1] *= 8
    return x


def _reference(x, w, b):
    return F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)


@functools.lru_cache(maxsize=None)
def _operands(case):
    """Random operands of a case (CPU fp32) and the float64 reference, computed once and shared."""
    B, Cin, Cout, H, W = case
    g = torch.Generator().manual_seed(B * 1000 + Cin * 10 + Cout + H)
    x = _border_scaled(torch.randn(B, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g)
    return x, w, b, _reference(x, w, b)


def _up(device, x, w, b, **kw):
    from ddpm_ood_amd import ops

    d = lambda t: t.to(device)
    return ops.conv(d(x), d(w), d(b), mode=ops.CONV_UPSAMPLE2, wino44h=ops.pack_wino44h_weight(d(w)), **kw)


def _profiled(fn):
    """fn() under the in-situ profiler: (result, the profile keys of the kernels that ran)."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    torch.cuda.synchronize()
    lib.ddpm_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.ddpm_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.ddpm_prof_report(buf, len(buf))
    return out, (set(json.loads(buf.value.decode())) if n > 0 else set())


def _hold(y, ref):
    err = (y.cpu().double() - ref).abs().max().item()
    bar = 2e-4 * (1 + ref.abs().max().item())
    print(f"max|err| {err:.3e}  bar {bar:.3e}")
    assert math.isfinite(err) and err < bar, (err, bar)


@pytest.mark.parametrize("case", CASES)
def test_upsample_zero_skip_vs_float64_reference(device, case, monkeypatch):
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    from ddpm_ood_amd import ops

    x, w, b, ref = _operands(case)
    y, keys = _profiled(lambda: _up(device, x, w, b))
    print("profile keys:", sorted(keys))
    assert "conv3x3_wino44h_up" in keys, keys  # the split-f16 F(4x4) Upsample kernel ran: nothing fell back
    y_f22 = ops.conv(x.to(device), w.to(device), b.to(device), mode=ops.CONV_UPSAMPLE2, wino=ops.pack_wino_weight(w.to(device)))
    torch.cuda.synchronize()
    assert not torch.equal(y, y_f22)  # ... and it is not the F(2x2) Upsample kernel's result
    _hold(y, ref)


@pytest.mark.parametrize("tap", range(9))
def test_position_map_one_hot_taps(device, tap, monkeypatch):
    """A weight that lives in ONE of the nine taps: a live position dropped, or handed to the wrong wave / accumulator tile /
    exchange-slab entry, breaks at least one tap."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    B, Cin, Cout, H, W = CASES[0]
    g = torch.Generator().manual_seed(100 + tap)
    x = _border_scaled(torch.randn(B, Cin, H, W, generator=g))
    w = torch.zeros(Cout, Cin, 3, 3)
    w[:, :, tap // 3, tap % 3] = torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)
    b = torch.randn(Cout, generator=g)
    y = _up(device, x, w, b)
    torch.cuda.synchronize()
    _hold(y, _reference(x, w, b))


@pytest.mark.parametrize("case", CASES)
def test_equals_plain_kernel_on_materialised_image(device, case, monkeypatch):
    """The unchanged non-UP kernel on the materialised F.interpolate image (mode NORMAL, same packed weights, no prologue: both
    forms scale V by 2^0 and use the same item geometry) executes all 36 positions; the skipped products are U * 0 and the
    live V values come from the same expressions, so the outputs are equal bit for bit (they were on the parent commit too)."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    from ddpm_ood_amd import ops

    x, w, b, ref = _operands(case)
    d = lambda t: t.to(device)
    wh = ops.pack_wino44h_weight(d(w))
    y_up = ops.conv(d(x), d(w), d(b), mode=ops.CONV_UPSAMPLE2, wino44h=wh)
    x_mat = F.interpolate(d(x), scale_factor=2, mode="nearest").contiguous()
    y_mat = ops.conv(x_mat, d(w), d(b), mode=ops.CONV_NORMAL, wino44h=wh)
    torch.cuda.synchronize()
    _hold(y_mat, ref)
    _hold(y_up, ref)
    print("bits that differ:", (y_up != y_mat).sum().item())
    assert torch.equal(y_up, y_mat)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]])
def test_deterministic_and_statistics(device, case, monkeypatch):
    """Two runs are bit-equal, the output does not depend on want_stats, and the epilogue's {mean, M2} per (image, cout, slice
    of rows) match the reference's mean and variance at the tolerances of tests/test_gpu_wino44h.py::_check_stats."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    x, w, b, ref = _operands(case)
    y = _up(device, x, w, b)
    y2 = _up(device, x, w, b)
    ys, st = _up(device, x, w, b, want_stats=True)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    assert torch.equal(y, ys)
    B, Cout, Ho, Wo = ref.shape
    assert st is not None and st.shape[:2] == (B, Cout) and st.shape[3] == 2, None if st is None else st.shape
    parts = st.shape[2]
    rd = ref.view(B, Cout, parts, (Ho // parts) * Wo)
    mean = rd.mean(-1)
    m2 = (rd - mean[..., None]).pow(2).sum(-1)
    sd = (m2 / rd.shape[-1]).sqrt()
    st = st.cpu().double()
    e_mean = (st[..., 0] - mean).abs().max().item()
    e_m2 = ((st[..., 1] - m2).abs() / (m2 + 1e-3 * m2.mean())).max().item()
    print(f"mean err {e_mean:.3e}  M2 rel err {e_m2:.3e}")
    assert e_mean <= 2e-6 * (1 + mean.abs().max().item() + sd.max().item())
    assert e_m2 <= 2e-5
