"""GPU: the family ddpm_conv_kernel_name reports is the kernel that runs.

One launch per row of the selection tables (csrc/conv_dispatch.hip), at the smallest descriptor of the host sweep
(tests/golden/conv_dispatch_parent.json) that selects the row, plus the smallest one whose family answers stats parts > 0 where
that is another descriptor.  The in-situ profiler has to show exactly one key, and it has to be one of the ProfScope names of
that family's launcher; a statistics slab is checked against float64 statistics of the produced tensor.
"""

import ctypes
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

# family -> prefixes of the ProfScope names of its launcher (copied from the .hip files); a key belongs to the family with the
# longest matching prefix ("conv3x3_wino44h_up" is wino44h's, not wino's)
PROF_KEYS = {
    "linear_skinny": ("linear_skinny",),
    "d3s": ("conv3x3_d3s",),
    "d3s2": ("conv3x3_d3s_stride2",),
    "d1s": ("conv1x1_d1s",),
    "wino44h": ("conv3x3_wino44h", "conv3d_wino44h"),
    "wino44": ("conv3x3_wino44", "conv3d_wino44"),
    "wino": ("conv3x3_wino", "conv3d_wino"),
    "s2h": ("conv3x3_s2h",),
    "conv1x1_dma": ("conv1x1_dma",),
    "mfma": ("conv3x3_mfma", "conv1x1_mfma", "conv3d_k3", "conv3d_k4s2", "conv3d_transpose_k4s2", "conv2d_k4s2",
             "conv2d_transpose_k4s2"),
    "direct": ("conv_direct", "conv3x3_small_cin", "conv3x3_small_cout"),
}


def _family_of(key):
    hits = [(len(p), fam) for fam, ps in PROF_KEYS.items() for p in ps if key.startswith(p)]
    return max(hits)[1] if hits else None


def _check_stats(y, st, parts):  # tolerances: tests/test_gpu_wino44h.py::_check_stats
    B, Cout = y.shape[:2]
    assert tuple(st.shape) == (B, Cout, parts, 2), st.shape
    yd = y.double().cpu().view(B, Cout, parts, -1)
    mean = yd.mean(-1)
    m2 = (yd - mean[..., None]).pow(2).sum(-1)
    st = st.cpu().double()
    sd = (m2 / yd.shape[-1]).sqrt()
    assert (st[..., 0] - mean).abs().max().item() <= 2e-6 * (1 + mean.abs().max().item() + sd.max().item())
    assert ((st[..., 1] - m2).abs() / (m2 + 1e-3 * m2.mean())).max().item() <= 2e-5


def _forms(ops, w, k, mode, names):
    """The packed forms `names` of weight w, as csrc/unet_engine.hip attaches them in this mode."""
    pack = {"wino": ops.pack_wino_weight, "wino44": ops.pack_wino44_weight, "folded": ops.fold_upsample_weight,
            "wino44h": ops.pack_conv1x1_h_weight if k == 1 else ops.pack_conv_s2h_weight if mode == ops.CONV_STRIDE2 else ops.pack_wino44h_weight,
            "d3h": ops.pack_conv_d1s_weight if k == 1 else ops.pack_conv_d3h_weight}
    out = {n: pack[n](w) for n in names}
    assert all(v is not None for v in out.values()), {n: v is not None for n, v in out.items()}
    return out


ALL3 = ("wino", "wino44", "wino44h", "d3h")
# (id, family, stats parts, B, C1, C2, Cout, H, ksize, mode, weight forms, extra): 2-D descriptors of the sweep
NORMAL, STRIDE2, UPSAMPLE2 = 0, 1, 2
CASES_2D = [
    ("linear_skinny", "linear_skinny", 0, 1, 64, 0, 64, 1, 1, NORMAL, (), {}),
    ("d3s", "d3s", 1, 1, 128, 0, 128, 8, 3, NORMAL, ALL3, {}),
    ("wino44h", "wino44h", 1, 128, 64, 0, 64, 16, 3, NORMAL, ("wino", "wino44", "wino44h"), {}),
    ("wino44", "wino44", 0, 256, 128, 0, 128, 8, 3, NORMAL, ALL3, {"split_f16": False}),
    ("wino", "wino", 0, 1, 64, 0, 64, 8, 3, NORMAL, ("wino", "wino44", "wino44h"), {}),
    ("wino_up", "wino", 2, 1, 128, 128, 128, 8, 3, UPSAMPLE2, ("folded", "wino", "wino44h", "d3h"), {}),
    ("d3s2", "d3s2", 1, 1, 128, 0, 128, 16, 3, STRIDE2, ("wino44h", "d3h"), {}),
    ("s2h", "s2h", 0, 1, 64, 0, 64, 8, 3, STRIDE2, ("wino44h",), {}),
    ("s2h_stats", "s2h", 1, 1, 64, 0, 64, 16, 3, STRIDE2, ("wino44h",), {}),
    ("d1s", "d1s", 0, 1, 128, 0, 128, 8, 1, NORMAL, ("wino44h", "d3h"), {}),
    ("conv1x1_dma", "conv1x1_dma", 0, 256, 128, 0, 128, 8, 1, NORMAL, (), {}),
    ("mfma", "mfma", 0, 1, 128, 0, 128, 1, 3, NORMAL, ALL3, {}),
    ("direct", "direct", 0, 1, 64, 0, 64, 1, 3, NORMAL, ("wino", "wino44", "wino44h"), {}),
    ("direct_conv_in", "direct", 1, 1, 1, 0, 128, 16, 3, NORMAL, (), {}),
]
# (id, family, B, C, D, H, op, weight forms): dims = 3
CASES_3D = [
    ("wino44h", "wino44h", 1, 256, 32, 32, "k3", ("wino", "wino44", "wino44h")),
    ("wino44", "wino44", 1, 256, 32, 32, "k3", ("wino", "wino44")),
    ("wino", "wino", 1, 128, 1, 8, "k3", ("wino",)),
    ("mfma", "mfma", 1, 128, 1, 8, "k3", ()),
    ("mfma_k4s2", "mfma", 1, 128, 8, 8, "k4s2", ()),
    ("mfma_transpose", "mfma", 1, 128, 1, 8, "transpose", ()),
]


@pytest.fixture
def launched():
    """Runs fn() with the profiler on; -> (result, family names ddpm_conv_kernel_name gave for the launched descriptors, report)."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    real = lib.ddpm_conv_f32

    def run(fn):
        names = []

        def spy(desc, stream):
            names.append(lib.ddpm_conv_kernel_name(desc).decode())
            return real(desc, stream)

        torch.cuda.synchronize()
        lib.ddpm_conv_f32 = spy
        lib.ddpm_prof_enable(1)
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            lib.ddpm_prof_enable(0)
            lib.ddpm_conv_f32 = real
        buf = ctypes.create_string_buffer(1 << 16)
        n = lib.ddpm_prof_report(buf, len(buf))
        return out, names, (json.loads(buf.value.decode()) if n > 0 else {})

    return run


def _assert_ran(names, report, family):
    assert names == [family], names
    assert len(report) == 1 and all(v["launches"] == 1 for v in report.values()), report
    key = next(iter(report))
    assert _family_of(key) == family, (key, family)


@pytest.mark.parametrize("case", CASES_2D, ids=[c[0] for c in CASES_2D])
def test_reported_family_runs_2d(device, launched, case):
    from ddpm_ood_amd import _lib, ops

    _, family, parts, B, C1, C2, Cout, H, k, mode, forms, extra = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C1, H, H, generator=g).to(device)
    x2 = torch.randn(B, C2, H, H, generator=g).to(device) if C2 else None
    w = (torch.randn(Cout, C1 + C2, k, k, generator=g) / (3 * (C1 + C2) ** 0.5)).to(device)
    bias = torch.randn(Cout, generator=g).to(device)
    if family == "linear_skinny":
        x, w = x[:, :, 0, 0].contiguous(), w[:, :, 0, 0].contiguous()
    kw = _forms(ops, w, k, mode, forms)
    prev = _lib.set_split_f16(extra.get("split_f16", True))
    try:
        (y, st), names, report = launched(lambda: ops.conv(x, w, bias, x2=x2, mode=mode, want_stats=True, **kw))
    finally:
        _lib.set_split_f16(prev)
    _assert_ran(names, report, family)
    assert (st is None) == (parts == 0)  # None: the parts == 0 answer
    if st is not None:
        _check_stats(y, st, parts)


@pytest.mark.parametrize("case", CASES_3D, ids=[c[0] for c in CASES_3D])
def test_reported_family_runs_3d(device, launched, case):
    from ddpm_ood_amd import ops

    _, family, B, Cc, D, H, op, forms = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cc, D, H, H, generator=g).to(device)
    k = 3 if op == "k3" else 4
    w = (torch.randn(Cc, Cc, k, k, k, generator=g) / (Cc * k ** 3) ** 0.5).to(device)
    pack = {"wino": ops.pack_wino3d_weight, "wino44": ops.pack_wino44_3d_weight, "wino44h": ops.pack_wino44h_3d_weight}
    kw = {n: pack[n](w) for n in forms}
    assert all(v is not None for v in kw.values())
    if op == "transpose":
        run = lambda: ops.conv_transpose(x, w)  # noqa: E731
    else:
        run = lambda: ops.conv3d(x, w, stride=1 if op == "k3" else 2, **kw)  # noqa: E731
    _, names, report = launched(run)
    _assert_ran(names, report, family)
