"""-m gpu: NaN, inf and overflow stay loud and inside their own image.

Two claims of the numeric guard ("Numeric guard"; include/ddpm_ood_hip.h) are held here at the op level:

* "an overflow is never silent": a NaN or inf that a kernel is handed or produces reaches its output the way it reaches the
  output of the same op in torch -- through every ReLU (F.relu(nan) = nan, where fmaxf(nan, 0) = 0) and through the LPIPS
  max-pool (F.max_pool2d keeps a NaN of its window) -- so that it ends in the status word and in the score;
* "a per-image result does not depend on the batch it rides in": the kernels that put several images into one workgroup or tile
  (F(4x4): 2 / 8 / 16 images per item, F(2x2): 4 per workgroup, conv1x1_dma: 256 / HW per tile, the 7x7 MFMA tile, the
  small-launch kernels, the statistics epilogues, linear_skinny's 32-row tiles, attention at 8 and 64 tokens) are run on a batch
  whose MIDDLE image is poisoned: the other images must come out bit-identical to the clean run.

tests/nonfinite_util.py has the three assertions; shapes are rows of the case tables of tests/test_gpu_ops.py, the kernel that
takes each is asserted through ddpm_conv_kernel_name.  NaN and inf are ordinary float data here: every buffer keeps its size.

Caps on the non-finite outputs per output plane (one poisoned input pixel, no GroupNorm -- a GroupNorm spreads it over its
group and the convolution behind it over the image, in torch too):
  direct / MFMA / 1x1, stride 1    9: the reference's own footprint, the 3x3 window positions that hold the pixel
  the same with nearest-x2        16: the pixel becomes a 2x2 block, 3x3 windows holding any of it: 4x4 positions
  stride 2                         4: outputs o with 2o - 1 <= h <= 2o + 1: at most 2 per axis
  F(2x2)                          16: an input tile is 4x4 pixels at stride 2, a pixel lies in at most 2 per axis = 4 tiles of 2x2
                                      outputs; a NaN in a tile reaches all of its transform, so all 4 outputs of each
  F(4x4), upsample forms too      64: an input tile is 6x6 at stride 4 (in the upsampled image for the upsample forms): at most
                                      2 per axis = 4 tiles of 4x4 outputs
  one-shot small-launch kernels    the direct kernels' caps (they are direct convolutions over channel slices)
"""

import math

import pytest
import torch
import torch.nn.functional as F

from nonfinite_util import NAN, check_poisoned, conv_families, interior, poison

pytestmark = pytest.mark.gpu

NORMAL, STRIDE2, UPSAMPLE2 = 0, 1, 2
KINDS = ("nan_pixel", "nan_image", "inf_pixel")


@pytest.fixture(autouse=True)
def _status_word_is_left_clean(device):
    """Every test here reads and clears the device status word when it is done: a poisoned run must not leak into a later test."""
    from ddpm_ood_amd import _lib

    _lib.status_read(clear=True)
    yield
    torch.cuda.synchronize()
    _lib.status_read(clear=True)


# ---- UNet convolutions (ops.conv) ------------------------------------------------------------------------------------------

W44 = {"DDPM_CONV_WINO44": "2"}      # the F(4x4) kernels also for launches smaller than the chip
D3S = {"DDPM_CONV_D3S": "2"}         # the one-shot small-launch kernels for any launch size
DMA = {"DDPM_CONV1X1_DMA_MIN_WG": "1"}  # conv1x1_dma.hip below its launch-size floor

# id: (family, env, forms, B, C1, C2, Cout, H, ksize, mode, gn, act (SiLU), chan_add, residual, tol, rms, cap, overflow scale)
# gn = False rows are the ones the caps apply to; overflow: split-f16 forms that read a raw tensor (3e4 behind the 2^3 pre-scale
# of the Downsample kernel, 3e5 behind 2^0)
CONV_CASES = {
    # direct and MFMA kernels: 7x7 (two images per 98-pixel tile) and 8x8, virtual concat
    "direct_7": ("direct", {}, ("force_direct",), 5, 256, 256, 256, 7, 3, NORMAL, True, True, True, False, 2e-5, None, None, None),
    "direct_7_raw": ("direct", {}, ("force_direct",), 5, 256, 256, 256, 7, 3, NORMAL, False, False, True, True, 2e-5, None, 9, None),
    "direct_8": ("direct", {}, ("force_direct",), 5, 256, 256, 256, 8, 3, NORMAL, True, True, True, False, 2e-5, None, None, None),
    "mfma_7": ("mfma", {}, (), 5, 256, 256, 256, 7, 3, NORMAL, True, True, True, False, 2e-5, None, None, None),
    "mfma_7_raw": ("mfma", {}, (), 5, 256, 256, 256, 7, 3, NORMAL, False, False, True, True, 2e-5, None, 9, None),
    "mfma_8": ("mfma", {}, (), 5, 256, 256, 256, 8, 3, NORMAL, True, True, True, False, 2e-5, None, None, None),
    "mfma_8_raw": ("mfma", {}, (), 5, 256, 256, 256, 8, 3, NORMAL, False, False, False, True, 2e-5, None, 9, None),
    # F(2x2): four images per workgroup
    "wino_8": ("wino", {}, ("wino",), 5, 256, 256, 256, 8, 3, NORMAL, True, True, True, False, 4e-5, None, None, None),
    "wino_8_raw": ("wino", {}, ("wino",), 5, 8, 0, 64, 8, 3, NORMAL, False, False, False, True, 4e-5, None, 16, None),
    # F(4x4) fp32 and split-f16: two images per item at 16x16, eight at 8x8 (ragged last item)
    "wino44_16": ("wino44", W44, ("wino44",), 5, 256, 0, 256, 16, 3, NORMAL, True, True, False, True, 2e-4, 1e-5, None, None),
    "wino44_16_raw": ("wino44", W44, ("wino44",), 5, 256, 0, 256, 16, 3, NORMAL, False, False, False, True, 2e-4, 1e-5, 64, None),
    "wino44_8": ("wino44", W44, ("wino44",), 19, 128, 128, 64, 8, 3, NORMAL, True, True, True, True, 2e-4, 1e-5, None, None),
    "wino44_8_raw": ("wino44", W44, ("wino44",), 19, 128, 128, 64, 8, 3, NORMAL, False, False, True, True, 2e-4, 1e-5, 64, None),
    "wino44h_16": ("wino44h", W44, ("wino44h",), 5, 256, 0, 256, 16, 3, NORMAL, True, True, False, True, 2e-4, 1e-5, None, None),
    "wino44h_16_raw": ("wino44h", W44, ("wino44h",), 5, 256, 0, 256, 16, 3, NORMAL, False, False, False, True, 2e-4, 1e-5, 64, 3e5),
    "wino44h_8": ("wino44h", W44, ("wino44h",), 19, 128, 128, 64, 8, 3, NORMAL, True, True, True, True, 2e-4, 1e-5, None, None),
    "wino44h_8_raw": ("wino44h", W44, ("wino44h",), 19, 128, 128, 64, 8, 3, NORMAL, False, False, True, True, 2e-4, 1e-5, 64, 3e5),
    # upsample forms: four images per item at 4x4 low-res, one at 8x8
    "up_direct_4": ("direct", {}, ("force_direct",), 5, 64, 0, 128, 4, 3, UPSAMPLE2, False, False, False, True, 2e-5, None, 16, None),
    "up_mfma_8": ("mfma", {}, (), 3, 256, 0, 256, 8, 3, UPSAMPLE2, False, False, False, True, 2e-5, None, 16, None),
    "up_folded_4": ("mfma", {}, ("folded",), 5, 64, 0, 128, 4, 3, UPSAMPLE2, False, False, False, True, 2e-5, None, 16, None),
    "up_folded_8": ("mfma", {}, ("folded",), 3, 256, 0, 256, 8, 3, UPSAMPLE2, False, False, False, True, 2e-5, None, 16, None),
    "up_wino_4": ("wino", {}, ("wino",), 5, 64, 0, 128, 4, 3, UPSAMPLE2, False, False, False, True, 4e-5, None, 16, None),
    "up_wino_8": ("wino", {}, ("wino",), 3, 256, 0, 256, 8, 3, UPSAMPLE2, False, False, False, True, 4e-5, None, 16, None),
    "up_wino44h_4": ("wino44h", W44, ("wino44h",), 5, 64, 0, 128, 4, 3, UPSAMPLE2, False, False, False, False, 2e-4, 1e-5, 64, 3e5),
    "up_wino44h_8": ("wino44h", W44, ("wino44h",), 3, 256, 0, 256, 8, 3, UPSAMPLE2, False, False, False, False, 2e-4, 1e-5, 64, 3e5),
    # stride 2 on the split-f16 kernel, the 64 x 128 form (B = 4); the chip-filling form has its own test below
    "s2h_4": ("s2h", {}, ("wino44h",), 4, 128, 0, 128, 16, 3, STRIDE2, False, False, False, False, 2e-5, None, 4, 3e4),
    # conv1x1_dma: four images per 256-pixel tile at HW = 64, sixteen at HW = 16; the GroupNorm prologue needs HW % 64 == 0
    "dma_64": ("conv1x1_dma", DMA, (), 5, 256, 128, 128, 8, 1, NORMAL, False, False, False, True, 2e-5, None, 9, 3e5),
    "dma_16": ("conv1x1_dma", DMA, (), 19, 256, 0, 256, 4, 1, NORMAL, False, False, True, False, 2e-5, None, 9, 3e5),
    "dma_gn_64": ("conv1x1_dma", DMA, (), 5, 256, 0, 768, 8, 1, NORMAL, True, False, False, False, 2e-5, None, None, None),
    # the one-shot small-launch kernels at batch 3
    "d3s_16": ("d3s", D3S, ("d3h",), 3, 128, 0, 128, 16, 3, NORMAL, True, True, True, True, 2e-5, None, None, None),
    "d3s_8_raw": ("d3s", D3S, ("d3h",), 3, 64, 0, 128, 8, 3, NORMAL, False, False, False, True, 2e-5, None, 9, 3e5),
    "d3s_up_8": ("d3s", D3S, ("d3h",), 3, 128, 0, 256, 8, 3, UPSAMPLE2, False, False, False, False, 2e-5, None, 16, 3e5),
    "d3s2_32": ("d3s2", D3S, ("d3h",), 3, 64, 0, 128, 32, 3, STRIDE2, False, False, False, False, 2e-5, None, 4, 3e5),
    "d1s_16": ("d1s", D3S, ("d1s",), 3, 128, 0, 256, 16, 1, NORMAL, False, False, False, False, 2e-5, None, 9, 3e5),
    "d1s_gn_8": ("d1s", D3S, ("d1s",), 3, 256, 0, 768, 8, 1, NORMAL, True, False, False, False, 2e-5, None, None, None),
    # conv_in: the small-cin kernel with the statistics epilogue (DPP segment merges over 256-pixel slices)
    "conv_in_32": ("direct", {}, (), 5, 1, 0, 128, 32, 3, NORMAL, False, False, False, False, 2e-5, None, 9, None),
}


def _conv_params():
    out = []
    for cid, c in CONV_CASES.items():
        for kind in KINDS + (("overflow",) if c[-1] else ()):
            out.append(pytest.param(cid, kind, id=f"{cid}-{kind}"))
    return out


def _ref_conv64(t, w, b, gn, act, mode, chan_off, k):
    """tests/test_gpu_ops.py::_ref_conv in float64."""
    xin = t["x"].double() if t.get("x2") is None else torch.cat([t["x"], t["x2"]], 1).double()
    if gn is not None:
        gamma, beta, G = gn
        xin = F.group_norm(xin, G, gamma.double(), beta.double(), 1e-6)
    if act:
        xin = F.silu(xin)
    if mode == UPSAMPLE2:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xin, w.double(), b.double(), stride=2 if mode == STRIDE2 else 1, padding=1 if k == 3 else 0)
    if t.get("chan_add") is not None:
        y = y + t["chan_add"].double()[:, chan_off:chan_off + w.shape[0], None, None]
    if t.get("residual") is not None:
        y = y + t["residual"].double()
    return y


def _pack_forms(ops, w, forms, k, mode):
    pack = {"wino": ops.pack_wino_weight, "wino44": ops.pack_wino44_weight, "folded": ops.fold_upsample_weight,
            "wino44h": ops.pack_conv_s2h_weight if mode == STRIDE2 else ops.pack_wino44h_weight, "d3h": ops.pack_conv_d3h_weight,
            "d1s": ops.pack_conv_d1s_weight}
    kw = {}
    for f in forms:
        if f == "force_direct":
            kw["force_direct"] = True
        else:
            kw["d3h" if f == "d1s" else f] = pack[f](w)
            assert kw["d3h" if f == "d1s" else f] is not None, f
    return kw


def _conv_setup(device, cid):
    """-> (run, ref, inputs, case) of a row of CONV_CASES; run asserts the family that takes the launch."""
    from ddpm_ood_amd import ops

    case = CONV_CASES[cid]
    family, _, forms, B, C1, C2, Cout, H, k, mode, gn, act, chan, res = case[:14]
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    Cin = C1 + C2
    Ho = H // 2 if mode == STRIDE2 else 2 * H if mode == UPSAMPLE2 else H
    inputs = {"x": torch.randn(B, C1, H, H, generator=g)}
    if C2:
        inputs["x2"] = torch.randn(B, C2, H, H, generator=g) * 1.5 + 0.3
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    gamma, beta = torch.randn(Cin, generator=g) * 0.2 + 1, torch.randn(Cin, generator=g) * 0.2
    if chan:
        inputs["chan_add"] = torch.randn(B, Cout + 64, generator=g)
    if res:
        inputs["residual"] = torch.randn(B, Cout, Ho, Ho, generator=g)
    wd, bd, gd, bed = (t.to(device) for t in (w, b, gamma, beta))
    kw = _pack_forms(ops, wd, forms, k, mode)

    def run(t):
        d = {n: v.to(device) for n, v in t.items()}
        gs = gh = None
        if gn:
            gs, gh = ops.gn_scale_shift(d["x"], gd, bed, 32, 1e-6, x2=d.get("x2"))
        with conv_families() as names:
            out = ops.conv(d["x"], wd, bd, x2=d.get("x2"), gscale=gs, gshift=gh, act=ops.ACT_SILU if act else ops.ACT_NONE, mode=mode,
                           chan_add=d.get("chan_add"), chan_add_offset=32 if chan else 0, residual=d.get("residual"),
                           want_stats=True, **kw)
        assert names == [family], (names, family)
        return out

    def ref(t):
        return _ref_conv64(t, w, b, (gamma, beta, 32) if gn else None, act, mode, 32, k)

    return run, ref, inputs, case


@pytest.mark.parametrize("cid,kind", _conv_params())
def test_conv_poisoned_image(device, cid, kind, monkeypatch):
    for name, value in CONV_CASES[cid][1].items():
        monkeypatch.setenv(name, value)
    run, ref, inputs, case = _conv_setup(device, cid)
    B, tol, rms, cap, scale = case[3], case[14], case[15], case[16], case[17]
    check_poisoned(run, ref, inputs, "x", kind, img=B // 2, tol=tol, rms=rms, cap=cap, scale=scale)


@pytest.mark.parametrize("kind", KINDS + ("overflow",))
def test_conv_stride2_chip_filling_form_poisoned_image(device, kind):
    """conv_s2h.hip's four-tile form (260 images of 16x16 -> 8x8: two images per tile, four tiles per workgroup): one image
    poisoned, its eight neighbours -- the other images of its workgroup among them -- bit-identical."""
    from ddpm_ood_amd import ops

    B, Cc, H, img = 260, 128, 16, 130
    near = [i for i in range(img - 4, img + 5) if i != img]
    g = torch.Generator().manual_seed(5)
    inputs = {"x": torch.randn(B, Cc, H, H, generator=g)}
    w = torch.randn(Cc, Cc, 3, 3, generator=g) / math.sqrt(Cc * 9)
    wd = w.to(device)
    ws = ops.pack_conv_s2h_weight(wd)

    def run(t):
        with conv_families() as names:
            out = ops.conv(t["x"].to(device), wd, None, mode=ops.CONV_STRIDE2, wino44h=ws, want_stats=True)
        assert names == ["s2h"], names
        return out

    def ref(t):
        return F.conv2d(t["x"][near + [img]].double(), w.double(), None, stride=2, padding=1)

    check_poisoned(run, ref, inputs, "x", kind, img=img, tol=2e-5, cap=4, scale=3e4, neighbours=near)


# ---- GroupNorm, linear --------------------------------------------------------------------------------------------------------

def _gn_check(x, x2, gamma, beta, sc0, sh0, sc1, sh1, img, bad_x):
    """scale / shift [B, C] of the clean and of the poisoned run against F.group_norm in float64 (tolerance 5e-6 of
    tests/test_gpu_ops.py::test_gn_scale_shift): the other images' rows bit-identical, the poisoned image's NaN in exactly the
    group of the NaN, right everywhere else."""
    for i in range(x.shape[0]):
        if i != img:
            assert torch.equal(sc0[i], sc1[i]) and torch.equal(sh0[i], sh1[i]), i
    xin = (bad_x if x2 is None else torch.cat([bad_x, x2], 1)).double()[img:img + 1]
    ref = F.group_norm(xin, 32, gamma.double(), beta.double(), 1e-6)
    got = xin * sc1[img].cpu().double()[None, :, None] + sh1[img].cpu().double()[None, :, None]
    rn, gn = ~torch.isfinite(ref), ~torch.isfinite(got)
    assert rn.any() and not rn.all()
    assert torch.equal(rn, gn)
    err = (got - ref)[~rn].abs().max().item()
    assert err <= 5e-6 * (1 + ref[~rn].abs().max().item()), err


@pytest.mark.parametrize("B,C1,C2,HW", [(3, 256, 128, 256), (3, 256, 256, 64), (3, 64, 0, 4096), (3, 96, 0, 1026)])
def test_gn_scale_shift_poisoned_image(device, B, C1, C2, HW):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C1, HW, generator=g) * 2 + 0.7
    x2 = torch.randn(B, C2, HW, generator=g) - 1 if C2 else None
    gamma, beta = torch.randn(C1 + C2, generator=g), torch.randn(C1 + C2, generator=g)
    d = lambda t: None if t is None else t.to(device)  # noqa: E731
    bad = poison(x, "nan_pixel", 1)
    sc0, sh0 = ops.gn_scale_shift(d(x), d(gamma), d(beta), 32, 1e-6, x2=d(x2))
    sc1, sh1 = ops.gn_scale_shift(d(bad), d(gamma), d(beta), 32, 1e-6, x2=d(x2))
    _gn_check(x, x2, gamma, beta, sc0, sh0, sc1, sh1, 1, bad)


@pytest.mark.parametrize("B,C1,C2,HW", [(5, 256, 128, 256), (3, 256, 256, 64), (3, 32, 0, 100)])
def test_channel_stats_and_gn_finalize_poisoned_image(device, B, C1, C2, HW):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(B * 1000 + C1 + HW)
    x = torch.randn(B, C1, HW, generator=g) * 1.7 + 0.6
    x2 = torch.randn(B, C2, HW, generator=g) * 0.4 - 2.0 if C2 else None
    gamma, beta = torch.randn(C1 + C2, generator=g) * 0.3 + 1, torch.randn(C1 + C2, generator=g) * 0.3
    d = lambda t: None if t is None else t.to(device)  # noqa: E731
    img = B // 2
    bad = poison(x, "nan_pixel", img)
    st2 = ops.channel_stats(d(x2)) if C2 else None
    st0, st1 = ops.channel_stats(d(x)), ops.channel_stats(d(bad))
    for i in range(B):
        if i != img:
            assert torch.equal(st0[i], st1[i]), i
    nan_rows = ~torch.isfinite(st1[img, :, 0, 0]).cpu()
    want = torch.zeros(C1, dtype=torch.bool)
    want[interior(x, img)[1]] = True
    assert torch.equal(nan_rows, want)  # the mean of the NaN's channel, and of no other
    sc0, sh0 = ops.gn_finalize(st0, d(gamma), d(beta), 32, 1e-6, HW, stats2=st2)
    sc1, sh1 = ops.gn_finalize(st1, d(gamma), d(beta), 32, 1e-6, HW, stats2=st2)
    _gn_check(x, x2, gamma, beta, sc0, sh0, sc1, sh1, img, bad)


@pytest.mark.parametrize("kind", ["nan_pixel", "nan_image", "inf_pixel"])
def test_linear_poisoned_row(device, kind):
    """linear_skinny_kernel's 32-row tiles at 33 rows: a poisoned row leaves the other 32 bit-identical."""
    from ddpm_ood_amd import ops

    B, Cin, Cout = 33, 160, 64
    g = torch.Generator().manual_seed(3)
    inputs = {"x": torch.randn(B, Cin, generator=g)}
    w = torch.randn(Cout, Cin, generator=g) / math.sqrt(Cin)
    b = torch.randn(Cout, generator=g)
    wd, bd = w.to(device), b.to(device)

    def run(t):
        with conv_families() as names:
            out = ops.conv(t["x"].to(device), wd, bd, act=1)
        assert names == ["linear_skinny"], names
        return out

    check_poisoned(run, lambda t: F.linear(F.silu(t["x"].double()), w.double(), b.double()), inputs, "x", kind, img=16, tol=2e-5)


# ---- attention ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part,kind", [("q", "nan_pixel"), ("k", "nan_pixel"), ("v", "nan_pixel"), ("qkv", "overflow")])
@pytest.mark.parametrize("B,heads,N", [(3, 1, 64), (3, 2, 100), (5, 1, 8)])
@pytest.mark.parametrize("use_scratch", [True, False])
def test_attention_poisoned_image(device, B, heads, N, part, kind, use_scratch, monkeypatch):
    """Both attention kernels (use_scratch with DDPM_ATTN_FA=2: the register-resident one for multiples of 64 tokens; the
    LDS-exchange kernels otherwise) with one q / k / v element of the middle image NaN: in torch a NaN of q reaches the outputs
    of its query, a NaN of k every output of the image, a NaN of v its channel.  overflow: the image's q, k and v times 1e4
    (beyond the range of the hi halves' products): each output is non-finite or right."""
    monkeypatch.setenv("DDPM_ATTN_FA", "2")
    from ddpm_ood_amd import ops

    C = 256 * heads
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, 3 * C, N, generator=g)
    qkv[:, :C] *= 1.5
    inputs = {"qkv": qkv, "res": torch.randn(B, C, N, generator=g)}
    scale = 1 / math.sqrt(C / heads)

    def run(t):
        return ops.attention(t["qkv"].to(device), t["res"].to(device), heads, scale, use_scratch=use_scratch)

    def ref(t):
        q, k, v = (x.reshape(B, heads, 256, N) for x in t["qkv"].double().split(C, dim=1))
        s = torch.einsum("bhdi,bhdj->bhij", q, k) * scale
        return torch.einsum("bhij,bhdj->bhdi", s.softmax(-1), v).reshape(B, C, N) + t["res"].double()

    channel = {"q": 0, "k": C, "v": 2 * C, "qkv": 0}[part] + 1
    check_poisoned(run, ref, inputs, "qkv", kind, img=B // 2, tol=1e-5, scale=1e4, channel=channel)


# ---- ReLU and max-pool semantics against torch -------------------------------------------------------------------------------

def _conv3d_setup(device, form, B, Cin, Cout, D, H):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(17 + H)
    inputs = {"x": torch.randn(B, Cin, D, H, H, generator=g), "residual": torch.randn(B, Cout, D, H, H, generator=g)}
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    b = torch.randn(Cout, generator=g)
    wd, bd = w.to(device), b.to(device)
    in_relu = form == "mfma"  # (the Winograd forms take no input ReLU)
    kw = {"mfma": {}, "wino": {"wino": ops.pack_wino3d_weight(wd)},
          "wino44": {"wino": ops.pack_wino3d_weight(wd), "wino44": ops.pack_wino44_3d_weight(wd)},
          "wino44h": {"wino44h": ops.pack_wino44h_3d_weight(wd)}}[form]
    assert all(v is not None for v in kw.values())

    def run(t):
        with conv_families() as names:
            out = ops.conv3d(t["x"].to(device), wd, bd, act=ops.ACT_RELU if in_relu else ops.ACT_NONE, out_act=ops.ACT_RELU,
                             residual=t["residual"].to(device), **kw)
        assert names == [form], (names, form)
        return out

    def ref(t):
        x = t["x"].double()
        return F.relu(F.conv3d(F.relu(x) if in_relu else x, w.double(), b.double(), padding=1) + t["residual"].double())

    return run, ref, inputs


CONV3D_CASES = {
    # form: (env, B, Cin, Cout, D, H, tol, rms, cap per (channel, depth slice), overflow scale)
    "mfma": ({}, 3, 128, 128, 2, 8, 2e-5, None, 9, None),        # the depth-tap MFMA kernel, ReLU on the input as well
    "wino": ({}, 3, 8, 128, 5, 16, 4e-5, None, 16, None),        # F(2x2) per depth tap
    "wino44": (W44, 3, 8, 128, 5, 32, 2e-4, 1e-5, 64, None),     # F(4x4) per depth tap
    "wino44h": (W44, 3, 16, 128, 5, 32, 2e-4, 1e-5, 64, 3e5),    # split-f16 F(4x4): the residual unit whose overflow was silent
}


@pytest.mark.parametrize("form,key,kind", [(f, k, v) for f, c in CONV3D_CASES.items() for k, v in
                                           (("x", "nan_pixel"), ("x", "nan_image"), ("x", "inf_pixel"), ("residual", "nan_pixel"),
                                            ("x", "overflow")) if v != "overflow" or c[-1]])
def test_conv3d_relu_epilogue_keeps_nan(device, form, key, kind, monkeypatch):
    """The VQ-VAE residual-unit convolution relu(conv3d(x) + residual) on every kernel that has the ReLU epilogue: a NaN of the
    input or of the residual is a NaN of the output (F.relu keeps it); for the residual the mask is the reference's exactly."""
    env, B, Cin, Cout, D, H, tol, rms, cap, scale = CONV3D_CASES[form]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    run, ref, inputs = _conv3d_setup(device, form, B, Cin, Cout, D, H)
    check_poisoned(run, ref, inputs, key, kind, img=1, tol=tol, rms=rms, cap=cap if key == "x" else None, scale=scale,
                   exact_mask=key == "residual")


@pytest.mark.parametrize("kind", ["nan_pixel", "nan_image", "inf_pixel", "overflow"])
def test_conv_transpose_parity_relu_keeps_nan(device, kind, monkeypatch):
    """The VQ-VAE's largest up-convolution as eight parity convolutions on the split-f16 F(4x4) kernel (2^0 pre-scale) with the
    ReLU epilogue, at the forced shape of test_conv_transpose3d_as_eight_parity_convolutions (sub-batches of two: images 0 and 1
    share a launch).  overflow: inf - inf = NaN in the input transform must come out as NaN, not as relu's 0."""
    monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    from ddpm_ood_amd import ops

    B, Cin, Cout, D, H, W = 3, 32, 128, 2, 32, 64
    g = torch.Generator().manual_seed(31)
    inputs = {"x": torch.randn(B, Cin, D, H, W, generator=g)}
    w = torch.randn(Cin, Cout, 4, 4, 4, generator=g) / math.sqrt(Cin * 8)
    b = torch.randn(Cout, generator=g)
    wd, bd = w.to(device), b.to(device)
    assert ops.conv_transpose_parity_supported(inputs["x"].to(device), wd)
    pw = ops.pack_convT_parity_weights(wd)

    def run(t):
        with conv_families() as names:
            out = ops.conv_transpose_parity(t["x"].to(device), pw, bd, out_act=ops.ACT_RELU, sub_batch=2)
        assert names == ["wino44h"] * 16, names
        return out

    def ref(t):
        return F.relu(F.conv_transpose3d(t["x"].double(), w.double(), b.double(), stride=2, padding=1))

    # cap: per parity at most 4 tiles of 4x4 outputs = 64 positions of the input grid in a slice, interleaved from the 4
    # in-plane parities of that output slice: 256
    check_poisoned(run, ref, inputs, "x", kind, img=1, tol=2e-4, rms=1e-5, cap=256, scale=3e5)


@pytest.mark.parametrize("op,kind", [(o, k) for o in ("transpose", "k4s2", "cin1", "generic", "generic_residual", "generic_transposed")
                                     for k in ("nan_pixel", "nan_image", "inf_pixel") if o != "generic_residual" or k == "nan_pixel"])
def test_vqvae_edge_and_generic_relu_keeps_nan(device, op, kind):
    """ops.conv_transpose and ops.conv3d(stride=2) with out_act = ReLU (conv_mfma.hip), ops.conv3d_k4s2_cin1(relu=True) and the
    generic convnd kernel with relu (conv3d_edge.hip), NaN in the input; generic_residual: NaN in the residual that feeds the
    output ReLU (mask equal to the reference's)."""
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(29)
    key, exact, tol = "x", False, 2e-5
    if op == "transpose":
        Cin, Cout, sp = 8, 128, (2, 2, 2)
        w = torch.randn(Cin, Cout, 4, 4, 4, generator=g) / math.sqrt(Cin * 8)
        b = torch.randn(Cout, generator=g)
        wd, bd = w.to(device), b.to(device)
        run = lambda t: ops.conv_transpose(t["x"].to(device), wd, bd, out_act=ops.ACT_RELU)  # noqa: E731
        ref = lambda t: F.relu(F.conv_transpose3d(t["x"].double(), w.double(), b.double(), stride=2, padding=1))  # noqa: E731
    elif op == "k4s2":
        Cin, Cout, sp = 8, 128, (4, 4, 4)
        w = torch.randn(Cout, Cin, 4, 4, 4, generator=g) / math.sqrt(Cin * 64)
        b = torch.randn(Cout, generator=g)
        wd, bd = w.to(device), b.to(device)
        run = lambda t: ops.conv3d(t["x"].to(device), wd, bd, stride=2, out_act=ops.ACT_RELU)  # noqa: E731
        ref = lambda t: F.relu(F.conv3d(t["x"].double(), w.double(), b.double(), stride=2, padding=1))  # noqa: E731
    elif op == "cin1":
        Cin, Cout, sp = 1, 16, (8, 12, 20)
        w = torch.randn(Cout, 1, 4, 4, 4, generator=g) / 8
        b = torch.randn(Cout, generator=g)
        wd, bd = w.to(device), b.to(device)
        run = lambda t: ops.conv3d_k4s2_cin1(t["x"].to(device), wd, bd, relu=True)  # noqa: E731
        ref = lambda t: F.relu(F.conv3d(t["x"].double(), w.double(), b.double(), stride=2, padding=1))  # noqa: E731
    else:
        transposed = op == "generic_transposed"
        Cin, Cout, sp, tol = (6, 3, (6, 8, 10), 2e-6) if transposed else (5, 7, (6, 8, 10), 2e-6)
        k, stride = (4, 2) if transposed else (3, 1)
        w = torch.randn(*((Cin, Cout) if transposed else (Cout, Cin)), k, k, k, generator=g) / math.sqrt(Cin * k ** 3)
        b = torch.randn(Cout, generator=g)
        wd, bd = w.to(device), b.to(device)
        f = F.conv_transpose3d if transposed else F.conv3d
        run = lambda t: ops.convnd_generic(t["x"].to(device), wd, bd, stride=stride, padding=1, transposed=transposed,  # noqa: E731
                                           residual=t["residual"].to(device), relu=True)
        ref = lambda t: F.relu(f(t["x"].double(), w.double(), b.double(), stride=stride, padding=1) + t["residual"].double())  # noqa: E731
        if op == "generic_residual":
            key, exact = "residual", True
    inputs = {"x": torch.randn(3, Cin, *sp, generator=g)}
    if op.startswith("generic"):
        out_sp = tuple(2 * e for e in sp) if op == "generic_transposed" else sp
        inputs["residual"] = torch.randn(3, Cout, *out_sp, generator=g)
    check_poisoned(run, ref, inputs, key, kind, img=1, tol=tol, exact_mask=exact)


@pytest.mark.parametrize("kind", ["nan_pixel", "nan_image", "inf_pixel"])
@pytest.mark.parametrize("layer", ["conv1_grey", "conv2_scalar", "conv2_mfma", "conv3_mfma"])
def test_lpips_conv_relu_keeps_nan(device, layer, kind):
    """The LPIPS-AlexNet convolutions with their ReLU, both kernels (one thread per output; fp32 MFMA for the same-padded stride-1
    layers): a NaN pixel of the reconstruction stays a NaN of the features, as in the reference's network."""
    from ddpm_ood_amd import ops

    N, Cx, Cin, H, W, Cout, k, stride, pad, mfma = {"conv1_grey": (5, 1, 3, 32, 32, 64, 11, 4, 2, False),
                                                    "conv2_scalar": (4, 64, 64, 7, 7, 192, 5, 1, 2, False),
                                                    "conv2_mfma": (3, 64, 64, 15, 11, 192, 5, 1, 2, True),
                                                    "conv3_mfma": (3, 8, 8, 9, 9, 32, 3, 1, 1, True)}[layer]
    g = torch.Generator().manual_seed(N + Cin + H + k)
    inputs = {"x": torch.rand(N, Cx, H, W, generator=g)}
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    wd, bd = w.to(device), b.to(device)
    if mfma:
        assert ops.lpips_conv_mfma_supported(Cin, H, W, Cout, k)
        packed = ops.lpips_pack_conv_weight(wd)
        run = lambda t: ops.lpips_conv_mfma(t["x"].to(device), packed, bd, Cout, k, relu=True)  # noqa: E731
    else:
        run = lambda t: ops.lpips_conv(t["x"].to(device), wd, bd, stride, pad, True)  # noqa: E731

    def ref(t):
        x = t["x"].double()
        return F.relu(F.conv2d(x.expand(N, Cin, H, W) if Cx == 1 else x, w.double(), b.double(), stride=stride, padding=pad))

    check_poisoned(run, ref, inputs, "x", kind, img=N // 2, tol=2e-5)


@pytest.mark.parametrize("shape", [(3, 64, 7, 7), (3, 5, 15, 12), (3, 2, 3, 3)])
def test_maxpool3s2_keeps_nan(device, shape):
    """F.max_pool2d(x, 3, 2) returns NaN for a window that holds one, whatever its position in the window (first, middle, last)."""
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g)
    want_clean = F.max_pool2d(x, 3, 2)
    for pos in ((0, 0), (shape[2] // 2, shape[3] // 2), (shape[2] - 1, shape[3] - 1), (1, 2)):
        bad = x.clone()
        bad[1, 1, pos[0], pos[1]] = NAN
        bad[1, 0, pos[0], pos[1]] = float("-inf")
        y = ops.maxpool3s2(bad.to(device)).cpu()
        want = F.max_pool2d(bad, 3, 2)
        assert torch.isnan(want[1, 1]).any() or pos == (shape[2] - 1, shape[3] - 1)  # (a last column no window reaches)
        assert torch.equal(torch.isnan(y), torch.isnan(want)), pos
        assert torch.equal(y[~torch.isnan(want)], want[~torch.isnan(want)])
        assert torch.equal(y[0], want_clean[0]) and torch.equal(y[2], want_clean[2])


def test_lpips_score_of_a_nan_reconstruction_is_nan(device):
    """Whole LPIPS(normalize=True): image 1 of the second argument holds one NaN pixel -> its value is NaN like the oracle's, the
    other images' values are bit-identical to the clean run's."""
    import oracle
    from ddpm_ood_amd.perceptual import LPIPS

    g = torch.Generator().manual_seed(32)
    x, y = torch.rand(3, 1, 32, 32, generator=g), torch.rand(3, 1, 32, 32, generator=g)
    bad = poison(y, "nan_pixel", 1)
    hip = LPIPS(seed=3)
    ref = oracle.LPIPSAlex()
    ref.load_state_dict(hip.state_dict())
    want = ref(x, bad, normalize=True).flatten()
    hip = hip.to(device)
    clean = hip(x.to(device), y.to(device), normalize=True).flatten().cpu()
    got = hip(x.to(device), bad.to(device), normalize=True).flatten().cpu()
    assert math.isnan(want[1].item()) and torch.isfinite(want[[0, 2]]).all()
    assert math.isnan(got[1].item())
    assert torch.equal(got[[0, 2]], clean[[0, 2]])


# ---- VQ-VAE encoder, whole engine -----------------------------------------------------------------------------------------------

def test_vqvae_encoder_carries_a_nan_pixel_to_the_quantiser(device):
    """The 2-D 128-channel VQ-VAE of test_vqvae_2d_mfma_friendly_layers_match_oracle: every encoder layer ends in a ReLU, so a NaN
    pixel reaches the quantiser -- and status bit 4 -- only if the ReLUs keep it.  The oracle's latent of that image holds NaN;
    the latents of its neighbours are bit-identical to the clean run's."""
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd.vqvae import VQVAE as PV
    from oracle.vqvae import VQVAE as OV

    cfg = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(128, 128), num_res_layers=2,
               num_res_channels=(128, 128), downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1)),
               upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0)), num_embeddings=32, embedding_dim=128)
    torch.manual_seed(1)
    o = OV(**cfg).eval()
    with torch.no_grad():
        o.quantizer.quantizer.embedding.weight.mul_(3.0)
    p = PV(**cfg)
    p.load_state_dict(o.state_dict())
    p = p.to(device).eval()
    x = torch.rand(3, 1, 32, 32, generator=torch.Generator().manual_seed(2))
    bad = poison(x, "nan_pixel", 1)
    with torch.no_grad():
        zo = o.encode_stage_2_inputs(bad)
        assert torch.isnan(zo[1]).any() and torch.isfinite(zo[[0, 2]]).all()
        _lib.status_read(clear=True)
        z0 = p.encode_stage_2_inputs(x.to(device))
        torch.cuda.synchronize()
        assert _lib.status_read(clear=True) == 0
        z1 = p.encode_stage_2_inputs(bad.to(device))
        torch.cuda.synchronize()
        word = _lib.status_read(clear=True)
    assert word & 4, f"status word {word}: the quantiser saw no non-finite latent"
    assert torch.equal(z0[0], z1[0]) and torch.equal(z0[2], z1[2])
    assert (~torch.isfinite(z1[1])).any()


@pytest.mark.parametrize("B,graph,fused", [(5, "0", "1"), (5, "1", "1"), (5, "0", "0"), (5, "1", "0"), (70, "0", "1"), (70, "0", "0")])
def test_unet_forward_with_one_nan_image(device, B, graph, fused, monkeypatch):
    """The small UNet forward with image 2 all-NaN, eager and replayed from a captured graph, GroupNorm statistics from the
    producers' epilogues (they take over at 70 images of 32x32) and from the reading kernel: the other images are bit-identical
    to the run with a clean image 2, image 2 is NaN everywhere."""
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    monkeypatch.setenv("DDPM_UNET_GRAPH", graph)
    monkeypatch.setenv("DDPM_GN_FUSED", fused)
    m = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    m.load_state_dict(random_state_dict("small", 1, seed=1))
    m = m.to(device).eval()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 1, 32, 32, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g).to(device)
    bad = poison(x, "nan_image", 2)
    others = [i for i in range(B) if i != 2]
    with torch.no_grad():
        clean = [m(x.to(device), timesteps=t).clone() for _ in range(3 if graph == "1" else 1)]  # eager, capture, replay
        outs = [m(bad.to(device), timesteps=t).clone() for _ in range(3 if graph == "1" else 1)]
    torch.cuda.synchronize()
    assert torch.isfinite(clean[0]).all() and all(torch.equal(c, clean[0]) for c in clean)
    for y in outs:
        assert torch.equal(y[others], clean[0][others])
        assert torch.isnan(y[2]).all()
