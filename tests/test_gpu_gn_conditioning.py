"""-m gpu: the conditioning of the GroupNorm statistics -- large DC offsets, first-order between-slice / between-channel terms,
variances near eps, constant and dead planes -- through every kernel that produces, merges or reads {mean, M2} pairs.

The rest of the suite feeds these kernels randn * s + m with |m| <= 2 and s >= 0.4: a kernel that formed M2 from a sum and a sum
of squares, or merged slices with a wrong count, would pass it (the cancellation is 1e-7 there, a wrong merge term 1e-3).  Here
the same kernels see (seeded CPU generator, all of them):

    dc(k)      N(0, 1) + k, k = 10, 100, 1000             chan_dc    channel 0 of every group at mean 1000, the others at 0
    slice_dc   +50 / -50 halves (a ramp of `parts` levels) + N(0, 1)      tiny       1e-3 N(0, 1): the variance is about eps
    const(c)   whole groups equal to c = 0, 0.5, -3, 1024 (power-of-two counts: every partial sum is exact)
    one_live   one channel of every group N(0, 1), the others exactly 0

References are float64 on the CPU; for emitted statistics, the float64 statistics of the tensor the kernel itself wrote.  With
u = 2^-24, L the largest |value| of a slice / group, sigma its float64 standard deviation and kappa = L / sigma:

    emitted {mean, M2}      |d mean| <= 8 u L, |d M2| / M2 <= 2e-5 + 1e-7 kappa; const(c): mean == c, M2 == 0 bit for bit; dead
                            channels report {0, 0}; output bit-identical with / without statistics; statistics bit-reproducible
    sc, sh (finalize, reading)   |d sc| <= (1e-5 + 1e-7 kappa) |sc64|,
                            |d sh| <= (1e-5 + 1e-7 kappa) |sc64 mu| + 8 u |sc64| L + 2 u |beta|; const(c): sc within 2 ulp of
                            fp32(gamma / sqrt(eps)), |c sc + sh - beta| <= 4 u |sc c| + 2 u |beta|
    GroupNorm + SiLU prologue at kappa = 1000    err <= 2 x (fp32 ATen on the CPU, same sc / sh) + the family's own bound
    training kernels        mean / rstd as sc / sh (gamma = 1, beta = 0); y, dx, dgamma, dbeta <= 2 x fp32 CPU autograd + 3e-6 / 1e-5
    whole network           err <= 2 x (fp32 oracle against the float64 oracle) + 1e-4 (1 + max|ref|), fused against reading too

2e-5 is the suite's well-conditioned M2 bound; 1e-7 kappa is 4 x the 2.4e-8 kappa of a pairwise fp32 Chan merge from two-value
leaves (each partial mean is rounded at the scale of the offset); 8 u L is 4 x the 1.1 * 2 u L of the same merge.  The
sum-of-squares shortcut misses the M2 bound 60-fold at kappa = 100.  No number here comes from the kernels under test.

Worst errors measured on an MI355X as a share of the bound they were held to (each case prints its own: `pytest -s`):

    block (worst case of it)                          measured                 bound
    channel_stats  mean / M2                          1.4e-04 / 1.3e-07        4.8e-04 / 2.0e-05   (no growth in kappa: two passes)
    wino44h normal  mean / M2                         4.0e-06 / 3.2e-05        1.8e-05 / 1.3e-04   M2: 2.1e-8 kappa
    wino44h upsample                                  5.4e-06 / 2.9e-05        2.5e-05 / 1.3e-04
    wino44h split launch (reduce pass)                2.4e-06 / 3.1e-05        9.1e-06 / 1.3e-04   2.5e-8 kappa
    s2h, both forms                                   1.0e-05 / 2.6e-05        4.9e-05 / 1.3e-04   2.0e-8 kappa
    small-cin direct kernel                           9.2e-06 / 2.7e-05        4.9e-05 / 2.0e-04   1.2e-8 kappa
    F(2x2) upsample (wino)                            4.7e-06 / 5.5e-05        1.8e-05 / 1.2e-04   3.5e-8 kappa
    d3s                                               7.6e-06 / 3.2e-05        4.8e-05 / 1.3e-04   2.2e-8 kappa
    gn_finalize  sc / sh                              4.9e-06 / 3.0e-08        1.2e-04 / 2.6e-07
    gn_finalize  const: sc / normalised value         3.1e-05 / 8.3e-05        6.1e-05 / 2.7e-04   (sc: 1 ulp)
    gn_scale_shift wave<4|8|16>, block  sc / sh       6.6e-07 / 4.0e-08        2.4e-05 / 4.8e-07
    gn_scale_shift  const: sc / normalised value      1.9e-06 / 6.0e-05        1.9e-06 / 1.6e-04   (sc: 2 ulp in wave<4>, 1 ulp elsewhere)
    prologue wino44h / wino44  max (fp32 ATen)        3.0e-05 / 3.5e-05 (8.3e-05)    1.4e-03
    prologue wino / d3s                               2.6e-05 (6.8e-05) / 2.3e-05 (6.3e-05)    2.4e-04 / 1.4e-04
    prologue mfma / direct / conv1x1_dma              7.8e-05 / 7.7e-05 / 1.5e-04 (= fp32 ATen's)    2.6e-04 / 2.7e-04 / 4.4e-04
    training  mean, rstd as sc / sh                   1.2e-06 / 4.5e-08        2.2e-05 / 5.1e-07
    training  y / dx / dgamma / dbeta                 3.9e-05 / 3.3e-05 / 6.8e-05 / 4.5e-05    6.6e-05 / 7.6e-05 / 2.1e-04 / 7.4e-05
    training  const: dbeta against sum dy             2.1e-07                  2e-06
    UNet  fused / reading / fused - reading           6.4e-06 / 6.1e-06 / 7.6e-06    2.8e-04   (fp32 oracle: 2.2e-06)

Every merging epilogue's M2 error grows linearly in kappa (kappa = 10 / 100 / 1000: 4.5e-07 / 3.0e-06 / 3.2e-05 on wino44h); none
needed more than 1e-7 kappa, and no kernel needed a fix.  With the leaf of conv_wino44r.hip's epilogue replaced by a
sum-of-squares leaf (a scratch build, discarded) the kappa = 100 cases of wino44h miss their M2 bound 18- to 70-fold.
"""

import math

import pytest
import torch
import torch.nn.functional as F
from test_gpu_conv_select import _assert_ran, launched  # noqa: F401  (launched: the fixture)
from test_gpu_rect import _launch
from test_gpu_unet import _pair

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GROUPS, EPS = 32, 1e-6
NORMAL, STRIDE2, UPSAMPLE2 = 0, 1, 2
DC = {"dc10": 10.0, "dc100": 100.0, "dc1000": 1000.0}
CONST = {"const0": 0.0, "const0.5": 0.5, "const-3": -3.0, "const1024": 1024.0}
PATTERNS = (*DC, "chan_dc", "slice_dc", "tiny", *CONST, "one_live")


def _note(block, what, **shares):
    """measured / bound per quantity, as tests/test_gpu_rect.py prints them"""
    print(f"gnc[{block}] {what}: " + ", ".join(f"{k} {e:.3e} / {b:.3e} ({e / b if b else 0.0:.2f})" for k, (e, b) in shares.items()))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) & 0x7FFFFFFF)


def _ramp(H, W, levels):
    """[H, W]: contiguous runs of H W / levels pixels at levels from +50 down to -50 (two levels: the halves of the plane)"""
    lv = torch.linspace(50.0, -50.0, levels)
    return lv[(torch.arange(H * W) * levels) // (H * W)].view(H, W)


def _pattern(name, B, C, H, W, g, parts=1):
    """[B, C, H, W] of one input pattern; groups of C / 32 channels"""
    cpg = max(C // GROUPS, 1)
    if name in CONST:
        return torch.full((B, C, H, W), CONST[name])
    x = torch.randn(B, C, H, W, generator=g)
    if name in DC:
        x += DC[name]
    elif name == "chan_dc":
        x[:, ::cpg] += 1000.0
    elif name == "slice_dc":
        x += _ramp(H, W, max(2, parts))
    elif name == "tiny":
        x *= 1e-3
    elif name == "one_live":
        live = torch.zeros(C, dtype=torch.bool)
        live[::cpg] = True
        x[:, ~live] = 0.0
    return x


def _pow2(n):
    return n & (n - 1) == 0


# ---- 1. emitted statistics -------------------------------------------------------------------------------------------------------

def _hold_slab(block, what, y, st, parts, nref=8):
    """st [B, C, parts, 2] against the float64 {mean, M2} of the slices of y (contiguous runs of HW / parts values), per slice."""
    B, C = y.shape[:2]
    assert st is not None and tuple(st.shape) == (B, C, parts, 2), None if st is None else st.shape
    assert y[0, 0].numel() % parts == 0
    n = min(B, nref)
    yd = y[:n].double().cpu().reshape(n, C, parts, -1)
    got = st[:n].double().cpu()
    assert torch.isfinite(got).all()
    mean = yd.mean(-1)
    m2 = (yd - mean[..., None]).pow(2).sum(-1)
    L, sigma = yd.abs().amax(-1), (m2 / yd.shape[-1]).sqrt()
    flat = m2 == 0  # constant slices (const(c), the dead channels of one_live): exact
    assert torch.equal(got[..., 0][flat], mean[flat]) and (got[..., 1][flat] == 0).all(), (what, "constant slices")
    live = ~flat
    if not live.any():
        print(f"gnc[{block}] {what}: {int(flat.sum())} constant slices exact")
        return
    kappa = L[live] / sigma[live]
    e_mean, b_mean = (got[..., 0] - mean).abs()[live], 8 * U * L[live]
    e_m2, b_m2 = (got[..., 1] - m2).abs()[live] / m2[live], 2e-5 + 1e-7 * kappa
    i, j = int((e_mean / b_mean).argmax()), int((e_m2 / b_m2).argmax())
    _note(block, f"{what} kappa {kappa.max().item():.3g}", mean=(e_mean[i].item(), b_mean[i].item()), M2=(e_m2[j].item(), b_m2[j].item()))
    assert (e_mean <= b_mean).all(), (what, e_mean[i].item(), b_mean[i].item())
    assert (e_m2 <= b_m2).all(), (what, e_m2[j].item(), b_m2[j].item(), kappa[j].item())


@pytest.mark.parametrize("HW", [256, 1024, 4096, 49, 16388])
def test_channel_stats_conditioning(device, HW):
    """channel_stats_kernel<1 | 4 | 16> (planes held in registers), the scalar path (49) and a plane beyond the register limit."""
    from ddpm_ood_amd import ops

    H = {256: 16, 1024: 32, 4096: 64, 49: 7, 16388: 4}[HW]
    for name in PATTERNS:
        if name in CONST and not _pow2(HW):
            continue
        x = _pattern(name, 2, 64, H, HW // H, _gen(HW, PATTERNS.index(name))).to(device)
        st = ops.channel_stats(x)
        _hold_slab("channel_stats", f"HW {HW} {name}", x, st, 1)
        assert torch.equal(st, ops.channel_stats(x))


W44 = {"DDPM_CONV_WINO44": "2"}  # lifts the launch-size gate of the F(4x4) kernels, so that B stays small
ALL3 = ("wino", "wino44", "wino44h", "d3h")
# (id, family, stats parts, B, Cin, Cout, input H, mode, weight forms, env, takes a residual, split launch): the smallest emitting
# shapes of the families' own tests, one per distinct parts value
EMIT = [
    ("w44h-8", "wino44h", 1, 3, 64, 64, 8, NORMAL, ("wino44h",), W44, True, False),
    ("w44h-16", "wino44h", 1, 3, 64, 64, 16, NORMAL, ("wino44h",), W44, True, False),
    ("w44h-32", "wino44h", 2, 2, 64, 64, 32, NORMAL, ("wino44h",), W44, True, False),
    ("w44h-64", "wino44h", 8, 1, 64, 64, 64, NORMAL, ("wino44h",), W44, True, False),
    ("w44h-up-16", "wino44h", 2, 2, 256, 256, 16, UPSAMPLE2, ("wino44h",), W44, False, False),
    ("w44h-up-8", "wino44h", 1, 3, 256, 256, 8, UPSAMPLE2, ("wino44h",), W44, False, False),
    ("w44h-split-32", "wino44h", 4, 16, 128, 128, 32, NORMAL, ("wino44h",), {}, True, True),
    ("w44h-split-16", "wino44h", 1, 32, 256, 256, 16, NORMAL, ("wino44h",), {}, True, True),
    ("s2h-32", "s2h", 2, 3, 128, 128, 32, STRIDE2, ("wino44h",), {}, False, False),
    ("s2h4-32", "s2h", 2, 513, 16, 128, 32, STRIDE2, ("wino44h",), {}, False, False),
    ("small-cin-32", "direct", 4, 2, 1, 128, 32, NORMAL, (), {}, False, False),
    ("wino-up-16", "wino", 8, 2, 256, 256, 16, UPSAMPLE2, ("wino",), {}, True, False),
    ("wino-up-8", "wino", 2, 3, 256, 256, 8, UPSAMPLE2, ("wino",), {}, True, False),
    ("wino-up-4", "wino", 1, 3, 64, 128, 4, UPSAMPLE2, ("wino",), {}, True, False),
    ("d3s-8", "d3s", 1, 1, 128, 128, 8, NORMAL, ALL3, {}, False, False),
]


def _pack(ops, w, mode, names):
    pack = {"wino": ops.pack_wino_weight, "wino44": ops.pack_wino44_weight,
            "wino44h": ops.pack_conv_s2h_weight if mode == STRIDE2 else ops.pack_wino44h_weight, "d3h": ops.pack_conv_d3h_weight}
    out = {n: pack[n](w) for n in names}
    assert all(v is not None for v in out.values()), {n: v is not None for n, v in out.items()}
    return out


def _out_extent(mode, e):
    return (e + 1) // 2 if mode == STRIDE2 else 2 * e if mode == UPSAMPLE2 else e


def _emit_operands(name, case, g):
    """(x, w, bias, residual) whose convolution PRODUCES the pattern: offsets through the bias (dc, chan_dc), the slice ramp
    through the residual where the family takes one, else through a centre-tap weight over an input that carries the ramp."""
    _, _, parts, B, Cin, Cout, H, mode, _, _, takes_res, _ = case
    Ho = _out_extent(mode, H)
    cpg = Cout // GROUPS
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)  # output N(0, 1)
    b, residual = torch.zeros(Cout), None
    if name in DC:
        b += DC[name]
    elif name == "chan_dc":
        b[::cpg] = 1000.0
    elif name == "slice_dc" and takes_res:
        residual = _ramp(Ho, Ho, max(2, parts)).expand(B, Cout, Ho, Ho).contiguous()
    elif name == "slice_dc":
        w = torch.zeros_like(w)
        w[torch.arange(Cout), torch.arange(Cout) % Cin, 1, 1] = 1.0
        x = x + _ramp(H, H, max(2, parts))
    elif name == "tiny":
        w *= 1e-3
    elif name in CONST:
        w = torch.zeros_like(w)
        b += CONST[name]
    elif name == "one_live":
        dead = torch.ones(Cout, dtype=torch.bool)
        dead[::cpg] = False
        w[dead] = 0.0
    return x, w, b, residual


@pytest.mark.parametrize("case", EMIT, ids=[c[0] for c in EMIT])
def test_emitted_statistics_conditioning(device, launched, case, monkeypatch):  # noqa: F811
    from ddpm_ood_amd import ops

    cid, family, parts, B, Cin, Cout, H, mode, forms, env, _, split = case
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    if not env:
        monkeypatch.delenv("DDPM_CONV_WINO44", raising=False)
    for name in PATTERNS:
        x, w, b, residual = (None if t is None else t.to(device) for t in _emit_operands(name, case, _gen(B, Cin, H, PATTERNS.index(name))))
        kw = dict(mode=mode, residual=residual, **_pack(ops, w, mode, forms))
        run = lambda: ops.conv(x, w, b, want_stats=True, **kw)  # noqa: E731
        if split:  # (the reduce pass is a second kernel of the same family)
            y, st = _launch(run, family)
        else:
            (y, st), names, report = launched(run)
            _assert_ran(names, report, family)
        _hold_slab(family + {NORMAL: "", STRIDE2: " s2", UPSAMPLE2: " up"}[mode] + (" split" if split else ""), f"{cid} {name}", y, st, parts)
        y_again, st_again = run()
        assert torch.equal(y, y_again) and torch.equal(st, st_again)  # bit-reproducible
        assert torch.equal(y, ops.conv(x, w, b, **kw))  # the same output without statistics
        if name in CONST:
            assert (y == CONST[name]).all()
        if name == "one_live":
            dead = torch.ones(Cout, dtype=torch.bool)
            dead[::Cout // GROUPS] = False
            assert (y[:, dead.to(device)] == 0).all() and (st[:, dead.to(device)] == 0).all()
            assert (st[:, (~dead).to(device), :, 1] > 0).all()
    if split:  # the split launch really ran: the unsplit kernel adds the partial sums in another order
        monkeypatch.setenv("DDPM_CONV_WINO44", "2")
        assert not torch.equal(y, ops.conv(x, w, b, **kw))


# ---- 2. merging and reading kernels ----------------------------------------------------------------------------------------------

def _gn64(x, gamma, beta):
    """float64 GroupNorm of x [B, C, ...] per (image, channel): sc, sh, and the group's mu, L, variance"""
    B, C = x.shape[:2]
    xg = x.double().reshape(B, GROUPS, -1)
    mu = xg.mean(-1)
    var = (xg - mu[..., None]).pow(2).mean(-1)
    ex = lambda t: t.repeat_interleave(C // GROUPS, 1)  # noqa: E731
    sc = gamma.double()[None] * ex(1.0 / (var + EPS).sqrt())
    return sc, beta.double()[None] - sc * ex(mu), ex(mu), ex(xg.abs().amax(-1)), ex(var)


def _ulp32(t):
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


def _hold_sc_sh(block, what, sc, sh, x, gamma, beta, nref=8):
    """fp32 scale / shift [B, C] against the float64 GroupNorm of x (CPU), per channel, with its group's kappa."""
    n = min(x.shape[0], nref)
    sc, sh = sc[:n].double().cpu(), sh[:n].double().cpu()
    assert torch.isfinite(sc).all() and torch.isfinite(sh).all(), what
    sc64, sh64, mu, L, var = _gn64(x[:n], gamma, beta)
    be = beta.double()[None].expand_as(sc64)
    flat = var == 0
    if flat.any():  # const(c): the variance is exactly 0, eps is the whole denominator
        want = (gamma.double() / math.sqrt(EPS)).float()[None].expand_as(sc64)
        e_sc, b_sc = (sc - want.double()).abs()[flat], 2 * _ulp32(want)[flat]
        c = mu[flat]
        e_n, b_n = (c * sc[flat] + sh[flat] - be[flat]).abs(), 4 * U * (sc[flat] * c).abs() + 2 * U * be[flat].abs()
        i, j = int((e_sc - b_sc).argmax()), int((e_n - b_n).argmax())
        _note(block, f"{what} const", sc=(e_sc[i].item(), b_sc[i].item()), norm=(e_n[j].item(), b_n[j].item()))
        assert (e_sc <= b_sc).all() and (e_n <= b_n).all(), (what, e_sc[i].item(), b_sc[i].item(), e_n[j].item(), b_n[j].item())
    live = ~flat
    if live.any():
        kappa = L[live] / var[live].sqrt()
        tol = 1e-5 + 1e-7 * kappa
        e_sc, b_sc = (sc - sc64).abs()[live], tol * sc64.abs()[live]
        e_sh = (sh - sh64).abs()[live]
        b_sh = tol * (sc64 * mu).abs()[live] + 8 * U * (sc64.abs() * L)[live] + 2 * U * be.abs()[live]
        i, j = int((e_sc / b_sc).argmax()), int((e_sh / b_sh).argmax())
        _note(block, f"{what} kappa {kappa.max().item():.3g}", sc=(e_sc[i].item(), b_sc[i].item()), sh=(e_sh[j].item(), b_sh[j].item()))
        assert (e_sc <= b_sc).all(), (what, e_sc[i].item(), b_sc[i].item())
        assert (e_sh <= b_sh).all(), (what, e_sh[j].item(), b_sh[j].item())


def _affine(C, g):
    return torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.3


def _slab(x, parts):
    """[B, C, parts, 2] = {mean, M2} of the slices of x, computed in float64 and rounded to fp32 once"""
    xs = x.double().reshape(x.shape[0], x.shape[1], parts, -1)
    mean = xs.mean(-1)
    return torch.stack([mean, (xs - mean[..., None]).pow(2).sum(-1)], -1).float()


# (B, C1, C2, HW, parts1, parts2): every merge depth alone, and across the seam-straddling concat (384 = 256 + 128: 12 per group)
FINALIZE = [(2, 128, 0, 256, 1, 0), (2, 128, 0, 256, 2, 0), (2, 128, 0, 256, 4, 0), (2, 128, 0, 256, 8, 0),
            (5, 256, 128, 256, 2, 4), (5, 256, 128, 256, 8, 1), (5, 256, 128, 256, 4, 8), (5, 256, 128, 256, 1, 2)]


@pytest.mark.parametrize("case", FINALIZE, ids=["-".join(map(str, c)) for c in FINALIZE])
def test_gn_finalize_conditioning(device, case):
    from ddpm_ood_amd import ops

    B, C1, C2, HW, p1, p2 = case
    C, H = C1 + C2, int(math.isqrt(HW))
    for name in PATTERNS:
        if name in CONST and not _pow2(C // GROUPS * HW):
            continue
        g = _gen(*case, PATTERNS.index(name))
        x = _pattern(name, B, C, H, H, g, parts=max(p1, p2))
        gamma, beta = _affine(C, g)
        st1, st2 = _slab(x[:, :C1], p1).to(device), _slab(x[:, C1:], p2).to(device) if C2 else None
        sc, sh = ops.gn_finalize(st1, gamma.to(device), beta.to(device), GROUPS, EPS, HW, stats2=st2)
        _hold_sc_sh("gn_finalize" + (" concat" if C2 else ""), f"parts {p1}/{p2} {name}", sc, sh, x, gamma, beta)
        sc2, sh2 = ops.gn_finalize(st1, gamma.to(device), beta.to(device), GROUPS, EPS, HW, stats2=st2)
        assert torch.equal(sc, sc2) and torch.equal(sh, sh2)


# (B, C1, C2, HW) -> gn_scale_shift_wave_kernel<4>, <8>, <16>, the block kernel, its scalar path, the concat
READING = [("wave4", 2, 128, 0, 64), ("wave8", 2, 256, 0, 256), ("wave16", 2, 128, 0, 1024), ("block", 2, 128, 0, 4096),
           ("block-scalar", 3, 32, 0, 49), ("concat", 2, 256, 128, 256)]


@pytest.mark.parametrize("case", READING, ids=[c[0] for c in READING])
def test_gn_scale_shift_conditioning(device, case):
    from ddpm_ood_amd import ops

    cid, B, C1, C2, HW = case
    C, H = C1 + C2, int(math.isqrt(HW))
    for name in PATTERNS:
        if name in CONST and not _pow2(C // GROUPS * HW):
            continue
        g = _gen(B, C1, C2, HW, PATTERNS.index(name))
        x = _pattern(name, B, C, H, H, g, parts=2)
        gamma, beta = _affine(C, g)
        x1, x2 = x[:, :C1].contiguous().to(device), x[:, C1:].contiguous().to(device) if C2 else None
        sc, sh = ops.gn_scale_shift(x1, gamma.to(device), beta.to(device), GROUPS, EPS, x2=x2)
        _hold_sc_sh("gn_scale_shift " + cid, name, sc, sh, x, gamma, beta)


# ---- 3. the GroupNorm (+ SiLU) prologue of the convolutions at kappa = 1000 ---------------------------------------------------------

# (family, B, C, Cout, H, ksize, weight forms, env, the family's well-conditioned bound: tests/test_gpu_rect.py's table)
PROLOGUE = [
    ("wino44h", 2, 128, 128, 32, 3, ("wino44h",), W44, "f44"),
    ("wino44", 2, 128, 128, 32, 3, ("wino44",), W44, "f44"),
    ("wino", 3, 128, 128, 8, 3, ("wino",), {}, "f32"),
    ("mfma", 2, 128, 128, 16, 3, (), {}, "f32"),
    ("d3s", 1, 128, 128, 8, 3, ALL3, {}, "d3s"),
    ("conv1x1_dma", 67, 128, 384, 16, 1, (), {}, "f32"),
    ("direct", 2, 64, 64, 12, 3, (), {}, "f32"),
]


@pytest.mark.parametrize("case", PROLOGUE, ids=[c[0] for c in PROLOGUE])
def test_conv_prologue_conditioning(device, launched, case, monkeypatch):  # noqa: F811
    """x = N(0, 1) + 1000 under sc / sh computed in float64 and rounded to fp32 once: fp32 itself loses about kappa 2 u here, so
    the yardstick is the fp32 CPU evaluation of the same expression, not a fixed number."""
    from ddpm_ood_amd import ops

    family, B, C, Cout, H, k, forms, env, tol = case
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    g = _gen(B, C, Cout, H, k)
    x = _pattern("dc1000", B, C, H, H, g)
    w = torch.randn(Cout, C, k, k, generator=g) / math.sqrt(C * k * k)
    b = torch.randn(Cout, generator=g)
    gamma, beta = _affine(C, g)
    sc64, sh64, *_ = _gn64(x, gamma, beta)
    sc, sh = sc64.float(), sh64.float()
    act = lambda t: F.silu(t) if k == 3 else t  # noqa: E731  (the q / k / v projection has no activation)
    n = min(B, 8)
    ref = F.conv2d(act(x[:n].double() * sc[:n].double()[:, :, None, None] + sh[:n].double()[:, :, None, None]), w.double(), b.double(), padding=k // 2)
    aten = F.conv2d(act(x[:n] * sc[:n, :, None, None] + sh[:n, :, None, None]), w, b, padding=k // 2).double()
    d = lambda t: t.to(device)  # noqa: E731
    kw = _pack(ops, d(w), NORMAL, forms)
    (y, names, report) = launched(lambda: ops.conv(d(x), d(w), d(b), gscale=d(sc), gshift=d(sh), act=int(k == 3), **kw))
    _assert_ran(names, report, family)
    y = y[:n].double().cpu()
    scale = ref.abs().max().item()
    err, e_aten = (y - ref).abs().max().item(), (aten - ref).abs().max().item()
    own = {"f32": 2e-5 * (1 + scale), "f44": 2e-4 * (1 + scale), "d3s": 3e-6 * scale}[tol]
    shares = {"max": (err, 2 * e_aten + own), "aten": (e_aten, 2 * e_aten + own)}
    assert math.isfinite(err)
    if tol == "f44":
        rms = lambda t: t.pow(2).mean().sqrt().item()  # noqa: E731
        r, r_aten = rms(y - ref), rms(aten - ref)
        shares["rms"] = (r, 2 * r_aten + 1e-5 * (1 + rms(ref)))
        shares["aten rms"] = (r_aten, shares["rms"][1])
    _note("prologue " + family, f"{case[1:6]}", **shares)
    assert all(e <= bnd for e, bnd in shares.values()), shares


# ---- 4. training kernels ---------------------------------------------------------------------------------------------------------------

def _relmax(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("B,C,H", [(2, 64, 4), (2, 64, 5), (3, 256, 8), (1, 128, 64)])
def test_gn_training_kernels_conditioning(device, B, C, H):
    """gn_stats_kernel + gn_apply_kernel, gn_fwd_reg_kernel (planes of <= 1024 values), gn_bwd_reg_kernel / gn_bwd_kernel (the
    64 x 64 plane, the odd plane), accumulate off and on, against float64 autograd with fp32 CPU autograd as the yardstick."""
    from ddpm_ood_amd import train_ops as T

    dev = lambda t: t.to(device)  # noqa: E731
    for name in PATTERNS:
        const = name in CONST
        if const and not _pow2(C // GROUPS * H * H):
            continue
        act = 0 if const else 1
        g = _gen(B, C, H, PATTERNS.index(name))
        x = _pattern(name, B, C, H, H, g, parts=2)
        gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
        dy, base = torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)
        out = {}
        for dt in (torch.float64, torch.float32):
            xd, gd, bd = (t.to(dt).requires_grad_(True) for t in (x, gamma, beta))
            y = F.group_norm(xd, GROUPS, gd, bd, eps=EPS)
            y = F.silu(y) if act else y
            out[dt] = (y.detach(), *torch.autograd.grad(y, (xd, gd, bd), dy.to(dt)))
        ref, aten = out[torch.float64], out[torch.float32]
        e_aten = [_relmax(a, r) for a, r in zip(aten, ref)]  # y, dx, dgamma, dbeta
        mr = T.gn_stats(dev(x), GROUPS, EPS)
        y2 = T.gn_apply(dev(x), mr, dev(gamma), dev(beta), GROUPS, act)
        y1, mr1 = T.gn_forward(dev(x), dev(gamma), dev(beta), GROUPS, EPS, act)
        one = torch.ones(GROUPS), torch.zeros(GROUPS)
        for what, m in (("gn_stats", mr), ("gn_forward", mr1)):  # [B, G, 2] = {mean, rstd}: sc / sh of gamma = 1, beta = 0
            xg = x.reshape(B, GROUPS, -1)
            _hold_sc_sh("train " + what, f"{(B, C, H)} {name}", m[..., 1], -m[..., 1] * m[..., 0], xg, *one)
            mu64 = xg.double().mean(-1)
            Lg = xg.double().abs().amax(-1)
            assert ((m[..., 0].double().cpu() - mu64).abs() <= 8 * U * Lg).all(), (what, name)
        dgam, dbet = torch.empty(C, device=device), torch.empty(C, device=device)
        dx = T.gn_backward(dev(x), dev(dy), mr, dev(gamma), dev(beta), GROUPS, act, dgam, dbet)
        acc = T.gn_backward(dev(x), dev(dy), mr, dev(gamma), dev(beta), GROUPS, act, dgam, dbet, dx=dev(base), accumulate=True)
        assert all(torch.isfinite(t).all() for t in (y1, y2, dx, acc, dgam, dbet)), name
        if const:  # the issue's contract for constant groups: finite gradients, dbeta = sum dy
            e = _relmax(dbet, dy.double().sum(dim=(0, 2, 3)))
            _note("train const", f"{(B, C, H)} {name}", dbeta=(e, 2e-6))
            assert e <= 2e-6, (name, e)
            continue
        scale_dx = ref[1].abs().max().item()
        e_acc = float((acc.double().cpu() - (ref[1] + base.double())).abs().max())
        shares = {"y reg": (_relmax(y1, ref[0]), 2 * e_aten[0] + 3e-6), "y 2k": (_relmax(y2, ref[0]), 2 * e_aten[0] + 3e-6),
                  "dx": (_relmax(dx, ref[1]), 2 * e_aten[1] + 1e-5),
                  "dx acc": (e_acc, 2 * e_aten[1] * scale_dx + 1e-5 * (ref[1] + base.double()).abs().max().item()),
                  "dgamma": (_relmax(dgam, ref[2]), 2 * e_aten[2] + 1e-5), "dbeta": (_relmax(dbet, ref[3]), 2 * e_aten[3] + 1e-5)}
        _note("train", f"{(B, C, H)} {name}", **shares)
        assert all(e <= bnd for e, bnd in shares.values()), (name, shares)


# ---- 5. whole network: fused statistics (the attention epilogue among them) against reading statistics ------------------------------

@pytest.mark.parametrize("variant", ["dc100", "dead_group"])
def test_unet_fused_statistics_conditioning(device, variant, monkeypatch):
    """The small UNet at (1, 96, 32): every GroupNorm from the producers' epilogues, the N = 64 attention epilogue included.
    dc100: conv_in's bias raised until the first residual stream sits at kappa ~ 100.  dead_group: conv_in's first group of output
    channels zeroed -- constant planes all the way to the first GroupNorm."""
    import ctypes
    import json

    from ddpm_ood_amd import _lib
    from ddpm_ood_amd.synthetic import random_state_dict

    B, H, n = 96, 32, 4
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, 1, H, H, generator=g)
    t = torch.randint(0, 1000, (B,), generator=g)
    sd = random_state_dict("small", 1, seed=1)
    wk, bk = "conv_in.conv.weight", "conv_in.conv.bias"
    if variant == "dc100":
        h = F.conv2d(x[:n].double(), sd[wk].double(), sd[bk].double(), padding=1)
        sd[bk] = sd[bk] + float(100.0 * h.std())
        h = F.conv2d(x[:n].double(), sd[wk].double(), sd[bk].double(), padding=1).reshape(n, GROUPS, -1)
        kappa = (h.abs().amax(-1) / h.std(-1)).median().item()
        assert 50 <= kappa <= 200, kappa
    else:
        cpg = sd[wk].shape[0] // GROUPS
        sd[wk][:cpg] = 0.0
        sd[bk][:cpg] = 0.0
    ref, hip = _pair(device, 1)
    ref.load_state_dict(sd)
    hip.load_state_dict(sd)
    lib = _lib.load()
    lib.ddpm_prof_enable(1)
    y_fused = hip(x.to(device), timesteps=t.to(device)).cpu()
    torch.cuda.synchronize()
    lib.ddpm_prof_enable(0)
    buf = ctypes.create_string_buffer(1 << 18)
    prof = json.loads(buf.value.decode()) if lib.ddpm_prof_report(buf, len(buf)) > 0 else {}
    assert "gn_finalize" in prof and "gn_scale_shift" not in prof, sorted(prof)
    monkeypatch.setenv("DDPM_GN_FUSED", "0")
    y_read = hip(x.to(device), timesteps=t.to(device)).cpu()
    assert torch.isfinite(y_fused).all() and torch.isfinite(y_read).all()
    with torch.no_grad():
        y32 = ref(x[:n], timesteps=t[:n]).double()
        y64 = ref.double()(x[:n].double(), timesteps=t[:n])
    scale = y64.abs().max().item()
    assert scale > 0.05
    e_oracle = (y32 - y64).abs().max().item()
    bound = 2 * e_oracle + 1e-4 * (1 + scale)
    shares = {"fused": ((y_fused[:n].double() - y64).abs().max().item(), bound), "reading": ((y_read[:n].double() - y64).abs().max().item(), bound),
              "fused - reading": ((y_fused - y_read).abs().max().item(), bound), "fp32 oracle": (e_oracle, bound)}
    _note("UNet", variant, **shares)
    assert all(e <= bnd for e, bnd in shares.values()), shares
