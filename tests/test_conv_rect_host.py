"""CPU: the convolution selection table (csrc/conv_dispatch.hip) on rectangular images and non-cubic volumes.

tools/record_conv_dispatch.py's sweep (and the fixture recorded from it) only knows Wi == Hi.  The product takes the axes
separately (--image_roi is a per-axis crop), so this sweep sets Wi / Wo on their own and holds the four host-only answers to
the contracts their callers rely on: d3s / d3s2 refuse rectangles, statistics only come from the families that write them and
in a slicing ddpm_gn_finalize_f32 accepts (parts <= 8, Ho * Wo % parts == 0: a rectangle gives 3 and 6 for the first time),
the scratch the library asks for covers what the selected kernel uses, and ddpm_conv_takes_wino44h names the kernel that runs.
Pointers only matter for NULL-ness and alignment and device_cus() answers 256 without a device: the answers are an MI355X's.
"""

import ctypes as C
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# the rows of the two tables, the families with a stats_parts function, the `lib` fixture and the recorder: from the square test
square = _load("test_conv_dispatch_host", ROOT / "tests" / "test_conv_dispatch_host.py")
rec, lib = square.rec, square.lib
PLANAR, VOLUMETRIC, WRITES_STATS = square.PLANAR, square.VOLUMETRIC, square.WRITES_STATS

from ddpm_ood_amd._lib import ConvDesc  # noqa: E402  (record_conv_dispatch put the repository root on sys.path)

SQUARE_ONLY = ("d3s", "d3s2")        # `if (d.Ho != d.Wo) return false;` in their takes
NOT_AN_IMAGE = ("linear_skinny",)    # Linear: 1 x 1 "images" only

EXTENTS = (4, 8, 12, 16, 24, 32, 48, 64, 128)
CHANNELS = ((64, 0, 64), (128, 0, 128), (256, 128, 256), (1, 0, 128), (128, 0, 3))
BATCHES = (1, 16, 256)
KMODES = ((1, rec.NORMAL), (3, rec.NORMAL), (3, rec.STRIDE2), (3, rec.UPSAMPLE2))
# 3-D image axes: 64 is in it because the split-f16 F(4x4) kernel only takes 3-D slices of one image per item (>= 32 tiles in 9
# or 10 staging units of 64 pixels), and the smallest rectangles of that kind are 16 x 64 and 64 x 16
VOL_EXTENTS = (8, 16, 32, 64)
P = rec.P
PTR_NAMES = rec.PTRS


def _out(k, mode, e):
    return {rec.NORMAL: e, rec.STRIDE2: (e + 1) // 2 if k == 3 else e // 2, rec.UPSAMPLE2: 2 * e, rec.TRANSPOSE2: 2 * e}[mode]


def _desc(ptrs, c1, c2, b, cout, hi, wi, k, mode, di=0, do=0, dims=0):
    """A descriptor with the two image axes on their own (record_conv_dispatch.descriptor sets Wi = Hi)."""
    d = ConvDesc()
    ptrs |= P["in2"] if c2 else 0
    for i, n in enumerate(PTR_NAMES):
        if ptrs >> i & 1 and n != "scratch":
            setattr(d, n, 0x100000 * (i + 1))
    d.C1, d.C2, d.B, d.Cout, d.ksize, d.mode = c1, c2, b, cout, k, mode
    d.Hi, d.Wi, d.Ho, d.Wo = hi, wi, _out(k, mode, hi), _out(k, mode, wi)
    d.Di, d.Do, d.dims = di, do, dims
    if d.gscale:
        d.act = 1
    d.chan_add_stride = cout if d.chan_add else 0
    return d


def _planar(lib):
    """-> [(what, descriptor, wants scratch)]: the engine's weight forms, with scratch; for B = 16 also with the GroupNorm
    prologue + epilogue addends, and without scratch."""
    base = P["in1"] | P["out"] | P["bias"]
    out = []
    for c1, c2, cout in CHANNELS:
        for k, mode in KMODES:
            eng = base | rec.engine_forms(lib, c1 + c2, cout, k, mode)
            for hi in EXTENTS:
                for wi in EXTENTS:
                    if hi == wi:
                        continue
                    for b in BATCHES:
                        what = dict(C1=c1, C2=c2, Cout=cout, k=k, mode=mode, Hi=hi, Wi=wi, B=b)
                        out.append((what, _desc(eng, c1, c2, b, cout, hi, wi, k, mode), True))
                        if b == 16:
                            fused = eng | P["gscale"] | P["gshift"] | P["chan_add"] | P["residual"]
                            out.append((dict(what, fused=1), _desc(fused, c1, c2, b, cout, hi, wi, k, mode), True))
                            out.append((dict(what, scratch=0), _desc(eng, c1, c2, b, cout, hi, wi, k, mode), False))
    return out


def _volumetric():
    base = P["in1"] | P["out"] | P["bias"] | P["w_packed"]
    w, w44, w44h = P["w_wino"], P["w_wino44"], P["w_wino44h"]
    out = []
    for c in (128, 256):
        for dd in (1, 4, 8, 32):
            for hi in VOL_EXTENTS:
                for wi in VOL_EXTENTS:
                    if hi == wi:
                        continue
                    for b in (1, 16):
                        what = dict(C=c, D=dd, Hi=hi, Wi=wi, B=b)
                        for forms in (0, w, w | w44, w | w44 | w44h):
                            out.append((dict(what, op="k3", forms=forms),
                                        _desc(base | forms, c, 0, b, c, hi, wi, 3, rec.NORMAL, di=dd, do=dd, dims=3), True))
                        if dd >= 2:
                            out.append((dict(what, op="k4s2"),
                                        _desc(base, c, 0, b, c, hi, wi, 4, rec.STRIDE2, di=dd, do=dd // 2, dims=3), True))
                        out.append((dict(what, op="transpose"),
                                    _desc(base, c, 0, b, c, hi, wi, 4, rec.TRANSPOSE2, di=dd, do=2 * dd, dims=3), True))
    return out


def _ask(lib, d, scratch):
    """rec.ask for a ready descriptor: the scratch is attached at the size the library asks for."""
    d.scratch, d.scratch_floats = None, 0
    need = lib.ddpm_conv_scratch_floats(C.byref(d))
    if scratch and need:
        d.scratch, d.scratch_floats = 0x100000 * len(PTR_NAMES), need
    ref = C.byref(d)
    return (lib.ddpm_conv_kernel_name(ref).decode(), lib.ddpm_conv_stats_parts(ref), lib.ddpm_conv_scratch_floats(ref),
            lib.ddpm_conv_takes_wino44h(ref))


@pytest.fixture(scope="module")
def answers(lib):
    """{setting name: [(table, what, descriptor copy, (family, parts, scratch floats, takes wino44h))]} over both sweeps."""
    rows = [("2d",) + r for r in _planar(lib)] + [("3d",) + r for r in _volumetric()]
    out = {}
    for s in rec.SETTINGS:
        with rec.setting(lib, s):
            got = []
            for table, what, d, scratch in rows:
                a = _ask(lib, d, scratch)
                c = ConvDesc()
                C.memmove(C.byref(c), C.byref(d), C.sizeof(d))  # with the scratch _ask attached under this setting
                got.append((table, what, c, a))
        out[s["name"]] = got
    return out


def _each(answers):
    for name, rows in answers.items():
        for table, what, d, a in rows:
            yield (name, table, what), table, d, a


def test_sweep_is_rectangular_and_validates(answers):
    """Every descriptor has H != W, and a validated descriptor always gets a family (the planar table ends in `direct`, the
    volumetric one in `mfma`, for which these channel counts have a tiling)."""
    n = 0
    for what, table, d, (name, *_r) in _each(answers):
        assert d.Hi != d.Wi and d.Ho != d.Wo, what
        assert name in (PLANAR if table == "2d" else VOLUMETRIC), (what, name)
        n += 1
    assert n == len(rec.SETTINGS) * len(answers["default"]) and len(answers["default"]) > 4000


def test_square_only_families_refuse_rectangles(answers):
    for what, table, d, (name, *_r) in _each(answers):
        assert name not in SQUARE_ONLY, (what, name)


def test_statistics_contract_holds_on_rectangles(answers):
    """parts > 0 only from a family that writes stats_out, and only in a slicing ddpm_gn_finalize_f32 takes: parts <= 8 slices
    of Ho * Wo / parts pixels each."""
    seen = set()
    for what, table, d, (name, parts, _s, _t) in _each(answers):
        assert parts >= 0, (what, parts)
        if parts == 0:
            continue
        assert name in WRITES_STATS and table == "2d", (what, name, parts)
        assert parts <= 8 and (d.Ho * d.Wo) % parts == 0, (what, name, parts)
        seen.add(parts)
    assert {3, 6} <= seen, seen  # the slicings only a rectangle produces


def test_scratch_asked_for_covers_the_selected_kernel(lib, answers):
    for name, rows in answers.items():
        s = next(x for x in rec.SETTINGS if x["name"] == name)
        with rec.setting(lib, s):
            for table, what, d, (fam, _p, scratch, _t) in rows:
                assert scratch >= lib.ddpm_conv_kernel_scratch_floats(C.byref(d)), (name, what, fam)


def test_takes_wino44h_agrees_with_the_name(lib, answers):
    """As tests/test_conv_dispatch_host.py::test_answers_are_consistent_with_the_selected_row builds it: the descriptor
    ddpm_conv_takes_wino44h asks about has w_wino44h and a scratch as large as needed."""
    huge = C.c_size_t(-1).value
    took = 0
    for name, rows in answers.items():
        s = next(x for x in rec.SETTINGS if x["name"] == name)
        with rec.setting(lib, s):
            for table, what, d, (fam, _p, scratch, takes) in rows:
                if table == "3d" or d.ksize != 3:
                    assert not takes, (name, what)
                if fam == "wino44h" and table == "2d" and d.mode == rec.NORMAL:
                    assert takes, (name, what)  # it runs there: it would run there
                if not takes:
                    continue
                e = ConvDesc()
                C.memmove(C.byref(e), C.byref(d), C.sizeof(d))
                e.w_wino44h = e.w_wino44h or 0x5000000
                if not e.scratch:
                    e.scratch, e.scratch_floats = 0x4000000, huge
                assert lib.ddpm_conv_kernel_name(C.byref(e)) == b"wino44h", (name, what)
                took += 1
    assert took >= 100, took


def test_sweep_reaches_every_family_that_takes_rectangles(answers):
    sel = {}
    for what, table, d, (name, *_r) in _each(answers):
        sel[(table, name)] = sel.get((table, name), 0) + 1
    for n in PLANAR:
        if n not in SQUARE_ONLY + NOT_AN_IMAGE:
            assert sel.get(("2d", n), 0) >= 5, f"planar row {n}: selected by {sel.get(('2d', n), 0)} rectangular descriptors"
    for n in VOLUMETRIC:
        assert sel.get(("3d", n), 0) >= 3, f"volumetric row {n}: selected by {sel.get(('3d', n), 0)} non-cubic descriptors"
