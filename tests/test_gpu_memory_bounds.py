"""-m gpu: guard bands and poisoned buffers around every kernel's memory (tests/guard_util.py).

The rest of the suite asks whether the tensor a kernel was supposed to produce is close to a reference.  This file asks what
it cannot see: did the kernel write anywhere else, does the result depend on memory the caller never handed over, and does
it depend on what an uninitialised output / scratch / partials buffer happened to hold?

Every case runs one entry point three times:

  ordinary   the wrapper of ops.py / train_ops.py on ordinary tensors (torch.empty from the caching allocator);
  poisoned   the same call with EVERY pointer inside one guard-band arena: the inputs (weights and packed forms, bias, scale and
             shift, residual, chan_add) are arena views that are frozen bitwise, and every buffer the wrapper allocates itself --
             outputs, scratch, partials, statistics slabs, each sized by the library's size function -- is an arena view of
             exactly that size, filled with the poison NaN (guard_util.arena_allocations replaces the wrapper module's
             ``torch.empty``); guard_util.pointers_in_arena asserts for every C-ABI call that each pointer lies in the arena;
  zeroed     as poisoned, the writable views zero-filled.

and asserts (1) arena.check(): no write outside a writable view, none into an input; (2) the poisoned run's results are finite
and bit-identical to the ordinary run's (the arena preserves the 256-byte alignment, so the same kernel is selected; a NaN
means a value from outside the buffers was used arithmetically, multiplied by a zero mask included); (3) the zeroed run gives the
poisoned run's bits.  (4) Convolutions that use scratch run again with a scratch of exactly ddpm_conv_kernel_scratch_floats (the
same bits) and of one float less ("too small: runs unsplit": guards intact, and the result within the family's existing
tolerance against float64 -- the only non-bitwise comparison of this file; each bound names the test it comes from).

Convolutions run under a spy on ddpm_conv_f32 (as tests/test_gpu_rect.py::_launch): it records the family
ddpm_conv_kernel_name reports for the launched descriptor, which every case asserts, and swaps the scratch for (4).
"""

import contextlib
import ctypes
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from guard_util import POISON, Arena, arena_allocations, need_bytes, pointers_in_arena
from test_gpu_conv_select import CASES_2D, CASES_3D, PROF_KEYS
from test_gpu_ops import CONV_CASES
from test_gpu_train_ops import WGRAD

pytestmark = pytest.mark.gpu

NORMAL, STRIDE2, UPSAMPLE2 = 0, 1, 2


# ---- the three runs -------------------------------------------------------------------------------------------------------------

def _mods():
    from ddpm_ood_amd import ops, train_ops

    return [ops, train_ops]


def _nbytes(t):
    return t.numel() * t.element_size()


class _Run:
    pass


@contextlib.contextmanager
def _stop_on_gpu_fault():
    """A HIP error (an illegal access, a failed launch) ends the session: nothing more is started on a device that has faulted."""
    try:
        yield
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"GPU fault, stopping: {e}", returncode=3)
        raise


@contextlib.contextmanager
def _conv_spy(lib, log, scratch, alloc):
    """Spy on ddpm_conv_f32: log (family, ddpm_conv_kernel_scratch_floats, scratch floats given, ddpm_conv_kernel_scratch_floats of the launched
    descriptor, the swapped-in scratch) per launch.  scratch = "kernel" /
    "minus1": the launch gets a copy of the descriptor whose scratch is alloc(n) with n = what the selected family alone uses / one
    float less (only where it uses any)."""
    from ddpm_ood_amd._lib import ConvDesc

    inner = lib.ddpm_conv_f32
    keep = []

    def spy(desc, stream):
        d = ConvDesc.from_buffer_copy(desc._obj)
        nk = lib.ddpm_conv_kernel_scratch_floats(ctypes.byref(d))
        if scratch is not None and nk > 0:
            n = nk if scratch == "kernel" else nk - 1
            buf = alloc(n)
            keep.append(buf)
            d.scratch, d.scratch_floats = (buf.data_ptr() if n else None), n
        log.append((lib.ddpm_conv_kernel_name(ctypes.byref(d)).decode(), nk, int(d.scratch_floats),
                    lib.ddpm_conv_kernel_scratch_floats(ctypes.byref(d)), keep[0] if scratch is not None and nk > 0 else None))
        keep.append(d)
        return inner(ctypes.byref(d), stream)

    lib.ddpm_conv_f32 = spy
    try:
        yield
    finally:
        lib.ddpm_conv_f32 = inner


def _run(device, inputs, call, arena_sizes=None, zero=False, scratch=None):
    """call(tensors) -> tuple of result tensors (None allowed).  inputs: name -> (CPU tensor or None, input_only).  arena_sizes
    None: the ordinary run (and the byte sizes of the wrapper's allocations); else every tensor in an arena holding those sizes."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    r = _Run()
    r.log, r.called = [], []
    live = {k: v for k, v in inputs.items() if v[0] is not None}
    unet_fns = [n for n in _lib.SIGNATURES if n.startswith("ddpm_unet_")]  # (their void * arguments are engine handles)
    with _stop_on_gpu_fault():
        return _run_guarded(device, lib, r, live, call, arena_sizes, zero, scratch, unet_fns)


def _run_guarded(device, lib, r, live, call, arena_sizes, zero, scratch, unet_fns):
    from ddpm_ood_amd import _lib

    torch.cuda.synchronize()
    if arena_sizes is None:
        t = {k: v.to(device) for k, (v, _) in live.items()}
        with arena_allocations(_mods()) as alloc, _conv_spy(lib, r.log, scratch, lambda n: torch.empty(n, device=device)):
            res = call(t)
        torch.cuda.synchronize()
        r.arena = None
    else:
        sizes = [_nbytes(v) for v, _ in live.values()] + list(arena_sizes) + [max(arena_sizes, default=0)] * (scratch is not None)
        arena = r.arena = Arena(device, need_bytes(sizes))
        t = {k: arena.alloc(v.shape, v.dtype, fill=v, name=k, input_only=frozen) for k, (v, frozen) in live.items()}
        arena.freeze()
        with arena_allocations(_mods(), arena, zero) as alloc, pointers_in_arena(lib, _lib.SIGNATURES, arena, skip=unet_fns) as r.called, \
                _conv_spy(lib, r.log, scratch, lambda n: arena.alloc((n,), torch.float32, name=f"scratch[{n}]")):
            res = call(t)
        arena.check()  # (1)
    r.sizes, r.allocated = alloc.sizes, alloc.allocated
    r.res = [None if v is None else v.detach().clone() for v in (res if isinstance(res, (tuple, list)) else (res,))]
    return r


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, i)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, i, x.shape, y.shape)
            # torch.equal on the integer view: bitwise, so that a NaN compares equal to itself and -0.0 differs from 0.0
            ix, iy = (v.contiguous().reshape(-1).view(torch.uint8) for v in (x, y))
            assert torch.equal(ix, iy), f"{what}: result {i} differs in {int((ix != iy).sum())} of {ix.numel()} bytes"


def _all_finite(res, what):
    for i, x in enumerate(res):
        if x is not None and x.is_floating_point():
            assert bool(torch.isfinite(x).all()), f"{what}: result {i} holds {int((~torch.isfinite(x)).sum())} non-finite values"


def _bounds(device, inputs, call, size_fns=(), size_of=lambda n: n):
    """The three runs and assertions (1) - (3).  size_fns: size functions the call has to ask, each answer the exact element
    count (size_of(answer), where the buffer is a known multiple of it) of one of the buffers the call then allocated."""
    plain = _run(device, inputs, call)
    poison = _run(device, inputs, call, plain.sizes)
    zeroed = _run(device, inputs, call, plain.sizes, zero=True)
    _all_finite(poison.res, "poisoned run")  # (2)
    _same_bits(plain.res, poison.res, "ordinary vs poisoned arena")
    _same_bits(poison.res, zeroed.res, "poisoned vs zeroed arena")  # (3)
    for fn in size_fns:
        answers = {ret for name, ret in poison.called if name == fn}
        assert answers, f"{fn} was not asked"
        for n in answers - {0}:
            assert any(a.numel() == size_of(n) for a in poison.allocated), f"{fn} answered {n}: no buffer of exactly {size_of(n)}"
    return plain, poison


def _g(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0xFFFFFF)


def _env(monkeypatch, env):
    for var, val in (env or {}).items():
        monkeypatch.setenv(var, val)  # (conftest: a DDPM_* setenv reloads the library's switches)


# ---- 0. the detector on the device ------------------------------------------------------------------------------------------------

def test_arena_on_the_device_detects_a_single_element_write(device):
    """tests/test_guard_util_host.py's tampering on the device: plain torch indexing writes inside the arena's own allocation."""
    from guard_util import ALIGN, POISON, GuardViolation

    def arena():
        a = Arena(device, need_bytes([4 * 15, 2 * 7, 4 * 33]))
        x = a.alloc((3, 5), torch.float32, fill=torch.arange(15.0).view(3, 5), name="x", input_only=True)
        h = a.alloc((7,), torch.float16, name="h")
        y = a.alloc((33,), torch.float32, name="y")
        a.freeze()
        return a, x, h, y

    a, x, h, y = arena()
    assert all(t.data_ptr() % ALIGN == 0 and t.is_cuda for t in (x, h, y))
    assert y.view(torch.int32).cpu().tolist() == [POISON] * 33 and bool(torch.isnan(y).all())
    y.fill_(1.0)
    a.check()
    v = a.view_of(y)
    a.base[v.end:v.end + 4] = 0  # one element behind y
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view="y", side="after", offset=0, words=1)]
    a, x, h, y = arena()
    v = a.view_of(y)
    a.base[v.start - 4:v.start] = 0  # one element in front of y
    a.base[a.view_of(h).end:a.view_of(h).end + 2] = 0  # one f16 behind h (a view whose end is no multiple of 4)
    x[1, 1] = -1.0  # and a frozen input modified
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view="h", side="after", offset=0, words=1), dict(view="y", side="before", offset=4, words=1),
                                dict(view="x", side="input", offset=24, words=1)]


# ---- 1. convolutions: every row of the selection tables ------------------------------------------------------------------------

ALL3 = ("wino", "wino44", "wino44h", "d3h")
W44 = {"DDPM_CONV_WINO44": "2"}  # lifts the launch-size gate of the F(4x4) kernels, so that B stays small
D3S = {"DDPM_CONV_D3S": "2"}     # the small-launch kernels whatever the launch size


def K(name, family, B, C1, C2, Cout, H, W, k, mode, forms=(), *, parts=None, env=None, gn=False, act=False, chan=False, res=False,
      split_f16=True, linear=False, force_direct=False):
    return dict(name=name, family=family, B=B, C1=C1, C2=C2, Cout=Cout, H=H, W=W, k=k, mode=mode, forms=tuple(forms), parts=parts,
                env=env, gn=gn, act=act, chan=chan, res=res, split_f16=split_f16, linear=linear, force_direct=force_direct)


def _ragged(i, family, forms=(), env=None, tag="", **kw):
    """Row i of tests/test_gpu_ops.py::CONV_CASES (chan_add at chan_add_offset = 32 where the row takes it)."""
    B, C1, C2, Cout, H, k, mode, gn, act, chan, res = CONV_CASES[i]
    return K(f"ragged-{B}x{C1}+{C2}-{Cout}-{H}-k{k}m{mode}{tag}", family, B, C1, C2, Cout, H, H, k, mode, forms, env=env, gn=gn, act=act,
             chan=chan, res=res, **kw)


CONV_2D = [K("select-" + c[0], c[1], c[3], c[4], c[5], c[6], c[7], c[7], c[8], c[9], c[10], parts=c[2],
             split_f16=c[11].get("split_f16", True), linear=c[1] == "linear_skinny") for c in CASES_2D]
# the ragged rows of CONV_CASES (28x28: 4-row tiles of 112 / 128 px; 14x14: 7-row tiles; 7x7: two images per tile; odd batches; the
# GroupNorm group straddling the concat seam), each through every family that takes it
R28, R28S2, R14, R7, R7UP, R8ODD, R16SEAM = (CONV_CASES.index(row) for row in (  # (by value: .index raises if a row leaves the list)
    (3, 128, 0, 128, 28, 3, 0, True, True, True, False), (3, 128, 0, 128, 28, 3, 1, False, False, False, False),
    (2, 256, 128, 256, 14, 3, 0, True, True, True, False), (5, 256, 256, 256, 7, 3, 0, True, True, True, False),
    (3, 256, 0, 256, 7, 3, 2, False, False, False, False), (5, 256, 256, 256, 8, 3, 0, True, True, True, False),
    (2, 256, 128, 256, 16, 3, 0, True, True, True, False)))
D3S0 = {"DDPM_CONV_D3S": "0"}
CONV_2D += [
    # 28 / 14 / 7-wide images have no Winograd / split-f16 tiling: with every form attached the MFMA kernel's ragged tiles still run
    _ragged(R28, "mfma"), _ragged(R28, "direct", force_direct=True, tag="-direct"), _ragged(R28, "mfma", ALL3, env=W44, tag="-forms"),
    _ragged(R28S2, "mfma"), _ragged(R28S2, "mfma", ("wino44h", "d3h"), env=D3S, tag="-forms"),
    _ragged(R14, "mfma"), _ragged(R14, "mfma", ALL3, env=W44, tag="-forms"),
    _ragged(R7, "mfma"), _ragged(R7, "mfma", ALL3, env={**W44, **D3S}, tag="-forms"),
    _ragged(R7UP, "mfma"), _ragged(R7UP, "mfma", ("folded", "wino", "wino44h", "d3h"), env={**W44, **D3S}, tag="-forms"),
    _ragged(R7UP, "mfma", ("folded", "wino", "wino44h", "d3h"), env={"DDPM_UP_WINO44H": "0"}, tag="-upw44h0"),
    # odd batch at 8x8, and the GroupNorm group straddling the concat seam at 16x16: through every family that takes them
    _ragged(R8ODD, "mfma"), _ragged(R8ODD, "d3s", ALL3, tag="-d3s"), _ragged(R8ODD, "wino", ALL3, env=D3S0, tag="-forms"),
    _ragged(R8ODD, "wino44h", ALL3, env={**W44, **D3S0}, tag="-w44"),
    _ragged(R8ODD, "wino44", ALL3, env={**W44, **D3S0, "DDPM_WINO44_F16X3": "0"}, tag="-w44-f32"),
    _ragged(R8ODD, "mfma", env={"DDPM_CONV_SPLITK": "0"}, tag="-splitk0"), _ragged(R8ODD, "mfma", env={"DDPM_CONV_SPLITK": "1"}, tag="-splitk1"),
    _ragged(R8ODD, "wino", ALL3, env={**D3S0, "DDPM_WINO44_SPLIT": "0"}, tag="-w44split0"),
    _ragged(R16SEAM, "mfma"), _ragged(R16SEAM, "d3s", ALL3, tag="-d3s"), _ragged(R16SEAM, "wino", ALL3, env=D3S0, tag="-forms"),
    _ragged(R16SEAM, "wino44h", ALL3, env={**W44, **D3S0}, tag="-w44"),
    _ragged(R16SEAM, "wino44", ALL3, env={**W44, **D3S0, "DDPM_WINO44_F16X3": "0"}, tag="-w44-f32"),
    # upsample on the F(4x4) kernel and with it switched off; the split-K of the fused q / k / v projection (test_conv_mfma_split_k)
    K("up-w44h-8", "wino44h", 2, 128, 0, 128, 8, 8, 3, UPSAMPLE2, ("wino", "wino44h"), env={**W44, **D3S0}),
    K("up-w44h-off-8", "wino", 2, 128, 0, 128, 8, 8, 3, UPSAMPLE2, ("wino", "wino44h"), env={**W44, **D3S0, "DDPM_UP_WINO44H": "0"}),
    K("splitk-qkv", "mfma", 4, 256, 0, 768, 8, 8, 1, NORMAL, gn=True),
    K("splitk-s2", "mfma", 16, 256, 0, 256, 16, 16, 3, STRIDE2, chan=True),
    K("d3s2-16", "d3s2", 3, 128, 0, 128, 16, 16, 3, STRIDE2, ("wino44h", "d3h"), env=D3S),
    K("d3s-up-8", "d3s", 3, 128, 0, 256, 8, 8, 3, UPSAMPLE2, ("d3h",), env=D3S),
    K("d1s-concat-8", "d1s", 5, 256, 128, 256, 8, 8, 1, NORMAL, ("d3h",), env=D3S, res=True),
    K("w44-split-8", "wino44", 128, 128, 0, 256, 8, 8, 3, NORMAL, ("wino", "wino44"), gn=True, act=True, chan=True, res=True),
    K("w44h-split-48x32", "wino44h", 16, 128, 0, 128, 48, 32, 3, NORMAL, ("wino", "wino44h"), gn=True, act=True, chan=True, res=True),
    K("s2h-form2-32x16", "s2h", 5, 128, 0, 128, 32, 16, 3, STRIDE2, ("wino44h",), env={"DDPM_DOWN_S2H": "2"}),
    K("s2h-form3-16x32", "s2h", 5, 128, 0, 128, 16, 32, 3, STRIDE2, ("wino44h",), env={"DDPM_DOWN_S2H": "3"}),
]
# Rectangles.  12 x 20 and 20 x 12 with the forms of one family per tiling attached: the selection table gives none of the Winograd /
# split-f16 / DMA families a tiling at these extents (5 and 3 tiles of four: no item shape), so the family each case asserts is
# the one the table falls to -- still with that family's forms in the descriptor.  Next to each, the smallest rectangle pair the
# family does take (tests/test_gpu_rect.py::CASES).  Odd extents into stride 2 ((Hi + 1) // 2): 7 -> 4 and 15 -> 8.
for _h, _w in ((12, 20), (20, 12)):
    CONV_2D += [
        K(f"rect-{_h}x{_w}-w44h-forms-run-mfma", "mfma", 9, 128, 0, 128, _h, _w, 3, NORMAL, ("wino44h",), env=W44),
        K(f"rect-{_h}x{_w}-wino-forms-run-mfma", "mfma", 3, 128, 0, 128, _h, _w, 3, NORMAL, ("wino",), gn=True, act=True, chan=True, res=True),
        K(f"rect-{_h}x{_w}-s2h-forms-run-mfma", "mfma", 3, 128, 0, 128, _h, _w, 3, STRIDE2, ("wino44h",)),
        K(f"rect-mfma-{_h}x{_w}", "mfma", 3, 256, 128, 256, _h, _w, 3, NORMAL, gn=True, act=True, chan=True, res=True),
        K(f"rect-direct-{_h}x{_w}", "direct", 2, 64, 0, 64, _h, _w, 3, NORMAL),
        K(f"rect-{_h}x{_w}-dma-forms-run-mfma", "mfma", 16, 256, 128, 256, _h, _w, 1, NORMAL, ("wino44h",), gn=True, res=True),
        K(f"rect-{_h}x{_w}-d1s-forms-run-mfma", "mfma", 1, 256, 128, 256, _h, _w, 1, NORMAL, ("wino44h", "d3h"), gn=True, res=True),
    ]
for _h, _w in ((8, 32), (32, 8)):
    CONV_2D += [K(f"rect-w44h-{_h}x{_w}", "wino44h", 9, 64, 0, 64, _h, _w, 3, NORMAL, ("wino44h",), env=W44)]
for _h, _w in ((8, 16), (16, 8)):
    CONV_2D += [
        K(f"rect-wino-{_h}x{_w}", "wino", 3, 128, 0, 128, _h, _w, 3, NORMAL, ("wino",), gn=True, act=True, chan=True, res=True),
        K(f"rect-s2h-{_h}x{_w}", "s2h", 3, 128, 0, 128, _h, _w, 3, STRIDE2, ("wino44h",)),
        K(f"rect-d1s-{_h}x{_w}", "d1s", 1, 256, 128, 256, _h, _w, 1, NORMAL, ("wino44h", "d3h"), gn=True, res=True),
    ]
for _h, _w in ((32, 64), (64, 32)):
    CONV_2D += [K(f"rect-dma-{_h}x{_w}", "conv1x1_dma", 16, 128, 0, 128, _h, _w, 1, NORMAL, ("wino44h",), gn=True, res=True)]
for _h, _w in ((7, 15), (15, 7)):
    CONV_2D += [
        K(f"odd-s2-mfma-{_h}x{_w}", "mfma", 3, 128, 0, 128, _h, _w, 3, STRIDE2),
        K(f"odd-s2-direct-{_h}x{_w}", "direct", 3, 64, 0, 64, _h, _w, 3, STRIDE2),
        K(f"odd-s2-forms-{_h}x{_w}", "mfma", 3, 128, 0, 128, _h, _w, 3, STRIDE2, ("wino44h", "d3h"), env=D3S),
    ]


def _out_extent(mode, e):
    return (e + 1) // 2 if mode == STRIDE2 else 2 * e if mode == UPSAMPLE2 else e


def _conv2d_operands(device, c):
    """-> inputs (CPU tensors; all input-only) and ref(): the float64 reference.  GroupNorm scale / shift and the packed weight
    forms are made on the device by the ordinary wrappers."""
    from ddpm_ood_amd import ops

    g = _g(c["name"])
    B, C1, C2, Cout, H, W, k, mode = (c[n] for n in ("B", "C1", "C2", "Cout", "H", "W", "k", "mode"))
    Cin = C1 + C2
    x = torch.randn(B, C1, H, W, generator=g) * 1.3 + 0.2
    x2 = torch.randn(B, C2, H, W, generator=g) * 1.5 + 0.3 if C2 else None
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    Ho, Wo = _out_extent(mode, H), _out_extent(mode, W)
    gamma = beta = chan_add = residual = gscale = gshift = None
    d = lambda t: None if t is None else t.to(device)  # noqa: E731
    if c["gn"]:
        gamma, beta = torch.randn(Cin, generator=g) * 0.2 + 1, torch.randn(Cin, generator=g) * 0.2
        gscale, gshift = (t.cpu() for t in ops.gn_scale_shift(d(x), d(gamma), d(beta), 32, 1e-6, x2=d(x2)))
    if c["chan"]:
        chan_add = torch.randn(B, Cout + 64, generator=g)
    if c["res"]:
        residual = torch.randn(B, Cout, Ho, Wo, generator=g)
    if c["linear"]:
        x, w = x[:, :, 0, 0].contiguous(), w[:, :, 0, 0].contiguous()
    pack = {"wino": ops.pack_wino_weight, "wino44": ops.pack_wino44_weight, "folded": ops.fold_upsample_weight,
            "wino44h": ops.pack_conv1x1_h_weight if k == 1 else ops.pack_conv_s2h_weight if mode == STRIDE2 else ops.pack_wino44h_weight,
            "d3h": ops.pack_conv_d1s_weight if k == 1 else ops.pack_conv_d3h_weight}
    forms = {n: pack[n](d(w)) for n in c["forms"]}
    assert all(v is not None for v in forms.values()), {n: v is not None for n, v in forms.items()}
    packed = ops.pack_conv_weight(d(w))
    inputs = dict(x=x, x2=x2, w=w, b=b, gscale=gscale, gshift=gshift, chan_add=chan_add, residual=residual,
                  packed=None if packed is None else packed.cpu(), **{n: v.cpu() for n, v in forms.items()})

    def ref():
        xin = (x if x2 is None else torch.cat([x, x2], 1)).double()
        w64 = w.double()
        if c["linear"]:
            xin, w64 = xin[:, :, None, None], w64[:, :, None, None]
        if c["gn"]:
            xin = F.group_norm(xin, 32, gamma.double(), beta.double(), 1e-6)
        if c["act"]:
            xin = F.silu(xin)
        if mode == UPSAMPLE2:
            xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        y = F.conv2d(xin, w64, b.double(), stride=2 if mode == STRIDE2 else 1, padding=k // 2)
        if chan_add is not None:
            y = y + chan_add.double()[:, 32:32 + Cout, None, None]
        return y if residual is None else y + residual.double()

    return {n: (v, True) for n, v in inputs.items()}, ref


def _conv2d_call(c, forms=None, want_stats=True):
    from ddpm_ood_amd import ops

    forms = c["forms"] if forms is None else forms

    def call(t):
        return ops.conv(t["x"], t["w"], t["b"], x2=t.get("x2"), gscale=t.get("gscale"), gshift=t.get("gshift"), act=int(c["act"]),
                        mode=c["mode"], chan_add=t.get("chan_add"), chan_add_offset=32 if c["chan"] else 0, residual=t.get("residual"),
                        packed=t.get("packed"), want_stats=want_stats, force_direct=c["force_direct"], **{n: t[n] for n in forms})

    return call


FP32 = ("linear_skinny", "wino", "mfma", "direct", "conv1x1_dma")


def _hold(family, y, ref, y_fp32=None):
    """The bound the family's own test holds it to against float64 (the "too small" runs: the only tolerances of this file)."""
    y, scale = y.detach().cpu().double(), ref.abs().max().item()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    err = (y - ref).abs().max().item()
    assert math.isfinite(err)
    if family in FP32:  # tests/test_gpu_ops.py::_close (test_conv, test_conv_mfma_split_k, test_conv_winograd)
        bound = 2e-5 * (1 + scale)
    elif family in ("wino44", "wino44h"):  # tests/test_gpu_ops.py::test_conv_winograd_f4x4 (and _channel_split)
        bound = 2e-4 * (1 + scale)
        rms, rbound = (y - ref).pow(2).mean().sqrt().item(), 1e-5 * (1 + ref.pow(2).mean().sqrt().item())
        assert rms < rbound, (family, rms, rbound)
    elif family in ("d3s", "d3s2", "d1s"):  # test_conv_small_launch_split_f16_vs_conv2d, test_conv_stride2_small_launch_vs_conv2d,
        bound = 3e-6 * scale                # test_conv1x1_small_launch_split_f16_vs_conv2d (tests/test_gpu_ops.py)
    else:  # s2h: tests/test_gpu_ops.py::test_conv_stride2_split_f16_vs_conv2d
        assert family == "s2h", family
        e_old = (y_fp32.detach().cpu().double() - ref).abs().max().item()
        bound = max(2 * e_old, 2e-6 * scale)
    print(f"bounds[{family}] too-small scratch: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (family, err, bound)


def _scratch_sizes(device, inputs, call, plain, poison, ref, fp32_call=None, small_call=None):
    """(4): the scratch at exactly ddpm_conv_kernel_scratch_floats, and one float less.  small_call: the call without a statistics
    slab (the slab is sized for the family that takes the full scratch; with less, another family may run)."""
    family, nk, given = poison.log[0][:3]
    if nk == 0:
        return
    assert given >= nk, (given, nk)  # (the default run: exactly ddpm_conv_scratch_floats, asserted by _bounds)
    exact = _run(device, inputs, call, plain.sizes, scratch="kernel")
    assert [e[0] for e in exact.log] == [family] and exact.log[0][2] == nk, exact.log
    _same_bits(poison.res, exact.res, "scratch of ddpm_conv_scratch_floats vs ddpm_conv_kernel_scratch_floats")
    small = _run(device, inputs, small_call or call, plain.sizes, scratch="minus1")  # arena.check(): the too-small scratch's guards are intact
    ran = small.log[0][0]
    assert small.log[0][2] == nk - 1, small.log
    # No assertion can be made on the too-small scratch's contents or on the bits: the launcher takes the largest split whose
    # slabs fit the scratch it was given (the size function is an upper bound over the splits it may choose, so one float less
    # often runs the very same split), or the table falls to a family with a smaller need -- each may write the buffer, and
    # the first may give the same bits.  What is asserted is the bound: nothing behind the nk - 1 floats (arena.check() above; a
    # launcher that ran a split of the full advertised size would put its last float on the first guard word), and the result.
    assert small.log[0][4].numel() == nk - 1
    _all_finite(small.res[:1], "scratch one float too small")
    y32 = _run(device, inputs, fp32_call).res[0] if ran == "s2h" else None
    _hold(ran, small.res[0], ref(), y32)


@pytest.mark.parametrize("c", CONV_2D, ids=[c["name"] for c in CONV_2D])
def test_conv2d_stays_inside_its_buffers(device, monkeypatch, c):
    from ddpm_ood_amd import _lib

    _env(monkeypatch, c["env"])
    prev = _lib.set_split_f16(c["split_f16"])
    try:
        inputs, ref = _conv2d_operands(device, c)
        call = _conv2d_call(c)
        plain, poison = _bounds(device, inputs, call, size_fns=("ddpm_conv_scratch_floats",))
        for r in (plain, poison):
            assert [e[0] for e in r.log] == [c["family"]], (r.log, c["family"])
        y, st = poison.res
        parts = [ret for name, ret in poison.called if name == "ddpm_conv_stats_parts"][-1]
        assert (st is None) == (parts == 0) and (st is None or tuple(st.shape) == (c["B"], c["Cout"], parts, 2))
        if c["parts"] is not None:
            assert parts == c["parts"], (parts, c["parts"])
        _scratch_sizes(device, inputs, call, plain, poison, ref, _conv2d_call(c, forms=(), want_stats=False), _conv2d_call(c, want_stats=False))
    finally:
        _lib.set_split_f16(prev)


# (name, family, B, Cin, Cout, (D, H, W), op, weight forms, residual): the rows of CASES_3D, non-cubic volumes through each of them, and the
# split-K of the MFMA kernel on 4^3 volumes (tests/test_gpu_ops.py::test_conv_mfma_split_k)
CONV_3D = [("select-" + c[0], c[1], c[2], c[3], c[3], (c[4], c[5], c[5]), c[6], c[7], False) for c in CASES_3D]
for _v in ((4, 8, 12), (6, 4, 8)):
    _n = "x".join(map(str, _v))
    CONV_3D += [
        (f"k3-mfma-{_n}", "mfma", 2, 128, 128, _v, "k3", (), True),
        (f"k3-wino-{_n}", "mfma", 2, 128, 128, _v, "k3", ("wino",), True),  # (no Winograd tiling at these slices: the forms attached,
        (f"k3-forms-{_n}", "mfma", 2, 128, 128, _v, "k3", ("wino", "wino44", "wino44h"), False),  # the table falls to the MFMA kernel)
        (f"k3s2-mfma-{_n}", "mfma", 2, 128, 128, _v, "k3s2", (), False),
        (f"k4s2-mfma-{_n}", "mfma", 2, 64, 128, _v, "k4s2", (), False),
        (f"transpose-mfma-{_n}", "mfma", 2, 64, 128, _v, "transpose", (), False),
    ]
CONV_3D += [("splitk-4x4x4", "mfma", 2, 256, 256, (4, 4, 4), "k3", (), True),
            # the smallest non-cubic volumes the Winograd families take (tests/test_gpu_rect.py::CASES_3D)
            ("k3-wino-4x8x16", "wino", 1, 128, 128, (4, 8, 16), "k3", ("wino",), True),
            ("k3-wino44-3x16x32", "wino44", 2, 64, 128, (3, 16, 32), "k3", ("wino", "wino44"), True),
            ("k3-wino44h-1x16x64", "wino44h", 1, 64, 128, (1, 16, 64), "k3", ("wino", "wino44", "wino44h"), True),
            ("k3-wino44h-4x64x16", "wino44h", 1, 64, 128, (4, 64, 16), "k3", ("wino", "wino44", "wino44h"), False)]
ENV_3D = {n: W44 for n in ("k3-wino44-3x16x32", "k3-wino44h-1x16x64", "k3-wino44h-4x64x16")}


@pytest.mark.parametrize("c", CONV_3D, ids=[c[0] for c in CONV_3D])
def test_conv3d_stays_inside_its_buffers(device, monkeypatch, c):
    from ddpm_ood_amd import ops

    name, family, B, Cin, Cout, (D, H, W), op, forms, res = c
    _env(monkeypatch, ENV_3D.get(name))
    g = _g(name)
    x = torch.randn(B, Cin, D, H, W, generator=g)
    k = 3 if op in ("k3", "k3s2") else 4
    wshape = (Cin, Cout, k, k, k) if op == "transpose" else (Cout, Cin, k, k, k)
    w = torch.randn(wshape, generator=g) / math.sqrt(Cin * k ** 3)
    b = torch.randn(Cout, generator=g)
    stride = 1 if op == "k3" else 2
    pack = {"wino": ops.pack_wino3d_weight, "wino44": ops.pack_wino44_3d_weight, "wino44h": ops.pack_wino44h_3d_weight}
    kw = {n: pack[n](w.to(device)) for n in forms}
    assert all(v is not None for v in kw.values())
    packed = (ops.pack_convT_weight if op == "transpose" else ops.pack_conv3d_weight)(w.to(device))
    if op == "transpose":
        ref = lambda: F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2, padding=1)  # noqa: E731
        call = lambda t: ops.conv_transpose(t["x"], t["w"], t["b"], packed=t["packed"])  # noqa: E731
        residual = None
    else:
        y0 = F.conv3d(x.double(), w.double(), b.double(), stride=stride, padding=1)
        residual = torch.randn(y0.shape, generator=g) if res else None
        ref = lambda: y0 if residual is None else y0 + residual.double()  # noqa: E731
        call = lambda t: ops.conv3d(t["x"], t["w"], t["b"], stride=stride, packed=t["packed"], residual=t.get("residual"),  # noqa: E731
                                    **{n: t[n] for n in forms})
    inputs = {n: (v, True) for n, v in dict(x=x, w=w, b=b, residual=residual, packed=packed.cpu(), **{n: v.cpu() for n, v in kw.items()}).items()}
    plain, poison = _bounds(device, inputs, call, size_fns=() if op == "transpose" else ("ddpm_conv_scratch_floats",))
    for r in (plain, poison):
        assert [e[0] for e in r.log] == [family], (r.log, family)
    _scratch_sizes(device, inputs, call, plain, poison, ref)


def test_every_convolution_family_has_a_bounds_case():
    """Every family ddpm_conv_kernel_name can return (the families of PROF_KEYS) is asserted by at least one case above."""
    covered = {c["family"] for c in CONV_2D} | {c[1] for c in CONV_3D}
    assert covered == set(PROF_KEYS), set(PROF_KEYS) ^ covered
    assert {c[1] for c in CONV_3D} == {"wino44h", "wino44", "wino", "mfma"}  # the rows of the volumetric table


@pytest.mark.parametrize("force", [True, False])
def test_conv_transpose_as_parity_convolutions_stays_inside_its_buffers(device, monkeypatch, force):
    """pack_convT_parity_weights + conv_transpose_parity: the eight parity tensors (`tmp`) are views of ONE arena buffer, so a
    parity convolution overrunning its slice lands in its neighbour's -- caught by the bitwise comparison of the result."""
    from ddpm_ood_amd import ops

    if force:
        monkeypatch.setenv("DDPM_CONV_WINO44", "2")
    B, Cin, Cout, D, H, W = 3, 64, 128, 2, 32, 32
    g = _g("parity")
    x = torch.randn(B, Cin, D, H, W, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, 4, generator=g) / math.sqrt(Cin * 8)
    b = torch.randn(Cout, generator=g)

    def call(t):
        assert ops.conv_transpose_parity_supported(t["x"], t["w"])
        pw = ops.pack_convT_parity_weights(t["w"])
        return (ops.conv_transpose_parity(t["x"], pw, t["b"], out_act=ops.ACT_RELU, sub_batch=2),) + tuple(p for q in pw for p in q[1:])

    plain, poison = _bounds(device, dict(x=(x, True), w=(w, True), b=(b, True)), call)
    assert {e[0] for e in poison.log} == ({"wino44h"} if force else {e[0] for e in plain.log}) and len(poison.log) == 16


@pytest.mark.parametrize("dims,cin,cout,k,stride,pad,transposed,ext", [
    (2, 3, 5, 3, 1, 1, False, (7, 9)), (2, 8, 16, 4, 2, 1, False, (10, 6)), (2, 16, 8, 4, 2, 1, True, (5, 7)),
    (3, 2, 7, 3, 1, 1, False, (3, 5, 7)), (3, 5, 3, 4, 2, 1, True, (3, 2, 5)), (3, 4, 4, 3, 2, 1, False, (5, 4, 7))])
def test_generic_convolution_stays_inside_its_buffers(device, dims, cin, cout, k, stride, pad, transposed, ext):
    from ddpm_ood_amd import ops

    g = _g("generic", dims, cin, cout, k, stride, transposed)
    x = torch.randn((2, cin) + ext, generator=g)
    w = torch.randn(((cin, cout) if transposed else (cout, cin)) + (k,) * dims, generator=g) / math.sqrt(cin * k ** dims)
    b = torch.randn(cout, generator=g)
    oe = tuple((e - 1) * stride - 2 * pad + k if transposed else (e + 2 * pad - k) // stride + 1 for e in ext)
    res = torch.randn((2, cout) + oe, generator=g)
    _bounds(device, dict(x=(x, True), w=(w, True), b=(b, True), res=(res, True)),
            lambda t: ops.convnd_generic(t["x"], t["w"], t["b"], stride=stride, padding=pad, transposed=transposed, residual=t["res"], relu=True))


@pytest.mark.parametrize("B,C,D,H,W", [(2, 16, 4, 6, 10), (1, 32, 2, 2, 2), (3, 8, 6, 2, 14)])
def test_vqvae_edge_layers_stay_inside_their_buffers(device, B, C, D, H, W):
    """The k4-s2 edge layers of the VQ-VAE: conv3d 1 -> C over [2D, 2H, 2W] and conv_transpose3d C -> 1 over [D, H, W]."""
    from ddpm_ood_amd import ops

    g = _g("edge", B, C, D, H, W)
    x = torch.randn(B, 1, 2 * D, 2 * H, 2 * W, generator=g)
    w = torch.randn(C, 1, 4, 4, 4, generator=g) / 8
    b = torch.randn(C, generator=g)
    _bounds(device, dict(x=(x, True), w=(w, True), b=(b, True)), lambda t: ops.conv3d_k4s2_cin1(t["x"], t["w"], t["b"], relu=True))
    z = torch.randn(B, C, D, H, W, generator=g)
    b1 = torch.randn(1, generator=g)
    _bounds(device, dict(x=(z, True), w=(w, True), b=(b1, True)), lambda t: ops.convT3d_k4s2_cout1(t["x"], t["w"], t["b"]))


# ---- 2. weight packers: the output view is exactly the size function's answer ----------------------------------------------------

def _packers():
    from ddpm_ood_amd import ops

    # (wrapper, its size function, kernel extents, [(Cout, Cin)]: the smallest supported multiples and a second pair that is no
    # power of two)
    return {
        "pack_conv_weight_k3": (ops.pack_conv_weight, "ddpm_packed_conv_weight_floats", (3, 3), [(128, 4), (384, 12)]),
        "pack_conv_weight_k1": (ops.pack_conv_weight, "ddpm_packed_conv_weight_floats", (1, 1), [(128, 4), (384, 12)]),
        "pack_conv_weight_linear": (ops.pack_conv_weight, "ddpm_packed_conv_weight_floats", (), [(128, 4), (384, 12)]),
        "pack_wino_weight": (ops.pack_wino_weight, "ddpm_wino_weight_floats", (3, 3), [(64, 8), (192, 24)]),
        "pack_wino44_weight": (ops.pack_wino44_weight, "ddpm_wino44_weight_floats", (3, 3), [(64, 8), (192, 24)]),
        "fold_upsample_weight": (ops.fold_upsample_weight, "ddpm_folded_upsample_weight_floats", (3, 3), [(128, 8), (384, 24)]),
        "pack_wino44h_weight": (ops.pack_wino44h_weight, "ddpm_wino44h_weight_halves", (3, 3), [(64, 16), (192, 96)]),
        "pack_conv1x1_h_weight": (ops.pack_conv1x1_h_weight, "ddpm_conv1x1_h_weight_halves", (1, 1), [(128, 16), (384, 96)]),
        "pack_conv_d3h_weight": (ops.pack_conv_d3h_weight, "ddpm_conv_d3h_weight_halves", (3, 3), [(128, 8), (384, 24)]),
        "pack_conv_d1s_weight": (ops.pack_conv_d1s_weight, "ddpm_conv_d1s_weight_halves", (1, 1), [(64, 128), (192, 384)]),
        "pack_conv_s2h_weight": (ops.pack_conv_s2h_weight, "ddpm_conv_s2h_weight_halves", (3, 3), [(64, 8), (192, 24)]),
        "pack_conv3d_weight_k3": (ops.pack_conv3d_weight, None, (3, 3, 3), [(128, 4), (384, 12)]),
        "pack_conv3d_weight_k4": (ops.pack_conv3d_weight, None, (4, 4, 4), [(128, 4), (384, 12)]),
        "pack_wino3d_weight": (ops.pack_wino3d_weight, "ddpm_wino_weight_floats", (3, 3, 3), [(64, 8), (192, 24)]),
        "pack_wino44_3d_weight": (ops.pack_wino44_3d_weight, "ddpm_wino44_weight_floats", (3, 3, 3), [(64, 8), (192, 24)]),
        "pack_wino44h_3d_weight": (ops.pack_wino44h_3d_weight, "ddpm_wino44h_weight_halves", (3, 3, 3), [(64, 16), (192, 96)]),
        "pack_convT_weight_2d": (ops.pack_convT_weight, "ddpm_packed_convtr_weight_floats", (4, 4), [(128, 8), (384, 24)]),
        "pack_convT_weight_3d": (ops.pack_convT_weight, "ddpm_packed_convtr_weight_floats", (4, 4, 4), [(128, 8), (384, 24)]),
        "lpips_pack_conv_weight_k5": (ops.lpips_pack_conv_weight, None, (5, 5), [(32, 2), (96, 6)]),
        "lpips_pack_conv_weight_k3": (ops.lpips_pack_conv_weight, None, (3, 3), [(32, 2), (96, 6)]),
    }


PACKERS = ["pack_conv_weight_k3", "pack_conv_weight_k1", "pack_conv_weight_linear", "pack_wino_weight", "pack_wino44_weight",
           "fold_upsample_weight", "pack_wino44h_weight", "pack_conv1x1_h_weight", "pack_conv_d3h_weight", "pack_conv_d1s_weight",
           "pack_conv_s2h_weight", "pack_conv3d_weight_k3", "pack_conv3d_weight_k4", "pack_wino3d_weight", "pack_wino44_3d_weight",
           "pack_wino44h_3d_weight", "pack_convT_weight_2d", "pack_convT_weight_3d", "lpips_pack_conv_weight_k5",
           "lpips_pack_conv_weight_k3"]


@pytest.mark.parametrize("second", [False, True], ids=["smallest", "not-a-power-of-two"])
@pytest.mark.parametrize("name", PACKERS)
def test_weight_packer_fills_exactly_its_size(device, name, second):
    from ddpm_ood_amd import ops

    assert sorted(PACKERS) == sorted(_packers())
    # every pack_* of ops.py is in the table (pack_convT_parity_weights: with conv_transpose_parity above)
    assert {n for n in vars(ops) if n.startswith("pack_")} - {"pack_convT_parity_weights"} <= {f.__name__ for f, *_ in _packers().values()}
    fn, size_fn, kext, chans = _packers()[name]
    cout, cin = chans[second]
    shape = ((cin, cout) if fn is ops.pack_convT_weight else (cout, cin)) + kext
    w = torch.randn(shape, generator=_g(name, second))

    def call(t):
        out = fn(t["w"])
        assert out is not None, (name, shape)
        return out

    # the 3-D forms are one 2-D form per depth tap: 3 n floats for the 2-D answer n; the split-f16 planes share one 64-half tail
    size_of = {"pack_wino3d_weight": lambda n: 3 * n, "pack_wino44_3d_weight": lambda n: 3 * n,
               "pack_wino44h_3d_weight": lambda n: 3 * (n - 64) + 64}.get(name, lambda n: n)
    _bounds(device, dict(w=(w, True)), call, size_fns=(size_fn,) if size_fn else (), size_of=size_of)


# ---- 3. GroupNorm ----------------------------------------------------------------------------------------------------------------

GN_SHAPES = [(2, 256, 256, 64), (2, 256, 0, 256), (2, 128, 0, 1024), (1, 64, 0, 4096), (2, 768, 0, 4096), (1, 64, 0, 49), (1, 96, 0, 1026),
             (3, 256, 128, 256)]  # wave<4>, wave<8>, wave<16>, block register-hold, block loop, block scalar (x 2), the seam


@pytest.mark.parametrize("B,C1,C2,HW", GN_SHAPES)
def test_gn_scale_shift_stays_inside_its_buffers(device, B, C1, C2, HW):
    from ddpm_ood_amd import ops

    g = _g("gn", B, C1, C2, HW)
    x = torch.randn(B, C1, HW, generator=g) * 2 + 0.7
    x2 = torch.randn(B, C2, HW, generator=g) - 1 if C2 else None
    gamma, beta = torch.randn(C1 + C2, generator=g), torch.randn(C1 + C2, generator=g)
    _bounds(device, dict(x=(x, True), x2=(x2, True), gamma=(gamma, True), beta=(beta, True)),
            lambda t: ops.gn_scale_shift(t["x"], t["gamma"], t["beta"], 32, 1e-6, x2=t.get("x2")))


@pytest.mark.parametrize("parts1,parts2", [(1, 0), (3, 0), (8, 0), (3, 8), (1, 1)])
def test_gn_finalize_stays_inside_its_buffers(device, parts1, parts2):
    from ddpm_ood_amd import ops

    g = _g("finalize", parts1, parts2)
    B, C1, C2, hw = 3, 96, 64 if parts2 else 0, 48 * 8

    def slab(C, parts):
        st = torch.randn(B, C, parts, 2, generator=g)
        st[..., 1] = st[..., 1].abs() * hw / parts  # M2 >= 0
        return st

    st1, st2 = slab(C1, parts1), (slab(C2, parts2) if parts2 else None)
    gamma, beta = torch.randn(C1 + C2, generator=g), torch.randn(C1 + C2, generator=g)
    _bounds(device, dict(st=(st1, True), st2=(st2, True), gamma=(gamma, True), beta=(beta, True)),
            lambda t: ops.gn_finalize(t["st"], t["gamma"], t["beta"], 32, 1e-6, hw, stats2=t.get("st2")))


@pytest.mark.parametrize("hw", [16, 1024, 4100, 49])
def test_channel_stats_stays_inside_its_buffers(device, hw):
    from ddpm_ood_amd import ops

    x = torch.randn(3, 40, hw, generator=_g("chanstats", hw)) * 1.5 + 0.4
    _bounds(device, dict(x=(x, True)), lambda t: ops.channel_stats(t["x"]))


# ---- 4. attention ----------------------------------------------------------------------------------------------------------------

def _attention_operands(B, heads, N, with_res):
    Cc = 256 * heads
    g = _g("attention", B, heads, N)
    qkv = torch.randn(B, 3 * Cc, N, generator=g)
    qkv[:, :Cc] *= 1.5
    res = torch.randn(B, Cc, N, generator=g) if with_res else None
    return dict(qkv=(qkv, True), res=(res, True)), 1 / math.sqrt(256)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("B,heads,N", [(2, 1, 8), (1, 3, 100), (2, 2, 256)])
def test_attention_stays_inside_its_buffers(device, B, heads, N, with_res):
    from ddpm_ood_amd import ops

    inputs, scale = _attention_operands(B, heads, N, with_res)
    _, poison = _bounds(device, inputs, lambda t: ops.attention(t["qkv"], t.get("res"), heads, scale, use_scratch=False))
    assert "ddpm_attention_f32" in [n for n, _ in poison.called]


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("B,heads,N,fa", [(3, 1, 64, True), (2, 2, 128, True), (1, 1, 1024, False), (1, 3, 100, True)])
def test_attention_with_scratch_stays_inside_its_buffers(device, monkeypatch, B, heads, N, fa, with_res):
    """ddpm_attention_ws_f32 with a scratch of exactly ddpm_attention_scratch_floats; N = 100 (no multiple of 64) has to ignore the
    scratch it is given: the size function's answer for it, or for N = 128 if that answer is 0."""
    from ddpm_ood_amd import _lib, ops

    if fa:
        monkeypatch.setenv("DDPM_ATTN_FA", "2")
    lib = _lib.load()
    inputs, scale = _attention_operands(B, heads, N, with_res)
    Cc = 256 * heads

    def call(t):
        n = lib.ddpm_attention_scratch_floats(B, Cc, N, heads)
        if N % 64:
            n = n or lib.ddpm_attention_scratch_floats(B, Cc, 128, heads)
        assert n > 0
        out = ops.torch.empty((B, Cc, N), dtype=torch.float32, device=device)
        scratch = ops.torch.empty(n, dtype=torch.float32, device=device)
        ops.check(lib.ddpm_attention_ws_f32(ops.ptr(t["qkv"]), ops.ptr(t.get("res")), ops.ptr(out), B, Cc, N, heads, scale, ops.ptr(scratch), n,
                                            ops.stream_ptr()), "attention")
        return out

    plain, poison = _bounds(device, inputs, call, size_fns=("ddpm_attention_scratch_floats",))
    if N % 64:  # the scratch was ignored: the plain kernel's bits
        y = ops.attention(inputs["qkv"][0].to(device), None if not with_res else inputs["res"][0].to(device), heads, scale, use_scratch=False)
        _same_bits(poison.res, [y], "attention with an unusable scratch vs without")


# ---- 5. elementwise, sampling and noise ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [128, 67])
def test_timestep_embedding_stays_inside_its_buffers(device, dim):
    from ddpm_ood_amd import ops

    t = torch.tensor([0, 650, 990], dtype=torch.int64)
    freqs = torch.exp(-math.log(10000) * torch.arange(0, dim // 2, dtype=torch.float32) / (dim // 2))
    _bounds(device, dict(t=(t, True), freqs=(freqs, True)), lambda v: ops.timestep_embedding(v["t"], v["freqs"], dim))


@pytest.mark.parametrize("shape", [(3, 1, 4, 5), (2, 3, 8, 8), (1, 1, 3, 5), (1, 1, 1, 1), (2, 1, 33, 31)])
def test_add_noise_and_clamp_mse_stay_inside_their_buffers(device, shape):
    import numpy as np

    from ddpm_ood_amd import ops

    g = _g("add_noise", shape)
    x0, noise = torch.rand(shape, generator=g), torch.randn(shape, generator=g)
    a, b = np.linspace(0.3, 0.9, shape[0], dtype=np.float32), np.linspace(0.8, 0.2, shape[0], dtype=np.float32)
    if x0[0].numel() % 4 == 0 or shape[0] == 1:  # the float4 path, and the scalar tail a single image may have
        _bounds(device, dict(x0=(x0, True), noise=(noise, True)), lambda t: ops.add_noise(t["x0"], t["noise"], a, b, b_scale=1.7))
    else:  # a batch of images that are no multiple of 4 floats is refused before anything is launched
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.add_noise(x0.to(device), noise.to(device), a, b, b_scale=1.7)
    rec = torch.randn(shape, generator=g) * 0.8 + 0.5
    _bounds(device, dict(x0=(x0, True), rec=(rec, False)), lambda t: (ops.clamp_mse_(t["x0"], t["rec"], 1.7), t["rec"]))


@pytest.mark.parametrize("numel", [1, 255, 1027])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_plms_step_stays_inside_its_buffers(device, kind, numel):
    from ddpm_ood_amd import ops

    g = _g("plms", kind, numel)
    n_eps = {0: 1, 1: 2, 2: 2, 3: 3, 4: 4}[kind]
    inputs = dict(sample=(torch.randn(numel, generator=g), True), **{f"e{i}": (torch.randn(numel, generator=g), True) for i in range(n_eps)})
    for v in (False, True):
        _bounds(device, inputs, lambda t: ops.plms_step(t["sample"], [t[f"e{i}"] for i in range(n_eps)], kind, 1.01, 0.3, 0.7,
                                                        v_prediction=v, v_a=0.9, v_b=-0.4))  # noqa: B023


@pytest.mark.parametrize("row_numel", [1, 3, 1025])
def test_ancestral_step_and_randn_rows_stay_inside_their_buffers(device, row_numel):
    from ddpm_ood_amd import ops

    B = 3
    g = _g("ancestral", row_numel)
    sample, eps = torch.randn(B, row_numel, generator=g), torch.randn(B, row_numel, generator=g)
    streams = torch.tensor([5, -3, 1 << 40], dtype=torch.int64)
    kw = dict(sqrt_ac=0.8, sqrt_1m_ac=0.6, c0=0.3, ct=0.69, seed=11)
    for pt in ("epsilon", "v_prediction", "sample"):
        _bounds(device, dict(sample=(sample, True), eps=(eps, True), streams=(streams, True)),
                lambda t: ops.ancestral_step(t["sample"], t["eps"], sigma=0.1, row_streams=t["streams"], prediction_type=pt, **kw))  # noqa: B023
    _bounds(device, dict(sample=(sample, True), eps=(eps, True)),
            lambda t: ops.ancestral_step(t["sample"], t["eps"], sigma=0.0, return_pred=False, **kw)[:1])
    _bounds(device, dict(streams=(streams, True)), lambda t: ops.randn_rows((B, row_numel), 11, t["streams"]))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 2, 3, 5, 7)])
def test_simplex_noise_stays_inside_its_buffers(device, shape):
    from ddpm_ood_amd import ops

    seeds = torch.arange(shape[0] * shape[1], dtype=torch.int64).view(shape[0], shape[1]) * 977 + 13
    t = torch.tensor([10, 650], dtype=torch.int64)
    _bounds(device, dict(seeds=(seeds, True), t=(t, True)), lambda v: ops.simplex_noise(shape, v["seeds"], v["t"]))


# ---- 6. training kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (100, 70, 45), (256, 512, 32), (5, 300, 257), (128, 192, 4096), (68, 132, 72)])
def test_gemm_stays_inside_its_buffers(device, M, N, K):
    """tests/test_gpu_train_ops.py::test_gemm_plain_and_transposed_operands: plain into an uninitialised C, then A^T, B^T and a
    transposed C with alpha / beta (C is read: an input that is written)."""
    from ddpm_ood_amd import train_ops as T

    g = _g("gemm", M, N, K)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)

    def plain(t):
        Cm = T.torch.empty(M, N, dtype=torch.float32, device=device)
        return T.gemm(t["A"], t["B"], Cm, M, N, K, a_m=K, a_k=1, b_k=N, b_n=1, c_m=N, c_n=1)

    _, p = _bounds(device, dict(A=(A, True), B=(B, True)), plain, size_fns=("ddpm_gemm_scratch_floats",))
    if (M, N, K) == (128, 192, 4096):  # few tiles and a long K: the K range is split into scratch slabs
        assert max(ret for name, ret in p.called if name == "ddpm_gemm_scratch_floats") > 0
    C0 = torch.randn(N, M, generator=g)
    _bounds(device, dict(A=(A.t().contiguous(), True), B=(B.t().contiguous(), True), C=(C0, False)),
            lambda t: T.gemm(t["A"], t["B"], t["C"], M, N, K, a_m=1, a_k=M, b_k=1, b_n=K, c_m=1, c_n=M, alpha=0.5, beta=2.0),
            size_fns=("ddpm_gemm_scratch_floats",))


def test_gemm_two_level_k_and_batches_stay_inside_their_buffers(device):
    """The strided forms of test_gemm_two_level_k_and_batch_like_a_1x1_weight_gradient_and_attention, the split-f16 one included."""
    from ddpm_ood_amd import train_ops as T

    g = _g("gemm2")
    Bq, co, ci, hw = 5, 192, 128, 64
    dy, x = 0.3 * torch.randn(Bq, co, hw, generator=g), 2.0 * torch.randn(Bq, ci, hw, generator=g)
    for flag in (True, False):
        def wgrad(t):
            dw = T.torch.empty(co, ci, dtype=torch.float32, device=device)
            return T.gemm(t["dy"], t["x"], dw, co, ci, Bq * hw, k_inner=hw, a_m=hw, a_k=1, a_k_outer=co * hw, b_n=hw, b_k=1,
                          b_k_outer=ci * hw, c_m=ci, c_n=1, split_f16=flag)  # noqa: B023

        _bounds(device, dict(dy=(dy, True), x=(x, True)), wgrad, size_fns=("ddpm_gemm_scratch_floats",))
    Bn, heads, d, n = 2, 3, 16, 40
    q, k = torch.randn(Bn, heads * d, n, generator=g), torch.randn(Bn, heads * d, n, generator=g)

    def scores(t):
        S = T.torch.empty(Bn * heads, n, n, dtype=torch.float32, device=device)
        return T.gemm(t["q"], t["k"], S, n, n, d, a_m=1, a_k=n, b_k=n, b_n=1, c_m=n, c_n=1, batch=Bn * heads, batch_inner=heads,
                      a_batch=d * n, a_batch_outer=heads * d * n, b_batch=d * n, b_batch_outer=heads * d * n, c_batch=n * n,
                      c_batch_outer=heads * n * n, alpha=0.25)

    _bounds(device, dict(q=(q, True), k=(k, True)), scores, size_fns=("ddpm_gemm_scratch_floats",))


@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("case", WGRAD, ids=["-".join(map(str, c)) for c in WGRAD])
def test_conv_wgrad_stays_inside_its_buffers(device, case, generic):
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, H, W, k, s = case
    g = _g("wgrad", case)
    a = torch.randn(B, cin, H, W, generator=g)
    dy = torch.randn(B, cout, (H + s - 1) // s, (W + s - 1) // s, generator=g)
    _bounds(device, dict(a=(a, True), dy=(dy, True)), lambda t: T.conv_wgrad(t["a"], t["dy"], k, s, force_generic=generic),
            size_fns=() if generic else ("ddpm_conv_wgrad_scratch_floats",))


def test_conv_wgrad_with_operand_maxima_stays_inside_its_buffers(device):
    """a_absmax / dy_absmax handed in (tests/test_gpu_rect.py::test_conv_wgrad_operand_maxima_on_a_rectangle): two more inputs."""
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, H, W = 3, 64, 128, 8, 16
    g = _g("wgrad-maxima")
    a, dy = 40.0 * torch.randn(B, cin, H, W, generator=g), 3e-7 * torch.randn(B, cout, H, W, generator=g)
    amax, dmax = a.abs().view(B, -1).amax(dim=1).view(torch.int32), dy.abs().view(B * 4, -1).amax(dim=1).view(torch.int32)
    _bounds(device, dict(a=(a, True), dy=(dy, True), amax=(amax, True), dmax=(dmax, True)),
            lambda t: T.conv_wgrad(t["a"], t["dy"], 3, 1, a_absmax=t["amax"], dy_absmax=t["dmax"]), size_fns=("ddpm_conv_wgrad_scratch_floats",))


@pytest.mark.parametrize("case", [(2, 128, 128, (8, 8, 8), 1), (3, 64, 128, (4, 4, 4), 1), (2, 128, 64, (8, 8, 8), 2), (2, 64, 64, (4, 4, 4), 2),
                                  (1, 64, 64, (2, 2, 2), 1), (2, 128, 64, (4, 8, 16), 1), (2, 128, 64, (2, 16, 8), 2)])
def test_conv3d_wgrad_stays_inside_its_buffers(device, case):
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, ext, s = case
    g = _g("wgrad3d", case)
    a = torch.randn((B, cin) + ext, generator=g)
    dy = torch.randn((B, cout) + tuple((e + s - 1) // s for e in ext), generator=g)
    _bounds(device, dict(a=(a, True), dy=(dy, True)), lambda t: T.conv3d_wgrad(t["a"], t["dy"], s), size_fns=("ddpm_conv3d_wgrad_scratch_floats",))


@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
@pytest.mark.parametrize("B,cin,cout,ext", [(2, 128, 64, (8, 12, 16)), (2, 64, 128, (8, 12, 16)), (3, 64, 64, (12, 20)), (2, 1, 8, (8, 12, 16)),
                                            (2, 8, 16, (16, 12)), (16, 64, 64, (16, 16))])
def test_conv_k4s2_wgrad_stays_inside_its_buffers(device, B, cin, cout, ext, generic):
    """tests/test_gpu_k4s2_wgrad.py::CASES and the split pixel stream of its second test, 2-D and 3-D, both forms."""
    from ddpm_ood_amd import train_ops as T

    g = _g("k4s2", B, cin, cout, ext)
    a = torch.randn((B, cin) + ext, generator=g)
    dy = torch.randn((B, cout) + tuple(e // 2 for e in ext), generator=g)
    _bounds(device, dict(a=(a, True), dy=(dy, True)), lambda t: T.conv_k4s2_wgrad(t["a"], t["dy"], force_generic=generic),
            size_fns=("ddpm_conv_k4s2_wgrad_scratch_floats",))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,C,H", [(2, 64, 4), (2, 64, 5), (2, 96, 7), (2, 384, 16), (1, 128, 64)])
def test_group_norm_training_kernels_stay_inside_their_buffers(device, B, C, H, act):
    from ddpm_ood_amd import train_ops as T

    g = _g("gn-train", B, C, H)
    x, dy = torch.randn(B, C, H, H, generator=g) * 1.5 + 0.3, torch.randn(B, C, H, H, generator=g)
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.3
    par = dict(x=(x, True), gamma=(gamma, True), beta=(beta, True))
    _bounds(device, dict(x=(x, True)), lambda t: T.gn_stats(t["x"], 32, 1e-6))
    mr = T.gn_stats(x.to(device), 32, 1e-6).cpu()
    _bounds(device, dict(mr=(mr, True), **par), lambda t: T.gn_apply(t["x"], t["mr"], t["gamma"], t["beta"], 32, act))
    _bounds(device, par, lambda t: T.gn_forward(t["x"], t["gamma"], t["beta"], 32, 1e-6, act, want_absmax=True))
    _bounds(device, par, lambda t: T.gn_forward(t["x"], t["gamma"], t["beta"], 32, 1e-6, act))

    def backward(t, **kw):
        dgamma, dbeta = T.torch.empty(C, dtype=torch.float32, device=device), T.torch.empty(C, dtype=torch.float32, device=device)
        out = T.gn_backward(t["x"], t["dy"], t["mr"], t["gamma"], t["beta"], 32, act, dgamma, dbeta, dx=t.get("dx"), accumulate="dx" in t, **kw)
        return (out if isinstance(out, tuple) else (out,)) + (dgamma, dbeta)

    bw = dict(dy=(dy, True), mr=(mr, True), **par)
    _bounds(device, bw, backward)
    _bounds(device, bw, lambda t: backward(t, want_absmax=True, want_rowsum=True))
    _bounds(device, dict(dx=(torch.randn(B, C, H, H, generator=g), False), **bw), lambda t: backward(t, want_rowsum=True))


@pytest.mark.parametrize("n", [1, 255, 4099])
def test_elementwise_training_kernels_stay_inside_their_buffers(device, n):
    from ddpm_ood_amd import train_ops as T

    g = _g("elementwise", n)
    x, dy, y = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g), torch.randn(n, generator=g)
    _bounds(device, dict(x=(x, True)), lambda t: T.silu(t["x"]))
    _bounds(device, dict(x=(x, True), dy=(dy, True)), lambda t: T.silu_backward(t["x"], t["dy"]))
    _bounds(device, dict(y=(y, True), dy=(dy, True)), lambda t: T.relu_backward(t["y"], t["dy"]))
    _bounds(device, dict(x=(x, True), dy=(dy, True)), lambda t: T.axpby(t["x"], t["dy"], 0.5, -2.0))
    _bounds(device, dict(x=(x, False)), lambda t: T.scale_check_(t["x"], 0.25))
    _bounds(device, dict(x=(x, False)), lambda t: T.fill_(t["x"], 1.5))
    _, p = _bounds(device, dict(x=(x, True), y=(y, True)), lambda t: T.mse_loss_grad(t["x"], t["y"]))
    assert any(a.numel() == (n + 255) // 256 for a in p.allocated)  # the partials: ceil(n / 256)
    # Adam on a flat buffer: parameter and both moments are updated in place
    _bounds(device, dict(p=(x, False), g=(dy, True), m=(y * 0.1, False), v=(y.abs() * 0.01, False)),
            lambda t: (T.adam_step_(t["p"], t["g"], t["m"], t["v"], 1e-3, 0.9, 0.999, 1e-8, 3, 0.5), t["p"], t["m"], t["v"])[1:])
    _bounds(device, {}, lambda t: T.randn((n,), device, 7, 3))


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 33), (300, 5), (5, 300), (64, 256)])
def test_row_column_and_softmax_kernels_stay_inside_their_buffers(device, rows, cols):
    from ddpm_ood_amd import train_ops as T

    g = _g("rows", rows, cols)
    x, dp = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    _bounds(device, dict(x=(x, True)), lambda t: T.row_sum(t["x"], rows, cols))
    _bounds(device, dict(x=(x, True)), lambda t: T.col_sum(t["x"], rows, cols))
    _bounds(device, dict(x=(x, True), acc=(torch.randn(cols, generator=g), False)),
            lambda t: T.col_sum(t["x"], rows, cols, out=t["acc"], alpha=0.5, accumulate=True))
    _bounds(device, dict(s=(x, False)), lambda t: T.softmax_rows_(t["s"], rows, cols))
    p = torch.softmax(x, dim=1)
    _bounds(device, dict(p=(p, True), dp=(dp, False)), lambda t: T.softmax_backward_rows_(t["p"], t["dp"], rows, cols))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 1), (2, 2, 3, 5, 7), (1, 1, 1, 1, 1), (3, 5, 16, 16)])
def test_resampling_and_weight_transposition_stay_inside_their_buffers(device, shape):
    from ddpm_ood_amd import train_ops as T

    g = _g("resample", shape)
    x = torch.randn(shape, generator=g)
    big = torch.randn(shape[:2] + tuple(2 * e for e in shape[2:]), generator=g)
    _bounds(device, dict(x=(x, True)), lambda t: T.upsample2(t["x"]))
    _bounds(device, dict(x=(x, True)), lambda t: T.zero_stuff2(t["x"]))
    _bounds(device, dict(x=(big, True)), lambda t: T.sumpool2(t["x"]))
    _bounds(device, dict(w=(x, True)), lambda t: T.conv_weight_rot180t(t["w"]))  # [Cout, Cin, k, k(, k)] of any extents
    src, dst = torch.randn(shape, generator=g), torch.randn((shape[0], shape[1] + 3) + shape[2:], generator=g)
    _bounds(device, dict(src=(src, True), dst=(dst, False)), lambda t: T.chan_copy(t["src"], t["dst"], shape[1] - 1, 1, 2, accumulate=True)
            if shape[1] > 1 else T.chan_copy(t["src"], t["dst"], 1, 0, 3))


# ---- 6b. scratch one float too small: the documented fall-backs, guards intact ---------------------------------------------------

@contextlib.contextmanager
def _one_float_less(name):
    """The size function `name` answers one float less than it needs: the wrapper then allocates and hands over a scratch that
    is one float too small (an arena view of exactly that size in the arena runs)."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    real = getattr(lib, name)
    setattr(lib, name, lambda *a: max(real(*a) - 1, 0))
    try:
        yield
    finally:
        setattr(lib, name, real)


def _rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_gemm_with_a_scratch_one_float_too_small_runs_its_k_slices_in_turn(device):
    """ddpm_gemm_desc.scratch: "NULL / too small: the same K slices run as one launch each".  Guards intact, the too-small scratch
    untouched, the same bits in all three runs, and the family's bound: 2e-6 of max |C| against float64, tests/test_gpu_train_ops.py::
    test_gemm_plain_and_transposed_operands.  (Finding 1 of DESIGN 4.0: the fall-back used to walk all 4 096 products of an
    element as ONE fp32 accumulation chain and measured 2.553e-06 here.)"""
    from ddpm_ood_amd import train_ops as T

    M, N, K = 128, 192, 4096
    g = _g("gemm", M, N, K)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    ref = A.double() @ B.double()

    def call(t):
        with _one_float_less("ddpm_gemm_scratch_floats"):
            Cm = T.torch.empty(M, N, dtype=torch.float32, device=device)
            return T.gemm(t["A"], t["B"], Cm, M, N, K, a_m=K, a_k=1, b_k=N, b_n=1, c_m=N, c_n=1)

    _, p = _bounds(device, dict(A=(A, True), B=(B, True)), call)
    gd = [a for a in p.allocated if a.numel() != M * N]
    assert len(gd) == 1 and gd[0].numel() > 0  # the too-small scratch was really handed over ...
    assert bool((gd[0].view(torch.int32) == POISON).all())  # ... and not used
    e = _rel(p.res[0], ref)
    print(f"bounds[gemm] too-small scratch: err {e:.3e} bound 2.000e-06")
    assert e < 2e-6, e

    def call2(t):  # alpha / beta: C is read by the first slice only
        with _one_float_less("ddpm_gemm_scratch_floats"):
            return T.gemm(t["A"], t["B"], t["C"], M, N, K, a_m=K, a_k=1, b_k=N, b_n=1, c_m=N, c_n=1, alpha=0.5, beta=2.0)

    _, p = _bounds(device, dict(A=(A, True), B=(B, True), C=(C0, False)), call2)
    e = _rel(p.res[0], 0.5 * ref + 2.0 * C0.double())
    print(f"bounds[gemm] too-small scratch, alpha / beta: err {e:.3e} bound 2.000e-06")
    assert e < 2e-6, e


@pytest.mark.parametrize("case", [(3, 192, 64, 16, 16, 3, 1), (3, 64, 64, 12, 12, 3, 1), (3, 64, 128, 16, 16, 3, 2)])
def test_conv_wgrad_with_a_scratch_one_float_too_small(device, case):
    """Too small for the matrix-pipe form: ddpm_conv_wgrad_f32 falls to the generic form.  Bound: 3e-6 relative to the gradient's
    largest element against float64 autograd, tests/test_gpu_train_ops.py::test_conv_wgrad_vs_autograd."""
    from ddpm_ood_amd import train_ops as T

    B, cin, cout, H, W, k, s = case
    g = _g("wgrad", case)
    a = torch.randn(B, cin, H, W, generator=g)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.double(), w, stride=s, padding=k // 2)
    dy = torch.randn(y.shape, generator=g)
    (ref,) = torch.autograd.grad(y, w, dy.double())

    def call(t):
        with _one_float_less("ddpm_conv_wgrad_scratch_floats"):
            return T.conv_wgrad(t["a"], t["dy"], k, s)

    _, p = _bounds(device, dict(a=(a, True), dy=(dy, True)), call)
    assert len(p.allocated) == 2 and _rel(p.res[0], ref) < 3e-6, _rel(p.res[0], ref)


def test_wgrad_forms_that_require_their_scratch_refuse_one_float_less(device):
    """conv3d_wgrad and the matrix-pipe form of conv_k4s2_wgrad need their scratch: one float less is refused before a launch, and
    nothing in the arena is touched."""
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd import train_ops as T

    lib = _lib.load()
    g = _g("refuse")
    for fn, size_fn, a, dy in (
            (lambda t: T.conv3d_wgrad(t["a"], t["dy"], 1), "ddpm_conv3d_wgrad_scratch_floats",
             torch.randn(2, 64, 4, 4, 4, generator=g), torch.randn(2, 64, 4, 4, 4, generator=g)),
            (lambda t: T.conv_k4s2_wgrad(t["a"], t["dy"]), "ddpm_conv_k4s2_wgrad_scratch_floats",
             torch.randn(3, 64, 12, 20, generator=g), torch.randn(3, 64, 6, 10, generator=g))):
        plain = _run(device, dict(a=(a, True), dy=(dy, True)), fn)
        arena = Arena(device, need_bytes([_nbytes(a), _nbytes(dy)] + plain.sizes))
        t = dict(a=arena.alloc(a.shape, a.dtype, fill=a, name="a", input_only=True), dy=arena.alloc(dy.shape, dy.dtype, fill=dy, name="dy", input_only=True))
        arena.freeze()
        with arena_allocations(_mods(), arena) as got, pointers_in_arena(lib, _lib.SIGNATURES, arena), _one_float_less(size_fn):
            with pytest.raises(ValueError, match="scratch"):
                fn(t)
        arena.check()
        dw = got.allocated[0]
        assert bool((dw.view(torch.int32) == 0x7FC0DEAD).all())  # the output is still poison: nothing ran


@pytest.mark.parametrize("B,heads,N,fa", [(3, 1, 64, True), (1, 1, 1024, False)])
def test_attention_with_a_scratch_one_float_too_small_is_the_plain_kernel(device, monkeypatch, B, heads, N, fa):
    """ddpm_attention_ws_f32 wants "at least ddpm_attention_scratch_floats": with one float less it has to run exactly
    ddpm_attention_f32 (bitwise) and leave the too-small scratch alone."""
    from ddpm_ood_amd import _lib, ops

    if fa:
        monkeypatch.setenv("DDPM_ATTN_FA", "2")
    lib = _lib.load()
    inputs, scale = _attention_operands(B, heads, N, True)
    Cc = 256 * heads

    def call(t):
        n = lib.ddpm_attention_scratch_floats(B, Cc, N, heads) - 1
        assert n > 0
        out = ops.torch.empty((B, Cc, N), dtype=torch.float32, device=device)
        scratch = ops.torch.empty(n, dtype=torch.float32, device=device)
        ops.check(lib.ddpm_attention_ws_f32(ops.ptr(t["qkv"]), ops.ptr(t["res"]), ops.ptr(out), B, Cc, N, heads, scale, ops.ptr(scratch), n,
                                            ops.stream_ptr()), "attention")
        return out

    _, p = _bounds(device, inputs, call)
    assert bool((p.allocated[1].view(torch.int32) == 0x7FC0DEAD).all())  # the scratch was not used: still poison
    y = ops.attention(inputs["qkv"][0].to(device), inputs["res"][0].to(device), heads, scale, use_scratch=False)
    _same_bits(p.res[:1], [y], "attention with a too-small scratch vs ddpm_attention_f32")
    y_fa = ops.attention(inputs["qkv"][0].to(device), inputs["res"][0].to(device), heads, scale, use_scratch=True)
    assert not torch.equal(y, y_fa)  # (with the full scratch the register-resident kernel runs: other bits)


def test_every_size_function_is_asked_by_a_case():
    """Every size function of the C ABI is named in the source of the case (or helper) of this file that asks it and checks the
    buffer against its answer -- through size_fns of _bounds, or by an assertion of its own."""
    import ctypes as C
    import inspect

    from ddpm_ood_amd._lib import SIGNATURES

    asked = {
        "ddpm_conv_scratch_floats": "test_conv2d_stays_inside_its_buffers", "ddpm_conv_kernel_scratch_floats": "_conv_spy",
        "ddpm_conv_stats_parts": "test_conv2d_stays_inside_its_buffers", "ddpm_attention_scratch_floats": "test_attention_with_scratch_stays_inside_its_buffers",
        "ddpm_gemm_scratch_floats": "test_gemm_stays_inside_its_buffers", "ddpm_conv_wgrad_scratch_floats": "test_conv_wgrad_stays_inside_its_buffers",
        "ddpm_conv3d_wgrad_scratch_floats": "test_conv3d_wgrad_stays_inside_its_buffers",
        "ddpm_conv_k4s2_wgrad_scratch_floats": "test_conv_k4s2_wgrad_stays_inside_its_buffers", "ddpm_vq_train_partials": "test_quantiser_stays_inside_its_buffers",
        "ddpm_spectral_partials": "test_spectral_amp_grad_stays_inside_its_buffers",
        "ddpm_unet_workspace_bytes": "_unet_case", "ddpm_unet_workspace_bytes3d": "_unet_case", "ddpm_unet_param_blob_floats": "_unets",
        **{fn: "_packers" for _, fn, _, _ in _packers().values() if fn},
    }
    sized = {n for n, (res, _) in SIGNATURES.items() if res is C.c_size_t} | {"ddpm_conv_stats_parts"}
    assert sized == set(asked), sized ^ set(asked)
    for fn, where in asked.items():
        assert fn in inspect.getsource(globals()[where]), (fn, where)


# ---- 7. quantiser ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,K", [(2, 32, 27, 64), (1, 3, 5, 7), (2, 64, 64, 256),
                                     (16, 8, 64, 16)])  # (the last: the quantiser call of test_trainer_parameter_gradients_of_the_total_loss)
def test_quantiser_stays_inside_its_buffers(device, B, D, S, K):
    """code_norms is exactly K floats and the partials exactly ddpm_vq_train_partials doubles (the wrappers' allocations)."""
    from ddpm_ood_amd import ops

    g = _g("vq", B, D, S, K)
    x, e = torch.randn(B, D, S, generator=g), torch.randn(K, D, generator=g)
    _, p = _bounds(device, dict(x=(x, True), e=(e, True)), lambda t: ops.vq_nearest(t["x"], t["e"]))
    assert sorted(a.numel() for a in p.allocated) == sorted([B * S, B * D * S, K])
    _, p = _bounds(device, dict(x=(x, True), e=(e, True)), lambda t: ops.vq_train_assign(t["x"], t["e"], 0.25)[:5],
                   size_fns=("ddpm_vq_train_partials",))
    assert K in [a.numel() for a in p.allocated]
    idx, _, counts, dw, _ = p.res
    cs, emaw = torch.rand(K, generator=g) * 3, torch.randn(K, D, generator=g)
    _bounds(device, dict(cs=(cs, False), emaw=(emaw, False), e=(e, False), counts=(counts.cpu(), True), dw=(dw.cpu(), True)),
            lambda t: (ops.vq_train_update(t["cs"], t["emaw"], t["e"], t["counts"], t["dw"], 0.99, 1e-5), t["cs"], t["emaw"], t["e"])[1:])
    dout, dloss = torch.randn(B, D, S, generator=g), torch.randn((), generator=g)
    _bounds(device, dict(dout=(dout, True), x=(x, True), e=(e, True), idx=(idx.cpu(), True), dloss=(dloss, True)),
            lambda t: ops.vq_train_backward(t["dout"], t["x"], t["e"], t["idx"], t["dloss"], 0.25))
    _bounds(device, dict(x=(x, True), e=(e, True), idx=(idx.cpu(), True)), lambda t: ops.vq_train_backward(None, t["x"], t["e"], t["idx"], None, 0.25))


# ---- 8. loss terms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(5, 1, 3, 32, 32, 64, 11, 4, 2, True), (3, 3, 3, 35, 27, 64, 11, 4, 2, True), (4, 64, 64, 7, 7, 192, 5, 1, 2, False),
                                  (2, 10, 10, 5, 6, 7, 3, 1, 1, False)])
def test_lpips_conv_stays_inside_its_buffers(device, case):
    from ddpm_ood_amd import ops

    N, Cx, Cin, H, W, Cout, k, stride, pad, affine = case
    g = _g("lpips_conv", case)
    x = torch.rand(N, Cx, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    a = torch.rand(Cin, generator=g) + 0.5 if affine else None
    s = torch.randn(Cin, generator=g) if affine else None
    _, p = _bounds(device, dict(x=(x, True), w=(w, True), b=(b, True), a=(a, True), s=(s, True)),
                   lambda t: ops.lpips_conv(t["x"], t["w"], t["b"], stride, pad, True, t.get("a"), t.get("s")))
    Ho, Wo = p.res[0].shape[2:]
    bm = torch.randn(Cout, Ho, Wo, generator=g)
    xf = x.expand(N, Cin, H, W).contiguous()
    _bounds(device, dict(x=(xf, True), w=(w, True), bm=(bm, True)), lambda t: ops.lpips_conv_biasmap(t["x"], t["w"], t["bm"], stride, pad, True))
    if Cin == 3:  # the first layer's input gradient, through the broadcast and as RGB
        gout = torch.randn(N, Cout, Ho, Wo, generator=g)
        _bounds(device, dict(g=(gout, True), w=(w, True), a=(a, True)),
                lambda t: ops.lpips_conv1_dgrad(t["g"], t["w"], Cx, H, W, stride, pad, in_scale=t.get("a")))


def test_lpips_conv1_dgrad_on_an_odd_image_stays_inside_its_buffers(device):
    from ddpm_ood_amd import ops

    N, H, W, Cout, k, stride, pad = 1, 34, 33, 64, 11, 4, 2
    g = _g("dgrad")
    w = torch.randn(Cout, 3, k, k, generator=g) / 19
    gout = torch.randn(N, Cout, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, generator=g)
    a = torch.rand(3, generator=g) + 0.5
    for cx in (1, 3):
        _bounds(device, dict(g=(gout, True), w=(w, True), a=(a, True)),
                lambda t: ops.lpips_conv1_dgrad(t["g"], t["w"], cx, H, W, stride, pad, in_scale=t["a"]))  # noqa: B023


@pytest.mark.parametrize("case", [(3, 64, 15, 11, 192, 5), (2, 8, 9, 9, 32, 3)])
def test_lpips_conv_mfma_stays_inside_its_buffers(device, case):
    from ddpm_ood_amd import ops

    N, Cin, H, W, Cout, k = case
    assert ops.lpips_conv_mfma_supported(Cin, H, W, Cout, k)
    g = _g("lpips_mfma", case)
    x = torch.rand(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    packed = ops.lpips_pack_conv_weight(w.to(device)).cpu()
    for relu in (False, True):
        _bounds(device, dict(x=(x, True), packed=(packed, True), b=(b, True)),
                lambda t: ops.lpips_conv_mfma(t["x"], t["packed"], t["b"], Cout, k, relu=relu))  # noqa: B023


@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (3, 4, 15, 15), (1, 2, 3, 3)])
def test_maxpool_and_its_backward_stay_inside_their_buffers(device, shape):
    from ddpm_ood_amd import ops

    g = _g("maxpool", shape)
    x = torch.randn(shape, generator=g)
    _, p = _bounds(device, dict(x=(x, True)), lambda t: ops.maxpool3s2(t["x"]))
    dy = torch.randn(p.res[0].shape, generator=g)
    _bounds(device, dict(x=(x, True), dy=(dy, True)), lambda t: ops.maxpool3s2_backward(t["x"], t["dy"], relu_mask=True))
    _bounds(device, dict(x=(x, True), dy=(dy, True), acc=(torch.randn(shape, generator=g), False)),
            lambda t: ops.maxpool3s2_backward(t["x"], t["dy"], out=t["acc"]))


@pytest.mark.parametrize("C,H,W", [(64, 7, 9), (256, 1, 1)])
def test_lpips_layer_and_its_backward_stay_inside_their_buffers(device, C, H, W):
    from ddpm_ood_amd import ops

    N = 3
    g = _g("lpips_layer", C, H, W)
    f0, f1 = torch.rand(N, C, H, W, generator=g), torch.rand(N, C, H, W, generator=g)
    f0[1] = 0  # an all-zero feature vector: the 1e-10 guard
    lin, up = torch.rand(C, generator=g) / C, torch.randn(N, generator=g)
    feats = dict(f0=(f0, True), f1=(f1, True), lin=(lin, True))
    _bounds(device, feats, lambda t: ops.lpips_layer(t["f0"], t["f1"], t["lin"]))
    _bounds(device, dict(acc=(torch.rand(N, generator=g), False), **feats), lambda t: ops.lpips_layer(t["f0"], t["f1"], t["lin"], t["acc"]))
    _bounds(device, dict(up=(up, True), **feats), lambda t: ops.lpips_layer_backward(t["f0"], t["f1"], t["lin"], t["up"]))
    _bounds(device, dict(up=(up, True), acc=(torch.randn(N, C, H, W, generator=g), False), **feats),
            lambda t: ops.lpips_layer_backward(t["f0"], t["f1"], t["lin"], t["up"], out=t["acc"], relu_mask=False))


@pytest.mark.parametrize("n", [1, 255, 300000])
def test_spectral_amp_grad_stays_inside_its_buffers(device, n):
    """n = 300 000 > 1024 * 256: the grid-stride loop wraps; the partials are exactly ddpm_spectral_partials(n) doubles."""
    from ddpm_ood_amd import train_ops as T

    g = _g("spectral", n)
    r, x = torch.randn(2, n, generator=g), torch.randn(2, n, generator=g)
    r[:, 0] = 0  # |R| = 0: the gradient is 0 there
    dloss = torch.tensor([0.7])
    _bounds(device, dict(r=(r, True), x=(x, True), dloss=(dloss, True)),
            lambda t: T.spectral_amp_grad(t["r"], t["x"], t["dloss"], want_loss=True, want_grad=True), size_fns=("ddpm_spectral_partials",))
    _bounds(device, dict(r=(r, True), x=(x, True)), lambda t: T.spectral_amp_grad(t["r"], t["x"], None, want_loss=True)[:1],
            size_fns=("ddpm_spectral_partials",))
    _bounds(device, dict(r=(r, True), x=(x, True), dloss=(dloss, True)),
            lambda t: T.spectral_amp_grad(t["r"], t["x"], t["dloss"], want_loss=False, want_grad=True)[1:])


# ---- 9. the UNet engine: every layer's scratch carved out of one workspace -------------------------------------------------------

_UNETS = {}


def _unets(device, spatial_dims, channels):
    """(ordinary model, guarded model, the arena holding the guarded model's parameter blob -- frozen)."""
    from ddpm_ood_amd import DiffusionModelUNet, _lib
    from ddpm_ood_amd import unet as unet_mod
    from ddpm_ood_amd.synthetic import random_state_dict
    from test_gpu_unet import SMALL

    key = (spatial_dims, channels)
    if key not in _UNETS:
        sd = random_state_dict(channels=channels, seed=1, config=SMALL, spatial_dims=spatial_dims)
        models = []
        for _ in range(2):
            m = DiffusionModelUNet(spatial_dims, channels, channels, **SMALL)
            m.load_state_dict(sd)
            models.append(m.to(device).eval())
        plain, guarded = models
        with arena_allocations([unet_mod]) as rec:
            plain._sync(device)
        blob_arena = Arena(device, need_bytes(rec.sizes))
        with arena_allocations([unet_mod], blob_arena) as got:
            guarded._sync(device)
        (blob,) = got.allocated
        assert guarded._blob is blob and rec.sizes == [4 * blob.numel()]
        assert blob.numel() == _lib.load().ddpm_unet_param_blob_floats(guarded._engine)  # exactly the advertised size
        blob_arena.view_of(blob).input_only = True
        blob_arena.freeze()
        blob_arena.check()
        _UNETS[key] = (plain, guarded, blob_arena)
    return _UNETS[key]


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """Frees this file's cached UNets and hands the caching allocator's blocks back to the driver when the file is done.
    It is here because of an OPEN fault (finding 2): the one whole-suite run made with this file present, and
    without this fixture, ended in `HIP error: an illegal memory access was encountered` in tests/test_gpu_vqvae_loss_terms.py::
    test_trainer_parameter_gradients_of_the_total_loss, ten minutes after this file had finished in the same process.  That test
    runs none of this file's code; the cause is not found.  The fixture only keeps this file's several GB of freed arenas out of
    the allocator state the later files run in -- it explains nothing, and if the fault is an access past a buffer that the old
    layout happened to forgive, it is still there."""
    yield
    import gc

    _UNETS.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


UNET_CASES = [(2, 1, 1, (16, 16)), (2, 1, 3, (16, 16)), (2, 1, 1, (12, 20)), (2, 1, 3, (12, 20)), (3, 128, 1, (4, 8, 16))]


@pytest.mark.parametrize("d3s", ["0", "2"])
@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("sd,channels,B,ext", UNET_CASES, ids=[f"{c[0]}d-B{c[2]}-{'x'.join(map(str, c[3]))}" for c in UNET_CASES])
def test_unet_forward_stays_inside_a_workspace_of_exactly_the_advertised_size(device, monkeypatch, sd, channels, B, ext, fused, d3s):
    """The SMALL configuration of tests/test_gpu_unet.py with input, timesteps, output, parameter blob and a workspace of exactly
    ddpm_unet_workspace_bytes / ...bytes3d in arenas: poisoned and zero-filled workspaces give the ordinary call's bits."""
    with _stop_on_gpu_fault():
        _unet_case(device, monkeypatch, sd, channels, B, ext, fused, d3s)


def _unet_case(device, monkeypatch, sd, channels, B, ext, fused, d3s):
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd import unet as unet_mod

    monkeypatch.setenv("DDPM_GN_FUSED", fused)
    monkeypatch.setenv("DDPM_CONV_D3S", d3s)
    lib = _lib.load()
    plain, guarded, blob_arena = _unets(device, sd, channels)
    g = _g("unet", sd, B, ext)
    x = torch.randn((B, channels) + ext, generator=g)
    t = torch.tensor([650, 30, 990][:B], dtype=torch.int64)
    D, H, W = ((1,) + ext) if sd == 2 else ext
    need = lib.ddpm_unet_workspace_bytes3d(guarded._engine, B, D, H, W)
    assert need > 0
    if sd == 2:
        assert lib.ddpm_unet_workspace_bytes(guarded._engine, B, H, W) == need
    plain._workspace = None
    want = plain(x.to(device), t.to(device))
    torch.cuda.synchronize()
    assert plain._workspace.numel() == need
    outs = []
    for zero in (False, True):
        arena = Arena(device, need_bytes([_nbytes(x), _nbytes(t), need, _nbytes(want)]))
        xa = arena.alloc(x.shape, x.dtype, fill=x, name="x", input_only=True)
        ta = arena.alloc(t.shape, t.dtype, fill=t, name="timesteps", input_only=True)
        ws = arena.alloc((need,), torch.uint8, name="workspace")
        if zero:
            ws.zero_()
        arena.freeze()
        guarded._workspace = ws
        with arena_allocations([unet_mod], arena, zero) as got:
            y = guarded(xa, ta)
        assert guarded._workspace is ws and len(got.allocated) == 1 and got.allocated[0] is y  # the output; no new workspace, no new blob
        assert all(a.contains(p.data_ptr()) for a, p in ((arena, xa), (arena, ta), (arena, ws), (arena, y), (blob_arena, guarded._blob)))
        arena.check()
        blob_arena.check()
        guarded._workspace = None
        outs.append(y.clone())
    _all_finite(outs, "UNet forward in the arena")
    _same_bits([want], outs[:1], "UNet: ordinary vs poisoned workspace")
    _same_bits(outs[:1], outs[1:], "UNet: poisoned vs zeroed workspace")
