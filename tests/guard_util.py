"""An arena with guard bands: did a kernel write anywhere else, read memory it was never handed, or depend on what an
uninitialised buffer happened to hold?

``Arena(device, nbytes)`` is ONE buffer filled with a poison word, the quiet NaN 0x7FC0DEAD (compared as int32, never as float:
NaN != NaN).  ``alloc`` carves contiguous views out of it: the start 256-byte aligned (what the dispatchers' alignment tests see
from the caching allocator), the guard beginning at the first byte after the view's last element, at least 64 KiB of poison
between two views and at least 1 MiB behind the last one.  A view is either filled from a CPU tensor or left poisoned (outputs,
scratch, partials, statistics slabs); views marked ``input_only`` are snapshot by ``freeze`` and must come back bit-identical.
``check`` synchronises and asserts that every guard word still holds the poison and every frozen input its snapshot; a failure
names the neighbouring view, the byte offset from that view's edge and the number of words that changed (GuardViolation.findings).

An overrun longer than a guard lands in the next view, which is verified too (a frozen input bitwise, an output by the test's
comparison with the ordinary call); every access a kernel makes within 1 MiB of its last buffer stays inside the one allocation.

``ArenaTorch`` / ``arena_allocations`` put the buffers a wrapper allocates ITSELF into the arena: the wrappers of ops.py /
train_ops.py size every output, scratch and partials buffer by the library's size functions and take it from ``torch.empty``; with
the module's ``torch`` name replaced by an ArenaTorch those calls return poisoned (or zero-filled) arena views of exactly the
requested size, so the wrapper's own call of the C ABI runs with every pointer inside the arena.  ``pointers_in_arena`` wraps the
library's entry points and asserts exactly that for each call.
"""

from __future__ import annotations

import contextlib
import ctypes

import torch

POISON = 0x7FC0DEAD  # quiet NaN with a recognisable payload
ALIGN = 256
GUARD = 64 << 10
TAIL_GUARD = 1 << 20
_POISON_BYTES = tuple(POISON.to_bytes(4, "little"))


class GuardViolation(AssertionError):
    """findings: dicts {view, side ('before' | 'after' | 'input'), offset, words}.  offset: bytes from the view's edge to the
    nearest change -- 'after': to the first changed byte, 0 is the byte right behind the last element; 'before': back to the first
    byte of the nearest changed word, 4 is the word right in front of the first element; 'input': the byte offset of the first changed word inside the view."""

    def __init__(self, findings):
        self.findings = findings
        super().__init__("; ".join(
            f"{f['words']} word(s) changed inside frozen input '{f['view']}', first at byte {f['offset']}" if f["side"] == "input" else
            f"{f['words']} guard word(s) changed {f['side']} view '{f['view']}', nearest {f['offset']} byte(s) "
            f"{'behind its end' if f['side'] == 'after' else 'in front of its start'}" for f in findings))


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes (flat uint8): bitwise comparisons that NaN payloads survive."""
    return t.contiguous().reshape(-1).view(torch.uint8)


def need_bytes(sizes) -> int:
    """Arena size that holds views of these byte sizes."""
    return sum(int(s) + GUARD + ALIGN for s in sizes) + TAIL_GUARD + 2 * ALIGN


class _View:
    def __init__(self, name, start, nbytes, tensor, input_only):
        self.name, self.start, self.end, self.tensor, self.input_only = name, start, start + nbytes, tensor, input_only
        self.snapshot = None


class Arena:
    def __init__(self, device, nbytes: int):
        nbytes = (int(nbytes) + 3) & ~3
        words = torch.full((nbytes // 4,), POISON, dtype=torch.int32, device=device)
        self.base = words.view(torch.uint8)  # the one allocation; tests tamper through it
        self.device = self.base.device
        self.nbytes = nbytes
        self.views = []
        assert self.base.data_ptr() % 4 == 0
        self._pattern = torch.tensor(_POISON_BYTES * 2, dtype=torch.uint8, device=device)

    # ---- carving ----------------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype=torch.float32, fill=None, *, name=None, input_only=False) -> torch.Tensor:
        """A contiguous view of `shape`; fill=None leaves it poisoned, else the CPU tensor `fill` is copied in."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        cursor = self.views[-1].end if self.views else 0
        p0 = self.base.data_ptr()
        start = ((p0 + cursor + GUARD + ALIGN - 1) // ALIGN) * ALIGN - p0
        if start + nbytes + TAIL_GUARD > self.nbytes:
            raise MemoryError(f"arena of {self.nbytes} bytes cannot hold a view of {nbytes} bytes at {start} plus its 1 MiB tail guard")
        t = self.base[start:start + nbytes].view(dtype).view(shape)
        if fill is not None:
            fill = torch.as_tensor(fill)
            assert tuple(fill.shape) == shape and fill.dtype == dtype, (fill.shape, fill.dtype, shape, dtype)
            t.copy_(fill)
        v = _View(name or f"view{len(self.views)}", start, nbytes, t, input_only)
        self.views.append(v)
        assert t.data_ptr() % ALIGN == 0 and t.is_contiguous()
        return t

    def contains(self, ptr: int) -> bool:
        return self.base.data_ptr() <= ptr < self.base.data_ptr() + self.nbytes

    def view_of(self, t: torch.Tensor):
        for v in self.views:
            if v.tensor.data_ptr() == t.data_ptr() and v.end - v.start == t.numel() * t.element_size():
                return v
        raise KeyError("not a view of this arena")

    def freeze(self) -> None:
        """Bitwise snapshot of every input-only view."""
        for v in self.views:
            if v.input_only:
                v.snapshot = self.base[v.start:v.end].clone()

    # ---- verification -----------------------------------------------------------------------------------------------------
    def _changed(self, g0: int, g1: int) -> torch.Tensor:
        """Sorted arena byte offsets in [g0, g1) of the changed guard words (a ragged head / tail: of the changed bytes)."""
        a0 = min((g0 + 3) & ~3, g1)
        a1 = max(g1 & ~3, a0)
        out = []
        for b0, b1 in ((g0, a0), (a1, g1)):  # bytes next to a view whose size is no multiple of 4
            if b1 > b0:
                want = self._pattern[b0 % 4:b0 % 4 + (b1 - b0)]
                out.append(b0 + torch.nonzero(self.base[b0:b1] != want).reshape(-1))
        if a1 > a0:
            bad = torch.nonzero(self.base[a0:a1].view(torch.int32) != POISON).reshape(-1)
            out.append(a0 + 4 * bad)
        return torch.sort(torch.cat(out)).values.cpu() if out else torch.empty(0, dtype=torch.int64)

    def check(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        findings = []
        edges = [(None, 0)] + [(v, v.end) for v in self.views]
        nexts = [(v, v.start) for v in self.views] + [(None, self.nbytes)]
        for (prev, g0), (nxt, g1) in zip(edges, nexts):
            bad = self._changed(g0, g1)
            if bad.numel() == 0:
                continue
            # a changed word belongs to the nearer view (the first guard has only a following view, the last only a preceding one)
            mid = g1 if nxt is None else g0 if prev is None else (g0 + g1) // 2
            lo, hi = bad[bad < mid], bad[bad >= mid]
            if lo.numel():
                findings.append(dict(view=prev.name, side="after", offset=int(lo[0]) - prev.end, words=int(torch.unique(lo // 4).numel())))
            if hi.numel():
                findings.append(dict(view=nxt.name, side="before", offset=nxt.start - int(hi[-1]), words=int(torch.unique(hi // 4).numel())))
        for v in self.views:
            if v.snapshot is not None:
                diff = torch.nonzero(self.base[v.start:v.end] != v.snapshot).reshape(-1).cpu()
                if diff.numel():
                    findings.append(dict(view=v.name, side="input", offset=int(diff[0]) // 4 * 4, words=int(torch.unique(diff // 4).numel())))
        if findings:
            raise GuardViolation(findings)


# ---- the wrappers' own allocations, taken from an arena ----------------------------------------------------------------------

class ArenaTorch:
    """Stands in for the ``torch`` name of a wrapper module: empty / empty_like / zeros / zeros_like come out of `arena`
    (poisoned, or zero-filled with zero_fill=True; zeros always zero-filled), everything else is torch's.  arena=None only records:
    the calls go to torch, and ``sizes`` lists the bytes of each -- what an arena for the same call has to hold."""

    def __init__(self, arena=None, zero_fill=False):
        self._arena, self._zero_fill = arena, zero_fill
        self.sizes, self.allocated = [], []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device, zero):
        dtype = dtype or torch.float32
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        self.sizes.append(numel * torch.empty((), dtype=dtype).element_size())
        if self._arena is None:
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
        assert torch.device(device).type == self._arena.device.type
        t = self._arena.alloc(shape, dtype, name=f"alloc{len(self.allocated)}{list(shape)}")
        if zero or self._zero_fill:
            t.zero_()
        self.allocated.append(t)
        return t

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size

    def empty(self, *size, dtype=None, device=None):
        return self._alloc(self._shape(size), dtype, device, False)

    def zeros(self, *size, dtype=None, device=None):
        return self._alloc(self._shape(size), dtype, device, True)

    def empty_like(self, t, dtype=None):
        return self._alloc(t.shape, dtype or t.dtype, t.device, False)

    def zeros_like(self, t, dtype=None):
        return self._alloc(t.shape, dtype or t.dtype, t.device, True)


@contextlib.contextmanager
def arena_allocations(modules, arena=None, zero_fill=False):
    """Within the block, `modules` (ops, train_ops, ...) allocate through an ArenaTorch (yielded)."""
    proxy = ArenaTorch(arena, zero_fill)
    saved = [m.torch for m in modules]
    for m in modules:
        m.torch = proxy
    try:
        yield proxy
    finally:
        for m, t in zip(modules, saved):
            m.torch = t


def _struct_pointers(s):
    return [(f[0], getattr(s, f[0])) for f in s._fields_ if f[1] is ctypes.c_void_p]


@contextlib.contextmanager
def pointers_in_arena(lib, signatures, arena, skip=()):
    """Within the block every entry point of `lib` is logged -- yields the list of (name, return value) -- and those that take
    device pointers (two or more void * arguments, the last being the stream; the void * fields of a descriptor passed by
    reference) assert that each non-null one lies inside `arena`.  `skip`: entry points whose void * arguments are no device
    buffers (engine handles)."""
    called, saved = [], {}

    def wrap(name, real, argtypes):
        takes_desc = any(isinstance(a, type) and issubclass(a, ctypes._Pointer) and issubclass(a._type_, ctypes.Structure)
                         for a in argtypes)
        where = [i for i, a in enumerate(argtypes) if a is ctypes.c_void_p][:-1]
        if name in skip or not (takes_desc or len(where) >= 1):
            where, takes_desc = [], False

        def fn(*args):
            ptrs = [(f"argument {i}", args[i]) for i in where]
            if takes_desc:
                for a in args:
                    obj = getattr(a, "_obj", None)  # ctypes.byref(descriptor)
                    if isinstance(obj, ctypes.Structure):
                        ptrs += _struct_pointers(obj)
            for what, p in ptrs:
                p = getattr(p, "value", p)
                assert not p or arena.contains(int(p)), f"{name}: {what} = {int(p):#x} is outside the arena"
            ret = real(*args)
            called.append((name, ret))
            return ret

        return fn

    for name, (_, argtypes) in signatures.items():
        saved[name] = getattr(lib, name)
        setattr(lib, name, wrap(name, saved[name], argtypes))
    try:
        yield called
    finally:
        for name, real in saved.items():
            setattr(lib, name, real)
