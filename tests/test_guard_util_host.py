"""The guard-band arena of tests/guard_util.py on CPU tensors: the detector has to be able to fail, and to say where."""

import pytest
import torch

from guard_util import ALIGN, GUARD, POISON, TAIL_GUARD, Arena, ArenaTorch, GuardViolation, arena_allocations, bits, need_bytes

SHAPES = [((3, 5), torch.float32), ((7,), torch.float16), ((2, 3), torch.int64), ((5,), torch.uint8), ((0,), torch.float32),
          ((1,), torch.float32)]


def _arena():
    sizes = [torch.empty(s, dtype=d).numel() * torch.empty((), dtype=d).element_size() for s, d in SHAPES]
    a = Arena("cpu", need_bytes(sizes + [16]))  # room for one more small view
    views = []
    for i, (s, d) in enumerate(SHAPES):
        fill = None if i % 2 else (torch.arange(torch.empty(s).numel()).reshape(s) + 1).to(d)
        views.append(a.alloc(s, d, fill=fill, name=f"v{i}", input_only=fill is not None))
    a.freeze()
    return a, views


def _words(a, b0, b1):
    return a.base[b0:b1].view(torch.int32)


def test_views_are_aligned_and_guards_start_at_the_last_element():
    a, views = _arena()
    p0 = a.base.data_ptr()
    for t, v, (s, d) in zip(views, a.views, SHAPES):
        assert t.data_ptr() % ALIGN == 0 and t.is_contiguous() and tuple(t.shape) == s and t.dtype == d
        assert t.numel() == 0 or v.start == t.data_ptr() - p0  # (an empty tensor has no address)
        assert (p0 + v.start) % ALIGN == 0 and v.end == v.start + t.numel() * t.element_size()  # no rounding up of the end
    # at least 64 KiB of poison in front of every view, 1 MiB behind the last; nothing but poison outside the views
    edges = [0] + [v.end for v in a.views]
    for g0, v in zip(edges, a.views):
        assert v.start - g0 >= GUARD
    assert a.nbytes - a.views[-1].end >= TAIL_GUARD
    covered = torch.zeros(a.nbytes, dtype=torch.bool)
    for v in a.views:
        covered[v.start:v.end] = True
    pattern = torch.tensor(list(POISON.to_bytes(4, "little")), dtype=torch.uint8).repeat(a.nbytes // 4)
    assert torch.equal(a.base[~covered], pattern[~covered])
    # the byte right behind a 14-byte (7 x f16) and a 5-byte view is guard, the byte in front of each view too
    for v in a.views:
        assert not covered[v.end] and not covered[v.start - 1]
    with pytest.raises(MemoryError):
        a.alloc((1 << 20,), torch.float32)


def test_clean_run_passes_and_poison_round_trips_bit_exactly():
    a, views = _arena()
    a.check()
    out = views[1]  # poisoned f16 view: 3 whole poison words and a half
    assert bits(out).tolist() == (list(POISON.to_bytes(4, "little")) * 4)[:14]
    f = a.alloc((4,), torch.float32)
    assert torch.isnan(f).all() and f.view(torch.int32).tolist() == [POISON] * 4
    back = f.clone().cpu().numpy().view("int32").tolist()  # through a copy and numpy
    assert back == [POISON] * 4
    assert not (f == f).any()  # which is why the arena compares int32
    views[1].fill_(1.0)  # writing an output is no violation
    a.check()


@pytest.mark.parametrize("index", [0, 1, 2, 3, 5])
def test_write_one_element_outside_a_view_names_the_view_and_offset(index):
    es = torch.empty((), dtype=SHAPES[index][1]).element_size()
    a, views = _arena()
    v = a.views[index]
    a.base[v.end:v.end + es] = 0  # one element behind the view, through the base buffer
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view=f"v{index}", side="after", offset=0, words=(es + 3) // 4)], e.value.findings
    assert f"v{index}" in str(e.value) and "behind its end" in str(e.value)
    a, views = _arena()
    v = a.views[index]
    a.base[v.start - es:v.start] = 0  # one element in front of it
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view=f"v{index}", side="before", offset=4, words=(es + 3) // 4)], e.value.findings
    assert "in front of its start" in str(e.value)


def test_far_overrun_is_attributed_to_the_nearer_view_with_its_distance():
    a, _ = _arena()
    v0, v1 = a.views[0], a.views[1]
    _words(a, v0.end + 4096, v0.end + 4096 + 12)[:] = 0
    gap_end = v1.start - 256
    _words(a, gap_end, gap_end + 4)[:] = 7
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view="v0", side="after", offset=4096, words=3), dict(view="v1", side="before", offset=256, words=1)]
    # the arena's own head and tail guards
    b, _ = _arena()
    _words(b, 0, 4)[:] = 0
    _words(b, b.nbytes - 4, b.nbytes)[:] = 0
    with pytest.raises(GuardViolation) as e:
        b.check()
    assert [(f["view"], f["side"]) for f in e.value.findings] == [("v0", "before"), ("v5", "after")]
    assert e.value.findings[1]["offset"] == b.nbytes - 4 - b.views[-1].end


def test_modified_frozen_input_is_reported_and_nan_payload_changes_count():
    a, views = _arena()
    views[2][1, 2] += 1
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert e.value.findings == [dict(view="v2", side="input", offset=5 * 8, words=1)]
    # an input holding NaNs: same bits pass, another payload fails (a float comparison could tell neither)
    b = Arena("cpu", need_bytes([16]))
    x = b.alloc((4,), torch.float32, fill=torch.tensor([1.0, float("nan"), 2.0, float("nan")]), name="x", input_only=True)
    b.freeze()
    b.check()
    x.view(torch.int32)[3] = POISON
    with pytest.raises(GuardViolation) as e:
        b.check()
    assert e.value.findings == [dict(view="x", side="input", offset=12, words=1)]


def test_wrapper_allocations_come_out_of_the_arena():
    import types

    mod = types.SimpleNamespace(torch=torch)
    with arena_allocations([mod]) as rec:  # recording only
        t = mod.torch.empty((2, 3), dtype=torch.float16, device="cpu")
        mod.torch.zeros(5, dtype=torch.float32, device="cpu")
        mod.torch.empty_like(t)
        mod.torch.empty((), dtype=torch.float64, device="cpu")
    assert rec.sizes == [12, 20, 12, 8] and mod.torch is torch
    a = Arena("cpu", need_bytes(rec.sizes))
    with arena_allocations([mod], a) as got:
        e = mod.torch.empty((2, 3), dtype=torch.float16, device="cpu")
        z = mod.torch.zeros(5, dtype=torch.float32, device="cpu")
        assert mod.torch.float32 is torch.float32  # everything else is torch's
    assert all(a.contains(t.data_ptr()) for t in (e, z)) and len(got.allocated) == 2
    assert bits(e).tolist() == (list(POISON.to_bytes(4, "little")) * 3) and z.tolist() == [0.0] * 5
    a.view_of(e)
    with arena_allocations([mod], Arena("cpu", need_bytes(rec.sizes)), zero_fill=True):
        assert mod.torch.empty(3, dtype=torch.float32, device="cpu").tolist() == [0.0] * 3
    assert isinstance(ArenaTorch().Tensor, type)
