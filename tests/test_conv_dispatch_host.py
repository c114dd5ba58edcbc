"""CPU: the convolution selection table (csrc/conv_dispatch.hip) decides what the hand-written dispatcher before it decided.

tests/golden/conv_dispatch_parent.json holds, for a sweep of descriptors and switch settings, the four host-only answers of the
commit before the table existed (tools/record_conv_dispatch.py recorded them; its docstring says how): the family that
takes the descriptor, ddpm_conv_stats_parts, ddpm_conv_scratch_floats and ddpm_conv_takes_wino44h.  Pointers only matter for
NULL-ness and alignment and device_cus() answers 256 without a device, as on an MI355X: the answers are the GPU machine's.

The fixture's "parent_mirror_disagrees" is empty: on this sweep the parent's hand-written mirror (its conv_stats_parts) named
the family its if-chain launched everywhere, so every row has to match exactly.
"""

import ctypes as C
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("record_conv_dispatch", ROOT / "tools" / "record_conv_dispatch.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

# the rows of the two tables of csrc/conv_dispatch.hip, and those with a stats_parts function
PLANAR = ("linear_skinny", "d3s", "wino44h", "wino44", "wino", "d3s2", "s2h", "d1s", "conv1x1_dma", "mfma", "direct")
VOLUMETRIC = ("wino44h", "wino44", "wino", "mfma")
WRITES_STATS = ("d3s", "wino44h", "wino", "d3s2", "s2h", "direct")
# d3s and d3s2 only take square 8 / 16 / 32-wide outputs (d3s_geom, d3s2_take), for which their reduce pass always has a
# slicing (wino_split_reduce_stats_parts): no descriptor they take can answer 0
ALWAYS_WRITES = ("d3s", "d3s2")


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    if not _lib.lib_path().exists():
        import __graft_entry__ as g

        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fix():
    return json.loads(rec.FIXTURE.read_text())


def _rows(fix, name):
    return range(len(fix["descs"])) if name == "default" else fix["slice"]


def test_fixture_is_the_recorders_sweep(lib, fix):
    rows, sliced = rec.sweep(lib)
    assert fix["descs"] == rows and fix["slice"] == sliced and fix["settings"] == rec.SETTINGS
    assert rec.FIXTURE.stat().st_size < 256 * 1024
    assert fix["parent_mirror_disagrees"] == []


def test_same_answers_as_the_parent_commit(lib, fix):
    bad = []
    for s in fix["settings"]:
        with rec.setting(lib, s):
            for i, want in zip(_rows(fix, s["name"]), fix["answers"][s["name"]]):
                got = rec.ask(lib, fix["descs"][i])
                if got != want:
                    bad.append((s["name"], dict(zip(fix["fields"], fix["descs"][i])), {"parent": want, "now": got}))
    assert not bad, f"{len(bad)} descriptors changed their dispatch, e.g. {bad[:3]}"


def test_sweep_covers_every_row_and_both_statistics_answers(fix):
    sel, pos, zero = rec.coverage(fix)
    for table, names in (("2d", PLANAR), ("3d", VOLUMETRIC)):
        for n in names:
            assert sel.get((table, n), 0) >= 5, f"{table} row {n}: selected by {sel.get((table, n), 0)} descriptors"
    for n in WRITES_STATS:
        assert n in pos, f"{n} never answers stats parts > 0"
        assert n in zero or n in ALWAYS_WRITES, f"{n} never answers stats parts == 0"


def test_answers_are_consistent_with_the_selected_row(lib, fix):
    huge = C.c_size_t(-1).value
    for s in fix["settings"]:
        with rec.setting(lib, s):
            for i in _rows(fix, s["name"]):
                row = fix["descs"][i]
                name, parts, scratch, takes = rec.ask(lib, row)
                what = (s["name"], dict(zip(fix["fields"], row)))
                assert parts == 0 or name in WRITES_STATS, what
                d = rec.descriptor(row)
                d.scratch = None
                if row[0] & rec.P["scratch"] and scratch:
                    d.scratch, d.scratch_floats = 0x4000000, scratch
                assert scratch >= lib.ddpm_conv_kernel_scratch_floats(C.byref(d)), what
                if takes:  # the descriptor ddpm_conv_takes_wino44h asks about: w_wino44h given, scratch as large as needed
                    d.w_wino44h = d.w_wino44h or 0x5000000
                    if not d.scratch:
                        d.scratch, d.scratch_floats = 0x4000000, huge
                    assert lib.ddpm_conv_kernel_name(C.byref(d)) == b"wino44h", what


# (the last one: a threshold no launch reaches; a switch that used to be read once into a static)
_FAMILY_SWITCHES = [("DDPM_LINEAR_SKINNY", "0", "linear_skinny"), ("DDPM_CONV_WINOGRAD", "0", "wino"),
                    ("DDPM_CONV1X1_DMA", "0", "conv1x1_dma"), ("DDPM_CONV1X1_DMA_MIN_WG", "1000000000", "conv1x1_dma")]


@pytest.mark.parametrize("var,value,family", _FAMILY_SWITCHES, ids=[f"{v}-{f}" for v, _, f in _FAMILY_SWITCHES])
def test_family_switches_follow_reload_env(lib, fix, monkeypatch, var, value, family):
    default = fix["answers"]["default"]
    assert any(a[0] == family for a in default)
    monkeypatch.setenv(var, value)  # (conftest: a DDPM_* setenv reloads the switches)
    assert not any(rec.ask(lib, row)[0] == family for row in fix["descs"])
    monkeypatch.delenv(var)
    assert [rec.ask(lib, row) for row in fix["descs"]] == default


def test_kernel_name_of_a_null_or_invalid_descriptor_is_empty(lib):
    from ddpm_ood_amd._lib import ConvDesc

    assert lib.ddpm_conv_kernel_name(None) == b""
    assert lib.ddpm_conv_kernel_name(C.byref(ConvDesc())) == b"" and b"null tensor" in lib.ddpm_last_error()
