"""Record what the convolution dispatcher decides for a sweep of descriptors -> tests/golden/conv_dispatch_parent.json.

The four questions are host-only (which family takes the descriptor, its stats parts, its scratch floats, whether it takes
wino44h) and look at pointers only for NULL-ness and 16-byte alignment, so they are asked with fake pointers, without a GPU
(device_cus() answers 256 without a device, which is what an MI355X has).

The fixture is recorded ONCE from the commit before the selection table (csrc/conv_dispatch.hip) existed:

    git worktree add /tmp/parent <that commit>
    (cd /tmp/parent && patch -p1 < tools/patches/conv_dispatch_name.patch && bash ddpm_ood_amd/csrc/build.sh)
    python tools/record_conv_dispatch.py --lib /tmp/parent/ddpm_ood_amd/libddpm_ood_hip.so

(the patch adds ddpm_conv_kernel_name to that commit as a name-returning copy of its conv_dispatch if-chain; its
ddpm_conv_stats_parts was a hand-written mirror of the chain, so the two may disagree: such rows go under
"parent_mirror_disagrees" with both answers, and "answers" then holds what the kernel that actually runs would write).
tests/test_conv_dispatch_host.py replays the fixture against the built library.  `--check` replays it here and prints the
coverage of the sweep instead of writing.
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ddpm_ood_amd._lib import ConvDesc  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "conv_dispatch_parent.json"
NORMAL, STRIDE2, UPSAMPLE2, TRANSPOSE2 = 0, 1, 2, 3
# descriptor row: FIELDS in this order; "ptrs" = bit i set <-> pointer PTRS[i] is non-NULL (a fake, 256-byte aligned address)
FIELDS = ("ptrs", "C1", "C2", "B", "Cout", "Hi", "Ho", "ksize", "mode", "act", "force_direct", "Di", "Do", "dims")
PTRS = ("in1", "out", "bias", "w_raw", "w_packed", "in2", "gscale", "gshift", "chan_add", "residual", "w_folded", "w_wino",
        "w_wino44", "w_wino44h", "w_d3h", "scratch")
P = {n: 1 << i for i, n in enumerate(PTRS)}
# the families that write stats_out: what the parent's launchers themselves keep desc.stats_out for
STATS_FAMILIES = ("d3s", "wino44h", "wino", "d3s2", "s2h", "direct")
# switch settings the H = 8 / H = 32 slices are replayed under ("default": the whole sweep)
SETTINGS = [
    {"name": "default", "env": {}, "split_f16": 1},
    {"name": "DDPM_CONV_WINO44=0", "env": {"DDPM_CONV_WINO44": "0"}, "split_f16": 1},
    {"name": "DDPM_CONV_WINO44=2", "env": {"DDPM_CONV_WINO44": "2"}, "split_f16": 1},
    {"name": "DDPM_CONV_D3S=0", "env": {"DDPM_CONV_D3S": "0"}, "split_f16": 1},
    {"name": "DDPM_CONV_D3S=2", "env": {"DDPM_CONV_D3S": "2"}, "split_f16": 1},
    {"name": "DDPM_DOWN_S2H=0", "env": {"DDPM_DOWN_S2H": "0"}, "split_f16": 1},
    {"name": "DDPM_UP_WINO44H=0", "env": {"DDPM_UP_WINO44H": "0"}, "split_f16": 1},
    {"name": "DDPM_CONV_SPLITK=0", "env": {"DDPM_CONV_SPLITK": "0"}, "split_f16": 1},
    {"name": "split_f16=0", "env": {}, "split_f16": 0},
]
CHANNELS = [(1, 0, 128), (3, 0, 256), (128, 0, 1), (128, 0, 3), (64, 0, 64), (96, 0, 96), (128, 0, 128), (128, 128, 128),
            (256, 0, 256), (256, 256, 256), (512, 0, 256), (128, 0, 384)]
BATCHES = [1, 2, 16, 128, 256, 1024]
EXTENTS = [1, 8, 16, 32, 64]
KMODES = [(1, NORMAL), (3, NORMAL), (3, STRIDE2), (3, UPSAMPLE2)]


def load(path):
    lib = C.CDLL(str(path))
    for name, res in (("ddpm_conv_kernel_name", C.c_char_p), ("ddpm_conv_stats_parts", C.c_int),
                      ("ddpm_conv_scratch_floats", C.c_size_t), ("ddpm_conv_takes_wino44h", C.c_int)):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = [C.POINTER(ConvDesc)]
    for name in ("ddpm_packed_conv_weight_floats", "ddpm_wino_weight_floats", "ddpm_wino44_weight_floats",
                 "ddpm_wino44h_weight_halves", "ddpm_conv_d3h_weight_halves", "ddpm_conv_d1s_weight_halves",
                 "ddpm_conv1x1_h_weight_halves", "ddpm_conv_s2h_weight_halves", "ddpm_folded_upsample_weight_floats"):
        getattr(lib, name).restype = C.c_size_t
    return lib


def engine_forms(lib, cin, cout, k, mode):
    """The weight forms csrc/unet_engine.hip keeps for a 2-D convolution of this shape and attaches in this mode."""
    p = P["w_raw"]
    packed = lib.ddpm_packed_conv_weight_floats(cout, cin, k) != 0
    if packed:
        p |= P["w_packed"]
    if k == 1:
        if packed and lib.ddpm_conv1x1_h_weight_halves(cout, cin):
            p |= P["w_wino44h"]
        if lib.ddpm_conv_d1s_weight_halves(cout, cin):
            p |= P["w_d3h"]
        return p
    d3h = P["w_d3h"] if lib.ddpm_conv_d3h_weight_halves(cout, cin) else 0
    wino = P["w_wino"] if lib.ddpm_wino_weight_floats(cout, cin) else 0
    w44h = P["w_wino44h"] if lib.ddpm_wino44h_weight_halves(cout, cin) else 0
    if mode == NORMAL:
        p |= wino | w44h | d3h | (P["w_wino44"] if wino and lib.ddpm_wino44_weight_floats(cout, cin) else 0)
    elif mode == STRIDE2:
        p |= d3h | (P["w_wino44h"] if lib.ddpm_conv_s2h_weight_halves(cout, cin) else 0)
    elif lib.ddpm_folded_upsample_weight_floats(cout, cin):
        p |= P["w_folded"] | wino | w44h | d3h
    return p


def sweep(lib):
    """-> (descriptor rows, indices of the rows every switch setting replays)."""
    rows, sliced = [], []
    base = P["in1"] | P["out"] | P["bias"]

    def add(ptrs, c1, c2, b, cout, hi, k, mode, act=0, fd=0, di=0, do=0, dims=0, in_slice=False):
        ho = {NORMAL: hi, STRIDE2: (hi + 1) // 2 if k == 3 else hi // 2, UPSAMPLE2: 2 * hi, TRANSPOSE2: 2 * hi}[mode]
        rows.append([ptrs | (P["in2"] if c2 else 0), c1, c2, b, cout, hi, ho, k, mode, act, fd, di, do, dims])
        if in_slice:
            sliced.append(len(rows) - 1)

    for c1, c2, cout in CHANNELS:
        for k, mode in KMODES:
            eng = base | engine_forms(lib, c1 + c2, cout, k, mode) | P["scratch"]
            raw = base | (eng & (P["w_raw"] | P["w_packed"])) | P["scratch"]
            for h in EXTENTS:
                for b in BATCHES:
                    thin = h in (8, 32) and b in (1, 16, 256)
                    add(eng, c1, c2, b, cout, h, k, mode, in_slice=thin)
                    if not thin:
                        continue
                    add(raw, c1, c2, b, cout, h, k, mode)  # w_raw and w_packed only
                    if b == 1:
                        continue
                    # one at a time around the grid: GroupNorm + SiLU prologue, no scratch, force_direct, the epilogue addends
                    add(eng | P["gscale"] | P["gshift"], c1, c2, b, cout, h, k, mode, act=1)
                    add(eng & ~P["scratch"], c1, c2, b, cout, h, k, mode)
                    add(eng, c1, c2, b, cout, h, k, mode, fd=1)
                    add(eng | P["chan_add"] | P["residual"], c1, c2, b, cout, h, k, mode)
    # 3-D (VQ-VAE, 3-D UNet): k3 s1 with and without the Winograd forms, k4 s2, ConvTranspose k4 s2
    v = base | P["w_packed"] | P["scratch"]
    for c in (128, 256):
        for d in (1, 8, 32):
            for h in (8, 16, 32):
                for b in (1, 16):
                    s = h in (8, 32)
                    for forms in (0, P["w_wino"], P["w_wino"] | P["w_wino44"], P["w_wino"] | P["w_wino44"] | P["w_wino44h"]):
                        add(v | forms, c, 0, b, c, h, 3, NORMAL, di=d, do=d, dims=3, in_slice=s)
                    add(v, c, 0, b, c, h, 4, STRIDE2, di=d, do=d // 2, dims=3, in_slice=s)
                    add(v, c, 0, b, c, h, 4, TRANSPOSE2, di=d, do=2 * d, dims=3, in_slice=s)
    return rows, sliced


def descriptor(row):
    r = dict(zip(FIELDS, row))
    d = ConvDesc()
    for i, n in enumerate(PTRS):
        if r["ptrs"] >> i & 1:
            setattr(d, n, 0x100000 * (i + 1))
    for n in ("C1", "C2", "B", "Cout", "Hi", "Ho", "ksize", "mode", "act", "force_direct", "Di", "Do", "dims"):
        setattr(d, n, r[n])
    d.Wi, d.Wo = r["Hi"], r["Ho"]
    d.chan_add_stride = r["Cout"] if d.chan_add else 0
    return d


def ask(lib, row):
    """-> [family, stats parts, scratch floats, takes wino44h]; a row with "scratch" carries it at the size the library asks for."""
    d = descriptor(row)
    d.scratch = None
    need = lib.ddpm_conv_scratch_floats(C.byref(d))
    if row[0] & P["scratch"] and need:
        d.scratch, d.scratch_floats = 0x100000 * len(PTRS), need
    ref = C.byref(d)
    return [lib.ddpm_conv_kernel_name(ref).decode(), lib.ddpm_conv_stats_parts(ref), lib.ddpm_conv_scratch_floats(ref),
            lib.ddpm_conv_takes_wino44h(ref)]


class setting:
    """The library under one switch setting (environment + ddpm_set_split_f16); the default is restored on exit."""

    def __init__(self, lib, s):
        self.lib, self.s = lib, s

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.s["env"]}
        os.environ.update(self.s["env"])
        self.lib.ddpm_reload_env()
        self.lib.ddpm_set_split_f16(self.s["split_f16"])

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.lib.ddpm_reload_env()
        self.lib.ddpm_set_split_f16(1)


def record(lib):
    rows, sliced = sweep(lib)
    answers, disagree = {}, []
    for s in SETTINGS:
        idx = list(range(len(rows))) if s["name"] == "default" else sliced
        with setting(lib, s):
            out = []
            for i in idx:
                a = ask(lib, rows[i])
                if a[1] > 0 and a[0] not in STATS_FAMILIES:  # the mirror promised statistics the launched kernel never writes
                    disagree.append({"setting": s["name"], "desc": i, "family": a[0], "mirror_stats_parts": a[1], "stats_parts": 0})
                    a[1] = 0
                out.append(a)
        answers[s["name"]] = out
    return {"fields": FIELDS, "ptrs": PTRS, "settings": SETTINGS, "parent_mirror_disagrees": disagree, "descs": rows,
            "slice": sliced, "answers": answers}


def coverage(fix):
    sel, pos, zero = {}, set(), set()
    for name, a in fix["answers"].items():
        for i, (fam, parts, _, _) in zip(range(len(fix["descs"])) if name == "default" else fix["slice"], a):
            key = ("3d" if fix["descs"][i][-1] == 3 or fix["descs"][i][7] == 4 else "2d", fam)
            sel[key] = sel.get(key, 0) + 1
            (pos if parts > 0 else zero).add(fam)
    return sel, pos, zero


def dump(fix):
    def lines(items):
        return "[\n" + ",\n".join(json.dumps(x, separators=(",", ":")) for x in items) + "\n]"

    head = {k: fix[k] for k in ("fields", "ptrs", "settings", "parent_mirror_disagrees")}
    body = json.dumps(head, indent=1)[:-2] + ',\n "descs": ' + lines(fix["descs"])
    body += ',\n "slice": ' + json.dumps(fix["slice"], separators=(",", ":")) + ',\n "answers": {\n'
    return body + ",\n".join(f" {json.dumps(name)}: {lines(a)}" for name, a in fix["answers"].items()) + "\n }\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", required=True, help="libddpm_ood_hip.so that exports ddpm_conv_kernel_name")
    ap.add_argument("--check", action="store_true", help="compare with the fixture and print the coverage; write nothing")
    args = ap.parse_args()
    fix = record(load(args.lib))
    sel, pos, zero = coverage(fix)
    for key in sorted(sel):
        print(f"{key[0]} {key[1] or '(refused)':14s} {sel[key]:6d}")
    print("stats parts > 0:", sorted(pos), " == 0:", sorted(zero & set(STATS_FAMILIES)))
    print(f"{len(fix['descs'])} descriptors, {sum(len(a) for a in fix['answers'].values())} answers, "
          f"{len(fix['parent_mirror_disagrees'])} mirror disagreements")
    if args.check:
        want = json.loads(FIXTURE.read_text())
        same = json.loads(json.dumps(fix)) == want
        print("fixture matches" if same else "fixture DIFFERS")
        return 0 if same else 1
    FIXTURE.write_text(dump(fix))
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
