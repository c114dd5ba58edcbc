"""CPU: the host side of the training attention (tests/test_gpu_train_attention*.py run the kernels) -- the two
entry points' argument checks (no device is reached), header / SIGNATURES / exports, the wrappers' refusals, the knob's parsing, and
the build-time property the kernels live by: 128 to 256 live registers per lane at head dim 256 without a byte of scratch."""

import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("ddpm_attention_train_fwd_f32", "ddpm_attention_train_bwd_f32")
FAKE = 0x10000  # never dereferenced: the argument checks come first
STEP = 1 << 24


@pytest.fixture(scope="module")
def lib():
    from ddpm_ood_amd import _lib

    return _lib.load()


def test_entry_points_are_declared_exported_bound_and_add_no_size_function(lib):
    from ddpm_ood_amd import _lib

    header = (ROOT / "include" / "ddpm_ood_hip.h").read_text()
    for name, pointers in zip(NAMES, (5, 10)):
        assert re.search(rf"\bint {name}\(", header)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is C.c_int
        assert args == [C.c_void_p] * pointers + [C.c_int] * 4 + [C.c_float, C.c_void_p]  # buffers, B C N heads, scale, stream
        proto = re.search(rf"\bint {name}\(([^;]*)\);", header).group(1)
        assert proto.count("*") == pointers and proto.count("int ") == 4 and "ddpm_stream_t stream" in proto
    assert not [n for n, (res, _) in _lib.SIGNATURES.items() if res is C.c_size_t and "attention_train" in n]
    assert lib.ddpm_abi_version() == 10 == _lib.ABI_VERSION  # additive entries: the ABI version stays
    assert "#define DDPM_ABI_VERSION 10" in header


def _refusals(f, n_ptr):
    ok = [FAKE + i * STEP for i in range(n_ptr)]
    from ddpm_ood_amd import _lib

    err = _lib.load().ddpm_last_error
    for i in range(n_ptr):
        ptrs = list(ok)
        ptrs[i] = None
        assert f(*ptrs, 1, 256, 64, 1, 0.0625, None) == -1 and b"null" in err()
    for B, C_, N, heads, msg in ((1, 128, 64, 1, b"head dim 256"), (1, 256, 64, 2, b"head dim 256"), (1, 512, 64, 1, b"head dim 256"),
                                 (1, 256, 96, 1, b"multiple of 64"), (1, 256, 0, 1, b"multiple of 64"),
                                 (1, 256, -64, 1, b"multiple of 64"), (1, 256, 32, 1, b"multiple of 64"),
                                 (0, 256, 64, 1, b"positive"), (1, 0, 64, 0, b"positive"), (-1, 256, 64, 1, b"positive"),
                                 (64, 2048, 16384, 8, b"32-bit"), (2, 256, 1 << 22, 1, b"32-bit")):
        assert f(*ok, B, C_, N, heads, 0.0625, None) == -1 and msg in err(), (B, C_, N, heads, err())
    ptrs = list(ok)
    ptrs[0] += 4  # q off a 16-byte boundary
    assert f(*ptrs, 1, 256, 64, 1, 0.0625, None) == -1 and b"aligned" in err()


def test_forward_refuses_bad_arguments(lib):
    _refusals(lib.ddpm_attention_train_fwd_f32, 5)


def test_backward_refuses_bad_arguments(lib):
    _refusals(lib.ddpm_attention_train_bwd_f32, 10)


def test_wrappers_refuse_before_any_launch():
    import torch

    from ddpm_ood_amd import train_ops as T

    x = torch.zeros(1, 256, 64)
    with pytest.raises(ValueError, match="device tensor"):
        T.attention_fwd(x, x, x, 1, 0.0625)
    with pytest.raises(ValueError, match="device tensor"):
        T.attention_bwd(x, x, x, x, x, torch.zeros(1, 1, 64), 1, 0.0625)
    assert T.ATTN_HEAD_DIM == 256
    assert T.attention_takes(256, 64, 1) and T.attention_takes(768, 4096, 3)
    assert not T.attention_takes(256, 96, 1) and not T.attention_takes(256, 64, 2) and not T.attention_takes(128, 8, 1)
    assert not T.attention_takes(256, 0, 1) and not T.attention_takes(0, 64, 0)


def test_the_knob_is_documented_where_the_others_are():
    design = (ROOT / "DESIGN.md").read_text()
    assert "DDPM_TRAIN_ATTN" in design and "### 3.28" in design
    src = (ROOT / "ddpm_ood_amd" / "train_native.py").read_text()
    assert 'os.environ.get("DDPM_TRAIN_ATTN", "gemm")' in src  # the default: nothing changes for who does not set it


def test_kernels_use_no_scratch_and_do_not_spill_in_their_loops(tmp_path):
    """tools/asm_spill_report.py over the gfx950 assembly of csrc/attention_train.hip, compiled with build.sh's flags (cross-
    compilation: no GPU needed).  A wave holds its own tile (64 or 128 registers) and its accumulators (64 or 128) for the whole
    loop; one register too many and hipcc would quietly park some of them in scratch memory around every MFMA group."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "attention_train.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-value",
                    "--cuda-device-only", "-S", str(ROOT / "ddpm_ood_amd" / "csrc" / "attention_train.hip"), "-o", str(asm)],
                   check=True, stderr=subprocess.DEVNULL, timeout=600)
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "asm_spill_report.py"), str(asm)], capture_output=True, text=True,
                         check=True, timeout=120).stdout
    rows = [l for l in out.splitlines() if "attn_train" in l]
    assert len(rows) == 3, out  # forward, dq, dk / dv (the delta pre-pass has no MFMA)
    for row in rows:
        m = re.search(r"scratch bytes\s+(\S+)\s+compiler AGPR accesses by depth \[.*?\]\s+scratch instructions by depth \[(.*?)\]", row)
        assert m, row
        assert m.group(1) == "0" and [int(v) for v in m.group(2).split(",")] == [0, 0, 0, 0], row
    text = asm.read_text()
    assert text.count("v_mfma_f32_16x16x4_f32") >= 256 + 384 + 512  # exact fp32 products, fully unrolled blocks
    assert not re.search(r"\.private_segment_fixed_size:\s*[1-9]", text)
