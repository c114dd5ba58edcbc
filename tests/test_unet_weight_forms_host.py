"""CPU: the UNet engine's weight-form table (csrc/unet_engine.hip) allocates and attaches what the hand-written sites before it did.

tests/golden/unet_forms_parent.json holds, for a sweep of configurations created with and without DDPM_CONV_D3S=0, three host-only
answers of the commit before the table existed (tools/record_unet_forms.py recorded them; its docstring says how): the size of
the parameter blob, the ordered (name, numel) parameter list, and the workspace size at a few input shapes.  Every packed form is
allocated on its own 64-float granule, so the blob size is the sum over the forms kept; the sizing pass attaches the forms to its
descriptors and asks conv_scratch_floats, which looks at the pointers, so the workspace size follows what is attached.
device_cus() answers 256 without a device, as on an MI355X: the answers are the GPU machine's.
"""

import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("record_unet_forms", ROOT / "tools" / "record_unet_forms.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


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


def test_fixture_is_the_recorders_sweep(fix):
    assert fix["sweep"] == json.loads(json.dumps(rec.sweep()))
    assert sorted(fix["params"]) == sorted(rec.CONFIGS)
    assert sorted(fix["host"]) == sorted(f"{c}|{e['name']}" for c in rec.CONFIGS for e in rec.HOST_ENVS)
    assert rec.FIXTURE.stat().st_size < 256 * 1024


def test_sweep_has_the_convolutions_the_roles_differ_in(fix):
    names = {c: [n for n, _ in fix["params"][c]] for c in fix["params"]}
    for c in ("two_level", "two_level_noproj"):  # channel counts change: skip 1x1, down- and upsampler, fused q / k / v
        for part in ("skip_connection.conv.weight", "downsampler.op.conv.weight", "upsampler.conv.conv.weight", "to_q.weight",
                     "proj_attn.weight", "time_emb_proj.weight"):
            assert any(n.endswith(part) for n in names[c]), (c, part)
    # the planes of conv_d3s.hip are a creation-time decision: without them the blob is smaller everywhere
    for c in rec.CONFIGS:
        assert fix["host"][f"{c}|DDPM_CONV_D3S=0"]["blob_floats"] < fix["host"][f"{c}|default"]["blob_floats"], c


@pytest.mark.parametrize("config", list(rec.CONFIGS))
@pytest.mark.parametrize("env", [e["name"] for e in rec.HOST_ENVS])
def test_same_blob_parameters_and_workspace_as_the_parent_commit(lib, fix, config, env):
    e = next(e for e in rec.HOST_ENVS if e["name"] == env)
    row = rec.host_row(lib, rec.CONFIGS[config], e["env"])
    want = fix["host"][f"{config}|{env}"]
    assert row["blob_floats"] == want["blob_floats"]
    assert row["params"] == fix["params"][config]
    assert row["workspace"] == want["workspace"]
    assert all(w[-1] > 0 for w in row["workspace"])


@pytest.mark.parametrize("setting", [s["name"] for s in rec.GPU_SETTINGS])
def test_settings_of_the_digest_test_reach_their_families(lib, setting):
    """The descriptors tests/test_gpu_unet_forms_digest.py names per setting: the dispatcher's answer needs no GPU."""
    s = next(s for s in rec.GPU_SETTINGS if s["name"] == setting)
    assert rec.families(lib, s) == s["families"]
