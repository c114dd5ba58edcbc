"""GPU: a forward of the UNet engine gives the bits the commit before the weight-form table (csrc/unet_engine.hip) gave.

tests/golden/unet_forms_parent.json, "digests": SHA-256 of the output of one eager forward per (configuration, switch setting),
recorded on an MI355X from that commit by tools/record_unet_forms.py --gpu (two processes, which agreed on every row: the
kernels are fixed-order).  The settings steer the convolutions to different kernel families, hence to different packed weight
forms: a form that is not allocated, not refreshed by ddpm_unet_set_param or attached to the wrong launches changes the bits (or
the family, which the first test pins).  Weights, input and timesteps come from one seeded torch.Generator
(record_unet_forms.fill_state_dict / forward); the environment is set before the engine is created.
"""

import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("record_unet_forms", ROOT / "tools" / "record_unet_forms.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)
SETTINGS = {s["name"]: s for s in rec.GPU_SETTINGS}


@pytest.fixture(scope="module")
def fix():
    return json.loads(rec.FIXTURE.read_text())


def test_every_row_has_a_digest_and_every_setting_its_families(device, fix):
    from ddpm_ood_amd import _lib

    assert sorted(fix["digests"]) == sorted(f"{c}|{s}" for c in rec.GPU_CONFIGS for s in SETTINGS)
    for s in rec.GPU_SETTINGS:
        assert rec.families(_lib.load(), s) == s["families"], s["name"]
    # the settings do not all run one kernel: the two_level rows differ pairwise
    assert len({fix["digests"][f"two_level|{s}"] for s in SETTINGS}) == len(SETTINGS)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("config", list(rec.GPU_CONFIGS))
def test_forward_has_the_parent_commits_bits(device, fix, config, setting):
    from ddpm_ood_amd import _lib

    y = rec.forward(_lib.load(), config, SETTINGS[setting])
    assert rec.digest(y) == fix["digests"][f"{config}|{setting}"]
