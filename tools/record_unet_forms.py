"""Record what the UNet engine allocates and computes for a sweep of configurations -> tests/golden/unet_forms_parent.json.

Which packed weight forms a convolution carries (csrc/unet_engine.hip) shows in three host-only numbers -- the size of the
parameter blob, the parameter list, and the workspace size (the sizing pass attaches the forms and asks conv_scratch_floats,
which looks at the pointers) -- and in the bits of a forward.  ddpm_unet_create, ddpm_unet_param_blob_floats and
ddpm_unet_workspace_bytes[3d] need no GPU (device_cus() answers 256 without a device, which is what an MI355X has).

The fixture is recorded ONCE from the commit before the weight-form table existed:

    git worktree add /tmp/parent <that commit>
    (cd /tmp/parent && bash ddpm_ood_amd/csrc/build.sh && cp <this file> tools/)
    (cd /tmp/parent && python tools/record_unet_forms.py --gpu --out /tmp/run1.json)      # on an MI355X, two processes
    (cd /tmp/parent && python tools/record_unet_forms.py --gpu --out /tmp/run2.json)
    python tools/record_unet_forms.py --lib /tmp/parent/ddpm_ood_amd/libddpm_ood_hip.so --digests /tmp/run1.json /tmp/run2.json

(--gpu runs the package the file sits in; a digest is only kept if every --digests file agrees on it.)
tests/test_unet_weight_forms_host.py replays the host rows and tests/test_gpu_unet_forms_digest.py the digests against the
built library.  `--check` replays the host rows here instead of writing.
"""

from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
import record_conv_dispatch as rcd  # noqa: E402
from ddpm_ood_amd._lib import UNetConfig  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "unet_forms_parent.json"
SMALL = dict(num_channels=[128, 256, 256], attention_levels=[0, 0, 1], num_res_blocks=1, num_head_channels=256)
BIG = dict(num_channels=[256, 512, 768], attention_levels=[1, 1, 1], num_res_blocks=2, num_head_channels=256)
# two levels, channel counts change: a skip 1x1 and concatenated-input residual convolutions exist
TWO_LEVEL = dict(num_channels=[128, 256], attention_levels=[0, 1], num_res_blocks=1, num_head_channels=256)
CONFIGS = {
    "small": dict(spatial_dims=2, channels=1, use_proj_attn=0, **SMALL),  # trainer.MODEL_CONFIGS
    "big": dict(spatial_dims=2, channels=1, use_proj_attn=0, **BIG),
    "two_level": dict(spatial_dims=2, channels=1, use_proj_attn=1, **TWO_LEVEL),
    "two_level_noproj": dict(spatial_dims=2, channels=1, use_proj_attn=0, **TWO_LEVEL),
    "small3d": dict(spatial_dims=3, channels=128, use_proj_attn=0, **SMALL),  # tests/test_gpu_configs.py: SMALL, 3-D
}
HOST_ENVS = [{"name": "default", "env": {}}, {"name": "DDPM_CONV_D3S=0", "env": {"DDPM_CONV_D3S": "0"}}]
SHAPES_2D = [[1, 32], [2, 32], [16, 32], [256, 32], [2, 64]]  # (B, H = W)
SHAPES_3D = [[b, d, h] for b in (1, 4) for d, h in ((4, 8), (4, 4), (8, 4))]  # (B, D, H = W)
# one eager forward per (configuration, setting); "families": what ddpm_conv_kernel_name has to answer for the configuration's
# representative descriptors (REPRESENTATIVE) under the setting -- the digests must not all come from one kernel
# (configuration, B, D, H = W).  B = 64: the DMA-fed 1x1 kernel takes launches of 64 workgroups or more, which B = 2 never has;
# 8 x 8 slices: the smallest the 3-D F(2x2) kernel takes (at 4 x 4 every 3x3x3 convolution runs on the MFMA kernel)
GPU_CONFIGS = {"two_level": ["two_level", 2, 1, 32], "small3d": ["small3d", 2, 4, 4], "two_level_b64": ["two_level", 64, 1, 32],
               "small3d_8": ["small3d", 2, 4, 8]}
GPU_SETTINGS = [
    {"name": "default", "env": {}, "families": {"res": "d3s", "down": "d3s2", "skip": "d1s"}},
    {"name": "wino44h", "env": {"DDPM_CONV_D3S": "0", "DDPM_CONV_WINO44": "2"},
     "families": {"res": "wino44h", "down": "s2h", "skip_b64": "conv1x1_dma", "up": "wino44h"}},
    {"name": "wino44", "env": {"DDPM_CONV_D3S": "0", "DDPM_CONV_WINO44": "2", "DDPM_WINO44_F16X3": "0"},
     "families": {"res": "wino44"}},
    {"name": "wino", "env": {"DDPM_CONV_D3S": "0", "DDPM_CONV_WINO44": "0"}, "families": {"res": "wino", "up": "wino"}},
    # no Winograd family at all: the MFMA kernel on the packed form, the upsampler on its folded form
    {"name": "mfma", "env": {"DDPM_CONV_D3S": "0", "DDPM_CONV_WINO44": "0", "DDPM_CONV_WINOGRAD": "0"},
     "families": {"res": "mfma", "up": "mfma", "skip": "mfma"}},
]
# launches of the two_level forwards (32 x 32 input): (B, C1, C2, Cout, Hi, ksize, mode, GroupNorm + SiLU prologue and residual?)
REPRESENTATIVE = {
    "res": (2, 256, 0, 256, 16, 3, rcd.NORMAL, True),     # down_blocks.1.resnets.0.conv2
    "down": (2, 128, 0, 128, 32, 3, rcd.STRIDE2, False),  # down_blocks.0.downsampler
    "skip": (2, 128, 0, 256, 16, 1, rcd.NORMAL, False),   # down_blocks.1.resnets.0.skip_connection
    "skip_b64": (64, 128, 0, 256, 16, 1, rcd.NORMAL, False),
    "up": (2, 256, 0, 256, 16, 3, rcd.UPSAMPLE2, False),  # up_blocks.0.upsampler
}
SEED = 20240607


def load(path=None):
    if path is None:
        from ddpm_ood_amd import _lib

        return _lib.load()
    lib = rcd.load(path)
    lib.ddpm_last_error.restype = C.c_char_p
    lib.ddpm_unet_create.restype = C.c_void_p
    lib.ddpm_unet_create.argtypes = [C.POINTER(UNetConfig)]
    lib.ddpm_unet_destroy.argtypes = [C.c_void_p]
    for name, res, args in (("ddpm_unet_param_blob_floats", C.c_size_t, []), ("ddpm_unet_num_params", C.c_int, []),
                            ("ddpm_unet_param_name", C.c_char_p, [C.c_int]), ("ddpm_unet_param_numel", C.c_int64, [C.c_int]),
                            ("ddpm_unet_workspace_bytes", C.c_size_t, [C.c_int] * 3),
                            ("ddpm_unet_workspace_bytes3d", C.c_size_t, [C.c_int] * 4)):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = [C.c_void_p] + args
    return lib


def unet_config(spec) -> UNetConfig:
    """The ddpm_unet_config DiffusionModelUNet._config() fills for this configuration (without building the module)."""
    cfg = UNetConfig()
    cfg.spatial_dims, cfg.in_channels, cfg.out_channels = spec["spatial_dims"], spec["channels"], spec["channels"]
    cfg.num_levels = len(spec["num_channels"])
    for i, (c, a) in enumerate(zip(spec["num_channels"], spec["attention_levels"])):
        cfg.num_channels[i], cfg.attention_levels[i] = c, a
        cfg.num_res_blocks[i], cfg.num_head_channels[i] = spec["num_res_blocks"], spec["num_head_channels"]
    cfg.norm_num_groups, cfg.norm_eps, cfg.use_proj_attn = 32, 1e-6, spec["use_proj_attn"]
    return cfg


def model_kwargs(spec):
    return dict(spatial_dims=spec["spatial_dims"], in_channels=spec["channels"], out_channels=spec["channels"],
                num_channels=tuple(spec["num_channels"]), attention_levels=tuple(bool(a) for a in spec["attention_levels"]),
                num_res_blocks=spec["num_res_blocks"], num_head_channels=spec["num_head_channels"],
                use_proj_attn=bool(spec["use_proj_attn"]))


class environment:
    """The library's switches under these DDPM_* variables (set before the engine is created); restored on exit."""

    def __init__(self, lib, env):
        self.lib, self.env = lib, env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        self.lib.ddpm_reload_env()

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        self.lib.ddpm_reload_env()


def host_row(lib, spec, env):
    """-> {"blob_floats", "params": [[name, numel], ...], "workspace": [shape + [bytes], ...]} of an engine created under env."""
    with environment(lib, env):
        cfg = unet_config(spec)
        h = C.c_void_p(lib.ddpm_unet_create(C.byref(cfg)))
        assert h, lib.ddpm_last_error()
        try:
            params = [[lib.ddpm_unet_param_name(h, i).decode(), lib.ddpm_unet_param_numel(h, i)]
                      for i in range(lib.ddpm_unet_num_params(h))]
            if spec["spatial_dims"] == 3:
                ws = [[b, d, e, lib.ddpm_unet_workspace_bytes3d(h, b, d, e, e)] for b, d, e in SHAPES_3D]
            else:
                ws = [[b, e, lib.ddpm_unet_workspace_bytes(h, b, e, e)] for b, e in SHAPES_2D]
            return {"blob_floats": lib.ddpm_unet_param_blob_floats(h), "params": params, "workspace": ws}
        finally:
            lib.ddpm_unet_destroy(h)


def record_host(lib):
    """-> (parameter lists per configuration, rows per "configuration|environment"); the list does not depend on the environment."""
    params, rows = {}, {}
    for cname, spec in CONFIGS.items():
        for e in HOST_ENVS:
            row = host_row(lib, spec, e["env"])
            assert params.setdefault(cname, row["params"]) == row["params"], (cname, e["name"])
            rows[f"{cname}|{e['name']}"] = {"blob_floats": row["blob_floats"], "workspace": row["workspace"]}
    return params, rows


def families(lib, setting):
    """ddpm_conv_kernel_name of the REPRESENTATIVE descriptors (weight forms as the engine attaches them) under the setting."""
    out = {}
    with environment(lib, setting["env"]):
        for key in setting["families"]:
            b, c1, c2, cout, hi, k, mode, fused = REPRESENTATIVE[key]
            p = rcd.P
            ptrs = p["in1"] | p["out"] | p["bias"] | p["scratch"] | rcd.engine_forms(lib, c1 + c2, cout, k, mode)
            if setting["env"].get("DDPM_CONV_D3S") == "0":  # read when the engine is created: no d3h / d1s planes
                ptrs &= ~p["w_d3h"]
            if fused:
                ptrs |= p["gscale"] | p["gshift"] | p["residual"]
            ho = {rcd.NORMAL: hi, rcd.STRIDE2: (hi + 1) // 2, rcd.UPSAMPLE2: 2 * hi}[mode]
            out[key] = rcd.ask(lib, [ptrs, c1, c2, b, cout, hi, ho, k, mode, int(fused), 0, 0, 0, 0])[0]
    return out


def fill_state_dict(model, seed=SEED):
    """Every entry of the state_dict from one torch.Generator: weights N(0, 1 / fan_in), GroupNorm gammas 1 + 0.1 N, biases 0.1 N."""
    import torch

    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if v.ndim >= 2:
            sd[k] = r * float(v[0].numel()) ** -0.5
        else:
            sd[k] = 1 + 0.1 * r if k.endswith(".weight") else 0.1 * r
    return sd


def forward(lib, cname, setting):
    """One eager forward of the configuration under the setting -> the output as a host tensor."""
    import torch

    from ddpm_ood_amd import DiffusionModelUNet

    config, b, d, e = GPU_CONFIGS[cname]
    spec = CONFIGS[config]
    with environment(lib, setting["env"]):
        model = DiffusionModelUNet(**model_kwargs(spec))
        assert bytes(model._config()) == bytes(unet_config(spec)), cname
        model.load_state_dict(fill_state_dict(model))
        model = model.to("cuda:0").eval()
        g = torch.Generator().manual_seed(SEED + 1)
        shape = (b, spec["channels"]) + ((d, e, e) if spec["spatial_dims"] == 3 else (e, e))
        x = torch.randn(shape, generator=g)
        t = torch.randint(0, 1000, (b,), generator=g)
        y = model(x.to("cuda:0"), timesteps=t.to("cuda:0")).cpu()
        del model
    assert torch.isfinite(y).all() and y.abs().max() > 1e-3, (cname, setting["name"])
    return y


def digest(y) -> str:
    return hashlib.sha256(y.contiguous().numpy().tobytes()).hexdigest()


def record_gpu(lib):
    return {f"{c}|{s['name']}": digest(forward(lib, c, s)) for c in GPU_CONFIGS for s in GPU_SETTINGS}


def sweep():
    return {"configs": CONFIGS, "host_envs": HOST_ENVS, "shapes_2d": SHAPES_2D, "shapes_3d": SHAPES_3D,
            "gpu_configs": GPU_CONFIGS, "gpu_settings": GPU_SETTINGS, "seed": SEED}


def dump(fix):
    def lines(d):
        return "{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n }"

    return "{" + ",".join(f'\n "{k}": {lines(fix[k])}' for k in ("sweep", "params", "host", "digests")) + "\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", help="libddpm_ood_hip.so to ask the host-only questions (default: the one in this tree)")
    ap.add_argument("--check", action="store_true", help="compare the host rows with the fixture; write nothing")
    ap.add_argument("--gpu", action="store_true", help="run the forwards on cuda:0 with this tree's package; needs --out")
    ap.add_argument("--out", help="with --gpu: the JSON file the digests go to")
    ap.add_argument("--digests", nargs="+", default=[], help="--gpu outputs to take the digests from")
    args = ap.parse_args()
    lib = load(args.lib)
    if args.gpu:
        Path(args.out).write_text(json.dumps(record_gpu(lib), indent=1) + "\n")
        print(f"wrote {args.out}")
        return 0
    params, rows = record_host(lib)
    for s in GPU_SETTINGS:
        got = families(lib, s)
        print(f"{s['name']:8s} {got}")
        assert got == s["families"], (s["name"], got)
    if args.check:
        want = json.loads(FIXTURE.read_text())
        same = want["sweep"] == json.loads(json.dumps(sweep())) and want["params"] == params and want["host"] == rows
        print("fixture matches" if same else "fixture DIFFERS")
        return 0 if same else 1
    runs = [json.loads(Path(p).read_text()) for p in args.digests]
    unstable = sorted(k for r in runs for k in r if r[k] != runs[0].get(k))
    if unstable:
        print("digests differ between the runs (not recorded):", unstable)
    digests = {k: v for k, v in runs[0].items() if k not in unstable} if runs else {}
    FIXTURE.write_text(dump({"sweep": sweep(), "params": params, "host": rows, "digests": digests}))
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes, {len(rows)} host rows, {len(digests)} digests)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
