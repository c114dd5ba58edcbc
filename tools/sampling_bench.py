"""Measurements behind DESIGN 3.16 (development / evidence tool; summary kept under profiles/sampling.md).

  1. the fused ancestral step against the unfused composition (train_ops.randn + the same arithmetic in torch ops) at
     [8, 1, 32, 32] and [1024, 1, 32, 32]: median of --launches event-timed calls after warm-up, and the mean of the same calls
     issued back to back (host launch cost included);
  2. sampling throughput (images/s) of the sample.py loop on `small` at 32x32x1 for 8 and 256 samples, 1000-step DDPM and
     100-step PNDM, with DDPM_UNET_GRAPH unset and set to 1, against the ATen route doing the same loop (unet_forward_torch
     under no_grad + a torch-op step).

    python tools/sampling_bench.py [--launches 300] [--out sampling_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

SCHED = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)


def timed(fn, launches, warmup=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / launches
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, wall * 1e6  # us, us


def step_bench(dev, launches):
    from ddpm_ood_amd import DDPMScheduler, train_ops
    from ddpm_ood_amd.scheduler import sampling_key

    out = {}
    s = DDPMScheduler(**SCHED)
    t = 500
    sa, sb, c0, ct, sigma = s.step_coefficients(t)
    for B in (8, 1024):
        x, e = torch.randn(B, 1, 32, 32, device=dev), torch.randn(B, 1, 32, 32, device=dev)
        s.step(e, t, x)  # uploads the stream table

        def fused():
            return s.step(e, t, x)

        def unfused():
            z = train_ops.randn(tuple(x.shape), dev, sampling_key(0), t)
            x0 = ((x - sb * e) / sa).clamp_(-1, 1)
            return c0 * x0 + ct * x + sigma * z, x0

        f_ev, f_wall = timed(fused, launches)
        u_ev, u_wall = timed(unfused, launches)
        n = x.numel()
        out[f"B{B}"] = {"fused_us_event_median": round(f_ev, 2), "fused_us_back_to_back": round(f_wall, 2),
                        "unfused_us_event_median": round(u_ev, 2), "unfused_us_back_to_back": round(u_wall, 2),
                        "fused_GBps_at_16B_per_element_with_pred": round(16.0 * n / (f_ev * 1e-6) / 1e9, 1),
                        "fused_GBps_at_12B_per_element": round(12.0 * n / (f_ev * 1e-6) / 1e9, 1)}
        print(f"step B={B}:", out[f"B{B}"], flush=True)
    return out


def loop_bench(dev):
    from ddpm_ood_amd import DiffusionInferer, DiffusionModelUNet, ops
    from ddpm_ood_amd.sampling import make_sampling_scheduler
    from ddpm_ood_amd.scheduler import sampling_key, sampling_streams
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.train import unet_forward_torch
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    model = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    model.load_state_dict(random_state_dict("small", 1, seed=1))
    model = model.to(dev).eval()
    kw = dict(prediction_type="epsilon", beta_schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    res = {}

    def aten_loop(x, sched, kind):
        B = x.shape[0]
        ets = []
        with torch.no_grad():
            for t in [int(v) for v in sched.timesteps]:
                eps = unet_forward_torch(model, x, torch.full((B,), t, device=dev))
                if kind == "ddpm":
                    sa, sb, c0, ct, sigma = sched.step_coefficients(t)
                    x0 = ((x - sb * eps) / sa).clamp_(-1, 1)
                    x = c0 * x0 + ct * x + (sigma * torch.randn_like(x) if sigma else 0)
                else:  # the same number of forwards and a step of the same cost (Euler form of the PLMS transfer)
                    sc, ce, dn, _, _ = sched.plms_coefficients(t, max(t - 10, 0))
                    x = sc * x - ce * eps / dn
        return x

    for n in (8, 256):
        x_t = ops.randn_rows((n, 1, 32, 32), sampling_key(0), sampling_streams(range(n), 1000), device=dev)
        for kind in ("ddpm", "pndm"):
            for route in ("hip", "hip_graph", "aten"):
                sched = make_sampling_scheduler(kind, **kw)
                if route == "hip_graph":
                    os.environ["DDPM_UNET_GRAPH"] = "1"
                else:
                    os.environ.pop("DDPM_UNET_GRAPH", None)
                inf = DiffusionInferer()
                run = (lambda: aten_loop(x_t, sched, kind)) if route == "aten" else (lambda: inf.sample(x_t, model, sched))
                if kind == "pndm" or n == 8:  # warm-up: the short loops whole, the long ones through their first use below
                    run()
                    sched = make_sampling_scheduler(kind, **kw)
                else:
                    model(x_t, timesteps=torch.zeros(n, dtype=torch.int64, device=dev))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res[f"n{n}_{kind}_{route}"] = {"seconds": round(dt, 3), "images_per_s": round(n / dt, 2)}
                print(f"n={n} {kind} {route}: {dt:.3f} s, {n / dt:.2f} images/s", flush=True)
    os.environ.pop("DDPM_UNET_GRAPH", None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--out", default="sampling_bench.json")
    ap.add_argument("--skip-loops", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "step": step_bench(dev, a.launches)}
    if not a.skip_loops:
        out["loops"] = loop_bench(dev)
    Path(a.out).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
