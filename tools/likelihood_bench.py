"""Measurements behind DESIGN 3.20 (development / evidence tool; summary kept under profiles/likelihood.md).

  1. throughput (images/s) of the full T = 1000 variational bound on `small` at 32x32x1 for 16 and 1 024 images, with
     rows_per_forward = N (the package's loop order: one timestep per forward) and = 1 024 (timesteps packed); --runs runs of
     each, alternating, after one warm-up of each;
  2. the two row kernels by themselves (the library's ProfScope: hipEvent-bracketed launches) at 16 and 1 024 rows.

    python tools/likelihood_bench.py [--runs 3] [--out likelihood_bench.json]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

SCHED = dict(schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--images", default="16,1024")
    ap.add_argument("--packed", type=int, default=1024)
    ap.add_argument("--out", default="likelihood_bench.json")
    a = ap.parse_args()
    from ddpm_ood_amd import DDPMScheduler, DiffusionInferer, DiffusionModelUNet, _lib, ops
    from ddpm_ood_amd.data import synthetic_images
    from ddpm_ood_amd.synthetic import random_state_dict
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    dev = torch.device("cuda:0")
    lib = _lib.load()
    model = DiffusionModelUNet(2, 1, 1, **MODEL_CONFIGS["small"])
    model.load_state_dict(random_state_dict("small", 1, seed=1))
    model = model.to(dev).eval()
    sched = DDPMScheduler(1000, **SCHED)
    inf = DiffusionInferer(sched)
    out = {"device": torch.cuda.get_device_name(0), "throughput": [], "kernels": {}}

    for n in [int(v) for v in a.images.split(",")]:
        x0 = synthetic_images("blobs", n, 1, 32, seed=0).to(dev)
        modes = sorted({n, a.packed})
        for rows in modes:  # warm-up: allocations, the engine's workspaces of both batch sizes
            sched.set_timesteps(max(1, 4 * rows // n))
            inf.get_likelihood(x0, model, rows_per_forward=rows)
        sched.set_timesteps(1000)
        for run in range(a.runs):
            for rows in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                total = inf.get_likelihood(x0, model, rows_per_forward=rows)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = {"images": n, "rows_per_forward": rows, "run": run, "forwards": -(-n * 1000 // rows),
                       "seconds": round(dt, 4), "images_per_s": round(n / dt, 3), "mean_nll": float(total.mean())}
                out["throughput"].append(rec)
                print(json.dumps(rec), flush=True)

    coef = sched.likelihood_coefficients_device(dev)
    for rows in (16, 1024):
        x0 = synthetic_images("blobs", 16, 1, 32, seed=0).to(dev)
        noise = torch.randn_like(x0)
        idx = ops.VlbRows([r % 16 for r in range(rows)], [(37 * r) % 1000 for r in range(rows)], 16, 1000, dev)
        x_t = ops.vlb_noise_rows(x0, noise, idx, None, coef)
        eps = torch.randn_like(x_t)
        term = torch.empty(rows, device=dev)
        for _ in range(10):
            ops.vlb_noise_rows(x0, noise, idx, None, coef, out=x_t)
            ops.vlb_term_rows(x0, x_t, eps, idx, None, coef, out=term)
        torch.cuda.synchronize()
        lib.ddpm_prof_enable(1)
        for _ in range(100):
            ops.vlb_noise_rows(x0, noise, idx, None, coef, out=x_t)
            ops.vlb_term_rows(x0, x_t, eps, idx, None, coef, out=term)
        lib.ddpm_prof_enable(0)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.ddpm_prof_report(buf, len(buf))
        prof = json.loads(buf.value.decode())
        rec = {k: {"us_per_launch": round(v["ms"] / v["launches"] * 1e3, 2), "GBps": round(v["bytes"] / v["ms"] / 1e6, 1)}
               for k, v in prof.items() if k.startswith("vlb_")}
        out["kernels"][f"rows{rows}"] = rec
        print(f"kernels at {rows} rows of 32x32x1:", json.dumps(rec), flush=True)
    Path(a.out).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
