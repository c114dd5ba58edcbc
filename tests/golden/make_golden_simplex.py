"""Record the simplex-noise fixture from the reference's own function (run here, in the build container).

    python tests/golden/make_golden_simplex.py [--reference DIR]

Unlike make_golden.py, which pins the CPU oracle, this fixture pins the REFERENCE's arithmetic: its
src/utils/simplex_noise.py needs only numpy and numba, and with a stand-in ``numba`` module (njit = identity,
prange = range) it runs unmodified.  The file is imported at run time, nothing of it is kept: the .npz holds
seeds, timesteps, shapes and the noise the reference computed for them.

simplex_noise.npz
  slice_{k}            float64 [H, W]: rand_3d_fixed_T_octaves((H, W), [T], octaves, persistence, frequency)[0]
                       of a fresh Simplex_CLASS seeded with slice_seed[k] (before generate_simplex_noise's fp32 cast)
  slice_seed           int64 [N]
  slice_t              int64 [N]
  slice_hw             int64 [N, 2]
  slice_params         float64 [N, 3]: octaves, persistence, frequency
  {call}_noise         float32: generate_simplex_noise(simplex, x, t, in_channels=C) on x of shape {call}_shape
  {call}_t             int64 [B]
  {call}_seeds         int64 [C * B]: the seeds newSeed drew, in draw order (channel-major: for i < C, for j < B)
  {call}_shape         int64: x.shape
for call in (call2d, call3d).
"""

import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "simplex_noise.npz"

SIZES = ((32, 32), (28, 28), (64, 64), (8, 8), (16, 40))
TIMESTEPS = (0, 1, 10, 499, 500, 970, 999)
DEFAULT = (6, 0.8, 64)
OTHER = (2, 0.6, 16)  # one entry of the (dead) random_param table: a non-default parameter set
SEED_RANGE = 10**10  # newSeed: np.random.randint(-10**10, 10**10)


def load_reference(ref_root: Path):
    """src/utils/simplex_noise.py of the reference with a stand-in numba (its kernels then run as plain Python)."""
    numba = types.ModuleType("numba")
    numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    numba.prange = range
    sys.modules.setdefault("numba", numba)
    path = ref_root / "src" / "utils" / "simplex_noise.py"
    spec = importlib.util.spec_from_file_location("_reference_simplex_noise", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def slice_cases(rng):
    seeds = [-SEED_RANGE, SEED_RANGE - 1, -(2**63), 2**63 - 1]
    cases = []
    for hw in SIZES:
        for t in TIMESTEPS:
            seed = seeds.pop(0) if seeds else int(rng.integers(-SEED_RANGE, SEED_RANGE))
            cases.append((seed, t, hw, DEFAULT))
    cases.append((int(rng.integers(-SEED_RANGE, SEED_RANGE)), 500, (28, 28), OTHER))
    cases.append((int(rng.integers(-SEED_RANGE, SEED_RANGE)), 37, (16, 40), OTHER))
    return cases


def whole_call(ref, shape, t, np_seed):
    """generate_simplex_noise as the reference's trainers call it, recording the seeds its newSeed draws."""
    np.random.seed(np_seed)
    simplex = ref.Simplex_CLASS()
    drawn = []
    original = simplex.newSeed

    def recording_new_seed(seed=None):
        while not seed:  # newSeed draws again for a falsy seed
            seed = int(np.random.randint(-SEED_RANGE, SEED_RANGE))
        drawn.append(seed)
        original(seed)

    simplex.newSeed = recording_new_seed
    x = torch.zeros(shape)
    tt = torch.tensor(t, dtype=torch.int64)
    noise = ref.generate_simplex_noise(simplex, x=x, t=tt, in_channels=shape[1])
    assert len(drawn) == shape[0] * shape[1]
    return noise.numpy().astype(np.float32), np.array(drawn, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference", help="checkout of the reference project")
    ap.add_argument("--out", default=str(OUT))
    args = ap.parse_args()
    ref = load_reference(Path(args.reference))
    rng = np.random.default_rng(20261016)
    data = {}
    cases = slice_cases(rng)
    for k, (seed, t, (h, w), (octaves, persistence, frequency)) in enumerate(cases):
        simplex = ref.Simplex_CLASS()
        simplex.newSeed(seed)
        out = simplex.rand_3d_fixed_T_octaves((h, w), np.array([t], dtype=np.int64), octaves, persistence, frequency)
        assert out.shape == (1, h, w) and out.dtype == np.float64
        data[f"slice_{k}"] = out[0]
    data["slice_seed"] = np.array([c[0] for c in cases], dtype=np.int64)
    data["slice_t"] = np.array([c[1] for c in cases], dtype=np.int64)
    data["slice_hw"] = np.array([c[2] for c in cases], dtype=np.int64)
    data["slice_params"] = np.array([c[3] for c in cases], dtype=np.float64)
    for name, shape, t, np_seed in (("call2d", (3, 3, 16, 16), [0, 250, 999], 1), ("call3d", (2, 2, 4, 8, 8), [500, 7], 2)):
        noise, seeds = whole_call(ref, shape, t, np_seed)
        data[f"{name}_noise"] = noise
        data[f"{name}_t"] = np.array(t, dtype=np.int64)
        data[f"{name}_seeds"] = seeds
        data[f"{name}_shape"] = np.array(shape, dtype=np.int64)
    np.savez_compressed(args.out, **data)
    std = [float(data[f"slice_{k}"].std()) for k in range(len(cases))]
    print(f"wrote {args.out}: {len(cases)} slices (std {min(std):.3f} .. {max(std):.3f}), 2 whole calls")


if __name__ == "__main__":
    main()
