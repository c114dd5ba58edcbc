"""CLI: draw samples from a trained DDPM (the counterpart of the sample grids the reference logs during validation).

Model flags as in train_ddpm.py / reconstruct.py (same names and defaults), plus what sampling needs:

    python sample.py --output_dir=... --model_name=fashionmnist --is_grayscale=1 --image_size=32 \
        --beta_schedule=scaled_linear_beta --beta_start=0.0015 --beta_end=0.0195 --num_samples=64
    python sample.py ... --scheduler=pndm --num_inference_steps=100      # deterministic PLMS, 10x fewer forwards
    torchrun --nproc_per_node=8 --master-addr 127.0.0.1 sample.py ...    # sample i on rank i % 8, rank 0 writes

Writes <out>/samples.npy ([N, C, ...] fp32 in [0, 1]) and <out>/samples.png (a tiled grid; for 3-D the slices at 0.25 / 0.5 /
0.75 of the last axis, one row per volume).  Sample i depends on (checkpoint, --seed, i) only -- not on --batch_size or on the
number of ranks.
"""

import argparse
import ast

# (flag, type, default, help)
_FLAGS = [
    ("seed", int, 2, "seed of the sampling noise"),
    ("output_dir", str, None, "root directory holding <model_name>/checkpoint.pth"),
    ("model_name", str, None, "run directory name"),
    ("spatial_dimension", int, 2, "2 or 3"),
    ("image_size", None, None, "extent of the images the model was trained on (required: no dataset is read)"),
    ("latent_pad", ast.literal_eval, None, "F.pad-style padding of the latent"),
    ("vqvae_checkpoint", None, None, "VQ-VAE checkpoint for latent diffusion"),
    ("ddpm_checkpoint_epoch", None, None, "use checkpoint_<epoch>.pth instead of checkpoint.pth"),
    ("prediction_type", None, "epsilon", "epsilon, v_prediction or sample"),
    ("model_type", None, "small", "small or big"),
    ("beta_schedule", None, "linear_beta", "linear[_beta] | scaled_linear[_beta] | sigmoid[_beta] | cosine"),
    ("beta_start", float, 1e-4, "first beta"),
    ("beta_end", float, 2e-2, "last beta"),
    ("b_scale", float, 1, "data scale the model was trained with (samples are divided by it)"),
    ("snr_shift", float, 1, "SNR shift factor of the schedule"),
    ("is_grayscale", int, 0, "1-channel data"),
]

_SAMPLING = [
    ("num_samples", int, 8, "how many samples to draw"),
    ("batch_size", int, 8, "samples per batch"),
    ("num_inference_steps", int, None, "steps of the sampler (default: 1000 for ddpm, 100 for pndm)"),
    ("out", str, None, "output directory (default: <output_dir>/<model_name>/samples)"),
    ("use_proj_attn", int, 0, "1: apply AttentionBlock.proj_attn (as reconstruct.py)"),
    ("verbose", int, 0, "1: print progress every 100 steps"),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default, text in _FLAGS:
        kw = {"default": default, "help": text}
        if typ not in (None, str):
            kw["type"] = typ
        parser.add_argument(f"--{name}", **kw)
    grp = parser.add_argument_group("sampling")
    for name, typ, default, text in _SAMPLING:
        grp.add_argument(f"--{name}", type=typ, default=default, help=text)
    grp.add_argument("--scheduler", default="ddpm", choices=["ddpm", "pndm"],
                     help="ddpm: ancestral sampling (stochastic); pndm: PLMS (deterministic given the initial noise)")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    import torch.distributed as dist

    from ddpm_ood_amd.sampling import Sampler

    try:
        Sampler(args).sample()
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
