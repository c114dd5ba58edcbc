"""CLI of the likelihood baseline: the DDPM variational bound of every image under the trained model.

Model and dataset flags are reconstruct.py's (same names, types and defaults: its parser is reused), so the launch line of a
reconstruction run scores the same sets by likelihood:

    python likelihood.py --output_dir=... --model_name=fashionmnist --validation_ids=... \
        --in_ids=... --out_ids=a.csv,b_vflip.csv --is_grayscale=1 \
        --beta_schedule=scaled_linear_beta --beta_start=0.0015 --beta_end=0.0195 --batch_size=1024
    torchrun --nproc_per_node=8 --master-addr 127.0.0.1 likelihood.py ...     # images sharded over the ranks, rank 0 writes

Writes <output_dir>/<model_name>/ood/likelihood_{val,in,<name>}.csv with the columns filename,type,nll,bpd (nll: the bound in
nats per dimension, summed over the timesteps; bpd = nll / ln 2) -- `ood_detection.py --score likelihood` reads them.  The
results_*.csv files of reconstruct.py are not touched.  An image's row depends on (checkpoint, --seed, its index) only, up to the
UNet's batch-dependent rounding -- not on --batch_size or on the number of ranks.
"""

import reconstruct

# flags whose meaning differs from reconstruct.py's: (flag, new default, help)
_OVERRIDES = [
    ("seed", 2, "seed of the per-image noise (one noise per image, shared by all timesteps)"),
    ("batch_size", 256, "ROWS per UNet forward: up to this many images per batch, and the timesteps of a smaller batch are "
                        "packed to fill it"),
    ("num_inference_steps", None, "evaluate the bound on this many strided timesteps (default: all 1000)"),
]


def build_parser():
    parser = reconstruct.build_parser()
    parser.description = __doc__
    for name, default, text in _OVERRIDES:
        action = next(a for a in parser._actions if a.dest == name)
        action.default, action.help = default, text
    grp = parser.add_argument_group("likelihood")
    grp.add_argument("--save_terms", type=int, default=0,
                     help="1: also write likelihood_terms_<name>.npy, the [N, n_t] per-timestep terms")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    import torch.distributed as dist

    from ddpm_ood_amd.likelihood import Likelihood

    try:
        Likelihood(args).likelihood(args)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
