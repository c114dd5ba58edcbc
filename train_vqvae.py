"""CLI of the VQ-VAE training loop (stage 1 of the latent-diffusion configuration): flag names, types and defaults of the
reference's train_vqvae.py, so the README's command keeps working.

    python train_vqvae.py --output_dir=... --model_name=vqvae_decathlon --training_ids=... --validation_ids=... \
        --is_grayscale=1 --n_epochs=300 --batch_size=8 --eval_freq=10 --cache_data=0 --spatial_dimension=3 --image_roi=[160,160,128] \
        --image_size=128 --vqvae_num_embeddings=2048 --vqvae_embedding_dim=128
    torchrun --nproc_per_node=8 --master-addr 127.0.0.1 train_vqvae.py ...   # one rank per MI355X

The optimised loss is L1 + quantisation loss; DDPM_VQVAE_LOSS_TERMS=perceptual,spectral (environment, no flag) adds the
reference's 0.001 x LPIPS and Jukebox spectral terms on HIP kernels, DDPM_LPIPS_WEIGHTS=<state_dict file> loads trained LPIPS
weights.  --adversarial_weight / --adversarial_warmup are accepted, and the trainer says loudly which of the reference's loss
terms are not built (ddpm_ood_amd/vqvae_train.py).
"""

import argparse
import ast

_FLAGS = [
    ("seed", int, 2), ("output_dir", str, None), ("model_name", str, None), ("training_ids", str, None),
    ("validation_ids", str, None), ("spatial_dimension", int, 3), ("image_size", None, None),
    ("image_roi", ast.literal_eval, None),
    # model
    ("vqvae_in_channels", int, 1), ("vqvae_out_channels", int, 1), ("vqvae_num_res_layers", int, 3),
    ("vqvae_downsample_parameters", ast.literal_eval, ((2, 4, 1, 1), (2, 4, 1, 1), (2, 4, 1, 1), (2, 4, 1, 1))),
    ("vqvae_upsample_parameters", ast.literal_eval, ((2, 4, 1, 1, 0), (2, 4, 1, 1, 0), (2, 4, 1, 1, 0), (2, 4, 1, 1, 0))),
    ("vqvae_num_channels", ast.literal_eval, [128, 128, 128, 256]),
    ("vqvae_num_res_channels", ast.literal_eval, [128, 128, 128, 256]),
    ("vqvae_num_embeddings", int, 256), ("vqvae_embedding_dim", int, 256), ("vqvae_decay", float, 0.99),
    ("vqvae_commitment_cost", float, 0.25), ("vqvae_epsilon", float, 1e-5), ("vqvae_dropout", float, 0.0),
    ("vqvae_ddp_sync", bool, True),  # type=bool as in the reference: any non-empty string is True
    ("vqvae_learning_rate", float, 3e-4),
    # training
    ("batch_size", int, 4), ("n_epochs", int, 300), ("eval_freq", int, 10), ("augmentation", int, 1),
    ("adversarial_weight", float, 0.01), ("adversarial_warmup", int, 0), ("num_workers", int, 8), ("cache_data", int, 1),
    ("checkpoint_every", int, 100), ("is_grayscale", int, 0), ("quick_test", int, 0),
]


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, typ, default in _FLAGS:
        kw = {"default": default}
        if typ not in (None, str):
            kw["type"] = typ
        parser.add_argument(f"--{name}", **kw)
    return parser.parse_args(argv)


if __name__ == "__main__":
    args = parse_args()
    from ddpm_ood_amd.vqvae_train import VQVAETrainer

    trainer = VQVAETrainer(args)
    trainer.train(args)
