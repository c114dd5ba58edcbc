"""Close the latent-diffusion loop at toy size on synthetic blobs, as tools/train_synthetic.py does for pixel DDPMs: train a small
2-D VQ-VAE with the product trainer (L1 per epoch, final perplexity), then load its checkpoint through
``train_ddpm.py --vqvae_checkpoint`` for a --quick_test epoch and through ``reconstruct.py`` for one batch (development /
evidence tool; log kept under profiles/).

    python tools/train_vqvae_synthetic.py [--epochs 30] [--n_train 256] [--out /tmp/vqvae_synth]
                                          [--loss_terms perceptual,spectral] [--vqvae_only 1]

--loss_terms sets DDPM_VQVAE_LOSS_TERMS for the run (the perceptual and spectral terms of the generator loss); --vqvae_only 1
stops after the VQ-VAE (the with / without comparison of profiles/vqvae_training.md).
"""
import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--n_train", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--out", default="/tmp/vqvae_synth")
    ap.add_argument("--loss_terms", default=None, help="DDPM_VQVAE_LOSS_TERMS for this run (default: the environment's)")
    ap.add_argument("--vqvae_only", type=int, default=0)
    a = ap.parse_args()
    if a.loss_terms is not None:
        os.environ["DDPM_VQVAE_LOSS_TERMS"] = a.loss_terms
    import reconstruct as rcli
    import train_ddpm
    import train_vqvae
    from ddpm_ood_amd.train import DDPMTrainer
    from ddpm_ood_amd.trainer import Reconstruct
    from ddpm_ood_amd.vqvae_train import VQVAETrainer

    data = f"n={a.n_train}:size={a.size}"
    vargs = train_vqvae.parse_args([
        "--output_dir", a.out, "--model_name", "vqvae_synthetic", "--is_grayscale", "1", "--spatial_dimension", "2",
        "--training_ids", f"synthetic:blobs:{data}:seed=1", "--validation_ids", f"synthetic:blobs:n=32:size={a.size}:seed=10",
        "--vqvae_num_channels", "(32, 64)", "--vqvae_num_res_channels", "(32, 64)", "--vqvae_num_res_layers", "1",
        "--vqvae_downsample_parameters", "((2, 4, 1, 1), (2, 4, 1, 1))",
        "--vqvae_upsample_parameters", "((2, 4, 1, 1, 0), (2, 4, 1, 1, 0))", "--vqvae_num_embeddings", "64",
        "--vqvae_embedding_dim", "8", "--n_epochs", str(a.epochs), "--batch_size", str(a.batch), "--eval_freq", "10",
        "--checkpoint_every", "0"])
    t0 = time.time()
    tr = VQVAETrainer(vargs)
    tr.train(vargs)
    print(f"trained {a.epochs} epochs ({tr.last_stats['optimised_loss']}) in {time.time() - t0:.1f} s; L1 {tr.history[0][2]:.5f} -> "
          f"{tr.history[-1][2]:.5f}; final perplexity {tr.last_stats['perplexity']:.2f} of {vargs.vqvae_num_embeddings} codes; best epoch loss {tr.best_loss:.6f}")
    ckpt = str(Path(a.out) / "vqvae_synthetic" / "checkpoint.pth")
    del tr
    torch.cuda.empty_cache()
    if a.vqvae_only:
        return

    sched = ["--beta_schedule", "scaled_linear_beta", "--beta_start", "0.0015", "--beta_end", "0.0195"]
    common = ["--output_dir", a.out, "--model_name", "ldm_synthetic", "--is_grayscale", "1", "--vqvae_checkpoint", ckpt]
    targs = train_ddpm.parse_args(common + sched + [
        "--training_ids", f"synthetic:blobs:n=32:size={a.size}:seed=1", "--validation_ids", f"synthetic:blobs:n=32:size={a.size}:seed=10",
        "--n_epochs", "1", "--batch_size", "16", "--eval_freq", "1", "--checkpoint_every", "0", "--quick_test", "1"])
    dt = DDPMTrainer(targs)
    dt.train(targs)
    print(f"train_ddpm.py --vqvae_checkpoint: one --quick_test epoch on {dt.ddpm_channels}-channel latents, loss {dt.history[-1][1]:.5f}")
    del dt
    torch.cuda.empty_cache()
    rargs = rcli.parse_args(common + sched + [
        "--validation_ids", f"synthetic:blobs:n=16:size={a.size}:seed=10", "--in_ids", f"synthetic:blobs:n=16:size={a.size}:seed=11",
        "--out_ids", f"synthetic:noise:n=16:size={a.size}:seed=12:name=MNIST", "--inference_skip_factor", "32", "--batch_size", "16"])
    rec = Reconstruct(rargs)
    rec.reconstruct(rargs)
    print("reconstruct.py: one batch per set through the trained VQ-VAE and the quick-test latent DDPM")


if __name__ == "__main__":
    main()
