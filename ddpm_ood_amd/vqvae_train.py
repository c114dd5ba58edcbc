"""VQ-VAE training: the stage-1 checkpoint of the latent-diffusion configuration (``train_vqvae.py``).

Mirrors the reference's src/trainers/vqvae_trainer.py (model from the ``vqvae_*`` flags, ``vqvae_config.json`` with its 15 keys,
Adam at ``--vqvae_learning_rate``, epoch loop, five-key checkpoint dict, resume, ``best_loss = 1000``, ``--checkpoint_every``,
``--eval_freq``, ``--quick_test``).  What runs where:
  * the quantiser's training step -- nearest-code search, per-code counts and sums, EMA codebook update, commitment loss and
    its straight-through backward -- is HIP (``vq.hip``: ddpm_vq_train_{assign,update,backward}_f32) behind ``VQTrainFunction``;
  * the encoder / decoder gradients go by default through PyTorch-ROCm autograd over ``encode_train`` / ``decode_train``: a
    differentiable ATen forward that evaluates the SAME parameter holders the HIP engine of ``vqvae.VQVAE`` reads.
    ``DDPM_VQVAE_NATIVE=1`` runs them on the library instead (``vqvae_native.py``): forward on the eval path's
    kernels, backward on the weight-gradient kernels (3x3 / 3x3x3 and k4 s2 p1) and the inference kernels as input-gradient
    convolutions; ``last_stats["conv_gradients"]`` says which route a step took;
  * the optimised loss is L1 + quantisation (commitment) loss by default.  ``DDPM_VQVAE_LOSS_TERMS`` (a comma list drawn from
    ``perceptual``, ``spectral``; unknown names raise) adds the reference's 0.001 x LPIPS-AlexNet term and its Jukebox spectral
    term, forward and backward on HIP kernels (``loss_terms.py``); ``DDPM_LPIPS_WEIGHTS=<state_dict file>`` loads
    trained LPIPS weights (without it the seeded ones are used and a loud warning says so).  The least-squares patch-adversarial
    loss and its discriminator are NOT built: ``--adversarial_weight`` / ``--adversarial_warmup`` are accepted, one loud warning
    names what is still missing, ``last_stats["missing_loss_terms"]`` records it.
Training never goes through ``VQVAE.forward`` or ``self.training`` (a fresh module has training=True and callers of the eval path
do not always call .eval()): ``vqvae_forward_train`` is the training forward.
Quirks of the reference: KEPT ``epoch_loss = sum of batch-mean losses / number of images`` (it picks the "best"
checkpoint), ``global_step += batch size``, ``--vqvae_ddp_sync type=bool`` (any non-empty string is True); FIXED (Q23): the
reference saves and restores a second, never-stepped optimiser (lr 2.5e-5) under ``optimizer_state_dict`` -- here it is the
optimiser that steps, so a resumed run keeps its moments.
"""

from __future__ import annotations

import json
import os
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib, loss_terms, ops, vqvae_native
from .data import get_data_loader
from .perceptual import LPIPS
from .vqvae import VQVAE, _ResidualUnit

MISSING_LOSS_TERMS = ("perceptual (0.001 x LPIPS)", "Jukebox spectral", "patch-adversarial (and its discriminator)")
CONFIG_KEYS = ("spatial_dims", "in_channels", "out_channels", "num_res_layers", "downsample_parameters", "upsample_parameters",
               "num_channels", "num_res_channels", "num_embeddings", "embedding_dim", "decay", "commitment_cost", "epsilon",
               "dropout", "ddp_sync")
_TERM_OF_MISSING = ("perceptual", "spectral", None)  # the loss_terms name that builds MISSING_LOSS_TERMS[i]
_WARNED = set()


def _loss_text(head: str, terms, times: str = "") -> str:
    return head + "".join({"perceptual": f" + 0.001 {times}perceptual", "spectral": " + spectral"}[t] for t in terms)


def _all_reduce(flat: torch.Tensor) -> None:
    if dist.get_backend() == "gloo" and flat.is_cuda:  # test hook: two ranks on one GPU (see trainer.BaseTrainer)
        host = flat.cpu()
        dist.all_reduce(host)
        flat.copy_(host)
    else:
        dist.all_reduce(flat)  # RCCL over xGMI: one collective


def _distributed() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


# ---- the quantiser's training step ---------------------------------------------------------------------------------------

class VQTrainFunction(torch.autograd.Function):
    """EMAQuantizer.forward in training mode over the three HIP entry points.  forward: (x [B, D, *S], quantizer holder,
    update_codebook) -> (x + (e_idx - x), commitment loss, idx int32, local counts [K]); the EMA update runs here, without a
    graph, as the package runs it under no_grad -- after the search, so outputs and loss belong to the codebook as it was.
    backward: dx = dout + 2 commitment_cost / numel (x - e_idx) dloss (straight-through + commitment)."""

    @staticmethod
    def forward(ctx, x, quantizer, update_codebook):
        x = x.float().contiguous()
        e = quantizer.embedding.weight.data
        cc = float(quantizer.commitment_cost)
        idx, out, counts, dw, loss, sums = ops.vq_train_assign(x, e, cc)
        local_counts = counts
        if update_codebook:
            searched = e.clone()  # the backward needs the codes the search saw; the update below moves them in place
            if quantizer.ddp_sync and _distributed():
                local_counts = counts.clone()
                _all_reduce(sums)  # counts and dw of every rank: ONE collective of K (D + 1) floats
            ops.vq_train_update(quantizer.ema_cluster_size, quantizer.ema_w, e, counts, dw, float(quantizer.decay),
                                float(quantizer.epsilon))
        else:
            searched = e
        ctx.save_for_backward(x, idx, searched)
        ctx.cc = cc
        ctx.mark_non_differentiable(idx, local_counts)
        return out, loss, idx, local_counts

    @staticmethod
    def backward(ctx, dout, dloss, _didx, _dcounts):
        x, idx, e = ctx.saved_tensors
        dout = None if dout is None else dout.float().contiguous()
        dloss = None if dloss is None else dloss.float().contiguous()
        return ops.vq_train_backward(dout, x, e, idx, dloss, ctx.cc), None, None


# ---- differentiable forward over the parameter holders ---------------------------------------------------------------------

def _conv_train(layer, x):
    c = layer.conv
    sd = c.weight.ndim - 2
    if layer.is_transposed:
        f = F.conv_transpose2d if sd == 2 else F.conv_transpose3d
        y = f(x, c.weight, c.bias, stride=c.stride, padding=c.padding, output_padding=c.output_padding, dilation=c.dilation)
    else:
        f = F.conv2d if sd == 2 else F.conv3d
        y = f(x, c.weight, c.bias, stride=c.stride, padding=c.padding, dilation=c.dilation)
    return y if layer.conv_only else F.relu(y)


def _stack_train(stack, x):
    for blk in stack.blocks:
        if isinstance(blk, _ResidualUnit):
            x = F.relu(x + _conv_train(blk.conv2, _conv_train(blk.conv1, x)))
        else:
            x = _conv_train(blk, x)
    return x


def native_conv_gradients() -> bool:
    """DDPM_VQVAE_NATIVE=1: the encoder / decoder run forward on the eval path's HIP kernels and backward on the library's
    weight- and input-gradient kernels (``vqvae_native``).  Unset or 0: the ATen route above.  Read per call."""
    return os.environ.get("DDPM_VQVAE_NATIVE", "0") not in ("", "0")


def _check_trainable(model):
    if getattr(model, "dropout", 0.0):
        raise NotImplementedError(f"vqvae_dropout = {model.dropout}: dropout is not built (the reference trains with 0.0)")


def encode_train(model: VQVAE, images: torch.Tensor) -> torch.Tensor:
    """``model.encode`` with autograd over the model's own parameters: ATen ops (any device, 2-D or 3-D), or -- DDPM_VQVAE_NATIVE=1 --
    the eval path's HIP kernels with a native backward (device only)."""
    _check_trainable(model)
    if native_conv_gradients():
        return vqvae_native.stack_train(model.encoder, images)
    return _stack_train(model.encoder, images.float())


def decode_train(model: VQVAE, quantizations: torch.Tensor) -> torch.Tensor:
    """``model.decode`` with autograd over the model's own parameters: ATen ops, or the HIP kernels (see ``encode_train``)."""
    _check_trainable(model)
    if native_conv_gradients():
        return vqvae_native.stack_train(model.decoder, quantizations)
    return _stack_train(model.decoder, quantizations.float())


def vqvae_forward_train(model: VQVAE, images: torch.Tensor, update_codebook: bool = True):
    """The training forward: (reconstruction, quantization_loss), differentiable w.r.t. the encoder / decoder parameters; the
    codebook and its two EMA buffers move in place when ``update_codebook`` (never through a gradient).  Sets
    ``model.quantizer.perplexity = exp(-sum p log(p + 1e-10))`` from this batch's code counts.  The quantiser op is device-only."""
    z = encode_train(model, images)
    q, loss, _idx, counts = VQTrainFunction.apply(z, model.quantizer.quantizer, bool(update_codebook))
    with torch.no_grad():
        p = counts / counts.sum()
        model.quantizer.perplexity = torch.exp(-torch.sum(p * torch.log(p + 1e-10)))
    return decode_train(model, q), loss


def epoch_loss_of(batch_losses, batch_sizes) -> float:
    """The reference's epoch loss (vqvae_trainer.py: generator_epoch_loss / epoch_step): the SUM of the batch-mean losses over the
    NUMBER OF IMAGES -- not a mean of anything (it shrinks with the batch size), kept because it decides which checkpoint is
    "best" against ``best_loss = 1000``."""
    return sum(batch_losses) / max(sum(batch_sizes), 1)


# ---- the trainer ------------------------------------------------------------------------------------------------------------

class VQVAETrainer:
    def __init__(self, args):
        if not torch.cuda.is_available():
            raise RuntimeError("No ROCm device visible: the quantiser's training step is HIP and has no CPU fallback")
        _lib.load()
        if "LOCAL_RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
            print("Setting up DDP.")
            self.ddp = True
            local_rank = int(os.environ["LOCAL_RANK"])
            if local_rank != 0:
                sys.stdout = sys.stderr = open(os.devnull, "w")
            if not dist.is_initialized():
                dist.init_process_group(backend=os.environ.get("DDPM_DIST_BACKEND", "nccl"), init_method="env://")
            shared = os.environ.get("DDPM_DIST_SHARED_DEVICE", "0") == "1"
            self.device = torch.device("cuda:0" if shared else f"cuda:{local_rank}")
        else:
            self.ddp = False
            self.device = torch.device("cuda:0")
        torch.cuda.set_device(self.device)
        self.rank = dist.get_rank() if self.ddp else 0
        self.world = dist.get_world_size() if self.ddp else 1

        print(f"Arguments: {str(args)}")
        for k, v in vars(args).items():
            print(f"  {k}: {v}")

        self.spatial_dimension = args.spatial_dimension
        vqvae_args = {
            "spatial_dims": args.spatial_dimension, "in_channels": args.vqvae_in_channels,
            "out_channels": args.vqvae_out_channels, "num_res_layers": args.vqvae_num_res_layers,
            "downsample_parameters": args.vqvae_downsample_parameters, "upsample_parameters": args.vqvae_upsample_parameters,
            "num_channels": args.vqvae_num_channels, "num_res_channels": args.vqvae_num_res_channels,
            "num_embeddings": args.vqvae_num_embeddings, "embedding_dim": args.vqvae_embedding_dim, "decay": args.vqvae_decay,
            "commitment_cost": args.vqvae_commitment_cost, "epsilon": args.vqvae_epsilon, "dropout": args.vqvae_dropout,
            "ddp_sync": args.vqvae_ddp_sync,
        }
        assert tuple(vqvae_args) == CONFIG_KEYS
        if args.vqvae_dropout:
            raise NotImplementedError(f"--vqvae_dropout {args.vqvae_dropout}: dropout is not built (the reference trains with 0.0)")
        torch.manual_seed(int(args.seed))
        self.model = VQVAE(**vqvae_args).to(self.device)
        print(f"{sum(p.numel() for p in self.model.parameters()):,} model parameters")

        self.adv_weight = args.adversarial_weight
        self.adversarial_warmup = bool(args.adversarial_warmup)
        self.loss_terms = loss_terms.parse_terms(os.environ.get("DDPM_VQVAE_LOSS_TERMS"))
        missing = [m for m, t in zip(MISSING_LOSS_TERMS, _TERM_OF_MISSING) if t not in self.loss_terms]
        self.last_stats = {"missing_loss_terms": missing, "optimised_loss": _loss_text("l1 + quantization", self.loss_terms)}
        self.last_stats["conv_gradients"] = "native" if native_conv_gradients() else "aten"
        self.last_terms = {}
        if "missing_terms" not in _WARNED:
            _WARNED.add("missing_terms")
            what = _loss_text("L1 + quantisation", self.loss_terms, "x ") + (" loss" if self.loss_terms else " loss ONLY")
            print(f"WARNING: this VQ-VAE trainer optimises {what}.  NOT built: " + "; ".join(missing)
                  + f".  --adversarial_weight {self.adv_weight} / --adversarial_warmup {int(self.adversarial_warmup)} are accepted "
                  "and have no effect; a checkpoint trained here is not the reference's recipe.", file=sys.stderr, flush=True)
        self.lpips = None
        if "perceptual" in self.loss_terms:
            self.lpips = LPIPS().to(self.device)
            weights = os.environ.get("DDPM_LPIPS_WEIGHTS")
            if weights:
                sd = torch.load(weights, map_location="cpu", weights_only=True)
                self.lpips.load_pretrained_state_dict(sd.get("state_dict", sd) if isinstance(sd, dict) else sd)
                self.lpips.to(self.device)
                print(f"Loaded LPIPS weights from {weights}.")
            elif "lpips_weights" not in _WARNED:
                _WARNED.add("lpips_weights")
                print("WARNING: DDPM_LPIPS_WEIGHTS is not set: the perceptual term runs on SEEDED SYNTHETIC LPIPS-AlexNet weights "
                      "(the trained ones need the network).  It is then NOT the reference's perceptual loss: the arithmetic is, "
                      "the metric is not.", file=sys.stderr, flush=True)
            self.last_stats["lpips_pretrained"] = bool(self.lpips.pretrained)

        # embedding.weight is moved by the EMA update only: no gradient, not an optimiser parameter
        codebook = self.model.quantizer.quantizer.embedding.weight
        codebook.requires_grad_(False)
        self.params = [p for p in self.model.parameters() if p is not codebook]
        for p in self.params:
            p.requires_grad_(True)
        self.optimizer = torch.optim.Adam(params=self.params, lr=args.vqvae_learning_rate)

        self.run_dir = Path(args.output_dir) / args.model_name
        checkpoint_path = self.run_dir / "checkpoint.pth"
        if checkpoint_path.exists():
            checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
            self.start_epoch = checkpoint["epoch"] + 1
            self.global_step = checkpoint["global_step"]
            self.model.load_state_dict(checkpoint["model_state_dict"])
            self.best_loss = checkpoint["best_loss"]
            self.optimizer.load_state_dict(checkpoint["optimizer_state_dict"])  # the optimiser that steps (Q23)
            print(f"Resuming training using checkpoint {checkpoint_path} at epoch {self.start_epoch}")
        else:
            self.start_epoch, self.best_loss, self.global_step = 0, 1000, 0
        self._broadcast_initial_state()

        if self.rank == 0:
            self.run_dir.mkdir(parents=True, exist_ok=True)
            with open(self.run_dir / "vqvae_config.json", "w") as f:
                json.dump(vqvae_args, f, indent=4)

        if args.quick_test:
            print("Quick test enabled, only running on a single train and eval batch.")
        self.quick_test = bool(args.quick_test)
        self.num_epochs = args.n_epochs
        self.seed = int(args.seed)
        # --augmentation / --cache_data / --num_workers are accepted and have no effect, as in train.DDPMTrainer
        kw = dict(batch_size=args.batch_size, is_grayscale=bool(args.is_grayscale),
                  image_size=int(args.image_size) if args.image_size else args.image_size,
                  spatial_dimension=args.spatial_dimension, image_roi=args.image_roi)
        self.train_loader = get_data_loader(args.training_ids, rank=self.rank, world=self.world, **kw)
        self.val_loader = get_data_loader(args.validation_ids, rank=self.rank, world=self.world, **kw)
        self.history = []  # (epoch, epoch loss, mean L1)
        self._epoch = self._step = 0  # what the 2.5-D perceptual term's slice draw is seeded with, beside the seed
        if self.lpips is not None:
            src = self.train_loader.images
            first = src[0] if len(src) else None
            if first is not None and min(first.shape[1:]) < loss_terms.MIN_LPIPS_SIZE:
                raise ValueError(f"DDPM_VQVAE_LOSS_TERMS=perceptual needs spatial sizes >= {loss_terms.MIN_LPIPS_SIZE} (AlexNet's "
                                 f"second max-pool is empty below), the training images are {tuple(first.shape[1:])}")

    def _broadcast_initial_state(self):
        """Every rank starts from rank 0's parameters and buffers (DistributedDataParallel's constructor in the reference)."""
        if not self.ddp:
            return
        tensors = [p.data for p in self.model.parameters()] + [b.data for b in self.model.buffers()]
        flat = torch.cat([t.reshape(-1).float() for t in tensors])
        if dist.get_backend() == "gloo" and flat.is_cuda:
            host = flat.cpu()
            dist.broadcast(host, src=0)
            flat.copy_(host)
        else:
            dist.broadcast(flat, src=0)
        off = 0
        for t in tensors:
            t.copy_(flat[off: off + t.numel()].view_as(t))
            off += t.numel()

    def _sync_grads(self):
        """ONE flat all_reduce of every gradient per step (train.DDPMTrainer._sync_grads), averaged over ranks."""
        if not self.ddp:
            return
        grads = [p.grad for p in self.params if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        _all_reduce(flat)
        flat /= self.world
        off = 0
        for g in grads:
            g.copy_(flat[off: off + g.numel()].view_as(g))
            off += g.numel()

    def extra_terms(self, reconstruction: torch.Tensor, images: torch.Tensor):
        """The enabled terms of DDPM_VQVAE_LOSS_TERMS as the generator loss adds them: (their weighted sum or None, {name: the
        unweighted value as a detached device scalar}).  Local to this rank's batch: the flat-gradient all_reduce carries them."""
        total, values = None, {}
        for name in self.loss_terms:
            if name == "perceptual":
                idx = None
                if self.spatial_dimension == 3:
                    idx = loss_terms.fake3d_slice_indices(images.shape, self.seed + self.rank, self._epoch, self._step)
                v = loss_terms.perceptual_term(self.lpips, reconstruction.float(), images.float(), self.spatial_dimension, idx)
                w = loss_terms.PERCEPTUAL_WEIGHT
            else:
                v = loss_terms.spectral_term(reconstruction.float(), images.float())
                w = loss_terms.SPECTRAL_WEIGHT
            values[name] = v.detach()
            total = w * v if total is None else total + w * v
        return total, values

    def train_step(self, images: torch.Tensor):
        """One optimisation step on a device batch -> (total loss, L1, quantisation loss) as device scalars; the values of the
        enabled extra terms (unweighted) go to ``self.last_terms``."""
        self.optimizer.zero_grad(set_to_none=True)
        self.last_stats["conv_gradients"] = "native" if native_conv_gradients() else "aten"
        reconstruction, quantization_loss = vqvae_forward_train(self.model, images, update_codebook=True)
        recons_loss = F.l1_loss(reconstruction.float(), images.float())
        total = recons_loss + quantization_loss
        if self.loss_terms:
            extra, self.last_terms = self.extra_terms(reconstruction, images)
            total = total + extra
        total.backward()
        self._sync_grads()
        self.optimizer.step()
        self._step += 1
        return total.detach(), recons_loss.detach(), quantization_loss.detach()

    def train_epoch(self, epoch: int) -> float:
        n_local = len(self.train_loader.names)
        order = torch.randperm(n_local, generator=torch.Generator().manual_seed(self.seed + epoch))
        if self.ddp:  # equal step counts on every rank: the short shards wrap around (a missing all_reduce would hang the job)
            n_all = len(getattr(self.train_loader, "all_names", self.train_loader.names))
            n_even = -(-n_all // self.world)
            if n_local == 0:
                raise ValueError(f"rank {self.rank}: empty training shard ({n_all} images over {self.world} ranks)")
            if n_local < n_even:
                order = torch.cat([order, order[: n_even - n_local]])
        bs = self.train_loader.batch_size
        src = self.train_loader.images
        losses, l1s, sizes = [], [], []
        terms = {t: [] for t in self.loss_terms}
        self._epoch, self._step = epoch, 0
        t0 = time.time()
        for s in range(0, len(order), bs):
            idx = order[s: s + bs]
            images = (src[idx] if torch.is_tensor(src) else torch.stack([src[int(i)] for i in idx])).to(self.device)
            total, l1, _q = self.train_step(images)
            losses.append(total.item())
            l1s.append(l1.item())
            for t in terms:
                terms[t].append(self.last_terms[t].item())
            sizes.append(images.shape[0])
            self.global_step += images.shape[0]
            if self.quick_test:
                break
        epoch_loss = epoch_loss_of(losses, sizes)
        mean_l1 = sum(l1s) / max(len(l1s), 1)
        perplexity = float(self.model.quantizer.perplexity)
        self.last_stats.update(epoch=epoch, epoch_loss=epoch_loss, l1=mean_l1, perplexity=perplexity)
        self.history.append((epoch, epoch_loss, mean_l1))
        extra = ""
        for t, vals in terms.items():
            self.last_stats[t] = sum(vals) / max(len(vals), 1)
            extra += f", {t} {self.last_stats[t]:.6f}"
        print(f"Epoch {epoch}: loss {epoch_loss:.6f} (sum of batch means / images), L1 {mean_l1:.6f}{extra}, perplexity "
              f"{perplexity:.2f} ({time.time() - t0:.1f} s)")
        return epoch_loss

    @torch.no_grad()
    def val_epoch(self, epoch: int) -> float:
        tot, n = 0.0, 0
        for batch in self.val_loader:
            images = batch["image"].to(self.device)
            reconstruction, quantization_loss = vqvae_forward_train(self.model, images, update_codebook=False)
            loss = F.l1_loss(reconstruction.float(), images.float()) + quantization_loss
            if self.loss_terms:  # the reference validates on the generator loss
                self._step = n
                loss = loss + self.extra_terms(reconstruction, images)[0]
            tot += loss.item()
            n += 1
            if self.quick_test:
                break
        val = tot / max(n, 1)
        self.last_stats["val_loss"] = val
        print(f"Validation {epoch}: {_loss_text('L1 + quantisation', self.loss_terms)} loss {val:.6f}")
        return val

    def save_checkpoint(self, path, epoch, save_message=None):
        if self.rank != 0:
            return
        checkpoint = {"epoch": epoch + 1,  # save epoch + 1, so we resume on the next epoch
                      "global_step": self.global_step, "model_state_dict": self.model.state_dict(),
                      "optimizer_state_dict": self.optimizer.state_dict(), "best_loss": self.best_loss}
        print(save_message)
        torch.save(checkpoint, path)

    def train(self, args):
        for epoch in range(self.start_epoch, self.num_epochs):
            epoch_loss = self.train_epoch(epoch)
            if epoch_loss < self.best_loss:
                self.best_loss = epoch_loss
                self.save_checkpoint(self.run_dir / "checkpoint.pth", epoch,
                                     save_message=f"Saving checkpoint for model with loss {self.best_loss}")
            if args.checkpoint_every != 0 and (epoch + 1) % args.checkpoint_every == 0:
                self.save_checkpoint(self.run_dir / f"checkpoint_{epoch + 1}.pth", epoch,
                                     save_message=f"Saving checkpoint at epoch {epoch + 1}")
            if (epoch + 1) % args.eval_freq == 0:
                self.val_epoch(epoch)
        print("Training completed.")
        if self.ddp:
            dist.destroy_process_group()
