"""``Likelihood``: the trainer behind ``likelihood.py`` -- the model's own variational bound of every image of a dataset, the
likelihood baseline the reconstruction-based scores are compared against.

Set-up is ``BaseTrainer``'s (checkpoint, VQ-VAE or passthrough, latent pad, b_scale, SNR shift, the training
``DDPMScheduler``) and the datasets are ``Reconstruct``'s (``--validation_ids`` / ``--in_ids`` / ``--out_ids`` with the
``_vflip`` / ``_hflip`` variants).  What the bound sees is what training noises: ``encode_stage_2_inputs(images)`` (padded)
``* b_scale``.  The loop is ``DiffusionInferer.get_likelihood`` with ``--batch_size`` ROWS per UNet forward: a batch holds up
to that many images, and a smaller one packs several timesteps into each forward.  Images are sharded round-robin over the
ranks; every rank's [n, n_t] terms return through one all_gather and rank 0 writes.
"""

from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import torch
import torch.nn.functional as F

from . import _lib
from .data import get_data_loader
from .inferer import DiffusionInferer
from .sampling import gather_samples
from .trainer import BaseTrainer, dataset_stem


def likelihood_table(names, dataset_type: str, terms: np.ndarray) -> pd.DataFrame:
    """filename, type, nll, bpd of [N, n_t] per-timestep terms: nll = the float64 sum over t (nats per dimension),
    bpd = nll / ln 2."""
    nll = np.asarray(terms, dtype=np.float64).sum(axis=1)
    stems = [Path(n).stem.replace(".nii", "").replace(".gz", "") for n in names]
    return pd.DataFrame({"filename": stems, "type": dataset_type, "nll": nll, "bpd": nll / math.log(2.0)})


class Likelihood(BaseTrainer):
    def __init__(self, args):
        args.simplex_noise = 0  # (BaseTrainer reads it; the bound is defined for Gaussian noise)
        super().__init__(args)
        if not self.found_checkpoint:
            raise FileNotFoundError("Failed to find a saved model checkpoint.")
        self.out_dir = self.run_dir / "ood"
        if self.rank == 0:
            self.out_dir.mkdir(exist_ok=True)
        self.seed = int(args.seed)
        self.batch_size = int(args.batch_size)
        if self.batch_size < 1:
            raise ValueError("--batch_size must be positive")
        self.save_terms = bool(getattr(args, "save_terms", 0))
        if args.num_inference_steps is not None:
            self.scheduler.set_timesteps(int(args.num_inference_steps))
        self.timesteps = [int(t) for t in self.scheduler.timesteps]
        self.inferer = DiffusionInferer(self.scheduler)
        self._loader_args = dict(batch_size=self.batch_size, is_grayscale=bool(args.is_grayscale),
                                 image_size=self.image_size, drop_last=False, spatial_dimension=args.spatial_dimension,
                                 image_roi=args.image_roi, rank=self.rank, world=self.world)
        self.last_stats = {}

    def _loader(self, ids, first_n, **flips):
        return get_data_loader(ids, first_n=int(first_n) if first_n else first_n, **flips, **self._loader_args)

    @torch.no_grad()
    def get_terms(self, loader):
        """[N, n_t] fp32 terms of every image of the dataset (all ranks' shards, in image order) and their names."""
        self.model.eval()
        ids_all, terms_all = [], []
        _lib.status_read(clear=True)
        for batch in loader:
            images = batch["image"].to(self.device, non_blocking=True).float().contiguous()
            x0 = self.vqvae_model.encode_stage_2_inputs(images).float().contiguous()
            if self.do_latent_pad:
                x0 = F.pad(input=x0, pad=self.latent_pad, mode="constant", value=0)
            x0 = (x0 * self.b_scale).contiguous()
            _, terms = self.inferer.get_likelihood(x0, self.model, save_intermediates=True,
                                                   scaled_input_range=(0, self.b_scale), seed=self.seed,
                                                   row_ids=batch["index"], rows_per_forward=self.batch_size)
            word = _lib.status_read(clear=True)
            if word:
                print(f"WARNING: {_lib.status_text(word)} in the bound of images {batch['index'][0]} .. {batch['index'][-1]}: "
                      f"their terms are not finite", file=sys.__stderr__, flush=True)
                self.last_stats["batches_nonfinite"] = self.last_stats.get("batches_nonfinite", 0) + 1
            ids_all.extend(int(i) for i in batch["index"])
            terms_all.append(terms.t().to(torch.float32))  # (the terms are fp32 values: exact)
        n_t = len(self.timesteps)
        terms = torch.cat(terms_all, dim=0) if terms_all else torch.zeros((0, n_t), dtype=torch.float32)
        ids = torch.tensor(ids_all, dtype=torch.int64, device=self.device)
        n_total = len(loader.all_names)
        ids, terms = gather_samples(ids, terms.to(self.device), -(-n_total // self.world))
        assert ids.cpu().tolist() == list(range(n_total))
        return terms.cpu().numpy(), list(loader.all_names)

    def _write(self, loader, dataset_type: str, name: str) -> None:
        terms, names = self.get_terms(loader)
        if self.rank != 0:
            return
        likelihood_table(names, dataset_type, terms).to_csv(self.out_dir / f"likelihood_{name}.csv", index=False)
        if self.save_terms:
            np.save(self.out_dir / f"likelihood_terms_{name}.npy", terms)
        print(f"Wrote the bound of {terms.shape[0]} images over {terms.shape[1]} timesteps to likelihood_{name}.csv")

    def likelihood(self, args):
        if bool(args.run_val):
            self._write(self._loader(args.validation_ids, args.first_n_val), "val", "val")
        if bool(args.run_in):
            self._write(self._loader(args.in_ids, args.first_n), "in", "in")
        if bool(args.run_out):
            for out in args.out_ids.split(","):
                flips, suffix = {}, ""
                if "vflip" in out:
                    out, flips, suffix = out.replace("_vflip", ""), {"add_vflip": True}, "_vflip"
                elif "hflip" in out:
                    out, flips, suffix = out.replace("_hflip", ""), {"add_hflip": True}, "_hflip"
                self._write(self._loader(out, args.first_n, **flips), "out", dataset_stem(out) + suffix)
