"""-m gpu: VQ-VAE training end to end -- the differentiable forward against the HIP eval path and against float64 autograd over
the oracle's layers, the CLI and its checkpoint, the checkpoint through the existing --vqvae_checkpoint path, training progress,
the missing-terms warning, two ranks.  Everything on synthetic blobs: a 2-D VQ-VAE with num_channels (8, 16), two down-levels,
K = 16 codes of D = 8, 16 images of 16 x 16."""

import argparse
import json
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

CFG = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(8, 16), num_res_layers=1, num_res_channels=(8, 16),
           downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1)), upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0)),
           num_embeddings=16, embedding_dim=8, decay=0.99, commitment_cost=0.25, epsilon=1e-5)
CONFIG_KEYS = {"spatial_dims", "in_channels", "out_channels", "num_res_layers", "downsample_parameters", "upsample_parameters",
               "num_channels", "num_res_channels", "num_embeddings", "embedding_dim", "decay", "commitment_cost", "epsilon",
               "dropout", "ddp_sync"}
CLI = ["--spatial_dimension", "2", "--is_grayscale", "1", "--vqvae_num_channels", "(8, 16)", "--vqvae_num_res_channels", "(8, 16)",
       "--vqvae_num_res_layers", "1", "--vqvae_downsample_parameters", "((2, 4, 1, 1), (2, 4, 1, 1))",
       "--vqvae_upsample_parameters", "((2, 4, 1, 1, 0), (2, 4, 1, 1, 0))", "--vqvae_num_embeddings", "16",
       "--vqvae_embedding_dim", "8", "--training_ids", "synthetic:blobs:n=16:size=16:seed=1",
       "--validation_ids", "synthetic:blobs:n=16:size=16:seed=2", "--batch_size", "16"]
PROGRESS_STEPS = 20  # chosen on an MI355X: L1 on the fixed batch falls from step 0 on (figures in profiles/vqvae_training.md)


def _images():
    from ddpm_ood_amd.data import synthetic_images

    return synthetic_images("blobs", 16, 1, 16, seed=1)


def _args(tmp_path, name="vq", **over):
    import train_vqvae

    a = train_vqvae.parse_args(CLI + ["--output_dir", str(tmp_path), "--model_name", name])
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.fixture(scope="module")
def pair(device):
    """(oracle VQ-VAE on the host, product VQ-VAE on the device) with the same weights; the codebook spread over the latents' range
    so that more than one code is in use."""
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.vqvae import VQVAE

    torch.manual_seed(11)
    o = OV(**CFG).eval()
    with torch.no_grad():
        z = o.encode(_images())
        o.quantizer.quantizer.embedding.weight.mul_(z.std()).add_(z.mean(dim=(0, 2, 3))[None])
        o.quantizer.quantizer.ema_w.copy_(o.quantizer.quantizer.embedding.weight)
    m = VQVAE(**CFG)
    m.load_state_dict(o.state_dict())
    return o, m.to(device)


def _gaps(z: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    """relative gap between the two nearest codes per latent position, float64 -> [B, *S]"""
    flat = z.detach().cpu().double().movedim(1, -1).reshape(-1, z.shape[1])
    E = E.detach().cpu().double()
    d = (flat * flat).sum(1, keepdim=True) - 2.0 * flat @ E.t() + (E * E).sum(1)[None]
    b = torch.topk(d, 2, dim=1, largest=False).values
    return ((b[:, 1] - b[:, 0]) / b[:, 0].abs().clamp_min(1e-12)).reshape(z.shape[0], *z.shape[2:])


def test_training_forward_matches_the_hip_eval_path(device, pair):
    """vqvae_forward_train(update_codebook=False) under no_grad against model(images) on the HIP kernels, at the bound
    tests/test_gpu_ops.py / test_gpu_configs.py hold the VQ-VAE to against the oracle (1e-5 on latents, 2e-5 on reconstructions,
    relative to 1 + max |ref|); where no code flips the indices are equal."""
    from ddpm_ood_amd.vqvae_train import VQTrainFunction, encode_train, vqvae_forward_train

    _, m = pair
    x = _images().to(device)
    q = m.quantizer.quantizer
    state = [t.clone() for t in (q.embedding.weight.data, q.ema_cluster_size, q.ema_w)]
    with torch.no_grad():
        r_hip, zero = m(x)
        z_hip = m.encode(x)
        idx_hip = m.index_quantize(x)
        z_t = encode_train(m, x)
        _, qloss, idx_t, counts = VQTrainFunction.apply(z_t, q, False)
        r_t, qloss2 = vqvae_forward_train(m, x, update_codebook=False)
    for a, b in zip(state, (q.embedding.weight.data, q.ema_cluster_size, q.ema_w)):
        assert torch.equal(a, b)
    assert float(zero) == 0.0 and float(qloss) > 0 and torch.equal(qloss, qloss2)
    assert (z_t - z_hip).abs().max().item() <= 1e-5 * (1 + z_hip.abs().max().item())
    safe = _gaps(z_hip, q.embedding.weight) > 1e-4  # positions that are not near-ties: no flip possible at 1e-5 latent error
    assert bool(safe.any()) and torch.equal(idx_t.long()[safe.to(device)], idx_hip[safe.to(device)])
    same = (idx_t.long() == idx_hip).flatten(1).all(1)
    assert bool(same.any())
    assert (r_t - r_hip)[same].abs().max().item() <= 2e-5 * (1 + r_hip.abs().max().item())
    assert len(torch.unique(idx_hip)) > 1
    p = counts / counts.sum()
    assert float(m.quantizer.perplexity) == pytest.approx(float(torch.exp(-(p * torch.log(p + 1e-10)).sum())), rel=1e-6)


def test_parameter_gradients_match_float64_autograd_over_the_oracle(device, pair):
    """Encoder and decoder gradients of L1 + quantisation loss against float64 autograd over the oracle's layers, the
    straight-through and commitment terms wired here; the oracle is fed the HIP indices.  Bar: the project's 1e-4 for parameter
    gradients (max-norm relative, floored at 1e-5 of the model's largest gradient, as tests/test_gpu_train.py measures it)."""
    import copy

    from ddpm_ood_amd.vqvae_train import VQTrainFunction, decode_train, encode_train

    o, m = pair
    o = copy.deepcopy(o).double()
    x = _images()
    for p in m.parameters():
        p.grad = None
        p.requires_grad_(True)
    z = encode_train(m, x.to(device))
    qz, qloss, idx, _ = VQTrainFunction.apply(z, m.quantizer.quantizer, False)
    r = decode_train(m, qz)
    (F.l1_loss(r, x.to(device)) + qloss).backward()

    x64 = x.double()
    zo = o.encode(x64)
    e = o.quantizer.quantizer.embedding.weight.detach()[idx.long().cpu()].movedim(-1, 1)
    ro = o.decode(zo + (e - zo).detach())
    lo = F.l1_loss(ro, x64) + CFG["commitment_cost"] * F.mse_loss(e, zo)
    lo.backward()
    assert abs(qloss.item() - (CFG["commitment_cost"] * F.mse_loss(e, zo)).item()) <= 2e-6 * lo.item()
    ref = dict(o.named_parameters())
    gmax = max(float(p.grad.abs().max()) for n, p in ref.items() if p.grad is not None)
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        if "embedding" in n:
            assert p.grad is None  # the codebook moves by EMA only
            continue
        gr = ref[n].grad
        rel = float((p.grad.cpu().double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5 * gmax))
        worst = max(worst, (n, rel), key=lambda kv: kv[1])
        assert rel <= 1e-4, (n, rel)
    print(f"worst parameter-gradient error: {worst[1]:.2e} ({worst[0]})")
    for p in m.parameters():
        p.grad = None


def test_cli_writes_checkpoint_and_config_and_resumes(device, tmp_path):
    """train_vqvae.py --quick_test 1 --n_epochs 1, then a second invocation that resumes at epoch + 1."""
    argv = [sys.executable, str(ROOT / "train_vqvae.py"), *CLI, "--output_dir", str(tmp_path), "--model_name", "cli",
            "--quick_test", "1", "--checkpoint_every", "1", "--eval_freq", "1"]
    out = subprocess.run(argv + ["--n_epochs", "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert out.stderr.count("NOT built") == 1 and "Validation 0" in out.stdout
    run = tmp_path / "cli"
    ck = torch.load(run / "checkpoint.pth", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "best_loss"}
    assert ck["epoch"] == 1 and ck["global_step"] == 16 and ck["best_loss"] < 1000
    sd = ck["model_state_dict"]
    assert "quantizer.quantizer.ema_cluster_size" in sd and "quantizer.quantizer.ema_w" in sd
    assert float(sd["quantizer.quantizer.ema_cluster_size"].sum()) > 0  # the EMA update ran
    cfg = json.load(open(run / "vqvae_config.json"))
    assert set(cfg) == CONFIG_KEYS and len(cfg) == 15
    assert ck["optimizer_state_dict"]["param_groups"][0]["lr"] == 3e-4 and ck["optimizer_state_dict"]["state"]  # the one that steps
    # the checkpoint stores epoch + 1 and the reference resumes at checkpoint["epoch"] + 1 (kept, as train.DDPMTrainer keeps it):
    # after epoch 0 the next invocation starts at epoch 2
    out = subprocess.run(argv + ["--n_epochs", "3"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    assert re.search(rf"Resuming training using checkpoint .* at epoch {ck['epoch'] + 1}\b", out.stdout), out.stdout[-1500:]
    assert "Epoch 2:" in out.stdout and "Epoch 0:" not in out.stdout and "Epoch 1:" not in out.stdout
    ck2 = torch.load(run / "checkpoint_3.pth", map_location="cpu", weights_only=False)
    assert ck2["epoch"] == 3 and ck2["global_step"] == 32


@pytest.fixture(scope="module")
def trained(device, tmp_path_factory):
    """One trainer, PROGRESS_STEPS steps on ONE fixed batch, then a checkpoint -- shared by the tests below."""
    from ddpm_ood_amd.vqvae_train import VQVAETrainer

    root = tmp_path_factory.mktemp("vqtrain")
    a = _args(root, "fixed", n_epochs=1, checkpoint_every=0)
    tr = VQVAETrainer(a)
    x = _images().to(device)
    e0 = tr.model.quantizer.quantizer.embedding.weight.detach().clone()
    l1 = [float(tr.train_step(x)[1]) for _ in range(PROGRESS_STEPS + 1)]  # l1[i]: L1 of the forward BEFORE update i
    tr.save_checkpoint(tr.run_dir / "checkpoint.pth", 0, "saving")
    return tr, root, l1, e0


def test_training_makes_progress_on_a_fixed_batch(trained):
    tr, _, l1, e0 = trained
    print(f"L1 on the fixed batch: step 0 {l1[0]:.6f} -> step {PROGRESS_STEPS} {l1[-1]:.6f}; perplexity "
          f"{float(tr.model.quantizer.perplexity):.3f}")
    assert l1[-1] < l1[0]
    assert not torch.equal(tr.model.quantizer.quantizer.embedding.weight.detach(), e0)
    assert all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_checkpoint_loads_through_the_existing_paths(device, trained):
    """VQVAE(**config).load_state_dict and BaseTrainer's --vqvae_checkpoint loader accept the files; the loaded model encodes
    exactly as the trained one."""
    from ddpm_ood_amd.trainer import BaseTrainer
    from ddpm_ood_amd.vqvae import VQVAE

    tr, root, _, _ = trained
    run = root / "fixed"
    cfg = json.load(open(run / "vqvae_config.json"))
    m = VQVAE(**cfg)
    m.load_state_dict(torch.load(run / "checkpoint.pth", map_location="cpu", weights_only=False)["model_state_dict"])
    bt = object.__new__(BaseTrainer)
    bt.device = device
    bt._setup_stage1(argparse.Namespace(is_grayscale=1, vqvae_checkpoint=str(run / "checkpoint.pth")))
    assert bt.ddpm_channels == 8
    x = _images().to(device)
    with torch.no_grad():
        want = tr.model.encode_stage_2_inputs(x)
        assert torch.equal(m.to(device).eval().encode_stage_2_inputs(x), want)
        assert torch.equal(bt.vqvae_model.encode_stage_2_inputs(x), want)


def test_missing_terms_warning_is_printed_once_and_recorded(device, tmp_path, capsys):
    from ddpm_ood_amd import vqvae_train

    vqvae_train._WARNED.clear()
    capsys.readouterr()
    a = vqvae_train.VQVAETrainer(_args(tmp_path, "w1"))
    b = vqvae_train.VQVAETrainer(_args(tmp_path, "w2"))
    err = capsys.readouterr().err
    assert err.count("NOT built") == 1 and "LPIPS" in err and "Jukebox" in err and "adversarial" in err
    for t in (a, b):
        assert len(t.last_stats["missing_loss_terms"]) == 3 and "LPIPS" in t.last_stats["missing_loss_terms"][0]
    with pytest.raises(NotImplementedError, match="dropout"):
        vqvae_train.VQVAETrainer(_args(tmp_path, "w3", vqvae_dropout=0.1))


# ---- two ranks (fresh child processes, gloo transport on one device as tests/test_gpu_dist.py) --------------------------------

_RANK_SCRIPT = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import train_vqvae
from ddpm_ood_amd import ops
from ddpm_ood_amd.vqvae_train import VQVAETrainer
a = train_vqvae.parse_args(sys.argv[3:] + ["--output_dir", sys.argv[2], "--model_name", "ranks"])
tr = VQVAETrainer(a)
rec = []
orig = ops.vq_train_assign
def spy(x, e, cc):
    out = orig(x, e, cc)
    rec.append((x.detach().cpu(), out[0].cpu()))
    return out
ops.vq_train_assign = spy
x = tr.train_loader.images.to(tr.device)  # this rank's shard: 16 / world images, one batch
w = []
for _ in range(2):
    tr.train_step(x)
    q = tr.model.quantizer.quantizer
    cs = q.ema_cluster_size.double()
    n = cs.sum()
    w.append(((cs + q.epsilon) / (n + q.num_embeddings * q.epsilon) * n).cpu())
torch.save({"codebook": tr.model.quantizer.quantizer.embedding.weight.detach().cpu(), "rec": rec, "w": w,
            "n": int(x.shape[0])}, f"{sys.argv[2]}/rank{tr.rank}_of_{tr.world}.pt")
if tr.ddp:
    import torch.distributed as dist
    dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_hold_one_codebook(device, tmp_path):
    """With vqvae_ddp_sync both ranks hold bit-identical codebooks after 2 steps, and they equal a one-rank run over the same 16
    images within the dw bound: either run's dw is a fixed-order fp32 sum within count_k 2^-24 sum |x| of the exact one, so two
    runs differ by at most twice that, propagated through (1 - decay) / w_k and the second step's decay, plus 4 ulp."""
    from test_gpu_dist import _launch_ranks

    _launch_ranks(2, ["-c", _RANK_SCRIPT, str(ROOT), str(tmp_path), *CLI], tmp_path, timeout=600)
    out = subprocess.run([sys.executable, "-c", _RANK_SCRIPT, str(ROOT), str(tmp_path), *CLI], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    r0, r1 = (torch.load(tmp_path / f"rank{r}_of_2.pt", weights_only=False) for r in (0, 1))
    one = torch.load(tmp_path / "rank0_of_1.pt", weights_only=False)
    assert r0["n"] == r1["n"] == 8 and one["n"] == 16
    assert torch.equal(r0["codebook"], r1["codebook"])
    K, decay = 16, 0.99
    bound = torch.zeros(K, 8, dtype=torch.float64)
    for step, (x, idx) in enumerate(one["rec"]):
        flat = x.double().movedim(1, -1).reshape(-1, 8)
        i = idx.reshape(-1).long()
        counts = torch.bincount(i, minlength=K).double()
        absx = torch.zeros(K, 8, dtype=torch.float64).index_add_(0, i, flat.abs())
        bound = decay * bound + (1 - decay) * 2 * counts[:, None] * 2.0 ** -24 * absx
    E1, E2 = one["codebook"].double(), r0["codebook"].double()
    ulp = torch.exp2(torch.floor(torch.log2(E1.abs().clamp_min(2.0 ** -126))) - 23)
    err = (E1 - E2).abs()
    lim = bound / one["w"][-1][:, None] + 4 * ulp
    print(f"two ranks vs one: worst codebook difference / bound {(err / lim).max():.3f}")
    assert bool((err <= lim).all())
