"""CPU: the host side of VQ-VAE training -- the CLI's flag table against the reference's (extracted as data), the differentiable
ATen encoder / decoder against the oracle VQ-VAE, and the reference's epoch-loss quirk."""

import json
from pathlib import Path

import pytest
import torch

G = Path(__file__).resolve().parent / "golden"

CFG = dict(spatial_dims=2, in_channels=1, out_channels=1, num_channels=(8, 16), num_res_layers=1, num_res_channels=(8, 16),
           downsample_parameters=((2, 4, 1, 1), (2, 4, 1, 1)), upsample_parameters=((2, 4, 1, 1, 0), (2, 4, 1, 1, 0)),
           num_embeddings=16, embedding_dim=8)


def test_cli_flags_match_the_reference():
    """train_vqvae.parse_args([]) carries the reference's 34 flags and defaults (tests/golden/train_vqvae_cli_flags.json, extracted
    with ast by tests/golden/make_golden_vqvae_flags.py); the ast.literal_eval flags parse tuples; --vqvae_ddp_sync keeps type=bool."""
    import train_vqvae

    flags = json.load(open(G / "train_vqvae_cli_flags.json"))
    assert len(flags) == 34
    a = train_vqvae.parse_args([])
    assert set(vars(a)) == set(flags), set(vars(a)) ^ set(flags)
    for k, v in flags.items():
        assert json.loads(json.dumps(getattr(a, k))) == v["default"], k
    types = {name: (None if typ in (None, str) else typ.__name__) for name, typ, _ in train_vqvae._FLAGS}
    assert types == {k: v["type"] for k, v in flags.items()}
    b = train_vqvae.parse_args(["--vqvae_num_channels", "(8, 16)", "--image_roi", "(160, 160, -1)",
                                "--vqvae_downsample_parameters", "((2, 4, 1, 1), (2, 4, 1, 1))", "--vqvae_ddp_sync", "False"])
    assert b.vqvae_num_channels == (8, 16) and b.image_roi == (160, 160, -1)
    assert b.vqvae_downsample_parameters == ((2, 4, 1, 1), (2, 4, 1, 1))
    assert b.vqvae_ddp_sync is True  # the reference's quirk: bool("False") is True


@pytest.mark.parametrize("spatial_dims,shape", [(2, (3, 1, 16, 20)), (3, (2, 1, 8, 12, 8))])
def test_aten_encoder_and_decoder_match_the_oracle_on_cpu(spatial_dims, shape):
    """encode_train / decode_train evaluate the product model's own parameters with ATen ops: on CPU tensors they equal the oracle
    VQ-VAE's encode / decode at fp32 rounding, and gradients reach every encoder / decoder parameter; the quantiser op stays
    device-only and raises like the rest of VQVAE."""
    from oracle.vqvae import VQVAE as OV
    from ddpm_ood_amd.vqvae import VQVAE
    from ddpm_ood_amd.vqvae_train import decode_train, encode_train, vqvae_forward_train

    cfg = dict(CFG, spatial_dims=spatial_dims)
    torch.manual_seed(5)
    o = OV(**cfg).eval()
    m = VQVAE(**cfg)
    m.load_state_dict(o.state_dict())
    x = torch.rand(shape, generator=torch.Generator().manual_seed(6))
    z = encode_train(m, x)
    with torch.no_grad():
        zo = o.encode(x)
        assert z.shape == zo.shape and (z - zo).abs().max() <= 1e-6 * (1 + zo.abs().max())
        ro = o.decode(zo)
    r = decode_train(m, z)
    assert r.shape == x.shape and (r.detach() - ro).abs().max() <= 1e-6 * (1 + ro.abs().max())
    (r - x).abs().mean().backward()
    for n, p in m.named_parameters():
        if "embedding" in n:
            assert p.grad is None
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vqvae_forward_train(m, x)
    with pytest.raises(NotImplementedError, match="dropout"):
        encode_train(VQVAE(**dict(cfg, dropout=0.1)), x)


def test_epoch_loss_is_the_sum_of_batch_means_over_the_number_of_images():
    """The reference's quirk (generator_epoch_loss / epoch_step with epoch_step += batch size), which picks the best checkpoint."""
    from ddpm_ood_amd.vqvae_train import epoch_loss_of

    losses, sizes = [0.5, 0.25, 1.0], [4, 4, 2]
    assert epoch_loss_of(losses, sizes) == pytest.approx(1.75 / 10)
    assert epoch_loss_of(losses, sizes) != pytest.approx(sum(losses) / 3)
    assert epoch_loss_of([0.5], [4]) == pytest.approx(0.125)  # --quick_test: one batch
