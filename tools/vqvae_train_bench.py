"""Time the HIP quantiser training step (assign + update + backward) against the same arithmetic in torch ops on the same
device (one-hot, mm, EMA lines, mse_loss) -- same process, same box, medians of event-timed repetitions.  Results:
profiles/vqvae_training.md.

    python tools/vqvae_train_bench.py [--reps 50] [--full-step 1] [--terms 1] [--native 1]

--native 1 times the full step on both routes of the encoder / decoder gradients in the same process -- the ATen route and
DDPM_VQVAE_NATIVE=1 (vqvae_native.py) -- and the k4 s2 p1 weight-gradient kernel alone on the README's 256 -> 256 levels.

--terms 1 also times the perceptual and the spectral term of DDPM_VQVAE_LOSS_TERMS (forward + backward w.r.t. the reconstruction)
at the README configuration -- one 64^3 volume, 2.5-D LPIPS over three axes with half the slices kept -- on the HIP kernels and
through PyTorch-ROCm autograd (torch.fft, F.conv2d, F.max_pool2d), and the full training step with both terms.
    rocprofv3 --kernel-trace --stats -d out -o step -- python tools/vqvae_train_bench.py --quantiser 0 --reps 25
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def quantiser(N, D, K, reps, dev):
    from ddpm_ood_amd import ops

    g = torch.Generator().manual_seed(1)
    x = torch.randn(N // 512, D, 8, 8, 8, generator=g).to(dev)  # volumes of 8^3 latent positions
    E0 = torch.randn(K, D, generator=g).to(dev)
    dout, dloss = torch.randn(x.shape, generator=g).to(dev), torch.ones((), device=dev)
    cc, decay, eps = 0.25, 0.99, 1e-5
    st = dict(E=E0.clone(), cs=torch.ones(K, device=dev), w=E0.clone())

    def hip():
        idx, out, counts, dw, loss, _ = ops.vq_train_assign(x, st["E"], cc)
        searched = st["E"].clone()
        ops.vq_train_update(st["cs"], st["w"], st["E"], counts, dw, decay, eps)
        return ops.vq_train_backward(dout, x, searched, idx, dloss, cc)

    parts = {"assign": lambda: ops.vq_train_assign(x, st["E"], cc)}
    idx, out, counts, dw, loss, _ = ops.vq_train_assign(x, st["E"], cc)
    parts["update"] = lambda: ops.vq_train_update(st["cs"], st["w"], st["E"], counts, dw, decay, eps)
    parts["backward"] = lambda: ops.vq_train_backward(dout, x, st["E"], idx, dloss, cc)
    ts = dict(E=E0.clone(), cs=torch.ones(K, device=dev), w=E0.clone())

    def torch_ops():
        flat = x.movedim(1, -1).reshape(-1, D)
        dist = (flat ** 2).sum(1, keepdim=True) + (ts["E"].t() ** 2).sum(0, keepdim=True) - 2 * flat @ ts["E"].t()
        i = torch.max(-dist, dim=1)[1]
        enc = F.one_hot(i, K).float()
        q = F.embedding(i, ts["E"])
        ts["cs"].mul_(decay).add_(enc.sum(0) * (1 - decay))
        n = ts["cs"].sum()
        wk = (ts["cs"] + eps) / (n + K * eps) * n
        ts["w"].mul_(decay).add_((flat.t() @ enc).t() * (1 - decay))
        ts["E"].copy_(ts["w"] / wk[:, None])
        loss_t = cc * F.mse_loss(q, flat)
        dflat = dout.movedim(1, -1).reshape(-1, D) + (2 * cc / flat.numel()) * (flat - q) * dloss
        return loss_t, dflat

    rows = [("HIP assign + update + backward", timed(hip, reps))]
    rows += [(f"  HIP {k} alone", timed(f, reps)) for k, f in parts.items()]
    rows.append(("torch ops (one-hot, mm, EMA lines, mse_loss)", timed(torch_ops, reps)))
    print(f"(B*S, D, K) = ({N}, {D}, {K}); median [min .. max] us over {reps} repetitions")
    for name, (med, lo, hi) in rows:
        print(f"  {name:<48s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]")


def _aten_lpips(lp, in0, in1):
    """LPIPS(normalize=False) over the module's own weights with ATen ops and autograd (the baseline of --terms)."""
    def feats(x):
        x = (x.expand(-1, 3, -1, -1) - lp.scaling_layer.shift) / lp.scaling_layer.scale
        net, out = lp.net, []
        for k, (conv, pool) in enumerate(((net.slice1[0], False), (net.slice2[1], True), (net.slice3[1], True), (net.slice4[0], False),
                                          (net.slice5[0], False))):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, conv.weight, conv.bias, stride=conv.stride, padding=conv.padding))
            out.append(x)
        return out
    norm = lambda f: f / (torch.sqrt((f ** 2).sum(1, keepdim=True)) + 1e-10)  # noqa: E731
    val = 0
    for k, (a, b) in enumerate(zip(feats(in0), feats(in1))):
        val = val + (lp.lins[k].model[1].weight * (norm(a) - norm(b)) ** 2).sum(1).mean((1, 2))
    return val


def loss_terms_bench(dev, reps):
    """Each term's forward + backward on one 64^3 volume: HIP kernels against PyTorch-ROCm autograd, same process."""
    from ddpm_ood_amd import loss_terms
    from ddpm_ood_amd.perceptual import LPIPS

    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 1, 64, 64, 64, generator=g).to(dev)
    r = (0.8 * x + 0.1 + 0.05 * torch.randn(x.shape, generator=g).to(dev)).requires_grad_(True)
    lp = LPIPS().to(dev)
    idx = [i.to(dev) for i in loss_terms.fake3d_slice_indices(x.shape, 1, 0, 0)]

    def run(fn):
        def inner():
            r.grad = None
            fn().backward()
        return inner

    def aten_perceptual():
        total = 0
        for perm, i in zip(loss_terms._VIEWS, idx):
            rs, xs = r.permute(*perm), x.permute(*perm)
            total = total + _aten_lpips(lp, rs.reshape(-1, *rs.shape[2:])[i], xs.reshape(-1, *xs.shape[2:])[i]).mean()
        return total

    def aten_spectral():
        a = lambda t: torch.fft.fftn(t, dim=(1, 2, 3, 4), norm="ortho").abs()  # noqa: E731
        return ((a(r) - a(x)) ** 2).mean()

    rows = [("perceptual, HIP (3 x 32 slices of 64 x 64)", run(lambda: loss_terms.perceptual_term(lp, r, x, 3, idx))),
            ("perceptual, ATen autograd", run(aten_perceptual)),
            ("spectral, HIP (dense DFT on train_ops.gemm)", run(lambda: loss_terms.spectral_term(r, x))),
            ("spectral, ATen autograd (torch.fft)", run(aten_spectral))]
    vals = [float(f().detach()) for f in (lambda: loss_terms.perceptual_term(lp, r, x, 3, idx), aten_perceptual,
                                 lambda: loss_terms.spectral_term(r, x), aten_spectral)]
    print(f"loss terms, forward + backward on one 64^3 volume; median [min .. max] us over {reps} repetitions (values: perceptual "
          f"{vals[0]:.6e} / {vals[1]:.6e}, spectral {vals[2]:.6e} / {vals[3]:.6e})")
    for name, fn in rows:
        med, lo, hi = timed(fn, reps)
        print(f"  {name:<48s} {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]")


def k4s2_wgrad_bench(dev, reps):
    """ddpm_conv_k4s2_wgrad_f32 on the README VQ-VAE's 256 -> 256 down-levels (batch 1 of 64^3: inputs of 32^3, 16^3, 8^3) and on the
    1 -> 256 first layer (generic form): median time and the achieved rate over 2 B S_out Cout Cin 64 operations."""
    from ddpm_ood_amd import train_ops as T

    g = torch.Generator().manual_seed(1)
    print(f"k4 s2 p1 weight gradient; median [min .. max] us over {reps} repetitions")
    for cin, cout, n in ((256, 256, 32), (256, 256, 16), (256, 256, 8), (1, 256, 64)):
        a = torch.randn(1, cin, n, n, n, generator=g).to(dev)
        dy = torch.randn(1, cout, n // 2, n // 2, n // 2, generator=g).to(dev)
        med, lo, hi = timed(lambda: T.conv_k4s2_wgrad(a, dy), reps)
        flop = 2.0 * (n // 2) ** 3 * cout * cin * 64
        print(f"  {cin:3d} -> {cout} at {n}^3 (split {T.conv_k4s2_wgrad_split(a, dy)}) {med:9.1f} [{lo:9.1f} .. {hi:9.1f}]  "
              f"{flop / med / 1e6:7.2f} TFLOP/s")


def full_step(dev, reps, terms=()):
    """One full training step at the README configuration (batch 1 of 64^3: the volume the test suite runs the README VQ-VAE on)
    with the quantiser step timed inside it; terms: the extra loss terms of DDPM_VQVAE_LOSS_TERMS, timed inside it too."""
    from ddpm_ood_amd import ops
    from ddpm_ood_amd.vqvae import VQVAE
    from ddpm_ood_amd.vqvae_train import vqvae_forward_train

    cfg = dict(spatial_dims=3, in_channels=1, out_channels=1, num_channels=(256,) * 4, num_res_layers=3,
               num_res_channels=(256,) * 4, downsample_parameters=((2, 4, 1, 1),) * 4, upsample_parameters=((2, 4, 1, 1, 0),) * 4,
               num_embeddings=2048, embedding_dim=128, decay=0.99)
    torch.manual_seed(1)
    m = VQVAE(**cfg).to(dev)
    m.quantizer.quantizer.embedding.weight.requires_grad_(False)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=3e-4)
    x = torch.rand(1, 1, 64, 64, 64, device=dev)
    q_us = []
    names = ("vq_train_assign", "vq_train_update", "vq_train_backward")
    orig = {n: getattr(ops, n) for n in names}

    def wrap(fn):
        def inner(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            q_us.append((s, e))
            return r
        return inner

    for n in names:
        setattr(ops, n, wrap(orig[n]))
    if terms:
        from ddpm_ood_amd import loss_terms
        from ddpm_ood_amd.perceptual import LPIPS

        lp = LPIPS().to(dev)
        idx = loss_terms.fake3d_slice_indices(x.shape, 1, 0, 0)

    def step():
        opt.zero_grad(set_to_none=True)
        r, ql = vqvae_forward_train(m, x)
        loss = F.l1_loss(r, x) + ql
        if "perceptual" in terms:
            loss = loss + loss_terms.PERCEPTUAL_WEIGHT * loss_terms.perceptual_term(lp, r, x, 3, idx)
        if "spectral" in terms:
            loss = loss + loss_terms.spectral_term(r, x)
        loss.backward()
        opt.step()

    med, lo, hi = timed(step, reps, warmup=3)
    torch.cuda.synchronize()
    per_step = [sum(s.elapsed_time(e) for s, e in q_us[i: i + 3]) * 1e3 for i in range(3 * 3, len(q_us), 3)]
    for n in names:
        setattr(ops, n, orig[n])
    qm = statistics.median(per_step)
    from ddpm_ood_amd.vqvae_train import native_conv_gradients

    print(f"full training step ({' + '.join(('l1', 'quantisation') + tuple(terms))}; conv gradients: "
          f"{'native' if native_conv_gradients() else 'aten'}), README VQ-VAE, batch 1 of 64^3 (64 latent positions): median {med / 1e3:.2f} ms "
          f"[{lo / 1e3:.2f} .. {hi / 1e3:.2f}] over {reps} steps; quantiser (3 HIP entry points) {qm:.1f} us = {100 * qm / med:.2f} % of the step")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--full-step", type=int, default=1)
    ap.add_argument("--quantiser", type=int, default=1, help="0: only the full step (e.g. under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--terms", type=int, default=0, help="1: time the perceptual and spectral loss terms, alone and inside the step")
    ap.add_argument("--native", type=int, default=0, help="1: the full step on the ATen route and with DDPM_VQVAE_NATIVE=1, and the "
                                                           "k4 s2 weight-gradient kernel alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.quantiser:
        quantiser(2048, 128, 2048, a.reps, dev)   # batch 4 of 128^3 through four stride-2 levels: 4 x 8^3 latent positions
        quantiser(16384, 128, 2048, a.reps, dev)
    if a.full_step:
        full_step(dev, max(5, a.reps // 5))
    if a.native:
        import os

        k4s2_wgrad_bench(dev, a.reps)
        was = os.environ.get("DDPM_VQVAE_NATIVE")
        for leg in ("0", "1", "0", "1"):  # alternating: the spread between equal legs is the noise
            os.environ["DDPM_VQVAE_NATIVE"] = leg
            full_step(dev, max(5, a.reps // 5))
        if was is None:
            del os.environ["DDPM_VQVAE_NATIVE"]
        else:
            os.environ["DDPM_VQVAE_NATIVE"] = was
    if a.terms:
        loss_terms_bench(dev, max(5, a.reps // 5))
        for terms in (("perceptual",), ("spectral",), ("perceptual", "spectral")):
            full_step(dev, max(5, a.reps // 5), terms)
