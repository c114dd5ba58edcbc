"""The two fixed-function terms of the VQ-VAE generator loss, forward and backward on this library's kernels (SURVEY.md A.8,
DESIGN.md 3.18; the reference's src/trainers/vqvae_trainer.py adds ``0.001 x PerceptualLoss + JukeboxLoss`` to L1 + quantisation).

Definitions, RECALLED (the ``generative`` package is not installed here):

* spectral term -- ``JukeboxLoss(spatial_dims)`` with its defaults: ``A(t) = |fftn(t, dim=(1, ..., spatial_dims + 1), norm="ortho")|``
  (the CHANNEL axis is inside the transform), ``loss = mean over all elements of (A(recon) - A(image))^2``, weight 1.0.
  Here: dense per-axis DFTs -- two real matrices cos / sqrt(n), -sin / sqrt(n) per length, built in float64 on the host, rounded
  once to fp32, cached per (n, device) -- as strided batched products on ``train_ops.gemm`` (fp32 MFMA, no transpose pass, any
  length; split_f16 stays off), one fused elementwise kernel for the value and the spectrum-side gradient
  ``G = (2 / N) dloss (|R| - |X|) R / |R|``, and -- the ortho transform being unitary -- the inverse DFT of G, real part, as the
  gradient.  DEVIATION: ``G = 0`` where ``|R| = 0`` (autograd over torch.fft gives NaN there).
* perceptual term -- ``PerceptualLoss(spatial_dims, network_type="alex", is_fake_3d=True)``: ``lpips(recon, image)`` with
  ``normalize=False`` (QUIRK, kept: the package feeds [0, 1] images to a network that expects [-1, 1]).  2-D: the mean over the
  batch.  3-D: for each of the three spatial axes move that axis into the batch (slices ``[B len, C, ., .]``), keep ``int(n 0.5)``
  slices chosen by a permutation, take the mean LPIPS over them; the three means are summed.  Weight 0.001.
  DEVIATION: the slice indices are drawn on the HOST from a seeded ``torch.Generator`` (trainer seed, epoch, step) and passed in
  as index tensors -- a run is reproducible and a test supplies its own.  Where a feature vector is all-zero the gradient of
  its norm is taken as 0 (autograd: NaN).

Both are ``torch.autograd.Function``s that differentiate with respect to the reconstruction only: the target branch and every
LPIPS weight are constants.  Device tensors only; no torch.fft, rocFFT or rocBLAS on the path.
"""

from __future__ import annotations

import math

import torch

from . import ops, train_ops

KNOWN_TERMS = ("perceptual", "spectral")
PERCEPTUAL_WEIGHT = 0.001
SPECTRAL_WEIGHT = 1.0
MIN_LPIPS_SIZE = 32  # AlexNet's second max-pool is empty below
FAKE3D_KEEP = 0.5


def parse_terms(env_value) -> tuple:
    """``DDPM_VQVAE_LOSS_TERMS``: a comma list drawn from KNOWN_TERMS -> the enabled terms in KNOWN_TERMS order; empty / None: ()."""
    names = [s.strip() for s in (env_value or "").split(",") if s.strip()]
    unknown = sorted(set(names) - set(KNOWN_TERMS))
    if unknown:
        raise ValueError(f"DDPM_VQVAE_LOSS_TERMS: unknown term(s) {unknown}; known: {', '.join(KNOWN_TERMS)}")
    return tuple(t for t in KNOWN_TERMS if t in names)


# ---- dense ortho DFT ----------------------------------------------------------------------------------------------------------

def dft_matrices64(n: int):
    """(C, S) float64 [n, n]: C[k, j] = cos(2 pi j k / n) / sqrt(n), S[k, j] = -sin(2 pi j k / n) / sqrt(n) -- the ortho-normalised
    DFT is C + i S.  The angle is reduced with integer arithmetic (j k mod n) before it meets pi."""
    k = torch.arange(n, dtype=torch.int64)
    ang = (-2.0 * math.pi / n) * ((k[:, None] * k[None, :]) % n).double()
    return torch.cos(ang) / math.sqrt(n), torch.sin(ang) / math.sqrt(n)


_DFT_CACHE = {}


def dft_block(n: int, device) -> torch.Tensor:
    """fp32 [2n, 2n] = [[C, -S], [S, C]] on ``device``: (re, im) -> (re, im) of one forward transform; its transpose is the
    inverse (C and S are symmetric).  Rounded to fp32 once, cached per (n, device)."""
    key = (int(n), str(device))
    m = _DFT_CACHE.get(key)
    if m is None:
        c, s = dft_matrices64(n)
        m = _DFT_CACHE[key] = torch.cat([torch.cat([c, -s], 1), torch.cat([s, c], 1)], 0).float().contiguous().to(device)
    return m


def _dft_axis(src, complex_in: bool, complex_out: bool, shape, axis: int, inverse: bool):
    """One axis of the transform of a tensor of ``shape`` held as planes: src is [2, *shape] (complex_in) or [*shape]; returns
    [2, *shape] (complex_out) or [*shape] (the real part).  The axis is addressed by its element stride, no transpose."""
    n = shape[axis]
    P = math.prod(shape)
    inner = math.prod(shape[axis + 1:])
    outer = P // (n * inner)
    F = dft_block(n, src.device)
    dst = torch.empty(((2,) if complex_out else ()) + tuple(shape), dtype=torch.float32, device=src.device)
    ncout = 2 if complex_out else 1
    K = 2 * n if complex_in else n
    # the (c_out, k) x (c_in, j) entry of the forward block F, or of its transpose
    m_out, m_in, c_out, c_in = (2 * n, 1, 2 * n * n, n) if not inverse else (1, 2 * n, n, 2 * n * n)
    if inner == 1:  # last axis: rows = everything else, columns = the axis
        train_ops.gemm(src, F, dst, outer, n, K, k_inner=n, a_m=n, a_k=1, a_k_outer=P, b_n=m_out, b_k=m_in, b_k_outer=c_in,
                       c_m=n, c_n=1, batch=ncout, b_batch=c_out, c_batch=P)
        return dst
    step = 65535 // ncout  # the grid's z extent
    for o0 in range(0, outer, step):
        oc = min(step, outer - o0)
        off = o0 * n * inner
        train_ops.gemm(F, src, dst, n, inner, K, k_inner=n, a_m=m_out, a_k=m_in, a_k_outer=c_in, b_k=inner, b_k_outer=P, b_n=1,
                       c_m=inner, c_n=1, batch=ncout * oc, batch_inner=oc, a_batch=0, a_batch_outer=c_out, b_batch=n * inner,
                       b_batch_outer=0, c_batch=n * inner, c_batch_outer=P, b_off=off, c_off=off)
    return dst


def _axes(shape):
    return [a for a in range(1, len(shape)) if shape[a] > 1]


def dft_forward(t: torch.Tensor) -> torch.Tensor:
    """[2 (re, im), *t.shape]: fftn(t, dim = every axis but the first, norm="ortho") of a real device tensor."""
    t = t.float().contiguous()
    shape = tuple(t.shape)
    axes = _axes(shape)
    if not axes:
        z = torch.zeros((2,) + shape, dtype=torch.float32, device=t.device)
        z[0].copy_(t)
        return z
    z = t
    for i, a in enumerate(axes):
        z = _dft_axis(z, i > 0, True, shape, a, False)
    return z


def dft_inverse_real(z: torch.Tensor) -> torch.Tensor:
    """The real part of the inverse of ``dft_forward`` -- its adjoint, the transform being unitary."""
    shape = tuple(z.shape[1:])
    axes = _axes(shape)
    if not axes:
        return z[0].clone()
    for i, a in enumerate(axes):
        z = _dft_axis(z, True, i + 1 < len(axes), shape, a, True)
    return z


def spectral_closed_form64(recon: torch.Tensor, image: torch.Tensor):
    """(loss, d loss / d recon) in float64 torch on the host by the SAME closed form and the same dense matrices the device path
    uses (tests hold it against autograd over torch.fft): the definition, not the product path."""
    def fwd(re, im, sign):
        for a in _axes(re.shape):
            c, s = dft_matrices64(re.shape[a])
            s = sign * s
            rm, qm = re.movedim(a, -1), im.movedim(a, -1)
            re, im = (rm @ c - qm @ s).movedim(-1, a), (rm @ s + qm @ c).movedim(-1, a)
        return re, im
    r, x = recon.double(), image.double()
    rr, ri = fwd(r, torch.zeros_like(r), 1.0)
    xr, xi = fwd(x, torch.zeros_like(x), 1.0)
    ar, ax = torch.sqrt(rr * rr + ri * ri), torch.sqrt(xr * xr + xi * xi)
    loss = ((ar - ax) ** 2).mean()
    g = torch.where(ar > 0, (2.0 / ar.numel()) * (ar - ax) / ar.clamp_min(1e-300), torch.zeros_like(ar))
    return loss, fwd(g * rr, g * ri, -1.0)[0]


class SpectralLossFunction(torch.autograd.Function):
    """(recon, image) [B, C, *spatial] -> the Jukebox spectral loss, a device scalar; backward: the gradient w.r.t. recon."""

    @staticmethod
    def forward(ctx, recon, image):
        if not (recon.is_cuda and image.is_cuda):
            raise RuntimeError("the spectral term runs on the HIP kernels: ROCm device tensors only")
        if recon.shape != image.shape:
            raise ValueError(f"spectral term: {tuple(recon.shape)} vs {tuple(image.shape)}")
        zr, zx = dft_forward(recon.detach()), dft_forward(image.detach())
        loss, _ = train_ops.spectral_amp_grad(zr, zx)
        ctx.save_for_backward(zr, zx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        zr, zx = ctx.saved_tensors
        _, g = train_ops.spectral_amp_grad(zr, zx, dloss=dloss.float().reshape(1).contiguous(), want_loss=False, want_grad=True)
        return dft_inverse_real(g), None


def spectral_term(recon: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    return SpectralLossFunction.apply(recon, image)


# ---- LPIPS with a gradient ----------------------------------------------------------------------------------------------------

def _rotated(lpips, conv, device):
    """(rotated + transposed weight [Cin, Cout, k, k], its MFMA packing or None) of one stride-1 layer, cached like ``_packed``."""
    key = ("rot", id(conv))
    tag = (conv.weight.data_ptr(), conv.weight._version, str(device))
    hit = lpips._packed.get(key)
    if hit is None or hit[0] != tag:
        rot = train_ops.conv_weight_rot180t(conv.weight.detach())
        hit = lpips._packed[key] = (tag, rot, ops.pack_conv_weight(rot) if rot.shape[-1] == 3 else None)
    return hit[1], hit[2]


class LPIPSGradFunction(torch.autograd.Function):
    """(recon, image [n, 1|3, H, W], lpips module) -> LPIPS(recon, image, normalize=False) [n], the scoring path's bits; backward:
    one upstream scalar per pair -> the gradient w.r.t. recon.  ``last_paths`` names, per stride-1 layer, the route its input
    gradient took at the latest backward ("mfma": ops.conv over the packed rotated weight; "generic": ops.lpips_conv)."""

    last_paths = {}

    @staticmethod
    def forward(ctx, recon, image, lpips):
        if not (recon.is_cuda and image.is_cuda):
            raise RuntimeError("the perceptual term runs on the HIP kernels: ROCm device tensors only")
        if recon.shape != image.shape or recon.ndim != 4 or recon.shape[1] not in (1, 3):
            raise ValueError(f"LPIPS wants two equal [N, 1|3, H, W] batches, got {tuple(recon.shape)} and {tuple(image.shape)}")
        if min(recon.shape[2:]) < MIN_LPIPS_SIZE:
            raise ValueError(f"the perceptual term needs spatial sizes >= {MIN_LPIPS_SIZE} (AlexNet's second max-pool is empty "
                             f"below), got {tuple(recon.shape[2:])}")
        n = recon.shape[0]
        feats = lpips._features_hip(torch.cat([recon.detach().float(), image.detach().float()], 0).contiguous(), False)
        val = None
        for k, f in enumerate(feats):
            val = ops.lpips_layer(f[:n], f[n:], lpips.lins[k].model[1].weight.reshape(-1), val)
        ctx.lpips = lpips
        ctx.in_shape = tuple(recon.shape)
        ctx.save_for_backward(*feats)
        return val

    @staticmethod
    def backward(ctx, dval):
        lpips, feats = ctx.lpips, ctx.saved_tensors
        n, cx, H, W = ctx.in_shape
        up = dval.float().reshape(n).contiguous()
        net = lpips.net
        convs = [net.slice1[0], net.slice2[1], net.slice3[1], net.slice4[0], net.slice5[0]]
        lins = [lin.model[1].weight.reshape(-1) for lin in lpips.lins]
        paths = {}

        def dgrad(k, g):  # gradient w.r.t. the input of stride-1 layer k given the gradient before its ReLU
            rot, packed = _rotated(lpips, convs[k], g.device)
            if packed is not None:
                paths[k] = "mfma"
                return ops.conv(g, rot, None, packed=packed)
            paths[k] = "generic"
            return ops.lpips_conv(g, rot, None, 1, rot.shape[-1] // 2, False)

        g = ops.lpips_layer_backward(feats[4][:n], feats[4][n:], lins[4], up)
        for k in (3, 2):  # no pool between slices 3, 4 and 5: the layer's own term adds into the convolution's
            g = ops.lpips_layer_backward(feats[k][:n], feats[k][n:], lins[k], up, out=dgrad(k + 1, g))
        for k in (1, 0):
            d = dgrad(k + 1, g)
            g = ops.lpips_layer_backward(feats[k][:n], feats[k][n:], lins[k], up)
            ops.maxpool3s2_backward(feats[k][:n], d, out=g, relu_mask=True)
        LPIPSGradFunction.last_paths = paths
        scale = lpips.scaling_layer.scale.reshape(-1)
        return ops.lpips_conv1_dgrad(g, convs[0].weight, cx, H, W, 4, 2, in_scale=(1.0 / scale).contiguous()), None, None


def fake3d_slice_indices(shape, seed: int, epoch: int, step: int, keep_ratio: float = FAKE3D_KEEP):
    """The kept slices of the 2.5-D perceptual term for a [B, C, D, H, W] batch: three int64 host tensors (axes D, H, W), each
    ``int(B len keep_ratio)`` distinct indices into the ``B len`` slices of that axis -- the head of a permutation drawn from a
    ``torch.Generator`` seeded by (seed, epoch, step)."""
    if len(shape) != 5:
        raise ValueError(f"fake3d_slice_indices wants a [B, C, D, H, W] shape, got {tuple(shape)}")
    g = torch.Generator().manual_seed(((int(seed) * 1_000_003 + int(epoch)) * 1_000_003 + int(step)) % (2 ** 63 - 1))
    out = []
    for axis in (2, 3, 4):
        n = shape[0] * shape[axis]
        out.append(torch.randperm(n, generator=g)[: int(n * keep_ratio)].clone())
    return out


_VIEWS = ((0, 2, 1, 3, 4), (0, 3, 1, 2, 4), (0, 4, 1, 2, 3))


def perceptual_term(lpips, recon, image, spatial_dims: int, slice_indices=None) -> torch.Tensor:
    """The reference's perceptual term BEFORE its 0.001 weight (a device scalar).  3-D: ``slice_indices`` = three index tensors
    (``fake3d_slice_indices``), required -- this function draws nothing."""
    if min(recon.shape[2:]) < MIN_LPIPS_SIZE:
        raise ValueError(f"the perceptual term needs spatial sizes >= {MIN_LPIPS_SIZE} (AlexNet's second max-pool is empty "
                         f"below), got {tuple(recon.shape[2:])}")
    if spatial_dims == 2:
        return LPIPSGradFunction.apply(recon, image, lpips).mean()
    if spatial_dims != 3:
        raise NotImplementedError("Perceptual loss is implemented only in 2D and 3D.")
    if slice_indices is None or len(slice_indices) != 3:
        raise ValueError("the 2.5-D perceptual term needs three slice-index tensors (fake3d_slice_indices)")
    total = None
    for perm, idx in zip(_VIEWS, slice_indices):
        idx = idx.to(recon.device, torch.int64)
        if idx.numel() == 0:
            raise ValueError("the 2.5-D perceptual term: an axis keeps no slice")
        r = recon.float().permute(*perm)
        r = r.reshape(-1, *r.shape[2:]).index_select(0, idx)
        x = image.float().permute(*perm)
        x = x.reshape(-1, *x.shape[2:]).index_select(0, idx)
        v = LPIPSGradFunction.apply(r, x, lpips).mean()
        total = v if total is None else total + v
    return total
