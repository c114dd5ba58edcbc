"""Helper of tests/test_gpu_nonfinite.py: one batch run clean and with one poisoned image, three assertions.

For an op `run` over a batch of B >= 3 images and the same op in plain torch on the CPU (`ref`, float64):

1. neighbours untouched: out[i] of every unpoisoned image i is BIT-identical between the clean run and the poisoned run (same
   shapes, same call -> same kernel), and so are its rows of a statistics slab;
2. loud: wherever the reference is non-finite, the kernel's output is non-finite;
3. never finite and wrong: every finite output of the poisoned image is within the op's own tolerance of the reference.

A cap on the number of non-finite outputs per output plane keeps 2 and 3 from passing on an output that is NaN everywhere.
"""

import contextlib

import torch

NAN, INF = float("nan"), float("inf")


@contextlib.contextmanager
def conv_families():
    """Records the family ddpm_conv_kernel_name gives for every descriptor launched inside (tests/test_gpu_conv_select.py holds
    that name to the kernel that runs)."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    real = lib.ddpm_conv_f32
    names = []

    def spy(desc, stream):
        names.append(lib.ddpm_conv_kernel_name(desc).decode())
        return real(desc, stream)

    lib.ddpm_conv_f32 = spy
    try:
        yield names
    finally:
        lib.ddpm_conv_f32 = real


def interior(t, img, channel=None):
    """Index of one interior element of image `img`: channel 1 (0 of a one-channel tensor), the middle of every other extent."""
    c = min(1, t.shape[1] - 1) if channel is None else channel
    return (img, c) + tuple(s // 2 for s in t.shape[2:])


def poison(t, kind, img, scale=None, channel=None):
    """A copy of t with image `img` poisoned: "nan_pixel" / "inf_pixel" one interior element, "nan_image" all of it, "overflow"
    the image times `scale` (beyond the operand range of a split-f16 form)."""
    t = t.clone()
    if kind == "nan_image":
        t[img] = NAN
    elif kind == "nan_pixel":
        t[interior(t, img, channel)] = NAN
    elif kind == "inf_pixel":
        t[interior(t, img, channel)] = INF
    elif kind == "overflow":
        t[img] *= scale
    else:
        raise ValueError(kind)
    return t


def check_poisoned(run, ref, inputs, key, kind, *, img, tol, rms=None, cap=None, scale=None, exact_mask=False, neighbours=None,
                   channel=None, stats_hw=None):
    """run(inputs) -> out or (out, stats slab or None) on the device; ref(inputs) -> the same op in float64 on the CPU (images
    `neighbours + [img]` suffice when `neighbours` is given).  `inputs[key]` is poisoned.  Returns (clean out, poisoned out,
    reference) on the CPU."""
    bad = dict(inputs)
    bad[key] = poison(inputs[key], kind, img, scale, channel)
    y0, y1 = run(inputs), run(bad)
    torch.cuda.synchronize()
    st0 = st1 = None
    if isinstance(y0, tuple):
        (y0, st0), (y1, st1) = y0, y1
    y0, y1 = y0.cpu(), y1.cpu()
    B = y0.shape[0]
    assert B >= 3 and 0 < img < B - 1  # a middle image: neighbours on both sides
    assert torch.isfinite(y0).all()
    others = [i for i in range(B) if i != img] if neighbours is None else list(neighbours)
    # 1. neighbours untouched
    for i in others:
        assert torch.equal(y0[i], y1[i]), f"{kind} in image {img} changed image {i}: {(~(y0[i] == y1[i])).sum().item()} values"
    if st0 is not None:
        s0, s1 = st0.cpu(), st1.cpu()
        for i in others:
            assert torch.equal(s0[i], s1[i]), f"{kind} in image {img} changed the statistics rows of image {i}"
    r = ref(bad).double()
    got = y1.double()
    if r.shape[0] != B:  # the reference priced `others + [img]` only
        pos = {n: j for j, n in enumerate(others + [img])}
        r_img, r_all = r[pos[img]], r
    else:
        r_img, r_all = r[img], r
    g_img = got[img]
    assert g_img.shape == r_img.shape, (g_img.shape, r_img.shape)
    rn, gn = ~torch.isfinite(r_img), ~torch.isfinite(g_img)
    print(f"{kind}: reference non-finite {int(rn.sum())}, kernel non-finite {int(gn.sum())} of {gn.numel()}")
    # 2. loud
    if kind == "overflow":
        assert not rn.any()  # float64 takes the scaled image: each output is either non-finite or right
    else:
        assert rn.any()
        assert (gn | ~rn).all(), f"{int((rn & ~gn).sum())} outputs are finite where the reference is not"
    if kind == "nan_image":
        assert torch.isnan(g_img).all()
    if exact_mask:  # an elementwise epilogue: the same mask as the reference's
        assert torch.equal(gn, rn)
    # 3. never finite and wrong
    if kind != "inf_pixel":
        ok = ~gn & ~rn
        bound = 1.0 + r_all[torch.isfinite(r_all)].abs().max().item()
        if ok.any():
            err = (g_img - r_img)[ok]
            emax = err.abs().max().item()
            print(f"{kind}: max error of the finite outputs {emax:.3e} (bound {tol * bound:.3e})")
            assert emax <= tol * bound, (emax, tol * bound)
            if rms is not None:
                erms = err.pow(2).mean().sqrt().item()
                assert erms <= rms * (1.0 + r_img[ok].pow(2).mean().sqrt().item()), erms
    # a tile kernel may spread one NaN over the tiles that hold it, no further
    if cap is not None and kind == "nan_pixel":
        worst = int(gn.flatten(-2).sum(-1).max())
        assert worst <= cap, f"{worst} non-finite outputs in one output plane, cap {cap}"
        assert int(rn.flatten(-2).sum(-1).max()) <= cap  # (the reference alone meets the cap)
    # the statistics slab of the poisoned image: non-finite mean wherever its slice holds a non-finite output, and the pair as
    # gn_finalize consumes it gives a non-finite scale or shift (M2 may be clamped: the mean carries the NaN)
    if st1 is not None and kind in ("nan_pixel", "nan_image"):
        from ddpm_ood_amd import ops

        parts = st1.shape[2]
        hit = ~torch.isfinite(y1[img]).reshape(y1.shape[1], parts, -1).all(-1)
        mean_bad = ~torch.isfinite(st1[img, :, :, 0].cpu())
        assert hit.any() and mean_bad[hit].all(), "a slice with a non-finite output has a finite mean in the statistics slab"
        C = y1.shape[1]
        ones, zeros = torch.ones(C, device=st1.device), torch.zeros(C, device=st1.device)
        hw = stats_hw or y1[0, 0].numel()
        sc, sh = ops.gn_finalize(st1, ones, zeros, 32, 1e-6, hw)
        sc0, sh0 = ops.gn_finalize(st0, ones, zeros, 32, 1e-6, hw)
        g_hit = hit.any(-1).reshape(32, -1).any(-1).repeat_interleave(C // 32)
        nf = ~(torch.isfinite(sc[img]) & torch.isfinite(sh[img])).cpu()
        assert nf[g_hit].all(), "gn_finalize made a finite scale and shift from the statistics of a group with a NaN"
        for i in others:
            assert torch.equal(sc[i], sc0[i]) and torch.equal(sh[i], sh0[i])
    return y0, y1, r
