"""-m gpu: the native training step (ddpm_ood_amd/train_native.py) over CONSECUTIVE steps -- everything that carries state from
one step to the next: the packed weight forms that have to follow every Adam update, the stepper's Adam state, "one writer per
gradient, nothing to zero" under a changing batch size, the memoised F(4x4) dispatcher answer under a switch flip, and the
adaptive loss-scale controller (a NaN batch, a change of batch size).

The trajectory tests are TEACHER-FORCED: before step k the reference loads the native model's current state_dict(), so Adam's
rounding-level sign flips cannot grow into two different trajectories, and every step is held to the one-step tests' own bounds
(tests/test_gpu_train.py: loss 1e-5 relative against the float64 oracle / 2e-5 against ATen autograd, every parameter gradient
1e-4 max-norm relative, floored at 1e-5 of the model's largest gradient).  Each case also PROVES that it can see a stale form: the
reference gradient at the previous step's parameters, on this step's batch, has to differ from the one at the current parameters
by >= 1e-2 (100 x the bar) in more than half of the parameter tensors -- decided by the reference alone.

The figures measured on an MI355X (worst gradient error per case and step, the sensitivity ratios, err / err_fresh of the
batch-size test) are in DESIGN.md 3.14, "Consecutive steps"."""

import ctypes
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 2.5e-5
GRAD_BAR = 1e-4
SENSITIVITY = 1e-2


# ---- models, batches, references --------------------------------------------------------------------------------------------

def _sd(channels=1, dims=2):
    from ddpm_ood_amd.synthetic import random_state_dict

    return random_state_dict("small", channels, spatial_dims=dims, seed=1)


def _model(device, sd, channels=1, dims=2):
    from ddpm_ood_amd import DiffusionModelUNet
    from ddpm_ood_amd.trainer import MODEL_CONFIGS

    m = DiffusionModelUNet(dims, channels, channels, **MODEL_CONFIGS["small"])
    m.load_state_dict(sd)
    return m.to(device).train()


def _stepper(device, sd, channels=1, dims=2, setup=None):
    from ddpm_ood_amd.train_native import NativeUNetStep

    m = _model(device, sd, channels, dims)
    with torch.no_grad():
        st = NativeUNetStep(m, lr=LR)
    if setup:
        setup(st)
    return st


def _batches(device, sizes, channels=1, size=32, dims=2, seed=31):
    """One (images, timesteps, noise) per step, each drawn on its own from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for B in sizes:
        shape = (B, channels) + (size,) * dims
        out.append((torch.rand(shape, generator=g).to(device), torch.randint(0, 1000, (B,), generator=g).to(device),
                    torch.randn(shape, generator=g).to(device)))
    return out


def _snapshot(model):
    """The parameters as they are now (state_dict() hands out views of the stepper's flat buffer)."""
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


class _OracleRef:
    """CPU oracle.DiffusionModelUNet in float64 under torch autograd."""
    loss_bar = 1e-5

    def __init__(self, device, channels=1, dims=2):
        import oracle
        from ddpm_ood_amd.trainer import MODEL_CONFIGS

        self.m = oracle.DiffusionModelUNet(dims, channels, channels, **MODEL_CONFIGS["small"]).double().train()

    def __call__(self, sd, x, t, noise):
        self.m.load_state_dict({k: v.detach().cpu().double() for k, v in sd.items()})
        for p in self.m.parameters():
            p.grad = None
        loss = torch.nn.functional.mse_loss(self.m(x.cpu().double(), timesteps=t.cpu()), noise.cpu().double())
        loss.backward()
        return loss.item(), {k: (None if p.grad is None else p.grad.clone()) for k, p in self.m.named_parameters()}


class _AtenRef:
    """PyTorch-ROCm autograd over MIOpen / rocBLAS on the same device (the DDPM_TRAIN_NATIVE=0 route), with its deterministic
    kernels: to_k.bias has an analytically zero gradient, and the atomics of the default kernels move the reference's own
    rounding there from run to run (tests/test_gpu_train_attention_step.py::_parity; the 3-D case sits within 3 x of the bar
    there).  The first use of a batch size in a process pays MIOpen's kernel search for its convolution shapes (B = 64 and
    B = 37: ~18 s once, either kind of kernel); the later tests of this file find them searched."""
    loss_bar = 2e-5

    def __init__(self, device, channels=1, dims=2):
        self.m = _model(device, _sd(channels, dims), channels, dims)
        for p in self.m.parameters():
            p.requires_grad_(True)

    def __call__(self, sd, x, t, noise):
        from ddpm_ood_amd.train import unet_forward_torch

        with torch.no_grad():
            self.m.load_state_dict(sd)
        for p in self.m.parameters():
            p.grad = None
        was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            loss = torch.nn.functional.mse_loss(unet_forward_torch(self.m, x, t), noise)
            loss.backward()
        finally:
            torch.use_deterministic_algorithms(was[0], warn_only=was[1])
        return loss.item(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in self.m.named_parameters()}


def _gmax(grads):
    return max(float(g.abs().max()) for g in grads.values() if g is not None)


def _check_gradients(st, grads, what):
    """The one-step tests' comparison -> (worst error, its parameter)."""
    ph = dict(st.model.named_parameters())
    assert set(ph) == set(grads)
    gmax = _gmax(grads)
    worst = ("", 0.0)
    for k, gr in grads.items():
        gh = ph[k].grad
        if gr is None:  # (proj_attn: present in the state_dict, unused in the forward)
            assert gh is None or float(gh.abs().max()) == 0.0, (what, k)
            continue
        # (to_k.bias has an analytically ZERO gradient: measured against the parameter's own scale, floored at 1e-5 of the model's
        # largest gradient)
        rel = float((gh.to(gr.device, gr.dtype) - gr).abs().max() / max(float(gr.abs().max()), 1e-5 * gmax))
        worst = max(worst, (k, rel), key=lambda kv: kv[1])
        assert rel <= GRAD_BAR, (what, k, rel)
    return worst[1], worst[0]


def _sensitivity(cur, prev):
    """The reference's gradient at the current against the previous parameters, same batch, in the norm of _check_gradients ->
    (share of the parameter tensors that differ by >= SENSITIVITY, median difference)."""
    gmax = _gmax(cur)
    d = [float((prev[k] - g).abs().max() / max(float(g.abs().max()), 1e-5 * gmax)) for k, g in cur.items() if g is not None]
    d.sort()
    return sum(x >= SENSITIVITY for x in d) / len(d), d[len(d) // 2]


def _profiled(fn):
    """fn() under the library's in-situ profiler -> (result, {key: launches})."""
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    lib.ddpm_prof_report(buf, len(buf))  # (drops whatever an earlier test left unreported)
    lib.ddpm_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.ddpm_prof_enable(0)
    n = lib.ddpm_prof_report(buf, len(buf))
    report = json.loads(buf.value.decode()) if n > 0 else {}
    return out, {k: v["launches"] for k, v in report.items()}


# ---- the trajectory ---------------------------------------------------------------------------------------------------------

CASES = {  # id: (channels, size, dims, batch sizes per step, reference, attention route, F(4x4) forms asserted)
    "small-oracle64-gemm": (1, 32, 2, (4, 4, 3), _OracleRef, "gemm", False),
    "small-oracle64-recompute": (1, 32, 2, (4, 4, 3), _OracleRef, "recompute", False),
    "small-f4x4": (1, 32, 2, (64, 64, 37), _AtenRef, "gemm", True),
    "latent3d": (128, 8, 3, (4, 3), _AtenRef, "gemm", False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_follow_the_updated_parameters(device, monkeypatch, case):
    """Loss and every parameter gradient of step k against a reference that holds the native model's parameters AFTER k - 1 native
    Adam steps: a packed form (F(4x4), F(2x2), stride-2, rotated / transposed, 1x1 operands, the 3-D forms) or a gradient left
    over from the step before is 100 x the bar off (asserted: the sensitivity condition).  The last batch is ragged."""
    channels, size, dims, sizes, Ref, route, f4x4 = CASES[case]
    monkeypatch.setenv("DDPM_TRAIN_ATTN", route)
    st = _stepper(device, _sd(channels, dims), channels, dims)
    ref = Ref(device, channels, dims)
    prev_sd = None
    for k, (x, t, noise) in enumerate(_batches(device, sizes, channels, size, dims), start=1):
        sd = _snapshot(st.model)
        loss_r, grads = ref(sd, x, t, noise)
        if prev_sd is not None:
            _, stale = ref(prev_sd, x, t, noise)
            share, median = _sensitivity(grads, stale)
            print(f"{case} step {k}: a gradient at the previous parameters differs by >= {SENSITIVITY} in {share:.0%} of the "
                  f"tensors (median {median:.3g})")
            assert share > 0.5, f"step {k} cannot tell updated from stale parameters: {share:.0%} of the tensors, median {median:.3g}"
        with torch.no_grad():
            loss_h, launches = _profiled(lambda: st.loss_and_grads(x, t, noise))
        assert abs(loss_h.item() - loss_r) <= ref.loss_bar * abs(loss_r), (k, loss_h.item(), loss_r)
        worst, name = _check_gradients(st, grads, f"step {k}")
        print(f"{case} step {k} (B = {x.shape[0]}): loss {loss_r:.6f}, worst gradient error {worst:.2e} ({name})")
        if route == "recompute":
            assert any(r[0] == "recompute" for r in st.attn_routes), st.attn_routes
        if f4x4:  # otherwise the case did not run the forms it is there for
            assert any(key.startswith("conv3x3_wino44h") for key in launches), sorted(launches)
            assert st.dgrad_form == "wino44h" and st.overflow_retries == 0
        prev_sd = sd
        with torch.no_grad():
            st.adam_step()
    assert st.step_count == len(sizes)


def test_adam_state_carries_across_steps(device):
    """step_count, m, v in the flat buffers and the bias correction at step >= 2: torch.optim.Adam in float64 on a copy of the
    INITIAL parameters, fed the native gradients, stays within 6e-7 of the flat parameter buffer over five steps (the bound of
    test_adam_kernel_matches_torch_adam_over_five_steps: same kernel, same step count, |p| <= 4), and the checkpointed state is
    the replay's.  Moment bounds: every intermediate of m_k = m + (g - m)(1 - b1) and v_k = b2 v + (1 - b2) g g is at most
    A_k = b A_(k-1) + (1 - b) |term|; per step 3 roundings and the fp32 constants the kernel receives (b as a float: 1 - b is
    off by up to 2^-24 b / (1 - b) relative, 9 x 2^-24 for b1 and 999 x 2^-24 for b2), so (5 x 4 + b / (1 - b)) 2^-24 A, rounded
    up to (32 + b / (1 - b)) 2^-24 A, plus fp32's smallest normal where g g underflows."""
    sizes = (4, 4, 4, 4, 3)
    st = _stepper(device, _sd())
    p0 = st.flat.detach().cpu().double()
    assert float(p0.abs().max()) <= 4.0
    replay = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([replay], lr=LR)
    u, tiny = 2.0 ** -24, 2.0 ** -126
    Am, Av = torch.zeros_like(p0), torch.zeros_like(p0)
    for k, (x, t, noise) in enumerate(_batches(device, sizes, seed=41), start=1):
        with torch.no_grad():
            st.loss_and_grads(x, t, noise)
        g = st.gflat.detach().cpu().double()
        assert bool(torch.isfinite(g).all())
        replay.grad = g.clone()
        opt.step()
        with torch.no_grad():
            st.adam_step()
        err = float((st.flat.detach().cpu().double() - replay.detach()).abs().max())
        print(f"step {k}: max |flat - float64 replay| = {err:.2e}")
        assert err < 6e-7, (k, err)
        Am, Av = 0.9 * Am + 0.1 * g.abs(), 0.999 * Av + 0.001 * g * g
        ref = opt.state[replay]
        assert st.step_count == k == int(ref["step"])
        sd = st.state_dict()["state"]
        assert sorted(sd) == list(range(len(st.params)))
        for i, p in enumerate(st.params):
            off, n = st.offsets[id(p)]
            assert float(sd[i]["step"]) == k and sd[i]["exp_avg"].shape == p.shape
            em = (sd[i]["exp_avg"].cpu().double().reshape(-1) - ref["exp_avg"][off: off + n]).abs()
            ev = (sd[i]["exp_avg_sq"].cpu().double().reshape(-1) - ref["exp_avg_sq"][off: off + n]).abs()
            assert bool((em <= (32 + 9) * u * Am[off: off + n] + tiny).all()), (k, i, float(em.max()))
            assert bool((ev <= (32 + 999) * u * Av[off: off + n] + tiny).all()), (k, i, float(ev.max()))


def test_state_dict_round_trip_mid_trajectory(device):
    """Two steps, save the model and the stepper, load both into fresh ones, steps 3 and 4 on both with the same inputs: the same
    loss scale, then the same bits in the gradient and the parameter buffers (same kernels, inputs and order)."""
    import copy

    batches = _batches(device, (4, 4, 4, 3), seed=51)
    a = _stepper(device, _sd())
    with torch.no_grad():
        for x, t, noise in batches[:2]:
            a.loss_and_grads(x, t, noise)
            a.adam_step()
    model_sd, step_sd = _snapshot(a.model), copy.deepcopy(a.state_dict())
    g = torch.Generator().manual_seed(5)
    other = {k: (torch.randn(v.shape, generator=g) * 0.05 if v.is_floating_point() else v.clone()) for k, v in _sd().items()}
    b = _stepper(device, other)  # (different weights: everything b computes has to come from what it loads)
    with torch.no_grad():
        b.model.load_state_dict(model_sd)
        b.load_state_dict(step_sd)
    assert b.step_count == a.step_count == 2
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    for k, (x, t, noise) in enumerate(batches[2:], start=3):
        with torch.no_grad():
            la, lb = a.loss_and_grads(x, t, noise), b.loss_and_grads(x, t, noise)
        assert a.loss_scale == b.loss_scale, (k, a.loss_scale, b.loss_scale)
        assert torch.equal(la, lb) and torch.equal(a.gflat, b.gflat), k
        with torch.no_grad():
            a.adam_step()
            b.adam_step()
        assert torch.equal(a.flat, b.flat), k
    assert a.step_count == b.step_count == 4


def test_switch_toggle_does_not_strand_the_f4x4_cache(device):
    """_w44_cache memoises a dispatcher answer that depends on the run-time switches, and the reconstruction guard flips them in
    the training process.  Three B = 64 steps: switches as they are, split-f16 off, on again.  Gradients at the bar in all three;
    the third step launches what the first did (a stale False would drop the wino44h keys); the middle one launches no more plain
    direct convolutions than the first (a stale True packs only the F(4x4) form and the dispatcher falls to conv_direct)."""
    from ddpm_ood_amd import _lib

    st = _stepper(device, _sd())
    ref = _AtenRef(device)
    reports = []

    def step(x, t, noise, what):
        _, grads = ref(_snapshot(st.model), x, t, noise)

        def run():
            st.loss_and_grads(x, t, noise)
            st.adam_step()  # (leaves the gradient buffer alone: it is compared below)

        with torch.no_grad():
            _, launches = _profiled(run)
        worst, name = _check_gradients(st, grads, what)
        print(f"{what}: worst gradient error {worst:.2e} ({name}); wino44h launches "
              f"{sum(v for k, v in launches.items() if k.startswith('conv3x3_wino44h'))}, conv_direct {launches.get('conv_direct', 0)}")
        reports.append(launches)

    batches = _batches(device, (64, 64, 64), seed=61)
    assert _lib.split_f16() is True
    try:
        step(*batches[0], "switches as they are")
        assert _lib.set_split_f16(False) is True
        step(*batches[1], "split-f16 off")
        _lib.set_split_f16(True)
        step(*batches[2], "split-f16 on again")
    finally:
        _lib.set_split_f16(True)
    base, mid, last = reports
    assert any(k.startswith("conv3x3_wino44h") for k in base), sorted(base)
    assert not any(k.startswith("conv3x3_wino44h") for k in mid), sorted(mid)
    assert last == base, {k: (base.get(k), last.get(k)) for k in set(base) | set(last) if base.get(k) != last.get(k)}
    assert mid.get("conv_direct", 0) <= base.get("conv_direct", 0), (mid.get("conv_direct", 0), base.get("conv_direct", 0))
    assert st.overflow_retries == 0


# ---- the loss-scale controller ---------------------------------------------------------------------------------------------

def test_a_nan_batch_costs_one_pass_and_no_scale(device):
    """A batch with one NaN pixel (NaN arithmetic is not a fault): the loss comes back non-finite, the backward ran once, the
    retry counters and the scale are what they were, and the gradient buffer holds the non-finite gradient -- never the previous
    step's finite one, which adam_step would apply.  The clean step after it needs no retry and gives the bits a fresh stepper at
    the same scale gives."""
    (x0, t0, n0), (x1, t1, n1), (x2, t2, n2) = _batches(device, (64, 64, 64), seed=71)
    st = _stepper(device, _sd())
    with torch.no_grad():
        st.loss_and_grads(x0, t0, n0)
        assert bool(torch.isfinite(st.gflat).all())
        st.adam_step()
    before = (st.overflow_retries, st.fp32_dgrad_steps, st.loss_scale)
    assert before[:2] == (0, 0) and before[2] >= 2.0 ** 20
    calls = []
    real = st.backward

    def spy(dpred):
        calls.append(1)
        return real(dpred)

    st.backward = spy
    x1 = x1.clone()
    x1[5, 0, 7, 9] = float("nan")
    with torch.no_grad():
        loss = st.loss_and_grads(x1, t1, n1)
    assert not bool(torch.isfinite(loss).all())
    assert len(calls) <= 1, len(calls)
    assert (st.overflow_retries, st.fp32_dgrad_steps, st.loss_scale) == before
    assert not bool(torch.isfinite(st.gflat).all())
    # (no adam_step: the trainer's business; the parameters are still the ones after step 1)
    del calls[:]
    with torch.no_grad():
        st.loss_and_grads(x2, t2, n2)
    assert len(calls) == 1 and (st.overflow_retries, st.fp32_dgrad_steps, st.loss_scale) == before
    assert bool(torch.isfinite(st.gflat).all())

    def same_scale(s):
        s.loss_scale = before[2]

    fresh = _stepper(device, _snapshot(st.model), setup=same_scale)
    with torch.no_grad():
        fresh.loss_and_grads(x2, t2, n2)
    assert fresh.loss_scale == before[2] and fresh.overflow_retries == 0
    assert torch.equal(st.gflat, fresh.gflat)


@pytest.mark.parametrize("order", [(4, 64), (64, 4)], ids=["4-then-64", "64-then-4"])
def test_scale_survives_a_change_of_batch_size(device, monkeypatch, order):
    """The second step of a stepper whose first batch had another size: its distance from the fp32-pipe form (DDPM_TRAIN_DGRAD=wino,
    as test_loss_scale_of_the_f16_input_gradients_and_its_overflow_retry measures it) is at most twice that of a fresh stepper
    that derived its scale from this batch (2: a scale one or two binades from the derived one), and nothing overflowed."""
    b1, b2 = _batches(device, order, seed=81)
    st = _stepper(device, _sd())
    with torch.no_grad():
        st.loss_and_grads(*b1)
        st.adam_step()
        first_scale = st.loss_scale
        sd = _snapshot(st.model)
        st.loss_and_grads(*b2)
    assert st.scale_adaptive and st.dgrad_form == "wino44h"
    fresh = _stepper(device, sd)
    with torch.no_grad():
        fresh.loss_and_grads(*b2)
    monkeypatch.setenv("DDPM_TRAIN_DGRAD", "wino")
    fp32 = _stepper(device, sd)
    monkeypatch.delenv("DDPM_TRAIN_DGRAD")
    assert fp32.dgrad_form == "wino" and not fp32.scale_adaptive
    with torch.no_grad():
        fp32.loss_and_grads(*b2)
    ref = fp32.gflat
    scale = float(ref.abs().max())
    err = float((st.gflat - ref).abs().max()) / scale
    err_fresh = float((fresh.gflat - ref).abs().max()) / scale
    print(f"B = {order[0]} then {order[1]}: scale 2^{int(math.log2(first_scale))} -> 2^{int(math.log2(st.loss_scale))} "
          f"(fresh 2^{int(math.log2(fresh.loss_scale))}); err {err:.3e}, err_fresh {err_fresh:.3e}")
    assert st.overflow_retries == 0 and fresh.overflow_retries == 0
    assert err <= 2 * err_fresh, (err, err_fresh)
