"""CPU: the host side of sampling -- DDPMScheduler.set_timesteps / step coefficients against a float64 evaluation of the closed
form, the DiffusionInferer loop on stubs, the sample.py flags and the PNG writer through data.py's own reader."""

import math

import numpy as np
import pytest
import torch

SCHEDULES = [("linear_beta", {}), ("scaled_linear_beta", dict(beta_start=0.0015, beta_end=0.0195)), ("sigmoid_beta", {}),
             ("cosine", {})]


def _closed_form(s, t, variance_type):
    """float64, straight from the issue's formulas, on the scheduler's tables as they are now."""
    ac = s.alphas_cumprod.double().numpy()
    beta, alpha = float(s.betas.double()[t]), float(s.alphas.double()[t])
    a_t = float(ac[t])
    a_p = float(ac[t - 1]) if t > 0 else 1.0
    c0 = math.sqrt(a_p) * beta / (1 - a_t)
    ct = math.sqrt(alpha) * (1 - a_p) / (1 - a_t)
    var = max((1 - a_p) / (1 - a_t) * beta, 1e-20) if variance_type == "fixed_small" else beta
    return math.sqrt(a_t), math.sqrt(1 - a_t), c0, ct, (0.0 if t == 0 else math.sqrt(var))


@pytest.mark.parametrize("schedule,kw", SCHEDULES)
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("variance_type", ["fixed_small", "fixed_large"])
def test_step_coefficients_match_the_closed_form(schedule, kw, shift, variance_type):
    from ddpm_ood_amd import DDPMScheduler
    from ddpm_ood_amd.trainer import snr_shift_tables

    s = DDPMScheduler(num_train_timesteps=1000, schedule=schedule, variance_type=variance_type, **kw)
    before = s.step_coefficients(500)
    if shift:
        snr_shift_tables(s, 3.0)  # reassigns betas / alphas / alphas_cumprod: the memo must not serve the old tables
        assert s.step_coefficients(500) != before
    for t in range(1000):
        got = s.step_coefficients(t)
        want = _closed_form(s, t, variance_type)
        for g, w in zip(got, want):
            # what the kernel receives is the fp32 rounding of the value: half an ulp of fp32, relative 2^-24
            assert abs(float(np.float32(g)) - w) <= 2.0 ** -24 * abs(w) + 1e-45, (t, got, want)
        assert s.step_coefficients(t) is got  # memoised
    assert s.step_coefficients(0)[4] == 0.0  # the last step adds no noise
    if variance_type == "fixed_large":
        for t in (1, 500, 999):
            assert s.step_coefficients(t)[4] == math.sqrt(float(s.betas.double()[t]))
    else:
        assert 0.0 < s.step_coefficients(1)[4] < math.sqrt(float(s.betas[1]))


def test_memo_follows_repeated_table_reassignment():
    """Three reassignments in a row (the earlier tables are freed, so a later tensor may take one of their id()s): every call
    answers from the tables as they are NOW, for the ancestral and the PLMS coefficients, and no entry of a dropped table stays."""
    from ddpm_ood_amd import DDPMScheduler, PNDMScheduler
    from ddpm_ood_amd.trainer import snr_shift_tables

    kw = dict(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    d, p = DDPMScheduler(**kw), PNDMScheduler(skip_prk_steps=True, **kw)
    seen = set()
    for shift in (2.0, 3.0, 0.5):
        for s in (d, p):
            snr_shift_tables(s, shift)
        got = d.step_coefficients(500)
        for g, w in zip(got, _closed_form(d, 500, "fixed_small")):
            assert abs(float(np.float32(g)) - w) <= 2.0 ** -24 * abs(w)
        a_t, a_p = float(p.alphas_cumprod[500]), float(p.alphas_cumprod[490])
        pl = p.plms_coefficients(500, 490)
        assert pl[0] == pytest.approx(math.sqrt(a_p / a_t), rel=1e-6) and pl[1] == pytest.approx(a_p - a_t, rel=1e-5)
        assert len(d._coef_cache) == 1 and len(p._coef_cache) == 1
        assert (got, pl) not in seen
        seen.add((got, pl))


def test_pndm_reset_forgets_the_history_and_keeps_the_timesteps():
    from ddpm_ood_amd import PNDMScheduler

    for form, n in (("monai", 10), ("diffusers", 11)):
        s = PNDMScheduler(skip_prk_steps=True, timestep_list=form)
        s.set_timesteps(10)
        ts = s.timesteps.tolist()
        assert len(ts) == n
        s.ets, s.counter, s.cur_sample = [1, 2], 5, object()
        s.reset()
        assert s.ets == [] and s.counter == 0 and s.cur_sample is None
        assert s.timesteps.tolist() == ts and s.num_inference_steps == n


def test_set_timesteps_and_constructor_checks():
    from ddpm_ood_amd import DDPMScheduler

    s = DDPMScheduler()
    assert s.variance_type == "fixed_small" and s.clip_sample is True and s.prediction_type == "epsilon"
    assert s.timesteps.tolist() == list(range(999, -1, -1))
    s.set_timesteps(25)
    assert s.timesteps.tolist() == list(range(960, -1, -40)) and s.num_inference_steps == 25
    s.set_timesteps(1000)
    assert s.timesteps.tolist() == list(range(999, -1, -1))
    s.set_timesteps(3)
    assert s.timesteps.tolist() == [666, 333, 0]
    with pytest.raises(ValueError, match="cannot be larger"):
        s.set_timesteps(1001)
    for vt in ("learned", "learned_range"):
        with pytest.raises(NotImplementedError):
            DDPMScheduler(variance_type=vt)
    with pytest.raises(ValueError):
        DDPMScheduler(variance_type="nonsense")
    with pytest.raises(ValueError):
        DDPMScheduler(prediction_type="nonsense")
    with pytest.raises(ValueError):
        s.step_coefficients(1000)


def test_step_refuses_host_tensors():
    """No quiet fall-back: the step is a HIP kernel, a CPU tensor is an error."""
    from ddpm_ood_amd import DDPMScheduler

    s = DDPMScheduler()
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        s.step(torch.zeros(2, 1, 4, 4), 10, torch.zeros(2, 1, 4, 4))


def test_stream_addressing():
    from ddpm_ood_amd.scheduler import sampling_key, sampling_streams

    assert sampling_streams([0, 1, 7], 999) == [999, 65536 + 999, 7 * 65536 + 999]
    assert sampling_streams(range(2), 1000) == [1000, 65536 + 1000]  # x_T: t = num_train_timesteps
    with pytest.raises(ValueError):
        sampling_streams([0], 65536)
    # the training step keys its noise with seed * 7919 + rank < 2^63: the sampling key always has bit 63 set
    for seed in (0, 2, 12345, 2 ** 40):
        k = sampling_key(seed)
        assert k >> 63 == 1 and k & (2 ** 63 - 1) == seed and k < 2 ** 64
        assert all(k != s * 7919 + r for s in (0, 2, seed) for r in range(8))
    assert sampling_key(3) != sampling_key(4)


class _StubModel:
    def __init__(self, log):
        self.log = log

    def __call__(self, x, timesteps=None):
        assert timesteps.dtype == torch.int64 and timesteps.shape == (x.shape[0],)
        assert len(set(timesteps.tolist())) == 1
        self.log.append(("model", int(timesteps[0]), float(x.flatten()[0])))
        return x * 0 + 1.0


class _StubAncestral:
    """step(model_output, timestep, sample, *, seed, row_ids) like DDPMScheduler"""

    def __init__(self, timesteps, log):
        self.timesteps = torch.tensor(timesteps)
        self.log = log

    def step(self, model_output, timestep, sample, *, seed=0, row_ids=None):
        self.log.append(("step", int(timestep), seed, tuple(row_ids)))
        return sample + model_output, None


class _StubPlain:
    """step(model_output, timestep, sample) like PNDMScheduler: takes no seed"""

    def __init__(self, timesteps, log):
        self.timesteps = torch.tensor(timesteps)
        self.log = log

    def step(self, model_output, timestep, sample):
        self.log.append(("step", int(timestep)))
        return sample + model_output, None


def test_inferer_loop_order_and_intermediates():
    from ddpm_ood_amd import DiffusionInferer

    log = []
    ts = [900, 700, 500, 350, 200, 100, 0]
    inf = DiffusionInferer()
    x0 = torch.zeros(3, 1, 2, 2)
    out, inter = inf.sample(x0, _StubModel(log), _StubAncestral(ts, log), save_intermediates=True, intermediate_steps=100,
                            seed=11, row_ids=[4, 5, 6])
    assert [e[0] for e in log] == ["model", "step"] * len(ts)  # one forward, then one step, per timestep, in order
    assert [e[1] for e in log[0::2]] == ts and [e[1] for e in log[1::2]] == ts
    assert [e[2] for e in log[0::2]] == [float(i) for i in range(len(ts))]  # the model sees the previous step's output
    assert all(e[2:] == (11, (4, 5, 6)) for e in log[1::2])
    assert torch.equal(out, x0 + len(ts))
    # an intermediate after every step with t % 100 == 0: all but t = 350
    assert [float(i.flatten()[0]) for i in inter] == [1.0, 2.0, 3.0, 5.0, 6.0, 7.0]
    out2 = inf.sample(x0, _StubModel([]), _StubAncestral(ts, []))
    assert torch.is_tensor(out2) and torch.equal(out2, out)
    log.clear()
    inf.sample(x0, _StubModel([]), _StubAncestral([5, 0], log))
    assert log == [("step", 5, 0, (0, 1, 2)), ("step", 0, 0, (0, 1, 2))]  # defaults: seed 0, row ids 0 .. B - 1
    # a scheduler whose step takes no seed is called without one; the constructor's scheduler is the default
    log.clear()
    out3 = DiffusionInferer(_StubPlain(ts, log)).sample(x0, _StubModel([]), seed=5)
    assert log == [("step", t) for t in ts] and torch.equal(out3, out)
    with pytest.raises(ValueError):
        DiffusionInferer().sample(x0, _StubModel([]))


def test_inferer_accepts_the_pndm_scheduler_signature():
    """PNDMScheduler.step(model_output, timestep, sample) has no seed / row_ids: the inferer must not pass them (the step itself
    is a HIP kernel: here only its host side up to the device check runs)."""
    import inspect

    from ddpm_ood_amd import DiffusionInferer, PNDMScheduler

    s = PNDMScheduler(skip_prk_steps=True)
    s.set_timesteps(10)
    assert list(inspect.signature(s.step).parameters) == ["model_output", "timestep", "sample"]
    calls = []
    s.step_plms = lambda mo, t, x: (calls.append(t), x - mo)[1]
    out = DiffusionInferer().sample(torch.zeros(2, 1, 2, 2), _StubModel([]), s, seed=3, row_ids=[8, 9])
    assert calls == [900, 800, 700, 600, 500, 400, 300, 200, 100, 0] and torch.equal(out, torch.full((2, 1, 2, 2), -10.0))


def test_sample_cli_defaults():
    import sample
    import train_ddpm

    a = sample.parse_args([])
    assert (a.num_samples, a.batch_size, a.seed, a.scheduler, a.num_inference_steps, a.out) == (8, 8, 2, "ddpm", None, None)
    t = train_ddpm.parse_args([])
    for name in ("output_dir", "model_name", "model_type", "spatial_dimension", "is_grayscale", "image_size", "vqvae_checkpoint",
                 "latent_pad", "beta_schedule", "beta_start", "beta_end", "prediction_type", "snr_shift", "b_scale",
                 "ddpm_checkpoint_epoch", "seed"):
        assert getattr(a, name) == getattr(t, name), name  # the model flags of train_ddpm.py, same defaults
    a = sample.parse_args(["--scheduler", "pndm", "--num_inference_steps", "100", "--latent_pad", "(1,1,0,0)", "--num_samples", "5",
                           "--out", "/tmp/x", "--image_size", "32"])
    assert a.scheduler == "pndm" and a.num_inference_steps == 100 and a.latent_pad == (1, 1, 0, 0) and a.num_samples == 5
    with pytest.raises(SystemExit):
        sample.parse_args(["--scheduler", "ddim"])


def test_sampling_scheduler_factory():
    from ddpm_ood_amd import DDPMScheduler, PNDMScheduler
    from ddpm_ood_amd.sampling import make_sampling_scheduler

    kw = dict(prediction_type="epsilon", beta_schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    d = make_sampling_scheduler("ddpm", **kw)
    assert isinstance(d, DDPMScheduler) and len(d.timesteps) == 1000
    p = make_sampling_scheduler("pndm", **kw)
    assert isinstance(p, PNDMScheduler) and len(p.timesteps) == 100
    shifted = make_sampling_scheduler("ddpm", snr_shift=3.0, num_inference_steps=25, **kw)
    assert len(shifted.timesteps) == 25 and not torch.equal(shifted.alphas_cumprod, d.alphas_cumprod)
    with pytest.raises(ValueError):
        make_sampling_scheduler("ddim", **kw)


@pytest.mark.parametrize("shape", [(9, 13), (9, 13, 3), (1, 1), (28, 28, 1)])
def test_png_writer_round_trips_through_the_reader(tmp_path, shape):
    from ddpm_ood_amd.data import read_png, write_png

    a = np.random.default_rng(0).integers(0, 256, size=shape, dtype=np.uint8)
    write_png(tmp_path / "a.png", a)
    back = read_png(str(tmp_path / "a.png"))
    want = a[..., 0] if a.ndim == 3 and a.shape[2] == 1 else a
    assert back.dtype == np.float32 and back.shape == want.shape and np.array_equal(back, want.astype(np.float32))
    with pytest.raises(ValueError):
        write_png(tmp_path / "b.png", a.astype(np.float32))


def test_sample_grid_layouts(tmp_path):
    from ddpm_ood_amd.data import read_png
    from ddpm_ood_amd.sampling import sample_grid, write_samples

    x = np.zeros((8, 1, 4, 6), dtype=np.float32)
    for i in range(8):
        x[i] = i / 8
    g = sample_grid(x)
    assert g.shape == (2 * 4, 4 * 6) and g.dtype == np.uint8  # 2 x 4 tiles, row-major
    assert g[0, 0] == 0 and g[0, 6] == round(255 / 8) and g[4, 0] == round(255 * 4 / 8) and g[7, 23] == round(255 * 7 / 8)
    assert sample_grid(np.zeros((4, 3, 5, 5), dtype=np.float32)).shape == (10, 10, 3)
    assert sample_grid(np.zeros((7, 1, 5, 5), dtype=np.float32)).shape == (10, 20)  # ragged: padded with a black tile
    v = np.zeros((2, 1, 4, 5, 8), dtype=np.float32)
    v[1, 0, :, :, 4] = 1.0
    gv = sample_grid(v)  # one row per volume, slices 2 / 4 / 6 of the last axis
    assert gv.shape == (2 * 4, 3 * 5) and gv[4:, 5:10].min() == 255 and gv[:4].max() == 0 and gv[4:, :5].max() == 0
    write_samples(tmp_path / "o", "samples", x)
    assert np.array_equal(np.load(tmp_path / "o" / "samples.npy"), x)
    assert np.array_equal(read_png(str(tmp_path / "o" / "samples.png")), g.astype(np.float32))


def test_val_grids_are_opt_in_and_no_new_training_flag():
    """DDPM_VAL_SAMPLES is read on the Python side; train_ddpm.py grows no flag for it."""
    import inspect

    import train_ddpm
    from ddpm_ood_amd import train

    assert not any("sample" in name for name, _, _ in train_ddpm._FLAGS)
    src = inspect.getsource(train.DDPMTrainer.val_epoch)
    assert 'os.environ.get("DDPM_VAL_SAMPLES", "0")' in src
