"""Host: the retry and scale policy of NativeUNetStep.loss_and_grads (ddpm_ood_amd/train_native.py) driven by a scripted sequence
of "non-finite after the unscale pass?" answers -- no GPU, no kernel.  The stepper is built with object.__new__ and its forward,
backward and the four library calls of the step (T.mse_loss_grad, T.axpby, T.scale_check_, _lib.status_read) are stubs that
record what the policy did: how many backward passes, at which scale, on which input-gradient form.  What tests/test_gpu_train.py
pins on the device (3 retries, one fp32-pipe step, 2^52 from 2^60) is pinned here as a sequence too, beside the cases no device
test can script: a gradient that stays non-finite on the fp32 pipe, regrowth, and a batch-size change."""

import pytest

N4 = 4 * 32 * 32      # elements of a batch of four 1 x 32 x 32 predictions: the derived scale is 2^(11 + 8)
N64 = 64 * 32 * 32


class _Pred:
    def __init__(self, n):
        self._n = n

    def numel(self):
        return self._n


@pytest.fixture
def stepper(monkeypatch):
    """-> make(answers, loss=..., numel=...): a stubbed stepper; st.script answers each status read (True: the flag is set),
    st.passes records (scale the backward ran at, dgrad_form, _scaled) per backward pass."""
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd import train_native as TN

    def make(loss_scale=None, dgrad_form="wino44h"):
        st = object.__new__(TN.NativeUNetStep)
        st.dgrad_form, st.loss_scale = dgrad_form, loss_scale
        st.scale_adaptive = loss_scale is None and dgrad_form == "wino44h"
        if st.loss_scale is None and not st.scale_adaptive:
            st.loss_scale = 1.0
        st._scale_exp, st._scaled, st._clean_steps, st._tape = None, False, 0, None
        st.overflow_retries = st.fp32_dgrad_steps = 0
        st.script, st.passes, st.loss_value, st.numel, st.reads, st.loss_reads = [], [], 0.5, N4, 0, 0

        def forward(noisy, timesteps):
            st._tape = "tape"
            return _Pred(st.numel)

        def backward(dpred):
            assert st._tape == "tape"  # every repeat runs on the forward's tape
            st.passes.append((dpred, st.dgrad_form, st._scaled))
            st._tape = None

        st.forward, st.backward = forward, backward
        return st

    class _Loss:  # the 1-element device tensor: reading it is a synchronising copy, which a clean step must not pay
        def __init__(self, st):
            self.st = st

        def __float__(self):
            self.st.loss_reads += 1
            return float(self.st.loss_value)

    current = {}

    def mse_loss_grad(pred, target):
        return _Loss(current["st"]), 1.0  # dpred0 = 1: the scaled dpred IS the scale

    def axpby(x, y, alpha, beta, out=None):
        assert y is None and beta == 0.0
        return x * alpha

    def scale_check_(g, alpha):
        current["unscale"].append(alpha)

    def status_read(clear=True):
        st = current["st"]
        st.reads += 1
        assert clear
        return _lib.STATUS_NONFINITE_GRAD if st.script.pop(0) else 0

    monkeypatch.setattr(TN.T, "mse_loss_grad", mse_loss_grad)
    monkeypatch.setattr(TN.T, "axpby", axpby)
    monkeypatch.setattr(TN.T, "scale_check_", scale_check_)
    monkeypatch.setattr(_lib, "status_read", status_read)

    def step(st, answers, loss=0.5, numel=None):
        """One loss_and_grads; -> the backward passes of this step [(scale, dgrad_form, _scaled)]."""
        current["st"], current["unscale"] = st, []
        st.gflat = None
        st.script, st.loss_value = list(answers), loss
        if numel is not None:
            st.numel = numel
        before = len(st.passes)
        out = st.loss_and_grads(None, None, None)
        assert isinstance(out, _Loss) and out.st is st  # the loss comes back as the device gave it
        assert not st.script, "the policy read the status word fewer times than scripted"
        passes = st.passes[before:]
        # every pass is unscaled by exactly the factor it was scaled with
        assert current["unscale"] == [1.0 / s for s, _, _ in passes]
        return passes

    make.step = step
    return make


def test_clean_steps_double_the_scale_after_the_growth_interval(stepper):
    from ddpm_ood_amd.train_native import NativeUNetStep

    st = stepper()
    n = NativeUNetStep.SCALE_GROWTH_INTERVAL
    assert n == 2000
    for i in range(n - 1):
        passes = stepper.step(st, [False])
        assert passes == [(2.0 ** 19, "wino44h", True)]
    assert st.loss_scale == 2.0 ** 19 and st._clean_steps == n - 1
    stepper.step(st, [False])
    assert st.loss_scale == 2.0 ** 20 and st._clean_steps == 0
    assert stepper.step(st, [False]) == [(2.0 ** 20, "wino44h", True)]
    assert st.overflow_retries == 0 and st.fp32_dgrad_steps == 0
    assert st.loss_reads == 0  # the loss is never read back on a clean step


def test_one_overflow_drops_the_scale_by_16_and_repeats_once(stepper):
    st = stepper()
    for _ in range(5):
        stepper.step(st, [False])
    passes = stepper.step(st, [True, False])
    assert passes == [(2.0 ** 19, "wino44h", True), (2.0 ** 15, "wino44h", True)]
    assert st.loss_scale == 2.0 ** 15 and st.overflow_retries == 1 and st.fp32_dgrad_steps == 0 and st.dgrad_form == "wino44h"
    assert st._clean_steps == 1  # the count starts again with this step
    assert stepper.step(st, [False]) == [(2.0 ** 15, "wino44h", True)]  # the lowered scale is kept


def test_three_overflows_end_on_the_fp32_pipe_for_this_step_only(stepper):
    """tests/test_gpu_train.py's sequence: 2^60 -> 2^56 -> 2^52, then the input gradients on the fp32 pipe at scale 1."""
    st = stepper()
    st.loss_scale = 2.0 ** 60
    passes = stepper.step(st, [True, True, True, False], numel=N64)
    assert passes == [(2.0 ** 60, "wino44h", True), (2.0 ** 56, "wino44h", True), (2.0 ** 52, "wino44h", True), (1.0, "wino", False)]
    assert st.overflow_retries == 3 and st.fp32_dgrad_steps == 1 and st.loss_scale == 2.0 ** 52
    assert st.dgrad_form == "wino44h"  # restored
    st.loss_scale = 2.0 ** 24
    assert stepper.step(st, [False]) == [(2.0 ** 24, "wino44h", True)]
    assert st.fp32_dgrad_steps == 1


def test_a_gradient_still_non_finite_on_the_fp32_pipe_gives_the_scale_back(stepper):
    """A genuine non-finite gradient under a finite loss: the three repeats cannot be avoided (nothing tells it from an overflow
    before the fp32 pipe has had its turn), but the scale and the clean-step count are what the step started with."""
    st = stepper()
    for _ in range(7):
        stepper.step(st, [False])
    passes = stepper.step(st, [True, True, True, True])
    assert [p[1] for p in passes] == ["wino44h", "wino44h", "wino44h", "wino"] and passes[-1][0] == 1.0
    assert st.loss_scale == 2.0 ** 19 and st._clean_steps == 7 and st.dgrad_form == "wino44h"
    assert st.loss_reads == 1  # read once, on the first flagged pass
    assert stepper.step(st, [False]) == [(2.0 ** 19, "wino44h", True)]
    assert st._clean_steps == 8


@pytest.mark.parametrize("loss", [float("nan"), float("inf")])
def test_a_non_finite_loss_is_not_retried(stepper, loss):
    st = stepper()
    for _ in range(3):
        stepper.step(st, [False])
    passes = stepper.step(st, [True], loss=loss)
    assert len(passes) == 1 and st.reads == 4
    assert st.overflow_retries == 0 and st.fp32_dgrad_steps == 0 and st.loss_scale == 2.0 ** 19 and st._clean_steps == 3
    assert st.dgrad_form == "wino44h"
    assert stepper.step(st, [False]) == [(2.0 ** 19, "wino44h", True)]


def test_the_scale_follows_the_element_count_of_each_batch(stepper):
    """A ragged last batch and a change of batch size move the scale with n: what an overflow took off stays off, relative to
    the batch; a scale somebody set before the first step is taken as it is."""
    st = stepper()
    assert stepper.step(st, [False], numel=N4) == [(2.0 ** 19, "wino44h", True)]
    assert stepper.step(st, [False], numel=N64) == [(2.0 ** 23, "wino44h", True)]
    assert stepper.step(st, [False], numel=37 * 1024) == [(2.0 ** 22, "wino44h", True)]  # floor(log2(37 * 512)) = 14
    assert stepper.step(st, [False], numel=N4) == [(2.0 ** 19, "wino44h", True)]
    assert [p[0] for p in stepper.step(st, [True, False], numel=N4)] == [2.0 ** 19, 2.0 ** 15]
    assert stepper.step(st, [False], numel=N64) == [(2.0 ** 19, "wino44h", True)]  # 2^4 under the derived 2^23
    fresh = stepper()
    assert stepper.step(fresh, [False], numel=N64) == [(2.0 ** 23, "wino44h", True)]
    given = stepper()
    given.loss_scale = 2.0 ** 21
    assert stepper.step(given, [False], numel=N64) == [(2.0 ** 21, "wino44h", True)]
    assert stepper.step(given, [False], numel=N4) == [(2.0 ** 17, "wino44h", True)]


def test_a_fixed_scale_and_the_fp32_form_never_repeat(stepper):
    """DDPM_TRAIN_LOSS_SCALE=<n> and DDPM_TRAIN_DGRAD=wino: one pass whatever the status word says, the scale never moves."""
    fixed = stepper(loss_scale=4096.0)
    assert stepper.step(fixed, [True], numel=N64) == [(4096.0, "wino44h", True)]
    assert stepper.step(fixed, [False], numel=N4) == [(4096.0, "wino44h", True)]
    assert fixed.loss_scale == 4096.0 and fixed.overflow_retries == 0
    fp32 = stepper(dgrad_form="wino")
    assert stepper.step(fp32, [True]) == [(1.0, "wino", False)]
    assert fp32.loss_scale == 1.0 and fp32.overflow_retries == 0 and fp32.loss_reads == 0


def test_the_f4x4_answer_cache_is_keyed_on_the_switch_state(monkeypatch):
    """_takes_wino44h memoises a dispatcher answer that depends on the run-time switches: a change of the master switch or a
    reload of the DDPM_* variables asks again (a stale answer costs the F(4x4) kernel, or drops to the plain direct one)."""
    from ddpm_ood_amd import _lib
    from ddpm_ood_amd import train_native as TN

    state = {"gen": 0, "split": True}
    asked = []

    def takes(shape, cout):
        asked.append((shape, cout, state["split"]))
        return state["split"]

    monkeypatch.setattr(_lib, "switch_state", lambda: (state["gen"], state["split"]))
    monkeypatch.setattr(TN.ops, "conv_takes_wino44h", takes)
    st = object.__new__(TN.NativeUNetStep)
    st._w44_cache, st._w44_state = {}, None
    shape = (64, 128, 32, 32)
    assert st._takes_wino44h(shape, 128) is True and st._takes_wino44h(shape, 128) is True and len(asked) == 1
    state["split"] = False
    assert st._takes_wino44h(shape, 128) is False and len(asked) == 2
    state["split"] = True
    assert st._takes_wino44h(shape, 128) is True and len(asked) == 3
    state["gen"] += 1  # reload_env
    assert st._takes_wino44h(shape, 128) is True and len(asked) == 4
    assert st._takes_wino44h(shape, 256) is True and st._takes_wino44h(shape, 256) is True and len(asked) == 5


def test_switch_state_counts_reloads_and_reads_the_master_switch_back():
    from ddpm_ood_amd import _lib

    lib = _lib.load()
    s0 = _lib.switch_state()
    _lib.reload_env()
    s1 = _lib.switch_state()
    assert s1[0] == s0[0] + 1 and s1[1] == s0[1]
    prev = lib.ddpm_set_split_f16(0)  # past the wrapper, as some callers do
    try:
        assert _lib.switch_state() == (s1[0], False)
    finally:
        lib.ddpm_set_split_f16(prev)
    assert _lib.switch_state() == (s1[0], bool(prev))
