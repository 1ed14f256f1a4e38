"""CPU: the restatement of Blur Integrated Gradients (tests/blur_ig_ref.py) against a literal transcription of saliency's BlurIG.GetMask
loop on scipy.ndimage.gaussian_filter, against the closed form of a linear model and against its own completeness error; the host side
of brainxai.blur_ig (schedule, taps, table) against the restatement; the argument checks of brainxai.blur_ig / blur_path / gaussian_blur
that run before anything reaches a device; and the limits of the bx_blur_rows / bx_blurig_* entry points."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.ndimage import _filters

import brainxai
from brainxai import _lib
from brainxai import explain as X
from tests import blur_ig_ref as R

BX_EINVAL, BX_EUNSUPPORTED = -1, -6


def _recorder(monkeypatch):
    reached = []

    class Recorder:
        def __getattr__(self, name):
            def call(*args):
                reached.append(name)
                raise RuntimeError(f"{name} called")
            return call
    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: SimpleNamespace(cuda_stream=0))
    return reached


# ---- saliency's loop, transcribed ---------------------------------------------------------------------------------------------------------
def _saliency_blur(image, sigma):
    """saliency.core.blur_ig.gaussian_blur: an image [H,W,C], the channels are not blurred."""
    if sigma == 0:
        return image
    return ndimage.gaussian_filter(image, sigma=[sigma, sigma, 0], mode="constant")


def _saliency_blur_ig(x_value, grad_fn, max_sigma=50, steps=100, grad_step=0.01, sqrt=False):
    """BlurIG.GetMask of PAIR's saliency (core/blur_ig.py), batch size 1: x_value [H,W,C] fp64, grad_fn(x_step) -> the gradient of
    the explained output by x_step.  Returns (attribution, sigmas, step_vector_diff, the x_step list, the gaussian_gradient list)."""
    if sqrt:
        sigmas = [math.sqrt(float(i) * max_sigma / float(steps)) for i in range(0, steps + 1)]
    else:
        sigmas = [float(i) * max_sigma / float(steps) for i in range(0, steps + 1)]
    step_vector_diff = [sigmas[i + 1] - sigmas[i] for i in range(0, steps)]
    total_gradients = np.zeros_like(x_value, dtype=np.float64)
    x_steps, gaussian_gradients = [], []
    for i in range(steps):
        x_step = _saliency_blur(x_value, sigmas[i])
        gaussian_gradient = (_saliency_blur(x_value, sigmas[i] + grad_step) - x_step) / grad_step
        x_steps.append(x_step)
        gaussian_gradients.append(gaussian_gradient)
        tmp = step_vector_diff[i] * np.multiply(gaussian_gradient, grad_fn(x_step))
        total_gradients += tmp
    total_gradients *= -1.0
    return total_gradients, sigmas, step_vector_diff, x_steps, gaussian_gradients


class _Smooth(torch.nn.Module):
    """A small fixed differentiable model of an image [*, C, H, W]: log-softmax of a linear map of tanh(x)."""

    def __init__(self, shape, K=3, seed=5):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(int(np.prod(shape)), K, generator=g, dtype=torch.float64) * 0.2)

    def forward(self, x):
        return torch.log_softmax(torch.tanh(x.flatten(1)) @ self.w, dim=1)


def _grad_of(model, c):
    def fn(x_step):                                                     # [H,W,C] -> [H,W,C]
        xi = torch.from_numpy(np.ascontiguousarray(x_step.transpose(2, 0, 1)))[None].requires_grad_(True)
        (g,) = torch.autograd.grad(model(xi)[0, c], xi)
        return g[0].numpy().transpose(1, 2, 0)
    return fn


@pytest.mark.parametrize("sqrt", [False, True])
def test_restatement_equals_saliencys_loop(sqrt):
    C, H, W, n, max_sigma, eps = 2, 16, 24, 7, 6.0, 0.01
    x = np.random.default_rng(3).standard_normal((1, C, H, W))
    model = _Smooth((C, H, W))
    sig = R.sigmas(n, max_sigma, sqrt)
    w = R.weights(sig)
    rows, deriv = R.path(x, sig[:n], eps, "hw", dtype=np.float64)
    vals, _ = R.values(model, rows, deriv, w)
    for c in range(3):
        want, s_sig, s_diff, x_steps, g_grads = _saliency_blur_ig(x[0].transpose(1, 2, 0), _grad_of(model, c), max_sigma, n, eps, sqrt)
        assert s_sig == sig and np.array_equal(-np.array(s_diff), w), "schedule and weights must be saliency's exactly"
        for i in range(n):
            lit_x, lit_d = x_steps[i].transpose(2, 0, 1), g_grads[i].transpose(2, 0, 1)
            assert np.abs(rows[0, i] - lit_x).max() <= 1e-13 * np.abs(lit_x).max()
            if R.radius(sig[i] + eps) == 0:                             # sigma = 0: both blurs are the identity
                assert not lit_d.any() and not deriv[0, i].any()
                continue
            err = np.abs(deriv[0, i] - lit_d).max() / np.abs(lit_d).max()
            assert err <= 1e-12, f"step {i} (sigma {sig[i]}): decomposed D differs from the literal difference by {err:.2e} of its maximum"
        err = np.abs(vals[0, c].numpy() - want.transpose(2, 0, 1)).max() / np.abs(want).max()
        print(f"sqrt={sqrt} class {c}: attribution differs from saliency's loop by {err:.2e} of its maximum")
        assert err <= 1e-11


def test_taps_are_scipys():
    for s in (0.01, 0.37, 0.38, 1.5, 3.75, 6.0, 40.0, 50.01):
        R_ = R.radius(s)
        assert R_ == int(4.0 * s + 0.5)
        if R_ == 0:
            assert np.array_equal(R.taps64(s), [1.0]) and np.array_equal(X.gaussian_taps(s), [1.0])
            continue
        want = _filters._gaussian_kernel1d(s, 0, R_)
        assert np.array_equal(R.taps64(s), want) and np.array_equal(X.gaussian_taps(s), want), s
    assert np.array_equal(R.taps64(0.0), [1.0]) and np.array_equal(X.gaussian_taps(0.0), [1.0])
    assert (R.step_taps(0.37, 0.01)[3], R.step_taps(0.0, 0.01)[3]) == ((1, 2), (0, 0))


@pytest.mark.parametrize("sqrt", [False, True])
def test_host_schedule_and_table_are_the_restatements(sqrt):
    n, max_sigma, eps = 9, 12.5, 0.01
    sig = R.sigmas(n, max_sigma, sqrt)
    assert X.blur_sigmas(n, max_sigma, sqrt) == sig and len(sig) == n + 1 and sig[0] == 0.0
    taps, rad = X.blur_taps(sig[:n], eps)
    want_t, want_r = R.table(sig[:n], eps)
    assert taps.dtype == np.float32 and rad.dtype == np.int32 and np.array_equal(rad, want_r)
    assert np.array_equal(taps.view(np.int32), want_t.view(np.int32))
    assert np.array_equal(taps[0, 0, taps.shape[2] // 2 - 1:taps.shape[2] // 2 + 2], [0.0, 1.0, 0.0]) and not taps[0, 2].any()
    # d is formed in fp64 before the rounding: not the difference of the rounded taps
    i, Rm = 3, taps.shape[2] // 2
    a64, b64 = R.taps64(sig[i]), R.taps64(sig[i] + eps)
    assert len(a64) == len(b64)
    assert np.array_equal(taps[i, 2, Rm - len(a64) // 2:Rm + len(a64) // 2 + 1], ((b64 - a64) / eps).astype(np.float32))
    one, r1 = X.blur_taps([2.0])
    assert one.shape == (1, 3, 17) and np.array_equal(r1, [[8, 8]]) and not one[0, 1:].any()
    assert np.array_equal(one[0, 0], R.taps64(2.0).astype(np.float32))


@pytest.mark.parametrize("axes", ["hw", "h", "w"])
def test_closed_form_of_a_linear_model(axes):
    """F(x) = <a, x>: the gradient is a wherever it is taken, so values = -sum_i Delta_i a (.) D_i exactly."""
    B, C, H, W, n, eps = 2, 2, 9, 11, 5, 0.01
    rng = np.random.default_rng(1)
    x, a = rng.standard_normal((B, C, H, W)), rng.standard_normal((2, C, H, W))

    class Linear(torch.nn.Module):
        def forward(self, xi):
            return xi.flatten(1) @ torch.from_numpy(a).flatten(1).T
    sig = R.sigmas(n, 3.0)
    rows, deriv = R.path(x, sig[:n], eps, axes)
    vals, scale = R.values(Linear(), rows, deriv, R.weights(sig))
    want = np.zeros((B, 2, C, H, W))
    for i in range(n):
        want += -(sig[i + 1] - sig[i]) * a[None] * deriv[:, i][:, None]
    assert np.abs(vals.numpy() - want).max() <= 1e-14 * np.abs(want).max()
    assert bool((scale > 0).all())


def test_completeness_error_halves_with_four_times_the_steps():
    """The left Riemann sum is first order in the step: from n to 4n steps the reference's own delta shrinks about fourfold on a smooth
    model; at least a halving is asserted."""
    C, H, W, eps, max_sigma = 1, 12, 14, 0.01, 4.0
    x = np.random.default_rng(7).standard_normal((2, C, H, W))
    model = _Smooth((C, H, W), seed=9)
    delta = {}
    for n in (8, 32):
        sig = R.sigmas(n, max_sigma)
        rows, deriv = R.path(x, sig[:n], eps, "hw")
        vals, _ = R.values(model, rows, deriv, R.weights(sig))
        drop = R.outputs(model, x) - R.outputs(model, R.blur(x, sig[n], "hw"))
        delta[n] = (vals.flatten(2).sum(2) - drop).abs()
    ratio = float((delta[32] / delta[8]).max())
    print(f"completeness error, 8 -> 32 steps: largest ratio {ratio:.3f}; delta(8) {delta[8].flatten().tolist()}, delta(32) {delta[32].flatten().tolist()}")
    assert ratio <= 0.5


def test_accumulate_and_row_sum_restatements():
    rng = np.random.default_rng(2)
    B, n, per = 3, 5, 7
    g, D = rng.standard_normal((B * n, per)).astype(np.float32), rng.standard_normal((B * n, per)).astype(np.float32)
    w = rng.standard_normal(n)
    one = R.accumulate(g, D, w, B, n)
    two = R.accumulate(g[:7], D[:7], w, B, n)
    two = R.accumulate(g[7:], D[7:], w, B, n, two, row0=7)
    assert np.array_equal(one, two)
    want = (w[None, :, None] * g.reshape(B, n, per).astype(np.float64) * D.reshape(B, n, per)).sum(1)
    assert np.abs(one[:, 0] - want).max() <= 1e-14 * np.abs(want).max()
    v = rng.standard_normal((4, 333)).astype(np.float32)
    assert np.abs(R.sum_rows(v) - v.astype(np.float64).sum(1)).max() <= 1e-12
    assert np.array_equal(R.sum_rows(np.ones((2, 1), dtype=np.float32)), [1.0, 1.0])


# ---- refusals of the drivers ------------------------------------------------------------------------------------------------------------
B, C, H, W, CH, T = 2, 4, 16, 24, 19, 2000


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


BAD = {
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "blur_ig: unknown input"),
    "input_none_eeg": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "input_none_spec": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "axes_unknown": ("multimodal", dict(axes="xy"), ValueError, "unknown axes 'xy'"),
    "axes_number": ("multimodal", dict(axes=2), ValueError, "unknown axes 2"),
    "axes_eeg_hw": ("multimodal", dict(input="eeg", axes="hw"), ValueError, "only 'w'"),
    "axes_eeg_h": ("eegnet", dict(input="eeg", axes="h"), ValueError, "only 'w'"),
    "steps_zero": ("multimodal", dict(steps=0), ValueError, "steps = 0 < 1"),
    "steps_negative": ("multimodal", dict(steps=-2), ValueError, "steps = -2 < 1"),
    "steps_float": ("multimodal", dict(steps=2.5), ValueError, "steps must be an int"),
    "steps_bool": ("eegnet", dict(input="eeg", steps=True), ValueError, "steps must be an int"),
    "sigma_zero": ("multimodal", dict(max_sigma=0.0), ValueError, "max_sigma must be a finite number > 0"),
    "sigma_negative": ("multimodal", dict(max_sigma=-1.0), ValueError, "max_sigma must be a finite number > 0"),
    "sigma_nan": ("multimodal", dict(max_sigma=float("nan")), ValueError, "max_sigma must be a finite number > 0"),
    "sigma_inf": ("deep", dict(input="eeg", max_sigma=float("inf")), ValueError, "max_sigma must be a finite number > 0"),
    "sigma_word": ("multimodal", dict(max_sigma="5"), ValueError, "max_sigma must be a finite number > 0"),
    "grad_step_zero": ("multimodal", dict(grad_step=0), ValueError, "grad_step must be a finite number > 0"),
    "grad_step_negative": ("multimodal", dict(grad_step=-0.01), ValueError, "grad_step must be a finite number > 0"),
    "grad_step_nan": ("eegnet", dict(input="eeg", grad_step=float("nan")), ValueError, "grad_step must be a finite number > 0"),
    "radius_beyond": ("multimodal", dict(max_sigma=5000.0), ValueError, "filter radius 20000"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg_all": ("multimodal", dict(input="eeg", class_idx="all", sqrt=True), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(class_idx=3, return_parts=True, axes="h"), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", class_idx="all", axes="w"), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", class_idx=torch.tensor([5, 0]), max_batch=3), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kind, kw, exc, match = BAD[case]
    eeg, spec = _inputs()
    if kind == "multimodal":
        model = brainxai.build_multimodal(CH, T, C)
    elif kind.startswith("spectrogram"):
        model = brainxai.Spectrogram_Model(33 if kind.endswith("33") else 6, in_channels=C)
        eeg = eeg if kind.endswith("with_eeg") else None
    else:
        model = brainxai.EEGNet(6, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(6, Chans=CH, Samples=T)
        spec = None
    args = dict(steps=5, max_sigma=3.0)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.blur_ig(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * per
        brainxai.blur_ig(model, None, one.expand(128, 1, 1000, 1000), steps=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * n
        brainxai.blur_ig(model, None, one.expand(1 << 16, 1, 2, 2), steps=1 << 15, max_sigma=1.0)
    with pytest.raises(ValueError, match="65535"):                        # B * Kc planes
        brainxai.blur_ig(model, None, one.expand(4096, 1, 2, 2), steps=1, class_idx="all")
    with pytest.raises(ValueError, match="LDS"):                          # both axes: a 4-column strip of 2 x 1200 rows and the taps
        brainxai.blur_ig(model, None, one.expand(1, 1, 1200, 8), steps=2)
    assert reached == []


def test_helpers_refuse_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    x = torch.zeros(2, 3, 8, 8)
    for bad in (5, torch.zeros(3, 8, 8), torch.zeros(0, 1, 2, 2)):
        with pytest.raises(ValueError, match="blur_path: (x must be|empty input)"):
            brainxai.blur_path(bad, steps=2, max_sigma=1.0)
        with pytest.raises(ValueError, match="gaussian_blur: (x must be|empty input)"):
            brainxai.gaussian_blur(bad, 1.0)
    with pytest.raises(ValueError, match="steps = 0 < 1"):
        brainxai.blur_path(x, steps=0, max_sigma=1.0)
    with pytest.raises(ValueError, match="max_sigma must be"):
        brainxai.blur_path(x, steps=2, max_sigma=0)
    with pytest.raises(ValueError, match="grad_step must be"):
        brainxai.blur_path(x, steps=2, max_sigma=1.0, grad_step=0.0)
    with pytest.raises(ValueError, match="unknown axes"):
        brainxai.blur_path(x, steps=2, max_sigma=1.0, axes="t")
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.blur_path(torch.zeros(1, 1, 1, 1).expand(1 << 16, 1, 2, 2), steps=1 << 15, max_sigma=1.0)
    with pytest.raises(ValueError, match="filter radius"):
        brainxai.blur_path(x, steps=2, max_sigma=9000.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.blur_path(x, steps=2, max_sigma=1.0)
    for bad in (-1.0, float("nan"), float("inf"), [1.0, -2.0], torch.tensor([0.5, float("nan")])):
        with pytest.raises(ValueError, match="sigma must be finite and >= 0"):
            brainxai.gaussian_blur(x, bad)
    with pytest.raises(ValueError, match=r"sigma of shape \(3,\)"):
        brainxai.gaussian_blur(x, torch.ones(3))
    with pytest.raises(ValueError, match="sigma must be a number or one per sample"):
        brainxai.gaussian_blur(x, "wide")
    with pytest.raises(ValueError, match="unknown axes"):
        brainxai.gaussian_blur(x, 1.0, axes="both")
    with pytest.raises(ValueError, match="filter radius"):
        brainxai.gaussian_blur(x, 5000.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.gaussian_blur(x, torch.tensor([1.0, 0.0]))
    assert reached == []


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def rows(Bn=3, n=4, Cc=2, Hh=10, Ww=12, axes=0, TW=5, per_sample=0, row0=0, rows=12):
        return lib.bx_blur_rows(None, None, None, None, None, Bn, n, Cc, Hh, Ww, axes, TW, per_sample, row0, rows, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(Cc=0), b"bad shape"), (dict(Hh=0), b"bad shape"), (dict(Ww=0), b"bad shape"),
                     (dict(axes=3), b"unknown axes"), (dict(axes=-1), b"unknown axes"), (dict(TW=4), b"tap width"), (dict(TW=0), b"tap width"),
                     (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"), (dict(row0=10, rows=3), b"rows row0"),
                     (dict(Bn=1 << 16, n=1 << 15), b"32-bit"), (dict(Bn=1 << 11, Hh=1 << 10, Ww=1 << 10, rows=1), b"32-bit"),
                     (dict(Bn=1000, n=1000, Hh=64, Ww=64, Cc=1, rows=1 << 19), b"rows * per"), (dict(), b"null pointer"), (dict(axes=2, row0=11, rows=1), b"null pointer")]:
        rc = rows(**kw)
        assert rc == BX_EINVAL and b"bx_blur_rows" in msg() and word in msg(), (kw, rc, msg())
    assert rows(TW=2 * 16385 + 1) == BX_EUNSUPPORTED and b"radius 16385" in msg()
    assert rows(Cc=65536, Hh=2, Ww=2, rows=1) == BX_EUNSUPPORTED and b"65536 channels" in msg()
    assert rows(Hh=1200, Ww=8, TW=2 * 1300 + 1, rows=1) == BX_EUNSUPPORTED and b"strip" in msg()          # x is NULL: D is absent, one plane
    assert rows(Hh=2100, Ww=8, TW=801, rows=1) == BX_EUNSUPPORTED and b"strip" in msg()
    assert rows(Hh=2, Ww=6000, TW=2 * 6000 + 1, axes=2, rows=1) == BX_EUNSUPPORTED and b"taps on either side" in msg()
    assert rows(Hh=2100, Ww=8, TW=801, axes=1, rows=1) == BX_EINVAL and b"null pointer" in msg()          # one axis needs no strip

    def acc(Bn=3, n=4, per=100, row0=0, rows=12, Kc=6, slot=0):
        return lib.bx_blurig_accumulate(None, None, None, None, Bn, n, per, Kc, slot, row0, rows, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"),
                     (dict(row0=10, rows=3), b"rows row0"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"), (dict(Bn=1 << 11, per=1 << 20, rows=1), b"32-bit"),
                     (dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per"), (dict(Kc=0), b"class slot"), (dict(slot=6), b"class slot"),
                     (dict(slot=-1), b"class slot"), (dict(Bn=1 << 10, per=1 << 18, Kc=32, rows=1), b"B * Kc * per"), (dict(), b"null pointer")]:
        rc = acc(**kw)
        assert rc == BX_EINVAL and b"bx_blurig_accumulate" in msg() and word in msg(), (kw, rc, msg())
    assert acc(Kc=33) == BX_EUNSUPPORTED and b"33 classes" in msg()

    def tot(Rr=4, Ln=100):
        return lib.bx_blurig_sum_rows(None, None, Rr, Ln, None)
    for kw, word in [(dict(Rr=0), b"bad shape"), (dict(Ln=0), b"bad shape"), (dict(Rr=1 << 11, Ln=1 << 20), b"32-bit"), (dict(), b"null pointer")]:
        rc = tot(**kw)
        assert rc == BX_EINVAL and b"bx_blurig_sum_rows" in msg() and word in msg(), (kw, rc, msg())
