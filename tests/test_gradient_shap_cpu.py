"""CPU: brainxai.gradient_shap / channel_importance argument checks that run before anything reaches a device, the limits of the
bx_expgrad_* / bx_mean_abs_rows entry points, the draws against the oracle's, and the restatement of the definition
(tests/gradient_shap_ref.py) against the closed form of a linear model."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from brainxai import explain as X
from oracle import ref_torch as O
from tests import gradient_shap_ref as R

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


B, C, H, W, CH, T, NB, N = 2, 4, 16, 24, 19, 2000, 3, 5


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


def _bg(input):
    return torch.zeros(NB, 1, CH, T) if input == "eeg" else torch.zeros(NB, C, H, W)


_IDX, _ALPHA = np.zeros((B, N), dtype=np.int64), np.full((B, N), 0.5, dtype=np.float32)

# name -> (model kind, keyword overrides, exception, message); the spectrogram is 4 x 16 x 24, the EEG input 19 x 2000, Nb = 3, n = 5
BAD = {
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "gradient_shap: unknown input"),
    "input_none_eeg": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "input_none_spec": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "nsamples_zero": ("multimodal", dict(nsamples=0), ValueError, "nsamples = 0 < 1"),
    "nsamples_negative": ("eegnet", dict(nsamples=-3), ValueError, "nsamples = -3 < 1"),
    "nsamples_float": ("eegnet", dict(nsamples=2.5), ValueError, "nsamples must be an int"),
    "nsamples_bool": ("eegnet", dict(nsamples=True), ValueError, "nsamples must be an int"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", dict(input="spec", class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("deep", dict(class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", dict(input="spec"), ValueError, "33 classes"),
    "background_none": ("multimodal", dict(background=None), ValueError, "gradient_shap: background of shape"),
    "background_shape": ("multimodal", dict(background=torch.zeros(NB, 1, CH, T - 1)), ValueError, "gradient_shap: background of shape"),
    "background_other_input": ("multimodal", dict(input="spec", background=torch.zeros(NB, 1, CH, T)), ValueError, "gradient_shap: background of shape"),
    "background_three_axes": ("eegnet", dict(background=torch.zeros(NB, CH, T)), ValueError, "gradient_shap: background of shape"),
    "background_empty": ("eegnet", dict(background=torch.zeros(0, 1, CH, T)), ValueError, "empty background"),
    "draws_not_pair": ("multimodal", dict(draws=_IDX), ValueError, "draws must be"),
    "draws_idx_float": ("multimodal", dict(draws=(_IDX.astype(np.float32), _ALPHA)), ValueError, "draws must be"),
    "draws_alpha_int": ("multimodal", dict(draws=(_IDX, _IDX)), ValueError, "draws must be"),
    "draws_shape": ("multimodal", dict(draws=(_IDX[:, :4], _ALPHA[:, :4])), ValueError, "draws of shapes"),
    "draws_shape_alpha": ("eegnet", dict(draws=(_IDX, _ALPHA.T)), ValueError, "draws of shapes"),
    "draws_index_high": ("multimodal", dict(draws=(_IDX + NB, _ALPHA)), ValueError, r"index outside \[0, Nb = 3\)"),
    "draws_index_negative": ("deep", dict(draws=(torch.from_numpy(_IDX) - 1, torch.from_numpy(_ALPHA))), ValueError, r"index outside \[0, Nb = 3\)"),
    "draws_alpha_nan": ("multimodal", dict(draws=(_IDX, _ALPHA * np.nan)), ValueError, "alpha is not finite"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_spec_all": ("multimodal", dict(input="spec", class_idx="all"), RuntimeError, "no CPU path"),
    "cpu_multimodal_draws": ("multimodal", dict(draws=(_IDX, _ALPHA), class_idx=[1, 2]), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(input="spec", class_idx=3, return_parts=True), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(class_idx="all", seed=7), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(class_idx=torch.tensor([5, 0]), max_batch=3), RuntimeError, "no CPU path"),
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
    args = dict(input="eeg", nsamples=N)
    args.update(kw)
    background = args.pop("background") if "background" in args else _bg(args["input"] if args["input"] in ("eeg", "spec") else "eeg")
    with pytest.raises(exc, match=match):
        brainxai.gradient_shap(model, eeg, spec, background, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_offset_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    big = one.expand(128, 1, 1000, 1000)                                # a view: 32 * 128 * 10^6 values is past 2^31
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.gradient_shap(model, None, big, one.expand(2, 1, 1000, 1000), input="spec", nsamples=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # Nb * per
        brainxai.gradient_shap(model, None, one.expand(1, 1, 1000, 1000), one.expand(4096, 1, 1000, 1000), input="spec", nsamples=1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * n
        brainxai.gradient_shap(model, None, one.expand(1 << 16, 1, 2, 2), one.expand(2, 1, 2, 2), input="spec", nsamples=1 << 15)
    assert reached == []


@pytest.mark.parametrize("top", [0, -1, 20, True, 2.5, "3"])
def test_channel_importance_refuses_bad_top(monkeypatch, top):
    reached = _recorder(monkeypatch)
    with pytest.raises(ValueError, match="channel_importance: top"):
        brainxai.channel_importance(torch.zeros(2, 6, 1, CH, 50), top=top)
    assert reached == []


def test_channel_importance_refuses_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    with pytest.raises(ValueError, match="top needs values with at least two axes"):
        brainxai.channel_importance(torch.zeros(50), top=1)
    for bad in (None, np.zeros((3, 4), dtype=np.float32), torch.zeros(3, 0), torch.zeros(())):
        with pytest.raises(ValueError, match="non-empty tensor"):
            brainxai.channel_importance(bad)
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.channel_importance(torch.zeros(1, 1).expand(1 << 16, 1 << 15))
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.channel_importance(torch.zeros(2, CH, 50), top=CH)
    with pytest.raises(ValueError, match="unknown input"):
        brainxai.GradientExplainer(None, None, input="both")
    assert reached == []


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    row_cases = [(dict(Bn=0), b"bad shape"), (dict(Nb=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(row0=-1), b"rows row0"),
                 (dict(rows=0), b"rows row0"), (dict(row0=10, rows=3), b"rows row0"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"),
                 (dict(Bn=1 << 11, per=1 << 20, rows=1), b"32-bit"), (dict(Nb=1 << 11, per=1 << 20, rows=1), b"32-bit"),
                 (dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per"), (dict(), b"null pointer"), (dict(row0=11, rows=1), b"null pointer")]

    def rows(Bn=3, Nb=4, n=4, per=100, row0=0, rows=12):
        return lib.bx_expgrad_rows(None, None, None, None, None, Bn, Nb, n, per, row0, rows, None)
    for kw, word in row_cases:
        rc = rows(**kw)
        assert rc == BX_EINVAL and b"bx_expgrad_rows" in msg() and word in msg(), (kw, rc, msg())

    def acc(Bn=3, Nb=4, n=4, per=100, row0=0, rows=12, Kc=6, slot=0):
        return lib.bx_expgrad_accumulate(None, None, None, None, None, Bn, Nb, n, per, Kc, slot, row0, rows, None)
    for kw, word in row_cases + [(dict(Kc=0), b"class slot"), (dict(slot=6), b"class slot"), (dict(slot=-1), b"class slot"),
                                 (dict(Bn=1 << 10, per=1 << 18, Kc=32, rows=1), b"B * Kc * per")]:
        rc = acc(**kw)
        assert rc == BX_EINVAL and b"bx_expgrad_accumulate" in msg() and word in msg(), (kw, rc, msg())
    assert acc(Kc=33) == BX_EUNSUPPORTED and b"33 classes" in msg()

    def fin(BK=12, Cc=4, HW=100, n=5):
        return lib.bx_expgrad_finish(None, None, None, BK, Cc, HW, n, None)
    for kw, word in [(dict(BK=0), b"bad shape"), (dict(Cc=0), b"bad shape"), (dict(HW=0), b"bad shape"), (dict(n=0), b"bad shape"),
                     (dict(BK=1 << 12, HW=1 << 18), b"32-bit"), (dict(BK=65536, Cc=1, HW=1), b"planes"), (dict(), b"null pointer")]:
        rc = fin(**kw)
        assert rc == BX_EINVAL and b"bx_expgrad_finish" in msg() and word in msg(), (kw, rc, msg())

    def seed(cls_all=0, Bn=3, n=4, K=6, row0=0, rows=12):
        return lib.bx_expgrad_seed(None, cls_all, None, Bn, n, K, row0, rows, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(K=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(row0=12, rows=1), b"rows row0"),
                     (dict(rows=0), b"rows row0"), (dict(cls_all=6), b"outside [0, 6)"), (dict(cls_all=-1), b"outside [0, 6)"), (dict(), b"null pointer")]:
        rc = seed(**kw)
        assert rc == BX_EINVAL and b"bx_expgrad_seed" in msg() and word in msg(), (kw, rc, msg())

    for (Rn, Ln), word in [((0, 5), b"bad shape"), ((5, 0), b"bad shape"), ((1 << 16, 1 << 15), b"32-bit"), ((19, 2000), b"null pointer")]:
        rc = lib.bx_mean_abs_rows(None, None, Rn, Ln, None)
        assert rc == BX_EINVAL and b"bx_mean_abs_rows" in msg() and word in msg(), (Rn, Ln, rc, msg())


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def _linear(D, K, seed, logsoftmax=True):
    torch.manual_seed(seed)
    layers = [torch.nn.Flatten(), torch.nn.Linear(D, K)] + ([torch.nn.LogSoftmax(dim=1)] if logsoftmax else [])
    return torch.nn.Sequential(*layers)


@pytest.mark.parametrize("seed,Bn,Nb,n", [(0, 1, 1, 1), (3, 2, 5, 12), (7, 4, 100, 200)])
def test_draws_helper_equals_the_restatement(seed, Bn, Nb, n):
    idx, alpha = X._gradshap_draws("gradient_shap", Bn, Nb, n, seed, None)
    want_idx, want_alpha = R.draws(seed, Bn, Nb, n)
    assert idx.dtype == np.int32 and alpha.dtype == np.float32 and idx.shape == alpha.shape == (Bn, n)
    assert np.array_equal(idx, want_idx) and np.array_equal(alpha, want_alpha)
    assert idx.min() >= 0 and idx.max() < Nb and alpha.min() >= 0 and alpha.max() < 1
    again = X._gradshap_draws("gradient_shap", Bn, Nb, n, seed, (torch.from_numpy(idx).long(), alpha.astype(np.float64)))
    assert again[0].dtype == np.int32 and again[1].dtype == np.float32 and np.array_equal(again[0], idx) and np.array_equal(again[1], alpha)


def test_draws_are_the_oracles():
    """The oracle makes its draws inside: the restatement on the helper's draws reproduces the oracle's result for the same seed to
    fp32 rounding (the oracle runs in fp32 here), and another seed's draws do not."""
    Bn, Nb, n, shape = 3, 4, 6, (1, 3, 7)
    model = _linear(21, 5, 1)
    x, bg = O.seeded((Bn, *shape), 5, "randn"), O.seeded((Nb, *shape), 6, "randn")
    want = O.expected_gradients(model, x, bg, nsamples=n, seed=11).double()
    idx, alpha = X._gradshap_draws("gradient_shap", Bn, Nb, n, 11, None)
    m64 = _linear(21, 5, 1).double()
    got = R.values(m64, x, bg, idx, alpha)
    scale = float(want.abs().max())
    assert got.shape == want.shape == (Bn, 5, *shape)
    assert float((got - want).abs().max()) <= 1e-5 * scale
    other = R.values(m64, x, bg, *X._gradshap_draws("gradient_shap", Bn, Nb, n, 12, None))
    assert float((other - want).abs().max()) >= 1e-2 * scale


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_closed_form_of_a_linear_model():
    """F_c(x) = w_c . x + b_c has the gradient w_c everywhere: phi[b,c] = (x[b] - mean of the drawn backgrounds) * w_c.  With inputs on
    a dyadic grid every difference and every mean is exact."""
    Bn, Nb, n, shape, K = 2, 4, 8, (3, 4, 5), 3
    g = np.random.default_rng(0)
    x = (g.integers(-64, 64, (Bn, *shape)) / 8).astype(np.float32)
    bg = (g.integers(-64, 64, (Nb, *shape)) / 8).astype(np.float32)
    idx, alpha = R.draws(4, Bn, Nb, n)
    model = _linear(60, K, 2, logsoftmax=False).double()
    w = model[1].weight.detach().numpy().reshape(K, *shape)
    got = R.values(model, torch.from_numpy(x), torch.from_numpy(bg), idx, alpha).numpy()
    want = (x.astype(np.float64)[:, None] - bg.astype(np.float64)[idx].mean(1)[:, None]) * w[None]
    assert np.abs(got - want).max() <= 64 * 2.0 ** -52 * np.abs(want).max()
    # the accumulate / finish restatement on those gradients gives the same values, and the map is their channel sum
    acc = None
    for c in range(K):
        grads = np.broadcast_to(w[c].astype(np.float32), (Bn * n, *shape))
        acc, _ = R.accumulate(x, bg, idx, grads[:9], acc, slot=c, Kc=K)
        acc, _ = R.accumulate(x, bg, idx, grads[9:], acc, slot=c, Kc=K, row0=9)          # split inside sample 1
    vals, amap = R.finish(acc, n, shape, channels=shape[0])
    want32 = (x.astype(np.float64)[:, None] - bg.astype(np.float64)[idx].mean(1)[:, None]) * w.astype(np.float32).astype(np.float64)[None]
    assert np.abs(vals - want32).max() <= 2.0 ** -23 * np.abs(want32).max()
    assert np.abs(amap - want32.sum(2)).max() <= 2.0 ** -22 * np.abs(want32).sum(2).max()


def test_rows_restatement():
    Bn, Nb, n = 2, 3, 4
    x, bg = O.seeded((Bn, 1, 3, 5), 1, "randn"), O.seeded((Nb, 1, 3, 5), 2, "randn")
    x[0, 0, 1, 2] = -0.0
    bg[1] = x[1]                                                         # a background equal to the sample: d = 0, the row is the sample itself
    idx = np.array([[0, 1, 2, 0], [1, 1, 0, 2]], dtype=np.int32)
    alpha = np.array([[0.0, 0.25, float(np.nextafter(np.float32(1), np.float32(0))), 0.5], [0.3, 0.0, 1.0, 0.7]], dtype=np.float32)
    r = R.rows(x, bg, idx, alpha).reshape(Bn, n, 1, 3, 5)
    assert r.dtype == np.float32
    assert np.array_equal(r[0, 0], bg[0].numpy()) and np.array_equal(r[1, 1], bg[1].numpy()), "alpha = 0 gives the background bit for bit"
    assert np.array_equal(r[1, 0], x[1].numpy())
    exact = bg.double().numpy()[idx] + alpha.astype(np.float64)[:, :, None, None, None] * (x.double().numpy()[:, None] - bg.double().numpy()[idx])
    assert np.abs(r - exact).max() <= 3 * 2.0 ** -24 * max(np.abs(x.numpy()).max(), np.abs(bg.numpy()).max()) * 2
    d = R.diffs(x, bg, idx).reshape(Bn, n, 1, 3, 5)
    assert np.array_equal(d[1, 0], np.zeros((1, 3, 5), dtype=np.float32))


def test_channel_importance_restatement():
    v = np.array([[[1.0, -3.0], [2.0, 2.0], [-2.0, -2.0], [0.0, 0.5]]])
    imp, order = R.channel_importance(v, top=3)
    assert np.array_equal(imp, [[2.0, 2.0, 2.0, 0.25]]) and np.array_equal(order, [[0, 1, 2]])
    assert np.array_equal(R.channel_importance(v[:, ::-1], top=4)[1], [[1, 2, 3, 0]])
