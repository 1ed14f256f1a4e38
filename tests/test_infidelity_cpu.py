"""CPU: brainxai.infidelity / sensitivity_max argument checks that run before anything reaches a device, the limits of the
bx_infidelity_* / bx_sensitivity_* entry points, and the restatement of the definitions (tests/infidelity_ref.py) against closed forms
of linear models in fp64, with the statistics of the restatement's uniform draws."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import infidelity_ref as R
from tests import smooth_grad_ref as SG

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


# ---- the restatement against closed forms, in fp64 --------------------------------------------------------------------------------------
def _exact_case(grouped, eeg):
    """(x, sigma, z, Phi, score, shape) with x, sigma and z on grids coarse enough that sigma * z and x - sigma * z are exact in fp32:
    the rows then carry no rounding.  Phi fp32 [B,1,cells] is any attribution; score is the raw output of the linear model whose weights
    are Phi spread over the elements (all the weight of a pixel / time column on its first channel / electrode), sample b's rows
    against sample b's weights: it sees exactly Delta = <Phi, I>."""
    rng = np.random.default_rng(3)
    B, n = 2, 7
    shape = (1, 5, 12) if eeg else (3, 4, 6)
    cells = (shape[2] if eeg else shape[1] * shape[2]) if grouped else int(np.prod(shape))
    x = (np.round(rng.standard_normal((B, *shape)) * 64) / 64).astype(np.float32)
    z32 = (np.round(SG.noise(B, n, cells, 11) * 256) / 256).astype(np.float32)
    sig = np.array([0.5, 0.25], dtype=np.float32)
    Ie = R.noise_per_element(R.perturbation(sig, z32), (B, *shape), grouped, eeg)
    assert np.array_equal(x[:, None].astype(np.float64) - Ie, R.rows(x, sig, z32, grouped, eeg).reshape(B, n, *shape).astype(np.float64)), "rows not exact"
    phi = rng.standard_normal((B, 1, cells)).astype(np.float32)
    we = np.zeros((B, *shape))
    if not grouped:
        we[:] = phi.reshape(B, *shape)
    elif eeg:
        we[:, 0, 0, :] = phi.reshape(B, -1)
    else:
        we[:, 0] = phi.reshape(B, shape[1], shape[2])

    def score(rows):
        r = rows.numpy().reshape(len(rows), -1)
        per_sample = n if len(r) == B * n else 1
        return np.array([[float(np.dot(r[j], we[j // per_sample].ravel()))] for j in range(len(r))])
    return x, sig, z32, phi, score, shape


@pytest.mark.parametrize("grouped,eeg", [(False, False), (True, False), (False, True), (True, True)], ids=["spec elements", "spec pixels", "eeg elements", "eeg columns"])
def test_infidelity_restatement_equals_the_closed_forms_of_a_linear_model(grouped, eeg):
    x, sig, z32, w, score, shape = _exact_case(grouped, eeg)
    B, n = z32.shape[:2]
    d_w, _ = R.dots(R.perturbation(sig, z32), w)
    base = (d_w * d_w).sum(-1) / n                                         # sum d^2 / n  [B,1]
    assert (base > 0).all()
    infid, beta, d, delta = R.infidelity(score, x, sig, z32, w, grouped, eeg)
    assert d.shape == delta.shape == (B, 1, n) and np.array_equal(d, d_w) and (beta == 1).all()
    print(f"Phi = w: infidelity / (sum d^2 / n) = {(infid / base).max():.3e}")
    assert (infid <= 1e-20 * base).all(), "Phi = w must explain a linear score exactly"
    two = (2 * w).astype(np.float32)
    infid2, _, d2, _ = R.infidelity(score, x, sig, z32, two, grouped, eeg)
    assert np.array_equal(d2, 2 * d_w) and np.allclose(infid2, base, rtol=1e-12, atol=0), "Phi = 2w leaves (2d - d)^2 = d^2"
    infid2n, beta2n, _, _ = R.infidelity(score, x, sig, z32, two, grouped, eeg, normalize=True)
    assert np.allclose(beta2n, 0.5, rtol=1e-12, atol=0) and (infid2n <= 1e-20 * base).all(), "normalize finds beta = 1/2"
    infid0, beta0, d0, delta0 = R.infidelity(score, x, sig, z32, np.zeros_like(w), grouped, eeg, normalize=True)
    assert not d0.any() and (beta0 == 0).all() and np.allclose(infid0, (delta0 * delta0).sum(-1) / n, rtol=1e-15, atol=0), "Phi = 0 leaves mean Delta^2, beta = 0"
    assert np.allclose(infid0, base, rtol=1e-10, atol=0)
    # -z everywhere is another valid draw; rows x + I against the dot of +I are not: Delta changes sign and (d + d)^2 = 4 d^2
    flipped, _, _, _ = R.infidelity(score, x, sig, -z32, w, grouped, eeg)
    assert (flipped <= 1e-20 * base).all()
    Ie = R.noise_per_element(R.perturbation(sig, z32), x.shape, grouped, eeg)
    S = score(torch.from_numpy((x[:, None] + Ie).reshape(-1, *shape)).double()).reshape(B, n, 1)
    wrong, _ = R.finish(d_w, R.drops(score(torch.from_numpy(x).double()), S))
    assert np.allclose(wrong, 4 * base, rtol=1e-10, atol=0)


def test_finish_orders_and_edge_cases():
    d = np.array([[[1.0, -2.0, 0.5]], [[0.0, 0.0, 0.0]]])
    delta = np.array([[[0.5, -1.0, 0.25]], [[0.3, -0.1, 0.2]]])
    infid, beta = R.finish(d, delta, normalize=True)
    assert beta[0, 0] == 0.5 and infid[0, 0] == 0.0
    assert beta[1, 0] == 0.0 and np.isclose(infid[1, 0], (0.09 + 0.01 + 0.04) / 3, rtol=1e-15)
    infid, beta = R.finish(d, delta)
    assert (beta == 1).all() and np.isclose(infid[0, 0], (0.25 + 1.0 + 0.0625) / 3, rtol=1e-15)
    assert np.array_equal(R.drops(np.array([[1.0, 2.0]]), np.array([[[0.5, 1.0], [0.25, 3.0]]])), np.array([[[0.5, 0.75], [1.0, -1.0]]]))


def test_rows_restatement():
    x = np.array([[[[1.0, -0.0, 3.5], [2.0, 2.0, 2.0]]]], dtype=np.float32)            # [1,1,2,3]
    z32 = SG.noise(1, 2, 6, 9).astype(np.float32)
    sig = np.array([1.75], dtype=np.float32)
    r = R.rows(x, sig, z32)
    assert r.dtype == np.float32 and r.shape == (2, 1, 2, 3)
    assert np.array_equal(r.reshape(2, 6), (x.reshape(1, 6) - (np.float32(1.75) * z32[0]).astype(np.float32)).astype(np.float32))
    assert np.array_equal(R.rows(x, np.zeros(1, np.float32), z32), np.broadcast_to(x, (2, 1, 2, 3))), "sigma = 0 gives the sample itself"
    nz = (np.float32(1.75) * z32[0, :, :3]).astype(np.float32)              # [n, 3]: one draw per time column / per pixel column
    col = R.rows(x, sig, z32[:, :, :3], grouped=True, eeg=True)            # both electrodes move by the same draw
    assert col.shape == (2, 1, 2, 3)
    assert np.array_equal(col[:, 0, 0], (x[0, 0, 0][None] - nz).astype(np.float32)) and np.array_equal(col[:, 0, 1], (x[0, 0, 1][None] - nz).astype(np.float32))
    pix = R.rows(np.broadcast_to(x, (1, 3, 2, 3)).copy(), sig, z32, grouped=True)          # three equal channels, six pixels
    assert pix.shape == (2, 3, 2, 3) and np.array_equal(pix[:, 0], pix[:, 1]) and np.array_equal(pix[:, 0], r[:, 0])


def test_sensitivity_restatement_equals_the_closed_form_of_a_linear_explanation():
    rng = np.random.default_rng(5)
    B, n, shape = 3, 6, (1, 4, 9)
    A = rng.standard_normal((5, 36))
    x = rng.standard_normal((B, *shape)).astype(np.float32)
    x[2] = 0.0                                                             # Phi(x) = 0: the denominator is 1
    radius = np.array([0.02, 0.5, 0.125], dtype=np.float32)
    u32 = R.uniform(B, n, 36, 8).reshape(B, n, *shape)

    def explain(rows):
        return rows.numpy().reshape(len(rows), 36) @ A.T
    sens, dist, norms = R.sensitivity(explain, x, radius, u32)
    delta = R.uniform_rows(x, radius, u32).astype(np.float64).reshape(B, n, 36) - x.astype(np.float64).reshape(B, 1, 36)   # what the rows really moved by
    want_dist = np.sqrt(((delta @ A.T) ** 2).sum(-1))
    want_norm = np.sqrt(((x.astype(np.float64).reshape(B, 36) @ A.T) ** 2).sum(-1))
    assert norms[2] == 0 and np.allclose(norms, want_norm, rtol=1e-13, atol=0)
    assert np.allclose(dist, want_dist, rtol=1e-9, atol=0)
    want = want_dist.max(1) / np.array([want_norm[0], want_norm[1], 1.0])
    assert np.allclose(sens, want, rtol=1e-9, atol=0) and sens[2] == dist[2].max()
    assert (np.abs(delta) <= radius.astype(np.float64)[:, None, None] * (1 + 2.0 ** -20) + np.abs(x.astype(np.float64).reshape(B, 1, 36)) * 2.0 ** -23).all()


# ---- the uniform draws ------------------------------------------------------------------------------------------------------------------
def test_uniform_draws_statistics_prefix_and_stream():
    B, n, per = 2, 6, 38000
    u = R.uniform(B, n, per, 0)
    assert u.dtype == np.float32 and u.shape == (B, n, per)
    assert (u >= -1).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 23, np.round(u.astype(np.float64) * 2.0 ** 23)), "a draw is a multiple of 2^-23: exact in fp32"
    N = u.size
    u64 = u.astype(np.float64)
    mean, var = float(u64.mean()), float((u64 * u64).mean())
    lag1 = abs(float(np.corrcoef(u64[..., :-1].ravel(), u64[..., 1:].ravel())[0, 1]))
    print(f"uniform draws {B}x{n}x{per}: mean {mean:.5f}, mean square {var:.5f} (1/3), lag-1 correlation {lag1:.2e}")
    assert abs(mean) <= 5 * np.sqrt(1 / 3 / N)
    assert abs(var - 1 / 3) <= 5 * np.sqrt(4 / 45 / N)                      # Var(u^2) = 1/5 - 1/9
    assert lag1 <= 5 / np.sqrt(N)
    assert np.array_equal(R.uniform(B, 3, per, 0), u[:, :3]), "a longer run must extend a shorter one"
    assert np.array_equal(R.uniform(1, n, per, 0), u[:1])
    assert np.array_equal(R.uniform(B, n, 1665, 0), u[:, :, :1665]), "an element's draw does not depend on the row length"
    assert not np.array_equal(R.uniform(B, n, per, 1), u)
    assert not np.array_equal(R.uniform(B, n, per, 0, word3=0), u), "counter word 3 = 1 is a stream apart from the normal draws' words"
    w0 = SG.philox((np.uint64(0), np.uint64(0), np.uint64(0), np.uint64(1)), (0, 0)).reshape(4)
    assert np.array_equal(u[0, 0, :4], (w0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1))


# ---- refusals of the drivers ------------------------------------------------------------------------------------------------------------
B, C, H, W, CH, T, K = 2, 4, 16, 24, 19, 2000, 6


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


def _model(kind):
    if kind == "multimodal":
        return brainxai.build_multimodal(CH, T, C)
    if kind.startswith("spectrogram"):
        return brainxai.Spectrogram_Model(33 if kind.endswith("33") else K, in_channels=C)
    return brainxai.EEGNet(K, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(K, Chans=CH, Samples=T)


SPEC_MAP, EEG_MAP = (B, H, W), (B, CH, T)
# name -> (model kind, attribution shape (None: not a tensor), keyword overrides, exception, message)
BAD = {
    "input_unknown": ("multimodal", SPEC_MAP, dict(input="both"), ValueError, "infidelity: unknown input"),
    "input_none_eeg": ("spectrogram", EEG_MAP, dict(input="eeg"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", EEG_MAP, dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "score_unknown": ("multimodal", SPEC_MAP, dict(score="logit"), ValueError, "unknown score 'logit'"),
    "score_none": ("eegnet", EEG_MAP, dict(input="eeg", score=None), ValueError, "unknown score None"),
    "attribution_list": ("multimodal", None, dict(), ValueError, "attribution must be a tensor"),
    "map_spec_transposed": ("multimodal", (B, W, H), dict(), ValueError, r"wrong map shape \(2, 24, 16\) for input='spec'.*\[B,C,H,W\] = \(2, 4, 16, 24\) or \[B,H,W\] = \(2, 16, 24\)"),
    "map_spec_channels": ("multimodal", (B, 3, H, W), dict(), ValueError, "wrong map shape"),
    "map_spec_batch": ("spectrogram", (B + 1, H, W), dict(), ValueError, "wrong map shape"),
    "map_spec_is_eeg": ("multimodal", EEG_MAP, dict(), ValueError, "wrong map shape"),
    "map_eeg_is_spec": ("multimodal", SPEC_MAP, dict(input="eeg"), ValueError, r"wrong map shape .* for input='eeg'.*\[B,1,Chans,T\].*\[B,Chans,T\].*\[B,1,T\] = \(2, 1, 2000\)"),
    "map_eeg_electrodes": ("eegnet", (B, CH), dict(input="eeg"), ValueError, "wrong map shape"),
    "map_eeg_columns_wide": ("deep", (B, 2, T), dict(input="eeg"), ValueError, "wrong map shape"),
    "all_without_class_axis_spec": ("multimodal", SPEC_MAP, dict(class_idx="all"), ValueError, "class_idx='all' needs an attribution with a class axis"),
    "all_without_class_axis_elements": ("multimodal", (B, C, H, W), dict(class_idx="all"), ValueError, "class axis after B"),
    "all_without_class_axis_eeg": ("eegnet", (B, 1, T), dict(input="eeg", class_idx="all"), ValueError, "class axis after B"),
    "all_wrong_class_count": ("multimodal", (B, K + 1, H, W), dict(class_idx="all"), ValueError, r"wrong map shape.*\[B,K,H,W\] = \(2, 6, 16, 24\)"),
    "class_axis_without_all": ("multimodal", (B, K, H, W), dict(class_idx=1), ValueError, "wrong map shape"),
    "both_scales": ("multimodal", SPEC_MAP, dict(noise_level=0.1, stdev=0.2), ValueError, "noise_level or stdev, not both"),
    "both_scales_tensor": ("eegnet", EEG_MAP, dict(input="eeg", noise_level=0.1, stdev=torch.ones(B)), ValueError, "noise_level or stdev, not both"),
    "level_negative": ("multimodal", SPEC_MAP, dict(noise_level=-0.1), ValueError, "noise_level must be a finite number >= 0"),
    "stdev_negative": ("multimodal", SPEC_MAP, dict(stdev=-1.0), ValueError, "stdev must be finite and >= 0"),
    "stdev_tensor_shape": ("multimodal", SPEC_MAP, dict(stdev=torch.ones(3)), ValueError, r"stdev of shape \(3,\)"),
    "max_batch": ("multimodal", SPEC_MAP, dict(max_batch=0), ValueError, "max_batch = 0"),
    "nsamples_zero": ("multimodal", SPEC_MAP, dict(nsamples=0), ValueError, "nsamples = 0 < 1"),
    "nsamples_float": ("eegnet", EEG_MAP, dict(input="eeg", nsamples=2.5), ValueError, "nsamples must be an int"),
    "nsamples_bool": ("deep", (B, 1, T), dict(input="eeg", nsamples=True), ValueError, "nsamples must be an int"),
    "seed_negative": ("multimodal", SPEC_MAP, dict(seed=-1), ValueError, "seed must be an int in"),
    "seed_wide": ("multimodal", SPEC_MAP, dict(seed=1 << 64), ValueError, "seed must be an int in"),
    "seed_float": ("multimodal", SPEC_MAP, dict(seed=1.0), ValueError, "seed must be an int in"),
    "class_high": ("multimodal", SPEC_MAP, dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", SPEC_MAP, dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", SPEC_MAP, dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", SPEC_MAP, dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", SPEC_MAP, dict(), ValueError, "33 classes"),
    "cpu_multimodal_pixels": ("multimodal", SPEC_MAP, dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_elements_all": ("multimodal", (B, K, C, H, W), dict(class_idx="all", normalize=True), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", EEG_MAP, dict(input="eeg", class_idx=[1, 2], score="logprob", stdev=torch.tensor([0.1, 0.0])), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", (B, C, H, W), dict(class_idx=3, return_parts=True, seed=(1 << 64) - 1), RuntimeError, "no CPU path"),
    "cpu_eegnet_columns": ("eegnet", (B, 1, T), dict(input="eeg", seed=7, noise_level=0), RuntimeError, "no CPU path"),
    "cpu_eegnet_all_columns": ("eegnet", (B, K, 1, T), dict(input="eeg", class_idx="all"), RuntimeError, "no CPU path"),
    "cpu_deep_elements": ("deep", (B, 1, CH, T), dict(input="eeg", class_idx=torch.tensor([5, 0]), max_batch=3, stdev=0.5), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_infidelity_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kind, shape, kw, exc, match = BAD[case]
    eeg, spec = _inputs()
    model = _model(kind)
    if kind.startswith("spectrogram"):
        eeg = eeg if kind.endswith("with_eeg") else None
    elif kind != "multimodal":
        spec = None
    attribution = [[0.0]] if shape is None else torch.zeros(shape)
    args = dict(nsamples=5)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.infidelity(model, eeg, spec, attribution, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_infidelity_offset_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * cells: 128 * 32 * 10^6 values (views)
        brainxai.infidelity(model, None, one.expand(128, 1, 1000, 1000), torch.zeros(1).expand(128, 32, 1000, 1000), nsamples=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * n * K
        brainxai.infidelity(model, None, one.expand(1 << 12, 1, 2, 2), torch.zeros(1).expand(1 << 12, 2, 2), nsamples=1 << 15)
    assert reached == []


SENS_BAD = {
    "explain_none": (dict(explain=None), ValueError, "explain must be a callable"),
    "explain_tensor": (dict(explain=torch.zeros(2)), ValueError, "explain must be a callable"),
    "input_unknown": (dict(input="both"), ValueError, "sensitivity_max: unknown input"),
    "input_none": (dict(input="eeg", eeg=None), ValueError, "tensor is None"),
    "radius_negative": (dict(radius=-0.1), ValueError, "radius must be finite and >= 0"),
    "radius_tensor_negative": (dict(radius=torch.tensor([0.1, -0.1])), ValueError, "radius must be finite and >= 0"),
    "radius_nan": (dict(radius=float("nan")), ValueError, "radius must be finite and >= 0"),
    "radius_shape": (dict(radius=torch.ones(3)), ValueError, r"radius of shape \(3,\)"),
    "radius_list": (dict(radius=[0.1, 0.2]), ValueError, "radius must be a number or a tensor"),
    "radius_level_negative": (dict(radius_level=-0.02), ValueError, "radius_level must be a finite number >= 0"),
    "radius_level_inf": (dict(radius_level=float("inf")), ValueError, "radius_level must be a finite number >= 0"),
    "both_radii": (dict(radius=0.1, radius_level=0.02), ValueError, "radius or radius_level, not both"),
    "nsamples_zero": (dict(nsamples=0), ValueError, "nsamples = 0 < 1"),
    "nsamples_float": (dict(nsamples=1.5), ValueError, "nsamples must be an int"),
    "seed_negative": (dict(seed=-1), ValueError, "seed must be an int in"),
    "max_batch": (dict(max_batch=0), ValueError, "max_batch = 0"),
    "other_batch": (dict(eeg=torch.zeros(3, 1, CH, T)), ValueError, "same batch size"),
    "cpu_spec": (dict(), RuntimeError, "no CPU path"),
    "cpu_eeg": (dict(input="eeg", radius=torch.tensor([0.1, 0.0]), return_parts=True), RuntimeError, "no CPU path"),
    "cpu_stand_alone": (dict(eeg=None, radius_level=0.0, seed=(1 << 64) - 1), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(SENS_BAD))
def test_sensitivity_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kw, exc, match = SENS_BAD[case]
    eeg, spec = _inputs()
    called = []

    def explain(e, s, sample):
        called.append(sample)
        return s
    args = dict(explain=explain, eeg=eeg, spec=spec, nsamples=4)
    args.update(kw)
    fn = args.pop("explain")
    e, s = args.pop("eeg"), args.pop("spec")
    with pytest.raises(exc, match=match):
        brainxai.sensitivity_max(fn, e, s, **args)
    assert reached == [] and called == [], f"library entry points reached: {reached}; explain called {len(called)} times"


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def check(name, fn, cases):
        for kw, word, *code in cases:
            rc = fn(**kw)
            assert rc == (code[0] if code else BX_EINVAL) and name.encode() in msg() and word in msg(), (name, kw, rc, msg())
    chunk = [(dict(Bn=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(b0=-1), b"samples b0"), (dict(nb=0), b"samples b0"), (dict(b0=2, nb=2), b"samples b0"),
             (dict(n0=-1), b"draws n0"), (dict(n=0), b"draws n0"), (dict(n0=3, n=3), b"draws n0"), (dict(), b"null pointer"), (dict(b0=2, nb=1, n0=4, n=1), b"null pointer")]

    def spec(Bn=3, Cc=4, Hh=16, Ww=24, Cp=8, pix=1, N=5, b0=0, nb=3, n0=0, n=5, dtype=0):
        return lib.bx_infidelity_rows_spec(None, None, None, Bn, Cc, Hh, Ww, Cp, pix, N, b0, nb, n0, n, 7, dtype, None)
    check("bx_infidelity_rows_spec", spec, chunk + [
        (dict(Cc=0), b"0 channels", BX_EUNSUPPORTED), (dict(Cc=5), b"5 channels", BX_EUNSUPPORTED), (dict(Cp=4), b"Cp = 4"), (dict(Hh=0), b"bad shape"),
        (dict(Bn=1 << 10, Hh=1 << 10, Ww=1 << 10, nb=1), b"32-bit offsets"), (dict(Bn=1 << 16, N=1 << 15, nb=1, n=1), b"32-bit offsets"),
        (dict(Hh=1 << 10, Ww=1 << 10, N=64, n=64), b"32-bit byte offsets"), (dict(Bn=70000, nb=70000, Hh=1, Ww=1, n=1), b"32-bit byte offsets")])
    assert spec(dtype=9) < 0

    def eeg(Bn=3, Ch=19, Tt=2000, col=0, N=5, b0=0, nb=3, n0=0, n=5):
        return lib.bx_infidelity_rows_eeg(None, None, None, Bn, Ch, Tt, col, N, b0, nb, n0, n, 7, None)
    check("bx_infidelity_rows_eeg", eeg, chunk + [
        (dict(Ch=0), b"bad shape"), (dict(Tt=0), b"bad shape"), (dict(Bn=1 << 12, Ch=1 << 10, Tt=1 << 10, nb=1), b"32-bit offsets"),
        (dict(Ch=1 << 10, Tt=1 << 10, N=1 << 10, n=1 << 10, nb=1), b"32-bit byte offsets"), (dict(col=1), b"null pointer")])

    rows = [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"),
            (dict(row0=10, rows=3), b"rows row0"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"), (dict(Bn=1 << 11, per=1 << 20, rows=1), b"32-bit"),
            (dict(), b"null pointer"), (dict(row0=11, rows=1), b"null pointer")]

    def dot(Bn=3, n=4, per=100, Kc=6, row0=0, rows=12):
        return lib.bx_infidelity_dot(None, None, None, Bn, n, per, Kc, (1 << 64) - 1, row0, rows, None)
    check("bx_infidelity_dot", dot, rows + [(dict(Kc=0), b"bad class count"), (dict(Kc=33), b"33 classes", BX_EUNSUPPORTED),
                                            (dict(Bn=1 << 10, per=1 << 18, Kc=32, rows=1), b"B * Kc * cells")])

    def fin(Bn=3, n=5, Kk=6, norm=0):
        return lib.bx_infidelity_finish(None, None, None, None, None, None, None, Bn, n, Kk, norm, None)
    check("bx_infidelity_finish", fin, [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(Kk=0), b"bad shape"), (dict(Kk=33), b"33 classes", BX_EUNSUPPORTED),
                                        (dict(Bn=1 << 16, n=1 << 12, Kk=32), b"32-bit"), (dict(), b"null pointer"), (dict(norm=1), b"null pointer")])

    def srows(Bn=3, n=4, per=100, row0=0, rows=12):
        return lib.bx_sensitivity_rows(None, None, None, Bn, n, per, 5, row0, rows, None)
    check("bx_sensitivity_rows", srows, rows + [(dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per")])

    def sdist(Bn=3, n=4, per=100, row0=0, rows=12):
        return lib.bx_sensitivity_dist(None, None, None, Bn, n, per, row0, rows, None)
    check("bx_sensitivity_dist", sdist, rows + [(dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per")])

    def sfin(Bn=3, n=4):
        return lib.bx_sensitivity_finish(None, None, None, Bn, n, None)
    check("bx_sensitivity_finish", sfin, [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"), (dict(), b"null pointer")])
