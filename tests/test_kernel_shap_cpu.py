"""CPU: the restatement of Kernel SHAP (tests/kernel_shap_ref.py) against brute-force Shapley values, brainxai.kernel_shap's argument
checks that run before anything reaches a device, and the limits of the bx_shap_* entry points.

Bound of the reference checks: (M + N) 2^-52 kappa(Xt' W Xt) max|phi| -- the textbook bound of a Cholesky solve with the length of the
Gram sums added (the bound tests/test_gpu_kernel_shap.py applies to bx_shap_fit)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import kernel_shap_ref as R

BX_EINVAL, BX_EUNSUPPORTED = -1, -6
EPS = 2.0 ** -52


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


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 5, 8])
def test_exact_set_reproduces_brute_force_shapley_values(M):
    g = np.random.default_rng(M)
    v = g.standard_normal(2 ** M)
    Z, w, exact = R.coalition_set(M, 2 ** M - 2)
    assert exact and Z.shape == (2 ** M - 2, M) and np.array_equal(R.coalition_index(Z), np.arange(1, 2 ** M - 1))
    assert abs(sum(w[Z.sum(1) == s].sum() for s in range(1, M)) - sum((M - 1) / (s * (M - s)) for s in range(1, M))) < 1e-12
    assert not R.coalition_set(M, 2 ** M - 3)[2] or M == 2           # one short of the exact budget: sampled (M = 2 has no smaller even set)
    Y = v[R.coalition_index(Z)][:, None]
    want = R.brute_force(M, v)
    bound = (M + Z.shape[0]) * EPS * R.gram_cond(Z, w) * np.abs(want).max()
    for how in ("normal", "lstsq"):
        got = R.fit(Z, w, Y, v[:1], v[-1:], how)[0]
        err = np.abs(got - want).max()
        print(f"M = {M} {how}: |fit - brute force| {err:.1e} (bound {bound:.1e})")
        assert err <= bound
        assert abs(got.sum() - (v[-1] - v[0])) <= 4 * EPS * np.abs(got).sum()


@pytest.mark.parametrize("M,N", [(19, 64), (37, 96), (256, 1024)])
def test_sampled_set_reproduces_a_linear_game(M, N):
    Z, w, exact = R.coalition_set(M, N, seed=0)
    assert not exact and Z.shape == (N, M) and (w == 1).all()
    assert np.array_equal(Z[0::2] + Z[1::2], np.ones((N // 2, M), dtype=np.uint8)), "rows 2j and 2j+1 are complements"
    size = Z.sum(1)
    assert size.min() >= 1 and size.max() <= M - 1
    a = np.random.default_rng(1).standard_normal((M, 3))
    got = R.fit(Z, w, Z @ a + 0.25, np.full(3, 0.25), a.sum(0) + 0.25)
    kappa = R.gram_cond(Z, w)
    bound = (M + N) * EPS * kappa * np.abs(a).max()
    print(f"M = {M} N = {N}: kappa {kappa:.3g} |fit - linear game| {np.abs(got - a.T).max():.1e} (bound {bound:.1e})")
    assert np.abs(got - a.T).max() <= bound
    both = R.fit(Z, w, Z @ a + 0.25, np.full(3, 0.25), a.sum(0) + 0.25, "lstsq")
    assert np.abs(got - both).max() <= bound
    assert R.coalition_set(M, N + 1, seed=0)[0].shape == (N, M), "an odd budget is rounded down to even"
    assert not np.array_equal(R.coalition_set(M, N, seed=1)[0], Z)


def test_values_add_up_and_the_operator_is_the_fit():
    M, N = 19, 64
    Z, w, _ = R.coalition_set(M, N)
    g = np.random.default_rng(5)
    S, clean, empty = g.random((2, N, 3)), g.random((2, 3)), g.random((2, 3))
    phi = R.values(Z, w, S, clean, empty)
    assert phi.shape == (2, 3, M)
    assert np.abs(phi.sum(2) - (clean - empty)).max() <= 4 * EPS * np.abs(phi).sum(2).max()
    op = R.solution_operator(Z, w)
    assert op.shape == (M, N + 2)
    again = np.einsum("mn,bnk->bkm", op, np.concatenate([S, clean[:, None], empty[:, None]], axis=1))
    amp = R.amplification(Z, w)
    assert np.abs(again - phi).max() <= (M + N) * EPS * R.gram_cond(Z, w) * amp
    assert np.abs(op[:, :N].sum(1) + op[:, N] + op[:, N + 1]).max() <= 1e-12, "a constant added to every score moves no value"


def test_masks_and_rows_of_the_restatement():
    seg = R.grid_segments(4, 6, 2, 3)
    assert np.array_equal(seg, np.array([[0, 0, 1, 1, 2, 2]] * 2 + [[3, 3, 4, 4, 5, 5]] * 2))
    Z = np.array([[1, 0, 0, 0, 0, 1], [0, 1, 1, 1, 1, 0]], dtype=np.uint8)
    m = R.masks(seg, Z)
    assert m.shape == (2, 4, 6) and m[0, 0, 0] and m[0, 3, 5] and m[0].sum() == 8 and np.array_equal(m[1], ~m[0])
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6) + 1
    x[0, 1, 0, 0] = -0.0
    got = R.perturbed(x, m[0], [7.0, 8.0, 9.0])
    assert torch.equal(got[:, :, :2, :2], x[:, :, :2, :2]) and bool((got[:, 1, :2, 2:] == 8.0).all()) and torch.signbit(got[0, 1, 0, 0])
    e = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(2, 1, 5, 6)
    cols = R.perturbed(e, R.masks(R.grid_segments(1, 6, 1, 3), np.array([[0, 1, 0]], dtype=np.uint8))[0], torch.arange(5.0) * 100)
    assert torch.equal(cols[:, :, :, 2:4], e[:, :, :, 2:4]) and bool((cols[:, 0, 3, :2] == 300.0).all()) and bool((cols[:, 0, 3, 4:] == 300.0).all())


def test_coalition_builder_equals_the_reference():
    from brainxai import explain as X
    for M, n, seed in [(2, 2050, 0), (6, 62, 0), (6, 61, 3), (11, 2070, 0), (19, 64, 0), (37, 97, 0), (256, 1024, 0), (19, 2086, 7)]:
        Z, w, exact = X._shap_coalitions("kernel_shap", M, n, seed, None)
        Zr, wr, er = R.coalition_set(M, n, seed)
        assert exact == er and Z.dtype == np.uint8 and w.dtype == np.float64 and np.array_equal(Z, Zr) and np.array_equal(w, wr), (M, n, seed)
    seg, M = X._shap_segments("kernel_shap", (2, 3), "spec", 16, 24)
    assert M == 6 and np.array_equal(seg, R.grid_segments(16, 24, 2, 3)) and np.array_equal(seg, brainxai.grid_segments(16, 24, 2, 3))
    seg, M = X._shap_segments("kernel_shap", "electrodes", "eeg", 19, 50)
    assert M == 19 and seg.shape == (19, 50) and np.array_equal(seg, np.arange(19)[:, None].repeat(50, 1))
    seg, M = X._shap_segments("kernel_shap", ("time", 8), "eeg", 37, 3000)
    assert M == 8 and seg.shape == (1, 3000) and np.array_equal(seg, R.grid_segments(1, 3000, 1, 8))


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------------
B, C, H, W, CH, T = 2, 4, 16, 24, 19, 2000


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


def _gap():
    seg = brainxai.grid_segments(H, W, 2, 3).copy()
    seg[seg == 4] = 6
    return seg


Z6 = np.array([[1, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 1, 1]], dtype=np.uint8)

# name -> (model kind, keyword overrides, exception, message); the spectrogram is 16 x 24, the EEG input 19 x 2000
BAD = {
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "unknown input"),
    "score_unknown": ("multimodal", dict(score="logit"), ValueError, "unknown score"),
    "input_none": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "labels_with_a_gap": ("multimodal", dict(segments=_gap()), ValueError, "every label present"),
    "labels_negative": ("multimodal", dict(segments=brainxai.grid_segments(H, W, 2, 3) - 1), ValueError, "every label present"),
    "labels_float": ("multimodal", dict(segments=np.zeros((H, W), dtype=np.float32)), ValueError, "must hold integers"),
    "labels_shape": ("multimodal", dict(segments=np.zeros((H, W + 1), dtype=np.int32)), ValueError, "label map of shape"),
    "labels_time_row_for_spec": ("spectrogram", dict(segments=brainxai.grid_segments(1, W, 1, 3)), ValueError, "label map of shape"),
    "one_player": ("multimodal", dict(segments=(1, 1)), ValueError, "1 players"),
    "one_player_map": ("spectrogram", dict(segments=np.zeros((H, W), dtype=np.int64)), ValueError, "1 players"),
    "players_257": ("eegnet", dict(input="eeg", segments=("time", 257)), ValueError, "257 players"),
    "players_257_map": ("multimodal", dict(segments=(np.arange(H * W) % 257).reshape(H, W)), ValueError, "257 players"),
    "grid_outside": ("multimodal", dict(segments=(17, 2)), ValueError, "outside 1..16 x 1..24"),
    "electrodes_for_spec": ("multimodal", dict(segments="electrodes"), ValueError, "segments 'electrodes'"),
    "time_for_spec": ("spectrogram", dict(segments=("time", 4)), ValueError, r"\('time', n\)"),
    "segments_word": ("eegnet", dict(input="eeg", segments="channels"), ValueError, "segments 'channels'"),
    "too_few_samples": ("eegnet", dict(input="eeg", segments="electrodes", num_samples=17), ValueError, "N = 16 coalitions"),
    "too_few_samples_grid": ("multimodal", dict(segments=(4, 6), num_samples=22), ValueError, "N = 22 coalitions"),
    "too_few_given": ("multimodal", dict(coalitions=(Z6[:4], None)), ValueError, "N = 4 coalitions"),
    "num_samples_float": ("multimodal", dict(num_samples=64.0), ValueError, "num_samples must be"),
    "given_all_zero_row": ("multimodal", dict(coalitions=(np.vstack([Z6, np.zeros((1, 6), dtype=np.uint8)]), None)), ValueError, "all-zero or all-one"),
    "given_all_one_row": ("multimodal", dict(coalitions=(np.vstack([np.ones((1, 6), dtype=np.uint8), Z6]), None)), ValueError, "all-zero or all-one"),
    "given_width": ("multimodal", dict(coalitions=(Z6[:, :5], None)), ValueError, r"shape \[N, M = 6\]"),
    "given_not_binary": ("multimodal", dict(coalitions=(Z6 * 2, None)), ValueError, "0 / 1"),
    "weights_length": ("multimodal", dict(coalitions=(Z6, np.ones(4))), ValueError, "4 weights for 5 coalitions"),
    "weights_negative": ("multimodal", dict(coalitions=(Z6, -np.ones(5))), ValueError, "positive and finite"),
    "coalitions_not_a_pair": ("multimodal", dict(coalitions=Z6), ValueError, "must be a pair"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=[0, 1, 2]), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(B, C, H, W - 1)), ValueError, "kernel_shap: baseline of shape"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_all": ("multimodal", dict(class_idx="all", score="logprob", num_samples=24, segments=(4, 6)), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", dict(input="eeg", segments="electrodes", num_samples=64, baseline=torch.zeros(CH)), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(baseline=torch.zeros(B, C, H, W), class_idx=[1, 2], coalitions=(Z6, np.arange(1.0, 6.0))), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", segments=("time", 8)), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", segments=(19, 4), class_idx=torch.tensor([5, 0])), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kind, kw, exc, match = BAD[case]
    eeg, spec = _inputs()
    if kind == "multimodal":
        model = brainxai.build_multimodal(CH, T, C)
    elif kind.startswith("spectrogram"):
        model, eeg = brainxai.Spectrogram_Model(33 if kind.endswith("33") else 6, in_channels=C), None
    else:
        model = brainxai.EEGNet(6, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(6, Chans=CH, Samples=T)
        spec = None
    args = dict(segments=(2, 3))
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.kernel_shap(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_offset_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    big = torch.zeros(1, 1, 1, 1).expand(128, 1, 1000, 1000)             # a view: 32 * 128 * 10^6 map values is past 2^31
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.kernel_shap(model, None, big, segments=(2, 2), class_idx="all")
    with pytest.raises(ValueError, match="cells per sample"):
        brainxai.kernel_shap(model, None, torch.zeros(1, 1, 1, 1).expand(1, 1, 1024, 1024), segments=(2, 2))
    assert reached == []


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    dom_cases = [(dict(Hm=0), BX_EINVAL, b"bad shape"), (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per map"), (dict(M=1), BX_EUNSUPPORTED, b"1 players"),
                 (dict(M=257), BX_EUNSUPPORTED, b"257 players"), (dict(M=0), BX_EUNSUPPORTED, b"players")]
    row_cases = [(dict(n0=-1), BX_EINVAL, b"coalitions n0"), (dict(n=0), BX_EINVAL, b"coalitions n0"), (dict(n0=90, n=7), BX_EINVAL, b"coalitions n0"),
                 (dict(N=0), BX_EINVAL, b"N = 0"), (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(kind=3), BX_EINVAL, b"baseline_kind"), (dict(kind=-1), BX_EINVAL, b"baseline_kind")]

    def spec(Bn=1, Cc=3, Hm=64, Wm=128, Cp=8, M=37, N=96, n0=0, n=96, dt=_lib.BX_F32, kind=0):
        return lib.bx_shap_perturb_spec(None, None, kind, None, Bn, Cc, Hm, Wm, Cp, None, None, M, N, n0, n, dt, None)
    for kw, code, word in dom_cases + row_cases + [(dict(Cc=5), BX_EUNSUPPORTED, b"channels"), (dict(Cc=0), BX_EUNSUPPORTED, b"channels"), (dict(Cp=16), BX_EINVAL, b"Cp"),
                                                   (dict(Hm=512, Wm=512, N=600, n=600), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                                                   (dict(M=2, N=2, n=1, n0=1), BX_EINVAL, b"null pointer"), (dict(M=256), BX_EINVAL, b"null pointer")]:
        rc = spec(**kw)
        assert rc == code and b"bx_shap_perturb_spec" in msg() and word in msg(), (kw, rc, msg())
    assert spec(dt=7) < 0 and b"dtype" in msg()

    def eeg(Bn=1, Hm=19, Wm=2000, rows=19, M=19, N=64, n0=0, n=64, kind=0):
        return lib.bx_shap_perturb_eeg(None, None, kind, None, Bn, Hm, Wm, rows, None, None, M, N, n0, n, None)
    for kw, code, word in row_cases[:3] + row_cases[4:] + [(dict(rows=2), BX_EINVAL, b"map_rows = 2"), (dict(rows=0), BX_EINVAL, b"map_rows = 0"), (dict(Hm=0, rows=0), BX_EINVAL, b"map_rows"),
                                                          (dict(M=1), BX_EUNSUPPORTED, b"1 players"), (dict(M=257), BX_EUNSUPPORTED, b"257 players"),
                                                          (dict(Hm=1024, Wm=1024, rows=1), BX_EUNSUPPORTED, b"values per sample"), (dict(Wm=0), BX_EINVAL, b"bad shape"),
                                                          (dict(Bn=64, Hm=64, Wm=15000, rows=1, N=64), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                                                          (dict(rows=1), BX_EINVAL, b"null pointer")]:
        rc = eeg(**kw)
        assert rc == code and b"bx_shap_perturb_eeg" in msg() and word in msg(), (kw, rc, msg())

    def fit(Bn=2, N=64, K=6, M=19, ws=1 << 20):
        return lib.bx_shap_fit(None, None, None, None, None, None, Bn, N, K, M, None, ws, None, None, None)
    fit_cases = [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(K=0), BX_EINVAL, b"bad shape"), (dict(K=33), BX_EUNSUPPORTED, b"33 classes"), (dict(M=1), BX_EUNSUPPORTED, b"1 players"),
                 (dict(M=257, N=300), BX_EUNSUPPORTED, b"257 players"), (dict(N=17), BX_EINVAL, b"N = 17 coalitions"), (dict(Bn=1 << 16, N=2048, K=32), BX_EINVAL, b"32-bit")]
    for kw, code, word in fit_cases + [(dict(), BX_EINVAL, b"null pointer"), (dict(N=18, K=32), BX_EINVAL, b"null pointer"), (dict(M=2, N=1), BX_EINVAL, b"null pointer")]:
        rc = fit(**kw)
        assert rc == code and b"bx_shap_fit" in msg() and word in msg(), (kw, rc, msg())
    for kw, _, _ in fit_cases:
        a = dict(Bn=2, N=64, K=6, M=19)
        a.update(kw)
        assert lib.bx_shap_fit_workspace(a["Bn"], a["N"], a["K"], a["M"], 1) == 0
    assert lib.bx_shap_fit_workspace(2, 64, 6, 19, 1) == (18 * 18 + 12 * 18) * 8 and lib.bx_shap_fit_workspace(2, 64, 6, 19, 0) == (18 * 18 + 2 * 18) * 8

    def vmap(Bn=2, Rr=6, Hm=64, Wm=128, M=37):
        return lib.bx_shap_value_map(None, None, None, Bn, Rr, Hm, Wm, M, None)
    for kw, code, word in dom_cases + [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(Rr=0), BX_EINVAL, b"bad shape"), (dict(Rr=33), BX_EUNSUPPORTED, b"33 classes"),
                                       (dict(Bn=4096, Rr=32, Hm=512, Wm=512), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = vmap(**kw)
        assert rc == code and b"bx_shap_value_map" in msg() and word in msg(), (kw, rc, msg())
