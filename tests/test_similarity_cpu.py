"""CPU: the restatement of brainxai.map_similarity (tests/similarity_ref.py) against scipy and a brute-force SSIM, the argument checks of
map_similarity / agreement_matrix / randomization_test that run before anything reaches a device, randomization_layers, the
re-initialisation bounds against torch's, and the limits of the bx_rank_average / bx_map_corr / bx_topk_overlap / bx_row_minmax /
bx_ssim_rows / bx_param_uniform entry points."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.stats
import torch

import brainxai
from brainxai import _lib
from brainxai import explain as X
from tests import similarity_ref as R

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


# ---- the restatement against scipy --------------------------------------------------------------------------------------------------------
def _tied(R_=4, N=300, seed=2):
    rng = np.random.default_rng(seed)
    a = (np.round(rng.standard_normal((R_, N)) * 4) / 4).astype(np.float32)          # values rounded to 1/4: heavy ties
    b = (np.round((0.6 * a + 0.8 * rng.standard_normal((R_, N))) * 4) / 4).astype(np.float32)
    return a, b


def test_restatement_agrees_with_scipy_on_heavy_ties():
    a, b = _tied()
    assert all(len(np.unique(row)) < 40 for row in a)
    ranks = R.average_ranks(a)
    for r in range(len(a)):
        assert np.array_equal(ranks[r], scipy.stats.rankdata(-a[r].astype(np.float64), method="average") - 1)
        assert np.isclose(R.spearman(a, b)[r], scipy.stats.spearmanr(a[r], b[r]).statistic, rtol=0, atol=1e-13)
        assert np.isclose(R.corr(a, b)[r], scipy.stats.pearsonr(a[r].astype(np.float64), b[r].astype(np.float64)).statistic, rtol=0, atol=1e-13)
    assert np.allclose(R.pearson(a, b), R.corr(a, b), rtol=0, atol=1e-13)
    assert np.allclose(R.spearman(a, b, abs=True), [scipy.stats.spearmanr(np.abs(p), np.abs(q)).statistic for p, q in zip(a, b)], rtol=0, atol=1e-13)
    # the definition: #{key > key_i} + (#{key = key_i} - 1) / 2, half-integers that fp32 holds exactly
    k = a[0].astype(np.float64)
    want = np.array([(k > v).sum() + ((k == v).sum() - 1) / 2 for v in k])
    assert np.array_equal(ranks[0], want) and np.array_equal(ranks.astype(np.float32).astype(np.float64), ranks)
    assert np.isnan(R.corr(np.ones((1, 5), np.float32), a[:1, :5])[0])


def test_rank_keys_follow_bx_rank_desc():
    x = np.array([[np.nan, -0.0, 0.0, 1.0, -np.inf, 1.0]], dtype=np.float32)
    assert np.array_equal(R.average_ranks(x)[0], [4.5, 2.5, 2.5, 0.5, 4.5, 0.5])
    assert np.array_equal(R.stable_ranks(x)[0], [4, 2, 3, 0, 5, 1])
    assert np.array_equal(R.average_ranks(-x, abs=True)[0], R.average_ranks(np.abs(x))[0])
    assert R.topk_overlap(x, x, 2)[0] == 1.0 and R.topk_overlap(x, -x, 2)[0] == 0.0
    assert [R.topk_count(t, 384) for t in (0.1, 1.0, 1e-9, 5, 384)] == [39, 384, 1, 5, 384]


def _ssim_brute(a, b, window, win, data_range):
    """Window by window: the moments of every full window from its cells, nothing filtered."""
    X_, Y_, Rg = R.ssim_cells(a, b, data_range, False)
    taps = R.gaussian_taps() if window == "gaussian" else np.full(win, 1.0 / win)
    H, W = X_.shape[1:]
    wy = taps if H > 1 else np.ones(1)
    wx = taps if W > 1 else np.ones(1)
    w2 = np.outer(wy, wx)
    NP = w2.size
    cov = 1.0 if window == "gaussian" else NP / (NP - 1.0)
    C1, C2 = (0.01 * Rg) ** 2, (0.03 * Rg) ** 2
    out = []
    for x, y in zip(X_, Y_):
        S = []
        for i in range(H - len(wy) + 1):
            for j in range(W - len(wx) + 1):
                p, q = x[i:i + len(wy), j:j + len(wx)], y[i:i + len(wy), j:j + len(wx)]
                ux, uy = (w2 * p).sum(), (w2 * q).sum()
                vx, vy, vxy = cov * ((w2 * p * p).sum() - ux * ux), cov * ((w2 * q * q).sum() - uy * uy), cov * ((w2 * p * q).sum() - ux * uy)
                S.append((2 * ux * uy + C1) * (2 * vxy + C2) / ((ux * ux + uy * uy + C1) * (vx + vy + C2)))
        out.append(np.mean(S))
    return np.array(out)


@pytest.mark.parametrize("shape,window,win,data_range", [((7, 8), "uniform", 7, None), ((11, 13), "uniform", 7, None), ((11, 13), "gaussian", None, None),
                                                         ((7, 8), "uniform", 3, 2.0), ((1, 20), "uniform", 7, None), ((15, 1), "gaussian", None, 1.5)])
def test_ssim_restatement_equals_brute_force(shape, window, win, data_range):
    rng = np.random.default_rng(7)
    a = rng.standard_normal((3, *shape)).astype(np.float32)
    b = (0.5 * a + rng.standard_normal((3, *shape))).astype(np.float32)
    got = R.ssim(a, b, window, win, data_range)
    want = _ssim_brute(a, b, window, 11 if window == "gaussian" else win, data_range)
    assert np.allclose(got, want, rtol=0, atol=1e-12), (got, want)
    assert (np.abs(got) < 0.999).all()
    same = R.ssim(a, a, window, win, data_range)
    assert (same == 1.0).all(), "identical maps give exactly 1"


def test_gaussian_taps_are_scipys():
    want = R.gaussian_taps()
    assert len(want) == 11 and int(3.5 * 1.5 + 0.5) == 5
    assert np.array_equal(X._sim_taps("gaussian", 11), want)
    assert np.array_equal(X._sim_taps("uniform", 7), np.full(7, 1 / 7))


# ---- refusals of the drivers ------------------------------------------------------------------------------------------------------------
A = torch.zeros(2, 16, 24)
SIM_BAD = {
    "unequal_shapes": ((A, torch.zeros(2, 24, 16)), dict(), ValueError, "equal shapes"),
    "one_axis": ((torch.zeros(5), torch.zeros(5)), dict(), ValueError, "at least two axes"),
    "not_a_tensor": ((A, [[0.0]]), dict(), ValueError, "must be tensors"),
    "too_many_cells": ((torch.zeros(1).expand(1, 1024, 1024), torch.zeros(1).expand(1, 1024, 1024)), dict(), ValueError, r"1048576 cells per map.*1\.\.1048575"),
    "win_even": ((A, A), dict(win_size=4), ValueError, "odd int"),
    "win_float": ((A, A), dict(win_size=7.0), ValueError, "odd int"),
    "win_with_gaussian": ((A, A), dict(window="gaussian", win_size=11), ValueError, "win_size is fixed by window='gaussian'"),
    "win_larger_than_axis": ((A, A), dict(win_size=17), ValueError, "exceeds a filtered axis"),
    "gaussian_larger_than_axis": ((torch.zeros(2, 10, 24), torch.zeros(2, 10, 24)), dict(window="gaussian"), ValueError, "exceeds a filtered axis"),
    "line_shorter_than_win": ((torch.zeros(2, 1, 6), torch.zeros(2, 1, 6)), dict(), ValueError, "exceeds a filtered axis"),
    "window_unknown": ((A, A), dict(window="hann"), ValueError, "unknown window"),
    "data_range_zero": ((A, A), dict(data_range=0.0), ValueError, "data_range"),
    "rows_above_strip": ((torch.zeros(1, 407, 8), torch.zeros(1, 407, 8)), dict(), ValueError, "at most 406 rows"),
    "topk_zero": ((A, A), dict(topk=0.0), ValueError, r"outside \(0, 1\]"),
    "topk_above_one": ((A, A), dict(topk=1.5), ValueError, r"outside \(0, 1\]"),
    "topk_int_above_n": ((A, A), dict(topk=385), ValueError, "outside 1..N = 384"),
    "topk_int_zero": ((A, A), dict(topk=0), ValueError, "outside 1..N"),
    "metric_unknown": ((A, A), dict(metrics=("spearman", "kendall")), ValueError, "unknown metric 'kendall'"),
    "metrics_empty": ((A, A), dict(metrics=()), ValueError, "unknown metric"),
    "cpu": ((A, A), dict(), RuntimeError, "no CPU path"),
    "cpu_line_abs": ((torch.zeros(3, 1, 64), torch.zeros(3, 1, 64)), dict(abs=True, metrics="ssim", data_range=2.0), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(SIM_BAD))
def test_map_similarity_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    (a, b), kw, exc, match = SIM_BAD[case]
    with pytest.raises(exc, match=match):
        brainxai.map_similarity(a, b, **kw)
    assert reached == [], f"library entry points reached: {reached}"


def test_agreement_matrix_bad_arguments_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    for maps, kw, exc, match in [({}, dict(), ValueError, "non-empty dict"), ({"a": A, "b": torch.zeros(2, 16, 25)}, dict(), ValueError, "equal shapes"),
                                 ({"a": A, "b": A}, dict(metric="kendall"), ValueError, "unknown metric"), ({"a": A}, dict(metric=("ssim", "topk")), ValueError, "one name"),
                                 ({"a": A, "b": A}, dict(metric="ssim", win_size=2), ValueError, "odd int"), ({"a": A, "b": A}, dict(), RuntimeError, "no CPU path")]:
        with pytest.raises(exc, match=match):
            brainxai.agreement_matrix(maps, **kw)
    assert reached == []


def _models():
    return {"multimodal": brainxai.build_multimodal(19, 2000, 4), "spectrogram": brainxai.Spectrogram_Model(6, in_channels=4),
            "eegnet": brainxai.EEGNet(6, Chans=19, Samples=2000), "deep": brainxai.EEGNetAttentionDeep(6, Chans=19, Samples=2000)}


def test_randomization_test_bad_arguments_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    called = []

    def explain(m, e, s):
        called.append(1)
        return torch.zeros(2, 16, 24)
    nets = _models()
    half = brainxai.Spectrogram_Model(6, in_channels=4)
    half.block5.conv2.half()
    for model, kw, exc, match in [
            (nets["multimodal"], dict(layers=["fc2", "spectrogram_model.block6"]), ValueError, "unknown layer 'spectrogram_model.block6'"),
            (nets["multimodal"], dict(layers=[("fc2", "fc3")]), ValueError, "unknown layer 'fc3'"),
            (nets["multimodal"], dict(layers=["fc2", ("fc1", "fc2")]), ValueError, "repeats a tensor"),
            (nets["multimodal"], dict(layers=["log_softmax"]), ValueError, "no parameters to re-initialise"),
            (nets["multimodal"], dict(layers=[]), ValueError, "layers is empty"),
            (half, dict(), ValueError, "float16 parameter; parameters must be float32"),
            (nets["multimodal"], dict(order="random"), ValueError, "unknown order 'random'"),
            (nets["multimodal"], dict(input="both"), ValueError, "unknown input"),
            (nets["eegnet"], dict(input="spec"), ValueError, "does not fit a stand-alone EEGNet"),
            (nets["multimodal"], dict(metrics=("spearman", "hog")), ValueError, "unknown metric 'hog'"),
            (nets["multimodal"], dict(seed=-1), ValueError, "seed must be an int in"),
            (nets["multimodal"], dict(explain=None), ValueError, "explain must be a callable"),
            (nets["multimodal"], dict(), RuntimeError, "no CPU path"),
            (nets["deep"], dict(input="eeg", order="independent", layers=["dense2", ("conv2", "batchnorm4")]), RuntimeError, "no CPU path")]:
        kw = dict(kw)
        fn = kw.pop("explain", explain)
        with pytest.raises(exc, match=match):
            brainxai.randomization_test(model, fn, None, None, **kw)
    assert reached == [] and called == [], f"library entry points reached: {reached}; explain called {len(called)} times"


# ---- randomization_layers -----------------------------------------------------------------------------------------------------------------
def _flat(layers):
    return [n for layer in layers for n in ((layer,) if isinstance(layer, str) else layer)]


@pytest.mark.parametrize("kind,input,path,first,last", [
    ("multimodal", "spec", ("fc1", "fc2", "spectrogram_model"), ["fc2", "fc1", "spectrogram_model.fc", "spectrogram_model.block5"], "spectrogram_model.block1"),
    ("multimodal", "eeg", ("fc1", "fc2", "eeg_model"), ["fc2", "fc1", "eeg_model.dense", ("eeg_model.separableConv", "eeg_model.batchnorm3")], ("eeg_model.conv1", "eeg_model.batchnorm1")),
    ("spectrogram", "spec", ("",), ["fc", "block5", "block4"], "block1"),
    ("eegnet", "eeg", ("",), ["dense", ("separableConv", "batchnorm3"), ("depthwiseConv", "batchnorm2")], ("conv1", "batchnorm1")),
    ("deep", "eeg", ("",), ["dense2", "dense1", "attention_layer", ("conv2", "batchnorm4"), ("separableConv", "batchnorm3")], ("conv1", "batchnorm1"))])
def test_randomization_layers_cover_the_explained_path_once(kind, input, path, first, last):
    model = _models()[kind]
    layers = brainxai.randomization_layers(model, input)
    assert layers[:len(first)] == first and layers[-1] == last, layers
    covered = []
    for n in _flat(layers):
        covered += [id(q) for q in X._resolve(model, n).parameters()]
    assert len(covered) == len(set(covered)), "a parameter appears twice"
    want = {id(q) for name, q in model.named_parameters() if any(name.startswith(p) for p in path)}
    assert set(covered) == want, "the parametrised modules of the explained path and nothing else"
    if kind == "multimodal":
        other = "eeg_model" if input == "spec" else "spectrogram_model"
        assert not any(n.startswith(other) for n in _flat(layers))
    plans = X._rand_plan("t", model, layers)                                # every tensor of the path is written or reset, buffers included
    owned = {id(t) for _, o in plans for t in o}
    bufs = {id(t) for name, t in model.named_buffers() if any(name.startswith(p) for p in path)}
    assert want | bufs == owned
    written = {id(a[1]) for acts, _ in plans for a in acts}
    assert written == owned


def test_randomization_layers_refusals():
    with pytest.raises(ValueError, match="unknown input"):
        brainxai.randomization_layers(_models()["multimodal"], "both")
    with pytest.raises(ValueError, match="does not fit"):
        brainxai.randomization_layers(_models()["spectrogram"], "eeg")
    with pytest.raises(ValueError, match="no default layer list"):
        brainxai.randomization_layers(torch.nn.Linear(3, 2), "eeg")


# ---- re-initialisation bounds ---------------------------------------------------------------------------------------------------------------
def test_reinitialisation_bounds_are_torchs():
    """torch's reset_parameters: kaiming_uniform_(a=sqrt(5)) has gain sqrt(2 / 6) and bound gain sqrt(3 / fan_in) = 1 / sqrt(fan_in); the
    bias is drawn from the same bound."""
    nets = _models()
    seen = set()
    for kind, input in (("multimodal", "spec"), ("multimodal", "eeg"), ("deep", "eeg")):
        model = nets[kind]
        for acts, _ in X._rand_plan("t", model, brainxai.randomization_layers(model, input)):
            for a in acts:
                if a[0] != "uniform":
                    continue
                q, bound = a[1], a[2]
                owner = next(m for m in model.modules() if any(p is q for p in m.parameters(recurse=False)))
                fi, _ = torch.nn.init._calculate_fan_in_and_fan_out(owner.weight)
                assert X._rand_fan_in(owner.weight) == fi == R.fan_in(owner.weight)
                gain = torch.nn.init.calculate_gain("leaky_relu", math.sqrt(5))
                assert math.isclose(bound, gain * math.sqrt(3.0 / fi), rel_tol=1e-15) and math.isclose(bound, 1 / math.sqrt(fi), rel_tol=1e-15)
                seen.add((type(owner).__name__, tuple(owner.weight.shape[1:])))
    assert {k for k, _ in seen} == {"Conv2d", "Linear"} and len(seen) >= 10          # 3x3, 1x1, (1,64), (Chans,1) grouped, (1,16) and the heads
    # the host restatement draws inside the bound and keeps positions apart
    w = R.param_uniform(1027, 0.125, 5, 0, 0)
    assert w.dtype == np.float32 and (np.abs(w) <= 0.125).all() and np.abs(w).max() > 0.12
    assert not np.array_equal(w, R.param_uniform(1027, 0.125, 5, 1, 0)) and not np.array_equal(w, R.param_uniform(1027, 0.125, 5, 0, 1))
    assert np.array_equal(w[:5], R.param_uniform(5, 0.125, 5, 0, 0))


def test_reinit_state_dict_orders():
    model = brainxai.Spectrogram_Model(6, in_channels=4)
    layers = brainxai.randomization_layers(model, "spec")
    with torch.no_grad():
        for m in model.modules():                                           # a trained BatchNorm: nothing sits at its reset value
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.fill_(2.0), m.bias.fill_(0.5), m.running_mean.fill_(-1.0), m.running_var.fill_(3.0), m.num_batches_tracked.fill_(9)
    sd0 ={k: v.clone() for k, v in model.state_dict().items()}
    casc, ind = R.reinit_state_dict(model, layers, 3, "cascade", 2), R.reinit_state_dict(model, layers, 3, "independent", 2)
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items()), "the model itself is not touched"
    for k in sd0:
        stage = 0 if k.startswith("fc") else 1 if k.startswith("block5") else 2 if k.startswith("block4") else None
        if stage is None:
            assert torch.equal(casc[k], sd0[k]) and torch.equal(ind[k], sd0[k]), k
        else:
            assert not torch.equal(casc[k], sd0[k]), k
            if stage == 2:
                assert torch.equal(casc[k], ind[k]), "a layer's draws do not depend on the order"
            else:
                assert torch.equal(ind[k], sd0[k]), k
    assert float(casc["block4.bn.weight"].min()) == 1.0 and float(casc["block4.bn.running_var"].max()) == 1.0 and int(casc["block4.bn.num_batches_tracked"]) == 0


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    big = 1 << 20

    def check(name, fn, cases):
        for kw, word, *code in cases:
            rc = fn(**kw)
            assert rc == (code[0] if code else BX_EINVAL) and name.encode() in msg() and word in msg(), (name, kw, rc, msg())
    rows = [(dict(Rn=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(N=big), b"supported 1..1048575", BX_EUNSUPPORTED), (dict(Rn=1 << 12, N=big - 1), b"32-bit offsets"),
            (dict(), b"null pointer")]

    def ravg(Rn=3, N=100, ws=1 << 30):
        return lib.bx_rank_average(None, None, None, Rn, N, 0, None, ws, None)
    check("bx_rank_average", ravg, rows + [(dict(Rn=65536, N=4), b"65536 rows", BX_EUNSUPPORTED)])
    assert lib.bx_rank_average_workspace(3, 100) == 1200 and lib.bx_rank_average_workspace(3, big) == 0 and lib.bx_rank_average_workspace(0, 5) == 0

    def corr(Rn=3, N=100):
        return lib.bx_map_corr(None, None, None, Rn, N, 1, None)
    check("bx_map_corr", corr, rows)

    def topk(Rn=3, N=100, k=10):
        return lib.bx_topk_overlap(None, None, None, Rn, N, k, None)
    check("bx_topk_overlap", topk, rows + [(dict(k=0), b"k = 0 outside"), (dict(k=101), b"k = 101 outside")])

    def mm(Rn=3, N=100):
        return lib.bx_row_minmax(None, None, None, Rn, N, 0, None)
    check("bx_row_minmax", mm, [(dict(Rn=0), b"bad shape"), (dict(N=0), b"bad shape"), (dict(Rn=1 << 16, N=1 << 15), b"32-bit offsets"), (dict(), b"null pointer")])

    def ssim(Rn=3, H=16, W=24, win=7, dr=1.0, cov=49 / 48, ws=1 << 30):
        return lib.bx_ssim_rows(None, None, None, None, None, None, None, dr, cov, None, Rn, H, W, win, 0, None, ws, None)
    check("bx_ssim_rows", ssim, [
        (dict(Rn=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(H=1024, W=1024), b"cells per map", BX_EUNSUPPORTED), (dict(win=4), b"not an odd number"),
        (dict(win=0), b"not an odd number"), (dict(win=65, H=100, W=100), b"window 65", BX_EUNSUPPORTED), (dict(win=17), b"exceeds a filtered axis"),
        (dict(H=1, W=6), b"exceeds a filtered axis"), (dict(H=407, W=8), b"H = 407 rows", BX_EUNSUPPORTED), (dict(Rn=65536), b"65536 rows", BX_EUNSUPPORTED),
        (dict(dr=0.0), b"data_range"), (dict(cov=float("inf")), b"data_range and cov_norm"), (dict(), b"null pointer"), (dict(H=406, W=7), b"null pointer"),
        (dict(H=1, W=1000), b"null pointer"), (dict(H=1000, W=1), b"null pointer")])
    # the strip: the widest of 64 .. 4 with H * SW <= 1624, halved while half of it covers every column of positions
    assert [lib.bx_ssim_strip(*s) for s in ((19, 2000, 7), (19, 70, 7), (19, 38, 7), (19, 10, 7), (128, 256, 7), (64, 128, 11), (406, 7, 7), (407, 7, 7), (1, 64, 7),
                                            (3000, 1, 11), (25, 500, 7), (26, 500, 7), (7, 7, 7), (16, 24, 17))] == [64, 64, 32, 4, 8, 16, 4, 0, 64, 64, 64, 32, 4, 0]
    assert lib.bx_ssim_rows_workspace(3, 19, 71, 7) == 3 * 2 * 8 and lib.bx_ssim_rows_workspace(3, 407, 8, 7) == 0 and lib.bx_ssim_rows_workspace(0, 16, 24, 7) == 0

    def pu(n=10, bound=0.5):
        return lib.bx_param_uniform(None, n, bound, 7, 0, 0, None)
    check("bx_param_uniform", pu, [(dict(n=0), b"n = 0 outside"), (dict(n=1 << 31), b"outside"), (dict(bound=-1.0), b"bound must be finite"),
                                   (dict(bound=float("inf")), b"bound must be finite"), (dict(), b"null pointer")])
