"""CPU: the two restatements of Guided Integrated Gradients (tests/guided_ig_ref.py) against each other and against what the algorithm
must give, and the argument checks of brainxai.guided_ig that run before anything reaches a device.

(b) against (a).  (a) is the algorithm in fp64; (b) stores x, g and every X(alpha) in fp32 and adds in the device's order.  The path is
made of decisions -- which cells the clamp moves, which cells are selected, whether they go all the way, whether another pass follows --
and a rounding can flip one, after which the two walk different paths and no bound relates them.  So the cases here are chosen (by
their seeds, on this side, once) such that the two take the same decisions at every pass, which the test asserts before anything else;
given that, the distance between the two is bounded cell by cell by rules that follow from the operations (u = 2^-24; both form
X(alpha) in the same fp64 operations and (b) rounds it to fp32 once):
    a cell sent to X_min or X_max      |x_b - x_a| <= u |X|: x agrees within the fp32 rounding of X(alpha), whatever it was before
    a cell moved by gamma <= 1          x' = x + gamma (X_max - x) carries the cell's own error, gamma's share of X_max's rounding, the
                                        error of gamma = (L_cur - L_target) / L_S times the distance moved, and one more rounding;
                                        the error of gamma follows from those of the sums, each at most the sum of its cells' errors
    the gradient                        |g_b - g_a| <= Lip(|x_b - x_a|) + u |g|, Lip the function's own bound (|A| e for the quadratic form)
    the attribution                     every pass adds (x - x_old) g: (e + e_old) |g| + |x - x_old| dg + (e + e_old) dg;  fl32 adds u |attr|
guided_ig_ref.Bound carries them along (a)'s run; the test asserts |x_b - x_a| <= e and |values_b - attr_a| <= the bound, cell by cell,
and prints the worst ratio and the size of the bound against the attribution (it stays below 1e-2 of the largest value in every case:
the bound is not vacuous)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import guided_ig_ref as R


# ---- functions with analytic gradients --------------------------------------------------------------------------------------------------
def _quadratic(P, seed):
    """F = x'Ax / 2 + c'x, A symmetric: grad = A x + c; |grad(x + d) - grad(x)| <= |A| |d|"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((P, P))
    A = (A + A.T) / (2 * math.sqrt(P))
    c = rng.standard_normal(P)
    return (lambda x: A @ x + c), (lambda e: np.abs(A) @ e), (lambda x: 0.5 * x @ A @ x + c @ x)


def _steep(P, seed):
    """F = sum w_e x_e^2 / 2 + c'x with a few very steep coordinates (w = 1e3 on every ninth cell): grad = w x + c"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, P)
    w[::9] = 1e3
    c = rng.standard_normal(P)
    return (lambda x: w * x + c), (lambda e: w * e), (lambda x: 0.5 * (w * x * x).sum() + c @ x)


FUNCS = {"quadratic": _quadratic, "steep": _steep}
# (function, P, fraction, max_dist, steps, seed): seeds at which (a) and (b) take the same decisions throughout (at the last step the
# cells left are all selected and gamma is 1 up to rounding, so rounding decides it and not every seed keeps the two together)
SEEDS = {("steep", 250, 0.25, 1.0): 2}
CASES = [(f, P, fr, md, n, SEEDS.get((f, P, fr, md), 1)) for f in sorted(FUNCS) for P in (1, 7, 250) for fr, md, n in
         ((0.25, 0.02, 8), (0.1, 0.02, 8), (1.0, 0.05, 5), (0.25, 1.0, 8), (0.25, 0.0, 8))]


def _points(P, seed):
    rng = np.random.default_rng(100 + seed)
    return rng.standard_normal(P).astype(np.float32), (0.3 * rng.standard_normal(P)).astype(np.float32)


@pytest.mark.parametrize("func,P,fraction,max_dist,steps,seed", CASES)
def test_fp32_restatement_against_the_literal_one(func, P, fraction, max_dist, steps, seed):
    grad, lip, _ = FUNCS[func](P, seed)
    x_in, x_base = _points(P, seed)
    bound = R.Bound(P, lip)
    a = R.literal(x_in, x_base, grad, steps, fraction, max_dist, bound=bound)
    b = R.run(x_in, x_base, grad, steps, fraction, max_dist)
    assert a["status"] == b["status"] == R.OK and np.array_equal(a["iters"], b["iters"]), (a["iters"], b["iters"])
    assert R.same_trace(a["trace"], b["trace"]), "the two restatements take different decisions: choose another seed for this case"
    ex = np.abs(b["x"].astype(np.float64) - a["x"])
    assert (ex <= bound.e).all(), f"x: {float((ex / np.maximum(bound.e, 1e-300)).max()):.3f} x the bound"
    vb = bound.values_bound(a["attr"])
    ev = np.abs(b["values"].astype(np.float64) - a["attr"])
    ratio, size = float((ev / vb).max()), float(vb.max() / np.abs(a["attr"]).max())
    print(f"{func} P = {P} fraction {fraction} max_dist {max_dist}: passes {a['iters'].tolist()}, values {ratio:.3f} x the bound, the bound {size:.2e} of the largest value")
    assert np.isfinite(vb).all() and ratio <= 1.0 and size < 1e-2


@pytest.mark.parametrize("func", sorted(FUNCS))
@pytest.mark.parametrize("P", [1, 7, 250])
def test_max_dist_zero_is_the_left_riemann_sum(func, P):
    grad, _, _ = FUNCS[func](P, 11)
    x_in, x_base = _points(P, 11)
    for steps in (1, 8):
        want = R.left_riemann(x_in, x_base, grad, steps)
        a = R.literal(x_in, x_base, grad, steps, 0.25, 0.0)
        assert a["status"] == R.OK and (a["iters"] == 1).all()
        assert np.abs(a["attr"] - want).max() <= 1e-13 * np.abs(want).max()
        b = R.run(x_in, x_base, grad, steps, 0.25, 0.0)                     # fp32 points: the same sum within their rounding
        assert b["status"] == R.OK and (b["iters"] == 1).all() and np.array_equal(b["x"], x_in)
        assert np.abs(b["attr"] - want).max() <= 1e-5 * np.abs(want).max()


def test_completeness_error_falls_with_the_steps():
    P = 250
    grad, _, F = _quadratic(P, 21)
    x_in, x_base = _points(P, 21)
    delta = {}
    for steps in (8, 64):
        a = R.literal(x_in, x_base, grad, steps, 0.25, 0.02)
        assert a["status"] == R.OK
        delta[steps] = abs(a["attr"].sum() - (F(x_in.astype(np.float64)) - F(x_base.astype(np.float64))))
    print(f"completeness error of the quadratic form: {delta[8]:.3e} at 8 steps, {delta[64]:.3e} at 64")
    assert delta[64] <= 0.5 * delta[8]


def test_input_at_the_baseline_returns_zeros():
    grad, _, _ = _quadratic(7, 3)
    x = _points(7, 3)[0]
    a, b = R.literal(x, x, grad, 4, 0.25, 0.02), R.run(x, x, grad, 4, 0.25, 0.02)
    for r in (a, b):
        assert r["status"] == R.OK and not r["attr"].any() and not r["iters"].any() and np.array_equal(r["x"], x) and r["L_total"] == 0


def test_row_sum_and_select():
    rng = np.random.default_rng(5)
    for P in (1, 63, 64, 65, 1024, 1025, 5000):
        v = np.abs(rng.standard_normal(P))
        assert abs(R.row_sum(v) - math.fsum(v)) <= 1e-13 * math.fsum(v)
    assert R.row_sum([1.0]) == 1.0 and R.row_sum(np.ones(2049)) == 2049.0
    keys = np.array([2.0, 1.0, 1.0, 5.0, 1.0, 9.0])
    arrived = np.array([False, False, True, False, False, False])
    assert R._select(keys, arrived, 0).tolist() == [False, True, False, False, True, False]          # every tie of theta, no arrived cell
    assert R._select(keys, arrived, 2).tolist() == [True, True, False, False, True, False]
    assert R._select(keys, np.array([True] * 5 + [False]), 3).tolist() == [False] * 5 + [True]        # theta = +inf: every cell that has not arrived
    assert not R._select(keys, np.ones(6, dtype=bool), 3).any()


@pytest.mark.parametrize("func", sorted(FUNCS))
def test_pass_cap_against_observed_counts(func):
    """ceil(P / (k + 1)) + 2 bounds every step's passes, and is nearly reached where one cell moves per pass (k = 0); a cap below what a
    step needs stops the row with CAP, in both restatements at the same pass."""
    for P, fraction in ((7, 0.25), (250, 0.25), (250, 0.1), (63, 0.01), (250, 1.0)):
        grad, _, _ = FUNCS[func](P, 31)
        x_in, x_base = _points(P, 31)
        k = R.rank_k(P, fraction)
        cap = R.pass_cap(P, k)
        assert (k, cap) == brainxai.guided_ig_passes(P, fraction)
        a = R.literal(x_in, x_base, grad, 6, fraction, 0.02)
        assert a["status"] == R.OK and a["cap"] == cap and a["iters"].max() <= cap - 1, (P, fraction, a["iters"], cap)
        print(f"{func} P = {P} fraction {fraction}: k = {k}, cap {cap}, passes {a['iters'].tolist()}")
    assert brainxai.guided_ig_passes(63, 0.01) == (0, 65) and brainxai.guided_ig_passes(38000, 0.25) == (9499, 6) and brainxai.guided_ig_passes(1, 1.0) == (0, 3)
    grad, _, _ = FUNCS[func](63, 31)
    x_in, x_base = _points(63, 31)
    free = R.literal(x_in, x_base, grad, 6, 0.01, 0.02)
    assert free["iters"].max() > 5
    for run in (R.literal, R.run):
        short = run(x_in, x_base, grad, 6, 0.01, 0.02, cap=5)
        first = int(np.argmax(free["iters"] > 5))
        assert short["status"] == R.CAP and short["iters"][first] == 5 and not short["iters"][first + 1:].any() and (short["iters"][:first] == free["iters"][:first]).all()


def test_a_nan_gradient_stops_the_row():
    grad, _, _ = _quadratic(7, 3)
    x_in, x_base = _points(7, 3)
    calls = []

    def bad(x):
        calls.append(1)
        g = grad(x)
        if len(calls) == 3:
            g[2] = np.nan
        return g
    for run in (R.literal, R.run):
        calls.clear()
        r = run(x_in, x_base, bad, 5, 0.25, 0.02)
        assert r["status"] == R.NAN and (r["iters"][:2] > 0).all() and not r["iters"][2:].any() and np.isfinite(r["attr"]).all()


# ---- refusals of the driver -------------------------------------------------------------------------------------------------------------
B, C, H, W, CH, T = 2, 4, 16, 24, 19, 2000


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


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


BAD = {
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "guided_ig: unknown input"),
    "input_none_eeg": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "input_none_spec": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "steps_zero": ("multimodal", dict(steps=0), ValueError, "steps = 0 < 1"),
    "steps_negative": ("multimodal", dict(steps=-2), ValueError, "steps = -2 < 1"),
    "steps_float": ("multimodal", dict(steps=2.5), ValueError, "steps must be an int"),
    "steps_bool": ("eegnet", dict(input="eeg", steps=True), ValueError, "steps must be an int"),
    "fraction_zero": ("multimodal", dict(fraction=0.0), ValueError, r"fraction must be a number in \(0, 1\]"),
    "fraction_above": ("multimodal", dict(fraction=1.5), ValueError, r"fraction must be a number in \(0, 1\]"),
    "fraction_nan": ("deep", dict(input="eeg", fraction=float("nan")), ValueError, r"fraction must be a number in \(0, 1\]"),
    "fraction_word": ("multimodal", dict(fraction="0.25"), ValueError, r"fraction must be a number in \(0, 1\]"),
    "max_dist_negative": ("multimodal", dict(max_dist=-0.1), ValueError, r"max_dist must be a number in \[0, 1\]"),
    "max_dist_above": ("eegnet", dict(input="eeg", max_dist=1.01), ValueError, r"max_dist must be a number in \[0, 1\]"),
    "max_dist_nan": ("multimodal", dict(max_dist=float("nan")), ValueError, r"max_dist must be a number in \[0, 1\]"),
    "max_dist_bool": ("multimodal", dict(max_dist=True), ValueError, r"max_dist must be a number in \[0, 1\]"),
    "fraction_too_small": ("multimodal", dict(input="eeg", fraction=1e-4), ValueError, "too small for an input of 38000 cells"),
    "fraction_too_small_spec": ("spectrogram", dict(fraction=0.0006), ValueError, "too small for an input of 1536 cells"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(3, 5)), ValueError, "baseline of shape"),
    "baseline_word": ("multimodal", dict(baseline="grey"), ValueError, "baseline is neither"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg_all": ("multimodal", dict(input="eeg", class_idx="all", max_dist=0.0), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(class_idx=3, return_parts=True, baseline=torch.zeros(B, C, H, W)), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", class_idx="all", fraction=1.0, keep_path=True), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", class_idx=torch.tensor([5, 0]), max_batch=3, baseline=torch.zeros(CH)), RuntimeError, "no CPU path"),
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
    args = dict(steps=5)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.guided_ig(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    with pytest.raises(ValueError, match="cells per sample"):             # a row of 2^20 cells
        brainxai.guided_ig(model, None, one.expand(1, 1, 1024, 1024), steps=1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * per
        brainxai.guided_ig(model, None, one.expand(128, 1, 1000, 1000), steps=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * steps
        brainxai.guided_ig(model, None, one.expand(1 << 15, 1, 2, 2), steps=1 << 16)
    with pytest.raises(ValueError, match="65535"):                        # B * Kc rows
        brainxai.guided_ig(model, None, one.expand(4096, 1, 2, 2), steps=1, class_idx="all")
    assert reached == []


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
BX_EINVAL, BX_EUNSUPPORTED = -1, -6


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def init(Bn=3, Kc=2, P=100):
        return lib.bx_guided_ig_init(None, None, 0, None, None, None, None, Bn, Kc, P, None)

    def step(Bn=3, Kc=2, P=100, i=0, n=4, k=24, max_dist=0.02, cap=6, row0=0, rows=6):
        return lib.bx_guided_ig_step(None, None, None, None, None, None, None, None, Bn, Kc, P, i, n, k, max_dist, cap, row0, rows, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(Kc=0), b"bad shape"), (dict(P=0), b"bad shape"), (dict(), b"null pointer")]:
        assert init(**kw) == BX_EINVAL and b"bx_guided_ig_init" in msg() and word in msg(), (kw, msg())
    for kw, word in [(dict(P=1 << 20), b"cells"), (dict(Bn=1 << 15, Kc=2), b"rows, supported"), (dict(Bn=1 << 12, Kc=1, P=(1 << 20) - 1), b"32-bit")]:
        assert init(**kw) == BX_EUNSUPPORTED and word in msg(), (kw, msg())
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(P=0), b"bad shape"), (dict(i=4), b"step 4"), (dict(i=-1), b"step -1"), (dict(n=0), b"step"),
                     (dict(k=100), b"rank k"), (dict(k=-1), b"rank k"), (dict(max_dist=-0.5), b"max_dist"), (dict(max_dist=1.5), b"max_dist"),
                     (dict(max_dist=float("nan")), b"max_dist"), (dict(cap=0), b"cap"), (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"),
                     (dict(row0=4, rows=3), b"rows row0"), (dict(), b"null pointer")]:
        assert step(**kw) == BX_EINVAL and b"bx_guided_ig_step" in msg() and word in msg(), (kw, msg())
    for kw, word in [(dict(P=1 << 20, k=0), b"cells"), (dict(Bn=1 << 15, Kc=2), b"rows, supported"), (dict(Bn=1 << 12, Kc=1, P=(1 << 20) - 1), b"32-bit"),
                     (dict(Bn=1 << 15, Kc=1, n=1 << 16), b"32-bit")]:
        assert step(**kw) == BX_EUNSUPPORTED and word in msg(), (kw, msg())
