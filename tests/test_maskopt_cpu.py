"""CPU: the restatement of the optimised perturbation masks (tests/maskopt_ref.py) against torch autograd, the properties the
definition promises, and the argument checks of brainxai.mask_explain that run before anything reaches a device.

Restatement against torch.  On a toy score (a fixed random linear map plus log-softmax, fp64) the restatement's G at every iteration and
its grids after 5 Adam iterations are compared with autograd through F.interpolate(mode="bilinear", align_corners=False) and
torch.optim.Adam + clamp_, everything in fp64 on torch's side.  The two differ by the fp32 rounding of the interpolation weights, of
x - base, of m, and of the gradient and the output the restatement is handed (the definition's g and y are fp32).  Both start from the
same random grid in (0.2, 0.8) instead of all ones: from all ones the first Adam step moves every cell by lr up to a few 1e-9, which
fp32 storage rounds away, so the neighbour differences are exactly 0 in the restatement and of either sign in fp64 -- TV_1's sign(d)
then differs by the whole term, which says nothing about either side.
Measured here (seed 0; the worst over the 12 + 2 cases, relative to the largest |G| of the case, and absolute on grids in [0, 1]):
    G      1.384e-6 (the [1,T] domain; 2.7e-7 elsewhere)        the grids after 5 iterations      9.70e-7
The bounds are 10 x those figures (headroom for another seed): G_TOL = 1.4e-5, M_TOL = 9.7e-6."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib
from tests import maskopt_ref as R

G_TOL, M_TOL = 1.4e-5, 9.7e-6
SET = dict(lr=0.02, l1=0.01, tv_w=0.2, b1=0.9, b2=0.999, eps=1e-8)


# ---- the restatement against torch ------------------------------------------------------------------------------------------------------
def _case(shape, map_rows, gh, gw, kind, K=4, Kc=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    B = shape[0]
    per = int(np.prod(shape[1:]))
    base = {0: np.float32(0.25), 1: rng.standard_normal(shape[2] if map_rows else shape[1]).astype(np.float32) * 0.3,
            2: (0.3 * rng.standard_normal(shape)).astype(np.float32)}[kind]
    A = torch.from_numpy(rng.standard_normal((K, per)) / np.sqrt(per))
    b = torch.from_numpy(rng.standard_normal(K))
    m0 = rng.uniform(0.2, 0.8, (B * Kc, gh, gw)).astype(np.float32)
    classes = rng.integers(0, K, B * Kc)
    return x, base, A, b, m0, classes


def _toy(A, b, X):
    return torch.log_softmax(X.reshape(len(X), -1) @ A.T + b, dim=1)


def _restated(x, base, kind, A, b, m0, classes, map_rows, Kc, mode, score, beta, n):
    st = R.init(len(m0), *m0.shape[1:])
    st["m"][:] = m0
    history = np.zeros((len(m0), n, 3))
    Gs = []
    for it in range(n):
        rows = torch.from_numpy(R.rows(x, base, kind, st["m"], Kc, map_rows)).double().requires_grad_(True)
        logp = _toy(A, b, rows)
        (g,) = torch.autograd.grad(logp[torch.arange(len(m0)), torch.from_numpy(classes)].sum(), rows)
        G = np.zeros(m0.shape)
        R.step(st, x, base, kind, g.float().numpy(), logp.detach().float().numpy(), classes, map_rows, Kc, it, history, mode=mode, score=score, beta=beta,
               G_out=G, **SET)
        Gs.append(G)
    assert not st["status"].any()
    return np.stack(Gs), st["m"], history


def _torch_side(x, base, kind, A, b, m0, classes, map_rows, Kc, mode, score, beta, n):
    xp, by_row = R.planes(x, map_rows)
    bp = torch.from_numpy(np.ascontiguousarray(R.base_planes(base, kind, xp, by_row))).double()
    xp = torch.from_numpy(xp).double()
    Hm, Wm = xp.shape[2:]
    m = torch.from_numpy(m0).double().requires_grad_(True)
    opt = torch.optim.Adam([m], lr=SET["lr"], betas=(SET["b1"], SET["b2"]), eps=SET["eps"])
    samples = torch.arange(len(m0)) // Kc
    cls = torch.from_numpy(classes)
    Gs = []
    for _ in range(n):
        opt.zero_grad()
        M = F.interpolate(m[:, None], size=(Hm, Wm), mode="bilinear", align_corners=False)
        X = bp[samples] + M * (xp[samples] - bp[samples])
        logp = _toy(A, b, X)[torch.arange(len(m0)), cls]
        s = logp if score == R.LOGPROB else logp.exp()
        tv = ((m[:, :, 1:] - m[:, :, :-1]).abs() ** beta).sum((1, 2)) + ((m[:, 1:] - m[:, :-1]).abs() ** beta).sum((1, 2))
        area = (1 - m).mean((1, 2)) if mode == R.DELETION else m.mean((1, 2))
        loss = SET["l1"] * area + SET["tv_w"] * tv + (s if mode == R.DELETION else -s)
        loss.sum().backward()
        Gs.append(m.grad.detach().numpy().copy())
        opt.step()
        with torch.no_grad():
            m.clamp_(0, 1)
    return np.stack(Gs), m.detach().numpy()


def _compare(what, shape, map_rows, gh, gw, kind, mode, score, beta, n=5):
    x, base, A, b, m0, classes = _case(shape, map_rows, gh, gw, kind)
    G_r, m_r, hist = _restated(x, base, kind, A, b, m0, classes, map_rows, 2, mode, score, beta, n)
    G_t, m_t = _torch_side(x, base, kind, A, b, m0, classes, map_rows, 2, mode, score, beta, n)
    eg = float(np.abs(G_r - G_t).max() / np.abs(G_t).max())
    em = float(np.abs(m_r.astype(np.float64) - m_t).max())
    print(f"{what}: G {eg:.3e} of its maximum, grids after {n} iterations {em:.3e}; moved {float(np.abs(m_t - m0).max()):.3f}")
    assert float(np.abs(m_t - m0).max()) > 0.05, "the comparison needs grids that moved"
    assert eg <= G_TOL and em <= M_TOL, (eg, em)
    assert np.isfinite(hist).all() and (hist[:, :, 1] > 0).all()


@pytest.mark.parametrize("beta", [1, 2, 3])
@pytest.mark.parametrize("score", [R.PROB, R.LOGPROB])
@pytest.mark.parametrize("mode", [R.DELETION, R.PRESERVATION])
def test_restatement_against_torch_autograd_and_adam(mode, score, beta):
    _compare(f"spectrogram 3 x 10 x 13, grid 4 x 5, mode {mode}, score {score}, beta {beta}", (2, 3, 10, 13), 0, 4, 5, 1 + (beta % 2), mode, score, beta)


@pytest.mark.parametrize("map_rows,gh,kind", [(7, 3, 1), (1, 1, 2)])
def test_restatement_against_torch_eeg_domains(map_rows, gh, kind):
    _compare(f"EEG 7 x 45, map_rows {map_rows}", (2, 1, 7, 45), map_rows, gh, 6, kind, R.DELETION, R.PROB, 3)


# ---- properties -----------------------------------------------------------------------------------------------------------------------------
DOMAINS = [((1, 1), (1, 1)), ((1, 65), (1, 8)), ((5, 4), (5, 4)), ((19, 333), (1, 1)), ((19, 333), (7, 8)), ((100, 75), (7, 8)), ((100, 75), (32, 32)),
           ((70, 256), (16, 32)), ((19, 2000), (8, 8))]


@pytest.mark.parametrize("dom,grid", DOMAINS)
def test_all_ones_grid_upsamples_to_exactly_one(dom, grid):
    assert (R.upsample(np.ones(grid, dtype=np.float32), *dom) == np.float32(1.0)).all()
    z = R.upsample(np.zeros(grid, dtype=np.float32), *dom)
    assert not z.any()
    rng = np.random.default_rng(3)
    m = rng.uniform(0, 1, grid).astype(np.float32)
    M = R.upsample(m, *dom)
    assert M.min() >= m.min() - 1e-6 and M.max() <= m.max() + 1e-6
    want = F.interpolate(torch.from_numpy(m).double()[None, None], size=dom, mode="bilinear", align_corners=False)[0, 0].numpy()
    assert np.abs(M - want).max() <= 4e-6                                 # the fp32 weights against torch's fp64 ones: l carries the rounding of s <= 32


@pytest.mark.parametrize("dom,grid", DOMAINS)
def test_footprints_cover_every_pixel_and_hold_every_weight(dom, grid):
    for n, g in zip(dom, grid):
        i0, i1, l = R.axis(n, g)
        assert (np.diff(i0) >= 0).all() and i0.min() >= 0 and i1.max() <= g - 1 and (l >= 0).all() and (l < 1).all()
        w = R.weights(i0, i1, l, g)
        covered = np.zeros(n, dtype=int)
        for j in range(g):
            lo, hi = R.footprint(i0, j)
            covered[lo:hi] += 1
            assert not w[:lo, j].any() and not w[hi:, j].any(), "a weight outside the footprint"
        assert (covered >= 1).all()


def test_data_gradient_of_a_constant_t_sums_to_its_total():
    """The weights of a pixel are fl32(1 - l) and l.  Where n / g is a power of two, s has few bits, 1 - l is exact and they add up to
    exactly 1: the grid sum of G_data is the pixel sum of t within fp64 rounding (1e-13 of it: a few thousand adds of 2^-53 each).  At
    other shapes fl32(1 - l) carries one fp32 rounding, 2^-25 per axis, so the sums agree within 2^-24 of the total plus that."""
    for (Hm, Wm), (gh, gw), tol in [((64, 128), (8, 16), 1e-13), ((16, 16), (16, 16), 1e-13), ((100, 75), (7, 8), 2.0 ** -24 + 1e-13),
                                    ((19, 333), (7, 8), 2.0 ** -24 + 1e-13)]:
        x = np.full((1, 3, Hm, Wm), 0.75, dtype=np.float32)
        g = np.ones((1, 3, Hm, Wm), dtype=np.float32)
        G = R.data_gradient(x, np.float32(0.25), 0, g, 0, gh, gw, 1)
        total = 3 * 0.5 * Hm * Wm
        assert abs(G.sum() - total) <= tol * total, (Hm, Wm, gh, gw, G.sum() - total)


def _state(Rn, gh, gw, seed):
    rng = np.random.default_rng(seed)
    st = R.init(Rn, gh, gw)
    st["m"][:] = rng.uniform(0, 1, (Rn, gh, gw)).astype(np.float32)
    return st, rng


def test_zero_gradient_without_regularisers_leaves_the_grid_bit_for_bit():
    st, rng = _state(3, 5, 6, 1)
    x = rng.standard_normal((3, 2, 11, 13)).astype(np.float32)
    before = st["m"].copy()
    hist = np.zeros((3, 2, 3))
    for it in range(2):
        R.step(st, x, np.float32(0), 0, np.zeros((3, 2, 11, 13), dtype=np.float32), np.zeros((3, 4), dtype=np.float32), [0, 1, 2], 0, 1, it, hist,
               mode=R.DELETION, score=R.PROB, beta=3, lr=0.1, l1=0.0, tv_w=0.0, b1=0.9, b2=0.999, eps=1e-8)
    assert np.array_equal(st["m"].view(np.int32), before.view(np.int32)) and not st["mu"].any() and not st["nu"].any()
    assert (hist[:, :, 0] == 1.0).all() and np.allclose(hist[:, 0, 1], before.astype(np.float64).mean((1, 2)), rtol=1e-14)


def test_clamping_at_both_ends():
    st, rng = _state(2, 4, 4, 2)
    x = np.ones((2, 1, 8, 8), dtype=np.float32)
    g = np.ones((2, 1, 8, 8), dtype=np.float32)
    g[1] = -1.0
    hist = np.zeros((2, 1, 3))
    R.step(st, x, np.float32(0), 0, g, np.zeros((2, 3), dtype=np.float32), [0, 0], 0, 1, 0, hist, mode=R.DELETION, score=R.LOGPROB, beta=2, lr=5.0, l1=0.0, tv_w=0.0,
           b1=0.9, b2=0.999, eps=1e-8)
    assert (st["m"][0] == 0.0).all() and (st["m"][1] == 1.0).all()


def test_a_nan_stops_its_row_alone():
    st, rng = _state(3, 3, 4, 4)
    x = rng.standard_normal((3, 1, 9, 10)).astype(np.float32)
    hist = np.zeros((3, 3, 3))
    kw = dict(mode=R.PRESERVATION, score=R.PROB, beta=1, lr=0.1, l1=0.01, tv_w=0.2, b1=0.9, b2=0.999, eps=1e-8)
    for it in range(3):
        g = rng.standard_normal((3, 1, 9, 10)).astype(np.float32)
        y = np.log(np.full((3, 2), 0.5, dtype=np.float32))
        if it == 1:
            g[1, 0, 4, 7] = np.nan
        if it == 2:
            y[2, 1] = np.nan
        before = {k: st[k].copy() for k in ("m", "mu", "nu")}
        R.step(st, x, np.float32(0.1), 0, g, y, [0, 1, 1], 9, 1, it, hist, **kw)
        stopped = [r for r in range(3) if st["status"][r] == R.NAN]
        assert stopped == {0: [], 1: [1], 2: [1, 2]}[it]
        for r in range(3):
            same = all(np.array_equal(st[k][r], before[k][r]) for k in before)
            assert same == (r in stopped), (it, r)
    assert (hist[1, 1:] == 0).all() and (hist[2, 2] == 0).all() and (hist[0, :, 0] == 0.5).all()


def test_lane_sum_and_tv():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 1024):
        v = rng.uniform(0, 1, n)
        assert abs(R.lane_sum(v) - v.sum()) <= 1e-13 * v.sum()
    m = rng.uniform(0, 1, (6, 7)).astype(np.float32)
    for beta in (1, 2, 3):
        want = (np.abs(np.diff(m.astype(np.float64), axis=1)) ** beta).sum() + (np.abs(np.diff(m.astype(np.float64), axis=0)) ** beta).sum()
        assert abs(R.tv(m, beta) - want) <= 1e-13 * want
        md = torch.from_numpy(m).double().requires_grad_(True)
        tvt = ((md[:, 1:] - md[:, :-1]).abs() ** beta).sum() + ((md[1:] - md[:-1]).abs() ** beta).sum()
        tvt.backward()
        assert np.abs(R.tv_gradient(m, beta) - md.grad.numpy()).max() <= 1e-12          # the derivative against autograd's


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
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "mask_explain: unknown input"),
    "mode_unknown": ("multimodal", dict(mode="insertion"), ValueError, "mask_explain: unknown mode"),
    "score_unknown": ("multimodal", dict(score="logit"), ValueError, "mask_explain: unknown score"),
    "cells_unknown": ("multimodal", dict(input="eeg", cells="electrode"), ValueError, "mask_explain: unknown cells"),
    "cells_time_spec": ("multimodal", dict(cells="time"), ValueError, "cells='time' masks time columns"),
    "input_none_eeg": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "grid_zero": ("multimodal", dict(grid=0), ValueError, "grid = 0 < 1"),
    "grid_pair_zero": ("multimodal", dict(grid=(0, 4)), ValueError, r"grid 0 x 4 outside"),
    "grid_pair_33": ("multimodal", dict(input="eeg", grid=(4, 33)), ValueError, r"grid 4 x 33 outside"),
    "grid_above_domain": ("multimodal", dict(grid=(17, 4)), ValueError, r"grid 17 x 4 outside 1..min\(32, 16\)"),
    "grid_above_domain_time": ("eegnet", dict(input="eeg", cells="time", grid=(2, 8)), ValueError, r"grid 2 x 8 outside 1..min\(32, 1\)"),
    "grid_word": ("multimodal", dict(grid="fine"), ValueError, "grid must be an int or a pair"),
    "beta_zero": ("multimodal", dict(tv_beta=0), ValueError, "tv_beta must be 1, 2 or 3"),
    "beta_four": ("multimodal", dict(tv_beta=4), ValueError, "tv_beta must be 1, 2 or 3"),
    "beta_float": ("multimodal", dict(tv_beta=2.5), ValueError, "tv_beta must be 1, 2 or 3"),
    "iterations_zero": ("multimodal", dict(iterations=0), ValueError, "iterations = 0 < 1"),
    "iterations_float": ("multimodal", dict(iterations=2.5), ValueError, "iterations must be an int"),
    "lr_negative": ("multimodal", dict(lr=-0.1), ValueError, "lr must be a finite number >= 0"),
    "l1_negative": ("deep", dict(input="eeg", l1=-1e-3), ValueError, "l1 must be a finite number >= 0"),
    "tv_negative": ("multimodal", dict(tv=-0.2), ValueError, "tv must be a finite number >= 0"),
    "tv_nan": ("multimodal", dict(tv=float("nan")), ValueError, "tv must be a finite number >= 0"),
    "betas_one": ("multimodal", dict(betas=(0.9, 1.0)), ValueError, r"betas \(0.9, 1.0\) outside \[0, 1\)"),
    "betas_negative": ("multimodal", dict(betas=(-0.1, 0.999)), ValueError, r"outside \[0, 1\)"),
    "betas_single": ("multimodal", dict(betas=0.9), ValueError, "betas must be a pair"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(3, 5)), ValueError, "baseline of shape"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_eeg_time_all": ("multimodal", dict(input="eeg", cells="time", class_idx="all", mode="preservation", score="logprob"), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(class_idx=3, return_parts=True, baseline=torch.zeros(B, C, H, W), grid=(16, 24)), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", class_idx="all", keep_path=True, grid=64, tv_beta=1), RuntimeError, "no CPU path"),
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
    args = dict(iterations=3)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.mask_explain(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    with pytest.raises(ValueError, match="cells per mask"):               # a domain of 2^20 cells
        brainxai.mask_explain(model, None, one.expand(1, 1, 1024, 1024), iterations=1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * per
        brainxai.mask_explain(model, None, one.expand(128, 1, 1000, 1000), iterations=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * iterations * 3
        brainxai.mask_explain(model, None, one.expand(1 << 15, 1, 2, 2), iterations=1 << 15)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * iterations * per with keep_path
        brainxai.mask_explain(model, None, one.expand(64, 1, 256, 256), iterations=1024, keep_path=True)
    with pytest.raises(ValueError, match="65535"):                        # B * Kc rows
        brainxai.mask_explain(model, None, one.expand(4096, 1, 2, 2), iterations=1, class_idx="all")
    assert reached == []


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
BX_EINVAL, BX_EUNSUPPORTED = -1, -6


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def init(Bn=3, Kc=2, gh=4, gw=5, row0=0, rows=6):
        return lib.bx_maskopt_init(None, None, None, None, Bn, Kc, gh, gw, row0, rows, None)

    def masks(Bn=3, Kc=2, gh=4, gw=5, Hm=10, Wm=13, row0=0, rows=6):
        return lib.bx_maskopt_masks(None, None, Bn, Kc, gh, gw, Hm, Wm, row0, rows, None)

    def rows_spec(Bn=3, Kc=2, Cc=3, Hh=10, Ww=13, gh=4, gw=5, kind=0, row0=0, rows=6):
        return lib.bx_maskopt_rows_spec(None, None, None, kind, None, Bn, Kc, Cc, Hh, Ww, gh, gw, row0, rows, None)

    def rows_eeg(Bn=3, Kc=2, Chans=7, Tt=45, map_rows=7, gh=3, gw=5, kind=0, row0=0, rows=6):
        return lib.bx_maskopt_rows_eeg(None, None, map_rows, None, kind, None, Bn, Kc, Chans, Tt, gh, gw, row0, rows, None)

    def step(Bn=3, Kc=2, Cc=3, Hh=10, Ww=13, map_rows=0, K=6, gh=4, gw=5, kind=0, mode=0, score=0, beta=3, lr=0.1, l1=0.01, tv=0.2, b1=0.9, b2=0.999,
             eps=1e-8, c1=0.1, c2=0.001, it=0, n=4, row0=0, rows=6):
        return lib.bx_maskopt_step(None, None, kind, *([None] * 10), Bn, Kc, Cc, Hh, Ww, map_rows, K, gh, gw, mode, score, beta, lr, l1, tv, b1, b2, eps, c1, c2,
                                   it, n, row0, rows, None)
    for fn, name in ((init, b"bx_maskopt_init"), (masks, b"bx_maskopt_masks"), (rows_spec, b"bx_maskopt_rows_spec"), (rows_eeg, b"bx_maskopt_rows_eeg"),
                     (step, b"bx_maskopt_step")):
        for kw, word in [(dict(Bn=0), b"bad shape"), (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"), (dict(row0=4, rows=3), b"rows row0"),
                         (dict(gh=0), b"grid 0 x"), (dict(), b"null pointer")]:
            assert fn(**kw) == BX_EINVAL and name in msg() and word in msg(), (name, kw, msg())
        for kw, word in [(dict(gw=33), b"grid"), (dict(Bn=1 << 15), b"rows, supported")]:
            assert fn(**kw) == BX_EUNSUPPORTED and name in msg() and word in msg(), (name, kw, msg())
    for fn in (masks, rows_spec, step):
        assert fn(gh=11) == BX_EUNSUPPORTED and b"grid 11 x 5" in msg()                       # above the domain
    assert masks(Hm=1024, Wm=1024, gh=4) == BX_EUNSUPPORTED and b"cells per mask" in msg()
    assert rows_eeg(map_rows=3) == BX_EINVAL and b"map_rows=3" in msg()
    assert rows_eeg(map_rows=1, gh=3) == BX_EUNSUPPORTED and b"grid 3 x 5" in msg()          # a [1,T] domain has one row of cells
    assert rows_spec(kind=3) == BX_EINVAL and b"baseline_kind 3" in msg()
    for kw, word in [(dict(K=0), b"bad shape K"), (dict(mode=2), b"mode 2"), (dict(score=-1), b"score -1"), (dict(beta=0), b"tv_beta"), (dict(beta=4), b"tv_beta"),
                     (dict(lr=-1.0), b"must be >= 0"), (dict(l1=-1.0), b"must be >= 0"), (dict(tv=float("nan")), b"must be >= 0"), (dict(b1=1.0), b"betas"),
                     (dict(b2=-0.5), b"betas"), (dict(c1=0.0), b"bias corrections"), (dict(c2=1.5), b"bias corrections"), (dict(it=4), b"iteration 4"),
                     (dict(it=-1), b"iteration -1"), (dict(n=0), b"iteration"), (dict(map_rows=5), b"map_rows = 5")]:
        assert step(**kw) == BX_EINVAL and b"bx_maskopt_step" in msg() and word in msg(), (kw, msg())
    for kw, word in [(dict(K=33), b"33 classes"), (dict(Bn=1 << 12, Kc=1, Cc=1, Hh=1023, Ww=1024, rows=1), b"32-bit"), (dict(Bn=1 << 15, Kc=1, n=1 << 15), b"32-bit")]:
        assert step(**kw) == BX_EUNSUPPORTED and word in msg(), (kw, msg())
