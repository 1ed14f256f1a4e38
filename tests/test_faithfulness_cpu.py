"""CPU: deletion / insertion argument checks that run before anything reaches a device, the limits of the bx_rank_desc / bx_faith_*
entry points, and the restatement (tests/faith_ref.py) against the counting definition of the rank and numpy's trapezoid rule."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import faith_ref as R

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


B, C, H, W, CH, T = 2, 4, 16, 24, 19, 2000


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


SPEC_MAP, EEG_MAP, COL_MAP = torch.rand(B, H, W), torch.rand(B, CH, T), torch.rand(B, 1, T)

# name -> (model kind, keyword overrides, exception, message)
BAD = {
    "map_shape_spec": ("multimodal", dict(attribution=torch.rand(B, H, W + 1)), ValueError, "wrong map shape"),
    "map_shape_spec_channels": ("multimodal", dict(attribution=torch.rand(B, C, H, W)), ValueError, "wrong map shape"),
    "map_shape_eeg": ("multimodal", dict(input="eeg", attribution=torch.rand(B, CH, T // 4)), ValueError, "wrong map shape"),
    "map_for_other_input": ("multimodal", dict(input="eeg", attribution=SPEC_MAP), ValueError, "wrong map shape"),
    "input_none_eeg": ("eegnet", dict(input="spec", attribution=SPEC_MAP), ValueError, "tensor is None"),
    "input_none_spec": ("spectrogram", dict(input="eeg", attribution=EEG_MAP), ValueError, "tensor is None"),
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "unknown input"),
    "steps_zero": ("multimodal", dict(steps=0), ValueError, "steps = 0"),
    "steps_above_n": ("multimodal", dict(steps=H * W + 1), ValueError, f"steps = {H * W + 1}"),
    "steps_above_n_columns": ("multimodal", dict(input="eeg", attribution=COL_MAP, steps=T + 1), ValueError, f"steps = {T + 1}"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "mode": ("multimodal", dict(mode="morf"), ValueError, "unknown mode"),
    "score": ("multimodal", dict(score="logit"), ValueError, "unknown score"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("multimodal", dict(class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_all": ("multimodal", dict(class_idx="all"), ValueError, "class_idx"),
    "baseline_length": ("multimodal", dict(baseline=[0.0, 1.0, 2.0]), ValueError, "baseline of shape"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(B, C, H, W - 1)), ValueError, "baseline of shape"),
    "baseline_per_channel_for_eeg": ("eegnet", dict(input="eeg", attribution=EEG_MAP, baseline=torch.zeros(C)), ValueError, "baseline of shape"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", dict(input="eeg", attribution=COL_MAP, baseline=torch.zeros(CH)), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(baseline=torch.zeros(B, C, H, W), class_idx=[1, 2], mode="deletion", score="logprob"), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", attribution=EEG_MAP, baseline=torch.zeros(B, 1, CH, T)), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", attribution=COL_MAP, class_idx=torch.tensor([5, 0])), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kind, kw, exc, match = BAD[case]
    eeg, spec = _inputs()
    if kind == "multimodal":
        model = brainxai.build_multimodal(CH, T, C)
    elif kind == "spectrogram":
        model, eeg = brainxai.Spectrogram_Model(6, in_channels=C), None
    else:
        model = brainxai.EEGNet(6, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(6, Chans=CH, Samples=T)
        spec = None
    args = dict(attribution=SPEC_MAP, steps=8)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.deletion_insertion(model, eeg, spec, args.pop("attribution"), **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_attribution_ranks_refuses_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.attribution_ranks(torch.rand(2, 5, 7))
    with pytest.raises(ValueError, match="at least two axes"):
        brainxai.attribution_ranks(torch.rand(7))
    with pytest.raises(ValueError, match="cells per sample"):
        brainxai.attribution_ranks(torch.empty(1, 1 << 20))
    assert reached == []


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    big = 1 << 20

    def rank(Bn=1, N=100, ws=0):
        return lib.bx_rank_desc(None, None, Bn, N, None, ws, None)
    for kw, code, word in [(dict(N=big), BX_EUNSUPPORTED, b"cells per row"), (dict(N=0), BX_EINVAL, b"bad shape"), (dict(Bn=0), BX_EINVAL, b"bad shape"),
                           (dict(Bn=4096, N=big - 1), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = rank(**kw)
        assert rc == code and b"bx_rank_desc" in msg() and word in msg(), (kw, rc, msg())
    for Bn, N in [(1, big), (1, 0), (0, 10), (4096, big - 1), (-1, 5)]:
        assert lib.bx_rank_desc_workspace(Bn, N) == 0
    sizes = [lib.bx_rank_desc_workspace(1, N) for N in (1, 7, 32768, 120000, big - 1)]
    assert sizes[0] >= 8 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.bx_rank_desc_workspace(64, 32768) >= 64 * sizes[2]

    def spec(Bn=1, Cc=3, Hh=8, Ww=8, Cp=8, per=4, i0=0, n=5, ins=0, dt=_lib.BX_F32, kind=0):
        return lib.bx_faith_perturb_spec(None, None, None, kind, None, Bn, Cc, Hh, Ww, Cp, per, i0, n, ins, dt, None)
    for kw, code, word in [(dict(Hh=1024, Ww=1024), BX_EUNSUPPORTED, b"cells per sample"), (dict(Cc=5), BX_EUNSUPPORTED, b"channels"),
                           (dict(Cc=0), BX_EUNSUPPORTED, b"channels"), (dict(per=0), BX_EINVAL, b"per = 0"), (dict(per=65), BX_EINVAL, b"per = 65"),
                           (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(Hh=0), BX_EINVAL, b"bad shape"), (dict(Cp=16), BX_EINVAL, b"Cp"),
                           (dict(i0=-1), BX_EINVAL, b"points i0"), (dict(n=0), BX_EINVAL, b"points i0"),
                           (dict(i0=60, n=6), BX_EINVAL, b"points i0"), (dict(kind=3), BX_EINVAL, b"baseline_kind"),
                           (dict(Hh=1000, Ww=1000, per=31250, n=33, Bn=8), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = spec(**kw)
        assert rc == code and b"bx_faith_perturb_spec" in msg() and word in msg(), (kw, rc, msg())
    assert spec(dt=7) < 0 and b"dtype" in msg()
    # several points at the clamped cut are part of the contract: 64 cells, per = 3 (steps = 22..31), points up to 31 have k = 64
    for kw in (dict(i0=12, n=5), dict(per=3, i0=0, n=32), dict(per=3, i0=25, n=7), dict(per=64, i0=0, n=65), dict(Hh=1, Ww=7, per=2, n=6)):
        assert spec(**kw) == BX_EINVAL and b"null pointer" in msg(), (kw, msg())

    def eeg(Bn=1, Ch=19, Tt=200, rows=19, per=100, i0=0, n=5, ins=0, kind=0):
        return lib.bx_faith_perturb_eeg(None, None, rows, None, kind, None, Bn, Ch, Tt, per, i0, n, ins, None)
    for kw, code, word in [(dict(Ch=64, Tt=16384, rows=64), BX_EUNSUPPORTED, b"cells per sample"), (dict(rows=2), BX_EINVAL, b"map_rows"),
                           (dict(per=0), BX_EINVAL, b"per = 0"), (dict(rows=1, per=201), BX_EINVAL, b"per = 201"), (dict(Tt=0), BX_EINVAL, b"bad shape"),
                           (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(rows=1, per=4, i0=199, n=3), BX_EINVAL, b"points i0"), (dict(kind=-1), BX_EINVAL, b"baseline_kind"),
                           (dict(Bn=64, Ch=64, Tt=15000, rows=1, per=150, n=33), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = eeg(**kw)
        assert rc == code and b"bx_faith_perturb_eeg" in msg() and word in msg(), (kw, rc, msg())

    for kw in (dict(i0=38, n=2), dict(rows=1, Tt=2000, per=32, n=65), dict(rows=1, Tt=2000, per=2, i0=1400, n=101)):   # T = 2000 columns, steps = 64 / 1500
        assert eeg(**kw) == BX_EINVAL and b"null pointer" in msg(), (kw, msg())

    def curve(Bn=2, P=9, K=6):
        return lib.bx_faith_curve(None, None, None, None, Bn, P, K, 0, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(P=1), b"bad shape"), (dict(K=0), b"bad shape"), (dict(Bn=1 << 20, P=1025, K=6), b"32-bit"),
                     (dict(), b"null pointer")]:
        rc = curve(**kw)
        assert rc == BX_EINVAL and b"bx_faith_curve" in msg() and word in msg(), (kw, rc, msg())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _special_rows():
    nan, inf = np.float32("nan"), np.float32("inf")
    g = np.random.default_rng(3)
    rows = [np.array([0.5, -0.0, 0.0, nan, inf, -inf, 0.5, nan, -0.0, 2.0, -inf, inf, 0.0, -1.0], dtype=np.float32),
            np.zeros(14, dtype=np.float32),
            np.floor(g.random(14) * 3).astype(np.float32),
            g.standard_normal(14).astype(np.float32),
            np.array([nan] * 7 + [-inf] * 7, dtype=np.float32)]
    return np.stack(rows)


def test_rank_restatement_equals_the_counting_definition():
    a = _special_rows()
    got, want = R.ranks(a), R.ranks_by_counting(a)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert all(np.array_equal(np.sort(r), np.arange(a.shape[1])) for r in got)
    # the documented consequences: +inf first, NaN with -inf last, ties (also -0.0 with +0.0, NaN with -inf) by ascending index
    assert list(got[0][[4, 11]]) == [0, 1] and list(got[0][[3, 5, 7, 10]]) == [10, 11, 12, 13]
    assert list(got[0][[1, 2, 8, 12]]) == [5, 6, 7, 8]
    assert np.array_equal(got[1], np.arange(14)) and np.array_equal(got[4], np.arange(14))
    g = np.random.default_rng(8)
    b = np.floor(g.random((3, 300)) * 8).astype(np.float32) / 8
    assert np.array_equal(R.ranks(b), R.ranks_by_counting(b))
    assert np.array_equal(R.ranks(b.reshape(3, 20, 15)), R.ranks(b))                   # cells are the flattened trailing axes


@pytest.mark.parametrize("steps", [1, 2, 16, 33])
def test_auc_restatement_equals_numpy_trapezoid(steps):
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    curve = np.random.default_rng(steps).random(steps + 1).astype(np.float32)
    got, want = R.auc(curve), trapezoid(curve.astype(np.float64), dx=1.0 / steps)
    # both are sums of steps + 1 positive terms in some order: each addition rounds by at most eps of a partial sum <= ~2 steps x want
    assert abs(got - want) <= 2 * (steps + 2) * np.finfo(np.float64).eps * want, (got, want)


@pytest.mark.parametrize("N,steps", [(8192, 16), (7500, 16), (38000, 32), (7, 7), (7, 3), (1, 1)])
def test_cuts_and_perturbed_inputs(N, steps):
    per, ks = R.cuts(N, steps)
    assert per == -(-N // steps) and len(ks) == steps + 1 and ks[0] == 0 and ks[-1] == N and all(0 <= k <= N for k in ks)
    x = torch.arange(2 * 3 * N, dtype=torch.float64).reshape(2, 3, 1, N) + 1
    rank = R.ranks(np.random.default_rng(N).random((2, N)).astype(np.float32))
    for k in (ks[0], ks[len(ks) // 2], ks[-1]):
        d, i = R.perturbed(x, rank, 0.0, k, False), R.perturbed(x, rank, 0.0, k, True)
        assert torch.equal(d + i, x) and int((d[:, 0] == 0).sum()) == 2 * k and int((i[:, 0] != 0).sum()) == 2 * k
    assert torch.equal(R.perturbed(x, rank, -1.0, 0, False), x) and torch.equal(R.perturbed(x, rank, -1.0, N, True), x)
    assert bool((R.perturbed(x, rank, [7.0, 8.0, 9.0], N, False)[:, 1] == 8.0).all())
