"""CPU: brainxai.occlusion argument checks that run before anything reaches a device, the limits of the bx_occlusion_* entry points, and
the restatement of the definition (tests/occlusion_ref.py) against a literal Captum-style construction of the padded window masks."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib
from tests import occlusion_ref as R

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


# name -> (model kind, keyword overrides, exception, message); the spectrogram is 16 x 24, the EEG input 19 x 2000
BAD = {
    "window_zero": ("multimodal", dict(window=0), ValueError, "window 0 x 0"),
    "window_above_rows": ("multimodal", dict(window=(17, 4)), ValueError, "window 17 x 4"),
    "window_above_columns": ("spectrogram", dict(window=(4, 25)), ValueError, "window 4 x 25"),
    "window_int_above_electrodes": ("eegnet", dict(input="eeg", window=20), ValueError, "window 20 x 20"),
    "window_above_time": ("deep", dict(input="eeg", window=(1, 2001)), ValueError, "window 1 x 2001"),
    "window_triple": ("multimodal", dict(window=(4, 4, 4)), ValueError, "window must be"),
    "window_float": ("multimodal", dict(window=(4.0, 4)), ValueError, "window must be"),
    "window_bool": ("multimodal", dict(window=True), ValueError, "window must be"),
    "stride_zero": ("multimodal", dict(stride=0), ValueError, "stride 0 x 0"),
    "stride_negative": ("spectrogram", dict(stride=(2, -1)), ValueError, "stride 2 x -1"),
    "stride_above_window": ("multimodal", dict(stride=(5, 4)), ValueError, "stride 5 x 4"),
    "stride_above_window_eeg": ("eegnet", dict(input="eeg", window=(1, 250), stride=(1, 251)), ValueError, "stride 1 x 251"),
    "stride_word": ("multimodal", dict(stride="tiles"), ValueError, "stride must be"),
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "unknown input"),
    "score_unknown": ("multimodal", dict(score="logit"), ValueError, "unknown score"),
    "input_none_eeg": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "input_none_spec": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("deep", dict(input="eeg", window=(1, T), class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "baseline_length": ("multimodal", dict(baseline=[0.0, 1.0, 2.0]), ValueError, "occlusion: baseline of shape"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(B, C, H, W - 1)), ValueError, "occlusion: baseline of shape"),
    "baseline_per_channel_for_eeg": ("eegnet", dict(input="eeg", window=(1, T), baseline=torch.zeros(C)), ValueError, "occlusion: baseline of shape"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_all": ("multimodal", dict(class_idx="all", score="logprob", stride=1), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", dict(input="eeg", window=(1, T), baseline=torch.zeros(CH)), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(baseline=torch.zeros(B, C, H, W), class_idx=[1, 2], window=(5, 7), stride=(3, 4)), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", window=(CH, 250), stride=(CH, 125), baseline=torch.zeros(B, 1, CH, T)), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", window=(4, 300), stride=(3, 170), class_idx=torch.tensor([5, 0])), RuntimeError, "no CPU path"),
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
    args = dict(window=4)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.occlusion(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_offset_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    big = torch.zeros(1, 1, 1, 1).expand(128, 1, 1000, 1000)             # a view: 32 * 128 * 10^6 map values is past 2^31
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.occlusion(model, None, big, window=500, class_idx="all")
    with pytest.raises(ValueError, match="cells per sample"):
        brainxai.occlusion(model, None, torch.zeros(1, 1, 1, 1).expand(1, 1, 1024, 1024), window=8)
    assert reached == []


def test_geometry_helper_equals_the_reference():
    from brainxai import explain as X
    for Hm, Wm, window, stride in [(16, 24, (5, 7), (3, 4)), (100, 75, (32, 10), (32, 5)), (64, 128, (64, 128), None), (19, 2000, (1, 2000), None),
                                   (19, 2000, (19, 250), (19, 125)), (16, 24, 4, 1), (37, 3000, (4, 300), (3, 170))]:
        assert X._occlusion_geometry("occlusion", window, stride, Hm, Wm) == R.geometry(Hm, Wm, window, stride)


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    geom_cases = [(dict(Hm=0), BX_EINVAL, b"bad shape"), (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per map"), (dict(wh=0), BX_EINVAL, b"window 0 x 32"),
                  (dict(wh=65), BX_EINVAL, b"window 65 x 32"), (dict(ww=129), BX_EINVAL, b"window 16 x 129"), (dict(sh=0), BX_EINVAL, b"stride 0 x 16"),
                  (dict(sh=17), BX_EINVAL, b"stride 17 x 16"), (dict(sw=33), BX_EINVAL, b"stride 8 x 33"), (dict(sw=-1), BX_EINVAL, b"stride 8 x -1")]
    row_cases = [(dict(n0=-1), BX_EINVAL, b"windows n0"), (dict(n=0), BX_EINVAL, b"windows n0"), (dict(n0=40, n=10), BX_EINVAL, b"windows n0"),
                 (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(kind=3), BX_EINVAL, b"baseline_kind"), (dict(kind=-1), BX_EINVAL, b"baseline_kind")]

    def spec(Bn=1, Cc=3, Hm=64, Wm=128, Cp=8, wh=16, ww=32, sh=8, sw=16, n0=0, n=49, dt=_lib.BX_F32, kind=0):        # 7 x 7 windows
        return lib.bx_occlusion_perturb_spec(None, None, kind, None, Bn, Cc, Hm, Wm, Cp, wh, ww, sh, sw, n0, n, dt, None)
    for kw, code, word in geom_cases + row_cases + [(dict(Cc=5), BX_EUNSUPPORTED, b"channels"), (dict(Cc=0), BX_EUNSUPPORTED, b"channels"), (dict(Cp=16), BX_EINVAL, b"Cp"),
                                                    (dict(Hm=512, Wm=512, wh=1, ww=1, sh=1, sw=1, n=600), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                                                    (dict(wh=64, ww=128, sh=64, sw=128, n=1), BX_EINVAL, b"null pointer")]:
        rc = spec(**kw)
        assert rc == code and b"bx_occlusion_perturb_spec" in msg() and word in msg(), (kw, rc, msg())
    assert spec(dt=7) < 0 and b"dtype" in msg()

    def eeg(Bn=1, Hm=64, Wm=128, wh=16, ww=32, sh=8, sw=16, n0=0, n=49, kind=0):
        return lib.bx_occlusion_perturb_eeg(None, None, kind, None, Bn, Hm, Wm, wh, ww, sh, sw, n0, n, None)
    for kw, code, word in geom_cases + row_cases + [(dict(Bn=64, Hm=64, Wm=15000, wh=1, ww=15000, sh=1, sw=15000, n=64), BX_EINVAL, b"32-bit"),
                                                    (dict(), BX_EINVAL, b"null pointer"), (dict(Hm=19, Wm=2000, wh=1, ww=2000, sh=1, sw=2000, n=19), BX_EINVAL, b"null pointer")]:
        rc = eeg(**kw)
        assert rc == code and b"bx_occlusion_perturb_eeg" in msg() and word in msg(), (kw, rc, msg())

    def acc(Bn=2, N=49, K=6, Hm=64, Wm=128, wh=16, ww=32, sh=8, sw=16):
        return lib.bx_occlusion_accumulate(None, None, None, None, None, Bn, N, K, Hm, Wm, wh, ww, sh, sw, None)
    for kw, code, word in geom_cases + [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(K=0), BX_EINVAL, b"bad shape"), (dict(K=33), BX_EUNSUPPORTED, b"classes"),
                                        (dict(N=48), BX_EINVAL, b"7 x 7 windows"), (dict(N=50), BX_EINVAL, b"7 x 7 windows"),
                                        (dict(Bn=4096, K=32, Hm=512, Wm=512, wh=512, ww=512, sh=512, sw=512, N=1), BX_EINVAL, b"32-bit"),
                                        (dict(Bn=1 << 16, K=32, Hm=32, Wm=32, wh=1, ww=1, sh=1, sw=1, N=1024), BX_EINVAL, b"32-bit"),
                                        (dict(), BX_EINVAL, b"null pointer"), (dict(K=32), BX_EINVAL, b"null pointer")]:
        rc = acc(**kw)
        assert rc == code and b"bx_occlusion_accumulate" in msg() and word in msg(), (kw, rc, msg())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
# domain, window, stride (None = tiles), (ny, nx)
GEOMETRIES = {"16x24 window 5x7 stride 3x4": (16, 24, (5, 7), (3, 4), (5, 6)), "100x75 window 32x10 stride 32x5": (100, 75, (32, 10), (32, 5), (4, 14)),
              "64x128 one window": (64, 128, (64, 128), None, (1, 1)), "19x2000 electrodes": (19, 2000, (1, 2000), None, (19, 1)),
              "19x2000 window 19x250 stride 19x125": (19, 2000, (19, 250), (19, 125), (1, 15)), "16x24 window 4x4 stride 1": (16, 24, (4, 4), 1, (13, 21))}


def captum_style(drops, Hm, Wm, window, stride):
    """Captum's Occlusion, literally: for window j at current_index = (iy sh, ix sw), a ones tensor of the window's shape is padded with
    F.pad to the domain -- left pads = current_index, right pads = remaining = domain - (current_index + window), a negative pad crops
    -- and total += drop * mask, weights += mask; the attribution is total / weights.  drops [N] fp64."""
    wh, ww, sh, sw, ny, nx = R.geometry(Hm, Wm, window, stride)
    total, weights = torch.zeros(Hm, Wm, dtype=torch.float64), torch.zeros(Hm, Wm, dtype=torch.float64)
    window_tsr = torch.ones(wh, ww, dtype=torch.float64)
    for iy in range(ny):
        for ix in range(nx):
            current_index = (iy * sh, ix * sw)
            remaining = (Hm - (current_index[0] + wh), Wm - (current_index[1] + ww))
            pad_values = [val for pr in zip(remaining, current_index) for val in pr]
            pad_values.reverse()                                     # F.pad takes the last axis first: (left, right) = (current_index, remaining)
            mask = F.pad(window_tsr, tuple(pad_values))
            assert tuple(mask.shape) == (Hm, Wm)
            total += float(drops[iy * nx + ix]) * mask
            weights += mask
    return (total / weights).numpy(), weights.numpy()


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_restatement_equals_captum_style_construction(name):
    Hm, Wm, window, stride, grid = GEOMETRIES[name]
    geom = R.geometry(Hm, Wm, window, stride)
    assert geom[4:] == grid
    ny, nx = grid
    N = ny * nx
    m = R.masks(Hm, Wm, window, stride)
    cnt = R.counts(m)
    assert m.shape == (N, Hm, Wm) and cnt.min() >= 1
    assert (ny - 1) * geom[2] + geom[0] >= Hm and (nx - 1) * geom[3] + geom[1] >= Wm
    assert m[N - 1, Hm - 1, Wm - 1] and m[N - 1].sum() > 0 and m[0, 0, 0], "the last window touches the border"
    assert R.bounds(geom, Hm, Wm, N - 1)[1] == Hm and R.bounds(geom, Hm, Wm, N - 1)[3] == Wm
    if name == "16x24 window 4x4 stride 1":
        assert N == 273 and cnt.max() == 16
    # cnt(p) = cy(y) * cx(x) in closed form
    wh, ww, sh, sw = geom[:4]
    cy = np.array([min(ny - 1, y // sh) - max(0, -(-(y - wh + 1) // sh)) + 1 for y in range(Hm)])
    cx = np.array([min(nx - 1, x // sw) - max(0, -(-(x - ww + 1) // sw)) + 1 for x in range(Wm)])
    assert np.array_equal(cnt, cy[:, None] * cx[None, :])
    g = np.random.default_rng(N)
    S, S0 = g.random((2, N, 3)), g.random((2, 3))
    got = R.attribution(S, S0, m)
    for b in range(2):
        for k in range(3):
            want, weights = captum_style(S0[b, k] - S[b, :, k], Hm, Wm, window, stride)
            assert np.array_equal(weights, cnt.astype(np.float64))
            assert np.abs(got[b, k] - want).max() <= 16 * 2.0 ** -52 * np.abs(S0[b, k] - S[b, :, k]).max()       # the order of an fp64 sum of <= 16 terms


def test_perturbed_restatement_is_a_selection():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6) + 1
    x[0, 1, 2, 3] = -0.0
    m = R.masks(4, 6, (2, 3), (2, 2))
    assert m.shape == (2 * 3, 4, 6)
    got = R.perturbed(x, m[4], [7.0, 8.0, 9.0])                      # window (1, 1): rows 2..3, columns 2..4
    assert bool((got[:, 1, 2:4, 2:5] == 8.0).all()) and torch.equal(got[:, :, :2], x[:, :, :2]) and torch.equal(got[:, :, :, :2], x[:, :, :, :2])
    keep = R.perturbed(x, m[0], 0.5)
    assert torch.signbit(keep[0, 1, 2, 3]) and float(keep[0, 0, 0, 0]) == 0.5
    whole = R.perturbed(x, R.masks(4, 6, (4, 6))[0], -0.0)
    assert bool(torch.signbit(whole).all())
    e = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(2, 1, 5, 6)
    el = R.perturbed(e, R.masks(5, 6, (1, 6))[3], torch.arange(5.0) * 100)
    assert bool((el[:, 0, 3] == 300.0).all()) and torch.equal(el[:, 0, :3], e[:, 0, :3]) and torch.equal(el[:, 0, 4], e[:, 0, 4])


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_planted_cell(name):
    """Scores that drop only for the windows covering a cell p*.  The mean over a cell's windows reaches the full drop exactly where
    every window of the cell also covers p*, so the map's maximum is attained at p* and on the cells whose windows are a subset of
    p*'s.  Where no cell has a strict subset of p*'s windows (p* at a corner, where one window covers it, or far from the border) that
    set lies within the common intersection of p*'s windows; a cell covered by only some of p*'s windows reaches the maximum too."""
    Hm, Wm, window, stride, _ = GEOMETRIES[name]
    m = R.masks(Hm, Wm, window, stride)
    N = m.shape[0]
    flat = m.reshape(N, -1)
    checked = 0
    for spot in [(0, 0), (Hm // 2, Wm // 3), (Hm - 1, Wm - 1)]:
        covering = m[:, spot[0], spot[1]]
        S0 = np.full((1, 1), 0.9)
        S = np.where(covering, 0.2, 0.9).reshape(1, N, 1)
        amap = R.attribution(S, S0, m)[0, 0]
        common = m[covering].all(0)
        assert common[spot] and amap.max() == pytest.approx(0.7) and amap.min() >= 0.0 and amap[spot] == pytest.approx(0.7)
        attained = amap >= 0.7 * (1 - 1e-12)
        subset = ~(flat & ~covering[:, None]).any(0).reshape(Hm, Wm)      # cells none of whose windows misses p*
        assert np.array_equal(attained, subset)
        assert m[covering].any(0)[attained].all(), "outside p*'s windows the map is below its maximum"
        strict = subset & (flat.sum(0).reshape(Hm, Wm) < covering.sum())
        if not strict.any():
            checked += 1
            assert common[attained].all() and common[np.unravel_index(int(amap.argmax()), amap.shape)]
    assert checked >= 2                                              # the corners always qualify: one window covers them
