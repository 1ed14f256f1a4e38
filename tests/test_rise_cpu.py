"""CPU: brainxai.rise / brainxai.rise_masks argument checks that run before anything reaches a device, the limits of the bx_rise_*
entry points, and the restatement of the mask definition (tests/rise_ref.py) against F.interpolate plus crop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import rise_ref as R

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


def _set(N=5, gh=4, gw=4, Hm=H, Wm=W):
    return R.draw(N, gh, gw, Hm, Wm, 0.5, 1)


def _edit(pair, which, index, value):
    arrays = [a.copy() for a in pair]
    arrays[which][index] = value
    return tuple(arrays)


# name -> (model kind, keyword overrides, exception, message); the spectrogram is 16 x 24 and grid 4 gives 4 x 6 cells
BAD = {
    "grid_zero": ("multimodal", dict(grid=0), ValueError, "grid 0 x 0"),
    "grid_above_32": ("multimodal", dict(input="eeg", grid=(4, 33)), ValueError, "grid 4 x 33"),
    "grid_above_rows": ("multimodal", dict(grid=(17, 4)), ValueError, "grid 17 x 4"),
    "grid_above_electrodes": ("eegnet", dict(input="eeg", grid=20), ValueError, "grid 20 x 20"),
    "grid_rows_on_time_columns": ("eegnet", dict(input="eeg", cells="time", grid=(2, 8)), ValueError, "grid 2 x 8"),
    "grid_triple": ("multimodal", dict(grid=(4, 4, 4)), ValueError, "grid must be"),
    "p1_zero": ("multimodal", dict(p1=0.0), ValueError, "p1 = 0.0"),
    "p1_above_one": ("multimodal", dict(p1=1.5), ValueError, "p1 = 1.5"),
    "p1_negative": ("spectrogram", dict(p1=-0.5), ValueError, "p1 = -0.5"),
    "num_masks_zero": ("multimodal", dict(num_masks=0), ValueError, "num_masks = 0"),
    "masks_not_a_pair": ("multimodal", dict(masks=np.zeros((5, 4, 4), dtype=np.uint8)), ValueError, "masks must be a pair|bits of shape"),
    "masks_wrong_grid": ("multimodal", dict(masks=_set(gh=4, gw=5)), ValueError, "bits of shape"),
    "masks_shifts_shape": ("multimodal", dict(masks=(_set()[0], _set(N=6)[1])), ValueError, "shifts of shape"),
    "masks_shifts_float": ("multimodal", dict(masks=(_set()[0], _set()[1].astype(np.float32))), ValueError, "shifts of shape"),
    "masks_bits_two": ("multimodal", dict(masks=_edit(_set(), 0, (2, 1, 1), 2)), ValueError, "0 / 1 only"),
    "masks_bits_float": ("multimodal", dict(masks=(_set()[0] * 0.5, _set()[1])), ValueError, "0 / 1 only"),
    "masks_dy_at_cell": ("multimodal", dict(masks=_edit(_set(), 1, (3, 0), 4)), ValueError, r"shifts outside \[0, cell\)"),
    "masks_dx_at_cell": ("multimodal", dict(masks=_edit(_set(), 1, (0, 1), 6)), ValueError, r"shifts outside \[0, cell\)"),
    "masks_shift_negative": ("multimodal", dict(masks=_edit(_set(), 1, (4, 1), -1)), ValueError, r"shifts outside \[0, cell\)"),
    "time_cells_for_spec": ("multimodal", dict(cells="time"), ValueError, "cells='time'"),
    "cells_unknown": ("multimodal", dict(input="eeg", cells="electrode"), ValueError, "unknown cells"),
    "normalize_unknown": ("multimodal", dict(normalize="mean"), ValueError, "unknown normalize"),
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "unknown input"),
    "input_none_eeg": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "input_none_spec": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("multimodal", dict(class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "baseline_length": ("multimodal", dict(baseline=[0.0, 1.0, 2.0]), ValueError, "rise: baseline of shape"),
    "baseline_shape": ("multimodal", dict(baseline=torch.zeros(B, C, H, W - 1)), ValueError, "rise: baseline of shape"),
    "baseline_per_channel_for_eeg": ("eegnet", dict(input="eeg", baseline=torch.zeros(C)), ValueError, "rise: baseline of shape"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_all": ("multimodal", dict(class_idx="all", normalize="coverage", masks=_set()), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", dict(input="eeg", cells="time", grid=16, baseline=torch.zeros(CH)), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(baseline=torch.zeros(B, C, H, W), class_idx=[1, 2], grid=(2, 3)), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", grid=(4, 16), baseline=torch.zeros(B, 1, CH, T)), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", cells="time", class_idx=torch.tensor([5, 0])), RuntimeError, "no CPU path"),
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
    args = dict(num_masks=5, grid=4)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.rise(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_rise_masks_refuses_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.rise_masks((16, 24), num_masks=3, grid=4, device="cpu")
    with pytest.raises(ValueError, match="size must be a pair"):
        brainxai.rise_masks(16, num_masks=3)
    with pytest.raises(ValueError, match="cells per mask"):
        brainxai.rise_masks((1024, 1024), num_masks=3)
    with pytest.raises(ValueError, match="grid 8 x 8"):
        brainxai.rise_masks((4, 24), num_masks=3, grid=8)
    with pytest.raises(ValueError, match="shifts outside"):
        brainxai.rise_masks((16, 24), grid=4, masks=_edit(_set(), 1, (0, 0), 4))
    assert reached == []


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def masks(N=10, gh=8, gw=8, Hm=64, Wm=128, n0=0, n=10):
        return lib.bx_rise_masks(None, None, None, N, gh, gw, Hm, Wm, n0, n, None)
    shape_cases = [(dict(N=0, n=1), BX_EINVAL, b"bad shape"), (dict(Hm=0), BX_EINVAL, b"bad shape"), (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per mask"),
                   (dict(gh=0), BX_EINVAL, b"grid 0 x 8"), (dict(gw=33), BX_EUNSUPPORTED, b"grid 8 x 33"), (dict(Hm=7), BX_EUNSUPPORTED, b"grid 8 x 8"),
                   (dict(n0=-1), BX_EINVAL, b"masks n0"), (dict(n=0), BX_EINVAL, b"masks n0"), (dict(n0=6, n=5), BX_EINVAL, b"masks n0")]
    for kw, code, word in shape_cases + [(dict(N=1 << 20, n=1 << 20), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                                         (dict(gh=32, gw=32, Hm=32, Wm=32), BX_EINVAL, b"null pointer"), (dict(gh=1, gw=16, Hm=1, Wm=2000), BX_EINVAL, b"null pointer")]:
        rc = masks(**kw)
        assert rc == code and b"bx_rise_masks" in msg() and word in msg(), (kw, rc, msg())

    def spec(Bn=1, Cc=3, Hm=64, Wm=128, Cp=8, N=10, gh=8, gw=8, n0=0, n=10, dt=_lib.BX_F32, kind=0):
        return lib.bx_rise_perturb_spec(None, None, None, None, kind, None, Bn, Cc, Hm, Wm, Cp, N, gh, gw, n0, n, dt, None)
    for kw, code, word in shape_cases + [(dict(Cc=5), BX_EUNSUPPORTED, b"channels"), (dict(Cc=0), BX_EUNSUPPORTED, b"channels"), (dict(Cp=16), BX_EINVAL, b"Cp"),
                                         (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(kind=3), BX_EINVAL, b"baseline_kind"),
                                         (dict(Hm=512, Wm=512, N=600, n=600), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = spec(**kw)
        assert rc == code and b"bx_rise_perturb_spec" in msg() and word in msg(), (kw, rc, msg())
    assert spec(dt=7) < 0 and b"dtype" in msg()

    def eeg(Bn=1, Ch=19, Tt=2000, rows=19, N=10, gh=4, gw=16, n0=0, n=10, kind=0):
        return lib.bx_rise_perturb_eeg(None, None, None, rows, None, kind, None, Bn, Ch, Tt, N, gh, gw, n0, n, None)
    for kw, code, word in [(dict(rows=2), BX_EINVAL, b"map_rows"), (dict(Tt=0), BX_EINVAL, b"bad shape"), (dict(Ch=64, Tt=16384, rows=64), BX_EUNSUPPORTED, b"cells per mask"),
                           (dict(rows=1), BX_EUNSUPPORTED, b"grid 4 x 16"), (dict(gh=20), BX_EUNSUPPORTED, b"grid 20 x 16"), (dict(gw=0), BX_EINVAL, b"grid 4 x 0"),
                           (dict(n0=8, n=3), BX_EINVAL, b"masks n0"), (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(kind=-1), BX_EINVAL, b"baseline_kind"),
                           (dict(Bn=64, Ch=64, Tt=15000, rows=1, gh=1, N=40, n=40), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                           (dict(rows=1, gh=1), BX_EINVAL, b"null pointer")]:
        rc = eeg(**kw)
        assert rc == code and b"bx_rise_perturb_eeg" in msg() and word in msg(), (kw, rc, msg())

    def acc(Bn=2, N=10, K=6, gh=8, gw=8, Hm=64, Wm=128, p1=0.5, norm=0):
        return lib.bx_rise_accumulate(None, None, None, None, None, None, Bn, N, K, gh, gw, Hm, Wm, p1, norm, None)
    for kw, code, word in [(dict(N=0), BX_EINVAL, b"bad shape"), (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(K=0), BX_EINVAL, b"bad shape"),
                           (dict(K=33), BX_EUNSUPPORTED, b"classes"), (dict(gh=33), BX_EUNSUPPORTED, b"grid 33 x 8"), (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per mask"),
                           (dict(p1=0.0), BX_EINVAL, b"p1"), (dict(p1=1.25), BX_EINVAL, b"p1"), (dict(norm=2), BX_EINVAL, b"normalize"),
                           (dict(Bn=4096, N=1 << 20, K=6), BX_EINVAL, b"32-bit"), (dict(Bn=4096, K=32, Hm=512, Wm=512), BX_EINVAL, b"32-bit"),
                           (dict(), BX_EINVAL, b"null pointer"), (dict(p1=1.0, norm=1, K=32), BX_EINVAL, b"null pointer")]:
        rc = acc(**kw)
        assert rc == code and b"bx_rise_accumulate" in msg() and word in msg(), (kw, rc, msg())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
SHAPES = {"64x128 grid 8": (64, 128, 8, 8), "100x75 grid 7": (100, 75, 7, 7), "128x256 grid 8": (128, 256, 8, 8), "1x2000 grid 1x16": (1, 2000, 1, 16),
          "19x2000 grid 4x16": (19, 2000, 4, 16), "400x300 grid 7": (400, 300, 7, 7)}
BOUND = 2e-6                 # values in [0, 1], each a handful of fp32 roundings


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_restatement_equals_interpolate_plus_crop(shape):
    Hm, Wm, gh, gw = SHAPES[shape]
    bits, shifts = R.draw(64, gh, gw, Hm, Wm, 0.5, 7)
    ch, cw = R.cells(Hm, Wm, gh, gw)
    assert shifts[:, 0].max() < ch and shifts[:, 1].max() < cw and (ch == 1 or shifts[:, 0].max() > 0) and shifts[:, 1].max() > 0
    got, want = R.masks(bits, shifts, Hm, Wm), R.masks_interpolate(bits, shifts, Hm, Wm)
    assert got.dtype == np.float32 and got.shape == want.shape == (64, Hm, Wm)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"restatement against F.interpolate + crop, {shape}: {worst:.2e}")
    assert worst <= BOUND
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float(got.max()) - float(got.min()) > 0.9
    ones, zeros = R.masks(np.ones_like(bits), shifts, Hm, Wm), R.masks(np.zeros_like(bits), shifts, Hm, Wm)
    assert np.array_equal(ones, np.ones_like(ones)) and np.array_equal(zeros, np.zeros_like(zeros))


def test_draw_is_reproducible_and_masks_argument_repeats_it():
    a, b, c = R.draw(50, 8, 8, 64, 128, 0.5, 3), R.draw(50, 8, 8, 64, 128, 0.5, 3), R.draw(50, 8, 8, 64, 128, 0.5, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    assert a[0].dtype == np.uint8 and a[0].shape == (50, 8, 8) and a[1].dtype == np.int32 and a[1].shape == (50, 2)
    assert abs(float(a[0].mean()) - 0.5) < 0.05 and set(np.unique(a[0])) == {0, 1}
    assert float(R.draw(400, 8, 8, 64, 128, 0.25, 0)[0].mean()) < 0.3 and R.draw(9, 8, 8, 64, 128, 1.0, 0)[0].all()
    # the package draws the same set from the same seed, and takes it back through masks=
    from brainxai import explain as X
    geom = X._rise_geometry("rise", 8, 64, 128)
    assert geom == (8, 8, 8, 16) and X._rise_geometry("rise", 8, 1, 2000) == (1, 8, 1, 250) and X._rise_geometry("rise", (4, 16), 19, 2000) == (4, 16, 5, 125)
    mine = X._rise_mask_set("rise", 50, geom, 0.5, 3, None)
    assert np.array_equal(mine[0], a[0]) and np.array_equal(mine[1], a[1]) and mine[0].dtype == np.uint8 and mine[1].dtype == np.int32
    again = X._rise_mask_set("rise", 4000, geom, 0.5, 99, (torch.from_numpy(a[0]), a[1].astype(np.int64)))
    assert np.array_equal(again[0], a[0]) and np.array_equal(again[1], a[1]) and again[1].dtype == np.int32


def test_perturbed_and_saliency_restatements():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6) + 1
    one, zero = np.ones((4, 6), dtype=np.float32), np.zeros((4, 6), dtype=np.float32)
    assert torch.equal(R.perturbed(x, one, 0.0), x) and torch.equal(R.perturbed(x, zero, 0.25), torch.full_like(x, 0.25))
    assert bool((R.perturbed(x, zero, [7.0, 8.0, 9.0])[:, 1] == 8.0).all())
    e = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(2, 1, 5, 6)
    col = np.array([[1, 0, 1, 0, 0.5, 1]], dtype=np.float32)
    got = R.perturbed(e, col, 0.0)
    assert torch.equal(got[:, :, :, 1], torch.zeros(2, 1, 5)) and torch.equal(got[:, :, :, 4], e[:, :, :, 4] * 0.5) and torch.equal(got[:, :, :, 5], e[:, :, :, 5])
    # the planted case: P[n] = m_n(p*) puts the maximum of the map at p*
    bits, shifts = R.draw(200, 4, 4, 16, 24, 0.5, 5)
    m = R.masks(bits, shifts, 16, 24)
    P = m[:, 5, 7].astype(np.float64).reshape(1, -1, 1)
    sal = R.saliency(P, m, 0.5, "expected")[0, 0]
    assert np.unravel_index(int(sal.argmax()), sal.shape) == (5, 7)
    assert np.allclose(R.saliency(np.ones((1, 200, 1)), m, 0.5, "coverage"), 1.0, rtol=0, atol=1e-12)
