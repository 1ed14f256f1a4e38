"""CPU: the definition behind brainxai.spectral_gradients / spectral_occlusion.  The closed form of tests/spectral_ref.py against a literal
transcription of braindecode's compute_amplitude_gradients (rfft -> amplitudes and phases -> irfft -> model -> autograd by the
amplitudes) on the oracle's EEGNet in fp64; Parseval per electrode; the band bins at their edges; the twiddle table; every refusal of the
drivers with the library unloadable, and of the entry points given null pointers; and, on the reference alone, that the end-to-end GPU
cases tell the definition from its three likeliest mistakes."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from oracle import ref_torch as O
from tests import spectral_ref as R
from tests.test_gpu_spectral import E2E_BOUND

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


# ---- braindecode's loop, transcribed ------------------------------------------------------------------------------------------------------
def _transcription(model64, x):
    """fp64 [B, K, Chans, F]: d out[:, c] / d amplitudes, by autograd through irfft(amps * exp(i phases))."""
    X = np.fft.rfft(x.double().numpy(), axis=-1)
    amps = torch.tensor(np.abs(X), requires_grad=True)
    phases = torch.tensor(np.angle(X))
    rows = torch.fft.irfft(amps * torch.exp(1j * phases), n=x.shape[-1], dim=-1)
    out = model64(rows)
    return torch.stack([torch.autograd.grad(out[:, c].sum(), amps, retain_graph=True)[0][:, 0] for c in range(out.shape[1])], 1).numpy(), np.abs(X)


@pytest.mark.parametrize("Chans,T", [(5, 512), (19, 2000)])
def test_closed_form_is_autograd_by_the_amplitudes(Chans, T):
    model64 = copy.deepcopy(O.fill_params(O.EEGNet(6, Chans=Chans, Samples=T, dropoutRate=0.0), seed=33).eval()).double()
    x = O.seeded((2, 1, Chans, T), 92, "randn")
    x[1, 0, 0] = 0.0                                                        # a zero row: u = 1
    want, A = _transcription(model64, x)
    grad = R.path_gradient(model64, x, 1).numpy()
    got = R.oracle_map(x.numpy(), grad, "amplitude_gradient")
    err = float((R.pair_max(got - want) / R.pair_max(want)).max())
    print(f"{Chans} x {T}: closed form against autograd by the amplitudes {err:.2e} of each (sample, class) maximum")
    assert err <= 1e-12
    gxa = R.oracle_map(x.numpy(), grad, "gradient_x_amplitude")
    assert float((R.pair_max(gxa - A[:, None, 0] * want) / R.pair_max(gxa)).max()) <= 1e-12, "gradient x amplitude is A times the amplitude gradient"


@pytest.mark.parametrize("T", [1, 2, 3, 7, 64, 125, 2000])
def test_parseval_per_electrode(T):
    x, g = O.seeded((3, 4, T), 5, "randn").numpy(), O.seeded((3, 4, T), 6, "randn").numpy()
    x[0, 0] = 0.0
    total = R.maps(x, g, "gradient_x_amplitude").sum(-1)
    want = (x.astype(np.float64) * g).sum(-1)
    assert np.abs(total - want).max() <= 1e-13 * np.abs(x.astype(np.float64) * g).sum(-1).max()


# ---- bands and the table ----------------------------------------------------------------------------------------------------------------
def test_band_bins_at_the_edges():
    bins = brainxai.spectral_band_bins
    assert bins("clinical", 2000, 40.0) == [(25, 200), (200, 400), (400, 650), (650, 1001)]        # 0.02 Hz a bin; beta is cut at Nyquist (20 Hz)
    assert bins("clinical", 3000, 200.0) == [(8, 60), (60, 120), (120, 195), (195, 450)]           # 1/15 Hz a bin: 0.5 Hz falls between bins 7 and 8
    assert bins([(4.0, 8.0)], 2000, 40.0) == [(200, 400)]                   # an edge exactly on a bin belongs to the band it opens
    assert bins([(25.0, 30.0)], 2000, 40.0) == [(1001, 1001)]               # beyond Nyquist: no bin
    assert bins([(0.0101, 0.0199)], 2000, 40.0) == [(1, 1)]                 # between two bins: empty
    assert bins([(3.0, 3.0)], 2000, 40.0) == [(150, 150)]                   # lo == hi: empty
    assert bins([(0.0, 0.5), (0.0, 0.51)], 7) == [(0, 4), (0, 4)]           # odd T, cycles per sample: F = 4, no Nyquist bin
    assert bins([(0.0, 1.0), (0.5, 1.0)], 1) == [(0, 1), (1, 1)]            # T = 1: the mean alone
    assert bins([(0.0, 0.5), (0.5, 0.6), (0.0, 0.6)], 2) == [(0, 1), (1, 2), (0, 2)]               # T = 2: the mean and Nyquist
    for T, fs, bands in [(2000, 40.0, "clinical"), (3000, 200.0, "clinical"), (7, None, [(0.0, 0.3), (0.3, 0.5), (0.1, 0.1)]), (125, 33.3, [(0.1, 7.77), (7.77, 16.65)]),
                         (2, None, [(0.0, 1.0)]), (1, 5.0, [(0.0, 1.0), (1.0, 2.0)])]:
        assert bins(bands, T, fs) == R.band_bins(bands, T, fs), (T, fs, bands)
    assert list(brainxai.CLINICAL_BANDS.values()) == R.CLINICAL


@pytest.mark.parametrize("T", [1, 2, 3, 4, 7, 8, 64, 125, 333, 2000, 3000, 8192])
def test_twiddle_table(T):
    tw = brainxai.spectral_twiddles(T)
    assert tw.shape == (T, 2) and tw.dtype == np.float64 and tw.flags.c_contiguous
    j = np.arange(T)
    exact = np.stack([np.cos(2 * np.pi * j / T), np.sin(2 * np.pi * j / T)], 1)
    assert np.abs(tw - exact).max() <= 17 * 2.0 ** -53                      # the plain formula's own error: 2.5 u on an angle of up to 2 pi, and a rounding
    assert np.abs(tw[:, 0] ** 2 + tw[:, 1] ** 2 - 1).max() <= 4 * 2.0 ** -53
    if T % 4 == 0:                                                          # quarter turns are exact
        assert tw[[0, T // 4, T // 2, 3 * T // 4]].tolist() == [[1, 0], [0, 1], [-1, 0], [0, -1]]
    x = O.seeded((T,), 3, "randn").double().numpy()                         # the direct sum over the table is numpy's rfft
    idx = np.outer(np.arange(T // 2 + 1), j) % T
    X = (x * tw[idx, 0]).sum(1) - 1j * (x * tw[idx, 1]).sum(1)
    assert np.abs(X - np.fft.rfft(x)).max() <= (T + 4) * 2.0 ** -53 * np.abs(x).sum()


# ---- discrimination, on the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", R.E2E_STEPS)
@pytest.mark.parametrize("kind", R.E2E_KINDS)
def test_end_to_end_cases_discriminate(kind, steps):
    for map_kind in R.MAP_KINDS:
        moved = R.movements(kind, steps, map_kind)
        print(f"{kind} steps {steps} {map_kind}: the reference moves by (least over (sample, class), of its maximum) {moved}")
        for how, v in moved.items():
            assert v > 100 * E2E_BOUND, f"{kind} steps {steps} {map_kind}: {how} moves the reference by only {v:.3e}"


# ---- refusals of the drivers ------------------------------------------------------------------------------------------------------------
B, CH, T = 2, 19, 2000


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, 4, 16, 24, generator=g)


def _model(kind):
    if kind == "multimodal":
        return brainxai.build_multimodal(CH, T, 4)
    if kind == "spectrogram":
        return brainxai.Spectrogram_Model(6, in_channels=4)
    if kind == "eegnet33":
        return brainxai.EEGNet(33, Chans=CH, Samples=T)
    return brainxai.EEGNet(6, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(6, Chans=CH, Samples=T)


BAD_GRADIENTS = {
    "kind_unknown": ("multimodal", dict(kind="phase_gradient"), ValueError, "unknown kind 'phase_gradient'"),
    "kind_number": ("eegnet", dict(kind=1), ValueError, "unknown kind 1"),
    "steps_zero": ("multimodal", dict(steps=0), ValueError, "steps = 0 < 1"),
    "steps_negative": ("eegnet", dict(steps=-3), ValueError, "steps = -3 < 1"),
    "steps_float": ("multimodal", dict(steps=2.5), ValueError, "steps must be an int"),
    "steps_bool": ("deep", dict(steps=True), ValueError, "steps must be an int"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "eeg_none": ("multimodal", dict(eeg=None), ValueError, "tensor is None"),
    "eeg_three_dims": ("eegnet", dict(eeg=torch.zeros(2, CH, T)), ValueError, r"must be a tensor \[B,1,Chans,T\]"),
    "eeg_is_a_spectrogram": ("multimodal", dict(eeg=torch.zeros(2, 4, 16, 24)), ValueError, r"must be a tensor \[B,1,Chans,T\]"),
    "eeg_empty": ("eegnet", dict(eeg=torch.zeros(0, 1, CH, T)), ValueError, "empty input"),
    "T_beyond": ("eegnet", dict(eeg=torch.zeros(1, 1, 1, 1).expand(2, 1, CH, 8193)), ValueError, "T = 8193, supported 1..8192"),
    "model_spectrogram": ("spectrogram", dict(), ValueError, "needs a MultimodalModel, an EEGNet"),
    "multimodal_without_spec": ("multimodal", dict(spec=None), ValueError, "needs both inputs"),
    "classes_above_32": ("eegnet33", dict(), ValueError, "33 classes"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("eegnet", dict(class_idx=[0, 1, 2]), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "fs_zero": ("multimodal", dict(fs=0.0), ValueError, "fs must be a finite number > 0"),
    "fs_nan": ("eegnet", dict(fs=float("nan")), ValueError, "fs must be a finite number > 0"),
    "fs_word": ("eegnet", dict(fs="40"), ValueError, "fs must be a finite number > 0"),
    "bands_clinical_without_fs": ("multimodal", dict(bands="clinical"), ValueError, "need fs"),
    "bands_word": ("multimodal", dict(bands="gamma", fs=40.0), ValueError, "unknown bands 'gamma'"),
    "bands_inverted": ("eegnet", dict(bands=[(8.0, 4.0)], fs=40.0), ValueError, "negative or inverted"),
    "bands_negative": ("eegnet", dict(bands=[(-1.0, 4.0)], fs=40.0), ValueError, "negative or inverted"),
    "bands_nan": ("eegnet", dict(bands=[(0.0, float("nan"))]), ValueError, "finite numbers"),
    "bands_not_pairs": ("eegnet", dict(bands=[1.0, 2.0]), ValueError, "sequence of"),
    "bands_empty": ("eegnet", dict(bands=[]), ValueError, "no bands"),
    "offsets": ("eegnet", dict(eeg=torch.zeros(1, 1, 1, 1).expand(1 << 14, 1, CH, T), class_idx="all"), ValueError, "32-bit offsets"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_eegnet_all": ("eegnet", dict(class_idx="all", steps=5, kind="gradient_x_amplitude", bands="clinical", fs=40.0, return_parts=True), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(class_idx=torch.tensor([5, 0]), max_batch=3), RuntimeError, "no CPU path"),
}
BAD_OCCLUSION = {
    "cells_unknown": ("multimodal", dict(cells="electrode"), ValueError, "unknown cells 'electrode'"),
    "cells_number": ("eegnet", dict(cells=0), ValueError, "unknown cells 0"),
    "score_unknown": ("multimodal", dict(score="logit"), ValueError, "unknown score 'logit'"),
    "max_batch": ("eegnet", dict(max_batch=-1), ValueError, "max_batch = -1"),
    "eeg_three_dims": ("eegnet", dict(eeg=torch.zeros(2, CH, T)), ValueError, r"must be a tensor \[B,1,Chans,T\]"),
    "T_beyond": ("eegnet", dict(eeg=torch.zeros(1, 1, 1, 1).expand(2, 1, CH, 9000)), ValueError, "T = 9000, supported 1..8192"),
    "model_spectrogram": ("spectrogram", dict(), ValueError, "needs a MultimodalModel, an EEGNet"),
    "classes_above_32": ("eegnet33", dict(), ValueError, "33 classes"),
    "class_high": ("deep", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "bands_clinical_without_fs": ("multimodal", dict(bands="clinical", fs=None), ValueError, "need fs"),
    "bands_inverted": ("eegnet", dict(bands=[(0.0, 4.0), (13.0, 8.0)]), ValueError, "negative or inverted"),
    "bands_negative": ("multimodal", dict(bands=[(-0.5, 4.0)]), ValueError, "negative or inverted"),
    "bands_none": ("eegnet", dict(bands=None), ValueError, "sequence of"),
    "fs_negative": ("eegnet", dict(fs=-40.0), ValueError, "fs must be a finite number > 0"),
    "offsets": ("eegnet", dict(eeg=torch.zeros(1, 1, 1, 1).expand(1 << 15, 1, CH, T), bands=[(0.0, 1.0)] * 2048, cells="electrode_band"), ValueError, "32-bit offsets"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(cells="electrode_band", class_idx="all", score="logprob", return_parts=True), RuntimeError, "no CPU path"),
}


def _refused(monkeypatch, fn, table, case, defaults):
    reached = _recorder(monkeypatch)
    kind, kw, exc, match = table[case]
    eeg, spec = _inputs()
    args = dict(eeg=eeg, spec=spec if kind == "multimodal" else None, **defaults)
    args.update(kw)
    eeg, spec = args.pop("eeg"), args.pop("spec")
    with pytest.raises(exc, match=match):
        fn(_model(kind), eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


@pytest.mark.parametrize("case", sorted(BAD_GRADIENTS))
def test_spectral_gradients_refuses_before_launch(monkeypatch, case):
    _refused(monkeypatch, brainxai.spectral_gradients, BAD_GRADIENTS, case, {})


@pytest.mark.parametrize("case", sorted(BAD_OCCLUSION))
def test_spectral_occlusion_refuses_before_launch(monkeypatch, case):
    _refused(monkeypatch, brainxai.spectral_occlusion, BAD_OCCLUSION, case, dict(bands="clinical", fs=40.0))


def test_helpers_refuse_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    for bad in (5, torch.zeros(7), torch.zeros(2, 3, 4, 5), torch.zeros(2, 2, 3, 4, 5)):
        with pytest.raises(ValueError, match="eeg_spectrum: x must be a tensor"):
            brainxai.eeg_spectrum(bad)
    with pytest.raises(ValueError, match="eeg_spectrum: empty input"):
        brainxai.eeg_spectrum(torch.zeros(0, 3, 8))
    with pytest.raises(ValueError, match="T = 8193"):
        brainxai.eeg_spectrum(torch.zeros(1, 1, 1).expand(2, 3, 8193))
    with pytest.raises(ValueError, match="fs must be"):
        brainxai.eeg_spectrum(torch.zeros(2, 3, 8), fs=0)
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.eeg_spectrum(torch.zeros(1, 1, 1).expand(1 << 10, 1 << 9, 8192))
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.eeg_spectrum(torch.zeros(2, 1, 3, 8), fs=40.0)
    m = torch.zeros(2, 3, 5)
    with pytest.raises(ValueError, match="T must be an int"):
        brainxai.band_sums(m, [(0.0, 0.5)], T=0)
    with pytest.raises(ValueError, match=r"F = T // 2 \+ 1 = 6"):
        brainxai.band_sums(m, [(0.0, 0.5)], T=10)
    with pytest.raises(ValueError, match="map must be a tensor"):
        brainxai.band_sums([1.0] * 5, [(0.0, 0.5)], T=8)
    with pytest.raises(ValueError, match="need fs"):
        brainxai.band_sums(m, "clinical", T=8)
    with pytest.raises(ValueError, match="negative or inverted"):
        brainxai.band_sums(m, [(0.3, 0.1)], T=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.band_sums(m, [(0.0, 0.5)], T=8)
    assert reached == []


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def dft(Rn=6, Tn=100):
        return lib.bx_rdft_rows(None, None, None, None, Rn, Tn, None)
    for kw, word in [(dict(Rn=0), b"bad shape"), (dict(Tn=0), b"bad shape"), (dict(Rn=1 << 19, Tn=1 << 12), b"32-bit"), (dict(), b"null pointer"),
                     (dict(Tn=8192), b"null pointer")]:
        rc = dft(**kw)
        assert rc == BX_EINVAL and b"bx_rdft_rows" in msg() and word in msg(), (kw, rc, msg())
    assert dft(Tn=8193) == BX_EUNSUPPORTED and b"T = 8193, supported 1..8192" in msg()

    def acc(Bn=3, n=4, per=100, row0=0, rows=12, Kc=6, slot=0):
        return lib.bx_spectral_accumulate(None, None, None, Bn, n, per, Kc, slot, row0, rows, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(row0=-1), b"rows row0"), (dict(rows=0), b"rows row0"),
                     (dict(row0=10, rows=3), b"rows row0"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"), (dict(Bn=1 << 11, per=1 << 20, rows=1), b"32-bit"),
                     (dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per"), (dict(Kc=0), b"class slot"), (dict(slot=6), b"class slot"),
                     (dict(slot=-1), b"class slot"), (dict(Bn=1 << 10, per=1 << 18, Kc=32, rows=1), b"B * Kc * per"), (dict(), b"null pointer")]:
        rc = acc(**kw)
        assert rc == BX_EINVAL and b"bx_spectral_accumulate" in msg() and word in msg(), (kw, rc, msg())
    assert acc(Kc=33) == BX_EUNSUPPORTED and b"33 classes" in msg()

    def val(Bn=2, Kc=6, Chans=19, Tn=2000, kind=0):
        return lib.bx_spectral_values(None, None, None, None, None, Bn, Kc, Chans, Tn, kind, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(Kc=0), b"bad shape"), (dict(Chans=0), b"bad shape"), (dict(Tn=0), b"bad shape"), (dict(kind=2), b"unknown kind"),
                     (dict(kind=-1), b"unknown kind"), (dict(Bn=1 << 10, Chans=1 << 8, Tn=1 << 12), b"32-bit"), (dict(), b"null pointer")]:
        rc = val(**kw)
        assert rc == BX_EINVAL and b"bx_spectral_values" in msg() and word in msg(), (kw, rc, msg())
    assert val(Kc=33) == BX_EUNSUPPORTED and b"33 classes" in msg()
    assert val(Tn=10000) == BX_EUNSUPPORTED and b"T = 10000" in msg()

    def band(Rn=10, Fn=100, nb=4):
        return lib.bx_band_sum(None, None, None, Rn, Fn, nb, None)
    for kw, word in [(dict(Rn=0), b"bad shape"), (dict(Fn=0), b"bad shape"), (dict(nb=0), b"bad shape"), (dict(Rn=1 << 20, Fn=1 << 11), b"32-bit"),
                     (dict(Rn=1 << 20, nb=1 << 11), b"32-bit"), (dict(), b"null pointer")]:
        rc = band(**kw)
        assert rc == BX_EINVAL and b"bx_band_sum" in msg() and word in msg(), (kw, rc, msg())

    def stop(Bn=2, Chans=19, Tn=2000, nb=4, cells=0, n0=0, n=4):
        return lib.bx_bandstop_rows(None, None, None, None, None, None, Bn, Chans, Tn, nb, cells, n0, n, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(Chans=0), b"bad shape"), (dict(nb=0), b"bad shape"), (dict(Tn=0), b"bad shape"), (dict(cells=2), b"unknown cells"),
                     (dict(n0=-1), b"rows n0"), (dict(n=0), b"rows n0"), (dict(n0=3, n=2), b"rows n0"), (dict(cells=1, n0=70, n=7), b"rows n0"),
                     (dict(Bn=1 << 6, nb=1 << 10, n=1 << 10), b"32-bit"), (dict(), b"null pointer"), (dict(cells=1, n0=70, n=6), b"null pointer")]:
        rc = stop(**kw)
        assert rc == BX_EINVAL and b"bx_bandstop_rows" in msg() and word in msg(), (kw, rc, msg())
    assert stop(Tn=8193) == BX_EUNSUPPORTED and b"T = 8193" in msg()


def test_header_symbols_are_bound():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brainxai.h")).read()
    names = ["bx_rdft_rows", "bx_spectral_accumulate", "bx_spectral_values", "bx_band_sum", "bx_bandstop_rows"]
    lib = _lib.load()
    for name in names:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/brainxai.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, f"{name}: the ctypes signature does not match the header"
        assert hasattr(lib, name)
    assert (_lib.BX_SPECTRAL_MAX_T, _lib.BX_SPECTRAL_AMPLITUDE_GRADIENT, _lib.BX_SPECTRAL_GRADIENT_X_AMPLITUDE) == (8192, 0, 1)
    assert re.search(r"#define BX_SPECTRAL_MAX_T 8192\b", header)
