"""CPU: brainxai.smooth_grad / smooth_grad_noise argument checks that run before anything reaches a device, the limits of the
bx_smoothgrad_* entry points, and the restatement of the definition (tests/smooth_grad_ref.py): Philox4x32-10 against the Random123
known answers, the statistics of the restatement's noise, and the three estimators against the closed form of a quadratic model."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import smooth_grad_ref as R

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


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox(tuple(np.uint64(c) for c in counter), key)
    assert got.dtype == np.uint32 and tuple(int(v) for v in got.reshape(4)) == want
    both = R.philox((np.array([counter[0], 0], dtype=np.uint64), np.array([counter[1], 0], dtype=np.uint64), np.array([counter[2], 0], dtype=np.uint64),
                     np.array([counter[3], 0], dtype=np.uint64)), key)                     # vectorised over counters
    assert tuple(int(v) for v in both[:, 0]) == want


# ---- the restatement's noise ----------------------------------------------------------------------------------------------------------
def test_restatement_noise_statistics_and_prefix():
    B, n, per = 2, 6, 38000
    z, r = R.noise(B, n, per, 0, with_r=True)
    assert z.shape == r.shape == (B, n, per) and np.isfinite(z).all() and (np.abs(z) <= r).all()
    N = z.size
    mean, std = float(z.mean()), float(z.std())
    flat = z.reshape(B * n, per)
    row_corr = max(abs(float(np.corrcoef(flat[i], flat[i + 1])[0, 1])) for i in range(B * n - 1))
    lag1 = abs(float(np.corrcoef(z[..., :-1].ravel(), z[..., 1:].ravel())[0, 1]))
    print(f"restatement noise {B}x{n}x{per}: mean {mean:.4f}, std {std:.4f}, row-to-row correlation {row_corr:.2e}, lag-1 correlation {lag1:.2e}")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(std - 1) <= 5 / np.sqrt(2 * N)
    assert row_corr <= 5 / np.sqrt(per)
    assert lag1 <= 5 / np.sqrt(N)
    assert np.array_equal(R.noise(B, 3, per, 0), z[:, :3]), "a longer run must extend a shorter one"
    assert np.array_equal(R.noise(1, n, per, 0), z[:1])
    assert np.array_equal(R.noise(B, n, 1665, 0), z[:, :, :1665]), "an element's draw does not depend on the row length"
    assert not np.array_equal(R.noise(B, n, per, 1), z)
    assert not np.array_equal(R.noise(B, n, 64, 1 << 32), z[:, :, :64]), "the high word of the seed is the second key word"


# ---- the restatement against a closed form --------------------------------------------------------------------------------------------
class _Quadratic(torch.nn.Module):
    """F_c(x) = a_c / 2 * sum x^2: the gradient is a_c * x."""

    def __init__(self, a):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(a, dtype=torch.float64))

    def forward(self, x):
        return 0.5 * self.a[None] * (x * x).flatten(1).sum(1, keepdim=True)


def test_restatement_equals_the_closed_form_of_a_quadratic_model():
    B, n, shape = 2, 7, (3, 4, 5)
    a = [0.5, -1.25, 2.0]
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((B, *shape)).astype(np.float32))
    z32 = R.noise(B, n, 60, 5).astype(np.float32).reshape(B, n, *shape)
    sig = R.sigma(x, 0.15)
    assert sig.dtype == np.float32 and sig.shape == (B,) and (sig > 0).all()
    mean, sq, var = (t.numpy() for t in R.values(_Quadratic(a), x, z32, sig))
    assert mean.shape == sq.shape == var.shape == (B, 3, *shape)
    x64, z64, s64 = x.double().numpy(), z32.astype(np.float64), sig.astype(np.float64)[:, None, None, None]
    av = np.array(a)[None, :, None, None, None]
    want_mean = av * (x64 + s64 * z64.mean(1))[:, None]
    want_var = av ** 2 * (s64 ** 2 * z64.var(1))[:, None]
    want_sq = want_var + want_mean ** 2
    # a row is x + sigma z within two fp32 roundings, 2^-23 of the largest row; a gradient a * row within 2^-23 M, M the largest
    # gradient; its square within 2 * 2^-23 M^2, and the variance sees that in both of its terms
    r64 = R.rows(x, sig, z32).astype(np.float64)
    M = np.abs(av).max() * np.abs(r64).max()
    for got, want, bound, name in ((mean, want_mean, 2.0 ** -23 * M, "mean"), (sq, want_sq, 2.0 ** -22 * M * M, "mean square"),
                                   (var, want_var, 2.0 ** -21 * M * M, "variance")):
        err = float(np.abs(got - want).max())
        print(f"closed form, {name}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, name
    # accumulate / finish on those gradients give the same values, split inside a sample or not, and the map is the channel maximum
    for c, ac in enumerate(a):
        g = (ac * r64).astype(np.float32)
        S1, S2, _ = R.accumulate(g[:9], B, n)
        S1, S2, _ = R.accumulate(g[9:], B, n, S1, S2, row0=9)
        one = R.accumulate(g, B, n)
        assert np.array_equal(S1, one[0]) and np.array_equal(S2, one[1])
        for kind, want in (("smoothgrad", mean), ("smoothgrad_sq", sq), ("vargrad", var)):
            vals, amap = R.finish(S1, S2, n, kind, shape)
            assert vals.dtype == np.float32 and vals.shape == (B, 1, *shape) and amap.shape == (B, 1, 4, 5)
            assert np.abs(vals[:, 0] - want[:, c]).max() <= 2.0 ** -20 * np.abs(want[:, c]).max()
            assert np.array_equal(amap, np.abs(vals).max(2))


def test_sigma_and_rows_restatement():
    x = np.array([[[1.0, -0.0, 3.5]], [[2.0, 2.0, 2.0]], [[0.0, -0.0, 0.0]]], dtype=np.float32)
    sig = R.sigma(x, 0.5)
    assert np.array_equal(sig, np.array([1.75, 0.0, 0.0], dtype=np.float32)) and not np.signbit(sig).any()
    z32 = R.noise(3, 2, 3, 9).astype(np.float32).reshape(3, 2, 1, 3)
    r = R.rows(x, sig, z32).reshape(3, 2, 1, 3)
    assert r.dtype == np.float32
    assert np.array_equal(r[1], np.broadcast_to(x[1], (2, 1, 3))), "sigma = 0 gives the sample itself"
    assert np.array_equal(r[0], (x[0][None] + (np.float32(1.75) * z32[0]).astype(np.float32)).astype(np.float32))


# ---- refusals of the drivers ------------------------------------------------------------------------------------------------------------
B, C, H, W, CH, T = 2, 4, 16, 24, 19, 2000


def _inputs():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 1, CH, T, generator=g), torch.rand(B, C, H, W, generator=g)


# name -> (model kind, keyword overrides, exception, message); the spectrogram is 4 x 16 x 24, the EEG input 19 x 2000
BAD = {
    "input_unknown": ("multimodal", dict(input="both"), ValueError, "smooth_grad: unknown input"),
    "input_none_eeg": ("spectrogram", dict(input="eeg"), ValueError, "tensor is None"),
    "input_none_spec": ("eegnet", dict(input="spec"), ValueError, "tensor is None"),
    "model_spec_for_eeg": ("spectrogram_with_eeg", dict(input="eeg"), ValueError, "needs a MultimodalModel, an EEGNet"),
    "kind_unknown": ("multimodal", dict(kind="smooth"), ValueError, "unknown kind 'smooth'"),
    "kind_none": ("multimodal", dict(kind=None), ValueError, "unknown kind None"),
    "kind_number": ("eegnet", dict(input="eeg", kind=2), ValueError, "unknown kind 2"),
    "both_scales": ("multimodal", dict(noise_level=0.1, stdev=0.2), ValueError, "noise_level or stdev, not both"),
    "both_scales_tensor": ("multimodal", dict(noise_level=0.1, stdev=torch.ones(B)), ValueError, "noise_level or stdev, not both"),
    "level_negative": ("multimodal", dict(noise_level=-0.1), ValueError, "noise_level must be a finite number >= 0"),
    "level_nan": ("multimodal", dict(noise_level=float("nan")), ValueError, "noise_level must be a finite number >= 0"),
    "level_inf": ("eegnet", dict(input="eeg", noise_level=float("inf")), ValueError, "noise_level must be a finite number >= 0"),
    "level_beyond_fp32": ("eegnet", dict(input="eeg", noise_level=1e39), ValueError, "beyond fp32"),
    "level_word": ("multimodal", dict(noise_level="0.1"), ValueError, "noise_level must be a finite number >= 0"),
    "stdev_negative": ("multimodal", dict(stdev=-1.0), ValueError, "stdev must be finite and >= 0"),
    "stdev_nan": ("multimodal", dict(stdev=float("nan")), ValueError, "stdev must be finite and >= 0"),
    "stdev_tensor_negative": ("multimodal", dict(stdev=torch.tensor([0.1, -0.1])), ValueError, "stdev must be finite and >= 0"),
    "stdev_tensor_inf": ("deep", dict(input="eeg", stdev=torch.tensor([0.1, float("inf")])), ValueError, "stdev must be finite and >= 0"),
    "stdev_beyond_fp32": ("multimodal", dict(stdev=1e39), ValueError, "stdev must be finite and >= 0"),
    "stdev_tensor_shape": ("multimodal", dict(stdev=torch.ones(3)), ValueError, r"stdev of shape \(3,\)"),
    "stdev_list": ("multimodal", dict(stdev=[0.1, 0.2]), ValueError, "stdev must be a number or a tensor"),
    "max_batch": ("multimodal", dict(max_batch=0), ValueError, "max_batch = 0"),
    "nsamples_zero": ("multimodal", dict(nsamples=0), ValueError, "nsamples = 0 < 1"),
    "nsamples_negative": ("eegnet", dict(input="eeg", nsamples=-3), ValueError, "nsamples = -3 < 1"),
    "nsamples_float": ("eegnet", dict(input="eeg", nsamples=2.5), ValueError, "nsamples must be an int"),
    "nsamples_bool": ("eegnet", dict(input="eeg", nsamples=True), ValueError, "nsamples must be an int"),
    "seed_negative": ("multimodal", dict(seed=-1), ValueError, "seed must be an int in"),
    "seed_wide": ("multimodal", dict(seed=1 << 64), ValueError, "seed must be an int in"),
    "seed_float": ("multimodal", dict(seed=1.0), ValueError, "seed must be an int in"),
    "class_high": ("multimodal", dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("deep", dict(input="eeg", class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "classes_above_32": ("spectrogram33", dict(), ValueError, "33 classes"),
    "cpu_multimodal": ("multimodal", dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg_all": ("multimodal", dict(input="eeg", class_idx="all", kind="vargrad"), RuntimeError, "no CPU path"),
    "cpu_multimodal_stdev": ("multimodal", dict(stdev=torch.tensor([0.1, 0.0]), class_idx=[1, 2], kind="smoothgrad_sq"), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", dict(class_idx=3, return_parts=True, seed=(1 << 64) - 1), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", dict(input="eeg", class_idx="all", seed=7, noise_level=0), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", dict(input="eeg", class_idx=torch.tensor([5, 0]), max_batch=3, stdev=0.5), RuntimeError, "no CPU path"),
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
    args = dict(nsamples=5)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.smooth_grad(model, eeg, spec, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_offset_limits_raise_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    model = brainxai.Spectrogram_Model(32, in_channels=1)
    one = torch.zeros(1, 1, 1, 1)
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * Kc * per: 32 * 128 * 10^6 values (a view)
        brainxai.smooth_grad(model, None, one.expand(128, 1, 1000, 1000), nsamples=1, class_idx="all")
    with pytest.raises(ValueError, match="32-bit offsets"):               # B * n
        brainxai.smooth_grad(model, None, one.expand(1 << 16, 1, 2, 2), nsamples=1 << 15)
    with pytest.raises(ValueError, match="65535"):                        # B * Kc planes
        brainxai.smooth_grad(model, None, one.expand(4096, 1, 2, 2), nsamples=1, class_idx="all")
    assert reached == []


def test_noise_helper_refuses_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    for shape in (5, (4,), (2, 0, 3), "ab", (2, None)):
        with pytest.raises(ValueError, match="smooth_grad_noise: shape"):
            brainxai.smooth_grad_noise(shape, nsamples=2)
    with pytest.raises(ValueError, match="nsamples = 0 < 1"):
        brainxai.smooth_grad_noise((2, 3), nsamples=0)
    with pytest.raises(ValueError, match="nsamples must be an int"):
        brainxai.smooth_grad_noise((2, 3), nsamples=1.5)
    with pytest.raises(ValueError, match="seed must be an int in"):
        brainxai.smooth_grad_noise((2, 3), nsamples=2, seed=-5)
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.smooth_grad_noise((1 << 16, 2), nsamples=1 << 15)
    with pytest.raises(ValueError, match="32-bit offsets"):
        brainxai.smooth_grad_noise((1 << 11, 1 << 10, 1 << 10), nsamples=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        brainxai.smooth_grad_noise((2, 3), nsamples=2, device="cpu")
    assert reached == []


# ---- refusals of the entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    row_cases = [(dict(Bn=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(row0=-1), b"rows row0"),
                 (dict(rows=0), b"rows row0"), (dict(row0=10, rows=3), b"rows row0"), (dict(Bn=1 << 16, n=1 << 15), b"32-bit"),
                 (dict(Bn=1 << 11, per=1 << 20, rows=1), b"32-bit"), (dict(Bn=1000, n=1000, per=1 << 12, rows=1 << 19), b"rows * per"),
                 (dict(), b"null pointer"), (dict(row0=11, rows=1), b"null pointer")]

    def rows(Bn=3, n=4, per=100, row0=0, rows=12, seed=(1 << 64) - 1):
        return lib.bx_smoothgrad_rows(None, None, None, Bn, n, per, seed, row0, rows, None)
    for kw, word in row_cases:
        rc = rows(**kw)
        assert rc == BX_EINVAL and b"bx_smoothgrad_rows" in msg() and word in msg(), (kw, rc, msg())

    def acc(Bn=3, n=4, per=100, row0=0, rows=12, Kc=6, slot=0):
        return lib.bx_smoothgrad_accumulate(None, None, None, Bn, n, per, Kc, slot, row0, rows, None)
    for kw, word in row_cases + [(dict(Kc=0), b"class slot"), (dict(slot=6), b"class slot"), (dict(slot=-1), b"class slot"),
                                 (dict(Bn=1 << 10, per=1 << 18, Kc=32, rows=1), b"B * Kc * per")]:
        rc = acc(**kw)
        assert rc == BX_EINVAL and b"bx_smoothgrad_accumulate" in msg() and word in msg(), (kw, rc, msg())
    assert acc(Kc=33) == BX_EUNSUPPORTED and b"33 classes" in msg()

    def fin(BK=12, Cc=4, HW=100, n=5, kind=0):
        return lib.bx_smoothgrad_finish(None, None, None, None, BK, Cc, HW, n, kind, None)
    for kw, word in [(dict(BK=0), b"bad shape"), (dict(Cc=0), b"bad shape"), (dict(HW=0), b"bad shape"), (dict(n=0), b"bad shape"), (dict(kind=3), b"unknown kind"),
                     (dict(kind=-1), b"unknown kind"), (dict(BK=1 << 12, HW=1 << 18), b"32-bit"), (dict(BK=65536, Cc=1, HW=1), b"planes"),
                     (dict(), b"null pointer"), (dict(kind=2), b"null pointer")]:
        rc = fin(**kw)
        assert rc == BX_EINVAL and b"bx_smoothgrad_finish" in msg() and word in msg(), (kw, rc, msg())

    def sig(Bn=3, per=100, level=0.15):
        return lib.bx_smoothgrad_sigma(None, None, Bn, per, level, None)
    for kw, word in [(dict(Bn=0), b"bad shape"), (dict(per=0), b"bad shape"), (dict(Bn=1 << 11, per=1 << 20), b"32-bit"), (dict(level=-0.5), b"noise level"),
                     (dict(level=float("nan")), b"noise level"), (dict(level=float("inf")), b"noise level"), (dict(), b"null pointer"), (dict(level=0.0), b"null pointer")]:
        rc = sig(**kw)
        assert rc == BX_EINVAL and b"bx_smoothgrad_sigma" in msg() and word in msg(), (kw, rc, msg())
