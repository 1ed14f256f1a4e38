"""CPU: brainxai.score_cam argument checks that run before anything reaches a device, the limits of the bx_scorecam_* entry points,
and the restatement of the definition (tests/scorecam_ref.py) against F.interpolate."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib
from tests import scorecam_ref as S

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


# name -> (model kind, positional target or None, keyword overrides, exception, message)
BAD = {
    "weights_unknown": ("multimodal", None, dict(weights="softmax"), ValueError, "unknown weights"),
    "target_unknown": ("multimodal", "spectrogram_model.block6", dict(), ValueError, "unsupported target"),
    "target_unknown_eeg": ("multimodal", "eeg_model.batchnorm1", dict(), ValueError, "unsupported target"),
    "target_not_a_string": ("multimodal", 5, dict(), ValueError, "target_layer must be a string"),
    "target_conv1": ("multimodal", "eeg_model.conv1", dict(), ValueError, "never formed"),
    "target_conv1_stand_alone": ("eegnet", "conv1", dict(), ValueError, "never formed"),
    "class_high": ("multimodal", None, dict(class_idx=6), ValueError, r"outside \[0, 6\)"),
    "class_negative": ("spectrogram", "block3", dict(class_idx=-1), ValueError, r"outside \[0, 6\)"),
    "class_list_high": ("multimodal", "eeg_model.separableConv", dict(class_idx=[0, 7]), ValueError, r"outside \[0, 6\)"),
    "class_list_length": ("multimodal", None, dict(class_idx=torch.tensor([0, 1, 2])), ValueError, "one class per sample"),
    "class_word": ("multimodal", None, dict(class_idx="every"), ValueError, "class_idx 'every'"),
    "baseline_length": ("multimodal", None, dict(baseline=[0.0, 1.0, 2.0]), ValueError, "score_cam: baseline of shape"),
    "baseline_shape": ("multimodal", "block2.conv2", dict(baseline=torch.zeros(B, C, H, W - 1)), ValueError, "score_cam: baseline of shape"),
    "baseline_per_channel_for_eeg": ("eegnet", "depthwiseConv", dict(baseline=torch.zeros(C)), ValueError, "score_cam: baseline of shape"),
    "max_batch_zero": ("multimodal", None, dict(max_batch=0), ValueError, "max_batch = 0"),
    "max_batch_negative": ("eegnet", "separableConv", dict(max_batch=-3), ValueError, "max_batch = -3"),
    "second_input_missing_spec_target": ("multimodal_no_eeg", None, dict(), ValueError, "needs both inputs"),
    "second_input_missing_eeg_target": ("multimodal_no_spec", "eeg_model.depthwiseConv", dict(), ValueError, "needs both inputs"),
    "input_none": ("multimodal_no_spec", "block5", dict(), ValueError, "tensor is None"),
    "eeg_target_on_spectrogram_model": ("spectrogram", "eeg_model.depthwiseConv", dict(), ValueError, "tensor is None"),
    "spectrogram_target_on_eegnet": ("eegnet", "block5", dict(), ValueError, "tensor is None"),
    "cpu_multimodal": ("multimodal", None, dict(), RuntimeError, "no CPU path"),
    "cpu_multimodal_all": ("multimodal", "block3", dict(class_idx="all", weights="increase", relu=False), RuntimeError, "no CPU path"),
    "cpu_multimodal_eeg": ("multimodal", "eeg_model.separableConv", dict(baseline=torch.zeros(CH), upsample=False), RuntimeError, "no CPU path"),
    "cpu_spectrogram": ("spectrogram", "block1.conv3", dict(baseline=torch.zeros(B, C, H, W), class_idx=[1, 2]), RuntimeError, "no CPU path"),
    "cpu_eegnet": ("eegnet", "eeg_model.depthwiseConv", dict(baseline=torch.zeros(B, 1, CH, T), return_parts=True), RuntimeError, "no CPU path"),
    "cpu_deep": ("deep", "separableConv", dict(class_idx=torch.tensor([5, 0])), RuntimeError, "no CPU path"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_raise_before_launch(monkeypatch, case):
    reached = _recorder(monkeypatch)
    kind, target, kw, exc, match = BAD[case]
    eeg, spec = _inputs()
    if kind.startswith("multimodal"):
        model = brainxai.build_multimodal(CH, T, C)
        eeg = None if kind == "multimodal_no_eeg" else eeg
        spec = None if kind == "multimodal_no_spec" else spec
    elif kind == "spectrogram":
        model, eeg = brainxai.Spectrogram_Model(6, in_channels=C), None
    else:
        model = brainxai.EEGNet(6, Chans=CH, Samples=T) if kind == "eegnet" else brainxai.EEGNetAttentionDeep(6, Chans=CH, Samples=T)
        spec = None
    args = (model, eeg, spec) if target is None else (model, eeg, spec, target)
    with pytest.raises(exc, match=match):
        brainxai.score_cam(*args, **kw)
    assert reached == [], f"library entry points reached: {reached}"


def test_other_eegnet_geometries_are_refused_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    net = brainxai.EEGNet(6, Chans=CH, Samples=T, F1=4, D=2, F2=8)
    with pytest.raises(ValueError, match="tuned EEGNet family"):
        brainxai.score_cam(net, _inputs()[0], None, "depthwiseConv")
    assert reached == []


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string

    def plane(h=2, w=4, Cn=16, Bn=2, dt=_lib.BX_F32):
        return dt, h * w * Cn, 1, w * Cn, Cn, Bn, Cn, h, w

    def rng(Hm=64, Wm=128, ws=1 << 20, **kw):
        dt, sb, sc, sy, sx, Bn, Cn, h, w = plane(**kw)
        return lib.bx_scorecam_range(None, dt, sb, sc, sy, sx, Bn, Cn, h, w, Hm, Wm, None, None, None, None, ws, None)
    for kw, code, word in [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(h=0), BX_EINVAL, b"bad shape"), (dict(Wm=0), BX_EINVAL, b"bad shape"),
                           (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per mask"), (dict(h=1024, w=1024), BX_EUNSUPPORTED, b"cells per mask"),
                           (dict(h=512, w=512, Cn=256, Bn=64), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = rng(**kw)
        assert rc == code and b"bx_scorecam_range" in msg() and word in msg(), (kw, rc, msg())
    assert rng(dt=7) < 0 and b"dtype" in msg()
    assert lib.bx_scorecam_range(None, 0, 64, 1, -8, 2, 2, 16, 2, 4, 64, 128, None, None, None, None, 0, None) == BX_EINVAL and b"negative stride" in msg()
    assert lib.bx_scorecam_range_workspace(2, 16, 64, 128) == 2 * 16 * 2 * 2 * 4 and lib.bx_scorecam_range_workspace(2, 16, 1024, 1024) == 0
    assert lib.bx_scorecam_range_workspace(0, 16, 64, 128) == 0

    def spec(Cin=3, Hm=64, Wm=128, Cp=8, b0=0, nb=2, k0=0, n=16, kind=0, out_dt=_lib.BX_F32, **kw):
        dt, sb, sc, sy, sx, Bn, Cn, h, w = plane(**kw)
        return lib.bx_scorecam_perturb_spec(None, None, dt, sb, sc, sy, sx, Cn, h, w, None, None, None, kind, None, Bn, Cin, Hm, Wm, Cp, b0, nb, k0, n,
                                            out_dt, None)
    for kw, code, word in [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(Hm=1024, Wm=1024), BX_EUNSUPPORTED, b"cells per mask"),
                           (dict(b0=1), BX_EINVAL, b"samples b0"), (dict(nb=0), BX_EINVAL, b"samples b0"), (dict(b0=-1), BX_EINVAL, b"samples b0"),
                           (dict(k0=8, n=9), BX_EINVAL, b"channels k0"), (dict(n=0), BX_EINVAL, b"channels k0"), (dict(k0=-1), BX_EINVAL, b"channels k0"),
                           (dict(kind=3), BX_EINVAL, b"baseline_kind"), (dict(Cin=5), BX_EUNSUPPORTED, b"input channels"),
                           (dict(Cin=0), BX_EUNSUPPORTED, b"input channels"), (dict(Cp=16), BX_EINVAL, b"Cp"),
                           (dict(Hm=512, Wm=512, Cn=600, n=600, nb=1), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                           (dict(h=64, w=128, out_dt=_lib.BX_BF16, dt=_lib.BX_BF16), BX_EINVAL, b"null pointer")]:
        rc = spec(**kw)
        assert rc == code and b"bx_scorecam_perturb_spec" in msg() and word in msg(), (kw, rc, msg())
    assert spec(out_dt=7) < 0 and b"dtype" in msg()

    def eeg(Bn=2, Cn=16, w=500, Ch=19, Tt=2000, b0=0, nb=2, k0=0, n=16, kind=0):
        return lib.bx_scorecam_perturb_eeg(None, None, _lib.BX_F32, Cn * w, w, 1, Cn, w, None, None, None, kind, None, Bn, Ch, Tt, b0, nb, k0, n, None)
    for kw, code, word in [(dict(Tt=0), BX_EINVAL, b"bad shape"), (dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(w=0), BX_EINVAL, b"bad shape"),
                           (dict(b0=1), BX_EINVAL, b"samples b0"), (dict(k0=15, n=2), BX_EINVAL, b"channels k0"), (dict(kind=-1), BX_EINVAL, b"baseline_kind"),
                           (dict(Bn=256, nb=256, Ch=64, Tt=15000), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                           (dict(w=2000, Tt=2000), BX_EINVAL, b"null pointer")]:
        rc = eeg(**kw)
        assert rc == code and b"bx_scorecam_perturb_eeg" in msg() and word in msg(), (kw, rc, msg())

    def comb(K=6, mode=0, **kw):
        dt, sb, sc, sy, sx, Bn, Cn, h, w = plane(**kw)
        return lib.bx_scorecam_combine(None, None, None, None, None, dt, sb, sc, sy, sx, Bn, Cn, h, w, K, mode, 1, None, None, None, None)
    for kw, code, word in [(dict(Bn=0), BX_EINVAL, b"bad shape"), (dict(K=0), BX_EINVAL, b"bad shape"), (dict(K=33), BX_EUNSUPPORTED, b"classes"),
                           (dict(mode=2), BX_EINVAL, b"weight_mode"), (dict(h=1024, w=1024), BX_EUNSUPPORTED, b"cells per mask"),
                           (dict(K=32, Bn=4096, h=128, w=256, Cn=1), BX_EINVAL, b"32-bit"), (dict(), BX_EINVAL, b"null pointer"),
                           (dict(mode=1, K=32), BX_EINVAL, b"null pointer")]:
        rc = comb(**kw)
        assert rc == code and b"bx_scorecam_combine" in msg() and word in msg(), (kw, rc, msg())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
PLANES = {"2x4 to 64x128": (2, 4, 64, 128), "7x5 to 100x75": (7, 5, 100, 75), "16x24 to 16x24": (16, 24, 16, 24), "1x500 to 1x2000": (1, 500, 1, 2000),
          "1x2000 to 1x2000": (1, 2000, 1, 2000)}


def _planes(h, w, Cn=16, seed=0):
    """float32 [Cn,h,w]: every channel an offset plus a tenth of it in noise, odd channels negative, channel 1 constant.
    The bound below counts roundings of VALUES.  The source coordinate s = scale (o + 0.5) - 0.5 has a rounding of its own, and
    F.interpolate's build forms it with a fused multiply-add while the definition (and the kernels) round the product first: the two
    l = s - i0 differ by up to an ulp of s (4.8e-7 for s in [4, 8)), which enters the result multiplied by the DIFFERENCE of the two
    neighbours.  On unit-variance noise that term alone is 6 ulps of the largest magnitude at 7x5 -> 100x75 (2 with the coordinate
    fused, checked in fp64); here neighbours differ by a fraction of their magnitude, so the value roundings are what is measured."""
    g = np.random.default_rng(seed)
    a = (np.float32(2.0) + np.float32(0.1) * g.standard_normal((Cn, h, w)).astype(np.float32)).astype(np.float32)
    a[1::2] = -a[1::2]
    a[1] = np.float32(0.375)
    return a


@pytest.mark.parametrize("case", sorted(PLANES))
def test_upsample_restatement_equals_interpolate(case):
    h, w, Hm, Wm = PLANES[case]
    a = _planes(h, w)
    got = S.upsample(a, Hm, Wm)
    want = F.interpolate(torch.from_numpy(a)[None], size=(Hm, Wm), mode="bilinear", align_corners=False)[0].numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (16, Hm, Wm)
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    bound = 4 * float(np.spacing(np.abs(a).max()))                   # a handful of fp32 roundings at the plane's largest magnitude
    print(f"upsample restatement against F.interpolate, {case}: {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound
    if (h, w) == (Hm, Wm):
        assert np.array_equal(got, a), "up-sampling to the plane's own size is the identity (up to the sign of a zero)"
    lo, hi, scale, valid = S.ranges(got)
    assert lo.dtype == hi.dtype == scale.dtype == np.float32 and valid.dtype == bool
    assert not valid[1] and scale[1] == 0 and lo[1] == hi[1] == np.float32(0.375), "a constant plane is invalid"
    assert valid[[0, 2, 3]].all() and hi[3] < 0 and lo[2] > 0 and (valid.sum() == 15)
    m = S.mask(got, lo, scale)
    assert m.dtype == np.float32 and float(m.min()) >= 0.0 and float(m.max()) <= 1.0
    assert (m[1] == 0).all() and (m[valid].reshape(15, -1).min(1) == 0).all() and (m[valid].reshape(15, -1).max(1) >= 1 - 2.0 ** -22).all()


def test_rows_weights_and_sum_restatements():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6) + 1
    M = np.zeros((2, 3, 4, 6), dtype=np.float32)
    M[:, 1] = 1.0
    M[:, 2] = 0.5
    r = S.rows(x, M, 0.25)
    assert tuple(r.shape) == (6, 3, 4, 6) and torch.equal(r[0], torch.full_like(x[0], 0.25)) and torch.equal(r[1], x[0]) and torch.equal(r[4], x[1])
    assert torch.equal(r[5], 0.25 + 0.5 * (x[1] - 0.25))
    assert torch.equal(S.rows(x, M, 0.25, 1, 1, 1, 2), r[4:6])
    P = np.random.default_rng(1).random((2, 3, 5)).astype(np.float32)
    Pb = np.random.default_rng(2).random((2, 5)).astype(np.float32)
    valid = np.array([[True, False, True], [True, True, True]])
    w = S.weights(P, Pb, valid, "prob")
    assert w.shape == (2, 5, 3) and w.dtype == np.float32 and (w[0, :, 1] == 0).all() and w[1, 4, 2] == P[1, 2, 4]
    wi = S.weights(P, Pb, valid, "increase")
    assert wi.dtype == np.float32 and wi[1, 4, 2] == np.float32(P[1, 2, 4] - Pb[1, 4]) and (wi[0, :, 1] == 0).all()
    A = np.random.default_rng(3).standard_normal((2, 3, 2, 2)).astype(np.float32)
    raw, mag = S.combine(w, A)
    assert raw.shape == (2, 5, 2, 2) and np.isclose(raw[1, 4, 1, 0], sum(float(P[1, k, 4]) * float(A[1, k, 1, 0]) for k in range(3)), rtol=1e-14, atol=0)
    assert (mag >= np.abs(raw)).all()
