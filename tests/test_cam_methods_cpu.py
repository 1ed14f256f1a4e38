"""CPU: Grad-CAM++ / Layer-CAM argument checks that run before anything reaches a device, and the closed forms the last-stage
kernel uses (include/brainxai.h, bx_cam_head) against the general definitions in fp64."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import brainxai
from brainxai import _lib

EPS = 1e-6


def _desc(F1=8, D=2, F2=16, K1=64, chans=19, T=2000):
    return _lib.EegDesc(2, chans, T, F1, D, F2, K1, 16, 4, 8, 0, 1e-5, 0.1, 0.0, 0, _lib.BX_F32, 1, -1.0)


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


@pytest.mark.parametrize("layer", ["spectrogram_model.block5", "spectrogram_model.block3", "spectrogram_model.block2.conv1",
                                   "eeg_model.conv1", "eeg_model.separableConv"])
def test_unknown_method_raises_before_launch(monkeypatch, layer):
    reached = _recorder(monkeypatch)
    net = brainxai.build_multimodal(19, 2000, 4)
    with pytest.raises(ValueError, match="'gradcam'.*'gradcam\\+\\+'.*'layercam'"):
        brainxai.grad_cam(net, torch.zeros(1, 1, 19, 2000), torch.zeros(1, 4, 32, 64), layer, method="bogus")
    assert reached == [], f"library entry points reached: {reached}"


def test_sweep_unknown_method_raises_before_launch(monkeypatch):
    reached = _recorder(monkeypatch)
    net = brainxai.build_multimodal(19, 2000, 4)
    with pytest.raises(ValueError, match="'gradcam'.*'gradcam\\+\\+'.*'layercam'"):
        brainxai.GradCamSweep(net, torch.zeros(1, 1, 19, 2000), torch.zeros(1, 4, 32, 64), method="GradCAM++")
    assert reached == []


def test_cam_reduce_refuses_bad_method():
    lib = _lib.load()
    for method in (-1, 3, 7):
        rc = lib.bx_cam_reduce(None, None, None, None, 1, 1, 4, 8, method, 1, _lib.BX_F32, None)
        assert rc < 0 and b"unknown method" in lib.bx_last_error_string()
    # Layer-CAM has no channel weights: a weights buffer is refused before any pointer is touched
    rc = lib.bx_cam_reduce(None, None, None, ctypes.c_void_p(16), 1, 1, 4, 8, _lib.BX_CAM_LAYERCAM, 1, _lib.BX_F32, None)
    assert rc < 0 and b"Layer-CAM" in lib.bx_last_error_string()
    for method in (_lib.BX_CAM_GRADCAM_PP, _lib.BX_CAM_LAYERCAM):
        rc = lib.bx_cam_reduce(None, None, None, None, 0, 1, 4, 8, method, 1, _lib.BX_F32, None)
        assert rc < 0 and b"bx_cam_reduce" in lib.bx_last_error_string()


def test_cam_head_refuses_bad_method():
    lib = _lib.load()
    null = [None] * 12
    rc = lib.bx_cam_head(*null, 2, 16, 8, 6, 32, -1, 3, 1, _lib.BX_F32, None)
    assert rc < 0 and b"unknown method" in lib.bx_last_error_string()
    wts = [None] * 11 + [ctypes.c_void_p(16)]
    rc = lib.bx_cam_head(*wts, 2, 16, 8, 6, 32, -1, _lib.BX_CAM_LAYERCAM, 1, _lib.BX_F32, None)
    assert rc < 0 and b"Layer-CAM" in lib.bx_last_error_string()
    rc = lib.bx_cam_head_sweep(None, None, None, None, 16, *[None] * 8, 2, 4, 4, 8, 6, 32, 8, 8, -1, -2, 1, _lib.BX_F32, None)
    assert rc < 0 and b"unknown method" in lib.bx_last_error_string()


def test_eeg_cam_refuses_bad_method_and_generic_geometry():
    lib = _lib.load()
    d = _desc()
    for method in (-1, 3):
        rc = lib.bx_eeg_cam(ctypes.byref(d), None, None, None, None, 1, _lib.BX_EEG_CAM_CONV1, method, 1, None, None, None, None, 0, None)
        assert rc < 0 and b"unknown method" in lib.bx_last_error_string()
        assert lib.bx_eeg_cam_workspace(ctypes.byref(d), 1, _lib.BX_EEG_CAM_CONV1, method) == 0
        assert b"unknown method" in lib.bx_last_error_string()
    rc = lib.bx_eeg_cam(ctypes.byref(d), None, None, None, None, 1, _lib.BX_EEG_CAM_DEPTHWISE, _lib.BX_CAM_LAYERCAM, 1, None, None,
                        ctypes.c_void_p(16), None, 0, None)
    assert rc < 0 and b"Layer-CAM" in lib.bx_last_error_string()
    # workspaces: Grad-CAM++ needs what Grad-CAM needs; Layer-CAM at conv1 keeps the per-element gradient [B, nm, 16, T]
    for target in (_lib.BX_EEG_CAM_CONV1, _lib.BX_EEG_CAM_DEPTHWISE, _lib.BX_EEG_CAM_SEPARABLE):
        assert lib.bx_eeg_cam_workspace(ctypes.byref(d), 6, target, _lib.BX_CAM_GRADCAM) == lib.bx_eeg_gradcam_workspace(ctypes.byref(d), 6, target)
        assert lib.bx_eeg_cam_workspace(ctypes.byref(d), 6, target, _lib.BX_CAM_GRADCAM_PP) >= 2 * 6 * 64 * 4
    assert lib.bx_eeg_cam_workspace(ctypes.byref(d), 6, _lib.BX_EEG_CAM_CONV1, _lib.BX_CAM_LAYERCAM) >= 2 * 6 * 16 * 2000 * 4
    BX_EUNSUPPORTED = -6
    for g in (_desc(F1=4, D=3, F2=8, K1=128), _desc(K1=128), _desc(chans=65), _desc(T=16000)):
        for method in (_lib.BX_CAM_GRADCAM_PP, _lib.BX_CAM_LAYERCAM):
            rc = lib.bx_eeg_cam(ctypes.byref(g), None, None, None, None, 1, _lib.BX_EEG_CAM_CONV1, method, 1, None, None, None, None, 0, None)
            assert rc == BX_EUNSUPPORTED and b"tuned family" in lib.bx_last_error_string()
            for target in (_lib.BX_EEG_CAM_CONV1, _lib.BX_EEG_CAM_SEPARABLE):
                assert lib.bx_eeg_cam_workspace(ctypes.byref(g), 1, target, method) == 0


def _general(A, G, method):
    """The definitions of include/brainxai.h in fp64: A, G [K, S] -> (raw [S], w [K] or None)."""
    if method == "layercam":
        return (G.clamp_min(0) * A).sum(0), None
    S = A.sum(1, keepdim=True)
    den = 2 * G ** 2 + S * G ** 3 + EPS
    alpha = torch.where(G == 0, torch.zeros_like(G), G ** 2 / den)
    w = (G.clamp_min(0) * alpha).sum(1)
    return (w[:, None] * A).sum(0), w


def _closed(A, g, method):
    """The last-stage forms: G[k, s] = g[k] at every position, S[k] = HW gap[k]."""
    HW = A.shape[1]
    if method == "layercam":
        w = g.clamp_min(0)
    else:
        S = HW * A.mean(1)
        w = torch.where(g > 0, HW * g ** 3 / (2 * g ** 2 + S * g ** 3 + EPS), torch.zeros_like(g))
    return (w[:, None] * A).sum(0), w


@pytest.mark.parametrize("method", ["gradcam++", "layercam"])
@pytest.mark.parametrize("K,HW,seed", [(16, 64, 0), (128, 32, 1), (512, 8, 2)])
def test_last_stage_closed_forms_equal_definitions(method, K, HW, seed):
    gen = torch.Generator().manual_seed(seed)
    A = torch.rand(K, HW, generator=gen, dtype=torch.float64) * 2.0          # post-ReLU stage output: non-negative
    g = torch.randn(K, generator=gen, dtype=torch.float64) * 1e-2
    g[::7] = 0.0                                                              # exact zeros: alpha = 0 there
    G = g[:, None].expand(K, HW).contiguous()
    raw, w = _general(A, G, method)
    raw_c, w_c = _closed(A, g, method)
    assert torch.allclose(raw, raw_c, rtol=1e-12, atol=1e-14 * float(raw.abs().max()))
    if w is not None:
        assert torch.allclose(w, w_c, rtol=1e-12, atol=0.0)
