"""CPU: the EEG Grad-CAM entry point's argument and geometry checks, which run before anything reaches a device."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import brainxai
from brainxai import _lib


def _desc(F1=8, D=2, F2=16, K1=64, chans=19, T=2000):
    return _lib.EegDesc(2, chans, T, F1, D, F2, K1, 16, 4, 8, 0, 1e-5, 0.1, 0.0, 0, _lib.BX_F32, 1, -1.0)


def test_eeg_gradcam_null_pointers():
    lib = _lib.load()
    rc = lib.bx_eeg_gradcam(None, None, None, None, None, 1, _lib.BX_EEG_CAM_CONV1, 1, None, None, None, None, 0, None)
    assert rc < 0 and b"bx_eeg_gradcam" in lib.bx_last_error_string()
    d = _desc()
    rc = lib.bx_eeg_gradcam(ctypes.byref(d), None, None, None, None, 6, _lib.BX_EEG_CAM_SEPARABLE, 1, None, None, None, None, 0, None)
    assert rc < 0 and b"bx_eeg_gradcam" in lib.bx_last_error_string()
    assert lib.bx_eeg_gradcam_workspace(ctypes.byref(d), 6, _lib.BX_EEG_CAM_CONV1) >= 2 * 6 * 64 * 4
    assert lib.bx_eeg_gradcam_workspace(ctypes.byref(d), 6, 3) == 0          # unknown target


def test_eeg_gradcam_refuses_generic_geometry():
    lib = _lib.load()
    BX_EUNSUPPORTED = -6
    for d in (_desc(F1=4, D=3, F2=8, K1=128), _desc(K1=128), _desc(chans=65), _desc(T=16000)):
        # null data pointers: the geometry check comes first and touches nothing
        rc = lib.bx_eeg_gradcam(ctypes.byref(d), None, None, None, None, 1, _lib.BX_EEG_CAM_CONV1, 1, None, None, None, None, 0, None)
        assert rc == BX_EUNSUPPORTED and b"tuned family" in lib.bx_last_error_string()
        assert lib.bx_eeg_gradcam_workspace(ctypes.byref(d), 1, _lib.BX_EEG_CAM_CONV1) == 0
        off_d, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.bx_eeg_saved_layout(ctypes.byref(d), ctypes.byref(off_d), ctypes.byref(off_s)) == BX_EUNSUPPORTED
    d = _desc()
    off_d, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.bx_eeg_saved_layout(ctypes.byref(d), ctypes.byref(off_d), ctypes.byref(off_s)) == 0
    assert 0 < off_d.value < off_s.value < lib.bx_eeg_saved_bytes(ctypes.byref(d))


@pytest.mark.parametrize("layer", ["eeg_model.activation", "eeg_model.dropout", "eeg_model.batchnorm2", "eeg_model.avg_pool1",
                                   "eeg_model.dense"])
def test_eeg_gradcam_unsupported_target_raises_before_launch(monkeypatch, layer):
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
    net = brainxai.build_multimodal(19, 2000, 4)
    with pytest.raises(ValueError, match="eeg_model.conv1.*eeg_model.depthwiseConv.*eeg_model.separableConv"):
        brainxai.grad_cam(net, torch.zeros(1, 1, 19, 2000), torch.zeros(1, 4, 32, 64), layer)
    assert reached == [], f"library entry points reached: {reached}"
