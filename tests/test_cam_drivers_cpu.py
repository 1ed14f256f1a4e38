"""CPU: the pieces the class-activation drivers of explain.py share (grad_cam, its EEG and last-stage forms, score_cam's clean pass):
the class form, the result shaper, the capture of a spectrogram target and what it leaves behind, and the EEG target's saved plane."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
from torch import nn

import brainxai
from brainxai import _lib
from brainxai import explain as E


class Blk(nn.Module):
    """What the capture needs of a Block: its two capture attributes; the forward raises unless told otherwise."""

    def __init__(self, fail=True):
        super().__init__()
        self._preact, self._capture, self.fail = 0, None, fail

    def forward(self, x):
        if self.fail:
            raise RuntimeError("boom")
        return x


class Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.block2 = Blk()
        self.w = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return self.block2(x)


def _clean(blk):
    return blk._preact == 0 and blk._capture is None and len(blk._forward_hooks) == len(blk._forward_pre_hooks) == 0


def test_class_form():
    assert E._class_form(None) == (-1, False)
    assert E._class_form(0) == (0, False)
    assert E._class_form(5) == (5, False)
    assert E._class_form("all") == (-2, True)
    with pytest.raises(ValueError, match="best"):
        E._class_form("best")
    stub = Stub()
    with pytest.raises(ValueError, match="best"):            # refused before the forward pass, which would raise 'boom'
        brainxai.grad_cam(stub, None, torch.zeros(1, 4, 8, 8), "block2.conv1", class_idx="best")
    assert _clean(stub.block2)


def test_class_axis():
    B, nm = 2, 3
    t = torch.arange(B * nm, dtype=torch.float32).reshape(-1, 1, 1).expand(B * nm, 4, 5).contiguous()
    cam, raw, wts = E._class_axis(B, nm, True, t, None, t[:, :, 0])
    assert tuple(cam.shape) == (2, 3, 4, 5) and raw is None and tuple(wts.shape) == (2, 3, 4)
    for b in range(B):
        for c in range(nm):
            assert bool((cam[b, c] == b * 3 + c).all()) and bool((wts[b, c] == b * 3 + c).all())
    cam, raw, wts = E._class_axis(B, nm, False, t, None, t[:, :, 0])
    assert cam is t and raw is None and tuple(wts.shape) == (6, 4)


@pytest.mark.parametrize("conv_k", [0, 1])
def test_spec_target_leaves_the_block_clean(conv_k):
    x = torch.zeros(1, 4, 8, 8)
    blk = Blk(fail=False)
    with E._SpecTarget(blk, conv_k, want_input=True) as tgt:                      # normal exit
        assert blk._preact == conv_k and (blk._capture == {} if conv_k else blk._capture is None)
        assert len(blk._forward_hooks) + len(blk._forward_pre_hooks) == 1
        blk(x)
        assert tgt.leaf is x
    assert _clean(blk)
    with pytest.raises(KeyError):                                                 # an exception in the body
        with E._SpecTarget(blk, conv_k, want_input=True):
            raise KeyError("body")
    assert _clean(blk)
    blk = Blk()
    with pytest.raises(RuntimeError, match="boom"):                               # an exception from the block's own forward
        with E._SpecTarget(blk, conv_k, want_input=True):
            blk(x)
    assert _clean(blk)


def test_grad_cam_forward_failure_leaves_the_block_clean():
    stub = Stub()
    stub.train()
    assert stub.w.requires_grad
    with pytest.raises(RuntimeError, match="boom"):
        brainxai.grad_cam(stub, None, torch.zeros(1, 4, 8, 8), "block2.conv1")
    assert _clean(stub.block2)
    assert stub.training and stub.w.requires_grad


@pytest.mark.parametrize("layer", ["depthwiseConv", "separableConv"])
def test_eeg_target_plane(layer):
    lib = _lib.load()
    B, T = 2, 2000
    d = _lib.EegDesc(B, 19, T, 8, 2, 16, 64, 16, 4, 8, 0, 1e-5, 0.1, 0.0, 0, _lib.BX_F32, 1, -1.0)
    g = SimpleNamespace(F1=8, D=2, F2=16, P1=4)
    off_d, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.bx_eeg_saved_layout(ctypes.byref(d), ctypes.byref(off_d), ctypes.byref(off_s)) == 0
    off, shape = (off_d.value, (B, 16, 1, T)) if layer == "depthwiseConv" else (off_s.value, (B, 16, 1, T // 4))
    known = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    arena = torch.zeros(lib.bx_eeg_saved_bytes(ctypes.byref(d)), dtype=torch.uint8)
    arena[off:off + known.numel() * 4].view(torch.float32).copy_(known.flatten())
    A = E._eeg_target_plane(arena, d, g, B, T, layer)
    assert A.dtype == torch.float32 and tuple(A.shape) == shape and torch.equal(A, known)
    arena.fill_(255)                                                              # a copy: the arena can be reused
    assert torch.equal(A, known)
