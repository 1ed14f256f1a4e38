"""CPU: Block accepts the reference's pooling windows other than 2x2 (any non-overlapping window, int k or (ph, pw)), refuses
what the reference's pooling modules cannot mean, and the tail's C ABI sizes its workspace for the window."""
import ctypes

import pytest
import torch.nn as nn

import brainxai
from brainxai import _lib
from oracle import ref_torch as O


@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("k", [3, (3, 3), (1, 2), (4, 2)])
def test_block_builds_any_window(kind, k):
    mine, ref = brainxai.Block(4, 16, kind, k), O.Block(4, 16, kind, k)
    sm, sr = mine.state_dict(), ref.state_dict()
    assert list(sm) == list(sr)
    assert all(tuple(sm[n].shape) == tuple(sr[n].shape) for n in sr)
    assert type(mine.pool) is type(ref.pool) is (nn.MaxPool2d if kind == "max" else nn.AvgPool2d)
    assert mine.pool.kernel_size == ref.pool.kernel_size
    assert mine.pool_window == ((k, k) if isinstance(k, int) else k)


@pytest.mark.parametrize("k", [0, (0, 2), (2, 2, 2), -1, 2.5, (2, 1.5), (True, 2), "2"])
def test_block_refuses_bad_windows(k):
    with pytest.raises(ValueError):
        brainxai.Block(4, 16, "max", k)


def test_tail_workspace_follows_window():
    lib = _lib.load()
    d = _lib.TailDesc(2, 8, 8, 8, 16, 0, 1, 1e-5, 0.1, 0.0, 0, 0)
    assert (d.pool_h, d.pool_w) == (0, 0)                               # positional descriptors keep the 2x2 meaning
    w22 = lib.bx_block_tail_workspace(ctypes.byref(d))
    d.pool_h = d.pool_w = 2
    assert lib.bx_block_tail_workspace(ctypes.byref(d)) == w22 > 0
    assert lib.bx_block_tail_route_bytes(ctypes.byref(d)) > 0
    d.pool_h = d.pool_w = 3
    assert lib.bx_block_tail_workspace(ctypes.byref(d)) > 0
    assert lib.bx_block_tail_route_bytes(ctypes.byref(d)) == 0           # route nibbles are 2x2 only
    # a 1-row window keeps the skip gradient at full resolution: the workspace grows with the pooled map
    big = _lib.TailDesc(2, 64, 64, 8, 16, 0, 1, 1e-5, 0.1, 0.0, 0, 0)
    ws_big22 = lib.bx_block_tail_workspace(ctypes.byref(big))
    big.pool_h, big.pool_w = 1, 1
    assert lib.bx_block_tail_workspace(ctypes.byref(big)) >= ws_big22 + 4 * 2 * 64 * 64 * 8 * 3 // 4
    small = _lib.TailDesc(2, 2, 8, 8, 16, 0, 1, 1e-5, 0.1, 0.0, 0, 0)    # H < pool_h
    small.pool_h, small.pool_w = 3, 3
    assert lib.bx_block_tail_workspace(ctypes.byref(small)) == 0
    small.pool_h, small.pool_w = -1, 2
    assert lib.bx_block_tail_workspace(ctypes.byref(small)) == 0
