"""No GPU: the grouped weight-gradient entries refuse bad arguments before they touch a pointer or launch anything."""
import ctypes

from brainxai import _lib as L


def _layers(n, ci=64, co=64):
    arr = (L.WgradGroupLayer * max(n, 1))()
    for i in range(n):
        arr[i] = L.WgradGroupLayer(None, None, None, None, ci, ci, co)
    return arr


def test_group_entries_refuse_bad_arguments():
    lib = L.load()
    pend = (L.WgradPending * 4)()
    for n in (0, 4, -1):
        rc = lib.bx_conv3x3_wgrad_group(_layers(4), n, 3, 8, 16, L.BX_BF16, None, 0, pend, None)
        assert rc < 0 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
        assert lib.bx_conv3x3_wgrad_group_workspace(_layers(4), n, 3, 8, 16, L.BX_BF16) == 0
        assert b"bx_conv3x3_wgrad_group_workspace" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_wgrad_group(None, 3, 3, 8, 16, L.BX_BF16, None, 0, pend, None)          # no layer table
    assert rc < 0 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_wgrad_group(_layers(3), 3, 3, 8, 16, L.BX_BF16, None, 0, None, None)    # no pending table
    assert rc < 0 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_wgrad_group(_layers(3), 3, 3, 8, 16, L.BX_BF16, None, 0, pend, None)    # null tensors
    assert rc < 0 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_wgrad_group(_layers(3), 3, 3, 8, 16, L.BX_F32, None, 0, pend, None)     # fp32 storage
    assert rc == -6 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_wgrad_group(_layers(2, ci=16), 2, 3, 8, 16, L.BX_BF16, None, 0, pend, None)   # not a tile-owner shape
    assert rc == -6
    assert all(pend[i].valid == 0 for i in range(4))


def test_group_supported_and_workspace_without_gpu():
    lib = L.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    assert lib.bx_conv3x3_wgrad_group_supported(3, ints(256, 256, 128), ints(256, 256, 256), 16, L.BX_BF16) == 1
    assert lib.bx_conv3x3_wgrad_group_supported(1, ints(64), ints(128), 32, L.BX_BF16) == 1
    assert lib.bx_conv3x3_wgrad_group_supported(3, ints(32, 32, 16), ints(32, 32, 32), 128, L.BX_BF16) == 0     # stage 2's conv1
    assert lib.bx_conv3x3_wgrad_group_supported(3, ints(64, 64, 32), ints(64, 64, 64), 64, L.BX_F32) == 0
    assert lib.bx_conv3x3_wgrad_group_supported(4, ints(64, 64, 64, 64), ints(64, 64, 64, 64), 64, L.BX_BF16) == 0
    assert lib.bx_conv3x3_wgrad_group_supported(2, None, None, 64, L.BX_BF16) == 0
    # the group's workspace holds every layer's own partials (each region rounded up to 256 bytes)
    lay = (L.WgradGroupLayer * 3)()
    single = 0
    for i, (ci, co) in enumerate(((256, 256), (256, 256), (128, 256))):
        lay[i] = L.WgradGroupLayer(None, None, None, None, ci, ci, co)
        single += (lib.bx_conv3x3_wgrad_workspace(64, 8, 16, ci, co, L.BX_BF16, L.BX_ALGO_MFMA) + 255) // 256 * 256
    assert lib.bx_conv3x3_wgrad_group_workspace(lay, 3, 64, 8, 16, L.BX_BF16) == single > 0


def test_carry_many_refuses_bad_counts():
    lib = L.load()
    pend = (L.WgradPending * 4)()
    for n in (0, 4):
        rc = lib.bx_conv3x3_carry_many(None, None, None, None, None, None, None, 1, 4, 4, 8, 8, L.BX_BF16, 0, 0, pend, n, None)
        assert rc < 0 and b"bx_conv3x3_carry_many" in lib.bx_last_error_string()
    rc = lib.bx_conv3x3_carry_many(None, None, None, None, None, None, None, 1, 4, 4, 8, 8, L.BX_BF16, 0, 0, None, 3, None)
    assert rc < 0 and b"bx_conv3x3_carry_many" in lib.bx_last_error_string()
