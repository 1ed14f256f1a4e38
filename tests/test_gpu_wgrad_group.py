"""GPU: the weight gradients of one Block in ONE launch (bx_conv3x3_wgrad_group) with their sums carried by one convolution
launch (bx_conv3x3_carry_many).  Per workgroup the group launch does what the layer's own launch does and the sums keep their
slice count, so everything is compared bit for bit against the chained single-layer launches."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib as L
from brainxai import ops
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 3
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bf(t):
    return t.to(torch.bfloat16).float()


def _layer_data(h, w, chans, seed):
    """per layer: (x NHWC bf16, dz NHWC bf16, cin, cout, fp32 autograd dW, db of the bf16 operands)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for cin, cout in chans:
        x = _bf(torch.randn(B, cin, h, w, generator=g))
        dz = _bf(torch.randn(B, cout, h, w, generator=g) * 0.1)
        wt = torch.zeros(cout, cin, 3, 3, requires_grad=True)
        bias = torch.zeros(cout, requires_grad=True)
        (F.conv2d(x, wt, bias, padding=1) * dz).sum().backward()
        out.append((ops.to_nhwc(x.to(DEV), torch.bfloat16), ops.to_nhwc(dz.to(DEV), torch.bfloat16), cin, cout, wt.grad, bias.grad))
    return out


def _nan_grads(data):
    return [(torch.full((cout, cin, 3, 3), NAN, device=DEV), torch.full((cout,), NAN, device=DEV)) for _, _, cin, cout, _, _ in data]


def _group_layers(data, grads):
    arr = (L.WgradGroupLayer * len(data))()
    for i, ((xn, dzn, cin, cout, _, _), (dw, db)) in enumerate(zip(data, grads)):
        arr[i] = L.WgradGroupLayer(xn.data_ptr(), dzn.data_ptr(), dw.data_ptr(), db.data_ptr(), cin, xn.shape[3], cout)
    return arr


class _Carrier:
    """a small data-gradient style convolution (64 -> 32 channels at 16 x 32) that can carry pending sums"""

    def __init__(self):
        g = torch.Generator().manual_seed(21)
        wt = _bf(torch.randn(64, 32, 3, 3, generator=g) / 24).to(DEV)
        self.packed = ops._pack(wt, True, torch.bfloat16)
        self.g = ops.to_nhwc(torch.randn(B, 64, 16, 32, generator=g).to(DEV), torch.bfloat16)
        self.mk = ops.to_nhwc(torch.randn(B, 32, 16, 32, generator=g).to(DEV), torch.bfloat16)
        self.ad = ops.to_nhwc(torch.randn(B, 32, 16, 32, generator=g).to(DEV), torch.bfloat16)

    def _args(self, y):
        return (self.g.data_ptr(), None, self.packed[1].data_ptr(), None, self.mk.data_ptr(), self.ad.data_ptr(), y.data_ptr(), B, 16, 32,
                self.g.shape[3], self.packed[3], L.BX_BF16, 0, L.BX_ALGO_MFMA)

    def plain(self):
        y = torch.full((B, 16, 32, self.packed[3]), NAN, dtype=torch.bfloat16, device=DEV)
        L.check(L.load().bx_conv3x3(*self._args(y), _stream()), "conv")
        return y

    def carry(self, pend, n):
        y = torch.full((B, 16, 32, self.packed[3]), NAN, dtype=torch.bfloat16, device=DEV)
        L.check(L.load().bx_conv3x3_carry_many(*self._args(y), pend, n, _stream()), "conv carry_many")
        return y


CASES = [(8, 16, ((64, 64), (64, 64), (32, 64))),          # TW = 16, one tile per image, unequal Ci
         (4, 8, ((256, 256), (256, 256), (128, 256))),     # partial tile in both directions; nsplit 3 < 8: whole XCD lanes return early
         (24, 40, ((32, 32), (32, 32))),                   # TW = 32, ragged last column tile, nsplit 18 > 8, n = 2
         (16, 32, ((64, 128),))]                           # n = 1


@pytest.mark.parametrize("h,w,chans", CASES)
def test_group_equals_chain_bit_for_bit(h, w, chans):
    """bx_conv3x3_wgrad_group + carried sums == the same layers through bx_conv3x3_wgrad_chained (one extra trailing layer, so that
    every compared sum is taken by a carrying launch and has the carried slice count): torch.equal on dw and db; and both within
    test_wgrad_mfma's 1e-4 of the fp32 autograd reference."""
    lib = L.load()
    data = _layer_data(h, w, chans, seed=h * 100 + w)
    n = len(data)
    # chain: the compared layers in group order, then a trailing 32 -> 32 layer whose launch sums the last compared one
    chain = data + _layer_data(h, w, ((32, 32),), seed=7)
    want = _nan_grads(chain)
    pend, bufs = L.WgradPending(), []
    for (xn, dzn, cin, cout, _, _), (dw, db) in zip(chain, want):
        need = lib.bx_conv3x3_wgrad_workspace(B, h, w, xn.shape[3], cout, L.BX_BF16, L.BX_ALGO_MFMA)
        bufs.append(torch.empty(need, dtype=torch.uint8, device=DEV))
        L.check(lib.bx_conv3x3_wgrad_chained(xn.data_ptr(), dzn.data_ptr(), dw.data_ptr(), db.data_ptr(), B, h, w, cin, xn.shape[3], cout, L.BX_BF16,
                                             L.BX_ALGO_MFMA, bufs[-1].data_ptr(), bufs[-1].numel(), ctypes.byref(pend), _stream()), "wgrad chained")
    L.check(lib.bx_conv3x3_wgrad_finish(ctypes.byref(pend), _stream()), "finish")
    # group
    got = _nan_grads(data)
    layers = _group_layers(data, got)
    ci = (ctypes.c_int * n)(*[d[0].shape[3] for d in data])
    co = (ctypes.c_int * n)(*[d[3] for d in data])
    assert lib.bx_conv3x3_wgrad_group_supported(n, ci, co, w, L.BX_BF16) == 1
    need = lib.bx_conv3x3_wgrad_group_workspace(layers, n, B, h, w, L.BX_BF16)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    pends = (L.WgradPending * 3)()
    L.check(lib.bx_conv3x3_wgrad_group(layers, n, B, h, w, L.BX_BF16, ws.data_ptr(), ws.numel(), pends, _stream()), "wgrad group")
    assert [pends[i].valid for i in range(3)] == [1] * n + [0] * (3 - n)
    torch.cuda.synchronize()
    assert all(torch.isnan(dw).all() for dw, _ in got)        # the group launch sums nothing
    _Carrier().carry(pends, n)
    assert all(pends[i].valid == 0 for i in range(3))
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(got[i][0], want[i][0]), i
        assert torch.equal(got[i][1], want[i][1]), i
        assert rel_err(got[i][0].cpu(), data[i][4]) < 1e-4, i
        assert rel_err(got[i][1].cpu(), data[i][5]) < 1e-4, i


def test_carrying_three_sums_changes_nothing_else():
    """a convolution through bx_conv3x3_carry_many with three pendings returns what bx_conv3x3 returns and leaves nothing pending"""
    lib = L.load()
    h, w = 8, 16
    data = _layer_data(h, w, ((64, 64), (64, 64), (32, 64)), seed=3)
    got = _nan_grads(data)
    layers = _group_layers(data, got)
    ws = torch.empty(lib.bx_conv3x3_wgrad_group_workspace(layers, 3, B, h, w, L.BX_BF16), dtype=torch.uint8, device=DEV)
    pends = (L.WgradPending * 3)()
    L.check(lib.bx_conv3x3_wgrad_group(layers, 3, B, h, w, L.BX_BF16, ws.data_ptr(), ws.numel(), pends, _stream()), "wgrad group")
    conv = _Carrier()
    y_plain = conv.plain()
    y_carry = conv.carry(pends, 3)
    assert [pends[i].valid for i in range(3)] == [0, 0, 0]
    torch.cuda.synchronize()
    assert not torch.isnan(y_plain.float()).any()
    assert torch.equal(y_carry.view(torch.int16), y_plain.view(torch.int16))
    for dw, db in got:
        assert not torch.isnan(dw).any() and not torch.isnan(db).any()


def test_refusals_launch_nothing():
    lib = L.load()
    h, w = 8, 16
    data = _layer_data(h, w, ((64, 64), (64, 64), (32, 64), (32, 32)), seed=5)
    grads = _nan_grads(data)
    ok = _group_layers(data[:3], grads[:3])
    need = lib.bx_conv3x3_wgrad_group_workspace(ok, 3, B, h, w, L.BX_BF16)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def refused(layers, n, dtype, ws_bytes, pends=None):
        pends = pends if pends is not None else (L.WgradPending * 4)()
        before = bytes(pends)
        rc = lib.bx_conv3x3_wgrad_group(layers, n, B, h, w, dtype, ws.data_ptr(), ws_bytes, pends, _stream())
        assert rc < 0 and b"bx_conv3x3_wgrad_group" in lib.bx_last_error_string()
        assert bytes(pends) == before
        return rc

    refused(_group_layers(data, grads), 4, L.BX_BF16, need)                                     # n = 4
    narrow = _layer_data(h, w, ((16, 32),), seed=6)                                             # a layer with Ci_p = 16
    assert refused(_group_layers(data[:2] + narrow, grads[:2] + [grads[3]]), 3, L.BX_BF16, need) == -6
    assert lib.bx_conv3x3_wgrad_group_supported(3, (ctypes.c_int * 3)(64, 64, 16), (ctypes.c_int * 3)(64, 64, 32), w, L.BX_BF16) == 0
    refused(ok, 3, L.BX_F32, need)                                                              # fp32 storage
    assert refused(ok, 3, L.BX_BF16, need - 1) == -4                                            # a workspace one byte short
    inside = (L.WgradPending * 4)()
    inside[1].valid, inside[1].partial = 1, ws.data_ptr() + 256                                 # a pending inside the workspace
    refused(ok, 3, L.BX_BF16, need, inside)
    assert b"workspace" in lib.bx_last_error_string()
    torch.cuda.synchronize()
    for dw, db in grads:
        assert torch.isnan(dw).all() and torch.isnan(db).all()


BLOCKS = [((32, 64, "max"), (3, 32, 8, 16), True), ((32, 64, "max"), (2, 32, 24, 40), True), ((64, 64, "avg"), (3, 64, 16, 32), True),
          ((16, 32, "max"), (3, 16, 16, 32), False)]       # conv1 16 -> 32 is no tile-owner shape: both settings take the old path


@pytest.mark.parametrize("blk_args,xshape,grouped", BLOCKS)
def test_block_gradients_equal_with_and_without_the_group(blk_args, xshape, grouped):
    res, launches = {}, {}
    saved = (ops.WGRAD_GROUP, ops.CONV_PROFILE)
    try:
        for on in (True, False):
            ops.WGRAD_GROUP = on
            torch.manual_seed(13)
            blk = brainxai.Block(*blk_args, (2, 2), dropout_p=0.0).to(DEV).train()
            blk.compute_dtype = torch.bfloat16
            x = torch.randn(*xshape, generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_(True)
            out = blk(x)
            ops.CONV_PROFILE = prof = []
            (out.float() * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum().backward()
            ops.CONV_PROFILE = None
            launches[on] = sum(1 for e in prof if e[0] == "wgrad")
            res[on] = [x.grad] + [p.grad for _, p in sorted(blk.named_parameters())]
    finally:
        ops.WGRAD_GROUP, ops.CONV_PROFILE = saved
    torch.cuda.synchronize()
    assert launches == {True: 1 if grouped else 3, False: 3}
    assert len(res[True]) == 1 + 10 and all(g is not None for g in res[True])
    for a, b in zip(res[True], res[False]):
        assert not torch.isnan(a).any()
        assert torch.equal(a, b)
