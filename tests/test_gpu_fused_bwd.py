"""GPU: stage 1's fused backward (bx_conv3x3_bwd_fused, k_conv_mfma_bwd) against the entry points it replaces, called directly on the
same bf16 operands: the data gradient (bx_conv3x3 with the ReLU mask) must be bit-identical, the weight and bias gradients
(bx_conv3x3_wgrad) equal up to fp32 reassociation -- checked against the unfused result and against an fp64 sum of the same operands."""
import ctypes

import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import ops
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5


def _operands(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    xl = torch.randn(B, H, W, 16, generator=g)
    xl[torch.rand(B, H, W, 16, generator=g) < 0.3] = 0.0          # positive, negative and zero activations: every mask decision
    dz = torch.randn(B, H, W, 16, generator=g)
    x0 = torch.zeros(B, H, W, 8)
    x0[..., :4] = torch.rand(B, H, W, 4, generator=g)              # the padded 4-plane block input
    w = torch.randn(16, 16, 3, 3, generator=g) / 12
    bf = lambda t: t.to(DEV).to(torch.bfloat16).contiguous()        # noqa: E731
    return bf(xl), bf(dz), bf(x0), w.to(DEV)


def _dgrad(dz, xl, pm):
    B, H, W, _ = dz.shape
    out = torch.full_like(dz, 7.0)
    L.check(L.load().bx_conv3x3(dz.data_ptr(), None, pm.data_ptr(), None, xl.data_ptr(), None, out.data_ptr(), B, H, W, 16, 16, L.BX_BF16, 0,
                                L.BX_ALGO_MFMA, 0), "bx_conv3x3")
    return out


def _wgrad(x, dz, cin):
    lib = L.load()
    B, H, W, cip = x.shape
    need = lib.bx_conv3x3_wgrad_workspace(B, H, W, cip, 16, L.BX_BF16, L.BX_ALGO_MFMA)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dw, db = torch.full((16, cin, 3, 3), float("nan"), device=DEV), torch.full((16,), float("nan"), device=DEV)
    L.check(lib.bx_conv3x3_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H, W, cin, cip, 16, L.BX_BF16, L.BX_ALGO_MFMA,
                                 ws.data_ptr(), ws.numel(), 0), "bx_conv3x3_wgrad")
    return dw, db


def _wgrad_f64(x, dz, cin):
    """dW[o][i][dy][dx] = sum_p x[p + (dy-1, dx-1)][i] dz[p][o] and db = sum_p dz[p] in fp64, nine per-tap matrix products"""
    B, H, W, _ = x.shape
    xp = torch.nn.functional.pad(x.double()[..., :cin], (0, 0, 1, 1, 1, 1))
    d = dz.double().reshape(-1, 16)
    dw = torch.empty(16, cin, 3, 3, dtype=torch.float64, device=DEV)
    for dy in range(3):
        for dx in range(3):
            dw[:, :, dy, dx] = (xp[:, dy:dy + H, dx:dx + W, :].reshape(-1, cin).t() @ d).t()
    return dw, d.sum(0)


def _fused(dz, xl, pm, x0=None, pending=None, cin0=4):
    lib = L.load()
    B, H, W, _ = dz.shape
    need = lib.bx_conv3x3_bwd_fused_workspace(B, H, W, 1 if x0 is not None else 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)        # noqa: E731
    dw, db = nan(16, 16, 3, 3), nan(16)
    dw0, db0 = (nan(16, cin0, 3, 3), nan(16)) if x0 is not None else (None, None)
    dzo = torch.full_like(dz, 7.0) if x0 is None else None
    p = lambda t: None if t is None else t.data_ptr()               # noqa: E731
    L.check(lib.bx_conv3x3_bwd_fused(dz.data_ptr(), xl.data_ptr(), pm.data_ptr(), p(dzo), p(x0), dw.data_ptr(), db.data_ptr(), p(dw0), p(db0),
                                     B, H, W, cin0, ws.data_ptr(), ws.numel(), ctypes.byref(pending) if pending is not None else None, 0),
            "bx_conv3x3_bwd_fused")
    return dzo, dw, db, dw0, db0, ws


SHAPES = [(64, 128, 256), (3, 20, 45), (2, 13, 70)]                 # the benchmark's stage 1; partial edge tiles in both directions


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_layer_matches_unfused_entry_points(B, H, W):
    """F3 form: dZ_{L-1} stored, bit for bit what bx_conv3x3 with the activation mask stores; dW / db to fp32 reassociation"""
    xl, dz, _, w = _operands(B, H, W, B + H + W)
    pm = ops._pack(w, True, torch.bfloat16)[1]
    want = _dgrad(dz, xl, pm)
    rw, rb = _wgrad(xl, dz, 16)
    dzo, dw, db, _, _, _ = _fused(dz, xl, pm)
    torch.cuda.synchronize()
    assert torch.equal(dzo.view(torch.int16), want.view(torch.int16))
    assert 0.2 < float((dzo != 0).float().mean()) < 0.8                 # the mask did act
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL
    fw, fb = _wgrad_f64(xl, dz, 16)
    assert rel_err(dw.double(), fw) <= TOL and rel_err(db.double(), fb) <= TOL


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_fused_conv2_form_takes_conv1_weight_gradient(B, H, W):
    """W1 form (block input without a gradient): dZ1 is not stored; conv2's dW / db and conv1's dW0 / db0 (4 logical of 8 padded
    input channels) against bx_conv3x3_wgrad on the unfused dZ1, and against fp64 sums; both summed by the call's one reduce launch"""
    xl, dz, x0, w = _operands(B, H, W, 3 * B + H)
    pm = ops._pack(w, True, torch.bfloat16)[1]
    dz1 = _dgrad(dz, xl, pm)
    rw, rb = _wgrad(xl, dz, 16)
    rw0, rb0 = _wgrad(x0, dz1, 4)
    pend = L.WgradPending()
    dzo, dw, db, dw0, db0, _ = _fused(dz, xl, pm, x0=x0, pending=pend)
    assert dzo is None and pend.valid == 0
    torch.cuda.synchronize()
    assert rel_err(dw, rw) <= TOL and rel_err(db, rb) <= TOL
    assert rel_err(dw0, rw0) <= TOL and rel_err(db0, rb0) <= TOL
    fw, fb = _wgrad_f64(xl, dz, 16)
    fw0, fb0 = _wgrad_f64(x0, dz1, 4)
    assert rel_err(dw.double(), fw) <= TOL and rel_err(db.double(), fb) <= TOL
    assert rel_err(dw0.double(), fw0) <= TOL and rel_err(db0.double(), fb0) <= TOL


def test_fused_chain_carries_the_pending_sum_and_ends_in_one_reduce():
    """conv3's launch leaves its partials pending; conv2's launch sums them in its front workgroups and ends the chain with one
    two-job reduce: dW3 is still unsummed after the first call, everything is summed after the second"""
    B, H, W = 4, 24, 70
    x2, dz3, x0, w3 = _operands(B, H, W, 21)
    x1, _, _, w2 = _operands(B, H, W, 22)
    p3, p2 = ops._pack(w3, True, torch.bfloat16)[1], ops._pack(w2, True, torch.bfloat16)[1]
    pend = L.WgradPending()
    dz2, dw3, db3, _, _, ws3 = _fused(dz3, x2, p3, pending=pend)
    assert pend.valid == 1
    torch.cuda.synchronize()
    assert torch.isnan(dw3).all() and torch.isnan(db3).all()
    _, dw2, db2, dw1, db1, _ = _fused(dz2, x1, p2, x0=x0, pending=pend)
    assert pend.valid == 0
    torch.cuda.synchronize()
    dz1 = _dgrad(dz2, x1, p2)
    for got, want in (((dw3, db3), _wgrad(x2, dz3, 16)), ((dw2, db2), _wgrad(x1, dz2, 16)), ((dw1, db1), _wgrad(x0, dz1, 4))):
        assert rel_err(got[0], want[0]) <= TOL and rel_err(got[1], want[1]) <= TOL
    del ws3


def test_fused_refuses_its_own_pending_workspace():
    B, H, W = 2, 16, 32
    xl, dz, _, w = _operands(B, H, W, 5)
    pm = ops._pack(w, True, torch.bfloat16)[1]
    pend = L.WgradPending()
    dzo, dw, db, _, _, ws = _fused(dz, xl, pm, pending=pend)
    rc = L.load().bx_conv3x3_bwd_fused(dz.data_ptr(), xl.data_ptr(), pm.data_ptr(), dzo.data_ptr(), None, dw.data_ptr(), db.data_ptr(), None,
                                       None, B, H, W, 0, ws.data_ptr(), ws.numel(), ctypes.byref(pend), 0)
    assert rc != 0
    L.check(L.load().bx_conv3x3_wgrad_finish(ctypes.byref(pend), 0), "finish")
    torch.cuda.synchronize()


@pytest.mark.parametrize("input_grad", [False, True])
def test_stage1_block_backward_matches_unfused_path(input_grad):
    """A stage-1 Block (4 planes -> 16, bf16) forward + backward: the fused path against the same Block with activations kept
    (ops.keep_block_activations: the debugging hook takes the unfused kernels).  The block input without a gradient takes the W1
    form; with one, conv2's launch stores dZ1 for conv1's data gradient."""
    res = {}
    for keep in (False, True):
        torch.manual_seed(3)
        blk = brainxai.Block(4, 16, "max", (2, 2), dropout_p=0.0).to(DEV).train()
        blk.compute_dtype = torch.bfloat16
        if keep:
            ops.keep_block_activations(blk)
        x = torch.rand(4, 4, 64, 96, generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_(input_grad)
        out = blk(x)
        (out.float() * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum().backward()
        res[keep] = (out.detach().float(), x.grad.clone() if input_grad else None, {n: p.grad.clone() for n, p in blk.named_parameters()})
    torch.cuda.synchronize()
    assert torch.equal(res[False][0], res[True][0])
    if input_grad:
        assert rel_err(res[False][1], res[True][1]) <= TOL
    for n, g in res[True][2].items():
        assert rel_err(res[False][2][n], g) <= TOL, n
