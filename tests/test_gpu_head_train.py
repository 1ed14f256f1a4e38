"""The training head in one native call (bx_mm_head_train: forward, KL-divergence loss and its gradient, input half of the
backward in ONE launch; parameter gradients and the loss value in a second) against the three entries it replaces --
bx_mm_head_fwd, bx_kldiv_fwd_bwd, bx_mm_head_bwd -- on the same inputs.  Those are held against the fp64 oracle by
tests/test_gpu_heads.py; here every comparison is torch.equal: both paths run the same device functions, so no bit may move.

Shapes are the smallest that reach each code path and ragged edge (csrc/heads.hip):
  B 1 / 3 / 9         below, and above but not a multiple of, the 8-sample unroll of k_mm_head_bwd_w
  HW 5 / 32 / 40      the GAP loop loads 32 pixels per trip: a tail alone, one full trip, a full trip and a tail
  N 6, K 992, C 256, Hd 128    the shipped head: FAST forward, register-prefetch backward
  N 3, C 64, Hd 16    fewer rows than waves, threads beyond C and Hd
  N 8                 leaves the FAST forward (2N > 12), keeps the prefetch backward
  K 1030 / C 320      leave the register-prefetch backward (K 1030 the FAST forward as well)
"""
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RED = {"mean": 0, "batchmean": 1, "sum": 2}

# (B, H, W, N, K, C, Hd)
SHAPES = [(1, 1, 5, 6, 992, 256, 128), (3, 4, 8, 6, 992, 256, 128), (9, 1, 5, 6, 992, 256, 128), (9, 4, 8, 6, 992, 256, 128),
          (3, 1, 5, 3, 992, 64, 16), (9, 4, 8, 3, 992, 64, 16), (9, 1, 5, 8, 992, 256, 128), (3, 1, 5, 6, 1030, 256, 128),
          (9, 1, 5, 6, 992, 320, 128), (3, 5, 8, 6, 992, 256, 128), (3, 5, 8, 8, 992, 256, 128)]


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(shape, dt, seed=0):
    B, H, W, N, K, C, Hd = shape
    g = torch.Generator().manual_seed(1000 + seed)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a
    feat = torch.rand(B, H, W, C, generator=g).to(dt)
    ef = torch.randn(B, K, generator=g)
    params = (u(N, C, a=4 * (6.0 / C) ** 0.5), u(N, a=0.1), u(N, K, a=(6.0 / K) ** 0.5), u(N, a=0.1),
              u(Hd, 2 * N, a=(3.0 / N) ** 0.5), u(Hd, a=0.1), u(N, Hd, a=(6.0 / Hd) ** 0.5), u(N, a=0.1))
    target = torch.softmax(torch.randn(B, N, generator=g), 1)
    target[torch.rand(B, N, generator=g) < 0.3] = 0.0                  # exact zeros: the `t > 0` branch of the loss
    target[0, 0] = 0.0
    return tuple(t.to(DEV).contiguous() for t in (feat, ef, *params, target))


def _buffers(shape, dt):
    """every output of either path, NaN-filled: (gap, slp, elp, hidden, logp, loss, dlogp, dfeat, def, 8 parameter gradients)"""
    B, H, W, N, K, C, Hd = shape
    nan = lambda *s, d=torch.float32: torch.full(s, float("nan"), dtype=d, device=DEV)
    return [nan(B, C), nan(B, N), nan(B, N), nan(B, Hd), nan(B, N), nan(1), nan(B, N), nan(B, H, W, C, d=dt), nan(B, K),
            nan(N, C), nan(N), nan(N, K), nan(N), nan(Hd, 2 * N), nan(Hd), nan(N, Hd), nan(N)]


NAMES = ["gap", "spec_logp", "eeg_logp", "hidden", "logp", "loss", "dlogp", "dfeat", "d_eeg_feat",
         "d_fc_w", "d_fc_b", "d_dense_w", "d_dense_b", "dw1", "db1", "dw2", "db2"]


def _separate(shape, dt, args, red, gs):
    B, H, W, N, K, C, Hd = shape
    feat, ef, fcw, fcb, dw, db, w1, b1, w2, b2, target = args
    lib = L.load()
    out = _buffers(shape, dt)
    gap, slp, elp, hidden, logp, loss, dlogp, dfeat, def_ = out[:9]
    ws = torch.empty(lib.bx_mm_head_workspace(B, N, Hd), dtype=torch.uint8, device=DEV)
    L.check(lib.bx_mm_head_fwd(_p(feat), _p(ef), _p(fcw), _p(fcb), _p(dw), _p(db), _p(w1), _p(b1), _p(w2), _p(b2), _p(gap), _p(slp), _p(elp),
                               _p(hidden), _p(logp), B, H * W, C, K, N, Hd, ops.bx_dtype(dt), _stream()), "bx_mm_head_fwd")
    L.check(lib.bx_kldiv_fwd_bwd(_p(logp), _p(target), _p(loss), _p(dlogp), B, N, RED[red], gs, _stream()), "bx_kldiv_fwd_bwd")
    L.check(lib.bx_mm_head_bwd(_p(dlogp), _p(logp), _p(hidden), _p(slp), _p(elp), _p(gap), _p(ef), _p(fcw), _p(dw), _p(w1), _p(w2),
                               _p(dfeat), _p(def_), *[_p(t) for t in out[9:]], _p(ws), ws.numel(), B, H * W, C, K, N, Hd, ops.bx_dtype(dt),
                               _stream()), "bx_mm_head_bwd")
    torch.cuda.synchronize()
    return out


def _fused(shape, dt, args, red, gs, out=None, ws=None):
    B, H, W, N, K, C, Hd = shape
    feat, ef, fcw, fcb, dw, db, w1, b1, w2, b2, target = args
    lib = L.load()
    out = _buffers(shape, dt) if out is None else out
    gap, slp, elp, hidden, logp, loss, dlogp, dfeat, def_ = out[:9]
    ws = torch.empty(lib.bx_mm_head_workspace(B, N, Hd), dtype=torch.uint8, device=DEV) if ws is None else ws
    L.check(lib.bx_mm_head_train(_p(feat), _p(ef), _p(fcw), _p(fcb), _p(dw), _p(db), _p(w1), _p(b1), _p(w2), _p(b2), _p(target), _p(gap),
                                 _p(slp), _p(elp), _p(hidden), _p(logp), _p(loss), _p(dlogp), _p(dfeat), _p(def_), *[_p(t) for t in out[9:]],
                                 _p(ws), ws.numel(), B, H * W, C, K, N, Hd, RED.get(red, red), gs, ops.bx_dtype(dt), _stream()), "bx_mm_head_train")
    torch.cuda.synchronize()
    return out


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert not torch.isnan(b.float()).any(), f"{what}: the separate launches left NaN in {name}"
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} of {a.numel()} entries, " \
                                  f"max |diff| {float((a.float() - b.float()).abs().max()):.3e}"


@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("red", ["mean", "batchmean", "sum"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_HW%d_N%d_K%d_C%d_Hd%d" % (s[0], s[1] * s[2], s[3], s[4], s[5], s[6]))
def test_train_head_equals_the_three_entries(shape, dt, red, gs):
    args = _case(shape, dt)
    assert int((args[-1] == 0).sum()) > 0
    _same(_fused(shape, dt, args, red, gs), _separate(shape, dt, args, red, gs), f"{shape} {dt} {red} {gs}")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_train_head_pooling_over_more_than_one_trip(dt):
    """HW = 40: a full trip of 32 pixels and a tail of 8.  Both paths share the pooling loop, so equality between them says nothing
    about it: the pooled map is held against the fp64 mean.  Bound: the HW adds each round a partial sum below HW (values in [0, 1))
    by at most 2^-24 of it, the product with 1 / HW rounds twice more, so |gap - mean| <= (HW + 2) * 2^-24."""
    shape = (3, 5, 8, 6, 992, 256, 128)
    args = _case(shape, dt, seed=3)
    gap = _fused(shape, dt, args, "mean", 1.0)[0]
    want = args[0].double().mean(dim=(1, 2))
    err = float((gap.double() - want).abs().max())
    print(f"pooled map over HW = 40, {dt}: max |gap - fp64 mean| = {err:.3e}")
    assert err <= 42 * 2.0 ** -24


def test_train_head_three_calls_on_the_same_buffers():
    """nothing is left over between calls: same buffers, same workspace, identical bits each time"""
    shape, dt = (9, 4, 8, 6, 992, 256, 128), torch.bfloat16
    args = _case(shape, dt, seed=1)
    want = _separate(shape, dt, args, "mean", 1.0)
    out = _buffers(shape, dt)
    ws = torch.empty(L.load().bx_mm_head_workspace(9, 6, 128), dtype=torch.uint8, device=DEV)
    for call in range(3):
        _fused(shape, dt, args, "mean", 1.0, out=out, ws=ws)
        _same(out, want, f"call {call}")


def test_train_head_optional_outputs():
    """dlogp, the feature gradients, the loss and any parameter gradient may be NULL; what is asked for keeps its bits"""
    shape, dt = (3, 1, 5, 6, 992, 256, 128), torch.float32
    args = _case(shape, dt, seed=2)
    want = _separate(shape, dt, args, "batchmean", 1.0)
    B, H, W, N, K, C, Hd = shape
    feat, ef, fcw, fcb, dw, db, w1, b1, w2, b2, target = args
    lib = L.load()
    for drop in ({5, 6, 7, 8}, set(range(9, 17)), {5} | set(range(9, 17)), {9, 12, 14}):
        out = _buffers(shape, dt)
        ptr = [None if i in drop else _p(t) for i, t in enumerate(out)]
        ws = torch.empty(lib.bx_mm_head_workspace(B, N, Hd), dtype=torch.uint8, device=DEV)
        L.check(lib.bx_mm_head_train(_p(feat), _p(ef), _p(fcw), _p(fcb), _p(dw), _p(db), _p(w1), _p(b1), _p(w2), _p(b2), _p(target),
                                     *ptr, _p(ws), ws.numel(), B, H * W, C, K, N, Hd, 1, 1.0, ops.bx_dtype(dt), _stream()), "bx_mm_head_train")
        torch.cuda.synchronize()
        for i, (name, a, b) in enumerate(zip(NAMES, out, want)):
            if i in drop:
                assert torch.isnan(a.float()).all(), f"{name} was not asked for but written"
            else:
                assert torch.equal(a, b), name


def test_train_head_refusals():
    shape, dt = (3, 1, 5, 6, 992, 256, 128), torch.float32
    args = _case(shape, dt)
    with pytest.raises(RuntimeError, match="reduction"):
        _fused(shape, dt, args, 3, 1.0)
    with pytest.raises(RuntimeError, match="workspace"):
        _fused(shape, dt, args, "mean", 1.0, ws=torch.empty(16, dtype=torch.uint8, device=DEV))


# ---- plumbing: the training step forms with the switch on and off ----------------------------------------------------------------
def _small_step_run(fused, graphed, dt):
    """two (eager) or three (eager, captured, replayed) steps of a small multimodal model from one seed"""
    g = torch.Generator().manual_seed(5)
    eeg = torch.randn(4, 1, 19, 2000, generator=g).to(DEV)
    spec = torch.rand(4, 4, 32, 64, generator=g).to(DEV)
    labels = torch.softmax(torch.randn(4, 6, generator=g), 1)
    labels[0, 1] = 0.0
    labels = labels.to(DEV)
    old = ops.HEAD_FUSED
    ops.HEAD_FUSED = fused
    try:
        torch.manual_seed(21)
        net = brainxai.build_multimodal(19, 2000, 4, dropout=0.5, compute_dtype=dt).to(DEV).train()
        opt = brainxai.FlatAdamW(net.parameters(), lr=1e-3)
        crit = brainxai.KLDivLoss()
        ops.manual_seed(99)
        assert net.can_forward_loss(crit) == fused
        res = []
        if graphed:
            step = brainxai.GraphedTrainStep(net, opt, crit, strict=True)
            for _ in range(3):
                loss, out = step([eeg, spec], labels)
                res.append((loss.clone(), out.clone()))
            assert step.enabled and len(step._graphs) == 1
        else:
            for _ in range(2):
                loss, out = brainxai.train_step(net, opt, eeg, spec, labels, crit)
                res.append((loss.clone(), out.clone()))
        torch.cuda.synchronize()
        return res, opt.flat_p.clone(), [p.detach().clone() for p in net.parameters()]
    finally:
        ops.HEAD_FUSED = old
        ops.clear_grad_views()


@pytest.mark.parametrize("graphed", [False, True], ids=["train_step", "graphed"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_training_steps_with_the_switch_on_and_off(dt, graphed):
    on, off = _small_step_run(True, graphed, dt), _small_step_run(False, graphed, dt)
    for i, ((l1, o1), (l0, o0)) in enumerate(zip(on[0], off[0])):
        assert torch.equal(l1, l0), f"step {i}: loss {float(l1)!r} vs {float(l0)!r}"
        assert torch.equal(o1, o0), f"step {i}: log-probabilities differ"
    assert torch.equal(on[1], off[1])
    for a, b in zip(on[2], off[2]):
        assert torch.equal(a, b)


def test_forward_loss_only_where_it_may_replace_the_launches():
    torch.manual_seed(3)
    net = brainxai.build_multimodal(19, 2000, 4, dropout=0.0).to(DEV).train()
    crit = brainxai.KLDivLoss("batchmean")
    assert net.can_forward_loss(crit)
    assert not net.can_forward_loss(torch.nn.KLDivLoss(reduction="batchmean"))
    with torch.no_grad():
        assert not net.can_forward_loss(crit)
    net.eval()
    assert not net.can_forward_loss(crit)
    net.train()
    for mod in (net.fc1, net.fc2, net, crit):
        h = mod.register_forward_hook(lambda *a: None)
        assert not net.can_forward_loss(crit)
        h.remove()
    h = net.fc2.register_full_backward_hook(lambda *a: None)
    assert not net.can_forward_loss(crit)
    h.remove()
    assert net.can_forward_loss(crit)
    with pytest.raises(RuntimeError, match="forward_loss"):
        net.forward_loss(torch.zeros(1, 1, 19, 2000, device=DEV), torch.zeros(1, 4, 32, 64, device=DEV), torch.zeros(1, 6, device=DEV),
                         torch.nn.KLDivLoss())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_forward_loss_with_another_upstream_gradient(dt):
    """(2 * loss).backward(): the upstream gradient is not the cached unit -- same gradients as the separate launches give for it"""
    g = torch.Generator().manual_seed(6)
    eeg = torch.randn(3, 1, 19, 2000, generator=g).to(DEV)
    spec = torch.rand(3, 4, 32, 64, generator=g).to(DEV)
    labels = torch.softmax(torch.randn(3, 6, generator=g), 1).to(DEV)
    torch.manual_seed(8)
    net = brainxai.build_multimodal(19, 2000, 4, dropout=0.0, compute_dtype=dt).to(DEV).train()
    crit = brainxai.KLDivLoss("sum")
    grads = []
    for fused in (True, False):
        net.zero_grad(set_to_none=True)
        if fused:
            loss, out = net.forward_loss(eeg, spec, labels, crit)
        else:
            out = net(eeg, spec)
            loss = crit(out, labels)
        (loss * 2.0).backward()
        torch.cuda.synchronize()
        grads.append((loss.detach().clone(), out.detach().clone(), [p.grad.clone() for p in net.parameters()]))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    for (n, _), a, b in zip(net.named_parameters(), grads[0][2], grads[1][2]):
        assert torch.equal(a, b), n
