"""GPU: Block with pooling windows other than 2x2 (the general pooling / routing kernels of csrc/tail.hip) against the oracle.

oracle.ref_torch.decision_matched_twin only knows 2x2 windows, so this file carries its own fp64 twin of the oracle Block: the
ReLU decisions are pinned from the GPU forward's kept y1, y2, y3 and the max-pool arg-max from its y3, and a bf16-storage mode
rounds at the same points as decision_matched_twin(storage=torch.bfloat16).  Whether the pinned decisions are legitimate is
checked on the way: every one the twin's own arithmetic would take the other way must be a tie at the storage resolution."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import brainxai
from brainxai import ops
from oracle import ref_torch as O
from tests.golden_util import grad_close, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3
TIGHT = 2e-4
WINDOWS = [(1, 1), (1, 2), (2, 1), 3, (4, 4), (2, 3), (4, 2)]
SHAPES = [(4, 16, 24, 36, 3), (3, 16, 50, 37, 3), (16, 32, 25, 38, 3), (4, 16, 128, 256, 8)]      # Cin, C, H, W, B


def _hw(win):
    return (win, win) if isinstance(win, int) else tuple(win)


def _windows(t, ph, pw):
    """[B, C, H, W] -> [B, C, H//ph, W//pw, ph*pw]: the floor-pool's windows, elements in row-major order"""
    B, C, H, W = t.shape
    Ho, Wo = H // ph, W // pw
    t = t[:, :, :Ho * ph, :Wo * pw].reshape(B, C, Ho, ph, Wo, pw).permute(0, 1, 2, 4, 3, 5)
    return t.reshape(B, C, Ho, Wo, ph * pw)


def _twin(ref, keep, storage=None, tie=1e-5):
    """fp64 copy of the oracle Block ``ref`` (untouched by any forward) and its forward with the GPU forward's decisions pinned"""
    twin = copy.deepcopy(ref).double()
    twin.train(ref.training)
    theirs = [a.detach().permute(0, 3, 1, 2).double().cpu() for a in keep["acts"]]
    st = (lambda t: O._StoreAs.apply(t, storage)) if storage is not None else (lambda t: t)
    stg = (lambda t: O._StoreGradAs.apply(t, storage)) if storage is not None else (lambda t: t)
    ph, pw = _hw(ref.pool.kernel_size)

    def forward(x):
        x = st(x)                                           # the fp32 input is converted to the storage type once
        y = x
        for k, conv in enumerate((twin.conv1, twin.conv2, twin.conv3)):
            z = conv(y)
            mask = theirs[k] > 0
            with torch.no_grad():
                bad = (z > 0) != mask
                assert not bool(bad.any()) or float(z.abs()[bad].max()) <= tie * float(z.abs().max()), f"conv{k + 1}: not a ReLU tie"
            y = st(z * mask.to(z.dtype))
        if isinstance(twin.pool, nn.MaxPool2d):
            idx = _windows(theirs[2], ph, pw).argmax(-1, keepdim=True)      # first maximum (torch.argmax, as ATen's pool)
            wy = _windows(y, ph, pw)
            with torch.no_grad():
                gap = wy.max(-1).values - wy.gather(-1, idx).squeeze(-1)
                assert float(gap.max()) <= tie * float(y.abs().max()), "max-pool: not a tie"
            y = wy.gather(-1, idx).squeeze(-1)
        else:
            y = st(F.avg_pool2d(y, (ph, pw)))
        y = twin.dropout(twin.bn(y))
        skip = F.interpolate(stg(x), size=y.shape[-2:], mode="bilinear", align_corners=False)
        return st(y + twin.conv1x1(skip))
    return twin, forward


def _block_pair(cin, c, kind, win, dt):
    ref = O.fill_params(O.Block(cin, c, kind, win, dropout_p=0.0), seed=7)
    mine = brainxai.Block(cin, c, kind, win, dropout_p=0.0)
    mine.load_state_dict(ref.state_dict())
    brainxai.set_compute_dtype(mine, dt)
    return ref, mine.to(DEV)


def _cos(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def _run(cin, c, h, w, b, kind, win, mode, dt):
    """(mine, ref, twin, x grads): one forward + backward of each side on the same inputs"""
    ref, mine = _block_pair(cin, c, kind, win, dt)
    ph, pw = _hw(win)
    x = O.seeded((b, cin, h, w), 15, "randn")
    r = O.seeded((b, c, h // ph, w // pw), 16, "randn")
    train = mode == "train"
    ref.train(train); mine.train(train)
    ref64 = copy.deepcopy(ref).double()
    keep = ops.keep_block_activations(mine)[""]            # {module name: dict}; the Block itself is ""
    xm = x.clone().to(DEV).requires_grad_(True)
    ym = mine(xm)
    (ym.float() * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    twin, fwd = _twin(ref, keep, storage=torch.bfloat16 if dt == torch.bfloat16 else None, tie=1e-5 if dt == torch.float32 else 1e-2)
    xt = x.double().requires_grad_(True)
    (fwd(xt) * r.double()).sum().backward()
    with torch.no_grad():
        y64 = ref64(x.double())
        y32 = ref(x)
    assert tuple(ym.shape) == (b, c, h // ph, w // pw)
    return mine, ref64, twin, ym.detach().float().cpu(), y64, y32, xm.grad, xt.grad


@pytest.mark.parametrize("win", WINDOWS, ids=str)
@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("cin,c,h,w,b", SHAPES, ids=lambda v: str(v))
def test_block_window_fp32(cin, c, h, w, b, kind, win):
    for mode in ("eval", "train"):
        label = f"{kind}{_hw(win)} {cin}->{c} {h}x{w} {mode}"
        mine, ref64, twin, ym, y64, _, gx, gt = _run(cin, c, h, w, b, kind, win, mode, torch.float32)
        assert rel_err(ym, y64) < TIGHT, label
        grad_close(gx.float().cpu(), gt, TOL, label=label + " dx")
        fl = 1e-2 * max(float(q.grad.abs().max()) for q in twin.parameters())
        for (n, p), (_, q) in zip(mine.named_parameters(), twin.named_parameters()):
            grad_close(p.grad.float().cpu(), q.grad, TOL, label=f"{label} d{n}", floor=fl)
        if mode == "train":
            assert rel_err(mine.bn.running_mean.cpu(), ref64.bn.running_mean) < TIGHT, label
            assert rel_err(mine.bn.running_var.cpu(), ref64.bn.running_var) < TIGHT, label
            assert int(mine.bn.num_batches_tracked) == 1


@pytest.mark.parametrize("win", WINDOWS, ids=str)
@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("cin,c,h,w,b", SHAPES[:2], ids=lambda v: str(v))
def test_block_window_bf16(cin, c, h, w, b, kind, win):
    for mode in ("eval", "train"):
        label = f"bf16 {kind}{_hw(win)} {cin}->{c} {h}x{w} {mode}"
        mine, _, twin, ym, _, y32, gx, gt = _run(cin, c, h, w, b, kind, win, mode, torch.bfloat16)
        assert rel_err(ym, y32) < 2e-2, label
        pairs = [("x", gx, gt)] + [(n, p.grad, q.grad) for (n, p), (_, q) in zip(mine.named_parameters(), twin.named_parameters())]
        for n, a, want in pairs:
            if want.numel() >= 1024:
                assert _cos(a, want) >= 0.998, f"{label} d{n}: cosine {_cos(a, want):.5f}"


def test_block_window_dropout():
    """p = 0.5 with a 3x3 window and the 1x1 skip zeroed: out is the dropout output alone"""
    torch.manual_seed(3)
    blk = brainxai.Block(16, 32, "max", 3, dropout_p=0.5).to(DEV).train()
    with torch.no_grad():
        blk.conv1x1.weight.zero_(); blk.conv1x1.bias.zero_()
    x = torch.randn(16, 16, 60, 60, device=DEV)
    with torch.no_grad():
        ops.manual_seed(1234, DEV); y1 = blk(x).clone()
        ops.manual_seed(1234, DEV); y2 = blk(x).clone()
        blk.dropout.p = 0.0
        y0 = blk(x).clone()
    assert y1.shape == (16, 32, 20, 20) and y1.numel() >= 10 ** 5
    assert torch.equal(y1, y2)
    assert bool((y0 != 0).all())
    dropped = y1 == 0
    assert abs(float(dropped.double().mean()) - 0.5) <= 0.01
    kept = ~dropped
    torch.testing.assert_close(y1[kept], 2 * y0[kept], rtol=2e-7, atol=0)


def _swapped(mod, dt=None):
    net = mod.build_multimodal(19, 2000, 4, dropout=0.0)
    sp = net.spectrogram_model
    sp.block1 = mod.Block(4, 16, "max", (4, 4), dropout_p=0.0)
    sp.block4 = mod.Block(64, 128, "avg", (1, 2), dropout_p=0.0)
    if dt is not None:
        sp.block1.salt, sp.block4.salt = 1, 4               # what Spectrogram_Model gives its stages
        brainxai.set_compute_dtype(net, dt)
    return net


def _model_pair(seed):
    ref = O.fill_params(_swapped(O), seed=seed)
    mine = _swapped(brainxai, torch.float32)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV)


def test_model_swapped_stages_fp32_train3():
    ref, mine = _model_pair(41)
    eeg, spec = O.seeded((4, 1, 19, 2000), 61, "randn"), O.seeded((4, 4, 128, 256), 62, "rand")
    labels = torch.softmax(O.seeded((4, 6), 63, "randn"), 1)
    e, s, lab = eeg.to(DEV), spec.to(DEV), labels.to(DEV)
    feats = {}
    hooks = [getattr(mine.spectrogram_model, f"block{i}").register_forward_hook(lambda m, i, o, k=i: feats.__setitem__(k, tuple(o.shape[-2:])))
             for i in range(1, 6)]
    ref.eval(); mine.eval()
    with torch.no_grad():
        y = mine(e, s)
        assert rel_err(y.float().cpu(), ref(eeg, spec)) < TOL
    for hk in hooks:
        hk.remove()
    assert feats == {1: (32, 64), 2: (16, 32), 3: (8, 16), 4: (8, 8), 5: (4, 4)}
    ref.train(); mine.train()
    opt_r = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    opt_m = brainxai.FlatAdamW(mine.parameters(), lr=1e-3)
    crit = brainxai.KLDivLoss()
    losses, losses_r = [], []
    pnames = {k for k, _ in ref.named_parameters()}
    try:
        for step in range(3):
            losses_r.append(O.train_step(ref, opt_r, eeg, spec, labels)[0])
            loss, _ = brainxai.train_step(mine, opt_m, e, s, lab, crit)
            losses.append(float(loss))
            if step == 0:
                # the BatchNorm statistics of the one forward both sides ran with the same weights (later ones follow the drifting
                # weights of a chaotic trajectory: block5 averages 64 values per channel here)
                for (n, t), (_, t2) in zip(mine.state_dict().items(), ref.state_dict().items()):
                    if n not in pnames:
                        assert float((t.detach().float().cpu() - t2.float()).abs().max()) <= TOL * max(1.0, float(t2.float().abs().max())), n
        assert abs(losses[0] - losses_r[0]) <= TOL * abs(losses_r[0])
        np.testing.assert_allclose(np.array(losses), np.array(losses_r), rtol=3e-2)
        for (n, t), (_, t2) in zip(mine.named_parameters(), ref.named_parameters()):
            # test_multimodal_train3's 3-step bound: 3 steps x (<= 1.05 lr per step per side) x 2 sides
            assert float((t.detach().float().cpu() - t2.float()).abs().max()) <= 6.5e-3 * max(1.0, float(t2.abs().max())), n
    finally:
        opt_m.close()
        ops.clear_grad_views()


def test_model_swapped_stages_bf16_graphed():
    def make():
        torch.manual_seed(9)
        m = _swapped(brainxai, torch.bfloat16).to(DEV).train()
        return m, brainxai.FlatAdamW(m.parameters(), lr=1e-3)
    batches = [((O.seeded((4, 1, 19, 2000), 90 + i, "randn").to(DEV), O.seeded((4, 4, 128, 256), 95 + i, "rand").to(DEV)),
                torch.softmax(O.seeded((4, 6), 99 + i, "randn"), 1).to(DEV)) for i in range(5)]
    crit = brainxai.KLDivLoss()
    try:
        m1, o1 = make(); ops.manual_seed(1234)
        eager = [float(brainxai.train_step(m1, o1, e, s, y, crit)[0]) for (e, s), y in batches]
        p1 = torch.cat([p.detach().flatten() for p in m1.parameters()]).clone()
        o1.close()
        m2, o2 = make(); ops.manual_seed(1234)
        step = brainxai.GraphedTrainStep(m2, o2, crit)
        graphed = [float(step([e, s], y)[0]) for (e, s), y in batches]
        torch.cuda.synchronize()
        p2 = torch.cat([p.detach().flatten() for p in m2.parameters()])
        assert step.enabled and len(step._graphs) == 1
        assert all(np.isfinite(eager))
        assert graphed == eager
        assert torch.equal(p1, p2)
        o2.close()
    finally:
        ops.clear_grad_views()


def test_model_swapped_stages_gradcam():
    ref, mine = _model_pair(51)
    eeg, spec = O.seeded((2, 1, 19, 2000), 52, "randn"), O.seeded((2, 4, 128, 256), 53, "rand")
    e, s = eeg.to(DEV), spec.to(DEV)
    ref.eval(); mine.eval()
    for layer in ("spectrogram_model.block1", "spectrogram_model.block4.conv3", "spectrogram_model.block5"):
        cam = brainxai.grad_cam(mine, e, s, layer, class_idx="all")
        want = O.grad_cam(ref, eeg, spec, layer, class_idx="all")
        raw = O.grad_cam(ref, eeg, spec, layer, class_idx="all", relu=False)
        assert cam.shape == want.shape == (2, 6, 128, 256), layer
        assert rel_err(cam.float().cpu(), want, floor=float(raw.abs().max())) < TOL, layer
