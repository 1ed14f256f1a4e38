"""GPU: Grad-CAM++ and Layer-CAM (grad_cam(..., method=...), GradCamSweep(method=...), bx_cam_reduce) against the definitions of
include/brainxai.h applied in fp64: on seeded activations and gradients at the kernel level, and on the oracle's own activations and
gradients (forward hook + autograd on the oracle's classes, run in fp64) end to end."""
import contextlib
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib as L
from brainxai import ops
from oracle import ref_torch as O
from tests.cam_ref import cam as cam_fp64
from tests.eeg_gradcam_setup import bn_nontrivial, rel
from tests.eeg_gradcam_setup import inputs as eeg_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3                     # north_star: 1e-3 relative fp32
EPS = 1e-6                     # part of the Grad-CAM++ definition
METHODS = ("gradcam++", "layercam")
SPEC_TARGETS = ("spectrogram_model.block5", "spectrogram_model.block5.conv3", "spectrogram_model.block3", "spectrogram_model.block1",
                "spectrogram_model.block2.conv1")
EEG_TARGETS = ("eeg_model.conv1", "eeg_model.depthwiseConv", "eeg_model.separableConv")


def _resolve(model, dotted):
    for part in dotted.split("."):
        model = getattr(model, part)
    return model


def oracle(ref64, fwd, target, class_idx, method):
    """(raw, w, out, cond) of `method` at `target` of the fp64 oracle; fwd() runs its forward.  Stacked like grad_cam's parts."""
    grabbed = {}
    h = _resolve(ref64, target).register_forward_hook(lambda _m, _i, o: grabbed.__setitem__("A", o))
    try:
        out = fwd()
    finally:
        h.remove()
    A = grabbed["A"]
    if class_idx is None:
        scores = [out.gather(1, out.argmax(1, keepdim=True)).sum()]
    elif isinstance(class_idx, str):
        scores = [out[:, c].sum() for c in range(out.shape[1])]
    else:
        scores = [out[:, int(class_idx)].sum()]
    raws, ws, conds, sgs = [], [], [], []
    for sc in scores:
        (G,) = torch.autograd.grad(sc, A, retain_graph=True)
        raw, w, cond, sg = cam_fp64(A.detach(), G, method)
        raws.append(raw); ws.append(w); conds.append(cond); sgs.append(sg)
    stack = (lambda xs: torch.stack(xs, 1)) if isinstance(class_idx, str) else (lambda xs: xs[0])
    return stack(raws), None if ws[0] is None else stack(ws), out.detach(), min(conds), max(sgs)


def _last_linear(model):
    for name in ("fc2", "dense2", "fc"):
        if hasattr(model, name):
            return getattr(model, name)
    raise AttributeError(type(model).__name__)


@contextlib.contextmanager
def _head_scaled(models, f):
    """The models' last linear layer scaled by f (a power of two: undone exactly).  Every gradient at a target flows through that
    layer, so G scales with it (the softmax's own gradient stays O(1))."""
    with torch.no_grad():
        for m in models:
            _last_linear(m).weight.mul_(f)
    try:
        yield
    finally:
        with torch.no_grad():
            for m in models:
                _last_linear(m).weight.div_(f)


def clear_scale(ref64, fwd64, target, class_idx):
    """Grad-CAM++ cancels where S G -> -2 (2 G^2 + S G^3 = G^2 (2 + S G)).  At random initialisation |S G| of the counted elements
    reaches 4 (EEG conv1) to 235 (block1) over tens of thousands of elements, so no input seed keeps every one clear of -2.  The
    fixture instead scales the last linear layer (both models) by the power of two f that brings the largest |S G| to <= 1/2: then
    2 + S G >= 1 everywhere, and the oracle asserts the margin the tests need."""
    sg = oracle(ref64, fwd64, target, class_idx, "gradcam++")[4]
    return 2.0 ** -max(0, math.ceil(math.log2(max(sg, 1e-30) / 0.5)))


# ---- kernel level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nm", [1, 6])
@pytest.mark.parametrize("HW,C", [(8192, 16), (2048, 32), (512, 64), (128, 128), (32, 256)])
@pytest.mark.parametrize("method", METHODS)
def test_cam_reduce_against_fp64_definition(method, HW, C, nm, dtype):
    B = 3
    lib = L.load()
    code = {"gradcam++": L.BX_CAM_GRADCAM_PP, "layercam": L.BX_CAM_LAYERCAM}[method]
    for seed in range(1000, 1010):                 # the first seed whose Grad-CAM++ denominators stay clear of cancellation
        g = torch.Generator().manual_seed(seed + HW + C + nm)
        A = (torch.rand(B, HW, C, generator=g) * 2.0 - 0.5).to(dtype)
        G = (torch.randn(B * nm, HW, C, generator=g) * 1e-2).to(dtype)
        G[:, ::5, ::3] = 0.0
        A64 = A.double().permute(0, 2, 1).repeat_interleave(nm, 0)                 # [B*nm, C, HW], exactly the stored values
        raw_o, w_o, cond, _ = cam_fp64(A64, G.double().permute(0, 2, 1), method)
        if cond >= 1e-2:
            break
    assert cond >= 1e-2, "no seed keeps the Grad-CAM++ denominators clear of cancellation"
    Ad, Gd = A.to(DEV).contiguous(), G.to(DEV).contiguous()
    for relu in (0, 1):
        cam = torch.empty(B * nm, HW, dtype=torch.float32, device=DEV)
        wts = torch.empty(B * nm, C, dtype=torch.float32, device=DEV) if w_o is not None else None
        L.check(lib.bx_cam_reduce(Ad.data_ptr(), Gd.data_ptr(), cam.data_ptr(), None if wts is None else wts.data_ptr(), B * nm, nm, HW, C,
                                  code, relu, ops.bx_dtype(dtype), ops._stream()), "bx_cam_reduce")
        torch.cuda.synchronize()
        want = raw_o.clamp_min(0) if relu else raw_o
        assert rel(cam, want, float(raw_o.abs().max())) <= 1e-5, (method, HW, C, nm, dtype, relu)
        if wts is not None:
            assert rel(wts, w_o) <= 1e-5
        # fixed-order sums: a second launch gives the same bits
        cam2 = torch.empty_like(cam)
        L.check(lib.bx_cam_reduce(Ad.data_ptr(), Gd.data_ptr(), cam2.data_ptr(), None, B * nm, nm, HW, C, code, relu, ops.bx_dtype(dtype),
                                  ops._stream()), "bx_cam_reduce")
        assert torch.equal(cam, cam2)


# ---- end to end against the oracle ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, dropout=0.0), seed=5)
    bn_nontrivial(ref.eeg_model, 6)
    mine = brainxai.build_multimodal(19, 2000, 4, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    return copy.deepcopy(ref).double().eval(), mine.to(DEV)


def _inputs(B, seed=11):
    return O.seeded((B, 1, 19, 2000), seed, "randn"), O.seeded((B, 4, 32, 64), seed + 1, "rand")


def _check(ref64, fwd64, mine, args, target, class_idx, method):
    f = clear_scale(ref64, fwd64, target, class_idx) if method == "gradcam++" else 1.0
    with _head_scaled((ref64, mine), f):
        raw_o, w_o, _, cond, _ = oracle(ref64, fwd64, target, class_idx, method)
        if method == "gradcam++":
            assert cond >= 1e-2, f"fixture too close to Grad-CAM++ denominator cancellation ({cond:.1e})"
        cam, raw, w, _, _ = brainxai.grad_cam(mine, *args, target, class_idx, upsample=False, return_parts=True, method=method)
        torch.cuda.synchronize()
    raw_o = raw_o.reshape(raw.shape)
    rs = float(raw_o.abs().max())
    errs = [rel(raw, raw_o), rel(cam, raw_o.clamp_min(0), rs)]
    if method == "layercam":
        assert w is None
    else:
        assert tuple(w.shape) == tuple(w_o.shape)
        errs.append(rel(w, w_o))
    assert max(errs) < TOL, (target, class_idx, method, errs)


@pytest.mark.parametrize("class_idx", [None, 3, "all"])
@pytest.mark.parametrize("target", SPEC_TARGETS + EEG_TARGETS)
@pytest.mark.parametrize("method", METHODS)
def test_methods_match_oracle(pair, method, target, class_idx):
    ref64, mine = pair
    eeg, spec = _inputs(2)
    _check(ref64, lambda: ref64(eeg.double(), spec.double()), mine, (eeg.to(DEV), spec.to(DEV)), target, class_idx, method)


@pytest.mark.parametrize("chans,samples,B", [(3, 1030, 2), (2, 40, 1)])
@pytest.mark.parametrize("method", METHODS)
def test_methods_match_oracle_ragged_and_tiny_eeg(method, chans, samples, B):
    """The EEG targets off the multiples of four (the last two geometries of test_eeg_gradcam_pool_tails_and_native_geometry in
    tests/test_gpu_eeg_gradcam.py, with its weights and inputs).  At 1030 Layer-CAM's zero tail is the two positions behind
    T1 P1 = 1028."""
    ref = O.fill_params(O.build_multimodal(chans, samples, 4, dropout=0.0), seed=7)
    bn_nontrivial(ref.eeg_model, 8)
    mine = brainxai.build_multimodal(chans, samples, 4, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    ref64, mine = copy.deepcopy(ref).double().eval(), mine.to(DEV)
    eeg, spec = eeg_inputs(B, chans, samples, seed=13)
    for target in EEG_TARGETS:
        _check(ref64, lambda: ref64(eeg.double(), spec.double()), mine, (eeg.to(DEV), spec.to(DEV)), target, "all", method)


@pytest.mark.parametrize("method", METHODS)
def test_sweep_form_matches_oracle(pair, method):
    """bx_cam_head_sweep (EEG head and up-sampling in the launch) against the fp64 maps, up-sampled the same way."""
    ref64, mine = pair
    eeg, spec = _inputs(4, seed=31)
    fwd64 = lambda: ref64(eeg.double(), spec.double())          # noqa: E731
    f = clear_scale(ref64, fwd64, "spectrogram_model.block5", "all") if method == "gradcam++" else 1.0
    with _head_scaled((ref64, mine), f):
        raw_o, _, _, cond, _ = oracle(ref64, fwd64, "spectrogram_model.block5", "all", method)
        assert cond >= 1e-2
        want = F.interpolate(raw_o.clamp_min(0).flatten(0, 1)[:, None], size=spec.shape[-2:], mode="bilinear", align_corners=False)[:, 0]
        e, s = eeg.to(DEV), spec.to(DEV)
        maps = brainxai.GradCamSweep(mine, e, s, class_idx="all", method=method)(e, s)
        torch.cuda.synchronize()
        assert rel(maps.flatten(0, 1), want, float(raw_o.abs().max())) < TOL


@pytest.mark.parametrize("method", METHODS)
def test_standalone_nets(method):
    ref_net = O.fill_params(O.EEGNetAttentionDeep(6, Chans=19, Samples=2048, dropoutRate=0.0), seed=21)
    bn_nontrivial(ref_net, 22)
    mine = brainxai.EEGNetAttentionDeep(6, Chans=19, Samples=2048, dropoutRate=0.0)
    mine.load_state_dict(ref_net.state_dict())
    mine.to(DEV)
    ref64 = copy.deepcopy(ref_net).double().eval()
    eeg = O.seeded((2, 1, 19, 2048), 23, "randn")
    for target in ("conv1", "depthwiseConv", "separableConv"):
        for class_idx in (None, "all"):
            _check(ref64, lambda: ref64(eeg.double()), mine, (eeg.to(DEV), None), target, class_idx, method)
    sref = O.fill_params(O.Spectrogram_Model(6, in_channels=4), seed=25)
    smine = brainxai.Spectrogram_Model(6, in_channels=4)
    smine.load_state_dict(sref.state_dict())
    smine.to(DEV)
    sref64 = copy.deepcopy(sref).double().eval()
    spec = O.seeded((2, 4, 32, 64), 27, "rand")
    for target in ("block2", "block4.conv2"):
        _check(sref64, lambda: sref64(spec.double()), smine, (None, spec.to(DEV)), target, "all", method)


# ---- bf16 storage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_bf16_storage_against_fp32_storage(method):
    """The default target in bf16 storage against the same method in fp32 storage, on the fp32 maps' scale.

    Derived bound.  raw[p] = sum_k w'_k A[p,k], w' = the method's transform of the Grad-CAM weight w (include/brainxai.h,
    bx_cam_head).  bf16 storage rounds every stored activation to 8 significand bits: the stage output A arrives with an error of
    dA = eps_A max|A| and w (computed from A's average through the fp32 heads) with one of dw = eps_w max|w|, both measured here from
    the two storages' own parts (A and the Grad-CAM weights of return_parts; eps_A is asserted <= 2^-7, the bound
    test_bf16_gradcam_sweep_against_fp32_oracle asserts for the same stage output).  To first order
        |d raw[p]| <= dA sum_k |w'_k| + sum_k |dw'_k| |A[p,k]|,   |dw'_k| <= |dw'/dw|_k dw + |dw'/dS|_k HW dA   (S = HW gap),
    with the derivatives of the method's transform taken from the oracle in fp64: Layer-CAM dw'/dw = 1 (w > 0), dw'/dS = 0;
    Grad-CAM++ w' = HW w^3 / den, den = 2 w^2 + S w^3 + 1e-6, dw'/dw = HW (3 w^2 den - w^3 (4 w + 3 S w^2)) / den^2 and
    dw'/dS = -HW w^6 / den^2 -- both grow as den cancels, so the bound carries the fixture's own cancellation.  The bound is
    evaluated per position of every map and its largest value, over max|raw|, is the tolerance (x 1.25 for second-order terms)."""
    g = torch.Generator().manual_seed(4243)
    n = 8
    spec = torch.rand(n, 4, 64, 128, generator=g)
    eeg = torch.randn(n, 1, 19, 2000, generator=g)
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, dropout=0.0), seed=5).eval()
    parts = {}
    for dt in (torch.float32, torch.bfloat16):
        mine = brainxai.build_multimodal(19, 2000, 4, dropout=0.0, compute_dtype=dt)
        mine.load_state_dict(ref.state_dict())
        mine.to(DEV).eval()
        e, s = eeg.to(DEV), spec.to(DEV)
        _, raw, _, _, _ = brainxai.grad_cam(mine, e, s, class_idx="all", upsample=False, return_parts=True, method=method)
        _, _, w, A, _ = brainxai.grad_cam(mine, e, s, class_idx="all", upsample=False, return_parts=True)
        parts[dt] = (raw.double().cpu(), w.double().cpu(), A.double().cpu())           # A [n, HW, C] channels-last
    raw32, w32, A32 = parts[torch.float32]
    eps_A = float((parts[torch.bfloat16][2] - A32).abs().max() / A32.abs().max())
    eps_w = float((parts[torch.bfloat16][1] - w32).abs().max() / w32.abs().max())
    assert eps_A <= 2.0 ** -7
    ref64 = copy.deepcopy(ref).double()
    grabbed = {}
    h = ref64.spectrogram_model.block5.register_forward_hook(lambda _m, _i, o: grabbed.__setitem__("A", o))
    out = ref64(eeg.double(), spec.double())
    h.remove()
    A = grabbed["A"].detach().flatten(2)                            # [n, C, HW]
    HW = A.shape[2]
    dA, bound = eps_A * float(A.abs().max()), 0.0
    scale = float(raw32.abs().max())
    for c in range(out.shape[1]):
        (G,) = torch.autograd.grad(out[:, c].sum(), grabbed["A"], retain_graph=True)
        wv = G.flatten(2).mean(2)                                   # [n, C]: the gradient is the same at every position
        S = A.sum(2)
        dw = eps_w * float(wv.abs().max())
        pos = (wv > 0).double()
        if method == "layercam":
            wp, d_w, d_S = wv.clamp_min(0), pos, torch.zeros_like(wv)
        else:
            den = 2 * wv ** 2 + S * wv ** 3 + EPS
            wp = pos * HW * wv ** 3 / den
            d_w = pos * HW * (3 * wv ** 2 * den - wv ** 3 * (4 * wv + 3 * S * wv ** 2)) / den ** 2
            d_S = pos * HW * wv ** 6 / den ** 2
        dwp = d_w.abs() * dw + d_S.abs() * HW * dA                  # [n, C]
        per_pos = dA * wp.abs().sum(1, keepdim=True) + (dwp[:, :, None] * A.abs()).sum(1)
        bound = max(bound, float(per_pos.max()))
    tol = 1.25 * bound / scale
    err = float((parts[torch.bfloat16][0] - raw32).abs().max()) / scale
    print(f"{method} bf16 vs fp32 storage: {err:.2e} <= {tol:.2e} (eps_A {eps_A:.1e}, eps_w {eps_w:.1e})")
    assert err <= tol


# ---- sweep replay and state -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_sweep_equals_eager_bit_for_bit(pair, method):
    _, mine = pair
    eeg, spec = (t.to(DEV) for t in _inputs(8, seed=41))
    sweep = brainxai.GradCamSweep(mine, eeg, spec, class_idx="all", method=method)
    for b in (8, 3):                                       # a full batch, then a ragged last batch (its own capture)
        e, s = eeg[:b].contiguous(), spec[:b].contiguous()
        got = sweep(e, s).clone()
        want = brainxai.grad_cam(mine, e, s, class_idx="all", method=method)
        torch.cuda.synchronize()
        assert got.shape == want.shape and torch.equal(got, want), (method, b)
    # and the methods are different maps
    g0 = brainxai.grad_cam(mine, eeg, spec, class_idx="all")
    assert not torch.equal(g0, brainxai.grad_cam(mine, eeg, spec, class_idx="all", method=method))


@pytest.mark.parametrize("target", ["spectrogram_model.block5", "spectrogram_model.block3", "eeg_model.conv1"])
@pytest.mark.parametrize("method", METHODS)
def test_state_restored(pair, method, target):
    _, mine = pair
    eeg, spec = (t.to(DEV) for t in _inputs(2, seed=51))
    mine.train()
    mine.fc1.weight.requires_grad_(False)
    try:
        flags = [p.requires_grad for p in mine.parameters()]
        brainxai.grad_cam(mine, eeg, spec, target, method=method)
        assert mine.training and all(m.training for m in mine.modules())
        assert [p.requires_grad for p in mine.parameters()] == flags
    finally:
        mine.fc1.weight.requires_grad_(True)
        mine.eval()
