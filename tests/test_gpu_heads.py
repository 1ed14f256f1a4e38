"""GPU: the classifier heads, the KL loss and the last-stage Grad-CAM at class counts other than six.

The head kernels choose their code path by the class count N (csrc/heads.hip):
    N <= 6        fused multimodal head, FAST register path (2N <= 12, K <= 1024, C <= 1024)
    7 <= N <= 16  fused head, general path (models.MultimodalModel._fusable: fc1 width * 2N <= 4096)
    17 <= N <= 32 three separate ops (bx_gap_fc_lsm_*, bx_linear_lsm_*, bx_fusion_head_*)
    N > 32        refused (HEAD_MAX_N); bx_gradcam_head alone accepts N <= 64
and N sets the trip counts and guards inside each kernel (the unrolled HEAD_MAX_N loops of lsm_bwd_row, the four waves of
k_linear_lsm_fwd, the 8-wide class steps of k_gradcam_head, the grid's y extent under class mode "all").  NS below puts a class
count on each side of every one of those boundaries.  Every head is compared with an fp64 torch restatement of the same operation.

Tolerances (fp32 arithmetic, unit roundoff u = 6e-8):
  OP_TOL = 1e-4  a K-term fp32 dot product accumulates rounding like a random walk, sqrt(K) u = 2.3e-6 at K = 1488 relative to
                 the sum of |terms|; the forward rounds logp = z - lse at |z| up to ~50 (confident regime), 4e-6 relative in every
                 p_j.  Where a result is a cancelling sum of such terms the error is measured against a smaller value: at N = 2
                 each logit-gradient row is (g, -g), and the bias gradient summed over 3 samples came out 6.9e-5 from fp64 on the
                 device (the fusion head's input gradient, a sum over 128 hidden units, 2.2e-5); every other case stayed below
                 2e-5.  The largest error per head and N is printed by test_zz_heads_report (GPU log).  The planted bugs this file
                 must catch (a capped row loop, an unguarded 0 * log 0, the cancelling 1 - p backward, an off-by-one class guard)
                 move the result by 1e-1 or more, or to NaN.
  bf16 storage   the features are rounded to bf16 first and the fp64 reference gets the same rounded values, so the comparison
                 measures the kernel's fp32 arithmetic only (OP_TOL); a gradient STORED as bf16 may sit one bf16 ulp from the
                 fp64 value (round to nearest of an fp32 result that itself carries ~1e-7 relative error can cross a rounding
                 boundary), plus OP_TOL of the tensor's scale where an element is small against the dot product it came from.
  MODEL_TOL      the model-level cases are held to the tolerances tests/test_gpu_parity.py holds the N = 6 model to.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib as L
from brainxai import explain, ops
from oracle import ref_torch as O
from tests.cam_ref import _fusion_ref, _gen, _lsm, _uniform          # (the fp64 LogSoftmax whose backward does not cancel lives there)
from tests.golden_util import grad_close, matched_oracle, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NS = (1, 2, 3, 6, 7, 8, 16, 17, 32)
OP_TOL = 1e-4
TIGHT = 2e-4            # fp32 product against the fp64 oracle, whole model (tests/test_gpu_parity.py)
MODEL_TOL = 1e-3        # north_star: 1e-3 relative fp32 (parameter gradients on the scale of the model's largest)
CONFIDENT = 45.0        # the confident regime's smallest lead of one class's logit over all others: p_c = 1 - O(e^-45) is 1 in fp32
LDS_ROWS = 15360        # bx_linear_lsm_bwd / bx_gap_fc_lsm_bwd: (B + 256) * N <= 15360 (LDS gradient tile)
WORST = {}              # (head, N) -> worst relative error seen, printed by test_zz_heads_report


def _note(head, n, err):
    WORST[(head, n)] = max(WORST.get((head, n), 0.0), err)


def _cmp(got, want, head, n, label, tol=OP_TOL):
    """grad_close (strict max-norm relative error; exactly zero where the reference is exactly zero)."""
    torch.cuda.synchronize()
    err = grad_close(got.detach().float().cpu(), want.detach(), tol, label=f"{head} N={n} {label}")
    _note(head, n, err)
    return err


def _cmp_bf16(got, want, head, n, label):
    """A bf16-stored result within one bf16 ulp of the fp64 value (+ OP_TOL of the tensor's scale)."""
    torch.cuda.synchronize()
    g, w = got.detach().float().cpu().double().flatten(), want.detach().double().flatten()
    _, e = torch.frexp(w)                                          # w = m 2^e, 0.5 <= |m| < 1; bf16 keeps 8 significant bits
    ulp = torch.where(w == 0, torch.zeros_like(w), torch.ldexp(torch.ones_like(w), e - 8))
    scale = max(float(w.abs().max()), 1e-30)
    d = (g - w).abs()
    bad = ~(d <= ulp + OP_TOL * scale)                             # (NaN fails)
    assert not bool(bad.any()), f"{head} N={n} {label}: {int(bad.sum())} elements beyond one bf16 ulp (worst {float((d - ulp).max()) / scale:.3e})"
    _note(head + " (bf16: beyond 1 ulp)", n, float((d - ulp).clamp_min(0).max()) / scale)


def _upstream(regime, B, N, c0, g):
    """Random: a random dlogp.  Confident: -onehot(c0), the gradient KL with a one-hot target (or Grad-CAM's score) sends in: then
    every dlogit is O(e^-45), and a backward that forms dy_c - p_c * sum(dy) = dy_c (1 - p_c) rounds it to 0."""
    if regime == "random":
        return torch.randn(B, N, generator=g)
    return -F.one_hot(torch.full((B,), c0), N).float()


def _confident(fn, args, bias, c0):
    """Raise the final bias of class c0 so that, in every sample, its logit leads all others by at least CONFIDENT (the largest
    lead is CONFIDENT plus the spread of the leads over the batch)."""
    if args[bias].shape[0] < 2:
        return
    with torch.no_grad():
        y = fn(*[t.double() for t in args])
        others = torch.cat((y[:, :c0], y[:, c0 + 1:]), 1).max(1).values
        args[bias][c0] += float(CONFIDENT - (y[:, c0] - others).min())


def _fp64(fn, tensors, upstream):
    """fn on fp64 copies of ``tensors``: (output, gradient of each input) for the upstream gradient ``upstream``."""
    xs = [t.detach().cpu().double().requires_grad_(True) for t in tensors]
    y = fn(*xs)
    y.backward(upstream.double())
    return y.detach(), [x.grad for x in xs]


def _dev(*ts, grad=True):
    return [t.to(DEV).requires_grad_(grad) for t in ts]


def _nan_like(t):
    return torch.full_like(t, float("nan"))


# ================================================================================================================================
# 1. Op level: every head against fp64
# --------------------------------------------------------------------------------------------------------------------------------
def _linear_case(B, K, N, regime, seed):
    g = _gen(seed)
    x = torch.randn(B, K, generator=g)
    w = _uniform((N, K), (6.0 / K) ** 0.5, g)
    b = _uniform((N,), 0.1, g)
    c0 = N - 1                                                     # the last class: beyond any row loop capped at N = 6
    if regime == "confident":
        _confident(_linear_ref, (x, w, b), 2, c0)
    return x, w, b, _upstream(regime, B, N, c0, g)


def _linear_ref(x, w, b):
    return _lsm(x @ w.T + b)


@pytest.mark.parametrize("N", NS)
def test_linear_lsm_against_fp64(N):
    """EEGNet's dense head (LinearLsmFn).  K = 1, 63, 200, 992, 1488: tails of the 64- and 256-wide loops of k_linear_lsm_fwd;
    B = 257 runs the `b += 256` loop of k_linear_lsm_bwd_w (at N = 32 the LDS limit stops at B = 224, test_batch_limit_*)."""
    for K in (1, 63, 200, 992, 1488):
        for B in (1, 3, 64, 257):
            if (B + 256) * N > LDS_ROWS:
                continue
            for regime in ("random", "confident"):
                x, w, b, up = _linear_case(B, K, N, regime, seed=1000 * N + K + B)
                y_r, (dx_r, dw_r, db_r) = _fp64(_linear_ref, (x, w, b), up)
                xg, wg, bg = _dev(x, w, b)
                y = ops.LinearLsmFn.apply(xg, wg, bg)
                y.backward(up.to(DEV))
                tag = f"K={K} B={B} {regime}"
                _cmp(y, y_r, "linear_lsm fwd", N, tag)
                _cmp(xg.grad, dx_r, "linear_lsm bwd", N, tag + " dx")
                _cmp(wg.grad, dw_r, "linear_lsm bwd", N, tag + " dw")
                _cmp(bg.grad, db_r, "linear_lsm bwd", N, tag + " db")


@pytest.mark.parametrize("N", NS)
def test_linear_lsm_backward_optional_outputs(N):
    """bx_linear_lsm_bwd with dx, dw, db each null in turn: the outputs that are asked for are still exact."""
    lib = L.load()
    for K, B in ((200, 64), (1488, 3)):
        x, w, b, up = _linear_case(B, K, N, "random", seed=7 * N + K)
        y_r, (dx_r, dw_r, db_r) = _fp64(_linear_ref, (x, w, b), up)
        xg, wg, bg, upg = (t.to(DEV) for t in (x, w, b, up))
        with torch.no_grad():
            logp = ops.LinearLsmFn.apply(xg, wg, bg)
        for want in ((1, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1)):
            outs = [_nan_like(t) if on else None for t, on in zip((xg, wg, bg), want)]
            L.check(lib.bx_linear_lsm_bwd(upg.data_ptr(), logp.data_ptr(), xg.data_ptr(), wg.data_ptr(),
                                          *[ops._p(t) for t in outs], B, K, N, ops._stream()), "bx_linear_lsm_bwd")
            for t, r, name in zip(outs, (dx_r, dw_r, db_r), ("dx", "dw", "db")):
                if t is not None:
                    _cmp(t, r, "linear_lsm bwd", N, f"K={K} B={B} only {want} {name}")


def _gap_case(B, H, W, C, N, dt, regime, seed):
    g = _gen(seed)
    feat = torch.rand(B, H, W, C, generator=g).to(dt)              # (ReLU'd stage output: non-negative)
    w = _uniform((N, C), (6.0 / C) ** 0.5, g) * 4
    b = _uniform((N,), 0.1, g)
    c0 = N - 1
    if regime == "confident":
        _confident(_gap_ref, (feat, w, b), 2, c0)
    return feat, w, b, _upstream(regime, B, N, c0, g)


def _gap_ref(feat, w, b):
    return _lsm(feat.mean(dim=(1, 2)) @ w.T + b)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", NS)
def test_gap_fc_lsm_against_fp64(N, dt):
    """Spectrogram head (GapFcLsmFn): NHWC features in fp32 or bf16 storage, C = 256; HW = 4, 15, 21 are not multiples of 8
    (k_gap's tail loop), 16 is.  bf16: the reference reads the same bf16 values; the bf16 feature gradient to one ulp."""
    for (H, W), B in (((2, 2), 1), ((3, 5), 5), ((4, 4), 3), ((3, 7), 64)):
        for regime in ("random", "confident"):
            feat, w, b, up = _gap_case(B, H, W, 256, N, dt, regime, seed=31 * N + H * W + B)
            y_r, (df_r, dw_r, db_r) = _fp64(_gap_ref, (feat, w, b), up)
            fg, wg, bg = _dev(feat, w, b)
            y = ops.GapFcLsmFn.apply(fg, wg, bg)
            y.backward(up.to(DEV))
            tag = f"HW={H}x{W} B={B} {dt} {regime}"
            _cmp(y, y_r, "gap_fc_lsm fwd", N, tag)
            assert fg.grad.dtype == dt
            if dt == torch.bfloat16:
                _cmp_bf16(fg.grad, df_r, "gap_fc_lsm bwd", N, tag + " dfeat")
            else:
                _cmp(fg.grad, df_r, "gap_fc_lsm bwd", N, tag + " dfeat")
            _cmp(wg.grad, dw_r, "gap_fc_lsm bwd", N, tag + " dw")
            _cmp(bg.grad, db_r, "gap_fc_lsm bwd", N, tag + " db")


@pytest.mark.parametrize("N", NS)
def test_gap_fc_lsm_backward_optional_outputs(N):
    lib = L.load()
    B, H, W, C = 5, 3, 5, 256
    feat, w, b, up = _gap_case(B, H, W, C, N, torch.float32, "random", seed=5 * N)
    y_r, (df_r, dw_r, db_r) = _fp64(_gap_ref, (feat, w, b), up)
    fg, wg, bg, upg = (t.to(DEV) for t in (feat, w, b, up))
    gap = torch.empty(B, C, device=DEV)
    logp = torch.empty(B, N, device=DEV)
    L.check(lib.bx_gap_fc_lsm_fwd(fg.data_ptr(), wg.data_ptr(), bg.data_ptr(), gap.data_ptr(), logp.data_ptr(), B, H * W, C, N,
                                  L.BX_F32, ops._stream()), "bx_gap_fc_lsm_fwd")
    _cmp(gap, feat.double().mean(dim=(1, 2)), "gap_fc_lsm fwd", N, "gap")
    for want in ((1, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 1)):
        outs = [_nan_like(t) if on else None for t, on in zip((fg, wg, bg), want)]
        L.check(lib.bx_gap_fc_lsm_bwd(upg.data_ptr(), logp.data_ptr(), gap.data_ptr(), wg.data_ptr(), *[ops._p(t) for t in outs],
                                      B, H * W, C, N, L.BX_F32, ops._stream()), "bx_gap_fc_lsm_bwd")
        for t, r, name in zip(outs, (df_r, dw_r, db_r), ("dfeat", "dw", "db")):
            if t is not None:
                _cmp(t, r, "gap_fc_lsm bwd", N, f"only {want} {name}")


def _fusion_case(B, N, Hd, regime, seed):
    g = _gen(seed)
    e = torch.log_softmax(torch.randn(B, N, generator=g) * 2, 1)
    s = torch.log_softmax(torch.randn(B, N, generator=g) * 2, 1)
    w1 = _uniform((Hd, 2 * N), (6.0 / (2 * N)) ** 0.5, g)
    b1 = _uniform((Hd,), 0.1, g)
    w2 = _uniform((N, Hd), (6.0 / Hd) ** 0.5, g)
    b2 = _uniform((N,), 0.1, g)
    c0 = N - 1
    if regime == "confident":
        _confident(_fusion_ref, (e, s, w1, b1, w2, b2), 5, c0)
    return (e, s, w1, b1, w2, b2), _upstream(regime, B, N, c0, g)


def _fusion_hds(N):
    return (128,) + ((2 * N,) if (2 * N) % 64 else ())         # Hd = 2N: the smallest legal width, a ragged last wave


@pytest.mark.parametrize("N", NS)
def test_fusion_head_against_fp64(N):
    """cat -> Linear(2N, Hd) -> ReLU -> Linear(Hd, N) -> LogSoftmax (FusionHeadFn), Hd = 128 and Hd = 2N; B = 70 gives
    k_fusion_bwd_w's lanes a second trip over the batch."""
    for Hd in _fusion_hds(N):
        for B in (1, 4, 70):
            for regime in ("random", "confident"):
                args, up = _fusion_case(B, N, Hd, regime, seed=77 * N + Hd + B)
                y_r, grads_r = _fp64(_fusion_ref, args, up)
                gargs = _dev(*args)
                y = ops.FusionHeadFn.apply(*gargs)
                y.backward(up.to(DEV))
                tag = f"Hd={Hd} B={B} {regime}"
                _cmp(y, y_r, "fusion_head fwd", N, tag)
                for t, r, name in zip(gargs, grads_r, ("de", "ds", "dw1", "db1", "dw2", "db2")):
                    _cmp(t.grad, r, "fusion_head bwd", N, f"{tag} {name}")


@pytest.mark.parametrize("N", NS)
def test_fusion_head_backward_optional_outputs(N):
    lib = L.load()
    Hd, B = _fusion_hds(N)[-1], 6
    args, up = _fusion_case(B, N, Hd, "random", seed=3 * N)
    y_r, grads_r = _fp64(_fusion_ref, args, up)
    e, s, w1, b1, w2, b2 = (t.to(DEV) for t in args)
    upg = up.to(DEV)
    hidden, logp = torch.empty(B, Hd, device=DEV), torch.empty(B, N, device=DEV)
    L.check(lib.bx_fusion_head_fwd(*[t.data_ptr() for t in (e, s, w1, b1, w2, b2, hidden, logp)], B, N, Hd, ops._stream()),
            "bx_fusion_head_fwd")
    for want in ((1, 0, 1, 0, 0, 1), (0, 1, 0, 1, 1, 0), (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1)):
        outs = [_nan_like(t) if on else None for t, on in zip((e, s, w1, b1, w2, b2), want)]
        L.check(lib.bx_fusion_head_bwd(upg.data_ptr(), logp.data_ptr(), hidden.data_ptr(), e.data_ptr(), s.data_ptr(), w1.data_ptr(),
                                       w2.data_ptr(), *[ops._p(t) for t in outs], B, N, Hd, ops._stream()), "bx_fusion_head_bwd")
        for t, r, name in zip(outs, grads_r, ("d_eeg_logp", "d_spec_logp", "dw1", "db1", "dw2", "db2")):
            if t is not None:
                _cmp(t, r, "fusion_head bwd", N, f"only {want} {name}")


def _mm_fast(N, K, C):
    """the dispatch rule of bx_mm_head_fwd (csrc/heads.hip)"""
    return 2 * N <= 12 and N <= 8 and K <= 1024 and C <= 1024


# (N, K, Hd, path): Hd * 2N <= 4096 is the fused head's LDS limit, hence Hd = 120 / 64 at N = 17 / 32
MM_CASES = ([(n, 992, 128, "fast") for n in (1, 2, 3, 6)] + [(n, 992, 128, "general: N > 6") for n in (7, 8, 16)]
            + [(17, 992, 120, "general: N > 6"), (32, 992, 64, "general: N > 6")]
            + [(n, 1488, 128, "general: K > 1024") for n in (1, 2, 3, 6)])


def _mm_case(B, H, W, C, K, N, Hd, dt, regime, seed):
    g = _gen(seed)
    feat = torch.rand(B, H, W, C, generator=g).to(dt)
    ef = torch.randn(B, K, generator=g)
    fcw, fcb = _uniform((N, C), (6.0 / C) ** 0.5, g) * 4, _uniform((N,), 0.1, g)
    dw, db = _uniform((N, K), (6.0 / K) ** 0.5, g), _uniform((N,), 0.1, g)
    w1, b1 = _uniform((Hd, 2 * N), (6.0 / (2 * N)) ** 0.5, g), _uniform((Hd,), 0.1, g)
    w2, b2 = _uniform((N, Hd), (6.0 / Hd) ** 0.5, g), _uniform((N,), 0.1, g)
    args = (feat, ef, fcw, fcb, dw, db, w1, b1, w2, b2)
    c0 = N - 1
    if regime == "confident":
        _confident(_mm_ref, args, 9, c0)
    return args, _upstream(regime, B, N, c0, g)


def _mm_ref(feat, ef, fcw, fcb, dw, db, w1, b1, w2, b2):
    s = _lsm(feat.mean(dim=(1, 2)) @ fcw.T + fcb)
    e = _lsm(ef @ dw.T + db)
    return _fusion_ref(e, s, w1, b1, w2, b2)


MM_NAMES = ("dfeat", "d_eeg_feat", "d_fc_w", "d_fc_b", "d_dense_w", "d_dense_b", "dw1", "db1", "dw2", "db2")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,K,Hd,path", MM_CASES)
def test_multimodal_head_against_fp64(N, K, Hd, path, dt):
    """The fused head (MultimodalHeadFn) on each of its forward paths, asserted from the launcher's own rule; C = 256, HW = 15
    (not a multiple of the forward's 16-position loop).  Every input and parameter gradient, then every optional output null
    in turn (the wrapper passes null for each tensor that needs no gradient)."""
    C, H, W = 256, 3, 5
    assert _mm_fast(N, K, C) == (path == "fast"), path
    for B in (1, 5):
        for regime in ("random", "confident"):
            args, up = _mm_case(B, H, W, C, K, N, Hd, dt, regime, seed=13 * N + K + B)
            y_r, grads_r = _fp64(_mm_ref, args, up)
            gargs = _dev(*args)
            y = ops.MultimodalHeadFn.apply(*gargs)
            y.backward(up.to(DEV))
            tag = f"{path} K={K} Hd={Hd} B={B} {dt} {regime}"
            _cmp(y, y_r, "mm_head fwd", N, tag)
            for t, r, name in zip(gargs, grads_r, MM_NAMES):
                if name == "dfeat" and dt == torch.bfloat16:
                    assert t.grad.dtype == dt
                    _cmp_bf16(t.grad, r, "mm_head bwd", N, f"{tag} {name}")
                else:
                    _cmp(t.grad, r, "mm_head bwd", N, f"{tag} {name}")
    args, up = _mm_case(3, H, W, C, K, N, Hd, dt, "random", seed=17 * N + K)
    _, grads_r = _fp64(_mm_ref, args, up)
    for parity in (0, 1):
        gargs = [t.to(DEV).requires_grad_(i % 2 == parity) for i, t in enumerate(args)]
        ops.MultimodalHeadFn.apply(*gargs).backward(up.to(DEV))
        for i, (t, r, name) in enumerate(zip(gargs, grads_r, MM_NAMES)):
            if i % 2 != parity:
                assert t.grad is None
            elif name == "dfeat" and dt == torch.bfloat16:
                _cmp_bf16(t.grad, r, "mm_head bwd", N, f"{path} only every other ({parity}) {name}")
            else:
                _cmp(t.grad, r, "mm_head bwd", N, f"{path} only every other ({parity}) {name}")


def _targets(kind, B, N, g):
    if kind == "positive":
        return torch.softmax(torch.randn(B, N, generator=g), 1)
    if kind == "votes":                                             # vote fractions: most rows hold exact zeros
        v = torch.randint(0, 3, (B, N), generator=g).float()
        if N > 1:
            v[::2, N - 1] = 0
        v[:, 0] += (v.sum(1) == 0).float()
        return v / v.sum(1, keepdim=True)
    return F.one_hot(torch.randint(0, N, (B,), generator=g), N).float()


@pytest.mark.parametrize("kind", ["positive", "votes", "onehot"])
@pytest.mark.parametrize("N", NS)
def test_kldiv_against_fp64(N, kind):
    """KLDivFn against torch.nn.functional.kl_div in fp64 (its convention for a zero target: loss 0, gradient 0).  All three
    reductions, grad_scale 1 and 0.37; B = 5 and B = 64 (B N > 256: the 256-thread stride loop of k_kldiv)."""
    for B in (5, 64):
        g = _gen(100 * N + B + len(kind))
        logp = torch.log_softmax(torch.randn(B, N, generator=g) * 2, 1)
        t = _targets(kind, B, N, g)
        if kind == "votes" and N > 1:
            assert bool((t == 0).any())
        for red in ("mean", "batchmean", "sum"):
            for gs in (1.0, 0.37):
                lr = logp.double().requires_grad_(True)
                loss_r = F.kl_div(lr, t.double(), reduction=red)
                (loss_r * gs).backward()
                lg = logp.to(DEV).requires_grad_(True)
                loss = ops.KLDivFn.apply(lg, t.to(DEV), red, gs)
                loss.backward()
                tag = f"{kind} B={B} {red} gs={gs}"
                _cmp(loss, loss_r.detach(), "kldiv loss", N, tag)
                _cmp(lg.grad, lr.grad, "kldiv grad", N, tag)


# ================================================================================================================================
# 2. Model level: the three head routes end to end (EEG 19 x 2000, spectrogram 4 x 32 x 64, B = 4)
# --------------------------------------------------------------------------------------------------------------------------------
def _mm_models(N, seed, dt=torch.float32):
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0), seed=seed)
    mine = brainxai.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0, compute_dtype=dt)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV)


def _mm_inputs(N, B=4, seed=11):
    g = _gen(seed + N)
    return (O.seeded((B, 1, 19, 2000), seed, "randn"), O.seeded((B, 4, 32, 64), seed + 1, "rand"),
            _targets("votes", B, N, g))


def _model_step(mine, eeg, spec, labels):
    mine.zero_grad(set_to_none=True)
    keep = ops.keep_block_activations(mine)
    y = mine(eeg.to(DEV), spec.to(DEV))
    loss = brainxai.KLDivLoss()(y, labels.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return y.detach().cpu(), loss.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in mine.named_parameters()}, keep


@pytest.mark.parametrize("N", [2, 7, 16, 17, 32])
def test_multimodal_model_at_n_classes(N):
    """build_multimodal(num_classes=N) against the oracle's: logits, the KL loss (vote-fraction targets with zeros) and every
    parameter gradient against the decision-matched fp64 twin (as test_multimodal_train3).  N <= 16 runs the fused head,
    N >= 17 the three separate ops; at N = 7 and 16 the unfused path (ops.FUSED_HEAD = False) must agree too."""
    ref, mine = _mm_models(N, seed=41 + N)
    assert mine._fusable() == (N <= 16)
    eeg, spec, labels = _mm_inputs(N)
    ref.train(); mine.train()
    runs = {}
    try:
        for fused in ((True, False) if N in (7, 16) else (True,)):
            ops.FUSED_HEAD = fused
            assert mine._fusable() == (fused and N <= 16)
            route = "fused head" if mine._fusable() else "separate heads"
            y, loss, grads, keep = _model_step(mine, eeg, spec, labels)
            twin, _ = matched_oracle(O, copy.deepcopy(ref), (eeg, spec), keep, f"mm N={N} fused={fused}")
            ops.keep_block_activations(mine, on=False)
            out_t = twin(eeg.double(), spec.double())
            loss_t = O.kl_div(out_t, labels.double())
            loss_t.backward()
            assert y.shape == (4, N)
            err = rel_err(y, out_t.detach())
            _note(f"model {route} logits", N, err)
            assert err < TIGHT, err
            err = rel_err(loss, loss_t.detach())
            _note(f"model {route} loss", N, err)
            assert err < TIGHT, err
            fl = 1e-2 * max(float(q.grad.abs().max()) for q in twin.parameters())
            for n, q in twin.named_parameters():
                e = grad_close(grads[n], q.grad, MODEL_TOL, label=f"mm N={N} fused={fused} d{n}", floor=fl)
                _note(f"model {route} grads", N, e)
            runs[fused] = (y, grads)
    finally:
        ops.FUSED_HEAD = True
        ops.keep_block_activations(mine, on=False)
    if False in runs:
        (yf, gf), (ys, gs) = runs[True], runs[False]
        assert rel_err(yf, ys) < 1e-5
        fl = 1e-2 * max(float(g.abs().max()) for g in gs.values())
        for n in gf:
            assert rel_err(gf[n], gs[n], floor=fl) < 1e-4, n


def test_multimodal_model_bf16_at_seven_classes():
    """bf16 storage at N = 7 (fused head, general path) against the fp32 oracle, at the bounds test_gpu_bench_config.py holds
    the N = 6 model to: logits 2e-2, loss 1e-2, and gradient direction."""
    ref, mine = _mm_models(7, seed=48, dt=torch.bfloat16)
    assert mine._fusable()
    eeg, spec, labels = _mm_inputs(7)
    ref.train(); mine.train()
    out_r = ref(eeg, spec)
    loss_r = O.kl_div(out_r, labels)
    loss_r.backward()
    y, loss, grads, _ = _model_step(mine, eeg, spec, labels)
    ops.keep_block_activations(mine, on=False)
    e_out, e_loss = rel_err(y, out_r.detach()), rel_err(loss, loss_r.detach())
    _note("model bf16 logits", 7, e_out)
    _note("model bf16 loss", 7, e_loss)
    assert e_out < 2e-2 and e_loss < 1e-2, (e_out, e_loss)
    for n, q in ref.named_parameters():
        head = n.startswith(("fc1.", "fc2.", "eeg_model.dense.", "spectrogram_model.fc."))
        if head or q.numel() >= 1024:
            cos = float(F.cosine_similarity(grads[n].flatten().double(), q.grad.flatten().double(), dim=0))
            assert cos > (0.99 if head else 0.85), (n, cos)


def _eeg_pair(cls, N, seed):
    ref = O.fill_params(getattr(O, cls)(N, Chans=19, Samples=2000, dropoutRate=0.0), seed=seed)
    mine = getattr(brainxai, cls)(N, Chans=19, Samples=2000, dropoutRate=0.0)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV)


@pytest.mark.parametrize("N", [2, 16])
@pytest.mark.parametrize("cls", ["EEGNet", "EEGNetAttentionDeep"])
def test_eeg_nets_at_n_classes(cls, N):
    """Stand-alone EEGNet / EEGNetAttentionDeep with nb_classes = N: output, input and parameter gradients against the fp64
    oracle, evaluation and training mode (batchnorm1's exactly-zero training gradient on the floor, as in test_gpu_parity.py)."""
    ref, mine = _eeg_pair(cls, N, seed=60 + N)
    x = O.seeded((3, 1, 19, 2000), 61, "randn")
    r = O.seeded((3, N), 62, "randn")
    for mode in ("eval", "train"):
        ref64 = copy.deepcopy(ref).double().train(mode == "train")
        mine.train(mode == "train"); mine.zero_grad(set_to_none=True)
        xr = x.double().requires_grad_(True)
        yr = ref64(xr); (yr * r.double()).sum().backward()
        xm = x.to(DEV).requires_grad_(True)
        ym = mine(xm); (ym * r.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert ym.shape == (3, N)
        err = rel_err(ym.detach().cpu(), yr.detach())
        _note(f"{cls} logits", N, err)
        assert err < TIGHT, (mode, err)
        _note(f"{cls} grads", N, grad_close(xm.grad.cpu(), xr.grad, TIGHT, label=f"{cls} N={N} {mode} dx"))
        fl = 1e-2 * max(float(q.grad.abs().max()) for q in ref64.parameters())
        for (n, p), (_, q) in zip(mine.named_parameters(), ref64.named_parameters()):
            tol = MODEL_TOL if (mode == "train" and n.startswith("batchnorm1.")) else TIGHT
            _note(f"{cls} grads", N, grad_close(p.grad.cpu(), q.grad, tol, label=f"{cls} N={N} {mode} d{n}", floor=fl))


def test_eeg_attention_deep_refuses_seventeen_classes():
    """EEGNetAttentionDeep's head kernels hold at most 16 classes (DP_MAXN): the documented RuntimeError, raised on the host
    before the head launches."""
    net = brainxai.EEGNetAttentionDeep(17, Chans=19, Samples=2000, dropoutRate=0.0).to(DEV).eval()
    x = torch.randn(2, 1, 19, 2000, device=DEV)
    with torch.no_grad():
        feat = net.features(x)
        with pytest.raises(RuntimeError, match="<= 16 classes"):
            net.head(feat)
        with pytest.raises(RuntimeError, match="<= 16 classes"):
            net(x)


# ================================================================================================================================
# 3. Attribution at N != 6
# --------------------------------------------------------------------------------------------------------------------------------
CAM_TOL = 1e-3          # tests/test_gpu_parity.py::test_gradcam_targets, tests/test_gpu_eeg_gradcam.py


def _tie_top_two(ref, N, eeg, spec):
    """fc2 rows 0 and N-1 equal and lifted 2 above every other logit: the fused output's two largest logits are bit-identical on
    any arithmetic, and the arg-max must be the first of them (class 0), as torch.argmax picks.  (Their Grad-CAM maps are
    identical too -- equal fc2 rows give equal gradients -- so the maps cannot show which one was taken; bx_class_seed, which the
    other Grad-CAM forms use, is checked for the first-maximum rule directly in test_class_seed_and_softmax_rows.)"""
    with torch.no_grad():
        ref.fc2.weight[N - 1] = ref.fc2.weight[0]
        ref.fc2.bias[N - 1] = ref.fc2.bias[0]
        out = copy.deepcopy(ref).double().eval()(eeg.double(), spec.double())
        lift = float((out[:, 1:N - 1].max(1).values - out[:, 0]).max()) + 2.0
        ref.fc2.bias[0] += lift
        ref.fc2.bias[N - 1] += lift


# (a tie at N = 2 would tie every class: both maps are then exactly zero, and only rounding noise is left to compare)
@pytest.mark.parametrize("N,tie", [(2, False), (16, False), (17, False), (32, False), (16, True), (32, True)])
def test_last_stage_gradcam_at_n_classes(N, tie):
    """bx_gradcam_head (and, for N <= 16, the sweep form with the EEG head and the up-sampling inside) against the oracle's hook
    Grad-CAM in fp64: raw maps, ReLU'd maps and channel weights; class_idx None, a fixed class and "all" (grid.y = N)."""
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0), seed=70 + N)
    eeg, spec = O.seeded((3, 1, 19, 2000), 71, "randn"), O.seeded((3, 4, 32, 64), 72, "rand")
    if tie:
        _tie_top_two(ref, N, eeg, spec)
    mine = brainxai.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    mine.to(DEV)
    ref64 = copy.deepcopy(ref).double()
    e, s = eeg.to(DEV), spec.to(DEV)
    for class_idx in (None, N - 1, "all"):
        cam_r, raw_r, w_r, _, out_r = O.grad_cam(ref64, eeg.double(), spec.double(), class_idx=class_idx, upsample=False, return_parts=True)
        if tie:
            assert bool((out_r.argmax(1) == 0).all())
        cam, raw, w, _, out = brainxai.grad_cam(mine, e, s, class_idx=class_idx, upsample=False, return_parts=True)
        torch.cuda.synchronize()
        assert tuple(raw.shape) == tuple(raw_r.shape) and tuple(w.shape) == tuple(w_r.shape)
        rs = float(raw_r.abs().max())
        errs = (rel_err(raw.cpu(), raw_r), rel_err(cam.cpu(), cam_r, floor=rs), rel_err(w.cpu(), w_r), rel_err(out.cpu(), out_r))
        _note("gradcam head", N, max(errs))
        assert max(errs) < CAM_TOL, (class_idx, errs)
        up_r = O.grad_cam(ref64, eeg.double(), spec.double(), class_idx=class_idx)
        up = brainxai.grad_cam(mine, e, s, class_idx=class_idx)            # N <= 16: bx_gradcam_head_sweep
        torch.cuda.synchronize()
        assert tuple(up.shape) == tuple(up_r.shape)
        err = rel_err(up.cpu(), up_r, floor=rs)
        _note("gradcam sweep" if N <= 16 else "gradcam head + resize", N, err)
        assert err < CAM_TOL, (class_idx, err)


def test_gradcam_head_above_the_separate_heads_limit():
    """bx_gradcam_head accepts N <= 64 although the separate heads stop at 32: N = 48 through the C entry point (the EEG
    log-probs given directly) against the fp64 restatement, every class ("all") and the arg-max; N = 65 is refused."""
    lib = L.load()
    g = _gen(5)
    B, h, w_, C, N, Hd = 2, 2, 4, 256, 48, 128
    A = torch.rand(B, h, w_, C, generator=g)
    e_lp = torch.log_softmax(torch.randn(B, N, generator=g) * 2, 1)
    fcw, fcb = _uniform((N, C), (6.0 / C) ** 0.5, g) * 4, _uniform((N,), 0.1, g)
    w1, b1 = _uniform((Hd, 2 * N), (6.0 / (2 * N)) ** 0.5, g), _uniform((Hd,), 0.1, g)
    w2, b2 = _uniform((N, Hd), (6.0 / Hd) ** 0.5, g), _uniform((N,), 0.1, g)
    Ad = A.double().requires_grad_(True)
    out_r = _fusion_ref(e_lp.double(), _lsm(Ad.mean(dim=(1, 2)) @ fcw.double().T + fcb.double()), w1.double(), b1.double(),
                        w2.double(), b2.double())
    dev = [t.to(DEV) for t in (A, e_lp, fcw, fcb, w1, b1, w2, b2)]
    for mode in (-2, -1):
        classes = list(range(N)) if mode == -2 else None
        nm = N if mode == -2 else 1
        wr, rawr = [], []
        for c in (classes if classes is not None else [None]):
            score = out_r.gather(1, out_r.argmax(1, keepdim=True)).sum() if c is None else out_r[:, c].sum()
            (G,) = torch.autograd.grad(score, Ad, retain_graph=True)
            wk = G.mean(dim=(1, 2))
            wr.append(wk)
            rawr.append((A.double() * wk[:, None, None, :]).sum(-1))
        wr, rawr = torch.stack(wr, 1).reshape(B * nm, C), torch.stack(rawr, 1).reshape(B * nm, h, w_)
        out = torch.empty(B, N, device=DEV)
        cam, raw = torch.empty(B * nm, h, w_, device=DEV), torch.empty(B * nm, h, w_, device=DEV)
        wts = torch.empty(B * nm, C, device=DEV)
        L.check(lib.bx_gradcam_head(*[t.data_ptr() for t in dev], out.data_ptr(), cam.data_ptr(), raw.data_ptr(), wts.data_ptr(),
                                    B, h * w_, C, N, Hd, mode, 1, L.BX_F32, ops._stream()), "bx_gradcam_head")
        torch.cuda.synchronize()
        errs = (rel_err(out.cpu(), out_r.detach()), rel_err(wts.cpu(), wr), rel_err(raw.cpu(), rawr),
                rel_err(cam.cpu(), rawr.clamp_min(0), floor=float(rawr.abs().max())))
        _note("gradcam head (C entry)", N, max(errs))
        assert max(errs) < CAM_TOL, (mode, errs)
    bad = lib.bx_gradcam_head(*[t.data_ptr() for t in dev], out.data_ptr(), cam.data_ptr(), None, None, B, h * w_, C, 65, Hd, -1, 1,
                              L.BX_F32, ops._stream())
    assert bad != 0 and b"N=65" in lib.bx_last_error_string()


@pytest.mark.parametrize("N", [2, 16])
def test_eeg_target_gradcam_at_n_classes(N):
    """Grad-CAM at the EEG branch's convolutions with N classes (bx_eeg_gradcam gets N gradient maps under "all"), at the
    tolerance of tests/test_gpu_eeg_gradcam.py, against the oracle's hook Grad-CAM in fp64: this two-class model puts
    p = 1 - 1.6e-6 on its arg-max class, where the fp32 oracle's log-softmax backward keeps only 2 digits of 1 - p."""
    from tests.eeg_gradcam_setup import TARGETS, bn_nontrivial, inputs
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0), seed=80 + N)
    bn_nontrivial(ref.eeg_model, 81 + N)
    mine = brainxai.build_multimodal(19, 2000, 4, num_classes=N, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    mine.to(DEV)
    ref64 = copy.deepcopy(ref).double()
    eeg, spec = inputs(2, 19, 2000, seed=83)
    for target in TARGETS:
        for class_idx in (None, N - 1, "all"):
            cam_r, raw_r, w_r, A_r, _ = O.grad_cam(ref64, eeg.double(), spec.double(), "eeg_model." + target, class_idx, upsample=False,
                                                   return_parts=True)
            cam, raw, w, A, _ = brainxai.grad_cam(mine, eeg.to(DEV), spec.to(DEV), "eeg_model." + target, class_idx, upsample=False,
                                                  return_parts=True)
            torch.cuda.synchronize()
            assert tuple(raw.shape) == tuple(raw_r.shape) and tuple(w.shape) == tuple(w_r.shape)
            rs = float(raw_r.abs().max())
            errs = (rel_err(raw.cpu(), raw_r), rel_err(cam.cpu(), cam_r, floor=rs), rel_err(w.cpu(), w_r))
            if A is not None:
                errs += (rel_err(A.cpu(), A_r),)
            _note("gradcam EEG targets", N, max(errs))
            assert max(errs) < CAM_TOL, (target, class_idx, errs)


@pytest.mark.parametrize("N", NS + (64,))
def test_class_seed_and_softmax_rows(N):
    """bx_class_seed (the one-hot gradient seeds of the hook-based Grad-CAM forms: arg-max = FIRST maximum, as torch.argmax) and
    bx_softmax_rows (LIME's predict_fn) at N classes, rows > B (row r takes sample r % B), with exact ties in the logits."""
    lib = L.load()
    g = _gen(90 + N)
    B = 5
    logp = torch.log_softmax(torch.randn(B, N, generator=g) * 3, 1)
    if N > 1:
        logp[1, N - 1] = logp[1, 0] = logp[1].max() + 1.0              # tie between the first and the last class
        logp[2, :] = -float(torch.log(torch.tensor(float(N))))          # every class tied
    lg = logp.to(DEV)
    for mode in [-1, 0, N - 1]:
        seed = explain._class_seed(lg, mode, rows=2 * B)
        torch.cuda.synchronize()
        cls = logp.argmax(1) if mode == -1 else torch.full((B,), mode)
        want = F.one_hot(cls, N).float().repeat(2, 1)
        assert torch.equal(seed.cpu(), want), mode
    x = torch.randn(300, N, generator=g) * 4                            # 300 rows: two workgroups
    y = torch.empty(300, N, device=DEV)
    xg = x.to(DEV)
    L.check(lib.bx_softmax_rows(xg.data_ptr(), y.data_ptr(), 300, N, ops._stream()), "bx_softmax_rows")
    _cmp(y, torch.softmax(x.double(), 1), "softmax_rows", N, "300 rows")


@pytest.mark.parametrize("N", [2, 17])
def test_lime_predict_fn_at_n_classes(N):
    """predict_fn on a Spectrogram_Model(N) (GapFcLsmFn head): softmax of the eval-mode forward against the oracle's."""
    import numpy as np
    ref = O.fill_params(O.Spectrogram_Model(N), seed=21 + N)
    mine = brainxai.Spectrogram_Model(N)
    mine.load_state_dict(ref.state_dict())
    mine.to(DEV)
    imgs = (np.random.default_rng(3).random((3, 64, 96, 3)) * 255.9).astype(np.float64)
    x = torch.from_numpy(imgs.astype(np.uint8)).permute(0, 3, 1, 2).double() / 255.0
    ref64 = copy.deepcopy(ref).double().eval()
    with torch.no_grad():
        want = torch.softmax(ref64(x), 1).numpy()
    got = brainxai.predict_fn(list(imgs), mine, DEV)
    assert got.shape == (3, N)
    err = float(np.abs(got - want).max())
    _note("predict_fn", N, err)
    assert err < 1e-5 and np.allclose(got.sum(1), 1.0, atol=1e-5)


# ================================================================================================================================
# 4. Limits are refused, not overrun
# --------------------------------------------------------------------------------------------------------------------------------
def test_thirty_three_classes_are_refused():
    """N = 33 is beyond every separate head (HEAD_MAX_N = 32): the model's first forward and each stand-alone head raise."""
    net = brainxai.build_multimodal(19, 2000, 4, num_classes=33, dropout=0.0).to(DEV)
    assert not net._fusable()
    with pytest.raises(RuntimeError, match="N<=32"):
        net(torch.randn(2, 1, 19, 2000, device=DEV), torch.rand(2, 4, 32, 64, device=DEV))
    N, B, K, C, Hd = 33, 2, 64, 256, 128
    r = lambda *s: torch.randn(*s, device=DEV)
    with pytest.raises(RuntimeError, match="N<=32"):
        ops.LinearLsmFn.apply(r(B, K), r(N, K), r(N))
    with pytest.raises(RuntimeError, match="bx_gap_fc_lsm_fwd"):
        ops.GapFcLsmFn.apply(r(B, 2, 2, C), r(N, C), r(N))
    with pytest.raises(RuntimeError, match="N<=32"):
        ops.FusionHeadFn.apply(r(B, N), r(B, N), r(Hd, 2 * N), r(Hd), r(N, Hd), r(N))
    with pytest.raises(RuntimeError, match="N <= 32"):
        ops.MultimodalHeadFn.apply(r(B, 2, 2, C), r(B, K), r(N, C), r(N), r(N, K), r(N), r(32, 2 * N), r(32), r(N, 32), r(N))


@pytest.mark.parametrize("head", ["linear", "gap"])
def test_batch_limit_of_the_separate_heads_at_32_classes(head):
    """(B + 256) N <= 15360: at N = 32 the last batch is 224.  B = 224 is exact against fp64; B = 225 runs forward but its
    backward raises instead of overrunning the LDS gradient tile."""
    N = 32
    for B in (224, 225):
        if head == "linear":
            x, w, b, up = _linear_case(B, 200, N, "random", seed=B)
            fn, Fn = _linear_ref, ops.LinearLsmFn
        else:
            x, w, b, up = _gap_case(B, 2, 3, 256, N, torch.float32, "random", seed=B)
            fn, Fn = _gap_ref, ops.GapFcLsmFn
        xg, wg, bg = _dev(x, w, b)
        y = Fn.apply(xg, wg, bg)
        if B == 224:
            y_r, grads_r = _fp64(fn, (x, w, b), up)
            y.backward(up.to(DEV))
            _cmp(y, y_r, f"{head} at the batch limit", N, "fwd")
            for t, r_, name in zip((xg, wg, bg), grads_r, ("dx", "dw", "db")):
                _cmp(t.grad, r_, f"{head} at the batch limit", N, name)
        else:
            torch.cuda.synchronize()
            assert (B + 256) * N > LDS_ROWS
            with pytest.raises(RuntimeError, match=r"\(B\+256\)\*N <= 15360"):
                y.backward(up.to(DEV))


def test_zz_heads_report():
    """Not a check: prints the worst relative error recorded per head and class count (kept in the GPU log)."""
    print("\n[heads] worst observed error against fp64 (head, N, error):")
    for (head, n), err in sorted(WORST.items()):
        print(f"[heads]   {head:40s} N={n:<3d} {err:.3e}")
