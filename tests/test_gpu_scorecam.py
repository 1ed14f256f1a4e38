"""GPU: brainxai.score_cam and the bx_scorecam_* entry points against the restatement of the definition (tests/scorecam_ref.py):
the range of every up-sampled channel and the perturbed rows bit for bit, the weighted sum against numpy fp64, and the maps end to
end against the oracle's classes run in fp64 on the CPU, on the models and inputs of tests/perturb_gpu.py.

Bounds.  Range: lo and hi are selections among values both sides compute with the same fp32 operations, so they match bit for bit;
scale is one fp32 division, allowed one ulp.  Weighted sum: one fp32 rounding of the result, relative 2^-23, plus C 2^-52 sum_k |w_k
A_k| for the order of the fp64 sum of C terms, plus one fp32 subnormal step.  End to end, fp32 storage: |raw - ref|(s) <= 1e-5 sum_k
|A[k, s]|: the project's probability bound (TOL of tests/perturb_gpu.py) carried through a sum with the coefficients A[k, s].  The
reference takes the GPU's own activation for its masks and its sum -- the rows are then identical by the bit-for-bit test -- and its
probabilities from the oracle's model in fp64.  Every compared case is first checked ON THE REFERENCE SIDE to discriminate: the
reference with its weights rotated by C/2 channels differs from the true one by more than 100 x the bound somewhere in every sample
-- a sum that paired weights with the wrong channels cannot pass.
bf16 storage: BF16_LOGP x the log-probability scale x sum_k |A[k, s]| (tests/perturb_gpu.py).
Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import perturb_gpu as PG
from tests import cam_ref
from tests import scorecam_ref as S
from tests.attrib_cases import RESIZE_BOUND
from tests.perturb_gpu import DEV, TOL

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---- activations in both layouts ------------------------------------------------------------------------------------------------------------
PLANES = {"2x4 to 64x128": (2, 4, 64, 128), "7x5 to 100x75": (7, 5, 100, 75), "16x24 to 16x24": (16, 24, 16, 24), "1x500 to 1x2000": (1, 500, 1, 2000),
          "1x2000 to 1x2000": (1, 2000, 1, 2000)}
NCH = 16


def _activation(h, w, dt, layout, B=2, seed=0):
    """-> (device tensor in `layout`, plane arguments (dtype, sb, sc, sy, sx, C, h, w), float32 [B,C,h,w] as the kernels read it).
    Channel 1 is constant, channel 2 all negative, channel 3 has -0.0 entries (its extremes are not zero); 'nhwc' is the spectrogram
    branch's [B,h,w,C], 'planar' is [B,C,h,w] -- with h = 1 the EEG branch's saved maps."""
    a = np.random.default_rng(seed + 31 * h + w).standard_normal((B, NCH, h, w)).astype(f32)
    a[:, 1] = f32(0.375)
    a[:, 2] = -np.abs(a[:, 2]) - f32(0.5)
    flat = a.reshape(B, NCH, h * w)                                  # (a view)
    flat[:, 3, ::3] = f32(-0.0)
    flat[:, 3, 1] = f32(-2.0)
    flat[:, 3, 2] = f32(3.0)
    t = torch.from_numpy(a).to(dt)
    logical = t.float().numpy()
    if layout == "nhwc":
        d = t.permute(0, 2, 3, 1).contiguous().to(DEV)
        plane = (ops.bx_dtype(dt), h * w * NCH, 1, w * NCH, NCH, NCH, h, w)
    else:
        d = t.contiguous().to(DEV)
        plane = (ops.bx_dtype(dt), NCH * h * w, h * w, w, 1, NCH, h, w)
    return d, plane, logical


# ---- 1. the range of every up-sampled channel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nhwc", "planar"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(PLANES))
def test_range_equals_the_restatement(case, dt, layout):
    h, w, Hm, Wm = PLANES[case]
    B = 2
    A_d, plane, a = _activation(h, w, dt, layout)
    lo_w, hi_w, scale_w, valid_w = S.ranges(S.upsample(a, Hm, Wm))
    assert not valid_w[:, 1].any() and valid_w.sum() == B * (NCH - 1) and (hi_w[:, 2] < 0).all()
    lib = L.load()
    lo, hi, scale = (torch.full((B, NCH), float("nan"), dtype=torch.float32, device=DEV) for _ in range(3))
    nbytes = lib.bx_scorecam_range_workspace(B, NCH, Hm, Wm)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    L.check(lib.bx_scorecam_range(PG.p(A_d), *plane[:5], B, *plane[5:], Hm, Wm, PG.p(lo), PG.p(hi), PG.p(scale), PG.p(ws), nbytes, PG.stream()), "bx_scorecam_range")
    torch.cuda.synchronize()
    lo, hi, scale = lo.cpu().numpy(), hi.cpu().numpy(), scale.cpu().numpy()
    assert not (np.isnan(lo).any() or np.isnan(hi).any() or np.isnan(scale).any()), "unwritten elements"
    assert np.array_equal(lo.view(np.int32), lo_w.view(np.int32)) and np.array_equal(hi.view(np.int32), hi_w.view(np.int32)), f"{case} {layout}"
    ulps = np.abs(scale.view(np.int32).astype(np.int64) - scale_w.view(np.int32).astype(np.int64))
    print(f"bx_scorecam_range {case} {layout} {dt}: lo, hi bit-equal; scale bit-equal: {bool((ulps == 0).all())} (worst {int(ulps.max())} ulp)")
    assert ulps.max() <= 1 and (scale[~valid_w] == 0).all()
    if layout == "nhwc" or h == 1:                                   # the helper of explain.py reads the two layouts the model produces
        got = X._scorecam_range(A_d if layout == "nhwc" else A_d.reshape(B, NCH, 1, w), layout != "nhwc", Hm, Wm)
        assert all(torch.equal(g.cpu(), torch.from_numpy(v)) for g, v in zip(got, (lo, hi, scale)))


# ---- 2. perturbed rows, bit for bit ---------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 16), (3, 9), (15, 1)]
CIN = {"2x4 to 64x128": 4, "7x5 to 100x75": 3, "16x24 to 16x24": 4, "1x500 to 1x2000": 3, "1x2000 to 1x2000": 4}


def _masks(a, Hm, Wm):
    U = S.upsample(a, Hm, Wm)
    lo, _, scale, _ = S.ranges(U)
    return S.mask(U, lo, scale), lo, scale


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("case", sorted(PLANES))
def test_perturbed_spectrogram_rows_bit_for_bit(case, kind, dt):
    h, w, H, W = PLANES[case]
    B, Cin = 2, CIN[case]
    layout = "nhwc" if kind != "per_channel" else "planar"
    A_d, plane, a = _activation(h, w, dt, layout)                    # the activation is stored as the rows are: fp32 or bf16
    M, lo, scale = _masks(a, H, W)
    x, base, bkind, base_d = PG.row_inputs((B, Cin, H, W), kind)
    x_d, lo_d, scale_d = x.to(DEV), torch.from_numpy(lo).to(DEV), torch.from_numpy(scale).to(DEV)
    lib = L.load()
    for k0, n in WINDOWS:
        for b0, nb in ((0, B), (1, 1)):                              # the second sample group does not start at 0
            out = torch.full((nb * n, H, W, 8), float("nan"), dtype=dt, device=DEV)
            L.check(lib.bx_scorecam_perturb_spec(PG.p(x_d), PG.p(A_d), *plane, PG.p(lo_d), PG.p(scale_d), PG.p(base_d), bkind, PG.p(out), B, Cin, H, W, 8, b0, nb, k0, n,
                                                 ops.bx_dtype(dt), PG.stream()), "bx_scorecam_perturb_spec")
            want = ops.to_nhwc(S.rows(x, M, base, b0, nb, k0, n).to(DEV), dt)
            torch.cuda.synchronize()
            PG.assert_same_rows(out, want, f"{case} {kind} channels {(k0, n)} samples {(b0, nb)}", Cin)
            if layout == "nhwc":
                helper = X._scorecam_perturb(x_d, A_d, False, lo_d, scale_d, base_d, bkind, b0, nb, k0, n, dt)
                assert torch.equal(PG.bits(helper), PG.bits(want))
    # an invalid channel's row is the baseline (up to the sign of a zero)
    const = X._scorecam_perturb(x_d, A_d, False, lo_d, scale_d, base_d, bkind, 0, B, 1, 1, dt) if layout == "nhwc" else None
    if const is not None:
        want = ops.to_nhwc(S.rows(x, np.zeros((B, 1, H, W), dtype=f32), base).to(DEV), dt)
        assert torch.equal(const.float(), want.float())


@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("chans,T", [(19, 2000), (5, 333)])
@pytest.mark.parametrize("w_of_T", [1, 4], ids=["depthwise", "separable"])
@pytest.mark.parametrize("dt_a", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_perturbed_eeg_rows_bit_for_bit(dt_a, w_of_T, chans, T, kind):
    B, w = 2, T // w_of_T
    A_d, plane, a = _activation(1, w, dt_a, "planar")
    M, lo, scale = _masks(a, 1, T)
    x, base, bkind, base_d = PG.row_inputs((B, 1, chans, T), kind)
    x_d, lo_d, scale_d = x.to(DEV), torch.from_numpy(lo).to(DEV), torch.from_numpy(scale).to(DEV)
    dtype_a, sb, sc, _, sx, Cn, _, _ = plane
    for k0, n in WINDOWS:
        for b0, nb in ((0, B), (1, 1)):
            out = torch.full((nb * n, 1, chans, T), float("nan"), dtype=torch.float32, device=DEV)
            L.check(L.load().bx_scorecam_perturb_eeg(PG.p(x_d), PG.p(A_d), dtype_a, sb, sc, sx, Cn, w, PG.p(lo_d), PG.p(scale_d), PG.p(base_d), bkind, PG.p(out),
                                                     B, chans, T, b0, nb, k0, n, PG.stream()), "bx_scorecam_perturb_eeg")
            want = S.rows(x, M, base, b0, nb, k0, n).to(DEV)
            torch.cuda.synchronize()
            PG.assert_same_rows(out, want, f"{chans}x{T} plane {w} {kind} channels {(k0, n)} samples {(b0, nb)}")
            helper = X._scorecam_perturb(x_d, A_d, True, lo_d, scale_d, base_d, bkind, b0, nb, k0, n, torch.float32)
            assert torch.equal(PG.bits(helper), PG.bits(want))


@pytest.mark.parametrize("case", ["1x500 to 1x2000", "1x2000 to 1x2000"])
def test_both_entry_points_agree_on_one_row_planes(case):
    """A [1,T] mask domain through the spectrogram entry point (H = 1) and through the EEG one: the same mask values."""
    _, w, _, T = PLANES[case]
    A_d, plane, a = _activation(1, w, torch.float32, "planar")
    _, lo, scale = _masks(a, 1, T)
    x = O.seeded((2, 1, 1, T), 9, "randn")
    x_d, lo_d, scale_d, zero = x.to(DEV), torch.from_numpy(lo).to(DEV), torch.from_numpy(scale).to(DEV), torch.zeros(1, device=DEV)
    eeg_rows = X._scorecam_perturb(x_d, A_d, True, lo_d, scale_d, zero, 0, 0, 2, 0, NCH, torch.float32)
    out = torch.full((2 * NCH, 1, T, 8), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.load().bx_scorecam_perturb_spec(PG.p(x_d), PG.p(A_d), *plane, PG.p(lo_d), PG.p(scale_d), PG.p(zero), 0, PG.p(out), 2, 1, 1, T, 8, 0, 2, 0, NCH, L.BX_F32,
                                              PG.stream()), "bx_scorecam_perturb_spec")
    assert torch.equal(PG.bits(out[:, 0, :, 0].contiguous()), PG.bits(eeg_rows[:, 0, 0, :].contiguous()))


# ---- 3. the weighted sum ------------------------------------------------------------------------------------------------------------------
COMBINE = {"16 channels, 20x15, nhwc fp32": (16, 20, 15, torch.float32, "nhwc"), "256 channels, 4x8, nhwc fp32": (256, 4, 8, torch.float32, "nhwc"),
           "256 channels, 4x8, nhwc bf16": (256, 4, 8, torch.bfloat16, "nhwc"), "16 channels, 1x500, planar fp32": (16, 1, 500, torch.float32, "planar")}


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "signed"])
@pytest.mark.parametrize("mode", ["prob", "increase"])
@pytest.mark.parametrize("case", sorted(COMBINE))
def test_weighted_sum_against_numpy_fp64(case, mode, relu):
    Cn, h, w, dt, layout = COMBINE[case]
    B, K = 3, 6
    g = np.random.default_rng(Cn + h)
    a = torch.from_numpy(g.standard_normal((B, Cn, h, w)).astype(f32)).to(dt)
    A_d = (a.permute(0, 2, 3, 1) if layout == "nhwc" else a).contiguous().to(DEV)
    plane = (ops.bx_dtype(dt),) + ((h * w * Cn, 1, w * Cn, Cn) if layout == "nhwc" else (Cn * h * w, h * w, w, 1))
    a = a.float().numpy()
    P, Pb = g.random((B, Cn, K)).astype(f32), g.random((B, K)).astype(f32)
    valid = g.random((B, Cn)) > 0.2
    classes = g.integers(0, K, size=B).astype(np.int32)
    w_all = S.weights(P, Pb, valid, mode)                            # fp32 [B,K,C]: one rounding for 'increase'
    assert w_all.dtype == f32
    want, mag = S.combine(w_all, a)
    P_d, Pb_d, valid_d = torch.from_numpy(P).to(DEV), torch.from_numpy(Pb).to(DEV), torch.from_numpy(valid).to(DEV)
    worst = {}
    for name, cls_d, nm in (("all", None, K), ("per sample", torch.from_numpy(classes).to(DEV), 1)):
        raw, cam = (torch.full((B * nm, h * w), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
        wts = torch.full((B * nm, Cn), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.load().bx_scorecam_combine(PG.p(P_d), PG.p(Pb_d) if mode == "increase" else None, PG.p(cls_d), PG.p(valid_d), PG.p(A_d), *plane, B, Cn, h, w, K,
                                             X._SCORECAM_WEIGHTS[mode], 1 if relu else 0, PG.p(raw), PG.p(cam), PG.p(wts), PG.stream()), "bx_scorecam_combine")
        torch.cuda.synchronize()
        raw, cam, wts = raw.cpu().numpy().reshape(B, nm, h, w), cam.cpu().numpy().reshape(B, nm, h, w), wts.cpu().numpy().reshape(B, nm, Cn)
        assert not (np.isnan(raw).any() or np.isnan(cam).any() or np.isnan(wts).any()), "unwritten elements"
        sel = (lambda t: t) if cls_d is None else (lambda t: t[np.arange(B), classes][:, None])
        bound = 2.0 ** -23 * np.abs(sel(want)) + Cn * 2.0 ** -52 * sel(mag) + 2.0 ** -149
        worst[name] = float((np.abs(raw.astype(np.float64) - sel(want)) / bound).max())
        assert worst[name] <= 1.0, (case, mode, name, worst)
        assert np.array_equal(cam, np.maximum(raw, 0) if relu else raw)
        assert np.array_equal(wts.view(np.int32), np.ascontiguousarray(sel(w_all)).view(np.int32)), "weights: w to one fp32 rounding"
        assert (wts[np.broadcast_to(~valid[:, None, :], wts.shape)] == 0).all()
        only = torch.full((B * nm, h * w), float("nan"), dtype=torch.float32, device=DEV)        # cam alone: the raw pointer may be null
        again = torch.empty(B * nm, Cn, dtype=torch.float32, device=DEV)
        L.check(L.load().bx_scorecam_combine(PG.p(P_d), PG.p(Pb_d) if mode == "increase" else None, PG.p(cls_d), PG.p(valid_d), PG.p(A_d), *plane, B, Cn, h, w, K,
                                             X._SCORECAM_WEIGHTS[mode], 1 if relu else 0, None, PG.p(only), PG.p(again),
                                             PG.stream()), "bx_scorecam_combine")
        assert np.array_equal(only.cpu().numpy().reshape(B, nm, h, w).view(np.int32), cam.view(np.int32))
    print(f"bx_scorecam_combine {case} {mode} relu={relu}: worst error / bound: all classes {worst['all']:.2f}, per-sample classes {worst['per sample']:.2f}")


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------------------
def _reference(a, x, Hm, Wm, f, clean, what, baseline=0.0):
    """The reference of one case from the activation ``a`` float32 [B,C,h,w] the GPU returned: masks and rows by the restatement,
    probabilities from f(b, rows) -> log-probabilities (the oracle in fp64), both weightings, with the guard on the reference side."""
    B, Cn = a.shape[:2]
    U = S.upsample(a, Hm, Wm)
    lo, hi, scale, valid = S.ranges(U)
    M = S.mask(U, lo, scale)
    P = S.scores(f, x, M, baseline)
    base_rows = S.rows(x, np.zeros((B, 1, Hm, Wm), dtype=f32), baseline)
    with torch.no_grad():
        P_base = torch.cat([torch.softmax(f(b, base_rows[b:b + 1]).double(), dim=1) for b in range(B)]).numpy()
    cls = clean.argmax(1).numpy()
    bound = TOL * np.abs(a.astype(np.float64)).sum(1)                                            # [B,h,w]: the fp32 bound, also the guard's unit
    ref = {"classes": cls, "P": P, "P_base": P_base, "lo": lo, "hi": hi, "valid": valid, "bound": bound}
    for mode in ("prob", "increase"):
        wts = S.weights(P, P_base, valid, mode)
        raw, _ = S.combine(wts, a)
        rot, _ = S.combine(np.roll(wts, Cn // 2, axis=2), a)
        margin = np.array([(np.abs(rot[b, cls[b]] - raw[b, cls[b]]) / bound[b]).max() for b in range(B)])
        pc = P[np.arange(B), :, cls]
        print(f"{what} {mode}: reference classes {cls} valid {int(valid.sum())}/{valid.size} P[k,c] {pc.min():.3f}..{pc.max():.3f} P_base[c] "
              f"{P_base[np.arange(B), cls].round(3)} |rotated - true| / bound {margin.round(0)}")
        assert margin.min() > 100, f"{what} {mode}: rotating the weights moves the reference by {margin.min():.1f} x the bound only"
        ref[mode] = raw
    return ref


def _compare(raw, ref, mode, what, all_classes=False, tol=TOL):
    B = raw.shape[0]
    assert raw.is_cuda and raw.dtype == torch.float32
    g = raw.cpu().numpy().astype(np.float64)
    want = ref[mode] if all_classes else ref[mode][np.arange(B), ref["classes"]]
    bound = (ref["bound"][:, None] if all_classes else ref["bound"]) * (tol / TOL)
    assert g.shape == want.shape, (g.shape, want.shape)
    worst = float((np.abs(g - want) / bound).max())
    print(f"score_cam {what} {mode}: worst |raw - reference| / bound {worst:.3f} (largest |raw - reference| {float(np.abs(g - want).max()):.2e})")
    assert worst <= 1.0
    return worst


def _nchw(A):
    return A.float().permute(0, 3, 1, 2).contiguous().cpu().numpy()


def _against_fp64_resize(cam, low, size, label):
    """The up-sampled map against the fp64 resize of the low-resolution one (tests/cam_ref.py), at the bound of
    tests/test_gpu_attrib_kernels.py::test_resize_bilinear: the comparison beside it is the kernel against itself."""
    want = cam_ref.resize(low.cpu().numpy(), *size)
    err = float(np.abs(cam.cpu().numpy().astype(np.float64) - want).max()) / (float(low.abs().max()) + 1e-30)
    print(f"score_cam {label}: up-sampled map {err:.2e} of max|map| from the fp64 resize (bound {RESIZE_BOUND:.1e})")
    assert tuple(cam.shape) == want.shape and err <= RESIZE_BOUND


@functools.lru_cache(maxsize=None)
def _mm_setting(dt=torch.float32):
    ref_model, mine = PG.scaled_multimodal(dt)
    eeg, spec = (t[:2].contiguous() for t in PG.mm_inputs())
    r64 = copy.deepcopy(ref_model).double()
    with torch.no_grad():
        clean = r64(eeg.double(), spec.double())
    return mine, eeg, spec, r64, clean


@pytest.mark.parametrize("target", ["block5", "spectrogram_model.block3", "block1", "spectrogram_model.block2.conv2"])
def test_spectrogram_targets_against_fp64_oracle(target):
    mine, eeg, spec, r64, clean = _mm_setting()
    e, s = eeg.to(DEV), spec.to(DEV)
    res = brainxai.score_cam(mine, e, s, target, return_parts=True)
    f = lambda b, xs: r64(eeg[b:b + 1].double().repeat(xs.shape[0], 1, 1, 1), xs.double())          # noqa: E731
    a = _nchw(res.A)
    ref = _reference(a, spec, 64, 128, f, clean, target)
    B, Cn, h, w = a.shape
    # the parts
    assert torch.equal(res.A, brainxai.grad_cam(mine, e, s, target, return_parts=True)[3]), "the activation grad_cam takes"
    assert np.array_equal(res.classes.cpu().numpy(), ref["classes"]) and res.classes.dtype == torch.int64
    assert np.array_equal(res.lo.cpu().numpy(), ref["lo"]) and np.array_equal(res.hi.cpu().numpy(), ref["hi"])
    assert np.array_equal(res.valid.cpu().numpy(), ref["valid"]) and tuple(res.probs.shape) == (B, Cn, 6)
    worst_p = float(np.abs(res.probs.cpu().numpy().astype(np.float64) - ref["P"]).max())
    worst_o = float(np.abs(res.out.cpu().numpy().astype(np.float64) - clean.numpy()).max())
    print(f"score_cam {target}: |P - reference| {worst_p:.2e}, |clean log-probabilities - reference| {worst_o:.2e}")
    assert worst_p <= TOL
    assert tuple(res.raw.shape) == (B, h, w) and tuple(res.cam.shape) == (B, 64, 128) and tuple(res.weights.shape) == (B, Cn)
    _compare(res.raw, ref, "prob", target)
    low = brainxai.score_cam(mine, e, s, target, upsample=False)
    assert torch.equal(low, res.raw.clamp_min(0)) and torch.equal(res.cam, X.resize_bilinear(low, (64, 128)) if (h, w) != (64, 128) else low)
    _against_fp64_resize(res.cam, low, (64, 128), target)
    # the paper's weighting: P_base exceeds every P[k, c] on these inputs, so the map is compared before the ReLU
    inc = brainxai.score_cam(mine, e, s, target, weights="increase", relu=False, upsample=False, return_parts=True)
    assert torch.equal(inc.probs, res.probs) and torch.equal(inc.cam, inc.raw)
    _compare(inc.raw, ref, "increase", target)
    # every class at once costs no further forward pass and slices to the per-class calls
    every = brainxai.score_cam(mine, e, s, target, class_idx="all", return_parts=True)
    assert every.classes is None and tuple(every.raw.shape) == (B, 6, h, w) and tuple(every.cam.shape) == (B, 6, 64, 128)
    assert torch.equal(every.probs, res.probs)
    _compare(every.raw, ref, "prob", target + ", all classes", all_classes=True)
    assert torch.equal(every.cam[torch.arange(B, device=DEV), res.classes], res.cam)
    four = brainxai.score_cam(mine, e, s, target, class_idx=4, return_parts=True)
    assert torch.equal(four.cam, every.cam[:, 4]) and torch.equal(four.raw, every.raw[:, 4]) and torch.equal(four.weights, every.weights[:, 4])
    cls = res.classes.tolist()
    for form in (cls, torch.tensor(cls), torch.tensor(cls, device=DEV, dtype=torch.int32)):
        assert torch.equal(brainxai.score_cam(mine, e, s, target, class_idx=form), res.cam)
    # max_batch values that split the channels differently change no bit
    for mb in (7, 64, 4096):
        other = brainxai.score_cam(mine, e, s, target, max_batch=mb, return_parts=True)
        assert torch.equal(other.probs, res.probs) and torch.equal(other.raw, res.raw) and torch.equal(other.cam, res.cam), f"max_batch {mb}"


# ---- 5. EEG targets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["depthwiseConv", "eeg_model.separableConv"])
def test_eeg_targets_stand_alone_against_fp64_oracle(target):
    ref_model, mine = PG.eegnet_pair()
    xe = O.seeded((2, 1, 19, 2000), 91, "randn")
    n64 = copy.deepcopy(ref_model).double()
    with torch.no_grad():
        clean = n64(xe.double())
    res = brainxai.score_cam(mine, xe.to(DEV), None, target, return_parts=True)
    a = res.A.cpu().numpy()
    w = 2000 if target == "depthwiseConv" else 500
    assert a.shape == (2, 16, 1, w) and a.dtype == f32
    assert torch.equal(res.A, brainxai.grad_cam(mine, xe.to(DEV), None, target, return_parts=True)[3])
    ref = _reference(a, xe, 1, 2000, lambda b, xs: n64(xs.double()), clean, f"EEGNet {target}")
    assert np.array_equal(res.classes.cpu().numpy(), ref["classes"]) and np.array_equal(res.lo.cpu().numpy(), ref["lo"])
    assert tuple(res.raw.shape) == (2, 1, w) and tuple(res.cam.shape) == (2, 1, 2000)
    _compare(res.raw.reshape(2, 1, w), ref, "prob", f"EEGNet {target}")
    low = brainxai.score_cam(mine, xe.to(DEV), None, target, upsample=False)
    assert tuple(low.shape) == (2, 1, w) and torch.equal(res.cam, X.resize_bilinear(low, (1, 2000)) if w != 2000 else low)
    _against_fp64_resize(res.cam, low, (1, 2000), f"EEGNet {target}")
    inc = brainxai.score_cam(mine, xe.to(DEV), None, target, weights="increase", relu=False, return_parts=True, max_batch=5)
    assert torch.equal(inc.probs, res.probs)
    _compare(inc.raw.reshape(2, 1, w), ref, "increase", f"EEGNet {target}")
    every = brainxai.score_cam(mine, xe.to(DEV), None, target, class_idx="all", return_parts=True, baseline=torch.zeros(19))
    assert tuple(every.cam.shape) == (2, 6, 1, 2000) and torch.equal(every.cam[torch.arange(2, device=DEV), res.classes], res.cam)
    _compare(every.raw.reshape(2, 6, 1, w), ref, "prob", f"EEGNet {target}, all classes", all_classes=True)


@functools.lru_cache(maxsize=None)
def _mm_eeg_setting():
    """scaled_multimodal() scales the EEG head to 0.05: masking EEG time columns then moves the fused probability by 0.008 and rotated
    weights move the reference by 60 - 150 x the bound only (checked on the CPU with the oracle's activations).  With the EEG head
    at 0.5 the same check gives 860 - 1 640 x, the clean p 0.43 / 0.54 and P[k, c] 0.47 - 0.57."""
    ref_model, mine = PG.scaled_multimodal()
    with torch.no_grad():
        ref_model.eeg_model.dense.weight *= 10.0
    mine.load_state_dict(ref_model.state_dict())
    eeg, spec = (t[:2].contiguous() for t in PG.mm_inputs())
    r64 = copy.deepcopy(ref_model).double()
    with torch.no_grad():
        clean = r64(eeg.double(), spec.double())
    return mine.eval(), eeg, spec, r64, clean


@pytest.mark.parametrize("target", ["eeg_model.depthwiseConv", "eeg_model.separableConv"])
def test_eeg_targets_of_the_multimodal_model_against_fp64_oracle(target):
    mine, eeg, spec, r64, clean = _mm_eeg_setting()
    e, s = eeg.to(DEV), spec.to(DEV)
    res = brainxai.score_cam(mine, e, s, target, return_parts=True)
    a = res.A.cpu().numpy()
    w = a.shape[3]
    f = lambda b, xs: r64(xs.double(), spec[b:b + 1].double().repeat(xs.shape[0], 1, 1, 1))          # noqa: E731
    ref = _reference(a, eeg, 1, 2000, f, clean, f"multimodal {target}")
    assert torch.equal(res.A, brainxai.grad_cam(mine, e, s, target, return_parts=True)[3])
    assert np.array_equal(res.classes.cpu().numpy(), ref["classes"]) and tuple(res.cam.shape) == (2, 1, 2000)
    _compare(res.raw.reshape(2, 1, w), ref, "prob", f"multimodal {target}")
    inc = brainxai.score_cam(mine, e, s, target, weights="increase", relu=False, return_parts=True)
    _compare(inc.raw.reshape(2, 1, w), ref, "increase", f"multimodal {target}")
    for mb in (7, 64, 4096):                                         # the spectrogram branch runs once per sample whatever the split
        other = brainxai.score_cam(mine, e, s, target, max_batch=mb, return_parts=True)
        assert torch.equal(other.probs, res.probs) and torch.equal(other.cam, res.cam), f"max_batch {mb}"


# ---- 6. bf16 storage ----------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_maps():
    """bf16 storage.  The activation is the bf16 model's own (widened exactly), the masked rows are bit-identical to the host-built
    ones (test_perturbed_spectrogram_rows_bit_for_bit); the probabilities stay within the project's derived bf16 bound of the fp32
    oracle's (BF16_LOGP of tests/perturb_gpu.py), carried through the sum with the coefficients A[k, s].  Measured on the MI355X
    (block3, log-probability scale 3.29): probabilities 6.8e-4 from the oracle's (bound 6.6e-2); raw 2.7e-2 ('prob') and 2.9e-2
    ('increase') at the worst position, 0.003 of the bound there."""
    mine, eeg, spec, r64, clean = _mm_setting(torch.bfloat16)
    e, s = eeg.to(DEV), spec.to(DEV)
    scale = float(clean.abs().max())
    res = brainxai.score_cam(mine, e, s, "block3", return_parts=True)
    assert res.A.dtype == torch.bfloat16
    f = lambda b, xs: r64(eeg[b:b + 1].double().repeat(xs.shape[0], 1, 1, 1), xs.double())          # noqa: E731
    ref = _reference(_nchw(res.A), spec, 64, 128, f, clean, f"block3 (bf16 case, log-probability scale {scale:.2f})")
    assert np.array_equal(res.classes.cpu().numpy(), ref["classes"])
    assert np.array_equal(res.lo.cpu().numpy(), ref["lo"]) and np.array_equal(res.hi.cpu().numpy(), ref["hi"])
    worst_p = float(np.abs(res.probs.cpu().numpy().astype(np.float64) - ref["P"]).max())
    print(f"score_cam block3 bf16: |P - reference| {worst_p:.2e} (bound {PG.BF16_LOGP * scale:.2e})")
    assert worst_p <= PG.BF16_LOGP * scale
    _compare(res.raw, ref, "prob", "block3, bf16 storage", tol=PG.BF16_LOGP * scale)
    inc = brainxai.score_cam(mine, e, s, "block3", weights="increase", relu=False, return_parts=True)
    _compare(inc.raw, ref, "increase", "block3, bf16 storage", tol=PG.BF16_LOGP * scale)


# ---- 7. interface ---------------------------------------------------------------------------------------------------------------------------
def test_interface_forms():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    mine.train()
    for p in list(mine.parameters())[:3]:
        p.requires_grad_(False)
    before = PG.model_state(mine)
    cam = brainxai.score_cam(mine, eeg, spec)
    assert PG.model_state(mine) == before and all(m.training for m in mine.modules()) and all(p.grad is None for p in mine.parameters())
    assert cam.is_cuda and cam.dtype == torch.float32 and tuple(cam.shape) == (3, 64, 128) and bool(torch.isfinite(cam).all()) and float(cam.min()) >= 0.0
    full = brainxai.score_cam(mine, eeg, spec, return_parts=True)
    assert isinstance(full, brainxai.ScoreCamResult) and torch.equal(full.cam, cam)
    assert float((full.probs.sum(2) - 1).abs().max()) <= 1e-6 and full.valid.dtype == torch.bool and bool((full.hi >= full.lo).all())
    with torch.no_grad():
        want = mine.eval()(eeg, spec)
        mine.train()
    assert torch.equal(full.classes, want.argmax(1)) and float((full.out - want).abs().max()) <= TOL
    # the map goes straight into the faithfulness tools
    r = brainxai.deletion_insertion(mine, eeg, spec, cam, steps=8)
    assert tuple(r.deletion.shape) == (3, 9) and tuple(r.ranks.shape) == (3, 64 * 128) and bool(torch.isfinite(r.deletion).all())
    for target in ("eeg_model.depthwiseConv", "eeg_model.separableConv"):
        amap = brainxai.score_cam(mine, eeg, spec, target)
        assert tuple(amap.shape) == (3, 1, 2000)
        r = brainxai.deletion_insertion(mine, eeg, spec, amap, input="eeg", steps=8)
        assert tuple(r.ranks.shape) == (3, 2000) and bool(torch.isfinite(r.insertion_auc).all())
    assert tuple(brainxai.attribution_ranks(brainxai.score_cam(mine, eeg, spec, "block4", class_idx="all")[:, 2]).shape) == (3, 64 * 128)
    assert PG.model_state(mine) == before and all(p.grad is None for p in mine.parameters())


def test_stand_alone_models():
    for dt in (torch.float32, torch.bfloat16):
        net = brainxai.set_compute_dtype(brainxai.Spectrogram_Model(6, in_channels=4).to(DEV), dt)
        s = torch.rand(2, 4, 64, 128, device=DEV)
        res = brainxai.score_cam(net, None, s, "block4", baseline=[0.1, 0.2, 0.3, 0.4], return_parts=True)
        with torch.no_grad():
            want = net.eval()(s).float().argmax(1)
            net.train()
        assert tuple(res.cam.shape) == (2, 64, 128) and tuple(res.raw.shape) == (2, 4, 8) and res.A.dtype == dt
        assert bool(torch.isfinite(res.cam).all()) and net.training and torch.equal(res.classes, want)
        if dt == torch.float32:
            assert torch.equal(res.A, brainxai.grad_cam(net, None, s, "block4", return_parts=True)[3])
    net = brainxai.EEGNetAttentionDeep(6, Chans=19, Samples=2000).to(DEV)
    e = torch.randn(2, 1, 19, 2000, device=DEV)
    for target, w in (("depthwiseConv", 2000), ("separableConv", 500)):
        res = brainxai.score_cam(net, e, None, target, baseline=torch.zeros(19, device=DEV), upsample=False, return_parts=True)
        assert tuple(res.cam.shape) == (2, 1, w) and bool(torch.isfinite(res.cam).all())
        assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
