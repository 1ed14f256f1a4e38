"""CPU: what tests/test_gpu_attrib_kernels.py rests on.
  1. the references of tests/cam_ref.py against independent ones (F.interpolate in float64, torch's own autograd and log_softmax, the
     closed forms the last-stage kernel uses);
  2. the reference-only measurements behind the GPU tolerances: the same definitions in plain float32 against fp64 on every shape and
     seed of tests/attrib_cases.py (a quarter of each bound at most), and the float32 resize against the fp64 one (the GPU bound is
     four times the worst);
  3. the refusals of the five entry points, which return before any launch and name the entry point."""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from brainxai import _lib
from tests import attrib_cases as K
from tests import cam_ref as R

REDUCE_TOL = 1e-5              # tests/test_gpu_cam_methods.py::test_cam_reduce_against_fp64_definition
CAM_TOL = 1e-3                 # tests/test_gpu_heads.py, tests/test_gpu_parity.py::test_gradcam_targets
ptr = ctypes.c_void_p


def _rel(a, b, scale=None):
    b = b.double()
    scale = float(b.abs().max()) if scale is None else scale
    return float((a.double() - b).abs().max()) / (scale + 1e-30)


# ---- 1. the references against independent ones ---------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,H,W", sorted(set(K.RESIZE_PLANES + K.SWEEP_PLANES)))
def test_resize_is_interpolate_in_float64(h, w, H, W):
    src = K.resize_input(h, w).astype(np.float64)
    want = F.interpolate(torch.from_numpy(src)[None], size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    got = R.resize(src, H, W)
    assert got.shape == want.shape and got.dtype == np.float64
    assert float(np.abs(got - want).max()) <= 1e-12


def _plain_head(A, e_lp, fcw, fcb, w1, b1, w2, b2):
    """The heads with torch's own layers (no code of tests/cam_ref.py)."""
    s = torch.log_softmax(F.linear(A.mean(1), fcw, fcb), 1)
    return torch.log_softmax(F.linear(torch.relu(F.linear(torch.cat((e_lp, s), 1), w1, b1)), w2, b2), 1)


@pytest.mark.parametrize("i", [0, 7, 11, 19])
def test_head_gradcam_weights_are_the_mean_gradient(i):
    A, e_lp, wts, ref = K.head_case(i)
    c = K.HEAD_CASES[i]
    assert c["method"] == "gradcam"
    Ad = A.double().requires_grad_(True)
    out = _plain_head(Ad, e_lp.double(), *[t.double() for t in wts])
    assert _rel(ref.out, out.detach()) <= 1e-12
    classes = range(c["N"]) if c["mode"] == -2 else [None if c["mode"] == -1 else c["mode"]]
    ws = []
    for cls in classes:
        score = out.gather(1, out.argmax(1, keepdim=True)).sum() if cls is None else out[:, cls].sum()
        (G,) = torch.autograd.grad(score, Ad, retain_graph=True)
        ws.append(G.mean(1))
    want = torch.stack(ws, 1).reshape(ref.w.shape)
    assert _rel(ref.w, want) <= 1e-10
    assert _rel(ref.raw, (want[:, None, :] * A.double().repeat_interleave(len(ws), 0)).sum(-1)) <= 1e-10


@pytest.mark.parametrize("i", [1, 9, 14, 16, 24])
def test_position_constant_gradient_gives_the_closed_forms(i):
    """At the last stage G[k, s] = g[k] at every position: cam's Grad-CAM++ weight must equal HW campp_term(g, HW gap) and Layer-CAM's
    map sum_k max(g_k, 0) A[k, s] -- the forms k_gradcam_head evaluates (csrc/attrib.hip)."""
    A, e_lp, wts, ref = K.head_case(i)
    c = K.HEAD_CASES[i]
    assert c["method"] == "gradcam++"
    g = R.head(A, e_lp, *wts, c["mode"], "gradcam").w                                   # [B*nm, C]
    nm = g.shape[0] // A.shape[0]
    A64 = A.double().repeat_interleave(nm, 0)                                            # [B*nm, HW, C]
    HW = A.shape[1]
    S = HW * A64.mean(1)
    closed = torch.where(g > 0, HW * g ** 3 / (2 * g ** 2 + S * g ** 3 + R.EPS), torch.zeros_like(g))
    assert float((closed > 0).double().mean()) > 0.1
    assert torch.allclose(ref.w, closed, rtol=1e-9, atol=0.0)
    lay = R.head(A, e_lp, *wts, c["mode"], "layercam")
    assert lay.w is None
    assert torch.allclose(lay.raw, (g.clamp_min(0)[:, None, :] * A64).sum(-1), rtol=1e-9, atol=1e-12 * float(lay.raw.abs().max()))


def test_saliency_reference():
    g = K.saliency_input(257, 3, 8, "f32").numpy()
    want = np.array([2.0 * max(abs(float(v)) for v in row[:3]) for row in g])
    got = R.saliency(g, 3, 2.0)
    assert np.array_equal(got, want) and got[0] == 18.0 and got[1] == 0.0 and got[2] == 0.0 and not np.signbit(got[2])
    assert float(got.max()) < K.PAD / 2


# ---- 2. the cases and what the GPU tolerances rest on ------------------------------------------------------------------------------
def test_case_tables_cover_what_they_must():
    assert K.reduce_hws(2048) == (1, 2, 15, 17, 34) and K.reduce_hws(8) == (1, 63, 65, 1023, 1025, 2113)
    seen = collections.defaultdict(set)
    for c in K.HEAD_CASES:
        for k, v in c.items():
            seen[k].add(v if k != "mode" or v < 0 else "fixed")
        assert c["mode"] in (-2, -1, c["N"] - 1)
    assert seen["C"] == {8, 64, 512, 1024, 2048} and seen["N"] == {1, 3, 6, 9} and seen["Hd"] == {1, 100, 300}
    assert seen["mode"] == {-2, -1, "fixed"} and seen["method"] == set(K.METHODS) and seen["dt"] == {"f32", "bf16"}
    assert seen["raw"] == {True, False} and seen["wout"] == {True, False}
    for C in seen["C"]:                                      # every C meets an HW on both sides of its trips
        hws = {c["HW"] for c in K.HEAD_CASES if c["C"] == C}
        trip = 16384 // C
        assert min(hws) < trip < max(hws) and set(K.head_hws(C)) <= hws
    seen = collections.defaultdict(set)
    for c in K.SWEEP_CASES:
        for k, v in c.items():
            seen[k].add(v)
    assert seen["Fe"] == {1, 63, 65, 300} and seen["C"] == {8, 256, 1024} and seen["method"] == set(K.METHODS) and seen["mode"] == {-2, -1}
    assert {(c["h"], c["w"], c["H"], c["W"]) for c in K.SWEEP_CASES} == set(K.SWEEP_PLANES)
    assert {256 % (c["W"] // 4) == 0 for c in K.SWEEP_CASES} == {True, False}
    for h, w, H, W in K.SWEEP_PLANES:
        assert W % 4 == 0
    n = [K.RESIZE_N * H * W for _, _, H, W in K.RESIZE_PLANES]
    assert any(W % 4 == 0 and (k // 4) % 256 for k, (_, _, _, W) in zip(n, K.RESIZE_PLANES))
    assert any(W % 4 and k > 4096 * 256 for k, (_, _, _, W) in zip(n, K.RESIZE_PLANES))


@pytest.mark.parametrize("C", K.REDUCE_CS)
def test_float32_reduce_stays_within_a_quarter_of_the_bound(C):
    """The definitions in plain float32 torch on every (HW, maps_per_act, dtype, method) the GPU test runs at this C."""
    worst = 0.0
    for HW in K.reduce_hws(C):
        for nm in K.REDUCE_NMS:
            for dt in K.DTYPES:
                A, G, refs = K.reduce_case(C, HW, nm, dt)
                A32 = A.float().permute(0, 2, 1).repeat_interleave(nm, 0)
                G32 = G.float().permute(0, 2, 1)
                for m in K.METHODS:
                    raw, w, _, _ = R.cam(A32, G32, m)
                    errs = [_rel(raw, refs[m][0])] + ([] if w is None else [_rel(w, refs[m][1])])
                    worst = max(worst, *errs)
                    assert max(errs) <= 0.25 * REDUCE_TOL, (C, HW, nm, dt, m, errs)
    print(f"float32 cam at C={C}: worst {worst:.2e} of the largest value (bound {REDUCE_TOL:g})")


def _head_errs(ref, got):
    errs = {"out": _rel(got.out, ref.out), "raw": _rel(got.raw, ref.raw)}
    if ref.w is not None:
        errs["w"] = _rel(got.w, ref.w)
    return errs


@pytest.mark.parametrize("i", range(len(K.HEAD_CASES)), ids=[K.case_id(c) for c in K.HEAD_CASES])
def test_float32_head_stays_within_a_quarter_of_the_bound(i):
    A, e_lp, wts, ref = K.head_case(i)
    c = K.HEAD_CASES[i]
    errs = _head_errs(ref, R.head(A, e_lp, *wts, c["mode"], c["method"], dtype=torch.float32))
    print(f"float32 head {K.case_id(c)}: {errs}")
    assert max(errs.values()) <= 0.25 * CAM_TOL, errs


@pytest.mark.parametrize("i", range(len(K.SWEEP_CASES)), ids=[K.case_id(c) for c in K.SWEEP_CASES])
def test_float32_sweep_stays_within_a_quarter_of_the_bound(i):
    A, eeg, wts, ref = K.sweep_case(i)
    c = K.SWEEP_CASES[i]
    got = R.head(A, eeg, *wts, c["mode"], c["method"], dtype=torch.float32)
    errs = _head_errs(ref, got)
    want = R.resize(ref.cam.reshape(-1, c["h"], c["w"]).numpy(), c["H"], c["W"])
    up = R.resize_f32(got.cam.reshape(-1, c["h"], c["w"]).numpy(), c["H"], c["W"])
    errs["up"] = float(np.abs(up - want).max()) / (float(ref.raw.abs().max()) + 1e-30)
    print(f"float32 sweep {K.case_id(c)}: {errs}")
    assert max(errs.values()) <= 0.25 * CAM_TOL, errs


def test_float32_resize_against_fp64_sets_the_gpu_bound():
    """Reference against reference on exactly the inputs of the GPU test, relative to max|src|."""
    worst = 0.0
    for h, w, H, W in K.RESIZE_PLANES:
        src = K.resize_input(h, w)
        err = float(np.abs(R.resize_f32(src, H, W).astype(np.float64) - R.resize(src, H, W)).max()) / float(np.abs(src).max())
        print(f"float32 resize {h}x{w} -> {H}x{W}: {err:.3e} of max|src|")
        worst = max(worst, err)
    print(f"worst {worst:.3e}; RESIZE_WORST_F32 {K.RESIZE_WORST_F32:.3e}; GPU bound {K.RESIZE_BOUND:.3e}")
    assert worst <= K.RESIZE_WORST_F32 <= 1.25 * worst
    for h, w, H, W in K.RESIZE_PLANES:                                  # a neighbouring-pixel error is orders above the bound
        if (h, w) != (1, 1):
            src = K.resize_input(h, w)
            shifted = np.roll(src, 1, axis=-1 if w > 1 else -2)
            assert float(np.abs(R.resize(shifted, H, W) - R.resize(src, H, W)).max()) / float(np.abs(src).max()) > 1e4 * K.RESIZE_BOUND


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
P16 = ptr(4096)                # a dummy non-null, 16-byte aligned pointer: every refusal below is reached before the launch


def _refused(lib, rc, name):
    msg = lib.bx_last_error_string()
    assert rc == -1 and name.encode() + b":" in msg and b"launch" not in msg, (rc, msg)      # BX_EINVAL, from a BX_REQUIRE


def test_cam_reduce_refusals_name_the_entry_point():
    lib = _lib.load()
    for method, name in ((_lib.BX_CAM_GRADCAM_PP, "bx_cam_reduce"), (_lib.BX_CAM_LAYERCAM, "bx_cam_reduce"), (_lib.BX_CAM_GRADCAM, "bx_gradcam_reduce")):
        for n_maps, mpa, HW, C in ((2, 1, 4, 24), (2, 1, 4, 4096), (2, 1, 4, 4), (5, 2, 4, 8), (2, 1, 0, 8)):
            _refused(lib, lib.bx_cam_reduce(P16, P16, P16, None, n_maps, mpa, HW, C, method, 1, _lib.BX_F32, None), name)
    for n_maps, mpa, HW, C in ((2, 1, 4, 24), (2, 1, 4, 4096), (2, 1, 4, 4), (5, 2, 4, 8), (2, 1, 0, 8)):
        _refused(lib, lib.bx_gradcam_reduce(P16, P16, P16, None, n_maps, mpa, HW, C, 1, _lib.BX_BF16, None), "bx_gradcam_reduce")


def test_cam_head_refusals_name_the_entry_point():
    lib = _lib.load()
    ptrs = [P16] * 9 + [P16, None, None]                              # ... out_logp, cam, raw, weights_out
    for method, name in ((_lib.BX_CAM_GRADCAM_PP, "bx_cam_head"), (_lib.BX_CAM_LAYERCAM, "bx_cam_head"), (_lib.BX_CAM_GRADCAM, "bx_gradcam_head")):
        for HW, C in ((4, 24), (4, 4096), (4, 4), (0, 8)):
            _refused(lib, lib.bx_cam_head(*ptrs, 2, HW, C, 6, 32, -1, method, 1, _lib.BX_F32, None), name)
    for HW, C in ((4, 24), (4, 4096), (4, 4), (0, 8)):
        _refused(lib, lib.bx_gradcam_head(*ptrs, 2, HW, C, 6, 32, -1, 1, _lib.BX_F32, None), "bx_gradcam_head")


def test_cam_head_sweep_refusals_name_the_entry_point():
    lib = _lib.load()

    def call(method, maps=P16, Fe=16, h=4, w=4, C=8, H=8, W=8):
        return lib.bx_cam_head_sweep(P16, P16, P16, P16, Fe, *[P16] * 6, None, maps, 2, h, w, C, 6, 32, H, W, -1, method, 1, _lib.BX_F32, None)
    for method, name in ((_lib.BX_CAM_GRADCAM_PP, "bx_cam_head_sweep"), (_lib.BX_CAM_LAYERCAM, "bx_cam_head_sweep"),
                         (_lib.BX_CAM_GRADCAM, "bx_gradcam_head_sweep")):
        _refused(lib, call(method, W=6), name)
        assert b"multiple of 4" in lib.bx_last_error_string()
        _refused(lib, call(method, maps=ptr(4096 + 4)), name)
        assert b"16-byte aligned" in lib.bx_last_error_string()
        _refused(lib, call(method, Fe=0), name)
        # LDS: (2 C + 2 Hd + 5 N + 2048 + h w) floats; 16 + 64 + 30 + 2048 + 14226 = 16384 floats = 64 KiB is the last that fits
        _refused(lib, call(method, h=1, w=14227), name)
        assert b"LDS" in lib.bx_last_error_string()
    _refused(lib, lib.bx_gradcam_head_sweep(P16, P16, P16, P16, 16, *[P16] * 6, None, P16, 2, 128, 128, 8, 6, 32, 8, 8, -1, 1, _lib.BX_F32, None),
             "bx_gradcam_head_sweep")
    assert b"LDS" in lib.bx_last_error_string()


def test_saliency_and_resize_refusals_name_the_entry_point():
    lib = _lib.load()
    for C, Cs in ((9, 8), (3, 12), (4, 4), (0, 8)):
        _refused(lib, lib.bx_saliency_reduce(P16, P16, 1, 16, C, Cs, 1.0, _lib.BX_F32, None), "bx_saliency_reduce")
    for N, h, w, H, W in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 0, 4), (1, 2, 2, 4, 0)):
        _refused(lib, lib.bx_resize_bilinear(P16, P16, N, h, w, H, W, None), "bx_resize_bilinear")
