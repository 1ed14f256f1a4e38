"""GPU: the kernels of csrc/attrib.hip behind grad_cam, GradCamSweep, saliency and every driver that up-samples a map -- k_gradcam,
k_cam, k_gradcam_head, k_resize_bilinear, k_resize_bilinear4, k_saliency -- away from the sizes the multimodal model produces,
through the C entry points on seeded tensors, against the fp64 references of tests/cam_ref.py.  The shapes (tests/attrib_cases.py)
put a size on each side of every trip count and tail mask of those kernels; DESIGN.md section 2 lists which branch each reaches.

Every output buffer is pre-filled with NaN and followed, in the same allocation, by a guard of 64 NaN floats: no element may be left
unwritten and the guard must be untouched.  Every output is computed twice and must be bit-equal (the kernels sum in a fixed order).
A bf16 input is rounded first and the reference reads the rounded values.  The last position and channel never hold a zero, so a
clamped load that is added instead of masked shows.

Bounds (none is new; tests/test_attrib_ref_cpu.py shows that plain float32 arithmetic stays within a quarter of each on these inputs):
  REDUCE_TOL 1e-5 of the largest value  bx_cam_reduce maps and weights (test_cam_reduce_against_fp64_definition)
  CAM_TOL    1e-3                       the heads' maps, weights and log-probabilities (tests/test_gpu_heads.py)
  PAIR_TOL   1e-6                       the sweep against bx_cam_head + bx_resize_bilinear (test_gpu_parity.py::test_gradcam_targets)
  RESIZE_BOUND 1.6e-5 of max|src|       4 x 3.952e-6, the worst deviation of the float32 restatement of the resize from the fp64 one on
                                        exactly these inputs (100x75 -> 7x5; all other planes <= 4.7e-7); a neighbouring-pixel error
                                        is of order 1
  bit-equal                             identity resize, saliency, bx_gradcam_* against method 0, repeated launches."""
import numpy as np
import pytest
import torch

from brainxai import _lib as L
from brainxai import ops
from tests import attrib_cases as K
from tests import cam_ref as R
from tests.eeg_gradcam_setup import rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REDUCE_TOL = 1e-5
CAM_TOL = 1e-3
PAIR_TOL = 1e-6
GUARD = 64
CODE = {"gradcam": L.BX_CAM_GRADCAM, "gradcam++": L.BX_CAM_GRADCAM_PP, "layercam": L.BX_CAM_LAYERCAM}


class Out:
    """n fp32 outputs, NaN, `offset` floats into an allocation that ends in GUARD more NaN floats."""

    def __init__(self, n, offset=0):
        self.n, self.offset = n, offset
        self.buf = torch.full((offset + n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.view = self.buf[offset:offset + n]
        self.ptr = self.view.data_ptr()

    def get(self, label=""):
        """-> the outputs on the host, after checking that all were written and nothing around them was."""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        body = host[self.offset:self.offset + self.n]
        assert not bool(torch.isnan(body).any()), f"{label}: {int(torch.isnan(body).sum())} of {self.n} outputs left unwritten"
        assert bool(torch.isnan(host[:self.offset]).all()) and bool(torch.isnan(host[self.offset + self.n:]).all()), f"{label}: guard overwritten"
        return body.clone()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


# ================================================================================================ a. bx_cam_reduce
def _reduce(lib, Ad, Gd, n_maps, nm, HW, C, method, relu, dt, want_w, wrapper=False):
    cam, wts = Out(n_maps * HW), Out(n_maps * C) if want_w else None
    args = (Ad.data_ptr(), Gd.data_ptr(), cam.ptr, None if wts is None else wts.ptr, n_maps, nm, HW, C)
    tail = (relu, ops.bx_dtype(K.DTYPES[dt]), ops._stream())
    if wrapper:
        L.check(lib.bx_gradcam_reduce(*args, *tail), "bx_gradcam_reduce")
    else:
        L.check(lib.bx_cam_reduce(*args, CODE[method], *tail), "bx_cam_reduce")
    label = f"cam_reduce {method} C={C} HW={HW} nm={nm} {dt} relu={relu}"
    return cam.get(label), None if wts is None else wts.get(label + " weights")


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("C,HW", K.REDUCE_SHAPES)
def test_cam_reduce(C, HW, dt):
    """k_gradcam (method 0), k_cam<Grad-CAM++> with both cam_colsum passes, k_cam<Layer-CAM>.  C = 8: one lane per position; C >= 512:
    the `c0 += 512` loop; HW from reduce_hws(C): the clamped index with masked add, the store mask, less than one position group."""
    lib = L.load()
    B = K.REDUCE_B
    worst = 0.0
    for nm in K.REDUCE_NMS:
        A, G, refs = K.reduce_case(C, HW, nm, dt)
        Ad, Gd = _dev(A, G)
        for method in K.METHODS:
            raw_o, w_o, _, _ = refs[method]
            scale = float(raw_o.abs().max())
            for relu in (0, 1):
                want = (raw_o.clamp_min(0) if relu else raw_o).reshape(-1)
                for want_w in ((True, False) if w_o is not None else (False,)):
                    cam, wts = _reduce(lib, Ad, Gd, B * nm, nm, HW, C, method, relu, dt, want_w)
                    errs = [rel(cam, want, scale)] + ([rel(wts, w_o.reshape(-1))] if want_w else [])
                    worst = max(worst, *errs)
                    assert max(errs) <= REDUCE_TOL, (method, C, HW, nm, dt, relu, want_w, errs)
                    cam2, wts2 = _reduce(lib, Ad, Gd, B * nm, nm, HW, C, method, relu, dt, want_w)
                    assert _bits_equal(cam, cam2) and (not want_w or _bits_equal(wts, wts2)), "a second launch differs"
                    if method == "gradcam":
                        cam3, wts3 = _reduce(lib, Ad, Gd, B * nm, nm, HW, C, method, relu, dt, want_w, wrapper=True)
                        assert _bits_equal(cam, cam3) and (not want_w or _bits_equal(wts, wts3)), "bx_gradcam_reduce differs from method 0"
    print(f"[attrib] cam_reduce C={C} HW={HW} {dt}: worst {worst:.2e}")


# ================================================================================================ b. bx_cam_head
def _head(lib, dev, B, HW, C, N, Hd, mode, method, relu, dt, want_raw, want_w, wrapper=False):
    nm = N if mode == -2 else 1
    out, cam = Out(B * N), Out(B * nm * HW)
    raw, wts = Out(B * nm * HW) if want_raw else None, Out(B * nm * C) if want_w else None
    args = (*[t.data_ptr() for t in dev], out.ptr, cam.ptr, None if raw is None else raw.ptr, None if wts is None else wts.ptr, B, HW, C, N, Hd, mode)
    tail = (relu, ops.bx_dtype(K.DTYPES[dt]), ops._stream())
    if wrapper:
        L.check(lib.bx_gradcam_head(*args, *tail), "bx_gradcam_head")
    else:
        L.check(lib.bx_cam_head(*args, CODE[method], *tail), "bx_cam_head")
    label = f"cam_head {method} C={C} HW={HW} N={N} Hd={Hd} mode={mode} {dt}"
    return (out.get(label + " out"), cam.get(label + " cam"), None if raw is None else raw.get(label + " raw"),
            None if wts is None else wts.get(label + " weights"))


def _head_check(got, ref, relu, label):
    out, cam, raw, wts = got
    scale = float(ref.raw.abs().max())
    errs = {"out": rel(out, ref.out.reshape(-1)), "cam": rel(cam, (ref.cam if relu else ref.raw).reshape(-1), scale)}
    if raw is not None:
        errs["raw"] = rel(raw, ref.raw.reshape(-1), scale)
    if wts is not None:
        errs["w"] = rel(wts, ref.w.reshape(-1))
    print(f"[attrib] {label}: {errs}")
    assert max(errs.values()) < CAM_TOL, (label, errs)


@pytest.mark.parametrize("i", range(len(K.HEAD_CASES)), ids=[K.case_id(c) for c in K.HEAD_CASES])
def test_cam_head(i):
    """k_gradcam_head through bx_cam_head: the GAP's eight-loads-per-trip tail, the position reduce's tail (C <= 512) and the one-wave-
    per-position branch (C > 512), the 8-wide class steps (N = 9) and the 16-wide ones over 2N, Hd off the wave and workgroup sizes."""
    c = K.HEAD_CASES[i]
    lib = L.load()
    A, e_lp, wts, ref = K.head_case(i)
    dev = _dev(A, e_lp, *wts)
    shape = (K.HEAD_B, c["HW"], c["C"], c["N"], c["Hd"], c["mode"])
    for relu in (1, 0):
        got = _head(lib, dev, *shape, c["method"], relu, c["dt"], c["raw"], c["wout"])
        _head_check(got, ref, relu, f"cam_head {K.case_id(c)} relu={relu}")
        again = _head(lib, dev, *shape, c["method"], relu, c["dt"], c["raw"], c["wout"])
        assert all(a is None or _bits_equal(a, b) for a, b in zip(got, again)), "a second launch differs"
        if not relu and got[2] is not None:
            assert _bits_equal(got[1], got[2]), "relu = 0: cam is raw"
    if c["mode"] == -2:                                           # the old entry point is method 0
        zero = _head(lib, dev, *shape, "gradcam", 1, c["dt"], True, True)
        wrap = _head(lib, dev, *shape, "gradcam", 1, c["dt"], True, True, wrapper=True)
        assert all(_bits_equal(a, b) for a, b in zip(zero, wrap)), "bx_gradcam_head differs from bx_cam_head with method 0"
        if c["method"] != "gradcam":
            _head_check(zero, R.head(A, e_lp, *wts, -2, "gradcam"), 1, f"cam_head {K.case_id(c)} as Grad-CAM")


# ================================================================================================ c. bx_cam_head_sweep
@pytest.mark.parametrize("i", range(len(K.SWEEP_CASES)), ids=[K.case_id(c) for c in K.SWEEP_CASES])
def test_cam_head_sweep(i):
    """The EEG dense head's Fe tail and the in-kernel up-sampling (256 % (W/4) == 0 and not, odd H, identity, down-sampling), against the
    fp64 reference up-sampled by cam_ref.resize and against bx_cam_head followed by bx_resize_bilinear."""
    c = K.SWEEP_CASES[i]
    lib = L.load()
    B, h, w, H, W, C, N, Hd, Fe, mode = K.HEAD_B, c["h"], c["w"], c["H"], c["W"], c["C"], c["N"], c["Hd"], c["Fe"], c["mode"]
    A, eeg, wts, ref = K.sweep_case(i)
    nm = N if mode == -2 else 1
    Ad, ef, dw, db = _dev(A, *eeg)
    hw = _dev(*wts)
    dtc = ops.bx_dtype(K.DTYPES[c["dt"]])
    label = f"cam_head_sweep {K.case_id(c)}"

    def sweep():
        out, maps = Out(B * N), Out(B * nm * H * W)
        assert maps.ptr % 16 == 0
        L.check(lib.bx_cam_head_sweep(Ad.data_ptr(), ef.data_ptr(), dw.data_ptr(), db.data_ptr(), Fe, *[t.data_ptr() for t in hw], out.ptr,
                                      maps.ptr, B, h, w, C, N, Hd, H, W, mode, CODE[c["method"]], 1, dtc, ops._stream()), "bx_cam_head_sweep")
        return out.get(label + " out"), maps.get(label + " maps")
    out, maps = sweep()
    out2, maps2 = sweep()
    assert _bits_equal(out, out2) and _bits_equal(maps, maps2), "a second launch differs"
    scale = float(ref.raw.abs().max())
    want = torch.from_numpy(R.resize(ref.cam.reshape(B * nm, h, w).numpy(), H, W)).reshape(-1)
    errs = {"out": rel(out, ref.out.reshape(-1)), "maps": rel(maps, want, scale)}
    # the three-launch form on the same inputs: the library's own dense head, bx_cam_head, bx_resize_bilinear
    e_lp = ops.LinearLsmFn.apply(ef, dw, db).contiguous()
    out3, cam3, _, _ = _head(lib, [Ad, e_lp, *hw], B, h * w, C, N, Hd, mode, c["method"], 1, c["dt"], False, False)
    small = cam3.to(DEV)
    up3 = Out(B * nm * H * W)
    L.check(lib.bx_resize_bilinear(small.data_ptr(), up3.ptr, B * nm, h, w, H, W, ops._stream()), "bx_resize_bilinear")
    up3 = up3.get(label + " resize")
    pair = float((maps.double() - up3.double()).abs().max())
    errs["pair"] = pair / (float(up3.abs().max()) + 1e-30)
    print(f"[attrib] {label}: {errs}")
    assert errs["out"] < CAM_TOL and errs["maps"] < CAM_TOL, errs
    assert pair <= PAIR_TOL * float(up3.abs().max()) + 1e-12, errs


# ================================================================================================ d. bx_resize_bilinear
@pytest.mark.parametrize("h,w,H,W", K.RESIZE_PLANES, ids=[f"{h}x{w}-to-{H}x{W}" for h, w, H, W in K.RESIZE_PLANES])
def test_resize_bilinear(h, w, H, W):
    """Measured float32-restatement error 3.952e-6 of max|src| (100x75 -> 7x5), bound RESIZE_BOUND = 1.6e-5 (tests/attrib_cases.py).
    A destination on a 16-byte boundary takes k_resize_bilinear4 when W % 4 == 0; the same buffer one float further, or any other W,
    takes k_resize_bilinear."""
    lib = L.load()
    n = K.RESIZE_N
    src = K.resize_input(h, w)
    want = torch.from_numpy(R.resize(src, H, W)).reshape(-1)
    scale = float(np.abs(src).max())
    sd = torch.from_numpy(src).to(DEV)
    for offset in ((0, 1) if W % 4 == 0 else (0,)):
        label = f"resize {h}x{w} -> {H}x{W} " + ("vector" if W % 4 == 0 and offset == 0 else "scalar") + " kernel"
        runs = []
        for _ in range(2):
            dst = Out(n * H * W, offset)
            assert (dst.ptr % 16 == 0) == (offset == 0)
            L.check(lib.bx_resize_bilinear(sd.data_ptr(), dst.ptr, n, h, w, H, W, ops._stream()), "bx_resize_bilinear")
            runs.append(dst.get(label))
        assert _bits_equal(*runs), "a second launch differs"
        err = rel(runs[0], want, scale)
        print(f"[attrib] {label}: {err:.3e} of max|src| (bound {K.RESIZE_BOUND:.1e})")
        assert err <= K.RESIZE_BOUND, (label, err)
        if (h, w) == (H, W):
            assert _bits_equal(runs[0], torch.from_numpy(src).reshape(-1)), "identity sizes must copy"


# ================================================================================================ e. bx_saliency_reduce
def _saliency(lib, g, npix, C, Cs, scale, dt):
    gd = g.to(DEV).contiguous()
    B = 3 if npix % 3 == 0 else 1                    # (the kernel sees B * HW pixels)
    runs = []
    for _ in range(2):
        out = Out(npix)
        L.check(lib.bx_saliency_reduce(gd.data_ptr(), out.ptr, B, npix // B, C, Cs, scale, ops.bx_dtype(K.DTYPES[dt]), ops._stream()), "bx_saliency_reduce")
        runs.append(out.get(f"saliency C={C} Cs={Cs} npix={npix} {dt} scale={scale}"))
    assert _bits_equal(*runs), "a second launch differs"
    want = torch.from_numpy(R.saliency(g.double().numpy(), C, scale).astype(np.float32))
    assert float(want.max()) < K.PAD / 4 and bool((want[:min(npix, 3)] == torch.tensor([9.0 * scale, 0.0, 0.0])[:min(npix, 3)]).all())
    bad = runs[0].view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"saliency C={C} Cs={Cs} npix={npix} {dt} scale={scale}: {int(bad.sum())} pixels differ, first {int(bad.nonzero()[0])}"


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("C,Cs", K.SALIENCY_CHANNELS)
def test_saliency_reduce(C, Cs, dt):
    """The `c0 + j < C` mask over channels padded with 1e30, C > 8 (a second trip over the channels), both storage types: a maximum
    times a power of two, so bit-equal to the reference."""
    lib = L.load()
    for npix in K.SALIENCY_NPIX:
        g = K.saliency_input(npix, C, Cs, dt)
        for scale in (1.0, 2.0):
            _saliency(lib, g, npix, C, Cs, scale, dt)


@pytest.mark.parametrize("dt,scale", [("f32", 2.0), ("bf16", 1.0)])
def test_saliency_reduce_grid_stride(dt, scale):
    """4096 * 256 + 3 pixels (32 MB in fp32): the last three take a second trip of the grid-stride loop."""
    _saliency(L.load(), K.saliency_input(K.SALIENCY_LARGE, 1, 8, dt), K.SALIENCY_LARGE, 1, 8, scale, dt)
