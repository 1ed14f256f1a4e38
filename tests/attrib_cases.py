"""The shapes and seeded inputs of tests/test_gpu_attrib_kernels.py, shared with tests/test_attrib_ref_cpu.py, which measures on the
references alone what the GPU bounds rest on.  Nothing here imports the package under test.

Every set of sizes is derived from the loops of csrc/attrib.hip it is meant to leave and re-enter:
  k_cam / cam_colsum   a position's channels sit on lpp = min(C/8, 64) lanes, ppw = 64 / lpp positions per wave, four groups of four
                       waves per trip: T = 16 ppw positions (= 4 slots of cam_colsum, slots = 2048 / C, for C <= 512)
  k_gradcam_head       the GAP takes 8 slots positions per trip and the position reduce (C <= 512) 32 ppw: both 16384 / C
  HW in {1, ppw - 1, ppw + 1, T - 1, T + 1, 2 T + ppw + 1}: less than a group, a ragged group, a ragged trip, a third trip."""
import functools
import math

import numpy as np
import torch

from tests import cam_ref as R

f32 = np.float32
METHODS = ("gradcam", "gradcam++", "layercam")
COND_MIN = 1e-2                # the Grad-CAM++ denominators stay this clear of cancellation (tests/test_gpu_cam_methods.py)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _hws(ppw, T):
    return tuple(sorted({hw for hw in (1, ppw - 1, ppw + 1, T - 1, T + 1, 2 * T + ppw + 1) if hw > 0}))


# ================================================================================================ a. bx_cam_reduce
REDUCE_B = 2
REDUCE_CS = (8, 64, 256, 512, 2048)
REDUCE_NMS = (1, 5)


def reduce_hws(C):
    ppw = 64 // min(C // 8, 64)
    return _hws(ppw, 16 * ppw)


REDUCE_SHAPES = tuple((C, hw) for C in REDUCE_CS for hw in reduce_hws(C))


@functools.lru_cache(maxsize=None)
def reduce_case(C, HW, nm, dt):
    """-> (A [B, HW, C], G [B*nm, HW, C] in the stored dtype, {method: (raw, w, cond, sg)} in fp64 from the stored values).  Drawn as
    test_cam_reduce_against_fp64_definition draws them (the same seed search for the Grad-CAM++ conditioning); the zeroed gradient
    entries leave the last position alone, so that a clamped load that is added instead of masked changes the sums."""
    B, dtype = REDUCE_B, DTYPES[dt]
    for seed in range(1000, 1010):
        g = torch.Generator().manual_seed(seed + HW + C + nm)
        A = (torch.rand(B, HW, C, generator=g) * 2.0 - 0.5).to(dtype)
        G = (torch.randn(B * nm, HW, C, generator=g) * 1e-2).to(dtype)
        last = G[:, HW - 1].clone()
        G[:, ::5, ::3] = 0.0
        G[:, HW - 1] = last
        A64 = A.double().permute(0, 2, 1).repeat_interleave(nm, 0)                 # [B*nm, C, HW], exactly the stored values
        G64 = G.double().permute(0, 2, 1)
        refs = {m: R.cam(A64, G64, m) for m in METHODS}
        if refs["gradcam++"][2] >= COND_MIN:
            break
    assert refs["gradcam++"][2] >= COND_MIN, "no seed keeps the Grad-CAM++ denominators clear of cancellation"
    assert bool((A[:, HW - 1] != 0).all()) and bool((G[:, HW - 1] != 0).all())
    return A, G, refs


# ================================================================================================ b. bx_cam_head
HEAD_B = 2
HEAD_MARGIN = 1e-4             # smallest |hidden pre-activation| / arg-max lead a case may have: 100 x the fp32 error of either


def head_hws(C):
    if C > 512:                                   # one wave per position; the GAP trip is 16 (C = 1024) or 8 (C = 2048) positions
        return (1, 3, 5, 16384 // C + 1)
    return _hws(512 // C, 16384 // C)


def _head_cases():
    shapes = [(C, hw) for C in (8, 64, 512, 1024, 2048) for hw in head_hws(C)] + [(64, 9)]
    Ns, Hds = (3, 6, 9, 3, 6, 9, 6), (1, 100, 300, 100, 300)
    cases = []
    for i, (C, HW) in enumerate(shapes):
        N = 1 if i == len(shapes) - 1 else Ns[i % len(Ns)]
        mode = (-2, -1, N - 1)[(i + i // 3) % 3]
        method = METHODS[(i + i // 3 + i // 9) % 3]
        cases.append(dict(C=C, HW=HW, N=N, Hd=Hds[i % len(Hds)], mode=mode, method=method, dt=("f32", "bf16")[(i + i // 2) % 2],
                          raw=i % 4 != 1, wout=method != "layercam" and i % 5 != 2))
    return tuple(cases)


HEAD_CASES = _head_cases()


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k not in ("raw", "wout"))


def _head_weights(g, C, N, Hd):
    fcw, fcb = R._uniform((N, C), (6.0 / C) ** 0.5, g) * 4, R._uniform((N,), 0.1, g)
    w1, b1 = R._uniform((Hd, 2 * N), (6.0 / (2 * N)) ** 0.5, g), R._uniform((Hd,), 0.1, g)
    w2, b2 = R._uniform((N, Hd), (6.0 / Hd) ** 0.5, g), R._uniform((N,), 0.1, g)
    return [fcw, fcb, w1, b1, w2, b2]


def _head_search(draw, B, N, mode, method):
    """The first of ten seeds whose reference is a fair fp32 target: every ReLU decision of the hidden layer and the arg-max decided by
    more than HEAD_MARGIN, no sample whose maps are all zero (a dead hidden layer), and for Grad-CAM++ -- after fc_w is scaled by the
    power of two that brings the largest |S G| of a counted element to <= 1/2 (clear_scale of tests/test_gpu_cam_methods.py) -- the
    denominators COND_MIN clear of cancellation.  Every criterion is a property of the fp64 reference."""
    why = None
    for seed in range(10):
        A, eeg, wts = draw(seed)
        ref = R.head(A, eeg, *wts, mode, method)
        if method == "gradcam++":
            for _ in range(4):
                if ref.sg <= 0.5:
                    break
                wts[0] = wts[0] * 2.0 ** -math.ceil(math.log2(ref.sg / 0.5))
                ref = R.head(A, eeg, *wts, mode, method)
        alive = N == 1 or bool((ref.raw.reshape(B, -1).abs().max(1).values > 0).all())
        why = (ref.margin, ref.lead, ref.sg, ref.cond, alive)
        if ref.margin >= HEAD_MARGIN and (mode != -1 or ref.lead >= HEAD_MARGIN) and ref.sg <= 0.5 and ref.cond >= COND_MIN and alive:
            return A, eeg, wts, ref
    raise AssertionError(f"no seed gives a fair reference (margin, lead, |S G|, conditioning, alive) = {why}")


@functools.lru_cache(maxsize=None)
def head_case(i):
    """-> (A [B, HW, C] stored dtype, e_lp [B, N], [fcw, fcb, w1, b1, w2, b2], the fp64 reference of tests/cam_ref.head)."""
    c = HEAD_CASES[i]
    B, C, HW, N, Hd = HEAD_B, c["C"], c["HW"], c["N"], c["Hd"]

    def draw(seed):
        g = R._gen(7000 + 10 * i + seed)
        A = torch.rand(B, HW, C, generator=g).to(DTYPES[c["dt"]])
        e_lp = torch.log_softmax(torch.randn(B, N, generator=g) * 2, 1)
        return A, e_lp, _head_weights(g, C, N, Hd)
    A, e_lp, wts, ref = _head_search(draw, B, N, c["mode"], c["method"])
    assert bool((A[:, HW - 1] != 0).all())
    return A, e_lp, wts, ref


# ================================================================================================ c. bx_cam_head_sweep
SWEEP_PLANES = ((2, 4, 64, 128), (3, 5, 7, 12), (3, 5, 10, 20), (1, 7, 1, 28), (4, 4, 4, 4), (5, 6, 3, 4), (2, 3, 9, 100))


def _sweep_cases():
    Cs, Fes = (8, 256, 1024), (1, 63, 65, 300)
    cases = []
    for i in range(2 * len(SWEEP_PLANES)):
        h, w, H, W = SWEEP_PLANES[i % len(SWEEP_PLANES)]
        cases.append(dict(h=h, w=w, H=H, W=W, C=Cs[(i + i // 7) % 3], Fe=Fes[i % 4], N=(6, 3)[i % 2], Hd=(100, 64)[i // 7],
                          mode=(-2, -1)[(i + i // 7) % 2], method=METHODS[(i + i // 3) % 3], dt=("f32", "bf16")[(i // 2) % 2]))
    return tuple(cases)


SWEEP_CASES = _sweep_cases()


@functools.lru_cache(maxsize=None)
def sweep_case(i):
    """-> (A [B, h*w, C], (eeg_feat [B, Fe], dense_w [N, Fe], dense_b [N]), the six head tensors, the fp64 reference)."""
    c = SWEEP_CASES[i]
    B, C, HW, N, Hd, Fe = HEAD_B, c["C"], c["h"] * c["w"], c["N"], c["Hd"], c["Fe"]

    def draw(seed):
        g = R._gen(9000 + 10 * i + seed)
        A = torch.rand(B, HW, C, generator=g).to(DTYPES[c["dt"]])
        ef = torch.randn(B, Fe, generator=g)
        dw, db = R._uniform((N, Fe), (6.0 / Fe) ** 0.5, g), R._uniform((N,), 0.1, g)
        assert bool((ef[:, Fe - 1] != 0).all()) and bool((dw[:, Fe - 1] != 0).all())
        return A, (ef, dw, db), _head_weights(g, C, N, Hd)
    return _head_search(draw, B, N, c["mode"], c["method"])


# ================================================================================================ d. bx_resize_bilinear
RESIZE_N = 3
#                1 pixel      scalar kernel  vector kernel  identity                        down-sampling
RESIZE_PLANES = ((1, 1, 5, 7), (7, 5, 100, 75), (2, 4, 64, 128), (16, 24, 16, 24), (5, 7, 5, 7), (9, 13, 4, 6), (100, 75, 7, 5),
                 (1, 500, 1, 2000),       # N H W / 4 = 1500: the last workgroup of the vector kernel is ragged
                 (3, 3, 6, 10),
                 (3, 5, 7, 12),           # N H W / 4 = 63: less than one workgroup
                 (7, 5, 600, 601))        # W % 4 != 0 and N H W = 1 081 800 > 4096 * 256: the scalar kernel's grid-stride loop
# worst |resize_f32 - resize| / max|src| over RESIZE_PLANES on these inputs: 3.952e-6, at 100x75 -> 7x5 (every other plane stays below
# 4.7e-7; tests/test_attrib_ref_cpu.py prints each and asserts this figure): the fp32 rounding of the source coordinate -- up to 93
# at a scale of 100/7 -- times the neighbour difference.  The GPU bound is four times this: csrc/attrib.hip is built with
# -ffp-contract=fast while the restatement rounds every product.
RESIZE_WORST_F32 = 4.0e-6
RESIZE_BOUND = 4 * RESIZE_WORST_F32


@functools.lru_cache(maxsize=None)
def resize_input(h, w):
    """float32 [3, h, w], unit-variance noise: neighbouring pixels differ by O(1), so a wrong index or clamp is an O(1) error."""
    return np.random.default_rng(500 + 31 * h + w).standard_normal((RESIZE_N, h, w)).astype(f32)


# ================================================================================================ e. bx_saliency_reduce
SALIENCY_CHANNELS = ((1, 8), (3, 8), (4, 8), (8, 8), (9, 16), (16, 16), (3, 16))
SALIENCY_NPIX = (1, 255, 257)
SALIENCY_LARGE = 4096 * 256 + 3                 # one pixel-thread per pixel up to 4096 workgroups of 256: three pixels take a second trip
PAD = 1e30                                      # what the padded channels C .. Cs-1 hold: an unmasked one decides every maximum


def saliency_input(npix, C, Cs, dt, seed=0):
    """[npix, Cs] in the stored dtype.  Pixel 0 has its largest magnitude negative, pixel 1 is all zero, pixel 2 all -0.0."""
    g = torch.randn(npix, Cs, generator=R._gen(300 + seed + npix % 1000 + 17 * C + Cs))
    g[0, C - 1] = -9.0
    if npix > 1:
        g[1, :C] = 0.0
    if npix > 2:
        g[2, :C] = -0.0
    g[:, C:] = PAD
    g = g.to(DTYPES[dt])
    assert npix <= 3 or bool((g[npix - 1, :C] != 0).all())
    return g
