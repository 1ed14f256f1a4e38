"""The definition of Score-CAM (Wang et al., CVPR-W 2020) as include/brainxai.h pins it, restated with numpy and torch on the CPU --
what brainxai.score_cam and the bx_scorecam_* entry points are tested against.  Nothing here imports the package under test.

A [..., C, h, w] is the target activation (float32; a bf16 activation is widened first, which is exact).  The mask domain [Hm,Wm] is
[H,W] of a spectrogram [B,Cin,H,W] (one value for all channels of a pixel) or [1,T] of an EEG input [B,1,Chans,T] (a time column
across electrodes).  Every product and every sum of ``upsample``, ``mask`` and the rows is a single float32 operation."""
import numpy as np
import torch

from tests import perturb_ref, rise_ref

f32 = np.float32


def axis(n_out, n_in):
    """Output coordinates 0..n_out-1 -> (i0, i1, l): the index rule of bilinear, align_corners=False (csrc/bx_common.h bilinear_src)."""
    scale = f32(n_in) / f32(n_out)
    s = scale * (np.arange(n_out).astype(f32) + f32(0.5)) - f32(0.5)
    s = np.maximum(s, f32(0.0)).astype(f32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0.astype(f32)).astype(f32)


def upsample(A, Hm, Wm):
    """float32 [..., h, w] -> [..., Hm, Wm]: horizontal blend first, then vertical, one float32 rounding per product and per sum."""
    A = np.asarray(A)
    assert A.dtype == f32
    y0, y1, ly = axis(Hm, A.shape[-2])
    x0, x1, lx = axis(Wm, A.shape[-1])
    ly = ly[:, None]
    one = f32(1.0)
    r0, r1 = A[..., y0, :], A[..., y1, :]
    top = (one - lx) * r0[..., x0] + lx * r0[..., x1]
    bot = (one - lx) * r1[..., x0] + lx * r1[..., x1]
    out = (one - ly) * top + ly * bot
    assert out.dtype == f32
    return out


def ranges(U):
    """U [..., Hm, Wm] -> (lo, hi, scale, valid) over the last two axes: the extremes of the UP-SAMPLED plane (a zero extreme is +0.0),
    valid = hi > lo, scale = 1 / (hi - lo) in float32 where valid, else 0."""
    lo = (U.min(axis=(-2, -1)) + f32(0.0)).astype(f32)
    hi = (U.max(axis=(-2, -1)) + f32(0.0)).astype(f32)
    valid = hi > lo
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(valid, f32(1.0) / (hi - lo), f32(0.0)).astype(f32)
    return lo, hi, scale, valid


def mask(U, lo, scale):
    """M = min((U - lo) * scale, 1), float32, in [0, 1]; an invalid channel (scale 0) gives 0 everywhere."""
    m = np.minimum((U - lo[..., None, None]) * scale[..., None, None], f32(1.0))
    assert m.dtype == f32
    return m


def rows(x, M, baseline, b0=0, nb=None, k0=0, n=None):
    """x [B,Cin,H,W] or [B,1,Chans,T], M float32 [B,C,Hm,Wm] -> the perturbed rows (b, k), b in b0..b0+nb-1, k in k0..k0+n-1,
    sample-major: base + M_k (x - base) with three roundings (tests/rise_ref.py::perturbed)."""
    nb = x.shape[0] - b0 if nb is None else nb
    n = M.shape[1] - k0 if n is None else n
    out = []
    for b in range(b0, b0 + nb):
        bb = baseline[b:b + 1] if isinstance(baseline, torch.Tensor) and baseline.dim() == 4 else baseline
        out += [rise_ref.perturbed(x[b:b + 1], M[b, k], bb) for k in range(k0, k0 + n)]
    return torch.cat(out)


def weights(P, P_base, valid, mode):
    """P [B,C,K], P_base [B,K] -> w [B,K,C] in P's dtype: P[b,k,c] ('prob') or P[b,k,c] - P_base[b,c] ('increase'); 0 where invalid."""
    P = np.asarray(P)
    w = P if mode == "prob" else P - np.asarray(P_base, dtype=P.dtype)[:, None, :]
    return np.where(np.asarray(valid)[:, :, None], w, P.dtype.type(0)).transpose(0, 2, 1)


def combine(w, A):
    """w [B,K,C], A [B,C,h,w] -> (raw fp64 [B,K,h,w] = sum_k w_k A_k, mag fp64 = sum_k |w_k A_k|)."""
    w, A = np.asarray(w, dtype=np.float64), np.asarray(A, dtype=np.float64)
    return np.einsum("bkc,bchw->bkhw", w, A), np.einsum("bkc,bchw->bkhw", np.abs(w), np.abs(A))


def scores(f, x, M, baseline=0.0, chunk=64):
    """f: perturbed input [R,...] of ONE sample -> log-probabilities [R,K] (torch; called as f(b, rows)).  Returns P [B,C,K] fp64:
    the softmax probabilities of sample b seen through channel k."""
    per = []
    for b in range(M.shape[0]):
        bb = baseline[b:b + 1] if isinstance(baseline, torch.Tensor) and baseline.dim() == 4 else baseline
        per.append(perturb_ref.sweep(lambda xs: f(b, xs), x[b:b + 1], M[b], bb, rise_ref.perturbed, "prob", False, chunk))
    return np.concatenate(per)
