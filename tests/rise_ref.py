"""The definition of RISE saliency (Petsiuk et al., BMVC 2018) restated with numpy and torch on the CPU -- what brainxai.rise /
brainxai.rise_masks and the bx_rise_* entry points are tested against.  Nothing here imports the package under test.

Mask domain [Hm,Wm]: [H,W] of a spectrogram [B,C,H,W] (one value for all channels of a pixel), [Chans,T] of an EEG input
[B,1,Chans,T], or [1,T] (a time column across electrodes).  Grid gh x gw, cell size ch = ceil(Hm / gh), cw = ceil(Wm / gw).
Mask n is the crop [dy:dy+Hm, dx:dx+Wm] of the bilinear, align_corners=False up-sampling of bits[n] to (gh+1) ch x (gw+1) cw."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.perturb_ref import baseline_tensor, sweep  # noqa: F401  (baseline_tensor is part of this module's interface)

f32 = np.float32


def cells(Hm, Wm, gh, gw):
    return -(-Hm // gh), -(-Wm // gw)


def draw(N, gh, gw, Hm, Wm, p1, seed):
    """(bits uint8 [N,gh,gw], shifts int32 [N,2] = (dy, dx)) from one RandomState(seed), in the order of the definition."""
    ch, cw = cells(Hm, Wm, gh, gw)
    rs = np.random.RandomState(seed)
    bits = (rs.rand(N, gh, gw) < p1).astype(np.uint8)
    dy = rs.randint(0, ch, N)
    dx = rs.randint(0, cw, N)
    return bits, np.stack([dy, dx], axis=1).astype(np.int32)


def axis(u, g, c):
    """Up-sampled coordinates u (int array) -> (i0, i1, l): every operation a single float32 one."""
    scale = f32(g) / f32((g + 1) * c)
    s = (u.astype(f32) + f32(0.5)) * scale - f32(0.5)
    s = np.maximum(s, f32(0.0)).astype(f32)
    i0 = np.minimum(s.astype(np.int64), g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    return i0, i1, (s - i0.astype(f32)).astype(f32)


def masks(bits, shifts, Hm, Wm):
    """float32 [N,Hm,Wm], the closed form: horizontal blend first, then vertical, one float32 rounding per product and per sum."""
    bits = np.asarray(bits)
    N, gh, gw = bits.shape
    ch, cw = cells(Hm, Wm, gh, gw)
    out = np.empty((N, Hm, Wm), dtype=f32)
    one = f32(1.0)
    for n in range(N):
        v = (bits[n] != 0).astype(f32)
        y0, y1, ly = axis(np.arange(Hm) + int(shifts[n][0]), gh, ch)
        x0, x1, lx = axis(np.arange(Wm) + int(shifts[n][1]), gw, cw)
        lx, ly = lx[None, :], ly[:, None]
        top = ((one - lx) * v[y0][:, x0]).astype(f32) + (lx * v[y0][:, x1]).astype(f32)
        bot = ((one - lx) * v[y1][:, x0]).astype(f32) + (lx * v[y1][:, x1]).astype(f32)
        out[n] = ((one - ly) * top.astype(f32)).astype(f32) + (ly * bot.astype(f32)).astype(f32)
    return out


def masks_interpolate(bits, shifts, Hm, Wm):
    """The same masks the way the paper's code builds them: up-sample the whole grid (F.interpolate), then crop."""
    bits = np.asarray(bits)
    N, gh, gw = bits.shape
    ch, cw = cells(Hm, Wm, gh, gw)
    up = F.interpolate(torch.from_numpy((bits != 0).astype(f32))[:, None], size=((gh + 1) * ch, (gw + 1) * cw), mode="bilinear", align_corners=False)[:, 0]
    return np.stack([up[n, int(dy):int(dy) + Hm, int(dx):int(dx) + Wm].numpy() for n, (dy, dx) in enumerate(np.asarray(shifts))])


def perturbed(x, m, baseline):
    """base + m * (x - base) in x's dtype, three roundings.  x [B,C,H,W] or [B,1,Chans,T]; m one mask [Hm,Wm] (Hm = 1: a time-column
    mask, applied to every electrode)."""
    base = baseline_tensor(baseline, x).expand_as(x)
    mm = torch.as_tensor(np.asarray(m)).to(x.dtype).reshape(1, 1, m.shape[0], m.shape[1])
    return base + mm * (x - base)


def denominator(m, p1, normalize):
    """D [Hm,Wm] in fp64."""
    cov = m.astype(np.float64).sum(0)
    return cov if normalize == "coverage" else np.full(cov.shape, np.float64(m.shape[0]) * np.float64(p1))


def saliency(P, m, p1, normalize="expected"):
    """P [B,N,K], m float32 [N,Hm,Wm] -> fp64 [B,K,Hm,Wm] = sum_n P[b,n,k] m_n / D; a cell no mask reached gets 0."""
    D = denominator(m, p1, normalize)
    num = np.einsum("bnk,nhw->bkhw", np.asarray(P, dtype=np.float64), m.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D > 0, num / D, 0.0)


def scores(f, x, m, baseline=0.0, chunk=64):
    """f: perturbed input [R,...] -> log-probabilities [R,K] (torch).  Returns P [B,N,K] fp64 numpy: softmax probabilities of sample b
    seen through mask n.  f sees mask-major batches [n*B, ...]."""
    return sweep(f, x, m, baseline, perturbed, "prob", False, chunk)
