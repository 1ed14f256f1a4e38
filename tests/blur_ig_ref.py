"""numpy / torch-fp64 restatement of brainxai.blur_ig (the definition is pinned in include/brainxai.h):

    sigma_i = i max_sigma / n (sqrt: its square root), i = 0..n, in Python floats;   w_i = -(sigma_{i+1} - sigma_i)
    R(s) = int(4 s + 0.5),  g_s[t] = exp(-0.5 / s^2 t^2) / sum_t exp(..),  t = -R..R;  g_0 = the identity
    a = g_{sigma_i},  b = g_{sigma_i + eps},  d = (b - a) / eps in fp64 with a zero-padded to b's radius;  each rounded to fp32 once
    both axes:  X_i = A_y A_x x,  D_i = B_y (D_x x) + D_y (A_x x);     one axis:  X_i = A x,  D_i = D x      (zero padding outside the image)
    values[b,c] = sum_i w_i dF_c/dx(X_i) D_i;    delta[b,c] = sum_e values - (F_c(x) - F_c(blur_{sigma_n}(x)))

with F_c the model's output log-probability.  Rows are numbered j = b * n + i, sample-major.  The filters here are fp64 correlations of
the fp32 taps (the device's are fp32 fmaf chains: compared under a bound, not bit for bit); accumulate and the row sum are exact."""
import math

import numpy as np
import torch
from scipy import ndimage

AXES = {"hw": (2, 3), "h": (2,), "w": (3,)}                # of an array [B, C, H, W]


def sigmas(steps, max_sigma, sqrt=False):
    if sqrt:
        return [math.sqrt(float(i) * max_sigma / float(steps)) for i in range(0, steps + 1)]
    return [float(i) * max_sigma / float(steps) for i in range(0, steps + 1)]


def weights(sig):
    return np.array([-(sig[i + 1] - sig[i]) for i in range(len(sig) - 1)], dtype=np.float64)


def radius(s):
    return int(4.0 * float(s) + 0.5)


def taps64(s):
    """fp64 [2 R + 1]: scipy.ndimage's Gaussian taps at truncate 4; the identity where R = 0."""
    R = radius(s)
    if R == 0:
        return np.ones(1)
    t = np.arange(-R, R + 1)
    phi = np.exp(-0.5 / (s * s) * t ** 2)
    return phi / phi.sum()


def step_taps(s, eps, dtype=np.float32):
    """(a, b, d) fp32 [2 R_b + 1] of one step, and (R_a, R_b); dtype=np.float64 keeps them unrounded (for the comparison with scipy)."""
    a, b = taps64(s), taps64(s + eps)
    Ra, Rb = len(a) // 2, len(b) // 2
    a_pad = np.zeros(2 * Rb + 1)
    a_pad[Rb - Ra:Rb + Ra + 1] = a
    return a_pad.astype(dtype), b.astype(dtype), ((b - a_pad) / eps).astype(dtype), (Ra, Rb)


def table(sig, eps):
    """The device's tap table of the scales ``sig``: (taps fp32 [E,3,TW], radius int32 [E,2])."""
    steps = [step_taps(s, eps) for s in sig]
    Rmax = max(r[1] for *_, r in steps)
    taps, rad = np.zeros((len(sig), 3, 2 * Rmax + 1), dtype=np.float32), np.zeros((len(sig), 2), dtype=np.int32)
    for e, (a, b, d, (Ra, Rb)) in enumerate(steps):
        rad[e] = Ra, Rb
        for f, v in enumerate((a, b, d)):
            taps[e, f, Rmax - Rb:Rmax + Rb + 1] = v
    return taps, rad


def _filter(x, taps, axis):
    return ndimage.correlate1d(x, np.asarray(taps, dtype=np.float64), axis=axis, mode="constant", cval=0.0)


def step_rows(x, s, eps, axes, dtype=np.float32):
    """(X, D) fp64 of x [B,C,H,W] at one scale, in the decomposed form, from the fp32 taps (dtype=np.float64: from unrounded ones)."""
    x = np.asarray(x, dtype=np.float64)
    a, b, d, _ = step_taps(s, eps, dtype)
    ax = AXES[axes]
    if len(ax) == 1:
        return _filter(x, a, ax[0]), _filter(x, d, ax[0])
    ha, hd = _filter(x, a, 3), _filter(x, d, 3)
    return _filter(ha, a, 2), _filter(hd, b, 2) + _filter(ha, d, 2)


def path(x, sig, eps, axes, dtype=np.float32):
    """(rows, deriv) fp64 [B, n, C, H, W] for the scales sig[0..n-1]."""
    pairs = [step_rows(x, s, eps, axes, dtype) for s in sig]
    return np.stack([p[0] for p in pairs], 1), np.stack([p[1] for p in pairs], 1)


def blur(x, s, axes):
    """x [B,C,H,W] blurred with one sigma or one per sample, fp64, from the fp32 taps."""
    x = np.asarray(x, dtype=np.float64)
    ss = np.broadcast_to(np.asarray(s, dtype=np.float64), (len(x),))
    out = np.empty_like(x)
    for i, si in enumerate(ss):
        a = taps64(float(si)).astype(np.float32)
        y = x[i:i + 1]
        for axis in AXES[axes]:
            y = _filter(y, a, axis)
        out[i] = y[0]
    return out


def rows_bound(x, s, eps, axes):
    """The kernel's error bounds (bX, bD), fp64 [B] per sample, for one scale.  A chain of T fmaf has T roundings: its error is at most
    T u sum|t_i x_i| (u = 2^-24, to first order).  One axis: X within (T + 1) u A_a M and D within (T + 1) u A_d M, with A = sum |fp32
    taps|, M = max |x| of the sample, T = the taps that can land inside the image = min(2 R_b + 1, extent), and 1 for the second-order
    terms (T u < 1 / T up to T = 4096).  Both axes: the horizontal results carry T_x u A M each and are rounded inside that count; the
    vertical chain of X has T_y terms, that of D 2 T_y; so X within (T_x + T_y + 2) u A_a^2 M and D within
    (2 T_y + T_x + 2) u (A_b A_d + A_d A_a) M."""
    x = np.asarray(x, dtype=np.float64)
    a, b, d, (Ra, Rb) = step_taps(s, eps)
    Aa, Ab, Ad = (float(np.abs(v.astype(np.float64)).sum()) for v in (a, b, d))
    M = np.abs(x).reshape(len(x), -1).max(1)
    H, W = x.shape[2:]
    u = 2.0 ** -24
    Ty, Tx = min(2 * Rb + 1, H), min(2 * Rb + 1, W)
    if axes == "hw":
        return (Tx + Ty + 2) * u * Aa * Aa * M, (2 * Ty + Tx + 2) * u * (Ab * Ad + Ad * Aa) * M
    T = Ty if axes == "h" else Tx
    return (T + 1) * u * Aa * M, (T + 1) * u * Ad * M


def accumulate(g, D, w, B, n, acc=None, slot=0, Kc=1, row0=0):
    """acc fp64 [B,Kc,per] += over the rows row0 .. row0 + len(g) - 1, per sample in ascending step, of w[i] * (g * D): g * D of two
    floats is exact in fp64, the product with w and the sum are one rounding each."""
    g = np.asarray(g, dtype=np.float32).reshape(len(g), -1).astype(np.float64)
    D = np.asarray(D, dtype=np.float32).reshape(len(D), -1).astype(np.float64)
    acc = np.zeros((B, Kc, g.shape[1])) if acc is None else acc
    for r in range(len(g)):
        j = row0 + r
        acc[j // n, slot] += w[j % n] * (g[r] * D[r])
    return acc


def sum_rows(v):
    """fp64 [R]: the sum of every row of v fp32 [R, L] in the device's order: 64 partial sums over t = l, l + 64, ... in ascending t, then
    the xor butterfly with offsets 32, 16, .., 1 (lane 0's value)."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    R, Ln = v.shape
    part = np.zeros((R, 64))
    for t0 in range(0, Ln, 64):
        m = min(64, Ln - t0)
        part[:, :m] += v[:, t0:t0 + m]
    lanes = np.arange(64)
    o = 32
    while o:
        part = part + part[:, lanes ^ o]
        o >>= 1
    return part[:, 0].copy()


def two_input(model64, other, input, n=1):
    """forward(rows) of a two-input fp64 model: the other input is the sample's own, each repeated over n consecutive rows."""
    o = torch.as_tensor(other).double().repeat_interleave(n, dim=0)
    return (lambda xi: model64(xi, o)) if input == "eeg" else (lambda xi: model64(o, xi))


def values(forward, rows, deriv, w):
    """(values fp64 [B,K,*trail], scale fp64 [B,K]) of ``forward`` -- an fp64 model or any callable taking all B * n rows, sample-major,
    at once -- on rows and deriv [B,n,*trail] (any float dtype): values = sum_i w_i dF_c/dx(rows_i) deriv_i, and
    scale = sum_i |w_i| max|g_i| max|D_i|, what the end-to-end bound multiplies."""
    r = torch.as_tensor(rows).double()
    D = torch.as_tensor(deriv).double()
    B, n = r.shape[:2]
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).view(1, n, *([1] * (r.dim() - 2)))
    xi = r.reshape(B * n, *r.shape[2:]).clone().requires_grad_(True)
    y = forward(xi)
    vals = torch.zeros(B, y.shape[1], *r.shape[2:], dtype=torch.float64)
    scale = torch.zeros(B, y.shape[1], dtype=torch.float64)
    dmax = D.abs().flatten(2).max(2).values                                     # [B, n]
    for c in range(y.shape[1]):
        (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
        g = g.reshape(B, n, *r.shape[2:])
        vals[:, c] = (wt * g * D).sum(1)
        scale[:, c] = (wt.flatten(1).abs() * g.abs().flatten(2).max(2).values * dmax).sum(1)
    return vals, scale


def outputs(forward, x):
    """fp64 [B,K]: the model's output on x."""
    with torch.no_grad():
        return forward(torch.as_tensor(x).double())
