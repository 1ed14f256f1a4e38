"""numpy / torch-fp64 restatement of brainxai.infidelity and brainxai.sensitivity_max (the definitions are pinned in include/brainxai.h):

    infidelity       I[b,k,cell] = fl32(sigma[b] * z[b,k,cell])            z: smooth_grad's stream (tests/smooth_grad_ref.noise) over the cells
                     row[b,k,e]  = fl32(x[b,e] - I[b,k,cell(e)])            two separate fp32 roundings
                     d[b,c,k]    = sum_cell (double)I * (double)Phi[b,c,cell]
                     Delta[b,c,k] = (double)s_c(x[b]) - (double)s_c(row[b,k])
                     infid[b,c]  = (1/n) sum_k (beta d - Delta)^2,   beta = 1 or (sum_k d Delta) / (sum_k d d), 0 when that sum is 0
    sensitivity_max  u[b,k,e]    = (w >> 8) 2^-23 - 1,  w = word e & 3 of Philox4x32-10(counter = (e >> 2, k, b, 1), key = seed's two halves)
                     row[b,k,e]  = fl32(x[b,e] + fl32(r[b] * u[b,k,e]))
                     sens[b]     = max_k ||Phi(row[b,k]) - Phi(x[b])||_2 / ||Phi(x[b])||_2,   the denominator 1 when the norm is 0

Cells: the elements of the input, or with ``grouped`` the pixels [H,W] of a spectrogram [C,H,W] (one draw moves all channels) / the time
columns [T] of an EEG input [1,Chans,T] (one draw moves all electrodes).  Rows are numbered j = b * n + k, sample-major.  Everything
from z32 (fp32, the device's own dump or any array) on is exact; the uniform draws are exact from the words (no libm in them)."""
import numpy as np
import torch

from tests.smooth_grad_ref import philox


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


# ---- infidelity -------------------------------------------------------------------------------------------------------------------------
def noise_per_element(I, x_shape, grouped, eeg):
    """I fp32 [B,n,cells] -> [B,n,*x_shape[1:]]: the noise every element of the input sees."""
    B, n = I.shape[:2]
    if not grouped:
        return I.reshape(B, n, *x_shape[1:])
    if eeg:                                                                   # cells = T, shared by the electrodes
        return np.broadcast_to(I.reshape(B, n, 1, 1, x_shape[3]), (B, n, *x_shape[1:]))
    return np.broadcast_to(I.reshape(B, n, 1, x_shape[2], x_shape[3]), (B, n, *x_shape[1:]))     # cells = H*W, shared by the channels


def perturbation(sig, z32):
    """I fp32 [B,n,cells] = fl32(sigma * z) of z32 fp32 [B,n,...] (flattened over the cells)."""
    z32 = _np32(z32)
    B, n = z32.shape[:2]
    s = np.asarray(sig, dtype=np.float32).reshape(B, 1, 1)
    return (s * z32.reshape(B, n, -1)).astype(np.float32)


def rows(x, sig, z32, grouped=False, eeg=False):
    """fp32 [B*n, *x.shape[1:]] = fl32(x - fl32(sigma * z)): numpy float32 never fuses."""
    x = _np32(x)
    I = noise_per_element(perturbation(sig, z32), x.shape, grouped, eeg)
    return (x[:, None] - I).astype(np.float32).reshape(-1, *x.shape[1:])


def dots(I, phi):
    """d fp64 [B,Kc,n] and the bound's sum |I Phi| [B,Kc,n]; I fp32 [B,n,cells], phi [B,Kc,cells]."""
    I64, p64 = I.astype(np.float64), np.asarray(phi, dtype=np.float32).astype(np.float64)
    prod = I64[:, None, :, :] * p64[:, :, None, :]                              # [B,Kc,n,cells], every product exact
    return prod.sum(-1), np.abs(prod).sum(-1)


def drops(clean, S):
    """Delta fp64 [B,K,n] from the scores of the clean input [B,K] and of the rows [B,n,K]."""
    return np.asarray(clean, dtype=np.float64)[:, :, None] - np.asarray(S, dtype=np.float64).transpose(0, 2, 1)


def finish(d, delta, normalize=False):
    """(infid, beta) fp64 [B,Kc] of d, Delta fp64 [B,Kc,n], operation by operation in ascending k as the definition orders them."""
    B, Kc, n = d.shape
    infid, beta = np.zeros((B, Kc)), np.ones((B, Kc))
    for b in range(B):
        for c in range(Kc):
            if normalize:
                sdd = sd2 = 0.0
                for k in range(n):
                    sdd += d[b, c, k] * delta[b, c, k]
                    sd2 += d[b, c, k] * d[b, c, k]
                beta[b, c] = 0.0 if sd2 == 0.0 else sdd / sd2
            s = 0.0
            for k in range(n):
                t = beta[b, c] * d[b, c, k] - delta[b, c, k]
                s += t * t
            infid[b, c] = s / n
    return infid, beta


def infidelity(score, x, sig, z32, phi, grouped=False, eeg=False, normalize=False):
    """The whole definition for ``score``: fp32-valued rows [R,...] (a torch fp64 tensor) -> scores [R,K] (tensor or array).  phi
    [B,Kc,cells] with Kc = K (every class) or, with one class per sample already selected by ``score``, Kc = K = 1.
    -> (infid [B,Kc], beta [B,Kc], d [B,Kc,n], Delta [B,Kc,n])."""
    x = _np32(x)
    z32 = _np32(z32)
    B, n = z32.shape[:2]
    I = perturbation(sig, z32)
    r = rows(x, sig, z32, grouped, eeg)
    with torch.no_grad():
        S = np.asarray(score(torch.from_numpy(r).double()), dtype=np.float64).reshape(B, n, -1)
        clean = np.asarray(score(torch.from_numpy(x).double()), dtype=np.float64)
    d, _ = dots(I, phi)
    delta = drops(clean, S)
    return finish(d, delta, normalize) + (d, delta)


# ---- sensitivity_max --------------------------------------------------------------------------------------------------------------------
def uniform(B, n, per, seed, word3=1):
    """u fp32 [B,n,per], exact: (w >> 8) 2^-23 - 1 with w the word e & 3 of the block of counter (e >> 2, k, b, word3)."""
    seed = int(seed)
    Q = (per + 3) // 4
    q = np.arange(Q, dtype=np.uint64)[None, None, :]
    k = np.arange(n, dtype=np.uint64)[None, :, None]
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    w = philox((q, k, b, np.uint64(word3)), (seed & 0xFFFFFFFF, seed >> 32))     # [4, B, n, Q]
    w = np.moveaxis(w, 0, -1).reshape(B, n, Q * 4)[:, :, :per]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return u.astype(np.float32)


def uniform_rows(x, radius, u32):
    """fp32 [B*n, *x.shape[1:]] = fl32(x + fl32(r * u)) of u32 fp32 [B,n,...]."""
    x, u32 = _np32(x), _np32(u32)
    B, n = u32.shape[:2]
    r = np.asarray(radius, dtype=np.float32).reshape(B, *([1] * (u32.ndim - 1)))
    dl = (r * u32.reshape(B, n, *x.shape[1:])).astype(np.float32)
    return (x[:, None] + dl).astype(np.float32).reshape(B * n, *x.shape[1:])


def distances(phi_rows, phi_clean, n):
    """(dist fp64 [B,n], norms fp64 [B]) of explanations [B*n,...] and [B,...] (fp32 values), sums in fp64."""
    a = np.asarray(phi_rows, dtype=np.float64).reshape(len(phi_rows), -1)
    c = np.asarray(phi_clean, dtype=np.float64).reshape(len(phi_clean), -1)
    B = len(c)
    diff = a.reshape(B, n, -1) - c[:, None]
    return np.sqrt((diff * diff).sum(-1)), np.sqrt((c * c).sum(-1))


def sens_finish(dist, norms):
    return dist.max(1) / np.where(norms == 0.0, 1.0, norms)


def sensitivity(explain, x, radius, u32):
    """explain: rows [R,...] (torch fp64) -> explanations [R,...].  -> (sens [B], dist [B,n], norms [B])."""
    x = _np32(x)
    n = u32.shape[1]
    r = uniform_rows(x, radius, u32)
    dist, norms = distances(np.asarray(explain(torch.from_numpy(r).double())), np.asarray(explain(torch.from_numpy(x).double())), n)
    return sens_finish(dist, norms), dist, norms
