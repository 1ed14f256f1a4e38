"""numpy / torch-fp64 restatement of brainxai.gradient_shap (the definition is pinned in include/brainxai.h):

    phi[b,c,e] = (1/n) * sum_{k=0..n-1} d[b,k,e] * dF_c/dx( r[b,k] )[e]
    d[b,k] = x[b] - bg[idx[b,k]]                      (one fp32 rounding)
    r[b,k] = bg[idx[b,k]] + fl(alpha[b,k] * d[b,k])   (product and sum rounded separately)

with F_c the model's output log-probability.  Rows are numbered j = b * n + k, sample-major."""
import numpy as np
import torch


def draws(seed, B, Nb, n):
    """(idx int32 [B,n], alpha fp32 [B,n]): one default_rng(seed); per sample the background indices, then the interpolation points --
    what oracle.ref_torch.expected_gradients consumes."""
    rng = np.random.default_rng(seed)
    idx, alpha = np.empty((B, n), dtype=np.int32), np.empty((B, n), dtype=np.float32)
    for b in range(B):
        idx[b] = rng.integers(0, Nb, size=n)
        alpha[b] = rng.random(n).astype(np.float32)
    return idx, alpha


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def diffs(x, bg, idx):
    """d fp32 [B*n, ...]"""
    x, bg = _np32(x), _np32(bg)
    B, n = idx.shape
    return (x[:, None] - bg[idx]).astype(np.float32).reshape(B * n, *x.shape[1:])


def rows(x, bg, idx, alpha):
    """r fp32 [B*n, ...]: three separate fp32 roundings (numpy float32 arithmetic never fuses)."""
    x, bg = _np32(x), _np32(bg)
    B, n = idx.shape
    base = bg[idx].reshape(B * n, *x.shape[1:])
    d = diffs(x, bg, idx)
    a = np.asarray(alpha, dtype=np.float32).reshape(B * n, *([1] * (x.ndim - 1)))
    ad = (a * d).astype(np.float32)
    return (base + ad).astype(np.float32)


def accumulate(x, bg, idx, g, acc=None, slot=0, Kc=1, row0=0):
    """acc fp64 [B,Kc,per] += the sum over the rows row0 .. row0 + len(g) - 1, per sample in ascending k, of d * g in fp64; g fp32
    [rows, ...].  Returns (acc, absacc) with absacc the same sum of |d * g| (for error bounds)."""
    B, n = idx.shape
    d = diffs(x, bg, idx).reshape(B * n, -1).astype(np.float64)
    g = np.asarray(g, dtype=np.float32).reshape(len(g), -1).astype(np.float64)
    per = d.shape[1]
    acc = np.zeros((B, Kc, per)) if acc is None else acc
    absacc = np.zeros((B, per))
    for r in range(len(g)):
        j = row0 + r
        acc[j // n, slot] += d[j] * g[r]
        absacc[j // n] += np.abs(d[j] * g[r])
    return acc, absacc


def finish(acc, n, shape, channels=None):
    """values fp32 [B,Kc,*shape] = fl32(acc / n); map fp32 [B,Kc,H,W] = fl32 of the fp64 sum over the channels (spectrogram: channels = C)
    or values without the unit axis (EEG: channels None)."""
    B, Kc, _ = acc.shape
    v = (acc / n).reshape(B, Kc, *shape)
    values = v.astype(np.float32)
    if channels is None:
        return values, values[:, :, 0]
    m = np.zeros((B, Kc, *shape[1:]))
    for c in range(channels):
        m += v[:, :, c]
    return values, m.astype(np.float32)


def values(model64, x, bg, idx, alpha, other=None, input="eeg"):
    """phi fp64 [B,K,*x.shape[1:]] of an fp64 torch model on the fp32 rows of the restatement.  A two-input model (other given) takes
    (eeg, spec) with the other input the sample's own, repeated over the draws."""
    B, n = idx.shape
    d = torch.from_numpy(diffs(x, bg, idx)).double().reshape(B, n, *x.shape[1:])
    r = torch.from_numpy(rows(x, bg, idx, alpha)).double().reshape(B, n, *x.shape[1:])
    out = None
    was_training = model64.training
    model64.eval()
    for b in range(B):
        xi = r[b].clone().requires_grad_(True)
        if other is None:
            y = model64(xi)
        else:
            o = other[b:b + 1].double().expand(n, *other.shape[1:]).contiguous()
            y = model64(xi, o) if input == "eeg" else model64(o, xi)
        if out is None:
            out = torch.zeros(B, y.shape[1], *x.shape[1:], dtype=torch.float64)
        for c in range(y.shape[1]):
            (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
            out[b, c] = (g * d[b]).sum(0) / n
    model64.train(was_training)
    return out


def channel_importance(v, top=None):
    """mean |v| over the last axis in fp64 -> fp64 [...]; with top the indices of the n largest along the new last axis, descending, ties
    by the lower index (computed on the fp32 rounding, which is what is ranked)."""
    v = np.asarray(v, dtype=np.float64)
    imp = np.abs(v).sum(-1) / v.shape[-1]
    if top is None:
        return imp
    order = np.argsort(-imp.astype(np.float32), axis=-1, kind="stable")
    return imp, order[..., :top]
