"""numpy fp64 restatement of TracIn (include/brainxai.h, "TracIn"), operation by operation: every sequential sum is a loop over the
summed index, vectorised over rows or pairs, every product and sum a separate numpy operation (one rounding each).  It also holds the
selection rule as a stable sort.  A plain module: no tests."""
import math

import numpy as np

LOG2E = 1.4426950408889634
LN2_HI = 0.6931471803691238
LN2_LO = 1.9082149292705877e-10
EXP_C = [1.0 / math.factorial(i) for i in range(14)]
LOG_C = [1.0 / (2 * i + 3) for i in range(11)]
MULTIMODAL_LAYERS = ("fc2", "fc1", "eeg_model.dense", "spectrogram_model.fc")


def _f64(x):
    """fp32 values (what the kernels read) or fp64 ones (the CPU tests' exact chain) as fp64, unchanged."""
    return np.asarray(x).astype(np.float64)


def exp(x):
    """The header's exp on an fp64 array."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        xc = np.where(np.isfinite(x), np.clip(x, -708.0, 709.0), 0.0)
        n = np.rint(xc * LOG2E)
        r = (xc - n * LN2_HI) - n * LN2_LO
        p = np.full_like(r, EXP_C[13])
        for i in range(12, -1, -1):
            p = p * r + EXP_C[i]
        out = np.ldexp(p, n.astype(np.int32))
        out = np.where(x < -708.0, 0.0, out)
        out = np.where(x > 709.0, np.inf, out)
        return np.where(np.isnan(x), x, out)


def log(x):
    """The header's log on an fp64 array of positive finite values."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    low = m < 0.7071067811865476
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e).astype(np.float64)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = np.full_like(z, LOG_C[10])
    for i in range(9, -1, -1):
        p = p * z + LOG_C[i]
    t = 2.0 * s
    return e * LN2_HI + ((t + t * (z * p)) + e * LN2_LO)


def seq_sum(terms, axis=-1):
    """Sequential sum over ``axis`` in ascending index from +0."""
    terms = np.moveaxis(np.asarray(terms, dtype=np.float64), axis, 0)
    s = np.zeros(terms.shape[1:], dtype=np.float64)
    for k in range(terms.shape[0]):
        s = s + terms[k]
    return s


def targets(target, K):
    """fp32 [n,K] distributions, or integer labels [n] -> their one-hot rows; fp64 [n,K]."""
    target = np.asarray(target)
    if target.ndim == 1:
        return (target[:, None] == np.arange(K)[None, :]).astype(np.float64)
    return target.astype(np.float64)


def loss_and_seed(logp, target):
    """-> (T [n], loss [n], delta = T p - t [n,K]) from fp32 logp [n,K] and targets as ``targets`` takes them."""
    lp = _f64(logp)
    t = targets(target, lp.shape[1])
    T = seq_sum(t, axis=1)
    with np.errstate(all="ignore"):
        terms = np.where(t > 0.0, t * (log(np.where(t > 0.0, t, 1.0)) - lp), 0.0)
        loss = seq_sum(terms, axis=1)
        delta = T[:, None] * exp(lp) - t
    return T, loss, delta


def factors_single(logp, target):
    """-> (delta fp64 [n,K], loss fp64 [n])."""
    _, loss, d = loss_and_seed(logp, target)
    return d, loss


def factors_multimodal(logp, target, hidden, e, s, w1, w2):
    """-> (delta fp64 [n, K + Hd + K + K] = delta_2 | delta_1 | delta_e | delta_s, loss fp64 [n]).  w1 fp32 [Hd,2K], w2 fp32 [K,Hd]."""
    _, loss, d2 = loss_and_seed(logp, target)
    K = d2.shape[1]
    h, w1, w2 = _f64(hidden), _f64(w1), _f64(w2)
    with np.errstate(all="ignore"):
        u = seq_sum(w2[None, :, :] * d2[:, :, None], axis=1)                      # [n,Hd], over the rows k of W2
        d1 = np.where(h > 0, u, 0.0)
        v = seq_sum(w1[None, :, :] * d1[:, :, None], axis=1)                      # [n,2K], over the rows h of W1
        ve, vs = v[:, :K], v[:, K:]
        de = ve - exp(_f64(e)) * seq_sum(ve, axis=1)[:, None]
        ds = vs - exp(_f64(s)) * seq_sum(vs, axis=1)[:, None]
    return np.concatenate([d2, d1, de, ds], axis=1), loss


def pair_dot(A, B):
    """[n,W] x [m,W] -> [n,m]: the sequential sum over the features of the rounded products."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    s = np.zeros((A.shape[0], B.shape[0]), dtype=np.float64)
    for f in range(A.shape[1]):
        s = s + A[:, f][:, None] * B[:, f][None, :]
    return s


def layer_terms(train, test, dwidth, mask=None):
    """train / test: (delta fp64 [n, sum dwidth], [act fp32 [n, awidth_l]]) -> the list of the selected layers' terms [n,m] in layer
    order (None for a layer the mask leaves out)."""
    out, off = [], 0
    for l, w in enumerate(dwidth):
        if mask is None or mask >> l & 1:
            dd = pair_dot(train[0][:, off:off + w], test[0][:, off:off + w])
            aa = pair_dot(_f64(train[1][l]), _f64(test[1][l]))
            out.append(dd * (aa + 1.0))
        else:
            out.append(None)
        off += w
    return out


def checkpoint_scores(train, test, dwidth, mask=None):
    """sum_l of the selected layers' terms from +0, in layer order."""
    s = None
    for t in layer_terms(train, test, dwidth, mask):
        if t is not None:
            s = (np.zeros_like(t) if s is None else s) + t
    return s


def scores(checkpoints, etas, dwidth, mask=None):
    """checkpoints: [(train, test)] as ``layer_terms`` takes them -> S fp64 [n,m]: the first checkpoint stores eta * sum, the later add."""
    S = None
    for (train, test), eta in zip(checkpoints, etas):
        t = float(eta) * checkpoint_scores(train, test, dwidth, mask)
        S = t if S is None else S + t
    return S


def self_influence(checkpoints, etas, dwidth, mask=None):
    """checkpoints: [side] -> fp64 [n]: the diagonal of ``scores`` of every side against itself, computed row by row."""
    out = None
    for side, eta in zip(checkpoints, etas):
        s, off = None, 0
        for l, w in enumerate(dwidth):
            if mask is None or mask >> l & 1:
                d = side[0][:, off:off + w]
                a = _f64(side[1][l])
                term = seq_sum(d * d, axis=1) * (seq_sum(a * a, axis=1) + 1.0)
                s = (np.zeros_like(term) if s is None else s) + term
            off += w
        t = float(eta) * s
        out = t if out is None else out + t
    return out


def select(S, k, largest):
    """S fp64 [N,M] -> (idx int32 [M,k], val fp64 [M,k]): per column the k largest (smallest) values, sorted by value, ties by ascending
    row, -0.0 equal to +0.0, NaN last -- a stable sort."""
    S = np.asarray(S, dtype=np.float64)
    key = np.where(S == 0.0, 0.0, S)
    key = -key if largest else key
    key = np.where(np.isnan(key), np.inf, key)
    idx = np.empty((S.shape[1], k), dtype=np.int32)
    val = np.empty((S.shape[1], k), dtype=np.float64)
    for j in range(S.shape[1]):
        order = np.argsort(key[:, j], kind="stable")[:k]
        idx[j], val[j] = order, S[order, j]
    return idx, val
