"""The definition of Kernel SHAP (Lundberg & Lee, NeurIPS 2017; paired sampling: Covert & Lee, AISTATS 2021) restated with numpy and
torch on the CPU in fp64 -- what brainxai.kernel_shap and the bx_shap_* entry points are tested against.  Nothing here imports the
package under test.

Players and coalitions.  The players are the M labels 0..M-1 of an int label map seg over the input's map domain: [H,W] of a
spectrogram [B,C,H,W] (a cell is a pixel with all its channels), [Chans,T] or [1,T] of an EEG input [B,1,Chans,T].  One label map serves
the whole batch.  A coalition z in {0,1}^M shows the input on the cells whose label is in z and the baseline elsewhere.  v_b,k(z) is the
class score ('prob' or 'logprob') of sample b, class k; v(1) is the unperturbed input, v(0) the baseline.

Values.  phi[b,k,.] minimises sum_n w_n (v(z_n) - phi0 - sum_i phi_i z_ni)^2 subject to phi0 = v(0) and sum_i phi_i = v(1) - v(0).
The constraint is eliminated on the last player: Xt[n,i] = z_ni - z_n,M-1 for i < M-1, yt_n = v(z_n) - v(0) - z_n,M-1 D with
D = v(1) - v(0); (Xt' W Xt) phi' = Xt' W yt, phi_M-1 = D - sum phi'.

Coalition set.  Exact, when 2^M - 2 <= num_samples: every proper non-empty coalition in increasing order of the integer whose bit i is
player i, w = (M-1) / (C(M,s) s (M-s)), s = |z|.  Sampled, otherwise: N = num_samples rounded down to even,
rng = numpy.random.default_rng(seed), sizes = rng.choice(arange(1, M), size=N//2, p ~ (M-1) / (s (M-s))), row 2j is
rng.permutation(M)[:sizes[j]], row 2j+1 its complement, all weights 1."""
import math

import numpy as np
import torch

from tests.perturb_ref import baseline_tensor, score_fn, sweep  # noqa: F401  (baseline_tensor is part of this module's interface)


def coalition_set(M, num_samples, seed=0):
    """-> (Z uint8 [N,M], w fp64 [N], exact)."""
    if 2 ** M - 2 <= num_samples:
        Z = np.array([[(c >> i) & 1 for i in range(M)] for c in range(1, 2 ** M - 1)], dtype=np.uint8)
        s = Z.sum(1)
        return Z, np.array([(M - 1) / (math.comb(M, int(k)) * int(k) * (M - int(k))) for k in s]), True
    N = num_samples // 2 * 2
    rng = np.random.default_rng(seed)
    k = np.arange(1, M)
    p = (M - 1) / (k * (M - k))
    sizes = rng.choice(k, size=N // 2, p=p / p.sum())
    Z = np.zeros((N, M), dtype=np.uint8)
    for j, s in enumerate(sizes):
        Z[2 * j, rng.permutation(M)[:s]] = 1
        Z[2 * j + 1] = 1 - Z[2 * j]
    return Z, np.ones(N), False


def grid_segments(H, W, rows, cols):
    """int32 [H,W]: rows x cols tiles, label = row * cols + col, tile r holds the y with (y * rows) // H == r."""
    return ((np.arange(H)[:, None] * rows // H) * cols + (np.arange(W)[None, :] * cols // W)).astype(np.int32)


def masks(seg, Z):
    """bool [N,Hm,Wm]: True where coalition n shows the input."""
    return np.asarray(Z).astype(bool)[:, np.asarray(seg)]


def perturbed(x, m, baseline):
    """x [B,C,H,W] or [B,1,Chans,T] seen through one coalition's mask m (bool [Hm,Wm]; Hm = 1 applies to every electrode): x where m,
    the baseline elsewhere -- a selection (torch.where)."""
    base = baseline_tensor(baseline, x).expand_as(x)
    mm = torch.as_tensor(np.asarray(m)).reshape(1, 1, m.shape[0], m.shape[1]).expand_as(x)
    return torch.where(mm, x, base)


def reduced(Z, w):
    """-> (Xt fp64 [N,M-1], last fp64 [N,1], A = Xt' W Xt)."""
    Z = np.asarray(Z, dtype=np.float64)
    last = Z[:, -1:]
    Xt = Z[:, :-1] - last
    return Xt, last, (Xt * np.asarray(w, dtype=np.float64)[:, None]).T @ Xt


def gram_cond(Z, w):
    return float(np.linalg.cond(reduced(Z, w)[2]))


def fit(Z, w, Y, v0, v1, how="normal"):
    """Z [N,M], w [N], Y [N,R] (the scores of R games), v0 / v1 [R] -> phi fp64 [R,M].  how='normal': the normal equations by Cholesky;
    'lstsq': numpy's lstsq on the sqrt(w)-scaled system."""
    w = np.asarray(w, dtype=np.float64)
    Y, v0, v1 = (np.asarray(a, dtype=np.float64) for a in (Y, v0, v1))
    Xt, last, A = reduced(Z, w)
    d = v1 - v0
    yt = (Y - v0) - last * d
    if how == "normal":
        Lc = np.linalg.cholesky(A)
        head = np.linalg.solve(Lc.T, np.linalg.solve(Lc, (Xt * w[:, None]).T @ yt))
    else:
        sw = np.sqrt(w)[:, None]
        head = np.linalg.lstsq(Xt * sw, yt * sw, rcond=None)[0]
    return np.vstack([head, d - head.sum(0)]).T


def values(Z, w, S, clean, empty, how="normal"):
    """S [B,N,K], clean / empty [B,K] -> phi fp64 [B,K,M]."""
    S = np.asarray(S, dtype=np.float64)
    B, N, K = S.shape
    phi = fit(Z, w, S.transpose(1, 0, 2).reshape(N, B * K), np.asarray(empty, dtype=np.float64).reshape(-1), np.asarray(clean, dtype=np.float64).reshape(-1), how)
    return phi.reshape(B, K, -1)


def solution_operator(Z, w):
    """fp64 [M, N+2]: phi = Op @ (v(z_0), ..., v(z_N-1), v(1), v(0)) -- the fit is linear in the scores."""
    N = np.asarray(Z).shape[0]
    Y = np.hstack([np.eye(N), np.zeros((N, 2))])
    return fit(Z, w, Y, np.eye(N + 2)[N + 1], np.eye(N + 2)[N]).T


def amplification(Z, w):
    """The largest absolute row sum of the solution operator: an error of e on every score moves a value by at most amp * e."""
    return float(np.abs(solution_operator(Z, w)).sum(1).max())


def brute_force(M, v):
    """Shapley values by the definition.  v: fp64 [2^M], the value of the coalition whose bit i is player i."""
    phi = np.zeros(M)
    for i in range(M):
        for c in range(2 ** M):
            if not (c >> i) & 1:
                s = bin(c).count("1")
                phi[i] += math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) * (v[c | (1 << i)] - v[c])
    return phi


def coalition_index(Z):
    """The integer whose bit i is player i, per row."""
    return (np.asarray(Z, dtype=np.int64) << np.arange(np.asarray(Z).shape[1], dtype=np.int64)).sum(1)


def scores(f, x, m, baseline=0.0, score="prob", chunk=32):
    """f: input rows [R,...] -> log-probabilities (or logits) [R,K] (torch).  Returns (S [B,N,K], clean [B,K], empty [B,K]) fp64 numpy:
    the softmax probability (score='logprob': its logarithm) of sample b under coalition n, of the unperturbed sample and of the
    baseline.  f sees coalition-major batches [n*B, ...]: the samples of coalition n0, then those of n0 + 1, ..."""
    S, clean = sweep(f, x, m, baseline, perturbed, score, True, chunk)
    with torch.no_grad():
        empty = score_fn(score)(f(perturbed(x, np.zeros_like(m[0]), baseline))).numpy()
    return S, clean, empty


def all_coalition_values(M, game):
    """fp64 [2^M]: game(z) for every z, indexed by coalition_index."""
    return np.array([game(np.array([(c >> i) & 1 for i in range(M)], dtype=np.uint8)) for c in range(2 ** M)])
