"""numpy fp64 restatement of TCAV (include/brainxai.h, "TCAV") that does not share the algebra under test: no Gram matrix and no dual
coefficients.  Ridge is solved in the PRIMAL, on the centred activations of the problem's fit rows,
    (X^T X + lambda I) w = X^T (y - ybar),    lambda = ridge tr(X X^T) / rows,
by a dense solve of the D x D system while D <= PRIMAL_DENSE_MAX; beyond it (the end-to-end targets reach D = 16384, a 2 GiB matrix) the
same normal equations are solved in the basis of the right singular vectors of X, in which they are diagonal: with lambda > 0 the
solution lies in the row space of X, so w = V diag(s / (s^2 + lambda)) U^T (y - ybar) is the same w.  The mean difference is computed
literally.  Decision values, accuracies, scores and Welch's test come from their definitions.  A plain module: no tests."""
import math

import numpy as np

PRIMAL_DENSE_MAX = 4200
U64 = 2.0 ** -53


def problems(Q, R):
    """[(concept index or -1, random index, positive set, negative set)] in the package's order: concept problems (q, r), q major, then
    the null problems (N_r, N_{(r+1) % R}) when R >= 2.  Set s is the s-th of the Q concept sets followed by the R random sets."""
    return [(q, r, q, Q + r) for q in range(Q) for r in range(R)] + ([(-1, r, Q + r, Q + (r + 1) % R) for r in range(R)] if R >= 2 else [])


def held_out(n, holdout):
    """The number of examples at the end of a set that are kept out of the fit: ceil(h n)."""
    return int(math.ceil(holdout * n - 1e-12))


def primal_ridge(X, y, ridge):
    """X fp64 [rows, D] (uncentred fit rows), y +-1 -> (w, lambda, mean of X, ybar)."""
    mu, ybar = X.mean(axis=0), float(y.mean())
    Xc = X - mu
    lam = ridge * float((Xc * Xc).sum()) / X.shape[0]
    r = y - ybar
    if X.shape[1] <= PRIMAL_DENSE_MAX:
        w = np.linalg.solve(Xc.T @ Xc + lam * np.eye(X.shape[1]), Xc.T @ r)
    else:
        U, s, Vt = np.linalg.svd(Xc, full_matrices=False)
        w = Vt.T @ ((s / (s * s + lam)) * (U.T @ r))
    return w, lam, mu, ybar


def fit(pos, neg, classifier, ridge, holdout):
    """One problem from the activations pos, neg fp64 [n, D] -> dict(w, norm, v, lam, decision [2n] (positives first, held-out rows
    included), accuracy, holdout_accuracy (NaN without held-out rows), cond_bound)."""
    n = pos.shape[0]
    nh = held_out(n, holdout)
    keep = np.arange(n) < n - nh
    X = np.concatenate([pos[keep], neg[keep]])
    y = np.concatenate([np.ones(int(keep.sum())), -np.ones(int(keep.sum()))])
    allrows = np.concatenate([pos, neg])
    ally = np.concatenate([np.ones(n), -np.ones(n)])
    fitmask = np.concatenate([keep, keep])
    if classifier == "ridge":
        w, lam, mu, ybar = primal_ridge(X, y, ridge)
        decision = (allrows - mu) @ w + ybar
        cond = X.shape[0] / ridge + 1.0
    else:
        mp, mn = pos[keep].mean(axis=0), neg[keep].mean(axis=0)
        w, lam, cond = mp - mn, 0.0, 1.0
        decision = allrows @ w - 0.5 * (mp @ w + mn @ w)
    norm = float(np.sqrt(w @ w))
    hit = np.where(decision > 0, 1.0, -1.0) == ally
    return dict(w=w, norm=norm, v=w / norm if norm > 0 else w, lam=lam, decision=decision, accuracy=float(hit[fitmask].mean()),
                holdout_accuracy=float(hit[~fitmask].mean()) if nh else float("nan"), cond_bound=cond, rows=X.shape[0],
                radius=float(np.sqrt(((allrows - X.mean(axis=0)) ** 2).sum(axis=1)).max()))


def fit_all(sets, Q, classifier="ridge", ridge=1e-2, holdout=0.0):
    """sets: the Q concept sets followed by the R random sets, fp64 [n, D] each -> the problems' fits in the package's order."""
    R = len(sets) - Q
    return [fit(sets[sp], sets[sn], classifier, ridge, holdout) for _, _, sp, sn in problems(Q, R)]


def fit_tolerance(rows, D, cond):
    """The relative bound of a fit: 16 (rows + D) 2^-53 cond.  The dual route rounds G0 (D + 2 roundings per entry), centres it and
    factorises it (Cholesky: a backward error of about 3 rows 2^-53 |K|, turned into a forward error by cond(K + lambda I) <= rows / ridge
    + 1); the primal route does the same with D in the place of rows and the same condition number.  4 (rows + D) 2^-53 cond on either
    side, and a factor 2 for the second-order terms."""
    return 16.0 * (rows + D) * U64 * cond


def sensitivities(G, V):
    """S[r, p] = G[r] . V[p], fp64."""
    return np.asarray(G, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T


def scores(S, classes, K):
    """S fp64 [rows, P], classes int [rows] -> (score, mean, mean_abs fp64 [P, K], counts [K]); NaN for a class without rows."""
    P = S.shape[1]
    out = [np.full((P, K), np.nan) for _ in range(3)]
    counts = np.zeros(K, dtype=np.int64)
    for k in range(K):
        sel = S[np.asarray(classes) == k]
        counts[k] = sel.shape[0]
        if sel.shape[0]:
            out[0][:, k] = (sel > 0).sum(axis=0) / sel.shape[0]
            out[1][:, k] = sel.sum(axis=0) / sel.shape[0]
            out[2][:, k] = np.abs(sel).sum(axis=0) / sel.shape[0]
    return out[0], out[1], out[2], counts


def welch(a, b):
    """Welch's two-sided test of two 1-D samples from its definition -> (t, dof, p); NaN when a sample has fewer than 2 values or a
    variance is 0.  The Student t tail is scipy's."""
    from scipy import stats
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size < 2 or b.size < 2:
        return (float("nan"),) * 3
    va, vb = a.var(ddof=1) / a.size, b.var(ddof=1) / b.size
    if not (va > 0 and vb > 0):
        return (float("nan"),) * 3
    t = (a.mean() - b.mean()) / math.sqrt(va + vb)
    dof = (va + vb) ** 2 / (va ** 2 / (a.size - 1) + vb ** 2 / (b.size - 1))
    return float(t), float(dof), float(2.0 * stats.t.sf(abs(t), dof))


def planted(n, D, c, seed, sets=2):
    """``sets`` example sets fp64 [n, D] of unit Gaussian activations, the first carrying + c d along a random unit direction d."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(D)
    d /= np.sqrt(d @ d)
    out = [rng.standard_normal((n, D)) for _ in range(sets)]
    out[0] = out[0] + c * d
    return out, d
