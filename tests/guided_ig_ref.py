"""numpy restatements of brainxai.guided_ig (Guided Integrated Gradients, Kapishnikov et al., CVPR 2021; the definition is pinned in
include/brainxai.h).  For one row (a (sample, class) pair of P cells), n steps, fraction, max_dist and k = floor((P - 1) fraction):

    L_total = sum |x_in - x_base|;   X(alpha) = x_base + alpha (x_in - x_base), x_in for alpha >= 1 and x_base for alpha <= 0
    step i:  alpha = (i + 1) / n, a_min = max(alpha - max_dist, 0), a_max = min(alpha + max_dist, 1), L_target = L_total (1 - alpha),
             g = grad F(x) once; then passes:
        x_old = x;  a_e = (x_e - x_base_e) / (x_in_e - x_base_e) (a_max where x_in_e == x_base_e);  x_e = X(a_min)_e where a_e < a_min
        L_cur = sum |x_in - x|;  math.isclose(L_target, L_cur, rel_tol=1e-9, abs_tol=1e-9):  attr += (x - x_old) g, the step ends
        key_e = |g_e|, +inf where x_e == X(a_max)_e (arrived);  theta = the k-th smallest key;  S = {not arrived, key <= theta}
        L_S = sum_S |X(a_max) - x|;  gamma = (L_cur - L_target) / L_S, +inf when L_S = 0
        on S:  gamma > 1: x = X(a_max);  0 < gamma <= 1: x += gamma (X(a_max) - x);  gamma <= 0: nothing
        attr += (x - x_old) g;  go on while gamma > 1 and L_S > 0

(a) ``literal``: the algorithm as it stands, everything in fp64, with a caller-supplied grad_func; optionally it carries, cell by cell,
    a bound of how far restatement (b) may be from it (``Bound`` below).
(b) ``init`` / ``step``: the header's definition with its fp32 storage (x, g and every X(alpha) are fp32, each formed in fp64 and
    rounded once) and the device's order of the three sums (``row_sum``), rows r = b * Kc + slot, windows of rows: what the kernels are
    compared with bit for bit."""
import math

import numpy as np

THREADS = 1024
OK, CAP, NAN = 0, 1, 2
U = 2.0 ** -24                                             # |fl32(v) - v| <= U |v|


def rank_k(P, fraction):
    return int(math.floor((P - 1) * float(fraction)))


def pass_cap(P, k):
    return -(-P // (k + 1)) + 2


def window(i, n, max_dist):
    alpha = (i + 1) / n
    return max(alpha - max_dist, 0.0), min(alpha + max_dist, 1.0), 1.0 - alpha


def row_sum(v):
    """The device's sum of fp64 v [P]: 1024 partial sums over e = t, t + 1024, ... in ascending e; inside every 64 consecutive partials
    the xor butterfly with offsets 32, 16, .., 1; the 16 totals in ascending order."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros(THREADS)
    for e0 in range(0, len(v), THREADS):
        m = min(THREADS, len(v) - e0)
        part[:m] += v[e0:e0 + m]
    part = part.reshape(THREADS // 64, 64)
    lanes = np.arange(64)
    o = 32
    while o:
        part = part + part[:, lanes ^ o]
        o >>= 1
    t = part[0, 0]
    for w in range(1, THREADS // 64):
        t = t + part[w, 0]
    return float(t)


def _close(a, b):
    return math.isclose(a, b, rel_tol=1e-9, abs_tol=1e-9)


def _select(keys, arrived, k):
    keys = np.where(arrived, np.inf, keys)
    theta = np.partition(keys, k)[k]
    return ~arrived & (keys <= theta)


def _decisions(clamped, S, gamma, more):
    """A pass as the decisions it took: (the cells the clamp moved, the cells selected -- none when the pass ended at step 4 --, whether
    they went all the way (gamma > 1), whether another pass follows).  A pass that ends at step 4 and one that finds S empty are the
    same pass: nothing but the clamp moves and the step ends."""
    S = np.zeros(len(clamped), dtype=bool) if S is None else np.asarray(S)
    return clamped.copy(), S.copy(), bool(gamma > 1) and bool(S.any()), bool(more)


# ---- (a) the algorithm in fp64 -----------------------------------------------------------------------------------------------------------
class Bound:
    """Cell by cell, how far restatement (b) may be from (a) while both make the same decisions (clamps, ends, S, gamma > 1), to first
    order with the second-order products kept.  e bounds |x_b - x_a|, ea bounds |attr_b - attr_a|; grad_err(e) bounds |grad F(x_b) -
    grad F(x_a)| given e.  The rules (u = 2^-24; both restatements form X(alpha) in the same fp64 operations, (b) rounds it to fp32):
        gradient      dg = grad_err(e) + u |g|                                      ((b) rounds its gradient to fp32)
        clamped cell  e = u |X_min|                                                 (whatever it was before)
        L_cur         dL = sum e + 2^-50 P L_cur                                    (the sums differ in order only)
        gamma > 1     e = u |X_max| on S
        gamma <= 1    dLS = sum_S (e + u |X_max|),  dN = dL + 2^-50 L_total,  dgam = (dN + gamma dLS) / (L_S - dLS)  (inf when L_S <= dLS)
                      on S:  e' = e + (gamma + dgam) (e + u |X_max|) + dgam |X_max - x| + u (|x'| + the rest)
        every pass    ea += (e + e_old) |g| + |x - x_old| dg + (e + e_old) dg
    and fl32(attr) adds u |attr|."""

    def __init__(self, P, grad_err):
        self.e, self.ea, self.grad_err = np.zeros(P), np.zeros(P), grad_err

    def values_bound(self, attr):
        return self.ea + U * (np.abs(attr) + self.ea)


def literal(x_in, x_base, grad_func, steps, fraction, max_dist, cap=None, bound=None, largest_first=False):
    """-> dict(attr fp64 [P], x fp64 [P], iters [steps], status, trace).  trace[i] is the list of the step's passes, each
    the tuple of ``_decisions``: what (b) has to share for ``bound`` to hold.
    largest_first: the selection inverted (the cells with the LARGEST |g| move first), for discrimination checks."""
    x_in, x_base = np.asarray(x_in, dtype=np.float64).ravel(), np.asarray(x_base, dtype=np.float64).ravel()
    P, n = len(x_in), int(steps)
    k = rank_k(P, fraction)
    cap = pass_cap(P, k) if cap is None else cap
    d = x_in - x_base
    L_total = float(np.abs(d).sum())
    x, attr = x_base.copy(), np.zeros(P)
    iters, trace, status = np.zeros(n, dtype=np.int32), [], OK

    def point(alpha):
        return x_in.copy() if alpha >= 1 else (x_base.copy() if alpha <= 0 else x_base + alpha * d)
    for i in range(n):
        trace.append([])
        if status != OK or L_total == 0:
            continue
        a_min, a_max, left = window(i, n, max_dist)
        x_min, x_max, L_target = point(a_min), point(a_max), L_total * left
        g = np.asarray(grad_func(x.copy()), dtype=np.float64).ravel()
        if np.isnan(g).any():
            status = NAN
            continue
        dg = None if bound is None else bound.grad_err(bound.e) + U * np.abs(g)
        while True:
            iters[i] += 1
            x_old = x.copy()
            e_old = None if bound is None else bound.e.copy()
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.where(d == 0, a_max, (x - x_base) / d)
            clamped = (a < a_min) & (x != x_min)                    # a cell already at X_min may be sent there again: no move
            x[clamped] = x_min[clamped]
            if bound is not None:
                bound.e[clamped] = U * np.abs(x_min[clamped])
            L_cur = float(np.abs(x_in - x).sum())
            dL = None if bound is None else bound.e.sum() + 2.0 ** -50 * P * L_cur
            ended = _close(L_target, L_cur)
            S, more, gamma = None, False, 0.0
            if not ended:
                arrived = x == x_max
                S = _select(-np.abs(g) if largest_first else np.abs(g), arrived, k)
                L_S = float(np.abs(x_max - x)[S].sum())
                gamma = (L_cur - L_target) / L_S if L_S > 0 else math.inf
                more = gamma > 1 and L_S > 0
                if gamma > 1:
                    x[S] = x_max[S]
                    if bound is not None:
                        bound.e[S] = U * np.abs(x_max[S])
                elif gamma > 0:
                    gap = (x_max - x)[S]
                    x[S] = x[S] + gamma * gap
                    if bound is not None:
                        eS, um = bound.e[S], U * np.abs(x_max[S])
                        dLS = float((eS + um).sum())
                        dgam = (dL + 2.0 ** -50 * L_total + gamma * dLS) / (L_S - dLS) if L_S > dLS else math.inf
                        rest = eS + (gamma + dgam) * (eS + um) + dgam * np.abs(gap)
                        bound.e[S] = rest + U * (np.abs(x[S]) + rest)
            attr += (x - x_old) * g
            if bound is not None:
                bound.ea += (bound.e + e_old) * np.abs(g) + np.abs(x - x_old) * dg + (bound.e + e_old) * dg
            trace[i].append(_decisions(clamped, S, gamma, more))
            if not more:
                break
            if iters[i] >= cap:
                status = CAP
                break
    return dict(attr=attr, x=x, iters=iters, status=status, trace=trace, L_total=L_total, k=k, cap=cap)


def left_riemann(x_in, x_base, grad_func, steps):
    """sum_i grad F(X(i/n)) (X((i+1)/n) - X(i/n)) in fp64: what max_dist = 0 has to give."""
    x_in, x_base = np.asarray(x_in, dtype=np.float64).ravel(), np.asarray(x_base, dtype=np.float64).ravel()
    d = x_in - x_base
    pts = [x_base.copy()] + [x_in.copy() if i == steps else x_base + (i / steps) * d for i in range(1, steps + 1)]
    return sum(np.asarray(grad_func(pts[i].copy()), dtype=np.float64).ravel() * (pts[i + 1] - pts[i]) for i in range(steps))


# ---- (b) the header's definition: fp32 storage, the device's sums --------------------------------------------------------------------------
def point32(base, xin, alpha):
    """X(alpha) fp32 of fp32 base, xin: difference, product and sum in fp64 (one rounding each), then one rounding to fp32."""
    if alpha >= 1.0:
        return xin.copy()
    if alpha <= 0.0:
        return base.copy()
    b64 = base.astype(np.float64)
    return (b64 + alpha * (xin.astype(np.float64) - b64)).astype(np.float32)


def init(x_in, x_base, Kc):
    """The state bx_guided_ig_init leaves: dict(x fp32 [R,P], attr fp64 [R,P], L_total fp64 [R], status i32 [R]); x_in, x_base fp32
    [B,P] (x_base may be one number)."""
    x_in = np.ascontiguousarray(x_in, dtype=np.float32)
    B, P = x_in.shape
    x_base = np.ascontiguousarray(np.broadcast_to(np.asarray(x_base, dtype=np.float32), (B, P)))
    R = B * Kc
    L = np.array([row_sum(np.abs(x_in[r // Kc].astype(np.float64) - x_base[r // Kc].astype(np.float64))) for r in range(R)])
    return dict(x_in=x_in, x_base=x_base, Kc=Kc, x=np.repeat(x_base, Kc, axis=0), attr=np.zeros((R, P)), L_total=L, status=np.zeros(R, dtype=np.int32))


def step(st, g, i, n, k, max_dist, cap, row0=0, iters=None, trace=None, largest_first=False):
    """bx_guided_ig_step: every pass of step i for rows row0 .. row0 + len(g) - 1, in place; g fp32 [rows,P].  iters i32 [R,n] takes the
    pass counts; trace (a list) takes row row0's passes in the form of ``literal``."""
    g = np.asarray(g, dtype=np.float32)
    a_min, a_max, left = window(i, n, max_dist)
    for rr in range(len(g)):
        r = row0 + rr
        b = r // st["Kc"]
        xin, base, gr, x, attr = st["x_in"][b], st["x_base"][b], g[rr], st["x"][r], st["attr"][r]
        passes = 0
        if st["status"][r] == OK and st["L_total"][r] != 0.0:
            in64, b64, g64 = xin.astype(np.float64), base.astype(np.float64), gr.astype(np.float64)
            d = in64 - b64
            x_min, x_max, L_target = point32(base, xin, a_min), point32(base, xin, a_max), st["L_total"][r] * left
            if np.isnan(gr).any():
                st["status"][r] = NAN
            else:
                while True:
                    passes += 1
                    x_old = x.astype(np.float64)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        a = np.where(d == 0, a_max, (x_old - b64) / d)
                    clamped = a < a_min
                    xc = np.where(clamped, x_min, x)
                    clamped = clamped & (xc != x)
                    L_cur = row_sum(np.abs(in64 - xc.astype(np.float64)))
                    ended = _close(L_target, L_cur)
                    S, more, gamma, xn = None, False, 0.0, xc
                    if not ended:
                        arrived = xc == x_max
                        mag = np.abs(gr).astype(np.float64)
                        S = _select(-mag if largest_first else mag, arrived, k)
                        gap = x_max.astype(np.float64) - xc.astype(np.float64)
                        L_S = row_sum(np.where(S, np.abs(gap), 0.0))
                        gamma = (L_cur - L_target) / L_S if L_S > 0 else math.inf
                        more = gamma > 1 and L_S > 0
                        if gamma > 1:
                            xn = np.where(S, x_max, xc)
                        elif gamma > 0:
                            xn = np.where(S, (xc.astype(np.float64) + gamma * gap).astype(np.float32), xc)
                    attr += (xn.astype(np.float64) - x_old) * g64
                    x[:] = xn
                    if trace is not None and rr == 0:
                        trace.append(_decisions(clamped, S, gamma, more))
                    if not more:
                        break
                    if passes >= cap:
                        st["status"][r] = CAP
                        break
        if iters is not None:
            iters[r, i] = passes


def run(x_in, x_base, grad_func, steps, fraction, max_dist, cap=None, largest_first=False):
    """(b) for one row with a caller-supplied grad_func (fp64 in, rounded to fp32): dict like ``literal``'s, values = fl32(attr)."""
    x_in = np.asarray(x_in, dtype=np.float32).reshape(1, -1)
    P = x_in.shape[1]
    st = init(x_in, np.asarray(x_base, dtype=np.float32).reshape(1, -1), 1)
    k = rank_k(P, fraction)
    cap = pass_cap(P, k) if cap is None else cap
    iters, trace = np.zeros((1, steps), dtype=np.int32), []
    for i in range(steps):
        trace.append([])
        g = np.asarray(grad_func(st["x"][0].astype(np.float64)), dtype=np.float64).astype(np.float32).reshape(1, P)
        step(st, g, i, steps, k, max_dist, cap, iters=iters, trace=trace[i], largest_first=largest_first)
    return dict(attr=st["attr"][0], values=st["attr"][0].astype(np.float32), x=st["x"][0], iters=iters[0], status=int(st["status"][0]), trace=trace,
                L_total=float(st["L_total"][0]), k=k, cap=cap)


def replay(x_in, x_base, Kc, grads, fraction, max_dist, largest_first=False):
    """(b) for rows [R,P] fed the gradients grads fp32 [R,n,P] of a call (its dump): -> (path fp32 [R,n,P] the point at the top of every
    step, values fp32 [R,P], iters i32 [R,n], status i32 [R]).  The point moves as the definition says whatever the gradients are, so a
    replay with other parameters shows what a driver that ignored them would have returned from the same gradients."""
    grads = np.asarray(grads, dtype=np.float32)
    R, n, P = grads.shape
    st = init(x_in, x_base, Kc)
    k = rank_k(P, fraction)
    iters, path = np.zeros((R, n), dtype=np.int32), np.empty((R, n, P), dtype=np.float32)
    for i in range(n):
        path[:, i] = st["x"]
        step(st, grads[:, i], i, n, k, max_dist, pass_cap(P, k), iters=iters, largest_first=largest_first)
    return path, st["attr"].astype(np.float32), iters, st["status"].copy()


def same_trace(ta, tb):
    """Whether two traces hold the same decisions, step by step and pass by pass."""
    if len(ta) != len(tb) or any(len(a) != len(b) for a, b in zip(ta, tb)):
        return False
    return all(np.array_equal(ca, cb) and np.array_equal(Sa, Sb) and fa == fb and ma == mb
               for sa, sb in zip(ta, tb) for (ca, Sa, fa, ma), (cb, Sb, fb, mb) in zip(sa, sb))
