"""numpy restatement of brainxai.mask_explain's device side (optimised perturbation masks, Fong & Vedaldi, ICCV 2017; the definition is
pinned in include/brainxai.h): rows, masks, gradient, Adam step, history and status, with the fp32 and fp64 roundings and the orders of
the sums exactly as the header writes them.

Mask domain [Hm,Wm], grid gh x gw.  Row r = b * Kc + slot owns m_r fp32 [gh,gw] (1.0 at the start) and mu_r, nu_r fp64 (0 at the start).
Up-sampling M = U(m), per axis in fp32 without fused multiply-adds, pixel u of n, g cells:
    s = max(0, (u + 0.5) * (g / n) - 0.5),  i0 = min(int(s), g - 1),  i1 = min(i0 + 1, g - 1),  l = s - i0
    M = (1 - ly) * ((1 - lx) * m[y0][x0] + lx * m[y0][x1]) + ly * ((1 - lx) * m[y1][x0] + lx * m[y1][x1])
Rows X = base + M * (x - base), three fp32 roundings.  The input is seen as Cs planes of Hm x Wm that share a mask value: the C channels
of a spectrogram; one plane for an EEG input with a [Chans,T] domain; the Chans electrodes (planes of 1 x T) under a [1,T] domain.
Gradient in fp64 from g = dF_c/dX fp32:
    t(p) = SUM_c (double)g[c,p] * (double)fl32(x[c,p] - base[c,p]), from 0.0 in plane order
    hs[y,j] = SUM_x wx(x,j) * t(y,x) from 0.0 over cell j's footprint (the pixels whose i0 is j - 1 or j) in ascending x
    G_data[i,j] = sign * w_r * SUM_y wy(y,i) * hs[y,j] likewise in ascending y;  w(u,j) = (j == i0 ? (double)fl32(1 - l) : 0) + (j == i1 ? (double)l : 0)
    w_r = 1 (logprob) or (double)expf(y_r[c]) (prob), expf the correctly rounded fp32 exponential;  sign + deletion, - preservation
    G = (G_data -+ l1 / (gh gw)) + tv * dTV
Adam (fp64):  mu = b1 mu + (1 - b1) G;  nu = b2 nu + ((1 - b2) G) G;  m = clamp(fl32(m - (lr (mu / c1)) / (sqrt(nu / c2) + eps)), 0, 1)
History before the update: (s_c, SUM m / (gh gw), TV_beta(m)); the two sums lane-strided (64 partials over e = l, l + 64, ...) plus the xor
butterfly.  Status: y_r[c] NaN or a NaN in G_data stops the row (NAN) before anything is written; a stopped row stays as it is."""
import numpy as np

OK, NAN = 0, 1
DELETION, PRESERVATION = 0, 1
PROB, LOGPROB = 0, 1
F32 = np.float32


def axis(n, g):
    """-> (i0 int [n], i1 int [n], l fp32 [n]) of an axis of n pixels and g cells."""
    u = np.arange(n, dtype=F32)
    scale = F32(g) / F32(n)
    s = (u + F32(0.5)) * scale - F32(0.5)
    s = np.where(s < 0, F32(0), s).astype(F32)
    i0 = np.minimum(s.astype(np.int64), g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    return i0, i1, (s - i0.astype(F32)).astype(F32)


def footprint(i0, j):
    """[lo, hi): the pixels whose i0 is j - 1 or j."""
    idx = np.nonzero((i0 == j - 1) | (i0 == j))[0]
    return (0, 0) if len(idx) == 0 else (int(idx[0]), int(idx[-1]) + 1)


def weights(i0, i1, l, g):
    """fp64 [n,g]: w(u,j), the forward's fp32 weights widened."""
    n = len(i0)
    w = np.zeros((n, g))
    l0 = (F32(1) - l).astype(F32).astype(np.float64)
    w[np.arange(n), i0] = l0
    np.add.at(w, (np.arange(n), i1), l.astype(np.float64))          # i1 == i0 at the clamped end: the sum of the two
    return w


def upsample(m, Hm, Wm):
    """U(m): fp32 [...,gh,gw] -> fp32 [...,Hm,Wm]."""
    m = np.asarray(m, dtype=F32)
    gh, gw = m.shape[-2:]
    y0, y1, ly = axis(Hm, gh)
    x0, x1, lx = axis(Wm, gw)
    one = F32(1)

    def blend(rows):                                                    # [...,gw] at rows y -> [...,Hm,Wm]
        r = m[..., rows, :]
        return ((one - lx) * r[..., x0]).astype(F32) + (lx * r[..., x1]).astype(F32)
    top, bot = blend(y0).astype(F32), blend(y1).astype(F32)
    lyc = ly[:, None]
    return (((one - lyc) * top).astype(F32) + (lyc * bot).astype(F32)).astype(F32)


def planes(x, map_rows):
    """The input as planes that share a mask value: x [B,C,H,W] -> ([B,Cs,Hm,Wm] view, by_row)."""
    B, C, H, W = x.shape
    if map_rows == 0:
        return x, False
    assert C == 1 and map_rows in (H, 1)
    if map_rows == H:
        return x, True
    return x.reshape(B, H, 1, W), False


def base_planes(base, kind, xp, by_row):
    """The baseline broadcast to the planes' shape, fp32."""
    B, Cs, Hm, Wm = xp.shape
    base = np.asarray(base, dtype=F32)
    if kind == 0:
        return np.broadcast_to(base.reshape(()), xp.shape)
    if kind == 1:
        return np.broadcast_to(base.reshape((1, 1, Hm, 1) if by_row else (1, Cs, 1, 1)), xp.shape)
    return base.reshape(xp.shape)


def rows(x, base, kind, m, Kc, map_rows, row0=0, count=None):
    """fp32 [count,C,H,W]: base + U(m_r) * (x_b - base) of rows row0 .. row0+count-1; x fp32 [B,C,H,W], m fp32 [R,gh,gw]."""
    x = np.asarray(x, dtype=F32)
    xp, by_row = planes(x, map_rows)
    bp = base_planes(base, kind, xp, by_row)
    count = len(m) - row0 if count is None else count
    Hm, Wm = xp.shape[2:]
    out = np.empty((count, *xp.shape[1:]), dtype=F32)
    for rr in range(count):
        r = row0 + rr
        b = r // Kc
        M = upsample(m[r], Hm, Wm)[None]
        d = (xp[b] - bp[b]).astype(F32)
        out[rr] = (bp[b] + (M * d).astype(F32)).astype(F32)
    return out.reshape(count, *x.shape[1:])


def lane_sum(v):
    """fp64 [..,G] -> [..]: 64 partial sums over e = l, l + 64, ... in ascending e, then the xor butterfly (offsets 32, 16, .., 1)."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros(v.shape[:-1] + (64,))
    for e0 in range(0, v.shape[-1], 64):
        k = min(64, v.shape[-1] - e0)
        part[..., :k] += v[..., e0:e0 + k]
    lanes = np.arange(64)
    o = 32
    while o:
        part = part + part[..., lanes ^ o]
        o >>= 1
    return part[..., 0]


def _pow(a, beta):
    return a if beta == 1 else (a * a if beta == 2 else (a * a) * a)


def _tv_grad(d, beta):
    if beta == 1:
        return np.sign(d)
    if beta == 2:
        return 2.0 * d
    return (3.0 * d) * np.abs(d)


def tv(m, beta):
    """TV_beta of fp32 [...,gh,gw] in the device's order -> fp64 [...]."""
    v = np.asarray(m, dtype=F32).astype(np.float64)
    term = np.zeros(v.shape)
    term[..., :, :-1] += _pow(np.abs(v[..., :, 1:] - v[..., :, :-1]), beta)
    term[..., :-1, :] += _pow(np.abs(v[..., 1:, :] - v[..., :-1, :]), beta)
    return lane_sum(term.reshape(*v.shape[:-2], -1))


def tv_gradient(m, beta):
    v = np.asarray(m, dtype=F32).astype(np.float64)
    acc = np.zeros(v.shape)
    dh = _tv_grad(v[..., :, 1:] - v[..., :, :-1], beta)                  # of cell (i, j+1) minus cell (i, j)
    dv = _tv_grad(v[..., 1:, :] - v[..., :-1, :], beta)
    acc[..., :, 1:] += dh
    acc[..., :, :-1] -= dh
    acc[..., 1:, :] += dv
    acc[..., :-1, :] -= dv
    return acc


def expf(y):
    """The correctly rounded fp32 exponential."""
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(y, dtype=F32).astype(np.float64)).astype(F32)


def data_gradient(x, base, kind, g, map_rows, gh, gw, Kc, row0=0):
    """SUM_y wy * SUM_x wx * t, fp64 [rows,gh,gw], without sign and w_r; g fp32 [rows,C,H,W] of rows row0 ..."""
    x = np.asarray(x, dtype=F32)
    xp, by_row = planes(x, map_rows)
    bp = base_planes(base, kind, xp, by_row)
    B, Cs, Hm, Wm = xp.shape
    g = np.asarray(g, dtype=F32).reshape(-1, Cs, Hm, Wm)
    n = len(g)
    samples = (row0 + np.arange(n)) // Kc
    d = (xp - bp).astype(F32).astype(np.float64)
    t = np.zeros((n, Hm, Wm))
    for c in range(Cs):
        t = t + g[:, c].astype(np.float64) * d[samples, c]
    x0, x1, lx = axis(Wm, gw)
    y0, y1, ly = axis(Hm, gh)
    wx, wy = weights(x0, x1, lx, gw), weights(y0, y1, ly, gh)
    with np.errstate(invalid="ignore"):
        hs = np.zeros((n, Hm, gw))
        for j in range(gw):
            lo, hi = footprint(x0, j)
            for xx in range(lo, hi):
                hs[:, :, j] = hs[:, :, j] + wx[xx, j] * t[:, :, xx]
        out = np.zeros((n, gh, gw))
        for i in range(gh):
            lo, hi = footprint(y0, i)
            for yy in range(lo, hi):
                out[:, i, :] = out[:, i, :] + wy[yy, i] * hs[:, yy, :]
    return out


def init(R, gh, gw):
    return dict(m=np.ones((R, gh, gw), dtype=F32), mu=np.zeros((R, gh, gw)), nu=np.zeros((R, gh, gw)), status=np.zeros(R, dtype=np.int32))


def step(st, x, base, kind, g, y, classes, map_rows, Kc, it, history, *, mode, score, beta, lr, l1, tv_w, b1, b2, eps, row0=0, G_out=None, acc=None):
    """bx_maskopt_step on the state st (in place) for rows row0 .. row0+len(g)-1: g fp32 [rows,C,H,W], y fp32 [rows,K], classes int [R],
    history fp64 [R,n,3]; G_out fp64 [R,gh,gw] takes G of the rows that took the step; acc: ``data_gradient`` of these rows, where the caller has it."""
    gh, gw = st["m"].shape[1:]
    n = len(g)
    y = np.asarray(y, dtype=F32)
    acc = data_gradient(x, base, kind, g, map_rows, gh, gw, Kc, row0) if acc is None else acc
    c1, c2 = 1.0 - b1 ** (it + 1), 1.0 - b2 ** (it + 1)
    l1n = l1 / float(gh * gw)
    for rr in range(n):
        r = row0 + rr
        if st["status"][r] != OK:
            continue
        yv = y[rr, classes[r]]
        sc = float(expf(yv)) if score == PROB else float(yv)
        with np.errstate(invalid="ignore", over="ignore"):
            Gd = (float(expf(yv)) if score == PROB else 1.0) * acc[rr]
        if mode == PRESERVATION:
            Gd = -Gd
        if np.isnan(yv) or np.isnan(Gd).any():
            st["status"][r] = NAN
            continue
        m = st["m"][r]
        history[r, it] = (sc, lane_sum(m.astype(np.float64).reshape(-1)) / float(gh * gw), tv(m, beta))
        reg = tv_w * tv_gradient(m, beta)
        G = ((Gd - l1n) if mode == DELETION else (Gd + l1n)) + reg
        if G_out is not None:
            G_out[r] = G
        mu = b1 * st["mu"][r] + (1.0 - b1) * G
        nu = b2 * st["nu"][r] + ((1.0 - b2) * G) * G
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            to = (m.astype(np.float64) - (lr * (mu / c1)) / (np.sqrt(nu / c2) + eps)).astype(F32)
        st["mu"][r], st["nu"][r] = mu, nu
        st["m"][r] = np.where(to < 0, F32(0), np.where(to > 1, F32(1), to))


def replay(x, base, kind, grads, outs, classes, map_rows, Kc, gh, gw, *, mode, score, beta, lr, l1, tv_w, b1, b2, eps):
    """The loop fed a call's dumped gradients fp32 [R,n,C,H,W] and outputs fp32 [R,n,K] -> (path fp32 [R,n,gh,gw]: the grid at the top of
    every iteration, the final state, history fp64 [R,n,3]).  The grid moves as the definition says whatever the gradients are, so a
    replay with other settings shows what a driver that ignored them would have returned from the same gradients."""
    R, n = grads.shape[:2]
    st = init(R, gh, gw)
    history = np.zeros((R, n, 3))
    path = np.empty((R, n, gh, gw), dtype=F32)
    for it in range(n):
        path[:, it] = st["m"]
        step(st, x, base, kind, grads[:, it], outs[:, it], classes, map_rows, Kc, it, history, mode=mode, score=score, beta=beta, lr=lr, l1=l1,
             tv_w=tv_w, b1=b1, b2=b2, eps=eps)
    return path, st, history
