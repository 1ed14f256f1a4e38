"""numpy / torch-fp64 restatement of brainxai.smooth_grad (the definition is pinned in include/brainxai.h):

    (w0,w1,w2,w3) = Philox4x32-10(counter = (e >> 2, k, b, 0), key = (seed & 0xffffffff, seed >> 32))
    u = ((wa >> 8) + 1) 2^-24,  t = (wb >> 8) 2^-23,  r = sqrt(-2 log u),  z_even = r cos(pi t),  z_odd = r sin(pi t)
    row[b,k] = fl32(x[b] + fl32(sigma[b] * z[b,k])),   g = dF_c/dx(row),   S1 = sum_k g,   S2 = sum_k g^2   (fp64, ascending k)
    mean = S1 / n,   mean square = S2 / n,   variance = max(0, (S2 - S1 * S1 / n) / n)

with F_c the model's output log-probability.  Rows are numbered j = b * n + k, sample-major.  Box-Muller is fp64 here (the device's is
fp32 with its own logf / cospif / sinpif: compared under a bound, not bit for bit); everything from z32 on is exact."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """Philox4x32-10 of the Random123 library.  counter: four uint32 arrays (broadcast together), key: two ints -> uint32 [4, ...]."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def noise(B, n, per, seed, with_r=False):
    """z fp64 [B, n, per]: the exact Box-Muller values of the definition's (u, t); with_r: also r = sqrt(-2 log u) per element."""
    seed = int(seed)
    Q = (per + 3) // 4
    q = np.arange(Q, dtype=np.uint64)[None, None, :]
    k = np.arange(n, dtype=np.uint64)[None, :, None]
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    w = philox((q, k, b, np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))            # [4, B, n, Q]
    z, rr = np.empty((B, n, Q, 4)), np.empty((B, n, Q, 4))
    for pair in range(2):
        wa, wb = w[2 * pair].astype(np.uint64), w[2 * pair + 1].astype(np.uint64)
        u = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        t = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -23
        r = np.sqrt(-2.0 * np.log(u))
        z[..., 2 * pair], z[..., 2 * pair + 1] = r * np.cos(np.pi * t), r * np.sin(np.pi * t)
        rr[..., 2 * pair] = rr[..., 2 * pair + 1] = r
    z, rr = z.reshape(B, n, Q * 4)[:, :, :per], rr.reshape(B, n, Q * 4)[:, :, :per]
    return (z, rr) if with_r else z


def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def sigma(x, level):
    """fp32 [B] = fl32(level * |fl32(max - min)|) per sample, float32 arithmetic throughout."""
    x = _np32(x).reshape(len(x), -1)
    rng = np.abs((x.max(1) - x.min(1)).astype(np.float32))
    return (np.float32(level) * rng).astype(np.float32)


def rows(x, sig, z32):
    """fp32 [B*n, ...] = fl32(x + fl32(sigma * z)) of z32 fp32 [B, n, ...]: two separate fp32 roundings (numpy float32 never fuses)."""
    x, z32 = _np32(x), _np32(z32)
    B, n = z32.shape[:2]
    s = np.asarray(sig, dtype=np.float32).reshape(B, *([1] * (z32.ndim - 1)))
    nz = (s * z32).astype(np.float32)
    return (x[:, None] + nz).astype(np.float32).reshape(B * n, *x.shape[1:])


def accumulate(g, B, n, S1=None, S2=None, slot=0, Kc=1, row0=0):
    """S1, S2 fp64 [B,Kc,per] += the sums over the rows row0 .. row0 + len(g) - 1, per sample in ascending k, of g and g * g in fp64;
    g fp32 [rows, ...].  Returns (S1, S2, abs1) with abs1 the same sum of |g| (for error bounds; the terms of S2 are positive)."""
    g = np.asarray(g, dtype=np.float32).reshape(len(g), -1).astype(np.float64)
    per = g.shape[1]
    S1 = np.zeros((B, Kc, per)) if S1 is None else S1
    S2 = np.zeros((B, Kc, per)) if S2 is None else S2
    abs1 = np.zeros((B, per))
    for r in range(len(g)):
        j = row0 + r
        S1[j // n, slot] += g[r]
        S2[j // n, slot] += g[r] * g[r]
        abs1[j // n] += np.abs(g[r])
    return S1, S2, abs1


KINDS = ("smoothgrad", "smoothgrad_sq", "vargrad")


def finish64(S1, S2, n, kind):
    """The values of ``kind`` in fp64, operation by operation as the definition orders them."""
    if kind == "smoothgrad":
        return S1 / n
    if kind == "smoothgrad_sq":
        return S2 / n
    return np.maximum(0.0, (S2 - S1 * S1 / n) / n)


def finish(S1, S2, n, kind, shape):
    """values fp32 [B,Kc,*shape] and map fp32 [B,Kc,*shape[1:]] = max over the leading (channel) axis of shape of |values|."""
    B, Kc, _ = S1.shape
    values = finish64(S1, S2, n, kind).reshape(B, Kc, *shape).astype(np.float32)
    return values, np.abs(values).max(2)


def values(model64, x, z32, sig, other=None, input="eeg", with_gmax=False):
    """(mean, mean square, variance), each fp64 [B,K,*x.shape[1:]], of an fp64 torch model on the fp32 rows of the restatement.  A
    two-input model (other given) takes (eeg, spec) with the other input the sample's own, repeated over the draws.  with_gmax: also
    M fp64 [B,K], the largest |g| over the draws and elements."""
    z32 = _np32(z32)
    B, n = z32.shape[:2]
    r = torch.from_numpy(rows(x, sig, z32)).double().reshape(B, n, *x.shape[1:])
    mean = sq = var = gmax = None
    was_training = model64.training
    model64.eval()
    for b in range(B):
        xi = r[b].clone().requires_grad_(True)
        if other is None:
            y = model64(xi)
        else:
            o = other[b:b + 1].double().expand(n, *other.shape[1:]).contiguous()
            y = model64(xi, o) if input == "eeg" else model64(o, xi)
        if mean is None:
            mean = torch.zeros(B, y.shape[1], *x.shape[1:], dtype=torch.float64)
            sq, var, gmax = torch.zeros_like(mean), torch.zeros_like(mean), torch.zeros(B, y.shape[1], dtype=torch.float64)
        for c in range(y.shape[1]):
            (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
            s1, s2 = g.sum(0), (g * g).sum(0)
            mean[b, c], sq[b, c] = s1 / n, s2 / n
            var[b, c] = torch.clamp((s2 - s1 * s1 / n) / n, min=0.0)
            gmax[b, c] = g.abs().max()
    model64.train(was_training)
    return (mean, sq, var, gmax) if with_gmax else (mean, sq, var)
