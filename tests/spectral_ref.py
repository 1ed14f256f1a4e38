"""The definition of brainxai.spectral_gradients / spectral_occlusion (include/brainxai.h) restated in numpy fp64 on numpy's own FFT, the
kernels' error bounds derived from their operations, and the fp64 oracle side of the end-to-end tests.  A plain module: no tests.

For a row x[0..T), F = T // 2 + 1:  X = rfft(x);  c_0 = 1, c_{T/2} = 1 for even T, c_f = 2 otherwise;  u = X / |X| (1 where X == 0);
with g the gradient by the row and G = rfft(g):
    amplitude gradient    (c_f / T) Re(u_f conj(G_f))          gradient x amplitude    (c_f / T) Re(X_f conj(G_f))
band component y_q = irfft(X restricted to [lo_q, hi_q)); a band-stopped row is fl32(x - y_q)."""
import numpy as np
import torch

U = 2.0 ** -53
CLINICAL = [(0.5, 4.0), (4.0, 8.0), (8.0, 13.0), (13.0, 30.0)]


def weights(T):
    c = np.full(T // 2 + 1, 2.0)
    c[0] = 1.0
    if T % 2 == 0:
        c[T // 2] = 1.0
    return c


def rdft(x):
    """complex128 [..., F] of the last axis, numpy's pocketfft in fp64."""
    return np.fft.rfft(np.asarray(x, dtype=np.float64), axis=-1)


def unit(X):
    """X / |X|, and 1 + 0i where X is exactly zero (numpy's angle(0) = 0)."""
    A = np.abs(X)
    return np.where(A == 0, 1.0 + 0.0j, X / np.where(A == 0, 1.0, A))


def maps(x, g, kind, variant=None):
    """fp64 [..., F]: the map of rows x and their gradients g (same shape, or g with extra leading axes that broadcast).  variant (the
    discrimination checks, None for the definition): 'conj' drops the conjugate, 'cf' sets c_f = 1, 'unit' sets u = 1."""
    T = np.shape(x)[-1]
    X, G = rdft(x), rdft(g)
    c = np.ones(T // 2 + 1) if variant == "cf" else weights(T)
    lead = X if kind == "gradient_x_amplitude" else (np.ones_like(X) if variant == "unit" else unit(X))
    return c / T * np.real(lead * (G if variant == "conj" else np.conj(G)))


def band_bins(bands, T, fs=None):
    """[(f_lo, f_hi)]: bin f belongs to (lo, hi) iff lo * T <= f * fs < hi * T in fp64."""
    edges = CLINICAL if isinstance(bands, str) else list(bands)
    out = []
    for lo, hi in edges:
        inside = [f for f in range(T // 2 + 1) if float(lo) * T <= float(f) * (1.0 if fs is None else float(fs)) < float(hi) * T]
        start = sum(1 for f in range(T // 2 + 1) if float(f) * (1.0 if fs is None else float(fs)) < float(lo) * T)
        out.append((start, start + len(inside)))
        assert inside == list(range(start, start + len(inside)))
    return out


def band_sum(values, bins):
    """fp64 [..., nb]: ascending sequential sums of the fp32 values from +0, the device's order."""
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    out = np.zeros(v.shape[:-1] + (len(bins),))
    for q, (lo, hi) in enumerate(bins):
        for f in range(lo, hi):
            out[..., q] = out[..., q] + v[..., f]
    return out


def band_component(x, lo, hi):
    """fp64: the part of the rows x (last axis T) carried by bins [lo, hi)."""
    T = np.shape(x)[-1]
    X = rdft(x)
    keep = np.zeros(T // 2 + 1)
    keep[lo:hi] = 1.0
    return np.fft.irfft(X * keep, n=T, axis=-1)


def bandstop_rows(x, bins, cells):
    """fp64 [B, N, 1, Chans, T]: x [B,1,Chans,T] with band q removed from every electrode (cells 'band', row q) or from electrode e alone
    (cells 'electrode_band', row q * Chans + e), before the rounding to fp32."""
    x = np.asarray(x, dtype=np.float64)
    B, _, Chans, T = x.shape
    rows = []
    for lo, hi in bins:
        y = band_component(x, lo, hi)
        if cells == "band":
            rows.append(x - y)
        else:
            for e in range(Chans):
                r = x.copy()
                r[:, :, e] -= y[:, :, e]
                rows.append(r)
    return np.stack(rows, axis=1)


def accumulate(g, w, B, n, acc=None, slot=0, Kc=1, row0=0):
    """acc fp64 [B,Kc,per] += w[k] * g over rows row0 .. row0 + len(g) - 1 (row j = b * n + k), ascending: product and sum one rounding each."""
    g = np.asarray(g, dtype=np.float32).reshape(len(g), -1).astype(np.float64)
    acc = np.zeros((B, Kc, g.shape[1])) if acc is None else acc
    for r in range(len(g)):
        j = row0 + r
        acc[j // n, slot] = acc[j // n, slot] + w[j % n] * g[r]
    return acc


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def dft_bound(x):
    """fp64 [..., 1]: (T + 4) 2^-53 sum_t |x_t| per row -- T fused multiply-adds of at most sum |x| each, a table entry within two units,
    and numpy's own error."""
    x = np.asarray(x, dtype=np.float64)
    return (x.shape[-1] + 4) * U * np.abs(x).sum(-1, keepdims=True)


def values_bound(x, g, kind, want):
    """Per bin: (c_f / T) (eps_X |G_f| / |X_f| + eps_G) + 2^-24 |value|; the first term only for the amplitude gradient (a phase error of
    eps_X / |X| turns u against G)."""
    T = np.shape(x)[-1]
    X, G = rdft(x), rdft(g)
    b = dft_bound(g) * np.ones(G.shape)
    if kind == "amplitude_gradient":
        A = np.abs(X)
        b = b + dft_bound(x) * np.abs(G) / np.where(A == 0, 1.0, A)
    return weights(T) / T * b + 2.0 ** -24 * np.abs(want)


def tiny_bins(x):
    """bool [..., F]: bins with |X_f| < 2^-30 sum_t |x_t|, where the phase is rounding noise (left out of the amplitude-gradient comparison)."""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(rdft(x)) < 2.0 ** -30 * np.abs(x).sum(-1, keepdims=True)


def bandstop_bound(x, row, lo, hi):
    """Per element: 2^-24 |row| + ((hi - lo) + 2) 2^-53 sum c_f |X_f| / T + (hi - lo) (2 / T) eps_X."""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[-1]
    X = np.abs(rdft(x)) * weights(T)
    return 2.0 ** -24 * np.abs(row) + ((hi - lo) + 2) * U * X[..., lo:hi].sum(-1, keepdims=True) / T + (hi - lo) * (2.0 / T) * dft_bound(x)


# ---- the oracle side --------------------------------------------------------------------------------------------------------------------
def nodes(n):
    """(alpha, w) of the path: one point at 1 for n = 1, the Gauss-Legendre nodes on [0, 1] otherwise."""
    if n == 1:
        return np.ones(1), np.ones(1)
    t, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (1.0 + t), 0.5 * w


def path_rows(x, n):
    """fp32 [B, n, ...]: fl32(fl32(alpha_k) * x), the rows the driver differentiates at."""
    a = torch.from_numpy(nodes(n)[0].astype(np.float32))
    x = torch.as_tensor(x, dtype=torch.float32)
    return a.view(1, n, *([1] * (x.dim() - 1))) * x[:, None]


def path_gradient(forward, x, n):
    """fp64 [B, K, 1, Chans, T]: sum_k w_k dF_c/dx(alpha_k x) of ``forward`` (an fp64 model or a callable on all B * n rows, sample-major)."""
    rows = path_rows(x, n).double()
    B = rows.shape[0]
    xi = rows.reshape(B * n, *rows.shape[2:]).clone().requires_grad_(True)
    y = forward(xi)
    w = torch.from_numpy(nodes(n)[1]).view(1, n, *([1] * (rows.dim() - 2)))
    out = []
    for c in range(y.shape[1]):
        (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
        out.append((w * g.reshape(rows.shape)).sum(1))
    return torch.stack(out, 1)


def two_input(model64, other, n=1):
    """forward(rows) of the two-input fp64 model on EEG rows: the spectrogram is the sample's own, repeated over n consecutive rows."""
    o = torch.as_tensor(other).double().repeat_interleave(n, dim=0)
    return lambda xi: model64(xi, o)


def outputs(forward, x):
    with torch.no_grad():
        return forward(torch.as_tensor(x).double())


def oracle_map(x, grad, kind, variant=None):
    """fp64 [B, K, Chans, F] from x [B,1,Chans,T] and the gradient [B,K,1,Chans,T]."""
    x = np.asarray(x, dtype=np.float64)
    return maps(x[:, None, 0], np.asarray(grad, dtype=np.float64)[:, :, 0], kind, variant)


# ---- the end-to-end cases, reference side -----------------------------------------------------------------------------------------------
import copy            # noqa: E402
import functools       # noqa: E402

from oracle import ref_torch as O      # noqa: E402

E2E_KINDS = ("eegnet", "deep", "multimodal", "small")
E2E_STEPS = (1, 5)
MAP_KINDS = ("amplitude_gradient", "gradient_x_amplitude")
VARIANTS = {"amplitude_gradient": ("conj", "cf", "unit"), "gradient_x_amplitude": ("conj", "cf")}


def oracle_case(kind):
    """-> (ref, x, other): the oracle's model in fp32 with the parameters of the GPU tests' cases (tests/grad_gpu.eeg_models; 'small' is a
    generic EEGNet at 5 x 512), the explained EEG input and the spectrogram (None for the stand-alone nets)."""
    if kind == "eegnet":
        return O.fill_params(O.EEGNet(6, Chans=19, Samples=2000, dropoutRate=0.0), seed=31).eval(), O.seeded((2, 1, 19, 2000), 91, "randn"), None
    if kind == "deep":
        return O.fill_params(O.EEGNetAttentionDeep(6, Chans=19, Samples=2000, dropoutRate=0.0), seed=61).eval(), O.seeded((2, 1, 19, 2000), 12, "randn"), None
    if kind == "small":
        return O.fill_params(O.EEGNet(6, Chans=5, Samples=512, dropoutRate=0.0), seed=33).eval(), O.seeded((2, 1, 5, 512), 92, "randn"), None
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, dropout=0.0), seed=42).eval()
    with torch.no_grad():                                                 # tests/perturb_gpu.scaled_multimodal
        ref.spectrogram_model.fc.weight *= 0.05
        ref.eeg_model.dense.weight *= 0.05
        ref.fc2.weight *= 0.5
    return ref, O.seeded((2, 1, 19, 2000), 12, "randn"), O.seeded((2, 4, 32, 64), 11, "rand")


@functools.lru_cache(maxsize=None)
def oracle_gradient(kind, n):
    """(x, fp64 path-weighted gradient [B,K,1,Chans,T], fp64 outputs at x [B,K], at the zero input [B,K]); computed once, never written to."""
    ref, x, other = oracle_case(kind)
    f64 = copy.deepcopy(ref).double().eval()
    many = f64 if other is None else two_input(f64, other, n)
    one = f64 if other is None else two_input(f64, other)
    return x, path_gradient(many, x, n), outputs(one, x), outputs(one, torch.zeros_like(x))


def pair_max(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return a.reshape(a.shape[0], a.shape[1], -1).max(2)


def movements(kind, n, map_kind):
    """{variant: the least, over (sample, class), of max|variant - definition| / max|definition|} on the fp64 reference alone."""
    x, grad, _, _ = oracle_gradient(kind, n)
    want = oracle_map(x.numpy(), grad.numpy(), map_kind)
    return {v: float((pair_max(oracle_map(x.numpy(), grad.numpy(), map_kind, v) - want) / pair_max(want)).min()) for v in VARIANTS[map_kind]}
