"""numpy / scipy restatement of brainxai.map_similarity and of the re-initialiser of brainxai.randomization_test (the definitions are
pinned in include/brainxai.h):

    keys       the cell values with NaN counted as -inf and -0.0 equal to +0.0 (|value| first with ``abs``): bx_rank_desc's convention
    ranks      scipy.stats.rankdata(-key, method="average") - 1: the average descending 0-based rank
    spearman   scipy.stats.spearmanr = Pearson's correlation of those ranks
    pearson    scipy.stats.pearsonr; ``corr`` is the plain two-pass fp64 form, NaN for a constant row
    topk       the cells of rank < k in both stable descending sorts (np.argsort(-key, kind="stable")), divided by k
    ssim       scikit-image's structural_similarity restated from scipy.ndimage.uniform_filter1d / correlate1d in fp64, cropped to the
               positions whose whole window lies inside the map, an axis of extent 1 not filtered
    draws      fl32(bound * u), u = (w >> 8) 2^-23 - 1, w = word e & 3 of Philox4x32-10(counter = (e >> 2, j, s, 2), key = seed's halves)
"""
import math

import numpy as np
import scipy.ndimage
import scipy.stats
import torch

from tests.smooth_grad_ref import philox


def keys(x, abs=False):
    """float32 [..]: what the ranks order by."""
    k = np.array(x, dtype=np.float32, copy=True)
    if abs:
        k = np.abs(k)
    k[np.isnan(k)] = -np.inf
    k[k == 0] = 0.0
    return k


def average_ranks(x, abs=False):
    """fp64 [R,N]: the tie-averaged descending 0-based ranks of every row."""
    k = keys(x, abs).astype(np.float64)
    return np.stack([scipy.stats.rankdata(-row, method="average") - 1.0 for row in k])


def stable_ranks(x, abs=False):
    """int64 [R,N]: the position of every cell in a stable descending sort of its row (bx_rank_desc)."""
    k = keys(x, abs).astype(np.float64)
    out = np.empty(k.shape, dtype=np.int64)
    for r, row in enumerate(k):
        out[r, np.argsort(-row, kind="stable")] = np.arange(row.size)
    return out


def _vals(x, abs):
    v = np.asarray(x, dtype=np.float32).astype(np.float64)
    return np.abs(v) if abs else v


def corr(a, b, abs=False):
    """fp64 [R]: the two-pass Pearson correlation of the rows in numpy fp64, clamped to [-1, 1]; NaN where a centred sum of squares is 0."""
    x, y = _vals(a, abs), _vals(b, abs)
    dx, dy = x - x.mean(1, keepdims=True), y - y.mean(1, keepdims=True)
    sxx, syy, sxy = (dx * dx).sum(1), (dy * dy).sum(1), (dx * dy).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.clip(sxy / np.sqrt(sxx * syy), -1.0, 1.0)
    r[(sxx == 0) | (syy == 0)] = np.nan
    return r


def pearson(a, b, abs=False):
    """scipy.stats.pearsonr row by row."""
    x, y = _vals(a, abs), _vals(b, abs)
    return np.array([scipy.stats.pearsonr(p, q).statistic if len(p) > 1 else np.nan for p, q in zip(x, y)])


def spearman(a, b, abs=False):
    return corr(average_ranks(a, abs), average_ranks(b, abs))


def topk_count(topk, N):
    return int(topk) if isinstance(topk, (int, np.integer)) else min(N, max(1, math.ceil(float(topk) * N)))


def topk_overlap(a, b, k, abs=False):
    """fp64 [R]: |{i : rank_a[i] < k and rank_b[i] < k}| / k."""
    ra, rb = stable_ranks(a, abs), stable_ranks(b, abs)
    return ((ra < k) & (rb < k)).sum(1) / float(k)


def gaussian_taps():
    """The taps of scipy.ndimage.gaussian_filter1d(sigma=1.5, truncate=3.5): radius 5, read off scipy itself."""
    e = np.zeros(11)
    e[5] = 1.0
    return scipy.ndimage.gaussian_filter1d(e, 1.5, truncate=3.5, mode="constant")


def rescale(x):
    """fp64: every map [.., H, W] to [0, 1] by its own extremes; a constant map becomes zeros."""
    lo, hi = x.min((-2, -1), keepdims=True), x.max((-2, -1), keepdims=True)
    span = hi - lo
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(span == 0, 0.0, (x - lo) / np.where(span == 0, 1.0, span))


def ssim_cells(a, b, data_range, abs):
    """(X, Y fp64 [R,H,W], R): the cells SSIM compares and the dynamic range."""
    x, y = _vals(a, abs), _vals(b, abs)
    if data_range is None:
        return rescale(x), rescale(y), 1.0
    return x, y, float(data_range)


def ssim_map(X, Y, R, window="uniform", win_size=None):
    """S fp64 [R, Ho, Wo] over the positions whose whole window lies inside the map, and the window width."""
    win = 11 if window == "gaussian" else (7 if win_size is None else win_size)
    axes = [ax for ax in (1, 2) if X.shape[ax] > 1]
    assert axes and all(X.shape[ax] >= win for ax in axes)
    NP = win ** len(axes)
    cov = 1.0 if window == "gaussian" else NP / (NP - 1.0)
    taps = gaussian_taps() if window == "gaussian" else None

    def F(v):
        for ax in axes:
            v = scipy.ndimage.correlate1d(v, taps, axis=ax, mode="constant") if taps is not None else scipy.ndimage.uniform_filter1d(v, win, axis=ax, mode="constant")
        return v
    ux, uy, uxx, uyy, uxy = F(X), F(Y), F(X * X), F(Y * Y), F(X * Y)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    pad = win // 2
    crop = tuple(slice(pad, S.shape[ax] - pad) if ax in axes else slice(None) for ax in range(3))
    return S[crop], win


def ssim(a, b, window="uniform", win_size=None, data_range=None, abs=False):
    """fp64 [R]: the mean SSIM of the maps a, b [R,H,W]."""
    X, Y, R = ssim_cells(a, b, data_range, abs)
    S, _ = ssim_map(X, Y, R, window, win_size)
    return S.reshape(len(S), -1).mean(1)


# ---- the re-initialiser ---------------------------------------------------------------------------------------------------------------
def param_uniform(n, bound, seed, j, s):
    """fp32 [n] = fl32(fl32(bound) * u), exact from the Philox words."""
    seed = int(seed)
    Q = (n + 3) // 4
    w = philox((np.arange(Q, dtype=np.uint64), np.uint64(j), np.uint64(s), np.uint64(2)), (seed & 0xFFFFFFFF, seed >> 32))     # [4, Q]
    w = np.moveaxis(w, 0, -1).reshape(Q * 4)[:n]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return (np.float32(bound) * u).astype(np.float32)


def fan_in(weight):
    return int(weight.shape[1]) * int(np.prod(weight.shape[2:], dtype=np.int64))


def _resolve(model, dotted):
    mod = model
    for part in dotted.split("."):
        mod = getattr(mod, part)
    return mod


def reinit_layer_(sd, model, layer, seed, s):
    """Re-initialise ``layer`` (a dotted name or a tuple of names) in the host state_dict ``sd``, as stage s of the test's list.  The
    model is read for its structure only: the modules' types, the order of their parameters and their shapes."""
    names = (layer,) if isinstance(layer, str) else tuple(layer)
    position = {}
    for n in names:
        for pname, _ in _resolve(model, n).named_parameters():
            position.setdefault(f"{n}.{pname}", len(position))
    for n in names:
        for sub_name, sub in _resolve(model, n).named_modules():
            full = f"{n}.{sub_name}" if sub_name else n
            if isinstance(sub, (torch.nn.Conv2d, torch.nn.Linear)):
                bound = 1.0 / math.sqrt(fan_in(sub.weight))
                for pname in ("weight", "bias"):
                    if getattr(sub, pname) is not None:
                        old = sd[f"{full}.{pname}"]
                        sd[f"{full}.{pname}"] = torch.from_numpy(param_uniform(old.numel(), bound, seed, position[f"{full}.{pname}"], s)).reshape(old.shape)
            elif isinstance(sub, torch.nn.modules.batchnorm._BatchNorm):
                for pname, value in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0), ("num_batches_tracked", 0)):
                    sd[f"{full}.{pname}"] = torch.full_like(sd[f"{full}.{pname}"], value)


def reinit_state_dict(model, layers, seed, order, stage):
    """The state_dict of ``model`` (any device; copied to the host) as it stands at ``stage`` of the randomization test."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for s, layer in enumerate(layers[:stage + 1]):
        if order == "cascade" or s == stage:
            reinit_layer_(sd, model, layer, seed, s)
    return sd
