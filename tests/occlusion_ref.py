"""The definition of occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's Occlusion) restated with numpy and torch on the CPU --
what brainxai.occlusion and the bx_occlusion_* entry points are tested against.  Nothing here imports the package under test.

Domain [Hm,Wm]: [H,W] of a spectrogram [B,C,H,W] (a cell is a pixel with all its channels) or [Chans,T] of an EEG input [B,1,Chans,T].
Window (wh, ww), stride (sh, sw) with 1 <= sh <= wh <= Hm, 1 <= sw <= ww <= Wm; ny = 1 + ceil((Hm - wh) / sh), nx likewise; window
j = iy * nx + ix covers rows [iy sh, min(iy sh + wh, Hm)) and columns [ix sw, min(ix sw + ww, Wm))."""
import numpy as np
import torch

from tests.perturb_ref import baseline_tensor, sweep  # noqa: F401  (baseline_tensor is part of this module's interface)


def pair(v):
    return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def geometry(Hm, Wm, window, stride=None):
    """-> (wh, ww, sh, sw, ny, nx); stride None = the window (tiles)."""
    wh, ww = pair(window)
    sh, sw = (wh, ww) if stride is None else pair(stride)
    assert 1 <= sh <= wh <= Hm and 1 <= sw <= ww <= Wm, (Hm, Wm, window, stride)
    return wh, ww, sh, sw, 1 + -(-(Hm - wh) // sh), 1 + -(-(Wm - ww) // sw)


def bounds(geom, Hm, Wm, j):
    """Window j -> (y0, y1, x0, x1), half-open, clipped at the border."""
    wh, ww, sh, sw, ny, nx = geom
    iy, ix = divmod(j, nx)
    return iy * sh, min(iy * sh + wh, Hm), ix * sw, min(ix * sw + ww, Wm)


def masks(Hm, Wm, window, stride=None):
    """bool [N,Hm,Wm]: True where window j covers the cell."""
    geom = geometry(Hm, Wm, window, stride)
    N = geom[4] * geom[5]
    m = np.zeros((N, Hm, Wm), dtype=bool)
    for j in range(N):
        y0, y1, x0, x1 = bounds(geom, Hm, Wm, j)
        m[j, y0:y1, x0:x1] = True
    return m


def perturbed(x, m, baseline):
    """x [B,C,H,W] or [B,1,Chans,T] with the cells of one window m (bool [Hm,Wm]) taken from the baseline: a selection (torch.where)."""
    base = baseline_tensor(baseline, x).expand_as(x)
    mm = torch.as_tensor(np.asarray(m)).reshape(1, 1, m.shape[0], m.shape[1]).expand_as(x)
    return torch.where(mm, base, x)


def counts(m):
    """int64 [Hm,Wm]: windows covering each cell."""
    return m.sum(0).astype(np.int64)


def attribution(S, S0, m):
    """S [B,N,K], S0 [B,K], m bool [N,Hm,Wm] -> fp64 [B,K,Hm,Wm]: the mean of S0 - S over the windows covering a cell."""
    drop = np.asarray(S0, dtype=np.float64)[:, None, :] - np.asarray(S, dtype=np.float64)
    return np.einsum("bnk,nhw->bkhw", drop, m.astype(np.float64)) / counts(m).astype(np.float64)


def scores(f, x, m, baseline=0.0, score="prob", chunk=32):
    """f: input rows [R,...] -> log-probabilities (or logits) [R,K] (torch).  Returns (S [B,N,K], S0 [B,K]) fp64 numpy: the softmax
    probability (score='logprob': its logarithm) of sample b with window n occluded, and of the unperturbed sample.  f sees
    window-major batches [n*B, ...]: the samples of window n0, then those of window n0 + 1, ..."""
    return sweep(f, x, m, baseline, perturbed, score, True, chunk)
