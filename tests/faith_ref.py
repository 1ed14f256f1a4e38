"""The definition of the deletion / insertion curves (the causal metric of RISE, Petsiuk et al., BMVC 2018) restated with numpy and
torch on the CPU -- what brainxai.attribution_ranks / brainxai.deletion_insertion and the bx_rank_desc / bx_faith_* entry points
are tested against.  Nothing here imports the package under test.

A map has N cells per sample.  Spectrogram input [B,C,H,W]: map [B,H,W], a cell is a pixel with all its channels.  EEG input
[B,1,Chans,T]: map [B,Chans,T] (a cell is one electrode at one time step) or [B,1,T] (a whole time column)."""
import numpy as np
import torch

from tests.perturb_ref import baseline_tensor  # noqa: F401  (part of this module's interface)


def keys(a):
    """fp32 sort keys [B,N]: NaN counts as -inf, -0.0 as +0.0."""
    a = np.asarray(a, dtype=np.float32)
    a = a.reshape(a.shape[0], -1)
    k = np.where(np.isnan(a), np.float32(-np.inf), a).astype(np.float32)
    return np.where(k == 0, np.float32(0.0), k)


def ranks(a):
    """int32 [B,N]: position of every cell in a stable descending sort of its row, ties by ascending flat index."""
    k = keys(a)
    out = np.empty(k.shape, dtype=np.int32)
    for b in range(k.shape[0]):
        order = np.argsort(-k[b], kind="stable")
        out[b, order] = np.arange(k.shape[1], dtype=np.int32)
    return out


def ranks_by_counting(a):
    """The same by the counting definition: rank[i] = #{j : key[j] > key[i]} + #{j < i : key[j] == key[i]} (O(N^2): small rows)."""
    k = keys(a)
    out = np.empty(k.shape, dtype=np.int32)
    for b in range(k.shape[0]):
        row = k[b]
        for i in range(row.size):
            out[b, i] = int((row > row[i]).sum()) + int((row[:i] == row[i]).sum())
    return out


def cuts(N, steps):
    """(per, [k_0 .. k_steps]): per = ceil(N / steps), k_i = min(N, i * per)."""
    per = -(-N // steps)
    return per, [min(N, i * per) for i in range(steps + 1)]


def cell_mask(rank, k, shape):
    """bool tensor broadcastable to the input `shape`: True where the cell's rank is below the cut k.  rank: [B,N] array."""
    B = shape[0]
    below = torch.from_numpy(np.asarray(rank) < k)
    if below.shape[1] == shape[2] * shape[3]:                       # pixels of [B,C,H,W] / electrode x time cells of [B,1,Chans,T]
        return below.reshape(B, 1, shape[2], shape[3])
    assert below.shape[1] == shape[3], (below.shape, shape)        # time columns of [B,1,Chans,T]
    return below.reshape(B, 1, 1, shape[3])


def perturbed(x, rank, baseline, k, insertion):
    """The input at cut k: deletion takes cells of rank < k from the baseline and the others from x, insertion the other way round."""
    below = cell_mask(rank, k, x.shape)
    base = baseline_tensor(baseline, x).expand_as(x)
    return torch.where(below, x, base) if insertion else torch.where(below, base, x)


def auc(curve):
    """RISE's auc: (sum(curve) - curve[0]/2 - curve[-1]/2) / steps, accumulated in fp64 in index order."""
    s = np.float64(0.0)
    for v in curve:
        s = s + np.float64(v)
    return ((s - np.float64(curve[0]) / 2.0) - np.float64(curve[-1]) / 2.0) / np.float64(len(curve) - 1)


def curves(f, x, rank, steps, baseline=0.0, classes=None, score="prob"):
    """f: perturbed input [B,...] -> log-probabilities [B,K] (torch).  Returns a dict: deletion, insertion [B,steps+1] (fp64),
    deletion_auc, insertion_auc [B], classes [B], fractions [steps+1]."""
    N = np.asarray(rank).shape[1]
    _, ks = cuts(N, steps)
    with torch.no_grad():
        logp = {name: torch.stack([f(perturbed(x, rank, baseline, k, ins)) for k in ks], dim=1).double().numpy()
                for name, ins in (("deletion", False), ("insertion", True))}                           # [B, P, K]
    B = x.shape[0]
    if classes is None:
        classes = logp["deletion"][:, 0].argmax(1)
    classes = np.broadcast_to(np.asarray(classes, dtype=np.int64), (B,))
    out = {"classes": classes, "fractions": np.array(ks, dtype=np.float64) / N}
    for name in ("deletion", "insertion"):
        lp = logp[name][np.arange(B), :, classes]
        out[name] = lp if score == "logprob" else np.exp(lp)
        out[name + "_auc"] = np.array([auc(row) for row in out[name]])
    return out
