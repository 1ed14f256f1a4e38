"""numpy fp64 restatement of Fusion SHAP (include/brainxai.h, "Fusion SHAP"): brute force over the vote masks, the mean over the
background rows, the Shapley sum, the modality game and its interaction, and the twins of the host helpers (players -> vote masks,
weights).  A plain module: no tests.  Nothing here shares code with the package.

Votes: z = (e_0..e_K-1, s_0..s_K-1); bit i of a mask set = vote i comes from the sample, clear = from the background row.  A head is
(w1 [Hd,2K], b1 [Hd], w2 [K,Hd], b2 [K])."""
import math

import numpy as np


# ---- host helpers' twins ---------------------------------------------------------------------------------------------------------------------
def players(form, K):
    """The three named forms -> a list of M lists of votes; a partition passes through."""
    if form == "modality":
        return [list(range(K)), list(range(K, 2 * K))]
    if form == "class":
        return [[c, K + c] for c in range(K)]
    if form == "votes":
        return [[i] for i in range(2 * K)]
    return [list(g) for g in form]


def coalition_masks(groups):
    """uint32 [2^M]: the vote mask of coalition S (bit i of S = player i), by the definition, one player and one vote at a time."""
    M = len(groups)
    out = np.zeros(1 << M, dtype=np.uint32)
    for S in range(1 << M):
        mask = 0
        for i in range(M):
            if S >> i & 1:
                for vote in groups[i]:
                    mask |= 1 << vote
        out[S] = mask
    return out


def modality_masks(K):
    """uint32 [4]: none, all EEG votes, all spectrogram votes, all."""
    e = (1 << K) - 1
    return np.array([0, e, e << K, e | (e << K)], dtype=np.uint32)


def weights(M):
    """fp64 [M]: s! (M - s - 1)! / M! for s = 0..M-1."""
    return np.array([math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) for s in range(M)], dtype=np.float64)


def banzhaf_weights(M):
    """The wrong weights a discriminating test must tell from the right ones: uniform 2^-(M-1)."""
    return np.full(M, 2.0 ** -(M - 1), dtype=np.float64)


# ---- the head and the value function ---------------------------------------------------------------------------------------------------------
def head(z, params, relu=True):
    """fp64 log-probabilities [..., K] of fused rows z [..., 2K]."""
    w1, b1, w2, b2 = (np.asarray(p, dtype=np.float64) for p in params)
    h = z @ w1.T + b1
    if relu:
        h = np.maximum(h, 0.0)
    logit = h @ w2.T + b2
    m = logit.max(axis=-1, keepdims=True)
    return logit - (m + np.log(np.exp(logit - m).sum(axis=-1, keepdims=True)))


def scores(logp, score):
    return np.exp(logp) if score == "prob" else logp


def mask_bits(masks, K):
    """bool [NS, 2K]."""
    return (np.asarray(masks, dtype=np.uint64)[:, None] >> np.arange(2 * K, dtype=np.uint64)[None, :] & np.uint64(1)).astype(bool)


def compose(zx, zb_row, bits):
    """[NS, 2K]: the sample's votes where the bit is set, the background row's elsewhere."""
    return np.where(bits, zx[None, :], zb_row[None, :])


def values(e_x, s_x, e_bg, s_bg, masks, params, score, relu=True):
    """v fp64 [B, NS, K]: the mean over the background rows of the score of every class under every mask."""
    K = e_x.shape[1]
    zx = np.concatenate([e_x, s_x], axis=1).astype(np.float64)
    zb = np.concatenate([e_bg, s_bg], axis=1).astype(np.float64)
    bits = mask_bits(masks, K)
    v = np.zeros((zx.shape[0], len(masks), K), dtype=np.float64)
    for b in range(zx.shape[0]):
        for j in range(zb.shape[0]):
            v[b] += scores(head(compose(zx[b], zb[j], bits), params, relu), score)
    return v / zb.shape[0]


def shapley(v, w):
    """phi [..., M] of v [..., 2^M] (coalition = the integer whose bit i is player i) with the size weights w [M]."""
    M = len(w)
    S = np.arange(1 << M)
    size = np.array([bin(s).count("1") for s in S])
    phi = np.zeros(v.shape[:-1] + (M,), dtype=np.float64)
    for i in range(M):
        without = S[(S >> i & 1) == 0]
        phi[..., i] = ((v[..., without | (1 << i)] - v[..., without]) * w[size[without]]).sum(axis=-1)
    return phi


def interaction(v4):
    """v(all) - v(EEG) - v(spec) + v(none) of v4 [..., 4] = (none, EEG, spec, all)."""
    return v4[..., 3] - v4[..., 1] - v4[..., 2] + v4[..., 0]


def explain(e_x, s_x, e_bg, s_bg, groups, params, score, classes=None, relu=True, w=None):
    """-> dict(values [B,K,M] or [B,M] with classes, modality [B,(K,)2], interaction [B(,K)], v [B,2^M,K], clean, empty [B,K])."""
    K = e_x.shape[1]
    v = values(e_x, s_x, e_bg, s_bg, coalition_masks(groups), params, score, relu)
    v4 = values(e_x, s_x, e_bg, s_bg, modality_masks(K), params, score, relu)
    phi = shapley(v.transpose(0, 2, 1), weights(len(groups)) if w is None else w)
    mod = shapley(v4.transpose(0, 2, 1), weights(2))
    inter = interaction(v4.transpose(0, 2, 1))
    if classes is not None:
        rows = np.arange(v.shape[0])
        phi, mod, inter = phi[rows, classes], mod[rows, classes], inter[rows, classes]
    return dict(values=phi, modality=mod, interaction=inter, v=v, clean=v4[:, 3], empty=v4[:, 0])


def linear_closed_form(e_x, s_x, e_bg, s_bg, groups, params):
    """The values of the log-probability's LOGIT part for a head without the ReLU -- there the logits are linear in z, so player i's
    value for logit c is sum over its votes of (w2 w1)[c, vote] * (z_vote - mean background z_vote): [B, K, M]."""
    w1, b1, w2, b2 = (np.asarray(p, dtype=np.float64) for p in params)
    lin = w2 @ w1                                                         # [K, 2K]
    dz = np.concatenate([e_x, s_x], axis=1).astype(np.float64) - np.concatenate([e_bg, s_bg], axis=1).astype(np.float64).mean(axis=0)[None, :]
    return np.stack([(lin[None, :, g] * dz[:, None, g]).sum(axis=-1) for g in groups], axis=-1)


def logit_values(e_x, s_x, e_bg, s_bg, masks, params, relu=True):
    """The value function of the raw logits (no log-softmax) [B, NS, K]: what ``linear_closed_form`` is the Shapley value of."""
    w1, b1, w2, b2 = (np.asarray(p, dtype=np.float64) for p in params)
    K = e_x.shape[1]
    zx = np.concatenate([e_x, s_x], axis=1).astype(np.float64)
    zb = np.concatenate([e_bg, s_bg], axis=1).astype(np.float64)
    bits = mask_bits(masks, K)
    v = np.zeros((zx.shape[0], len(masks), K), dtype=np.float64)
    for b in range(zx.shape[0]):
        for j in range(zb.shape[0]):
            h = compose(zx[b], zb[j], bits) @ w1.T + b1
            v[b] += (np.maximum(h, 0.0) if relu else h) @ w2.T + b2
    return v / zb.shape[0]


# ---- the inputs the tests share --------------------------------------------------------------------------------------------------------------
def random_head(K, Hd, seed):
    """A head drawn at torch's default bounds, U(-1/sqrt(fan_in), 1/sqrt(fan_in)), fp32."""
    g = np.random.default_rng(seed)
    b1, b2 = 1.0 / math.sqrt(2 * K), 1.0 / math.sqrt(Hd)
    return tuple(g.uniform(-b, b, size=s).astype(np.float32) for b, s in ((b1, (Hd, 2 * K)), (b1, (Hd,)), (b2, (K, Hd)), (b2, (K,))))


def random_votes(N, K, seed):
    """fp32 [N,K] log-probabilities: log_softmax(2 N(0,1))."""
    x = 2.0 * np.random.default_rng(seed).standard_normal((N, K))
    m = x.max(axis=1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))).astype(np.float32)
