"""What the restatements of the perturb-and-predict attributions (tests/rise_ref.py, occlusion_ref.py, kernel_shap_ref.py,
scorecam_ref.py, faith_ref.py) have in common: the baseline forms and the chunked sweep of a model over the perturbed rows.  Each
restatement keeps its own ``perturbed`` and its own reductions.  Nothing here imports the package under test."""
import numpy as np
import torch


def baseline_tensor(baseline, x):
    """The three baseline forms as a tensor broadcastable to x: a number; one value per channel (x [B,C,H,W]) or per electrode
    (x [B,1,Chans,T]); a tensor of x's shape."""
    if np.ndim(baseline) == 0:
        return torch.full((1, 1, 1, 1), float(baseline), dtype=x.dtype)
    t = torch.as_tensor(np.asarray(baseline)).to(x.dtype)
    if t.dim() == 1:
        return t.reshape(1, 1, -1, 1) if x.shape[1] == 1 else t.reshape(1, -1, 1, 1)    # [B,1,Chans,T]: per electrode; else per channel
    return t.reshape(x.shape)


def score_fn(score):
    """Model output [R,K] (log-probabilities or logits) -> the fp64 softmax probability ('prob') or its logarithm ('logprob')."""
    return (lambda z: torch.log_softmax(z.double(), dim=1)) if score == "logprob" else (lambda z: torch.softmax(z.double(), dim=1))


def sweep(f, x, m, baseline, perturbed, score, clean, chunk):
    """f: input rows [R,...] -> log-probabilities (or logits) [R,K] (torch); perturbed(x, m[n], baseline) -> x [B,...] seen through mask
    n.  Returns S fp64 numpy [B,N,K], the score of sample b under mask n; with clean=True (S, S0 [B,K]), S0 the score of x itself.
    f sees mask-major batches [n*B, ...] of ``chunk`` masks: the samples of mask n0, then those of mask n0 + 1, ..."""
    B, N = x.shape[0], m.shape[0]
    fn = score_fn(score)
    rows = []
    with torch.no_grad():
        S0 = fn(f(x)).numpy() if clean else None
        for n0 in range(0, N, chunk):
            out = fn(f(torch.cat([perturbed(x, m[n], baseline) for n in range(n0, min(N, n0 + chunk))])))
            rows.append(out.reshape(-1, B, out.shape[1]))
    S = torch.cat(rows).permute(1, 0, 2).contiguous().numpy()
    return (S, S0) if clean else S
