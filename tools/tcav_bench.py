#!/usr/bin/env python3
"""Times brainxai.tcav on the benchmark model (spectrogram 4 x 128 x 256, EEG 19 x 2000, K = 6 classes): B = 64 test samples, Q = 4
concepts, R = 10 random sets, n = 50 examples per set (M = 700 stacked rows, P = 50 classifiers), class_idx=None, at
'spectrogram_model.block5' (D = 8192) and 'spectrogram_model.block1' (D = 131072), fp32 and bf16 storage.

Per (target, storage) one JSON line: the split of one call into activations / gram (mean + Gram) / fit / vectors / gradients / sensitivity
(+ score) -- device events around every phase, median of --iters calls after --warmup -- and the same pass composed from torch pieces,
timed phase by phase in the same run, alternating: activations by a forward hook, the centred Gram matrix as an fp64 torch.matmul, one
fp64 torch.linalg.solve per problem in the dual, the CAVs as an fp64 matmul, the gradients by the package's capture and autograd, the
dot products as an fp64 einsum and the scores by comparisons.  The largest differences between the two sets of CAVs and scores are
reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import explain as X

H, W, C, CHANS, T, K = 128, 256, 4, 19, 2000, 6


def lap(prof, name):
    return X._lap(prof, name)


def composed(model, eeg, spec, sets, Q, target, ridge, prof):
    """The pass from torch pieces -> (V fp64 [P,D], scores fp64 [P,K])."""
    net = model.spectrogram_model
    m = X._TARGET.match(target)
    blk = getattr(net, f"block{m.group(1)}")
    n, R = sets[0].shape[0], len(sets) - Q
    with X._eval_frozen(model):
        with lap(prof, "activations"), torch.no_grad():
            kept = []
            h = blk.register_forward_hook(lambda _m, _i, o: kept.append(o.detach().permute(0, 2, 3, 1).reshape(o.shape[0], -1)))
            for s in sets:
                net(s)
            h.remove()
            A = torch.cat(kept).double()
        with lap(prof, "gram"):
            Ac = A - A.mean(dim=0)
            G0 = Ac @ Ac.T
        with lap(prof, "fit"):
            pairs = [(q, Q + r) for q in range(Q) for r in range(R)] + [(Q + r, Q + (r + 1) % R) for r in range(R)]
            ar = torch.arange(n, device=A.device)
            y = torch.cat([torch.ones(n), -torch.ones(n)]).double().to(A.device)
            Hm = torch.eye(2 * n, dtype=torch.float64, device=A.device) - 1.0 / (2 * n)
            beta = torch.zeros(len(pairs), A.shape[0], dtype=torch.float64, device=A.device)
            for p, (sp, sn) in enumerate(pairs):
                I = torch.cat([sp * n + ar, sn * n + ar])
                Kc = Hm @ G0[I][:, I] @ Hm
                lam = ridge * torch.trace(Kc) / (2 * n)
                beta[p, I] = Hm @ torch.linalg.solve(Kc + lam * torch.eye(2 * n, dtype=torch.float64, device=A.device), Hm @ y)
        with lap(prof, "vectors"):
            Wv = beta @ Ac
            V = Wv / Wv.norm(dim=1, keepdim=True)
        with lap(prof, "gradients"):
            x = spec.clone().requires_grad_(True)
            with X._SpecTarget(blk, 0, want_input=True) as tgt:
                out = model(eeg, x)
                G = X._class_grads(out, tgt.leaf, -1, tgt.grad)
        with lap(prof, "sensitivity"):
            S = torch.einsum("bd,pd->bp", G.reshape(G.shape[0], -1).double(), V)
            cls = out.detach().argmax(dim=1)
            scores = torch.stack([(S[cls == k] > 0).double().mean(dim=0) for k in range(K)], dim=1)
    return V, scores


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--concepts", type=int, default=4)
    ap.add_argument("--randoms", type=int, default=10)
    ap.add_argument("--examples", type=int, default=50)
    ap.add_argument("--targets", default="spectrogram_model.block5,spectrogram_model.block1")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tcav_bench needs a GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    eeg, spec = torch.randn(a.batch, 1, CHANS, T, generator=g).to(dev), torch.rand(a.batch, C, H, W, generator=g).to(dev)
    Q, R, n = a.concepts, a.randoms, a.examples
    sets = [torch.rand(n, C, H, W, generator=g).to(dev) for _ in range(Q + R)]
    for q in range(Q):
        sets[q][:, :, 16 * q:16 * (q + 1)] += 0.5                    # a band of the spectrogram per concept
    concepts, randoms = {f"band{q}": sets[q] for q in range(Q)}, sets[Q:]
    for dt_name in a.dtypes.split(","):
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt_name]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        for target in a.targets.split(","):
            def new(prof):
                return X._tcav(model, eeg, spec, concepts, randoms, None, "spec", target, "ridge", 1e-2, 0.0, None, a.max_batch, True, profile=prof)

            def old(prof):
                return composed(model, eeg, spec, sets, Q, target, 1e-2, prof)
            for _ in range(a.warmup):
                new([])
                if not a.no_composed:
                    old([])
            new_s, old_s = [], []
            for _ in range(a.iters):                                 # alternating, one process, one device
                prof = []
                res = new(prof)
                new_s.append(split(prof))
                if not a.no_composed:
                    prof = []
                    V_old, sc_old = old(prof)
                    old_s.append(split(prof))
            med = {k: round(float(np.median([r[k] for r in new_s])), 3) for k in new_s[0]}
            line = {"target": target, "storage": dt_name, "B": a.batch, "Q": Q, "R": R, "n": n, "M": (Q + R) * n, "P": int(res.cavs.vectors.shape[0]),
                    "D": int(res.cavs.vectors.shape[1]), "split_ms": med, "total_ms": round(sum(med.values()), 3),
                    "spread_total_ms": [round(min(sum(r.values()) for r in new_s), 3), round(max(sum(r.values()) for r in new_s), 3)]}
            if not a.no_composed:
                cmed = {k: round(float(np.median([r[k] for r in old_s])), 3) for k in old_s[0]}
                concept = [k for k in ("gram", "fit", "vectors", "sensitivity")]
                line.update({"composed_split_ms": cmed, "composed_total_ms": round(sum(cmed.values()), 3),
                             "composed_over_new_total": round(sum(cmed.values()) / sum(med.values()), 2),
                             "composed_over_new_concept_side": round(sum(cmed[k] for k in concept) / sum(med[k] for k in concept), 2),
                             "max_cav_difference": float((V_old - res.cavs.vectors.double()).norm(dim=1).max()),
                             "max_score_difference": float(torch.nan_to_num(sc_old - torch.cat([res.scores_per_random.reshape(Q * R, K), res.null_scores])).abs().max())})
            print(json.dumps(line), flush=True)
        del model


if __name__ == "__main__":
    main()
