#!/usr/bin/env python3
"""Times brainxai.tracin on the benchmark model (spectrogram 4 x 128 x 256, EEG 19 x 2000, K = 6 classes): N = 16384 training rows, M = 64
test rows, 3 checkpoints, all four layers, top = 10.

Per storage one JSON line: the split of one call into forward (the model's passes and the fused head) / factors / scores / topk -- device
events around every phase, median of --iters calls after --warmup -- and the same pass composed from torch pieces, timed phase by phase
in the same run, alternating: the branches' features by the package's kernels, the heads, the closed-form factors, the pairwise sums as
fp64 torch.einsum and the selection as torch.topk, all on the device without autograd.  The largest difference between the two score
matrices and the agreement of the selected sets are reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import explain as X
from brainxai import ops

H, W, C, CHANS, T, K = 128, 256, 4, 19, 2000, 6


def lap(prof, name):
    return X._lap(prof, name)


def composed(model, cks, rates, train, test, top, max_batch, prof):
    """The pass from torch pieces -> (S fp64 [N,M], proponents, opponents)."""
    em, sm = model.eeg_model, model.spectrogram_model
    saved = [(t, t.detach().clone()) for t in list(model.parameters()) + list(model.buffers())]

    def side(data):
        eeg, spec, target = data
        deltas, acts = [], []
        for b0 in range(0, eeg.shape[0], max_batch):
            with lap(prof, "forward"):
                ef = em.features(eeg[b0:b0 + max_batch]).float()
                gap = sm.features(spec[b0:b0 + max_batch]).float().mean(dim=(2, 3))
                s = torch.log_softmax(gap @ sm.fc.weight.T + sm.fc.bias, dim=1)
                e = torch.log_softmax(ef @ em.dense.weight.T + em.dense.bias, dim=1)
                a1 = torch.cat([e, s], dim=1)
                h = torch.relu(a1 @ model.fc1.weight.T + model.fc1.bias)
                logp = torch.log_softmax(h @ model.fc2.weight.T + model.fc2.bias, dim=1)
            with lap(prof, "factors"):
                t = target[b0:b0 + max_batch].double()
                d2 = t.sum(dim=1, keepdim=True) * logp.double().exp() - t
                d1 = (d2 @ model.fc2.weight.double()) * (h > 0)
                v = d1 @ model.fc1.weight.double()
                de = v[:, :K] - e.double().exp() * v[:, :K].sum(dim=1, keepdim=True)
                ds = v[:, K:] - s.double().exp() * v[:, K:].sum(dim=1, keepdim=True)
            deltas.append((d2, d1, de, ds))
            acts.append((h, a1, ef, gap))
        return [torch.cat([d[l] for d in deltas]) for l in range(4)], [torch.cat([a[l] for a in acts]) for l in range(4)]

    S = None
    try:
        with X._eval_frozen(model), torch.no_grad():
            for sd, eta in zip(cks, rates):
                model.load_state_dict(sd)
                ops.bump_param_epoch()
                (dte, ate), (dtr, atr) = side(test), side(train)
                with lap(prof, "scores"):
                    part = sum(torch.einsum("ik,jk->ij", dtr[l], dte[l]) * (torch.einsum("if,jf->ij", atr[l].double(), ate[l].double()) + 1.0) for l in range(4))
                    S = eta * part if S is None else S + eta * part
            with lap(prof, "topk"):
                pro = torch.topk(S.T, top, dim=1).indices
                opp = torch.topk(S.T, top, dim=1, largest=False).indices
    finally:
        X._rand_restore(saved)
    return S, pro, opp


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=16384)
    ap.add_argument("--test", type=int, default=64)
    ap.add_argument("--checkpoints", type=int, default=3)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--block-rows", type=int, default=16384)
    ap.add_argument("--no-composed", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tracin_bench needs a GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)

    def data(n):
        return (torch.randn(n, 1, CHANS, T, generator=g, device=dev), torch.rand(n, C, H, W, generator=g, device=dev),
                torch.softmax(torch.randn(n, K, generator=g, device=dev), dim=1))
    train, test = data(a.train), data(a.test)
    rates = [1.0, 0.5, 0.1, 0.05][:a.checkpoints] + [0.01] * max(0, a.checkpoints - 4)
    for dt_name in a.dtypes.split(","):
        dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt_name]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        cks = []
        for c in range(a.checkpoints):
            gc = torch.Generator(device=dev).manual_seed(10 + c)
            cks.append({k: (v * (1 + 0.05 * torch.randn(v.shape, generator=gc, device=dev)) if v.is_floating_point() and "running" not in k else v.clone())
                        for k, v in model.state_dict().items()})

        def new(prof):
            return X._tracin(model, cks, train, test, "all", rates, a.top, a.max_batch, a.block_rows, True, True, profile=prof)

        def old(prof):
            return composed(model, cks, rates, train, test, a.top, a.max_batch, prof)
        for _ in range(a.warmup):
            new([])
            if not a.no_composed:
                old([])
        new_s, old_s = [], []
        for _ in range(a.iters):                                     # alternating, one process, one device
            prof = []
            res = new(prof)
            new_s.append(split(prof))
            if not a.no_composed:
                prof = []
                S_old, pro_old, opp_old = old(prof)
                old_s.append(split(prof))
        med = {k: round(float(np.median([r[k] for r in new_s])), 3) for k in new_s[0]}
        line = {"storage": dt_name, "N": a.train, "M": a.test, "checkpoints": a.checkpoints, "top": a.top, "max_batch": a.max_batch, "block_rows": a.block_rows,
                "split_ms": med, "total_ms": round(sum(med.values()), 3),
                "spread_total_ms": [round(min(sum(r.values()) for r in new_s), 3), round(max(sum(r.values()) for r in new_s), 3)]}
        if not a.no_composed:
            cmed = {k: round(float(np.median([r[k] for r in old_s])), 3) for k in old_s[0]}
            analytic = ("factors", "scores", "topk")
            same = lambda x, y: float(np.mean([len(set(p.tolist()) & set(q.tolist())) / a.top for p, q in zip(x.cpu(), y.cpu())]))
            line.update({"composed_split_ms": cmed, "composed_total_ms": round(sum(cmed.values()), 3),
                         "composed_over_new_total": round(sum(cmed.values()) / sum(med.values()), 2),
                         "composed_over_new_analytics": round(sum(cmed[k] for k in analytic) / sum(med[k] for k in analytic), 2),
                         "max_score_difference_relative": float((S_old - res.scores).abs().max() / res.scores.abs().max()),
                         "proponents_shared": same(pro_old, res.proponents), "opponents_shared": same(opp_old, res.opponents)})
        print(json.dumps(line), flush=True)
        del model


if __name__ == "__main__":
    main()
