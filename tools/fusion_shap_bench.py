#!/usr/bin/env python3
"""Times brainxai.fusion_shap on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000; K = 6 classes, Hd = 128): B
samples, players='votes' (M = 12: 4096 coalitions + the 4 modality masks), Nb background samples.

Per Nb one JSON line: the split of one call into branches / values / shapley (device events around every phase, median of --iters calls
after --warmup), the head evaluations per second of the values launch, and the same values pass composed from the pieces that exist
without the kernel, timed in the same run, alternating: composed rows by torch indexing, ops.FusionHeadFn, bx_softmax_rows, an fp64
running mean over the background rows.  The largest difference between the two sets of values v is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O

H, W, C, CHANS, T, K = 128, 256, 4, 19, 2000, 6


def composed_values(model, votes, bg, masks_d):
    """v fp64 [B,NS,K] of probabilities from existing pieces, one background row at a time (B * NS composed rows in memory)."""
    lib = L.load()
    B, NS = votes.e.shape[0], masks_d.shape[0]
    bits = ((masks_d.to(torch.int64)[:, None] >> torch.arange(2 * K, device=masks_d.device)[None, :]) & 1).bool()
    zx, zb = torch.cat([votes.e, votes.s], 1), torch.cat([bg.e, bg.s], 1)
    total = torch.zeros(B, NS, K, dtype=torch.float64, device=masks_d.device)
    with torch.no_grad():
        for j in range(zb.shape[0]):
            rows = torch.where(bits[None], zx[:, None, :], zb[j][None, None, :]).reshape(B * NS, 2 * K)
            logp = ops.FusionHeadFn.apply(rows[:, :K].contiguous(), rows[:, K:].contiguous(), model.fc1.weight, model.fc1.bias, model.fc2.weight,
                                          model.fc2.bias).float().contiguous()
            probs = torch.empty_like(logp)
            L.check(lib.bx_softmax_rows(logp.data_ptr(), probs.data_ptr(), B * NS, K, torch.cuda.current_stream().cuda_stream), "bx_softmax_rows")
            total += probs.double().reshape(B, NS, K)
    return total / zb.shape[0]


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--backgrounds", default="1,100")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fusion_shap_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=torch.bfloat16).to(dev).eval()
    batch = O.synthetic_batch(batch=a.batch, in_channels=C, height=H, width=W, chans=CHANS)
    eeg, spec = batch["eeg"].to(dev).float().contiguous(), batch["spec"].to(dev).float().contiguous()
    masks = X._fusion_masks(X._fusion_players("fusion_shap_bench", "votes", K), K)
    masks_d = torch.from_numpy(masks.view(np.int32)).to(dev)
    for Nb in (int(v) for v in a.backgrounds.split(",")):
        g = torch.Generator().manual_seed(Nb)
        bg = (torch.randn(Nb, 1, CHANS, T, generator=g).to(dev), torch.rand(Nb, C, H, W, generator=g).to(dev))

        def fused(prof):
            return X._fusion_shap(model, eeg, spec, bg, "votes", None, "prob", a.max_batch, True, profile=prof)

        def old(res):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            v = composed_values(model, res.votes, res.background, masks_d)
            e1.record()
            torch.cuda.synchronize()
            return v, e0.elapsed_time(e1)
        for _ in range(a.warmup):
            old(fused([]))
        torch.cuda.synchronize()
        new_s, old_ms = [], []
        for _ in range(a.iters):                                     # alternating, one process, one device
            prof = []
            res = fused(prof)
            new_s.append(split(prof))
            v_old, ms = old(res)
            old_ms.append(ms)
        med = {k: round(float(np.median([r[k] for r in new_s])), 3) for k in new_s[0]}
        comp = round(float(np.median(old_ms)), 3)
        evals = a.batch * Nb * masks.shape[0]
        n = masks.shape[0] - 4
        diff = float((res.v - v_old[:, :n]).abs().max())
        print(json.dumps({"batch": a.batch, "Nb": Nb, "players": "votes", "M": 12, "masks": int(masks.shape[0]), "head_evaluations": evals,
                          "split_ms": med, "total_ms": round(sum(med.values()), 3),
                          "values_Gevals_per_s": round(evals / (med["values"] * 1e-3) / 1e9, 3),
                          "composed_values_ms": comp, "composed_over_kernel": round(comp / med["values"], 2),
                          "spread_values_ms": [round(min(r["values"] for r in new_s), 3), round(max(r["values"] for r in new_s), 3)],
                          "spread_composed_ms": [round(min(old_ms), 3), round(max(old_ms), 3)],
                          "max_abs_difference_of_v": diff, "efficiency_gap": float((res.values.sum(-1) - (res.clean - res.empty).gather(
                              1, res.classes[:, None])[:, 0]).abs().max())}), flush=True)


if __name__ == "__main__":
    main()
