#!/usr/bin/env python3
"""Times brainxai.deletion_insertion on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000, B = 64, steps = 32,
both curves) in bf16 and fp32 storage, and scores the package's attribution methods with it.

Per (storage, input) one JSON line: ms per call from device events around --iters calls after --warmup, the split of one further
call into rank / perturb / forward / curve (device events around each phase), and the same curves computed the way a user would
without it -- torch.sort + torch.where + model(eeg, spec) per step, the unchanged branch evaluated again at every step -- timed in
the same run, alternating, with the largest difference between the two results.

Then one table (JSON line per method): mean deletion / insertion area of the three class-activation methods, saliency, integrated
gradients and a 16 x 16-grid LIME heat-map on the synthetic batch (--table-batch samples), bf16 storage."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import explain as X
from oracle import ref_torch as O

H, W, C, CHANS, T = 128, 256, 4, 19, 2000


def composed(model, eeg, spec, amap, which, steps):
    """The curves from what the package offered before: torch.sort, torch.where on fp32 tensors, the whole model per step."""
    x = spec if which == "spec" else eeg
    B = x.shape[0]
    flat = amap.reshape(B, -1).float()
    key = torch.where(torch.isnan(flat), torch.full_like(flat, float("-inf")), flat)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    N = flat.shape[1]
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(N, device=x.device).expand(B, N))
    rank = rank.reshape(B, 1, x.shape[2], x.shape[3]) if N == x.shape[2] * x.shape[3] else rank.reshape(B, 1, 1, x.shape[3])
    per = -(-N // steps)
    was = model.training
    model.eval()
    outs = {"deletion": [], "insertion": []}
    zero = torch.zeros_like(x)
    with torch.no_grad():
        for i in range(steps + 1):
            below = rank < min(N, i * per)
            for m in outs:
                xi = torch.where(below, zero, x) if m == "deletion" else torch.where(below, x, zero)
                outs[m].append(model(eeg, xi) if which == "spec" else model(xi, spec))
        cls = outs["deletion"][0].argmax(1)
        res = {m: torch.stack(v, 1).float().exp()[torch.arange(B), :, cls] for m, v in outs.items()}
    model.train(was)
    return res


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--inputs", default="spec,eeg")
    ap.add_argument("--table-batch", type=int, default=16)
    ap.add_argument("--no-table", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "faithfulness_bench needs a GPU"
    dev = torch.device("cuda", 0)
    batch = O.synthetic_batch(batch=a.batch, in_channels=C, height=H, width=W, chans=CHANS)
    eeg, spec = batch["eeg"].to(dev).float().contiguous(), batch["spec"].to(dev)
    for dname in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        es, ss = brainxai.saliency(model, eeg, spec)
        for which in a.inputs.split(","):
            amap = ss if which == "spec" else es
            call = lambda: brainxai.deletion_insertion(model, eeg, spec, amap, input=which, steps=a.steps)                         # noqa: E731
            phases = lambda prof: X._deletion_insertion(model, eeg, spec, amap, which, "both", a.steps, 0.0, None, "prob", 256, profile=prof)   # noqa: E731
            old = lambda: composed(model, eeg, spec, amap, which, a.steps)                                                        # noqa: E731
            for _ in range(a.warmup):
                call(); old()
            torch.cuda.synchronize()
            new_ms, old_ms = [], []
            for _ in range(a.iters):                                 # alternating, one process, one device
                new_ms.append(timed(call, 1))
                old_ms.append(timed(old, 1))
            prof = []
            res = phases(prof)
            torch.cuda.synchronize()
            split = {}
            for name, e0, e1 in prof:
                split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
            ref = old()
            diff = max(float((res.deletion - ref["deletion"]).abs().max()), float((res.insertion - ref["insertion"]).abs().max()))
            rows = 2 * (a.steps + 1) * a.batch
            print(json.dumps({"storage": dname, "input": which, "batch": a.batch, "steps": a.steps, "rows": rows,
                              "ms_per_call": round(float(np.median(new_ms)), 3), "ms_min": round(min(new_ms), 3),
                              "split_ms": {k: round(v, 3) for k, v in split.items()},
                              "forward_share": round(split.get("forward", 0.0) / max(sum(split.values()), 1e-9), 3),
                              "rows_per_s": round(rows / (float(np.median(new_ms)) * 1e-3)),
                              "composed_ms_per_call": round(float(np.median(old_ms)), 3), "composed_ms_min": round(min(old_ms), 3),
                              "max_abs_difference": diff}), flush=True)
    for B, N in ((64, 32768), (64, 38000), (1, 32768), (1, 120000), (1, (1 << 20) - 1)):      # bx_rank_desc alone: one workgroup per row
        vals = torch.rand(B, N, device=dev)
        brainxai.attribution_ranks(vals)
        torch.cuda.synchronize()
        print(json.dumps({"rank_only": True, "batch": B, "cells": N, "ms": round(timed(lambda: brainxai.attribution_ranks(vals), 5), 3)}), flush=True)
    if a.no_table:
        return
    # The table needs a model whose output depends on its input: deterministic test weights (oracle.fill_params) with the heads scaled
    # down as in tests/test_gpu_faithfulness.py (unscaled they saturate at p = 0.9999); a default-initialised model is flat.
    n = a.table_batch
    ref = O.fill_params(O.build_multimodal(CHANS, T, C, dropout=0.0), seed=42)
    with torch.no_grad():
        ref.spectrogram_model.fc.weight *= 0.05
        ref.eeg_model.dense.weight *= 0.05
        ref.fc2.weight *= 0.5
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=torch.bfloat16)
    model.load_state_dict(ref.state_dict())
    model = model.to(dev).eval()
    imgs = (spec[:n].permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8)             # LIME takes 8-bit images:
    e, s = eeg[:n].contiguous(), (imgs.permute(0, 3, 1, 2).float() / 255.0).contiguous()            # every method sees the quantised batch
    maps = {m: brainxai.grad_cam(model, e, s, method=m) for m in ("gradcam", "gradcam++", "layercam")}
    maps["saliency"] = brainxai.saliency(model, e, s)[1]
    maps["integrated_gradients"] = brainxai.integrated_gradients(model, (e, s), n_steps=20)[1].abs().sum(1)
    with torch.no_grad():
        cls = model(e, s).argmax(1).tolist()
    seg = brainxai.grid_segments(H, W, 16, 16)
    imgs_h = imgs.cpu().numpy()
    heat = []
    for b in range(n):                                               # LIME explains the spectrogram branch (forward_spectrogram) for the fused model's class
        exp = brainxai.lime_image(model, imgs_h[b], seg, labels=(cls[b],), num_samples=300)
        heat.append(exp.heatmap(cls[b]))
    maps["lime_16x16"] = torch.stack(heat)
    maps["random"] = torch.rand(n, H, W, device=dev)
    for name, amap in maps.items():
        r = brainxai.deletion_insertion(model, e, s, amap, steps=a.steps, class_idx=cls)
        print(json.dumps({"method": name, "samples": n, "deletion_auc": round(float(r.deletion_auc.mean()), 5),
                          "insertion_auc": round(float(r.insertion_auc.mean()), 5)}), flush=True)


if __name__ == "__main__":
    main()
