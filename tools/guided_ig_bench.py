#!/usr/bin/env python3
"""Times brainxai.guided_ig at the benchmark shapes (multimodal model, 64 samples, the arg-max class, fraction 0.25, max_dist 0.02).

Configurations: the 4 x 128 x 256 spectrogram input and the 19 x 2000 EEG input.  Per configuration one JSON line with two variants
timed in one process, alternating, after --warmup calls of each, with device events around the whole call (the last event is
synchronised on):
  fused     brainxai.guided_ig: a step's inner loop is one launch (bx_guided_ig_step), the host is asked nothing inside a step
  composed  the same pass from torch pieces: the clamp, the sums (torch fp64 sums), torch.kthvalue for the threshold, torch.where for
            the moves, all rows of a pass batched; the inner loop's `while` is tested on the host after every pass (one round trip
            each), as a composition from torch pieces has to
Both follow the definition of include/brainxai.h up to the order of the fp64 sums, so the two results agree unless a rounding flips a
decision; their difference is reported against the largest value, not asserted.  Each variant's median and its spread (min .. max
over --iters) are reported, the ratio of the medians, the split of one call of each variant into forward / backward / step / finish
(device events around every phase; the composed variant's step phase contains its host round trips), the fused step phase against the
model passes of the same call, and the passes the steps took (worst and mean, from the result's ``iterations``)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import explain as X
from oracle import ref_torch as O

K = 6
CHANS, T, H, W, C = 19, 2000, 128, 256, 4
CONFIGS = {"spec": "spec", "eeg": "eeg"}


def point(xb, d, xin, alpha):
    if alpha >= 1.0:
        return xin
    if alpha <= 0.0:
        return xb
    return (xb.double() + alpha * d).float()


def composed_step(xin, xb, x, g, attr, L_total, i, n, k, max_dist):
    """One step for rows [R,P] from torch pieces; -> (x, passes).  attr is updated in place."""
    alpha = (i + 1) / n
    a_min, a_max = max(alpha - max_dist, 0.0), min(alpha + max_dist, 1.0)
    d = xin.double() - xb.double()
    x_min, x_max = point(xb, d, xin, a_min), point(xb, d, xin, a_max)
    L_target = L_total * (1.0 - alpha)
    active = L_total != 0
    inf = torch.tensor(math.inf, dtype=torch.float64, device=x.device)
    passes = 0
    while True:
        passes += 1
        x_old = x
        a = torch.where(d == 0, a_max, (x.double() - xb.double()) / d)
        x = torch.where((a < a_min) & active[:, None], x_min, x)
        L_cur = (xin.double() - x.double()).abs().sum(1)
        close = (L_target - L_cur).abs() <= torch.clamp(1e-9 * torch.maximum(L_target.abs(), L_cur.abs()), min=1e-9)
        rows = active & ~close
        arrived = x == x_max
        keys = torch.where(arrived, math.inf, g.abs())
        theta = torch.kthvalue(keys, k + 1, dim=1).values
        S = ~arrived & (keys <= theta[:, None]) & rows[:, None]
        gap = x_max.double() - x.double()
        L_S = (gap.abs() * S).sum(1)
        gamma = torch.where(L_S > 0, (L_cur - L_target) / L_S, inf)
        x = torch.where(S & (gamma > 1)[:, None], x_max, x)
        x = torch.where(S & ((gamma > 0) & (gamma <= 1))[:, None], (x.double() + gamma[:, None] * gap).float(), x)
        attr += torch.where(active[:, None], (x.double() - x_old.double()) * g.double(), 0.0)
        active = rows & (gamma > 1) & (L_S > 0)
        if not bool(active.any()):                                  # the host's test of the loop: one round trip per pass
            return x, passes


def composed(model, eeg, spec, which, n, fraction, max_dist, max_batch, profile=None):
    """The values of the arg-max class from torch pieces; the chunking and the model passes are those of brainxai.guided_ig."""
    x = spec if which == "spec" else eeg
    net = model.spectrogram_model if which == "spec" else model.eeg_model
    B, dev, per = x.shape[0], x.device, x[0].numel()
    k, _ = brainxai.guided_ig_passes(per, fraction)
    max_rows = X._row_cap(x, which, getattr(net, "compute_dtype", torch.float32) if which == "spec" else torch.float32, max_batch)
    worst = 0
    with X._eval_frozen(model):
        with torch.no_grad(), X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, eeg if which == "spec" else spec, which == "spec")
            out = X._fuse(model, True, which == "spec", net(x), fixed).float()
            classes = out.argmax(1)
        xin = x.reshape(B, per)
        xb = torch.zeros_like(xin)
        xr, attr = xb.clone(), torch.zeros(B, per, dtype=torch.float64, device=dev)
        L_total = (xin.double() - xb.double()).abs().sum(1)
        for i in range(n):
            for row0 in range(0, B, max_rows):
                rows = min(max_rows, B - row0)
                sl = slice(row0, row0 + rows)
                with X._lap(profile, "forward"):
                    r = xr[sl].reshape(rows, *x.shape[1:]).detach().requires_grad_(True)
                    y = X._fuse(model, True, which == "spec", net(r), fixed[sl]).float()
                with X._lap(profile, "backward"):
                    seed = torch.zeros(rows, K, dtype=torch.float32, device=dev)
                    seed[torch.arange(rows, device=dev), classes[sl]] = 1.0
                    (g,) = torch.autograd.grad(y, r, grad_outputs=seed)
                with torch.no_grad(), X._lap(profile, "step"):
                    xr[sl], passes = composed_step(xin[sl], xb[sl], xr[sl], g.reshape(rows, per).float(), attr[sl], L_total[sl], i, n, k, max_dist)
                    worst = max(worst, passes)
        with X._lap(profile, "finish"):
            values = attr.float().reshape(B, *x.shape[1:])
    return values, worst


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return {k: round(v, 3) for k, v in out.items()}


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--fraction", type=float, default=0.25)
    ap.add_argument("--max-dist", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"), help="storage of the spectrogram branch")
    ap.add_argument("--skip-composed", action="store_true", help="time the fused path alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "guided_ig_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.steps
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
    eeg, spec = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev), O.seeded((B, C, H, W), 3, "rand").to(dev)
    for name in a.configs.split(","):
        which = CONFIGS[name]

        def fused(prof=None):
            return X._guided_ig(model, eeg, spec, which, n, a.fraction, a.max_dist, 0.0, None, a.max_batch, False, True, profile=prof)

        def old(prof=None):
            return composed(model, eeg, spec, which, n, a.fraction, a.max_dist, a.max_batch, profile=prof)
        variants = {"fused": fused} if a.skip_composed else {"fused": fused, "composed": old}
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms, outs = {v: [] for v in variants}, {}
        for _ in range(a.iters):                                     # alternating, one process, one device
            for v, fn in variants.items():
                t, outs[v] = timed(fn)
                ms[v].append(t)
        phases = {}
        for v, fn in variants.items():
            prof = []
            fn(prof)
            phases[v] = split(prof)
        res = outs["fused"]
        per = (spec if which == "spec" else eeg)[0].numel()
        k, cap = brainxai.guided_ig_passes(per, a.fraction)
        it = res.iterations.cpu().numpy()
        model_ms = phases["fused"]["forward"] + phases["fused"]["backward"]
        line = {"config": name, "storage": a.dtype if which == "spec" else "fp32", "input": which, "batch": B, "steps": n, "cells": per, "fraction": a.fraction,
                "max_dist": a.max_dist, "k": k, "cap": cap, "max_batch": a.max_batch, "iters": a.iters}
        for v in variants:
            line[v] = stats(ms[v])
        line["fused_split_ms"] = phases["fused"]
        line["fused_step_over_model_passes"] = round(phases["fused"]["step"] / model_ms, 4)
        line["fused_step_ms_per_step"] = round(phases["fused"]["step"] / n, 4)
        line["passes_worst"], line["passes_mean"] = int(it.max()), round(float(it.mean()), 3)
        if not a.skip_composed:
            line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
            line["composed_step_over_fused_step"] = round(phases["composed"]["step"] / phases["fused"]["step"], 3)
            line["max_abs_difference_over_max"] = float((outs["composed"][0] - res.values).abs().max()) / float(res.values.abs().max())
            line["composed_passes_worst"] = outs["composed"][1]
            line["composed_split_ms"] = phases["composed"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
