#!/usr/bin/env python3
"""Times brainxai.spectral_gradients and brainxai.spectral_occlusion at the benchmark shape (multimodal model, 64 samples, 19 x 2000 EEG).

Configurations: spectral_gradients for one class (the arg-max) and for class_idx='all', each at steps 1 and 50; spectral_occlusion with
the clinical bands at 40 Hz for cells 'band' and 'electrode_band'.  Per configuration one JSON line with two variants timed in one
process, alternating, after --warmup calls of each, with device events around the whole call (the last event is synchronised on):
  fused     the package's call
  composed  the same pass from torch pieces: torch.fft.rfft of x and of the gradient sums (the library FFT), the path rows alpha * x, the
            library's forward, torch.autograd.grad, the weighted sum in torch fp64 with index_add per sample, the map from complex
            tensor arithmetic; for the occlusion the rows x - irfft(X * band mask) rounded to fp32 and the library's forward
Each variant's median and its spread (min .. max over --iters) are reported, the ratio of the medians, the split of one call of each
variant into its phases -- 'transform' (x -> X), 'rows', 'forward', 'backward', 'accumulate', 'values' (the gradient's transform and the
map); 'perturb' for the occlusion's rows -- from device events around every phase, the share of the two transform phases in the fused
call, and the achieved rate of the fused transform against its 2 T F fused multiply-adds per row."""
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

K, CHANS, T, H, W, C, FS = 6, 19, 2000, 128, 256, 4, 40.0
F = T // 2 + 1
GRADIENT_CONFIGS = {"one_steps1": (None, 1), "one_steps50": (None, 50), "all_steps1": ("all", 1), "all_steps50": ("all", 50)}
OCCLUSION_CONFIGS = {"occlusion_band": "band", "occlusion_electrode_band": "electrode_band"}


def weights(dev):
    c = torch.full((F,), 2.0, dtype=torch.float64, device=dev)
    c[0] = 1.0
    if T % 2 == 0:
        c[T // 2] = 1.0
    return c


def composed_gradients(model, eeg, spec, kind, n, class_idx, max_batch, profile=None):
    """The map from torch pieces; the chunking and the forward passes are those of brainxai.spectral_gradients."""
    net, dev, B = model.eeg_model, eeg.device, eeg.shape[0]
    per = CHANS * T
    alpha, w = (np.ones(1), np.ones(1)) if n == 1 else X.ig_nodes(n)
    alpha_d, w_d = torch.from_numpy(alpha.astype(np.float32)).to(dev), torch.from_numpy(np.asarray(w, dtype=np.float64)).to(dev)
    Kc = K if class_idx == "all" else 1
    max_rows = min(X._row_cap(eeg, "eeg", torch.float32, max_batch), ((1 << 31) - 1) // per)
    with X._eval_frozen(model):
        with torch.no_grad(), X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, spec, False)
            out = X._fuse(model, True, False, net(eeg), fixed).float()
            classes = out.argmax(1)
        with X._lap(profile, "transform"):
            Xf = torch.fft.rfft(eeg[:, 0].double(), dim=-1)
        acc = torch.zeros(B, Kc, per, dtype=torch.float64, device=dev)
        for row0 in range(0, B * n, max_rows):
            rows = min(max_rows, B * n - row0)
            with torch.no_grad(), X._lap(profile, "rows"):
                j = torch.arange(row0, row0 + rows, device=dev)
                sample, step = j // n, j % n
                r = alpha_d[step].view(-1, 1, 1, 1) * eeg[sample]
            with X._lap(profile, "forward"):
                r.requires_grad_(True)
                y = X._fuse(model, True, False, net(r), fixed[sample]).float()
            for slot in range(Kc):
                with X._lap(profile, "backward"):
                    seed = torch.zeros(rows, K, dtype=torch.float32, device=dev)
                    seed[torch.arange(rows, device=dev), classes[sample] if Kc == 1 else slot] = 1.0
                    (g,) = torch.autograd.grad(y, r, grad_outputs=seed, retain_graph=slot + 1 < Kc)
                with X._lap(profile, "accumulate"):
                    acc[:, slot].index_add_(0, sample, w_d[step].view(-1, 1) * g.double().flatten(1))
        with X._lap(profile, "values"):
            G = torch.fft.rfft(acc.reshape(B, Kc, CHANS, T), dim=-1)
            lead = Xf[:, None]
            if kind == "amplitude_gradient":
                A = lead.abs()
                lead = torch.where(A == 0, torch.ones_like(lead), lead / torch.where(A == 0, torch.ones_like(A), A))
            amap = (weights(dev) / T * (lead * G.conj()).real).float()
    return amap if Kc > 1 else amap[:, 0]


def composed_occlusion(model, eeg, spec, bins, cells, max_batch, profile=None):
    """The drops of the arg-max class from torch pieces: rows x - irfft(X * band mask), the library's forward and softmax."""
    net, dev, B = model.eeg_model, eeg.device, eeg.shape[0]
    nb = len(bins)
    N = nb if cells == "band" else nb * CHANS
    mask = torch.zeros(nb, F, dtype=torch.float64, device=dev)
    for q, (lo, hi) in enumerate(bins):
        mask[q, lo:hi] = 1.0
    max_rows = X._row_cap(eeg, "eeg", torch.float32, max_batch)
    with X._eval_frozen(model), torch.no_grad():
        with X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, spec, False)
            clean = X._softmax_rows(X._rows_forward(model, net, True, False, eeg, fixed))
            classes = clean.argmax(1)
        with X._lap(profile, "transform"):
            Xf = torch.fft.rfft(eeg[:, 0].double(), dim=-1)
        S = torch.empty(B, N, K, dtype=torch.float32, device=dev)
        for b0, ng, n0, n in X._faith_chunks(B, N, max_rows):
            with X._lap(profile, "perturb"):
                j = torch.arange(n0, n0 + n, device=dev)
                q = j if cells == "band" else j // CHANS
                y = torch.fft.irfft(Xf[b0:b0 + ng, None] * mask[q][None, :, None, :], n=T, dim=-1)              # [ng, n, Chans, T]
                if cells != "band":
                    y = y * torch.nn.functional.one_hot(j % CHANS, CHANS).double()[None, :, :, None]
                rows = (eeg[b0:b0 + ng].double() - y).float().reshape(ng * n, 1, CHANS, T)
            with X._lap(profile, "forward"):
                S[b0:b0 + ng, n0:n0 + n] = X._softmax_rows(X._rows_forward(model, net, True, False, rows, fixed[b0:b0 + ng].repeat_interleave(n, dim=0))).reshape(ng, n, K)
        d = (clean[:, None] - S).gather(2, classes.reshape(B, 1, 1).expand(B, N, 1))[:, :, 0]
    return d if cells == "band" else d.reshape(B, nb, CHANS).transpose(1, 2)


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
    ap.add_argument("--kind", default="gradient_x_amplitude", choices=sorted(X._SPECTRAL_KINDS))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(list(GRADIENT_CONFIGS) + list(OCCLUSION_CONFIGS)))
    ap.add_argument("--skip-composed", action="store_true", help="time the fused path alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "spectral_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B = a.batch
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=torch.bfloat16).to(dev).eval()
    eeg, spec = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev), O.seeded((B, C, H, W), 3, "rand").to(dev)
    bins = brainxai.spectral_band_bins("clinical", T, FS)
    for name in a.configs.split(","):
        if name in GRADIENT_CONFIGS:
            class_idx, n = GRADIENT_CONFIGS[name]

            def fused(prof=None):
                return X._spectral_gradients(model, eeg, spec, a.kind, n, None, None, class_idx, a.max_batch, False, profile=prof)

            def old(prof=None):
                return composed_gradients(model, eeg, spec, a.kind, n, class_idx, a.max_batch, profile=prof)
            line = {"config": name, "call": "spectral_gradients", "kind": a.kind, "classes": K if class_idx == "all" else 1, "steps": n, "rows": B * n}
        else:
            cells = OCCLUSION_CONFIGS[name]

            def fused(prof=None):
                return X._spectral_occlusion(model, eeg, spec, "clinical", FS, cells, None, "prob", a.max_batch, False, profile=prof)

            def old(prof=None):
                return composed_occlusion(model, eeg, spec, bins, cells, a.max_batch, profile=prof)
            line = {"config": name, "call": "spectral_occlusion", "cells": cells, "bands": bins, "rows": B * len(bins) * (1 if cells == "band" else CHANS)}
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
        line.update({"batch": B, "chans": CHANS, "T": T, "max_batch": a.max_batch, "iters": a.iters})
        for v in variants:
            line[v] = stats(ms[v])
        line["fused_split_ms"] = phases["fused"]
        spectral = phases["fused"].get("transform", 0.0) + phases["fused"].get("values", 0.0) + phases["fused"].get("perturb", 0.0)
        line["fused_spectral_share"] = round(spectral / max(sum(phases["fused"].values()), 1e-9), 4)
        fma = 2.0 * T * F * B * CHANS                                # x -> X: two fused multiply-adds per (t, f) of every row
        line["transform_GFMA_per_s"] = round(fma / (phases["fused"]["transform"] * 1e-3) / 1e9, 1)
        if not a.skip_composed:
            line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
            line["fused_slower_than_composed_beyond_spread"] = bool(line["fused"]["min_ms"] > line["composed"]["max_ms"])
            line["max_abs_difference_over_max"] = float((outs["composed"] - outs["fused"]).abs().max()) / float(outs["fused"].abs().max())
            line["composed_split_ms"] = phases["composed"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
