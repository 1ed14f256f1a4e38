#!/usr/bin/env python3
"""Times brainxai.smooth_grad at the benchmark shapes (n = 50 draws per sample, noise level 0.15, all 6 classes, 4 samples).

Configurations: the stand-alone EEGNet at 19 x 2000, and the multimodal model with the 4 x 128 x 256 spectrogram input and with the
19 x 2000 EEG input.  Per configuration one JSON line with two variants timed in one process, alternating, after --warmup calls of
each, with device events around the whole call (the last event is synchronised on):
  fused     brainxai.smooth_grad
  composed  the same pass from torch pieces: torch.randn for the noise of a pass (materialised), a scale kernel and an add kernel for
            the rows, the library's forward, torch.autograd.grad per class, sums of g and g * g in torch fp64 index_add-ed per sample,
            the estimator and the channel maximum in torch
The composed pass draws other noise (torch's generator), so the two results agree as estimates only; their difference is reported
against the largest value, not asserted.  Each variant's median and its spread (min .. max over --iters) are reported, the ratio of
the medians, the split of one call of each variant into sigma / rows / forward / backward / accumulate / finish (device events around
every phase), and for the fused row launches the achieved rates: bytes computed from the shapes (every row written once; x comes from
cache) over the device-event time of the rows phase as a share of the 8 TB/s HBM peak, and normal draws per second."""
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

HBM_PEAK = 8.0e12
K = 6
CONFIGS = {"eegnet_19x2000": ("eegnet", "eeg"), "multimodal_spec_4x128x256": ("multimodal", "spec"), "multimodal_eeg_19x2000": ("multimodal", "eeg")}
CHANS, T, H, W, C = 19, 2000, 128, 256, 4


def composed(model, eeg, spec, which, n, level, kind, max_batch, gen, profile=None):
    """The three estimators of every class from torch pieces; the chunking and the forward passes are those of brainxai.smooth_grad."""
    x = spec if which == "spec" else eeg
    multimodal = hasattr(model, "eeg_model")
    net = (model.spectrogram_model if which == "spec" else model.eeg_model) if multimodal else model
    B, dev = x.shape[0], x.device
    dt = getattr(net, "compute_dtype", torch.float32) if which == "spec" else torch.float32
    max_rows = X._row_cap(x, which, dt, max_batch)
    with X._eval_frozen(model):
        with X._lap(profile, "sigma"):
            flat = x.flatten(1)
            sigma = level * (flat.amax(1) - flat.amin(1))
        with torch.no_grad(), X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, eeg if which == "spec" else spec, which == "spec") if multimodal else None
        S1 = torch.zeros(B, K, x[0].numel(), dtype=torch.float64, device=dev)
        S2 = torch.zeros_like(S1)
        for row0 in range(0, B * n, max_rows):
            rows = min(max_rows, B * n - row0)
            with X._lap(profile, "rows"):
                sample = torch.arange(row0, row0 + rows, device=dev) // n
                z = torch.randn(rows, *x.shape[1:], device=dev, generator=gen)
                nz = z * sigma[sample].view(-1, 1, 1, 1)
                r = (x[sample] + nz).requires_grad_(True)
            with X._lap(profile, "forward"):
                y = X._fuse(model, multimodal, which == "spec", net(r), None if fixed is None else fixed[sample]).float()
            for c in range(K):
                with X._lap(profile, "backward"):
                    seed = torch.zeros(rows, K, dtype=torch.float32, device=dev)
                    seed[:, c] = 1.0
                    (g,) = torch.autograd.grad(y, r, grad_outputs=seed, retain_graph=c + 1 < K)
                with X._lap(profile, "accumulate"):
                    g64 = g.double().flatten(1)
                    S1[:, c].index_add_(0, sample, g64)
                    S2[:, c].index_add_(0, sample, g64 * g64)
        with X._lap(profile, "finish"):
            v = {"smoothgrad": S1 / n, "smoothgrad_sq": S2 / n, "vargrad": ((S2 - S1 * S1 / n) / n).clamp_min(0.0)}[kind]
            values = v.float().reshape(B, K, *x.shape[1:])
            amap = values.abs().amax(2)
    return values, amap


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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--nsamples", type=int, default=50)
    ap.add_argument("--noise-level", type=float, default=0.15)
    ap.add_argument("--kind", default="vargrad", choices=sorted(X._SMOOTHGRAD_KINDS))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"), help="storage of the spectrogram branch (multimodal configurations)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "smooth_grad_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.nsamples
    for name in a.configs.split(","):
        kind, which = CONFIGS[name]
        torch.manual_seed(0)
        eeg, spec = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev), None
        if kind == "eegnet":
            model = brainxai.EEGNet(K, Chans=CHANS, Samples=T, dropoutRate=0.0).to(dev).eval()
        else:
            dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
            model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
            spec = O.seeded((B, C, H, W), 3, "rand").to(dev)
        x = spec if which == "spec" else eeg
        per = x[0].numel()
        gen = torch.Generator(device=dev).manual_seed(0)

        def fused(prof=None):
            return X._smooth_grad(model, eeg, spec, which, n, a.noise_level, None, a.kind, "all", 0, a.max_batch, True, profile=prof).values

        def old(prof=None):
            return composed(model, eeg, spec, which, n, a.noise_level, a.kind, a.max_batch, gen, profile=prof)[0]
        variants = {"fused": fused, "composed": old}
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
        row_bytes = B * n * per * 4
        rate = row_bytes / (phases["fused"]["rows"] * 1e-3)
        line = {"config": name, "storage": a.dtype if which == "spec" else "fp32", "input": which, "kind": a.kind, "batch": B, "nsamples": n, "classes": K,
                "rows": B * n, "max_batch": a.max_batch, "iters": a.iters}
        for v in variants:
            line[v] = stats(ms[v])
        line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
        line["fused_slower_than_composed_beyond_spread"] = bool(line["fused"]["min_ms"] > line["composed"]["max_ms"])
        line["max_abs_difference_over_max"] = float((outs["composed"] - outs["fused"]).abs().max()) / float(outs["fused"].abs().max())
        line.update({"fused_split_ms": phases["fused"], "composed_split_ms": phases["composed"], "rows_bytes": row_bytes, "rows_GBps": round(rate / 1e9, 1),
                     "rows_share_of_hbm_peak": round(rate / HBM_PEAK, 4), "rows_Gnormals_per_s": round(B * n * per / (phases["fused"]["rows"] * 1e-3) / 1e9, 2)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
