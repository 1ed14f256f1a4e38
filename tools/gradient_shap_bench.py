#!/usr/bin/env python3
"""Times brainxai.gradient_shap at the reference's SHAP setting (background of 100, 200 draws per sample, all 6 classes, 4 samples).

Configurations: the stand-alone EEGNet at 19 x 2000 and 37 x 3000 (what the reference explains), and the multimodal model with the
4 x 128 x 256 spectrogram input.  Per configuration one JSON line with three variants timed in one process, alternating, after
--warmup calls of each, with device events around the whole call (the last event is synchronised on):
  fused     brainxai.gradient_shap
  host_loop brainxai.expected_gradients on the same seed, hence the same draws (stand-alone models only: it takes no other input)
  composed  the same pass from torch pieces: gathered backgrounds, x - b, b + a * d, the library's forward, torch.autograd.grad per
            class, (d * g) in fp64 index_add-ed per sample
Each variant's median and its spread (min .. max over --iters) are reported, the ratios of the medians, the split of one fused call
into rows / forward / backward / accumulate / finish (device events around every phase), and the accumulate launches' achieved
bandwidth: bytes computed from the shapes (the gradient rows and the gathered background rows read once, x read and the fp64 sum read
and written once per sample a call touches) over the device-event time of the accumulate phase, as a share of the 8 TB/s HBM peak --
the gathered background (Nb rows) mostly comes from cache, so the figure is an algorithmic rate, not HBM traffic."""
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
CONFIGS = {"eegnet_19x2000": ("eegnet", 19, 2000), "eegnet_37x3000": ("eegnet", 37, 3000), "multimodal_spec_4x128x256": ("multimodal", 19, 2000)}
H, W, C = 128, 256, 4


def composed(model, eeg, spec, bg, which, idx_d, alpha_d, max_batch):
    """Expected gradients of every class from torch pieces; the chunking and the forward passes are those of brainxai.gradient_shap."""
    x = spec if which == "spec" else eeg
    multimodal = hasattr(model, "eeg_model")
    net = (model.spectrogram_model if which == "spec" else model.eeg_model) if multimodal else model
    B, n = idx_d.shape
    dev = x.device
    dt = getattr(net, "compute_dtype", torch.float32) if which == "spec" else torch.float32
    max_rows = X._row_cap(x, which, dt, max_batch)
    flat_idx, flat_alpha = idx_d.reshape(-1).long(), alpha_d.reshape(-1)
    with X._eval_frozen(model):
        with torch.no_grad():
            fixed = X._fixed_branch(model, eeg if which == "spec" else spec, which == "spec") if multimodal else None
        acc = torch.zeros(B, K, x[0].numel(), dtype=torch.float64, device=dev)
        for row0 in range(0, B * n, max_rows):
            rows = min(max_rows, B * n - row0)
            sample = torch.arange(row0, row0 + rows, device=dev) // n
            base = bg[flat_idx[row0:row0 + rows]]
            d = x[sample] - base
            r = (base + flat_alpha[row0:row0 + rows].view(-1, 1, 1, 1) * d).requires_grad_(True)
            y = X._fuse(model, multimodal, which == "spec", net(r), None if fixed is None else fixed[sample]).float()
            for c in range(K):
                seed = torch.zeros(rows, K, dtype=torch.float32, device=dev)
                seed[:, c] = 1.0
                (g,) = torch.autograd.grad(y, r, grad_outputs=seed, retain_graph=c + 1 < K)
                acc[:, c].index_add_(0, sample, (d.double() * g.double()).flatten(1))
    return (acc / n).float().reshape(B, K, *x.shape[1:])


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
    return out


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def accumulate_bytes(B, n, per, max_rows):
    """Bytes the accumulate launches of one call need, per class: see the module docstring."""
    total = 0
    for row0 in range(0, B * n, max_rows):
        rows = min(max_rows, B * n - row0)
        touched = (row0 + rows - 1) // n - row0 // n + 1
        total += rows * per * 4 * 2 + touched * per * (4 + 8 + 8)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--nsamples", type=int, default=200)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"), help="storage of the spectrogram branch (multimodal configuration)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gradient_shap_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, Nb, n = a.batch, a.background, a.nsamples
    for name in a.configs.split(","):
        kind, chans, T = CONFIGS[name]
        torch.manual_seed(0)
        eeg, bge = O.seeded((B, 1, chans, T), 1, "randn").to(dev), O.seeded((Nb, 1, chans, T), 2, "randn").to(dev)
        spec = bgs = None
        if kind == "eegnet":
            model, which, bg = brainxai.EEGNet(K, Chans=chans, Samples=T, dropoutRate=0.0).to(dev).eval(), "eeg", bge
        else:
            dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
            model = brainxai.build_multimodal(chans, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
            spec, bgs = O.seeded((B, C, H, W), 3, "rand").to(dev), O.seeded((Nb, C, H, W), 4, "rand").to(dev)
            which, bg = "spec", bgs
        x = spec if which == "spec" else eeg
        per = x[0].numel()
        idx, alpha = X._gradshap_draws("gradient_shap_bench", B, Nb, n, 0, None)
        idx_d, alpha_d = torch.from_numpy(idx).to(dev), torch.from_numpy(alpha).to(dev)

        def fused(prof=None):
            return X._gradient_shap(model, eeg, spec, bg, which, n, "all", 0, None, a.max_batch, True, profile=prof).values

        def old():
            return composed(model, eeg, spec, bg, which, idx_d, alpha_d, a.max_batch)
        variants = {"fused": fused, "composed": old}
        if kind == "eegnet":
            variants["host_loop"] = lambda: brainxai.expected_gradients(model, eeg, bg, nsamples=n, seed=0, max_batch=a.max_batch)
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        ms, outs = {v: [] for v in variants}, {}
        for _ in range(a.iters):                                     # alternating, one process, one device
            for v, fn in variants.items():
                t, outs[v] = timed(fn)
                ms[v].append(t)
        prof = []
        fused(prof)
        phases = {k: round(v, 3) for k, v in split(prof).items()}
        dt_rows = getattr(model.spectrogram_model, "compute_dtype", torch.float32) if which == "spec" else torch.float32
        nbytes = K * accumulate_bytes(B, n, per, X._row_cap(x, which, dt_rows, a.max_batch))
        rate = nbytes / (phases["accumulate"] * 1e-3)
        line = {"config": name, "storage": a.dtype if which == "spec" else "fp32", "input": which, "batch": B, "background": Nb, "nsamples": n, "classes": K,
                "rows": B * n, "max_batch": a.max_batch, "iters": a.iters}
        for v in variants:
            line[v] = stats(ms[v])
        scale = float(outs["fused"].abs().max())
        for v in variants:
            if v != "fused":
                line[f"{v}_over_fused"] = round(line[v]["median_ms"] / line["fused"]["median_ms"], 3)
                line[f"fused_slower_than_{v}_beyond_spread"] = bool(line["fused"]["min_ms"] > line[v]["max_ms"])
                line[f"max_abs_difference_{v}_over_max"] = float((outs[v] - outs["fused"]).abs().max()) / scale
        line.update({"fused_split_ms": phases, "accumulate_bytes": nbytes, "accumulate_GBps": round(rate / 1e9, 1),
                     "accumulate_share_of_hbm_peak": round(rate / HBM_PEAK, 4)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
