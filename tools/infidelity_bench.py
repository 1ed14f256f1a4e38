#!/usr/bin/env python3
"""Times brainxai.infidelity by phase at the benchmark geometry (B = 64 samples, n = 10 draws per sample, noise level 0.15, the arg-max
class): the multimodal model with the 4 x 128 x 256 spectrogram input (pixel cells, the maps every method returns) and with the
19 x 2000 EEG input (element cells), spectrogram branch in bf16 storage and in fp32 storage.

Per configuration one JSON line with two variants timed in one process, alternating, after --warmup calls of each, with device events
around the whole call (the last event is synchronised on):
  fused     brainxai.infidelity
  composed  the same pass from torch pieces: torch.randn for the noise of a pass (materialised), a scale kernel and a subtract kernel for
            the rows, ops.to_nhwc for the layout, the library's forward and softmax, a torch fp64 dot of the stored noise with the
            attribution, the drops and the mean square in torch fp64
The composed pass draws other noise (torch's generator), so the two results agree as estimates only; their ratio is reported, not
asserted.  Each variant's median and its spread (min .. max over --iters) are reported, the ratio of the medians, the split of one call
of each variant into sigma / perturb / forward / dot / finish (device events around every phase), and for the fused row launches the
achieved rate: bytes computed from the shapes (every row written once; x comes from cache) over the device-event time of the perturb
phase, as a share of the 8 TB/s HBM peak."""
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
from oracle import ref_torch as O

HBM_PEAK = 8.0e12
K = 6
CHANS, T, H, W, C = 19, 2000, 128, 256, 4


def composed(model, eeg, spec, phi, which, n, level, max_batch, gen, profile=None):
    """infidelity [B] fp64 of the arg-max class from torch pieces; the chunking and the forward passes are those of brainxai.infidelity."""
    is_spec = which == "spec"
    x, other = (spec, eeg) if is_spec else (eeg, spec)
    net = model.spectrogram_model if is_spec else model.eeg_model
    B, dev = x.shape[0], x.device
    dt = getattr(net, "compute_dtype", torch.float32) if is_spec else torch.float32
    max_rows = X._row_cap(x, which, dt, max_batch)
    pf = phi.reshape(B, -1).double()

    def scores(rows, rep):
        rows = ops.to_nhwc(rows, dt) if is_spec else rows
        return X._softmax_rows(X._rows_forward(model, net, True, is_spec, rows, rep))
    with X._eval_frozen(model), torch.no_grad():
        with X._lap(profile, "sigma"):
            flat = x.flatten(1)
            sigma = level * (flat.amax(1) - flat.amin(1))
        with X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, other, is_spec)
            clean = scores(x, fixed)
        cls = clean.argmax(1)
        S = torch.empty(B, n, K, dtype=torch.float32, device=dev)
        d = torch.empty(B, n, dtype=torch.float64, device=dev)
        for b0, nb, n0, nn in X._faith_chunks(B, n, max_rows):
            with X._lap(profile, "perturb"):
                z = torch.randn(nb, nn, *phi.shape[1:], device=dev, generator=gen)
                nz = z * sigma[b0:b0 + nb].view(-1, *([1] * (z.dim() - 1)))
                rows = (x[b0:b0 + nb, None] - (nz[:, :, None] if is_spec else nz.reshape(nb, nn, *x.shape[1:]))).reshape(nb * nn, *x.shape[1:])
            with X._lap(profile, "forward"):
                S[b0:b0 + nb, n0:n0 + nn] = scores(rows, fixed[b0:b0 + nb].repeat_interleave(nn, dim=0)).reshape(nb, nn, K)
            with X._lap(profile, "dot"):
                d[b0:b0 + nb, n0:n0 + nn] = (nz.reshape(nb, nn, -1).double() * pf[b0:b0 + nb, None]).sum(-1)
        with X._lap(profile, "finish"):
            idx = cls.view(B, 1, 1).expand(B, n, 1)
            drops = clean.gather(1, cls[:, None]).double() - S.gather(2, idx)[..., 0].double()
            infid = ((d - drops) ** 2).mean(1)
    return infid


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
    ap.add_argument("--nsamples", type=int, default=10)
    ap.add_argument("--noise-level", type=float, default=0.15)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--inputs", default="spec,eeg")
    ap.add_argument("--dtypes", default="bf16,fp32", help="storage of the spectrogram branch")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "infidelity_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.nsamples
    eeg = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev)
    spec = O.seeded((B, C, H, W), 3, "rand").to(dev)
    for dtype in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        for which in a.inputs.split(","):
            x = spec if which == "spec" else eeg
            phi = O.seeded((B, H, W) if which == "spec" else (B, CHANS, T), 5, "randn").to(dev)
            gen = torch.Generator(device=dev).manual_seed(0)

            def fused(prof=None):
                return X._infidelity(model, eeg, spec, phi, which, n, a.noise_level, None, False, None, "prob", 0, a.max_batch, False, profile=prof)

            def old(prof=None):
                return composed(model, eeg, spec, phi, which, n, a.noise_level, a.max_batch, gen, profile=prof)
            variants = {"fused": fused, "composed": old}
            for _ in range(a.warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            ms, outs = {v: [] for v in variants}, {}
            for _ in range(a.iters):                                 # alternating, one process, one device
                for v, fn in variants.items():
                    t, outs[v] = timed(fn)
                    ms[v].append(t)
            phases = {}
            for v, fn in variants.items():
                prof = []
                fn(prof)
                phases[v] = split(prof)
            row_bytes = B * n * (H * W * 8 * (2 if dt == torch.bfloat16 else 4) if which == "spec" else x[0].numel() * 4)
            rate = row_bytes / (phases["fused"]["perturb"] * 1e-3)
            line = {"config": f"multimodal_{which}", "storage": dtype if which == "spec" else "fp32 rows, " + dtype + " other branch", "input": which,
                    "cells": int(phi[0].numel()), "batch": B, "nsamples": n, "rows": B * n, "max_batch": a.max_batch, "iters": a.iters}
            for v in variants:
                line[v] = stats(ms[v])
            line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
            line["fused_slower_than_composed_beyond_spread"] = bool(line["fused"]["min_ms"] > line["composed"]["max_ms"])
            line["mean_infidelity_fused_over_composed"] = float(outs["fused"].mean() / outs["composed"].mean())
            line.update({"fused_split_ms": phases["fused"], "composed_split_ms": phases["composed"], "perturb_bytes": row_bytes,
                         "perturb_GBps": round(rate / 1e9, 1), "perturb_share_of_hbm_peak": round(rate / HBM_PEAK, 4)})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
