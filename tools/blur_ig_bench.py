#!/usr/bin/env python3
"""Times brainxai.blur_ig at the benchmark shapes (multimodal model, 64 samples, n = 50 steps, the arg-max class).

Configurations: the 4 x 128 x 256 spectrogram input (both axes) and the 19 x 2000 EEG input (time axis), each at max_sigma 50 and 10.
Per configuration one JSON line with two variants timed in one process, alternating, after --warmup calls of each, with device events
around the whole call (the last event is synchronised on):
  fused     brainxai.blur_ig
  composed  the same pass from torch pieces: per-row grouped conv2d blurs with the same fp32 taps (one row of taps per filtered axis,
            zero padding), the literal difference (blur(sigma + eps) - blur(sigma)) / eps, the library's forward, torch.autograd.grad,
            the weighted product summed in torch fp64 with index_add per sample, the channel sum in torch
Both follow the same path, so the two results agree up to the cancellation of the literal difference; their difference is reported
against the largest value, not asserted.  Each variant's median and its spread (min .. max over --iters) are reported, the ratio of
the medians, the split of one call of each variant into rows / forward / backward / accumulate / finish (device events around every
phase), and for the fused row launches the achieved rates against the algorithmic figures of DESIGN.md section 4: FLOPs = 2 per tap that
lands inside the image, for two horizontal and three vertical filters (two filters with one axis), bytes = x read once, X and D
written once."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import brainxai
from brainxai import explain as X
from oracle import ref_torch as O

HBM_PEAK, FP32_PEAK = 8.0e12, 157.3e12
K = 6
CHANS, T, H, W, C = 19, 2000, 128, 256, 4
CONFIGS = {"spec_sigma50": ("spec", 50.0), "spec_sigma10": ("spec", 10.0), "eeg_sigma50": ("eeg", 50.0), "eeg_sigma10": ("eeg", 10.0)}


def inside(Ln, R):
    """Taps of a radius-R filter that land inside a line of Ln, summed over its Ln outputs."""
    p = np.arange(Ln)
    return int((np.minimum(p, R) + np.minimum(Ln - 1 - p, R) + 1).sum())


def row_flops(shape, axes, radius):
    """FLOPs of the rows of one sample: per step 2 per tap inside the image; a over R_a, b and d over R_b."""
    Cc, Hh, Ww = shape
    total = 0
    for Ra, Rb in radius.tolist():
        if Rb == 0:
            continue
        if axes == "hw":
            total += 2 * Cc * (Hh * (inside(Ww, Ra) + inside(Ww, Rb)) + Ww * (inside(Hh, Ra) + 2 * inside(Hh, Rb)))
        else:
            lines, Ln = (Cc * Hh, Ww) if axes == "w" else (Cc * Ww, Hh)
            total += 2 * lines * (inside(Ln, Ra) + inside(Ln, Rb))
    return total


def conv_blur(r, taps, axes):
    """r [rows, C, H, W] blurred with one row of taps [rows, TW] per row of r, zero padding: one grouped conv2d per filtered axis."""
    rows, Cc, Hh, Ww = r.shape
    TW = taps.shape[1]
    y = r.reshape(1, rows * Cc, Hh, Ww)
    wt = taps.repeat_interleave(Cc, dim=0)
    if "w" in axes:
        y = F.conv2d(y, wt.view(rows * Cc, 1, 1, TW), padding=(0, TW // 2), groups=rows * Cc)
    if "h" in axes:
        y = F.conv2d(y, wt.view(rows * Cc, 1, TW, 1), padding=(TW // 2, 0), groups=rows * Cc)
    return y.reshape(rows, Cc, Hh, Ww)


def composed(model, eeg, spec, which, n, max_sigma, eps, axes, max_batch, profile=None):
    """The values of the arg-max class from torch pieces; the chunking and the forward passes are those of brainxai.blur_ig."""
    x = spec if which == "spec" else eeg
    net = model.spectrogram_model if which == "spec" else model.eeg_model
    B, dev = x.shape[0], x.device
    sig = X.blur_sigmas(n, max_sigma)
    taps, _ = X.blur_taps(sig[:n], eps)
    ta, tb = torch.from_numpy(taps[:, 0]).to(dev), torch.from_numpy(taps[:, 1]).to(dev)
    w = torch.tensor([-(sig[i + 1] - sig[i]) for i in range(n)], dtype=torch.float64, device=dev)
    max_rows = X._row_cap(x, which, getattr(net, "compute_dtype", torch.float32) if which == "spec" else torch.float32, max_batch, x[0].numel() * 4)
    with X._eval_frozen(model):
        with torch.no_grad(), X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, eeg if which == "spec" else spec, which == "spec")
            out = X._fuse(model, True, which == "spec", net(x), fixed).float()
            classes = out.argmax(1)
        acc = torch.zeros(B, x[0].numel(), dtype=torch.float64, device=dev)
        for row0 in range(0, B * n, max_rows):
            rows = min(max_rows, B * n - row0)
            with torch.no_grad(), X._lap(profile, "rows"):
                j = torch.arange(row0, row0 + rows, device=dev)
                sample, step = j // n, j % n
                xr = x[sample]
                r = conv_blur(xr, ta[step], axes)
                D = (conv_blur(xr, tb[step], axes) - r) / eps
            with X._lap(profile, "forward"):
                r.requires_grad_(True)
                y = X._fuse(model, True, which == "spec", net(r), fixed[sample]).float()
            with X._lap(profile, "backward"):
                seed = torch.zeros(rows, K, dtype=torch.float32, device=dev)
                seed[torch.arange(rows, device=dev), classes[sample]] = 1.0
                (g,) = torch.autograd.grad(y, r, grad_outputs=seed)
            with X._lap(profile, "accumulate"):
                acc.index_add_(0, sample, (w[step].view(-1, 1) * (g.double() * D.double()).flatten(1)))
        with X._lap(profile, "finish"):
            values = acc.float().reshape(B, *x.shape[1:])
            amap = acc.reshape(B, *x.shape[1:]).sum(1).float()
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--grad-step", type=float, default=0.01)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"), help="storage of the spectrogram branch")
    ap.add_argument("--skip-composed", action="store_true", help="time the fused path alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "blur_ig_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.steps
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
    eeg, spec = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev), O.seeded((B, C, H, W), 3, "rand").to(dev)
    for name in a.configs.split(","):
        which, max_sigma = CONFIGS[name]
        axes = "hw" if which == "spec" else "w"
        x = spec if which == "spec" else eeg
        per = x[0].numel()

        def fused(prof=None):
            return X._blur_ig(model, eeg, spec, which, n, max_sigma, False, a.grad_step, axes, None, a.max_batch, True, profile=prof).values

        def old(prof=None):
            return composed(model, eeg, spec, which, n, max_sigma, a.grad_step, axes, a.max_batch, profile=prof)[0]
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
        _, radius = X.blur_taps(X.blur_sigmas(n, max_sigma)[:n], a.grad_step)
        flops, nbytes = B * row_flops(tuple(x.shape[1:]), axes, radius), B * n * per * 4 * 3
        sec = phases["fused"]["rows"] * 1e-3
        line = {"config": name, "storage": a.dtype if which == "spec" else "fp32", "input": which, "axes": axes, "max_sigma": max_sigma, "batch": B, "steps": n,
                "rows": B * n, "max_batch": a.max_batch, "iters": a.iters}
        for v in variants:
            line[v] = stats(ms[v])
        line["fused_split_ms"] = phases["fused"]
        if not a.skip_composed:
            line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
            line["composed_rows_over_fused_rows"] = round(phases["composed"]["rows"] / phases["fused"]["rows"], 3)
            line["fused_slower_than_composed_beyond_spread"] = bool(line["fused"]["min_ms"] > line["composed"]["max_ms"])
            line["max_abs_difference_over_max"] = float((outs["composed"] - outs["fused"]).abs().max()) / float(outs["fused"].abs().max())
            line["composed_split_ms"] = phases["composed"]
        line.update({"rows_flop": flops, "rows_bytes": nbytes, "rows_GFLOPs": round(flops / sec / 1e9, 1), "rows_share_of_fp32_peak": round(flops / sec / FP32_PEAK, 4),
                     "rows_GBps": round(nbytes / sec / 1e9, 1), "rows_share_of_hbm_peak": round(nbytes / sec / HBM_PEAK, 4),
                     "rows_GFLOP_per_row": round(flops / (B * n) / 1e9, 4)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
