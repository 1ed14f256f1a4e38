#!/usr/bin/env python3
"""Times Grad-CAM on the EEG branch of the bench model (EEG 19 x 2000, spectrogram 4 x 128 x 256, B = 64, evaluation mode): one
JSON line per (target, class_idx) with the time per explain.grad_cam call from device events after warm-up, beside the
spectrogram_model.block3 target at the same batch for comparison.

The share of HBM peak of the conv1 map kernel needs its kernel time, which comes from a profiler run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/eeg_gradcam_bench.py --only conv1:all --iters 20
    python tools/eeg_gradcam_bench.py --only conv1:all --kernel-stats OUT

The second form reads k_eeg_cam_conv1's average duration from the profiler's output (stats CSV or rocpd database) and reports algorithmic bytes
((x + cam [+ raw]) x 4) over that time as a fraction of 8 TB/s, together with the FMA count over the non-packed fp32 VALU rate."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import brainxai

B, CIN, H, W, CHANS, T = 64, 4, 128, 256, 19, 2000
HBM_PEAK = 8.0e12                    # bytes/s
FMA_RATE = 256 * 64 * 2.4e9          # fp32 FMAs/s without packed fp32: 256 CUs x 64 lanes x 2.4 GHz
N_CLS = 6


def conv1_cost(nm, with_raw=False):
    """Algorithmic bytes and FMAs of k_eeg_cam_conv1 at the bench shape (K1 = 64 taps)."""
    x = B * CHANS * T * 4
    maps = B * nm * CHANS * T * 4 * (2 if with_raw else 1)
    return x + maps, B * nm * CHANS * T * 64


def kernel_avg_ns(path, name):
    """Average duration (ns) of kernel `name` from rocprofv3 output: a *kernel_stats.csv (--output-format csv) or the rocpd database."""
    files = sorted(glob.glob(os.path.join(path, "**", "*"), recursive=True)) if os.path.isdir(path) else [path]
    for fn in files:
        if fn.endswith("kernel_stats.csv"):
            with open(fn) as f:
                for row in csv.DictReader(f):
                    if name in row.get("Name", ""):
                        return float(row["AverageNs"])
        elif fn.endswith(".db"):
            import sqlite3
            row = sqlite3.connect(fn).execute("select avg(end - start) from kernels where name like ?", (f"%{name}%",)).fetchone()
            if row and row[0] is not None:
                return float(row[0])
    raise SystemExit(f"{name} not found under {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="target:class, e.g. conv1:all (class: all | none)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --stats output (file or directory): report the conv1 kernel's share")
    a = ap.parse_args()
    if a.kernel_stats:
        ns = kernel_avg_ns(a.kernel_stats, "k_eeg_cam_conv1")
        nm = 1 if (a.only or "conv1:all").endswith("none") else N_CLS
        nbytes, fmas = conv1_cost(nm)
        print(json.dumps({"kernel": "k_eeg_cam_conv1", "maps_per_sample": nm, "avg_us": round(ns / 1e3, 2), "bytes": nbytes,
                          "hbm_share": round(nbytes / (ns * 1e-9) / HBM_PEAK, 3), "fma": fmas,
                          "fma_share_nonpacked": round(fmas / (ns * 1e-9) / FMA_RATE, 3)}))
        return
    assert torch.cuda.is_available(), "eeg_gradcam_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = brainxai.build_multimodal(CHANS, T, CIN, dropout=0.5).to(dev).eval()
    eeg = torch.randn(B, 1, CHANS, T, device=dev)
    spec = torch.rand(B, CIN, H, W, device=dev)
    cases = [(t, c) for t in ("eeg_model.conv1", "eeg_model.depthwiseConv", "eeg_model.separableConv", "spectrogram_model.block3")
             for c in ("all", None)]
    if a.only:
        tgt, cls = a.only.split(":")
        cases = [(t, c) for t, c in cases if t.endswith(tgt) and str(c).lower() == cls.lower()]
    for target, cls in cases:
        for _ in range(a.warmup):
            brainxai.grad_cam(model, eeg, spec, target, cls)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.iters):
            brainxai.grad_cam(model, eeg, spec, target, cls)
        ev[1].record()
        torch.cuda.synchronize()
        us = ev[0].elapsed_time(ev[1]) * 1e3 / a.iters
        print(json.dumps({"target": target, "class_idx": cls, "batch": B, "us_per_call": round(us, 1),
                          "maps_per_s": round(B * (N_CLS if cls == "all" else 1) / (us * 1e-6))}), flush=True)


if __name__ == "__main__":
    main()
