#!/usr/bin/env python3
"""Times brainxai.lime_image (perturb -> forward -> softmax on the device, fp64 ridge fit on the device) on a Spectrogram_Model in
fp32 and bf16 storage: one JSON line per (case, storage, batch) with the time per explanation from device events after warm-up,
perturbed images/s, and the algorithmic bytes of bx_lime_perturb (the batch written once + image and label map read once per
workgroup pass of 8 samples).

Cases: the reference's call (400 x 300 x 3, N = 100, a 10 x 5 grid for its ~50 SLIC segments), the package default N = 1000 at
S = 192 (400 x 300 x 3, 16 x 12 tiles) and the bench input (128 x 256 x 4, N = 1000, 8 x 16 tiles).

--ref R alternates R times, in the same process, between lime_image and the path the package offered before it: the numpy +
scikit-learn restatement (tests/lime_ref.py: numpy perturbation, uint8 host-to-device copy, scikit-learn fit on the host) around
brainxai.predict_fn; both are timed on the wall clock around a device synchronisation, and median / min / max are reported.
The restatement has no batch form: for a batch it runs once per image.

Kernel times come from a profiler run of their own,

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/lime_bench.py --iters 3 --batches 1

where bx_lime_perturb's bytes here over its kernel time are its share of HBM bandwidth."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai

CASES = {"reference": (400, 300, 3, 100, 10, 5), "default": (400, 300, 3, 1000, 16, 12), "bench": (128, 256, 4, 1000, 8, 16)}   # H W C N rows cols
MAX_BATCH = 256


def perturb_bytes(B, H, W, C, N, esize):
    passes = sum((min(MAX_BATCH, N - n0) + 7) // 8 for n0 in range(0, N, MAX_BATCH))
    return B * (N * H * W * 8 * esize + passes * (H * W * C + H * W * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ref", type=int, default=0, help="alternations with the numpy + scikit-learn path (0: none)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lime_bench needs a GPU"
    dev = torch.device("cuda", 0)
    if a.ref:
        from tests import lime_ref
    for case in a.cases.split(","):
        H, W, C, N, rows, cols = CASES[case]
        seg = brainxai.grid_segments(H, W, rows, cols)
        for dname in a.dtypes.split(","):
            dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
            torch.manual_seed(0)
            model = brainxai.set_compute_dtype(brainxai.Spectrogram_Model(6, in_channels=C), dt).to(dev).eval()
            for B in (int(b) for b in a.batches.split(",")):
                imgs = (np.random.default_rng(B).random((B, H, W, C)) * 255.9).astype(np.uint8)
                segs = np.stack([seg] * B)
                call = lambda: brainxai.lime_image(model, imgs, segs, num_samples=N, max_batch=MAX_BATCH)      # noqa: E731
                for _ in range(a.warmup):
                    call()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / a.iters / B
                rec = {"case": case, "storage": dname, "batch": B, "H": H, "W": W, "C": C, "num_samples": N, "segments": rows * cols,
                       "ms_per_explanation": round(ms, 3), "perturbed_images_per_s": round(N / (ms * 1e-3)),
                       "perturb_bytes": perturb_bytes(B, H, W, C, N, 2 if dt == torch.bfloat16 else 4)}
                if a.ref:
                    clf = lambda ims: brainxai.predict_fn(ims, model, max_batch=MAX_BATCH)                     # noqa: E731
                    new, old = [], []
                    for _ in range(a.ref):
                        torch.cuda.synchronize(); t = time.perf_counter()
                        call()
                        torch.cuda.synchronize(); new.append((time.perf_counter() - t) * 1e3 / B)
                        t = time.perf_counter()
                        for b in range(B):
                            lime_ref.explain(imgs[b], segs[b], clf, num_samples=N)
                        torch.cuda.synchronize(); old.append((time.perf_counter() - t) * 1e3 / B)
                    for name, v in (("new", new), ("ref", old)):
                        rec[f"{name}_wall_ms"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                    rec["alternations"] = a.ref
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
