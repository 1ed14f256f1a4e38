#!/usr/bin/env python3
"""Times every class-activation method (grad_cam(..., method=...)) on the bench model (EEG 19 x 2000, spectrogram 4 x 128 x 256,
B = 64, all six classes, evaluation mode) in bf16 and fp32 storage: one JSON line per (storage, case, method) with the time per call
from device events after warm-up, maps/s, and the algorithmic bytes of the method's own reduce kernel(s).

Cases: the default target through GradCamSweep (bx_cam_head_sweep), spectrogram_model.block5.conv3 / block3 / block1 through grad_cam
(autograd to the target, then bx_cam_reduce), and EEG conv1 / separableConv (bx_eeg_cam).  The call time includes the forward and the
backward to the target; the kernel time of the reduce comes from a profiler run of its own,

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/cam_methods_bench.py --iters 20

and its bytes here over that time are its share of HBM bandwidth."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import brainxai

B, CIN, H, W, CHANS, T = 64, 4, 128, 256, 19, 2000
N_CLS = 6
METHODS = ("gradcam", "gradcam++", "layercam")
# (h, w, C) of each spectrogram target at the bench shape
SPEC_SHAPES = {"spectrogram_model.block5": (4, 8, 256), "spectrogram_model.block5.conv3": (8, 16, 256),
               "spectrogram_model.block3": (16, 32, 64), "spectrogram_model.block1": (64, 128, 16)}
CASES = ("spectrogram_model.block5", "spectrogram_model.block5.conv3", "spectrogram_model.block3", "spectrogram_model.block1",
         "eeg_model.conv1", "eeg_model.separableConv")


def reduce_bytes(case, method, esize):
    """Algorithmic bytes of the method's reduce launch(es) for one call: each input read once, each output written once."""
    nm = B * N_CLS
    K1, F = 64, 16
    if case == "spectrogram_model.block5":         # A read once; the up-sampled maps written (fp32)
        h, w, C = SPEC_SHAPES[case]
        return B * h * w * C * esize + nm * H * W * 4
    if case in SPEC_SHAPES:                         # A once, G per map, cam (+ weights); the autograd backward is not counted
        h, w, C = SPEC_SHAPES[case]
        return B * h * w * C * esize + nm * h * w * C * esize + nm * h * w * 4 + (0 if method == "layercam" else nm * C * 4)
    T1, T2 = T // 4, T // 32
    if case == "eeg_model.separableConv":           # smap, dfeat, cam
        return B * F * T1 * 4 + nm * F * T2 * 4 + nm * T1 * 4
    # conv1: dmap, smap, dfeat in the gradient kernel; x and the maps in the map kernel; Layer-CAM also writes and reads Gd [16, T]
    grad = B * F * T * 4 + B * F * T1 * 4 + nm * F * T2 * 4
    maps = B * CHANS * T * 4 + nm * CHANS * T * 4
    extra = 2 * nm * F * T * 4 if method == "layercam" else nm * K1 * 4 * 2
    return grad + maps + extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cam_methods_bench needs a GPU"
    dev = torch.device("cuda", 0)
    for dname in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, CIN, dropout=0.5, compute_dtype=dt).to(dev).eval()
        eeg = torch.randn(B, 1, CHANS, T, device=dev)
        spec = torch.rand(B, CIN, H, W, device=dev)
        for case in CASES:
            for method in METHODS:
                if case == "spectrogram_model.block5":
                    sweep = brainxai.GradCamSweep(model, eeg, spec, class_idx="all", method=method)
                    call = lambda: sweep(eeg, spec)                                             # noqa: E731
                else:
                    call = lambda: brainxai.grad_cam(model, eeg, spec, case, "all", upsample=False, method=method)   # noqa: E731
                for _ in range(a.warmup):
                    call()
                torch.cuda.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / a.iters
                print(json.dumps({"storage": dname, "case": case, "method": method, "batch": B, "classes": N_CLS,
                                  "ms_per_call": round(ms, 3), "maps_per_s": round(B * N_CLS / (ms * 1e-3)),
                                  "reduce_bytes": reduce_bytes(case, method, 2 if dt == torch.bfloat16 else 4)}), flush=True)


if __name__ == "__main__":
    main()
