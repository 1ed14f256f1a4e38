#!/usr/bin/env python3
"""Times brainxai.rise on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000, N = 4000 masks, grid 8) in bf16
and fp32 storage.

Per (storage, input) one JSON line: the split of one call into perturb / forward / accumulate (device events around every phase,
median of --iters calls after --warmup), perturb + accumulate as a share of the forward time, the perturb kernel's achieved write
bandwidth (the bytes of the masked rows it must write over its time), and the same pass composed from what the package offered
before, timed in the same run, alternating: the masks materialised (rise_masks, N x Hm x Wm fp32), a torch broadcast multiply into
ops.to_nhwc for the rows, a torch.einsum for the weighted sum.  The forward passes are the same code in both; the largest difference
between the two maps is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O

H, W, C, CHANS, T = 128, 256, 4, 19, 2000


def composed(model, eeg, spec, which, bits, shifts, grid, p1, max_batch, profile):
    """RISE from existing pieces; the chunking and the forward passes are those of brainxai.rise."""
    x = spec if which == "spec" else eeg
    B, N = x.shape[0], bits.shape[0]
    Hm, Wm = (H, W) if which == "spec" else (CHANS, T)
    lib = L.load()

    def lap(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        profile.append((name, e0, e1))
        return e1
    dt = getattr(model.spectrogram_model, "compute_dtype", torch.float32) if which == "spec" else torch.float32
    with X._eval_frozen(model), torch.no_grad():
        done = lap("masks")
        m = brainxai.rise_masks((Hm, Wm), grid=grid, masks=(bits, shifts), device=x.device)
        done.record()
        done = lap("forward")
        fixed = (model.eeg_model(eeg) if which == "spec" else model.spectrogram_model(spec)).float().contiguous()
        classes = model(eeg, spec).float().argmax(1)
        done.record()
        P = torch.empty(B, N, 6, dtype=torch.float32, device=x.device)
        for b0, nb, n0, n in X._faith_chunks(B, N, max_batch):
            done = lap("perturb")
            rows = (m[n0:n0 + n][None, :, None] * x[b0:b0 + nb, None]).reshape(nb * n, *x.shape[1:])          # zero baseline
            rows = ops.to_nhwc(rows, dt) if which == "spec" else rows
            done.record()
            done = lap("forward")
            if which == "spec":
                out = model.spectrogram_model(rows.permute(0, 3, 1, 2))
            else:
                out = model.eeg_model(rows)
            rep = fixed[b0:b0 + nb].repeat_interleave(n, dim=0)
            e, s = (rep, out) if which == "spec" else (out, rep)
            logp = ops.FusionHeadFn.apply(e, s, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias).float().contiguous()
            probs = torch.empty_like(logp)
            L.check(lib.bx_softmax_rows(logp.data_ptr(), probs.data_ptr(), nb * n, 6, torch.cuda.current_stream().cuda_stream), "bx_softmax_rows")
            P[b0:b0 + nb, n0:n0 + n] = probs.reshape(nb, n, 6)
            done.record()
        done = lap("accumulate")
        w = P[torch.arange(B, device=x.device), :, classes]                                               # [B, N]
        sal = torch.einsum("bn,nhw->bhw", w, m) / (N * p1)
        done.record()
    return sal


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--masks", type=int, default=4000)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--inputs", default="spec,eeg")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rise_bench needs a GPU"
    dev = torch.device("cuda", 0)
    batch = O.synthetic_batch(batch=a.batch, in_channels=C, height=H, width=W, chans=CHANS)
    eeg, spec = batch["eeg"].to(dev).float().contiguous(), batch["spec"].to(dev).float().contiguous()
    p1 = 0.5
    for dname in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        for which in a.inputs.split(","):
            Hm, Wm = (H, W) if which == "spec" else (CHANS, T)
            geom = X._rise_geometry("rise_bench", a.grid, Hm, Wm)
            bits, shifts = X._rise_mask_set("rise_bench", a.masks, geom, p1, 0, None)

            def fused(prof):
                return X._rise(model, eeg, spec, which, a.masks, a.grid, p1, None, 0.0, "expected", 0, (bits, shifts), "electrode_time", a.max_batch, False,
                               profile=prof)

            def old(prof):
                return composed(model, eeg, spec, which, bits, shifts, a.grid, p1, a.max_batch, prof)
            for _ in range(a.warmup):
                fused([]); old([])
            torch.cuda.synchronize()
            new_s, old_s = [], []
            for _ in range(a.iters):                                 # alternating, one process, one device
                prof = []
                sal = fused(prof)
                new_s.append(split(prof))
                prof = []
                ref = old(prof)
                old_s.append(split(prof))
            med = lambda rows: {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}      # noqa: E731
            new_ms, old_ms = med(new_s), med(old_s)
            row_bytes = H * W * 8 * (2 if dt == torch.bfloat16 else 4) if which == "spec" else CHANS * T * 4
            out_bytes = a.batch * a.masks * row_bytes
            print(json.dumps({"storage": dname, "input": which, "batch": a.batch, "masks": a.masks, "grid": a.grid, "rows": a.batch * a.masks,
                              "split_ms": new_ms, "total_ms": round(sum(new_ms.values()), 3),
                              "perturb_plus_accumulate_over_forward": round((new_ms["perturb"] + new_ms["accumulate"]) / new_ms["forward"], 4),
                              "perturb_output_bytes": out_bytes, "perturb_write_GBps": round(out_bytes / (new_ms["perturb"] * 1e-3) / 1e9, 1),
                              "composed_split_ms": old_ms, "composed_total_ms": round(sum(old_ms.values()), 3),
                              "composed_non_forward_ms": round(sum(v for k, v in old_ms.items() if k != "forward"), 3),
                              "materialised_mask_bytes": a.masks * Hm * Wm * 4,
                              "max_abs_difference": float((sal - ref).abs().max()), "map_span": float(sal.max() - sal.min())}), flush=True)


if __name__ == "__main__":
    main()
