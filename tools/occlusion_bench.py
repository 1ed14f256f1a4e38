#!/usr/bin/env python3
"""Times brainxai.occlusion on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000) in bf16 and fp32 storage.

Per (storage, input, geometry) one JSON line: the split of one call into perturb / forward / accumulate (device events around every
phase, median of --iters calls after --warmup), perturb + accumulate as a share of the forward time, the perturb kernel's achieved
write bandwidth (the bytes of the occluded rows it must write over its time), and the same pass composed from torch pieces, timed in
the same run, alternating: boolean window masks, torch.where rows into ops.to_nhwc, a torch.einsum over the masks for the map.  The
forward passes are the same code in both; the largest difference between the two maps is reported."""
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
# input -> geometries (window, stride): a dense sliding window and a band / segment ablation each
GEOMETRIES = {"spec": [((16, 32), (8, 16)), ((8, 256), (4, 256))], "eeg": [((1, 2000), (1, 2000)), ((19, 100), (19, 50))]}


def window_masks(geom, Hm, Wm, device):
    wh, ww, sh, sw, ny, nx = geom
    y, x = torch.arange(Hm, device=device), torch.arange(Wm, device=device)
    y0, x0 = torch.arange(ny, device=device) * sh, torch.arange(nx, device=device) * sw
    my = (y[None] >= y0[:, None]) & (y[None] < y0[:, None] + wh)                                     # [ny, Hm]
    mx = (x[None] >= x0[:, None]) & (x[None] < x0[:, None] + ww)                                     # [nx, Wm]
    return (my[:, None, :, None] & mx[None, :, None, :]).reshape(ny * nx, Hm, Wm)


def composed(model, eeg, spec, which, geom, max_batch, profile):
    """Occlusion from torch pieces; the chunking and the forward passes are those of brainxai.occlusion."""
    x = spec if which == "spec" else eeg
    B, N = x.shape[0], geom[4] * geom[5]
    Hm, Wm = (H, W) if which == "spec" else (CHANS, T)
    lib = L.load()

    def lap(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        profile.append((name, e0, e1))
        return e1

    def run(rows, rep):
        out = model.spectrogram_model(rows.permute(0, 3, 1, 2)) if which == "spec" else model.eeg_model(rows)
        e, s = (rep, out) if which == "spec" else (out, rep)
        logp = ops.FusionHeadFn.apply(e, s, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias).float().contiguous()
        probs = torch.empty_like(logp)
        L.check(lib.bx_softmax_rows(logp.data_ptr(), probs.data_ptr(), logp.shape[0], 6, torch.cuda.current_stream().cuda_stream), "bx_softmax_rows")
        return probs
    dt = getattr(model.spectrogram_model, "compute_dtype", torch.float32) if which == "spec" else torch.float32
    with X._eval_frozen(model), torch.no_grad():
        done = lap("masks")
        m = window_masks(geom, Hm, Wm, x.device)
        done.record()
        done = lap("forward")
        fixed = (model.eeg_model(eeg) if which == "spec" else model.spectrogram_model(spec)).float().contiguous()
        clean = run(ops.to_nhwc(x, dt) if which == "spec" else x, fixed)
        classes = clean.argmax(1)
        done.record()
        S = torch.empty(B, N, 6, dtype=torch.float32, device=x.device)
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        for b0, nb, n0, n in X._faith_chunks(B, N, max_batch):
            done = lap("perturb")
            rows = torch.where(m[n0:n0 + n][None, :, None], zero, x[b0:b0 + nb, None]).reshape(nb * n, *x.shape[1:])      # zero baseline
            rows = ops.to_nhwc(rows, dt) if which == "spec" else rows
            done.record()
            done = lap("forward")
            S[b0:b0 + nb, n0:n0 + n] = run(rows, fixed[b0:b0 + nb].repeat_interleave(n, dim=0)).reshape(nb, n, 6)
            done.record()
        done = lap("accumulate")
        sel = torch.arange(B, device=x.device)
        drop = (clean[sel, classes][:, None] - S[sel, :, classes]).double()                               # [B, N]
        mf = m.double()
        amap = (torch.einsum("bn,nhw->bhw", drop, mf) / mf.sum(0)).float()
        done.record()
    return amap


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--inputs", default="spec,eeg")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "occlusion_bench needs a GPU"
    dev = torch.device("cuda", 0)
    batch = O.synthetic_batch(batch=a.batch, in_channels=C, height=H, width=W, chans=CHANS)
    eeg, spec = batch["eeg"].to(dev).float().contiguous(), batch["spec"].to(dev).float().contiguous()
    for dname in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        for which in a.inputs.split(","):
            if which == "eeg" and dname != a.dtypes.split(",")[0]:
                continue                                             # the EEG rows are fp32 in either storage
            Hm, Wm = (H, W) if which == "spec" else (CHANS, T)
            for window, stride in GEOMETRIES[which]:
                geom = X._occlusion_geometry("occlusion_bench", window, stride, Hm, Wm)
                N = geom[4] * geom[5]

                def fused(prof):
                    return X._occlusion(model, eeg, spec, which, window, stride, 0.0, None, "prob", a.max_batch, False, profile=prof)

                def old(prof):
                    return composed(model, eeg, spec, which, geom, a.max_batch, prof)
                for _ in range(a.warmup):
                    fused([]); old([])
                torch.cuda.synchronize()
                new_s, old_s = [], []
                for _ in range(a.iters):                             # alternating, one process, one device
                    prof = []
                    amap = fused(prof)
                    new_s.append(split(prof))
                    prof = []
                    ref = old(prof)
                    old_s.append(split(prof))
                med = lambda rows: {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}      # noqa: E731
                new_ms, old_ms = med(new_s), med(old_s)
                row_bytes = H * W * 8 * (2 if dt == torch.bfloat16 else 4) if which == "spec" else CHANS * T * 4
                out_bytes = a.batch * N * row_bytes
                print(json.dumps({"storage": dname if which == "spec" else "fp32 rows", "input": which, "window": window, "stride": stride, "grid": geom[4:],
                                  "batch": a.batch, "rows": a.batch * N, "split_ms": new_ms, "total_ms": round(sum(new_ms.values()), 3),
                                  "perturb_plus_accumulate_over_forward": round((new_ms["perturb"] + new_ms["accumulate"]) / new_ms["forward"], 4),
                                  "perturb_output_bytes": out_bytes, "perturb_write_GBps": round(out_bytes / (new_ms["perturb"] * 1e-3) / 1e9, 1),
                                  "composed_split_ms": old_ms, "composed_total_ms": round(sum(old_ms.values()), 3),
                                  "composed_non_forward_ms": round(sum(v for k, v in old_ms.items() if k != "forward"), 3),
                                  "max_abs_difference": float((amap - ref).abs().max()), "map_span": float(amap.max() - amap.min())}), flush=True)


if __name__ == "__main__":
    main()
