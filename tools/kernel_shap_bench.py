#!/usr/bin/env python3
"""Times brainxai.kernel_shap on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000) in bf16 and fp32 storage.

Cases: the EEG input with the 19 electrodes as players, and the spectrogram with an 8 x 16 time-by-frequency grid (128 players), both
with the default budget of 2 M + 2048 coalitions.  Per (storage, case) one JSON line: the split of one call into perturb / forward / fit
(device events around every phase, median of --iters calls after --warmup), perturb + fit as a share of the forward time, the perturb
kernel's achieved write bandwidth, and the same pass composed from torch pieces, timed in the same run, alternating: boolean coalition
masks gathered through the label map, torch.where rows into ops.to_nhwc, torch.linalg.lstsq on the sqrt(w)-scaled reduced system in
fp64 (on the device; on the host where the device build lacks it, which the line says).  The forward passes are the same code in both;
the largest difference between the two sets of values is reported."""
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
CASES = {"eeg": ("electrodes", "electrodes"), "spec": ((8, 16), "8x16 grid")}


def composed(model, eeg, spec, which, seg, Z, w, max_batch, profile):
    """Kernel SHAP from torch pieces; the chunking and the forward passes are those of brainxai.kernel_shap."""
    x = spec if which == "spec" else eeg
    B, (N, M) = x.shape[0], Z.shape
    lib = L.load()
    where = {"lstsq": "device"}

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
    lay = (lambda r: ops.to_nhwc(r, dt)) if which == "spec" else (lambda r: r)
    with X._eval_frozen(model), torch.no_grad():
        done = lap("masks")
        Z_d, seg_d, w_d = torch.from_numpy(Z).to(x.device), torch.from_numpy(seg).to(x.device).long(), torch.from_numpy(w).to(x.device)
        m = Z_d.bool()[:, seg_d]                                                                         # [N, Hm, Wm]
        done.record()
        done = lap("forward")
        fixed = (model.eeg_model(eeg) if which == "spec" else model.spectrogram_model(spec)).float().contiguous()
        clean = run(lay(x), fixed)
        empty = run(lay(torch.zeros_like(x)), fixed)                                                     # zero baseline
        classes = clean.argmax(1)
        done.record()
        S = torch.empty(B, N, 6, dtype=torch.float32, device=x.device)
        zero = torch.zeros((), dtype=x.dtype, device=x.device)
        for b0, nb, n0, n in X._faith_chunks(B, N, max_batch):
            done = lap("perturb")
            rows = lay(torch.where(m[n0:n0 + n][None, :, None], x[b0:b0 + nb, None], zero).reshape(nb * n, *x.shape[1:]))
            done.record()
            done = lap("forward")
            S[b0:b0 + nb, n0:n0 + n] = run(rows, fixed[b0:b0 + nb].repeat_interleave(n, dim=0)).reshape(nb, n, 6)
            done.record()
        done = lap("fit")
        sel = torch.arange(B, device=x.device)
        v1, v0 = clean[sel, classes].double(), empty[sel, classes].double()
        last = Z_d[:, -1:].double()
        sw = w_d.sqrt()[:, None]
        A = (Z_d[:, :-1].double() - last) * sw                                                           # [N, M-1]
        Y = ((S[sel, :, classes].double().T - v0[None]) - last * (v1 - v0)[None]) * sw                   # [N, B]
        try:
            head = torch.linalg.lstsq(A, Y).solution
        except RuntimeError:
            where["lstsq"] = "host"
            head = torch.linalg.lstsq(A.cpu(), Y.cpu()).solution.to(x.device)
        phi = torch.cat([head, (v1 - v0)[None] - head.sum(0, keepdim=True)]).T.contiguous()              # [B, M]
        amap = phi.float()[:, seg_d]
        done.record()
    return phi, amap, where["lstsq"]


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
    ap.add_argument("--inputs", default="eeg,spec")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kernel_shap_bench needs a GPU"
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
            segments, label = CASES[which]
            Hd, Wd = (H, W) if which == "spec" else (CHANS, T)
            seg, M = X._shap_segments("kernel_shap_bench", segments, which, Hd, Wd)
            Z, w, exact = X._shap_coalitions("kernel_shap_bench", M, 2 * M + 2048, 0, None)
            N = Z.shape[0]

            def fused(prof):
                return X._kernel_shap(model, eeg, spec, which, segments, None, 0.0, None, "prob", 0, None, a.max_batch, True, profile=prof)

            def old(prof):
                return composed(model, eeg, spec, which, seg, Z, w, a.max_batch, prof)
            for _ in range(a.warmup):
                fused([]); old([])
            torch.cuda.synchronize()
            new_s, old_s = [], []
            for _ in range(a.iters):                                 # alternating, one process, one device
                prof = []
                res = fused(prof)
                new_s.append(split(prof))
                prof = []
                ref, _, where = old(prof)
                old_s.append(split(prof))
            med = lambda rows: {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}      # noqa: E731
            new_ms, old_ms = med(new_s), med(old_s)
            row_bytes = H * W * 8 * (2 if dt == torch.bfloat16 else 4) if which == "spec" else CHANS * T * 4
            out_bytes = a.batch * (N + 1) * row_bytes
            print(json.dumps({"storage": dname if which == "spec" else "fp32 rows", "input": which, "players": label, "M": M, "N": N, "exact": exact,
                              "batch": a.batch, "rows": a.batch * (N + 2), "split_ms": new_ms, "total_ms": round(sum(new_ms.values()), 3),
                              "perturb_plus_fit_over_forward": round((new_ms["perturb"] + new_ms["fit"]) / new_ms["forward"], 4),
                              "perturb_output_bytes": out_bytes, "perturb_write_GBps": round(out_bytes / (new_ms["perturb"] * 1e-3) / 1e9, 1),
                              "composed_split_ms": old_ms, "composed_total_ms": round(sum(old_ms.values()), 3),
                              "composed_non_forward_ms": round(sum(v for k, v in old_ms.items() if k != "forward"), 3), "composed_lstsq_on": where,
                              "composed_over_fused": round(sum(old_ms.values()) / sum(new_ms.values()), 3),
                              "max_abs_difference_of_values": float((res.values - ref).abs().max()), "values_span": float(res.values.max() - res.values.min())}),
                  flush=True)


if __name__ == "__main__":
    main()
