#!/usr/bin/env python3
"""Times brainxai.mask_explain at the benchmark shapes (multimodal model, 64 samples, the arg-max class, deletion, a 16 x 16 grid, the
default regularisers).

Configurations: the 4 x 128 x 256 spectrogram input and the 19 x 2000 EEG input.  Per configuration one JSON line with two variants
timed in one process, alternating, after --warmup calls of each, with device events around the whole call (the last event is
synchronised on):
  fused     brainxai.mask_explain: the rows are one launch (bx_maskopt_rows_*), everything behind the backward pass is bx_maskopt_step
  composed  the same loop from torch pieces: F.interpolate(mode="bilinear", align_corners=False) of an fp32 parameter, the blend,
            autograd through both down to the grid, the regularisers as torch expressions, torch.optim.Adam and clamp_; the model
            passes and the chunking are those of brainxai.mask_explain
The composed loop keeps its moments in fp32 and sums in torch's order, so the two results agree to fp32 rounding carried through the
iterations; their difference is reported, not asserted.  Each variant's median and its spread (min .. max over --iters) are reported,
the ratio of the medians, the split of one call of each variant into rows / forward / backward / step / finish (device events around
every phase) and the fused rows + step phases against the model passes of the same call."""
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

K = 6
CHANS, T, H, W, C = 19, 2000, 128, 256, 4
CONFIGS = {"spec": "spec", "eeg": "eeg"}


def composed(model, eeg, spec, which, n, grid, lr, l1, tv, beta, max_batch, profile=None):
    """The deletion masks of the arg-max class from torch pieces -> (map [B,Hm,Wm], grids [B,gh,gw])."""
    x = spec if which == "spec" else eeg
    net = model.spectrogram_model if which == "spec" else model.eeg_model
    B, dev = x.shape[0], x.device
    Hm, Wm = x.shape[2:]
    gh, gw = min(grid, Hm, 32), min(grid, Wm, 32)
    max_rows = X._row_cap(x, which, getattr(net, "compute_dtype", torch.float32) if which == "spec" else torch.float32, max_batch)
    with X._eval_frozen(model):
        with torch.no_grad(), X._lap(profile, "forward"):
            fixed = X._fixed_branch(model, eeg if which == "spec" else spec, which == "spec")
            out = X._fuse(model, True, which == "spec", net(x), fixed).float()
            classes = out.argmax(1)
        m = torch.ones(B, 1, gh, gw, device=dev, requires_grad=True)
        opt = torch.optim.Adam([m], lr=lr)
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            for row0 in range(0, B, max_rows):
                sl = slice(row0, min(B, row0 + max_rows))
                with X._lap(profile, "rows"):
                    M = F.interpolate(m[sl], size=(Hm, Wm), mode="bilinear", align_corners=False)
                    r = M * x[sl]                                            # base = 0: base + M * (x - base)
                with X._lap(profile, "forward"):
                    y = X._fuse(model, True, which == "spec", net(r), fixed[sl]).float()
                with X._lap(profile, "backward"):
                    s = y.gather(1, classes[sl, None])[:, 0].exp()
                    ms = m[sl, 0]
                    tvs = ((ms[:, :, 1:] - ms[:, :, :-1]).abs() ** beta).sum((1, 2)) + ((ms[:, 1:] - ms[:, :-1]).abs() ** beta).sum((1, 2))
                    (l1 * (1 - ms).mean((1, 2)) + tv * tvs + s).sum().backward()
            with torch.no_grad(), X._lap(profile, "step"):
                opt.step()
                m.clamp_(0, 1)
        with torch.no_grad(), X._lap(profile, "finish"):
            amap = 1 - F.interpolate(m, size=(Hm, Wm), mode="bilinear", align_corners=False)[:, 0]
    return amap, m.detach()[:, 0]


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
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--l1", type=float, default=0.01)
    ap.add_argument("--tv", type=float, default=0.2)
    ap.add_argument("--tv-beta", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"), help="storage of the spectrogram branch")
    ap.add_argument("--skip-composed", action="store_true", help="time the fused path alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mask_explain_bench needs a GPU"
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.iterations
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
    eeg, spec = O.seeded((B, 1, CHANS, T), 1, "randn").to(dev), O.seeded((B, C, H, W), 3, "rand").to(dev)
    for name in a.configs.split(","):
        which = CONFIGS[name]

        def fused(prof=None):
            return X._mask_explain(model, eeg, spec, which, "deletion", a.grid, n, a.lr, a.l1, a.tv, a.tv_beta, (0.9, 0.999), 1e-8, 0.0, "electrode_time", None,
                                   "prob", a.max_batch, False, True, profile=prof)

        def old(prof=None):
            return composed(model, eeg, spec, which, n, a.grid, a.lr, a.l1, a.tv, a.tv_beta, a.max_batch, profile=prof)
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
        res = outs["fused"]
        ph = phases["fused"]
        model_ms = ph["forward"] + ph["backward"]
        line = {"config": name, "storage": a.dtype if which == "spec" else "fp32", "input": which, "batch": B, "iterations": n, "grid": list(res.grid),
                "domain": list(res.upsampled.shape[-2:]), "max_batch": a.max_batch, "iters": a.iters}
        for v in variants:
            line[v] = stats(ms[v])
        line["fused_split_ms"] = ph
        line["fused_rows_and_step_over_model_passes"] = round((ph["rows"] + ph["step"]) / model_ms, 4)
        line["fused_rows_ms_per_iteration"] = round(ph["rows"] / n, 4)
        line["fused_step_ms_per_iteration"] = round(ph["step"] / n, 4)
        line["score_first_last"] = [round(float(res.history[:, 0, 0].mean()), 4), round(float(res.history[:, -1, 0].mean()), 4)]
        line["mean_grid_last"] = round(float(res.history[:, -1, 1].mean()), 4)
        if not a.skip_composed:
            pc = phases["composed"]
            line["composed_over_fused"] = round(line["composed"]["median_ms"] / line["fused"]["median_ms"], 3)
            line["composed_split_ms"] = pc
            line["composed_around_over_fused_around"] = round((pc["rows"] + pc["step"] + pc["backward"] - ph["backward"]) / (ph["rows"] + ph["step"]), 3)
            line["max_abs_grid_difference"] = float((outs["composed"][1] - res.mask).abs().max())
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
