#!/usr/bin/env python3
"""Times brainxai.map_similarity by phase for the two map shapes of the benchmark geometry, [64,128,256] (spectrogram maps) and
[64,19,2000] (electrode-by-time maps), and one brainxai.randomization_test of grad_cam over the default spectrogram cascade.

Per shape one JSON line with two variants timed in one process, alternating, after --warmup calls of each, with device events around
every phase (the last event is synchronised on):
  fused     the library's kernels: ranks (bx_rank_desc and bx_rank_average of both maps), correlations (bx_map_corr over the ranks and
            over the values, bx_topk_overlap), ssim (bx_row_minmax of both maps and bx_ssim_rows, uniform window of 7)
  composed  the same pass from torch pieces on the same device: ranks from two argsorts per map (stable, descending; ties are NOT
            averaged -- torch has no rankdata), fp64 correlations and the top-k count from comparisons, SSIM from the rescaled maps with
            fp64 avg_pool2d over the five moment planes (stride 1, no padding: the cropped positions)
Each phase's median and spread (min .. max over --iters) are reported with the ratio of the medians, whichever way it falls, and the
largest difference of the two results per metric (the composed ranks differ where cells tie; random maps have almost none).
The randomization line times the whole call (grad_cam at block5, eight stages, spearman and ssim) and, for scale, nine plain grad_cam
calls -- what the maps alone cost."""
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

SHAPES = {"spec_maps": (64, 128, 256), "eeg_maps": (64, 19, 2000)}
PHASES = ("ranks", "correlations", "ssim")
WIN, TOPK = 7, 0.1


def lap(prof, name, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    prof.append((name, e0, e1))
    return out


def fused(a, b, prof):
    H, W = a.shape[-2:]
    k = max(1, int(np.ceil(TOPK * H * W)))
    A, Bm = X._SimMap(a, False), X._SimMap(b, False)
    taps = torch.from_numpy(X._sim_taps("uniform", WIN)).to(a.device)
    cov = WIN * WIN / (WIN * WIN - 1.0)
    lap(prof, "ranks", lambda: (A.average_ranks(), Bm.average_ranks()))
    out = lap(prof, "correlations", lambda: {m: X._sim_metric(m, A, Bm, H, W, WIN, cov, k, taps, None) for m in ("spearman", "pearson", "topk")})
    out["ssim"] = lap(prof, "ssim", lambda: X._sim_metric("ssim", A, Bm, H, W, WIN, cov, k, taps, None))
    return out


def _corr64(x, y):
    x, y = x.double(), y.double()
    dx, dy = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
    return (dx * dy).sum(1) / torch.sqrt((dx * dx).sum(1) * (dy * dy).sum(1))


def composed(a, b, prof):
    R, H, W = a.shape
    N = H * W
    k = max(1, int(np.ceil(TOPK * N)))
    fa, fb = a.reshape(R, N), b.reshape(R, N)

    def ranks(v):
        return torch.argsort(torch.argsort(v, dim=1, descending=True, stable=True), dim=1)
    ra, rb = lap(prof, "ranks", lambda: (ranks(fa), ranks(fb)))
    out = lap(prof, "correlations", lambda: {"spearman": _corr64(ra, rb), "pearson": _corr64(fa, fb), "topk": ((ra < k) & (rb < k)).sum(1).double() / k})

    def ssim():
        def unit(v):
            v = v.double()
            lo, hi = v.amin((1, 2), keepdim=True), v.amax((1, 2), keepdim=True)
            return (v - lo) / (hi - lo)
        x, y = unit(a), unit(b)
        planes = torch.stack([x, y, x * x, y * y, x * y], 1)
        ux, uy, uxx, uyy, uxy = F.avg_pool2d(planes, WIN, stride=1).unbind(1)
        cov = WIN * WIN / (WIN * WIN - 1.0)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        S = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
        return S.mean((1, 2))
    out["ssim"] = lap(prof, "ssim", ssim)
    return out


def split(prof):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in prof:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(min(ms)), 3), "max_ms": round(float(max(ms)), 3)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="spec_maps,eeg_maps")
    ap.add_argument("--no-randomization", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "map_similarity_bench needs a GPU"
    dev = torch.device("cuda", 0)
    for name in a.shapes.split(","):
        shape = SHAPES[name]
        x = O.seeded(shape, 21, "randn").to(dev)
        y = (0.7 * x + 0.5 * O.seeded(shape, 22, "randn").to(dev)).contiguous()
        variants = {"fused": fused, "composed": composed}
        for _ in range(a.warmup):
            for fn in variants.values():
                fn(x, y, [])
        torch.cuda.synchronize()
        ms = {v: {p: [] for p in PHASES} for v in variants}
        outs = {}
        for _ in range(a.iters):                                     # alternating, one process, one device
            for v, fn in variants.items():
                prof = []
                outs[v] = fn(x, y, prof)
                for p, t in split(prof).items():
                    ms[v][p].append(t)
        line = {"config": name, "shape": list(shape), "win": WIN, "topk": TOPK, "iters": a.iters}
        for p in PHASES:
            f, c = stats(ms["fused"][p]), stats(ms["composed"][p])
            line[p] = {"fused": f, "composed": c, "composed_over_fused": round(c["median_ms"] / f["median_ms"], 3),
                       "fused_slower_than_composed_beyond_spread": bool(f["min_ms"] > c["max_ms"])}
        line["max_abs_difference"] = {m: float((outs["fused"][m] - outs["composed"][m]).abs().max()) for m in outs["fused"]}
        print(json.dumps(line), flush=True)
    if not a.no_randomization:
        B = 64
        torch.manual_seed(0)
        model = brainxai.build_multimodal(19, 2000, 4, dropout=0.0, compute_dtype=torch.bfloat16).to(dev).eval()
        eeg = O.seeded((B, 1, 19, 2000), 1, "randn").to(dev)
        spec = O.seeded((B, 4, 128, 256), 3, "rand").to(dev)

        def cam(m, e, s):
            return brainxai.grad_cam(m, e, s, "spectrogram_model.block5")

        def test():
            return brainxai.randomization_test(model, cam, eeg, spec, seed=0)

        def maps_alone():
            return [cam(model, eeg, spec) for _ in range(9)]
        for _ in range(a.warmup):
            test(), maps_alone()
        torch.cuda.synchronize()
        ms = {"randomization_test": [], "nine_grad_cam_calls": []}
        for _ in range(a.iters):
            ms["randomization_test"].append(timed(test)[0])
            ms["nine_grad_cam_calls"].append(timed(maps_alone)[0])
        res = test()
        line = {"config": "randomization_test grad_cam block5, default spectrogram cascade", "batch": B, "storage": "bf16", "stages": len(res.layers),
                "metrics": list(res.similarity), "iters": a.iters}
        line.update({k: stats(v) for k, v in ms.items()})
        line["mean_similarity_by_stage"] = {m: [round(float(t), 4) for t in v.nanmean(0).tolist()] for m, v in res.similarity.items()}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
