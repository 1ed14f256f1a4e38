#!/usr/bin/env python3
"""Times brainxai.score_cam on the benchmark model and shapes (spectrogram 4 x 128 x 256, EEG 19 x 2000, B = 4) at block5 and block3 in
bf16 and fp32 storage.

Per (storage, target) one JSON line: the split of one call into range / perturb / forward / combine (device events around every
phase, median of --iters calls after --warmup), range + perturb + combine as a share of the forward time, the perturb kernel's
achieved write bandwidth (the bytes of the masked rows it must write over its time), and the same pass composed from torch pieces,
timed in the same run, alternating: F.interpolate of the whole activation (B x C x H x W fp32 of up-sampled planes), amin / amax,
the normalisation and a broadcast multiply into ops.to_nhwc for the rows, a torch.einsum for the sum.  The forward passes are the
same code in both; the largest difference between the two maps is reported."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O

H, W, C, CHANS, T = 128, 256, 4, 19, 2000


def composed(model, eeg, spec, target, max_batch, profile):
    """Score-CAM (weights='prob', zero baseline, arg-max class) from torch pieces; the chunking and the forward passes are those of
    brainxai.score_cam."""
    B = spec.shape[0]
    lib = L.load()
    sm = model.spectrogram_model
    blk = getattr(sm, target)

    def lap(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        profile.append((name, e0, e1))
        return e1

    def probabilities(e, s):
        logp = ops.FusionHeadFn.apply(e, s, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias).float().contiguous()
        probs = torch.empty_like(logp)
        L.check(lib.bx_softmax_rows(logp.data_ptr(), probs.data_ptr(), logp.shape[0], 6, torch.cuda.current_stream().cuda_stream), "bx_softmax_rows")
        return probs
    dt = getattr(sm, "compute_dtype", torch.float32)
    with X._eval_frozen(model), torch.no_grad():
        done = lap("forward")
        fixed = model.eeg_model(eeg).float().contiguous()
        grabbed = {}
        hook = blk.register_forward_hook(lambda _m, _i, o: grabbed.__setitem__("A", o))
        try:
            s_out = sm(spec)
        finally:
            hook.remove()
        classes = probabilities(fixed, s_out).argmax(1)
        A = grabbed["A"].float()                                                                        # logical NCHW
        done.record()
        done = lap("range")
        U = F.interpolate(A, size=(H, W), mode="bilinear", align_corners=False)                          # B x C x H x W floats
        lo, hi = U.amin(dim=(2, 3), keepdim=True), U.amax(dim=(2, 3), keepdim=True)
        scale = torch.where(hi > lo, 1.0 / (hi - lo), torch.zeros_like(hi))
        done.record()
        Cn = A.shape[1]
        P = torch.empty(B, Cn, 6, dtype=torch.float32, device=spec.device)
        for b0, nb, k0, n in X._faith_chunks(B, Cn, max_batch):
            done = lap("perturb")
            M = ((U[b0:b0 + nb, k0:k0 + n] - lo[b0:b0 + nb, k0:k0 + n]) * scale[b0:b0 + nb, k0:k0 + n]).clamp_max(1.0)
            rows = ops.to_nhwc((M[:, :, None] * spec[b0:b0 + nb, None]).reshape(nb * n, *spec.shape[1:]), dt)       # zero baseline
            done.record()
            done = lap("forward")
            out = sm(rows.permute(0, 3, 1, 2))
            P[b0:b0 + nb, k0:k0 + n] = probabilities(fixed[b0:b0 + nb].repeat_interleave(n, dim=0), out).reshape(nb, n, 6)
            done.record()
        done = lap("combine")
        w = P[torch.arange(B, device=spec.device), :, classes] * (hi > lo).reshape(B, Cn)
        cam = X.resize_bilinear(torch.einsum("bk,bkhw->bhw", w, A).clamp_min(0).contiguous(), (H, W))
        done.record()
    return cam


def split(profile):
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in profile:
        out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--targets", default="block5,block3")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "scorecam_bench needs a GPU"
    dev = torch.device("cuda", 0)
    batch = O.synthetic_batch(batch=a.batch, in_channels=C, height=H, width=W, chans=CHANS)
    eeg, spec = batch["eeg"].to(dev).float().contiguous(), batch["spec"].to(dev).float().contiguous()
    for dname in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[dname]
        torch.manual_seed(0)
        model = brainxai.build_multimodal(CHANS, T, C, dropout=0.0, compute_dtype=dt).to(dev).eval()
        for target in a.targets.split(","):
            def fused(prof):
                return X._score_cam(model, eeg, spec, target, None, "prob", 0.0, True, True, a.max_batch, True, profile=prof)

            def old(prof):
                return composed(model, eeg, spec, target, a.max_batch, prof)
            for _ in range(a.warmup):
                fused([]); old([])
            torch.cuda.synchronize()
            new_s, old_s = [], []
            for _ in range(a.iters):                                 # alternating, one process, one device
                prof = []
                res = fused(prof)
                new_s.append(split(prof))
                prof = []
                ref = old(prof)
                old_s.append(split(prof))
            med = lambda rows: {k: round(float(np.median([r[k] for r in rows])), 3) for k in rows[0]}      # noqa: E731
            new_ms, old_ms = med(new_s), med(old_s)
            Cn, h, w = res.A.shape[3], res.A.shape[1], res.A.shape[2]
            out_bytes = a.batch * Cn * H * W * 8 * (2 if dt == torch.bfloat16 else 4)
            print(json.dumps({"storage": dname, "target": target, "batch": a.batch, "channels": Cn, "plane": [h, w], "rows": a.batch * Cn,
                              "split_ms": new_ms, "total_ms": round(sum(new_ms.values()), 3),
                              "non_forward_over_forward": round(sum(v for k, v in new_ms.items() if k != "forward") / new_ms["forward"], 4),
                              "perturb_output_bytes": out_bytes, "perturb_write_GBps": round(out_bytes / (new_ms["perturb"] * 1e-3) / 1e9, 1),
                              "composed_split_ms": old_ms, "composed_total_ms": round(sum(old_ms.values()), 3),
                              "composed_non_forward_ms": round(sum(v for k, v in old_ms.items() if k != "forward"), 3),
                              "materialised_mask_bytes": a.batch * Cn * H * W * 4,
                              "max_abs_difference": float((res.cam - ref).abs().max()), "map_span": float(res.cam.max() - res.cam.min())}), flush=True)


if __name__ == "__main__":
    main()
