"""Helpers shared by the parity tests: fixture loading, the digest rule of oracle/make_golden.py and the
comparison metrics.

Metrics
  rel_err(a, b)            max|a-b| / max|b|                        -- forward values (continuous in the inputs)
  grad_close(a, b, tol..)  the same for gradients, STRICT: no outliers are tolerated.  ``floor`` floors the denominator so that a
                           gradient that is mathematically zero (e.g. d/d gamma of a BatchNorm directly followed by a
                           linear map and another BatchNorm) is compared on the scale of its neighbours, not of its
                           own rounding noise.

Discontinuities.  A gradient is a discontinuous function of the activations (ReLU'(0), max-pool arg-max): one pre-activation
that is +1e-9 on one implementation and -1e-9 on the other changes a patch of an input gradient by O(1), and -- through a late
stage with few positions -- every upstream weight gradient by O(1e-2).  At the benchmark size (100 M activations) a few dozen
such ties exist in every forward.  Round 1 "tolerated" outliers on the ASSUMPTION that they were tie flips.  Now nothing is
assumed:
  * matched_oracle() compares the implementation's stored post-ReLU activations with the oracle's fp64 trace.  Every
    disagreement must be a demonstrated tie (|z|/S < 1e-4, in practice 1e-7 .. 1e-10); anything larger fails the test there.
  * the gradient TARGET is then the fp64 oracle run with those same decisions pinned (oracle.ref_torch.decision_matched_twin).
    With the decisions equal on both sides the comparison is strict again (checked on the CPU: the reference's own fp32
    gradients are 1.6e-2 from the plain fp64 ones when 3 ReLUs flip, and 1.7e-5 from the decision-matched ones).
  * fixtures (recorded fp32 outputs of the reference) are generated on inputs where neither the reference nor the HIP path
    flips (oracle/make_golden.py, tools/flip_scan.py), so they are compared strictly as well.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = 20000
REPORT = []          # (label, max-rel-err, outlier fraction) collected for the end-of-run summary


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _flat(t):
    return torch.as_tensor(t).detach().double().flatten().cpu()


def rel_err(a, b, floor=0.0):
    a, b = _flat(a), _flat(b)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


def grad_close(got, want, tol, label="", floor=0.0, flips=None):
    """Strict.  ``flips`` (observed activation flips of the forward under test, if the caller looked) only enriches the message."""
    a, b = _flat(got), _flat(want)
    assert a.shape == b.shape, f"{label}: {a.shape} vs {b.shape}"
    scale = max(float(b.abs().max()), floor, 1e-30)
    d = (a - b).abs()
    err = float(d.max() / scale)
    frac = float((d > tol * scale).double().mean())
    REPORT.append((label, err, frac))
    if not err <= tol:          # (a NaN anywhere makes err NaN, which `err > tol` would let through)
        hint = ""
        if flips:
            hint = (f"; the forward under test flipped {len(flips)} activation decision(s) against the exact forward ({describe_flips(flips)}): "
                    "compare with matched_oracle(), or re-pick this fixture's input seeds (tools/flip_scan.py)")
        raise AssertionError(f"{label}: rel err {err:.3e} > {tol} at flat index {int(d.argmax())} ({frac:.2%} of elements beyond the tolerance){hint}")
    return err


def describe_flips(flips, limit=4):
    items = [f"{f['stage']}.conv{f['conv']}@{f['index']} |z|/S={f['margin']:.1e}" for f in flips[:limit]]
    return "; ".join(items) + (f"; ... {len(flips)} in all" if len(flips) > limit else "")


def _nchw_acts(keep, trace):
    acts = {}
    for name, d in keep.items():
        if "acts" in d and name in trace:
            acts[name] = [t.detach().float().permute(0, 3, 1, 2)[:, :trace[name]["z"][k].shape[1]].cpu() for k, t in enumerate(d["acts"])]
    return acts


def observed_flips(oracle_mod, ref, args, keep, label=""):
    """Demonstrated activation flips of a GPU forward.  ``ref``: the oracle model in the state the forward saw (call this
    before stepping it); ``args``: the CPU inputs; ``keep``: what brainxai.ops.keep_block_activations(model) returned before
    that forward.  A disagreement whose oracle margin is NOT tiny is an error, not a flip, and fails here."""
    return matched_oracle(oracle_mod, ref, args, keep, label, twin=False)[1]


def matched_oracle(oracle_mod, ref, args, keep, label="", twin=True, storage=None):
    """(fp64 oracle with the GPU forward's ReLU / max-pool decisions pinned, list of observed flips).  See the module docstring.
    ``storage=torch.bfloat16``: the twin restates the product's bf16 storage mode (oracle.ref_torch.decision_matched_twin); the
    legitimacy of the pinned decisions is then read from the twin's own decision log (check_decisions) after its forward."""
    trace = oracle_mod.relu_pool_trace(ref, args)
    acts = _nchw_acts(keep, trace)
    if storage is not None:
        return oracle_mod.decision_matched_twin(ref, acts, storage=storage), None
    flips, errors = oracle_mod.activation_flips(trace, acts)
    assert not errors, f"{label}: activations disagree with the fp64 oracle beyond a tie: {describe_flips(errors)}"
    if flips:
        print(f"[parity] {label}: {len(flips)} activation decision(s) differ from the exact forward, all demonstrated ties: {describe_flips(flips)}")
    return (oracle_mod.decision_matched_twin(ref, acts) if twin else None), flips


def check_decisions(twin, tie, label=""):
    """After a forward of a decision-matched twin: every pinned decision its own arithmetic would have taken the other way must be
    within ``tie`` of a tie (|z|/S for a ReLU, window gap / S for a max-pool).  Returns (count, largest margin)."""
    n = sum(e["count"] for e in twin.decision_log)
    worst = max((e["margin"] for e in twin.decision_log), default=0.0)
    bad = [e for e in twin.decision_log if e["margin"] >= tie]
    assert not bad, f"{label}: pinned decisions that are NOT ties at resolution {tie:g}: {bad[:4]}"
    return n, worst


def summarize(t):
    f = _flat(t)
    ramp = torch.linspace(0.5, 1.5, f.numel(), dtype=torch.float64)
    return np.array([f.sum(), f.abs().sum(), (f * ramp).sum(), (f * f).sum()], dtype=np.float64)


def check(fix, key, value, tol=1e-5, what="", floor=0.0, robust=False, digest=True, flips=None):
    """Compare ``value`` with fixture entry ``key`` (full array, or digest + head for big ones).
    floor: absolute scale below which the reference is treated as zero; robust: gradient-style comparison."""
    value = torch.as_tensor(value).detach().cpu()
    if key in fix:
        want = torch.as_tensor(fix[key])
        assert tuple(value.shape) == tuple(want.shape), f"{what}{key}: shape {tuple(value.shape)} != {tuple(want.shape)}"
        if robust:
            return grad_close(value, want, tol, label=what + key, floor=floor, flips=flips)
        err = rel_err(value, want, floor)
        REPORT.append((what + key, err, 0.0))
        assert err <= tol, f"{what}{key}: rel err {err:.3e} > {tol}"
        return err
    assert key + "#sum" in fix, f"{key} missing from fixture"
    head = torch.as_tensor(fix[key + "#head"])
    got_head = value.flatten()[: head.numel()]
    if robust:
        err = grad_close(got_head, head, tol, label=what + key + "#head", floor=floor, flips=flips)
    else:
        err = rel_err(got_head, head, floor)
        assert err <= tol, f"{what}{key}#head: rel err {err:.3e} > {tol}"
    if not digest:
        return err
    got, want = summarize(value), fix[key + "#sum"]
    # abs-sum and square-sum are well conditioned; the signed sums are checked against the abs-sum scale
    scale = np.array([want[1], want[1], want[1], want[3]]) + 1e-30
    derr = float(np.max(np.abs(got - want) / scale))
    dtol = tol
    assert derr <= dtol, f"{what}{key}#sum: digest err {derr:.3e} > {dtol}"
    REPORT.append((what + key + "#sum", derr, 0.0))
    return max(err, derr)
