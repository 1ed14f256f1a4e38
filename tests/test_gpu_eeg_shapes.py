"""The EEGNet front end (csrc/eeg.hip, eeg_mfma.hip, eeg_collapse.hip, eeg_generic.hip) off the model's own geometry: row lengths that
are no multiple of 4 or 8, temporal kernels other than 64 taps, one electrode up to one past the tuned range, batch sizes on both
sides of the launch-shape thresholds, the bounds of the collapsed training route and rows longer than the tuned backward holds.
The cases, the references and the tolerances are tests/eeg_ref.py (checked without a GPU by tests/test_eeg_ref_cpu.py).

Through the public model, per case and storage type, every route:
  all/eval, all/train        fp32 storage, input gradient and parameter gradients wanted (the layer-by-layer kernels)
  dx/collapsed, dx/collapsed-dx, dx/layered
                             evaluation mode, parameters frozen, only dL/dx wanted (as test_eeg_input_gradient_of_an_attribution_pass)
  train/mfma, train/valu     bf16 storage, training, no input gradient, ops.EEG_COLLAPSE off, with and without BX_EEG_NO_MFMA
  train/collapse             bf16 storage, training, no input gradient, ops.EEG_COLLAPSE on: the collapsed front end where
                             eeg_collapsed() admits the case, else whatever the refusal falls back to -- held to the same bound
A route whose kernel the descriptor rules exclude (the matrix-core kernels and the collapsed forms at kernLength != 64, the collapsed
training route at T % 8 != 0 or outside 96 <= T <= 3072, the tuned kernels at Chans > 64 or T > 15000) still runs and its fallback's
values are held to the same bound.  Compared: log-probabilities, dL/dx, every parameter gradient, the BatchNorms' running statistics
after a training pass and -- where the saved arena has the tuned layout (eeg_ref.Case.maps) -- the depthwise and separable maps
elementwise, read out of the arena with ops.eeg_features_keep and bx_eeg_saved_layout, and the pooled features.

Worst observed on an MI355X (each (case, route, quantity) is printed as a [parity] line; DESIGN.md section 2, "EEGNet front end off the
model's shapes", has the case table):
  fp32 storage, error / tolerance:  all/train 0.091 (batchnorm1.bias at B = 255), all/eval 0.043, dx/* <= 0.004
  bf16 storage, error / max(E_q, 2^-9), allowed 4:  train/mfma 1.010, train/collapse 1.010 (its fallback at T % 8 != 0), train/valu 1.014,
      dx/layered 1.005, dx/collapsed-dx 1.005, dx/collapsed 0.94 (its fallback at kernLength != 64) -- the kernels round the values the
      twin rounds; where a collapsed form itself runs the maps are within 5.8e-7 (held to the fp32 tolerance), and the vanishing
      gradients of the collapsed training route are 6.2e-4 of the largest gradient entry (bound 4 * 2^-9 = 7.8e-3 of it).
Rows of 4100 (fp32) and 5100 (bf16) samples: before the route became a function of the descriptor (eeg_tuned(), csrc/eeg_internal.h)
the forward was accepted and the backward raised "T too long" / "T/P1 too long for the LDS tile"; they now run on the general kernels
whenever a backward can follow.
"""
import contextlib
import ctypes
import os

import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import ops
from tests import eeg_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}                 # (storage, route) -> (ratio, case, quantity)


@contextlib.contextmanager
def _switches(collapse=None, no_mfma=False, layered=False):
    keep = ops.EEG_COLLAPSE
    try:
        if collapse is not None:
            ops.EEG_COLLAPSE = collapse
        if no_mfma:
            os.environ["BX_EEG_NO_MFMA"] = "1"
        if layered:
            os.environ["BX_EEG_DX_LAYERED"] = "1"
        yield
    finally:
        os.environ.pop("BX_EEG_NO_MFMA", None)
        os.environ.pop("BX_EEG_DX_LAYERED", None)
        ops.EEG_COLLAPSE = keep
        ops.clear_grad_views()


def _model(case, storage):
    cls = brainxai.EEGNet if case.arch == "EEGNet" else brainxai.EEGNetAttentionDeep
    net = cls(R.NB, dropoutRate=0.0, **R.model_kwargs(case)).to(DEV)
    return brainxai.set_compute_dtype(net, torch.bfloat16 if storage == "bf16" else torch.float32)


def _maps(net, case, mode, xd):
    """The depthwise and separable outputs and the pooled features of a forward without autograd under the switches in force, out of
    its saved arena; {} where the arena has no tuned layout -- which must be exactly where the case table says so."""
    g = net._geom
    with torch.no_grad():
        feat, saved, desc, _, _ = ops.eeg_features_keep(net, xd)
    torch.cuda.synchronize()
    off_d, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = L.load().bx_eeg_saved_layout(ctypes.byref(desc), ctypes.byref(off_d), ctypes.byref(off_s))
    B, T = case.batch, case.samples
    T1 = T // g.P1
    out = {"pool2": feat.reshape(B, g.F2, 1, T1 // g.P2).double().cpu()}
    assert (rc == 0) == (mode in case.maps), f"bx_eeg_saved_layout returned {rc} in {mode} mode, the case table expects maps in {case.maps}"
    if rc == 0:
        FD = g.F1 * g.D
        out["dw"] = saved[off_d.value:off_d.value + B * FD * T * 4].view(torch.float32).reshape(B, FD, 1, T).double().cpu()
        out["sep"] = saved[off_s.value:off_s.value + B * g.F2 * T1 * 4].view(torch.float32).reshape(B, g.F2, 1, T1).double().cpu()
    return out


def _run(net, case, ref, mode, want_dx, want_params):
    """One forward / backward of the model under test from the reference's initial state; the result in eeg_ref's format."""
    r = R.inputs(case)[1].to(DEV)
    xd = ref["x"].to(DEV)
    net.load_state_dict(ref["state"])
    net.train(mode == "train")
    for p in net.parameters():
        p.requires_grad_(want_params)
        p.grad = None
    xm = xd.clone().requires_grad_(want_dx)
    out = net(xm)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().double().cpu(), "dx": xm.grad.double().cpu() if want_dx else None, "grads": {}, "running": {}}
    if want_params:
        res["grads"] = {n: p.grad.double().cpu() for n, p in net.named_parameters()}
    if mode == "train":
        res["running"] = {k: v.double().cpu() for k, v in net.state_dict().items() if "running_" in k}
        res["nbt"] = {k: int(v) for k, v in net.state_dict().items() if k.endswith("num_batches_tracked")}
    net.load_state_dict(ref["state"])
    res.update(_maps(net, case, mode, xd))
    return res


def _collapsed_training_admits(case):
    """eeg_collapsed() of csrc/eeg.hip for a bf16 training pass without an input gradient"""
    return (case.kern == 64 and case.chans <= 64 and 96 <= case.samples <= 3072 and case.samples % 8 == 0)


def _excluded(case, route):
    """Why the descriptor rules keep the kernel a route is named after from running at this case (its fallback's values are still held
    to the route's bound), or None."""
    if case.chans > 64 or case.samples > 4096:
        # (every route here announces a backward: rows past the tuned backward's 4096 take the general kernels, as Chans > 64 does)
        return "general kernels (Chans > 64 or a row the tuned backward cannot hold)"
    if route in ("train/mfma", "dx/collapsed", "dx/collapsed-dx") and case.kern != 64:
        return "kernLength != 64: the matrix-core kernels and the collapsed forms need 64 taps"
    if route == "train/collapse" and not _collapsed_training_admits(case):
        return ("kernLength != 64" if case.kern != 64 else "T % 8 != 0" if case.samples % 8 else "T < 96" if case.samples < 96 else "T > 3072") + \
               ": eeg_collapsed() refuses, the layer-by-layer kernels run"
    return None


def _routes(storage):
    eval_dx = [("dx/collapsed", "eval", dict(collapse=True), True, False), ("dx/collapsed-dx", "eval", dict(collapse=False), True, False),
               ("dx/layered", "eval", dict(collapse=False, layered=True), True, False)]
    if storage == "fp32":
        return [("all/eval", "eval", {}, True, True), ("all/train", "train", {}, True, True)] + eval_dx
    return eval_dx + [("train/mfma", "train", dict(collapse=False), False, True), ("train/valu", "train", dict(collapse=False, no_mfma=True), False, True),
                      ("train/collapse", "train", dict(collapse=True), False, True)]


@pytest.mark.parametrize("tag,storage", [(c.tag, s) for c in R.CASES for s in c.storages])
def test_eeg_front_end_off_the_models_shapes(tag, storage):
    case = R.BY_TAG[tag]
    net = _model(case, storage)
    failures = []
    for route, mode, sw, want_dx, want_params in _routes(storage):
        zero = R.zero_grads(case, mode)
        ref = R.reference(tag, mode, "exact" if storage == "fp32" else "rounded")
        if _excluded(case, route):
            print(f"[parity] eeg-shapes {tag} {storage} {route}: not the route's own kernel -- {_excluded(case, route)}; its fallback is held to the same bound")
        try:
            with _switches(**sw):
                got = _run(net, case, ref, mode, want_dx, want_params)
        except RuntimeError as e:
            failures.append(f"{route}: raised {e}")
            print(f"[parity] eeg-shapes {tag} {storage} {route}: RAISED {e}")
            continue
        if storage == "fp32":
            dev = R.deviations(got, ref, zero)
            lim = {n: R.fp32_limit(n, zero) for n in dev}
        else:
            dev = R.deviations(got, ref, zero, floored=False)
            collapsed = route == "train/collapse" and _collapsed_training_admits(case)
            lim = R.bf16_limits(R.reference(tag, mode, "twin"), ref, zero, rounded_operands=collapsed)
            if collapsed:
                for n in dev:
                    if n.startswith("batchnorm1.running_"):
                        lim[n] = R.COLLAPSED_BN1_TOL        # fp64 sums of the input's sufficient statistics
            if collapsed or (route == "dx/collapsed" and case.kern == 64 and case.chans <= 64):
                # The collapsed forms never store the conv1 output, so nothing of the forward (and, in evaluation mode, of the input
                # gradient) is rounded to bf16: fp32 arithmetic on bf16-representable operands, held to the fp32 tolerance.  This is also
                # what shows that the collapsed front end ran where eeg_collapsed() admits the case.
                for n in ("out", "pool2", "dw", "sep") + (("dx",) if mode == "eval" else ()):
                    if n in lim:
                        lim[n] = R.TIGHT
        for n in sorted(dev):
            ratio = dev[n] / lim[n]
            print(f"[parity] eeg-shapes {tag} {storage} {route} {n}: {dev[n]:.2e} (bound {lim[n]:.2e}, ratio {ratio:.2f})")
            if not dev[n] <= lim[n]:
                failures.append(f"{route} {n}: {dev[n]:.3e} > {lim[n]:.3e}")
            if ratio == ratio and ratio > WORST.get((storage, route), (0.0,))[0]:
                WORST[(storage, route)] = (ratio, tag, n)
        for k, v in got.get("nbt", {}).items():
            if v != 1:
                failures.append(f"{route} {k} = {v} after one training pass")
        expected = {"out", "pool2"} | ({"dx"} if want_dx else set()) | ({"dw", "sep"} if mode in case.maps else set())
        missing = expected - set(dev)
        if want_params:
            missing |= {"grad." + n for n in ref["grads"]} - set(dev)
        if mode == "train":
            missing |= set(ref["running"]) - set(dev)
        if missing:
            failures.append(f"{route}: not compared: {sorted(missing)}")
    assert not failures, f"{tag} {storage}: " + "; ".join(failures)


def test_zz_eeg_shapes_report():
    """Not a check: the worst error / bound per storage type and route of the cases above (kept in the GPU log)."""
    print("\n[parity] eeg-shapes worst error / bound per route (storage, route, ratio, case, quantity):")
    for (storage, route), (ratio, tag, n) in sorted(WORST.items()):
        print(f"[parity]   {storage:5s} {route:16s} {ratio:6.3f}  {tag}  {n}")
