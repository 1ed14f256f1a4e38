"""References, wrong references and the case table of the EEGNet front end's shape tests (tests/test_eeg_ref_cpu.py runs them on the
CPU, tests/test_gpu_eeg_shapes.py holds the HIP kernels to them).  Everything here is the oracle (oracle/ref_torch.py) in fp64.

  exact()         the oracle network in fp64: stage maps, log-probabilities, input gradient, every parameter gradient, running statistics
  oracle32()      the same in fp32 -- what the project's fp32 tolerance has to leave room for
  rounded_twin()  fp64 with x and conv1.weight rounded to bf16 and the conv1 output stored as bf16 (value and gradient): the
                  yardstick of bf16 storage noise, not a target
  mutants()       deliberately wrong references; a tolerance that cannot tell them from exact() cannot tell a wrong kernel either

Tolerances.  fp32 storage: the project's TIGHT = 2e-4 of a quantity's largest entry; parameter gradients on the floor 1e-2 x the largest
gradient entry of the model; gradients that vanish in theory (zero_* / eps_* of a case) at TOL = 1e-3 on that floor.  bf16 storage:
E_q = max|q(rounded_twin) - q(exact)| / max|q(exact)| on bf16-representable x and conv1.weight, and the kernel must stay within
BF16_FACTOR * max(E_q, 2^-9) of exact(): the twin rounds each stored value once, the weight-gradient kernels also round their two
operands (dL/du and x or c1), i.e. at most three roundings of relative size 2^-9 where the twin has one, plus fp32 accumulation --
hence 4; 2^-9 is bf16's half-ulp and keeps a lucky small realisation of the twin from setting the bar.  The vanishing gradients under
bf16 storage: see bf16_limits().
"""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import ref_torch as O

NB = 6
SEED = 131                       # parameters (O.fill_params), x = O.seeded(.., SEED + 1, "randn"), r = O.seeded(.., SEED + 2, "randn")
TIGHT, TOL = 2e-4, 1e-3          # tests/test_gpu_parity.py
BF16_FLOOR, BF16_FACTOR = 2.0 ** -9, 4.0
COLLAPSED_BN1_TOL = 2e-5         # BatchNorm1's running statistics of the collapsed training route (fp64 sums), as test_eegnet_collapsed_front_end
MUTANTS = ("last_step", "pad_shift", "last_electrode", "last_tap")
ELEMENTWISE = ("dw", "sep", "dx")

# Gradients that vanish in train mode (both sides then hold rounding noise, compared on the floor at TOL):
#   zero_*  exactly: batchnorm1.bias (BatchNorm2 removes any shift of its input rows); with one attention token the query and the key
#           (softmax over a single score is 1 whatever they are)
#   eps_*   up to BatchNorm's eps: a scale of BatchNorm2's input rows (batchnorm1.weight; depthwiseConv.weight at Chans = 1) or of
#           BatchNorm1's (conv1.weight at kernLength = 1) changes the normalised output only through var + eps, so the true gradient is
#           of relative size eps / var -- far below the floor, not below fp64 rounding
ZERO_TRAIN, EPS_TRAIN = ("batchnorm1.bias",), ("batchnorm1.weight",)
ONE_TOKEN = ("attention_layer.query.weight", "attention_layer.query.bias", "attention_layer.key.weight", "attention_layer.key.bias")
LAST_STEP_BF16 = {"last_step": "bf16 bound only: the last sample reaches 1/64 of the taps of the last 32 outputs and moves the maps by less "
                               "than 10 x 4 x E_q at this row length (it stays in the fp32 check)"}

# tag, arch, (Chans, Samples, batch, kernLength), storages run on the GPU, mutants dropped from the bf16 discrimination check (name ->
# reason), vanishing gradients per mode, modes in which the saved arena of a pass without autograd has the tuned layout
# (bx_eeg_saved_layout), what the case reaches
Case = namedtuple("Case", "tag arch chans samples batch kern storages drop zero_train eps_train zero_eval maps reaches")


def _case(chans, samples, batch, kern, reaches, arch="EEGNet", storages=("fp32", "bf16"), drop=None, zero_train=ZERO_TRAIN, eps_train=EPS_TRAIN,
          zero_eval=(), maps=("eval", "train"), tag=None):
    tag = tag or f"{'deep' if arch != 'EEGNet' else 'eeg'}{chans}x{samples}b{batch}k{kern}"
    return Case(tag, arch, chans, samples, batch, kern, tuple(storages), dict(drop or {}), tuple(zero_train), tuple(eps_train), tuple(zero_eval),
                tuple(maps), reaches)


CASES = [
    _case(3, 133, 2, 64, "T % 4 = 1: the scalar tails of k_eeg_conv1_bwd, k_eeg_conv1_mfma, k_eeg_conv1_wgrad_mfma, k_eegc_dx; T % 8 != 0 in "
                         "k_eeg_dw_bwd_a; T1 = 33 (T1 & 3 != 0 in k_eeg_sep_bwd); both pools drop a tail; collapsed training refuses T % 8", drop=LAST_STEP_BF16),
    _case(1, 34, 3, 64, "one electrode; a row shorter than the kernel (every output reads both zero halos); T % 4 = 2; T2 = 1",
          eps_train=EPS_TRAIN + ("depthwiseConv.weight",)),
    _case(64, 70, 2, 64, "Chans = EEG_MAXCH: sdw full, seven batches of ten (the last ragged), k_eeg_dw_bwd_a's widest grid"),
    _case(65, 64, 2, 64, "the default family one electrode past the tuned range: general kernels; T = K1", maps=()),
    _case(10, 1001, 2, 64, "exactly one batch of ten electrodes in k_eeg_dw; odd T"),
    _case(11, 250, 3, 64, "one electrode more than a batch of ten; a 250 Hz second"),
    _case(4, 96, 2, 64, "the collapsed training route's lower bound T = 96"),
    _case(4, 88, 2, 64, "the first multiple of 8 below the collapsed route's lower bound"),
    _case(2, 3072, 2, 64, "bx_eegc_corr_max_T(): the collapsed training route's upper bound"),
    _case(2, 3080, 2, 64, "the first multiple of 8 above bx_eegc_corr_max_T()"),
    _case(5, 131, 2, 1, "a single tap: K1 == 64 gates of the MFMA, collapsed and k_eegc_dx routes; padl1 = 0",
          eps_train=EPS_TRAIN + ("conv1.weight",)),
    _case(5, 131, 2, 8, "8 taps: even 'same' split 3 | 4, one tap octet in the weight gradient"),
    _case(5, 131, 2, 32, "32 taps: even 'same' split 15 | 16"),
    _case(5, 131, 2, 33, "33 taps: odd kernel, K1 not a multiple of 8 (kb < K1, kk < K1 in the weight gradient)"),
    _case(5, 131, 2, 63, "63 taps: odd kernel one short of the tuned maximum"),
    _case(2, 1030, 256, 64, "k_eeg_sep<4> at exactly 512 workgroups; k_eeg_sep_bwd with both halves in one workgroup (B * 4 >= 1024); fold3 at "
                            "exactly rows * 16 = 8192"),
    _case(2, 1030, 255, 64, "k_eeg_sep<2> at 510 workgroups; k_eeg_sep_bwd split over two workgroups; fold3 below 8192"),
    _case(2, 4100, 2, 64, "a row past k_eeg_conv1_bwd's 256 * EEG_DX_MAX = 4096", storages=("fp32",), maps=("eval",), drop=LAST_STEP_BF16),
    _case(2, 5100, 2, 64, "a row past k_eeg_sep_bwd's LDS tile (T/4 <= 1248)", storages=("bf16",), maps=("eval",), drop=LAST_STEP_BF16),
    _case(2, 15001, 2, 64, "a row past EEG_MAXT: general kernels in every mode", maps=(), drop=LAST_STEP_BF16),
    _case(5, 301, 2, 64, "the same front end under the deep head at T % 4 = 1 (T1 = 75, T2 = 9, one attention token)", arch="EEGNetAttentionDeep",
          zero_train=ZERO_TRAIN + ONE_TOKEN, zero_eval=ONE_TOKEN, drop=LAST_STEP_BF16),
]
BY_TAG = {c.tag: c for c in CASES}


def model_kwargs(case):
    return dict(Chans=case.chans, Samples=case.samples, kernLength=case.kern)


def inputs(case):
    """(x, r): the seeded input and the seeded weights on the log-probabilities (loss = sum(out * r))."""
    return (O.seeded((case.batch, 1, case.chans, case.samples), SEED + 1, "randn"), O.seeded((case.batch, NB), SEED + 2, "randn"))


def zero_grads(case, mode):
    """every gradient compared on the floor at TOL in this mode"""
    return case.zero_train + case.eps_train if mode == "train" else case.zero_eval


def kept_mutants(case, bound):
    """the mutants the ``bound`` ("fp32" | "bf16") has to tell apart at this case"""
    return tuple(m for m in MUTANTS if bound == "fp32" or m not in case.drop)


def bf16_round(t):
    return t.bfloat16().to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
def _run(arch, kw, x, r, mode, dtype=torch.float64, rounded=False, store=False, mutant=None, seed=SEED):
    cls = O.EEGNet if arch == "EEGNet" else O.EEGNetAttentionDeep
    net = O.fill_params(cls(NB, dropoutRate=0.0, **kw), seed=seed)
    x = x.clone().float()
    with torch.no_grad():
        if rounded:
            net.conv1.weight.copy_(bf16_round(net.conv1.weight))
            x = bf16_round(x)
        if mutant == "last_tap":
            net.conv1.weight[..., -1] = 0.0
        elif mutant == "last_electrode":
            net.depthwiseConv.weight[:, :, -1, :] = 0.0
        elif mutant == "last_step":
            x[..., -1] = 0.0
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dtype)
    net.train(mode == "train")
    if mutant == "pad_shift":                      # 'same' padding moved by one sample: left (K-1)//2 + 1, right K - 1 - (K-1)//2 - 1
        k = kw["kernLength"]
        pl = (k - 1) // 2
        conv1 = net.conv1
        conv1.forward = lambda inp: F.conv2d(F.pad(inp, (pl + 1, k - 1 - pl - 1)), conv1.weight)
    keep = {}
    hooks = [net.depthwiseConv.register_forward_hook(lambda m, i, o: keep.__setitem__("dw", o)),
             net.separableConv.register_forward_hook(lambda m, i, o: keep.__setitem__("sep", o))]
    if store:
        hooks.append(net.conv1.register_forward_hook(lambda m, i, o: O._StoreAs.apply(o, torch.bfloat16)))
    xr = x.to(dtype).requires_grad_(True)
    st = net.stages(xr)
    (st["out"] * r.to(dtype)).sum().backward()
    for h in hooks:
        h.remove()
    res = {"dw": keep["dw"], "sep": keep["sep"], "pool2": st["pool2"], "out": st["out"], "dx": xr.grad}
    res = {k: v.detach().double() for k, v in res.items()}
    res["grads"] = {n: p.grad.detach().double() for n, p in net.named_parameters()}
    res["running"] = {k: v.detach().double().clone() for k, v in net.state_dict().items() if "running_" in k}
    res["state"] = state                            # fp32 parameters and buffers BEFORE the pass: what the model under test loads
    res["x"] = x                                    # the input as fed (rounded / mutated)
    return res


def exact(model_kwargs, x, r, mode, arch="EEGNet", rounded=False):
    """fp64 oracle.  ``rounded``: x and conv1.weight rounded to bf16 first (what the bf16 routes are fed), nothing else."""
    return _run(arch, model_kwargs, x, r, mode, rounded=rounded)


def oracle32(model_kwargs, x, r, mode, arch="EEGNet"):
    return _run(arch, model_kwargs, x, r, mode, dtype=torch.float32)


def rounded_twin(model_kwargs, x, r, mode, arch="EEGNet"):
    return _run(arch, model_kwargs, x, r, mode, rounded=True, store=True)


def mutants(model_kwargs, x, r, mode, arch="EEGNet", names=MUTANTS):
    return {m: _run(arch, model_kwargs, x, r, mode, mutant=m) for m in names}


@lru_cache(maxsize=16)
def reference(tag, mode, kind="exact"):
    """Shared by the tests of a case, computed once and never modified: kind in exact | rounded | twin | oracle32 | a mutant's name."""
    c = BY_TAG[tag]
    x, r = inputs(c)
    kw = model_kwargs(c)
    if kind == "exact":
        return exact(kw, x, r, mode, c.arch)
    if kind == "rounded":
        return exact(kw, x, r, mode, c.arch, rounded=True)
    if kind == "twin":
        return rounded_twin(kw, x, r, mode, c.arch)
    if kind == "oracle32":
        return oracle32(kw, x, r, mode, c.arch)
    return mutants(kw, x, r, mode, c.arch, names=(kind,))[kind]


# ---------------------------------------------------------------------------------------------------------------------------------
def quantities(res):
    """name -> tensor of everything a result holds that is compared."""
    q = {k: res[k] for k in ("out", "dx", "dw", "sep", "pool2") if res.get(k) is not None}
    q.update({"grad." + n: g for n, g in res.get("grads", {}).items() if g is not None})
    q.update({k: v for k, v in res.get("running", {}).items()})
    return q


def grad_floor(ref):
    """the scale of 'a gradient that matters' (tests/test_gpu_parity.py _gscale): 1e-2 of the largest parameter-gradient entry"""
    return 1e-2 * max(float(g.abs().max()) for g in ref["grads"].values())


def deviations(got, ref, zero=(), floored=True):
    """name -> max|got - ref| / scale for every quantity ``got`` holds.  scale = the reference quantity's largest entry; parameter
    gradients on the floor grad_floor(ref) when ``floored`` (the fp32 rule), else only those named in ``zero`` (the bf16 rule)."""
    gq, rq = quantities(got), quantities(ref)
    fl = grad_floor(ref)
    out = {}
    for name, g in gq.items():
        w = rq[name]
        assert tuple(g.shape) == tuple(w.shape), (name, tuple(g.shape), tuple(w.shape))
        scale = float(w.abs().max())
        if name.startswith("grad.") and (floored or name[5:] in zero):
            scale = max(scale, fl)
        d = float((g.double() - w).abs().max())
        out[name] = d / max(scale, 1e-300) if d == d else float("nan")
    return out


def fp32_limit(name, zero=()):
    return TOL if name.startswith("grad.") and name[5:] in zero else TIGHT


def bf16_limits(twin, ref, zero=(), rounded_operands=False):
    """name -> BF16_FACTOR * max(E_q, 2^-9) relative to the quantity's largest entry.

    A vanishing gradient (``zero``) has no scale of its own; it is compared on the floor, as in the fp32 rule.  Its bound:
      * layer-by-layer kernels: such a gradient is an fp32 sum over the STORED values (the bf16 conv1 output is what the forward
        normalised, so the cancellation is that of fp32 arithmetic): the fp32 rule, TOL on the floor -- unless the twin itself shows
        storage noise there (conv1.weight at kernLength = 1: the gradient at conv1's output is stored too), then BF16_FACTOR * E_q;
      * ``rounded_operands`` (the collapsed training route, whose correlation kernel takes dL/du and x as bf16 operands): the terms
        that cancel are each rounded, which leaves up to 2^-9 of the TERMS' size, not of the sum's; the terms are those of the
        non-vanishing gradients of the same layer, whose scale is the largest gradient entry: BF16_FACTOR * 2^-9 of that entry, i.e.
        of 100 floors.  (The floor at that factor would ask for cancellation to 1/100 of one operand rounding.)"""
    fl, gmax = grad_floor(ref), grad_floor(ref) * 100.0
    out = {}
    for n, e in deviations(twin, ref, zero, floored=False).items():
        if n.startswith("grad.") and n[5:] in zero:
            out[n] = max(TOL, BF16_FACTOR * e)
            if rounded_operands:
                out[n] = max(out[n], BF16_FACTOR * BF16_FLOOR * gmax / fl)
        else:
            out[n] = BF16_FACTOR * max(e, BF16_FLOOR)
    return out
