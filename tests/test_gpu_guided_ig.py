"""GPU: brainxai.guided_ig and the bx_guided_ig_init / bx_guided_ig_step entry points against the restatement of the definition
(tests/guided_ig_ref.py, restatement (b)): the point x, the fp64 attribution, the pass counts and the status of every row bit for bit,
from the states the restatement itself reaches at the first, a middle and the last step; then the driver end to end.

End to end the path is chosen by the gradients, so the driver is checked in three parts that together pin it: (i) the restatement,
fed the call's own dumped gradients, reproduces the dumped path, the values and the pass counts bit for bit; (ii) every dumped gradient
is the fp64 oracle's gradient at the dumped point within TOL = 1e-3 of its maximum (the project's fp32 gradient bound, GG.worst) -- the
plain oracle for the EEG branch (ELU, average pooling: no decisions), the oracle whose ReLU / max-pool decisions are pinned to those of
the GPU forward of the same points (tests/golden_util.matched_oracle) for the spectrogram branch; (iii) delta is the fixed-order sum of
the values minus the drop of the outputs, recomputed in fp64 on the host.  Every end-to-end case is first checked ON THE REFERENCE SIDE
to discriminate: replayed from the same gradients with the fraction halved, with max_dist = 0 and with the selection inverted (the
largest |g| first), the values of every (sample, class) move by more than 100 x the tolerance of the comparison they guard -- a driver
that ignored the fraction, the window or the order of the selection cannot pass (i).  That comparison is (i), which is bit for bit on
fp32 values: it tolerates nothing, and the most two fp32 values of one (sample, class) can differ by without a bit of the computation
having changed is one rounding, u = 2^-24 of the largest; so the replay has to move by more than MOVED = 100 u of the largest value.
(The figures are printed.  With the same gradients the values depend on the path only through the change of the gradient along it,
which is small for these models over six steps: the least observed moves are 2.8e-5 of the maximum with the fraction halved, 8.9e-3 with
max_dist = 0 and 1.8e-2 with the selection inverted -- far above MOVED, far below the 100 x 1e-3 that (ii)'s tolerance would ask.)
No test provokes the pass cap or a fault; the cap is covered by the CPU restatement (tests/test_guided_ig_cpu.py)."""
import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import blur_ig_ref as BR
from tests import grad_gpu as GG
from tests import guided_ig_ref as R
from tests import perturb_gpu as PG
from tests.golden_util import matched_oracle
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3
MOVED = 100 * 2.0 ** -24

# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# row lengths: one cell; one below, at and above a wave; 5 x 333 (more than the workgroup's 1024 threads); 3 x 100 x 75 and 19 x 2000
LENGTHS = [1, 63, 64, 65, 1665, 22500, 38000]
SETS = ["quantised", "signs and zeros", "a third at the baseline", "odd baseline"]
KB = 3
K0 = 0.01                                            # k = floor(62 * 0.01) = 0 at P = 63


def _combos(P):
    """(fraction, max_dist, Kc, n): the full cross on the short rows, the corners on the long ones (the restatement runs on the host)."""
    if P <= 65:
        return [(f, m, Kc, 5) for f in (0.25, 1.0, K0) for m in (0.0, 0.02, 1.0) for Kc in (1, 3)] + [(0.25, 0.02, 3, 1), (K0, 0.0, 1, 1)]
    if P <= 1665:
        return [(f, m, Kc, 5) for f in (0.25, 1.0) for m in (0.0, 0.02, 1.0) for Kc in (1, 3)] + [(0.25, 0.02, 3, 1)]
    return [(0.25, 0.02, 3, 5), (1.0, 0.0, 1, 5), (0.25, 1.0, 1, 5), (0.25, 0.02, 1, 1)]


def _windows(Rn):
    """all rows; from inside sample 0 to inside the last sample; the last row alone"""
    return sorted({(0, Rn), (1, max(1, Rn - 2)), (Rn - 1, 1)})


def _inputs(P, kind):
    """(x_in fp32 [KB,P], baseline: a number or fp32 [KB,P])"""
    rng = np.random.default_rng(1000 + P + 7 * SETS.index(kind))
    x = rng.standard_normal((KB, P)).astype(np.float32)
    if kind == "odd baseline":
        return x, (0.3 + 0.1 * rng.standard_normal((KB, P))).astype(np.float32)
    if kind == "a third at the baseline":
        base = (0.2 * rng.standard_normal((KB, P))).astype(np.float32)
        x[:, ::3] = base[:, ::3]
        return x, base
    return x, 0.125


def _gradients(P, kind, Rn, i):
    rng = np.random.default_rng(5000 + 31 * P + 7 * SETS.index(kind) + i)
    if kind == "quantised":                            # four magnitudes: theta falls inside a large tie
        return (rng.choice([0.5, 1.0, 2.0, 4.0], size=(Rn, P)) * rng.choice([-1.0, 1.0], size=(Rn, P))).astype(np.float32)
    g = rng.standard_normal((Rn, P)).astype(np.float32)
    if kind == "signs and zeros":
        g[:, ::5] = 0.0
        g[:, 2::7] = -0.0
    return g


def _state_dev(st, iters):
    return {k: PG.dev(st[k].copy()) for k in ("x", "attr", "L_total", "status")} | {"iters": PG.dev(iters.copy())}


def _same(got, want, what):
    for key in ("x", "attr", "L_total", "status", "iters"):
        g = got[key].cpu().numpy()
        assert np.array_equal(PG.np_bits(g), PG.np_bits(want[key])), f"{what}: {key} differs from the restatement in {int((PG.np_bits(g) != PG.np_bits(want[key])).sum())} places"


def _launch_step(xin_d, base_d, sd, g_d, B, Kc, P, i, n, k, max_dist, cap, row0, rows):
    L.check(L.load().bx_guided_ig_step(PG.p(xin_d), PG.p(base_d), PG.p(sd["x"]), PG.p(g_d), PG.p(sd["attr"]), PG.p(sd["L_total"]), PG.p(sd["status"]),
                                       PG.p(sd["iters"]), B, Kc, P, i, n, k, max_dist, cap, row0, rows, PG.stream()), "bx_guided_ig_step")


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("P", LENGTHS)
def test_init_and_step_bit_for_bit(P, kind):
    x_in, base = _inputs(P, kind)
    base_rows = np.broadcast_to(np.asarray(base, dtype=np.float32), x_in.shape).copy()
    xin_d, base_d = PG.dev(x_in), PG.dev(base_rows)
    worst = 0
    for fraction, max_dist, Kc, n in _combos(P):
        what = f"P = {P}, {kind}, fraction {fraction}, max_dist {max_dist}, Kc {Kc}, n {n}"
        Rn, k = KB * Kc, R.rank_k(P, fraction)
        cap = R.pass_cap(P, k)
        st = R.init(x_in, base, Kc)
        # init: the baseline as one number where it is one, as rows otherwise
        got = {"x": torch.full((Rn, P), float("nan"), device=DEV), "attr": torch.full((Rn, P), float("nan"), dtype=torch.float64, device=DEV),
               "L_total": torch.full((Rn,), float("nan"), dtype=torch.float64, device=DEV), "status": torch.full((Rn,), 7, dtype=torch.int32, device=DEV)}
        one = PG.dev(np.asarray([base], dtype=np.float32)) if np.ndim(base) == 0 else None
        L.check(L.load().bx_guided_ig_init(PG.p(xin_d), PG.p(base_d if one is None else one), int(one is None), PG.p(got["x"]), PG.p(got["attr"]),
                                           PG.p(got["L_total"]), PG.p(got["status"]), KB, Kc, P, PG.stream()), "bx_guided_ig_init")
        iters = np.zeros((Rn, n), dtype=np.int32)
        _same(got | {"iters": PG.dev(iters)}, st | {"iters": iters}, what + ", init")
        for i in range(n):
            g = _gradients(P, kind, Rn, i)
            if i in (0, n // 2, n - 1):                 # from the state the restatement has reached
                for row0, rows in _windows(Rn):
                    sd = _state_dev(st, iters)
                    _launch_step(xin_d, base_d, sd, PG.dev(g[row0:row0 + rows]), KB, Kc, P, i, n, k, max_dist, cap, row0, rows)
                    want = {key: st[key].copy() for key in ("x", "attr", "L_total", "status")} | {"x_in": st["x_in"], "x_base": st["x_base"], "Kc": Kc}
                    want_iters = iters.copy()
                    R.step(want, g[row0:row0 + rows], i, n, k, max_dist, cap, row0=row0, iters=want_iters)
                    _same(sd, want | {"iters": want_iters}, f"{what}, step {i}, rows {row0}..{row0 + rows}")
            R.step(st, g, i, n, k, max_dist, cap, iters=iters)
        assert not st["status"].any() and (iters <= cap - 1).all(), f"{what}: the restatement itself left the bounds of a step"
        worst = max(worst, int(iters.max()))
    print(f"guided_ig step P = {P}, {kind}: {len(_combos(P))} parameter sets, most passes in a step {worst}")


def test_a_nan_gradient_stops_its_row_alone():
    P, Kc, n, fraction, max_dist = 1665, 1, 3, 0.25, 0.02
    x_in, base = _inputs(P, "odd baseline")
    k = R.rank_k(P, fraction)
    cap = R.pass_cap(P, k)
    st = R.init(x_in, base, Kc)
    iters = np.zeros((KB, n), dtype=np.int32)
    xin_d, base_d = PG.dev(x_in), PG.dev(base)
    sd = _state_dev(st, iters)
    for i in range(n):
        g = _gradients(P, "odd baseline", KB, i)
        if i == 1:
            g[1, 777] = np.nan
        before = st["x"][1].copy(), st["attr"][1].copy()
        R.step(st, g, i, n, k, max_dist, cap, iters=iters)
        _launch_step(xin_d, base_d, sd, PG.dev(g), KB, Kc, P, i, n, k, max_dist, cap, 0, KB)
        _same(sd, st | {"iters": iters}, f"step {i}")
        if i >= 1:                                      # stopped before anything of the step was written, and left alone afterwards
            assert np.array_equal(st["x"][1], before[0]) and np.array_equal(st["attr"][1], before[1]) and iters[1, i] == 0
    assert sd["status"].cpu().tolist() == [L.BX_GUIDED_OK, L.BX_GUIDED_NAN, L.BX_GUIDED_OK]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
EN = 6
MAX_DIST = 0.02
SETTINGS = [(0.25, "zero"), (0.1, "blur"), (0.25, "blur"), (0.1, "zero")]


def _baseline(x, input, which):
    return 0.0 if which == "zero" else brainxai.gaussian_blur(x.to(DEV), 6.0 if input == "eeg" else 3.0, axes="w" if input == "eeg" else "hw")


def _check_call(what, res, x, base, classes, fraction, grad_at):
    """res: GuidedIGResult of class_idx = classes ('all', or one class per sample) with keep_path; grad_at(points [R*n,...], cls [R*n]) is
    the fp64 oracle's gradient of each point's class."""
    B, per = x.shape[0], x[0].numel()
    every = isinstance(classes, str)
    Kc = res.out.shape[1] if every else 1
    Rn = B * Kc
    flat = (lambda t: t.reshape(Rn, *t.shape[(2 if every else 1):]))
    grads, path, values, iters = (flat(t).cpu() for t in (res.gradients, res.path, res.values, res.iterations))
    assert grads.shape == path.shape == (Rn, EN, *x.shape[1:]) and values.shape == (Rn, *x.shape[1:]) and iters.shape == (Rn, EN) and iters.dtype == torch.int32
    xin = x.reshape(B, per).numpy()
    bs = np.zeros((B, per), dtype=np.float32) if not isinstance(base, torch.Tensor) else base.cpu().reshape(B, per).numpy()
    g_np = grads.reshape(Rn, EN, per).numpy()
    # the reference side first: the same gradients, other parameters
    p_ref, v_ref, it_ref, st_ref = R.replay(xin, bs, Kc, g_np, fraction, MAX_DIST)
    assert not st_ref.any()
    want = torch.from_numpy(v_ref).reshape(Rn, 1, per)
    moved = {"fraction halved": R.replay(xin, bs, Kc, g_np, fraction / 2, MAX_DIST)[1], "max_dist = 0": R.replay(xin, bs, Kc, g_np, fraction, 0.0)[1],
             "largest |g| first": R.replay(xin, bs, Kc, g_np, fraction, MAX_DIST, largest_first=True)[1]}
    least = {how: float((GG.per_pair_max(torch.from_numpy(alt).reshape(Rn, 1, per) - want) / GG.per_pair_max(want)).min()) for how, alt in moved.items()}
    print(f"{what}: the replay moves by (least over (sample, class), of its maximum) " + ", ".join(f"{how} {v:.3e}" for how, v in least.items()))
    for how, v in least.items():
        assert v > MOVED, f"{what}: {how} moves the replayed values by only {v:.3e}"
    # (i) the call's own gradients reproduce its path, values and pass counts
    assert np.array_equal(PG.np_bits(path.reshape(Rn, EN, per).numpy()), PG.np_bits(p_ref)), f"{what}: the path is not the restatement's"
    assert np.array_equal(PG.np_bits(values.reshape(Rn, per).numpy()), PG.np_bits(v_ref)), f"{what}: the values are not the restatement's"
    assert np.array_equal(iters.numpy(), it_ref), f"{what}: the pass counts are not the restatement's"
    print(f"{what}: passes per step, worst {int(it_ref.max())}, mean {float(it_ref.mean()):.2f}")
    # (ii) the dumped gradients are the oracle's at the dumped points
    cls = (torch.arange(Kc).repeat(B) if every else torch.as_tensor(classes)).repeat_interleave(EN)
    want_g = grad_at(path.reshape(Rn * EN, *x.shape[1:]), cls).reshape(Rn, EN, per)
    err = GG.worst(grads.reshape(Rn, EN, per), want_g)
    print(f"{what}: gradients {err:.3e} of the per-(row, step) maximum")
    assert err <= TOL, f"{what}: gradients {err:.3e}"
    # (iii) delta
    out, end = res.out.double().cpu(), res.endpoint.double().cpu()
    drop = out - end if every else (out - end).gather(1, res.classes.cpu()[:, None])
    own = torch.from_numpy(BR.sum_rows(values.reshape(Rn, per).numpy())).reshape(drop.shape) - drop
    assert torch.equal(res.delta.cpu().reshape(own.shape), own), f"{what}: delta is not the fixed-order sum of the values minus the drop of the outputs"
    print(f"{what}: delta {res.delta.cpu().flatten().tolist()}")


def _grad_rows(forward):
    def grad_at(points, cls):
        xi = points.double().clone().requires_grad_(True)
        y = forward(xi)
        (g,) = torch.autograd.grad(y.gather(1, cls[:, None]).sum(), xi)
        return g
    return grad_at


@pytest.mark.parametrize("fraction,which", SETTINGS)
@pytest.mark.parametrize("kind", ["eegnet", "multimodal", "deep"])
def test_eeg_input_end_to_end(kind, fraction, which):
    _, mine, f64, x, other = GG.eeg_models(kind)
    classes = [4, 1]
    base = _baseline(x, "eeg", which)
    res = brainxai.guided_ig(mine, x.to(DEV), None if other is None else other.to(DEV), input="eeg", steps=EN, fraction=fraction, max_dist=MAX_DIST, baseline=base,
                             class_idx=classes, keep_path=True, return_parts=True)
    assert res.values.shape == (2, 1, 19, 2000) and res.map.shape == (2, 19, 2000) and res.classes.tolist() == classes and res.delta.dtype == torch.float64
    assert (res.steps, res.fraction, res.max_dist) == (EN, fraction, MAX_DIST) and torch.equal(res.map, res.values[:, 0])
    forward = f64 if other is None else BR.two_input(f64, other, "eeg", EN)
    _check_call(f"guided_ig eeg input, {kind}, fraction {fraction}, {which} baseline", res, x, base, classes, fraction, _grad_rows(forward))
    one = f64 if other is None else BR.two_input(f64, other, "eeg")
    lmax = float(BR.outputs(one, x).abs().max())
    b_rows = torch.zeros_like(x) if which == "zero" else base.cpu()
    assert float((res.out.double().cpu() - BR.outputs(one, x)).abs().max()) <= TOL * lmax and float((res.endpoint.double().cpu() - BR.outputs(one, b_rows)).abs().max()) <= TOL * lmax


@pytest.mark.parametrize("fraction,which", SETTINGS)
@pytest.mark.parametrize("kind", ["spectrogram", "multimodal"])
def test_spec_input_end_to_end(kind, fraction, which):
    ref, mine = PG.scaled_multimodal()
    eeg, spec = GG.mm_inputs()
    classes = "all" if kind == "spectrogram" else [4, 1]
    if kind == "spectrogram":
        ref, mine, eeg = ref.spectrogram_model, mine.spectrogram_model, None
    base = _baseline(spec, "spec", which)
    res = brainxai.guided_ig(mine, None if eeg is None else eeg.to(DEV), spec.to(DEV), input="spec", steps=EN, fraction=fraction, max_dist=MAX_DIST, baseline=base,
                             class_idx=classes, keep_path=True, return_parts=True)
    Kc = 6 if classes == "all" else 1
    assert res.values.shape[-3:] == (4, 32, 64) and res.map.shape == ((2, 6, 32, 64) if Kc == 6 else (2, 32, 64))
    v64 = res.values.double()                                           # the map rounds the fp64 channel sum once, the values each once
    assert bool(((res.map.double() - v64.sum(-3)).abs() <= 2.0 ** -24 * (v64.abs().sum(-3) + res.map.double().abs()) + 1e-45).all()), "the map is the channel sum"
    what = f"guided_ig spec input, {kind}, fraction {fraction}, {which} baseline"
    # the decisions of the GPU forward of the dumped points: one pass through the spectrogram branch
    flat = res.path.reshape(2 * Kc * EN, *spec.shape[1:]).cpu()
    keep = ops.keep_block_activations(mine)
    try:
        with X._eval_frozen(mine):
            (mine.spectrogram_model if eeg is not None else mine)(flat.to(DEV).requires_grad_(True))
        torch.cuda.synchronize()
    finally:
        ops.keep_block_activations(mine, on=False)
    args = (flat,) if eeg is None else (eeg.repeat_interleave(Kc * EN, dim=0), flat)
    twin, flips = matched_oracle(O, ref, args, keep, what)
    print(f"{what}: {len(flips)} decision flips")
    _check_call(what, res, spec, base, classes, fraction, _grad_rows((lambda xi: twin(xi)) if eeg is None else (lambda xi: twin(args[0].double(), xi))))


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_class_forms_and_max_batch():
    mine, eeg, spec = GG.iface()
    for input, shape in (("eeg", (19, 2000)), ("spec", (32, 64))):
        kw = dict(input=input, steps=4, fraction=0.25, max_dist=MAX_DIST)
        every = brainxai.guided_ig(mine, eeg, spec, class_idx="all", return_parts=True, keep_path=True, **kw)
        assert every.map.shape == (2, 6, *shape) and every.out.shape == every.endpoint.shape == (2, 6) and every.delta.shape == (2, 6) and every.classes is None
        assert every.iterations.shape == (2, 6, 4) and every.path.shape == every.gradients.shape == (2, 6, 4, *every.values.shape[2:])
        top = brainxai.guided_ig(mine, eeg, spec, return_parts=True, **kw)
        assert top.map.shape == (2, *shape) and top.values.dim() == 4 and top.delta.shape == (2,) and top.iterations.shape == (2, 4) and top.path is None and top.gradients is None
        assert torch.equal(top.classes, every.out.argmax(1)) and torch.equal(top.out, every.out) and torch.equal(top.endpoint, every.endpoint)
        for b in range(2):
            assert torch.equal(top.map[b], every.map[b, int(top.classes[b])]) and torch.equal(top.delta[b], every.delta[b, int(top.classes[b])])
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.guided_ig(mine, eeg, spec, class_idx=form, return_parts=True, **kw)
            assert per.classes.tolist() == [4, 1]
            assert torch.equal(per.map[0], every.map[0, 4]) and torch.equal(per.map[1], every.map[1, 1])
        assert torch.equal(brainxai.guided_ig(mine, eeg, spec, class_idx=2, **kw), every.map[:, 2])
        for mb in (1, 3, 256):                       # 12 rows in passes of 1, of 3 (a pass ends inside a sample) and in one
            small = brainxai.guided_ig(mine, eeg, spec, class_idx="all", max_batch=mb, return_parts=True, **kw)
            assert torch.equal(small.values, every.values) and torch.equal(small.iterations, every.iterations) and torch.equal(small.delta, every.delta), \
                f"guided_ig {input}: max_batch {mb} changes bits"


def test_downstream_and_restored_state():
    mine, eeg, spec = GG.iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        res = brainxai.guided_ig(mine, eeg, spec, input="spec", steps=4, return_parts=True)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    for input in ("spec", "eeg"):
        amap = res.map if input == "spec" else brainxai.guided_ig(mine, eeg, spec, input="eeg", steps=4)
        ranks = brainxai.attribution_ranks(amap)
        assert ranks.shape == (2, amap[0].numel())
        curves = brainxai.deletion_insertion(mine, eeg, spec, amap, input=input, steps=4)
        assert torch.equal(curves.ranks, ranks) and bool(torch.isfinite(curves.deletion).all()) and bool(torch.isfinite(curves.insertion).all())
    sm = mine.spectrogram_model
    alone = brainxai.guided_ig(sm, None, spec, steps=3, baseline=torch.full((4,), 0.5), class_idx="all", return_parts=True)
    assert alone.values.shape == (2, 6, 4, 32, 64) and float(alone.values.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(alone.out, sm(spec).float())
