"""GPU: brainxai.gradient_shap / channel_importance / GradientExplainer and the bx_expgrad_* / bx_mean_abs_rows entry points against the
restatement of the definition (tests/gradient_shap_ref.py): the interpolants bit for bit, the running sum, the mean and the map
against numpy fp64, and the attributions end to end against the oracle's classes run in fp64 on the CPU.

Bounds.  Kernels: |got - want| <= |want| 2^-23 + 2^-52 sum_k |d g| + 2^-149 per element (one fp32 rounding of an fp64 sum of exact
products).  End to end: 1e-3 of the per-(sample, class) maximum, the project's fp32 gradient bound (TOL of tests/test_gpu_parity.py).
Every end-to-end case is first checked ON THE REFERENCE SIDE to discriminate: the fp64 reference with the background indices shifted
by one differs by more than 100 x the bound for every (sample, class), with the interpolation points rolled by one draw by more than
50 x -- a row kernel that gathered the wrong background or ignored alpha cannot pass.  The EEG branch (ELU, average pooling: no
decisions) is compared with the plain fp64 oracle; the spectrogram branch with the fp64 oracle whose ReLU / max-pool decisions are
pinned to those of the GPU forward of the same rows (tests/golden_util.matched_oracle: every disagreement with the exact forward
must be a demonstrated tie; with none the twin is the plain oracle).
Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import grad_gpu as GG
from tests import gradient_shap_ref as R
from tests import perturb_gpu as PG
from tests.golden_util import matched_oracle
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# trailing shape of the input: a spectrogram [C,H,W] or an EEG input [1,Chans,T]; per = 768, 22500, 8192, 1665 (no multiple of four), 38000
SHAPES = {"spec 2x16x24": (2, 16, 24), "spec 3x100x75": (3, 100, 75), "spec 4x32x64": (4, 32, 64), "eeg 5x333": (1, 5, 333), "eeg 19x2000": (1, 19, 2000)}
KB, KNB, KN = 3, 3, 5
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
IDX = np.array([[0, 1, 2, 0, 1], [2, 2, 1, 0, 0], [1, 0, 2, 1, 2]], dtype=np.int32)          # every background, and repeats
ALPHA = np.array([[0.0, 0.25, BELOW_ONE, 0.7, 0.5], [0.3, 0.0, 0.9, BELOW_ONE, 0.125], [0.6, 0.1, 0.0, 0.45, BELOW_ONE]], dtype=np.float32)
WINDOWS = [(0, 15), (2, 10), (14, 1)]              # all rows; from inside sample 0 to inside sample 2; the last row alone


def _kernel_case(name):
    shape = SHAPES[name]
    seed = 100 + sorted(SHAPES).index(name)
    x, bg = O.seeded((KB, *shape), seed, "randn"), O.seeded((KNB, *shape), seed + 50, "randn")
    x.view(-1)[::7] = -0.0
    bg.view(-1)[3::11] = -0.0
    return shape, x, bg


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_bit_for_bit(name):
    shape, x, bg = _kernel_case(name)
    per = int(np.prod(shape))
    want = R.rows(x, bg, IDX, ALPHA)
    assert np.signbit(want).any() and not np.isnan(want).any()
    lib = L.load()
    xd, bd, idx_d, alpha_d = PG.dev(x), PG.dev(bg), PG.dev(IDX), PG.dev(ALPHA)
    for row0, rows in WINDOWS:
        out = torch.full((rows, *shape), float("nan"), dtype=torch.float32, device=DEV)
        L.check(lib.bx_expgrad_rows(PG.p(xd), PG.p(bd), PG.p(idx_d), PG.p(alpha_d), PG.p(out), KB, KNB, KN, per, row0, rows, PG.stream()), "bx_expgrad_rows")
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), f"{name} rows {row0}..{row0 + rows}: elements left unwritten"
        assert np.array_equal(got.view(np.int32), want[row0:row0 + rows].view(np.int32)), f"{name} rows {row0}..{row0 + rows}"
    print(f"rows {name}: per {per}, windows {WINDOWS} bit for bit")


def _bound_ratio(got, want, absum):
    bound = np.abs(want) * 2.0 ** -23 + 2.0 ** -52 * absum + 2.0 ** -149
    return float((np.abs(got.astype(np.float64) - want) / bound).max())


@pytest.mark.parametrize("Kc", [1, 3])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accumulate_and_finish_against_numpy(name, Kc):
    shape, x, bg = _kernel_case(name)
    per, rows_all = int(np.prod(shape)), KB * KN
    slot = Kc // 2
    g = O.seeded((rows_all, *shape), 7, "randn")
    lib = L.load()
    xd, bd, idx_d, gd = PG.dev(x), PG.dev(bg), PG.dev(IDX), PG.dev(g)
    SENTINEL = 7.25

    def run(splits, mis=False):
        acc = torch.full((KB, Kc, per), SENTINEL, dtype=torch.float64, device=DEV)
        acc[:, slot] = 0.0
        for row0, rows in splits:
            gs = gd[row0:row0 + rows].contiguous()
            L.check(lib.bx_expgrad_accumulate(PG.p(xd), PG.p(bd), PG.p(idx_d), PG.p(PG.misaligned(gs) if mis else gs), PG.p(acc), KB, KNB, KN, per, Kc, slot,
                                              row0, rows, PG.stream()), "bx_expgrad_accumulate")
        return acc
    one, two = run([(0, rows_all)]), run([(0, 7), (7, rows_all - 7)])                    # row 7 is inside sample 1
    assert torch.equal(one, two), f"{name}: two calls split inside a sample differ from one call"
    mis = run([(0, 7), (7, rows_all - 7)], mis=True)                                     # element by element, whatever per % 4
    assert torch.equal(one.view(torch.int64), mis.view(torch.int64)), f"{name}: a misaligned g changes the sum"
    others = [k for k in range(Kc) if k != slot]
    assert bool((one[:, others] == SENTINEL).all()), "the slots of other classes were touched"
    want_acc, absacc = R.accumulate(x, bg, IDX, g.numpy())
    exact = bool(np.array_equal(one[:, slot].cpu().numpy(), want_acc[:, 0]))
    spec = name.startswith("spec")
    Cc, HW = (shape[0], shape[1] * shape[2]) if spec else (1, per)
    acc = one.clone()
    acc[:, others] = 0.0
    values = torch.full((KB, Kc, *shape), float("nan"), dtype=torch.float32, device=DEV)
    amap = torch.full((KB, Kc, shape[1], shape[2]), float("nan"), dtype=torch.float32, device=DEV) if spec else None
    L.check(lib.bx_expgrad_finish(PG.p(acc), PG.p(values), PG.p(amap), KB * Kc, Cc, HW, KN, PG.stream()), "bx_expgrad_finish")
    values = values.cpu().numpy()
    assert not np.isnan(values).any()
    want = (want_acc[:, 0] / KN).reshape(KB, *shape)
    rv = _bound_ratio(values[:, slot], want, absacc.reshape(KB, *shape))
    assert rv <= 1.0, f"{name}: values {rv:.3f} x the bound"
    assert not values[:, others].any(), "an untouched slot (zero sum) must give zero values"
    rm = 0.0
    if spec:
        amap = amap.cpu().numpy()
        assert not np.isnan(amap).any()
        rm = _bound_ratio(amap[:, slot], want.sum(1), absacc.reshape(KB, *shape).sum(1))
        assert rm <= 1.0, f"{name}: map {rm:.3f} x the bound"
    print(f"accumulate {name} Kc={Kc}: split == one call bit for bit, fp64 sum equal to numpy's bit for bit: {exact}, values {rv:.3f} x bound, map {rm:.3f} x bound")


@pytest.mark.parametrize("Ln", [1, 333, 2000])
def test_mean_abs_rows_against_numpy(Ln):
    v = O.seeded((3, 7, Ln), 40 + Ln, "randn")                            # 21 rows: the last workgroup is not full
    v.view(-1)[::5] = -0.0
    got = brainxai.channel_importance(PG.dev(v))
    assert got.shape == (3, 7) and got.dtype == torch.float32
    want = R.channel_importance(v.numpy())
    bound = np.abs(want) * 2.0 ** -23 + Ln * 2.0 ** -52 * np.abs(v.numpy().astype(np.float64)).mean()
    ratio = float((np.abs(got.cpu().numpy().astype(np.float64) - want) / bound).max())
    print(f"mean_abs_rows L={Ln}: {ratio:.3f} x bound")
    assert ratio <= 1.0


def test_channel_importance_top_with_exact_ties():
    v = O.seeded((2, 8, 333), 9, "randn")
    v[:, 4], v[:, 6] = -v[:, 1], v[:, 1].abs()                            # the same |.| in the same order: exact ties of channels 1, 4, 6
    v[:, 0], v[:, 7] = 0.0, -0.0                                          # and a tie at zero
    imp, order = brainxai.channel_importance(PG.dev(v), top=8)
    imp_h, order_h = imp.cpu().numpy(), order.cpu().numpy()
    assert order.dtype == torch.int64 and order_h.shape == (2, 8)
    assert np.array_equal(imp_h[:, 1], imp_h[:, 4]) and np.array_equal(imp_h[:, 1], imp_h[:, 6]) and not imp_h[:, [0, 7]].any()
    want = np.argsort(-imp_h, axis=-1, kind="stable")
    assert np.array_equal(order_h, want) and np.array_equal(order_h[:, -2:], [[0, 7], [0, 7]])
    for b in range(2):
        pos = {int(c): i for i, c in enumerate(order_h[b])}
        assert pos[1] + 1 == pos[4] and pos[4] + 1 == pos[6], "ties by the lower index"
    imp3, top3 = brainxai.channel_importance(PG.dev(v), top=3)
    assert torch.equal(imp3, imp) and np.array_equal(top3.cpu().numpy(), want[:, :3])
    assert np.array_equal(R.channel_importance(v.numpy(), top=8)[1], want)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _guard(what, f64, want, x, bg, idx, alpha, other, input):
    """Reference side alone: the inputs discriminate the background gather and the interpolation points."""
    Nb = bg.shape[0]
    scale = GG.per_pair_max(want)
    shifted = GG.per_pair_max(R.values(f64, x, bg, (idx + 1) % Nb, alpha, other, input) - want) / scale
    rolled = GG.per_pair_max(R.values(f64, x, bg, idx, np.roll(alpha, 1, axis=1), other, input) - want) / scale
    print(f"{what}: reference with idx shifted {float(shifted.min()):.3f}, with alpha rolled {float(rolled.min()):.3f} of the per-(sample, class) maximum (least)")
    assert float(shifted.min()) > 100 * TOL, f"{what}: shifting the background indices moves the reference by only {float(shifted.min()):.3e}"
    assert float(rolled.min()) > 50 * TOL, f"{what}: rolling alpha moves the reference by only {float(rolled.min()):.3e}"


@functools.lru_cache(maxsize=None)
def _eeg_case(kind):
    """(ref, mine, x, bg, other, n, seed, max_batch, idx, alpha, want fp64 [B,K,1,Chans,T]); computed once, never written to."""
    ref, mine, f64, x, other = GG.eeg_models(kind)
    if kind == "eegnet":
        bg, n, seed, max_batch = O.seeded((5, 1, 19, 2000), 92, "randn"), 12, 3, 8
    else:
        bg, n, seed, max_batch = O.seeded((3, 1, 19, 2000), 14, "randn"), 6, 3, 256
    idx, alpha = R.draws(seed, x.shape[0], bg.shape[0], n)
    want = R.values(f64, x, bg, idx, alpha, other, "eeg")
    if kind == "eegnet":                                                  # the oracle's own estimator, run in fp64, is the target there
        oracle = O.expected_gradients(f64, x.double(), bg.double(), nsamples=n, seed=seed).double()
        assert GG.worst(want, oracle) <= 1e-6, "the restatement and the oracle's estimator disagree"
        want = oracle
    _guard(f"gradient_shap eeg input, {kind}", f64, want, x, bg, idx, alpha, other, "eeg")
    return ref, mine, x, bg, other, n, seed, max_batch, idx, alpha, want


@pytest.mark.parametrize("kind", ["eegnet", "multimodal", "deep"])
def test_eeg_input_against_the_fp64_oracle(kind):
    ref, mine, x, bg, other, n, seed, max_batch, idx, alpha, want = _eeg_case(kind)
    res = brainxai.gradient_shap(mine, x.to(DEV), None if other is None else other.to(DEV), bg.to(DEV), input="eeg", nsamples=n, class_idx="all",
                                 seed=seed, max_batch=max_batch, return_parts=True)
    assert res.values.shape == want.shape == (2, 6, 1, 19, 2000) and res.attribution.shape == (2, 6, 19, 2000) and res.classes is None
    assert np.array_equal(res.idx, idx) and np.array_equal(res.alpha, alpha) and res.nsamples == n
    assert torch.equal(res.attribution, res.values[:, :, 0])
    err = GG.worst(res.values, want)
    line = f"gradient_shap eeg input, {kind}: worst per-(sample, class) error {err:.3e} of the maximum (bound {TOL})"
    assert err <= TOL, line
    if other is None:                                                     # the host-loop estimator on the same seed: the same draws
        old = brainxai.expected_gradients(mine, x.to(DEV), bg.to(DEV), nsamples=n, seed=seed, max_batch=max_batch)
        eo, eb = GG.worst(old, want), GG.worst(res.values, old.cpu())
        line += f"; expected_gradients {eo:.3e}; between the two {eb:.3e}"
        assert eb <= TOL, line
    print(line)


def _spec_case():
    (eeg, spec), bg = GG.mm_inputs(), O.seeded((3, 4, 32, 64), 13, "rand")
    idx, alpha = R.draws(3, 2, 3, 6)
    return eeg, spec, bg, idx, alpha


def _composed(model, eeg, spec, bg, idx_d, alpha_d, max_batch):
    """The same pass from existing pieces: rows from the restatement's formula in torch fp32 (a subtraction, a product and a sum, each
    its own kernel), the library's forward, torch.autograd.grad with the pass composition of gradient_shap, products and running sum
    in torch fp64 in ascending draw order.  -> (rows fp32 [B*n,...], phi fp64 [B,K,C,H,W], sum of |d g| / 1 [B,K,C,H,W])."""
    B, n = idx_d.shape
    net = model.spectrogram_model
    K = int(model.fc2.out_features)
    with X._eval_frozen(model):
        with torch.no_grad():
            fixed = X._fixed_branch(model, eeg, True)
        base = bg[idx_d.long()]
        d = spec[:, None] - base
        ad = alpha_d[:, :, None, None, None] * d
        r_all = (base + ad).reshape(B * n, *spec.shape[1:])
        d = d.reshape(B * n, *spec.shape[1:]).double()
        max_rows = X._row_cap(spec, "spec", net.compute_dtype, max_batch)
        acc = torch.zeros(B, K, *spec.shape[1:], dtype=torch.float64, device=spec.device)
        absacc = torch.zeros_like(acc)
        for row0 in range(0, B * n, max_rows):
            rows = min(max_rows, B * n - row0)
            r = r_all[row0:row0 + rows].clone().requires_grad_(True)
            rep = fixed[torch.arange(row0, row0 + rows, device=spec.device) // n]
            y = X._fuse(model, True, True, net(r), rep).float()
            for c in range(K):
                seed = torch.zeros(rows, K, dtype=torch.float32, device=spec.device)
                seed[:, c] = 1.0
                (g,) = torch.autograd.grad(y, r, grad_outputs=seed, retain_graph=c + 1 < K)
                for q in range(rows):
                    j = row0 + q
                    t = d[j] * g[q].double()
                    acc[j // n, c] += t
                    absacc[j // n, c] += t.abs()
    return r_all, acc / n, absacc


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_spec_input_against_the_same_pass_from_pieces(dt):
    """The gradients are then the same launches on the same bits: what remains is the bound of the accumulate kernel."""
    _, mine = PG.scaled_multimodal(dt)
    eeg, spec, bg, idx, alpha = _spec_case()
    eeg, spec, bg = eeg.to(DEV), spec.to(DEV), bg.to(DEV)
    max_batch = 5                                                         # three passes; the first two end inside a sample
    res = brainxai.gradient_shap(mine, eeg, spec, bg, input="spec", nsamples=6, class_idx="all", draws=(idx, alpha), max_batch=max_batch, return_parts=True)
    r_all, want, absacc = _composed(mine, eeg, spec, bg, PG.dev(idx), PG.dev(alpha), max_batch)
    assert np.array_equal(r_all.cpu().numpy().view(np.int32), R.rows(spec, bg, idx, alpha).view(np.int32)), "the composed rows are not the restatement's"
    assert res.values.shape == (2, 6, 4, 32, 64) and res.attribution.shape == (2, 6, 32, 64)
    want, absacc = want.cpu().numpy(), absacc.cpu().numpy()
    assert float(np.abs(want).max()) > 0
    rv = _bound_ratio(res.values.cpu().numpy(), want, absacc)
    rm = _bound_ratio(res.attribution.cpu().numpy(), want.sum(2), absacc.sum(2))
    same = bool(np.array_equal(res.values.cpu().numpy(), want.astype(np.float32)))
    print(f"gradient_shap spec input vs composed pass, {dt}: values {rv:.3f} x bound, map {rm:.3f} x bound, bit for bit: {same}")
    assert rv <= 1.0 and rm <= 1.0


def test_spec_input_against_the_fp64_oracle():
    ref, mine = PG.scaled_multimodal()
    eeg, spec, bg, idx, alpha = _spec_case()
    B, n = idx.shape
    f64 = copy.deepcopy(ref).double().eval()
    plain = R.values(f64, spec, bg, idx, alpha, eeg, "spec")
    _guard("gradient_shap spec input, multimodal", f64, plain, spec, bg, idx, alpha, eeg, "spec")
    keep = ops.keep_block_activations(mine)
    try:                                                                  # one pass of 12 rows: the last forward, whose activations keep holds
        res = brainxai.gradient_shap(mine, eeg.to(DEV), spec.to(DEV), bg.to(DEV), input="spec", nsamples=n, class_idx="all", seed=3, return_parts=True)
        torch.cuda.synchronize()
    finally:
        ops.keep_block_activations(mine, on=False)
    assert np.array_equal(res.idx, idx) and np.array_equal(res.alpha, alpha)
    rows = torch.from_numpy(R.rows(spec, bg, idx, alpha))
    eeg_rep = eeg.repeat_interleave(n, dim=0)
    twin, flips = matched_oracle(O, ref, (eeg_rep, rows), keep, "gradient_shap spec input")
    d = torch.from_numpy(R.diffs(spec, bg, idx)).double()
    xi = rows.double().requires_grad_(True)
    y = twin(eeg_rep.double(), xi)
    want = torch.zeros_like(plain)
    for c in range(y.shape[1]):
        (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
        want[:, c] = (g * d).reshape(B, n, *spec.shape[1:]).sum(1) / n
    err, err_plain = GG.worst(res.values, want), GG.worst(res.values, plain)
    line = (f"gradient_shap spec input, multimodal 4x32x64: {len(flips)} decision flips; worst per-(sample, class) error {err:.3e} against the "
            f"decision-matched fp64 oracle, {err_plain:.3e} against the plain one (bound {TOL})")
    print(line)
    assert err <= TOL, line
    want_map = want.sum(2)
    assert GG.worst(res.attribution, want_map) <= TOL


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def _iface():
    return GG.iface() + GG.backgrounds()


def test_repeatable_draws_and_max_batch():
    mine, eeg, spec, bge, bgs = _iface()
    kw = dict(input="eeg", nsamples=6, class_idx="all", seed=3)
    a = brainxai.gradient_shap(mine, eeg, spec, bge, return_parts=True, **kw)
    b = brainxai.gradient_shap(mine, eeg, spec, bge, **kw)
    assert torch.equal(a.attribution, b), "two calls differ"
    c = brainxai.gradient_shap(mine, eeg, spec, bge, input="eeg", nsamples=6, class_idx="all", seed=99, draws=(torch.from_numpy(a.idx), a.alpha.astype(np.float64)))
    assert torch.equal(a.attribution, c), "draws= differs from the seed path"
    other = brainxai.gradient_shap(mine, eeg, spec, bge, input="eeg", nsamples=6, class_idx="all", seed=4)
    assert not torch.equal(a.attribution, other)
    small = brainxai.gradient_shap(mine, eeg, spec, bge, max_batch=5, **kw)
    err = GG.worst(small, a.attribution.cpu())
    print(f"gradient_shap max_batch 5 vs 256: {err:.3e} of the per-(sample, class) maximum, bit for bit: {torch.equal(small, a.attribution)}")
    assert err <= TOL
    s_kw = dict(input="spec", nsamples=4, class_idx="all", seed=1)
    assert torch.equal(brainxai.gradient_shap(mine, eeg, spec, bgs, **s_kw), brainxai.gradient_shap(mine, eeg, spec, bgs, **s_kw))


def test_class_forms():
    mine, eeg, spec, bge, bgs = _iface()
    for input, bg, shape in (("eeg", bge, (19, 2000)), ("spec", bgs, (32, 64))):
        kw = dict(input=input, nsamples=4, seed=5)
        every = brainxai.gradient_shap(mine, eeg, spec, bg, class_idx="all", return_parts=True, **kw)
        assert every.attribution.shape == (2, 6, *shape) and every.out.shape == (2, 6) and every.classes is None
        top = brainxai.gradient_shap(mine, eeg, spec, bg, return_parts=True, **kw)
        assert top.attribution.shape == (2, *shape) and top.values.shape[0] == 2 and top.values.dim() == 4
        assert torch.equal(top.classes, every.out.argmax(1)) and torch.equal(top.out, every.out)
        for b in range(2):
            assert torch.equal(top.attribution[b], every.attribution[b, int(top.classes[b])])
            assert torch.equal(top.values[b], every.values[b, int(top.classes[b])])
        for c in range(6):
            one = brainxai.gradient_shap(mine, eeg, spec, bg, class_idx=c, **kw)
            assert torch.equal(one, every.attribution[:, c]), f"{input}: 'all' differs from the call for class {c}"
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.gradient_shap(mine, eeg, spec, bg, class_idx=form, return_parts=True, **kw)
            assert per.classes.tolist() == [4, 1]
            assert torch.equal(per.attribution[0], every.attribution[0, 4]) and torch.equal(per.attribution[1], every.attribution[1, 1])


def test_explainer_modes_and_downstream():
    mine, eeg, spec, bge, bgs = _iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        vals = brainxai.GradientExplainer(mine, bge).shap_values(eeg, spec, nsamples=4, seed=2)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    res = brainxai.gradient_shap(mine, eeg, spec, bge, input="eeg", nsamples=4, class_idx="all", seed=2, return_parts=True)
    assert isinstance(vals, list) and len(vals) == 6 and all(isinstance(v, np.ndarray) and v.shape == tuple(eeg.shape) for v in vals)
    assert np.array_equal(np.stack(vals, 1), res.values.cpu().numpy())
    sv = brainxai.GradientExplainer(mine, bgs, input="spec").shap_values(spec, eeg, nsamples=4, seed=2)
    assert len(sv) == 6 and sv[0].shape == tuple(spec.shape)
    # the reference's reduction: mean |.| over time per electrode, top electrodes
    imp, top = brainxai.channel_importance(res.values, top=5)
    assert imp.shape == (2, 6, 1, 19) and top.shape == (2, 6, 1, 5)
    want = R.channel_importance(res.values.cpu().numpy())
    assert float(np.abs(imp.cpu().numpy() - want).max()) <= 2.0 ** -22 * float(want.max())
    # the maps drop into the faithfulness tools as they are
    for input, bg in (("eeg", bge), ("spec", bgs)):
        amap = brainxai.gradient_shap(mine, eeg, spec, bg, input=input, nsamples=4, seed=2)
        ranks = brainxai.attribution_ranks(amap)
        assert ranks.shape == (2, amap[0].numel())
        curves = brainxai.deletion_insertion(mine, eeg, spec, amap, input=input, steps=4)
        assert torch.equal(curves.ranks, ranks) and bool(torch.isfinite(curves.deletion).all()) and bool(torch.isfinite(curves.insertion).all())


def test_stand_alone_spectrogram_model():
    mine, eeg, spec, bge, bgs = _iface()
    sm = mine.spectrogram_model
    res = brainxai.gradient_shap(sm, None, spec, bgs, input="spec", nsamples=4, class_idx="all", seed=2, return_parts=True)
    assert res.values.shape == (2, 6, 4, 32, 64) and res.attribution.shape == (2, 6, 32, 64) and bool(torch.isfinite(res.values).all())
    assert float(res.values.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(res.out, sm(spec).float())
    total = res.values.double().sum(2)
    assert float((res.attribution.double() - total).abs().max()) <= 4 * 2.0 ** -24 * float(res.values.abs().sum(2).max())
    assert torch.equal(res.attribution[:, 3], brainxai.gradient_shap(sm, None, spec, bgs, input="spec", nsamples=4, class_idx=3, seed=2))
