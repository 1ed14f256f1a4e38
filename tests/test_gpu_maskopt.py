"""GPU: brainxai.mask_explain and the bx_maskopt_* entry points against the restatement of the definition (tests/maskopt_ref.py): the
rows, the up-sampled masks, G, the grid, the moments, the history and the status bit for bit, from the states the restatement itself
reaches at the first, a middle and the last iteration; then the driver end to end.

End to end the grid is moved by the gradients, so the driver is checked in three parts that together pin it: (i) the restatement, fed
the call's own dumped gradients and outputs, reproduces the dumped path, the grids, the history and the map bit for bit; (ii) every
dumped gradient is the fp64 oracle's gradient at the rows of the dumped grid within TOL = 1e-3 of its maximum (the project's fp32
gradient bound, GG.worst) -- the plain oracle for the EEG branch, the oracle whose ReLU / max-pool decisions are pinned to those of the
GPU forward of the same rows (tests/golden_util.matched_oracle) for the spectrogram branch; (iii) final, clean and reference are forward
passes of the restated rows.  Every end-to-end case is first checked ON THE REFERENCE SIDE to discriminate: replayed from the same
gradients with the mode flipped, with l1 doubled and with lr halved, the grid of every (sample, class) moves by more than MOVED -- a
driver that ignored the mode, the regulariser or the step size cannot pass (i).  (i) is bit for bit on fp32 grids in [0, 1]: it
tolerates nothing, and the most two such values can differ by without a bit of the computation having changed is one rounding, u = 2^-24
of the range; so a replay has to move by more than MOVED = 100 u of the range.  The least observed moves are printed.
No test provokes a fault or an out-of-range launch."""
import copy

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
from tests import maskopt_ref as R
from tests import perturb_gpu as PG
from tests.golden_util import matched_oracle
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3
MOVED = 100 * 2.0 ** -24

# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# (domain, grid, layouts): a layout is ('spec', C) -- x [B,C,Hm,Wm] -- or ('eeg', Chans) -- x [B,1,Chans,Wm], the domain [1,Wm] taking
# map_rows = 1 and every other one map_rows = Chans = Hm
CASES = [((1, 1), (1, 1), [("spec", 1)]),                                  # smallest
         ((1, 65), (1, 8), [("eeg", 5), ("spec", 3)]),                     # [1,T] cells: the electrodes are the channels of a column
         ((5, 4), (5, 4), [("spec", 4)]),                                  # cell size 1, i0 == i1 clamps everywhere
         ((19, 333), (1, 1), [("eeg", 19)]),                               # one cell sees every pixel
         ((19, 333), (7, 8), [("eeg", 19), ("spec", 3)]),                  # row length not a multiple of 4
         ((100, 75), (7, 8), [("spec", 3)]),                               # domain not a multiple of the grid
         ((100, 75), (32, 32), [("spec", 1)]),                             # largest grid
         ((70, 256), (16, 32), [("spec", 4)]),                             # general
         ((19, 2000), (8, 8), [("eeg", 19)]),                              # longest footprint
         ((2, 4100), (2, 5), [("spec", 3)])]                               # a line longer than the step's tile of 2048 pixels: footprints cross tiles
KB, KC, K, N_IT = 3, 3, 6, 5
RN = KB * KC
SETS = ["quantised", "signs and zeros", "normal"]
WINDOWS = [(0, RN), (1, RN - 3), (RN - 1, 1)]                              # all rows; inside the first sample to inside the last; the last row alone
SETTINGS = dict(lr=0.1, l1=0.01, tv_w=0.2, b1=0.9, b2=0.999, eps=1e-8)


def _combos(cells):
    """(mode, score, beta): the full cross on the small domains, four corners that hold every value on the large ones (the restatement
    runs on the host)."""
    if cells <= 2000:
        return [(m, s, b) for m in (R.DELETION, R.PRESERVATION) for s in (R.PROB, R.LOGPROB) for b in (1, 2, 3)]
    return [(R.DELETION, R.PROB, 3), (R.PRESERVATION, R.LOGPROB, 1), (R.DELETION, R.LOGPROB, 2), (R.PRESERVATION, R.PROB, 3)]


def _shape(dom, layout):
    what, c = layout
    if what == "spec":
        return (KB, c, *dom), 0
    return (KB, 1, c, dom[1]), (1 if dom[0] == 1 else c)


def _base(kind, shape, map_rows, rng):
    if kind == 0:
        return np.asarray([0.125], dtype=np.float32)
    if kind == 1:
        return (0.3 * rng.standard_normal(shape[2] if map_rows else shape[1])).astype(np.float32)
    return (0.3 * rng.standard_normal(shape)).astype(np.float32)


def _gradients(kind, shape, rng):
    g_shape = (RN, *shape[1:])
    if kind == "quantised":
        return (rng.choice([0.5, 1.0, 2.0, 4.0], size=g_shape) * rng.choice([-1.0, 1.0], size=g_shape)).astype(np.float32)
    g = rng.standard_normal(g_shape).astype(np.float32)
    if kind == "signs and zeros":
        flat = g.reshape(RN, -1)
        flat[:, ::5] = 0.0
        flat[:, 2::7] = -0.0
    return g


def _outputs(rng):
    z = rng.standard_normal((RN, K))
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def _state_dev(st, history, G):
    return {k: PG.dev(st[k].copy()) for k in ("m", "mu", "nu", "status")} | {"history": PG.dev(history.copy()), "G": PG.dev(G.copy())}


def _same(got, want, what):
    for key, ref in want.items():
        g = got[key].cpu().numpy()
        assert g.shape == ref.shape and np.array_equal(PG.np_bits(g), PG.np_bits(ref)), \
            f"{what}: {key} differs from the restatement in {int((PG.np_bits(g) != PG.np_bits(ref)).sum())} of {ref.size} places"


def _launch_rows(x_d, m_d, base_d, kind, shape, map_rows, grid, row0, rows):
    out = torch.full((rows, *shape[1:]), float("nan"), device=DEV)
    if map_rows == 0:
        L.check(L.load().bx_maskopt_rows_spec(PG.p(x_d), PG.p(m_d), PG.p(base_d), kind, PG.p(out), KB, KC, *shape[1:], *grid, row0, rows, PG.stream()),
                "bx_maskopt_rows_spec")
    else:
        L.check(L.load().bx_maskopt_rows_eeg(PG.p(x_d), PG.p(m_d), map_rows, PG.p(base_d), kind, PG.p(out), KB, KC, shape[2], shape[3], *grid, row0, rows,
                                             PG.stream()), "bx_maskopt_rows_eeg")
    return out


def _launch_step(x_d, base_d, kind, g_d, y_d, cls_d, sd, scratch, shape, map_rows, grid, combo, it, row0, rows):
    mode, score, beta = combo
    s = SETTINGS
    c1, c2 = 1.0 - s["b1"] ** (it + 1), 1.0 - s["b2"] ** (it + 1)
    L.check(L.load().bx_maskopt_step(PG.p(x_d), PG.p(base_d), kind, PG.p(g_d), PG.p(y_d), PG.p(cls_d), PG.p(sd["m"]), PG.p(sd["mu"]), PG.p(sd["nu"]),
                                     PG.p(sd["status"]), PG.p(sd["history"]), PG.p(sd["G"]), PG.p(scratch), KB, KC, *shape[1:], map_rows, K, *grid, mode, score, beta,
                                     s["lr"], s["l1"], s["tv_w"], s["b1"], s["b2"], s["eps"], c1, c2, it, N_IT, row0, rows, PG.stream()), "bx_maskopt_step")


def _seeded_grid(grid, rng):
    """A grid in [0, 1] with cells exactly at 0 and exactly at 1."""
    m = rng.uniform(0, 1, (RN, *grid)).astype(np.float32)
    flat = m.reshape(RN, -1)
    flat[:, ::3] = 0.0
    flat[:, 1::4] = 1.0
    return m


@pytest.mark.parametrize("dom,grid,layouts", CASES, ids=[f"{d[0]}x{d[1]}-grid{g[0]}x{g[1]}" for d, g, _ in CASES])
def test_kernels_bit_for_bit(dom, grid, layouts):
    lib = L.load()
    Hm, Wm = dom
    for li, layout in enumerate(layouts):
        shape, map_rows = _shape(dom, layout)
        rng = np.random.default_rng(1000 + 31 * Hm + Wm + 7 * grid[1] + li)
        x = rng.standard_normal(shape).astype(np.float32)
        x.reshape(-1)[::11] = -0.0
        classes = rng.integers(0, K, RN).astype(np.int32)
        cls_d = PG.dev(classes)
        x_al, x_mis = PG.dev(x), PG.misaligned(PG.dev(x))
        scratch = torch.empty(RN, Hm, grid[1], dtype=torch.float64, device=DEV)
        what0 = f"domain {dom}, grid {grid}, {layout[0]} {layout[1]}"
        # init: the window's rows only
        for row0, rows in WINDOWS:
            got = {"m": torch.full((RN, *grid), 7.0, device=DEV), "mu": torch.full((RN, *grid), 7.0, dtype=torch.float64, device=DEV),
                   "nu": torch.full((RN, *grid), 7.0, dtype=torch.float64, device=DEV), "status": torch.full((RN,), 7, dtype=torch.int32, device=DEV)}
            L.check(lib.bx_maskopt_init(PG.p(got["m"]), PG.p(got["mu"]), PG.p(got["nu"]), PG.p(got["status"]), KB, KC, *grid, row0, rows, PG.stream()), "bx_maskopt_init")
            want = {"m": np.full((RN, *grid), 7.0, dtype=np.float32), "mu": np.full((RN, *grid), 7.0), "nu": np.full((RN, *grid), 7.0),
                    "status": np.full(RN, 7, dtype=np.int32)}
            fresh = R.init(RN, *grid)
            for key in want:
                want[key][row0:row0 + rows] = fresh[key][row0:row0 + rows]
            _same(got, want, f"{what0}, init rows {row0}..{row0 + rows}")
        # rows and masks: every baseline kind, aligned and misaligned inputs, every window
        m_np = _seeded_grid(grid, rng)
        m_d = PG.dev(m_np)
        for kind in (0, 1, 2):
            base = _base(kind, shape, map_rows, rng)
            for x_d, how in ((x_al, "aligned"), (x_mis, "misaligned")):
                base_d = PG.misaligned(PG.dev(base)) if (kind == 2 and how == "misaligned") else PG.dev(base)
                for row0, rows in WINDOWS:
                    got = _launch_rows(x_d, m_d, base_d, kind, shape, map_rows, grid, row0, rows)
                    want = R.rows(x, base if kind else base[0], kind, m_np, KC, map_rows, row0, rows)
                    _same({"rows": got}, {"rows": want}, f"{what0}, rows, baseline kind {kind}, {how}, rows {row0}..{row0 + rows}")
        for row0, rows in WINDOWS:
            up = torch.full((rows, Hm, Wm), float("nan"), device=DEV)
            L.check(lib.bx_maskopt_masks(PG.p(m_d), PG.p(up), KB, KC, *grid, Hm, Wm, row0, rows, PG.stream()), "bx_maskopt_masks")
            _same({"masks": up}, {"masks": R.upsample(m_np[row0:row0 + rows], Hm, Wm)}, f"{what0}, masks rows {row0}..{row0 + rows}")
        ones = torch.empty(RN, Hm, Wm, device=DEV)
        L.check(lib.bx_maskopt_masks(PG.p(torch.ones(RN, *grid, device=DEV)), PG.p(ones), KB, KC, *grid, Hm, Wm, 0, RN, PG.stream()), "bx_maskopt_masks")
        assert bool((ones == 1.0).all()), f"{what0}: an all-ones grid does not up-sample to exactly 1.0"
        # the step
        for ci, combo in enumerate(_combos(Hm * Wm)):
            kind = ci % 3
            base = _base(kind, shape, map_rows, rng)
            base_ref = base if kind else base[0]
            mis = ci % 2 == 1                                            # every other parameter set takes the element-by-element path
            x_d = x_mis if mis else x_al
            base_d = PG.misaligned(PG.dev(base)) if (kind == 2 and mis) else PG.dev(base)
            st = R.init(RN, *grid)
            if ci % 4 != 0:                                              # not from all ones: cells at 0 and at 1 from the first iteration on
                st["m"][:] = _seeded_grid(grid, rng)
            history = np.zeros((RN, N_IT, 3))
            kw = dict(mode=combo[0], score=combo[1], beta=combo[2], **SETTINGS)
            for it in range(N_IT):
                g = _gradients(SETS[(ci + it) % 3], shape, rng)
                y = _outputs(rng)
                acc = R.data_gradient(x, base_ref, kind, g, map_rows, *grid, KC)
                if it in (0, N_IT // 2, N_IT - 1):                       # from the state the restatement has reached
                    for row0, rows in WINDOWS:
                        G = np.full((RN, *grid), np.nan)
                        sd = _state_dev(st, history, G)
                        g_d = PG.dev(g[row0:row0 + rows])
                        _launch_step(x_d, base_d, kind, PG.misaligned(g_d) if mis else g_d, PG.dev(y[row0:row0 + rows]), cls_d, sd, scratch, shape, map_rows, grid,
                                     combo, it, row0, rows)
                        want = {k: st[k].copy() for k in ("m", "mu", "nu", "status")}
                        want_h = history.copy()
                        R.step(want, x, base_ref, kind, g[row0:row0 + rows], y[row0:row0 + rows], classes, map_rows, KC, it, want_h, row0=row0, G_out=G,
                               acc=acc[row0:row0 + rows], **kw)
                        _same(sd, want | {"history": want_h, "G": G}, f"{what0}, {combo}, baseline kind {kind}, iteration {it}, rows {row0}..{row0 + rows}")
                R.step(st, x, base_ref, kind, g, y, classes, map_rows, KC, it, history, acc=acc, **kw)
            assert not st["status"].any() and np.isfinite(history).all()
        print(f"{what0}: {len(_combos(Hm * Wm))} parameter sets bit for bit")


def test_a_nan_gradient_stops_its_row_alone():
    dom, grid, shape, map_rows = (19, 333), (7, 8), (KB, 1, 19, 333), 19
    rng = np.random.default_rng(77)
    x = rng.standard_normal(shape).astype(np.float32)
    base = _base(2, shape, map_rows, rng)
    classes = rng.integers(0, K, RN).astype(np.int32)
    x_d, base_d, cls_d = PG.dev(x), PG.dev(base), PG.dev(classes)
    scratch = torch.empty(RN, dom[0], grid[1], dtype=torch.float64, device=DEV)
    st = R.init(RN, *grid)
    history = np.zeros((RN, N_IT, 3))
    G = np.full((RN, *grid), np.nan)
    sd = _state_dev(st, history, G)
    combo = (R.DELETION, R.PROB, 3)
    for it in range(3):
        g = _gradients("normal", shape, rng)
        y = _outputs(rng)
        if it == 1:
            g[4, 0, 11, 200] = np.nan
        if it == 2:
            y[7, classes[7]] = np.nan
        before = {k: st[k].copy() for k in ("m", "mu", "nu")}
        R.step(st, x, base, 2, g, y, classes, map_rows, KC, it, history, mode=combo[0], score=combo[1], beta=combo[2], G_out=G, **SETTINGS)
        _launch_step(x_d, base_d, 2, PG.dev(g), PG.dev(y), cls_d, sd, scratch, shape, map_rows, grid, combo, it, 0, RN)
        _same(sd, {k: st[k] for k in ("m", "mu", "nu", "status")} | {"history": history, "G": G}, f"iteration {it}")
        for r in ([4] if it == 1 else [4, 7] if it == 2 else []):       # stopped before anything of the step was written, and left alone afterwards
            assert all(np.array_equal(st[k][r], before[k][r]) for k in before) and not history[r, it].any()
    want = [L.BX_MASKOPT_OK] * RN
    want[4] = want[7] = L.BX_MASKOPT_NAN
    assert sd["status"].cpu().tolist() == want


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
EN = 6


def _blur(x, input):
    return brainxai.gaussian_blur(x.to(DEV), 6.0 if input == "eeg" else 3.0, axes="w" if input == "eeg" else "hw")


def _replay(res, x, base_np, kind, classes_np, map_rows, Kc, **change):
    Rn = len(classes_np)
    flat = (lambda t: t.reshape(Rn, *t.shape[(2 if Kc > 1 else 1):]).cpu().numpy())
    kw = dict(mode=X._MASKOPT_MODES[res.mode], score=X._MASKOPT_SCORES[res.score], beta=res.tv_beta, lr=res.lr, l1=res.l1, tv_w=res.tv, b1=res.betas[0],
              b2=res.betas[1], eps=res.eps)
    kw.update(change)
    return R.replay(x.numpy(), base_np, kind, flat(res.gradients), flat(res.outputs), classes_np, map_rows, Kc, *res.grid, **kw)


def _check_call(what, res, x, base, map_rows, grad_at, forward_rows):
    """res: MaskExplainResult with keep_path; grad_at(points [R*n,...], cls [R*n]) is the fp64 oracle's gradient of each point's class;
    forward_rows(rows [R,...] on the device) the package's own log-probabilities [R,K] of rows, composed as the driver composes them."""
    B = x.shape[0]
    every = res.classes is None
    Kn = res.out.shape[1]
    Kc = Kn if every else 1
    Rn = B * Kc
    gh, gw = res.grid
    flat = (lambda t: t.reshape(Rn, *t.shape[(2 if every else 1):]).cpu())
    classes_np = (np.tile(np.arange(Kn), B) if every else res.classes.cpu().numpy()).astype(np.int64)
    kind, base_np = (0, np.float32(base)) if not isinstance(base, torch.Tensor) else (2, base.cpu().numpy())
    grads, outs, path, mask, hist = (flat(t) for t in (res.gradients, res.outputs, res.path, res.mask, res.history))
    assert grads.shape == (Rn, EN, *x.shape[1:]) and outs.shape == (Rn, EN, Kn) and path.shape == (Rn, EN, gh, gw) and mask.shape == (Rn, gh, gw)
    assert hist.shape == (Rn, EN, 3) and hist.dtype == torch.float64
    # the reference side first: the same gradients, other settings
    p_ref, st_ref, h_ref = _replay(res, x, base_np, kind, classes_np, map_rows, Kc)
    assert not st_ref["status"].any()
    moved = {"mode flipped": _replay(res, x, base_np, kind, classes_np, map_rows, Kc, mode=1 - X._MASKOPT_MODES[res.mode])[1]["m"],
             "l1 doubled": _replay(res, x, base_np, kind, classes_np, map_rows, Kc, l1=2 * res.l1)[1]["m"],
             "lr halved": _replay(res, x, base_np, kind, classes_np, map_rows, Kc, lr=res.lr / 2)[1]["m"]}
    least = {how: float(np.abs(alt.astype(np.float64) - st_ref["m"]).reshape(Rn, -1).max(1).min()) for how, alt in moved.items()}
    print(f"{what}: the replay moves the grid by (least over (sample, class), of the range [0, 1]) " + ", ".join(f"{how} {v:.3e}" for how, v in least.items()))
    for how, v in least.items():
        assert v > MOVED, f"{what}: {how} moves the replayed grid by only {v:.3e}"
    # (i) the call's own gradients and outputs reproduce its path, grids, history and map
    assert np.array_equal(PG.np_bits(path.numpy()), PG.np_bits(p_ref)), f"{what}: the path is not the restatement's"
    assert np.array_equal(PG.np_bits(mask.numpy()), PG.np_bits(st_ref["m"])), f"{what}: the grids are not the restatement's"
    assert np.array_equal(PG.np_bits(hist.numpy()), PG.np_bits(h_ref)), f"{what}: the history is not the restatement's"
    Hm, Wm = res.upsampled.shape[-2:]
    up_ref = R.upsample(st_ref["m"], Hm, Wm)
    assert np.array_equal(PG.np_bits(flat(res.upsampled).numpy()), PG.np_bits(up_ref)), f"{what}: the up-sampled masks are not the restatement's"
    map_ref = (np.float32(1) - up_ref).astype(np.float32) if res.mode == "deletion" else up_ref
    assert np.array_equal(PG.np_bits(flat(res.map).numpy()), PG.np_bits(map_ref)), f"{what}: the map is not the restatement's"
    print(f"{what}: score {hist[:, 0, 0].tolist()} -> {hist[:, -1, 0].tolist()}, mean grid {float(hist[:, -1, 1].min()):.3f} .. {float(hist[:, -1, 1].max()):.3f}")
    # (ii) the dumped gradients are the oracle's at the rows of the dumped grids
    points = torch.from_numpy(np.stack([R.rows(x.numpy(), base_np, kind, p_ref[:, it], Kc, map_rows) for it in range(EN)], axis=1))
    cls = torch.from_numpy(classes_np).repeat_interleave(EN)
    want_g = grad_at(points.reshape(Rn * EN, *x.shape[1:]), cls).reshape(Rn, EN, -1)
    err = GG.worst(grads.reshape(Rn, EN, -1), want_g)
    print(f"{what}: gradients {err:.3e} of the per-(row, iteration) maximum")
    assert err <= TOL, f"{what}: gradients {err:.3e}"
    # (iii) final, clean and reference are forward passes of the restated rows
    def scores(logp):
        s = logp if res.score == "logprob" else X._softmax_rows(logp.contiguous())
        return s.gather(1, torch.from_numpy(classes_np).to(DEV)[:, None])[:, 0]
    with torch.no_grad():
        last = forward_rows(torch.from_numpy(R.rows(x.numpy(), base_np, kind, st_ref["m"], Kc, map_rows)).to(DEV))
        zero = forward_rows(torch.from_numpy(R.rows(x.numpy(), base_np, kind, np.zeros_like(st_ref["m"]), Kc, map_rows)).to(DEV))
        assert torch.equal(flat(res.final), scores(last).cpu()), f"{what}: final is not the score of the rows of the final grid"
        assert torch.equal(flat(res.clean), scores(res.out.repeat_interleave(Kc, dim=0)).cpu()), f"{what}: clean is not the score of the clean output"
        ref_err = float((flat(res.reference) - scores(zero).cpu()).abs().max())
        assert ref_err <= PG.TOL, f"{what}: reference differs from the score of the all-baseline rows by {ref_err:.3e}"
    return points


def _grad_rows(forward):
    def grad_at(points, cls):
        xi = points.double().clone().requires_grad_(True)
        y = forward(xi)
        (g,) = torch.autograd.grad(y.gather(1, cls[:, None]).sum(), xi)
        return g
    return grad_at


EEG_CALLS = [("eegnet", "all", dict(mode="deletion", score="prob", tv_beta=3, grid=16), "zero", "electrode_time"),
             ("eegnet", None, dict(mode="preservation", score="logprob", tv_beta=1, grid=(4, 12)), "blur", "electrode_time"),
             ("multimodal", None, dict(mode="deletion", score="logprob", tv_beta=2, grid=8), "blur", "time"),
             ("multimodal", "all", dict(mode="preservation", score="prob", tv_beta=3, grid=(7, 9)), "zero", "electrode_time")]


@pytest.mark.parametrize("kind,classes,kw,which,cells", EEG_CALLS, ids=[f"{c[0]}-{c[1]}-{c[2]['mode']}-{c[4]}" for c in EEG_CALLS])
def test_eeg_input_end_to_end(kind, classes, kw, which, cells):
    if kind == "eegnet":
        ref, mine = PG.eegnet_pair()
        x, other = O.seeded((2, 1, 19, 2000), 91, "randn"), None
    else:
        ref, mine = PG.scaled_multimodal()
        x, other = GG.mm_inputs()
    f64 = copy.deepcopy(ref).double().eval()
    base = 0.0 if which == "zero" else _blur(x, "eeg")
    res = brainxai.mask_explain(mine, x.to(DEV), None if other is None else other.to(DEV), input="eeg", iterations=EN, baseline=base, cells=cells,
                                class_idx=classes, keep_path=True, return_parts=True, **kw)
    Kc = 6 if classes == "all" else 1
    Hm = 1 if cells == "time" else 19
    assert res.map.shape == ((2, 6, Hm, 2000) if Kc == 6 else (2, Hm, 2000)) and res.map.dtype == torch.float32 and res.iterations == EN
    Rn = 2 * Kc
    forward = f64 if other is None else BR.two_input(f64, other, "eeg", Kc * EN)
    net = mine if other is None else mine.eeg_model

    def forward_rows(rows):
        with X._eval_frozen(mine):
            if other is None:
                return net(rows).float().contiguous()
            fixed = X._fixed_branch(mine, other.to(DEV), False)
            return X._fuse(mine, True, False, net(rows), fixed.index_select(0, X._sample_of(0, Rn, Kc, DEV))).float().contiguous()
    _check_call(f"mask_explain eeg input, {kind}, class_idx {classes}, {kw}, {which} baseline, cells {cells}", res, x, base, 1 if cells == "time" else 19,
                _grad_rows(forward), forward_rows)


SPEC_CALLS = [("multimodal", None, dict(mode="deletion", score="prob", tv_beta=3, grid=8), "blur"),
              ("spectrogram", "all", dict(mode="preservation", score="logprob", tv_beta=2, grid=(5, 7), l1=1.0), "zero")]
# (l1 = 1 in the second call: from a grid of ones a class whose log-probability every cell raises keeps its grid clamped at 1 under the
# default l1 -- its replays then cannot move, whatever the driver does; with l1 / (gh gw) = 0.029 per cell every row leaves the clamp.)


@pytest.mark.parametrize("kind,classes,kw,which", SPEC_CALLS, ids=[f"{c[0]}-{c[1]}-{c[2]['mode']}" for c in SPEC_CALLS])
def test_spec_input_end_to_end(kind, classes, kw, which):
    ref, mine = PG.scaled_multimodal()
    eeg, spec = GG.mm_inputs()
    if kind == "spectrogram":
        ref, mine, eeg = ref.spectrogram_model, mine.spectrogram_model, None
    base = 0.0 if which == "zero" else _blur(spec, "spec")
    res = brainxai.mask_explain(mine, None if eeg is None else eeg.to(DEV), spec.to(DEV), input="spec", iterations=EN, baseline=base, class_idx=classes,
                                keep_path=True, return_parts=True, **kw)
    Kc = 6 if classes == "all" else 1
    Rn = 2 * Kc
    assert res.map.shape == ((2, 6, 32, 64) if Kc == 6 else (2, 32, 64)) and res.map.dtype == torch.float32
    what = f"mask_explain spec input, {kind}, class_idx {classes}, {kw}, {which} baseline"
    net = mine if eeg is None else mine.spectrogram_model

    def forward_rows(rows):
        with X._eval_frozen(mine):
            if eeg is None:
                return net(rows).float().contiguous()
            fixed = X._fixed_branch(mine, eeg.to(DEV), True)
            return X._fuse(mine, True, True, net(rows), fixed.index_select(0, X._sample_of(0, Rn, Kc, DEV))).float().contiguous()
    # the rows of the dumped grids (the restatement's: (i) shows them to be the call's), then the decisions of their GPU forward
    kind_b, base_np = (0, np.float32(0.0)) if which == "zero" else (2, base.cpu().numpy())
    every = classes == "all"
    path = res.path.reshape(Rn, EN, *res.grid).cpu().numpy()
    flat = torch.from_numpy(np.stack([R.rows(spec.numpy(), base_np, kind_b, path[:, it], Kc, 0) for it in range(EN)], axis=1)).reshape(Rn * EN, *spec.shape[1:])
    keep = ops.keep_block_activations(mine)
    try:
        with X._eval_frozen(mine):
            net(flat.to(DEV).requires_grad_(True))
        torch.cuda.synchronize()
    finally:
        ops.keep_block_activations(mine, on=False)
    args = (flat,) if eeg is None else (eeg.repeat_interleave(Kc * EN, dim=0), flat)
    twin, flips = matched_oracle(O, ref, args, keep, what)
    print(f"{what}: {len(flips)} decision flips")
    _check_call(what, res, spec, base, 0, _grad_rows((lambda xi: twin(xi)) if eeg is None else (lambda xi: twin(args[0].double(), xi))), forward_rows)
    assert every == (res.classes is None)


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_class_forms_and_max_batch():
    mine, eeg, spec = GG.iface()
    for input, shape, extra in (("eeg", (19, 2000), {}), ("spec", (32, 64), {}), ("eeg", (1, 2000), dict(cells="time"))):
        kw = dict(input=input, iterations=4, grid=6, **extra)
        every = brainxai.mask_explain(mine, eeg, spec, class_idx="all", return_parts=True, keep_path=True, **kw)
        gh, gw = every.grid
        assert every.map.shape == (2, 6, *shape) and every.mask.shape == (2, 6, gh, gw) and every.history.shape == (2, 6, 4, 3) and every.classes is None
        assert every.final.shape == every.clean.shape == every.reference.shape == (2, 6) and every.path.shape == (2, 6, 4, gh, gw)
        assert (gh, gw) == ((1, 6) if extra else (6, 6)) and bool((every.path[:, :, 0] == 1.0).all())
        top = brainxai.mask_explain(mine, eeg, spec, return_parts=True, **kw)
        assert top.map.shape == (2, *shape) and top.mask.shape == (2, gh, gw) and top.final.shape == (2,) and top.path is None and top.gradients is None
        assert torch.equal(top.classes, every.out.argmax(1)) and torch.equal(top.out, every.out)
        for b in range(2):
            assert torch.equal(top.map[b], every.map[b, int(top.classes[b])]) and torch.equal(top.history[b], every.history[b, int(top.classes[b])])
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.mask_explain(mine, eeg, spec, class_idx=form, return_parts=True, **kw)
            assert per.classes.tolist() == [4, 1] and torch.equal(per.map[0], every.map[0, 4]) and torch.equal(per.map[1], every.map[1, 1])
        assert torch.equal(brainxai.mask_explain(mine, eeg, spec, class_idx=2, **kw), every.map[:, 2])
        for mb in (1, 5, 256):                       # 12 rows in passes of 1, of 5 (a prime: a pass ends inside a sample) and in one
            small = brainxai.mask_explain(mine, eeg, spec, class_idx="all", max_batch=mb, return_parts=True, **kw)
            assert torch.equal(small.mask, every.mask) and torch.equal(small.history, every.history) and torch.equal(small.map, every.map) \
                and torch.equal(small.final, every.final), f"mask_explain {input}: max_batch {mb} changes bits"


def test_downstream_and_restored_state():
    mine, eeg, spec = GG.iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        res = brainxai.mask_explain(mine, eeg, spec, input="spec", iterations=4, grid=8, baseline=_blur(spec, "spec"), return_parts=True)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    assert res.map.shape == (2, 32, 64) and res.map.dtype == torch.float32 and float(res.map.min()) >= 0.0 and float(res.map.max()) <= 1.0
    for input in ("spec", "eeg"):
        amap = res.map if input == "spec" else brainxai.mask_explain(mine, eeg, spec, input="eeg", iterations=3, mode="preservation", baseline=_blur(eeg, "eeg"))
        assert amap.dtype == torch.float32 and amap.shape == ((2, 32, 64) if input == "spec" else (2, 19, 2000))
        ranks = brainxai.attribution_ranks(amap)
        assert ranks.shape == (2, amap[0].numel())
        curves = brainxai.deletion_insertion(mine, eeg, spec, amap, input=input, steps=4)
        assert torch.equal(curves.ranks, ranks) and bool(torch.isfinite(curves.deletion).all()) and bool(torch.isfinite(curves.insertion).all())
    sm = mine.spectrogram_model
    alone = brainxai.mask_explain(sm, None, spec, iterations=3, baseline=torch.full((4,), 0.5), class_idx="all", return_parts=True)
    assert alone.map.shape == (2, 6, 32, 64) and float(alone.map.max()) > 0
    with torch.no_grad():
        assert torch.equal(alone.out, sm(spec).float())
