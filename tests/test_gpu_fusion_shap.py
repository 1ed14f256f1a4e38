"""GPU: Fusion SHAP -- bx_fusion_values, bx_shapley_exact, bx_fusion_interaction through ctypes with chosen votes and random heads, and
the driver end to end, against the numpy fp64 restatement (tests/fusion_shap_ref.py).

The tolerance of a value v is measured in the test against code that exists without this feature.  d0 = max |v_composed - v_ref|, where
v_composed pushes the same composed rows (torch indexing) through bx_fusion_head_fwd (+ bx_softmax_rows) and averages in fp64.  The new
kernel must stay within tol = max(4 d0, 16 * 2^-24 * scale), scale = 1 for probabilities and max |log-probability| for
log-probabilities: the kernel reassociates the (2K+1)-term first-layer sum (the groups' joins), whose worst-case rounding bound equals the
existing order's while the realised errors need not (the factor 4); d0 can by chance be a rounding or two (the floor).  A Shapley value
is a sum of differences of values with weights that add up to 1, so it carries 2 tol, the modality values likewise, the interaction
(four values) 4 tol.  Every d0 and deviation is printed.

Shapes.  K in {2, 3, 6, 8}, Hd in {2K, 64, 65, 128, 200}, Nb in {1, 2, 65}, B in {1, 3}: all twenty (K, Hd) pairs, every Nb and every B
with every K and with every Hd >= 64 -- not the full cross product, whose fp64 restatement at K = 8 (65536 masks) with Nb = 65 and
Hd = 200 alone takes longer than the rest of the file.  The hidden units are tiled from (K, Hd) = (6, 128), (6, 200) and (8, >= 64) on;
one coalition per thread everywhere but (8, ., ., 3), which takes two.  PATHS adds the shapes at which the launcher takes its other
paths: four coalitions per thread (B * ceil(NS / 1024) >= 256) at K = 6 and K = 8, and K = 9, where the votes are cut into four groups."""
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from oracle import ref_torch as O
from tests import fusion_shap_ref as R
from tests import perturb_gpu as PG

pytestmark = pytest.mark.gpu

FLOOR = 16 * 2.0 ** -24
SCORES = {"prob": L.BX_FUSION_SCORE_PROB, "logprob": L.BX_FUSION_SCORE_LOGPROB}
#        K   Hd  Nb  B
SHAPES = [(2, 4, 1, 1), (2, 64, 2, 3), (2, 65, 65, 3), (2, 128, 65, 1), (2, 200, 1, 3),
          (3, 6, 65, 3), (3, 64, 1, 1), (3, 65, 2, 3), (3, 128, 2, 1), (3, 200, 65, 3),
          (6, 12, 2, 3), (6, 64, 65, 1), (6, 65, 1, 3), (6, 128, 65, 3), (6, 200, 2, 1),
          (8, 16, 65, 1), (8, 64, 2, 3), (8, 65, 1, 1), (8, 128, 1, 3), (8, 200, 2, 1)]
PATHS = [(6, 12, 1, 64), (8, 16, 1, 4), (9, 18, 2, 1)]


def _bits64(t):
    return t.contiguous().view(torch.int64)


def _values(ex, sx, eb, sb, masks, head, score):
    """bx_fusion_values on device tensors -> fp64 [B,NS,K], pre-filled with NaN (every element must be written)."""
    B, K = ex.shape
    Nb, NS, Hd = eb.shape[0], masks.shape[0], head[0].shape[0]
    v = torch.full((B, NS, K), float("nan"), dtype=torch.float64, device=PG.DEV)
    L.check(L.load().bx_fusion_values(PG.p(ex), PG.p(sx), PG.p(eb), PG.p(sb), PG.p(masks), *(PG.p(t) for t in head), SCORES[score], PG.p(v),
                                      B, Nb, NS, K, Hd, PG.stream()), "bx_fusion_values")
    torch.cuda.synchronize()
    assert not torch.isnan(v).any(), "unwritten values"
    return v


def _composed(ex, sx, eb, sb, masks, head, score):
    """The same values from the pieces that exist without the kernel: composed rows by torch indexing, bx_fusion_head_fwd,
    bx_softmax_rows, an fp64 mean over the background rows."""
    lib = L.load()
    B, K = ex.shape
    Nb, NS, Hd = eb.shape[0], masks.shape[0], head[0].shape[0]
    bits = ((masks.to(torch.int64)[:, None] >> torch.arange(2 * K, device=PG.DEV)[None, :]) & 1).bool()
    zx, zb = torch.cat([ex, sx], 1), torch.cat([eb, sb], 1)
    total = torch.zeros(B, NS, K, dtype=torch.float64, device=PG.DEV)
    for j in range(Nb):
        rows = torch.where(bits[None], zx[:, None, :], zb[j][None, None, :]).reshape(B * NS, 2 * K)
        e, s = rows[:, :K].contiguous(), rows[:, K:].contiguous()
        hidden = torch.empty(B * NS, Hd, dtype=torch.float32, device=PG.DEV)
        out = torch.empty(B * NS, K, dtype=torch.float32, device=PG.DEV)
        L.check(lib.bx_fusion_head_fwd(PG.p(e), PG.p(s), *(PG.p(t) for t in head), PG.p(hidden), PG.p(out), B * NS, K, Hd, PG.stream()), "bx_fusion_head_fwd")
        if score == "prob":
            probs = torch.empty_like(out)
            L.check(lib.bx_softmax_rows(PG.p(out), PG.p(probs), B * NS, K, PG.stream()), "bx_softmax_rows")
            out = probs
        total += out.double().reshape(B, NS, K)
    return total / Nb


def _tolerance(v_ref, v_composed, score):
    d0 = float(np.abs(v_composed - v_ref).max())
    scale = 1.0 if score == "prob" else float(np.abs(v_ref).max())
    return d0, max(4 * d0, FLOOR * scale)


def _case(K, Hd, Nb, B, seed):
    host = (R.random_votes(B, K, 10 + seed), R.random_votes(B, K, 20 + seed), R.random_votes(Nb, K, 30 + seed), R.random_votes(Nb, K, 40 + seed))
    head = R.random_head(K, Hd, seed)
    return host, head, tuple(PG.dev(a) for a in host), tuple(PG.dev(a) for a in head)


def _full_masks(K):
    return np.arange(1 << (2 * K), dtype=np.int64).astype(np.uint32)


def _dev_masks(masks):
    return PG.dev(np.ascontiguousarray(masks).view(np.int32))


@pytest.mark.parametrize("score", ["prob", "logprob"])
@pytest.mark.parametrize("K,Hd,Nb,B", SHAPES + PATHS, ids=lambda v: str(v))
def test_values(K, Hd, Nb, B, score):
    seed = (K + Hd + Nb + B) % 3
    host, head, dv, dh = _case(K, Hd, Nb, B, seed)
    full = _full_masks(K)
    NS = full.shape[0]
    got = _values(*dv, _dev_masks(full), dh, score)
    # ---- against the restatement, within the measured tolerance (at most 2^16 masks of a longer list go through the fp64 side) ----
    sel = np.arange(NS) if NS <= 1 << 16 else np.arange(0, NS, NS >> 16)
    ref = R.values(*host, full[sel], head, score)
    comp = _composed(*dv, _dev_masks(full[sel]), dh, score).cpu().numpy()
    d0, tol = _tolerance(ref, comp, score)
    dev_ = float(np.abs(got.cpu().numpy()[:, sel] - ref).max())
    print(f"K {K} Hd {Hd} Nb {Nb} B {B} {score}: d0 = {d0:.2e}, kernel deviation = {dev_:.2e}, tol = {tol:.2e}, span of v = {np.ptp(ref):.2e}")
    assert np.ptp(ref) > 100 * tol, "the case does not discriminate"
    assert dev_ <= tol
    # ---- bit for bit: no value depends on the list it stands in ----
    e = (1 << K) - 1
    lists = {"modality": np.array([0, e, e << K, e | (e << K)], dtype=np.int64),
             "one": np.array([(NS // 3) | 1], dtype=np.int64),
             "window": np.arange(NS // 3, NS // 3 + min(NS // 2, 1500) + 1, dtype=np.int64),
             "cut head": np.arange(0, NS // 2 + 1, dtype=np.int64),
             "cut tail": np.arange(NS // 2 + 1, NS, dtype=np.int64)}
    for name, idx in lists.items():
        sub = _values(*dv, _dev_masks(full[idx]), dh, score)
        assert torch.equal(_bits64(sub), _bits64(got[:, torch.from_numpy(idx).to(PG.DEV)])), f"{name}: the values depend on the list"
    # ---- bit for bit: with the sample as the one background row every coalition composes the sample ----
    some = _dev_masks(np.concatenate([full[:: max(1, NS >> 12)], full[-1:]]))
    for b in range(min(B, 3)):
        xb = (dv[0][b:b + 1].contiguous(), dv[1][b:b + 1].contiguous())
        same = _values(*xb, *xb, some, dh, score)
        assert torch.equal(_bits64(same), _bits64(same[:, -1:].expand_as(same))), "background = sample: v(S) != v(all)"
        assert torch.equal(_bits64(same[:, -1]), _bits64(got[b:b + 1, -1])), "v(all) depends on the background"


def test_values_mean_is_a_running_sum_in_row_order():
    """Nb identical background rows give the bits of one: the fp64 sum of Nb equal fp32 scores and the division are exact."""
    host, head, dv, dh = _case(3, 65, 1, 3, 0)
    masks = _dev_masks(_full_masks(3))
    one = _values(*dv, masks, dh, "prob")
    many = _values(dv[0], dv[1], dv[2].repeat(7, 1), dv[3].repeat(7, 1), masks, dh, "prob")
    assert torch.equal(_bits64(one), _bits64(many))


@pytest.mark.parametrize("M", [1, 2, 3, 12, 16])
def test_shapley_exact(M):
    """Against the restatement to 1e-12 of max |v|: at most 2^M <= 65536 fp64 roundings of terms no larger than max |v| is 7e-12 in the
    worst case and far less realised."""
    lib = L.load()
    Rr = 2 if M == 16 else 5
    v = np.random.default_rng(M).standard_normal((Rr, 1 << M))
    w = brainxai.shapley_weights(M)
    phi = torch.full((Rr, M), float("nan"), dtype=torch.float64, device=PG.DEV)
    v_d, w_d = PG.dev(v), PG.dev(w)
    L.check(lib.bx_shapley_exact(PG.p(v_d), PG.p(w_d), PG.p(phi), Rr, M, PG.stream()), "bx_shapley_exact")
    got = phi.cpu().numpy()
    want = R.shapley(v, R.weights(M))
    bound = 1e-12 * np.abs(v).max()
    err, eff = np.abs(got - want).max(), np.abs(got.sum(-1) - (v[:, -1] - v[:, 0])).max()
    print(f"M {M}: |phi - ref| = {err:.1e}, |sum phi - (v(all) - v(none))| = {eff:.1e}, bound {bound:.1e}")
    assert not np.isnan(got).any() and err <= bound and eff <= bound
    assert np.abs(got - R.shapley(v, R.banzhaf_weights(M))).max() > 100 * bound or M <= 2


def test_interaction():
    v4 = np.random.default_rng(5).standard_normal((300, 4))
    out = torch.full((300,), float("nan"), dtype=torch.float64, device=PG.DEV)
    v_d = PG.dev(v4)
    L.check(L.load().bx_fusion_interaction(PG.p(v_d), PG.p(out), 300, PG.stream()), "bx_fusion_interaction")
    assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(R.interaction(v4)))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_values_to_shapley_on_random_heads(K, seed):
    """The three entry points in the driver's order on the games of tests/test_fusion_shap_cpu.py (same seeds: random heads at torch's
    default bounds, votes log_softmax(2 N(0,1)), Hd = 32, B = 3, Nb = 5).  Checked first on the reference side: Banzhaf weights and a
    modality value summed up from its members' values are more than 100 x the bound away, so neither mistake can pass."""
    lib = L.load()
    host, head, dv, dh = _case(K, 32, 5, 3, seed)
    groups = R.players("votes", K)
    M, n = 2 * K, 1 << (2 * K)
    masks = X._fusion_masks(groups, K)
    ref = R.explain(*host, groups, head, "prob")
    comp = _composed(*dv, _dev_masks(masks[:n]), dh, "prob").cpu().numpy()
    d0, tol = _tolerance(ref["v"], comp, "prob")
    wrong = R.explain(*host, groups, head, "prob", w=R.banzhaf_weights(M))["values"]
    summed = np.stack([ref["values"][..., :K].sum(-1), ref["values"][..., K:].sum(-1)], -1)
    guard = min(np.abs(wrong - ref["values"]).max(), np.abs(summed - ref["modality"]).max())
    assert guard > 100 * 2 * tol, f"the case does not discriminate: {guard:.1e}"
    v = _values(*dv, _dev_masks(masks), dh, "prob")
    rows = v.permute(0, 2, 1)
    game, duo = rows[..., :n].reshape(3 * K, n).contiguous(), rows[..., n:].reshape(3 * K, 4).contiguous()
    phi, mod, inter = (torch.full((3 * K, m), float("nan"), dtype=torch.float64, device=PG.DEV) for m in (M, 2, 1))
    w_m, w_2 = PG.dev(brainxai.shapley_weights(M)), PG.dev(brainxai.shapley_weights(2))
    L.check(lib.bx_shapley_exact(PG.p(game), PG.p(w_m), PG.p(phi), 3 * K, M, PG.stream()), "bx_shapley_exact")
    L.check(lib.bx_shapley_exact(PG.p(duo), PG.p(w_2), PG.p(mod), 3 * K, 2, PG.stream()), "bx_shapley_exact")
    L.check(lib.bx_fusion_interaction(PG.p(duo), PG.p(inter), 3 * K, PG.stream()), "bx_fusion_interaction")
    e_phi = np.abs(phi.cpu().numpy().reshape(3, K, M) - ref["values"]).max()
    e_mod = np.abs(mod.cpu().numpy().reshape(3, K, 2) - ref["modality"]).max()
    e_int = np.abs(inter.cpu().numpy().reshape(3, K) - ref["interaction"]).max()
    print(f"K {K} seed {seed}: d0 = {d0:.2e}, tol = {tol:.2e}, values {e_phi:.2e}, modality {e_mod:.2e}, interaction {e_int:.2e}, guard {guard:.1e}")
    assert e_phi <= 2 * tol and e_mod <= 2 * tol and e_int <= 4 * tol


# ---- the driver end to end -------------------------------------------------------------------------------------------------------------------
_SETUPS = {}


def _setup(K):
    """(model, eeg, spec, background inputs, votes, background votes, head on the host), built once per K and never changed."""
    if K not in _SETUPS:
        model = O.fill_params(brainxai.build_multimodal(19, 2000, 4, num_classes=K, dropout=0.0), seed=42)
        with torch.no_grad():                                             # as PG.scaled_multimodal: un-saturated heads
            model.spectrogram_model.fc.weight *= 0.05
            model.eeg_model.dense.weight *= 0.05
            model.fc2.weight *= 0.5
        model = model.to(PG.DEV).eval()
        eeg, spec = (t.to(PG.DEV) for t in PG.mm_inputs())
        bg = (O.seeded((5, 1, 19, 2000), 13, "randn").to(PG.DEV), O.seeded((5, 4, 64, 128), 14, "rand").to(PG.DEV))
        votes, bgv = brainxai.fusion_votes(model, eeg, spec), brainxai.fusion_votes(model, *bg)
        head = tuple(t.detach().cpu().numpy() for t in (model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias))
        _SETUPS[K] = (model, eeg, spec, bg, votes, bgv, head)
    return _SETUPS[K]


def _host(votes):
    return votes.e.cpu().numpy(), votes.s.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _driver_tol(K, score):
    """tol of the values v on the driver's own votes, measured on the full mask list as in test_values."""
    model, eeg, spec, bg, votes, bgv, head = _setup(K)
    full = _full_masks(K)
    dh = tuple(PG.dev(a) for a in head)
    ref = R.values(*_host(votes), *_host(bgv), full, head, score)
    comp = _composed(votes.e, votes.s, bgv.e, bgv.s, _dev_masks(full), dh, score).cpu().numpy()
    return _tolerance(ref, comp, score)


@pytest.mark.parametrize("K", [3, 6])
def test_fusion_votes_are_the_branches_outputs(K):
    model, eeg, spec, bg, votes, bgv, head = _setup(K)
    with torch.no_grad():
        e, s = model.eeg_model(eeg).float(), model.spectrogram_model(spec).float()
    assert votes.e.dtype == torch.float32 and votes.e.shape == (3, K) and bgv.s.shape == (5, K)
    assert torch.equal(PG.bits(votes.e), PG.bits(e)) and torch.equal(PG.bits(votes.s), PG.bits(s))
    small = brainxai.fusion_votes(model, eeg, spec, max_batch=1)
    assert torch.equal(PG.bits(small.e), PG.bits(votes.e)) and torch.equal(PG.bits(small.s), PG.bits(votes.s))


@pytest.mark.parametrize("score", ["prob", "logprob"])
@pytest.mark.parametrize("K", [3, 6])
def test_driver_against_the_restatement(K, score):
    model, eeg, spec, bg, votes, bgv, head = _setup(K)
    d0, tol = _driver_tol(K, score)
    state = PG.model_state(model)
    params = [q.detach().clone() for q in model.parameters()]
    custom = [[2 * K - 1, 0], list(range(1, K)), list(range(K, 2 * K - 1))]
    worst = 0.0
    for players, class_idx in (("votes", None), ("votes", "all"), ("modality", 1), ("class", torch.tensor([0, K - 1, 1])), (custom, "all"), ("class", "all")):
        res = brainxai.fusion_shap(model, eeg, spec, bg, players=players, class_idx=class_idx, score=score, return_parts=True)
        groups = R.players(players, K)
        ref = R.explain(*_host(res.votes), *_host(res.background), groups, head, score)
        if class_idx == "all":
            classes, pick = None, lambda a: a
        else:
            classes = ref["clean"].argmax(1) if class_idx is None else np.broadcast_to(np.asarray(class_idx), (3,))
            pick = lambda a: a[np.arange(3), classes]
            assert res.classes.dtype == torch.int64 and np.array_equal(res.classes.cpu().numpy(), classes)
        assert res.classes is None or class_idx != "all"
        M = len(groups)
        assert res.values.dtype == torch.float64 and res.values.shape == ((3, K, M) if class_idx == "all" else (3, M))
        assert res.modality.shape == ((3, K, 2) if class_idx == "all" else (3, 2)) and res.interaction.shape == ((3, K) if class_idx == "all" else (3,))
        assert res.v.shape == (3, 1 << M, K) and res.masks.shape == (1 << M,) and res.players == groups and res.score == score
        errs = {"v": (np.abs(res.v.cpu().numpy() - ref["v"]).max(), tol), "clean": (np.abs(res.clean.cpu().numpy() - ref["clean"]).max(), tol),
                "empty": (np.abs(res.empty.cpu().numpy() - ref["empty"]).max(), tol),
                "values": (np.abs(res.values.cpu().numpy() - pick(ref["values"])).max(), 2 * tol),
                "modality": (np.abs(res.modality.cpu().numpy() - pick(ref["modality"])).max(), 2 * tol),
                "interaction": (np.abs(res.interaction.cpu().numpy() - pick(ref["interaction"])).max(), 4 * tol)}
        print(f"K {K} {score} players {players if isinstance(players, str) else 'custom'} class_idx {class_idx if isinstance(class_idx, (str, int, type(None))) else 'tensor'}: "
              f"d0 = {d0:.2e}, tol = {tol:.2e}, " + ", ".join(f"{k} {e:.2e}" for k, (e, _) in errs.items()))
        for name, (err, bound) in errs.items():
            assert err <= bound, f"{name}: {err:.2e} > {bound:.2e}"
        worst = max(worst, errs["values"][0])
        assert np.abs(pick(ref["values"])).max() > 100 * 2 * tol, "the case does not discriminate"
        # efficiency on the device's own numbers: 2^M fp64 terms of at most max |v|
        gap = (res.values.sum(-1) - (res.clean - res.empty if class_idx == "all" else (res.clean - res.empty).gather(1, res.classes[:, None])[:, 0])).abs().max()
        assert float(gap) <= 1e-12 * float(res.v.abs().max())
        # the plain call returns the values
        plain = brainxai.fusion_shap(model, eeg, spec, res.background, players=players, class_idx=class_idx, score=score)
        assert torch.equal(_bits64(plain), _bits64(res.values))
    assert PG.model_state(model) == state and all(torch.equal(a, b) for a, b in zip(params, model.parameters()))


@pytest.mark.parametrize("K", [3, 6])
def test_driver_clean_is_the_models_score(K):
    """clean = v(all) against the model's own forward pass.  clean is within tol of the fp64 head on the fp32 votes; the model's own
    forward (its fused head launch, which also recomputes the votes) carries the project's recorded fp32 bound PG.TOL = 1e-5 on a
    probability or a log-probability: the two are within tol + PG.TOL of one another."""
    model, eeg, spec, bg, votes, bgv, head = _setup(K)
    for score in ("prob", "logprob"):
        d0, tol = _driver_tol(K, score)
        res = brainxai.fusion_shap(model, eeg, spec, bgv, players="modality", score=score, return_parts=True)
        with torch.no_grad():
            logp = model(eeg, spec).float()
        own = (logp.exp() if score == "prob" else logp).double()
        truth = torch.from_numpy(R.scores(R.head(np.concatenate(_host(votes), 1).astype(np.float64), head), score)).to(PG.DEV)
        err, err_truth = float((res.clean - own).abs().max()), float((res.clean - truth).abs().max())
        print(f"K {K} {score}: |clean - model's own score| = {err:.2e} (bound {tol + PG.TOL:.2e}), |clean - fp64 head on the votes| = {err_truth:.2e} (tol {tol:.2e})")
        assert err_truth <= tol and err <= tol + PG.TOL


@pytest.mark.parametrize("K", [3, 6])
def test_driver_bit_for_bit(K):
    model, eeg, spec, bg, votes, bgv, head = _setup(K)
    base = brainxai.fusion_shap(model, eeg, spec, bg, players="votes", class_idx="all", return_parts=True)
    # max_batch changes no bit
    for mb in (1, 2):
        res = brainxai.fusion_shap(model, eeg, spec, bg, players="votes", class_idx="all", max_batch=mb, return_parts=True)
        for a, b in ((res.values, base.values), (res.modality, base.modality), (res.interaction, base.interaction), (res.v, base.v)):
            assert torch.equal(_bits64(a), _bits64(b)), f"max_batch {mb}"
        assert torch.equal(PG.bits(res.votes.e), PG.bits(base.votes.e)) and torch.equal(PG.bits(res.background.s), PG.bits(base.background.s))
    # a background given as inputs and as its votes is the same background
    res = brainxai.fusion_shap(model, eeg, spec, bgv, players="votes", class_idx="all", return_parts=True)
    assert torch.equal(_bits64(res.values), _bits64(base.values))
    # a players='modality' call returns the modality of a players='votes' call, and of every other game
    for players in ("modality", "class"):
        res = brainxai.fusion_shap(model, eeg, spec, bgv, players=players, class_idx="all", return_parts=True)
        assert torch.equal(_bits64(res.modality), _bits64(base.modality)) and torch.equal(_bits64(res.interaction), _bits64(base.interaction))
        assert torch.equal(_bits64(res.clean), _bits64(base.clean)) and torch.equal(_bits64(res.empty), _bits64(base.empty))
        if players == "modality":
            assert torch.equal(_bits64(res.values), _bits64(base.modality))
    # 'uniform' is one background row of fl32(-log K)
    row = torch.full((1, K), float(np.float32(-np.log(K))), dtype=torch.float32, device=PG.DEV)
    a = brainxai.fusion_shap(model, eeg, spec, "uniform", players="class", score="logprob", return_parts=True)
    b = brainxai.fusion_shap(model, eeg, spec, brainxai.FusionVotes(row, row.clone()), players="class", score="logprob", return_parts=True)
    assert torch.equal(_bits64(a.values), _bits64(b.values)) and torch.equal(_bits64(a.empty), _bits64(b.empty))
    assert a.background.e.shape == (1, K) and torch.equal(PG.bits(a.background.e), PG.bits(row))


def test_modality_importance():
    model, eeg, spec, bg, votes, bgv, head = _setup(6)
    res = brainxai.fusion_shap(model, eeg, spec, bgv, players="votes", class_idx="all", return_parts=True)
    for values, got in ((res.values, brainxai.modality_importance(res)), (res.modality[:, 0], brainxai.modality_importance(res.modality[:, 0]))):
        want = np.abs(values.cpu().numpy()).mean(0)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        # the values rounded to fp32 once (2^-24 each), an fp64 sum, one rounding of the mean
        assert np.abs(got.cpu().numpy() - want).max() <= 2.0 ** -22 * want.max()
