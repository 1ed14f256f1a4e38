"""GPU: TCAV -- bx_tcav_mean, bx_tcav_gram, bx_tcav_fit, bx_tcav_vectors, bx_tcav_sensitivity and bx_tcav_score through ctypes, and
``train_cavs`` / ``tcav`` end to end, against the numpy fp64 restatement (tests/tcav_ref.py), whose ridge is solved in the primal.

Bounds, with u = 2^-53.
  mean      bit for bit: the definition is a sequential fp64 sum in row order and one division, which numpy restates operation by operation.
  Gram      |G0 - ref| <= 2 (D + M) u sum_d |a_id - mean_d| |a_jd - mean_d| entry by entry.  Both sides centre with the same (bit-equal)
            mean, so the inputs of the dot products are the same numbers; a D-term dot product in any order carries at most
            D u sum |terms| to first order, once for the kernel (whose FMAs round less) and once for numpy's; the M is slack for the form
            the bound is stated in.  Symmetry is checked bit for bit.
  fit       tcav_ref.fit_tolerance = 16 (rows + D) u cond, cond = rows / ridge + 1 for ridge and 1 for the mean difference (derived
            there), relative: |w - w_ref| <= tol |w_ref| in the 2-norm (w from the kernel's beta through the centred activations),
            | |w| - |w_ref| | <= tol |w_ref|, |lambda - ref| <= tol ref, |decision - ref| <= tol (|w_ref| max_j |a_j - mean_fit| + 1).
            Accuracies exactly, after the reference's decision values are seen to stay 100 bounds away from the threshold.
  CAV       a unit vector stored in fp32: |v - v_ref| <= 2 tol + 2^-23 in the 2-norm (normalising doubles a relative error; 2^-24 per
            component for the storage, and as much again for the kernel's own fp64 sum and division); | |v| - 1 | <= 2^-23.
  S         from downloaded CAVs: |S - ref| <= 2 D u sum_d |g_d| |v_d|, as for the Gram matrix.  End to end, where the CAV itself
            carries its bound: |S - ref| <= (2 tol + 2^-23) |g|_2 (Cauchy-Schwarz).  Scores exactly, after the reference's |S| are seen
            to stay 100 bounds away from zero; the means of S within the bound of S.
The observed worst figures are printed by every test (-s) and recorded in DESIGN.md section 6, TCAV.

Shapes.  Gram: (M, D) in {(1,1), (3,1), (5,257), (33,4099), (130,8192)} -- one row, one feature, a partial chunk of 32 features, one and
several feature splits (D > 512), one and several 64-row tiles with an off-diagonal tile -- as plain Gaussians and as post-ReLU-like
rows max(z + 3.2, 0) (mean^2 / var about 10), fp32 and bf16.  Fit: n in {2, 3, 17, 256} examples per set (4 to 512 rows per problem: one
thread per row, the trailing update's 32 x 32 blocks partial and full), both classifiers, holdout 0 and 0.25."""
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import perturb_gpu as PG
from tests import tcav_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
CLASSIFIERS = {"ridge": L.BX_TCAV_RIDGE, "mean_difference": L.BX_TCAV_MEAN_DIFFERENCE}


def _code(t):
    return ops.bx_dtype(t.dtype)


def _host64(t):
    return t.detach().double().cpu().numpy()


def _mean_gram(A):
    """bx_tcav_mean and bx_tcav_gram on a device tensor [M,D] -> (mean fp64 [D], G0 fp64 [M,M]), pre-filled with NaN."""
    lib = L.load()
    M, D = A.shape
    mean = torch.full((D,), float("nan"), dtype=torch.float64, device=PG.DEV)
    G = torch.full((M, M), float("nan"), dtype=torch.float64, device=PG.DEV)
    L.check(lib.bx_tcav_mean(PG.p(A), PG.p(mean), M, D, _code(A), PG.stream()), "bx_tcav_mean")
    ws = torch.empty(max(lib.bx_tcav_gram_workspace(M, D), 16), dtype=torch.uint8, device=PG.DEV)
    L.check(lib.bx_tcav_gram(PG.p(A), PG.p(mean), PG.p(G), M, D, _code(A), PG.p(ws), ws.numel(), PG.stream()), "bx_tcav_gram")
    torch.cuda.synchronize()
    return mean, G


def _row_order_mean(A64):
    s = np.zeros(A64.shape[1])
    for i in range(A64.shape[0]):
        s = s + A64[i]
    return s / A64.shape[0]


@pytest.mark.parametrize("kind", ["gauss", "relu"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,D", [(1, 1), (3, 1), (5, 257), (33, 4099), (130, 8192)])
def test_mean_and_gram(M, D, dt, kind):
    z = O.seeded((M, D), 7 + M, "randn")
    A = (torch.clamp(z + 3.2, min=0.0) if kind == "relu" else z).to(dt).to(PG.DEV).contiguous()
    A64 = _host64(A)
    if kind == "relu" and M > 3:
        print(f"mean^2 / var of the rows: {float(A64.mean() ** 2 / A64.var()):.1f}")
    assert L.load().bx_tcav_gram_workspace(M, D) // (64 * 64 * 8 * (((M + 63) // 64) * ((M + 63) // 64 + 1) // 2)) == (1 if D <= 512 else -(-D // 512))
    mean, G = _mean_gram(A)
    want_mean = _row_order_mean(A64)
    assert np.array_equal(PG.np_bits(mean.cpu().numpy()), PG.np_bits(want_mean)), "mean: not the row-order fp64 sum"
    Xc = A64 - want_mean
    want, bound = Xc @ Xc.T, 2.0 * (D + M) * U * (np.abs(Xc) @ np.abs(Xc).T)
    got = G.cpu().numpy()
    assert not np.isnan(got).any(), "unwritten entries"
    err = np.abs(got - want)
    print(f"gram M={M} D={D} {dt} {kind}: worst |G0 - ref| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"worst relative to the diagonal scale {float(err.max() / max(np.abs(want).max(), 1e-300)):.1e}")
    assert (err <= bound).all()
    assert np.array_equal(PG.np_bits(got), PG.np_bits(got.T)), "G0 is not symmetric bit for bit"


def test_unsupported_sizes_are_refused():
    lib = L.load()
    a = torch.zeros(4, dtype=torch.float32, device=PG.DEV)
    d = torch.zeros(4, dtype=torch.float64, device=PG.DEV)
    assert lib.bx_tcav_mean(PG.p(a), PG.p(d), 8193, 1, L.BX_F32, PG.stream()) != 0
    assert lib.bx_tcav_mean(PG.p(a), PG.p(d), 1, (1 << 24) + 1, L.BX_F32, PG.stream()) != 0
    assert lib.bx_tcav_gram_workspace(8193, 4) == 0 and lib.bx_tcav_fit_workspace(1, 513) == 0
    assert lib.bx_tcav_score(PG.p(d), None, 1, 1, 33, PG.p(d), PG.p(d), PG.p(d), PG.p(a), PG.stream()) != 0
    assert lib.bx_tcav_sensitivity(PG.p(a), PG.p(a), PG.p(d), 2, 1, 1, 3, 4, L.BX_F32, PG.stream()) != 0     # rows 3..5 of 4


# ---- the fit -------------------------------------------------------------------------------------------------------------------------------
def _tables(Q, Rn, n, nh):
    problems, rows, labels, fit = X._tcav_problems(Q, Rn, n, nh)
    want = R.problems(Q, Rn)
    assert [tuple(p) for p in problems.tolist()] == [(q, r) for q, r, _, _ in want]
    for (_, _, sp, sn), row in zip(want, rows):
        assert row.tolist() == list(range(sp * n, sp * n + n)) + list(range(sn * n, sn * n + n))
    return problems, rows, labels, fit


def _fit(G0, rows, labels, fit, classifier, ridge, fill=float("nan")):
    """bx_tcav_fit on a host G0 -> dict of host arrays; every output is pre-filled with ``fill``."""
    lib = L.load()
    M, (P, NI) = G0.shape[0], rows.shape
    nf = int(fit[0].sum())
    G = PG.dev(G0)
    o = dict(beta=torch.full((P, M), fill, dtype=torch.float64, device=PG.DEV), norm=torch.full((P,), fill, dtype=torch.float64, device=PG.DEV),
             lam=torch.full((P,), fill, dtype=torch.float64, device=PG.DEV), decision=torch.full((P, NI), fill, dtype=torch.float64, device=PG.DEV),
             acc=torch.full((P, 2), fill, dtype=torch.float64, device=PG.DEV), status=torch.full((P,), -7, dtype=torch.int32, device=PG.DEV))
    ws = torch.empty(lib.bx_tcav_fit_workspace(P, nf), dtype=torch.uint8, device=PG.DEV)
    counts = torch.full((P,), NI, dtype=torch.int32, device=PG.DEV)
    rows_d, labels_d, fit_d = PG.dev(rows), PG.dev(labels), PG.dev(fit)
    L.check(lib.bx_tcav_fit(PG.p(G), M, PG.p(rows_d), PG.p(labels_d), PG.p(fit_d), PG.p(counts), P, NI, nf, CLASSIFIERS[classifier], ridge,
                            PG.p(ws), ws.numel(), PG.p(o["beta"]), PG.p(o["norm"]), PG.p(o["lam"]), PG.p(o["status"]), PG.p(o["decision"]), PG.p(o["acc"]),
                            PG.stream()), "bx_tcav_fit")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _relu_sets(n, D, count, seed):
    rng = np.random.default_rng(seed)
    return [(np.maximum(rng.standard_normal((n, D)) + 3.2, 0.0) + 0.5 * rng.standard_normal(D)).astype(np.float32).astype(np.float64) for _ in range(count)]


def _check_fit(got, ref, Ac, rows, D, what):
    """One problem's outputs against the primal reference (rows: its fit rows); returns the worst deviation / bound."""
    assert got["status"] == 0, f"{what}: status {got['status']}"
    tol = R.fit_tolerance(ref["rows"], D, ref["cond_bound"])
    dec_tol = tol * (ref["norm"] * ref["radius"] + 1.0)
    assert np.abs(ref["decision"]).min() > 100 * dec_tol, f"{what}: a reference decision value within 100 bounds of the threshold"
    w = got["beta"] @ Ac
    assert abs(got["beta"].sum()) <= tol * np.abs(got["beta"]).sum() and not got["beta"][np.setdiff1d(np.arange(Ac.shape[0]), rows)].any(), what
    figs = [np.sqrt(((w - ref["w"]) ** 2).sum()) / ref["norm"] / tol, abs(got["norm"] - ref["norm"]) / ref["norm"] / tol,
            np.abs(got["decision"] - ref["decision"]).max() / dec_tol]
    if ref["lam"] > 0:
        figs.append(abs(got["lam"] - ref["lam"]) / ref["lam"] / tol)
    else:
        assert got["lam"] == 0.0
    assert max(figs) <= 1.0, f"{what}: deviation / bound {figs}"
    assert got["acc"][0] == ref["accuracy"], what
    assert got["acc"][1] == ref["holdout_accuracy"] or (np.isnan(got["acc"][1]) and np.isnan(ref["holdout_accuracy"])), what
    return max(figs)


@pytest.mark.parametrize("holdout", [0.0, 0.25])
@pytest.mark.parametrize("classifier", ["ridge", "mean_difference"])
@pytest.mark.parametrize("n", [2, 3, 17, 256])
def test_fit_against_primal(n, classifier, holdout):
    D, Q, Rn = 300, 1, 2
    sets = _relu_sets(n, D, Q + Rn, 40 + n)
    A = np.concatenate(sets)
    Ac = A - A.mean(axis=0)
    _, rows, labels, fit = _tables(Q, Rn, n, R.held_out(n, holdout))
    got = _fit(Ac @ Ac.T, rows, labels, fit, classifier, 1e-2)
    refs = R.fit_all(sets, Q, classifier, 1e-2, holdout)
    worst = max(_check_fit({k: v[p] for k, v in got.items()}, ref, Ac, rows[p][fit[p] == 1], D, f"n={n} {classifier} h={holdout} problem {p}") for p, ref in enumerate(refs))
    print(f"fit n={n} {classifier} holdout={holdout}: worst deviation / bound {worst:.3g} (bound {R.fit_tolerance(refs[0]['rows'], D, refs[0]['cond_bound']):.2e})")


def test_fit_status_and_the_raise():
    n, D = 5, 40
    rng = np.random.default_rng(3)
    one = np.repeat(rng.standard_normal((1, D)), n, axis=0)
    other, third = rng.standard_normal((n, D)), rng.standard_normal((n, D))
    # ridge: the concept and random set 0 hold one example n times (tr K = 0); random set 1 differs
    A = np.concatenate([one, one, third])
    Ac = A - A.mean(axis=0)
    _, rows, labels, fit = _tables(1, 2, n, 0)
    got = _fit(Ac @ Ac.T, rows, labels, fit, "ridge", 1e-2)
    assert got["status"].tolist() == [1, 0, 0, 0]
    # mean difference: random set 0 repeats the concept's examples (w = 0)
    A = np.concatenate([other, other, third])
    Ac = A - A.mean(axis=0)
    got2 = _fit(Ac @ Ac.T, rows, labels, fit, "mean_difference", 1e-2)
    assert got2["status"].tolist() == [2, 0, 0, 0]
    for g in (got, got2):
        for p in (0,):                                               # a problem with a status leaves every output as it was
            assert np.isnan(g["beta"][p]).all() and np.isnan(g["norm"][p]) and np.isnan(g["lam"][p]) and np.isnan(g["decision"][p]).all() and np.isnan(g["acc"][p]).all()
        for p in (1, 2, 3):
            assert not np.isnan(g["beta"][p]).any() and g["norm"][p] > 0 and not np.isnan(g["decision"][p]).any()
    model = _spec_model()
    x = O.seeded((n, 4, 32, 64), 5, "rand").to(PG.DEV)
    y = O.seeded((n, 4, 32, 64), 6, "rand").to(PG.DEV)
    state = PG.model_state(model)
    with pytest.raises(RuntimeError, match="concept 'same' against random set 0 cannot be separated at spectrogram_model.block3.*w = 0"):
        brainxai.train_cavs(model, {"same": x}, [x.clone(), y], target_layer="block3", classifier="mean_difference")
    with pytest.raises(RuntimeError, match=r"concept 'flat' against random set 1 cannot be separated.*tr K = 0"):
        brainxai.train_cavs(model, {"flat": x[:1].expand(n, -1, -1, -1)}, [y, x[:1].expand(n, -1, -1, -1).clone()], target_layer="block3")
    assert PG.model_state(model) == state


# ---- vectors, sensitivity, score ------------------------------------------------------------------------------------------------------------
def _pipeline(sets32, Q, classifier, holdout, dt=torch.float32):
    """mean, Gram, fit and vectors on the device from fp32 host sets -> (A on the device, fit outputs, V fp32 host, refs, D)."""
    lib = L.load()
    n, D = sets32[0].shape
    A = PG.dev(np.concatenate(sets32)).to(dt).contiguous()
    mean, G = _mean_gram(A)
    Rn = len(sets32) - Q
    _, rows, labels, fit = _tables(Q, Rn, n, R.held_out(n, holdout))
    got = _fit(G.cpu().numpy(), rows, labels, fit, classifier, 1e-2)
    assert not got["status"].any()
    P = rows.shape[0]
    V = torch.full((P, D), float("nan"), dtype=torch.float32, device=PG.DEV)
    beta_d, norm_d, status_d = PG.dev(got["beta"]), PG.dev(got["norm"]), PG.dev(got["status"])
    L.check(lib.bx_tcav_vectors(PG.p(A), PG.p(mean), PG.p(beta_d), PG.p(norm_d), PG.p(status_d), PG.p(V), A.shape[0], D, P, _code(A), PG.stream()),
            "bx_tcav_vectors")
    torch.cuda.synchronize()
    sets64 = [_host64(A[s * n:(s + 1) * n]) for s in range(len(sets32))]
    return A, mean, got, V, R.fit_all(sets64, Q, classifier, 1e-2, holdout), rows


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("classifier", ["ridge", "mean_difference"])
def test_vectors_sensitivity_score(classifier, dt):
    lib = L.load()
    n, D, Q, Rn, K = 17, 1003, 2, 3, 4
    sets32 = [s.astype(np.float32) for s in _relu_sets(n, D, Q + Rn, 11)]
    A, mean, got, V, refs, rows = _pipeline(sets32, Q, classifier, 0.25, dt)
    P = V.shape[0]
    Vh = V.cpu().numpy()
    assert not np.isnan(Vh).any(), "unwritten CAV entries"
    # the CAVs from the downloaded dual coefficients, and against the primal reference
    Ac = _host64(A) - mean.cpu().numpy()
    for p, ref in enumerate(refs):
        want = got["beta"][p] @ Ac / got["norm"][p]
        slack = 2.0 ** -24 * np.abs(want) + 4 * rows.shape[1] * U * (np.abs(got["beta"][p]) @ np.abs(Ac)) / got["norm"][p]
        assert (np.abs(Vh[p] - want) <= slack).all()
        vb = 2 * R.fit_tolerance(ref["rows"], D, ref["cond_bound"]) + 2.0 ** -23
        assert abs(np.sqrt((Vh[p].astype(np.float64) ** 2).sum()) - 1.0) <= 2.0 ** -23
        assert np.sqrt(((Vh[p] - ref["v"]) ** 2).sum()) <= vb
    # a problem with a status keeps its row
    V2 = torch.full((P, D), 7.0, dtype=torch.float32, device=PG.DEV)
    st = torch.zeros(P, dtype=torch.int32, device=PG.DEV)
    st[1] = 3
    beta_d, norm_d = PG.dev(got["beta"]), PG.dev(got["norm"])
    L.check(lib.bx_tcav_vectors(PG.p(A), PG.p(mean), PG.p(beta_d), PG.p(norm_d), PG.p(st), PG.p(V2), A.shape[0], D, P, _code(A), PG.stream()), "bx_tcav_vectors")
    assert torch.equal(V2[1], torch.full((D,), 7.0, device=PG.DEV)) and torch.equal(PG.bits(V2[0]), PG.bits(V[0])) and torch.equal(PG.bits(V2[2:]), PG.bits(V[2:]))
    # sensitivities of 11 gradient rows written at row 3 of 16: in one call and cut into chunks, the same bits
    rows_total, row0, nr = 16, 3, 11
    G = (O.seeded((nr, D), 21, "randn") * torch.where(O.seeded((nr, D), 22, "rand") < 0.3, 0.0, 1.0)).to(dt).to(PG.DEV).contiguous()
    S = torch.full((rows_total, P), float("nan"), dtype=torch.float64, device=PG.DEV)
    L.check(lib.bx_tcav_sensitivity(PG.p(G), PG.p(V), PG.p(S), nr, D, P, row0, rows_total, _code(G), PG.stream()), "bx_tcav_sensitivity")
    S2 = torch.full_like(S, float("nan"))
    for a, b in ((0, 1), (1, 6), (6, 11)):
        L.check(lib.bx_tcav_sensitivity(PG.p(G[a:b]), PG.p(V), PG.p(S2), b - a, D, P, row0 + a, rows_total, _code(G), PG.stream()), "bx_tcav_sensitivity")
    torch.cuda.synchronize()
    Sh = S.cpu().numpy()
    assert np.isnan(Sh[:row0]).all() and np.isnan(Sh[row0 + nr:]).all(), "rows outside the window were written"
    assert np.array_equal(PG.np_bits(Sh), PG.np_bits(S2.cpu().numpy())), "the sensitivities depend on how the rows are cut"
    G64 = _host64(G)
    want = R.sensitivities(G64, Vh)
    bound = 2.0 * D * U * (np.abs(G64) @ np.abs(Vh.astype(np.float64)).T)
    err = np.abs(Sh[row0:row0 + nr] - want)
    print(f"sensitivity {classifier} {dt}: worst |S - ref| / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert (np.abs(want) > 100 * bound).all(), "a reference sensitivity within 100 bounds of zero: choose another seed"
    # scores: per-row classes with an empty class (class 2), and every row for every class
    classes = np.array([0, 1, 3, 3, 0, 1, 1, 0, 3, 0, 1], dtype=np.int32)
    for cls_d, cls_h, rws in ((PG.dev(classes), classes, nr), (None, np.arange(8) % K, 8)):
        Sd = PG.dev(np.ascontiguousarray(Sh[row0:row0 + rws]))
        outs = [torch.full((P, K), -5.0, dtype=torch.float64, device=PG.DEV) for _ in range(3)]
        counts = torch.full((K,), -5, dtype=torch.int32, device=PG.DEV)
        L.check(lib.bx_tcav_score(PG.p(Sd), PG.p(cls_d), rws, P, K, *(PG.p(t) for t in outs), PG.p(counts), PG.stream()), "bx_tcav_score")
        sc, mn, ma, cn = R.scores(want[:rws], cls_h, K)
        assert np.array_equal(outs[0].cpu().numpy(), sc, equal_nan=True) and counts.cpu().numpy().tolist() == cn.tolist()
        for o, w in ((outs[1], mn), (outs[2], ma)):
            assert np.array_equal(np.isnan(o.cpu().numpy()), np.isnan(w))
            assert np.nanmax(np.abs(o.cpu().numpy() - w)) <= 2 * float(bound.max())
        if cls_d is not None:
            assert np.isnan(sc[:, 2]).all() and cn[2] == 0


@pytest.mark.parametrize("n,D", [(3, 1), (8, 257), (20, 4099)])
@pytest.mark.parametrize("classifier", ["ridge", "mean_difference"])
def test_planted_concept(n, D, classifier):
    """The positives carry + c d: the kernel's CAV has the reference's cosine with d (which falls from 1.0 at D = 1 to about 0.14 at
    n = 20, D = 4099 -- no fixed threshold)."""
    sets, d = R.planted(n, D, 3.0, 50 + n, sets=3)
    sets32 = [s.astype(np.float32) for s in sets]
    _, _, _, V, refs, _ = _pipeline(sets32, 1, classifier, 0.0)
    Vh = V.cpu().numpy().astype(np.float64)
    for p in (0, 1):
        vb = 2 * R.fit_tolerance(refs[p]["rows"], D, refs[p]["cond_bound"]) + 2.0 ** -23
        cos, want = float(Vh[p] @ d), float(refs[p]["v"] @ d)
        print(f"planted n={n} D={D} {classifier} random set {p}: cosine {cos:.6f}, reference {want:.6f}, bound {vb:.1e}")
        assert abs(cos - want) <= vb and want > 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mm_model():
    ref = O.fill_params(O.build_multimodal(5, 512, 4, dropout=0.0), seed=42).eval()
    with torch.no_grad():
        ref.spectrogram_model.fc.weight *= 0.05
        ref.eeg_model.dense.weight *= 0.05
        ref.fc2.weight *= 0.5
    mine = brainxai.build_multimodal(5, 512, 4, dropout=0.0)
    mine.load_state_dict(ref.state_dict())
    return mine.to(PG.DEV).eval()


def _spec_model():
    return _mm_model().spectrogram_model


@functools.lru_cache(maxsize=None)
def _deep_model():
    torch.manual_seed(9)
    return brainxai.EEGNetAttentionDeep(6, Chans=5, Samples=512, dropoutRate=0.0).to(PG.DEV).eval()


B, NS, QN, RN = 5, 4, 2, 2
MODELS = {"mm": lambda: _mm_model(), "spec": _spec_model, "eegnet": lambda: _mm_model().eeg_model, "deep": _deep_model}
CASES = [("mm", "spec", "spectrogram_model.block5"), ("mm", "spec", "block3"), ("mm", "spec", "spectrogram_model.block2.conv2"),
         ("mm", "eeg", "eeg_model.features"), ("spec", "spec", "block3"), ("eegnet", "eeg", "features"), ("deep", "eeg", "eeg_model.features")]


def _inputs(inp):
    eeg, spec = O.seeded((B, 1, 5, 512), 12, "randn").to(PG.DEV), O.seeded((B, 4, 32, 64), 11, "rand").to(PG.DEV)
    shape, kind = ((NS, 4, 32, 64), "rand") if inp == "spec" else ((NS, 1, 5, 512), "randn")
    sets = [O.seeded(shape, 60 + s, kind).to(PG.DEV) for s in range(QN + RN)]
    if inp == "spec":
        sets[0][:, :, 8:16] += 0.5                                   # a band of the spectrogram: the first concept
        sets[1] = brainxai.gaussian_blur(sets[1], 2.0)               # a smoothed one: the second
    else:
        t = torch.arange(512, device=PG.DEV) / 200.0
        sets[0] += torch.sin(2 * np.pi * 10.0 * t)                   # alpha rhythm on every electrode
        sets[1] += 2.0 * torch.sin(2 * np.pi * 2.0 * t)              # delta slowing
    return eeg, spec, {"first": sets[0], "second": sets[1]}, sets[QN:]


def _capture(model, kind, inp, target, eeg, spec, sets, seeds):
    """Activations of the example sets and gradients of the test samples at the target, from the package's own forward and backward
    (explain._SpecTarget / ops.eeg_features_keep, one backward pass per one-hot seed [B,K]) -> (acts fp64 [sets][n,D], out, grads per seed)."""
    multimodal = kind == "mm"
    with X._eval_frozen(model):
        if inp == "spec":
            net = model.spectrogram_model if multimodal else model
            m = X._TARGET.match(target)
            blk, conv_k = getattr(net, f"block{m.group(1)}"), int(m.group(2) or 0)
            acts = []
            with torch.no_grad(), X._SpecTarget(blk, conv_k) as tgt:
                for s in sets:
                    net(s)
                    acts.append(_host64(tgt.act()).reshape(s.shape[0], -1))
            x = spec.clone().requires_grad_(True)
            with X._SpecTarget(blk, conv_k, want_input=True) as tgt:
                out = model(eeg, x) if multimodal else net(x)
                grads = [_host64(tgt.grad(torch.autograd.grad(out, tgt.leaf, grad_outputs=sd, retain_graph=True)[0])).reshape(B, -1) for sd in seeds(out)]
        else:
            net = model.eeg_model if multimodal else model
            with torch.no_grad():
                acts = [_host64(ops.eeg_features_keep(net, s)[0]) for s in sets]
                feat = ops.eeg_features_keep(net, eeg)[0]
                s_out = model.spectrogram_model(spec) if multimodal else None
            f = feat.detach().requires_grad_(True)
            with torch.enable_grad():
                out = X._eeg_head(net, f)
                if multimodal:
                    out = ops.FusionHeadFn.apply(out, s_out, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)
            grads = [_host64(torch.autograd.grad(out, f, grad_outputs=sd, retain_graph=True)[0]) for sd in seeds(out)]
    return acts, out.detach().float(), grads


def _seeds_for(class_idx, K):
    def seeds(out):
        if isinstance(class_idx, str):
            cls = [torch.full((B,), k, device=PG.DEV) for k in range(K)]
        elif class_idx is None:
            cls = [out.detach().argmax(dim=1)]
        else:
            cls = [torch.as_tensor(class_idx, device=PG.DEV).expand(B) if isinstance(class_idx, int) else torch.as_tensor(class_idx, device=PG.DEV)]
        return [torch.nn.functional.one_hot(c.long(), K).float() for c in cls]
    return seeds


def _check_end_to_end(model, kind, inp, target, class_idx, classifier="ridge", holdout=0.0, what=""):
    eeg, spec, concepts, randoms = _inputs(inp)
    args = (model, eeg if kind in ("mm", "eegnet", "deep") else None, spec if kind in ("mm", "spec") else None)
    state = PG.model_state(model)
    res = brainxai.tcav(*args, concepts, randoms, input=inp, target_layer=target, classifier=classifier, holdout=holdout, class_idx=class_idx, return_parts=True)
    assert PG.model_state(model) == state
    K = res.out.shape[1]
    acts, out, grads = _capture(model, kind, inp, target, eeg, spec, list(concepts.values()) + randoms, _seeds_for(class_idx, K))
    assert torch.equal(PG.bits(out), PG.bits(res.out)), "the captured pass is not the driver's"
    D = acts[0].shape[1]
    refs = R.fit_all(acts, QN, classifier, 1e-2, holdout)
    P = len(refs)
    Vref = np.stack([f["v"] for f in refs])
    Vh = res.cavs.vectors.cpu().numpy().astype(np.float64)
    vb = np.array([2 * R.fit_tolerance(f["rows"], D, f["cond_bound"]) + 2.0 ** -23 for f in refs])
    assert res.cavs.vectors.shape == (P, D) and int(np.prod(res.cavs.shape)) == D and res.cavs.vector("second", 1).shape == tuple(res.cavs.shape)
    dv = np.sqrt(((Vh - Vref) ** 2).sum(axis=1))
    assert (dv <= vb).all(), f"{what}: CAVs off by {dv / vb} bounds"
    assert np.array_equal(res.cavs.accuracy.cpu().numpy(), np.array([f["accuracy"] for f in refs]))
    assert np.array_equal(res.cavs.holdout_accuracy.cpu().numpy(), np.array([f["holdout_accuracy"] for f in refs]), equal_nan=True)
    assert np.abs(res.cavs.norms.cpu().numpy() / np.array([f["norm"] for f in refs]) - 1).max() <= vb.max()
    if isinstance(class_idx, str):
        G, classes = np.stack(grads, axis=1).reshape(B * K, D), np.arange(B * K) % K
        assert res.classes is None and res.sensitivity.shape == (B, K, P)
    else:
        G = grads[0]
        classes = out.argmax(dim=1).cpu().numpy() if class_idx is None else np.broadcast_to(np.asarray(class_idx), (B,))
        assert res.classes.cpu().numpy().tolist() == classes.tolist() and res.sensitivity.shape == (B, P)
    Sref = R.sensitivities(G, Vref)
    sb = np.sqrt((G * G).sum(axis=1))[:, None] * vb[None, :]
    err = np.abs(res.sensitivity.cpu().numpy().reshape(-1, P) - Sref)
    print(f"{what}: D = {D}, worst |v - ref| / bound {float((dv / vb).max()):.3f}, worst |S - ref| / bound {float((err / np.maximum(sb, 1e-300)).max()):.3f}, "
          f"smallest |S_ref| / bound {float((np.abs(Sref) / np.maximum(sb, 1e-300)).min()):.0f}")
    assert (np.abs(Sref) > 100 * sb).all(), f"{what}: a reference sensitivity within 100 bounds of zero: choose other seeds"
    assert (err <= sb).all()
    sc, mn, ma, cn = R.scores(Sref, classes, K)
    assert res.counts.cpu().numpy().tolist() == cn.tolist()
    assert np.array_equal(res.scores_per_random.cpu().numpy(), sc[:QN * RN].reshape(QN, RN, K), equal_nan=True)
    assert np.array_equal(res.null_scores.cpu().numpy(), sc[QN * RN:], equal_nan=True)
    assert np.array_equal(res.scores.cpu().numpy(), sc[:QN * RN].reshape(QN, RN, K).sum(axis=1) / RN, equal_nan=True)
    for o, w in ((res.mean_sensitivity, mn), (res.mean_abs_sensitivity, ma)):
        got = o.cpu().numpy().reshape(QN * RN, K)
        assert np.array_equal(np.isnan(got), np.isnan(w[:QN * RN])) and (np.isnan(got) | (np.abs(got - w[:QN * RN]) <= sb.max())).all()
    for q in range(QN):
        for k in range(K):
            want = R.welch(sc[q * RN:(q + 1) * RN, k], sc[QN * RN:, k])
            got = (float(res.t[q, k]), float(res.dof[q, k]), float(res.p_value[q, k]))
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)
    return res, args, concepts, randoms


@pytest.mark.parametrize("class_idx", [None, 2, [0, 5, 1, 1, 3], "all"], ids=["argmax", "int", "list", "all"])
@pytest.mark.parametrize("kind,inp,target", CASES, ids=[f"{k}-{t}" for k, _, t in CASES])
def test_tcav_end_to_end(kind, inp, target, class_idx):
    _check_end_to_end(MODELS[kind](), kind, inp, target, class_idx, what=f"{kind} {target} class_idx={class_idx!r}")


@pytest.mark.parametrize("kind,inp,target", [CASES[1], CASES[3]], ids=["spec", "eeg"])
def test_tcav_options_and_invariances(kind, inp, target):
    model = MODELS[kind]()
    res, args, concepts, randoms = _check_end_to_end(model, kind, inp, target, "all", "mean_difference", 0.25, what=f"{kind} {target} mean difference, holdout")
    kw = dict(input=inp, target_layer=target, classifier="mean_difference", holdout=0.25, class_idx="all")
    plain = brainxai.tcav(*args, concepts, randoms, **kw)
    assert torch.equal(plain.view(torch.int64), res.scores.view(torch.int64)) and plain.shape == (QN, res.out.shape[1])
    cavs = brainxai.train_cavs(model, concepts, randoms, input=inp, target_layer=target, classifier="mean_difference", holdout=0.25, keep_gram=True)
    assert cavs.gram.shape == ((QN + RN) * NS,) * 2 and torch.equal(cavs.gram, cavs.gram.T)
    assert cavs.decision.shape == (QN * RN + RN, 2 * NS) and cavs.problems.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [-1, 0], [-1, 1]]
    assert cavs.names == ["first", "second"] and cavs.target_layer == ("spectrogram_model.block3" if inp == "spec" else "eeg_model.features")
    again = brainxai.tcav(*args, cavs=cavs, input=inp, class_idx="all", return_parts=True)
    for a, b in ((again.cavs.vectors, res.cavs.vectors), (again.sensitivity, res.sensitivity), (again.scores, res.scores), (again.p_value, res.p_value)):
        assert torch.equal(PG.bits(a) if a.dtype != torch.float64 else a.view(torch.int64), PG.bits(b) if b.dtype != torch.float64 else b.view(torch.int64))
    for mb in (1, 3, 256):                                           # no bit depends on max_batch
        r = brainxai.tcav(*args, concepts, randoms, max_batch=mb, return_parts=True, **kw)
        assert torch.equal(PG.bits(r.cavs.vectors), PG.bits(res.cavs.vectors)), f"max_batch={mb}: the CAVs differ"
        assert torch.equal(r.sensitivity.view(torch.int64), res.sensitivity.view(torch.int64)), f"max_batch={mb}: the sensitivities differ"
        assert torch.equal(r.scores.view(torch.int64), res.scores.view(torch.int64)) and torch.equal(PG.bits(r.out), PG.bits(res.out))
    # the examples of every set in another order: the same classifiers up to rounding, the same scores
    perm = torch.tensor([2, 0, 3, 1], device=PG.DEV)
    r = brainxai.tcav(*args, {k: v[perm] for k, v in concepts.items()}, [v[perm] for v in randoms], input=inp, target_layer=target, class_idx="all", return_parts=True)
    base = brainxai.tcav(*args, concepts, randoms, input=inp, target_layer=target, class_idx="all", return_parts=True)
    D = base.cavs.vectors.shape[1]
    vb = 2 * (2 * R.fit_tolerance(2 * NS, D, 2 * NS / 1e-2 + 1) + 2.0 ** -23)
    dv = (r.cavs.vectors.double() - base.cavs.vectors.double()).norm(dim=1)
    print(f"{kind} {target}: permuted examples move the CAVs by {float(dv.max()):.2e} (bound {vb:.2e})")
    assert float(dv.max()) <= vb and torch.equal(r.scores, base.scores) and torch.equal(r.scores_per_random, base.scores_per_random)


def test_tcav_bf16_storage():
    model = brainxai.set_compute_dtype(_mm_model(), torch.bfloat16)
    try:
        res, *_ = _check_end_to_end(model, "mm", "spec", "block3", None, what="mm block3 bf16 storage")
        _check_end_to_end(model, "mm", "spec", "spectrogram_model.block2.conv2", "all", what="mm block2.conv2 bf16 storage")
    finally:
        brainxai.set_compute_dtype(model, torch.float32)
