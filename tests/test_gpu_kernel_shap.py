"""GPU: brainxai.kernel_shap and the bx_shap_* entry points against the restatement of the definition (tests/kernel_shap_ref.py):
perturbed rows bit for bit, the fit against numpy fp64 and brute-force Shapley values, and the values end to end against the oracle's
classes run in fp64 on the CPU with the same coalitions, on the models and inputs of tests/perturb_gpu.py.

Bounds.  bx_shap_fit alone: (M + N) 2^-52 kappa(Xt' W Xt) max|phi_ref| per case -- the textbook bound of a Cholesky solve with the
length of the Gram sums added; kappa is computed by the test.  End to end, fp32 storage: |scores - ref| <= 1e-5, the project's
probability bound (TOL of tests/perturb_gpu.py), and |values - ref| <= amp 1e-5 with amp the largest absolute row sum of the fit's
solution operator (the columns of clean and empty included; computed in numpy): the fit is linear in the scores.  Every compared case
passes the guard of tests/perturb_gpu.py first.  Additivity: |sum_m values - (clean - empty)| <= 2^-50 sum_m |values|, the sum taken
exactly (math.fsum).  bf16 storage: amp x BF16_LOGP x the log-probability scale (tests/perturb_gpu.py), the bound applied to the scores.
Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import kernel_shap_ref as R
from tests import perturb_gpu as PG
from tests.perturb_gpu import DEV, TOL

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _random_map(Hm, Wm, M, seed):
    """A seeded label map with every label present."""
    seg = np.random.default_rng(seed).integers(0, M, size=Hm * Wm).astype(np.int32)
    seg[:M] = np.arange(M)
    return seg.reshape(Hm, Wm)


# ---- 1. perturbed spectrogram rows, bit for bit ---------------------------------------------------------------------------------------------
# channels, H, W, label map, coalitions
SPEC_SHAPES = {"2x16x24 grid 2x3": (2, 16, 24, lambda: R.grid_segments(16, 24, 2, 3), lambda: R.coalition_set(6, 62)[0]),
               "3x100x75 random M=37": (3, 100, 75, lambda: _random_map(100, 75, 37, 1), lambda: R.coalition_set(37, 96)[0]),
               "4x64x128 random M=33": (4, 64, 128, lambda: _random_map(64, 128, 33, 2), lambda: R.coalition_set(33, 20)[0]),
               "4x64x128 random M=64": (4, 64, 128, lambda: _random_map(64, 128, 64, 3), lambda: R.coalition_set(64, 20)[0]),
               "4x64x128 random M=65": (4, 64, 128, lambda: _random_map(64, 128, 65, 4), lambda: R.coalition_set(65, 20)[0])}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(SPEC_SHAPES))
def test_perturbed_spectrogram_rows_bit_for_bit(shape, kind, dt):
    C, H, W, seg_of, Z_of = SPEC_SHAPES[shape]
    B = 2
    seg, Z = seg_of(), Z_of()
    N, M = Z.shape
    assert np.array_equal(np.unique(seg), np.arange(M))
    if shape == "2x16x24 grid 2x3":
        assert N == 62 and np.array_equal(X._shap_segments("kernel_shap", (2, 3), "spec", H, W)[0], seg)
    x, base, bkind, base_d = PG.row_inputs((B, C, H, W), kind)
    m = R.masks(seg, Z)
    assert m[:, seg == M - 1].any() and (~m[:, seg == M - 1]).any(), "the last player is shown in some rows and hidden in others"
    x_d, seg_d, Z_d = x.to(DEV), PG.dev(seg), PG.dev(Z)

    def launch(out, n0, n):
        L.check(L.load().bx_shap_perturb_spec(PG.p(x_d), PG.p(base_d), bkind, PG.p(out), B, C, H, W, 8, PG.p(seg_d), PG.p(Z_d), M, N, n0, n, ops.bx_dtype(dt), PG.stream()),
                "bx_shap_perturb_spec")
    PG.check_spec_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, PG.row_windows(N),
                       lambda b0, nb, n0, n: X._shap_perturb(x_d, seg_d, Z_d, M, base_d, bkind, b0, nb, n0, n, dt), dt, f"{shape} {kind}")


# ---- 2. perturbed EEG rows, bit for bit -----------------------------------------------------------------------------------------------------
# electrodes, T, label map ([Chans,T] or [1,T]), coalitions
EEG_SHAPES = {"5x333 random M=11": (5, 333, lambda: _random_map(5, 333, 11, 5), lambda: R.coalition_set(11, 30)[0]),
              "19x2000 electrodes": (19, 2000, lambda: np.arange(19, dtype=np.int32)[:, None].repeat(2000, 1), lambda: R.coalition_set(19, 64)[0]),
              "37x3000 time 8": (37, 3000, lambda: R.grid_segments(1, 3000, 1, 8), lambda: R.coalition_set(8, 20)[0])}


@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(EEG_SHAPES))
def test_perturbed_eeg_rows_bit_for_bit(shape, kind):
    chans, T, seg_of, Z_of = EEG_SHAPES[shape]
    B = 2
    seg, Z = seg_of(), Z_of()
    N, M = Z.shape
    map_rows = seg.shape[0]
    assert np.array_equal(np.unique(seg), np.arange(M)) and map_rows in (1, chans)
    named = {"19x2000 electrodes": "electrodes", "37x3000 time 8": ("time", 8)}.get(shape)
    if named is not None:
        assert np.array_equal(X._shap_segments("kernel_shap", named, "eeg", chans, T)[0], seg)
    x, base, bkind, base_d = PG.row_inputs((B, 1, chans, T), kind)
    m = R.masks(seg, Z)
    x_d, seg_d, Z_d = x.to(DEV), PG.dev(seg), PG.dev(Z)

    def launch(out, n0, n):
        L.check(L.load().bx_shap_perturb_eeg(PG.p(x_d), PG.p(base_d), bkind, PG.p(out), B, chans, T, map_rows, PG.p(seg_d), PG.p(Z_d), M, N, n0, n, PG.stream()),
                "bx_shap_perturb_eeg")
    PG.check_eeg_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, PG.row_windows(N),
                      lambda b0, nb, n0, n: X._shap_perturb(x_d, seg_d, Z_d, M, base_d, bkind, b0, nb, n0, n, torch.float32, map_rows), f"{shape} {kind}")


# ---- 3. the fit alone -----------------------------------------------------------------------------------------------------------------------
def _fit(S_d, clean_d, empty_d, cls_d, Z_d, w_d, fill=7.0):
    """-> (phi fp64 [B,R,M] numpy, info): bx_shap_fit on a pre-filled phi."""
    lib = L.load()
    B, N, K = S_d.shape
    M = Z_d.shape[1]
    nbytes = lib.bx_shap_fit_workspace(B, N, K, M, 1 if cls_d is None else 0)
    assert nbytes > 0
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    phi = torch.full((B, K if cls_d is None else 1, M), fill, dtype=torch.float64, device=DEV)
    info = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    L.check(lib.bx_shap_fit(PG.p(S_d), PG.p(clean_d), PG.p(empty_d), PG.p(cls_d), PG.p(Z_d), PG.p(w_d), B, N, K, M, PG.p(ws), nbytes, PG.p(phi), PG.p(info),
                            PG.stream()), "bx_shap_fit")
    torch.cuda.synchronize()
    return phi.cpu().numpy(), int(info.item())


# players, budget of coalitions (seed 0)
FIT = {"M=2 exact": (2, 2), "M=6 exact": (6, 62), "M=19 N=64": (19, 64), "M=37 N=96": (37, 96), "M=256 N=1024": (256, 1024)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", sorted(FIT))
def test_fit_against_numpy_fp64(case, B):
    M, budget = FIT[case]
    K = 6
    Z, w, exact = R.coalition_set(M, budget, seed=0)
    N = Z.shape[0]
    assert exact == case.endswith("exact") and N == budget
    g = np.random.default_rng(1000 * M + B)
    S, clean, empty = (g.random(s).astype(np.float32) for s in ((B, N, K), (B, K), (B, K)))
    classes = g.integers(0, K, size=B).astype(np.int32)
    want = R.values(Z, w, S, clean, empty)                          # [B,K,M], the normal equations
    kappa = R.gram_cond(Z, w)
    bound = (M + N) * EPS * kappa * np.abs(want).max()
    S_d, clean_d, empty_d, Z_d, w_d = (PG.dev(a) for a in (S, clean, empty, Z, w))
    got, info = _fit(S_d, clean_d, empty_d, None, Z_d, w_d)
    assert info == 0 and got.shape == (B, K, M) and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    got_c, info_c = _fit(S_d, clean_d, empty_d, PG.dev(classes), Z_d, w_d)
    sel = np.arange(B)
    assert info_c == 0 and got_c.shape == (B, 1, M) and np.array_equal(got_c[:, 0].view(np.int64), got[sel, classes].view(np.int64))
    lstsq = float(np.abs(R.values(Z, w, S, clean, empty, "lstsq") - want).max())
    print(f"bx_shap_fit {case} B={B}: kappa {kappa:.3g} max|phi| {np.abs(want).max():.3g} |fit - normal equations| {err:.2e} (bound {bound:.2e}; numpy's lstsq "
          f"differs from them by {lstsq:.2e})")
    assert err <= bound
    delta = clean.astype(np.float64) - empty.astype(np.float64)
    add = max(abs(math.fsum(got[b, k]) - delta[b, k]) / np.abs(got[b, k]).sum() for b in range(B) for k in range(K))
    assert add <= 2.0 ** -50, f"sum of the values misses clean - empty by {add:.1e} of sum |values|"
    if exact:
        idx = R.coalition_index(Z)
        for b in range(B):
            for k in range(K):
                v = np.zeros(2 ** M)
                v[idx], v[0], v[-1] = S[b, :, k], empty[b, k], clean[b, k]
                assert np.abs(got[b, k] - R.brute_force(M, v)).max() <= bound, "exact set: the brute-force Shapley values"
    again, _ = _fit(S_d, clean_d, empty_d, None, Z_d, w_d, fill=-3.0)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two runs agree bit for bit"


def test_fit_refuses_a_rank_deficient_set():
    """Two players that always appear together cannot be told apart: Xt' W Xt is exactly singular, a pivot vanishes."""
    M, N, K = 8, 40, 6
    Z = R.coalition_set(M, N, seed=3)[0].copy()
    Z[:, 5] = Z[:, 2]
    Z = Z[(Z.sum(1) > 0) & (Z.sum(1) < M)]
    N = Z.shape[0]
    assert N >= M - 1 and np.linalg.matrix_rank(R.reduced(Z, np.ones(N))[2]) == M - 2
    g = np.random.default_rng(0)
    S, clean, empty = (PG.dev(g.random(s).astype(np.float32)) for s in ((2, N, K), (2, K), (2, K)))
    phi, info = _fit(S, clean, empty, None, PG.dev(Z), PG.dev(np.ones(N)))
    print(f"bx_shap_fit rank-deficient set: info {info}")
    assert info == 6 and (phi == 7.0).all(), "the pivot of the second twin (index 5) vanishes; phi stays untouched"
    with pytest.raises(ValueError, match="undetermined.*more samples"):
        X._shap_fit(S, clean, empty, None, PG.dev(Z), PG.dev(np.ones(N)))
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    with pytest.raises(ValueError, match="undetermined.*more samples"):
        brainxai.kernel_shap(mine, eeg, spec, segments=(2, 4), coalitions=(Z, None))


def test_value_map_is_the_gather():
    g = np.random.default_rng(2)
    for Hm, Wm, M, B, Rr in [(16, 24, 6, 2, 1), (100, 75, 37, 3, 6), (1, 3000, 8, 2, 32), (19, 2000, 256, 1, 2)]:
        seg = _random_map(Hm, Wm, M, M)
        phi = g.standard_normal((B, Rr, M))
        out = torch.full((B, Rr, Hm, Wm), float("nan"), dtype=torch.float32, device=DEV)
        phi_d, seg_d = PG.dev(phi), PG.dev(seg)
        L.check(L.load().bx_shap_value_map(PG.p(phi_d), PG.p(seg_d), PG.p(out), B, Rr, Hm, Wm, M, PG.stream()), "bx_shap_value_map")
        assert np.array_equal(out.cpu().numpy(), phi.astype(np.float32)[:, :, seg])


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------------------
EEG_BASE = 1.0


def _head64(r64, e_out, s_out):
    return r64.log_softmax(r64.fc2(torch.relu(r64.fc1(torch.cat((e_out, s_out), dim=1)))))


@functools.lru_cache(maxsize=None)
def _reference(which):
    """(seg, Z, w, S, clean, empty) of the fp64 oracle; computed once, shared, never changed.  The branch whose input does not change is
    evaluated once per sample and repeated (eval mode: a row's output does not depend on the batch it is in).  Zero baseline, except for
    the EEG input of the multimodal model (EEG_BASE): against zeros, the mean of that input, the EEG branch moves the fused
    probability by 5e-3 only and the 19 values are too small for the guard at N = 64 (50 - 74 x the bound); against 1.0, one standard
    deviation, they move by 2e-2 (520 - 630 x)."""
    with torch.no_grad():
        if which in ("mm spec", "mm eeg"):
            ref_model, _ = PG.scaled_multimodal()
            eeg, spec = PG.mm_inputs()
            r64 = copy.deepcopy(ref_model).double()
            if which == "mm spec":
                seg, (Z, w, _) = R.grid_segments(64, 128, 2, 3), R.coalition_set(6, 2 * 6 + 2048)
                e_out = r64.eeg_model(eeg.double())
                x, f = spec, lambda xs: _head64(r64, e_out.repeat(xs.shape[0] // 3, 1), r64.spectrogram_model(xs))
            else:
                seg, (Z, w, _) = np.arange(19, dtype=np.int32)[:, None].repeat(2000, 1), R.coalition_set(19, 64)
                s_out = r64.spectrogram_model(spec.double())
                x, f = eeg, lambda xe: _head64(r64, r64.eeg_model(xe), s_out.repeat(xe.shape[0] // 3, 1))
            full = r64(eeg.double(), spec.double())
            assert float((f(x.double()) - full).abs().max()) <= 1e-12
        elif which == "spectrogram":
            ref_model, _ = PG.scaled_multimodal()
            n64 = copy.deepcopy(ref_model.spectrogram_model).double()
            seg, (Z, w, _) = R.grid_segments(64, 128, 3, 4), R.coalition_set(12, 40)
            x, f = PG.mm_inputs()[1], lambda xs: n64(xs)
        else:
            ref_model, _ = PG.eegnet_pair()
            n64 = copy.deepcopy(ref_model).double()
            seg, (Z, w, _) = R.grid_segments(1, 2000, 1, 6), R.coalition_set(6, 2 * 6 + 2048)
            x, f = O.seeded((3, 1, 19, 2000), 91, "randn"), lambda xe: n64(xe)
        S, clean, empty = R.scores(f, x.double(), R.masks(seg, Z), EEG_BASE if which == "mm eeg" else 0.0)
    return seg, Z, w, S, clean, empty


def _guarded(Z, w, S, clean, empty, cls, what, unit=TOL):
    """The fp64 reference values [B,K,M] and amp, with the guard on the reference side alone."""
    B, N = S.shape[0], S.shape[1]
    phi, amp = R.values(Z, w, S, clean, empty), R.amplification(Z, w)
    shuffled = R.values(Z, w, S[:, np.random.RandomState(1).permutation(N)], clean, empty)
    shown = f"amp {amp:.3g} kappa {R.gram_cond(Z, w):.3g} max|values| {[round(float(np.abs(phi[b, cls[b]]).max()), 4) for b in range(B)]}"
    PG.guard_moved(phi, shuffled, cls, amp * unit, what, shown, "values")
    return phi, amp


def _check(res, seg, Z, w, S, clean, empty, cls, what, all_classes=False):
    phi, amp = _guarded(Z, w, S, clean, empty, cls, what)
    B, M = S.shape[0], Z.shape[1]
    assert np.array_equal(res.coalitions, Z) and np.array_equal(res.weights, w) and np.array_equal(res.segments, seg)
    worst_s = max(float(np.abs(a.cpu().numpy().astype(np.float64) - r).max()) for a, r in ((res.scores, S), (res.clean, clean), (res.empty, empty)))
    got = res.values.cpu().numpy()
    want = phi if all_classes else phi[np.arange(B), cls]
    assert res.values.is_cuda and res.values.dtype == torch.float64 and got.shape == want.shape
    worst = float(np.abs(got - want).max())
    print(f"kernel_shap {what}: |scores - reference| {worst_s:.2e} (bound {TOL:.1e}) |values - reference| {worst:.2e} (bound {amp * TOL:.2e})")
    assert worst_s <= TOL and worst <= amp * TOL
    flat = got.reshape(-1, M)
    delta = (res.clean.cpu().numpy().astype(np.float64) - res.empty.cpu().numpy().astype(np.float64))
    delta = delta.reshape(-1) if all_classes else delta[np.arange(B), cls]
    add = max(abs(math.fsum(flat[q]) - delta[q]) / np.abs(flat[q]).sum() for q in range(flat.shape[0]))
    assert add <= 2.0 ** -50, f"sum of the values misses clean - empty by {add:.1e} of sum |values|"
    assert res.attribution.is_cuda and res.attribution.dtype == torch.float32
    assert np.array_equal(res.attribution.cpu().numpy(), got.astype(np.float32)[..., seg]), "the map is the values gathered through the label map"
    return worst


# class 5: the classes with p < 0.1 here move too little to discriminate
@pytest.mark.parametrize("class_idx", [None, 5, "all"], ids=["argmax", "class 5", "all classes"])
def test_spectrogram_input_exact_against_fp64_oracle(class_idx):
    seg, Z, w, S, clean, empty = _reference("mm spec")
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    res = brainxai.kernel_shap(mine, eeg, spec, segments=(2, 3), class_idx=class_idx, return_parts=True)
    assert res.exact and Z.shape == (62, 6)
    cls = clean.argmax(1) if class_idx in (None, "all") else np.full(3, class_idx)
    assert (res.classes is None) if class_idx == "all" else np.array_equal(res.classes.cpu().numpy(), cls)
    assert tuple(res.attribution.shape) == ((3, 6, 64, 128) if class_idx == "all" else (3, 64, 128))
    _check(res, seg, Z, w, S, clean, empty, cls, f"multimodal spec input 2x3 grid (exact), class_idx {class_idx}", all_classes=class_idx == "all")
    if class_idx is None:
        small = brainxai.kernel_shap(mine, eeg, spec, segments=(2, 3), max_batch=7, return_parts=True)
        for a, b in ((res.scores, small.scores), (res.clean, small.clean), (res.empty, small.empty), (res.values, small.values), (res.attribution, small.attribution)):
            assert torch.equal(a, b), "max_batch 256 and 7 give identical bits"
        assert tuple(brainxai.attribution_ranks(res.attribution).shape) == (3, 64 * 128)
        r = brainxai.deletion_insertion(mine, eeg, spec, res.attribution, steps=8)
        assert tuple(r.deletion.shape) == (3, 9) and bool(torch.isfinite(r.deletion).all())


def test_eeg_input_electrodes_against_fp64_oracle():
    seg, Z, w, S, clean, empty = _reference("mm eeg")
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    mine.train()
    before = PG.model_state(mine)
    res = brainxai.kernel_shap(mine, eeg, spec, input="eeg", segments="electrodes", num_samples=64, baseline=EEG_BASE, return_parts=True)
    assert PG.model_state(mine) == before and all(p.grad is None for p in mine.parameters())
    cls = clean.argmax(1)
    assert not res.exact and np.array_equal(res.classes.cpu().numpy(), cls) and tuple(res.attribution.shape) == (3, 19, 2000) and tuple(res.values.shape) == (3, 19)
    _check(res, seg, Z, w, S, clean, empty, cls, "multimodal EEG input, electrodes, N = 64")
    small = brainxai.kernel_shap(mine, eeg, spec, input="eeg", segments="electrodes", num_samples=64, baseline=EEG_BASE, max_batch=7, return_parts=True)
    assert torch.equal(res.scores, small.scores) and torch.equal(res.values, small.values) and torch.equal(res.attribution, small.attribution)
    again = brainxai.kernel_shap(mine, eeg, spec, input="eeg", segments=seg, coalitions=(res.coalitions, res.weights), baseline=EEG_BASE, class_idx=cls.tolist())
    assert torch.equal(again, res.attribution), "the returned parts repeat the call"
    assert tuple(brainxai.attribution_ranks(res.attribution).shape) == (3, 19 * 2000)


def test_stand_alone_spectrogram_model_against_fp64_oracle():
    seg, Z, w, S, clean, empty = _reference("spectrogram")
    _, mine = PG.scaled_multimodal()
    spec = PG.mm_inputs()[1].to(DEV)
    res = brainxai.kernel_shap(mine.spectrogram_model, None, spec, segments=(3, 4), num_samples=40, return_parts=True)
    cls = clean.argmax(1)
    assert not res.exact and np.array_equal(res.classes.cpu().numpy(), cls)
    _check(res, seg, Z, w, S, clean, empty, cls, "Spectrogram_Model 3x4 grid, N = 40")


def test_stand_alone_eegnet_against_fp64_oracle():
    seg, Z, w, S, clean, empty = _reference("eegnet")
    _, mine = PG.eegnet_pair()
    xe = O.seeded((3, 1, 19, 2000), 91, "randn").to(DEV)
    res = brainxai.kernel_shap(mine, xe, None, input="eeg", segments=("time", 6), class_idx="all", score="prob", return_parts=True)
    assert res.exact and res.classes is None and tuple(res.attribution.shape) == (3, 6, 1, 2000) and tuple(res.values.shape) == (3, 6, 6)
    _check(res, seg, Z, w, S, clean, empty, clean.argmax(1), "EEGNet 6 time slabs (exact), all classes", all_classes=True)
    lp = brainxai.kernel_shap(mine, xe, None, input="eeg", segments=("time", 6), score="logprob", return_parts=True)
    assert float((lp.scores.exp() - res.scores).abs().max()) <= 1e-6 and float(lp.scores.max()) <= 0.0
    want = R.values(Z, w, lp.scores.cpu().numpy(), lp.clean.cpu().numpy(), lp.empty.cpu().numpy())[np.arange(3), lp.classes.cpu().numpy()]
    assert np.abs(lp.values.cpu().numpy() - want).max() <= (6 + 62) * EPS * R.gram_cond(Z, w) * np.abs(want).max()


# ---- 5. bf16 storage ----------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_values():
    """bf16 storage.  The rows are bit-identical to the host-built ones (test_perturbed_spectrogram_rows_bit_for_bit); the values stay
    within the project's derived bf16 bound of the fp64 oracle's (BF16_LOGP of tests/perturb_gpu.py) for every score -- coalitions,
    clean and empty -- carried through the fit's solution operator, whose largest absolute row sum is amp."""
    seg, Z, w, S, clean, empty = _reference("mm spec")
    ref_model, mine = PG.scaled_multimodal(torch.bfloat16)
    eeg, spec = PG.mm_inputs()
    scale = PG.logp_scale(ref_model, eeg, spec)
    res = brainxai.kernel_shap(mine, eeg.to(DEV), spec.to(DEV), segments=(2, 3), return_parts=True)
    cls = clean.argmax(1)
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    phi, amp = _guarded(Z, w, S, clean, empty, cls, "multimodal spec input (bf16 case)")
    worst = float(np.abs(res.values.cpu().numpy() - phi[np.arange(3), cls]).max())
    print(f"kernel_shap multimodal spec input 2x3 grid, bf16 storage: |values - reference| {worst:.2e} (bound {amp * PG.BF16_LOGP * scale:.2e}, "
          f"log-probability scale {scale:.2f})")
    assert worst <= amp * PG.BF16_LOGP * scale
