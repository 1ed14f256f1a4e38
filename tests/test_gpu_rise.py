"""GPU: brainxai.rise / brainxai.rise_masks and the bx_rise_* entry points against the restatement of the definition
(tests/rise_ref.py): masks and perturbed rows bit for bit, the weighted sum against numpy fp64, and the maps end to end against the
oracle's classes run in fp64 on the CPU, on the models and inputs of tests/perturb_gpu.py.

Bounds.  Weighted sum: one fp32 rounding of the result, relative 2^-23, plus N 2^-52 relative for the order of the fp64 sum of N
non-negative terms (plus one fp32 subnormal step, 2^-149).  End to end, fp32 storage: |sal - ref| <= TOL max_p sum_n m_n(p) / D(p):
the project's probability bound (TOL of tests/perturb_gpu.py) carried through the weighted sum, whose weights m_n(p) / D(p) are
non-negative; the factor is computed from the reference masks.  Every compared case passes the guard of tests/perturb_gpu.py first.
bf16 storage: BF16_LOGP x the log-probability scale x the same factor (tests/perturb_gpu.py).
Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import perturb_gpu as PG
from tests import rise_ref as R
from tests.perturb_gpu import DEV, TOL

pytestmark = pytest.mark.gpu
N_E2E, GRID_E2E, P1 = 256, 8, 0.5


# ---- 1. the masks, bit for bit ------------------------------------------------------------------------------------------------------------
SHAPES = {"64x128 grid 8": (64, 128, 8, 8), "100x75 grid 7": (100, 75, 7, 7), "128x256 grid 8": (128, 256, 8, 8), "1x2000 grid 1x16": (1, 2000, 1, 16),
          "19x2000 grid 4x16": (19, 2000, 4, 16), "400x300 grid 7": (400, 300, 7, 7)}
WINDOWS = [(0, 5), (5, 38), (43, 20), (63, 1)]                       # 64 masks, split unevenly and across the kernel's groups of 8


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_masks_equal_the_restatement(shape):
    Hm, Wm, gh, gw = SHAPES[shape]
    bits, shifts = R.draw(64, gh, gw, Hm, Wm, 0.5, 7)
    want = torch.from_numpy(R.masks(bits, shifts, Hm, Wm))
    bits_d, shifts_d = PG.dev(bits), PG.dev(shifts)
    for n0, n in WINDOWS:
        out = torch.full((n, Hm, Wm), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.load().bx_rise_masks(PG.p(bits_d), PG.p(shifts_d), PG.p(out), 64, gh, gw, Hm, Wm, n0, n, PG.stream()), "bx_rise_masks")
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), "unwritten elements"
        assert torch.equal(PG.bits(out.cpu()), PG.bits(want[n0:n0 + n].contiguous())), f"{shape} window {(n0, n)}"
    whole = brainxai.rise_masks((Hm, Wm), grid=(gh, gw), masks=(bits, shifts), device=DEV)
    seeded, b2, s2 = brainxai.rise_masks((Hm, Wm), num_masks=64, grid=(gh, gw), p1=0.5, seed=7, device=DEV, return_parts=True)
    assert whole.is_cuda and whole.dtype == torch.float32 and torch.equal(PG.bits(whole.cpu()), PG.bits(want)) and torch.equal(whole, seeded)
    assert np.array_equal(b2, bits) and np.array_equal(s2, shifts)
    ones = brainxai.rise_masks((Hm, Wm), grid=(gh, gw), masks=(np.ones_like(bits), shifts), device=DEV)
    assert float(ones.min()) == 1.0 and float(ones.max()) == 1.0 and float(whole.min()) >= 0.0 and float(whole.max()) <= 1.0


# ---- 2. perturbed rows, bit for bit ---------------------------------------------------------------------------------------------------------
N_ROWS = 13
ROW_WINDOWS = [(0, 13), (3, 9), (12, 1)]


SPEC_SHAPES = {"4x64x128": (4, 64, 128, 8), "3x100x75": (3, 100, 75, 7), "4x128x256": (4, 128, 256, 8), "2x16x24": (2, 16, 24, (2, 3))}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(SPEC_SHAPES))
def test_perturbed_spectrogram_rows_bit_for_bit(shape, kind, dt):
    C, H, W, grid = SPEC_SHAPES[shape]
    B = 2
    geom = X._rise_geometry("rise", grid, H, W)
    x, base, bkind, base_d = PG.row_inputs((B, C, H, W), kind)
    bits, shifts = R.draw(N_ROWS, geom[0], geom[1], H, W, 0.5, 11)
    m = R.masks(bits, shifts, H, W)
    x_d, bits_d, shifts_d = x.to(DEV), PG.dev(bits), PG.dev(shifts)

    def launch(out, n0, n):
        L.check(L.load().bx_rise_perturb_spec(PG.p(x_d), PG.p(bits_d), PG.p(shifts_d), PG.p(base_d), bkind, PG.p(out), B, C, H, W, 8, N_ROWS, geom[0], geom[1],
                                              n0, n, ops.bx_dtype(dt), PG.stream()), "bx_rise_perturb_spec")
    PG.check_spec_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, ROW_WINDOWS,
                       lambda b0, nb, n0, n: X._rise_perturb(x_d, bits_d, shifts_d, geom, base_d, bkind, b0, nb, n0, n, dt), dt, f"{shape} {kind}")


@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("cells", ["electrode_time", "time"])
@pytest.mark.parametrize("chans,T", [(19, 2000), (37, 3000), (5, 333)])
def test_perturbed_eeg_rows_bit_for_bit(chans, T, cells, kind):
    B = 2
    map_rows = chans if cells == "electrode_time" else 1
    geom = X._rise_geometry("rise", (4, 16) if map_rows > 1 else 16, map_rows, T)
    x, base, bkind, base_d = PG.row_inputs((B, 1, chans, T), kind)
    bits, shifts = R.draw(N_ROWS, geom[0], geom[1], map_rows, T, 0.5, 13)
    m = R.masks(bits, shifts, map_rows, T)
    x_d, bits_d, shifts_d = x.to(DEV), PG.dev(bits), PG.dev(shifts)

    def launch(out, n0, n):
        L.check(L.load().bx_rise_perturb_eeg(PG.p(x_d), PG.p(bits_d), PG.p(shifts_d), map_rows, PG.p(base_d), bkind, PG.p(out), B, chans, T, N_ROWS, geom[0], geom[1],
                                             n0, n, PG.stream()), "bx_rise_perturb_eeg")
    PG.check_eeg_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, ROW_WINDOWS,
                      lambda b0, nb, n0, n: X._rise_perturb(x_d, bits_d, shifts_d, geom, base_d, bkind, b0, nb, n0, n, torch.float32, map_rows),
                      f"{chans}x{T} {cells} {kind}")


# ---- 3. the weighted sum ------------------------------------------------------------------------------------------------------------------
def _accumulate(P_d, cls_d, bits_d, shifts_d, B, N, K, gh, gw, Hm, Wm, p1, normalize):
    sal = torch.full((B, K if cls_d is None else 1, Hm, Wm), float("nan"), dtype=torch.float32, device=DEV)
    cov = torch.full((Hm, Wm), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.load().bx_rise_accumulate(PG.p(P_d), PG.p(cls_d), PG.p(bits_d), PG.p(shifts_d), PG.p(sal), PG.p(cov), B, N, K, gh, gw, Hm, Wm, p1,
                                        1 if normalize == "coverage" else 0, PG.stream()), "bx_rise_accumulate")
    torch.cuda.synchronize()
    return sal.cpu().numpy(), cov.cpu().numpy()


def _sum_bound(want, N):
    return np.abs(want) * (2.0 ** -23 + N * 2.0 ** -52) + 2.0 ** -149


# B, K, N (none fills a tile of 8 pairs or a chunk of 32 masks evenly), domain, grid, p1
ACC = {"3x6 of 70 masks, 64x128": (3, 6, 70, 64, 128, 8, 8, 0.5), "1x1 of 5 masks, 19x2000": (1, 1, 5, 19, 2000, 4, 16, 0.5),
       "5x32 of 33 masks, 100x75": (5, 32, 33, 100, 75, 7, 7, 0.25), "2x3 of 100 masks, 1x2000": (2, 3, 100, 1, 2000, 1, 16, 0.5),
       "9x2 of 64 masks, 16x24": (9, 2, 64, 16, 24, 2, 3, 1.0)}


@pytest.mark.parametrize("normalize", ["expected", "coverage"])
@pytest.mark.parametrize("case", sorted(ACC))
def test_weighted_sum_against_numpy_fp64(case, normalize):
    B, K, N, Hm, Wm, gh, gw, p1 = ACC[case]
    bits, shifts = R.draw(N, gh, gw, Hm, Wm, p1, 21)
    m = R.masks(bits, shifts, Hm, Wm)
    g = np.random.default_rng(N)
    P = g.random((B, N, K)).astype(np.float32)
    classes = g.integers(0, K, size=B).astype(np.int32)
    want = R.saliency(P, m, p1, normalize)
    want_cov = m.astype(np.float64).sum(0)
    P_d, bits_d, shifts_d = PG.dev(P), PG.dev(bits), PG.dev(shifts)
    got, cov = _accumulate(P_d, None, bits_d, shifts_d, B, N, K, gh, gw, Hm, Wm, p1, normalize)
    assert not np.isnan(got).any() and not np.isnan(cov).any(), "unwritten elements"
    excess = float((np.abs(got - want) / _sum_bound(want, N)).max())
    got_c, cov_c = _accumulate(P_d, PG.dev(classes), bits_d, shifts_d, B, N, K, gh, gw, Hm, Wm, p1, normalize)
    want_c = want[np.arange(B), classes][:, None]
    excess_c = float((np.abs(got_c - want_c) / _sum_bound(want_c, N)).max())
    excess_cov = float((np.abs(cov - want_cov) / _sum_bound(want_cov, N)).max())
    print(f"bx_rise_accumulate {case} {normalize}: worst error / bound: all classes {excess:.2f}, per-sample classes {excess_c:.2f}, coverage {excess_cov:.2f}")
    assert excess <= 1.0 and excess_c <= 1.0 and excess_cov <= 1.0
    assert np.array_equal(cov, cov_c) and np.array_equal(got[np.arange(B), classes], got_c[:, 0])
    again, cov_again = _accumulate(P_d, None, bits_d, shifts_d, B, N, K, gh, gw, Hm, Wm, p1, normalize)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)) and np.array_equal(cov.view(np.int32), cov_again.view(np.int32))
    if normalize == "coverage":                                      # a score that ignores the mask gives a flat map at that score
        flat, _ = _accumulate(PG.dev(np.full((B, N, K), 0.375, dtype=np.float32)), None, bits_d, shifts_d, B, N, K, gh, gw, Hm, Wm, p1, normalize)
        reached = want_cov > 0
        assert np.abs(flat[:, :, reached] - 0.375).max() <= 0.375 * (2.0 ** -23 + N * 2.0 ** -52) and (flat[:, :, ~reached] == 0).all()


def _planted(seed, Hm=64, Wm=128, gh=8, gw=8, N=200, p1=0.5):
    """A mask set, the cell p* whose mask values have the largest sum of squares, and P[n] = m_n(p*).  By Cauchy-Schwarz
    sum_n m_n(p*) m_n(p) <= sqrt(sum m_n(p*)^2 sum m_n(p)^2) <= sum m_n(p*)^2, so the expected-normalised map peaks at p*."""
    bits, shifts = R.draw(N, gh, gw, Hm, Wm, p1, seed)
    m = R.masks(bits, shifts, Hm, Wm)
    spot = np.unravel_index(int((m.astype(np.float64) ** 2).sum(0).argmax()), (Hm, Wm))
    return bits, shifts, m, spot, m[:, spot[0], spot[1]].reshape(1, N, 1).astype(np.float32)


def test_weighted_sum_finds_a_planted_cell():
    Hm, Wm, gh, gw, N, p1 = 64, 128, 8, 8, 200, 0.5
    spots = []
    for seed in (5, 6):
        bits, shifts, m, spot, P = _planted(seed)
        want = R.saliency(P, m, p1, "expected")[0, 0]
        assert np.unravel_index(int(want.argmax()), (Hm, Wm)) == spot                             # reference side first
        runner_up = np.sort(want.ravel())[-2]
        assert want[spot] - runner_up > 1e-4 * want[spot], "the peak must stand clear of fp32 rounding"
        got, _ = _accumulate(PG.dev(P), None, PG.dev(bits), PG.dev(shifts), 1, N, 1, gh, gw, Hm, Wm, p1, "expected")
        assert np.unravel_index(int(got[0, 0].argmax()), (Hm, Wm)) == spot
        spots.append(spot)
    assert spots[0] != spots[1]


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------------------
def _reference(f64, x, Hm, Wm, grid, what, classes=None, baseline=0.0, seed=0):
    """The fp64 oracle's scores and maps of one case, both normalisations, with the guard on the reference side alone."""
    geom = X._rise_geometry("rise", grid, Hm, Wm)
    bits, shifts = R.draw(N_E2E, geom[0], geom[1], Hm, Wm, P1, seed)
    m = R.masks(bits, shifts, Hm, Wm)
    B = x.shape[0]
    with torch.no_grad():
        clean = f64(x.double())
    cls = clean.argmax(1).numpy() if classes is None else np.broadcast_to(np.asarray(classes, dtype=np.int64), (B,))
    P = R.scores(f64, x.double(), m, baseline)
    perm = np.random.RandomState(1).permutation(N_E2E)
    ref = {"classes": cls, "bits": bits, "shifts": shifts, "P": P}
    for normalize in ("expected", "coverage"):
        factor = float((m.astype(np.float64).sum(0) / R.denominator(m, P1, normalize)).max())
        sal = R.saliency(P, m, P1, normalize)
        PG.guard_moved(sal, R.saliency(P[:, perm], m, P1, normalize), cls, TOL * factor, f"{what} {normalize}", f"factor {factor:.3f} {PG.spans(sal, cls)}")
        ref[normalize] = (sal, factor)
    return ref


def _compare(got, ref, normalize, what, tol=TOL, all_classes=False):
    sal, factor = ref[normalize]
    B = sal.shape[0]
    assert got.is_cuda and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    want = sal if all_classes else sal[np.arange(B), ref["classes"]]
    assert g.shape == want.shape
    worst = float(np.abs(g - want).max())
    print(f"rise {what} {normalize}: |map - reference| {worst:.2e} (bound {tol * factor:.2e})")
    assert worst <= tol * factor
    return worst


def test_spectrogram_input_against_fp64_oracle():
    ref_model, mine = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref_model).double()
    f = lambda xs: r64(eeg.double().repeat(xs.shape[0] // 3, 1, 1, 1), xs)                         # noqa: E731  (rows are mask-major there)
    ref = _reference(f, spec, 64, 128, GRID_E2E, "spec input")
    e, s = eeg.to(DEV), spec.to(DEV)
    for normalize in ("expected", "coverage"):
        res = brainxai.rise(mine, e, s, num_masks=N_E2E, grid=GRID_E2E, p1=P1, normalize=normalize, seed=0, return_parts=True)
        assert np.array_equal(res.bits, ref["bits"]) and np.array_equal(res.shifts, ref["shifts"])
        assert np.array_equal(res.classes.cpu().numpy(), ref["classes"])
        worst_p = float(np.abs(res.probs.cpu().numpy().astype(np.float64) - ref["P"]).max())
        print(f"rise spec input: |P - reference| {worst_p:.2e}")
        assert worst_p <= TOL
        _compare(res.saliency, ref, normalize, "spec input, fp32")
        every = brainxai.rise(mine, e, s, num_masks=N_E2E, grid=GRID_E2E, p1=P1, normalize=normalize, class_idx="all", masks=(res.bits, res.shifts))
        _compare(every, ref, normalize, "spec input, fp32, all classes", all_classes=True)


def test_spectrogram_input_baselines_and_classes_against_fp64_oracle():
    ref_model, mine = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref_model).double()
    f = lambda xs: r64(eeg.double().repeat(xs.shape[0] // 3, 1, 1, 1), xs)                         # noqa: E731
    base, cls = (0.5 * spec).contiguous(), [3, 5, 5]         # the other classes have p < 0.1 here: their maps move too little to discriminate
    ref = _reference(f, spec, 64, 128, (4, 16), "spec input, tensor baseline, classes per sample, grid 4x16", classes=cls, baseline=base.double(), seed=3)
    for normalize in ("expected", "coverage"):
        got = brainxai.rise(mine, eeg.to(DEV), spec.to(DEV), num_masks=N_E2E, grid=(4, 16), p1=P1, normalize=normalize, seed=3, class_idx=cls,
                            baseline=base.to(DEV), max_batch=100)
        _compare(got, ref, normalize, "spec input, tensor baseline, classes per sample")


@pytest.mark.parametrize("cells", ["electrode_time", "time"])
def test_eeg_input_against_fp64_oracle(cells):
    ref_model, mine = PG.eegnet_pair()
    xe = O.seeded((3, 1, 19, 2000), 91, "randn")
    n64 = copy.deepcopy(ref_model).double()
    Hm = 19 if cells == "electrode_time" else 1
    ref = _reference(lambda z: n64(z), xe, Hm, 2000, GRID_E2E, f"EEGNet, {cells}")
    for normalize in ("expected", "coverage"):
        res = brainxai.rise(mine, xe.to(DEV), None, input="eeg", cells=cells, num_masks=N_E2E, grid=GRID_E2E, p1=P1, normalize=normalize, seed=0,
                            return_parts=True)
        assert tuple(res.saliency.shape) == (3, Hm, 2000) and np.array_equal(res.classes.cpu().numpy(), ref["classes"])
        assert np.array_equal(res.bits, ref["bits"]) and np.array_equal(res.shifts, ref["shifts"])
        _compare(res.saliency, ref, normalize, f"EEGNet, {cells}, fp32")


# ---- 5. bf16 storage ----------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_maps():
    """bf16 storage.  The masked rows are bit-identical to the host-built ones (test_perturbed_spectrogram_rows_bit_for_bit); the map
    stays within the project's derived bf16 bound of the fp32 oracle's (BF16_LOGP of tests/perturb_gpu.py), carried through the
    non-negative weights m_n(p) / D(p).
    Measured on the MI355X: 3.07e-4 (expected) and 2.80e-4 (coverage), where the derived bound is 7.41e-2 and 6.58e-2."""
    ref_model, mine = PG.scaled_multimodal(torch.bfloat16)
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref_model).double()
    f = lambda xs: r64(eeg.double().repeat(xs.shape[0] // 3, 1, 1, 1), xs)                         # noqa: E731
    ref = _reference(f, spec, 64, 128, GRID_E2E, "spec input (bf16 case)")
    scale = PG.logp_scale(ref_model, eeg, spec)
    for normalize in ("expected", "coverage"):
        res = brainxai.rise(mine, eeg.to(DEV), spec.to(DEV), num_masks=N_E2E, grid=GRID_E2E, p1=P1, normalize=normalize, seed=0, return_parts=True)
        assert np.array_equal(res.classes.cpu().numpy(), ref["classes"])
        _compare(res.saliency, ref, normalize, f"spec input, bf16 storage (log-probability scale {scale:.2f})", tol=PG.BF16_LOGP * scale)


# ---- 6. interface ---------------------------------------------------------------------------------------------------------------------------
def test_interface_forms():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    mine.train()
    for p in list(mine.parameters())[:3]:
        p.requires_grad_(False)
    before = PG.model_state(mine)
    kw = dict(num_masks=40, grid=4, seed=2)
    sal = brainxai.rise(mine, eeg, spec, **kw)
    assert PG.model_state(mine) == before and all(m.training for m in mine.modules()) and all(p.grad is None for p in mine.parameters())
    assert sal.is_cuda and sal.dtype == torch.float32 and tuple(sal.shape) == (3, 64, 128) and bool(torch.isfinite(sal).all())
    full = brainxai.rise(mine, eeg, spec, return_parts=True, **kw)
    assert isinstance(full, brainxai.RiseResult) and torch.equal(full.saliency, sal)
    assert full.classes.dtype == torch.int64 and tuple(full.classes.shape) == (3,) and tuple(full.probs.shape) == (3, 40, 6) and full.probs.is_cuda
    assert tuple(full.coverage.shape) == (64, 128) and full.bits.shape == (40, 4, 4) and full.bits.dtype == np.uint8 and full.shifts.shape == (40, 2)
    assert float((full.probs.sum(2) - 1).abs().max()) <= 1e-6
    with torch.no_grad():
        want_cls = mine.eval()(eeg, spec).argmax(1)
        mine.train()
    assert torch.equal(full.classes, want_cls)
    masks = brainxai.rise_masks((64, 128), grid=4, masks=(full.bits, full.shifts), device=DEV)
    assert float((full.coverage.double() - masks.double().sum(0)).abs().max()) <= 40 * 2.0 ** -23      # one fp32 rounding of a sum <= 40
    # class forms
    every = brainxai.rise(mine, eeg, spec, class_idx="all", return_parts=True, **kw)
    assert tuple(every.saliency.shape) == (3, 6, 64, 128) and every.classes is None and torch.equal(every.probs, full.probs)
    assert torch.equal(every.saliency[torch.arange(3, device=DEV), full.classes], sal)
    four = brainxai.rise(mine, eeg, spec, class_idx=4, **kw)
    assert torch.equal(four, every.saliency[:, 4])
    cls = full.classes.tolist()
    for form in (cls, torch.tensor(cls), torch.tensor(cls, device=DEV, dtype=torch.int32)):
        assert torch.equal(brainxai.rise(mine, eeg, spec, class_idx=form, **kw), sal)
    # masks= repeats the seeded call; max_batch values that split the masks differently change no bit
    assert torch.equal(brainxai.rise(mine, eeg, spec, grid=4, masks=(full.bits, full.shifts)), sal)
    for mb in (7, 30, 1000):
        other = brainxai.rise(mine, eeg, spec, max_batch=mb, return_parts=True, **kw)
        assert torch.equal(other.probs, full.probs) and torch.equal(other.saliency, sal), f"max_batch {mb}"
    # the expected and the coverage normalisation differ by the coverage alone
    covn = brainxai.rise(mine, eeg, spec, normalize="coverage", **kw)
    assert float((covn * full.coverage - sal * (40 * 0.5)).abs().max()) <= 1e-4
    assert PG.model_state(mine) == before and all(p.grad is None for p in mine.parameters())
    # the EEG input of the multimodal model: the spectrogram branch runs once per sample
    for cells, shape in (("electrode_time", (3, 19, 2000)), ("time", (3, 1, 2000))):
        a = brainxai.rise(mine, eeg, spec, input="eeg", cells=cells, max_batch=256, return_parts=True, **kw)
        b = brainxai.rise(mine, eeg, spec, input="eeg", cells=cells, max_batch=9, return_parts=True, **kw)
        assert tuple(a.saliency.shape) == shape and torch.equal(a.classes, want_cls)
        assert torch.equal(a.probs, b.probs) and torch.equal(a.saliency, b.saliency)
    assert PG.model_state(mine) == before


def test_maps_fit_deletion_insertion_as_they_are():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    kw = dict(num_masks=64, grid=8, normalize="coverage")
    r = brainxai.deletion_insertion(mine, eeg, spec, brainxai.rise(mine, eeg, spec, **kw), steps=8)
    assert tuple(r.deletion.shape) == (3, 9) and tuple(r.ranks.shape) == (3, 64 * 128) and bool(torch.isfinite(r.deletion).all())
    for cells, n_cells in (("electrode_time", 19 * 2000), ("time", 2000)):
        amap = brainxai.rise(mine, eeg, spec, input="eeg", cells=cells, **kw)
        r = brainxai.deletion_insertion(mine, eeg, spec, amap, input="eeg", steps=8)
        assert tuple(r.ranks.shape) == (3, n_cells) and tuple(r.insertion.shape) == (3, 9) and bool(torch.isfinite(r.insertion_auc).all())
    assert tuple(brainxai.attribution_ranks(brainxai.rise(mine, eeg, spec, class_idx="all", **kw)[:, 2]).shape) == (3, 64 * 128)


def test_stand_alone_models():
    for dt in (torch.float32, torch.bfloat16):
        net = brainxai.set_compute_dtype(brainxai.Spectrogram_Model(6, in_channels=4).to(DEV), dt)
        s = torch.rand(2, 4, 64, 128, device=DEV)
        res = brainxai.rise(net, None, s, num_masks=24, grid=(4, 8), baseline=[0.1, 0.2, 0.3, 0.4], return_parts=True)
        with torch.no_grad():
            want = net.eval()(s).float().argmax(1)
            net.train()
        assert tuple(res.saliency.shape) == (2, 64, 128) and bool(torch.isfinite(res.saliency).all()) and net.training and torch.equal(res.classes, want)
    for cls in (brainxai.EEGNet, brainxai.EEGNetAttentionDeep):
        net = cls(6, Chans=19, Samples=2000).to(DEV)
        e = torch.randn(2, 1, 19, 2000, device=DEV)
        for cells, shape in (("electrode_time", (2, 19, 2000)), ("time", (2, 1, 2000))):
            res = brainxai.rise(net, e, None, input="eeg", cells=cells, num_masks=24, grid=8, baseline=torch.zeros(19, device=DEV), return_parts=True)
            assert tuple(res.saliency.shape) == shape and bool(torch.isfinite(res.saliency).all())
            # all-ones bits leave the input as it is: every score is the model's own probability
            ones = brainxai.rise(net, e, None, input="eeg", cells=cells, grid=8, masks=(np.ones_like(res.bits), res.shifts), return_parts=True)
            with torch.no_grad():
                net.eval()
                want = net(e).float().exp()
                net.train()
            assert float((ones.probs - want[:, None, :]).abs().max()) <= TOL
            assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
