"""GPU: brainxai.occlusion and the bx_occlusion_* entry points against the restatement of the definition (tests/occlusion_ref.py):
perturbed rows bit for bit, the map against numpy fp64, and the maps end to end against the oracle's classes run in fp64 on the CPU,
on the models and inputs of tests/perturb_gpu.py.

Bounds.  bx_occlusion_accumulate, per cell: |want| 2^-23 + M 2^-52 (sum_j |S0 - S_j|) / cnt + 2^-149, M the number of covering windows
-- one fp32 rounding of the result plus the fp64 rounding of M signed terms, their sum and the quotient.  End to end, fp32 storage:
|scores - ref| <= 1e-5, the project's probability bound (TOL of tests/perturb_gpu.py), and |attr - ref| <= 2e-5: the bound applies
to the clean and to the occluded score of each difference and carries through the mean, whose weights sum to 1.  Every compared case
passes the guard of tests/perturb_gpu.py first.  bf16 storage: 2 x BF16_LOGP x the log-probability scale (tests/perturb_gpu.py), the
bound applied to both scores of a difference.
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
from tests import occlusion_ref as R
from tests import perturb_gpu as PG
from tests.perturb_gpu import DEV, TOL

pytestmark = pytest.mark.gpu


# ---- 1. perturbed spectrogram rows, bit for bit ---------------------------------------------------------------------------------------------
# channels, H, W, window, stride
SPEC_SHAPES = {"2x16x24 window 5x7 stride 3x4": (2, 16, 24, (5, 7), (3, 4)), "3x100x75 window 32x10 stride 32x5": (3, 100, 75, (32, 10), (32, 5)),
               "4x64x128 window 16x32 stride 8x16": (4, 64, 128, (16, 32), (8, 16)), "4x64x128 one window": (4, 64, 128, (64, 128), None)}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(SPEC_SHAPES))
def test_perturbed_spectrogram_rows_bit_for_bit(shape, kind, dt):
    C, H, W, window, stride = SPEC_SHAPES[shape]
    B = 2
    geom = R.geometry(H, W, window, stride)
    assert X._occlusion_geometry("occlusion", window, stride, H, W) == geom
    wh, ww, sh, sw, ny, nx = geom
    N = ny * nx
    x, base, bkind, base_d = PG.row_inputs((B, C, H, W), kind)
    m = R.masks(H, W, window, stride)
    x_d = x.to(DEV)

    def launch(out, n0, n):
        L.check(L.load().bx_occlusion_perturb_spec(PG.p(x_d), PG.p(base_d), bkind, PG.p(out), B, C, H, W, 8, wh, ww, sh, sw, n0, n, ops.bx_dtype(dt), PG.stream()),
                "bx_occlusion_perturb_spec")
    PG.check_spec_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, PG.row_windows(N),
                       lambda b0, nb, n0, n: X._occlusion_perturb(x_d, geom, base_d, bkind, b0, nb, n0, n, dt), dt, f"{shape} {kind}")
    if N == 1 and kind == "scalar":                                  # one window: the row is the baseline
        out = X._occlusion_perturb(x_d, geom, base_d, bkind, 0, B, 0, 1, dt)
        assert float((out[:, :, :, :C].float() - 0.25).abs().max()) == 0.0


# ---- 2. perturbed EEG rows, bit for bit -----------------------------------------------------------------------------------------------------
EEG_SHAPES = {"5x333 window 2x50 stride 1x33": (5, 333, (2, 50), (1, 33)), "19x2000 electrodes": (19, 2000, (1, 2000), None),
              "19x2000 window 19x250 stride 19x125": (19, 2000, (19, 250), (19, 125)), "37x3000 window 4x300 stride 3x170": (37, 3000, (4, 300), (3, 170))}


@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(EEG_SHAPES))
def test_perturbed_eeg_rows_bit_for_bit(shape, kind):
    chans, T, window, stride = EEG_SHAPES[shape]
    B = 2
    geom = R.geometry(chans, T, window, stride)
    wh, ww, sh, sw, ny, nx = geom
    N = ny * nx
    x, base, bkind, base_d = PG.row_inputs((B, 1, chans, T), kind)
    m = R.masks(chans, T, window, stride)
    x_d = x.to(DEV)

    def launch(out, n0, n):
        L.check(L.load().bx_occlusion_perturb_eeg(PG.p(x_d), PG.p(base_d), bkind, PG.p(out), B, chans, T, wh, ww, sh, sw, n0, n, PG.stream()),
                "bx_occlusion_perturb_eeg")
    PG.check_eeg_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], m[j], bb), x, base, PG.row_windows(N),
                      lambda b0, nb, n0, n: X._occlusion_perturb(x_d, geom, base_d, bkind, b0, nb, n0, n, torch.float32, True), f"{shape} {kind}")


# ---- 3. the map -----------------------------------------------------------------------------------------------------------------------------
def _accumulate(S_d, S0_d, cls_d, B, N, K, Hm, Wm, geom):
    attr = torch.full((B, K if cls_d is None else 1, Hm, Wm), float("nan"), dtype=torch.float32, device=DEV)
    cnt = torch.full((Hm, Wm), -1, dtype=torch.int32, device=DEV)
    L.check(L.load().bx_occlusion_accumulate(PG.p(S_d), PG.p(S0_d), PG.p(cls_d), PG.p(attr), PG.p(cnt), B, N, K, Hm, Wm, *geom[:4], PG.stream()), "bx_occlusion_accumulate")
    torch.cuda.synchronize()
    return attr.cpu().numpy(), cnt.cpu().numpy()


# the geometries of tests/test_occlusion_cpu.py
ACC = {"16x24 window 5x7 stride 3x4": (16, 24, (5, 7), (3, 4)), "100x75 window 32x10 stride 32x5": (100, 75, (32, 10), (32, 5)),
       "64x128 one window": (64, 128, (64, 128), None), "19x2000 electrodes": (19, 2000, (1, 2000), None),
       "19x2000 window 19x250 stride 19x125": (19, 2000, (19, 250), (19, 125)), "16x24 window 4x4 stride 1": (16, 24, (4, 4), 1)}


@pytest.mark.parametrize("case", sorted(ACC))
def test_accumulate_against_numpy_fp64(case):
    Hm, Wm, window, stride = ACC[case]
    B, K = 5, 32
    geom = R.geometry(Hm, Wm, window, stride)
    N = geom[4] * geom[5]
    m = R.masks(Hm, Wm, window, stride)
    g = np.random.default_rng(N)
    S, S0 = g.random((B, N, K)).astype(np.float32), g.random((B, K)).astype(np.float32)
    classes = g.integers(0, K, size=B).astype(np.int32)
    want = R.attribution(S, S0, m)
    M = R.counts(m)
    absdrop = np.abs(S0.astype(np.float64)[:, None, :] - S.astype(np.float64))
    bound = np.abs(want) * 2.0 ** -23 + M * 2.0 ** -52 * np.einsum("bnk,nhw->bkhw", absdrop, m.astype(np.float64)) / M + 2.0 ** -149
    S_d, S0_d = PG.dev(S), PG.dev(S0)
    got, cnt = _accumulate(S_d, S0_d, None, B, N, K, Hm, Wm, geom)
    assert not np.isnan(got).any() and cnt.min() >= 1, "unwritten elements"
    assert cnt.dtype == np.int32 and np.array_equal(cnt, M)
    excess = float((np.abs(got - want) / bound).max())
    got_c, cnt_c = _accumulate(S_d, S0_d, PG.dev(classes), B, N, K, Hm, Wm, geom)
    sel = np.arange(B)
    excess_c = float((np.abs(got_c[:, 0] - want[sel, classes]) / bound[sel, classes]).max())
    print(f"bx_occlusion_accumulate {case}: {N} windows, counts {M.min()}..{M.max()}, worst error / bound: all classes {excess:.2f}, per-sample classes {excess_c:.2f}")
    assert excess <= 1.0 and excess_c <= 1.0
    assert np.array_equal(cnt, cnt_c) and np.array_equal(got[sel, classes].view(np.int32), got_c[:, 0].view(np.int32))
    again, cnt_again = _accumulate(S_d, S0_d, None, B, N, K, Hm, Wm, geom)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)) and np.array_equal(cnt, cnt_again)
    flat, _ = _accumulate(PG.dev(np.full((B, N, K), 0.375, dtype=np.float32)), PG.dev(np.full((B, K), 0.375, dtype=np.float32)), None, B, N, K, Hm, Wm, geom)
    assert (flat.view(np.int32) == 0).all(), "constant scores give an exactly-zero map"


def test_accumulate_finds_a_planted_cell():
    Hm, Wm, window, stride = 16, 24, (5, 7), (3, 4)
    geom = R.geometry(Hm, Wm, window, stride)
    m = R.masks(Hm, Wm, window, stride)
    N = m.shape[0]
    for spot in [(0, 0), (15, 23), (8, 11)]:
        covering = m[:, spot[0], spot[1]]
        S = np.where(covering, 0.25, 0.75).astype(np.float32).reshape(1, N, 1)
        got, _ = _accumulate(PG.dev(S), PG.dev(np.full((1, 1), 0.75, dtype=np.float32)), None, 1, N, 1, Hm, Wm, geom)
        assert got[0, 0][spot] == 0.5 == got.max() and m[covering].any(0)[got[0, 0] == 0.5].all()
        assert np.array_equal(got[0, 0].astype(np.float64), R.attribution(S, np.full((1, 1), 0.75), m)[0, 0].astype(np.float32).astype(np.float64))


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------------------------
SPEC_GEOMS = {"16x32 stride 8x16": ((16, 32), (8, 16)), "10x24 stride 7x24": ((10, 24), (7, 24)), "64x16 stride 64x8": ((64, 16), (64, 8))}
EEG_GEOMS = {"electrodes": ((1, 2000), None), "19x250 stride 19x125": ((19, 250), (19, 125)), "4x300 stride 3x170": ((4, 300), (3, 170))}


def _guarded(S, S0, m, cls, what, tol=2 * TOL):
    """The fp64 reference map of the explained classes, with the guard on the reference side alone."""
    N = S.shape[1]
    amap = R.attribution(S, S0, m)
    perm = np.random.RandomState(1).permutation(N)
    if N > 1:
        PG.guard_moved(amap, R.attribution(S[:, perm], S0, m), cls, tol, what)
    return amap


@functools.lru_cache(maxsize=None)
def _mm_reference(which, name):
    """(masks, S, S0, classes) of the fp64 oracle for the scaled multimodal model, zero baseline; computed once, shared, never changed."""
    ref_model, _ = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref_model).double()
    if which == "spec":
        window, stride = SPEC_GEOMS[name]
        x, m = spec, R.masks(64, 128, window, stride)
        f = lambda xs: r64(eeg.double().repeat(xs.shape[0] // 3, 1, 1, 1), xs)                     # noqa: E731  (rows are window-major there)
    else:
        window, stride = EEG_GEOMS[name]
        x, m = eeg, R.masks(19, 2000, window, stride)
        f = lambda xe: r64(xe, spec.double().repeat(xe.shape[0] // 3, 1, 1, 1))                    # noqa: E731
    S, S0 = R.scores(f, x.double(), m)
    return m, S, S0, S0.argmax(1)


def _check(res, m, S, S0, cls, what, tol=TOL, all_classes=False):
    amap = _guarded(S, S0, m, cls, what) if not all_classes else R.attribution(S, S0, m)
    B = S.shape[0]
    worst_s = max(float(np.abs(res.scores.cpu().numpy().astype(np.float64) - S).max()), float(np.abs(res.clean.cpu().numpy().astype(np.float64) - S0).max()))
    got = res.attribution.cpu().numpy().astype(np.float64)
    want = amap if all_classes else amap[np.arange(B), cls]
    assert res.attribution.is_cuda and res.attribution.dtype == torch.float32 and got.shape == want.shape
    worst = float(np.abs(got - want).max())
    print(f"occlusion {what}: |scores - reference| {worst_s:.2e} (bound {tol:.1e}) |map - reference| {worst:.2e} (bound {2 * tol:.1e})")
    assert worst_s <= tol and worst <= 2 * tol
    assert np.array_equal(res.counts.cpu().numpy(), R.counts(m))
    return worst


@pytest.mark.parametrize("name", sorted(SPEC_GEOMS))
def test_spectrogram_input_against_fp64_oracle(name):
    m, S, S0, cls = _mm_reference("spec", name)
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    window, stride = SPEC_GEOMS[name]
    res = brainxai.occlusion(mine, eeg, spec, window=window, stride=stride, return_parts=True)
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    _check(res, m, S, S0, cls, f"multimodal spec input {name}, fp32")


def test_spectrogram_input_all_classes_against_fp64_oracle():
    name = "16x32 stride 8x16"
    m, S, S0, cls = _mm_reference("spec", name)
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    res = brainxai.occlusion(mine, eeg, spec, window=SPEC_GEOMS[name][0], stride=SPEC_GEOMS[name][1], class_idx="all", return_parts=True, max_batch=100)
    assert res.classes is None and tuple(res.attribution.shape) == (3, 6, 64, 128)
    _check(res, m, S, S0, cls, f"multimodal spec input {name}, fp32, all classes", all_classes=True)


def test_spectrogram_input_tensor_baseline_and_classes_against_fp64_oracle():
    ref_model, mine = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref_model).double()
    f = lambda xs: r64(eeg.double().repeat(xs.shape[0] // 3, 1, 1, 1), xs)                         # noqa: E731
    base, cls = (0.5 * spec).contiguous(), np.array([3, 5, 5])       # the other classes have p < 0.1 here: their maps move too little to discriminate
    window, stride = SPEC_GEOMS["16x32 stride 8x16"]
    m = R.masks(64, 128, window, stride)
    S, S0 = R.scores(f, spec.double(), m, base.double())
    res = brainxai.occlusion(mine, eeg.to(DEV), spec.to(DEV), window=window, stride=stride, baseline=base.to(DEV), class_idx=cls.tolist(), max_batch=100,
                             return_parts=True)
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    _check(res, m, S, S0, cls, "multimodal spec input 16x32 stride 8x16, tensor baseline, classes per sample")


@pytest.mark.parametrize("name", sorted(EEG_GEOMS))
def test_eeg_input_of_the_multimodal_model_against_fp64_oracle(name):
    m, S, S0, cls = _mm_reference("eeg", name)
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    window, stride = EEG_GEOMS[name]
    res = brainxai.occlusion(mine, eeg, spec, input="eeg", window=window, stride=stride, return_parts=True)
    assert np.array_equal(res.classes.cpu().numpy(), cls) and tuple(res.attribution.shape) == (3, 19, 2000)
    _check(res, m, S, S0, cls, f"multimodal EEG input {name}, fp32")


@pytest.mark.parametrize("name", sorted(EEG_GEOMS))
def test_stand_alone_eegnet_against_fp64_oracle(name):
    ref_model, mine = PG.eegnet_pair()
    xe = O.seeded((3, 1, 19, 2000), 91, "randn")
    n64 = copy.deepcopy(ref_model).double()
    window, stride = EEG_GEOMS[name]
    m = R.masks(19, 2000, window, stride)
    S, S0 = R.scores(lambda z: n64(z), xe.double(), m)
    cls = S0.argmax(1)
    res = brainxai.occlusion(mine, xe.to(DEV), None, input="eeg", window=window, stride=stride, return_parts=True)
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    _check(res, m, S, S0, cls, f"EEGNet {name}, fp32")


# ---- 5. bf16 storage ----------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_maps():
    """bf16 storage.  The occluded rows are bit-identical to the host-built ones (test_perturbed_spectrogram_rows_bit_for_bit); the map
    stays within the project's derived bf16 bound of the fp64 oracle's (BF16_LOGP of tests/perturb_gpu.py), for the clean and the
    occluded score of each difference, carried through the mean, whose weights sum to 1.  Measured on the MI355X: 3.00e-4, where the derived bound is 1.32e-1."""
    name = "16x32 stride 8x16"
    m, S, S0, cls = _mm_reference("spec", name)
    ref_model, mine = PG.scaled_multimodal(torch.bfloat16)
    eeg, spec = PG.mm_inputs()
    scale = PG.logp_scale(ref_model, eeg, spec)
    res = brainxai.occlusion(mine, eeg.to(DEV), spec.to(DEV), window=SPEC_GEOMS[name][0], stride=SPEC_GEOMS[name][1], return_parts=True)
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    want = _guarded(S, S0, m, cls, "multimodal spec input (bf16 case)")[np.arange(3), cls]
    worst = float(np.abs(res.attribution.cpu().numpy().astype(np.float64) - want).max())
    print(f"occlusion multimodal spec input {name}, bf16 storage: |map - reference| {worst:.2e} (bound {2 * PG.BF16_LOGP * scale:.2e}, log-probability scale {scale:.2f})")
    assert worst <= 2 * PG.BF16_LOGP * scale


# ---- 6. interface ---------------------------------------------------------------------------------------------------------------------------
def test_interface_forms():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    mine.train()
    for p in list(mine.parameters())[:3]:
        p.requires_grad_(False)
    before = PG.model_state(mine)
    kw = dict(window=(16, 32), stride=(8, 16))
    amap = brainxai.occlusion(mine, eeg, spec, **kw)
    assert PG.model_state(mine) == before and all(mod.training for mod in mine.modules()) and all(p.grad is None for p in mine.parameters())
    assert amap.is_cuda and amap.dtype == torch.float32 and tuple(amap.shape) == (3, 64, 128) and bool(torch.isfinite(amap).all())
    full = brainxai.occlusion(mine, eeg, spec, return_parts=True, **kw)
    assert isinstance(full, brainxai.OcclusionResult) and torch.equal(full.attribution, amap) and full.grid == (7, 7)
    assert full.classes.dtype == torch.int64 and tuple(full.classes.shape) == (3,) and full.classes.is_cuda
    assert full.scores.dtype == torch.float32 and tuple(full.scores.shape) == (3, 49, 6) and full.scores.is_cuda
    assert full.clean.dtype == torch.float32 and tuple(full.clean.shape) == (3, 6) and full.clean.is_cuda
    assert full.counts.dtype == torch.int32 and tuple(full.counts.shape) == (64, 128) and full.counts.is_cuda
    assert full.drops.dtype == torch.float32 and tuple(full.drops.shape) == (3, 7, 7) and full.drops.is_cuda
    assert float((full.scores.sum(2) - 1).abs().max()) <= 1e-6 and float((full.clean.sum(1) - 1).abs().max()) <= 1e-6
    assert np.array_equal(full.counts.cpu().numpy(), R.counts(R.masks(64, 128, (16, 32), (8, 16))))
    sel = torch.arange(3, device=DEV)
    assert torch.equal(full.drops, (full.clean[:, None, :] - full.scores)[sel, :, full.classes].reshape(3, 7, 7))
    with torch.no_grad():
        want_cls = mine.eval()(eeg, spec).argmax(1)
        mine.train()
    assert torch.equal(full.classes, want_cls)
    # class forms
    every = brainxai.occlusion(mine, eeg, spec, class_idx="all", return_parts=True, **kw)
    assert tuple(every.attribution.shape) == (3, 6, 64, 128) and every.classes is None and torch.equal(every.scores, full.scores)
    assert tuple(every.drops.shape) == (3, 6, 7, 7) and torch.equal(every.drops, (every.clean[:, None, :] - every.scores).permute(0, 2, 1).reshape(3, 6, 7, 7))
    assert torch.equal(every.attribution[sel, full.classes], amap) and torch.equal(every.drops[sel, full.classes], full.drops)
    four = brainxai.occlusion(mine, eeg, spec, class_idx=4, **kw)
    assert torch.equal(four, every.attribution[:, 4])
    cls = full.classes.tolist()
    for form in (cls, torch.tensor(cls), torch.tensor(cls, device=DEV, dtype=torch.int32)):
        assert torch.equal(brainxai.occlusion(mine, eeg, spec, class_idx=form, **kw), amap)
    # max_batch values that split the windows differently change no bit
    for mb in (7, 30, 1000):
        other = brainxai.occlusion(mine, eeg, spec, max_batch=mb, return_parts=True, **kw)
        assert torch.equal(other.scores, full.scores) and torch.equal(other.clean, full.clean) and torch.equal(other.attribution, amap), f"max_batch {mb}"
    # score='logprob' is the accumulate of the returned log-probabilities
    lp = brainxai.occlusion(mine, eeg, spec, score="logprob", class_idx="all", return_parts=True, **kw)
    assert float((lp.scores.exp() - full.scores).abs().max()) <= 1e-6 and float(lp.scores.max()) <= 0.0
    m = R.masks(64, 128, (16, 32), (8, 16))
    want = R.attribution(lp.scores.cpu().numpy(), lp.clean.cpu().numpy(), m)
    drop_max = float(np.abs(lp.clean.cpu().numpy().astype(np.float64)[:, None] - lp.scores.cpu().numpy().astype(np.float64)).max())
    bound = np.abs(want) * 2.0 ** -23 + 4 * 2.0 ** -52 * drop_max + 2.0 ** -149                          # the bound of test_accumulate_against_numpy_fp64, M <= 4
    assert (np.abs(lp.attribution.cpu().numpy().astype(np.float64) - want) <= bound).all()
    # stride=None is stride=window
    tiles = brainxai.occlusion(mine, eeg, spec, window=(16, 32), return_parts=True)
    same = brainxai.occlusion(mine, eeg, spec, window=(16, 32), stride=(16, 32), return_parts=True)
    assert tiles.grid == (4, 4) and torch.equal(tiles.attribution, same.attribution) and torch.equal(tiles.scores, same.scores)
    assert int(tiles.counts.min()) == 1 == int(tiles.counts.max())
    assert torch.equal(brainxai.occlusion(mine, eeg, spec, window=16, stride=8, return_parts=True).scores,
                       brainxai.occlusion(mine, eeg, spec, window=(16, 16), stride=(8, 8), return_parts=True).scores)
    assert PG.model_state(mine) == before and all(p.grad is None for p in mine.parameters())
    # the EEG input of the multimodal model: the spectrogram branch runs once per sample; electrode ablation
    a = brainxai.occlusion(mine, eeg, spec, input="eeg", window=(1, 2000), max_batch=256, return_parts=True)
    b = brainxai.occlusion(mine, eeg, spec, input="eeg", window=(1, 2000), max_batch=9, return_parts=True)
    assert tuple(a.attribution.shape) == (3, 19, 2000) and a.grid == (19, 1) and tuple(a.drops.shape) == (3, 19, 1) and torch.equal(a.classes, want_cls)
    assert torch.equal(a.scores, b.scores) and torch.equal(a.attribution, b.attribution)
    assert torch.equal(a.attribution, a.drops.expand(3, 19, 2000)), "one window per electrode: the map repeats the per-electrode drop"
    assert PG.model_state(mine) == before


def test_maps_fit_deletion_insertion_as_they_are():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    amap = brainxai.occlusion(mine, eeg, spec, window=(16, 32), stride=(8, 16))
    r = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8)
    assert tuple(r.deletion.shape) == (3, 9) and tuple(r.ranks.shape) == (3, 64 * 128) and bool(torch.isfinite(r.deletion).all())
    emap = brainxai.occlusion(mine, eeg, spec, input="eeg", window=(19, 250), stride=(19, 125))
    r = brainxai.deletion_insertion(mine, eeg, spec, emap, input="eeg", steps=8)
    assert tuple(r.ranks.shape) == (3, 19 * 2000) and tuple(r.insertion.shape) == (3, 9) and bool(torch.isfinite(r.insertion_auc).all())
    every = brainxai.occlusion(mine, eeg, spec, window=(16, 32), class_idx="all")
    assert tuple(brainxai.attribution_ranks(every[:, 2]).shape) == (3, 64 * 128)


def test_stand_alone_models():
    for dt in (torch.float32, torch.bfloat16):
        net = brainxai.set_compute_dtype(brainxai.Spectrogram_Model(6, in_channels=4).to(DEV), dt)
        s = torch.rand(2, 4, 64, 128, device=DEV)
        res = brainxai.occlusion(net, None, s, window=(16, 128), stride=(8, 128), baseline=[0.1, 0.2, 0.3, 0.4], return_parts=True)
        with torch.no_grad():
            want = net.eval()(s).float()
            net.train()
        assert tuple(res.attribution.shape) == (2, 64, 128) and res.grid == (7, 1) and bool(torch.isfinite(res.attribution).all()) and net.training
        assert torch.equal(res.classes, want.argmax(1)) and float((res.clean - want.exp()).abs().max()) <= (TOL if dt == torch.float32 else 2e-2)
        # a baseline equal to the input occludes nothing: every drop is exactly zero
        none = brainxai.occlusion(net, None, s, window=(16, 128), stride=(8, 128), baseline=s.clone(), return_parts=True)
        assert float(none.drops.abs().max()) == 0.0 and float(none.attribution.abs().max()) == 0.0
    for cls in (brainxai.EEGNet, brainxai.EEGNetAttentionDeep):
        net = cls(6, Chans=19, Samples=2000).to(DEV)
        e = torch.randn(2, 1, 19, 2000, device=DEV)
        res = brainxai.occlusion(net, e, None, input="eeg", window=(4, 300), stride=(3, 170), baseline=torch.zeros(19, device=DEV), return_parts=True)
        assert tuple(res.attribution.shape) == (2, 19, 2000) and res.grid == (6, 11) and bool(torch.isfinite(res.attribution).all())
        with torch.no_grad():
            net.eval()
            want = net(e).float().exp()
            net.train()
        assert float((res.clean - want).abs().max()) <= TOL
        assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
