"""GPU: brainxai.attribution_ranks / brainxai.deletion_insertion and the bx_rank_desc / bx_faith_* entry points against the
restatement of the definition (tests/faith_ref.py): ranks and perturbed rows bit for bit, the curve kernel against numpy, and the
curves end to end against the oracle's classes run in fp64 on the CPU.

Bounds.  fp32 storage: |curve - reference| <= 1e-5 absolute on probabilities and on the area, the project's probability bound (TOL of
tests/perturb_gpu.py; the area is a weighted mean of the points).  Every compared case is first checked ON THE REFERENCE SIDE to
move: its fp64 curve spans at least 0.1, and the curve under the reversed ranking differs from it by more than 100 x the bound
somewhere -- a perturb kernel that did nothing, or ranked backwards, cannot pass.
Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import faith_ref as R
from tests import perturb_gpu as PG
from tests.perturb_gpu import DEV, TOL

pytestmark = pytest.mark.gpu
STEPS = 16


# ---- 1. ranks, exact -------------------------------------------------------------------------------------------------------------------
RANK_N = [1, 7, 255, 256, 257, 4096, 32768, 38000, 111000, 120000]
RANK_KINDS = ["uniform", "quantised", "equal", "gradcam", "special"]


def _rank_values(kind, B, N, seed):
    g = np.random.default_rng(seed)
    if kind == "uniform":
        return g.random((B, N)).astype(np.float32) * 2 - 1
    if kind == "quantised":
        return (np.floor(g.random((B, N)) * 8) / 8).astype(np.float32)
    if kind == "equal":
        return np.full((B, N), 0.375, dtype=np.float32)
    if kind == "gradcam":                                            # a coarse ReLU'd map, bilinearly upsampled: zero regions and smooth slopes
        h = max(1, int(np.sqrt(N)))
        w = -(-N // h)
        coarse = torch.from_numpy(g.standard_normal((B, 1, 4, 8)).astype(np.float32)).clamp_min(0)
        up = F.interpolate(coarse, size=(max(h, 1), max(w, 1)), mode="bilinear", align_corners=False)
        return np.ascontiguousarray(up.reshape(B, -1)[:, :N].numpy())
    a = (np.floor(g.random((B, N)) * 8) / 8 - 0.5).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0], dtype=np.float32)
    for b in range(B):
        pos = g.integers(0, N, size=min(N, 40))
        a[b, pos] = specials[g.integers(0, specials.size, size=pos.size)]
    return a


@pytest.mark.parametrize("kind", RANK_KINDS)
@pytest.mark.parametrize("N", RANK_N)
def test_ranks_equal_the_restatement(N, kind):
    for B in (1, 3, 64):
        a = _rank_values(kind, B, N, 1000 * B + N)
        shaped = a.reshape(B, 400, 300) if N == 120000 else a.reshape(B, 128, 256) if N == 32768 else a.reshape(B, 19, 2000) if N == 38000 else a
        got = brainxai.attribution_ranks(PG.dev(shaped))
        torch.cuda.synchronize()
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (B, N)
        got = got.cpu().numpy()
        for b in range(B):
            assert np.array_equal(np.bincount(got[b].clip(0, N - 1), minlength=N), np.ones(N, dtype=np.int64)), f"row {b} is not a permutation"
        assert np.array_equal(got, R.ranks(a)), f"B={B} N={N} {kind}"


def test_ranks_repeat_and_ignore_the_layout():
    a = _rank_values("special", 3, 38000, 5)
    first = brainxai.attribution_ranks(PG.dev(a))
    again = brainxai.attribution_ranks(PG.dev(a).reshape(3, 19, 2000))
    strided = brainxai.attribution_ranks(PG.dev(np.ascontiguousarray(a.reshape(3, 19, 2000).transpose(0, 2, 1))).permute(0, 2, 1))
    assert torch.equal(first, again) and torch.equal(first, strided)


# ---- 2. perturbed rows, bit for bit ----------------------------------------------------------------------------------------------------
def _windows(steps):
    return [(0, steps + 1), (steps // 2 - 1, steps + 1 - (steps // 2 - 1)), (steps, 1)]


def _want_rows(x, rank, base, ks, i0, n, insertion):
    return PG.want_rows(lambda b, j, bb: R.perturbed(x[b:b + 1], rank[b:b + 1], bb, ks[j], insertion), x, base, i0, n)


SPEC_SHAPES = {"4x64x128": (4, 64, 128, 16), "3x100x75": (3, 100, 75, 16), "4x128x256": (4, 128, 256, 32)}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("insertion", [False, True], ids=["deletion", "insertion"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("shape", sorted(SPEC_SHAPES))
def test_perturbed_spectrogram_rows_bit_for_bit(shape, kind, insertion, dt):
    C, H, W, steps = SPEC_SHAPES[shape]
    B, N = 2, H * W
    x, base, bkind, base_d = PG.row_inputs((B, C, H, W), kind)
    rank = R.ranks(_rank_values("quantised", B, N, 17))
    per, ks = R.cuts(N, steps)
    assert shape != "3x100x75" or steps * per > N                    # the last cut is clamped there
    x_d, rank_d = x.to(DEV), PG.dev(rank)

    def launch(out, i0, n):
        L.check(L.load().bx_faith_perturb_spec(PG.p(x_d), PG.p(rank_d), PG.p(base_d), bkind, PG.p(out), B, C, H, W, 8, per, i0, n, int(insertion),
                                               ops.bx_dtype(dt), PG.stream()), "bx_faith_perturb_spec")
    PG.check_spec_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], rank[b:b + 1], bb, ks[j], insertion), x, base, _windows(steps),
                       lambda b0, nb, i0, n: X._faith_perturb(x_d, rank_d, base_d, bkind, b0, nb, i0, n, per, insertion, dt), dt, f"{shape} {kind}")


@pytest.mark.parametrize("insertion", [False, True], ids=["deletion", "insertion"])
@pytest.mark.parametrize("kind", ["scalar", "per_channel", "tensor"])
@pytest.mark.parametrize("cells", ["electrode_time", "time_column"])
@pytest.mark.parametrize("chans,T", [(19, 2000), (37, 3000), (5, 333)])
def test_perturbed_eeg_rows_bit_for_bit(chans, T, cells, kind, insertion):
    B, steps = 2, STEPS
    map_rows = chans if cells == "electrode_time" else 1
    N = map_rows * T
    x, base, bkind, base_d = PG.row_inputs((B, 1, chans, T), kind)
    rank = R.ranks(_rank_values("quantised", B, N, 23))
    per, ks = R.cuts(N, steps)
    x_d, rank_d = x.to(DEV), PG.dev(rank)

    def launch(out, i0, n):
        L.check(L.load().bx_faith_perturb_eeg(PG.p(x_d), PG.p(rank_d), map_rows, PG.p(base_d), bkind, PG.p(out), B, chans, T, per, i0, n, int(insertion),
                                              PG.stream()), "bx_faith_perturb_eeg")
    PG.check_eeg_rows(launch, lambda b, j, bb: R.perturbed(x[b:b + 1], rank[b:b + 1], bb, ks[j], insertion), x, base, _windows(steps),
                      lambda b0, nb, i0, n: X._faith_perturb(x_d, rank_d, base_d, bkind, b0, nb, i0, n, per, insertion, torch.float32, map_rows),
                      f"{chans}x{T} {cells} {kind}")


CLAMPED = {"spec 1x1x7, 5 steps": ((2, 1, 1, 7), None, 5), "spec 3x2x5, 7 steps": ((2, 3, 2, 5), None, 7), "spec 4x64x128, 120 steps": ((2, 4, 64, 128), None, 120),
           "eeg 19x2000 columns, 64 steps": ((2, 1, 19, 2000), 1, 64), "eeg 19x2000 columns, 1500 steps": ((2, 1, 19, 2000), 1, 1500),
           "eeg 3x7 cells, 17 steps": ((2, 1, 3, 7), 3, 17)}


@pytest.mark.parametrize("insertion", [False, True], ids=["deletion", "insertion"])
@pytest.mark.parametrize("case", sorted(CLAMPED))
def test_perturbed_rows_with_several_points_at_the_clamped_cut(case, insertion):
    """k_i = min(N, i * per) reaches N before the last point whenever (steps - 1) * ceil(N / steps) >= N: every such point is the
    all-baseline (deletion) / unperturbed (insertion) input, and asking for it is part of the contract."""
    shape, map_rows, steps = CLAMPED[case]
    B = shape[0]
    N = shape[2] * shape[3] if map_rows is None else map_rows * shape[3]
    per, ks = R.cuts(N, steps)
    tail = sum(k == N for k in ks)
    assert tail >= 2 and (steps - 1) * per >= N
    x = O.seeded(shape, 13, "randn")
    rank = R.ranks(_rank_values("quantised", B, N, 29))
    base = PG.baseline("per_channel", x, 5)
    bkind, base_d = PG.base_dev(base)
    x_d, rank_d = x.to(DEV), PG.dev(rank)
    first = steps + 1 - tail                                         # the first clamped point
    for i0, n in ([(0, steps + 1)] if steps <= 200 else []) + [(max(0, first - 3), min(tail + 3, 12)), (steps - 1, 2), (steps, 1)]:
        for dt in ((torch.float32, torch.bfloat16) if map_rows is None else (torch.float32,)):
            got = X._faith_perturb(x_d, rank_d, base_d, bkind, 0, B, i0, n, per, insertion, dt, map_rows)
            rows = _want_rows(x, rank, base, ks, i0, n, insertion).to(DEV)
            want = ops.to_nhwc(rows, dt) if map_rows is None else rows
            torch.cuda.synchronize()
            assert got.shape == want.shape and torch.equal(PG.bits(got), PG.bits(want)), f"{case} window {(i0, n)} {dt}"
    whole = base_d.reshape(1, -1, 1, 1).expand(shape) if map_rows is None else base_d.reshape(1, 1, -1, 1).expand(shape)
    last = X._faith_perturb(x_d, rank_d, base_d, bkind, 0, B, steps - 1, 2, per, insertion, torch.float32, map_rows)
    want_last = (x_d if insertion else whole.contiguous())
    want_last = ops.to_nhwc(want_last, torch.float32) if map_rows is None else want_last
    for j in range(2):                                               # both tail rows of every sample are the end point itself
        assert torch.equal(last.reshape(B, 2, *last.shape[1:])[:, j], want_last.reshape(last.reshape(B, 2, *last.shape[1:])[:, j].shape))


def test_many_steps_through_the_driver():
    """steps = 120 on 64 x 128 cells (per = 69: points 119 and 120 both at k = N) and steps = 64 / 1500 on 2000 time columns (2 / 501 points at k = N), end to end through
    deletion_insertion against the same model's ordinary forward on host-built inputs."""
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    es, ss = brainxai.saliency(mine, eeg, spec)
    for which, amap, steps in (("spec", ss, 120), ("eeg", es.sum(1, keepdim=True), 64), ("eeg", es.sum(1, keepdim=True), 1500)):
        res = brainxai.deletion_insertion(mine, eeg, spec, amap, input=which, steps=steps, max_batch=100)
        assert tuple(res.deletion.shape) == (3, steps + 1) and float(res.fractions[-2]) == 1.0 and float(res.fractions[-1]) == 1.0
        assert float((res.deletion[:, -1] - res.deletion[:, -2]).abs().max()) <= TOL
        worst = 0.0
        for m, ins in (("deletion", False), ("insertion", True)):
            host = _host_built_curve(mine, eeg, spec, which, res.ranks, 0.0, steps, res.classes, ins)
            worst = max(worst, float(np.abs(getattr(res, m).cpu().numpy().astype(np.float64) - host).max()))
        print(f"many steps, {which} input, {steps} steps: against the ordinary forward on host-built inputs {worst:.2e}")
        assert worst <= TOL


# ---- 3. the curve kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,K", [(5, 17, 6), (70, 33, 6), (1, 2, 3)])
def test_curve_kernel_against_numpy(B, P, K):
    g = torch.Generator().manual_seed(B + P)
    logp = torch.log_softmax(torch.randn(B, P, K, generator=g) * 2, dim=2).contiguous()
    classes = torch.randint(0, K, (B,), generator=g).to(torch.int32)
    logp_d, cls_d = logp.to(DEV), classes.to(DEV)
    for use_logprob in (0, 1):
        curve = torch.full((B, P), float("nan"), dtype=torch.float32, device=DEV)
        auc = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
        L.check(L.load().bx_faith_curve(PG.p(logp_d), PG.p(cls_d), PG.p(curve), PG.p(auc), B, P, K, use_logprob, PG.stream()), "bx_faith_curve")
        torch.cuda.synchronize()
        curve, auc = curve.cpu().numpy(), auc.cpu().numpy()
        lp = logp.numpy()[np.arange(B), :, classes.numpy()]
        if use_logprob:
            assert np.array_equal(curve, lp)
        else:
            want = np.exp(lp.astype(np.float64))
            rel = np.abs(curve - want) / want
            print(f"bx_faith_curve B={B} P={P}: exp within {rel.max() / 2.0 ** -24:.2f} x 2^-24 relative")
            assert rel.max() <= 2.0 ** -22                           # 1 ulp of exp plus the rounding of the result
        for b in range(B):
            assert auc[b] == R.auc(curve[b]), "the area is the fp64 sum of the returned fp32 points in index order"


# ---- 4. end to end against the oracle ---------------------------------------------------------------------------------------------------
def _reference(f64, x, amap, what, steps=STEPS, **kw):
    """Reference curves of one case, with the guard on the test's inputs (reference side alone)."""
    rank = R.ranks(amap.numpy())
    c = R.curves(f64, x.double(), rank, steps, **kw)
    rev = R.curves(f64, x.double(), rank.shape[1] - 1 - rank, steps, **kw)
    for m in ("deletion", "insertion"):
        span = c[m].max(1) - c[m].min(1)
        moved = np.abs(c[m] - rev[m]).max(1)
        print(f"{what} {m}: reference p0 {c['deletion'][:, 0].round(3)} span {span.round(3)} |curve - reversed| {moved.round(4)} auc {c[m + '_auc'].round(4)}")
        assert span.min() >= 0.1, f"{what} {m}: the reference curve spans {span.min():.3f} < 0.1: not a discriminating input"
        assert moved.min() > 100 * TOL, f"{what} {m}: reversing the ranking moves the reference curve by {moved.min():.1e} only"
    return rank, c


def _compare(res, rank, c, what, tol=TOL):
    assert torch.equal(res.ranks.cpu(), torch.from_numpy(rank))
    assert np.array_equal(res.classes.cpu().numpy(), c["classes"])
    assert res.fractions.dtype == torch.float64 and np.array_equal(res.fractions.numpy(), c["fractions"])
    worst = {}
    for m in ("deletion", "insertion"):
        curve, auc = getattr(res, m), getattr(res, m + "_auc")
        assert curve.is_cuda and curve.dtype == torch.float32 and auc.is_cuda and auc.dtype == torch.float64
        worst[m] = float(np.abs(curve.cpu().numpy().astype(np.float64) - c[m]).max())
        worst[m + "_auc"] = float(np.abs(auc.cpu().numpy() - c[m + "_auc"]).max())
    print(f"deletion_insertion {what}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= tol, worst
    return worst


def _oracle_maps(ref, eeg, spec):
    cam = O.grad_cam(ref, eeg, spec)
    es, ss = O.saliency(ref, eeg, spec)
    return {"gradcam": cam.float().contiguous(), "saliency": ss.float().contiguous()}, es.float().contiguous()


def test_spectrogram_input_against_fp64_oracle():
    ref, mine = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref).double()
    maps, _ = _oracle_maps(ref, eeg, spec)
    maps["random"] = O.seeded((3, 64, 128), 5, "rand")
    aucs = {}
    for name, amap in maps.items():
        rank, c = _reference(lambda xs: r64(eeg.double(), xs), spec, amap, f"spec input, {name}")
        res = brainxai.deletion_insertion(mine, eeg.to(DEV), spec.to(DEV), amap.to(DEV), steps=STEPS)
        _compare(res, rank, c, f"spec input, {name}, fp32")
        aucs[name] = c["deletion_auc"].mean()
    assert len({round(v, 3) for v in aucs.values()}) == 3            # the three orders are told apart in the third decimal at least


def CASES(spec):
    """Baseline forms, class forms and the score: classes other than the arg-max one (class 3) have p ~ 0.04-0.2 here, whose
    probability curves span too little to discriminate; the log-probability curves of classes 1, 4 and 5 do."""
    return [("per-channel baseline", [0.0, 0.1, 0.0, 0.2], None, "prob"), ("tensor baseline, classes per sample, logprob", (0.2 * spec).contiguous(), [1, 4, 5], "logprob"),
            ("zero baseline, class 5, logprob", 0.0, 5, "logprob"), ("zero baseline, logprob", 0.0, None, "logprob")]


def test_spectrogram_input_baselines_and_classes_against_fp64_oracle():
    ref, mine = PG.scaled_multimodal()
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref).double()
    amap = _oracle_maps(ref, eeg, spec)[0]["saliency"]
    f = lambda xs: r64(eeg.double(), xs)
    for what, base, cls, score in CASES(spec):
        rank, c = _reference(f, spec, amap, f"spec input, {what}", baseline=base, classes=cls, score=score)
        res = brainxai.deletion_insertion(mine, eeg.to(DEV), spec.to(DEV), amap.to(DEV), steps=STEPS, class_idx=cls, score=score,
                                          baseline=base.to(DEV) if isinstance(base, torch.Tensor) else base)
        _compare(res, rank, c, f"spec input, {what}")          # a log-probability is the model's output itself: the same bound holds


def test_eeg_input_against_fp64_oracle():
    ref, mine = PG.eegnet_pair()
    xe = O.seeded((3, 1, 19, 2000), 91, "randn")
    n64 = copy.deepcopy(ref).double()
    x2 = xe.clone().requires_grad_(True)
    out = ref(x2)
    (g,) = torch.autograd.grad(out.gather(1, out.argmax(1, keepdim=True)).sum(), x2)
    sal = g.abs()[:, 0].contiguous()
    cols = sal.sum(1, keepdim=True).contiguous()
    # steps = 64 on 2000 time columns: per = 32, so the last TWO points sit at the clamped cut k = N
    for name, amap, steps in (("electrode x time", sal, STEPS), ("time columns", cols, STEPS), ("time columns, 64 steps", cols, 64)):
        _, ks = R.cuts(amap[0].numel(), steps)
        assert steps in (STEPS,) or sum(k == ks[-1] for k in ks) > 1
        rank, c = _reference(lambda z: n64(z), xe, amap, f"EEGNet, {name}", steps=steps)
        res = brainxai.deletion_insertion(mine, xe.to(DEV), None, amap.to(DEV), input="eeg", steps=steps)
        assert tuple(res.deletion.shape) == (3, steps + 1)
        _compare(res, rank, c, f"EEGNet, {name}, fp32")


# ---- 5. identities that need no reference -----------------------------------------------------------------------------------------------
def _host_built_curve(model, eeg, spec, which, ranks, base, steps, classes, insertion):
    """The same model's ordinary forward on torch.where inputs, one curve point at a time: [B, steps+1] probabilities (fp64, host)."""
    x = spec if which == "spec" else eeg
    N = ranks.shape[1]
    _, ks = R.cuts(N, steps)
    cols = []
    with torch.no_grad():
        for k in ks:
            below = ranks < k
            below = below.reshape(x.shape[0], 1, x.shape[2], x.shape[3]) if N == x.shape[2] * x.shape[3] else below.reshape(x.shape[0], 1, 1, x.shape[3])
            b = torch.full_like(x, base)
            xi = torch.where(below, x, b) if insertion else torch.where(below, b, x)
            out = model(eeg, xi) if which == "spec" else model(xi, spec)
            cols.append(out.float().gather(1, classes[:, None])[:, 0].double().exp().cpu())
    return torch.stack(cols, 1).numpy()


@pytest.mark.parametrize("which", ["spec", "eeg"])
def test_identities_and_max_batch(which):
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    es, ss = brainxai.saliency(mine, eeg, spec)
    amap = ss if which == "spec" else es
    kw = dict(input=which, steps=STEPS, baseline=0.5)
    a = brainxai.deletion_insertion(mine, eeg, spec, amap, max_batch=256, **kw)
    b = brainxai.deletion_insertion(mine, eeg, spec, amap, max_batch=5, **kw)
    with torch.no_grad():
        p_x = mine(eeg, spec).float().exp().gather(1, a.classes[:, None])[:, 0]
        blank = torch.full_like(spec if which == "spec" else eeg, 0.5)
        p_b = (mine(eeg, blank) if which == "spec" else mine(blank, spec)).float().exp().gather(1, a.classes[:, None])[:, 0]
    worst = max(float((a.deletion[:, 0] - a.insertion[:, -1]).abs().max()), float((a.deletion[:, 0] - p_x).abs().max()),
                float((a.deletion[:, -1] - a.insertion[:, 0]).abs().max()), float((a.deletion[:, -1] - p_b).abs().max()))
    chunks = max(float((a.deletion - b.deletion).abs().max()), float((a.insertion - b.insertion).abs().max()),
                 float((a.deletion_auc - b.deletion_auc).abs().max()), float((a.insertion_auc - b.insertion_auc).abs().max()))
    print(f"identities, {which} input: end points {worst:.2e}, max_batch 5 vs 256 {chunks:.2e}")
    assert worst <= TOL and chunks <= TOL
    assert torch.equal(a.ranks, b.ranks) and torch.equal(a.classes, b.classes)
    # the rows themselves do not depend on how the pass is cut
    x = (spec if which == "spec" else eeg).float().contiguous()
    base = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    rows = {}
    for mb in (5, 256):
        full = [[None] * (STEPS + 1) for _ in range(3)]
        for b0, nb, i0, n in X._faith_chunks(3, STEPS + 1, mb):
            assert nb * n <= mb
            out = X._faith_perturb(x, a.ranks, base, 0, b0, nb, i0, n, -(-a.ranks.shape[1] // STEPS), False, torch.float32,
                                   None if which == "spec" else amap.shape[1])
            for r in range(nb * n):
                full[b0 + r // n][i0 + r % n] = out[r]
        rows[mb] = torch.stack([torch.stack(f) for f in full])
    assert torch.equal(PG.bits(rows[5].contiguous()), PG.bits(rows[256].contiguous()))
    # the broadcast branch: every point against the ordinary two-branch forward of the same model
    for m, ins in (("deletion", False), ("insertion", True)):
        host = _host_built_curve(mine, eeg, spec, which, a.ranks, 0.5, STEPS, a.classes, ins)
        d = float(np.abs(getattr(a, m).cpu().numpy().astype(np.float64) - host).max())
        print(f"identities, {which} input, {m}: against the ordinary forward on host-built inputs {d:.2e}")
        assert d <= TOL


# ---- 6. bf16 storage ---------------------------------------------------------------------------------------------------------------------
BF16_CHUNK_BOUND = 4 * 2.80e-7       # 4 x the observed worst difference (docstring of test_bf16_storage_curves)


def test_bf16_storage_curves():
    """bf16 storage.  The perturbed rows are bit-identical to the host-built ones (test_perturbed_spectrogram_rows_bit_for_bit), so
    the curve is compared with the same GPU model's ordinary forward on torch.where inputs, one point (B = 3 rows) at a time: any
    difference comes from batch-size-dependent kernel choices (and the separate fusion-head launch).  Separately the bf16 curve stays
    within the project's derived bf16 bound of the fp32 oracle's curve (BF16_LOGP of tests/perturb_gpu.py).
    Measured on the MI355X: 2.80e-7 against the ordinary forward (bounded at 4 x that, far below the 4e-3 cap: the convolution
    kernels chosen for 51 rows and for 3 give the same bf16 activations here, what is left is the fp32 head); 7.6e-4 against the
    fp32 oracle's curve, where the derived bound is 6.6e-2."""
    ref, mine = PG.scaled_multimodal(torch.bfloat16)
    eeg, spec = PG.mm_inputs()
    r64 = copy.deepcopy(ref).double()
    amap = _oracle_maps(ref, eeg, spec)[0]["gradcam"]
    rank, c = _reference(lambda xs: r64(eeg.double(), xs), spec, amap, "spec input, gradcam (bf16 case)")
    e, s = eeg.to(DEV), spec.to(DEV)
    res = brainxai.deletion_insertion(mine, e, s, amap.to(DEV), steps=STEPS)
    assert torch.equal(res.ranks.cpu(), torch.from_numpy(rank))
    scale = PG.logp_scale(ref, eeg, spec)
    worst_host = worst_oracle = 0.0
    for m, ins in (("deletion", False), ("insertion", True)):
        got = getattr(res, m).cpu().numpy().astype(np.float64)
        host = _host_built_curve(mine, e, s, "spec", res.ranks, 0.0, STEPS, res.classes, ins)
        worst_host = max(worst_host, float(np.abs(got - host).max()))
        if np.array_equal(res.classes.cpu().numpy(), c["classes"]):
            worst_oracle = max(worst_oracle, float(np.abs(got - c[m]).max()))
    print(f"bf16 curves: against the ordinary forward on host-built inputs {worst_host:.2e}; against the fp32 oracle's curve {worst_oracle:.2e} "
          f"(bound {PG.BF16_LOGP * scale:.2e}, log-probability scale {scale:.2f})")
    assert np.array_equal(res.classes.cpu().numpy(), c["classes"])
    assert worst_oracle <= PG.BF16_LOGP * scale
    assert worst_host < 4e-3                                          # the hard cap: the project's bf16 logit figure
    assert worst_host <= BF16_CHUNK_BOUND


# ---- 7. interface ------------------------------------------------------------------------------------------------------------------------
def test_interface_forms():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    mine.train()
    for p in list(mine.parameters())[:3]:
        p.requires_grad_(False)
    before = PG.model_state(mine)
    amap = brainxai.grad_cam(mine, eeg, spec)
    full = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8)
    assert PG.model_state(mine) == before and all(m.training for m in mine.modules()) and all(p.grad is None for p in mine.parameters())
    assert isinstance(full, brainxai.FaithfulnessCurves) and tuple(full.deletion.shape) == (3, 9) and tuple(full.ranks.shape) == (3, 64 * 128)
    assert full.classes.dtype == torch.int64 and tuple(full.fractions.shape) == (9,) and float(full.fractions[0]) == 0.0 and float(full.fractions[-1]) == 1.0
    # mode subsets: the other mode's fields are None, the computed one is the same curve
    d = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8, mode="deletion")
    i = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8, mode="insertion")
    assert d.insertion is None and d.insertion_auc is None and i.deletion is None and i.deletion_auc is None
    assert float((d.deletion - full.deletion).abs().max()) <= TOL and float((i.insertion - full.insertion).abs().max()) <= TOL
    assert torch.equal(d.classes, full.classes) and torch.equal(i.classes, full.classes)
    # class_idx forms
    cls = full.classes.tolist()
    for form in (cls, torch.tensor(cls), torch.tensor(cls, device=DEV, dtype=torch.int32)):
        r = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8, class_idx=form)
        assert float((r.deletion - full.deletion).abs().max()) <= TOL and r.classes.tolist() == cls
    r4 = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8, class_idx=4)
    assert r4.classes.tolist() == [4, 4, 4]
    with torch.no_grad():
        want = mine.eval()(eeg, spec)[:, 4].exp()
        mine.train()
    assert float((r4.deletion[:, 0] - want).abs().max()) <= TOL
    # score='logprob' is the logarithm of score='prob'
    lp = brainxai.deletion_insertion(mine, eeg, spec, amap, steps=8, score="logprob")
    assert float((lp.deletion.exp() - full.deletion).abs().max()) <= TOL and float(lp.deletion.max()) <= 0.0
    assert PG.model_state(mine) == before and all(p.grad is None for p in mine.parameters())


def test_attribution_outputs_fit_as_they_are():
    _, mine = PG.scaled_multimodal()
    eeg, spec = (t.to(DEV) for t in PG.mm_inputs())
    for method in ("gradcam", "gradcam++", "layercam"):
        r = brainxai.deletion_insertion(mine, eeg, spec, brainxai.grad_cam(mine, eeg, spec, method=method), steps=8)
        assert tuple(r.deletion.shape) == (3, 9) and bool(torch.isfinite(r.deletion).all())
    for target, cells in (("eeg_model.conv1", 19 * 2000), ("eeg_model.depthwiseConv", 2000), ("eeg_model.separableConv", 2000)):
        amap = brainxai.grad_cam(mine, eeg, spec, target, class_idx=1)
        r = brainxai.deletion_insertion(mine, eeg, spec, amap, input="eeg", steps=8, class_idx=1)
        assert tuple(r.ranks.shape) == (3, cells) and tuple(r.insertion.shape) == (3, 9)
    es, ss = brainxai.saliency(mine, eeg, spec)
    rs = brainxai.deletion_insertion(mine, eeg, spec, ss, steps=8)
    re = brainxai.deletion_insertion(mine, eeg, spec, es, input="eeg", steps=8)
    assert float((rs.deletion[:, 0] - re.deletion[:, 0]).abs().max()) <= TOL
    ig_e, ig_s = brainxai.integrated_gradients(mine, (eeg, spec), n_steps=4)
    r = brainxai.deletion_insertion(mine, eeg, spec, ig_s.abs().sum(1), steps=8)
    assert bool(torch.isfinite(r.insertion_auc).all())


def test_stand_alone_models_and_lime_heatmap():
    torch.manual_seed(3)
    spec_net = brainxai.Spectrogram_Model(6).to(DEV)
    img = (np.random.default_rng(3).random((64, 96, 3)) * 255.9).astype(np.uint8)
    exp = brainxai.lime_image(spec_net, img, brainxai.grid_segments(64, 96, 4, 6), num_samples=40, max_batch=20)
    label = exp.top_labels[0]
    x = (torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0).to(DEV)
    r = brainxai.deletion_insertion(spec_net, None, x, exp.heatmap(label)[None], input="spec", steps=12, class_idx=label)
    with torch.no_grad():
        want = spec_net.eval()(x)[:, label].exp()
    assert float((r.deletion[:, 0] - want).abs().max()) <= TOL and float((r.insertion[:, -1] - want).abs().max()) <= TOL
    assert sorted(set(r.ranks[0].tolist())) == list(range(64 * 96))
    for dt in (torch.float32, torch.bfloat16):
        net = brainxai.set_compute_dtype(brainxai.Spectrogram_Model(6, in_channels=4).to(DEV), dt)
        s = torch.rand(2, 4, 64, 128, device=DEV)
        r = brainxai.deletion_insertion(net, None, s, torch.rand(2, 64, 128, device=DEV), steps=8, baseline=[0.1, 0.2, 0.3, 0.4])
        assert bool(torch.isfinite(r.deletion).all()) and net.training
    for cls in (brainxai.EEGNet, brainxai.EEGNetAttentionDeep):
        net = cls(6, Chans=19, Samples=2000).to(DEV)
        e = torch.randn(2, 1, 19, 2000, device=DEV)
        for amap in (brainxai.grad_cam(net, e, None, "conv1"), brainxai.grad_cam(net, e, None, "depthwiseConv")):
            r = brainxai.deletion_insertion(net, e, None, amap, input="eeg", steps=8, baseline=torch.zeros(19, device=DEV))
            with torch.no_grad():
                net.eval()
                want = net(e).float().exp().gather(1, r.classes[:, None])[:, 0]
                net.train()
            assert float((r.deletion[:, 0] - want).abs().max()) <= TOL and float((r.insertion[:, -1] - want).abs().max()) <= TOL
            assert net.training and all(p.requires_grad and p.grad is None for p in net.parameters())
