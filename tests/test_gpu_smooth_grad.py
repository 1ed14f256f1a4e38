"""GPU: brainxai.smooth_grad / smooth_grad_noise and the bx_smoothgrad_* entry points against the restatement of the definition
(tests/smooth_grad_ref.py): the noise against the exact Box-Muller values of the Philox words, the noise scale and the rows bit for
bit, the running sums and the three estimators against numpy fp64, and the attributions end to end against the oracle's classes run in
fp64 on the CPU.

Bounds.  Noise: |z - want| <= NOISE_C 2^-24 max(1, r), r = sqrt(-2 log u) of the element (see NOISE_C).  Sums: bit for bit numpy's fp64
sums in the same order.  Values: one fp32 rounding, plus the fp64 roundings of the sums and of the four fp64 operations of the variance
(S1^2 / n <= S2): mean and mean square |want| 2^-23 + (n-1) 2^-53 sum|term| + 2^-149, variance |want| 2^-23 + (2n+2) 2^-53 S2/n +
2^-149.  End to end, per (sample, class): the mean within TOL = 1e-3 of its maximum (the project's fp32 gradient bound, TOL of
tests/test_gpu_parity.py); with M the largest |g| over the draws, a gradient error d <= TOL M moves g^2 by 2 g d + d^2, so the mean
square is within (2 TOL + TOL^2) M^2, and the variance, which sees that in both of its terms, within twice as much.
The reference's z is the device's own dump (brainxai.smooth_grad_noise), which the noise test pins: the reference's rows are then the
device's bit for bit.  Every end-to-end case is first checked ON THE REFERENCE SIDE to discriminate: with -z, with another seed's z and
with sigma halved the fp64 reference of every kind moves by more than 100 x TOL of its maximum for every (sample, class) -- a row
kernel that dropped the noise, its sign or its scale cannot pass.  The EEG branch (ELU, average pooling: no decisions) is compared with
the plain fp64 oracle; the spectrogram branch with the same pass composed from pieces under the kernel bounds, and with the fp64
oracle whose ReLU / max-pool decisions are pinned to those of the GPU forward of the same rows (tests/golden_util.matched_oracle).
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
from tests import perturb_gpu as PG
from tests import smooth_grad_ref as R
from tests.golden_util import matched_oracle
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3
# The device's z against the exact Box-Muller value of the same (u, t), in units of 2^-24 max(1, r).  Expected from the operations: logf
# within 1 ulp and the correctly rounded sqrtf leave r within about 1 ulp = 2^-23 r; cospif / sinpif within 1-2 ulp of a value <= 1; the
# product rounds once more: a few units.  Observed worst on the MI355X over the seven shapes below: 3.097 units (eeg 19x2000; 1.241 to
# 3.077 on the others); the bound is four times that, since the device's libm may move by an ulp between releases.  A wrong counter or
# word mapping gives errors of order 2^24 units.
NOISE_OBSERVED = 3.097
NOISE_C = 4 * NOISE_OBSERVED


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# trailing shape of the input: a spectrogram [C,H,W] or an EEG input [1,Chans,T]; per = 768, 22500, 8192, 1665 (no multiple of four), 38000,
# 1 and 63 (one partial Philox block; the last block partial)
SHAPES = {"spec 2x16x24": (2, 16, 24), "spec 3x100x75": (3, 100, 75), "spec 4x32x64": (4, 32, 64), "eeg 5x333": (1, 5, 333), "eeg 19x2000": (1, 19, 2000),
          "eeg 1x1": (1, 1, 1), "eeg 7x9": (1, 7, 9)}
KB, KN = 3, 5
WINDOWS = [(0, 15), (2, 10), (14, 1)]              # all rows; from inside sample 0 to inside sample 2; the last row alone
SEED = 0x9E3779B97F4A7C15                           # both key words in use
LEVEL = 0.15


def _kernel_case(name):
    shape = SHAPES[name]
    x = O.seeded((KB, *shape), 200 + sorted(SHAPES).index(name), "randn")
    x.view(-1)[::7] = -0.0
    x[1] = 2.5                                      # a constant sample: sigma = 0, its rows are the sample itself
    return shape, x


@functools.lru_cache(maxsize=None)
def _dump(name):
    """The device's z of a kernel case, [KB, KN, *shape] on the host; computed once, never written to."""
    z = brainxai.smooth_grad_noise((KB, *SHAPES[name]), nsamples=KN, seed=SEED, device=DEV)
    assert z.shape == (KB, KN, *SHAPES[name]) and z.dtype == torch.float32 and z.is_cuda
    return z.cpu().numpy()


def _launch_rows(x, sigma, out, per, row0, rows, seed=SEED):
    L.check(L.load().bx_smoothgrad_rows(PG.p(x), PG.p(sigma), PG.p(out), KB, KN, per, seed, row0, rows, PG.stream()), "bx_smoothgrad_rows")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_noise_against_the_fp64_restatement(name):
    shape = SHAPES[name]
    per = int(np.prod(shape))
    got = _dump(name).reshape(KB, KN, per)
    want, r = R.noise(KB, KN, per, SEED, with_r=True)
    assert np.isfinite(got).all()
    ratio = float((np.abs(got.astype(np.float64) - want) / (2.0 ** -24 * np.maximum(1.0, r))).max())
    print(f"noise {name}: per {per}, worst |z - want| = {ratio:.3f} x 2^-24 max(1, r); largest |z| {np.abs(got).max():.3f}, largest r {r.max():.3f}")
    assert ratio <= NOISE_C, f"{name}: {ratio:.3f} units, bound {NOISE_C}"
    # every window's dump is the slice of the full dump, bit for bit; also on the element-by-element path (misaligned output)
    full = got.reshape(KB * KN, per)
    for row0, rows in WINDOWS:
        out = torch.full((rows, per), float("nan"), dtype=torch.float32, device=DEV)
        _launch_rows(None, None, out, per, row0, rows)
        assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(full[row0:row0 + rows])), f"{name} window {row0}..{row0 + rows}"
        mis = PG.misaligned(torch.full((rows, per), float("nan"), dtype=torch.float32, device=DEV))
        _launch_rows(None, None, mis, per, row0, rows)
        assert np.array_equal(PG.np_bits(mis.cpu().numpy()), PG.np_bits(full[row0:row0 + rows])), f"{name} window {row0}..{row0 + rows}, misaligned"
    # a shorter run is a prefix; another seed is another stream
    short = brainxai.smooth_grad_noise((KB, *shape), nsamples=3, seed=SEED, device=DEV).cpu().numpy()
    assert np.array_equal(PG.np_bits(short), PG.np_bits(_dump(name)[:, :3]))
    other = brainxai.smooth_grad_noise((KB, *shape), nsamples=KN, seed=SEED + 1, device=DEV).cpu().numpy()
    assert not np.array_equal(other, _dump(name))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sigma_bit_for_bit(name):
    shape, x = _kernel_case(name)
    per = int(np.prod(shape))
    zeros = torch.zeros(1, *shape)
    zeros.view(-1)[::2] = -0.0                       # zeros of both signs: the range is zero, its sign must not leak
    x = torch.cat([x, zeros])
    want = R.sigma(x, LEVEL)
    assert want[1] == 0 and want[3] == 0 and not np.signbit(want).any() and (per == 1 or (want[[0, 2]] > 0).all())
    for xd in (PG.dev(x), PG.misaligned(PG.dev(x))):
        sig = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.load().bx_smoothgrad_sigma(PG.p(xd), PG.p(sig), 4, per, LEVEL, PG.stream()), "bx_smoothgrad_sigma")
        assert np.array_equal(PG.np_bits(sig.cpu().numpy()), PG.np_bits(want)), f"{name}: {sig.cpu().numpy()} against {want}"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_bit_for_bit(name):
    shape, x = _kernel_case(name)
    per = int(np.prod(shape))
    sig = R.sigma(x, LEVEL)
    if per > 1:
        assert sig[1] == 0 and sig[0] > 0 and sig[2] > 0
    else:
        sig = np.array([0.5, 0.0, 1.25], dtype=np.float32)     # one element per sample has no range
    want = R.rows(x, sig, _dump(name))
    assert not np.isnan(want).any() and np.array_equal(want.reshape(KB, KN, per)[1], np.full((KN, per), 2.5, dtype=np.float32))
    xd, sd = PG.dev(x), PG.dev(sig)
    paths = [("aligned", xd, False), ("misaligned input", PG.misaligned(xd), False), ("misaligned output", xd, True)]
    for row0, rows in WINDOWS:
        for what, xin, mis_out in paths:
            out = torch.full((rows, *shape), float("nan"), dtype=torch.float32, device=DEV)
            out = PG.misaligned(out) if mis_out else out
            _launch_rows(xin, sd, out, per, row0, rows)
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), f"{name} rows {row0}..{row0 + rows}, {what}: elements left unwritten"
            assert np.array_equal(PG.np_bits(got), PG.np_bits(want[row0:row0 + rows])), f"{name} rows {row0}..{row0 + rows}, {what}"
    print(f"rows {name}: per {per} ({'16-byte and ' if per % 4 == 0 else ''}element-by-element path), windows {WINDOWS} bit for bit")


def _ratio(got, want, slack):
    bound = np.abs(want) * 2.0 ** -23 + slack + 2.0 ** -149
    return float((np.abs(got.astype(np.float64) - want) / bound).max())


@pytest.mark.parametrize("Kc", [1, 3])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accumulate_and_finish_against_numpy(name, Kc):
    shape, _ = _kernel_case(name)
    per, rows_all, n = int(np.prod(shape)), KB * KN, KN
    slot = Kc // 2
    g = O.seeded((rows_all, *shape), 7, "randn")
    g.view(-1)[::5] = -0.0
    lib = L.load()
    gd = PG.dev(g)
    SENTINEL = 7.25

    def run(splits, mis=False):
        S1 = torch.full((KB, Kc, per), SENTINEL, dtype=torch.float64, device=DEV)
        S2 = torch.full((KB, Kc, per), SENTINEL, dtype=torch.float64, device=DEV)
        S1[:, slot], S2[:, slot] = 0.0, 0.0
        for row0, rows in splits:
            gs = gd[row0:row0 + rows].contiguous()
            L.check(lib.bx_smoothgrad_accumulate(PG.p(PG.misaligned(gs) if mis else gs), PG.p(S1), PG.p(S2), KB, n, per, Kc, slot, row0, rows, PG.stream()),
                    "bx_smoothgrad_accumulate")
        return S1, S2
    one, two = run([(0, rows_all)]), run([(0, 7), (7, rows_all - 7)])                    # row 7 is inside sample 1
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]), f"{name}: two calls split inside a sample differ from one call"
    mis = run([(0, 7), (7, rows_all - 7)], mis=True)                                     # element by element, whatever per % 4
    assert torch.equal(one[0].view(torch.int64), mis[0].view(torch.int64)) and torch.equal(one[1].view(torch.int64), mis[1].view(torch.int64)), \
        f"{name}: a misaligned g changes the sums"
    others = [k for k in range(Kc) if k != slot]
    assert bool((one[0][:, others] == SENTINEL).all()) and bool((one[1][:, others] == SENTINEL).all()), "the slots of other classes were touched"
    w1, w2, abs1 = R.accumulate(g.numpy(), KB, n)
    assert np.array_equal(one[0][:, slot].cpu().numpy(), w1[:, 0]) and np.array_equal(one[1][:, slot].cpu().numpy(), w2[:, 0]), \
        f"{name}: the fp64 sums are not numpy's in the same order"
    spec = name.startswith("spec")
    Cc, HW = (shape[0], shape[1] * shape[2]) if spec else (1, per)
    S1, S2 = one[0].clone(), one[1].clone()
    S1[:, others], S2[:, others] = 0.0, 0.0
    line = []
    for kind in R.KINDS:
        values = torch.full((KB, Kc, *shape), float("nan"), dtype=torch.float32, device=DEV)
        amap = torch.full((KB, Kc, shape[1], shape[2]), float("nan"), dtype=torch.float32, device=DEV)
        L.check(lib.bx_smoothgrad_finish(PG.p(S1), PG.p(S2), PG.p(values), PG.p(amap), KB * Kc, Cc, HW, n, X._SMOOTHGRAD_KINDS[kind], PG.stream()),
                "bx_smoothgrad_finish")
        values, amap = values.cpu().numpy(), amap.cpu().numpy()
        assert not np.isnan(values).any() and not np.isnan(amap).any()
        want = R.finish64(w1[:, 0], w2[:, 0], n, kind)
        slack = {"smoothgrad": (n - 1) * 2.0 ** -53 * abs1 / n, "smoothgrad_sq": (n - 1) * 2.0 ** -53 * w2[:, 0] / n,
                 "vargrad": (2 * n + 2) * 2.0 ** -53 * w2[:, 0] / n}[kind]
        rv = _ratio(values[:, slot].reshape(KB, per), want, slack)
        assert rv <= 1.0, f"{name} {kind}: values {rv:.3f} x the bound"
        assert not values[:, others].any(), "an untouched slot (zero sums) must give zero values"
        ref_vals, ref_map = R.finish(w1, w2, n, kind, shape)
        same = bool(np.array_equal(values[:, slot], ref_vals[:, 0]))
        assert np.array_equal(amap, np.abs(values).max(2)), f"{name} {kind}: the map is not the channel maximum of |values|"
        assert not np.signbit(amap).any() and (kind == "smoothgrad" or not np.signbit(values).any())
        line.append(f"{kind} {rv:.3f} x bound (bit for bit the restatement's: {same})")
    print(f"accumulate / finish {name} Kc={Kc}: split == one call and S1, S2 == numpy bit for bit; values: " + "; ".join(line))


@pytest.mark.parametrize("n", [1, 4])
def test_exact_cases(n):
    """n = 1 with any gradients, n = 4 with gradients equal across the draws of a sample: S1 = n g and S2 = n g^2 fit in 53 bits (g^2 has
    at most 48), S1 * S1 / n = n g^2 = S2 exactly: the mean is the gradient bit for bit and the variance exactly 0."""
    shape, Bn = (2, 16, 24), 3
    per = int(np.prod(shape))
    g1 = O.seeded((Bn, 1, *shape), 17, "randn")
    assert bool((g1 != 0).all())                    # a sum that starts at +0.0 cannot return a zero's sign
    g = g1.expand(Bn, n, *shape).reshape(Bn * n, *shape).contiguous()
    lib = L.load()
    S1, S2 = (torch.zeros(Bn, 1, per, dtype=torch.float64, device=DEV) for _ in range(2))
    L.check(lib.bx_smoothgrad_accumulate(PG.p(PG.dev(g)), PG.p(S1), PG.p(S2), Bn, n, per, 1, 0, 0, Bn * n, PG.stream()), "bx_smoothgrad_accumulate")
    got = {}
    for kind in R.KINDS:
        values = torch.full((Bn, 1, *shape), float("nan"), dtype=torch.float32, device=DEV)
        amap = torch.full((Bn, 1, *shape[1:]), float("nan"), dtype=torch.float32, device=DEV)
        L.check(lib.bx_smoothgrad_finish(PG.p(S1), PG.p(S2), PG.p(values), PG.p(amap), Bn, shape[0], shape[1] * shape[2], n, X._SMOOTHGRAD_KINDS[kind],
                                         PG.stream()), "bx_smoothgrad_finish")
        got[kind] = values.cpu().numpy()[:, 0], amap.cpu().numpy()[:, 0]
    g1 = g1.numpy()[:, 0]
    assert np.array_equal(PG.np_bits(got["smoothgrad"][0]), PG.np_bits(g1)) and np.array_equal(PG.np_bits(got["smoothgrad"][1]), PG.np_bits(np.abs(g1).max(1)))
    assert np.array_equal(PG.np_bits(got["smoothgrad_sq"][0]), PG.np_bits((g1.astype(np.float64) ** 2).astype(np.float32)))
    assert not got["vargrad"][0].any() and not got["vargrad"][1].any() and not np.signbit(got["vargrad"][0]).any()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
EN, ESEED = 6, 3


def _device_noise(x, n=EN, seed=ESEED):
    return brainxai.smooth_grad_noise(tuple(x.shape), nsamples=n, seed=seed, device=DEV).cpu().numpy()


def _guard(what, f64, want, x, z, sig, other, input):
    """Reference side alone: the inputs discriminate the sign, the stream and the scale of the noise, for every kind."""
    moved = {"-z": R.values(f64, x, -z, sig, other, input), "another seed": R.values(f64, x, _device_noise(x, seed=ESEED + 1), sig, other, input),
             "sigma halved": R.values(f64, x, z, (sig * np.float32(0.5)).astype(np.float32), other, input)}
    least = {}
    for how, alt in moved.items():
        for kind, a, w in zip(R.KINDS, alt, want):
            least[how, kind] = float((GG.per_pair_max(a - w) / GG.per_pair_max(w)).min())
    print(f"{what}: the reference moves by (least over (sample, class), of its maximum) " + ", ".join(f"{how} / {kind} {v:.3f}" for (how, kind), v in least.items()))
    for key, v in least.items():
        assert v > 100 * TOL, f"{what}: {key} moves the reference by only {v:.3e}"


@functools.lru_cache(maxsize=None)
def _eeg_case(kind):
    """(mine, x, other, z, sigma, (mean, sq, var) fp64 [B,K,1,Chans,T], M fp64 [B,K]); computed once, never written to."""
    _, mine, f64, x, other = GG.eeg_models(kind)
    z, sig = _device_noise(x), R.sigma(x, LEVEL)
    *want, M = R.values(f64, x, z, sig, other, "eeg", with_gmax=True)
    _guard(f"smooth_grad eeg input, {kind}", f64, want, x, z, sig, other, "eeg")
    return mine, x, other, z, sig, tuple(want), M


def _check_kinds(what, results, want, M):
    """results: kind -> values tensor; want (mean, sq, var) fp64; M [B,K].  The end-to-end bounds of the module docstring."""
    line = []
    for kind, w in zip(R.KINDS, want):
        got = results[kind].detach().double().cpu()
        assert got.shape == w.shape and bool(torch.isfinite(got).all())
        err = GG.per_pair_max(got - w)
        bound = {"smoothgrad": TOL * GG.per_pair_max(w), "smoothgrad_sq": (2 * TOL + TOL * TOL) * M * M, "vargrad": 2 * (2 * TOL + TOL * TOL) * M * M}[kind]
        ratio = float((err / bound).max())
        line.append(f"{kind} {ratio:.3e} x bound (error {float((err / GG.per_pair_max(w)).max()):.3e} of the maximum)")
        assert ratio <= 1.0, f"{what}: {kind} {ratio:.3f} x the bound"
    print(f"{what}: " + "; ".join(line))


@pytest.mark.parametrize("kind", ["eegnet", "multimodal", "deep"])
def test_eeg_input_against_the_fp64_oracle(kind):
    mine, x, other, z, sig, want, M = _eeg_case(kind)
    results = {}
    for k in R.KINDS:
        res = brainxai.smooth_grad(mine, x.to(DEV), None if other is None else other.to(DEV), input="eeg", nsamples=EN, noise_level=LEVEL, kind=k,
                                   class_idx="all", seed=ESEED, return_parts=True)
        assert res.values.shape == (2, 6, 1, 19, 2000) and res.attribution.shape == (2, 6, 19, 2000) and res.classes is None
        assert (res.nsamples, res.kind, res.seed) == (EN, k, ESEED)
        assert np.array_equal(PG.np_bits(res.sigma.cpu().numpy()), PG.np_bits(sig))
        assert torch.equal(res.attribution, res.values[:, :, 0].abs())
        results[k] = res.values
    _check_kinds(f"smooth_grad eeg input, {kind}", results, want, M)


def _spec_case():
    eeg, spec = GG.mm_inputs()
    return eeg, spec, _device_noise(spec), R.sigma(spec, LEVEL)


def _composed(model, eeg, spec, z_d, sig_d, max_batch):
    """The same pass from existing pieces: rows x + sigma * z in torch fp32 (a product and a sum, each its own kernel), the library's
    forward, torch.autograd.grad with the pass composition of smooth_grad, sums of g and g^2 in torch fp64 in ascending draw order.
    -> (rows fp32 [B*n,...], S1, S2, sum |g|, each fp64 [B,K,C,H,W])."""
    B, n = z_d.shape[:2]
    net = model.spectrogram_model
    K = int(model.fc2.out_features)
    with X._eval_frozen(model):
        with torch.no_grad():
            fixed = X._fixed_branch(model, eeg, True)
        nz = sig_d[:, None, None, None, None] * z_d
        r_all = (spec[:, None] + nz).reshape(B * n, *spec.shape[1:])
        max_rows = X._row_cap(spec, "spec", net.compute_dtype, max_batch)
        S1 = torch.zeros(B, K, *spec.shape[1:], dtype=torch.float64, device=spec.device)
        S2, A1 = torch.zeros_like(S1), torch.zeros_like(S1)
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
                    j, t = row0 + q, g[q].double()
                    S1[j // n, c] += t
                    S2[j // n, c] += t * t
                    A1[j // n, c] += t.abs()
    return r_all, S1, S2, A1


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_spec_input_against_the_same_pass_from_pieces(dt):
    """The gradients are then the same launches on the same bits: what remains is the bound of the finish kernel."""
    _, mine = PG.scaled_multimodal(dt)
    eeg, spec, z, sig = _spec_case()
    eeg_d, spec_d = eeg.to(DEV), spec.to(DEV)
    max_batch, n = 5, EN                                                  # three passes; the first two end inside a sample
    r_all, S1, S2, A1 = _composed(mine, eeg_d, spec_d, PG.dev(z), PG.dev(sig), max_batch)
    assert np.array_equal(PG.np_bits(r_all.cpu().numpy()), PG.np_bits(R.rows(spec, sig, z))), "the composed rows are not the restatement's"
    S1, S2, A1 = S1.cpu().numpy(), S2.cpu().numpy(), A1.cpu().numpy()
    assert float(np.abs(S1).max()) > 0
    line = []
    for kind in R.KINDS:
        res = brainxai.smooth_grad(mine, eeg_d, spec_d, input="spec", nsamples=n, noise_level=LEVEL, kind=kind, class_idx="all", seed=ESEED,
                                   max_batch=max_batch, return_parts=True)
        assert res.values.shape == (2, 6, 4, 32, 64) and res.attribution.shape == (2, 6, 32, 64)
        want = R.finish64(S1, S2, n, kind)
        slack = {"smoothgrad": (n - 1) * 2.0 ** -53 * A1 / n, "smoothgrad_sq": (n - 1) * 2.0 ** -53 * S2 / n, "vargrad": (2 * n + 2) * 2.0 ** -53 * S2 / n}[kind]
        vals = res.values.cpu().numpy()
        rv = _ratio(vals, want, slack)
        same = bool(np.array_equal(vals, want.astype(np.float32)))
        assert torch.equal(res.attribution, res.values.abs().amax(2))
        line.append(f"{kind} {rv:.3f} x bound (bit for bit: {same})")
        assert rv <= 1.0, f"{kind}: {rv:.3f} x the bound"
    print(f"smooth_grad spec input vs composed pass, {dt}: " + "; ".join(line))


def test_spec_input_against_the_fp64_oracle():
    ref, mine = PG.scaled_multimodal()
    eeg, spec, z, sig = _spec_case()
    B, n = z.shape[:2]
    f64 = copy.deepcopy(ref).double().eval()
    plain = R.values(f64, spec, z, sig, eeg, "spec")
    _guard("smooth_grad spec input, multimodal", f64, plain, spec, z, sig, eeg, "spec")
    kw = dict(input="spec", nsamples=n, noise_level=LEVEL, class_idx="all", seed=ESEED, return_parts=True)
    results = {}
    keep = ops.keep_block_activations(mine)
    try:                                                                  # one pass of 12 rows: the last forward, whose activations keep holds
        results["smoothgrad"] = brainxai.smooth_grad(mine, eeg.to(DEV), spec.to(DEV), kind="smoothgrad", **kw).values
        torch.cuda.synchronize()
    finally:
        ops.keep_block_activations(mine, on=False)
    for kind in R.KINDS[1:]:                                              # the same rows, hence the same decisions
        results[kind] = brainxai.smooth_grad(mine, eeg.to(DEV), spec.to(DEV), kind=kind, **kw).values
    rows = torch.from_numpy(R.rows(spec, sig, z))
    eeg_rep = eeg.repeat_interleave(n, dim=0)
    twin, flips = matched_oracle(O, ref, (eeg_rep, rows), keep, "smooth_grad spec input")
    xi = rows.double().requires_grad_(True)
    y = twin(eeg_rep.double(), xi)
    want = tuple(torch.zeros_like(plain[0]) for _ in range(3))
    M = torch.zeros(B, y.shape[1], dtype=torch.float64)
    for c in range(y.shape[1]):
        (g,) = torch.autograd.grad(y[:, c].sum(), xi, retain_graph=True)
        g = g.reshape(B, n, *spec.shape[1:])
        s1, s2 = g.sum(1), (g * g).sum(1)
        want[0][:, c], want[1][:, c], want[2][:, c] = s1 / n, s2 / n, torch.clamp((s2 - s1 * s1 / n) / n, min=0.0)
        M[:, c] = g.abs().flatten(1).max(1).values
    print(f"smooth_grad spec input, multimodal 4x32x64: {len(flips)} decision flips")
    _check_kinds("smooth_grad spec input, multimodal 4x32x64, decision-matched fp64 oracle", results, want, M)


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_repeatable_prefix_and_max_batch():
    mine, eeg, spec = GG.iface()
    kw = dict(input="eeg", nsamples=EN, class_idx="all", seed=ESEED)
    a = brainxai.smooth_grad(mine, eeg, spec, return_parts=True, **kw)
    b = brainxai.smooth_grad(mine, eeg, spec, **kw)
    assert torch.equal(a.attribution, b), "two calls differ"
    assert not torch.equal(a.attribution, brainxai.smooth_grad(mine, eeg, spec, input="eeg", nsamples=EN, class_idx="all", seed=ESEED + 1))
    small = brainxai.smooth_grad(mine, eeg, spec, max_batch=5, return_parts=True, **kw)
    err = GG.worst(small.values, a.values)
    print(f"smooth_grad max_batch 5 vs 256: {err:.3e} of the per-(sample, class) maximum, bit for bit: {torch.equal(small.values, a.values)}")
    assert err <= TOL
    # nsamples = 3 sees the first three draws of nsamples = 6: the mean over the first three rows of the dumped noise, from pieces
    z, sig = PG.dev(_device_noise(eeg.cpu())), a.sigma
    three = brainxai.smooth_grad(mine, eeg, spec, input="eeg", nsamples=3, class_idx=2, seed=ESEED, return_parts=True)
    r = (eeg[:, None] + sig[:, None, None, None, None] * z[:, :3]).reshape(6, 1, 19, 2000).requires_grad_(True)
    with X._eval_frozen(mine):
        y = mine(r, spec.repeat_interleave(3, dim=0))
        (g,) = torch.autograd.grad(y[:, 2].sum(), r)
    gg = g.double().reshape(2, 3, 1, 19, 2000)
    err3 = GG.worst(three.values[:, None], gg.mean(1)[:, None])
    flipped = gg * torch.tensor([1.0, 1.0, -1.0], device=DEV, dtype=torch.float64).view(1, 3, 1, 1, 1)
    wrong = GG.worst(three.values[:, None], flipped.mean(1)[:, None])
    print(f"smooth_grad nsamples 3 against the first three dumped draws from pieces: {err3:.3e} of the maximum (one draw's sign flipped: {wrong:.3e})")
    assert err3 <= TOL < wrong
    s_kw = dict(input="spec", nsamples=4, class_idx="all", seed=1, kind="vargrad")
    assert torch.equal(brainxai.smooth_grad(mine, eeg, spec, **s_kw), brainxai.smooth_grad(mine, eeg, spec, **s_kw))


def test_class_forms():
    mine, eeg, spec = GG.iface()
    for input, shape in (("eeg", (19, 2000)), ("spec", (32, 64))):
        kw = dict(input=input, nsamples=4, seed=5, kind="smoothgrad_sq" if input == "spec" else "smoothgrad")
        every = brainxai.smooth_grad(mine, eeg, spec, class_idx="all", return_parts=True, **kw)
        assert every.attribution.shape == (2, 6, *shape) and every.out.shape == (2, 6) and every.classes is None
        top = brainxai.smooth_grad(mine, eeg, spec, return_parts=True, **kw)
        assert top.attribution.shape == (2, *shape) and top.values.shape[0] == 2 and top.values.dim() == 4
        assert torch.equal(top.classes, every.out.argmax(1)) and torch.equal(top.out, every.out)
        for b in range(2):
            assert torch.equal(top.attribution[b], every.attribution[b, int(top.classes[b])])
            assert torch.equal(top.values[b], every.values[b, int(top.classes[b])])
        for c in range(6):
            one = brainxai.smooth_grad(mine, eeg, spec, class_idx=c, **kw)
            assert torch.equal(one, every.attribution[:, c]), f"{input}: 'all' differs from the call for class {c}"
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.smooth_grad(mine, eeg, spec, class_idx=form, return_parts=True, **kw)
            assert per.classes.tolist() == [4, 1]
            assert torch.equal(per.attribution[0], every.attribution[0, 4]) and torch.equal(per.attribution[1], every.attribution[1, 1])


def test_stdev_modes_and_downstream():
    mine, eeg, spec = GG.iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        level = brainxai.smooth_grad(mine, eeg, spec, input="spec", nsamples=4, seed=2, class_idx="all", return_parts=True)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    assert level.sigma.shape == (2,) and np.array_equal(PG.np_bits(level.sigma.cpu().numpy()), PG.np_bits(R.sigma(spec.cpu(), 0.15))), "the default noise level is 0.15"
    # the absolute scale: per sample as a tensor, and one number for all
    per = brainxai.smooth_grad(mine, eeg, spec, input="spec", nsamples=4, seed=2, class_idx="all", stdev=level.sigma, return_parts=True)
    assert torch.equal(per.values, level.values) and torch.equal(per.sigma, level.sigma)
    s0 = float(level.sigma[0])
    one = brainxai.smooth_grad(mine, eeg, spec, input="spec", nsamples=4, seed=2, class_idx="all", stdev=s0, return_parts=True)
    assert torch.equal(one.sigma, torch.full((2,), s0, device=DEV))
    assert GG.worst(one.values[:1], level.values[:1]) <= TOL, "sample 0 has the same scale in both calls"
    both = brainxai.smooth_grad(mine, eeg, spec, input="spec", nsamples=4, seed=2, class_idx="all", stdev=torch.tensor([s0, s0], dtype=torch.float64))
    assert torch.equal(both, one.attribution)
    # without noise every draw is the plain gradient of the same row: the variance stays within its end-to-end bound of zero
    still = brainxai.smooth_grad(mine, eeg, spec, input="eeg", nsamples=4, class_idx="all", stdev=0.0, return_parts=True)
    novar = brainxai.smooth_grad(mine, eeg, spec, input="eeg", nsamples=4, class_idx="all", noise_level=0, kind="vargrad")
    M = float(still.values.abs().max())
    print(f"smooth_grad without noise: largest variance {float(novar.max()):.3e}, largest gradient {M:.3e}")
    assert M > 0 and float(novar.max()) <= 2 * (2 * TOL + TOL * TOL) * M * M
    # the maps drop into the faithfulness tools as they are
    for input in ("eeg", "spec"):
        for kind in R.KINDS:
            res = brainxai.smooth_grad(mine, eeg, spec, input=input, nsamples=4, seed=2, kind=kind, return_parts=True)
            assert torch.equal(res.attribution, res.values.abs().amax(1))
        ranks = brainxai.attribution_ranks(res.attribution)
        assert ranks.shape == (2, res.attribution[0].numel())
        curves = brainxai.deletion_insertion(mine, eeg, spec, res.attribution, input=input, steps=4)
        assert torch.equal(curves.ranks, ranks) and bool(torch.isfinite(curves.deletion).all()) and bool(torch.isfinite(curves.insertion).all())


def test_stand_alone_spectrogram_model():
    mine, eeg, spec = GG.iface()
    sm = mine.spectrogram_model
    res = brainxai.smooth_grad(sm, None, spec, nsamples=4, class_idx="all", seed=2, return_parts=True)
    assert res.values.shape == (2, 6, 4, 32, 64) and res.attribution.shape == (2, 6, 32, 64) and bool(torch.isfinite(res.values).all())
    assert float(res.values.abs().max()) > 0 and torch.equal(res.attribution, res.values.abs().amax(2))
    with torch.no_grad():
        assert torch.equal(res.out, sm(spec).float())
    assert torch.equal(res.attribution[:, 3], brainxai.smooth_grad(sm, None, spec, nsamples=4, class_idx=3, seed=2))
    var = brainxai.smooth_grad(sm, None, spec, nsamples=4, class_idx="all", seed=2, kind="vargrad", return_parts=True)
    sq = brainxai.smooth_grad(sm, None, spec, nsamples=4, class_idx="all", seed=2, kind="smoothgrad_sq", return_parts=True)
    resid = (sq.values.double() - res.values.double() ** 2 - var.values.double()).abs().max()
    assert float(resid) <= 4 * 2.0 ** -24 * float(sq.values.max()), "variance = mean square - mean^2"
