"""GPU: brainxai.infidelity / sensitivity_max and the bx_infidelity_* / bx_sensitivity_* entry points against the restatement of the
definitions (tests/infidelity_ref.py): the rows bit for bit given the device's own dumped noise, the uniform draws and rows bit for
bit from the Philox words, the dots, the finish and the distances against numpy fp64, and the metrics end to end against the same pass
composed from pieces and against the oracle's classes run in fp64 on the CPU.

Bounds, with u = 2^-53.
Dot.  Every product (double)I (double)Phi is exact; a sum of N terms in any order is within (N - 1) u sum|term| of the exact sum.  The
device's order (cells / 1024 terms per thread, then an 8-level tree) and numpy's pairwise sum both stay far inside that:
|d - numpy| <= cells u sum|I Phi| =: ed.  The restatement's z is the device's own dump, so nothing is added for z.
Finish.  Host and device perform the same IEEE fp64 operations in the same order (the file is built without contraction), so the results
are expected bit for bit; the assertion does not rely on it.  With S = sum_k d^2, each of the n products and n - 1 sums of
sum_k d Delta moves it by at most (n + 1) u sum|d Delta|, the same relative to S for S, and the quotient rounds once:
ebeta = ((n + 1) u sum|d Delta|) / S + |beta| (n + 3) u (0 without normalize).  t = beta d - Delta is two more roundings:
et = ebeta |d| + 2 u (|beta d| + |Delta|); the square, the n sums and the quotient: E = (1/n) sum_k (2 |t| et + et^2) + (n + 3) u infid.
Two results that are both within E of the exact value differ by at most 2 E.  With dots that carry ed, et grows by |beta| ed.
Distance.  The difference of two floats is exact in fp64; the square, the P sums and the root: |dist - exact| <= dist (P / 2 + 2) u,
twice that between two results.  The maximum and one quotient: 2 u more.
End to end, fp64 oracle: a score is within e = TOL = 1e-5 of the oracle's (tests/perturb_gpu.py: probabilities, and the same bound for
log-probabilities, the model's output itself); (beta d - Delta)^2 then moves by at most 2 |beta d - Delta| e + e^2, and infid by the mean
of that over the draws, plus the dot's share above.  Every such case is first checked ON THE REFERENCE SIDE to discriminate: with -z,
with another seed's z, with sigma halved and with Phi negated the fp64 reference moves by more than 100 x the bound for every (sample,
class) -- a kernel that dropped the noise, its sign, its scale or the attribution cannot pass.  Phi is the fp64 input gradient of the
score at noise level 0.15 (1.0 for the multimodal model), and the score is the log-probability: with probabilities the least likely class of EEGNet (p ~ 1e-3) has
drops so small against e that -z moves its reference by only 40 bounds and -Phi by 18 (10 and 134 at level 0.05); with
log-probabilities every class moves by more than 5000.  Probabilities are compared in the composed-pass test.  Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
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
from tests import infidelity_ref as R
from tests import perturb_gpu as PG
from tests import smooth_grad_ref as SG
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
TOL = PG.TOL

# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# trailing shape of the input: a spectrogram [C,H,W] (HW = 384; 35: the last Philox block partial, element cells of channels 1 and 2
# straddle two blocks; 7500; 2048) or an EEG input [1,Chans,T] (per = 1665, no multiple of four; 63; 1; 38000)
SHAPES = {"spec 2x16x24": (2, 16, 24), "spec 3x5x7": (3, 5, 7), "spec 3x100x75": (3, 100, 75), "spec 4x32x64": (4, 32, 64),
          "eeg 5x333": (1, 5, 333), "eeg 7x9": (1, 7, 9), "eeg 1x1": (1, 1, 1), "eeg 19x2000": (1, 19, 2000)}
KB, KN = 3, 5
WINDOWS = [(0, 15), (2, 10), (14, 1)]              # all rows; from inside sample 0 to inside sample 2; the last row alone
SEED = 0x9E3779B97F4A7C15                           # both key words in use
LEVEL = 0.15
FORMS = ["element", "grouped"]                      # grouped: a pixel with all its channels / a time column with all its electrodes


def _is_eeg(name):
    return name.startswith("eeg")


def _cell_shape(name, grouped):
    shape = SHAPES[name]
    if not grouped:
        return shape
    return (shape[2],) if _is_eeg(name) else shape[1:]


def _kernel_case(name):
    shape = SHAPES[name]
    x = O.seeded((KB, *shape), 300 + sorted(SHAPES).index(name), "randn")
    x.view(-1)[::7] = -0.0
    x[1] = 2.5                                      # a constant sample: sigma = 0, its rows are the sample itself
    sig = SG.sigma(x, LEVEL)
    if int(np.prod(shape)) == 1:
        sig = np.array([0.5, 0.0, 1.25], dtype=np.float32)     # one element per sample has no range
    assert sig[1] == 0 and sig[0] > 0 and sig[2] > 0
    return shape, x, sig


@functools.lru_cache(maxsize=None)
def _dump(name, grouped):
    """The device's z over the cells of a kernel case, [KB, KN, cells] on the host; computed once, never written to."""
    cs = _cell_shape(name, grouped)
    z = brainxai.smooth_grad_noise((KB, *cs), nsamples=KN, seed=SEED, device=DEV)
    assert z.shape == (KB, KN, *cs) and z.dtype == torch.float32
    return z.cpu().numpy().reshape(KB, KN, -1)


def _chunks_of_window(row0, rows):
    """A window of global rows j = b * n + k as chunk calls (b0, nb, n0, n) of one sample each, with the offset of their first row."""
    out, j = [], row0
    while j < row0 + rows:
        b, k = divmod(j, KN)
        n = min(KN - k, row0 + rows - j)
        out.append((j - row0, b, 1, k, n))
        j += n
    return out


def _launch_inf_rows(name, xd, sd, out, grouped, dt, b0, nb, n0, n):
    lib, shape = L.load(), SHAPES[name]
    if _is_eeg(name):
        L.check(lib.bx_infidelity_rows_eeg(PG.p(xd), PG.p(sd), PG.p(out), KB, shape[1], shape[2], int(grouped), KN, b0, nb, n0, n, SEED, PG.stream()),
                "bx_infidelity_rows_eeg")
    else:
        L.check(lib.bx_infidelity_rows_spec(PG.p(xd), PG.p(sd), PG.p(out), KB, *shape, 8, int(grouped), KN, b0, nb, n0, n, SEED, ops.bx_dtype(dt), PG.stream()),
                "bx_infidelity_rows_spec")


def _layout(want, name, dt):
    """The restatement's rows [R,...] fp32 in the layout the kernel writes: EEG rows as they are; spectrogram rows NHWC, 8 channels, dt
    (torch's fp32 -> bf16 conversion rounds to nearest even), channels C..7 zero."""
    t = torch.from_numpy(want)
    if _is_eeg(name):
        return t
    Rr, Cc, H, W = t.shape
    out = torch.zeros(Rr, H, W, 8, dtype=dt)
    out[..., :Cc] = t.permute(0, 2, 3, 1).to(dt)
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_infidelity_rows_bit_for_bit(name, form):
    grouped = form == "grouped"
    shape, x, sig = _kernel_case(name)
    eeg = _is_eeg(name)
    want32 = R.rows(x, sig, _dump(name, grouped), grouped, eeg)                          # [15, ...]
    assert not np.isnan(want32).any() and np.array_equal(want32.reshape(KB, KN, -1)[1], np.full((KN, int(np.prod(shape))), 2.5, dtype=np.float32))
    xd, sd = PG.dev(x), PG.dev(sig)
    row_shape = shape if eeg else (shape[1], shape[2], 8)
    for dt in ([torch.float32] if eeg else [torch.float32, torch.bfloat16]):
        want = _layout(want32, name, dt)
        inputs = [("aligned", xd, False), ("misaligned input", PG.misaligned(xd), False)] + ([("misaligned output", xd, True)] if eeg else [])
        for what, xin, mis_out in inputs:
            for row0, rows in WINDOWS:                                                   # a window of rows, sample by sample
                out = torch.full((rows, *row_shape), float("nan"), dtype=dt, device=DEV)
                out = PG.misaligned(out) if mis_out else out
                for at, b0, nb, n0, n in _chunks_of_window(row0, rows):
                    _launch_inf_rows(name, xin, sd, out[at:at + n], grouped, dt, b0, nb, n0, n)
                PG.assert_same_rows(out.cpu(), want[row0:row0 + rows], f"{name} {form} {dt} rows {row0}..{row0 + rows}, {what}", None if eeg else shape[0])
            for b0, nb, n0, n in ((0, KB, 0, KN), (1, 2, 1, 3), (2, 1, 4, 1)):           # rectangles of samples x draws: the chunks of a sweep
                out = torch.full((nb * n, *row_shape), float("nan"), dtype=dt, device=DEV)
                out = PG.misaligned(out) if mis_out else out
                _launch_inf_rows(name, xin, sd, out, grouped, dt, b0, nb, n0, n)
                pick = [b * KN + k for b in range(b0, b0 + nb) for k in range(n0, n0 + n)]
                PG.assert_same_rows(out.cpu(), want[pick], f"{name} {form} {dt} chunk {(b0, nb, n0, n)}, {what}", None if eeg else shape[0])
        if not eeg:
            assert not out.cpu().view(torch.int16 if dt == torch.bfloat16 else torch.int32)[..., 4:].any(), "channels 4..7 must hold zero bits"
    print(f"infidelity rows {name} {form}: windows {WINDOWS} and three chunks bit for bit, fp32{'' if eeg else ' and bf16'} storage")


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_uniform_draws_and_rows_bit_for_bit(name):
    shape, x, _ = _kernel_case(name)
    per = int(np.prod(shape))
    lib = L.load()
    u = R.uniform(KB, KN, per, SEED)
    assert (u >= -1).all() and (u < 1).all()
    radius = np.array([0.02, 0.0, 1.5], dtype=np.float32)
    want = R.uniform_rows(x, radius, u.reshape(KB, KN, *shape)).reshape(KB * KN, per)
    assert np.array_equal(want.reshape(KB, KN, per)[1], np.full((KN, per), 2.5, dtype=np.float32)), "radius 0 returns the sample itself"
    xd, rd = PG.dev(x), PG.dev(radius)
    full = u.reshape(KB * KN, per)
    for row0, rows in WINDOWS:
        for mis in (False, True):
            out = torch.full((rows, per), float("nan"), dtype=torch.float32, device=DEV)
            out = PG.misaligned(out) if mis else out
            L.check(lib.bx_sensitivity_rows(None, None, PG.p(out), KB, KN, per, SEED, row0, rows, PG.stream()), "bx_sensitivity_rows")
            assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(full[row0:row0 + rows])), f"{name} draws {row0}..{row0 + rows}, misaligned {mis}"
        for what, xin, mis_out in (("aligned", xd, False), ("misaligned input", PG.misaligned(xd), False), ("misaligned output", xd, True)):
            out = torch.full((rows, per), float("nan"), dtype=torch.float32, device=DEV)
            out = PG.misaligned(out) if mis_out else out
            L.check(lib.bx_sensitivity_rows(PG.p(xin), PG.p(rd), PG.p(out), KB, KN, per, SEED, row0, rows, PG.stream()), "bx_sensitivity_rows")
            got = out.cpu().numpy()
            assert not np.isnan(got).any(), f"{name} rows {row0}..{row0 + rows}, {what}: elements left unwritten"
            assert np.array_equal(PG.np_bits(got), PG.np_bits(want[row0:row0 + rows])), f"{name} rows {row0}..{row0 + rows}, {what}"
    out = torch.empty(KB * KN, per, dtype=torch.float32, device=DEV)
    L.check(lib.bx_sensitivity_rows(None, None, PG.p(out), KB, KN, per, SEED + 1, 0, KB * KN, PG.stream()), "bx_sensitivity_rows")
    assert per < 8 or not np.array_equal(out.cpu().numpy(), full), "another seed is another stream"
    z = brainxai.smooth_grad_noise((KB, *shape), nsamples=KN, seed=SEED, device=DEV).cpu().numpy().reshape(KB * KN, per)
    assert not np.array_equal(R.uniform(KB, KN, per, SEED, word3=0).reshape(KB * KN, per), full) and not np.array_equal(z, full)


@pytest.mark.parametrize("Kc", [1, 5])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_dot_against_numpy_and_across_windows(name, form, Kc):
    grouped = form == "grouped"
    _, _, sig = _kernel_case(name)
    z = _dump(name, grouped)
    cells = z.shape[2]
    phi = O.seeded((KB, Kc, cells), 23, "randn")
    phi.view(-1)[::5] = -0.0
    I = R.perturbation(sig, z)
    want, absum = R.dots(I, phi.numpy())
    lib, sd = L.load(), PG.dev(sig)

    def run(ph, row0, rows):
        d = torch.full((KB, Kc, KN), float("nan"), dtype=torch.float64, device=DEV)
        L.check(lib.bx_infidelity_dot(PG.p(ph), PG.p(sd), PG.p(d), KB, KN, cells, Kc, SEED, row0, rows, PG.stream()), "bx_infidelity_dot")
        return d.cpu().numpy()
    full = run(PG.dev(phi), 0, KB * KN)
    assert np.isfinite(full).all() and not full[1].any(), "sigma = 0 gives d = 0"
    bound = cells * U * absum
    ratio = float((np.abs(full - want)[bound > 0] / bound[bound > 0]).max())
    assert np.array_equal(full[bound == 0], want[bound == 0]) and ratio <= 1.0, f"{name} {form} Kc={Kc}: {ratio:.3f} x the bound"
    assert cells < 8 or float(np.abs(want[[0, 2]]).min()) > 1e3 * float(bound.max()), "the dots are far above their bound: a wrong draw cannot hide"
    for row0, rows in WINDOWS[1:]:
        part = run(PG.dev(phi), row0, rows).transpose(0, 2, 1).reshape(KB * KN, Kc)
        ref = full.transpose(0, 2, 1).reshape(KB * KN, Kc)
        assert np.array_equal(PG.np_bits(part[row0:row0 + rows]), PG.np_bits(ref[row0:row0 + rows])), f"{name}: window {row0}..{row0 + rows} differs from the full call"
        assert np.isnan(part[:row0]).all() and np.isnan(part[row0 + rows:]).all(), "rows outside the window were written"
    mis = run(PG.misaligned(PG.dev(phi)), 0, KB * KN)
    assert cells < 4 or np.abs(mis - want).max() <= bound.max(), "the element-by-element path"
    assert np.array_equal(PG.np_bits(mis), PG.np_bits(full)), "both paths add in the same order"
    print(f"dot {name} {form} Kc={Kc}: cells {cells}, worst |d - numpy| = {ratio:.3e} x cells u sum|I Phi|; windows and both load paths bit for bit")


def _finish_bound(d, delta, beta, infid, normalize, ed=0.0):
    """E of the module docstring, [B,Kc]."""
    n = d.shape[2]
    if normalize:
        S = (d * d).sum(-1)
        ebeta = np.where(S > 0, (n + 1) * U * np.abs(d * delta).sum(-1) / np.where(S > 0, S, 1.0), 0.0) + np.abs(beta) * (n + 3) * U
    else:
        ebeta = np.zeros_like(beta)
    t = beta[..., None] * d - delta
    et = ebeta[..., None] * np.abs(d) + 2 * U * (np.abs(beta[..., None] * d) + np.abs(delta)) + np.abs(beta[..., None]) * ed
    return (2 * np.abs(t) * et + et * et).sum(-1) / n + (n + 3) * U * infid


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("classes", [None, [4, 0, 2]], ids=["all", "per sample"])
def test_finish_against_numpy(classes, normalize):
    Bn, n, K = 3, 7, 6
    Kc = K if classes is None else 1
    rng = np.random.default_rng(4)
    d = rng.standard_normal((Bn, Kc, n))
    d[1] = 0.0                                                               # all-zero dots: beta = 0
    S = rng.random((Bn, n, K)).astype(np.float32)
    clean = rng.random((Bn, K)).astype(np.float32)
    cls = None if classes is None else torch.tensor(classes, dtype=torch.int32, device=DEV)
    infid, beta = (torch.full((Bn, Kc), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    drops = torch.full((Bn, Kc, n), float("nan"), dtype=torch.float64, device=DEV)
    dd, Sd, cd = PG.dev(d), PG.dev(S), PG.dev(clean)
    L.check(L.load().bx_infidelity_finish(PG.p(dd), PG.p(Sd), PG.p(cd), PG.p(cls), PG.p(infid), PG.p(beta), PG.p(drops), Bn, n, K,
                                          int(normalize), PG.stream()), "bx_infidelity_finish")
    infid, beta, drops = infid.cpu().numpy(), beta.cpu().numpy(), drops.cpu().numpy()
    delta = R.drops(clean, S)
    if classes is not None:
        delta = np.stack([delta[b, c][None] for b, c in enumerate(classes)])
    assert np.array_equal(PG.np_bits(drops), PG.np_bits(delta)), "a drop is one exact-operand fp64 subtraction"
    want, wbeta = R.finish(d, delta, normalize)
    assert (beta[1] == 0).all() if normalize else (beta == 1).all()
    E = _finish_bound(d, delta, wbeta, want, normalize)
    ratio = float((np.abs(infid - want) / (2 * E)).max())
    same = bool(np.array_equal(PG.np_bits(infid), PG.np_bits(want)) and np.array_equal(PG.np_bits(beta), PG.np_bits(wbeta)))
    print(f"finish {'all classes' if classes is None else 'one class per sample'}, normalize {normalize}: {ratio:.3e} x the bound, bit for bit: {same}")
    assert ratio <= 1.0 and np.allclose(beta, wbeta, rtol=1e-12, atol=0)
    assert np.allclose(infid[1], (delta[1] ** 2).sum(-1) / n, rtol=1e-14, atol=0), "zero dots leave the mean square of the drops"


@pytest.mark.parametrize("P", [1, 35, 1000, 38000])
def test_distance_and_sensitivity_finish_against_numpy(P):
    Bn, n = 3, 5
    lib = L.load()
    ref = O.seeded((Bn, P), 41, "randn")
    ref[1] = 0.0                                                             # a zero explanation: the denominator is 1
    a = ref.repeat_interleave(n, 0) + 0.01 * O.seeded((Bn * n, P), 42, "randn")
    want_dist, want_norm = R.distances(a.numpy(), ref.numpy(), n)
    ad, rd = PG.dev(a), PG.dev(ref)
    norms = torch.full((Bn,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(lib.bx_sensitivity_dist(PG.p(rd), None, PG.p(norms), Bn, 1, P, 0, Bn, PG.stream()), "bx_sensitivity_dist")
    full = torch.full((Bn * n,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(lib.bx_sensitivity_dist(PG.p(ad), PG.p(rd), PG.p(full), Bn, n, P, 0, Bn * n, PG.stream()), "bx_sensitivity_dist")
    for row0, rows in WINDOWS[1:]:
        for mis in (False, True):
            part = torch.full((rows,), float("nan"), dtype=torch.float64, device=DEV)
            rows_a = ad[row0:row0 + rows].contiguous()
            L.check(lib.bx_sensitivity_dist(PG.p(PG.misaligned(rows_a) if mis else rows_a), PG.p(rd), PG.p(part), Bn, n, P, row0, rows, PG.stream()), "bx_sensitivity_dist")
            assert torch.equal(part, full[row0:row0 + rows]), f"window {row0}..{row0 + rows} differs from the full call"
    norms_h, dist_h = norms.cpu().numpy(), full.cpu().numpy().reshape(Bn, n)
    rel = 2 * (P / 2 + 2) * U
    assert norms_h[1] == 0 and (np.abs(norms_h - want_norm) <= rel * want_norm).all() and (np.abs(dist_h - want_dist) <= rel * want_dist).all()
    assert (dist_h > 0).all()
    sens = torch.full((Bn,), float("nan"), dtype=torch.float64, device=DEV)
    L.check(lib.bx_sensitivity_finish(PG.p(full), PG.p(norms), PG.p(sens), Bn, n, PG.stream()), "bx_sensitivity_finish")
    want = R.sens_finish(want_dist, want_norm)
    got = sens.cpu().numpy()
    assert got[1] == dist_h[1].max(), "a zero norm divides by 1"
    assert (np.abs(got - want) <= (2 * rel + 2 * U) * want).all()
    print(f"distance P={P}: worst relative error {float((np.abs(dist_h - want_dist) / want_dist).max()):.3e}, bound {rel:.3e}")


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
EN, ESEED = 6, 3


def _device_noise(shape, n=EN, seed=ESEED):
    return brainxai.smooth_grad_noise(tuple(shape), nsamples=n, seed=seed, device=DEV).cpu().numpy()


def _composed_scores(model, eeg, spec, rows_all, n, max_batch, dt):
    """The scores of the clean spectrograms and of ``rows_all`` fp32 [B*n,C,H,W] from existing pieces: to_nhwc, the library's forward and
    softmax, in the batches of infidelity's own sweep.  -> (clean [B,K], S [B,n,K]) fp32 on the host."""
    B = spec.shape[0]
    net = model.spectrogram_model
    with X._eval_frozen(model), torch.no_grad():
        fixed = X._fixed_branch(model, eeg, True)
        clean = X._softmax_rows(X._rows_forward(model, net, True, True, ops.to_nhwc(spec, dt), fixed))
        K = clean.shape[1]
        S = torch.empty(B, n, K, dtype=torch.float32, device=DEV)
        r = rows_all.reshape(B, n, *spec.shape[1:])
        for b0, nb, n0, nn in X._faith_chunks(B, n, X._row_cap(spec, "spec", dt, max_batch)):
            rows = ops.to_nhwc(r[b0:b0 + nb, n0:n0 + nn].reshape(nb * nn, *spec.shape[1:]).contiguous(), dt)
            rep = fixed[b0:b0 + nb].repeat_interleave(nn, dim=0) if nn > 1 else fixed[b0:b0 + nb]
            S[b0:b0 + nb, n0:n0 + nn] = X._softmax_rows(X._rows_forward(model, net, True, True, rows, rep)).reshape(nb, nn, K)
    return clean.cpu().numpy(), S.cpu().numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_spec_input_against_the_same_pass_from_pieces(dt, form):
    """The scores are then the same launches on the same bits: the drops are equal bit for bit, what remains is the dot and finish bound."""
    grouped = form == "grouped"
    _, mine = PG.scaled_multimodal(dt)
    eeg, spec = GG.mm_inputs()
    eeg_d, spec_d = eeg.to(DEV), spec.to(DEV)
    B, n, max_batch = 2, EN, 5
    cs = (32, 64) if grouped else (4, 32, 64)
    z = _device_noise((B, *cs))
    sig = SG.sigma(spec, LEVEL)
    phi = O.seeded((B, 6, *cs), 19, "randn")
    # rows in torch from the dumped z: a product and a difference, each its own kernel
    zd, sd = PG.dev(z), PG.dev(sig)
    I_d = sd[:, None, None, None, None] * (zd[:, :, None] if grouped else zd)
    rows_all = (spec_d[:, None] - I_d).reshape(B * n, 4, 32, 64)
    assert np.array_equal(PG.np_bits(rows_all.cpu().numpy()), PG.np_bits(R.rows(spec, sig, z, grouped, False))), "the composed rows are not the restatement's"
    clean, S = _composed_scores(mine, eeg_d, spec_d, rows_all, n, max_batch, dt)
    I = R.perturbation(sig, z)
    d, absum = R.dots(I, phi.reshape(B, 6, -1).numpy())
    delta = R.drops(clean, S)
    ed = I.shape[2] * U * absum
    line = []
    for normalize in (False, True):
        res = brainxai.infidelity(mine, eeg_d, spec_d, phi.to(DEV), input="spec", nsamples=n, noise_level=LEVEL, normalize=normalize, class_idx="all",
                                  seed=ESEED, max_batch=max_batch, return_parts=True)
        assert res.infidelity.shape == res.beta.shape == (B, 6) and res.dots.shape == res.drops.shape == (B, 6, n) and res.classes is None
        assert res.infidelity.dtype == res.dots.dtype == torch.float64 and (res.nsamples, res.seed) == (n, ESEED)
        assert np.array_equal(PG.np_bits(res.sigma.cpu().numpy()), PG.np_bits(sig)) and np.array_equal(PG.np_bits(res.clean.cpu().numpy()), PG.np_bits(clean))
        assert np.array_equal(PG.np_bits(res.drops.cpu().numpy()), PG.np_bits(delta)), "drops must be bit for bit those of the composed pass"
        got_d = res.dots.cpu().numpy()
        rd = float((np.abs(got_d - d) / ed).max())
        want, wbeta = R.finish(d, delta, normalize)
        E = _finish_bound(d, delta, wbeta, want, normalize, ed)
        ri = float((np.abs(res.infidelity.cpu().numpy() - want) / (2 * E)).max())
        line.append(f"normalize {normalize}: dots {rd:.3e} x bound, infidelity {ri:.3e} x bound")
        assert rd <= 1.0 and ri <= 1.0 and float(want.min()) > 0
        whole = brainxai.infidelity(mine, eeg_d, spec_d, phi.to(DEV), input="spec", nsamples=n, noise_level=LEVEL, normalize=normalize, class_idx="all",
                                    seed=ESEED, return_parts=True)
        assert torch.equal(whole.dots, res.dots), "no bit of the dots may depend on max_batch"
    print(f"infidelity spec input ({form} cells) vs composed pass, {dt}: " + "; ".join(line))


def _oracle_reference(f64, x, other, grouped, z, sig, phi=None, logprob=True):
    """fp64 side of an EEG-input case.  -> (phi fp32 [B,K,cells], score, (infid, beta, d, Delta) of the restatement).  phi defaults to the
    fp64 input gradient of every class score (summed over the electrodes for time-column cells), rounded to fp32."""
    B = x.shape[0]

    def run(rows, o):
        lp = f64(rows) if other is None else f64(rows, o)
        return lp if logprob else lp.exp()

    def score(rows):
        return run(rows, None if other is None else other.double().repeat_interleave(len(rows) // B, 0)).detach().numpy()
    if phi is None:
        xi = x.double().requires_grad_(True)
        p = run(xi, None if other is None else other.double())
        g = torch.stack([torch.autograd.grad(p[:, c].sum(), xi, retain_graph=True)[0] for c in range(p.shape[1])], 1)      # [B,K,1,Chans,T]
        g = g.sum(3) if grouped else g
        phi = g.reshape(B, p.shape[1], -1).float().numpy()
    return phi, score, R.infidelity(score, x, sig, z, phi, grouped, True)


def _oracle_bound(d, delta, beta, ed):
    """[B,K]: the mean over the draws of 2 |beta d - Delta| e + e^2 with e = TOL, and the dot's share."""
    t = np.abs(beta[..., None] * d - delta)
    return (2 * t * TOL + TOL * TOL).mean(-1) + (2 * t * ed + ed * ed).mean(-1)


def _oracle_guard(what, f64, x, other, grouped, z, z_other, sig, phi, want, bound):
    """Reference side alone: the inputs discriminate the sign, the stream and the scale of the noise and the attribution."""
    half = (sig * np.float32(0.5)).astype(np.float32)
    moved = {"-z": (-z, sig, phi), "another seed": (z_other, sig, phi), "sigma halved": (z, half, phi), "Phi negated": (z, sig, -phi)}
    least = {}
    for how, (zz, ss, pp) in moved.items():
        alt = _oracle_reference(f64, x, other, grouped, zz, ss, pp)[2][0]
        least[how] = float((np.abs(alt - want) / bound).min())
    print(f"{what}: the reference moves by (least over (sample, class), in bounds) " + ", ".join(f"{how} {v:.1f}" for how, v in least.items()))
    for how, v in least.items():
        assert v > 100, f"{what}: {how} moves the reference by only {v:.2f} bounds"


# The multimodal model's heads are scaled down (tests/perturb_gpu.scaled_multimodal) and its EEG branch moves the output little: at level
# 0.15 -z moves its reference by only 60 bounds.  Time-column cells at level 1.0 move it by more than 1000 (checked on the reference side).
@pytest.mark.parametrize("kind,form,level", [("eegnet", "element", LEVEL), ("deep", "element", LEVEL), ("multimodal", "grouped", 1.0)])
def test_eeg_input_against_the_fp64_oracle(kind, form, level):
    grouped = form == "grouped"
    _, mine, f64, x, other = GG.eeg_models(kind)
    B = x.shape[0]
    cs = (2000,) if grouped else (1, 19, 2000)
    z, z_other, sig = _device_noise((B, *cs)), _device_noise((B, *cs), seed=ESEED + 1), SG.sigma(x, level)
    phi, _, (want, wbeta, d, delta) = _oracle_reference(f64, x, other, grouped, z, sig)
    _, absum = R.dots(R.perturbation(sig, z), phi)
    ed = phi.shape[2] * U * absum
    bound = _oracle_bound(d, delta, wbeta, ed)
    what = f"infidelity eeg input, {kind}, {form} cells, level {level}"
    _oracle_guard(what, f64, x, other, grouped, z, z_other, sig, phi, want, bound)
    attribution = torch.from_numpy(phi).reshape(B, 6, *((1, 2000) if grouped else (1, 19, 2000))).to(DEV)
    res = brainxai.infidelity(mine, x.to(DEV), None if other is None else other.to(DEV), attribution, input="eeg", nsamples=EN, noise_level=level,
                              class_idx="all", score="logprob", seed=ESEED, return_parts=True)
    assert res.infidelity.shape == (B, 6) and bool(torch.isfinite(res.infidelity).all()) and (res.beta == 1).all()
    rd = float((np.abs(res.dots.cpu().numpy() - d) / ed).max())
    rdrop = float(np.abs(res.drops.cpu().numpy() - delta).max() / (2 * TOL))
    ratio = float((np.abs(res.infidelity.cpu().numpy() - want) / bound).max())
    print(f"{what}: infidelity {ratio:.3e} x bound (worst relative error {float((np.abs(res.infidelity.cpu().numpy() - want) / want).max()):.3e}), "
          f"dots {rd:.3e} x bound, drops {rdrop:.3e} x 2 TOL")
    assert rd <= 1.0 and ratio <= 1.0, f"{what}: {ratio:.3f} x the bound"


# ---- interface --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _iface():
    """GG.iface() and an attribution for either input, [B,K,H,W] and [B,K,1,T]."""
    return GG.iface() + (PG.dev(O.seeded((2, 6, 32, 64), 19, "randn")), PG.dev(O.seeded((2, 6, 1, 2000), 20, "randn")))


def test_repeatable_prefix_and_seed():
    mine, eeg, spec, phi_s, _ = _iface()
    kw = dict(input="spec", nsamples=EN, class_idx="all", seed=ESEED, return_parts=True)
    a = brainxai.infidelity(mine, eeg, spec, phi_s, **kw)
    b = brainxai.infidelity(mine, eeg, spec, phi_s, **kw)
    for fa, fb in zip(a[:5], b[:5]):
        assert torch.equal(fa, fb), "two calls differ"
    plain = brainxai.infidelity(mine, eeg, spec, phi_s, input="spec", nsamples=EN, class_idx="all", seed=ESEED)
    assert torch.equal(plain, a.infidelity) and plain.dtype == torch.float64
    other = brainxai.infidelity(mine, eeg, spec, phi_s, **{**kw, "seed": ESEED + 1})
    assert not torch.equal(other.dots, a.dots) and not torch.equal(other.infidelity, a.infidelity)
    three = brainxai.infidelity(mine, eeg, spec, phi_s, **{**kw, "nsamples": 3})
    assert torch.equal(three.dots, a.dots[..., :3]) and torch.equal(three.drops, a.drops[..., :3]), "nsamples = 3 sees the first three draws of nsamples = 6"
    small = brainxai.infidelity(mine, eeg, spec, phi_s, max_batch=5, **kw)
    assert torch.equal(small.dots, a.dots)
    assert float((small.drops - a.drops).abs().max()) <= 2 * TOL


def test_class_forms():
    mine, eeg, spec, phi_s, phi_e = _iface()
    for input, phi in (("spec", phi_s), ("eeg", phi_e)):
        kw = dict(input=input, nsamples=4, seed=5, return_parts=True)
        every = brainxai.infidelity(mine, eeg, spec, phi, class_idx="all", **kw)
        assert every.infidelity.shape == (2, 6) and every.classes is None and every.clean.shape == (2, 6)
        top_cls = every.clean.argmax(1)
        top = brainxai.infidelity(mine, eeg, spec, phi[torch.arange(2, device=DEV), top_cls], **kw)
        assert top.infidelity.shape == (2,) and top.dots.shape == (2, 4) and torch.equal(top.classes, top_cls)
        for b in range(2):
            assert torch.equal(top.infidelity[b], every.infidelity[b, int(top_cls[b])])
        for c in range(6):
            one = brainxai.infidelity(mine, eeg, spec, phi[:, c], class_idx=c, **kw)
            assert torch.equal(one.infidelity, every.infidelity[:, c]) and torch.equal(one.dots, every.dots[:, c]) and torch.equal(one.drops, every.drops[:, c]), \
                f"{input}: 'all' differs from the call for class {c}"
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.infidelity(mine, eeg, spec, torch.stack([phi[0, 4], phi[1, 1]]), class_idx=form, **kw)
            assert per.classes.tolist() == [4, 1]
            assert torch.equal(per.infidelity, torch.stack([every.infidelity[0, 4], every.infidelity[1, 1]]))
        lp = brainxai.infidelity(mine, eeg, spec, phi, class_idx="all", score="logprob", **kw)
        assert torch.equal(lp.dots, every.dots) and not torch.equal(lp.drops, every.drops)
        assert float((lp.clean.exp() - every.clean).abs().max()) <= 1e-6


def test_normalize_is_invariant_to_the_scale_of_the_attribution():
    mine, eeg, spec, phi_s, _ = _iface()
    phi_s = phi_s.bfloat16().float()                                        # 8 significant bits: 7 * Phi is exact in fp32, so d scales by 7 up to fp64 sums
    assert torch.equal((phi_s * 7).double(), phi_s.double() * 7)
    kw = dict(input="spec", nsamples=EN, class_idx="all", seed=ESEED, normalize=True, return_parts=True)
    a = brainxai.infidelity(mine, eeg, spec, phi_s, **kw)
    b = brainxai.infidelity(mine, eeg, spec, phi_s * 7, **kw)
    rel = float(((a.infidelity - b.infidelity).abs() / a.infidelity).max())
    print(f"normalize: Phi x 7 moves the infidelity by {rel:.3e} relative; beta ratio {float((a.beta / b.beta).mean()):.6f}")
    assert rel <= 1e-12 and float(((a.beta / b.beta) - 7).abs().max()) <= 1e-10
    plain = brainxai.infidelity(mine, eeg, spec, phi_s, **{**kw, "normalize": False})
    assert bool((a.infidelity <= plain.infidelity * (1 + 1e-12)).all()), "beta minimises the mean square"


def test_state_is_restored_and_maps_are_accepted_as_they_are():
    mine, eeg, spec, _, _ = _iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        sal_e, sal_s = brainxai.saliency(mine, eeg, spec)
        got = brainxai.infidelity(mine, eeg, spec, sal_s, input="spec", nsamples=3)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    assert got.shape == (2,) and bool(torch.isfinite(got).all()) and bool((got >= 0).all())
    assert bool(torch.isfinite(brainxai.infidelity(mine, eeg, spec, sal_e, input="eeg", nsamples=3)).all())
    for input in ("spec", "eeg"):
        sg = brainxai.smooth_grad(mine, eeg, spec, input=input, nsamples=3, seed=2)
        occ = brainxai.occlusion(mine, eeg, spec, input=input, window=(8, 16) if input == "spec" else (19, 500))
        for amap in (sg, occ):
            v = brainxai.infidelity(mine, eeg, spec, amap, input=input, nsamples=3, normalize=True)
            assert v.shape == (2,) and bool(torch.isfinite(v).all())
    sm = mine.spectrogram_model                                             # stand-alone models, grad_cam's convention
    alone = brainxai.infidelity(sm, None, spec, sal_s, nsamples=3, return_parts=True)
    assert alone.infidelity.shape == (2,) and bool(torch.isfinite(alone.infidelity).all())
    alone_e = brainxai.infidelity(mine.eeg_model, eeg, None, sal_e.sum(1, keepdim=True), input="eeg", nsamples=3, stdev=0.25, return_parts=True)
    assert alone_e.dots.shape == (2, 3) and torch.equal(alone_e.sigma, torch.full((2,), 0.25, device=DEV))
    still = brainxai.infidelity(mine, eeg, spec, sal_s, nsamples=3, stdev=0.0, return_parts=True)
    assert not still.dots.any() and float(still.drops.abs().max()) <= 2 * TOL, "without noise every row is the sample itself"


# ---- sensitivity_max ----------------------------------------------------------------------------------------------------------------------
def test_sensitivity_max_of_saliency_against_the_rows_composed_in_torch():
    mine, eeg, spec, _, _ = _iface()
    B, n = 2, EN
    seen = []

    def explain(e, s, sample):
        seen.append(sample.clone())
        return brainxai.saliency(mine, e, s)[1]
    res = brainxai.sensitivity_max(explain, eeg, spec, input="spec", nsamples=n, seed=ESEED, max_batch=5, return_parts=True)
    assert res.sensitivity.shape == (B,) and res.distances.shape == (B, n) and res.norms.shape == (B,) and res.sensitivity.dtype == torch.float64
    assert np.array_equal(PG.np_bits(res.radius.cpu().numpy()), PG.np_bits(SG.sigma(spec.cpu(), 0.02))), "the default radius is 0.02 of the sample's range"
    want_samples = torch.arange(B).repeat_interleave(n)
    assert torch.equal(seen[0].cpu(), torch.arange(B)) and [len(s) for s in seen[1:]] == [5, 5, 2]
    assert torch.equal(torch.cat(seen[1:]).cpu(), want_samples) and seen[1].dtype == torch.int64 and seen[1].is_cuda
    # the same rows composed in torch from the dumped uniform draws, explained in the same chunks
    per = spec[0].numel()
    u = torch.empty(B * n, per, dtype=torch.float32, device=DEV)
    L.check(L.load().bx_sensitivity_rows(None, None, PG.p(u), B, n, per, ESEED, 0, B * n, PG.stream()), "bx_sensitivity_rows")
    assert np.array_equal(PG.np_bits(u.cpu().numpy()), PG.np_bits(R.uniform(B, n, per, ESEED).reshape(B * n, per)))
    dl = res.radius[:, None, None] * u.reshape(B, n, per)
    rows = (spec.reshape(B, 1, per) + dl).reshape(B * n, *spec.shape[1:])
    assert np.array_equal(PG.np_bits(rows.cpu().numpy()), PG.np_bits(R.uniform_rows(spec.cpu(), res.radius.cpu().numpy(), u.cpu().numpy().reshape(B, n, *spec.shape[1:]))))
    clean = brainxai.saliency(mine, eeg, spec)[1]
    phis = torch.cat([brainxai.saliency(mine, eeg[want_samples[i:i + 5]], rows[i:i + 5])[1] for i in range(0, B * n, 5)])
    want_dist, want_norm = R.distances(phis.cpu().numpy(), clean.cpu().numpy(), n)
    P = clean[0].numel()
    rel = 2 * (P / 2 + 2) * U
    dist, norms = res.distances.cpu().numpy(), res.norms.cpu().numpy()
    print(f"sensitivity_max of saliency: sensitivity {res.sensitivity.tolist()}, worst relative distance error {float((np.abs(dist - want_dist) / want_dist).max()):.3e} "
          f"(bound {rel:.3e})")
    assert (want_dist > 0).all() and (np.abs(dist - want_dist) <= rel * want_dist).all() and (np.abs(norms - want_norm) <= rel * want_norm).all()
    want = R.sens_finish(want_dist, want_norm)
    assert (np.abs(res.sensitivity.cpu().numpy() - want) <= (2 * rel + 2 * U) * want).all()
    whole = brainxai.sensitivity_max(explain, eeg, spec, input="spec", nsamples=n, seed=ESEED, max_batch=256, return_parts=True)
    assert [len(s) for s in seen[-2:]] == [B, B * n]
    assert float(((whole.distances - res.distances).abs() / res.distances).max()) <= 1e-3 and torch.equal(whole.norms, res.norms), \
        "max_batch = 5 and 256 explain the same rows"
    assert torch.equal(brainxai.sensitivity_max(explain, eeg, spec, input="spec", nsamples=n, seed=ESEED, max_batch=5), res.sensitivity)


def test_sensitivity_max_forms_and_refusals_on_the_device():
    mine, eeg, spec, _, _ = _iface()
    cls = torch.tensor([4, 1], device=DEV)
    # the EEG input, a class per sample through ``sample``, an absolute radius per sample
    res = brainxai.sensitivity_max(lambda e, s, i: brainxai.occlusion(mine, e, s, input="eeg", window=(19, 500), class_idx=cls[i]), eeg, spec, input="eeg",
                                   nsamples=3, radius=torch.tensor([0.0, 0.5]), return_parts=True)
    print(f"sensitivity_max of occlusion, eeg input, radius (0, 0.5): {res.sensitivity.tolist()}")
    assert res.distances.shape == (2, 3) and float(res.sensitivity[0]) <= 1e-3 and float(res.sensitivity[1]) > float(res.sensitivity[0]), \
        "radius 0 leaves the explanation where it is"
    assert torch.equal(res.radius, torch.tensor([0.0, 0.5], device=DEV))
    # a stand-alone model: the other input stays None
    sm = mine.spectrogram_model
    seen = []

    def alone(e, s, i):
        seen.append(e)
        return brainxai.occlusion(sm, None, s, window=(8, 16), class_idx=2)
    one = brainxai.sensitivity_max(alone, None, spec, nsamples=2, radius=0.01)
    assert one.shape == (2,) and bool(torch.isfinite(one).all()) and all(e is None for e in seen)
    # a zero explanation divides by 1; the trailing shape must not change between calls
    zero = brainxai.sensitivity_max(lambda e, s, i: torch.zeros(len(i), 3, device=DEV), eeg, spec, nsamples=2, return_parts=True)
    assert not zero.sensitivity.any() and not zero.norms.any()
    shapes = iter([(2, 3), (4, 5)])
    with pytest.raises(ValueError, match="trailing shape"):
        brainxai.sensitivity_max(lambda e, s, i: torch.zeros(*next(shapes), device=DEV), eeg, spec, nsamples=2)
    with pytest.raises(ValueError, match="explain must return"):
        brainxai.sensitivity_max(lambda e, s, i: torch.zeros(len(i) + 1, 3, device=DEV), eeg, spec, nsamples=2)
    with pytest.raises(ValueError, match="explain must return"):
        brainxai.sensitivity_max(lambda e, s, i: None, eeg, spec, nsamples=2)
