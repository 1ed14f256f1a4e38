"""GPU: brainxai.spectral_gradients / spectral_occlusion / eeg_spectrum / band_sums and the entry points of csrc/spectral.hip against the
restatement of the definition (tests/spectral_ref.py, on numpy's fp64 FFT), and end to end against the oracle's classes in fp64.

Bounds (u = 2^-53).  bx_rdft_rows: per bin |err| <= (T + 4) u sum_t |x_t| =: eps -- T fused multiply-adds whose partial sums stay below
sum |x|, a table entry within two units, numpy's own error.  bx_spectral_values: (c_f / T) (eps_X |G_f| / |X_f| + eps_G) + 2^-24 |value|
(the phase u = X / |X| moves by eps_X / |X_f|; gradient x amplitude has no phase: the first term is dropped); bins with
|X_f| < 2^-30 sum |x| -- rounding noise: the constant row's -- are left out of the amplitude-gradient comparison only.  The running sum
and the band sums: bit for bit.  bx_bandstop_rows: 2^-24 |row| + ((f_hi - f_lo) + 2) u sum c_f |X_f| / T + (f_hi - f_lo) (2 / T) eps_X.
End to end: the time-domain gradient within TOL = 1e-3 of each (sample, class) maximum (the project's fp32 gradient bound,
tests/test_gpu_parity.py); the map against the restatement of the device's own gradient within the kernel bound (for steps > 1 the
reported gradient is the fp32 rounding of the fp64 sums the map was formed from: G_f moves by up to 2^-24 sum |g| and the value by
(c_f / T) |X_f| times that, |u_f| = 1 for the amplitude gradient); the map against the full
fp64 oracle within E2E_BOUND = 4 x E2E_WORST, the worst figure observed on the MI355X (printed by the test, recorded in DESIGN.md
section 6), which in turn stays below 1/100 of the least movement of the discrimination checks (test_spectral_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from tests import blur_ig_ref as BR
from tests import grad_gpu as GG
from tests import perturb_gpu as PG
from tests import spectral_ref as R
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3
E2E_WORST = 8.6e-7                      # observed on the MI355X: the worst map error against the fp64 oracle, of each (sample, class) maximum
E2E_BOUND = 4 * E2E_WORST

# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# up to 2 x 3000 the table is staged in LDS; 1 x 4100 and 1 x 8192 read it from global memory (the band-stop kernel above T = 3072);
# 3 x 5, 3 x 19 and 3 x 2 rows leave the last group of 8 rows partial, 3 x 1 a single partial group
SHAPES = [(1, 1), (1, 2), (3, 3), (5, 7), (2, 64), (5, 125), (5, 333), (19, 2000), (2, 3000), (1, 4100), (1, 8192)]
KB, KN = 3, 5
WINDOWS = [(0, 15), (2, 10), (14, 1)]              # all rows; from inside sample 0 to inside sample 2; the last row alone
shapes = pytest.mark.parametrize("Chans,T", SHAPES, ids=[f"{c}x{t}" for c, t in SHAPES])


@functools.lru_cache(maxsize=None)
def _kernel_input(Chans, T):
    """x fp32 [KB,1,Chans,T]: randn with every 7th value -0.0, one all-zero row (sample 1, electrode 0) and one constant row (sample 2,
    the last electrode); never written to."""
    x = R.O.seeded((KB, 1, Chans, T), 400 + SHAPES.index((Chans, T)), "randn")
    x.view(-1)[::7] = -0.0
    x[1, 0, 0] = 0.0
    x[2, 0, Chans - 1] = 2.5
    return x


SPECIAL = lambda Chans: {(1, 0), (2, Chans - 1)}                           # noqa: E731  the zero and the constant row


@functools.lru_cache(maxsize=None)
def _table(T):
    return PG.dev(brainxai.spectral_twiddles(T))


def _device_spectrum(xd, T):
    R_ = xd.numel() // T
    re = torch.full((R_, T // 2 + 1), float("nan"), dtype=torch.float64, device=DEV)
    im = torch.full_like(re, float("nan"))
    L.check(L.load().bx_rdft_rows(PG.p(xd), PG.p(_table(T)), PG.p(re), PG.p(im), R_, T, PG.stream()), "bx_rdft_rows")
    return re, im


@shapes
def test_rdft_against_numpy(Chans, T):
    x = _kernel_input(Chans, T)
    want, bound = R.rdft(x.numpy()[:, 0]), R.dft_bound(x.numpy()[:, 0])
    re, im = _device_spectrum(PG.dev(x), T)
    got = (re.cpu().numpy() + 1j * im.cpu().numpy()).reshape(want.shape)
    assert not np.isnan(got).any(), "bins left unwritten"
    ratio = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) / np.where(bound > 0, bound, 1.0)
    print(f"rdft {Chans} x {T}: worst {ratio.max():.3f} x the bound (T + 4) u sum |x|")
    assert ratio.max() <= 1.0
    assert not got[1, 0].real.any() and not got[1, 0].imag.any(), "the zero row gives exactly 0"
    re2, im2 = _device_spectrum(PG.misaligned(PG.dev(x)), T)
    assert torch.equal(re2.view(torch.int64), re.view(torch.int64)) and torch.equal(im2.view(torch.int64), im.view(torch.int64)), "misaligned input"
    sre, sim, freqs = brainxai.eeg_spectrum(x.to(DEV), fs=40.0)
    assert sre.shape == (KB, Chans, T // 2 + 1) and torch.equal(sre.reshape(re.shape), re) and torch.equal(sim.reshape(im.shape), im)
    assert np.array_equal(freqs, np.arange(T // 2 + 1) * 40.0 / T)
    assert torch.equal(brainxai.eeg_spectrum(x[:, 0].to(DEV))[0], sre)


@pytest.mark.parametrize("kind", R.MAP_KINDS)
@shapes
def test_values_against_the_fp64_restatement(Chans, T, kind):
    x = _kernel_input(Chans, T)
    Kc, F = 2, T // 2 + 1
    g = torch.randn(KB, Kc, Chans, T, dtype=torch.float64, generator=torch.Generator().manual_seed(T))
    xd = PG.dev(x)
    re, im = _device_spectrum(xd, T)
    out = torch.full((KB, Kc, Chans, F), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.load().bx_spectral_values(PG.p(PG.dev(g)), PG.p(re), PG.p(im), PG.p(_table(T)), PG.p(out), KB, Kc, Chans, T, X._SPECTRAL_KINDS[kind], PG.stream()),
            "bx_spectral_values")
    got = out.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), "bins left unwritten"
    xr = x.numpy()[:, None, 0]                                               # [KB,1,Chans,T] against g [KB,Kc,Chans,T]
    want = R.maps(xr, g.numpy(), kind)
    bound = R.values_bound(xr, g.numpy(), kind, want)
    keep = np.ones(want.shape, dtype=bool)
    if kind == "amplitude_gradient":
        tiny = R.tiny_bins(x.numpy()[:, 0])                                  # [KB,Chans,F]
        assert {(int(b), int(e)) for b, e in zip(*np.nonzero(tiny.any(-1)))} <= SPECIAL(Chans), "only the constant row has bins of rounding noise"
        keep &= ~tiny[:, None]
    ratio = np.where(keep, np.abs(got - want) / np.where(bound > 0, bound, 1.0), 0.0)
    print(f"values {kind} {Chans} x {T}: worst {ratio.max():.3f} x the bound; {int((~keep).sum())} bins left out")
    assert ratio.max() <= 1.0
    if kind == "gradient_x_amplitude":                                       # Parseval: the bins of an electrode add up to sum_t g_t x_t
        dot = (xr.astype(np.float64) * g.numpy()).sum(-1)
        assert (np.abs(got.sum(-1) - dot) <= bound.sum(-1) + 1e-13 * np.abs(xr.astype(np.float64) * g.numpy()).sum(-1)).all()


@pytest.mark.parametrize("Kc", [1, 3])
@shapes
def test_accumulate_bit_for_bit(Chans, T, Kc):
    per, rows_all, n, slot = Chans * T, KB * KN, KN, Kc // 2
    g = R.O.seeded((rows_all, per), 7, "randn")
    g.view(-1)[::5] = -0.0
    w = np.random.default_rng(4).standard_normal(n)
    lib, gd, wd = L.load(), PG.dev(g), PG.dev(w)
    SENTINEL = 7.25

    def run(splits, mis=False):
        acc = torch.full((KB, Kc, per), SENTINEL, dtype=torch.float64, device=DEV)
        acc[:, slot] = 0.0
        for row0, rows in splits:
            gs = gd[row0:row0 + rows].contiguous()
            L.check(lib.bx_spectral_accumulate(PG.p(PG.misaligned(gs) if mis else gs), PG.p(wd), PG.p(acc), KB, n, per, Kc, slot, row0, rows, PG.stream()),
                    "bx_spectral_accumulate")
        return acc
    full = run([WINDOWS[0]])
    want = R.accumulate(g.numpy(), w, KB, n)
    assert np.array_equal(PG.np_bits(full[:, slot].cpu().numpy()), PG.np_bits(want[:, 0])), "the fp64 sums are not numpy's in the same order"
    assert bool((full[:, [k for k in range(Kc) if k != slot]] == SENTINEL).all()), "the slots of other classes were touched"
    (row0, rows), (last0, last) = WINDOWS[1], WINDOWS[2]
    pieces = run([(0, row0), (row0, rows), (row0 + rows, last0 - row0 - rows), (last0, last)], mis=True)
    assert torch.equal(full, pieces), "calls split inside a sample differ from one call"
    for row0, rows in WINDOWS[1:]:                                           # a window alone: numpy's sums of those rows
        alone = run([(row0, rows)])
        assert np.array_equal(alone[:, slot].cpu().numpy(), R.accumulate(g.numpy()[row0:row0 + rows], w, KB, n, row0=row0)[:, 0]), (row0, rows)


@shapes
def test_band_sum_bit_for_bit(Chans, T):
    F = T // 2 + 1
    v = R.O.seeded((KB * Chans, F), 9, "randn")
    v.view(-1)[::3] *= 1e-3
    bins = [(0, F), (0, 0), (min(1, F), min(3, F)), (F // 2, F), (F, F)]
    for vd in (PG.dev(v), PG.misaligned(PG.dev(v))):
        out = torch.full((KB * Chans, len(bins)), float("nan"), dtype=torch.float64, device=DEV)
        L.check(L.load().bx_band_sum(PG.p(vd), PG.p(torch.tensor(bins, dtype=torch.int32, device=DEV)), PG.p(out), KB * Chans, F, len(bins), PG.stream()), "bx_band_sum")
        assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(R.band_sum(v.numpy(), bins)))
    assert not PG.np_bits(out[:, 1].cpu().numpy()).any(), "the empty band gives +0"
    edges = [(0.0, 0.6), (0.1, 0.1), (0.2, 0.4)]
    got = brainxai.band_sums(v.reshape(KB, Chans, F).to(DEV), edges, T=T)
    assert got.shape == (KB, Chans, 3) and np.array_equal(got.cpu().numpy().reshape(-1, 3), R.band_sum(v.numpy(), R.band_bins(edges, T)))


def _launch_bandstop(xd, re, im, T, bins_d, nb, cells, n0, n, out):
    Bn, _, Chans, _ = xd.shape
    L.check(L.load().bx_bandstop_rows(PG.p(xd), PG.p(re), PG.p(im), PG.p(_table(T)), PG.p(bins_d), PG.p(out), Bn, Chans, T, nb, X._SPECTRAL_CELLS[cells], n0, n,
                                      PG.stream()), "bx_bandstop_rows")


@pytest.mark.parametrize("cells", ["band", "electrode_band"])
@shapes
def test_bandstop_rows_against_the_fp64_restatement(Chans, T, cells):
    F = T // 2 + 1
    x = _kernel_input(Chans, T)
    bins = [(0, F), (F // 2, F // 2), (min(1, F - 1), min(2, F)), (F // 3, min(F, 2 * F // 3 + 1)), (F - 1, F)]        # all; empty; one bin; a third; the last bin
    nb = len(bins)
    N = nb if cells == "band" else nb * Chans
    xd, bins_d = PG.dev(x), torch.tensor(bins, dtype=torch.int32, device=DEV)
    re, im = _device_spectrum(xd, T)
    full = torch.full((KB * N, 1, Chans, T), float("nan"), dtype=torch.float32, device=DEV)
    _launch_bandstop(xd, re, im, T, bins_d, nb, cells, 0, N, full)
    got = full.cpu().numpy().reshape(KB, N, 1, Chans, T)
    assert not np.isnan(got).any(), "elements left unwritten"
    want = R.bandstop_rows(x.numpy(), bins, cells)
    xn, worst = x.numpy(), 0.0
    for j in range(N):
        q, sel = (j, None) if cells == "band" else divmod(j, Chans)
        lo, hi = bins[q]
        for e in range(Chans):
            if (sel is not None and e != sel) or lo == hi:                   # unselected electrodes and empty bands: x bit for bit
                assert np.array_equal(PG.np_bits(got[:, j, 0, e]), PG.np_bits(xn[:, 0, e])), f"row {j} electrode {e} is not x bit for bit"
                continue
            bound = R.bandstop_bound(xn[:, 0, e], want[:, j, 0, e], lo, hi)
            ratio = np.abs(got[:, j, 0, e] - want[:, j, 0, e]) / np.where(bound > 0, bound, 1.0)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"row {j} (bins {lo}..{hi}) electrode {e}: {ratio.max():.3f} x the bound"
    print(f"bandstop {cells} {Chans} x {T}: worst {worst:.3f} x the bound")
    for n0, n in PG.row_windows(N):                                          # chunked calls give the slices of the full call
        part = torch.full((KB * n, 1, Chans, T), float("nan"), dtype=torch.float32, device=DEV)
        _launch_bandstop(xd, re, im, T, bins_d, nb, cells, n0, n, part)
        assert torch.equal(PG.bits(part).reshape(KB, n, -1), PG.bits(full).reshape(KB, N, -1)[:, n0:n0 + n]), f"rows {n0}..{n0 + n}"
    one = torch.full((N, 1, Chans, T), float("nan"), dtype=torch.float32, device=DEV)      # a sample group that does not start at 0
    _launch_bandstop(xd[1:2], re[Chans:2 * Chans], im[Chans:2 * Chans], T, bins_d, nb, cells, 0, N, one)
    assert torch.equal(PG.bits(one), PG.bits(full[N:2 * N]))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_model(kind):
    """(mine, x, other) on the device for an end-to-end case, with the parameters and inputs of spectral_ref.oracle_case."""
    ref, x, other = R.oracle_case(kind)
    if kind == "small":
        mine = brainxai.EEGNet(6, Chans=5, Samples=512, dropoutRate=0.0)
        mine.load_state_dict(ref.state_dict())
        mine = mine.to(DEV).eval()
    else:
        _, mine, _, gx, gother = GG.eeg_models(kind)
        assert torch.equal(gx, x) and (other is None or torch.equal(gother, other))
    return mine, x.to(DEV), None if other is None else other.to(DEV)


@pytest.mark.parametrize("steps", R.E2E_STEPS)
@pytest.mark.parametrize("kind", R.E2E_KINDS)
def test_against_the_fp64_oracle(kind, steps):
    mine, xd, other = _device_model(kind)
    x, grad, ref_out, ref_zero = R.oracle_gradient(kind, steps)
    Bn, _, Chans, T = x.shape
    bands, fs = ("clinical", 40.0) if T == 2000 else ([(0.0, 0.1), (0.1, 0.25), (0.3, 0.3), (0.25, 0.6)], None)
    least = min(min(R.movements(kind, steps, mk).values()) for mk in R.MAP_KINDS)
    assert E2E_BOUND < least / 100, f"the end-to-end bound {E2E_BOUND:.1e} does not stay below 1/100 of the least movement {least:.3e}"
    for map_kind in R.MAP_KINDS:
        what = f"spectral_gradients {kind} steps {steps} {map_kind}"
        res = brainxai.spectral_gradients(mine, xd, other, kind=map_kind, steps=steps, fs=fs, bands=bands, class_idx="all", return_parts=True)
        assert res.map.shape == (Bn, 6, Chans, T // 2 + 1) and res.gradient.shape == (Bn, 6, 1, Chans, T) and res.classes is None
        assert (res.kind, res.steps, res.band_bins) == (map_kind, steps, R.band_bins(bands, T, fs)) and np.array_equal(res.freqs, np.arange(T // 2 + 1) * (fs or 1.0) / T)
        # the time-domain gradient against the oracle's
        g_err = GG.worst(res.gradient, grad)
        assert float((res.out.double().cpu() - ref_out).abs().max()) <= TOL * float(ref_out.abs().max())
        # the map against the restatement of the device's own gradient
        g_dev = res.gradient.double().cpu().numpy()
        got = res.map.double().cpu().numpy()
        own = R.oracle_map(x.numpy(), g_dev, map_kind)
        xr, gr = x.numpy()[:, None, 0], g_dev[:, :, 0]
        bound = R.values_bound(xr, gr, map_kind, own)
        if steps > 1:                                                        # the reported gradient is the fp32 rounding of the sums the map came from
            lead = np.abs(R.rdft(xr)) if map_kind == "gradient_x_amplitude" else 1.0      # |G_f| moves by up to 2^-24 sum |g|, the value by |X_f| or |u_f| = 1 times that
            bound = bound + R.weights(T) / T * lead * 2.0 ** -24 * np.abs(gr).sum(-1, keepdims=True)
        k_ratio = float((np.abs(got - own) / bound).max())
        # the map against the full fp64 oracle
        want = R.oracle_map(x.numpy(), grad.numpy(), map_kind)
        e2e = GG.worst(res.map, torch.from_numpy(want))
        print(f"{what}: gradient {g_err:.3e} of the maximum; map {k_ratio:.3f} x the kernel bound on its own gradient; map against the oracle {e2e:.3e} "
              f"of the maximum (E2E_WORST {E2E_WORST:.1e}, least movement {least:.3f})")
        assert g_err <= TOL and k_ratio <= 1.0 and e2e <= E2E_BOUND
        # bands
        assert torch.equal(res.bands, brainxai.band_sums(res.map, bands, T=T, fs=fs)) and res.bands.shape == (Bn, 6, Chans, len(res.band_bins))
        assert np.array_equal(res.bands.cpu().numpy(), R.band_sum(res.map.cpu().numpy(), res.band_bins))
        # delta
        if steps > 1 and map_kind == "gradient_x_amplitude":
            with torch.no_grad():
                zero = (mine(torch.zeros_like(xd)) if other is None else mine(torch.zeros_like(xd), other)).double()
            total = torch.from_numpy(BR.sum_rows(res.map.cpu().numpy().reshape(Bn * 6, -1))).reshape(Bn, 6)
            host = total - (res.out.double() - zero).cpu()
            lmax = float(ref_out.abs().max())
            assert res.delta.shape == (Bn, 6) and res.delta.dtype == torch.float64 and float((res.delta.cpu() - host).abs().max()) <= 1e-5 * lmax
            ref_delta = torch.from_numpy(want.reshape(Bn, 6, -1).sum(-1)) - (ref_out - ref_zero)
            d_tol = E2E_BOUND * torch.from_numpy(R.pair_max(want)) * Chans * (T // 2 + 1) + 2 * TOL * lmax
            print(f"{what}: delta {res.delta.cpu().flatten().tolist()} (reference {ref_delta.flatten().tolist()})")
            assert bool(((res.delta.cpu() - ref_delta).abs() <= d_tol).all())
        else:
            assert res.delta is None
        # the other class forms are slices of 'all'
        if map_kind == R.MAP_KINDS[steps > 1]:
            top = brainxai.spectral_gradients(mine, xd, other, kind=map_kind, steps=steps, return_parts=True)
            assert top.map.shape == (Bn, Chans, T // 2 + 1) and top.gradient.shape == (Bn, 1, Chans, T) and top.bands is None and top.band_bins is None
            assert torch.equal(top.classes, res.out.argmax(1)) and torch.equal(top.out, res.out)
            listed = brainxai.spectral_gradients(mine, xd, other, kind=map_kind, steps=steps, fs=fs, bands=bands, class_idx=[4, 1], return_parts=True)
            assert listed.classes.tolist() == [4, 1] and listed.bands.shape == (Bn, Chans, len(res.band_bins))
            for b in range(Bn):
                for part, c in ((top, int(top.classes[b])), (listed, [4, 1][b])):
                    same_g = torch.equal(part.gradient[b], res.gradient[b, c])
                    assert GG.worst(part.gradient[b][None, None], res.gradient[b, c][None, None]) <= TOL
                    assert not same_g or torch.equal(part.map[b], res.map[b, c]), "the same gradient gives the same map"
                    if part.delta is not None:
                        assert part.delta.shape == (Bn,) and (not same_g or abs(float(part.delta[b] - res.delta[b, c])) <= 1e-5)
            assert torch.equal(brainxai.spectral_gradients(mine, xd, other, kind=map_kind, steps=steps, class_idx=[4, 1]), listed.map)


@pytest.mark.parametrize("kind", ["eegnet", "multimodal"])
def test_no_bit_depends_on_max_batch(kind):
    mine, xd, other = _device_model(kind)
    kw = dict(kind="gradient_x_amplitude", steps=5, class_idx="all", return_parts=True)
    every = brainxai.spectral_gradients(mine, xd, other, **kw)
    for mb in (1, 3):                                # 10 rows in passes of 1 and of 3 (ending inside a sample)
        small = brainxai.spectral_gradients(mine, xd, other, max_batch=mb, **kw)
        same = torch.equal(small.gradient, every.gradient)
        err = GG.worst(small.gradient, every.gradient)
        print(f"spectral_gradients {kind} max_batch {mb} vs 256: gradients bit for bit: {same} ({err:.3e} of the maximum)")
        assert err <= TOL
        if same:
            assert torch.equal(small.map, every.map) and torch.equal(small.delta, every.delta), "given the same gradients no bit of the map depends on max_batch"
        else:                                        # the backward passes differ with the batch: the map follows them within the gradient bound
            assert GG.worst(small.map, every.map) <= TOL


# ---- spectral occlusion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", ["band", "electrode_band"])
@pytest.mark.parametrize("kind", ["eegnet", "multimodal", "small"])
def test_spectral_occlusion_against_the_fp64_oracle(kind, cells):
    mine, xd, other = _device_model(kind)
    ref, x, _ = R.oracle_case(kind)
    Bn, _, Chans, T = x.shape
    F = T // 2 + 1
    # T = 2000 at 40 Hz: two clinical bands, every bin, no bin; 512 samples in cycles per sample: two bands, no bin, every bin
    bands, fs = ([(0.5, 4.0), (4.0, 8.0), (0.0, 30.0), (25.0, 30.0)], 40.0) if T == 2000 else ([(0.0, 0.1), (0.1, 0.25), (0.3, 0.3), (0.0, 0.6)], None)
    res = brainxai.spectral_occlusion(mine, xd, other, bands=bands, fs=fs, cells=cells, class_idx="all", return_parts=True)
    bins = R.band_bins(bands, T, fs)
    nb = len(bins)
    N = nb if cells == "band" else nb * Chans
    assert res.band_bins == bins and res.scores.shape == (Bn, N, 6) and res.clean.shape == (Bn, 6) and res.classes is None
    assert res.drops.shape == ((Bn, 6, nb) if cells == "band" else (Bn, 6, Chans, nb)) and res.drops.dtype == torch.float32
    # the device's own rows through the fp64 oracle
    re, im, _ = brainxai.eeg_spectrum(xd)
    rows = torch.full((Bn * N, 1, Chans, T), float("nan"), dtype=torch.float32, device=DEV)
    _launch_bandstop(xd, re.reshape(-1, F), im.reshape(-1, F), T, torch.tensor(bins, dtype=torch.int32, device=DEV), nb, cells, 0, N, rows)
    rows = rows.cpu()
    f64 = R.copy.deepcopy(ref).double().eval()
    fwd = f64 if other is None else R.two_input(f64, other.cpu(), N)
    want = R.outputs(fwd, rows).exp().reshape(Bn, N, 6)
    clean = R.outputs(f64 if other is None else R.two_input(f64, other.cpu()), x).exp()
    s_err, c_err = float((res.scores.double().cpu() - want).abs().max()), float((res.clean.double().cpu() - clean).abs().max())
    ref_drops = (clean[:, None] - want).permute(0, 2, 1)
    ref_drops = ref_drops if cells == "band" else ref_drops.reshape(Bn, 6, nb, Chans).transpose(2, 3)
    d_err = float((res.drops.double().cpu() - ref_drops).abs().max())
    span = float(ref_drops.abs().max())
    print(f"spectral_occlusion {kind} {cells}: scores {s_err:.2e}, clean {c_err:.2e}, drops {d_err:.2e} (largest drop {span:.3e})")
    assert s_err <= PG.TOL and c_err <= PG.TOL and d_err <= 2 * PG.TOL
    assert span > 100 * 2 * PG.TOL, "the drops are too small to tell anything"
    assert torch.equal(res.drops, (res.clean[:, None] - res.scores).permute(0, 2, 1).reshape(res.drops.shape) if cells == "band" else
                       (res.clean[:, None] - res.scores).permute(0, 2, 1).reshape(Bn, 6, nb, Chans).transpose(2, 3))
    empty = [q for q, (lo, hi) in enumerate(bins) if lo == hi]
    assert empty and float(res.drops[..., empty].abs().max()) <= 2 * PG.TOL, "a band without a bin: its rows are x and take the clean input's path"
    if cells == "band":                              # every bin removed: the zero input, up to the rounding of x - y
        q = bins.index((0, F))
        assert float(rows.reshape(Bn, N, -1)[:, q].abs().max()) <= 2.0 ** -20 * float(x.abs().max())
        zero = R.outputs(f64 if other is None else R.two_input(f64, other.cpu()), torch.zeros_like(x)).exp()
        assert float((res.drops[:, :, q].double().cpu() - (clean - zero)).abs().max()) <= 2 * PG.TOL
    else:                                            # a row differs from x in exactly one electrode
        differs = (rows.reshape(Bn, nb, Chans, Chans, T) != x.reshape(Bn, 1, 1, Chans, T)).any(-1)          # [B, q, e selected, e]
        for q, (lo, hi) in enumerate(bins):
            assert torch.equal(differs[:, q], torch.eye(Chans, dtype=torch.bool).expand(Bn, -1, -1) if lo < hi else torch.zeros(Bn, Chans, Chans, dtype=torch.bool))
    # the class forms agree where they overlap; max_batch changes no bit of a forward-only pass beyond the project's bound
    kw = dict(bands=bands, fs=fs, cells=cells)
    top = brainxai.spectral_occlusion(mine, xd, other, return_parts=True, **kw)
    assert torch.equal(top.classes, res.clean.argmax(1)) and torch.equal(top.scores, res.scores)
    listed = brainxai.spectral_occlusion(mine, xd, other, class_idx=[4, 1], **kw)
    one = brainxai.spectral_occlusion(mine, xd, other, class_idx=2, score="prob", **kw)
    for b in range(Bn):
        assert torch.equal(top.drops[b], res.drops[b, int(top.classes[b])]) and torch.equal(listed[b], res.drops[b, [4, 1][b]]) and torch.equal(one[b], res.drops[b, 2])
    logp = brainxai.spectral_occlusion(mine, xd, other, class_idx="all", score="logprob", return_parts=True, **kw)
    assert float((logp.scores.exp() - res.scores).abs().max()) <= PG.TOL
    chunked = brainxai.spectral_occlusion(mine, xd, other, class_idx="all", max_batch=3, **kw)
    assert float((chunked - res.drops).abs().max()) <= 2 * PG.TOL


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_state_is_restored_and_refusals_hold_on_the_gpu():
    mine, eeg, spec = GG.iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        before = PG.model_state(mine)
        amap = brainxai.spectral_gradients(mine, eeg, spec, steps=2, kind="gradient_x_amplitude")
        drops = brainxai.spectral_occlusion(mine, eeg, spec, bands="clinical", fs=40.0)
        assert PG.model_state(mine) == before and mine.training and not frozen.requires_grad
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    assert amap.shape == (2, 19, 1001) and amap.dtype == torch.float32 and amap.is_cuda and drops.shape == (2, 4) and not eeg.requires_grad
    net = mine.eeg_model                                                     # a stand-alone branch with spec=None
    alone = brainxai.spectral_gradients(net, eeg, None, class_idx="all", return_parts=True)
    with torch.no_grad():
        assert torch.equal(alone.out, net(eeg).float()) and alone.map.shape == (2, 6, 19, 1001) and float(alone.map.abs().max()) > 0
    assert brainxai.spectral_occlusion(net, eeg, None, bands=[(0.0, 0.1)], cells="electrode_band").shape == (2, 19, 1)
    for call, exc, match in [
            (lambda: brainxai.spectral_gradients(mine, eeg, spec, kind="phase"), ValueError, "unknown kind"),
            (lambda: brainxai.spectral_gradients(mine, eeg, spec, steps=0), ValueError, "steps = 0 < 1"),
            (lambda: brainxai.spectral_gradients(mine, spec, spec), ValueError, r"\[B,1,Chans,T\]"),
            (lambda: brainxai.spectral_gradients(mine, eeg, spec, bands="clinical"), ValueError, "need fs"),
            (lambda: brainxai.spectral_gradients(mine, eeg, spec, bands=[(3.0, 1.0)]), ValueError, "negative or inverted"),
            (lambda: brainxai.spectral_gradients(mine, eeg, spec, class_idx=9), ValueError, r"outside \[0, 6\)"),
            (lambda: brainxai.spectral_gradients(mine, eeg.cpu(), spec), RuntimeError, "no CPU path"),
            (lambda: brainxai.spectral_gradients(mine, eeg, spec.cpu()), RuntimeError, "no CPU path"),
            (lambda: brainxai.spectral_occlusion(mine, eeg, spec, bands="clinical", fs=40.0, cells="both"), ValueError, "unknown cells"),
            (lambda: brainxai.spectral_occlusion(mine, eeg, spec, bands=[(-1.0, 2.0)]), ValueError, "negative or inverted"),
            (lambda: brainxai.spectral_occlusion(mine, eeg.cpu(), spec, bands=[(0.0, 0.2)]), RuntimeError, "no CPU path"),
            (lambda: brainxai.eeg_spectrum(eeg.cpu()), RuntimeError, "no CPU path"),
            (lambda: brainxai.band_sums(amap.cpu(), "clinical", T=2000, fs=40.0), RuntimeError, "no CPU path")]:
        with pytest.raises(exc, match=match):
            call()
