"""GPU: brainxai.blur_ig / blur_path / gaussian_blur and the bx_blur_rows / bx_blurig_* entry points against the restatement of the
definition (tests/blur_ig_ref.py): the rows X and their scale derivative D against fp64 filters of the same fp32 taps, the identity rows
bit for bit, the running sum and the row sum bit for bit numpy's in the same order, the blur against scipy, and the attributions end to
end against the oracle's classes run in fp64 on the CPU.

Bounds.  Rows (derived in blur_ig_ref.rows_bound from the operations): a chain of T fmaf has T roundings, so its error is at most
T u sum|t_i x_i| <= T u A M with u = 2^-24, A = sum |fp32 taps| of the pass, M = max |x| of the sample, T = the taps that can land inside
the image = min(2 R_b + 1, extent); the rounding of the intermediate is the last of those T.  One axis: X within (T + 1) u A_a M, D within
(T + 1) u A_d M (the 1 covers the second-order terms up to T = 4096).  Both axes: the error of the horizontal pass is carried through the
vertical taps, and D's vertical chain has 2 T_y terms: X within (T_x + T_y + 2) u A_a^2 M, D within (2 T_y + T_x + 2) u (A_b A_d + A_d A_a) M.
gaussian_blur against scipy (whose taps are fp64): the bound of X plus the rounding of the taps, u A M per filtered axis (a relative
error u on every tap, carried through the other pass).  Sums: bit for bit.  End to end, per (sample, class):
TOL sum_i |w_i| max|g_i| max|D_i| with TOL = 1e-3, the project's fp32 gradient bound (TOL of tests/test_gpu_parity.py).
The reference's rows and D end to end are the device's own dump (brainxai.blur_path), which the row tests pin.  Every end-to-end case
is first checked ON THE REFERENCE SIDE to discriminate: with D negated, with the schedule halved and with the rows replaced by the
unblurred input the fp64 attribution of every (sample, class) moves by more than 100 x TOL of its maximum -- a driver that dropped the
sign, the schedule or the blur cannot pass.  The EEG branch (ELU, average pooling: no decisions) is compared with the plain fp64 oracle;
the spectrogram branch with the fp64 oracle whose ReLU / max-pool decisions are pinned to those of the GPU forward of the same rows
(tests/golden_util.matched_oracle).  Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import blur_ig_ref as R
from tests import grad_gpu as GG
from tests import perturb_gpu as PG
from tests.golden_util import matched_oracle
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-3
EPS = 0.01

# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
# trailing shape of the input: a spectrogram [C,H,W] or an EEG input [1,Chans,T]; widths 24 and 64 take the 16-byte path, 75, 7, 333, 1
# and 9 the element-by-element one; 100 x 75 and 19 x 2000 need more than one workgroup per plane or line
SHAPES = {"spec 2x16x24": (2, 16, 24), "spec 3x100x75": (3, 100, 75), "spec 4x32x64": (4, 32, 64), "spec 1x5x7": (1, 5, 7), "eeg 5x333": (1, 5, 333),
          "eeg 19x2000": (1, 19, 2000), "eeg 1x1": (1, 1, 1), "eeg 7x9": (1, 7, 9)}
CASES = [(name, axes) for name in sorted(SHAPES) for axes in (("w",) if name.startswith("eeg") else ("hw", "h", "w"))]
KB, KN = 3, 5
WINDOWS = [(0, 15), (2, 10), (14, 1)]              # all rows; from inside sample 0 to inside sample 2; the last row alone


def _case_sigmas(shape, axes):
    """Five scales: 0 (R_b = 0, the identity); 0.37 (radii 1 and 2); a mid radius (6); R = the smaller filtered extent - 1; R beyond the
    larger filtered extent, so that every tap run is clipped on both sides."""
    ext = [shape[1 + "hw".index(a)] for a in axes]
    sig = [0.0, 0.37, 1.5, (min(ext) - 1) / 4.0, max(ext) / 4.0 + 1.0]
    rad = [R.step_taps(s, EPS)[3] for s in sig]
    assert rad[0] == (0, 0) and rad[1] == (1, 2) and rad[2] == (6, 6) and rad[3] == (min(ext) - 1,) * 2 and rad[4][0] > max(ext)
    return sig


def _kernel_input(name):
    x = O.seeded((KB, *SHAPES[name]), 300 + sorted(SHAPES).index(name), "randn")
    x.view(-1)[::7] = -0.0
    x[1] = 2.5                                      # a constant sample
    return x


@functools.lru_cache(maxsize=None)
def _kernel_case(name, axes):
    """(x, sigmas, taps, radius, want X, want D fp64 [KB*KN, ...], bound X, bound D fp64 [KB*KN]); computed once, never written to."""
    x = _kernel_input(name)
    sig = _case_sigmas(SHAPES[name], axes)
    taps, rad = R.table(sig, EPS)
    wx, wd = R.path(x.numpy(), sig, EPS, axes)
    bounds = [R.rows_bound(x.numpy(), s, EPS, axes) for s in sig]
    bx, bd = np.stack([b[0] for b in bounds], 1), np.stack([b[1] for b in bounds], 1)          # [KB, KN]
    return x, sig, taps, rad, wx.reshape(KB * KN, *SHAPES[name]), wd.reshape(KB * KN, *SHAPES[name]), bx.reshape(-1), bd.reshape(-1)


def _ratio(err, bound):
    """err / bound; an all-zero sample has the bound 0, which only the error 0 meets."""
    return float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf"))


def _launch_rows(x, taps_d, rad_d, TW, out, deriv, shape, axes, row0, rows, n=KN, B=KB, per_sample=0):
    L.check(L.load().bx_blur_rows(PG.p(x), PG.p(taps_d), PG.p(rad_d), PG.p(out), PG.p(deriv), B, n, shape[0], shape[1], shape[2], X._BLUR_AXES[axes], TW,
                                  per_sample, row0, rows, PG.stream()), "bx_blur_rows")


@pytest.mark.parametrize("name,axes", CASES)
def test_rows_against_the_fp64_restatement(name, axes):
    shape = SHAPES[name]
    x, sig, taps, rad, wx, wd, bx, bd = _kernel_case(name, axes)
    xd, taps_d, rad_d = PG.dev(x), PG.dev(taps), PG.dev(rad)
    paths = [("aligned", xd, False), ("misaligned input", PG.misaligned(xd), False), ("misaligned output", xd, True)]
    worst = [0.0, 0.0]
    for row0, rows in WINDOWS:
        for what, xin, mis_out in paths:
            out = torch.full((rows, *shape), float("nan"), dtype=torch.float32, device=DEV)
            der = torch.full((rows, *shape), float("nan"), dtype=torch.float32, device=DEV)
            if mis_out:
                out, der = PG.misaligned(out), PG.misaligned(der)
            _launch_rows(xin, taps_d, rad_d, taps.shape[2], out, der, shape, axes, row0, rows)
            alone = torch.full((rows, *shape), float("nan"), dtype=torch.float32, device=DEV)            # without D: the same X
            _launch_rows(xin, taps_d, rad_d, taps.shape[2], alone, None, shape, axes, row0, rows)
            got_x, got_d = out.cpu().numpy(), der.cpu().numpy()
            where = f"{name} axes {axes} rows {row0}..{row0 + rows}, {what}"
            assert not np.isnan(got_x).any() and not np.isnan(got_d).any(), f"{where}: elements left unwritten"
            assert np.array_equal(PG.np_bits(alone.cpu().numpy()), PG.np_bits(got_x)), f"{where}: X without D differs from X with D"
            for r in range(rows):
                j = row0 + r
                if rad[j % KN, 1] == 0:              # R_b = 0: x bit for bit, signs of zero included, and D = +0
                    assert np.array_equal(PG.np_bits(got_x[r]), PG.np_bits(x[j // KN].numpy())), f"{where}: identity row {j}"
                    assert not PG.np_bits(got_d[r]).any(), f"{where}: D of identity row {j} is not +0"
                    continue
                ex = _ratio(np.abs(got_x[r] - wx[j]).max(), bx[j])
                ed = _ratio(np.abs(got_d[r] - wd[j]).max(), bd[j])
                worst = [max(worst[0], ex), max(worst[1], ed)]
                assert ex <= 1.0 and ed <= 1.0, f"{where}: row {j} (sigma {sig[j % KN]:.4g}) X {ex:.3f}, D {ed:.3f} x the bound"
    print(f"rows {name} axes {axes}: radii {rad.tolist()}; worst X {worst[0]:.3f}, D {worst[1]:.3f} x the bound; windows {WINDOWS} aligned and misaligned")


@pytest.mark.parametrize("name,axes", [("spec 2x16x24", "hw"), ("spec 1x5x7", "h"), ("eeg 7x9", "w"), ("eeg 5x333", "w")])
def test_all_radii_zero_is_the_input_bit_for_bit(name, axes):
    shape = SHAPES[name]
    x = _kernel_input(name)
    sig = [0.0, 0.05, 0.1, 0.11, 0.0]                                   # R(sigma + 0.01) = 0 for all of them
    taps, rad = R.table(sig, EPS)
    assert not rad.any() and taps.shape[2] == 1
    for xin, mis in ((PG.dev(x), False), (PG.misaligned(PG.dev(x)), True)):
        out = torch.full((KB * KN, *shape), float("nan"), dtype=torch.float32, device=DEV)
        der = torch.full((KB * KN, *shape), float("nan"), dtype=torch.float32, device=DEV)
        if mis:
            out, der = PG.misaligned(out), PG.misaligned(der)
        _launch_rows(xin, PG.dev(taps), PG.dev(rad), 1, out, der, shape, axes, 0, KB * KN)
        want = x.numpy()[:, None].repeat(KN, 1).reshape(KB * KN, *shape)
        assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(want)) and not PG.np_bits(der.cpu().numpy()).any()


@pytest.mark.parametrize("Kc", [1, 3])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accumulate_bit_for_bit(name, Kc):
    shape = SHAPES[name]
    per, rows_all, n, slot = int(np.prod(shape)), KB * KN, KN, Kc // 2
    g, D = O.seeded((rows_all, *shape), 7, "randn"), O.seeded((rows_all, *shape), 8, "randn")
    g.view(-1)[::5] = -0.0
    w = np.random.default_rng(4).standard_normal(n)
    lib, gd, Dd, wd = L.load(), PG.dev(g), PG.dev(D), PG.dev(w)
    SENTINEL = 7.25

    def run(splits, mis=False):
        acc = torch.full((KB, Kc, per), SENTINEL, dtype=torch.float64, device=DEV)
        acc[:, slot] = 0.0
        for row0, rows in splits:
            gs, Ds = gd[row0:row0 + rows].contiguous(), Dd[row0:row0 + rows].contiguous()
            if mis:
                gs, Ds = PG.misaligned(gs), PG.misaligned(Ds)
            L.check(lib.bx_blurig_accumulate(PG.p(gs), PG.p(Ds), PG.p(wd), PG.p(acc), KB, n, per, Kc, slot, row0, rows, PG.stream()), "bx_blurig_accumulate")
        return acc
    one, two, three = run([(0, rows_all)]), run([(0, 7), (7, rows_all - 7)]), run([(0, 2), (2, 10), (12, 2), (14, 1)], mis=True)
    assert torch.equal(one, two) and torch.equal(one, three), f"{name}: calls split inside a sample differ from one call"
    others = [k for k in range(Kc) if k != slot]
    assert bool((one[:, others] == SENTINEL).all()), "the slots of other classes were touched"
    want = R.accumulate(g.numpy(), D.numpy(), w, KB, n)
    assert np.array_equal(one[:, slot].cpu().numpy(), want[:, 0]), f"{name}: the fp64 sums are not numpy's in the same order"


@pytest.mark.parametrize("Ln", [1, 63, 64, 65, 1665, 38000])
def test_row_sum_bit_for_bit(Ln):
    v = O.seeded((5, Ln), 21, "randn")
    v.view(-1)[::3] *= 1e-3
    for vd in (PG.dev(v), PG.misaligned(PG.dev(v))):
        out = torch.full((5,), float("nan"), dtype=torch.float64, device=DEV)
        L.check(L.load().bx_blurig_sum_rows(PG.p(vd), PG.p(out), 5, Ln, PG.stream()), "bx_blurig_sum_rows")
        assert np.array_equal(PG.np_bits(out.cpu().numpy()), PG.np_bits(R.sum_rows(v.numpy())))


@pytest.mark.parametrize("name,axes", CASES)
def test_gaussian_blur_against_scipy(name, axes):
    shape = SHAPES[name]
    x = _kernel_input(name)
    ext = [shape[1 + "hw".index(a)] for a in axes]
    per_sample = [0.0, 1.5, max(ext) / 4.0 + 1.0]
    worst = 0.0
    for sigma in (2.0, per_sample, torch.tensor(per_sample)):
        got = brainxai.gaussian_blur(x.to(DEV), sigma, axes=axes)
        assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy()
        ss = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (KB,))
        for b in range(KB):
            if ss[b] == 0:
                assert np.array_equal(PG.np_bits(got[b]), PG.np_bits(x[b].numpy())), "sigma = 0 returns the sample bit for bit"
                continue
            sc = [0.0, 0.0, 0.0]
            for a in axes:
                sc[1 + "hw".index(a)] = ss[b]
            want = ndimage.gaussian_filter(x[b].double().numpy(), sigma=sc, mode="constant", truncate=4.0)
            a32 = R.taps64(float(ss[b])).astype(np.float32)
            A, M, T = float(np.abs(a32).sum()), float(x[b].abs().max()), [min(len(a32), e) for e in ext]
            u = 2.0 ** -24
            bound = ((sum(T) + 2) * u * A ** len(ext) * M if len(ext) == 2 else (T[0] + 1) * u * A * M) + len(ext) * u * A ** len(ext) * M
            assert np.abs(R.blur(x[b:b + 1].numpy(), ss[b], axes)[0] - want).max() <= len(ext) * u * A ** len(ext) * M, "the restatement against scipy"
            ratio = _ratio(np.abs(got[b] - want).max(), bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{name} axes {axes} sigma {ss[b]}: {ratio:.3f} x the bound"
    print(f"gaussian_blur {name} axes {axes}: worst {worst:.3f} x the bound against scipy.ndimage.gaussian_filter")


def test_blur_path_is_the_row_kernel():
    name, axes, n, ms = "spec 3x100x75", "hw", 4, 6.0
    x = _kernel_input(name)
    for sqrt in (False, True):
        rows, deriv, sig = brainxai.blur_path(x.to(DEV), steps=n, max_sigma=ms, sqrt=sqrt)
        assert sig == R.sigmas(n, ms, sqrt) and rows.shape == deriv.shape == (KB, n, *SHAPES[name]) and rows.dtype == deriv.dtype == torch.float32
        wx, wd = R.path(x.numpy(), sig[:n], EPS, axes)
        for i in range(1, n):
            bx, bd = R.rows_bound(x.numpy(), sig[i], EPS, axes)
            assert (np.abs(rows[:, i].cpu().numpy() - wx[:, i]).reshape(KB, -1).max(1) <= bx).all()
            assert (np.abs(deriv[:, i].cpu().numpy() - wd[:, i]).reshape(KB, -1).max(1) <= bd).all()
        assert torch.equal(rows[:, 0].cpu(), x) and not deriv[:, 0].any()
        last = brainxai.gaussian_blur(x.to(DEV), sig[n - 1])
        assert torch.equal(last, rows[:, n - 1]), "gaussian_blur at a path's sigma is the path's row, bit for bit"
    ex = _kernel_input("eeg 5x333").to(DEV)
    r_w, d_w, _ = brainxai.blur_path(ex, steps=3, max_sigma=5.0, axes="w")
    assert torch.equal(r_w[:, 2], brainxai.gaussian_blur(ex, 2 * 5.0 / 3, axes="w"))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
EN = 6
MAX_SIGMA = {"eeg": 8.0, "spec": 3.0}


def _device_path(x, input, sqrt):
    rows, deriv, sig = brainxai.blur_path(x.to(DEV), steps=EN, max_sigma=MAX_SIGMA[input], sqrt=sqrt, grad_step=EPS, axes="w" if input == "eeg" else "hw")
    return rows.cpu(), deriv.cpu(), sig


def guard(what, forward, x, rows, deriv, sig, want, input, sqrt):
    """Reference side alone: the attribution discriminates the sign of D, the schedule and the blur of the rows."""
    n, axes = len(sig) - 1, "w" if input == "eeg" else "hw"
    half = R.sigmas(n, MAX_SIGMA[input] / 2, sqrt)
    rows_h, deriv_h = R.path(x.numpy(), half[:n], EPS, axes)
    plain = x[:, None].expand(-1, n, *x.shape[1:])
    moved = {"D negated": R.values(forward, rows, -deriv, R.weights(sig))[0], "schedule halved": R.values(forward, rows_h, deriv_h, R.weights(half))[0],
             "rows unblurred": R.values(forward, plain, deriv, R.weights(sig))[0]}
    least = {how: float((GG.per_pair_max(alt - want) / GG.per_pair_max(want)).min()) for how, alt in moved.items()}
    print(f"{what}: the reference moves by (least over (sample, class), of its maximum) " + ", ".join(f"{how} {v:.3f}" for how, v in least.items()))
    for how, v in least.items():
        assert v > 100 * TOL, f"{what}: {how} moves the reference by only {v:.3e}"


def _check(what, res, want, scale, ref_out, ref_end, per):
    """values within TOL scale per (sample, class); endpoint within TOL of the largest |log-probability|; delta against the reference's
    own within per * TOL * scale (every element's bound, summed) plus the two outputs' bounds, and against the device's own parts."""
    got = res.values.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    ratio = float((GG.per_pair_max(got - want) / (TOL * scale)).max())
    print(f"{what}: values {ratio:.3e} x the bound ({float((GG.per_pair_max(got - want) / GG.per_pair_max(want)).max()):.3e} of the maximum)")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} x the bound"
    lmax = float(ref_out.abs().max())
    assert float((res.out.double().cpu() - ref_out).abs().max()) <= TOL * lmax and float((res.endpoint.double().cpu() - ref_end).abs().max()) <= TOL * lmax
    ref_delta = want.flatten(2).sum(2) - (ref_out - ref_end)
    d_err = (res.delta.cpu() - ref_delta).abs() / (per * TOL * scale + 2 * TOL * lmax)
    own = torch.from_numpy(R.sum_rows(res.values.cpu().numpy().reshape(-1, per))).reshape(want.shape[:2]) - (res.out.double().cpu() - res.endpoint.double().cpu())
    assert torch.equal(res.delta.cpu(), own), f"{what}: delta is not the fixed-order sum of the values minus the drop of the outputs"
    print(f"{what}: delta {res.delta.cpu().flatten().tolist()} (reference {ref_delta.flatten().tolist()}), {float(d_err.max()):.3e} x its bound")
    assert float(d_err.max()) <= 1.0


@pytest.mark.parametrize("sqrt", [False, True], ids=["linear", "sqrt"])
@pytest.mark.parametrize("kind", ["eegnet", "multimodal", "deep"])
def test_eeg_input_against_the_fp64_oracle(kind, sqrt):
    _, mine, f64, x, other = GG.eeg_models(kind)
    rows, deriv, sig = _device_path(x, "eeg", sqrt)
    forward = f64 if other is None else R.two_input(f64, other, "eeg", EN)
    want, scale = R.values(forward, rows, deriv, R.weights(sig))
    what = f"blur_ig eeg input, {kind}, sqrt={sqrt}"
    guard(what, forward, x, rows, deriv, sig, want, "eeg", sqrt)
    res = brainxai.blur_ig(mine, x.to(DEV), None if other is None else other.to(DEV), input="eeg", steps=EN, max_sigma=MAX_SIGMA["eeg"], sqrt=sqrt,
                           class_idx="all", return_parts=True)
    assert res.values.shape == (2, 6, 1, 19, 2000) and res.map.shape == (2, 6, 19, 2000) and res.classes is None and res.delta.dtype == torch.float64
    assert (res.sigmas, res.steps, res.max_sigma, res.sqrt, res.grad_step, res.axes) == (sig, EN, MAX_SIGMA["eeg"], sqrt, EPS, "w")
    assert torch.equal(res.map, res.values[:, :, 0])
    one = f64 if other is None else R.two_input(f64, other, "eeg")
    end = R.outputs(one, brainxai.gaussian_blur(x.to(DEV), sig[EN], axes="w").cpu())
    _check(what, res, want, scale, R.outputs(one, x), end, 19 * 2000)


@pytest.mark.parametrize("sqrt", [False, True], ids=["linear", "sqrt"])
@pytest.mark.parametrize("kind", ["spectrogram", "multimodal"])
def test_spec_input_against_the_decision_matched_oracle(kind, sqrt):
    ref, mine = PG.scaled_multimodal()
    eeg, spec = GG.mm_inputs()
    if kind == "spectrogram":
        ref, mine, eeg = ref.spectrogram_model, mine.spectrogram_model, None
    rows, deriv, sig = _device_path(spec, "spec", sqrt)
    f64 = copy.deepcopy(ref).double().eval()
    plain_fwd = f64 if eeg is None else R.two_input(f64, eeg, "spec", EN)
    plain, _ = R.values(plain_fwd, rows, deriv, R.weights(sig))
    what = f"blur_ig spec input, {kind}, sqrt={sqrt}"
    guard(what, plain_fwd, spec, rows, deriv, sig, plain, "spec", sqrt)
    res = brainxai.blur_ig(mine, None if eeg is None else eeg.to(DEV), spec.to(DEV), input="spec", steps=EN, max_sigma=MAX_SIGMA["spec"], sqrt=sqrt,
                           class_idx="all", return_parts=True)
    assert res.values.shape == (2, 6, 4, 32, 64) and res.map.shape == (2, 6, 32, 64) and res.axes == "hw"
    v64 = res.values.double()                                           # the map rounds the fp64 channel sum once, the values each once
    assert bool(((res.map.double() - v64.sum(2)).abs() <= 2.0 ** -24 * (v64.abs().sum(2) + res.map.double().abs()) + 1e-45).all()), "the map is the channel sum"
    # the decisions of the GPU forward of the same rows: one pass of 12 rows through the spectrogram branch
    flat = rows.reshape(2 * EN, *spec.shape[1:])
    keep = ops.keep_block_activations(mine)
    try:
        with X._eval_frozen(mine):
            (mine.spectrogram_model if eeg is not None else mine)(flat.to(DEV).requires_grad_(True))
        torch.cuda.synchronize()
    finally:
        ops.keep_block_activations(mine, on=False)
    args = (flat,) if eeg is None else (eeg.repeat_interleave(EN, dim=0), flat)
    twin, flips = matched_oracle(O, ref, args, keep, what)
    print(f"{what}: {len(flips)} decision flips")
    want, scale = R.values((lambda xi: twin(xi)) if eeg is None else (lambda xi: twin(args[0].double(), xi)), rows, deriv, R.weights(sig))
    one = f64 if eeg is None else R.two_input(f64, eeg, "spec")
    end = R.outputs(one, brainxai.gaussian_blur(spec.to(DEV), sig[EN]).cpu())
    _check(what, res, want, scale, R.outputs(one, spec), end, 4 * 32 * 64)


# ---- interface --------------------------------------------------------------------------------------------------------------------------
def test_class_forms_and_max_batch():
    mine, eeg, spec = GG.iface()
    for input, shape in (("eeg", (19, 2000)), ("spec", (32, 64))):
        kw = dict(input=input, steps=EN, max_sigma=MAX_SIGMA[input])
        every = brainxai.blur_ig(mine, eeg, spec, class_idx="all", return_parts=True, **kw)
        assert every.map.shape == (2, 6, *shape) and every.out.shape == every.endpoint.shape == (2, 6) and every.delta.shape == (2, 6) and every.classes is None
        top = brainxai.blur_ig(mine, eeg, spec, return_parts=True, **kw)
        assert top.map.shape == (2, *shape) and top.values.dim() == 4 and top.delta.shape == (2,)
        assert torch.equal(top.classes, every.out.argmax(1)) and torch.equal(top.out, every.out) and torch.equal(top.endpoint, every.endpoint)
        for b in range(2):
            assert torch.equal(top.map[b], every.map[b, int(top.classes[b])]) and torch.equal(top.delta[b], every.delta[b, int(top.classes[b])])
        for form in ([4, 1], torch.tensor([4, 1]), np.array([4, 1])):
            per = brainxai.blur_ig(mine, eeg, spec, class_idx=form, return_parts=True, **kw)
            assert per.classes.tolist() == [4, 1]
            assert torch.equal(per.map[0], every.map[0, 4]) and torch.equal(per.map[1], every.map[1, 1])
        assert torch.equal(brainxai.blur_ig(mine, eeg, spec, class_idx=2, **kw), every.map[:, 2])
        for mb in (5, 1):                            # 12 rows in passes of 5 (ending inside a sample) and of 1
            small = brainxai.blur_ig(mine, eeg, spec, class_idx="all", max_batch=mb, return_parts=True, **kw)
            err = GG.worst(small.values, every.values)
            print(f"blur_ig {input} max_batch {mb} vs 256: {err:.3e} of the per-(sample, class) maximum, bit for bit: {torch.equal(small.values, every.values)}")
            assert err <= TOL


def test_downstream_and_restored_state():
    mine, eeg, spec = GG.iface()
    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        res = brainxai.blur_ig(mine, eeg, spec, input="spec", steps=4, max_sigma=3.0, sqrt=True, return_parts=True)
        assert mine.training and not frozen.requires_grad and all(p.requires_grad for p in mine.parameters() if p is not frozen)
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    for input, x in (("spec", spec), ("eeg", eeg)):
        amap = res.map if input == "spec" else brainxai.blur_ig(mine, eeg, spec, input="eeg", steps=4, max_sigma=8.0)
        ranks = brainxai.attribution_ranks(amap)
        assert ranks.shape == (2, amap[0].numel())
        curves = brainxai.deletion_insertion(mine, eeg, spec, amap, input=input, steps=4)
        assert torch.equal(curves.ranks, ranks) and bool(torch.isfinite(curves.deletion).all()) and bool(torch.isfinite(curves.insertion).all())
        blurred = brainxai.gaussian_blur(x, 4.0, axes="hw" if input == "spec" else "w")
        based = brainxai.deletion_insertion(mine, eeg, spec, amap, input=input, steps=4, baseline=blurred)
        assert bool(torch.isfinite(based.deletion).all()) and not torch.equal(based.deletion, curves.deletion)
    sm = mine.spectrogram_model
    alone = brainxai.blur_ig(sm, None, spec, steps=4, max_sigma=3.0, axes="w", class_idx="all", return_parts=True)
    assert alone.values.shape == (2, 6, 4, 32, 64) and alone.axes == "w" and float(alone.values.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(alone.out, sm(spec).float())
