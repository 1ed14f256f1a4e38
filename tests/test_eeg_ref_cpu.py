"""The references of the EEGNet shape tests (tests/eeg_ref.py) checked against each other, without a GPU: what
tests/test_gpu_eeg_shapes.py holds the kernels to must (a) be met by the fp32 oracle alone, with room to spare, and (b) tell a
deliberately wrong network -- a dropped last sample, a padding moved by one, a dropped last electrode, a dropped last tap -- from the
right one, by a factor of ten, at every case of the table; and the gradients the table exempts must really vanish."""
import pytest

from tests import eeg_ref as R

# (Chans, Samples, batch, kernLength) of every case the table has to hold
REQUIRED = [(3, 133, 2, 64), (1, 34, 3, 64), (64, 70, 2, 64), (65, 64, 2, 64), (10, 1001, 2, 64), (11, 250, 3, 64), (4, 96, 2, 64), (4, 88, 2, 64),
            (2, 3072, 2, 64), (2, 3080, 2, 64), (5, 131, 2, 1), (5, 131, 2, 8), (5, 131, 2, 32), (5, 131, 2, 33), (5, 131, 2, 63),
            (2, 1030, 256, 64), (2, 1030, 255, 64), (2, 4100, 2, 64), (2, 5100, 2, 64), (2, 15001, 2, 64), (5, 301, 2, 64)]


def test_case_table():
    have = {(c.chans, c.samples, c.batch, c.kern): c for c in R.CASES}
    assert set(REQUIRED) <= set(have), sorted(set(REQUIRED) - set(have))
    assert len({c.tag for c in R.CASES}) == len(R.CASES)
    assert have[(5, 301, 2, 64)].arch == "EEGNetAttentionDeep"
    assert have[(2, 4100, 2, 64)].storages == ("fp32",) and have[(2, 5100, 2, 64)].storages == ("bf16",)
    for c in R.CASES:
        assert set(c.drop) <= set(R.MUTANTS) and all(c.drop.values()), (c.tag, c.drop)          # dropped by name, with a reason
        for bound in ("fp32", "bf16"):
            assert len(R.kept_mutants(c, bound)) >= 3, (c.tag, bound)
        assert "batchnorm1.bias" in c.zero_train and "batchnorm1.weight" in c.eps_train
        assert ("depthwiseConv.weight" in c.eps_train) == (c.chans == 1) and ("conv1.weight" in c.eps_train) == (c.kern == 1), c.tag
        # the tuned layout is defined in the tuned family only
        assert not c.maps or (c.chans <= 64 and c.kern <= 64 and c.samples <= 15000), c.tag


@pytest.mark.parametrize("tag", [c.tag for c in R.CASES])
def test_reference_meets_the_bounds_and_mutants_do_not(tag):
    case = R.BY_TAG[tag]
    failures = []
    for mode in ("eval", "train"):
        zero = R.zero_grads(case, mode)
        ex = R.reference(tag, mode, "exact")
        # (1) the fp32 oracle alone is within the fp32 tolerance of the fp64 one
        d32 = R.deviations(R.reference(tag, mode, "oracle32"), ex, zero)
        worst = max(d32, key=lambda n: d32[n] / R.fp32_limit(n, zero))
        print(f"[eeg-ref] {tag} {mode}: fp32 oracle worst {worst} {d32[worst]:.2e} (tolerance {R.fp32_limit(worst, zero):.0e})")
        failures += [f"{mode} fp32 oracle {n}: {e:.3e}" for n, e in d32.items() if not e <= R.fp32_limit(n, zero)]
        # (2) the exempted gradients vanish: exactly (fp64 rounding) or up to BatchNorm's eps (far below the floor they are compared on)
        gmax = max(float(g.abs().max()) for g in ex["grads"].values())
        exact0 = case.zero_train if mode == "train" else case.zero_eval
        eps0 = case.eps_train if mode == "train" else ()
        for n, g in ex["grads"].items():
            rel = float(g.abs().max()) / gmax
            if n in exact0 and not rel < 1e-12:
                failures.append(f"{mode} d{n} is exempted as exactly zero but is {rel:.2e} of the largest gradient entry")
            if n in eps0:
                print(f"[eeg-ref] {tag} {mode}: d{n} = {rel:.2e} of the largest gradient entry (zero up to BatchNorm's eps)")
                if not rel < 1e-3:        # a tenth of the floor 1e-2: the floor, not the gradient's own size, sets the scale of the comparison
                    failures.append(f"{mode} d{n} is exempted as vanishing but is {rel:.2e} of the largest gradient entry")
            if n not in zero and not rel > 1e-6:
                failures.append(f"{mode} d{n} is {rel:.2e} of the largest gradient entry and not in the table's exemptions")
        # (3) every mutant moves some compared quantity by more than ten times its tolerance: the fp32 one, and for the elementwise maps and
        # the input gradient the bf16 one
        rounded = R.reference(tag, mode, "rounded")
        lim16 = R.bf16_limits(R.reference(tag, mode, "twin"), rounded, zero)
        E = {n: lim16[n] / R.BF16_FACTOR for n in R.ELEMENTWISE}
        print(f"[eeg-ref] {tag} {mode}: bf16 bounds " + ", ".join(f"{n} {lim16[n]:.2e}" for n in R.ELEMENTWISE) + f" (max(E_q, 2^-9) {min(E.values()):.2e} .. {max(E.values()):.2e})")
        x, r = R.inputs(case)
        for m in R.MUTANTS:
            mu = R.mutants(R.model_kwargs(case), x, r, mode, case.arch, names=(m,))[m]
            dm = R.deviations(mu, ex, zero)
            f32 = max(dm[n] / R.fp32_limit(n, zero) for n in dm)
            dmb = R.deviations(mu, ex, zero, floored=False)
            f16 = max(dmb[n] / lim16[n] for n in R.ELEMENTWISE)
            print(f"[eeg-ref] {tag} {mode}: mutant {m:14s} moves a quantity to {f32:8.1f} x the fp32 tolerance, a map to {f16:6.1f} x the bf16 bound")
            if m in R.kept_mutants(case, "fp32") and not f32 > 10.0:
                failures.append(f"{mode} mutant {m}: only {f32:.2f} x the fp32 tolerance")
            if m in R.kept_mutants(case, "bf16") and not f16 > 10.0:
                failures.append(f"{mode} mutant {m}: only {f16:.2f} x the bf16 bound")
    assert not failures, f"{tag}: " + "; ".join(failures)


def test_rounded_twin_differs_from_exact_only_by_storage():
    """The twin and exact(rounded=True) see the same bf16-representable x and conv1.weight (so operand rounding is no part of E_q), and the
    twin's depthwise map differs by what a bf16 conv1 output gives: more than fp64 rounding, less than a percent."""
    tag = "eeg3x133b2k64"
    ex, tw, full = R.reference(tag, "train", "rounded"), R.reference(tag, "train", "twin"), R.reference(tag, "train", "exact")
    for k in ("conv1.weight", "depthwiseConv.weight"):
        assert (ex["state"][k] == tw["state"][k]).all()
    assert (ex["x"] == tw["x"]).all() and (R.bf16_round(ex["x"]) == ex["x"]).all() and not (full["x"] == ex["x"]).all()
    assert (R.bf16_round(ex["state"]["conv1.weight"]) == ex["state"]["conv1.weight"]).all()
    e = R.deviations(tw, ex, floored=False)
    assert 1e-4 < e["dw"] < 1e-2 and 1e-4 < e["dx"] < 1e-2, e


def test_route_is_a_function_of_the_descriptor():
    """Rows the register-tiled backward cannot hold (T > 256 * EEG_DX_MAX = 4096) go to the general kernels whenever the descriptor
    announces a backward (training mode, or grad = 1), in every entry point alike; an evaluation-mode pass nothing differentiates keeps
    the tuned forward and its arena layout up to T = 15000."""
    import ctypes

    from brainxai import _lib
    lib = _lib.load()
    BX_EUNSUPPORTED = -6

    def desc(T, training, grad, dtype=_lib.BX_F32, collapse=0, B=2):
        d = _lib.EegDesc(B, 2, T, 8, 2, 16, 64, 16, 4, 8, training, 1e-5, 0.1, 0.0, 0, dtype, collapse, -1.0)
        d.grad = grad
        return d

    def tuned(d):
        off_d, off_s = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib.bx_eeg_saved_layout(ctypes.byref(d), ctypes.byref(off_d), ctypes.byref(off_s))
        assert rc in (0, BX_EUNSUPPORTED)
        return rc == 0

    for T in (4096, 4100, 5100, 15000, 15001):
        for training in (0, 1):
            for grad in (0, 1):
                for collapse in (0, 1):
                    d32, d16 = desc(T, training, grad, _lib.BX_F32, collapse), desc(T, training, grad, _lib.BX_BF16, collapse)
                    want = T <= 15000 and (T <= 4096 or not (training or grad))
                    assert tuned(d32) == want and tuned(d16) == want, (T, training, grad, collapse)
                    n32, n16 = lib.bx_eeg_saved_bytes(ctypes.byref(d32)), lib.bx_eeg_saved_bytes(ctypes.byref(d16))
                    assert n32 > 0 and n16 > 0 and lib.bx_eeg_workspace(ctypes.byref(d32)) > 0 and lib.bx_eeg_workspace(ctypes.byref(d16)) > 0
                    # bx_eeg_saved_bytes follows the same predicate: only the tuned route stores the conv1 output in the storage type
                    # (the general kernels keep it in fp32 whatever the descriptor says)
                    assert (n16 < n32) == want, (T, training, grad, collapse, n16, n32)
    assert tuned(desc(4096, 1, 1, B=256)) and not tuned(desc(4097, 1, 0)) and not tuned(desc(4097, 0, 1)) and tuned(desc(4097, 0, 0))
