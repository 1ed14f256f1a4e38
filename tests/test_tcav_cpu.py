"""CPU: TCAV's reference against an independent dual solve, the package's Welch test against scipy, the orientation of the CAVs and every
refusal of ``train_cavs`` / ``tcav`` (none of which needs a device).

The primal reference (tests/tcav_ref.py) and the dual solve written here (the algebra of include/brainxai.h, "TCAV", in numpy) must give
the same w within tcav_ref.fit_tolerance: 16 (rows + D) 2^-53 cond with cond = rows / ridge + 1."""
import numpy as np
import pytest
import scipy.stats
import torch

import brainxai
from brainxai import explain as X
from tests import tcav_ref as R


def _sets(n, D, count, seed, offset=3.0):
    rng = np.random.default_rng(seed)
    return [np.maximum(rng.standard_normal((n, D)) + offset, 0.0) + 0.3 * s * rng.standard_normal(D) for s in range(count)]


def _dual(sets, sp, sn, ridge):
    """(w, lambda, decision) by the dual route: global centring, G0, K = H G0[I,I] H, (K + lambda I) alpha = H y, beta = H alpha."""
    A = np.concatenate(sets)
    n = sets[0].shape[0]
    Ac = A - A.mean(axis=0)
    G0 = Ac @ Ac.T
    I = np.concatenate([sp * n + np.arange(n), sn * n + np.arange(n)])
    y = np.concatenate([np.ones(n), -np.ones(n)])
    H = np.eye(2 * n) - 1.0 / (2 * n)
    K = H @ G0[np.ix_(I, I)] @ H
    lam = ridge * np.trace(K) / (2 * n)
    beta = H @ np.linalg.solve(K + lam * np.eye(2 * n), H @ y)
    s = G0[np.ix_(I, I)] @ beta
    return beta @ Ac[I], lam, s - s.mean() + y.mean()


@pytest.mark.parametrize("n,D,Rn", [(2, 1, 2), (3, 7, 2), (8, 257, 3), (20, 4099, 3)])
def test_primal_reference_matches_dual(n, D, Rn):
    sets = _sets(n, D, 1 + Rn, 100 + n)
    ref = R.fit_all(sets, 1, "ridge", 1e-2, 0.0)
    assert len(ref) == Rn + Rn
    for (q, r, sp, sn), f in zip(R.problems(1, Rn), ref):
        w, lam, dec = _dual(sets, sp, sn, 1e-2)
        tol = R.fit_tolerance(2 * n, D, f["cond_bound"])
        err = np.sqrt(((w - f["w"]) ** 2).sum()) / f["norm"]
        print(f"n={n} D={D} problem {(q, r)}: |w_dual - w_primal| / |w| = {err:.2e}, bound {tol:.2e}")
        assert err <= tol
        assert abs(lam - f["lam"]) <= tol * f["lam"]
        assert np.abs(dec - f["decision"]).max() <= tol * (f["norm"] * f["radius"] + 1.0)


@pytest.mark.parametrize("classifier", ["ridge", "mean_difference"])
def test_orientation(classifier):
    sets, d = R.planted(12, 40, 3.0, 5, sets=3)
    for f in R.fit_all(sets, 1, classifier, 1e-2, 0.25)[:2]:
        assert f["decision"][:12].mean() > f["decision"][12:].mean()
        assert f["v"] @ d > 0
        assert abs(f["v"] @ f["v"] - 1.0) < 1e-12


def test_welch_against_scipy():
    rng = np.random.default_rng(1)
    for Rn in (2, 3, 10):
        a, b = rng.random((4, 5, Rn)), rng.random((5, Rn))
        t, dof, p = brainxai.welch_t_test(a, b[None])
        want = scipy.stats.ttest_ind(a, np.broadcast_to(b, a.shape), axis=-1, equal_var=False)
        assert np.abs(t - want.statistic).max() <= 1e-13 * np.abs(want.statistic).max()
        assert np.abs(dof - want.df).max() <= 1e-13 * want.df.max()
        assert np.abs(p - want.pvalue).max() <= 1e-12
        for i in range(4):
            for k in range(5):
                assert np.allclose(R.welch(a[i, k], b[k]), (t[i, k], dof[i, k], p[i, k]), rtol=1e-12, atol=1e-12)
    same = np.array([0.25, 0.5, 0.75])
    t, dof, p = brainxai.welch_t_test(same, same)                    # equal samples
    assert t == 0.0 and p == 1.0 and abs(dof - 4.0) < 1e-12
    for a, b in (([1.0, 1.0, 1.0], [0.2, 0.4, 0.9]), ([0.2, 0.4, 0.9], [0.5, 0.5, 0.5]), ([0.5], [0.1, 0.2]), ([np.nan, 0.5], [0.1, 0.2])):
        assert all(np.isnan(v) for v in brainxai.welch_t_test(a, b))   # a zero variance, one value, a NaN score
    big = brainxai.welch_t_test([0.9, 0.95, 1.0, 0.92], [0.1, 0.12, 0.08, 0.11])
    want = scipy.stats.ttest_ind([0.9, 0.95, 1.0, 0.92], [0.1, 0.12, 0.08, 0.11], equal_var=False)
    assert abs(big[2] - want.pvalue) <= 1e-12 * want.pvalue + 1e-300 or abs(big[2] / want.pvalue - 1) < 1e-9


def test_incomplete_beta():
    from scipy import special
    for a, b, x in ((0.5, 0.5, 0.3), (2.0, 0.5, 0.9), (7.3, 0.5, 0.01), (50.0, 0.5, 0.999), (1.0, 3.0, 0.5)):
        assert abs(brainxai.regularized_incomplete_beta(a, b, x) - special.betainc(a, b, x)) <= 1e-13


# ---- refusals: raised from host arguments alone, on CPU tensors and a CPU model -------------------------------------------------------
def _mm():
    return brainxai.build_multimodal(5, 512, 4, dropout=0.0).eval()


def _spec_sets(n=4, Q=2, Rn=2, shape=(4, 32, 64)):
    return {f"c{q}": torch.rand(n, *shape) for q in range(Q)}, [torch.rand(n, *shape) for _ in range(Rn)]


def _eeg_sets(n=4, Rn=2):
    return {"alpha": torch.rand(n, 1, 5, 512)}, [torch.rand(n, 1, 5, 512) for _ in range(Rn)]


def test_refusals_need_no_device(monkeypatch):
    model = _mm()
    eeg, spec = torch.rand(3, 1, 5, 512), torch.rand(3, 4, 32, 64)
    con, ran = _spec_sets()
    econ, eran = _eeg_sets()

    def both(match, *, concepts=con, randoms=ran, **kw):
        """The refusal is raised by train_cavs and by tcav alike."""
        with pytest.raises(ValueError, match=match):
            brainxai.train_cavs(model, concepts, randoms, **kw)
        with pytest.raises(ValueError, match=match):
            brainxai.tcav(model, eeg, spec, concepts, randoms, **kw)

    both("unknown target_layer", target_layer="spectrogram_model.block6")
    both("unknown target_layer", target_layer="eeg_model.depthwiseConv", input="eeg", concepts=econ, randoms=eran)
    both("belongs to the EEG branch but input='spec'", target_layer="eeg_model.features")
    both("belongs to the spectrogram branch but input='eeg'", target_layer="block3", input="eeg", concepts=econ, randoms=eran)
    both("input must be", input="both")
    both(r"randoms\[1\] holds 5 examples", randoms=[ran[0], torch.rand(5, 4, 32, 64)])
    both("1 examples per set, supported 2..256", concepts={"a": torch.rand(1, 4, 32, 64)}, randoms=[torch.rand(1, 4, 32, 64)])
    both("257 examples per set, supported 2..256", concepts={"a": torch.rand(257, 4, 32, 64)}, randoms=[torch.rand(257, 4, 32, 64)])
    both("holdout = 0.25 leaves 1 of 2", concepts={"a": torch.rand(2, 4, 32, 64)}, randoms=[torch.rand(2, 4, 32, 64)], holdout=0.25)
    both("holdout must be", holdout=0.5)
    both("unknown classifier 'logistic'", classifier="logistic")
    both("ridge must be", ridge=0.0)
    both("ridge must be", ridge=-1e-2)
    both("randoms must be a list", randoms=[])
    both("concepts must be a non-empty dict", concepts={})
    with pytest.raises(ValueError, match=r"concepts\['c1'\] holds examples shaped \(4, 32, 32\)"):
        brainxai.train_cavs(model, {"c0": con["c0"], "c1": torch.rand(4, 4, 32, 32)}, ran)
    with pytest.raises(ValueError, match=r"holds examples shaped \(4, 16, 64\), the explained input's are \(4, 32, 64\)"):
        brainxai.tcav(model, eeg, spec, *_spec_sets(shape=(4, 16, 64)))
    with pytest.raises(ValueError, match="either cavs="):
        brainxai.tcav(model, eeg, spec)
    fake = X.CavSet(torch.zeros(6, 512), np.array([(0, 0), (0, 1), (1, 0), (1, 1), (-1, 0), (-1, 1)]), ["c0", "c1"], None, None, None, None, None, None,
                    "spectrogram_model.block5", "spec", (1, 2, 256), "ridge", 1e-2, 0.0, 4)
    assert (fake.Q, fake.R) == (2, 2) and fake.vector("c1", 1).shape == (1, 2, 256) and fake.index("c1", 1) == 3
    with pytest.raises(ValueError, match="either cavs="):
        brainxai.tcav(model, eeg, spec, con, ran, cavs=fake)
    with pytest.raises(ValueError, match="cavs must be a CavSet"):
        brainxai.tcav(model, eeg, spec, cavs=(1, 2))
    with pytest.raises(ValueError, match="trained for input='spec' at spectrogram_model.block5 with 512 features"):
        brainxai.tcav(model, eeg, spec, cavs=fake, target_layer="block4")
    with pytest.raises(ValueError, match="with 512 features; this call explains input='spec' at spectrogram_model.block5 with 1024"):
        brainxai.tcav(model, eeg, torch.rand(3, 4, 64, 64), cavs=fake)
    with pytest.raises(ValueError, match="needs a MultimodalModel or a Spectrogram_Model"):
        brainxai.train_cavs(model.eeg_model, con, ran)
    with pytest.raises(ValueError, match="class outside"):
        brainxai.tcav(model, eeg, spec, con, ran, class_idx=6)
    # the stack of activations against the free memory of the device: block1 of 16 examples is 16 * 16 * 32 * 16 fp32 values
    monkeypatch.setattr(X, "_tcav_free_bytes", lambda dev: 1000)
    with pytest.raises(ValueError, match=rf"{16 * 16 * 32 * 16 * 4} bytes; 1000 bytes of device memory are free"):
        brainxai.train_cavs(model, con, ran, target_layer="block1")
    with pytest.raises(ValueError, match=rf"{16 * 16 * 32 * 16 * 4} bytes; 1000 bytes"):
        brainxai.tcav(model, eeg, spec, con, ran, target_layer="block1")
    monkeypatch.undo()
    # with nothing left to refuse, the closing refusal: there is no CPU path
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        brainxai.train_cavs(model, con, ran)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        brainxai.tcav(model, eeg, spec, econ, eran, input="eeg")
    assert not model.training and all(q.requires_grad for q in model.parameters())
