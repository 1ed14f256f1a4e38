"""tests/data_ref.py pinned on the CPU: each parameterised reference equals, at its defaults, the oracle function it restates (which
the golden fixtures pin), and the host logic of the chunked-scan stacker restated there sends every case of
tests/test_gpu_data_kernels.py down the path that case was written for.  No GPU, no library."""
import warnings

import numpy as np
import pytest

from oracle import ref_torch as O
from tests import data_ref as D


# ------------------------------------------------------------------------------------------------ references == oracle at the defaults
def test_stack_iir_ref_is_the_oracle():
    """Same calls in the same order (clip, nan_to_num, / 32 in float32; lfilter in fp64; [::5]); the oracle rounds to float32 last."""
    raw = O.synthetic_batch(batch=2, seed=61, stacked=False)["raw_eeg"].numpy()
    want = O.stack_eeg_batch(raw).numpy()
    got = D.stack_iir_ref(raw)
    assert got.dtype == np.float64 and got.shape == want.shape == (2, 1, 19, 2000)
    assert np.array_equal(got.astype(np.float32), want)
    sel = D.stack_iir_ref(raw, channels=[3, 0, 18])
    assert np.array_equal(sel, got[:, :, [3, 0, 18]])


def test_montage_ref_is_the_oracle():
    """Same operations per row: lfilter and the z-score work row by row, so building the 37 selected rows directly instead of
    filtering 38 and selecting afterwards changes no value; np.roll along the row equals the oracle's roll over the flattened array
    on the kept columns because L % 4 is 0 or 1."""
    frames = O.synthetic_frames(batch=2, seed=7)
    rows = O.montage_rows()
    ra, rb = [r[0] for r in rows], [r[1] for r in rows]
    for f in frames:
        assert np.array_equal(D.montage_ref(f, ra, rb, 3000), O.montage_transform(f))
    f = O.synthetic_frames(batch=1, length=4001, seed=9, nan_rate=5e-4)[0]
    assert np.array_equal(D.montage_ref(f, ra, rb, 3000), O.montage_transform(f))
    assert np.array_equal(D.montage_ref(f, ra, rb, 640), O.montage_transform(f, fixed_length=640))
    bad = f.copy(); bad[0, 5] = np.nan
    with pytest.raises(ValueError, match="NaN from t = 0"):
        D.montage_ref(bad, ra, rb, 3000)


def test_specprep_ref_is_the_oracle():
    frames = O.synthetic_spectrogram_frames(batch=2, seed=5)
    assert np.array_equal(D.specprep_ref(frames[0], None), O.spectrogram_transform(frames[0], None))
    assert np.array_equal(D.specprep_ref(frames[1], 60), O.spectrogram_transform(frames[1], 60))
    f64 = frames[1].astype(np.float64)
    assert np.array_equal(D.specprep_ref(f64, 700), O.spectrogram_transform(f64, 700))
    # the window really is an argument: 200 columns leave rows 200.. of the plane zero before the filters
    assert not np.array_equal(D.specprep_ref(f64, 60, window=200), D.specprep_ref(f64, 60))


def test_regions_ref_is_the_oracle():
    frames = O.synthetic_spectrogram_frames(batch=2, seed=5)
    assert np.array_equal(D.regions_ref(frames[0], None), O.spectrogram_regions_transform(frames[0], None))
    assert np.array_equal(D.regions_ref(frames[1], 60, (32, 100)), O.spectrogram_regions_transform(frames[1], 60, (32, 100)))
    assert np.array_equal(D.regions_ref(frames[1][:, :200], 20, (16, 16), 40, 2), O.spectrogram_regions_transform(frames[1][:, :200], 20, (16, 16), 40, 2))
    # a window wholly outside the recording: all padding, 0 everywhere (the oracle agrees, through an empty slice)
    out = D.regions_ref(frames[0], 2 * 320 + 6, (8, 8))
    assert out.shape == (4, 8, 8) and not out.any()
    assert np.array_equal(out, O.spectrogram_regions_transform(frames[0], 2 * 320 + 6, (8, 8)))
    # a window without a finite value: the oracle's nanmean of an empty set makes everything NaN; the convention here is 0
    nan = np.full((40, 8), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.isnan(O.spectrogram_regions_transform(nan, 0, (4, 4), 40, 2)).all()
    out = D.regions_ref(nan, 0, (4, 4), 40, 2)
    assert out.shape == (2, 4, 4) and not out.any()
    # NaN rows above zero padding: the padding is finite, the oracle has a value and the wrapper passes it through
    out = D.regions_ref(nan, 40, (4, 4), 40, 2)
    assert np.isfinite(out).all() and not out.any()


# ------------------------------------------------------------------------------------------------ the scan's host logic
def _lds(G, Craw, C):
    return 4 * (((G * 40 * Craw + 7) // 4) * 4 + 4) + G * C * 4 * 8


@pytest.mark.parametrize("C,Craw,G,R,lds,path", [
    (19, 19, 26, 22, 94880, "scan"), (19, 20, 26, 22, 99040, "scan"), (5, 5, 102, 98, None, "scan"), (37, 37, 13, 9, None, "scan"),
    (64, 64, 8, 4, None, "scan"), (1, 1, 512, 508, 98336, "scan"), (3, 19, 170, 166, 533152, "sequential"),
    (19, 64, 26, 22, None, "sequential"), (8, 5, 64, 60, None, "scan"),
    # G = 5 and Kc = 4: the warm-up test `Kc >= G - 1` is only made while the power is still above 1e-13, and A^(4 S) is already
    # below it, so the scan runs with ONE chunk of output per workgroup
    (100, 100, 5, 1, None, "scan")])
def test_scan_geometry(C, Craw, G, R, lds, path):
    p = D.scan_plan(C, Craw)
    assert (p["path"], p["G"], p["Kc"], p["R"]) == (path, G, 4, R), p
    assert p["lds"] == _lds(G, Craw, C) and (lds is None or p["lds"] == lds)
    assert (p["lds"] <= 160 * 1024) == (path == "scan")


@pytest.mark.parametrize("cutoff,C,Kc,pole,path,R", [(20.0, 19, 4, 0.795, "scan", 22), (10.0, 19, 8, 0.888, "scan", 18),
                                                     (2.0, 19, None, 0.976, "sequential", None), (2.0, 5, 40, 0.976, "scan", 62)])
def test_scan_warmup(cutoff, C, Kc, pole, path, R):
    p = D.scan_plan(C, C, cutoff=cutoff)
    assert p["path"] == path and p["R"] == R, p
    assert abs(D.pole_modulus(cutoff=cutoff) - pole) < 5e-4
    if Kc is not None:
        assert p["Kc"] == Kc
    else:
        assert "warm-up" in p["why"] and p["Kc"] >= p["G"] - 1


def test_scan_only_order4_step5_and_aligned():
    assert D.scan_plan(19, 19, order=3)["path"] == "sequential" and D.scan_plan(19, 19, step=4)["path"] == "sequential"
    assert D.scan_plan(19, 19, aligned=False)["path"] == "sequential" and D.scan_plan(513, 513)["path"] == "sequential"
    # the benchmark's own geometry never leaves the aligned path: that is why the cases below exist
    assert D.scan_shifts(64, 10000, 19, D.scan_plan(19, 19)) == {0} and not D.scan_ragged_end(10000, 19)


@pytest.mark.parametrize("case", D.STACKER_CASES, ids=[c["id"] for c in D.STACKER_CASES])
def test_stacker_case_takes_its_path(case):
    C = case["Craw"] if case["channels"] is None else len(case["channels"])
    p = D.scan_plan(C, case["Craw"], order=case["order"], step=case["step"], cutoff=case["cutoff"])
    assert p["path"] == case["path"], p
    if case["shifts"] is not None:
        assert D.scan_shifts(case["B"], case["L"], case["Craw"], p) == case["shifts"]
    if case["ragged"] is not None:
        assert D.scan_ragged_end(case["L"], case["Craw"]) == case["ragged"]
    if case["channels"] is not None:
        assert max(case["channels"]) < case["Craw"]


def test_stacker_cases_cover_what_they_claim():
    by = {c["id"]: c for c in D.STACKER_CASES}
    assert len(by) == len(D.STACKER_CASES)
    a1 = set().union(*(c["shifts"] for c in D.STACKER_CASES if c["id"].startswith("A1")))
    assert a1 == {0, 1, 2, 3}
    p19 = D.scan_plan(19, 19)
    nwg = lambda L: -(-L // (p19["R"] * 40))                           # 880 samples per workgroup
    assert [nwg(L) for L in (1721, 1722, 1723, 1761, 203, 37)] == [2, 2, 2, 3, 1, 1] and 37 < 40
    scan_idx = [c for c in D.STACKER_CASES if c["path"] == "scan" and c["channels"] is not None]
    assert any(len(c["channels"]) > c["Craw"] for c in scan_idx) and any(len(set(c["channels"])) < len(c["channels"]) for c in scan_idx)
    widths = {c["Craw"] for c in D.STACKER_CASES if c["id"].startswith("A3")}
    assert widths >= {1, 5, 37, 64}
    for c in (c for c in D.STACKER_CASES if c["id"].startswith("A3")):
        p = D.scan_plan(c["Craw"], c["Craw"])
        assert c["L"] == 4 * p["R"] * 40 + 13 and p["lds"] > 64 * 1024
    kcs = {D.scan_plan(len(c["channels"]) if c["channels"] else c["Craw"], c["Craw"], cutoff=c["cutoff"])["Kc"] for c in D.STACKER_CASES if c["path"] == "scan"}
    assert kcs == {4, 8, 40}
    seq = [(c["order"], c["step"]) for c in D.STACKER_CASES if c["path"] == "sequential"]
    assert {o for o, s in seq if s == 5} >= {1, 2, 3, 5, 6, 7, 8} and {s for o, s in seq} >= {1, 2, 4, 5, 7}
    assert (4, 5) in seq                                               # order 4, step 5 reaches the sequential kernel through a fallback
    # A6: one sample further into a contiguous tensor is L * Craw floats further: off a 16-byte boundary
    assert (1003 * 19) % 4 != 0


def test_inputs_hit_the_boundaries():
    p = D.scan_plan(19, 19)
    wg = p["R"] * 40
    x = D.eeg_input(3, 2, 1723, 19, wg)
    assert x.dtype == np.float32 and 5e-4 < np.isnan(x).mean() < 0.2 and (np.abs(np.nan_to_num(x)) > 1024).any()
    assert np.isnan(x[:, 0]).any() and (x[:, 0] > 1024).any() and np.isnan(x[:, -1]).any() and (x[:, -1] < -1024).any()
    for n in range(40, 1723, 40):
        pair = x[:, n - 1:n + 1]
        assert np.isnan(pair[:, 0]).any() or np.isnan(pair[:, 1]).any()
        assert (np.abs(np.nan_to_num(pair)) > 1024).any()
    for n in range(wg, 1723, wg):
        assert (x[:, n - 1] == 4000.0).all() and np.isnan(x[:, n]).all()
    f = D.frames_input(1, 2, 401, 3)
    assert not np.isnan(f[:, 0]).any() and np.isnan(f).any()
    ra, rb = D.montage_rows_for(3, 37)
    assert max(ra + rb) < 3 and ra[1] == rb[1] and -1 in rb and any(b >= 0 and a != b for a, b in zip(ra, rb))


def test_region_radii():
    """The anti-aliasing radii the GPU cases name, from the same formula the wrapper uses (int(4 sigma + 0.5), sigma = (f - 1) / 2)."""
    def radius(n_in, n_out):
        return (len(O.resize_gaussian_weights(n_in, n_out)) - 1) // 2
    assert radius(90, 20) == 7 and radius(95, 20) == 8 and radius(100, 20) == 8 and radius(102, 20) == 8 and radius(104, 20) == 8
    assert radius(105, 20) == 9                                        # the first window that 20 columns cannot take
    assert radius(5, 1) == 8 and radius(3, 1) == 4 and radius(10, 33) == 0 and radius(1, 1) == 0
