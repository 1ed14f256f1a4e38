"""The four data-side HIP entry points (bx_eeg_stack_iir, bx_eeg_montage_stack, bx_spec_preprocess, bx_spec_regions) away from the
workload's own geometry, against the fp64 references of tests/data_ref.py: the branches written for other sizes -- unaligned tile
staging, the channel index inside the scan, other filter orders and steps, truncation, the smallest legal planes, the largest
anti-aliasing radius, windows shorter than the filter, windows outside the recording.  tests/test_data_ref_cpu.py proves on the CPU
which kernel each stacker case takes.

Bounds are those of the existing tests of the same entry points (tests/test_gpu_parity.py): all four kernels compute in fp64 and round
once to fp32, so 1e-5 (stacker) and 2e-5 (the others) of the largest reference value.  Every comparison prints its deviation; run
with -s to read them, the last test prints the worst per kernel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import ops
from tests import data_ref as D
from tests.golden_util import REPORT, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {"stack_iir": 1e-5, "montage": 2e-5, "spec_preprocess": 2e-5, "spec_regions": 2e-5}
WORST = {}
DBL = C.POINTER(C.c_double)
BX_EWORKSPACE = -4                                   # include/brainxai.h


def _cmp(kernel, label, got, want):
    got = got.detach().cpu()
    want = torch.as_tensor(np.asarray(want))
    assert tuple(got.shape) == tuple(want.shape), f"{kernel} {label}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), f"{kernel} {label}: non-finite output"
    err = rel_err(got, want)
    REPORT.append((f"data/{kernel}/{label}", err, 0.0))
    if err > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (err, label)
    print(f"[data] {kernel} {label}: rel err {err:.3e}")
    assert err <= TOL[kernel], f"{kernel} {label}: rel err {err:.3e} > {TOL[kernel]}"
    return err


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ================================================================================================ A. bx_eeg_stack_iir
def _stacker_of(case):
    return brainxai.EEGStacker(channel_index=case["channels"], cutoff_freq=case["cutoff"], order=case["order"], downsample=case["step"])


def _stacker_input(i, case):
    C_out = case["Craw"] if case["channels"] is None else len(case["channels"])
    plan = D.scan_plan(C_out, case["Craw"], order=case["order"], step=case["step"], cutoff=case["cutoff"])
    wg = plan["R"] * D.SCAN_S if plan["path"] == "scan" else 880
    return C_out, D.eeg_input(1000 + i, case["B"], case["L"], case["Craw"], wg)


@pytest.mark.parametrize("i", range(len(D.STACKER_CASES)), ids=[c["id"] for c in D.STACKER_CASES])
def test_stacker(i):
    """Measured on MI355X: 3.0e-8 ... 5.4e-8 of the largest output for every case (one fp32 rounding of the fp64 result) except
    A7-2Hz-C5, 1.18e-7: the scan's 40-chunk warm-up at a 2 Hz cutoff truncates the filter's memory at 8.5e-12 of the output (the host's
    1e-13 bound is on A^(Kc S), the state it multiplies is larger), enough to round one of the case's 15 000 outputs the other way."""
    case = D.STACKER_CASES[i]
    C_out, raw = _stacker_input(i, case)
    want = D.stack_iir_ref(raw, case["channels"], case["order"], case["cutoff"], step=case["step"])
    got = _stacker_of(case)(_dev(raw))
    assert tuple(got.shape) == (case["B"], 1, C_out, -(-case["L"] // case["step"]))
    _cmp("stack_iir", f"{case['id']} ({case['path']})", got, want)


def test_stacker_scan_and_sequential_agree():
    """A6.  One sample further into a contiguous tensor the rows start L * Craw floats later -- off a 16-byte boundary when that is no
    multiple of 4 -- and the stacker takes the one-thread-per-row kernel; the same values in a tensor of their own take the scan.  Both
    are fp32 roundings of fp64 results that differ by the scan's 1e-13 warm-up truncation and by summation order, so an element
    differs by at most one fp32 step of its own size: the bound is 2 ulp of the row's largest value."""
    L_, Craw = 1003, 19
    base = _dev(D.eeg_input(77, 4, L_, Craw, 880))
    mis = base[1:]
    assert mis.is_contiguous() and base.data_ptr() % 16 == 0 and mis.data_ptr() % 16 != 0
    fresh = mis.clone()
    assert fresh.data_ptr() % 16 == 0
    st = brainxai.EEGStacker()
    seq, scan = st(mis), st(fresh)
    want = D.stack_iir_ref(mis.cpu().numpy())
    _cmp("stack_iir", "A6 misaligned (sequential)", seq, want)
    _cmp("stack_iir", "A6 aligned (scan)", scan, want)
    ulp = np.spacing(np.abs(want).max(axis=-1, keepdims=True).astype(np.float32)).astype(np.float64)
    diff = (seq.cpu().numpy().astype(np.float64) - scan.cpu().numpy().astype(np.float64)) / ulp
    worst = float(np.abs(diff).max())
    WORST["stack_iir scan-vs-sequential (ulp of the row maximum)"] = (worst, "A6")
    print(f"[data] stack_iir A6: scan vs sequential differ by at most {worst:.3f} ulp of the row maximum")
    assert worst <= 2.0


def test_stacker_refusals():
    raw = _dev(D.eeg_input(5, 2, 80, 19))
    with pytest.raises(RuntimeError, match=r"order must be 1\.\.8"):
        brainxai.EEGStacker(order=9)(raw)
    with pytest.raises(RuntimeError, match=r"order must be 1\.\.8"):            # the same requirement covers scale != 0
        brainxai.EEGStacker(scale=0.0)(raw)
    with pytest.raises(RuntimeError, match="channel index exceeds the raw channel count"):
        brainxai.EEGStacker(channel_index=[0, 19])(raw)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        brainxai.EEGStacker()(raw.cpu())
    with pytest.raises(RuntimeError, match=r"expected raw EEG \[B, L, C\]"):
        brainxai.EEGStacker()(raw[0])


# ================================================================================================ B. bx_eeg_montage_stack
_MONT = None


def _montage(raw_np, ra, rb, out_len, claim_short=0):
    """The C entry point as EEGMontageStacker.__call__ drives it, with the column count, rows and length free.
    -> (return code, out [B, 1, R, out_len], status).  ``claim_short``: bytes taken off the workspace size TOLD to the library (the
    buffer itself is always full size, so nothing could be written out of bounds even if the check were missing)."""
    global _MONT
    if _MONT is None:
        _MONT = brainxai.EEGMontageStacker()
    st = _MONT
    raw = _dev(raw_np.astype(np.float32))
    B, Lr, Craw = raw.shape
    R = len(ra)
    assert max(max(ra), max(rb)) < Craw and min(ra) >= 0
    lib = L.load()
    a, b = torch.tensor(ra, dtype=torch.int32, device=DEV), torch.tensor(rb, dtype=torch.int32, device=DEV)
    out = torch.full((B, 1, R, out_len), float("nan"), dtype=torch.float32, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)              # the call has to clear it
    need = lib.bx_eeg_montage_workspace(B, Lr, Craw, R)
    ws = ops.workspace(max(need, 256), raw.device)
    assert ws.numel() >= need
    rc = lib.bx_eeg_montage_stack(ops._p(raw), ops._p(a), ops._p(b), ops._p(out), B, Lr, Craw, R, out_len,
                                  st.b1.ctypes.data_as(DBL), st.a1.ctypes.data_as(DBL), len(st.b1) - 1,
                                  st.b2.ctypes.data_as(DBL), st.a2.ctypes.data_as(DBL), len(st.b2) - 1,
                                  st.eps, ops._p(status), ops._p(ws), need - claim_short, ops._stream())
    return rc, out, status


def _montage_want(frames, ra, rb, out_len):
    return np.stack([D.montage_ref(f, ra, rb, out_len) for f in frames])


def _std_rows():
    rows = brainxai.EEGMontageStacker().rows
    return [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize("out_len", [100, 999, 1000, 1001, 1, 63, 64, 65])
def test_montage_truncation(out_len):
    """L = 4001 keeps K = 1000 columns: shorter outputs truncate, 1001 pads one zero; 63 / 64 / 65 straddle the transpose tile."""
    frames = D.frames_input(11, 2, 4001, 20)
    ra, rb = _std_rows()
    rc, out, status = _montage(frames, ra, rb, out_len)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", f"L4001 out_len {out_len}", out, _montage_want(frames, ra, rb, out_len))


@pytest.mark.parametrize("L_", [5, 8, 9])
def test_montage_smallest_lengths(L_):
    frames = D.frames_input(12 + L_, 2, L_, 20, nan_rate=0.0)
    ra, rb = _std_rows()
    rc, out, status = _montage(frames, ra, rb, 4)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", f"L{L_}", out, _montage_want(frames, ra, rb, 4))


@pytest.mark.parametrize("L_,msg", [(4, "bad sizes"), (6, "L % 4"), (7, "L % 4")])
def test_montage_refused_lengths(L_, msg):
    ra, rb = _std_rows()
    rc, _, _ = _montage(D.frames_input(3, 1, L_, 20, nan_rate=0.0), ra, rb, 4)
    assert rc != 0
    with pytest.raises(RuntimeError, match=msg):
        L.check(rc, "bx_eeg_montage_stack")


@pytest.mark.parametrize("Craw,R,B", [(1, 1, 1), (1, 2, 4), (3, 2, 1), (3, 37, 4), (20, 65, 1), (20, 37, 4), (70, 1, 1), (70, 2, 4), (70, 65, 4)])
def test_montage_widths(Craw, R, B):
    """B * Craw and B * R below, at and across one 64-thread block; rows mix single columns and differences, row 1 is a column minus
    itself (all zero: z-score 0 / (0 + eps) = 0)."""
    frames = D.frames_input(100 * Craw + R + B, B, 401, Craw)
    ra, rb = D.montage_rows_for(Craw, R)
    rc, out, status = _montage(frames, ra, rb, 128)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", f"Craw {Craw} R {R} B {B}", out, _montage_want(frames, ra, rb, 128))
    if R > 1:
        assert float(out[:, 0, 1].abs().max()) == 0.0


def test_montage_nan_placement_and_status():
    ra, rb = _std_rows()
    frames = D.frames_input(21, 2, 801, 20, nan_rate=0.0)
    last = frames.copy(); last[:, -1, :] = np.nan                                          # on the last sample only, every column
    rc, out, status = _montage(last, ra, rb, 256)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", "NaN on the last sample", out, _montage_want(last, ra, rb, 256))
    first = frames.copy(); first[:, 1, :] = np.nan                                         # sample 1 of every column: only t = 0 is kept
    rc, out, status = _montage(first, ra, rb, 256)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", "NaN on sample 1 of every column", out, _montage_want(first, ra, rb, 256))
    # a column that is NaN from t = 0: reported, finite, and -- as include/brainxai.h says -- treated as all-zero after the first
    # filter, which is what the reference computes for a column of zeros; rows that do not touch the column are unaffected
    dead = frames.copy(); dead[0, 0, 5] = np.nan
    rc, out, status = _montage(dead, ra, rb, 256)
    assert rc == 0 and int(status.item()) == 1
    zeroed = frames.copy(); zeroed[0, :, 5] = 0.0
    want = _montage_want(zeroed, ra, rb, 256)
    clean = [r for r in range(len(ra)) if ra[r] != 5 and rb[r] != 5]
    _cmp("montage", "column NaN from t = 0, other rows", out[:, :, clean], want[:, :, clean])
    _cmp("montage", "column NaN from t = 0, all rows", out, want)
    # the next call clears the status
    rc, out, status = _montage(frames, ra, rb, 256)
    assert rc == 0 and int(status.item()) == 0
    _cmp("montage", "after a status-1 call", out, _montage_want(frames, ra, rb, 256))


def test_montage_workspace_one_byte_short():
    ra, rb = _std_rows()
    rc, out, _ = _montage(D.frames_input(3, 1, 401, 20), ra, rb, 128, claim_short=1)
    assert rc == BX_EWORKSPACE
    assert bool(torch.isnan(out).all())                                        # refused on the host: nothing was launched
    with pytest.raises(RuntimeError, match="workspace"):
        L.check(rc, "bx_eeg_montage_stack")


# ================================================================================================ C. bx_spec_preprocess
def _specprep_case(R, W, Ccols, Trows, window, offs, seed):
    """-> (raw [B, Trows, Ccols] float32 with NaNs on the corners of every sample's gathered region, want [B, 3, R, W])."""
    B = len(offs)
    raw = D.spec_input(seed, B, Trows, Ccols)
    jn = min(Trows, W)
    for b, off in enumerate(offs):
        o = 0 if off is None else off // 2
        live = min(R, Ccols if off is None else window, Ccols - o)             # rows of the plane that come from the recording
        if live <= 0:
            continue
        for i in {0, live - 1}:
            for j in {0, jn - 1}:
                raw[b, j, o + i] = np.nan
    want = np.stack([D.specprep_ref(raw[b].astype(np.float64), offs[b], (R, W), window) for b in range(B)])
    return raw, want


def _specprep_run(R, W, window, raw, offs, label, want):
    pre = brainxai.SpectrogramPreprocessor(image_size=(R, W), window=window)
    got = pre(_dev(raw), None if offs[0] is None else offs)
    assert int(pre.last_status.item()) == 0, label
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2]), label
    _cmp("spec_preprocess", label, got, want)
    return got


def _specprep_geometries(R, W):
    k = 0
    for Ccols in (7, 40, 400):
        for Trows in (3, W, W + 9):
            window = (R, max(1, R - 3), R + 5)[k % 3]
            k += 1
            yield Ccols, Trows, window


@pytest.mark.parametrize("R,W", [(11, 5), (12, 8), (37, 53), (400, 300)])
def test_specprep_sizes_and_offsets(R, W):
    """The smallest legal plane (R = 11 > filtfilt's 9 + 1, W = 5 > the gaussian's radius), odd sizes and the workload's own, each
    over narrow / wide recordings and short / exact / long ones; per geometry one batch of three offsets (0; a window that ends
    exactly at the last column, or at the second-to-last on an odd offset; a window that starts at the last column) and one
    sample without offsets."""
    for n, (Ccols, Trows, window) in enumerate(_specprep_geometries(R, W)):
        end = max(Ccols - window, 0)
        offs = [0, 2 * end + (n & 1), 2 * (Ccols - 1)]
        seed = 7 * R + 3 * W + n
        raw, want = _specprep_case(R, W, Ccols, Trows, window, offs, seed)
        _specprep_run(R, W, window, raw, offs, f"{R}x{W} Ccols {Ccols} Trows {Trows} window {window} offsets {offs}", want)
        raw, want = _specprep_case(R, W, Ccols, Trows, window, [None], seed + 1)
        _specprep_run(R, W, window, raw, [None], f"{R}x{W} Ccols {Ccols} Trows {Trows} no offsets", want)


@pytest.mark.parametrize("R,W", [(11, 5), (37, 53)])
def test_specprep_window_beyond_the_recording(R, W):
    """A window that starts past the last column is all padding: a constant plane, 0 after the min-max, status 0 -- next to a
    sample with an ordinary window in the same call."""
    Ccols, Trows, offs = 40, W + 9, [2 * 40, 6, 2 * 40 + 7]
    raw, want = _specprep_case(R, W, Ccols, Trows, R, offs, 90 + R)
    assert not want[0].any() and not want[2].any() and want[1].any()
    got = _specprep_run(R, W, R, raw, offs, f"{R}x{W} windows beyond the recording", want)
    assert float(got[0].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


def test_specprep_all_nan_row_and_refusals():
    R, W = 12, 8
    raw = D.spec_input(4, 2, W + 9, 40)
    raw[1, :, 3] = np.nan                                                      # column 3 -> row 3 of the plane, NaN over all W columns
    pre = brainxai.SpectrogramPreprocessor(image_size=(R, W), window=R)
    got = pre(_dev(raw), [0, 0])
    assert int(pre.last_status.item()) & 1 and bool(torch.isfinite(got).all())
    _cmp("spec_preprocess", "sample next to an all-NaN row", got[:1], D.specprep_ref(raw[0].astype(np.float64), 0, (R, W), R)[None])
    pre(_dev(raw[:1]), [0])
    assert int(pre.last_status.item()) == 0                                    # cleared by the next call
    with pytest.raises(ValueError, match="9-tap"):
        brainxai.SpectrogramPreprocessor(sigma=2.0)
    with pytest.raises(RuntimeError, match="R must exceed"):
        brainxai.SpectrogramPreprocessor(image_size=(10, 8))(_dev(raw))
    with pytest.raises(RuntimeError, match="bad sizes"):
        brainxai.SpectrogramPreprocessor(image_size=(12, 4))(_dev(raw))


# ================================================================================================ D. bx_spec_regions
def _regions_run(label, raw, offs, out_hw, window, regions):
    B = raw.shape[0]
    want = np.stack([D.regions_ref(raw[b].astype(np.float64), None if offs is None else offs[b], out_hw, window, regions) for b in range(B)])
    got = brainxai.SpectrogramRegionStacker(out_hw=out_hw, window=window, regions=regions)(_dev(raw), offs)
    _cmp("spec_regions", label, got, want)
    return got, want


# id, bins, regions, Trows, window, out_hw, offsets
REGION_CASES = [
    ("radius 7 x 8 (the limit)", 90, 2, 120, 95, (20, 20), [0, 20, 60]),
    ("radius 8 at window 104", 10, 1, 110, 104, (10, 20), [0, 5, 12]),
    ("radius 8 beyond a 5-sample window", 6, 2, 20, 5, (6, 1), [0, 8, 34]),
    ("radius 4 beyond 3 bins", 3, 2, 20, 12, (1, 12), [0, 8, 20]),
    ("both radii beyond the data", 3, 1, 9, 5, (1, 1), [0, 3, 10]),
    ("one bin, one time sample", 1, 3, 6, 1, (1, 1), [0, 4, 10]),
    ("one bin, one time sample, enlarged", 1, 2, 6, 1, (3, 4), [0, 4, 10]),
    ("up-scaling on both axes", 10, 2, 30, 12, (33, 50), [0, 10, 40]),
    ("identity", 10, 2, 30, 12, (10, 12), [0, 10, 40]),
    ("tile 1x1", 4, 2, 12, 5, (1, 1), [0, 4, 16]),
    ("tile 15x17", 20, 2, 60, 40, (15, 17), [0, 10, 50]),
    ("tile 16x16", 20, 2, 60, 40, (16, 16), [0, 10, 50]),
    ("tile 17x33", 20, 2, 60, 40, (17, 33), [0, 10, 50]),
    ("1 region", 7, 1, 30, 16, (5, 9), [0, 6, 40]),
    ("2 regions", 7, 2, 30, 16, (5, 9), [0, 6, 40]),
    ("3 regions", 7, 3, 30, 16, (5, 9), [0, 6, 40]),
    ("window 1", 6, 2, 20, 1, (4, 1), [0, 7, 38]),
    ("window 3", 6, 2, 20, 3, (4, 2), [0, 7, 36]),
    ("window 7", 6, 2, 20, 7, (4, 4), [0, 7, 30]),
    ("window 8", 6, 2, 20, 8, (4, 4), [0, 7, 30]),
    ("window 9", 6, 2, 20, 9, (4, 5), [0, 7, 30]),
    ("windows half and wholly outside", 8, 2, 20, 16, (6, 10), [24, 40, 51]),
]


@pytest.mark.parametrize("i", range(len(REGION_CASES)), ids=[c[0].replace(" ", "-") for c in REGION_CASES])
def test_regions(i):
    label, bins, regions, Trows, window, out_hw, offs = REGION_CASES[i]
    raw = D.spec_input(300 + i, len(offs), Trows, regions * bins, nan_rate=5e-3)
    got, want = _regions_run(label, raw, offs, out_hw, window, regions)
    assert tuple(got.shape) == (len(offs), regions, out_hw[0], out_hw[1])
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    for b, off in enumerate(offs):
        if off // 2 >= Trows:                                                  # all padding: 0 and finite
            assert float(got[b].abs().max()) == 0.0
    none, _ = _regions_run(label + ", no offsets", raw[:1], None, out_hw, window, regions)
    assert tuple(none.shape) == (1, regions, out_hw[0], out_hw[1])


def test_regions_all_nan_window():
    """A window without one finite value.  The reference's normalize_signal takes nanmean of an empty set: NaN, and its output is NaN
    everywhere.  The kernel's convention (include/brainxai.h) is the fill value handle_nan uses for an all-NaN row, 0: the plane is
    constant and the output 0, which is what regions_ref returns.  With zero padding in the window the finite values are the
    zeros, the reference has a value (0 everywhere as well) and both agree without a convention."""
    raw = D.spec_input(41, 3, 30, 16)
    raw[1, :16] = np.nan                                                       # sample 1: offset 0, window 16 -> all NaN
    raw[2, 20:] = np.nan                                                       # sample 2: offset 40 -> rows 20..29 NaN + 6 rows of padding
    got, want = _regions_run("all-NaN windows", raw, [0, 0, 40], (6, 10), 16, 2)
    assert want[0].any() and not want[1].any() and not want[2].any()
    assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


def test_regions_refusals():
    raw = _dev(D.spec_input(42, 1, 120, 10))
    with pytest.raises(RuntimeError, match="anti-aliasing radius"):
        brainxai.SpectrogramRegionStacker(out_hw=(10, 20), window=105, regions=1)(raw)          # the first window with radius 9
    with pytest.raises(RuntimeError, match="bins"):
        brainxai.SpectrogramRegionStacker(out_hw=(4, 4), window=8, regions=3)(raw)              # 10 % 3 != 0
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        brainxai.SpectrogramRegionStacker(out_hw=(4, 4), window=8, regions=1)(raw.cpu())


# ================================================================================================
def test_zz_worst_deviations():
    """Prints what the comparisons above measured (they ran first: pytest keeps file order)."""
    for kernel, (err, label) in sorted(WORST.items()):
        print(f"[data] worst {kernel}: {err:.3e} ({label})")
    assert all(math.isfinite(err) for err, _ in WORST.values())
