"""The four data-side chains (EEG stacker, montage stacker, spectrogram pre-processing, spectrogram region planes) restated with
numpy and scipy in fp64, with every size the HIP entry points accept turned into an argument -- what bx_eeg_stack_iir,
bx_eeg_montage_stack, bx_spec_preprocess and bx_spec_regions are tested against away from the workload's own geometry.  Nothing here
imports the package under test.  At the default arguments each function equals the oracle function it restates
(tests/test_data_ref_cpu.py), and those are pinned by the golden fixtures.

scan_plan() restates the HOST side of the chunked-scan stacker (launch_stack_scan in csrc/attrib.hip): which of the two kernels a
geometry takes, and how far its staged tiles start off a 16-byte boundary.  The GPU cases are chosen by path, so the CPU suite pins
the prediction for each of them."""
import numpy as np

from oracle import ref_torch as O


# ------------------------------------------------------------------------------------------------ EEG stacker
def stack_iir_ref(raw, channels=None, order=4, cutoff=20.0, fs=200.0, step=5, clip=1024.0, scale=32.0):
    """raw [B, L, Craw] -> fp64 [B, 1, C, ceil(L / step)].  select -> clip -> NaN -> 0 -> / scale in float32 (as the reference
    dataset does it on its float32 frames), scipy.signal.lfilter(butter(order)) along time in fp64, every step-th sample."""
    from scipy.signal import butter, lfilter
    x = np.asarray(raw, dtype=np.float32)
    if channels is not None:
        x = x[:, :, list(channels)]
    y = np.nan_to_num(np.clip(x, np.float32(-clip), np.float32(clip)), nan=0) / np.float32(scale)
    assert y.dtype == np.float32
    b, a = butter(order, cutoff / (0.5 * fs), btype="low", analog=False)
    y = lfilter(b, a, y.astype(np.float64), axis=1)
    return np.ascontiguousarray(y[:, ::step, :].transpose(0, 2, 1))[:, None]


# ------------------------------------------------------------------------------------------------ montage stacker
def montage_ref(frame, row_a, row_b, out_len, low=0.5, high=20.0, fs=200.0, eps=1e-6):
    """oracle.ref_torch.montage_transform with the raw column count (frame [L, Craw]), the output rows (row r = column row_a[r],
    minus column row_b[r] when row_b[r] >= 0) and the output length passed in.  float32 [1, R, out_len].
    A column that is NaN from its first sample is refused: the reference drops it and mis-indexes the rest."""
    from scipy.signal import lfilter
    (b5, a5), (b6, a6) = O.montage_coeffs(low, high, fs)
    L = frame.shape[0]
    assert L % 4 in (0, 1), "the reference's np.roll over the flattened array crosses rows for other lengths"
    waves = lfilter(b5, a5, frame.T, axis=1)
    if np.isnan(waves).all(axis=1).any():
        raise ValueError("a column is NaN from t = 0")
    data = waves.copy()
    where_nan = np.isnan(data)
    mean_values = np.nanmean(data, axis=1, keepdims=True) if where_nan.any() else np.zeros((data.shape[0], 1))
    mean_values[np.isnan(mean_values)] = 0
    data[where_nan] = np.take(mean_values, np.where(where_nan)[0])
    rows = np.zeros((len(row_a), data.shape[1]))
    for r, (a, b) in enumerate(zip(row_a, row_b)):
        rows[r] = data[a] - data[b] if b >= 0 else data[a]
    y = lfilter(b6, a6, rows, axis=1)
    y = (y + np.roll(y, -1, axis=1) + np.roll(y, -2, axis=1) + np.roll(y, -3, axis=1)) / 4
    y = y[:, 0:-1:4]
    y = (y - np.mean(y, axis=1, keepdims=True)) / (np.std(y, axis=1, keepdims=True) + eps)
    if y.shape[1] < out_len:
        y = np.hstack((y, np.zeros((y.shape[0], out_len - y.shape[1]))))
    else:
        y = y[:, :out_len]
    return y[np.newaxis].astype(np.float32)


# ------------------------------------------------------------------------------------------------ spectrogram pre-processing
def specprep_ref(raw, offset=None, image_size=(400, 300), window=300):
    """oracle.ref_torch.spectrogram_transform with the 300-column window as an argument.  raw [Trows, Ccols]; float32
    [3, rows, cols].  A row that is entirely NaN is refused, as there."""
    from scipy.ndimage import gaussian_filter
    from scipy.signal import filtfilt
    x = np.asarray(raw, dtype=np.float64) if raw.dtype != np.float32 else raw
    if offset is not None:
        o = offset // 2
        basic = x[:, o:o + window]
        basic = np.pad(basic, ((0, 0), (0, max(0, window - basic.shape[1]))), mode="constant")
    else:
        basic = x
    s = basic.T
    rows, cols = image_size
    s = np.vstack((s, np.zeros((rows - s.shape[0], s.shape[1])))) if s.shape[0] < rows else s[:rows, :]
    s = np.hstack((s, np.zeros((s.shape[0], cols - s.shape[1])))) if s.shape[1] < cols else s[:, :cols]
    s = s[~np.isnan(s).all(axis=1)]
    if s.shape[0] != rows:
        raise ValueError("a row is entirely NaN")
    where_nan = np.isnan(s)
    if where_nan.any():
        mv = np.nanmean(s, axis=1, keepdims=True)
        mv[np.isnan(mv)] = 0
        s = s.copy()
        s[where_nan] = np.take(mv, np.where(where_nan)[0])
    s = s - np.mean(s, axis=0)
    b, a, _ = O.notch_coeffs()
    s = filtfilt(b, a, s, axis=0)
    s = gaussian_filter(s, sigma=1.0)
    s = np.nan_to_num(s, nan=np.nanmean(s))
    s = (s - np.min(s)) / (np.max(s) - np.min(s) + 1e-6)
    return np.tile(s[..., None], (1, 1, 3)).astype(np.float32).transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------------ spectrogram region planes
def regions_ref(raw, offset=None, out_hw=(128, 256), window=300, regions=4):
    """oracle.ref_torch.spectrogram_regions_transform, plus the two windows it has no value for.  raw [Trows, regions * bins];
    float32 [regions, out_h, out_w].
      * a window wholly outside the recording is all zero padding: a constant plane, 0 after the min-max;
      * a window without one finite value: normalize_signal's nanmean of an empty set is NaN and the reference's output is NaN
        everywhere.  The convention here (and in the kernel, see include/brainxai.h) is the one the reference's own handle_nan
        uses for an all-NaN row: the fill value is 0, so the plane is constant and the output 0."""
    raw = np.asarray(raw, dtype=np.float64)
    o = 0 if offset is None else int(offset) // 2
    win = raw[o:o + window]
    if win.shape[0] == 0 or (win.shape[0] == window and np.isnan(win).all()):
        return np.zeros((regions, int(out_hw[0]), int(out_hw[1])), dtype=np.float32)
    return O.spectrogram_regions_transform(raw, offset, out_hw, window, regions)


# ------------------------------------------------------------------------------------------------ host logic of the chunked scan
SCAN_S = 40                      # samples per chunk: step 5 x 8 kept outputs
SCAN_LDS_LIMIT = 160 * 1024


def scan_plan(C, Craw, order=4, step=5, cutoff=20.0, fs=200.0, aligned=True):
    """-> dict(path='scan'|'sequential', G, Kc, R, lds, why): launch_stack_scan's decisions for C output rows out of Craw raw columns.
    G chunks per workgroup, Kc warm-up chunks (smallest with max|A^(Kc S)| < 1e-13), R = G - Kc chunks of output per workgroup."""
    from scipy.signal import butter
    plan = dict(path="sequential", G=None, Kc=None, R=None, lds=None, why="")
    if order != 4 or step != 5:
        plan["why"] = "only order 4, step 5 is instantiated"
        return plan
    if C > 512 or not aligned:
        plan["why"] = "C > 512 or raw not 16-byte aligned"
        return plan
    b, a = butter(order, cutoff / (0.5 * fs), btype="low", analog=False)
    a = a / a[0]
    A = np.zeros((order, order))
    A[:, 0] = -a[1:]
    A[np.arange(order - 1), np.arange(1, order)] += 1.0
    AS = np.linalg.matrix_power(A, SCAN_S)
    G = 512 // C
    plan["G"] = G
    M, Kc = AS.copy(), 1
    while True:
        mx = np.abs(M).max()
        if mx < 1e-13:
            break
        if not mx < 1e6 or Kc >= G - 1:
            plan["Kc"], plan["why"] = Kc, "warm-up does not fit (Kc >= G - 1)"
            return plan
        M = M @ AS
        Kc += 1
    tile_f = (G * SCAN_S * Craw + 4 + 3) // 4 * 4 + 4
    lds = 4 * tile_f + G * C * order * 8
    plan.update(Kc=Kc, R=G - Kc, lds=lds)
    if lds > SCAN_LDS_LIMIT or C * (G - Kc) * 8 > tile_f:
        plan["why"] = "LDS"
        return plan
    plan["path"] = "scan"
    return plan


def scan_shifts(B, L, Craw, plan):
    """The set of `shift` values (float offset of a staged tile from a 16-byte boundary) over all samples and workgroups."""
    R, Kc = plan["R"], plan["Kc"]
    nwg = -(-L // (R * SCAN_S))
    return {((b * L + (w * R - Kc) * SCAN_S) * Craw) % 4 for b in range(B) for w in range(nwg)}


def scan_ragged_end(L, Craw):
    """True when a sample's last valid float ends off a 16-byte boundary for some sample (L * Craw not a multiple of 4)."""
    return (L * Craw) % 4 != 0


def pole_modulus(order=4, cutoff=20.0, fs=200.0):
    from scipy.signal import butter
    b, a = butter(order, cutoff / (0.5 * fs), btype="low", analog=False)
    return float(np.abs(np.roots(a)).max())


# ------------------------------------------------------------------------------------------------ seeded inputs
def eeg_input(seed, B, L, Craw, wg_samples=None, scale=100.0):
    """Raw EEG [B, L, Craw] float32: microvolt-scale noise, about 0.1 % NaNs, about 0.1 % samples far beyond the clip, and NaN /
    saturating values placed on both sides of every 40-sample chunk boundary (n = 40k - 1, 40k), of every workgroup boundary
    (n = wg_samples * w), and on the first and last sample (alternating over the columns)."""
    g = np.random.default_rng(seed)
    x = (scale * g.standard_normal((B, L, Craw))).astype(np.float32)
    u = g.random(x.shape)
    x[u < 1e-3] = np.nan
    x[u > 1.0 - 1e-3] *= 50.0
    for k in range(1, -(-L // SCAN_S)):
        n, c = SCAN_S * k, k % Craw
        x[:, n - 1, c], x[:, n, c] = np.nan, 5000.0
        c = (k + 1) % Craw
        if n + 1 < L:
            x[:, n - 1, c], x[:, n, c] = -5000.0, np.nan
    if wg_samples:
        for n in range(wg_samples, L, wg_samples):
            x[:, n - 1, :] = 4000.0
            x[:, n, :] = np.nan
    # last, so that nothing above hides them: the first and the last float of a sample (column 0 at t = 0, column Craw - 1 at
    # t = L - 1) are among those a tile that starts or ends off a 16-byte boundary stages separately, and they saturate
    cols = np.arange(Craw)
    x[:, L - 1, cols % 2 == (Craw - 1) % 2] = -5000.0
    x[:, L - 1, cols % 2 != (Craw - 1) % 2] = np.nan
    x[:, 0, cols % 2 == 0] = 5000.0
    x[:, 0, cols % 2 == 1] = np.nan
    return x


def frames_input(seed, B, L, Craw, nan_rate=1e-3):
    """Raw frames [B, L, Craw] float32 like oracle.ref_torch.synthetic_frames (drift + 10 Hz rhythm + noise) at any column count; the
    NaNs never sit at t = 0, so no column is NaN from the start."""
    g = np.random.default_rng(seed)
    t = np.arange(L)[None, :, None] / 200.0
    x = 40 * g.standard_normal((B, L, Craw)) + 60 * np.sin(2 * np.pi * 10 * t + g.uniform(0, 6, (B, 1, Craw))) + 200 * g.standard_normal((B, 1, Craw))
    x = x.astype(np.float32)
    m = g.random((B, L, Craw)) < nan_rate
    m[:, :1] = False
    x[m] = np.nan
    return x


def spec_input(seed, B, Trows, C, nan_rate=2e-3):
    """Parquet-like spectrogram values [B, Trows, C] float32: positive, heavy-tailed, a few NaNs."""
    g = np.random.default_rng(seed)
    x = np.exp(g.standard_normal((B, Trows, C)) * 1.5 + np.linspace(2, -2, C)[None, None, :]).astype(np.float32)
    x[g.random(x.shape) < nan_rate] = np.nan
    return x


def montage_rows_for(Craw, R):
    """(row_a, row_b) for R output rows over Craw columns: single columns mixed with differences; row 1 (when there is one) is a
    column minus itself -- an all-zero row, whose z-score is 0 / (0 + eps)."""
    ra = [r % Craw for r in range(R)]
    rb = [-1 if r % 3 == 0 else (r % Craw + 1 + r // 3) % Craw for r in range(R)]
    if R > 1:
        rb[1] = ra[1]
    return ra, rb


# ------------------------------------------------------------------------------------------------ the stacker's GPU cases
def _case(id, L, Craw=19, B=3, channels=None, order=4, step=5, cutoff=20.0, path="scan", shifts=None, ragged=None):
    return dict(id=id, B=B, L=L, Craw=Craw, channels=channels, order=order, step=step, cutoff=cutoff, path=path, shifts=shifts, ragged=ragged)


REPEATED_INDEX = [18, 0, 0, 7, 19, 3, 11, 5, 2, 16, 9, 1, 14, 6, 12, 4, 17, 8, 13]       # 19 of 20 columns, column 0 twice

# `path` is what the host logic must choose and `shifts` the tile offsets it must produce (tests/test_data_ref_cpu.py asserts both
# against scan_plan / scan_shifts); tests/test_gpu_data_kernels.py runs every case against stack_iir_ref.
STACKER_CASES = (
    # A1: tiles that start and end off a 16-byte boundary
    [_case("A1-L1721", 1721, shifts={0, 2, 3}, ragged=True), _case("A1-L1722", 1722, shifts={0, 2}, ragged=True),
     _case("A1-L1723", 1723, shifts={0, 1, 2}, ragged=True), _case("A1-L203", 203, shifts={0, 1, 2}, ragged=True),
     _case("A1-L37", 37, shifts={0, 2, 3}, ragged=True),
     _case("A1-L1761", 1761, shifts={0, 2, 3}, ragged=True)]        # 2 x 880 + 1: a third workgroup with one sample
    # A2: the scan with a channel index
    + [_case(f"A2-19of20-L{L}", L, Craw=20, channels=list(range(19)), shifts={0}) for L in (10000, 1003)]
    + [_case(f"A2-repeat-L{L}", L, Craw=20, channels=REPEATED_INDEX, shifts={0}) for L in (10000, 1003)]
    + [_case("A2-8of5-L10000", 10000, Craw=5, channels=[4, 0, 0, 3, 1, 2, 4, 1], shifts={0}),
       _case("A2-8of5-L1003", 1003, Craw=5, channels=[4, 0, 0, 3, 1, 2, 4, 1], shifts={0, 2, 3}, ragged=True)]
    # A3: other widths, four full workgroups and a ragged fifth (L = 4 R S + 13); C = 100 leaves R = 1 chunk of output per workgroup
    + [_case("A3-C1", 4 * 508 * 40 + 13, Craw=1, B=2), _case("A3-C5", 4 * 98 * 40 + 13, Craw=5, B=2),
       _case("A3-C37", 4 * 9 * 40 + 13, Craw=37, B=2), _case("A3-C64", 4 * 4 * 40 + 13, Craw=64, B=2),
       _case("A3-C100", 4 * 1 * 40 + 13, Craw=100, B=2)]
    # A4: decimation edges
    + [_case(f"A4-L{L}", L) for L in (1, 4, 5, 6, 39, 40, 41, 9999)]
    # A5: the one-thread-per-row kernel (order 4, step 5 at 20 Hz is the scan: listed so that every order is compared)
    + [_case(f"A5-order{o}", 1003, order=o, path="scan" if o == 4 else "sequential") for o in range(1, 9)]
    + [_case(f"A5-order{o}-step{s}", 1003, order=o, step=s, path="sequential") for o in (2, 4) for s in (1, 2, 4, 7)]
    + [_case("A5-2Hz", 1003, cutoff=2.0, path="sequential")]
    # sequential because of LDS, as in the existing indexed test, and because the raw rows are too wide
    + [_case("A5-3of19", 1003, channels=[3, 0, 18], path="sequential"), _case("A5-19of64", 203, Craw=64, channels=list(range(19)), path="sequential")]
    # A7: longer warm-ups
    + [_case("A7-10Hz", 1723, cutoff=10.0, shifts={0, 1, 2}, ragged=True), _case("A7-2Hz-C5", 5003, Craw=5, cutoff=2.0, shifts={0, 2, 3}, ragged=True)]
)
