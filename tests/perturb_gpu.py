"""What the GPU tests of the perturb-and-predict attributions (deletion / insertion, RISE, occlusion, Score-CAM, Kernel SHAP, LIME,
gradient_shap) share: device handles, the models and inputs they are run on, the bit-for-bit check of the perturbed rows and the
guard on the reference side.  A plain module: no tests, no fixtures of pytest's.

Bounds.  TOL, fp32 storage: |p - reference| <= 1e-5 absolute on probabilities.  The project's recorded fp32 logit parity is 1e-6
(README, test_gpu_bench_config.py) and |dp| <= p (1 - p) 2 max|dlogit| <= 0.5 max|dlogit|, so 1e-5 leaves about a tenfold margin at
logits of order 1; the reference's own fp32-vs-fp64 noise on these cases is 1.5e-7.  A log-probability is the model's output itself:
the same bound holds.  BF16_LOGP, bf16 storage: log-probabilities within 2e-2 of their scale (test_bench_config_bf16_train_step),
the scale being the largest |log-probability| of the fp64 oracle on the unperturbed inputs (logp_scale), and |dp| = p |dlogp| <=
|dlogp|.  A method carries either bound through its own reduction (a weighted sum, a mean, a fit) and says how in its own docstring.
The guard: every compared case is first checked ON THE REFERENCE SIDE to discriminate: the reference with its score rows shuffled
across the masks differs from the true one by more than 100 x the bound for every sample (guard_moved) -- a reduction that paired
scores with the wrong masks cannot pass."""
import copy

import numpy as np
import torch

import brainxai
from brainxai import ops
from oracle import ref_torch as O

DEV = torch.device("cuda:0")
TOL = 1e-5
BF16_LOGP = 2e-2


def p(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def np_bits(a):
    """A numpy array's bits as integers of its item size: equality then tells -0.0 from 0.0 and compares NaNs."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def misaligned(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary: the entry points then take the element-by-element path."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def model_state(model):
    return model.training, [q.requires_grad for q in model.parameters()]


# ---- models and inputs ----------------------------------------------------------------------------------------------------------------------
def baseline(kind, x, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "scalar":
        return 0.25
    if kind == "per_channel":
        return torch.rand(x.shape[2] if x.shape[1] == 1 else x.shape[1], generator=g) - 0.5
    return torch.rand(x.shape, generator=g) - 0.5


def base_host(base):
    """-> (the entry points' baseline kind 0 / 1 / 2, fp32 host tensor [1] / [C or Chans] / x's shape)."""
    if not isinstance(base, torch.Tensor):
        return 0, torch.tensor([base], dtype=torch.float32)
    return (1 if base.dim() == 1 else 2), base.contiguous()


def base_dev(base):
    kind, t = base_host(base)
    return kind, t.to(DEV)


def row_inputs(shape, kind):
    """The input of a row test, [B,C,H,W] or [B,1,Chans,T], with -0.0 planted (a row keeps a zero's sign), and its baseline of
    ``kind``: (x, base, the entry points' baseline kind, base on the device)."""
    eeg = shape[1] == 1
    x = O.seeded(shape, 6 if eeg else 3, "randn")
    x[:, :, ::3 if eeg else 7, ::11 if eeg else 5] = -0.0
    base = baseline(kind, x, 8 if eeg else 4)
    return (x, base) + base_dev(base)


def scaled_multimodal(dt=torch.float32):
    """fill_params(seed=42) as it stands saturates (p = 0.9999, the deletion curve stays above 0.99 until the last point): the heads
    are scaled down so that p0 ~ 0.54 and the spectrogram-input curves span 0.17."""
    ref = O.fill_params(O.build_multimodal(19, 2000, 4, dropout=0.0), seed=42).eval()
    with torch.no_grad():
        ref.spectrogram_model.fc.weight *= 0.05
        ref.eeg_model.dense.weight *= 0.05
        ref.fc2.weight *= 0.5
    mine = brainxai.build_multimodal(19, 2000, 4, dropout=0.0, compute_dtype=dt)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV).eval()


def mm_inputs():
    return O.seeded((3, 1, 19, 2000), 12, "randn"), O.seeded((3, 4, 64, 128), 11, "rand")


def eegnet_pair():
    ref = O.fill_params(O.EEGNet(6, 19, 2000), seed=31).eval()
    mine = brainxai.EEGNet(6, Chans=19, Samples=2000)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV).eval()


# ---- perturbed rows, bit for bit ------------------------------------------------------------------------------------------------------------
def want_rows(row_of, x, base, n0, n):
    """The reference rows n0..n0+n-1 of every sample of x, sample-major: row_of(b, j, base_b) is the method's restatement of row j of
    sample b, [1,...] (the index, not x[b:b+1]: the curves' rows also need the sample's ranks); a baseline of x's shape is cut to
    the sample."""
    rows = []
    for b in range(x.shape[0]):
        bb = base[b:b + 1] if isinstance(base, torch.Tensor) and base.dim() == 4 else base
        rows += [row_of(b, n0 + j, bb) for j in range(n)]
    return torch.cat(rows)


def row_windows(N):
    """(n0, n) of N rows per sample: all; a range that starts past 0, crosses the kernels' groups of 8 and ends on the last row; the last alone."""
    return sorted({(0, N), (N // 3, N - N // 3), (N - 1, 1)})


def assert_same_rows(got, want, what, C=None):
    """Every element written, the reference's shape and the reference's bits (a zero's sign included); with C given the rows are
    [R,H,W,8] and the padding channels C..7 are exactly zero.  Works on tensors of any device."""
    assert not torch.isnan(got.float()).any(), f"{what}: unwritten elements"
    assert got.shape == want.shape and torch.equal(bits(got), bits(want)), what
    if C is not None:
        assert float(got[..., C:].float().abs().max()) == 0.0, f"{what}: padding channels"


def _check_rows(launch, row_of, x, base, windows, writer, out_shape, dt, C, what):
    B = x.shape[0]
    for n0, n in windows:
        out = torch.full((B * n, *out_shape), float("nan"), dtype=dt, device=DEV)
        launch(out, n0, n)
        want = want_rows(row_of, x, base, n0, n).to(DEV)
        want = want if C is None else ops.to_nhwc(want, dt)
        torch.cuda.synchronize()
        assert_same_rows(out, want, f"{what} window {(n0, n)}", C)
        for b0, nb in ((0, B), (1, 1)):                              # the second sample group does not start at 0
            assert_same_rows(writer(b0, nb, n0, n), want[b0 * n:(b0 + nb) * n], f"{what} window {(n0, n)} row writer, samples {(b0, nb)}", C)


def check_spec_rows(launch, row_of, x, base, windows, writer, dt, what):
    """Spectrogram rows [B*n,H,W,8] in ``dt`` of x [B,C,H,W], B >= 2, for every (n0, n) of ``windows``.  launch(out, n0, n) runs the entry
    point on rows n0..n0+n-1 of all samples into ``out`` (pre-filled with NaN); row_of and base are want_rows's; writer(b0, nb, n0, n)
    is the driver's row writer on samples b0..b0+nb-1."""
    _check_rows(launch, row_of, x, base, windows, writer, (x.shape[2], x.shape[3], 8), dt, x.shape[1], what)


def check_eeg_rows(launch, row_of, x, base, windows, writer, what):
    """The same for the fp32 EEG rows [B*n,1,Chans,T] of x [B,1,Chans,T]."""
    _check_rows(launch, row_of, x, base, windows, writer, x.shape[1:], torch.float32, None, what)


# ---- the guard on the reference side and the bf16 scale -------------------------------------------------------------------------------------
def spans(ref, classes):
    return f"span {[round(float(np.ptp(ref[b, c])), 4) for b, c in enumerate(classes)]}"


def guard_moved(true_ref, shuffled_ref, classes, tol, what, shown=None, noun="map"):
    """true_ref, shuffled_ref [B,K,...]: the reference of the explained class must move by more than 100 x tol for every sample when
    the score rows are shuffled.  ``shown`` replaces the span in the printed line."""
    moved = np.array([np.abs(true_ref[b, c] - shuffled_ref[b, c]).max() for b, c in enumerate(classes)])
    print(f"{what}: reference classes {classes} {spans(true_ref, classes) if shown is None else shown} |{noun} - shuffled| / bound {(moved / tol).round(0)}")
    assert moved.min() > 100 * tol, f"{what}: shuffling the scores moves the reference {noun} by {moved.min():.1e} only"


def logp_scale(ref_model, *inputs):
    """The largest |log-probability| of the fp64 oracle on the unperturbed inputs: the scale of the bf16 bound."""
    with torch.no_grad():
        return float(copy.deepcopy(ref_model).double()(*(t.double() for t in inputs)).abs().max())
