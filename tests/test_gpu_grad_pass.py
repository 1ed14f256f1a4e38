"""GPU: the pass behind the gradient drivers (explain._GradPass), at its seam: the chunking by max_batch, the gradient seeds read at
the rows of a chunk, and the model's state when a driver's own step fails.  Its sampled route serves gradient_shap, smooth_grad and
blur_ig (n rows per sample, one backward pass per class slot), its per-row route guided_ig and mask_explain (one row per (sample,
class), iterated).

Shapes: the interface model of tests/grad_gpu.py, B = 2, EEG 19x2000 and spectrogram 4x32x64.  Sampled route: n = 6 draws (Nb = 3
backgrounds) or 6 blur steps: 12 rows.  max_batch 256 is one chunk, 1 a chunk per row; at 5 and 7 the chunks begin and end inside a
sample and the last one is short.  Per-row route: class_idx='all', 2 x 6 = 12 rows, 3 steps / iterations, max_batch 5: three chunks
per iteration (that no bit of these two drivers' results depends on max_batch is asserted by test_class_forms_and_max_batch of
tests/test_gpu_guided_ig.py and tests/test_gpu_maskopt.py).
Bound: against the one-chunk call the values stay within TOL = 1e-3 of the per-(sample, class) maximum, the project's fp32 gradient
bound (TOL of tests/test_gpu_parity.py) -- gradients of batches composed differently need not be bit-equal; what does not pass through
a chunk (the classes, the clean output, sigma, the draws, blur_ig's endpoint and schedule) is equal bit for bit.  The guard, on the
one-chunk side alone: explaining classes [1, 4] instead of [4, 1] moves the values by more than 100 x TOL for every sample, so a seed
read at the wrong row cannot pass.
Observed figures are printed by each test (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from tests import grad_gpu as GG
from tests import perturb_gpu as PG

pytestmark = pytest.mark.gpu
TOL = 1e-3
N = 6
STEPS = 3
BLUR_MAX_SIGMA = {"eeg": 8.0, "spec": 3.0}                    # those of tests/test_gpu_blur_ig.py: the filters fit both inputs
# the driver's own per-chunk launch, the one that is made to fail: the row writers of the sampled route, the step / the rows of the per-row one
SAMPLED = {"gradient_shap": "bx_expgrad_rows", "smooth_grad": "bx_smoothgrad_rows", "blur_ig": "bx_blur_rows"}
PER_ROW = {"guided_ig": "bx_guided_ig_step", "mask_explain": "bx_maskopt_rows_{input}"}
CLASS_FORMS = {"top": None, "pair": [4, 1], "swapped": [1, 4], "all": "all"}
sampled_and_inputs = pytest.mark.parametrize("driver,input", [(d, i) for d in SAMPLED for i in ("eeg", "spec")])
drivers_and_inputs = pytest.mark.parametrize("driver,input", [(d, i) for d in (*SAMPLED, *PER_ROW) for i in ("eeg", "spec")])


def _call(driver, input, form, max_batch):
    mine, eeg, spec = GG.iface()
    kw = dict(input=input, class_idx=CLASS_FORMS[form], max_batch=max_batch, return_parts=True)
    if driver == "gradient_shap":
        return brainxai.gradient_shap(mine, eeg, spec, GG.backgrounds()[input == "spec"], nsamples=N, seed=3, **kw)
    if driver == "smooth_grad":
        return brainxai.smooth_grad(mine, eeg, spec, nsamples=N, seed=3, **kw)
    if driver == "blur_ig":
        return brainxai.blur_ig(mine, eeg, spec, steps=N, max_sigma=BLUR_MAX_SIGMA[input], **kw)
    if driver == "guided_ig":
        return brainxai.guided_ig(mine, eeg, spec, steps=STEPS, keep_path=True, **kw)
    return brainxai.mask_explain(mine, eeg, spec, iterations=STEPS, grid=6, keep_path=True, **kw)


@functools.lru_cache(maxsize=None)
def _one_chunk(driver, input, form):
    """The call whose 12 rows are one chunk; computed once, never written to."""
    return _call(driver, input, form, 256)


def _with_class_axis(res, t):
    """[B,K,...] for GG.worst: a result for one class per sample has no class axis."""
    return t if res.classes is None else t[:, None]


def _same(a, b):
    if a is None or b is None:
        return a is b
    return torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(a, b)


@pytest.mark.parametrize("form", ["top", "pair", "all"])
@sampled_and_inputs
def test_chunks_against_one_chunk(driver, input, form):
    one = _one_chunk(driver, input, form)
    # classes, out, sigma / idx, alpha / endpoint, sigmas, and what was given; blur_ig's map and delta are sums of its values
    fixed = [f for f in one._fields if f not in ("attribution", "map", "values", "delta")]
    line = []
    for max_batch in (1, 5, 7):
        res = _call(driver, input, form, max_batch)
        for f in fixed:
            assert _same(getattr(res, f), getattr(one, f)), f"{driver} {input} {form}, max_batch {max_batch}: {f} differs from the one-chunk call"
        err = GG.worst(_with_class_axis(res, res.values), _with_class_axis(one, one.values))
        line.append(f"max_batch {max_batch}: {err:.3e}")
        assert err <= TOL, f"{driver} {input} {form}, max_batch {max_batch}: values {err:.3e} of the maximum, bound {TOL}"
    print(f"{driver} {input} input, classes {form}: of the per-(sample, class) maximum, " + "; ".join(line))


@sampled_and_inputs
def test_swapped_classes_move_the_one_chunk_result(driver, input):
    pair, swapped = _one_chunk(driver, input, "pair"), _one_chunk(driver, input, "swapped")
    assert pair.classes.tolist() == [4, 1] and swapped.classes.tolist() == [1, 4]
    moved = GG.per_pair_max((pair.values - swapped.values)[:, None]) / GG.per_pair_max(pair.values[:, None])
    print(f"{driver} {input} input: classes [1, 4] instead of [4, 1] move the values by {moved.flatten().tolist()} of the per-sample maximum")
    assert float(moved.min()) > 100 * TOL, f"{driver} {input}: swapping the classes moves the result by only {float(moved.min()):.3e}"


class _RowWriterFailed(Exception):
    pass


@drivers_and_inputs
def test_state_after_a_failing_row_writer(driver, input, monkeypatch):
    """A Python exception out of the driver's own per-chunk launch, in the second chunk: the training flag and every requires_grad come
    back, and the next call returns the bits of a call made before."""
    mine, _, _ = GG.iface()
    form = "all" if driver in PER_ROW else "pair"                                    # 12 rows either way: three chunks of at most 5
    name = {**SAMPLED, **PER_ROW}[driver].format(input=input)
    fresh = _call(driver, input, form, 5)
    lib, launch, calls = L.load(), getattr(L.load(), name), []

    def failing(*args):
        calls.append(len(args))
        if len(calls) == 2:
            raise _RowWriterFailed
        return launch(*args)

    mine.train()
    frozen = mine.fc1.bias
    frozen.requires_grad_(False)
    try:
        before = PG.model_state(mine)
        with monkeypatch.context() as patch:
            patch.setattr(lib, name, failing)
            with pytest.raises(_RowWriterFailed):
                _call(driver, input, form, 5)
        assert len(calls) == 2 and getattr(lib, name) is launch
        assert PG.model_state(mine) == before and mine.training and not frozen.requires_grad
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    again = _call(driver, input, form, 5)
    for f in fresh._fields:
        assert _same(getattr(again, f), getattr(fresh, f)), f"{driver} {input}: {f} after the failed call differs from the call before it"
