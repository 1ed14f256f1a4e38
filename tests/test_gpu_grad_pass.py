"""GPU: the pass that gradient_shap and smooth_grad share (explain._GradPass), at its seam: the chunking by max_batch, the gradient
seeds read at the rows of a chunk, and the model's state when a driver's own step fails.

Shapes: the interface model of tests/grad_gpu.py, B = 2, EEG 19x2000 and spectrogram 4x32x64, n = 6 draws (Nb = 3 backgrounds): 12 rows.
max_batch 256 is one chunk, 1 a chunk per row; at 5 and 7 the chunks begin and end inside a sample and the last one is short.
Bound: against the one-chunk call the values stay within TOL = 1e-3 of the per-(sample, class) maximum, the project's fp32 gradient
bound (TOL of tests/test_gpu_parity.py) -- gradients of batches composed differently need not be bit-equal; what does not pass through
a chunk (the classes, the clean output, sigma, the draws) is equal bit for bit.  The guard, on the one-chunk side alone: explaining
classes [1, 4] instead of [4, 1] moves the values by more than 100 x TOL for every sample, so a seed read at the wrong row cannot pass.
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
DRIVERS = {"gradient_shap": "bx_expgrad_rows", "smooth_grad": "bx_smoothgrad_rows"}          # the driver's own row launch
CLASS_FORMS = {"top": None, "pair": [4, 1], "swapped": [1, 4], "all": "all"}
drivers_and_inputs = pytest.mark.parametrize("driver,input", [(d, i) for d in DRIVERS for i in ("eeg", "spec")])


def _call(driver, input, form, max_batch):
    mine, eeg, spec = GG.iface()
    kw = dict(input=input, nsamples=N, class_idx=CLASS_FORMS[form], seed=3, max_batch=max_batch, return_parts=True)
    if driver == "gradient_shap":
        return brainxai.gradient_shap(mine, eeg, spec, GG.backgrounds()[input == "spec"], **kw)
    return brainxai.smooth_grad(mine, eeg, spec, **kw)


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
@drivers_and_inputs
def test_chunks_against_one_chunk(driver, input, form):
    one = _one_chunk(driver, input, form)
    fixed = [f for f in one._fields if f not in ("attribution", "values")]           # classes, out, sigma / idx, alpha, and what was given
    line = []
    for max_batch in (1, 5, 7):
        res = _call(driver, input, form, max_batch)
        for f in fixed:
            assert _same(getattr(res, f), getattr(one, f)), f"{driver} {input} {form}, max_batch {max_batch}: {f} differs from the one-chunk call"
        err = GG.worst(_with_class_axis(res, res.values), _with_class_axis(one, one.values))
        line.append(f"max_batch {max_batch}: {err:.3e}")
        assert err <= TOL, f"{driver} {input} {form}, max_batch {max_batch}: values {err:.3e} of the maximum, bound {TOL}"
    print(f"{driver} {input} input, classes {form}: of the per-(sample, class) maximum, " + "; ".join(line))


@drivers_and_inputs
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
    """A Python exception out of the driver's write step, in the second chunk: the training flag and every requires_grad come back, and
    the next call returns the bits of a call made before."""
    mine, _, _ = GG.iface()
    fresh = _call(driver, input, "pair", 5)
    lib, launch, calls = L.load(), getattr(L.load(), DRIVERS[driver]), []

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
            patch.setattr(lib, DRIVERS[driver], failing)
            with pytest.raises(_RowWriterFailed):
                _call(driver, input, "pair", 5)
        assert len(calls) == 2 and getattr(lib, DRIVERS[driver]) is launch
        assert PG.model_state(mine) == before and mine.training and not frozen.requires_grad
    finally:
        frozen.requires_grad_(True)
        mine.eval()
    again = _call(driver, input, "pair", 5)
    for f in fresh._fields:
        assert _same(getattr(again, f), getattr(fresh, f)), f"{driver} {input}: {f} after the failed call differs from the call before it"
