"""CPU: the shared assertions of tests/perturb_gpu.py on tensors of a few dozen elements -- every defect the bit-for-bit row check and
the reference-side guard exist to catch must raise, and an exact copy must pass."""
import numpy as np
import pytest
import torch

from tests import perturb_gpu as PG

C = 3


def _rows(dt=torch.float32):
    """[4,2,3,8] rows as the kernels write them: values in channels 0..C-1 with a -0.0 among them, zeros in the padding."""
    t = torch.zeros(4, 2, 3, 8)
    t[..., :C] = torch.randn(4, 2, 3, C, generator=torch.Generator().manual_seed(0))
    t[1, 1, 2, 0] = -0.0
    return t.to(dt)


# defect -> (element, the value put there or None to flip its lowest mantissa bit, what the failure says)
DEFECTS = {"unwritten element": ((2, 1, 1, 1), float("nan"), "unwritten"), "flipped low mantissa bit": ((0, 0, 1, 0), None, "^case$"),
           "+0.0 for -0.0": ((1, 1, 2, 0), 0.0, "^case$"), "non-zero padding channel": ((0, 0, 0, 6), 0.5, "^case$")}


def _spoil(t, at, value):
    if value is None:
        PG.bits(t)[at] ^= 1
    else:
        t[at] = value


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_exact_copy_passes(dt):
    want = _rows(dt)
    PG.assert_same_rows(want.clone(), want, "copy", C)
    PG.assert_same_rows(want[..., 0].clone(), want[..., 0].contiguous(), "copy, EEG form")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_one_defect_raises(defect, dt):
    at, value, message = DEFECTS[defect]
    want, got = _rows(dt), _rows(dt)
    _spoil(got, at, value)
    changed = PG.bits(got) != PG.bits(want)
    assert int(changed.sum()) == 1 and (defect != "+0.0 for -0.0" or torch.equal(got, want))
    with pytest.raises(AssertionError, match=message):
        PG.assert_same_rows(got, want, "case", C)


def test_padding_in_the_reference_too_raises():
    want = _rows()
    _spoil(want, *DEFECTS["non-zero padding channel"][:2])           # only the padding check can see it
    with pytest.raises(AssertionError, match="padding"):
        PG.assert_same_rows(want.clone(), want, "case", C)


def test_wrong_row_count_raises():
    want = _rows()
    for got in (want[:3].clone(), torch.cat([want, want[:1]])):
        with pytest.raises(AssertionError, match="^case$"):
            PG.assert_same_rows(got, want, "case", C)


def test_want_rows_is_sample_major_and_cuts_a_tensor_baseline():
    x = torch.arange(2 * 1 * 2 * 3, dtype=torch.float32).reshape(2, 1, 2, 3)
    seen = []

    def row_of(b, j, bb):
        seen.append((b, j, bb if not isinstance(bb, torch.Tensor) else tuple(bb.shape)))
        return x[b:b + 1] + 100 * j
    rows = PG.want_rows(row_of, x, 10 * x, 3, 2)
    assert [s[:2] for s in seen] == [(0, 3), (0, 4), (1, 3), (1, 4)] and all(s[2] == (1, 1, 2, 3) for s in seen)
    assert tuple(rows.shape) == (4, 1, 2, 3) and torch.equal(rows[2], x[1] + 300)
    seen.clear()
    PG.want_rows(row_of, x, 0.25, 0, 1)
    assert [s[2] for s in seen] == [0.25, 0.25]


def test_guard_moved():
    tol = 1e-5
    ref = np.random.default_rng(0).random((3, 6, 4, 5))
    classes = np.array([2, 0, 5])
    with pytest.raises(AssertionError, match="shuffling the scores moves the reference map by"):
        PG.guard_moved(ref, ref.copy(), classes, tol, "equal")
    near = ref.copy()
    near[np.arange(3), classes, 0, 0] += 99 * tol                    # not more than 100 x tol
    with pytest.raises(AssertionError):
        PG.guard_moved(ref, near, classes, tol, "below the limit")
    moved = ref.copy()
    moved[np.arange(3), classes, 1, 1] += 101 * tol
    PG.guard_moved(ref, moved, classes, tol, "moved")
    moved[1, classes[1]] = ref[1, classes[1]]                        # every sample has to move, and in its own class
    moved[1, 3] += 1.0
    with pytest.raises(AssertionError, match="values"):
        PG.guard_moved(ref, moved, classes, tol, "one sample still", "max|values| 1", "values")


@pytest.mark.parametrize("shape", [(2, 4, 6, 5), (2, 1, 7, 9)], ids=["spectrogram", "eeg"])
def test_baseline_kinds_and_shapes(shape):
    x = torch.zeros(shape)
    per = shape[2] if shape[1] == 1 else shape[1]
    want = {"scalar": (0, (1,)), "per_channel": (1, (per,)), "tensor": (2, shape)}
    for kind, (code, base_shape) in want.items():
        base = PG.baseline(kind, x, 4)
        again = PG.baseline(kind, x, 4)
        assert torch.equal(torch.as_tensor(base), torch.as_tensor(again)), "seeded"
        got_code, host = PG.base_host(base)
        assert got_code == code and tuple(host.shape) == base_shape and host.dtype == torch.float32 and host.is_contiguous()
        assert float(host.min()) >= -0.5 and float(host.max()) <= 0.5
        if torch.cuda.is_available():
            dev_code, dev_t = PG.base_dev(base)
            assert dev_code == code and dev_t.is_cuda and torch.equal(dev_t.cpu(), host)
