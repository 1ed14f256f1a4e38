"""CPU: LIME argument checks that run before anything reaches a device, the limits of the bx_lime_* entry points, the restatement
(tests/lime_ref.py) against scikit-learn, grid_segments, and LimeExplanation.get_image_and_mask against the restatement."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib
from tests import lime_ref as R

BX_EINVAL, BX_EUNSUPPORTED = -1, -6


def _recorder(monkeypatch):
    reached = []

    class Recorder:
        def __getattr__(self, name):
            def call(*args):
                reached.append(name)
                raise RuntimeError(f"{name} called")
            return call
    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: SimpleNamespace(cuda_stream=0))
    return reached


def _image(H=16, W=24, C=3):
    return (np.random.default_rng(0).random((H, W, C)) * 255.9).astype(np.uint8)


def _gap():
    seg = brainxai.grid_segments(16, 24, 2, 3).copy()
    seg[seg == 4] = 7                                               # labels 0..3, 5, 7: a gap
    return seg


def _negative():
    seg = brainxai.grid_segments(16, 24, 2, 3).copy()
    seg[0, 0] = -1
    return seg


BAD = {
    "gap": (dict(segments=_gap()), ValueError, "every label"),
    "negative": (dict(segments=_negative()), ValueError, "negative label"),
    "shape": (dict(segments=brainxai.grid_segments(16, 20, 2, 3)), ValueError, "do not match"),
    "float_labels": (dict(segments=brainxai.grid_segments(16, 24, 2, 3).astype(np.float32)), ValueError, "integer label map"),
    "too_many_segments": (dict(image=_image(40, 40), segments=np.arange(1600, dtype=np.int32).reshape(40, 40)), ValueError, "1600 segments"),
    "channels": (dict(image=_image(C=5)), ValueError, "5 channels"),
    "forward_selection": (dict(feature_selection="forward_selection"), ValueError, "'auto'.*'none'.*'highest_weights'"),
    "lasso_path": (dict(feature_selection="lasso_path"), ValueError, "'auto'.*'none'.*'highest_weights'"),
    "auto_small": (dict(feature_selection="auto", num_features=6), ValueError, "forward_selection.*'none' or 'highest_weights'"),
    "one_sample": (dict(num_samples=1), ValueError, "num_samples = 1"),
    "label_high": (dict(labels=(0, 6)), ValueError, r"outside \[0, 6\)"),
    "label_negative": (dict(labels=(-1,)), ValueError, r"outside \[0, 6\)"),
    "masks_shape": (dict(masks=np.ones((10, 5), np.uint8), num_samples=10), ValueError, "masks must be 0/1"),
    "masks_values": (dict(masks=np.full((10, 6), 2, np.uint8), num_samples=10), ValueError, "masks must be 0/1"),
    "cpu_model": (dict(), RuntimeError, "must live on the GPU"),
}


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("wrapper", ["spectrogram", "multimodal"])
def test_bad_arguments_raise_before_launch(monkeypatch, case, wrapper):
    reached = _recorder(monkeypatch)
    net = brainxai.Spectrogram_Model(6) if wrapper == "spectrogram" else brainxai.build_multimodal(19, 2000, 3)
    kw, exc, match = BAD[case]
    args = dict(image=_image(), segments=brainxai.grid_segments(16, 24, 2, 3), num_samples=20)
    args.update(kw)
    with pytest.raises(exc, match=match):
        brainxai.lime_image(net, **args)
    assert reached == [], f"library entry points reached: {reached}"


def test_entry_points_refuse_limits_given_null_pointers():
    lib = _lib.load()
    msg = lib.bx_last_error_string
    # (B, H, W, C, S)
    for B, H, W, C, S, code, word in [(1, 8, 8, 3, 0, BX_EUNSUPPORTED, b"segments"), (1, 8, 8, 3, 1025, BX_EUNSUPPORTED, b"segments"),
                                      (1, 8, 8, 0, 4, BX_EUNSUPPORTED, b"channels"), (1, 8, 8, 5, 4, BX_EUNSUPPORTED, b"channels"),
                                      (0, 8, 8, 3, 4, BX_EINVAL, b"bad shape"), (1, 8, 8, 3, 4, BX_EINVAL, b"null pointer")]:
        rc = lib.bx_lime_segment_mean(None, None, None, B, H, W, C, S, None)
        assert rc == code and b"bx_lime_segment_mean" in msg() and word in msg(), (rc, msg())
        rc = lib.bx_lime_perturb(None, None, None, None, None, B, H, W, C, 8, S, 10, 0, 10, _lib.BX_F32, None)
        assert rc == code and b"bx_lime_perturb" in msg() and word in msg(), (rc, msg())
    for N, n0, n, word in [(1, 0, 1, b"N = 1"), (10, 5, 6, b"outside"), (10, -1, 2, b"outside"), (10, 0, 0, b"outside")]:
        rc = lib.bx_lime_perturb(None, None, None, None, None, 1, 8, 8, 3, 8, 4, N, n0, n, _lib.BX_F32, None)
        assert rc == BX_EINVAL and word in msg(), (rc, msg())
    assert lib.bx_lime_perturb(None, None, None, None, None, 1, 8, 8, 3, 16, 4, 10, 0, 10, _lib.BX_F32, None) == BX_EINVAL and b"Cp" in msg()
    assert lib.bx_lime_perturb(None, None, None, None, None, 1, 8, 8, 3, 8, 4, 10, 0, 10, 7, None) < 0 and b"dtype" in msg()
    assert lib.bx_lime_perturb(None, None, None, None, None, 1, 4096, 4096, 3, 8, 4, 100, 0, 64, _lib.BX_F32, None) == BX_EINVAL and b"32-bit" in msg()

    def fit(B=1, N=10, S=4, Sp=4, K=6, nl=2, alpha=1.0, kw=0.25, used=None):
        return lib.bx_lime_fit(None, None, None, used, B, N, S, Sp, K, nl, alpha, kw, None, 0, None, None, None, None, None, None)
    for kw, code, word in [(dict(S=0, Sp=0), BX_EUNSUPPORTED, b"segments"), (dict(S=1025, Sp=1025), BX_EUNSUPPORTED, b"segments"),
                           (dict(K=33), BX_EUNSUPPORTED, b"classes"), (dict(N=1), BX_EINVAL, b"N = 1"), (dict(nl=7), BX_EINVAL, b"labels"),
                           (dict(nl=0), BX_EINVAL, b"labels"), (dict(Sp=5), BX_EINVAL, b"used features"), (dict(Sp=0), BX_EINVAL, b"used features"),
                           (dict(alpha=0.0), BX_EINVAL, b"alpha"), (dict(kw=0.0), BX_EINVAL, b"kernel_width"),
                           (dict(Sp=3), BX_EINVAL, b"`used` list"), (dict(), BX_EINVAL, b"null pointer")]:
        rc = fit(**kw)
        assert rc == code and b"bx_lime_fit" in msg() and word in msg(), (kw, rc, msg())
    shape = lambda **kw: {**dict(B=1, N=10, S=4, Sp=4, K=6, nl=2), **kw}
    for bad in (shape(S=1025, Sp=4), shape(K=33), shape(N=1), shape(Sp=5), shape(nl=7), shape(B=0)):
        assert lib.bx_lime_fit_workspace(bad["B"], bad["N"], bad["S"], bad["Sp"], bad["K"], bad["nl"]) == 0
    sizes = [lib.bx_lime_fit_workspace(1, 100, S, S, 6, 5) for S in (1, 48, 192, 1024)]
    assert sizes[0] >= 8 and all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 1024 * 1024 * 8
    assert lib.bx_lime_fit_workspace(3, 100, 48, 48, 6, 5) >= 3 * sizes[1]
    assert lib.bx_lime_fit_workspace(1, 100, 192, 10, 6, 1) < sizes[2]

    for kw, code, word in [(dict(S=1025, Sp=4), BX_EUNSUPPORTED, b"segments"), (dict(Sp=5), BX_EINVAL, b"used features"),
                           (dict(nl=33), BX_EINVAL, b"labels"), (dict(Sp=3), BX_EINVAL, b"used features"), (dict(), BX_EINVAL, b"null pointer")]:
        a = {**dict(B=1, nl=2, H=8, W=8, S=4, Sp=4), **kw}
        rc = lib.bx_lime_weight_map(None, None, None, None, a["B"], a["nl"], a["H"], a["W"], a["S"], a["Sp"], None)
        assert rc == code and b"bx_lime_weight_map" in msg() and word in msg(), (kw, rc, msg())


# ---- the restatement against scikit-learn ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", [(100, 48), (1000, 192), (300, 300)])
def test_distance_identity_against_sklearn(N, S):
    data = R.draw_masks(N, S, np.random.RandomState(N + S))
    data[1, :] = 0                                                  # an all-zero row: distance 1
    d = R.distances(data)
    err = np.abs(R.distances_closed_form(data) - d).max()
    print(f"distance identity N={N} S={S}: {err:.1e}")
    assert err < 1e-14 and d[1] == 1.0                               # scikit-learn's own d[0] is a few ulp of 1 above zero


@pytest.mark.parametrize("N,S,alpha", [(100, 48, 1.0), (1000, 192, 1.0), (300, 300, 1.0), (100, 48, 0.01), (64, 1, 1.0)])
def test_closed_form_fit_against_sklearn_ridge(N, S, alpha):
    rs = np.random.RandomState(7 * N + S)
    data = R.draw_masks(N, S, rs)
    y = rs.rand(N)
    w = R.kernel(R.distances(data))
    beta, icpt, score, pred = R.ridge_closed_form(data, y, w, alpha)
    beta_r, icpt_r, score_r, pred_r = R.ridge_sklearn(data, y, w, alpha)
    scale = np.abs(beta_r).max()
    errs = (np.abs(beta - beta_r).max() / scale, abs(icpt - icpt_r), abs(score - score_r), abs(pred - pred_r))
    print(f"closed form vs Ridge N={N} S={S} alpha={alpha}: coef {errs[0]:.1e} intercept {errs[1]:.1e} score {errs[2]:.1e} pred {errs[3]:.1e}")
    assert max(errs) < 1e-12


def test_mask_draw_follows_the_randomstate_rule():
    rs = np.random.RandomState(11)
    want = [np.random.RandomState(11).randint(0, 2, 2 * 20 * 7)[:140].reshape(20, 7), None]
    want[1] = np.random.RandomState(11).randint(0, 2, 2 * 20 * 7)[140:].reshape(20, 7)      # the second image continues the stream
    for b in range(2):
        got = R.draw_masks(20, 7, rs)
        assert (got[0] == 1).all() and np.array_equal(got[1:], want[b][1:])


@pytest.mark.parametrize("H,W,rows,cols", [(64, 96, 8, 8), (100, 75, 10, 5), (400, 300, 16, 12), (33, 47, 5, 7), (7, 7, 7, 7), (5, 9, 1, 1)])
def test_grid_segments(H, W, rows, cols):
    seg = brainxai.grid_segments(H, W, rows, cols)
    assert seg.shape == (H, W) and seg.dtype == np.int32
    assert np.array_equal(np.unique(seg), np.arange(rows * cols))
    r, c = seg // cols, seg % cols
    assert (r == r[:, :1]).all() and (c == c[:1, :]).all()                                  # label = row * cols + col of a tile grid
    assert (np.diff(r[:, 0]) >= 0).all() and (np.diff(c[0]) >= 0).all()
    hs, ws = np.bincount(r[:, 0]), np.bincount(c[0])
    assert hs.max() - hs.min() <= 1 and ws.max() - ws.min() <= 1 and hs.min() >= 1 and ws.min() >= 1
    with pytest.raises(ValueError):
        brainxai.grid_segments(H, W, H + 1, cols)
    with pytest.raises(ValueError):
        brainxai.grid_segments(H, W, rows, 0)


FLAGS = [dict(), dict(positive_only=False), dict(positive_only=False, negative_only=True), dict(hide_rest=True), dict(num_features=2),
         dict(min_weight=0.25), dict(positive_only=False, min_weight=0.25, num_features=4), dict(positive_only=False, hide_rest=True),
         dict(positive_only=False, negative_only=True, min_weight=0.35, hide_rest=True)]


@pytest.mark.parametrize("flags", FLAGS, ids=[",".join(f"{k}={v}" for k, v in f.items()) or "default" for f in FLAGS])
@pytest.mark.parametrize("dtype", [np.uint8, np.float64])
def test_get_image_and_mask_against_restatement(flags, dtype):
    image = (np.random.default_rng(2).random((12, 18, 3)) * 255.9).astype(dtype)
    seg = brainxai.grid_segments(12, 18, 2, 3)
    exp = [(4, -0.5), (1, 0.4), (0, 0.3), (5, -0.2), (2, 0.1), (3, 0.0)]
    mine = brainxai.LimeExplanation(image, seg)
    mine.local_exp[2] = list(exp)
    ref = SimpleNamespace(image=image, segments=seg, local_exp={2: list(exp)})
    got, want = mine.get_image_and_mask(2, **flags), R.get_image_and_mask(ref, 2, **flags)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype
    assert np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype
    assert np.array_equal(image, ref.image), "the explanation's image is not modified"
    with pytest.raises(KeyError):
        mine.get_image_and_mask(3)
    with pytest.raises(ValueError):
        mine.get_image_and_mask(2, positive_only=True, negative_only=True)


def test_restatement_against_the_package():
    """Only where the lime package is installed: tests/lime_ref.py against LimeImageExplainer itself."""
    lime_image = pytest.importorskip("lime.lime_image")
    image = (np.random.default_rng(4).random((24, 30, 3)) * 255.9).astype(np.uint8)
    seg = brainxai.grid_segments(24, 30, 3, 4)
    Wm = np.random.default_rng(5).standard_normal((3, 4))

    def clf(ims):
        z = np.asarray(ims, np.float64).mean((1, 2)) @ Wm / 64.0
        return np.exp(z) / np.exp(z).sum(1, keepdims=True)
    theirs = lime_image.LimeImageExplainer(random_state=3).explain_instance(image, clf, top_labels=2, num_samples=50, segmentation_fn=lambda im: seg)
    rs = np.random.RandomState(3)
    rs.randint(0, high=1000)                # explain_instance draws the segmenter's seed from the same stream before the masks
    mine = R.explain(image, seg, clf, top_labels=2, num_samples=50, random_state=rs)
    assert list(theirs.top_labels) == mine.top_labels
    for k in mine.top_labels:
        assert [f for f, _ in theirs.local_exp[k]] == [f for f, _ in mine.local_exp[k]]
        assert np.allclose([v for _, v in theirs.local_exp[k]], [v for _, v in mine.local_exp[k]], rtol=0, atol=1e-12)
        assert abs(theirs.intercept[k] - mine.intercept[k]) < 1e-12 and abs(theirs.score[k] - mine.score[k]) < 1e-12
        assert abs(float(np.ravel(theirs.local_pred[k])[0]) - mine.local_pred[k]) < 1e-12
        for flags in FLAGS:
            a, b = theirs.get_image_and_mask(k, **flags), R.get_image_and_mask(mine, k, **flags)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
