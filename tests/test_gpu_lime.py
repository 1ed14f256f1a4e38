"""GPU: brainxai.lime_image and the bx_lime_* entry points against the numpy + scikit-learn restatement (tests/lime_ref.py).

Bounds of the fit comparisons (1e-9 of the largest |beta| for coefficients, 1e-9 absolute for intercept, score, local_pred): the
system matrix has eigenvalues in [alpha, alpha + sum(w) S]; for every case compared its condition number, computed with numpy on
the reference side, is asserted below 300, so a backward-stable fp64 factorisation leaves about S * 2.2e-16 * cond <= 7e-11 and a
reordered N-term sum 2e-13.  Observed worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from brainxai import ops
from oracle import ref_torch as O
from tests import lime_ref as R
from tests import perturb_gpu as PG
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _pair(make_ref, make_mine, seed):
    ref = O.fill_params(make_ref(), seed=seed)
    mine = make_mine()
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV)


def _voronoi(H, W, cells, singles, seed):
    """Irregular label map: nearest of `cells` random sites, plus `singles` one-pixel segments; labels 0..S-1 without a gap."""
    g = np.random.default_rng(seed)
    sites = np.stack([g.integers(0, H, cells), g.integers(0, W, cells)], 1)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - sites[:, 0]) ** 2 + (xx[..., None] - sites[:, 1]) ** 2
    seg = d.argmin(-1)
    for i in range(singles):
        seg[g.integers(0, H), g.integers(0, W)] = cells + i
    seg = np.unique(seg, return_inverse=True)[1].reshape(H, W).astype(np.int32)
    assert (np.bincount(seg.ravel()) == 1).sum() >= 1
    return seg


def _u8(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 255.9).astype(np.uint8)


def _segment_mean(img, seg, S):
    B, H, W, C = img.shape
    col = torch.empty(B, S, C, dtype=torch.uint8, device=DEV)
    img_d, seg_d = PG.dev(img), PG.dev(seg)                              # held until the launch is queued: a temporary's block is reused at once
    L.check(L.load().bx_lime_segment_mean(PG.p(img_d), PG.p(seg_d), PG.p(col), B, H, W, C, S, PG.stream()), "bx_lime_segment_mean")
    torch.cuda.synchronize()
    return col


def _perturb(img_u8, seg, col, Z, n0, n, dt):
    B, H, W, C = img_u8.shape
    S, N = Z.shape[2], Z.shape[1]
    x = torch.full((B * n, H, W, 8), float("nan"), dtype=dt, device=DEV)
    img_d, seg_d, Z_d = PG.dev(img_u8), PG.dev(seg), PG.dev(Z)
    L.check(L.load().bx_lime_perturb(PG.p(img_d), PG.p(seg_d), PG.p(col), PG.p(Z_d), PG.p(x), B, H, W, C, 8, S, N, n0, n, ops.bx_dtype(dt),
                                     PG.stream()), "bx_lime_perturb")
    torch.cuda.synchronize()
    return x


def _u8_to_nhwc(imgs_u8, dt):
    n, H, W, C = imgs_u8.shape
    x = torch.empty(n, H, W, 8, dtype=dt, device=DEV)
    src = PG.dev(imgs_u8)
    L.check(L.load().bx_u8_to_nhwc(PG.p(src), PG.p(x), n, H, W, C, 8, 1.0 / 255.0, ops.bx_dtype(dt), PG.stream()), "bx_u8_to_nhwc")
    torch.cuda.synchronize()
    return x


GEOMETRIES = {
    "100x75x3_grid10x5": lambda: (_u8((100, 75, 3), 1), brainxai.grid_segments(100, 75, 10, 5)),
    "128x256x4_voronoi": lambda: (_u8((128, 256, 4), 2), _voronoi(128, 256, 70, 6, 3)),
    "400x300x3_grid16x12": lambda: (_u8((400, 300, 3), 4), brainxai.grid_segments(400, 300, 16, 12)),
}


# ---- 1. perturbed batch, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hide", [None, 0, (12, 200, 77, 3)], ids=["mean", "zero", "tuple"])
@pytest.mark.parametrize("B,n0,n", [(1, 0, 11), (3, 5, 9)])
@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
def test_perturbed_batch_bit_for_bit(geom, B, n0, n, hide, dt):
    img1, seg1 = GEOMETRIES[geom]()
    H, W, C = img1.shape
    imgs = np.stack([img1] + [_u8(img1.shape, 50 + b) for b in range(1, B)])
    segs = np.stack([seg1] + [np.ascontiguousarray(seg1[::-1, ::-1]) for _ in range(1, B)])
    S, N = int(seg1.max()) + 1, 16
    hide = hide if hide is None or np.ndim(hide) == 0 else hide[:C]
    rs = np.random.RandomState(9)
    Z = np.stack([R.draw_masks(N, S, rs) for _ in range(B)]).astype(np.uint8)
    col_h = X._lime_colours_host(imgs, segs, S, hide)
    col = _segment_mean(imgs, segs, S) if col_h is None else PG.dev(col_h)
    got = _perturb(imgs, segs, col, Z, n0, n, dt)
    want = []
    for b in range(B):
        fudged = R.fudged_image(imgs[b], segs[b], hide)
        want += R.perturbed_images(imgs[b], segs[b], fudged, Z[b, n0:n0 + n])
    want = _u8_to_nhwc(np.stack(want).astype(np.uint8), dt)
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.equal(got, want)
    assert not torch.isnan(got.float()).any()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_perturbed_batch_float_image(dt):
    """A float image holding 0..255: kept pixels truncated as predict_fn does, colour table from numpy (by design), equal bits."""
    img = np.random.default_rng(5).random((100, 75, 3)) * 255.9
    seg = brainxai.grid_segments(100, 75, 10, 5)
    S, N = 50, 12
    means = np.array([[np.mean(img[seg == s][:, c]) for c in range(3)] for s in range(S)])
    gap = np.abs(means - np.round(means)).min()
    print(f"float image: smallest distance of a segment mean from an integer {gap:.2e}")
    assert gap >= 1e-6                                               # truncation of the means cannot depend on summation order
    Z = R.draw_masks(N, S, np.random.RandomState(2)).astype(np.uint8)[None]
    col = PG.dev(X._lime_colours_host(img[None], seg[None], S, None))
    got = _perturb(img[None].astype(np.uint8), seg[None], col, Z, 0, N, dt)
    want = np.stack(R.perturbed_images(img, seg, R.fudged_image(img, seg), Z[0])).astype(np.uint8)
    assert torch.equal(got, _u8_to_nhwc(want, dt))


# ---- 2. segment means ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["grid", "voronoi", "bands"])
def test_segment_means_equal_numpy(case):
    if case == "grid":
        img, seg = GEOMETRIES["400x300x3_grid16x12"]()
    elif case == "voronoi":
        img, seg = GEOMETRIES["128x256x4_voronoi"]()
    else:                                                            # row bands (one covers whole rows), and one-pixel segments inside them
        img, seg = _u8((90, 130, 1), 8), brainxai.grid_segments(90, 130, 5, 1).copy()
        seg[0, 0], seg[45, 77], seg[89, 129] = 5, 6, 7
    S = int(seg.max()) + 1
    imgs, segs = np.stack([img, img[::-1].copy()]), np.stack([seg, seg])
    got = _segment_mean(imgs, segs, S).cpu().numpy()
    for b in range(2):
        want = np.array([[np.mean(imgs[b][segs[b] == s][:, c]) for c in range(img.shape[2])] for s in range(S)]).astype(np.uint8)
        assert np.array_equal(got[b], want)
    assert (np.bincount(seg.ravel()) == 1).any() or case == "grid"


# ---- 3. the fit alone ----------------------------------------------------------------------------------------------------------------
def _fit(Z, P, labels, used, alpha, kw=0.25):
    args = (PG.dev(Z), PG.dev(P), PG.dev(labels), None if used is None else PG.dev(used))
    out = X._lime_fit(*args, alpha, kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _compare_fit(Z, P, labels, used, alpha, got, what):
    coef, icpt, score, pred, wts = got
    worst = dict(coef=0.0, intercept=0.0, score=0.0, local_pred=0.0, cond=0.0)
    for b in range(Z.shape[0]):
        w = R.kernel(R.distances(Z[b].astype(np.int64)))
        assert np.abs(wts[b] - w).max() < 1e-12
        cols = np.arange(Z.shape[2]) if used is None else used[b]
        data = Z[b][:, cols].astype(np.float64)
        cond = np.linalg.cond(R.ridge_system(data, w, alpha))
        assert cond < 300, f"{what}: condition number {cond:.0f}: the 1e-9 bound is not derived for it"
        worst["cond"] = max(worst["cond"], cond)
        for l, k in enumerate(labels[b]):
            c_r, i_r, s_r, p_r = R.ridge_sklearn(data, P[b][:, k].astype(np.float64), w, alpha)
            worst["coef"] = max(worst["coef"], np.abs(coef[b, l] - c_r).max() / np.abs(c_r).max())
            worst["intercept"] = max(worst["intercept"], abs(icpt[b, l] - i_r))
            worst["score"] = max(worst["score"], abs(score[b, l] - s_r))
            worst["local_pred"] = max(worst["local_pred"], abs(pred[b, l] - p_r))
    print(f"lime fit {what}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst["coef"], worst["intercept"], worst["score"], worst["local_pred"]) < TOL
    return worst


def _random_problem(B, N, S, K, seed):
    rs = np.random.RandomState(seed)
    Z = np.stack([R.draw_masks(N, S, rs) for _ in range(B)]).astype(np.uint8)
    P = rs.rand(B, N, K).astype(np.float32)
    return Z, P


@pytest.mark.parametrize("N,S,K,alpha", [(100, 48, 6, 1.0), (1000, 192, 6, 1.0), (300, 300, 2, 1.0), (64, 1, 6, 1.0), (64, 1024, 6, 1.0),
                                         (100, 48, 6, 0.01), (1000, 192, 6, 0.01), (200, 50, 6, 0.01)])
def test_fit_against_sklearn_ridge(N, S, K, alpha):
    B = 2 if S <= 300 else 1
    Z, P = _random_problem(B, N, S, K, 1000 * S + N)
    labels = np.stack([np.random.RandomState(b).permutation(K)[:min(K, 5)] for b in range(B)]).astype(np.int32)
    got = _fit(Z, P, labels, None, alpha)
    _compare_fit(Z, P, labels, None, alpha, got, f"N={N} S={S} K={K} alpha={alpha}")
    again = _fit(Z, P, labels, None, alpha)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two launches give identical bits"


def test_fit_on_a_used_subset():
    Z, P = _random_problem(2, 200, 50, 6, 77)
    used = np.stack([np.random.RandomState(5 + b).permutation(50)[:10] for b in range(2)]).astype(np.int32)
    labels = np.array([[3], [0]], dtype=np.int32)
    got = _fit(Z, P, labels, used, 1.0)
    _compare_fit(Z, P, labels, used, 1.0, got, "N=200 S=50 used=10")
    # 8. the weight map: beta of the pixel's segment, 0 outside the subset
    seg = brainxai.grid_segments(40, 60, 5, 10)
    segs = np.stack([seg, seg[::-1].copy()])
    out = torch.empty(2, 1, 40, 60, dtype=torch.float32, device=DEV)
    coef_d, used_d, segs_d = PG.dev(got[0]), PG.dev(used), PG.dev(segs)
    L.check(L.load().bx_lime_weight_map(PG.p(coef_d), PG.p(used_d), PG.p(segs_d), PG.p(out), 2, 1, 40, 60, 50, 10, PG.stream()), "bx_lime_weight_map")
    torch.cuda.synchronize()
    for b in range(2):
        full = np.zeros(50)
        full[used[b]] = got[0][b, 0]
        assert np.array_equal(out[b, 0].cpu().numpy(), full[segs[b]].astype(np.float32))


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def _models(kind, dt):
    ref, spec = _pair(lambda: O.Spectrogram_Model(6), lambda: brainxai.Spectrogram_Model(6), 21)
    model = spec if kind == "spectrogram" else brainxai.MultimodalModel(brainxai.EEGNet(6, Chans=19, Samples=2000), spec).to(DEV)
    return brainxai.set_compute_dtype(model, dt)


def _assert_explanation(mine, ref, what):
    """mine: LimeExplanation; ref: lime_ref.explain fed the same classifier.  Fit figures against Ridge fed mine's own P."""
    assert np.array_equal(mine.masks, ref.masks)
    P = mine.probs.cpu().numpy()
    assert P.dtype == ref.probs.dtype and np.array_equal(P, ref.probs), f"{what}: P differs, max {np.abs(P - ref.probs).max():.2e}"
    assert mine.top_labels == ref.top_labels
    assert np.abs(mine.weights - ref.weights).max() < 1e-12
    worst = dict(coef=0.0, intercept=0.0, score=0.0, local_pred=0.0)
    for k in ref.local_exp:
        want, got = dict(ref.local_exp[k]), dict(mine.local_exp[k])
        assert sorted(want) == sorted(got)
        big = max(abs(v) for v in want.values())
        worst["coef"] = max(worst["coef"], max(abs(got[f] - want[f]) for f in want) / big)
        worst["intercept"] = max(worst["intercept"], abs(mine.intercept[k] - ref.intercept[k]))
        worst["score"] = max(worst["score"], abs(mine.score[k] - ref.score[k]))
        worst["local_pred"] = max(worst["local_pred"], abs(mine.local_pred[k] - ref.local_pred[k]))
        a = [abs(v) for _, v in ref.local_exp[k]]
        for i, (f, _) in enumerate(ref.local_exp[k]):              # order: wherever the reference's neighbours are clearly apart
            clear = (i == 0 or a[i - 1] - a[i] > 1e-8 * big) and (i == len(a) - 1 or a[i] - a[i + 1] > 1e-8 * big)
            if clear:
                assert mine.local_exp[k][i][0] == f, f"{what}: label {k} position {i}"
    print(f"lime end to end {what}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < TOL


@pytest.mark.parametrize("kind,dt", [("spectrogram", torch.float32), ("multimodal", torch.float32), ("spectrogram", torch.bfloat16)],
                         ids=["spectrogram-fp32", "multimodal-fp32", "spectrogram-bf16"])
def test_end_to_end_against_restatement(kind, dt):
    model = _models(kind, dt)
    img, seg = _u8((64, 96, 3), 3), brainxai.grid_segments(64, 96, 4, 6)
    M, N = 32, 100
    clf = lambda ims: brainxai.predict_fn(ims, model, max_batch=M)
    ref = R.explain(img, seg, clf, num_samples=N, seed=4)
    model.train()
    mine = brainxai.lime_image(model, img, seg, num_samples=N, seed=4, max_batch=M)
    assert model.training
    _assert_explanation(mine, ref, f"{kind} {dt}")
    for k in ref.local_exp:
        cond = np.linalg.cond(R.ridge_system(ref.masks.astype(np.float64), ref.weights, 1.0))
        assert cond < 300
    # explicit labels, a hide colour and feature_selection='none'
    ref2 = R.explain(img, seg, clf, labels=(4, 1), hide_color=0, num_samples=60, seed=1, feature_selection="none")
    mine2 = brainxai.lime_image(model, img, seg, labels=(4, 1), hide_color=0, num_samples=60, seed=1, feature_selection="none", max_batch=M)
    assert mine2.top_labels is None and sorted(mine2.local_exp) == [1, 4]
    _assert_explanation(mine2, ref2, f"{kind} {dt} labels hide_color=0")
    # 8. the heat map is beta of the pixel's segment
    for k in mine.local_exp:
        beta = np.zeros(24)
        for f, v in mine.local_exp[k]:
            beta[f] = v
        hm = mine.heatmap(k)
        assert hm.is_cuda and hm.dtype == torch.float32 and np.array_equal(hm.cpu().numpy(), beta[seg].astype(np.float32))


def test_end_to_end_float_image():
    model = _models("spectrogram", torch.float32)
    img, seg = np.random.default_rng(6).random((64, 96, 3)) * 255.9, brainxai.grid_segments(64, 96, 4, 6)
    clf = lambda ims: brainxai.predict_fn(ims, model, max_batch=32)
    ref = R.explain(img, seg, clf, num_samples=50, seed=2, top_labels=2)
    mine = brainxai.lime_image(model, img, seg, num_samples=50, seed=2, top_labels=2, max_batch=32)
    _assert_explanation(mine, ref, "float image")
    assert mine.image.dtype == np.float64


# ---- 5. highest_weights ----------------------------------------------------------------------------------------------------------------
def test_highest_weights_selects_and_refits_like_the_restatement():
    model = _models("spectrogram", torch.float32)
    img, seg = _u8((64, 96, 3), 12), brainxai.grid_segments(64, 96, 5, 10)
    clf = lambda ims: brainxai.predict_fn(ims, model, max_batch=64)
    kw = dict(num_samples=200, num_features=10, feature_selection="highest_weights", top_labels=2)
    for seed in range(10):                                           # the seed is chosen on the reference side only
        ref = R.explain(img, seg, clf, seed=seed, **kw)
        gaps = []
        for k in ref.top_labels:
            first = np.sort(np.abs(R.Ridge(alpha=0.01, fit_intercept=True).fit(ref.masks, ref.probs[:, k].astype(np.float64),
                                                                              sample_weight=ref.weights).coef_))[::-1]
            gaps.append((first[9] - first[10]) / first[0])
        if min(gaps) > 1e-6:
            break
    else:
        pytest.fail("no seed in 0..9 separates the reference's 10th and 11th |beta| by 1e-6 of the largest")
    print(f"highest_weights: seed {seed}, reference gaps {gaps}")
    mine = brainxai.lime_image(model, img, seg, seed=seed, max_batch=64, **kw)
    for k in ref.top_labels:
        assert sorted(f for f, _ in mine.local_exp[k]) == sorted(int(f) for f in ref.used[k]) and len(mine.local_exp[k]) == 10
    _assert_explanation(mine, ref, "highest_weights")
    hm = mine.heatmap(ref.top_labels[0]).cpu().numpy()
    beta = np.zeros(50)
    for f, v in mine.local_exp[ref.top_labels[0]]:
        beta[f] = v
    assert np.array_equal(hm, beta[seg].astype(np.float32)) and (beta == 0).sum() == 40


# ---- 6. batches, repeatability, max_batch ----------------------------------------------------------------------------------------------
def _same_bits(a, b):
    assert np.array_equal(a.masks, b.masks) and torch.equal(a.probs, b.probs) and np.array_equal(a.weights, b.weights)
    assert a.top_labels == b.top_labels and a.local_exp == b.local_exp
    assert a.intercept == b.intercept and a.score == b.score and a.local_pred == b.local_pred


def test_batch_equals_singles_and_repeats():
    model = _models("spectrogram", torch.float32)
    imgs = np.stack([_u8((64, 96, 3), 30 + b) for b in range(3)])
    seg = brainxai.grid_segments(64, 96, 4, 6)
    segs = np.stack([seg, seg[::-1].copy(), _voronoi(64, 96, 22, 2, 1)])
    assert len({int(s.max()) for s in segs}) == 1
    batch = brainxai.lime_image(model, imgs, segs, num_samples=80, seed=3, max_batch=32)
    assert isinstance(batch, list) and len(batch) == 3
    rs = np.random.RandomState(3)                                    # one stream, image order
    for b in range(3):
        assert np.array_equal(batch[b].masks, R.draw_masks(80, 24, rs))
        single = brainxai.lime_image(model, imgs[b], segs[b], num_samples=80, masks=batch[b].masks, max_batch=32)
        _same_bits(single, batch[b])
    again = brainxai.lime_image(model, imgs, segs, num_samples=80, seed=3, max_batch=32)
    for a, b in zip(batch, again):
        _same_bits(a, b)


def test_max_batch_changes_nothing_beyond_the_forward():
    model = _models("spectrogram", torch.float32)
    img, seg = _u8((64, 96, 3), 3), brainxai.grid_segments(64, 96, 4, 6)
    a = brainxai.lime_image(model, img, seg, num_samples=100, seed=4, max_batch=7)
    b = brainxai.lime_image(model, img, seg, num_samples=100, seed=4, max_batch=256)
    assert np.array_equal(a.masks, b.masks) and a.top_labels == b.top_labels
    dP = float((a.probs - b.probs).abs().max())
    dbeta = max(abs(dict(a.local_exp[k])[f] - v) for k in b.local_exp for f, v in b.local_exp[k])
    print(f"max_batch 7 vs 256: max |dP| {dP:.2e}, max |dbeta| {dbeta:.2e}")
    # beta = A^-1 X^T W y with ||A^-1|| <= 1/alpha = 1 and 0/1 features: |dbeta| <= sum(w) max|dP|; zero when the forward is chunk-independent
    assert dbeta <= a.weights.sum() * dP


# ---- 7. nothing of the training state is touched ---------------------------------------------------------------------------------------
def test_training_state_is_left_alone():
    model = _models("multimodal", torch.float32)
    img, seg = _u8((64, 96, 3), 3), brainxai.grid_segments(64, 96, 4, 6)
    for mode in (True, False):
        model.train(mode)
        brainxai.lime_image(model, img, seg, num_samples=20, max_batch=8)
        assert model.training == mode and all(m.training == mode for m in model.modules())
    assert all(p.grad is None for p in model.parameters()) and all(p.requires_grad for p in model.parameters())
    torch.manual_seed(0)
    net = brainxai.build_multimodal(19, 2000, 3, dropout=0.0).to(DEV)
    opt = brainxai.FlatAdamW(net.parameters(), lr=1e-3)
    try:
        e, s = torch.randn(2, 1, 19, 2000, device=DEV), torch.rand(2, 3, 64, 96, device=DEV)
        y = torch.softmax(torch.randn(2, 6, device=DEV), 1)
        brainxai.KLDivLoss()(net(e, s), y).backward()
        g = opt.flat_g.clone()
        state = copy.deepcopy(net.state_dict())
        brainxai.lime_image(net, img, seg, num_samples=20, max_batch=8)
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_g, g) and float(g.abs().max()) > 0
        assert all(torch.equal(v, net.state_dict()[k]) for k, v in state.items())
    finally:
        ops.clear_grad_views()


# ---- 9. the training loop's LIME tail --------------------------------------------------------------------------------------------------
def test_training_loop_explains_every_nth_epoch(tmp_path):
    """tests/lime_loop_child.py in a process of its own: three training loops capture and drop a dozen multi-branch step graphs, and
    the suite's process later tears an RCCL communicator down with graphs alive on purpose (test_gpu_parity.py) -- a teardown that
    has been sensitive to what was captured beside it.  This file adds no captured graph to that process."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lime_loop_child.py")
    p = subprocess.run([sys.executable, child, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "lime_loop_child: ok" in p.stdout, f"child exit code {p.returncode}"
