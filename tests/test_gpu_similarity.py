"""GPU: brainxai.map_similarity / agreement_matrix / randomization_test and the bx_rank_average / bx_map_corr / bx_topk_overlap /
bx_row_minmax / bx_ssim_rows / bx_param_uniform entry points against the restatement of the definitions (tests/similarity_ref.py):
average ranks, top-k overlaps and parameter draws exactly, the correlations and SSIM against numpy / scipy fp64 under derived bounds,
the stage maps of the randomization test bit for bit against a fresh model loaded with the host restatement's parameters.

Bounds, with u = 2^-53.
Correlation.  A sum of N fp64 terms in any order is within (N - 1) u sum|term| of exact.  Means: |m^ - m| <= N u mean|x| =: d0.  The centred
values fl(x - m^) carry the common shift d0 and one rounding u |d| each; since sum d = 0 exactly, the shift enters the three centred sums
only in second order (N d0^2 = N^2 u^2 (N mean|x|^2), against Sxx of order N var: N^2 u^2 mean^2 / var, far below u for the rows used here,
whose mean^2 / var is at most 3 -- that of ranks 0..N-1, of |normal| rows it is 1.75, of normal rows about 1/N).  The positive sums Sxx, Syy
are then within (N + 4) u of themselves, Sxy within (N + 3) u sum|dx dy| <= (N + 3) u sqrt(Sxx Syy) (Cauchy-Schwarz), and
r = Sxy / sqrt(Sxx Syy) adds half the relative error of each of Sxx, Syy times |r| <= 1 and three roundings (four allowed):
    |r^ - r| <= (N + 3) u + (N + 4) u + 4 u  <=  E_corr(N) = (2 N + 16) u        (1.7e-11 at N = 38000; c = 2 in c N u)
Two results each within E_corr of the exact value differ by at most 2 E_corr: that is what is asserted, against numpy's two-pass fp64 form
and against scipy.stats.spearmanr / pearsonr.
SSIM with data_range=None.  The cells lie in [0, 1] and are formed by the same IEEE operations on both sides.  A moment is a sum of win
products tap * cell along a row and, with two filtered axes, of win products tap * moment down a column; the taps are positive and sum to
1, so every moment lies in [0, 1] and is within (win + 1) u, or (2 win + 2) u, of exact -- at most em = 2 NP u for every window used here
(NP = win^axes >= 3).  vx = c (uxx - ux^2) with c <= 1.5 is then within 3 c em <= 5 em =: ev, likewise vy, vxy.  With A1 = 2 ux uy + C1,
A2 = 2 vxy + C2, B1 = ux^2 + uy^2 + C1 >= C1 = 1e-4, B2 = vx + vy + C2 >= C2 = 9e-4: |dA1|, |dB1| <= 4 em, |dA2|, |dB2| <= 2 ev = 10 em, and
since 0 <= A1 / B1 <= 1 and |A2 / B2| <= 1,
    |dS| <= (|dA1| + |dB1|) / C1 + (|dA2| + |dB2|) / C2 = em (8 / C1 + 20 / C2) = 1.03e5 em     (2.7e-9 at NP = 121, 1.1e-9 at NP = 49)
and the mean over P positions adds (P + 8) u:  E_ssim = 2 NP u (8e4 + 20 / 9e-4) + (P + 8) u.  With a caller's data_range D and raw cells
of magnitude up to M the same holds for the cells divided by D: first moments scale by m = M / D and second moments by m^2, so E_ssim is
multiplied by max(1, m)^2.  Two results each within E_ssim differ by at most 2 E_ssim.
Every compared case is first checked ON THE REFERENCE SIDE to discriminate: with b negated, b permuted and abs flipped the reference
correlation moves by more than 100 bounds, with b shifted by one column and with b's contrast halved the reference SSIM does.  Observed
worst figures are printed by each test (run with -s) and recorded in DESIGN.md section 6."""
import functools
import math

import numpy as np
import pytest
import scipy.stats
import torch

import brainxai
from brainxai import _lib as L
from brainxai import ops
from tests import perturb_gpu as PG
from tests import similarity_ref as R
from tests.perturb_gpu import DEV

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
BX_EUNSUPPORTED = -6
SEED = 0x9E3779B97F4A7C15                           # both key words in use


def e_corr(N):
    return (2 * N + 16) * U


def e_ssim(NP, P, m=1.0):
    return (2 * NP * U * (8 / 1e-4 + 20 / 9e-4) + (P + 8) * U) * max(1.0, m) ** 2


# ---- average ranks --------------------------------------------------------------------------------------------------------------------------
def _rank_rows(N, seed):
    """[3,N]: a row of normals rounded to 1/4 (heavy ties) with NaN, -0.0 and +0.0 planted, an all-equal row, a row of 3 distinct values."""
    rng = np.random.default_rng(seed)
    x = np.empty((3, N), dtype=np.float32)
    x[0] = np.round(rng.standard_normal(N) * 4) / 4
    if N >= 8:
        x[0, ::7] = np.nan
        x[0, 1::5] = -0.0
        x[0, 2::5] = 0.0
    x[1] = 2.5
    x[2] = rng.integers(0, 3, N).astype(np.float32) - 1.0
    return x


def _device_ranks(x, abs):
    lib = L.load()
    Rn, N = x.shape
    xd = PG.dev(x)
    keyed = torch.from_numpy(np.abs(x)).to(DEV) if abs else xd      # bx_rank_desc has no flag: it ranks |x|; bx_rank_average reads x itself
    ranks = torch.empty(Rn, N, dtype=torch.int32, device=DEV)
    nb = lib.bx_rank_desc_workspace(Rn, N)
    ws = torch.empty(nb // 4, dtype=torch.int32, device=DEV)
    L.check(lib.bx_rank_desc(PG.p(keyed), PG.p(ranks), Rn, N, PG.p(ws), nb, PG.stream()), "bx_rank_desc")
    avg = torch.full((Rn, N), float("nan"), dtype=torch.float32, device=DEV)
    nb = lib.bx_rank_average_workspace(Rn, N)
    assert nb == Rn * N * 4
    ws2 = torch.empty(nb // 4, dtype=torch.int32, device=DEV)
    L.check(lib.bx_rank_average(PG.p(xd), PG.p(ranks), PG.p(avg), Rn, N, int(abs), PG.p(ws2), nb, PG.stream()), "bx_rank_average")
    return ranks.cpu().numpy(), avg.cpu().numpy()


@pytest.mark.parametrize("N", [1, 2, 257, 1025, 38000])
def test_average_ranks_equal_rankdata(N):
    x = _rank_rows(N, N)
    for abs in (False, True):
        ranks, avg = _device_ranks(x, abs)
        want = R.average_ranks(x, abs)
        assert np.array_equal(ranks, R.stable_ranks(x, abs))
        assert avg.dtype == np.float32 and np.array_equal(avg.astype(np.float64), want), f"N = {N}, abs = {abs}"
        assert np.array_equal(want[1], np.full(N, (N - 1) / 2)), "an all-equal row has one rank"
    plain = np.random.default_rng(N + 1).standard_normal((3, N)).astype(np.float32)           # (almost) no ties: a row without any has its stable ranks
    ranks, avg = _device_ranks(plain, False)
    assert np.array_equal(avg.astype(np.float64), R.average_ranks(plain))
    untied = [r for r in range(3) if len(np.unique(plain[r])) == N]
    assert np.array_equal(avg[untied], ranks[untied].astype(np.float32))
    xd, rd, ad = PG.dev(x), PG.dev(ranks), PG.dev(avg)                 # a workspace one byte short is refused before a launch
    assert L.load().bx_rank_average(PG.p(xd), PG.p(rd), PG.p(ad), 3, N, 0, PG.p(ad), 3 * N * 4 - 1, PG.stream()) == -4


# ---- correlations ---------------------------------------------------------------------------------------------------------------------------
CORR_N = [2, 24, 760, 4099, 38000]


@functools.lru_cache(maxsize=None)
def _corr_case(N):
    """(a, b) fp32 [3,N] of standard normals, b correlated with a; at N = 2 rows for which |.| changes the sign of r."""
    rng = np.random.default_rng(40 + N)
    if N == 2:
        a = np.array([[-1.5, 0.5], [0.25, -2.0], [-0.75, 0.125]], dtype=np.float32)
        b = np.array([[0.5, 1.25], [-1.0, 1.5], [1.5, 2.5]], dtype=np.float32)
        return a, b
    a = rng.standard_normal((3, N)).astype(np.float32)
    b = (0.6 * a + 0.8 * rng.standard_normal((3, N))).astype(np.float32)
    return a, b


def _corr_device(a, b, abs):
    out = torch.full((a.shape[0],), 7.0, dtype=torch.float64, device=DEV)
    ad, bd = PG.dev(a), PG.dev(b)
    L.check(L.load().bx_map_corr(PG.p(ad), PG.p(bd), PG.p(out), a.shape[0], a.shape[1], int(abs), PG.stream()), "bx_map_corr")
    return out.cpu().numpy()


@pytest.mark.parametrize("N", CORR_N)
def test_map_corr_against_fp64_numpy(N):
    """|bx_map_corr - numpy two-pass fp64| <= 2 E_corr(N), abs on and off; a constant row is NaN on both sides; N = 2 gives +-1."""
    a, b = _corr_case(N)
    tol = 2 * e_corr(N)
    worst = 0.0
    for abs in (False, True):
        ref = R.corr(a, b, abs)
        moved = [np.abs(R.corr(a, np.roll(b, 1, axis=1), abs) - ref), np.abs(R.corr(a, b, not abs) - ref)]
        if not abs:                                     # |b| does not see b's sign
            moved.append(np.abs(R.corr(a, -b) - ref))
        assert np.min(moved) > 100 * tol, f"N = {N}, abs = {abs}: the reference moves by {np.min(moved):.1e} only"
        got = _corr_device(a, b, abs)
        err = np.abs(got - ref).max()
        worst = max(worst, err)
        assert err <= tol, f"N = {N}, abs = {abs}: {err:.2e} > {tol:.2e}"
        assert np.abs(got - R.pearson(a, b, abs)).max() <= tol
        if N == 2:
            assert np.array_equal(np.abs(ref), np.ones(3)) and np.array_equal(np.sign(got), ref) and np.abs(np.abs(got) - 1.0).max() <= tol
    print(f"bx_map_corr N = {N}: worst |r - numpy| = {worst:.2e}, bound 2 E = {tol:.2e}")
    const = a.copy()
    const[1] = 0.75
    got, ref = _corr_device(const, b, False), R.corr(const, b)
    assert np.isnan(got[1]) and np.isnan(ref[1]) and np.abs(got[[0, 2]] - ref[[0, 2]]).max() <= tol
    assert np.isnan(_corr_device(b, const, True)[1])


@pytest.mark.parametrize("N", [257, 38000])
def test_spearman_against_scipy_on_tied_data(N):
    rng = np.random.default_rng(N)
    a = (np.round(rng.standard_normal((3, N)) * 4) / 4).astype(np.float32)
    b = (np.round((0.6 * a + 0.8 * rng.standard_normal((3, N))) * 4) / 4).astype(np.float32)
    tol = 2 * e_corr(N)
    for abs in (False, True):
        ref = R.spearman(a, b, abs)
        assert np.abs(R.spearman(a, -b, abs) - ref).min() > 100 * tol or abs
        assert np.abs(R.spearman(a, np.roll(b, 1, axis=1), abs) - ref).min() > 100 * tol
        got = brainxai.map_similarity(PG.dev(a).reshape(3, 1, N), PG.dev(b).reshape(3, 1, N), metrics=("spearman",), abs=abs, return_parts=True)
        assert np.array_equal(got.ranks_a.cpu().numpy().reshape(3, N).astype(np.float64), R.average_ranks(a, abs))
        rho = got.spearman.cpu().numpy()
        want = np.array([scipy.stats.spearmanr(np.abs(p) if abs else p, np.abs(q) if abs else q).statistic for p, q in zip(a, b)])
        err = max(np.abs(rho - ref).max(), np.abs(rho - want).max())
        print(f"spearman N = {N} abs = {abs}: worst |rho - scipy| = {err:.2e}, bound 2 E = {tol:.2e}")
        assert err <= tol


# ---- top-k overlap --------------------------------------------------------------------------------------------------------------------------
def test_topk_overlap_is_exact():
    N, k = 400, 40
    rng = np.random.default_rng(9)
    a = rng.permutation(N).astype(np.float32)[None].repeat(3, 0)
    for r in range(3):
        a[r] = rng.permutation(N)
    b = a.copy()
    for r in range(3):                                 # half of a's top cells leave b's top, as many others enter it: exactly k / 2 are shared
        top = np.argsort(-a[r], kind="stable")
        b[r, top[:k // 2]] = -10.0 - np.arange(k // 2)
        b[r, top[k:k + k // 2]] = 1000.0 + np.arange(k // 2)
    assert k == R.topk_count(0.1, N) and np.array_equal(R.topk_overlap(a, b, k), np.full(3, 0.5))
    tied = (np.round(rng.standard_normal((3, N)) * 2) / 2).astype(np.float32)       # ties across the cut: the stable order decides
    lib = L.load()
    for x, y in ((a, b), (tied, np.roll(tied, 3, axis=1)), (tied, tied)):
        ra, rb = (PG.dev(R.stable_ranks(v).astype(np.int32)) for v in (x, y))
        for kk in (1, N, k):
            out = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
            L.check(lib.bx_topk_overlap(PG.p(ra), PG.p(rb), PG.p(out), 3, N, kk, PG.stream()), "bx_topk_overlap")
            assert np.array_equal(out.cpu().numpy(), R.topk_overlap(x, y, kk)), kk
    got = brainxai.map_similarity(PG.dev(a).reshape(3, 20, 20), PG.dev(b).reshape(3, 20, 20), metrics=("topk",), topk=0.1, return_parts=True)
    assert got.k == k and np.array_equal(got.topk.cpu().numpy(), np.full(3, 0.5))


# ---- SSIM -----------------------------------------------------------------------------------------------------------------------------------
# name -> (H, W, window, win_size, data_range, abs, what is special)
SSIM_CASES = {
    "uniform 7x7": (7, 7, "uniform", None, None, False, None), "uniform 7x8": (7, 8, "uniform", None, None, False, None),
    "uniform 9x23": (9, 23, "uniform", None, None, False, None), "uniform 19x40": (19, 40, "uniform", None, None, False, None),
    "uniform line 1x64": (1, 64, "uniform", None, None, False, None), "uniform column 40x1": (40, 1, "uniform", None, None, False, None),
    "win3 3x3": (3, 3, "uniform", 3, None, False, None), "win3 5x4": (5, 4, "uniform", 3, None, False, None),
    "gaussian 11x11": (11, 11, "gaussian", None, None, False, None), "gaussian 13x37": (13, 37, "gaussian", None, None, False, None),
    "strip exactly 19x70": (19, 70, "uniform", None, None, False, None), "strip plus one 19x71": (19, 71, "uniform", None, None, False, None),
    "largest 406x9": (406, 9, "uniform", None, None, False, None),
    "constant side 9x23": (9, 23, "uniform", None, None, False, "constant"), "data_range 2 9x23": (9, 23, "uniform", None, 2.0, False, None),
    "abs 9x23": (9, 23, "uniform", None, None, True, None), "abs data_range gaussian 13x37": (13, 37, "gaussian", None, 2.0, True, None),
}


@pytest.mark.parametrize("name", sorted(SSIM_CASES))
def test_ssim_rows_against_fp64_restatement(name):
    """|mean SSIM - restatement| <= 2 E_ssim through map_similarity (bx_row_minmax + bx_ssim_rows); ssim(a, a) within E_ssim of 1."""
    H, W, window, win_size, data_range, abs, special = SSIM_CASES[name]
    rng = np.random.default_rng(sorted(SSIM_CASES).index(name))
    a = rng.standard_normal((3, H, W)).astype(np.float32)
    b = (0.7 * a + 0.5 * rng.standard_normal((3, H, W))).astype(np.float32)
    if special == "constant":
        b[1] = -3.0
    win = 11 if window == "gaussian" else (win_size or 7)
    axes = (H > 1) + (W > 1)
    P = (H - win + 1 if H > 1 else 1) * (W - win + 1 if W > 1 else 1)
    m = 1.0 if data_range is None else float(np.abs(np.concatenate([a.ravel(), b.ravel()])).max()) / data_range
    tol = 2 * e_ssim(win ** axes, P, m)
    strip = L.load().bx_ssim_strip(H, W, win)
    if name.startswith("strip"):
        assert strip == 64 and (W - win + 1) - strip == (0 if "exactly" in name else 1)
    kw = dict(metrics=("ssim",), window=window, win_size=win_size, data_range=data_range, abs=abs)
    ref = R.ssim(a, b, window, win_size, data_range, abs)
    if special is None and min(H, W) != 3:              # the reference discriminates (a 3x3 map is one window: a shift leaves nothing to compare)
        shifted = np.roll(b, 1, axis=2 if W > 1 else 1)
        halved = (0.5 * b).astype(np.float32)
        moved = [np.abs(R.ssim(a, shifted, window, win_size, data_range, abs) - ref).min()]
        if data_range is not None:                      # with data_range=None a map is rescaled by its own extremes: its contrast cannot matter
            moved.append(np.abs(R.ssim(a, halved, window, win_size, data_range, abs) - ref).min())
        else:
            assert np.abs(R.ssim(a, halved, window, win_size, None, abs) - ref).max() < 1e-12
        assert min(moved) > 100 * tol, f"{name}: the reference moves by {min(moved):.1e} only"
    res = brainxai.map_similarity(PG.dev(a), PG.dev(b), return_parts=True, **kw)
    got = res.ssim.cpu().numpy()
    err = np.abs(got - ref).max()
    print(f"ssim {name}: strip {strip}, worst |ssim - restatement| = {err:.2e}, bound 2 E = {tol:.2e}, values {np.round(ref, 4)}")
    assert got.shape == (3,) and err <= tol, f"{name}: {err:.2e} > {tol:.2e}"
    if data_range is None:
        v = np.abs(a) if abs else a
        assert np.array_equal(res.lo.cpu().numpy()[0], v.min((1, 2))) and np.array_equal(res.hi.cpu().numpy()[0], v.max((1, 2)))
    else:
        assert res.lo is None
    same = brainxai.map_similarity(PG.dev(a), PG.dev(a), **kw).ssim.cpu().numpy()
    assert np.abs(same - 1.0).max() <= tol / 2, f"{name}: ssim(a, a) = {same}"


def test_ssim_rows_past_the_largest_map_is_refused():
    lib = L.load()
    a = torch.zeros(1, 407, 9, device=DEV)
    taps = torch.full((7,), 1 / 7, dtype=torch.float64, device=DEV)
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    rc = lib.bx_ssim_rows(PG.p(a), PG.p(a), PG.p(taps), None, None, None, None, 1.0, 49 / 48, PG.p(out), 1, 407, 9, 7, 0, PG.p(ws), 512, PG.stream())
    assert rc == BX_EUNSUPPORTED and b"H = 407 rows" in lib.bx_last_error_string()
    assert lib.bx_ssim_strip(406, 9, 7) == 4 and lib.bx_ssim_strip(407, 9, 7) == 0
    with pytest.raises(ValueError, match="at most 406 rows"):
        brainxai.map_similarity(a, a, metrics=("ssim",))
    torch.cuda.synchronize()
    assert float(out) == 0.0


# ---- parameter draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_param_uniform_bit_for_bit(n):
    lib = L.load()
    bound = 1.0 / math.sqrt(27.0)
    streams = {}
    for j, s in ((0, 0), (3, 5), (5, 3)):
        for aligned in (True, False):
            buf = torch.full((n + 9,), float("nan"), dtype=torch.float32, device=DEV)
            view = buf[4:4 + n] if aligned else buf[1:1 + n]
            assert (view.data_ptr() % 16 == 0) == aligned
            L.check(lib.bx_param_uniform(view.data_ptr(), n, bound, SEED, j, s, PG.stream()), "bx_param_uniform")
            got = buf.cpu().numpy()
            lo = 4 if aligned else 1
            want = R.param_uniform(n, bound, SEED, j, s)
            assert np.array_equal(PG.np_bits(got[lo:lo + n]), PG.np_bits(want)), (n, j, s, aligned)
            assert np.isnan(got[:lo]).all() and np.isnan(got[lo + n:]).all(), "nothing outside the tensor is written"
            assert (np.abs(want) <= np.float32(bound)).all()
        streams[(j, s)] = want
    if n >= 4:
        assert not np.array_equal(streams[(0, 0)], streams[(3, 5)]) and not np.array_equal(streams[(3, 5)], streams[(5, 3)])
    assert not np.array_equal(R.param_uniform(n, bound, SEED & 0xFFFFFFFF, 0, 0), streams[(0, 0)]), "the high key word is in use"
    assert not np.array_equal(R.param_uniform(n, bound, SEED >> 32 << 32, 0, 0), streams[(0, 0)]), "the low key word is in use"


# ---- map_similarity end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 24), (2, 4, 16, 24), (3, 1, 64)], ids=["B,H,W", "B,K,H,W", "B,1,T"])
@pytest.mark.parametrize("abs", [False, True], ids=["signed", "abs"])
def test_map_similarity_end_to_end(shape, abs):
    rng = np.random.default_rng(len(shape) * 10 + shape[-1])
    a = (np.round(rng.standard_normal(shape) * 8) / 8).astype(np.float32)            # some ties
    b = (np.round((0.7 * a + 0.6 * rng.standard_normal(shape)) * 8) / 8).astype(np.float32)
    H, W = shape[-2:]
    N = H * W
    fa, fb = a.reshape(-1, N), b.reshape(-1, N)
    res = brainxai.map_similarity(PG.dev(a), PG.dev(b), abs=abs, topk=0.25, return_parts=True)
    lead = shape[:-2]
    for m in ("spearman", "pearson", "ssim", "topk"):
        assert getattr(res, m).shape == lead and getattr(res, m).dtype == torch.float64
    tc = 2 * e_corr(N)
    assert np.abs(res.pearson.cpu().numpy().ravel() - R.corr(fa, fb, abs)).max() <= tc
    assert np.abs(res.spearman.cpu().numpy().ravel() - R.spearman(fa, fb, abs)).max() <= tc
    assert res.k == math.ceil(0.25 * N) and np.array_equal(res.topk.cpu().numpy().ravel(), R.topk_overlap(fa, fb, res.k, abs))
    axes = (H > 1) + (W > 1)
    P = (H - 6 if H > 1 else 1) * (W - 6)
    assert np.abs(res.ssim.cpu().numpy().ravel() - R.ssim(a.reshape(-1, H, W), b.reshape(-1, H, W), abs=abs)).max() <= 2 * e_ssim(7 ** axes, P)
    assert res.ranks_a.shape == shape and np.array_equal(res.ranks_b.cpu().numpy().reshape(-1, N).astype(np.float64), R.average_ranks(fb, abs))
    assert res.lo.shape == (2, *lead) and res.args["win_size"] == 7
    only = brainxai.map_similarity(PG.dev(a), PG.dev(b), abs=abs, metrics="pearson")
    assert only.spearman is None and only.ranks_a is None and torch.equal(only.pearson, res.pearson)


def test_agreement_matrix():
    rng = np.random.default_rng(77)
    base = rng.standard_normal((2, 16, 24)).astype(np.float32)
    maps = {"cam": PG.dev(base), "saliency": PG.dev((base + 0.5 * rng.standard_normal(base.shape)).astype(np.float32)),
            "rise": PG.dev(rng.standard_normal(base.shape).astype(np.float32))}
    for metric in ("spearman", "pearson", "ssim", "topk"):
        mat, names = brainxai.agreement_matrix(maps, metric=metric, abs=True)
        assert names == ["cam", "saliency", "rise"] and mat.shape == (3, 3, 2) and mat.dtype == torch.float64
        assert torch.equal(mat, mat.transpose(0, 1)) and torch.equal(mat[[0, 1, 2], [0, 1, 2]], torch.ones(3, 2, dtype=torch.float64, device=DEV))
        for i in range(3):
            for j in range(3):
                if i != j:
                    pair = getattr(brainxai.map_similarity(maps[names[i]], maps[names[j]], metrics=(metric,), abs=True), metric)
                    assert torch.equal(mat[i, j], pair), (metric, i, j)
    assert float(brainxai.agreement_matrix(maps)[0][0, 1].min()) > 0.5 > float(brainxai.agreement_matrix(maps)[0][0, 2].abs().max())


# ---- the randomization test -----------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    """Equal shapes and equal bytes: tells -0.0 from 0.0 and compares NaNs."""
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _assert_restored(model, before, what):
    after = model.state_dict()
    assert list(after) == list(before)
    for k, v in after.items():
        assert v.dtype == before[k].dtype and _same_bits(v, before[k]), f"{what}: {k} not restored"


def _fresh_multimodal(sd):
    net = brainxai.build_multimodal(19, 2000, 4, dropout=0.0)
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def _fresh_eegnet(sd):
    net = brainxai.EEGNet(6, Chans=19, Samples=2000)
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def _cam(m, e, s):
    return brainxai.grad_cam(m, e, s, "spectrogram_model.block5", relu=False)       # the rectified map of this model is all zeros: nothing to rank


def _sal(m, e, s):
    return brainxai.saliency(m, e, s)[1]


def _eeg_cam(m, e, s):
    return brainxai.grad_cam(m, e, None, "separableConv")


def _check_stage_maps(res, model, fresh, explain, eeg, spec, stages):
    for s in stages:
        twin = fresh(R.reinit_state_dict(model, res.layers, res.seed, res.order, s))
        want = explain(twin, eeg, spec)
        assert torch.equal(PG.bits(res.maps[s]), PG.bits(want)), f"{res.order}: the map of stage {s} ({res.layers[s]}) differs from a fresh model with the restated parameters"


def _check_similarity(res, **kw):
    for s, phi in enumerate(res.maps):
        pair = brainxai.map_similarity(res.original, phi, metrics=tuple(res.similarity), **kw)
        for m, v in res.similarity.items():
            assert v.shape == (*res.original.shape[:-2], len(res.layers)) and _same_bits(v[..., s], getattr(pair, m)), (m, s)


def test_randomization_multimodal_grad_cam():
    """Both orders on the default spectrogram cascade, inside a pack_reuse scope opened before the calls and beside a GradCamSweep built
    before them: the stale-pack cases.  Restored, stage maps, shared first stage, similarity values, the other branch untouched."""
    _, model = PG.scaled_multimodal()
    eeg, spec = (PG.dev(t) for t in PG.mm_inputs())
    before = _state(model)
    sweep = brainxai.GradCamSweep(model, eeg, spec, class_idx=None, relu=False)
    swept = sweep(eeg, spec).clone()
    eeg_params = [q for n, q in model.named_parameters() if n.startswith("eeg_model")] + [q for n, q in model.named_buffers() if n.startswith("eeg_model")]
    sums = []

    def explain(m, e, s):
        sums.append(torch.stack([q.double().sum() for q in eeg_params]))
        return _cam(m, e, s)
    layers = brainxai.randomization_layers(model, "spec")
    assert len(layers) == 8
    with ops.pack_reuse():
        phi0 = _cam(model, eeg, spec).clone()
        assert float(phi0.flatten(1).std(1).min()) > 0 and torch.equal(PG.bits(swept), PG.bits(phi0))
        casc = brainxai.randomization_test(model, explain, eeg, spec, seed=SEED, keep_maps=True, metrics=("spearman", "ssim", "pearson", "topk"), abs=True)
        assert torch.equal(PG.bits(_cam(model, eeg, spec)), PG.bits(phi0)), "stale packed weights after the restore"
        ind = brainxai.randomization_test(model, explain, eeg, spec, order="independent", seed=SEED, keep_maps=True)
        assert torch.equal(PG.bits(_cam(model, eeg, spec)), PG.bits(phi0))
    _assert_restored(model, before, "multimodal grad_cam")
    assert torch.equal(PG.bits(sweep(eeg, spec)), PG.bits(swept)), "the sweep replays stale packed weights"
    assert torch.equal(PG.bits(_cam(model, eeg, spec)), PG.bits(phi0))
    sums = torch.stack(sums).cpu()
    assert len(sums) == 18 and torch.equal(sums, sums[:1].expand_as(sums)), "input='spec' wrote the EEG branch"
    for res, order in ((casc, "cascade"), (ind, "independent")):
        assert res.layers == layers and res.order == order and res.seed == SEED and len(res.maps) == 8
        assert torch.equal(PG.bits(res.original), PG.bits(phi0)) and res.original.shape == (3, 64, 128)
        _check_stage_maps(res, model, _fresh_multimodal, _cam, eeg, spec, (0, 2, 7))
    assert torch.equal(PG.bits(casc.maps[0]), PG.bits(ind.maps[0])), "stage 0 of the two orders is the same model"
    assert not torch.equal(casc.maps[2], ind.maps[2])
    _check_similarity(casc, abs=True)
    _check_similarity(ind)
    assert set(casc.similarity) == {"spearman", "ssim", "pearson", "topk"} and set(ind.similarity) == {"spearman", "ssim"}
    for res in (casc, ind):
        for m, v in res.similarity.items():
            print(f"randomization grad_cam block5 {res.order} {m}: " + " ".join(f"{x:.3f}" for x in v.nanmean(0).tolist()))


def test_randomization_restores_when_explain_raises():
    _, model = PG.scaled_multimodal()
    eeg, spec = (PG.dev(t) for t in PG.mm_inputs())
    before = _state(model)
    phi0 = _cam(model, eeg, spec).clone()
    calls = []

    def explain(m, e, s):
        calls.append(1)
        if len(calls) == 4:                               # the clean call, stages 0 and 1, then stage 2
            raise FloatingPointError("stage 2")
        return _cam(m, e, s)
    with ops.pack_reuse():
        with pytest.raises(FloatingPointError, match="stage 2"):
            brainxai.randomization_test(model, explain, eeg, spec, seed=1)
        assert len(calls) == 4
        assert torch.equal(PG.bits(_cam(model, eeg, spec)), PG.bits(phi0))
    _assert_restored(model, before, "explain raised")


def test_randomization_multimodal_saliency():
    _, model = PG.scaled_multimodal()
    eeg, spec = (PG.dev(t) for t in PG.mm_inputs())
    before = _state(model)
    phi0 = _sal(model, eeg, spec).clone()
    res = brainxai.randomization_test(model, _sal, eeg, spec, seed=3, keep_maps=True, layers=["fc2", "spectrogram_model.fc", ("spectrogram_model.block5", "spectrogram_model.block4"),
                                                                                                 "spectrogram_model.block1"])
    _assert_restored(model, before, "multimodal saliency")
    assert torch.equal(PG.bits(_sal(model, eeg, spec)), PG.bits(phi0)) and torch.equal(PG.bits(res.original), PG.bits(phi0))
    assert res.layers[2] == ("spectrogram_model.block5", "spectrogram_model.block4")
    _check_stage_maps(res, model, _fresh_multimodal, _sal, eeg, spec, (0, 2, 3))
    _check_similarity(res)
    for m, v in res.similarity.items():
        print(f"randomization saliency cascade {m}: " + " ".join(f"{x:.3f}" for x in v.nanmean(0).tolist()))


@pytest.mark.parametrize("order", ["cascade", "independent"])
def test_randomization_eegnet_grad_cam(order):
    _, model = PG.eegnet_pair()
    eeg = PG.dev(PG.mm_inputs()[0])
    before = _state(model)
    phi0 = _eeg_cam(model, eeg, None).clone()
    res = brainxai.randomization_test(model, _eeg_cam, eeg, None, input="eeg", order=order, seed=SEED, keep_maps=True)
    _assert_restored(model, before, "eegnet grad_cam")
    assert torch.equal(PG.bits(_eeg_cam(model, eeg, None)), PG.bits(phi0))
    assert res.layers == ["dense", ("separableConv", "batchnorm3"), ("depthwiseConv", "batchnorm2"), ("conv1", "batchnorm1")] and res.original.shape == (3, 1, 2000)
    _check_stage_maps(res, model, _fresh_eegnet, _eeg_cam, eeg, None, (0, 2, 3))
    _check_similarity(res)
    for m, v in res.similarity.items():
        print(f"randomization eegnet grad_cam separableConv {order} {m}: " + " ".join(f"{x:.3f}" for x in v.nanmean(0).tolist()))
