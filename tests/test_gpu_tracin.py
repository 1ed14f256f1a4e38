"""GPU: TracIn -- bx_tracin_factors, bx_tracin_scores, bx_tracin_self and bx_tracin_topk through ctypes, and ``tracin`` /
``self_influence`` end to end, against the numpy fp64 restatement (tests/tracin_ref.py).

Everything the library computes is compared bit for bit: the definition (include/brainxai.h, "TracIn") fixes every operation and its
order, its exp and log included, and the reference restates them one numpy operation each.  The selection is exact.
The one bound is that of the independent route of the end-to-end test: the same scores from ``torch.autograd`` through the product
model, per example (KLDivLoss('sum') backwarded, the four layers' .grad dotted in fp64).  That route is fp32.  Its own rounding is
measured first -- an fp32 CPU-torch restatement of the four layers on the downloaded activations against the fp64 reference, relative
to |g_i|_2 |g_j|_2 -- and the product model's route is allowed 8 x that (the margin covers bx_mm_head_bwd's different summation orders).
Both figures are printed (-s) and recorded in DESIGN.md section 6, TracIn.

Shapes.  Factors: rows in {1, 5, 67}, (K, Hd) in {(1,2), (6,128), (32,256)}, both modes, distributions with zeros and integer labels,
hidden rows with exact zeros.  Scores and self: (block rows, M) in {(1,1), (33,5), (130,65)} -- partial and several 64-row tiles on both
axes -- at widths (K, Hd, C, F) in {(1,2,1,1), (6,128,256,992), (5,33,1024,4096)} (one feature, a whole number of 32-feature chunks,
partial chunks and the limits).  Top-k: N in {1, 5, 257, 70001} (one and several sweeps of 256 threads, several 32-row key tiles), M in
{1, 3, 65}, k in {1, 3, 256}."""
import ctypes as C

import numpy as np
import pytest
import torch

import brainxai
from brainxai import _lib as L
from brainxai import explain as X
from tests import perturb_gpu as PG
from tests import tracin_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [(1, 2, 1, 1), (6, 128, 256, 992), (5, 33, 1024, 4096)]
BLOCKS = [(1, 1), (33, 5), (130, 65)]


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    bad = np.flatnonzero(PG.np_bits(got).ravel() != PG.np_bits(np.ascontiguousarray(want, dtype=got.dtype)).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} against {want.ravel()[bad[0]]!r}"


def _widths(K, Hd, Cc, F):
    return (K, Hd, K, K), (Hd, 2 * K, F, Cc)


def _shape(dw, aw):
    sh = L.TracinShape()
    sh.layers = len(dw)
    for l in range(len(dw)):
        sh.dwidth[l], sh.awidth[l] = dw[l], aw[l]
    return sh


def _side(delta, acts, rows=None):
    s = L.TracinSide()
    s.delta, s.rows = PG.p(delta), int(delta.shape[0]) if rows is None else rows
    for l, a in enumerate(acts):
        s.act[l] = PG.p(a)
    return s


def _rand_side(n, dw, aw, seed):
    rng = np.random.default_rng(seed)
    delta = rng.standard_normal((n, sum(dw)))
    acts = [rng.standard_normal((n, w)).astype(np.float32) for w in aw]
    delta[::3, ::5] = 0.0
    return (delta, acts), (PG.dev(delta), [PG.dev(a) for a in acts])


def _scores(train, test, dw, aw, S, row0, eta, store, mask):
    L.check(L.load().bx_tracin_scores(C.byref(_side(*train)), C.byref(_side(*test)), C.byref(_shape(dw, aw)), PG.p(S), int(S.shape[0]), row0, eta, store, mask,
                                      PG.stream()), "bx_tracin_scores")


def _self(side, dw, aw, out, row0, eta, store, mask):
    L.check(L.load().bx_tracin_self(C.byref(_side(*side)), C.byref(_shape(dw, aw)), PG.p(out), int(out.shape[0]), row0, eta, store, mask, PG.stream()),
            "bx_tracin_self")


# ---- factors --------------------------------------------------------------------------------------------------------------------------
def _factor_inputs(rows, K, Hd, seed):
    g = torch.Generator().manual_seed(seed)
    lsm = lambda: torch.log_softmax(2.0 * torch.randn(rows, K, generator=g), dim=1)
    logp, e, s = lsm(), lsm(), lsm()
    hidden = torch.relu(torch.randn(rows, Hd, generator=g))                 # about half of every row is exactly zero
    w1, w2 = 0.3 * torch.randn(Hd, 2 * K, generator=g), 0.3 * torch.randn(K, Hd, generator=g)
    t = torch.rand(rows, K, generator=g)
    t[torch.rand(rows, K, generator=g) < 0.3] = 0.0
    t[:, -1] += 0.05
    t = t / t.sum(dim=1, keepdim=True) * (0.5 + torch.rand(rows, 1, generator=g))            # T != 1
    labels = torch.randint(0, K, (rows,), generator=g, dtype=torch.int32)
    return logp, e, s, hidden, w1, w2, t.contiguous(), labels


def _factors(logp, target, hidden, e, s, w1, w2, mode):
    rows, K = logp.shape
    Hd = int(hidden.shape[1]) if mode == L.BX_TRACIN_MULTIMODAL else 0
    d = {k: PG.dev(v) for k, v in dict(logp=logp, target=target, hidden=hidden, e=e, s=s, w1=w1, w2=w2).items()}
    dist = target.dtype == torch.float32
    delta = torch.full((rows, 3 * K + Hd if mode == L.BX_TRACIN_MULTIMODAL else K), float("nan"), dtype=torch.float64, device=PG.DEV)
    loss = torch.full((rows,), float("nan"), dtype=torch.float64, device=PG.DEV)
    status = torch.full((rows,), -1, dtype=torch.int32, device=PG.DEV)
    multi = mode == L.BX_TRACIN_MULTIMODAL
    L.check(L.load().bx_tracin_factors(PG.p(d["logp"]), PG.p(d["target"]) if dist else None, None if dist else PG.p(d["target"]),
                                       PG.p(d["hidden"]) if multi else None, PG.p(d["e"]) if multi else None, PG.p(d["s"]) if multi else None,
                                       PG.p(d["w1"]) if multi else None, PG.p(d["w2"]) if multi else None, PG.p(delta), PG.p(loss), PG.p(status), rows, K, Hd,
                                       mode, PG.stream()), "bx_tracin_factors")
    torch.cuda.synchronize()
    return delta, loss, status


@pytest.mark.parametrize("K,Hd", [(1, 2), (6, 128), (32, 256)])
@pytest.mark.parametrize("rows", [1, 5, 67])
def test_factors_bit_for_bit(rows, K, Hd):
    logp, e, s, hidden, w1, w2, t, labels = _factor_inputs(rows, K, Hd, 10 * rows + K)
    assert (hidden == 0).any() and (K == 1 or (t == 0).any() or rows == 1)
    for target in (t, labels):
        kind = "distributions" if target is t else "labels"
        delta, loss, status = _factors(logp, target, hidden, e, s, w1, w2, L.BX_TRACIN_MULTIMODAL)
        want_d, want_l = R.factors_multimodal(logp.numpy(), target.numpy(), hidden.numpy(), e.numpy(), s.numpy(), w1.numpy(), w2.numpy())
        _same(delta, want_d, f"multimodal factors, {kind}")
        _same(loss, want_l, f"multimodal loss, {kind}")
        assert not status.any()
        delta, loss, status = _factors(logp, target, hidden, e, s, w1, w2, L.BX_TRACIN_SINGLE)
        want_d, want_l = R.factors_single(logp.numpy(), target.numpy())
        _same(delta, want_d, f"single-layer factors, {kind}")
        _same(loss, want_l, f"single-layer loss, {kind}")
        assert not status.any()
    if K > 1:
        assert np.abs(want_d).max() > 1e-3                                   # the factors are not all zero


def test_factors_status_rows():
    logp, e, s, hidden, w1, w2, t, labels = _factor_inputs(9, 6, 128, 3)
    logp, t, labels = logp.clone(), t.clone(), labels.clone()
    logp[2, 4] = float("nan")
    t[5, 1] = -0.25
    t[7] = 0.0
    for mode in (L.BX_TRACIN_MULTIMODAL, L.BX_TRACIN_SINGLE):
        delta, loss, status = _factors(logp, t, hidden, e, s, w1, w2, mode)
        assert status.cpu().tolist() == [0, 0, L.BX_TRACIN_NONFINITE, 0, 0, L.BX_TRACIN_BAD_TARGET, 0, L.BX_TRACIN_BAD_TARGET, 0]
        keep = [0, 1, 3, 4, 6, 8]
        want = R.factors_multimodal(logp.numpy()[keep], t.numpy()[keep], hidden.numpy()[keep], e.numpy()[keep], s.numpy()[keep], w1.numpy(), w2.numpy()) \
            if mode == L.BX_TRACIN_MULTIMODAL else R.factors_single(logp.numpy()[keep], t.numpy()[keep])
        _same(delta[keep], want[0], "the factors of the rows beside the flagged ones")
        _same(loss[keep], want[1], "their losses")
    labels[3] = 6
    assert _factors(logp, labels, hidden, e, s, w1, w2, L.BX_TRACIN_SINGLE)[2].cpu().tolist() == [0, 0, 1, 2, 0, 0, 0, 0, 0]


# ---- scores and self ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Hd,Cc,F", WIDTHS)
@pytest.mark.parametrize("rows,M", BLOCKS)
def test_scores_and_self_bit_for_bit(rows, M, K, Hd, Cc, F):
    dw, aw = _widths(K, Hd, Cc, F)
    (tr_h, tr_d), (te_h, te_d) = _rand_side(rows, dw, aw, rows + K), _rand_side(M, dw, aw, 100 + M + K)
    terms = R.layer_terms(tr_h, te_h, dw)
    for mask in (1, 2, 4, 8, 15):
        want = None
        for l in range(4):
            if mask >> l & 1:
                want = (np.zeros_like(terms[l]) if want is None else want) + terms[l]
        S = torch.full((rows, M), float("nan"), dtype=torch.float64, device=PG.DEV)
        _scores(tr_d, te_d, dw, aw, S, 0, 0.5, 1, mask)
        _same(S, 0.5 * want, f"scores, mask {mask}")
        want_self = R.self_influence([tr_h], [0.5], dw, mask)
        out = torch.full((rows,), float("nan"), dtype=torch.float64, device=PG.DEV)
        _self(tr_d, dw, aw, out, 0, 0.5, 1, mask)
        _same(out, want_self, f"self, mask {mask}")
        D = torch.full((rows, rows), float("nan"), dtype=torch.float64, device=PG.DEV)
        if rows <= 4096:
            _scores(tr_d, tr_d, dw, aw, D, 0, 0.5, 1, mask)
            _same(out, D.diagonal().cpu().numpy(), f"self against the diagonal of the scores, mask {mask}")
    # two checkpoints into rows 4.. of a larger S whose other rows stay as they were; the second block of factors is another draw
    (tr2_h, tr2_d), (te2_h, te2_d) = _rand_side(rows, dw, aw, 200 + rows), _rand_side(M, dw, aw, 300 + M)
    want = R.scores([(tr_h, te_h), (tr2_h, te2_h)], (0.5, 0.003), dw)
    N = rows + 7
    fill = np.random.default_rng(1).standard_normal((N, M))
    S = PG.dev(fill.copy())
    S[4:4 + rows] = float("nan")
    _scores(tr_d, te_d, dw, aw, S, 4, 0.5, 1, 15)
    _scores(tr2_d, te2_d, dw, aw, S, 4, 0.003, 0, 15)
    fill[4:4 + rows] = want
    _same(S, fill, "two accumulating calls at row0 = 4")
    self2 = PG.dev(fill[:, 0].copy())
    _self(tr_d, dw, aw, self2, 4, 0.5, 1, 15)
    _self(tr2_d, dw, aw, self2, 4, 0.003, 0, 15)
    fill[4:4 + rows, 0] = R.self_influence([tr_h, tr2_h], (0.5, 0.003), dw)
    _same(self2, fill[:, 0], "two accumulating self calls at row0 = 4")
    if rows > 1:                                                              # the same block in two calls
        cut = rows // 3 + 1
        one = torch.full((rows, M), float("nan"), dtype=torch.float64, device=PG.DEV)
        two = one.clone()
        _scores(tr_d, te_d, dw, aw, one, 0, 0.003, 1, 15)
        part = lambda a, b: (tr_d[0][a:b].contiguous(), [x[a:b].contiguous() for x in tr_d[1]])
        _scores(part(0, cut), te_d, dw, aw, two, 0, 0.003, 1, 15)
        _scores(part(cut, rows), te_d, dw, aw, two, cut, 0.003, 1, 15)
        assert torch.equal(one.view(torch.int64), two.view(torch.int64)) and not torch.isnan(one).any()


# ---- top-k ----------------------------------------------------------------------------------------------------------------------------
def _topk(S, k, largest):
    lib = L.load()
    N, M = S.shape
    ws = torch.empty(max(lib.bx_tracin_topk_workspace(N, M), 8), dtype=torch.uint8, device=PG.DEV)
    idx = torch.full((M, k), -1, dtype=torch.int32, device=PG.DEV)
    val = torch.full((M, k), float("nan"), dtype=torch.float64, device=PG.DEV)
    L.check(lib.bx_tracin_topk(PG.p(S), N, M, k, largest, PG.p(idx), PG.p(val), PG.p(ws), ws.numel(), PG.stream()), "bx_tracin_topk")
    torch.cuda.synchronize()
    return idx, val


@pytest.mark.parametrize("M", [1, 3, 65])
@pytest.mark.parametrize("N", [1, 5, 257, 70001])
def test_topk_exact(N, M):
    rng = np.random.default_rng(N + M)
    S = rng.standard_normal((N, M))
    for j in range(M):                                                       # column kinds: Gaussian, four levels, signed zeros, all equal, negative only
        kind = j % 5
        if kind == 1:
            S[:, j] = rng.choice([-1.5, 0.0, 0.25, 3.0], size=N)
        elif kind == 2:
            S[:, j] = np.where(rng.random(N) < 0.5, 0.0, -0.0)
        elif kind == 3:
            S[:, j] = 0.75
        elif kind == 4:
            S[:, j] = -np.abs(S[:, j]) - 1.0
    S_d = PG.dev(S)
    for k in (1, 3, 256):
        if k > N:
            continue
        for largest in (1, 0):
            idx, val = _topk(S_d, k, largest)
            want_i, want_v = R.select(S, k, bool(largest))
            _same(idx, want_i, f"indices N={N} M={M} k={k} largest={largest}")
            _same(val, want_v, f"values N={N} M={M} k={k} largest={largest}")


# ---- limits -----------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_before_a_pointer_is_touched():
    lib = L.load()
    dw, aw = _widths(6, 128, 256, 32)
    def _side_null(rows):
        s = L.TracinSide()
        s.rows = rows
        return s

    def refused(rc, text):
        assert rc == -6 and text in lib.bx_last_error_string().decode(), lib.bx_last_error_string()

    args = lambda tr, te, shape, N: (C.byref(_side_null(tr)), C.byref(_side_null(te)), C.byref(shape), None, N, 0, 1.0, 1, 15, None)
    refused(lib.bx_tracin_scores(*args(8, 4097, _shape(dw, aw), 8)), "4097 test rows")
    refused(lib.bx_tracin_scores(*args(65537, 4, _shape(dw, aw), 65537)), "65537 training rows")
    refused(lib.bx_tracin_scores(*args(8, 2048, _shape(dw, aw), 1 << 20)), "N * M")
    refused(lib.bx_tracin_scores(*args(8, 8, _shape(dw, (128, 12, 4097, 256)), 8)), "4097 inputs")
    refused(lib.bx_tracin_self(C.byref(_side_null(8)), C.byref(_shape(dw, (128, 12, 4097, 256))), None, 8, 0, 1.0, 1, 15, None), "4097 inputs")
    refused(lib.bx_tracin_topk(None, 300, 4097, 1, 1, None, None, None, 0, None), "4097 columns")
    refused(lib.bx_tracin_topk(None, 300, 4, 257, 1, None, None, None, 0, None), "k = 257")
    refused(lib.bx_tracin_topk(None, 1 << 20, 2048, 1, 1, None, None, None, 0, None), "N * M")
    assert lib.bx_tracin_topk(None, 3, 4, 4, 1, None, None, None, 0, None) == -1 and b"k = 4 of N = 3" in lib.bx_last_error_string()
    assert lib.bx_tracin_topk_workspace(1 << 20, 2048) == 0
    refused(lib.bx_tracin_factors(None, None, None, None, None, None, None, None, None, None, None, 4, 33, 128, 0, None), "33 classes")
    refused(lib.bx_tracin_factors(None, None, None, None, None, None, None, None, None, None, None, 4, 6, 257, 0, None), "257 hidden units")


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _tiny_model():
    torch.manual_seed(5)
    m = brainxai.MultimodalModel(brainxai.EEGNet(6, Chans=4, Samples=64), brainxai.Spectrogram_Model(6, in_channels=1), num_classes=6)
    with torch.no_grad():                                                   # running statistics of a model that has seen data
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    return m.to(PG.DEV).eval()


def _data(n, seed, labels=False):
    g = torch.Generator().manual_seed(seed)
    eeg, spec = torch.randn(n, 1, 4, 64, generator=g), torch.rand(n, 1, 32, 32, generator=g)
    target = torch.randint(0, 6, (n,), generator=g) if labels else torch.softmax(2 * torch.randn(n, 6, generator=g), dim=1)
    return eeg.to(PG.DEV), spec.to(PG.DEV), target.to(PG.DEV)


def _checkpoints(model, tmp_path):
    base = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sds = []
    for c in range(3):
        g = torch.Generator().manual_seed(40 + c)
        sds.append({k: (v * (1 + 0.2 * torch.randn(v.shape, generator=g).to(v.device)) if v.is_floating_point() and "running" not in k else v.clone())
                    for k, v in base.items()})
    path = tmp_path / "ck2.pth"
    torch.save({"epoch": 3, "state_dict": {k: v.cpu() for k, v in sds[2].items()}}, path)
    return sds, [sds[0], {"state_dict": sds[1], "epoch": 2}, str(path)]


def _activations(model, sd, eeg, spec):
    """The activations of the four layers under the weights ``sd``, downloaded: (acts as the library orders them, logp, hidden, e, s, w1, w2)."""
    import copy
    m = copy.deepcopy(model)
    m.load_state_dict(sd)
    lib = L.load()
    n = eeg.shape[0]
    with torch.no_grad(), X._eval_frozen(m):
        ef = m.eeg_model.features(eeg).float().contiguous()
        feat = m.spectrogram_model.features(spec).permute(0, 2, 3, 1).contiguous()
        gap = torch.empty(n, 256, device=PG.DEV)
        s, e, logp = (torch.empty(n, 6, device=PG.DEV) for _ in range(3))
        hidden = torch.empty(n, 128, device=PG.DEV)
        p = [t.detach() for t in (m.spectrogram_model.fc.weight, m.spectrogram_model.fc.bias, m.eeg_model.dense.weight, m.eeg_model.dense.bias, m.fc1.weight,
                                  m.fc1.bias, m.fc2.weight, m.fc2.bias)]
        L.check(lib.bx_mm_head_fwd(PG.p(feat), PG.p(ef), *[PG.p(t) for t in p], PG.p(gap), PG.p(s), PG.p(e), PG.p(hidden), PG.p(logp), n,
                                   feat.shape[1] * feat.shape[2], 256, ef.shape[1], 6, 128, L.BX_F32, PG.stream()), "bx_mm_head_fwd")
        gap1, s1 = torch.empty_like(gap), torch.empty_like(s)              # the stand-alone branches' own heads
        L.check(lib.bx_gap_fc_lsm_fwd(PG.p(feat), PG.p(p[0]), PG.p(p[1]), PG.p(gap1), PG.p(s1), n, feat.shape[1] * feat.shape[2], 256, 6, L.BX_F32,
                                      PG.stream()), "bx_gap_fc_lsm_fwd")
        e1 = m.eeg_model(eeg).float()
    h = lambda t: t.cpu().numpy()
    return dict(acts=[h(hidden), np.concatenate([h(e), h(s)], axis=1), h(ef), h(gap)], logp=h(logp), hidden=h(hidden), e=h(e), s=h(s), w1=h(m.fc1.weight.detach()),
                w2=h(m.fc2.weight.detach()), model=m, alone=[(h(e1), h(ef)), (h(s1), h(gap1))])


def _ref_side(a, target):
    delta, loss = R.factors_multimodal(a["logp"], target.cpu().numpy(), a["hidden"], a["e"], a["s"], a["w1"], a["w2"])
    return (delta, a["acts"]), loss


ETAS = (1, 0.5, 0.1)
DW = (6, 128, 6, 6)


def _snapshot(model):
    return [t.detach().clone() for t in list(model.parameters()) + list(model.buffers())]


def _unchanged(model, snap):
    return all(torch.equal(a.detach().reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
               for a, b in zip(list(model.parameters()) + list(model.buffers()), snap))


def test_end_to_end_multimodal(tmp_path):
    model = _tiny_model()
    train, test = _data(7, 1), _data(3, 2)
    sds, cks = _checkpoints(model, tmp_path)
    snap = _snapshot(model)
    res = brainxai.tracin(model, cks, train, test, learning_rates=ETAS, top=4, keep_scores=True, return_parts=True)
    assert _unchanged(model, snap) and model.training is False
    sides, train_l, test_l = [], [], []
    for sd in sds:
        (tr, l_tr), (te, l_te) = _ref_side(_activations(model, sd, *train[:2]), train[2]), _ref_side(_activations(model, sd, *test[:2]), test[2])
        sides.append((tr, te))
        train_l.append(l_tr)
        test_l.append(l_te)
    want = R.scores(sides, ETAS, DW)
    _same(res.scores, want, "scores")
    _same(res.train_losses, np.stack(train_l), "training losses")
    _same(res.test_losses, np.stack(test_l), "test losses")
    assert res.N == 7 and res.layers == R.MULTIMODAL_LAYERS and res.learning_rates == (1.0, 0.5, 0.1)
    for largest, idx, val in ((True, res.proponents, res.proponent_scores), (False, res.opponents, res.opponent_scores)):
        want_i, want_v = R.select(want, 4, largest)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_i)
        _same(val, want_v, "selected scores")
    for kw in (dict(max_batch=2), dict(block_rows=3), dict(max_batch=2, block_rows=3)):
        again = brainxai.tracin(model, cks, train, test, learning_rates=ETAS, top=4, keep_scores=True, return_parts=True, **kw)
        assert torch.equal(again.scores.view(torch.int64), res.scores.view(torch.int64)), kw
        assert torch.equal(again.proponents, res.proponents) and torch.equal(again.opponents, res.opponents)
    batches = [tuple(t[a:b].cpu() for t in train) for a, b in ((0, 3), (3, 4), (4, 7))]          # a re-iterable of host batches
    lazy = brainxai.tracin(model, cks, batches, test, learning_rates=ETAS, top=4, keep_scores=True, return_parts=True)
    assert torch.equal(lazy.scores.view(torch.int64), res.scores.view(torch.int64)) and lazy.N == 7
    pro, opp = brainxai.tracin(model, cks, train, test, learning_rates=ETAS, top=4)
    assert torch.equal(pro, res.proponents) and torch.equal(opp, res.opponents)
    # layers: 'head' is the sum of fc2's and fc1's terms
    head = brainxai.tracin(model, cks, train, test, layers="head", learning_rates=ETAS, top=1, keep_scores=True, return_parts=True)
    _same(head.scores, R.scores(sides, ETAS, DW, mask=3), "layers='head'")
    assert head.layers == ("fc2", "fc1")
    # self-influence: the diagonal of tracin(train, train)
    diag = brainxai.tracin(model, cks, train, train, learning_rates=ETAS, top=1, keep_scores=True, return_parts=True).scores.diagonal()
    si, top = brainxai.self_influence(model, cks, train, learning_rates=ETAS, top=3, max_batch=4)
    assert torch.equal(si.view(torch.int64), diag.contiguous().view(torch.int64))
    _same(si, R.self_influence([s[0] for s in sides], ETAS, DW), "self-influence")
    assert np.array_equal(top.cpu().numpy(), R.select(si.cpu().numpy()[:, None], 3, True)[0][0])
    assert _unchanged(model, snap)
    # a checkpoint with a missing key raises in the middle; the model is put back
    broken = dict(sds[1])
    del broken["fc1.bias"]
    with pytest.raises(ValueError, match="tracin: checkpoint 1: its keys are not the model's"):
        brainxai.tracin(model, [cks[0], broken, cks[2]], train, test, top=2)
    assert _unchanged(model, snap)
    # a flagged example is named
    bad = (train[0], train[1], train[2].clone())
    bad[2][5] = 0.0
    with pytest.raises(ValueError, match="tracin: checkpoint 0: training example 5 has a target with a negative entry or no mass"):
        brainxai.tracin(model, cks, bad, test, top=2)
    assert _unchanged(model, snap)


def test_end_to_end_branches(tmp_path):
    model = _tiny_model()
    sds, _ = _checkpoints(model, tmp_path)
    train, test = _data(7, 3, labels=True), _data(3, 4)
    for branch, prefix, which in ((model.eeg_model, "eeg_model.", 0), (model.spectrogram_model, "spectrogram_model.", 1)):
        cks = [{k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)} for sd in sds]
        snap = _snapshot(branch)
        res = brainxai.tracin(branch, cks, (train[which], train[2]), (test[which], test[2]), learning_rates=ETAS, top=2, max_batch=3, keep_scores=True,
                              return_parts=True)
        assert _unchanged(branch, snap)
        sides = []
        for sd in sds:
            pair = []
            for data in (train, test):
                a = _activations(model, sd, *data[:2])
                logp, act = a["alone"][which]
                delta, _ = R.factors_single(logp, data[2].cpu().numpy())
                pair.append((delta, [act]))
            sides.append(tuple(pair))
        want = R.scores(sides, ETAS, (6,))
        _same(res.scores, want, f"{prefix} scores")
        assert np.array_equal(res.proponents.cpu().numpy(), R.select(want, 2, True)[0])
        si = brainxai.self_influence(branch, cks, (train[which], train[2]), learning_rates=ETAS)
        _same(si, R.self_influence([s[0] for s in sides], ETAS, (6,)), f"{prefix} self-influence")


def _head_fp32(a, target, dtype):
    """The four layers on the downloaded activations in CPU torch at ``dtype``: per-example gradients of KLDivLoss('sum')."""
    m = a["model"]
    P = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (m.fc2.weight, m.fc2.bias, m.fc1.weight, m.fc1.bias, m.eeg_model.dense.weight,
                                                                   m.eeg_model.dense.bias, m.spectrogram_model.fc.weight, m.spectrogram_model.fc.bias)]
    feat, gap, t = (torch.from_numpy(x).to(dtype) for x in (a["acts"][2], a["acts"][3], target))
    out = []
    for i in range(feat.shape[0]):
        s = torch.log_softmax(gap[i:i + 1] @ P[6].T + P[7], dim=1)
        e = torch.log_softmax(feat[i:i + 1] @ P[4].T + P[5], dim=1)
        logp = torch.log_softmax(torch.relu(torch.cat([e, s], dim=1) @ P[2].T + P[3]) @ P[0].T + P[1], dim=1)
        l = torch.nn.functional.kl_div(logp, t[i:i + 1], reduction="sum")
        out.append(torch.cat([g.double().flatten() for g in torch.autograd.grad(l, P)]))
    return torch.stack(out)


def test_end_to_end_against_autograd_through_the_model(tmp_path):
    model = _tiny_model()
    train, test = _data(7, 1), _data(3, 2)
    sds, cks = _checkpoints(model, tmp_path)
    res = brainxai.tracin(model, cks, train, test, learning_rates=ETAS, top=2, keep_scores=True, return_parts=True)
    S = res.scores.cpu().numpy()
    own, route, scale = np.zeros_like(S), np.zeros_like(S), np.zeros_like(S)
    names = ["fc2", "fc1", "eeg_model.dense", "spectrogram_model.fc"]
    for sd, eta in zip(sds, ETAS):
        a_tr, a_te = _activations(model, sd, *train[:2]), _activations(model, sd, *test[:2])
        g_tr, g_te = _head_fp32(a_tr, train[2].cpu().numpy(), torch.float32), _head_fp32(a_te, test[2].cpu().numpy(), torch.float32)
        own += eta * (g_tr @ g_te.T).numpy()
        m = a_tr["model"].eval()
        grads = []
        for data in (train, test):
            rows = []
            for i in range(data[0].shape[0]):
                m.zero_grad(set_to_none=True)
                brainxai.KLDivLoss("sum")(m(data[0][i:i + 1], data[1][i:i + 1]), data[2][i:i + 1]).backward()
                rows.append(torch.cat([q.grad.double().flatten() for n in names for q in (X._resolve(m, n).weight, X._resolve(m, n).bias)]))
            grads.append(torch.stack(rows))
        route += eta * (grads[0] @ grads[1].T).cpu().numpy()
        scale += eta * (grads[0].norm(dim=1)[:, None] * grads[1].norm(dim=1)[None, :]).cpu().numpy()
    rho_own, rho = (np.abs(own - S) / scale).max(), (np.abs(route - S) / scale).max()
    print(f"tracin against autograd: fp32 restatement {rho_own:.3e} of |g_i||g_j|, the product model's route {rho:.3e} (ratio {rho / rho_own:.2f}, allowed 8)")
    assert np.abs(S).max() > 1e3 * rho_own * scale.max()                      # the scores stand far above the route's rounding
    assert (np.abs(route - S) <= 8 * rho_own * scale).all()
