"""CPU: TracIn's reference (tests/tracin_ref.py) against autograd and against a first-order expansion, its selection rule, and every
refusal of ``tracin`` / ``self_influence`` (none of which needs a device).

Autograd.  A float64 torch restatement of the four layers -- gap -> fc -> LogSoftmax, features -> dense -> LogSoftmax, cat -> fc1 ->
ReLU -> fc2 -> LogSoftmax -- runs on random activations; ``torch.autograd.grad`` of KLDivLoss(reduction='sum') of one example gives the
gradients of every layer's weight and bias, and their dot products over two examples must equal the reference's per-layer terms
(delta_i . delta_j)(a_i . a_j + 1) within 4 D 2^-53 sum|terms|: both sides are fp64 and D, the layer's width, is the larger of its fan-in
and fan-out.  sum|terms| is the term evaluated with the absolute value of everything that is added on the way to it (_companion):
delta_2~ = T p + t, delta_1~ = (|W2|^T delta_2~) (.) [h > 0], v~ = |W1|^T delta_1~, delta_e~ = v_e~ + exp(e) sum(v_e~), and
(delta_i~ . delta_j~)(|a_i| . |a_j| + 1) -- the quantity a forward error analysis of either route is relative to.  (A first version summed
|gW_i gW_j| + |gb_i gb_j| over autograd's own gradients.  That is no bound for a correct fp64 route: the factors of the three layers
behind fc2 come out of sums over K and Hd terms that cancel, and both routes carry those sums' rounding, which the gradients' own size
does not show; the reference missed it by a factor 1.32 on one pair of eeg_model.dense at (6,128,16,32) with labels, at a relative
difference of 1.9e-14.)
First order.  On the same restatement one SGD step of size eta on example i changes l_j by -eta S[i,j] + r(eta), r = O(eta^2): r(eta) /
r(eta / 2) = 4 (1 + O(eta)).  The step is measured by what it does: eta_0 = 2^-9 / S[i,i], a first-order change of i's own loss by 2^-9 (at 2^-6 a
hidden unit of one case changes sign inside the step, where the loss is not smooth)
(S[i,i] is the squared norm of i's gradient, in the thousands on these activations).  A wrong sign or a missing layer leaves a linear
remainder (ratio 2); the band 4 +- 0.2 at eta_0 and eta_0 / 2 separates the two, and the remainder at eta_0 must be below a tenth of
eta_0 |S| for the pair with the largest |S|."""
import re

import numpy as np
import pytest
import torch

import brainxai
from brainxai import explain as X
from tests import tracin_ref as R

WIDTHS = [(1, 2, 1, 1), (3, 8, 5, 7), (6, 128, 16, 32)]
LAYERS = R.MULTIMODAL_LAYERS


class _Head(torch.nn.Module):
    """The four layers in float64 on given activations."""

    def __init__(self, K, Hd, C, F, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter((torch.randn(*s, generator=g) * 0.4).double())
        self.fc_w, self.fc_b, self.dense_w, self.dense_b = mk(K, C), mk(K), mk(K, F), mk(K)
        self.w1, self.b1, self.w2, self.b2 = mk(Hd, 2 * K), mk(Hd), mk(K, Hd), mk(K)

    def groups(self):
        return [(self.w2, self.b2), (self.w1, self.b1), (self.dense_w, self.dense_b), (self.fc_w, self.fc_b)]      # the library's layer order

    def forward(self, gap, feat):
        s = torch.log_softmax(gap @ self.fc_w.T + self.fc_b, dim=1)
        e = torch.log_softmax(feat @ self.dense_w.T + self.dense_b, dim=1)
        h = torch.relu(torch.cat([e, s], dim=1) @ self.w1.T + self.b1)
        return torch.log_softmax(h @ self.w2.T + self.b2, dim=1), h, e, s


def _kl_sum(logp, t):
    return torch.where(t > 0, t * (torch.log(torch.where(t > 0, t, torch.ones_like(t))) - logp), torch.zeros_like(t)).sum()


def _case(K, Hd, C, F, kind, n=5, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + K)
    net = _Head(K, Hd, C, F, seed + 7)
    gap, feat = torch.rand(n, C, generator=g).double(), torch.randn(n, F, generator=g).double()
    if kind == "labels":
        labels = torch.randint(0, K, (n,), generator=g)
        t, target = torch.nn.functional.one_hot(labels, K).double(), labels.numpy()
    else:
        t = torch.rand(n, K, generator=g)
        t[torch.rand(n, K, generator=g) < 0.3] = 0.0
        t[:, 0] += 0.1                                                       # no row without mass
        t = t / t.sum(dim=1, keepdim=True)
        if kind == "unnormalised":
            t = t * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
        t = t.float().double()                                               # what an fp32 target holds
        target = t.numpy()
    return net, gap, feat, t, target


def _companion(net, gap, feat, t):
    """The factors with every added term replaced by its absolute value, fp64 [n, K + Hd + K + K], and the |activations|."""
    with torch.no_grad():
        logp, h, e, s = net(gap, feat)
        K = logp.shape[1]
        d2 = t.sum(dim=1, keepdim=True) * logp.exp() + t
        d1 = (d2 @ net.w2.abs()) * (h > 0)
        v = d1 @ net.w1.abs()
        de = v[:, :K] + e.exp() * v[:, :K].sum(dim=1, keepdim=True)
        ds = v[:, K:] + s.exp() * v[:, K:].sum(dim=1, keepdim=True)
    return torch.cat([d2, d1, de, ds], dim=1).numpy(), [np.abs(a) for a in (h.numpy(), torch.cat([e, s], dim=1).numpy(), feat.numpy(), gap.numpy())]


def _reference(net, gap, feat, target):
    with torch.no_grad():
        logp, h, e, s = net(gap, feat)
    delta, loss = R.factors_multimodal(logp.numpy(), target, h.numpy(), e.numpy(), s.numpy(), net.w1.detach().numpy(), net.w2.detach().numpy())
    acts = [h.numpy(), torch.cat([e, s], dim=1).numpy(), feat.numpy(), gap.numpy()]
    return delta, loss, acts


@pytest.mark.parametrize("kind", ["distribution", "unnormalised", "labels"])
@pytest.mark.parametrize("K,Hd,C,F", WIDTHS)
def test_reference_terms_match_autograd(K, Hd, C, F, kind):
    net, gap, feat, t, target = _case(K, Hd, C, F, kind)
    n = gap.shape[0]
    delta, loss, acts = _reference(net, gap, feat, target)
    grads = []
    for i in range(n):
        logp = net(gap[i:i + 1], feat[i:i + 1])[0]
        l = _kl_sum(logp, t[i:i + 1])
        ti, lpi = t[i].numpy(), logp.detach().numpy()[0]
        scale = float((ti * (np.abs(np.log(np.where(ti > 0, ti, 1.0))) + np.abs(lpi))).sum())
        assert abs(float(l.detach()) - loss[i]) <= 8 * K * 2.0 ** -53 * scale           # K terms, each a few roundings of its two logarithms' size
        flat = torch.autograd.grad(l, [q for pair in net.groups() for q in pair])
        grads.append([(flat[2 * k].numpy(), flat[2 * k + 1].numpy()) for k in range(4)])
    dwidth = (K, Hd, K, K)
    terms = R.layer_terms((delta, acts), (delta, acts), dwidth)
    scales = R.layer_terms(*(_companion(net, gap, feat, t),) * 2, dwidth)
    widths = [max(Hd, K), max(2 * K, Hd), max(F, K), max(C, K)]
    worst = 0.0
    for l in range(4):
        for i in range(n):
            for j in range(n):
                (wi, bi), (wj, bj) = grads[i][l], grads[j][l]
                want = float((wi * wj).sum() + (bi * bj).sum())
                tol = 4 * widths[l] * 2.0 ** -53 * float(scales[l][i, j])
                err = abs(terms[l][i, j] - want)
                worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else np.inf))
                assert err <= tol, f"{LAYERS[l]} pair {(i, j)}: {terms[l][i, j]!r} against autograd's {want!r}, bound {tol:.2e}"
    print(f"K={K} Hd={Hd} C={C} F={F} {kind}: worst |term - autograd| / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", ["distribution", "labels"])
@pytest.mark.parametrize("K,Hd,C,F", WIDTHS[1:])
def test_first_order_change_of_the_loss(K, Hd, C, F, kind):
    net, gap, feat, t, target = _case(K, Hd, C, F, kind, seed=3)
    n = gap.shape[0]
    delta, _, acts = _reference(net, gap, feat, target)
    S = R.scores([((delta, acts), (delta, acts))], [1.0], (K, Hd, K, K))
    params = [q for pair in net.groups() for q in pair]
    saved = [q.detach().clone() for q in params]
    with torch.no_grad():
        base = np.array([float(_kl_sum(net(gap[j:j + 1], feat[j:j + 1])[0], t[j:j + 1])) for j in range(n)])

    def remainder(i, eta):
        g = torch.autograd.grad(_kl_sum(net(gap[i:i + 1], feat[i:i + 1])[0], t[i:i + 1]), params)
        with torch.no_grad():
            for q, gq in zip(params, g):
                q -= eta * gq
            after = np.array([float(_kl_sum(net(gap[j:j + 1], feat[j:j + 1])[0], t[j:j + 1])) for j in range(n)])
            for q, s in zip(params, saved):
                q.copy_(s)
        return after - base + eta * S[i]

    checked = 0
    for i in range(n):
        eta = 2.0 ** -9 / S[i, i]
        r = [remainder(i, eta / d) for d in (1, 2, 4)]
        j = int(np.abs(S[i]).argmax())
        assert abs(r[0][j]) <= 0.1 * eta * abs(S[i, j]), f"pair {(i, j)}: the loss moves by {r[0][j] - eta * S[i, j]:.3e}, -eta S = {-eta * S[i, j]:.3e}"
        for j in range(n):
            if abs(r[2][j]) < 1e-12:                                         # a remainder at the rounding of the losses says nothing
                continue
            q1, q2 = r[0][j] / r[1][j], r[1][j] / r[2][j]
            assert abs(q1 - 4.0) <= 0.2 and abs(q2 - 4.0) <= 0.2, f"pair {(i, j)}: remainder ratios {q1:.3f}, {q2:.3f}"
            checked += 1
    assert checked >= n


def test_exp_and_log_are_accurate():
    x = np.concatenate([np.linspace(-40.0, 0.5, 4001), [-708.0, 0.0, 709.0]])
    with np.errstate(over="ignore"):
        assert np.all(np.abs(R.exp(x) - np.exp(x)) <= 4 * 2.0 ** -53 * np.exp(x))
    assert R.exp(np.array([0.0]))[0] == 1.0 and R.exp(np.array([-709.0]))[0] == 0.0 and np.isnan(R.exp(np.array([np.nan]))[0])
    t = np.concatenate([np.float32(np.random.default_rng(0).random(4000)) + np.float32(1e-30), [1.0, 0.5, 2.0, 1e-38, 3e38]]).astype(np.float64)
    assert np.all(np.abs(R.log(t) - np.log(t)) <= 4 * 2.0 ** -53 * np.maximum(np.abs(np.log(t)), 2.0 ** -10))
    assert R.log(np.array([1.0]))[0] == 0.0


def test_selection_rule():
    S = np.array([[1.0, -1.0, 0.0], [3.0, -3.0, -0.0], [3.0, -2.0, 0.0], [-0.0, -3.0, 0.0], [0.0, -5.0, -0.0], [3.0, -1.0, 0.0]])
    idx, val = R.select(S, 4, True)
    assert idx.tolist() == [[1, 2, 5, 0], [0, 5, 2, 1], [0, 1, 2, 3]]
    assert val[0].tolist() == [3.0, 3.0, 3.0, 1.0] and val[1].tolist() == [-1.0, -1.0, -2.0, -3.0]
    assert np.signbit(val[2]).tolist() == [False, True, False, False]          # the values are S's own, a zero's sign included
    idx, val = R.select(S, 6, False)                                           # k = N
    assert idx.tolist() == [[3, 4, 0, 1, 2, 5], [4, 1, 3, 2, 0, 5], [0, 1, 2, 3, 4, 5]]
    assert val[1].tolist() == [-5.0, -3.0, -3.0, -2.0, -1.0, -1.0]
    idx, _ = R.select(S[:, 1:2], 1, True)                                      # a negative-only column
    assert idx.tolist() == [[0]]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _tiny(K=6):
    torch.manual_seed(0)
    return brainxai.MultimodalModel(brainxai.EEGNet(K, Chans=4, Samples=64), brainxai.Spectrogram_Model(K, in_channels=1), num_classes=K)


def _data(n, K=6, labels=False):
    g = torch.Generator().manual_seed(n)
    target = torch.randint(0, K, (n,), generator=g) if labels else torch.softmax(torch.randn(n, K, generator=g), dim=1)
    return torch.randn(n, 1, 4, 64, generator=g), torch.rand(n, 1, 32, 32, generator=g), target


def _refused(text, fn, *args, exc=ValueError, **kw):
    with pytest.raises(exc, match="^" + re.escape(text) + "$"):
        fn(*args, **kw)


def test_tracin_is_exported():
    assert brainxai.tracin is X.tracin and brainxai.self_influence is X.self_influence
    assert brainxai.TracInResult._fields == ("proponents", "proponent_scores", "opponents", "opponent_scores", "scores", "train_losses", "test_losses",
                                             "layers", "learning_rates", "N")


def test_refusals_of_the_model():
    m, train, test = _tiny(), _data(5), _data(2)
    cks = [m.state_dict()]
    _refused("tracin: needs a MultimodalModel, a Spectrogram_Model or an EEGNet, got Linear", brainxai.tracin, torch.nn.Linear(2, 2), cks, train, test)
    deep = brainxai.MultimodalModel(brainxai.EEGNet(6, Chans=4, Samples=64), brainxai.Spectrogram_Model(6, in_channels=1))
    deep.eeg_model = brainxai.EEGNetAttentionDeep(6, Chans=4, Samples=64)
    _refused("tracin: an EEGNetAttentionDeep branch is out of scope; the EEG branch must be an EEGNet", brainxai.tracin, deep, cks, train, test)
    hooked = _tiny()
    hooked.eeg_model.register_forward_hook(lambda *a: None)
    _refused("tracin: needs the un-hooked reference MultimodalModel (EEGNet, Spectrogram_Model, head Linear(2K,Hd) -> ReLU -> Linear(Hd,K) with "
             "Hd * 2K <= 4096): its activations come from the fused head", brainxai.tracin, hooked, cks, train, test)
    _refused("self_influence: K = 33 classes, Hd = 128 hidden units, C = 256 channels, F = 32 EEG features; supported K <= 32, Hd <= 256, C <= 1024, "
             "F <= 4096", brainxai.self_influence, _tiny(33), cks, train)
    wide = brainxai.EEGNet(6, Chans=4, Samples=32 * 257)
    _refused("tracin: K = 6 classes, Hd = 1 hidden units, C = 1 channels, F = 4112 EEG features; supported K <= 32, Hd <= 256, C <= 1024, F <= 4096",
             brainxai.tracin, wide, cks, train[::2], test[::2])


def test_refusals_of_the_options():
    m, train, test = _tiny(), _data(5), _data(2)
    cks = [m.state_dict(), {"state_dict": m.state_dict()}]
    names = "('fc2', 'fc1', 'eeg_model.dense', 'spectrogram_model.fc')"
    _refused(f"tracin: unknown layer 'fc3'; use 'all', 'head' or any of {names}", brainxai.tracin, m, cks, train, test, layers=["fc2", "fc3"])
    _refused(f"tracin: unknown layer 'everything'; use 'all', 'head' or any of {names}", brainxai.tracin, m, cks, train, test, layers="everything")
    _refused("tracin: layers is empty", brainxai.tracin, m, cks, train, test, layers=[])
    _refused("tracin: layers must be 'all', 'head' or a sequence of layer names, got int", brainxai.tracin, m, cks, train, test, layers=3)
    _refused("self_influence: unknown layer 'head'; use 'all' or any of ('dense',)", brainxai.self_influence, m.eeg_model, cks, train[::2], layers="head")
    _refused("tracin: checkpoints is empty", brainxai.tracin, m, [], train, test)
    _refused("tracin: checkpoints must be a sequence of state dicts, dicts with a 'state_dict' key or paths, got OrderedDict", brainxai.tracin, m,
             m.state_dict(), train, test)
    _refused("tracin: checkpoint 1 must be a state dict, a dict with a 'state_dict' key or a path, got int", brainxai.tracin, m, [cks[0], 3], train, test)
    _refused("tracin: 3 learning rates for 2 checkpoints", brainxai.tracin, m, cks, train, test, learning_rates=(1, 2, 3))
    _refused("tracin: learning rate 1 must be a finite number, got inf", brainxai.tracin, m, cks, train, test, learning_rates=(1, float("inf")))
    _refused("tracin: learning rate 0 must be a finite number, got 'a'", brainxai.tracin, m, cks, train, test, learning_rates=("a", 1))
    _refused("tracin: learning_rates must be None or one number per checkpoint, got float", brainxai.tracin, m, cks, train, test, learning_rates=0.1)
    _refused("tracin: max_batch = 0 < 1", brainxai.tracin, m, cks, train, test, max_batch=0)
    _refused("tracin: block_rows = 0 outside 1..1073741824", brainxai.tracin, m, cks, train, test, block_rows=0)
    _refused("tracin: top = 0 outside 1..256", brainxai.tracin, m, cks, train, test, top=0)
    _refused("tracin: top = 257 outside 1..256", brainxai.tracin, m, cks, train, test, top=257)
    _refused("tracin: top = None outside 1..256", brainxai.tracin, m, cks, train, test, top=None)
    _refused("tracin: top = 6 outside 1..5", brainxai.tracin, m, cks, train, test, top=6)
    _refused("self_influence: top = 6 outside 1..5", brainxai.self_influence, m, cks, train, top=6)


def test_refusals_of_the_data():
    m, train, test = _tiny(), _data(5), _data(2)
    cks = [m.state_dict()]
    form = "(eeg [n,1,Chans,T], spec [n,C,H,W], target)"
    lazy = ", or a re-iterable of such batches (a one-shot iterator cannot be walked once per checkpoint)"
    _refused(f"tracin: train{lazy} must be the tensors {form}", brainxai.tracin, m, cks, iter([train]), test)
    _refused(f"tracin: train{lazy} must be the tensors {form}", brainxai.tracin, m, cks, train[0], test)
    _refused(f"tracin: test must be the tensors {form}", brainxai.tracin, m, cks, train, [test])
    _refused(f"tracin: train must be the tensors {form}", brainxai.tracin, m, cks, train[:2], test)
    _refused(f"tracin: train must be the tensors {form}", brainxai.tracin, m, cks, (train[0][:, 0], train[1], train[2]), test)
    _refused("tracin: test hold 2 EEG and 1 spectrogram samples", brainxai.tracin, m, cks, train, (test[0], test[1][:1], test[2]))
    _refused("tracin: train are empty", brainxai.tracin, m, cks, tuple(t[:0] for t in train), test)
    _refused("tracin: the target of train must be fp32 [5, 6] or an integer tensor [5], got torch.float64 (5, 6)", brainxai.tracin, m, cks,
             (train[0], train[1], train[2].double()), test)
    _refused("tracin: the target of test must be fp32 [2, 6] or an integer tensor [2], got torch.int64 (2, 1)", brainxai.tracin, m, cks, train,
             (test[0], test[1], torch.zeros(2, 1, dtype=torch.int64)))
    _refused("self_influence: train must be the tensors (x, target) with x [n,C,H,W]", brainxai.self_influence, m.spectrogram_model, cks, train)
    _refused("self_influence: train must be the tensors (x, target) with x [n,1,Chans,T]", brainxai.self_influence, m.eeg_model, cks, (train[0][:, 0], train[2]))
    big = (torch.zeros(4097, 1, 4, 64), torch.zeros(4097, 1, 32, 32), torch.zeros(4097, dtype=torch.int64))
    _refused("tracin: 4097 test examples, supported 1..4096", brainxai.tracin, m, cks, train, big)


def test_there_is_no_cpu_path():
    m, train, test = _tiny(), _data(5), _data(2, labels=True)
    cks = [m.state_dict()]
    _refused("brainxai.tracin: the model, train and test must live on the GPU; there is no CPU path", brainxai.tracin, m, cks, train, test, top=2, exc=RuntimeError)
    _refused("brainxai.self_influence: the model and train must live on the GPU; there is no CPU path", brainxai.self_influence, m, cks, train,
             exc=RuntimeError)
    _refused("brainxai.self_influence: the model and train must live on the GPU; there is no CPU path", brainxai.self_influence, m.eeg_model, cks,
             [(train[0], train[2])], top=2, exc=RuntimeError)
