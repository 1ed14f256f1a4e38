"""CPU: Fusion SHAP's restatement against itself, its power to discriminate (checked before any GPU comparison is trusted), the host
helpers against their twins, and every refusal of the driver.  Nothing reaches the library's kernels.

TOL_GPU is the floor of the GPU comparison's tolerance for probabilities, 16 * 2^-24 (tests/test_gpu_fusion_shap.py: the kernel stays
within max(4 d0, 16 * 2^-24 * scale) of this restatement); the discrimination checks ask for more than 100 x that.  SEEDS are the
seeds the GPU tests draw their heads and votes from."""
import math
import re

import numpy as np
import pytest
import torch

import brainxai
from brainxai import explain as X
from tests import fusion_shap_ref as R

TOL_GPU = 16 * 2.0 ** -24
SEEDS = (0, 1, 2)
KS = (2, 3, 6)


def _game(K, seed, Hd=32, B=3, Nb=5):
    return (R.random_votes(B, K, 10 + seed), R.random_votes(B, K, 20 + seed), R.random_votes(Nb, K, 30 + seed), R.random_votes(Nb, K, 40 + seed),
            R.random_head(K, Hd, seed))


# ---- the restatement against itself --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("score", ["prob", "logprob"])
def test_efficiency(K, score):
    ex, sx, eb, sb, head = _game(K, 0)
    for form in ("votes", "modality", "class"):
        res = R.explain(ex, sx, eb, sb, R.players(form, K), head, score)
        gap = np.abs(res["values"].sum(-1) - (res["clean"] - res["empty"])).max()
        print(f"K {K} {score} {form}: |sum phi - (v(all) - v(none))| = {gap:.1e}")
        assert gap <= 1e-12
        assert np.abs(res["modality"].sum(-1) - (res["clean"] - res["empty"])).max() <= 1e-12
    # v(all) is the sample's own score, v(none) the mean score of the background rows
    z = np.concatenate([ex, sx], 1).astype(np.float64)
    assert np.abs(res["clean"] - R.scores(R.head(z, head), score)).max() <= 1e-15
    zb = np.concatenate([eb, sb], 1).astype(np.float64)
    assert np.abs(res["empty"] - R.scores(R.head(zb, head), score).mean(0)[None]).max() <= 1e-15


def test_null_player():
    K = 3
    ex, sx, eb, sb, head = _game(K, 1)
    w1 = head[0].copy()
    w1[:, [1, K + 2]] = 0.0                                               # votes 1 and K + 2 never reach the hidden layer
    res = R.explain(ex, sx, eb, sb, R.players("votes", K), (w1,) + head[1:], "prob")
    assert np.abs(res["values"][..., [1, K + 2]]).max() == 0.0
    assert np.abs(res["values"]).max() > 1e-3


def test_background_equal_to_the_sample():
    K = 3
    ex, sx, _, _, head = _game(K, 2, B=1)
    res = R.explain(ex, sx, ex, sx, R.players("votes", K), head, "logprob")
    assert np.abs(res["values"]).max() == 0.0 and np.abs(res["modality"]).max() == 0.0 and np.abs(res["interaction"]).max() == 0.0


@pytest.mark.parametrize("form", ["votes", "class", "modality"])
def test_linear_head_closed_form(form):
    """Without the ReLU the logits are linear in the votes: the Shapley value of a player is its votes' own term."""
    K = 3
    ex, sx, eb, sb, head = _game(K, 0)
    groups = R.players(form, K)
    v = R.logit_values(ex, sx, eb, sb, R.coalition_masks(groups), head, relu=False)
    phi = R.shapley(v.transpose(0, 2, 1), R.weights(len(groups)))
    want = R.linear_closed_form(ex, sx, eb, sb, groups, head)
    assert np.abs(phi - want).max() <= 1e-13
    with_relu = R.shapley(R.logit_values(ex, sx, eb, sb, R.coalition_masks(groups), head).transpose(0, 2, 1), R.weights(len(groups)))
    assert np.abs(with_relu - want).max() > 1e-3 or form == "modality"    # the ReLU is what makes the game non-additive


def test_permuting_the_players_permutes_the_values():
    K = 3
    ex, sx, eb, sb, head = _game(K, 1)
    groups = [[0, 4], [1], [2, 3, 5]]
    perm = [2, 0, 1]
    a = R.explain(ex, sx, eb, sb, groups, head, "prob")["values"]
    b = R.explain(ex, sx, eb, sb, [groups[p] for p in perm], head, "prob")["values"]
    assert np.abs(b - a[..., perm]).max() <= 1e-15


# ---- discrimination ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_discriminates(K, seed):
    """A kernel with the wrong (Banzhaf) weights, or a modality value summed up from its members' values, cannot pass the GPU
    comparison: on the seeds it uses both differ from the right answer by more than 100 x its tolerance."""
    ex, sx, eb, sb, head = _game(K, seed)
    groups = R.players("votes", K)
    right = R.explain(ex, sx, eb, sb, groups, head, "prob")
    wrong = R.explain(ex, sx, eb, sb, groups, head, "prob", w=R.banzhaf_weights(2 * K))
    banzhaf = np.abs(right["values"] - wrong["values"]).max()
    summed = np.stack([right["values"][..., :K].sum(-1), right["values"][..., K:].sum(-1)], -1)
    member = np.abs(right["modality"] - summed).max()
    print(f"K {K} seed {seed}: |shapley - banzhaf| = {banzhaf:.1e}, |modality - summed members| = {member:.1e}, 100 x tol = {100 * TOL_GPU:.1e}")
    assert banzhaf > 100 * TOL_GPU and member > 100 * TOL_GPU


# ---- host helpers --------------------------------------------------------------------------------------------------------------------------
def test_shapley_weights():
    for M in range(1, 17):
        w = brainxai.shapley_weights(M)
        assert w.dtype == np.float64 and w.shape == (M,)
        assert np.array_equal(w, R.weights(M))
        total = sum(float(w[s]) * math.comb(M - 1, s) for s in range(M))      # over the 2^(M-1) coalitions without a player
        assert abs(total - 1.0) <= 1e-14, (M, total)
    for bad in (0, 17, 2.0, True, "2"):
        with pytest.raises(ValueError, match="shapley_weights: M must be an int in 1..16"):
            brainxai.shapley_weights(bad)


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_mask_expansion(K):
    for form in ("modality", "class", "votes", [[2 * K - 1, 0], list(range(1, 2 * K - 1))]):
        groups = X._fusion_players("t", form, K)
        assert groups == R.players(form, K)
        masks = X._fusion_masks(groups, K)
        assert masks.dtype == np.uint32 and masks.shape == ((1 << len(groups)) + 4,)
        assert np.array_equal(masks[:-4], R.coalition_masks(groups))
        assert np.array_equal(masks[-4:], R.modality_masks(K))
    mod = X._fusion_masks(X._fusion_players("t", "modality", K), K)
    assert np.array_equal(mod[:4], mod[4:])                               # the modality game's own coalitions are its four masks


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
CH, T, H, W = 4, 64, 16, 16


def _mm(K=6):
    return brainxai.build_multimodal(CH, T, 1, num_classes=K)


def _inputs(B=2):
    return torch.zeros(B, 1, CH, T), torch.zeros(B, 1, H, W)


def _refused(exc, text, model, eeg, spec, background="uniform", **kw):
    with pytest.raises(exc, match=re.escape(text)):
        brainxai.fusion_shap(model, eeg, spec, background, **kw)


def test_refuses_a_stand_alone_model():
    eeg, spec = _inputs()
    for model in (brainxai.EEGNet(6, Chans=CH, Samples=T, kernLength=16), brainxai.Spectrogram_Model(6, in_channels=1)):
        _refused(ValueError, "fusion_shap: needs a MultimodalModel", model, eeg, spec)
        with pytest.raises(ValueError, match="fusion_votes: needs a MultimodalModel"):
            brainxai.fusion_votes(model, eeg, spec)


def test_refuses_a_foreign_head():
    model = _mm()
    model.fc1 = torch.nn.Linear(13, 128)
    _refused(ValueError, "the head must be Linear(2K,Hd) -> ReLU -> Linear(Hd,K)", model, *_inputs())
    model = _mm()
    model.fc1, model.fc2 = torch.nn.Linear(12, 8), torch.nn.Linear(8, 6)
    _refused(ValueError, "K = 6 classes and Hd = 8 hidden units; supported 1 <= K <= 16, 2K <= Hd <= 1024", model, *_inputs())


def test_refuses_votes_at_nine_classes():
    eeg, spec = _inputs()
    with pytest.raises(ValueError) as err:
        brainxai.fusion_shap(_mm(9), eeg, spec, "uniform", players="votes")
    assert "players='votes' has 2K = 18 players" in str(err.value) and "'modality'" in str(err.value) and "'class'" in str(err.value)
    # the coarser games of the same model pass every argument check and stop at the missing GPU
    for players in ("modality", "class"):
        _refused(RuntimeError, "there is no CPU path", _mm(9), eeg, spec, players=players)


def test_refuses_bad_partitions():
    model, (eeg, spec) = _mm(2), _inputs()
    for players, text in (([[0, 1], [1, 2, 3]], "vote 1 belongs to two players"),
                          ([[0, 1], [3]], "the players leave out the votes [2]"),
                          ([[0, 1, 2, 3], []], "an empty player"),
                          ([[0, 1, 2], [4]], "vote 4 outside range(4)"),
                          ([[0, 1, 2], [-1]], "vote -1 outside range(4)"),
                          ([[0.0, 1, 2, 3]], "vote 0.0 outside range(4)"),
                          ([], "0 players, supported 1..16"),
                          (7, "players must be 'votes', 'modality', 'class' or a list of lists of votes"),
                          ("branches", "unknown players 'branches'")):
        _refused(ValueError, text, model, eeg, spec, players=players)
    K = 9
    _refused(ValueError, "17 players, supported 1..16", _mm(K), eeg, spec, players=[[i] for i in range(16)] + [[16, 17]])


def test_refuses_bad_inputs_and_backgrounds():
    model, (eeg, spec) = _mm(), _inputs()
    _refused(ValueError, "the inputs have 3 EEG and 2 spectrogram samples", model, torch.zeros(3, 1, CH, T), spec)
    _refused(ValueError, "the inputs must be the tensors eeg [N,1,Chans,T] and spec [N,C,H,W]", model, None, spec)
    _refused(ValueError, "the background (eeg_bg, spec_bg) have 5 EEG and 4 spectrogram samples", model, eeg, spec,
             (torch.zeros(5, 1, CH, T), torch.zeros(4, 1, H, W)))
    _refused(ValueError, "the background samples are shaped", model, eeg, spec, (torch.zeros(5, 1, CH, T), torch.zeros(5, 1, H, W + 1)))
    _refused(ValueError, "the background holds 5 EEG and 4 spectrogram rows", model, eeg, spec, brainxai.FusionVotes(torch.zeros(5, 6), torch.zeros(4, 6)))
    _refused(ValueError, "a FusionVotes background holds two fp32 tensors [Nb, 6]", model, eeg, spec, brainxai.FusionVotes(torch.zeros(5, 5), torch.zeros(5, 5)))
    _refused(ValueError, "a FusionVotes background holds two fp32 tensors [Nb, 6]", model, eeg, spec,
             brainxai.FusionVotes(torch.zeros(5, 6, dtype=torch.float64), torch.zeros(5, 6)))
    _refused(ValueError, "unknown background 'zeros'", model, eeg, spec, "zeros")
    _refused(ValueError, "background must be 'uniform', (eeg_bg, spec_bg) or a FusionVotes, got Tensor", model, eeg, spec, torch.zeros(5, 6))


def test_refuses_bad_score_class_and_max_batch():
    model, (eeg, spec) = _mm(), _inputs()
    _refused(ValueError, "fusion_shap: unknown score 'logit'; use 'prob' or 'logprob'", model, eeg, spec, score="logit")
    _refused(ValueError, "fusion_shap: class outside [0, 6)", model, eeg, spec, class_idx=6)
    _refused(ValueError, "fusion_shap: class_idx 'every'", model, eeg, spec, class_idx="every")
    _refused(ValueError, "fusion_shap: class_idx must be None, an int, 'all' or 2 integers", model, eeg, spec, class_idx=[0, 1, 2])
    _refused(ValueError, "fusion_shap: max_batch = 0 < 1", model, eeg, spec, max_batch=0)


def test_refuses_the_cpu():
    model, (eeg, spec) = _mm(), _inputs()
    text = "brainxai.fusion_shap: the model, its inputs and the background must live on the GPU; there is no CPU path"
    _refused(RuntimeError, text, model, eeg, spec)
    _refused(RuntimeError, text, model, eeg, spec, (eeg, spec))
    _refused(RuntimeError, text, model, eeg, spec, brainxai.FusionVotes(torch.zeros(5, 6), torch.zeros(5, 6)))
    with pytest.raises(RuntimeError, match=re.escape("brainxai.fusion_votes: the model and its inputs must live on the GPU; there is no CPU path")):
        brainxai.fusion_votes(model, eeg, spec)
    with pytest.raises(RuntimeError, match=re.escape("brainxai.modality_importance: the values must live on the GPU; there is no CPU path")):
        brainxai.modality_importance(torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="modality_importance: values must be fusion_shap's values"):
        brainxai.modality_importance(torch.zeros(3))


def test_the_boundary_declares_the_entry_points():
    import os
    from brainxai import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "brainxai.h")).read()
    lib = _lib.load()
    for name in ("bx_fusion_values", "bx_shapley_exact", "bx_fusion_interaction"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/brainxai.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1, f"{name}: the ctypes signature does not match the header"
        assert hasattr(lib, name)
    assert (_lib.BX_FUSION_SCORE_PROB, _lib.BX_FUSION_SCORE_LOGPROB) == (0, 1)
    # limits are refused before any pointer is touched (no GPU needed)
    assert lib.bx_fusion_values(None, None, None, None, None, None, None, None, None, 0, None, 1, 1, 1, 17, 64, None) < 0
    assert b"1 <= K <= 16" in lib.bx_last_error_string()
    assert lib.bx_fusion_values(None, None, None, None, None, None, None, None, None, 0, None, 1, 1, 1, 6, 11, None) < 0
    assert lib.bx_fusion_values(None, None, None, None, None, None, None, None, None, 0, None, 1, 1, 1, 6, 1025, None) < 0
    assert lib.bx_fusion_values(None, None, None, None, None, None, None, None, None, 2, None, 1, 1, 1, 6, 128, None) < 0
    assert lib.bx_fusion_values(None, None, None, None, None, None, None, None, None, 0, None, 1, 1, 1, 6, 128, None) < 0
    assert b"null pointer" in lib.bx_last_error_string()
    assert lib.bx_shapley_exact(None, None, None, 1, 17, None) < 0 and lib.bx_shapley_exact(None, None, None, 1, 0, None) < 0
    assert lib.bx_shapley_exact(None, None, None, 1 << 16, 16, None) < 0
    assert lib.bx_fusion_interaction(None, None, 0, None) < 0
