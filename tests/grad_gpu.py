"""What the GPU tests of the sampled-gradient attributions and their scores (gradient_shap, smooth_grad, infidelity, sensitivity_max)
share: the per-(sample, class) error measure, and the models and inputs they are run on.  A plain module: no tests, no fixtures of
pytest's.  Everything cached here is computed once and never written to."""
import copy
import functools

import torch

import brainxai
from oracle import ref_torch as O
from tests import perturb_gpu as PG
from tests.perturb_gpu import DEV


def per_pair_max(t):
    t = torch.as_tensor(t).detach().double().cpu()
    return t.abs().flatten(2).max(2).values                                # [B, K]


def worst(got, want):
    """max over (sample, class) of max|got - want| / max|want|, for [B,K,...] of the same shape; got must be finite."""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all())
    return float((per_pair_max(got.detach().double().cpu() - want.detach().double().cpu()) / per_pair_max(want)).max())


def mm_inputs():
    return O.seeded((2, 1, 19, 2000), 12, "randn"), O.seeded((2, 4, 32, 64), 11, "rand")


@functools.lru_cache(maxsize=None)
def iface():
    """(model, eeg, spec) on the device: the scaled multimodal model and mm_inputs, for the interface tests."""
    _, mine = PG.scaled_multimodal()
    eeg, spec = mm_inputs()
    return mine, eeg.to(DEV), spec.to(DEV)


@functools.lru_cache(maxsize=None)
def backgrounds():
    """(EEG, spectrogram) background sets of gradient_shap on the device, Nb = 3 each."""
    return O.seeded((3, 1, 19, 2000), 14, "randn").to(DEV), O.seeded((3, 4, 32, 64), 13, "rand").to(DEV)


def eeg_models(kind):
    """-> (ref, mine, f64, x, other) of an EEG-input case: the oracle's model, the package's on the device with the same parameters, the
    oracle's in fp64, the explained input and the other input (None for the stand-alone 'eegnet' and 'deep')."""
    if kind == "eegnet":                                                  # the inputs of test_gpu_parity.test_expected_gradients_shap_style
        ref = O.fill_params(O.EEGNet(6, Chans=19, Samples=2000, dropoutRate=0.0), seed=31).eval()
        mine = brainxai.EEGNet(6, Chans=19, Samples=2000, dropoutRate=0.0)
        x, other = O.seeded((2, 1, 19, 2000), 91, "randn"), None
    elif kind == "deep":
        ref = O.fill_params(O.EEGNetAttentionDeep(6, Chans=19, Samples=2000, dropoutRate=0.0), seed=61).eval()
        mine = brainxai.EEGNetAttentionDeep(6, Chans=19, Samples=2000, dropoutRate=0.0)
        x, other = mm_inputs()[0], None
    else:
        ref, mine = PG.scaled_multimodal()
        x, other = mm_inputs()
    if kind != "multimodal":
        mine.load_state_dict(ref.state_dict())
        mine = mine.to(DEV).eval()
    return ref, mine, copy.deepcopy(ref).double().eval(), x, other
