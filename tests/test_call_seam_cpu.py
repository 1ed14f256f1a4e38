"""CPU: the seam the attribution drivers share before their pass -- the input's name, the tensors, the model and the explained classes,
the closing GPU refusal -- for the drivers tests/test_perturb_refusals_cpu.py does not cover: gradient_shap, smooth_grad, blur_ig,
guided_ig, mask_explain, spectral_gradients, spectral_occlusion, infidelity, sensitivity_max and tcav.  Exact texts, and which of two
errors is reported when two are present; the drivers do not all order their checks alike (tcav looks at max_batch before anything
else, sensitivity_max has no model and no classes), and the table records what each does.  Tiny models and inputs; nothing reaches
the library."""
from types import SimpleNamespace

import pytest
import torch

import brainxai
from brainxai import _lib

B, H, W, CH, T, K = 2, 16, 16, 4, 64, 6


def _models(kind):
    if kind == "multimodal":
        return brainxai.build_multimodal(CH, T, 1)
    if kind == "spectrogram":
        return brainxai.Spectrogram_Model(K, in_channels=1)
    return brainxai.EEGNet(K, Chans=CH, Samples=T, kernLength=16)


def _call(fn, kind, kw):
    kw = dict(kw)
    eeg = kw.pop("eeg", torch.zeros(B, 1, CH, T))
    spec = kw.pop("spec", torch.zeros(B, 1, H, W))
    model = _models(kind)
    tail = (1, CH, T) if kw.get("input") == "eeg" or fn.startswith("spectral") else (1, H, W)
    if fn == "gradient_shap":
        return brainxai.gradient_shap(model, eeg, spec, torch.zeros(3, *tail), **kw)
    if fn == "infidelity":
        lead = (B, K) if isinstance(kw.get("class_idx"), str) and kw["class_idx"] == "all" else (B,)   # 'all' scores a map per class
        return brainxai.infidelity(model, eeg, spec, torch.zeros(*lead, *tail[1:]), **kw)
    if fn == "sensitivity_max":
        return brainxai.sensitivity_max(lambda e, s, sample: s, eeg, spec, **kw)
    if fn == "tcav":
        kw.setdefault("target_layer", None if kw.get("input") == "eeg" else "block3")   # 16 x 16 does not reach block5
        return brainxai.tcav(model, eeg, spec, {"c": torch.zeros(2, *tail)}, [torch.zeros(2, *tail)], **kw)
    if fn == "blur_ig":
        kw.update(steps=3, max_sigma=1.0)                                                # a blur that fits 16 x 16
    if fn == "spectral_occlusion":
        kw.setdefault("bands", [(0.0, 0.25)])
    return getattr(brainxai, fn)(model, eeg, spec, **kw)


UNKNOWN = "unknown input 'both'; use 'spec' or 'eeg'"
MAX_BATCH = "max_batch = 0 < 1"
BOTH_INPUTS = "a MultimodalModel needs both inputs with the same batch size"
CLASS_HIGH = f"class outside [0, {K})"
GPU = {"gradient_shap": "the model, its inputs and the background", "infidelity": "the model, its inputs and the attribution",
       "sensitivity_max": "the inputs"}

CASES = []                                                            # (function, model kind, keywords, exception, exact message)


def _add(name, fn, kind, kw, exc, msg):
    CASES.append(pytest.param(fn, kind, kw, exc, msg, id=f"{fn}-{name}"))


# the drivers with an ``input`` argument, a model and classes
for who in ("gradient_shap", "smooth_grad", "blur_ig", "guided_ig", "mask_explain", "infidelity", "tcav"):
    first = MAX_BATCH if who == "tcav" else UNKNOWN                   # tcav checks max_batch before anything else
    for name, kind, kw, msg in [
        ("input_unknown_and_max_batch", "multimodal", dict(input="both", max_batch=0), first),
        ("input_unknown", "multimodal", dict(input="both"), "input must be 'spec' or 'eeg', got 'both'" if who == "tcav" else UNKNOWN),
        ("max_batch_and_none", "spectrogram", dict(input="eeg", eeg=None, max_batch=0), MAX_BATCH),
        ("none_eeg", "eegnet", dict(input="eeg", eeg=None), "input='eeg' but that tensor is None"),
        ("none_spec", "spectrogram", dict(input="spec", spec=None), "input='spec' but that tensor is None"),
        ("rank_eeg", "eegnet", dict(input="eeg", eeg=torch.zeros(B, CH, T)), "the eeg input must be a tensor [B,1,Chans,T]"),
        ("batch_mismatch_and_class_word", "multimodal", dict(input="spec", eeg=torch.zeros(B + 1, 1, CH, T), class_idx="every"), BOTH_INPUTS),
        ("batch_mismatch_eeg_and_class_word", "multimodal", dict(input="eeg", spec=torch.zeros(B + 1, 1, H, W), class_idx="every"), BOTH_INPUTS),
        ("other_none", "multimodal", dict(input="spec", eeg=None), BOTH_INPUTS),
        ("class_word", "multimodal", dict(input="spec", class_idx="every"), "class_idx 'every'; use None, an int, one class per sample or 'all'"),
        ("class_high", "multimodal", dict(input="spec", class_idx=K), CLASS_HIGH),
        ("class_high_eeg", "eegnet", dict(input="eeg", class_idx=[0, K]), CLASS_HIGH),
    ]:
        _add(name, who, kind, kw, ValueError, f"{who}: {msg}")
    if who != "tcav":                                                 # tcav words the wrong model by its target (below)
        _add("model_for_spec_and_class_high", who, "eegnet", dict(input="spec", class_idx=K), ValueError,
             f"{who}: input='spec' needs a MultimodalModel or a Spectrogram_Model")
    for name, kind, kw in [("cpu_multimodal", "multimodal", dict(input="spec")), ("cpu_multimodal_eeg_all", "multimodal", dict(input="eeg", class_idx="all")),
                           ("cpu_spectrogram", "spectrogram", dict(input="spec", class_idx=[1, 2])),
                           ("cpu_eegnet", "eegnet", dict(input="eeg", class_idx=torch.tensor([5, 0])))]:
        _add(name, who, kind, kw, RuntimeError, f"brainxai.{who}: {GPU.get(who, 'the model and its inputs')} must live on the GPU; there is no CPU path")

_add("model_for_spec_and_class_high", "tcav", "eegnet", dict(input="spec", class_idx=K), ValueError, "tcav: input='spec' needs a MultimodalModel or a Spectrogram_Model")
_add("target_and_none", "tcav", "multimodal", dict(input="spec", spec=None, target_layer="block6"), ValueError,
     "tcav: unknown target_layer 'block6'; use 'spectrogram_model.blockN[.convK]' (input='spec') or 'eeg_model.features' (input='eeg')")
_add("class_high_and_shape", "tcav", "multimodal", dict(input="spec", class_idx=K, target_layer="block5"), ValueError, f"tcav: {CLASS_HIGH}")
_add("shape_and_cpu", "tcav", "multimodal", dict(input="spec", target_layer="block5"), ValueError, "tcav: a spectrogram of 16 x 16 does not reach block5")

# the two that fix input='eeg'
for who in ("spectral_gradients", "spectral_occlusion"):
    for name, kind, kw, msg in [
        ("max_batch_and_none", "eegnet", dict(eeg=None, max_batch=0), MAX_BATCH),
        ("none_eeg", "eegnet", dict(eeg=None), "input='eeg' but that tensor is None"),
        ("eeg_planes", "eegnet", dict(eeg=torch.zeros(B, 2, CH, T)), "the eeg input must be a tensor [B,1,Chans,T]"),
        ("batch_mismatch_and_class_word", "multimodal", dict(spec=torch.zeros(B + 1, 1, H, W), class_idx="every"), BOTH_INPUTS),
        ("other_none", "multimodal", dict(spec=None), BOTH_INPUTS),
        ("wrong_model_and_class_high", "spectrogram", dict(class_idx=K), "input='eeg' needs a MultimodalModel, an EEGNet or an EEGNetAttentionDeep"),
        ("class_word", "multimodal", dict(class_idx="every"), "class_idx 'every'; use None, an int, one class per sample or 'all'"),
        ("class_high", "multimodal", dict(class_idx=K), CLASS_HIGH),
    ]:
        _add(name, who, kind, kw, ValueError, f"{who}: {msg}")
    for name, kind, kw in [("cpu_multimodal", "multimodal", dict()), ("cpu_multimodal_all", "multimodal", dict(class_idx="all")),
                           ("cpu_eegnet", "eegnet", dict(spec=None, class_idx=[5, 0]))]:
        _add(name, who, kind, kw, RuntimeError, f"brainxai.{who}: the model and its inputs must live on the GPU; there is no CPU path")

# sensitivity_max: an input's name and tensors, no model and no classes
who = "sensitivity_max"
for name, kw, msg in [
    ("input_unknown_and_max_batch", dict(input="both", max_batch=0), UNKNOWN),
    ("max_batch_and_none", dict(input="eeg", eeg=None, max_batch=0), MAX_BATCH),
    ("none_spec", dict(input="spec", spec=None), "input='spec' but that tensor is None"),
    ("rank_spec", dict(input="spec", spec=torch.zeros(B, H, W)), "the spec input must be a tensor [B,C,H,W]"),
    ("batch_mismatch", dict(input="spec", eeg=torch.zeros(B + 1, 1, CH, T)), "the other input must be None or a tensor with the same batch size"),
    ("batch_mismatch_eeg", dict(input="eeg", spec=torch.zeros(B + 1, 1, H, W)), "the other input must be None or a tensor with the same batch size"),
]:
    _add(name, who, "multimodal", kw, ValueError, f"{who}: {msg}")
for name, kw in [("cpu_both", dict(input="spec")), ("cpu_eeg_alone", dict(input="eeg", spec=None))]:
    _add(name, who, "multimodal", kw, RuntimeError, f"brainxai.{who}: the inputs must live on the GPU; there is no CPU path")


@pytest.mark.parametrize("fn, kind, kw, exc, msg", CASES)
def test_refusal_text(monkeypatch, fn, kind, kw, exc, msg):
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
    with pytest.raises(exc) as err:
        _call(fn, kind, kw)
    assert str(err.value) == msg
    assert reached == [], f"library entry points reached: {reached}"
