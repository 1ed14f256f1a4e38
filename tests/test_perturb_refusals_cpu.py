"""CPU: the exact refusal texts of the five perturb-and-predict drivers (deletion_insertion, rise, occlusion, kernel_shap, score_cam)
for the argument errors their shared checks cover, and which of two errors is reported when two are present.  Tiny models and inputs;
nothing reaches the library."""
from types import SimpleNamespace

import pytest
import torch

import brainxai
from brainxai import _lib

B, H, W, CH, T, K = 2, 16, 16, 4, 64, 6
S5 = "spectrogram_model.block5"
DW = "eeg_model.depthwiseConv"


def _models(kind):
    if kind == "multimodal":
        return brainxai.build_multimodal(CH, T, 1)
    if kind.startswith("spectrogram"):
        return brainxai.Spectrogram_Model(33 if kind.endswith("33") else K, in_channels=1)
    return brainxai.EEGNet(33 if kind.endswith("33") else K, Chans=CH, Samples=T, kernLength=16)


def _call(fn, kind, kw):
    kw = dict(kw)
    eeg = kw.pop("eeg", torch.zeros(B, 1, CH, T))
    spec = kw.pop("spec", torch.zeros(B, 1, H, W))
    model = _models(kind)
    if fn == "score_cam":
        target = kw.pop("target", S5)
        return brainxai.score_cam(model, eeg, spec, target, **kw)
    inp = kw.get("input", "spec")
    if fn == "deletion_insertion":
        kw.setdefault("attribution", torch.zeros(B, CH, T) if inp == "eeg" else torch.zeros(B, H, W))
        return brainxai.deletion_insertion(model, eeg, spec, kw.pop("attribution"), **kw)
    if fn == "occlusion":
        kw.setdefault("window", 4)
    if fn == "rise":
        kw.setdefault("grid", 2)                                      # fits the 4 electrode rows of the EEG domain too
    if fn == "kernel_shap":
        kw.setdefault("segments", (2, 2))
    return getattr(brainxai, fn)(model, eeg, spec, **kw)


GPU = {"deletion_insertion": "brainxai.deletion_insertion: the model, its inputs and the attribution must live on the GPU; there is no CPU path",
       "rise": "brainxai.rise: the model and its inputs must live on the GPU; there is no CPU path",
       "occlusion": "brainxai.occlusion: the model and its inputs must live on the GPU; there is no CPU path",
       "kernel_shap": "brainxai.kernel_shap: the model and its inputs must live on the GPU; there is no CPU path",
       "score_cam": "brainxai.score_cam: the model and its inputs must live on the GPU; there is no CPU path"}
SHAPE_MSG = ("baseline of shape {} is none of: a number, one value per {} [{}], a tensor of the input's shape {}")

CASES = []                                                            # (id, function, model kind, keywords, exception, exact message)


def _add(name, fn, kind, kw, exc, msg):
    CASES.append(pytest.param(fn, kind, kw, exc, msg, id=f"{fn}-{name}"))


for who in ("deletion_insertion", "rise", "occlusion", "kernel_shap"):
    all_ok = who != "deletion_insertion"
    use = "use None, an int, one class per sample or 'all'" if all_ok else "use None, an int or one class per sample"
    must = f"must be None, an int, 'all' or {B} integers (one class per sample)" if all_ok else f"must be None, an int or {B} integers (one class per sample)"
    for name, kind, kw, exc, msg in [
        ("input_unknown", "multimodal", dict(input="both"), ValueError, "unknown input 'both'; use 'spec' or 'eeg'"),
        ("input_unknown_and_max_batch", "multimodal", dict(input="both", max_batch=0), ValueError, "unknown input 'both'; use 'spec' or 'eeg'"),
        ("max_batch_and_none", "spectrogram", dict(input="eeg", eeg=None, max_batch=0), ValueError, "max_batch = 0 < 1"),
        ("none_eeg", "spectrogram", dict(input="eeg", eeg=None), ValueError, "input='eeg' but that tensor is None"),
        ("none_spec", "eegnet", dict(spec=None), ValueError, "input='spec' but that tensor is None"),
        ("not_a_tensor", "spectrogram", dict(spec=[[1.0]]), ValueError, "the spec input must be a tensor [B,C,H,W]"),
        ("rank_spec", "spectrogram", dict(spec=torch.zeros(B, H, W)), ValueError, "the spec input must be a tensor [B,C,H,W]"),
        ("rank_eeg", "eegnet", dict(input="eeg", eeg=torch.zeros(B, CH, T)), ValueError, "the eeg input must be a tensor [B,1,Chans,T]"),
        ("eeg_planes", "eegnet", dict(input="eeg", eeg=torch.zeros(B, 2, CH, T)), ValueError, "the eeg input must be a tensor [B,1,Chans,T]"),
        ("channels_0", "spectrogram", dict(spec=torch.zeros(B, 0, H, W)), ValueError, "0 channels, supported 1..4"),
        ("channels_5", "spectrogram", dict(spec=torch.zeros(B, 5, H, W)), ValueError, "5 channels, supported 1..4"),
        ("channels_5_and_wrong_model", "eegnet", dict(spec=torch.zeros(B, 5, H, W)), ValueError, "5 channels, supported 1..4"),
        ("batch_mismatch", "multimodal", dict(eeg=torch.zeros(B + 1, 1, CH, T)), ValueError, "a MultimodalModel needs both inputs with the same batch size"),
        ("batch_mismatch_eeg", "multimodal", dict(input="eeg", spec=torch.zeros(B + 1, 1, H, W)), ValueError,
         "a MultimodalModel needs both inputs with the same batch size"),
        ("other_none", "multimodal", dict(eeg=None), ValueError, "a MultimodalModel needs both inputs with the same batch size"),
        ("batch_mismatch_and_class_word", "multimodal", dict(eeg=torch.zeros(B + 1, 1, CH, T), class_idx="every"), ValueError,
         "a MultimodalModel needs both inputs with the same batch size"),
        ("model_for_spec", "eegnet", dict(), ValueError, "input='spec' needs a MultimodalModel or a Spectrogram_Model"),
        ("model_for_eeg", "spectrogram", dict(input="eeg"), ValueError, "input='eeg' needs a MultimodalModel, an EEGNet or an EEGNetAttentionDeep"),
        ("model_for_spec_and_class_high", "eegnet", dict(class_idx=K), ValueError, "input='spec' needs a MultimodalModel or a Spectrogram_Model"),
        ("class_word", "multimodal", dict(class_idx="every"), ValueError, f"class_idx 'every'; {use}"),
        ("class_bool", "multimodal", dict(class_idx=True), ValueError, f"class_idx {must}"),
        ("class_float_tensor", "spectrogram", dict(class_idx=torch.tensor([0.0, 1.0])), ValueError, f"class_idx {must}"),
        ("class_bool_tensor", "spectrogram", dict(class_idx=torch.tensor([True, False])), ValueError, f"class_idx {must}"),
        ("class_length", "multimodal", dict(class_idx=[0, 1, 2]), ValueError, f"class_idx {must}"),
        ("class_matrix", "eegnet", dict(input="eeg", class_idx=[[0, 1]]), ValueError, f"class_idx {must}"),
        ("class_high", "multimodal", dict(class_idx=K), ValueError, f"class outside [0, {K})"),
        ("class_negative_in_list", "eegnet", dict(input="eeg", class_idx=[0, -1]), ValueError, f"class outside [0, {K})"),
        ("class_word_and_baseline", "multimodal", dict(class_idx="every", baseline=[0.0, 1.0]), ValueError, f"class_idx 'every'; {use}"),
        ("class_high_and_baseline", "spectrogram", dict(class_idx=[0, K], baseline="zero"), ValueError, f"class outside [0, {K})"),
        ("baseline_word", "multimodal", dict(baseline="zero"), ValueError,
         "baseline is neither a number, a sequence nor a tensor (could not convert string to float: 'zero')"),
        ("baseline_length", "multimodal", dict(baseline=[0.0, 1.0]), ValueError, SHAPE_MSG.format((2,), "channel", 1, (B, 1, H, W))),
        ("baseline_shape", "spectrogram", dict(baseline=torch.zeros(B, 1, H, W - 1)), ValueError,
         SHAPE_MSG.format((B, 1, H, W - 1), "channel", 1, (B, 1, H, W))),
        ("baseline_per_channel_for_eeg", "eegnet", dict(input="eeg", baseline=torch.zeros(CH + 1)), ValueError,
         SHAPE_MSG.format((CH + 1,), "electrode", CH, (B, 1, CH, T))),
        ("baseline_matrix_for_eeg", "multimodal", dict(input="eeg", baseline=torch.zeros(CH, T)), ValueError,
         SHAPE_MSG.format((CH, T), "electrode", CH, (B, 1, CH, T))),
        ("baseline_and_cpu", "multimodal", dict(baseline=[[0.0]]), ValueError, SHAPE_MSG.format((1, 1), "channel", 1, (B, 1, H, W))),
    ]:
        _add(name, who, kind, kw, exc, f"{who}: {msg}")
    for name, kind, kw in [("cpu_multimodal", "multimodal", dict()), ("cpu_multimodal_eeg", "multimodal", dict(input="eeg", baseline=torch.zeros(CH))),
                           ("cpu_spectrogram", "spectrogram", dict(class_idx=[1, 2], baseline=torch.zeros(B, 1, H, W))),
                           ("cpu_spectrogram_squeezed_baseline", "spectrogram", dict(baseline=torch.zeros(B, H, W))),
                           ("cpu_eegnet", "eegnet", dict(input="eeg", class_idx=torch.tensor([5, 0]), baseline=True))]:
        _add(name, who, kind, kw, RuntimeError, GPU[who])

# more than 32 classes: deletion_insertion has no such limit, the others refuse before they look at class_idx
_add("classes_33", "deletion_insertion", "spectrogram33", dict(), RuntimeError, GPU["deletion_insertion"])
for who in ("rise", "occlusion", "kernel_shap"):
    _add("classes_33", who, "spectrogram33", dict(), ValueError, f"{who}: 33 classes, supported 1..32")
    _add("classes_33_eeg", who, "eegnet33", dict(input="eeg"), ValueError, f"{who}: 33 classes, supported 1..32")
    _add("classes_33_and_class_word", who, "spectrogram33", dict(class_idx="every"), ValueError, f"{who}: 33 classes, supported 1..32")
    _add("class_all_cpu", who, "multimodal", dict(class_idx="all"), RuntimeError, GPU[who])
_add("class_all", "deletion_insertion", "multimodal", dict(class_idx="all"), ValueError,
     "deletion_insertion: class_idx 'all'; use None, an int or one class per sample")

# checks of one driver on either side of the shared ones
_add("steps_and_wrong_model", "deletion_insertion", "eegnet", dict(steps=0), ValueError, f"deletion_insertion: steps = 0 outside 1..N = {H * W}")
_add("channels_and_map_shape", "deletion_insertion", "spectrogram", dict(spec=torch.zeros(B, 5, H, W), attribution=torch.zeros(B, H)), ValueError,
     "deletion_insertion: 5 channels, supported 1..4")
_add("mode_and_none", "deletion_insertion", "spectrogram", dict(input="eeg", eeg=None, mode="neither"), ValueError,
     "deletion_insertion: unknown mode 'neither'; use one of 'both', 'deletion', 'insertion'")
_add("grid_and_wrong_model", "rise", "eegnet", dict(grid=0), ValueError, "rise: grid 0 x 0 outside 1..min(32, 16) x 1..min(32, 16)")
_add("baseline_and_p1", "rise", "multimodal", dict(baseline=[0.0, 1.0], p1=2.0), ValueError, "rise: " + SHAPE_MSG.format((2,), "channel", 1, (B, 1, H, W)))
_add("class_high_and_p1", "rise", "multimodal", dict(class_idx=K, p1=2.0), ValueError, f"rise: class outside [0, {K})")
_add("p1_and_cpu", "rise", "multimodal", dict(p1=2.0), ValueError, "rise: p1 = 2.0 outside (0, 1]")
_add("window_and_wrong_model", "occlusion", "eegnet", dict(window=17), ValueError, "occlusion: window 17 x 17 outside 1..16 x 1..16")
_add("score_and_none", "occlusion", "spectrogram", dict(input="eeg", eeg=None, score="logit"), ValueError,
     "occlusion: unknown score 'logit'; use 'prob' or 'logprob'")

who = "score_cam"
use = "use None, an int, one class per sample or 'all'"
must = f"must be None, an int, 'all' or {B} integers (one class per sample)"
for name, kind, kw, exc, msg in [
    ("target_unknown", "multimodal", dict(target="both"), ValueError,
     "unsupported target 'both'; use 'spectrogram_model.blockN[.convK]', 'eeg_model.depthwiseConv' or 'eeg_model.separableConv'"),
    ("max_batch_and_none", "eegnet", dict(spec=None, max_batch=0), ValueError, "max_batch = 0 < 1"),
    ("none_spec", "eegnet", dict(spec=None), ValueError, f"target '{S5}' reads the spectrogram input, but that tensor is None"),
    ("none_eeg", "spectrogram", dict(target=DW, eeg=None), ValueError, f"target '{DW}' reads the EEG input, but that tensor is None"),
    ("rank_spec", "spectrogram", dict(spec=torch.zeros(B, H, W)), ValueError, "the spectrogram input must be a tensor [B,C,H,W]"),
    ("rank_eeg", "eegnet", dict(target=DW, eeg=torch.zeros(B, CH, T)), ValueError, "the EEG input must be a tensor [B,1,Chans,T]"),
    ("eeg_planes", "eegnet", dict(target=DW, eeg=torch.zeros(B, 2, CH, T)), ValueError, "the EEG input must be a tensor [B,1,Chans,T]"),
    ("batch_mismatch", "multimodal", dict(eeg=torch.zeros(B + 1, 1, CH, T)), ValueError, "a MultimodalModel needs both inputs with the same batch size"),
    ("batch_mismatch_eeg", "multimodal", dict(target=DW, spec=torch.zeros(B + 1, 1, H, W)), ValueError,
     "a MultimodalModel needs both inputs with the same batch size"),
    ("other_none", "multimodal", dict(eeg=None), ValueError, "a MultimodalModel needs both inputs with the same batch size"),
    ("model_for_spec", "eegnet", dict(), ValueError, "a spectrogram target needs a MultimodalModel or a Spectrogram_Model"),
    ("model_for_eeg", "spectrogram", dict(target=DW), ValueError, "an EEG target needs a MultimodalModel, an EEGNet or an EEGNetAttentionDeep"),
    ("wrong_model_and_channels_5", "eegnet", dict(spec=torch.zeros(B, 5, H, W)), ValueError,
     "a spectrogram target needs a MultimodalModel or a Spectrogram_Model"),
    ("batch_mismatch_and_channels_5", "multimodal", dict(spec=torch.zeros(B, 5, H, W), eeg=torch.zeros(B + 1, 1, CH, T)), ValueError,
     "a MultimodalModel needs both inputs with the same batch size"),
    ("channels_0", "spectrogram", dict(spec=torch.zeros(B, 0, H, W)), ValueError, "0 channels, supported 1..4"),
    ("channels_5", "spectrogram", dict(spec=torch.zeros(B, 5, H, W)), ValueError, "5 channels, supported 1..4"),
    ("channels_5_and_classes_33", "spectrogram33", dict(spec=torch.zeros(B, 5, H, W)), ValueError, "5 channels, supported 1..4"),
    ("classes_33", "spectrogram33", dict(), ValueError, "33 classes, supported 1..32"),
    ("classes_33_eeg", "eegnet33", dict(target=DW), ValueError, "33 classes, supported 1..32"),
    ("classes_33_and_class_word", "spectrogram33", dict(class_idx="every"), ValueError, "33 classes, supported 1..32"),
    ("class_word", "multimodal", dict(class_idx="every"), ValueError, f"class_idx 'every'; {use}"),
    ("class_bool", "multimodal", dict(class_idx=True), ValueError, f"class_idx {must}"),
    ("class_float_tensor", "spectrogram", dict(class_idx=torch.tensor([0.0, 1.0])), ValueError, f"class_idx {must}"),
    ("class_length", "multimodal", dict(class_idx=[0, 1, 2]), ValueError, f"class_idx {must}"),
    ("class_high", "multimodal", dict(class_idx=K), ValueError, f"class outside [0, {K})"),
    ("class_negative_in_list", "eegnet", dict(target=DW, class_idx=[0, -1]), ValueError, f"class outside [0, {K})"),
    ("class_word_and_baseline", "multimodal", dict(class_idx="every", baseline=[0.0, 1.0]), ValueError, f"class_idx 'every'; {use}"),
    ("class_high_and_baseline", "spectrogram", dict(class_idx=[0, K], baseline="zero"), ValueError, f"class outside [0, {K})"),
    ("baseline_word", "multimodal", dict(baseline="zero"), ValueError,
     "baseline is neither a number, a sequence nor a tensor (could not convert string to float: 'zero')"),
    ("baseline_length", "multimodal", dict(baseline=[0.0, 1.0]), ValueError, SHAPE_MSG.format((2,), "channel", 1, (B, 1, H, W))),
    ("baseline_shape", "spectrogram", dict(baseline=torch.zeros(B, 1, H, W - 1)), ValueError, SHAPE_MSG.format((B, 1, H, W - 1), "channel", 1, (B, 1, H, W))),
    ("baseline_per_channel_for_eeg", "eegnet", dict(target=DW, baseline=torch.zeros(CH + 1)), ValueError,
     SHAPE_MSG.format((CH + 1,), "electrode", CH, (B, 1, CH, T))),
    ("weights_and_none", "eegnet", dict(spec=None, weights="softmax"), ValueError, "unknown weights 'softmax'; use 'prob' or 'increase'"),
]:
    _add(name, who, kind, kw, exc, f"{who}: {msg}")
for name, kind, kw in [("cpu_multimodal", "multimodal", dict()), ("cpu_multimodal_all", "multimodal", dict(class_idx="all", weights="increase")),
                       ("cpu_multimodal_eeg", "multimodal", dict(target=DW, baseline=torch.zeros(CH))),
                       ("cpu_spectrogram", "spectrogram", dict(target="block3.conv2", class_idx=[1, 2], baseline=torch.zeros(B, 1, H, W))),
                       ("cpu_eegnet", "eegnet", dict(target="separableConv", class_idx=torch.tensor([5, 0])))]:
    _add(name, who, kind, kw, RuntimeError, GPU[who])


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


def test_faith_baseline_keeps_its_name_and_wording():
    from brainxai import explain as X
    x = torch.zeros(B, 1, H, W)
    assert X._faith_baseline(0.5, x, 1, "channel")[0] == 0 and X._faith_baseline([1.0], x, 1, "channel")[0] == 1
    assert X._faith_baseline(torch.zeros(B, H, W), x, 1, "channel")[0] == 2
    with pytest.raises(ValueError) as err:
        X._faith_baseline([0.0, 1.0], x, 1, "channel")
    assert str(err.value) == "deletion_insertion: " + SHAPE_MSG.format((2,), "channel", 1, (B, 1, H, W))
