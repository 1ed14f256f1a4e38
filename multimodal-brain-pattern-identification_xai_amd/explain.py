"""Attribution over the multimodal model on the HIP path.

* ``grad_cam``                -- canonical Grad-CAM (the reference ships none): forward,
                                 backward from the class score to the target layer only, then the fused
                                 activation x gradient channel-reduce kernel (bx_cam_reduce); method=
                                 'gradcam++' / 'layercam' for Grad-CAM++ and Layer-CAM at every target.
* ``saliency`` / ``generate_saliency_maps`` -- reference XAI_Multimodality.py:3101-3133.
* ``integrated_gradients``    -- Captum-default semantics (imported but never called by the reference, NB:51).
* ``lime_image``              -- LIME for images as lime 0.2.0.1's explain_instance defines it (reference
                                 XAI_Multimodality.py:1658-1670): perturbed batch, forward passes and the weighted
                                 ridge surrogate on the GPU (bx_lime_*); ``predict_fn`` is its callback alone.
* ``deletion_insertion``      -- deletion / insertion curves of any of those maps (the causal metric of RISE, Petsiuk et al.,
                                 BMVC 2018; not in the reference): exact ranks (``attribution_ranks``, bx_rank_desc), perturbed
                                 batches in the model's layout (bx_faith_perturb_*), forward passes, curves and areas (bx_faith_curve).
* ``rise``                    -- RISE saliency (the same paper; not in the reference): black-box maps of either input from randomly
                                 masked forward passes; the masks are recomputed from their bit grids inside the perturb and
                                 weighted-sum kernels (bx_rise_perturb_*, bx_rise_accumulate) and never stored; ``rise_masks`` builds them.
* ``score_cam``               -- Score-CAM (Wang et al., CVPR-W 2020; not in the reference): a class-activation map at every Grad-CAM
                                 target but conv1 whose channel weights are class probabilities of the input seen through each
                                 up-sampled activation channel; the masks are recomputed from the activation planes inside the range
                                 and perturb kernels (bx_scorecam_range, bx_scorecam_perturb_*) and never stored; fp64 channel sum
                                 (bx_scorecam_combine).
* ``occlusion``               -- occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's Occlusion; not in the reference): the
                                 drop of the class score when a sliding window of either input shows the baseline -- electrode or
                                 time-segment ablation on the EEG input, band or slab ablation on the spectrogram; deterministic; the
                                 occluded rows are a selection written in the model's layout (bx_occlusion_perturb_*), the map an
                                 fp64 mean over the covering windows in fixed order (bx_occlusion_accumulate).
* ``kernel_shap``             -- Kernel SHAP (Lundberg & Lee, NeurIPS 2017; the reference's SHAP is a GradientExplainer on the EEG branch,
                                 reduced to per-electrode importances): Shapley values of the segments of either input -- electrodes,
                                 time slabs, a time-by-frequency grid -- from forward passes of coalitions; exact for few players,
                                 paired sampling otherwise; the values add up to score(input) - score(baseline).  The rows are a
                                 selection written in the model's layout (bx_shap_perturb_*), the constrained fit is fp64 in fixed
                                 order (bx_shap_fit), the map the values gathered through the label map (bx_shap_value_map).
* ``gradient_shap``           -- expected gradients (SHAP's GradientExplainer, reference XAI_Multimodality.py:2283-2290) of either input
                                 of the multimodal model or of a stand-alone branch, batched over samples, draws and classes: the
                                 interpolants of a pass in one launch (bx_expgrad_rows), one forward pass for all classes, an fp64 running
                                 sum in fixed draw order after every backward pass (bx_expgrad_accumulate), the mean and the
                                 channel-summed map (bx_expgrad_finish).  ``channel_importance`` is the reference's mean |.| per
                                 electrode (bx_mean_abs_rows), ``GradientExplainer`` SHAP's calling form.  ``expected_gradients`` is
                                 the same estimator as a host loop over one stand-alone model.
* ``smooth_grad``             -- SmoothGrad, SmoothGrad^2 and VarGrad (Smilkov et al. 2017; Hooker et al. 2019; Captum's NoiseTunnel, which
                                 the reference imports) of either input of the multimodal model or of a stand-alone branch: the
                                 Gaussian noise is drawn in registers from Philox4x32-10 counters while the noisy rows of a pass are
                                 written (bx_smoothgrad_sigma, bx_smoothgrad_rows) and never stored, one forward pass for all
                                 classes, fp64 running sums of the gradient and its square in fixed draw order
                                 (bx_smoothgrad_accumulate), the mean / mean square / variance and the channel-max map
                                 (bx_smoothgrad_finish).  ``smooth_grad_noise`` returns the draws.
* ``blur_ig``                 -- Blur Integrated Gradients (Xu et al., CVPR 2020; saliency.BlurIG; not in the reference): integrated
                                 gradients along the path through Gaussian scale space, without a baseline, of either input; the
                                 blurred rows of a pass and their scale derivative come from one launch of separable filters
                                 (bx_blur_rows), an fp64 running sum of w * gradient * derivative in fixed step order
                                 (bx_blurig_accumulate), the completeness error from fp64 row sums (bx_blurig_sum_rows).
                                 ``blur_path`` returns the rows, ``gaussian_blur`` is the same kernel as a plain blur.
* ``guided_ig``               -- Guided Integrated Gradients (Kapishnikov et al., CVPR 2021; saliency.GuidedIG; not in the reference):
                                 the adaptive path from a baseline to the input on which, at every step, only the cells with the
                                 smallest |gradient| move; every (sample, class) pair walks its own path, and a step's whole inner
                                 loop -- clamp, fp64 sums, the exact k-th smallest |gradient| by a radix select, move, fp64
                                 attribution -- is one launch (bx_guided_ig_init, bx_guided_ig_step) between the model's passes.
* ``spectral_gradients`` / ``spectral_occlusion`` -- the EEG input explained by frequency (Schirrmeister et al. 2017; braindecode's
                                 compute_amplitude_gradients; not in the reference): a real DFT of any length as a direct fp64 sum over a
                                 host-made twiddle table (bx_rdft_rows), the path-weighted gradient summed in fp64 in fixed step order
                                 (bx_spectral_accumulate), amplitude gradient / gradient x amplitude per bin with the gradient's
                                 transform in registers (bx_spectral_values), band sums (bx_band_sum); forward-only, the drop of the
                                 score with a band removed, rows written in the EEG layout (bx_bandstop_rows).  ``eeg_spectrum``
                                 returns the transform, ``band_sums`` reduces any per-bin map.
* ``infidelity`` / ``sensitivity_max`` -- the two measures of Yeh et al. (NeurIPS 2019; Captum's metrics.infidelity and
                                 metrics.sensitivity_max) for any of those maps: rows minus SmoothGrad's Gaussian stream written in the
                                 model's layout (bx_infidelity_rows_*), the fp64 dot of the same noise with the attribution in fixed
                                 order (bx_infidelity_dot), drops, beta and the mean square (bx_infidelity_finish); uniformly perturbed
                                 rows (bx_sensitivity_rows), fp64 distances of the caller's explanations (bx_sensitivity_dist) and
                                 the largest relative one (bx_sensitivity_finish).
* ``map_similarity`` / ``agreement_matrix`` / ``randomization_test`` -- the sanity checks of Adebayo et al. (NeurIPS 2018): Spearman's
                                 correlation over tie-averaged ranks (bx_rank_desc, bx_rank_average), Pearson's in fp64 (bx_map_corr), the
                                 overlap of the top-k cells (bx_topk_overlap) and the mean windowed SSIM of scikit-image
                                 (bx_row_minmax, bx_ssim_rows) of two maps; the model parameter randomization test re-initialises
                                 the layers from the output towards the input with counter-based draws (bx_param_uniform), compares
                                 every stage's map with the trained model's and restores the parameters bit for bit.
* ``fusion_shap``             -- the exact Shapley values of the two modalities (Lundberg & Lee, NeurIPS 2017; not in the reference): the
                                 players are the votes -- log-probabilities -- the two branches hand to the fusion head, alone, by
                                 modality, by class or in any partition; all 2^M coalitions are enumerated against a joint background,
                                 the head evaluated on every (sample, background row, coalition) in one launch that shares the first
                                 layer between coalitions through LDS tables and averages in fp64 (bx_fusion_values); fixed-order fp64
                                 Shapley sums, the modality game and its interaction (bx_shapley_exact, bx_fusion_interaction).
                                 ``fusion_votes`` returns the votes, ``modality_importance`` the mean |value| per player.
* ``mask_explain``            -- optimised perturbation masks (Fong & Vedaldi, ICCV 2017; the basis of TorchRay's extremal perturbations;
                                 not in the reference): per (sample, class) a gh x gw grid, up-sampled bilinearly, is learned by Adam so
                                 that deleting (or preserving only) the smallest smooth region changes the class score; the rows
                                 (bx_maskopt_rows_*) and one step per iteration -- the fold of dF/dX through the blend and the
                                 up-sampling onto the grid in fp64 in a fixed order, the L1 and TV regularisers, Adam, the clamp, the
                                 history and the status (bx_maskopt_init, bx_maskopt_step) -- between the model's passes;
                                 bx_maskopt_masks up-samples the grids for the result.
* ``tcav`` / ``train_cavs``   -- Testing with Concept Activation Vectors (Kim et al., ICML 2018; Captum's concept.TCAV; not in the
                                 reference): whether a concept, given as example inputs, moves a class at a layer.  The activations of
                                 every concept and random example are stacked once; their centred fp64 Gram matrix (bx_tcav_mean,
                                 bx_tcav_gram) serves every linear classifier -- dual ridge by Cholesky or the mean difference, one
                                 workgroup per problem (bx_tcav_fit) -- the CAVs (bx_tcav_vectors), fp64 directional derivatives
                                 against all of them in a fixed order (bx_tcav_sensitivity) and the scores (bx_tcav_score);
                                 ``welch_t_test`` is the host's significance test against the null problems.
* ``tracin`` / ``self_influence`` -- TracIn (Pruthi et al., NeurIPS 2020; Captum's influence.TracInCPFast; not in the reference): which
                                 training examples made the model decide as it does on a test example, and which training labels
                                 the model fights against, from the checkpoints the training loop writes.  Through the four Linear
                                 layers a per-example gradient is an outer product, so the forward passes' activations and the
                                 closed-form factors (bx_tracin_factors) suffice; the pairwise fp64 sums of a block of training rows
                                 against all test rows are one tiled launch (bx_tracin_scores), the diagonal bx_tracin_self, the
                                 top proponents and opponents an exact radix select (bx_tracin_topk).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
import numbers
import re

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ops import _p, _stream


@contextlib.contextmanager
def _eval_frozen(model):
    """eval() mode with parameters detached from autograd (so backward passes skip every weight-gradient
    kernel); both restored on exit."""
    was_training = model.training
    flags = [(p, p.requires_grad) for p in model.parameters()]
    model.eval()
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        with ops.pack_reuse():                            # the weights stand for the whole pass: packed once, on its first forward
            yield
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        model.train(was_training)


def _resolve(model, dotted):
    mod = model
    for part in dotted.split("."):
        mod = getattr(mod, part)
    return mod


def _class_seed(out: torch.Tensor, class_mode: int, rows=None) -> torch.Tensor:
    """[rows, n_classes] one-hot gradient seeds: row r selects class ``class_mode`` (>= 0) or the arg-max class of
    ``out[r % B]`` (-1); one library launch (bx_class_seed)."""
    B, n = out.shape
    rows = B if rows is None else rows
    seed = torch.empty(rows, n, dtype=torch.float32, device=out.device)
    logp = out.detach().float().contiguous()
    L.check(L.load().bx_class_seed(_p(logp), _p(seed), rows, B, n, int(class_mode), _stream()), "bx_class_seed")
    return seed


def _class_form(class_idx):
    """``grad_cam``'s class_idx -> (class mode, stacked): None = -1 (each sample's arg-max), an int c = c, 'all' = -2 (every class; the
    result then carries a class axis).  Any other string is refused."""
    if class_idx is None:
        return -1, False
    if isinstance(class_idx, str):
        if class_idx != "all":
            raise ValueError(class_idx)
        return -2, True
    return int(class_idx), False


def _class_grads(out, leaf, mode, read=None):
    """d out[:, c] / d leaf for the class(es) of ``mode``: one seed launch and one backward pass per class, stacked to [B*nm, ...] with
    map index = sample * nm + class.  ``read(g)`` replaces each returned gradient by the one to keep."""
    seeds = [_class_seed(out, c) for c in (range(out.shape[1]) if mode == -2 else (mode,))]
    grads = []
    for sd in seeds:
        (g,) = torch.autograd.grad(out, leaf, grad_outputs=sd, retain_graph=True)
        grads.append(g if read is None else read(g))
    return torch.stack(grads, dim=1).flatten(0, 1) if len(grads) > 1 else grads[0]


def _class_axis(B, nm, stacked, cam, raw=None, wts=None):
    """(cam, raw, wts), each [B*nm, ...] -> [B, nm, ...] when the result is stacked over the classes; None passes through."""
    return tuple(t.reshape(B, nm, *t.shape[1:]) if stacked and t is not None else t for t in (cam, raw, wts))


def _cam_result(B, nm, stacked, return_parts, cam, raw, wts, A, out):
    """What every ``grad_cam`` path returns: the map, or with return_parts (cam, raw, weights, A, out)."""
    cam, raw, wts = _class_axis(B, nm, stacked, cam, raw, wts)
    return (cam, raw, wts, A, out) if return_parts else cam


class _SpecTarget:
    """Capture of a spectrogram target over the forward passes of a ``with`` body: the output of ``blk`` (conv_k = 0, a forward hook), or
    the pre-ReLU output of its convolution conv_k in 1..3 (the block's own capture mode; ``want_input`` also keeps the block's input,
    which is what autograd can differentiate against).  On exit, however the body ends, every hook is removed and the block is out
    of capture mode."""

    def __init__(self, blk, conv_k, want_input=False):
        self.blk, self.conv_k, self.want_input, self.leaf, self.hooks = blk, conv_k, want_input, None, []

    def __enter__(self):
        if self.conv_k:
            self.blk._preact, self.blk._capture = self.conv_k, {}
            if self.want_input:
                self.hooks.append(self.blk.register_forward_pre_hook(lambda _m, args: setattr(self, "leaf", args[0])))
        else:
            self.hooks.append(self.blk.register_forward_hook(lambda _m, _i, o: setattr(self, "leaf", o)))
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()
        self.blk._preact, self.blk._capture = 0, None

    def act(self):
        """The target's activation, NHWC."""
        return self.blk._capture["act"] if self.conv_k else self.leaf.detach().permute(0, 2, 3, 1).contiguous()

    def grad(self, g):
        """The gradient at the target, NHWC, after the backward pass that returned ``g`` for ``leaf``."""
        return self.blk._capture["grad"] if self.conv_k else g.permute(0, 2, 3, 1).contiguous()


_METHODS = {"gradcam": L.BX_CAM_GRADCAM, "gradcam++": L.BX_CAM_GRADCAM_PP, "layercam": L.BX_CAM_LAYERCAM}


def _method_code(method):
    if method not in _METHODS:
        raise ValueError(f"unknown class-activation method {method!r}; use one of " + ", ".join(f"'{k}'" for k in _METHODS))
    return _METHODS[method]


def _reduce(A_nhwc, G_nhwc, maps_per_act, relu, method=L.BX_CAM_GRADCAM):
    lib = L.load()
    n_maps, h, w, c = G_nhwc.shape
    cam = torch.empty(n_maps, h, w, dtype=torch.float32, device=G_nhwc.device)
    wts = None if method == L.BX_CAM_LAYERCAM else torch.empty(n_maps, c, dtype=torch.float32, device=G_nhwc.device)
    L.check(lib.bx_cam_reduce(_p(A_nhwc), _p(G_nhwc), _p(cam), _p(wts), n_maps, maps_per_act, h * w, c, method, 1 if relu else 0,
                              ops.bx_dtype(A_nhwc.dtype), _stream()), "bx_cam_reduce")
    return cam, wts


def resize_bilinear(maps: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(maps[:,None], size, mode='bilinear', align_corners=False)[:,0] on fp32 [N,h,w]."""
    n, h, w = maps.shape
    H, W = size
    maps = maps.contiguous()
    out = torch.empty(n, H, W, dtype=torch.float32, device=maps.device)
    L.check(L.load().bx_resize_bilinear(_p(maps), _p(out), n, h, w, H, W, _stream()), "bx_resize_bilinear")
    return out


_TARGET = re.compile(r"^(?:spectrogram_model\.)?block([1-5])(?:\.conv([1-3]))?$")
_EEG_TARGETS = {"conv1": L.BX_EEG_CAM_CONV1, "depthwiseConv": L.BX_EEG_CAM_DEPTHWISE, "separableConv": L.BX_EEG_CAM_SEPARABLE}
_EEG_TARGET = re.compile(r"^(?:eeg_model\.)?(" + "|".join(_EEG_TARGETS) + r")$")


def _check_samples(em, f):
    if f.shape[1] != em.dense.in_features:
        raise RuntimeError(f"EEGNet: {f.shape[1]} features but dense expects {em.dense.in_features} (Samples mismatch)")


def _eeg_head(em, f):
    """The EEG branch after block 2 on the features f (EEGNet: dense + LogSoftmax; EEGNetAttentionDeep: its head)."""
    if hasattr(em, "head"):
        return em.head(f)
    _check_samples(em, f)
    return ops.LinearLsmFn.apply(f, em.dense.weight, em.dense.bias)


def _eeg_target_plane(saved, desc, g, B, T, layer):
    """The activation of EEG target ``layer`` cloned out of the byte arena ``saved`` of a forward pass (bx_eeg_saved_layout gives the
    offsets): fp32 [B, F1*D, 1, T] for 'depthwiseConv', [B, F2, 1, T//P1] for 'separableConv'."""
    off_d, off_s = C.c_size_t(0), C.c_size_t(0)
    L.check(L.load().bx_eeg_saved_layout(C.byref(desc), C.byref(off_d), C.byref(off_s)), "bx_eeg_saved_layout")
    off, ch, t = (off_d.value, g.F1 * g.D, T) if layer == "depthwiseConv" else (off_s.value, g.F2, T // g.P1)
    return saved[off:off + B * ch * t * 4].view(torch.float32).reshape(B, ch, 1, t).clone()


def _grad_cam_eeg(model, eeg, spec, layer, class_idx, upsample, relu, return_parts, method=L.BX_CAM_GRADCAM):
    """Grad-CAM (or Grad-CAM++ / Layer-CAM) at an EEGNet block-1/2 convolution (explain.grad_cam).  The EEG branch runs forward once
    without autograd, keeping its saved arena; the rest of the model runs on a detached feature leaf, autograd gives dy_c/dfeat for
    each class seed; then ONE bx_eeg_cam call does the backward to the target and the reduce of the method (and for conv1 the FIR
    over x)."""
    from .models import EEGNet, EEGNetAttentionDeep
    multimodal = hasattr(model, "eeg_model")
    em = model.eeg_model if multimodal else model
    if not isinstance(em, (EEGNet, EEGNetAttentionDeep)):
        raise ValueError(f"EEG Grad-CAM needs an EEGNet / EEGNetAttentionDeep branch, got {type(em).__name__}")
    if multimodal and spec is None:
        raise ValueError("EEG Grad-CAM on a MultimodalModel needs the spectrogram input too")
    mode, stacked = _class_form(class_idx)
    target = _EEG_TARGETS[layer]
    lib = L.load()
    g = em._geom
    B, T = eeg.shape[0], eeg.shape[-1]
    n_cls = model.fc2.out_features if multimodal else (em.dense2.out_features if hasattr(em, "dense2") else em.dense.out_features)
    nm = n_cls if stacked else 1
    probe = L.EegDesc(B, eeg.shape[-2], T, g.F1, g.D, g.F2, g.K1, g.K2, g.P1, g.P2, 0, 1e-5, 0.1, 0.0, 0, L.BX_F32, 0, -1.0)
    if lib.bx_eeg_cam_workspace(C.byref(probe), nm, target, method) == 0:
        raise ValueError(f"EEG Grad-CAM supports the tuned EEGNet family only: F1=8, D=2, F2=16, K2=16, kernLength <= 64, Chans <= 64, "
                         f"T <= 15000, at most 64 classes (got F1={g.F1}, D={g.D}, F2={g.F2}, kernLength={g.K1}, Chans={eeg.shape[-2]}, "
                         f"T={T}, {nm} maps per sample)")
    with _eval_frozen(model):
        with torch.no_grad():
            feat, saved, desc, params, x = ops.eeg_features_keep(em, eeg)
            s_out = model.spectrogram_model(spec) if multimodal else None
        f = feat.detach().requires_grad_(True)
        with torch.enable_grad():
            out = _eeg_head(em, f)
            if multimodal:
                out = ops.FusionHeadFn.apply(out, s_out, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)
        dfeat = _class_grads(out, f, mode).contiguous()
        Ch, T1 = desc.Chans, T // g.P1
        shape1, nw = {L.BX_EEG_CAM_CONV1: ((Ch, T), g.F1), L.BX_EEG_CAM_DEPTHWISE: ((1, T), g.F1 * g.D),
                      L.BX_EEG_CAM_SEPARABLE: ((1, T1), g.F2)}[target]
        dev = feat.device
        cam = torch.empty(B * nm, *shape1, dtype=torch.float32, device=dev)
        raw = torch.empty_like(cam) if (return_parts and relu) else None
        wts = torch.empty(B * nm, nw, dtype=torch.float32, device=dev) if return_parts and method != L.BX_CAM_LAYERCAM else None
        ws = ops.workspace(lib.bx_eeg_cam_workspace(C.byref(desc), nm, target, method), dev)
        L.check(lib.bx_eeg_cam(C.byref(desc), C.byref(params), _p(x), _p(saved), _p(dfeat), nm, target, method, 1 if relu else 0,
                               _p(cam), _p(raw), _p(wts), _p(ws), ws.numel(), _stream()), "bx_eeg_cam")
        if raw is None:
            raw = cam
        A = _eeg_target_plane(saved, desc, g, B, T, layer) if return_parts and target != L.BX_EEG_CAM_CONV1 else None
        if upsample and target == L.BX_EEG_CAM_SEPARABLE:
            cam = resize_bilinear(cam.reshape(B * nm, 1, T1), (1, T))
    return _cam_result(B, nm, stacked, return_parts, cam, raw, wts, A, out.detach())


def _grad_cam_last_stage(model, eeg, spec, class_idx, upsample, relu, return_parts, method=L.BX_CAM_GRADCAM):
    """Default target (the last stage feeds the heads directly): no autograd and no framework arithmetic at all.  The two
    branches run forward, then ONE launch (bx_cam_head) does both heads forward, their backward for every requested class
    and the method's channel reduce; a second launch upsamples the maps."""
    lib = L.load()
    sm = model.spectrogram_model
    mode, stacked = _class_form(class_idx)
    with torch.no_grad():
        em = model.eeg_model
        H, W = spec.shape[-2:]
        # sweep form: the EEG branch's dense + LogSoftmax and the up-sampling ride in the head launch (two launches fewer per batch)
        # (the EEG branch beside the spectrogram branch, as the captured training step runs them, does not pay here: 440 vs 433 us
        # per batch -- the evaluation-mode branch is 55 us of five launches and the fork / join costs about as much as it hides)
        sweep = upsample and not return_parts and W % 4 == 0 and hasattr(model, "_fusable") and model._fusable()
        e = (em.features(eeg) if sweep else em(eeg)).contiguous()        # the branch's log-probabilities; sweep form: its features
        A = sm.features(spec).permute(0, 2, 3, 1).contiguous()
        B, h, w, C = A.shape
        N, Hd = model.fc2.out_features, model.fc1.out_features
        nm = N if stacked else 1
        if sweep:
            _check_samples(em, e)
            lds_floats = 2 * C + 2 * Hd + 5 * N + (256 // (C // 8)) * C + h * w
            if lds_floats * 4 <= 64 * 1024:
                maps = torch.empty(B * nm, H, W, dtype=torch.float32, device=A.device)
                L.check(lib.bx_cam_head_sweep(_p(A), _p(e), _p(em.dense.weight), _p(em.dense.bias), e.shape[1], _p(sm.fc.weight),
                                              _p(sm.fc.bias), _p(model.fc1.weight), _p(model.fc1.bias), _p(model.fc2.weight),
                                              _p(model.fc2.bias), None, _p(maps), B, h, w, C, N, Hd, H, W, mode, method, 1 if relu else 0,
                                              ops.bx_dtype(A.dtype), _stream()), "bx_cam_head_sweep")
                return _class_axis(B, nm, stacked, maps)[0]
            e = ops.LinearLsmFn.apply(e, em.dense.weight, em.dense.bias).contiguous()
        dev = A.device
        out = torch.empty(B, N, dtype=torch.float32, device=dev)
        cam = torch.empty(B * nm, h, w, dtype=torch.float32, device=dev)
        raw = torch.empty_like(cam) if return_parts else None
        wts = torch.empty(B * nm, C, dtype=torch.float32, device=dev) if return_parts and method != L.BX_CAM_LAYERCAM else None
        L.check(lib.bx_cam_head(_p(A), _p(e), _p(sm.fc.weight), _p(sm.fc.bias), _p(model.fc1.weight), _p(model.fc1.bias),
                                _p(model.fc2.weight), _p(model.fc2.bias), _p(out), _p(cam), _p(raw), _p(wts), B, h * w, C, N, Hd, mode,
                                method, 1 if relu else 0, ops.bx_dtype(A.dtype), _stream()), "bx_cam_head")
        if upsample:
            cam = resize_bilinear(cam, spec.shape[-2:])
    return _cam_result(B, nm, stacked, return_parts, cam, raw, wts, A, out)


class GradCamSweep:
    """Grad-CAM at the default target replayed from captured hipGraphs -- for sweeps over many batches (BASELINE configs[3]:
    10 000 samples, all classes).  The launches of `grad_cam` are captured once per batch shape on static input buffers (the
    ragged last batch of a sweep gets its own capture the first time it is seen); a call copies the batch in and replays them,
    so the sweep runs at GPU speed instead of at the host's launch rate.  The returned tensor is that graph's static output
    buffer: clone it if it must outlive the next call with the same shape.  ``method`` is that of `grad_cam` ('gradcam',
    'gradcam++', 'layercam'); a replay runs the eager call's launches, so its maps equal ``grad_cam(..., method=method)``.

    The captured launches hold no weight-packing jobs: a call re-packs first when a parameter changed since the last pack -- as far
    as torch's version counters and this library's own optimizer kernels can tell.  A parameter rewritten through a ``.data`` view
    between two calls is NOT seen: call ``invalidate()`` after such an edit.

        sweep = GradCamSweep(model, eeg_batch, spec_batch, class_idx="all")
        for eeg, spec in loader:
            maps = sweep(eeg, spec)          # [B, 6, H, W]
    """

    def __init__(self, model, eeg, spec, class_idx="all", upsample=True, relu=True, method="gradcam"):
        code = _method_code(method)
        if not (eeg.is_cuda and spec.is_cuda):
            raise RuntimeError("brainxai.GradCamSweep needs CUDA tensors; there is no CPU path")
        self.model, self.args = model, (class_idx, upsample, relu, code)
        self._graphs = {}
        self._capture(eeg, spec)

    def invalidate(self):
        """Force the next call to re-pack the weights (after parameter edits torch cannot see, e.g. through ``.data``)."""
        ops.bump_param_epoch()

    @staticmethod
    def _slot_ready(t):
        return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()

    def _capture(self, eeg, spec):
        model = self.model
        class_idx, upsample, relu, method = self.args
        s_eeg, s_spec = eeg.detach().clone().contiguous(), spec.detach().clone().contiguous()
        # The kernels that read the raw batch take its address from a device slot (ops.INPUT_SLOTS): a replay on the caller's own
        # fp32 tensors costs one 16-byte store instead of two copies (43 MB per batch of 64 at the bench shape, ~20 us).  Inputs in
        # another dtype / layout still go through the static buffers.
        slots = torch.zeros(2, dtype=torch.int64, device=s_eeg.device) if self._slot_ready(s_eeg) and self._slot_ready(s_spec) else None
        if slots is not None:
            L.check(L.load().bx_store_u64x2(slots.data_ptr(), s_eeg.data_ptr(), s_spec.data_ptr(), ops._stream()), "bx_store_u64x2")
            ops.INPUT_SLOTS[s_eeg.data_ptr()] = slots.data_ptr()
            ops.INPUT_SLOTS[s_spec.data_ptr()] = slots.data_ptr() + 8
        was_training = model.training
        model.eval()
        try:
            with ops.pack_reuse():                       # (bumps the parameter epoch: the first warm-up run packs the weights)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):                   # allocate workspaces / pack tables on the capture stream
                        _grad_cam_last_stage(model, s_eeg, s_spec, class_idx, upsample, relu, False, method)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = _grad_cam_last_stage(model, s_eeg, s_spec, class_idx, upsample, relu, False, method)
        finally:
            model.train(was_training)
            used = (False, False)
            if slots is not None:
                # which inputs the captured kernels really read through their slot (fp32 storage converts the spectrogram in another
                # kernel, a non-default EEGNet geometry reads x in several): the others are fed through the static buffers
                used = (ops.INPUT_SLOTS.pop(s_eeg.data_ptr(), None) == "used", ops.INPUT_SLOTS.pop(s_spec.data_ptr(), None) == "used")
                ops._SLOT_ADDR.pop(s_eeg.data_ptr(), None)
                ops._SLOT_ADDR.pop(s_spec.data_ptr(), None)
        plan = getattr(model.spectrogram_model, "_pack_plan", None)
        # the warm-up runs packed the weights eagerly, so the captured launches hold no pack jobs when the plan was fresh: a replay
        # must then make sure it still is (training between two sweeps, load_state_dict, ...)
        entry = (graph, s_eeg, s_spec, out, slots, plan, used)
        self._graphs[(tuple(eeg.shape), tuple(spec.shape))] = entry
        return entry

    def __call__(self, eeg, spec):
        entry = self._graphs.get((tuple(eeg.shape), tuple(spec.shape)))
        if entry is None:
            if eeg.shape[0] != spec.shape[0] or eeg.shape[0] == 0:
                raise RuntimeError(f"GradCamSweep: bad batch {tuple(eeg.shape)} / {tuple(spec.shape)}")
            entry = self._capture(eeg, spec)
        graph, s_eeg, s_spec, out, slots, plan, used = entry
        if plan is not None and not plan.fresh():
            if getattr(self.model.spectrogram_model, "_pack_plan", None) is not plan:
                # the parameters moved to other storage (a new FlatAdamW arena): the graph's operand buffers are orphaned
                self._graphs.clear()
                return self.__call__(eeg, spec)
            plan.run()                                   # repack eagerly; the graph's convolutions read the same operand buffers
        ptrs = []
        for t, st, via_slot in ((eeg, s_eeg, used[0]), (spec, s_spec, used[1])):
            if via_slot and self._slot_ready(t):
                ptrs.append(t.data_ptr())
            else:
                st.copy_(t, non_blocking=True)
                ptrs.append(st.data_ptr())
        if slots is not None:
            L.check(L.load().bx_store_u64x2(slots.data_ptr(), ptrs[0], ptrs[1], ops._stream()), "bx_store_u64x2")
        graph.replay()
        return out


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous shard [lo, hi) of ``n`` samples for ``rank`` of ``world``: sizes differ by at most one, lower ranks take the
    remainder, every sample belongs to exactly one rank (attribution sweeps shard by sample, no collective)."""
    base, rem = divmod(int(n), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sharded_sweep(fn, n_samples, batch_size, fetch, rank=None, world=None, gather=True, group=None):
    """Run an attribution ``fn`` over ``n_samples`` samples sharded contiguously over the ranks of the process group
    (BASELINE configs[3] / configs[4]).  ``fetch(lo, hi)`` returns the inputs (a tuple of tensors) of samples [lo, hi) already on
    this rank's device; ``fn(*inputs)`` returns a tensor whose first axis is the sample axis (e.g. Grad-CAM maps [b, 6, H, W]
    from a GradCamSweep, or integrated-gradients attributions).  Each rank walks its shard in batches of ``batch_size`` (the last
    one ragged).  ``gather=True``: rank 0 returns the [n_samples, ...] result in sample order (one padded ``dist.gather``), the
    other ranks None; ``gather=False``: every rank returns (lo, its shard's result).  Without a process group: one shard."""
    import torch.distributed as dist
    have_pg = dist.is_available() and dist.is_initialized()
    if rank is None:
        rank = dist.get_rank(group) if have_pg else 0
    if world is None:
        world = dist.get_world_size(group) if have_pg else 1
    lo, hi = shard_bounds(n_samples, rank, world)
    if gather and world > 1 and n_samples < world:
        # decided from (n_samples, world), which every rank knows, BEFORE any collective: all ranks raise together instead of the
        # empty ones raising while the others wait in dist.gather
        raise RuntimeError("sharded_sweep(gather=True) needs at least one sample per rank; use gather=False for tiny sweeps")
    parts = []
    for b0 in range(lo, hi, batch_size):
        b1 = min(hi, b0 + batch_size)
        parts.append(fn(*fetch(b0, b1)).clone())         # clone: fn may return a static graph buffer
    mine = torch.cat(parts) if parts else None
    if not gather:
        return lo, mine
    if world == 1:
        return mine
    # every rank needs the trailing shape to build its padded block: take it from a rank that has samples
    cap = shard_bounds(n_samples, 0, world)[1]           # rank 0 holds the largest shard
    pad = torch.zeros(cap, *mine.shape[1:], dtype=mine.dtype, device=mine.device)
    pad[:mine.shape[0]] = mine
    blocks = [torch.empty_like(pad) for _ in range(world)] if rank == 0 else None
    dist.gather(pad, blocks, dst=0, group=group)
    if rank != 0:
        return None
    sizes = [shard_bounds(n_samples, r, world) for r in range(world)]
    return torch.cat([blk[:b - a] for blk, (a, b) in zip(blocks, sizes)])


def grad_cam(model, eeg, spec, target_layer="spectrogram_model.block5", class_idx=None, upsample=True, relu=True,
             return_parts=False, method="gradcam"):
    """Grad-CAM heat-maps of ``model(eeg, spec)``.

    score y_c = the model's output log-probability of class c;  w[b,k] = mean_hw dy_c/dA[b,k];
    cam[b] = ReLU(sum_k w[b,k] A[b,k]); optionally bilinear-upsampled to the spectrogram's H x W.

    method:       'gradcam' (above), 'gradcam++' or 'layercam'.  With A[k,s] the target's activation (channel k, position s
                  over the axes Grad-CAM averages), G = dy_c/dA and eps = 1e-6:
                    'gradcam++': S_k = sum_s A[k,s];  alpha[k,s] = G^2 / (2 G^2 + S_k G^3 + eps), 0 where G == 0;
                                 w_k = sum_s max(G[k,s], 0) alpha[k,s] (a sum, not a mean);  raw[s] = sum_k w_k A[k,s]
                                 (Chattopadhyay et al., WACV 2018, eq. 19)
                    'layercam':  raw[s] = sum_k max(G[k,s], 0) A[k,s]   (Jiang et al., TIP 2021)
                  cam = ReLU(raw) if relu, then the same optional up-sampling; no normalisation.  Every target, class_idx form
                  and option below works with every method.

    target_layer: 'spectrogram_model.blockN' (stage output) or 'spectrogram_model.blockN.convK'
                  (that convolution's pre-ReLU output, i.e. what a hook on the reference's nn.Conv2d sees);
                  or an EEG-branch convolution (its output, before its BatchNorm; 'eeg_model.' is optional, and a
                  stand-alone EEGNet / EEGNetAttentionDeep is called as grad_cam(net, eeg, None, 'conv1')):
                    'eeg_model.conv1'          -> electrode x time maps [B, Chans, T]
                    'eeg_model.depthwiseConv'  -> [B, 1, T]
                    'eeg_model.separableConv'  -> [B, 1, T//4]; upsample=True resizes it to [B, 1, T] (bilinear)
                  The conv1 and depthwiseConv maps are at input resolution already: `upsample` leaves them as they are.
                  EEG targets need the tuned EEGNet family (F1=8, D=2, F2=16, kernLength <= 64, Chans <= 64,
                  T <= 15000); other geometries raise ValueError.
    class_idx:    None -> each sample's arg-max class; int -> that class; 'all' -> every class, output
                  gains a class axis [B, n_classes, H, W].
    return_parts: (cam, raw, weights, A, out).  For EEG targets weights is [B(, n_classes), channels of the target]
                  and A the target's activation [B, channels, 1, time] -- None for conv1, whose [B, 8, Chans, T]
                  output is never formed (in evaluation mode its map is one combined 1-D filter over the input).
                  weights holds w_k of the method: the Grad-CAM++ w_k for 'gradcam++', and None for 'layercam', whose
                  weights vary with the position.
    The model's training mode and every parameter's requires_grad are restored on return.
    """
    code = _method_code(method)
    me = _EEG_TARGET.match(target_layer)
    if me:
        return _grad_cam_eeg(model, eeg, spec, me.group(1), class_idx, upsample, relu, return_parts, code)
    if target_layer.startswith("eeg_model."):
        raise ValueError(f"unsupported EEG Grad-CAM target {target_layer!r}; use one of "
                         + ", ".join(f"'eeg_model.{k}'" for k in _EEG_TARGETS))
    m = _TARGET.match(target_layer)
    if not m:
        raise ValueError(f"unsupported Grad-CAM target {target_layer!r}; use 'spectrogram_model.blockN[.convK]' or one of "
                         + ", ".join(f"'eeg_model.{k}'" for k in _EEG_TARGETS))
    spec_model = model.spectrogram_model if hasattr(model, "spectrogram_model") else model
    blk = getattr(spec_model, f"block{m.group(1)}")
    conv_k = int(m.group(2)) if m.group(2) else 0
    if conv_k == 0 and m.group(1) == "5" and hasattr(model, "eeg_model") and hasattr(model, "fc1"):
        was_training = model.training
        model.eval()
        try:
            return _grad_cam_last_stage(model, eeg, spec, class_idx, upsample, relu, return_parts, code)
        finally:
            model.train(was_training)
    mode, stacked = _class_form(class_idx)
    with _eval_frozen(model):
        spec_in = spec.detach().clone().requires_grad_(True)
        with _SpecTarget(blk, conv_k, want_input=True) as tgt:
            out = model(eeg, spec_in) if hasattr(model, "spectrogram_model") else model(spec_in)
            G = _class_grads(out, tgt.leaf, mode, tgt.grad)
            A = tgt.act()
        B, nm = out.shape[0], out.shape[1] if stacked else 1
        cam, wts = _reduce(A, G, nm, relu, code)
        raw = _reduce(A, G, nm, False, code)[0] if (return_parts and relu) else cam
        if upsample:
            cam = resize_bilinear(cam, spec.shape[-2:])
    return _cam_result(B, nm, stacked, return_parts, cam, raw, wts, A, out.detach())


def _abs(t: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(t)
    L.check(L.load().bx_abs(_p(t), _p(out), t.numel(), _stream()), "bx_abs")
    return out


def saliency(model, eeg, spec, reference_quirk=False):
    """|d max-logprob / d input| (reference XAI_Multimodality.py:3109-3129): returns
    (eeg_sal [B,Chans,T], spec_sal [B,H,W]); the spectrogram map is the max over channels.
    ``reference_quirk=True`` doubles the spectrogram map as the reference's second backward() does."""
    with _eval_frozen(model):
        e = eeg.detach().clone().float().requires_grad_(True)
        s = spec.detach().clone().float().requires_grad_(True)
        out = model(e, s)
        seed = _class_seed(out, -1)
        ge, gs = torch.autograd.grad(out, (e, s), grad_outputs=seed)
    B, Cc, H, W = gs.shape
    g_nhwc = ops.to_nhwc(gs, torch.float32)
    smap = torch.empty(B, H, W, dtype=torch.float32, device=gs.device)
    L.check(L.load().bx_saliency_reduce(_p(g_nhwc), _p(smap), B, H * W, Cc, g_nhwc.shape[3], 2.0 if reference_quirk else 1.0,
                                        L.BX_F32, _stream()), "bx_saliency_reduce")
    return _abs(ge.contiguous())[:, 0], smap


def generate_saliency_maps(model, dataloader, plot_eeg=None, plot_spectrogram=None, device=None):
    """Reference signature (XAI_Multimodality.py:3101).  Iterates ``((eeg, spec), label)`` batches, computes the
    reference's maps (batch element 0 of each batch, spectrogram map with its 2x accumulation quirk) and hands
    them to the optional plot callbacks; also returns them as a list of (eeg_map, spec_map) numpy pairs."""
    device = device or next(model.parameters()).device
    results = []
    for (eeg_data, spectrogram_data), _label in dataloader:
        e, s = eeg_data.to(device)[:1], spectrogram_data.to(device)[:1]
        es, ss = saliency(model, e, s, reference_quirk=True)
        pair = (es[0].cpu().numpy(), ss[0].cpu().numpy())
        results.append(pair)
        if plot_eeg is not None:
            plot_eeg(pair[0])
        if plot_spectrogram is not None:
            plot_spectrogram(pair[1])
    return results


def ig_nodes(n_steps=50):
    x, w = np.polynomial.legendre.leggauss(n_steps)
    return 0.5 * (1.0 + x), 0.5 * w


def _axpby(x, y, alpha, beta):
    L.check(L.load().bx_axpby(_p(x), _p(y), x.numel(), float(alpha), float(beta), _stream()), "bx_axpby")


def integrated_gradients(model, inputs, baselines=None, target=None, n_steps=50, max_batch=1024):
    """(x - x') * sum_k w_k grad F_target(x' + a_k (x - x')) with Gauss-Legendre nodes (Captum's default rule).
    inputs = (eeg [B,1,Ch,T], spec [B,C,H,W]); the k-loop is batched: up to ``max_batch`` interpolants per pass (sized for
    288 GB of HBM: a pass keeps ~18 MB of activations per interpolant at the benchmark shapes in bf16 storage, 35 MB in fp32;
    measured at 50 x B=64: 256 -> 1380, 512 -> 1415, 1024 -> 1472 samples/s -- the late stages stop being latency-bound)."""
    eeg, spec = (t.detach().float().contiguous() for t in inputs)
    be, bs = baselines if baselines is not None else (torch.zeros_like(eeg), torch.zeros_like(spec))
    be, bs = be.float().contiguous(), bs.float().contiguous()
    B = eeg.shape[0]
    alphas, steps = ig_nodes(n_steps)
    acc_e, acc_s = torch.zeros_like(eeg), torch.zeros_like(spec)
    alphas_dev = torch.tensor([float(a) for a in alphas], dtype=torch.float32, device=eeg.device)
    steps_dev = torch.tensor([float(w) for w in steps], dtype=torch.float32, device=eeg.device)
    per_pass = max(1, max_batch // B)
    # the kernels address an activation tensor with 32-bit byte offsets: keep the largest one of a pass (stage 1: H x W x 16
    # channels) under 2 GiB
    sm_ = getattr(model, "spectrogram_model", None)
    esize = 2 if getattr(sm_, "compute_dtype", torch.float32) == torch.bfloat16 else 4
    cap = ((1 << 31) - 1) // max(1, spec.shape[2] * spec.shape[3] * 16 * esize)
    per_pass = max(1, min(per_pass, cap // B))
    with _eval_frozen(model):
        with torch.no_grad():
            base_out = model(eeg, spec)                     # arg-max class of the un-interpolated input (Captum: target of the input)
        tmode = -1 if target is None else int(target)
        for k0 in range(0, n_steps, per_pass):
            ks = range(k0, min(n_steps, k0 + per_pass))
            xe = torch.empty(len(ks), *eeg.shape, dtype=torch.float32, device=eeg.device)
            xs = torch.empty(len(ks), *spec.shape, dtype=torch.float32, device=spec.device)
            a_dev, w_dev = alphas_dev[k0:k0 + len(ks)], steps_dev[k0:k0 + len(ks)]
            lib_ = L.load()
            L.check(lib_.bx_ig_interpolate(_p(eeg), _p(be), _p(a_dev), _p(xe), eeg.numel(), len(ks), _stream()), "bx_ig_interpolate")
            L.check(lib_.bx_ig_interpolate(_p(spec), _p(bs), _p(a_dev), _p(xs), spec.numel(), len(ks), _stream()), "bx_ig_interpolate")
            xe = xe.flatten(0, 1).requires_grad_(True)
            xs = xs.flatten(0, 1).requires_grad_(True)
            out = model(xe, xs)
            seed = _class_seed(base_out, tmode, rows=len(ks) * B)      # row k*B + b -> class of sample b
            ge, gs = torch.autograd.grad(out, (xe, xs), grad_outputs=seed)
            ge, gs = ge.contiguous(), gs.contiguous()
            L.check(lib_.bx_ig_accumulate(_p(ge), _p(w_dev), _p(acc_e), acc_e.numel(), len(ks), _stream()), "bx_ig_accumulate")
            L.check(lib_.bx_ig_accumulate(_p(gs), _p(w_dev), _p(acc_s), acc_s.numel(), len(ks), _stream()), "bx_ig_accumulate")
    de, ds = eeg.clone(), spec.clone()
    _axpby(be, de, -1.0, 1.0)
    _axpby(bs, ds, -1.0, 1.0)
    lib = L.load()
    L.check(lib.bx_mul(_p(acc_e), _p(de), _p(acc_e), acc_e.numel(), _stream()), "bx_mul")
    L.check(lib.bx_mul(_p(acc_s), _p(ds), _p(acc_s), acc_s.numel(), _stream()), "bx_mul")
    return acc_e, acc_s


def expected_gradients(model, x, background, nsamples=200, seed=0, max_batch=256):
    """SHAP GradientExplainer's estimator for a single-input model (the reference explains ``multimodal_model.eeg_model``,
    XAI_Multimodality.py:2283-2290):  phi_c(x) = E_{b, a}[(x - b) * d f_c/dx (b + a (x - b))], b drawn from ``background``,
    a ~ U(0,1); draws from numpy's default_rng(seed) in sample-major order.  Returns [B, n_classes, *x.shape[1:]].
    Interpolants are built with bx_axpby, gradients come from the HIP backward, products/means from bx_mul / bx_axpby."""
    x = x.detach().float().contiguous()
    background = background.detach().float().contiguous()
    rng = np.random.default_rng(seed)
    B = x.shape[0]
    lib = L.load()
    with _eval_frozen(model):
        with torch.no_grad():
            n_cls = model(x[:1]).shape[1]
        out = torch.zeros(B, n_cls, *x.shape[1:], dtype=torch.float32, device=x.device)
        for i in range(B):
            idx = rng.integers(0, background.shape[0], size=nsamples)
            alpha = rng.random(nsamples).astype(np.float32)
            for k0 in range(0, nsamples, max_batch):
                ks = range(k0, min(nsamples, k0 + max_batch))
                base = background[torch.as_tensor(idx[k0:k0 + len(ks)], device=x.device)].contiguous()
                diff = x[i:i + 1].expand_as(base).contiguous()
                _axpby(base, diff, -1.0, 1.0)                               # diff = x - b
                xi = base.clone()
                for j, k in enumerate(ks):
                    _axpby(diff[j], xi[j], float(alpha[k]), 1.0)            # b + a (x - b)
                xi.requires_grad_(True)
                y = model(xi)
                for c in range(n_cls):
                    seed_c = _class_seed(y, c)
                    (g,) = torch.autograd.grad(y, xi, grad_outputs=seed_c, retain_graph=True)
                    g = g.contiguous()
                    L.check(lib.bx_mul(_p(g), _p(diff), _p(g), g.numel(), _stream()), "bx_mul")
                    for j in range(len(ks)):
                        _axpby(g[j], out[i, c], 1.0 / nsamples, 1.0)
    return out


def predict_fn(images, model, device=None, max_batch=256):
    """LIME's batched-inference callback (reference XAI_Multimodality.py:1567-1574, :2710-2717; called by
    ``lime_image.LimeImageExplainer.explain_instance`` with the perturbed copies of one spectrogram image).

    images: sequence / array of H x W x C images (LIME passes float arrays holding 0..255 values; the reference casts them with
    ``astype(np.uint8)`` and applies torchvision's ToTensor = x / 255, channels first).  model: a single-input spectrogram model
    (``Spectrogram_Model`` or ``multimodal.forward_spectrogram``).  Returns ``softmax(model(batch))`` as a numpy array [N, classes]
    exactly like the reference (the model already ends in LogSoftmax, so these are its class probabilities).
    The uint8 -> channels-last conversion, the forward pass and the softmax all run on the GPU, ``max_batch`` images per pass."""
    imgs = np.ascontiguousarray(np.stack([np.asarray(im) for im in images]).astype(np.uint8))
    if imgs.ndim != 4:
        raise ValueError(f"predict_fn expects images [N, H, W, C], got {imgs.shape}")
    device = torch.device(device) if device is not None else next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("brainxai.predict_fn: the model must live on the GPU; there is no CPU path")
    fwd = model.forward_spectrogram if hasattr(model, "forward_spectrogram") else model
    net = model.spectrogram_model if hasattr(model, "spectrogram_model") else model
    dt = getattr(net, "compute_dtype", torch.float32)
    was_training = model.training
    model.eval()
    lib = L.load()
    N, H, W, Cc = imgs.shape
    out = []
    try:
        with torch.no_grad():
            for i0 in range(0, N, max_batch):
                chunk = torch.from_numpy(imgs[i0:i0 + max_batch]).to(device)
                n = chunk.shape[0]
                x = torch.empty(n, H, W, ops.pad8(Cc), dtype=dt, device=device)
                L.check(lib.bx_u8_to_nhwc(_p(chunk), _p(x), n, H, W, Cc, ops.pad8(Cc), 1.0 / 255.0, ops.bx_dtype(dt), _stream()), "bx_u8_to_nhwc")
                logp = fwd(x.permute(0, 3, 1, 2)).float().contiguous()       # a logical-NCHW view of the internal layout: no further copy
                probs = torch.empty_like(logp)
                L.check(lib.bx_softmax_rows(_p(logp), _p(probs), n, logp.shape[1], _stream()), "bx_softmax_rows")
                out.append(probs.cpu())
    finally:
        model.train(was_training)
    return torch.cat(out).numpy()


# ------------------------------------------------------------------------------------------------
# LIME for images (lime 0.2.0.1, LimeImageExplainer.explain_instance; reference XAI_Multimodality.py:1658-1670)
_LIME_MAX_S, _LIME_MAX_C, _LIME_MAX_K = 1024, 4, 32
_LIME_SELECTIONS = ("auto", "none", "highest_weights")


def grid_segments(H, W, rows, cols):
    """Label map [H, W] (int32) of rows x cols time-by-frequency tiles, label = row * cols + col; tile heights (widths) differ by at
    most one pixel when H (W) is not divisible.  The built-in segmentation for spectrograms; ``lime_image`` takes any label map."""
    H, W, rows, cols = int(H), int(W), int(rows), int(cols)
    if not (1 <= rows <= H and 1 <= cols <= W):
        raise ValueError(f"grid_segments: need 1 <= rows <= H and 1 <= cols <= W, got H={H} W={W} rows={rows} cols={cols}")
    r = (np.arange(H, dtype=np.int64) * rows) // H
    c = (np.arange(W, dtype=np.int64) * cols) // W
    return (r[:, None] * cols + c[None, :]).astype(np.int32)


class LimeExplanation:
    """What ``lime_image`` returns for one image, with the attribute names of lime's ImageExplanation: ``image``, ``segments``,
    ``top_labels``, ``local_exp`` {label: [(feature, weight), ...] by descending |weight|}, ``intercept``, ``score``, ``local_pred``
    {label: float}; plus ``weights`` [N] (kernel weights), ``masks`` [N, S] uint8, ``probs`` (device tensor [N, K])."""

    def __init__(self, image, segments):
        self.image, self.segments = image, segments
        self.top_labels = None
        self.local_exp, self.intercept, self.score, self.local_pred = {}, {}, {}, {}
        self.weights = self.masks = self.probs = None
        self._seg_dev, self._coef_dev, self._used_dev = None, {}, {}

    def heatmap(self, label):
        """Device tensor [H, W] fp32: the surrogate's weight of each pixel's segment (0 for features the fit did not use)."""
        if label not in self._coef_dev:
            raise KeyError("Label not in explanation")
        coef, used, seg = self._coef_dev[label], self._used_dev[label], self._seg_dev
        H, W = seg.shape
        out = torch.empty(H, W, dtype=torch.float32, device=seg.device)
        with torch.cuda.device(seg.device):
            L.check(L.load().bx_lime_weight_map(_p(coef), _p(used), _p(seg), _p(out), 1, 1, H, W, self.masks.shape[1], coef.numel(), _stream()),
                    "bx_lime_weight_map")
        return out

    def get_image_and_mask(self, label, positive_only=True, negative_only=False, hide_rest=False, num_features=5, min_weight=0.0):
        """lime's ImageExplanation.get_image_and_mask (host numpy: presentation).  Returns (image, mask)."""
        if label not in self.local_exp:
            raise KeyError("Label not in explanation")
        if positive_only and negative_only:
            raise ValueError("Positive_only and negative_only cannot be true at the same time.")
        segments, image, exp = self.segments, self.image, self.local_exp[label]
        mask = np.zeros(segments.shape, segments.dtype)
        temp = np.zeros(image.shape) if hide_rest else image.copy()
        if positive_only or negative_only:
            if positive_only:
                fs = [f for f, w in exp if w > 0 and w > min_weight][:num_features]
            else:
                fs = [f for f, w in exp if w < 0 and abs(w) > min_weight][:num_features]
            for f in fs:
                temp[segments == f] = image[segments == f].copy()
                mask[segments == f] = 1
            return temp, mask
        for f, w in exp[:num_features]:
            if abs(w) < min_weight:
                continue
            c = 0 if w < 0 else 1
            mask[segments == f] = -1 if w < 0 else 1
            temp[segments == f] = image[segments == f].copy()
            temp[segments == f, c] = np.max(image)
        return temp, mask


def _lime_colours_host(img, seg, S, hide_color):
    """The fudged colour table u8 [B,S,C] where the package's arithmetic is float (a float image: segment means over the float
    values, truncated; hide_color: the given colour), or None for a uint8 image with hide_color=None (bx_lime_segment_mean)."""
    B, Cc = img.shape[0], img.shape[3]
    if hide_color is not None:
        return np.broadcast_to(np.broadcast_to(np.asarray(hide_color, dtype=np.float64), (Cc,)).astype(np.uint8), (B, S, Cc))
    if img.dtype == np.uint8:
        return None
    out = np.empty((B, S, Cc), dtype=np.uint8)
    for b in range(B):
        for s in range(S):
            out[b, s] = np.array([np.mean(img[b][seg[b] == s][:, c]) for c in range(Cc)]).astype(np.uint8)
    return out


def _lime_fit(Z, P, labels, used, alpha, kernel_width):
    """bx_lime_fit on device tensors: Z u8 [B,N,S], P f32 [B,N,K], labels i32 [B,nl], used i32 [B,S'] or None."""
    lib = L.load()
    B, N, S = Z.shape
    K, nl = P.shape[2], labels.shape[1]
    Sp = S if used is None else used.shape[1]
    dev = Z.device
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    coef, icpt, score, pred, wts = f64(B, nl, Sp), f64(B, nl), f64(B, nl), f64(B, nl), f64(B, N)
    nbytes = lib.bx_lime_fit_workspace(B, N, S, Sp, K, nl)
    if nbytes == 0:
        L.check(-1, "bx_lime_fit_workspace")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    L.check(lib.bx_lime_fit(_p(Z), _p(P), _p(labels), _p(used), B, N, S, Sp, K, nl, float(alpha), float(kernel_width), _p(ws), nbytes,
                            _p(coef), _p(icpt), _p(score), _p(pred), _p(wts), _stream()), "bx_lime_fit")
    return coef, icpt, score, pred, wts


def lime_image(model, image, segments, *, labels=None, top_labels=5, hide_color=None, num_features=100000, num_samples=1000,
               feature_selection="auto", kernel_width=0.25, alpha=1.0, seed=0, masks=None, max_batch=256, device=None):
    """LIME for images as lime 0.2.0.1's ``LimeImageExplainer.explain_instance`` defines it (the reference's call:
    XAI_Multimodality.py:1658-1670), with the perturbed batch, the forward passes and the weighted ridge surrogate on the GPU.

    image: numpy array or tensor [H,W,C] (C <= 4), or a batch [B,H,W,C] with ``segments`` [B,H,W] (a list of explanations comes back;
    the images share N and S and draw their masks from one ``RandomState(seed)`` stream in image order).  uint8 images run wholly on
    the device.  Float arrays holding 0..255 (what the package hands its callback) are accepted: kept pixels are truncated as
    ``predict_fn`` does, and their fudged colours -- S x C segment means over the float values, then truncated, as the package
    computes them -- are taken on the HOST with numpy and uploaded as the colour table.
    segments: integer label map with labels exactly 0..S-1 (S <= 1024); ``grid_segments`` builds tiles, skimage output passes as is.
    model: ``Spectrogram_Model`` or a ``MultimodalModel`` (through ``forward_spectrogram``), on the GPU; it runs in eval mode and gets
    its training flag back; nothing needs a gradient.
    masks: optional Z [N,S] / [B,N,S] of 0/1 replacing the draw (row 0 is set to ones; ``seed`` is then unused).
    labels: classes to explain; None = the ``top_labels`` most probable classes of the unperturbed image.
    hide_color: None = a hidden segment shows its own per-channel mean; otherwise that colour (a number or one per channel).
    feature_selection: 'none', 'highest_weights' or 'auto' (= 'highest_weights' for num_features > 6, which uses every feature when
    num_features >= S).  Semantics per step: DESIGN.md section 1, row G.  Returns a ``LimeExplanation`` (a list for a batch)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    if feature_selection not in _LIME_SELECTIONS:
        raise ValueError(f"lime_image: feature_selection {feature_selection!r} is not supported; use one of "
                         + ", ".join(f"'{s}'" for s in _LIME_SELECTIONS) + " ('forward_selection' and 'lasso_path' are not built)")
    num_features, N = int(num_features), int(num_samples)
    if feature_selection == "auto":
        if num_features <= 6:
            raise ValueError("lime_image: feature_selection='auto' with num_features <= 6 means 'forward_selection', which is not "
                             "supported; use 'none' or 'highest_weights'")
        feature_selection = "highest_weights"
    if num_features < 1:
        raise ValueError(f"lime_image: num_features = {num_features} < 1")
    if N < 2:
        raise ValueError(f"lime_image: num_samples = {N} < 2")
    if int(max_batch) < 1:
        raise ValueError(f"lime_image: max_batch = {max_batch} < 1")
    if not (float(kernel_width) > 0 and float(alpha) > 0):
        raise ValueError("lime_image: kernel_width and alpha must be positive")
    img = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    seg = segments.detach().cpu().numpy() if isinstance(segments, torch.Tensor) else np.asarray(segments)
    single = img.ndim == 3
    if single:
        img, seg = img[None], seg[None] if seg.ndim == 2 else seg
    if img.ndim != 4 or seg.ndim != 3 or seg.shape != img.shape[:3]:
        raise ValueError(f"lime_image: image {tuple(np.shape(image))} and segments {tuple(np.shape(segments))} do not match "
                         "([H,W,C] with [H,W], or [B,H,W,C] with [B,H,W])")
    B, H, W, Cc = img.shape
    if not 1 <= Cc <= _LIME_MAX_C:
        raise ValueError(f"lime_image: {Cc} channels, supported 1..{_LIME_MAX_C}")
    if not np.issubdtype(seg.dtype, np.integer):
        raise ValueError(f"lime_image: segments must be an integer label map, got {seg.dtype}")
    if seg.min() < 0:
        raise ValueError("lime_image: negative label in segments")
    S = int(seg.max()) + 1
    if S > _LIME_MAX_S:
        raise ValueError(f"lime_image: {S} segments, supported 1..{_LIME_MAX_S}")
    for b in range(B):
        if np.unique(seg[b]).size != S:
            raise ValueError(f"lime_image: segments{'' if single else f'[{b}]'} must use every label 0..{S - 1} (features are indexed by label)")
    fwd = model.forward_spectrogram if hasattr(model, "forward_spectrogram") else model
    net = model.spectrogram_model if hasattr(model, "spectrogram_model") else model
    K = int(net.fc.out_features)
    if K > _LIME_MAX_K:
        raise ValueError(f"lime_image: {K} classes, supported up to {_LIME_MAX_K}")
    if labels is not None:
        labels = [int(k) for k in labels]
        if not labels or len(labels) > K or any(not 0 <= k < K for k in labels):
            raise ValueError(f"lime_image: labels {labels} outside [0, {K})")
    elif not 1 <= int(top_labels):
        raise ValueError(f"lime_image: top_labels = {top_labels} < 1")
    if masks is not None:
        Zh = np.asarray(masks.detach().cpu().numpy() if isinstance(masks, torch.Tensor) else masks)
        if Zh.ndim == 2:
            Zh = Zh[None]
        if Zh.shape != (B, N, S) or not np.isin(Zh, (0, 1)).all():
            raise ValueError(f"lime_image: masks must be 0/1 of shape [{'' if single else 'B, '}num_samples, S] = {(B, N, S)}, got {Zh.shape}")
        Zh = Zh.astype(np.uint8)
    else:
        rs = np.random.RandomState(seed)
        Zh = np.stack([rs.randint(0, 2, N * S).reshape(N, S) for _ in range(B)]).astype(np.uint8)
    Zh[:, 0, :] = 1
    device = torch.device(device) if device is not None else next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("brainxai.lime_image: the model must live on the GPU; there is no CPU path")
    colours_h = _lime_colours_host(img, seg, S, hide_color)
    img_u8 = np.ascontiguousarray(img.astype(np.uint8))

    lib = L.load()
    dt = getattr(net, "compute_dtype", torch.float32)
    img_d = torch.from_numpy(img_u8).to(device)
    seg_d = torch.from_numpy(np.ascontiguousarray(seg.astype(np.int32))).to(device)
    Z_d = torch.from_numpy(Zh).to(device)
    P = torch.empty(B, N, K, dtype=torch.float32, device=device)
    was_training = model.training
    model.eval()
    try:
        with torch.cuda.device(device), torch.no_grad():
            if colours_h is None:
                col_d = torch.empty(B, S, Cc, dtype=torch.uint8, device=device)
                L.check(lib.bx_lime_segment_mean(_p(img_d), _p(seg_d), _p(col_d), B, H, W, Cc, S, _stream()), "bx_lime_segment_mean")
            else:
                col_d = torch.from_numpy(np.ascontiguousarray(colours_h)).to(device)
            for b in range(B):                                     # the chunks of one image are the chunks predict_fn would run
                for n0 in range(0, N, int(max_batch)):
                    n = min(int(max_batch), N - n0)
                    x = torch.empty(n, H, W, ops.pad8(Cc), dtype=dt, device=device)
                    L.check(lib.bx_lime_perturb(_p(img_d[b]), _p(seg_d[b]), _p(col_d[b]), _p(Z_d[b]), _p(x), 1, H, W, Cc, ops.pad8(Cc), S, N, n0, n,
                                                ops.bx_dtype(dt), _stream()), "bx_lime_perturb")
                    logp = fwd(x.permute(0, 3, 1, 2)).float().contiguous()
                    L.check(lib.bx_softmax_rows(_p(logp), _p(P[b, n0:n0 + n]), n, K, _stream()), "bx_softmax_rows")
            # ---- labels: the K probabilities of each unperturbed image are all that is read back before the fit ----
            if labels is None:
                p0 = P[:, 0, :].cpu().numpy()
                t = min(int(top_labels), K)
                lab_h = np.stack([np.argsort(p0[b])[-t:][::-1] for b in range(B)]).astype(np.int32)
            else:
                lab_h = np.tile(np.asarray(labels, dtype=np.int32), (B, 1))
            nl = lab_h.shape[1]
            lab_d = torch.from_numpy(np.ascontiguousarray(lab_h)).to(device)
            if feature_selection == "none" or num_features >= S:
                coef, icpt, score, pred, wts = _lime_fit(Z_d, P, lab_d, None, alpha, kernel_width)
                fits = [(coef[:, l], None, icpt[:, l], score[:, l], pred[:, l]) for l in range(nl)]
            else:                                                  # 'highest_weights': first fit at alpha = 0.01 picks the features per label
                coef0 = _lime_fit(Z_d, P, lab_d, None, 0.01, kernel_width)[0].cpu().numpy()
                fits = []
                for l in range(nl):
                    used_h = np.stack([np.argsort(-np.abs(coef0[b, l] * Zh[b, 0]), kind="stable")[:num_features] for b in range(B)])
                    used_d = torch.from_numpy(np.ascontiguousarray(used_h.astype(np.int32))).to(device)
                    coef, icpt, score, pred, wts = _lime_fit(Z_d, P, lab_d[:, l:l + 1].contiguous(), used_d, alpha, kernel_width)
                    fits.append((coef[:, 0], used_d, icpt[:, 0], score[:, 0], pred[:, 0]))
    finally:
        model.train(was_training)
    wts_h = wts.cpu().numpy()
    host = [(c.cpu().numpy(), None if u is None else u.cpu().numpy(), i.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()) for c, u, i, s, p in fits]
    out = []
    for b in range(B):
        e = LimeExplanation(img[b], seg[b])
        e.top_labels = None if labels is not None else [int(k) for k in lab_h[b]]
        e.weights, e.masks, e.probs, e._seg_dev = wts_h[b], Zh[b], P[b], seg_d[b]
        for l in range(nl):
            k = int(lab_h[b, l])
            c, u, i, s, p = host[l]
            feats = np.arange(S) if u is None else u[b]
            e.local_exp[k] = sorted(zip((int(f) for f in feats), (float(v) for v in c[b])), key=lambda fv: abs(fv[1]), reverse=True)
            e.intercept[k], e.score[k], e.local_pred[k] = float(i[b]), float(s[b]), float(p[b])
            e._coef_dev[k] = fits[l][0][b].contiguous()
            e._used_dev[k] = None if fits[l][1] is None else fits[l][1][b].contiguous()
        out.append(e)
    return out[0] if single else out


# ------------------------------------------------------------------------------------------------
# Deletion / insertion curves (the causal metric of RISE, Petsiuk et al., BMVC 2018): how faithful is an attribution map?
_FAITH_MAX_N, _FAITH_MAX_C = (1 << 20) - 1, 4
_FAITH_MODES, _FAITH_SCORES, _FAITH_INPUTS = ("both", "deletion", "insertion"), ("prob", "logprob"), ("spec", "eeg")

FaithfulnessCurves = collections.namedtuple("FaithfulnessCurves", "deletion insertion deletion_auc insertion_auc classes fractions ranks")
FaithfulnessCurves.__doc__ = """What ``deletion_insertion`` returns: ``deletion`` / ``insertion`` fp32 [B, steps+1] and ``deletion_auc`` /
``insertion_auc`` fp64 [B] on the device (None for the mode that was not asked for), ``classes`` int64 [B] (device), ``fractions``
fp64 [steps+1] = k_i / N (host) and ``ranks`` int32 [B, N] (device)."""


def attribution_ranks(attribution):
    """int32 [B, N] on the device: the position of every cell of ``attribution`` [B, ...] (N = the cells of one sample, flattened) in a
    stable descending sort of its sample, ties by ascending flat index, NaN counted as -inf and -0.0 equal to +0.0 --
    ``np.argsort(-key, kind="stable")`` inverted.  Exact; one launch chain (bx_rank_desc), no host round trip."""
    if not isinstance(attribution, torch.Tensor) or attribution.dim() < 2:
        raise ValueError("attribution_ranks: attribution must be a tensor [B, ...] with at least two axes")
    B = int(attribution.shape[0])
    N = attribution.numel() // B if B else 0
    if B < 1 or not 1 <= N <= _FAITH_MAX_N:
        raise ValueError(f"attribution_ranks: {N} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    if not attribution.is_cuda:
        raise RuntimeError("brainxai.attribution_ranks: the attribution must live on the GPU; there is no CPU path")
    lib = L.load()
    a = attribution.detach().reshape(B, N).to(torch.float32).contiguous()
    ranks = torch.empty(B, N, dtype=torch.int32, device=a.device)
    nbytes = lib.bx_rank_desc_workspace(B, N)
    if nbytes == 0:
        L.check(-1, "bx_rank_desc_workspace")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        L.check(lib.bx_rank_desc(_p(a), _p(ranks), B, N, _p(ws), nbytes, _stream()), "bx_rank_desc")
    return ranks


def _faith_chunks(B, P, max_rows):
    """(b0, nb, i0, n): sample groups x windows of curve points with nb * n <= max_rows rows (one row when max_rows < 1); the rows of
    a sample sit together, which is what lets the unchanged branch's output be repeated instead of recomputed."""
    nb = max(1, min(B, max_rows))
    n = max(1, max_rows // nb)
    for b0 in range(0, B, nb):
        for i0 in range(0, P, n):
            yield b0, min(nb, B - b0), i0, min(n, P - i0)


def _empty_rows(x, rows, dt, eeg_rows):
    """-> (out, dims): ``rows`` empty rows in the model's layout, [rows,H,W,pad8(C)] in dt with dims = (C, H, W, pad8(C)) for a
    spectrogram x [B,C,H,W], fp32 [rows,1,Chans,T] with dims = (Chans, T) for eeg_rows."""
    if eeg_rows:
        _, _, Chans, T = x.shape
        return torch.empty(rows, 1, Chans, T, dtype=torch.float32, device=x.device), (Chans, T)
    _, Cc, H, W = x.shape
    return torch.empty(rows, H, W, ops.pad8(Cc), dtype=dt, device=x.device), (Cc, H, W, ops.pad8(Cc))


def _row_buffers(x, base, kind, b0, nb, n, dt, eeg_rows):
    """What a row writer starts from -> (xs, bs, out, dims): samples b0..b0+nb-1 of x and of a kind-2 baseline (any other baseline as
    it is), and the nb*n empty rows of ``_empty_rows``."""
    return (x[b0:b0 + nb], base[b0:b0 + nb] if kind == 2 else base, *_empty_rows(x, nb * n, dt, eeg_rows))


def _faith_perturb(x, ranks, base, kind, b0, nb, i0, n, per, insertion, dt, map_rows=None):
    """Rows (b, j), b in b0..b0+nb-1, j in 0..n-1, of the perturbed batch at curve points i0 + j.  x: fp32 [B,C,H,W] -> internal
    layout [nb*n,H,W,8] in dt (bx_faith_perturb_spec), or with map_rows fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T] (bx_faith_perturb_eeg)."""
    lib = L.load()
    xs, bs, out, dims = _row_buffers(x, base, kind, b0, nb, n, dt, map_rows is not None)
    rs = ranks[b0:b0 + nb]
    if map_rows is None:
        L.check(lib.bx_faith_perturb_spec(_p(xs), _p(rs), _p(bs), kind, _p(out), nb, *dims, per, i0, n, 1 if insertion else 0, ops.bx_dtype(dt),
                                          _stream()), "bx_faith_perturb_spec")
    else:
        L.check(lib.bx_faith_perturb_eeg(_p(xs), _p(rs), map_rows, _p(bs), kind, _p(out), nb, *dims, per, i0, n, 1 if insertion else 0, _stream()),
                "bx_faith_perturb_eeg")
    return out


def _baseline_for(who, baseline, x, per_len, what):
    """-> (kind, fp32 host or device tensor): 0 one value, 1 one per channel / electrode, 2 a tensor of the input's shape."""
    if isinstance(baseline, numbers.Real) and not isinstance(baseline, bool):
        return 0, torch.tensor([float(baseline)], dtype=torch.float32)
    try:
        t = baseline.detach() if isinstance(baseline, torch.Tensor) else torch.as_tensor(np.asarray(baseline, dtype=np.float32))
    except (TypeError, ValueError) as exc:
        raise ValueError(f"{who}: baseline is neither a number, a sequence nor a tensor ({exc})") from None
    if t.dim() == 0:
        return 0, t.reshape(1)
    if t.dim() == 1 and t.shape[0] == per_len:
        return 1, t
    if tuple(t.shape) == tuple(x.shape) or (x.shape[1] == 1 and tuple(t.shape) == (x.shape[0],) + tuple(x.shape[2:])):
        return 2, t
    raise ValueError(f"{who}: baseline of shape {tuple(t.shape)} is none of: a number, one value per {what} [{per_len}], "
                     f"a tensor of the input's shape {tuple(x.shape)}")


def _faith_baseline(baseline, x, per_len, what):
    return _baseline_for("deletion_insertion", baseline, x, per_len, what)


# ---- what the drivers that run rows through the model share: each driver keeps its own order of checks, built from the pieces below;
# the checks every one of them makes -- the input, the tensors, the model, the classes, the GPU -- fill one record, _Call, and the
# passes are built from it.  The perturb-and-predict drivers (deletion_insertion, rise, occlusion, kernel_shap, score_cam,
# spectral_occlusion, infidelity) keep their own clean pass and send their rows through one _RowPass; the gradient drivers
# (gradient_shap, smooth_grad, blur_ig, spectral_gradients by its sampled route; guided_ig, mask_explain by its per-row route) go
# through one _GradPass ----
@contextlib.contextmanager
def _lap(profile, name):
    """Device events around a phase, appended to ``profile`` as (name, start, end); nothing when profile is None."""
    if profile is None:
        yield
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    profile.append((name, e0, e1))


def _max_batch(who, v):
    v = int(v)
    if v < 1:
        raise ValueError(f"{who}: max_batch = {v} < 1")
    return v


def _draw_count(who, nsamples):
    if isinstance(nsamples, bool) or not isinstance(nsamples, numbers.Integral):
        raise ValueError(f"{who}: nsamples must be an int, got {nsamples!r}")
    if int(nsamples) < 1:
        raise ValueError(f"{who}: nsamples = {int(nsamples)} < 1")
    return int(nsamples)


def _stream_seed(who, seed):
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{who}: seed must be an int in [0, 2^64), got {seed!r}")
    return int(seed)


def _nonempty(who, x):
    """-> B, the samples of an input that has elements."""
    B = int(x.shape[0])
    if B < 1 or x.numel() == 0:
        raise ValueError(f"{who}: empty input of shape {tuple(x.shape)}")
    return B


def _level_or_absolute(who, B, level_name, level, absolute_name, absolute, default, level_first):
    """-> (level, None) or (None, absolute fp32 host [B]): a scale given as a fraction of each sample's range (``default`` when neither
    is given) or as the caller's absolute value, a number or one per sample.  smooth_grad's wording (level_first) names the level
    first and reports a level beyond fp32 in a message of its own; sensitivity_max's folds that case into its one message."""
    if level is not None and absolute is not None:
        raise ValueError(f"{who}: give {level_name if level_first else absolute_name} or {absolute_name if level_first else level_name}, not both")
    if absolute is None:
        lv = default if level is None else level
        if isinstance(lv, bool) or not isinstance(lv, numbers.Real) or not math.isfinite(lv) or lv < 0 or (lv > 3.0e38 and not level_first):
            raise ValueError(f"{who}: {level_name} must be a finite number >= 0, got {level!r}")
        if lv > 3.0e38:
            raise ValueError(f"{who}: {level_name} {level!r} is beyond fp32")
        return float(lv), None
    if isinstance(absolute, torch.Tensor):
        a = absolute.detach().to("cpu", torch.float64).numpy()
        if a.shape != (B,):
            raise ValueError(f"{who}: {absolute_name} of shape {tuple(absolute.shape)}; expected a number or [B] = [{B}]")
    elif isinstance(absolute, numbers.Real) and not isinstance(absolute, bool):
        a = np.full(B, float(absolute), dtype=np.float64)
    else:
        raise ValueError(f"{who}: {absolute_name} must be a number or a tensor [B], got {type(absolute).__name__}")
    if not np.isfinite(a).all() or (a < 0).any() or (a > 3.0e38).any():
        raise ValueError(f"{who}: {absolute_name} must be finite and >= 0")
    return None, np.ascontiguousarray(a.astype(np.float32))


def _range_scale(xs, level, host_values):
    """fp32 [B] on the device of xs (fp32, contiguous): ``level`` times each sample's range (bx_smoothgrad_sigma), or the caller's own
    values uploaded -- the two results of ``_level_or_absolute``."""
    if host_values is not None:
        return torch.from_numpy(host_values).to(xs.device)
    B = int(xs.shape[0])
    scale = torch.empty(B, dtype=torch.float32, device=xs.device)
    L.check(L.load().bx_smoothgrad_sigma(_p(xs), _p(scale), B, xs.numel() // B, level, _stream()), "bx_smoothgrad_sigma")
    return scale


def _per_cell(who, x, input_is_spec):
    """-> (per_len, what): the length and the name of a one-value-per-channel / per-electrode baseline; a spectrogram has 1..4 channels."""
    if not input_is_spec:
        return int(x.shape[2]), "electrode"
    Cc = int(x.shape[1])
    if not 1 <= Cc <= _FAITH_MAX_C:
        raise ValueError(f"{who}: {Cc} channels, supported 1..{_FAITH_MAX_C}")
    return Cc, "channel"


def _need_gpu(who, what, model, *tensors):
    """The closing refusal: every tensor that is given (None: a stand-alone model's other input) and the model live on the GPU."""
    if not (all(t.is_cuda for t in tensors if t is not None) and next(model.parameters()).is_cuda):
        raise RuntimeError(f"brainxai.{who}: {what} must live on the GPU; there is no CPU path")


def _explained_classes(who, class_idx, B, K, allow_all):
    """-> (cls_h, all_classes): one class per sample as a host list (None: the arg-max of the clean input, or every class)."""
    use, must = ("None, an int, one class per sample or 'all'", "None, an int, 'all' or") if allow_all else ("None, an int or one class per sample", "None, an int or")
    if class_idx is None:
        return None, False
    if isinstance(class_idx, str):
        if not (allow_all and class_idx == "all"):
            raise ValueError(f"{who}: class_idx {class_idx!r}; use {use}")
        return None, True
    if isinstance(class_idx, numbers.Integral) and not isinstance(class_idx, bool):
        cls_h = [int(class_idx)] * B
    else:
        cls_t = class_idx.detach().cpu() if isinstance(class_idx, torch.Tensor) else torch.as_tensor(np.asarray(class_idx))
        if cls_t.dim() != 1 or cls_t.shape[0] != B or cls_t.dtype.is_floating_point or cls_t.dtype == torch.bool:
            raise ValueError(f"{who}: class_idx must be {must} {B} integers (one class per sample)")
        cls_h = [int(c) for c in cls_t.tolist()]
    if any(not 0 <= c < K for c in cls_h):
        raise ValueError(f"{who}: class outside [0, {K})")
    return cls_h, False


class _Call:
    """The record of a checked call: what a driver establishes before its pass, and what the pass is then built from.  It is filled in
    steps, each a refusal or two and the fields they make safe to read, because the drivers put checks of their own between them:
      named(input)           'spec' or 'eeg'                                     -> input, input_is_spec
      tensors(eeg, spec)     the explained tensor, [B,C,H,W] or [B,1,Chans,T]    -> x, other, B, per (the elements of a sample)
      target()               the model and the other input                      -> multimodal, K, net, dt (the rows' storage dtype)
      classes(class_idx)     at most 32 classes, then ``_explained_classes``     -> cls_h, all_classes, Kc (K for 'all', else 1)
      need_gpu(what, *extra) the closing refusal: the model, x, the other input of a MultimodalModel and the driver's extras
    ``explained`` is target and classes, which most drivers make one after the other.  Three drivers join late: spectral_gradients
    and spectral_occlusion have no input to name (input='eeg' at construction), tcav resolves its input from the target (the same),
    and score_cam, which words the tensors' refusals by target, hands in the tensors it checked (``given``).  sensitivity_max, which
    explains a function, has no model: it stops after the tensors."""

    def __init__(self, who, model, input=None):
        self.who, self.model, self.input, self.input_is_spec = who, model, input, input == "spec"

    def named(self, input):
        if input not in _FAITH_INPUTS:
            raise ValueError(f"{self.who}: unknown input {input!r}; use 'spec' or 'eeg'")
        self.input, self.input_is_spec = input, input == "spec"
        return self

    def tensors(self, eeg, spec):
        x, form = (spec, "[B,C,H,W]") if self.input_is_spec else (eeg, "[B,1,Chans,T]")
        if x is None:
            raise ValueError(f"{self.who}: input={self.input!r} but that tensor is None")
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or (not self.input_is_spec and x.shape[1] != 1):
            raise ValueError(f"{self.who}: the {self.input} input must be a tensor {form}")
        return self.given(x, eeg if self.input_is_spec else spec)

    def given(self, x, other):
        self.x, self.other, self.B = x, other, int(x.shape[0])
        self.per = x.numel() // self.B if self.B else 0              # an empty batch is the driver's to refuse
        return self

    def target(self):
        """Whether ``model`` has both branches (``other`` is then the input of the branch that does not read x), its class count, and
        the branch that reads x.  score_cam words the two stand-alone refusals by target, the others by input."""
        who, model = self.who, self.model
        self.multimodal = hasattr(model, "spectrogram_model") and hasattr(model, "eeg_model")
        what = f"input={self.input!r}"
        if who == "score_cam":
            what = "a spectrogram target" if self.input_is_spec else "an EEG target"
        if self.multimodal:
            if not isinstance(self.other, torch.Tensor) or self.other.shape[0] != self.x.shape[0]:
                raise ValueError(f"{who}: a MultimodalModel needs both inputs with the same batch size")
            self.K, self.net = int(model.fc2.out_features), model.spectrogram_model if self.input_is_spec else model.eeg_model
        elif self.input_is_spec:
            if not (hasattr(model, "block1") and hasattr(model, "fc")):
                raise ValueError(f"{who}: {what} needs a MultimodalModel or a Spectrogram_Model")
            self.K, self.net = int(model.fc.out_features), model
        else:
            if not hasattr(model, "depthwiseConv"):
                raise ValueError(f"{who}: {what} needs a MultimodalModel, an EEGNet or an EEGNetAttentionDeep")
            self.K, self.net = int(model.dense.out_features if hasattr(model, "dense") else model.dense2.out_features), model
        self.dt = getattr(self.net, "compute_dtype", torch.float32) if self.input_is_spec else torch.float32
        return self

    def classes(self, class_idx, allow_all=True):
        """One class per sample as a host list, or every class; the 32-class limit is that of the drivers that can explain every class."""
        if allow_all and self.K > _RISE_MAX_K:
            raise ValueError(f"{self.who}: {self.K} classes, supported 1..{_RISE_MAX_K}")
        self.cls_h, self.all_classes = _explained_classes(self.who, class_idx, self.B, self.K, allow_all)
        self.Kc = self.K if self.all_classes else 1
        return self

    def explained(self, class_idx):
        return self.target().classes(class_idx)

    def need_gpu(self, what, *extra):
        _need_gpu(self.who, what, self.model, self.x, self.other if self.multimodal else None, *extra)

    def row_cap(self, max_batch, beside=0):
        return _row_cap(self.x, self.input, self.dt, max_batch, beside)


def _row_cap(x, input, dt, max_batch, beside=0):
    """Rows per forward pass: max_batch, capped so that a pass addresses its largest activation with 32-bit byte offsets -- stage 1's
    H x W x 16 channels in dt for a spectrogram [B,C,H,W], EEGNet's F1 x Chans x T in fp32 for an EEG input [B,1,Chans,T].  beside: the
    bytes per row of a buffer the driver keeps beside the rows (blur_ig's D), addressed within the same limit."""
    cells = int(x.shape[2]) * int(x.shape[3])
    row_bytes = cells * 16 * (2 if dt == torch.bfloat16 else 4) if input == "spec" else 8 * cells * 4
    return max(1, min(max_batch, ((1 << 31) - 1) // max(row_bytes, beside)))


def _fixed_branch(model, other, input_is_spec):
    """The output of the branch whose input does not change, fp32 [B, features]: once per sample."""
    o = other.detach().to(torch.float32).contiguous()
    return (model.eeg_model(o) if input_is_spec else model.spectrogram_model(o)).float().contiguous()


def _fuse(model, multimodal, input_is_spec, out, rep):
    """Log-probabilities of the whole model from the perturbed branch's output and the other branch's output ``rep``, row for row."""
    if not multimodal:
        return out
    e, s = (rep, out) if input_is_spec else (out, rep)
    return ops.FusionHeadFn.apply(e, s, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)


def _rows_forward(model, net, multimodal, input_is_spec, rows, rep):
    """fp32 log-probabilities [rows, K] of a batch in the model's layout (spectrogram rows are the internal NHWC layout: the branch gets
    a logical-NCHW view, no further copy)."""
    out = net(rows.permute(0, 3, 1, 2) if input_is_spec else rows)
    return _fuse(model, multimodal, input_is_spec, out, rep).float().contiguous()


def _softmax_rows(logp):
    """fp32 probabilities of fp32 log-probabilities [rows, K] (bx_softmax_rows)."""
    probs = torch.empty_like(logp)
    L.check(L.load().bx_softmax_rows(_p(logp), _p(probs), logp.shape[0], logp.shape[1], _stream()), "bx_softmax_rows")
    return probs


def _class_tensor(cls_h, all_classes, clean_scores, dev):
    """The explained classes as int32 [B] on the device, None for every class: the host list of ``_explained_classes``, or the arg-max
    of the clean input's fp32 scores [B, K]."""
    if cls_h is not None:
        return torch.tensor(cls_h, dtype=torch.int32, device=dev)
    if all_classes:
        return None
    return clean_scores.argmax(dim=1).to(torch.int32).contiguous()


class _Pass:
    """What the row pass and the gradient pass are built from alike: a checked ``_Call``, whose facts they keep under their own names,
    the device, the rows per forward pass (``_row_cap``), the unchanged branch's output ``fixed`` (None until ``fix_other`` and for a
    stand-alone model) and the laps of ``profile``.  ``xs`` is the explained input, fp32 and contiguous inside ``open()``."""

    def __init__(self, call, max_batch, profile, beside=0):
        self.call, self.profile, self.fixed = call, profile, None
        self.model, self.net, self.multimodal, self.K, self.input_is_spec = call.model, call.net, call.multimodal, call.K, call.input_is_spec
        self.xs, self.dev, self.B, self.dt = call.x, call.x.device, call.B, call.dt
        self.max_rows = call.row_cap(max_batch, beside)

    def lap(self, name):
        return _lap(self.profile, name)

    def fix_other(self):
        """Run the branch whose input does not change, once per sample (nothing for a stand-alone model); the lap is the caller's."""
        if self.multimodal:
            self.fixed = _fixed_branch(self.model, self.call.other, self.input_is_spec)


class _RowPass(_Pass):
    """What the five drivers do alike once their arguments are checked: rows of perturbed samples, written in the model's layout, run
    through the branch that reads them, the other branch's per-sample output is repeated into the fusion head, and the scores of every
    class land in fp32 [B, N, K].  A driver brings its row writer and its clean pass; the chunking by max_batch, the layout, the repeat,
    the fusion and the 'perturb' / 'forward' laps of ``profile`` are here.  Inside ``open()``, ``xs`` is the explained input (fp32,
    contiguous) and ``base`` the baseline on the device in its kind's shape."""

    def __init__(self, call, kind, base, max_batch, profile):
        super().__init__(call, max_batch, profile)
        self.kind, self.base = kind, base

    @contextlib.contextmanager
    def open(self):
        """The pass's device, eval mode with frozen parameters, no autograd."""
        with torch.cuda.device(self.dev), _eval_frozen(self.model), torch.no_grad():
            self.xs = self.xs.detach().to(torch.float32).contiguous()
            self.base = self.base.to(self.dev, torch.float32).reshape(self.xs.shape if self.kind == 2 else (-1,)).contiguous()
            yield self

    def groups(self):
        """(b0, nb): the samples in groups of at most max_rows, the groups of ``sweep``."""
        for b0 in range(0, self.B, self.max_rows):
            yield b0, min(self.max_rows, self.B - b0)

    def clean_rows(self, b0, nb):
        """Samples b0..b0+nb-1 unperturbed, in the layout of the rows."""
        return ops.to_nhwc(self.xs[b0:b0 + nb], self.dt) if self.input_is_spec else self.xs[b0:b0 + nb]

    def scores(self, rows, b0, nb, n=1, logprob=False):
        """fp32 [nb*n, K] log-probabilities (logprob) or probabilities of rows in the model's layout, n consecutive ones per sample of
        b0..b0+nb-1; one row per sample takes the other branch's output as it is, without the launch of a repeat."""
        rep = None
        if self.fixed is not None:
            rep = self.fixed[b0:b0 + nb]
            if n > 1:
                rep = rep.repeat_interleave(n, dim=0)
        logp = _rows_forward(self.model, self.net, self.multimodal, self.input_is_spec, rows, rep)
        return logp if logprob else _softmax_rows(logp)

    def sweep(self, N, write, logprob=False):
        """fp32 [B, N, K]: the scores of the N perturbed rows of every sample; ``write(b0, nb, n0, n)`` returns rows (b, j), b in
        b0..b0+nb-1, j in n0..n0+n-1, sample-major, in the model's layout."""
        out = torch.empty(self.B, N, self.K, dtype=torch.float32, device=self.dev)
        for b0, nb, n0, n in _faith_chunks(self.B, N, self.max_rows):
            with self.lap("perturb"):
                rows = write(b0, nb, n0, n)
            with self.lap("forward"):
                out[b0:b0 + nb, n0:n0 + n] = self.scores(rows, b0, nb, n, logprob).reshape(nb, n, self.K)
        return out


def _sample_chunks(total, max_rows):
    """(row0, rows): sample-major rows j = b * n + k in windows of at most max_rows, which may begin and end inside a sample."""
    for row0 in range(0, total, max_rows):
        yield row0, min(max_rows, total - row0)


def _sample_of(row0, rows, n, dev):
    """int64 [rows] on the device: the sample b = j // n of rows j = row0..row0+rows-1."""
    return torch.div(torch.arange(row0, row0 + rows, dtype=torch.int64, device=dev), n, rounding_mode="floor")


class _GradPass(_Pass):
    """What the gradient drivers do alike once their arguments are checked: rows run through the branch that reads them with the other
    branch's per-sample output gathered into the fusion head, and backward passes from one-hot seeds (bx_expgrad_seed), in chunks of at
    most max_batch rows.  Two routes, one pass object:
      sampled  (gradient_shap, smooth_grad, blur_ig, spectral_gradients): n sampled rows per sample, sample-major; ``sweep`` runs every
               chunk forward once and backward once per explained class slot.  The driver brings its row writer and its accumulate;
               ``sums`` are the fp64 sums carried between chunks.
      per row  (guided_ig, mask_explain; built with n = 1): R = B * Kc rows, one per (sample, class), iterated; ``row_steps`` runs every
               chunk of every iteration forward and backward once, the seed naming each row's own class (``row_classes``).  The driver
               brings its row writer and its step; ``baseline_rows`` / ``endpoint`` are the path's other end, ``stopped`` the one read of
               the rows' status, ``per_row`` the class axis of what the driver kept per row.
    The clean pass, the 'forward' / 'rows' / 'backward' / 'accumulate' / 'step' laps of ``profile``, ``finish_values``, ``completeness``
    and ``result`` serve both.  Inside ``open()``, ``xs`` is the explained input (fp32, contiguous); ``clean`` sets ``out``, ``classes``
    and ``fixed`` (None for a stand-alone model).  Cc, HW: the channels and pixels a finish launch reduces over."""

    def __init__(self, call, n, max_batch, profile, beside=0):
        super().__init__(call, max_batch, profile, beside)
        self.n, self.cls_h, self.all_classes, self.per, self.Kc, self.total = n, call.cls_h, call.all_classes, call.per, call.Kc, call.B * n
        self.max_rows = min(self.max_rows, ((1 << 31) - 1) // self.per)
        self.Cc, self.HW = (int(call.x.shape[1]), int(call.x.shape[2]) * int(call.x.shape[3])) if self.input_is_spec else (1, self.per)

    @contextlib.contextmanager
    def open(self):
        """The pass's device, eval mode with frozen parameters; autograd stays on, for the gradients with respect to the rows."""
        with torch.cuda.device(self.dev), _eval_frozen(self.model):
            self.xs = self.xs.detach().to(torch.float32).contiguous()
            yield self

    def clean(self):
        """The clean pass: the branch whose input does not change (once per sample), ``out`` fp32 [B,K] and the explained classes."""
        with torch.no_grad(), self.lap("forward"):
            self.fix_other()
            self.out = _fuse(self.model, self.multimodal, self.input_is_spec, self.net(self.xs), self.fixed).float().contiguous()
        self.classes = _class_tensor(self.cls_h, self.all_classes, self.out, self.dev)

    def sums(self, count):
        """``count`` fp64 zero sums [B,Kc,per]: what is carried between chunks, so that no bit depends on max_batch."""
        return [torch.zeros(self.B, self.Kc, self.per, dtype=torch.float64, device=self.dev) for _ in range(count)]

    def forward(self, r, row0, rows, per_sample):
        """fp32 [rows, K]: the model's output of rows row0..row0+rows-1, ``per_sample`` consecutive ones per sample, with the other
        branch's output of the sample each row belongs to."""
        rep = self.fixed.index_select(0, _sample_of(row0, rows, per_sample, self.dev)) if self.multimodal else None
        return _fuse(self.model, self.multimodal, self.input_is_spec, self.net(r), rep).float()

    def sweep(self, write, accumulate):
        """For every chunk: ``write(row0, rows)`` returns the fp32 rows in the input's own layout; one forward pass; then per class slot
        one backward pass and ``accumulate(g, slot, row0, rows)``, g fp32 contiguous: the gradient of the slot's class by the rows."""
        lib = L.load()
        for row0, rows in _sample_chunks(self.total, self.max_rows):
            with self.lap("rows"):
                r = write(row0, rows)
            with self.lap("forward"):
                r.requires_grad_(True)
                y = self.forward(r, row0, rows, self.n)
            seed_rows = torch.empty(rows, self.K, dtype=torch.float32, device=self.dev)
            for slot in range(self.Kc):
                with self.lap("backward"):
                    L.check(lib.bx_expgrad_seed(_p(self.classes), slot if self.all_classes else -1, _p(seed_rows), self.B, self.n, self.K, row0, rows,
                                                _stream()), "bx_expgrad_seed")
                    (g,) = torch.autograd.grad(y, r, grad_outputs=seed_rows, retain_graph=slot + 1 < self.Kc)
                    g = g.to(torch.float32).contiguous()
                with self.lap("accumulate"):
                    accumulate(g, slot, row0, rows)
            del y, r

    def row_classes(self):
        """int32 [R], contiguous: the class of every (sample, class) row."""
        if not self.all_classes:
            return self.classes.contiguous()
        return torch.arange(self.K, dtype=torch.int32, device=self.dev).repeat(self.B).contiguous()

    def baseline_rows(self, kind, base):
        """The baseline of ``_baseline_for`` as a contiguous fp32 tensor of the input's shape, on the device."""
        base = base.to(self.dev, torch.float32)
        if kind == 2:
            return base.reshape(self.xs.shape).contiguous()
        return base.reshape((1, -1, 1, 1) if self.input_is_spec or kind == 0 else (1, 1, -1, 1)).expand_as(self.xs).contiguous()

    def endpoint(self, xb):
        """fp32 [B,K]: the model's output at ``xb`` (the input's shape), the other branch's output as in the clean pass."""
        with torch.no_grad(), self.lap("forward"):
            return _fuse(self.model, self.multimodal, self.input_is_spec, self.net(xb), self.fixed).float().contiguous()

    def row_steps(self, iterations, write, step, rows_lap=False):
        """For every iteration i and every chunk of the R = B * Kc rows: ``write(row0, rows)`` returns the fp32 rows in the input's own
        layout (under the 'rows' lap with rows_lap; a writer that returns a view of rows the driver keeps has nothing to time); one
        forward pass; one backward pass from the seed of each row's own class; then ``step(i, g, y, row0, rows)``, g the gradient by the
        rows and y the model's output of them, both fp32, contiguous and detached."""
        lib, R = L.load(), self.B * self.Kc
        row_cls = self.row_classes()
        seed_rows = torch.empty(min(self.max_rows, R), self.K, dtype=torch.float32, device=self.dev)
        for i in range(iterations):
            for row0, rows in _sample_chunks(R, self.max_rows):
                with self.lap("rows") if rows_lap else contextlib.nullcontext():
                    r = write(row0, rows)
                with self.lap("forward"):
                    r.requires_grad_(True)
                    y = self.forward(r, row0, rows, self.Kc)
                with self.lap("backward"):
                    L.check(lib.bx_expgrad_seed(_p(row_cls), -1, _p(seed_rows), R, 1, self.K, row0, rows, _stream()), "bx_expgrad_seed")
                    (g,) = torch.autograd.grad(y, r, grad_outputs=seed_rows[:rows])
                    g, yd = g.to(torch.float32).contiguous(), y.detach().contiguous()
                del y, r
                with self.lap("step"):
                    step(i, g, yd, row0, rows)

    def stopped(self, who, status, ok, why):
        """The one read of the rows' status words (int32 [R]): the first row that is not ``ok`` is reported as its (sample, class slot),
        with ``why(code)`` as the reason."""
        st = status.cpu()
        if bool((st != ok).any()):
            bad = int((st != ok).nonzero()[0])
            raise RuntimeError(f"brainxai.{who}: sample {bad // self.Kc}, class slot {bad % self.Kc} stopped: {why(int(st[bad]))}")

    def per_row(self, t):
        """What a driver kept per row, [R,...], with the class axis [B,Kc,...] for class_idx='all'; None stays None."""
        return t.reshape(self.B, self.Kc, *t.shape[1:]) if t is not None and self.all_classes else t

    def finish_values(self, acc, n):
        """-> (values fp32 [B,Kc,*x.shape[1:]], map fp32 [B,Kc,*x.shape[2:]]): the fp64 sums [B*Kc, per] divided by n and rounded, and
        summed over the channels (bx_expgrad_finish); the lap is the driver's."""
        values = self.empty(*self.xs.shape[1:])
        amap = self.empty(*self.xs.shape[2:]) if self.input_is_spec else None
        L.check(L.load().bx_expgrad_finish(_p(acc), _p(values), _p(amap), self.B * self.Kc, self.Cc, self.HW, n, _stream()), "bx_expgrad_finish")
        return values, values[:, :, 0] if amap is None else amap                  # an EEG input has one channel: the map is the values

    def empty(self, *trail):
        """fp32 [B,Kc,*trail], empty: ``empty(*xs.shape[1:])`` is the estimator element by element, for the driver's finish launch."""
        return torch.empty(self.B, self.Kc, *trail, dtype=torch.float32, device=self.dev)

    def completeness(self, values, per, reference):
        """fp64 [B] or [B,K]: the sum of the ``per`` values of each (sample, class) row (bx_blurig_sum_rows: fp64, fixed order) minus
        out - ``reference`` (fp32 [B,K], the model's output at the path's other end) of the row's class."""
        total = torch.empty(self.B, self.Kc, dtype=torch.float64, device=self.dev)
        L.check(L.load().bx_blurig_sum_rows(_p(values), _p(total), self.B * self.Kc, per, _stream()), "bx_blurig_sum_rows")
        drop = self.out.double() - reference.double()
        return total - drop if self.all_classes else (total - drop.gather(1, self.classes.long()[:, None]))[:, 0]

    def result(self, return_parts, parts, amap, values, *rest):
        """The map alone, or ``parts(map, values, classes int64 [B] or None, out, *rest)``; the class axis stays for class_idx='all' only."""
        if not self.all_classes:
            amap, values = amap[:, 0], values[:, 0]
        if not return_parts:
            return amap
        return parts(amap, values, None if self.classes is None else self.classes.long(), self.out, *rest)


def deletion_insertion(model, eeg, spec, attribution, *, input="spec", mode="both", steps=32, baseline=0.0, class_idx=None, score="prob",
                       max_batch=256):
    """Deletion and insertion curves of an attribution map (the causal metric of RISE, Petsiuk et al., BMVC 2018).

    The cells of the chosen input are ranked by decreasing attribution (``attribution_ranks``).  With per = ceil(N / steps), curve
    point i (0..steps) has the cut k_i = min(N, i * per).  Deletion input at point i: cells of rank < k_i come from the baseline, the
    others from the input; insertion: cells of rank < k_i come from the input, the others from the baseline.  Each curve follows
    p_c = softmax probability of the explained class (score='logprob': its log-probability); its area is RISE's
    (sum(curve) - curve[0]/2 - curve[-1]/2) / steps in fp64.  A faithful map gives a small deletion and a large insertion area.

    input:       'spec': attribution [B,H,W], a cell is a pixel with all its channels (C <= 4); 'eeg': attribution [B,Chans,T] (a cell is
                 one electrode at one time step) or [B,1,T] (a whole time column).  The outputs of grad_cam (int / None class),
                 saliency, a channel-reduced IG result and LimeExplanation.heatmap(label)[None] fit as they are.
    model:       a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None, input='spec'); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None, input='eeg') -- the convention of grad_cam.
    baseline:    a number; one value per channel (spec) / electrode (eeg); or a tensor of the input's shape (a per-sample mean, or a
                 blurred copy: ``gaussian_blur(x, sigma)`` returns one).
    class_idx:   None = each sample's arg-max class on the unperturbed input; an int; or one class per sample (sequence / tensor [B]).
    mode:        'both', 'deletion' or 'insertion'; the fields of the other mode are None.
    max_batch:   rows (perturbed samples) per forward pass.
    Forward-only: (steps + 1) * B evaluations per mode, in eval mode without autograd; the perturbed rows are written once, straight
    in the model's layout (bx_faith_perturb_*), and weights are packed once for the whole pass.  In a MultimodalModel the branch
    whose input does not change runs once per SAMPLE, not once per row, and its output is repeated into the fusion head: for
    input='eeg' that removes almost all of the work (the spectrogram branch dominates), for input='spec' it saves little.
    The training flag and every requires_grad are restored on return.  Returns ``FaithfulnessCurves``."""
    return _deletion_insertion(model, eeg, spec, attribution, input, mode, steps, baseline, class_idx, score, max_batch)


def _deletion_insertion(model, eeg, spec, attribution, input, mode, steps, baseline, class_idx, score, max_batch, profile=None):
    """``deletion_insertion`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'rank',
    'perturb', 'forward', 'curve' -- device events around every phase of the pass (tools/faithfulness_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "deletion_insertion"
    call = _Call(who, model).named(input)
    if mode not in _FAITH_MODES:
        raise ValueError(f"{who}: unknown mode {mode!r}; use one of " + ", ".join(f"'{m}'" for m in _FAITH_MODES))
    if score not in _FAITH_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    steps = int(steps)
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    if not isinstance(attribution, torch.Tensor):
        raise ValueError(f"{who}: attribution must be a tensor")
    B = call.B
    per_len, what = _per_cell(who, x, call.input_is_spec)
    if call.input_is_spec:
        H, W = int(x.shape[2]), int(x.shape[3])
        if tuple(attribution.shape) != (B, H, W):
            raise ValueError(f"{who}: wrong map shape {tuple(attribution.shape)} for input='spec'; expected [B,H,W] = {(B, H, W)}")
        map_rows, N = None, H * W
    else:
        Chans, T = int(x.shape[2]), int(x.shape[3])
        if tuple(attribution.shape) == (B, Chans, T):
            map_rows = Chans
        elif tuple(attribution.shape) == (B, 1, T):
            map_rows = 1
        else:
            raise ValueError(f"{who}: wrong map shape {tuple(attribution.shape)} for input='eeg'; expected [B,Chans,T] = {(B, Chans, T)} or "
                             f"[B,1,T] = {(B, 1, T)}")
        N = map_rows * T
    if B < 1 or not 1 <= N <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {N} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    if not 1 <= steps <= N:
        raise ValueError(f"{who}: steps = {steps} outside 1..N = {N}")
    K = call.target().classes(class_idx, allow_all=False).K
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    call.need_gpu("the model, its inputs and the attribution", attribution)

    lib = L.load()
    dev = x.device
    P, per = steps + 1, -(-N // steps)
    rp = _RowPass(call, kind, base, max_batch, profile)

    with rp.open():
        with rp.lap("rank"):
            ranks = attribution_ranks(attribution)
        if call.multimodal:
            with rp.lap("forward"):
                rp.fix_other()
        logps = {}
        for m in ("deletion", "insertion"):
            if mode in ("both", m):
                logps[m] = rp.sweep(P, lambda *chunk: _faith_perturb(rp.xs, ranks, rp.base, kind, *chunk, per, m == "insertion", rp.dt, map_rows),
                                    logprob=True)
        # there is no clean pass: the unperturbed input is a curve's first or last point
        unperturbed = logps["deletion"][:, 0] if "deletion" in logps else logps["insertion"][:, P - 1]
        classes = _class_tensor(call.cls_h, False, unperturbed, dev)
        res = {}
        with rp.lap("curve"):
            for m, logp in logps.items():
                curve = torch.empty(B, P, dtype=torch.float32, device=dev)
                auc = torch.empty(B, dtype=torch.float64, device=dev)
                L.check(lib.bx_faith_curve(_p(logp), _p(classes), _p(curve), _p(auc), B, P, K, 1 if score == "logprob" else 0, _stream()),
                        "bx_faith_curve")
                res[m] = (curve, auc)
    fractions = torch.tensor([min(N, i * per) / N for i in range(P)], dtype=torch.float64)
    d, i = res.get("deletion", (None, None)), res.get("insertion", (None, None))
    return FaithfulnessCurves(d[0], i[0], d[1], i[1], classes.long(), fractions, ranks)


# ------------------------------------------------------------------------------------------------
# RISE (Petsiuk et al., BMVC 2018): black-box saliency from randomly masked forward passes.  The definition is pinned in
# include/brainxai.h; tests/rise_ref.py restates it in numpy.
_RISE_MAX_G, _RISE_MAX_K, _RISE_MAX_MASKS = 32, 32, (1 << 24) - 1
_RISE_NORMALIZE, _RISE_CELLS = ("expected", "coverage"), ("electrode_time", "time")

RiseResult = collections.namedtuple("RiseResult", "saliency classes probs coverage bits shifts")
RiseResult.__doc__ = """What ``rise(..., return_parts=True)`` returns: ``saliency`` fp32 [B,Hm,Wm] or [B,K,Hm,Wm], ``classes`` int64 [B] (None for
class_idx='all'), ``probs`` fp32 [B,N,K] (the class probabilities of every masked input), ``coverage`` fp32 [Hm,Wm] = the sum of the
masks, all on the device; ``bits`` uint8 [N,gh,gw] and ``shifts`` int32 [N,2] = (dy, dx) on the host: ``masks=(bits, shifts)`` repeats the call."""


def _rise_geometry(who, grid, Hm, Wm):
    """-> (gh, gw, ch, cw): the grid as a pair, checked against the mask domain, and the cell size ceil(Hm / gh) x ceil(Wm / gw)."""
    if isinstance(grid, numbers.Integral) and not isinstance(grid, bool):
        gh = gw = int(grid)
        if Hm == 1:                                                   # a [1, T] domain has one row of cells
            gh = 1
    else:
        try:
            gh, gw = (int(v) for v in grid)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: grid must be an int or a pair (gh, gw), got {grid!r}") from None
    if not (1 <= gh <= min(_RISE_MAX_G, Hm) and 1 <= gw <= min(_RISE_MAX_G, Wm)):
        raise ValueError(f"{who}: grid {gh} x {gw} outside 1..min({_RISE_MAX_G}, {Hm}) x 1..min({_RISE_MAX_G}, {Wm})")
    return gh, gw, -(-Hm // gh), -(-Wm // gw)


def _rise_mask_set(who, num_masks, geom, p1, seed, masks):
    """-> (bits uint8 [N,gh,gw], shifts int32 [N,2]) on the host: drawn from np.random.RandomState(seed), or ``masks`` checked."""
    gh, gw, ch, cw = geom
    if isinstance(p1, bool) or not isinstance(p1, numbers.Real) or not 0.0 < float(p1) <= 1.0:
        raise ValueError(f"{who}: p1 = {p1!r} outside (0, 1]")
    if masks is None:
        N = int(num_masks)
        if not 1 <= N <= _RISE_MAX_MASKS:
            raise ValueError(f"{who}: num_masks = {N} outside 1..{_RISE_MAX_MASKS}")
        rs = np.random.RandomState(seed)
        bits = (rs.rand(N, gh, gw) < float(p1)).astype(np.uint8)
        dy = rs.randint(0, ch, N)
        dx = rs.randint(0, cw, N)
        return bits, np.stack([dy, dx], axis=1).astype(np.int32)
    try:
        bits, shifts = masks
        bits = np.asarray(bits.cpu() if isinstance(bits, torch.Tensor) else bits)
        shifts = np.asarray(shifts.cpu() if isinstance(shifts, torch.Tensor) else shifts)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: masks must be a pair (bits [N,{gh},{gw}], shifts [N,2])") from None
    if bits.ndim != 3 or bits.shape[1:] != (gh, gw) or not 1 <= bits.shape[0] <= _RISE_MAX_MASKS:
        raise ValueError(f"{who}: bits of shape {bits.shape}; expected [N,{gh},{gw}] with 1 <= N <= {_RISE_MAX_MASKS}")
    if shifts.shape != (bits.shape[0], 2) or shifts.dtype.kind not in "iu":
        raise ValueError(f"{who}: shifts of shape {shifts.shape} ({shifts.dtype}); expected integers [N,2] = {(bits.shape[0], 2)}")
    if bits.dtype.kind not in "biu" or not np.isin(bits, (0, 1)).all():
        raise ValueError(f"{who}: bits must hold 0 / 1 only")
    if (shifts < 0).any() or (shifts[:, 0] >= ch).any() or (shifts[:, 1] >= cw).any():
        raise ValueError(f"{who}: shifts outside [0, cell): dy in 0..{ch - 1}, dx in 0..{cw - 1}")
    return np.ascontiguousarray(bits.astype(np.uint8)), np.ascontiguousarray(shifts.astype(np.int32))


def rise_masks(size, *, num_masks=4000, grid=8, p1=0.5, seed=0, masks=None, device=None, return_parts=False):
    """The RISE masks themselves, fp32 [N,Hm,Wm] on the device (bx_rise_masks) -- for tests, plots and callers who want them;
    ``rise`` never builds them.  size = (Hm, Wm); grid, p1, seed, masks as in ``rise``.  return_parts: (masks, bits, shifts)."""
    who = "rise_masks"
    try:
        Hm, Wm = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be a pair (Hm, Wm), got {size!r}") from None
    if Hm < 1 or Wm < 1 or Hm * Wm > _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hm} x {Wm} cells per mask, supported 1..{_FAITH_MAX_N}")
    geom = _rise_geometry(who, grid, Hm, Wm)
    bits, shifts = _rise_mask_set(who, num_masks, geom, p1, seed, masks)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"brainxai.{who}: the masks are built on the GPU; there is no CPU path")
    lib = L.load()
    N = bits.shape[0]
    with torch.cuda.device(dev):
        bits_d, shifts_d = torch.from_numpy(bits).to(dev), torch.from_numpy(shifts).to(dev)
        out = torch.empty(N, Hm, Wm, dtype=torch.float32, device=dev)
        step = max(1, ((1 << 31) - 1) // (Hm * Wm))
        for n0 in range(0, N, step):
            n = min(step, N - n0)
            L.check(lib.bx_rise_masks(_p(bits_d), _p(shifts_d), _p(out[n0:n0 + n]), N, geom[0], geom[1], Hm, Wm, n0, n, _stream()), "bx_rise_masks")
    return (out, bits, shifts) if return_parts else out


def _rise_perturb(x, bits_d, shifts_d, geom, base, kind, b0, nb, n0, n, dt, map_rows=None):
    """Rows (b, j), b in b0..b0+nb-1, j in 0..n-1: sample b seen through mask n0 + j.  x fp32 [B,C,H,W] -> internal layout
    [nb*n,H,W,8] in dt (bx_rise_perturb_spec), or with map_rows fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T] (bx_rise_perturb_eeg)."""
    lib = L.load()
    xs, bs, out, dims = _row_buffers(x, base, kind, b0, nb, n, dt, map_rows is not None)
    N = bits_d.shape[0]
    if map_rows is None:
        L.check(lib.bx_rise_perturb_spec(_p(xs), _p(bits_d), _p(shifts_d), _p(bs), kind, _p(out), nb, *dims, N, geom[0], geom[1], n0, n,
                                         ops.bx_dtype(dt), _stream()), "bx_rise_perturb_spec")
    else:
        L.check(lib.bx_rise_perturb_eeg(_p(xs), _p(bits_d), _p(shifts_d), map_rows, _p(bs), kind, _p(out), nb, *dims, N, geom[0], geom[1], n0, n,
                                        _stream()), "bx_rise_perturb_eeg")
    return out


def rise(model, eeg, spec, *, input="spec", num_masks=4000, grid=8, p1=0.5, class_idx=None, baseline=0.0, normalize="expected", seed=0,
         masks=None, cells="electrode_time", max_batch=256, return_parts=False):
    """RISE saliency (Petsiuk et al., BMVC 2018): sal[b,k,p] = sum_n P[b,n,k] m_n(p) / D(p), where m_n is the n-th random smooth mask,
    P[b,n,k] the softmax probability of class k for the input base + m_n (x - base), and D the normaliser.  Forward-only, so it
    explains either input of the multimodal model; the map has the input's own shape and fits ``deletion_insertion`` and
    ``attribution_ranks`` as it is.

    input:       'spec': masks over [H,W], one value for all channels of a pixel (C <= 4), map [B,H,W]; 'eeg': masks over [Chans,T],
                 map [B,Chans,T], or with cells='time' over [1,T] (a column's value applies to every electrode), map [B,1,T].
    model:       a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None, input='spec'); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None, input='eeg') -- the convention of grad_cam and deletion_insertion.
    masks:       mask n is the crop [dy:dy+Hm, dx:dx+Wm] of the bilinear (align_corners=False) up-sampling of a gh x gw grid of 0 / 1
                 to (gh+1) ch x (gw+1) cw, ch = ceil(Hm / gh), cw = ceil(Wm / gw).  grid: an int or a pair, 1..min(32, Hm) x
                 1..min(32, Wm) (an int grid over a [1,T] domain means (1, grid)).  The draw is on the host from one
                 np.random.RandomState(seed): bits = rand(N, gh, gw) < p1, dy = randint(0, ch, N), dx = randint(0, cw, N);
                 masks=(bits [N,gh,gw], shifts [N,2]) replaces it.  One mask set serves the whole batch, as in the paper's code.
                 (The paper's code resizes with skimage.transform.resize(order=1, mode='reflect'): the same coordinate map, and for a
                 two-tap filter a reflected border equals the clamped one used here -- not checked here, skimage is not a dependency.)
    baseline:    what a masked-out cell shows: a number; one value per channel (spec) / electrode (eeg); a tensor of the input's shape.
    class_idx:   None = each sample's arg-max class on the unmasked input; an int; one class per sample (sequence / tensor [B]);
                 'all' = every class, the map gains a class axis [B,K,Hm,Wm] (K <= 32).
    normalize:   'expected': D = N p1, the paper's choice; 'coverage': D(p) = sum_n m_n(p), which removes the Monte-Carlo
                 unevenness of how often each cell was shown (at N = 256 that unevenness is most of an 'expected' map).
    max_batch:   rows (masked inputs) per forward pass.
    N * B forward evaluations in eval mode without autograd.  The masks never exist in memory: the masked rows are written straight in
    the model's layout from the bit grids (bx_rise_perturb_*), and the weighted sum recomputes every mask value in registers
    (bx_rise_accumulate, fp64, fixed order: identical bits run to run and for every max_batch).  In a MultimodalModel the branch whose
    input does not change runs once per sample and its output is repeated into the fusion head.  The training flag and every
    requires_grad are restored on return.  Returns the map (device, fp32), or ``RiseResult`` with return_parts."""
    return _rise(model, eeg, spec, input, num_masks, grid, p1, class_idx, baseline, normalize, seed, masks, cells, max_batch, return_parts)


def _rise(model, eeg, spec, input, num_masks, grid, p1, class_idx, baseline, normalize, seed, masks, cells, max_batch, return_parts, profile=None):
    """``rise`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'perturb', 'forward',
    'accumulate' -- device events around every phase of the pass (tools/rise_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "rise"
    call = _Call(who, model).named(input)
    if normalize not in _RISE_NORMALIZE:
        raise ValueError(f"{who}: unknown normalize {normalize!r}; use 'expected' or 'coverage'")
    if cells not in _RISE_CELLS:
        raise ValueError(f"{who}: unknown cells {cells!r}; use 'electrode_time' or 'time'")
    if cells == "time" and input != "eeg":
        raise ValueError(f"{who}: cells='time' masks time columns of the EEG input; input='spec' has no such map")
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = call.B
    per_len, what = _per_cell(who, x, call.input_is_spec)
    if call.input_is_spec:
        map_rows, Hm, Wm = None, int(x.shape[2]), int(x.shape[3])
    else:
        map_rows = 1 if cells == "time" else int(x.shape[2])
        Hm, Wm = map_rows, int(x.shape[3])
    if B < 1 or not 1 <= Hm * Wm <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hm * Wm} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    geom = _rise_geometry(who, grid, Hm, Wm)
    K, cls_h, all_classes = call.explained(class_idx).K, call.cls_h, call.all_classes
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    bits, shifts = _rise_mask_set(who, num_masks, geom, p1, seed, masks)
    N = int(bits.shape[0])
    if B * N * K >= 1 << 31 or B * K * Hm * Wm >= 1 << 31:
        raise ValueError(f"{who}: B * N * K = {B * N * K} or B * K * Hm * Wm = {B * K * Hm * Wm} beyond 32-bit offsets; use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    dev = x.device
    rp = _RowPass(call, kind, base, max_batch, profile)

    with rp.open():
        bits_d, shifts_d = torch.from_numpy(bits).to(dev), torch.from_numpy(shifts).to(dev)
        clean = None
        with rp.lap("forward"):
            rp.fix_other()
            if cls_h is None and not all_classes:                   # the explained class: the arg-max on the unmasked input, one pass
                clean = (model(eeg, spec) if call.multimodal else model(rp.xs)).float()
        classes = _class_tensor(cls_h, all_classes, clean, dev)
        P = rp.sweep(N, lambda *chunk: _rise_perturb(rp.xs, bits_d, shifts_d, geom, rp.base, kind, *chunk, rp.dt, map_rows))
        with rp.lap("accumulate"):
            sal = torch.empty((B, K, Hm, Wm) if all_classes else (B, Hm, Wm), dtype=torch.float32, device=dev)
            coverage = torch.empty(Hm, Wm, dtype=torch.float32, device=dev)
            L.check(lib.bx_rise_accumulate(_p(P), _p(classes), _p(bits_d), _p(shifts_d), _p(sal), _p(coverage), B, N, K, geom[0], geom[1], Hm, Wm,
                                           float(p1), 1 if normalize == "coverage" else 0, _stream()), "bx_rise_accumulate")
    if not return_parts:
        return sal
    return RiseResult(sal, None if classes is None else classes.long(), P, coverage, bits, shifts)


# ------------------------------------------------------------------------------------------------
# Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's Occlusion): the drop of the class score when a sliding window of the
# input is replaced by the baseline.  The definition is pinned in include/brainxai.h; tests/occlusion_ref.py restates it.
OcclusionResult = collections.namedtuple("OcclusionResult", "attribution drops classes scores clean counts grid")
OcclusionResult.__doc__ = """What ``occlusion(..., return_parts=True)`` returns: ``attribution`` fp32 [B,Hm,Wm] or [B,K,Hm,Wm] (what the plain call
returns), ``drops`` fp32 [B,ny,nx] or [B,K,ny,nx] = clean - scores per window, ``classes`` int64 [B] (None for class_idx='all'), ``scores``
fp32 [B,N,K] (the score of every class for every occluded input, window j = iy * nx + ix), ``clean`` fp32 [B,K] (the scores of the
unperturbed input), ``counts`` int32 [Hm,Wm] = the number of windows covering each cell, all on the device; ``grid`` = (ny, nx)."""


def _occlusion_pair(who, name, value):
    if isinstance(value, numbers.Integral) and not isinstance(value, bool):
        return int(value), int(value)
    try:
        a, b = value
        if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (a, b)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be an int or a pair of ints, got {value!r}") from None
    return int(a), int(b)


def _occlusion_geometry(who, window, stride, Hm, Wm):
    """-> (wh, ww, sh, sw, ny, nx): window and stride as pairs, checked against the domain, and the window positions per axis."""
    wh, ww = _occlusion_pair(who, "window", window)
    sh, sw = (wh, ww) if stride is None else _occlusion_pair(who, "stride", stride)
    if not (1 <= wh <= Hm and 1 <= ww <= Wm):
        raise ValueError(f"{who}: window {wh} x {ww} outside 1..{Hm} x 1..{Wm}")
    if not (1 <= sh <= wh and 1 <= sw <= ww):
        raise ValueError(f"{who}: stride {sh} x {sw} outside 1..window = {wh} x {ww} (a stride above the window leaves cells uncovered)")
    return wh, ww, sh, sw, 1 + -(-(Hm - wh) // sh), 1 + -(-(Wm - ww) // sw)


def _occlusion_perturb(x, geom, base, kind, b0, nb, n0, n, dt, eeg_input=False):
    """Rows (b, j), b in b0..b0+nb-1, j in 0..n-1: sample b with window n0 + j taken from the baseline.  x fp32 [B,C,H,W] -> internal
    layout [nb*n,H,W,8] in dt (bx_occlusion_perturb_spec), or with eeg_input fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T]
    (bx_occlusion_perturb_eeg)."""
    lib = L.load()
    xs, bs, out, dims = _row_buffers(x, base, kind, b0, nb, n, dt, eeg_input)
    if not eeg_input:
        L.check(lib.bx_occlusion_perturb_spec(_p(xs), _p(bs), kind, _p(out), nb, *dims, *geom[:4], n0, n, ops.bx_dtype(dt), _stream()),
                "bx_occlusion_perturb_spec")
    else:
        L.check(lib.bx_occlusion_perturb_eeg(_p(xs), _p(bs), kind, _p(out), nb, *dims, *geom[:4], n0, n, _stream()), "bx_occlusion_perturb_eeg")
    return out


def occlusion(model, eeg, spec, *, input="spec", window, stride=None, baseline=0.0, class_idx=None, score="prob", max_batch=256,
              return_parts=False):
    """Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's ``Occlusion``): slide a window over the input, replace it by the
    baseline and record how much the class score drops.  attr[b,k,p] = the mean, over the windows j that cover cell p, of
    S0[b,k] - S[b,j,k], with S0 the score of the unperturbed input and S[b,j,.] that of the input with window j occluded.
    Deterministic and forward-only, so it explains either input of the multimodal model; the map has the input's own shape and fits
    ``deletion_insertion`` and ``attribution_ranks`` as it is.

    input:       'spec': windows over [H,W], a cell is a pixel with all its channels (C <= 4), map [B,H,W]; 'eeg': windows over
                 [Chans,T], map [B,Chans,T].  window=(1, T) on the EEG input is electrode ablation, (Chans, w) time-segment
                 ablation; (h, W) / (H, w) on the spectrogram occlude a frequency band / a time slab.
    model:       a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None, input='spec'); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None, input='eeg') -- the convention of grad_cam, deletion_insertion and rise.
    window:      an int or a pair (wh, ww), 1 <= wh <= Hm, 1 <= ww <= Wm.
    stride:      None = the window itself (tiles); an int or a pair (sh, sw) with 1 <= sh <= wh, 1 <= sw <= ww (Captum's rule: every
                 cell is covered).  ny = 1 + ceil((Hm - wh) / sh) by nx = 1 + ceil((Wm - ww) / sw) windows, window j = iy * nx + ix at
                 rows iy * sh .., columns ix * sw ..; the last window of an axis is clipped at the border, as Captum's padded mask is.
    baseline:    what an occluded cell shows: a number; one value per channel (spec) / electrode (eeg); a tensor of the input's shape.
    class_idx:   None = each sample's arg-max class on the unperturbed input; an int; one class per sample (sequence / tensor [B]);
                 'all' = every class, the map gains a class axis [B,K,Hm,Wm] (K <= 32).
    score:       'prob': the softmax probability; 'logprob': the log-probability.
    max_batch:   rows (occluded inputs) per forward pass; no bit of the result depends on it.
    (N + 1) * B forward evaluations in eval mode without autograd.  The occluded rows are written straight in the model's layout
    (bx_occlusion_perturb_*: a selection, every element is bit for bit the input's or the baseline's); the map is an fp64 gather
    in fixed order, rounded once (bx_occlusion_accumulate).  In a MultimodalModel the branch whose input does not change runs once per
    sample and its output is repeated into the fusion head.  The training flag and every requires_grad are restored on return.
    Returns the map (device, fp32), or ``OcclusionResult`` with return_parts (its ``drops`` for window=(1, T) on the EEG input are
    the per-electrode importances)."""
    return _occlusion(model, eeg, spec, input, window, stride, baseline, class_idx, score, max_batch, return_parts)


def _occlusion(model, eeg, spec, input, window, stride, baseline, class_idx, score, max_batch, return_parts, profile=None):
    """``occlusion`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'perturb', 'forward',
    'accumulate' -- device events around every phase of the pass (tools/occlusion_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "occlusion"
    call = _Call(who, model).named(input)
    if score not in _FAITH_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = call.B
    Hm, Wm = int(x.shape[2]), int(x.shape[3])
    per_len, what = _per_cell(who, x, call.input_is_spec)
    if B < 1 or not 1 <= Hm * Wm <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hm * Wm} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    geom = _occlusion_geometry(who, window, stride, Hm, Wm)
    ny, nx = geom[4:]
    N = ny * nx
    K, cls_h, all_classes = call.explained(class_idx).K, call.cls_h, call.all_classes
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    if B * N * K >= 1 << 31 or B * K * Hm * Wm >= 1 << 31:
        raise ValueError(f"{who}: B * N * K = {B * N * K} or B * K * Hm * Wm = {B * K * Hm * Wm} beyond 32-bit offsets; use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    dev = x.device
    use_logprob = score == "logprob"
    rp = _RowPass(call, kind, base, max_batch, profile)

    with rp.open():
        with rp.lap("forward"):
            rp.fix_other()
            # the unperturbed input takes the path of the occluded rows, in chunks of the same size
            clean = torch.empty(B, K, dtype=torch.float32, device=dev)
            for b0, nb in rp.groups():
                clean[b0:b0 + nb] = rp.scores(rp.clean_rows(b0, nb), b0, nb, logprob=use_logprob)
        classes = _class_tensor(cls_h, all_classes, clean, dev)
        S = rp.sweep(N, lambda *chunk: _occlusion_perturb(rp.xs, geom, rp.base, kind, *chunk, rp.dt, input == "eeg"), logprob=use_logprob)
        with rp.lap("accumulate"):
            attr = torch.empty((B, K, Hm, Wm) if all_classes else (B, Hm, Wm), dtype=torch.float32, device=dev)
            counts = torch.empty(Hm, Wm, dtype=torch.int32, device=dev)
            L.check(lib.bx_occlusion_accumulate(_p(S), _p(clean), _p(classes), _p(attr), _p(counts), B, N, K, Hm, Wm, *geom[:4], _stream()),
                    "bx_occlusion_accumulate")
        if not return_parts:
            return attr
        d = clean[:, None, :] - S                                   # [B,N,K]
        if all_classes:
            drops = d.permute(0, 2, 1).reshape(B, K, ny, nx).contiguous()
        else:
            drops = d.gather(2, classes.long().reshape(B, 1, 1).expand(B, N, 1)).reshape(B, ny, nx)
    return OcclusionResult(attr, drops, None if classes is None else classes.long(), S, clean, counts, (ny, nx))


# ------------------------------------------------------------------------------------------------
# Kernel SHAP (Lundberg & Lee, NeurIPS 2017; paired sampling: Covert & Lee, AISTATS 2021): Shapley values of the segments of either
# input from forward passes alone.  The definition is pinned in include/brainxai.h; tests/kernel_shap_ref.py restates it.
_SHAP_MAX_M = 256

KernelShapResult = collections.namedtuple("KernelShapResult", "attribution values classes scores clean empty coalitions weights segments exact")
KernelShapResult.__doc__ = """What ``kernel_shap(..., return_parts=True)`` returns: ``attribution`` fp32 [B,Hm,Wm] or [B,K,Hm,Wm] (what the plain call
returns), ``values`` fp64 [B,M] or [B,K,M] = the Shapley value of every player (with segments='electrodes' the per-electrode
importances), ``classes`` int64 [B] (None for class_idx='all'), ``scores`` fp32 [B,N,K] (the score of every class under every coalition),
``clean`` / ``empty`` fp32 [B,K] (the scores of the unperturbed input and of the baseline), all on the device; ``coalitions`` uint8 [N,M],
``weights`` fp64 [N] and ``segments`` int32 [Hm,Wm] on the host (``coalitions=(coalitions, weights)`` repeats the call); ``exact``: whether
the set is every proper non-empty coalition, so that the values are the exact Shapley values."""


def _shap_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _shap_segments(who, segments, input, Hd, Wd):
    """-> (seg int32 [Hm,Wm] on the host, M): the label map over the map domain, [H,W] for a spectrogram and [Chans,T] or [1,T] for the
    EEG input (Hd x Wd is the input's own H x W / Chans x T)."""
    if isinstance(segments, str):
        if segments != "electrodes" or input != "eeg":
            raise ValueError(f"{who}: segments {segments!r}; use a label map, (rows, cols)" + (", 'electrodes' or ('time', n)" if input == "eeg" else
                                                                                              " (the words name segmentations of the EEG input)"))
        seg = np.repeat(np.arange(Hd, dtype=np.int32)[:, None], Wd, axis=1)
    elif isinstance(segments, (tuple, list)) and len(segments) == 2 and isinstance(segments[0], str) and segments[0] == "time":
        if input != "eeg" or not _shap_int(segments[1]) or not 1 <= segments[1] <= Wd:
            raise ValueError(f"{who}: segments {segments!r}; ('time', n) cuts the EEG input's {Wd} time steps into 1 <= n <= T slabs")
        seg = grid_segments(1, Wd, 1, int(segments[1]))
    elif isinstance(segments, (tuple, list)) and len(segments) == 2 and all(_shap_int(v) for v in segments):
        rows, cols = int(segments[0]), int(segments[1])
        if not (1 <= rows <= Hd and 1 <= cols <= Wd):
            raise ValueError(f"{who}: segments (rows, cols) = {(rows, cols)} outside 1..{Hd} x 1..{Wd}")
        seg = grid_segments(Hd, Wd, rows, cols)
    else:
        try:
            seg = segments.detach().cpu().numpy() if isinstance(segments, torch.Tensor) else np.asarray(segments)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{who}: segments is neither a label map, (rows, cols) nor a named segmentation ({exc})") from None
        if seg.dtype.kind not in "iu":
            raise ValueError(f"{who}: the label map must hold integers, got {seg.dtype}")
        shapes = [(Hd, Wd)] + ([(1, Wd)] if input == "eeg" else [])
        if tuple(seg.shape) not in shapes:
            raise ValueError(f"{who}: label map of shape {tuple(seg.shape)}; expected " + " or ".join(str(list(s)) for s in shapes))
    M = int(seg.max()) + 1
    if int(seg.min()) < 0 or not np.array_equal(np.unique(seg), np.arange(M)):
        raise ValueError(f"{who}: the labels must be 0..M-1 with every label present; got {np.unique(seg).size} labels in {int(seg.min())}..{M - 1}")
    if not 2 <= M <= _SHAP_MAX_M:
        raise ValueError(f"{who}: {M} players, supported 2..{_SHAP_MAX_M}")
    return np.ascontiguousarray(seg.astype(np.int32)), M


def _shap_coalitions(who, M, num_samples, seed, coalitions):
    """-> (Z uint8 [N,M], weights fp64 [N], exact): the coalition set of include/brainxai.h, built on the host."""
    if coalitions is not None:
        try:
            Z, w = coalitions
            Z = np.asarray(Z.detach().cpu() if isinstance(Z, torch.Tensor) else Z)
            w = None if w is None else np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: coalitions must be a pair (Z [N,M], weights [N] or None)") from None
        if Z.ndim != 2 or Z.shape[1] != M or Z.dtype.kind not in "biuf" or not np.isin(Z, (0, 1)).all():
            raise ValueError(f"{who}: coalitions must be 0 / 1 in shape [N, M = {M}], got {tuple(Z.shape)}")
        Z = np.ascontiguousarray(Z.astype(np.uint8))
        size = Z.sum(1)
        if ((size == 0) | (size == M)).any():
            raise ValueError(f"{who}: a coalition row is all-zero or all-one; the constraint already holds the baseline and the input")
        if w is None:
            w = np.ones(Z.shape[0], dtype=np.float64)
        if w.shape != (Z.shape[0],):
            raise ValueError(f"{who}: {w.size} weights for {Z.shape[0]} coalitions")
        if not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError(f"{who}: the weights must be positive and finite")
        exact = False
    else:
        if not _shap_int(num_samples):
            raise ValueError(f"{who}: num_samples must be an int or None, got {num_samples!r}")
        if (1 << M) - 2 <= num_samples:
            c = np.arange(1, (1 << M) - 1, dtype=np.int64)
            Z = ((c[:, None] >> np.arange(M, dtype=np.int64)[None, :]) & 1).astype(np.uint8)
            per_size = np.array([0.0] + [(M - 1) / (math.comb(M, s) * s * (M - s)) for s in range(1, M)])
            w, exact = per_size[Z.sum(1)], True
        else:
            N = int(num_samples) // 2 * 2
            if N < max(2, M - 1):
                raise ValueError(f"{who}: num_samples = {num_samples} gives N = {N} coalitions, which cannot determine {M} players (N >= M - 1)")
            rng = np.random.default_rng(seed)
            s = np.arange(1, M)
            p = (M - 1) / (s * (M - s))
            sizes = rng.choice(s, size=N // 2, p=p / p.sum())
            Z = np.zeros((N, M), dtype=np.uint8)
            for j, k in enumerate(sizes):
                Z[2 * j, rng.permutation(M)[:k]] = 1
                Z[2 * j + 1] = 1 - Z[2 * j]
            w, exact = np.ones(N, dtype=np.float64), False
    if Z.shape[0] < M - 1:
        raise ValueError(f"{who}: N = {Z.shape[0]} coalitions cannot determine {M} players (N >= M - 1)")
    return Z, np.ascontiguousarray(w), exact


def _shap_perturb(x, seg_d, Z_d, M, base, kind, b0, nb, n0, n, dt, map_rows=None):
    """Rows (b, j), b in b0..b0+nb-1, j in 0..n-1: sample b under coalition n0 + j of Z_d.  x fp32 [B,C,H,W] -> internal layout
    [nb*n,H,W,8] in dt (bx_shap_perturb_spec), or with map_rows fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T] (bx_shap_perturb_eeg)."""
    lib = L.load()
    xs, bs, out, dims = _row_buffers(x, base, kind, b0, nb, n, dt, map_rows is not None)
    N = Z_d.shape[0]
    if map_rows is None:
        L.check(lib.bx_shap_perturb_spec(_p(xs), _p(bs), kind, _p(out), nb, *dims, _p(seg_d), _p(Z_d), M, N, n0, n, ops.bx_dtype(dt), _stream()),
                "bx_shap_perturb_spec")
    else:
        L.check(lib.bx_shap_perturb_eeg(_p(xs), _p(bs), kind, _p(out), nb, *dims, map_rows, _p(seg_d), _p(Z_d), M, N, n0, n, _stream()),
                "bx_shap_perturb_eeg")
    return out


def _shap_fit(S, clean, empty, classes, Z_d, w_d):
    """phi fp64 [B,R,M] (R = 1 with classes, else K) of scores S fp32 [B,N,K] (bx_shap_fit); ValueError when the coalitions leave the
    values undetermined."""
    lib = L.load()
    B, N, K = S.shape
    M = Z_d.shape[1]
    nbytes = lib.bx_shap_fit_workspace(B, N, K, M, 1 if classes is None else 0)
    if nbytes == 0:
        L.check(-1, "bx_shap_fit_workspace")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=S.device)
    phi = torch.zeros(B, K if classes is None else 1, M, dtype=torch.float64, device=S.device)
    info = torch.zeros(1, dtype=torch.int32, device=S.device)
    L.check(lib.bx_shap_fit(_p(S), _p(clean), _p(empty), _p(classes), _p(Z_d), _p(w_d), B, N, K, M, _p(ws), nbytes, _p(phi), _p(info), _stream()),
            "bx_shap_fit")
    bad = int(info.item())
    if bad:
        raise ValueError(f"kernel_shap: the {N} coalitions leave the values of the {M} players undetermined (the fit's pivot {bad - 1} vanishes): "
                         "more samples are needed")
    return phi


def kernel_shap(model, eeg, spec, *, input="spec", segments, num_samples=None, baseline=0.0, class_idx=None, score="prob", seed=0, coalitions=None,
                max_batch=256, return_parts=False):
    """Kernel SHAP (Lundberg & Lee, NeurIPS 2017): the Shapley values of the M segments of one input, estimated from forward passes of
    coalitions -- the input on the segments of the coalition, the baseline elsewhere.  phi[b,k,.] minimises
    sum_n w_n (v(z_n) - v(0) - sum_i phi_i z_ni)^2 subject to sum_i phi_i = v(1) - v(0), with v(z) the class score under coalition z, so
    the values of a sample add up exactly to score(input) - score(baseline), which LIME, occlusion and RISE do not give.  Forward-only,
    so it explains either input of the multimodal model (the reference's SHAP, a GradientExplainer on the EEG branch reduced to
    per-electrode importances, is ``segments='electrodes'`` here); the map has the input's own shape and fits ``deletion_insertion`` and
    ``attribution_ranks`` as it is.

    input:       'spec': segments over [H,W], a cell is a pixel with all its channels (C <= 4), map [B,H,W]; 'eeg': segments over
                 [Chans,T], map [B,Chans,T], or over [1,T] (a label applies to every electrode), map [B,1,T].
    model:       a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None, input='spec'); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None, input='eeg') -- the convention of grad_cam, deletion_insertion, rise and occlusion.
    segments:    an int label map over the domain with the labels 0..M-1 all present (2 <= M <= 256; one map for the whole batch);
                 (rows, cols) = ``grid_segments(Hm, Wm, rows, cols)``; for the EEG input also 'electrodes' (label = electrode) and
                 ('time', n) (n slabs over [1,T]).
    num_samples: the budget of coalitions, None = 2 M + 2048.  When 2^M - 2 <= num_samples every proper non-empty coalition is used, in
                 increasing order of the integer whose bit i is player i, with the Shapley kernel w = (M-1) / (C(M,s) s (M-s)): the
                 exact Shapley values.  Otherwise N = num_samples rounded down to even; one np.random.default_rng(seed) draws
                 sizes = rng.choice(arange(1, M), N/2, p ~ (M-1) / (s (M-s))), row 2j = the players rng.permutation(M)[:sizes[j]], row
                 2j+1 its complement (paired sampling, Covert & Lee 2021), all weights 1.  One set serves the whole batch.
    coalitions:  (Z [N,M] of 0 / 1, weights [N] or None) replaces the set; an all-zero or all-one row is refused.
    baseline:    what a cell outside the coalition shows: a number; one value per channel (spec) / electrode (eeg); a tensor of the
                 input's shape.
    class_idx:   None = each sample's arg-max class on the unperturbed input; an int; one class per sample (sequence / tensor [B]);
                 'all' = every class, the map gains a class axis [B,K,Hm,Wm] (K <= 32).
    score:       'prob': the softmax probability; 'logprob': the log-probability.
    max_batch:   rows (coalitions) per forward pass; no bit of the result depends on it.
    (N + 2) * B forward evaluations in eval mode without autograd.  The rows are written straight in the model's layout
    (bx_shap_perturb_*: a selection, every element is bit for bit the input's or the baseline's); the fit is fp64 with every sum in a
    fixed order (bx_shap_fit: one Gram matrix and one Cholesky factorisation per call, shared by all samples and classes); the map is
    the values gathered through the label map (bx_shap_value_map).  In a MultimodalModel the branch whose input does not change runs
    once per sample and its output is repeated into the fusion head.  ValueError when the coalitions leave the values undetermined.
    The training flag and every requires_grad are restored on return.  Returns the map (device, fp32), or ``KernelShapResult`` with
    return_parts."""
    return _kernel_shap(model, eeg, spec, input, segments, num_samples, baseline, class_idx, score, seed, coalitions, max_batch, return_parts)


def _kernel_shap(model, eeg, spec, input, segments, num_samples, baseline, class_idx, score, seed, coalitions, max_batch, return_parts, profile=None):
    """``kernel_shap`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'perturb', 'forward',
    'fit' -- device events around every phase of the pass (tools/kernel_shap_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "kernel_shap"
    call = _Call(who, model).named(input)
    if score not in _FAITH_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = call.B
    Hd, Wd = int(x.shape[2]), int(x.shape[3])
    per_len, what = _per_cell(who, x, call.input_is_spec)
    if B < 1 or not 1 <= Hd * Wd <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hd * Wd} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    seg, M = _shap_segments(who, segments, input, Hd, Wd)
    Hm, Wm = seg.shape
    map_rows = None if call.input_is_spec else Hm
    K, cls_h, all_classes = call.explained(class_idx).K, call.cls_h, call.all_classes
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    Z, weights, exact = _shap_coalitions(who, M, 2 * M + 2048 if num_samples is None else num_samples, seed, coalitions)
    N = int(Z.shape[0])
    if B * N * K >= 1 << 31 or B * K * Hm * Wm >= 1 << 31 or N * M >= 1 << 31:
        raise ValueError(f"{who}: B * N * K = {B * N * K}, B * K * Hm * Wm = {B * K * Hm * Wm} or N * M = {N * M} beyond 32-bit offsets; "
                         "use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    dev = x.device
    use_logprob = score == "logprob"
    rp = _RowPass(call, kind, base, max_batch, profile)

    with rp.open():
        seg_d, Z_d, w_d = torch.from_numpy(seg).to(dev), torch.from_numpy(Z).to(dev), torch.from_numpy(weights).to(dev)
        none_d = torch.zeros(1, M, dtype=torch.uint8, device=dev)      # the empty coalition: the baseline itself
        clean, empty = (torch.empty(B, K, dtype=torch.float32, device=dev) for _ in range(2))
        if call.multimodal:
            with rp.lap("forward"):
                rp.fix_other()
        # v(1) and v(0): the unperturbed input and the baseline take the path of the coalition rows, in chunks of the same size
        for b0, nb in rp.groups():
            with rp.lap("perturb"):
                rows0 = _shap_perturb(rp.xs, seg_d, none_d, M, rp.base, kind, b0, nb, 0, 1, rp.dt, map_rows)
            with rp.lap("forward"):
                clean[b0:b0 + nb] = rp.scores(rp.clean_rows(b0, nb), b0, nb, logprob=use_logprob)
                empty[b0:b0 + nb] = rp.scores(rows0, b0, nb, logprob=use_logprob)
        classes = _class_tensor(cls_h, all_classes, clean, dev)
        S = rp.sweep(N, lambda *chunk: _shap_perturb(rp.xs, seg_d, Z_d, M, rp.base, kind, *chunk, rp.dt, map_rows), logprob=use_logprob)
        with rp.lap("fit"):
            phi = _shap_fit(S, clean, empty, classes, Z_d, w_d)
            R = phi.shape[1]
            attr = torch.empty((B, K, Hm, Wm) if all_classes else (B, Hm, Wm), dtype=torch.float32, device=dev)
            L.check(lib.bx_shap_value_map(_p(phi), _p(seg_d), _p(attr), B, R, Hm, Wm, M, _stream()), "bx_shap_value_map")
    if not return_parts:
        return attr
    return KernelShapResult(attr, phi if all_classes else phi[:, 0], None if classes is None else classes.long(), S, clean, empty, Z, weights, seg, exact)


# ------------------------------------------------------------------------------------------------
# Score-CAM (Wang et al., CVPR-W 2020): a class-activation map whose channel weights come from forward passes of the input seen
# through each up-sampled activation channel.  The definition is pinned in include/brainxai.h; tests/scorecam_ref.py restates it.
_SCORECAM_WEIGHTS = {"prob": L.BX_SCORECAM_PROB, "increase": L.BX_SCORECAM_INCREASE}

ScoreCamResult = collections.namedtuple("ScoreCamResult", "cam raw weights A out probs lo hi valid classes")
ScoreCamResult.__doc__ = """What ``score_cam(..., return_parts=True)`` returns, all on the device: ``cam`` (what the plain call returns), ``raw`` fp32
[B(,K),h,w] before ReLU and up-sampling, ``weights`` fp32 [B(,K),C] = w_k, ``A`` the target's activation (NHWC [B,h,w,C] in the model's
storage dtype for a spectrogram target, fp32 [B,C,1,T'] for an EEG target), ``out`` the log-probabilities of the clean input [B,K],
``probs`` fp32 [B,C,K] (the class probabilities of the input seen through every channel), ``lo`` / ``hi`` fp32 [B,C] (the extremes of
every up-sampled channel), ``valid`` bool [B,C] (hi > lo) and ``classes`` int64 [B] (None for class_idx='all')."""


def _scorecam_plane(A, eeg_target):
    """-> (dtype code, sb, sc, sy, sx, C, h, w): how the library addresses channel k of sample b of A (NHWC [B,h,w,C], or [B,C,1,T'])."""
    if eeg_target:
        B, Cc, _, w = A.shape
        return ops.bx_dtype(A.dtype), Cc * w, w, 0, 1, Cc, 1, w
    B, h, w, Cc = A.shape
    return ops.bx_dtype(A.dtype), h * w * Cc, 1, w * Cc, Cc, Cc, h, w


def _scorecam_range(A, eeg_target, Hm, Wm):
    """lo, hi, scale fp32 [B,C]: the extremes of every channel of A up-sampled to Hm x Wm, and 1 / (hi - lo) or 0 (bx_scorecam_range)."""
    lib = L.load()
    pl = _scorecam_plane(A, eeg_target)
    B, Cc = A.shape[0], pl[5]
    lo, hi, scale = (torch.empty(B, Cc, dtype=torch.float32, device=A.device) for _ in range(3))
    nbytes = lib.bx_scorecam_range_workspace(B, Cc, Hm, Wm)
    if nbytes == 0:
        L.check(-1, "bx_scorecam_range_workspace")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=A.device)
    L.check(lib.bx_scorecam_range(_p(A), *pl[:5], B, *pl[5:], Hm, Wm, _p(lo), _p(hi), _p(scale), _p(ws), nbytes, _stream()), "bx_scorecam_range")
    return lo, hi, scale


def _scorecam_perturb(x, A, eeg_target, lo, scale, base, kind, b0, nb, k0, n, dt):
    """Rows (b, k), b in b0..b0+nb-1, k in k0..k0+n-1: sample b seen through channel k of A.  x fp32 [B,Cin,H,W] -> internal layout
    [nb*n,H,W,8] in dt (bx_scorecam_perturb_spec), or for an EEG target fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T] (bx_scorecam_perturb_eeg)."""
    lib = L.load()
    pl = _scorecam_plane(A, eeg_target)
    B = x.shape[0]
    out, dims = _empty_rows(x, nb * n, dt, eeg_target)               # no slices: the library takes the whole x and base, and b0
    if not eeg_target:
        L.check(lib.bx_scorecam_perturb_spec(_p(x), _p(A), *pl, _p(lo), _p(scale), _p(base), kind, _p(out), B, *dims, b0, nb, k0, n, ops.bx_dtype(dt),
                                             _stream()), "bx_scorecam_perturb_spec")
    else:
        L.check(lib.bx_scorecam_perturb_eeg(_p(x), _p(A), pl[0], pl[1], pl[2], pl[4], pl[5], pl[7], _p(lo), _p(scale), _p(base), kind, _p(out), B, *dims,
                                            b0, nb, k0, n, _stream()), "bx_scorecam_perturb_eeg")
    return out


def score_cam(model, eeg, spec, target_layer="spectrogram_model.block5", *, class_idx=None, weights="prob", baseline=0.0, upsample=True, relu=True,
              max_batch=256, return_parts=False):
    """Score-CAM (Wang et al., CVPR-W 2020): a class-activation map at ``target_layer`` whose channel weights come from forward passes
    instead of gradients.  With A[k] channel k of the target's activation (a plane h x w), x the input the target's branch reads,
    base the baseline and c the class:

        U_k  = bilinear up-sampling (align_corners=False) of A[k] to the input's map domain;  lo_k, hi_k = its extremes
        M_k  = min((U_k - lo_k) / (hi_k - lo_k), 1) in [0, 1]   (a channel with hi_k = lo_k is invalid: its weight is 0)
        P[k] = softmax probabilities of the model for base + M_k (x - base)
        w_k  = P[k, c] (weights='prob', the authors' published code)  or  P[k, c] - P_base[c] (weights='increase', the paper's
               increase of confidence; P_base = the probabilities of the all-baseline input)
        raw  = sum_k w_k A[k] at the activation's own resolution;  cam = ReLU(raw) if relu, then the optional up-sampling

    These are the conventions of ``grad_cam``: the sum runs over A itself, the map is up-sampled afterwards (``resize_bilinear``) and
    there is no final normalisation.  The authors' script instead sums the UP-SAMPLED planes and min-max normalises the result; for a
    linear up-sampling the two sums agree, the normalisation is left to the caller.  pytorch-grad-cam's softmax over the channels of
    w is not applied either.

    target_layer: 'spectrogram_model.blockN' or 'spectrogram_model.blockN.convK' (the strings and the activation of ``grad_cam``): the
                  masks cover the spectrogram [H,W], one value for all channels of a pixel (C <= 4), map [B,h,w] or, up-sampled,
                  [B,H,W].  'eeg_model.depthwiseConv' / 'eeg_model.separableConv': the masks cover time columns of the EEG input, one
                  value for every electrode, map [B,1,T] (separableConv: [B,1,T//4], resized to [B,1,T] by ``upsample``); the tuned
                  EEGNet family only, as in ``grad_cam``.  'eeg_model.conv1' is refused: its activation is never formed.
    model:        a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None); a stand-alone EEGNet / EEGNetAttentionDeep
                  (spec=None, 'depthwiseConv' / 'separableConv') -- the convention of grad_cam and rise.
    class_idx:    None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]);
                  'all' = every class, the map gains a class axis [B,K,...] (K <= 32) at no further forward pass.
    baseline:     what a masked-out cell shows: a number; one value per channel (spectrogram) / electrode (EEG); a tensor of the
                  input's shape.
    max_batch:    rows (masked inputs) per forward pass.
    C * B forward evaluations (plus B for weights='increase') in eval mode without autograd, no backward pass.  The B x C masks never
    exist in memory: the rows are written straight in the model's layout from the activation planes (bx_scorecam_perturb_*), and the
    sum runs in fp64 in channel order (bx_scorecam_combine): identical bits run to run and for every max_batch.  In a MultimodalModel
    the branch whose input does not change runs once per sample and its output is repeated into the fusion head.  The training flag
    and every requires_grad are restored on return.  The map fits ``deletion_insertion`` and ``attribution_ranks`` as it is.
    Returns the map (device, fp32), or ``ScoreCamResult`` with return_parts."""
    return _score_cam(model, eeg, spec, target_layer, class_idx, weights, baseline, upsample, relu, max_batch, return_parts)


def _score_cam(model, eeg, spec, target_layer, class_idx, weights, baseline, upsample, relu, max_batch, return_parts, profile=None):
    """``score_cam`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'range', 'perturb',
    'forward', 'combine' -- device events around every phase of the pass (tools/scorecam_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "score_cam"
    if weights not in _SCORECAM_WEIGHTS:
        raise ValueError(f"{who}: unknown weights {weights!r}; use 'prob' or 'increase'")
    max_batch = _max_batch(who, max_batch)
    if not isinstance(target_layer, str):
        raise ValueError(f"{who}: target_layer must be a string, got {target_layer!r}")
    me, ms = _EEG_TARGET.match(target_layer), _TARGET.match(target_layer)
    if me:
        if me.group(1) == "conv1":
            raise ValueError(f"{who}: 'eeg_model.conv1' is no Score-CAM target: its [B,8,Chans,T] activation is never formed; use "
                             "'eeg_model.depthwiseConv' or 'eeg_model.separableConv'")
        eeg_target, x = True, eeg
    elif ms:
        eeg_target, x = False, spec
    else:
        raise ValueError(f"{who}: unsupported target {target_layer!r}; use 'spectrogram_model.blockN[.convK]', 'eeg_model.depthwiseConv' or "
                         "'eeg_model.separableConv'")
    if x is None:
        raise ValueError(f"{who}: target {target_layer!r} reads the {'EEG' if eeg_target else 'spectrogram'} input, but that tensor is None")
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or (eeg_target and x.shape[1] != 1):
        raise ValueError(f"{who}: the {'EEG' if eeg_target else 'spectrogram'} input must be a tensor " + ("[B,1,Chans,T]" if eeg_target else "[B,C,H,W]"))
    call = _Call(who, model, "eeg" if eeg_target else "spec").given(x, spec if eeg_target else eeg).target()
    B, K, net, multimodal = call.B, call.K, call.net, call.multimodal
    if eeg_target:
        from .models import EEGNet, EEGNetAttentionDeep
        if not isinstance(net, (EEGNet, EEGNetAttentionDeep)):
            raise ValueError(f"{who}: an EEG target needs an EEGNet / EEGNetAttentionDeep branch, got {type(net).__name__}")
        Chans, T = int(x.shape[2]), int(x.shape[3])
        g = net._geom
        if not (g.F1 == 8 and g.D == 2 and g.F2 == 16 and g.K2 == 16 and g.K1 <= 64 and 1 <= Chans <= 64 and g.P1 <= T <= 15000):
            raise ValueError(f"{who}: EEG targets support the tuned EEGNet family only: F1=8, D=2, F2=16, K2=16, kernLength <= 64, Chans <= 64, "
                             f"T <= 15000 (got F1={g.F1}, D={g.D}, F2={g.F2}, kernLength={g.K1}, Chans={Chans}, T={T})")
        Hm, Wm = 1, T
    else:
        Hm, Wm = int(x.shape[2]), int(x.shape[3])
    per_len, what = _per_cell(who, x, not eeg_target)
    if B < 1 or not 1 <= Hm * Wm <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hm * Wm} cells per sample (B = {B}), supported 1..{_FAITH_MAX_N}")
    cls_h, all_classes = call.classes(class_idx).cls_h, call.all_classes
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    call.need_gpu("the model and its inputs")

    lib = L.load()
    dev = x.device
    nm = call.Kc
    rp = _RowPass(call, kind, base, max_batch, profile)

    with rp.open():
        xs = rp.xs
        with rp.lap("forward"):
            # the clean pass: the activation, the explained class, and the branch whose input does not change (once per sample)
            rp.fix_other()
            if eeg_target:
                feat, saved, desc, _, _ = ops.eeg_features_keep(net, xs)
                A = _eeg_target_plane(saved, desc, g, B, T, me.group(1))
                clean = _eeg_head(net, feat)
            else:
                with _SpecTarget(getattr(net, f"block{ms.group(1)}"), int(ms.group(2) or 0)) as tgt:
                    clean = net(xs)
                    A = tgt.act()
            out = _fuse(model, multimodal, not eeg_target, clean, rp.fixed).float().contiguous()
        pl = _scorecam_plane(A, eeg_target)
        Cn, h, w = pl[5], pl[6], pl[7]
        classes = _class_tensor(cls_h, all_classes, out, dev)
        with rp.lap("range"):
            lo, hi, scale = _scorecam_range(A, eeg_target, Hm, Wm)
            valid = hi > lo
        P_base = None
        if weights == "increase":
            # the all-baseline input: the row of a channel whose scale is 0.  Not a sweep(1, ...): the store into its [B,1,K] would be
            # a launch that the concatenation of one sample group (the usual case) does not have
            zero = torch.zeros(B, Cn, dtype=torch.float32, device=dev)
            for b0, nb in rp.groups():
                with rp.lap("perturb"):
                    rows = _scorecam_perturb(xs, A, eeg_target, zero, zero, rp.base, kind, b0, nb, 0, 1, rp.dt)
                with rp.lap("forward"):
                    pb = rp.scores(rows, b0, nb)
                    P_base = pb if P_base is None else torch.cat([P_base, pb])
            P_base = P_base.contiguous()
        P = rp.sweep(Cn, lambda *chunk: _scorecam_perturb(xs, A, eeg_target, lo, scale, rp.base, kind, *chunk, rp.dt))
        with rp.lap("combine"):
            raw = torch.empty(B * nm, h, w, dtype=torch.float32, device=dev)
            cam = torch.empty_like(raw) if relu else None
            wts = torch.empty(B * nm, Cn, dtype=torch.float32, device=dev)
            L.check(lib.bx_scorecam_combine(_p(P), _p(P_base), _p(classes), _p(valid), _p(A), *pl[:5], B, Cn, h, w, K, _SCORECAM_WEIGHTS[weights],
                                            1 if relu else 0, _p(raw), _p(cam), _p(wts), _stream()), "bx_scorecam_combine")
            if cam is None:
                cam = raw
            if upsample and (h, w) != (Hm, Wm):
                cam = resize_bilinear(cam, (Hm, Wm))
    if eeg_target:
        cam, raw = cam.reshape(B * nm, 1, -1), raw.reshape(B * nm, 1, -1)
    cam, raw, wts = _class_axis(B, nm, all_classes, cam, raw, wts)
    if not return_parts:
        return cam
    return ScoreCamResult(cam, raw, wts, A, out, P, lo, hi, valid, None if classes is None else classes.long())


# ------------------------------------------------------------------------------------------------
# Expected gradients, batched (SHAP's GradientExplainer; the one attribution the reference computes from SHAP).  The definition is
# pinned in include/brainxai.h; tests/gradient_shap_ref.py restates it.
GradientShapResult = collections.namedtuple("GradientShapResult", "attribution values classes out idx alpha nsamples")
GradientShapResult.__doc__ = """What ``gradient_shap(..., return_parts=True)`` returns: ``attribution`` fp32 [B,H,W] / [B,Chans,T], with a class axis for
class_idx='all' (what the plain call returns), ``values`` fp32 [B(,K),*x.shape[1:]] (the estimator element by element), ``classes`` int64
[B] (None for class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), all on the device; ``idx`` int32 [B,n] and
``alpha`` fp32 [B,n] on the host: ``draws=(idx, alpha)`` repeats the call; ``nsamples`` = n."""


def _gradshap_draws(who, B, Nb, n, seed, draws):
    """-> (idx int32 [B,n], alpha fp32 [B,n]) on the host.  From one np.random.default_rng(seed), sample by sample: the background indices
    of a sample, then its interpolation points -- the draws of ``expected_gradients``; or ``draws`` checked."""
    if draws is None:
        rng = np.random.default_rng(seed)
        idx, alpha = np.empty((B, n), dtype=np.int32), np.empty((B, n), dtype=np.float32)
        for b in range(B):
            idx[b] = rng.integers(0, Nb, size=n)
            alpha[b] = rng.random(n).astype(np.float32)
        return idx, alpha
    if not isinstance(draws, (tuple, list)) or len(draws) != 2:
        raise ValueError(f"{who}: draws must be (idx [B,n] integer, alpha [B,n] float)")
    idx, alpha = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in draws)
    if idx.dtype.kind not in "iu" or alpha.dtype.kind != "f":
        raise ValueError(f"{who}: draws must be (idx [B,n] integer, alpha [B,n] float), got dtypes {idx.dtype}, {alpha.dtype}")
    if idx.shape != (B, n) or alpha.shape != (B, n):
        raise ValueError(f"{who}: draws of shapes {idx.shape}, {alpha.shape}; expected [B,n] = {(B, n)} twice")
    if idx.min() < 0 or idx.max() >= Nb:
        raise ValueError(f"{who}: draws index outside [0, Nb = {Nb})")
    if not np.isfinite(alpha).all():
        raise ValueError(f"{who}: draws alpha is not finite")
    return np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(alpha.astype(np.float32))


def gradient_shap(model, eeg, spec, background, *, input="eeg", nsamples=200, class_idx=None, seed=0, draws=None, max_batch=256, return_parts=False):
    """Expected gradients (SHAP's GradientExplainer; the reference's ``shap.GradientExplainer(eeg_model, background).shap_values(x)``), for
    either input of the multimodal model or a stand-alone branch, batched over samples, draws and classes:
        phi[b,c] = (1/n) sum_k d[b,k] * dF_c/dx(r[b,k]),   d[b,k] = x[b] - bg[idx[b,k]],   r[b,k] = bg[idx[b,k]] + alpha[b,k] * d[b,k]
    with F_c the model's output log-probability of class c.  The map has the input's own shape and fits ``deletion_insertion`` and
    ``attribution_ranks`` as it is.

    input:       'eeg': x = eeg [B,1,Chans,T], map [B,Chans,T]; 'spec': x = spec [B,C,H,W], map [B,H,W] = the values summed over the
                 channels (a sum keeps the attributions additive).
    model:       a MultimodalModel (the other input stays the sample's own); a stand-alone Spectrogram_Model (eeg=None, input='spec');
                 a stand-alone EEGNet / EEGNetAttentionDeep (spec=None, input='eeg').
    background:  [Nb, *x.shape[1:]], the set the baselines are drawn from.
    nsamples:    n, the draws per sample.  One np.random.default_rng(seed) gives, sample by sample, idx = rng.integers(0, Nb, n) and then
                 alpha = rng.random(n).astype(float32): the draws of ``expected_gradients`` for the same seed.
    draws:       (idx [B,n] integer, alpha [B,n] float) replaces them.
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,...] (K <= 32): one forward pass then serves K backward passes.
    max_batch:   rows (interpolants) per pass, capped so that a pass addresses its largest activation with 32-bit offsets.  The sum over
                 the draws is carried in fp64 between passes, so, given the same gradients, no bit of the result depends on it.
    The rows of a pass are written by one launch (bx_expgrad_rows), the one-hot gradient seeds by one (bx_expgrad_seed); every backward
    pass is followed by one bx_expgrad_accumulate (fp64, ascending draw order, no atomics), and bx_expgrad_finish divides by n and sums
    the channels.  In a MultimodalModel the branch whose input does not change runs once per sample and its output is gathered into the
    fusion head.  The training flag and every requires_grad are restored on return.  Returns the map (device, fp32), or
    ``GradientShapResult`` with return_parts."""
    return _gradient_shap(model, eeg, spec, background, input, nsamples, class_idx, seed, draws, max_batch, return_parts)


def _gradient_shap(model, eeg, spec, background, input, nsamples, class_idx, seed, draws, max_batch, return_parts, profile=None):
    """``gradient_shap`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'rows', 'forward',
    'backward', 'accumulate', 'finish' -- device events around every phase of the pass (tools/gradient_shap_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "gradient_shap"
    call = _Call(who, model).named(input)
    n, max_batch = _draw_count(who, nsamples), _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = _nonempty(who, x)
    if not isinstance(background, torch.Tensor) or background.dim() != 4 or tuple(background.shape[1:]) != tuple(x.shape[1:]):
        got = tuple(background.shape) if isinstance(background, torch.Tensor) else type(background).__name__
        raise ValueError(f"{who}: background of shape {got}; expected [Nb, {', '.join(str(int(v)) for v in x.shape[1:])}] like the {input} input")
    Nb = int(background.shape[0])
    if Nb < 1:
        raise ValueError(f"{who}: empty background (Nb = 0)")
    Kc, per = call.explained(class_idx).Kc, call.per
    if B * n >= 1 << 31 or B * Kc * per >= 1 << 31 or Nb * per >= 1 << 31:
        raise ValueError(f"{who}: B * n = {B * n}, B * Kc * per = {B * Kc * per} or Nb * per = {Nb * per} beyond 32-bit offsets; use fewer samples per call")
    idx, alpha = _gradshap_draws(who, B, Nb, n, seed, draws)
    call.need_gpu("the model, its inputs and the background", background)

    lib = L.load()
    gp = _GradPass(call, n, max_batch, profile)

    with gp.open():
        xs = gp.xs
        bgs = background.detach().to(gp.dev, torch.float32).contiguous()
        idx_d, alpha_d = torch.from_numpy(idx).to(gp.dev), torch.from_numpy(alpha).to(gp.dev)
        gp.clean()
        acc, = gp.sums(1)

        def write(row0, rows):
            r = torch.empty(rows, *xs.shape[1:], dtype=torch.float32, device=gp.dev)
            L.check(lib.bx_expgrad_rows(_p(xs), _p(bgs), _p(idx_d), _p(alpha_d), _p(r), B, Nb, n, per, row0, rows, _stream()), "bx_expgrad_rows")
            return r

        gp.sweep(write, lambda g, slot, row0, rows: L.check(lib.bx_expgrad_accumulate(
            _p(xs), _p(bgs), _p(idx_d), _p(g), _p(acc), B, Nb, n, per, Kc, slot, row0, rows, _stream()), "bx_expgrad_accumulate"))
        with gp.lap("finish"):
            values, amap = gp.finish_values(acc, n)
    return gp.result(return_parts, GradientShapResult, amap, values, idx, alpha, n)


def channel_importance(values, top=None):
    """The reference's reduction of its SHAP values (XAI_Multimodality.py: mean |.| over time per electrode, then the top-n electrodes):
    mean |values| over the last axis of [..., L] -> fp32 [...], one launch (bx_mean_abs_rows: fp64 sum in a fixed order, one rounding).
    With ``top=n`` returns (importance, indices): int64 [..., n], the n largest along the new last axis in descending order, ties by
    the lower index.  On ``GradientShapResult.values`` [B,K,1,Chans,T] that is the reference's electrode ranking."""
    who = "channel_importance"
    if not isinstance(values, torch.Tensor) or values.dim() < 1 or values.numel() == 0:
        raise ValueError(f"{who}: values must be a non-empty tensor [..., L]")
    lead = tuple(int(v) for v in values.shape[:-1])
    Ln = int(values.shape[-1])
    R = values.numel() // Ln
    if top is not None:
        if isinstance(top, bool) or not isinstance(top, numbers.Integral):
            raise ValueError(f"{who}: top must be None or an int, got {top!r}")
        if not lead:
            raise ValueError(f"{who}: top needs values with at least two axes [..., channels, L]")
        if not 1 <= int(top) <= lead[-1]:
            raise ValueError(f"{who}: top = {int(top)} outside 1..{lead[-1]}")
    if R * Ln >= 1 << 31:
        raise ValueError(f"{who}: {R * Ln} values beyond 32-bit offsets")
    if not values.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the values must live on the GPU; there is no CPU path")
    v = values.detach().to(torch.float32).contiguous()
    imp = torch.empty(lead, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        L.check(L.load().bx_mean_abs_rows(_p(v), _p(imp), R, Ln, _stream()), "bx_mean_abs_rows")
    if top is None:
        return imp
    order = torch.sort(imp, dim=-1, descending=True, stable=True).indices
    return imp, order[..., :int(top)].contiguous()


class GradientExplainer:
    """SHAP's calling form over ``gradient_shap``: ``GradientExplainer(model, background).shap_values(x)`` returns a list of K numpy
    arrays shaped like x, one per class -- the reference's two lines (XAI_Multimodality.py:2283-2290) run unchanged apart from the
    import.  ``input`` names the input x is ('eeg' or 'spec'); a MultimodalModel also takes the other input as ``other``."""

    def __init__(self, model, background, input="eeg"):
        if input not in _FAITH_INPUTS:
            raise ValueError(f"GradientExplainer: unknown input {input!r}; use 'spec' or 'eeg'")
        self.model, self.background, self.input = model, background, input

    def shap_values(self, x, other=None, nsamples=200, seed=0):
        eeg, spec = (x, other) if self.input == "eeg" else (other, x)
        res = gradient_shap(self.model, eeg, spec, self.background, input=self.input, nsamples=nsamples, class_idx="all", seed=seed, return_parts=True)
        vals = res.values.cpu().numpy()
        return [vals[:, c] for c in range(vals.shape[1])]


# ------------------------------------------------------------------------------------------------
# SmoothGrad, SmoothGrad^2 and VarGrad (Captum's NoiseTunnel over saliency; the reference imports Captum).  The definition is pinned in
# include/brainxai.h; tests/smooth_grad_ref.py restates it.
SmoothGradResult = collections.namedtuple("SmoothGradResult", "attribution values classes out sigma nsamples kind seed")
SmoothGradResult.__doc__ = """What ``smooth_grad(..., return_parts=True)`` returns: ``attribution`` fp32 [B,H,W] / [B,Chans,T], with a class axis for
class_idx='all' (what the plain call returns), ``values`` fp32 [B(,K),*x.shape[1:]] (the estimator element by element), ``classes`` int64
[B] (None for class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), ``sigma`` fp32 [B] (the noise scale of
every sample), all on the device; ``nsamples``, ``kind`` and ``seed`` as given: ``stdev=sigma`` with them repeats the call."""

_SMOOTHGRAD_KINDS = {"smoothgrad": 0, "smoothgrad_sq": 1, "vargrad": 2}          # BX_SMOOTHGRAD_MEAN / _SQ / _VAR


def smooth_grad_noise(shape, *, nsamples, seed=0, device=None):
    """The standard normal draws of ``smooth_grad`` themselves, fp32 [B, n, *shape[1:]] on the device, for an explained input of
    ``shape`` = [B, ...] -- for tests, plots and callers who want them; ``smooth_grad`` never stores them.  Written by the kernel that
    writes the noisy rows (bx_smoothgrad_rows without an input), so row[b,k] = x[b] + sigma[b] * z[b,k] holds bit for bit.  The draws
    of (b, k) depend on seed alone: a longer run extends a shorter one."""
    who = "smooth_grad_noise"
    try:
        shape = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: shape must be a sequence of ints [B, ...], got {shape!r}") from None
    if len(shape) < 2 or min(shape) < 1:
        raise ValueError(f"{who}: shape {shape}; expected [B, ...] with at least two axes, all >= 1")
    n, seed = _draw_count(who, nsamples), _stream_seed(who, seed)
    B, per = shape[0], int(np.prod(shape[1:]))
    if B * n >= 1 << 31 or B * per >= 1 << 31:
        raise ValueError(f"{who}: B * n = {B * n} or B * per = {B * per} beyond 32-bit offsets")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"brainxai.{who}: the noise is drawn on the GPU; there is no CPU path")
    lib = L.load()
    with torch.cuda.device(dev):
        z = torch.empty(B * n, *shape[1:], dtype=torch.float32, device=dev)
        for row0, rows in _sample_chunks(B * n, max(1, ((1 << 31) - 1) // per)):
            L.check(lib.bx_smoothgrad_rows(None, None, _p(z[row0:row0 + rows]), B, n, per, seed, row0, rows, _stream()), "bx_smoothgrad_rows")
    return z.reshape(B, n, *shape[1:])


def smooth_grad(model, eeg, spec, *, input="spec", nsamples=50, noise_level=None, stdev=None, kind="smoothgrad", class_idx=None, seed=0, max_batch=256,
                return_parts=False):
    """SmoothGrad (Smilkov et al. 2017), SmoothGrad^2 and VarGrad (Hooker et al. 2019; Adebayo et al. 2018) -- Captum's NoiseTunnel over
    the input gradient -- for either input of the multimodal model or a stand-alone branch, batched over samples, draws and classes:
        g[b,k] = dF_c/dx( x[b] + sigma[b] * z[b,k] ),   z standard normal,   F_c the model's output log-probability of class c
        kind='smoothgrad': mean_k g;   'smoothgrad_sq': mean_k g^2;   'vargrad': the population variance of g over the draws.
    The map is the largest |value| over the input's channels (``saliency``'s convention) and fits ``deletion_insertion`` and
    ``attribution_ranks`` as it is.

    input:       'spec': x = spec [B,C,H,W], map [B,H,W]; 'eeg': x = eeg [B,1,Chans,T], map [B,Chans,T].
    model:       a MultimodalModel (the other input stays the sample's own); a stand-alone Spectrogram_Model (eeg=None, input='spec');
                 a stand-alone EEGNet / EEGNetAttentionDeep (spec=None, input='eeg').
    noise_level: the paper's noise level: sigma[b] = noise_level * (max x[b] - min x[b]) (bx_smoothgrad_sigma); 0.15 when neither
                 noise_level nor stdev is given.
    stdev:       the absolute standard deviation instead: a number, or one per sample (tensor [B]).  Giving both is refused.
    nsamples:    n, the draws per sample.  The noise is drawn on the device from Philox4x32-10 counters (element, draw, sample) keyed by
                 ``seed`` (0 <= seed < 2^64) and never stored; the draws of a sample depend neither on nsamples (a longer run extends a
                 shorter one) nor on max_batch.  ``smooth_grad_noise`` returns them.
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,...] (K <= 32): one forward pass then serves K backward passes.
    max_batch:   rows (noisy inputs) per pass, capped so that a pass addresses its largest activation with 32-bit offsets.  The sums
                 over the draws are carried in fp64 between passes, so, given the same gradients, no bit of the result depends on it.
    The rows of a pass are written by one launch (bx_smoothgrad_rows), the one-hot gradient seeds by one (bx_expgrad_seed); every backward
    pass is followed by one bx_smoothgrad_accumulate (fp64 sums of g and g^2, ascending draw order, no atomics), and bx_smoothgrad_finish
    forms the values and the map.  In a MultimodalModel the branch whose input does not change runs once per sample and its output is
    gathered into the fusion head.  The training flag and every requires_grad are restored on return.  Returns the map (device, fp32),
    or ``SmoothGradResult`` with return_parts."""
    return _smooth_grad(model, eeg, spec, input, nsamples, noise_level, stdev, kind, class_idx, seed, max_batch, return_parts)


def _smooth_grad(model, eeg, spec, input, nsamples, noise_level, stdev, kind, class_idx, seed, max_batch, return_parts, profile=None):
    """``smooth_grad`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'sigma', 'rows',
    'forward', 'backward', 'accumulate', 'finish' -- device events around every phase of the pass (tools/smooth_grad_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "smooth_grad"
    call = _Call(who, model).named(input)
    if not isinstance(kind, str) or kind not in _SMOOTHGRAD_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r}; use 'smoothgrad', 'smoothgrad_sq' or 'vargrad'")
    n, seed, max_batch = _draw_count(who, nsamples), _stream_seed(who, seed), _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = _nonempty(who, x)
    level, sd = _level_or_absolute(who, B, "noise_level", noise_level, "stdev", stdev, 0.15, True)
    Kc, per = call.explained(class_idx).Kc, call.per
    if B * n >= 1 << 31 or B * Kc * per >= 1 << 31 or B * Kc > 65535:
        raise ValueError(f"{who}: B * n = {B * n} or B * Kc * per = {B * Kc * per} beyond 32-bit offsets, or B * Kc = {B * Kc} > 65535; use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    gp = _GradPass(call, n, max_batch, profile)

    with gp.open():
        xs = gp.xs
        with gp.lap("sigma"):
            sigma = _range_scale(xs, level, sd)
        gp.clean()
        S1, S2 = gp.sums(2)

        def write(row0, rows):
            r = torch.empty(rows, *xs.shape[1:], dtype=torch.float32, device=gp.dev)
            L.check(lib.bx_smoothgrad_rows(_p(xs), _p(sigma), _p(r), B, n, per, seed, row0, rows, _stream()), "bx_smoothgrad_rows")
            return r

        gp.sweep(write, lambda g, slot, row0, rows: L.check(lib.bx_smoothgrad_accumulate(
            _p(g), _p(S1), _p(S2), B, n, per, Kc, slot, row0, rows, _stream()), "bx_smoothgrad_accumulate"))
        with gp.lap("finish"):
            values, amap = gp.empty(*xs.shape[1:]), gp.empty(*xs.shape[2:])
            L.check(lib.bx_smoothgrad_finish(_p(S1), _p(S2), _p(values), _p(amap), B * Kc, gp.Cc, gp.HW, n, _SMOOTHGRAD_KINDS[kind], _stream()),
                    "bx_smoothgrad_finish")
    return gp.result(return_parts, SmoothGradResult, amap, values, sigma, n, kind, seed)


# ------------------------------------------------------------------------------------------------
# Blur Integrated Gradients (Xu, Venugopalan, Sundararajan, CVPR 2020; PAIR's saliency.BlurIG) and the Gaussian blur behind it.  The
# definition is pinned in include/brainxai.h; tests/blur_ig_ref.py restates it.
BlurIGResult = collections.namedtuple("BlurIGResult", "map values classes out endpoint delta sigmas steps max_sigma sqrt grad_step axes")
BlurIGResult.__doc__ = """What ``blur_ig(..., return_parts=True)`` returns: ``map`` fp32 [B,H,W] / [B,Chans,T], with a class axis for class_idx='all'
(what the plain call returns), ``values`` fp32 [B(,K),*x.shape[1:]] (the attribution element by element), ``classes`` int64 [B] (None
for class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), ``endpoint`` fp32 [B,K] (those of the input blurred
with the last sigma), ``delta`` fp64 [B] or [B,K] (sum of the values - (F_c(x) - endpoint_c): the completeness error of the left
Riemann sum), all on the device; ``sigmas`` the n + 1 Python floats of the schedule; the other fields as given."""

_BLUR_AXES = {"hw": L.BX_BLUR_AXES_HW, "h": L.BX_BLUR_AXES_H, "w": L.BX_BLUR_AXES_W}
_BLUR_LDS = 65536                                                                  # the row kernel's LDS budget (include/brainxai.h)


def blur_sigmas(steps, max_sigma, sqrt=False):
    """The n + 1 scales of the blur path in Python floats, exactly as saliency computes them: i * max_sigma / n, or its square root."""
    if sqrt:
        return [math.sqrt(float(i) * max_sigma / float(steps)) for i in range(0, steps + 1)]
    return [float(i) * max_sigma / float(steps) for i in range(0, steps + 1)]


def _blur_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)                                           # scipy.ndimage.gaussian_filter1d, truncate = 4


def gaussian_taps(sigma):
    """fp64 [2 R + 1]: the taps of scipy.ndimage.gaussian_filter1d(sigma, truncate=4), R = int(4 sigma + 0.5); the identity for
    sigma = 0 (and wherever R = 0)."""
    R = _blur_radius(sigma)
    if R == 0:
        return np.ones(1, dtype=np.float64)
    t = np.arange(-R, R + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * t ** 2)
    return phi / phi.sum()


def blur_taps(sigmas, grad_step=None):
    """The tap table of bx_blur_rows for the scales ``sigmas``: (taps fp32 [E,3,TW], radius int32 [E,2]) on the host.  Per entry
    a = g_sigma, b = g_{sigma+eps} and d = (b - a) / eps, formed in fp64 with a zero-padded to b's radius and rounded to fp32 once, tap t at
    index TW // 2 + t; radius = (R_a, R_b).  grad_step None: a alone (b and d stay zero, R_b = R_a)."""
    E = len(sigmas)
    ab = []
    for s in sigmas:
        a = gaussian_taps(s)
        b = a if grad_step is None else gaussian_taps(float(s) + grad_step)
        ab.append((a, b))
    Rmax = max(len(b) // 2 for _, b in ab)
    TW = 2 * Rmax + 1
    taps, radius = np.zeros((E, 3, TW), dtype=np.float32), np.zeros((E, 2), dtype=np.int32)
    for e, (a, b) in enumerate(ab):
        Ra, Rb = len(a) // 2, len(b) // 2
        radius[e] = Ra, Rb
        a_pad = np.zeros(2 * Rb + 1, dtype=np.float64)
        a_pad[Rb - Ra:Rb + Ra + 1] = a
        taps[e, 0, Rmax - Rb:Rmax + Rb + 1] = a_pad
        if grad_step is not None:
            taps[e, 1, Rmax - Rb:Rmax + Rb + 1] = b
            taps[e, 2, Rmax - Rb:Rmax + Rb + 1] = (b - a_pad) / grad_step
    return taps, radius


def _blur_axes(who, axes, eeg_input):
    if axes is None:
        return "w" if eeg_input else "hw"
    if not isinstance(axes, str) or axes not in _BLUR_AXES:
        raise ValueError(f"{who}: unknown axes {axes!r}; use 'hw', 'h' or 'w'")
    if eeg_input and axes != "w":
        raise ValueError(f"{who}: axes {axes!r} for the EEG input; the electrode order carries no geometry, only 'w' (time) is filtered")
    return axes


def _blur_steps(who, steps, max_sigma, sqrt, grad_step):
    if isinstance(steps, bool) or not isinstance(steps, numbers.Integral):
        raise ValueError(f"{who}: steps must be an int, got {steps!r}")
    if int(steps) < 1:
        raise ValueError(f"{who}: steps = {int(steps)} < 1")
    for name, v in (("max_sigma", max_sigma), ("grad_step", grad_step)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v <= 0:
            raise ValueError(f"{who}: {name} must be a finite number > 0, got {v!r}")
    return int(steps), float(max_sigma), bool(sqrt), float(grad_step)


def _blur_fits(who, x, axes, Rmax, deriv):
    """Refuses what bx_blur_rows would: a radius beyond the kernel's, and two filtered axes whose 4-column strip does not fit its LDS."""
    if Rmax > L.BX_BLUR_MAX_RADIUS:
        raise ValueError(f"{who}: filter radius {Rmax} (4 sigma), supported up to {L.BX_BLUR_MAX_RADIUS}; use a smaller sigma")
    H, W = int(x.shape[2]), int(x.shape[3])
    RC = min(Rmax, {"hw": max(H, W), "h": H, "w": W}[axes] - 1)                    # only taps that can join two points of the image are staged
    TP = 4 * ((RC + 6) // 4) + 4
    if 16 * TP > _BLUR_LDS or (axes == "hw" and 4 * (6 * TP + (2 if deriv else 1) * 4 * ((H + 3) // 4) * 8) > _BLUR_LDS):
        raise ValueError(f"{who}: H x W = {H} x {W} with filter radius {Rmax}: the taps and a strip of the intermediates do not fit the kernel's "
                         f"{_BLUR_LDS} bytes of LDS")
    if int(x.shape[1]) > 65535:
        raise ValueError(f"{who}: {int(x.shape[1])} channels, supported 1..65535")


def _blur_rows(lib, xs, taps_d, rad_d, TW, out, deriv, n, axes, per_sample, row0, rows):
    B, Cc, H, W = (int(v) for v in xs.shape)
    L.check(lib.bx_blur_rows(_p(xs), _p(taps_d), _p(rad_d), _p(out), _p(deriv), B, n, Cc, H, W, _BLUR_AXES[axes], TW, per_sample, row0, rows, _stream()),
            "bx_blur_rows")


def _blur_input(who, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be a tensor [B,C,H,W] (an EEG input [B,1,Chans,T] with axes='w')")
    return _nonempty(who, x)


def blur_path(x, *, steps, max_sigma, sqrt=False, grad_step=0.01, axes=None):
    """The rows of ``blur_ig`` themselves: (rows fp32 [B,n,*x.shape[1:]], deriv fp32 [B,n,*x.shape[1:]], sigmas) -- X_i = x blurred with
    sigma_i and D_i = (blur_{sigma_i + grad_step}(x) - X_i) / grad_step for i = 0..n-1, written by the kernel that writes the rows of a
    pass (bx_blur_rows) -- for scale-space plots and tests; ``blur_ig`` never stores more than a pass of them.  x [B,C,H,W]; axes
    'hw' (default), 'h' or 'w' (an EEG input [B,1,Chans,T] is blurred along time with axes='w')."""
    who = "blur_path"
    B = _blur_input(who, x)
    axes = _blur_axes(who, axes, False)
    n, max_sigma, sqrt, eps = _blur_steps(who, steps, max_sigma, sqrt, grad_step)
    per = x.numel() // B
    if B * n >= 1 << 31 or B * per >= 1 << 31:
        raise ValueError(f"{who}: B * n = {B * n} or B * per = {B * per} beyond 32-bit offsets")
    sigmas = blur_sigmas(n, max_sigma, sqrt)
    taps, radius = blur_taps(sigmas[:n], eps)
    _blur_fits(who, x, axes, taps.shape[2] // 2, True)
    if not x.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the rows are written on the GPU; there is no CPU path")
    lib = L.load()
    with torch.cuda.device(x.device):
        xs = x.detach().to(torch.float32).contiguous()
        taps_d, rad_d = torch.from_numpy(taps).to(xs.device), torch.from_numpy(radius).to(xs.device)
        rows_out = torch.empty(B * n, *xs.shape[1:], dtype=torch.float32, device=xs.device)
        deriv = torch.empty_like(rows_out)
        for row0, rows in _sample_chunks(B * n, max(1, ((1 << 31) - 1) // per)):
            _blur_rows(lib, xs, taps_d, rad_d, taps.shape[2], rows_out[row0:row0 + rows], deriv[row0:row0 + rows], n, axes, 0, row0, rows)
    return rows_out.reshape(B, n, *xs.shape[1:]), deriv.reshape(B, n, *xs.shape[1:]), sigmas


def gaussian_blur(x, sigma, *, axes=None):
    """x [B,C,H,W] blurred with a Gaussian of standard deviation ``sigma`` (a number, or one per sample: a sequence or tensor [B]), fp32
    in the input's shape: scipy.ndimage.gaussian_filter's taps (truncate 4) and zero padding (mode='constant'), per channel, along
    ``axes`` = 'hw' (default), 'h' or 'w' (an EEG input [B,1,Chans,T] is blurred along time with axes='w').  sigma = 0 returns the
    input bit for bit.  The kernel of ``blur_ig``'s rows with one row per sample (bx_blur_rows).  The result passes as the tensor
    ``baseline=`` of deletion_insertion, rise, occlusion, kernel_shap and score_cam."""
    who = "gaussian_blur"
    B = _blur_input(who, x)
    axes = _blur_axes(who, axes, False)
    if isinstance(sigma, numbers.Real) and not isinstance(sigma, bool):
        sig = [float(sigma)]
    else:
        try:
            sig_a = sigma.detach().to("cpu", torch.float64).numpy() if isinstance(sigma, torch.Tensor) else np.asarray(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: sigma must be a number or one per sample [B], got {type(sigma).__name__}") from None
        if sig_a.shape != (B,):
            raise ValueError(f"{who}: sigma of shape {tuple(sig_a.shape)}; expected a number or [B] = [{B}]")
        sig = [float(v) for v in sig_a]
    if any(not math.isfinite(v) or v < 0 for v in sig):
        raise ValueError(f"{who}: sigma must be finite and >= 0")
    per = x.numel() // B
    if B * per >= 1 << 31:
        raise ValueError(f"{who}: B * per = {B * per} beyond 32-bit offsets")
    taps, radius = blur_taps(sig)
    _blur_fits(who, x, axes, taps.shape[2] // 2, False)
    if not x.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the blur runs on the GPU; there is no CPU path")
    lib = L.load()
    with torch.cuda.device(x.device):
        xs = x.detach().to(torch.float32).contiguous()
        out = torch.empty_like(xs)
        _blur_rows(lib, xs, torch.from_numpy(taps).to(xs.device), torch.from_numpy(radius).to(xs.device), taps.shape[2], out, None, 1, axes,
                   int(len(sig) > 1), 0, B)
    return out


def blur_ig(model, eeg, spec, *, input="spec", steps=50, max_sigma=50.0, sqrt=False, grad_step=0.01, axes=None, class_idx=None, max_batch=256,
            return_parts=False):
    """Blur Integrated Gradients (Xu, Venugopalan, Sundararajan, CVPR 2020; saliency.BlurIG): integrated gradients along the path through
    Gaussian scale space from the input to a heavily blurred copy of it -- no baseline -- for either input of the multimodal model or a
    stand-alone branch, batched over samples, steps and classes:
        values[b,c] = sum_{i<n} w_i * dF_c/dx( X_i ) * D_i,      X_i = blur_{sigma_i}(x[b]),   D_i = (blur_{sigma_i + grad_step}(x[b]) - X_i) / grad_step,
        sigma_i = i * max_sigma / n (sqrt: its square root),  w_i = -(sigma_{i+1} - sigma_i),  F_c the model's output log-probability of class c
    with scipy.ndimage.gaussian_filter's taps (truncate 4) and zero padding, per channel.  The map is the values summed over the
    input's channels (attributions stay additive) and fits ``deletion_insertion`` and ``attribution_ranks`` as it is.

    input:       'spec': x = spec [B,C,H,W], map [B,H,W]; 'eeg': x = eeg [B,1,Chans,T], map [B,Chans,T].
    model:       a MultimodalModel (the other input stays the sample's own); a stand-alone Spectrogram_Model (eeg=None, input='spec');
                 a stand-alone EEGNet / EEGNetAttentionDeep (spec=None, input='eeg').
    axes:        the filtered axes: 'hw' (the default for a spectrogram, saliency's [sigma, sigma, 0]), 'h' or 'w'; the EEG input is
                 blurred along time only ('w', its default): a progressive low-pass.
    steps, max_sigma, sqrt, grad_step: saliency's arguments; the filter radius int(4 (max_sigma + grad_step) + 0.5) is at most 16384.
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,...] (K <= 32): one forward pass then serves K backward passes.
    max_batch:   rows (blurred inputs) per pass, capped so that a pass addresses its largest activation and its D with 32-bit offsets.
                 The sum over the steps is carried in fp64 between passes, so, given the same gradients, no bit depends on it.
    The rows of a pass and their D are written by one launch (bx_blur_rows: separable filters, D as B_y(D_x x) + D_y(A_x x), no global
    intermediate), the one-hot gradient seeds by one (bx_expgrad_seed); every backward pass is followed by one bx_blurig_accumulate
    (fp64, ascending step order, no atomics), and bx_expgrad_finish rounds the values and sums the channels.  ``endpoint`` is the
    model's output on the input blurred with sigma_n and ``delta`` the completeness error sum(values) - (F_c(x) - endpoint_c) of the
    left Riemann sum (bx_blurig_sum_rows: fp64, fixed order); it is reported, not minimised.  In a MultimodalModel the branch whose
    input does not change runs once per sample.  The training flag and every requires_grad are restored on return.  Returns the map
    (device, fp32), or ``BlurIGResult`` with return_parts."""
    return _blur_ig(model, eeg, spec, input, steps, max_sigma, sqrt, grad_step, axes, class_idx, max_batch, return_parts)


def _blur_ig(model, eeg, spec, input, steps, max_sigma, sqrt, grad_step, axes, class_idx, max_batch, return_parts, profile=None):
    """``blur_ig`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'rows', 'forward',
    'backward', 'accumulate', 'finish' -- device events around every phase of the pass (tools/blur_ig_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "blur_ig"
    call = _Call(who, model).named(input)
    axes = _blur_axes(who, axes, not call.input_is_spec)
    n, max_sigma, sqrt, eps = _blur_steps(who, steps, max_sigma, sqrt, grad_step)
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = _nonempty(who, x)
    Kc, per = call.explained(class_idx).Kc, call.per
    if B * n >= 1 << 31 or B * Kc * per >= 1 << 31 or B * Kc > 65535:
        raise ValueError(f"{who}: B * n = {B * n} or B * Kc * per = {B * Kc * per} beyond 32-bit offsets, or B * Kc = {B * Kc} > 65535; use fewer samples per call")
    sigmas = blur_sigmas(n, max_sigma, sqrt)
    taps, radius = blur_taps(sigmas[:n], eps)
    end_taps, end_radius = blur_taps(sigmas[n:])
    _blur_fits(who, x, axes, max(taps.shape[2], end_taps.shape[2]) // 2, True)
    w = np.array([-(sigmas[i + 1] - sigmas[i]) for i in range(n)], dtype=np.float64)
    call.need_gpu("the model and its inputs")

    lib = L.load()
    gp = _GradPass(call, n, max_batch, profile, beside=per * 4)

    with gp.open():
        xs = gp.xs
        taps_d, rad_d, w_d = torch.from_numpy(taps).to(gp.dev), torch.from_numpy(radius).to(gp.dev), torch.from_numpy(w).to(gp.dev)
        gp.clean()
        acc, = gp.sums(1)
        kept = {}                                                   # the chunk's D, written beside its rows, read by its accumulates

        def write(row0, rows):
            r = torch.empty(rows, *xs.shape[1:], dtype=torch.float32, device=gp.dev)
            kept["D"] = torch.empty_like(r)
            _blur_rows(lib, xs, taps_d, rad_d, taps.shape[2], r, kept["D"], n, axes, 0, row0, rows)
            return r

        gp.sweep(write, lambda g, slot, row0, rows: L.check(lib.bx_blurig_accumulate(
            _p(g), _p(kept["D"]), _p(w_d), _p(acc), B, n, per, Kc, slot, row0, rows, _stream()), "bx_blurig_accumulate"))
        with gp.lap("finish"):
            values, amap = gp.finish_values(acc, 1)
            last = torch.empty_like(xs)                             # the end of the path: x blurred with sigma_n
            _blur_rows(lib, xs, torch.from_numpy(end_taps).to(gp.dev), torch.from_numpy(end_radius).to(gp.dev), end_taps.shape[2], last, None, 1, axes, 0, 0, B)
            with torch.no_grad():
                endpoint = _fuse(model, call.multimodal, gp.input_is_spec, call.net(last), gp.fixed).float().contiguous()
            delta = gp.completeness(values, per, endpoint)
    return gp.result(return_parts, BlurIGResult, amap, values, endpoint, delta, sigmas, n, max_sigma, sqrt, eps, axes)


# ------------------------------------------------------------------------------------------------
# Guided Integrated Gradients (Kapishnikov et al., CVPR 2021; PAIR's saliency.GuidedIG).  The definition is pinned in include/brainxai.h;
# tests/guided_ig_ref.py restates it.
GuidedIGResult = collections.namedtuple("GuidedIGResult", "map values classes out endpoint delta iterations path gradients steps fraction max_dist baseline")
GuidedIGResult.__doc__ = """What ``guided_ig(..., return_parts=True)`` returns: ``map`` fp32 [B,H,W] / [B,Chans,T], with a class axis for class_idx='all'
(what the plain call returns), ``values`` fp32 [B(,K),*x.shape[1:]] (the attribution element by element), ``classes`` int64 [B] (None
for class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), ``endpoint`` fp32 [B,K] (those of the baseline),
``delta`` fp64 [B] or [B,K] (sum of the values - (F_c(x) - endpoint_c): the completeness error), ``iterations`` int32 [B(,K),steps] (the
passes every step took), ``path`` and ``gradients`` fp32 [B(,K),steps,*x.shape[1:]] (the point and the gradient at the top of every step;
None without keep_path), all on the device; the other fields as given."""

_GUIDED_MAX_CELLS = (1 << 20) - 1                                                 # a row of bx_guided_ig_step (include/brainxai.h)
_GUIDED_MAX_PASSES = 1024


def guided_ig_passes(cells, fraction):
    """(k, cap): the rank k = floor((cells - 1) * fraction) of the threshold among a row's |gradients| (numpy's quantile(.., 'lower') index)
    and the most passes a step of ``guided_ig`` can take, ceil(cells / (k + 1)) + 2."""
    k = int(math.floor((int(cells) - 1) * float(fraction)))
    return k, -(-int(cells) // (k + 1)) + 2


def _guided_steps(who, steps, fraction, max_dist):
    if isinstance(steps, bool) or not isinstance(steps, numbers.Integral):
        raise ValueError(f"{who}: steps must be an int, got {steps!r}")
    if int(steps) < 1:
        raise ValueError(f"{who}: steps = {int(steps)} < 1")
    if isinstance(fraction, bool) or not isinstance(fraction, numbers.Real) or not 0 < fraction <= 1:
        raise ValueError(f"{who}: fraction must be a number in (0, 1], got {fraction!r}")
    if isinstance(max_dist, bool) or not isinstance(max_dist, numbers.Real) or not 0 <= max_dist <= 1:
        raise ValueError(f"{who}: max_dist must be a number in [0, 1], got {max_dist!r}")
    return int(steps), float(fraction), float(max_dist)


def guided_ig(model, eeg, spec, *, input="spec", steps=200, fraction=0.25, max_dist=0.02, baseline=0.0, class_idx=None, max_batch=256,
              keep_path=False, return_parts=False):
    """Guided Integrated Gradients (Kapishnikov et al., CVPR 2021; saliency.GuidedIG): integrated gradients along a path from the
    baseline to the input that is chosen while it is walked -- at every step only the ``fraction`` of the cells with the smallest
    |gradient| move, and no cell strays further than ``max_dist`` from the straight line -- so that cells whose large gradients have
    nothing to do with the prediction do not collect attribution on the way.  For either input of the multimodal model or a
    stand-alone branch, batched over samples and classes; F_c is the model's output log-probability of class c.

    input:       'spec': x = spec [B,C,H,W], map [B,H,W] (the values summed over the channels); 'eeg': x = eeg [B,1,Chans,T], map
                 [B,Chans,T] (the values themselves).
    model:       a MultimodalModel (the other input stays the sample's own); a stand-alone Spectrogram_Model (eeg=None, input='spec');
                 a stand-alone EEGNet / EEGNetAttentionDeep (spec=None, input='eeg').
    steps, fraction, max_dist: saliency's x_steps, fraction and max_dist; max_dist = 0 walks the straight line (the left Riemann sum of
                 integrated gradients).  A fraction so small that a step could take more than 1024 passes is refused.
    baseline:    a number, one value per channel / electrode, or a tensor of the input's shape (``gaussian_blur``'s result fits).
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,...] (K <= 32).  Every (sample, class) pair walks a path of its own.
    max_batch:   rows ((sample, class) points) per forward and backward pass.  No bit of the result depends on it.
    keep_path:   keep the point and the gradient at the top of every step (``path``, ``gradients`` of the result).
    Per step and per pass of at most max_batch rows: one forward pass, one backward pass whose one-hot seed names each row's own class
    (bx_expgrad_seed), and one bx_guided_ig_step, which runs every pass of the step's inner loop for those rows on the device -- the
    clamp to the window, the fp64 sums, the exact k-th smallest |gradient| by a radix select, the move and the fp64 attribution -- so
    the host is not asked anything inside a step; the rows' status is read once, after the last step.  bx_expgrad_finish rounds the
    values and sums the channels; ``delta`` is the completeness error sum(values) - (F_c(x) - F_c(baseline)) (bx_blurig_sum_rows), reported,
    not minimised.  In a MultimodalModel the branch whose input does not change runs once per sample.  The training flag and every
    requires_grad are restored on return.  Returns the map (device, fp32), or ``GuidedIGResult`` with return_parts."""
    return _guided_ig(model, eeg, spec, input, steps, fraction, max_dist, baseline, class_idx, max_batch, keep_path, return_parts)


def _guided_ig(model, eeg, spec, input, steps, fraction, max_dist, baseline, class_idx, max_batch, keep_path, return_parts, profile=None):
    """``guided_ig`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'forward', 'backward',
    'step', 'finish' -- device events around every phase of the pass (tools/guided_ig_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "guided_ig"
    call = _Call(who, model).named(input)
    n, fraction, max_dist = _guided_steps(who, steps, fraction, max_dist)
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = _nonempty(who, x)
    Kc, per = call.explained(class_idx).Kc, call.per
    R = B * Kc
    if per > _GUIDED_MAX_CELLS:
        raise ValueError(f"{who}: {per} cells per sample, supported 1..{_GUIDED_MAX_CELLS}")
    if R * n >= 1 << 31 or R * per >= 1 << 31 or R > 65535:
        raise ValueError(f"{who}: B * Kc * steps = {R * n} or B * Kc * per = {R * per} beyond 32-bit offsets, or B * Kc = {R} > 65535; use fewer samples per call")
    per_len, what = _per_cell(who, x, call.input_is_spec)
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    k, cap = guided_ig_passes(per, fraction)
    if cap > _GUIDED_MAX_PASSES:
        raise ValueError(f"{who}: fraction = {fraction!r} is too small for an input of {per} cells: a step could take {cap} passes, "
                         f"supported up to {_GUIDED_MAX_PASSES}")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    gp = _GradPass(call, 1, max_batch, profile)
    with gp.open():
        xs, dev, trail = gp.xs, gp.dev, tuple(gp.xs.shape[1:])
        xb = gp.baseline_rows(kind, base)
        gp.clean()
        xr = torch.empty(R, *trail, dtype=torch.float32, device=dev)             # the moving points, one row per (sample, class)
        attr = torch.empty(R, per, dtype=torch.float64, device=dev)
        l_total = torch.empty(R, dtype=torch.float64, device=dev)
        status = torch.empty(R, dtype=torch.int32, device=dev)
        iters = torch.zeros(R, n, dtype=torch.int32, device=dev)
        path = torch.empty(R, n, *trail, dtype=torch.float32, device=dev) if keep_path else None
        grads = torch.empty(R, n, *trail, dtype=torch.float32, device=dev) if keep_path else None
        with gp.lap("step"):
            L.check(lib.bx_guided_ig_init(_p(xs), _p(xb), 1, _p(xr), _p(attr), _p(l_total), _p(status), B, Kc, per, _stream()), "bx_guided_ig_init")
        endpoint = gp.endpoint(xb)

        def step(i, g, y, row0, rows):
            if keep_path:                                           # the point and the gradient at the top of the step
                path[row0:row0 + rows, i] = xr[row0:row0 + rows]
                grads[row0:row0 + rows, i] = g
            L.check(lib.bx_guided_ig_step(_p(xs), _p(xb), _p(xr), _p(g), _p(attr), _p(l_total), _p(status), _p(iters), B, Kc, per, i, n, k,
                                          max_dist, cap, row0, rows, _stream()), "bx_guided_ig_step")

        gp.row_steps(n, lambda row0, rows: xr[row0:row0 + rows].detach(), step)    # the kernel's own rows: no copy
        with gp.lap("finish"):
            values, amap = gp.finish_values(attr, 1)
            delta = gp.completeness(values, per, endpoint)
        gp.stopped(who, status, L.BX_GUIDED_OK,
                   lambda code: "a NaN among the gradients" if code == L.BX_GUIDED_NAN else f"a step that did not end within {cap} passes")
    return gp.result(return_parts, GuidedIGResult, amap, values, endpoint, delta, gp.per_row(iters), gp.per_row(path), gp.per_row(grads), n, fraction,
                     max_dist, baseline)


# ------------------------------------------------------------------------------------------------
# Optimised perturbation masks (Fong & Vedaldi, ICCV 2017, "meaningful perturbations"; the basis of TorchRay's extremal perturbations).
# The definition is pinned in include/brainxai.h; tests/maskopt_ref.py restates it.
MaskExplainResult = collections.namedtuple("MaskExplainResult", "map mask upsampled history final clean reference classes out path gradients outputs input mode "
                                           "grid iterations lr l1 tv tv_beta betas eps baseline cells score")
MaskExplainResult.__doc__ = """What ``mask_explain(..., return_parts=True)`` returns: ``map`` fp32 [B,Hm,Wm], with a class axis for class_idx='all' (what
the plain call returns: 1 - upsampled for deletion, upsampled for preservation), ``mask`` fp32 [B(,K),gh,gw] (the learned grids),
``upsampled`` fp32 [B(,K),Hm,Wm] (U(mask)), ``history`` fp64 [B(,K),iterations,3] = (score, mean of the grid, TV_beta of the grid) before
every update, ``final`` fp32 [B(,K)] (the score of the input seen through the final mask, from one more forward pass), ``clean`` and
``reference`` fp32 [B(,K)] (the score of the input itself and of the all-baseline input), ``classes`` int64 [B] (None for
class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), ``path`` fp32 [B(,K),iterations,gh,gw], ``gradients`` fp32
[B(,K),iterations,*x.shape[1:]] and ``outputs`` fp32 [B(,K),iterations,K] (the grid, the gradient and the model's output at the top of every
iteration; None without keep_path), all on the device; the other fields as given (``grid`` as the pair used)."""

_MASKOPT_MODES = {"deletion": L.BX_MASKOPT_DELETION, "preservation": L.BX_MASKOPT_PRESERVATION}
_MASKOPT_SCORES = {"prob": L.BX_MASKOPT_PROB, "logprob": L.BX_MASKOPT_LOGPROB}
_MASKOPT_MAX_ROWS = 65535


def _maskopt_grid(who, grid, Hm, Wm):
    """-> (gh, gw): a pair as given, an int clipped per axis to min(grid, Hm / Wm, 32); checked against the domain."""
    if isinstance(grid, numbers.Integral) and not isinstance(grid, bool):
        if int(grid) < 1:
            raise ValueError(f"{who}: grid = {int(grid)} < 1")
        gh, gw = min(int(grid), Hm, _RISE_MAX_G), min(int(grid), Wm, _RISE_MAX_G)
    else:
        try:
            gh, gw = (int(v) for v in grid)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: grid must be an int or a pair (gh, gw), got {grid!r}") from None
    if not (1 <= gh <= min(_RISE_MAX_G, Hm) and 1 <= gw <= min(_RISE_MAX_G, Wm)):
        raise ValueError(f"{who}: grid {gh} x {gw} outside 1..min({_RISE_MAX_G}, {Hm}) x 1..min({_RISE_MAX_G}, {Wm})")
    return gh, gw


def _maskopt_settings(who, iterations, lr, l1, tv, tv_beta, betas, eps):
    if isinstance(iterations, bool) or not isinstance(iterations, numbers.Integral):
        raise ValueError(f"{who}: iterations must be an int, got {iterations!r}")
    if int(iterations) < 1:
        raise ValueError(f"{who}: iterations = {int(iterations)} < 1")
    for name, v in (("lr", lr), ("l1", l1), ("tv", tv), ("eps", eps)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}")
    if isinstance(tv_beta, bool) or not isinstance(tv_beta, numbers.Integral) or int(tv_beta) not in (1, 2, 3):
        raise ValueError(f"{who}: tv_beta must be 1, 2 or 3, got {tv_beta!r}")
    try:
        b1, b2 = (float(v) for v in betas)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: betas must be a pair (b1, b2), got {betas!r}") from None
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"{who}: betas ({b1}, {b2}) outside [0, 1)")
    return int(iterations), float(lr), float(l1), float(tv), int(tv_beta), b1, b2, float(eps)


def mask_explain(model, eeg, spec, *, input="spec", mode="deletion", grid=16, iterations=300, lr=0.1, l1=0.01, tv=0.2, tv_beta=3, betas=(0.9, 0.999),
                 eps=1e-8, baseline=0.0, cells="electrode_time", class_idx=None, score="prob", max_batch=256, keep_path=False, return_parts=False):
    """Optimised perturbation masks (Fong & Vedaldi, ICCV 2017, "meaningful perturbations"; the basis of TorchRay's extremal
    perturbations): per (sample, class) the smallest smooth region whose removal (mode='deletion') or whose preservation alone
    ('preservation') changes the class score is learned by Adam -- the objective behind ``deletion_insertion``, optimised directly.
    The mask is a gh x gw grid m in [0, 1], up-sampled bilinearly (align_corners=False) to the mask domain, M = U(m); the model sees
    X = base + M (x - base), and per row
        deletion      L = l1 mean(1 - m) + tv TV_beta(m) + s_c(X)          preservation  L = l1 mean(m) + tv TV_beta(m) - s_c(X)
    with TV_beta the sum of |d|^beta over the neighbour differences of the grid.

    input:       'spec': masks over [H,W], one value for all channels of a pixel, map [B,H,W]; 'eeg': masks over [Chans,T], map
                 [B,Chans,T], or with cells='time' over [1,T] (a column's value applies to every electrode), map [B,1,T].
    model:       a MultimodalModel (the other input stays the sample's own); a stand-alone Spectrogram_Model (eeg=None, input='spec');
                 a stand-alone EEGNet / EEGNetAttentionDeep (spec=None, input='eeg').
    grid:        a pair (gh, gw) in 1..min(32, Hm) x 1..min(32, Wm), or an int, clipped per axis to min(grid, Hm or Wm, 32).
    iterations, lr, betas, eps: Adam's, from a grid of ones; l1, tv, tv_beta (1, 2 or 3): the regularisers.
    baseline:    what a masked-out cell shows: a number, one value per channel / electrode, or a tensor of the input's shape
                 (``gaussian_blur``'s result is Fong & Vedaldi's blurred reference).
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,...] (K <= 32).  Every (sample, class) pair learns a mask of its own.
    score:       'prob' or 'logprob': s_c, the class probability or the log-probability.
    max_batch:   rows ((sample, class) pairs) per forward and backward pass.  No bit of the result depends on it.
    keep_path:   keep the grid, the gradient and the output at the top of every iteration (``path``, ``gradients``, ``outputs``).
    The map is 1 - U(m) for deletion and U(m) for preservation: high means important, and it fits ``deletion_insertion``,
    ``attribution_ranks``, ``map_similarity`` and ``infidelity`` as it is.  Per iteration and per pass of at most max_batch rows: the rows
    (bx_maskopt_rows_*), one forward pass, one backward pass whose one-hot seed names each row's own class (bx_expgrad_seed), and one
    bx_maskopt_step, which folds dF/dX back through the blend and the up-sampling onto the grid in fp64 in a fixed order, adds the
    regularisers, takes the Adam step, clamps, and records the history -- the host is asked nothing; the rows' status is read once,
    after the last iteration.  In a MultimodalModel the branch whose input does not change runs once per sample.  The training flag and
    every requires_grad are restored on return.  Returns the map (device, fp32), or ``MaskExplainResult`` with return_parts."""
    return _mask_explain(model, eeg, spec, input, mode, grid, iterations, lr, l1, tv, tv_beta, betas, eps, baseline, cells, class_idx, score, max_batch,
                         keep_path, return_parts)


def _mask_explain(model, eeg, spec, input, mode, grid, iterations, lr, l1, tv, tv_beta, betas, eps, baseline, cells, class_idx, score, max_batch, keep_path,
                  return_parts, profile=None):
    """``mask_explain`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'rows', 'forward',
    'backward', 'step', 'finish' -- device events around every phase of the pass (tools/mask_explain_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "mask_explain"
    call = _Call(who, model).named(input)
    if mode not in _MASKOPT_MODES:
        raise ValueError(f"{who}: unknown mode {mode!r}; use 'deletion' or 'preservation'")
    if score not in _MASKOPT_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    if cells not in _RISE_CELLS:
        raise ValueError(f"{who}: unknown cells {cells!r}; use 'electrode_time' or 'time'")
    if cells == "time" and input != "eeg":
        raise ValueError(f"{who}: cells='time' masks time columns of the EEG input; input='spec' has no such map")
    n, lr, l1, tv, tv_beta, b1, b2, eps = _maskopt_settings(who, iterations, lr, l1, tv, tv_beta, betas, eps)
    max_batch = _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    B = _nonempty(who, x)
    per_len, what = _per_cell(who, x, call.input_is_spec)
    if call.input_is_spec:
        map_rows, Hm, Wm = 0, int(x.shape[2]), int(x.shape[3])
    else:
        map_rows = 1 if cells == "time" else int(x.shape[2])
        Hm, Wm = map_rows, int(x.shape[3])
    if not 1 <= Hm * Wm <= _FAITH_MAX_N:
        raise ValueError(f"{who}: {Hm * Wm} cells per mask, supported 1..{_FAITH_MAX_N}")
    gh, gw = _maskopt_grid(who, grid, Hm, Wm)
    K, Kc, per, all_classes = call.explained(class_idx).K, call.Kc, call.per, call.all_classes
    R = B * Kc
    if R * per >= 1 << 31 or R * n * 3 >= 1 << 31 or R * Hm * Wm >= 1 << 31 or (keep_path and R * n * per >= 1 << 31) or R > _MASKOPT_MAX_ROWS:
        raise ValueError(f"{who}: B * Kc * per = {R * per}, B * Kc * iterations * 3 = {R * n * 3}" + (f", B * Kc * iterations * per = {R * n * per} (keep_path)" if keep_path else "")
                         + f" beyond 32-bit offsets, or B * Kc = {R} > {_MASKOPT_MAX_ROWS}; use fewer samples per call")
    kind, base = _baseline_for(who, baseline, x, per_len, what)
    call.need_gpu("the model and its inputs")

    lib = L.load()
    gp = _GradPass(call, 1, max_batch, profile)
    code_mode, code_score = _MASKOPT_MODES[mode], _MASKOPT_SCORES[score]
    Cc, Hh, Ww = (int(v) for v in x.shape[1:])
    with gp.open():
        xs, dev, trail = gp.xs, gp.dev, tuple(gp.xs.shape[1:])
        base = base.to(dev, torch.float32).reshape(xs.shape if kind == 2 else (-1,)).contiguous()
        gp.clean()
        row_cls = gp.row_classes()
        m = torch.empty(R, gh, gw, dtype=torch.float32, device=dev)              # the grids, one row per (sample, class)
        mu = torch.empty(R, gh, gw, dtype=torch.float64, device=dev)
        nu = torch.empty(R, gh, gw, dtype=torch.float64, device=dev)
        status = torch.empty(R, dtype=torch.int32, device=dev)
        history = torch.zeros(R, n, 3, dtype=torch.float64, device=dev)
        scratch = torch.empty(min(gp.max_rows, R), Hm, gw, dtype=torch.float64, device=dev)
        path = torch.empty(R, n, gh, gw, dtype=torch.float32, device=dev) if keep_path else None
        grads = torch.empty(R, n, *trail, dtype=torch.float32, device=dev) if keep_path else None
        outs = torch.empty(R, n, K, dtype=torch.float32, device=dev) if keep_path else None

        def write(row0, rows):
            r = torch.empty(rows, *trail, dtype=torch.float32, device=dev)
            if gp.input_is_spec:
                L.check(lib.bx_maskopt_rows_spec(_p(xs), _p(m), _p(base), kind, _p(r), B, Kc, Cc, Hh, Ww, gh, gw, row0, rows, _stream()), "bx_maskopt_rows_spec")
            else:
                L.check(lib.bx_maskopt_rows_eeg(_p(xs), _p(m), map_rows, _p(base), kind, _p(r), B, Kc, Hh, Ww, gh, gw, row0, rows, _stream()), "bx_maskopt_rows_eeg")
            return r

        def scores(logp):
            """fp32 [B(,K)] scores of log-probabilities [R,K], row r's own class (every class for class_idx='all')"""
            s = logp if score == "logprob" else _softmax_rows(logp)
            return s.gather(1, row_cls.long()[:, None])[:, 0]

        def step(it, g, y, row0, rows):
            if keep_path:                                           # the grid, the gradient and the output at the top of the iteration
                path[row0:row0 + rows, it] = m[row0:row0 + rows]
                grads[row0:row0 + rows, it] = g
                outs[row0:row0 + rows, it] = y
            L.check(lib.bx_maskopt_step(_p(xs), _p(base), kind, _p(g), _p(y), _p(row_cls), _p(m), _p(mu), _p(nu), _p(status), _p(history), None,
                                        _p(scratch), B, Kc, Cc, Hh, Ww, map_rows, K, gh, gw, code_mode, code_score, tv_beta, lr, l1, tv, b1, b2, eps,
                                        1.0 - b1 ** (it + 1), 1.0 - b2 ** (it + 1), it, n, row0, rows, _stream()), "bx_maskopt_step")

        with gp.lap("step"):
            L.check(lib.bx_maskopt_init(_p(m), _p(mu), _p(nu), _p(status), B, Kc, gh, gw, 0, R, _stream()), "bx_maskopt_init")
        endpoint = gp.endpoint(gp.baseline_rows(kind, base))
        gp.row_steps(n, write, step, rows_lap=True)
        with gp.lap("finish"), torch.no_grad():
            up = torch.empty(R, Hm, Wm, dtype=torch.float32, device=dev)
            L.check(lib.bx_maskopt_masks(_p(m), _p(up), B, Kc, gh, gw, Hm, Wm, 0, R, _stream()), "bx_maskopt_masks")
            amap = 1.0 - up if mode == "deletion" else up
            last = torch.empty(R, K, dtype=torch.float32, device=dev)
            for row0, rows in _sample_chunks(R, gp.max_rows):
                last[row0:row0 + rows] = gp.forward(write(row0, rows), row0, rows, Kc)
            rep = (lambda t: t.repeat_interleave(Kc, dim=0) if all_classes else t)
            final, clean, reference = scores(last), scores(rep(gp.out)), scores(rep(endpoint))
        gp.stopped(who, status, L.BX_MASKOPT_OK, lambda code: "a NaN among the gradients or the outputs")
    shape = gp.per_row
    parts = (lambda amap, mask, classes, out, *rest: MaskExplainResult(amap, mask, *rest[:5], classes, out, *rest[5:]))
    return gp.result(return_parts, parts, amap.reshape(B, Kc, Hm, Wm), m.reshape(B, Kc, gh, gw), shape(up), shape(history), shape(final), shape(clean),
                     shape(reference), shape(path), shape(grads), shape(outs), input, mode, (gh, gw), n, lr, l1, tv, tv_beta, (b1, b2), eps, baseline, cells, score)


# ------------------------------------------------------------------------------------------------
# Spectral attributions of the EEG input: amplitude gradients and spectral occlusion (Schirrmeister et al., Hum. Brain Mapp. 2017;
# braindecode's compute_amplitude_gradients).  The definition is pinned in include/brainxai.h; tests/spectral_ref.py restates it.
SpectralGradientsResult = collections.namedtuple("SpectralGradientsResult", "map bands gradient classes out freqs band_bins delta kind steps")
SpectralGradientsResult.__doc__ = """What ``spectral_gradients(..., return_parts=True)`` returns: ``map`` fp32 [B,Chans,F], with a class axis for
class_idx='all' (what the plain call returns), ``bands`` fp64 [B(,K),Chans,nb] (the map summed over each band's bins; None without
bands), ``gradient`` fp32 [B(,K),1,Chans,T] (the time-domain, path-weighted gradient the map was formed from), ``classes`` int64 [B]
(None for class_idx='all'), ``out`` fp32 [B,K] (the log-probabilities of the clean input), all on the device; ``freqs`` numpy fp64 [F]
(the bins' frequencies f fs / T, cycles per sample without fs), ``band_bins`` the bands' bin ranges [(f_lo, f_hi), ...] (None without
bands), ``delta`` fp64 [B] or [B,K] (sum of the map - (F_c(x) - F_c(0)), the completeness error of the quadrature; only for steps > 1
with kind='gradient_x_amplitude', None otherwise); ``kind`` and ``steps`` as given."""
SpectralOcclusionResult = collections.namedtuple("SpectralOcclusionResult", "drops scores clean classes band_bins")
SpectralOcclusionResult.__doc__ = """What ``spectral_occlusion(..., return_parts=True)`` returns: ``drops`` fp32 [B(,K),nb] or [B(,K),Chans,nb] (what
the plain call returns), ``scores`` fp32 [B,N,K] (the score of every class for every band-stopped input; row j = q for cells='band',
j = q * Chans + e for 'electrode_band'), ``clean`` fp32 [B,K], ``classes`` int64 [B] (None for class_idx='all'), all on the device;
``band_bins`` the bands' bin ranges [(f_lo, f_hi), ...]."""

_SPECTRAL_KINDS = {"amplitude_gradient": L.BX_SPECTRAL_AMPLITUDE_GRADIENT, "gradient_x_amplitude": L.BX_SPECTRAL_GRADIENT_X_AMPLITUDE}
_SPECTRAL_CELLS = {"band": L.BX_SPECTRAL_CELLS_BAND, "electrode_band": L.BX_SPECTRAL_CELLS_ELECTRODE_BAND}
CLINICAL_BANDS = {"delta": (0.5, 4.0), "theta": (4.0, 8.0), "alpha": (8.0, 13.0), "beta": (13.0, 30.0)}       # Hz


def spectral_twiddles(T):
    """fp64 numpy [T,2]: (cos, sin)(2 pi j / T), j = 0..T-1 -- the table the transform kernels walk.  The angle is reduced to an octant
    in integers first, so that sin and cos are only evaluated on [0, pi/4]: multiples of a quarter turn are exact (a Nyquist bin has
    no imaginary part) and every entry is within about one unit in the last place."""
    j = np.arange(T, dtype=np.int64)
    octant, rem = np.divmod(8 * j, T)
    odd = (octant & 1).astype(bool)
    phi = np.pi * np.where(odd, T - rem, rem).astype(np.float64) / (4.0 * T)
    c, s = np.cos(phi), np.sin(phi)
    major, minor = np.where(odd, s, c), np.where(odd, c, s)               # (cos, sin) of the angle folded into the first quadrant
    quad = octant >> 1
    cos = np.select([quad == 0, quad == 1, quad == 2], [major, -minor, -major], minor)
    sin = np.select([quad == 0, quad == 1, quad == 2], [minor, major, -minor], -major)
    return np.ascontiguousarray(np.stack([cos, sin], axis=1))


def _spectral_fs(who, fs):
    if fs is None:
        return None
    if isinstance(fs, bool) or not isinstance(fs, numbers.Real) or not math.isfinite(fs) or fs <= 0:
        raise ValueError(f"{who}: fs must be a finite number > 0 or None, got {fs!r}")
    return float(fs)


def spectral_band_bins(bands, T, fs=None, who="spectral_band_bins"):
    """-> [(f_lo, f_hi), ...]: the bin range of every band of a length-T transform.  Bin f belongs to (lo, hi) iff lo <= f fs / T < hi,
    decided in fp64 as lo T <= f fs < hi T.  bands: 'clinical' (delta, theta, alpha, beta of CLINICAL_BANDS; needs fs in Hz) or a
    sequence of (lo, hi) with 0 <= lo <= hi; fs None: edges in cycles per sample.  A band may hold no bin."""
    fs = _spectral_fs(who, fs)
    if isinstance(bands, str):
        if bands != "clinical":
            raise ValueError(f"{who}: unknown bands {bands!r}; use 'clinical' or a sequence of (lo, hi)")
        if fs is None:
            raise ValueError(f"{who}: bands='clinical' are in Hz and need fs (the stacker's 19 x 2000 traces are 40 Hz, the montage's 37 x 3000 are 200 Hz)")
        edges = list(CLINICAL_BANDS.values())
    else:
        try:
            edges = [(lo, hi) for lo, hi in bands]
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bands must be 'clinical' or a sequence of (lo, hi) pairs, got {bands!r}") from None
    if not edges:
        raise ValueError(f"{who}: no bands given")
    f = np.arange(int(T) // 2 + 1, dtype=np.float64) * (1.0 if fs is None else fs)
    bins = []
    for lo, hi in edges:
        if any(isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) for v in (lo, hi)):
            raise ValueError(f"{who}: band edges must be finite numbers, got {(lo, hi)!r}")
        if lo < 0 or hi < lo:
            raise ValueError(f"{who}: band {(lo, hi)!r} has a negative or inverted edge; use 0 <= lo <= hi")
        bins.append((int(np.count_nonzero(f < float(lo) * T)), int(np.count_nonzero(f < float(hi) * T))))
    return bins


def _spectral_shape(who, x):
    """-> (B, Chans, T, F) of an EEG input within the transform's limit."""
    B = _nonempty(who, x)
    Chans, T = int(x.shape[2]), int(x.shape[3])
    if T > L.BX_SPECTRAL_MAX_T:
        raise ValueError(f"{who}: T = {T}, supported 1..{L.BX_SPECTRAL_MAX_T}")
    return B, Chans, T, T // 2 + 1


def _rdft(lib, xs, tw_d, T):
    """(re, im) fp64 [R,F] of fp32 rows xs [..., T] (R = the other axes flattened), bx_rdft_rows."""
    R = xs.numel() // T
    re = torch.empty(R, T // 2 + 1, dtype=torch.float64, device=xs.device)
    im = torch.empty_like(re)
    L.check(lib.bx_rdft_rows(_p(xs), _p(tw_d), _p(re), _p(im), R, T, _stream()), "bx_rdft_rows")
    return re, im


def _band_sum(lib, values, bins_d, nb):
    F = int(values.shape[-1])
    out = torch.empty(*values.shape[:-1], nb, dtype=torch.float64, device=values.device)
    L.check(lib.bx_band_sum(_p(values), _p(bins_d), _p(out), values.numel() // F, F, nb, _stream()), "bx_band_sum")
    return out


def eeg_spectrum(x, *, fs=None):
    """(re, im, freqs): the real DFT of every electrode's trace, fp64 [B,Chans,F] each on the device, F = T // 2 + 1, and the bins'
    frequencies (numpy fp64 [F]: f fs / T, cycles per sample without fs) -- X_f = sum_t x_t exp(-2 pi i f t / T), numpy's rfft, by the
    kernel ``spectral_gradients`` and ``spectral_occlusion`` transform their input with (bx_rdft_rows: a direct fp64 sum in ascending t for
    any 1 <= T <= 8192, twiddles from a host-made fp64 table).  x: an EEG input [B,1,Chans,T] or [B,Chans,T]."""
    who = "eeg_spectrum"
    fs = _spectral_fs(who, fs)
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"{who}: x must be a tensor [B,1,Chans,T] or [B,Chans,T]")
    x4 = x if x.dim() == 4 else x[:, None]
    B, Chans, T, F = _spectral_shape(who, x4)
    if B * Chans * T >= 1 << 31:
        raise ValueError(f"{who}: B * Chans * T = {B * Chans * T} beyond 32-bit offsets")
    if not x.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the transform runs on the GPU; there is no CPU path")
    lib = L.load()
    with torch.cuda.device(x.device):
        xs = x4.detach().to(torch.float32).contiguous()
        re, im = _rdft(lib, xs, torch.from_numpy(spectral_twiddles(T)).to(xs.device), T)
    return re.reshape(B, Chans, F), im.reshape(B, Chans, F), np.arange(F, dtype=np.float64) * (1.0 if fs is None else fs) / T


def band_sums(map, bands, *, T, fs=None):
    """fp64 [..., nb]: a map [..., F] of a length-T transform (F = T // 2 + 1; ``spectral_gradients``' map, or anything per bin) summed
    over each band's bins in ascending f (bx_band_sum).  bands and fs as in ``spectral_band_bins``."""
    who = "band_sums"
    if isinstance(T, bool) or not isinstance(T, numbers.Integral) or T < 1:
        raise ValueError(f"{who}: T must be an int >= 1, got {T!r}")
    bins = spectral_band_bins(bands, int(T), fs, who)
    if not isinstance(map, torch.Tensor) or map.dim() < 1 or int(map.shape[-1]) != int(T) // 2 + 1 or map.numel() == 0:
        raise ValueError(f"{who}: map must be a tensor [..., F] with F = T // 2 + 1 = {int(T) // 2 + 1}")
    if map.numel() >= 1 << 31:
        raise ValueError(f"{who}: {map.numel()} elements, beyond 32-bit offsets")
    if not map.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the sums are taken on the GPU; there is no CPU path")
    lib = L.load()
    with torch.cuda.device(map.device):
        return _band_sum(lib, map.detach().to(torch.float32).contiguous(), torch.tensor(bins, dtype=torch.int32, device=map.device), len(bins))


def spectral_gradients(model, eeg, spec, *, kind="amplitude_gradient", steps=1, fs=None, bands=None, class_idx=None, max_batch=256, return_parts=False):
    """The EEG input explained by frequency: amplitude gradients (Schirrmeister et al. 2017; braindecode's
    compute_amplitude_gradients) in closed form.  With X the real DFT of an electrode's trace x (F = T // 2 + 1 bins), u = X / |X| its
    phase, g the gradient of the explained log-probability F_c by the trace and G its DFT, c_f = 1 for f = 0 and the Nyquist bin, 2
    otherwise:
        kind='amplitude_gradient':    dF_c/dA_f     = (c_f / T) Re(u_f conj(G_f))   -- what autograd through irfft(A e^{i phi}) gives by A
        kind='gradient_x_amplitude':  A_f dF_c/dA_f = (c_f / T) Re(X_f conj(G_f))   -- per electrode it sums over f to sum_t g_t x_t
    steps = n > 1 replaces g by sum_k w_k dF_c/dx(alpha_k x) with ``ig_nodes(n)``: the path from zero amplitude to x at x's phase, so
    that gradient x amplitude is integrated gradients per frequency and sums to F_c(x) - F_c(0) up to the quadrature error ``delta``.

    model:       a MultimodalModel (the spectrogram stays the sample's own, its branch runs once per sample); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None).  eeg [B,1,Chans,T], T <= 8192, any length (no power of two needed).
    fs, bands:   the sampling rate (Hz) and the bands of ``spectral_band_bins``: 'clinical' or (lo, hi) pairs; with bands the parts
                 carry the map summed per band.  fs has no default: the stacker's 19 x 2000 traces are 40 Hz, the montage's 200 Hz.
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample (sequence / tensor [B]); 'all' =
                 every class, the map gains a class axis [B,K,Chans,F] (K <= 32): one forward pass then serves K backward passes.
    max_batch:   rows (path points) per pass.  The gradient sum is carried in fp64 between passes, so, given the same gradients, no
                 bit depends on it.
    X is transformed once per call (bx_rdft_rows); the path rows are bx_expgrad_rows against a zero background (exactly fl32(alpha x)),
    the seeds bx_expgrad_seed; every backward pass is followed by one bx_spectral_accumulate (fp64, ascending step order, no atomics);
    bx_spectral_values transforms the gradient sums in registers and forms the map; bx_band_sum the bands.  All transforms are direct
    fp64 sums in a fixed order over a host-made twiddle table.  The training flag and every requires_grad are restored on return.
    Returns the map (device, fp32), or ``SpectralGradientsResult`` with return_parts."""
    return _spectral_gradients(model, eeg, spec, kind, steps, fs, bands, class_idx, max_batch, return_parts)


def _spectral_gradients(model, eeg, spec, kind, steps, fs, bands, class_idx, max_batch, return_parts, profile=None):
    """``spectral_gradients`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'transform',
    'rows', 'forward', 'backward', 'accumulate', 'values' -- device events around every phase (tools/spectral_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "spectral_gradients"
    if not isinstance(kind, str) or kind not in _SPECTRAL_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r}; use 'amplitude_gradient' or 'gradient_x_amplitude'")
    if isinstance(steps, bool) or not isinstance(steps, numbers.Integral):
        raise ValueError(f"{who}: steps must be an int, got {steps!r}")
    n = int(steps)
    if n < 1:
        raise ValueError(f"{who}: steps = {n} < 1")
    max_batch = _max_batch(who, max_batch)
    call = _Call(who, model, "eeg").tensors(eeg, spec)
    B, Chans, T, F = _spectral_shape(who, call.x)
    fs = _spectral_fs(who, fs)
    band_bins = None if bands is None else spectral_band_bins(bands, T, fs, who)
    Kc, per, all_classes = call.explained(class_idx).Kc, call.per, call.all_classes
    if B * n >= 1 << 31 or B * Kc * per >= 1 << 31:
        raise ValueError(f"{who}: B * n = {B * n} or B * Kc * per = {B * Kc * per} beyond 32-bit offsets; use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    alpha, w = (np.ones(1), np.ones(1)) if n == 1 else ig_nodes(n)
    gp = _GradPass(call, n, max_batch, profile)

    with gp.open():
        xs, dev = gp.xs, gp.dev
        tw_d = torch.from_numpy(spectral_twiddles(T)).to(dev)
        w_d = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
        alpha_d = torch.from_numpy(np.tile(alpha.astype(np.float32), B)).to(dev)
        zero_bg = torch.zeros(1, per, dtype=torch.float32, device=dev)
        idx_d = torch.zeros(B * n, dtype=torch.int32, device=dev)
        gp.clean()
        with gp.lap("transform"):
            re, im = _rdft(lib, xs, tw_d, T)                        # X once per call, whatever the classes
        acc, = gp.sums(1)

        def write(row0, rows):
            r = torch.empty(rows, *xs.shape[1:], dtype=torch.float32, device=dev)
            L.check(lib.bx_expgrad_rows(_p(xs), _p(zero_bg), _p(idx_d), _p(alpha_d), _p(r), B, 1, n, per, row0, rows, _stream()), "bx_expgrad_rows")
            return r

        gp.sweep(write, lambda g, slot, row0, rows: L.check(lib.bx_spectral_accumulate(
            _p(g), _p(w_d), _p(acc), B, n, per, Kc, slot, row0, rows, _stream()), "bx_spectral_accumulate"))
        with gp.lap("values"):
            amap = gp.empty(Chans, F)
            L.check(lib.bx_spectral_values(_p(acc), _p(re), _p(im), _p(tw_d), _p(amap), B, Kc, Chans, T, _SPECTRAL_KINDS[kind], _stream()),
                    "bx_spectral_values")
        if not return_parts:
            return amap if all_classes else amap[:, 0]
        gradient, _ = gp.finish_values(acc, 1)
        band_vals = None if band_bins is None else _band_sum(lib, amap, torch.tensor(band_bins, dtype=torch.int32, device=dev), len(band_bins))
        delta = None
        if n > 1 and kind == "gradient_x_amplitude":
            with torch.no_grad():                                   # F(0): EEGNet in eval mode treats every row alike, one row serves all samples
                at_zero = call.net(torch.zeros_like(xs[:1]))
                at_zero = _fuse(model, call.multimodal, False, at_zero.expand(B, -1).contiguous(), gp.fixed).float()
            delta = gp.completeness(amap, Chans * F, at_zero)
        if not all_classes:
            amap, gradient = amap[:, 0], gradient[:, 0]
            band_vals = None if band_vals is None else band_vals[:, 0]
    freqs = np.arange(F, dtype=np.float64) * (1.0 if fs is None else fs) / T
    return SpectralGradientsResult(amap, band_vals, gradient, None if gp.classes is None else gp.classes.long(), gp.out, freqs, band_bins, delta, kind, n)


def spectral_occlusion(model, eeg, spec, *, bands, fs=None, cells="band", class_idx=None, score="prob", max_batch=256, return_parts=False):
    """Spectral perturbation of the EEG input (Schirrmeister et al. 2017, forward-only): remove one frequency band from the traces and
    record how much the class score drops.  drops[b,k,q] = S0[b,k] - S[b,j,k], with S0 the score of the clean input and S[b,j,.] that
    of the input whose band q is stopped: x - y_q, y_q the band's component of x (the inverse transform of X restricted to the band's
    bins, formed in fp64 and subtracted before one rounding to fp32).

    bands, fs:   the bands of ``spectral_band_bins``: 'clinical' (needs fs in Hz) or (lo, hi) pairs; a band without a bin leaves the
                 input as it is and drops 0.
    cells:       'band': every electrode loses the band, drops [B(,K),nb]; 'electrode_band': one electrode at a time,
                 drops [B(,K),Chans,nb] -- "which band, at which electrode".
    model, class_idx, max_batch: as ``spectral_gradients``;  score: 'prob' or 'logprob'.
    (N + 1) * B forward evaluations in eval mode without autograd, N = nb or Chans * nb; the clean input takes the path of the rows, as
    in ``occlusion``.  X is transformed once (bx_rdft_rows); the rows are written straight in the EEG layout (bx_bandstop_rows: an
    electrode the row does not select is x bit for bit).  The training flag and every requires_grad are restored on return.  Returns
    the drops (device, fp32), or ``SpectralOcclusionResult`` with return_parts."""
    return _spectral_occlusion(model, eeg, spec, bands, fs, cells, class_idx, score, max_batch, return_parts)


def _spectral_occlusion(model, eeg, spec, bands, fs, cells, class_idx, score, max_batch, return_parts, profile=None):
    """``spectral_occlusion`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'transform',
    'perturb', 'forward'."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "spectral_occlusion"
    if not isinstance(cells, str) or cells not in _SPECTRAL_CELLS:
        raise ValueError(f"{who}: unknown cells {cells!r}; use 'band' or 'electrode_band'")
    if score not in _FAITH_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    max_batch = _max_batch(who, max_batch)
    call = _Call(who, model, "eeg").tensors(eeg, spec)
    B, Chans, T, F = _spectral_shape(who, call.x)
    band_bins = spectral_band_bins(bands, T, fs, who)
    nb = len(band_bins)
    N = nb if cells == "band" else nb * Chans
    K, cls_h, all_classes = call.explained(class_idx).K, call.cls_h, call.all_classes
    if B * N * K >= 1 << 31 or B * Chans * T >= 1 << 31:
        raise ValueError(f"{who}: B * N * K = {B * N * K} or B * Chans * T = {B * Chans * T} beyond 32-bit offsets; use fewer samples per call")
    call.need_gpu("the model and its inputs")

    lib = L.load()
    dev = call.x.device
    use_logprob = score == "logprob"
    rp = _RowPass(call, 0, torch.zeros(1), max_batch, profile)

    with rp.open():
        xs = rp.xs
        with rp.lap("forward"):
            rp.fix_other()
            clean = torch.empty(B, K, dtype=torch.float32, device=dev)
            for b0, ng in rp.groups():                              # the clean input takes the path of the rows, in chunks of the same size
                clean[b0:b0 + ng] = rp.scores(rp.clean_rows(b0, ng), b0, ng, logprob=use_logprob)
        classes = _class_tensor(cls_h, all_classes, clean, dev)
        with rp.lap("transform"):
            tw_d = torch.from_numpy(spectral_twiddles(T)).to(dev)
            bins_d = torch.tensor(band_bins, dtype=torch.int32, device=dev)
            re, im = _rdft(lib, xs, tw_d, T)

        def write(b0, ng, n0, n):
            out = torch.empty(ng * n, 1, Chans, T, dtype=torch.float32, device=dev)
            L.check(lib.bx_bandstop_rows(_p(xs[b0:b0 + ng]), _p(re[b0 * Chans:(b0 + ng) * Chans]), _p(im[b0 * Chans:(b0 + ng) * Chans]), _p(tw_d), _p(bins_d),
                                         _p(out), ng, Chans, T, nb, _SPECTRAL_CELLS[cells], n0, n, _stream()), "bx_bandstop_rows")
            return out

        S = rp.sweep(N, write, logprob=use_logprob)
        d = clean[:, None, :] - S                                   # [B,N,K]
        if not all_classes:
            d = d.gather(2, classes.long().reshape(B, 1, 1).expand(B, N, 1))
        d = d.permute(0, 2, 1)                                      # [B,K or 1,N]
        drops = (d if cells == "band" else d.reshape(B, -1, nb, Chans).transpose(2, 3)).contiguous()
        if not all_classes:
            drops = drops[:, 0]
    if not return_parts:
        return drops
    return SpectralOcclusionResult(drops, S, clean, None if classes is None else classes.long(), band_bins)

# ------------------------------------------------------------------------------------------------
# Infidelity and max-sensitivity (Yeh et al., NeurIPS 2019; Captum's metrics.infidelity and metrics.sensitivity_max): how well an
# attribution predicts the effect of a small perturbation, and how stable it is around the input.  The definitions are pinned in
# include/brainxai.h; tests/infidelity_ref.py restates them.
InfidelityResult = collections.namedtuple("InfidelityResult", "infidelity beta dots drops clean classes sigma nsamples seed")
InfidelityResult.__doc__ = """What ``infidelity(..., return_parts=True)`` returns: ``infidelity`` and ``beta`` fp64 [B] or [B,K] (beta is 1 without
normalize), ``dots`` and ``drops`` fp64 [B,n] or [B,K,n] (d and Delta of every draw), ``clean`` fp32 [B,K] (the scores of the unperturbed
input), ``classes`` int64 [B] (None for class_idx='all'), ``sigma`` fp32 [B], all on the device; ``nsamples`` and ``seed`` as given."""

SensitivityResult = collections.namedtuple("SensitivityResult", "sensitivity distances norms radius nsamples seed")
SensitivityResult.__doc__ = """What ``sensitivity_max(..., return_parts=True)`` returns: ``sensitivity`` fp64 [B], ``distances`` fp64 [B,n] (the L2
distance of every perturbed explanation from the clean one), ``norms`` fp64 [B] (the L2 norm of the clean explanation), ``radius`` fp32
[B], all on the device; ``nsamples`` and ``seed`` as given."""


def _infidelity_cells(who, attribution, x, input_is_spec, all_classes, K):
    """-> (grouped, cells): whether a draw moves a whole pixel / time column (else one element), and the cells of a sample."""
    B = int(x.shape[0])
    lead = (B, K) if all_classes else (B,)
    shape = tuple(attribution.shape)
    if input_is_spec:
        Cc, H, W = (int(v) for v in x.shape[1:])
        forms = {lead + (Cc, H, W): (False, Cc * H * W), lead + (H, W): (True, H * W)}
        names = ("[B,K,C,H,W]", "[B,K,H,W]") if all_classes else ("[B,C,H,W]", "[B,H,W]")
    else:
        Chans, T = int(x.shape[2]), int(x.shape[3])
        forms = {lead + (1, Chans, T): (False, Chans * T), lead + (Chans, T): (False, Chans * T), lead + (1, T): (True, T)}
        names = ("[B,K,1,Chans,T]", "[B,K,Chans,T]", "[B,K,1,T]") if all_classes else ("[B,1,Chans,T]", "[B,Chans,T]", "[B,1,T]")
    if shape not in forms:
        if all_classes and shape in {s[:1] + s[2:] for s in forms}:
            raise ValueError(f"{who}: class_idx='all' needs an attribution with a class axis after B; got {shape}, expected one of "
                             + " or ".join(f"{nm} = {s}" for nm, s in zip(names, forms)))
        raise ValueError(f"{who}: wrong map shape {shape} for input={'spec' if input_is_spec else 'eeg'!r}; expected "
                         + " or ".join(f"{nm} = {s}" for nm, s in zip(names, forms)))
    return forms[shape]


def _infidelity_rows(x, sigma, grouped, N, seed, b0, nb, n0, n, dt, eeg_rows):
    """Rows (b, j), b in b0..b0+nb-1, j in 0..n-1: sample b minus the noise of draw n0 + j.  x fp32 [B,C,H,W] -> internal layout
    [nb*n,H,W,8] in dt (bx_infidelity_rows_spec), or with eeg_rows fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T] (bx_infidelity_rows_eeg)."""
    lib = L.load()
    out, dims = _empty_rows(x, nb * n, dt, eeg_rows)
    B = int(x.shape[0])
    if not eeg_rows:
        L.check(lib.bx_infidelity_rows_spec(_p(x), _p(sigma), _p(out), B, *dims, 1 if grouped else 0, N, b0, nb, n0, n, seed, ops.bx_dtype(dt), _stream()),
                "bx_infidelity_rows_spec")
    else:
        L.check(lib.bx_infidelity_rows_eeg(_p(x), _p(sigma), _p(out), B, *dims, 1 if grouped else 0, N, b0, nb, n0, n, seed, _stream()),
                "bx_infidelity_rows_eeg")
    return out


def infidelity(model, eeg, spec, attribution, *, input="spec", nsamples=10, noise_level=None, stdev=None, normalize=False, class_idx=None, score="prob",
               seed=0, max_batch=256, return_parts=False):
    """Infidelity of an attribution (Yeh et al., NeurIPS 2019; Captum's ``metrics.infidelity`` with Gaussian perturbations): how well the
    attribution predicts the drop of the class score under a small perturbation of the input,
        I[b,k] = sigma[b] * z[b,k],   d = <I, Phi>,   Delta = s_c(x) - s_c(x - I),   infid[b] = mean_k (beta d - Delta)^2
    with z standard normal and s_c the probability (score='logprob': the log-probability) of the explained class.  Small is faithful.

    attribution: the features are its cells.  input='spec': [B,C,H,W] (a cell is an element) or [B,H,W] (a cell is a pixel: one draw moves
                 all its channels -- the maps every method here returns); input='eeg': [B,1,Chans,T] / [B,Chans,T] (elements) or [B,1,T]
                 (a whole time column).  With class_idx='all' it carries a class axis after B, [B,K,...] (K <= 32).  The maps of
                 grad_cam, saliency, smooth_grad, occlusion, rise, kernel_shap ... fit as they are.
    model:       a MultimodalModel; a stand-alone Spectrogram_Model (eeg=None, input='spec'); a stand-alone EEGNet /
                 EEGNetAttentionDeep (spec=None, input='eeg') -- the convention of grad_cam.
    noise_level / stdev: the scale of the perturbation, as in ``smooth_grad``: sigma[b] = noise_level * the sample's range (0.15 when
                 neither is given), or an absolute stdev, a number or one per sample.  Giving both is refused.
    nsamples:    n, the draws per sample.  z is SmoothGrad's stream with the cell as its element: ``smooth_grad_noise((B, *cell_shape),
                 nsamples=n, seed=seed)`` returns exactly these draws; those of (b, k) depend neither on nsamples nor on max_batch.
    normalize:   Captum's scaling: beta[b] = sum_k d Delta / sum_k d^2 (0 when the denominator is 0) makes the result invariant to the
                 scale of the attribution; otherwise beta = 1.
    class_idx:   None = each sample's arg-max class on the clean input; an int; one class per sample; 'all' (``occlusion``'s conventions).
    max_batch:   rows (perturbed inputs) per forward pass; no bit of ``dots`` depends on it.
    (n + 1) * B forward evaluations in eval mode without autograd.  The rows are written straight in the model's layout with the noise
    in registers (bx_infidelity_rows_*); the dot draws the noise again and sums in fp64 in an order that depends on the shapes alone
    (bx_infidelity_dot); bx_infidelity_finish forms the drops, beta and the mean square.  In a MultimodalModel the branch whose input
    does not change runs once per sample.  The training flag and every requires_grad are restored on return.  Returns fp64 [B] (or
    [B,K]) on the device, or ``InfidelityResult`` with return_parts."""
    return _infidelity(model, eeg, spec, attribution, input, nsamples, noise_level, stdev, normalize, class_idx, score, seed, max_batch, return_parts)


def _infidelity(model, eeg, spec, attribution, input, nsamples, noise_level, stdev, normalize, class_idx, score, seed, max_batch, return_parts, profile=None):
    """``infidelity`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'sigma', 'perturb',
    'forward', 'dot', 'finish' -- device events around every phase of the pass (tools/infidelity_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "infidelity"
    call = _Call(who, model).named(input)
    if score not in _FAITH_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    n, seed, max_batch = _draw_count(who, nsamples), _stream_seed(who, seed), _max_batch(who, max_batch)
    x = call.tensors(eeg, spec).x
    if not isinstance(attribution, torch.Tensor):
        raise ValueError(f"{who}: attribution must be a tensor")
    B = _nonempty(who, x)
    is_spec = call.input_is_spec
    _per_cell(who, x, is_spec)
    level, sd = _level_or_absolute(who, B, "noise_level", noise_level, "stdev", stdev, 0.15, True)
    K, Kc, per, cls_h, all_classes = call.explained(class_idx).K, call.Kc, call.per, call.cls_h, call.all_classes
    grouped, cells = _infidelity_cells(who, attribution, x, is_spec, all_classes, K)
    if B * n * K >= 1 << 31 or B * Kc * cells >= 1 << 31 or B * per >= 1 << 31:
        raise ValueError(f"{who}: B * n * K = {B * n * K}, B * Kc * cells = {B * Kc * cells} or B * per = {B * per} beyond 32-bit offsets; use fewer samples per call")
    call.need_gpu("the model, its inputs and the attribution", attribution)

    lib = L.load()
    dev = x.device
    use_logprob = score == "logprob"
    rp = _RowPass(call, 0, torch.zeros(1), max_batch, profile)

    with rp.open():
        with rp.lap("sigma"):
            sigma = _range_scale(rp.xs, level, sd)
        phi = attribution.detach().to(torch.float32).reshape(B, Kc, cells).contiguous()
        with rp.lap("forward"):
            rp.fix_other()
            # the unperturbed input takes the path of the perturbed rows, in chunks of the same size
            clean = torch.empty(B, K, dtype=torch.float32, device=dev)
            for b0, nb in rp.groups():
                clean[b0:b0 + nb] = rp.scores(rp.clean_rows(b0, nb), b0, nb, logprob=use_logprob)
        classes = _class_tensor(cls_h, all_classes, clean, dev)
        S = rp.sweep(n, lambda *chunk: _infidelity_rows(rp.xs, sigma, grouped, n, seed, *chunk, rp.dt, not is_spec), logprob=use_logprob)
        with rp.lap("dot"):
            dots = torch.empty(B, Kc, n, dtype=torch.float64, device=dev)
            L.check(lib.bx_infidelity_dot(_p(phi), _p(sigma), _p(dots), B, n, cells, Kc, seed, 0, B * n, _stream()), "bx_infidelity_dot")
        with rp.lap("finish"):
            infid = torch.empty(B, Kc, dtype=torch.float64, device=dev)
            beta, drops = torch.empty_like(infid), torch.empty_like(dots)
            L.check(lib.bx_infidelity_finish(_p(dots), _p(S), _p(clean), _p(classes), _p(infid), _p(beta), _p(drops), B, n, K, 1 if normalize else 0,
                                             _stream()), "bx_infidelity_finish")
    if not all_classes:
        infid, beta, dots, drops = infid[:, 0], beta[:, 0], dots[:, 0], drops[:, 0]
    if not return_parts:
        return infid
    return InfidelityResult(infid, beta, dots, drops, clean, None if classes is None else classes.long(), sigma, n, seed)


def _sensitivity_explain(who, explain, eeg_rows, spec_rows, sample, trail):
    """One call of the explanation function -> fp32 [rows, P] contiguous and its trailing shape, which must equal ``trail`` if given."""
    rows = int(sample.shape[0])
    phi = explain(eeg_rows, spec_rows, sample)
    if not isinstance(phi, torch.Tensor) or not phi.is_cuda or phi.dim() < 2 or int(phi.shape[0]) != rows or not phi.dtype.is_floating_point:
        raise ValueError(f"{who}: explain must return a floating-point device tensor [rows, ...] with rows = {rows}, got "
                         + (f"{tuple(phi.shape)} {phi.dtype} on {phi.device}" if isinstance(phi, torch.Tensor) else type(phi).__name__))
    if trail is not None and tuple(phi.shape[1:]) != trail:
        raise ValueError(f"{who}: explain returned the trailing shape {tuple(phi.shape[1:])}, the clean call returned {trail}")
    return phi.detach().to(torch.float32).reshape(rows, -1).contiguous(), tuple(phi.shape[1:])


def sensitivity_max(explain, eeg, spec, *, input="spec", nsamples=10, radius=None, radius_level=None, seed=0, max_batch=256, return_parts=False):
    """Max-sensitivity of an explanation function (Yeh et al., NeurIPS 2019; Captum's ``metrics.sensitivity_max``): how far the
    explanation moves, relative to its norm, when the input moves inside a small L-infinity ball,
        sens[b] = max_k || Phi(x[b] + r[b] * u[b,k]) - Phi(x[b]) ||_2 / || Phi(x[b]) ||_2,   u uniform in [-1, 1) per element
    (the denominator is 1 when the norm is 0, Captum's rule).  Small is stable.

    explain:     ``explain(eeg_rows, spec_rows, sample)`` -> a floating-point device tensor [rows, ...]: any of the package's attribution
                 calls behind a lambda.  ``sample`` is int64 [rows] on the device and names the sample each row perturbs, so that a caller
                 can pass ``class_idx=cls[sample]``; the input that is not perturbed is repeated per row (None stays None, for a
                 stand-alone model).  It is called once on the clean batch, then on chunks of at most max_batch rows; the trailing
                 shape of its result must be the same on every call.
    input:       'spec': the spectrogram [B,C,H,W] is perturbed; 'eeg': the EEG input [B,1,Chans,T].  Rows are fp32 in the input's own
                 layout, always perturbed element by element.
    radius / radius_level: r[b]: an absolute radius, a number or one per sample (tensor [B]); or radius_level times the sample's range
                 (bx_smoothgrad_sigma).  radius_level = 0.02 when neither is given; giving both is refused.
    nsamples:    n, the draws per sample, from Philox4x32-10 counters (element, draw, sample, 1) keyed by ``seed``: a stream apart from
                 smooth_grad's; the draws of (b, k) depend neither on nsamples nor on max_batch.
    The rows of a chunk are written by one launch (bx_sensitivity_rows), the distances are fp64 sums in fixed order, one workgroup per row
    (bx_sensitivity_dist; the norms of the clean explanation are the same kernel without a second operand), bx_sensitivity_finish takes
    the maximum and divides.  Returns fp64 [B] on the device, or ``SensitivityResult`` with return_parts."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "sensitivity_max"
    if not callable(explain):
        raise ValueError(f"{who}: explain must be a callable (eeg_rows, spec_rows, sample) -> tensor, got {type(explain).__name__}")
    record = _Call(who, None).named(input)                          # a function is explained: there is no model to check
    n, seed, max_batch = _draw_count(who, nsamples), _stream_seed(who, seed), _max_batch(who, max_batch)
    x, other = record.tensors(eeg, spec).x, record.other
    B = _nonempty(who, x)
    level, rad = _level_or_absolute(who, B, "radius_level", radius_level, "radius", radius, 0.02, False)
    if other is not None and (not isinstance(other, torch.Tensor) or other.shape[0] != B):
        raise ValueError(f"{who}: the other input must be None or a tensor with the same batch size")
    per = record.per
    if B * n >= 1 << 31 or B * per >= 1 << 31:
        raise ValueError(f"{who}: B * n = {B * n} or B * per = {B * per} beyond 32-bit offsets; use fewer samples per call")
    if not (x.is_cuda and (other is None or other.is_cuda)):
        raise RuntimeError(f"brainxai.{who}: the inputs must live on the GPU; there is no CPU path")

    lib = L.load()
    dev = x.device
    total = B * n
    max_rows = max(1, min(max_batch, ((1 << 31) - 1) // per))

    def call(rows_x, sample, trail):
        """explain on rows of the perturbed input; the other input is the clean batch itself (trail None) or repeated per row"""
        o = other if other is None or trail is None else other.index_select(0, sample)
        return _sensitivity_explain(who, explain, *((o, rows_x) if input == "spec" else (rows_x, o)), sample, trail)

    with torch.cuda.device(dev):
        xs = x.detach().to(torch.float32).contiguous()
        r = _range_scale(xs, level, rad)
        phi0, trail = call(xs, torch.arange(B, dtype=torch.int64, device=dev), None)
        P = int(phi0.shape[1])
        if P < 1 or B * P >= 1 << 31:
            raise ValueError(f"{who}: explain returned {P} values per row; B * P must stay within 1..2^31 - 1")
        norms = torch.empty(B, dtype=torch.float64, device=dev)
        L.check(lib.bx_sensitivity_dist(_p(phi0), None, _p(norms), B, 1, P, 0, B, _stream()), "bx_sensitivity_dist")
        dist = torch.empty(total, dtype=torch.float64, device=dev)
        max_rows = max(1, min(max_rows, ((1 << 31) - 1) // P))
        for row0, rows in _sample_chunks(total, max_rows):
            rx = torch.empty(rows, *xs.shape[1:], dtype=torch.float32, device=dev)
            L.check(lib.bx_sensitivity_rows(_p(xs), _p(r), _p(rx), B, n, per, seed, row0, rows, _stream()), "bx_sensitivity_rows")
            phi, _ = call(rx, _sample_of(row0, rows, n, dev), trail)
            L.check(lib.bx_sensitivity_dist(_p(phi), _p(phi0), _p(dist[row0:row0 + rows]), B, n, P, row0, rows, _stream()), "bx_sensitivity_dist")
            del phi, rx
        sens = torch.empty(B, dtype=torch.float64, device=dev)
        L.check(lib.bx_sensitivity_finish(_p(dist), _p(norms), _p(sens), B, n, _stream()), "bx_sensitivity_finish")
    if not return_parts:
        return sens
    return SensitivityResult(sens, dist.reshape(B, n), norms, r, n, seed)


# ---- similarity of two maps and the model parameter randomization test ------------------------------------------------------------------
_SIM_METRICS = ("spearman", "pearson", "ssim", "topk")
_SIM_WINDOWS = ("uniform", "gaussian")
_SIM_ORDERS = ("cascade", "independent")

MapSimilarityResult = collections.namedtuple("MapSimilarityResult", "spearman pearson ssim topk ranks_a ranks_b k lo hi args",
                                             defaults=(None,) * 10)
MapSimilarityResult.__doc__ = """What ``map_similarity`` returns: ``spearman``, ``pearson``, ``ssim``, ``topk`` fp64 tensors of the maps' leading shape on the
device (None for a metric that was not asked for).  With return_parts also ``ranks_a`` / ``ranks_b`` (the tie-averaged ranks, fp32, the
maps' shape; None without 'spearman'), ``k`` (the top-k count; None without 'topk'), ``lo`` / ``hi`` (fp32 [2, *leading]: the extremes of
a and of b that SSIM rescaled by; None with a data_range or without 'ssim') and ``args`` (the options as a dict)."""

RandomizationResult = collections.namedtuple("RandomizationResult", "layers similarity original maps order seed")
RandomizationResult.__doc__ = """What ``randomization_test`` returns: ``layers`` (the names, output first; a group is a tuple), ``similarity`` {metric:
fp64 [*leading, n]} on the device (stage s compares the original map with the map after layer s was re-initialised), ``original`` (the
map of the trained model), ``maps`` (the n stage maps with keep_maps, else None), ``order`` and ``seed`` as given."""


def _sim_taps(window, win):
    """fp64 [win]: 1 / win, or the taps of scipy.ndimage.gaussian_filter1d(sigma=1.5, truncate=3.5) (radius 5)."""
    if window == "uniform":
        return np.full(win, 1.0 / win, dtype=np.float64)
    t = np.arange(-(win // 2), win // 2 + 1)
    phi = np.exp(-0.5 / (1.5 * 1.5) * t ** 2)
    return phi / phi.sum()


def _sim_options(who, shape, metrics, window, win_size, data_range, topk):
    """Everything about the options that can be refused, refused; -> (metrics, H, W, N, win, cov_norm, k)."""
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in _SIM_METRICS]
    if bad or not metrics:
        raise ValueError(f"{who}: unknown metric {bad[0] if bad else metrics!r}; use any of {_SIM_METRICS}")
    if len(shape) < 2:
        raise ValueError(f"{who}: a map needs at least two axes, [..., H, W]; got the shape {tuple(shape)}")
    H, W = int(shape[-2]), int(shape[-1])
    N = H * W
    if not 1 <= N <= _FAITH_MAX_N or any(int(v) < 1 for v in shape):
        raise ValueError(f"{who}: {N} cells per map (shape {tuple(shape)}), supported 1..{_FAITH_MAX_N}")
    win = cov = k = None
    if "ssim" in metrics:
        if window not in _SIM_WINDOWS:
            raise ValueError(f"{who}: unknown window {window!r}; use 'uniform' or 'gaussian'")
        if window == "gaussian":
            if win_size is not None:
                raise ValueError(f"{who}: win_size is fixed by window='gaussian' (sigma 1.5, truncate 3.5: 11); do not pass it")
            win = 11
        else:
            win = 7 if win_size is None else win_size
            if not isinstance(win, numbers.Integral) or isinstance(win, bool) or win < 1 or win % 2 == 0:
                raise ValueError(f"{who}: win_size must be an odd int >= 1, got {win_size!r}")
            win = int(win)
        if win > L.BX_SSIM_MAX_WIN:
            raise ValueError(f"{who}: win_size = {win}, supported 1..{L.BX_SSIM_MAX_WIN}")
        filtered = [v for v in (H, W) if v > 1]
        if not filtered:
            raise ValueError(f"{who}: ssim of a map of one cell is not defined")
        if min(filtered) < win:
            raise ValueError(f"{who}: win_size = {win} exceeds a filtered axis of the map [{H}, {W}]")
        NP = win ** len(filtered)
        if window == "uniform" and NP < 2:
            raise ValueError(f"{who}: the uniform window needs win_size >= 3 (the sample covariance of one cell is not defined)")
        cov = NP / (NP - 1.0) if window == "uniform" else 1.0
        if data_range is not None and (not isinstance(data_range, numbers.Real) or isinstance(data_range, bool) or not 0 < float(data_range) < math.inf):
            raise ValueError(f"{who}: data_range must be None or a finite number > 0, got {data_range!r}")
        if len(filtered) == 2 and H * 4 > 1624:
            raise ValueError(f"{who}: ssim supports maps of at most 406 rows, got [{H}, {W}]")
    if "topk" in metrics:
        if isinstance(topk, bool) or not isinstance(topk, numbers.Real):
            raise ValueError(f"{who}: topk must be a fraction in (0, 1] or an int in 1..N, got {topk!r}")
        if isinstance(topk, numbers.Integral):
            if not 1 <= topk <= N:
                raise ValueError(f"{who}: topk = {topk} outside 1..N = {N}")
            k = int(topk)
        else:
            if not 0 < float(topk) <= 1:
                raise ValueError(f"{who}: the fraction topk = {topk!r} lies outside (0, 1]")
            k = min(N, max(1, math.ceil(float(topk) * N)))
    return metrics, H, W, N, win, cov, k


class _SimMap:
    """One map tensor [*leading, H, W] as fp32 rows [R,N] on the device, with what the metrics need of it computed once: the stable
    ranks, the tie-averaged ranks and the extremes."""

    def __init__(self, t, abs):
        self.lead = tuple(t.shape[:-2])
        self.R = int(np.prod(self.lead, dtype=np.int64)) if self.lead else 1
        self.N = int(t.shape[-2]) * int(t.shape[-1])
        self.shape = tuple(t.shape)
        self.v = t.detach().to(torch.float32).reshape(self.R, self.N).contiguous()
        self.abs = 1 if abs else 0
        self._ranks = self._avg = self._range = None

    def ranks(self):
        if self._ranks is None:
            lib, v = L.load(), self.v
            if self.abs:                                              # bx_rank_desc has no flag: it ranks a copy of |v|
                v = torch.empty_like(self.v)
                L.check(lib.bx_abs(_p(self.v), _p(v), self.v.numel(), _stream()), "bx_abs")
            self._ranks = torch.empty(self.R, self.N, dtype=torch.int32, device=v.device)
            nbytes = lib.bx_rank_desc_workspace(self.R, self.N)
            if nbytes == 0:
                L.check(-1, "bx_rank_desc_workspace")
            ws = torch.empty(nbytes // 4, dtype=torch.int32, device=v.device)
            L.check(lib.bx_rank_desc(_p(v), _p(self._ranks), self.R, self.N, _p(ws), nbytes, _stream()), "bx_rank_desc")
        return self._ranks

    def average_ranks(self):
        if self._avg is None:
            lib, ranks = L.load(), self.ranks()
            self._avg = torch.empty(self.R, self.N, dtype=torch.float32, device=self.v.device)
            nbytes = lib.bx_rank_average_workspace(self.R, self.N)
            if nbytes == 0:
                L.check(-1, "bx_rank_average_workspace")
            ws = torch.empty(nbytes // 4, dtype=torch.int32, device=self.v.device)
            L.check(lib.bx_rank_average(_p(self.v), _p(ranks), _p(self._avg), self.R, self.N, self.abs, _p(ws), nbytes, _stream()), "bx_rank_average")
        return self._avg

    def extremes(self):
        if self._range is None:
            lo = torch.empty(self.R, dtype=torch.float32, device=self.v.device)
            hi = torch.empty_like(lo)
            L.check(L.load().bx_row_minmax(_p(self.v), _p(lo), _p(hi), self.R, self.N, self.abs, _stream()), "bx_row_minmax")
            self._range = (lo, hi)
        return self._range


def _sim_metric(metric, A, B, H, W, win, cov, k, taps_d, data_range):
    """fp64 [*leading] of one metric for two prepared maps."""
    lib = L.load()
    out = torch.empty(A.R, dtype=torch.float64, device=A.v.device)
    if metric == "pearson":
        L.check(lib.bx_map_corr(_p(A.v), _p(B.v), _p(out), A.R, A.N, A.abs, _stream()), "bx_map_corr")
    elif metric == "spearman":
        L.check(lib.bx_map_corr(_p(A.average_ranks()), _p(B.average_ranks()), _p(out), A.R, A.N, 0, _stream()), "bx_map_corr")
    elif metric == "topk":
        L.check(lib.bx_topk_overlap(_p(A.ranks()), _p(B.ranks()), _p(out), A.R, A.N, k, _stream()), "bx_topk_overlap")
    else:
        rng = (None,) * 4 if data_range is not None else A.extremes() + B.extremes()
        nbytes = lib.bx_ssim_rows_workspace(A.R, H, W, win)
        if nbytes == 0:
            L.check(-1, "bx_ssim_rows_workspace")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=A.v.device)
        L.check(lib.bx_ssim_rows(_p(A.v), _p(B.v), _p(taps_d), *(_p(t) for t in rng), 1.0 if data_range is None else float(data_range), cov, _p(out),
                                 A.R, H, W, win, A.abs, _p(ws), nbytes, _stream()), "bx_ssim_rows")
    return out.reshape(A.lead)


def _sim_check_maps(who, maps):
    first = maps[0]
    for t in maps:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: the maps must be tensors, got {type(t).__name__}")
        if tuple(t.shape) != tuple(first.shape):
            raise ValueError(f"{who}: the maps must have equal shapes, got {tuple(first.shape)} and {tuple(t.shape)}")
        if not t.dtype.is_floating_point:
            raise ValueError(f"{who}: the maps must be floating-point tensors, got {t.dtype}")


def _sim_need_gpu(who, maps):
    if not all(t.is_cuda for t in maps):
        raise RuntimeError(f"brainxai.{who}: the maps must live on the GPU; there is no CPU path")
    if len({t.device for t in maps}) != 1:
        raise ValueError(f"{who}: the maps live on different devices")
    R = maps[0].numel() // (int(maps[0].shape[-2]) * int(maps[0].shape[-1]))
    if R > 65535 or maps[0].numel() >= 1 << 31:
        raise ValueError(f"{who}: {R} maps per call, supported 1..65535 (and fewer than 2^31 cells in all)")


def map_similarity(a, b, *, metrics=_SIM_METRICS, abs=False, window="uniform", win_size=None, data_range=None, topk=0.1, return_parts=False):
    """How alike two attribution maps are, by the measures of Adebayo et al. ("Sanity Checks for Saliency Maps", NeurIPS 2018) and
    Ghorbani et al. (AAAI 2019): Spearman's rank correlation, Pearson's correlation, the mean structural similarity and the overlap of
    the top-k cells.  Everything runs on the device; only the result leaves it.

    a, b:        fp32 device tensors of equal shape [..., H, W]: the last two axes are the map ([H,W], [Chans,T] or [1,T]), all leading
                 axes are batch, so [B,H,W] and the class-axis form [B,K,H,W] fit as the package returns them.  1 <= H * W < 2^20.
    metrics:     any of 'spearman', 'pearson', 'ssim', 'topk'.
    abs:         compare |a| and |b| (Adebayo et al. report both forms); the modulus is taken in registers.
    spearman:    Pearson's correlation of the tie-averaged ranks, ``scipy.stats.spearmanr``; the keys are ``attribution_ranks``'s (NaN
                 counts as -inf, -0.0 equals +0.0).  NaN for a constant map, as scipy returns.
    pearson:     fp64, two passes, in an order that depends on H * W alone (``scipy.stats.pearsonr``).
    topk:        |{cells among the k largest of both maps}| / k over the stable ranks; k = max(1, ceil(topk * N)) for a fraction in
                 (0, 1], topk itself for an int.
    ssim:        the mean SSIM of scikit-image's ``structural_similarity`` over the positions whose window lies inside the map.
                 window='uniform': win_size (odd, default 7) equal taps and the sample covariance -- skimage's defaults;
                 window='gaussian': sigma 1.5 truncated at 3.5 sigma (11 taps) and the population covariance -- Wang et al.'s setting
                 (skimage's gaussian_weights=True, use_sample_covariance=False).  An axis of extent 1 is not filtered: [1,T] maps get
                 1-D SSIM.  data_range=None rescales each map to [0, 1] by its own extremes first (a constant map becomes zeros), the
                 procedure of Adebayo et al.; a number compares the raw values with that dynamic range.  A filtered axis shorter
                 than the window is refused, as skimage does; with two filtered axes H <= 406.
    Returns ``MapSimilarityResult``: one fp64 tensor of the leading shape per requested metric."""
    who = "map_similarity"
    _sim_check_maps(who, [a, b])
    metrics, H, W, N, win, cov, k = _sim_options(who, a.shape, metrics, window, win_size, data_range, topk)
    _sim_need_gpu(who, [a, b])
    with torch.cuda.device(a.device):
        A, B = _SimMap(a, abs), _SimMap(b, abs)
        taps_d = torch.from_numpy(_sim_taps(window, win)).to(a.device) if "ssim" in metrics else None
        vals = {m: _sim_metric(m, A, B, H, W, win, cov, k, taps_d, data_range) for m in metrics}
        if not return_parts:
            return MapSimilarityResult(**vals)
        parts = dict(k=k, args=dict(metrics=metrics, abs=bool(abs), window=window, win_size=win, data_range=data_range, topk=topk))
        if "spearman" in metrics:
            parts.update(ranks_a=A.average_ranks().reshape(A.shape), ranks_b=B.average_ranks().reshape(A.shape))
        if "ssim" in metrics and data_range is None:
            (la, ha), (lb, hb) = A.extremes(), B.extremes()
            parts.update(lo=torch.stack([la, lb]).reshape(2, *A.lead), hi=torch.stack([ha, hb]).reshape(2, *A.lead))
    return MapSimilarityResult(**vals, **parts)


def agreement_matrix(maps, *, metric="spearman", abs=False, window="uniform", win_size=None, data_range=None, topk=0.1):
    """The "do my methods agree" table: ``metric`` of ``map_similarity`` for every pair of the maps {name: tensor [..., H, W]}, all of one
    shape.  Each map is ranked once and each pair compared once; the matrix is symmetric with a unit diagonal.
    Returns (fp64 [M, M, *leading] on the device, the names in the dict's order); entry [i, j] equals
    ``map_similarity(maps[i], maps[j], metrics=(metric,), ...)`` bit for bit."""
    who = "agreement_matrix"
    if not isinstance(maps, dict) or not maps:
        raise ValueError(f"{who}: maps must be a non-empty dict name -> tensor")
    if not isinstance(metric, str):
        raise ValueError(f"{who}: metric must be one name, got {metric!r}")
    names, tensors = list(maps), list(maps.values())
    _sim_check_maps(who, tensors)
    _, H, W, N, win, cov, k = _sim_options(who, tensors[0].shape, (metric,), window, win_size, data_range, topk)
    _sim_need_gpu(who, tensors)
    dev = tensors[0].device
    with torch.cuda.device(dev):
        prepared = [_SimMap(t, abs) for t in tensors]
        taps_d = torch.from_numpy(_sim_taps(window, win)).to(dev) if metric == "ssim" else None
        M = len(names)
        out = torch.ones(M, M, *prepared[0].lead, dtype=torch.float64, device=dev)
        for i in range(M):
            for j in range(i + 1, M):
                out[i, j] = _sim_metric(metric, prepared[i], prepared[j], H, W, win, cov, k, taps_d, data_range)
                out[j, i] = out[i, j]
    return out, names


def _rand_branch(prefix, net):
    """The stages of a stand-alone branch, output first; a convolution brings the BatchNorm that follows it."""
    from . import models as M
    p = prefix + "." if prefix else ""
    if isinstance(net, M.Spectrogram_Model):
        return [p + "fc"] + [f"{p}block{i}" for i in range(5, 0, -1)]
    trunk = [(p + "separableConv", p + "batchnorm3"), (p + "depthwiseConv", p + "batchnorm2"), (p + "conv1", p + "batchnorm1")]
    if isinstance(net, M.EEGNetAttentionDeep):
        return [p + "dense2", p + "dense1", p + "attention_layer", (p + "conv2", p + "batchnorm4")] + trunk
    if isinstance(net, M.EEGNet):
        return [p + "dense"] + trunk
    raise ValueError(f"randomization_layers: no default layer list for a {type(net).__name__}; pass layers=")


def randomization_layers(model, input="spec"):
    """The default stages of ``randomization_test``, output first: for a MultimodalModel ``fc2``, ``fc1``, then the explained branch's
    head and stages from last to first (the other branch is not touched); for a stand-alone branch its own list.  An entry is a dotted
    module name, or a tuple of names re-initialised together (a convolution of the EEG nets with the BatchNorm that follows it)."""
    from . import models as M
    if input not in _FAITH_INPUTS:
        raise ValueError(f"randomization_layers: unknown input {input!r}; use 'spec' or 'eeg'")
    if isinstance(model, M.MultimodalModel):
        return ["fc2", "fc1"] + (_rand_branch("spectrogram_model", model.spectrogram_model) if input == "spec" else _rand_branch("eeg_model", model.eeg_model))
    if isinstance(model, M.Spectrogram_Model) != (input == "spec"):
        raise ValueError(f"randomization_layers: input={input!r} does not fit a stand-alone {type(model).__name__}")
    return _rand_branch("", model)


def _rand_fan_in(weight):
    """torch.nn.init._calculate_fan_in_and_fan_out's fan_in: the input features times the receptive field."""
    return int(weight.shape[1]) * int(np.prod(weight.shape[2:], dtype=np.int64))


def _rand_plan(who, model, layers):
    """-> per layer the list of actions ('uniform', tensor, bound, j) / ('fill', tensor, value) and the list of every tensor the layer
    owns.  j is the parameter's position in the layer's named_parameters() (a group: its modules' lists one after the other)."""
    plans = []
    seen = set()
    for layer in layers:
        names = (layer,) if isinstance(layer, str) else tuple(layer)
        if not names or not all(isinstance(n, str) for n in names):
            raise ValueError(f"{who}: a layer is a dotted module name or a tuple of names, got {layer!r}")
        mods = []
        for n in names:
            try:
                mods.append(_resolve(model, n))
            except AttributeError:
                raise ValueError(f"{who}: unknown layer {n!r}: the model has no such module") from None
            if not isinstance(mods[-1], torch.nn.Module):
                raise ValueError(f"{who}: unknown layer {n!r}: not a module")
        position = {}
        for m in mods:
            for _, q in m.named_parameters():
                position.setdefault(id(q), len(position))
        actions, owned = [], []
        for m in mods:
            for sub in m.modules():
                own = list(sub.parameters(recurse=False))
                if isinstance(sub, (torch.nn.Conv2d, torch.nn.Linear)):
                    bound = 1.0 / math.sqrt(_rand_fan_in(sub.weight))
                    actions += [("uniform", q, bound, position[id(q)]) for q in (sub.weight, sub.bias) if q is not None]
                elif isinstance(sub, torch.nn.modules.batchnorm._BatchNorm):
                    actions += [("fill", t, v) for t, v in ((sub.weight, 1.0), (sub.bias, 0.0), (sub.running_mean, 0.0), (sub.running_var, 1.0),
                                                            (sub.num_batches_tracked, 0)) if t is not None]
                elif own:
                    raise ValueError(f"{who}: layer {layer!r} holds parameters of a {type(sub).__name__}; only Conv2d, Linear and BatchNorm are re-initialised")
                owned += own + list(sub.buffers(recurse=False))
        if not actions:
            raise ValueError(f"{who}: layer {layer!r} has no parameters to re-initialise")
        for t in owned:
            if id(t) in seen:
                raise ValueError(f"{who}: layer {layer!r} repeats a tensor of an earlier layer")
            seen.add(id(t))
        for a in actions:
            if a[0] == "uniform" and a[1].dtype != torch.float32:
                raise ValueError(f"{who}: layer {layer!r} has a {a[1].dtype} parameter; parameters must be float32")
        plans.append((actions, owned))
    return plans


def _rand_apply(actions, seed, stage):
    lib = L.load()
    for a in actions:
        if a[0] == "uniform":
            _, q, bound, j = a
            t = q.data
            if not t.is_contiguous():
                raise ValueError("randomization_test: a parameter is not contiguous")
            L.check(lib.bx_param_uniform(_p(t), t.numel(), bound, seed, j, stage, _stream()), "bx_param_uniform")
        else:
            a[1].data.fill_(a[2])
    ops.bump_param_epoch()                                # the writes bump no version counter: packed weights are stale from here


def _rand_restore(saved):
    for t, copy in saved:
        t.data.copy_(copy)
    ops.bump_param_epoch()


def randomization_test(model, explain, eeg, spec, *, input="spec", layers=None, order="cascade", metrics=("spearman", "ssim"), abs=False, seed=0,
                       keep_maps=False, window="uniform", win_size=None, data_range=None, topk=0.1):
    """The model parameter randomization test of Adebayo et al. ("Sanity Checks for Saliency Maps", NeurIPS 2018): the weights are
    re-initialised layer by layer from the output towards the input, after each stage the map is recomputed and compared with the map of
    the trained model.  A method whose maps do not change does not explain the model.

    explain:     ``explain(model, eeg, spec)`` -> a map tensor as ``map_similarity`` accepts it: any of the package's attribution calls
                 behind a lambda, e.g. ``lambda m, e, s: brainxai.grad_cam(m, e, s)``.
    layers:      dotted module names, output first; a tuple of names is one stage.  Default ``randomization_layers(model, input)``.
    order:       'cascade': stage s has layers 0..s re-initialised; 'independent': layer s alone, the rest keeps its trained values.
                 A layer's draws do not depend on the order.
    metrics, abs, window, win_size, data_range, topk: ``map_similarity``'s.
    Re-initialisation, deterministic in ``seed``: every Conv2d / Linear weight and bias of the layer gets fl32(bound * u), bound =
    1 / sqrt(fan_in) (torch's default kaiming_uniform_(a=sqrt(5)) and its bias bound), u uniform in [-1, 1) from Philox4x32-10 counters
    (element >> 2, j, s, 2) keyed by seed -- j the tensor's position in the layer's named_parameters(), s the layer's position in
    ``layers`` (bx_param_uniform); BatchNorm gets weight 1, bias 0, running mean 0, running variance 1 and num_batches_tracked 0.
    Every parameter and buffer of the listed modules is copied on the device first and restored bit for bit in a ``finally``; the
    parameter epoch is bumped after every write (ops.bump_param_epoch), so ``pack_reuse`` scopes and a ``GradCamSweep`` repack.
    Returns ``RandomizationResult``."""
    who = "randomization_test"
    if not callable(explain):
        raise ValueError(f"{who}: explain must be a callable (model, eeg, spec) -> tensor, got {type(explain).__name__}")
    if input not in _FAITH_INPUTS:
        raise ValueError(f"{who}: unknown input {input!r}; use 'spec' or 'eeg'")
    if order not in _SIM_ORDERS:
        raise ValueError(f"{who}: unknown order {order!r}; use 'cascade' or 'independent'")
    seed = _stream_seed(who, seed)
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in _SIM_METRICS]
    if bad or not metrics:
        raise ValueError(f"{who}: unknown metric {bad[0] if bad else metrics!r}; use any of {_SIM_METRICS}")
    layers = list(randomization_layers(model, input) if layers is None else layers)
    if not layers:
        raise ValueError(f"{who}: layers is empty")
    plans = _rand_plan(who, model, layers)
    if not all(t.is_cuda for _, owned in plans for t in owned):
        raise RuntimeError(f"brainxai.{who}: the model must live on the GPU; there is no CPU path")
    options = dict(metrics=metrics, abs=abs, window=window, win_size=win_size, data_range=data_range, topk=topk)

    phi0 = explain(model, eeg, spec)
    if not isinstance(phi0, torch.Tensor):
        raise ValueError(f"{who}: explain must return a tensor, got {type(phi0).__name__}")
    _sim_check_maps(who, [phi0])
    _sim_options(who, phi0.shape, **{k: v for k, v in options.items() if k != "abs"})
    phi0 = phi0.detach().clone()
    sims = {m: [] for m in metrics}
    maps = [] if keep_maps else None
    with torch.cuda.device(phi0.device):
        saved = [[(t, t.detach().clone()) for t in owned] for _, owned in plans]
        try:
            for s, (actions, _) in enumerate(plans):
                if order == "independent" and s > 0:
                    _rand_restore(saved[s - 1])
                _rand_apply(actions, seed, s)
                phi = explain(model, eeg, spec)
                if not isinstance(phi, torch.Tensor) or tuple(phi.shape) != tuple(phi0.shape):
                    raise ValueError(f"{who}: explain returned {tuple(phi.shape) if isinstance(phi, torch.Tensor) else type(phi).__name__} at stage {s}, "
                                     f"{tuple(phi0.shape)} for the trained model")
                res = map_similarity(phi0, phi, **options)
                for m in metrics:
                    sims[m].append(getattr(res, m))
                if keep_maps:
                    maps.append(phi.detach().clone())
        finally:
            _rand_restore([pair for group in saved for pair in group])
    return RandomizationResult(layers, {m: torch.stack(v, dim=-1) for m, v in sims.items()}, phi0, maps, order, seed)


# ------------------------------------------------------------------------------------------------
# Fusion SHAP: the exact Shapley values of the votes (log-probabilities) the two branches hand to the fusion head.  The definition is
# pinned in include/brainxai.h; tests/fusion_shap_ref.py restates it.
_FUSION_MAX_M = 16
_FUSION_SCORES = {"prob": L.BX_FUSION_SCORE_PROB, "logprob": L.BX_FUSION_SCORE_LOGPROB}
FusionVotes = collections.namedtuple("FusionVotes", "e s")
FusionVotes.__doc__ = """The two branches' votes of N samples: ``e`` (EEG) and ``s`` (spectrogram), fp32 [N,K] log-probabilities each, on the device.
``fusion_votes`` returns one; ``fusion_shap`` takes one as its background, so a background set runs through the branches once."""
FusionShapResult = collections.namedtuple("FusionShapResult", "values modality interaction v classes clean empty votes background players masks score")
FusionShapResult.__doc__ = """What ``fusion_shap(..., return_parts=True)`` returns: ``values`` fp64 [B,M] or [B,K,M] (what the plain call returns), ``modality`` fp64
[B(,K),2] (the M = 2 game of the EEG votes against the spectrogram votes, (EEG, spec); not the sum of the members' values of a finer game),
``interaction`` fp64 [B(,K)] = v(all) - v(EEG) - v(spec) + v(none), ``v`` fp64 [B,2^M,K] (the value of every class under every coalition
of the players, coalition = the integer whose bit i is player i), ``classes`` int64 [B] (None for class_idx='all'), ``clean`` / ``empty`` fp64
[B,K] = v(all) / v(none) (the scores of the samples and the mean scores of the background rows), ``votes`` and ``background`` (the
samples' and the background's ``FusionVotes``), all on the device; ``players`` (a list of M lists of votes, vote i < K = the EEG branch's
i-th, vote K + i = the spectrogram branch's), ``masks`` uint32 [2^M] (bit i = vote i comes from the sample) on the host; ``score`` as given."""


def shapley_weights(M):
    """fp64 [M] on the host: weights[s] = s! (M - s - 1)! / M!, the weight of a coalition of size s in a game of M players (each exact
    integer quotient rounded once).  Summed over the 2^(M-1) coalitions without a player they give 1."""
    if isinstance(M, bool) or not isinstance(M, numbers.Integral) or not 1 <= int(M) <= _FUSION_MAX_M:
        raise ValueError(f"shapley_weights: M must be an int in 1..{_FUSION_MAX_M}, got {M!r}")
    M = int(M)
    return np.array([math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) for s in range(M)], dtype=np.float64)


def _fusion_players(who, players, K):
    """-> the players as a list of M lists of votes (vote i < K: the EEG branch's i-th, vote K + i: the spectrogram branch's)."""
    if isinstance(players, str):
        if players == "modality":
            return [list(range(K)), list(range(K, 2 * K))]
        if players == "class":
            if K > _FUSION_MAX_M:
                raise ValueError(f"{who}: players='class' has {K} players, more than {_FUSION_MAX_M}; use 'modality' or an explicit partition")
            return [[c, K + c] for c in range(K)]
        if players == "votes":
            if 2 * K > _FUSION_MAX_M:
                raise ValueError(f"{who}: players='votes' has 2K = {2 * K} players, more than {_FUSION_MAX_M}; use 'modality' or 'class'")
            return [[i] for i in range(2 * K)]
        raise ValueError(f"{who}: unknown players {players!r}; use 'votes', 'modality', 'class' or a partition of range({2 * K})")
    try:
        groups = [[v for v in grp] for grp in players]
    except TypeError:
        raise ValueError(f"{who}: players must be 'votes', 'modality', 'class' or a list of lists of votes") from None
    if not 1 <= len(groups) <= _FUSION_MAX_M:
        raise ValueError(f"{who}: {len(groups)} players, supported 1..{_FUSION_MAX_M}")
    seen = set()
    for grp in groups:
        if not grp:
            raise ValueError(f"{who}: an empty player")
        for vt in grp:
            if isinstance(vt, bool) or not isinstance(vt, numbers.Integral) or not 0 <= int(vt) < 2 * K:
                raise ValueError(f"{who}: vote {vt!r} outside range({2 * K})")
            if int(vt) in seen:
                raise ValueError(f"{who}: vote {int(vt)} belongs to two players")
            seen.add(int(vt))
    if len(seen) != 2 * K:
        raise ValueError(f"{who}: the players leave out the votes {sorted(set(range(2 * K)) - seen)}")
    return [[int(vt) for vt in grp] for grp in groups]


def _fusion_masks(groups, K):
    """uint32 [2^M + 4] on the host: the vote mask of every coalition of the M players, coalition = the integer whose bit i is player
    i, then the four masks of the modality game (none, EEG, spec, all) -- ordinary entries of the one list the kernel walks."""
    M = len(groups)
    gm = [sum(1 << vt for vt in grp) for grp in groups]
    S = np.arange(1 << M, dtype=np.uint64)
    masks = np.zeros(1 << M, dtype=np.uint64)
    for i in range(M):
        masks |= ((S >> np.uint64(i)) & np.uint64(1)) * np.uint64(gm[i])
    e_half = (1 << K) - 1
    return np.concatenate([masks, np.array([0, e_half, e_half << K, e_half | e_half << K], dtype=np.uint64)]).astype(np.uint32)


def _fusion_head(who, model):
    """-> (K, Hd) of a MultimodalModel with the reference's head, cat -> Linear(2K,Hd) -> ReLU -> Linear(Hd,K) -> LogSoftmax; anything
    else is refused."""
    lin = torch.nn.Linear
    if not (hasattr(model, "eeg_model") and hasattr(model, "spectrogram_model") and isinstance(getattr(model, "fc1", None), lin)
            and isinstance(getattr(model, "fc2", None), lin)):
        raise ValueError(f"{who}: needs a MultimodalModel (two branches and the fusion head fc1 -> ReLU -> fc2); a stand-alone branch has no modalities to weigh")
    K, Hd = int(model.fc2.out_features), int(model.fc1.out_features)
    if int(model.fc1.in_features) != 2 * K or int(model.fc2.in_features) != Hd or model.fc1.bias is None or model.fc2.bias is None:
        raise ValueError(f"{who}: the head must be Linear(2K,Hd) -> ReLU -> Linear(Hd,K) with biases; got fc1 {tuple(model.fc1.weight.shape)}, fc2 {tuple(model.fc2.weight.shape)}")
    if not (1 <= K <= 16 and 2 * K <= Hd <= 1024):
        raise ValueError(f"{who}: K = {K} classes and Hd = {Hd} hidden units; supported 1 <= K <= 16, 2K <= Hd <= 1024")
    return K, Hd


def _fusion_inputs(who, eeg, spec, what="the inputs"):
    """-> N: ``eeg`` [N,1,Chans,T] and ``spec`` [N,C,H,W] with the same N >= 1."""
    if not (isinstance(eeg, torch.Tensor) and eeg.dim() == 4 and eeg.shape[1] == 1 and isinstance(spec, torch.Tensor) and spec.dim() == 4):
        raise ValueError(f"{who}: {what} must be the tensors eeg [N,1,Chans,T] and spec [N,C,H,W]")
    if eeg.shape[0] != spec.shape[0]:
        raise ValueError(f"{who}: {what} have {int(eeg.shape[0])} EEG and {int(spec.shape[0])} spectrogram samples; both branches vote on the same samples")
    if eeg.shape[0] < 1 or eeg.numel() == 0 or spec.numel() == 0:
        raise ValueError(f"{who}: {what} are empty")
    return int(eeg.shape[0])


def _fusion_branches(model, eeg, spec, max_batch):
    """``FusionVotes`` of the samples: both branches in passes of at most max_batch rows (inside eval mode, without autograd)."""
    sm = model.spectrogram_model
    cap = min(_row_cap(spec, "spec", getattr(sm, "compute_dtype", torch.float32), max_batch), _row_cap(eeg, "eeg", torch.float32, max_batch))
    xe, xs = eeg.detach().to(torch.float32).contiguous(), spec.detach().to(torch.float32).contiguous()
    N = int(xe.shape[0])
    e = torch.cat([model.eeg_model(xe[i:i + cap]).float() for i in range(0, N, cap)]).contiguous()
    s = torch.cat([sm(xs[i:i + cap]).float() for i in range(0, N, cap)]).contiguous()
    return FusionVotes(e, s)


def fusion_votes(model, eeg, spec, max_batch=256):
    """The votes of both branches of a MultimodalModel on N samples: ``FusionVotes(e, s)``, fp32 [N,K] log-probabilities each -- what
    ``fusion_shap`` explains and what it takes as a background, so that a background set runs through the branches once for many
    calls.  Eval mode without autograd, passes of at most max_batch rows; no bit depends on max_batch.  The training flag and every
    requires_grad are restored on return."""
    who = "fusion_votes"
    max_batch = _max_batch(who, max_batch)
    _fusion_head(who, model)
    _fusion_inputs(who, eeg, spec)
    _need_gpu(who, "the model and its inputs", model, eeg, spec)
    with torch.cuda.device(eeg.device), _eval_frozen(model), torch.no_grad():
        return _fusion_branches(model, eeg, spec, max_batch)


def fusion_shap(model, eeg, spec, background, *, players="votes", class_idx=None, score="prob", max_batch=256, return_parts=False):
    """How much of a decision came from the EEG branch and how much from the spectrogram branch: the exact Shapley values of the votes
    the two branches hand to the fusion head.  Every other attribution here explains one input while the other is held; this one
    explains the fusion.  The model is a late fusion: each branch emits K log-probabilities (its votes) and the head is
    cat -> Linear(2K,Hd) -> ReLU -> Linear(Hd,K) -> LogSoftmax, so the game has at most 2K players, every coalition is enumerated -- no
    sampling, no surrogate fit -- and both branches run once per sample and once per background sample.
        v_c(S) = mean over the background rows j of score_c( head( the sample's votes on S, row j's votes elsewhere ) )
        phi_i  = sum over S without i of |S|! (M - |S| - 1)! / M! (v(S + i) - v(S))
    and the values of a sample add up to score(sample) - mean score(background).

    model:       a MultimodalModel with the reference's head; anything else is refused.
    background:  (eeg_bg, spec_bg) with Nb samples each, run through the branches in passes of at most max_batch; 'uniform': one row with
                 every vote -log K, the vote of a branch that knows nothing (no data needed); a ``FusionVotes`` (``fusion_votes``): votes
                 already computed.  A background row supplies both branches' votes of the same sample (a joint, interventional background).
    players:     'votes': every vote alone, M = 2K <= 16; 'modality': M = 2, all EEG votes against all spectrogram votes; 'class': M = K,
                 {e_c, s_c} per class -- which class's evidence, from both branches together, moved the explained class; or a partition
                 of range(2K) into lists (vote i < K = the EEG branch's i-th, vote K + i = the spectrogram branch's), M <= 16.
    class_idx:   None = each sample's arg-max class; an int; one class per sample (sequence / tensor [B]); 'all' = every class, the
                 result gains a class axis.
    score:       'prob': the softmax probability; 'logprob': the log-probability.
    max_batch:   rows per pass through the branches; no bit of the result depends on it.
    One launch evaluates the head on every (sample, background row, coalition) in fp32 and averages in fp64 in the rows' order
    (bx_fusion_values); the Shapley sums are fp64 in a fixed order with the host's weights (bx_shapley_exact, ``shapley_weights``).  The
    modality game and the interaction come from the same launch and the same code path for every ``players``.  The training flag and
    every requires_grad are restored on return.  Returns the values fp64 [B,M] ([B,K,M] for 'all') on the device, or ``FusionShapResult``
    with return_parts."""
    return _fusion_shap(model, eeg, spec, background, players, class_idx, score, max_batch, return_parts)


def _fusion_shap(model, eeg, spec, background, players, class_idx, score, max_batch, return_parts, profile=None):
    """``fusion_shap`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'branches', 'values',
    'shapley' -- device events around every phase (tools/fusion_shap_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "fusion_shap"
    if score not in _FUSION_SCORES:
        raise ValueError(f"{who}: unknown score {score!r}; use 'prob' or 'logprob'")
    max_batch = _max_batch(who, max_batch)
    K, Hd = _fusion_head(who, model)
    B = _fusion_inputs(who, eeg, spec)
    groups = _fusion_players(who, players, K)
    M = len(groups)
    cls_h, all_classes = _explained_classes(who, class_idx, B, K, allow_all=True)
    bg_votes, bg_inputs = None, ()
    if isinstance(background, str):
        if background != "uniform":
            raise ValueError(f"{who}: unknown background {background!r}; use 'uniform', (eeg_bg, spec_bg) or a FusionVotes")
        Nb = 1
    elif isinstance(background, FusionVotes):
        e_b, s_b = background
        if not all(isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == K and t.dtype == torch.float32 for t in (e_b, s_b)):
            raise ValueError(f"{who}: a FusionVotes background holds two fp32 tensors [Nb, {K}]")
        if e_b.shape[0] != s_b.shape[0] or e_b.shape[0] < 1:
            raise ValueError(f"{who}: the background holds {int(e_b.shape[0])} EEG and {int(s_b.shape[0])} spectrogram rows; a row is one sample's two votes")
        bg_votes, Nb = background, int(e_b.shape[0])
    elif isinstance(background, (tuple, list)) and len(background) == 2:
        Nb = _fusion_inputs(who, background[0], background[1], "the background (eeg_bg, spec_bg)")
        if tuple(background[0].shape[1:]) != tuple(eeg.shape[1:]) or tuple(background[1].shape[1:]) != tuple(spec.shape[1:]):
            raise ValueError(f"{who}: the background samples are shaped {tuple(background[0].shape[1:])} / {tuple(background[1].shape[1:])}, "
                             f"the inputs {tuple(eeg.shape[1:])} / {tuple(spec.shape[1:])}")
        bg_inputs = tuple(background)
    else:
        raise ValueError(f"{who}: background must be 'uniform', (eeg_bg, spec_bg) or a FusionVotes, got {type(background).__name__}")
    masks = _fusion_masks(groups, K)
    NS, n = int(masks.shape[0]), 1 << M
    if B > 65535 or B * NS * K >= 1 << 31:
        raise ValueError(f"{who}: B = {B} samples (limit 65535) or B * (2^M + 4) * K = {B * NS * K} beyond 32-bit offsets; use fewer samples per call")
    _need_gpu(who, "the model, its inputs and the background", model, eeg, spec, *bg_inputs, *(bg_votes or ()))

    lib = L.load()
    dev = eeg.device
    with torch.cuda.device(dev), _eval_frozen(model), torch.no_grad():
        with _lap(profile, "branches"):
            votes = _fusion_branches(model, eeg, spec, max_batch)
            if bg_inputs:
                bg_votes = _fusion_branches(model, bg_inputs[0].to(dev), bg_inputs[1].to(dev), max_batch)
            elif bg_votes is None:
                row = torch.full((1, K), float(np.float32(-math.log(K))), dtype=torch.float32, device=dev)
                bg_votes = FusionVotes(row, row.clone())
            else:
                bg_votes = FusionVotes(*(t.detach().to(dev).contiguous() for t in bg_votes))
        w1, b1, w2, b2 = (t.detach().to(torch.float32).contiguous() for t in (model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias))
        masks_d = torch.from_numpy(masks.view(np.int32)).to(dev)
        with _lap(profile, "values"):
            v = torch.empty(B, NS, K, dtype=torch.float64, device=dev)
            L.check(lib.bx_fusion_values(_p(votes.e), _p(votes.s), _p(bg_votes.e), _p(bg_votes.s), _p(masks_d), _p(w1), _p(b1), _p(w2), _p(b2),
                                         _FUSION_SCORES[score], _p(v), B, Nb, NS, K, Hd, _stream()), "bx_fusion_values")
        with _lap(profile, "shapley"):
            empty, clean = v[:, n].contiguous(), v[:, n + 3].contiguous()            # the modality game's none and all
            classes = _class_tensor(cls_h, all_classes, clean, dev)
            # one row per (sample, class): the explained class's column of every coalition (a gather; the arithmetic is the library's)
            rows = v.permute(0, 2, 1) if all_classes else v.gather(2, classes.long()[:, None, None].expand(B, NS, 1)).permute(0, 2, 1)
            R = B * (K if all_classes else 1)
            game, duo = rows[..., :n].reshape(R, n).contiguous(), rows[..., n:].reshape(R, 4).contiguous()
            values, modality, interaction = (torch.empty(R, m, dtype=torch.float64, device=dev) for m in (M, 2, 1))
            for vr, m, out in ((game, M, values), (duo, 2, modality)):
                w_d = torch.from_numpy(shapley_weights(m)).to(dev)
                L.check(lib.bx_shapley_exact(_p(vr), _p(w_d), _p(out), R, m, _stream()), "bx_shapley_exact")
            L.check(lib.bx_fusion_interaction(_p(duo), _p(interaction), R, _stream()), "bx_fusion_interaction")
    lead = (B, K) if all_classes else (B,)
    values, modality, interaction = values.reshape(*lead, M), modality.reshape(*lead, 2), interaction.reshape(*lead)
    if not return_parts:
        return values
    return FusionShapResult(values, modality, interaction, v[:, :n].contiguous(), None if classes is None else classes.long(), clean, empty, votes,
                            bg_votes, groups, masks[:n].copy(), score)


def modality_importance(values):
    """The dataset-level figure: the mean |phi| of every player over the samples.  values: ``fusion_shap``'s values fp64 [B,M] or [B,K,M],
    or its ``FusionShapResult`` -> fp32 [M] or [K,M] (bx_mean_abs_rows: an fp64 sum over the samples in a fixed order, one rounding).
    On ``FusionShapResult.modality`` it is the share of the two modalities."""
    who = "modality_importance"
    if isinstance(values, FusionShapResult):
        values = values.values
    if not isinstance(values, torch.Tensor) or values.dim() not in (2, 3) or values.numel() == 0:
        raise ValueError(f"{who}: values must be fusion_shap's values [B,M] or [B,K,M] or its FusionShapResult")
    if not values.is_cuda:
        raise RuntimeError(f"brainxai.{who}: the values must live on the GPU; there is no CPU path")
    return channel_importance(values.movedim(0, -1))


# ---- TCAV: concept activation vectors and TCAV scores (include/brainxai.h, "TCAV") ----
_TCAV_CLASSIFIERS = {"ridge": L.BX_TCAV_RIDGE, "mean_difference": L.BX_TCAV_MEAN_DIFFERENCE}
_TCAV_EEG_TARGET = re.compile(r"^(?:eeg_model\.)?features$")
_TCAV_MAX_N = 256
_TCAV_STATUS = {1: "its examples do not differ in this layer (tr K = 0)", 2: "the two sets have the same mean in this layer (w = 0)",
                3: "the Cholesky factorisation met a non-positive pivot", 4: "the problem is malformed"}


class CavSet(collections.namedtuple("CavSet", "vectors problems names accuracy holdout_accuracy norms lam decision gram target_layer input shape "
                                              "classifier ridge holdout n")):
    """What ``train_cavs`` returns: ``vectors`` fp32 [P,D] on the device (unit CAVs, oriented towards the concept), ``problems`` int64
    host [P,2] -- row p of ``vectors`` separates concept problems[p,0] from random set problems[p,1]; the null problems come last with
    problems[p,0] = -1: random set problems[p,1] against random set (problems[p,1] + 1) % R -- ``names`` (the concepts in order),
    ``accuracy`` and ``holdout_accuracy`` fp64 [P] (NaN without held-out rows), ``norms`` fp64 [P] = |w|, ``lam`` fp64 [P], ``decision``
    fp64 [P,2n] (positives first, then negatives, held-out rows included), ``gram`` fp64 [M,M] (keep_gram=True, else None),
    ``target_layer`` and ``input`` (normalised), ``shape`` (the unflattened activation shape) and the arguments ``classifier``,
    ``ridge``, ``holdout`` and the set size ``n``."""
    __slots__ = ()

    @property
    def Q(self):
        return len(self.names)

    @property
    def R(self):
        return int((self.problems[:, 0] == 0).sum()) if self.Q else int((self.problems[:, 0] < 0).sum())

    def index(self, name, r):
        """The row of ``vectors`` for concept ``name`` against random set r."""
        if name not in self.names:
            raise KeyError(f"CavSet: no concept {name!r}; it holds " + ", ".join(repr(s) for s in self.names))
        if not 0 <= int(r) < self.R:
            raise IndexError(f"CavSet: random set {r} outside 0..{self.R - 1}")
        return self.names.index(name) * self.R + int(r)

    def vector(self, name, r=0):
        """The CAV of concept ``name`` against random set r, reshaped to the activation's shape."""
        return self.vectors[self.index(name, r)].reshape(self.shape)


TcavResult = collections.namedtuple("TcavResult", "scores scores_per_random null_scores p_value t dof mean_sensitivity mean_abs_sensitivity sensitivity "
                                                  "classes out counts cavs")
TcavResult.__doc__ = """What ``tcav(..., return_parts=True)`` returns: ``scores`` fp64 [Q,K] (what the plain call returns: the mean over the random sets),
``scores_per_random`` fp64 [Q,R,K], ``null_scores`` fp64 [R,K] (random set against random set; [0,K] when R < 2), ``p_value``, ``t``, ``dof`` fp64
[Q,K] (Welch's two-sided test of the R concept scores against the R null scores; NaN when R < 2 or a variance is 0),
``mean_sensitivity`` and ``mean_abs_sensitivity`` fp64 [Q,R,K], ``sensitivity`` fp64 [B,P] ([B,K,P] for class_idx='all'; P counts the null
problems too, in ``cavs.problems``' order), ``classes`` int64 [B] (None for 'all'), ``out`` fp32 [B,K], ``counts`` int64 [K] (the samples
behind each class's score) and ``cavs``, the ``CavSet``.  A class without samples has NaN scores."""


def _betacf(a, b, x):
    """The continued fraction of the incomplete beta function by the modified Lentz method (Numerical Recipes 6.4)."""
    tiny, qab, qap, qam = 1e-300, a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (tiny if abs(d) < tiny else d)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / (tiny if abs(d) < tiny else d)
            c = 1.0 + aa / c
            c = tiny if abs(c) < tiny else c
            de = d * c
            h *= de
        if abs(de - 1.0) < 1e-16:
            break
    return h


def regularized_incomplete_beta(a, b, x):
    """I_x(a, b) in fp64 on the host: the continued fraction, on the side of the symmetry point where it converges fast."""
    if not (a > 0 and b > 0) or math.isnan(x):
        return float("nan")
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def welch_t_test(a, b):
    """Welch's two-sided t-test of two samples along the last axis (scipy.stats.ttest_ind(a, b, axis=-1, equal_var=False), without
    scipy) -> (t, dof, p), fp64 numpy arrays of the leading shape.  NaN where a sample has fewer than 2 values, a variance is 0 or a
    value is NaN.  The Student t distribution comes from the regularised incomplete beta function, p = I_{dof / (dof + t^2)}(dof / 2, 1 / 2)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    lead = np.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    na, nb = a.shape[-1], b.shape[-1]
    t, dof, p = (np.full(lead, np.nan) for _ in range(3))
    if na < 2 or nb < 2:
        return t, dof, p
    a, b = np.broadcast_to(a, lead + (na,)), np.broadcast_to(b, lead + (nb,))
    for ix in np.ndindex(*lead):
        u, v = a[ix], b[ix]
        va, vb = float(u.var(ddof=1)) / na, float(v.var(ddof=1)) / nb
        if not (va > 0.0 and vb > 0.0):                              # a zero variance, or a NaN
            continue
        t[ix] = (float(u.mean()) - float(v.mean())) / math.sqrt(va + vb)
        dof[ix] = (va + vb) ** 2 / (va * va / (na - 1) + vb * vb / (nb - 1))
        p[ix] = regularized_incomplete_beta(0.5 * dof[ix], 0.5, dof[ix] / (dof[ix] + t[ix] * t[ix]))
    return t, dof, p


def _tcav_target(who, model, input, target_layer):
    """-> (input_is_spec, multimodal, net, target name, (stage, conv_k) or None): the explained branch and the normalised target."""
    if input not in ("spec", "eeg"):
        raise ValueError(f"{who}: input must be 'spec' or 'eeg', got {input!r}")
    input_is_spec = input == "spec"
    if target_layer is None:
        target_layer = "spectrogram_model.block5" if input_is_spec else "eeg_model.features"
    ms = _TARGET.match(target_layer) if isinstance(target_layer, str) else None
    me = _TCAV_EEG_TARGET.match(target_layer) if isinstance(target_layer, str) else None
    if not ms and not me:
        raise ValueError(f"{who}: unknown target_layer {target_layer!r}; use 'spectrogram_model.blockN[.convK]' (input='spec') or "
                         "'eeg_model.features' (input='eeg')")
    if bool(ms) != input_is_spec:
        raise ValueError(f"{who}: target_layer {target_layer!r} belongs to the {'spectrogram' if ms else 'EEG'} branch but input={input!r}; "
                         "a branch's activation depends on its own input only")
    multimodal = hasattr(model, "spectrogram_model") and hasattr(model, "eeg_model")
    net = (model.spectrogram_model if input_is_spec else model.eeg_model) if multimodal else model
    if input_is_spec:
        if not (hasattr(net, "block1") and hasattr(net, "fc")):
            raise ValueError(f"{who}: input='spec' needs a MultimodalModel or a Spectrogram_Model")
        stage, conv_k = int(ms.group(1)), int(ms.group(2)) if ms.group(2) else 0
        return True, multimodal, net, f"spectrogram_model.block{stage}" + (f".conv{conv_k}" if conv_k else ""), (stage, conv_k)
    from .models import EEGNet, EEGNetAttentionDeep
    if not isinstance(net, (EEGNet, EEGNetAttentionDeep)):
        raise ValueError(f"{who}: input='eeg' needs a MultimodalModel, an EEGNet or an EEGNetAttentionDeep")
    return False, multimodal, net, "eeg_model.features", None


def _tcav_shape(who, net, where, tail):
    """The unflattened activation shape of one example whose input is shaped ``tail`` (C,H,W or 1,Chans,T), from the geometry alone."""
    if where is None:
        g = net._geom
        feats = g.F2 * (int(tail[2]) // (g.P1 * g.P2))
        if feats < 1:
            raise ValueError(f"{who}: {int(tail[2])} time samples leave no EEG features")
        return (feats,)
    H, W = int(tail[1]), int(tail[2])
    for i in range(1, where[0] + 1):
        blk = getattr(net, f"block{i}")
        if i == where[0] and where[1]:
            break
        H, W = H // blk.pool_window[0], W // blk.pool_window[1]
    if H < 1 or W < 1:
        raise ValueError(f"{who}: a spectrogram of {int(tail[1])} x {int(tail[2])} does not reach block{where[0]}")
    return (H, W, int(getattr(net, f"block{where[0]}").out_channels))


def _tcav_options(who, classifier, ridge, holdout):
    if classifier not in _TCAV_CLASSIFIERS:
        raise ValueError(f"{who}: unknown classifier {classifier!r}; use " + " or ".join(f"'{k}'" for k in _TCAV_CLASSIFIERS))
    if isinstance(ridge, bool) or not isinstance(ridge, numbers.Real) or not math.isfinite(ridge) or not ridge > 0:
        raise ValueError(f"{who}: ridge must be a finite number > 0, got {ridge!r}")
    if isinstance(holdout, bool) or not isinstance(holdout, numbers.Real) or not 0 <= holdout < 0.5:
        raise ValueError(f"{who}: holdout must be a fraction in [0, 0.5), got {holdout!r}")
    return float(ridge), float(holdout)


def _tcav_sets(who, concepts, randoms, input_is_spec, tail, holdout):
    """-> (names, the Q + R example tensors in stacking order, n, held-out rows per set, the examples' shape).  ``tail``: the explained input's shape without
    its batch axis, or None (``train_cavs``: the first set's)."""
    if not isinstance(concepts, dict) or not concepts or not all(isinstance(k, str) for k in concepts):
        raise ValueError(f"{who}: concepts must be a non-empty dict of name -> example tensor")
    if not isinstance(randoms, (list, tuple)) or len(randoms) < 1:
        raise ValueError(f"{who}: randoms must be a list of at least one example tensor")
    form = "[n,C,H,W]" if input_is_spec else "[n,1,Chans,T]"
    sets = [(f"concepts[{k!r}]", t) for k, t in concepts.items()] + [(f"randoms[{r}]", t) for r, t in enumerate(randoms)]
    n = None
    for what, t in sets:
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or (not input_is_spec and t.shape[1] != 1) or t.numel() == 0:
            raise ValueError(f"{who}: {what} must be a tensor {form}")
        if tail is None:
            tail = tuple(t.shape[1:])
        if tuple(t.shape[1:]) != tuple(tail):
            raise ValueError(f"{who}: {what} holds examples shaped {tuple(t.shape[1:])}, the explained input's are {tuple(tail)}")
        if n is None:
            n = int(t.shape[0])
        if int(t.shape[0]) != n:
            raise ValueError(f"{who}: {what} holds {int(t.shape[0])} examples, {sets[0][0]} {n}; every set must have the same size")
    if not 2 <= n <= _TCAV_MAX_N:
        raise ValueError(f"{who}: {n} examples per set, supported 2..{_TCAV_MAX_N}")
    nh = int(math.ceil(holdout * n - 1e-12))
    if n - nh < 2:
        raise ValueError(f"{who}: holdout = {holdout} leaves {n - nh} of {n} examples per set for the fit; at least 2 are needed")
    if len(sets) * n > L.BX_TCAV_MAX_M:
        raise ValueError(f"{who}: {len(sets)} sets of {n} examples stack to {len(sets) * n} rows, supported up to {L.BX_TCAV_MAX_M}")
    return list(concepts), [t for _, t in sets], n, nh, tuple(tail)


def _tcav_free_bytes(dev):
    """The free memory of a GPU in bytes; None for any other device (the closing refusal then speaks)."""
    return int(torch.cuda.mem_get_info(dev)[0]) if dev.type == "cuda" else None


def _tcav_fits_memory(who, model, net, where, sets, shape):
    """The refusal of a stack of activations [M,D], in the branch's storage dtype, beyond the free memory of the model's device."""
    M, D, dev = len(sets) * int(sets[0].shape[0]), int(np.prod(shape)), next(model.parameters()).device
    esize = 2 if where is not None and getattr(net, "compute_dtype", torch.float32) == torch.bfloat16 else 4
    need, free = M * D * esize, _tcav_free_bytes(dev)
    if free is not None and need > free:
        raise ValueError(f"{who}: the stacked activations, {M} rows of {D} features, take {need} bytes; {free} bytes of device memory are free -- "
                         "use fewer or smaller sets, or a deeper target_layer")


def _tcav_problems(Q, R, n, nh):
    """The problems' tables: (problems int64 [P,2], rows, labels, fit int32 [P,2n]).  Set s occupies the stacked rows s n .. s n + n - 1."""
    pairs = [(q, r, q, Q + r) for q in range(Q) for r in range(R)] + ([(-1, r, Q + r, Q + (r + 1) % R) for r in range(R)] if R >= 2 else [])
    ar = np.arange(n)
    rows = np.array([np.concatenate([sp * n + ar, sn * n + ar]) for _, _, sp, sn in pairs], dtype=np.int32)
    labels = np.tile(np.concatenate([np.ones(n), -np.ones(n)]).astype(np.int32), (len(pairs), 1))
    fit = np.tile(np.concatenate([ar < n - nh, ar < n - nh]).astype(np.int32), (len(pairs), 1))
    return np.array([(q, r) for q, r, _, _ in pairs], dtype=np.int64).reshape(len(pairs), 2), rows, labels, fit


def _tcav_pair_name(names, problems, p, R):
    q, r = int(problems[p, 0]), int(problems[p, 1])
    return f"concept {names[q]!r} against random set {r}" if q >= 0 else f"random set {r} against random set {(r + 1) % R} (a null problem)"


def _tcav_activations(net, where, sets, D, dt, cap, dev):
    """The stacked activations [M,D] in the branch's storage dtype: every example once through the explained branch, without autograd."""
    n = int(sets[0].shape[0])
    A = torch.empty(len(sets) * n, D, dtype=dt, device=dev)
    ctx = _SpecTarget(getattr(net, f"block{where[0]}"), where[1]) if where is not None else contextlib.nullcontext()
    with torch.no_grad(), ctx as tgt:
        for s, t in enumerate(sets):
            xs = t.detach().to(dev, torch.float32).contiguous()
            for i in range(0, n, cap):
                if where is None:
                    a = ops.eeg_features_keep(net, xs[i:i + cap])[0]
                else:
                    net(xs[i:i + cap])
                    a = tgt.act()
                A[s * n + i:s * n + i + a.shape[0]] = a.reshape(a.shape[0], D)
    return A


def train_cavs(model, concepts, randoms, *, input="spec", target_layer=None, classifier="ridge", ridge=1e-2, holdout=0.0, max_batch=256,
               keep_gram=False):
    """Concept activation vectors of a layer (Kim et al., ICML 2018): for every (concept, random set) pair a linear classifier between the
    layer's activations of the concept's examples and of the random set's, whose unit normal, oriented towards the concept, is the CAV;
    with two random sets or more also the null problems, random set r against random set r + 1.

    concepts:     dict name -> examples; randoms: list of example tensors.  Examples are inputs of the explained branch alone, [n,C,H,W]
                  (input='spec') or [n,1,Chans,T] ('eeg'): a branch's activation depends on its own input only.  Every set has the same
                  2 <= n <= 256 examples.  Building the sets is the caller's job (``gaussian_blur``, ``eeg_spectrum`` / ``band_sums`` and the
                  stackers of ``brainxai.data`` help).
    target_layer: 'spectrogram_model.blockN' or '.blockN.convK' (what ``grad_cam`` captures there, flattened NHWC) or
                  'eeg_model.features' (the flattened block-2 features of an EEGNet / EEGNetAttentionDeep); the prefix is optional and a
                  stand-alone branch is accepted.  Default: block5 / features.
    classifier:   'ridge': least squares with lambda = ridge * tr(K) / rows, solved in the dual by an fp64 Cholesky factorisation;
                  'mean_difference': the difference of the two sets' mean activations (Pattern-CAV, Pahde et al. 2022).
    holdout:      0 <= h < 0.5: the last ceil(h n) examples of every set are kept out of the fit; ``holdout_accuracy`` is theirs.
    The examples run through the branch once, in passes of at most max_batch, in evaluation mode without autograd; the Gram matrix of
    the stacked, centred activations is computed once (bx_tcav_mean, bx_tcav_gram) and every classifier is a function of it
    (bx_tcav_fit); bx_tcav_vectors forms the CAVs.  A pair that cannot be separated -- identical examples -- raises, naming the pair.
    The training flag and every requires_grad are restored on return.  Returns a ``CavSet``."""
    who = "train_cavs"
    max_batch = _max_batch(who, max_batch)
    input_is_spec, _, net, target, where = _tcav_target(who, model, input, target_layer)
    ridge, holdout = _tcav_options(who, classifier, ridge, holdout)
    names, sets, n, nh, tail = _tcav_sets(who, concepts, randoms, input_is_spec, None, holdout)
    shape = _tcav_shape(who, net, where, tail)
    _tcav_fits_memory(who, model, net, where, sets, shape)
    return _train_cavs(who, model, net, input, target, where, names, sets, n, nh, shape, classifier, ridge, holdout, max_batch, keep_gram, None)


def _train_cavs(who, model, net, input, target, where, names, sets, n, nh, shape, classifier, ridge, holdout, max_batch, keep_gram, profile):
    """``train_cavs`` once its arguments are checked.  profile: phases 'activations', 'gram', 'fit', 'vectors'."""
    Q, R, D = len(names), len(sets) - len(names), int(np.prod(shape))
    M = (Q + R) * n
    dev = next(model.parameters()).device
    dt = getattr(net, "compute_dtype", torch.float32) if where is not None else torch.float32
    _need_gpu(who, "the model and the example sets", model, *sets)
    lib = L.load()
    problems, rows, labels, fit = _tcav_problems(Q, R, n, nh)
    P, NI, nf = int(rows.shape[0]), 2 * n, 2 * (n - nh)
    with torch.cuda.device(dev), _eval_frozen(model):
        with _lap(profile, "activations"):
            cap = _row_cap(sets[0], input, dt, max_batch)
            A = _tcav_activations(net, where, sets, D, dt, cap, dev)
        code = ops.bx_dtype(A.dtype)
        with _lap(profile, "gram"):
            mean = torch.empty(D, dtype=torch.float64, device=dev)
            gram = torch.empty(M, M, dtype=torch.float64, device=dev)
            L.check(lib.bx_tcav_mean(_p(A), _p(mean), M, D, code, _stream()), "bx_tcav_mean")
            ws = ops.workspace(lib.bx_tcav_gram_workspace(M, D), dev)
            L.check(lib.bx_tcav_gram(_p(A), _p(mean), _p(gram), M, D, code, _p(ws), ws.numel(), _stream()), "bx_tcav_gram")
        with _lap(profile, "fit"):
            rows_d, labels_d, fit_d = (torch.from_numpy(a).to(dev) for a in (rows, labels, fit))
            counts_d = torch.full((P,), NI, dtype=torch.int32, device=dev)
            beta = torch.zeros(P, M, dtype=torch.float64, device=dev)
            norms, lam = (torch.full((P,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
            decision = torch.full((P, NI), float("nan"), dtype=torch.float64, device=dev)
            acc = torch.full((P, 2), float("nan"), dtype=torch.float64, device=dev)
            status = torch.empty(P, dtype=torch.int32, device=dev)
            ws = ops.workspace(lib.bx_tcav_fit_workspace(P, nf), dev)
            L.check(lib.bx_tcav_fit(_p(gram), M, _p(rows_d), _p(labels_d), _p(fit_d), _p(counts_d), P, NI, nf, _TCAV_CLASSIFIERS[classifier], ridge,
                                    _p(ws), ws.numel(), _p(beta), _p(norms), _p(lam), _p(status), _p(decision), _p(acc), _stream()), "bx_tcav_fit")
            st = status.cpu()                                        # the one read of the problems' status
            if bool((st != 0).any()):
                bad = int((st != 0).nonzero()[0])
                raise RuntimeError(f"brainxai.{who}: {_tcav_pair_name(names, problems, bad, R)} cannot be separated at {target}: "
                                   f"{_TCAV_STATUS.get(int(st[bad]), 'status ' + str(int(st[bad])))}")
        with _lap(profile, "vectors"):
            V = torch.empty(P, D, dtype=torch.float32, device=dev)
            L.check(lib.bx_tcav_vectors(_p(A), _p(mean), _p(beta), _p(norms), _p(status), _p(V), M, D, P, code, _stream()), "bx_tcav_vectors")
    return CavSet(V, problems, names, acc[:, 0].contiguous(), acc[:, 1].contiguous(), norms, lam, decision, gram if keep_gram else None, target, input,
                  tuple(shape), classifier, ridge, holdout, n)


def tcav(model, eeg, spec, concepts=None, randoms=None, *, cavs=None, input="spec", target_layer=None, classifier="ridge", ridge=1e-2, holdout=0.0,
         class_idx=None, max_batch=256, return_parts=False):
    """Testing with Concept Activation Vectors (Kim et al., ICML 2018; Captum's concept.TCAV): does the model use a concept -- alpha
    rhythm, delta slowing, a muscle artefact, given as example inputs -- when it decides for a class, and at which depth?  Every other
    explanation of the package is a map of one sample; this one is a number per (concept, class) over a set of samples.
        S_k(x; v) = grad_a F_k(x) . v        the directional derivative of class k's log-probability along the unit CAV v at the layer
        score     = the share of the samples x explained for class k with S_k(x; v) > 0
    computed against every random set (``train_cavs``) and averaged over them; the same scores of the null problems, random set against
    random set, are what a concept has to beat: ``p_value`` is Welch's two-sided t-test of the R concept scores against the R null scores.

    eeg, spec:    the samples to test, as for ``grad_cam``; a stand-alone branch takes None for the other input.
    concepts, randoms / cavs: the example sets (``train_cavs`` runs first, with input, target_layer, classifier, ridge, holdout), or a
                  ``CavSet`` trained before, which must fit input, target_layer and the activation's size.  One or the other.
    class_idx:    None: a sample counts for its arg-max class (a class without samples scores NaN); an int c: every sample, explained for
                  class c; one class per sample; 'all': every sample for every class.
    The samples run as ``grad_cam``'s general path does -- capture, one forward and one backward pass per class seed, in passes of at
    most max_batch samples; 'eeg_model.features' runs the EEG branch without autograd and differentiates the head alone.  The dot
    products are fp64 sums in an order that depends on the activation's size alone (bx_tcav_sensitivity), the scores one launch
    (bx_tcav_score); no bit of the result depends on max_batch.  The training flag and every requires_grad are restored on return.
    Returns the scores fp64 [Q,K] on the device, or ``TcavResult`` with return_parts."""
    return _tcav(model, eeg, spec, concepts, randoms, cavs, input, target_layer, classifier, ridge, holdout, class_idx, max_batch, return_parts)


def _tcav(model, eeg, spec, concepts, randoms, cavs, input, target_layer, classifier, ridge, holdout, class_idx, max_batch, return_parts, profile=None):
    """``tcav`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'activations', 'gram',
    'fit', 'vectors' (``train_cavs``), 'gradients', 'sensitivity' -- device events around every phase (tools/tcav_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "tcav"
    max_batch = _max_batch(who, max_batch)
    if (cavs is None) == (concepts is None and randoms is None):
        raise ValueError(f"{who}: pass either cavs= (a CavSet from train_cavs) or the example sets concepts and randoms, not both and not neither")
    if cavs is not None and not isinstance(cavs, CavSet):
        raise ValueError(f"{who}: cavs must be a CavSet from train_cavs, got {type(cavs).__name__}")
    if cavs is not None and target_layer is None:
        target_layer = cavs.target_layer
    input_is_spec, _, net, target, where = _tcav_target(who, model, input, target_layer)
    call = _Call(who, model, input).tensors(eeg, spec)
    x, B = call.x, _nonempty(who, call.x)
    K, Kc, cls_h, all_classes = call.explained(class_idx).K, call.Kc, call.cls_h, call.all_classes
    multimodal, other = call.multimodal, call.other
    shape = _tcav_shape(who, net, where, tuple(x.shape[1:]))
    D = int(np.prod(shape))
    if cavs is None:
        ridge, holdout = _tcav_options(who, classifier, ridge, holdout)
        names, sets, n, nh, _ = _tcav_sets(who, concepts, randoms, input_is_spec, tuple(x.shape[1:]), holdout)
        _tcav_fits_memory(who, model, net, where, sets, shape)
    elif cavs.input != input or cavs.target_layer != target or int(cavs.vectors.shape[1]) != D:
        raise ValueError(f"{who}: the CavSet was trained for input={cavs.input!r} at {cavs.target_layer} with {int(cavs.vectors.shape[1])} features; "
                         f"this call explains input={input!r} at {target} with {D}")
    call.need_gpu("the model and its inputs", other)               # the other input wherever it is given, beside a stand-alone branch too
    if cavs is None:
        cavs = _train_cavs(who, model, net, input, target, where, names, sets, n, nh, shape, classifier, ridge, holdout, max_batch, False, profile)
    call.need_gpu("the CavSet", cavs.vectors)

    lib = L.load()
    dev = x.device
    V = cavs.vectors.contiguous()
    P = int(V.shape[0])
    cap = call.row_cap(max_batch)
    with torch.cuda.device(dev), _eval_frozen(model):
        xs = x.detach().to(torch.float32).contiguous()
        xo = other.detach().to(torch.float32).contiguous() if multimodal else None
        out = torch.empty(B, K, dtype=torch.float32, device=dev)
        classes = None if all_classes else torch.empty(B, dtype=torch.int32, device=dev)
        if cls_h is not None:
            classes.copy_(torch.tensor(cls_h, dtype=torch.int32))
        S = torch.empty(Kc, B, P, dtype=torch.float64, device=dev)
        for b0 in range(0, B, cap):
            nb = min(cap, B - b0)
            with _lap(profile, "gradients"), contextlib.ExitStack() as stack:
                if input_is_spec:
                    leaf_in = xs[b0:b0 + nb].clone().requires_grad_(True)
                    tgt = stack.enter_context(_SpecTarget(getattr(net, f"block{where[0]}"), where[1], want_input=True))
                    y = model(xo[b0:b0 + nb], leaf_in) if multimodal else net(leaf_in)
                    leaf, read = tgt.leaf, tgt.grad
                else:
                    with torch.no_grad():
                        feat = ops.eeg_features_keep(net, xs[b0:b0 + nb])[0]
                        s_out = model.spectrogram_model(xo[b0:b0 + nb]) if multimodal else None
                    leaf = feat.detach().requires_grad_(True)
                    with torch.enable_grad():
                        y = _eeg_head(net, leaf)
                        if multimodal:
                            y = ops.FusionHeadFn.apply(y, s_out, model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias)
                    read = lambda g: g
                yd = y.detach().float().contiguous()
                out[b0:b0 + nb] = yd
                if cls_h is None and not all_classes:
                    classes[b0:b0 + nb] = yd.argmax(dim=1).to(torch.int32)
                seed = torch.empty(nb, K, dtype=torch.float32, device=dev)
                grads = []
                for slot in range(Kc):
                    L.check(lib.bx_expgrad_seed(None if all_classes else _p(classes[b0:b0 + nb]), slot if all_classes else -1, _p(seed), nb, 1, K, 0, nb,
                                                _stream()), "bx_expgrad_seed")
                    (g,) = torch.autograd.grad(y, leaf, grad_outputs=seed, retain_graph=slot + 1 < Kc)
                    grads.append(read(g).contiguous())
                    if grads[-1].dtype not in (torch.float32, torch.bfloat16):
                        grads[-1] = grads[-1].float()
                del y, leaf
            with _lap(profile, "sensitivity"):
                for slot, g in enumerate(grads):
                    if g.numel() != nb * D:
                        raise RuntimeError(f"brainxai.{who}: the gradient at {target} has {g.numel() // nb} values per sample, the CAVs {D}")
                    L.check(lib.bx_tcav_sensitivity(_p(g), _p(V), _p(S[slot]), nb, D, P, b0, B, ops.bx_dtype(g.dtype), _stream()), "bx_tcav_sensitivity")
            del grads
        with _lap(profile, "sensitivity"):
            sens = S.permute(1, 0, 2).contiguous() if all_classes else S[0]
            score, mean_s, mean_abs = (torch.empty(P, K, dtype=torch.float64, device=dev) for _ in range(3))
            counts = torch.empty(K, dtype=torch.int32, device=dev)
            L.check(lib.bx_tcav_score(_p(sens), _p(classes), B * Kc, P, K, _p(score), _p(mean_s), _p(mean_abs), _p(counts), _stream()), "bx_tcav_score")
    # ---- the host's share: the mean over the random sets and Welch's test, on [P,K] numbers ----
    Q, R = cavs.Q, cavs.R
    sc_h = score.cpu().numpy()
    per_random, null = sc_h[:Q * R].reshape(Q, R, K), sc_h[Q * R:].reshape(-1, K)
    scores_h = per_random.sum(axis=1) / R
    if not return_parts:
        return torch.from_numpy(scores_h).to(dev)
    t, dof, pv = welch_t_test(per_random.transpose(0, 2, 1), null.T[None]) if R >= 2 else (np.full((Q, K), np.nan),) * 3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return TcavResult(up(scores_h), up(per_random), up(null), up(pv), up(t), up(dof), mean_s[:Q * R].reshape(Q, R, K), mean_abs[:Q * R].reshape(Q, R, K), sens,
                      None if classes is None else classes.long(), out, counts.long(), cavs)


# ------------------------------------------------------------------------------------------------
# TracIn: training-data influence and self-influence through the model's Linear layers.  The definition is pinned in
# include/brainxai.h; tests/tracin_ref.py restates it.
_TRACIN_LAYERS = ("fc2", "fc1", "eeg_model.dense", "spectrogram_model.fc")
_TRACIN_MAX_M, _TRACIN_MAX_BLOCK, _TRACIN_MAX_TOP = 4096, 65536, 256
_TRACIN_STATUS = {L.BX_TRACIN_NONFINITE: "a non-finite activation, target or factor",
                  L.BX_TRACIN_BAD_TARGET: "a target with a negative entry or no mass, or a label outside the classes"}
TracInResult = collections.namedtuple("TracInResult", "proponents proponent_scores opponents opponent_scores scores train_losses test_losses layers "
                                                      "learning_rates N")
TracInResult.__doc__ = """What ``tracin(..., return_parts=True)`` returns: ``proponents`` / ``opponents`` int64 [M,top] (the training examples with the largest /
smallest scores per test example, best first; what the plain call returns), ``proponent_scores`` / ``opponent_scores`` fp64 [M,top], ``scores``
fp64 [N,M] (None without keep_scores), ``train_losses`` fp64 [C,N] and ``test_losses`` fp64 [C,M] (KLDivLoss(reduction='sum') per example at
every checkpoint), all on the device; ``layers`` (the layers summed, in the library's order), ``learning_rates`` (one per checkpoint) and ``N``."""
SelfInfluenceResult = collections.namedtuple("SelfInfluenceResult", "self_influence top top_scores train_losses layers learning_rates N")
SelfInfluenceResult.__doc__ = """What ``self_influence(..., return_parts=True)`` returns: ``self_influence`` fp64 [N], ``top`` int64 [top] and ``top_scores`` fp64 [top]
(the most self-influential examples, the mislabel candidates; None without top), ``train_losses`` fp64 [C,N], on the device; ``layers``,
``learning_rates`` and ``N``."""


def _tracin_model(who, model):
    """-> the layers of the model as the library sees them: kind, K, Hd, names, dwidth, awidth.  Anything else is refused."""
    from .models import EEGNet, EEGNetAttentionDeep, Spectrogram_Model
    lin = torch.nn.Linear
    ns = collections.namedtuple("_TracinPlan", "kind K Hd names dwidth awidth")

    def limits(K, Hd, Cc, F):
        if not (1 <= K <= 32 and 1 <= Hd <= 256 and 1 <= Cc <= 1024 and 1 <= F <= 4096):
            raise ValueError(f"{who}: K = {K} classes, Hd = {Hd} hidden units, C = {Cc} channels, F = {F} EEG features; "
                             f"supported K <= 32, Hd <= 256, C <= 1024, F <= 4096")

    if hasattr(model, "eeg_model") and hasattr(model, "spectrogram_model"):
        em, sm = model.eeg_model, model.spectrogram_model
        if isinstance(em, EEGNetAttentionDeep):
            raise ValueError(f"{who}: an EEGNetAttentionDeep branch is out of scope; the EEG branch must be an EEGNet")
        if not all(isinstance(m, lin) for m in (getattr(model, "fc1", None), getattr(model, "fc2", None), getattr(em, "dense", None), getattr(sm, "fc", None))):
            raise ValueError(f"{who}: needs a MultimodalModel with the Linear layers fc2, fc1, eeg_model.dense and spectrogram_model.fc")
        K, Hd, F, Cc = int(model.fc2.out_features), int(model.fc1.out_features), int(em.dense.in_features), int(sm.fc.in_features)
        limits(K, Hd, Cc, F)
        if not (hasattr(model, "_fusable") and model._fusable()):
            raise ValueError(f"{who}: needs the un-hooked reference MultimodalModel (EEGNet, Spectrogram_Model, head Linear(2K,Hd) -> ReLU -> Linear(Hd,K) "
                             f"with Hd * 2K <= 4096): its activations come from the fused head")
        return ns("multimodal", K, Hd, _TRACIN_LAYERS, (K, Hd, K, K), (Hd, 2 * K, F, Cc))
    if type(model) is Spectrogram_Model:
        K, Cc = int(model.fc.out_features), int(model.fc.in_features)
        limits(K, 1, Cc, 1)
        return ns("spec", K, 0, ("fc",), (K,), (Cc,))
    if type(model) is EEGNet:
        K, F = int(model.dense.out_features), int(model.dense.in_features)
        limits(K, 1, 1, F)
        return ns("eeg", K, 0, ("dense",), (K,), (F,))
    raise ValueError(f"{who}: needs a MultimodalModel, a Spectrogram_Model or an EEGNet, got {type(model).__name__}")


def _tracin_layers(who, plan, layers):
    """-> (mask, names): bit l of mask selects the plan's layer l."""
    names = plan.names
    if isinstance(layers, str):
        if layers == "all":
            layers = names
        elif layers == "head" and plan.kind == "multimodal":
            layers = ("fc2", "fc1")
        else:
            layers = (layers,)
    try:
        layers = list(layers)
    except TypeError:
        raise ValueError(f"{who}: layers must be 'all', 'head' or a sequence of layer names, got {type(layers).__name__}") from None
    if not layers:
        raise ValueError(f"{who}: layers is empty")
    mask = 0
    for name in layers:
        if name not in names:
            raise ValueError(f"{who}: unknown layer {name!r}; use 'all'{', ' + repr('head') if plan.kind == 'multimodal' else ''} or any of {names}")
        mask |= 1 << names.index(name)
    return mask, tuple(n for l, n in enumerate(names) if mask >> l & 1)


def _tracin_checkpoints(who, checkpoints, learning_rates):
    """-> (the checkpoints as a list, one finite learning rate per checkpoint)."""
    import os
    if isinstance(checkpoints, (str, bytes, dict, os.PathLike)) or not hasattr(checkpoints, "__len__") or not hasattr(checkpoints, "__getitem__"):
        raise ValueError(f"{who}: checkpoints must be a sequence of state dicts, dicts with a 'state_dict' key or paths, got {type(checkpoints).__name__}")
    cks = list(checkpoints)
    if not cks:
        raise ValueError(f"{who}: checkpoints is empty")
    for c, ck in enumerate(cks):
        if not isinstance(ck, (dict, str, os.PathLike)):
            raise ValueError(f"{who}: checkpoint {c} must be a state dict, a dict with a 'state_dict' key or a path, got {type(ck).__name__}")
    if learning_rates is None:
        return cks, [1.0] * len(cks)
    try:
        rates = list(learning_rates)
    except TypeError:
        raise ValueError(f"{who}: learning_rates must be None or one number per checkpoint, got {type(learning_rates).__name__}") from None
    if len(rates) != len(cks):
        raise ValueError(f"{who}: {len(rates)} learning rates for {len(cks)} checkpoints")
    for c, r in enumerate(rates):
        if isinstance(r, bool) or not isinstance(r, numbers.Real) or not math.isfinite(float(r)):
            raise ValueError(f"{who}: learning rate {c} must be a finite number, got {r!r}")
    return cks, [float(r) for r in rates]


def _tracin_int(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
        raise ValueError(f"{who}: {name} = {v!r} outside {lo}..{hi}")
    return int(v)


def _tracin_form(plan):
    return {"multimodal": "(eeg [n,1,Chans,T], spec [n,C,H,W], target)", "eeg": "(x, target) with x [n,1,Chans,T]",
            "spec": "(x, target) with x [n,C,H,W]"}[plan.kind]


def _tracin_batch(who, plan, batch, what):
    """-> n: one batch in tensor form, (eeg, spec, target) for a MultimodalModel, (x, target) for a stand-alone branch."""
    form = _tracin_form(plan)
    want = 3 if plan.kind == "multimodal" else 2
    if not (isinstance(batch, (tuple, list)) and len(batch) == want and all(isinstance(t, torch.Tensor) for t in batch)):
        raise ValueError(f"{who}: {what} must be the tensors {form}")
    *xs, target = batch
    ok = all(x.dim() == 4 for x in xs) and (plan.kind == "spec" or xs[0].shape[1] == 1)
    if not ok:
        raise ValueError(f"{who}: {what} must be the tensors {form}")
    n = int(xs[0].shape[0])
    if any(int(x.shape[0]) != n for x in xs):
        raise ValueError(f"{who}: {what} hold {int(xs[0].shape[0])} EEG and {int(xs[1].shape[0])} spectrogram samples")
    if n < 1 or any(x.numel() == 0 for x in xs):
        raise ValueError(f"{who}: {what} are empty")
    is_dist = target.dtype == torch.float32 and tuple(target.shape) == (n, plan.K)
    is_label = target.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) and tuple(target.shape) == (n,)
    if not (is_dist or is_label):
        raise ValueError(f"{who}: the target of {what} must be fp32 [{n}, {plan.K}] or an integer tensor [{n}], got {target.dtype} {tuple(target.shape)}")
    return n


def _tracin_data(who, plan, data, what, tensors_only):
    """-> (n or None, batches): ``data`` in tensor form is one batch (n known); anything else re-iterable is a stream of batches."""
    if isinstance(data, (tuple, list)) and data and all(isinstance(t, torch.Tensor) for t in data):
        return _tracin_batch(who, plan, data, what), None
    if tensors_only or isinstance(data, (str, bytes, dict, torch.Tensor)) or not hasattr(data, "__iter__") or iter(data) is data:
        more = "" if tensors_only else ", or a re-iterable of such batches (a one-shot iterator cannot be walked once per checkpoint)"
        raise ValueError(f"{who}: {what}{more} must be the tensors {_tracin_form(plan)}")
    return None, data


class _TracinWalk:
    """The checkpoints' walk: the model's parameters and buffers are copied on the device on entry and put back bit for bit on exit;
    ``load(c)`` writes checkpoint c's weights, ``passes(data)`` runs the data through the model in passes of at most max_batch rows and
    yields every pass's activations, factors, losses and status words."""

    def __init__(self, who, model, plan, checkpoints, max_batch, profile):
        self.who, self.model, self.plan, self.checkpoints, self.max_batch, self.profile = who, model, plan, checkpoints, max_batch, profile
        self.dev = next(model.parameters()).device
        self.lib = L.load()
        self.ld = sum(plan.dwidth)
        shape = L.TracinShape()
        shape.layers = len(plan.names)
        for l, (dw, aw) in enumerate(zip(plan.dwidth, plan.awidth)):
            shape.dwidth[l], shape.awidth[l] = dw, aw
        self.shape = shape

    def __enter__(self):
        self.saved = [(t, t.detach().clone()) for t in list(self.model.parameters()) + list(self.model.buffers())]
        return self

    def __exit__(self, *exc):
        _rand_restore(self.saved)

    def load(self, c):
        who, ck = self.who, self.checkpoints[c]
        if not isinstance(ck, dict):
            ck = torch.load(ck, map_location="cpu", weights_only=False)
            if not isinstance(ck, dict):
                raise ValueError(f"{who}: checkpoint {c} holds a {type(ck).__name__}, not a state dict")
        sd = ck["state_dict"] if isinstance(ck.get("state_dict"), dict) else ck
        own = self.model.state_dict()
        missing, extra = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
        if missing or extra:
            raise ValueError(f"{who}: checkpoint {c}: its keys are not the model's (missing {missing[:3]}, unexpected {extra[:3]})")
        with torch.no_grad():
            self.model.load_state_dict(sd, strict=True)
        ops.bump_param_epoch()
        if self.plan.kind == "multimodal":
            self.w1, self.w2 = (t.detach().to(torch.float32).contiguous() for t in (self.model.fc1.weight, self.model.fc2.weight))

    def side(self, delta, acts, rows):
        s = L.TracinSide()
        s.delta, s.rows = _p(delta), rows
        for l, a in enumerate(acts):
            s.act[l] = _p(a)
        return s

    def _batches(self, data, what):
        if isinstance(data, (tuple, list)) and all(isinstance(t, torch.Tensor) for t in data):
            yield data
            return
        for batch in data:
            _tracin_batch(self.who, self.plan, batch, f"a batch of {what}")
            yield tuple(t.to(self.dev) for t in batch)

    def passes(self, data, what):
        """-> (n, acts, delta, loss, status) per pass, the rows in the data's order."""
        plan, model, lib, dev = self.plan, self.model, self.lib, self.dev
        K, Hd = plan.K, plan.Hd
        for batch in self._batches(data, what):
            *xs, target = batch
            xs = [x.detach().to(torch.float32).contiguous() for x in xs]
            dist = target.dtype == torch.float32
            target = target.detach().contiguous() if dist else target.detach().to(torch.int32).contiguous()
            if plan.kind == "multimodal":
                cap = min(_row_cap(xs[1], "spec", getattr(model.spectrogram_model, "compute_dtype", torch.float32), self.max_batch),
                          _row_cap(xs[0], "eeg", torch.float32, self.max_batch))
            else:
                cap = _row_cap(xs[0], plan.kind, getattr(model, "compute_dtype", torch.float32) if plan.kind == "spec" else torch.float32, self.max_batch)
            for b0 in range(0, int(xs[0].shape[0]), cap):
                n = min(cap, int(xs[0].shape[0]) - b0)
                tgt = target[b0:b0 + n]
                logp = torch.empty(n, K, dtype=torch.float32, device=dev)
                with _lap(self.profile, "forward"):
                    if plan.kind == "multimodal":
                        em, sm = model.eeg_model, model.spectrogram_model
                        ef = em.features(xs[0][b0:b0 + n]).float().contiguous()
                        feat = sm.features(xs[1][b0:b0 + n]).permute(0, 2, 3, 1).contiguous()
                        Cc, F = int(feat.shape[3]), int(ef.shape[1])
                        if (Hd, 2 * K, F, Cc) != tuple(plan.awidth):
                            raise RuntimeError(f"brainxai.{self.who}: the branches emit {F} EEG features and {Cc} channels, the layers expect "
                                               f"{plan.awidth[2]} and {plan.awidth[3]} (Samples mismatch)")
                        gap = torch.empty(n, Cc, dtype=torch.float32, device=dev)
                        votes = torch.empty(2, n, K, dtype=torch.float32, device=dev)           # the EEG branch's, then the spectrogram branch's
                        hidden = torch.empty(n, Hd, dtype=torch.float32, device=dev)
                        p = [t.detach() for t in (sm.fc.weight, sm.fc.bias, em.dense.weight, em.dense.bias, model.fc1.weight, model.fc1.bias,
                                                  model.fc2.weight, model.fc2.bias)]
                        L.check(lib.bx_mm_head_fwd(_p(feat), _p(ef), *[_p(t) for t in p], _p(gap), _p(votes[1]), _p(votes[0]), _p(hidden), _p(logp), n,
                                                   int(feat.shape[1]) * int(feat.shape[2]), Cc, F, K, Hd, ops.bx_dtype(feat.dtype), _stream()), "bx_mm_head_fwd")
                        acts = [hidden, torch.cat([votes[0], votes[1]], dim=1), ef, gap]
                    elif plan.kind == "spec":
                        feat = model.features(xs[0][b0:b0 + n]).permute(0, 2, 3, 1).contiguous()
                        Cc = int(feat.shape[3])
                        if Cc != plan.awidth[0]:
                            raise RuntimeError(f"brainxai.{self.who}: block5 emits {Cc} channels, fc expects {plan.awidth[0]}")
                        gap = torch.empty(n, Cc, dtype=torch.float32, device=dev)
                        L.check(lib.bx_gap_fc_lsm_fwd(_p(feat), _p(model.fc.weight.detach()), _p(model.fc.bias.detach()), _p(gap), _p(logp), n,
                                                      int(feat.shape[1]) * int(feat.shape[2]), Cc, K, ops.bx_dtype(feat.dtype), _stream()), "bx_gap_fc_lsm_fwd")
                        acts = [gap]
                    else:
                        ef = model.features(xs[0][b0:b0 + n]).float().contiguous()
                        if int(ef.shape[1]) != plan.awidth[0]:
                            raise RuntimeError(f"brainxai.{self.who}: EEGNet emits {int(ef.shape[1])} features, dense expects {plan.awidth[0]} (Samples mismatch)")
                        L.check(lib.bx_linear_lsm_fwd(_p(ef), _p(model.dense.weight.detach()), _p(model.dense.bias.detach()), _p(logp), n, int(ef.shape[1]), K,
                                                      _stream()), "bx_linear_lsm_fwd")
                        acts = [ef]
                with _lap(self.profile, "factors"):
                    delta = torch.empty(n, self.ld, dtype=torch.float64, device=dev)
                    loss = torch.empty(n, dtype=torch.float64, device=dev)
                    status = torch.empty(n, dtype=torch.int32, device=dev)
                    multi = plan.kind == "multimodal"
                    L.check(lib.bx_tracin_factors(_p(logp), _p(tgt) if dist else None, None if dist else _p(tgt), _p(hidden) if multi else None,
                                                  _p(votes[0]) if multi else None, _p(votes[1]) if multi else None, _p(self.w1) if multi else None,
                                                  _p(self.w2) if multi else None, _p(delta), _p(loss), _p(status), n, K, Hd,
                                                  L.BX_TRACIN_MULTIMODAL if multi else L.BX_TRACIN_SINGLE, _stream()), "bx_tracin_factors")
                yield n, acts, delta, loss, status

    def check(self, c, status, what):
        """The status words of a checkpoint's rows, read once: raises naming the first flagged example."""
        st = torch.cat(status).cpu().numpy()
        bad = np.flatnonzero(st)
        if bad.size:
            raise ValueError(f"{self.who}: checkpoint {c}: {what} example {int(bad[0])} has {_TRACIN_STATUS.get(int(st[bad[0]]), 'a bad status')}")


def _tracin_common(who, model, checkpoints, layers, learning_rates, top, max_batch, block_rows, top_default):
    plan = _tracin_model(who, model)
    mask, names = _tracin_layers(who, plan, layers)
    cks, rates = _tracin_checkpoints(who, checkpoints, learning_rates)
    max_batch = _max_batch(who, max_batch)
    block_rows = min(_tracin_int(who, "block_rows", block_rows, 1, 1 << 30), _TRACIN_MAX_BLOCK)
    if top is not None or not top_default:
        top = _tracin_int(who, "top", top, 1, _TRACIN_MAX_TOP)
    return plan, mask, names, cks, rates, max_batch, block_rows, top


def _tracin_top(who, top, N):
    if top is not None and top > N:
        raise ValueError(f"{who}: top = {top} outside 1..{min(_TRACIN_MAX_TOP, N)}")


def _tracin_topk(lib, S, N, M, k, largest):
    """-> (idx int64 [M,k], val fp64 [M,k]) of S fp64 [N,M]."""
    dev = S.device
    ws = torch.empty(max(int(lib.bx_tracin_topk_workspace(N, M)), 8) // 8, dtype=torch.int64, device=dev)
    idx = torch.empty(M, k, dtype=torch.int32, device=dev)
    val = torch.empty(M, k, dtype=torch.float64, device=dev)
    L.check(lib.bx_tracin_topk(_p(S), N, M, k, largest, _p(idx), _p(val), _p(ws), ws.numel() * 8, _stream()), "bx_tracin_topk")
    return idx.long(), val


def tracin(model, checkpoints, train, test, *, layers="all", learning_rates=None, top=10, max_batch=256, block_rows=16384, keep_scores=False,
           return_parts=False):
    """Which training examples made the model decide as it does on the test examples: TracIn (Pruthi et al., NeurIPS 2020; Captum's
    influence.TracInCPFast) through the model's last Linear layers, from checkpoints the training loop already writes.
        S[i,j] = sum_c eta_c sum_l (delta_l,i . delta_l,j)(a_l,i . a_l,j + 1)
    the gradient dot product of KLDivLoss(reduction='sum') of training example i and test example j with respect to the weights and
    biases of fc2, fc1, eeg_model.dense and spectrogram_model.fc, exactly: their per-example gradients are outer products, so no
    per-example backward pass runs.  A positive score marks a proponent (a gradient step on i lowers j's loss), a negative one an opponent.

    model:          a MultimodalModel (the un-hooked reference architecture with an EEGNet branch), a Spectrogram_Model or an EEGNet.
    checkpoints:    a non-empty sequence; every entry a state_dict, a dict with a 'state_dict' key (what ``save_checkpoint`` writes) or a
                    path to one (loaded as ``load_checkpoint`` does).  The keys must be the model's.
    train:          (eeg, spec, target) for a MultimodalModel, (x, target) for a stand-alone branch, on the model's device; or a re-iterable
                    of such batches (a DataLoader), walked once per checkpoint, every batch moved to the device.  target: fp32 [n,K]
                    distributions, or integer labels [n].
    test:           the same tensor form, M <= 4096 examples.
    layers:         'all'; 'head' (fc1 and fc2); a sequence out of 'fc2', 'fc1', 'eeg_model.dense', 'spectrogram_model.fc'; 'fc' / 'dense' is
                    the one layer of a stand-alone branch.
    learning_rates: None (all 1) or one finite number per checkpoint.
    top:            proponents and opponents returned per test example, 1..min(256, N).
    max_batch:      rows per forward pass; block_rows: training rows per score launch.  No bit of the result depends on either.
    Eval mode without autograd; forward passes through the model's own kernels, then the factors in closed form (bx_tracin_factors), one
    tiled fp64 launch per block of training rows against all test rows (bx_tracin_scores) and an exact radix select per test example
    (bx_tracin_topk).  Every parameter and buffer of the model is copied on the device first and restored bit for bit in a ``finally``;
    the training flag and every requires_grad likewise.  Returns (proponents, opponents), int64 [M,top] each, or ``TracInResult`` with
    return_parts."""
    return _tracin(model, checkpoints, train, test, layers, learning_rates, top, max_batch, block_rows, keep_scores, return_parts)


def _tracin(model, checkpoints, train, test, layers, learning_rates, top, max_batch, block_rows, keep_scores, return_parts, profile=None):
    """``tracin`` itself.  profile: None, or a list that receives (phase, start event, end event) with phase in 'forward', 'factors',
    'scores', 'topk' -- device events around every phase (tools/tracin_bench.py sums them)."""
    # ---- everything that can be refused is refused here, before the library is touched ----
    who = "tracin"
    plan, mask, names, cks, rates, max_batch, block_rows, top = _tracin_common(who, model, checkpoints, layers, learning_rates, top, max_batch, block_rows, False)
    N, train_iter = _tracin_data(who, plan, train, "train", False)
    M, _ = _tracin_data(who, plan, test, "test", True)
    if M > _TRACIN_MAX_M:
        raise ValueError(f"{who}: {M} test examples, supported 1..{_TRACIN_MAX_M}")
    if N is not None:
        _tracin_top(who, top, N)
        if N * M >= 1 << 31:
            raise ValueError(f"{who}: N * M = {N * M} scores, supported below 2^31; use fewer test examples per call")
    _need_gpu(who, "the model, train and test", model, *test, *(train if train_iter is None else ()))

    dev = next(model.parameters()).device
    Cn = len(cks)
    with torch.cuda.device(dev), _eval_frozen(model), torch.no_grad(), _TracinWalk(who, model, plan, cks, max_batch, profile) as walk:
        lib = walk.lib
        S = None if N is None else torch.empty(N, M, dtype=torch.float64, device=dev)
        train_losses, test_losses = [], []
        for c in range(Cn):
            walk.load(c)
            parts = list(walk.passes(test, "test"))
            t_acts = [torch.cat([p[1][l] for p in parts]) for l in range(len(plan.names))]
            t_delta, t_status = torch.cat([p[2] for p in parts]), [p[4] for p in parts]
            test_losses.append(torch.cat([p[3] for p in parts]))
            t_side = walk.side(t_delta, t_acts, M)
            blocks, pend, npend, row0, losses, status = [], [], 0, 0, [], []

            def flush():
                nonlocal pend, npend, row0
                acts = [torch.cat([p[0][l] for p in pend]) for l in range(len(plan.names))]
                delta = torch.cat([p[1] for p in pend])
                out, n_all, r0 = (S, N, row0) if S is not None else (torch.empty(npend, M, dtype=torch.float64, device=dev), npend, 0)
                with _lap(profile, "scores"):
                    L.check(lib.bx_tracin_scores(C.byref(walk.side(delta, acts, npend)), C.byref(t_side), C.byref(walk.shape), _p(out), n_all, r0, rates[c],
                                                 1 if c == 0 else 0, mask, _stream()), "bx_tracin_scores")
                if S is None:
                    blocks.append(out)
                row0 += npend
                pend, npend = [], 0

            for n, acts, delta, loss, st in walk.passes(train if train_iter is None else train_iter, "train"):
                losses.append(loss)
                status.append(st)
                o = 0
                while o < n:
                    take = min(n - o, block_rows - npend)
                    if N is not None and row0 + npend + take > N:
                        raise ValueError(f"{who}: train yields more than the {N} examples of its first pass at checkpoint {c}")
                    pend.append(([a[o:o + take] for a in acts], delta[o:o + take]))
                    npend += take
                    o += take
                    if npend == block_rows:
                        flush()
            if npend:
                flush()
            if S is None:
                if not blocks:
                    raise ValueError(f"{who}: train yields no batches")
                S = torch.cat(blocks)
                N = int(S.shape[0])
                _tracin_top(who, top, N)
                if N * M >= 1 << 31:
                    raise ValueError(f"{who}: N * M = {N * M} scores, supported below 2^31; use fewer test examples per call")
            elif row0 != N:
                raise ValueError(f"{who}: train yields {row0} examples at checkpoint {c}, {N} in its first pass")
            train_losses.append(torch.cat(losses))
            walk.check(c, t_status, "test")
            walk.check(c, status, "training")
        with _lap(profile, "topk"):
            pro, pro_s = _tracin_topk(lib, S, N, M, top, 1)
            opp, opp_s = _tracin_topk(lib, S, N, M, top, 0)
    if not return_parts:
        return pro, opp
    return TracInResult(pro, pro_s, opp, opp_s, S if keep_scores else None, torch.stack(train_losses), torch.stack(test_losses), names, tuple(rates), N)


def self_influence(model, checkpoints, train, *, layers="all", learning_rates=None, top=None, max_batch=256, block_rows=16384, return_parts=False):
    """The influence of every training example on itself, self[i] = sum_c eta_c sum_l |delta_l,i|^2 (|a_l,i|^2 + 1): ``tracin``'s score of
    (i, i), bit for bit.  Examples the model fights against -- mislabelled ones first -- have the largest values.  The arguments are
    ``tracin``'s (block_rows is accepted for symmetry; a row needs no partner).  Returns fp64 [N] on the device; with ``top`` also the
    indices int64 [top] of the most self-influential examples (bx_tracin_topk), as (self_influence, top); ``SelfInfluenceResult`` with
    return_parts."""
    return _self_influence(model, checkpoints, train, layers, learning_rates, top, max_batch, block_rows, return_parts)


def _self_influence(model, checkpoints, train, layers, learning_rates, top, max_batch, block_rows, return_parts, profile=None):
    who = "self_influence"
    plan, mask, names, cks, rates, max_batch, block_rows, top = _tracin_common(who, model, checkpoints, layers, learning_rates, top, max_batch, block_rows, True)
    N, train_iter = _tracin_data(who, plan, train, "train", False)
    if N is not None:
        _tracin_top(who, top, N)
        if N >= 1 << 31:
            raise ValueError(f"{who}: N = {N} examples, supported below 2^31")
    _need_gpu(who, "the model and train", model, *(train if train_iter is None else ()))

    dev = next(model.parameters()).device
    with torch.cuda.device(dev), _eval_frozen(model), torch.no_grad(), _TracinWalk(who, model, plan, cks, max_batch, profile) as walk:
        lib = walk.lib
        out = None if N is None else torch.empty(N, dtype=torch.float64, device=dev)
        train_losses = []
        for c in range(len(cks)):
            walk.load(c)
            row0, chunks, losses, status = 0, [], [], []
            for n, acts, delta, loss, st in walk.passes(train if train_iter is None else train_iter, "train"):
                losses.append(loss)
                status.append(st)
                if out is not None and row0 + n > N:
                    raise ValueError(f"{who}: train yields more than the {N} examples of its first pass at checkpoint {c}")
                dst, n_all, r0 = (out, N, row0) if out is not None else (torch.empty(n, dtype=torch.float64, device=dev), n, 0)
                with _lap(profile, "scores"):
                    L.check(lib.bx_tracin_self(C.byref(walk.side(delta, acts, n)), C.byref(walk.shape), _p(dst), n_all, r0, rates[c], 1 if c == 0 else 0, mask,
                                               _stream()), "bx_tracin_self")
                if out is None:
                    chunks.append(dst)
                row0 += n
            if out is None:
                if not chunks:
                    raise ValueError(f"{who}: train yields no batches")
                out = torch.cat(chunks)
                N = int(out.shape[0])
                _tracin_top(who, top, N)
            elif row0 != N:
                raise ValueError(f"{who}: train yields {row0} examples at checkpoint {c}, {N} in its first pass")
            train_losses.append(torch.cat(losses))
            walk.check(c, status, "training")
        idx = val = None
        if top is not None:
            with _lap(profile, "topk"):
                idx, val = _tracin_topk(lib, out, N, 1, top, 1)
                idx, val = idx[0], val[0]
    if return_parts:
        return SelfInfluenceResult(out, idx, val, torch.stack(train_losses), names, tuple(rates), N)
    return out if top is None else (out, idx)
