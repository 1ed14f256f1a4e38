"""GPU: Grad-CAM at the EEG branch's convolutions (eeg_model.conv1 / depthwiseConv / separableConv) through bx_eeg_gradcam,
against the oracle's forward-hook Grad-CAM on the same weights."""
import pytest
import torch
import torch.nn.functional as F

import brainxai
from oracle import ref_torch as O
from tests.eeg_gradcam_setup import TARGETS, bn_nontrivial, inputs, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3                     # north_star: 1e-3 relative fp32


def _mm_pair(chans, samples, seed=5, kern=64):
    ref = O.build_multimodal(chans, samples, 4, dropout=0.0)
    if kern != 64:
        ref.eeg_model = O.EEGNet(6, Chans=chans, Samples=samples, dropoutRate=0.0, kernLength=kern)
    O.fill_params(ref, seed=seed)
    bn_nontrivial(ref.eeg_model, seed + 1)
    mine = brainxai.build_multimodal(chans, samples, 4, dropout=0.0)
    if kern != 64:
        mine.eeg_model = brainxai.EEGNet(6, Chans=chans, Samples=samples, dropoutRate=0.0, kernLength=kern)
    mine.load_state_dict(ref.state_dict())
    return ref, mine.to(DEV)


class _Two(torch.nn.Module):
    """A stand-alone EEG net in the oracle's two-argument calling convention."""

    def __init__(self, net):
        super().__init__()
        self.eeg_model = net

    def forward(self, eeg, _spec):
        return self.eeg_model(eeg)


def _check(ref, mine, eeg, spec, target, class_idx):
    """Product raw / weights within TOL of the oracle's; cam on the scale of raw."""
    cam_r, raw_r, w_r, A_r, _ = O.grad_cam(ref, eeg, spec, "eeg_model." + target, class_idx, upsample=False, return_parts=True)
    cam, raw, w, A, _ = brainxai.grad_cam(mine, eeg.to(DEV), spec.to(DEV), "eeg_model." + target, class_idx, upsample=False, return_parts=True)
    torch.cuda.synchronize()
    want = tuple(raw_r.shape)
    assert tuple(raw.shape) == want and tuple(cam.shape) == want and tuple(w.shape) == tuple(w_r.shape)
    rs = float(raw_r.abs().max())
    e_raw, e_cam, e_w = rel(raw, raw_r), rel(cam, cam_r, rs), rel(w, w_r)
    assert max(e_raw, e_cam, e_w) < TOL, (target, class_idx, e_raw, e_cam, e_w)
    if target == "conv1":
        assert A is None
    else:
        assert tuple(A.shape) == tuple(A_r.shape) and rel(A, A_r) < TOL


@pytest.fixture(scope="module")
def bench_pair():
    return _mm_pair(19, 2000)


@pytest.mark.parametrize("class_idx", [None, 3, "all"])
@pytest.mark.parametrize("target", TARGETS)
def test_eeg_gradcam_matches_oracle(bench_pair, target, class_idx):
    ref, mine = bench_pair
    eeg, spec = inputs(2, 19, 2000)
    _check(ref, mine, eeg, spec, target, class_idx)


@pytest.mark.parametrize("chans,samples,B", [(19, 2100, 2), (5, 300, 1), (37, 3000, 2), (3, 1030, 2), (2, 40, 1)])
def test_eeg_gradcam_pool_tails_and_native_geometry(chans, samples, B):
    # 2100 and 300: T//4 is not a multiple of 8, so the second pooling drops a tail (T2*P2 < T1)
    # 1030: T % 4 = 2 (scalar stores in the conv1 map kernel, no 16-byte dmap loads), T1 = 257 (a second tile with one live step),
    #       T2 P2 = 256 < T1, T1 P1 = 1028 < T, and a second conv1 workgroup of six steps
    # 40:   T1 = 10, T2 = 1: one pooled column, fewer steps than threads everywhere, the tile halo mostly outside the row
    ref, mine = _mm_pair(chans, samples, seed=7)
    eeg, spec = inputs(B, chans, samples, seed=13)
    for target in TARGETS:
        _check(ref, mine, eeg, spec, target, "all")


def test_eeg_gradcam_kernlength_32():
    # a 32-tap conv1 takes the layer-by-layer evaluation path (its arena also holds the conv1 output)
    ref, mine = _mm_pair(19, 2000, seed=9, kern=32)
    eeg, spec = inputs(2, 19, 2000, seed=17)
    for target in TARGETS:
        _check(ref, mine, eeg, spec, target, "all")


def test_eeg_gradcam_bench_batch(bench_pair):
    ref, mine = bench_pair
    eeg, spec = inputs(64, 19, 2000, seed=19)
    for target in TARGETS:
        _check(ref, mine, eeg, spec, target, None)


@pytest.mark.parametrize("cls", ["EEGNet", "EEGNetAttentionDeep"])
def test_eeg_gradcam_standalone_nets(cls):
    chans, samples = 19, 2048
    ref_net = O.fill_params(getattr(O, cls)(6, Chans=chans, Samples=samples, dropoutRate=0.0), seed=21)
    bn_nontrivial(ref_net, 22)
    mine = getattr(brainxai, cls)(6, Chans=chans, Samples=samples, dropoutRate=0.0)
    mine.load_state_dict(ref_net.state_dict())
    mine.to(DEV)
    ref = _Two(ref_net)
    eeg = O.seeded((2, 1, chans, samples), 23, "randn")
    for target in TARGETS:
        for class_idx in (None, "all"):
            cam_r, raw_r, w_r, _, _ = O.grad_cam(ref, eeg, None, "eeg_model." + target, class_idx, upsample=False, return_parts=True)
            # the prefix is optional for a stand-alone net
            cam, raw, w, _, _ = brainxai.grad_cam(mine, eeg.to(DEV), None, target, class_idx, upsample=False, return_parts=True)
            rs = float(raw_r.abs().max())
            errs = (rel(raw, raw_r), rel(cam, cam_r, rs), rel(w, w_r))
            assert max(errs) < TOL, (cls, target, class_idx, errs)


def test_eeg_gradcam_upsample(bench_pair):
    _, mine = bench_pair
    eeg, spec = (t.to(DEV) for t in inputs(2, 19, 2000, seed=29))
    small = brainxai.grad_cam(mine, eeg, spec, "eeg_model.separableConv", "all", upsample=False)
    up = brainxai.grad_cam(mine, eeg, spec, "eeg_model.separableConv", "all", upsample=True)
    assert tuple(small.shape) == (2, 6, 1, 500) and tuple(up.shape) == (2, 6, 1, 2000)
    want = F.interpolate(small.cpu().reshape(12, 1, 1, 500), size=(1, 2000), mode="bilinear", align_corners=False).reshape(up.shape)
    assert rel(up, want) <= 1e-6
    for target in ("conv1", "depthwiseConv"):
        a = brainxai.grad_cam(mine, eeg, spec, "eeg_model." + target, 3, upsample=False)
        b = brainxai.grad_cam(mine, eeg, spec, "eeg_model." + target, 3, upsample=True)
        assert a.shape == b.shape and torch.equal(a, b)


def test_eeg_gradcam_bf16_storage():
    ref, mine32 = _mm_pair(19, 2000, seed=31)
    mine16 = brainxai.build_multimodal(19, 2000, 4, dropout=0.0)
    mine16.load_state_dict(ref.state_dict())
    brainxai.set_compute_dtype(mine16, torch.bfloat16)
    mine16.to(DEV)
    eeg, spec = (t.to(DEV) for t in inputs(2, 19, 2000, seed=37))
    for target in TARGETS:
        _, r32, *_ = brainxai.grad_cam(mine32, eeg, spec, "eeg_model." + target, "all", upsample=False, return_parts=True, relu=False)
        _, r16, *_ = brainxai.grad_cam(mine16, eeg, spec, "eeg_model." + target, "all", upsample=False, return_parts=True, relu=False)
        assert rel(r16, r32.cpu()) <= 2e-2, target     # the bound the bf16 Grad-CAM of the spectrogram branch is held to


def test_eeg_gradcam_restores_state_and_leaves_spectrogram_path(bench_pair):
    _, mine = bench_pair
    eeg, spec = (t.to(DEV) for t in inputs(2, 19, 2000, seed=41))
    mine.train()
    mine.fc1.weight.requires_grad_(False)
    flags = [p.requires_grad for p in mine.parameters()]
    before = brainxai.grad_cam(mine, eeg, spec, "spectrogram_model.block5", "all").clone()
    for target in TARGETS:
        brainxai.grad_cam(mine, eeg, spec, "eeg_model." + target, "all")
        assert mine.training and all(m.training for m in mine.modules())
        assert [p.requires_grad for p in mine.parameters()] == flags
    after = brainxai.grad_cam(mine, eeg, spec, "spectrogram_model.block5", "all")
    assert torch.equal(before, after)
    mine.fc1.weight.requires_grad_(True)
    mine.eval()


def test_eeg_gradcam_generic_geometry_raises():
    net = brainxai.EEGNet(6, Chans=19, Samples=2000, dropoutRate=0.0, F1=4, D=3, F2=8, kernLength=128).to(DEV)
    with pytest.raises(ValueError, match="F1=8"):
        brainxai.grad_cam(net, torch.randn(2, 1, 19, 2000, device=DEV), None, "eeg_model.conv1")
