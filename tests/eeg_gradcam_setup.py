"""The EEG-branch Grad-CAM setting shared by tests/test_gpu_eeg_gradcam.py, tests/test_gpu_cam_methods.py and tests/test_gpu_heads.py:
targets, BatchNorm statistics away from identity, inputs and the relative error."""
import torch

from oracle import ref_torch as O

TARGETS = ("conv1", "depthwiseConv", "separableConv")


def bn_nontrivial(eeg_net, seed):
    """BatchNorm running statistics and affine parameters far from identity, so that every s_k / h_k enters the maps."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name in ("batchnorm1", "batchnorm2", "batchnorm3"):
            bn = getattr(eeg_net, name)
            n = bn.num_features
            bn.running_mean.copy_(torch.rand(n, generator=g) * 1.0 - 0.5)
            bn.running_var.copy_(torch.rand(n, generator=g) * 2.8 + 0.2)
            bn.weight.copy_(torch.rand(n, generator=g) * 1.7 + 0.3)
            bn.bias.copy_(torch.rand(n, generator=g) * 1.0 - 0.5)


def rel(a, b, scale=None):
    """max |a - b| over ``scale`` (default: max |b|), in fp64 on the host."""
    b = b.detach().double()
    scale = float(b.abs().max()) if scale is None else scale
    return float((a.detach().cpu().double() - b).abs().max()) / (scale + 1e-30)


def inputs(B, chans, samples, seed=11):
    return O.seeded((B, 1, chans, samples), seed, "randn"), O.seeded((B, 4, 32, 64), seed + 1, "rand")
