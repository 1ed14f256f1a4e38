"""What include/brainxai.h pins for the class-activation reduces, the last-stage heads, the bilinear resize and the saliency reduce,
restated with numpy and torch on the CPU -- what tests/test_gpu_attrib_kernels.py holds bx_cam_reduce, bx_cam_head, bx_cam_head_sweep,
bx_resize_bilinear and bx_saliency_reduce to.  Nothing here imports the package under test.

Every function computes in the dtype of its inputs: float64 inputs give the reference, float32 inputs the same definition in plain
float32 (tests/test_attrib_ref_cpu.py measures one against the other: the rounding a correct fp32 kernel may show)."""
import types

import numpy as np
import torch

from tests.scorecam_ref import upsample as resize_f32      # noqa: F401  (the float32 restatement of the same resize; re-exported)

EPS = 1e-6                     # part of the Grad-CAM++ definition


# ---- channel reduces ------------------------------------------------------------------------------------------------------------
def cam(A, G, method):
    """A, G [B, K, *spatial] -> (raw [B, *spatial], w [B, K] or None, worst conditioning of a counted element, the largest
    |S G| of a counted element).  method: "gradcam", "gradcam++" or "layercam"."""
    dims = tuple(range(2, A.dim()))
    if method == "layercam":
        return (G.clamp_min(0) * A).sum(1), None, 1.0, 0.0
    if method == "gradcam":
        w = G.mean(dims)
        return (w.reshape(*w.shape, *([1] * len(dims))) * A).sum(1), w, 1.0, 0.0
    assert method == "gradcam++", method
    S = A.sum(dims, keepdim=True)
    den = 2 * G ** 2 + S * G ** 3 + EPS
    alpha = torch.where(G == 0, torch.zeros_like(G), G ** 2 / den)
    w = (G.clamp_min(0) * alpha).sum(dims)
    counted = G > 0
    cond = (den.abs() / (2 * G ** 2 + (S * G ** 3).abs() + EPS))[counted]
    sg = (S * G).abs()[counted]
    raw = (w.reshape(*w.shape, *([1] * len(dims))) * A).sum(1)
    return raw, w, float(cond.min()) if cond.numel() else 1.0, float(sg.max()) if sg.numel() else 0.0


# ---- the heads ------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(shape, bound, g):
    return (torch.rand(shape, generator=g) * 2 - 1) * bound


class _LogSoftmax(torch.autograd.Function):
    """LogSoftmax over dim 1 whose backward forms 1 - p_n as the sum of the OTHER probabilities:
        dz_n = dy_n sum_{j != n} p_j - p_n sum_{j != n} dy_j.
    torch's own backward, dy - p sum(dy), cancels in fp64 too: once p_n > 1 - 1e-16 it returns dz_n = 0 where the true value is
    -sum_{j != n} p_j (the confident regime of tests/test_gpu_heads.py reaches p_n = 1 - e^-45, and a two-class model at 1 - 1.6e-6
    already costs the fp32 oracle 1e-2 of its Grad-CAM weights)."""

    @staticmethod
    def forward(ctx, z):
        y = z - torch.logsumexp(z, dim=1, keepdim=True)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        p = y.exp()
        off = 1.0 - torch.eye(y.shape[1], dtype=y.dtype)                 # off[n, j] = (j != n)
        return dy * (p @ off.T) - p * (dy @ off.T)


def _lsm(z):
    return _LogSoftmax.apply(z)


def _fusion_ref(e, s, w1, b1, w2, b2):
    return _lsm(torch.relu(torch.cat((e, s), 1) @ w1.T + b1) @ w2.T + b2)


def head(A, eeg, fcw, fcb, w1, b1, w2, b2, class_mode, method="gradcam", dtype=torch.float64):
    """The last stage of the multimodal model and its class-activation maps, by the GENERAL definition: the two heads run forward in
    ``dtype``, autograd gives G = d score / dA for every requested class, and cam(A, G, method) reduces it (the kernel instead uses
    that G is the same at every position; tests/test_attrib_ref_cpu.py shows the two agree).

    A [B, HW, C] channels-last, the stored values.  eeg: the EEG branch's log-probabilities [B, N], or (eeg_feat [B, Fe], dense_w
    [N, Fe], dense_b [N]) for the dense layer + LogSoftmax in front of them.  class_mode -2: every class (maps ordered sample-major,
    class-minor), -1: the sample's arg-max class (the FIRST maximum), >= 0: that class.
    -> namespace(out [B, N], raw [B*nm, HW], cam = max(raw, 0), w [B*nm, C] or None, cond, sg (the Grad-CAM++ conditioning figures of
    cam), margin: the smallest |pre-activation| of the fusion head's hidden layer -- a ReLU decision an fp32 kernel could take the
    other way -- and, for class_mode -1, lead: the smallest lead of the arg-max log-probability over the runner-up)."""
    t = lambda x: x.detach().to(dtype)                                   # noqa: E731
    Ad = t(A).requires_grad_(True)
    B, HW, C = Ad.shape
    s = _lsm(Ad.mean(1) @ t(fcw).T + t(fcb))
    e = _lsm(t(eeg[0]) @ t(eeg[1]).T + t(eeg[2])) if isinstance(eeg, (tuple, list)) else t(eeg)
    pre = torch.cat((e, s), 1) @ t(w1).T + t(b1)
    out = _lsm(torch.relu(pre) @ t(w2).T + t(b2))
    N = out.shape[1]
    if class_mode == -2:
        scores = [out[:, c].sum() for c in range(N)]
    elif class_mode == -1:
        scores = [out.gather(1, out.argmax(1, keepdim=True)).sum()]      # torch.argmax: the first maximum
    else:
        scores = [out[:, int(class_mode)].sum()]
    At = Ad.detach().permute(0, 2, 1)                                     # [B, C, HW]
    raws, ws, conds, sgs = [], [], [], []
    for sc in scores:
        (G,) = torch.autograd.grad(sc, Ad, retain_graph=True)
        raw, w, cond, sg = cam(At, G.permute(0, 2, 1), method)
        raws.append(raw); ws.append(w); conds.append(cond); sgs.append(sg)
    raw = torch.stack(raws, 1).reshape(B * len(scores), HW)
    top = out.detach().topk(min(2, N), 1).values
    return types.SimpleNamespace(out=out.detach(), raw=raw, cam=raw.clamp_min(0),
                                 w=None if ws[0] is None else torch.stack(ws, 1).reshape(B * len(scores), C),
                                 cond=min(conds), sg=max(sgs), margin=float(pre.detach().abs().min()),
                                 lead=float((top[:, 0] - top[:, 1]).min()) if N > 1 else float("inf"))


# ---- resize -----------------------------------------------------------------------------------------------------------------------
def _axis64(n_out, n_in):
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def resize(src, H, W):
    """[..., h, w] -> float64 [..., H, W]: bilinear, align_corners=False, no antialiasing; values and coordinates in fp64."""
    A = np.asarray(src, dtype=np.float64)
    y0, y1, ly = _axis64(H, A.shape[-2])
    x0, x1, lx = _axis64(W, A.shape[-1])
    ly = ly[:, None]
    r0, r1 = A[..., y0, :], A[..., y1, :]
    top = (1.0 - lx) * r0[..., x0] + lx * r0[..., x1]
    bot = (1.0 - lx) * r1[..., x0] + lx * r1[..., x1]
    return (1.0 - ly) * top + ly * bot


# ---- saliency ---------------------------------------------------------------------------------------------------------------------
def saliency(g, C, scale):
    """g [..., Cs] -> float64 [...]: scale * max over the first C channels of |g|."""
    return np.float64(scale) * np.abs(np.asarray(g, dtype=np.float64)[..., :C]).max(axis=-1)
