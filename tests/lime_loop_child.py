"""Run by tests/test_gpu_lime.py::test_training_loop_explains_every_nth_epoch in a process of its own (argument: a scratch directory).
train_and_validate_combined on a two-batch toy loader, epochs = 4, n = 2: explain_fn is called after epochs 2 and 4 with the
explanation of that epoch's weights (equal, bit for bit, to lime_image on the checkpoint just written); a run with explain_fn and a
run without it from the same seeds return the same histories and the same final state_dict bit for bit; a bare image is cut into
8 x 8 tiles.  Exit code 0 and a last line 'lime_loop_child: ok' when every assertion held."""
import os
import pathlib
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import brainxai  # noqa: E402
from brainxai import ops  # noqa: E402
from oracle import ref_torch as O  # noqa: E402

DEV = torch.device("cuda:0")


def _toy_loader(n_batches, b, seed):
    out = []
    for i in range(n_batches):
        eeg = O.seeded((b, 1, 19, 2000), seed + 10 * i, "randn")
        spec = O.seeded((b, 4, 64, 128), seed + 10 * i + 1, "rand")
        lab = F.one_hot(torch.randint(0, 6, (b,), generator=torch.Generator().manual_seed(seed + 10 * i + 2)), 6).float()
        out.append(((eeg, spec), lab))
    return out


def _same_bits(a, b):
    assert np.array_equal(a.masks, b.masks) and torch.equal(a.probs, b.probs) and np.array_equal(a.weights, b.weights)
    assert a.top_labels == b.top_labels and a.local_exp == b.local_exp
    assert a.intercept == b.intercept and a.score == b.score and a.local_pred == b.local_pred


def main(tmp_path):
    img = (np.random.default_rng(17).random((64, 128, 4)) * 255.9).astype(np.uint8)
    seg = brainxai.grid_segments(64, 128, 4, 8)
    seen = []

    def run(sub, explain_fn, sample):
        torch.manual_seed(3)
        ops.manual_seed(1234, DEV)                                  # the dropout counters restart with every run
        net = brainxai.build_multimodal(19, 2000, 4, dropout=0.5).to(DEV)
        opt = brainxai.FlatAdamW(net.parameters(), lr=1e-3)
        try:
            hist = brainxai.train_and_validate_combined(net, _toy_loader(2, 8, 300), _toy_loader(1, 8, 400), 4, opt, brainxai.KLDivLoss(), DEV,
                                                        str(tmp_path / sub), n=2, sample_spectrogram=sample, explain_fn=explain_fn)
        finally:
            ops.clear_grad_views()
        return hist, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}

    def explain_fn(epoch, exp):
        shutil.copy(tmp_path / "with" / "combined_checkpoint.pth.tar", tmp_path / f"epoch{epoch}.pth.tar")
        seen.append((epoch, exp))
    hist_a, sd_a = run("with", explain_fn, (img, seg))
    hist_b, sd_b = run("without", None, (img, seg))
    assert [e for e, _ in seen] == [2, 4]
    assert hist_a == hist_b, "the explanation must not disturb the training trajectory"
    assert sd_a.keys() == sd_b.keys() and all(torch.equal(sd_a[k], sd_b[k]) for k in sd_a)
    for epoch, exp in seen:
        ck = torch.load(tmp_path / f"epoch{epoch}.pth.tar", map_location="cpu", weights_only=False)
        assert ck["epoch"] == epoch
        fresh = brainxai.build_multimodal(19, 2000, 4, dropout=0.5)
        fresh.load_state_dict(ck["state_dict"])
        _same_bits(exp, brainxai.lime_image(fresh.to(DEV), img, seg))
    seen.clear()
    run("bare", lambda epoch, exp: seen.append((epoch, exp)), img)
    assert [e for e, _ in seen] == [2, 4] and np.array_equal(seen[0][1].segments, brainxai.grid_segments(64, 128, 8, 8))
    torch.cuda.synchronize()
    print("lime_loop_child: ok", flush=True)


if __name__ == "__main__":
    main(pathlib.Path(sys.argv[1]))
