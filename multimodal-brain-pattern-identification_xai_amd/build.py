"""Build libbrainxai.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbrainxai.so")
SOURCES = ["core.hip", "conv3x3.hip", "conv3x3_mfma.hip", "conv3x3_split.hip", "tail.hip", "heads.hip", "eeg.hip", "eeg_generic.hip", "eeg_mfma.hip", "eeg_collapse.hip", "eeg_deep.hip", "eeg_cam.hip", "attrib.hip", "montage.hip", "specprep.hip", "lime.hip", "faith.hip", "rise.hip", "scorecam.hip", "occlusion.hip", "shap.hip", "expgrad.hip", "smoothgrad.hip", "infidelity.hip", "blurig.hip", "spectral.hip", "similarity.hip", "guided_ig.hip", "fusion_shap.hip", "maskopt.hip", "tcav.hip", "tracin.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=fast", "-Wall", "-Wno-unused-function"]
# No packed-fp32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32), round 3.  Found with the EEG branch running beside the
# spectrogram branch (ops.OVERLAP_EEG): k_eeg_sep, whose inner loop hipcc had vectorised into v_pk_fma_f32, returned wrong LOW halves of
# a few result pairs whenever kernels of the other branch shared its CUs (128 of 200 graph replays of the forward differed from the
# serial run, 0 of 200 with scalar v_fmac_f32; tools/overlap_fwd_check.py) -- alone on the chip the same code never failed.  Every
# parity test stands (hipcc contracts a few multiply-adds differently without the packed forms, so results are not bit-identical to
# the packed build's, only equally accurate), and the step time did not move.
# (The host pass of hipcc does not know the feature and says so once per file; build() drops that line.)
if os.environ.get("BX_PACKED_FP32", "0") != "1":
    FLAGS += ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# per-file additions (later flags win): the montage IIR must round every product and sum separately, as scipy's C loop does; the RISE
# mask value and base + m * (x - base) likewise, so that a numpy float32 restatement matches them bit for bit; Score-CAM's up-sampled
# activation planes, masks and rows for the same reason; the expected-gradients interpolants bg + alpha * (x - bg) likewise; SmoothGrad's
# Box-Muller, x + sigma * z and the four fp64 operations of the variance likewise; infidelity's x - sigma * z, x + radius * u and the fp64
# operations of beta * d - drop likewise; Blur IG's filters are explicit fmaf chains and its accumulate's g * D, w * (g * D) and sum three
# separate fp64 roundings; the spectral accumulate's w * g and sum likewise (its transforms name their fma); the randomization test's
# draws bound * u and the fp64 sums of the map correlations and of SSIM likewise; Guided IG's points base + alpha * (x - base), its moves
# x + gamma * (X_max - x) and its attr += (x - x_old) * g likewise; Fusion SHAP names every fmaf of the head, and the Shapley sum's
# w * (v(S + i) - v(S)) and its running sum are separate fp64 roundings; the optimised masks' up-sampling, base + M * (x - base), the
# fp64 footprint sums w * t, the regularisers and every operation of the Adam step likewise; TCAV's fits, vectors and dot products round every
# product and sum on their own and its Gram matrix names its fma; TracIn's factors, its exp and log and its pairwise sums likewise
EXTRA_FLAGS = {"tracin.hip": ["-ffp-contract=off"], "tcav.hip": ["-ffp-contract=off"], "fusion_shap.hip": ["-ffp-contract=off"], "maskopt.hip": ["-ffp-contract=off"],
"montage.hip": ["-ffp-contract=off"], "specprep.hip": ["-ffp-contract=off"], "rise.hip": ["-ffp-contract=off"],
               "scorecam.hip": ["-ffp-contract=off"], "expgrad.hip": ["-ffp-contract=off"], "smoothgrad.hip": ["-ffp-contract=off"],
               "infidelity.hip": ["-ffp-contract=off"], "blurig.hip": ["-ffp-contract=off"], "spectral.hip": ["-ffp-contract=off"],
               "similarity.hip": ["-ffp-contract=off"], "guided_ig.hip": ["-ffp-contract=off"]}



def _digest():
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)) + ["../../include/brainxai.h"]:
        p = os.path.join(CSRC, name)
        if os.path.isfile(p) and (p.endswith(".hip") or p.endswith(".h")):
            h.update(name.encode())
            h.update(open(p, "rb").read())
    h.update((" ".join(FLAGS) + repr(sorted(EXTRA_FLAGS.items()))).encode())
    return h.hexdigest()


def build(force=False, verbose=True):
    stamp = LIB + ".stamp"
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read() == dig:
        return LIB
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(HERE, "build", src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [HIPCC, *FLAGS, *EXTRA_FLAGS.get(src, []), "-c", os.path.join(CSRC, src), "-o", obj]
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            failed = True
            sys.stderr.write(f"--- hipcc failed on {src} ---\n{out}\n")
        else:
            out = "\n".join(l for l in out.splitlines() if "is not a recognized feature for this target" not in l)
            if verbose and out.strip():
                sys.stderr.write(f"--- hipcc warnings for {src} ---\n{out}\n")
    if failed:
        raise RuntimeError("libbrainxai build failed")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB])
    open(stamp, "w").write(dig)
    if verbose:
        print(f"built {LIB}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
