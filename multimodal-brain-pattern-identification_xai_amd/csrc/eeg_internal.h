// EEGNet kernels' shared host-side layout: the register-tiled family's geometry and the saved-for-backward arena that
// bx_eeg_features_fwd fills (eeg.hip) and later passes read (eeg.hip backward, eeg_cam.hip Grad-CAM).  Internal to the library.
#pragma once
#include "bx_common.h"

#define EEG_TT 256           // time steps per workgroup in the temporal conv
#define EEG_MAXK 64
#define EEG_MAXF 16          // F1*D and F2 upper bound
#define EEG_MAXCH 64
#define EEG_MAXT 15000       // longest row the tuned FORWARD's one-row LDS tile holds (evaluation-mode passes nothing differentiates: inference,
                             // Grad-CAM); a pass that a backward can follow is tuned only while eeg_tuned_bwd_holds(), see eeg_tuned()
#define EEG_DX_MAX 16        // dx values a thread of k_eeg_conv1_bwd can own: T <= 256 * EEG_DX_MAX
#define EEG_LDS_MAX ((size_t)160 * 1024)      // dynamic LDS a tuned backward kernel may ask for
#define EEGC_RS_BYTES ((size_t)(64 * 64 + 64) * sizeof(double))

struct EegGeom {
  int B, Ch, T, F1, D, FD, F2, K1, K2, P1, P2, T1, T2, padl1, padl2;
  size_t off_c1, off_d, off_p1, off_s, off_stats, total;   // saved arena (bytes)
};
static int eeg_geom(const bxEegDesc* d, EegGeom* g) {
  g->B = d->B; g->Ch = d->Chans; g->T = d->T; g->F1 = d->F1; g->D = d->D; g->FD = d->F1 * d->D; g->F2 = d->F2;
  g->K1 = d->K1; g->K2 = d->K2; g->P1 = d->P1; g->P2 = d->P2;
  if (d->B <= 0 || d->Chans <= 0 || d->T <= 0) return -1;
  if (d->F1 != 8 || g->FD != 16 || d->F2 != 16) return -2;          // register-tiled for the EEGNet-8,2 family
  if (d->K1 < 1 || d->K1 > EEG_MAXK || d->K2 != 16) return -3;
  if (d->Chans > EEG_MAXCH || d->P1 < 1 || d->P2 < 1) return -4;
  g->T1 = d->T / d->P1; g->T2 = g->T1 / d->P2;
  if (g->T2 < 1) return -5;
  g->padl1 = (d->K1 - 1) / 2; g->padl2 = (d->K2 - 1) / 2;
  size_t o = 0;
  {   // conv1 output, or (collapsed front end) the input's sufficient statistics R[64][64], S[64] in fp64
    size_t c1b = (size_t)g->B * g->F1 * g->Ch * g->T * bx_esize(d->dtype);
    if (c1b < EEGC_RS_BYTES) c1b = EEGC_RS_BYTES;
    g->off_c1 = o; o += bx_align_up(c1b, 256);
  }
  g->off_d = o;  o += bx_align_up((size_t)g->B * g->FD * g->T * 4, 256);
  g->off_p1 = o; o += bx_align_up((size_t)g->B * g->FD * g->T1 * 4, 256);
  g->off_s = o;  o += bx_align_up((size_t)g->B * g->F2 * g->T1 * 4, 256);
  g->off_stats = o; o += bx_align_up((size_t)4 * (g->F1 + g->FD + g->F2) * 4, 256);
  g->total = o;
  return 0;
}
// stats block: [mean1 F1][invstd1 F1][scale1 F1][shift1 F1][mean2 FD]...[mean3 F2]...
struct EegStats { float *mean1, *inv1, *sc1, *sh1, *mean2, *inv2, *sc2, *sh2, *mean3, *inv3, *sc3, *sh3; };
static EegStats eeg_stats(const EegGeom& g, void* saved) {
  float* p = (float*)((char*)saved + g.off_stats);
  EegStats s;
  s.mean1 = p; s.inv1 = p + g.F1; s.sc1 = p + 2 * g.F1; s.sh1 = p + 3 * g.F1; p += 4 * g.F1;
  s.mean2 = p; s.inv2 = p + g.FD; s.sc2 = p + 2 * g.FD; s.sh2 = p + 3 * g.FD; p += 4 * g.FD;
  s.mean3 = p; s.inv3 = p + g.F2; s.sc3 = p + 2 * g.F2; s.sh3 = p + 3 * g.F2;
  return s;
}
// ---- what the tuned backward holds: the expressions its launchers (bx_eeg_features_bwd, eeg.hip) check, in one place ----
// k_eeg_sep_bwd: row pitch of its LDS tiles, multiple of 4 with pitch/4 odd (the 16 fd rows a wave reads then fall on different bank groups)
__host__ __device__ inline int eeg_sepb_pitch(int T1) { int tp = ((T1 + 7) & ~7) + 24; if (((tp >> 2) & 1) == 0) tp += 4; return tp; }
// ... its two halves run in separate workgroups while that is what gives every CU two
static inline bool eeg_sepb_split(int B) { return B * 4 < 1024; }
static inline size_t eeg_sepb_lds(int B, int T1) {
  const size_t tile = (size_t)16 * eeg_sepb_pitch(T1);
  return (eeg_sepb_split(B) ? (tile + (tile > 4096 ? tile : 4096)) : (2 * tile + 4096)) * sizeof(float);
}
// k_eeg_conv1_bwd: four dc1 rows and the x row with 64-sample halos, plus the [256][16] combine buffer
static inline size_t eeg_conv1_bwd_lds(int T) { return ((size_t)5 * ((T + 2 * EEG_MAXK + 3) & ~3) + 4096) * sizeof(float); }
// Every backward goes through k_eeg_sep_bwd.  k_eeg_conv1_bwd is the fp32 path and what every other route falls back to: the matrix-core
// weight gradient (eeg_mfma.hip) is taken only while its own LDS fits and BX_EEG_NO_MFMA is unset, the collapsed forms only at
// kernLength 64 -- neither can be read off the descriptor, so its limits decide.  (bx_eegc_dx_launch's own limit is Chans <= EEG_MAXCH,
// which eeg_geom already enforces.)
static bool eeg_tuned_bwd_holds(const EegGeom& g) {
  return eeg_sepb_lds(g.B, g.T1) <= EEG_LDS_MAX && eeg_conv1_bwd_lds(g.T) <= EEG_LDS_MAX && g.T <= 256 * EEG_DX_MAX;
}
// The route is a function of the descriptor alone: bx_eeg_saved_bytes, bx_eeg_workspace, bx_eeg_saved_layout, the forward, the backward and
// the class-activation kernels all ask here and cannot disagree.  Tuned: the reference's default family AND rows that fit the forward's
// one-row LDS tile AND -- when a backward can follow (training mode, or bxEegDesc.grad) -- rows that the tuned backward holds.
// Everything else: the general kernels (eeg_generic.hip).
static bool eeg_tuned(const bxEegDesc* d, EegGeom* g) {
  if (eeg_geom(d, g) != 0 || d->T > EEG_MAXT) return false;
  return !(d->training || d->grad) || eeg_tuned_bwd_holds(*g);
}
