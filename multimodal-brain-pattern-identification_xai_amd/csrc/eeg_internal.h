// EEGNet kernels' shared host-side layout: the register-tiled family's geometry and the saved-for-backward arena that
// bx_eeg_features_fwd fills (eeg.hip) and later passes read (eeg.hip backward, eeg_cam.hip Grad-CAM).  Internal to the library.
#pragma once
#include "bx_common.h"

#define EEG_TT 256           // time steps per workgroup in the temporal conv
#define EEG_MAXK 64
#define EEG_MAXF 16          // F1*D and F2 upper bound
#define EEG_MAXCH 64
#define EEG_MAXT 15000       // longest row the tuned kernels' one-row LDS tile holds
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
// the tuned path needs the reference's default family AND rows that fit its one-row LDS tile; everything else: general kernels
static bool eeg_tuned(const bxEegDesc* d, EegGeom* g) { return eeg_geom(d, g) == 0 && d->T <= EEG_MAXT; }
