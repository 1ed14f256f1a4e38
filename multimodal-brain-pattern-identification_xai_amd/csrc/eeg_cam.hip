// Class-activation maps on the EEG branch (EEGNet blocks 1-2, reference models.py:271-285) in evaluation mode, from the arena that
// bx_eeg_features_fwd saved for the same input: the depthwise output dmap [B,16,T], the separable output smap [B,16,T1] and the
// three BatchNorms' scale s / shift h.  phi = dy_c/dfeat [F2,T2] per map (map m = sample * nm + class).  Per map:
//   Gs[o,t]  = s3[o] ELU'(s3[o] smap[o,t] + h3[o]) phi[o,t/P2] / P2          (t < T2*P2, else 0)
//   Gp1[q,t] = sum_o sum_j ws[o,q,j] Gs[o,t-j+7]                              (K2 = 16 'same': left pad 7)
//   Gd[q,t]  = s2[q] ELU'(s2[q] dmap[q,t] + h2[q]) Gp1[q,t/P1] / P1           (t < T1*P1, else 0)
// Grad-CAM (bx_eeg_gradcam) folds the gradient into its spatial sums:
//   separableConv: w[o] = mean_t Gs[o,t], map = sum_o w[o] smap[o]
//   depthwiseConv: w[q] = mean_t Gd[q,t], map = sum_q w[q] dmap[q]
//   conv1:         w[f] = s1[f]/(Chans T) sum_{q in f} (sum_ch wd[q,ch]) (sum_t Gd[q,t]); BatchNorm1 is affine in evaluation mode, so
//                  sum_f w[f] conv1_f(x) is ONE K1-tap filter kappa = sum_f w[f] k1[f] over the input: the [B,F1,Chans,T] conv1
//                  output is never formed.
//   Only sum_t Gd[q,t] is needed, and it folds the pooling: sum_t Gd[q,t] = sum_t1 Gp1[q,t1] (s2[q]/P1) sum_p ELU'(..dmap[q,P1 t1+p]..).
// Grad-CAM++ and Layer-CAM (bx_eeg_cam, methods BX_CAM_GRADCAM_PP / BX_CAM_LAYERCAM) form the gradient per element in the same
// kernels.  Tuned family: F1 = 8, D = 2, F1 D = F2 = 16.
#include <type_traits>
#include "eeg_internal.h"

#define CAM_TT 256           // pooled time steps per tile of k_eeg_cam_back (one per thread)
#define CAM_GP (CAM_TT + 16) // Gs tile row: index i <-> t = t0 - 8 + i (i < CAM_TT + 15 is read)
#define CAM1_TT 1024         // time steps per workgroup of the conv1 map kernels (4 per thread)
#define CAM_MAX_NM 64        // maps per sample (classes) one call serves

// 16 per-thread sums -> out[k] = scale * block total (fixed order: DPP wave sums, then the four waves in order).  256 threads.
__device__ __forceinline__ void cam_block_sum16(const float (&acc)[16], float* red, float* out, float scale) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) red[wave * 16 + k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int k = threadIdx.x;
    out[k] = ((red[k] + red[16 + k]) + (red[32 + k] + red[48 + k])) * scale;
  }
  __syncthreads();
}
// one element of a map: raw as it is, cam after the optional ReLU
__device__ __forceinline__ void cam_put(float* cam, float* raw, size_t i, float s, int relu) {
  if (raw) raw[i] = s;
  cam[i] = relu ? fmaxf(s, 0.f) : s;
}
// map m over a sample's 16 rows of length n: map[t] = sum_k w[k] rows[k][t]
__device__ __forceinline__ void cam_map16(const float* w, const float* rows, int n, size_t m, float* cam, float* raw, int relu) {
  for (int t = threadIdx.x; t < n; t += 256) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s = fmaf(w[k], rows[(size_t)k * n + t], s);
    cam_put(cam, raw, m * n + t, s, relu);
  }
}

// separableConv target: one workgroup per map.  With Gs[o,t] as above (0 for t >= T2 P2):
//   Grad-CAM:   w[o] = mean_t Gs[o,t] (the 1/P2 joins the mean);                  raw = sum_o w[o] smap[o]
//   Grad-CAM++: S[o] = sum_t smap[o,t];  w[o] = sum_t campp_term(Gs[o,t], S[o]);  raw = sum_o w[o] smap[o]
//   Layer-CAM:  raw[t] = sum_o max(Gs[o,t], 0) smap[o,t]                          (one pass)
template <int METHOD>
__global__ __launch_bounds__(256) void k_eeg_cam_sep(const float* __restrict__ smap, EegStats st, const float* __restrict__ dfeat,
                                                     float* __restrict__ cam, float* __restrict__ raw, float* __restrict__ wout, EegGeom g,
                                                     int nm, int relu) {
  __shared__ float red[64], sw[16], sS[16], ssc[16], ssh[16];
  const int m = blockIdx.x, b = m / nm, tid = threadIdx.x;
  if (tid < 16) { ssc[tid] = st.sc3[tid]; ssh[tid] = st.sh3[tid]; }
  __syncthreads();
  const int T1 = g.T1, T2 = g.T2, P2 = g.P2, TP = T2 * P2;
  const float* sb = smap + (size_t)b * 16 * T1;
  const float* phi = dfeat + (size_t)m * 16 * T2;
  const float inv_p2 = 1.f / (float)P2;
  auto dact = [&](int o, int t) {                                      // s3[o] ELU'(s3[o] smap[o,t] + h3[o])
    const float a = ssc[o], z = fmaf(a, sb[(size_t)o * T1 + t], ssh[o]);
    return z > 0.f ? a : a * expf(z);
  };
  auto gs = [&](int o, int t) { return dact(o, t) * phi[o * T2 + t / P2] * inv_p2; };      // Gs[o,t], t < TP
  if constexpr (METHOD == BX_CAM_LAYERCAM) {
    for (int t = tid; t < T1; t += 256) {
      float s = 0.f;
      if (t < TP) {
#pragma unroll
        for (int o = 0; o < 16; ++o) s = fmaf(fmaxf(gs(o, t), 0.f), sb[(size_t)o * T1 + t], s);
      }
      if (raw) raw[(size_t)m * T1 + t] = s;                             // (written out: through cam_put this loop takes 95 VGPRs for 62)
      cam[(size_t)m * T1 + t] = relu ? fmaxf(s, 0.f) : s;
    }
    return;
  }
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = 0.f;
  if constexpr (METHOD == BX_CAM_GRADCAM) {
    for (int t = tid; t < TP; t += 256)
#pragma unroll
      for (int o = 0; o < 16; ++o) acc[o] = fmaf(dact(o, t), phi[o * T2 + t / P2], acc[o]);
    cam_block_sum16(acc, red, sw, 1.f / ((float)P2 * (float)T1));
  } else {
    for (int t = tid; t < T1; t += 256)
#pragma unroll
      for (int o = 0; o < 16; ++o) acc[o] += sb[(size_t)o * T1 + t];
    cam_block_sum16(acc, red, sS, 1.f);
#pragma unroll
    for (int o = 0; o < 16; ++o) acc[o] = 0.f;
    for (int t = tid; t < TP; t += 256)
#pragma unroll
      for (int o = 0; o < 16; ++o) acc[o] += campp_term(gs(o, t), sS[o]);
    cam_block_sum16(acc, red, sw, 1.f);
  }
  if (wout && tid < 16) wout[(size_t)m * 16 + tid] = sw[tid];
  cam_map16(sw, sb, T1, m, cam, raw, relu);
}

// ---- the pieces of k_eeg_cam_back's tile walk ---------------------------------------------------------------------------------
// The Gs tile of pooled steps t0 .. t0 + CAM_TT - 1 with the 15-step halo of the 16-tap transposed convolution.  16 * CAM_GP =
// 17 * 256: all 17 of a thread's smap / phi loads are issued before the first use (clamped, then masked).  sc3 / sh3: s3, h3 in LDS.
__device__ __forceinline__ void cam_gs_tile(float* sG, const float* sb, const float* phi, const float* sc3, const float* sh3, int t0,
                                            int T1, int T2, int P2) {
  const int TP2 = T2 * P2;
  const float inv_p2 = 1.f / (float)P2;
  lds_fill<17>(sG, 16 * CAM_GP, [&](int i) {
    const int o = i / CAM_GP, k = i - o * CAM_GP, t = t0 - 8 + k;
    const bool ok = t >= 0 && t < TP2 && k < CAM_TT + 15;
    const int tc = ok ? t : 0;
    const float a = sc3[o], z = fmaf(a, sb[(size_t)o * T1 + tc], sh3[o]);
    const float v = (z > 0.f ? a : a * expf(z)) * phi[o * T2 + tc / P2] * inv_p2;
    return ok ? v : 0.f;
  });
}
// Gp1[0..15] of the thread's step from the tile (wave-uniform 16-byte weight reads: one Gs read + 4 weight reads per 16 FMAs)
__device__ __forceinline__ void cam_gp1(const float* sG, const float* sW, float (&gp)[16]) {
#pragma unroll
  for (int q = 0; q < 16; ++q) gp[q] = 0.f;
  for (int o = 0; o < 16; ++o) {
    const float* gr = sG + o * CAM_GP + threadIdx.x;                  // gr[15 - j] <-> Gs[o, t - j + 7]
    const float4* wr = reinterpret_cast<const float4*>(sW + o * 256);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float gv = gr[15 - j];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const float4 w4 = wr[j * 4 + qq];
        gp[4 * qq + 0] = fmaf(w4.x, gv, gp[4 * qq + 0]);
        gp[4 * qq + 1] = fmaf(w4.y, gv, gp[4 * qq + 1]);
        gp[4 * qq + 2] = fmaf(w4.z, gv, gp[4 * qq + 2]);
        gp[4 * qq + 3] = fmaf(w4.w, gv, gp[4 * qq + 3]);
      }
    }
  }
}
// Grad-CAM's pooled factor of step t: e2[q] = (s2[q] / P1) sum_p ELU'(s2[q] dmap[q, P1 t + p] + h2[q]); one 16-byte load per row
// when vec4 (P1 = 4 and 16-byte aligned rows)
__device__ __forceinline__ void cam_pool_dact(const float* db, const float* sc2, const float* sh2, int t, int T, int P1, bool vec4,
                                              float (&e2)[16]) {
  const float inv_p1 = 1.f / (float)P1;
  if (vec4) {
    float4 dv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) dv[q] = *reinterpret_cast<const float4*>(db + (size_t)q * T + (size_t)t * 4);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float a = sc2[q], h = sh2[q];
      const float d4[4] = {dv[q].x, dv[q].y, dv[q].z, dv[q].w};
      float e = 0.f;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float z = fmaf(a, d4[p], h);
        e += z > 0.f ? 1.f : expf(z);
      }
      e2[q] = e * a * inv_p1;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float a = sc2[q], h = sh2[q];
      const float* dr = db + (size_t)q * T + (size_t)t * P1;
      float e = 0.f;
      for (int p = 0; p < P1; ++p) {
        const float z = fmaf(a, dr[p], h);
        e += z > 0.f ? 1.f : expf(z);
      }
      e2[q] = e * a * inv_p1;
    }
  }
}
// the conv1 target's combined kernel kappa[j] = sum_f w[f] k1[f,j], zero beyond K1: the FIR of k_eeg_cam_conv1 runs K1p taps
__device__ __forceinline__ void cam_kappa(const float* w, const float* w1, int K1, int K1p, float* kappa) {      // 8 = F1: eeg_tuned() admits no other
  for (int j = threadIdx.x; j < K1p; j += 256) {
    float k = 0.f;
    if (j < K1)
      for (int f = 0; f < 8; ++f) k = fmaf(w[f], w1[(size_t)f * K1 + j], k);
    kappa[j] = k;
  }
}

// depthwiseConv (TGT 1) and conv1 (TGT 0) targets: one workgroup per map.  The pooled axis is walked in tiles of CAM_TT steps: the
// tile's Gs is formed in LDS, a thread forms Gp1[0..15] of its step t, and then
//   Grad-CAM    folds it with the pooled ELU' of dmap (requested before the FMA loop) into its running sum_t Gd.  Depthwise target: a
//               second pass writes the map; conv1 target: w[f] and the combined kernel kappa to the workspace.
//   otherwise   Gd per element over the step's P1 positions, Gd[q, P1 t + p] = s2[q] ELU'(s2[q] dmap[q, P1 t + p] + h2[q]) Gp1[q,t] / P1
//               (0 for positions >= T1 P1):
//     depthwise, Layer-CAM:  raw[t] = sum_q max(Gd[q,t], 0) dmap[q,t], written as the tiles are walked
//     depthwise, Grad-CAM++: S[q] = sum_t dmap[q,t] first; w[q] = sum_t campp_term(Gd[q,t], S[q]); then the map sum_q w[q] dmap[q]
//     conv1,     Grad-CAM++: G1[f,ch,t] = s1[f] (wd[2f,ch] Gd[2f,t] + wd[2f+1,ch] Gd[2f+1,t]) for every electrode, from the registers;
//                            S[f] = sum_{ch,t} conv1_f(x)[ch,t] = sum_j k1[f,j] X[j], X[j] the sum of x over the window that tap j
//                            sees ('same' padding); w[f] = sum_{ch,t} campp_term(G1, S[f]) -> kappa, then k_eeg_cam_conv1 as for Grad-CAM
//     conv1,     Layer-CAM:  Gd [16][Tp] of the map to the workspace (zero-padded to Tp), for k_eeg_cam_conv1_lc
// work: the conv1 target's workspace, kappa [B*nm][K1p] or Layer-CAM's Gd [B*nm][16][Tp].
template <int TGT, int METHOD>
__global__ __launch_bounds__(256) void k_eeg_cam_back(const float* __restrict__ dmap, const float* __restrict__ smap, EegStats st,
                                                      const float* __restrict__ dfeat, const float* __restrict__ ws, const float* __restrict__ wd,
                                                      const float* __restrict__ w1, const float* __restrict__ x, float* __restrict__ cam,
                                                      float* __restrict__ raw, float* __restrict__ wout, float* __restrict__ work, int K1p, int Tp,
                                                      EegGeom g, int nm, int relu) {
  __shared__ __attribute__((aligned(16))) float sW[16 * 16 * 16];   // [o][j][q] <- separableConv.weight [o][q][1][j]
  __shared__ float sG[16 * CAM_GP];
  __shared__ float red[64], sS[16], sc[4][16], swf[16], sX[EEG_MAXK];  // sc: s3, h3, s2, h2
  __shared__ float sWd[TGT == 0 && METHOD == BX_CAM_GRADCAM_PP ? 16 * EEG_MAXCH : 1];
  const int m = blockIdx.x, b = m / nm, tid = threadIdx.x;
  lds_fill<16>(sW, 4096, [&](int i) { const int q = i & 15, j = (i >> 4) & 15, o = i >> 8; return ws[(o * 16 + q) * 16 + j]; });
  if (tid < 16) { sc[0][tid] = st.sc3[tid]; sc[1][tid] = st.sh3[tid]; sc[2][tid] = st.sc2[tid]; sc[3][tid] = st.sh2[tid]; }
  const int T = g.T, T1 = g.T1, T2 = g.T2, P1 = g.P1, P2 = g.P2, Ch = g.Ch;
  const float* sb = smap + (size_t)b * 16 * T1;
  const float* db = dmap + (size_t)b * 16 * T;
  const float* phi = dfeat + (size_t)m * 16 * T2;
  const float inv_p1 = 1.f / (float)P1;
  const bool vec4 = P1 == 4 && T % 4 == 0;                             // dmap rows 16-byte aligned (the arena region is)
  float acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  if constexpr (METHOD == BX_CAM_GRADCAM_PP && TGT == 1) {
    for (int t = tid; t < T; t += 256)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] += db[(size_t)q * T + t];
    cam_block_sum16(acc, red, sS, 1.f);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  } else if constexpr (METHOD == BX_CAM_GRADCAM_PP && TGT == 0) {
    const float* xb = x + (size_t)b * Ch * T;
    for (int i = tid; i < 16 * Ch; i += 256) sWd[i] = wd[i];
    float tot = 0.f;
    for (int i = tid; i < Ch * T; i += 256) tot += xb[i];
    tot = wave_sum(tot);
    if ((tid & 63) == 0) red[tid >> 6] = tot;
    __syncthreads();
    tot = (red[0] + red[1]) + (red[2] + red[3]);
    if (tid < g.K1) {                                                  // tap j reads x[u], u = t + j - padl1: drop what lies outside
      const int d = tid - g.padl1;
      const int lo = d > 0 ? 0 : T + d, hi = d > 0 ? d : T;           // the excluded columns [lo, hi)
      float ex = 0.f;
      for (int ch = 0; ch < Ch; ++ch)
        for (int u = lo; u < hi; ++u) ex += xb[(size_t)ch * T + u];
      sX[tid] = tot - ex;
    }
    __syncthreads();
    if (tid < 8) {
      float s = 0.f;
      for (int j = 0; j < g.K1; ++j) s = fmaf(w1[(size_t)tid * g.K1 + j], sX[j], s);
      sS[tid] = s;
      swf[tid] = st.sc1[tid];
    }
  }
  for (int t0 = 0; t0 < T1; t0 += CAM_TT) {
    __syncthreads();                // first trip: sW / sc staged; later trips: the previous tile's readers are done
    cam_gs_tile(sG, sb, phi, sc[0], sc[1], t0, T1, T2, P2);
    const int t = t0 + tid;
    float e2[16];
    if constexpr (METHOD == BX_CAM_GRADCAM) {
      if (t < T1) cam_pool_dact(db, sc[2], sc[3], t, T, P1, vec4, e2);
    }
    __syncthreads();
    if (t < T1) {
      float gp[16];
      cam_gp1(sG, sW, gp);
      if constexpr (METHOD == BX_CAM_GRADCAM) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = fmaf(gp[q], e2[q], acc[q]);
      } else {
        for (int p = 0; p < P1; ++p) {
          const int tt = t * P1 + p;
          float dv[16], gdv[16];
#pragma unroll
          for (int q = 0; q < 16; ++q) dv[q] = db[(size_t)q * T + tt];
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float a = sc[2][q], z = fmaf(a, dv[q], sc[3][q]);
            gdv[q] = (z > 0.f ? a : a * expf(z)) * gp[q] * inv_p1;
          }
          if constexpr (TGT == 1 && METHOD == BX_CAM_LAYERCAM) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) s = fmaf(fmaxf(gdv[q], 0.f), dv[q], s);
            cam_put(cam, raw, (size_t)m * T + tt, s, relu);
          } else if constexpr (TGT == 1) {
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] += campp_term(gdv[q], sS[q]);
          } else if constexpr (METHOD == BX_CAM_LAYERCAM) {
#pragma unroll
            for (int q = 0; q < 16; ++q) work[((size_t)m * 16 + q) * Tp + tt] = gdv[q];
          } else {
            for (int ch = 0; ch < Ch; ++ch)
#pragma unroll
              for (int f = 0; f < 8; ++f) {
                const float g1 = swf[f] * fmaf(sWd[(2 * f) * Ch + ch], gdv[2 * f], sWd[(2 * f + 1) * Ch + ch] * gdv[2 * f + 1]);
                acc[f] += campp_term(g1, sS[f]);
              }
          }
        }
      }
    }
  }
  if constexpr (METHOD == BX_CAM_LAYERCAM) {                           // positions T1 P1 <= t < T: no gradient
    for (int tt = T1 * P1 + tid; tt < (TGT == 1 ? T : Tp); tt += 256) {
      if constexpr (TGT == 1) {
        cam_put(cam, raw, (size_t)m * T + tt, 0.f, 0);
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) work[((size_t)m * 16 + q) * Tp + tt] = 0.f;
      }
    }
    return;
  }
  __syncthreads();
  // the target's weights into swf: 16 of the depthwise channels, 8 of the conv1 filters
  if constexpr (METHOD == BX_CAM_GRADCAM) {
    cam_block_sum16(acc, red, sS, 1.f);                                 // sS[q] = sum_t Gd[q,t]
    if (TGT == 1) {
      if (tid < 16) swf[tid] = sS[tid] / (float)T;
    } else if (tid < 8) {                                               // 8 = F1 (eeg_tuned() admits no other), as in the other methods
      const int f = tid, D = g.D;
      float s = 0.f;
      for (int d = 0; d < D; ++d) {
        const int q = f * D + d;
        float c = 0.f;
        for (int ch = 0; ch < Ch; ++ch) c += wd[(size_t)q * Ch + ch];
        s = fmaf(c, sS[q], s);
      }
      swf[f] = st.sc1[f] * s / ((float)Ch * (float)T);
    }
    __syncthreads();
  } else {
    cam_block_sum16(acc, red, swf, 1.f);                                // Grad-CAM++: the block totals are the weights
  }
  constexpr int NW = TGT == 1 ? 16 : 8;
  if (wout && tid < NW) wout[(size_t)m * NW + tid] = swf[tid];
  if constexpr (TGT == 1) cam_map16(swf, db, T, m, cam, raw, relu);
  else cam_kappa(swf, w1, g.K1, K1p, work + (size_t)m * K1p);
}

// conv1 map: raw[m,ch,t] = sum_j kappa[m,j] x[b,ch,t+j-padl1] for the nm maps of sample b.  grid (T / CAM1_TT, Chans, B): the
// x row tile plus its K1p+4 halo is read into LDS once and serves every map; a thread produces 4 consecutive steps with a sliding
// window (one 16-byte LDS read and one wave-uniform 16-byte kappa read per 16 FMAs) and writes them with one 16-byte store.
__global__ __launch_bounds__(256) void k_eeg_cam_conv1(const float* __restrict__ x, const float* __restrict__ kappa, float* __restrict__ cam,
                                                       float* __restrict__ raw, int Ch, int T, int K1p, int padl, int nm, int relu, int vec) {
  extern __shared__ __attribute__((aligned(16))) float sx[];          // [CAM1_TT + K1p + 4]: sx[k] <-> x[t0 - padl + k] (0 outside [0, T))
  const int t0 = blockIdx.x * CAM1_TT, ch = blockIdx.y, b = blockIdx.z;
  const float* xr = x + ((size_t)b * Ch + ch) * T;
  lds_fill<5>(sx, CAM1_TT + K1p + 4, [&](int k) { const int t = t0 - padl + k; return (t >= 0 && t < T) ? xr[t] : 0.f; });
  __syncthreads();
  const int tl = 4 * threadIdx.x, tt = t0 + tl;
  if (tt >= T) return;
  for (int mm = 0; mm < nm; ++mm) {
    const size_t m = (size_t)b * nm + mm;
    const float* kp = kappa + m * K1p;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float4 cur = *reinterpret_cast<const float4*>(sx + tl);
    for (int j0 = 0; j0 < K1p; j0 += 4) {
      const float4 nxt = *reinterpret_cast<const float4*>(sx + tl + j0 + 4);
      const float4 k4 = *reinterpret_cast<const float4*>(kp + j0);
      const float win[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
      const float kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(kk[u], win[u + i], acc[i]);
      cur = nxt;
    }
    const size_t o = (m * Ch + ch) * T + tt;
    if (vec && tt + 3 < T) {
      if (raw) *reinterpret_cast<float4*>(raw + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      if (relu) for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.f);
      *reinterpret_cast<float4*>(cam + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      for (int i = 0; i < 4 && tt + i < T; ++i) {
        if (raw) raw[o + i] = acc[i];
        cam[o + i] = relu ? fmaxf(acc[i], 0.f) : acc[i];
      }
    }
  }
}

// conv1 target, Layer-CAM: raw[m,ch,t] = sum_f max(G1[f,ch,t], 0) A1[f,ch,t] with A1 = conv1_f(x) ('same', no bias) and
// G1[f,ch,t] = s1[f] (wd[2f,ch] Gd[m,2f,t] + wd[2f+1,ch] Gd[m,2f+1,t]) (Gd from the workspace).  grid (T / CAM1_TT, Chans, B) as
// k_eeg_cam_conv1: the x row tile with its halo and the 8 filters in LDS; a thread forms A1 of its 4 steps for the 8 filters once
// (sliding window, 8 x K1p x 4 FMAs) and serves every map of the sample from those registers.
__global__ __launch_bounds__(256) void k_eeg_cam_conv1_lc(const float* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ wd,
                                                          EegStats st, const float* __restrict__ gd, float* __restrict__ cam,
                                                          float* __restrict__ raw, int Ch, int T, int K1, int K1p, int padl, int Tp, int nm,
                                                          int relu, int vec) {
  extern __shared__ __attribute__((aligned(16))) float sx[];          // [CAM1_TT + K1p + 4] x tile | [8][K1p] conv1 taps (zero beyond K1)
  __shared__ float sg[16];                                             // s1[f] wd[q,ch] of this electrode, q = 2f + d
  float* sk = sx + CAM1_TT + K1p + 4;
  const int t0 = blockIdx.x * CAM1_TT, ch = blockIdx.y, b = blockIdx.z;
  const float* xr = x + ((size_t)b * Ch + ch) * T;
  lds_fill<5>(sx, CAM1_TT + K1p + 4, [&](int k) { const int t = t0 - padl + k; return (t >= 0 && t < T) ? xr[t] : 0.f; });
  lds_fill<2>(sk, 8 * K1p, [&](int i) { const int f = i / K1p, j = i - f * K1p; return j < K1 ? w1[(size_t)f * K1 + (j < K1 ? j : 0)] : 0.f; });
  if (threadIdx.x < 16) sg[threadIdx.x] = st.sc1[threadIdx.x >> 1] * wd[(size_t)threadIdx.x * Ch + ch];
  __syncthreads();
  const int tl = 4 * threadIdx.x, tt = t0 + tl;
  if (tt >= T) return;
  float a1[8][4];
#pragma unroll
  for (int f = 0; f < 8; ++f)
#pragma unroll
    for (int i = 0; i < 4; ++i) a1[f][i] = 0.f;
  float4 cur = *reinterpret_cast<const float4*>(sx + tl);
  for (int j0 = 0; j0 < K1p; j0 += 4) {
    const float4 nxt = *reinterpret_cast<const float4*>(sx + tl + j0 + 4);
    const float win[8] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z, nxt.w};
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      const float4 k4 = *reinterpret_cast<const float4*>(sk + f * K1p + j0);
      const float kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) a1[f][i] = fmaf(kk[u], win[u + i], a1[f][i]);
    }
    cur = nxt;
  }
  for (int mm = 0; mm < nm; ++mm) {
    const size_t m = (size_t)b * nm + mm;
    const float* gr = gd + m * 16 * Tp + tt;                            // Tp % 4 == 0 and tt % 4 == 0: 16-byte loads inside the row
    float4 g4[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) g4[q] = *reinterpret_cast<const float4*>(gr + (size_t)q * Tp);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      const float e[4] = {g4[2 * f].x, g4[2 * f].y, g4[2 * f].z, g4[2 * f].w}, o[4] = {g4[2 * f + 1].x, g4[2 * f + 1].y, g4[2 * f + 1].z, g4[2 * f + 1].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(fmaxf(fmaf(sg[2 * f], e[i], sg[2 * f + 1] * o[i]), 0.f), a1[f][i], acc[i]);
    }
    const size_t oi = (m * Ch + ch) * T + tt;
    if (vec && tt + 3 < T) {
      if (raw) *reinterpret_cast<float4*>(raw + oi) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      if (relu) for (int i = 0; i < 4; ++i) acc[i] = fmaxf(acc[i], 0.f);
      *reinterpret_cast<float4*>(cam + oi) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      for (int i = 0; i < 4 && tt + i < T; ++i) {
        if (raw) raw[oi + i] = acc[i];
        cam[oi + i] = relu ? fmaxf(acc[i], 0.f) : acc[i];
      }
    }
  }
}

static int cam_k1p(const EegGeom& g) { return (g.K1 + 3) / 4 * 4; }

// Grad-CAM and Grad-CAM++: the combined kernels kappa [B*nm][K1p] of the conv1 target; Layer-CAM: the conv1 target's Gd [B*nm][16][Tp]
static int cam_tp(const EegGeom& g) { return (g.T + 3) / 4 * 4; }
static size_t eeg_cam_ws(const bxEegDesc* d, int maps_per_act, int target, int method) {
  EegGeom g;
  if (!d || !eeg_tuned(d, &g) || maps_per_act < 1 || maps_per_act > CAM_MAX_NM || target < BX_EEG_CAM_CONV1 || target > BX_EEG_CAM_SEPARABLE)
    return 0;
  const size_t per_map = method == BX_CAM_LAYERCAM ? (size_t)16 * cam_tp(g) : (size_t)cam_k1p(g);
  return bx_align_up((size_t)g.B * maps_per_act * per_map * sizeof(float), 256);
}
extern "C" size_t bx_eeg_gradcam_workspace(const bxEegDesc* d, int maps_per_act, int target) {
  return eeg_cam_ws(d, maps_per_act, target, BX_CAM_GRADCAM);
}
extern "C" size_t bx_eeg_cam_workspace(const bxEegDesc* d, int maps_per_act, int target, int method) {
  if (method < BX_CAM_GRADCAM || method > BX_CAM_LAYERCAM) {
    bx_set_error("bx_eeg_cam_workspace: unknown method %d (0 = Grad-CAM, 1 = Grad-CAM++, 2 = Layer-CAM)", method);
    return 0;
  }
  return eeg_cam_ws(d, maps_per_act, target, method);
}

extern "C" int bx_eeg_saved_layout(const bxEegDesc* d, size_t* off_dmap, size_t* off_smap) {
  BX_REQUIRE(d && off_dmap && off_smap, "bx_eeg_saved_layout: null pointer");
  EegGeom g;
  if (!eeg_tuned(d, &g)) BX_FAIL(BX_EUNSUPPORTED, "bx_eeg_saved_layout: EEG geometry outside the tuned family");
  *off_dmap = g.off_d;
  *off_smap = g.off_s;
  return BX_OK;
}

static int eeg_cam(const char* who, const bxEegDesc* d, const bxEegParams* p, const float* x, const void* saved, const float* dfeat,
                   int maps_per_act, int target, int method, int relu, float* cam, float* raw, float* weights, void* workspace,
                   size_t workspace_bytes, hipStream_t s) {
  BX_REQUIRE(method >= BX_CAM_GRADCAM && method <= BX_CAM_LAYERCAM, "%s: unknown method %d (0 = Grad-CAM, 1 = Grad-CAM++, 2 = Layer-CAM)", who, method);
  BX_REQUIRE(method != BX_CAM_LAYERCAM || !weights, "%s: Layer-CAM has no channel weights (weights must be NULL)", who);
  BX_REQUIRE(d, "%s: null descriptor", who);
  EegGeom g;
  if (!eeg_tuned(d, &g))
    BX_FAIL(BX_EUNSUPPORTED, "%s: EEG geometry outside the tuned family (needs F1=8, D=2, F2=16, K2=16, kernLength <= %d, "
            "Chans <= %d, T <= %d)", who, EEG_MAXK, EEG_MAXCH, EEG_MAXT);
  BX_REQUIRE(p && p->sep_w && p->dw_w && p->conv1_w && saved && dfeat && cam, "%s: null pointer", who);
  BX_REQUIRE(target >= BX_EEG_CAM_CONV1 && target <= BX_EEG_CAM_SEPARABLE, "%s: unknown target %d", who, target);
  BX_REQUIRE(!d->training, "%s: needs the arena of an evaluation-mode forward (training = 0)", who);
  BX_REQUIRE(maps_per_act >= 1 && maps_per_act <= CAM_MAX_NM, "%s: maps_per_act %d outside [1, %d]", who, maps_per_act, CAM_MAX_NM);
  BX_REQUIRE(g.B <= 65535 && (long long)g.B * maps_per_act <= (1ll << 30), "%s: batch %d too large", who, g.B);
  const EegStats st = eeg_stats(g, const_cast<void*>(saved));
  const float* dmap = (const float*)((const char*)saved + g.off_d);
  const float* smap = (const float*)((const char*)saved + g.off_s);
  const int n_maps = g.B * maps_per_act, rl = relu ? 1 : 0, K1p = cam_k1p(g), Tp = cam_tp(g);
  const bool lc = method == BX_CAM_LAYERCAM;
  if (target == BX_EEG_CAM_SEPARABLE) {
    BX_DISPATCH_CAM(method, M, hipLaunchKernelGGL(k_eeg_cam_sep<M>, dim3(n_maps), dim3(256), 0, s, smap, st, dfeat, cam, raw, weights, g, maps_per_act, rl));
    BX_CHECK_LAUNCH("bx_eeg_gradcam (separableConv)");
    return BX_OK;
  }
  // k_eeg_cam_back<TGT, method>.  The depthwise target reads neither x, work, K1p nor Tp; Layer-CAM's weights are NULL (checked above)
  auto back = [&](auto tgt, float* work) {
    BX_DISPATCH_CAM(method, M, hipLaunchKernelGGL((k_eeg_cam_back<decltype(tgt)::value, M>), dim3(n_maps), dim3(256), 0, s, dmap, smap, st, dfeat,
                                                  p->sep_w, p->dw_w, p->conv1_w, x, cam, raw, weights, work, K1p, Tp, g, maps_per_act, rl));
  };
  if (target == BX_EEG_CAM_DEPTHWISE) {
    back(std::integral_constant<int, 1>(), nullptr);
    BX_CHECK_LAUNCH("bx_eeg_gradcam (depthwiseConv)");
    return BX_OK;
  }
  BX_REQUIRE(x, "%s: the conv1 target reads the input x", who);
  const size_t need = eeg_cam_ws(d, maps_per_act, target, method);
  if (!workspace || workspace_bytes < need) BX_FAIL(BX_EWORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
  float* work = (float*)workspace;                                     // kappa, or Layer-CAM's Gd
  back(std::integral_constant<int, 0>(), work);
  BX_CHECK_LAUNCH(lc ? "bx_eeg_cam (conv1 gradient)" : "bx_eeg_gradcam (conv1 weights)");
  const dim3 grid(bx_ceil_div(g.T, CAM1_TT), g.Ch, g.B);
  const int vec = g.T % 4 == 0 && ((uintptr_t)cam & 15) == 0 && ((uintptr_t)raw & 15) == 0;
  if (lc)
    hipLaunchKernelGGL(k_eeg_cam_conv1_lc, grid, dim3(256), (size_t)(CAM1_TT + 9 * K1p + 4) * sizeof(float), s, x, p->conv1_w, p->dw_w, st, work,
                       cam, raw, g.Ch, g.T, g.K1, K1p, g.padl1, Tp, maps_per_act, rl, vec);
  else
    hipLaunchKernelGGL(k_eeg_cam_conv1, grid, dim3(256), (size_t)(CAM1_TT + K1p + 4) * sizeof(float), s, x, work, cam, raw, g.Ch, g.T, K1p, g.padl1,
                       maps_per_act, rl, vec);
  BX_CHECK_LAUNCH(lc ? "bx_eeg_cam (conv1 Layer-CAM map)" : "bx_eeg_gradcam (conv1 map)");
  return BX_OK;
}

extern "C" int bx_eeg_gradcam(const bxEegDesc* d, const bxEegParams* p, const float* x, const void* saved, const float* dfeat, int maps_per_act,
                              int target, int relu, float* cam, float* raw, float* weights, void* workspace, size_t workspace_bytes,
                              bxStream stream) {
  return eeg_cam("bx_eeg_gradcam", d, p, x, saved, dfeat, maps_per_act, target, BX_CAM_GRADCAM, relu, cam, raw, weights, workspace,
                 workspace_bytes, (hipStream_t)stream);
}
extern "C" int bx_eeg_cam(const bxEegDesc* d, const bxEegParams* p, const float* x, const void* saved, const float* dfeat, int maps_per_act,
                          int target, int method, int relu, float* cam, float* raw, float* weights, void* workspace, size_t workspace_bytes,
                          bxStream stream) {
  return eeg_cam(method == BX_CAM_GRADCAM ? "bx_eeg_gradcam" : "bx_eeg_cam", d, p, x, saved, dfeat, maps_per_act, target, method, relu, cam, raw,
                 weights, workspace, workspace_bytes, (hipStream_t)stream);
}
