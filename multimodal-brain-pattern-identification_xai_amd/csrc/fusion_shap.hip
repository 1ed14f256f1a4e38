// Fusion SHAP: exact Shapley values of the votes the two branches hand to the fusion head (include/brainxai.h, "Fusion SHAP").
//   cat -> Linear(2K,Hd) -> ReLU -> Linear(Hd,K) -> LogSoftmax     the head of heads.hip: k_fusion_fwd, evaluated B * Nb * NS times
// The first layer is affine in the composed row, so a workgroup keeps, per (sample, background row) pair and tile of hidden units, one
// table per group of at most 8 votes with the group's partial sum for every setting of its bits; a coalition then costs one LDS read
// per group, the adds, the ReLU and the second layer's K multiply-adds per hidden unit.  A thread owns whole coalitions: their K
// logits and the K fp64 running sums over the background rows live in its registers, so nothing crosses threads and no bit of a
// value depends on the grid, on the list or on how it is cut into launches.
#include "bx_common.h"

#define FS_THREADS 256
#define FS_LDS_FLOATS 16384                       // 64 KB: tables | second-layer tile | the two vote rows
#define FS_MAX_GROUPS 4

// the 2K votes in groups of at most 8 bits of the mask (one per half for K <= 8, two above), and the tile of hidden units
struct FsGeom {
  int K, Hd, EPH, HT, ntiles;                     // EPH: table entries per hidden unit = sum_g 2^bits[g]
  int bits[FS_MAX_GROUPS], shift[FS_MAX_GROUPS], off[FS_MAX_GROUPS];
};

// KM >= K: the static bound of the class loops; NG groups; MPT coalitions per thread
template <int KM, int NG, int MPT>
__global__ __launch_bounds__(FS_THREADS) void k_fusion_values(const float* __restrict__ e_x, const float* __restrict__ s_x,
    const float* __restrict__ e_bg, const float* __restrict__ s_bg, const uint32_t* __restrict__ masks, const float* __restrict__ w1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, double* __restrict__ v, FsGeom g, int Nb,
    int NS, int score_kind) {
  extern __shared__ float sm[];                   // tab[HT][EPH] | w2s[HT][KM] | zx[2K] | zb[2K]
  const int K = g.K, Hd = g.Hd, EPH = g.EPH, tid = threadIdx.x, b = blockIdx.y;
  float* tab = sm;
  float* w2s = tab + (size_t)g.HT * EPH;
  float* zx = w2s + (size_t)g.HT * KM;
  float* zb = zx + 2 * K;
  const uint32_t all = 2 * K >= 32 ? 0xffffffffu : (1u << (2 * K)) - 1u;

  int off[MPT][NG], sidx[MPT];
  double acc[MPT][KM];
#pragma unroll
  for (int q = 0; q < MPT; ++q) {
    sidx[q] = ((int)blockIdx.x * MPT + q) * FS_THREADS + tid;
    const uint32_t mask = masks[sidx[q] < NS ? sidx[q] : 0] & all;       // a thread past the list walks entry 0 and stores nothing
#pragma unroll
    for (int u = 0; u < NG; ++u) off[q][u] = g.off[u] + (int)((mask >> g.shift[u]) & ((1u << g.bits[u]) - 1u));
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[q][k] = 0.0;
  }
  if (tid < 2 * K) zx[tid] = tid < K ? e_x[(size_t)b * K + tid] : s_x[(size_t)b * K + tid - K];

  for (int j = 0; j < Nb; ++j) {
    __syncthreads();                              // the last tile of row j - 1 has been read
    if (tid < 2 * K) zb[tid] = tid < K ? e_bg[(size_t)j * K + tid] : s_bg[(size_t)j * K + tid - K];
    float lg[MPT][KM];
#pragma unroll
    for (int q = 0; q < MPT; ++q)
#pragma unroll
      for (int k = 0; k < KM; ++k) lg[q][k] = k < K ? b2[k] : 0.f;

    for (int t = 0; t < g.ntiles; ++t) {
      const int h0 = t * g.HT, ht = Hd - h0 < g.HT ? Hd - h0 : g.HT;
      __syncthreads();                            // zb is written, the previous tile has been read
      // tables: entry (hidden unit, group, m) = the group's votes through w1 as one fmaf chain in ascending vote order, the first
      // group's starting from b1 and the others' from 0; bit set = the sample's vote, clear = the background row's
      for (int idx = tid; idx < ht * EPH; idx += FS_THREADS) {
        const int hl = idx / EPH, r = idx - hl * EPH;
        int gb = g.bits[0], gs = g.shift[0], go = 0;
        bool first = true;
#pragma unroll
        for (int u = 1; u < NG; ++u)
          if (r >= g.off[u]) { gb = g.bits[u]; gs = g.shift[u]; go = g.off[u]; first = false; }
        const int m = r - go;
        const float* wr = w1 + (size_t)(h0 + hl) * 2 * K;
        float wv[8];
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) wv[bit] = wr[gs + (bit < gb ? bit : gb - 1)];     // clamped, unconditional loads
        float a = first ? b1[h0 + hl] : 0.f;
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
          const int i = gs + (bit < gb ? bit : gb - 1);
          const float z = (m >> bit) & 1 ? zx[i] : zb[i];
          if (bit < gb) a = fmaf(wv[bit], z, a);
        }
        tab[idx] = a;
      }
      for (int idx = tid; idx < ht * KM; idx += FS_THREADS) {
        const int hl = idx / KM, k = idx - hl * KM;
        w2s[idx] = k < K ? w2[(size_t)k * Hd + h0 + hl] : 0.f;      // a zero weight leaves the unused logits alone
      }
      __syncthreads();
      for (int hl = 0; hl < ht; ++hl) {
        const float* row = tab + (size_t)hl * EPH;
        float wk[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) wk[k] = w2s[hl * KM + k];
#pragma unroll
        for (int q = 0; q < MPT; ++q) {
          float pre = row[off[q][0]];
#pragma unroll
          for (int u = 1; u < NG; ++u) pre += row[off[q][u]];
          const float hv = fmaxf(pre, 0.f);
#pragma unroll
          for (int k = 0; k < KM; ++k) lg[q][k] = fmaf(wk[k], hv, lg[q][k]);
        }
      }
    }
    // the clean head's log-softmax; a probability is bx_softmax_rows of the log-probabilities, as the other drivers score
#pragma unroll
    for (int q = 0; q < MPT; ++q) {
      float m = -INFINITY, se = 0.f;
#pragma unroll
      for (int k = 0; k < KM; ++k) if (k < K) m = fmaxf(m, lg[q][k]);
#pragma unroll
      for (int k = 0; k < KM; ++k) if (k < K) se += expf(lg[q][k] - m);
      const float lse = m + logf(se);
      float lp[KM];
#pragma unroll
      for (int k = 0; k < KM; ++k) lp[k] = lg[q][k] - lse;
      if (score_kind == BX_FUSION_SCORE_LOGPROB) {
#pragma unroll
        for (int k = 0; k < KM; ++k) if (k < K) acc[q][k] += (double)lp[k];
      } else {
        float m2 = -INFINITY, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) if (k < K) m2 = fmaxf(m2, lp[k]);
#pragma unroll
        for (int k = 0; k < KM; ++k) if (k < K) s2 += expf(lp[k] - m2);
#pragma unroll
        for (int k = 0; k < KM; ++k) if (k < K) acc[q][k] += (double)(expf(lp[k] - m2) / s2);
      }
    }
  }
  const double nb = (double)Nb;
#pragma unroll
  for (int q = 0; q < MPT; ++q)
    if (sidx[q] < NS) {
      double* out = v + ((size_t)b * NS + sidx[q]) * K;
#pragma unroll
      for (int k = 0; k < KM; ++k) if (k < K) out[k] = acc[q][k] / nb;
    }
}

static FsGeom fs_geometry(int K, int Hd, int KM) {
  FsGeom g;
  g.K = K; g.Hd = Hd;
  int n = 0, at = 0;
  for (int half = 0; half < 2; ++half)
    for (int lo = 0; lo < K; lo += 8) {
      g.bits[n] = K - lo < 8 ? K - lo : 8;
      g.shift[n] = half * K + lo;
      g.off[n] = at;
      at += 1 << g.bits[n];
      ++n;
    }
  for (; n < FS_MAX_GROUPS; ++n) { g.bits[n] = 1; g.shift[n] = 0; g.off[n] = at; }     // never reached: r < EPH = off of the first unused group
  g.EPH = at;
  const int ht_max = (FS_LDS_FLOATS - 4 * K) / (g.EPH + KM);
  g.ntiles = bx_ceil_div(Hd, ht_max < Hd ? ht_max : Hd);
  g.HT = bx_ceil_div(Hd, g.ntiles);
  return g;
}

template <int KM, int NG, int MPT>
static void fs_launch(const float* e_x, const float* s_x, const float* e_bg, const float* s_bg, const uint32_t* masks, const float* w1,
                      const float* b1, const float* w2, const float* b2, double* v, int B, int Nb, int NS, int K, int Hd, int score_kind,
                      hipStream_t s) {
  const FsGeom g = fs_geometry(K, Hd, KM);
  const size_t lds = ((size_t)g.HT * (g.EPH + KM) + 4 * K) * sizeof(float);
  hipLaunchKernelGGL((k_fusion_values<KM, NG, MPT>), dim3(bx_ceil_div(NS, FS_THREADS * MPT), B), dim3(FS_THREADS), lds, s, e_x, s_x, e_bg, s_bg,
                     masks, w1, b1, w2, b2, v, g, Nb, NS, score_kind);
}

// coalitions per thread: the most (4, 2, 1) that still gives every CU a workgroup; the values do not depend on it
template <int KM, int NG>
static void fs_dispatch_mpt(const float* e_x, const float* s_x, const float* e_bg, const float* s_bg, const uint32_t* masks, const float* w1,
                            const float* b1, const float* w2, const float* b2, double* v, int B, int Nb, int NS, int K, int Hd, int score_kind,
                            hipStream_t s) {
  const long long want = 256;
  if (KM <= 8 && (long long)B * bx_ceil_div(NS, FS_THREADS * 4) >= want)
    fs_launch<KM, NG, (KM <= 8 ? 4 : 1)>(e_x, s_x, e_bg, s_bg, masks, w1, b1, w2, b2, v, B, Nb, NS, K, Hd, score_kind, s);
  else if ((long long)B * bx_ceil_div(NS, FS_THREADS * 2) >= want)
    fs_launch<KM, NG, 2>(e_x, s_x, e_bg, s_bg, masks, w1, b1, w2, b2, v, B, Nb, NS, K, Hd, score_kind, s);
  else
    fs_launch<KM, NG, 1>(e_x, s_x, e_bg, s_bg, masks, w1, b1, w2, b2, v, B, Nb, NS, K, Hd, score_kind, s);
}

extern "C" int bx_fusion_values(const float* e_x, const float* s_x, const float* e_bg, const float* s_bg, const uint32_t* masks,
                                const float* w1, const float* b1, const float* w2, const float* b2, int score_kind, double* v, int B, int Nb,
                                int NS, int K, int Hd, bxStream stream) {
  BX_REQUIRE(B > 0 && B <= 65535 && Nb > 0 && NS > 0, "bx_fusion_values: need 1 <= B <= 65535, Nb >= 1, NS >= 1 (B = %d, Nb = %d, NS = %d)", B, Nb, NS);
  BX_REQUIRE(K >= 1 && K <= 16 && Hd >= 2 * K && Hd <= 1024, "bx_fusion_values: need 1 <= K <= 16 and 2K <= Hd <= 1024 (K = %d, Hd = %d)", K, Hd);
  BX_REQUIRE(score_kind == BX_FUSION_SCORE_PROB || score_kind == BX_FUSION_SCORE_LOGPROB, "bx_fusion_values: unknown score kind %d", score_kind);
  BX_REQUIRE((long long)B * NS * K < (1ll << 31), "bx_fusion_values: B * NS * K = %lld beyond 32-bit offsets", (long long)B * NS * K);
  BX_REQUIRE(e_x && s_x && e_bg && s_bg && masks && w1 && b1 && w2 && b2 && v, "bx_fusion_values: null pointer");
  hipStream_t s = (hipStream_t)stream;
#define FS_GO(KM, NG) fs_dispatch_mpt<KM, NG>(e_x, s_x, e_bg, s_bg, masks, w1, b1, w2, b2, v, B, Nb, NS, K, Hd, score_kind, s)
  if (K <= 4) FS_GO(4, 2);
  else if (K <= 6) FS_GO(6, 2);
  else if (K <= 8) FS_GO(8, 2);
  else FS_GO(16, 4);
#undef FS_GO
  BX_CHECK_LAUNCH("bx_fusion_values");
  return BX_OK;
}

// ------------------------------------------------------------------------------------------------
// phi[r,i] = sum over the coalitions S without player i, in ascending S, of weights[|S|] * (v[r, S + i] - v[r, S]): one thread per
// (row, player), every product and sum rounded on its own
__global__ __launch_bounds__(256) void k_shapley_exact(const double* __restrict__ v, const double* __restrict__ w, double* __restrict__ phi,
                                                        int R, int M) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= R * M) return;
  const int r = idx / M, i = idx - r * M;
  const double* vr = v + ((size_t)r << M);
  const uint32_t bit = 1u << i, half = 1u << (M - 1);
  double s = 0.0;
  for (uint32_t t = 0; t < half; ++t) {
    const uint32_t S = ((t >> i) << (i + 1)) | (t & (bit - 1u));          // t with a zero inserted at bit i: ascending t is ascending S
    s += w[__popc(S)] * (vr[S | bit] - vr[S]);
  }
  phi[idx] = s;
}
extern "C" int bx_shapley_exact(const double* v, const double* weights, double* phi, int R, int M, bxStream stream) {
  BX_REQUIRE(R > 0 && M >= 1 && M <= 16, "bx_shapley_exact: need R >= 1 and 1 <= M <= 16 (R = %d, M = %d)", R, M);
  BX_REQUIRE(((long long)R << M) < (1ll << 31), "bx_shapley_exact: R * 2^M = %lld beyond 32-bit offsets", (long long)R << M);
  BX_REQUIRE(v && weights && phi, "bx_shapley_exact: null pointer");
  hipLaunchKernelGGL(k_shapley_exact, dim3(bx_ceil_div((long long)R * M, 256)), dim3(256), 0, (hipStream_t)stream, v, weights, phi, R, M);
  BX_CHECK_LAUNCH("bx_shapley_exact");
  return BX_OK;
}

// out[r] = ((v(all) - v(EEG)) - v(spec)) + v(none) of the modality game's rows v [R,4] = (none, EEG, spec, all)
__global__ __launch_bounds__(256) void k_fusion_interaction(const double* __restrict__ v, double* __restrict__ out, int R) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const double* vr = v + (size_t)r * 4;
  out[r] = ((vr[3] - vr[1]) - vr[2]) + vr[0];
}
extern "C" int bx_fusion_interaction(const double* v, double* out, int R, bxStream stream) {
  BX_REQUIRE(R > 0 && R < (1 << 29), "bx_fusion_interaction: need 1 <= R < 2^29 (R = %d)", R);
  BX_REQUIRE(v && out, "bx_fusion_interaction: null pointer");
  hipLaunchKernelGGL(k_fusion_interaction, dim3(bx_ceil_div(R, 256)), dim3(256), 0, (hipStream_t)stream, v, out, R);
  BX_CHECK_LAUNCH("bx_fusion_interaction");
  return BX_OK;
}
