// LIME for images (lime 0.2.0.1, LimeImageExplainer.explain_instance; reference XAI_Multimodality.py:1658-1670), everything after the
// segmentation: the fudged colour table, the perturbed batch straight in the model's channels-last layout, the weighted ridge
// surrogate in fp64 and the per-pixel weight map.  See include/brainxai.h for the contract of each entry point.
#include "perturb_rows.h"

#define LIME_MAX_S 1024
#define LIME_MAX_K 32

static int lime_shape_ok(const char* who, int B, int H, int W, int S) {
  BX_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  if (S < 1 || S > LIME_MAX_S) BX_FAIL(BX_EUNSUPPORTED, "%s: %d segments, supported 1..%d", who, S, LIME_MAX_S);
  BX_REQUIRE((long long)B * H * W < (1ll << 31), "%s: label map beyond 32-bit offsets", who);
  return BX_OK;
}
static int lime_channels_ok(const char* who, int C) {
  if (C < 1 || C > PERTURB_MAX_C) BX_FAIL(BX_EUNSUPPORTED, "%s: %d channels, supported 1..%d (Cp = 8)", who, C, PERTURB_MAX_C);
  return BX_OK;
}

// ---- fudged colours: per (segment, channel) mean of the image, truncated -------------------------------------------------------------
// A workgroup owns nseg = ceil(S / 64) consecutive labels of one image: it scans the whole label map with coalesced loads (the map is
// L2-resident; S = 50 -> 50 workgroups of one label each) and adds only its own pixels to 64-bit integer sums in LDS.  Integer
// addition is order-free, so the result does not depend on scheduling; no workspace and no zeroing launch are needed.
#define LIME_SEG_WG 16
__global__ __launch_bounds__(1024) void k_lime_segment_mean(const unsigned char* __restrict__ img, const int* __restrict__ seg,
                                                            unsigned char* __restrict__ colours, int HW, int C, int S, int nseg) {
  __shared__ unsigned long long acc[LIME_SEG_WG * (PERTURB_MAX_C + 1)];
  const int b = blockIdx.y, s0 = blockIdx.x * nseg, tid = threadIdx.x;
  const int mine = S - s0 < nseg ? S - s0 : nseg;
  if (tid < LIME_SEG_WG * (PERTURB_MAX_C + 1)) acc[tid] = 0ull;
  __syncthreads();
  const int* sg = seg + (size_t)b * HW;
  const unsigned char* im = img + (size_t)b * HW * C;
  for (int p = tid; p < HW; p += 1024) {
    const int s = sg[p] - s0;
    if ((unsigned)s < (unsigned)mine) {
      atomicAdd(&acc[s * (PERTURB_MAX_C + 1) + PERTURB_MAX_C], 1ull);
      for (int c = 0; c < C; ++c) atomicAdd(&acc[s * (PERTURB_MAX_C + 1) + c], (unsigned long long)im[(size_t)p * C + c]);
    }
  }
  __syncthreads();
  if (tid < mine * C) {
    const int s = tid / C, c = tid % C;
    const unsigned long long n = acc[s * (PERTURB_MAX_C + 1) + PERTURB_MAX_C];
    colours[((size_t)b * S + s0 + s) * C + c] = n ? (unsigned char)((double)acc[s * (PERTURB_MAX_C + 1) + c] / (double)n) : (unsigned char)0;
  }
}
extern "C" int bx_lime_segment_mean(const unsigned char* img, const int* segments, unsigned char* colours, int B, int H, int W, int C,
                                    int S, bxStream stream) {
  int rc = lime_shape_ok("bx_lime_segment_mean", B, H, W, S);
  if (rc) return rc;
  if ((rc = lime_channels_ok("bx_lime_segment_mean", C))) return rc;
  BX_REQUIRE(img && segments && colours, "bx_lime_segment_mean: null pointer");
  BX_REQUIRE(B <= 65535, "bx_lime_segment_mean: B = %d", B);
  const int nseg = (S + 63) / 64;                                   // <= LIME_SEG_WG for S <= 1024
  hipLaunchKernelGGL(k_lime_segment_mean, dim3(bx_ceil_div(S, nseg), B), dim3(1024), 0, (hipStream_t)stream, img, segments, colours, H * W, C, S, nseg);
  BX_CHECK_LAUNCH("bx_lime_segment_mean");
  return BX_OK;
}

// ---- perturbed batch ---------------------------------------------------------------------------------------------------------------
// x[(b*n + j), p, :] = scale * (Z[b, n0+j, seg[p]] ? img[b, p, :] : colours[b, seg[p], :]), channels C..7 zero: the expression of
// k_u8_to_nhwc applied to the perturbed uint8 image, which is never materialised.  One thread per pixel; a workgroup writes its 256
// pixels for PERTURB_SPW samples, whose mask rows sit in LDS as bits, so the image and the label map are read once per PERTURB_SPW
// samples (from L2) and the output is written once.  The skeleton is perturb_rows.h's, but this kernel reads a uint8 NHWC image, takes
// its colours from LDS and has no baseline kinds, so it shares that header's host checks, grid and store and keeps its own body.
template <typename T>
__global__ __launch_bounds__(256) void k_lime_perturb(const unsigned char* __restrict__ img, const int* __restrict__ seg,
                                                      const unsigned char* __restrict__ colours, const unsigned char* __restrict__ Z,
                                                      T* __restrict__ x, int HW, int C, int S, int N, int n0, int n, float scale) {
  __shared__ uint32_t bits[PERTURB_SPW][LIME_MAX_S / 32];
  __shared__ unsigned char col[LIME_MAX_S * PERTURB_MAX_C];
  const int b = blockIdx.z, j0 = blockIdx.y * PERTURB_SPW, tid = threadIdx.x;
  {
    const int sj = tid >> 5, w = tid & 31, j = j0 + sj;
    uint32_t m = 0u;
    if (j < n && w * 32 < S) {
      const unsigned char* zr = Z + ((size_t)b * N + n0 + j) * S;
#pragma unroll
      for (int i = 0; i < 32; ++i) {                  // unconditional (clamped) loads: all in flight together
        const int s = w * 32 + i;
        const unsigned char v = zr[s < S ? s : 0];
        if (s < S && v) m |= 1u << i;
      }
    }
    bits[sj][w] = m;
  }
  for (int i = tid; i < S * C; i += 256) col[i] = colours[(size_t)b * S * C + i];
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p >= HW) return;
  int s = seg[(size_t)b * HW + p];
  s = (unsigned)s < (unsigned)S ? s : 0;
  float keep[PERTURB_MAX_C], hide[PERTURB_MAX_C];
#pragma unroll
  for (int c = 0; c < PERTURB_MAX_C; ++c) {
    keep[c] = c < C ? (float)img[((size_t)b * HW + p) * C + c] * scale : 0.f;
    hide[c] = c < C ? (float)col[s * C + c] * scale : 0.f;
  }
  for (int sj = 0; sj < PERTURB_SPW && j0 + sj < n; ++sj) {
    const bool on = (bits[sj][s >> 5] >> (s & 31)) & 1u;
    float v[PERTURB_MAX_C];
#pragma unroll
    for (int c = 0; c < PERTURB_MAX_C; ++c) v[c] = on ? keep[c] : hide[c];
    perturb_store8(x, (size_t)b * n + j0 + sj, HW, p, v);
  }
}
extern "C" int bx_lime_perturb(const unsigned char* img, const int* segments, const unsigned char* colours, const unsigned char* Z,
                               void* x, int B, int H, int W, int C, int Cp, int S, int N, int n0, int n, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  int rc = lime_shape_ok("bx_lime_perturb", B, H, W, S);
  if (rc) return rc;
  if ((rc = perturb_layout_ok("bx_lime_perturb", "channels", C, Cp)) != BX_OK) return rc;
  BX_REQUIRE(N >= 2, "bx_lime_perturb: num_samples N = %d < 2", N);
  BX_REQUIRE(n0 >= 0 && n > 0 && (long long)n0 + n <= N, "bx_lime_perturb: rows n0 = %d, n = %d outside 0..N = %d", n0, n, N);
  if ((rc = perturb_rows_ok("bx_lime_perturb", "B", B, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(img && segments && colours && Z && x, "bx_lime_perturb: null pointer");
  const dim3 grid = perturb_grid((long long)H * W, 256, n, B);
  const float scale = (float)(1.0 / 255.0);
  BX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((k_lime_perturb<T>), grid, dim3(256), 0, (hipStream_t)stream, img, segments, colours, Z,
                                                 (T*)x, H * W, C, S, N, n0, n, scale));
  BX_CHECK_LAUNCH("bx_lime_perturb");
  return BX_OK;
}

// ---- weighted ridge surrogate, fp64 ------------------------------------------------------------------------------------------------
// Every sum below is taken by one thread in index order or by a fixed-shape tree: no float atomics, identical bits run to run.
__device__ __forceinline__ int lime_col(const int* __restrict__ used, int j, int S) {
  if (!used) return j;
  const int c = used[j];
  return (unsigned)c < (unsigned)S ? c : 0;
}

// w_n = sqrt(exp(-d_n^2 / kw^2)), d_n = 1 - sqrt(sum_s Z[n,s] / S): the cosine distance to the all-ones row 0
__global__ __launch_bounds__(256) void k_lime_weights(const unsigned char* __restrict__ Z, double* __restrict__ w, int N, int S, double kw) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N) return;
  const unsigned char* zr = Z + ((size_t)b * N + n) * S;
  int cnt = 0;
  for (int s = 0; s < S; ++s) cnt += zr[s] ? 1 : 0;
  const double d = 1.0 - sqrt((double)cnt / (double)S);
  w[(size_t)b * N + n] = sqrt(exp(-(d * d) / (kw * kw)));
}

// Gram matrix G[s][t] = sum_n w_n z_ns z_nt (32 x 32 tiles, workgroups 0 .. T*T-1 of an image) and the right-hand sides
// r[l][s] = sum_n w_n z_ns (y_n,label(l) - ybar_l) (workgroups T*T .. T*T+T-1, written into coef).  Z is binary, so an entry is a sum
// of w_n over the rows where both bits are set; a chunk of 256 rows is staged in LDS as two 32-bit masks and a weight per row.
// y is centred BEFORE the products, as scikit-learn does: a class whose probability hardly moves over the neighbourhood would
// otherwise lose its coefficients in the cancellation sum w z y - W xbar ybar.  Every right-hand-side workgroup takes the weighted
// means itself (same fixed order, same bits); the first one leaves them in `stats` ([0..31] ybar_l, [32] sum w) for k_lime_solve.
__device__ __forceinline__ double lime_sum256(double v, double* red) {          // 256 threads, fixed tree
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
#define LIME_STATS 40                  // doubles per image behind the Gram matrices in the workspace
__global__ __launch_bounds__(256) void k_lime_gram(const unsigned char* __restrict__ Z, const float* __restrict__ P, const int* __restrict__ labels,
                                                   const int* __restrict__ used, const double* __restrict__ w, double* __restrict__ G,
                                                   double* __restrict__ stats, double* __restrict__ coef, int N, int S, int Sp, int K, int nl) {
  __shared__ uint32_t ms[256], mt[256];
  __shared__ double wl[256], yb[LIME_MAX_K];
  __shared__ float ys[LIME_MAX_K][256];          // right-hand-side role: the chunk's probabilities of the nl labels (a global load
  __shared__ int labs[LIME_MAX_K];               // per row inside the inner loop is a serial L2 round trip per row: 350 us at N = 1000)
  const int T = (Sp + 31) / 32, b = blockIdx.y, tid = threadIdx.x;
  const bool gram = (int)blockIdx.x < T * T;
  const int ts = gram ? (int)blockIdx.x / T : (int)blockIdx.x - T * T, tt = gram ? (int)blockIdx.x % T : 0;
  const int lo = tid & 31, q = tid >> 5;
  const int* ub = used ? used + (size_t)b * Sp : nullptr;
  int lu[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) lu[u] = q + 8 * u < nl ? q + 8 * u : 0;
  if (tid < nl) {
    const int k = labels[(size_t)b * nl + tid];
    labs[tid] = k < 0 ? 0 : (k >= K ? K - 1 : k);
  }
  __syncthreads();
  double ybar[4] = {0.0, 0.0, 0.0, 0.0};
  if (!gram) {
    double v = 0.0;
    for (int n = tid; n < N; n += 256) v += w[(size_t)b * N + n];
    const double Wsum = lime_sum256(v, wl);
    for (int l = 0; l < nl; ++l) {
      const int k = labs[l];
      v = 0.0;
      for (int n = tid; n < N; n += 256) v += w[(size_t)b * N + n] * (double)P[((size_t)b * N + n) * K + k];
      const double t = lime_sum256(v, wl);
      if (tid == 0) yb[l] = t / Wsum;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) ybar[u] = q + 8 * u < nl ? yb[q + 8 * u] : 0.0;
    if (ts == 0) {
      if (tid < nl) stats[(size_t)b * LIME_STATS + tid] = yb[tid];
      if (tid == 0) stats[(size_t)b * LIME_STATS + 32] = Wsum;
    }
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int n0 = 0; n0 < N; n0 += 256) {
    __syncthreads();
    const int n = n0 + tid;
    uint32_t a = 0u, c = 0u;
    double wv = 0.0;
    if (n < N) {
      const unsigned char* zr = Z + ((size_t)b * N + n) * S;
#pragma unroll
      for (int i = 0; i < 32; ++i) {                  // unconditional (clamped) loads, so that they are all in flight together
        const int js = ts * 32 + i, jt = tt * 32 + i;
        const unsigned char vs = zr[lime_col(ub, js < Sp ? js : 0, S)], vt = zr[lime_col(ub, jt < Sp ? jt : 0, S)];
        if (js < Sp && vs) a |= 1u << i;
        if (gram && jt < Sp && vt) c |= 1u << i;
      }
      wv = w[(size_t)b * N + n];
      if (!gram)
        for (int l = 0; l < nl; ++l) ys[l][tid] = P[((size_t)b * N + n) * K + labs[l]];
    }
    ms[tid] = a; mt[tid] = c; wl[tid] = wv;
    __syncthreads();
    const int cnt = N - n0 < 256 ? N - n0 : 256;
    if (gram) {
      for (int r = 0; r < cnt; ++r) {
        const uint32_t sm = ms[r] >> (q * 4);
        const bool t_on = (mt[r] >> lo) & 1u;
        const double x = wl[r];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (t_on && ((sm >> u) & 1u)) ? x : 0.0;
      }
    } else {
      for (int r = 0; r < cnt; ++r) {
        const bool s_on = (ms[r] >> lo) & 1u;
        const double x = wl[r];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += s_on ? x * ((double)ys[lu[u]][r] - ybar[u]) : 0.0;
      }
    }
  }
  if (gram) {
    const int t = tt * 32 + lo;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int s = ts * 32 + q * 4 + u;
      if (s < Sp && t < Sp) G[((size_t)b * Sp + s) * Sp + t] = acc[u];
    }
  } else {
    const int s = ts * 32 + lo;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int l = q + 8 * u;
      if (l < nl && s < Sp) coef[((size_t)b * nl + l) * Sp + s] = acc[u];
    }
  }
}

// One workgroup per image: centring and alpha I, Cholesky of the lower triangle in place in the workspace (column j in LDS for
// the trailing update) with the right-hand sides' forward substitution inside it, their backward substitution in coef, then
// intercept, local_pred and the weighted R^2.  R^2 needs no pass over the N rows: with A beta = r and A = L L^T the residual sum
// sum w (y - yhat)^2 = D - 2 beta.r + beta.(A - alpha I) beta = D - |L^T beta|^2 - alpha |beta|^2, D = sum w (y - ybar)^2, and
// L^T beta is the forward substitution's result, whose squares are summed as its entries appear: R^2 = (|y'|^2 + alpha |beta|^2) / D.
__global__ __launch_bounds__(1024) void k_lime_solve(const unsigned char* __restrict__ Z, const float* __restrict__ P, const int* __restrict__ labels,
                                                     const int* __restrict__ used, const double* __restrict__ w, double* __restrict__ Gall,
                                                     const double* __restrict__ stats, double* __restrict__ coef_all, double* __restrict__ intercept, double* __restrict__ score,
                                                     double* __restrict__ local_pred, int N, int S, int Sp, int K, int nl, double alpha) {
  __shared__ double red[1024], xb[LIME_MAX_S], dg[LIME_MAX_S], col[LIME_MAX_S];
  __shared__ double ybar[LIME_MAX_K], yj[LIME_MAX_K], dev[LIME_MAX_K], ysqs[LIME_MAX_K];
  __shared__ int lab[LIME_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x;
  double* G = Gall + (size_t)b * Sp * Sp;
  double* coef = coef_all + (size_t)b * nl * Sp;
  const double* wb = w + (size_t)b * N;
  const float* Pb = P + (size_t)b * N * K;
  const unsigned char* Zb = Z + (size_t)b * N * S;
  const int* ub = used ? used + (size_t)b * Sp : nullptr;
  if (tid < nl) {
    const int k = labels[(size_t)b * nl + tid];
    lab[tid] = k < 0 ? 0 : (k >= K ? K - 1 : k);
  }
  __syncthreads();
  const double Wsum = stats[(size_t)b * LIME_STATS + 32];
  if (tid < nl) ybar[tid] = stats[(size_t)b * LIME_STATS + tid];
  __syncthreads();
  // 32 threads per label: delta_l = sum w (y - ybar) (what the computed mean leaves: rounding-sized, kept all the same) and
  // D_l = sum w (y - ybar)^2; lane partials over n = lane, lane + 32, ... combined by lane 0 in lane order
  const int grp = tid >> 5, lane = tid & 31;
  {
    double d1 = 0.0, d2 = 0.0;
    if (grp < nl)
      for (int n = lane; n < N; n += 32) {
        const double t = (double)Pb[(size_t)n * K + lab[grp]] - ybar[grp];
        d1 += wb[n] * t;
        d2 += wb[n] * t * t;
      }
    red[tid] = d1; col[tid] = d2;
    __syncthreads();
    if (grp < nl && lane == 0) {
      double s1 = 0.0, s2 = 0.0;
      for (int q = 0; q < 32; ++q) { s1 += red[tid + q]; s2 += col[tid + q]; }
      yj[grp] = s1; dev[grp] = s2;
    }
    __syncthreads();
  }
  for (int s = tid; s < Sp; s += 1024) xb[s] = G[(size_t)s * Sp + s] / Wsum;            // z is 0/1: sum w z = sum w z^2 = G[s][s]
  __syncthreads();
  for (int idx = tid; idx < Sp * Sp; idx += 1024) {
    const int i = idx / Sp, k = idx % Sp;
    G[idx] = G[idx] - Wsum * xb[i] * xb[k] + (i == k ? alpha : 0.0);
  }
  for (int idx = tid; idx < nl * Sp; idx += 1024) coef[idx] -= xb[idx % Sp] * yj[idx / Sp];
  __syncthreads();
  // Cholesky, right-looking; the diagonal of L goes to dg[], G keeps the strict lower triangle of L.  The right-hand sides ride
  // along as nl more rows of the matrix: column j's step also takes y_j = r_j / L_jj and r_k -= L_kj y_j (forward substitution
  // L y = r), so no sweep of its own -- two barriers and an L2 round trip per column -- is spent on it.
  const int tx = tid & 31, ty = tid >> 5;
  double ysq = 0.0;
  for (int j = 0; j < Sp; ++j) {
    const double d = sqrt(G[(size_t)j * Sp + j]);
    if (tid == 0) dg[j] = d;
    for (int i = j + 1 + tid; i < Sp; i += 1024) {
      const double x = G[(size_t)i * Sp + j] / d;
      G[(size_t)i * Sp + j] = x;
      col[i] = x;
    }
    if (tid >= 1024 - nl) {
      const int l = 1023 - tid;
      const double x = coef[(size_t)l * Sp + j] / d;
      coef[(size_t)l * Sp + j] = x;
      yj[l] = x;
      ysq += x * x;
    }
    __syncthreads();
    const int m0 = j + 1, m = Sp - m0, nt = (m + 31) / 32;
    for (int bi = 0; bi < nt; ++bi) {
      const int i = m0 + bi * 32 + ty;
      if (i >= Sp) continue;
      const double ci = col[i];
      for (int bk = 0; bk <= bi; ++bk) {
        const int k = m0 + bk * 32 + tx;
        if (k <= i) G[(size_t)i * Sp + k] -= ci * col[k];
      }
    }
    for (int idx = tid; idx < nl * m; idx += 1024) {
      const int l = idx / m, k = m0 + idx % m;
      coef[(size_t)l * Sp + k] -= col[k] * yj[l];
    }
    __syncthreads();
  }
  // L^T beta = y
  for (int j = Sp - 1; j >= 0; --j) {
    if (tid < nl) {
      const double x = coef[(size_t)tid * Sp + j] / dg[j];
      coef[(size_t)tid * Sp + j] = x;
      yj[tid] = x;
    }
    __syncthreads();
    for (int idx = tid; idx < nl * j; idx += 1024) {
      const int l = idx / j, i = idx % j;
      coef[(size_t)l * Sp + i] -= G[(size_t)j * Sp + i] * yj[l];
    }
    __syncthreads();
  }
  {
    double dot = 0.0, row0 = 0.0, b2 = 0.0;
    if (grp < nl)
      for (int s = lane; s < Sp; s += 32) {
        const double be = coef[(size_t)grp * Sp + s];
        dot += xb[s] * be;
        row0 += Zb[lime_col(ub, s, S)] ? be : 0.0;
        b2 += be * be;
      }
    red[tid] = dot; col[tid] = row0; dg[tid] = b2;
    if (tid >= 1024 - nl) ysqs[1023 - tid] = ysq;
    __syncthreads();
    if (grp < nl && lane == 0) {
      dot = row0 = b2 = 0.0;
      for (int q = 0; q < 32; ++q) { dot += red[tid + q]; row0 += col[tid + q]; b2 += dg[tid + q]; }
      const double c0 = ybar[grp] - dot, fit = ysqs[grp] + alpha * b2, D = dev[grp];
      intercept[(size_t)b * nl + grp] = c0;
      local_pred[(size_t)b * nl + grp] = c0 + row0;
      score[(size_t)b * nl + grp] = D != 0.0 ? fit / D : (fit == 0.0 ? 1.0 : 0.0);
    }
  }
}

static int lime_fit_ok(const char* who, int B, int N, int S, int Sp, int K, int nl) {
  BX_REQUIRE(B > 0, "%s: B = %d", who, B);
  if (S < 1 || S > LIME_MAX_S) BX_FAIL(BX_EUNSUPPORTED, "%s: %d segments, supported 1..%d", who, S, LIME_MAX_S);
  BX_REQUIRE(Sp >= 1 && Sp <= S, "%s: %d used features of %d", who, Sp, S);
  if (K < 1 || K > LIME_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, K, LIME_MAX_K);
  BX_REQUIRE(nl >= 1 && nl <= K, "%s: %d labels of %d classes", who, nl, K);
  BX_REQUIRE(N >= 2, "%s: num_samples N = %d < 2", who, N);
  BX_REQUIRE((unsigned long long)B * N * S < (1ull << 32) && (unsigned long long)B * Sp * Sp * 8 < (1ull << 32) && B <= 65535,
             "%s: masks or workspace beyond 32-bit byte offsets", who);
  return BX_OK;
}
extern "C" size_t bx_lime_fit_workspace(int B, int N, int S, int S_used, int K, int nl) {
  if (lime_fit_ok("bx_lime_fit_workspace", B, N, S, S_used, K, nl) != BX_OK) return 0;
  return ((size_t)B * S_used * S_used + (size_t)B * LIME_STATS) * sizeof(double);
}
extern "C" int bx_lime_fit(const unsigned char* Z, const float* P, const int* labels, const int* used, int B, int N, int S, int S_used,
                           int K, int nl, double alpha, double kernel_width, void* workspace, size_t workspace_bytes, double* coef,
                           double* intercept, double* score, double* local_pred, double* weights, bxStream stream) {
  const int rc = lime_fit_ok("bx_lime_fit", B, N, S, S_used, K, nl);
  if (rc) return rc;
  BX_REQUIRE(alpha > 0.0 && kernel_width > 0.0, "bx_lime_fit: alpha = %g and kernel_width = %g must be positive", alpha, kernel_width);
  BX_REQUIRE(used || S_used == S, "bx_lime_fit: %d used features of %d need the `used` list", S_used, S);
  BX_REQUIRE(Z && P && labels && coef && intercept && score && local_pred && weights && workspace, "bx_lime_fit: null pointer");
  if (workspace_bytes < bx_lime_fit_workspace(B, N, S, S_used, K, nl))
    BX_FAIL(BX_EWORKSPACE, "bx_lime_fit: workspace of %zu bytes, need %zu", workspace_bytes, bx_lime_fit_workspace(B, N, S, S_used, K, nl));
  BX_REQUIRE(((uintptr_t)workspace & 7) == 0, "bx_lime_fit: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int T = (S_used + 31) / 32;
  hipLaunchKernelGGL(k_lime_weights, dim3(bx_ceil_div(N, 256), B), dim3(256), 0, s, Z, weights, N, S, kernel_width);
  hipLaunchKernelGGL(k_lime_gram, dim3(T * T + T, B), dim3(256), 0, s, Z, P, labels, used, weights, (double*)workspace,
                     (double*)workspace + (size_t)B * S_used * S_used, coef, N, S, S_used, K, nl);
  hipLaunchKernelGGL(k_lime_solve, dim3(B), dim3(1024), 0, s, Z, P, labels, used, weights, (double*)workspace,
                     (double*)workspace + (size_t)B * S_used * S_used, coef, intercept, score,
                     local_pred, N, S, S_used, K, nl, alpha);
  BX_CHECK_LAUNCH("bx_lime_fit");
  return BX_OK;
}

// ---- per-pixel weight map: map[b, l, p] = beta[b, l, segments[b, p]] (0 for features outside `used`) ----------------------------------
__global__ __launch_bounds__(256) void k_lime_weight_map(const double* __restrict__ coef, const int* __restrict__ used, const int* __restrict__ seg,
                                                         float* __restrict__ map, int HW, int S, int Sp, int nl) {
  __shared__ float full[LIME_MAX_S];
  const int l = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  for (int i = tid; i < S; i += 256) full[i] = 0.f;
  __syncthreads();
  const int* ub = used ? used + (size_t)b * Sp : nullptr;
  for (int j = tid; j < Sp; j += 256) full[lime_col(ub, j, S)] = (float)coef[((size_t)b * nl + l) * Sp + j];
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p >= HW) return;
  const int s = seg[(size_t)b * HW + p];
  map[((size_t)b * nl + l) * HW + p] = (unsigned)s < (unsigned)S ? full[s] : 0.f;
}
extern "C" int bx_lime_weight_map(const double* coef, const int* used, const int* segments, float* map, int B, int nl, int H, int W, int S,
                                  int S_used, bxStream stream) {
  const int rc = lime_shape_ok("bx_lime_weight_map", B, H, W, S);
  if (rc) return rc;
  BX_REQUIRE(S_used >= 1 && S_used <= S && (used || S_used == S), "bx_lime_weight_map: %d used features of %d", S_used, S);
  BX_REQUIRE(nl >= 1 && nl <= LIME_MAX_K && B <= 65535, "bx_lime_weight_map: %d labels (1..%d), B = %d", nl, LIME_MAX_K, B);
  BX_REQUIRE((unsigned long long)B * nl * H * W * 4 < (1ull << 32), "bx_lime_weight_map: map beyond 32-bit byte offsets");
  BX_REQUIRE(coef && segments && map, "bx_lime_weight_map: null pointer");
  hipLaunchKernelGGL(k_lime_weight_map, dim3(bx_ceil_div((long long)H * W, 256), nl, B), dim3(256), 0, (hipStream_t)stream, coef, used, segments,
                     map, H * W, S, S_used, nl);
  BX_CHECK_LAUNCH("bx_lime_weight_map");
  return BX_OK;
}
