// Infidelity and max-sensitivity of an explanation (Yeh et al., NeurIPS 2019; Captum's metrics.infidelity and metrics.sensitivity_max):
// the rows x - sigma * z written straight in the model's layouts with SmoothGrad's Gaussian stream drawn in registers, the fp64 dot of
// the same noise with the attribution, the drops and the mean square of (beta * dot - drop); the uniformly perturbed rows of
// sensitivity_max, the fp64 distance of two rows and the largest relative distance.  The forward passes between rows and finish are the
// model's own kernels; the explanations of sensitivity_max are the caller's.  See include/brainxai.h for the definition and each entry
// point.  The file is compiled with -ffp-contract=off: sigma * z and x - (sigma * z) are two separate fp32 roundings, beta * d - drop two
// fp64 ones, so that a numpy restatement matches the rows bit for bit given z.
#include "perturb_rows.h"
#include "sample_rows.h"

#define INF_MAX_K 32
#define INF_DOT_CK 4                    // classes a dot workgroup serves with one pass over the noise (one class alone: 1)

static int inf_chunk_ok(const char* who, int B, int N, int b0, int nb, int n0, int n) {
  BX_REQUIRE(B > 0 && N > 0, "%s: bad shape B=%d N=%d", who, B, N);
  BX_REQUIRE(b0 >= 0 && nb >= 1 && (long long)b0 + nb <= B, "%s: samples b0 = %d, nb = %d outside 0..B = %d", who, b0, nb, B);
  BX_REQUIRE(n0 >= 0 && n >= 1 && (long long)n0 + n <= N, "%s: draws n0 = %d, n = %d outside 0..N = %d", who, n0, n, N);
  return BX_OK;
}

// ---- infidelity: the rows ---------------------------------------------------------------------------------------------------------------
// I[i] = fl32(sigma * z) of the cells cell0 .. cell0 + 3 of draw k of sample b.  cell0 % 4 == 0: one Philox block; otherwise the cells
// straddle two blocks, both are drawn and the four values picked with constant register indices (sh is the same in every lane).
__device__ __forceinline__ void inf_noise4(uint32_t cell0, uint32_t k, uint32_t b, uint32_t k0, uint32_t k1, float s, float I[4]) {
  const uint32_t sh = cell0 & 3u, qa = cell0 >> 2;
  float z[8];
  sg_normal4(qa, k, b, k0, k1, z);
  if (sh) {
    sg_normal4(qa + 1u, k, b, k0, k1, z + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = sh == 1u ? z[i + 1] : sh == 2u ? z[i + 2] : z[i + 3];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) I[i] = s * z[i];
}

// x fp32 NCHW [B,C,H,W] -> rows [nb*n,H,W,8] in T.  A thread owns the pixels 4q .. 4q+3 and all their channels, for the PERTURB_SPW rows
// of its group: pixel cells (per_pixel) share one Philox block of counter q over the channels; element cells c * HW + p take the block(s)
// of every channel.  V = 4: 16-byte loads of x (HW % 4 == 0, aligned x, so that no channel's cells straddle blocks); V = 1: element by
// element, the last block of a plane may be partial.  Every pixel of every row is written once, all 8 channels of it.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_infid_rows_spec(const float* __restrict__ x, const float* __restrict__ sigma, T* __restrict__ out, int HW, int C,
                                                         int per_pixel, int b0, int n0, int n, uint32_t k0, uint32_t k1) {
  const int q = blockIdx.x * 256 + threadIdx.x, p0 = q * 4;
  if (p0 >= HW) return;
  const int bl = blockIdx.z, b = b0 + bl, j0 = blockIdx.y * PERTURB_SPW;
  const int m = V == 4 ? 4 : (HW - p0 < 4 ? HW - p0 : 4);
  float xv[PERTURB_MAX_C][4];
#pragma unroll
  for (int c = 0; c < PERTURB_MAX_C; ++c) {
    const float* src = x + ((size_t)b * C + (c < C ? c : 0)) * HW + p0;      // clamped, unconditional loads
    if (V == 4) {
      ld4(src, 0, xv[c]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[c][i] = src[i < m ? i : 0];
    }
  }
  const float s = sigma[b];
  for (int sj = 0; sj < PERTURB_SPW && j0 + sj < n; ++sj) {
    const uint32_t k = (uint32_t)(n0 + j0 + sj);
    float I[PERTURB_MAX_C][4];
    if (per_pixel) {
      inf_noise4((uint32_t)p0, k, (uint32_t)b, k0, k1, s, I[0]);
#pragma unroll
      for (int c = 1; c < PERTURB_MAX_C; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) I[c][i] = I[0][i];
    } else {
#pragma unroll
      for (int c = 0; c < PERTURB_MAX_C; ++c) {
        if (c < C) {
          inf_noise4((uint32_t)c * (uint32_t)HW + (uint32_t)p0, k, (uint32_t)b, k0, k1, s, I[c]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) I[c][i] = 0.f;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < m) {
        float v[PERTURB_MAX_C];
#pragma unroll
        for (int c = 0; c < PERTURB_MAX_C; ++c) v[c] = c < C ? xv[c][i] - I[c][i] : 0.f;
        perturb_store8(out, (size_t)bl * n + j0 + sj, HW, p0 + i, v);
      }
  }
}
extern "C" int bx_infidelity_rows_spec(const float* x, const float* sigma, void* out, int B, int C, int H, int W, int Cp, int per_pixel, int N, int b0,
                                       int nb, int n0, int n, uint64_t seed, int dtype, bxStream stream) {
  const char* who = "bx_infidelity_rows_spec";
  BX_DTYPE_OK(dtype);
  BX_REQUIRE(H > 0 && W > 0, "%s: bad shape H=%d W=%d", who, H, W);
  int rc = inf_chunk_ok(who, B, N, b0, nb, n0, n);
  if (rc) return rc;
  if ((rc = perturb_layout_ok(who, "channels", C, Cp)) != BX_OK) return rc;
  BX_REQUIRE((long long)B * C * H * W < (1ll << 31) && (long long)B * N < (1ll << 31), "%s: B * C * H * W or B * N beyond 32-bit offsets", who);
  if ((rc = perturb_rows_ok(who, "nb", nb, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && sigma && out, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", who);
  const int HW = H * W;
  const dim3 grid = perturb_grid(bx_ceil_div(HW, 4), 256, n, nb);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const bool vec = sample_vec4(HW, x);
  BX_DISPATCH_DTYPE(dtype, T, {
    if (vec) hipLaunchKernelGGL((k_infid_rows_spec<T, 4>), grid, dim3(256), 0, (hipStream_t)stream, x, sigma, (T*)out, HW, C, per_pixel ? 1 : 0, b0, n0, n, k0, k1);
    else hipLaunchKernelGGL((k_infid_rows_spec<T, 1>), grid, dim3(256), 0, (hipStream_t)stream, x, sigma, (T*)out, HW, C, per_pixel ? 1 : 0, b0, n0, n, k0, k1);
  });
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// fp32 [B,1,Chans,T] -> [nb*n,1,Chans,T].  The sample is E lines of L cells that share their draws: element cells are one line of
// L = Chans * T, time-column cells E = Chans lines of L = T.  A thread owns the cells 4q .. 4q+3 of every line: the noise of its group's
// rows is drawn once, then the lines are walked.  V = 4: 16-byte accesses (L % 4 == 0, aligned pointers); V = 1: element by element.
template <int V>
__global__ __launch_bounds__(256) void k_infid_rows_eeg(const float* __restrict__ x, const float* __restrict__ sigma, float* __restrict__ out, int E, int L,
                                                        int b0, int n0, int n, uint32_t k0, uint32_t k1) {
  const int q = blockIdx.x * 256 + threadIdx.x, t0 = q * 4;
  if (t0 >= L) return;
  const int bl = blockIdx.z, b = b0 + bl, j0 = blockIdx.y * PERTURB_SPW;
  const int m = V == 4 ? 4 : (L - t0 < 4 ? L - t0 : 4);
  const float s = sigma[b];
  float I[PERTURB_SPW][4];
#pragma unroll
  for (int sj = 0; sj < PERTURB_SPW; ++sj) {
    if (j0 + sj < n) {
      inf_noise4((uint32_t)t0, (uint32_t)(n0 + j0 + sj), (uint32_t)b, k0, k1, s, I[sj]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) I[sj][i] = 0.f;
    }
  }
  const size_t per = (size_t)E * L;
  for (int ch = 0; ch < E; ++ch) {
    const float* src = x + (size_t)b * per + (size_t)ch * L + t0;
    float xv[4];
    if (V == 4) {
      ld4(src, 0, xv);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] = src[i < m ? i : 0];
    }
#pragma unroll
    for (int sj = 0; sj < PERTURB_SPW; ++sj)
      if (j0 + sj < n) {
        float* dst = out + ((size_t)bl * n + j0 + sj) * per + (size_t)ch * L + t0;
        if (V == 4) {
          *reinterpret_cast<float4*>(dst) = make_float4(xv[0] - I[sj][0], xv[1] - I[sj][1], xv[2] - I[sj][2], xv[3] - I[sj][3]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (i < m) dst[i] = xv[i] - I[sj][i];
        }
      }
  }
}
extern "C" int bx_infidelity_rows_eeg(const float* x, const float* sigma, float* out, int B, int Chans, int T, int per_column, int N, int b0, int nb,
                                      int n0, int n, uint64_t seed, bxStream stream) {
  const char* who = "bx_infidelity_rows_eeg";
  BX_REQUIRE(Chans > 0 && T > 0, "%s: bad shape Chans=%d T=%d", who, Chans, T);
  int rc = inf_chunk_ok(who, B, N, b0, nb, n0, n);
  if (rc) return rc;
  BX_REQUIRE((long long)B * Chans * T < (1ll << 31) && (long long)B * N < (1ll << 31), "%s: B * Chans * T or B * N beyond 32-bit offsets", who);
  if ((rc = perturb_rows_ok(who, "nb", nb, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && sigma && out, "%s: null pointer", who);
  const int E = per_column ? Chans : 1, L = per_column ? T : Chans * T;
  const dim3 grid = perturb_grid(bx_ceil_div(L, 4), 256, n, nb);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  if (sample_vec4(L, x, out))
    hipLaunchKernelGGL((k_infid_rows_eeg<4>), grid, dim3(256), 0, (hipStream_t)stream, x, sigma, out, E, L, b0, n0, n, k0, k1);
  else
    hipLaunchKernelGGL((k_infid_rows_eeg<1>), grid, dim3(256), 0, (hipStream_t)stream, x, sigma, out, E, L, b0, n0, n, k0, k1);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- fixed-order sum of 256 per-thread fp64 partials: a pairwise tree over the thread index, the same for every launch -------------------
template <int NV>
__device__ __forceinline__ void inf_block_sum(double (&sm)[NV][256], const double (&acc)[NV]) {
#pragma unroll
  for (int v = 0; v < NV; ++v) sm[v][threadIdx.x] = acc[v];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
#pragma unroll
      for (int v = 0; v < NV; ++v) sm[v][threadIdx.x] += sm[v][threadIdx.x + st];
    }
    __syncthreads();
  }
}

// ---- infidelity: the dot ------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, group of CK classes): the noise of the row is drawn again (it was never stored), thread t takes the
// Philox blocks t, t + 256, ... in ascending order, the products (double)I * (double)phi are exact, the per-thread sums meet in the
// tree above.  The order is a function of `cells` alone: no bit of d depends on how the rows were split into calls.  No atomics.
template <int CK>
__global__ __launch_bounds__(256) void k_infid_dot(const float* __restrict__ phi, const float* __restrict__ sigma, double* __restrict__ d, int n, int cells,
                                                   int Kc, uint32_t k0, uint32_t k1, int row0, int vec) {
  __shared__ double sm[CK][256];
  const int j = row0 + blockIdx.x, b = j / n, k = j - b * n, c0 = blockIdx.y * CK;
  const float s = sigma[b];
  const int quads = (cells + 3) >> 2;
  double acc[CK];
#pragma unroll
  for (int cc = 0; cc < CK; ++cc) acc[cc] = 0.0;
  for (int q = threadIdx.x; q < quads; q += 256) {
    float I[4];
    inf_noise4((uint32_t)q * 4u, (uint32_t)k, (uint32_t)b, k0, k1, s, I);
    const int m = cells - q * 4 < 4 ? cells - q * 4 : 4;
#pragma unroll
    for (int cc = 0; cc < CK; ++cc) {
      const int c = c0 + cc < Kc ? c0 + cc : Kc - 1;                         // clamped: a spare slot repeats the last class and is not stored
      const float* ph = phi + ((size_t)b * Kc + c) * cells + (size_t)q * 4;
      float pv[4];
      if (vec) {
        ld4(ph, 0, pv);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = ph[i < m ? i : 0];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < m) acc[cc] += (double)I[i] * (double)pv[i];
    }
  }
  inf_block_sum<CK>(sm, acc);
  if ((int)threadIdx.x < CK && c0 + (int)threadIdx.x < Kc) d[((size_t)b * Kc + c0 + threadIdx.x) * n + k] = sm[threadIdx.x][0];
}
extern "C" int bx_infidelity_dot(const float* phi, const float* sigma, double* d, int B, int n, int cells, int Kc, uint64_t seed, int row0, int rows,
                                 bxStream stream) {
  const char* who = "bx_infidelity_dot";
  SAMPLE_TRY(sample_rows_ok(who, B, n, cells, row0, rows, false));
  BX_REQUIRE(Kc >= 1, "%s: bad class count Kc=%d", who, Kc);
  if (Kc > INF_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, Kc, INF_MAX_K);
  BX_REQUIRE((long long)B * Kc * cells < (1ll << 31) && (long long)B * Kc * n < (1ll << 31), "%s: B * Kc * cells or B * Kc * n beyond 32-bit offsets", who);
  BX_REQUIRE(phi && sigma && d, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)d & 7) == 0, "%s: d must be 8-byte aligned", who);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const int vec = sample_vec4(cells, phi);
  if (Kc == 1)
    hipLaunchKernelGGL((k_infid_dot<1>), dim3(rows, 1), dim3(256), 0, (hipStream_t)stream, phi, sigma, d, n, cells, Kc, k0, k1, row0, vec);
  else
    hipLaunchKernelGGL((k_infid_dot<INF_DOT_CK>), dim3(rows, bx_ceil_div(Kc, INF_DOT_CK)), dim3(256), 0, (hipStream_t)stream, phi, sigma, d, n, cells, Kc, k0,
                       k1, row0, vec);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- infidelity: drops, beta and the mean square ----------------------------------------------------------------------------------------
// One thread per (sample, class) pair q, draws in ascending k; every operation is fp64 and rounds on its own.
__global__ __launch_bounds__(64) void k_infid_finish(const double* __restrict__ d, const float* __restrict__ S, const float* __restrict__ clean,
                                                     const int* __restrict__ classes, double* __restrict__ infid, double* __restrict__ beta,
                                                     double* __restrict__ drops, int Q, int n, int K, int normalize) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= Q) return;
  int b = q, c;
  if (classes) { c = classes[q]; c = c < 0 ? 0 : (c >= K ? K - 1 : c); }
  else { b = q / K; c = q - b * K; }
  const double* dq = d + (size_t)q * n;
  double* dr = drops + (size_t)q * n;
  const double s0 = (double)clean[(size_t)b * K + c];
  double sdd = 0.0, sd2 = 0.0;
  for (int k = 0; k < n; ++k) {
    const double dl = s0 - (double)S[((size_t)b * n + k) * K + c];
    dr[k] = dl;
    const double dk = dq[k];
    sdd += dk * dl;
    sd2 += dk * dk;
  }
  const double bt = normalize ? (sd2 == 0.0 ? 0.0 : sdd / sd2) : 1.0;
  double sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double t = bt * dq[k] - dr[k];
    sum += t * t;
  }
  infid[q] = sum / (double)n;
  beta[q] = bt;
}
extern "C" int bx_infidelity_finish(const double* d, const float* S, const float* clean, const int* classes, double* infid, double* beta, double* drops,
                                    int B, int n, int K, int normalize, bxStream stream) {
  const char* who = "bx_infidelity_finish";
  BX_REQUIRE(B > 0 && n > 0 && K >= 1, "%s: bad shape B=%d n=%d K=%d", who, B, n, K);
  if (K > INF_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, K, INF_MAX_K);
  BX_REQUIRE((long long)B * n * K < (1ll << 31), "%s: B * n * K beyond 32-bit offsets", who);
  BX_REQUIRE(d && S && clean && infid && beta && drops, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)d | (uintptr_t)infid | (uintptr_t)beta | (uintptr_t)drops) & 7) == 0, "%s: the fp64 arrays must be 8-byte aligned", who);
  const int Q = classes ? B : B * K;
  hipLaunchKernelGGL(k_infid_finish, dim3(bx_ceil_div(Q, 64)), dim3(64), 0, (hipStream_t)stream, d, S, clean, classes, infid, beta, drops, Q, n, K,
                     normalize ? 1 : 0);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- sensitivity_max: the rows -----------------------------------------------------------------------------------------------------------
// The noise rows of sample_rows.h with the uniform draw: row = fl32(x + fl32(radius * u)), u in [-1, 1) from word e & 3 of the block of
// counter (e >> 2, k, b, 1).  x == nullptr: the row is u itself.
extern "C" int bx_sensitivity_rows(const float* x, const float* radius, float* out, int B, int n, int per, uint64_t seed, int row0, int rows,
                                   bxStream stream) {
  const char* who = "bx_sensitivity_rows";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  BX_REQUIRE(out && (x == nullptr) == (radius == nullptr), "%s: null pointer (x and radius are given or omitted together)", who);
  return sample_noise_rows<SampleUniform>(who, stream, x, radius, out, n, per, seed, row0, rows);
}

// ---- sensitivity_max: distances and the result --------------------------------------------------------------------------------------------
// One workgroup per row: dist[r] = sqrt( sum_e ((double)a[r,e] - (double)ref[(row0 + r) / n, e])^2 ), thread t takes e = t, t + 256, ... in
// ascending order, then the fixed tree.  ref == nullptr: the norm of a[r].  The difference of two floats is exact in fp64.
__global__ __launch_bounds__(256) void k_sens_dist(const float* __restrict__ a, const float* __restrict__ ref, double* __restrict__ dist, int n, int per,
                                                   int row0) {
  __shared__ double sm[1][256];
  const int r = blockIdx.x, b = (row0 + r) / n;
  const float* ar = a + (size_t)r * per;
  const float* rr = ref ? ref + (size_t)b * per : nullptr;
  double acc[1] = {0.0};
  for (int e = threadIdx.x; e < per; e += 256) {
    double v = (double)ar[e];
    if (rr) v -= (double)rr[e];
    acc[0] += v * v;
  }
  inf_block_sum<1>(sm, acc);
  if (threadIdx.x == 0) dist[r] = sqrt(sm[0][0]);
}
extern "C" int bx_sensitivity_dist(const float* a, const float* ref, double* dist, int B, int n, int per, int row0, int rows, bxStream stream) {
  const char* who = "bx_sensitivity_dist";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  BX_REQUIRE(a && dist, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)dist & 7) == 0, "%s: dist must be 8-byte aligned", who);
  hipLaunchKernelGGL(k_sens_dist, dim3(rows), dim3(256), 0, (hipStream_t)stream, a, ref, dist, n, per, row0);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// sens[b] = max_k dist[b,k] / (norms[b] == 0 ? 1 : norms[b]): one thread per sample
__global__ __launch_bounds__(64) void k_sens_finish(const double* __restrict__ dist, const double* __restrict__ norms, double* __restrict__ sens, int B,
                                                    int n) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double m = dist[(size_t)b * n];
  for (int k = 1; k < n; ++k) {
    const double v = dist[(size_t)b * n + k];
    m = v > m ? v : m;
  }
  const double nb = norms[b];
  sens[b] = m / (nb == 0.0 ? 1.0 : nb);
}
extern "C" int bx_sensitivity_finish(const double* dist, const double* norms, double* sens, int B, int n, bxStream stream) {
  const char* who = "bx_sensitivity_finish";
  BX_REQUIRE(B > 0 && n > 0, "%s: bad shape B=%d n=%d", who, B, n);
  BX_REQUIRE((long long)B * n < (1ll << 31), "%s: B * n beyond 32-bit offsets", who);
  BX_REQUIRE(dist && norms && sens, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)dist | (uintptr_t)norms | (uintptr_t)sens) & 7) == 0, "%s: the fp64 arrays must be 8-byte aligned", who);
  hipLaunchKernelGGL(k_sens_finish, dim3(bx_ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, dist, norms, sens, B, n);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
