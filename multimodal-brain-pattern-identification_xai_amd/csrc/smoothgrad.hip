// SmoothGrad, SmoothGrad^2 and VarGrad (Smilkov et al. 2017; Hooker et al. 2019; Adebayo et al. 2018; Captum's NoiseTunnel): the
// per-sample noise scale, the noisy rows of every (sample, draw) pair written in one launch with their Gaussian noise drawn in
// registers (Philox4x32-10 counters, Box-Muller), the fp64 running sums of the gradient and of its square in fixed draw order, and the
// mean / mean square / variance with the channel-max map.  The forward and backward passes between rows and accumulate are the model's
// own kernels; the one-hot gradient seeds are bx_expgrad_seed.  See include/brainxai.h for the definition and each entry point.
// The file is compiled with -ffp-contract=off: sigma * z and x + (sigma * z) are two separate fp32 roundings, and the variance is four
// separate fp64 operations, so that a numpy restatement matches the rows bit for bit given z.
#include "bx_philox.h"

#define SG_MAX_K 32

// global row j = b * n + k (sample-major); a call handles rows [row0, row0 + rows), which may start and end inside a sample
static int sg_rows_ok(const char* who, int B, int n, int per, int row0, int rows) {
  BX_REQUIRE(B > 0 && n > 0 && per > 0, "%s: bad shape B=%d n=%d per=%d", who, B, n, per);
  BX_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * per < (1ll << 31), "%s: B * n or B * per beyond 32-bit offsets", who);
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= (long long)B * n, "%s: rows row0 = %d, rows = %d outside 0..B * n = %d", who, row0, rows,
             B * n);
  BX_REQUIRE((long long)rows * per < (1ll << 31), "%s: rows * per beyond 32-bit offsets", who);
  return BX_OK;
}
static inline bool sg_vec4(int per, const void* a, const void* b, const void* c) {
  return per % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
}

// ---- the noise scale --------------------------------------------------------------------------------------------------------------------
// One workgroup per sample.  Minimum and maximum do not depend on the order they are taken in, apart from the sign of a zero; the
// modulus of the range clears that one bit, so the result is a function of the sample alone.
__device__ __forceinline__ float sg_wave_min(float v) { return -wave_max(-v); }
__global__ __launch_bounds__(256) void k_smoothgrad_sigma(const float* __restrict__ x, float* __restrict__ sigma, int per, float level) {
  __shared__ float s_lo[4], s_hi[4];
  const float* row = x + (size_t)blockIdx.x * per;
  float lo = row[0], hi = lo;
  for (int e = threadIdx.x; e < per; e += 256) {
    const float v = row[e];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  lo = sg_wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    const float range = fabsf(hi - lo);
    sigma[blockIdx.x] = level * range;
  }
}
extern "C" int bx_smoothgrad_sigma(const float* x, float* sigma, int B, int per, float level, bxStream stream) {
  BX_REQUIRE(B > 0 && per > 0, "bx_smoothgrad_sigma: bad shape B=%d per=%d", B, per);
  BX_REQUIRE((long long)B * per < (1ll << 31), "bx_smoothgrad_sigma: B * per beyond 32-bit offsets");
  BX_REQUIRE(level >= 0.f && level <= 3.0e38f, "bx_smoothgrad_sigma: noise level %g is negative or not finite", (double)level);
  BX_REQUIRE(x && sigma, "bx_smoothgrad_sigma: null pointer");
  hipLaunchKernelGGL(k_smoothgrad_sigma, dim3(B), dim3(256), 0, (hipStream_t)stream, x, sigma, per, level);
  BX_CHECK_LAUNCH("bx_smoothgrad_sigma");
  return BX_OK;
}

// ---- the noise --------------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 and the fp32 Box-Muller normals (sg_philox, sg_normal2, sg_normal4) live in bx_philox.h, shared with infidelity.hip.

// ---- the rows ---------------------------------------------------------------------------------------------------------------------------
// A thread owns the four consecutive elements 4q .. 4q+3 of a row -- one Philox block -- and walks the rows of its workgroup row; every
// element of every row is written once, the noise lives in registers only.  V = 4: one 16-byte load and store (per % 4 == 0, aligned
// pointers); V = 1: element by element, the last block of a row may be partial.  x == nullptr: the row is z itself.
template <int V>
__global__ __launch_bounds__(256) void k_smoothgrad_rows(const float* __restrict__ x, const float* __restrict__ sigma, float* __restrict__ out, int n, int per,
                                                         uint32_t k0, uint32_t k1, int row0, int rows) {
  const int q = blockIdx.x * 256 + threadIdx.x, e = q * 4;
  if (e >= per) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const int j = row0 + r, b = j / n, k = j - b * n;
    float z[4];
    sg_normal4((uint32_t)q, (uint32_t)k, (uint32_t)b, k0, k1, z);
    float* o = out + (size_t)r * per + e;
    if (V == 4) {
      if (x) {
        const float s = sigma[b];
        const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)b * per + e);
        const float n0 = s * z[0], n1 = s * z[1], n2 = s * z[2], n3 = s * z[3];
        *reinterpret_cast<float4*>(o) = make_float4(xv.x + n0, xv.y + n1, xv.z + n2, xv.w + n3);
      } else {
        *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
      }
    } else {
      const int m = per - e < 4 ? per - e : 4;
      const float s = x ? sigma[b] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < m) {
          if (x) {
            const float nz = s * z[i];
            o[i] = x[(size_t)b * per + e + i] + nz;
          } else {
            o[i] = z[i];
          }
        }
    }
  }
}
extern "C" int bx_smoothgrad_rows(const float* x, const float* sigma, float* out, int B, int n, int per, uint64_t seed, int row0, int rows, bxStream stream) {
  const int rc = sg_rows_ok("bx_smoothgrad_rows", B, n, per, row0, rows);
  if (rc) return rc;
  BX_REQUIRE(out && (x == nullptr) == (sigma == nullptr), "bx_smoothgrad_rows: null pointer (x and sigma are given or omitted together)");
  const int gy = rows < 65535 ? rows : 65535, quads = bx_ceil_div(per, 4);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  if (sg_vec4(per, x, out, nullptr))
    hipLaunchKernelGGL((k_smoothgrad_rows<4>), dim3(bx_ceil_div(quads, 256), gy), dim3(256), 0, (hipStream_t)stream, x, sigma, out, n, per, k0, k1, row0, rows);
  else
    hipLaunchKernelGGL((k_smoothgrad_rows<1>), dim3(bx_ceil_div(quads, 256), gy), dim3(256), 0, (hipStream_t)stream, x, sigma, out, n, per, k0, k1, row0, rows);
  BX_CHECK_LAUNCH("bx_smoothgrad_rows");
  return BX_OK;
}

// ---- the running sums -------------------------------------------------------------------------------------------------------------------
// A thread owns V consecutive elements of one sample (blockIdx.y walks the samples the call touches) and loops over that sample's draws
// inside the call in ascending k, four rows' loads in flight.  The square of a float is exact in fp64; both sums are fp64.  One thread
// per element and no atomics: the bits are a function of the inputs alone, and sums carried between calls equal the sums of one call.
#define SG_ACC_THREADS 64
template <int V>
__global__ __launch_bounds__(SG_ACC_THREADS) void k_smoothgrad_accumulate(const float* __restrict__ g, double* __restrict__ S1, double* __restrict__ S2, int n,
                                                                           int per, int Kc, int slot, int row0, int rows, int b_first, int b_count) {
  const int e = (blockIdx.x * SG_ACC_THREADS + threadIdx.x) * V;
  if (e >= per) return;
  for (int bi = blockIdx.y; bi < b_count; bi += gridDim.y) {
    const int b = b_first + bi;
    const int j0 = b * n > row0 ? b * n : row0;
    const int j1 = (b + 1) * n < row0 + rows ? (b + 1) * n : row0 + rows;
    const size_t at = ((size_t)b * Kc + slot) * per + e;
    double s1[V], s2[V];
#pragma unroll
    for (int q = 0; q < V; ++q) { s1[q] = S1[at + q]; s2[q] = S2[at + q]; }
    int j = j0;
    for (; j + 4 <= j1; j += 4) {
      float gv[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* p = g + (size_t)(j + u - row0) * per + e;
        if (V == 4) ld4(p, 0, gv[u]); else gv[u][0] = p[0];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const double d = (double)gv[u][q];
          s1[q] += d;
          s2[q] += d * d;
        }
    }
    for (; j < j1; ++j) {
      float gv[V];
      const float* p = g + (size_t)(j - row0) * per + e;
      if (V == 4) ld4(p, 0, gv); else gv[0] = p[0];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const double d = (double)gv[q];
        s1[q] += d;
        s2[q] += d * d;
      }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) { S1[at + q] = s1[q]; S2[at + q] = s2[q]; }
  }
}
extern "C" int bx_smoothgrad_accumulate(const float* g, double* S1, double* S2, int B, int n, int per, int Kc, int slot, int row0, int rows, bxStream stream) {
  const int rc = sg_rows_ok("bx_smoothgrad_accumulate", B, n, per, row0, rows);
  if (rc) return rc;
  BX_REQUIRE(Kc >= 1 && slot >= 0 && slot < Kc, "bx_smoothgrad_accumulate: class slot %d outside 0..Kc = %d", slot, Kc);
  if (Kc > SG_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_smoothgrad_accumulate: %d classes, supported 1..%d", Kc, SG_MAX_K);
  BX_REQUIRE((long long)B * Kc * per < (1ll << 31), "bx_smoothgrad_accumulate: B * Kc * per beyond 32-bit offsets");
  BX_REQUIRE(g && S1 && S2, "bx_smoothgrad_accumulate: null pointer");
  BX_REQUIRE((((uintptr_t)S1 | (uintptr_t)S2) & 7) == 0, "bx_smoothgrad_accumulate: S1 and S2 must be 8-byte aligned");
  const int b_first = row0 / n, b_count = (row0 + rows - 1) / n - b_first + 1;
  const int gy = b_count < 65535 ? b_count : 65535;
  if (sg_vec4(per, g, nullptr, nullptr))
    hipLaunchKernelGGL((k_smoothgrad_accumulate<4>), dim3(bx_ceil_div(per / 4, SG_ACC_THREADS), gy), dim3(SG_ACC_THREADS), 0, (hipStream_t)stream, g, S1, S2, n,
                       per, Kc, slot, row0, rows, b_first, b_count);
  else
    hipLaunchKernelGGL((k_smoothgrad_accumulate<1>), dim3(bx_ceil_div(per, SG_ACC_THREADS), gy), dim3(SG_ACC_THREADS), 0, (hipStream_t)stream, g, S1, S2, n,
                       per, Kc, slot, row0, rows, b_first, b_count);
  BX_CHECK_LAUNCH("bx_smoothgrad_accumulate");
  return BX_OK;
}

// ---- values and map ---------------------------------------------------------------------------------------------------------------------
// A thread owns one cell p of one (sample, class) plane set: values[q,c,p] for the C channels -- the mean S1 / n, the mean square S2 / n
// or the population variance max(0, (S2 - S1 * S1 / n) / n), fp64 operations rounded one by one, then one fp32 rounding -- and
// map[q,p] = the largest |values[q,c,p]| over the channels.
__global__ __launch_bounds__(256) void k_smoothgrad_finish(const double* __restrict__ S1, const double* __restrict__ S2, float* __restrict__ values,
                                                           float* __restrict__ map, int C, int HW, double n, int kind) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const size_t q = blockIdx.y;
  float m = 0.f;
  for (int c = 0; c < C; ++c) {
    const size_t o = (q * C + c) * HW + p;
    double v;
    if (kind == BX_SMOOTHGRAD_MEAN) {
      v = S1[o] / n;
    } else if (kind == BX_SMOOTHGRAD_SQ) {
      v = S2[o] / n;
    } else {
      const double s1 = S1[o];
      const double sq = s1 * s1;
      const double mean_sq = sq / n;
      const double d = S2[o] - mean_sq;
      v = d / n;
      v = v > 0.0 ? v : 0.0;
    }
    const float f = (float)v;
    values[o] = f;
    m = fmaxf(m, fabsf(f));
  }
  if (map) map[q * HW + p] = m;
}
extern "C" int bx_smoothgrad_finish(const double* S1, const double* S2, float* values, float* map, int BK, int C, int HW, int n, int kind, bxStream stream) {
  BX_REQUIRE(BK > 0 && C > 0 && HW > 0 && n > 0, "bx_smoothgrad_finish: bad shape BK=%d C=%d HW=%d n=%d", BK, C, HW, n);
  BX_REQUIRE(kind == BX_SMOOTHGRAD_MEAN || kind == BX_SMOOTHGRAD_SQ || kind == BX_SMOOTHGRAD_VAR, "bx_smoothgrad_finish: unknown kind %d", kind);
  BX_REQUIRE((long long)BK * C * HW < (1ll << 31), "bx_smoothgrad_finish: BK * C * HW beyond 32-bit offsets");
  BX_REQUIRE(BK <= 65535, "bx_smoothgrad_finish: %d planes, supported 1..65535", BK);
  BX_REQUIRE(S1 && S2 && values, "bx_smoothgrad_finish: null pointer");
  hipLaunchKernelGGL(k_smoothgrad_finish, dim3(bx_ceil_div(HW, 256), BK), dim3(256), 0, (hipStream_t)stream, S1, S2, values, map, C, HW, (double)n, kind);
  BX_CHECK_LAUNCH("bx_smoothgrad_finish");
  return BX_OK;
}
