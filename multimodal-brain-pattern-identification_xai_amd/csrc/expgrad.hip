// Expected gradients (SHAP's GradientExplainer; Erion et al. 2021), batched: the interpolants of every (sample, draw) pair written in one
// launch, the fp64 running sum of (x - background) * gradient in fixed draw order, the mean and the channel-summed map, the one-hot
// gradient seeds of sample-major rows and the reference's mean |.| per electrode.  The forward and backward passes between rows and
// accumulate are the model's own kernels.  See include/brainxai.h for the definition and the contract of each entry point.
// The file is compiled with -ffp-contract=off: d = x - bg, alpha * d and bg + (alpha * d) are three separate fp32 roundings, so that a
// numpy float32 restatement matches the rows bit for bit.
#include "bx_common.h"

#define EG_MAX_K 32

// global row j = b * n + k (sample-major); a call handles rows [row0, row0 + rows), which may start and end inside a sample
static int eg_rows_ok(const char* who, int B, int Nb, int n, int per, int row0, int rows) {
  BX_REQUIRE(B > 0 && Nb > 0 && n > 0 && per > 0, "%s: bad shape B=%d Nb=%d n=%d per=%d", who, B, Nb, n, per);
  BX_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * per < (1ll << 31) && (long long)Nb * per < (1ll << 31),
             "%s: B * n, B * per or Nb * per beyond 32-bit offsets", who);
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= (long long)B * n, "%s: rows row0 = %d, rows = %d outside 0..B * n = %d", who, row0, rows,
             B * n);
  BX_REQUIRE((long long)rows * per < (1ll << 31), "%s: rows * per beyond 32-bit offsets", who);
  return BX_OK;
}
static inline bool eg_vec4(int per, const void* a, const void* b, const void* c, const void* d) {
  return per % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}
__device__ __forceinline__ int eg_clamp(int v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

template <int V> struct EgVec;
template <> struct EgVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <> struct EgVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// ---- the interpolants -------------------------------------------------------------------------------------------------------------------
// A thread owns V consecutive elements of a row and walks the rows of its workgroup row; every element of every row is written once.
template <int V>
__global__ __launch_bounds__(256) void k_expgrad_rows(const float* __restrict__ x, const float* __restrict__ bg, const int* __restrict__ idx,
                                                      const float* __restrict__ alpha, float* __restrict__ out, int Nb, int n, int per, int row0, int rows) {
  const int e = (blockIdx.x * 256 + threadIdx.x) * V;
  if (e >= per) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const int j = row0 + r, b = j / n;
    const int i = eg_clamp(idx[j], Nb);
    const float a = alpha[j];
    EgVec<V> xv, bv, o;
    xv.load(x + (size_t)b * per + e);
    bv.load(bg + (size_t)i * per + e);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const float d = xv.v[q] - bv.v[q];
      const float ad = a * d;
      o.v[q] = bv.v[q] + ad;
    }
    o.store(out + (size_t)r * per + e);
  }
}
extern "C" int bx_expgrad_rows(const float* x, const float* bg, const int* idx, const float* alpha, float* out, int B, int Nb, int n, int per, int row0,
                               int rows, bxStream stream) {
  const int rc = eg_rows_ok("bx_expgrad_rows", B, Nb, n, per, row0, rows);
  if (rc) return rc;
  BX_REQUIRE(x && bg && idx && alpha && out, "bx_expgrad_rows: null pointer");
  const int gy = rows < 65535 ? rows : 65535;
  if (eg_vec4(per, x, bg, out, nullptr))
    hipLaunchKernelGGL((k_expgrad_rows<4>), dim3(bx_ceil_div(per / 4, 256), gy), dim3(256), 0, (hipStream_t)stream, x, bg, idx, alpha, out, Nb, n, per, row0, rows);
  else
    hipLaunchKernelGGL((k_expgrad_rows<1>), dim3(bx_ceil_div(per, 256), gy), dim3(256), 0, (hipStream_t)stream, x, bg, idx, alpha, out, Nb, n, per, row0, rows);
  BX_CHECK_LAUNCH("bx_expgrad_rows");
  return BX_OK;
}

// ---- the running sum --------------------------------------------------------------------------------------------------------------------
// A thread owns V consecutive elements of one sample (blockIdx.y walks the samples the call touches) and loops over that sample's draws
// inside the call in ascending k, four rows' loads (gradient and gathered background) in flight.  d is one fp32 rounding; the product of
// two floats is exact in fp64; the sum is fp64.  One thread per element and no atomics: the bits are a function of the inputs alone, and
// a sum carried through acc between calls equals the sum of one call.
#define EG_ACC_THREADS 64
template <int V>
__global__ __launch_bounds__(EG_ACC_THREADS) void k_expgrad_accumulate(const float* __restrict__ x, const float* __restrict__ bg, const int* __restrict__ idx,
                                                                        const float* __restrict__ g, double* __restrict__ acc, int Nb, int n, int per, int Kc,
                                                                        int slot, int row0, int rows, int b_first, int b_count) {
  const int e = (blockIdx.x * EG_ACC_THREADS + threadIdx.x) * V;
  if (e >= per) return;
  for (int bi = blockIdx.y; bi < b_count; bi += gridDim.y) {
    const int b = b_first + bi;
    const int j0 = b * n > row0 ? b * n : row0;
    const int j1 = (b + 1) * n < row0 + rows ? (b + 1) * n : row0 + rows;
    EgVec<V> xv;
    xv.load(x + (size_t)b * per + e);
    double* ap = acc + ((size_t)b * Kc + slot) * per + e;
    double s[V];
#pragma unroll
    for (int q = 0; q < V; ++q) s[q] = ap[q];
    int j = j0;
    for (; j + 4 <= j1; j += 4) {
      EgVec<V> gv[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        gv[u].load(g + (size_t)(j + u - row0) * per + e);
        bv[u].load(bg + (size_t)eg_clamp(idx[j + u], Nb) * per + e);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const float d = xv.v[q] - bv[u].v[q];
          s[q] += (double)d * (double)gv[u].v[q];
        }
    }
    for (; j < j1; ++j) {
      EgVec<V> gv, bv;
      gv.load(g + (size_t)(j - row0) * per + e);
      bv.load(bg + (size_t)eg_clamp(idx[j], Nb) * per + e);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const float d = xv.v[q] - bv.v[q];
        s[q] += (double)d * (double)gv.v[q];
      }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) ap[q] = s[q];
  }
}
extern "C" int bx_expgrad_accumulate(const float* x, const float* bg, const int* idx, const float* g, double* acc, int B, int Nb, int n, int per, int Kc,
                                     int slot, int row0, int rows, bxStream stream) {
  const int rc = eg_rows_ok("bx_expgrad_accumulate", B, Nb, n, per, row0, rows);
  if (rc) return rc;
  BX_REQUIRE(Kc >= 1 && slot >= 0 && slot < Kc, "bx_expgrad_accumulate: class slot %d outside 0..Kc = %d", slot, Kc);
  if (Kc > EG_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_expgrad_accumulate: %d classes, supported 1..%d", Kc, EG_MAX_K);
  BX_REQUIRE((long long)B * Kc * per < (1ll << 31), "bx_expgrad_accumulate: B * Kc * per beyond 32-bit offsets");
  BX_REQUIRE(x && bg && idx && g && acc, "bx_expgrad_accumulate: null pointer");
  BX_REQUIRE(((uintptr_t)acc & 7) == 0, "bx_expgrad_accumulate: acc must be 8-byte aligned");
  const int b_first = row0 / n, b_count = (row0 + rows - 1) / n - b_first + 1;
  const int gy = b_count < 65535 ? b_count : 65535;
  if (eg_vec4(per, x, bg, g, nullptr))
    hipLaunchKernelGGL((k_expgrad_accumulate<4>), dim3(bx_ceil_div(per / 4, EG_ACC_THREADS), gy), dim3(EG_ACC_THREADS), 0, (hipStream_t)stream, x, bg, idx, g,
                       acc, Nb, n, per, Kc, slot, row0, rows, b_first, b_count);
  else
    hipLaunchKernelGGL((k_expgrad_accumulate<1>), dim3(bx_ceil_div(per, EG_ACC_THREADS), gy), dim3(EG_ACC_THREADS), 0, (hipStream_t)stream, x, bg, idx, g, acc,
                       Nb, n, per, Kc, slot, row0, rows, b_first, b_count);
  BX_CHECK_LAUNCH("bx_expgrad_accumulate");
  return BX_OK;
}

// ---- mean and map -----------------------------------------------------------------------------------------------------------------------
// A thread owns one cell p of one (sample, class) plane set: values[q,c,p] = fl32(acc / n) for the C channels, map[q,p] = fl32 of the fp64
// sum of acc / n over the channels in ascending order (with C = 1 the map is the values).
__global__ __launch_bounds__(256) void k_expgrad_finish(const double* __restrict__ acc, float* __restrict__ values, float* __restrict__ map, int C, int HW,
                                                        double n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const size_t q = blockIdx.y;
  double m = 0.0;
  for (int c = 0; c < C; ++c) {
    const size_t o = (q * C + c) * HW + p;
    const double v = acc[o] / n;
    values[o] = (float)v;
    m += v;
  }
  if (map) map[q * HW + p] = (float)m;
}
extern "C" int bx_expgrad_finish(const double* acc, float* values, float* map, int BK, int C, int HW, int n, bxStream stream) {
  BX_REQUIRE(BK > 0 && C > 0 && HW > 0 && n > 0, "bx_expgrad_finish: bad shape BK=%d C=%d HW=%d n=%d", BK, C, HW, n);
  BX_REQUIRE((long long)BK * C * HW < (1ll << 31), "bx_expgrad_finish: BK * C * HW beyond 32-bit offsets");
  BX_REQUIRE(BK <= 65535, "bx_expgrad_finish: %d planes, supported 1..65535", BK);
  BX_REQUIRE(acc && values, "bx_expgrad_finish: null pointer");
  hipLaunchKernelGGL(k_expgrad_finish, dim3(bx_ceil_div(HW, 256), BK), dim3(256), 0, (hipStream_t)stream, acc, values, map, C, HW, (double)n);
  BX_CHECK_LAUNCH("bx_expgrad_finish");
  return BX_OK;
}

// ---- gradient seeds of sample-major rows ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_expgrad_seed(const int* __restrict__ classes, int class_all, float* __restrict__ seed, int row0, int rows, int n,
                                                      int K) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int c = classes ? eg_clamp(classes[(row0 + r) / n], K) : class_all;
  for (int k = 0; k < K; ++k) seed[(size_t)r * K + k] = k == c ? 1.f : 0.f;
}
extern "C" int bx_expgrad_seed(const int* classes, int class_all, float* seed, int B, int n, int K, int row0, int rows, bxStream stream) {
  BX_REQUIRE(B > 0 && n > 0 && K > 0, "bx_expgrad_seed: bad shape B=%d n=%d K=%d", B, n, K);
  BX_REQUIRE((long long)B * n < (1ll << 31), "bx_expgrad_seed: B * n beyond 32-bit offsets");
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= (long long)B * n, "bx_expgrad_seed: rows row0 = %d, rows = %d outside 0..B * n = %d", row0,
             rows, B * n);
  BX_REQUIRE((long long)rows * K < (1ll << 31), "bx_expgrad_seed: rows * K beyond 32-bit offsets");
  BX_REQUIRE(classes || (class_all >= 0 && class_all < K), "bx_expgrad_seed: class %d outside [0, %d)", class_all, K);
  BX_REQUIRE(seed, "bx_expgrad_seed: null pointer");
  hipLaunchKernelGGL(k_expgrad_seed, dim3(bx_ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, classes, class_all, seed, row0, rows, n, K);
  BX_CHECK_LAUNCH("bx_expgrad_seed");
  return BX_OK;
}

// ---- mean |.| per row -------------------------------------------------------------------------------------------------------------------
// One wave per row, whatever the launch: lane l adds |v[r,t]| for t = l, l + 64, ... in ascending t in fp64, the 64 lane sums are added
// by the xor butterfly (offsets 32, 16, .., 1: the same tree in every lane), the quotient by L is fp64 and rounded to fp32 once.
__global__ __launch_bounds__(256) void k_mean_abs_rows(const float* __restrict__ v, float* __restrict__ out, int R, int L) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;                                          // wave-uniform
  const float* row = v + (size_t)r * L;
  double s = 0.0;
  for (int t = lane; t < L; t += 64) s += (double)fabsf(row[t]);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) out[r] = (float)(s / (double)L);
}
extern "C" int bx_mean_abs_rows(const float* v, float* out, int R, int L, bxStream stream) {
  BX_REQUIRE(R > 0 && L > 0, "bx_mean_abs_rows: bad shape R=%d L=%d", R, L);
  BX_REQUIRE((long long)R * L < (1ll << 31), "bx_mean_abs_rows: R * L beyond 32-bit offsets");
  BX_REQUIRE(v && out, "bx_mean_abs_rows: null pointer");
  hipLaunchKernelGGL(k_mean_abs_rows, dim3(bx_ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, v, out, R, L);
  BX_CHECK_LAUNCH("bx_mean_abs_rows");
  return BX_OK;
}
