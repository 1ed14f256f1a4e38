// Expected gradients (SHAP's GradientExplainer; Erion et al. 2021), batched: the interpolants of every (sample, draw) pair written in one
// launch, the fp64 running sum of (x - background) * gradient in fixed draw order (the walk of sample_rows.h), the mean and the
// channel-summed map, the one-hot gradient seeds of sample-major rows and the reference's mean |.| per electrode.  The forward and
// backward passes between rows and accumulate are the model's own kernels.  See include/brainxai.h for each entry point.
// The file is compiled with -ffp-contract=off: d = x - bg, alpha * d and bg + (alpha * d) are three separate fp32 roundings, so that a
// numpy float32 restatement matches the rows bit for bit.
#include "sample_rows.h"

// the window of sample_rows_ok, and the background's Nb rows
static int eg_rows_ok(const char* who, int B, int Nb, int n, int per, int row0, int rows) {
  BX_REQUIRE(B > 0 && Nb > 0 && n > 0 && per > 0, "%s: bad shape B=%d Nb=%d n=%d per=%d", who, B, Nb, n, per);
  BX_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * per < (1ll << 31) && (long long)Nb * per < (1ll << 31),
             "%s: B * n, B * per or Nb * per beyond 32-bit offsets", who);
  SAMPLE_TRY(sample_window_ok(who, B, n, row0, rows));
  return sample_out_ok(who, rows, per);
}
__device__ __forceinline__ int eg_clamp(int v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

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
    float xv[V], bv[V], o[V];
    sample_ld<V>(x + (size_t)b * per + e, xv);
    sample_ld<V>(bg + (size_t)i * per + e, bv);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const float d = xv[q] - bv[q];
      const float ad = a * d;
      o[q] = bv[q] + ad;
    }
    float* dst = out + (size_t)r * per + e;
    if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[V > 1 ? 1 : 0], o[V > 2 ? 2 : 0], o[V > 3 ? 3 : 0]);
    else dst[0] = o[0];
  }
}
extern "C" int bx_expgrad_rows(const float* x, const float* bg, const int* idx, const float* alpha, float* out, int B, int Nb, int n, int per, int row0,
                               int rows, bxStream stream) {
  SAMPLE_TRY(eg_rows_ok("bx_expgrad_rows", B, Nb, n, per, row0, rows));
  BX_REQUIRE(x && bg && idx && alpha && out, "bx_expgrad_rows: null pointer");
  const int gy = rows < 65535 ? rows : 65535;
  if (sample_vec4(per, x, bg, out))
    hipLaunchKernelGGL((k_expgrad_rows<4>), dim3(bx_ceil_div(per / 4, 256), gy), dim3(256), 0, (hipStream_t)stream, x, bg, idx, alpha, out, Nb, n, per, row0, rows);
  else
    hipLaunchKernelGGL((k_expgrad_rows<1>), dim3(bx_ceil_div(per, 256), gy), dim3(256), 0, (hipStream_t)stream, x, bg, idx, alpha, out, Nb, n, per, row0, rows);
  BX_CHECK_LAUNCH("bx_expgrad_rows");
  return BX_OK;
}

// ---- the running sum --------------------------------------------------------------------------------------------------------------------
// The term of row j is (x - bg[idx[j]]) * g: a thread keeps its elements of x, the gathered background is loaded beside g.  d is one fp32
// rounding; the product of two floats is exact in fp64.
struct EgTerm {
  const float* x; const float* bg; const int* idx; double* acc; int Nb;
  static constexpr int SUMS = 1;
  template <int V> struct Keep { float x[V]; };
  template <int V> struct Row { float bg[V]; };
  double* sum(int) const { return acc; }
  template <int V> __device__ __forceinline__ void sample(Keep<V>& k, int b, int per, int e) const { sample_ld<V>(x + (size_t)b * per + e, k.x); }
  template <int V> __device__ __forceinline__ void row(Row<V>& r, int j, int, int, int per, int e) const {
    sample_ld<V>(bg + (size_t)eg_clamp(idx[j], Nb) * per + e, r.bg);
  }
  template <int V> __device__ __forceinline__ void add(double (&s)[1][V], int q, const Keep<V>& k, float g, const Row<V>& r) const {
    const float d = k.x[q] - r.bg[q];
    s[0][q] += (double)d * (double)g;
  }
};
extern "C" int bx_expgrad_accumulate(const float* x, const float* bg, const int* idx, const float* g, double* acc, int B, int Nb, int n, int per, int Kc,
                                     int slot, int row0, int rows, bxStream stream) {
  const char* who = "bx_expgrad_accumulate";
  SAMPLE_TRY(eg_rows_ok(who, B, Nb, n, per, row0, rows));
  SAMPLE_TRY(sample_slot_ok(who, B, per, Kc, slot));
  BX_REQUIRE(x && bg && idx && g && acc, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)acc & 7) == 0, "%s: acc must be 8-byte aligned", who);
  return sample_accumulate<64, 4, 4>(who, stream, g, sample_vec4(per, x, bg, g), EgTerm{x, bg, idx, acc, Nb}, n, per, Kc, slot, row0, rows);
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

// ---- mean |.| per row: the wave row sum of sample_rows.h, |.| and the fp32 mean ------------------------------------------------------------
extern "C" int bx_mean_abs_rows(const float* v, float* out, int R, int L, bxStream stream) {
  return sample_row_sum<true>("bx_mean_abs_rows", stream, v, out, R, L);
}
