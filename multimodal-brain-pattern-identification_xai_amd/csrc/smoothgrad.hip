// SmoothGrad, SmoothGrad^2 and VarGrad (Smilkov et al. 2017; Hooker et al. 2019; Adebayo et al. 2018; Captum's NoiseTunnel): the
// per-sample noise scale, the noisy rows of every (sample, draw) pair written in one launch with their Gaussian noise drawn in
// registers (Philox4x32-10 counters, Box-Muller), the fp64 running sums of the gradient and of its square in fixed draw order, and the
// mean / mean square / variance with the channel-max map.  The rows and the sums are the noise rows and the walk of sample_rows.h.  The
// forward and backward passes between rows and accumulate are the model's own kernels; the one-hot gradient seeds are bx_expgrad_seed.
// See include/brainxai.h for the definition and each entry point.
// The file is compiled with -ffp-contract=off: sigma * z and x + (sigma * z) are two separate fp32 roundings, and the variance is four
// separate fp64 operations, so that a numpy restatement matches the rows bit for bit given z.
#include "sample_rows.h"

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

// ---- the rows: x + sigma * z, Philox4x32-10 and the fp32 Box-Muller normals of bx_philox.h (shared with infidelity.hip) -------------------
extern "C" int bx_smoothgrad_rows(const float* x, const float* sigma, float* out, int B, int n, int per, uint64_t seed, int row0, int rows, bxStream stream) {
  const char* who = "bx_smoothgrad_rows";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  BX_REQUIRE(out && (x == nullptr) == (sigma == nullptr), "%s: null pointer (x and sigma are given or omitted together)", who);
  return sample_noise_rows<SampleNormal>(who, stream, x, sigma, out, n, per, seed, row0, rows);
}

// ---- the running sums: g and g * g.  The square of a float is exact in fp64. ---------------------------------------------------------------
struct SgTerm {
  double* S1; double* S2;
  static constexpr int SUMS = 2;
  template <int V> struct Keep {};
  template <int V> struct Row {};
  double* sum(int i) const { return i ? S2 : S1; }
  template <int V> __device__ __forceinline__ void sample(Keep<V>&, int, int, int) const {}
  template <int V> __device__ __forceinline__ void row(Row<V>&, int, int, int, int, int) const {}
  template <int V> __device__ __forceinline__ void add(double (&s)[2][V], int q, const Keep<V>&, float g, const Row<V>&) const {
    const double d = (double)g;
    s[0][q] += d;
    s[1][q] += d * d;
  }
};
extern "C" int bx_smoothgrad_accumulate(const float* g, double* S1, double* S2, int B, int n, int per, int Kc, int slot, int row0, int rows, bxStream stream) {
  const char* who = "bx_smoothgrad_accumulate";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  SAMPLE_TRY(sample_slot_ok(who, B, per, Kc, slot));
  BX_REQUIRE(g && S1 && S2, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)S1 | (uintptr_t)S2) & 7) == 0, "%s: S1 and S2 must be 8-byte aligned", who);
  return sample_accumulate<64, 4, 4>(who, stream, g, sample_vec4(per, g), SgTerm{S1, S2}, n, per, Kc, slot, row0, rows);
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
