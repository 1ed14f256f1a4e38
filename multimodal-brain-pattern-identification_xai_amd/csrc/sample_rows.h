// What the sampled-gradient attributions (expected gradients, SmoothGrad, Blur IG, spectral gradients) and the sampled-row metrics
// (infidelity, sensitivity_max) do alike around rows j = b * n + k (sample-major; a call handles the window [row0, row0 + rows), which
// may start and end inside a sample): the host checks of such a window, the fp64 running sums of a per-row term, the rows x + scale *
// noise, and the fp64 sum of a row by one wave.  No sum here uses an atomic or depends on the launch geometry: a thread owns its
// outputs and adds its terms in ascending order, so the bits are a function of the inputs alone, and sums carried through memory
// between calls equal the sums of one call.
//
// A method's running sum is a Term, a small struct passed to k_sample_accumulate by value (its pointers):
//   static constexpr int SUMS                                          the fp64 sums it keeps, 1 or 2
//   double* sum(int i) const                                           their destinations [B,Kc,per] (host side: the launch passes them on)
//   template <int V> struct Keep; void sample(Keep<V>&, b, per, e)     what a thread keeps of sample b for its elements e .. e + V - 1
//   template <int V> struct Row;  void row(Row<V>&, j, k, r, per, e)   what it loads beside g for row j = b * n + k, row r of the call
//   void add(double (&s)[SUMS][V], q, const Keep<V>&, float g, const Row<V>&)     the fp64 update of element q's sums by one row
// The walk adds the rows in ascending j; the loads of U rows (g and Row) are issued before the first add.  Terms are instantiated only in
// files built with -ffp-contract=off (build.py), where every product and every sum of add() rounds on its own, as numpy's do.
// Check a new Term with tools/kernel_resources.py (registers, no scratch).
#pragma once
#include "bx_philox.h"

#define SAMPLE_MAX_K 32                // class slots of a running sum

// ---- host side: the checks of a sample-major window, worded with the entry point's name ----------------------------------------------
#define SAMPLE_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)
static inline int sample_window_ok(const char* who, int B, int n, int row0, int rows) {
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= (long long)B * n, "%s: rows row0 = %d, rows = %d outside 0..B * n = %d", who, row0, rows,
             B * n);
  return BX_OK;
}
// the rows a call reads or writes, [rows,per]
static inline int sample_out_ok(const char* who, int rows, int per) {
  BX_REQUIRE((long long)rows * per < (1ll << 31), "%s: rows * per beyond 32-bit offsets", who);
  return BX_OK;
}
// out = false: the call has no [rows,per] array (bx_infidelity_dot draws its rows again)
static inline int sample_rows_ok(const char* who, int B, int n, int per, int row0, int rows, bool out = true) {
  BX_REQUIRE(B > 0 && n > 0 && per > 0, "%s: bad shape B=%d n=%d per=%d", who, B, n, per);
  BX_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * per < (1ll << 31), "%s: B * n or B * per beyond 32-bit offsets", who);
  SAMPLE_TRY(sample_window_ok(who, B, n, row0, rows));
  return out ? sample_out_ok(who, rows, per) : BX_OK;
}
// the class slot of the sums [B,Kc,per] a call adds to
static inline int sample_slot_ok(const char* who, int B, int per, int Kc, int slot) {
  BX_REQUIRE(Kc >= 1 && slot >= 0 && slot < Kc, "%s: class slot %d outside 0..Kc = %d", who, slot, Kc);
  if (Kc > SAMPLE_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, Kc, SAMPLE_MAX_K);
  BX_REQUIRE((long long)B * Kc * per < (1ll << 31), "%s: B * Kc * per beyond 32-bit offsets", who);
  return BX_OK;
}
// 16-byte accesses of lines of `per` floats: every line starts aligned when the pointers are (a null pointer is)
static inline bool sample_vec4(int per, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return per % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
}

template <int V>
__device__ __forceinline__ void sample_ld(const float* p, float (&v)[V]) {
  if (V == 4) ld4(p, 0, v); else v[0] = p[0];
}

// ---- the running sums -----------------------------------------------------------------------------------------------------------------
// the rows j .. j + N - 1 of sample b: N rows' loads, then their adds in ascending j
template <int V, int N, typename Term>
__device__ __forceinline__ void sample_add_rows(const Term& term, const typename Term::template Keep<V>& keep, const float* __restrict__ g,
                                                double (&s)[Term::SUMS][V], int j, int b, int n, int per, int row0, int e) {
  float gv[N][V];
  typename Term::template Row<V> rv[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    sample_ld<V>(g + (size_t)(j + u - row0) * per + e, gv[u]);
    term.row(rv[u], j + u, j + u - b * n, j + u - row0, per, e);
  }
#pragma unroll
  for (int u = 0; u < N; ++u)
#pragma unroll
    for (int q = 0; q < V; ++q) term.add(s, q, keep, gv[u][q], rv[u]);
}
// A thread owns V consecutive elements of one sample (blockIdx.y walks the samples the call touches) and loops over that sample's rows
// inside the call, U at a time and then one by one.  The sums S0 = term.sum(0) and S1 = term.sum(1) arrive as arguments of their own:
// pointers inside a struct carry no __restrict__, and without it every store to a sum would stand between the compiler and the scalar
// loads of what a Term reads at a wave-uniform address (the weights w[k]).
template <int THREADS, int V, int U, typename Term>
__global__ __launch_bounds__(THREADS) void k_sample_accumulate(const float* __restrict__ g, double* __restrict__ S0, double* __restrict__ S1, Term term, int n,
                                                               int per, int Kc, int slot, int row0, int rows, int b_first, int b_count) {
  double* const sums[2] = {S0, S1};
  const int e = (blockIdx.x * THREADS + threadIdx.x) * V;
  if (e >= per) return;
  for (int bi = blockIdx.y; bi < b_count; bi += gridDim.y) {
    const int b = b_first + bi;
    const int j0 = b * n > row0 ? b * n : row0;
    const int j1 = (b + 1) * n < row0 + rows ? (b + 1) * n : row0 + rows;
    const size_t at = ((size_t)b * Kc + slot) * per + e;
    typename Term::template Keep<V> keep;
    term.sample(keep, b, per, e);
    double s[Term::SUMS][V];
#pragma unroll
    for (int q = 0; q < V; ++q)
#pragma unroll
      for (int i = 0; i < Term::SUMS; ++i) s[i][q] = sums[i][at + q];
    int j = j0;
    for (; j + U <= j1; j += U) sample_add_rows<V, U>(term, keep, g, s, j, b, n, per, row0, e);
    if (U > 1)
      for (; j < j1; ++j) sample_add_rows<V, 1>(term, keep, g, s, j, b, n, per, row0, e);
#pragma unroll
    for (int q = 0; q < V; ++q)
#pragma unroll
      for (int i = 0; i < Term::SUMS; ++i) sums[i][at + q] = s[i][q];
  }
}
// VMAX = 4: V = 4 where `vec` (sample_vec4 of per, g and whatever else the Term loads V elements of), else V = 1; VMAX = 1: V = 1
template <int THREADS, int VMAX, int U, typename Term>
static int sample_accumulate(const char* who, bxStream stream, const float* g, bool vec, const Term& term, int n, int per, int Kc, int slot, int row0,
                             int rows) {
  const int b_first = row0 / n, b_count = (row0 + rows - 1) / n - b_first + 1;
  const int gy = b_count < 65535 ? b_count : 65535;
  double* const S0 = term.sum(0);
  double* const S1 = Term::SUMS > 1 ? term.sum(1) : nullptr;
  if (VMAX == 4 && vec)
    hipLaunchKernelGGL((k_sample_accumulate<THREADS, VMAX, U, Term>), dim3(bx_ceil_div(per / 4, THREADS), gy), dim3(THREADS), 0, (hipStream_t)stream, g, S0, S1,
                       term, n, per, Kc, slot, row0, rows, b_first, b_count);
  else
    hipLaunchKernelGGL((k_sample_accumulate<THREADS, 1, U, Term>), dim3(bx_ceil_div(per, THREADS), gy), dim3(THREADS), 0, (hipStream_t)stream, g, S0, S1, term, n,
                       per, Kc, slot, row0, rows, b_first, b_count);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- the noise rows -------------------------------------------------------------------------------------------------------------------
// row = fl32(x + fl32(scale[b] * z)), two separate fp32 roundings, z from the block of counter (q, k, b) under the key (k0, k1): a Draw
// is sg_normal4 or sg_uniform4.  A thread owns the four consecutive elements 4q .. 4q+3 of a row -- one Philox block -- and walks the
// rows of its workgroup row; every element of every row is written once, the noise lives in registers only.  V = 4: one 16-byte load
// and store (per % 4 == 0, aligned pointers); V = 1: element by element, the last block of a row may be partial.  x == nullptr: the
// row is z itself.
struct SampleNormal {
  static __device__ __forceinline__ void draw4(uint32_t q, uint32_t k, uint32_t b, uint32_t k0, uint32_t k1, float z[4]) { sg_normal4(q, k, b, k0, k1, z); }
};
struct SampleUniform {
  static __device__ __forceinline__ void draw4(uint32_t q, uint32_t k, uint32_t b, uint32_t k0, uint32_t k1, float z[4]) { sg_uniform4(q, k, b, k0, k1, z); }
};
template <int V, typename Draw>
__global__ __launch_bounds__(256) void k_sample_noise_rows(const float* __restrict__ x, const float* __restrict__ scale, float* __restrict__ out, int n, int per,
                                                           uint32_t k0, uint32_t k1, int row0, int rows) {
  const int q = blockIdx.x * 256 + threadIdx.x, e = q * 4;
  if (e >= per) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const int j = row0 + r, b = j / n, k = j - b * n;
    float z[4];
    Draw::draw4((uint32_t)q, (uint32_t)k, (uint32_t)b, k0, k1, z);
    float* o = out + (size_t)r * per + e;
    const float s = x ? scale[b] : 0.f;
    if (V == 4) {
      if (x) {
        float xv[4];
        ld4(x + (size_t)b * per + e, 0, xv);
        const float n0 = s * z[0], n1 = s * z[1], n2 = s * z[2], n3 = s * z[3];
        *reinterpret_cast<float4*>(o) = make_float4(xv[0] + n0, xv[1] + n1, xv[2] + n2, xv[3] + n3);
      } else {
        *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);
      }
    } else {
      const int m = per - e < 4 ? per - e : 4;
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
template <typename Draw>
static int sample_noise_rows(const char* who, bxStream stream, const float* x, const float* scale, float* out, int n, int per, uint64_t seed, int row0,
                             int rows) {
  const int gy = rows < 65535 ? rows : 65535, quads = bx_ceil_div(per, 4);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  if (sample_vec4(per, x, out))
    hipLaunchKernelGGL((k_sample_noise_rows<4, Draw>), dim3(bx_ceil_div(quads, 256), gy), dim3(256), 0, (hipStream_t)stream, x, scale, out, n, per, k0, k1, row0,
                       rows);
  else
    hipLaunchKernelGGL((k_sample_noise_rows<1, Draw>), dim3(bx_ceil_div(quads, 256), gy), dim3(256), 0, (hipStream_t)stream, x, scale, out, n, per, k0, k1, row0,
                       rows);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- the sum of a row -----------------------------------------------------------------------------------------------------------------
// One wave per row, whatever the launch: lane l adds v[r,t] (ABS: |v[r,t]|) for t = l, l + 64, ... in ascending t in fp64, the 64 lane
// sums are added by the xor butterfly (offsets 32, 16, .., 1: the same tree in every lane).  An fp64 out takes the sum; an fp32 out the
// mean, the quotient by L in fp64 and rounded to fp32 once.
__device__ __forceinline__ void sample_row_put(double* out, double s, int) { *out = s; }
__device__ __forceinline__ void sample_row_put(float* out, double s, int L) { *out = (float)(s / (double)L); }
template <bool ABS, typename Out>
__global__ __launch_bounds__(256) void k_sample_row_sum(const float* __restrict__ v, Out* __restrict__ out, int R, int L) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;                                          // wave-uniform
  const float* row = v + (size_t)r * L;
  double s = 0.0;
  for (int t = lane; t < L; t += 64) s += (double)(ABS ? fabsf(row[t]) : row[t]);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) sample_row_put(out + r, s, L);
}
template <bool ABS, typename Out>
static int sample_row_sum(const char* who, bxStream stream, const float* v, Out* out, int R, int L) {
  BX_REQUIRE(R > 0 && L > 0, "%s: bad shape R=%d L=%d", who, R, L);
  BX_REQUIRE((long long)R * L < (1ll << 31), "%s: R * L beyond 32-bit offsets", who);
  BX_REQUIRE(v && out, "%s: null pointer", who);
  BX_REQUIRE(sizeof(Out) < 8 || ((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
  hipLaunchKernelGGL((k_sample_row_sum<ABS, Out>), dim3(bx_ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, v, out, R, L);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
