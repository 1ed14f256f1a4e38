// Guided Integrated Gradients (Kapishnikov et al., CVPR 2021; PAIR's saliency.GuidedIG): the adaptive path.  One workgroup owns one
// (sample, class) row for a whole step: it clamps the row to the step's window of the straight line, sums the distance left, finds the
// k-th smallest |gradient| among the cells that have not arrived by an exact radix select over the keys' bit patterns, moves the
// selected cells and adds (x - x_old) * g to the fp64 attribution -- as many passes as the step needs, without a word from the host.
// The forward and backward passes between steps are the model's own kernels; the one-hot seeds are bx_expgrad_seed and the finish is
// bx_expgrad_finish with n = 1.  See include/brainxai.h for the definition, the order of the sums and each entry point.
// A cell e is read and written by one thread only (e = t, t + GI_THREADS, ...), in every sweep of every pass, so the row needs no
// fence between sweeps; what the threads share goes through LDS: the sums' 16 wave totals, the 256 integer counters of a radix digit
// (integer adds: the counts do not depend on the order of arrival) and the select's running prefix.
// The file is compiled with -ffp-contract=off: alpha * d and base + (alpha * d), gamma * (X_max - x) and x + (..), (x - x_old) * g and
// the add to attr are separate fp64 roundings, so that a numpy restatement matches every bit.
#include "bx_common.h"

#define GI_THREADS 1024
#define GI_WAVES (GI_THREADS / 64)
#define GI_INF_BITS 0x7f800000u

// X(alpha) of one cell: fl32( base + alpha * (in - base) ) with the difference, the product and the sum in fp64; the ends bit for bit
__device__ __forceinline__ float gi_point(float base, float in, double alpha) {
  if (alpha >= 1.0) return in;
  if (alpha <= 0.0) return base;
  const double d = (double)in - (double)base;
  const double p = alpha * d;
  const double s = (double)base + p;
  return (float)s;
}
// step 2: where the cell's own alpha is below a_min it goes to X_min; a cell with in == base counts as a_max and never moves
__device__ __forceinline__ float gi_clamp(float x, float base, float in, double a_min, double a_max) {
  const double d = (double)in - (double)base;
  const double a = d == 0.0 ? a_max : ((double)x - (double)base) / d;
  return a < a_min ? gi_point(base, in, a_min) : x;
}
__device__ __forceinline__ uint32_t gi_key(float xc, float xmax, float g) { return xc == xmax ? GI_INF_BITS : (__float_as_uint(g) & 0x7fffffffu); }

// The sum of the block's 1024 partial sums, the same in every thread: inside a wave the xor butterfly (offsets 32, 16, .., 1: the same
// tree in every lane), then the 16 wave totals in ascending order.  red: 16 doubles of LDS.
__device__ __forceinline__ double gi_block_sum(double s, double* red) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();                                                   // the previous sum's readers are done with red
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = red[0];
  for (int w = 1; w < GI_WAVES; ++w) t += red[w];
  return t;
}

// A sweep over the row: f(e, in, base, x, g) for the thread's cells e = t, t + 1024, ... in ascending order (the order of the partial
// sums).  The loads of four cells are issued before the first of them is used: with one workgroup per row there are few waves to hide a
// load behind, and a sweep that waits for every cell's loads in turn is bound by their latency.
template <typename F>
__device__ __forceinline__ void gi_sweep(const float* __restrict__ in, const float* __restrict__ bs, const float* xr, const float* __restrict__ gr, int P, F f) {
  int e = threadIdx.x;
  for (; e + 3 * GI_THREADS < P; e += 4 * GI_THREADS) {
    float iv[4], bv[4], xv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      iv[u] = in[e + u * GI_THREADS]; bv[u] = bs[e + u * GI_THREADS]; xv[u] = xr[e + u * GI_THREADS]; gv[u] = gr[e + u * GI_THREADS];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) f(e + u * GI_THREADS, iv[u], bv[u], xv[u], gv[u]);
  }
  for (; e < P; e += GI_THREADS) f(e, in[e], bs[e], xr[e], gr[e]);
}

// One digit of the radix select: hist[0..256) counts the keys that share the prefix found so far by their next eight bits; the first
// wave finds the bin that holds rank kk and writes (prefix | bin << shift, kk - keys in the bins before it) to sel[0..2).
__device__ __forceinline__ void gi_pick_bin(const unsigned* hist, unsigned* sel, uint32_t prefix, unsigned kk, int shift) {
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    const unsigned c0 = hist[4 * l], c1 = hist[4 * l + 1], c2 = hist[4 * l + 2], c3 = hist[4 * l + 3];
    const unsigned tot = c0 + c1 + c2 + c3;
    unsigned incl = tot;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o, 64);
      if (l >= o) incl += up;
    }
    const unsigned excl = incl - tot;
    if (kk >= excl && kk < incl) {                                   // one lane: the counts add up to more than kk
      unsigned before = excl;
      int bin = 4 * l;
      if (kk >= before + c0) { before += c0; ++bin;
        if (kk >= before + c1) { before += c1; ++bin;
          if (kk >= before + c2) { before += c2; ++bin; } } }
      sel[0] = prefix | ((uint32_t)bin << shift);
      sel[1] = kk - before;
    }
  }
}

// ---- init: x = baseline, attr = 0, L_total, status = 0 --------------------------------------------------------------------------------
__global__ __launch_bounds__(GI_THREADS) void k_guided_ig_init(const float* __restrict__ x_in, const float* __restrict__ base, int base_rows, float* __restrict__ x,
                                                               double* __restrict__ attr, double* __restrict__ L_total, int* __restrict__ status, int Kc, int P,
                                                               int R) {
  __shared__ double red[GI_WAVES];
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = r / Kc;
    const float* in = x_in + (size_t)b * P;
    const float* bs = base_rows ? base + (size_t)b * P : nullptr;
    const float one = base_rows ? 0.f : base[0];
    double s = 0.0;
    for (int e = threadIdx.x; e < P; e += GI_THREADS) {
      const float bv = bs ? bs[e] : one;
      x[(size_t)r * P + e] = bv;
      attr[(size_t)r * P + e] = 0.0;
      s += fabs((double)in[e] - (double)bv);
    }
    const double tot = gi_block_sum(s, red);
    if (threadIdx.x == 0) { L_total[r] = tot; status[r] = 0; }
  }
}

extern "C" int bx_guided_ig_init(const float* x_in, const float* base, int base_rows, float* x, double* attr, double* L_total, int* status, int B, int Kc, int P,
                                 bxStream stream) {
  const char* who = "bx_guided_ig_init";
  BX_REQUIRE(B > 0 && Kc > 0 && P > 0, "%s: bad shape B=%d Kc=%d P=%d", who, B, Kc, P);
  const long long R = (long long)B * Kc;
  if (P >= (1 << 20)) BX_FAIL(BX_EUNSUPPORTED, "%s: rows of %d cells, supported 1..%d", who, P, (1 << 20) - 1);
  if (R > 65535) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld rows, supported 1..65535", who, R);
  if (R * P >= (1ll << 31)) BX_FAIL(BX_EUNSUPPORTED, "%s: R * P beyond 32-bit offsets", who);
  BX_REQUIRE(x_in && base && x && attr && L_total && status, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)attr | (uintptr_t)L_total) & 7) == 0, "%s: attr and L_total must be 8-byte aligned", who);
  hipLaunchKernelGGL(k_guided_ig_init, dim3((unsigned)R), dim3(GI_THREADS), 0, (hipStream_t)stream, x_in, base, base_rows, x, attr, L_total, status, Kc, P, (int)R);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- step -------------------------------------------------------------------------------------------------------------------------------
struct GiStep {
  double a_min, a_max, left;          // the window of the line and 1 - (i + 1) / n
  int Kc, P, i, n, k, cap, row0, rows;
};
__global__ __launch_bounds__(GI_THREADS) void k_guided_ig_step(const float* __restrict__ x_in, const float* __restrict__ x_base, float* __restrict__ x,
                                                               const float* __restrict__ g, double* __restrict__ attr, const double* __restrict__ L_total,
                                                               int* __restrict__ status, int* __restrict__ iters, GiStep s) {
  __shared__ double red[GI_WAVES];
  __shared__ unsigned hist[256];
  __shared__ unsigned sel[2];
  const int P = s.P, tid = threadIdx.x;
  for (int rr = blockIdx.x; rr < s.rows; rr += gridDim.x) {
    const int r = s.row0 + rr, b = r / s.Kc;
    const float* in = x_in + (size_t)b * P;
    const float* bs = x_base + (size_t)b * P;
    const float* gr = g + (size_t)rr * P;
    float* xr = x + (size_t)r * P;
    double* ar = attr + (size_t)r * P;
    const double Ltot = L_total[r];
    int passes = 0;
    if (status[r] == 0 && Ltot != 0.0) {                             // workgroup-uniform; a stopped row and a row at its baseline stay as they are
      const double Ltarget = Ltot * s.left;
      for (;;) {                                                     // at most cap passes
        ++passes;
        // sweep 1: the clamped row, the distance left, a NaN among the gradients, the first digit's counts
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        double part = 0.0;
        int nan = 0;
        gi_sweep(in, bs, xr, gr, P, [&](int, float iv, float bv, float xv, float gv) {
          const float xc = gi_clamp(xv, bv, iv, s.a_min, s.a_max);
          part += fabs((double)iv - (double)xc);
          nan |= gv != gv;
          const uint32_t key = gi_key(xc, gi_point(bv, iv, s.a_max), gv);
          atomicAdd(&hist[key >> 24], 1u);
        });
        if (__syncthreads_or(nan)) {                                 // nothing of the step has been written (a NaN shows in the first pass)
          if (tid == 0) status[r] = BX_GUIDED_NAN;
          passes = 0;
          break;
        }
        const double Lcur = gi_block_sum(part, red);
        const double diff = fabs(Ltarget - Lcur), big = fabs(Ltarget) > fabs(Lcur) ? fabs(Ltarget) : fabs(Lcur);
        const double rel = 1e-9 * big;
        const bool close = diff <= (rel > 1e-9 ? rel : 1e-9);
        uint32_t theta = 0u;
        double gamma = 0.0;
        bool more = false;
        if (!close) {
          // the k-th smallest key: four digits of eight bits, the first one counted above
          uint32_t prefix = 0u, mask = 0u;
          unsigned kk = (unsigned)s.k;
          for (int shift = 24; shift >= 0; shift -= 8) {
            if (shift != 24) {
              if (tid < 256) hist[tid] = 0u;
              __syncthreads();
              gi_sweep(in, bs, xr, gr, P, [&](int, float iv, float bv, float xv, float gv) {
                const uint32_t key = gi_key(gi_clamp(xv, bv, iv, s.a_min, s.a_max), gi_point(bv, iv, s.a_max), gv);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
              });
              __syncthreads();
            }
            gi_pick_bin(hist, sel, prefix, kk, shift);
            __syncthreads();
            prefix = sel[0];
            kk = sel[1];
            mask |= 255u << shift;
            __syncthreads();                                         // sel and hist are free again
          }
          theta = prefix;
          // sweep: the distance the selected cells have left
          double ps = 0.0;
          gi_sweep(in, bs, xr, gr, P, [&](int, float iv, float bv, float xv, float gv) {
            const float xc = gi_clamp(xv, bv, iv, s.a_min, s.a_max), xm = gi_point(bv, iv, s.a_max);
            const bool inS = xc != xm && gi_key(xc, xm, gv) <= theta;
            ps += inS ? fabs((double)xm - (double)xc) : 0.0;
          });
          const double LS = gi_block_sum(ps, red);
          gamma = LS > 0.0 ? (Lcur - Ltarget) / LS : (double)INFINITY;
          more = gamma > 1.0 && LS > 0.0;                            // L_S = 0: every cell has arrived, nothing is left to move
        }
        // last sweep: move the selected cells, add to the attribution, store the row
        gi_sweep(in, bs, xr, gr, P, [&](int e, float iv, float bv, float xo, float gv) {
          const float xc = gi_clamp(xo, bv, iv, s.a_min, s.a_max);
          float xn = xc;
          if (!close) {
            const float xm = gi_point(bv, iv, s.a_max);
            if (xc != xm && gi_key(xc, xm, gv) <= theta) {
              if (gamma > 1.0) {
                xn = xm;
              } else if (gamma > 0.0) {
                const double mv = gamma * ((double)xm - (double)xc);
                const double to = (double)xc + mv;
                xn = (float)to;
              }
            }
          }
          const double term = ((double)xn - (double)xo) * (double)gv;
          ar[e] += term;
          xr[e] = xn;
        });
        if (!more) break;
        if (passes >= s.cap) {
          if (tid == 0) status[r] = BX_GUIDED_CAP;
          break;
        }
      }
    }
    if (tid == 0) iters[(size_t)r * s.n + s.i] = passes;
    __syncthreads();
  }
}

extern "C" int bx_guided_ig_step(const float* x_in, const float* x_base, float* x, const float* g, double* attr, const double* L_total, int* status, int* iters,
                                 int B, int Kc, int P, int i, int n, int k, double max_dist, int cap, int row0, int rows, bxStream stream) {
  const char* who = "bx_guided_ig_step";
  BX_REQUIRE(B > 0 && Kc > 0 && P > 0, "%s: bad shape B=%d Kc=%d P=%d", who, B, Kc, P);
  BX_REQUIRE(n >= 1 && i >= 0 && i < n, "%s: step %d outside 0..n = %d", who, i, n);
  BX_REQUIRE(k >= 0 && k < P, "%s: rank k = %d outside 0..P = %d", who, k, P);
  BX_REQUIRE(max_dist >= 0.0 && max_dist <= 1.0, "%s: max_dist %g outside [0, 1]", who, max_dist);
  BX_REQUIRE(cap >= 1, "%s: cap = %d < 1", who, cap);
  const long long R = (long long)B * Kc;
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= R, "%s: rows row0 = %d, rows = %d outside 0..B * Kc = %lld", who, row0, rows, R);
  if (P >= (1 << 20)) BX_FAIL(BX_EUNSUPPORTED, "%s: rows of %d cells, supported 1..%d", who, P, (1 << 20) - 1);
  if (R > 65535) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld rows, supported 1..65535", who, R);
  if (R * P >= (1ll << 31) || R * n >= (1ll << 31)) BX_FAIL(BX_EUNSUPPORTED, "%s: R * P or R * n beyond 32-bit offsets", who);
  BX_REQUIRE(x_in && x_base && x && g && attr && L_total && status && iters, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)attr | (uintptr_t)L_total) & 7) == 0, "%s: attr and L_total must be 8-byte aligned", who);
  const double alpha = (double)(i + 1) / (double)n;
  GiStep s;
  s.a_min = alpha - max_dist > 0.0 ? alpha - max_dist : 0.0;
  s.a_max = alpha + max_dist < 1.0 ? alpha + max_dist : 1.0;
  s.left = 1.0 - alpha;
  s.Kc = Kc; s.P = P; s.i = i; s.n = n; s.k = k; s.cap = cap; s.row0 = row0; s.rows = rows;
  hipLaunchKernelGGL(k_guided_ig_step, dim3((unsigned)rows), dim3(GI_THREADS), 0, (hipStream_t)stream, x_in, x_base, x, g, attr, L_total, status, iters, s);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
