// Blur Integrated Gradients (Xu, Venugopalan, Sundararajan, CVPR 2020; PAIR's saliency.BlurIG) and the Gaussian blur behind it: the rows
// X_i = blur_{sigma_i}(x) of every (sample, step) pair and the scale-space derivative D_i beside them, written in one launch by
// separable filters whose taps the host computes; the fp64 running sum of w_i * gradient * D_i in fixed step order and the fp64 row
// sums behind the completeness error (the walk and the wave row sum of sample_rows.h).  The forward and backward passes between rows
// and accumulate are the model's own kernels; the one-hot gradient seeds are bx_expgrad_seed and the finish is bx_expgrad_finish with
// n = 1.  See include/brainxai.h for the definition, the tap table and each entry point.
// The file is compiled with -ffp-contract=off: every filter step is an explicit fmaf in ascending tap order, and the accumulate's
// g * D (exact), w * (g * D) and the sum are separate fp64 roundings, so that a numpy restatement matches the sums bit for bit.
#include "sample_rows.h"

#define BI_THREADS 128
#define BI_LDS_LIMIT 65536

// ---- taps -------------------------------------------------------------------------------------------------------------------------------
// A filter's taps sit in LDS as s[TP + t], t = -TP .. TP-1, zero outside its radius; TP = 4 * ceil((RC + 3) / 4) + 4, RC = the largest
// radius of the table clipped to extent - 1 (a tap beyond that never joins two points of the image), is a multiple of
// four, so that the four taps t = 4k .. 4k+3 are one 16-byte read at the same address in every lane (a broadcast), for every k the
// loops below visit (|k| <= ceil((R + 3) / 4), and one chunk before the first).
__host__ __device__ __forceinline__ int bi_kr(int R) { return (R + 6) >> 2; }          // chunks of four on either side that hold a tap
__host__ __device__ __forceinline__ int bi_tp(int Rmax) { return 4 * bi_kr(Rmax) + 4; }

struct BiRow {
  int b, entry, Ra, Rb;
};
__host__ __device__ __forceinline__ BiRow bi_row(int j, int n, int per_sample, const int* __restrict__ radius, int Rmax) {
  BiRow r;
  r.b = j / n;
  r.entry = per_sample ? j : j - r.b * n;
  const int ra = radius[2 * r.entry], rb = radius[2 * r.entry + 1];
  r.Rb = rb < 0 ? 0 : (rb > Rmax ? Rmax : rb);
  r.Ra = ra < 0 ? 0 : (ra > r.Rb ? r.Rb : ra);
  return r;
}
// filter f of table entry `entry` (fp32 [entries,3,TW], tap t at TW / 2 + t) into s[0 .. 2 TP), zero outside |t| <= R
__host__ __device__ __forceinline__ void bi_stage_taps(const float* __restrict__ taps, int entry, int f, int TW, int R, int TP, float* s, int tid,
                                                       int threads) {
  const float* src = taps + ((size_t)entry * 3 + f) * TW + (TW >> 1);
  for (int u = tid; u < 2 * TP; u += threads) {
    const int t = u - TP;
    s[u] = (t >= -R && t <= R) ? src[t] : 0.f;
  }
}
__host__ __device__ __forceinline__ void bi_tap4(const float* s, int TP, int k, float w[4]) {
  const float4 v = *reinterpret_cast<const float4*>(s + TP + 4 * k);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}

// four consecutive elements 4q .. 4q+3 of a line of L, zero outside it; V = 4: L % 4 == 0 and the line is 16-byte aligned
template <int V>
__host__ __device__ __forceinline__ void bi_ld(const float* __restrict__ line, int q, int L, float v[4]) {
  if (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(line + (size_t)q * 4);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 4 * q + e < L ? line[4 * q + e] : 0.f;
  }
}
template <int V>
__host__ __device__ __forceinline__ void bi_st(float* __restrict__ line, int q, int L, const float v[4]) {
  if (V == 4) {
    *reinterpret_cast<float4*>(line + (size_t)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < L) line[4 * q + e] = v[e];
  }
}

// ---- a filter along a contiguous line ---------------------------------------------------------------------------------------------------
// The outputs 4i .. 4i+3 of a line of L elements (Q = ceil(L / 4) chunks): out_a = sum_t a[t] line[p + t] and, with D, out_d likewise
// with the taps d.  The loop walks the input chunks i + k that lie inside the line and can hold a tap, in ascending k; one loaded
// chunk feeds 16 fmaf per filter, and for every output the taps come in ascending t.  Taps outside the radius are zero in LDS.
template <int V, bool D>
__host__ __device__ __forceinline__ void bi_line4(const float* __restrict__ line, int L, int Q, int i, int KR, const float* sa, const float* sd, int TP, float oa[4],
                                         float od[4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o) oa[o] = od[o] = 0.f;
  const int k_lo = -i > -KR ? -i : -KR, k_hi = Q - 1 - i < KR ? Q - 1 - i : KR;
  float wa[8], wd[8];
  bi_tap4(sa, TP, k_lo - 1, wa + 4);
  if (D) bi_tap4(sd, TP, k_lo - 1, wd + 4);
  for (int k = k_lo; k <= k_hi; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { wa[e] = wa[4 + e]; if (D) wd[e] = wd[4 + e]; }
    bi_tap4(sa, TP, k, wa + 4);
    if (D) bi_tap4(sd, TP, k, wd + 4);
    float v[4];
    bi_ld<V>(line, i + k, L, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int o = 0; o < 4; ++o) {                                  // tap t = 4k + e - o
        oa[o] = fmaf(wa[4 + e - o], v[e], oa[o]);
        if (D) od[o] = fmaf(wd[4 + e - o], v[e], od[o]);
      }
  }
}

// ---- a filter across lines --------------------------------------------------------------------------------------------------------------
// The 4 x 4 outputs of rows 4yb .. 4yb+3 and columns 4cx .. 4cx+3: X = sum_t a[t] P[y + t] and, with D,
// Dv = sum_t ( b[t] Pd[y + t] + d[t] P[y + t] ), one accumulator, the b term before the d term of the same t.  src(y, which, v) reads
// the four columns of plane `which` (0: P, 1: Pd) at row y, zero beyond the last row.  TWO: Pd exists (two filtered axes); with one
// filtered axis the b term is absent.  One loaded row feeds 16 fmaf per filter.
template <bool D, bool TWO, class Src>
__host__ __device__ __forceinline__ void bi_cross4(Src src, int QH, int yb, int KR, const float* sa, const float* sb, const float* sd, int TP, float X[4][4],
                                          float Dv[4][4]) {
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int c = 0; c < 4; ++c) X[o][c] = Dv[o][c] = 0.f;
  const int k_lo = -yb > -KR ? -yb : -KR, k_hi = QH - 1 - yb < KR ? QH - 1 - yb : KR;
  float wa[8], wb[8], wd[8];
  bi_tap4(sa, TP, k_lo - 1, wa + 4);
  if (D) bi_tap4(sd, TP, k_lo - 1, wd + 4);
  if (D && TWO) bi_tap4(sb, TP, k_lo - 1, wb + 4);
  for (int k = k_lo; k <= k_hi; ++k) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { wa[e] = wa[4 + e]; if (D) wd[e] = wd[4 + e]; if (D && TWO) wb[e] = wb[4 + e]; }
    bi_tap4(sa, TP, k, wa + 4);
    if (D) bi_tap4(sd, TP, k, wd + 4);
    if (D && TWO) bi_tap4(sb, TP, k, wb + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float p[4], pd[4];
      src(4 * (yb + k) + e, 0, p);
      if (D && TWO) src(4 * (yb + k) + e, 1, pd);
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                // tap t = 4k + e - o
          X[o][c] = fmaf(wa[4 + e - o], p[c], X[o][c]);
          if (D && TWO) Dv[o][c] = fmaf(wb[4 + e - o], pd[c], Dv[o][c]);
          if (D) Dv[o][c] = fmaf(wd[4 + e - o], p[c], Dv[o][c]);
        }
    }
  }
}

// ---- rows, both axes --------------------------------------------------------------------------------------------------------------------
// A workgroup owns (row, channel, strip of SW columns).  It forms Ha = A_x x and Hd = D_x x of its strip for all H image rows into LDS
// (row stride SW + 4 floats: the 16-byte reads of the vertical pass then spread over the banks), runs the three vertical filters from
// LDS and writes X = A_y Ha and D = B_y Hd + D_y Ha.  No global intermediate.  LDS: [3 filters][2 TP] taps, then Ha and Hd [HP][SW + 4].
// The work of thread `tid` between two barriers is one phase of bi_hw_phase: 0 the identity row, 1 the taps, 2 the horizontal pass, 3 the
// vertical pass and the stores.
struct BiGeom {
  int n, C, H, W, SW, TW, RC, per_sample, row0;
};
template <int V, bool D>
__host__ __device__ __forceinline__ void bi_hw_phase(int phase, int tid, const BiGeom& g, const BiRow& row, const float* __restrict__ x,
                                                     const float* __restrict__ taps, float* __restrict__ rows_out, float* __restrict__ deriv_out, float* lds,
                                                     int strip, int c, int r) {
  const int TP = bi_tp(g.RC), H = g.H, W = g.W, HP = (H + 3) & ~3, RS = g.SW + 4, SQ = g.SW >> 2;
  float* sa = lds;
  float* sb = sa + 2 * TP;
  float* sd = sb + 2 * TP;
  float* Ha = sd + 2 * TP;
  float* Hd = Ha + (size_t)HP * RS;
  const int col0 = strip * g.SW, QW = (W + 3) >> 2, QH = HP >> 2;
  const size_t plane = (size_t)H * W;
  const float* xp = x + ((size_t)row.b * g.C + c) * plane;
  float* xo = rows_out + ((size_t)r * g.C + c) * plane;
  float* dout = D ? deriv_out + ((size_t)r * g.C + c) * plane : nullptr;
  const int Ra = row.Ra < g.RC ? row.Ra : g.RC, Rb = row.Rb < g.RC ? row.Rb : g.RC;      // a tap beyond extent - 1 never lands inside the image
  const int KR = bi_kr(Rb);
  if (phase == 0) {                                                  // the identity: x bit for bit, D = +0
    const int cols = W - col0 < g.SW ? W - col0 : g.SW;
    for (int u = tid; u < H * cols; u += BI_THREADS) {
      const size_t at = (size_t)(u / cols) * W + col0 + u % cols;
      xo[at] = xp[at];
      if (D) dout[at] = 0.f;
    }
  } else if (phase == 1) {
    bi_stage_taps(taps, row.entry, 0, g.TW, Ra, TP, sa, tid, BI_THREADS);
    if (D) bi_stage_taps(taps, row.entry, 1, g.TW, Rb, TP, sb, tid, BI_THREADS);
    if (D) bi_stage_taps(taps, row.entry, 2, g.TW, Rb, TP, sd, tid, BI_THREADS);
  } else if (phase == 2) {
    for (int task = tid; task < HP * SQ; task += BI_THREADS) {
      const int y = task / SQ, ci = task - y * SQ;
      float ha[4] = {0.f, 0.f, 0.f, 0.f}, hd[4] = {0.f, 0.f, 0.f, 0.f};
      if (y < H && col0 + 4 * ci < W) bi_line4<V, D>(xp + (size_t)y * W, W, QW, (col0 >> 2) + ci, KR, sa, sd, TP, ha, hd);
      bi_st<4>(Ha + (size_t)y * RS, ci, RS, ha);
      if (D) bi_st<4>(Hd + (size_t)y * RS, ci, RS, hd);
    }
  } else {
    for (int task = tid; task < QH * SQ; task += BI_THREADS) {
      const int yb = task / SQ, cx = task - yb * SQ;
      if (col0 + 4 * cx >= W) continue;
      auto src = [&](int y, int which, float v[4]) { bi_ld<4>((which ? Hd : Ha) + (size_t)y * RS, cx, RS, v); };
      float X[4][4], Dv[4][4];
      bi_cross4<D, true>(src, QH, yb, KR, sa, sb, sd, TP, X, Dv);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int y = 4 * yb + o;
        if (y < H) {
          bi_st<V>(xo + (size_t)y * W, (col0 >> 2) + cx, W, X[o]);
          if (D) bi_st<V>(dout + (size_t)y * W, (col0 >> 2) + cx, W, Dv[o]);
        }
      }
    }
  }
}
template <int V, bool D>
__global__ __launch_bounds__(BI_THREADS) void k_blur_rows_hw(const float* __restrict__ x, const float* __restrict__ taps, const int* __restrict__ radius,
                                                             float* __restrict__ rows_out, float* __restrict__ deriv_out, BiGeom g, int rows) {
  extern __shared__ __align__(16) float bi_lds[];
  for (int r = blockIdx.z; r < rows; r += gridDim.z) {
    const BiRow row = bi_row(g.row0 + r, g.n, g.per_sample, radius, g.TW >> 1);
    if (row.Rb == 0) {
      bi_hw_phase<V, D>(0, threadIdx.x, g, row, x, taps, rows_out, deriv_out, bi_lds, blockIdx.x, blockIdx.y, r);
      continue;
    }
    __syncthreads();                                                 // the previous row's vertical pass has read the LDS
    bi_hw_phase<V, D>(1, threadIdx.x, g, row, x, taps, rows_out, deriv_out, bi_lds, blockIdx.x, blockIdx.y, r);
    __syncthreads();
    bi_hw_phase<V, D>(2, threadIdx.x, g, row, x, taps, rows_out, deriv_out, bi_lds, blockIdx.x, blockIdx.y, r);
    __syncthreads();
    bi_hw_phase<V, D>(3, threadIdx.x, g, row, x, taps, rows_out, deriv_out, bi_lds, blockIdx.x, blockIdx.y, r);
  }
}

// ---- rows, one axis ---------------------------------------------------------------------------------------------------------------------
// No LDS intermediate.  ALONG_W: a thread owns four adjacent outputs of one image line (X = A x, D = D x along it); else a 4 x 4 block
// of outputs, filtered across the lines.  LDS: [2 filters][2 TP] taps.  Phases of bi_1d_phase: 0 the identity row, 1 the taps, 2 the
// filter and the stores of task `task`.
template <int V, bool D, bool ALONG_W>
__host__ __device__ __forceinline__ void bi_1d_phase(int phase, int tid, int task, const BiGeom& g, const BiRow& row, const float* __restrict__ x,
                                                     const float* __restrict__ taps, float* __restrict__ rows_out, float* __restrict__ deriv_out, float* lds,
                                                     int r) {
  const int TP = bi_tp(g.RC), H = g.H, W = g.W, QW = (W + 3) >> 2, QH = (H + 3) >> 2;
  float* sa = lds;
  float* sd = sa + 2 * TP;
  const size_t per = (size_t)g.C * H * W;
  const int tasks = ALONG_W ? g.C * H * QW : g.C * QH * QW;          // below 2^31: the launcher checks
  const float* xp = x + (size_t)row.b * per;
  float* xo = rows_out + (size_t)r * per;
  float* dout = D ? deriv_out + (size_t)r * per : nullptr;
  const int Ra = row.Ra < g.RC ? row.Ra : g.RC, Rb = row.Rb < g.RC ? row.Rb : g.RC;      // a tap beyond extent - 1 never lands inside the image
  if (phase == 1) {
    bi_stage_taps(taps, row.entry, 0, g.TW, Ra, TP, sa, tid, BI_THREADS);
    if (D) bi_stage_taps(taps, row.entry, 2, g.TW, Rb, TP, sd, tid, BI_THREADS);
    return;
  }
  if (task >= tasks) return;
  const int KR = bi_kr(Rb);
  if (ALONG_W) {
    const int line = task / QW, q = task - line * QW;
    float oa[4], od[4] = {0.f, 0.f, 0.f, 0.f};
    if (phase == 0) bi_ld<V>(xp + (size_t)line * W, q, W, oa);       // the identity: x bit for bit, D = +0
    else bi_line4<V, D>(xp + (size_t)line * W, W, QW, q, KR, sa, sd, TP, oa, od);
    bi_st<V>(xo + (size_t)line * W, q, W, oa);
    if (D) bi_st<V>(dout + (size_t)line * W, q, W, od);
  } else {
    const int cq = task / QW, q = task - cq * QW, ch = cq / QH, yb = cq - ch * QH;
    const float* pl = xp + (size_t)ch * H * W;
    auto src = [&](int y, int, float v[4]) {
      if (y < H) bi_ld<V>(pl + (size_t)y * W, q, W, v);
      else v[0] = v[1] = v[2] = v[3] = 0.f;
    };
    float X[4][4], Dv[4][4];
    if (phase == 0) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        src(4 * yb + o, 0, X[o]);
        Dv[o][0] = Dv[o][1] = Dv[o][2] = Dv[o][3] = 0.f;
      }
    } else {
      bi_cross4<D, false>(src, QH, yb, KR, sa, sa, sd, TP, X, Dv);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int y = 4 * yb + o;
      if (y < H) {
        bi_st<V>(xo + ((size_t)ch * H + y) * W, q, W, X[o]);
        if (D) bi_st<V>(dout + ((size_t)ch * H + y) * W, q, W, Dv[o]);
      }
    }
  }
}
template <int V, bool D, bool ALONG_W>
__global__ __launch_bounds__(BI_THREADS) void k_blur_rows_1d(const float* __restrict__ x, const float* __restrict__ taps, const int* __restrict__ radius,
                                                             float* __restrict__ rows_out, float* __restrict__ deriv_out, BiGeom g, int rows) {
  extern __shared__ __align__(16) float bi_lds[];
  const int task = blockIdx.x * BI_THREADS + threadIdx.x;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const BiRow row = bi_row(g.row0 + r, g.n, g.per_sample, radius, g.TW >> 1);
    if (row.Rb == 0) {
      bi_1d_phase<V, D, ALONG_W>(0, threadIdx.x, task, g, row, x, taps, rows_out, deriv_out, bi_lds, r);
      continue;
    }
    __syncthreads();                                                 // the previous row's filters have read the taps
    bi_1d_phase<V, D, ALONG_W>(1, threadIdx.x, task, g, row, x, taps, rows_out, deriv_out, bi_lds, r);
    __syncthreads();
    bi_1d_phase<V, D, ALONG_W>(2, threadIdx.x, task, g, row, x, taps, rows_out, deriv_out, bi_lds, r);
  }
}

// the widest strip of the two-axis kernel whose LDS fits: taps 3 * 2 TP floats, two planes of HP x (SW + 4) floats (one without D)
static int bi_strip(int H, int RC, bool deriv, size_t* lds) {
  const int TP = bi_tp(RC), HP = (H + 3) & ~3;
  for (int SW = 16; SW >= 4; SW >>= 1) {
    const size_t need = ((size_t)6 * TP + (size_t)(deriv ? 2 : 1) * HP * (SW + 4)) * sizeof(float);
    if (need <= BI_LDS_LIMIT) { *lds = need; return SW; }
  }
  return 0;
}

struct BiLaunch {
  const float* x; const float* taps; const int* radius; float* rows_out; float* deriv_out;
  BiGeom g;
  int rows, axes;
  size_t lds;
  hipStream_t stream;
};
template <int V, bool D>
static void bi_launch(const BiLaunch& a) {
  const int gr = a.rows < 65535 ? a.rows : 65535, QW = (a.g.W + 3) / 4, QH = (a.g.H + 3) / 4;
  if (a.axes == BX_BLUR_AXES_HW)
    hipLaunchKernelGGL((k_blur_rows_hw<V, D>), dim3(bx_ceil_div(a.g.W, a.g.SW), a.g.C, gr), dim3(BI_THREADS), a.lds, a.stream, a.x, a.taps, a.radius, a.rows_out,
                       a.deriv_out, a.g, a.rows);
  else if (a.axes == BX_BLUR_AXES_W)
    hipLaunchKernelGGL((k_blur_rows_1d<V, D, true>), dim3(bx_ceil_div((long long)a.g.C * a.g.H * QW, BI_THREADS), gr), dim3(BI_THREADS), a.lds, a.stream, a.x,
                       a.taps, a.radius, a.rows_out, a.deriv_out, a.g, a.rows);
  else
    hipLaunchKernelGGL((k_blur_rows_1d<V, D, false>), dim3(bx_ceil_div((long long)a.g.C * QH * QW, BI_THREADS), gr), dim3(BI_THREADS), a.lds, a.stream, a.x,
                       a.taps, a.radius, a.rows_out, a.deriv_out, a.g, a.rows);
}

extern "C" int bx_blur_rows(const float* x, const float* taps, const int* radius, float* rows_out, float* deriv_out, int B, int n, int C, int H, int W, int axes,
                            int tap_width, int per_sample, int row0, int rows, bxStream stream) {
  BX_REQUIRE(B > 0 && n > 0 && C > 0 && H > 0 && W > 0, "bx_blur_rows: bad shape B=%d n=%d C=%d H=%d W=%d", B, n, C, H, W);
  BX_REQUIRE(axes == BX_BLUR_AXES_HW || axes == BX_BLUR_AXES_H || axes == BX_BLUR_AXES_W, "bx_blur_rows: unknown axes %d", axes);
  BX_REQUIRE(tap_width >= 1 && (tap_width & 1), "bx_blur_rows: tap width %d is not an odd number >= 1", tap_width);
  const long long per = (long long)C * H * W;
  BX_REQUIRE((long long)B * n < (1ll << 31) && (long long)B * per < (1ll << 31), "bx_blur_rows: B * n or B * per beyond 32-bit offsets");
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= (long long)B * n, "bx_blur_rows: rows row0 = %d, rows = %d outside 0..B * n = %d", row0, rows,
             B * n);
  BX_REQUIRE((long long)rows * per < (1ll << 31), "bx_blur_rows: rows * per beyond 32-bit offsets");
  BX_REQUIRE((long long)(per_sample ? B * n : n) * 3 * tap_width < (1ll << 31), "bx_blur_rows: the tap table is beyond 32-bit offsets");
  if ((tap_width >> 1) > BX_BLUR_MAX_RADIUS)
    BX_FAIL(BX_EUNSUPPORTED, "bx_blur_rows: radius %d, supported 0..%d", tap_width >> 1, BX_BLUR_MAX_RADIUS);
  if (C > 65535) BX_FAIL(BX_EUNSUPPORTED, "bx_blur_rows: %d channels, supported 1..65535", C);
  const int ext = axes == BX_BLUR_AXES_HW ? (H > W ? H : W) : (axes == BX_BLUR_AXES_H ? H : W);
  const int RC = (tap_width >> 1) < ext - 1 ? (tap_width >> 1) : ext - 1;       // the taps that can land inside the image
  size_t lds = (size_t)4 * bi_tp(RC) * sizeof(float);
  if (lds > BI_LDS_LIMIT) BX_FAIL(BX_EUNSUPPORTED, "bx_blur_rows: %d taps on either side do not fit %d bytes of LDS", RC, BI_LDS_LIMIT);
  int SW = 0;
  if (axes == BX_BLUR_AXES_HW) {
    SW = bi_strip(H, RC, deriv_out != nullptr, &lds);
    if (!SW)
      BX_FAIL(BX_EUNSUPPORTED, "bx_blur_rows: H = %d rows with %d taps on either side: a 4-column strip of the intermediates does not fit %d bytes of LDS", H, RC,
              BI_LDS_LIMIT);
  }
  BX_REQUIRE(x && taps && radius && rows_out, "bx_blur_rows: null pointer");
  const bool v4 = sample_vec4(W, x, rows_out, deriv_out);
  const BiLaunch L = {x, taps, radius, rows_out, deriv_out, {n, C, H, W, SW, tap_width, RC, per_sample, row0}, rows, axes, lds, (hipStream_t)stream};
  if (v4 && deriv_out) bi_launch<4, true>(L);
  else if (v4) bi_launch<4, false>(L);
  else if (deriv_out) bi_launch<1, true>(L);
  else bi_launch<1, false>(L);
  BX_CHECK_LAUNCH("bx_blur_rows");
  return BX_OK;
}

// ---- the running sum: w[i] * (g * D).  g * D of two floats is exact in fp64; w[i] * (g * D) and the sum are one fp64 rounding each. ---------
struct BiTerm {
  const float* deriv; const double* w; double* acc;
  static constexpr int SUMS = 1;
  template <int V> struct Keep {};
  template <int V> struct Row { float d[V]; double w; };
  double* sum(int) const { return acc; }
  template <int V> __device__ __forceinline__ void sample(Keep<V>&, int, int, int) const {}
  template <int V> __device__ __forceinline__ void row(Row<V>& r, int, int i, int rr, int per, int e) const {
    sample_ld<V>(deriv + (size_t)rr * per + e, r.d);
    r.w = w[i];
  }
  template <int V> __device__ __forceinline__ void add(double (&s)[1][V], int q, const Keep<V>&, float g, const Row<V>& r) const {
    const double gd = (double)g * (double)r.d[q];
    const double term = r.w * gd;
    s[0][q] += term;
  }
};
extern "C" int bx_blurig_accumulate(const float* g, const float* deriv, const double* w, double* acc, int B, int n, int per, int Kc, int slot, int row0, int rows,
                                    bxStream stream) {
  const char* who = "bx_blurig_accumulate";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  SAMPLE_TRY(sample_slot_ok(who, B, per, Kc, slot));
  BX_REQUIRE(g && deriv && w && acc, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)acc | (uintptr_t)w) & 7) == 0, "%s: w and acc must be 8-byte aligned", who);
  return sample_accumulate<64, 4, 1>(who, stream, g, sample_vec4(per, g, deriv), BiTerm{deriv, w, acc}, n, per, Kc, slot, row0, rows);
}

// ---- the sum of a row: the wave row sum of sample_rows.h, in the order of bx_mean_abs_rows -----------------------------------------------
extern "C" int bx_blurig_sum_rows(const float* v, double* out, int R, int L, bxStream stream) {
  return sample_row_sum<false>("bx_blurig_sum_rows", stream, v, out, R, L);
}
