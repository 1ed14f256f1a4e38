// Optimised perturbation masks (Fong & Vedaldi, ICCV 2017: "meaningful perturbations"; the basis of TorchRay's extremal perturbations):
// per (sample, class) row a gh x gw grid m in [0, 1] is learned by Adam so that the input seen through its bilinear up-sampling,
// base + U(m) * (x - base), loses (deletion) or keeps (preservation) the class score with the smallest smooth region.  The model's
// forward and backward passes between the launches are its own kernels; what is here is everything around them: the rows, the fold of
// dF/dX back through the blend and the up-sampling onto the grid, the regularisers, the Adam step, the history and the status.
// See include/brainxai.h for the definition, the order of every sum and each entry point.
// No sum uses an atomic or depends on the launch geometry: a thread owns its outputs and adds its terms in ascending order, so the bits
// are a function of the inputs alone.  The step is two launches: k_maskopt_hsum (one workgroup per line of a row) forms t(p) and the
// horizontal footprint sums into the caller's fp64 scratch [rows,Hm,gw]; k_maskopt_update (one workgroup per row, one thread per grid cell) sums
// vertically and does the rest with the row's grid staged in LDS.
// Compiled with -ffp-contract=off (build.py): every product and every sum rounds on its own, so that a numpy restatement matches bit
// for bit.
#include <math.h>
#include "bx_common.h"

#define MO_MAX_G 32                    // grid cells per axis
#define MO_MAX_K 32
#define MO_MAX_HW ((1 << 20) - 1)      // cells of a mask domain: the map drops straight into deletion_insertion
#define MO_MAX_ROWS 65535
#define MO_CELLS (MO_MAX_G * MO_MAX_G) // threads of the update workgroup: one per grid cell

// The planes a mask value is shared by.  A spectrogram [C,H,W]: Cs = C planes of Hm x Wm = H x W.  An EEG input [1,Chans,T] with an
// electrode-by-time domain: one plane of Chans x T, and a kind-1 baseline holds one value per row y (by_row).  An EEG input with a [1,T]
// domain: the Chans electrodes are the planes of 1 x T.
struct MoGeom {
  int Cs, Hm, Wm, by_row, gh, gw;
  float sy, sx;                        // g / n: grid cells per pixel
};
static MoGeom mo_geom(int C, int H, int W, int map_rows, int gh, int gw) {
  MoGeom g;
  if (map_rows == 0) { g.Cs = C; g.Hm = H; g.by_row = 0; }
  else if (map_rows == H) { g.Cs = 1; g.Hm = H; g.by_row = 1; }
  else { g.Cs = H; g.Hm = 1; g.by_row = 0; }
  g.Wm = W; g.gh = gh; g.gw = gw;
  g.sy = (float)gh / (float)g.Hm;
  g.sx = (float)gw / (float)W;
  return g;
}

// pixel u of an axis of g cells -> the two source cells and the weight of the second: bx_common.h's bilinear_src (align_corners=False)
__device__ __forceinline__ int mo_i0(int u, float scale, int g) {
  int i0, i1; float l;
  bilinear_src(u, scale, g, i0, i1, l);
  return i0;
}
// Cell j's footprint [lo, hi) on an axis of n pixels: the pixels whose first source cell i0 is j - 1 or j (every pixel that can give
// cell j a weight).  i0 is non-decreasing in u, so the two ends are found exactly from an estimate by walking; every loop is bounded by n.
__device__ __forceinline__ void mo_footprint(int j, float scale, int g, int n, int& lo, int& hi) {
  const float inv = (float)n / (float)g;
  float fa = ((float)j - 0.5f) * inv - 0.5f, fb = ((float)j + 1.5f) * inv - 0.5f;
  int a = fa < 0.f ? 0 : (fa > (float)n ? n : (int)fa);
  while (a > 0 && mo_i0(a - 1, scale, g) >= j - 1) --a;
  while (a < n && mo_i0(a, scale, g) < j - 1) ++a;
  int b = fb < (float)a ? a : (fb > (float)n ? n : (int)fb);
  while (b < n && mo_i0(b, scale, g) <= j) ++b;
  while (b > a && mo_i0(b - 1, scale, g) > j) --b;
  lo = a; hi = b;
}
// the weight pixel (i0, i1, l) gives cell j: the forward's fp32 weights 1 - l and l, widened exactly
__device__ __forceinline__ double mo_weight(int j, int i0, int i1, float l) {
  const float l0 = 1.f - l;
  return (j == i0 ? (double)l0 : 0.0) + (j == i1 ? (double)l : 0.0);
}
// horizontal blend first, then vertical; m = the row's grid [gh,gw]
__device__ __forceinline__ float mo_value(const float* __restrict__ m, int gw, int y0, int y1, float ly, int x0, int x1, float lx) {
  const float a = m[y0 * gw + x0], b = m[y0 * gw + x1], c = m[y1 * gw + x0], d = m[y1 * gw + x1];
  const float top = (1.f - lx) * a + lx * b, bot = (1.f - lx) * c + lx * d;
  return (1.f - ly) * top + ly * bot;
}
// the fp32 exponential, correctly rounded: the fp64 exponential rounded once (a restatement gets the same bits from any accurate exp)
__device__ __forceinline__ float mo_expf(float y) { return (float)exp((double)y); }

static inline bool mo_vec4(int W, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return W % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
}

// ---- host checks, worded with the entry point's name ---------------------------------------------------------------------------------------
static int mo_grid_ok(const char* who, int Hm, int Wm, int gh, int gw) {
  BX_REQUIRE(Hm > 0 && Wm > 0, "%s: bad shape Hm=%d Wm=%d", who, Hm, Wm);
  if ((long long)Hm * Wm > MO_MAX_HW) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld cells per mask, supported 1..%d", who, (long long)Hm * Wm, MO_MAX_HW);
  BX_REQUIRE(gh >= 1 && gw >= 1, "%s: grid %d x %d", who, gh, gw);
  if (gh > MO_MAX_G || gw > MO_MAX_G || gh > Hm || gw > Wm)
    BX_FAIL(BX_EUNSUPPORTED, "%s: grid %d x %d, supported 1..min(%d, Hm = %d) x 1..min(%d, Wm = %d)", who, gh, gw, MO_MAX_G, Hm, MO_MAX_G, Wm);
  return BX_OK;
}
static int mo_window_ok(const char* who, int B, int Kc, int row0, int rows) {
  BX_REQUIRE(B > 0 && Kc > 0, "%s: bad shape B=%d Kc=%d", who, B, Kc);
  const long long R = (long long)B * Kc;
  if (R > MO_MAX_ROWS) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld rows, supported 1..%d", who, R, MO_MAX_ROWS);
  BX_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= R, "%s: rows row0 = %d, rows = %d outside 0..B * Kc = %lld", who, row0, rows, R);
  return BX_OK;
}
static int mo_input_ok(const char* who, int C, int H, int W, int map_rows, int baseline_kind) {
  BX_REQUIRE(C > 0 && H > 0 && W > 0, "%s: bad shape C=%d H=%d W=%d", who, C, H, W);
  BX_REQUIRE(map_rows == 0 || (C == 1 && (map_rows == H || map_rows == 1)), "%s: map_rows = %d (0 for a spectrogram; Chans = %d or 1 for an EEG input, C = 1)", who,
             map_rows, H);
  BX_REQUIRE(baseline_kind >= 0 && baseline_kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel / electrode, 2 full tensor)", who, baseline_kind);
  return BX_OK;
}
#define MO_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// ---- init: m = 1, the moments 0, status OK -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maskopt_init(float* __restrict__ m, double* __restrict__ mu, double* __restrict__ nu, int* __restrict__ status, int G,
                                                      int row0, int rows) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * G) return;
  const int at = row0 * G + idx;
  m[at] = 1.f; mu[at] = 0.0; nu[at] = 0.0;
  if (idx % G == 0) status[row0 + idx / G] = BX_MASKOPT_OK;
}
extern "C" int bx_maskopt_init(float* m, double* mu, double* nu, int* status, int B, int Kc, int gh, int gw, int row0, int rows, bxStream stream) {
  const char* who = "bx_maskopt_init";
  MO_TRY(mo_window_ok(who, B, Kc, row0, rows));
  BX_REQUIRE(gh >= 1 && gw >= 1, "%s: grid %d x %d", who, gh, gw);
  if (gh > MO_MAX_G || gw > MO_MAX_G) BX_FAIL(BX_EUNSUPPORTED, "%s: grid %d x %d, supported 1..%d x 1..%d", who, gh, gw, MO_MAX_G, MO_MAX_G);
  BX_REQUIRE(m && mu && nu && status, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)mu | (uintptr_t)nu) & 7) == 0, "%s: mu and nu must be 8-byte aligned", who);
  const int G = gh * gw;
  hipLaunchKernelGGL(k_maskopt_init, dim3(bx_ceil_div((long long)rows * G, 256)), dim3(256), 0, (hipStream_t)stream, m, mu, nu, status, G, row0, rows);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- the up-sampled masks and the rows -----------------------------------------------------------------------------------------------------
// A thread owns V adjacent pixels of one line y of one row: V = 4 where every line starts 16-byte aligned (one 16-byte load and store
// per plane), V = 1 element by element.  The four grid values of a pixel come from the row's grid in global memory (at most 4 KiB a row,
// read by every thread of the row: it stays in the vector cache).
template <int V>
__device__ __forceinline__ void mo_line(const float* __restrict__ mr, const MoGeom& g, int y, int x, float (&M)[V]) {
  int y0, y1; float ly;
  bilinear_src(y, g.sy, g.gh, y0, y1, ly);
#pragma unroll
  for (int q = 0; q < V; ++q) {
    int x0, x1; float lx;
    bilinear_src(x + q, g.sx, g.gw, x0, x1, lx);
    M[q] = mo_value(mr, g.gw, y0, y1, ly, x0, x1, lx);
  }
}
template <int V>
__global__ __launch_bounds__(256) void k_maskopt_masks(const float* __restrict__ m, float* __restrict__ out, MoGeom g, int row0, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int WQ = g.Wm / V, xq = idx % WQ, line = idx / WQ, y = line % g.Hm, rr = line / g.Hm;
  float M[V];
  mo_line<V>(m + (size_t)(row0 + rr) * g.gh * g.gw, g, y, xq * V, M);
  float* o = out + (size_t)line * g.Wm + xq * V;
  if (V == 4) *reinterpret_cast<float4*>(o) = make_float4(M[0], M[1], M[2], M[3]);
  else o[0] = M[0];
}
extern "C" int bx_maskopt_masks(const float* m, float* out, int B, int Kc, int gh, int gw, int Hm, int Wm, int row0, int rows, bxStream stream) {
  const char* who = "bx_maskopt_masks";
  MO_TRY(mo_grid_ok(who, Hm, Wm, gh, gw));
  MO_TRY(mo_window_ok(who, B, Kc, row0, rows));
  BX_REQUIRE((long long)rows * Hm * Wm < (1ll << 31), "%s: rows * Hm * Wm beyond 32-bit offsets; use a smaller window", who);
  BX_REQUIRE(m && out, "%s: null pointer", who);
  const MoGeom g = mo_geom(1, Hm, Wm, 0, gh, gw);
  if (mo_vec4(Wm, out)) {
    const int total = rows * Hm * (Wm / 4);
    hipLaunchKernelGGL(k_maskopt_masks<4>, dim3(bx_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, m, out, g, row0, total);
  } else {
    const int total = rows * Hm * Wm;
    hipLaunchKernelGGL(k_maskopt_masks<1>, dim3(bx_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, m, out, g, row0, total);
  }
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// the baseline of plane c, line y, element `at` of the sample (at = (c * Hm + y) * Wm + x), by kind
template <int V>
__device__ __forceinline__ void mo_base(const float* __restrict__ base, int kind, const MoGeom& g, size_t sample, int c, int y, int at, float (&bv)[V]) {
  if (kind == 2) {
    if (V == 4) ld4(base + sample, at, bv); else bv[0] = base[sample + at];
  } else {
    const float v = kind == 0 ? base[0] : base[g.by_row ? y : c];
#pragma unroll
    for (int q = 0; q < V; ++q) bv[q] = v;
  }
}
// out[rr,c,y,x] = base + M * (x - base): three fp32 roundings, M shared by the Cs planes
template <int V>
__global__ __launch_bounds__(256) void k_maskopt_rows(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ base, int kind,
                                                      float* __restrict__ out, MoGeom g, int Kc, int row0, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int WQ = g.Wm / V, xq = idx % WQ, line = idx / WQ, y = line % g.Hm, rr = line / g.Hm;
  const int r = row0 + rr, b = r / Kc, per = g.Cs * g.Hm * g.Wm;
  float M[V];
  mo_line<V>(m + (size_t)r * g.gh * g.gw, g, y, xq * V, M);
  for (int c = 0; c < g.Cs; ++c) {
    const int at = (c * g.Hm + y) * g.Wm + xq * V;
    float xv[V], bv[V], ov[V];
    if (V == 4) ld4(x + (size_t)b * per, at, xv); else xv[0] = x[(size_t)b * per + at];
    mo_base<V>(base, kind, g, (size_t)b * per, c, y, at, bv);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const float d = xv[q] - bv[q];
      const float p = M[q] * d;
      ov[q] = bv[q] + p;
    }
    float* o = out + (size_t)rr * per + at;
    if (V == 4) *reinterpret_cast<float4*>(o) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    else o[0] = ov[0];
  }
}
static int mo_rows(const char* who, const float* x, const float* m, const float* baseline, int baseline_kind, float* out, int B, int Kc, int C, int H, int W,
                   int map_rows, int gh, int gw, int row0, int rows, bxStream stream) {
  MO_TRY(mo_input_ok(who, C, H, W, map_rows, baseline_kind));
  const MoGeom g = mo_geom(C, H, W, map_rows, gh, gw);
  MO_TRY(mo_grid_ok(who, g.Hm, g.Wm, gh, gw));
  MO_TRY(mo_window_ok(who, B, Kc, row0, rows));
  const long long per = (long long)C * H * W;
  BX_REQUIRE((long long)B * per < (1ll << 31) && (long long)rows * per < (1ll << 31), "%s: B * per or rows * per beyond 32-bit offsets; use a smaller window", who);
  BX_REQUIRE(x && m && baseline && out, "%s: null pointer", who);
  if (mo_vec4(W, x, out, baseline_kind == 2 ? baseline : nullptr)) {
    const int total = rows * g.Hm * (W / 4);
    hipLaunchKernelGGL(k_maskopt_rows<4>, dim3(bx_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, m, baseline, baseline_kind, out, g, Kc, row0, total);
  } else {
    const int total = rows * g.Hm * W;
    hipLaunchKernelGGL(k_maskopt_rows<1>, dim3(bx_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, m, baseline, baseline_kind, out, g, Kc, row0, total);
  }
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
extern "C" int bx_maskopt_rows_spec(const float* x, const float* m, const float* baseline, int baseline_kind, float* out, int B, int Kc, int C, int H, int W,
                                    int gh, int gw, int row0, int rows, bxStream stream) {
  return mo_rows("bx_maskopt_rows_spec", x, m, baseline, baseline_kind, out, B, Kc, C, H, W, 0, gh, gw, row0, rows, stream);
}
extern "C" int bx_maskopt_rows_eeg(const float* x, const float* m, int map_rows, const float* baseline, int baseline_kind, float* out, int B, int Kc, int Chans,
                                   int T, int gh, int gw, int row0, int rows, bxStream stream) {
  const char* who = "bx_maskopt_rows_eeg";
  BX_REQUIRE(Chans > 0 && T > 0 && (map_rows == Chans || map_rows == 1), "%s: bad shape Chans=%d T=%d map_rows=%d (Chans or 1)", who, Chans, T, map_rows);
  return mo_rows(who, x, m, baseline, baseline_kind, out, B, Kc, 1, Chans, T, map_rows, gh, gw, row0, rows, stream);
}

// ---- the step, first launch: t(p) and the horizontal footprint sums ------------------------------------------------------------------------
// One workgroup per line (rr, y).  The line is walked in tiles of MO_TILE pixels: all threads form t(y,x) = SUM_c (double)g *
// (double)fl32(x - base), in plane order, for the tile's pixels into LDS -- adjacent threads read adjacent pixels, V = 4 pixels per 16-byte
// load where every line starts 16-byte aligned, V = 1 otherwise --, then thread j < gw adds wx(x,j) * t(y,x) for the pixels of cell j's
// footprint inside the tile in ascending x to the sum it carries from tile to tile: hs[rr,y,j], with the adds in the definition's order.
// (A thread per (rr, y, j) that loaded its own footprint walked 2 Wm / gw pixels through dependent global loads: 87 us per launch at
// B = 64 for either benchmark shape, most of the step; DESIGN.md section 6 "Mask optimisation".)
#define MO_TILE 2048
#define MO_HSUM_THREADS 128
struct MoHsum {
  const float* x; const float* base; const float* g;
  int kind, Kc, row0;
};
template <int V>
__global__ __launch_bounds__(MO_HSUM_THREADS) void k_maskopt_hsum(MoHsum a, double* __restrict__ hs, MoGeom g) {
  __shared__ double t[MO_TILE];
  const int line = blockIdx.x, y = line % g.Hm, rr = line / g.Hm, j = threadIdx.x;
  const int b = (a.row0 + rr) / a.Kc, plane = g.Hm * g.Wm, per = g.Cs * plane;
  const float* __restrict__ xs = a.x + (size_t)b * per;
  const float* __restrict__ gr = a.g + (size_t)rr * per;
  int lo = 0, hi = 0;
  if (j < g.gw) mo_footprint(j, g.sx, g.gw, g.Wm, lo, hi);
  double acc = 0.0;
  for (int x0 = 0; x0 < g.Wm; x0 += MO_TILE) {
    const int x1 = x0 + MO_TILE < g.Wm ? x0 + MO_TILE : g.Wm;
    for (int x = x0 + (int)threadIdx.x * V; x < x1; x += MO_HSUM_THREADS * V) {
      double tv[V];
#pragma unroll
      for (int q = 0; q < V; ++q) tv[q] = 0.0;
      for (int c = 0; c < g.Cs; ++c) {
        const int at = c * plane + y * g.Wm + x;
        float gv[V], xv[V], bv[V];
        if (V == 4) { ld4(gr, at, gv); ld4(xs, at, xv); } else { gv[0] = gr[at]; xv[0] = xs[at]; }
        mo_base<V>(a.base, a.kind, g, (size_t)b * per, c, y, at, bv);
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const float d = xv[q] - bv[q];
          const double p = (double)gv[q] * (double)d;
          tv[q] += p;
        }
      }
#pragma unroll
      for (int q = 0; q < V; ++q) t[x - x0 + q] = tv[q];
    }
    __syncthreads();
    const int from = lo > x0 ? lo : x0, to = hi < x1 ? hi : x1;
    for (int x = from; x < to; ++x) {
      int i0, i1; float l;
      bilinear_src(x, g.sx, g.gw, i0, i1, l);
      const double p = mo_weight(j, i0, i1, l) * t[x - x0];
      acc += p;
    }
    __syncthreads();                                                 // the tile is free again
  }
  if (j < g.gw) hs[(size_t)line * g.gw + j] = acc;
}

// ---- the step, second launch: vertical sums, regularisers, Adam, history, status -------------------------------------------------------------
struct MoStep {
  double lr, l1n, tv, b1, b2, omb1, omb2, eps, c1, c2;     // l1n = l1 / (gh gw), omb = 1 - b
  int Kc, K, mode, score, beta, it, n, row0, Hm, gh, gw;
  float sy;
};
// |d|^beta and its derivative beta d |d|^(beta - 2) (sign(d) for beta = 1, 0 at d = 0): products, no pow
__device__ __forceinline__ double mo_tv_term(double d, int beta) {
  const double a = fabs(d);
  return beta == 1 ? a : (beta == 2 ? a * a : (a * a) * a);
}
__device__ __forceinline__ double mo_tv_grad(double d, int beta) {
  if (beta == 1) return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  if (beta == 2) return 2.0 * d;
  return (3.0 * d) * fabs(d);
}
__global__ __launch_bounds__(MO_CELLS) void k_maskopt_update(const double* __restrict__ hs, const float* __restrict__ y, const int* __restrict__ classes,
                                                             float* __restrict__ m, double* __restrict__ mu, double* __restrict__ nu, int* __restrict__ status,
                                                             double* __restrict__ history, double* __restrict__ G_out, MoStep s) {
  __shared__ float sm[MO_CELLS];
  const int rr = blockIdx.x, r = s.row0 + rr, e = threadIdx.x, gw = s.gw, gh = s.gh, G = gh * gw;
  if (status[r] != BX_MASKOPT_OK) return;                            // workgroup-uniform: a stopped row stays as it is
  int cls = classes[r];
  cls = cls < 0 ? 0 : (cls >= s.K ? s.K - 1 : cls);
  const float yv = y[(size_t)rr * s.K + cls];
  const int i = e / gw, j = e - i * gw;
  double Gd = 0.0;
  if (e < G) {
    sm[e] = m[(size_t)r * G + e];
    int lo, hi;
    mo_footprint(i, s.sy, gh, s.Hm, lo, hi);
    double acc = 0.0;
    for (int yy = lo; yy < hi; ++yy) {
      int i0, i1; float l;
      bilinear_src(yy, s.sy, gh, i0, i1, l);
      const double p = mo_weight(i, i0, i1, l) * hs[((size_t)rr * s.Hm + yy) * gw + j];
      acc += p;
    }
    const double wr = s.score == 0 ? (double)mo_expf(yv) : 1.0;      // the chain rule of the probability
    Gd = wr * acc;
    if (s.mode == 1) Gd = -Gd;
  }
  if (__syncthreads_or((Gd != Gd) | (yv != yv))) {                   // nothing of the step has been written; also the barrier behind sm
    if (e == 0) status[r] = BX_MASKOPT_NAN;
    return;
  }
  if (e < 64) {                                                      // history, before the update: lane-strided fp64 sums, xor butterfly
    double s1 = 0.0, s2 = 0.0;
    for (int t = e; t < G; t += 64) {
      const int ti = t / gw, tj = t - ti * gw;
      const double v = (double)sm[t];
      s1 += v;
      double term = 0.0;
      if (tj + 1 < gw) term += mo_tv_term((double)sm[t + 1] - v, s.beta);
      if (ti + 1 < gh) term += mo_tv_term((double)sm[t + gw] - v, s.beta);
      s2 += term;
    }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    if (e == 0) {
      double* h = history + ((size_t)r * s.n + s.it) * 3;
      h[0] = s.score == 0 ? (double)mo_expf(yv) : (double)yv;
      h[1] = s1 / (double)G;
      h[2] = s2;
    }
  }
  if (e >= G) return;
  const double v = (double)sm[e];
  double dtv = 0.0;
  if (j > 0) dtv += mo_tv_grad(v - (double)sm[e - 1], s.beta);
  if (j + 1 < gw) dtv -= mo_tv_grad((double)sm[e + 1] - v, s.beta);
  if (i > 0) dtv += mo_tv_grad(v - (double)sm[e - gw], s.beta);
  if (i + 1 < gh) dtv -= mo_tv_grad((double)sm[e + gw] - v, s.beta);
  const double reg = s.tv * dtv;
  const double Gl = s.mode == 0 ? Gd - s.l1n : Gd + s.l1n;
  const double Gt = Gl + reg;
  const size_t at = (size_t)r * G + e;
  if (G_out) G_out[at] = Gt;
  const double m1 = s.b1 * mu[at], m2 = s.omb1 * Gt;
  const double mun = m1 + m2;
  const double n1 = s.b2 * nu[at], n2 = (s.omb2 * Gt) * Gt;
  const double nun = n1 + n2;
  const double num = s.lr * (mun / s.c1), den = sqrt(nun / s.c2) + s.eps;
  const double to = v - num / den;
  const float mn = (float)to;
  mu[at] = mun; nu[at] = nun;
  m[at] = mn < 0.f ? 0.f : (mn > 1.f ? 1.f : mn);
}

extern "C" int bx_maskopt_step(const float* x, const float* baseline, int baseline_kind, const float* g, const float* y, const int* classes, float* m, double* mu,
                               double* nu, int* status, double* history, double* G_out, double* scratch, int B, int Kc, int C, int H, int W, int map_rows, int K,
                               int gh, int gw, int mode, int score, int tv_beta, double lr, double l1, double tv, double b1, double b2, double eps, double c1,
                               double c2, int it, int iterations, int row0, int rows, bxStream stream) {
  const char* who = "bx_maskopt_step";
  MO_TRY(mo_input_ok(who, C, H, W, map_rows, baseline_kind));
  const MoGeom geo = mo_geom(C, H, W, map_rows, gh, gw);
  MO_TRY(mo_grid_ok(who, geo.Hm, geo.Wm, gh, gw));
  MO_TRY(mo_window_ok(who, B, Kc, row0, rows));
  BX_REQUIRE(K >= 1, "%s: bad shape K=%d", who, K);
  if (K > MO_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, K, MO_MAX_K);
  BX_REQUIRE(mode == BX_MASKOPT_DELETION || mode == BX_MASKOPT_PRESERVATION, "%s: mode %d (0 deletion, 1 preservation)", who, mode);
  BX_REQUIRE(score == BX_MASKOPT_PROB || score == BX_MASKOPT_LOGPROB, "%s: score %d (0 prob, 1 logprob)", who, score);
  BX_REQUIRE(tv_beta >= 1 && tv_beta <= 3, "%s: tv_beta = %d outside 1..3", who, tv_beta);
  BX_REQUIRE(lr >= 0.0 && l1 >= 0.0 && tv >= 0.0 && eps >= 0.0, "%s: lr = %g, l1 = %g, tv = %g, eps = %g must be >= 0", who, lr, l1, tv, eps);
  BX_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "%s: betas (%g, %g) outside [0, 1)", who, b1, b2);
  BX_REQUIRE(c1 > 0.0 && c1 <= 1.0 && c2 > 0.0 && c2 <= 1.0, "%s: bias corrections c1 = %g, c2 = %g outside (0, 1]", who, c1, c2);
  BX_REQUIRE(iterations >= 1 && it >= 0 && it < iterations, "%s: iteration %d outside 0..iterations = %d", who, it, iterations);
  const long long R = (long long)B * Kc, per = (long long)C * H * W;
  if (B * per >= (1ll << 31) || rows * per >= (1ll << 31) || R * iterations * 3 >= (1ll << 31) || (long long)rows * geo.Hm * gw >= (1ll << 31))
    BX_FAIL(BX_EUNSUPPORTED, "%s: B * per, rows * per, R * iterations * 3 or rows * Hm * gw beyond 32-bit offsets", who);
  BX_REQUIRE(x && baseline && g && y && classes && m && mu && nu && status && history && scratch, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)mu | (uintptr_t)nu | (uintptr_t)history | (uintptr_t)G_out | (uintptr_t)scratch) & 7) == 0,
             "%s: mu, nu, history, G_out and scratch must be 8-byte aligned", who);
  const MoHsum a = {x, baseline, g, baseline_kind, Kc, row0};
  const int lines = rows * geo.Hm;
  if (mo_vec4(W, x, g, baseline_kind == 2 ? baseline : nullptr))
    hipLaunchKernelGGL(k_maskopt_hsum<4>, dim3(lines), dim3(MO_HSUM_THREADS), 0, (hipStream_t)stream, a, scratch, geo);
  else
    hipLaunchKernelGGL(k_maskopt_hsum<1>, dim3(lines), dim3(MO_HSUM_THREADS), 0, (hipStream_t)stream, a, scratch, geo);
  BX_CHECK_LAUNCH(who);
  MoStep s;
  s.lr = lr; s.l1n = l1 / (double)(gh * gw); s.tv = tv; s.b1 = b1; s.b2 = b2; s.omb1 = 1.0 - b1; s.omb2 = 1.0 - b2; s.eps = eps; s.c1 = c1; s.c2 = c2;
  s.Kc = Kc; s.K = K; s.mode = mode; s.score = score; s.beta = tv_beta; s.it = it; s.n = iterations; s.row0 = row0; s.Hm = geo.Hm; s.gh = gh; s.gw = gw;
  s.sy = geo.sy;
  hipLaunchKernelGGL(k_maskopt_update, dim3((unsigned)rows), dim3(bx_ceil_div(gh * gw, 64) * 64), 0, (hipStream_t)stream, scratch, y, classes, m, mu, nu, status, history, G_out, s);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
