// Similarity of two attribution maps and the re-initialiser of the model parameter randomization test (Adebayo et al., "Sanity Checks
// for Saliency Maps", NeurIPS 2018; Ghorbani et al., AAAI 2019): tie-averaged ranks behind Spearman's correlation, the fp64 two-pass
// Pearson correlation, the overlap of the top-k cells, a row's extremes, the mean windowed SSIM of scikit-image's structural_similarity
// and uniform draws for Conv2d / Linear parameters.  The stable ranks are bx_rank_desc's (faith.hip).  See include/brainxai.h for the
// definitions and each entry point.
// The file is compiled with -ffp-contract=off: the draws fl32(bound * u) match a numpy restatement bit for bit, and every fp64
// product and sum of the correlations and of SSIM rounds on its own, in an order that depends on the shapes alone.  No atomics.
#include "bx_philox.h"

#define SIM_MAX_N ((1 << 20) - 1)       // cells of a map, the limit of bx_rank_desc
#define SIM_LDS_LIMIT 65536
#define SIM_HEAD 72                     // doubles in front of the moment planes: BX_SSIM_MAX_WIN taps (64 slots) and the four wave sums (8 slots)
#define SIM_PLANE_CELLS ((SIM_LDS_LIMIT - SIM_HEAD * 8) / 40)       // cells (image rows x strip columns) of the five fp64 planes: 1624

static int sim_rows_ok(const char* who, int R, int N) {
  BX_REQUIRE(R > 0 && N > 0, "%s: bad shape R=%d N=%d", who, R, N);
  if (N > SIM_MAX_N) BX_FAIL(BX_EUNSUPPORTED, "%s: N = %d cells per row, supported 1..%d", who, N, SIM_MAX_N);
  BX_REQUIRE((long long)R * N < (1ll << 31), "%s: R * N = %lld beyond 32-bit offsets", who, (long long)R * N);
  return BX_OK;
}
#define SIM_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

__device__ __forceinline__ uint32_t sim_key(float v, int abs) { return bx_rank_key(abs ? fabsf(v) : v); }
__device__ __forceinline__ double sim_wave_sum(double s) {             // the xor butterfly of sample_rows.h: the same tree in every lane
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// ---- tie-averaged ranks -------------------------------------------------------------------------------------------------------------------
// sorted[r, ranks[r,i]] = key(values[r,i]): the keys of a row in ascending order, since ranks is the stable descending sort position.
__global__ __launch_bounds__(256) void k_rank_scatter(const float* __restrict__ values, const int* __restrict__ ranks, uint32_t* __restrict__ sorted, int N,
                                                      int abs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)blockIdx.y * N;
  const uint32_t pos = (uint32_t)ranks[row + i];
  if (pos < (uint32_t)N) sorted[row + pos] = sim_key(values[row + i], abs);    // a rank outside the row (not bx_rank_desc's) is dropped, never written
}
// avg[r,i] = #{key < key_i} + (#{key == key_i} - 1) / 2 = (lower + upper - 1) / 2 with the two bounds of key_i in the sorted row: an
// integer below 2^21 times 0.5, exact in fp32.
__global__ __launch_bounds__(256) void k_rank_average(const float* __restrict__ values, const uint32_t* __restrict__ sorted, float* __restrict__ avg, int N,
                                                      int abs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)blockIdx.y * N;
  const uint32_t* s = sorted + row;
  const uint32_t key = sim_key(values[row + i], abs);
  int lo = 0, hi = N;                                                // first position with s[pos] >= key
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (s[mid] < key) lo = mid + 1; else hi = mid; }
  const int lower = lo;
  hi = N;                                                            // first position with s[pos] > key
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (s[mid] <= key) lo = mid + 1; else hi = mid; }
  avg[row + i] = (float)(lower + lo - 1) * 0.5f;
}
extern "C" size_t bx_rank_average_workspace(int R, int N) {
  if (sim_rows_ok("bx_rank_average_workspace", R, N) != BX_OK) return 0;
  return (size_t)R * N * sizeof(uint32_t);
}
extern "C" int bx_rank_average(const float* values, const int* ranks, float* avg, int R, int N, int abs, void* workspace, size_t workspace_bytes,
                               bxStream stream) {
  const char* who = "bx_rank_average";
  SIM_TRY(sim_rows_ok(who, R, N));
  if (R > 65535) BX_FAIL(BX_EUNSUPPORTED, "%s: %d rows, supported 1..65535", who, R);
  BX_REQUIRE(values && ranks && avg && workspace, "%s: null pointer", who);
  if (workspace_bytes < bx_rank_average_workspace(R, N))
    BX_FAIL(BX_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, bx_rank_average_workspace(R, N));
  BX_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace not 4-byte aligned", who);
  const dim3 grid(bx_ceil_div(N, 256), R);
  hipLaunchKernelGGL(k_rank_scatter, grid, dim3(256), 0, (hipStream_t)stream, values, ranks, (uint32_t*)workspace, N, abs ? 1 : 0);
  hipLaunchKernelGGL(k_rank_average, grid, dim3(256), 0, (hipStream_t)stream, values, (const uint32_t*)workspace, avg, N, abs ? 1 : 0);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- Pearson's correlation of two rows ----------------------------------------------------------------------------------------------------
// the fixed-order sum of 256 per-thread fp64 partials of NV values: a pairwise tree over the thread index (stride 128, 64, .., 1), the
// order of bx_infidelity_dot; every thread returns with the totals in sm[v][0] and may overwrite sm after the closing barrier
template <int NV>
__device__ __forceinline__ void sim_block_sum(double (&sm)[NV][256], const double (&acc)[NV], double (&tot)[NV]) {
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
#pragma unroll
  for (int v = 0; v < NV; ++v) tot[v] = sm[v][0];
  __syncthreads();
}
// One workgroup of 256 per row: thread t takes e = t, t + 256, ... in ascending e (four loads per operand in flight, the adds stay in e
// order), the 256 partials meet in the tree above.  Pass 1: the two sums and the means; pass 2: the three centred sums.  (One wave per
// row, the order of bx_mean_abs_rows, was measured first: 64 rows keep 64 waves busy, and the two correlations and the top-k count of
// [64,19,2000] maps took 0.50 ms against 0.30 ms for torch's fp64 reductions.)
__global__ __launch_bounds__(256) void k_map_corr(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ r, int N, int abs) {
  __shared__ double sm[3][256];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = a + (size_t)row * N;
  const float* y = b + (size_t)row * N;
  auto val = [&](const float* p, int t) -> double { const float v = p[t]; return (double)(abs ? fabsf(v) : v); };
  double s1[3] = {0.0, 0.0, 0.0}, m[3];
  int t = tid;
  for (; t + 768 < N; t += 1024) {
    double xv[4], yv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { xv[u] = val(x, t + 256 * u); yv[u] = val(y, t + 256 * u); }
#pragma unroll
    for (int u = 0; u < 4; ++u) { s1[0] += xv[u]; s1[1] += yv[u]; }
  }
  for (; t < N; t += 256) { s1[0] += val(x, t); s1[1] += val(y, t); }
  sim_block_sum<3>(sm, s1, m);
  const double mx = m[0] / (double)N, my = m[1] / (double)N;
  double s2[3] = {0.0, 0.0, 0.0}, c[3];                              // sxx, syy, sxy
  t = tid;
  for (; t + 768 < N; t += 1024) {
    double xv[4], yv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { xv[u] = val(x, t + 256 * u) - mx; yv[u] = val(y, t + 256 * u) - my; }
#pragma unroll
    for (int u = 0; u < 4; ++u) { s2[0] += xv[u] * xv[u]; s2[1] += yv[u] * yv[u]; s2[2] += xv[u] * yv[u]; }
  }
  for (; t < N; t += 256) {
    const double dx = val(x, t) - mx, dy = val(y, t) - my;
    s2[0] += dx * dx; s2[1] += dy * dy; s2[2] += dx * dy;
  }
  sim_block_sum<3>(sm, s2, c);
  if (tid == 0) {
    double v = c[2] / sqrt(c[0] * c[1]);                             // a NaN input stays NaN
    if (c[0] == 0.0 || c[1] == 0.0) v = __longlong_as_double(0x7ff8000000000000ll);
    r[row] = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
  }
}
extern "C" int bx_map_corr(const float* a, const float* b, double* r, int R, int N, int abs, bxStream stream) {
  const char* who = "bx_map_corr";
  SIM_TRY(sim_rows_ok(who, R, N));
  BX_REQUIRE(a && b && r, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)r & 7) == 0, "%s: r must be 8-byte aligned", who);
  hipLaunchKernelGGL(k_map_corr, dim3(R), dim3(256), 0, (hipStream_t)stream, a, b, r, N, abs ? 1 : 0);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- overlap of the top-k cells -----------------------------------------------------------------------------------------------------------
// One workgroup of 256 per row: an integer count (order-free) through the waves' butterflies and four LDS words, divided by k once.
__global__ __launch_bounds__(256) void k_topk_overlap(const int* __restrict__ ra, const int* __restrict__ rb, double* __restrict__ out, int N, int k) {
  __shared__ int wc[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int* x = ra + (size_t)row * N;
  const int* y = rb + (size_t)row * N;
  int c = 0;
  for (int t = tid; t < N; t += 256) c += ((unsigned)x[t] < (unsigned)k && (unsigned)y[t] < (unsigned)k) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((tid & 63) == 0) wc[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) out[row] = (double)(wc[0] + wc[1] + wc[2] + wc[3]) / (double)k;
}
extern "C" int bx_topk_overlap(const int* ranks_a, const int* ranks_b, double* out, int R, int N, int k, bxStream stream) {
  const char* who = "bx_topk_overlap";
  SIM_TRY(sim_rows_ok(who, R, N));
  BX_REQUIRE(k >= 1 && k <= N, "%s: k = %d outside 1..N = %d", who, k, N);
  BX_REQUIRE(ranks_a && ranks_b && out, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)out & 7) == 0, "%s: out must be 8-byte aligned", who);
  hipLaunchKernelGGL(k_topk_overlap, dim3(R), dim3(256), 0, (hipStream_t)stream, ranks_a, ranks_b, out, N, k);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- a row's extremes -----------------------------------------------------------------------------------------------------------------------
// One wave per row; fminf / fmaxf skip a NaN, so a row with finite cells gives their extremes whatever the order.
__global__ __launch_bounds__(256) void k_row_minmax(const float* __restrict__ v, float* __restrict__ lo, float* __restrict__ hi, int R, int N, int abs) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= R) return;
  const float* x = v + (size_t)row * N;
  float mn = INFINITY, mx = -INFINITY;
  for (int t = lane; t < N; t += 64) {
    const float e = abs ? fabsf(x[t]) : x[t];
    mn = fminf(mn, e); mx = fmaxf(mx, e);
  }
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  if (lane == 0) { lo[row] = mn; hi[row] = mx; }
}
extern "C" int bx_row_minmax(const float* v, float* lo, float* hi, int R, int N, int abs, bxStream stream) {
  const char* who = "bx_row_minmax";
  BX_REQUIRE(R > 0 && N > 0, "%s: bad shape R=%d N=%d", who, R, N);
  BX_REQUIRE((long long)R * N < (1ll << 31), "%s: R * N beyond 32-bit offsets", who);
  BX_REQUIRE(v && lo && hi, "%s: null pointer", who);
  hipLaunchKernelGGL(k_row_minmax, dim3(bx_ceil_div(R, 4)), dim3(256), 0, (hipStream_t)stream, v, lo, hi, R, N, abs ? 1 : 0);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- mean SSIM ------------------------------------------------------------------------------------------------------------------------------
// The geometry every entry point and kernel derives from (H, W, win): a map with one axis of extent 1 is a line of W' = H * W cells,
// filtered along it only.  Ho x Wo are the positions whose whole window lies inside the map; a workgroup owns a strip of SW columns of
// them, the widest power of two from 64 down to 4 whose five planes of H x SW doubles fit, halved while half of it still covers Wo.
struct SimGeom {
  int H, W, two, Ho, Wo, SW, strips;
};
static int sim_geom(const char* who, int H, int W, int win, SimGeom* g) {
  BX_REQUIRE(H > 0 && W > 0, "%s: bad shape H=%d W=%d", who, H, W);
  if ((long long)H * W > SIM_MAX_N) BX_FAIL(BX_EUNSUPPORTED, "%s: H * W = %lld cells per map, supported 1..%d", who, (long long)H * W, SIM_MAX_N);
  BX_REQUIRE(win >= 1 && (win & 1), "%s: window %d is not an odd number >= 1", who, win);
  if (win > BX_SSIM_MAX_WIN) BX_FAIL(BX_EUNSUPPORTED, "%s: window %d, supported 1..%d", who, win, BX_SSIM_MAX_WIN);
  g->two = H > 1 && W > 1;
  g->H = g->two ? H : 1;
  g->W = g->two ? W : H * W;
  BX_REQUIRE(g->W >= win && (!g->two || g->H >= win), "%s: window %d exceeds a filtered axis of the map %d x %d", who, win, H, W);
  g->Ho = g->two ? g->H - win + 1 : 1;
  g->Wo = g->W - win + 1;
  if (g->H * 4 > SIM_PLANE_CELLS)
    BX_FAIL(BX_EUNSUPPORTED, "%s: H = %d rows: a 4-column strip of the five moment planes does not fit %d bytes of LDS (H <= %d)", who, g->H, SIM_LDS_LIMIT,
            SIM_PLANE_CELLS / 4);
  int sw = 64;
  while (g->H * sw > SIM_PLANE_CELLS) sw >>= 1;
  while (sw > 4 && (sw >> 1) >= g->Wo) sw >>= 1;
  g->SW = sw;
  g->strips = bx_ceil_div(g->Wo, sw);
  return BX_OK;
}

struct SimNorm {                        // lo, hi fp32 [R] of each operand (NULL: the raw values), its flag abs
  const float* lo_a; const float* hi_a; const float* lo_b; const float* hi_b;
  int abs;
};
// cell -> fp64: |v| with abs; (v - lo) / (hi - lo) with a range, 0 everywhere when hi == lo
__device__ __forceinline__ double sim_cell(float v, int abs, bool norm, double lo, double span) {
  const double d = (double)(abs ? fabsf(v) : v);
  if (!norm) return d;
  return span == 0.0 ? 0.0 : (d - lo) / span;
}

// Phase 1: the five moments of every (image row y, strip column x) filtered along the row, taps in ascending order, into LDS planes
// [5][H][SW].  Phase 2: thread t takes the positions (y, x) = t, t + 256, ... of the strip's Ho x SW outputs in ascending order, filters
// the planes down the column, forms S and adds it to its partial; the 256 partials meet in the butterfly and the four wave sums are
// added in wave order.  part[r, strip] takes the strip's sum.
__global__ __launch_bounds__(256) void k_ssim_strips(const float* __restrict__ a, const float* __restrict__ b, const double* __restrict__ taps, SimNorm nm,
                                                     double C1, double C2, double cov, double* __restrict__ part, SimGeom g, int win) {
  extern __shared__ double sim_lds[];
  double* tp = sim_lds;                                              // [64]
  double* wsum = sim_lds + 64;                                       // [8]
  double* pl = sim_lds + SIM_HEAD;                                   // [5][H][SW]
  const int r = blockIdx.y, x0 = blockIdx.x * g.SW, tid = threadIdx.x;
  const int cols = g.Wo - x0 < g.SW ? g.Wo - x0 : g.SW;              // valid output columns of this strip, >= 1
  const int HS = g.H * g.SW;
  if (tid < win) tp[tid] = taps[tid];
  const bool norm = nm.lo_a != nullptr;
  double la = 0.0, sa = 0.0, lb = 0.0, sb = 0.0;
  if (norm) {
    la = (double)nm.lo_a[r]; sa = (double)nm.hi_a[r] - la;
    lb = (double)nm.lo_b[r]; sb = (double)nm.hi_b[r] - lb;
  }
  __syncthreads();
  const float* am = a + (size_t)r * g.H * g.W;
  const float* bm = b + (size_t)r * g.H * g.W;
  for (int it = tid; it < HS; it += 256) {
    const int y = it / g.SW, x = it - y * g.SW;
    if (x >= cols) continue;                                         // x0 + x + win - 1 <= W - 1 holds for the valid columns only
    const float* ar = am + (size_t)y * g.W + x0 + x;
    const float* br = bm + (size_t)y * g.W + x0 + x;
    double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
    for (int t = 0; t < win; ++t) {
      const double w = tp[t], xv = sim_cell(ar[t], nm.abs, norm, la, sa), yv = sim_cell(br[t], nm.abs, norm, lb, sb);
      ux += w * xv; uy += w * yv; uxx += w * (xv * xv); uyy += w * (yv * yv); uxy += w * (xv * yv);
    }
    pl[it] = ux; pl[HS + it] = uy; pl[2 * HS + it] = uxx; pl[3 * HS + it] = uyy; pl[4 * HS + it] = uxy;
  }
  __syncthreads();
  const int wv = g.two ? win : 1, outs = g.Ho * g.SW;
  double acc = 0.0;
  for (int it = tid; it < outs; it += 256) {
    const int y = it / g.SW, x = it - y * g.SW;
    if (x >= cols) continue;
    double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
    if (g.two) {
      for (int t = 0; t < wv; ++t) {
        const double w = tp[t];
        const int at = (y + t) * g.SW + x;                           // y + t <= Ho - 1 + win - 1 = H - 1
        ux += w * pl[at]; uy += w * pl[HS + at]; uxx += w * pl[2 * HS + at]; uyy += w * pl[3 * HS + at]; uxy += w * pl[4 * HS + at];
      }
    } else {
      ux = pl[it]; uy = pl[HS + it]; uxx = pl[2 * HS + it]; uyy = pl[3 * HS + it]; uxy = pl[4 * HS + it];
    }
    const double vx = cov * (uxx - ux * ux), vy = cov * (uyy - uy * uy), vxy = cov * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    acc += (A1 * A2) / (B1 * B2);
  }
  acc = sim_wave_sum(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) part[(size_t)r * g.strips + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// out[r] = (sum of the row's strip sums in ascending strip order) / (Ho * Wo): one thread per row
__global__ __launch_bounds__(64) void k_ssim_finish(const double* __restrict__ part, double* __restrict__ out, int R, int strips, double count) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  double s = 0.0;
  for (int k = 0; k < strips; ++k) s += part[(size_t)r * strips + k];
  out[r] = s / count;
}
extern "C" int bx_ssim_strip(int H, int W, int win) {
  SimGeom g;
  return sim_geom("bx_ssim_strip", H, W, win, &g) == BX_OK ? g.SW : 0;
}
extern "C" size_t bx_ssim_rows_workspace(int R, int H, int W, int win) {
  SimGeom g;
  if (R <= 0 || R > 65535 || sim_geom("bx_ssim_rows_workspace", H, W, win, &g) != BX_OK) return 0;
  return (size_t)R * g.strips * sizeof(double);
}
extern "C" int bx_ssim_rows(const float* a, const float* b, const double* taps, const float* lo_a, const float* hi_a, const float* lo_b, const float* hi_b,
                            double data_range, double cov_norm, double* out, int R, int H, int W, int win, int abs, void* workspace, size_t workspace_bytes,
                            bxStream stream) {
  const char* who = "bx_ssim_rows";
  BX_REQUIRE(R > 0, "%s: bad shape R=%d", who, R);
  if (R > 65535) BX_FAIL(BX_EUNSUPPORTED, "%s: %d rows, supported 1..65535", who, R);
  SimGeom g;
  SIM_TRY(sim_geom(who, H, W, win, &g));
  BX_REQUIRE((long long)R * H * W < (1ll << 31), "%s: R * H * W beyond 32-bit offsets", who);
  BX_REQUIRE(data_range > 0.0 && data_range < INFINITY && cov_norm > 0.0 && cov_norm < INFINITY, "%s: data_range and cov_norm must be finite and > 0", who);
  const bool norm = lo_a || hi_a || lo_b || hi_b;
  BX_REQUIRE(!norm || (lo_a && hi_a && lo_b && hi_b), "%s: the four range arrays are given or omitted together", who);
  BX_REQUIRE(a && b && taps && out && workspace, "%s: null pointer", who);
  if (workspace_bytes < (size_t)R * g.strips * sizeof(double))
    BX_FAIL(BX_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, (size_t)R * g.strips * sizeof(double));
  BX_REQUIRE((((uintptr_t)workspace | (uintptr_t)out | (uintptr_t)taps) & 7) == 0, "%s: the fp64 arrays must be 8-byte aligned", who);
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const SimNorm nm = {lo_a, hi_a, lo_b, hi_b, abs ? 1 : 0};
  const size_t lds = ((size_t)SIM_HEAD + 5 * (size_t)g.H * g.SW) * sizeof(double);     // <= SIM_LDS_LIMIT by sim_geom
  hipLaunchKernelGGL(k_ssim_strips, dim3(g.strips, R), dim3(256), lds, (hipStream_t)stream, a, b, taps, nm, C1, C2, cov_norm, (double*)workspace, g, win);
  hipLaunchKernelGGL(k_ssim_finish, dim3(bx_ceil_div(R, 64)), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, out, R, g.strips,
                     (double)g.Ho * (double)g.Wo);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}

// ---- uniform re-initialisation of a parameter tensor --------------------------------------------------------------------------------------
// p[e] = fl32(bound * u), u = (w >> 8) * 2^-23 - 1 with w the word e & 3 of the Philox block of counter (e >> 2, j, s, 2): one block per
// thread serves four elements, the last block of a tensor may be partial.  V = 4: p is 16-byte aligned, one 16-byte store per full block.
template <int V>
__global__ __launch_bounds__(256) void k_param_uniform(float* __restrict__ p, uint32_t n, float bound, uint32_t j, uint32_t s, uint32_t k0, uint32_t k1) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q > (n - 1u) >> 2) return;
  uint32_t w[4];
  sg_philox(q, j, s, 2u, k0, k1, w);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = bound * sg_uniform(w[i]);
  const uint32_t e0 = q * 4u, m = n - e0 < 4u ? n - e0 : 4u;
  if (V == 4 && m == 4u) {
    *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((uint32_t)i < m) p[e0 + i] = v[i];
  }
}
extern "C" int bx_param_uniform(float* p, size_t n, float bound, uint64_t seed, uint32_t j, uint32_t s, bxStream stream) {
  const char* who = "bx_param_uniform";
  BX_REQUIRE(n >= 1 && n < ((size_t)1 << 31), "%s: n = %zu outside 1..2^31 - 1", who, n);
  BX_REQUIRE(bound >= 0.f && bound < INFINITY, "%s: bound must be finite and >= 0", who);
  BX_REQUIRE(p, "%s: null pointer", who);
  BX_REQUIRE(((uintptr_t)p & 3) == 0, "%s: p must be 4-byte aligned", who);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  const int blocks = bx_ceil_div(bx_ceil_div((long long)n, 4), 256);
  if (((uintptr_t)p & 15) == 0)
    hipLaunchKernelGGL((k_param_uniform<4>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, (uint32_t)n, bound, j, s, k0, k1);
  else
    hipLaunchKernelGGL((k_param_uniform<1>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, (uint32_t)n, bound, j, s, k0, k1);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
