// RISE saliency (Petsiuk et al., BMVC 2018): the masks, the perturbed batches straight in the model's layouts, and the weighted sum
// of the masks by the class probabilities.  A mask is a function of a gh x gw bit grid and two shift integers, so every kernel
// recomputes the value where it needs it from bit rows staged in LDS; the N x Hm x Wm masks exist in memory only when
// bx_rise_masks is asked for them.  The forward passes between perturb and accumulate are the model's own kernels.
// See include/brainxai.h for the definition and the contract of each entry point.
// Compiled with -ffp-contract=off (build.py): every product and sum below rounds on its own, which is what lets a numpy float32
// restatement of the mask and of base + m * (x - base) match bit for bit.
#include "perturb_rows.h"

#define RISE_MAX_G 32                  // grid cells per axis: one row of bits is one 32-bit word
#define RISE_MAX_K 32
#define RISE_MAX_HW ((1 << 20) - 1)    // cells of a map, the limit of bx_rank_desc: the map drops straight into deletion_insertion
#define RISE_CHUNK 32                  // masks staged per step of the weighted sum
#define RISE_TQ 8                      // (sample, class) pairs a thread of the weighted sum accumulates

struct RiseGeom {
  int gh, gw, ch, cw;                  // grid and cell size, ch = ceil(Hm / gh)
  float sy, sx;                        // g / ((g + 1) * c): source cells per up-sampled pixel
};
static RiseGeom rise_geom(int gh, int gw, int Hm, int Wm) {
  RiseGeom g;
  g.gh = gh; g.gw = gw; g.ch = bx_ceil_div(Hm, gh); g.cw = bx_ceil_div(Wm, gw);
  g.sy = (float)gh / (float)((gh + 1) * g.ch);
  g.sx = (float)gw / (float)((gw + 1) * g.cw);
  return g;
}

// up-sampled coordinate u -> the two source cells and the weight of the second (bilinear, align_corners=False)
__device__ __forceinline__ void rise_axis(int u, float scale, int g, int& i0, int& i1, float& l) {
  float s = ((float)u + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 < g - 1 ? i0 : g - 1;
  i1 = i0 + 1 < g - 1 ? i0 + 1 : g - 1;
  l = s - (float)i0;
}
// horizontal blend first, then vertical; rows = the mask's gh words, bit c of word r = bits[r][c]
__device__ __forceinline__ float rise_value(const uint32_t* rows, int y0, int y1, float ly, int x0, int x1, float lx) {
  const uint32_t r0 = rows[y0], r1 = rows[y1];
  const float a = (float)((r0 >> x0) & 1u), b = (float)((r0 >> x1) & 1u), c = (float)((r1 >> x0) & 1u), d = (float)((r1 >> x1) & 1u);
  const float top = (1.f - lx) * a + lx * b, bot = (1.f - lx) * c + lx * d;
  return (1.f - ly) * top + ly * bot;
}
// LDS rows[j * gh + r] = bit row r of mask first + j, j < count (masks past N - 1 repeat the last one); all threads call
__device__ __forceinline__ void rise_stage(uint32_t* rows, const unsigned char* __restrict__ bits, int first, int count, int N, int gh, int gw) {
  for (int i = threadIdx.x; i < count * gh; i += blockDim.x) {
    const int j = i / gh, r = i - j * gh, n = first + j < N ? first + j : N - 1;
    const unsigned char* src = bits + ((size_t)n * gh + r) * gw;
    uint32_t word = 0u;
    for (int c = 0; c < gw; ++c) word |= (src[c] != 0 ? 1u : 0u) << c;
    rows[i] = word;
  }
}
// the shift of mask n, kept inside [0, cell) whatever the caller uploaded (wave-uniform loads)
__device__ __forceinline__ void rise_shift(const int* __restrict__ shifts, int n, const RiseGeom& g, int& dy, int& dx) {
  dy = shifts[2 * (size_t)n]; dx = shifts[2 * (size_t)n + 1];
  dy = dy < 0 ? 0 : (dy > g.ch - 1 ? g.ch - 1 : dy);
  dx = dx < 0 ? 0 : (dx > g.cw - 1 ? g.cw - 1 : dx);
}

static int rise_shape_ok(const char* who, int N, int gh, int gw, int Hm, int Wm, int n0, int n) {
  BX_REQUIRE(N > 0 && Hm > 0 && Wm > 0, "%s: bad shape N=%d Hm=%d Wm=%d", who, N, Hm, Wm);
  if ((long long)Hm * Wm > RISE_MAX_HW) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld cells per mask, supported 1..%d", who, (long long)Hm * Wm, RISE_MAX_HW);
  BX_REQUIRE(gh >= 1 && gw >= 1, "%s: grid %d x %d", who, gh, gw);
  if (gh > RISE_MAX_G || gw > RISE_MAX_G || gh > Hm || gw > Wm)
    BX_FAIL(BX_EUNSUPPORTED, "%s: grid %d x %d, supported 1..min(%d, Hm = %d) x 1..min(%d, Wm = %d)", who, gh, gw, RISE_MAX_G, Hm, RISE_MAX_G, Wm);
  BX_REQUIRE(N < (1 << 24), "%s: N = %d masks, supported below 2^24", who, N);
  BX_REQUIRE(n0 >= 0 && n >= 1 && (long long)n0 + n <= N, "%s: masks n0 = %d, n = %d outside 0..N = %d", who, n0, n, N);
  return BX_OK;
}

// ---- the masks themselves ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rise_masks(const unsigned char* __restrict__ bits, const int* __restrict__ shifts, float* __restrict__ out,
                                                    RiseGeom g, int N, int HW, int Wm, int n0, int n) {
  __shared__ uint32_t rows[PERTURB_SPW * RISE_MAX_G];
  const int j0 = blockIdx.y * PERTURB_SPW, p = blockIdx.x * 256 + threadIdx.x;
  rise_stage(rows, bits, n0 + j0, PERTURB_SPW, N, g.gh, g.gw);
  __syncthreads();
  if (p >= HW) return;
  const int y = p / Wm, x = p - y * Wm;
  for (int sj = 0; sj < PERTURB_SPW && j0 + sj < n; ++sj) {
    int dy, dx, y0, y1, x0, x1; float ly, lx;
    rise_shift(shifts, n0 + j0 + sj, g, dy, dx);
    rise_axis(y + dy, g.sy, g.gh, y0, y1, ly);
    rise_axis(x + dx, g.sx, g.gw, x0, x1, lx);
    out[(size_t)(j0 + sj) * HW + p] = rise_value(rows + sj * g.gh, y0, y1, ly, x0, x1, lx);
  }
}
extern "C" int bx_rise_masks(const unsigned char* bits, const int* shifts, float* out, int N, int gh, int gw, int Hm, int Wm, int n0, int n,
                             bxStream stream) {
  const int rc = rise_shape_ok("bx_rise_masks", N, gh, gw, Hm, Wm, n0, n);
  if (rc) return rc;
  BX_REQUIRE((long long)n * Hm * Wm < (1ll << 31) && bx_ceil_div(n, PERTURB_SPW) <= 65535,
             "bx_rise_masks: n * Hm * Wm = %lld values beyond 32-bit offsets; use a smaller window", (long long)n * Hm * Wm);
  BX_REQUIRE(bits && shifts && out, "bx_rise_masks: null pointer");
  const dim3 grid(bx_ceil_div((long long)Hm * Wm, 256), bx_ceil_div(n, PERTURB_SPW));
  hipLaunchKernelGGL(k_rise_masks, grid, dim3(256), 0, (hipStream_t)stream, bits, shifts, out, rise_geom(gh, gw, Hm, Wm), N, Hm * Wm, Wm, n0, n);
  BX_CHECK_LAUNCH("bx_rise_masks");
  return BX_OK;
}

// ---- perturbed batches ------------------------------------------------------------------------------------------------------------------
// base + m * (x - base), the mask value m shared by the channels of a pixel (the kernels are perturb_rows.h's).  A group's bit rows are
// staged in LDS; a cell keeps its (y, x) and a row shifts it, finds its source cells and blends.
struct RiseMask {
  struct Lds { uint32_t rows[PERTURB_SPW * RISE_MAX_G]; };
  struct Cell { int y, x; };
  const unsigned char* bits;
  const int* shifts;
  RiseGeom g;
  int N, n0;
  __device__ __forceinline__ void stage(Lds& lds, int, int j0, int) const {
    rise_stage(lds.rows, bits, n0 + j0, PERTURB_SPW, N, g.gh, g.gw);
    __syncthreads();
  }
  __device__ __forceinline__ Cell cell(int, int, int y, int x) const { return {y, x}; }
  __device__ __forceinline__ float row(const Lds& lds, const Cell& c, int, int j0, int sj) const {
    int dy, dx, y0, y1, x0, x1; float ly, lx;
    rise_shift(shifts, n0 + j0 + sj, g, dy, dx);
    rise_axis(c.y + dy, g.sy, g.gh, y0, y1, ly);
    rise_axis(c.x + dx, g.sx, g.gw, x0, x1, lx);
    return rise_value(lds.rows + sj * g.gh, y0, y1, ly, x0, x1, lx);
  }
};
static int rise_baseline_ok(const char* who, int B, int kind) {
  BX_REQUIRE(B > 0, "%s: bad shape B=%d", who, B);
  BX_REQUIRE(kind >= 0 && kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel, 2 full tensor)", who, kind);
  return BX_OK;
}
extern "C" int bx_rise_perturb_spec(const float* x, const unsigned char* bits, const int* shifts, const float* baseline, int baseline_kind, void* out,
                                    int B, int C, int H, int W, int Cp, int N, int gh, int gw, int n0, int n, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  int rc = rise_shape_ok("bx_rise_perturb_spec", N, gh, gw, H, W, n0, n);
  if (rc) return rc;
  if ((rc = rise_baseline_ok("bx_rise_perturb_spec", B, baseline_kind)) != BX_OK) return rc;
  if ((rc = perturb_layout_ok("bx_rise_perturb_spec", "channels", C, Cp)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_rise_perturb_spec", "B", B, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && bits && shifts && baseline && out, "bx_rise_perturb_spec: null pointer");
  const RiseMask mask = {bits, shifts, rise_geom(gh, gw, H, W), N, n0};
  BX_DISPATCH_DTYPE(dtype, T, perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, B, C, H, W, 0, n, mask));
  BX_CHECK_LAUNCH("bx_rise_perturb_spec");
  return BX_OK;
}

// the mask row of element (ch, t) is ch for an electrode-by-time mask and 0 for a time-column mask
extern "C" int bx_rise_perturb_eeg(const float* x, const unsigned char* bits, const int* shifts, int map_rows, const float* baseline, int baseline_kind,
                                   float* out, int B, int Chans, int T, int N, int gh, int gw, int n0, int n, bxStream stream) {
  BX_REQUIRE(Chans > 0 && T > 0 && (map_rows == Chans || map_rows == 1), "bx_rise_perturb_eeg: bad shape Chans=%d T=%d map_rows=%d (Chans or 1)", Chans, T, map_rows);
  BX_REQUIRE((long long)Chans * T < (1ll << 31), "bx_rise_perturb_eeg: Chans * T beyond 32-bit offsets");
  int rc = rise_shape_ok("bx_rise_perturb_eeg", N, gh, gw, map_rows, T, n0, n);
  if (rc) return rc;
  if ((rc = rise_baseline_ok("bx_rise_perturb_eeg", B, baseline_kind)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_rise_perturb_eeg", "B", B, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && bits && shifts && baseline && out, "bx_rise_perturb_eeg: null pointer");
  const RiseMask mask = {bits, shifts, rise_geom(gh, gw, map_rows, T), N, n0};
  perturb_launch_eeg(stream, x, baseline, baseline_kind, out, B, Chans, T, map_rows, 0, n, mask);
  BX_CHECK_LAUNCH("bx_rise_perturb_eeg");
  return BX_OK;
}

// ---- the weighted sum -------------------------------------------------------------------------------------------------------------------
// A thread owns one cell p and RISE_TQ (sample, class) pairs; it walks the masks in index order, recomputes m_n(p) once per mask and
// adds (double)P * (double)m to each pair's fp64 register (the product of two fp32 values is exact in fp64).  The index of P depends
// on the workgroup and the loop counter alone, so its loads are wave-uniform; the bit rows arrive through LDS RISE_CHUNK masks at a
// time.  No atomics: the bits of the result are a function of the inputs alone.  One rounding to fp32, after the division.
__global__ __launch_bounds__(256) void k_rise_accumulate(const float* __restrict__ P, const int* __restrict__ classes, const unsigned char* __restrict__ bits,
                                                         const int* __restrict__ shifts, float* __restrict__ sal, float* __restrict__ coverage, RiseGeom g,
                                                         int N, int K, int Q, int HW, int Wm, double expected, int normalize) {
  __shared__ uint32_t rows[RISE_CHUNK * RISE_MAX_G];
  const int q0 = blockIdx.y * RISE_TQ, p = blockIdx.x * 256 + threadIdx.x, pc = p < HW ? p : HW - 1;
  const int y = pc / Wm, x = pc - y * Wm;
  size_t off[RISE_TQ];
  double acc[RISE_TQ], cov = 0.0;
#pragma unroll
  for (int t = 0; t < RISE_TQ; ++t) {
    const int q = q0 + t < Q ? q0 + t : Q - 1;                      // pairs past the end repeat the last one and are not written
    int b = q, k;
    if (classes) { k = classes[q]; k = k < 0 ? 0 : (k >= K ? K - 1 : k); }
    else { b = q / K; k = q - b * K; }
    off[t] = (size_t)b * N * K + k;
    acc[t] = 0.0;
  }
  for (int c0 = 0; c0 < N; c0 += RISE_CHUNK) {
    const int cnt = N - c0 < RISE_CHUNK ? N - c0 : RISE_CHUNK;
    __syncthreads();                                                // the previous chunk's rows are no longer read
    rise_stage(rows, bits, c0, cnt, N, g.gh, g.gw);
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int nn = c0 + j;
      int dy, dx, y0, y1, x0, x1; float ly, lx;
      rise_shift(shifts, nn, g, dy, dx);
      rise_axis(y + dy, g.sy, g.gh, y0, y1, ly);
      rise_axis(x + dx, g.sx, g.gw, x0, x1, lx);
      const double m = (double)rise_value(rows + j * g.gh, y0, y1, ly, x0, x1, lx);
      cov += m;
#pragma unroll
      for (int t = 0; t < RISE_TQ; ++t) acc[t] += (double)P[off[t] + (size_t)nn * K] * m;
    }
  }
  if (p >= HW) return;
  const double D = normalize ? cov : expected;
#pragma unroll
  for (int t = 0; t < RISE_TQ; ++t)
    if (q0 + t < Q) sal[(size_t)(q0 + t) * HW + p] = D > 0.0 ? (float)(acc[t] / D) : 0.f;
  if (blockIdx.y == 0) coverage[p] = (float)cov;
}
extern "C" int bx_rise_accumulate(const float* P, const int* classes, const unsigned char* bits, const int* shifts, float* sal, float* coverage, int B,
                                  int N, int K, int gh, int gw, int Hm, int Wm, double p1, int normalize, bxStream stream) {
  const int rc = rise_shape_ok("bx_rise_accumulate", N, gh, gw, Hm, Wm, 0, N > 0 ? N : 1);
  if (rc) return rc;
  BX_REQUIRE(B > 0 && K >= 1, "bx_rise_accumulate: bad shape B=%d K=%d", B, K);
  if (K > RISE_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_rise_accumulate: %d classes, supported 1..%d", K, RISE_MAX_K);
  BX_REQUIRE(p1 > 0.0 && p1 <= 1.0, "bx_rise_accumulate: p1 = %g outside (0, 1]", p1);
  BX_REQUIRE(normalize == 0 || normalize == 1, "bx_rise_accumulate: normalize %d (0 expected: N * p1, 1 coverage: the sum of the masks)", normalize);
  BX_REQUIRE((long long)B * N * K < (1ll << 31) && (long long)B * K * Hm * Wm < (1ll << 31) && bx_ceil_div((long long)B * K, RISE_TQ) <= 65535,
             "bx_rise_accumulate: B * N * K or B * K * Hm * Wm beyond 32-bit offsets");
  BX_REQUIRE(P && bits && shifts && sal && coverage, "bx_rise_accumulate: null pointer");
  const int Q = classes ? B : B * K;
  const dim3 grid(bx_ceil_div((long long)Hm * Wm, 256), bx_ceil_div(Q, RISE_TQ));
  hipLaunchKernelGGL(k_rise_accumulate, grid, dim3(256), 0, (hipStream_t)stream, P, classes, bits, shifts, sal, coverage, rise_geom(gh, gw, Hm, Wm), N, K, Q,
                     Hm * Wm, Wm, (double)N * p1, normalize);
  BX_CHECK_LAUNCH("bx_rise_accumulate");
  return BX_OK;
}
