// Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's Occlusion): the rows of an input with one sliding window replaced by the
// baseline, straight in the model's layouts, and the per-cell mean of the score drops of the windows that cover a cell.  A window is a
// function of its index and six integers, so no mask is ever stored.  The forward passes between perturb and accumulate are the
// model's own kernels.  See include/brainxai.h for the definition and the contract of each entry point.
// A row is a selection, not a blend: there is no multiply to contract, so the file needs no flags of its own.
#include "perturb_rows.h"

#define OCC_MAX_K 32
#define OCC_MAX_HW ((1 << 20) - 1)     // cells of a map, the limit of bx_rank_desc: the map drops straight into deletion_insertion

struct OccGeom {
  int wh, ww, sh, sw, ny, nx;          // window, stride, window positions per axis: n = 1 + ceil((size - w) / s)
};

// window j = iy * nx + ix covers rows [y0, y0 + wh) and columns [x0, x0 + ww); the domain's border clips it (a cell is inside the domain)
__device__ __forceinline__ void occ_window(const OccGeom& g, int j, int& y0, int& x0) {
  const int iy = j / g.nx;
  y0 = iy * g.sh; x0 = (j - iy * g.nx) * g.sw;
}
__device__ __forceinline__ bool occ_inside(int v, int lo, int w) { return (unsigned)(v - lo) < (unsigned)w; }

static int occ_geom_ok(const char* who, int Hm, int Wm, int wh, int ww, int sh, int sw, OccGeom* g) {
  BX_REQUIRE(Hm > 0 && Wm > 0, "%s: bad shape Hm=%d Wm=%d", who, Hm, Wm);
  if ((long long)Hm * Wm > OCC_MAX_HW) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld cells per map, supported 1..%d", who, (long long)Hm * Wm, OCC_MAX_HW);
  BX_REQUIRE(wh >= 1 && wh <= Hm && ww >= 1 && ww <= Wm, "%s: window %d x %d outside 1..%d x 1..%d", who, wh, ww, Hm, Wm);
  BX_REQUIRE(sh >= 1 && sh <= wh && sw >= 1 && sw <= ww, "%s: stride %d x %d outside 1..window = %d x %d (a larger stride leaves cells uncovered)", who, sh,
             sw, wh, ww);
  g->wh = wh; g->ww = ww; g->sh = sh; g->sw = sw;
  g->ny = 1 + bx_ceil_div(Hm - wh, sh); g->nx = 1 + bx_ceil_div(Wm - ww, sw);
  return BX_OK;
}
static int occ_rows_ok(const char* who, const OccGeom& g, int B, int kind, int n0, int n) {
  BX_REQUIRE(B > 0, "%s: bad shape B=%d", who, B);
  BX_REQUIRE(kind >= 0 && kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel, 2 full tensor)", who, kind);
  BX_REQUIRE(n0 >= 0 && n >= 1 && (long long)n0 + n <= (long long)g.ny * g.nx, "%s: windows n0 = %d, n = %d outside 0..N = %d x %d", who, n0, n, g.ny, g.nx);
  return BX_OK;
}

// ---- perturbed batches ------------------------------------------------------------------------------------------------------------------
// A cell keeps its (y, x); a row costs two wave-uniform window corners and two compares (the kernels are perturb_rows.h's).
struct OccMask {
  struct Lds {};
  struct Cell { int y, x; };
  OccGeom g;
  int n0;
  __device__ __forceinline__ void stage(Lds&, int, int, int) const {}
  __device__ __forceinline__ Cell cell(int, int, int y, int x) const { return {y, x}; }
  __device__ __forceinline__ bool row(const Lds&, const Cell& c, int, int j0, int sj) const {
    int y0, x0;
    occ_window(g, n0 + j0 + sj, y0, x0);
    return !(occ_inside(c.y, y0, g.wh) && occ_inside(c.x, x0, g.ww));
  }
};
extern "C" int bx_occlusion_perturb_spec(const float* x, const float* baseline, int baseline_kind, void* out, int B, int C, int H, int W, int Cp, int wh,
                                         int ww, int sh, int sw, int n0, int n, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  OccGeom g;
  int rc = occ_geom_ok("bx_occlusion_perturb_spec", H, W, wh, ww, sh, sw, &g);
  if (rc) return rc;
  if ((rc = occ_rows_ok("bx_occlusion_perturb_spec", g, B, baseline_kind, n0, n)) != BX_OK) return rc;
  if ((rc = perturb_layout_ok("bx_occlusion_perturb_spec", "channels", C, Cp)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_occlusion_perturb_spec", "B", B, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && baseline && out, "bx_occlusion_perturb_spec: null pointer");
  const OccMask mask = {g, n0};
  BX_DISPATCH_DTYPE(dtype, T, perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, B, C, H, W, 0, n, mask));
  BX_CHECK_LAUNCH("bx_occlusion_perturb_spec");
  return BX_OK;
}

// the cell of element (ch, t) is (ch, t)
extern "C" int bx_occlusion_perturb_eeg(const float* x, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int wh, int ww,
                                        int sh, int sw, int n0, int n, bxStream stream) {
  OccGeom g;
  int rc = occ_geom_ok("bx_occlusion_perturb_eeg", Chans, T, wh, ww, sh, sw, &g);
  if (rc) return rc;
  if ((rc = occ_rows_ok("bx_occlusion_perturb_eeg", g, B, baseline_kind, n0, n)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_occlusion_perturb_eeg", "B", B, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && baseline && out, "bx_occlusion_perturb_eeg: null pointer");
  const OccMask mask = {g, n0};
  perturb_launch_eeg(stream, x, baseline, baseline_kind, out, B, Chans, T, Chans, 0, n, mask);
  BX_CHECK_LAUNCH("bx_occlusion_perturb_eeg");
  return BX_OK;
}

// ---- the map ----------------------------------------------------------------------------------------------------------------------------
// A thread owns one cell p and walks the (sample, class) pairs of its workgroup row.  The windows that cover the cell are
// iy in [max(0, ceil((y - wh + 1) / sh)), min(ny - 1, y / sh)] times the same range in x: at most ceil(wh / sh) * ceil(ww / sw) of
// them, visited in ascending j = iy * nx + ix.  Each difference (double)S0 - (double)S, their sum and the quotient by the count are
// fp64; one rounding to fp32.  No atomics: the bits of the result are a function of the inputs alone.
__global__ __launch_bounds__(256) void k_occ_accumulate(const float* __restrict__ S, const float* __restrict__ S0, const int* __restrict__ classes,
                                                        float* __restrict__ attr, int* __restrict__ counts, OccGeom g, int N, int K, int Q, int HW, int Wm) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / Wm, x = p - y * Wm;
  const int iy0 = y - g.wh + 1 > 0 ? (y - g.wh + g.sh) / g.sh : 0, iy1 = y / g.sh < g.ny - 1 ? y / g.sh : g.ny - 1;
  const int ix0 = x - g.ww + 1 > 0 ? (x - g.ww + g.sw) / g.sw : 0, ix1 = x / g.sw < g.nx - 1 ? x / g.sw : g.nx - 1;
  const int cnt = (iy1 - iy0 + 1) * (ix1 - ix0 + 1);                // >= 1: stride <= window and the last window reaches the border
  if (blockIdx.y == 0) counts[p] = cnt;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    int b = q, k;
    if (classes) { k = classes[q]; k = k < 0 ? 0 : (k >= K ? K - 1 : k); }
    else { b = q / K; k = q - b * K; }
    const float* Sq = S + (size_t)b * N * K + k;
    const double s0 = (double)S0[(size_t)b * K + k];
    double acc = 0.0;
    for (int iy = iy0; iy <= iy1; ++iy)
      for (int ix = ix0; ix <= ix1; ++ix) acc += s0 - (double)Sq[(size_t)(iy * g.nx + ix) * K];
    attr[(size_t)q * HW + p] = (float)(acc / (double)cnt);
  }
}
extern "C" int bx_occlusion_accumulate(const float* S, const float* S0, const int* classes, float* attr, int* counts, int B, int N, int K, int Hm, int Wm,
                                       int wh, int ww, int sh, int sw, bxStream stream) {
  OccGeom g;
  const int rc = occ_geom_ok("bx_occlusion_accumulate", Hm, Wm, wh, ww, sh, sw, &g);
  if (rc) return rc;
  BX_REQUIRE(B > 0 && K >= 1, "bx_occlusion_accumulate: bad shape B=%d K=%d", B, K);
  if (K > OCC_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_occlusion_accumulate: %d classes, supported 1..%d", K, OCC_MAX_K);
  BX_REQUIRE((long long)g.ny * g.nx == N, "bx_occlusion_accumulate: N = %d scores per sample, the geometry has %d x %d windows", N, g.ny, g.nx);
  BX_REQUIRE((long long)B * N * K < (1ll << 31) && (long long)B * K * Hm * Wm < (1ll << 31),
             "bx_occlusion_accumulate: B * N * K or B * K * Hm * Wm beyond 32-bit offsets");
  BX_REQUIRE(S && S0 && attr && counts, "bx_occlusion_accumulate: null pointer");
  const int Q = classes ? B : B * K;
  const dim3 grid(bx_ceil_div((long long)Hm * Wm, 256), Q < 65535 ? Q : 65535);
  hipLaunchKernelGGL(k_occ_accumulate, grid, dim3(256), 0, (hipStream_t)stream, S, S0, classes, attr, counts, g, N, K, Q, Hm * Wm, Wm);
  BX_CHECK_LAUNCH("bx_occlusion_accumulate");
  return BX_OK;
}
