// Score-CAM (Wang et al., CVPR-W 2020): a class-activation map at a layer whose channel weights come from forward passes of the input
// seen through each up-sampled, min-max normalised activation channel.  No gradient.  The B x C masks of Hm x Wm values are never
// stored: the range pass, the perturb kernels and nothing else need a mask value, and each recomputes it in registers from the
// (small) activation plane.  The forward passes between perturb and combine are the model's own kernels.
// See include/brainxai.h for the definition and the contract of each entry point.
// Compiled with -ffp-contract=off (build.py): every product and sum of the up-sampling, of the mask and of base + m * (x - base)
// rounds on its own, which is what lets a numpy float32 restatement (tests/scorecam_ref.py) match them bit for bit.
#include "perturb_rows.h"
#include <math.h>

#define SC_MAX_K 32
#define SC_MAX_HW ((1 << 20) - 1)      // cells of a map, the limit of bx_rank_desc: the map drops straight into deletion_insertion
#define SC_PLANE 1024                  // values of one plane staged by a perturb workgroup (PERTURB_SPW planes: 32 KB)
#define SC_PLANE_LD (SC_PLANE + 4)     // LDS stride of a staged plane: 8 planes x 4 positions written by 32 lanes land on 32 banks
#define SC_RANGE_PLANE 4096            // values of the plane staged by a range workgroup
#define SC_RANGE_PER 16                // up-sampled values per thread of the range pass: 4096 per workgroup

// One activation: element (b, k, y, x) lives at A[b * sb + k * sc + y * sy + x * sx].  NHWC [B,h,w,C]: (h w C, 1, w C, C); the EEG
// branch's saved maps [B,C,w]: (C w, w, 0, 1) with h = 1.  ry = (float)h / (float)Hm and rx likewise: the scale of bilinear_src.
struct ScPlane {
  int sb, sc, sy, sx, h, w, C;
  float ry, rx;
};

// horizontal blend first, then vertical: the convention of bx_resize_bilinear
__device__ __forceinline__ float sc_blend(float a00, float a01, float a10, float a11, float ly, float lx) {
  const float top = (1.f - lx) * a00 + lx * a01, bot = (1.f - lx) * a10 + lx * a11;
  return (1.f - ly) * top + ly * bot;
}
__device__ __forceinline__ float sc_wave_min(float v) { return -wave_max(-v); }      // negation is exact

static int sc_plane_ok(const char* who, const void* A, int dtype, int sb, int sc, int sy, int sx, int B, int C, int h, int w, int Hm, int Wm,
                       ScPlane* pl) {
  BX_DTYPE_OK(dtype);
  BX_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0 && Hm > 0 && Wm > 0, "%s: bad shape B=%d C=%d plane %d x %d domain %d x %d", who, B, C, h, w, Hm, Wm);
  if ((long long)Hm * Wm > SC_MAX_HW || (long long)h * w > SC_MAX_HW)
    BX_FAIL(BX_EUNSUPPORTED, "%s: %lld cells per mask, %lld per plane, supported 1..%d", who, (long long)Hm * Wm, (long long)h * w, SC_MAX_HW);
  BX_REQUIRE(sb >= 0 && sc >= 0 && sy >= 0 && sx >= 0, "%s: negative stride (%d, %d, %d, %d)", who, sb, sc, sy, sx);
  const long long last = (long long)(B - 1) * sb + (long long)(C - 1) * sc + (long long)(h - 1) * sy + (long long)(w - 1) * sx;
  BX_REQUIRE(last < (1ll << 31) && (long long)B * C < (1ll << 31), "%s: activation beyond 32-bit offsets (last element %lld)", who, last);
  pl->sb = sb; pl->sc = sc; pl->sy = sy; pl->sx = sx; pl->h = h; pl->w = w; pl->C = C;
  pl->ry = (float)h / (float)Hm; pl->rx = (float)w / (float)Wm;
  (void)A;
  return BX_OK;
}

// ---- the range of every up-sampled plane -------------------------------------------------------------------------------------------------
// Level 1: workgroup (plane, chunk) takes min and max over its 4096 up-sampled values (a small plane is staged in LDS first; the
// chunks of a large one read it through the cache) and writes one pair.  Level 2: one thread per plane folds the pairs.  min and max
// do not depend on the order, so no atomics and no ordering are needed for identical bits.
template <typename TA, bool STAGED>
__global__ __launch_bounds__(256) void k_sc_range(const TA* __restrict__ A, ScPlane pl, int Hm, int Wm, int HW, int nchunk, float* __restrict__ part) {
  __shared__ float src[STAGED ? SC_RANGE_PLANE : 1];
  __shared__ float red[2][4];
  const int bk = blockIdx.x, b = bk / pl.C, k = bk - b * pl.C;
  const int base = b * pl.sb + k * pl.sc;
  if (STAGED) {
    for (int i = threadIdx.x; i < pl.h * pl.w; i += 256) {
      const int y = i / pl.w, x = i - y * pl.w;
      src[i] = ldf(A, (size_t)(base + y * pl.sy + x * pl.sx));
    }
    __syncthreads();
  }
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll 4
  for (int u = 0; u < SC_RANGE_PER; ++u) {
    const int p = blockIdx.y * (256 * SC_RANGE_PER) + u * 256 + threadIdx.x;
    const int pc = p < HW ? p : HW - 1;                               // past the end: the last value again, which moves neither extreme
    const int oy = pc / Wm, ox = pc - oy * Wm;
    int y0, y1, x0, x1; float ly, lx;
    bilinear_src(oy, pl.ry, pl.h, y0, y1, ly);
    bilinear_src(ox, pl.rx, pl.w, x0, x1, lx);
    float a00, a01, a10, a11;
    if (STAGED) {
      a00 = src[y0 * pl.w + x0]; a01 = src[y0 * pl.w + x1]; a10 = src[y1 * pl.w + x0]; a11 = src[y1 * pl.w + x1];
    } else {
      a00 = ldf(A, (size_t)(base + y0 * pl.sy + x0 * pl.sx)); a01 = ldf(A, (size_t)(base + y0 * pl.sy + x1 * pl.sx));
      a10 = ldf(A, (size_t)(base + y1 * pl.sy + x0 * pl.sx)); a11 = ldf(A, (size_t)(base + y1 * pl.sy + x1 * pl.sx));
    }
    const float v = sc_blend(a00, a01, a10, a11, ly, lx);
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  lo = sc_wave_min(lo); hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((size_t)bk * nchunk + blockIdx.y) * 2] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    part[((size_t)bk * nchunk + blockIdx.y) * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}
__global__ __launch_bounds__(256) void k_sc_range_fold(const float* __restrict__ part, int nchunk, int BC, float* __restrict__ lo, float* __restrict__ hi,
                                                       float* __restrict__ scale) {
  const int bk = blockIdx.x * 256 + threadIdx.x;
  if (bk >= BC) return;
  float l = INFINITY, h = -INFINITY;
  for (int c = 0; c < nchunk; ++c) { l = fminf(l, part[((size_t)bk * nchunk + c) * 2]); h = fmaxf(h, part[((size_t)bk * nchunk + c) * 2 + 1]); }
  l += 0.f; h += 0.f;                                                 // a zero extreme is +0.0 whichever zero the scan met first
  lo[bk] = l; hi[bk] = h;
  scale[bk] = h > l ? 1.f / (h - l) : 0.f;
}
static int sc_range_chunks(int Hm, int Wm) { return bx_ceil_div((long long)Hm * Wm, 256 * SC_RANGE_PER); }
extern "C" size_t bx_scorecam_range_workspace(int B, int C, int Hm, int Wm) {
  if (B <= 0 || C <= 0 || Hm <= 0 || Wm <= 0 || (long long)Hm * Wm > SC_MAX_HW || (long long)B * C >= (1ll << 31)) return 0;
  return (size_t)B * C * sc_range_chunks(Hm, Wm) * 2 * sizeof(float);
}
extern "C" int bx_scorecam_range(const void* A, int dtype, int sb, int sc, int sy, int sx, int B, int C, int h, int w, int Hm, int Wm, float* lo,
                                 float* hi, float* scale, void* workspace, size_t workspace_bytes, bxStream stream) {
  ScPlane pl;
  const int rc = sc_plane_ok("bx_scorecam_range", A, dtype, sb, sc, sy, sx, B, C, h, w, Hm, Wm, &pl);
  if (rc) return rc;
  const int nchunk = sc_range_chunks(Hm, Wm);
  BX_REQUIRE((unsigned long long)B * C * nchunk * 8 < (1ull << 32), "bx_scorecam_range: B * C * chunks = %lld pairs beyond 32-bit byte offsets",
             (long long)B * C * nchunk);
  BX_REQUIRE(A && lo && hi && scale && workspace, "bx_scorecam_range: null pointer");
  BX_REQUIRE(workspace_bytes >= bx_scorecam_range_workspace(B, C, Hm, Wm), "bx_scorecam_range: workspace of %zu bytes, needs %zu", workspace_bytes,
             bx_scorecam_range_workspace(B, C, Hm, Wm));
  float* part = (float*)workspace;
  const dim3 grid(B * C, nchunk);
  const bool staged = h * w <= SC_RANGE_PLANE;
  BX_DISPATCH_DTYPE(dtype, TA, {
    if (staged) hipLaunchKernelGGL((k_sc_range<TA, true>), grid, dim3(256), 0, (hipStream_t)stream, (const TA*)A, pl, Hm, Wm, Hm * Wm, nchunk, part);
    else hipLaunchKernelGGL((k_sc_range<TA, false>), grid, dim3(256), 0, (hipStream_t)stream, (const TA*)A, pl, Hm, Wm, Hm * Wm, nchunk, part);
  });
  BX_CHECK_LAUNCH("bx_scorecam_range");
  hipLaunchKernelGGL(k_sc_range_fold, dim3(bx_ceil_div((long long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, part, nchunk, B * C, lo, hi, scale);
  BX_CHECK_LAUNCH("bx_scorecam_range");
  return BX_OK;
}

// ---- perturbed batches ------------------------------------------------------------------------------------------------------------------
// base + m * (x - base), the mask value m of channel k of A shared by the input channels of a pixel (the kernels are perturb_rows.h's).
// A pixel's two source coordinates are taken once for the PERTURB_SPW rows of a group.  The group's planes are staged in LDS when each
// holds at most SC_PLANE values (the late stages: 2 x 4 ... 16 x 32); larger planes are as large as the image or half of it, every value
// is used by one to four pixels, and they are read through the cache.  With channel stride 1 (NHWC) the PERTURB_SPW channels of a
// position are adjacent in memory and the fill walks them fastest; otherwise it walks the positions of a plane fastest.
template <typename TA, bool STAGED>
struct ScMask {
  struct Lds { float src[STAGED ? PERTURB_SPW * SC_PLANE_LD : 1]; };
  struct Cell { int o00, o01, o10, o11; float ly, lx; };
  const TA* A;
  ScPlane pl;
  const float* lo;
  const float* scale;
  int k0;
  __device__ __forceinline__ void stage(Lds& lds, int b, int j0, int n) const {
    if (!STAGED) return;
    const int abase = b * pl.sb, hw = pl.h * pl.w;
    for (int i = threadIdx.x; i < PERTURB_SPW * hw; i += 256) {
      int j, s;
      if (pl.sc == 1) { s = i / PERTURB_SPW; j = i - s * PERTURB_SPW; }
      else { j = i / hw; s = i - j * hw; }
      const int kk = k0 + (j0 + j < n ? j0 + j : n - 1);              // rows past the window repeat its last channel and are not written
      const int y = s / pl.w, xx = s - y * pl.w;
      lds.src[j * SC_PLANE_LD + s] = ldf(A, (size_t)(abase + kk * pl.sc + y * pl.sy + xx * pl.sx));
    }
    __syncthreads();
  }
  __device__ __forceinline__ Cell cell(int, int, int oy, int ox) const {
    Cell c;
    int y0, y1, x0, x1;
    bilinear_src(oy, pl.ry, pl.h, y0, y1, c.ly);
    bilinear_src(ox, pl.rx, pl.w, x0, x1, c.lx);
    c.o00 = STAGED ? y0 * pl.w + x0 : y0 * pl.sy + x0 * pl.sx; c.o01 = STAGED ? y0 * pl.w + x1 : y0 * pl.sy + x1 * pl.sx;
    c.o10 = STAGED ? y1 * pl.w + x0 : y1 * pl.sy + x0 * pl.sx; c.o11 = STAGED ? y1 * pl.w + x1 : y1 * pl.sy + x1 * pl.sx;
    return c;
  }
  __device__ __forceinline__ float row(const Lds& lds, const Cell& c, int b, int j0, int sj) const {
    const int kk = k0 + j0 + sj;
    const float l = lo[(size_t)b * pl.C + kk], sc = scale[(size_t)b * pl.C + kk];      // wave-uniform
    float a00, a01, a10, a11;
    if (STAGED) {
      const float* s = lds.src + sj * SC_PLANE_LD;
      a00 = s[c.o00]; a01 = s[c.o01]; a10 = s[c.o10]; a11 = s[c.o11];
    } else {
      const size_t kb = (size_t)(b * pl.sb + kk * pl.sc);
      a00 = ldf(A, kb + c.o00); a01 = ldf(A, kb + c.o01); a10 = ldf(A, kb + c.o10); a11 = ldf(A, kb + c.o11);
    }
    return fminf((sc_blend(a00, a01, a10, a11, c.ly, c.lx) - l) * sc, 1.f);
  }
};
static int sc_window_ok(const char* who, int B, int C, int b0, int nb, int k0, int n, int kind) {
  BX_REQUIRE(b0 >= 0 && nb >= 1 && (long long)b0 + nb <= B, "%s: samples b0 = %d, nb = %d outside 0..B = %d", who, b0, nb, B);
  BX_REQUIRE(k0 >= 0 && n >= 1 && (long long)k0 + n <= C, "%s: channels k0 = %d, n = %d outside 0..C = %d", who, k0, n, C);
  BX_REQUIRE(kind >= 0 && kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel, 2 full tensor)", who, kind);
  return BX_OK;
}
extern "C" int bx_scorecam_perturb_spec(const float* x, const void* A, int dtype_a, int sb, int sc, int sy, int sx, int C, int h, int w, const float* lo,
                                        const float* scale, const float* baseline, int baseline_kind, void* out, int B, int Cin, int H, int W, int Cp,
                                        int b0, int nb, int k0, int n, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  ScPlane pl;
  int rc = sc_plane_ok("bx_scorecam_perturb_spec", A, dtype_a, sb, sc, sy, sx, B, C, h, w, H, W, &pl);
  if (rc) return rc;
  if ((rc = sc_window_ok("bx_scorecam_perturb_spec", B, C, b0, nb, k0, n, baseline_kind)) != BX_OK) return rc;
  if ((rc = perturb_layout_ok("bx_scorecam_perturb_spec", "input channels", Cin, Cp)) != BX_OK) return rc;
  BX_REQUIRE((long long)B * Cin * H * W < (1ll << 31), "bx_scorecam_perturb_spec: input beyond 32-bit offsets");
  if ((rc = perturb_rows_ok("bx_scorecam_perturb_spec", "nb", nb, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && A && lo && scale && baseline && out, "bx_scorecam_perturb_spec: null pointer");
  const bool staged = h * w <= SC_PLANE;
  BX_DISPATCH_DTYPE(dtype, T, BX_DISPATCH_DTYPE(dtype_a, TA, {
    if (staged) perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, nb, Cin, H, W, b0, n, ScMask<TA, true>{(const TA*)A, pl, lo, scale, k0});
    else perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, nb, Cin, H, W, b0, n, ScMask<TA, false>{(const TA*)A, pl, lo, scale, k0});
  }));
  BX_CHECK_LAUNCH("bx_scorecam_perturb_spec");
  return BX_OK;
}

// EEG: the plane is one row of w values (h = 1) and the mask value of column t serves every electrode.  A row of T or T/4 values is
// read where it is needed: consecutive lanes read consecutive values, and the Chans threads of a column share them through the cache.
// The vertical blend of the definition is kept although both of its rows are the plane's only row.
template <typename TA>
struct ScMaskEeg {
  struct Lds {};
  struct Cell { int o0, o1; float ly, lx; };
  const TA* A;
  ScPlane pl;
  const float* lo;
  const float* scale;
  int k0;
  __device__ __forceinline__ void stage(Lds&, int, int, int) const {}
  __device__ __forceinline__ Cell cell(int, int, int, int t) const {
    Cell c;
    int y0, y1, x0, x1;
    bilinear_src(0, pl.ry, 1, y0, y1, c.ly);
    bilinear_src(t, pl.rx, pl.w, x0, x1, c.lx);
    c.o0 = x0 * pl.sx; c.o1 = x1 * pl.sx;
    return c;
  }
  __device__ __forceinline__ float row(const Lds&, const Cell& c, int b, int j0, int sj) const {
    const int kk = k0 + j0 + sj;
    const float l = lo[(size_t)b * pl.C + kk], sc = scale[(size_t)b * pl.C + kk];      // wave-uniform
    const size_t kb = (size_t)(b * pl.sb + kk * pl.sc);
    const float a0 = ldf(A, kb + c.o0), a1 = ldf(A, kb + c.o1);
    return fminf((sc_blend(a0, a1, a0, a1, c.ly, c.lx) - l) * sc, 1.f);
  }
};
extern "C" int bx_scorecam_perturb_eeg(const float* x, const void* A, int dtype_a, int sb, int sc, int sx, int C, int w, const float* lo,
                                       const float* scale, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int b0,
                                       int nb, int k0, int n, bxStream stream) {
  BX_REQUIRE(Chans > 0 && T > 0 && (long long)Chans * T * (B > 0 ? B : 1) < (1ll << 31), "bx_scorecam_perturb_eeg: bad shape B=%d Chans=%d T=%d", B, Chans, T);
  ScPlane pl;
  int rc = sc_plane_ok("bx_scorecam_perturb_eeg", A, dtype_a, sb, sc, 0, sx, B, C, 1, w, 1, T, &pl);
  if (rc) return rc;
  if ((rc = sc_window_ok("bx_scorecam_perturb_eeg", B, C, b0, nb, k0, n, baseline_kind)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_scorecam_perturb_eeg", "nb", nb, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && A && lo && scale && baseline && out, "bx_scorecam_perturb_eeg: null pointer");
  BX_DISPATCH_DTYPE(dtype_a, TA, perturb_launch_eeg(stream, x, baseline, baseline_kind, out, nb, Chans, T, 1, b0, n,
                                                    ScMaskEeg<TA>{(const TA*)A, pl, lo, scale, k0}));
  BX_CHECK_LAUNCH("bx_scorecam_perturb_eeg");
  return BX_OK;
}

// ---- the map ----------------------------------------------------------------------------------------------------------------------------
// A thread owns one position s of one map (sample b, class c); it walks the channels in index order and adds (double)w_k * (double)A
// to its fp64 register (the product of two fp32 values is exact in fp64).  w_k depends on the workgroup and the loop counter alone, so
// its loads are wave-uniform.  No atomics: the bits of the result are a function of the inputs alone.  One rounding to fp32.
__device__ __forceinline__ float sc_weight(const float* __restrict__ P, const unsigned char* __restrict__ valid, size_t bk, int K, int c, int mode, float pb) {
  const float pk = P[bk * K + c];
  return valid[bk] ? (mode == BX_SCORECAM_INCREASE ? pk - pb : pk) : 0.f;
}
template <typename TA>
__global__ __launch_bounds__(256) void k_sc_combine(const float* __restrict__ P, const float* __restrict__ Pbase, const int* __restrict__ classes,
                                                    const unsigned char* __restrict__ valid, const TA* __restrict__ A, ScPlane pl, float* __restrict__ raw,
                                                    float* __restrict__ cam, float* __restrict__ wts, int K, int nm, int mode, int relu) {
  const int q = blockIdx.x, b = q / nm, hw = pl.h * pl.w;
  int c = q - b * nm;
  if (classes) { c = classes[b]; c = c < 0 ? 0 : (c >= K ? K - 1 : c); }
  const float pb = mode == BX_SCORECAM_INCREASE ? Pbase[(size_t)b * K + c] : 0.f;
  const int s = blockIdx.y * 256 + threadIdx.x, sc = s < hw ? s : hw - 1;
  const int y = sc / pl.w, xx = sc - y * pl.w;
  const size_t off = (size_t)(b * pl.sb + y * pl.sy + xx * pl.sx);
  double acc = 0.0;
  for (int k = 0; k < pl.C; ++k)
    acc += (double)sc_weight(P, valid, (size_t)b * pl.C + k, K, c, mode, pb) * (double)ldf(A, off + (size_t)k * pl.sc);
  if (s < hw) {
    const float r = (float)acc;
    if (raw) raw[(size_t)q * hw + s] = r;
    if (cam) cam[(size_t)q * hw + s] = relu ? fmaxf(r, 0.f) : r;
  }
  if (blockIdx.y == 0 && wts)
    for (int k = threadIdx.x; k < pl.C; k += 256) wts[(size_t)q * pl.C + k] = sc_weight(P, valid, (size_t)b * pl.C + k, K, c, mode, pb);
}
extern "C" int bx_scorecam_combine(const float* P, const float* P_base, const int* classes, const unsigned char* valid, const void* A, int dtype_a, int sb,
                                   int sc, int sy, int sx, int B, int C, int h, int w, int K, int weight_mode, int relu, float* raw, float* cam,
                                   float* weights, bxStream stream) {
  ScPlane pl;
  const int rc = sc_plane_ok("bx_scorecam_combine", A, dtype_a, sb, sc, sy, sx, B, C, h, w, h, w, &pl);
  if (rc) return rc;
  BX_REQUIRE(K >= 1, "bx_scorecam_combine: bad shape K=%d", K);
  if (K > SC_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_scorecam_combine: %d classes, supported 1..%d", K, SC_MAX_K);
  BX_REQUIRE(weight_mode == BX_SCORECAM_PROB || weight_mode == BX_SCORECAM_INCREASE, "bx_scorecam_combine: weight_mode %d (0 prob, 1 increase)", weight_mode);
  const int nm = classes ? 1 : K;
  BX_REQUIRE((long long)B * C * K < (1ll << 31) && (long long)B * nm * h * w < (1ll << 31) && (long long)B * nm * C < (1ll << 31),
             "bx_scorecam_combine: B * C * K, B * maps * h * w or B * maps * C beyond 32-bit offsets");
  BX_REQUIRE(P && valid && A && (raw || cam) && weights && (weight_mode == BX_SCORECAM_PROB || P_base), "bx_scorecam_combine: null pointer");
  const dim3 grid(B * nm, bx_ceil_div((long long)h * w, 256));
  BX_DISPATCH_DTYPE(dtype_a, TA, hipLaunchKernelGGL((k_sc_combine<TA>), grid, dim3(256), 0, (hipStream_t)stream, P, P_base, classes, valid, (const TA*)A, pl,
                                                    raw, cam, weights, K, nm, weight_mode, relu));
  BX_CHECK_LAUNCH("bx_scorecam_combine");
  return BX_OK;
}
