// TracIn (Pruthi et al., NeurIPS 2020; Captum's influence.TracInCPFast): the influence of training examples on test examples through the
// model's four Linear layers, whose per-example gradients are outer products delta (x) a -- so a gradient dot product is
// (delta_i . delta_j)(a_i . a_j + 1) and no per-example backward pass runs.  The factors delta in closed form (bx_tracin_factors), the
// pairwise sum of a block of training rows against all test rows (bx_tracin_scores), the self-influence (bx_tracin_self) and an exact
// top-k per test column (bx_tracin_topk).  See include/brainxai.h for the definition and the contract of each entry point.
// No floating-point atomics; every sum is sequential in ascending index.  Built with -ffp-contract=off: a * b + c below is two roundings.
#include "bx_common.h"
#include <math.h>

#define TI_MAX_K 32                    // classes
#define TI_MAX_HD 256                  // hidden units
#define TI_MAX_DW 256                  // width of a layer's delta
#define TI_MAX_AW 4096                 // width of a layer's activation
#define TI_MAX_M 4096                  // test rows
#define TI_MAX_BLOCK 65536             // training rows of a launch
#define TI_MAX_TOP 256
#define TI_TILE 64                     // rows of a tile, each side
#define TI_DC 32                       // features of a chunk in LDS
#define TI_SELF_ACT (4096 + 1024 + 256 + 64)
#define TI_SELF_DELTA (TI_MAX_K * 3 + TI_MAX_HD)

// ---- exp and log as fixed sequences of fp64 operations (include/brainxai.h restates them; tests/tracin_ref.py does in numpy) ----------
#define TI_LOG2E 1.4426950408889634
#define TI_LN2_HI 0.6931471803691238
#define TI_LN2_LO 1.9082149292705877e-10
__device__ __forceinline__ double ti_exp(double x) {
  if (x != x) return x;
  if (x < -708.0) return 0.0;
  if (x > 709.0) return INFINITY;
  const double n = rint(x * TI_LOG2E);
  const double r = (x - n * TI_LN2_HI) - n * TI_LN2_LO;
  const double c[14] = {1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
                        0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
                        2.08767569878681e-09, 1.6059043836821613e-10};
  double p = c[13];
#pragma unroll
  for (int i = 12; i >= 0; --i) p = p * r + c[i];
  return ldexp(p, (int)n);
}
// x > 0 and finite (an fp32 value, so never a denormal double)
__device__ __forceinline__ double ti_log(double x) {
  int e;
  double m = frexp(x, &e);
  if (m < 0.7071067811865476) { m = m * 2.0; e -= 1; }
  const double f = m - 1.0, s = f / (2.0 + f), z = s * s;
  const double c[11] = {0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091, 0.07692307692307693,
                        0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616, 0.043478260869565216};
  double p = c[10];
#pragma unroll
  for (int i = 9; i >= 0; --i) p = p * z + c[i];
  const double t = 2.0 * s, de = (double)e;
  return de * TI_LN2_HI + ((t + t * (z * p)) + de * TI_LN2_LO);
}

// ---- the factors: one workgroup per row -------------------------------------------------------------------------------------------------
// Thread k owns class k, thread h hidden unit h, thread m input m of fc1; a sum is one thread's loop in ascending index.
__global__ __launch_bounds__(256) void k_tracin_factors(const float* __restrict__ logp, const float* __restrict__ target, const int* __restrict__ labels,
                                                        const float* __restrict__ hidden, const float* __restrict__ eeg_logp,
                                                        const float* __restrict__ spec_logp, const float* __restrict__ w1, const float* __restrict__ w2,
                                                        double* __restrict__ delta, double* __restrict__ loss, int* __restrict__ status, int K, int Hd,
                                                        int mode) {
  __shared__ double s_t[TI_MAX_K], s_lp[TI_MAX_K], s_d2[TI_MAX_K], s_pe[TI_MAX_K], s_ps[TI_MAX_K], s_d1[TI_MAX_HD], s_v[2 * TI_MAX_K];
  __shared__ double s_T;
  __shared__ int s_bad[2];                                           // [0] a non-finite value, [1] a bad target
  const int tid = threadIdx.x, r = blockIdx.x;
  const bool multi = mode == BX_TRACIN_MULTIMODAL;
  const int LD = multi ? 3 * K + Hd : K;
  double* out = delta + (size_t)r * LD;
  if (tid < 2) s_bad[tid] = 0;
  __syncthreads();
  if (tid < K) {
    const double lp = (double)logp[(size_t)r * K + tid];
    double t;
    if (target) t = (double)target[(size_t)r * K + tid];
    else t = labels[r] == tid ? 1.0 : 0.0;
    s_lp[tid] = lp;
    s_t[tid] = t;
    if (!isfinite(lp) || !isfinite(t)) s_bad[0] = 1;
    if (t < 0.0) s_bad[1] = 1;
    if (multi) {
      const double e = (double)eeg_logp[(size_t)r * K + tid], s = (double)spec_logp[(size_t)r * K + tid];
      if (!isfinite(e) || !isfinite(s)) s_bad[0] = 1;
      s_pe[tid] = ti_exp(e);
      s_ps[tid] = ti_exp(s);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double T = 0.0;
    for (int k = 0; k < K; ++k) T += s_t[k];
    s_T = T;
    if (T <= 0.0) s_bad[1] = 1;
    if (!target && (labels[r] < 0 || labels[r] >= K)) s_bad[1] = 1;
    double l = 0.0;
    if (!s_bad[0] && !s_bad[1])
      for (int k = 0; k < K; ++k)
        if (s_t[k] > 0.0) l += s_t[k] * (ti_log(s_t[k]) - s_lp[k]);
    loss[r] = l;
    if (!isfinite(l)) s_bad[0] = 1;
  }
  __syncthreads();
  if (tid < K) {
    const double d = s_T * ti_exp(s_lp[tid]) - s_t[tid];
    s_d2[tid] = d;
    out[tid] = d;
    if (!isfinite(d)) s_bad[0] = 1;
  }
  if (multi) {
    __syncthreads();
    if (tid < Hd) {
      double u = 0.0;
      for (int k = 0; k < K; ++k) u += (double)w2[(size_t)k * Hd + tid] * s_d2[k];
      const float h = hidden[(size_t)r * Hd + tid];
      const double d = h > 0.f ? u : 0.0;
      s_d1[tid] = d;
      out[K + tid] = d;
      if (!isfinite(d) || !isfinite(h)) s_bad[0] = 1;
    }
    __syncthreads();
    if (tid < 2 * K) {
      double v = 0.0;
      for (int h = 0; h < Hd; ++h) v += (double)w1[(size_t)h * 2 * K + tid] * s_d1[h];
      s_v[tid] = v;
    }
    __syncthreads();
    if (tid < 2 * K) {
      const int half = tid >= K ? K : 0, k = tid - half;
      double sv = 0.0;
      for (int m = 0; m < K; ++m) sv += s_v[half + m];
      const double d = s_v[tid] - (half ? s_ps[k] : s_pe[k]) * sv;
      out[K + Hd + tid] = d;                                         // delta_e at K + Hd, delta_s at 2K + Hd
      if (!isfinite(d)) s_bad[0] = 1;
    }
  }
  __syncthreads();
  if (tid == 0) status[r] = s_bad[1] ? BX_TRACIN_BAD_TARGET : (s_bad[0] ? BX_TRACIN_NONFINITE : BX_TRACIN_OK);
}

extern "C" int bx_tracin_factors(const float* logp, const float* target, const int* labels, const float* hidden, const float* eeg_logp,
                                 const float* spec_logp, const float* w1, const float* w2, double* delta, double* loss, int* status, int rows, int K,
                                 int Hd, int mode, bxStream stream) {
  BX_REQUIRE(mode == BX_TRACIN_MULTIMODAL || mode == BX_TRACIN_SINGLE, "bx_tracin_factors: mode %d (0 multimodal, 1 single layer)", mode);
  BX_REQUIRE(rows >= 1 && K >= 1, "bx_tracin_factors: bad shape rows=%d K=%d", rows, K);
  if (K > TI_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_factors: %d classes, supported 1..%d", K, TI_MAX_K);
  if (mode == BX_TRACIN_MULTIMODAL) {
    BX_REQUIRE(Hd >= 1, "bx_tracin_factors: bad shape Hd=%d", Hd);
    if (Hd > TI_MAX_HD) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_factors: %d hidden units, supported 1..%d", Hd, TI_MAX_HD);
    BX_REQUIRE(hidden && eeg_logp && spec_logp && w1 && w2, "bx_tracin_factors: null pointer");
  }
  BX_REQUIRE(logp && delta && loss && status, "bx_tracin_factors: null pointer");
  BX_REQUIRE((target != nullptr) != (labels != nullptr), "bx_tracin_factors: give the targets or the labels, one of the two");
  hipLaunchKernelGGL(k_tracin_factors, dim3(rows), dim3(256), 0, (hipStream_t)stream, logp, target, labels, hidden, eeg_logp, spec_logp, w1, w2, delta, loss,
                     status, K, Hd, mode);
  BX_CHECK_LAUNCH("bx_tracin_factors");
  return BX_OK;
}

// ---- shapes shared by scores and self ---------------------------------------------------------------------------------------------------
static int ti_shape_ok(const char* who, const bxTracinShape* sh, int mask, int* ld) {
  BX_REQUIRE(sh, "%s: null shape", who);
  BX_REQUIRE(sh->layers >= 1 && sh->layers <= 4, "%s: %d layers, 1..4", who, sh->layers);
  BX_REQUIRE(mask > 0 && mask < (1 << sh->layers), "%s: layer mask %d selects nothing, or a layer beyond the %d there are", who, mask, sh->layers);
  int sum = 0;
  for (int l = 0; l < sh->layers; ++l) {
    BX_REQUIRE(sh->dwidth[l] >= 1 && sh->awidth[l] >= 1, "%s: layer %d has widths %d / %d", who, l, sh->dwidth[l], sh->awidth[l]);
    if (sh->dwidth[l] > TI_MAX_DW) BX_FAIL(BX_EUNSUPPORTED, "%s: layer %d has %d outputs, supported 1..%d", who, l, sh->dwidth[l], TI_MAX_DW);
    if (sh->awidth[l] > TI_MAX_AW) BX_FAIL(BX_EUNSUPPORTED, "%s: layer %d has %d inputs, supported 1..%d", who, l, sh->awidth[l], TI_MAX_AW);
    sum += sh->dwidth[l];
  }
  *ld = sum;
  return BX_OK;
}
static int ti_side_ok(const char* who, const bxTracinSide* s, const bxTracinShape* sh, int mask) {
  BX_REQUIRE(s && s->delta, "%s: null pointer", who);
  for (int l = 0; l < sh->layers; ++l)
    if (mask >> l & 1) BX_REQUIRE(s->act[l], "%s: layer %d is selected and has no activations", who, l);
  return BX_OK;
}

// ---- S[row0 + i, j] (+)= eta sum_l (delta_i . delta_j)(a_i . a_j + 1) --------------------------------------------------------------------
// A workgroup owns a 64 x 64 tile of (train, test) pairs, a thread 4 x 4 of them (k_tcav_gram's scheme).  A chunk of 32 features of the
// tile's 64 + 64 rows is staged in LDS feature-major as fp64, so that a thread's four row values are one 32-byte read shared by the 16
// threads of its row group (a broadcast).  Every pair's running sum stays in its thread's registers through all features of a layer.
template <typename T>
__device__ __forceinline__ void ti_tile_dot(const T* __restrict__ A, int lda, int rowsA, int ra0, const T* __restrict__ B, int ldb, int rowsB, int rb0, int W,
                                            double (*As)[TI_TILE + 2], double (*Bs)[TI_TILE + 2], double (&acc)[4][4]) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid >> 5, ld = tid & 31;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int c0 = 0; c0 < W; c0 += TI_DC) {
    __syncthreads();
    const int d = c0 + ld;
    const bool dok = d < W;
    T va[8], vb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                        // unconditional (clamped) loads: all in flight together
      const int gi = ra0 + lr + 8 * k, gj = rb0 + lr + 8 * k;
      va[k] = A[(size_t)(gi < rowsA ? gi : 0) * lda + (dok ? d : 0)];
      vb[k] = B[(size_t)(gj < rowsB ? gj : 0) * ldb + (dok ? d : 0)];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = lr + 8 * k;
      As[ld][r] = dok && ra0 + r < rowsA ? (double)va[k] : 0.0;
      Bs[ld][r] = dok && rb0 + r < rowsB ? (double)vb[k] : 0.0;
    }
    __syncthreads();
    const int cnt = W - c0 < TI_DC ? W - c0 : TI_DC;
#pragma unroll 4
    for (int dd = 0; dd < cnt; ++dd) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = As[dd][ty * 4 + u]; b[u] = Bs[dd][tx * 4 + u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
    }
  }
}

__global__ __launch_bounds__(256) void k_tracin_scores(bxTracinSide train, bxTracinSide test, bxTracinShape sh, int ld, double* __restrict__ S, int M, int row0,
                                                       double eta, int store, int mask) {
  __shared__ __attribute__((aligned(16))) double As[TI_DC][TI_TILE + 2];
  __shared__ __attribute__((aligned(16))) double Bs[TI_DC][TI_TILE + 2];
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, ra0 = blockIdx.y * TI_TILE, rb0 = blockIdx.x * TI_TILE;
  double total[4][4], dd[4][4], aa[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) total[u][v] = 0.0;
  int off = 0;
  for (int l = 0; l < sh.layers; ++l) {
    if (mask >> l & 1) {
      ti_tile_dot<double>(train.delta + off, ld, train.rows, ra0, test.delta + off, ld, test.rows, rb0, sh.dwidth[l], As, Bs, dd);
      ti_tile_dot<float>(train.act[l], sh.awidth[l], train.rows, ra0, test.act[l], sh.awidth[l], test.rows, rb0, sh.awidth[l], As, Bs, aa);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) total[u][v] += dd[u][v] * (aa[u][v] + 1.0);
    }
    off += sh.dwidth[l];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = ra0 + ty * 4 + u;
    if (i >= train.rows) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = rb0 + tx * 4 + v;
      if (j >= M) continue;
      double* p = S + (size_t)(row0 + i) * M + j;
      const double t = eta * total[u][v];
      *p = store ? t : *p + t;
    }
  }
}

extern "C" int bx_tracin_scores(const bxTracinSide* train, const bxTracinSide* test, const bxTracinShape* shape, double* S, int N, int row0, double eta,
                                int store, int layer_mask, bxStream stream) {
  int ld = 0;
  int rc = ti_shape_ok("bx_tracin_scores", shape, layer_mask, &ld);
  if (rc) return rc;
  BX_REQUIRE(train && test, "bx_tracin_scores: null pointer");
  const int M = test->rows, rows = train->rows;
  BX_REQUIRE(M >= 1 && rows >= 1 && N >= 1, "bx_tracin_scores: bad shape rows=%d M=%d N=%d", rows, M, N);
  if (M > TI_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_scores: %d test rows, supported 1..%d", M, TI_MAX_M);
  if (rows > TI_MAX_BLOCK) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_scores: %d training rows in a block, supported 1..%d", rows, TI_MAX_BLOCK);
  if ((long long)N * M >= (1ll << 31)) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_scores: N * M = %lld, supported below 2^31", (long long)N * M);
  BX_REQUIRE(row0 >= 0 && (long long)row0 + rows <= N, "bx_tracin_scores: rows %d..%d outside 0..%d", row0, row0 + rows, N);
  BX_REQUIRE(eta == eta && eta - eta == 0.0, "bx_tracin_scores: eta = %g is not a finite number", eta);
  if ((rc = ti_side_ok("bx_tracin_scores", train, shape, layer_mask))) return rc;
  if ((rc = ti_side_ok("bx_tracin_scores", test, shape, layer_mask))) return rc;
  BX_REQUIRE(S, "bx_tracin_scores: null pointer");
  hipLaunchKernelGGL(k_tracin_scores, dim3(bx_ceil_div(M, TI_TILE), bx_ceil_div(rows, TI_TILE)), dim3(256), 0, (hipStream_t)stream, *train, *test, *shape, ld, S,
                     M, row0, eta, store ? 1 : 0, layer_mask);
  BX_CHECK_LAUNCH("bx_tracin_scores");
  return BX_OK;
}

// ---- self[row0 + i] (+)= eta sum_l |delta_i|^2 (|a_i|^2 + 1): one workgroup per row ---------------------------------------------------------
// The row's factors and activations are staged in LDS with coalesced loads; thread 2l sums layer l's delta, thread 2l + 1 its
// activations, each sequentially in ascending index (the order of bx_tracin_scores), thread 0 folds the layers.
__global__ __launch_bounds__(256) void k_tracin_self(bxTracinSide side, bxTracinShape sh, int ld, double* __restrict__ out, int row0, double eta, int store,
                                                     int mask) {
  __shared__ double sd[TI_SELF_DELTA];
  __shared__ float sa[TI_SELF_ACT];
  __shared__ double sums[8];
  const int tid = threadIdx.x, r = blockIdx.x;
  for (int i = tid; i < ld; i += 256) sd[i] = side.delta[(size_t)r * ld + i];
  int aoff = 0;
  for (int l = 0; l < sh.layers; ++l) {
    if (mask >> l & 1)
      for (int i = tid; i < sh.awidth[l]; i += 256) sa[aoff + i] = side.act[l][(size_t)r * sh.awidth[l] + i];
    aoff += sh.awidth[l];
  }
  __syncthreads();
  if (tid < 2 * sh.layers && (mask >> (tid >> 1) & 1)) {
    const int l = tid >> 1;
    int doff = 0, ao = 0;
    for (int q = 0; q < l; ++q) { doff += sh.dwidth[q]; ao += sh.awidth[q]; }
    double s = 0.0;
    if (tid & 1) {
      const int W = sh.awidth[l];
#pragma unroll 8
      for (int i = 0; i < W; ++i) { const double a = (double)sa[ao + i]; s += a * a; }
    } else {
      const int W = sh.dwidth[l];
      for (int i = 0; i < W; ++i) { const double d = sd[doff + i]; s += d * d; }
    }
    sums[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int l = 0; l < sh.layers; ++l)
      if (mask >> l & 1) total += sums[2 * l] * (sums[2 * l + 1] + 1.0);
    const double t = eta * total;
    out[row0 + r] = store ? t : out[row0 + r] + t;
  }
}

extern "C" int bx_tracin_self(const bxTracinSide* side, const bxTracinShape* shape, double* self, int N, int row0, double eta, int store, int layer_mask,
                              bxStream stream) {
  int ld = 0;
  int rc = ti_shape_ok("bx_tracin_self", shape, layer_mask, &ld);
  if (rc) return rc;
  BX_REQUIRE(side, "bx_tracin_self: null pointer");
  const int rows = side->rows;
  BX_REQUIRE(rows >= 1 && N >= 1, "bx_tracin_self: bad shape rows=%d N=%d", rows, N);
  if (rows > TI_MAX_BLOCK) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_self: %d rows in a block, supported 1..%d", rows, TI_MAX_BLOCK);
  int asum = 0;
  for (int l = 0; l < shape->layers; ++l) asum += shape->awidth[l];
  if (ld > TI_SELF_DELTA || asum > TI_SELF_ACT)
    BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_self: %d factors and %d activations per row, supported %d and %d", ld, asum, TI_SELF_DELTA, TI_SELF_ACT);
  BX_REQUIRE(row0 >= 0 && (long long)row0 + rows <= N, "bx_tracin_self: rows %d..%d outside 0..%d", row0, row0 + rows, N);
  BX_REQUIRE(eta == eta && eta - eta == 0.0, "bx_tracin_self: eta = %g is not a finite number", eta);
  if ((rc = ti_side_ok("bx_tracin_self", side, shape, layer_mask))) return rc;
  BX_REQUIRE(self, "bx_tracin_self: null pointer");
  hipLaunchKernelGGL(k_tracin_self, dim3(rows), dim3(256), 0, (hipStream_t)stream, *side, *shape, ld, self, row0, eta, store ? 1 : 0, layer_mask);
  BX_CHECK_LAUNCH("bx_tracin_self");
  return BX_OK;
}

// ---- top-k per column: exact radix select over (key, row) ---------------------------------------------------------------------------------
// key: 64 bits whose unsigned order is the wanted rank order of the values (ascending key = better rank), -0.0 as +0.0, NaN last.  The
// keys are written transposed, [M, N], through a 32 x 32 LDS tile, so that the column's workgroup reads them contiguously in each of its
// passes.  The select runs over the 12 bytes (key, row index), most significant first -- all distinct, so ties go to the lower row.
__device__ __forceinline__ uint64_t ti_key(double v, int largest) {
  if (v != v) return ~0ull;
  if (v == 0.0) v = 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  const uint64_t mono = (u >> 63) ? ~u : (u | (1ull << 63));           // ascending value = ascending mono
  return largest ? ~mono : mono;
}

__global__ __launch_bounds__(256) void k_tracin_keys(const double* __restrict__ S, uint64_t* __restrict__ keys, int N, int M, int largest) {
  __shared__ uint64_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, j = j0 + tx;
    if (i < N && j < M) tile[r][tx] = ti_key(S[(size_t)i * M + j], largest);
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + r, i = i0 + tx;
    if (i < N && j < M) keys[(size_t)j * N + i] = tile[tx][r];
  }
}

// the first d of the 12 digits of (key, idx) against those of the prefix (pk, pi): -1 below, 0 equal, 1 above
__device__ __forceinline__ int ti_prefix_cmp(uint64_t key, uint32_t idx, uint64_t pk, uint32_t pi, int d) {
  if (d == 0) return 0;
  const int dk = d < 8 ? d : 8, sk = 64 - 8 * dk;
  const uint64_t a = key >> sk, b = pk >> sk;
  if (a != b) return a < b ? -1 : 1;
  if (d <= 8) return 0;
  const int si = 32 - 8 * (d - 8);
  const uint32_t c = idx >> si, e = pi >> si;
  return c == e ? 0 : (c < e ? -1 : 1);
}
__device__ __forceinline__ unsigned ti_digit(uint64_t key, uint32_t idx, int d) {
  return d < 8 ? (unsigned)(key >> (56 - 8 * d)) & 255u : (idx >> (24 - 8 * (d - 8))) & 255u;
}

__global__ __launch_bounds__(256) void k_tracin_select(const double* __restrict__ S, const uint64_t* __restrict__ keys, int N, int M, int k,
                                                       int* __restrict__ idx, double* __restrict__ val) {
  __shared__ unsigned hist[256];
  __shared__ uint64_t ck[TI_MAX_TOP];
  __shared__ int ci[TI_MAX_TOP];
  __shared__ uint64_t s_pk;
  __shared__ uint32_t s_pi;
  __shared__ unsigned s_kk, s_cnt, s_n;
  const int tid = threadIdx.x, j = blockIdx.x;
  const uint64_t* kj = keys + (size_t)j * N;
  if (tid == 0) { s_pk = 0ull; s_pi = 0u; s_kk = (unsigned)k; s_cnt = (unsigned)N; s_n = 0u; }
  __syncthreads();
  int d = 0;
  while (d < 12 && s_cnt != s_kk) {                                  // uniform: both are read after a barrier
    const uint64_t pk = s_pk;
    const uint32_t pi = s_pi;
    hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < N; i += 256) {
      const uint64_t key = kj[i];
      if (ti_prefix_cmp(key, (uint32_t)i, pk, pi, d) == 0) atomicAdd(&hist[ti_digit(key, (uint32_t)i, d)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0, kk = s_kk;
      for (unsigned b = 0; b < 256; ++b) {
        const unsigned h = hist[b];
        if (cum + h >= kk) {
          s_kk = kk - cum;
          s_cnt = h;
          if (d < 8) s_pk = pk | ((uint64_t)b << (56 - 8 * d));
          else s_pi = pi | (b << (24 - 8 * (d - 8)));
          break;
        }
        cum += h;
      }
    }
    ++d;
    __syncthreads();
  }
  // every row whose first d digits are not above the prefix's is in: exactly k of them
  const uint64_t pk = s_pk;
  const uint32_t pi = s_pi;
  for (int i = tid; i < N; i += 256) {
    const uint64_t key = kj[i];
    if (ti_prefix_cmp(key, (uint32_t)i, pk, pi, d) <= 0) {
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)k) { ck[slot] = key; ci[slot] = i; }
    }
  }
  __syncthreads();
  if (tid < k) {                                                     // rank among the survivors by (key, row): all distinct
    const uint64_t mk = ck[tid];
    const int mi = ci[tid];
    int rank = 0;
    for (int s = 0; s < k; ++s) rank += (ck[s] < mk || (ck[s] == mk && ci[s] < mi)) ? 1 : 0;
    idx[(size_t)j * k + rank] = mi;
    val[(size_t)j * k + rank] = S[(size_t)mi * M + j];
  }
}

static int ti_topk_ok(const char* who, int N, int M) {
  BX_REQUIRE(N >= 1 && M >= 1, "%s: bad shape N=%d M=%d", who, N, M);
  if (M > TI_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "%s: %d columns, supported 1..%d", who, M, TI_MAX_M);
  if ((long long)N * M >= (1ll << 31)) BX_FAIL(BX_EUNSUPPORTED, "%s: N * M = %lld, supported below 2^31", who, (long long)N * M);
  return BX_OK;
}
extern "C" size_t bx_tracin_topk_workspace(int N, int M) {
  if (ti_topk_ok("bx_tracin_topk_workspace", N, M) != BX_OK) return 0;
  return (size_t)N * M * sizeof(uint64_t);
}
extern "C" int bx_tracin_topk(const double* S, int N, int M, int k, int largest, int* idx, double* val, void* workspace, size_t workspace_bytes,
                              bxStream stream) {
  const int rc = ti_topk_ok("bx_tracin_topk", N, M);
  if (rc) return rc;
  BX_REQUIRE(k >= 1, "bx_tracin_topk: k = %d", k);
  if (k > TI_MAX_TOP) BX_FAIL(BX_EUNSUPPORTED, "bx_tracin_topk: k = %d, supported 1..%d", k, TI_MAX_TOP);
  BX_REQUIRE(k <= N, "bx_tracin_topk: k = %d of N = %d rows", k, N);
  BX_REQUIRE(largest == 0 || largest == 1, "bx_tracin_topk: largest = %d (0 or 1)", largest);
  BX_REQUIRE(S && idx && val && workspace, "bx_tracin_topk: null pointer");
  const size_t need = bx_tracin_topk_workspace(N, M);
  if (workspace_bytes < need) BX_FAIL(BX_EWORKSPACE, "bx_tracin_topk: workspace of %zu bytes, need %zu", workspace_bytes, need);
  BX_REQUIRE(((uintptr_t)workspace & 7) == 0, "bx_tracin_topk: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tracin_keys, dim3(bx_ceil_div(N, 32), bx_ceil_div(M, 32)), dim3(256), 0, s, S, (uint64_t*)workspace, N, M, largest);
  hipLaunchKernelGGL(k_tracin_select, dim3(M), dim3(256), 0, s, S, (const uint64_t*)workspace, N, M, k, idx, val);
  BX_CHECK_LAUNCH("bx_tracin_topk");
  return BX_OK;
}
