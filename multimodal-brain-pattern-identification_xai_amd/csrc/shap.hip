// Kernel SHAP (Lundberg & Lee, NeurIPS 2017; paired sampling: Covert & Lee, AISTATS 2021): the rows of an input in which the players of
// a coalition show the input and all others the baseline, straight in the model's layouts; the constrained weighted least-squares fit
// of the Shapley values in fp64; and the per-cell map of the values.  The forward passes between perturb and fit are the model's own
// kernels.  See include/brainxai.h for the definition and the contract of each entry point.
// A row is a selection, not a blend: there is no multiply to contract, so the file needs no flags of its own.
#include "perturb_rows.h"

#define SHAP_MAX_M 256                 // players
#define SHAP_MAX_K 32
#define SHAP_MAX_HW ((1 << 20) - 1)    // cells of a map, the limit of bx_rank_desc: the map drops straight into deletion_insertion

static int shap_domain_ok(const char* who, int Hm, int Wm, int M) {
  BX_REQUIRE(Hm > 0 && Wm > 0, "%s: bad shape Hm=%d Wm=%d", who, Hm, Wm);
  if ((long long)Hm * Wm > SHAP_MAX_HW) BX_FAIL(BX_EUNSUPPORTED, "%s: %lld cells per map, supported 1..%d", who, (long long)Hm * Wm, SHAP_MAX_HW);
  if (M < 2 || M > SHAP_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "%s: %d players, supported 2..%d", who, M, SHAP_MAX_M);
  return BX_OK;
}
static int shap_rows_ok(const char* who, int B, int kind, int M, int N, int n0, int n) {
  BX_REQUIRE(B > 0, "%s: bad shape B=%d", who, B);
  BX_REQUIRE(kind >= 0 && kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel, 2 full tensor)", who, kind);
  BX_REQUIRE(N >= 1 && (long long)N * M < (1ll << 31), "%s: N = %d coalitions of %d players", who, N, M);
  BX_REQUIRE(n0 >= 0 && n >= 1 && (long long)n0 + n <= N, "%s: coalitions n0 = %d, n = %d outside 0..N = %d", who, n0, n, N);
  return BX_OK;
}

// ---- perturbed batches ------------------------------------------------------------------------------------------------------------------
// The PERTURB_SPW coalition rows of a group sit in LDS as bits (8 rows x 8 words); a cell keeps its label; a row costs one LDS read
// and a bit test (the kernels are perturb_rows.h's).  A label outside 0..M-1 counts as player 0 (the driver refuses such maps).
struct ShapMask {
  struct Lds { uint32_t bits[PERTURB_SPW][SHAP_MAX_M / 32]; };
  typedef int Cell;
  const unsigned char* Z;              // [N, M]
  const int* seg;                      // [Hm * Wm]
  int M, n0;
  __device__ __forceinline__ void stage(Lds& lds, int, int j0, int n) const {
    const int tid = threadIdx.x;
    if (tid < PERTURB_SPW * (SHAP_MAX_M / 32)) {
      const int sj = tid / (SHAP_MAX_M / 32), w = tid % (SHAP_MAX_M / 32);
      uint32_t m = 0u;
      if (j0 + sj < n && w * 32 < M) {
        const unsigned char* zr = Z + (size_t)(n0 + j0 + sj) * M;
#pragma unroll
        for (int i = 0; i < 32; ++i) {                // unconditional (clamped) loads: all in flight together
          const int s = w * 32 + i;
          const unsigned char v = zr[s < M ? s : 0];
          if (s < M && v) m |= 1u << i;
        }
      }
      lds.bits[sj][w] = m;
    }
    __syncthreads();
  }
  __device__ __forceinline__ Cell cell(int, int idx, int, int) const {
    const int s = seg[idx];
    return (unsigned)s < (unsigned)M ? s : 0;
  }
  __device__ __forceinline__ bool row(const Lds& lds, const Cell& s, int, int, int sj) const { return (lds.bits[sj][s >> 5] >> (s & 31)) & 1u; }
};

extern "C" int bx_shap_perturb_spec(const float* x, const float* baseline, int baseline_kind, void* out, int B, int C, int H, int W, int Cp,
                                    const int* segments, const unsigned char* Z, int M, int N, int n0, int n, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  int rc = shap_domain_ok("bx_shap_perturb_spec", H, W, M);
  if (rc) return rc;
  if ((rc = shap_rows_ok("bx_shap_perturb_spec", B, baseline_kind, M, N, n0, n)) != BX_OK) return rc;
  if ((rc = perturb_layout_ok("bx_shap_perturb_spec", "channels", C, Cp)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_shap_perturb_spec", "B", B, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && baseline && out && segments && Z, "bx_shap_perturb_spec: null pointer");
  const ShapMask mask = {Z, segments, M, n0};
  BX_DISPATCH_DTYPE(dtype, T, perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, B, C, H, W, 0, n, mask));
  BX_CHECK_LAUNCH("bx_shap_perturb_spec");
  return BX_OK;
}

// map_rows = Chans: the cell of element (ch, t) is (ch, t); map_rows = 1: it is (0, t), a time column
extern "C" int bx_shap_perturb_eeg(const float* x, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int map_rows,
                                   const int* segments, const unsigned char* Z, int M, int N, int n0, int n, bxStream stream) {
  BX_REQUIRE(Chans > 0 && (map_rows == Chans || map_rows == 1), "bx_shap_perturb_eeg: map_rows = %d is neither Chans = %d nor 1", map_rows, Chans);
  int rc = shap_domain_ok("bx_shap_perturb_eeg", map_rows, T, M);
  if (rc) return rc;
  if ((long long)Chans * T > SHAP_MAX_HW) BX_FAIL(BX_EUNSUPPORTED, "bx_shap_perturb_eeg: %lld values per sample, supported 1..%d", (long long)Chans * T, SHAP_MAX_HW);
  if ((rc = shap_rows_ok("bx_shap_perturb_eeg", B, baseline_kind, M, N, n0, n)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_shap_perturb_eeg", "B", B, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && baseline && out && segments && Z, "bx_shap_perturb_eeg: null pointer");
  const ShapMask mask = {Z, segments, M, n0};
  perturb_launch_eeg(stream, x, baseline, baseline_kind, out, B, Chans, T, map_rows, 0, n, mask);
  BX_CHECK_LAUNCH("bx_shap_perturb_eeg");
  return BX_OK;
}

// ---- the constrained fit, fp64 --------------------------------------------------------------------------------------------------------
// With the constraint eliminated on the last player, Xt[n,i] = z_ni - z_n,M-1 (i < Mp = M - 1; -1, 0 or 1) and
// yt_n = v(z_n) - v(0) - z_n,M-1 (v(1) - v(0)).  Every sum below is taken by one thread in index order: no float atomics, identical
// bits run to run.

// G[i][j] = sum_n w_n Xt[n,i] Xt[n,j]: a workgroup owns a 16 x 16 tile, a thread one entry; a chunk of 256 rows is staged in LDS as
// two 16-bit masks (the tile's i and j players), the last player's bit and the weight per row.  A product is -1, 0 or 1, so a term
// is exact and the only roundings are the N adds.
__global__ __launch_bounds__(256) void k_shap_gram(const unsigned char* __restrict__ Z, const double* __restrict__ w, double* __restrict__ G, int N, int M) {
  __shared__ uint32_t zs[256];
  __shared__ int ls[256];
  __shared__ double wl[256];
  const int Mp = M - 1, tid = threadIdx.x, ti = blockIdx.y * 16, tj = blockIdx.x * 16, li = tid >> 4, lj = tid & 15;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += 256) {
    __syncthreads();
    const int n = n0 + tid;
    uint32_t m = 0u;
    int last = 0;
    double wv = 0.0;
    if (n < N) {
      const unsigned char* zr = Z + (size_t)n * M;
#pragma unroll
      for (int u = 0; u < 16; ++u) {                  // unconditional (clamped) loads: all in flight together
        const unsigned char a = zr[ti + u < M ? ti + u : 0], c = zr[tj + u < M ? tj + u : 0];
        if (a) m |= 1u << u;
        if (c) m |= 1u << (16 + u);
      }
      last = zr[Mp] ? 1 : 0;
      wv = w[n];
    }
    zs[tid] = m; ls[tid] = last; wl[tid] = wv;
    __syncthreads();
    const int cnt = N - n0 < 256 ? N - n0 : 256;
    for (int r = 0; r < cnt; ++r) {
      const uint32_t mr = zs[r];
      const int l = ls[r], xi = (int)((mr >> li) & 1u) - l, xj = (int)((mr >> (16 + lj)) & 1u) - l;
      acc += wl[r] * (double)(xi * xj);
    }
  }
  const int i = ti + li, j = tj + lj;
  if (i < Mp && j < Mp) G[(size_t)i * Mp + j] = acc;
}

// (sample, class) of right-hand side q: the sample's explained class, or every class
__device__ __forceinline__ void shap_pair(const int* __restrict__ classes, int q, int K, int& b, int& k) {
  b = q;
  if (classes) { k = classes[q]; k = k < 0 ? 0 : (k >= K ? K - 1 : k); }
  else { b = q / K; k = q - b * K; }
}

// r[q][i] = sum_n Xt[n,i] (w_n yt_n,q): a workgroup owns one right-hand side, thread i player i; a chunk of 256 products w_n yt_n and
// last-player bits is staged in LDS, the coalition bytes of the chunk come from L2 (coalesced over i)
__global__ __launch_bounds__(256) void k_shap_rhs(const float* __restrict__ S, const float* __restrict__ clean, const float* __restrict__ empty,
                                                  const int* __restrict__ classes, const unsigned char* __restrict__ Z, const double* __restrict__ w,
                                                  double* __restrict__ rhs, int N, int K, int M) {
  __shared__ double ys[256];
  __shared__ int ls[256];
  const int Mp = M - 1, tid = threadIdx.x, q = blockIdx.x;
  int b, k;
  shap_pair(classes, q, K, b, k);
  const double v0 = (double)empty[(size_t)b * K + k], delta = (double)clean[(size_t)b * K + k] - v0;
  const int i = tid < Mp ? tid : 0;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += 256) {
    __syncthreads();
    const int n = n0 + tid;
    int last = 0;
    double yv = 0.0;
    if (n < N) {
      last = Z[(size_t)n * M + Mp] ? 1 : 0;
      yv = w[n] * (((double)S[((size_t)b * N + n) * K + k] - v0) - (last ? delta : 0.0));
    }
    ys[tid] = yv; ls[tid] = last;
    __syncthreads();
    const int cnt = N - n0 < 256 ? N - n0 : 256;
    const unsigned char* zc = Z + (size_t)n0 * M + i;
#pragma unroll 8
    for (int r = 0; r < cnt; ++r) {
      const int xi = (zc[(size_t)r * M] ? 1 : 0) - ls[r];
      acc += (double)xi * ys[r];
    }
  }
  if (tid < Mp) rhs[(size_t)q * Mp + tid] = acc;
}

// One workgroup: Cholesky G = L L^T, right-looking, in place in the workspace (column j in LDS for the trailing update; L with its
// diagonal ends in the lower triangle).  A pivot that is not above Mp 2^-52 times its entry of G -- non-positive up to the rounding
// of the eliminations before it, which is all that is left of an exactly singular G -- stops the factorisation: info = index + 1.
__global__ __launch_bounds__(1024) void k_shap_chol(double* __restrict__ G, int Mp, int* __restrict__ info) {
  __shared__ double col[SHAP_MAX_M], dg0[SHAP_MAX_M];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  for (int i = tid; i < Mp; i += 1024) dg0[i] = G[(size_t)i * Mp + i];
  if (tid == 0) *info = 0;
  __syncthreads();
  const double tiny = (double)Mp * 2.220446049250313e-16;
  for (int j = 0; j < Mp; ++j) {
    const double a = G[(size_t)j * Mp + j];                        // the same value in every thread: the branch is uniform
    if (!(a > tiny * dg0[j])) {
      if (tid == 0) *info = j + 1;
      return;
    }
    const double d = sqrt(a);
    __syncthreads();                                                // every thread has read the pivot
    if (tid == 0) G[(size_t)j * Mp + j] = d;
    for (int i = j + 1 + tid; i < Mp; i += 1024) {
      const double x = G[(size_t)i * Mp + j] / d;
      G[(size_t)i * Mp + j] = x;
      col[i] = x;
    }
    __syncthreads();
    const int m0 = j + 1, m = Mp - m0, nt = (m + 31) / 32;
    for (int bi = 0; bi < nt; ++bi) {
      const int i = m0 + bi * 32 + ty;
      if (i >= Mp) continue;
      const double ci = col[i];
      for (int bk = 0; bk <= bi; ++bk) {
        const int k = m0 + bk * 32 + tx;
        if (k <= i) G[(size_t)i * Mp + k] -= ci * col[k];
      }
    }
    __syncthreads();
  }
}

// One workgroup per right-hand side, thread i owns entry i in a register: L y = r column by column (thread j publishes y_j, the
// threads below it take L_ij y_j off their entry), then L^T x = y from the last row up (row j of L, coalesced).  The last player gets
// delta - sum x, the sum taken by one thread in index order with Neumaier's compensation, so that the values of a (sample, class) add
// up to clean - empty to the last bit or two whatever M is.  info != 0: nothing is written.
__global__ __launch_bounds__(256) void k_shap_subst(const double* __restrict__ G, const double* __restrict__ rhs, const float* __restrict__ clean,
                                                    const float* __restrict__ empty, const int* __restrict__ classes, const int* __restrict__ info,
                                                    double* __restrict__ phi, int K, int M) {
  __shared__ double xs[SHAP_MAX_M];
  if (*info != 0) return;
  const int Mp = M - 1, tid = threadIdx.x, q = blockIdx.x;
  const bool mine = tid < Mp;
  const int i = mine ? tid : 0;
  double v = rhs[(size_t)q * Mp + i];
  const double d = G[(size_t)i * Mp + i];
  for (int j = 0; j < Mp; ++j) {
    if (tid == j) xs[j] = v = v / d;
    __syncthreads();
    if (mine && tid > j) v -= G[(size_t)i * Mp + j] * xs[j];
  }
  __syncthreads();
  for (int j = Mp - 1; j >= 0; --j) {
    if (tid == j) xs[j] = v = v / d;
    __syncthreads();
    if (tid < j) v -= G[(size_t)j * Mp + i] * xs[j];
  }
  if (mine) phi[(size_t)q * M + tid] = v;
  if (tid == 0) {
    int b, k;
    shap_pair(classes, q, K, b, k);
    const double delta = (double)clean[(size_t)b * K + k] - (double)empty[(size_t)b * K + k];
    double s = 0.0, c = 0.0;
    for (int j = 0; j < Mp; ++j) {
      const double x = xs[j], t = s + x;
      c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
      s = t;
    }
    phi[(size_t)q * M + Mp] = (delta - s) - c;
  }
}

static int shap_fit_ok(const char* who, int B, int N, int K, int M) {
  BX_REQUIRE(B > 0 && K >= 1, "%s: bad shape B=%d K=%d", who, B, K);
  if (M < 2 || M > SHAP_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "%s: %d players, supported 2..%d", who, M, SHAP_MAX_M);
  if (K > SHAP_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "%s: %d classes, supported 1..%d", who, K, SHAP_MAX_K);
  BX_REQUIRE(N >= M - 1, "%s: N = %d coalitions cannot determine %d players (N >= M - 1)", who, N, M);
  BX_REQUIRE((long long)B * N * K < (1ll << 31) && (long long)N * M < (1ll << 31) && (long long)B * K * M < (1ll << 31),
             "%s: B * N * K, N * M or B * K * M beyond 32-bit offsets", who);
  return BX_OK;
}
extern "C" size_t bx_shap_fit_workspace(int B, int N, int K, int M, int all_classes) {
  if (shap_fit_ok("bx_shap_fit_workspace", B, N, K, M) != BX_OK) return 0;
  const size_t Mp = M - 1, Q = (size_t)B * (all_classes ? K : 1);
  return (Mp * Mp + Q * Mp) * sizeof(double);
}
extern "C" int bx_shap_fit(const float* S, const float* clean, const float* empty, const int* classes, const unsigned char* Z, const double* weights,
                           int B, int N, int K, int M, void* workspace, size_t workspace_bytes, double* phi, int* info, bxStream stream) {
  const int rc = shap_fit_ok("bx_shap_fit", B, N, K, M);
  if (rc) return rc;
  BX_REQUIRE(S && clean && empty && Z && weights && workspace && phi && info, "bx_shap_fit: null pointer");
  const size_t need = bx_shap_fit_workspace(B, N, K, M, classes ? 0 : 1);
  if (workspace_bytes < need) BX_FAIL(BX_EWORKSPACE, "bx_shap_fit: workspace of %zu bytes, need %zu", workspace_bytes, need);
  BX_REQUIRE(((uintptr_t)workspace & 7) == 0, "bx_shap_fit: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int Mp = M - 1, Q = classes ? B : B * K, T = bx_ceil_div(Mp, 16);
  double* G = (double*)workspace;
  double* rhs = G + (size_t)Mp * Mp;
  hipLaunchKernelGGL(k_shap_gram, dim3(T, T), dim3(256), 0, s, Z, weights, G, N, M);
  hipLaunchKernelGGL(k_shap_rhs, dim3(Q), dim3(256), 0, s, S, clean, empty, classes, Z, weights, rhs, N, K, M);
  hipLaunchKernelGGL(k_shap_chol, dim3(1), dim3(1024), 0, s, G, Mp, info);
  hipLaunchKernelGGL(k_shap_subst, dim3(Q), dim3(256), 0, s, G, rhs, clean, empty, classes, info, phi, K, M);
  BX_CHECK_LAUNCH("bx_shap_fit");
  return BX_OK;
}

// ---- per-cell map: map[b, r, p] = (float) phi[b, r, seg[p]] ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shap_value_map(const double* __restrict__ phi, const int* __restrict__ seg, float* __restrict__ map, int HW, int M,
                                                        int Q) {
  __shared__ float val[SHAP_MAX_M];
  const int tid = threadIdx.x, p = blockIdx.x * 256 + tid;
  const int s = p < HW ? seg[p] : 0;
  for (int q = blockIdx.y; q < Q; q += gridDim.y) {
    __syncthreads();
    if (tid < M) val[tid] = (float)phi[(size_t)q * M + tid];
    __syncthreads();
    if (p < HW) map[(size_t)q * HW + p] = (unsigned)s < (unsigned)M ? val[s] : 0.f;
  }
}
extern "C" int bx_shap_value_map(const double* phi, const int* segments, float* map, int B, int R, int Hm, int Wm, int M, bxStream stream) {
  const int rc = shap_domain_ok("bx_shap_value_map", Hm, Wm, M);
  if (rc) return rc;
  BX_REQUIRE(B > 0 && R >= 1, "bx_shap_value_map: bad shape B=%d R=%d", B, R);
  if (R > SHAP_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_shap_value_map: %d classes, supported 1..%d", R, SHAP_MAX_K);
  BX_REQUIRE((long long)B * R * Hm * Wm < (1ll << 31), "bx_shap_value_map: B * R * Hm * Wm beyond 32-bit offsets");
  BX_REQUIRE(phi && segments && map, "bx_shap_value_map: null pointer");
  const int Q = B * R;
  hipLaunchKernelGGL(k_shap_value_map, dim3(bx_ceil_div((long long)Hm * Wm, 256), Q < 65535 ? Q : 65535), dim3(256), 0, (hipStream_t)stream, phi, segments,
                     map, Hm * Wm, M, Q);
  BX_CHECK_LAUNCH("bx_shap_value_map");
  return BX_OK;
}
