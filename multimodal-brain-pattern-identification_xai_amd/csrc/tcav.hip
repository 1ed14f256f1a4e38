// Testing with Concept Activation Vectors (Kim et al., ICML 2018; Captum's concept.TCAV; Pattern-CAVs: Pahde et al. 2022): the concept
// side of the method.  The activations of every concept and random example are stacked once, [M, D]; their globally centred Gram matrix
// G0 is computed once in fp64; every linear classifier (one per (concept, random set) pair and one per null pair) is then a function of
// G0 alone -- a dual ridge solve by Cholesky or the difference of the class means -- and the CAVs, the directional derivatives against
// all of them and the TCAV scores follow.  See include/brainxai.h for the definition and the contract of each entry point.
// No atomics; every sum is taken in an order that depends on the shapes alone.  Built with -ffp-contract=off: a * b + c below is two
// roundings unless it is written fma().
#include "bx_common.h"
#include <math.h>

#define TCAV_MAX_M 8192                // stacked rows
#define TCAV_MAX_D (1 << 24)           // features of an activation
#define TCAV_MAX_NI 512                // rows of a problem
#define TCAV_MAX_P 65535               // problems
#define TCAV_MAX_K 32                  // classes
#define TCAV_TILE 64                   // rows of a Gram tile
#define TCAV_DC 32                     // features of a chunk in LDS
#define TCAV_MAX_SPLIT 32              // workgroups that share the features of a tile
#define TCAV_MIN_SPLIT_LEN 512
#define TCAV_EPS 2.220446049250313e-16

static int tcav_stack_ok(const char* who, int M, int D) {
  BX_REQUIRE(M >= 1 && D >= 1, "%s: bad shape M=%d D=%d", who, M, D);
  if (M > TCAV_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "%s: %d stacked rows, supported 1..%d", who, M, TCAV_MAX_M);
  if (D > TCAV_MAX_D) BX_FAIL(BX_EUNSUPPORTED, "%s: %d features, supported 1..%d", who, D, TCAV_MAX_D);
  return BX_OK;
}

// ---- column mean, fp64, row order ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_tcav_mean(const T* __restrict__ A, double* __restrict__ mean, int M, int D) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
#pragma unroll 8
  for (int i = 0; i < M; ++i) s += (double)ldf(A, (size_t)i * D + d);
  mean[d] = s / (double)M;
}

extern "C" int bx_tcav_mean(const void* A, double* mean, int M, int D, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  const int rc = tcav_stack_ok("bx_tcav_mean", M, D);
  if (rc) return rc;
  BX_REQUIRE(A && mean, "bx_tcav_mean: null pointer");
  BX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(k_tcav_mean<T>, dim3(bx_ceil_div(D, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)A, mean, M, D));
  BX_CHECK_LAUNCH("bx_tcav_mean");
  return BX_OK;
}

// ---- G0 = (A - 1 mean^T)(A - 1 mean^T)^T, fp64 ---------------------------------------------------------------------------------------
// A workgroup owns a 64 x 64 tile of row pairs of the lower triangle and one split of the features; a thread owns 4 x 4 entries.  A chunk
// of 32 features of the tile's 64 + 64 rows is centred in fp64 and staged in LDS feature-major, so that a thread's four row values are
// one 32-byte read shared by the 16 threads of its row group (a broadcast) -- 16 fp64 FMAs per eight 8-byte LDS values.  The partial
// tiles go to the workspace [split][tile][64][64]; k_tcav_gram_reduce adds them in split order and writes both (i, j) and (j, i).
static inline int tcav_split_len(int D) {
  int len = (D + TCAV_MAX_SPLIT - 1) / TCAV_MAX_SPLIT;
  len = (len + TCAV_DC - 1) / TCAV_DC * TCAV_DC;
  return len < TCAV_MIN_SPLIT_LEN ? TCAV_MIN_SPLIT_LEN : len;
}
static inline int tcav_tiles(int M) { return (M + TCAV_TILE - 1) / TCAV_TILE; }

template <typename T>
__global__ __launch_bounds__(256) void k_tcav_gram(const T* __restrict__ A, const double* __restrict__ mean, double* __restrict__ part, int M, int D, int len) {
  const int tj = blockIdx.x, ti = blockIdx.y, sp = blockIdx.z;
  if (tj > ti) return;
  __shared__ __attribute__((aligned(16))) double As[TCAV_DC][TCAV_TILE + 2];
  __shared__ __attribute__((aligned(16))) double Bs[TCAV_DC][TCAV_TILE + 2];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lr = tid >> 5, ld = tid & 31;
  const int d0 = sp * len, d1 = d0 + len < D ? d0 + len : D;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int c0 = d0; c0 < d1; c0 += TCAV_DC) {
    __syncthreads();
    const int d = c0 + ld;
    const bool dok = d < d1;
    const double md = mean[dok ? d : d0];
    float va[8], vb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                      // unconditional (clamped) loads: all in flight together
      const int gi = ti * TCAV_TILE + lr + 8 * k, gj = tj * TCAV_TILE + lr + 8 * k;
      va[k] = ldf(A, (size_t)(gi < M ? gi : 0) * D + (dok ? d : d0));
      vb[k] = ldf(A, (size_t)(gj < M ? gj : 0) * D + (dok ? d : d0));
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = lr + 8 * k;
      As[ld][r] = dok && ti * TCAV_TILE + r < M ? (double)va[k] - md : 0.0;
      Bs[ld][r] = dok && tj * TCAV_TILE + r < M ? (double)vb[k] - md : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int dd = 0; dd < TCAV_DC; ++dd) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = As[dd][ty * 4 + u]; b[u] = Bs[dd][tx * 4 + u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
  }
  const size_t tl = (size_t)ti * (ti + 1) / 2 + tj, NT = (size_t)gridDim.y * (gridDim.y + 1) / 2;
  double* out = part + ((size_t)sp * NT + tl) * (TCAV_TILE * TCAV_TILE);
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) out[(ty * 4 + u) * TCAV_TILE + tx * 4 + v] = acc[u][v];
}

__global__ __launch_bounds__(256) void k_tcav_gram_reduce(const double* __restrict__ part, double* __restrict__ G0, int M, int S) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= M || j > i) return;
  const int ti = i / TCAV_TILE, tj = j / TCAV_TILE, T = (M + TCAV_TILE - 1) / TCAV_TILE;
  const size_t tl = (size_t)ti * (ti + 1) / 2 + tj, NT = (size_t)T * (T + 1) / 2;
  const double* src = part + tl * (TCAV_TILE * TCAV_TILE) + (size_t)(i - ti * TCAV_TILE) * TCAV_TILE + (j - tj * TCAV_TILE);
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += src[(size_t)k * NT * (TCAV_TILE * TCAV_TILE)];
  G0[(size_t)i * M + j] = s;
  G0[(size_t)j * M + i] = s;
}

extern "C" size_t bx_tcav_gram_workspace(int M, int D) {
  if (tcav_stack_ok("bx_tcav_gram_workspace", M, D) != BX_OK) return 0;
  const size_t T = tcav_tiles(M), S = bx_ceil_div(D, tcav_split_len(D));
  return S * (T * (T + 1) / 2) * (TCAV_TILE * TCAV_TILE) * sizeof(double);
}

extern "C" int bx_tcav_gram(const void* A, const double* mean, double* G0, int M, int D, int dtype, void* workspace, size_t workspace_bytes,
                            bxStream stream) {
  BX_DTYPE_OK(dtype);
  const int rc = tcav_stack_ok("bx_tcav_gram", M, D);
  if (rc) return rc;
  BX_REQUIRE(A && mean && G0 && workspace, "bx_tcav_gram: null pointer");
  const size_t need = bx_tcav_gram_workspace(M, D);
  if (workspace_bytes < need) BX_FAIL(BX_EWORKSPACE, "bx_tcav_gram: workspace of %zu bytes, need %zu", workspace_bytes, need);
  BX_REQUIRE(((uintptr_t)workspace & 15) == 0, "bx_tcav_gram: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int T = tcav_tiles(M), len = tcav_split_len(D), S = bx_ceil_div(D, len);
  BX_DISPATCH_DTYPE(dtype, Ty, hipLaunchKernelGGL(k_tcav_gram<Ty>, dim3(T, T, S), dim3(256), 0, s, (const Ty*)A, mean, (double*)workspace, M, D, len));
  hipLaunchKernelGGL(k_tcav_gram_reduce, dim3(bx_ceil_div(M, 16), bx_ceil_div(M, 16)), dim3(256), 0, s, (const double*)workspace, G0, M, S);
  BX_CHECK_LAUNCH("bx_tcav_gram");
  return BX_OK;
}

// ---- the classifiers: one workgroup per problem ---------------------------------------------------------------------------------------
// Thread a owns fit row a wherever a vector is held; the nf x nf matrix lives in the problem's slab of the workspace.  The Cholesky
// factorisation and the two substitutions are k_shap_chol's and k_shap_subst's schemes (right-looking, column j in LDS for the trailing
// update; a pivot that is not above nf 2^-52 times its entry of K + lambda I stops the problem).  Every reduction is one thread's loop
// in row order.  A problem that ends with a status writes that status and nothing else.
__global__ __launch_bounds__(1024) void k_tcav_fit(const double* __restrict__ G0, int M, const int* __restrict__ rows, const int* __restrict__ labels,
                                                   const int* __restrict__ fitmark, const int* __restrict__ counts, int NI, int classifier, double ridge,
                                                   double* __restrict__ slabs, int nfmax, double* __restrict__ beta, double* __restrict__ norm,
                                                   double* __restrict__ lam, int* __restrict__ status, double* __restrict__ decision,
                                                   double* __restrict__ accuracy) {
  __shared__ int fr[TCAV_MAX_NI], fj[TCAV_MAX_NI], ir[TCAV_MAX_NI], iy[TCAV_MAX_NI], ifit[TCAV_MAX_NI];
  __shared__ double fy[TCAV_MAX_NI], col[TCAV_MAX_NI], dg0[TCAV_MAX_NI], rm[TCAV_MAX_NI], bet[TCAV_MAX_NI], sd[TCAV_MAX_NI];
  __shared__ int sh_i[4];
  __shared__ double sh_d[8];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, p = blockIdx.x;
  int ni = counts[p];
  ni = ni < 0 ? 0 : (ni > NI ? NI : ni);
  for (int j = tid; j < ni; j += 1024) {
    ir[j] = rows[(size_t)p * NI + j];
    iy[j] = labels[(size_t)p * NI + j];
    ifit[j] = fitmark[(size_t)p * NI + j];
  }
  __syncthreads();
  if (tid == 0) {
    int nf = 0, np = 0, nn = 0, bad = 0;
    for (int j = 0; j < ni; ++j) {
      if (ir[j] < 0 || ir[j] >= M || (iy[j] != 1 && iy[j] != -1)) bad = 1;
      if (ifit[j] && !bad) {
        if (nf < nfmax) { fr[nf] = ir[j]; fj[nf] = j; fy[nf] = (double)iy[j]; }
        ++nf;
        if (iy[j] > 0) ++np; else ++nn;
      }
    }
    if (nf > nfmax || np < 1 || nn < 1) bad = 1;
    sh_i[0] = nf; sh_i[1] = np; sh_i[2] = nn; sh_i[3] = bad;
  }
  __syncthreads();
  const int nf = sh_i[0], np = sh_i[1], nn = sh_i[2];
  if (sh_i[3]) {                                                     // a malformed problem: the driver never builds one
    if (tid == 0) status[p] = 4;
    return;
  }
  const bool mine = tid < nf;
  const int me = mine ? tid : 0;
  const double ybar = ((double)np - (double)nn) / (double)nf;
  double lambda = 0.0;
  if (classifier == BX_TCAV_RIDGE) {
    double* K = slabs + (size_t)p * nfmax * nfmax;
    for (int idx = tid; idx < nf * nf; idx += 1024) {
      const int a = idx / nf, b = idx - a * nf;
      K[idx] = G0[(size_t)fr[a] * M + fr[b]];
    }
    __syncthreads();
    if (mine) {                                                      // row means of the gathered block (it is symmetric bit for bit)
      double s = 0.0;
      for (int b = 0; b < nf; ++b) s += K[(size_t)tid * nf + b];
      rm[tid] = s / (double)nf;
      col[tid] = K[(size_t)tid * nf + tid];
    }
    __syncthreads();
    if (tid == 0) {
      double g = 0.0, tg = 0.0;
      for (int a = 0; a < nf; ++a) { g += rm[a]; tg += col[a]; }
      sh_d[0] = g / (double)nf; sh_d[1] = tg;
    }
    __syncthreads();
    const double gm = sh_d[0], trG = sh_d[1];
    for (int idx = tid; idx < nf * nf; idx += 1024) {                // K = H G0[I,I] H
      const int a = idx / nf, b = idx - a * nf;
      K[idx] = ((K[idx] - rm[a]) - rm[b]) + gm;
    }
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int a = 0; a < nf; ++a) t += K[(size_t)a * nf + a];
      sh_d[2] = t;
    }
    __syncthreads();
    const double trK = sh_d[2];
    if (!(trK > (double)nf * TCAV_EPS * trG)) {                      // no scatter inside the problem beyond the rounding of the centring
      if (tid == 0) status[p] = 1;
      return;
    }
    lambda = ridge * trK / (double)nf;
    if (mine) {
      const double v = K[(size_t)tid * nf + tid] + lambda;
      K[(size_t)tid * nf + tid] = v;
      dg0[tid] = v;
    }
    __syncthreads();
    const double tiny = (double)nf * TCAV_EPS;
    for (int j = 0; j < nf; ++j) {
      const double a = K[(size_t)j * nf + j];                        // the same value in every thread: the branch is uniform
      if (!(a > tiny * dg0[j])) {
        if (tid == 0) status[p] = 3;
        return;
      }
      const double d = sqrt(a);
      __syncthreads();                                               // every thread has read the pivot
      if (tid == 0) K[(size_t)j * nf + j] = d;
      for (int i = j + 1 + tid; i < nf; i += 1024) {
        const double x = K[(size_t)i * nf + j] / d;
        K[(size_t)i * nf + j] = x;
        col[i] = x;
      }
      __syncthreads();
      const int m0 = j + 1, m = nf - m0, nt = (m + 31) / 32;
      for (int bi = 0; bi < nt; ++bi) {
        const int i = m0 + bi * 32 + ty;
        if (i >= nf) continue;
        const double ci = col[i];
        for (int bk = 0; bk <= bi; ++bk) {
          const int k = m0 + bk * 32 + tx;
          if (k <= i) K[(size_t)i * nf + k] -= ci * col[k];
        }
      }
      __syncthreads();
    }
    double v = fy[me] - ybar;                                        // (K + lambda I) alpha = H y
    const double d = K[(size_t)me * nf + me];
    for (int j = 0; j < nf; ++j) {
      if (tid == j) col[j] = v = v / d;
      __syncthreads();
      if (mine && tid > j) v -= K[(size_t)me * nf + j] * col[j];
    }
    __syncthreads();
    for (int j = nf - 1; j >= 0; --j) {
      if (tid == j) col[j] = v = v / d;
      __syncthreads();
      if (tid < j) v -= K[(size_t)j * nf + me] * col[j];
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int a = 0; a < nf; ++a) s += col[a];
      sh_d[3] = s / (double)nf;
    }
    __syncthreads();
    if (mine) bet[tid] = col[tid] - sh_d[3];                         // beta = H alpha
  } else {
    if (mine) bet[tid] = fy[tid] > 0.0 ? 1.0 / (double)np : -1.0 / (double)nn;
  }
  __syncthreads();
  // s_j = sum_a beta_a G0[row_j, fit row a] for every row of the problem, held-out rows included
  if (tid < ni) {
    const double* g = G0 + (size_t)ir[tid] * M;
    double s = 0.0;
    for (int a = 0; a < nf; ++a) s += bet[a] * g[fr[a]];
    sd[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double w2 = 0.0, sc = 0.0, sm = 0.0, sp = 0.0, sn = 0.0;
    for (int a = 0; a < nf; ++a) {
      const double s = sd[fj[a]], gaa = G0[(size_t)fr[a] * M + fr[a]];
      w2 += bet[a] * s;
      sc += fabs(bet[a]) * sqrt(gaa > 0.0 ? gaa : 0.0);
      sm += s;
      if (fy[a] > 0.0) sp += s; else sn += s;
    }
    sh_d[4] = w2; sh_d[5] = sc * sc;
    sh_d[6] = classifier == BX_TCAV_RIDGE ? sm / (double)nf - ybar : 0.5 * (sp / (double)np + sn / (double)nn);
  }
  __syncthreads();
  const double w2 = sh_d[4];
  if (!(w2 > (double)nf * TCAV_EPS * sh_d[5])) {                     // w = 0 up to the rounding of its own sum
    if (tid == 0) status[p] = 2;
    return;
  }
  if (tid < ni) sd[tid] = sd[tid] - sh_d[6];
  for (int i = tid; i < M; i += 1024) beta[(size_t)p * M + i] = 0.0;
  __syncthreads();
  if (mine) beta[(size_t)p * M + fr[tid]] = bet[tid];
  if (tid < ni) decision[(size_t)p * NI + tid] = sd[tid];
  if (tid == 0) {
    int okf = 0, okh = 0, nh = 0;
    for (int j = 0; j < ni; ++j) {
      const int hit = (sd[j] > 0.0 ? 1 : -1) == iy[j];
      if (ifit[j]) okf += hit; else { okh += hit; ++nh; }
    }
    accuracy[(size_t)p * 2] = (double)okf / (double)nf;
    accuracy[(size_t)p * 2 + 1] = nh ? (double)okh / (double)nh : NAN;
    norm[p] = sqrt(w2);
    lam[p] = lambda;
    status[p] = 0;
  }
}

static int tcav_fit_ok(const char* who, int P, int NI, int nfmax) {
  BX_REQUIRE(P >= 1 && NI >= 2 && nfmax >= 2 && nfmax <= NI, "%s: bad shape P=%d NI=%d nf=%d", who, P, NI, nfmax);
  if (NI > TCAV_MAX_NI) BX_FAIL(BX_EUNSUPPORTED, "%s: %d rows per problem, supported 2..%d", who, NI, TCAV_MAX_NI);
  if (P > TCAV_MAX_P) BX_FAIL(BX_EUNSUPPORTED, "%s: %d problems, supported 1..%d", who, P, TCAV_MAX_P);
  return BX_OK;
}
extern "C" size_t bx_tcav_fit_workspace(int P, int nfmax) {
  if (tcav_fit_ok("bx_tcav_fit_workspace", P, nfmax > 2 ? nfmax : 2, nfmax) != BX_OK) return 0;
  return (size_t)P * nfmax * nfmax * sizeof(double);
}
extern "C" int bx_tcav_fit(const double* G0, int M, const int* rows, const int* labels, const int* fit, const int* counts, int P, int NI, int nfmax,
                           int classifier, double ridge, void* workspace, size_t workspace_bytes, double* beta, double* norm, double* lam, int* status,
                           double* decision, double* accuracy, bxStream stream) {
  const int rc = tcav_fit_ok("bx_tcav_fit", P, NI, nfmax);
  if (rc) return rc;
  BX_REQUIRE(M >= 1, "bx_tcav_fit: bad shape M=%d", M);
  if (M > TCAV_MAX_M) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_fit: %d stacked rows, supported 1..%d", M, TCAV_MAX_M);
  BX_REQUIRE(classifier == BX_TCAV_RIDGE || classifier == BX_TCAV_MEAN_DIFFERENCE, "bx_tcav_fit: classifier %d (0 ridge, 1 mean difference)", classifier);
  BX_REQUIRE(classifier != BX_TCAV_RIDGE || (ridge > 0.0 && ridge < INFINITY), "bx_tcav_fit: ridge = %g is not a positive number", ridge);
  BX_REQUIRE(G0 && rows && labels && fit && counts && workspace && beta && norm && lam && status && decision && accuracy, "bx_tcav_fit: null pointer");
  const size_t need = bx_tcav_fit_workspace(P, nfmax);
  if (workspace_bytes < need) BX_FAIL(BX_EWORKSPACE, "bx_tcav_fit: workspace of %zu bytes, need %zu", workspace_bytes, need);
  BX_REQUIRE(((uintptr_t)workspace & 7) == 0, "bx_tcav_fit: workspace not 8-byte aligned");
  hipLaunchKernelGGL(k_tcav_fit, dim3(P), dim3(1024), 0, (hipStream_t)stream, G0, M, rows, labels, fit, counts, NI, classifier, ridge, (double*)workspace,
                     nfmax, beta, norm, lam, status, decision, accuracy);
  BX_CHECK_LAUNCH("bx_tcav_fit");
  return BX_OK;
}

// ---- the CAVs: V[p, d] = sum_i beta[p, i] (a_id - mean_d) / ||w_p||, fp64 in row order, stored fp32 ------------------------------------
// A thread owns one feature and eight problems; 256 rows of the eight dual vectors are staged in LDS, and a row none of them uses is
// skipped (its term is an exact zero).  A problem with a status keeps its row of V as it was.
#define TCAV_VP 8
template <typename T>
__global__ __launch_bounds__(256) void k_tcav_vectors(const T* __restrict__ A, const double* __restrict__ mean, const double* __restrict__ beta,
                                                      const double* __restrict__ norm, const int* __restrict__ status, float* __restrict__ V, int M, int D,
                                                      int P) {
  __shared__ double bs[256][TCAV_VP];
  __shared__ int nz[256];
  const int tid = threadIdx.x, d = blockIdx.x * 256 + tid, p0 = blockIdx.y * TCAV_VP, dc = d < D ? d : D - 1;
  const double md = mean[dc];
  double acc[TCAV_VP];
#pragma unroll
  for (int k = 0; k < TCAV_VP; ++k) acc[k] = 0.0;
  for (int i0 = 0; i0 < M; i0 += 256) {
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int k = 0; k < TCAV_VP; ++k) {
      const double b = (i0 + tid < M && p0 + k < P) ? beta[(size_t)(p0 + k) * M + i0 + tid] : 0.0;
      bs[tid][k] = b;
      any |= b != 0.0;
    }
    nz[tid] = any;
    __syncthreads();
    const int cnt = M - i0 < 256 ? M - i0 : 256;
    for (int r = 0; r < cnt; ++r) {
      if (!nz[r]) continue;                                          // uniform over the workgroup
      const double x = (double)ldf(A, (size_t)(i0 + r) * D + dc) - md;
#pragma unroll
      for (int k = 0; k < TCAV_VP; ++k) acc[k] += bs[r][k] * x;
    }
  }
  if (d < D) {
#pragma unroll
    for (int k = 0; k < TCAV_VP; ++k)
      if (p0 + k < P && status[p0 + k] == 0) V[(size_t)(p0 + k) * D + d] = (float)(acc[k] / norm[p0 + k]);
  }
}

extern "C" int bx_tcav_vectors(const void* A, const double* mean, const double* beta, const double* norm, const int* status, float* V, int M, int D,
                               int P, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  const int rc = tcav_stack_ok("bx_tcav_vectors", M, D);
  if (rc) return rc;
  BX_REQUIRE(P >= 1, "bx_tcav_vectors: bad shape P=%d", P);
  if (P > TCAV_MAX_P) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_vectors: %d problems, supported 1..%d", P, TCAV_MAX_P);
  BX_REQUIRE(A && mean && beta && norm && status && V, "bx_tcav_vectors: null pointer");
  BX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(k_tcav_vectors<T>, dim3(bx_ceil_div(D, 256), bx_ceil_div(P, TCAV_VP)), dim3(256), 0, (hipStream_t)stream,
                                                 (const T*)A, mean, beta, norm, status, V, M, D, P));
  BX_CHECK_LAUNCH("bx_tcav_vectors");
  return BX_OK;
}

// ---- directional derivatives: S[row0 + r, p] = sum_d G[r, d] V[p, d], fp64 ----------------------------------------------------------------
// A workgroup owns 4 gradient rows and 4 CAVs: thread t adds the features t, t + 256, ... in ascending order (a product of two fp32
// values is exact in fp64), the 256 partial sums of an entry are then added 16 by 16 in thread order.  The order depends on D alone, so
// no bit depends on how the rows were cut into chunks.
template <typename T>
__global__ __launch_bounds__(256) void k_tcav_sensitivity(const T* __restrict__ G, const float* __restrict__ V, double* __restrict__ S, int rows, int D,
                                                          int P, int row0) {
  __shared__ double sp[16][256];
  __shared__ double s2[16][16];
  const int tid = threadIdx.x, r0 = blockIdx.x * 4, p0 = blockIdx.y * 4;
  const T* g[4];
  const float* v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    g[u] = G + (size_t)(r0 + u < rows ? r0 + u : rows - 1) * D;
    v[u] = V + (size_t)(p0 + u < P ? p0 + u : P - 1) * D;
  }
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[u][k] = 0.0;
#pragma unroll 2
  for (int d = tid; d < D; d += 256) {
    double gv[4], vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { gv[u] = (double)ldf(g[u], (size_t)d); vv[u] = (double)v[u][d]; }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[u][k] += gv[u] * vv[k];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int k = 0; k < 4; ++k) sp[u * 4 + k][tid] = acc[u][k];
  __syncthreads();
  {
    const int o = tid >> 4, sl = tid & 15;
    double s = 0.0;
    for (int q = 0; q < 16; ++q) s += sp[o][sl * 16 + q];
    s2[o][sl] = s;
  }
  __syncthreads();
  if (tid < 16) {
    double s = 0.0;
    for (int q = 0; q < 16; ++q) s += s2[tid][q];
    const int r = r0 + (tid >> 2), p = p0 + (tid & 3);
    if (r < rows && p < P) S[(size_t)(row0 + r) * P + p] = s;
  }
}

extern "C" int bx_tcav_sensitivity(const void* G, const float* V, double* S, int rows, int D, int P, int row0, int rows_total, int dtype,
                                   bxStream stream) {
  BX_DTYPE_OK(dtype);
  BX_REQUIRE(rows >= 1 && D >= 1 && P >= 1, "bx_tcav_sensitivity: bad shape rows=%d D=%d P=%d", rows, D, P);
  if (D > TCAV_MAX_D) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_sensitivity: %d features, supported 1..%d", D, TCAV_MAX_D);
  if (P > TCAV_MAX_P) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_sensitivity: %d problems, supported 1..%d", P, TCAV_MAX_P);
  BX_REQUIRE(row0 >= 0 && (long long)row0 + rows <= rows_total, "bx_tcav_sensitivity: rows %d..%d outside 0..%d", row0, row0 + rows, rows_total);
  BX_REQUIRE(G && V && S, "bx_tcav_sensitivity: null pointer");
  BX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(k_tcav_sensitivity<T>, dim3(bx_ceil_div(rows, 4), bx_ceil_div(P, 4)), dim3(256), 0, (hipStream_t)stream,
                                                 (const T*)G, V, S, rows, D, P, row0));
  BX_CHECK_LAUNCH("bx_tcav_sensitivity");
  return BX_OK;
}

// ---- TCAV scores: per (problem, class) the share of positive derivatives, their mean and the mean of their size -------------------------
// One thread per (problem, class), the rows in ascending order.  classes NULL: row r is explained for class r % K (every sample for every
// class).  A class without rows gets NaN.
__global__ __launch_bounds__(64) void k_tcav_score(const double* __restrict__ S, const int* __restrict__ classes, int rows, int P, int K,
                                                   double* __restrict__ score, double* __restrict__ mean, double* __restrict__ mean_abs,
                                                   int* __restrict__ counts) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= P * K) return;
  const int p = idx / K, k = idx - p * K;
  int n = 0, pos = 0;
  double sm = 0.0, sa = 0.0;
  for (int r = 0; r < rows; ++r) {
    const int c = classes ? classes[r] : r % K;
    if (c != k) continue;
    const double v = S[(size_t)r * P + p];
    ++n;
    pos += v > 0.0 ? 1 : 0;
    sm += v;
    sa += fabs(v);
  }
  score[idx] = n ? (double)pos / (double)n : NAN;
  mean[idx] = n ? sm / (double)n : NAN;
  mean_abs[idx] = n ? sa / (double)n : NAN;
  if (p == 0) counts[k] = n;
}

extern "C" int bx_tcav_score(const double* S, const int* classes, int rows, int P, int K, double* score, double* mean, double* mean_abs, int* counts,
                             bxStream stream) {
  BX_REQUIRE(rows >= 1 && P >= 1 && K >= 1, "bx_tcav_score: bad shape rows=%d P=%d K=%d", rows, P, K);
  if (K > TCAV_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_score: %d classes, supported 1..%d", K, TCAV_MAX_K);
  if (P > TCAV_MAX_P) BX_FAIL(BX_EUNSUPPORTED, "bx_tcav_score: %d problems, supported 1..%d", P, TCAV_MAX_P);
  BX_REQUIRE(S && score && mean && mean_abs && counts, "bx_tcav_score: null pointer");
  hipLaunchKernelGGL(k_tcav_score, dim3(bx_ceil_div((long long)P * K, 64)), dim3(64), 0, (hipStream_t)stream, S, classes, rows, P, K, score, mean, mean_abs,
                     counts);
  BX_CHECK_LAUNCH("bx_tcav_score");
  return BX_OK;
}
