// Spectral attributions of the EEG input (amplitude gradients and spectral perturbation: Schirrmeister et al., Hum. Brain Mapp. 2017;
// braindecode's compute_amplitude_gradients): the real DFT of every electrode's trace for any length 1..8192 as a direct fp64 sum over a
// host-made twiddle table, the fp64 running sum of the path-weighted gradient in fixed step order (the walk of sample_rows.h), the
// amplitude gradient / gradient x amplitude per frequency bin with the gradient's transform kept in registers, band sums, and the
// band-stopped rows of spectral occlusion written in the EEG layout.  The forward and backward passes are the model's own kernels; the
// path rows are bx_expgrad_rows, the seeds bx_expgrad_seed.  See include/brainxai.h for the definition and each entry point.
// The file is compiled with -ffp-contract=off: the accumulate's w * g and its sum are two separate fp64 roundings (numpy's, bit for
// bit); the transforms ask for their fused multiply-adds by name (fma), one rounding per term, in ascending t or f.
// No sum here uses an atomic or depends on the launch geometry: a thread owns its output and walks its terms in ascending order.
#include "sample_rows.h"

#define SP_LDS 65536                  // dynamic LDS of a workgroup: the twiddle table where it fits (and a tile of bins in the band-stop kernel)
#define SP_TILE 1024                  // bins of a band staged at a time by the band-stop kernel (16 KiB)
typedef double2 sp_c;                 // (cos, sin) of a table entry; (re, im) of a staged bin

__device__ __forceinline__ double sp_cf(int f, int T) { return (f == 0 || 2 * f == T) ? 1.0 : 2.0; }

// ---- the table ---------------------------------------------------------------------------------------------------------------------------
// The lanes of a wave read entries j = (f t) mod T for consecutive f (or t): an arithmetic progression whose stride is even half of the
// time, so that a group of 16 lanes of a 16-byte LDS read lands on 8, 4, 2 or a single four-bank slot (measured: the plain layout ran
// at a seventh of the fp64 rate).  In LDS entry j lives at j ^ ((j >> 4) & 15): the slot within a run of 16 entries is mixed with the
// run's number, which spreads those progressions over the slots again.  The image takes sp_padded(T) entries.  A table too large for
// LDS beside the rows is read from global memory in its plain order.
static inline __host__ __device__ int sp_padded(int T) { return (T + 15) & ~15; }
struct SpTabLds {
  const sp_c* p;
  __device__ __forceinline__ sp_c operator[](int j) const { return p[j ^ ((j >> 4) & 15)]; }
};
struct SpTabGlobal {
  const sp_c* __restrict__ p;
  __device__ __forceinline__ sp_c operator[](int j) const { return p[j]; }
};
__device__ __forceinline__ void sp_stage_table(const sp_c* __restrict__ tw, int T, sp_c* lds) {
  for (int t = threadIdx.x; t < T; t += 256) lds[t ^ ((t >> 4) & 15)] = tw[t];
}

// ---- the transform body -----------------------------------------------------------------------------------------------------------------
// X_f = sum_t v_t (cos - i sin)(2 pi ((f t) mod T) / T) for RB consecutive rows at once: ascending t, one fma per term and part, the
// table index walked by integer add-and-wrap (f < T, so one conditional subtraction).  One table entry serves the RB rows.  The row
// values are the same for every lane of a wave (all lanes are at the same t), so they are read straight from global memory through the
// scalar cache and never pass through LDS, which the table reads have to themselves.  Rows beyond `valid` repeat the last valid one
// (computed, not stored).  Shared by bx_rdft_rows (fp32 rows) and bx_spectral_values (fp64 gradient sums).
#define SP_RB 8
template <typename Src, typename Tab>
__device__ __forceinline__ void sp_dft_bin(const Src* __restrict__ rows, int valid, Tab tab, int T, int f, double (&re)[SP_RB], double (&im)[SP_RB]) {
  const Src* rp[SP_RB];
#pragma unroll
  for (int i = 0; i < SP_RB; ++i) {
    rp[i] = rows + (size_t)(i < valid ? i : valid - 1) * T;
    re[i] = im[i] = 0.0;
  }
  int j = 0;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    const sp_c w = tab[j];
#pragma unroll
    for (int i = 0; i < SP_RB; ++i) {
      const double v = (double)rp[i][t];
      re[i] = fma(v, w.x, re[i]);
      im[i] = fma(-v, w.y, im[i]);
    }
    j += f;
    j -= j >= T ? T : 0;
  }
}
static inline bool sp_table_in_lds(int T) { return sp_padded(T) * 16 <= SP_LDS; }          // T <= 4096

// ---- x -> X -----------------------------------------------------------------------------------------------------------------------------
// A workgroup owns (SP_RB rows, 256 bins); a thread one bin of each of the rows.
template <bool TAB>
__global__ __launch_bounds__(256) void k_rdft_rows(const float* __restrict__ x, const sp_c* __restrict__ tw, double* __restrict__ re, double* __restrict__ im,
                                                   int R, int T, int F, int tiles) {
  extern __shared__ sp_c sp_lds[];
  const int grp = blockIdx.x / tiles, f = (blockIdx.x - grp * tiles) * 256 + threadIdx.x;
  const int r0 = grp * SP_RB, valid = R - r0 < SP_RB ? R - r0 : SP_RB;
  if (TAB) {
    sp_stage_table(tw, T, sp_lds);
    __syncthreads();
  }
  if (f >= F) return;
  double a[SP_RB], b[SP_RB];
  if (TAB) sp_dft_bin(x + (size_t)r0 * T, valid, SpTabLds{sp_lds}, T, f, a, b); else sp_dft_bin(x + (size_t)r0 * T, valid, SpTabGlobal{tw}, T, f, a, b);
#pragma unroll
  for (int i = 0; i < SP_RB; ++i)
    if (i < valid) {
      re[(size_t)(r0 + i) * F + f] = a[i];
      im[(size_t)(r0 + i) * F + f] = b[i];
    }
}
static int sp_shape_ok(const char* who, long long R, int T) {
  BX_REQUIRE(R > 0 && T > 0, "%s: bad shape rows=%lld T=%d", who, R, T);
  if (T > BX_SPECTRAL_MAX_T) BX_FAIL(BX_EUNSUPPORTED, "%s: T = %d, supported 1..%d", who, T, BX_SPECTRAL_MAX_T);
  BX_REQUIRE(R * T < (1ll << 31), "%s: rows * T beyond 32-bit offsets", who);
  BX_REQUIRE(R * bx_ceil_div(T / 2 + 1, 256) < (1ll << 31), "%s: rows * ceil(F / 256) beyond the grid", who);
  return BX_OK;
}
extern "C" int bx_rdft_rows(const float* x, const double* tw, double* re, double* im, int R, int T, bxStream stream) {
  const int rc = sp_shape_ok("bx_rdft_rows", R, T);
  if (rc) return rc;
  BX_REQUIRE(x && tw && re && im, "bx_rdft_rows: null pointer");
  BX_REQUIRE((((uintptr_t)tw & 15) | (((uintptr_t)re | (uintptr_t)im) & 7)) == 0, "bx_rdft_rows: tw must be 16-byte, re and im 8-byte aligned");
  const int F = T / 2 + 1, tiles = bx_ceil_div(F, 256), grid = bx_ceil_div(R, SP_RB) * tiles;
  const sp_c* tab = reinterpret_cast<const sp_c*>(tw);
  if (sp_table_in_lds(T))
    hipLaunchKernelGGL(k_rdft_rows<true>, dim3(grid), dim3(256), (size_t)sp_padded(T) * 16, (hipStream_t)stream, x, tab, re, im, R, T, F, tiles);
  else
    hipLaunchKernelGGL(k_rdft_rows<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, tab, re, im, R, T, F, tiles);
  BX_CHECK_LAUNCH("bx_rdft_rows");
  return BX_OK;
}

// ---- the running sum: w[k] * g, the walk of sample_rows.h with one element per thread -----------------------------------------------------
struct SpTerm {
  const double* w; double* acc;
  static constexpr int SUMS = 1;
  template <int V> struct Keep {};
  template <int V> struct Row { double w; };
  double* sum(int) const { return acc; }
  template <int V> __device__ __forceinline__ void sample(Keep<V>&, int, int, int) const {}
  template <int V> __device__ __forceinline__ void row(Row<V>& r, int, int k, int, int, int) const { r.w = w[k]; }
  template <int V> __device__ __forceinline__ void add(double (&s)[1][V], int q, const Keep<V>&, float g, const Row<V>& r) const {
    const double p = r.w * (double)g;
    s[0][q] = s[0][q] + p;
  }
};
extern "C" int bx_spectral_accumulate(const float* g, const double* w, double* acc, int B, int n, int per, int Kc, int slot, int row0, int rows, bxStream stream) {
  const char* who = "bx_spectral_accumulate";
  SAMPLE_TRY(sample_rows_ok(who, B, n, per, row0, rows));
  SAMPLE_TRY(sample_slot_ok(who, B, per, Kc, slot));
  BX_REQUIRE(g && w && acc, "%s: null pointer", who);
  BX_REQUIRE((((uintptr_t)acc | (uintptr_t)w) & 7) == 0, "%s: w and acc must be 8-byte aligned", who);
  return sample_accumulate<256, 1, 4>(who, stream, g, false, SpTerm{w, acc}, n, per, Kc, slot, row0, rows);
}

// ---- the values -------------------------------------------------------------------------------------------------------------------------
// A workgroup owns SP_RB consecutive (sample, class, electrode) rows of the fp64 gradient sums and 256 bins: a thread transforms them at
// its bin (G stays in registers) and combines each with X of the row's sample and electrode.
template <bool TAB>
__global__ __launch_bounds__(256) void k_spectral_values(const double* __restrict__ gsum, const double* __restrict__ xre, const double* __restrict__ xim,
                                                         const sp_c* __restrict__ tw, float* __restrict__ values, int R, int Kc, int Chans, int T, int F,
                                                         int tiles, int kind) {
  extern __shared__ sp_c sp_lds[];
  const int grp = blockIdx.x / tiles, f = (blockIdx.x - grp * tiles) * 256 + threadIdx.x;
  const int r0 = grp * SP_RB, valid = R - r0 < SP_RB ? R - r0 : SP_RB;
  if (TAB) {
    sp_stage_table(tw, T, sp_lds);
    __syncthreads();
  }
  if (f >= F) return;
  double gre[SP_RB], gim[SP_RB];
  if (TAB) sp_dft_bin(gsum + (size_t)r0 * T, valid, SpTabLds{sp_lds}, T, f, gre, gim); else sp_dft_bin(gsum + (size_t)r0 * T, valid, SpTabGlobal{tw}, T, f, gre, gim);
  const double scale = sp_cf(f, T) / (double)T;
#pragma unroll
  for (int i = 0; i < SP_RB; ++i)
    if (i < valid) {
      const int r = r0 + i, b = r / (Kc * Chans), e = r % Chans;
      const size_t xa = ((size_t)b * Chans + e) * F + f;
      double ur = xre[xa], ui = xim[xa];
      if (kind == BX_SPECTRAL_AMPLITUDE_GRADIENT) {
        if (ur == 0.0 && ui == 0.0) {
          ur = 1.0;
        } else {
          const double m = hypot(ur, ui);
          ur = ur / m;
          ui = ui / m;
        }
      }
      const double dot = fma(ui, gim[i], ur * gre[i]);
      values[(size_t)r * F + f] = (float)(scale * dot);
    }
}
extern "C" int bx_spectral_values(const double* gsum, const double* re, const double* im, const double* tw, float* values, int B, int Kc, int Chans, int T,
                                  int kind, bxStream stream) {
  BX_REQUIRE(B > 0 && Kc > 0 && Chans > 0, "bx_spectral_values: bad shape B=%d Kc=%d Chans=%d", B, Kc, Chans);
  if (Kc > SAMPLE_MAX_K) BX_FAIL(BX_EUNSUPPORTED, "bx_spectral_values: %d classes, supported 1..%d", Kc, SAMPLE_MAX_K);
  const long long RL = (long long)B * Kc * Chans;
  const int rc = sp_shape_ok("bx_spectral_values", RL, T);
  if (rc) return rc;
  BX_REQUIRE(kind == BX_SPECTRAL_AMPLITUDE_GRADIENT || kind == BX_SPECTRAL_GRADIENT_X_AMPLITUDE, "bx_spectral_values: unknown kind %d", kind);
  BX_REQUIRE(gsum && re && im && tw && values, "bx_spectral_values: null pointer");
  BX_REQUIRE((((uintptr_t)tw & 15) | (((uintptr_t)gsum | (uintptr_t)re | (uintptr_t)im) & 7)) == 0,
             "bx_spectral_values: tw must be 16-byte, the sums, re and im 8-byte aligned");
  const int R = (int)RL, F = T / 2 + 1, tiles = bx_ceil_div(F, 256), grid = bx_ceil_div(R, SP_RB) * tiles;
  const sp_c* tab = reinterpret_cast<const sp_c*>(tw);
  if (sp_table_in_lds(T))
    hipLaunchKernelGGL(k_spectral_values<true>, dim3(grid), dim3(256), (size_t)sp_padded(T) * 16, (hipStream_t)stream, gsum, re, im, tab, values, R, Kc, Chans, T,
                       F, tiles, kind);
  else
    hipLaunchKernelGGL(k_spectral_values<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, gsum, re, im, tab, values, R, Kc, Chans, T, F, tiles, kind);
  BX_CHECK_LAUNCH("bx_spectral_values");
  return BX_OK;
}

// ---- band sums --------------------------------------------------------------------------------------------------------------------------
// A thread owns one (row, band) and adds its bins in ascending f; bin ranges are clamped to 0 <= lo <= hi <= F.
__device__ __forceinline__ void sp_band(const int* __restrict__ bins, int q, int F, int& lo, int& hi) {
  lo = bins[2 * q];
  hi = bins[2 * q + 1];
  lo = lo < 0 ? 0 : (lo > F ? F : lo);
  hi = hi < lo ? lo : (hi > F ? F : hi);
}
__global__ __launch_bounds__(256) void k_band_sum(const float* __restrict__ v, const int* __restrict__ bins, double* __restrict__ out, int R, int F, int nb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= R * nb) return;
  const int r = i / nb, q = i - r * nb;
  int lo, hi;
  sp_band(bins, q, F, lo, hi);
  const float* row = v + (size_t)r * F;
  double s = 0.0;
  for (int f = lo; f < hi; ++f) s = s + (double)row[f];
  out[i] = s;
}
extern "C" int bx_band_sum(const float* values, const int* bins, double* out, int R, int F, int nb, bxStream stream) {
  BX_REQUIRE(R > 0 && F > 0 && nb > 0, "bx_band_sum: bad shape R=%d F=%d nb=%d", R, F, nb);
  BX_REQUIRE((long long)R * F < (1ll << 31) && (long long)R * nb < (1ll << 31), "bx_band_sum: R * F or R * nb beyond 32-bit offsets");
  BX_REQUIRE(values && bins && out, "bx_band_sum: null pointer");
  BX_REQUIRE(((uintptr_t)out & 7) == 0, "bx_band_sum: out must be 8-byte aligned");
  hipLaunchKernelGGL(k_band_sum, dim3(bx_ceil_div((long long)R * nb, 256)), dim3(256), 0, (hipStream_t)stream, values, bins, out, R, F, nb);
  BX_CHECK_LAUNCH("bx_band_sum");
  return BX_OK;
}

// ---- band-stopped rows ------------------------------------------------------------------------------------------------------------------
// A workgroup owns (output row, electrode, 256 time points).  An electrode the row does not select, and an empty band, are copied bit
// for bit.  Otherwise a thread owns one t: the band's bins, scaled by c_f (exact), pass through LDS SP_TILE at a time and the thread
// adds Re cos - Im sin in ascending f, the table index walked from (lo t) mod T by adding t; y = sum / T, out = fl32(double(x) - y).
template <bool TAB>
__global__ __launch_bounds__(256) void k_bandstop_rows(const float* __restrict__ x, const double* __restrict__ xre, const double* __restrict__ xim,
                                                       const sp_c* __restrict__ tw, const int* __restrict__ bins, float* __restrict__ out, int Chans, int T, int F,
                                                       int cells, int n0, int n, int tilesT) {
  extern __shared__ sp_c sp_lds[];
  sp_c* sX = sp_lds;                                   // [SP_TILE], then the table's image with TAB
  const int tt = blockIdx.x % tilesT, e = (blockIdx.x / tilesT) % Chans, rr = blockIdx.x / (tilesT * Chans);
  const int b = rr / n, j = n0 + (rr - b * n);
  const int q = cells == BX_SPECTRAL_CELLS_BAND ? j : j / Chans;
  const bool sel = cells == BX_SPECTRAL_CELLS_BAND || j - q * Chans == e;
  int lo, hi;
  sp_band(bins, q, F, lo, hi);
  const int t = tt * 256 + threadIdx.x;
  const size_t xrow = (size_t)b * Chans + e;
  const float* xr = x + xrow * T;
  float* o = out + ((size_t)rr * Chans + e) * T;
  if (!sel || lo >= hi) {                              // uniform over the workgroup
    if (t < T) o[t] = xr[t];
    return;
  }
  if (TAB) sp_stage_table(tw, T, sX + SP_TILE);
  const SpTabLds ltab{sX + SP_TILE};
  const int tc = t < T ? t : 0;
  int jj = (int)(((long long)lo * tc) % T);
  double s = 0.0;
  for (int f0 = lo; f0 < hi; f0 += SP_TILE) {
    const int m = hi - f0 < SP_TILE ? hi - f0 : SP_TILE;
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 256) {
      const double c = sp_cf(f0 + i, T);
      sX[i] = make_double2(c * xre[xrow * F + f0 + i], c * xim[xrow * F + f0 + i]);
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {
      const sp_c X = sX[i];
      const sp_c w = TAB ? ltab[jj] : tw[jj];
      s = fma(X.x, w.x, s);
      s = fma(-X.y, w.y, s);
      jj += tc;
      jj -= jj >= T ? T : 0;
    }
  }
  if (t < T) {
    const double y = s / (double)T;
    o[t] = (float)((double)xr[t] - y);
  }
}
extern "C" int bx_bandstop_rows(const float* x, const double* re, const double* im, const double* tw, const int* bins, float* out, int B, int Chans, int T, int nb,
                                int cells, int n0, int n, bxStream stream) {
  BX_REQUIRE(B > 0 && Chans > 0 && nb > 0, "bx_bandstop_rows: bad shape B=%d Chans=%d nb=%d", B, Chans, nb);
  const int rc = sp_shape_ok("bx_bandstop_rows", (long long)B * Chans, T);
  if (rc) return rc;
  BX_REQUIRE(cells == BX_SPECTRAL_CELLS_BAND || cells == BX_SPECTRAL_CELLS_ELECTRODE_BAND, "bx_bandstop_rows: unknown cells %d", cells);
  const long long N = cells == BX_SPECTRAL_CELLS_BAND ? nb : (long long)nb * Chans;
  BX_REQUIRE(n0 >= 0 && n >= 1 && (long long)n0 + n <= N, "bx_bandstop_rows: rows n0 = %d, n = %d outside 0..N = %lld", n0, n, N);
  const int tilesT = bx_ceil_div(T, 256);
  BX_REQUIRE((long long)B * n * Chans * T < (1ll << 31) && (long long)B * n * Chans * tilesT < (1ll << 31),
             "bx_bandstop_rows: B * n * Chans * T beyond 32-bit offsets");
  BX_REQUIRE(x && re && im && tw && bins && out, "bx_bandstop_rows: null pointer");
  BX_REQUIRE((((uintptr_t)tw & 15) | (((uintptr_t)re | (uintptr_t)im) & 7)) == 0, "bx_bandstop_rows: tw must be 16-byte, re and im 8-byte aligned");
  const int F = T / 2 + 1, grid = B * n * Chans * tilesT;
  const sp_c* tab = reinterpret_cast<const sp_c*>(tw);
  if ((SP_TILE + sp_padded(T)) * 16 <= SP_LDS)
    hipLaunchKernelGGL(k_bandstop_rows<true>, dim3(grid), dim3(256), (size_t)(SP_TILE + sp_padded(T)) * 16, (hipStream_t)stream, x, re, im, tab, bins, out, Chans, T, F, cells,
                       n0, n, tilesT);
  else
    hipLaunchKernelGGL(k_bandstop_rows<false>, dim3(grid), dim3(256), (size_t)SP_TILE * 16, (hipStream_t)stream, x, re, im, tab, bins, out, Chans, T, F, cells, n0,
                       n, tilesT);
  BX_CHECK_LAUNCH("bx_bandstop_rows");
  return BX_OK;
}
