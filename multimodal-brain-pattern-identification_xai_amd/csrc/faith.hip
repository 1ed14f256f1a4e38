// Deletion / insertion curves (the causal metric of RISE, Petsiuk et al., BMVC 2018) for any attribution map: the exact descending
// rank of every cell, the perturbed batches straight in the model's layouts, and the class curve with its area.  The forward
// passes between them are the model's own kernels.  See include/brainxai.h for the contract of each entry point.
#include "perturb_rows.h"

#define FAITH_MAX_N ((1 << 20) - 1)
#define RANK_WAVES 16                  // one 1024-thread workgroup per row; a wave owns a contiguous chunk of the row

// ---- rank: stable descending sort position of every cell ------------------------------------------------------------------------------
// Per-row LSD radix sort, four 8-bit passes, on key = ~(order-preserving image of the canonical value): ascending key order is
// descending value order, and a stable sort leaves ties in ascending flat index.  A pass is one launch, one workgroup per row:
//   count    each wave histograms its chunk into its own 256 LDS counters (integer adds: order-free);
//   scan     exclusive prefix over the 4096 counters in (digit, wave) order = where each wave's first cell of a digit goes;
//   scatter  a wave walks its chunk 64 cells at a time IN ORDER; lanes holding the same digit find each other with eight ballots,
//            take consecutive slots behind the wave's counter in lane order, and the last of them advances the counter.
// Nothing depends on scheduling: every cell's slot is a function of the row alone.  Pass 0 keys the values itself (flat index =
// position), pass 3 writes ranks[idx] = slot instead of another (key, idx) image.

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(1024) void k_rank_pass(const float* __restrict__ values, const uint32_t* __restrict__ kin, const uint32_t* __restrict__ iin,
                                                    uint32_t* __restrict__ kout, uint32_t* __restrict__ iout, int* __restrict__ ranks, int N,
                                                    int chunk, int shift) {
  __shared__ uint32_t cnt[256 * RANK_WAVES];                        // [digit][wave]
  __shared__ uint32_t wtot[RANK_WAVES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const size_t row = (size_t)blockIdx.x * N;
  const int lo = w * chunk < N ? w * chunk : N, hi = lo + chunk < N ? lo + chunk : N;
  auto key_at = [&](int i) -> uint32_t { return FIRST ? bx_rank_key(values[row + i]) : kin[row + i]; };
  for (int i = tid; i < 256 * RANK_WAVES; i += 1024) cnt[i] = 0u;
  __syncthreads();
  for (int i0 = lo; i0 < hi; i0 += 256) {
    uint32_t k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int i = i0 + u * 64 + lane; k[u] = key_at(i < hi ? i : hi - 1); }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * 64 + lane < hi) atomicAdd(&cnt[((k[u] >> shift) & 255u) * RANK_WAVES + w], 1u);
  }
  __syncthreads();
  {
    uint32_t c[4], s = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) { c[q] = cnt[tid * 4 + q]; s += c[q]; }
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t run = incl - s;
    for (int q = 0; q < w; ++q) run += wtot[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) { cnt[tid * 4 + q] = run; run += c[q]; }
  }
  __syncthreads();
  for (int i0 = lo; i0 < hi; i0 += 256) {
    uint32_t k[4], ix[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 64 + lane, ic = i < hi ? i : hi - 1;
      k[u] = key_at(ic);
      ix[u] = FIRST ? (uint32_t)ic : iin[row + ic];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool valid = i0 + u * 64 + lane < hi;
      const uint32_t d = (k[u] >> shift) & 255u;
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool on = (d >> bit) & 1u;
        const unsigned long long m = __ballot(valid && on);
        peers &= on ? m : ~m;
      }
      const int before = __popcll(peers & ((1ull << lane) - 1ull)), total = __popcll(peers);
      // the wave's counters are shared by its lanes: volatile accesses with wavefront-scope fences between the peers' reads, the last
      // peer's store and the next group's reads (LDS operations of one wave execute in order)
      volatile uint32_t* slot = &cnt[d * RANK_WAVES + w];
      uint32_t base = 0u;
      if (valid) base = *slot;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();                              // every peer has read the counter before the last one advances it
      if (valid && before == total - 1) *slot = base + (uint32_t)total;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (valid) {
        const uint32_t pos = base + (uint32_t)before;               // < N: the counters partition 0..N-1
        if (LAST) {
          if (ix[u] < (uint32_t)N) ranks[row + ix[u]] = (int)pos;
        } else if (pos < (uint32_t)N) {
          kout[row + pos] = k[u];
          iout[row + pos] = ix[u];
        }
      }
    }
  }
}

static int rank_shape_ok(const char* who, int B, int N) {
  BX_REQUIRE(B > 0 && N > 0, "%s: bad shape B=%d N=%d", who, B, N);
  if (N > FAITH_MAX_N) BX_FAIL(BX_EUNSUPPORTED, "%s: N = %d cells per row, supported 1..%d", who, N, FAITH_MAX_N);
  BX_REQUIRE((long long)B * N < (1ll << 31), "%s: B * N = %lld beyond 32-bit offsets", who, (long long)B * N);
  return BX_OK;
}
extern "C" size_t bx_rank_desc_workspace(int B, int N) {
  if (rank_shape_ok("bx_rank_desc_workspace", B, N) != BX_OK) return 0;
  return (size_t)B * N * 4 * sizeof(uint32_t);                      // two (key, index) images
}
extern "C" int bx_rank_desc(const float* values, int* ranks, int B, int N, void* workspace, size_t workspace_bytes, bxStream stream) {
  const int rc = rank_shape_ok("bx_rank_desc", B, N);
  if (rc) return rc;
  BX_REQUIRE(values && ranks && workspace, "bx_rank_desc: null pointer");
  if (workspace_bytes < bx_rank_desc_workspace(B, N))
    BX_FAIL(BX_EWORKSPACE, "bx_rank_desc: workspace of %zu bytes, need %zu", workspace_bytes, bx_rank_desc_workspace(B, N));
  BX_REQUIRE(((uintptr_t)workspace & 3) == 0, "bx_rank_desc: workspace not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t BN = (size_t)B * N;
  uint32_t* kA = (uint32_t*)workspace; uint32_t* iA = kA + BN; uint32_t* kB = iA + BN; uint32_t* iB = kB + BN;
  const int chunk = bx_ceil_div(bx_ceil_div(N, RANK_WAVES), 64) * 64;
  hipLaunchKernelGGL((k_rank_pass<true, false>), dim3(B), dim3(1024), 0, s, values, nullptr, nullptr, kA, iA, nullptr, N, chunk, 0);
  hipLaunchKernelGGL((k_rank_pass<false, false>), dim3(B), dim3(1024), 0, s, nullptr, kA, iA, kB, iB, nullptr, N, chunk, 8);
  hipLaunchKernelGGL((k_rank_pass<false, false>), dim3(B), dim3(1024), 0, s, nullptr, kB, iB, kA, iA, nullptr, N, chunk, 16);
  hipLaunchKernelGGL((k_rank_pass<false, true>), dim3(B), dim3(1024), 0, s, nullptr, kA, iA, nullptr, nullptr, ranks, N, chunk, 24);
  BX_CHECK_LAUNCH("bx_rank_desc");
  return BX_OK;
}

// ---- perturbed batches ----------------------------------------------------------------------------------------------------------------
// Row (b, j) carries curve point i0 + j with cut k = min(N, (i0 + j) * per): a cell whose rank is below the cut is REPLACED by the
// baseline (deletion) or is the only kind KEPT (insertion).  The kernels are perturb_rows.h's.
static int faith_window_ok(const char* who, int B, long long N, int per, int i0, int n, int kind) {
  BX_REQUIRE(B > 0 && N > 0, "%s: bad shape B=%d N=%lld", who, B, N);
  if (N > FAITH_MAX_N) BX_FAIL(BX_EUNSUPPORTED, "%s: N = %lld cells per sample, supported 1..%d", who, N, FAITH_MAX_N);
  BX_REQUIRE(per >= 1 && per <= N, "%s: per = %d cells per step outside 1..N = %lld", who, per, N);
  // a curve has steps + 1 <= N + 1 points and any number of them may sit at the clamped cut k = N ((steps - 1) * per >= N happens,
  // e.g. N = 7 with steps = 5): only the point index itself is bounded
  BX_REQUIRE(i0 >= 0 && n >= 1 && (long long)i0 + n - 1 <= N, "%s: points i0 = %d, n = %d outside 0..N = %lld (a curve has at most N steps)", who, i0, n, N);
  BX_REQUIRE(kind >= 0 && kind <= 2, "%s: baseline_kind %d (0 scalar, 1 per channel, 2 full tensor)", who, kind);
  return BX_OK;
}

// the rank of every cell is read once for the PERTURB_SPW rows of a group; a row compares it with its cut
struct FaithMask {
  struct Lds {};
  const int* ranks;
  int N, per, i0, insertion;
  __device__ __forceinline__ void stage(Lds&, int, int, int) const {}
  __device__ __forceinline__ int cell(int b, int idx, int, int) const { return ranks[(size_t)b * N + idx]; }
  __device__ __forceinline__ bool row(const Lds&, int r, int, int j0, int sj) const {
    const long long cut = (long long)(i0 + j0 + sj) * per;
    const bool below = (long long)r < (cut < N ? cut : (long long)N);
    return insertion ? below : !below;
  }
};
extern "C" int bx_faith_perturb_spec(const float* x, const int* ranks, const float* baseline, int baseline_kind, void* out, int B, int C, int H,
                                     int W, int Cp, int per, int i0, int n, int insertion, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  BX_REQUIRE(H > 0 && W > 0, "bx_faith_perturb_spec: bad shape H=%d W=%d", H, W);
  int rc = faith_window_ok("bx_faith_perturb_spec", B, (long long)H * W, per, i0, n, baseline_kind);
  if (rc) return rc;
  if ((rc = perturb_layout_ok("bx_faith_perturb_spec", "channels", C, Cp)) != BX_OK) return rc;
  if ((rc = perturb_rows_ok("bx_faith_perturb_spec", "B", B, n, H, W, Cp, dtype)) != BX_OK) return rc;
  BX_REQUIRE(x && ranks && baseline && out, "bx_faith_perturb_spec: null pointer");
  const FaithMask mask = {ranks, H * W, per, i0, insertion ? 1 : 0};
  BX_DISPATCH_DTYPE(dtype, T, perturb_launch_spec<T>(stream, x, baseline, baseline_kind, out, B, C, H, W, 0, n, mask));
  BX_CHECK_LAUNCH("bx_faith_perturb_spec");
  return BX_OK;
}

// the cell of element (ch, t) is ch * T + t for an electrode-by-time map and t for a time-column map
extern "C" int bx_faith_perturb_eeg(const float* x, const int* ranks, int map_rows, const float* baseline, int baseline_kind, float* out, int B,
                                    int Chans, int T, int per, int i0, int n, int insertion, bxStream stream) {
  BX_REQUIRE(Chans > 0 && T > 0 && (map_rows == Chans || map_rows == 1), "bx_faith_perturb_eeg: bad shape Chans=%d T=%d map_rows=%d (Chans or 1)", Chans, T, map_rows);
  BX_REQUIRE((long long)Chans * T < (1ll << 31), "bx_faith_perturb_eeg: Chans * T beyond 32-bit offsets");
  int rc = faith_window_ok("bx_faith_perturb_eeg", B, (long long)map_rows * T, per, i0, n, baseline_kind);
  if (rc) return rc;
  if ((rc = perturb_rows_ok("bx_faith_perturb_eeg", "B", B, n, Chans, T, 0, BX_F32)) != BX_OK) return rc;
  BX_REQUIRE(x && ranks && baseline && out, "bx_faith_perturb_eeg: null pointer");
  const FaithMask mask = {ranks, map_rows * T, per, i0, insertion ? 1 : 0};
  perturb_launch_eeg(stream, x, baseline, baseline_kind, out, B, Chans, T, map_rows, 0, n, mask);
  BX_CHECK_LAUNCH("bx_faith_perturb_eeg");
  return BX_OK;
}

// ---- curve and area ---------------------------------------------------------------------------------------------------------------------
// One thread per sample walks its P points in index order: curve[b, i] = exp(logp[b, i, c]) (or the log-probability itself), and
// auc = (sum - first / 2 - last / 2) / (P - 1) with the sum taken in fp64 over the fp32 points as stored.
__global__ __launch_bounds__(64) void k_faith_curve(const float* __restrict__ logp, const int* __restrict__ classes, float* __restrict__ curve,
                                                    double* __restrict__ auc, int B, int P, int K, int use_logprob) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int c = classes[b];
  c = c < 0 ? 0 : (c >= K ? K - 1 : c);
  double sum = 0.0;
  float first = 0.f, last = 0.f;
  for (int i = 0; i < P; ++i) {
    const float lp = logp[((size_t)b * P + i) * K + c];
    const float v = use_logprob ? lp : (float)exp((double)lp);     // fp64 exp, rounded once: the device's expf is a few ulp off at |lp| ~ 10
    curve[(size_t)b * P + i] = v;
    sum += (double)v;
    if (i == 0) first = v;
    last = v;
  }
  auc[b] = ((sum - (double)first / 2.0) - (double)last / 2.0) / (double)(P - 1);
}
extern "C" int bx_faith_curve(const float* logp, const int* classes, float* curve, double* auc, int B, int P, int K, int use_logprob, bxStream stream) {
  BX_REQUIRE(B > 0 && P >= 2 && K >= 1, "bx_faith_curve: bad shape B=%d P=%d (steps + 1 >= 2) K=%d", B, P, K);
  BX_REQUIRE((long long)B * P * K < (1ll << 31), "bx_faith_curve: B * P * K beyond 32-bit offsets");
  BX_REQUIRE(logp && classes && curve && auc, "bx_faith_curve: null pointer");
  hipLaunchKernelGGL(k_faith_curve, dim3(bx_ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, logp, classes, curve, auc, B, P, K, use_logprob ? 1 : 0);
  BX_CHECK_LAUNCH("bx_faith_curve");
  return BX_OK;
}
