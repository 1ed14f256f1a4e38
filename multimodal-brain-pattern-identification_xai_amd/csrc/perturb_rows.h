// The row writer of the perturb-and-predict attributions (deletion / insertion curves, RISE, occlusion, Score-CAM; LIME shares the
// host checks and the store): rows of an input in which every cell shows the input, the baseline or a blend of the two, written
// straight in the model's layouts.  One thread per pixel (k_perturb_spec) or per V time steps of one electrode (k_perturb_eeg);
// blockIdx.y walks groups of PERTURB_SPW rows, blockIdx.z walks samples; x and the baseline are read once per group.
//
// A method is a Mask, a small struct passed to the kernel by value (its geometry, pointers and the index of its first row):
//   struct Lds { ... };                                  what the workgroup stages in LDS (empty: nothing)
//   void stage(Lds&, int b, int j0, int n) const         called by every thread before the early exit; ends in a barrier if it stages
//   Cell cell(int b, int idx, int y, int x) const        once per thread and element: whatever the rows of a group share.  (y, x) is
//                                                         the element's cell of the map, idx = y * width + x
//   bool / float row(const Lds&, const Cell&, int b, int j0, int sj) const      row j0 + sj of the call: take x (bool), or the mask value m
// bool selects x or the baseline, so every bit of the result is the input's or the baseline's; float gives base + m * (x - base)
// and is instantiated only in files built with -ffp-contract=off (build.py), where the product and the sum round on their own.
#pragma once
#include "bx_common.h"

#define PERTURB_SPW 8                  // rows of one sample a workgroup writes for its 256 cells
#define PERTURB_MAX_C 4                // input channels of the internal layout (Cp = 8)

__device__ __forceinline__ float perturb_mix(bool take_x, bool, float xv, float bv, float) { return take_x ? xv : bv; }
__device__ __forceinline__ float perturb_mix(float m, bool live, float, float bv, float diff) { return live ? bv + m * diff : 0.f; }

// one pixel of row `row` in the internal layout (NHWC, 8 channels, 4..7 zero)
template <typename T>
__device__ __forceinline__ void perturb_store8(T* __restrict__ out, size_t row, int HW, int p, const float v4[PERTURB_MAX_C]) {
  float v[8];
#pragma unroll
  for (int c = 0; c < PERTURB_MAX_C; ++c) { v[c] = v4[c]; v[4 + c] = 0.f; }
  st8(out, (row * HW + p) * 8, v);
}

// x fp32 NCHW [.,C,H,W] -> rows [nb*n,H,W,8] in T, the expression of k_nchw_to_nhwc applied to the perturbed input, which is never
// built.  Sample b0 + blockIdx.z of x (and of a full-tensor baseline) goes to rows blockIdx.z * n ...
template <typename T, typename Mask>
__global__ __launch_bounds__(256) void k_perturb_spec(const float* __restrict__ x, const float* __restrict__ base, int kind, T* __restrict__ out, int HW,
                                                      int Wm, int C, int b0, int n, Mask mask) {
  __shared__ typename Mask::Lds lds;
  const int bl = blockIdx.z, b = b0 + bl, j0 = blockIdx.y * PERTURB_SPW, p = blockIdx.x * 256 + threadIdx.x;
  mask.stage(lds, b, j0, n);
  if (p >= HW) return;
  float xv[PERTURB_MAX_C], bv[PERTURB_MAX_C], diff[PERTURB_MAX_C];
#pragma unroll
  for (int c = 0; c < PERTURB_MAX_C; ++c) {
    const int cc = c < C ? c : 0;                                   // clamped, unconditional loads
    const float xc = x[((size_t)b * C + cc) * HW + p];
    const float bc = base[kind == 0 ? (size_t)0 : kind == 1 ? (size_t)cc : ((size_t)b * C + cc) * HW + p];
    xv[c] = c < C ? xc : 0.f;
    bv[c] = c < C ? bc : 0.f;
    diff[c] = c < C ? xc - bc : 0.f;
  }
  const int y = p / Wm;
  const auto cell = mask.cell(b, p, y, p - y * Wm);
  for (int sj = 0; sj < PERTURB_SPW && j0 + sj < n; ++sj) {
    const auto m = mask.row(lds, cell, b, j0, sj);
    float v[PERTURB_MAX_C];
#pragma unroll
    for (int c = 0; c < PERTURB_MAX_C; ++c) v[c] = perturb_mix(m, c < C, xv[c], bv[c], diff[c]);
    perturb_store8(out, (size_t)bl * n + j0 + sj, HW, p, v);
  }
}

// fp32 [.,1,Chans,T] -> [nb*n,1,Chans,T].  A thread owns V consecutive time steps of one electrode (V = 4 with 16-byte accesses when
// T % 4 == 0, else 1); element (ch, t) belongs to cell (ch, t) of an electrode-by-time map (map_rows = Chans) and to cell (0, t) of a
// time-column map (map_rows = 1).  cell() and row() are called once per time step q; what the V steps of a thread share (the row's
// window or shift, the map row's axis) is written once in the Mask and left to the compiler to compute once: after inlining the V calls
// repeat the same expressions.  Check a new Mask with tools/kernel_resources.py (registers, no scratch).
template <int V, typename Mask>
__global__ __launch_bounds__(256) void k_perturb_eeg(const float* __restrict__ x, const float* __restrict__ base, int kind, float* __restrict__ out,
                                                     int Chans, int T, int map_rows, int b0, int n, Mask mask) {
  __shared__ typename Mask::Lds lds;
  const int bl = blockIdx.z, b = b0 + bl, j0 = blockIdx.y * PERTURB_SPW, CT = Chans * T;
  const int e = (blockIdx.x * 256 + threadIdx.x) * V;
  mask.stage(lds, b, j0, n);
  if (e >= CT) return;
  const int ch = e / T, t = e - ch * T, y = map_rows == 1 ? 0 : ch;
  float xv[V], bv[V], diff[V];
  decltype(mask.cell(0, 0, 0, 0)) cell[V];
#pragma unroll
  for (int q = 0; q < V; ++q) {
    xv[q] = x[(size_t)b * CT + e + q];
    bv[q] = base[kind == 0 ? (size_t)0 : kind == 1 ? (size_t)ch : (size_t)b * CT + e + q];
    diff[q] = xv[q] - bv[q];
    cell[q] = mask.cell(b, y * T + t + q, y, t + q);
  }
  for (int sj = 0; sj < PERTURB_SPW && j0 + sj < n; ++sj) {
    float v[V];
#pragma unroll
    for (int q = 0; q < V; ++q) v[q] = perturb_mix(mask.row(lds, cell[q], b, j0, sj), true, xv[q], bv[q], diff[q]);
    float* dst = out + ((size_t)bl * n + j0 + sj) * CT + e;
    if (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[V > 1 ? 1 : 0], v[V > 2 ? 2 : 0], v[V > 3 ? 3 : 0]);
    else dst[0] = v[0];
  }
}

// ---- host side: the checks every perturb entry point makes, worded with the entry point's name, and the launches ----------------------
// `what` is "channels" or "input channels"
static inline int perturb_layout_ok(const char* who, const char* what, int C, int Cp) {
  if (C < 1 || C > PERTURB_MAX_C) BX_FAIL(BX_EUNSUPPORTED, "%s: %d %s, supported 1..%d (Cp = 8)", who, C, what, PERTURB_MAX_C);
  BX_REQUIRE(Cp == 8, "%s: Cp = %d, the internal layout of 1..4 channels has 8", who, Cp);
  return BX_OK;
}
// nb samples x n rows stay below 2^32 bytes and inside the grid.  Spectrogram rows have H x W pixels of Cp values in dtype, EEG rows
// (Cp = 0) H x W = Chans x T fp32 values; `samples` is the entry point's name for nb ("B" or "nb")
static inline int perturb_rows_ok(const char* who, const char* samples, int nb, int n, int H, int W, int Cp, int dtype) {
  const size_t cell_bytes = Cp ? Cp * bx_esize(dtype) : 4;
  BX_REQUIRE((unsigned long long)nb * n * H * W * cell_bytes < (1ull << 32) && bx_ceil_div(n, PERTURB_SPW) <= 65535 && nb <= 65535,
             "%s: output beyond 32-bit byte offsets (%s*n*%s = %lld %s); use fewer rows per call", who, samples, Cp ? "H*W" : "Chans*T",
             (long long)nb * n * H * W, Cp ? "pixels" : "values");
  return BX_OK;
}
static inline bool perturb_eeg_vec(int T, const void* x, const void* out) { return T % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0; }
static inline dim3 perturb_grid(long long cells, int cells_per_block, int n, int B) {
  return dim3(bx_ceil_div(cells, cells_per_block), bx_ceil_div(n, PERTURB_SPW), B);
}

template <typename T, typename Mask>
static void perturb_launch_spec(bxStream stream, const float* x, const float* base, int kind, void* out, int nb, int C, int H, int W, int b0, int n,
                                const Mask& mask) {
  hipLaunchKernelGGL((k_perturb_spec<T, Mask>), perturb_grid((long long)H * W, 256, n, nb), dim3(256), 0, (hipStream_t)stream, x, base, kind, (T*)out,
                     H * W, W, C, b0, n, mask);
}
template <typename Mask>
static void perturb_launch_eeg(bxStream stream, const float* x, const float* base, int kind, float* out, int nb, int Chans, int T, int map_rows, int b0,
                               int n, const Mask& mask) {
  const bool vec = perturb_eeg_vec(T, x, out);
  const dim3 grid = perturb_grid((long long)Chans * T, vec ? 1024 : 256, n, nb);
  if (vec) hipLaunchKernelGGL((k_perturb_eeg<4, Mask>), grid, dim3(256), 0, (hipStream_t)stream, x, base, kind, out, Chans, T, map_rows, b0, n, mask);
  else hipLaunchKernelGGL((k_perturb_eeg<1, Mask>), grid, dim3(256), 0, (hipStream_t)stream, x, base, kind, out, Chans, T, map_rows, b0, n, mask);
}
