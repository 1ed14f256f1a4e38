// Attribution reduce kernels and the EEG stacker.
//   bx_gradcam_reduce : canonical Grad-CAM channel reduce (the reference has no Grad-CAM)
//   bx_cam_reduce     : the same for Grad-CAM++ and Layer-CAM (bx_cam_head*: the last-stage form of all three methods)
//   bx_resize_bilinear: F.interpolate(mode='bilinear', align_corners=False) of the maps
//   bx_saliency_reduce: spec.grad.abs().max(dim=1)   reference XAI_Multimodality.py:3128-3129
//   bx_eeg_stack_iir  : _EEGTransformer.transform     reference root/src/data/dataset.py:73-104,125-131
#include "bx_common.h"

// One workgroup per map.  Phase 1: w[c] = mean_p G[p][c] -- every thread owns 8 channels of a pixel
// slice (16-byte loads, coalesced along C), LDS [slots][C] then a fixed-order column sum.
// Phase 2: raw[p] = sum_c w[c] A[p][c] -- one wave per pixel, 8 channels per lane, DPP/shuffle reduce.
template <typename T>
__global__ __launch_bounds__(256) void k_gradcam(const T* __restrict__ A, const T* __restrict__ G, float* __restrict__ cam,
                                                  float* __restrict__ wout, int HW, int C, int maps_per_act, int relu) {
  extern __shared__ float sm[];  // part[slots*C] | w[C]
  const int m = blockIdx.x;
  const int ncg = C / 8, slots = 256 / ncg;
  float* part = sm;
  float* w = sm + (size_t)slots * C;
  const T* g = G + (size_t)m * HW * C;
  const T* a = A + (size_t)(m / maps_per_act) * HW * C;
  const int cg = threadIdx.x % ncg, slot = threadIdx.x / ncg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = slot; p < HW; p += slots) {
    float v[8];
    ld8(g, (size_t)p * C + cg * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[slot * C + cg * 8 + j] = acc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int sl = 0; sl < slots; ++sl) s += part[sl * C + c];
    s /= (float)HW;
    w[c] = s;
    if (wout) wout[(size_t)m * C + c] = s;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int p = wave; p < HW; p += 4) {
    float s = 0.f;
    for (int c0 = lane * 8; c0 < C; c0 += 512) {
      float v[8];
      ld8(a, (size_t)p * C + c0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(w[c0 + j], v[j], s);
    }
    s = wave_sum(s);
    if (lane == 0) cam[(size_t)m * HW + p] = relu ? fmaxf(s, 0.f) : s;
  }
}

// Grad-CAM++ and Layer-CAM channel reduce (bx_cam_reduce; its method 0 launches k_gradcam above).  One workgroup per map.
//   Grad-CAM++  phase 0: S[c] = sum_p A[p][c] -- k_gradcam's column sum, over A (each of an activation's maps_per_act maps forms it
//                        again: its second and later reads of A come from L2, and the reduce needs no workspace);
//               phase 1: w[c] = sum_p campp_term(G[p][c], S[c]), the same column sum over G;  then raw[p] = sum_c w[c] A[p][c].
//   Layer-CAM   raw[p] = sum_c max(G[p][c], 0) A[p][c]: one streaming pass over A and G.
// The position reduce puts a position's channels on min(C/8, 64) neighbouring lanes (16-byte loads along C) and 64 / that many
// positions on a wave, four position groups per trip, segmented butterfly sum (fixed order: the result does not vary from run to run).
template <typename T, typename F>
__device__ __forceinline__ void cam_colsum(const T* x, int HW, int C, float* part, float* dst, F f) {
  const int ncg = C / 8, slots = 256 / ncg, cg = threadIdx.x % ncg, slot = threadIdx.x / ncg;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p0 = slot; p0 < HW; p0 += 4 * slots) {        // four 16-byte loads in flight per trip (clamped index, masked add)
    float v[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) { const int p = p0 + u * slots; ld8(x, (size_t)(p < HW ? p : HW - 1) * C + cg * 8, v[u]); }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += p0 + u * slots < HW ? f(v[u][j], cg * 8 + j) : 0.f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[slot * C + cg * 8 + j] = acc[j];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int sl = 0; sl < slots; ++sl) s += part[sl * C + c];
    dst[c] = s;
  }
  __syncthreads();
}

template <typename T, int METHOD>
__global__ __launch_bounds__(256) void k_cam(const T* __restrict__ A, const T* __restrict__ G, float* __restrict__ cam,
                                             float* __restrict__ wout, int HW, int C, int maps_per_act, int relu) {
  extern __shared__ float sm[];  // Grad-CAM++: part[2048] | S[C] | w[C]
  const int m = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const T* g = G + (size_t)m * HW * C;
  const T* a = A + (size_t)(m / maps_per_act) * HW * C;
  float* w = sm + 2048 + C;
  if constexpr (METHOD == BX_CAM_GRADCAM_PP) {
    float* S = sm + 2048;
    cam_colsum(a, HW, C, sm, S, [](float v, int) { return v; });
    cam_colsum(g, HW, C, sm, w, [&](float v, int c) { return campp_term(v, S[c]); });
    if (wout)
      for (int c = threadIdx.x; c < C; c += 256) wout[(size_t)m * C + c] = w[c];
  }
  const int lpp = C / 8 < 64 ? C / 8 : 64, ppw = 64 / lpp, sub = lane / lpp, cg = lane - sub * lpp;
  const int ngrp = (HW + ppw - 1) / ppw;                  // position groups; wave takes groups wave, wave + 4, ...
  for (int g0 = wave; g0 < ngrp; g0 += 16) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = cg * 8; c0 < C; c0 += 512) {
      float av[4][8], gv[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = (g0 + 4 * u) * ppw + sub;
        const size_t i = (size_t)(p < HW ? p : HW - 1) * C + c0;
        ld8(a, i, av[u]);
        if constexpr (METHOD == BX_CAM_LAYERCAM) ld8(g, i, gv[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) s[u] = fmaf(METHOD == BX_CAM_LAYERCAM ? fmaxf(gv[u][j], 0.f) : w[c0 + j], av[u][j], s[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      for (int o = lpp >> 1; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o, 64);
      const int p = (g0 + 4 * u) * ppw + sub;
      if (cg == 0 && g0 + 4 * u < ngrp && p < HW) cam[(size_t)m * HW + p] = relu ? fmaxf(s[u], 0.f) : s[u];
    }
  }
}

// What the CAM entry points check first, in this order: the method, Layer-CAM's absent channel weights, the dtype.
static int cam_check(const char* who, int method, const void* weights_out, int dtype) {
  BX_REQUIRE(method >= BX_CAM_GRADCAM && method <= BX_CAM_LAYERCAM, "%s: unknown method %d (0 = Grad-CAM, 1 = Grad-CAM++, 2 = Layer-CAM)", who, method);
  BX_REQUIRE(method != BX_CAM_LAYERCAM || !weights_out, "%s: Layer-CAM has no channel weights (weights_out must be NULL)", who);
  BX_DTYPE_OK(dtype);
  return BX_OK;
}
static bool cam_c_ok(int C) { return C % 8 == 0 && C >= 8 && C <= 2048 && 256 % (C / 8) == 0; }

extern "C" int bx_cam_reduce(const void* A, const void* G, float* cam, float* weights_out, int n_maps, int maps_per_act, int HW, int C,
                             int method, int relu, int dtype, bxStream stream) {
  const char* who = method == BX_CAM_GRADCAM ? "bx_gradcam_reduce" : "bx_cam_reduce";
  if (const int e = cam_check(who, method, weights_out, dtype)) return e;
  BX_REQUIRE(A && G && cam && n_maps > 0 && HW > 0 && maps_per_act > 0 && n_maps % maps_per_act == 0, "%s: bad arguments", who);
  BX_REQUIRE(cam_c_ok(C), "%s: C=%d must be 8*2^k, <= 2048", who, C);
  hipStream_t s = (hipStream_t)stream;
  if (method == BX_CAM_GRADCAM) {
    const size_t lds = ((size_t)(256 / (C / 8)) * C + C) * sizeof(float);
    BX_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL((k_gradcam<T>), dim3(n_maps), dim3(256), lds, s, (const T*)A, (const T*)G, cam, weights_out, HW, C, maps_per_act, relu));
  } else if (method == BX_CAM_GRADCAM_PP) {
    const size_t lds = ((size_t)2048 + 2 * C) * sizeof(float);
    BX_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL((k_cam<T, BX_CAM_GRADCAM_PP>), dim3(n_maps), dim3(256), lds, s, (const T*)A, (const T*)G, cam, weights_out, HW, C,
                         maps_per_act, relu));
  } else {
    BX_DISPATCH_DTYPE(dtype, T,
      hipLaunchKernelGGL((k_cam<T, BX_CAM_LAYERCAM>), dim3(n_maps), dim3(256), 0, s, (const T*)A, (const T*)G, cam, (float*)nullptr, HW, C,
                         maps_per_act, relu));
  }
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
extern "C" int bx_gradcam_reduce(const void* A, const void* G, float* cam, float* weights_out, int n_maps, int maps_per_act,
                                 int HW, int C, int relu, int dtype, bxStream stream) {
  return bx_cam_reduce(A, G, cam, weights_out, n_maps, maps_per_act, HW, C, BX_CAM_GRADCAM, relu, dtype, stream);
}

// ------------------------------------------------------------------------------------------------
// Grad-CAM at the LAST stage of the multimodal model in ONE launch (one workgroup per sample).  The stage output A feeds
// GAP -> fc -> LogSoftmax -> [cat with the EEG log-probs] -> fc1 -> ReLU -> fc2 -> LogSoftmax directly, so the gradient of a class
// score with respect to A is the same at every position, dgap/HW, and the Grad-CAM channel weights are w = dgap/HW: the kernel
// runs the two heads forward, their backward for every requested class (class_mode -2: all N classes, -1: the sample's arg-max
// class, >= 0: that class), and the channel reduce cam[p] = sum_k w[k] A[p][k] -- what used to be 4 library launches plus 7
// framework launches (argmax, scatter, four repeat_interleave, ...) and a materialised gradient tensor [B*N, HW, C].
// Sweep form (bx_gradcam_head_sweep; GcExtra.ef / .up non-null): the EEG branch's dense layer + LogSoftmax (a launch of its own per
// batch otherwise) and the bilinear up-sampling of the finished map (a second launch and a round trip of the small maps) run here too.
struct GcExtra { const float* ef; const float* dw; const float* db; int Fe; float* up; int h, w, H, W; };
template <typename T, int METHOD = BX_CAM_GRADCAM>
__global__ __launch_bounds__(256) void k_gradcam_head(const T* __restrict__ A, const float* __restrict__ e_lp, const float* __restrict__ fcw,
                                                       const float* __restrict__ fcb, const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out_lp,
                                                       float* __restrict__ cam, float* __restrict__ raw, float* __restrict__ wout,
                                                       int HW, int C, int N, int Hd, int class_mode, int relu, GcExtra ex) {
  extern __shared__ float sm[];
  float* gap = sm;                 // [C]
  float* w = gap + C;              // [C]
  float* hid = w + C;              // [Hd]
  float* dhid = hid + Hd;          // [Hd]
  float* cat = dhid + Hd;          // [2N]   EEG log-probs | spectrogram log-probs
  float* lp = cat + 2 * N;         // [N]    fused output log-probs
  float* dz = lp + N;              // [N]
  float* ds = dz + N;              // [N]
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* scam = ds + N + (size_t)(256 / (C / 8)) * C;       // [HW] the finished map, for the in-kernel up-sampling (sweep form only)
  const T* a = A + (size_t)b * HW * C;
  const float inv_hw = 1.f / (float)HW;
  // ---- forward: GAP.  C/8 channel groups x (256 / (C/8)) position slots run in parallel (16-byte loads, coalesced along C),
  // then a fixed-order column sum over the slots
  {
    const int ncg = C / 8, slots = 256 / ncg;                // host guarantees C = 8 * 2^k <= 2048
    float* part = ds + N;                                     // [slots][C] scratch behind the small vectors
    const int cg = tid % ncg, slot = tid / ncg;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p0 = slot; p0 < HW; p0 += 8 * slots) {         // eight 16-byte loads in flight per trip (clamped index, masked add)
      float v[8][8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int p = p0 + u * slots; ld8(a, (size_t)(p < HW ? p : HW - 1) * C + cg * 8, v[u]); }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += p0 + u * slots < HW ? v[u][j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[slot * C + cg * 8 + j] = acc[j];
    __syncthreads();
    for (int k = tid; k < C; k += 256) {
      float t = 0.f;
      for (int sl = 0; sl < slots; ++sl) t += part[sl * C + k];
      gap[k] = t * inv_hw;
    }
  }
  if (ex.ef) {                                             // EEG head: dense over the branch's features, then LogSoftmax
    const float* f = ex.ef + (size_t)b * ex.Fe;
    for (int n = wave; n < N; n += 4) {
      float acc = 0.f;
      for (int k0 = lane; k0 < ex.Fe; k0 += 256) {
        float wv[4], fv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int k = k0 + 64 * u < ex.Fe ? k0 + 64 * u : 0; wv[u] = ex.dw[(size_t)n * ex.Fe + k]; fv[u] = f[k]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = k0 + 64 * u < ex.Fe ? fmaf(wv[u], fv[u], acc) : acc;
      }
      acc = wave_sum(acc);
      if (lane == 0) dz[n] = acc + ex.db[n];              // logits parked in dz
    }
    __syncthreads();
    if (tid == 0) bx_lsm_row(dz, N, cat);
  } else if (tid < N) cat[tid] = e_lp[(size_t)b * N + tid];
  __syncthreads();
  // ---- fc + LogSoftmax (spectrogram branch head)
  for (int n = wave; n < N; n += 4) {
    float acc = 0.f;
    for (int k0 = lane; k0 < C; k0 += 256) {
      float wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) wv[u] = fcw[(size_t)n * C + (k0 + 64 * u < C ? k0 + 64 * u : 0)];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = k0 + 64 * u < C ? fmaf(wv[u], gap[k0 + 64 * u], acc) : acc;
    }
    acc = wave_sum(acc);
    if (lane == 0) ds[n] = acc + fcb[n];             // logits parked in ds
  }
  __syncthreads();
  if (tid == 0) bx_lsm_row(ds, N, cat + N);
  __syncthreads();
  // ---- fusion head forward
  for (int j = tid; j < Hd; j += 256) {                 // (rows of small matrices: all of a batch's loads before the first FMA -- a rolled
    float acc = b1[j];                                  //  loop is one L2 round trip per element, and nothing else runs in this workgroup)
    for (int i0 = 0; i0 < 2 * N; i0 += 16) {
      float wv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) wv[u] = w1[(size_t)j * 2 * N + (i0 + u < 2 * N ? i0 + u : 2 * N - 1)];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = i0 + u < 2 * N ? fmaf(wv[u], cat[i0 + u], acc) : acc;
    }
    hid[j] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  for (int n = wave; n < N; n += 4) {
    float acc = 0.f;
    for (int j = lane; j < Hd; j += 64) acc = fmaf(w2[(size_t)n * Hd + j], hid[j], acc);
    acc = wave_sum(acc);
    if (lane == 0) dz[n] = acc + b2[n];
  }
  __syncthreads();
  if (tid == 0) {
    bx_lsm_row(dz, N, lp);
    if (out_lp && blockIdx.y == 0)
      for (int n = 0; n < N; ++n) out_lp[(size_t)b * N + n] = lp[n];
  }
  __syncthreads();
  int first = class_mode, nm = 1;
  if (class_mode == -2) { first = 0; nm = N; }
  else if (class_mode == -1) {                          // first maximum, like torch.argmax
    first = 0;
    for (int n = 1; n < N; ++n) if (lp[n] > lp[first]) first = n;
  }
  // all classes: the launcher gives every (sample, class) its own workgroup (grid.y = N; the forward part above is recomputed, the
  // stage output comes from L2 for all but the first of a sample's workgroups) -- one workgroup per sample walked the classes
  // serially on a quarter of the chip (64 workgroups, 66 us per batch of 64)
  const int ci_lo = gridDim.y > 1 ? (int)blockIdx.y : 0, ci_hi = gridDim.y > 1 ? (int)blockIdx.y + 1 : nm;
  for (int ci = ci_lo; ci < ci_hi; ++ci) {
    const int c = first + ci;
    // ---- backward of the fused head for the score y_c = lp[c]:  d logits = onehot(c) - softmax
    if (tid < N) {                                       // (1 - p_c) as the sum of the other probabilities: no cancellation when p_c -> 1
      float others = 0.f;
      for (int jn = 0; jn < N; ++jn) if (jn != c) others += expf(lp[jn]);
      dz[tid] = tid == c ? others : -expf(lp[tid]);
    }
    __syncthreads();
    for (int j = tid; j < Hd; j += 256) {
      float acc = 0.f;
      for (int n0 = 0; n0 < N; n0 += 8) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = w2[(size_t)(n0 + u < N ? n0 + u : N - 1) * Hd + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = n0 + u < N ? fmaf(wv[u], dz[n0 + u], acc) : acc;
      }
      dhid[j] = hid[j] > 0.f ? acc : 0.f;
    }
    __syncthreads();
    for (int i = wave; i < N; i += 4) {                  // gradient w.r.t. the spectrogram branch's log-probs
      float acc = 0.f;
      for (int j = lane; j < Hd; j += 64) acc = fmaf(w1[(size_t)j * 2 * N + N + i], dhid[j], acc);
      acc = wave_sum(acc);
      if (lane == 0) ds[i] = acc;
    }
    __syncthreads();
    if (tid == 0) bx_lsm_bwd(ds, cat + N, N, dz);       // through the spectrogram head's LogSoftmax (dz is free again)
    __syncthreads();
    float* wdst = wout ? wout + ((size_t)b * nm + ci) * C : nullptr;
    for (int k = tid; k < C; k += 256) {                 // through fc and the mean over positions: w = W_fc^T dz_s / HW
      float acc = 0.f;
      for (int n0 = 0; n0 < N; n0 += 8) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = fcw[(size_t)(n0 + u < N ? n0 + u : N - 1) * C + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = n0 + u < N ? fmaf(wv[u], dz[n0 + u], acc) : acc;
      }
      acc *= inv_hw;
      if constexpr (METHOD == BX_CAM_LAYERCAM) {          // (the gradient is acc at every position, and S[k] = HW gap[k])
        acc = fmaxf(acc, 0.f);
      } else if constexpr (METHOD == BX_CAM_GRADCAM_PP) {
        acc = (float)HW * campp_term(acc, (float)HW * gap[k]);
      }
      w[k] = acc;
      if (wdst) wdst[k] = acc;
    }
    __syncthreads();
    const size_t mbase = ((size_t)b * nm + ci) * HW;
    if (C <= 512) {
      // a position's channels sit on C/8 neighbouring lanes (one 16-byte load each), 64 / (C/8) positions per wave at a time, eight
      // such groups in flight per trip; the channel weights of a lane are loop-invariant registers; segmented butterfly sum
      const int lpp = C / 8, ppw = 64 / lpp, sub = lane / lpp, cg = lane - sub * lpp;
      float wr[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) wr[j] = w[cg * 8 + j];
      const int ngrp = (HW + ppw - 1) / ppw;                 // position groups of the map; wave takes groups wave, wave + 4, ...
      for (int g0 = wave; g0 < ngrp; g0 += 4 * 8) {
        float v[8][8], acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int p = (g0 + 4 * u) * ppw + sub;
          ld8(a, (size_t)(p < HW ? p : HW - 1) * C + cg * 8, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float t = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) t = fmaf(wr[j], v[u][j], t);
          for (int o = lpp >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
          acc[u] = t;
        }
        if (cg == 0) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int p = (g0 + 4 * u) * ppw + sub;
            if (g0 + 4 * u < ngrp && p < HW) {
              const float cv = relu ? fmaxf(acc[u], 0.f) : acc[u];
              if (cam) cam[mbase + p] = cv;
              if (raw) raw[mbase + p] = acc[u];
              if (ex.up) scam[p] = cv;
            }
          }
        }
      }
    } else {
      for (int p = wave; p < HW; p += 4) {
        float acc = 0.f;
        for (int k0 = lane * 8; k0 < C; k0 += 512) {
          float v[8];
          ld8(a, (size_t)p * C + k0, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc = fmaf(w[k0 + j], v[j], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) {
          const float cv = relu ? fmaxf(acc, 0.f) : acc;
          if (cam) cam[mbase + p] = cv;
          if (raw) raw[mbase + p] = acc;
          if (ex.up) scam[p] = cv;
        }
      }
    }
    __syncthreads();
    if (ex.up) {                                         // F.interpolate(bilinear, align_corners=False) of this map: four columns per thread
      const int W4 = ex.W / 4;
      const float sy = (float)ex.h / (float)ex.H, sx = (float)ex.w / (float)ex.W;
      float4* dst = reinterpret_cast<float4*>(ex.up + ((size_t)b * nm + ci) * ex.H * ex.W);
      if (256 % W4 == 0) {                               // a thread keeps its four columns: the column interpolation is loop-invariant
        const int X4 = tid % W4, rows_per_trip = 256 / W4;
        int x0[4], x1[4]; float lx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bilinear_src(X4 * 4 + j, sx, ex.w, x0[j], x1[j], lx[j]);
        for (int Y = tid / W4; Y < ex.H; Y += rows_per_trip) {
          int y0, y1; float ly;
          bilinear_src(Y, sy, ex.h, y0, y1, ly);
          const float* r0 = scam + y0 * ex.w;
          const float* r1 = scam + y1 * ex.w;
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = (1.f - ly) * ((1.f - lx[j]) * r0[x0[j]] + lx[j] * r0[x1[j]]) + ly * ((1.f - lx[j]) * r1[x0[j]] + lx[j] * r1[x1[j]]);
          dst[Y * W4 + X4] = make_float4(o[0], o[1], o[2], o[3]);
        }
      } else {
        for (int i = tid; i < ex.H * W4; i += 256) {
          const int X4 = i % W4, Y = i / W4;
          int y0, y1; float ly;
          bilinear_src(Y, sy, ex.h, y0, y1, ly);
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int x0, x1; float lx;
            bilinear_src(X4 * 4 + j, sx, ex.w, x0, x1, lx);
            o[j] = (1.f - ly) * ((1.f - lx) * scam[y0 * ex.w + x0] + lx * scam[y0 * ex.w + x1]) + ly * ((1.f - lx) * scam[y1 * ex.w + x0] + lx * scam[y1 * ex.w + x1]);
          }
          dst[i] = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
      __syncthreads();
    }
  }
}

// The two head forms: the sizes (dims: the form's own positive counts), then the launch of the method's and dtype's kernel.
static int cam_head_sizes(const char* who, bool dims, int C, int N, int Hd) {
  BX_REQUIRE(dims && cam_c_ok(C) && N > 0 && N <= 64 && Hd > 0 && Hd <= 4096,
             "%s: unsupported sizes (C=%d must be 8*2^k <= 2048, N=%d <= 64, Hd=%d <= 4096)", who, C, N, Hd);
  return BX_OK;
}
static size_t cam_head_lds(int C, int N, int Hd) { return ((size_t)2 * C + 2 * Hd + 5 * N + (size_t)(256 / (C / 8)) * C) * sizeof(float); }
#define BX_CAM_HEAD_LAUNCH(...) BX_DISPATCH_CAM(method, M, BX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((k_gradcam_head<T, M>), __VA_ARGS__)))

extern "C" int bx_cam_head(const void* A, const float* eeg_logp, const float* fc_w, const float* fc_b, const float* w1, const float* b1,
                           const float* w2, const float* b2, float* out_logp, float* cam, float* raw, float* weights_out, int B, int HW,
                           int C, int N, int Hd, int class_mode, int method, int relu, int dtype, bxStream stream) {
  const char* who = method == BX_CAM_GRADCAM ? "bx_gradcam_head" : "bx_cam_head";
  if (const int e = cam_check(who, method, weights_out, dtype)) return e;
  BX_REQUIRE(A && eeg_logp && fc_w && fc_b && w1 && b1 && w2 && b2 && cam, "%s: null pointer", who);
  if (const int e = cam_head_sizes(who, B > 0 && HW > 0, C, N, Hd)) return e;
  BX_REQUIRE(class_mode >= -2 && class_mode < N, "%s: class %d out of range", who, class_mode);
  const GcExtra none = {nullptr, nullptr, nullptr, 0, nullptr, 0, 0, 0, 0};
  BX_CAM_HEAD_LAUNCH(dim3(B, class_mode == -2 ? N : 1), dim3(256), cam_head_lds(C, N, Hd), (hipStream_t)stream, (const T*)A, eeg_logp, fc_w, fc_b,
                     w1, b1, w2, b2, out_logp, cam, raw, weights_out, HW, C, N, Hd, class_mode, relu, none);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
extern "C" int bx_gradcam_head(const void* A, const float* eeg_logp, const float* fc_w, const float* fc_b, const float* w1, const float* b1,
                               const float* w2, const float* b2, float* out_logp, float* cam, float* raw, float* weights_out, int B, int HW,
                               int C, int N, int Hd, int class_mode, int relu, int dtype, bxStream stream) {
  return bx_cam_head(A, eeg_logp, fc_w, fc_b, w1, b1, w2, b2, out_logp, cam, raw, weights_out, B, HW, C, N, Hd, class_mode, BX_CAM_GRADCAM,
                     relu, dtype, stream);
}
extern "C" int bx_cam_head_sweep(const void* A, const float* eeg_feat, const float* dense_w, const float* dense_b, int Fe, const float* fc_w,
                                 const float* fc_b, const float* w1, const float* b1, const float* w2, const float* b2, float* out_logp,
                                 float* maps, int B, int h, int w, int C, int N, int Hd, int H, int W, int class_mode, int method, int relu,
                                 int dtype, bxStream stream) {
  const char* who = method == BX_CAM_GRADCAM ? "bx_gradcam_head_sweep" : "bx_cam_head_sweep";
  if (const int e = cam_check(who, method, nullptr, dtype)) return e;
  BX_REQUIRE(A && eeg_feat && dense_w && dense_b && fc_w && fc_b && w1 && b1 && w2 && b2 && maps, "%s: null pointer", who);
  const int HW = h * w;
  if (const int e = cam_head_sizes(who, B > 0 && h > 0 && w > 0 && Fe > 0, C, N, Hd)) return e;
  BX_REQUIRE(H > 0 && W > 0 && W % 4 == 0 && ((uintptr_t)maps & 15) == 0, "%s: W must be a multiple of 4 and maps 16-byte aligned", who);
  BX_REQUIRE(class_mode >= -2 && class_mode < N, "%s: class %d out of range", who, class_mode);
  const size_t lds = cam_head_lds(C, N, Hd) + HW * sizeof(float);
  BX_REQUIRE(lds <= 64 * 1024, "%s: stage output of %d positions x %d channels does not fit the workgroup's LDS", who, HW, C);
  const GcExtra ex = {eeg_feat, dense_w, dense_b, Fe, maps, h, w, H, W};
  BX_CAM_HEAD_LAUNCH(dim3(B, class_mode == -2 ? N : 1), dim3(256), lds, (hipStream_t)stream, (const T*)A, (const float*)nullptr, fc_w,
                     fc_b, w1, b1, w2, b2, out_logp, (float*)nullptr, (float*)nullptr, (float*)nullptr, HW, C, N, Hd, class_mode, relu, ex);
  BX_CHECK_LAUNCH(who);
  return BX_OK;
}
extern "C" int bx_gradcam_head_sweep(const void* A, const float* eeg_feat, const float* dense_w, const float* dense_b, int Fe, const float* fc_w,
                                     const float* fc_b, const float* w1, const float* b1, const float* w2, const float* b2, float* out_logp,
                                     float* maps, int B, int h, int w, int C, int N, int Hd, int H, int W, int class_mode, int relu, int dtype,
                                     bxStream stream) {
  return bx_cam_head_sweep(A, eeg_feat, dense_w, dense_b, Fe, fc_w, fc_b, w1, b1, w2, b2, out_logp, maps, B, h, w, C, N, Hd, H, W, class_mode,
                           BX_CAM_GRADCAM, relu, dtype, stream);
}

// ------------------------------------------------------------------------------------------------
__global__ void k_resize_bilinear(const float* __restrict__ src, float* __restrict__ dst, long long n, int h, int w, int H, int W,
                                  float sy, float sx) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int X = (int)(i % W);
    const long long r = i / W;
    const int Y = (int)(r % H);
    const long long m = r / H;
    int y0, y1, x0, x1; float ly, lx;
    bilinear_src(Y, sy, h, y0, y1, ly);
    bilinear_src(X, sx, w, x0, x1, lx);
    const float* s = src + m * h * w;
    dst[i] = (1.f - ly) * ((1.f - lx) * s[y0 * w + x0] + lx * s[y0 * w + x1]) + ly * ((1.f - lx) * s[y1 * w + x0] + lx * s[y1 * w + x1]);
  }
}
// four consecutive output columns per thread (one 16-byte store), 32-bit index arithmetic, one trip per thread: the scalar
// kernel above spent its time in 64-bit divisions and 4-byte stores (46 us for 384 maps of 128 x 256 = 1.1 TB/s of writes)
__global__ __launch_bounds__(256) void k_resize_bilinear4(const float* __restrict__ src, float* __restrict__ dst, unsigned n4, int h, int w, int H,
                                                          int W4, float sy, float sx) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n4) return;
  const unsigned X4 = i % (unsigned)W4, r = i / (unsigned)W4;
  const unsigned Y = r % (unsigned)H, m = r / (unsigned)H;
  int y0, y1; float ly;
  bilinear_src((int)Y, sy, h, y0, y1, ly);
  const float* s0 = src + (size_t)m * h * w + (size_t)y0 * w;
  const float* s1 = src + (size_t)m * h * w + (size_t)y1 * w;
  float a0[4], a1[4], b0[4], b1[4], lxs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int x0, x1;
    bilinear_src((int)(X4 * 4 + j), sx, w, x0, x1, lxs[j]);
    a0[j] = s0[x0]; a1[j] = s0[x1]; b0[j] = s1[x0]; b1[j] = s1[x1];
  }
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (1.f - ly) * ((1.f - lxs[j]) * a0[j] + lxs[j] * a1[j]) + ly * ((1.f - lxs[j]) * b0[j] + lxs[j] * b1[j]);
  reinterpret_cast<float4*>(dst)[i] = make_float4(o[0], o[1], o[2], o[3]);
}
extern "C" int bx_resize_bilinear(const float* src, float* dst, int N, int h, int w, int H, int W, bxStream stream) {
  BX_REQUIRE(src && dst && N > 0 && h > 0 && w > 0 && H > 0 && W > 0, "bx_resize_bilinear: bad arguments");
  const long long n = (long long)N * H * W;
  if (W % 4 == 0 && n / 4 < (1ll << 31) && ((uintptr_t)dst & 15) == 0) {
    hipLaunchKernelGGL(k_resize_bilinear4, dim3(bx_ceil_div(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, (unsigned)(n / 4), h, w, H,
                       W / 4, (float)h / (float)H, (float)w / (float)W);
    BX_CHECK_LAUNCH("bx_resize_bilinear");
    return BX_OK;
  }
  const int grid = bx_ceil_div(n, 256) > 4096 ? 4096 : bx_ceil_div(n, 256);
  hipLaunchKernelGGL(k_resize_bilinear, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, dst, n, h, w, H, W,
                     (float)h / (float)H, (float)w / (float)W);
  BX_CHECK_LAUNCH("bx_resize_bilinear");
  return BX_OK;
}

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void k_saliency(const T* __restrict__ g, float* __restrict__ out, long long npix, int C, int Cs, float scale) {
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    float m = 0.f;
    for (int c0 = 0; c0 < C; c0 += 8) {
      float v[8];
      ld8(g, (size_t)p * Cs + c0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) if (c0 + j < C) m = fmaxf(m, fabsf(v[j]));
    }
    out[p] = scale * m;
  }
}
extern "C" int bx_saliency_reduce(const void* g, float* out, int B, int HW, int C, int Cs, float scale, int dtype, bxStream stream) {
  BX_DTYPE_OK(dtype);
  BX_REQUIRE(g && out && B > 0 && HW > 0 && C > 0 && C <= Cs && Cs % 8 == 0, "bx_saliency_reduce: bad arguments");
  const long long npix = (long long)B * HW;
  const int grid = bx_ceil_div(npix, 256) > 4096 ? 4096 : bx_ceil_div(npix, 256);
  BX_DISPATCH_DTYPE(dtype, T,
    hipLaunchKernelGGL((k_saliency<T>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)g, out, npix, C, Cs, scale));
  BX_CHECK_LAUNCH("bx_saliency_reduce");
  return BX_OK;
}

// ------------------------------------------------------------------------------------------------
// EEG stacker: one thread per (sample, channel) row runs the direct-form-II-transposed recurrence
// scipy.signal.lfilter uses, in fp64, over the clipped / NaN-zeroed / scaled fp32 samples, and keeps
// every `step`-th output.  Lanes of a wave are neighbouring channels of a sample, so the per-step
// loads of one wave touch a few contiguous 76-byte records.
#define IIR_MAX_ORDER 8
struct IirCoef { double b[IIR_MAX_ORDER + 1]; double a[IIR_MAX_ORDER + 1]; };
__global__ void k_eeg_stack_iir(const float* __restrict__ raw, const int* __restrict__ chan, float* __restrict__ out, int nrows,
                                int L, int Craw, int C, IirCoef k, int order, int step, float clip, float inv_scale) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrows) return;
  const int b = row / C, c = row % C;
  const int col = chan ? chan[c] : c;
  const float* src = raw + (size_t)b * L * Craw + col;
  const int Lout = (L + step - 1) / step;
  float* dst = out + (size_t)row * Lout;
  double z[IIR_MAX_ORDER];
#pragma unroll
  for (int i = 0; i < IIR_MAX_ORDER; ++i) z[i] = 0.0;
  for (int n0 = 0; n0 < L; n0 += 8) {               // eight samples per trip: their loads are in flight together
    float raw8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) raw8[j] = n0 + j < L ? src[(size_t)(n0 + j) * Craw] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = n0 + j;
      if (n < L) {
        float xv = fminf(fmaxf(raw8[j], -clip), clip);   // np.clip keeps NaN; fminf/fmaxf drop it -> handle below
        if (raw8[j] != raw8[j]) xv = 0.f;                // np.nan_to_num(nan=0)
        const double x = (double)(xv * inv_scale);
        const double y = z[0] + k.b[0] * x;
#pragma unroll
        for (int i = 0; i < IIR_MAX_ORDER - 1; ++i)
          if (i < order - 1) z[i] = z[i + 1] + k.b[i + 1] * x - k.a[i + 1] * y;
        z[order - 1] = k.b[order] * x - k.a[order] * y;
        if (n % step == 0) dst[n / step] = (float)y;
      }
    }
  }
}
// ------------------------------------------------------------------------------------------------
// The same filter as a CHUNKED SCAN (round 2).  One thread per row above is 1 216 threads walking 10 000 samples each
// (19 waves on a 256-CU chip, 1.9 ms per 64-sample batch = 0.3 % of the HBM rate).  The recurrence is linear,
//     z' = A z + Bx,   y = z[0] + b0 x,        A = shift - a e0^T   (direct form II transposed, as scipy.signal.lfilter runs it)
// so a row is cut into chunks of S samples, one THREAD per (channel, chunk):
//   phase A  every chunk runs the recurrence from a ZERO state over its S samples (inputs staged once per workgroup into LDS with
//            coalesced 16-byte loads, already clipped / NaN-zeroed / scaled in fp32), keeps its decimated zero-state outputs in
//            registers and leaves its end state in LDS;
//   phase B  the true state entering chunk j is z_in[j+1] = A^S z_in[j] + (end state of chunk j): a short chain of ORDER x ORDER
//            products over the chunks in front of it inside the workgroup;
//   phase C  y[n] = y_zero_state[n] + e0^T A^n z_in  for the kept samples (rows of e0^T A^(m*step) precomputed on the host).
// A workgroup covers G chunks of one sample; what came before its window enters through Kc extra WARM-UP chunks in front of it,
// run from a zero state: the filter's memory decays like |pole|^n (0.795 for the reference's 4th-order 20 Hz Butterworth), and
// the host picks Kc so that ||A^(Kc*S)|| < 1e-13 -- below fp64 resolution of the outputs -- or falls back to the sequential kernel
// (filters with slow poles, e.g. the montage chain's 0.5 Hz band edge at radius 0.998, never take this path).  The first
// workgroup of a row reads zeros in its warm-up chunks: the exact zero initial state of lfilter.  All arithmetic stays fp64.
#define SCAN_MAX_KEEP 16
struct IirScan {
  double b[IIR_MAX_ORDER + 1], a[IIR_MAX_ORDER + 1];
  double AS[IIR_MAX_ORDER][IIR_MAX_ORDER];          // A^S
  double P[SCAN_MAX_KEEP][IIR_MAX_ORDER];           // e0^T A^(m*step), m < S/step
};
template <int ORDER, int STEP, int KEEP>
__global__ __launch_bounds__(512) void k_eeg_stack_scan(const float* __restrict__ raw, const int* __restrict__ chan, float* __restrict__ out, int L,
                                                         int Lout, int Craw, int C, IirScan k, int G, int Kc, float clip, float scale) {
  constexpr int S = STEP * KEEP;
  extern __shared__ float tile[];                    // [4 + G*S*Craw] staged inputs (later: [C][R*KEEP] outputs) | zs[G][C][ORDER] doubles
  const int R = G - Kc, w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int rows = G * S;
  const long long t_first = ((long long)w * R - Kc) * S;                  // time of tile row 0 (negative in the first workgroup)
  const long long gstart = ((long long)b * L + t_first) * Craw;           // float index of tile row 0 in `raw`
  const int shift = (int)(((gstart % 4) + 4) % 4);                         // tile_f[q] <-> raw[gstart - shift + q]: 16-byte aligned loads
  const long long gbase = gstart - shift;
  double* zs = reinterpret_cast<double*>(tile + (((size_t)rows * Craw + 4 + 3) / 4 * 4 + 4));
  // valid element range of the tile (times 0 <= t < L); everything else is zero input
  const long long r_lo = t_first < 0 ? -t_first : 0;
  const long long r_hi = (long long)L - t_first < rows ? (long long)L - t_first : rows;
  const int q_lo = shift + (int)r_lo * Craw, q_hi = shift + (int)(r_hi > 0 ? r_hi : 0) * Craw;
  const int nq4 = (shift + rows * Craw + 3) / 4;
  const int i_lo = (q_lo + 3) / 4, i_hi = q_hi / 4;                        // 16-byte groups that lie entirely inside the valid range
  const float4* g4 = reinterpret_cast<const float4*>(raw + gbase);
  auto prep = [&](float e) {                                               // reference dataset.py:88-90 in fp32, as numpy does it
    float xv = fminf(fmaxf(e, -clip), clip);                               // np.clip keeps NaN; fminf/fmaxf drop it -> handled next
    if (e != e) xv = 0.f;                                                  // np.nan_to_num(nan=0)
    return xv / scale;
  };
  for (int i0 = tid; i0 < nq4; i0 += 512 * 4) {                            // 4 x 16-byte loads per thread in flight per trip
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 512;
      const int ic = (i >= i_lo && i < i_hi) ? i : i_lo;                   // clamped, always valid: an unconditional load, selected afterwards
      v[u] = i_lo < i_hi ? g4[ic] : make_float4(0.f, 0.f, 0.f, 0.f);       // (the outer condition is workgroup-uniform)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 512;
      if (i < nq4) {
        const bool ok = i >= i_lo && i < i_hi;
        reinterpret_cast<float4*>(tile)[i] = ok ? make_float4(prep(v[u].x), prep(v[u].y), prep(v[u].z), prep(v[u].w)) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  __syncthreads();
  if (tid < 8) {                                                           // the (at most 3 + 3) valid elements in front of / behind the full groups
    const int q = (tid < 4 ? 4 * (i_lo - 1) : 4 * i_hi) + (tid & 3);
    if (q >= q_lo && q < q_hi && !(q >= 4 * i_lo && q < 4 * i_hi)) tile[q] = prep(raw[gbase + q]);
  }
  __syncthreads();
  const int j = tid / C, c = tid - j * C;                                 // lanes of a wave: neighbouring channels (LDS banks), then chunks
  const bool active = j < G;
  double z[ORDER], y0[KEEP];
#pragma unroll
  for (int i = 0; i < ORDER; ++i) z[i] = 0.0;
  if (active) {
    const float* src = tile + shift + (size_t)j * S * Craw + (chan ? chan[c] : c);
#pragma unroll
    for (int m = 0; m < KEEP; ++m) {
#pragma unroll
      for (int q = 0; q < STEP; ++q) {
        const double x = (double)src[(m * STEP + q) * Craw];
        const double y = z[0] + k.b[0] * x;
#pragma unroll
        for (int i = 0; i < ORDER - 1; ++i) z[i] = z[i + 1] + k.b[i + 1] * x - k.a[i + 1] * y;
        z[ORDER - 1] = k.b[ORDER] * x - k.a[ORDER] * y;
        if (q == 0) y0[m] = y;
      }
    }
#pragma unroll
    for (int i = 0; i < ORDER; ++i) zs[((size_t)j * C + c) * ORDER + i] = z[i];
  }
  __syncthreads();                                                        // end states visible; the input tile is dead from here on
  float* otile = tile;                                                    // [C][R*KEEP]
  if (active) {
    double zi[ORDER];
#pragma unroll
    for (int i = 0; i < ORDER; ++i) zi[i] = 0.0;
    for (int p = 0; p < j; ++p) {                                         // z_in[p+1] = A^S z_in[p] + end_state[p]
      double t[ORDER];
#pragma unroll
      for (int r = 0; r < ORDER; ++r) {
        double acc = zs[((size_t)p * C + c) * ORDER + r];
#pragma unroll
        for (int q = 0; q < ORDER; ++q) acc += k.AS[r][q] * zi[q];
        t[r] = acc;
      }
#pragma unroll
      for (int r = 0; r < ORDER; ++r) zi[r] = t[r];
    }
    if (j >= Kc) {
#pragma unroll
      for (int m = 0; m < KEEP; ++m) {
        double y = y0[m];
#pragma unroll
        for (int q = 0; q < ORDER; ++q) y += k.P[m][q] * zi[q];
        otile[(size_t)c * R * KEEP + (j - Kc) * KEEP + m] = (float)y;
      }
    }
  }
  __syncthreads();
  const int o_first = w * R * KEEP, per = R * KEEP;                       // this workgroup's outputs: [o_first, o_first + per) of every row
  for (int i = tid; i < C * per; i += 512) {
    const int cc = i / per, o = i - cc * per;
    if (o_first + o < Lout) out[((size_t)b * C + cc) * Lout + o_first + o] = otile[i];
  }
}

// host: A^n helpers in plain doubles (ORDER <= 8)
static void scan_matmul(int n, const double* X, const double* Y, double* Z) {
  double T[IIR_MAX_ORDER * IIR_MAX_ORDER];
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      double acc = 0.0;
      for (int q = 0; q < n; ++q) acc += X[r * n + q] * Y[q * n + c];
      T[r * n + c] = acc;
    }
  for (int i = 0; i < n * n; ++i) Z[i] = T[i];
}
template <int ORDER, int STEP, int KEEP>
static int launch_stack_scan(const float* raw, const int* chan, float* out, int B, int L, int Craw, int C, const double* bn, const double* an,
                             float clip, float scale, hipStream_t stream) {
  constexpr int S = STEP * KEEP;
  if (C > 512 || ((uintptr_t)raw & 15) != 0) return 0;
  const int G = 512 / C;
  double A[ORDER * ORDER], Pw[ORDER * ORDER], Astep[ORDER * ORDER];
  for (int r = 0; r < ORDER; ++r)
    for (int c = 0; c < ORDER; ++c) A[r * ORDER + c] = (c == 0 ? -an[r + 1] : 0.0) + (c == r + 1 ? 1.0 : 0.0);
  IirScan k;
  for (int i = 0; i <= IIR_MAX_ORDER; ++i) { k.b[i] = i <= ORDER ? bn[i] : 0.0; k.a[i] = i <= ORDER ? an[i] : 0.0; }
  for (int i = 0; i < ORDER * ORDER; ++i) { Pw[i] = (i / ORDER == i % ORDER) ? 1.0 : 0.0; Astep[i] = Pw[i]; }
  for (int q = 0; q < STEP; ++q) scan_matmul(ORDER, Astep, A, Astep);                     // A^STEP
  for (int m = 0; m < KEEP; ++m) {                                                        // Pw = A^(m*STEP); row 0 = e0^T A^(m*STEP)
    for (int q = 0; q < ORDER; ++q) k.P[m][q] = Pw[q];
    scan_matmul(ORDER, Pw, Astep, Pw);
  }
  for (int r = 0; r < ORDER; ++r)
    for (int c = 0; c < ORDER; ++c) k.AS[r][c] = Pw[r * ORDER + c];                       // A^S
  // warm-up length: smallest Kc with ||A^(Kc*S)||_max < 1e-13
  double M[ORDER * ORDER];
  for (int i = 0; i < ORDER * ORDER; ++i) M[i] = Pw[i];
  int Kc = 1;
  for (;; ++Kc) {
    double mx = 0.0;
    for (int i = 0; i < ORDER * ORDER; ++i) mx = fmax(mx, fabs(M[i]));
    if (mx < 1e-13) break;
    if (!(mx < 1e6) || Kc >= G - 1) return 0;                                            // slow or unstable poles: sequential kernel
    scan_matmul(ORDER, M, Pw, M);
  }
  const int R = G - Kc;
  const size_t tile_f = ((size_t)G * S * Craw + 4 + 3) / 4 * 4 + 4;
  const size_t lds = tile_f * sizeof(float) + (size_t)G * C * ORDER * sizeof(double);
  if (lds > 160 * 1024 || (size_t)C * R * KEEP > tile_f) return 0;
  static size_t attr_set = 0;
  if (lds > 64 * 1024 && lds > attr_set) {
    if (hipFuncSetAttribute((const void*)k_eeg_stack_scan<ORDER, STEP, KEEP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 0;
    attr_set = lds;
  }
  const int nwg = bx_ceil_div(L, R * S);
  hipLaunchKernelGGL((k_eeg_stack_scan<ORDER, STEP, KEEP>), dim3(nwg, B), dim3(512), lds, stream, raw, chan, out, L, (L + STEP - 1) / STEP, Craw, C, k,
                     G, Kc, clip, scale);
  return 1;
}

extern "C" int bx_eeg_stack_iir(const float* raw, const int* channel_index, float* out, int B, int L, int Craw, int C,
                                const double* b_host, const double* a_host, int order, int step, float clip, float scale,
                                bxStream stream) {
  BX_REQUIRE(raw && out && b_host && a_host && B > 0 && L > 0 && C > 0 && Craw >= 1, "bx_eeg_stack_iir: bad arguments");
  BX_REQUIRE(order >= 1 && order <= IIR_MAX_ORDER && step >= 1 && scale != 0.f, "bx_eeg_stack_iir: order must be 1..%d", IIR_MAX_ORDER);
  BX_REQUIRE(channel_index || C <= Craw, "bx_eeg_stack_iir: C > Craw without a channel index");
  IirCoef k;
  const double a0 = a_host[0];
  BX_REQUIRE(a0 != 0.0, "bx_eeg_stack_iir: a[0] == 0");
  for (int i = 0; i <= IIR_MAX_ORDER; ++i) { k.b[i] = i <= order ? b_host[i] / a0 : 0.0; k.a[i] = i <= order ? a_host[i] / a0 : 0.0; }
  BX_REQUIRE(B <= 65535, "bx_eeg_stack_iir: batch %d exceeds the grid's y extent", B);
  // the reference's configuration (4th order, keep every 5th sample) takes the chunked scan; anything else, or a filter whose
  // memory is too long for a warm-up, the one-thread-per-row recurrence
  if (order == 4 && step == 5 && launch_stack_scan<4, 5, 8>(raw, channel_index, out, B, L, Craw, C, k.b, k.a, clip, scale, (hipStream_t)stream)) {
    BX_CHECK_LAUNCH("bx_eeg_stack_iir (scan)");
    return BX_OK;
  }
  const int nrows = B * C;
  hipLaunchKernelGGL(k_eeg_stack_iir, dim3(bx_ceil_div(nrows, 64)), dim3(64), 0, (hipStream_t)stream, raw, channel_index, out,
                     nrows, L, Craw, C, k, order, step, clip, 1.f / scale);
  BX_CHECK_LAUNCH("bx_eeg_stack_iir");
  return BX_OK;
}
