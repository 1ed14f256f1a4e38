/* brainxai.h -- C ABI of libbrainxai.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * multimodal brain-pattern training + attribution hot path.
 *
 * The reference (KC-decoder/Multimodal-Brain-Pattern-Identification_XAI) has NO native code and no
 * FFI: its "native boundary" for this path is torch -> ATen -> cuDNN/cuBLAS.  Each entry point
 * below therefore cites the torch op chain of the reference it replaces
 * (M  = root/src/models/models.py, NB = root/jupyter_notebooks/XAI_Multimodality.py,
 *  DS = root/src/data/dataset.py, DDP = root/src/training/training_distributed.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the current HIP device unless marked host;
 *   - the caller owns every buffer including workspaces; the library never allocates, frees
 *     or retains pointers past a call; no call synchronises the device;
 *   - all launches go to the hipStream_t passed as `stream` (void* to keep hip headers out);
 *   - activations are channels-last: [B, H, W, C] (NHWC) for the 2-D CNN, [B, F, Chans, T]
 *     (NCHW, as the reference) for the EEG branch;
 *   - `dtype` is the STORAGE type of activations: BX_F32 or BX_BF16; arithmetic accumulates in
 *     fp32 always; parameters, parameter gradients and statistics are fp32;
 *   - return 0 on success, a negative BX_E* otherwise; bx_last_error_string() (thread-local)
 *     says why.  Nothing throws or aborts across this boundary.
 */
#ifndef BRAINXAI_H
#define BRAINXAI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BX_VERSION 100

enum { BX_F32 = 0, BX_BF16 = 1 };
enum { BX_POOL_MAX = 0, BX_POOL_AVG = 1 };
enum { BX_OK = 0, BX_EINVAL = -1, BX_EDTYPE = -2, BX_EALIGN = -3, BX_EWORKSPACE = -4, BX_EHIP = -5,
       BX_EUNSUPPORTED = -6 };
/* conv algorithm selector: 0 = library default, 1 = direct VALU (any dtype), 2 = MFMA implicit GEMM */
enum { BX_ALGO_AUTO = 0, BX_ALGO_DIRECT = 1, BX_ALGO_MFMA = 2 };
/* epilogue flags of bx_conv3x3 */
enum { BX_EPI_RELU = 1, BX_EPI_MASK_BITS = 2 };   /* MASK_BITS: relu_mask_src is the bit form written by bx_conv3x3_pair (MFMA path, Ci <= 32) */

typedef void* bxStream;

int bx_version(void);
const char* bx_last_error_string(void);

/* ---- layout ------------------------------------------------------------------------------- */
/* fp32 NCHW [B,C,H,W] -> dtype NHWC [B,H,W,Cp], channels C..Cp-1 zero.  Replaces the implicit
 * NCHW hand-off of DataLoader batches into Block.forward (M:62-63, NB:1595-1598). */
int bx_nchw_to_nhwc(const float* src, void* dst, int B, int C, int H, int W, int Cp, int dtype, bxStream stream);
/* dtype NHWC [B,H,W,Cs] -> fp32 NCHW [B,C,H,W] (first C channels). */
int bx_nhwc_to_nchw(const void* src, float* dst, int B, int C, int H, int W, int Cs, int dtype, bxStream stream);

/* ---- 3x3 convolution, stride 1, pad 1  (nn.Conv2d + F.relu, M:49-51,64-66; autograd bwd) ---- */
/* Pack fp32 OIHW weights [Cout,Cin,3,3] for bx_conv3x3.
 *   transpose_flip = 0: forward operand   Wp[tap][cin][cout]            (cin padded to Cin_p)
 *   transpose_flip = 1: data-gradient operand Wp[tap][cout][cin] = W[cout][cin][8-tap]
 * `packed_f32` ([9][I_p][O_p] fp32) is always written; `packed_mfma` (may be NULL) receives the
 * bf16 MFMA-fragment layout (see csrc/conv3x3_mfma.hip). I_p/O_p = channel counts rounded up to 8/16. */
int bx_conv3x3_pack(const float* w_oihw, float* packed_f32, void* packed_mfma, int Cout, int Cin,
                    int I_p, int O_p, int transpose_flip, bxStream stream);
/* bytes of the MFMA operand for padded dims (0 when the MFMA path does not cover them). */
size_t bx_conv3x3_packed_mfma_bytes(int I_p, int O_p);
/* fp32 STORAGE on the bf16 matrix cores (csrc/conv3x3_split.hip): every fp32 operand is split x = h + m + l (three bf16, 24
 * significand bits) and a product runs as the six MFMAs whose partial products reach 2^-18 of the largest, into the fp32
 * accumulator -- fp32-grade results (see the file's header).  bx_conv3x3_pack_split writes the weight operand in that layout
 * (images h, m, l; bx_conv3x3_packed_split_bytes, 0 when the path does not cover the padded dims); hand it to bx_conv3x3 /
 * bx_conv3x3_carry as `packed_mfma` with dtype BX_F32.  Same torch ops as bx_conv3x3_pack (M:49-51,64-66). */
size_t bx_conv3x3_packed_split_bytes(int I_p, int O_p);
int bx_conv3x3_pack_split(const float* w_oihw, void* packed_split, int Cout, int Cin, int I_p, int O_p, int transpose_flip,
                          bxStream stream);
/* All MFMA weight operands of a model in ONE launch.  `jobs_device` is a device array of njobs descriptors sorted by
 * block_begin (job j owns launch blocks [block_begin_j, block_begin_{j+1})); total_blocks = end of the last job. */
typedef struct {
  const void* w_oihw;      /* fp32 [Cout,Cin,3,3] */
  void* packed_mfma;       /* bx_conv3x3_packed_mfma_bytes(I_p, O_p) bytes (bx_conv3x3_packed_split_bytes with the split bit) */
  int Cout, Cin, I_p, O_p, transpose_flip, block_begin;   /* transpose_flip: bit 0 = data-gradient operand, bit 1 = split (fp32-storage) layout */
} bxPackJob;
int bx_conv3x3_pack_many(const bxPackJob* jobs_device, int njobs, int total_blocks, bxStream stream);
/* The same launch also converts the batch: src fp32 NCHW [B,C,H,W] -> dst bf16 NHWC [B,H,W,Cp] (what bx_nchw_to_nhwc does;
 * the two are independent and both sit at the start of every training step). */
int bx_conv3x3_pack_many_layout(const bxPackJob* jobs_device, int njobs, int total_blocks, const float* src_nchw,
                                void* dst_nhwc_bf16, int B, int C, int H, int W, int Cp, bxStream stream);
/* Evaluation sweeps (Grad-CAM over a dataset, integrated-gradients passes): njobs may be 0 (total_blocks 0, jobs_device ignored) when
 * no parameter changed since the operands were last packed -- the launch is then the layout conversion alone -- and the batch's address
 * may come from a DEVICE slot (src_slot != NULL: *src_slot is read by the kernel, src_nchw is ignored), so that a captured graph can be
 * replayed on the caller's batch without copying it into a static buffer (bx_store_u64x2 fills the slot, stream-ordered). */
int bx_conv3x3_pack_layout_ex(const bxPackJob* jobs_device, int njobs, int total_blocks, const float* src_nchw,
                              const float* const* src_slot, void* dst_nhwc_bf16, int B, int C, int H, int W, int Cp, bxStream stream);
/* The launch that opens a training step of the multimodal model (reference forward NB:1095-1105 with nn.Dropout in both
 * branches): packing, the optional layout conversion (src_nchw / dst_nhwc_bf16 both NULL: none) and bx_seed_next2's work
 * (both branches' dropout counters advance, out_a / out_b receive the seeds of this forward pass) in one launch. */
int bx_conv3x3_pack_many_step(const bxPackJob* jobs_device, int njobs, int total_blocks, const float* src_nchw,
                              void* dst_nhwc_bf16, int B, int C, int H, int W, int Cp, uint64_t* state_a, uint64_t* out_a,
                              uint64_t* state_b, uint64_t* out_b, bxStream stream);
/* conv1 + ReLU and conv2 + ReLU of a stage-1 Block (models.py:64-65) in ONE launch: conv1's output tile stays in LDS and is
 * written to y1 only when y1 != NULL (a backward pass will read it; evaluation-mode passes hand NULL).  Built for bf16 storage and
 * 8 (padded) -> 16 -> 16 channels (bx_conv3x3_pair_supported); results are bit-identical to two bx_conv3x3 calls with BX_EPI_RELU.
 * x [B,H,W,C0_p], y1 / y2 [B,H,W,C1]; packed*_mfma from bx_conv3x3_pack / _pack_many (forward operands).  Also built for
 * 16 -> 32 -> 32 and 32 -> 64 -> 64.  mask1 / mask2 (nullable, only with y1): the ReLU decisions of y1 / y2 as bits, uint8 [B,H,W,C1/4], bit r of byte q =
 * channel 4q + r is positive -- what the layers' data gradients read instead of the activations (bx_conv3x3 with BX_EPI_MASK_BITS:
 * 1/8 of the bytes in the HBM-bound early stages). */
int bx_conv3x3_pair_supported(int C0_p, int C1, int C2, int dtype);
int bx_conv3x3_pair(const void* x, const void* packed1_mfma, const float* bias1, const void* packed2_mfma, const float* bias2,
                    void* y1, void* y2, unsigned char* mask1, unsigned char* mask2, int B, int H, int W, int C0_p, int C1, int C2,
                    int dtype, bxStream stream);
/* y = epi(conv3x3(x, Wp) + bias);  x [B,H,W,Ci] -> y [B,H,W,Co], both `dtype`.
 *   bias (fp32 [Co]) may be NULL; flags & BX_EPI_RELU applies max(.,0);
 *   relu_mask_src (dtype [B,H,W,Co], may be NULL): y *= (relu_mask_src > 0)  -- the ReLU backward
 *     of the layer that produced the tensor whose gradient this call computes;
 *   addend (dtype [B,H,W,Co], may be NULL) is added last (skip-path gradient).
 * Forward uses (bias, RELU); data-gradient uses the transpose_flip pack + relu_mask_src/addend.
 * `packed_mfma` is the MFMA operand in the layout of `dtype`: bx_conv3x3_pack's for BX_BF16, bx_conv3x3_pack_split's for BX_F32
 * (algo AUTO takes the MFMA path whenever it is given and the shape is covered, else the direct kernel on packed_f32). */
int bx_conv3x3(const void* x, const float* packed_f32, const void* packed_mfma, const float* bias,
               const void* relu_mask_src, const void* addend, void* y,
               int B, int H, int W, int Ci, int Co, int dtype, int flags, int algo, bxStream stream);
/* Weight/bias gradient: dW[Cout,Cin,3,3] = sum_p X[p+tap] (x) dZ[p], db = sum_p dZ[p]  (fp32 out,
 * overwritten).  x [B,H,W,Ci_p], dz [B,H,W,Co].  Cin = logical input channels (<= Ci_p). */
size_t bx_conv3x3_wgrad_workspace(int B, int H, int W, int Ci_p, int Co, int dtype, int algo);
int bx_conv3x3_wgrad(const void* x, const void* dz, float* dw_oihw, float* dbias, int B, int H, int W,
                     int Cin, int Ci_p, int Co, int dtype, int algo, void* workspace, size_t workspace_bytes,
                     bxStream stream);
/* Chained form: the fixed-order sum of a layer's weight-gradient partials (a ~6 us launch of its own, 15 per training step)
 * rides in the NEXT layer's launch instead.  *pending (zero-initialised before the first call) describes partials that still
 * have to be summed: a valid *pending is reduced by this call's launch and then overwritten with this layer's; the caller
 * must give consecutive calls DIFFERENT workspaces (the pending partials live in the previous one), keep that workspace and
 * the previous dw/dbias alive until the next call, and end the chain with bx_conv3x3_wgrad_finish (e.g. at the end of
 * backward).  Paths that cannot carry a reduce (fp32 / direct kernels) finish the chain themselves. */
typedef struct {
  const void* partial; float* dw; float* db;
  int nsplit, Cin, Co, ma, nb, ztiles, nfrag4, valid;
} bxWgradPending;
int bx_conv3x3_wgrad_chained(const void* x, const void* dz, float* dw_oihw, float* dbias, int B, int H, int W, int Cin,
                             int Ci_p, int Co, int dtype, int algo, void* workspace, size_t workspace_bytes,
                             bxWgradPending* pending, bxStream stream);
int bx_conv3x3_wgrad_finish(bxWgradPending* pending, bxStream stream);
/* bx_conv3x3 that also ends a weight-gradient chain: a valid *pending is summed by extra workgroups of THIS launch (the
 * last weight gradient of a Block's backward is followed by that layer's data gradient, which then carries the sum
 * instead of a reduce launch of its own); *pending is invalid on return.  Paths that cannot carry it (fp32 / direct
 * kernels) finish the chain with a separate launch first.  Same arguments and results as bx_conv3x3 otherwise. */
int bx_conv3x3_carry(const void* x, const float* packed_f32, const void* packed_mfma, const float* bias,
                     const void* relu_mask_src, const void* addend, void* y, int B, int H, int W, int Ci, int Co,
                     int dtype, int flags, int algo, bxWgradPending* pending, bxStream stream);
/* bx_conv3x3_carry with up to three pending sums (npending = 1..3): every valid pending[i] is summed by extra workgroups of THIS
 * launch, in list order, each exactly as bx_conv3x3_carry would sum it alone; all are invalid on return.  A refused call
 * (rc != BX_OK) leaves the descriptors valid. */
int bx_conv3x3_carry_many(const void* x, const float* packed_f32, const void* packed_mfma, const float* bias,
                          const void* relu_mask_src, const void* addend, void* y, int B, int H, int W, int Ci, int Co,
                          int dtype, int flags, int algo, bxWgradPending* pending, int npending, bxStream stream);
/* The weight gradients of n = 1..3 layers of one Block (same B, H, W, bf16 storage) in ONE launch.  Every layer must be a shape of
 * the tile-owner kernel (Ci_p % 32 == 0, Co % 32 == 0: bx_conv3x3_wgrad_group_supported); list the heaviest layer first.
 * The launch sums nothing: pending[i] (i < n) must be invalid on entry (a valid one is refused, wherever its partials live, so one
 * inside `workspace` can never be overwritten) and describes layer i's partials on return -- hand the array
 * to bx_conv3x3_carry_many (or finish each with bx_conv3x3_wgrad_finish).  dw / db are then bit for bit those of
 * bx_conv3x3_wgrad_chained whose sum was carried.  The partials live in `workspace` (bx_conv3x3_wgrad_group_workspace bytes; 0 =
 * refused), which must stay alive and unused until the sums have run.  Errors launch nothing and leave `pending` as it was. */
typedef struct {
  const void* x; const void* dz;   /* [B,H,W,Ci_p], [B,H,W,Co] */
  float* dw; float* db;            /* [Co,Cin,3,3], [Co] (db may be NULL) */
  int Cin, Ci_p, Co;
} bxWgradGroupLayer;
int bx_conv3x3_wgrad_group_supported(int n, const int* Ci_p, const int* Co, int W, int dtype);
size_t bx_conv3x3_wgrad_group_workspace(const bxWgradGroupLayer* layers, int n, int B, int H, int W, int dtype);
int bx_conv3x3_wgrad_group(const bxWgradGroupLayer* layers, int n, int B, int H, int W, int dtype, void* workspace,
                           size_t workspace_bytes, bxWgradPending* pending, bxStream stream);
/* Stage 1's backward, bf16 storage: the data AND weight gradient of a 16 -> 16 conv3x3 layer in one pass over dz (one kernel).
 *   dz [B,H,W,16] = dZ_L, xl [B,H,W,16] = X_L = relu(z_{L-1}) (the layer's input), packed_flip = bx_conv3x3_pack's data-gradient
 *   operand (transpose_flip) of W_L.
 *   dzo != NULL, x0 == NULL: dzo = conv(dz, flipped W_L) * (xl > 0) -- bit-identical to bx_conv3x3 with that mask -- and
 *     dw / db [16,16,3,3] / [16] = bx_conv3x3_wgrad(xl, dz) up to fp32 reassociation.  Chained like bx_conv3x3_wgrad_chained: a valid
 *     *pending is summed by this launch and overwritten with dw / db's partials (pending == NULL: they are summed right away).
 *   dzo == NULL, x0 != NULL (the stage's conv2, block input without a gradient): the masked data gradient dZ_{L-1} is not stored;
 *     instead dw0 / db0 [16,Cin0,3,3] / [16] = bx_conv3x3_wgrad(x0, dZ_{L-1}) with x0 [B,H,W,8] the padded block input (Cin0 <= 8
 *     logical channels).  Both weight gradients are summed by one reduce launch that follows; *pending is invalid on return.
 *   workspace: bx_conv3x3_bwd_fused_workspace(B, H, W, x0 != NULL) bytes, not the one holding valid pending partials. */
size_t bx_conv3x3_bwd_fused_workspace(int B, int H, int W, int with_w1);
int bx_conv3x3_bwd_fused(const void* dz, const void* xl, const void* packed_flip, void* dzo, const void* x0, float* dw, float* db,
                         float* dw0, float* db0, int B, int H, int W, int Cin0, void* workspace, size_t workspace_bytes,
                         bxWgradPending* pending, bxStream stream);

/* Measurement hook: the next bx_block_conv3_tail_fwd call of this host thread records the two hipEvent_t (created by the caller,
 * timing enabled) immediately before and after its convolution kernel on the call's stream -- bench.py times the fused conv3 +
 * pool launch of the training step with it (events cannot bracket one kernel of a multi-launch call from outside).  One-shot. */
int bx_profile_next_conv3(void* ev_start, void* ev_stop);

/* ---- Block tail: pool -> BatchNorm2d -> Dropout -> + conv1x1(bilinear(x))  (M:67-76) ----------- */
typedef struct {
  int B, H, W;          /* conv3 output resolution; pooled map is [B, H/pool_h, W/pool_w] (floor) */
  int Cin_p;            /* channels of the block input x as stored (padded)            */
  int C;                /* block output channels                                        */
  int pool;             /* BX_POOL_MAX | BX_POOL_AVG                                    */
  int training;         /* 1: batch statistics + running-stat update; 0: running stats  */
  float eps, momentum;  /* 1e-5, 0.1 (nn.BatchNorm2d defaults)                          */
  float dropout_p;      /* 0 disables; mask = hash(seed[0], salt, element)              */
  uint32_t salt;
  int dtype;
  uint32_t* sync;       /* NULL, or BX_TAIL_SYNC_WORDS device words owned by THIS block instance, zero before the first call
                         * (the library leaves them zero): where bx_set_tree_max_rows allows it, the batch-statistics
                         * finalizes ride in the kernels that produce the partial sums (last workgroup to arrive).
                         * One block instance must not run on two streams at once with the same words. */
  void* route;          /* NULL, or bx_block_tail_route_bytes(d) bytes: one NIBBLE per pooled element saying which positions of its
                         * 2x2 window (bit q = row-major position q) receive its gradient -- the arg-max if positive (max pool,
                         * first maximum as ATen) or the positive ones (average pool).  That is all the backward needs of conv3's
                         * full-resolution output: bx_block_conv3_tail_fwd writes the nibbles (and may then be given y3 = NULL:
                         * the output is not stored), bx_block_tail_bwd reads them instead of y3 (which may be NULL).  1/16 of the
                         * bytes of y3 in each direction.  bf16 fused path and 2x2 windows only; ignored by bx_block_tail_fwd. */
  int pool_h, pool_w;   /* pooling window = stride (no padding, floor); 0 means 2, the reference's 2x2.  Windows other than 2x2 run
                         * the general pooling and routing kernels: bx_block_conv3_tail_fwd returns BX_EUNSUPPORTED for them,
                         * bx_block_tail_route_bytes returns 0, and bx_block_tail_bwd needs y3 (route NULL). */
} bxTailDesc;
size_t bx_block_tail_route_bytes(const bxTailDesc* d);
#define BX_TAIL_SYNC_WORDS 8192
#define BX_TAIL_SYNC_FWD 0          /* word offsets inside sync: forward statistics | backward statistics */
#define BX_TAIL_SYNC_BWD 4096
size_t bx_block_tail_workspace(const bxTailDesc* d);
/* y3: conv3 output [B,H,W,C]; x: block input [B,H,W,Cin_p]; w1x1 fp32 [C][Cin] OIHW(1x1), Cin logical;
 * bn_* fp32 [C]; num_batches_tracked int64[1]; seed uint64[1] (device, may be NULL if dropout_p==0).
 * Outputs: pooled [B,Ho,Wo,C] (pre-BN, kept for backward), out [B,Ho,Wo,C] (Ho = H/pool_h, Wo = W/pool_w),
 * save_mean/save_invstd fp32 [C] (statistics actually used). */
int bx_block_tail_fwd(const bxTailDesc* d, const void* y3, const void* x, const float* w1x1, int Cin,
                      const float* b1x1, const float* bn_weight, const float* bn_bias,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked,
                      const uint64_t* seed, void* pooled, void* out, float* save_mean, float* save_invstd,
                      void* workspace, size_t workspace_bytes, bxStream stream);
/* Policy of the in-launch finalizes (bxTailDesc.sync): a statistics pass with at most `rows` rows of partial sums is finished by
 * its last workgroup, a larger one by a separate finalize launch whose workgroups split the channels.  Default 0 = always the
 * separate launch (or the environment variable BX_TREE_MAX_ROWS at first use): measured on MI355X the in-launch form costs
 * every workgroup a drained store + ticket round trip and was 4-10 us SLOWER per pass than the ~6.5 us launch it removes
 * (DESIGN section 6).  Results do not depend on the choice beyond the rounding of double-precision sums. */
int bx_set_tree_max_rows(int rows);
/* Folded finalizes (round 3): the cross-workgroup sum of a statistics pass moves to the START of the kernel that consumes it -- every
 * workgroup of the apply kernel sums the producer's partial rows itself, in one fixed order, so no finalize launch (k_bn_finalize /
 * k_tail_bwd_mid) and no atomics are needed.  mask: bit 0 = backward passes, bit 1 = forward passes; default 3 (or the environment
 * variable BX_TAIL_FOLD at first use); a pass is folded only while rows x C stays small (the backward reduction launches
 * 8192 / C rows; the forward folds when its producer wrote at most 32768 / C rows -- the late stages).  Results do not depend
 * on the choice beyond the rounding of double-precision sums. */
int bx_set_tail_fold(int mask);
/* conv3 + tail forward in two launches (bf16 storage, MFMA-capable C, 2x2 window; otherwise BX_EUNSUPPORTED and the caller uses
 * bx_conv3x3 + bx_block_tail_fwd): y3 = relu(conv3x3(y2, w3) + b3) is stored for backward, and conv3's epilogue also
 * writes pooled = pool2x2(y3) and the batch statistics, so the pool never re-reads y3 from HBM.  w3_mfma is conv3's
 * MFMA operand from bx_conv3x3_pack (flip 0).  Same workspace size and the same
 * outputs as bx_block_tail_fwd (M:62-76). */
int bx_block_conv3_tail_fwd(const bxTailDesc* d, const void* y2, const void* w3_mfma, const float* b3, void* y3,
                            const void* x, const float* w1x1, int Cin, const float* b1x1, const float* bn_weight,
                            const float* bn_bias, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                            const uint64_t* seed, void* pooled, void* out, float* save_mean, float* save_invstd,
                            void* workspace, size_t workspace_bytes, bxStream stream);
/* Backward of the tail.  dout [B,Ho,Wo,C].  Produces
 *   dz3 [B,H,W,C]: gradient w.r.t. conv3's pre-activation (pool backward AND conv3's ReLU mask applied; zero in the rows and
 *                  columns the floor-pool drops),
 *   dx_skip [B,H,W,Cin_p] (may be NULL): gradient reaching the block input through the skip path,
 *   d_bn_weight, d_bn_bias, d_w1x1 [C][Cin], d_b1x1 (fp32, overwritten). */
int bx_block_tail_bwd(const bxTailDesc* d, const void* dout, const void* y3, const void* x, const void* pooled,
                      const float* w1x1, int Cin, const float* bn_weight, const float* save_mean,
                      const float* save_invstd, const uint64_t* seed, void* dz3, void* dx_skip,
                      float* d_bn_weight, float* d_bn_bias, float* d_w1x1, float* d_b1x1,
                      void* workspace, size_t workspace_bytes, bxStream stream);
/* y = max(x,0) elementwise (only used when a pre-ReLU conv output is an attribution target). */
int bx_relu(const void* x, void* y, size_t n, int dtype, bxStream stream);

/* ---- heads ------------------------------------------------------------------------------------ */
/* AdaptiveAvgPool2d(1) -> Linear(C,N) -> LogSoftmax (M:92-94,103-106).  feat [B,HW,C] dtype;
 * gap_out fp32 [B,C] (saved), logp fp32 [B,N].  N <= 32. */
int bx_gap_fc_lsm_fwd(const void* feat, const float* w, const float* b, float* gap_out, float* logp,
                      int B, int HW, int C, int N, int dtype, bxStream stream);
/* dlogp [B,N] -> dfeat [B,HW,C] (dtype), dW [N,C], db [N].  dfeat/dW/db may be NULL individually. */
int bx_gap_fc_lsm_bwd(const float* dlogp, const float* logp, const float* gap_out, const float* w,
                      void* dfeat, float* dw, float* db, int B, int HW, int C, int N, int dtype, bxStream stream);
/* Linear(K,N) -> LogSoftmax on fp32 features [B,K] (EEGNet dense, M:263-269,286-288). */
int bx_linear_lsm_fwd(const float* x, const float* w, const float* b, float* logp, int B, int K, int N,
                      bxStream stream);
int bx_linear_lsm_bwd(const float* dlogp, const float* logp, const float* x, const float* w, float* dx,
                      float* dw, float* db, int B, int K, int N, bxStream stream);
/* Fusion head: cat(eeg_logp, spec_logp) -> Linear(2N,Hd) -> ReLU -> Linear(Hd,N) -> LogSoftmax
 * (NB:1095-1105).  hidden fp32 [B,Hd] is saved for backward. */
int bx_fusion_head_fwd(const float* eeg_logp, const float* spec_logp, const float* w1, const float* b1,
                       const float* w2, const float* b2, float* hidden, float* logp, int B, int N, int Hd,
                       bxStream stream);
int bx_fusion_head_bwd(const float* dlogp, const float* logp, const float* hidden, const float* eeg_logp,
                       const float* spec_logp, const float* w1, const float* w2, float* d_eeg_logp,
                       float* d_spec_logp, float* dw1, float* db1, float* dw2, float* db2, int B, int N, int Hd,
                       bxStream stream);
/* Fused multimodal head: the three ops above in one launch forward / two backward, for MultimodalModel.forward
 * (NB:1095-1105 over models.py:103-106 and :286-288).  feat: block5 output [B,HW,C] channels-last `dtype`; eeg_feat fp32
 * [B,K] (EEGNet features).  Outputs of fwd (all fp32, all read again by bwd): gap_out [B,C], spec_logp / eeg_logp [B,N]
 * (the two branch outputs), hidden [B,Hd], logp [B,N].  bwd: dfeat [B,HW,C] `dtype` and d_eeg_feat [B,K] may be NULL;
 * parameter gradients are written when non-NULL.  Limits: C <= 1024, K <= 4096, N <= 32, Hd <= 256, Hd*2N <= 4096. */
size_t bx_mm_head_workspace(int B, int N, int Hd);
int bx_mm_head_fwd(const void* feat, const float* eeg_feat, const float* fc_w, const float* fc_b, const float* dense_w,
                   const float* dense_b, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* gap_out, float* spec_logp, float* eeg_logp, float* hidden, float* logp, int B, int HW, int C,
                   int K, int N, int Hd, int dtype, bxStream stream);
int bx_mm_head_bwd(const float* dlogp, const float* logp, const float* hidden, const float* spec_logp,
                   const float* eeg_logp, const float* gap, const float* eeg_feat, const float* fc_w,
                   const float* dense_w, const float* w1, const float* w2, void* dfeat, float* d_eeg_feat,
                   float* d_fc_w, float* d_fc_b, float* d_dense_w, float* d_dense_b, float* dw1, float* db1, float* dw2,
                   float* db2, void* workspace, size_t workspace_bytes, int B, int HW, int C, int K, int N, int Hd,
                   int dtype, bxStream stream);
/* The training head: bx_mm_head_fwd, bx_kldiv_fwd_bwd(logp, target, reduction, grad_scale) and bx_mm_head_bwd(dlogp) as TWO launches,
 * bit for bit what the three entries compute.  Launch 1, one workgroup per sample: the forward (all five outputs of bx_mm_head_fwd are
 * written), dlogp [B,N] = -target * grad_scale / denom (may be NULL) and the input half of the backward (dfeat / d_eeg_feat, may be
 * NULL, and the workspace).  Launch 2: the parameter gradients (written when non-NULL) and, in one more workgroup, loss[1] (may be
 * NULL).  target fp32 [B,N]; workspace as bx_mm_head_bwd; the gradients are those of the loss itself (upstream gradient 1). */
int bx_mm_head_train(const void* feat, const float* eeg_feat, const float* fc_w, const float* fc_b, const float* dense_w,
                     const float* dense_b, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* target, float* gap_out, float* spec_logp, float* eeg_logp, float* hidden, float* logp,
                     float* loss, float* dlogp, void* dfeat, float* d_eeg_feat, float* d_fc_w, float* d_fc_b,
                     float* d_dense_w, float* d_dense_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                     size_t workspace_bytes, int B, int HW, int C, int K, int N, int Hd, int reduction, float grad_scale,
                     int dtype, bxStream stream);
/* nn.KLDivLoss on log-prob input / prob target (NB:1989,1599): loss[1] and dlogp = -t/denom.
 * reduction: 0 'mean' (denom B*N), 1 'batchmean' (denom B), 2 'sum'.  grad_scale multiplies dlogp. */
int bx_kldiv_fwd_bwd(const float* logp, const float* target, float* loss, float* dlogp, int B, int N,
                     int reduction, float grad_scale, bxStream stream);

/* ---- EEGNet branch (M:239-289); activations fp32 or bf16 NCHW ------------------------------------ */
typedef struct {
  int B, Chans, T;      /* input [B,1,Chans,T] fp32                                  */
  int F1, D, F2;        /* 8, 2, 16 (the reference's defaults: register-tiled kernels; any other values: the general kernel set) */
  int K1, K2;           /* temporal kernel lengths 64 and 16 ('same': left pad (K-1)/2) */
  int P1, P2;           /* average-pool widths 4 and 8                               */
  int training;
  float eps, momentum, dropout_p;
  uint32_t salt;        /* bit 31 set: one mask entry per (sample, channel) = nn.Dropout2d (models.py:255) */
  int dtype;            /* storage of the big intermediates (conv1 output)           */
  int collapse;         /* 1: training passes with bf16 storage, K1 = 64, T >= 96, T % 8 == 0 never form the conv1 output
                         * [B,F1,Chans,T]: the electrodes are mixed first, BatchNorm1's statistics come from the input's
                         * autocorrelation, and the gradients of conv1 / bn1 / depthwiseConv from one correlation of dL/du
                         * with the input.  Such a pass has NO input gradient (dx must be NULL);
                         * forward and backward must see the same flag.  0: the layer-by-layer path. */
  float dropout_p2;     /* rate of the SECOND dropout (after pool 2); < 0: the same as dropout_p (EEGNet shares one module,
                         * models.py:255; EEGNetAttentionDeep has dropout1 / dropout2, models.py:152-164) */
  const float* const* x_slot;  /* NULL, or a DEVICE word holding the input's address (bx_store_u64x2): bx_eeg_features_fwd then reads x
                         * through it -- a captured graph is replayed on the caller's batch without a copy.  Collapsed evaluation-mode
                         * path only (collapse = 1, training = 0), where one kernel reads x and nothing is kept for a backward;
                         * the `x` argument must still be a valid pointer of the same shape (it is what an eager run reads). */
  int grad;             /* 1: bx_eeg_features_bwd will follow this forward (training = 1 implies it).  The register-tiled backward holds
                         * rows up to T = 4096 (its LDS tiles and per-thread dx registers); with a backward announced, longer rows run
                         * on the general kernel set in BOTH directions, so that a pass whose forward was accepted is computed by its
                         * backward.  0 with training = 0 (inference, Grad-CAM, attribution sweeps under no-grad): the register-tiled
                         * forward up to T = 15000, whose arena bx_eeg_saved_layout / bx_eeg_cam read.  Forward, backward, saved_bytes
                         * and workspace must see the same value. */
} bxEegDesc;
/* Parameter block: pointers to the fp32 tensors of the module, reference names in comments. */
typedef struct {
  const float* conv1_w;      /* conv1.weight        [F1,1,1,K1]      */
  const float* bn1_w; const float* bn1_b; float* bn1_rm; float* bn1_rv; int64_t* bn1_nbt;
  const float* dw_w;         /* depthwiseConv.weight [F1*D,1,Chans,1] */
  const float* bn2_w; const float* bn2_b; float* bn2_rm; float* bn2_rv; int64_t* bn2_nbt;
  const float* sep_w;        /* separableConv.weight [F2,F1*D,1,K2]  */
  const float* bn3_w; const float* bn3_b; float* bn3_rm; float* bn3_rv; int64_t* bn3_nbt;
} bxEegParams;
typedef struct {
  float* conv1_w; float* bn1_w; float* bn1_b; float* dw_w; float* bn2_w; float* bn2_b;
  float* sep_w; float* bn3_w; float* bn3_b;
} bxEegGrads;
/* Saved-for-backward arena layout is private; query its size, pass the same buffer to bwd. */
size_t bx_eeg_saved_bytes(const bxEegDesc* d);
size_t bx_eeg_workspace(const bxEegDesc* d);
/* x fp32 [B,1,Chans,T] -> feat fp32 [B, F2*(T/P1/P2)] (the Flatten() output fed to `dense`). */
int bx_eeg_features_fwd(const bxEegDesc* d, const bxEegParams* p, const float* x, const uint64_t* seed,
                        float* feat, void* saved, void* workspace, size_t workspace_bytes, bxStream stream);
/* dfeat [B, F2*T2] -> parameter gradients and (optional, may be NULL) dx fp32 [B,1,Chans,T]. */
int bx_eeg_features_bwd(const bxEegDesc* d, const bxEegParams* p, const float* x, const float* dfeat,
                        const uint64_t* seed, const void* saved, const bxEegGrads* g, float* dx,
                        void* workspace, size_t workspace_bytes, bxStream stream);
/* Byte offsets, inside the saved arena of the tuned family (F1=8, D=2, F2=16, K2=16, K1 <= 64, Chans <= 64, T <= 15000; with
 * training = 1 or grad = 1 in the descriptor T <= 4096, what the register-tiled backward holds), of the
 * depthwise output dmap fp32 [B,F1*D,T] and the separable output smap fp32 [B,F2,T/P1] (both before their BatchNorm).
 * BX_EUNSUPPORTED for any other geometry. */
int bx_eeg_saved_layout(const bxEegDesc* d, size_t* off_dmap, size_t* off_smap);

/* Grad-CAM on the EEGNet branch (canonical Grad-CAM; target = the module whose output a forward hook would see). */
enum { BX_EEG_CAM_CONV1 = 0, BX_EEG_CAM_DEPTHWISE = 1, BX_EEG_CAM_SEPARABLE = 2 };
/* 0 = unsupported (geometry outside the tuned family, maps_per_act outside [1,64], unknown target). */
size_t bx_eeg_gradcam_workspace(const bxEegDesc* d, int maps_per_act, int target);
/* saved: the arena of bx_eeg_features_fwd of the same x in evaluation mode (d->training = 0).  dfeat fp32 [B*nm, F2*T2]: the
 * gradient of each map's class score with respect to feat (nm = maps_per_act maps per sample, map = sample * nm + class).
 * Outputs (fp32; cam ReLU'd iff relu, raw the pre-ReLU map and may be NULL, weights may be NULL):
 *   BX_EEG_CAM_CONV1:     cam / raw [B*nm, Chans, T],  weights [B*nm, F1]   (reads x fp32 [B,1,Chans,T]; needs the workspace)
 *   BX_EEG_CAM_DEPTHWISE: cam / raw [B*nm, T],         weights [B*nm, F1*D]
 *   BX_EEG_CAM_SEPARABLE: cam / raw [B*nm, T/P1],      weights [B*nm, F2]
 * BX_EUNSUPPORTED (before touching any pointer) for a geometry outside the tuned family. */
int bx_eeg_gradcam(const bxEegDesc* d, const bxEegParams* p, const float* x, const void* saved, const float* dfeat,
                   int maps_per_act, int target, int relu, float* cam, float* raw, float* weights, void* workspace,
                   size_t workspace_bytes, bxStream stream);
/* The same for every class-activation method (BX_CAM_*, see "attribution" below); bx_eeg_gradcam = method BX_CAM_GRADCAM.  The
 * spatial axes are (Chans, T) for conv1, T for depthwiseConv and T/P1 for separableConv; A is the target's output (for conv1 the
 * 'same'-padded, bias-free conv1 of x, never stored), G its gradient formed per element from dfeat.  weights must be NULL for
 * BX_CAM_LAYERCAM.  The workspace of a method may be larger than Grad-CAM's: size it with bx_eeg_cam_workspace. */
size_t bx_eeg_cam_workspace(const bxEegDesc* d, int maps_per_act, int target, int method);
int bx_eeg_cam(const bxEegDesc* d, const bxEegParams* p, const float* x, const void* saved, const float* dfeat,
               int maps_per_act, int target, int method, int relu, float* cam, float* raw, float* weights, void* workspace,
               size_t workspace_bytes, bxStream stream);

/* ---- EEGNetAttentionDeep head (M:136-235, Attention M:109-134): everything after EEGNet's block 2 ----------
 * feat fp32 [B, F2*T2] (bx_eeg_features_fwd's output for the same input; the class's dropout2 is applied there)
 *   -> conv2 (1x16 'same', F2 -> F3, no bias) -> batchnorm4 -> ELU -> avg_pool3 (1x8) -> dropout3
 *   -> attention_layer over the L = T2/8 time steps (query/key/value = Linear(F3,F3), scale F3^-0.5)
 *   -> flatten (channel-major) -> dense1 (F3*L -> Hd) -> dense2 (Hd -> N) -> LogSoftmax.  All tensors fp32. */
typedef struct {
  int B, T2;            /* feat is [B, F2, T2]                                          */
  int F2, F3, K3, P3;   /* 16, 32, 16, 8                                                */
  int Hd, N;            /* dense1 width (128; power of two in [32,256]), classes (<=16) */
  int training;
  float eps, momentum, dropout_p;
  uint32_t salt;        /* bit 31 set: one mask entry per (sample, channel) = nn.Dropout2d (models.py:255) */
} bxEegDeepDesc;
typedef struct {
  const float* conv2_w;      /* conv2.weight [F3,F2,1,K3] */
  const float* bn4_w; const float* bn4_b; float* bn4_rm; float* bn4_rv; int64_t* bn4_nbt;
  const float* wq; const float* bq;   /* attention_layer.query.weight [F3,F3] / .bias */
  const float* wk; const float* bk;   /* attention_layer.key                          */
  const float* wv; const float* bv;   /* attention_layer.value                        */
  const float* w1; const float* b1;   /* dense1.weight [Hd, F3*L] (16-byte aligned) / .bias */
  const float* w2; const float* b2;   /* dense2.weight [N, Hd] / .bias                */
} bxEegDeepParams;
typedef struct {
  float* conv2_w; float* bn4_w; float* bn4_b; float* wq; float* bq; float* wk; float* bk; float* wv; float* bv;
  float* w1; float* b1; float* w2; float* b2;
} bxEegDeepGrads;
size_t bx_eeg_deep_saved_bytes(const bxEegDeepDesc* d);   /* 0 = unsupported geometry */
size_t bx_eeg_deep_workspace(const bxEegDeepDesc* d);
/* logp fp32 [B,N]; attn fp32 [B,L,L] = the softmax weights (the module's second return value), also read by bwd. */
int bx_eeg_deep_fwd(const bxEegDeepDesc* d, const bxEegDeepParams* p, const float* feat, const uint64_t* seed,
                    float* logp, float* attn, void* saved, void* workspace, size_t workspace_bytes, bxStream stream);
/* dlogp [B,N] -> dfeat [B,F2*T2] (may be NULL) and the parameter gradients (g may be NULL: inputs only). */
int bx_eeg_deep_bwd(const bxEegDeepDesc* d, const bxEegDeepParams* p, const float* feat, const float* dlogp,
                    const float* attn, const uint64_t* seed, const void* saved, const bxEegDeepGrads* g, float* dfeat,
                    void* workspace, size_t workspace_bytes, bxStream stream);

/* Stand-alone Attention module (M:109-134): x fp32 [B,L,D] -> out [B,L,D], attn [B,L,L] (softmax weights); D = 32, L <= 32.
 * qkv_saved fp32 [B,3,L,D] is written by fwd and read by bwd.  bwd: dattn (gradient w.r.t. the returned weights) and dx may
 * be NULL; parameter gradients are written when non-NULL (then workspace >= bx_attention_workspace(B) bytes). */
size_t bx_attention_workspace(int B);
int bx_attention_fwd(const float* x, const float* wq, const float* bq, const float* wk, const float* bk, const float* wv,
                     const float* bv, float* out, float* attn, float* qkv_saved, int B, int L, int D, bxStream stream);
int bx_attention_bwd(const float* dout, const float* dattn, const float* x, const float* attn, const float* qkv_saved,
                     const float* wq, const float* wk, const float* wv, float* dx, float* dwq, float* dbq, float* dwk,
                     float* dbk, float* dwv, float* dbv, void* workspace, size_t workspace_bytes, int B, int L, int D,
                     bxStream stream);

/* ---- attribution ----------------------------------------------------------------------------- */
/* Grad-CAM channel reduce (canonical; the reference has none -- SURVEY.md K18):
 *   w[m,c] = mean_p G[m,p,c];  raw[m,p] = sum_c w[m,c]*A[m/maps_per_act,p,c];  cam = relu ? max(raw,0) : raw.
 * G: [n_maps,HW,C], A: [n_maps/maps_per_act,HW,C], `dtype` channels-last (maps_per_act = classes per
 * sample sharing one activation).  cam fp32 [n_maps,HW]; weights_out fp32 [n_maps,C] may be NULL. */
int bx_gradcam_reduce(const void* A, const void* G, float* cam, float* weights_out, int n_maps, int maps_per_act,
                      int HW, int C, int relu, int dtype, bxStream stream);
/* Class-activation methods.  A[k,s]: the target's activation (channel k, position s), G = dy_c/dA, eps = 1e-6:
 *   BX_CAM_GRADCAM     w[k] = mean_s G[k,s];                                         raw[s] = sum_k w[k] A[k,s]
 *   BX_CAM_GRADCAM_PP  S[k] = sum_s A[k,s];  alpha[k,s] = G^2 / (2 G^2 + S[k] G^3 + eps), 0 where G == 0;
 *                      w[k] = sum_s max(G[k,s], 0) alpha[k,s]  (a sum, not a mean);   raw[s] = sum_k w[k] A[k,s]
 *   BX_CAM_LAYERCAM    raw[s] = sum_k max(G[k,s], 0) A[k,s]   (no channel weights: weights_out must be NULL)
 * cam = relu ? max(raw, 0) : raw; no normalisation.  Arithmetic is fp32 after the load for both storage types; fixed-order
 * sums, no atomics.  An unknown method, or Layer-CAM with non-NULL weights_out, returns BX_EINVAL. */
enum { BX_CAM_GRADCAM = 0, BX_CAM_GRADCAM_PP = 1, BX_CAM_LAYERCAM = 2 };
/* bx_gradcam_reduce for any method, same layouts and channel rule; bx_gradcam_reduce = method BX_CAM_GRADCAM. */
int bx_cam_reduce(const void* A, const void* G, float* cam, float* weights_out, int n_maps, int maps_per_act, int HW, int C,
                  int method, int relu, int dtype, bxStream stream);
/* Grad-CAM at the last stage of the multimodal model in one launch (canonical definition; the reference ships none, SURVEY fact
 * 3; heads = models.py:103-106 and XAI_Multimodality.py:1095-1105).  A: stage output NHWC [B,HW,C] (dtype); eeg_logp fp32 [B,N]
 * (EEG branch's log-probs); fc_* = Spectrogram_Model.fc, w1/b1 = fc1 [Hd,2N], w2/b2 = fc2 [N,Hd].  class_mode -2: every class
 * (nm = N maps per sample), -1: each sample's arg-max class, >= 0: that class (nm = 1).  Outputs: out_logp fp32 [B,N] (nullable),
 * cam fp32 [B*nm,HW] (ReLU'd iff relu), raw fp32 [B*nm,HW] (pre-ReLU, nullable), weights_out fp32 [B*nm,C] (nullable). */
int bx_gradcam_head(const void* A, const float* eeg_logp, const float* fc_w, const float* fc_b, const float* w1, const float* b1,
                    const float* w2, const float* b2, float* out_logp, float* cam, float* raw, float* weights_out, int B, int HW,
                    int C, int N, int Hd, int class_mode, int relu, int dtype, bxStream stream);
/* The same for sweeps over many batches: the EEG branch's own head (EEGNet.dense + LogSoftmax, models.py:287-289: eeg_feat fp32
 * [B,Fe], dense_w [N,Fe], dense_b [N]) and the bilinear up-sampling of the finished maps to H x W (W % 4 == 0) run in the same
 * launch; A is [B,h*w,C].  maps fp32 [B*nm,H,W]. */
int bx_gradcam_head_sweep(const void* A, const float* eeg_feat, const float* dense_w, const float* dense_b, int Fe, const float* fc_w,
                          const float* fc_b, const float* w1, const float* b1, const float* w2, const float* b2, float* out_logp,
                          float* maps, int B, int h, int w, int C, int N, int Hd, int H, int W, int class_mode, int relu, int dtype,
                          bxStream stream);
/* bx_gradcam_head / bx_gradcam_head_sweep for any method (the old entry points are method BX_CAM_GRADCAM).  At the last stage
 * G[k,s] = w[k] (the Grad-CAM weight) at every position and S[k] = HW gap[k], so a method only transforms the channel weights
 * before the same channel reduce:  Layer-CAM w'[k] = max(w[k], 0);  Grad-CAM++ w'[k] = w[k] > 0 ? HW w^3 / (2 w^2 + S w^3 + eps) : 0.
 * weights_out receives w' (the Grad-CAM++ w of the definition above) and must be NULL for Layer-CAM. */
int bx_cam_head(const void* A, const float* eeg_logp, const float* fc_w, const float* fc_b, const float* w1, const float* b1,
                const float* w2, const float* b2, float* out_logp, float* cam, float* raw, float* weights_out, int B, int HW,
                int C, int N, int Hd, int class_mode, int method, int relu, int dtype, bxStream stream);
int bx_cam_head_sweep(const void* A, const float* eeg_feat, const float* dense_w, const float* dense_b, int Fe, const float* fc_w,
                      const float* fc_b, const float* w1, const float* b1, const float* w2, const float* b2, float* out_logp,
                      float* maps, int B, int h, int w, int C, int N, int Hd, int H, int W, int class_mode, int method, int relu,
                      int dtype, bxStream stream);
/* Bilinear resize (align_corners=False) of fp32 maps [N,h,w] -> [N,H,W]  (F.interpolate). */
int bx_resize_bilinear(const float* src, float* dst, int N, int h, int w, int H, int W, bxStream stream);
/* Saliency reduce (NB:3121-3129): out[b,p] = scale * max_c |g[b,p,c]|, g NHWC `dtype` (first C of Cs). */
int bx_saliency_reduce(const void* g, float* out, int B, int HW, int C, int Cs, float scale, int dtype,
                       bxStream stream);
/* y = alpha*x + beta*y over fp32 (integrated-gradients accumulate, baseline interpolation). */
int bx_axpby(const float* x, float* y, size_t n, float alpha, float beta, bxStream stream);
int bx_mul(const float* a, const float* b, float* out, size_t n, bxStream stream);
/* Integrated gradients (Captum semantics): all K interpolants of a pass, out[k][i] = (1-a_k)*base[i] + a_k*x[i],
 * and the weighted accumulation acc[i] += sum_k w_k * grads[k][i] (k ascending); alphas / weights are device float[K]. */
int bx_ig_interpolate(const float* x, const float* base, const float* alphas_device, float* out, size_t n, int K, bxStream stream);
int bx_ig_accumulate(const float* grads, const float* weights_device, float* acc, size_t n, int K, bxStream stream);
/* out = |x| over fp32 (EEG saliency, NB:3121-3122). */
int bx_abs(const float* x, float* out, size_t n, bxStream stream);
/* out = x * scalar[0] with the scalar on the device (loss.backward()'s upstream gradient; no host sync). */
int bx_scale_dev(const float* x, const float* scalar, float* out, size_t n, bxStream stream);

/* ---- EEG stacker (DS:73-104,125-131): select/clip/nan->0,/32 -> Butterworth IIR -> decimate ---- */
/* raw fp32 [B,L,Craw]; channel_index int32[C] (device) selects columns; b,a = host double[order+1];
 * out fp32 [B,1,C,L/step].  fp64 state per (sample, channel) row. */
int bx_eeg_stack_iir(const float* raw, const int* channel_index, float* out, int B, int L, int Craw, int C,
                     const double* b_host, const double* a_host, int order, int step, float clip, float scale,
                     bxStream stream);

/* ---- native-pipeline EEG montage stacker (CombinedDataset.process_eeg, NB:1148-1164,1211-1276) ---- */
/* raw fp32 [B,L,Craw] (eeg.values of each frame); output row r is built from raw column row_a[r], minus column row_b[r]
 * when row_b[r] >= 0 (device int32[R] each, values < Craw).  Per raw column: lfilter(b1,a1) in fp64, NaN -> the row's
 * nanmean; per output row: (difference,) lfilter(b2,a2), mean of 4 consecutive samples at every 4th column of [0,L-1),
 * z-score with population std and eps, zero-padded / truncated to out_len.  out fp32 [B,R,out_len].
 * b*, a* = host double[order+1] (transfer-function coefficients, order <= 12).  L % 4 must be 0 or 1.
 * status: device int32[1], set to 1 when some raw row is NaN from its first sample (the reference drops such rows and
 * then mis-indexes; here the row is treated as all-zero after the first filter and the caller is told).
 * The mirror augmentation (cfg.AUGMENT) is a column permutation the caller applies through row_a/row_b. */
size_t bx_eeg_montage_workspace(int B, int L, int Craw, int R);
int bx_eeg_montage_stack(const float* raw, const int* row_a, const int* row_b, float* out, int B, int L, int Craw, int R,
                         int out_len, const double* b1, const double* a1, int order1, const double* b2, const double* a2,
                         int order2, float eps, int* status, void* workspace, size_t workspace_bytes, bxStream stream);

/* ---- native-pipeline spectrogram pre-processing (CombinedDataset.process_spectrogram, NB:1166-1204) ---- */
/* raw fp32 [B,Trows,Ccols] (the parquet frame's values without the time column, NaNs allowed); offsets: device int32[B]
 * (spectrogram_label_offset_seconds; the reference windows `sel` COLUMNS from offset//2) or NULL; out fp32 [B,3,R,W].
 * Chain: transpose -> pad/truncate to R x W -> NaN -> row nanmean -> subtract column means -> filtfilt(notch_b, notch_a)
 * along the rows (odd extension, 9 samples; notch_zi = scipy.signal.lfilter_zi) -> separable gaussian (gauss_w: 9 symmetric
 * weights, 'reflect' boundary) -> min-max with eps -> 3 identical channels.  The reference's final skimage resize is to
 * the array's own shape (identity).  status: device int32[1]; bit 0 = some row was entirely NaN (the reference drops it
 * and then really resamples: not reproduced), bit 1 = NaN after filtering. */
size_t bx_spec_preprocess_workspace(int B, int R, int W);
int bx_spec_preprocess(const float* raw, const int* offsets, float* out, int B, int Trows, int Ccols, int R, int W, int sel,
                       const double* notch_b, const double* notch_a, const double* notch_zi, const double* gauss_w,
                       float eps, int* status, void* workspace, size_t workspace_bytes, bxStream stream);

/* ---- benchmark-variant spectrogram stacker (spectrogram half): four region planes per sample ----------- */
/* raw fp32 [B,Trows,C] parquet values (C = regions x bins, NaNs allowed); offsets device int32[B] or NULL (window of `win` time
 * rows from offset // 2, zero padded; XAI_Multimodality.py:1178-1183); out fp32 [B,regions,Ho,Wo].  Chain: transpose ->
 * normalize_signal (root/src/utils/data_utils.py:133-136: NaN -> nanmean of the sample, min-max with eps) -> per region
 * resample_spectrogram (data_utils.py:145-147: skimage.transform.resize(mode='reflect', anti_aliasing=True): gaussian_filter
 * with the host-supplied 1-D weights gauss_y[2*radius_y+1] / gauss_x[2*radius_x+1] ('mirror' boundary; radius 0 = no filter),
 * then order-1 zoom with grid_mode coordinates, mirrored indices).  fp64 arithmetic.
 * A window without one finite value (every sample NaN, no zero padding): the reference's nanmean of an empty set is NaN and its
 * output NaN everywhere; here the fill value is 0, as the reference's handle_nan takes it for an all-NaN row, so the plane is
 * constant and the output 0.  A window wholly outside the recording is all padding: output 0 as well. */
size_t bx_spec_regions_workspace(int B);
int bx_spec_regions(const float* raw, const int* offsets, float* out, int B, int Trows, int C, int regions, int win, int Ho, int Wo,
                    const double* gauss_y, int radius_y, const double* gauss_x, int radius_x, float eps, void* workspace,
                    size_t workspace_bytes, bxStream stream);

/* ---- optimiser over the flat parameter arena (torch.optim.AdamW, NB:1988) ------------------------ */
/* p, g, m, v fp32 [n]; step_count device float[1]: incremented by this call, then used as t. */
int bx_adamw_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, float* step_count, bxStream stream);
/* The same step with the hyper-parameters in DEVICE memory, hyper fp32[8] = {lr, beta1, beta2, eps, weight_decay, grad_scale,
 * l2_lambda, unused} (a captured hipGraph follows a learning-rate schedule without re-capture), and with the DDP loop's manual
 * L2 penalty fused in (root/src/training/training_distributed.py:52-57: total_loss = loss + l2_lambda * sum p^2): 2*l2_lambda*p
 * is added to the scaled gradient before the moment updates; when sumsq_partials (fp32[bx_adamw_partials(n)]) and l2_value
 * (fp32[1]) are given, l2_value[0] = l2_lambda * sum p^2 over the parameters BEFORE this update (fixed-order sum).
 * step_count here is a device buffer of bx_adamw_step_words(n) 32-bit words: [0] the step count (float, incremented by this
 * call in the update launch itself and then used as t), the rest ticket counters the launch uses to find its last workgroup --
 * zero on entry, zero again on completion; concurrent launches must not share the buffer. */
size_t bx_adamw_partials(size_t n);
size_t bx_adamw_step_words(size_t n);
int bx_adamw_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, float* step_count,
                      float* sumsq_partials, float* l2_value, bxStream stream);
/* dst_device[0..7] = values_host[0..7], ordered on `stream`.  The eight values travel as kernel arguments (copied when the call
 * returns), so the host buffer needs no lifetime beyond the call -- how FlatAdamW refreshes `hyper` when a torch LR scheduler
 * changed param_groups (DDP:98-101), also between replays of a captured step. */
int bx_store_f32x8(float* dst_device, const float* values_host, bxStream stream);
/* dst_device[0] = a, dst_device[1] = b (64-bit words, e.g. device addresses for bxEegDesc.x_slot / bx_conv3x3_pack_layout_ex's src_slot);
 * the values travel as kernel arguments, the store is ordered on `stream`. */
int bx_store_u64x2(uint64_t* dst_device, uint64_t a, uint64_t b, bxStream stream);
/* sum of squares of a flat fp32 arena -> out[1] (DDP loop's manual L2 term, DDP:52-53). */
int bx_sumsq(const float* x, size_t n, float* out, bxStream stream);
/* LIME's batched inference (XAI_Multimodality.py:1567-1574): uint8 images [N,H,W,C] -> scale * value in the internal
 * channels-last layout [N,H,W,Cp] (dtype; channels C..Cp-1 zero) = torchvision ToTensor with scale 1/255; row-wise softmax. */
int bx_u8_to_nhwc(const unsigned char* src, void* dst, int N, int H, int W, int C, int Cp, float scale, int dtype, bxStream stream);
int bx_softmax_rows(const float* x, float* y, int rows, int N, bxStream stream);
/* ---- LIME for images (lime 0.2.0.1 LimeImageExplainer.explain_instance, XAI_Multimodality.py:1658-1670): everything after the
 * segmentation.  Limits of all four entry points: 1 <= S <= 1024 segments (labels 0..S-1), 1 <= C <= 4 image channels (Cp = 8),
 * K <= 32 classes, N >= 2 samples; refused with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* Fudged colours (hide_color=None): colours u8 [B,S,C] = per (segment, channel) mean of img u8 [B,H,W,C] over segments i32 [B,H,W],
 * exact 64-bit integer sum and count, double(sum) / count truncated -- bit for bit numpy's mean + astype(uint8).  A label without
 * pixels gets 0 (the Python layer refuses such label maps). */
int bx_lime_segment_mean(const unsigned char* img, const int* segments, unsigned char* colours, int B, int H, int W, int C, int S,
                         bxStream stream);
/* Rows n0 .. n0+n-1 of every image's neighbourhood, x [B*n, H, W, Cp] (dtype; image-major): pixel p of sample j is the image where
 * Z u8 [B,N,S] has Z[b, n0+j, segments[p]] != 0 and colours[b, segments[p]] elsewhere, as (float)u8 * (float)(1/255) -- what
 * bx_u8_to_nhwc gives for the perturbed uint8 image, which is never built; channels C..Cp-1 zero. */
int bx_lime_perturb(const unsigned char* img, const int* segments, const unsigned char* colours, const unsigned char* Z, void* x,
                    int B, int H, int W, int C, int Cp, int S, int N, int n0, int n, int dtype, bxStream stream);
/* Weighted ridge surrogate per image and label, fp64, fixed summation order (identical bits run to run).  Z u8 [B,N,S] masks,
 * P fp32 [B,N,K] class probabilities, labels i32 [B,nl] classes to explain, used i32 [B,S_used] feature subset (NULL: all,
 * S_used = S).  weights[b,n] = sqrt(exp(-d^2 / kernel_width^2)), d = 1 - sqrt(sum_s Z[b,n,s] / S) (cosine distance to the all-ones
 * row 0); then sklearn's Ridge(alpha, fit_intercept=True).fit(Z[:, used], P[:, label], sample_weight=weights): coef fp64
 * [B,nl,S_used] (in the order of `used`), intercept, score (weighted R^2) and local_pred (prediction for row 0) fp64 [B,nl].
 * workspace: bx_lime_fit_workspace bytes (0 for refused shapes), 8-byte aligned. */
size_t bx_lime_fit_workspace(int B, int N, int S, int S_used, int K, int nl);
int bx_lime_fit(const unsigned char* Z, const float* P, const int* labels, const int* used, int B, int N, int S, int S_used, int K, int nl,
                double alpha, double kernel_width, void* workspace, size_t workspace_bytes, double* coef, double* intercept, double* score,
                double* local_pred, double* weights, bxStream stream);
/* Per-pixel heat map fp32 [B,nl,H,W]: map[b,l,p] = (float)coef[b,l,j] where used[b,j] == segments[b,p], 0 for unused features. */
int bx_lime_weight_map(const double* coef, const int* used, const int* segments, float* map, int B, int nl, int H, int W, int S,
                       int S_used, bxStream stream);
/* ---- Deletion / insertion curves (the causal metric of RISE, Petsiuk et al., BMVC 2018; the reference ships no faithfulness
 * metric): score an attribution map by removing (deletion) or restoring (insertion) the input's cells in order of decreasing
 * attribution, a fixed number `per` per step, and following the explained class.  A map has N cells per sample, 1 <= N < 2^20
 * (refused with BX_EUNSUPPORTED above that, before any pointer is touched). */
/* ranks i32 [B,N]: position of cell i in a stable descending sort of values fp32 [B,N] over the flat index, ties by ascending
 * index: rank[b,i] = #{j : key[b,j] > key[b,i]} + #{j < i : key[b,j] == key[b,i]}, key = value with NaN counted as -inf and
 * -0.0 equal to +0.0.  Exact and deterministic (per-row radix sort; no result depends on the order of an atomic).  Every row of
 * ranks is a permutation of 0..N-1.  workspace: bx_rank_desc_workspace bytes (0 for refused shapes), 4-byte aligned. */
size_t bx_rank_desc_workspace(int B, int N);
int bx_rank_desc(const float* values, int* ranks, int B, int N, void* workspace, size_t workspace_bytes, bxStream stream);
/* Perturbed spectrogram rows.  x fp32 NCHW [B,C,H,W], ranks i32 [B,H*W] (a cell is a pixel with all its channels) ->
 * out [B*n, H, W, Cp] (dtype; sample-major: row b*n + j carries curve point i0 + j), channels C..Cp-1 zero, 1 <= C <= 4 (Cp = 8).
 * With the cut k = min(H*W, (i0 + j) * per): deletion (insertion = 0) takes cells of rank < k from the baseline and the others from
 * x, insertion the other way round.  Bit for bit bx_nchw_to_nhwc of that selection, which is never built.
 * baseline fp32, by baseline_kind: 0 one value, 1 one value per channel [C], 2 a tensor of x's shape.
 * Any number of points may sit at the clamped cut k = H*W (steps = 5 on 7 cells: per = 2, cuts 0 2 4 6 7 7); only the point index is
 * bounded, i0 >= 0, n >= 1, i0 + n - 1 <= H*W.  One call's output stays below 2^32 bytes. */
int bx_faith_perturb_spec(const float* x, const int* ranks, const float* baseline, int baseline_kind, void* out, int B, int C, int H,
                          int W, int Cp, int per, int i0, int n, int insertion, int dtype, bxStream stream);
/* Perturbed EEG rows.  x fp32 [B,1,Chans,T] -> out fp32 [B*n,1,Chans,T], same row order, cut and selection.  map_rows = Chans:
 * ranks i32 [B,Chans*T], a cell is one electrode at one time step; map_rows = 1: ranks i32 [B,T], a cell is a time column across
 * electrodes.  baseline_kind: 0 one value, 1 one value per electrode [Chans], 2 a tensor of x's shape. */
int bx_faith_perturb_eeg(const float* x, const int* ranks, int map_rows, const float* baseline, int baseline_kind, float* out, int B,
                         int Chans, int T, int per, int i0, int n, int insertion, bxStream stream);
/* logp fp32 [B,P,K] (log-probabilities of the P = steps + 1 curve points), classes i32 [B] -> curve fp32 [B,P] =
 * exp(logp[b,i,classes[b]]) (use_logprob: the log-probability itself) and auc fp64 [B] = (sum_i curve - curve[0]/2 - curve[P-1]/2)
 * / (P - 1), RISE's trapezoid rule on the unit interval; the sum runs in fp64 over the stored fp32 points in index order, one
 * thread per sample, so its bits do not depend on scheduling. */
int bx_faith_curve(const float* logp, const int* classes, float* curve, double* auc, int B, int P, int K, int use_logprob, bxStream stream);
/* ---- RISE saliency (Petsiuk et al., BMVC 2018; the reference ships no black-box attribution of the EEG input): the map of an input
 * is the average of N random smooth masks, each weighted by the class probability the model gives the input seen through it.
 * Mask domain [Hm,Wm]: [H,W] of a spectrogram (one value for all channels of a pixel, 1 <= C <= 4), [Chans,T] of an EEG input or
 * [1,T] (a time column across electrodes); Hm * Wm < 2^20.  Grid gh x gw with 1 <= gh <= min(32, Hm), 1 <= gw <= min(32, Wm); cell
 * size ch = ceil(Hm / gh), cw = ceil(Wm / gw).  bits u8 [N,gh,gw] (non-zero = 1), shifts i32 [N,2] = (dy, dx) with 0 <= dy < ch,
 * 0 <= dx < cw (values outside are clamped into the range); N < 2^24.
 * Mask n is the crop [dy:dy+Hm, dx:dx+Wm] of the bilinear, align_corners=False up-sampling of bits[n] (as 0.0 / 1.0) from gh x gw to
 * (gh+1) ch x (gw+1) cw.  Per axis, in fp32 and without fused multiply-adds, for the up-sampled coordinate u = y + dy (x + dx):
 *     s = max(0, (u + 0.5) * (g / ((g + 1) c)) - 0.5),  i0 = min(int(s), g - 1),  i1 = min(i0 + 1, g - 1),  l = s - i0,
 *     m = (1 - ly) * ((1 - lx) * b[y0][x0] + lx * b[y0][x1]) + ly * ((1 - lx) * b[y1][x0] + lx * b[y1][x1])
 * (horizontal blend first, then vertical; the convention of bx_resize_bilinear).  Every m lies in [0, 1]; all-ones bits give exactly
 * 1.0 and all-zero bits exactly 0.0.  No entry point but bx_rise_masks ever stores a mask: each recomputes m where it needs it from
 * the bit rows staged in LDS.  Limits are refused with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* out fp32 [n,Hm,Wm]: masks n0 .. n0+n-1 (for tests, plots and callers who want them; n * Hm * Wm < 2^31). */
int bx_rise_masks(const unsigned char* bits, const int* shifts, float* out, int N, int gh, int gw, int Hm, int Wm, int n0, int n,
                  bxStream stream);
/* Perturbed spectrogram rows.  x fp32 NCHW [B,C,H,W] -> out [B*n, H, W, Cp] (dtype; sample-major: row b*n + j is sample b seen
 * through mask n0 + j), channels C..Cp-1 zero, Cp = 8: base + m * (x - base) evaluated in fp32 as written (three roundings), then
 * stored as dtype -- bit for bit bx_nchw_to_nhwc of that tensor, which is never built.  baseline fp32, by baseline_kind as in
 * bx_faith_perturb_spec: 0 one value, 1 one value per channel [C], 2 a tensor of x's shape.  One call's output stays below 2^32 bytes. */
int bx_rise_perturb_spec(const float* x, const unsigned char* bits, const int* shifts, const float* baseline, int baseline_kind, void* out,
                         int B, int C, int H, int W, int Cp, int N, int gh, int gw, int n0, int n, int dtype, bxStream stream);
/* Perturbed EEG rows.  x fp32 [B,1,Chans,T] -> out fp32 [B*n,1,Chans,T], same row order and arithmetic.  map_rows = Chans: the mask
 * domain is [Chans,T]; map_rows = 1: it is [1,T] and a column's value is applied to every electrode.  baseline_kind: 0 one value,
 * 1 one value per electrode [Chans], 2 a tensor of x's shape. */
int bx_rise_perturb_eeg(const float* x, const unsigned char* bits, const int* shifts, int map_rows, const float* baseline, int baseline_kind,
                        float* out, int B, int Chans, int T, int N, int gh, int gw, int n0, int n, bxStream stream);
/* The map.  P fp32 [B,N,K] class probabilities of sample b seen through mask n (K <= 32); classes i32 [B] (one map per sample, of
 * that class) or NULL (a map for each of the K classes).  sal fp32 [B,Hm*Wm] or [B,K,Hm*Wm]:
 *     sal[b,k,p] = (sum_n P[b,n,k] m_n(p)) / D(p),   D = N p1 (normalize = 0, the paper's expected coverage) or
 *     D(p) = sum_n m_n(p) (normalize = 1, the coverage the masks really gave the cell; a cell no mask reached gets 0),
 * coverage fp32 [Hm*Wm] = sum_n m_n(p).  Both sums run in fp64 over n = 0..N-1 in index order in one thread's registers, every
 * term the exact product (double)P * (double)m; the quotient is taken in fp64 and rounded to fp32 once.  No atomics: the result's
 * bits are a function of the inputs alone. */
int bx_rise_accumulate(const float* P, const int* classes, const unsigned char* bits, const int* shifts, float* sal, float* coverage, int B,
                       int N, int K, int gh, int gw, int Hm, int Wm, double p1, int normalize, bxStream stream);
/* ---- Score-CAM (Wang et al., CVPR-W 2020; the reference ships no class-activation method): a class-activation map at a layer whose
 * channel weights come from forward passes of the input seen through each up-sampled activation channel; no gradient.
 * One activation is addressed by a base pointer, a dtype (BX_F32 / BX_BF16; bf16 is widened to fp32 first, which is exact) and four
 * non-negative element strides: element (b, k, y, x) of A [B, C, h, w] lives at A[b sb + k sc + y sy + x sx], every offset below 2^31.
 * The spectrogram branch's NHWC activation [B,h,w,C] is (h w C, 1, w C, C); the EEG branch's saved maps [B,C,T'] are (C T', T', 0, 1)
 * with h = 1.  The mask domain is [Hm,Wm]: [H,W] of the spectrogram, [1,T] of the EEG input; Hm Wm < 2^20 and h w < 2^20.
 * For one sample, with x the input, c the class and base the baseline:
 *   1. U_k = bilinear up-sampling of plane k to Hm x Wm, align_corners=False, per axis in fp32 and without fused multiply-adds
 *          s = max(scale (o + 0.5) - 0.5, 0), scale = (float)in / (float)out,  i0 = min((int)s, in - 1),  i1 = min(i0 + 1, in - 1),
 *          l = s - i0;   top = (1 - lx) a00 + lx a01,  bot = (1 - lx) a10 + lx a11,  U = (1 - ly) top + ly bot
 *      (horizontal blend first, then vertical: the convention of bx_resize_bilinear).
 *   2. lo_k = min U_k, hi_k = max U_k over the UP-SAMPLED plane (with align_corners=False the interior extremes of A are not
 *      attained); a zero extreme is +0.0.  Channel k is valid iff hi_k > lo_k; scale_k = 1 / (hi_k - lo_k) in fp32 if valid, else 0.
 *   3. M_k(p) = min((U_k(p) - lo_k) scale_k, 1), in [0, 1];  row k is x_k = base + M_k (x - base), three roundings, one mask value for
 *      all channels of a spectrogram pixel / all electrodes of an EEG time column.  An invalid channel's row is the baseline.
 *   4. P[k, j] = softmax probability of class j for x_k (the model's own kernels and bx_softmax_rows).
 *      BX_SCORECAM_PROB: w_k = P[k, c] (the authors' published code);  BX_SCORECAM_INCREASE: w_k = P[k, c] - P_base[c] in fp32, P_base
 *      the probabilities of the all-baseline input (the paper's increase of confidence);  w_k = 0 for an invalid channel.
 *   5. raw[s] = sum_k w_k A[k, s] at the activation's own resolution, in fp64 over k = 0..C-1 in index order, every term the exact
 *      product, one rounding to fp32;  cam = max(raw, 0) if relu.  No normalisation (the conventions of bx_cam_reduce; the authors'
 *      script sums up-sampled planes and min-max normalises the result).
 * No mask is ever stored: every kernel recomputes U where it needs it.  Every entry point writes every element of its outputs and
 * refuses its limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
#define BX_SCORECAM_PROB 0
#define BX_SCORECAM_INCREASE 1
/* lo, hi, scale fp32 [B,C] of step 2.  Two levels, no atomics: (plane, chunk of 4096 up-sampled values) -> one pair, then one fold per
 * plane.  workspace: bx_scorecam_range_workspace bytes (0 for refused shapes), 4-byte aligned. */
size_t bx_scorecam_range_workspace(int B, int C, int Hm, int Wm);
int bx_scorecam_range(const void* A, int dtype, int sb, int sc, int sy, int sx, int B, int C, int h, int w, int Hm, int Wm, float* lo,
                      float* hi, float* scale, void* workspace, size_t workspace_bytes, bxStream stream);
/* Perturbed spectrogram rows.  x fp32 NCHW [B,Cin,H,W], 1 <= Cin <= 4 -> out [nb*n, H, W, Cp] (dtype; row bl*n + j is sample b0 + bl
 * seen through channel k0 + j), channels Cin..Cp-1 zero, Cp = 8 -- bit for bit bx_nchw_to_nhwc of step 3's tensor, which is never
 * built.  lo, scale fp32 [B,C] are ARGUMENTS (bx_scorecam_range's, or a reference's: the rows then do not depend on how the device
 * rounds a division).  baseline fp32, by baseline_kind as in bx_rise_perturb_spec: 0 one value, 1 one value per channel [Cin], 2 a
 * tensor of x's shape.  A, lo, scale, x and a kind-2 baseline are indexed by the sample b0 + bl.  One call's output stays below 2^32 bytes. */
int bx_scorecam_perturb_spec(const float* x, const void* A, int dtype_a, int sb, int sc, int sy, int sx, int C, int h, int w, const float* lo,
                             const float* scale, const float* baseline, int baseline_kind, void* out, int B, int Cin, int H, int W, int Cp,
                             int b0, int nb, int k0, int n, int dtype, bxStream stream);
/* Perturbed EEG rows.  x fp32 [B,1,Chans,T] -> out fp32 [nb*n,1,Chans,T], same row order and arithmetic; the planes have h = 1 (w
 * values, strides sb, sc, sx) and column t's mask value applies to every electrode.  baseline_kind: 0 one value, 1 one value per
 * electrode [Chans], 2 a tensor of x's shape. */
int bx_scorecam_perturb_eeg(const float* x, const void* A, int dtype_a, int sb, int sc, int sx, int C, int w, const float* lo,
                            const float* scale, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int b0,
                            int nb, int k0, int n, bxStream stream);
/* Steps 4-5.  P fp32 [B,C,K] (K <= 32), P_base fp32 [B,K] (NULL for BX_SCORECAM_PROB), valid u8 [B,C] (non-zero = valid), classes
 * i32 [B] (one map per sample, nm = 1) or NULL (a map for each class, nm = K).  raw and / or cam fp32 [B*nm, h*w] (either may be NULL,
 * not both; map index = sample * nm + class), weights fp32 [B*nm, C] = w_k. */
int bx_scorecam_combine(const float* P, const float* P_base, const int* classes, const unsigned char* valid, const void* A, int dtype_a, int sb,
                        int sc, int sy, int sx, int B, int C, int h, int w, int K, int weight_mode, int relu, float* raw, float* cam,
                        float* weights, bxStream stream);
/* ---- Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; Captum's Occlusion; the reference ships no black-box attribution): slide a
 * window over the input, replace it by the baseline and record how much the class score drops.  Deterministic: no seed, no sampling.
 * Domain [Hm,Wm]: [H,W] of a spectrogram [B,C,H,W] (a cell is a pixel with all its channels, 1 <= C <= 4) or [Chans,T] of an EEG
 * input [B,1,Chans,T]; Hm * Wm < 2^20.  Window (wh, ww) and stride (sh, sw) with 1 <= sh <= wh <= Hm and 1 <= sw <= ww <= Wm
 * (stride <= window is Captum's rule: every cell is covered).
 * Window positions: ny = 1 + ceil((Hm - wh) / sh), nx = 1 + ceil((Wm - ww) / sw), N = ny * nx windows, window j = iy * nx + ix covers
 * rows [iy sh, min(iy sh + wh, Hm)) and columns [ix sw, min(ix sw + ww, Wm)): the last window of an axis is clipped at the border (what
 * Captum's padded mask does), and (ny - 1) sh + wh >= Hm, so it always reaches the border.
 * Row j of sample b is x[b] with the cells of window j taken from the baseline and every other element x itself: a selection, not a
 * blend -- every output element is bit for bit an element of x or of the baseline, -0.0 survives.  baseline fp32, by baseline_kind as in
 * bx_faith_perturb_*: 0 one value, 1 one value per channel [C] (spectrogram) / electrode [Chans] (EEG), 2 a tensor of x's shape.
 * With S[b,j,k] the score (softmax probability or log-probability) of class k for row j and S0[b,k] the score of the unperturbed input,
 *     attr[b,k,p] = (1 / cnt(p)) * sum over the windows j covering p, in ascending j, of (S0[b,k] - S[b,j,k]),
 * cnt(p) = cy(y) * cx(x) >= 1 the number of windows covering p: iy from max(0, ceil((y - wh + 1) / sh)) to min(ny - 1, floor(y / sh)),
 * likewise for x.  Each difference, the sum and the quotient are fp64; the result is rounded to fp32 once.  No atomics: the result's
 * bits are a function of the inputs alone.  Every entry point writes every element of its outputs and refuses its limits with
 * BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* Perturbed spectrogram rows.  x fp32 NCHW [B,C,H,W] -> out [B*n, H, W, Cp] (dtype; sample-major: row b*n + j is sample b with window
 * n0 + j occluded), channels C..Cp-1 zero, Cp = 8 -- bit for bit bx_nchw_to_nhwc of the selection, which is never built.
 * 0 <= n0, 1 <= n, n0 + n <= N.  One call's output stays below 2^32 bytes. */
int bx_occlusion_perturb_spec(const float* x, const float* baseline, int baseline_kind, void* out, int B, int C, int H, int W, int Cp, int wh,
                              int ww, int sh, int sw, int n0, int n, int dtype, bxStream stream);
/* Perturbed EEG rows.  x fp32 [B,1,Chans,T] -> out fp32 [B*n,1,Chans,T], same row order and selection over the domain [Chans,T]. */
int bx_occlusion_perturb_eeg(const float* x, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int wh, int ww,
                             int sh, int sw, int n0, int n, bxStream stream);
/* The map.  S fp32 [B,N,K], S0 fp32 [B,K], K <= 32; classes i32 [B] (one map per sample, of that class) or NULL (a map for each of the
 * K classes).  attr fp32 [B,Hm*Wm] or [B,K,Hm*Wm] as defined above, counts i32 [Hm*Wm] = cnt(p).  Refused when ny * nx != N;
 * B * N * K and B * K * Hm * Wm stay below 2^31. */
int bx_occlusion_accumulate(const float* S, const float* S0, const int* classes, float* attr, int* counts, int B, int N, int K, int Hm, int Wm,
                            int wh, int ww, int sh, int sw, bxStream stream);
/* ---- Kernel SHAP (Lundberg & Lee, NeurIPS 2017; the reference explains its EEG branch with shap.GradientExplainer and reduces the
 * values to per-electrode importances): Shapley values of M players from forward passes alone, so either input of the multimodal
 * model can be explained; the values of a sample add up to score(input) - score(baseline).
 * Players and coalitions.  The players are the M labels 0..M-1 (2 <= M <= 256, all present) of an int32 label map seg over the
 * input's map domain: [H,W] of a spectrogram [B,C,H,W] (a cell is a pixel with all its channels, 1 <= C <= 4), [Chans,T] or [1,T] (a
 * time column, every electrode) of an EEG input [B,1,Chans,T]; Hm * Wm < 2^20.  One label map serves the whole batch.  A coalition
 * z in {0,1}^M shows the input on the cells whose label is in z and the baseline elsewhere: a selection, not a blend -- every element
 * of a row is bit for bit an element of x or of the baseline, -0.0 survives.  baseline fp32, by baseline_kind as in
 * bx_faith_perturb_*: 0 one value, 1 one value per channel [C] (spectrogram) / electrode [Chans] (EEG), 2 a tensor of x's shape.
 * v_b,k(z) is the score (softmax probability or log-probability) of class k for sample b under coalition z; v(1) is the score of the
 * unperturbed input (clean), v(0) that of the baseline (empty).
 * Values.  phi[b,k,.] minimises sum_n w_n (v(z_n) - phi0 - sum_i phi_i z_ni)^2 subject to phi0 = v(0) and sum_i phi_i = v(1) - v(0).
 * The constraint is eliminated on the last player: Xt[n,i] = z_ni - z_n,M-1 for i < M-1 (-1, 0 or 1),
 * yt_n = v(z_n) - v(0) - z_n,M-1 D with D = v(1) - v(0); (Xt' W Xt) phi' = Xt' W yt is solved by Cholesky in fp64; phi_M-1 = D - sum phi'.
 * Coalition set (built by the caller; the same for every sample).  Exact, when 2^M - 2 <= num_samples: every proper non-empty
 * coalition in increasing order of the integer whose bit i is player i, w = (M-1) / (C(M,s) s (M-s)), s = |z| -- the exact Shapley
 * values.  Sampled, otherwise: N = num_samples rounded down to even, rng = numpy.random.default_rng(seed),
 * sizes = rng.choice(arange(1, M), size=N/2, p ~ (M-1) / (s (M-s))), row 2j = the players rng.permutation(M)[:sizes[j]], row 2j+1 its
 * complement (paired sampling, Covert & Lee 2021), all weights 1.  Given: any Z [N,M] without an all-zero or all-one row (the
 * constraint already holds those two) and weights [N] > 0.
 * Every entry point refuses its limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* Perturbed spectrogram rows.  x fp32 NCHW [B,C,H,W], segments i32 [H*W], Z u8 [N,M] (non-zero = the player is shown) -> out
 * [B*n, H, W, Cp] (dtype; sample-major: row b*n + j is sample b under coalition n0 + j), channels C..Cp-1 zero, Cp = 8 -- bit for bit
 * bx_nchw_to_nhwc of the selection, which is never built.  0 <= n0, 1 <= n, n0 + n <= N.  A label outside 0..M-1 counts as player 0.
 * Every element of out is written; one call's output stays below 2^32 bytes. */
int bx_shap_perturb_spec(const float* x, const float* baseline, int baseline_kind, void* out, int B, int C, int H, int W, int Cp,
                         const int* segments, const unsigned char* Z, int M, int N, int n0, int n, int dtype, bxStream stream);
/* Perturbed EEG rows.  x fp32 [B,1,Chans,T] -> out fp32 [B*n,1,Chans,T], same row order; segments i32 [map_rows*T] with
 * map_rows = Chans (element (ch,t) belongs to cell (ch,t)) or 1 (to cell (0,t)). */
int bx_shap_perturb_eeg(const float* x, const float* baseline, int baseline_kind, float* out, int B, int Chans, int T, int map_rows,
                        const int* segments, const unsigned char* Z, int M, int N, int n0, int n, bxStream stream);
/* The fit.  S fp32 [B,N,K] (the scores of the N coalitions), clean and empty fp32 [B,K], K <= 32; classes i32 [B] (R = 1: the values
 * of that class) or NULL (R = K: of every class); Z u8 [N,M], weights fp64 [N].  phi fp64 [B,R,M] as defined above; info i32 [1].
 * The Gram matrix is computed once per call, for B * R right-hand sides; every sum is taken by one thread in index order (the last
 * player's with Neumaier's compensation): no atomics, the result's bits are a function of the inputs alone.  A Cholesky pivot that is
 * not above (M-1) 2^-52 times its diagonal entry of the Gram matrix -- non-positive up to the rounding of the eliminations, which is
 * what an exactly singular matrix leaves -- writes its index + 1 to info and leaves phi untouched: the coalitions do not determine
 * the values.  Otherwise info = 0.  2 <= M <= 256, N >= M - 1, B * N * K < 2^31.  The workspace (8-byte aligned) holds the matrix and
 * the right-hand sides; bx_shap_fit_workspace returns its size in bytes (all_classes: classes is NULL), 0 for refused arguments. */
size_t bx_shap_fit_workspace(int B, int N, int K, int M, int all_classes);
int bx_shap_fit(const float* S, const float* clean, const float* empty, const int* classes, const unsigned char* Z, const double* weights,
                int B, int N, int K, int M, void* workspace, size_t workspace_bytes, double* phi, int* info, bxStream stream);
/* The map.  map[b,r,p] = (float) phi[b,r,segments[p]] (0 for a label outside 0..M-1); phi fp64 [B,R,M], map fp32 [B,R,Hm*Wm], R <= 32,
 * B * R * Hm * Wm < 2^31. */
int bx_shap_value_map(const double* phi, const int* segments, float* map, int B, int R, int Hm, int Wm, int M, bxStream stream);
/* ---- Expected gradients (SHAP's GradientExplainer, the one attribution the reference computes from SHAP; Erion et al. 2021), batched.
 * For the explained input x [B,per], a background set bg [Nb,per] of the same trailing shape, n draws per sample and F_c the model's
 * output log-probability of class c:
 *     phi[b,c,e] = (1/n) * sum_{k=0..n-1} d[b,k,e] * dF_c/dx( r[b,k] )[e]
 *     d[b,k] = x[b] - bg[idx[b,k]]                      (one fp32 rounding)
 *     r[b,k] = bg[idx[b,k]] + fl(alpha[b,k] * d[b,k])   (product and sum rounded separately, no fma)
 * Draws (made by the caller on the host): one numpy.random.default_rng(seed); for b = 0..B-1 in order idx[b] = rng.integers(0, Nb, n),
 * then alpha[b] = rng.random(n).astype(float32).  idx i32 [B,n], alpha fp32 [B,n], on the device; an index outside 0..Nb-1 counts as
 * the nearest end.  per = C*H*W of a spectrogram in its logical layout [C,H,W], or Chans*T of an EEG input [1,Chans,T]: the layout the
 * model takes as an autograd leaf.  Rows are numbered globally j = b * n + k, sample-major; a call handles rows [row0, row0 + rows),
 * which may start and end inside a sample.  The sum over k is fp64 in ascending k (d * g of two floats is exact in fp64), carried
 * between calls in acc, so the result does not depend on how the rows were split into calls; it is divided by n in fp64 and rounded to
 * fp32 once.  No atomics.  B * n, B * per, Nb * per, rows * per and B * Kc * per stay below 2^31; every entry point refuses its limits
 * with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* The interpolants: out fp32 [rows, per], row r = r[b,k] of global row row0 + r.  Every element of every row is written exactly once. */
int bx_expgrad_rows(const float* x, const float* bg, const int* idx, const float* alpha, float* out, int B, int Nb, int n, int per, int row0,
                    int rows, bxStream stream);
/* The running sum of one class slot: acc[b,slot,e] += sum of d[b,k,e] * g[j - row0, e] over the rows j = b * n + k of the call that belong
 * to sample b, in ascending k.  acc fp64 [B,Kc,per] (Kc <= 32; the other slots are not touched), g fp32 [rows, per] the input gradient of
 * the call's rows, read exactly once; d is recomputed from x and the gathered background row and never stored. */
int bx_expgrad_accumulate(const float* x, const float* bg, const int* idx, const float* g, double* acc, int B, int Nb, int n, int per, int Kc,
                          int slot, int row0, int rows, bxStream stream);
/* Mean and map.  acc fp64 [BK,C,HW] -> values fp32 [BK,C,HW] = fl32(acc / n) and map fp32 [BK,HW] = fl32 of the fp64 sum of acc / n over
 * the C channels in ascending order (a sum keeps the attributions additive).  A spectrogram passes its C and HW = H*W; an EEG input
 * passes C = 1, HW = Chans*T and map = NULL (its map is values itself).  BK = B * Kc <= 65535. */
int bx_expgrad_finish(const double* acc, float* values, float* map, int BK, int C, int HW, int n, bxStream stream);
/* Gradient seeds of sample-major rows: seed fp32 [rows,K], row r = onehot(classes[(row0 + r) / n]) with classes i32 [B] on the device (a
 * class outside 0..K-1 counts as the nearest end), or onehot(class_all) for every row when classes is NULL. */
int bx_expgrad_seed(const int* classes, int class_all, float* seed, int B, int n, int K, int row0, int rows, bxStream stream);
/* The reference's per-electrode reduction: out[r] = fl32( (sum_t |v[r,t]|) / L ) for v fp32 [R,L].  The sum is fp64 in an order that does
 * not depend on the launch: 64 partial sums over t = l, l + 64, ... (ascending), added by a fixed pairwise tree.  R * L < 2^31. */
int bx_mean_abs_rows(const float* v, float* out, int R, int L, bxStream stream);
/* ---- SmoothGrad, SmoothGrad^2 and VarGrad (Smilkov et al. 2017; Hooker et al. 2019; Adebayo et al. 2018; Captum's NoiseTunnel), batched.
 * For the explained input x [B,per], n draws per sample, a noise scale sigma[b] and F_c the model's output log-probability of class c:
 *     row[b,k,e] = fl32( x[b,e] + fl32( sigma[b] * z[b,k,e] ) )            (product and sum rounded separately, no fma)
 *     g[b,k]     = dF_c/dx( row[b,k] ),    S1 = sum_k g,    S2 = sum_k g * g      (fp64, ascending k; g * g of a float is exact in fp64)
 *     BX_SMOOTHGRAD_MEAN  S1 / n                              (SmoothGrad)
 *     BX_SMOOTHGRAD_SQ    S2 / n                              (SmoothGrad^2)
 *     BX_SMOOTHGRAD_VAR   max(0, (S2 - S1 * S1 / n) / n)      (VarGrad: the population variance; four fp64 operations, each rounded)
 * each then rounded to fp32 once; the map is the largest |value| over the input's channels (saliency's convention).
 * Noise.  For flat element e of a sample, q = e >> 2:
 *     (w0,w1,w2,w3) = Philox4x32-10( counter = (q, k, b, 0), key = (seed & 0xffffffff, seed >> 32) )
 * the Random123 generator (Salmon et al., SC 2011): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; a round maps the counter c to
 * ( hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0) ); ten rounds, the key advanced by (0x9E3779B9, 0xBB67AE85) before
 * every round but the first.  Box-Muller in fp32 on a word pair (wa, wb), every operation rounded on its own:
 *     u = ((wa >> 8) + 1) 2^-24 in (0,1],  t = (wb >> 8) 2^-23 in [0,2)   (both exact),   r = sqrtf(-2 logf(u)),
 *     z_even = r cospif(t),  z_odd = r sinpif(t);
 * (w0,w1) gives elements 4q, 4q+1 and (w2,w3) gives 4q+2, 4q+3.  The draws of (b, k) depend on nothing else: a longer run extends a
 * shorter one, and how the rows are split into calls does not matter.  logf, cospif and sinpif are the device library's: z is pinned
 * to the exact Box-Muller value of (u, t) within a few units of 2^-24 max(1, r), not bit for bit; everything after z is.
 * Rows are numbered globally j = b * n + k, sample-major; a call handles rows [row0, row0 + rows), which may start and end inside a
 * sample.  The sums are carried between calls in S1 and S2.  No atomics.  B * n, B * per, rows * per and B * Kc * per stay below 2^31;
 * every entry point refuses its limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
enum { BX_SMOOTHGRAD_MEAN = 0, BX_SMOOTHGRAD_SQ = 1, BX_SMOOTHGRAD_VAR = 2 };
/* The paper's noise level: sigma[b] = fl32( level * | fl32( max_e x[b,e] - min_e x[b,e] ) | ), one workgroup per sample; the modulus only
 * clears the sign of a zero range, so the bits do not depend on the order the extremes are found in.  x finite, level >= 0 finite. */
int bx_smoothgrad_sigma(const float* x, float* sigma, int B, int per, float level, bxStream stream);
/* The noisy rows: out fp32 [rows, per], row r = row[b,k] of global row row0 + r; sigma fp32 [B].  One Philox block serves four
 * elements; 16-byte accesses when per % 4 == 0 and the pointers are 16-byte aligned, element by element otherwise; the noise lives in
 * registers only.  Every element of every row is written exactly once.  With x == NULL (and sigma == NULL) the same kernel writes z
 * itself: one code path computes z. */
int bx_smoothgrad_rows(const float* x, const float* sigma, float* out, int B, int n, int per, uint64_t seed, int row0, int rows, bxStream stream);
/* The running sums of one class slot: S1[b,slot,e] += sum of g[j - row0, e] and S2[b,slot,e] += sum of g[j - row0, e]^2 over the rows
 * j = b * n + k of the call that belong to sample b, in ascending k.  S1, S2 fp64 [B,Kc,per] (Kc <= 32; the other slots are not
 * touched), g fp32 [rows, per] the input gradient of the call's rows, read exactly once. */
int bx_smoothgrad_accumulate(const float* g, double* S1, double* S2, int B, int n, int per, int Kc, int slot, int row0, int rows, bxStream stream);
/* Values and map.  S1, S2 fp64 [BK,C,HW] -> values fp32 [BK,C,HW] of ``kind`` and map fp32 [BK,HW] = max over the C channels of
 * |values| (map may be NULL).  A spectrogram passes its C and HW = H*W; an EEG input passes C = 1, HW = Chans*T.  BK = B * Kc <= 65535. */
int bx_smoothgrad_finish(const double* S1, const double* S2, float* values, float* map, int BK, int C, int HW, int n, int kind, bxStream stream);
/* ---- Infidelity and max-sensitivity of an explanation (Yeh et al., NeurIPS 2019; Captum's metrics.infidelity and
 * metrics.sensitivity_max).  Infidelity, for the explained input x [B,...], an attribution Phi [B,Kc,cells] whose cells are the features,
 * n draws per sample, a noise scale sigma[b] and s_c the model's fp32 probability (or log-probability) of class c:
 *     I[b,k,cell]  = fl32( sigma[b] * z[b,k,cell] )                       z: SmoothGrad's stream above, with `cell` as its element
 *     row[b,k,e]   = fl32( x[b,e] - I[b,k,cell(e)] )                      (product and difference rounded separately, no fma)
 *     d[b,c,k]     = sum_cell (double)I[b,k,cell] * (double)Phi[b,c,cell] (fp64; every product is exact)
 *     Delta[b,c,k] = (double)s_c(x[b]) - (double)s_c(row[b,k])
 *     infid[b,c]   = (1/n) sum_k ( beta d - Delta )^2                     (fp64, ascending k; product, difference, square, sum and the
 *                                                                          division by n each rounded on their own)
 *     beta = 1, or with `normalize` beta[b,c] = (sum_k d Delta) / (sum_k d d), 0 when the denominator is 0   (Captum's scaling)
 * Cells.  A spectrogram [C,H,W]: elements (cells = C*H*W, cell = its NCHW offset in the sample) or pixels (cells = H*W, one draw moves
 * the C channels of a pixel).  An EEG input [1,Chans,T]: elements (cells = Chans*T) or time columns (cells = T, one draw moves every
 * electrode).  z[b,k,cell] is word cell & 3 of the Philox block of counter (cell >> 2, k, b, 0): bx_smoothgrad_rows with x == NULL and
 * per = cells writes exactly these draws.
 * Rows are written straight in the model's layouts -- spectrogram rows NHWC with Cp = 8 channels in `dtype` (channels C..7 zero, the
 * rounding of bx_nchw_to_nhwc), EEG rows fp32 [rows,1,Chans,T] -- in the chunk form of the perturb-and-predict writers: a call writes
 * samples b0 .. b0+nb-1 and draws n0 .. n0+n-1 of the N draws, row (b - b0) * n + (k - n0); x and sigma are the whole arrays.  The noise
 * lives in registers only.  The order of the sum d is a function of `cells` alone: the noise is drawn again, thread t of one workgroup
 * per (b, k) takes the Philox blocks t, t + 256, ... in ascending order and the 256 partial sums meet in a pairwise tree over the thread
 * index (stride 128, 64, .., 1).  No atomics; no bit of d depends on how rows were split into calls.  Every entry point refuses its
 * limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
/* out [nb*n,H,W,Cp] in dtype (16-byte aligned); per_pixel != 0: pixel cells.  1 <= C <= 4, Cp = 8; 16-byte loads when H*W % 4 == 0 and
 * x is 16-byte aligned, element by element otherwise. */
int bx_infidelity_rows_spec(const float* x, const float* sigma, void* out, int B, int C, int H, int W, int Cp, int per_pixel, int N, int b0,
                            int nb, int n0, int n, uint64_t seed, int dtype, bxStream stream);
/* out fp32 [nb*n,1,Chans,T]; per_column != 0: time-column cells. */
int bx_infidelity_rows_eeg(const float* x, const float* sigma, float* out, int B, int Chans, int T, int per_column, int N, int b0, int nb, int n0,
                           int n, uint64_t seed, bxStream stream);
/* d fp64 [B,Kc,n]: the entries of the global rows j = b * n + k in [row0, row0 + rows) are written, every class of them (Kc <= 32);
 * phi fp32 [B,Kc,cells], sigma fp32 [B]. */
int bx_infidelity_dot(const float* phi, const float* sigma, double* d, int B, int n, int cells, int Kc, uint64_t seed, int row0, int rows,
                      bxStream stream);
/* One thread per explained (sample, class) pair q: classes i32 [B] on the device (Kc = 1; a class outside 0..K-1 counts as the nearest
 * end) or NULL for every class (Kc = K <= 32).  d fp64 [B,Kc,n], S fp32 [B,n,K] the scores of the rows, clean fp32 [B,K] those of the
 * unperturbed input -> infid, beta fp64 [B,Kc] and drops fp64 [B,Kc,n] = Delta. */
int bx_infidelity_finish(const double* d, const float* S, const float* clean, const int* classes, double* infid, double* beta, double* drops, int B,
                         int n, int K, int normalize, bxStream stream);
/* Max-sensitivity, for an explanation function Phi, n draws per sample and a radius r[b]:
 *     u[b,k,e]   = (float)(w >> 8) * 2^-23 - 1  in [-1, 1), exact;  w = word e & 3 of Philox4x32-10( counter = (e >> 2, k, b, 1), key as above )
 *     row[b,k,e] = fl32( x[b,e] + fl32( r[b] * u[b,k,e] ) )         fp32 in the input's own layout, always elementwise
 *     sens[b]    = max_k || Phi(row[b,k]) - Phi(x[b]) ||_2 / || Phi(x[b]) ||_2,   the denominator 1 when the norm is 0   (Captum's rule)
 * Counter word 3 is 1: a stream apart from the normal one.  The uniformly perturbed rows, out fp32 [rows, per], row r = global row
 * row0 + r = b * n + k; with x == NULL (and radius == NULL) the same kernel writes u itself. */
int bx_sensitivity_rows(const float* x, const float* radius, float* out, int B, int n, int per, uint64_t seed, int row0, int rows, bxStream stream);
/* dist[r] = sqrt( sum_e ( (double)a[r,e] - (double)ref[(row0 + r) / n, e] )^2 ) for a fp32 [rows, per], ref fp32 [B, per]; ref == NULL: the
 * norm of a[r].  One workgroup per row; thread t sums e = t, t + 256, ... in ascending order, then the tree above: fixed order. */
int bx_sensitivity_dist(const float* a, const float* ref, double* dist, int B, int n, int per, int row0, int rows, bxStream stream);
/* sens[b] = max_k dist[b,k] / (norms[b] == 0 ? 1 : norms[b]); dist fp64 [B,n], norms and sens fp64 [B]. */
int bx_sensitivity_finish(const double* dist, const double* norms, double* sens, int B, int n, bxStream stream);
/* ---- Blur Integrated Gradients (Xu, Venugopalan, Sundararajan, CVPR 2020; PAIR's saliency.BlurIG) and the Gaussian blur behind it.
 * For the explained input x [B,C,H,W] (an EEG input [B,1,Chans,T] is C = 1, H = Chans, W = T), n steps, max_sigma, grad_step = eps and
 * F_c the model's output log-probability of class c:
 *   Schedule (host, Python floats, as saliency computes it): sigma_i = i * max_sigma / n, or sqrt(i * max_sigma / n), i = 0..n;
 *     w_i = -(sigma_{i+1} - sigma_i).
 *   Taps (host, numpy fp64, rounded once to fp32; scipy.ndimage.gaussian_filter's with truncate 4): R(s) = int(4 s + 0.5),
 *     g_s[t] = exp(-0.5 / s^2 * t^2) / sum_t exp(..), t = -R..R; g_0 is the identity (R = 0).  Per step a = g_{sigma_i},
 *     b = g_{sigma_i + eps}, d = (b - a) / eps formed in fp64 with a zero-padded to b's radius.
 *   Rows: zero padding outside the image (scipy's mode="constant"), per channel, filters along `axes`.  With A, B, D the filters of
 *     the taps a, b, d along x (W) or y (H):
 *       both axes:  X_i = A_y A_x x,   D_i = B_y (D_x x) + D_y (A_x x)      -- exactly ( blur_{sigma_i+eps}(x) - X_i ) / eps in real
 *                   arithmetic (B_y B_x - A_y A_x = B_y (B_x - A_x) + (B_y - A_y) A_x), without the cancellation of the literal form
 *       one axis:   X_i = A x,         D_i = D x
 *     Every filter is a chain of fmaf(tap, input, sum) from +0 in ascending tap order over the taps that can land inside the image
 *     (a tap beyond a filter's radius, where the chain reaches one, counts as 0); the horizontal results Ha = A_x x and Hd = D_x x are
 *     rounded to fp32 once; D's vertical chain is one accumulator that takes, for each tap t in ascending order, b[t] Hd[y+t] and then
 *     d[t] Ha[y+t].  Where R_b = 0 the row is x bit for bit (signs of zero included) and D is +0.
 *   Attribution: values[b,c] = sum_{i<n} w_i * dF_c/dx(X_i) (.) D_i  (fp64: g * D of two floats is exact, w_i * (g * D) and the sum are one
 *     rounding each, ascending i, carried between calls), rounded to fp32 once (bx_expgrad_finish with n = 1, which also gives the
 *     channel-summed map).  endpoint[b] = F(blur_{sigma_n}(x[b])); delta[b,c] = sum_e values - (F_c(x) - endpoint_c): the completeness
 *     error of the left Riemann sum, reported, not minimised.
 * The tap table.  taps fp32 [entries, 3, tap_width]: filters a, b, d of an entry, tap t at index tap_width / 2 + t; tap_width is odd and
 * at least 2 max R_b + 1.  radius i32 [entries, 2] = (R_a, R_b) of an entry, R_a <= R_b <= tap_width / 2 (values outside are clamped);
 * the kernel reads a only within R_a and b, d only within R_b, so what the table holds beyond them does not matter.  Both on the
 * device.  Rows are numbered globally j = b * n + i, sample-major; a call handles rows [row0, row0 + rows), which may start and end
 * inside a sample.  Row j uses entry i (per_sample == 0: entries = n, the schedule shared by the samples) or entry j (per_sample != 0:
 * entries = B * n, a sigma of its own for every sample; bx_blur_rows with n = 1 is then a Gaussian blur with one sigma per sample).
 * B * n, B * per, rows * per and B * Kc * per stay below 2^31; every entry point refuses its limits with BX_EINVAL / BX_EUNSUPPORTED
 * before any pointer is touched. */
enum { BX_BLUR_AXES_HW = 0, BX_BLUR_AXES_H = 1, BX_BLUR_AXES_W = 2 };
#define BX_BLUR_MAX_RADIUS 16384
/* The rows: rows_out fp32 [rows,C,H,W] = X and deriv_out fp32 [rows,C,H,W] = D (NULL: X alone, the filters b and d are not read).  Every
 * element of every row is written exactly once; 16-byte accesses when W % 4 == 0 and x, rows_out and deriv_out are 16-byte aligned,
 * element by element otherwise.  Both axes: a workgroup owns (row, channel, strip of 16, 8 or 4 columns), keeps Ha and Hd of its strip
 * for all H image rows in LDS and filters vertically from there -- no global intermediate; the widest strip is taken for which
 *     4 * ( 6 TP + (2, or 1 without D) * 4 ceil(H / 4) * (strip + 4) ) <= 65536 bytes,   TP = 4 ceil((RC + 3) / 4) + 4,
 * RC = min(tap_width / 2, max(H, W) - 1): only taps that can join two points of the image are staged.  A shape whose 4-column strip
 * does not fit returns BX_EUNSUPPORTED (with D and radius 200: H <= 944).  One axis: no intermediate, 16 TP <= 65536 with RC from the
 * filtered extent.
 * A thread produces four adjacent outputs along the filter axis from each loaded group of four inputs; the taps of a row are staged in
 * LDS once per workgroup.  tap_width / 2 <= BX_BLUR_MAX_RADIUS, C <= 65535 (BX_EUNSUPPORTED above). */
int bx_blur_rows(const float* x, const float* taps, const int* radius, float* rows_out, float* deriv_out, int B, int n, int C, int H, int W, int axes,
                 int tap_width, int per_sample, int row0, int rows, bxStream stream);
/* The running sum of one class slot: acc[b,slot,e] += sum of w[i] * ( (double)g[j - row0, e] * (double)deriv[j - row0, e] ) over the rows
 * j = b * n + i of the call that belong to sample b, in ascending i.  acc fp64 [B,Kc,per] (Kc <= 32; the other slots are not touched),
 * w fp64 [n] on the device, g and deriv fp32 [rows, per]: the input gradient and D of the call's rows.  One thread per element, no
 * atomics: no bit depends on how the rows were split into calls. */
int bx_blurig_accumulate(const float* g, const float* deriv, const double* w, double* acc, int B, int n, int per, int Kc, int slot, int row0, int rows,
                         bxStream stream);
/* out[r] = sum_t (double)v[r,t] for v fp32 [R,L], out fp64 [R]: the sum behind delta, one row per (sample, class), in the order of
 * bx_mean_abs_rows -- 64 partial sums over t = l, l + 64, ... (ascending), added by a fixed pairwise tree.  R * L < 2^31. */
int bx_blurig_sum_rows(const float* v, double* out, int R, int L, bxStream stream);
/* ---- Guided Integrated Gradients (Kapishnikov et al., CVPR 2021; PAIR's saliency.GuidedIG): the adaptive path from a baseline to the
 * input that moves, at every step, only the cells with the smallest |gradient|.
 * One row is one (sample b, explained class c) pair of P cells, row r = b * Kc + slot.  fp32: the input x_in, the baseline x_base, the
 * moving point x (it starts at x_base) and g, the gradient of F_c (the model's output log-probability of class c) at x.  fp64: attr [P],
 * which starts at 0.  n steps, fraction in (0, 1], max_dist in [0, 1]; k = floor((P - 1) * fraction), computed by the host in fp64
 * (numpy's quantile(.., 'lower') index).  Every difference below is taken in fp64 from the fp32 values.
 *   L_total = SUM_e |x_in - x_base|.  A row with L_total = 0 never moves: its values are 0.
 *   X(alpha)_e = fl32( x_base_e + alpha * (x_in_e - x_base_e) ), alpha fp64; the product and the sum are one fp64 rounding each (no fma),
 *     then one rounding to fp32.  X(alpha) is x_in bit for bit for alpha >= 1 and x_base bit for bit for alpha <= 0.
 *   Step i = 0..n-1, with g taken once at the top of the step:  alpha = (i + 1) / n,  a_min = max(alpha - max_dist, 0),
 *     a_max = min(alpha + max_dist, 1),  X_min = X(a_min),  X_max = X(a_max),  L_target = L_total * (1 - alpha).  A NaN among the row's g
 *     stops the row before anything of the step is written (status BX_GUIDED_NAN).  Otherwise repeat (one repetition is a pass):
 *     1. x_old = x.
 *     2. a_e = (x_e - x_base_e) / (x_in_e - x_base_e) in fp64, a_max for a cell with x_in_e == x_base_e; where a_e < a_min, x_e = X_min_e.
 *     3. L_cur = SUM_e |x_in_e - x_e|.
 *     4. If |L_target - L_cur| <= max(1e-9 * max(|L_target|, |L_cur|), 1e-9) (Python's math.isclose): attr_e += (x_e - x_old_e) * g_e and
 *        the step ends.
 *     5. A cell has arrived when x_e == X_max_e (fp32 equality).  key_e = |g_e| for a cell that has not arrived, +inf for one that has;
 *        theta = the k-th smallest key (0-based, duplicates counted); S = { e not arrived : key_e <= theta }: every tie of theta is in S,
 *        theta = +inf selects every cell that has not arrived.
 *     6. L_S = SUM_e ( e in S ? |X_max_e - x_e| : 0 );  gamma = (L_cur - L_target) / L_S if L_S > 0, else +inf.
 *     7. On S:  gamma > 1: x_e = X_max_e;  0 < gamma <= 1: x_e = fl32( x_e + gamma * (X_max_e - x_e) ), product and sum one fp64 rounding
 *        each;  gamma <= 0 (rounding alone): nothing moves.
 *     8. attr_e += (x_e - x_old_e) * g_e: product and sum one fp64 rounding each; g is the gradient itself, not the key.
 *     9. Go on while gamma > 1 and L_S > 0.  L_S = 0 means that S is empty, which means that every cell has arrived: no further pass can
 *        move anything, the step ends.  (With max_dist = 0 every step ends this way once fp32 rounding keeps L_cur from meeting
 *        L_target to nine digits; the result is then the left Riemann sum SUM_i g(X(i/n)) * (X((i+1)/n) - X(i/n)).)
 *   Every pass that goes on makes at least min(k + 1, cells left) further cells arrive, so a step has at most ceil(P / (k + 1)) + 2
 *   passes; the host passes that number as `cap`, and a row that has made cap passes and would go on stops with BX_GUIDED_CAP.
 *   A row whose status is not 0 is left alone by every later step.  values = fl32(attr) (bx_expgrad_finish with n = 1).
 * Sums (L_total, L_cur, L_S), fp64 in an order that depends on P alone: 1024 partial sums over e = t, t + 1024, ... (ascending); inside
 * each group of 64 consecutive partials the xor butterfly (offsets 32, 16, .., 1: p_l += p_{l ^ o}); the 16 group totals added in
 * ascending order.
 * The kernel: one workgroup per row, a cell is owned by one thread through all sweeps of all passes; theta by an exact radix select
 * over the keys' bit patterns (non-negative fp32 values and +inf order as unsigned integers), four digits of eight bits, integer LDS
 * counters.  No loop is unbounded, no workgroup waits for another.  1 <= P < 2^20, R = B * Kc <= 65535, R * P < 2^31 and R * n < 2^31:
 * anything else is BX_EUNSUPPORTED before a pointer is touched. */
enum { BX_GUIDED_OK = 0, BX_GUIDED_CAP = 1, BX_GUIDED_NAN = 2 };
/* x fp32 [R,P] = the baseline of the row's sample, attr fp64 [R,P] = 0, L_total fp64 [R], status i32 [R] = 0.  x_in fp32 [B,P]; base
 * fp32 [B,P] (base_rows != 0) or one value for every cell (base_rows == 0, base[0]). */
int bx_guided_ig_init(const float* x_in, const float* base, int base_rows, float* x, double* attr, double* L_total, int* status, int B, int Kc, int P,
                      bxStream stream);
/* All passes of step i for rows row0 .. row0+rows-1 in one launch.  x_in, x_base fp32 [B,P]; x fp32 [R,P], attr fp64 [R,P], L_total
 * fp64 [R], status i32 [R] and iters i32 [R,n] are the whole arrays; g fp32 [rows,P] holds the gradients of the call's rows.  iters[r,i]
 * = the passes row r made in this step (0 for a row that is stopped, stops with BX_GUIDED_NAN or has L_total = 0). */
int bx_guided_ig_step(const float* x_in, const float* x_base, float* x, const float* g, double* attr, const double* L_total, int* status, int* iters,
                      int B, int Kc, int P, int i, int n, int k, double max_dist, int cap, int row0, int rows, bxStream stream);
/* ---- Spectral attributions of the EEG input: amplitude gradients and spectral occlusion (Schirrmeister et al., Hum. Brain Mapp. 2017;
 * braindecode's compute_amplitude_gradients).  For a row x[0..T) (one electrode of one sample), F = T / 2 + 1 bins (integer division):
 *   Transform:  X_f = sum_t x_t (cos th - i sin th),  th = 2 pi ((f t) mod T) / T,  f = 0..F-1.
 *   Weights:    c_0 = 1; c_{T/2} = 1 when T is even; c_f = 2 otherwise (the bins a real signal's spectrum holds twice).
 *   Phase:      u_f = X_f / |X_f|, and 1 + 0i when X_f is exactly zero (numpy's angle(0) = 0).
 *   With g the gradient of the explained log-probability F_c by the row and G its transform:
 *     amplitude gradient    dF_c/dA_f     = (c_f / T) Re(u_f conj(G_f))    -- autograd through irfft(A e^{i phi}) by A, braindecode's
 *     gradient x amplitude  A_f dF_c/dA_f = (c_f / T) Re(X_f conj(G_f))    -- per electrode it sums over f to sum_t g_t x_t (Parseval)
 *   Path form (steps = n > 1): g = sum_k w_k dF_c/dx(alpha_k x) with (alpha, w) the n Gauss-Legendre nodes and weights on [0, 1]
 *     (integrated_gradients' ig_nodes); the points alpha x share x's phase, so gradient x amplitude is integrated gradients from the
 *     zero-amplitude baseline per frequency: sum_{e,f} values = F_c(x) - F_c(0) up to the quadrature error (delta, reported).
 *   Band component:  y_q[t] = (1 / T) sum_{f in [lo_q, hi_q)} c_f (Re X_f cos th - Im X_f sin th); a band-stopped row is fl32(x - y_q).
 *   Bands: bin f belongs to (lo, hi) iff lo <= f fs / T < hi, decided on the host in fp64 as lo T <= f fs < hi T: one bin range
 *     [f_lo, f_hi) per band (fs absent: edges in cycles per sample).  A band without a bin sums to 0 and stops nothing.
 * The twiddle table tw fp64 [T,2] = (cos, sin)(2 pi j / T), j = 0..T-1, is computed on the host in fp64 and lives on the device; the
 * kernels walk j = (f t) mod T by integer add-and-wrap: no sincos and no fp32 angle on the device.  Every sum is fp64, one fma per
 * term, in an order that depends on T or the bin range alone (ascending t, ascending f); no atomics.  1 <= T <= BX_SPECTRAL_MAX_T
 * (BX_EUNSUPPORTED above); a workgroup transforms 8 rows at once, one table entry serving all of them: the table is staged in LDS
 * (T <= 4096; read from global memory above), the row values, which are the same for every lane of a wave, come through the scalar cache.  Every entry point refuses its limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
enum { BX_SPECTRAL_AMPLITUDE_GRADIENT = 0, BX_SPECTRAL_GRADIENT_X_AMPLITUDE = 1 };
enum { BX_SPECTRAL_CELLS_BAND = 0, BX_SPECTRAL_CELLS_ELECTRODE_BAND = 1 };
#define BX_SPECTRAL_MAX_T 8192
/* x fp32 [R,T] -> re, im fp64 [R,F].  A workgroup owns (8 rows, 256 bins), a thread one bin of each, ascending t.  Per bin
 * |error| <= (T + 4) 2^-53 sum_t |x_t|; a zero row gives exactly 0.  R * T < 2^31. */
int bx_rdft_rows(const float* x, const double* tw, double* re, double* im, int R, int T, bxStream stream);
/* The running sum of one class slot: acc[b,slot,e] += w[k] * (double)g[j - row0, e] over the rows j = b * n + k of the call that belong
 * to sample b, in ascending k (the product and the sum are one fp64 rounding each).  acc fp64 [B,Kc,per] (Kc <= 32; the other slots are
 * not touched), w fp64 [n] on the device, g fp32 [rows,per].  Rows are numbered globally, sample-major; a call handles rows
 * [row0, row0 + rows), which may start and end inside a sample.  One thread per element, no atomics: no bit depends on how the rows
 * were split into calls. */
int bx_spectral_accumulate(const float* g, const double* w, double* acc, int B, int n, int per, int Kc, int slot, int row0, int rows, bxStream stream);
/* values fp32 [B,Kc,Chans,F] from the fp64 gradient sums gsum [B,Kc,Chans,T] and X = (re, im) fp64 [B*Chans,F] of the samples, by
 * `kind`.  G_f is computed in registers with the transform body of bx_rdft_rows and never stored; the value is formed in fp64 and
 * rounded to fp32 once. */
int bx_spectral_values(const double* gsum, const double* re, const double* im, const double* tw, float* values, int B, int Kc, int Chans, int T, int kind,
                       bxStream stream);
/* out fp64 [R,nb]: out[r,q] = sum of (double)values[r,f] over f in [bins[q,0], bins[q,1]) in ascending f, from +0; bins int32 [nb,2] on
 * the device (ranges are clamped to 0 <= lo <= hi <= F).  values fp32 [R,F]. */
int bx_band_sum(const float* values, const int* bins, double* out, int R, int F, int nb, bxStream stream);
/* The rows of spectral occlusion in the EEG layout: out fp32 [B*n,1,Chans,T], rows (b, j) for j in [n0, n0 + n), sample-major.
 * cells = BAND: N = nb, row j = q has every electrode band-stopped.  cells = ELECTRODE_BAND: N = nb * Chans, row j = q * Chans + e has
 * electrode e band-stopped; every other electrode is x bit for bit, zero signs included, as is every electrode for a band without a
 * bin.  x fp32 [B,1,Chans,T], (re, im) fp64 [B*Chans,F] its transform.  y_q is summed in fp64 in ascending f, divided by T and
 * subtracted from double(x); the result is rounded to fp32 once. */
int bx_bandstop_rows(const float* x, const double* re, const double* im, const double* tw, const int* bins, float* out, int B, int Chans, int T, int nb,
                     int cells, int n0, int n, bxStream stream);
/* ---- Similarity of two attribution maps and the model parameter randomization test (Adebayo et al., "Sanity Checks for Saliency
 * Maps", NeurIPS 2018; Ghorbani et al., AAAI 2019; scipy.stats.spearmanr / pearsonr, scikit-image's structural_similarity).  A map is a
 * row of N = H * W cells, 1 <= N < 2^20 (the limit of bx_rank_desc; BX_EUNSUPPORTED above, before any pointer is touched); R rows.
 * With `abs` every kernel reads |v| in registers.
 *   pearson   r = sum (x - mx)(y - my) / sqrt( sum (x - mx)^2 * sum (y - my)^2 ), clamped to [-1, 1] as scipy does; fp64, two
 *             passes (means first), every product and sum rounded on its own.  One workgroup of 256 per row: thread t takes the cells
 *             t, t + 256, ... in ascending order and the 256 partial sums meet in a pairwise tree over the thread index (stride 128,
 *             64, .., 1), the order of bx_infidelity_dot: a function of N alone, no atomics.  NaN when either centred sum of squares
 *             is 0 (scipy's result for a constant input).
 *   spearman  the same correlation over tie-averaged ranks (scipy.stats.rankdata(method="average") of the negated keys, minus 1):
 *             avg[i] = #{key > key_i} + (#{key == key_i} - 1) / 2, key as in bx_rank_desc (NaN counts as -inf, -0.0 equals +0.0): a
 *             half-integer below 2^20, exact in fp32.
 *   topk      |{i : rank_a[i] < k and rank_b[i] < k}| / k over the stable ranks of bx_rank_desc: an exact integer divided once.
 *   ssim      the mean of S over the positions whose whole window lies inside the map (scikit-image's crop of (win - 1) / 2 per side,
 *             so no padding rule enters).  F is the separable filter of the `win` taps (odd) along each map axis of extent > 1; an axis
 *             of extent 1 is not filtered, and such a map is a line of H * W cells.  NP = win^(filtered axes).  With the cells X, Y:
 *               ux = F(X), uy = F(Y), uxx = F(X X), uyy = F(Y Y), uxy = F(X Y)
 *               vx = c (uxx - ux^2), vy = c (uyy - uy^2), vxy = c (uxy - ux uy)         c = cov_norm: NP / (NP - 1) for the uniform
 *               C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = data_range                         window, 1 for the Gaussian one
 *               S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
 *             Cells: with the four range arrays X = ((double)x - lo) / ((double)hi - (double)lo) per row, 0 everywhere when hi == lo
 *             (the rescaling to [0, 1] of Adebayo et al.; pass data_range = 1); without them the raw values.  All fp64: a moment is
 *             the sum of tap * value in ascending tap order along the row, then of tap * moment down the column.
 *   re-initialisation  p[e] = fl32( bound * u ), u = (float)(w >> 8) * 2^-23 - 1 in [-1, 1), w = word e & 3 of
 *             Philox4x32-10( counter = (e >> 2, j, s, 2), key = (seed & 0xffffffff, seed >> 32) ): j the tensor's position in its
 *             layer's parameters, s the layer's position in the test's list.  Counter word 3 is 2: a stream apart from the Gaussian
 *             (0) and the uniform (1) one.  bound = 1 / sqrt(fan_in) is torch's default for Conv2d / Linear weights and biases.
 * Every entry point refuses its limits with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched. */
#define BX_SSIM_MAX_WIN 63
/* avg fp32 [R,N] from values fp32 [R,N] and ranks i32 [R,N] = bx_rank_desc of the same keys (of |values| with abs: bx_rank_desc has no
 * flag, the caller ranks a copy of |values|; here |v| is formed in registers).  The keys are scattered to sorted order, then every cell
 * finds the two ends of its tie run by binary search.  workspace: bx_rank_average_workspace bytes (0 for refused shapes), 4-byte
 * aligned.  R <= 65535. */
size_t bx_rank_average_workspace(int R, int N);
int bx_rank_average(const float* values, const int* ranks, float* avg, int R, int N, int abs, void* workspace, size_t workspace_bytes, bxStream stream);
/* r fp64 [R]: pearson of the rows of a and b fp32 [R,N], values or ranks. */
int bx_map_corr(const float* a, const float* b, double* r, int R, int N, int abs, bxStream stream);
/* out fp64 [R]: topk of the rank rows ranks_a, ranks_b i32 [R,N]; 1 <= k <= N. */
int bx_topk_overlap(const int* ranks_a, const int* ranks_b, double* out, int R, int N, int k, bxStream stream);
/* lo, hi fp32 [R]: the extremes of every row of v fp32 [R,N] (of |v| with abs); a NaN cell is skipped.  (bx_smoothgrad_sigma returns
 * only level * (max - min) and bx_scorecam_range the extremes of bilinearly up-sampled planes: neither gives lo and hi of a row as it
 * stands.) */
int bx_row_minmax(const float* v, float* lo, float* hi, int R, int N, int abs, bxStream stream);
/* out fp64 [R]: ssim of the maps a, b fp32 [R,H,W].  taps fp64 [win] on the device; lo_a, hi_a, lo_b, hi_b fp32 [R] (all four or none).
 * A workgroup owns (map, strip of SW columns of positions): it keeps the five moments filtered along the rows, for all H rows of its
 * strip, in LDS as fp64 and filters down the columns from there -- no global intermediate; thread t adds S of the strip's positions
 * t, t + 256, ... (row-major) and the 256 partials meet in the butterfly and then in wave order.  A map's mean is the sum of its strip
 * sums in ascending strip order (a second launch) divided by the number of positions.  No atomics.
 * SW = bx_ssim_strip(H, W, win): the widest of 64, 32, 16, 8, 4 with H * SW <= 1624 (five planes of H * SW doubles beside the taps in
 * 65536 bytes), halved while half of it still covers all W - win + 1 columns; a line (an axis of extent 1) counts as H = 1.  The largest
 * map with two filtered axes therefore has H <= 406 rows (any W within N < 2^20); above, BX_EUNSUPPORTED (bx_ssim_strip: 0).
 * win odd, <= BX_SSIM_MAX_WIN and <= every filtered extent (BX_EINVAL: scikit-image refuses such a window too); R <= 65535.
 * workspace: bx_ssim_rows_workspace bytes (0 for refused shapes), 8-byte aligned. */
int bx_ssim_strip(int H, int W, int win);
size_t bx_ssim_rows_workspace(int R, int H, int W, int win);
int bx_ssim_rows(const float* a, const float* b, const double* taps, const float* lo_a, const float* hi_a, const float* lo_b, const float* hi_b,
                 double data_range, double cov_norm, double* out, int R, int H, int W, int win, int abs, void* workspace, size_t workspace_bytes,
                 bxStream stream);
/* p fp32 [n] on the device, 1 <= n < 2^31: the re-initialisation above.  One Philox block serves four elements; 16-byte stores when p is
 * 16-byte aligned, the partial last block element by element. */
int bx_param_uniform(float* p, size_t n, float bound, uint64_t seed, uint32_t j, uint32_t s, bxStream stream);
/* ---- Fusion SHAP: the exact Shapley values of the votes the two branches hand to the fusion head (Shapley 1953; Lundberg & Lee,
 * NeurIPS 2017, the interventional value function of Janzing et al., AISTATS 2020).  The model is a late fusion: each branch emits K
 * log-probabilities (its votes), the head F is cat -> Linear(2K,Hd) -> ReLU -> Linear(Hd,K) -> LogSoftmax (bx_fusion_head_fwd).  For
 * sample b the fused input is z = (e_0..e_K-1, s_0..s_K-1); vote i < K is the EEG branch's, vote K + i the spectrogram branch's.  A
 * player is a group of votes; the M <= 16 players partition the 2K votes.  For a coalition S of players, a class c and the background
 * rows z(j), j < Nb (a row supplies both branches' votes of the same background sample: a joint background):
 *     v_c(S) = (1/Nb) sum_j score_c( F( z on the votes of S, z(j) on the others ) )
 *     phi_i  = sum over S without i of |S|! (M - |S| - 1)! / M! * ( v(S + i) - v(S) )           over all 2^M coalitions
 * so that sum_i phi_i = v(all) - v(none) = score(sample) - mean score(background).  The modality game is the M = 2 game of {all EEG
 * votes}, {all spectrogram votes}; it is not the sum of its members' values in a finer game.  interaction = v(all) - v(EEG) - v(spec)
 * + v(none) of that game: positive when the two modalities reinforce each other for the class.
 * Every entry point refuses its limits with BX_EINVAL before any pointer is touched. */
#define BX_FUSION_SCORE_PROB 0
#define BX_FUSION_SCORE_LOGPROB 1
/* The values of a list of coalitions.  e_x, s_x fp32 [B,K] (the samples' votes), e_bg, s_bg fp32 [Nb,K] (the background rows'), masks
 * u32 [NS] on the device: bit i set = vote i comes from the sample, clear = from the background row; bits 2K.. are ignored.  The
 * players are expanded to vote masks by the caller, and the four masks of the modality game are ordinary entries of the list.  w1
 * [Hd,2K], b1 [Hd], w2 [K,Hd], b2 [K]: the head.  v fp64 [B,NS,K], every element written.
 * Arithmetic, the same for every mask.  fp32 with the clean head's operations.  The 2K votes are cut into groups of at most 8: for
 * K <= 8 the EEG half and the spectrogram half, for K > 8 votes 0..7, 8..K-1, K..K+7, K+8..2K-1.  The partial sum of a group is one fmaf
 * chain over its votes in ascending order, the first group's starting from b1[h] and the others' from 0; the pre-activation is the
 * groups' partial sums added in group order, ((g0 + g1) + g2) + g3.  (The clean head runs one chain over all 2K votes: the two differ
 * by the rounding of the joins.)  Then max(., 0); logit_k = one fmaf chain over h = 0..Hd-1 starting from b2[k], the clean head's order;
 * the max-shifted log-sum-exp in class order.  BX_FUSION_SCORE_LOGPROB scores the log-probability, BX_FUSION_SCORE_PROB
 * exp(lp_k - max lp) / sum_k exp(lp_k - max lp), which is bx_softmax_rows of it.  The mean over the background is an fp64 running sum
 * of the fp32 scores in the order j = 0..Nb-1, divided by Nb once.  No atomics; a thread owns a coalition from its first table read to
 * its store, so no bit of v depends on NS, on the position of a mask in the list, on how a list is cut into calls or on the grid.
 * A workgroup holds the groups' partial sums for every setting of a group's bits in LDS, per (sample, background row) pair and tile of
 * hidden units -- sum_g 2^bits(g) floats per hidden unit beside the second layer's tile, 64 KB at the most -- so a coalition costs one
 * LDS read per group, the adds, the ReLU and K multiply-adds per hidden unit.
 * 1 <= K <= 16 (a mask has 32 bits), 2K <= Hd <= 1024, B <= 65535, B * NS * K < 2^31. */
int bx_fusion_values(const float* e_x, const float* s_x, const float* e_bg, const float* s_bg, const uint32_t* masks, const float* w1,
                     const float* b1, const float* w2, const float* b2, int score_kind, double* v, int B, int Nb, int NS, int K, int Hd,
                     bxStream stream);
/* The Shapley sum.  v fp64 [R, 2^M]: row r holds one (sample, class) pair's values indexed by the coalition's integer (bit i = player
 * i); weights fp64 [M]: weights[s] = s! (M - s - 1)! / M!, the host's table; phi fp64 [R,M].  phi[r,i] is the sum over the coalitions
 * without player i, in ascending order of their integer, of weights[|S|] * (v[S + i] - v[S]); the difference, the product and the sum
 * are rounded one by one.  One thread per (row, player), no atomics.  1 <= M <= 16, R * 2^M < 2^31.  M = 2 on the rows (none, EEG, spec,
 * all) is the modality game. */
int bx_shapley_exact(const double* v, const double* weights, double* phi, int R, int M, bxStream stream);
/* out[r] = ((v[r,3] - v[r,1]) - v[r,2]) + v[r,0] of the modality game's rows v fp64 [R,4] = (none, EEG, spec, all).  R < 2^29. */
int bx_fusion_interaction(const double* v, double* out, int R, bxStream stream);
/* ---- Optimised perturbation masks (Fong & Vedaldi, ICCV 2017, "meaningful perturbations"; the basis of TorchRay's extremal
 * perturbations): per (sample, class) row the smallest smooth mask whose removal (deletion) or whose preservation alone changes the
 * class score is learned by Adam; the model's forward and backward passes between the launches are its own kernels.
 * Mask domain [Hm,Wm], as for RISE: [H,W] of a spectrogram (one value for all C channels of a pixel), [Chans,T] of an EEG input, or [1,T]
 * (a time column across electrodes); Hm * Wm < 2^20.  Grid gh x gw, 1 <= gh <= min(32, Hm), 1 <= gw <= min(32, Wm).
 * Row r = b * Kc + slot owns a parameter grid m_r fp32 [gh,gw] in [0, 1] (1.0 at the start) and the Adam moments mu_r, nu_r fp64 [gh,gw]
 * (0 at the start).
 * Up-sampling M = U(m): bilinear, align_corners=False, to Hm x Wm, in fp32 without fused multiply-adds (bx_resize_bilinear's
 * convention).  Per axis, for pixel u of an axis of n pixels and g cells:
 *     s = max(0, (u + 0.5) * (g / n) - 0.5),  i0 = min(int(s), g - 1),  i1 = min(i0 + 1, g - 1),  l = s - i0,
 *     M = (1 - ly) * ((1 - lx) * m[y0][x0] + lx * m[y0][x1]) + ly * ((1 - lx) * m[y1][x0] + lx * m[y1][x1])
 * (horizontal blend first, then vertical).  An all-ones grid gives exactly 1.0.
 * Rows: X = base + M * (x - base) in fp32 as written (three roundings), fp32 in the input's own layout ([rows,C,H,W] or [rows,1,Chans,T]:
 * they go through the model with requires_grad).  baseline_kind as in bx_rise_perturb_*: 0 one value, 1 one value per channel /
 * electrode, 2 a tensor of x's shape.
 * Objective, minimised per row, with s_c(X) the class probability (score BX_MASKOPT_PROB) or log-probability (BX_MASKOPT_LOGPROB):
 *     deletion      L = l1 mean(1 - m) + tv TV_beta(m) + s_c(X)          preservation  L = l1 mean(m) + tv TV_beta(m) - s_c(X)
 * TV_beta(m) = the sum of |d|^beta over every horizontal and vertical neighbour difference d, beta in {1, 2, 3}: |d|, |d| |d|,
 * (|d| |d|) |d|; its derivative by d is sign(d) (0 at d = 0), 2 d, (3 d) |d|.
 * Gradient, all in fp64, with g = dF_c/dX fp32 from the backward pass (F_c the output log-probability, one-hot seed: bx_expgrad_seed):
 *   1. t(p) = SUM_c (double)g[c,p] * (double)fl32(x[c,p] - base[c,p]), from 0.0 in channel order.  An EEG input with a [Chans,T] domain
 *      has one channel; under a [1,T] domain the electrodes are the channels of a column, in electrode order.
 *   2. G_data[i,j] = sign * w_r * SUM_y wy(y,i) * ( SUM_x wx(x,j) * t(y,x) ),  wx(x,j) = (j == i0 ? (double)fl32(1 - l) : 0) +
 *      (j == i1 ? (double)l : 0) (the forward's fp32 weights, widened exactly; an add of two doubles) and wy alike.  The inner sum first,
 *      from 0.0 over cell j's footprint in ascending x; then the outer one, from 0.0 over cell i's footprint in ascending y.  The
 *      footprint of cell j is every pixel whose i0 is j - 1 or j (a contiguous range; a pixel of it whose weight is 0 adds its exact
 *      zero product).  w_r = 1 for the log-probability and (double)expf(y_r[c]) for the probability, y_r the row's fp32 output: the
 *      chain rule of the probability; expf is the correctly rounded fp32 exponential, fl32(exp((double)y)).  sign = + for deletion,
 *      - for preservation.
 *   3. G = (G_data -+ l1 / (gh gw)) + tv * dTV, - for deletion and + for preservation; l1 / (gh gw) is one fp64 division;
 *      dTV[i,j] = from 0.0: + TV'(m[i][j] - m[i][j-1]) - TV'(m[i][j+1] - m[i][j]) + TV'(m[i][j] - m[i-1][j]) - TV'(m[i+1][j] - m[i][j]),
 *      each term only where the neighbour exists; the differences of the fp32 values are exact in fp64.
 *   Every product and every sum is rounded on its own (the file is built with -ffp-contract=off).
 * Adam, fp64, `it` counted from 0, c1 = 1 - b1^(it+1) and c2 = 1 - b2^(it+1) computed by the host in fp64:
 *     mu = b1 * mu + (1 - b1) * G;   nu = b2 * nu + ((1 - b2) * G) * G;
 *     m = clamp( fl32( (double)m - (lr * (mu / c1)) / (sqrt(nu / c2) + eps) ), 0, 1 ),   clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v).
 * History, recorded before the update: history[r,it] = ( s_c = (double)expf(y) or (double)y,  mean m = SUM m / (gh gw),  TV_beta(m) ).
 * The two sums over the grid run over the cells e = i gw + j in the order of bx_blurig_sum_rows: 64 partial sums over e = l, l + 64, ...
 * (ascending), added by the xor butterfly (offsets 32, 16, .., 1); cell e's TV term is, from 0.0, |m[i][j+1] - m[i][j]|^beta then
 * |m[i+1][j] - m[i][j]|^beta, each where the neighbour exists.
 * Status: a row whose y_r[c] is NaN or whose G_data holds a NaN -- every pixel lies in a footprint, so a NaN in g always does -- gets
 * BX_MASKOPT_NAN before anything of the step is written; m, the moments and the later history entries of a row whose status is not
 * BX_MASKOPT_OK are left alone by every later step.  Other rows are not affected.
 * The sums depend on the shapes alone: a thread owns its outputs and adds in ascending order, no atomics.  R = B * Kc <= 65535; every
 * offset stays below 2^31.  Limits are refused with BX_EINVAL / BX_EUNSUPPORTED before any pointer is touched.  Each entry point handles
 * the row window [row0, row0 + rows), which may begin and end inside a sample. */
enum { BX_MASKOPT_OK = 0, BX_MASKOPT_NAN = 1 };
enum { BX_MASKOPT_DELETION = 0, BX_MASKOPT_PRESERVATION = 1 };
enum { BX_MASKOPT_PROB = 0, BX_MASKOPT_LOGPROB = 1 };
/* m fp32 [R,gh,gw] = 1, mu and nu fp64 [R,gh,gw] = 0, status i32 [R] = BX_MASKOPT_OK, for the window's rows (the whole arrays are passed). */
int bx_maskopt_init(float* m, double* mu, double* nu, int* status, int B, int Kc, int gh, int gw, int row0, int rows, bxStream stream);
/* out fp32 [rows,Hm,Wm] = U(m_r) of the window's rows (for the result, plots and tests); m is the whole array.  rows * Hm * Wm < 2^31. */
int bx_maskopt_masks(const float* m, float* out, int B, int Kc, int gh, int gw, int Hm, int Wm, int row0, int rows, bxStream stream);
/* The rows of the window.  x fp32 [B,C,H,W] -> out fp32 [rows,C,H,W]; m the whole array; a kind-1 baseline holds C values. */
int bx_maskopt_rows_spec(const float* x, const float* m, const float* baseline, int baseline_kind, float* out, int B, int Kc, int C, int H, int W,
                         int gh, int gw, int row0, int rows, bxStream stream);
/* x fp32 [B,1,Chans,T] -> out fp32 [rows,1,Chans,T].  map_rows = Chans: the domain is [Chans,T]; map_rows = 1: it is [1,T] and a
 * column's value applies to every electrode.  A kind-1 baseline holds Chans values. */
int bx_maskopt_rows_eeg(const float* x, const float* m, int map_rows, const float* baseline, int baseline_kind, float* out, int B, int Kc, int Chans,
                        int T, int gh, int gw, int row0, int rows, bxStream stream);
/* One iteration for the window's rows: gradient, regularisers, Adam, clamp, history and status; the host is asked nothing.  x fp32
 * [B,C,H,W] with map_rows = 0 for a spectrogram, or [B,1,Chans,T] given as C = 1, H = Chans, W = T with map_rows = Chans or 1.  g fp32
 * [rows,C,H,W] and y fp32 [rows,K] belong to the window's rows; classes i32 [R] (the class of every row), m, mu, nu, status and history
 * fp64 [R,iterations,3] are the whole arrays.  G_out: NULL, or fp64 [R,gh,gw] that receives G of the rows that took the step.  scratch:
 * fp64 [rows,Hm,gw], the horizontal sums between the step's two launches (the first runs one workgroup per line (row, y): t of a tile of
 * the line into LDS with coalesced loads, then thread j adds cell j's footprint from there; the second runs one workgroup per row, one
 * thread per grid cell).  mode BX_MASKOPT_DELETION / _PRESERVATION,
 * score BX_MASKOPT_PROB / _LOGPROB, tv_beta 1..3; lr, l1, tv, eps >= 0; b1, b2 in [0, 1); c1, c2 in (0, 1]. */
int bx_maskopt_step(const float* x, const float* baseline, int baseline_kind, const float* g, const float* y, const int* classes, float* m, double* mu,
                    double* nu, int* status, double* history, double* G_out, double* scratch, int B, int Kc, int C, int H, int W, int map_rows, int K,
                    int gh, int gw, int mode, int score, int tv_beta, double lr, double l1, double tv, double b1, double b2, double eps, double c1,
                    double c2, int it, int iterations, int row0, int rows, bxStream stream);
/* ---- TCAV: Testing with Concept Activation Vectors (Kim et al., ICML 2018; Captum's concept.TCAV; the mean-difference "pattern" CAV of
 * Pahde et al. 2022).  a(x) in R^D is the activation of the target layer for one example, flattened in the order the capture returns
 * it (NHWC for a spectrogram target, the feature order for the EEG branch's features).  Concept sets P_1..P_Q and random sets N_1..N_R
 * of n examples each are stacked, set after set, into A [M,D], M = (Q + R) n.
 *     mean = column mean of A;   G0 = (A - 1 mean^T)(A - 1 mean^T)^T, fp64 [M,M], computed once.
 * The global centring removes the common offset of post-ReLU activations; every quantity below is a function of G0 alone.
 * A problem is a list of rows I of A (positives first, then negatives; at most 512), labels y = +1 / -1 and fit marks; the rows without a
 * fit mark are held out.  With F the nf fit rows, H = I - 11^T/nf and ybar the mean label of F:
 *     BX_TCAV_RIDGE            min (w a_i + b - y_i)^2 + lambda |w|^2 over F:  K = H G0[F,F] H,  lambda = ridge tr(K) / nf (relative, so the
 *                              scale of a layer or of bf16 storage does not matter),  (K + lambda I) alpha = H y by Cholesky,
 *                              beta = H alpha;  cond(K + lambda I) <= nf / ridge + 1 by construction
 *     BX_TCAV_MEAN_DIFFERENCE  beta_i = +1 / n+ on the positive fit rows, -1 / n- on the negative ones;  lambda = 0
 * Both have sum beta = 0, and from there one path:  w = sum_i beta_i (a_i - mean),  |w|^2 = beta^T G0[F,F] beta,  the CAV v = w / |w|
 * points towards the concept.  s_j = sum_i beta_i G0[F_i, j] for any stacked row j; the decision value of row j of I is
 * s_j - mean_F(s) + ybar (ridge) or s_j - (mean of s over the positive fit rows + mean over the negative ones) / 2 (mean difference);
 * a row is classified +1 when its decision value is > 0.
 * Status, per problem: 0 fitted; 1 tr(K) <= nf 2^-52 tr(G0[F,F]) -- no scatter inside the problem beyond the rounding of the centring
 * (ridge only); 2 |w|^2 <= nf 2^-52 (sum_i |beta_i| sqrt(G0[F_i,F_i]))^2 -- w = 0 up to the rounding of its own sum; 3 a Cholesky pivot
 * that is not above nf 2^-52 times its entry of K + lambda I (bx_shap_fit's criterion); 4 a malformed problem (a row outside 0..M-1, a
 * label other than +-1, a class without a fit row, more fit rows than nfmax).  A problem with a status writes its status and nothing
 * else.
 * Sensitivity S_k(x; v) = grad_a F_k(x) . v, F_k the output log-probability of class k; the TCAV score of (problem, class k) is the share
 * of the rows explained for class k whose S is > 0.
 * fp32 or bf16 activations and gradients (dtype as in bx_cam_reduce); no atomics; every sum is taken in an order that depends on the
 * shapes alone; the file is built with -ffp-contract=off and names its fused multiply-adds.  Limits: M <= 8192, D <= 2^24, at most 512
 * rows per problem, 65535 problems, 32 classes; beyond them BX_EUNSUPPORTED before any pointer is touched. */
enum { BX_TCAV_RIDGE = 0, BX_TCAV_MEAN_DIFFERENCE = 1 };
/* mean fp64 [D]: mean[d] = (sum_i (double)A[i,d], i ascending from 0.0) / M. */
int bx_tcav_mean(const void* A, double* mean, int M, int D, int dtype, bxStream stream);
/* G0 fp64 [M,M].  An entry is the sum over d of fma((double)A[i,d] - mean[d], (double)A[j,d] - mean[d], .): the features are cut into
 * S = ceil(D / len) splits of len = max(512, ceil(D / 32) rounded up to a multiple of 32) features, a split is summed in ascending d from
 * 0.0 by one workgroup per 64 x 64 tile of row pairs (features streamed through LDS 32 at a time), and the S partial sums, kept in the
 * workspace, are added in split order.  Only the tiles of the lower triangle are computed; (i, j) and (j, i) receive the same value,
 * so G0 is symmetric bit for bit.  Plain fp64 FMAs, not the f64 MFMA (TCAV).  workspace: 16-byte aligned. */
size_t bx_tcav_gram_workspace(int M, int D);
int bx_tcav_gram(const void* A, const double* mean, double* G0, int M, int D, int dtype, void* workspace, size_t workspace_bytes, bxStream stream);
/* P problems, one workgroup each.  rows, labels, fit i32 [P,NI] (row of A, +1 / -1, 1 = fit row / 0 = held out) and counts i32 [P] (the
 * rows of problem p are its first counts[p] entries); nfmax >= the largest number of fit rows.  workspace: P slabs of nfmax^2 doubles
 * (bx_tcav_fit_workspace), in which a problem gathers G0[F,F], centres it, adds lambda and factorises.  Outputs of a fitted problem:
 * beta fp64 [P,M] (the dual coefficients at the fit rows' columns, 0.0 elsewhere), norm fp64 [P] = |w|, lam fp64 [P], decision fp64
 * [P,NI] (its first counts[p] entries), accuracy fp64 [P,2] = the share of correctly classified fit rows and of held-out rows (NaN
 * without held-out rows); status i32 [P] is written for every problem.  ridge > 0 (ridge only). */
size_t bx_tcav_fit_workspace(int P, int nfmax);
int bx_tcav_fit(const double* G0, int M, const int* rows, const int* labels, const int* fit, const int* counts, int P, int NI, int nfmax,
                int classifier, double ridge, void* workspace, size_t workspace_bytes, double* beta, double* norm, double* lam, int* status,
                double* decision, double* accuracy, bxStream stream);
/* V fp32 [P,D]: V[p,d] = fl32( (sum_i beta[p,i] * ((double)A[i,d] - mean[d]), i ascending from 0.0, product and sum rounded one by one;
 * rows whose beta is 0.0 add nothing) / norm[p] ).  The row of a problem whose status is not 0 is left as it was. */
int bx_tcav_vectors(const void* A, const double* mean, const double* beta, const double* norm, const int* status, float* V, int M, int D, int P,
                    int dtype, bxStream stream);
/* S fp64 [rows_total,P]: S[row0 + r, p] = sum_d (double)G[r,d] * (double)V[p,d] for the rows r < rows of the gradient chunk G [rows,D]
 * (the product of two fp32 values is exact).  256 partial sums over d = t, t + 256, ... (ascending), added 16 by 16 in ascending t and
 * then in ascending group: the order depends on D alone, so no bit depends on how the rows are cut into chunks.  The other rows of S
 * are not touched. */
int bx_tcav_sensitivity(const void* G, const float* V, double* S, int rows, int D, int P, int row0, int rows_total, int dtype, bxStream stream);
/* score, mean, mean_abs fp64 [P,K] and counts i32 [K]: over the rows r (ascending) explained for class k -- classes i32 [rows], or
 * r % K when classes is NULL (every sample for every class, class fastest) -- the share with S[r,p] > 0, the mean of S[r,p] and the mean
 * of |S[r,p]|; NaN for a class without rows.  counts[k] = the number of rows of class k. */
int bx_tcav_score(const double* S, const int* classes, int rows, int P, int K, double* score, double* mean, double* mean_abs, int* counts,
                  bxStream stream);
/* ---- TracIn: training-data influence and self-influence (Pruthi et al., NeurIPS 2020; Captum's influence.TracInCPFast) through the
 * model's Linear layers -- fc2, fc1, eeg_model.dense, spectrogram_model.fc, in that order -- whose per-example gradients are outer
 * products delta (x) a, so that a gradient dot product is (delta_i . delta_j)(a_i . a_j + 1) and no per-example backward pass runs.
 * Loss of one row: KLDivLoss(reduction="sum"), l = sum_k t_k (log t_k - logp_k) with 0 log 0 = 0; t is the row's target distribution or
 * the one-hot of an integer label (then l = -logp_c).  With T = sum_k t_k, p = exp(logp), h = hidden, e / s the EEG / spectrogram
 * branch's log-probabilities, all in fp64 from the fp32 tensors of bx_mm_head_fwd:
 *     fc2                   delta_2 = T p - t                        [K]    a_2 = h                 [Hd]
 *     fc1                   delta_1 = (W2^T delta_2) (.) [h > 0]     [Hd]   a_1 = cat(e, s)         [2K]
 *                           v = W1^T delta_1                         [2K]   v_e = v[:K], v_s = v[K:]
 *     eeg_model.dense       delta_e = v_e - exp(e) sum(v_e)          [K]    a_e = the EEG features  [F]
 *     spectrogram_model.fc  delta_s = v_s - exp(s) sum(v_s)          [K]    a_s = gap_out           [C]
 * A stand-alone branch has its one layer: delta = T p - t, a = gap_out / the features.
 *     S[i,j]  = sum_c eta_c sum_l (delta_l,i . delta_l,j)(a_l,i . a_l,j + 1)        positive: a gradient step on i lowers j's loss
 *     self[i] = sum_c eta_c sum_l |delta_l,i|^2 (|a_l,i|^2 + 1)
 * Order of arithmetic (the file is built with -ffp-contract=off): every sum -- T, l, a dot product, W2^T delta_2 over the rows of W2,
 * W1^T delta_1 over the rows of W1, sum(v_e) -- is sequential in fp64 over ascending index from +0; each product is rounded once (the
 * product of two fp32 activations is exact); a layer's term is dd * (aa + 1); the terms of the selected layers are added from +0 in
 * layer order; the first checkpoint stores eta * sum, a later one adds it.  The gate [h > 0] selects +0.  exp and log are these
 * sequences of fp64 operations, Horner forms evaluated as p = p * x + c from the last coefficient:
 *     exp(x): NaN for NaN, 0 below -708, inf above 709; n = rint(x * 1.4426950408889634);
 *             r = (x - n * 0.6931471803691238) - n * 1.9082149292705877e-10;  ldexp(sum_{i=0..13} r^i / i!, n)   (1 / i! rounded to fp64)
 *     log(x): (m, q) = frexp(x), doubled with q - 1 when m < 0.7071067811865476;  f = m - 1, s = f / (2 + f), z = s * s,
 *             P = sum_{i=0..10} z^i / (2 i + 3);  q * 0.6931471803691238 + ((2 s + 2 s * (z * P)) + q * 1.9082149292705877e-10)
 * So no bit of a factor or a score depends on how the rows were cut into passes, blocks or launches.  No floating-point atomics.
 * Limits: K <= 32, Hd <= 256, a layer's delta <= 256 and activation <= 4096 wide, 1 <= M <= 4096 test rows, at most 65536 training rows
 * in a launch, N M < 2^31, 1 <= k <= 256; beyond them BX_EUNSUPPORTED (BX_EINVAL for a malformed call) before any pointer is touched. */
enum { BX_TRACIN_MULTIMODAL = 0, BX_TRACIN_SINGLE = 1 };
enum { BX_TRACIN_OK = 0, BX_TRACIN_NONFINITE = 1, BX_TRACIN_BAD_TARGET = 2 };
typedef struct {
  int layers;              /* 1..4, in the order above */
  int dwidth[4];           /* width of every layer's delta; a row of the delta array holds them side by side */
  int awidth[4];           /* width of every layer's activation */
} bxTracinShape;
typedef struct {
  const double* delta;     /* fp64 [rows, sum of dwidth] */
  const float* act[4];     /* fp32 [rows, awidth[l]]; may be NULL for a layer the mask leaves out */
  int rows;
} bxTracinSide;
/* logp, target, eeg_logp, spec_logp fp32 [rows,K]; labels i32 [rows] in place of target (exactly one of the two is given); hidden fp32
 * [rows,Hd]; w1 fp32 [Hd,2K], w2 fp32 [K,Hd].  BX_TRACIN_MULTIMODAL: delta fp64 [rows, K + Hd + K + K] = delta_2 | delta_1 | delta_e |
 * delta_s.  BX_TRACIN_SINGLE: delta fp64 [rows,K]; hidden, eeg_logp, spec_logp, w1, w2 and Hd are not read.  loss fp64 [rows].  status
 * i32 [rows]: BX_TRACIN_BAD_TARGET for a negative entry, T <= 0 or a label outside 0..K-1, else BX_TRACIN_NONFINITE for a non-finite
 * input or result, else 0; the factors and the loss of a flagged row are unspecified. */
int bx_tracin_factors(const float* logp, const float* target, const int* labels, const float* hidden, const float* eeg_logp,
                      const float* spec_logp, const float* w1, const float* w2, double* delta, double* loss, int* status, int rows, int K,
                      int Hd, int mode, bxStream stream);
/* S fp64 [N,M], M = test->rows: S[row0 + i, j] = eta * sum (store != 0) or S[row0 + i, j] + eta * sum, for the train->rows rows of the
 * block; the other rows of S are not touched.  layer_mask: bit l selects layer l.  A workgroup owns a 64 x 64 tile of pairs, both
 * sides' features stream through LDS 32 at a time and every pair's running sums stay in its thread's registers. */
int bx_tracin_scores(const bxTracinSide* train, const bxTracinSide* test, const bxTracinShape* shape, double* S, int N, int row0, double eta,
                     int store, int layer_mask, bxStream stream);
/* self fp64 [N]: self[row0 + i] = eta * sum or self[row0 + i] + eta * sum; bit-equal to the diagonal of bx_tracin_scores of the block
 * against itself.  One workgroup per row; the widths of all layers together: delta <= 352, activations <= 5440. */
int bx_tracin_self(const bxTracinSide* side, const bxTracinShape* shape, double* self, int N, int row0, double eta, int store, int layer_mask,
                   bxStream stream);
/* For every column j of S fp64 [N,M] the k rows with the largest (largest = 1) or smallest (0) values: idx i32 [M,k], val fp64 [M,k] =
 * S[idx, j], sorted by value (descending for the largest), ties by ascending row; -0.0 equals +0.0, NaN ranks last.  Exact: a radix
 * select over the 12 bytes (order-preserving 64-bit key, row) of the column, read from a transposed copy of the keys in the workspace
 * (N M 8 bytes, 8-byte aligned), then a rank sort of the k survivors.  k <= N. */
size_t bx_tracin_topk_workspace(int N, int M);
int bx_tracin_topk(const double* S, int N, int M, int k, int largest, int* idx, double* val, void* workspace, size_t workspace_bytes,
                   bxStream stream);
/* attribution seeds: seed fp32 [rows,N], row r = onehot(class of sample r % B); class_mode >= 0: that class, -1: arg-max of
 * logp fp32 [B,N] (first maximum).  Replaces the reference's output[0, argmax] indexing (XAI_Multimodality.py:3110-3111). */
int bx_class_seed(const float* logp, float* seed, int rows, int B, int N, int class_mode, bxStream stream);
/* dropout seed stream: out[0] = ++state[0] (a forward call and its backward read the same `out`). */
int bx_seed_next(uint64_t* state, uint64_t* out, bxStream stream);
/* two independent counters advanced by one launch (the two branches of the multimodal model draw one seed each per step) */
int bx_seed_next2(uint64_t* state_a, uint64_t* out_a, uint64_t* state_b, uint64_t* out_b, bxStream stream);

#ifdef __cplusplus
}
#endif
#endif /* BRAINXAI_H */
