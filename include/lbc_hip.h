/* lbc_hip.h -- C ABI of the MI355X-native LbC sensorimotor hot path.
 *
 * Plain pointers and sizes only (no torch types).  All device pointers are HBM
 * addresses on the current device; `stream` is a hipStream_t passed as void*.
 * Activations are NHWC fp32.  Convolution weights are read in the memory order
 * of a channels_last tensor with the reference's logical shapes:
 *   nn.Conv2d          (O,I,kh,kw) -> [O][kh][kw][I]
 *   nn.ConvTranspose2d (I,O,kh,kw) -> [I][kh][kw][O]
 * Every function returns 0 on success or a negative LBC_E* code; the message is
 * available from lbc_last_error().  Nothing here ever calls abort().
 *
 * The reference (dotchen/LearningByCheating) has no FFI layer: its per-step
 * arithmetic is delegated to torch.nn modules.  Each entry point below names
 * the reference call site whose arithmetic it replaces.
 */
#ifndef LBC_HIP_H
#define LBC_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* lbc_stream_t;

const char* lbc_last_error(void);
const char* lbc_backend(void);   /* "hip-gfx950" for the product library */
/* ABI version of THIS header; lbc_version() returns the one the library was built with -- a host compares the two at load time.
 * 100: rounds 1-3.  101: lbc_conv_desc grew split_workspace / split_workspace_bytes (round 4; the library still answered 100).
 * 200: lbc_conv_desc starts with struct_size, which every entry point checks (a descriptor from an older header, or one that was not
 *      initialised, is refused with LBC_EINVAL instead of being read past); lbc_adam_profile_elems.  Accepted: every struct_size from the
 *      ABI-200 layout (through split_workspace_bytes) up to the library's own sizeof -- fields appended later are optional for older hosts.
 * 201: lbc_conv_desc.bf16 = 4 / lbc_net_desc.precision = 3.  Later, without a new number: lbc_adam_state, lbc_adam_state_bytes,
 *      lbc_adam_step_guarded -- exports were only ADDED, every 201 host stays valid against this library, and a host that needs the
 *      guarded step finds out with dlsym (the Python binding fails on the missing symbol when it declares its signatures).
 *      Later again, the same way: lbc_adam_clip_state, lbc_adam_clip_state_bytes, lbc_adam_step_clipped (a new record type and
 *      new exports; lbc_adam_state and the guarded step are unchanged).  And once more: lbc_grad_accumulate (one new export, no
 *      record, nothing existing changed).  And again: lbc_adam_recipe, lbc_adam_recipe_state, lbc_adam_recipe_state_bytes,
 *      lbc_adam_step_recipe (a new descriptor, a new record type that starts with lbc_adam_clip_state's 64 bytes, new exports; the
 *      three existing steps and their records are unchanged).  And the same way: lbc_waypoint_metrics_desc,
 *      lbc_waypoint_metrics_state, lbc_waypoint_metrics_state_bytes, lbc_waypoint_metrics_update (a new descriptor, a new record
 *      type, two new exports; nothing existing changed).  And the same way: lbc_agent_desc, lbc_agent_state,
 *      lbc_agent_state_bytes, lbc_agent_control, lbc_agent_reset (a new descriptor, a new record type, three new exports; nothing
 *      existing changed).  And the same way: lbc_rollout_decide, lbc_rollout_stage_u8 (two new exports, no descriptor and no record
 *      type; nothing existing changed).  And the same way: lbc_visuals_desc, lbc_visuals_image_shape, lbc_visuals_render (a new
 *      descriptor, two new exports, no record type; nothing existing changed).
 * The size_t-returning *_workspace() queries and the int-returning *_supported() queries answer 0 for "none / no" AND for a refused
 * descriptor: a host that gets 0 checks lbc_last_error() (empty = a genuine 0), as tests/c_host/host.c does. */
#define LBC_HIP_ABI_VERSION 201
int lbc_version(void);

typedef struct lbc_conv_desc {
    unsigned struct_size;   /* = sizeof(lbc_conv_desc): start every descriptor as `lbc_conv_desc d = LBC_CONV_DESC_INIT;` -- all other
                               fields zero (no scratch, no fused ReLU, exact f32), then fill in the geometry */
    int N, H, W, C;     /* input tensor (NHWC) */
    int K;              /* output channels */
    int KH, KW, S, P;   /* filter size, stride, padding */
    int relu;           /* fuse ReLU into the epilogue */
    int bf16;           /* 0: exact f32 MFMA.  1: MFMA operands rounded to bf16 (RNE), f32 accumulate; tensors stay f32.
                           2: as 1, and the activation tensors (x, y, resid, dy, dx: the `void*` arguments) are bf16 in
                           HBM; weights, bias, statistics and weight gradients stay f32.
                           3: as 2, and `w` of the forward / input-gradient entry points is a bf16 copy of the weights in
                           the same (depth-contiguous) layout; weight gradients are still produced in f32.
                           4: split bf16 ("bf16x3"): tensors and weights f32 as in 0/1; each MFMA operand v is split into
                           hi = bf16(v), lo = bf16(v - hi) and the product is hi*hi' + hi*lo' + lo*hi' in f32 (~1e-5
                           relative instead of 1's ~1e-3).  Needs w_transposed = 1 where 1 does.  No grouped weight
                           gradient (lbc_conv2d_wgrad_group_supported answers 0); the stem entry points refuse it */
    int w_transposed;   /* lbc_conv2d_dgrad / lbc_deconv3x3s2_fwd only: `w` is the lbc_weight_transpose()d copy (depth-
                           contiguous for these GEMMs).  Required when bf16 = 1. */
    void* split_workspace;          /* optional (NULL = none): device scratch that lets lbc_conv2d_fwd / lbc_conv2d_dgrad launches with */
    size_t split_workspace_bytes;   /* few output tiles (3x3 / stride 1, bf16 = 3, small N*H*W) cut the channel contraction into ranges:
                                       f32 partial tiles here, summed in a fixed order by a second launch that does the epilogue.  A
                                       launch uses at most 8 * N*OH*OW*K * 4 bytes and ignores a scratch that is too small.  Results
                                       differ from the unsplit launch by f32 summation order only. */
} lbc_conv_desc;
#define LBC_CONV_DESC_INIT { (unsigned)sizeof(lbc_conv_desc) }

/* nn.Conv2d forward (reference bird_view/models/resnet.py:15-22,102; image.py:57).
 * y[N,OH,OW,K] = conv(x', w) (+bias) (+resid) (relu), x' = relu?(x*pre_scale+pre_shift) when
 * pre_scale != NULL (the producing BatchNorm applied on load; zero padding stays zero).
 * stats (nullable): per-workgroup partial (sum, sum^2) of y per channel, [rows][2][K];
 * *stats_rows receives the number of rows written.  Query: call with y == NULL (nothing is launched) and the SAME descriptor, resid
 * and pre_scale (NULL or not) as the real call -- they select the kernel, and the kernel sets the row count. */
int lbc_conv2d_fwd(const lbc_conv_desc* d, const void* x, const void* w, const float* bias,
                   const void* resid, const float* pre_scale, const float* pre_shift, int pre_relu,
                   void* y, float* stats, int* stats_rows, lbc_stream_t stream);

/* w[A][T][B] -> wt[B][T][A] (fp32).  Conv2d weights [K][T][C] -> [C][T][K] for lbc_conv2d_dgrad, ConvTranspose2d weights
 * [C][T][K] -> [K][T][C] for lbc_deconv3x3s2_fwd, when lbc_conv_desc.w_transposed = 1. */
int lbc_weight_transpose_f32(const float* w, float* wt, int A, int T, int B, lbc_stream_t stream);

/* Input gradient of nn.Conv2d (autograd of the call sites above; loss.backward() at
 * training/train_image_phase1.py:204).  dx[N,H,W,C] = dgrad(dy[N,OH,OW,K], w) (+resid). */
int lbc_conv2d_dgrad(const lbc_conv_desc* d, const void* dy, const void* w, const void* resid,
                     void* dx, lbc_stream_t stream);

/* Weight gradient of nn.Conv2d.  dw[K][KH][KW][C] = beta*dw + sum_m dy[m][k] * x'[gather(m)][c].
 * workspace must hold lbc_conv2d_wgrad_workspace(d) bytes. */
size_t lbc_conv2d_wgrad_workspace(const lbc_conv_desc* d);
int lbc_conv2d_wgrad(const lbc_conv_desc* d, const void* x, const void* dy,
                     const float* pre_scale, const float* pre_shift, int pre_relu,
                     float* dw, float beta, void* workspace, lbc_stream_t stream);

/* The weight gradients of n same-shaped 3x3 / stride-1 / pad-1 convolutions on bf16 tensors (d->bf16 >= 2) in ONE launch: the
 * BasicBlock convolutions of one ResNet stage (bird_view/models/resnet.py:15-22: layer1..4 hold 6 / 7 / 11 / 5 of one shape),
 * whose gradients autograd produces one by one behind loss.backward() (training/train_image_phase1.py:204).  dw[i][K][3][3][C] =
 * sum_m dy[i][m][k] * x'[i][gather(m)][c]; pre_scale / pre_shift: nullptr, or n per-channel vectors (x' = relu?(x * scale + shift)).
 * n <= 12; workspace: lbc_conv2d_wgrad_group_workspace(d, n) bytes.  lbc_conv2d_wgrad_group_supported(d): 1 when d's geometry and
 * dtype have the grouped kernel (otherwise call lbc_conv2d_wgrad per convolution). */
int lbc_conv2d_wgrad_group_supported(const lbc_conv_desc* d);
size_t lbc_conv2d_wgrad_group_workspace(const lbc_conv_desc* d, int n);
int lbc_conv2d_wgrad_group(const lbc_conv_desc* d, int n, const void* const* x, const void* const* dy,
                           const float* const* pre_scale, const float* const* pre_shift, int pre_relu,
                           float* const* dw, void* workspace, lbc_stream_t stream);

/* nn.ConvTranspose2d(C,K,3,2,1,1) forward (reference bird_view/models/image.py:39,42,45;
 * birdview.py:37,40,43).  x[N,H,W,C] -> y[N,2H,2W,K]; d->KH=KW=3, S=2, P=1 required. */
int lbc_deconv3x3s2_fwd(const lbc_conv_desc* d, const void* x, const void* w, const float* bias,
                        const float* pre_scale, const float* pre_shift, int pre_relu,
                        void* y, float* stats, int* stats_rows, lbc_stream_t stream);
int lbc_deconv3x3s2_dgrad(const lbc_conv_desc* d, const void* dy, const void* w, void* dx, lbc_stream_t stream);
size_t lbc_deconv3x3s2_wgrad_workspace(const lbc_conv_desc* d);
int lbc_deconv3x3s2_wgrad(const lbc_conv_desc* d, const void* x, const void* dy,
                          const float* pre_scale, const float* pre_shift, int pre_relu,
                          float* dw, float beta, void* workspace, lbc_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Whole-network executor: the LbC policy networks behind the reference's module API
 * (bird_view/models/image.py:22-89 ImagePolicyModelSS, birdview.py:47-79 BirdViewPolicyModelSS).
 * The executor keeps no device memory of its own: parameters/buffers are bound by pointer
 * under the reference's state_dict names, activations live in one caller-provided workspace.
 * ---------------------------------------------------------------------------------------- */
typedef struct lbc_net_desc {
    int arch;          /* 18 or 34 (BasicBlock ResNets; reference resnet.py:162-168) */
    int in_channels;   /* 3 (RGB, ImageNet-normalised on load) or 7 (bird-view) */
    int H, W;          /* input image size, multiples of 32 (160x384 / 192x192) */
    int normalize;     /* 1: (x-mean)/std with the ImageNet constants of image.py:32-35 */
    int max_batch;
    int precision;     /* 0: f32 everywhere (exact-f32 MFMA; the parity path).  1: convolution MFMA operands rounded to
                          bf16 with f32 accumulation; tensors, BatchNorm, softmax, loss, Adam and the stem stay f32.
                          2: as 1, and activations / activation gradients are stored as bf16 in the workspace (all
                          arithmetic on them stays f32; parameters, gradients, statistics, outputs stay f32).
                          3: "bf16x3": every convolution but the stem multiplies split-bf16 operands (lbc_conv_desc.bf16 = 4:
                          three bf16 MFMAs per fragment pair, f32 accumulation); tensors f32 as in 0, and the input repack, stem,
                          BatchNorm, head, loss and Adam run their exact-f32 kernels */
} lbc_net_desc;
typedef struct lbc_net lbc_net;

int lbc_net_create(const lbc_net_desc* d, lbc_net** out);
void lbc_net_destroy(lbc_net* net);
int lbc_net_num_tensors(const lbc_net* net);
/* kind: 0 = parameter (fp32), 1 = buffer fp32, 2 = buffer int64.  name = state_dict key. */
int lbc_net_tensor_info(const lbc_net* net, int i, char* name, int name_cap, int* kind, int* ndim, int* shape4);
size_t lbc_net_workspace_bytes(const lbc_net* net);
/* Introspection for parity tests: where the activations of the last training-mode forward lie in the workspace (NHWC
 * [N][H][W][C] from offset_bytes; elem_bytes 4 = f32, 2 = bf16 (precision 2), 1 = uint8).  Names follow the reference's module
 * paths: "conv.conv1" (raw stem output), "conv.maxpool", "conv.maxpool.idx" (arg-max tap 3 r + s of MaxPool2d(3,2,1), resnet.py:106),
 * "conv.layerL.B.conv1" / ".conv2" / ".downsample.0" (raw convolution outputs, resnet.py:41-49), "conv.layerL.B" (block output,
 * resnet.py:51-52), "conv.layerL.B.bn1.scale" / ".shift" ([C] f32 vectors, H = W = 1: bn1 with the batch statistics folded, so that
 * relu(bn1(.)) is positive exactly where conv1 * scale + shift > 0), "deconv.2" / ".5" / ".8" (decoder ReLU outputs, image.py:40,43,46).  A float64 checker that freezes the ReLU
 * masks and pooling choices read from here differentiates the same piecewise-linear function as lbc_net_backward. */
int lbc_net_num_activations(const lbc_net* net);
int lbc_net_activation_info(const lbc_net* net, int i, char* name, int name_cap, size_t* offset_bytes, int* hwc3, int* elem_bytes);
/* tensor_ptrs[i] / grad_ptrs[i] in lbc_net_tensor_info order; grad_ptrs may be NULL (inference only)
 * and its entries for buffers are ignored.  4-D weights must be in channels_last memory order. */
int lbc_net_bind(lbc_net* net, void* workspace, void* const* tensor_ptrs, float* const* grad_ptrs);
/* forward(image, velocity, command) of the reference modules.  image: NCHW fp32 [N,C,H,W] (the
 * reference signature); velocity [N]; command [N,4] one-hot.  Outputs: pred_sel [N,5,2] and
 * pred_all [N,4,5,2] (normalised [-1,1] camera/map coordinates).  train != 0: batch statistics,
 * running-stat update, activations kept for backward. */
int lbc_net_forward(lbc_net* net, int N, int train, const float* image, const float* velocity,
                    const float* command, float* pred_sel, float* pred_all, lbc_stream_t stream);
/* Same with the frames as the dataset stores them: uint8 NHWC [N,H,W,C], 0..255 (reference
 * bird_view/utils/datasets/image_lmdb.py:128-222 converts them to f32 CHW /255 on the host: 4x the H2D and input bytes).
 * /255, the ImageNet normalisation and the NHWC repack are fused into the stem's input pass. */
int lbc_net_forward_u8(lbc_net* net, int N, int train, const unsigned char* image_nhwc, const float* velocity,
                       const float* command, float* pred_sel, float* pred_all, lbc_stream_t stream);
/* Backward of the last training-mode forward: gradients of a scalar wrt pred_sel / pred_all
 * (either may be NULL) -> every bound parameter gradient (overwritten, not accumulated).
 * stage = -1 runs everything; stages 0..lbc_net_num_stages()-1 run in order (head+decoder,
 * layer4, layer3, layer2, layer1, stem) so gradient buckets can be all-reduced while the
 * remaining stages execute.  The residual blocks' weight gradients run on an internal side stream next to their input
 * gradients; every stage joins it before returning control of `stream` (LBC_NO_SIDE_STREAM=1 keeps everything on `stream`). */
int lbc_net_num_stages(void);
/* State lbc_net_backward() would differentiate: batch size and mode of the last forward, and a counter that every forward
 * increments -- a caller that holds several forward results (autograd) can detect that the workspace has moved on. */
int lbc_net_last_forward(const lbc_net* net, int* batch, int* train, long long* generation);
/* frozen = 1: the caller promises not to change parameters or buffers until it says otherwise (the frozen privileged teacher of
 * reference training/train_image_phase1.py:244-248, phase2_utils.py:70-77).  Eval-mode forwards then derive what they derive from
 * the weights alone -- the bf16 weight copies (precision 2) and every BatchNorm's folded affine -- on the first forward only instead of
 * on every one.  frozen = 0 (default) or any lbc_net_bind: derived again on the next forward. */
int lbc_net_set_frozen(lbc_net* net, int frozen);
int lbc_net_backward(lbc_net* net, const float* d_sel, const float* d_all, int stage, lbc_stream_t stream);
/* Synchronized BatchNorm for data-parallel training (not in the reference, which is single-device; the equivalent of wrapping
 * its modules in torch.nn.SyncBatchNorm): every BatchNorm of a training-mode forward normalises with the statistics of the
 * GLOBAL batch, and its backward uses the global gradient sums -- a per-GPU batch of 32 then trains like the 256-image batch
 * of BASELINE.json instead of eight 32-image batches.  Before each finalize the net reduces that layer's per-channel sums to
 * one row of `count` floats in `buf` and calls fn(ctx, buf, count, stream), which must enqueue an in-place SUM all-reduce
 * over the data-parallel group on `stream` (ncclAllReduce of RCCL takes exactly these arguments) and return 0, or non-zero
 * to abort the step (LBC_ELAUNCH).  dgamma / dbeta stay local sums, as every other parameter gradient: the caller's gradient
 * all-reduce completes them.  buf: device memory, buf_floats >= 1536.  fn == NULL switches back to local statistics.
 * Eval-mode forwards never call fn. */
typedef int (*lbc_allreduce_fn)(void* ctx, float* buf, int count, lbc_stream_t stream);
int lbc_net_set_sync_bn(lbc_net* net, lbc_allreduce_fn fn, void* ctx, int world_size, float* buf, int buf_floats);
/* The RCCL communicator that callback normally is (csrc/comm.cpp): one per process/GPU, built from an id that rank 0 creates and
 * the host distributes over whatever channel it has (torch.distributed broadcast, MPI, a file).  lbc_comm_create is collective
 * over the world and binds the calling thread's current HIP device.  lbc_comm_allreduce_f32 is an lbc_allreduce_fn with
 * ctx = the lbc_comm: ncclAllReduce(buf, buf, count, ncclFloat32, ncclSum) enqueued on `stream`, nothing else.
 * RCCL is bound at run time (the librccl.so already in the process, else the system one): without it these return
 * LBC_EINVAL with the reason in lbc_last_error(), the rest of the library is unaffected. */
#define LBC_COMM_ID_BYTES 128
typedef struct lbc_comm lbc_comm;
int lbc_comm_unique_id(unsigned char* id /* [LBC_COMM_ID_BYTES] */);
int lbc_comm_create(const unsigned char* id, int rank, int world_size, lbc_comm** out);
void lbc_comm_destroy(lbc_comm* comm);
int lbc_comm_world_size(const lbc_comm* comm);
int lbc_comm_allreduce_f32(void* comm, float* buf, int count, lbc_stream_t stream);

/* Losses (forward value per sample + gradient wrt pred), reference training/train_image_phase1.py:35-70,
 * train_image_phase0.py:36-89, train_birdview.py:33-54.  kind: 0 phase-0, 1 phase-1, 2 bird-view L1 (pixel targets), 3 L1 vs normalised targets.
 * rows = waypoints per sample (5 or 20).  dpred = grad_scale * d(sum_n loss[n])/dpred. */
typedef struct lbc_camera { float w, h, fov, world_y, fixed_offset, pixels_per_meter, crop_size; } lbc_camera;
int lbc_loss(int kind, const lbc_camera* cam, const float* pred, const float* target, int N, int rows,
             float grad_scale, float* loss_per_sample, float* dpred, lbc_stream_t stream);

/* Phase-2 (DAgger) resampling weight per sample: reference training/phase2_utils.py:50-59 (get_weight) on the selected
 * branch, applied as in train_image_phase2.py:203-206.  pred_sel [N,5,2] camera space, teacher_sel [N,5,2] map space. */
int lbc_phase2_weight(const lbc_camera* cam, const float* pred_sel, const float* teacher_sel, int N, float* weights,
                      lbc_stream_t stream);

/* Multi-tensor Adam (torch.optim.Adam semantics; reference training/train_image_phase1.py:252).
 * chunk table lives in device memory: see lbc_adam_chunk. */
typedef struct lbc_adam_chunk { float* p; const float* g; float* m; float* v; int n; int pad; } lbc_adam_chunk;
int lbc_adam_step(const lbc_adam_chunk* chunks_dev, int nchunks, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int step, lbc_stream_t stream);

/* Guarded Adam: the same update behind a scan of the gradients for NaN / +-Inf, decided on the device -- a step whose
 * gradients hold one non-finite element is skipped as a whole (p, m, v and the step count keep their bits) without the host
 * ever looking.  The reference has no such guard: its phase-1 / phase-2 loss unprojects with 1 / y
 * (training/train_image_phase1.py:43-64), and a waypoint on the horizon row turns every parameter into NaN.
 * The step count lives in a device record owned by the caller: lbc_adam_state_bytes() bytes of device memory, 8-byte aligned,
 * ZERO-filled once before the first call (a fresh optimizer), never written by the host while steps are in flight; to resume,
 * upload a record whose `step` (and counters) carry the saved values and whose other fields are zero.  Counters are 64-bit.
 * One call enqueues, in order: the scan (reads g once, raises scan_flag), one bookkeeping thread (bad = scan_flag, scan_flag = 0;
 * clean: step += 1, skipped_in_a_row = 0, coefficients of the new step computed in double; bad: skipped_total += 1,
 * skipped_in_a_row += 1), and the update (returns at once when bad != 0).  No device-to-host copy, no synchronisation: read the
 * record back (hipMemcpy after a stream synchronise) only where the host syncs anyway -- logging, checkpoints.
 * Under data parallelism call it after the gradient all-reduce: NaN / Inf survive a sum, the reduced bytes are the same on
 * every rank, so every rank takes the same decision. */
typedef struct lbc_adam_state {
    long long step;              /* number of APPLIED updates (torch.optim.Adam's state["step"]) */
    long long skipped_total;     /* steps skipped since the record was zeroed */
    long long skipped_in_a_row;  /* ... since the last applied step */
    int bad;                     /* decision of the last call: 1 = skipped */
    int scan_flag;               /* scratch of the scan; zero between calls */
    float lr_over_bc1;           /* lr / (1 - beta1^step)       of the last applied step */
    float inv_bc2_sqrt;          /* 1 / sqrt(1 - beta2^step) */
} lbc_adam_state;
size_t lbc_adam_state_bytes(void);
int lbc_adam_step_guarded(const lbc_adam_chunk* chunks_dev, int nchunks, double lr, double beta1, double beta2,
                          double eps, double weight_decay, lbc_adam_state* state_dev, lbc_stream_t stream);

/* Guarded Adam with gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, which the reference does not call): the
 * pass that looks for NaN / +-Inf also sums the squares of the gradients, so the global L2 norm, the clipping coefficient and
 * the skip decision are all taken on the device, again without a device-to-host copy or a synchronisation.
 * The record is lbc_adam_clip_state_bytes(nchunks) bytes of device memory owned by the caller: the header below followed by one
 * double per chunk (the chunks' partial sums of squares, scratch).  Same contract as the guarded step: ZERO-filled once, 8-byte
 * aligned, never written by the host while steps are in flight; to resume, upload a header that carries the saved counters
 * (step, skipped_*, clipped_total) and zeros elsewhere.
 * One call enqueues, in order: the norm pass (reads exactly the n elements of every chunk once; per chunk a sum of exact f64
 * squares, combined in a fixed order -- no atomics, so the same gradients give the same 8 bytes of grad_norm on every run and
 * every rank), one bookkeeping workgroup (adds the partials in a fixed order, then the bookkeeping of the guarded step; on a
 * clean step grad_norm = sqrt(sum) and
 *     clip_coef = (max_norm > 0 && max_norm / (grad_norm + 1e-6) < 1) ? (float)(max_norm / (grad_norm + 1e-6)) : 1.0f,
 * clipped_total += clip_coef < 1; on a skipped step all three keep the values of the last clean step), and the update: the
 * guarded update on g * clip_coef, the product rounded to f32 on its own.  With clip_coef == 1 the step is bit for bit
 * lbc_adam_step_guarded; with clip_coef < 1 it is lbc_adam_step_guarded on gradients multiplied by that float.
 * THE GRADIENT BUFFER IS NOT WRITTEN: g keeps the unclipped values (clipping costs no store of the gradients).
 * max_norm <= 0 measures the norm without clipping; a NaN max_norm is refused.  Under data parallelism call it after the
 * gradient all-reduce: every rank derives the same coefficient from the same bytes. */
typedef struct lbc_adam_clip_state {
    long long step;              /* the fields of lbc_adam_state, same meaning and offsets */
    long long skipped_total;
    long long skipped_in_a_row;
    int bad;
    int scan_flag;
    float lr_over_bc1;
    float inv_bc2_sqrt;
    double grad_norm;            /* global L2 norm of the gradients of the last clean step (before clipping) */
    float clip_coef;             /* what the last clean step multiplied its gradients by; 1 = not clipped */
    int reserved;                /* zero */
    long long clipped_total;     /* applied steps with clip_coef < 1 since the record was zeroed */
} lbc_adam_clip_state;
size_t lbc_adam_clip_state_bytes(int nchunks);
int lbc_adam_step_clipped(const lbc_adam_chunk* chunks_dev, int nchunks, double lr, double beta1, double beta2,
                          double eps, double weight_decay, double max_norm, lbc_adam_clip_state* state_dev, lbc_stream_t stream);

/* The training recipe on top of the clipped step: a learning-rate schedule evaluated on the device from the record's own step
 * count, decoupled weight decay (torch.optim.AdamW) and an exponential moving average of the parameters, in one step of three
 * launches like lbc_adam_step_clipped (norm pass, one bookkeeping launch, one update launch), again without a device-to-host
 * copy or a synchronisation.  The reference trains with a constant rate, no decay and no average.
 * The recipe is a host struct, read during the call only.  Start it as `lbc_adam_recipe r = LBC_ADAM_RECIPE_INIT;` -- struct_size is
 * checked like lbc_conv_desc's.  On a clean step the bookkeeping thread computes, in double, from k = step - 1 (the number of
 * updates applied before this one; a skipped step does not advance it):
 *     k < warmup_steps:   lr = base_lr * (warmup_start + (1 - warmup_start) * k / warmup_steps)
 *     else, j = k - warmup_steps:
 *       LBC_LR_CONSTANT   lr = base_lr
 *       LBC_LR_COSINE     lr = min_lr + (base_lr - min_lr) * 0.5 * (1 + cos(pi * min(j, T - W) / (T - W))),  T = total_steps, W = warmup_steps
 *       LBC_LR_STEP       lr = base_lr * gamma^floor(j / step_size)
 * lr_over_bc1 = (float)(lr / (1 - beta1^step)); decay_factor = decoupled ? (float)(1 - lr * weight_decay) : 1; ema_updates += 1 when
 * ema_decay > 0.  A skipped step keeps lr, decay_factor and ema_updates, as it keeps grad_norm.
 * The update is that of lbc_adam_step_clipped (same roundings: a recipe with a constant rate, no warm-up, coupled decay and no
 * average IS that step, bit for bit) with two additions.  decoupled != 0: p is first multiplied by decay_factor, the product rounded
 * to f32 on its own, and the coupled term is dropped.  ema_decay > 0: e = e + (float)(1 - ema_decay) * (p' - e) on the updated p'.
 * ema_dev is a device array of one float* per chunk: the chunk's slice of the shadow, in the element order and padding of m and v
 * (16-byte aligned like them); NULL when ema_decay == 0.  A skipped step returns before it loads anything: e keeps its bits too.
 * The record is lbc_adam_recipe_state_bytes(nchunks) bytes: the header below and one double per chunk; the contract of
 * lbc_adam_clip_state (zero-filled once, 8-byte aligned, counters uploaded to resume -- ema_updates with them).
 * Refused with LBC_EINVAL: a null recipe / state / table, a bad struct_size, a misaligned state, nchunks <= 0, an unknown schedule,
 * any NaN, base_lr < 0, warmup_steps < 0, warmup_start outside [0, 1], cosine with total_steps <= warmup_steps, step with
 * step_size < 1 or gamma <= 0, ema_decay outside [0, 1), ema_decay > 0 with ema_dev NULL, decoupled with weight_decay < 0. */
enum { LBC_LR_CONSTANT = 0, LBC_LR_COSINE = 1, LBC_LR_STEP = 2 };
typedef struct lbc_adam_recipe {
    unsigned struct_size;        /* = sizeof(lbc_adam_recipe) */
    int schedule;                /* LBC_LR_* */
    double base_lr;
    long long warmup_steps;      /* W: optimizer steps of linear warm-up; 0 = none */
    double warmup_start;         /* s0: the first step's fraction of base_lr */
    long long total_steps;       /* T (cosine): the rate reaches min_lr at step T and stays there */
    double min_lr;               /* (cosine) */
    long long step_size;         /* S (step) */
    double gamma;                /* (step) */
    double weight_decay;
    int decoupled;               /* 0: the coupled L2 term of lbc_adam_step; 1: AdamW */
    int reserved;                /* zero */
    double max_norm;             /* as lbc_adam_step_clipped: <= 0 measures the norm without clipping */
    double ema_decay;            /* 0 = no average; else in (0, 1) */
    double beta1, beta2, eps;
} lbc_adam_recipe;
#define LBC_ADAM_RECIPE_INIT { (unsigned)sizeof(lbc_adam_recipe), 0, 0.0, 0, 0.0, 0, 0.0, 1, 1.0, 0.0, 0, 0, 0.0, 0.0, 0.9, 0.999, 1e-8 }
typedef struct lbc_adam_recipe_state {
    long long step;              /* the 64 bytes of lbc_adam_clip_state, same meaning and offsets */
    long long skipped_total;
    long long skipped_in_a_row;
    int bad;
    int scan_flag;
    float lr_over_bc1;
    float inv_bc2_sqrt;
    double grad_norm;
    float clip_coef;
    int reserved;
    long long clipped_total;
    double lr;                   /* the schedule's rate of the last clean step */
    float decay_factor;          /* what that step multiplied p by in front of the update; 1 without decoupled decay */
    int reserved2;               /* zero */
    long long ema_updates;       /* applied steps that moved the average since the record was zeroed */
} lbc_adam_recipe_state;
size_t lbc_adam_recipe_state_bytes(int nchunks);
int lbc_adam_step_recipe(const lbc_adam_chunk* chunks_dev, int nchunks, const lbc_adam_recipe* recipe, float* const* ema_dev,
                         lbc_adam_recipe_state* state_dev, lbc_stream_t stream);

/* Gradient accumulation over micro-batches (what the reference would get from calling loss.backward() K times before
 * optimizer.step(); it never does): lbc_net_backward overwrites the bound gradients, so a caller that wants the sum of K backward
 * passes adds each one (or each stage's range of it, right behind that stage) into a buffer of its own, and points the optimizer's
 * chunk table and the gradient all-reduce at that buffer.
 * acc[i] = first ? g[i] : acc[i] + g[i], i < n.  first != 0 never READS acc (a NaN left there by a skipped window cannot survive).
 * g, acc: device f32, 16-byte aligned (LBC_EINVAL otherwise, nothing launched); the two ranges must NOT overlap (g == acc included:
 * the kernel reads and writes through restrict-qualified pointers); n >= 0, n == 0 launches nothing.  One f32 add per
 * element in call order: no atomics, no reassociation -- the same inputs give the same bits on every run and every rank. */
int lbc_grad_accumulate(const float* g, float* acc, long long n, int first, lbc_stream_t stream);

/* Waypoint error metrics in metres, accumulated on the device (csrc/metrics.hip).  Not in the reference, which logs only the
 * loss: displacement error of the COMMANDED branch's waypoints against the teacher (or the ground truth), per command and per
 * horizon step, split into a lateral (map x) and a longitudinal (map y) part, with the share of waypoints inside given tolerances.
 * One launch per batch adds that batch into the record below; nothing is read back until the host wants the numbers.
 * Call sequence: hipMemset the record to zero once (all-zero bytes are the empty record), lbc_waypoint_metrics_update per batch
 * on the stream of the loss, copy lbc_waypoint_metrics_state_bytes() bytes back where the host synchronises anyway.
 * Per sample n: c = the index of the first non-zero entry of command_onehot[n] (none: the sample counts in `samples`, in the
 * all-branch fields and in the loss, and in no commanded cell).  Per horizon step t < 5, in DOUBLE from the f32 inputs:
 *   prediction, pred_frame 0 (camera frame, the image models): the unprojection of lbc_loss kind 1 --
 *     xt = ((x + 1) w / 2 - w / 2) / f, yt = ((y + 1) h / 2 - h / 2) / f, f = w / (2 tan(fov pi / 360)) (computed on the host),
 *     z = world_y / yt, px = z xt pixels_per_meter + crop_size / 2, py = crop_size - z pixels_per_meter + fixed_offset pixels_per_meter;
 *   prediction, pred_frame 1 (map frame, the bird-view model): p = (v + 1) crop_size / 2;
 *   target: q = (target * target_scale + target_shift + 1) crop_size / 2 (a normalised map coordinate after scale and shift);
 *   dx = (px - qx) / pixels_per_meter, dy = (py - qy) / pixels_per_meter, e = sqrt(dx^2 + dy^2)   [metres].
 * A row whose e is not finite (a prediction on the horizon row, yt = 0; a NaN or an infinity anywhere) counts in `bad` and in
 * nothing else; cmd_count[c] - bad[c][t] is therefore the number of rows behind the sums of cell [c][t].
 * rows = 20: pred / target are (N,4,5,2), the commanded rows are picked out of them and the all_* fields see every branch;
 * rows = 5: pred / target are (N,5,2), the all_* fields are not touched.  loss (may be NULL: loss_* untouched): N per-sample values.
 * One workgroup, no atomics, no workspace, every sum in a fixed order: a sequence of calls gives the same bits on every run.
 * Reads stay inside pred / target / command_onehot / loss, writes inside the record.  N == 0 launches nothing.
 * Refused with LBC_EINVAL (nothing launched, the record untouched): a null or non-8-byte-aligned state, null pred / target /
 * command_onehot, N < 0, rows not 5 or 20, pred_frame not 0 or 1, nthresholds outside 0..4, a negative or non-finite threshold,
 * a struct_size other than sizeof(lbc_waypoint_metrics_desc) (start it as `lbc_waypoint_metrics_desc d = LBC_WAYPOINT_METRICS_DESC_INIT;`). */
typedef struct lbc_waypoint_metrics_desc {
    unsigned struct_size;        /* = sizeof(lbc_waypoint_metrics_desc) */
    int pred_frame;              /* 0: camera frame (unprojected), 1: map frame */
    int rows;                    /* 5 or 20 */
    int nthresholds;             /* 0..4 */
    double target_scale, target_shift;
    double thresholds_m[4];      /* metres; within[k] counts finite rows with e <= thresholds_m[k] */
    lbc_camera camera;
    int reserved;                /* zero */
} lbc_waypoint_metrics_desc;
#define LBC_WAYPOINT_METRICS_DESC_INIT { (unsigned)sizeof(lbc_waypoint_metrics_desc), 0, 5, 0, 1.0, 0.0, { 0.0, 0.0, 0.0, 0.0 }, \
                                         { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, 0 }
typedef struct lbc_waypoint_metrics_state {      /* 248 fields of 8 bytes; [c] command, [t] horizon step, [b] branch, [k] threshold */
    long long samples;           /* samples seen */
    long long updates;           /* launches (calls with N > 0) */
    long long cmd_count[4];      /* samples per command */
    double sum_e[4][5];          /* commanded branch, finite rows: sum of e */
    double sum_e2[4][5];         /*   ... of e^2 */
    double sum_abs_dx[4][5];     /*   ... of |dx| (lateral) */
    double sum_abs_dy[4][5];     /*   ... of |dy| (longitudinal) */
    double max_e[4][5];          /*   ... the largest e */
    long long bad[4][5];         /* commanded rows whose e is not finite */
    long long within[4][4][5];   /* [k][c][t]: finite rows with e <= thresholds_m[k]; k >= nthresholds untouched */
    double all_sum_e[4][5];      /* rows = 20 only, every sample for branch b: sum of e over finite rows */
    long long all_bad[4][5];     /*   ... rows whose e is not finite */
    double loss_sum;             /* sum of the finite per-sample losses */
    long long loss_bad;          /* per-sample losses that are not finite */
} lbc_waypoint_metrics_state;
size_t lbc_waypoint_metrics_state_bytes(void);
int lbc_waypoint_metrics_update(const lbc_waypoint_metrics_desc* desc, const float* pred, const float* target, const float* command_onehot,
                                const float* loss /* may be NULL */, int N, void* state, lbc_stream_t stream);

/* Training visuals on the device (csrc/visuals.hip): the grid of waypoint panels the reference's _log_visuals draws on the host
 * (training/train_image_phase0.py:91-147, train_image_phase1.py:72-128, train_birdview.py:57-99), rendered by ONE launch into a uint8
 * image [rows][cols][3] in device memory, from the tensors the loss launch has just read.  Nothing is read back by the library.
 * mode 0: phase 0; 1: phases 1 and 2; 2: bird-view.  pred / teacher_or_target are [N][5][2] f32 (modes 0, 2) or [N][4][5][2] (mode 1,
 * where the branch c = the first non-zero entry of command_onehot[n] is drawn, and no dot at all when the row is all zero).
 * Panel: modes 0 and 1, BH rows x (W + BW) columns -- the camera frame at rows (BH - H) / 2 .. + H - 1, columns 0 .. W - 1, black above
 *   and below it, the map canvas (BH x BW) at columns W .. W + BW - 1; mode 2, the canvas alone.  Nothing is resampled (the reference
 *   shrinks the canvas to the frame's height with cv2.resize).
 * Canvas: (0, 47, 0); then for channel i = 0..6 a pixel whose bird-view channel i is > 0 takes the reference's COLORS[i] (the highest set
 *   channel wins).  birdview is [N][BH][BW][7] u8 or, birdview_f32 != 0, [N][7][BH][BW] f32; NULL (modes 0 and 1): background only.
 * Frame: rgb [N][H][W][3] u8 as it is, or, rgb_f32 != 0, [N][3][H][W] f32 in [0, 1] as (uint8)(x * 255.0f) (f32 product, truncated).
 * Dots: 5 x 5 squares, rows int(y) - 2 .. int(y) + 2, columns int(x) - 2 .. int(x) + 2 (int truncates toward zero), clipped to their
 *   canvas or frame; a dot with a coordinate that is not finite or has |v| >= 2^30 is not drawn; a later dot covers an earlier one.
 *   All coordinates in DOUBLE from the f32 inputs, with f = w / (2 tan(fov pi / 360)) computed on the host:
 *   canvas, modes 0 and 1: teacher BLUE (0, 0, 255) at (t + 1) crop_size / 2; then, mode 1, the student RED (255, 0, 0) unprojected as
 *     under lbc_waypoint_metrics_update, pred_frame 0.
 *   frame, mode 0: teacher BLUE projected -- (px, py) = (t + 1) crop_size / 2, X = (px - crop_size / 2) / pixels_per_meter,
 *     Z = (crop_size - py) / pixels_per_meter + fixed_offset, u = f X / Z + w / 2, v = f world_y / Z + h / 2, clipped to [0, w] x [0, h]
 *     (a NaN stays a NaN); then, modes 0 and 1, the student RED at ((x + 1) w / 2, (y + 1) h / 2).
 *   canvas, mode 2: the ground truth BLUE at its pixel coordinates, then the prediction RED at (p + 1) crop_size / 2.
 *   (The reference's white marker at (0, 0) is an empty slice there and is left out.)
 * Text: white, on the canvas, over the dots: "Command: LEFT|RIGHT|STRAIGHT|FOLLOW" ("???" for an all-zero row) and "Loss: " + the
 *   per-sample loss as '%.2f' prints it (c = rint(v 100) in double, which is exact for an f32 v; "nan", "inf", "-inf").  Glyphs 5 x 7 from
 *   `font` (95 x 7 bytes, ASCII 32..126, bit 4 of a row byte = the left column), advance 6; line k = 1, 2 occupies canvas rows
 *   19 k - 6 .. 19 k from canvas column 0 and is cut at the canvas edge.
 * Selection: the candidates are samples 0 .. min(N, size) - 1.  sort != 0: panel slot k shows the candidate of rank k by loss,
 *   descending, ties by lower index first, a NaN before everything; sort == 0: slot k is sample k.
 * Grid: ncols panels per row, 2 black pixels around and between panels, unused slots of the last row black; rows = 2 +
 *   ceil(min(N, size) / ncols) (BH + 2), cols = 2 + ncols (panel columns + 2).  EVERY byte of the image is written by every launch,
 *   each exactly once: no atomics, and the same inputs give the same bytes.  No min / max normalisation (make_grid's normalize=True).
 * Refused with LBC_EINVAL (nothing launched, nothing written): a struct_size other than sizeof(lbc_visuals_desc) (start it as
 *   `lbc_visuals_desc d = LBC_VISUALS_DESC_INIT;`), an unknown mode, size outside 1..32, ncols < 1, N < 1, BH / BW / W outside 1..16384,
 *   H outside 1..BH (modes 0, 1), an image of 2^29 pixels or more, a NULL rgb (modes 0, 1), pred, teacher_or_target, command_onehot, loss,
 *   font or out, a NULL birdview in mode 2, an out that is not 4-byte aligned. */
typedef struct lbc_visuals_desc {
    unsigned struct_size;        /* = sizeof(lbc_visuals_desc) */
    lbc_camera camera;
    int mode;                    /* 0, 1, 2 */
    int size;                    /* panels at most: 1..32 */
    int sort;                    /* != 0: by loss, descending */
    int ncols;                   /* panels per grid row */
    int N;                       /* samples in the batch */
    int H, W;                    /* camera frame (modes 0, 1) */
    int BH, BW;                  /* map canvas */
    int rgb_f32, birdview_f32;   /* != 0: that tensor is f32 NCHW instead of u8 NHWC */
} lbc_visuals_desc;
#define LBC_VISUALS_DESC_INIT { (unsigned)sizeof(lbc_visuals_desc), { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, 0, 8, 0, 4, 0, 0, 0, 0, 0, 0, 0 }
int lbc_visuals_image_shape(const lbc_visuals_desc* desc, int* rows, int* cols);
int lbc_visuals_render(const lbc_visuals_desc* desc, const void* rgb, const void* birdview /* may be NULL */, const float* pred,
                       const float* teacher_or_target, const float* command_onehot, const float* loss, const unsigned char* font,
                       unsigned char* out, lbc_stream_t stream);

/* The agent half of the tick on the device (csrc/agent.hip): waypoints -> steer / throttle / brake for N independent agents in one
 * launch, the controller state kept in device memory.  Restates the arithmetic of the reference's two agents and their controllers
 * (bird_view/models/image.py:124-219 ImageAgent.run_step + unproject, birdview.py:104-174 BirdViewAgent.run_step, controller.py
 * ls_circle / PIDController / CustomController, common.py:38-51 signed_angle / project_point_to_circle, agent.py postprocess).
 * Call sequence: hipMemset lbc_agent_state_bytes(N) bytes to zero once (all-zero bytes are N fresh agents), one lbc_agent_control
 * per tick on the stream of lbc_net_forward_u8 with its pred_sel, lbc_agent_reset at every episode start.  Nothing is read back by
 * the library; the host copies the N x 8 doubles of `out` when it wants the controls.
 * One thread per agent, all arithmetic in DOUBLE, no atomics: the same inputs and state give the same bits on every run.
 * Per active agent i, with (x_k, y_k) = pred[i][k], k < 5, and c = the commanded branch of command_onehot[i] (0..3):
 *   LBC_AGENT_IMAGE:  a_k = (double)(float)(x_k + 1) * w / 2, b_k = (double)(float)(y_k + 1) * h / 2 (the sum rounded to f32, as the
 *     reference's f32 array + 1 is), f = w / (2 tan(fov pi / 360)) (computed on the host), xt = (a_k - w / 2) / f, yt = (b_k - h / 2) / f,
 *     z = world_y / yt, targets[k + 1] = (forward, lateral) = (z - fixed_offset, z xt);
 *     target_speed = the mean length of the 5 segments of targets[0..5] / (gap dt).
 *   LBC_AGENT_BIRDVIEW:  (a_k, b_k) = (double)(float)((v + 1) / 2 * crop_size), every step in f32 as the reference's f32 array,
 *     targets[k + 1] = ((crop_size - b_k) / pixels_per_meter, (a_k - crop_size / 2) / pixels_per_meter);
 *     target_speed = sum_{k = 1 .. speed_steps - 1} |(a_k, b_k) - (a_{k-1}, b_{k-1})| / (pixels_per_meter gap dt) / (speed_steps - 1).
 *   Both: targets[0] = (0, 0).  Least-squares circle through the six targets (u, v = coordinates minus their means; Suu, Suv, Svv,
 *     Suuu, Suvv, Svvv, Svuu their moment sums; the centre solves [[Suu, Suv], [Suv, Svv]] (cx, cy) = ((Suuu + Suvv) / 2, (Svvv + Svuu) / 2)
 *     by Cramer's rule with det = Suu Svv - Suv^2; r = sqrt(cx^2 + cy^2 + (Suu + Svv) / 6); the means are added back).
 *     The aim point is targets[steer_points[c]] projected onto the circle, centre + (p - centre) / |p - centre| r, and
 *     alpha = atan2(aim_y, aim_x), the signed angle of the aim point against the forward axis.
 *     Steering: alpha enters a window of the last turn_window values; steer = Kp alpha + Kd de + Ki ie with (Kp, Ki, Kd) = turn_pid[c],
 *     de = (newest - the one before) / dt, ie = (sum of the window, oldest first) dt, both 0 while the window holds fewer than two values.
 *     Speed: e = target_speed - speed[i] enters a window of the last speed_window values; throttle = Kp e + Ki ie + Kd de the same way
 *     with speed_pid.  BOTH windows advance on every active tick, braking ticks included.  (The reference's controllers carry
 *     their own 0.1 s next to the agents' DT = 0.1; here all three are `dt`.)
 *     IMAGE: target_speed <= engine_brake_threshold -> steer = throttle = 0; target_speed <= brake_threshold -> brake = 1.
 *     BIRDVIEW: target_speed < stop_threshold -> steer = throttle = 0, brake = 1.
 *   out[i] = { clip(steer, -1, 1), clip(throttle, 0, 1), clip(brake, 0, 1), target_speed, aim_x, aim_y, alpha, flags }.
 * Cases the reference leaves undefined (it raises, or divides by zero), decided here; `flags` is a double holding the sum of
 *   LBC_AGENT_FLAG_DEGENERATE (1): |det| <= 1e-12 Suu Svv (collinear targets -- a car driving dead straight; Suu Svv == 0 included),
 *     or the steer point lies on the centre: the aim point is targets[steer_points[c]] itself, the limit of the projection as the
 *     radius grows.  Everything else proceeds normally.
 *   LBC_AGENT_FLAG_BAD (2): a waypoint that is not finite; IMAGE: a waypoint on or above the horizon row (yt <= 0); a command row
 *     that is not one-hot (exactly one entry equal to 1, the others 0): out[i] = { 0, 0, 1, 0, 0, 0, 0, 2 } and the windows are NOT touched.
 *   LBC_AGENT_FLAG_INACTIVE (4): active != NULL and active[i] == 0: the state is not touched, out[i] = { 0, 0, 0, 0, 0, 0, 0, 4 }.
 * A speed[i] that is not finite is not a bad waypoint: it travels through the speed controller like any other number.
 * Reads: pred [N][5][2], speed [N], command_onehot [N][4], active [N] (nullable), the N records.  Writes: out [N][8] and the records of
 * active agents with a good waypoint.  N == 0 launches nothing.
 * lbc_agent_reset: the records of the agents with mask[i] != 0 (mask == NULL: all N) become all-zero bytes, on `stream`.
 * Refused with LBC_EINVAL (nothing launched, nothing written): a null or non-8-byte-aligned state or out, null pred / speed /
 * command_onehot, N < 0, a struct_size other than sizeof(lbc_agent_desc) (start it as `lbc_agent_desc d = LBC_AGENT_DESC_IMAGE_INIT;`
 * or `... = LBC_AGENT_DESC_BIRDVIEW_INIT;`), an unknown kind, n_steps other than 5, speed_steps outside 2..n_steps, turn_window outside
 * 2..10, speed_window outside 2..30, a steer point outside 0..n_steps, a gap, dt, fov, w, h, crop_size or pixels_per_meter that is not
 * a positive finite number (fov < 180), any other field that is not finite. */
enum { LBC_AGENT_IMAGE = 0, LBC_AGENT_BIRDVIEW = 1 };
enum { LBC_AGENT_FLAG_DEGENERATE = 1, LBC_AGENT_FLAG_BAD = 2, LBC_AGENT_FLAG_INACTIVE = 4 };
#define LBC_AGENT_TURN_WINDOW_MAX 10
#define LBC_AGENT_SPEED_WINDOW_MAX 30
typedef struct lbc_agent_desc {
    unsigned struct_size;        /* = sizeof(lbc_agent_desc) */
    int kind;                    /* LBC_AGENT_* */
    int n_steps;                 /* waypoints per agent: 5 */
    int speed_steps;             /* BIRDVIEW: target_speed from the first speed_steps - 1 segments (reference SPEED_STEPS = 3) */
    double w, h, fov;            /* IMAGE: camera frame in pixels, horizontal field of view in degrees */
    double world_y, fixed_offset;/* IMAGE: camera height and the forward offset of the unprojection, metres */
    double crop_size;            /* BIRDVIEW: side of the map crop in pixels */
    double pixels_per_meter;     /* BIRDVIEW */
    double gap, dt;              /* waypoints are gap frames of dt seconds apart */
    int steer_points[4];         /* per command: index into targets[0..n_steps] of the point the car aims at */
    double turn_pid[4][3];       /* per command: Kp, Ki, Kd of the steering controller */
    double speed_pid[3];         /* Kp, Ki, Kd of the speed controller */
    int turn_window, speed_window;   /* 2..10 and 2..30 */
    double engine_brake_threshold, brake_threshold;   /* IMAGE, m/s */
    double stop_threshold;       /* BIRDVIEW, m/s */
} lbc_agent_desc;
#define LBC_AGENT_DESC_IMAGE_INIT { (unsigned)sizeof(lbc_agent_desc), 0, 5, 3, 384.0, 160.0, 90.0, 1.4, 4.0, 192.0, 5.0, 5.0, 0.1, \
                                    { 4, 3, 2, 2 }, { { 0.5, 0.2, 0.0 }, { 0.7, 0.1, 0.0 }, { 1.0, 0.1, 0.0 }, { 1.0, 0.5, 0.0 } }, \
                                    { 0.8, 0.08, 0.0 }, 10, 30, 2.0, 2.0, 1.0 }
#define LBC_AGENT_DESC_BIRDVIEW_INIT { (unsigned)sizeof(lbc_agent_desc), 1, 5, 3, 384.0, 160.0, 90.0, 1.4, 4.0, 192.0, 5.0, 5.0, 0.1, \
                                       { 3, 2, 2, 2 }, { { 1.0, 0.1, 0.0 }, { 1.0, 0.1, 0.0 }, { 0.8, 0.1, 0.0 }, { 0.8, 0.1, 0.0 } }, \
                                       { 1.0, 0.1, 2.5 }, 10, 30, 2.0, 2.0, 1.0 }
typedef struct lbc_agent_state {     /* one agent's controllers, 336 bytes; all-zero bytes = a fresh agent */
    double turn_ring[LBC_AGENT_TURN_WINDOW_MAX];      /* the last min(turn_count, turn_window) alphas, slots 0 .. turn_window - 1 in use */
    double speed_ring[LBC_AGENT_SPEED_WINDOW_MAX];    /* the last speed errors, likewise */
    int turn_count, turn_head;   /* values held (saturates at the window), slot the next value goes to */
    int speed_count, speed_head;
} lbc_agent_state;
size_t lbc_agent_state_bytes(int n_agents);      /* n_agents * sizeof(lbc_agent_state); 0 for n_agents <= 0 */
int lbc_agent_control(const lbc_agent_desc* desc, const float* pred, const float* speed, const float* command_onehot,
                      const unsigned char* active /* may be NULL */, int N, void* state, double* out, lbc_stream_t stream);
int lbc_agent_reset(const unsigned char* mask /* may be NULL */, int N, void* state, lbc_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Single-operator entry points of the HBM-bound kernels: what the executor above launches between the
 * convolutions, exported so that every kernel has its own parity test against torch CPU (tests/test_ops.py).
 * act_bf16 = 1: the activation tensors (void*) are bf16 in HBM, arithmetic stays f32.
 * ---------------------------------------------------------------------------------------- */

/* nn.BatchNorm2d (reference resnet.py:31,34,104,137; image.py:38,41,44,56).
 * lbc_bn_stats: per-workgroup partial (sum, sum^2) rows of x[pixels][C] -> partial[rows][2][C] (the convolution epilogues
 *   produce the same rows for their outputs); *rows receives the row count (query with x == NULL allowed; <= 1024).
 * lbc_bn_finalize_stats: partial rows -> scale = gamma*invstd, shift = beta - mean*scale, saved mean / invstd; train != 0
 *   also updates running_mean / running_var (momentum, unbiased variance) and num_batches_tracked (all nullable);
 *   train == 0 takes the statistics from running_mean / running_var.
 * lbc_bn_apply_relu_add_fwd: y = relu?(x*scale + shift (+ resid [*rscale + rshift])). */
int lbc_bn_stats(const void* x, long long pixels, int C, int act_bf16, float* partial, int* rows, lbc_stream_t stream);
int lbc_bn_finalize_stats(const float* partial, int rows, int C, long long count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                          int train, float* scale, float* shift, float* save_mean, float* save_invstd, lbc_stream_t stream);
int lbc_bn_apply_relu_add_fwd(const void* x, void* y, long long pixels, int C, const float* scale, const float* shift,
                              const void* resid, const float* rscale, const float* rshift, int relu, int act_bf16,
                              lbc_stream_t stream);
/* BatchNorm2d backward (autograd of the call sites above), fused with the backward of a following ReLU:
 *   g = dz * (mask > 0)   (mask nullable; mask_scale/mask_shift nullable: mask := mask*mask_scale + mask_shift first)
 *   dbeta = sum g, dgamma = sum g*xhat, dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n) over the first Cout channels.
 * g_out (nullable, may alias dz) receives g.  workspace: lbc_bn_bwd_workspace(C) bytes. */
size_t lbc_bn_bwd_workspace(int C);
int lbc_bn_bwd(const void* x, const void* dz, const void* mask, const float* mask_scale, const float* mask_shift,
               void* g_out, const float* gamma, const float* mean, const float* invstd, long long pixels, int C, int Cout,
               float* dgamma, float* dbeta, void* dx, float* workspace, int act_bf16, lbc_stream_t stream);

/* bn1 -> relu -> nn.MaxPool2d(3,2,1) of the ResNet stem (reference resnet.py:149-152, :106) and its backward.
 * fwd: y[N,H,W,C] (pre-BN) -> p[N,H/2,W/2,C], idx = arg-max tap 0..8 per output element (u8, nullable).
 * bwd: dp -> g[N,H,W,C] = gradient wrt the BatchNorm output (ReLU mask applied) + BatchNorm-backward partial rows
 *   (sum g, sum g*xhat) in partial[rows][2][C]; *rows receives the row count (query with dp == NULL allowed). */
int lbc_maxpool3x3s2_fwd(const void* y, const float* scale, const float* shift, void* p, unsigned char* idx, int N, int H, int W,
                         int C, int act_bf16, lbc_stream_t stream);
int lbc_maxpool3x3s2_bwd(const void* dp, const unsigned char* idx, const void* y, const float* scale, const float* shift,
                         const float* mean, const float* invstd, void* g, float* partial, int* rows, int N, int H, int W, int C,
                         int act_bf16, lbc_stream_t stream);

/* Waypoint head: 4 x (BatchNorm2d(64) -> Conv2d(64,5,1) -> SpatialSoftmax) -> stack -> select_branch
 * (reference image.py:54-60,82-84; common.py:29-35,136-152).  All per-branch parameter arrays are [4] pointers. */
typedef struct lbc_head_desc {
    const void* h;             /* decoder output [N][OH*OW][64], f32 or bf16 */
    int N, OH, OW, act_bf16;
    const float* mean[4];      /* BatchNorm statistics per branch [64]; training mode: the four entries are the same batch statistics */
    const float* invstd[4];
    const float* gamma[4];
    const float* beta[4];
    const float* w[4];         /* [5][64] */
    const float* bias[4];      /* [5] */
    const float* pos_x[4];     /* SpatialSoftmax buffers [OH*OW] */
    const float* pos_y[4];
    const float* cmd;          /* [N][4] one-hot */
} lbc_head_desc;
/* workspace (floats): N*40 (row statistics, fwd -> bwd) + N*20*65 + 8*20*65 + 3*64 + N*16*20*4 */
size_t lbc_head_workspace(int N);
int lbc_head_fwd(const lbc_head_desc* d, float* pred_all, float* pred_sel, float* workspace, lbc_stream_t stream);
/* backward of the last lbc_head_fwd on the same workspace (training-mode statistics): d_all [N,4,5,2] / d_sel [N,5,2]
 * (either nullable) -> dh (like h) and the parameter gradients dgamma/dbeta [4][64], dw [4][5*64], dbias [4][5]. */
int lbc_head_bwd(const lbc_head_desc* d, const float* pred_all, const float* d_all, const float* d_sel, void* dh,
                 float* const* dgamma, float* const* dbeta, float* const* dw, float* const* dbias, float* workspace,
                 lbc_stream_t stream);

/* Stem: input pass + 7x7/2 convolution 3|7 -> 64 (reference resnet.py:102; common.py:101-109 NormalizeV2 fused).
 * lbc_nchw_to_input / lbc_u8nhwc_to_input: image -> xp[N][H+6][W+6][C] (3-pixel zero border; bf16 when xp_bf16),
 *   optionally ImageNet-normalised (normalize = 1, C = 3).
 * lbc_stem_fwd: xp, w[64][7][7][C] -> y[N][H/2][W/2][64] (+ statistics partial rows, nullable).
 * lbc_stem_wgrad: xp, dy -> dw[64][7][7][C]; workspace lbc_stem_wgrad_workspace() bytes.  bf16: lbc_conv_desc.bf16 modes 0/1/2; other values
 * (the split mode 4 included: there is no split stem, precision 3 runs the stem with 0) are refused with LBC_EINVAL. */
int lbc_nchw_to_input(const float* image_nchw, void* xp, int xp_bf16, int N, int C, int H, int W, int normalize, lbc_stream_t stream);
int lbc_u8nhwc_to_input(const unsigned char* image_nhwc, void* xp, int xp_bf16, int N, int C, int H, int W, int normalize,
                        lbc_stream_t stream);
int lbc_stem_fwd(const void* xp, const float* w, void* y, float* stats, int* stats_rows, int N, int H, int W, int C, int bf16,
                 lbc_stream_t stream);
size_t lbc_stem_wgrad_workspace(int N, int H, int W, int C);
int lbc_stem_wgrad(const void* xp, const void* dy, float* dw, void* workspace, int N, int H, int W, int C, int bf16,
                   lbc_stream_t stream);

/* Device-side input pipeline on the dataset's uint8 frames (what the reference does per sample in CPU dataloader workers).
 * lbc_birdview_crop_u8: the fixed crop of the stored 320 x 320 x 7 bird-view (reference image_lmdb.py:150-163: rows
 *   [58:250], cols [64:256]); generic window copy src[N][SH][SW][C] -> dst[N][H][W][C].
 * lbc_augment_rgb_u8: the "super_hard" colour augmentation recipe (reference bird_view/augmenter.py:227-279) on a batch
 *   of RGB frames [N][H][W][3], in place; per-image parameters (operator order, magnitudes, seed) come from the host
 *   (learningbycheating_amd/bird_view/augmenter.py), per-pixel randomness from a counter-based hash.  scratch: N*H*W*3
 *   floats (needed when any image's sequence contains the blur). */
typedef struct lbc_aug_params {
    int order[8];                /* 0 blur, 1 gaussian noise, 2 coarse dropout, 3 dropout, 4 add, 5 multiply, 6 contrast */
    int n_ops, blur_pos;         /* blur_pos = index of the blur in order[], n_ops if absent */
    unsigned seed;
    float blur_sigma;
    float noise_scale; int noise_per_channel;
    float coarse_p; int coarse_h, coarse_w, coarse_per_channel;
    float dropout_p; int dropout_per_channel;
    float add[3], multiply[3], contrast[3];
} lbc_aug_params;
int lbc_birdview_crop_u8(const unsigned char* src, unsigned char* dst, int N, int SH, int SW, int C, int y0, int x0, int H, int W,
                         lbc_stream_t stream);
/* lbc_birdview_warp_crop_u8: the jittered sample of the privileged agent's loader (reference bird_view/utils/datasets/birdview_lmdb.py:
 *   103-125): per image, cv2.warpAffine(bird_view, cv2.getRotationMatrix2D((160, 260), delta_angle, 1.0), (320, 320), INTER_LINEAR) and
 *   the 192 x 192 window at (y0, x0) of the result, in one pass.  params[n].im = the INVERTED 2 x 3 matrix (what warpAffine derives from
 *   its argument), source (X, Y) = (im[0] x + im[1] y + im[2], im[3] x + im[4] y + im[5]); OpenCV's 8-bit bilinear arithmetic (1/32-pixel
 *   coordinates, 15-bit weight table, zero border).  src [N][SH][SW][C] -> dst [N][H][W][C]. */
typedef struct lbc_warp_params { double im[6]; int y0, x0; } lbc_warp_params;
int lbc_birdview_warp_crop_u8(const unsigned char* src, unsigned char* dst, const lbc_warp_params* params_dev, int N, int SH, int SW, int C,
                              int H, int W, lbc_stream_t stream);
int lbc_augment_rgb_u8(unsigned char* images, const lbc_aug_params* params_dev, float* scratch, int N, int H, int W, int any_blur,
                       lbc_stream_t stream);

/* Device-resident prioritised replay buffer of phase 2 (reference training/phase2_utils.py:190-289): weighted sampling, frame gather
 * with the --batch_aug fan-out, and the write-back of the new weights, without a host round trip.  Every call only enqueues on
 * `stream`; none copies to the host or synchronises.  Indices are trusted where no bound is passed (gather, scatter, meta): they come
 * from lbc_replay_sample or from a permutation of the buffer.
 * lbc_replay_cdf: cdf[i] = w[0] + ... + w[i] in double (inclusive), n >= 1.  A weight that is negative, NaN or +-Inf contributes 0 and
 *   is counted in *bad_count (device memory, overwritten).  Deterministic (fixed summation order, no atomics); three launches.
 * lbc_replay_sample: B draws with replacement, probability w[i] / sum(w).  Draw j of step t is counter-based (no device state):
 *   h1 = hash3(seed ^ t_hi, 2j, t_lo), h2 = hash3(seed ^ t_hi, 2j + 1, t_lo) with t_lo / t_hi the 32-bit halves of `step` and
 *   hash3(s, a, b) = H(s ^ H(a * 0x9E3779B9 + H(b + 0x85EBCA6B))), H = the "lowbias32" finaliser (x ^= x >> 16; x *= 0x7feb352d;
 *   x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16);  u = ((h1 >> 5) * 2^26 + (h2 >> 6)) * 2^-53 * cdf[n-1];  idx[j] = the first i with
 *   cdf[i] > u.  An entry of weight 0 is never returned (exactly so where the prefix sums are exact; with arbitrary weights two
 *   neighbouring sums may differ by one unit in the last place of a double, which can give a zero weight a share of 2^-53 of the
 *   total); should the product round up to cdf[n-1], the last entry of non-zero weight is.  cdf[n-1] must be > 0 (the caller checks the total it reads back once per epoch).
 * lbc_replay_gather_u8: dst row b * reps + k = src row idx[b], k < reps (torch.repeat_interleave of the gathered rows).  row_bytes
 *   must be a multiple of 16 and both base pointers 16-byte aligned (LBC_EINVAL otherwise): rows move as 16-byte words.
 * lbc_replay_scatter_u8: dst row slot[m] = src row m, m < M (fills free slots, overwrites evicted ones); slots must be distinct.
 * lbc_replay_meta: speed_out[b * reps + k] = speed[idx[b]]; onehot_out[b * reps + k][0..3] = one-hot of clamp(cmd[idx[b]] - 1, 0, 3)
 *   (the rule of bird_view/utils/train_utils.py one_hot: commands are 1..4, anything below selects branch 0, anything above branch 3).
 * lbc_replay_writeback: new_w[idx[b]] = (w_batch[b * reps] + ... + w_batch[b * reps + reps - 1]) / reps, summed in f32 in index order.
 *   Where several b carry the same index the LAST one wins (numpy fancy assignment); idx[b] < 0 or >= n is ignored.  B <= 1024. */
int lbc_replay_cdf(const float* w, int n, double* cdf, long long* bad_count, lbc_stream_t stream);
int lbc_replay_sample(const double* cdf, int n, unsigned seed, unsigned long long step, int B, int* idx, lbc_stream_t stream);
int lbc_replay_gather_u8(const unsigned char* src, long long row_bytes, const int* idx, int B, int reps, unsigned char* dst, lbc_stream_t stream);
int lbc_replay_scatter_u8(const unsigned char* src, long long row_bytes, const int* slot, int M, unsigned char* dst, lbc_stream_t stream);
int lbc_replay_meta(const float* speed, const int* cmd, const int* idx, int B, int reps, float* speed_out, float* onehot_out, lbc_stream_t stream);
int lbc_replay_writeback(const float* w_batch, const int* idx, int B, int reps, int n, float* new_w, lbc_stream_t stream);

/* A replay buffer over a resident dataset holds frame INDICES instead of frames (training/replay.py DeviceReplayBuffer(source=...)).
 * lbc_replay_gather_indirect_u8: dst row b * reps + k = src row frame_of_slot[idx[b]], k < reps: lbc_replay_gather_u8 with a second
 *   index level, the same argument rules.  Both index levels are trusted.
 * lbc_replay_admit: m scored candidates (cw, cframe, ccmd, cspeed, each [m]) into a buffer of n occupied slots out of `limit`, in one
 *   launch of one workgroup; what m ReplayBuffer.add_data calls of the reference decide (phase2_utils.py:256-265), ties made definite.
 *   The slot arrays weights f32 / frame i32 / cmd i32 / speed f32, each [limit], and slot_of_frame i32 [F] (the slot that holds a frame,
 *   -1 = not stored) are read and written in place.  cframe must be distinct and inside [0, F): the caller checks, the kernel trusts.
 *   With key(w) = w if w is finite and >= 0, else -1 (unusable weights rank lowest; stored VALUES stay raw, as lbc_replay_cdf expects):
 *     1. refresh  a candidate whose frame is stored (slot_of_frame[f] >= 0) overwrites that slot's weight and takes no further part;
 *     2. append   the remaining candidates fill slots n, n + 1, ... in candidate order while there is room;
 *     3. compete  once the buffer is full, stored slots and the candidates still waiting are ranked by key descending, stored before
 *                 waiting at equal key, lower slot / candidate index first; the first `limit` stay; the evicted slots in ascending order
 *                 receive the surviving candidates in candidate order (frame, cmd, speed, raw weight).  A candidate appended in step 2
 *                 can be evicted by a later one of the same call.
 *   slot_of_frame is -1 for every evicted frame and the new slot for every admitted one.  record (device memory, 4 ints) =
 *   {n_after, refreshed, admitted, evicted}: occupied slots at the end; the count of step 1; candidates that occupy a slot at the end;
 *   frames stored before the call and gone after it.  No atomics: the result is a function of the inputs.  1 <= limit <= 2^20,
 *   1 <= m <= 2^20, 0 <= n <= limit, workspace_bytes >= lbc_replay_admit_workspace(limit, m) (device memory, contents irrelevant; the
 *   query returns 0 outside those ranges); anything else is LBC_EINVAL and launches nothing. */
int lbc_replay_gather_indirect_u8(const unsigned char* src, long long row_bytes, const int* frame_of_slot, const int* idx, int B, int reps,
                                  unsigned char* dst, lbc_stream_t stream);
size_t lbc_replay_admit_workspace(int limit, int m);
int lbc_replay_admit(float* weights, int* frame, int* cmd, float* speed, int* slot_of_frame, int F, int n, int limit, const float* cw, const int* cframe,
                     const int* ccmd, const float* cspeed, int m, void* workspace, size_t workspace_bytes, int* record, lbc_stream_t stream);

/* The on-policy tick of phase 2 (reference training/train_image_phase2.py:61-149 rollout, :45-58 get_control): after both networks and both
 * controllers have run for N agents, who drives is decided and what the agents saw is recorded on the device.  Both calls only enqueue on
 * `stream`.  The split into two launches is deliberate: the cursors and the tick counter are read and advanced by the ONE workgroup of
 * lbc_rollout_decide, never by the copy grid, whose late workgroups would otherwise see an advanced counter.
 * lbc_rollout_decide: one launch of one workgroup, 1 <= N <= 1024.  Reads per agent the student controller's and the teacher controller's
 *   row of 8 doubles (lbc_agent_control's output layout), weight [N] f32 (lbc_phase2_weight), speed [N], command_onehot [N][4], active [N]
 *   (NULL = all active); from device memory *p_student (double), *tick (64-bit counter), cursor [N] i32, dropped [N] i32.  Active agent a:
 *     u = hash3(seed ^ (unsigned)(tick >> 32), (unsigned)tick, a) / 2^32 in double (hash3 as under lbc_replay_sample); the applied control
 *     is the student's iff u < *p_student, else the teacher's.  If 0 <= cursor[a] < capacity: slot[a] = a * capacity + cursor[a], that
 *     slot's slot_cmd (1 + the index of the command's 1, the rule of lbc_agent_control), slot_speed and slot_weight are written, cursor[a]
 *     advances.  Otherwise slot[a] = -1 and dropped[a] advances (the reference stops appending at episode_length, :137).
 *   An inactive agent: slot[a] = -1, an all-zero row, cursor and dropped untouched.  One thread advances *tick by one.
 *   out [N][16] doubles: 0-2 applied steer / throttle / brake; 3 who (1 student, 0 teacher); 4 weight; 5 staged count after the tick;
 *   6, 7 the student's and the teacher's controller flags; 8-10 the student's controls; 11-13 the teacher's; 14 dropped this tick (0 / 1);
 *   15 zero.  slot_cmd / slot_speed / slot_weight hold N * capacity entries.  Double arithmetic, no atomics.
 * lbc_rollout_stage_u8: for every agent with 0 <= slot[a] < stage_rows, row a of rgb (rgb_row_bytes each) and row a of birdview go to row
 *   slot[a] of rgb_stage and birdview_stage; both kinds in one launch, 16 bytes per lane.  Reads nothing lbc_rollout_decide advances.
 * LBC_EINVAL with a message and nothing launched: a NULL pointer (but active), N outside [1, 1024], capacity < 1 or N * capacity >= 2^31,
 *   stage_rows < 1, row bytes that are not positive multiples of 16, frames or staging arrays that are not 16-byte aligned, doubles and the
 *   counter not 8-byte aligned. */
int lbc_rollout_decide(const double* student, const double* teacher, const float* weight, const float* speed, const float* command_onehot,
                       const unsigned char* active, int N, int capacity, unsigned seed, const double* p_student, unsigned long long* tick,
                       int* cursor, int* dropped, int* slot, int* slot_cmd, float* slot_speed, float* slot_weight, double* out, lbc_stream_t stream);
int lbc_rollout_stage_u8(const unsigned char* rgb, long long rgb_row_bytes, const unsigned char* birdview, long long birdview_row_bytes, const int* slot,
                         int N, long long stage_rows, unsigned char* rgb_stage, unsigned char* birdview_stage, lbc_stream_t stream);

/* Device-resident LMDB dataset (bird_view/utils/datasets/resident.py): the per-sample work of the host loader -- frame look-up, crop or
 * rotation of the bird-view map, waypoints -- over a batch of frames that live in HBM.  The host draws and uploads one record of four
 * int32 per sample, `draws[b] = (frame index, delta_angle in degrees, dx, dy)`; every call only enqueues on `stream`.  Indices are
 * trusted (no frame count is passed): the caller checks them on the host before it uploads them.  Offsets are 64-bit throughout.
 * (Exports added without a new ABI number; existing signatures unchanged.)
 * lbc_dataset_gather_crop_u8: dst[b * reps + r] = the window rows [y0, y0 + H), columns [x0, x0 + W) of src frame idx[b]; src
 *   [F][SH][SW][C], dst [B * reps][H][W][C].  Moves 16 bytes per lane when W * C, x0 * C, SW * C, SH * SW * C and both base pointers are
 *   multiples of 16, a byte per lane otherwise.  With the whole frame as the window this is an indexed row gather.
 * lbc_dataset_gather_warp_crop_u8: lbc_birdview_warp_crop_u8 through the record -- source frame draws[b].idx, inverted matrix
 *   table[draws[b].delta_angle + A].im (2 A + 1 entries, one per integer angle in [-A, A]; their y0 / x0 are not read), window origin
 *   rows draws[b].dy + (260 - H / 2) - H / 2, columns draws[b].dx + 160 - W / 2 (the ego pixel (160, 260) of the stored 320 x 320 map).
 *   The same per-pixel arithmetic as lbc_birdview_warp_crop_u8: equal inputs give equal bytes.
 * lbc_dataset_targets: loc[(b * reps + r)][k] (n_step x 2 f32, pixels of the crop) and speed[b * reps + r] of sample draws[b].idx from
 *   the measurement table [rows][5] f32 = (x, y, heading, speed, cmd), one row per stored frame, episodes contiguous; the sample's row
 *   is row_of_sample[idx], its k-th future position row + (k + 1) * gap (the caller guarantees that these rows belong to the same
 *   episode).  Restates the reference's image_lmdb.py:143-163 / birdview_lmdb.py:127-141: (x - ox) * 5 in f32, angle = heading +
 *   delta_angle * pi / 180 and everything after it in double, one cast to f32 at the end.
 * lbc_dataset_gather_rows_f32: dst[(b * reps + r) * R + j] = src[draws[b * stride] * R + j], j < R: an indexed gather of f32 rows (the
 *   cached waypoints of the frozen teacher, R = 50: all 4 x 5 x 2, then the selected 5 x 2).  stride = 4 reads the frame index out of
 *   the records above, stride = 1 a dense int32 index vector.  Moves 8 bytes per lane when R is even and both base pointers are
 *   multiples of 8 (200-byte rows are 8-byte aligned, not 16), 4 bytes per lane otherwise.  The words move as integers: NaN payloads,
 *   infinities and -0.0 arrive bit for bit.  No atomics; every launch writes the same bytes. */
int lbc_dataset_gather_crop_u8(const unsigned char* src, const int* idx, int B, int reps, int SH, int SW, int C, int y0, int x0, int H, int W,
                               unsigned char* dst, lbc_stream_t stream);
int lbc_dataset_gather_warp_crop_u8(const unsigned char* src, const int* draws, const lbc_warp_params* table, int A, int B, int reps, int SH, int SW,
                                    int C, int H, int W, unsigned char* dst, lbc_stream_t stream);
int lbc_dataset_targets(const float* table, const int* row_of_sample, const int* draws, int B, int reps, int gap, int n_step, int img_size, int crop_size,
                        float* loc, float* speed, lbc_stream_t stream);
int lbc_dataset_gather_rows_f32(const float* src, const int* draws, int stride, int B, int reps, int R, float* dst, lbc_stream_t stream);

/* Runtime options (A/B switches, tuning knobs, test hooks): names are the LBC_* environment variables that initialise the
 * table at load time; -1 = unset.  The one option read when a network is created (LBC_NO_SIDE_STREAM) applies to
 * networks created afterwards.  An LBC_* environment variable that is not in the table (a switch of an earlier round, a typo) is reported
 * on stderr when the library loads -- it would otherwise be ignored silently and an A/B script would measure nothing. */
int lbc_config_set(const char* name, long long value);
long long lbc_config_get(const char* name);

/* Built-in launch profiler: HIP-event timing of every kernel launch on its own stream, booked per
 * kernel class together with the launch's algorithmic flops and HBM bytes.  report() writes one
 * line per class "name count total_ms total_flops total_bytes" and resets the log. */
int lbc_profile_enable(int on);
int lbc_profile_report(char* buf, int cap);
/* parameter elements behind the optimizer's chunk table: only books the profiler's bytes of an lbc_adam_step launch (28 B per element) */
void lbc_adam_profile_elems(long long n);

#ifdef __cplusplus
}
#endif
#endif /* LBC_HIP_H */
