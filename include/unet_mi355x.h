/* unet_mi355x.h -- C-ABI of the MI355X-native UNet forward path.
 *
 * Drop-in for the reference segmentation call surface (tingyu-c/TW-invoice-unet-ocr-llm):
 *   unet_model.UNet(n_channels, n_classes)      unet_model.py:23-53   -> unet_create
 *   model.load_state_dict(torch.load(ckpt))     inference.py:17-24     -> unet_load_weights
 *   model(x)  (UNet.forward)                    unet_model.py:55-86    -> unet_forward (logits)
 *   sigmoid + per-field thresholds              inference.py:72-79     -> unet_forward (masks)
 *
 * The reference has no FFI (it is pure Python on torch); this header is the boundary a
 * ctypes/cffi binding loads.  Plain C types only; no torch or C++ types cross it.
 *
 * Conventions
 *   - return value: 0 = OK, negative = error (UNET_E*); unet_last_error() gives the
 *     message for the calling thread.  C++ exceptions never cross the ABI.
 *   - device pointers are caller-owned (e.g. torch data_ptr()); work is enqueued on the
 *     caller's HIP stream (hipStream_t passed as void*), with no hidden synchronisation
 *     except inside unet_load_weights / unet_reserve (allocation + upload) and the first
 *     unet_preprocess of a new photo geometry (coefficient upload), and unet_score_reserve or a
 *     unet_score whose scratch is too small (allocation; unet_loss_reserve / unet_loss_grad alike).  unet_forward never
 *     allocates: size the workspace with unet_reserve first.
 *   - a handle owns one workspace.  Calls on it must not overlap on the host (serialise them;
 *     the Python wrapper holds a lock).  On the device, a call issued on a different stream than
 *     the previous one waits for that previous call (hipStreamWaitEvent), so the workspace is
 *     never shared by two forwards in flight.
 */
#ifndef UNET_MI355X_H
#define UNET_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ABI_VERSION 5   /* 2: unet_forward requires unet_reserve; Cfg renumbered; fp16 range check. 3: unet_crop_stats.
                                 4: unet_launch_label_at, unet_small_batch_limit, unet_photo_graph_create, unet_block_*
                                 5: unet_photo_graph_set_masks (the masks copy is its own node); UNET_DTYPE_F32 as
                                    three bf16 terms, UNET_DTYPE_F32_EXACT the exact-fp32 MFMA
                                    (still 5, symbols added only: unet_score_reserve, unet_score, unet_score_entry,
                                    UNET_TGT_*; then unet_loss_reserve, unet_loss_grad, unet_loss_config; then
                                    unet_head_reserve, unet_head_forward, unet_head_backward; then unet_debug_fill,
                                    unet_block_debug_fill; then unet_head_forward_typed, unet_head_backward_typed;
                                    then unet_head_step_reserve, unet_head_step, unet_adamw_config;
                                    then unet_head_score_reserve, unet_head_score; then unet_launch_split_at;
                                    then unet_launch_walk_at, unet_block_launch_walk_at) */

/* error codes */
#define UNET_OK 0
#define UNET_EINVAL (-1)     /* bad argument (maps to ValueError)                    */
#define UNET_ESHAPE (-2)     /* unsupported shape, e.g. H or W not divisible by 16     */
#define UNET_ENOMEM (-3)     /* device allocation failed                               */
#define UNET_EHIP (-4)       /* HIP runtime error                                      */
#define UNET_ESTATE (-5)     /* call out of order (e.g. forward before weights)       */
#define UNET_EKEY (-6)       /* state_dict key missing / unexpected / wrong shape      */

/* compute / storage dtype of the activations and packed weights (accumulation is fp32).
 * UNET_DTYPE_F32: fp32 storage and weights; every product of the 3x3 and ConvTranspose layers computed as
 * three bf16 terms per operand (x = hi + mid + lo, 6 bf16 MFMA products per K block, fp32 accumulation):
 * fp32 accuracy (the reference's fp32 forward within 2e-5 of the logit scale, tests/test_forward_gpu.py)
 * on the 2.5 PFLOP/s bf16 pipe.  UNET_DTYPE_F32_EXACT: the same plan on the exact-fp32 MFMA
 * (v_mfma_f32_16x16x4_f32, 157 TFLOP/s). */
#define UNET_DTYPE_F32 0
#define UNET_DTYPE_BF16 1
#define UNET_DTYPE_F16 2
/* bf16 at resolution levels 2-4, fp16 at the two full-resolution levels 0-1 (where the mask
 * boundaries are decided): the precision plan of the headline benchmark, see DESIGN.md §2.
 * fp16 storage (UNET_DTYPE_F16, and levels 0-1 of MIXED) holds |v| <= 65504: unet_load_weights
 * refuses (UNET_EINVAL) a checkpoint whose BN-folded weights or biases exceed that at an fp16
 * level; activations beyond it would become inf -- use BF16 (fp32's range) or F32 for such nets. */
#define UNET_DTYPE_MIXED 3
#define UNET_DTYPE_F32_EXACT 4

/* input layouts / dtypes accepted by unet_forward */
#define UNET_LAYOUT_NCHW 0   /* [N][n_channels][H][W] (the reference's torch layout)             */
#define UNET_LAYOUT_NHWC 1   /* [N][H][W][n_channels] (decoded photos)                           */
#define UNET_IN_F32 0        /* float32 values                                                   */
#define UNET_IN_U8 1         /* uint8 values v, read as v / 255.0f (inference.py:40's scaling)   */

/* mask outputs of unet_forward */
#define UNET_MASK_NONE 0
#define UNET_MASK_U8 1    /* uint8 [N][n_classes][H][W], 1 where sigmoid(logit) > thr      */
#define UNET_MASK_BITS 2  /* uint8 [N][n_classes][H][W/8], bit b of byte x/8 = pixel x      */

typedef struct unet_handle unet_handle;

typedef struct unet_config {
  int n_channels;     /* input channels: 1 or 3 (UNet(n_channels=...), unet_model.py:24) */
  int n_classes;      /* 1..4 (UNet(n_classes=...); the app uses 3)                       */
  int dtype;          /* UNET_DTYPE_*                                                     */
  int device;         /* HIP device ordinal                                               */
  float thresholds[4];/* per-class probability thresholds (inference.py:76-78)           */
} unet_config;

typedef struct unet_tensor_view {
  const char* name;   /* state_dict key, e.g. "down1.net.0.weight"                       */
  const void* data;   /* host pointer, contiguous                                         */
  int dtype;          /* 0 = float32, 1 = int64 (num_batches_tracked; ignored)            */
  int ndim;
  int64_t shape[4];
} unet_tensor_view;

/* Create a handle for UNet(n_channels, n_classes) on cfg->device.
 * Replaces: unet_model.UNet.__init__ (unet_model.py:24-53). */
int unet_create(const unet_config* cfg, unet_handle** out);

/* Strictly load the 136-key reference state_dict (host fp32), fold eval BatchNorm
 * (eps 1e-5) into the convs, pre-pack NHWC/MFMA panels and upload them.
 * Replaces: load_state_dict(strict=True) + eval() (inference.py:20-23). */
int unet_load_weights(unet_handle* h, const unet_tensor_view* tensors, int n);

/* Bytes of device workspace unet_forward needs for (N, H, W). */
size_t unet_workspace_bytes(const unet_handle* h, int N, int H, int W);

/* Allocate (grow) the workspace for up to (N, H, W): unet_forward requires it (UNET_ESTATE
 * otherwise; ABI 1 allocated inside the forward) and then neither allocates nor synchronises
 * (graph-capturable).  Growing waits for the handle's queued work.
 * A forward issued on a stream under capture (unet_graph_create, or the caller's own capture, e.g.
 * torch.cuda.graph on its side stream) neither waits for nor records the handle's stream-order
 * event; ordering the replay after other work on the handle is then the caller's. */
int unet_reserve(unet_handle* h, int N, int H, int W);

/* Forward pass.  x: device tensor [N][n_channels][H][W] (x_layout UNET_LAYOUT_NCHW) or
 * [N][H][W][n_channels] (UNET_LAYOUT_NHWC) of fp32 (x_dtype UNET_IN_F32) or uint8 (UNET_IN_U8,
 * value / 255).
 * logits: device fp32 NCHW [N][n_classes][H][W] or NULL.
 * masks:  device uint8 per mask_kind or NULL (mask_kind UNET_MASK_NONE).
 * H, W must be divisible by 16 (the reference raises inside torch.cat otherwise).
 * Replaces: UNet.forward (unet_model.py:55-86) and inference.py:72-79. */
int unet_forward(unet_handle* h, const void* x, int x_layout, int x_dtype,
                 void* logits, void* masks, int mask_kind,
                 int N, int H, int W, void* hip_stream);

/* unet_forward, plus the bounding box of every (image, field) mask -- the np.where ->
 * min/max step of run_unet (inference.py:84-90) on the device, so a caller that only needs
 * the crop rectangles copies 16 bytes per field instead of the mask (and a multi-GPU caller
 * all-gathers 48 bytes per image).
 * boxes: device int32 [N][n_classes][4] = x_min, y_min, x_max, y_max in mask pixels
 *        (inclusive), all four -1 for an empty mask.
 * masks / mask_kind as for unet_forward; when masks is NULL (or mask_kind is
 * UNET_MASK_NONE) the masks go to the workspace and only the boxes are returned.
 * Replaces: UNet.forward + inference.py:72-90. */
int unet_forward_boxes(unet_handle* h, const void* x, int x_layout, int x_dtype,
                       void* logits, void* masks, int mask_kind, int32_t* boxes,
                       int N, int H, int W, void* hip_stream);

/* GPU preprocessing of one photo (inference.py:62-64 + preprocess, :30-44):
 * PIL Image.resize((ow, oh)) with Pillow's default BICUBIC filter -- bit-exact with Pillow's
 * fixed-point separable resampler --, convert("RGB") (gray replicated), /255 as float32, CHW.
 * Pass order: the horizontal pass first (8-bit intermediate), then the vertical pass, as Pillow's resampler
 * runs one resize.  One exception to "bit-exact with Image.resize": a newer Pillow's Image.resize (12.2 has the
 * branch, 10.2 does not) resizes a photo with ih > 100 * iw that it makes less tall (oh < ih) as two one-axis
 * resizes, the vertical one first, and its bytes then differ from this function's; such photos belong on the
 * host (the Python drop-in's run_unet routes them there).
 * img: device uint8 HWC [ih][iw][channels], channels 3 (mode "RGB"), 1 (mode "L") or 4 (RGBX: Pillow's own
 *      in-memory layout of an "RGB" image, 4 bytes per pixel, the 4th ignored -- uploaded without repacking);
 * x:   device fp32 [3][oh][ow] (e.g. one image's slot of the unet_forward input batch).
 * Coefficient tables are cached per (ih, iw, oh, ow) in the handle (first call per geometry
 * uploads them synchronously).  Stream-ordered on hip_stream. */
int unet_preprocess(unet_handle* h, const void* img, int ih, int iw, int channels,
                    float* x, int oh, int ow, void* hip_stream);

/* The crop step of run_unet (inference.py:92-127) on the device photo, so the host never reads
 * crop pixels: for every mask box (unet_forward_boxes' output, in a box_h x box_w mask), the crop
 * rectangle in photo pixels -- the reference's float64 arithmetic: scale = iw / box_w, x1 =
 * int(x_min * scale), x2 = int(x_max * scale), pad_x = int((x2 - x1) * pad) (pad = 0.15), clamp
 * to [0, iw] (y likewise) -- and the sum of the crop's uint8 values over every channel.  The
 * reference's rejections are then host tests: x2 <= x1 or y2 <= y1 (empty crop), and
 * np.array(crop).mean() < 3  <=>  sum < 3 * (x2 - x1) * (y2 - y1) * channels (numpy's float64 sum
 * of the integers is exact).  img: device uint8 HWC [ih][iw][channels] (unet_preprocess's input);
 * boxes: device int32 [n_boxes][4]; rects: device int32 [n_boxes][4] (x1, y1, x2, y2; -1s for an
 * empty box); sums: device uint64 [n_boxes] (channels 4 = RGBX: the sum over R, G, B).  Needs no handle;
 * stream-ordered on hip_stream. */
int unet_crop_stats(const void* img, int ih, int iw, int channels, const int32_t* boxes, int n_boxes,
                    int box_h, int box_w, double pad, int32_t* rects, uint64_t* sums, void* hip_stream);

/* Number of launch slots in one forward (first conv, 17 implicit-GEMM 3x3 convs with
 * the fused pool / head epilogues, 4 ConvTranspose2d), in execution order:
 * down1.0 down1.3 down2.0 down2.3 down3.0 down3.3 down4.0 down4.3 bottleneck.0
 * bottleneck.3 up4 conv4.0 conv4.3 up3 conv3.0 conv3.3 up2 conv2.0 conv2.3 up1 conv1.0
 * conv1.3+out_conv.  On the 16-bit plans up1 runs inside the conv2.3 launch (its slot issues no
 * kernel: empty label, ~0 ms); the environment variable UNET_MI355X_FUSE_UP1=0, read by
 * unet_create, keeps it a launch of its own. */
#define UNET_NUM_LAUNCHES 22
int unet_num_launches(void);

/* Kernel instantiation run by launch i of a forward (e.g.
 * "conv3x3_ring_kernel<__bf16, 1, 4, 8, 3, 0, 1, 0, __bf16, __bf16, 16, 16>"), spelled like the demangled
 * symbol that rocprofv3 reports; "" for a bad index or a slot fused into the previous launch. */
const char* unet_launch_label(const unet_handle* h, int i);

/* The same for a forward of N x H x W: batches N <= unet_small_batch_limit(h) run the small-batch
 * plan, whose split layers launch two kernels -- "partial kernel + splitk_reduce_kernel<...>" -- and
 * whose under-filled layers may run finer row tiles; N = 0 (or N above the limit) gives the
 * large-batch labels of unet_launch_label.  The string lives until the calling thread's next call. */
const char* unet_launch_label_at(const unet_handle* h, int i, int N, int H, int W);

/* The small-batch plan's choice for launch i of a forward of N x H x W, which the label does not spell out:
 * *ks = K slices (1: the launch runs unsplit), *rows = row tile of the launch (0: the layer's own, else 64 or
 * 128: finer tiles over the layer's packing).  (1, 0) for a slot that launches nothing, for N = 0 and for N
 * above unet_small_batch_limit.  Host arithmetic only: no HIP call, no allocation.  UNET_EINVAL for a bad
 * index, a negative shape or null pointers. */
int unet_launch_split_at(const unet_handle* h, int i, int N, int H, int W, int* ks, int* rows);

/* The walk of launch i of a forward of N x H x W.  The ring kernels are persistent: every row tile of the launch
 * has *slots walkers, and walker s takes the pixel tiles s, s + *slots, ... (for a split launch a tile means a
 * (tile, K slice) pair, and a walker keeps one slice); *items = the most tiles one walker takes.  (0, 0) for a
 * launch that is no ring kernel (the first conv, the pre-cast, the fp32 LDS-halo family), for a slot that
 * launches nothing and for N = 0.  The environment variable UNET_MI355X_WALKERS=k, read by unet_create and
 * unet_block_create (A/B and tests only; unset or 0 = no cap), caps *slots at k (k rounded down to a multiple of
 * the slice count, never below it).  The launcher's own arithmetic, with no launch, no HIP call and no
 * allocation.  UNET_EINVAL for a bad index, a negative shape or null pointers. */
int unet_launch_walk_at(const unet_handle* h, int i, int N, int H, int W, int* slots, int* items);

/* Largest batch of the small-batch (split-K) plan, 0 when it is off (UNET_MI355X_KSPLIT=0 at
 * unet_create).  An image's outputs are bitwise the same for every N <= the limit, and for every N
 * above it; the two regimes agree within the fp32-accumulation tolerance, not bit for bit, so a
 * caller that must reproduce batch-1 results exactly runs its batches in chunks of at most the limit
 * (inference.run_unet_batch does). */
int unet_small_batch_limit(const unet_handle* h);

/* unet_forward, plus HIP-event timing of every launch on the given stream (ms, in the
 * order above, launch_ms[UNET_NUM_LAUNCHES]).  Synchronises on the stream; for
 * measurement only. */
int unet_forward_timed(unet_handle* h, const void* x, int x_layout, int x_dtype,
                       void* logits, void* masks, int mask_kind,
                       int N, int H, int W, void* hip_stream, float* launch_ms);

/* Copy an intermediate activation of the last forward (debug / per-layer parity):
 * name in {"c1","p1","c2","p2","c3","p3","c4","p4","bn","c7","u1","u2","u3","u4","c8a"}
 * (c_k: encoder skips, p_k: pooled maps, u_k: ConvTranspose outputs, c7: conv2 output,
 * c8a: conv1.net.0 output).  "c7" is UNET_ESTATE after a forward with up1 fused into conv2.3
 * (conv2's output then never leaves the registers; UNET_MI355X_FUSE_UP1=0 keeps it).
 * dst: device buffer receiving fp32 NCHW [N][C][h][w]; *numel receives the element count
 * when dst is NULL. */
int unet_debug_fetch(unet_handle* h, const char* name, float* dst, size_t* numel, void* hip_stream);

/* Fill the handle's scratch memory with one byte value (debug / tests of history independence: every output of
 * every entry point is a function of its arguments and the loaded weights only, never of what an earlier call left
 * in the scratch, so a call after a fill must give what it gives on a fresh handle; tests/test_history_gpu.py
 * fills 0xFF, a NaN in every float format).  One hipMemsetAsync over the full allocated size of each scratch
 * allocation that exists: the forward workspace (unet_reserve), the score, loss and head scratch, and the
 * preprocess row buffer.  Untouched: weights, the zero page, resize tables, the mask-box sync entries (state with
 * a defined idle value, not scratch), whatever a unet_graph owns, caller buffers.  Stream-ordered after the
 * handle's previous call like unet_forward; allocates nothing and leaves captured graphs valid.  A fill between a
 * forward and its unet_debug_fetch destroys what the fetch reads.  A NULL handle or a byte outside 0..255 is
 * UNET_EINVAL before any HIP call; with nothing allocated it is UNET_OK. */
int unet_debug_fill(unet_handle* h, int byte, void* hip_stream);

/* hipGraph of one forward (unet_forward, or unet_forward_boxes when boxes != NULL) over fixed
 * device buffers and a fixed (N, H, W): the 22-launch sequence is captured once and replayed by
 * unet_graph_launch with one host call -- the launch-bound small-batch case (run_unet's batch
 * of 1, inference.py:42).  A graph is stale (UNET_ESTATE at launch) once unet_load_weights or a
 * growing unet_reserve re-allocates the handle's device memory; capture again then.  Destroy
 * graphs before their handle. */
typedef struct unet_graph unet_graph;
int unet_graph_create(unet_handle* h, const void* x, int x_layout, int x_dtype,
                      void* logits, void* masks, int mask_kind, int32_t* boxes,
                      int N, int H, int W, unet_graph** out);
int unet_graph_launch(unet_graph* g, void* hip_stream);
int unet_graph_destroy(unet_graph* g);

/* One graph per photo geometry: the whole device part of run_unet (inference.py:58-129) -- the
 * upload of the pinned host photo (h_img; NULL: the caller fills img), unet_preprocess to size x size
 * into x (on the 16-bit plans, when the photo's height differs from size, the resize writes the first
 * conv's pre-cast input into the workspace instead and x is not written; the graph owns its resize
 * tables and row buffer, so the handle's geometry cache may evict its own copy), unet_forward_boxes at N = 1 (masks / mask_kind / boxes as there), unet_crop_stats (pad,
 * rects, sums as there) and the copies of masks, boxes, rects and sums into the pinned host buffers
 * given (each may be NULL; the masks copy is a node of its own; of the others, copies whose device and
 * host buffers both follow the previous one's in memory, e.g. boxes | rects | sums carved from one
 * device and one host block, are made as one) -- captured once and replayed by unet_graph_launch: one
 * host call and one stream synchronisation per photo.  Needs unet_reserve(h, 1, size, size) first;
 * stale (UNET_ESTATE at launch) under the same rules as unet_graph_create's graphs.  Destroy with
 * unet_graph_destroy. */
int unet_photo_graph_create(unet_handle* h, const void* h_img, void* img, int ih, int iw, int channels, float* x,
                            int size, void* masks, int mask_kind, int32_t* boxes, double pad, int32_t* rects,
                            uint64_t* sums, void* h_masks, void* h_boxes, void* h_rects, void* h_sums,
                            unet_graph** out);
/* Retarget a photo graph's masks copy (created with h_masks != NULL) to another pinned host buffer of the
 * same size, for its next replays (hipGraphExecMemcpyNodeSetParams1D): one graph per photo geometry serves
 * any number of caller-held mask buffers.  Host-side only; replays already enqueued keep their target.
 * Call it under the same serialisation as unet_graph_launch. */
int unet_photo_graph_set_masks(unet_graph* g, void* h_masks);

/* Multi-GPU data parallelism: one process per GPU, each rank runs
 * unet_forward / unet_forward_boxes on its contiguous shard of the batch, and the one exchange
 * step is an all-gather of the per-rank bit-packed masks (or boxes) over RCCL/xGMI.  These
 * entry points give a C host that collective without torch.distributed; RCCL is loaded at run
 * time (dlopen), so a host that never calls them never loads it.
 *   rank 0: unet_comm_get_unique_id(id) -> send the UNET_COMM_ID_BYTES bytes to every rank
 *   every rank: unet_comm_init(h, rank, nranks, id); ... unet_allgather(h, my_masks,
 *     all_masks, bytes_per_rank, stream) (recv = nranks x bytes_per_rank, rank order);
 *     unet_comm_destroy(h) (also done by unet_destroy).
 * unet_allgather is stream-ordered like unet_forward (it follows the handle's previous call). */
#define UNET_COMM_ID_BYTES 128
int unet_comm_get_unique_id(void* id);
int unet_comm_init(unet_handle* h, int rank, int nranks, const void* id);
int unet_allgather(unet_handle* h, const void* send, void* recv, size_t bytes_per_rank, void* hip_stream);
int unet_comm_destroy(unet_handle* h);

/* Scoring of labelled pages on the device: what train.py:129-160 keeps a checkpoint by (InvoiceLoss,
 * train.py:18-59), the per-field mask IoU, and a threshold sweep -- 64 bytes per (image, field) come back instead
 * of the logits.
 * target forms: */
#define UNET_TGT_F32_NCHW 0  /* fp32 [N][C][H][W], values in [0,1]: the tensor dataset.py:33-34 hands the loss */
#define UNET_TGT_U8_NHWC 1   /* uint8 [N][H][W][C], v read as v / 255.0f: the .npy mask files of dataset.py:32 */
/* Per element, in fp32 and op by op as the reference (train.py:58, 24-29, 40-45; gamma = 2, alpha is the host's):
 *   p = 1 / (1 + expf(-x));  pt = p * t;  pc = clamp(p, 1e-7f, (float)(1 - 1e-7));
 *   bce = (t - 1) * max(logf(1 - pc), -100) - t * max(logf(pc), -100);  q = expf(-bce);  u = 1 - q;  f = u * u * bce
 * accumulated per (n, c) in fp64 over a summation tree that depends on H * W only: an entry is bitwise reproducible
 * and independent of N and of the other images of the batch.  n_pred counts x > unet_logit_cut(thr[c]) (the masks
 * epilogue's predicate), n_tgt counts t > 0.5f (train.py:76), n_both both.  A NaN logit makes the four sums of its
 * entry NaN and counts as not predicted.  From the entries:
 *   Dice loss  = mean over (n, c) of 1 - (2 sum_pt + smooth) / (sum_p + sum_t + smooth)
 *   focal loss = alpha * sum of sum_focal / sum of n_px
 *   IoU        = n_both / (n_pred + n_tgt - n_both) */
typedef struct unet_score_entry {
  double sum_p, sum_t, sum_pt, sum_focal;
  int64_t n_pred, n_tgt, n_both, n_px;
} unet_score_entry;

/* Size the handle's score scratch (its own allocation: unet_workspace_bytes / unet_reserve are unaffected) for
 * scores of up to N images of H x W with up to 4 classes and K sweep candidates (0 = no sweep).  Allocating
 * waits for the handle's queued work. */
int unet_score_reserve(unet_handle* h, int N, int H, int W, int K);

/* Score logits (device fp32 NCHW [N][C][H][W], e.g. unet_forward's output; C in 1..4, any H, W >= 1) against
 * target (device, layout per target_kind).  thresholds: C host floats, NULL = the handle's.  entries: device
 * unet_score_entry [N][C].
 * Sweep (optional): sweep_probs = K <= 64 strictly ascending host probabilities and hist = device int64
 * [N][C][2][K+1]; every element increments hist[n][c][t > 0.5f][b], b = #{k : x > unet_logit_cut(sweep_probs[k])},
 * so suffix sums over b give n_pred, n_both and n_tgt at every candidate.  Both NULL (K ignored) = no sweep.
 * Two launches on hip_stream, stream-ordered after the handle's previous call like unet_forward; needs no
 * weights.  A scratch too small for the call is grown synchronously (like unet_preprocess's first call of a
 * geometry), except on a stream under capture, where that is UNET_ESTATE: call unet_score_reserve first (a later
 * growth re-allocates the scratch a captured score reads).  Bad arguments are UNET_EINVAL before any HIP call. */
int unet_score(unet_handle* h, const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
               const float* thresholds, unet_score_entry* entries, const float* sweep_probs, int K, int64_t* hist,
               void* hip_stream);

/* The differentiable half of the same loss: what train.py:137-142 does with a batch of logits
 * (loss = criterion(logits, mask); loss.backward()).  InvoiceLoss (train.py:49-59; gamma = 2, as in unet_score) as
 * one device fp32 scalar, and its gradient at the logits.
 *   loss = dice_weight * mean over (n, c) of 1 - (2 sum_pt + smooth) / (sum_p + sum_t + smooth)
 *        + focal_weight * focal_alpha * sum of sum_focal / (N C H W)
 * from the sums of unet_score (fp64, bitwise the entries unet_score writes for the same tensors).  The gradient is
 * autograd's backward of the reference module in fp32, op by op on the element chain above, so the clamp of
 * train.py:41 passes or cuts an element's focal gradient where the reference does; the Dice branch's per-plane
 * coefficients are formed in fp64.  A NaN logit makes the loss, its own gradient and the gradient of its whole
 * (n, c) plane NaN, as torch does. */
typedef struct unet_loss_config {
  float dice_weight, focal_weight, focal_alpha, smooth;   /* the reference: 0.85, 0.15, 0.8, 1.0 */
} unet_loss_config;

/* Size the handle's loss scratch (its own allocation: unet_workspace_bytes, unet_reserve and the score scratch are
 * unaffected) for losses of up to N images of H x W with up to 4 classes.  Allocating waits for the handle's queued
 * work. */
int unet_loss_reserve(unet_handle* h, int N, int H, int W);

/* logits: device fp32 NCHW [N][C][H][W], C in 1..4, any H, W >= 1; target: device, layout per target_kind (UNET_TGT_*).
 * grad_out: device fp32 scalar, the upstream gradient of the loss, NULL = 1.0.  loss: device fp32 scalar (required).
 * grad_logits: device fp32 [N][C][H][W], NULL = loss only; it may not be logits itself.
 * Three or four launches on hip_stream (the two of a score, one block of coefficients, the element-wise gradient),
 * stream-ordered after the handle's previous call; no host round trip, capturable; needs no weights.  The scratch
 * grows as unet_score's does: synchronously, or UNET_ESTATE on a stream under capture (call unet_loss_reserve
 * first).  Bad arguments are UNET_EINVAL before any HIP call. */
int unet_loss_grad(unet_handle* h, const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
                   const unet_loss_config* cfg, const float* grad_out, float* loss, float* grad_logits,
                   void* hip_stream);

/* The output head on its own: out_conv = Conv2d(64, C, 1) (unet_model.py:50) forward and backward over a stored
 * feature map -- what fine-tuning the head on a frozen backbone needs (train.py:137-142 restricted to out_conv).
 *   feat: device fp32 NCHW [N][64][H][W] (DoubleConv's output);  w: device fp32 [C][64], the memory of a contiguous
 *   Conv2d(64, C, 1).weight;  b: device fp32 [C].  w and b are the caller's (e.g. torch parameters an optimizer
 *   owns): these calls need no weights loaded into the handle.  C in 1..4, any H, W >= 1; 64-bit indices.
 * Forward:  logits[n][c][p] = b[c] + sum_k w[c][k] feat[n][k][p], one fp32 fmaf chain from the bias, k ascending:
 *   bitwise independent of pointer alignment, of N and of the image's place in the batch.
 * Backward, from feat, grad_logits [N][C][H][W] and w:
 *   grad_w[c][k] = sum_{n,p} g[n][c][p] feat[n][k][p],  grad_b[c] = sum_{n,p} g[n][c][p]: products and sums in fp64
 *     over a summation tree that depends on (N, H, W) only, rounded to fp32 once; two launches (per-block partials
 *     stored to the scratch, then a fixed-order sum), no atomics: bitwise reproducible.
 *   grad_feat[n][k][p] = sum_c w[c][k] g[n][c][p]: the product of c = 0, then fp32 fmaf, c ascending.
 * IEEE propagation, nothing special-cased: a NaN feature reaches the logits of its pixel and grad_w[:, k] of its
 * channel only; a NaN gradient reaches grad_w[c][:], grad_b[c] of its class and grad_feat of its pixel only.
 * A feature channel that is zero everywhere gives grad_w[:, k] == 0.0 exactly (finite gradients). */

/* Size the handle's head scratch (its own allocation: unet_workspace_bytes, unet_reserve, the score and the loss
 * scratch are unaffected) for backward calls of up to N images of H x W with up to 4 classes.  Allocating waits
 * for the handle's queued work. */
int unet_head_reserve(unet_handle* h, int N, int H, int W);

/* One launch on hip_stream, stream-ordered after the handle's previous call; capturable.  logits: device fp32
 * [N][C][H][W]; it may not be feat.  Bad arguments are UNET_EINVAL before any HIP call. */
int unet_head_forward(unet_handle* h, const float* feat, const float* w, const float* b, float* logits,
                      int N, int C, int H, int W, void* hip_stream);

/* grad_w [C][64] and grad_b [C] come as a pair (both or both NULL); grad_feat [N][64][H][W] may be NULL; not all
 * three.  grad_feat may not be feat or grad_logits.  Up to three launches on hip_stream, stream-ordered after the
 * handle's previous call; no host round trip, capturable.  The scratch grows as unet_score's does: synchronously,
 * or UNET_ESTATE on a stream under capture (call unet_head_reserve first).  Bad arguments are UNET_EINVAL before
 * any HIP call. */
int unet_head_backward(unet_handle* h, const float* feat, const float* grad_logits, const float* w,
                       float* grad_w, float* grad_b, float* grad_feat, int N, int C, int H, int W, void* hip_stream);

/* The same two calls on a feature map stored in 16 bits (a feature cache of half the size: DESIGN.md section 11).
 * feat_dtype: UNET_DTYPE_F32 (feat is const float*, and the call runs the kernels of the untyped one),
 * UNET_DTYPE_F16 or UNET_DTYPE_BF16 (feat is device fp16 / bf16 NCHW [N][64][H][W]); any other value, MIXED and
 * F32_EXACT included, is UNET_EINVAL naming feat_dtype.  Each 16-bit feature is widened to fp32 once, exactly
 * (fp16 subnormals, signed zeros, infinities and NaNs included; bf16 is a 16-bit shift), and the arithmetic above
 * runs on the widened values: logits, grad_w, grad_b and grad_feat are, bit for bit, those of the untyped calls on
 * the widened tensor (where a feature is NaN, a NaN in the same places).  w, b, grad_logits and every output stay
 * fp32; the scratch is the same (unet_head_reserve does not depend on the type).  The aligned path (feat on 16
 * bytes, H W divisible by 8) reads 16 bytes, 8 pixels, per lane; other bases and sizes read the same values with
 * narrower loads.  Every other rule is that of the untyped calls: argument and alias checks before any HIP call,
 * stream order, capturable after unet_head_reserve (UNET_ESTATE for growth under capture), 64-bit indices. */
int unet_head_forward_typed(unet_handle* h, const void* feat, int feat_dtype, const float* w, const float* b,
                            float* logits, int N, int C, int H, int W, void* hip_stream);
int unet_head_backward_typed(unet_handle* h, const void* feat, int feat_dtype, const float* grad_logits,
                             const float* w, float* grad_w, float* grad_b, float* grad_feat,
                             int N, int C, int H, int W, void* hip_stream);

/* One training step of the head from ONE pass over the stored features: what
 * unet_head_forward_typed, unet_loss_grad, unet_head_backward_typed and an AdamW step compute in turn, without the
 * logits or their gradient ever reaching memory, without a gathered copy of a shuffled batch, in three launches.
 *   feat: the base of the whole feature cache, device [P][64][H][W] as feat_dtype (as unet_head_forward_typed);
 *   target: the base of the cache's masks, device, [P][C][H][W] fp32 or [P][H][W][C] uint8 per target_kind (UNET_TGT_*);
 *   pages: device int32 [N], the page of each of the N batch slots (any order, repeats allowed), or NULL: slot n is
 *   page n (then N <= P).  A page outside [0, P) is never used as an address: it makes every output of the call NaN.
 * Arithmetic: the logits are those of unet_head_forward, bit for bit; per element the fp32 chain of unet_score and
 * the focal branch of unet_loss_grad's backward, op by op, for an upstream gradient of 1; everything after that in
 * fp64: the gradient at a logit is (g0 e + A t + B) s, s = (1 - p) p, with A, B the Dice coefficients of its plane
 * by unet_loss_grad's formula, so
 *   grad_w[c][k] = sum_n ( g0 F[n][c][k] + A[n][c] T[n][c][k] + B[n][c] S[n][c][k] ),  grad_b with feat == 1,
 *   F, T, S = sum_p of (e s, t s, s) feat[n][k][p]
 * over a summation tree that depends on (N, H W) only, each gradient rounded to fp32 once.  loss is InvoiceLoss as
 * unet_loss_grad returns it.  Bitwise reproducible, independent of pointer alignment, and for 16-bit features the
 * bits of the call on the widened tensor.
 * opt == NULL: no update; w and b are only read, grad_w [C][64] and grad_b [C] are required.  opt != NULL: state
 * (device fp32, m_w [C][64], m_b [C], v_w [C][64], v_b [C]: 2 (64 C + C) floats, zero before step 1) is required,
 * grad_w / grad_b become optional as a pair, and w, b and state are updated as torch.optim.AdamW does:
 *   theta *= 1 - lr weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   theta -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * on the fp32-rounded gradient, evaluated in fp64, m, v and theta rounded to fp32 once each.  opt is read at the
 * call (a captured step replays with the lr and step it was captured with).
 * IEEE propagation, nothing special-cased: a NaN feature makes the loss, every gradient and every updated value
 * NaN (it reaches all logits of its pixel, hence every plane's Dice coefficients of its page); a NaN target of class
 * c makes the loss and grad_w[c][:], grad_b[c] (and the updated row c) NaN and leaves the other classes' bits.
 * Stream-ordered after the handle's previous call; no host round trip; capturable after unet_head_step_reserve
 * (the scratch, N * ceil(H W / 4096) * 199 C doubles, grows synchronously otherwise; UNET_ESTATE for growth under
 * capture).  Bad arguments -- NULL feat, target, cfg, w, b or loss, an output that is feat, target, w or b -- are
 * UNET_EINVAL before any HIP call. */
typedef struct unet_adamw_config {
  float lr, beta1, beta2, eps, weight_decay;   /* torch.optim.AdamW's: 1e-3, 0.9, 0.999, 1e-8, 1e-2 */
  int step;                                    /* 1-based: the count of this update */
} unet_adamw_config;

/* Size the handle's head-step scratch (its own allocation: unet_workspace_bytes, unet_reserve and the other scratch
 * buffers are unaffected) for steps of up to N batch slots of H x W with up to 4 classes.  Allocating waits for the
 * handle's queued work. */
int unet_head_step_reserve(unet_handle* h, int N, int H, int W);

int unet_head_step(unet_handle* h, const void* feat, int feat_dtype, const void* target, int target_kind,
                   const int32_t* pages, int P, int N, int C, int H, int W, const unet_loss_config* cfg,
                   float* w, float* b, float* loss, float* grad_w, float* grad_b,
                   const unet_adamw_config* opt, float* state, void* hip_stream);

/* Score the head from the stored features: what unet_head_forward_typed followed by
 * unet_score computes, from ONE pass over the feature cache, without the logits ever reaching memory and without a
 * gathered copy of the pages scored, in two launches.  Validation of a head fitted with unet_head_step.
 *   feat, feat_dtype, target, target_kind, pages, P, N: as in unet_head_step -- the bases of the whole cache
 *   [P][64][H][W] and of its masks, and the page of each of the N slots (device int32 [N], any order, repeats
 *   allowed; NULL: slot n is page n, then N <= P).
 *   w: device fp32 [C][64], b: device fp32 [C]; only read.  No weights need to be loaded into the handle.
 *   thresholds, entries, sweep_probs, K, hist: as in unet_score; entries is [N][C] and hist [N][C][2][K+1], by slot.
 * Arithmetic: the logits are those of unet_head_forward, bit for bit, 16-bit features widened exactly; per element
 * the fp32 chain of unet_score, op by op; the four sums in fp64 over a summation tree that depends on H W only, the
 * counts and bins as integers.  So n_pred, n_tgt, n_both, n_px and every bin equal unet_score's on those logits, and
 * the sums agree to fp64 rounding (another tree).  An entry is bitwise reproducible and independent of N, of the
 * slot, of the other slots' pages, of pointer alignment and of the feature type.
 * A page outside [0, P) is never used as an address: that slot's four sums are NaN, its counts and bins zero and its
 * n_px = H W; the other slots are unaffected.  A NaN feature makes the four sums of every class of its page NaN and
 * counts as not predicted; a NaN target of class c reaches that class's sums only.
 * Stream-ordered after the handle's previous call; no host round trip; capturable after unet_head_score_reserve (the
 * scratch, N C ceil(H W / 4096) partials of 48 bytes and with a sweep as many rows of 2 (K + 1) uint32, grows
 * synchronously otherwise; UNET_ESTATE for growth under capture).  unet_workspace_bytes is unaffected.  Bad arguments
 * -- NULL feat, w, b, target or entries, entries or hist aliasing an input -- are UNET_EINVAL before any HIP call. */
int unet_head_score_reserve(unet_handle* h, int N, int H, int W, int K);

int unet_head_score(unet_handle* h, const void* feat, int feat_dtype, const float* w, const float* b,
                    const void* target, int target_kind, const int32_t* pages, int P, int N, int C, int H, int W,
                    const float* thresholds, unet_score_entry* entries, const float* sweep_probs, int K,
                    int64_t* hist, void* hip_stream);

int unet_destroy(unet_handle* h);

/* Stand-alone DoubleConv block: unet_model.DoubleConv(in_ch, out_ch).forward (unet_model.py:6-20,
 * conv3x3 + BN + ReLU twice, padding 1) on its own, on the network's kernels: the first-conv kernel
 * for in_ch 1 or 3 (out_ch 64), the 8-wave MFMA rings (16-bit plans; MIXED = fp16 up to 128 output
 * channels, bf16 beyond, as the network's levels) or the fp32 LDS-halo kernels.  Supported: in_ch in
 * {1, 3} with out_ch 64, or in_ch a multiple of 32 with out_ch a multiple of 64 (on the 16-bit plans:
 * out_ch 64 or a multiple of 128, the ring tiles) -- every block of the reference UNet (UNET_ESHAPE
 * otherwise, at unet_block_create).  Any H, W >= 1.
 * unet_block_load_weights takes the block's own 14 state_dict keys (net.0.weight, net.0.bias,
 * net.1.weight / bias / running_mean / running_var / num_batches_tracked, and net.3 / net.4 alike;
 * BN folded, eps 1e-5).  x / y: device fp32 NCHW [N][in_ch][H][W] / [N][out_ch][H][W]; the workspace
 * is sized by unet_block_reserve (unet_block_forward never allocates). */
typedef struct unet_block unet_block;
typedef struct unet_block_config {
  int in_ch, out_ch;   /* DoubleConv(in_ch, out_ch) */
  int dtype;           /* UNET_DTYPE_* */
  int device;          /* HIP device ordinal */
} unet_block_config;
int unet_block_create(const unet_block_config* cfg, unet_block** out);
int unet_block_load_weights(unet_block* b, const unet_tensor_view* tensors, int n);
int unet_block_reserve(unet_block* b, int N, int H, int W);
int unet_block_forward(unet_block* b, const float* x, float* y, int N, int H, int W, void* hip_stream);
/* unet_debug_fill for a block: its workspace (unet_block_reserve), under the same rules. */
int unet_block_debug_fill(unet_block* b, int byte, void* hip_stream);
/* unet_launch_walk_at for a block's conv i (0 = net.0, 1 = net.3) at N x H x W. */
int unet_block_launch_walk_at(const unet_block* b, int i, int N, int H, int W, int* slots, int* items);
int unet_block_destroy(unet_block* b);

/* Message of the last error on this thread ("" if none). */
const char* unet_last_error(void);

int unet_abi_version(void);

/* Logit cut of a probability threshold: for every fp32 logit x,
 *   (1 / (1 + expf(-x)) > thr)  ==  (x > unet_logit_cut(thr)).
 * The masks epilogue thresholds logits with it (inference.py:72-78 thresholds
 * torch.sigmoid(logits)); host-only, no device call. */
float unet_logit_cut(float thr);

#ifdef __cplusplus
}
#endif
#endif /* UNET_MI355X_H */
