// The output head on its own: out_conv = Conv2d(64, C, 1) (unet_model.py:50) forward and backward over a stored
// NCHW feature map (unet_head_forward / unet_head_backward and their _typed forms, include/unet_mi355x.h) -- what
// fine-tuning the head on a frozen backbone needs.  The weights are device pointers (torch parameters), never the
// handle's.  The features are fp32, fp16 or bf16 (the kernels that read them are templates on the type); every
// 16-bit feature is widened to fp32 once, exactly, and all arithmetic below is on fp32 values, so a call on 16-bit
// features returns the bits of the fp32 call on the widened tensor.  Everything else is fp32.
//
//   forward    logit[n][c][p] = b[c] + sum_k w[c][k] feat[n][k][p]      one fp32 fmaf chain from the bias, k ascending
//   grad_feat  gf[n][k][p]    = sum_c w[c][k] g[n][c][p]                the product of c = 0, then fmaf, c ascending
//   grad_w     gw[c][k]       = sum_{n,p} g[n][c][p] feat[n][k][p]      fp64 products and sums, rounded to fp32 once
//   grad_b     gb[c]          = sum_{n,p} g[n][c][p]                    likewise
//
// Forward and grad_feat: a thread owns the pixels of one 16-byte load -- 4 consecutive pixels of one image, 8 in
// the forward over 16-bit features (an 8-byte load per lane runs at 0.54-0.70 of the 16-byte rate) -- and walks the
// 64 channel rows; 16-byte loads and stores where every row is aligned, scalar ones otherwise and at the plane's
// tail -- the same chain on the same values either way, so results do not depend on alignment, on N, on the image's
// place in the batch or on the pixels a thread owns.
//
// grad_w / grad_b: two launches, no float atomics, no counters (DESIGN.md sections 9-11).
//   1. head_partial_kernel: one block per span of kHeadSpan pixels of one image.  Per stage it brings kStage
//      pixels of the 64 feature rows (as fp32, whatever their type in memory: 16-bit rows are loaded 8 pixels per
//      lane and widened in registers) and of the C gradient rows (widened to fp64 once) into LDS; thread
//      (c, k) = (wave, lane) adds g[c][p] * feat[k][p] into four fp64 accumulators (pixel p mod 4), combined as
//      (a0 + a1) + (a2 + a3).  An fp32 x fp32 product is exact in fp64, so contraction to an fma changes nothing.
//      Wave c's lanes 0..31 also add up g[c] (4 pixels of every stage each) and combine by a shuffle tree.  The
//      block stores its 64 C + C partials into its own column of the slabs.  Pixels past the plane's end are staged
//      as zero in both operands.  No class is padded: waves c >= C only stage.
//   2. head_sum_kernel: one block per output sums that output's slab entries -- thread t the entries t, t + 256,
//      ... in ascending order, then a fixed shuffle / LDS tree -- and rounds to fp32.
// A feature NaN therefore reaches only the accumulators of its own k, a gradient NaN only those of its own c.
#include "unet_head.h"

namespace unet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 128;                 // pixels per LDS stage
constexpr int kRow = kStage + 4;            // padded feature row (floats): the 16-byte slots of lanes k, k + 1 differ by 33
constexpr int kStageQuads = kStage / 4;     // 16-byte groups per row and stage
constexpr int kFeatQuads = kHeadK * kStageQuads / kThreads;   // feature quads staged per thread and stage
static_assert(kHeadSpan % kStage == 0, "a span is a whole number of stages");
static_assert(kHeadK * kStageQuads == kFeatQuads * kThreads, "the stage's quads divide among the threads");
constexpr int kStageOcts = kStage / 8;      // 16-byte groups of 16-bit features per row and stage
constexpr int kFeatOcts = kHeadK * kStageOcts / kThreads;     // 16-bit feature groups staged per thread and stage
static_assert(kHeadFwdTile == 4 * kThreads, "a forward tile is one quad per thread");
static_assert(kHeadK * kStageOcts == kFeatOcts * kThreads && kStageOcts == 16 && kHeadK * kStageOcts == 1024,
              "group16_of's bit layout");
static_assert(kWaves == 4 && kStageQuads == 32, "thread (c, k) = (wave, lane); bias lanes 0..31");

__device__ inline double shfl_down_f64(double v, int off) { return __shfl_down(v, off, 64); }

// 4 consecutive floats at p, of which `left` >= 1 lie inside the plane (the rest read as 0)
__device__ inline float4 load_quad(const float* __restrict__ p, bool vec, long long left) {
  if (vec && left >= 4) return *reinterpret_cast<const float4*>(p);
  float4 v;
  v.x = p[0];
  v.y = left > 1 ? p[1] : 0.0f;
  v.z = left > 2 ? p[2] : 0.0f;
  v.w = left > 3 ? p[3] : 0.0f;
  return v;
}

__device__ inline void store_quad(float* __restrict__ p, bool vec, long long left, float4 v) {
  if (vec && left >= 4) {
    *reinterpret_cast<float4*>(p) = v;
    return;
  }
  p[0] = v.x;
  if (left > 1) p[1] = v.y;
  if (left > 2) p[2] = v.z;
  if (left > 3) p[3] = v.w;
}

// every 16-byte group (`group` elements: 4 fp32, 8 fp16 / bf16) of every row of a [rows][HW] tensor starts on 16 bytes
__device__ inline bool rows_aligned(const void* base, long long HW, int group = 4) {
  return ((uintptr_t)base & 15) == 0 && (HW & (group - 1)) == 0;
}

// Pixels of one 16-byte load of features stored as T
template <typename T>
constexpr int kGroup = 16 / (int)sizeof(T);

// fp16 / bf16 bits -> fp32, exact (subnormals, signed zeros, infinities and NaNs included): one conversion for
// fp16, a 16-bit shift for bf16
template <typename T>
__device__ inline float widen(unsigned v);
template <>
__device__ inline float widen<_Float16>(unsigned v) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)v);
}
template <>
__device__ inline float widen<__bf16>(unsigned v) {
  return __uint_as_float(v << 16);
}

// 8 consecutive 16-bit elements at p as stored, of which `left` >= 1 lie inside the plane (the rest read as +0)
__device__ inline uint4 load_oct(const unsigned short* __restrict__ p, bool vec, long long left) {
  if (vec && left >= 8) return *reinterpret_cast<const uint4*>(p);
  unsigned e[8];
  e[0] = p[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) e[i] = left > i ? p[i] : 0u;
  return make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
}

// the 4 pixels of two words of an oct, widened
template <typename T>
__device__ inline float4 widen_quad(unsigned lo, unsigned hi) {
  return make_float4(widen<T>(lo & 0xFFFFu), widen<T>(lo >> 16), widen<T>(hi & 0xFFFFu), widen<T>(hi >> 16));
}

// the kGroup<T> consecutive features at p as fp32, zero past the plane
__device__ inline void load_group(float (&x)[4], const float* __restrict__ p, bool vec, long long left) {
  const float4 v = load_quad(p, vec, left);
  x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
template <typename T>
__device__ inline void load_group(float (&x)[8], const T* __restrict__ p, bool vec, long long left) {
  const uint4 r = load_oct(reinterpret_cast<const unsigned short*>(p), vec, left);
  const float4 a = widen_quad<T>(r.x, r.y), b = widen_quad<T>(r.z, r.w);
  x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
  x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
}

template <typename T, int C>
__global__ __launch_bounds__(kThreads) void head_forward_kernel(const T* __restrict__ feat,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ b,
                                                                float* __restrict__ logits, long long HW,
                                                                long long tiles) {
  constexpr int G = kGroup<T>;   // pixels per thread; a tile is G * kThreads pixels
  const long long n = (long long)blockIdx.x / tiles;
  const long long p = ((long long)blockIdx.x % tiles) * (G * kThreads) + G * (long long)threadIdx.x;
  if (p >= HW) return;
  const long long left = HW - p;
  const T* fp = feat + n * kHeadK * HW + p;
  float* lp = logits + n * C * HW + p;
  const bool f_vec = rows_aligned(feat, HW, G), l_vec = rows_aligned(logits, HW);
  float acc[C][G];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float bc = b[c];
#pragma unroll
    for (int i = 0; i < G; ++i) acc[c][i] = bc;
  }
#pragma unroll 8
  for (int k = 0; k < kHeadK; ++k) {
    float x[G];
    load_group(x, fp + (long long)k * HW, f_vec, left);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float wk = w[c * kHeadK + k];
#pragma unroll
      for (int i = 0; i < G; ++i) acc[c][i] = fmaf(wk, x[i], acc[c][i]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int q = 0; q < G; q += 4)
      if (q == 0 || left > q)
        store_quad(lp + (long long)c * HW + q, l_vec, left - q,
                   make_float4(acc[c][q], acc[c][q + 1], acc[c][q + 2], acc[c][q + 3]));
  }
}

template <int C>
__global__ __launch_bounds__(kThreads) void head_grad_feat_kernel(const float* __restrict__ g,
                                                                  const float* __restrict__ w,
                                                                  float* __restrict__ gf, long long HW,
                                                                  long long tiles) {
  const long long n = (long long)blockIdx.x / tiles;
  const long long p = ((long long)blockIdx.x % tiles) * kHeadFwdTile + 4 * (long long)threadIdx.x;
  if (p >= HW) return;
  const long long left = HW - p;
  const float* gp = g + n * C * HW + p;
  float* op = gf + n * kHeadK * HW + p;
  const bool g_vec = rows_aligned(g, HW), o_vec = rows_aligned(gf, HW);
  float4 gv[C];
#pragma unroll
  for (int c = 0; c < C; ++c) gv[c] = load_quad(gp + (long long)c * HW, g_vec, left);
#pragma unroll 8
  for (int k = 0; k < kHeadK; ++k) {
    const float w0 = w[k];
    float4 o = make_float4(w0 * gv[0].x, w0 * gv[0].y, w0 * gv[0].z, w0 * gv[0].w);
#pragma unroll
    for (int c = 1; c < C; ++c) {
      const float wk = w[c * kHeadK + k];
      o.x = fmaf(wk, gv[c].x, o.x);
      o.y = fmaf(wk, gv[c].y, o.y);
      o.z = fmaf(wk, gv[c].z, o.z);
      o.w = fmaf(wk, gv[c].w, o.w);
    }
    store_quad(op + (long long)k * HW, o_vec, left, o);
  }
}

// One stage's features in a thread's registers, between its global loads and its LDS stores, by their type in
// memory.  Either way the LDS image is the same: s_f[row * kRow + pixel] as fp32, zero past the plane.
// fp32: kFeatQuads quads; 32 consecutive lanes take one row's 32 quads.
template <typename T>
struct StageFeat {
  float4 r[kFeatQuads];
  __device__ __forceinline__ void fetch(const float* __restrict__ fbase, long long HW, long long ps, int tid,
                                        bool f_vec) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int q = 0; q < kFeatQuads; ++q) {
      const int idx = q * kThreads + tid;
      const long long p = ps + 4 * (idx & 31);
      r[q] = p < HW ? load_quad(fbase + (long long)(idx >> 5) * HW + p, f_vec, HW - p) : zero;
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ s_f, int tid) const {
#pragma unroll
    for (int q = 0; q < kFeatQuads; ++q) {
      const int idx = q * kThreads + tid;
      *reinterpret_cast<float4*>(&s_f[(idx >> 5) * kRow + 4 * (idx & 31)]) = r[q];
    }
  }
};

// fp16 / bf16: kFeatOcts groups of 8 pixels as loaded (16 bytes per lane, half the registers of the fp32 stage),
// widened when they are stored.  Group idx of the stage's 1024 is (row, oct) with lanes 0..3 of every 8 on four
// consecutive octs of an even row and lanes 4..7 on the same octs of the row below: a wave's load still covers
// whole 256-byte rows, and each of the two ds_write_b128 of an oct is conflict-free -- the 8 lanes one LDS cycle
// serves write quads 8 floats apart (banks 0, 8, 16, 24 of 32) in rows one stride (132 floats: 4 banks) apart.  With
// 16 consecutive lanes on one row, lanes l and l + 4 of every 8 would share their banks.
__device__ __forceinline__ void group16_of(int idx, int& row, int& oct) {
  row = ((idx >> 5) << 1) | ((idx >> 2) & 1);
  oct = (((idx >> 3) & 3) << 2) | (idx & 3);
}

template <typename T>
struct StageFeat16 {
  uint4 r[kFeatOcts];
  __device__ __forceinline__ void fetch(const T* __restrict__ fbase, long long HW, long long ps, int tid, bool f_vec) {
    const unsigned short* base = reinterpret_cast<const unsigned short*>(fbase);
#pragma unroll
    for (int q = 0; q < kFeatOcts; ++q) {
      int row, oct;
      group16_of(q * kThreads + tid, row, oct);
      const long long p = ps + 8 * oct;
      r[q] = p < HW ? load_oct(base + (long long)row * HW + p, f_vec, HW - p) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ s_f, int tid) const {
#pragma unroll
    for (int q = 0; q < kFeatOcts; ++q) {
      int row, oct;
      group16_of(q * kThreads + tid, row, oct);
      float4* d = reinterpret_cast<float4*>(&s_f[row * kRow + 8 * oct]);
      d[0] = widen_quad<T>(r[q].x, r[q].y);
      d[1] = widen_quad<T>(r[q].z, r[q].w);
    }
  }
};
template <>
struct StageFeat<_Float16> : StageFeat16<_Float16> {};
template <>
struct StageFeat<__bf16> : StageFeat16<__bf16> {};

// one stage's global loads of a thread: its feature groups and (stage_g) its gradient quad, zero past the plane
template <typename T>
__device__ __forceinline__ void stage_fetch(StageFeat<T>& rf, float4& rg, const T* __restrict__ fbase,
                                            const float* __restrict__ gbase, long long HW, long long ps, int tid,
                                            bool stage_g, bool f_vec, bool g_vec) {
  rf.fetch(fbase, HW, ps, tid, f_vec);
  if (stage_g) {
    const long long p = ps + 4 * (tid & 31);
    rg = p < HW ? load_quad(gbase + (long long)(tid >> 5) * HW + p, g_vec, HW - p)
                : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// slabs: [64 C + C][nslabs] fp64, this block's column = its slab index
template <typename T>
__global__ __launch_bounds__(kThreads) void head_partial_kernel(const T* __restrict__ feat,
                                                                const float* __restrict__ g, int C, long long HW,
                                                                long long spans, long long nslabs,
                                                                double* __restrict__ slabs) {
  __shared__ __attribute__((aligned(16))) float s_f[kHeadK * kRow];
  __shared__ __attribute__((aligned(16))) double s_g[kWaves * kStage];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long slab = blockIdx.x;
  const long long n = slab / spans;
  const long long p0 = (slab % spans) * kHeadSpan;
  const long long span_len = HW - p0 < kHeadSpan ? HW - p0 : kHeadSpan;
  const int stages = (int)((span_len + kStage - 1) / kStage);
  const T* fbase = feat + n * kHeadK * HW;
  const float* gbase = g + n * C * HW;
  const bool f_vec = rows_aligned(feat, HW, kGroup<T>), g_vec = rows_aligned(g, HW);
  const int g_row = tid >> 5, g_quad = tid & 31;   // the gradient quad this thread stages (g_row < C)

  StageFeat<T> rf;
  float4 rg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, bias = 0.0;
  stage_fetch(rf, rg, fbase, gbase, HW, p0, tid, g_row < C, f_vec, g_vec);
  for (int st = 0; st < stages; ++st) {
    rf.store(s_f, tid);
    if (g_row < C) {
      double* d = &s_g[g_row * kStage + 4 * g_quad];
      d[0] = (double)rg.x;
      d[1] = (double)rg.y;
      d[2] = (double)rg.z;
      d[3] = (double)rg.w;
    }
    __syncthreads();
    if (st + 1 < stages)   // in flight under this stage's sums
      stage_fetch(rf, rg, fbase, gbase, HW, p0 + (long long)(st + 1) * kStage, tid, g_row < C, f_vec, g_vec);
    if (wave < C) {
      const float* fr = &s_f[lane * kRow];
      const double* gr = &s_g[wave * kStage];
#pragma unroll 8
      for (int j = 0; j < kStageQuads; ++j) {
        const float4 f = *reinterpret_cast<const float4*>(fr + 4 * j);
        const double2 g01 = *reinterpret_cast<const double2*>(gr + 4 * j);
        const double2 g23 = *reinterpret_cast<const double2*>(gr + 4 * j + 2);
        a0 += (double)f.x * g01.x;
        a1 += (double)f.y * g01.y;
        a2 += (double)f.z * g23.x;
        a3 += (double)f.w * g23.y;
      }
      if (lane < kStageQuads) {
        const double2 g01 = *reinterpret_cast<const double2*>(gr + 4 * lane);
        const double2 g23 = *reinterpret_cast<const double2*>(gr + 4 * lane + 2);
        bias += g01.x;
        bias += g01.y;
        bias += g23.x;
        bias += g23.y;
      }
    }
    __syncthreads();
  }
  if (wave < C) {
    slabs[((long long)wave * kHeadK + lane) * nslabs + slab] = (a0 + a1) + (a2 + a3);
    for (int off = 32; off > 0; off >>= 1) bias += shfl_down_f64(bias, off);
    if (lane == 0) slabs[((long long)C * kHeadK + wave) * nslabs + slab] = bias;
  }
}

// block o < 64 C: grad_w[o]; block 64 C + c: grad_b[c]
__global__ __launch_bounds__(kThreads) void head_sum_kernel(const double* __restrict__ slabs, int C, long long nslabs,
                                                            float* __restrict__ grad_w, float* __restrict__ grad_b) {
  __shared__ double s_sum[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int o = blockIdx.x;
  const double* row = slabs + (long long)o * nslabs;
  double a = 0.0;
  for (long long i = tid; i < nslabs; i += kThreads) a += row[i];   // a fixed order: thread, then wave, then block
  for (int off = 32; off > 0; off >>= 1) a += shfl_down_f64(a, off);
  if (lane == 0) s_sum[wave] = a;
  __syncthreads();
  if (tid == 0) {
    double t = s_sum[0];
    for (int v = 1; v < kWaves; ++v) t += s_sum[v];
    if (o < C * kHeadK)
      grad_w[o] = (float)t;
    else
      grad_b[o - C * kHeadK] = (float)t;
  }
}

template <typename T, int C>
hipError_t launch_forward(unsigned grid, const T* feat, const float* w, const float* b, float* logits, long long HW,
                          long long tiles, hipStream_t s) {
  hipLaunchKernelGGL((head_forward_kernel<T, C>), dim3(grid), dim3(kThreads), 0, s, feat, w, b, logits, HW, tiles);
  return hipGetLastError();
}

// tiles of G * kThreads pixels: never more than head_tiles(HW), the count the callers check against 31 bits
template <typename T>
hipError_t forward_of(const void* feat, const float* w, const float* b, float* logits, long long N, int C,
                      long long HW, hipStream_t s) {
  const long long tile = (long long)kGroup<T> * kThreads, tiles = (HW + tile - 1) / tile;
  const unsigned grid = (unsigned)(N * tiles);
  const T* f = static_cast<const T*>(feat);
  switch (C) {
    case 1: return launch_forward<T, 1>(grid, f, w, b, logits, HW, tiles, s);
    case 2: return launch_forward<T, 2>(grid, f, w, b, logits, HW, tiles, s);
    case 3: return launch_forward<T, 3>(grid, f, w, b, logits, HW, tiles, s);
    case 4: return launch_forward<T, 4>(grid, f, w, b, logits, HW, tiles, s);
    default: return hipErrorInvalidValue;
  }
}

template <typename T>
hipError_t launch_partial(const void* feat, const float* g, int C, long long HW, long long nslabs, double* slabs,
                          hipStream_t s) {
  hipLaunchKernelGGL(head_partial_kernel<T>, dim3((unsigned)nslabs), dim3(kThreads), 0, s,
                     static_cast<const T*>(feat), g, C, HW, head_spans(HW), nslabs, slabs);
  return hipGetLastError();
}

template <int C>
hipError_t launch_grad_feat(unsigned grid, const float* g, const float* w, float* gf, long long HW, long long tiles,
                            hipStream_t s) {
  hipLaunchKernelGGL((head_grad_feat_kernel<C>), dim3(grid), dim3(kThreads), 0, s, g, w, gf, HW, tiles);
  return hipGetLastError();
}

}  // namespace

size_t head_scratch_bytes(long long N, long long hw, int C) {
  return (size_t)(N * head_spans(hw)) * (size_t)(kHeadK * C + C) * sizeof(double);
}

hipError_t launch_head_forward(const void* feat, int feat_dtype, const float* w, const float* b, float* logits, int N,
                               int C, int H, int W, hipStream_t s) {
  const long long HW = (long long)H * W;
  if (N * head_tiles(HW) > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  switch (feat_dtype) {
    case UNET_DTYPE_F32: return forward_of<float>(feat, w, b, logits, N, C, HW, s);
    case UNET_DTYPE_F16: return forward_of<_Float16>(feat, w, b, logits, N, C, HW, s);
    case UNET_DTYPE_BF16: return forward_of<__bf16>(feat, w, b, logits, N, C, HW, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_head_backward(const void* feat, int feat_dtype, const float* g, const float* w, float* grad_w,
                                float* grad_b, float* grad_feat, int N, int C, int H, int W, void* scratch,
                                hipStream_t s) {
  const long long HW = (long long)H * W, tiles = head_tiles(HW), nslabs = N * head_spans(HW);
  if (N * tiles > 0x7FFFFFFFLL || C < 1 || C > 4) return hipErrorInvalidValue;
  if (feat_dtype != UNET_DTYPE_F32 && feat_dtype != UNET_DTYPE_F16 && feat_dtype != UNET_DTYPE_BF16)
    return hipErrorInvalidValue;
  if (grad_w) {
    double* slabs = static_cast<double*>(scratch);
    hipError_t e = feat_dtype == UNET_DTYPE_F32   ? launch_partial<float>(feat, g, C, HW, nslabs, slabs, s)
                   : feat_dtype == UNET_DTYPE_F16 ? launch_partial<_Float16>(feat, g, C, HW, nslabs, slabs, s)
                                                  : launch_partial<__bf16>(feat, g, C, HW, nslabs, slabs, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_sum_kernel, dim3((unsigned)(kHeadK * C + C)), dim3(kThreads), 0, s, slabs, C, nslabs,
                       grad_w, grad_b);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (!grad_feat) return hipSuccess;
  const unsigned grid = (unsigned)(N * tiles);
  switch (C) {
    case 1: return launch_grad_feat<1>(grid, g, w, grad_feat, HW, tiles, s);
    case 2: return launch_grad_feat<2>(grid, g, w, grad_feat, HW, tiles, s);
    case 3: return launch_grad_feat<3>(grid, g, w, grad_feat, HW, tiles, s);
    default: return launch_grad_feat<4>(grid, g, w, grad_feat, HW, tiles, s);
  }
}

}  // namespace unet
