// The output head on its own: out_conv = Conv2d(64, C, 1) (unet_model.py:50) forward and backward over a stored
// fp32 NCHW feature map (unet_head_forward / unet_head_backward, include/unet_mi355x.h) -- what fine-tuning the
// head on a frozen backbone needs.  The weights are device pointers (torch parameters), never the handle's.
//
//   forward    logit[n][c][p] = b[c] + sum_k w[c][k] feat[n][k][p]      one fp32 fmaf chain from the bias, k ascending
//   grad_feat  gf[n][k][p]    = sum_c w[c][k] g[n][c][p]                the product of c = 0, then fmaf, c ascending
//   grad_w     gw[c][k]       = sum_{n,p} g[n][c][p] feat[n][k][p]      fp64 products and sums, rounded to fp32 once
//   grad_b     gb[c]          = sum_{n,p} g[n][c][p]                    likewise
//
// Forward and grad_feat: a thread owns 4 consecutive pixels of one image and walks the 64 channel rows; 16-byte
// loads and stores where every row is aligned, scalar ones otherwise and at the plane's tail -- the same chain on
// the same values either way, so results do not depend on alignment, on N or on the image's place in the batch.
//
// grad_w / grad_b: two launches, no float atomics, no counters (DESIGN.md sections 9-11).
//   1. head_partial_kernel: one block per span of kHeadSpan pixels of one image.  Per stage it brings kStage
//      pixels of the 64 feature rows (fp32) and of the C gradient rows (widened to fp64 once) into LDS; thread
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
static_assert(kHeadFwdTile == 4 * kThreads, "a forward tile is one quad per thread");
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

// every quad of every row of a [rows][HW] tensor starts on 16 bytes
__device__ inline bool rows_aligned(const void* base, long long HW) {
  return ((uintptr_t)base & 15) == 0 && (HW & 3) == 0;
}

template <int C>
__global__ __launch_bounds__(kThreads) void head_forward_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ b,
                                                                float* __restrict__ logits, long long HW,
                                                                long long tiles) {
  const long long n = (long long)blockIdx.x / tiles;
  const long long p = ((long long)blockIdx.x % tiles) * kHeadFwdTile + 4 * (long long)threadIdx.x;
  if (p >= HW) return;
  const long long left = HW - p;
  const float* fp = feat + n * kHeadK * HW + p;
  float* lp = logits + n * C * HW + p;
  const bool f_vec = rows_aligned(feat, HW), l_vec = rows_aligned(logits, HW);
  float acc[C][4];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float bc = b[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[c][i] = bc;
  }
#pragma unroll 8
  for (int k = 0; k < kHeadK; ++k) {
    const float4 x = load_quad(fp + (long long)k * HW, f_vec, left);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float wk = w[c * kHeadK + k];
      acc[c][0] = fmaf(wk, x.x, acc[c][0]);
      acc[c][1] = fmaf(wk, x.y, acc[c][1]);
      acc[c][2] = fmaf(wk, x.z, acc[c][2]);
      acc[c][3] = fmaf(wk, x.w, acc[c][3]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    store_quad(lp + (long long)c * HW, l_vec, left, make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]));
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

// one stage's global loads of a thread: its feature quads and (stage_g) its gradient quad, zero past the plane
__device__ __forceinline__ void stage_fetch(float4 (&rf)[kFeatQuads], float4& rg, const float* __restrict__ fbase,
                                            const float* __restrict__ gbase, long long HW, long long ps, int tid,
                                            bool stage_g, bool f_vec, bool g_vec) {
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int q = 0; q < kFeatQuads; ++q) {
    const int idx = q * kThreads + tid;
    const long long p = ps + 4 * (idx & 31);
    rf[q] = p < HW ? load_quad(fbase + (long long)(idx >> 5) * HW + p, f_vec, HW - p) : zero;
  }
  if (stage_g) {
    const long long p = ps + 4 * (tid & 31);
    rg = p < HW ? load_quad(gbase + (long long)(tid >> 5) * HW + p, g_vec, HW - p) : zero;
  }
}

// slabs: [64 C + C][nslabs] fp64, this block's column = its slab index
__global__ __launch_bounds__(kThreads) void head_partial_kernel(const float* __restrict__ feat,
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
  const float* fbase = feat + n * kHeadK * HW;
  const float* gbase = g + n * C * HW;
  const bool f_vec = rows_aligned(feat, HW), g_vec = rows_aligned(g, HW);
  const int g_row = tid >> 5, g_quad = tid & 31;   // the gradient quad this thread stages (g_row < C)

  float4 rf[kFeatQuads];
  float4 rg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, bias = 0.0;
  stage_fetch(rf, rg, fbase, gbase, HW, p0, tid, g_row < C, f_vec, g_vec);
  for (int st = 0; st < stages; ++st) {
#pragma unroll
    for (int q = 0; q < kFeatQuads; ++q) {
      const int idx = q * kThreads + tid;
      *reinterpret_cast<float4*>(&s_f[(idx >> 5) * kRow + 4 * (idx & 31)]) = rf[q];
    }
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

template <int C>
hipError_t launch_forward(unsigned grid, const float* feat, const float* w, const float* b, float* logits,
                          long long HW, long long tiles, hipStream_t s) {
  hipLaunchKernelGGL((head_forward_kernel<C>), dim3(grid), dim3(kThreads), 0, s, feat, w, b, logits, HW, tiles);
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

hipError_t launch_head_forward(const float* feat, const float* w, const float* b, float* logits, int N, int C, int H,
                               int W, hipStream_t s) {
  const long long HW = (long long)H * W, tiles = head_tiles(HW);
  if (N * tiles > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(N * tiles);
  switch (C) {
    case 1: return launch_forward<1>(grid, feat, w, b, logits, HW, tiles, s);
    case 2: return launch_forward<2>(grid, feat, w, b, logits, HW, tiles, s);
    case 3: return launch_forward<3>(grid, feat, w, b, logits, HW, tiles, s);
    case 4: return launch_forward<4>(grid, feat, w, b, logits, HW, tiles, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_head_backward(const float* feat, const float* g, const float* w, float* grad_w, float* grad_b,
                                float* grad_feat, int N, int C, int H, int W, void* scratch, hipStream_t s) {
  const long long HW = (long long)H * W, tiles = head_tiles(HW), nslabs = N * head_spans(HW);
  if (N * tiles > 0x7FFFFFFFLL || C < 1 || C > 4) return hipErrorInvalidValue;
  if (grad_w) {
    double* slabs = static_cast<double*>(scratch);
    hipLaunchKernelGGL(head_partial_kernel, dim3((unsigned)nslabs), dim3(kThreads), 0, s, feat, g, C, HW,
                       head_spans(HW), nslabs, slabs);
    hipError_t e = hipGetLastError();
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
