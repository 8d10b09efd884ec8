// Scoring of logits against ground-truth masks on the device (unet_score, include/unet_mi355x.h): per
// (image, class) the sums and counts from which the host assembles the reference's InvoiceLoss (train.py:18-59),
// Dice, IoU and a threshold sweep.
//
// Two launches, no cross-block hand-off inside a launch:
//   1. score_span_kernel: one block per span of kScoreSpan contiguous elements of one (n, c) plane.  Thread t
//      owns the elements span + 1024 j + 4 t .. + 3 (j = 0..3) whatever the plane's alignment (aligned planes
//      load them as one 16-byte vector, others element by element), accumulates them in that order in fp64,
//      the block reduces per wave (shuffles, fixed order) and across its four waves through LDS (wave order),
//      and stores its partial -- and its histogram, when sweeping -- to a scratch slab with plain stores.
//   2. score_sum_kernel: one block per (n, c) sums the slabs in ascending span order and writes the entry.
// The summation tree of an entry therefore depends on H * W alone: an entry is bitwise reproducible and does
// not depend on N, on the image's place in the batch or on the pointers' alignment.  No float atomics, no
// counters to clear; the block-local histogram uses integer LDS atomics.
//
// Per-element arithmetic is fp32 and follows the reference op by op (built with -ffp-contract=off: no fused
// multiply-add where the reference rounds twice); only the accumulation is fp64.
#include "unet_score.h"

namespace unet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuads = kScoreSpan / (4 * kThreads);   // 16-byte groups per thread
constexpr int kMaxBins = 2 * (kScoreMaxK + 1);
static_assert(kScoreSpan == kQuads * 4 * kThreads, "a span is a whole number of quads per thread");

struct Acc {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned n[3] = {0u, 0u, 0u};
};

// train.py:58 (sigmoid), :24-29 (Dice sums), :40-45 (focal term, gamma = 2; alpha is the host's)
__device__ inline void score_element(float x, float t, float cut, Acc& a, bool& pred, bool& tgt) {
  const float p = 1.0f / (1.0f + expf(-x));
  const float pt_prod = p * t;
  const float lo = 1e-7f, hi = (float)(1.0 - 1e-7);
  const float pc = p < lo ? lo : (p > hi ? hi : p);   // NaN stays NaN, as torch.clamp
  float l1 = logf(1.0f - pc);
  l1 = l1 < -100.0f ? -100.0f : l1;
  float l0 = logf(pc);
  l0 = l0 < -100.0f ? -100.0f : l0;
  const float bce = (t - 1.0f) * l1 - t * l0;
  const float q = expf(-bce);
  const float u = 1.0f - q;
  const float f = u * u * bce;
  a.s[0] += (double)p;
  a.s[1] += (double)(x != x ? x : t);   // a NaN logit marks all four sums of its entry
  a.s[2] += (double)pt_prod;
  a.s[3] += (double)f;
  pred = x > cut;   // the masks epilogue's predicate; false for NaN
  tgt = t > 0.5f;   // train.py:76
  a.n[0] += pred ? 1u : 0u;
  a.n[1] += tgt ? 1u : 0u;
  a.n[2] += (pred && tgt) ? 1u : 0u;
}

// #{k : x > cut[k]} over the non-decreasing cuts in LDS; 0 for NaN
__device__ inline int sweep_bin(float x, const float* cut, int K) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x > cut[mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ inline double shfl_down_f64(double v, int off) { return __shfl_down(v, off, 64); }

// TC: 0 = fp32 NCHW target; 1..4 = uint8 NHWC target of TC classes (value / 255.0f)
template <int TC, bool SWEEP>
__global__ __launch_bounds__(kThreads) void score_span_kernel(const float* __restrict__ logits,
                                                              const void* __restrict__ target, int C, long long HW,
                                                              int spans, ScoreCuts cuts, ScorePartial* __restrict__ part,
                                                              uint32_t* __restrict__ hpart) {
  __shared__ float s_cut[kScoreMaxK];
  __shared__ uint32_t s_hist[kWaves][kMaxBins];
  __shared__ double s_sum[kWaves][4];
  __shared__ uint32_t s_cnt[kWaves][3];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long plane = blockIdx.x / spans;
  const long long e0 = (long long)(blockIdx.x % spans) * kScoreSpan;
  const int c = (int)(plane % C);
  const long long n = plane / C;
  const int K = SWEEP ? cuts.K : 0;
  const int bins = 2 * (K + 1);
  if (SWEEP) {
    if (tid < K) s_cut[tid] = cuts.sweep[tid];
    for (int i = tid; i < kWaves * kMaxBins; i += kThreads) (&s_hist[0][0])[i] = 0u;
    __syncthreads();
  }
  const float cut = cuts.thr[c];

  const float* lp = logits + plane * HW;
  const float* tf = TC == 0 ? static_cast<const float*>(target) + plane * HW : nullptr;
  const uint8_t* tb = TC != 0 ? static_cast<const uint8_t*>(target) + n * HW * TC : nullptr;   // the image's pixels
  const bool l_vec = ((uintptr_t)lp & 15) == 0;
  const bool t_vec = TC == 0 ? ((uintptr_t)tf & 15) == 0 : ((uintptr_t)tb & 3) == 0;

  Acc a;
  int cur = -1;        // run of equal histogram bins: one LDS atomic per run, not per element
  uint32_t run = 0;
  for (int j = 0; j < kQuads; ++j) {
    const long long e = e0 + (long long)j * (4 * kThreads) + 4 * tid;
    if (e >= HW) break;
    const bool full = e + 3 < HW;
    float x[4], t[4];
    if (full && l_vec) {
      const float4 v = *reinterpret_cast<const float4*>(lp + e);
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
      for (int i = 0; i < 4; ++i) x[i] = e + i < HW ? lp[e + i] : 0.0f;
    }
    if (TC == 0) {
      if (full && t_vec) {
        const float4 v = *reinterpret_cast<const float4*>(tf + e);
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
      } else {
        for (int i = 0; i < 4; ++i) t[i] = e + i < HW ? tf[e + i] : 0.0f;
      }
    } else {
      const uint8_t* q = tb + e * TC;   // 4 pixels x TC classes = TC 32-bit words
      if (full && t_vec) {
        uint32_t w[TC == 0 ? 1 : TC];
        for (int k = 0; k < TC; ++k) w[k] = reinterpret_cast<const uint32_t*>(q)[k];
        for (int i = 0; i < 4; ++i) {
          const int b = c + TC * i;
          uint32_t ws = w[0];
          for (int k = 1; k < TC; ++k) ws = (b >> 2) == k ? w[k] : ws;
          t[i] = (float)((ws >> ((b & 3) * 8)) & 255u) / 255.0f;
        }
      } else {
        for (int i = 0; i < 4; ++i) t[i] = e + i < HW ? (float)q[i * TC + c] / 255.0f : 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (e + i >= HW) break;
      bool pred, tgt;
      score_element(x[i], t[i], cut, a, pred, tgt);
      if (SWEEP) {
        const int bin = (tgt ? K + 1 : 0) + sweep_bin(x[i], s_cut, K);
        if (bin == cur) {
          ++run;
        } else {
          if (run) atomicAdd(&s_hist[wave][cur], run);
          cur = bin;
          run = 1;
        }
      }
    }
  }
  if (SWEEP && run) atomicAdd(&s_hist[wave][cur], run);

  // per wave: shuffle tree in a fixed order
  for (int off = 32; off > 0; off >>= 1) {
    for (int k = 0; k < 4; ++k) a.s[k] += shfl_down_f64(a.s[k], off);
    for (int k = 0; k < 3; ++k) a.n[k] += __shfl_down(a.n[k], off, 64);
  }
  if (lane == 0) {
    for (int k = 0; k < 4; ++k) s_sum[wave][k] = a.s[k];
    for (int k = 0; k < 3; ++k) s_cnt[wave][k] = a.n[k];
  }
  __syncthreads();
  // across the waves, in wave order; plain stores to this block's own slab
  ScorePartial* out = part + blockIdx.x;
  if (tid < 4) {
    double s = s_sum[0][tid];
    for (int w = 1; w < kWaves; ++w) s += s_sum[w][tid];
    out->s[tid] = s;
  } else if (tid < 8) {
    uint32_t v = 0;
    if (tid < 7)
      for (int w = 0; w < kWaves; ++w) v += s_cnt[w][tid - 4];
    out->n[tid - 4] = v;
  }
  if (SWEEP) {
    for (int i = tid; i < bins; i += kThreads) {
      uint32_t v = 0;
      for (int w = 0; w < kWaves; ++w) v += s_hist[w][i];
      hpart[(size_t)blockIdx.x * bins + i] = v;
    }
  }
}

__global__ __launch_bounds__(kThreads) void score_sum_kernel(const ScorePartial* __restrict__ part,
                                                             const uint32_t* __restrict__ hpart, int spans,
                                                             long long HW, int K, unet_score_entry* __restrict__ entries,
                                                             int64_t* __restrict__ hist) {
  const int tid = threadIdx.x;
  const size_t plane = blockIdx.x;
  const ScorePartial* p = part + plane * spans;
  unet_score_entry* e = entries + plane;
  if (tid < 4) {   // one thread per sum: the spans in ascending order
    double s = p[0].s[tid];
    for (int i = 1; i < spans; ++i) s += p[i].s[tid];
    (tid == 0 ? e->sum_p : tid == 1 ? e->sum_t : tid == 2 ? e->sum_pt : e->sum_focal) = s;
  } else if (tid < 7) {
    int64_t v = 0;
    for (int i = 0; i < spans; ++i) v += p[i].n[tid - 4];
    (tid == 4 ? e->n_pred : tid == 5 ? e->n_tgt : e->n_both) = v;
  } else if (tid == 7) {
    e->n_px = HW;
  }
  if (hist) {
    const int bins = 2 * (K + 1);
    for (int b = tid; b < bins; b += kThreads) {
      int64_t v = 0;
      for (int i = 0; i < spans; ++i) v += hpart[(plane * spans + i) * bins + b];
      hist[plane * bins + b] = v;
    }
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <int TC>
hipError_t launch_span(bool sweep, unsigned grid, const float* logits, const void* target, int C, long long HW,
                       int spans, const ScoreCuts& cuts, ScorePartial* part, uint32_t* hpart, hipStream_t s) {
  if (sweep)
    hipLaunchKernelGGL((score_span_kernel<TC, true>), dim3(grid), dim3(kThreads), 0, s, logits, target, C, HW, spans,
                       cuts, part, hpart);
  else
    hipLaunchKernelGGL((score_span_kernel<TC, false>), dim3(grid), dim3(kThreads), 0, s, logits, target, C, HW, spans,
                       cuts, part, hpart);
  return hipGetLastError();
}

}  // namespace

size_t score_scratch_bytes(long long planes, long long hw, int K) {
  const size_t blocks = (size_t)planes * (size_t)score_spans(hw);
  return align256(blocks * sizeof(ScorePartial)) + (K > 0 ? align256(blocks * 2 * (size_t)(K + 1) * sizeof(uint32_t)) : 0);
}

hipError_t launch_score(const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
                        const ScoreCuts& cuts, void* scratch, unet_score_entry* entries, int64_t* hist,
                        hipStream_t s) {
  const long long HW = (long long)H * W, planes = (long long)N * C, spans = score_spans(HW);
  if (planes * spans > 0x7FFFFFFFLL || C < 1 || C > 4) return hipErrorInvalidValue;
  const bool sweep = hist != nullptr && cuts.K > 0;
  const unsigned grid = (unsigned)(planes * spans);
  ScorePartial* part = static_cast<ScorePartial*>(scratch);
  uint32_t* hpart = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + align256((size_t)grid * sizeof(ScorePartial)));
  hipError_t e;
  const int tc = target_kind == UNET_TGT_F32_NCHW ? 0 : C;
  switch (tc) {
    case 0: e = launch_span<0>(sweep, grid, logits, target, C, HW, (int)spans, cuts, part, hpart, s); break;
    case 1: e = launch_span<1>(sweep, grid, logits, target, C, HW, (int)spans, cuts, part, hpart, s); break;
    case 2: e = launch_span<2>(sweep, grid, logits, target, C, HW, (int)spans, cuts, part, hpart, s); break;
    case 3: e = launch_span<3>(sweep, grid, logits, target, C, HW, (int)spans, cuts, part, hpart, s); break;
    default: e = launch_span<4>(sweep, grid, logits, target, C, HW, (int)spans, cuts, part, hpart, s); break;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_sum_kernel, dim3((unsigned)planes), dim3(kThreads), 0, s, part, hpart, (int)spans, HW,
                     sweep ? cuts.K : 0, entries, sweep ? hist : nullptr);
  return hipGetLastError();
}

}  // namespace unet
