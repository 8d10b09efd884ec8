// Scoring of the output head from the stored features (unet_head_score, include/unet_mi355x.h; DESIGN.md section
// 14): out_conv's logits scored against the masks where they are formed, without the logits ever reaching memory and
// without a gathered copy of the pages scored.  What unet_head_forward_typed followed by unet_score computes, from
// one pass over the feature cache.
//
// Two launches, no float atomics, no tickets, no counters to clear:
//   1. head_score_pass_kernel: one block per (batch slot n, span of kHeadSpan pixels), step_pass_kernel's staging
//      (unet_step.hip, restated here: that unit stays as it is): kStage pixels of the 64 feature rows to LDS as fp32,
//      16-byte loads on the aligned path, the next stage's loads in flight under this stage's arithmetic.  Thread
//      (pixel, class pair) forms its logits from LDS by unet_head_forward's chain (fmaf from the bias, k ascending:
//      bitwise those logits; the weights are read from LDS, one address per wave), runs score_element's statements
//      (unet_score.hip) in fp32, adds the four sums in fp64 and the three counts in uint32 and, when sweeping, counts
//      its bin in a block-local LDS histogram (integer LDS atomics, one per run of equal bins).  The block reduces
//      per wave (shuffles, fixed order), then the two waves of a class pair in wave order, and stores one
//      ScorePartial per class -- and its bins -- into its own slab column with plain stores.
//   2. head_score_sum_kernel: one block per (slot, class) sums the spans in ascending order and writes the entry.
// The summation tree of an entry depends on H W alone: an entry is bitwise reproducible and does not depend on N, on
// the slot, on the other slots' pages, on pointer alignment or on the feature type (16-bit features are widened
// exactly before any arithmetic, and the narrow loads of an unaligned base read the same values).
// A page index outside [0, P) is never used as an address: its blocks store NaN sums, zero counts and zero bins.
//
// Per-element arithmetic is fp32 and follows the reference op by op (built with -ffp-contract=off; the logit
// chain's fmaf is explicit); only the accumulation is fp64.
#include "unet_hscore.h"

namespace unet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 128;                 // pixels per LDS stage
constexpr int kRow = kStage + 4;            // padded feature row (floats), as step_pass_kernel's
constexpr int kStageQuads = kStage / 4;
constexpr int kFeatQuads = kHeadK * kStageQuads / kThreads;
constexpr int kStageOcts = kStage / 8;
constexpr int kFeatOcts = kHeadK * kStageOcts / kThreads;
constexpr int kMaxBins = 2 * (kScoreMaxK + 1);
constexpr int kMaxC = 4;
static_assert(kHeadSpan % kStage == 0, "a span is a whole number of stages");
static_assert(kHeadK * kStageQuads == kFeatQuads * kThreads, "the stage's quads divide among the threads");
static_assert(kHeadK * kStageOcts == kFeatOcts * kThreads && kStageOcts == 16 && kHeadK * kStageOcts == 1024,
              "group16_of's bit layout");
static_assert(kWaves == 4 && kHeadK == 64 && kThreads == 2 * kStage, "thread (pixel, class pair)");

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ inline double shfl_down_f64(double v, int off) { return __shfl_down(v, off, 64); }

// ---- step_pass_kernel's staging (unet_step.hip), restated: the same loads, the same LDS image
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

// every 16-byte group (`group` elements) of every row of a [rows][HW] tensor starts on 16 bytes
__device__ inline bool rows_aligned(const void* base, long long HW, int group) {
  return ((uintptr_t)base & 15) == 0 && (HW & (group - 1)) == 0;
}

template <typename T>
constexpr int kGroup = 16 / (int)sizeof(T);

// fp16 / bf16 bits -> fp32, exact
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

template <typename T>
__device__ inline float4 widen_quad(unsigned lo, unsigned hi) {
  return make_float4(widen<T>(lo & 0xFFFFu), widen<T>(lo >> 16), widen<T>(hi & 0xFFFFu), widen<T>(hi >> 16));
}

// One stage's features in a thread's registers, between its global loads and its LDS stores.  Either way the LDS
// image is s_f[row * kRow + pixel] as fp32, zero past the plane.  fp32: 32 consecutive lanes take one row's quads.
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

// fp16 / bf16: groups of 8 pixels as loaded, widened when stored; group idx of the stage's 1024 is (row, oct) with
// lanes 0..3 of every 8 on four consecutive octs of an even row and lanes 4..7 on the same octs of the row below
// (unet_head.hip has why: whole 256-byte rows per wave, conflict-free 16-byte LDS stores)
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

// ---- the target of one (page, class) at pixel p as stored (fp32 NCHW: its bits; uint8 NHWC: the byte), and its
// value as the score reads it (the byte / 255.0f).  Two steps, so that a prefetched target waits for its load only
// where it is used, a stage later.
__device__ inline unsigned load_target(const void* __restrict__ target, bool u8, long long page, int c, int C,
                                       long long HW, long long p) {
  if (u8) return static_cast<const uint8_t*>(target)[(page * HW + p) * C + c];
  return __float_as_uint(static_cast<const float*>(target)[(page * C + c) * HW + p]);
}
__device__ inline float target_value(unsigned raw, bool u8) {
  return u8 ? (float)raw / 255.0f : __uint_as_float(raw);
}

struct Acc {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned n[3] = {0u, 0u, 0u};
};

// score_element (unet_score.hip), statement for statement: train.py:58 (sigmoid), :24-29 (Dice sums), :40-45
// (focal term, gamma = 2; alpha is the host's)
__device__ inline void score_element(float x, float t, float cut, Acc& a, bool& tgt) {
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
  const bool pred = x > cut;   // the masks epilogue's predicate; false for NaN
  tgt = t > 0.5f;              // train.py:76
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

// part: [N C][spans] ScorePartial, hpart: [N C][spans][2 (K + 1)] uint32; this block's column of plane n C + c is
// its span.  (3 waves per SIMD, as step_pass_kernel: at four the fp32 staging registers spill)
template <typename T, bool SWEEP>
__global__ __launch_bounds__(kThreads, 3) void head_score_pass_kernel(
    const T* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ b,
    const void* __restrict__ target, int tgt_u8, const int32_t* __restrict__ pages, int P, int C, long long HW,
    long long spans, ScoreCuts cuts, ScorePartial* __restrict__ part, uint32_t* __restrict__ hpart) {
  __shared__ __attribute__((aligned(16))) float s_f[kHeadK * kRow];
  __shared__ __attribute__((aligned(16))) float s_w[kMaxC * kHeadK];
  __shared__ float s_cut[kScoreMaxK];
  __shared__ uint32_t s_hist[kMaxC][kMaxBins];
  __shared__ double s_sum[kWaves][2][4];
  __shared__ uint32_t s_cnt[kWaves][2][3];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: scalar branches, one LDS address per wave
  const long long n = blockIdx.x / spans;
  const long long sp = blockIdx.x % spans;
  const long long p0 = sp * kHeadSpan;
  const int K = SWEEP ? cuts.K : 0;
  const int bins = 2 * (K + 1);
  const long long page = pages ? (long long)pages[n] : n;
  if (page < 0 || page >= P) {   // no address is formed from it
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    if (tid < 8 * C) {
      ScorePartial* out = part + (n * C + (tid >> 3)) * spans + sp;
      const int j = tid & 7;
      if (j < 4) out->s[j] = nan; else out->n[j - 4] = 0u;
    }
    if (SWEEP)
      for (int i = tid; i < C * bins; i += kThreads)
        hpart[((n * C + i / bins) * spans + sp) * bins + i % bins] = 0u;
    return;
  }
  const long long span_len = HW - p0 < kHeadSpan ? HW - p0 : kHeadSpan;
  const int stages = (int)((span_len + kStage - 1) / kStage);
  const T* fbase = feat + page * kHeadK * HW;
  const bool f_vec = rows_aligned(feat, HW, kGroup<T>);
  // this thread's pixel of a stage and its two classes (waves 0, 1: classes 0 and 2; waves 2, 3: 1 and 3)
  const int px = tid & (kStage - 1), half = wave >> 1;
  const bool has[2] = {half < C, half + 2 < C};
  const int cls[2] = {has[0] ? half : 0, has[1] ? half + 2 : 0};   // the rows of w and of the target to read

  if (tid < C * kHeadK) s_w[tid] = w[tid];   // read after the first stage's barrier
  if (SWEEP) {
    if (tid < K) s_cut[tid] = cuts.sweep[tid];
    for (int i = tid; i < kMaxC * kMaxBins; i += kThreads) (&s_hist[0][0])[i] = 0u;
  }
  const float bq[2] = {b[cls[0]], b[cls[1]]};
  const float cut[2] = {cuts.thr[cls[0]], cuts.thr[cls[1]]};
  StageFeat<T> rf;
  unsigned rt[2] = {0u, 0u};
  auto fetch = [&](long long ps) {
    rf.fetch(fbase, HW, ps, tid, f_vec);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (has[i] && ps + px < HW) rt[i] = load_target(target, tgt_u8 != 0, page, cls[i], C, HW, ps + px);
  };
  Acc acc[2];
  int cur[2] = {-1, -1};        // runs of equal histogram bins: one LDS atomic per run, not per element
  uint32_t run[2] = {0u, 0u};
  fetch(p0);
  for (int st = 0; st < stages; ++st) {
    const long long ps = p0 + (long long)st * kStage;
    rf.store(s_f, tid);
    const float t_now[2] = {target_value(rt[0], tgt_u8 != 0), target_value(rt[1], tgt_u8 != 0)};
    __syncthreads();
    if (st + 1 < stages) fetch(ps + kStage);   // in flight under this stage's arithmetic
    if (has[0]) {
      float x[2] = {bq[0], bq[1]};
      const float4* w0 = reinterpret_cast<const float4*>(&s_w[cls[0] * kHeadK]);   // one address per wave: broadcast
      const float4* w1 = reinterpret_cast<const float4*>(&s_w[cls[1] * kHeadK]);
#pragma unroll 4
      for (int k = 0; k < kHeadK; k += 4) {
        const float4 a = w0[k >> 2], c = w1[k >> 2];
        const float f0 = s_f[k * kRow + px], f1 = s_f[(k + 1) * kRow + px], f2 = s_f[(k + 2) * kRow + px],
                    f3 = s_f[(k + 3) * kRow + px];
        x[0] = fmaf(a.x, f0, x[0]);
        x[1] = fmaf(c.x, f0, x[1]);
        x[0] = fmaf(a.y, f1, x[0]);
        x[1] = fmaf(c.y, f1, x[1]);
        x[0] = fmaf(a.z, f2, x[0]);
        x[1] = fmaf(c.z, f2, x[1]);
        x[0] = fmaf(a.w, f3, x[0]);
        x[1] = fmaf(c.w, f3, x[1]);
      }
      if (ps + px < HW) {   // nothing past the plane
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (!has[i]) continue;
          bool tgt;
          score_element(x[i], t_now[i], cut[i], acc[i], tgt);
          if (SWEEP) {
            const int bin = (tgt ? K + 1 : 0) + sweep_bin(x[i], s_cut, K);
            if (bin == cur[i]) {
              ++run[i];
            } else {
              if (run[i]) atomicAdd(&s_hist[cls[i]][cur[i]], run[i]);
              cur[i] = bin;
              run[i] = 1u;
            }
          }
        }
      }
    }
    __syncthreads();   // the stage is read: the next one may be stored
  }
  if (SWEEP) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (run[i]) atomicAdd(&s_hist[cls[i]][cur[i]], run[i]);
  }
  // per wave a shuffle tree in a fixed order, then the two waves of a class pair in wave order
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i].s[k] += shfl_down_f64(acc[i].s[k], off);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[i].n[k] += __shfl_down(acc[i].n[k], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_sum[wave][i][k] = acc[i].s[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) s_cnt[wave][i][k] = acc[i].n[k];
    }
  }
  __syncthreads();
  if (tid < 8 * C) {   // plain stores to this block's own column
    const int c = tid >> 3, j = tid & 7, hf = c & 1, i = c >> 1;
    ScorePartial* out = part + (n * C + c) * spans + sp;
    if (j < 4) out->s[j] = s_sum[2 * hf][i][j] + s_sum[2 * hf + 1][i][j];
    else out->n[j - 4] = j < 7 ? s_cnt[2 * hf][i][j - 4] + s_cnt[2 * hf + 1][i][j - 4] : 0u;
  }
  if (SWEEP)
    for (int i = tid; i < C * bins; i += kThreads)
      hpart[((n * C + i / bins) * spans + sp) * bins + i % bins] = s_hist[i / bins][i % bins];
}

// one block per plane n C + c: score_sum_kernel's order (unet_score.hip), the spans ascending
__global__ __launch_bounds__(kThreads) void head_score_sum_kernel(const ScorePartial* __restrict__ part,
                                                                  const uint32_t* __restrict__ hpart, long long spans,
                                                                  long long HW, int K,
                                                                  unet_score_entry* __restrict__ entries,
                                                                  int64_t* __restrict__ hist) {
  const int tid = threadIdx.x;
  const size_t plane = blockIdx.x;
  const ScorePartial* p = part + plane * spans;
  unet_score_entry* e = entries + plane;
  if (tid < 4) {   // one thread per sum
    double s = p[0].s[tid];
    for (long long i = 1; i < spans; ++i) s += p[i].s[tid];
    (tid == 0 ? e->sum_p : tid == 1 ? e->sum_t : tid == 2 ? e->sum_pt : e->sum_focal) = s;
  } else if (tid < 7) {
    int64_t v = 0;
    for (long long i = 0; i < spans; ++i) v += p[i].n[tid - 4];
    (tid == 4 ? e->n_pred : tid == 5 ? e->n_tgt : e->n_both) = v;
  } else if (tid == 7) {
    e->n_px = HW;
  }
  if (hist) {
    const int bins = 2 * (K + 1);
    for (int bn = tid; bn < bins; bn += kThreads) {
      int64_t v = 0;
      for (long long i = 0; i < spans; ++i) v += hpart[(plane * spans + i) * bins + bn];
      hist[plane * bins + bn] = v;
    }
  }
}

template <typename T>
hipError_t launch_pass(bool sweep, unsigned grid, const void* feat, const float* w, const float* b, const void* target,
                       int target_kind, const int32_t* pages, int P, int C, long long HW, long long spans,
                       const ScoreCuts& cuts, ScorePartial* part, uint32_t* hpart, hipStream_t s) {
  const int u8 = target_kind == UNET_TGT_U8_NHWC ? 1 : 0;
  if (sweep)
    hipLaunchKernelGGL((head_score_pass_kernel<T, true>), dim3(grid), dim3(kThreads), 0, s,
                       static_cast<const T*>(feat), w, b, target, u8, pages, P, C, HW, spans, cuts, part, hpart);
  else
    hipLaunchKernelGGL((head_score_pass_kernel<T, false>), dim3(grid), dim3(kThreads), 0, s,
                       static_cast<const T*>(feat), w, b, target, u8, pages, P, C, HW, spans, cuts, part, hpart);
  return hipGetLastError();
}

}  // namespace

size_t hscore_scratch_bytes(long long N, long long hw, int C, int K) {
  const size_t cols = (size_t)N * (size_t)C * (size_t)head_spans(hw);
  return align256(cols * sizeof(ScorePartial)) + (K > 0 ? align256(cols * 2 * (size_t)(K + 1) * sizeof(uint32_t)) : 0);
}

hipError_t launch_head_score(const void* feat, int feat_dtype, const float* w, const float* b, const void* target,
                             int target_kind, const int32_t* pages, int P, int N, int C, int H, int W,
                             const ScoreCuts& cuts, void* scratch, unet_score_entry* entries, int64_t* hist,
                             hipStream_t s) {
  const long long HW = (long long)H * W, spans = head_spans(HW), nslabs = N * spans;
  if (nslabs * 4 > 0x7FFFFFFFLL || C < 1 || C > kMaxC || P < 1) return hipErrorInvalidValue;
  const bool sweep = hist != nullptr && cuts.K > 0;
  const unsigned grid = (unsigned)nslabs;
  ScorePartial* part = static_cast<ScorePartial*>(scratch);
  uint32_t* hpart = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) +
                                                align256((size_t)nslabs * C * sizeof(ScorePartial)));
  hipError_t e;
  switch (feat_dtype) {
    case UNET_DTYPE_F32:
      e = launch_pass<float>(sweep, grid, feat, w, b, target, target_kind, pages, P, C, HW, spans, cuts, part, hpart, s);
      break;
    case UNET_DTYPE_F16:
      e = launch_pass<_Float16>(sweep, grid, feat, w, b, target, target_kind, pages, P, C, HW, spans, cuts, part, hpart,
                                s);
      break;
    case UNET_DTYPE_BF16:
      e = launch_pass<__bf16>(sweep, grid, feat, w, b, target, target_kind, pages, P, C, HW, spans, cuts, part, hpart,
                              s);
      break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(head_score_sum_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, s, part, hpart, spans, HW,
                     sweep ? cuts.K : 0, entries, sweep ? hist : nullptr);
  return hipGetLastError();
}

}  // namespace unet
