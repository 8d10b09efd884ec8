// One training step of the output head from one pass over the stored features (unet_head_step,
// include/unet_mi355x.h): out_conv's logits, InvoiceLoss, its gradient at the 64 C + C
// parameters and AdamW, without the logits or their gradient ever reaching memory.
//
// The gradient at a logit is (g0 e + A t + B) s with e the focal branch's gradient for an upstream 1, s = (1 - p) p
// and A, B the Dice coefficients of the logit's (page, class) plane, known only once the plane has been seen.  So
//   grad_w[c][k] = sum_n ( g0 F[n][c][k] + A[n][c] T[n][c][k] + B[n][c] S[n][c][k] )
//   F = sum_p (e_p s_p) feat_k[p],  T = sum_p (t_p s_p) feat_k[p],  S = sum_p s_p feat_k[p]
// and grad_b the same with feat == 1: three vectors per (page, class), accumulated where the logits are formed.
//
// Three launches, no float atomics, no tickets, no counters to clear:
//   1. step_pass_kernel: one block per (batch slot n, span of kHeadSpan pixels), head_partial_kernel's staging
//      (unet_head.hip, restated here: that unit stays as it is): kStage pixels of the 64 feature rows to LDS as
//      fp32, 16-byte loads on the aligned path, the next stage's loads in flight under this stage's sums.  Per stage
//      (a) thread (pixel, class pair) forms its logits from LDS by unet_head_forward's chain (fmaf from the bias, k
//      ascending: bitwise those logits; the weights are read from LDS, one address per wave), runs loss_chain and
//      focal_grad_unit in fp32, adds the four plane sums of unet_score_entry and the three bias rows in fp64 and
//      writes e s, t s and s to LDS as fp64; (b) wave = class, lane = (kk, pg): the feature rows kk, kk + 16,
//      kk + 32, kk + 48 at the pixel quads 4 jj + pg of the stage, three fp64 accumulators per row (an explicit
//      fma, one rounding per term, pixels ascending), the four pg of a row combined at the end as
//      (pg0 + pg1) + (pg2 + pg3).  One 16-byte read of a class's factors thus serves four feature rows: with
//      head_partial_kernel's lane = k the kernel was bound by LDS reads of the factors.
//      The block stores its step_entries(C) doubles into its own slab column.
//   2. step_coef_kernel: one block.  Per plane the four sums over its spans in ascending order, then the loss and
//      A, B by loss_coef_kernel's formula and order (unet_loss.hip), kept in fp64.
//   3. step_sum_kernel: one block per parameter sums g0 F + A T + B S over the slab columns in head_sum_kernel's
//      fixed order, rounds the gradient to fp32 once and, when asked, applies AdamW to its parameter in fp64.
// The summation trees depend on (N, H W) only; 16-bit features are widened exactly before any arithmetic, and the
// narrow loads of an unaligned base read the same values: the results do not depend on alignment or feature type.
// A page index outside [0, P) is never used as an address: its blocks store NaN partials.
#include "unet_step.h"

namespace unet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStage = 128;                 // pixels per LDS stage
constexpr int kRow = kStage + 4;            // padded feature row (floats), as head_partial_kernel's
constexpr int kStageQuads = kStage / 4;
constexpr int kFeatQuads = kHeadK * kStageQuads / kThreads;
constexpr int kStageOcts = kStage / 8;
constexpr int kFeatOcts = kHeadK * kStageOcts / kThreads;
static_assert(kHeadSpan % kStage == 0, "a span is a whole number of stages");
static_assert(kHeadK * kStageQuads == kFeatQuads * kThreads, "the stage's quads divide among the threads");
static_assert(kHeadK * kStageOcts == kFeatOcts * kThreads && kStageOcts == 16 && kHeadK * kStageOcts == 1024,
              "group16_of's bit layout");
static_assert(kWaves == 4 && kHeadK == 64 && kStage % 16 == 0 && kThreads == 2 * kStage,
              "wave = class, lane = (row mod 16, quad mod 4); thread (pixel, class pair)");

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ inline double shfl_down_f64(double v, int off) { return __shfl_down(v, off, 64); }

// ---- head_partial_kernel's staging (unet_head.hip), restated: the same loads, the same LDS image
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

// The element chain at one logit: score_element's sums (unet_score.hip) into a[0..3], and the three factors of the
// gradient.  s = (1 - p) p with the difference in fp32, as sigmoid's backward forms it, and the product exact in fp64.
__device__ inline void step_element(float x, float t, float alpha, double (&a)[4], double& es, double& ts,
                                    double& s) {
  const LossChain c = loss_chain(x, t);
  const float pt_prod = c.p * t;
  const float f = c.u * c.u * c.bce;
  a[0] += (double)c.p;
  a[1] += (double)(x != x ? x : t);   // a NaN logit marks all four sums of its entry
  a[2] += (double)pt_prod;
  a[3] += (double)f;
  const float e = focal_grad_unit(c, t, alpha);
  s = (double)(1.0f - c.p) * (double)c.p;
  es = (double)e * s;
  ts = (double)t * s;
}

// slabs: [step_entries(C)][nslabs] fp64, this block's column = its slab index.  Rows: (q C + c) 64 + k for
// q = F, T, S; then 3 * 64 C + q C + c (bias); then 3 * 65 C + 4 c + j (sum_p, sum_t, sum_pt, sum_focal)
// (3 waves per SIMD: the three blocks per CU that the LDS admits)
template <typename T>
__global__ __launch_bounds__(kThreads, 3) void step_pass_kernel(const T* __restrict__ feat,
                                                             const void* __restrict__ target, int tgt_u8,
                                                             const int32_t* __restrict__ pages, int P,
                                                             const float* __restrict__ w, const float* __restrict__ b,
                                                             int C, long long HW, long long spans, long long nslabs,
                                                             float alpha, double* __restrict__ slabs) {
  __shared__ __attribute__((aligned(16))) float s_f[kHeadK * kRow];
  __shared__ __attribute__((aligned(16))) double s_q[3][kWaves][kStage];   // e s, t s, s of class c
  __shared__ double s_sum[kWaves][2][7];
  __shared__ __attribute__((aligned(16))) float s_w[4 * kHeadK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: scalar branches, one LDS address per wave
  const long long slab = blockIdx.x;
  const long long n = slab / spans;
  const long long p0 = (slab % spans) * kHeadSpan;
  const long long page = pages ? (long long)pages[n] : n;
  if (page < 0 || page >= P) {   // no address is formed from it
    const double nan = __longlong_as_double(0x7FF8000000000000LL);
    for (long long e = tid; e < step_entries(C); e += kThreads) slabs[e * nslabs + slab] = nan;
    return;
  }
  const long long span_len = HW - p0 < kHeadSpan ? HW - p0 : kHeadSpan;
  const int stages = (int)((span_len + kStage - 1) / kStage);
  const T* fbase = feat + page * kHeadK * HW;
  const bool f_vec = rows_aligned(feat, HW, kGroup<T>);
  // (a): this thread's pixel of a stage and its two classes (waves 0, 1: classes 0 and 2; waves 2, 3: 1 and 3)
  const int px = tid & (kStage - 1), half = wave >> 1;
  const bool has[2] = {half < C, half + 2 < C};
  const int cls[2] = {has[0] ? half : 0, has[1] ? half + 2 : 0};   // the rows of w and of the target to read

  if (tid < C * kHeadK) s_w[tid] = w[tid];   // read after the first stage's barrier
  const float bq[2] = {b[cls[0]], b[cls[1]]};
  StageFeat<T> rf;
  unsigned rt[2] = {0u, 0u};
  auto fetch = [&](long long ps) {
    rf.fetch(fbase, HW, ps, tid, f_vec);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (has[i] && ps + px < HW) rt[i] = load_target(target, tgt_u8 != 0, page, cls[i], C, HW, ps + px);
  };
  double sums[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};   // the plane sums of the two classes
  double bias[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};            // ... and their bias rows: F, T, S with feat == 1
  double aF[4] = {0.0, 0.0, 0.0, 0.0}, aT[4] = {0.0, 0.0, 0.0, 0.0}, aS[4] = {0.0, 0.0, 0.0, 0.0};
  const int kk = lane & 15, pg = lane >> 4;
  fetch(p0);
  for (int st = 0; st < stages; ++st) {
    const long long ps = p0 + (long long)st * kStage;
    rf.store(s_f, tid);
    const float t_now[2] = {target_value(rt[0], tgt_u8 != 0), target_value(rt[1], tgt_u8 != 0)};
    __syncthreads();
    if (st + 1 < stages) fetch(ps + kStage);   // in flight under this stage's sums
    if (has[0]) {
      const bool in = ps + px < HW;
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
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (!has[i]) continue;
        double es = 0.0, ts = 0.0, s = 0.0;
        if (in) {   // zero past the plane
          step_element(x[i], t_now[i], alpha, sums[i], es, ts, s);
          bias[i][0] += es;
          bias[i][1] += ts;
          bias[i][2] += s;
        }
        s_q[0][half + 2 * i][px] = es;
        s_q[1][half + 2 * i][px] = ts;
        s_q[2][half + 2 * i][px] = s;
      }
    }
    __syncthreads();
    if (wave < C) {
      // (b): wave = class; lane = (kk, pg) takes the feature rows kk, kk + 16, kk + 32, kk + 48 at the quads
      // 4 jj + pg of the stage, so one read of the class's factors serves four rows
      const float* fr = &s_f[kk * kRow + 4 * pg];
      const double* qe = &s_q[0][wave][4 * pg];
      const double* qt = &s_q[1][wave][4 * pg];
      const double* qs = &s_q[2][wave][4 * pg];
#pragma unroll 2
      for (int o = 0; o < kStage; o += 16) {
        const double2* pe = reinterpret_cast<const double2*>(qe + o);
        const double2* pt = reinterpret_cast<const double2*>(qt + o);
        const double2* pq = reinterpret_cast<const double2*>(qs + o);
        const double2 e01 = pe[0], e23 = pe[1], t01 = pt[0], t23 = pt[1], s01 = pq[0], s23 = pq[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 f4 = *reinterpret_cast<const float4*>(fr + 16 * i * kRow + o);
          const double f0 = (double)f4.x, f1 = (double)f4.y, f2 = (double)f4.z, f3 = (double)f4.w;
          aF[i] = fma(e23.y, f3, fma(e23.x, f2, fma(e01.y, f1, fma(e01.x, f0, aF[i]))));
          aT[i] = fma(t23.y, f3, fma(t23.x, f2, fma(t01.y, f1, fma(t01.x, f0, aT[i]))));
          aS[i] = fma(s23.y, f3, fma(s23.x, f2, fma(s01.y, f1, fma(s01.x, f0, aS[i]))));
        }
      }
    }
    __syncthreads();
  }
  // the plane sums and bias rows: per wave a shuffle tree, then the two waves of a class pair in wave order
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      double v = j < 4 ? sums[i][j] : bias[i][j - 4];
      for (int off = 32; off > 0; off >>= 1) v += shfl_down_f64(v, off);
      if (lane == 0) s_sum[wave][i][j] = v;
    }
  if (wave < C) {   // the four pixel groups of a row: (pg 0 + pg 1) + (pg 2 + pg 3), stored by the lanes of pg 0
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double v = q == 0 ? aF[i] : q == 1 ? aT[i] : aS[i];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (pg == 0) slabs[((long long)(q * C + wave) * kHeadK + kk + 16 * i) * nslabs + slab] = v;
      }
  }
  __syncthreads();
  if (tid < 7 * C) {
    const int c = tid / 7, j = tid % 7, hf = c & 1, i = c >> 1;
    const long long row = j < 4 ? 3LL * (kHeadK * C + C) + 4 * c + j : 3LL * kHeadK * C + (j - 4) * C + c;
    slabs[row * nslabs + slab] = s_sum[2 * hf][i][j] + s_sum[2 * hf + 1][i][j];
  }
}

// coef[2 i], coef[2 i + 1] = A, B of plane i = n C + c, scaled by dice_weight / (N C): loss_coef_kernel's formula
// and order (unet_loss.hip) for an upstream gradient of 1, kept in fp64
__global__ __launch_bounds__(kThreads) void step_coef_kernel(const double* __restrict__ slabs, int C, long long planes,
                                                             long long spans, long long nslabs, long long HW,
                                                             LossParams prm, float* __restrict__ loss,
                                                             double* __restrict__ coef) {
  __shared__ double s_sum[kWaves][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double smooth = (double)prm.smooth;
  const double scale = (double)prm.dw / (double)planes;
  double dice = 0.0, focal = 0.0;
  for (long long i = tid; i < planes; i += kThreads) {   // a fixed order: thread, then wave, then block
    const long long n = i / C;
    const int c = (int)(i % C);
    const double* row = slabs + (3LL * (kHeadK * C + C) + 4 * c) * nslabs + n * spans;
    double s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = row[j * nslabs];
    for (long long sp = 1; sp < spans; ++sp)   // the spans in ascending order
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += row[j * nslabs + sp];
    const double den = s[0] + s[1] + smooth, num = 2.0 * s[2] + smooth;
    dice += 1.0 - num / den;
    focal += s[3];
    coef[2 * i] = -2.0 / den * scale;
    coef[2 * i + 1] = num / (den * den) * scale;
  }
  for (int off = 32; off > 0; off >>= 1) {
    dice += shfl_down_f64(dice, off);
    focal += shfl_down_f64(focal, off);
  }
  if (lane == 0) {
    s_sum[wave][0] = dice;
    s_sum[wave][1] = focal;
  }
  __syncthreads();
  if (tid == 0) {
    double d = s_sum[0][0], f = s_sum[0][1];
    for (int v = 1; v < kWaves; ++v) {
      d += s_sum[v][0];
      f += s_sum[v][1];
    }
    const double numel = (double)planes * (double)HW;
    *loss = (float)((double)prm.dw * (d / (double)planes) + (double)prm.fw * (double)prm.alpha * f / numel);
  }
}

// block o < 64 C: w[o]; block 64 C + c: b[c].  The gradient is the sum over the slab columns of g0 F + A T + B S
// (thread t the columns t, t + 256, ... in ascending order, then a fixed shuffle / LDS tree), rounded to fp32 once;
// AdamW (torch.optim.AdamW's formulas) then runs on that fp32 gradient in fp64 and rounds m, v and the parameter
// once each.  state: m_w, m_b, v_w, v_b.
__global__ __launch_bounds__(kThreads) void step_sum_kernel(const double* __restrict__ slabs,
                                                            const double* __restrict__ coef, int C, long long spans,
                                                            long long nslabs, float g0, float* __restrict__ w,
                                                            float* __restrict__ b, float* __restrict__ grad_w,
                                                            float* __restrict__ grad_b, StepAdam adam,
                                                            float* __restrict__ state) {
  __shared__ double s_sum[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int o = blockIdx.x, nw = C * kHeadK;
  const int c = o < nw ? o / kHeadK : o - nw;
  const long long r0 = o < nw ? o : 3LL * nw + c;                   // F's row of this output
  const long long rq = o < nw ? nw : C;                             // rows from F to T, and from T to S
  const double* rF = slabs + r0 * nslabs;
  const double* rT = rF + rq * nslabs;
  const double* rS = rT + rq * nslabs;
  const double g = (double)g0;
  double a = 0.0;
  for (long long i = tid; i < nslabs; i += kThreads) {
    const double* ab = coef + 2 * ((i / spans) * C + c);
    a += (g * rF[i] + ab[0] * rT[i]) + ab[1] * rS[i];
  }
  for (int off = 32; off > 0; off >>= 1) a += shfl_down_f64(a, off);
  if (lane == 0) s_sum[wave] = a;
  __syncthreads();
  if (tid != 0) return;
  double t = s_sum[0];
  for (int v = 1; v < kWaves; ++v) t += s_sum[v];
  const float grad = (float)t;
  if (grad_w) (o < nw ? grad_w[o] : grad_b[c]) = grad;
  if (!adam.on) return;
  float* theta = o < nw ? w + o : b + c;
  float* m = state + o;
  float* v = state + (nw + C) + o;
  const double gd = (double)grad;
  const double m1 = adam.beta1 * (double)*m + (1.0 - adam.beta1) * gd;
  const double v1 = adam.beta2 * (double)*v + (1.0 - adam.beta2) * gd * gd;
  double th = (double)*theta * adam.decay;
  th -= adam.lr / adam.bc1 * m1 / (sqrt(v1) / adam.bc2_sqrt + adam.eps);
  *m = (float)m1;
  *v = (float)v1;
  *theta = (float)th;
}

template <typename T>
hipError_t launch_pass(const void* feat, const void* target, int target_kind, const int32_t* pages, int P,
                       const float* w, const float* b, int C, long long HW, long long nslabs, float alpha,
                       double* slabs, hipStream_t s) {
  hipLaunchKernelGGL(step_pass_kernel<T>, dim3((unsigned)nslabs), dim3(kThreads), 0, s, static_cast<const T*>(feat),
                     target, target_kind == UNET_TGT_U8_NHWC ? 1 : 0, pages, P, w, b, C, HW, head_spans(HW), nslabs,
                     alpha, slabs);
  return hipGetLastError();
}

}  // namespace

size_t step_scratch_bytes(long long N, long long hw, int C) {
  return align256((size_t)(N * head_spans(hw)) * (size_t)step_entries(C) * sizeof(double)) +
         align256((size_t)N * C * 2 * sizeof(double));
}

hipError_t launch_head_step(const void* feat, int feat_dtype, const void* target, int target_kind,
                            const int32_t* pages, int P, int N, int C, int H, int W, const LossParams& prm, float* w,
                            float* b, float* loss, float* grad_w, float* grad_b, const StepAdam& adam, float* state,
                            void* scratch, hipStream_t s) {
  const long long HW = (long long)H * W, spans = head_spans(HW), nslabs = N * spans, planes = (long long)N * C;
  if (nslabs > 0x7FFFFFFFLL || C < 1 || C > 4 || P < 1) return hipErrorInvalidValue;
  double* slabs = static_cast<double*>(scratch);
  double* coef = reinterpret_cast<double*>(static_cast<char*>(scratch) +
                                           align256((size_t)nslabs * (size_t)step_entries(C) * sizeof(double)));
  hipError_t e;
  switch (feat_dtype) {
    case UNET_DTYPE_F32:
      e = launch_pass<float>(feat, target, target_kind, pages, P, w, b, C, HW, nslabs, prm.alpha, slabs, s);
      break;
    case UNET_DTYPE_F16:
      e = launch_pass<_Float16>(feat, target, target_kind, pages, P, w, b, C, HW, nslabs, prm.alpha, slabs, s);
      break;
    case UNET_DTYPE_BF16:
      e = launch_pass<__bf16>(feat, target, target_kind, pages, P, w, b, C, HW, nslabs, prm.alpha, slabs, s);
      break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(step_coef_kernel, dim3(1), dim3(kThreads), 0, s, slabs, C, planes, spans, nslabs, HW, prm, loss,
                     coef);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const float g0 = prm.fw / (float)((double)planes * (double)HW);   // mean's backward, fp32 as autograd
  hipLaunchKernelGGL(step_sum_kernel, dim3((unsigned)(kHeadK * C + C)), dim3(kThreads), 0, s, slabs, coef, C, spans,
                     nslabs, g0, w, b, grad_w, grad_b, adam, state);
  return hipGetLastError();
}

}  // namespace unet
