// The reference's InvoiceLoss (train.py:18-59) as a device scalar, with its gradient at the logits
// (unet_loss_grad, include/unet_mi355x.h): what train.py:137-142 does with a batch of logits.
//
// Three steps on one stream, no host round trip, no float atomics, no counters to clear:
//   1. launch_score (unet_score.hip, called, not copied): per (n, c) the fp64 sums sum_p, sum_t, sum_pt and
//      sum_focal, bitwise the entries unet_score writes.
//   2. loss_coef_kernel: one block.  In fp64, from the entries: the loss, stored as one fp32 scalar, and per plane
//      the Dice gradient's coefficients -- dDice_nc / dp_i = A_nc t_i + B_nc -- scaled by dice_weight / (N C) and
//      the upstream gradient, stored as fp32 pairs behind g0 = upstream * focal_weight / (N C H W).
//   3. loss_grad_kernel: one block per span of kScoreSpan elements of one plane, the score kernel's tiling and
//      loads.  Per element the forward chain is recomputed (loss_chain, unet_loss.h) and ATen's backward formulas
//      are walked in fp32 in autograd's order; 16-byte stores where the gradient's plane is aligned.
// The per-element arithmetic is fp32 and follows the reference op by op (built with -ffp-contract=off), so the
// clamp edge of train.py:41 cuts the gradient of a confidently wrong pixel where the reference cuts it.
#include "unet_loss.h"

namespace unet {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuads = kScoreSpan / (4 * kThreads);   // 16-byte groups per thread, as the score kernel
static_assert(kScoreSpan == kQuads * 4 * kThreads, "a span is a whole number of quads per thread");

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ inline double shfl_down_f64(double v, int off) { return __shfl_down(v, off, 64); }

// coef[0] = g0, coef[1] unused, coef[2 + 2 i], coef[3 + 2 i] = A, B of plane i
__global__ __launch_bounds__(kThreads) void loss_coef_kernel(const unet_score_entry* __restrict__ entries,
                                                             long long planes, long long HW, LossParams prm,
                                                             const float* __restrict__ grad_out,
                                                             float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ double s_sum[kWaves][2];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float up = grad_out ? *grad_out : 1.0f;
  const double smooth = (double)prm.smooth;
  const double scale = (double)prm.dw / (double)planes * (double)up;
  double dice = 0.0, focal = 0.0;
  for (long long i = tid; i < planes; i += kThreads) {   // a fixed order: thread, then wave, then block
    const unet_score_entry e = entries[i];
    const double den = e.sum_p + e.sum_t + smooth, num = 2.0 * e.sum_pt + smooth;
    dice += 1.0 - num / den;
    focal += e.sum_focal;
    coef[2 + 2 * i] = (float)(-2.0 / den * scale);
    coef[3 + 2 * i] = (float)(num / (den * den) * scale);
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
    for (int w = 1; w < kWaves; ++w) {
      d += s_sum[w][0];
      f += s_sum[w][1];
    }
    const double numel = (double)planes * (double)HW;
    *loss = (float)((double)prm.dw * (d / (double)planes) + (double)prm.fw * (double)prm.alpha * f / numel);
    coef[0] = up * prm.fw / (float)numel;   // mean's backward, fp32 as autograd
    coef[1] = 0.0f;
  }
}

// autograd's backward of InvoiceLoss at one element, fp32, in the order the engine runs the nodes
__device__ inline float loss_grad_element(float x, float t, float g0, float alpha, float A, float B) {
  const LossChain c = loss_chain(x, t);
  const float u2 = c.u * c.u;
  const float m1 = alpha * u2;                 // forward: (alpha * (1 - pt) ** 2) * bce
  const float g_m1 = g0 * c.bce;               // the product with bce
  float g_bce = g0 * m1;
  const float g_u2 = g_m1 * alpha;             // the product with alpha
  const float g_u = g_u2 * (2.0f * c.u);       // pow, exponent 2
  const float g_q = -g_u;                      // 1 - pt
  const float g_nb = g_q * c.q;                // exp: grad * result
  g_bce = g_bce + (-g_nb);                     // the negation; bce's second use
  float den = (1.0f - c.pc) * c.pc;
  den = den < 1e-12f ? 1e-12f : den;
  const float g_pc = g_bce * (c.pc - t) / den;   // binary_cross_entropy
  const float lo = 1e-7f, hi = (float)(1.0 - 1e-7);
  float g_p = (c.p >= lo && c.p <= hi) ? g_pc : 0.0f;   // clamp
  g_p = g_p + (A * t + B);                     // the Dice branch: NaN coefficients for a plane with a NaN logit
  return g_p * (1.0f - c.p) * c.p;             // sigmoid
}

// TC: 0 = fp32 NCHW target; 1..4 = uint8 NHWC target of TC classes (value / 255.0f)
template <int TC>
__global__ __launch_bounds__(kThreads) void loss_grad_kernel(const float* __restrict__ logits,
                                                             const void* __restrict__ target, int C, long long HW,
                                                             int spans, float alpha, const float* __restrict__ coef,
                                                             float* __restrict__ grad) {
  const int tid = threadIdx.x;
  const long long plane = blockIdx.x / spans;
  const long long e0 = (long long)(blockIdx.x % spans) * kScoreSpan;
  const int c = (int)(plane % C);
  const long long n = plane / C;
  const float g0 = coef[0], A = coef[2 + 2 * plane], B = coef[3 + 2 * plane];

  const float* lp = logits + plane * HW;
  float* gp = grad + plane * HW;
  const float* tf = TC == 0 ? static_cast<const float*>(target) + plane * HW : nullptr;
  const uint8_t* tb = TC != 0 ? static_cast<const uint8_t*>(target) + n * HW * TC : nullptr;   // the image's pixels
  const bool l_vec = ((uintptr_t)lp & 15) == 0, g_vec = ((uintptr_t)gp & 15) == 0;
  const bool t_vec = TC == 0 ? ((uintptr_t)tf & 15) == 0 : ((uintptr_t)tb & 3) == 0;

  for (int j = 0; j < kQuads; ++j) {
    const long long e = e0 + (long long)j * (4 * kThreads) + 4 * tid;
    if (e >= HW) break;
    const bool full = e + 3 < HW;
    float x[4], t[4], g[4];
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
    for (int i = 0; i < 4; ++i) g[i] = loss_grad_element(x[i], t[i], g0, alpha, A, B);
    if (full && g_vec) {
      *reinterpret_cast<float4*>(gp + e) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
      for (int i = 0; i < 4; ++i)
        if (e + i < HW) gp[e + i] = g[i];
    }
  }
}

template <int TC>
hipError_t launch_grad(unsigned grid, const float* logits, const void* target, int C, long long HW, int spans,
                       float alpha, const float* coef, float* grad, hipStream_t s) {
  hipLaunchKernelGGL((loss_grad_kernel<TC>), dim3(grid), dim3(kThreads), 0, s, logits, target, C, HW, spans, alpha,
                     coef, grad);
  return hipGetLastError();
}

}  // namespace

size_t loss_scratch_bytes(long long planes, long long hw) {
  return align256(score_scratch_bytes(planes, hw, 0)) + align256((size_t)planes * sizeof(unet_score_entry)) +
         align256((2 + 2 * (size_t)planes) * sizeof(float));
}

hipError_t launch_loss(const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
                       const LossParams& prm, const float* grad_out, float* loss, float* grad, void* scratch,
                       hipStream_t s) {
  const long long HW = (long long)H * W, planes = (long long)N * C, spans = score_spans(HW);
  if (planes * spans > 0x7FFFFFFFLL || C < 1 || C > 4) return hipErrorInvalidValue;
  char* base = static_cast<char*>(scratch);
  unet_score_entry* entries = reinterpret_cast<unet_score_entry*>(base + align256(score_scratch_bytes(planes, HW, 0)));
  float* coef = reinterpret_cast<float*>(reinterpret_cast<char*>(entries) +
                                         align256((size_t)planes * sizeof(unet_score_entry)));
  ScoreCuts cuts{};   // K = 0; the counts of the entries are not read
  hipError_t e = launch_score(logits, target, target_kind, N, C, H, W, cuts, scratch, entries, nullptr, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loss_coef_kernel, dim3(1), dim3(kThreads), 0, s, entries, planes, HW, prm, grad_out, loss, coef);
  e = hipGetLastError();
  if (e != hipSuccess || !grad) return e;
  const unsigned grid = (unsigned)(planes * spans);
  switch (target_kind == UNET_TGT_F32_NCHW ? 0 : C) {
    case 0: return launch_grad<0>(grid, logits, target, C, HW, (int)spans, prm.alpha, coef, grad, s);
    case 1: return launch_grad<1>(grid, logits, target, C, HW, (int)spans, prm.alpha, coef, grad, s);
    case 2: return launch_grad<2>(grid, logits, target, C, HW, (int)spans, prm.alpha, coef, grad, s);
    case 3: return launch_grad<3>(grid, logits, target, C, HW, (int)spans, prm.alpha, coef, grad, s);
    default: return launch_grad<4>(grid, logits, target, C, HW, (int)spans, prm.alpha, coef, grad, s);
  }
}

}  // namespace unet
