// Internal (non-ABI) declarations of the fused head training step (unet_step.hip), shared with the C-ABI host
// layer: out_conv's logits, InvoiceLoss, its gradient at the 64 C + C parameters and AdamW from one pass over the
// stored features (unet_head_step, include/unet_mi355x.h).
#pragma once
#include "unet_head.h"
#include "unet_loss.h"

namespace unet {

// Doubles one block of the pass stores (its slab column): per class the three 64-vectors F, T, S and their bias
// rows, then the four plane sums of unet_score_entry
__host__ __device__ inline long long step_entries(int C) { return 3LL * (kHeadK * C + C) + 4LL * C; }

// scratch bytes of a step over N batch slots of hw pixels with C classes: N * head_spans(hw) slab columns of
// step_entries(C) fp64 partials, then the Dice coefficients A, B of the N * C planes
size_t step_scratch_bytes(long long N, long long hw, int C);

// AdamW's constants of one call, by value and in fp64 (the host forms the bias corrections from the step count)
struct StepAdam {
  int on;          // 0: no update, the rest is not read
  double lr, beta1, beta2, eps;
  double decay;    // 1 - lr * weight_decay
  double bc1;      // 1 - beta1^t
  double bc2_sqrt; // sqrt(1 - beta2^t)
};

// The focal branch of loss_grad_element (unet_loss.hip), statement for statement, for an upstream gradient of 1 (a
// product with 1.0f is exact, so its statements are the ones that remain): autograd's backward of the focal term
// at p, fp32, in the order the engine runs the nodes, the clamp's pass / cut included.  The caller scales by
// g0 = focal_weight / (N C H W), adds the Dice branch A t + B and multiplies by sigmoid's (1 - p) p in fp64.
// Translation units that call this are built with -ffp-contract=off.
__device__ inline float focal_grad_unit(const LossChain& c, float t, float alpha) {
  const float u2 = c.u * c.u;
  const float m1 = alpha * u2;                 // forward: (alpha * (1 - pt) ** 2) * bce
  const float g_m1 = c.bce;                    // the product with bce
  float g_bce = m1;
  const float g_u2 = g_m1 * alpha;             // the product with alpha
  const float g_u = g_u2 * (2.0f * c.u);       // pow, exponent 2
  const float g_q = -g_u;                      // 1 - pt
  const float g_nb = g_q * c.q;                // exp: grad * result
  g_bce = g_bce + (-g_nb);                     // the negation; bce's second use
  float den = (1.0f - c.pc) * c.pc;
  den = den < 1e-12f ? 1e-12f : den;
  const float g_pc = g_bce * (c.pc - t) / den;   // binary_cross_entropy
  const float lo = 1e-7f, hi = (float)(1.0 - 1e-7);
  return (c.p >= lo && c.p <= hi) ? g_pc : 0.0f;   // clamp
}

// Three launches on s: the pass (one block per batch slot and span, its partials into the scratch), the
// coefficient block (*loss and the planes' A, B) and one block per parameter (grad_w / grad_b, either pair may be
// nullptr, and with adam.on the update of w, b and state).  pages: device int32 [N] or nullptr (slot n is page n).
hipError_t launch_head_step(const void* feat, int feat_dtype, const void* target, int target_kind,
                            const int32_t* pages, int P, int N, int C, int H, int W, const LossParams& prm, float* w,
                            float* b, float* loss, float* grad_w, float* grad_b, const StepAdam& adam, float* state,
                            void* scratch, hipStream_t s);

}  // namespace unet
