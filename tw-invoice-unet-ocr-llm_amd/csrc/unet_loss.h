// Internal (non-ABI) declarations of the differentiable InvoiceLoss (unet_loss.hip), shared with the C-ABI host
// layer: the loss as a device scalar and its gradient at the logits (unet_loss_grad, include/unet_mi355x.h).
#pragma once
#include "unet_score.h"

namespace unet {

// unet_loss_config by value (gamma is 2, as in the score)
struct LossParams {
  float dw, fw, alpha, smooth;
};

// The forward chain of one element, train.py:58 and :40-45: the values autograd saves for the backward pass.
struct LossChain {
  float p, pc, bce, q, u;
};

// score_element's arithmetic (unet_score.hip), statement for statement: the focal sum the loss is made of and the
// gradient must come from the same p, pc, bce, q and u.  Translation units that call this are built with
// -ffp-contract=off, as unet_score.hip is.
__device__ inline LossChain loss_chain(float x, float t) {
  LossChain c;
  c.p = 1.0f / (1.0f + expf(-x));
  const float lo = 1e-7f, hi = (float)(1.0 - 1e-7);
  c.pc = c.p < lo ? lo : (c.p > hi ? hi : c.p);   // NaN stays NaN, as torch.clamp
  float l1 = logf(1.0f - c.pc);
  l1 = l1 < -100.0f ? -100.0f : l1;
  float l0 = logf(c.pc);
  l0 = l0 < -100.0f ? -100.0f : l0;
  c.bce = (t - 1.0f) * l1 - t * l0;
  c.q = expf(-c.bce);
  c.u = 1.0f - c.q;
  return c;
}

// scratch bytes of a loss over `planes` planes of hw pixels: the score's slabs (no sweep), the entries and the
// gradient coefficients
size_t loss_scratch_bytes(long long planes, long long hw);

// Steps 1-3 on s: launch_score (entries into the scratch), the coefficient kernel (*loss and the per-plane Dice
// coefficients), and, with grad != nullptr, the element-wise gradient.  grad_out: device scalar or nullptr (1.0).
hipError_t launch_loss(const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
                       const LossParams& prm, const float* grad_out, float* loss, float* grad, void* scratch,
                       hipStream_t s);

}  // namespace unet
