// Internal (non-ABI) declarations of the scoring kernels (unet_score.hip), shared with the C-ABI host layer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/unet_mi355x.h"

namespace unet {

// Elements of one (image, class) plane that one block of launch 1 reduces: a compile-time constant, so the
// number of spans of a plane (and with it the summation tree of an entry) depends on H * W only.
constexpr int kScoreSpan = 4096;
constexpr int kScoreMaxK = 64;   // sweep candidates

// One block's partial of one span (launch 1 stores it, launch 2 sums the spans of a plane in ascending order).
struct ScorePartial {
  double s[4];      // sum_p, sum_t, sum_pt, sum_focal
  uint32_t n[4];    // n_pred, n_tgt, n_both, unused
};

// Kernel arguments passed by value (no upload, so a score is capturable as it stands).
struct ScoreCuts {
  float thr[4];              // per-class logit cut of the n_pred predicate (unet_logit_cut)
  int K;                     // sweep candidates, 0 = no sweep
  float sweep[kScoreMaxK];   // their logit cuts, non-decreasing
};

inline long long score_spans(long long hw) { return (hw + kScoreSpan - 1) / kScoreSpan; }
// scratch bytes of a score over `planes` planes of hw pixels with K sweep candidates
size_t score_scratch_bytes(long long planes, long long hw, int K);

// target_kind: UNET_TGT_F32_NCHW / UNET_TGT_U8_NHWC.  hist == nullptr (and cuts.K == 0): no sweep.
hipError_t launch_score(const float* logits, const void* target, int target_kind, int N, int C, int H, int W,
                        const ScoreCuts& cuts, void* scratch, unet_score_entry* entries, int64_t* hist,
                        hipStream_t s);

}  // namespace unet
