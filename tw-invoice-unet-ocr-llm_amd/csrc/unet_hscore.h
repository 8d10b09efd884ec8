// Internal (non-ABI) declarations of the head's scoring pass (unet_hscore.hip), shared with the C-ABI host layer:
// out_conv's logits formed from the stored features and scored against the masks where they are formed
// (unet_head_score, include/unet_mi355x.h).
#pragma once
#include "unet_head.h"
#include "unet_score.h"

namespace unet {

// scratch bytes of a head score over N batch slots of hw pixels with C classes and K sweep candidates: one
// ScorePartial per (slot, class, span of kHeadSpan pixels), then with K > 0 that many rows of 2 (K + 1) uint32 bins
size_t hscore_scratch_bytes(long long N, long long hw, int C, int K);

// Two launches on s: the pass (one block per batch slot and span, its partials into the scratch) and one block per
// (slot, class) that sums the spans in ascending order into entries [N][C] and, with a sweep, hist [N][C][2][K+1].
// feat / target: the bases of the whole cache of P pages; pages: device int32 [N] or nullptr (slot n is page n).
// hist == nullptr (and cuts.K == 0): no sweep.
hipError_t launch_head_score(const void* feat, int feat_dtype, const float* w, const float* b, const void* target,
                             int target_kind, const int32_t* pages, int P, int N, int C, int H, int W,
                             const ScoreCuts& cuts, void* scratch, unet_score_entry* entries, int64_t* hist,
                             hipStream_t s);

}  // namespace unet
