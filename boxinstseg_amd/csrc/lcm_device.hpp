// lcm_device.hpp -- the LocalConsistencyModule refinement of levelset.hip as the other translation units reach it.
// The kernels live in levelset.hip and take the affinity block of instance n through an optional index array (img_of): one copy of the
// device code serves bxi_lcm_refine_f32 (every instance its own affinity) and bxi_b2m_lcm_refine_f32 (one affinity per image, box2mask_loss.hip).
#pragma once

#include "common.hpp"

namespace bxi {

// aff [n_aff,8,h,w], phi / out [N,h,w].  img_of == nullptr: instance n reads affinity n (n_aff == N).  Otherwise instance n reads
// affinity img_of[n]; an index outside [0, n_aff) makes the instance inert: its plane of `out` is written as zeros.  Arguments are
// checked by the caller; the workspace rule is bxi_lcm_refine_f32's (bxi_lcm_workspace_bytes(N, h, w), only maps too large for LDS).
int lcm_refine_launch(const float* aff, const float* phi, const int* img_of, int n_aff, int N, int h, int w, int dilation, int iters,
                      int transpose, float* out, void* workspace, size_t workspace_bytes, hipStream_t s);

}  // namespace bxi
