// One row of test-time voting (engines/test.py:218-229): p[0..c) += softmax(x[0..c)).  The ONE definition both voting kernels run
// (k_vote in loss.hip: one fragment per call; k_fragment_vote in fragments.hip: a batch of fragments per call), so that a point's
// vote is the same sequence of the same fp32 operations whichever kernel folded its fragments.  The accumulation is an explicit fused
// multiply-add (what the compiler's default contraction made of `p[j] += e * inv`), so that no inline site can round it differently.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void pdf_vote_row(const float *__restrict__ x, int c, float *__restrict__ p) {
    float m = x[0];
    for (int j = 1; j < c; ++j) m = fmaxf(m, x[j]);
    float s = 0.f;
    for (int j = 0; j < c; ++j) s += __expf(x[j] - m);
    const float inv = 1.f / s;
    for (int j = 0; j < c; ++j) p[j] = __fmaf_rn(__expf(x[j] - m), inv, p[j]);
}
