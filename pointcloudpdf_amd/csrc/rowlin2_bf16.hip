// Streaming per-point Linear layers with bfloat16 product operands (MP = 2): kernels and host code in rowlin2_impl.h, dispatch in rowlin2.hip.
#include "rowlin2_impl.h"

namespace rl2 {
template int try_forward_mp<2>(const Forward &, hipStream_t, int *);
template int try_wgrad_mp<2>(const Wgrad &, hipStream_t);
template int try_wgrad_pair_mp<2>(const Wgrad (&)[2], bool, hipStream_t, RArgs *);
}  // namespace rl2
