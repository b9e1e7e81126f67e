// Streaming per-point Linear layers, fp32 operands (MP = 0) + the precision-independent helpers (RL2_MAIN_TU), the paired products and
// the ONE dispatch on the call's product-input mode (`mma_input` of the C entry points, include/pdfops.h): with_mp turns the run-time
// mode into the template argument MP of try_*_mp.  Interface: rowlin2.h.  Kernels and host code: rowlin2_impl.h.
#define RL2_MAIN_TU
#include "rowlin2_impl.h"
#include <type_traits>

namespace rl2 {
template int try_forward_mp<0>(const Forward &, hipStream_t, int *);
template int try_wgrad_mp<0>(const Wgrad &, hipStream_t);
template int try_forward2_mp<0>(const Forward (&)[2], hipStream_t);
template int try_wgrad_pair_mp<0>(const Wgrad (&)[2], bool, hipStream_t, RArgs *);
template int try_forward_stats2_mp<0>(const Forward (&)[2], hipStream_t);
template int try_wgrad_fwd_mp<0>(const Wgrad &, const Forward &, hipStream_t);
extern template int try_forward_mp<1>(const Forward &, hipStream_t, int *);   // rowlin2_f16.hip
extern template int try_wgrad_mp<1>(const Wgrad &, hipStream_t);
extern template int try_wgrad_pair_mp<1>(const Wgrad (&)[2], bool, hipStream_t, RArgs *);
extern template int try_forward_mp<2>(const Forward &, hipStream_t, int *);   // rowlin2_bf16.hip
extern template int try_wgrad_mp<2>(const Wgrad &, hipStream_t);
extern template int try_wgrad_pair_mp<2>(const Wgrad (&)[2], bool, hipStream_t, RArgs *);

template <class F>
static int with_mp(int mma, F f) {   // f(std::integral_constant<int, MP>)
    switch (mma) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    default: return f(std::integral_constant<int, 0>());
    }
}

int try_forward(const Forward &p, int mma, hipStream_t s, int *partial_rows) {
    return with_mp(mma, [&](auto mp) { return try_forward_mp<decltype(mp)::value>(p, s, partial_rows); });
}
int try_wgrad(const Wgrad &p, int mma, hipStream_t s) {
    return with_mp(mma, [&](auto mp) { return try_wgrad_mp<decltype(mp)::value>(p, s); });
}
int try_wgrad_pair(const Wgrad (&p)[2], bool pair, int mma, hipStream_t s, RArgs *r) {
    return with_mp(mma, [&](auto mp) { return try_wgrad_pair_mp<decltype(mp)::value>(p, pair, s, r); });
}
// The paired product kernels are built for fp32 operands only: mma_input 1 / 2 gets 0 here, i.e. two single launches.
int try_forward2(const Forward (&p)[2], int mma, hipStream_t s) { return mma == 0 ? try_forward2_mp<0>(p, s) : 0; }
int try_forward_stats2(const Forward (&p)[2], int mma, hipStream_t s) { return mma == 0 ? try_forward_stats2_mp<0>(p, s) : 0; }
int try_wgrad_fwd(const Wgrad &w, const Forward &f, int mma, hipStream_t s) { return mma == 0 ? try_wgrad_fwd_mp<0>(w, f, s) : 0; }
}  // namespace rl2
