// Fixed-order slot sums of the loss and metric passes (device-only, no state; gfx950 / wave64).
//
// Every workgroup of such a pass leaves its partial sums in its own slot and ONE workgroup adds the slots: no float atomics, nothing to
// zero beforehand, capturable, bit-reproducible.  A workgroup's values are combined in one of two orders:
//   by waves: a wave64 xor-butterfly per value, then thread 0 adds the LB / 64 wave totals in wave order (the tail of a row pass);
//   by lanes: every lane leaves its value in its own LDS cell, then thread 0 adds the LB cells in lane order (the tail of a finisher).
// Three combine entry points share these two orders: block_sum_by_waves, block_sum_wave_totals (by waves for values that are wave totals
// already, e.g. ballot counts: no butterfly) and block_sum_by_lanes; slot_total is by lanes over a finisher's slots.
// A pass's order, its element type, the number of sums it carries and its slot layout are part of its RESULTS: changing one of them at a
// call site changes the bits of the loss, so a site is converted to a helper only where the helper reproduces its order exactly.
//
// Calling rule: ALL LB threads of the block call a helper, under block-uniform control flow.  A helper keeps its LDS cells in a __shared__
// array of its own and STARTS with the barrier that frees those cells, so it may be called again in the same kernel (k_lv_loss: once per
// class) without a barrier at the call site.  Every sum starts from zero, as the loops these helpers replace did.
#pragma once
#include "pdfops_common.h"

// v = one value per wave and sum (already the same on every lane that matters: lane 0 of each wave stores it).  Thread 0 receives the
// sums over the waves, added in wave order, in `out` and true; the other threads receive false and leave `out` alone.
template <int LB, int K, typename T>
__device__ __forceinline__ bool block_sum_wave_totals(const T (&v)[K], T (&out)[K]) {
    __shared__ T red[K][LB / 64];
    __syncthreads();   // (a previous call's thread 0 has read its cells)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = T(0);
    for (int w = 0; w < LB / 64; ++w) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] += red[k][w];
    }
    return true;
}

// By waves: v (every thread's partial sums; left holding the wave totals) -> dst[0..K), written by thread 0.
template <int LB, int K, typename T>
__device__ __forceinline__ void block_sum_by_waves(T (&v)[K], T *dst) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = pdf_wave_sum(v[k]);
    T out[K];
    if (block_sum_wave_totals<LB>(v, out)) {
#pragma unroll
        for (int k = 0; k < K; ++k) dst[k] = out[k];
    }
}

// By lanes: v (every thread's partial sums) -> out on thread 0, which alone receives true.
template <int LB, int K, typename T>
__device__ __forceinline__ bool block_sum_by_lanes(const T (&v)[K], T (&out)[K]) {
    __shared__ T red[K][LB];
    __syncthreads();   // (a previous call's thread 0 has read its cells)
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = T(0);
    for (int t = 0; t < LB; ++t) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] += red[k][t];
    }
    return true;
}

// The finisher: slot g = the K values at slots + K g.  Lane l adds slots l, l + LB, ... in ascending order, then by lanes.
template <int LB, int K, typename T>
__device__ __forceinline__ bool slot_total(const T *slots, int nslots, T (&out)[K]) {
    T v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = T(0);
    for (int g = threadIdx.x; g < nslots; g += LB) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += slots[(size_t)K * g + k];
    }
    return block_sum_by_lanes<LB>(v, out);
}

// The backward of these passes: out = d * s over a grid-stride loop (the forward's unscaled buffer d is only read).  The caller forms s
// with its own expression: a quotient and a product round differently.
template <int LB>
__device__ __forceinline__ void pdf_scaled_copy(long total, const float *__restrict__ d, float s, float *__restrict__ out) {
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < total; e += (long)gridDim.x * LB) out[e] = d[e] * s;
}
