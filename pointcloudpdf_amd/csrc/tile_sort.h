// Stable LSD radix sort of 32-bit keys with one payload per key, 8-bit digits (four passes), as capturable launches: no host read,
// nothing to zero beforehand, integer counters only (the result does not depend on the order of arrival).  Shared by csrc/lovasz.hip
// (C segments of N keys, payload = unsigned) and csrc/openset_metrics.hip (one segment, payload = one byte).
//
//   k_ts_hist     tile = grid.x, segment = grid.y: the tile's digit counts -> hist[(segment * 256 + digit) * tiles + tile].
//   the scan      the exclusive scan of a segment's (digit, tile) counts = where every group starts in the pass's output.  Two forms:
//                   one level   k_ts_scan_segments, one workgroup per segment, lane = digit, in place: the group's start is hist[e];
//                   two levels  (ONE segment of up to 2^31 - 2 keys: a linear array of 256 * tiles words) k_ts_scan_chunks scans chunks of
//                               1024 words by a workgroup each, k_ts_scan_short the chunk totals: the start is hist[e] + gtot[e / 1024].
//   k_ts_scatter  position = start of the (digit, tile) group + keys of that digit in the tile's earlier waves + in the wave's earlier
//                 rounds + among the round's lower lanes (wave ballots: lanes with an equal digit, lower lane first): equal keys keep their
//                 order, as every pass of an LSD sort must.  Ping-pong between two buffers.
// Everything here has internal linkage: each translation unit keeps its own kernel symbols.
#pragma once
#include "pdfops_common.h"

namespace tile_sort {
namespace {

constexpr int LB = 256;
constexpr int ITEMS = 8;                 // keys per lane and tile: wave w owns 512 consecutive keys, round r the 64 at w * 512 + r * 64
constexpr int TILE = LB * ITEMS;         // 2048
constexpr int WAVES = LB / 64;
constexpr int RADIX = 256;               // 8-bit digits, four passes
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_CHUNK = LB * SCAN_ITEMS;   // 1024 words per workgroup of the first level of the two-level scan

__device__ __forceinline__ size_t pos(int tile, int w, int r, int lane) { return (size_t)tile * TILE + w * (ITEMS * 64) + r * 64 + lane; }

inline size_t chunks(size_t words) { return (words + SCAN_CHUNK - 1) / SCAN_CHUNK; }

// exclusive scan of the workgroup's 256 values (lane order); `s` = 256 words of LDS, free on entry, free again after the call
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *s) {
    unsigned x = v;
    s[threadIdx.x] = x;
    __syncthreads();
    for (int o = 1; o < LB; o <<= 1) {
        const unsigned y = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        x += y;
        s[threadIdx.x] = x;
        __syncthreads();
    }
    return x - v;
}

// hist[(seg * 256 + digit) * ntiles + tile] = number of keys of the segment's tile with that digit
__global__ __launch_bounds__(LB) void k_ts_hist(long n, int ntiles, int shift, const unsigned *__restrict__ keys, unsigned *__restrict__ hist) {
    __shared__ unsigned h[RADIX];
    const int tile = blockIdx.x, seg = blockIdx.y;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned *k = keys + (size_t)seg * n;
    for (int i = 0; i < ITEMS; ++i) {
        const size_t p = (size_t)tile * TILE + i * LB + threadIdx.x;
        if (p < (size_t)n) atomicAdd(&h[(k[p] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[((size_t)seg * RADIX + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// one level, in place: hist[seg][digit][tile] -> number of keys of the segment that precede the (digit, tile) group in the pass's output.
// One workgroup per segment, lane = digit.
__global__ __launch_bounds__(LB) void k_ts_scan_segments(int ntiles, unsigned *__restrict__ hist) {
    __shared__ unsigned s[LB];
    unsigned *h = hist + ((size_t)blockIdx.x * RADIX + threadIdx.x) * ntiles;
    unsigned sum = 0u;
    for (int t = 0; t < ntiles; ++t) sum += h[t];
    unsigned run = block_excl_scan(sum, s);
    for (int t = 0; t < ntiles; ++t) { const unsigned v = h[t]; h[t] = run; run += v; }
}

// first of two levels, in place: data[e] -> sum of the chunk's words before e; gtot[chunk] = the chunk's sum
__global__ __launch_bounds__(LB) void k_ts_scan_chunks(long len, unsigned *__restrict__ data, unsigned *__restrict__ gtot) {
    __shared__ unsigned s[LB];
    const long e0 = (long)blockIdx.x * SCAN_CHUNK + (long)threadIdx.x * SCAN_ITEMS;
    unsigned v[SCAN_ITEMS], sum = 0u;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = e0 + i < len ? data[e0 + i] : 0u; sum += v[i]; }
    unsigned run = block_excl_scan(sum, s);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (e0 + i < len) data[e0 + i] = run;
        run += v[i];
    }
    if (threadIdx.x == LB - 1) gtot[blockIdx.x] = run;
}

// a short array per workgroup, in place: data[b][e] -> sum of the array's words before e; total[b] = the array's sum (when asked for).
// Lane l scans the contiguous stretch [l * per, (l + 1) * per).
__global__ __launch_bounds__(LB) void k_ts_scan_short(int len, unsigned *__restrict__ data, unsigned *__restrict__ total) {
    __shared__ unsigned s[LB];
    unsigned *d = data + (size_t)blockIdx.x * len;
    const int per = (len + LB - 1) / LB, t0 = min(len, (int)threadIdx.x * per), t1 = min(len, t0 + per);
    unsigned sum = 0u;
    for (int t = t0; t < t1; ++t) sum += d[t];
    unsigned run = block_excl_scan(sum, s);
    for (int t = t0; t < t1; ++t) { const unsigned v = d[t]; d[t] = run; run += v; }
    if (total && threadIdx.x == LB - 1) total[blockIdx.x] = run;
}

// element e of an array scanned in two levels
__device__ __forceinline__ unsigned scanned(const unsigned *data, const unsigned *gtot, size_t e) { return data[e] + gtot[e / SCAN_CHUNK]; }

// stable scatter of one tile of one segment (see the head of the file).  TWO_LEVEL: how the scan left the group's start.
template <typename P, bool TWO_LEVEL>
__global__ __launch_bounds__(LB) void k_ts_scatter(long n, int ntiles, int shift, const unsigned *__restrict__ keys_in,
                                                   const P *__restrict__ pay_in, const unsigned *__restrict__ hist,
                                                   const unsigned *__restrict__ gtot, unsigned *__restrict__ keys_out,
                                                   P *__restrict__ pay_out) {
    __shared__ unsigned cnt[WAVES][RADIX];
    const int tile = blockIdx.x, sg = TWO_LEVEL ? 0 : blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;   // (two levels: ONE segment)
    const size_t seg = (size_t)sg * n;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) cnt[i][threadIdx.x] = 0u;
    __syncthreads();
    unsigned key[ITEMS], off[ITEMS];
    P val[ITEMS];
    const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const size_t p = pos(tile, w, r, lane);
        const bool valid = p < (size_t)n;
        key[r] = valid ? keys_in[seg + p] : 0u;
        val[r] = valid ? pay_in[seg + p] : (P)0;
        const unsigned d = (key[r] >> shift) & (RADIX - 1);
        unsigned long long peers = __ballot(valid);   // lanes of the round with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned before = valid ? cnt[w][d] : 0u;   // the wave's own counters: no other wave touches them
        off[r] = before + (unsigned)__popcll(peers & lower);
        __syncthreads();
        if (valid && (peers & lower) == 0ull) cnt[w][d] = before + (unsigned)__popcll(peers);   // the group's lowest lane
        __syncthreads();
    }
    {   // lane = digit: the waves' counts become the waves' starting positions
        const size_t e = ((size_t)sg * RADIX + threadIdx.x) * ntiles + tile;
        unsigned run = TWO_LEVEL ? scanned(hist, gtot, e) : hist[e];
#pragma unroll
        for (int i = 0; i < WAVES; ++i) { const unsigned v = cnt[i][threadIdx.x]; cnt[i][threadIdx.x] = run; run += v; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        if (pos(tile, w, r, lane) < (size_t)n) {
            const unsigned q = cnt[w][(key[r] >> shift) & (RADIX - 1)] + off[r];   // < n: the groups partition the segment's n keys
            if ((size_t)q >= (size_t)n) continue;                                    // (never taken; no store outside the buffers whatever happens)
            keys_out[seg + q] = key[r];
            pay_out[seg + q] = val[r];
        }
    }
}

// The four passes over `nseg` segments of n keys, from keys[0] / pay[0]; returns the index of the buffer pair that holds the sorted
// order.  Four passes whatever the data: nothing is decided on the host.  TWO_LEVEL sorts ONE segment (nseg == 1: its scan is one linear
// array) and needs gtot: chunks(tiles * 256) words.
template <typename P, bool TWO_LEVEL>
int sort(long n, int nseg, unsigned *const keys[2], P *const pay[2], unsigned *hist, unsigned *gtot, hipStream_t s) {
    const int nt = (int)((n + TILE - 1) / TILE);
    const dim3 grid((unsigned)nt, (unsigned)nseg);
    const long hlen = (long)nt * RADIX, hchunks = (long)chunks((size_t)hlen);
    int cur = 0;
    for (int shift = 0; shift < 32; shift += 8, cur ^= 1) {
        k_ts_hist<<<grid, LB, 0, s>>>(n, nt, shift, keys[cur], hist);
        if (TWO_LEVEL) {
            k_ts_scan_chunks<<<(unsigned)hchunks, LB, 0, s>>>(hlen, hist, gtot);
            k_ts_scan_short<<<1, LB, 0, s>>>((int)hchunks, gtot, nullptr);
        } else {
            k_ts_scan_segments<<<(unsigned)nseg, LB, 0, s>>>(nt, hist);
        }
        k_ts_scatter<P, TWO_LEVEL><<<grid, LB, 0, s>>>(n, nt, shift, keys[cur], pay[cur], hist, gtot, keys[cur ^ 1], pay[cur ^ 1]);
    }
    return cur;
}

}  // namespace
}  // namespace tile_sort
