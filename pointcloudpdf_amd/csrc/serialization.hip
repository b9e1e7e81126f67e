// Point Transformer V3's serialization (models/utils/structure.py:47-102, models/utils/serialization/) and the partition of its
// code-shift pooling (point_transformer_v3m1_base.py:384-396) as launches on the caller's stream: integers only, nothing allocated.
//
//   pdf_serial_codes            one launch, one thread per point: the (k, n) int64 codes of the requested curves.  z: bit i of x / y / z at
//                               3 i + 2 / 3 i + 1 / 3 i (what the reference's two 8-bit tables spell out).  hilbert: Skilling's transform of
//                               the three axes (per bit from the top: invert or exchange the lower bits against axis 0), the same
//                               interleave, and the prefix xor from the top bit (the reference's gray2binary over the 3 depth bits) -- a few
//                               integer operations per bit in registers, no table.
//   pdf_serial_sort             per code row the stable ascending order (two stable 32-bit radix sorts of csrc/tile_sort.h, low word first)
//                               and its inverse (a scatter).
//   pdf_serial_pool_partition   code0[order0] >> shift is already ascending: flags of the run starts, their scan, then per row the rank of
//                               its row index inside its run -- `sorted` lists a cluster's rows in ascending row index, as a stable sort of
//                               `cluster` does, so the segment reductions of csrc/grid_pool.hip add in the composition's order.
#include "tile_sort.h"

namespace sz {
namespace {

constexpr int TB = 256;

__device__ __forceinline__ unsigned long long interleave3(unsigned x, unsigned y, unsigned z, int depth) {
    unsigned long long key = 0ull;
    for (int i = 0; i < depth; ++i) {
        const unsigned long long m = 1ull << i;
        key |= (((unsigned long long)x & m) << (2 * i + 2)) | (((unsigned long long)y & m) << (2 * i + 1)) | (((unsigned long long)z & m) << (2 * i));
    }
    return key;
}

__device__ __forceinline__ unsigned long long hilbert3(unsigned x0, unsigned x1, unsigned x2, int depth) {
    unsigned X[3] = {x0, x1, x2};
    for (int bit = 0; bit < depth; ++bit) {   // from the top bit down, axes 0, 1, 2
        const unsigned q = 1u << (depth - 1 - bit), lower = q - 1u;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (X[d] & q) X[0] ^= lower;                                      // bit on: invert the lower bits of axis 0
            else { const unsigned t = (X[0] ^ X[d]) & lower; X[0] ^= t; X[d] ^= t; }   // bit off: exchange them with axis d
        }
    }
    unsigned long long h = interleave3(X[0], X[1], X[2], depth);
    h ^= h >> 1; h ^= h >> 2; h ^= h >> 4; h ^= h >> 8; h ^= h >> 16; h ^= h >> 32;   // Gray -> binary: xor of all higher bits
    return h;
}

__global__ __launch_bounds__(TB) void k_codes(long n, int k, int orders, int depth, const int *__restrict__ gc, const long long *__restrict__ batch,
                                              long long *__restrict__ code) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const unsigned mask = depth >= 32 ? 0xffffffffu : ((1u << depth) - 1u);
    const unsigned x = (unsigned)gc[i * 3] & mask, y = (unsigned)gc[i * 3 + 1] & mask, z = (unsigned)gc[i * 3 + 2] & mask;
    const unsigned long long b = (unsigned long long)batch[i] << (3 * depth);
    for (int j = 0; j < k; ++j) {
        const int o = (orders >> (4 * j)) & 15;
        const unsigned a0 = (o & 1) ? y : x, a1 = (o & 1) ? x : y;
        const unsigned long long c = (o & 2) ? hilbert3(a0, a1, z, depth) : interleave3(a0, a1, z, depth);
        code[(size_t)j * n + i] = (long long)(b | c);
    }
}

__global__ __launch_bounds__(TB) void k_split(long n, const long long *__restrict__ code, unsigned *__restrict__ klo, unsigned *__restrict__ khi,
                                              unsigned *__restrict__ pay) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const unsigned long long c = (unsigned long long)code[i];
    klo[i] = (unsigned)(c & 0xffffffffull);
    khi[i] = (unsigned)(c >> 32);
    pay[i] = (unsigned)i;
}

__global__ __launch_bounds__(TB) void k_gather_u32(long n, const unsigned *__restrict__ src, const unsigned *__restrict__ order,
                                                   unsigned *__restrict__ out) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) { const unsigned j = order[i]; out[i] = j < (unsigned long)n ? src[j] : 0u; }
}

__global__ __launch_bounds__(TB) void k_order_out(long n, const unsigned *__restrict__ order, long long *__restrict__ out, long long *__restrict__ inv) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const unsigned p = order[i];
    out[i] = (long long)p;
    if ((unsigned long)p < (unsigned long)n) inv[p] = (long long)i;
}

__device__ __forceinline__ bool row_ok(long long r, long n) { return r >= 0 && r < (long long)n; }

__device__ __forceinline__ bool starts_run(long i, long n, int shift, const long long *code, const long long *order) {
    if (i == 0) return true;
    const long long a = order[i], b = order[i - 1];
    if (!row_ok(a, n) || !row_ok(b, n)) return true;
    return (code[a] >> shift) != (code[b] >> shift);
}

__global__ __launch_bounds__(TB) void k_flags(long n, int shift, const long long *__restrict__ code, const long long *__restrict__ order,
                                              unsigned *__restrict__ flag) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) flag[i] = starts_run(i, n, shift, code, order) ? 1u : 0u;
}

__global__ __launch_bounds__(TB) void k_assign(long n, int shift, const long long *__restrict__ code, const long long *__restrict__ order,
                                               const unsigned *__restrict__ flag, const unsigned *__restrict__ ftot,
                                               long long *__restrict__ cluster, int *__restrict__ idx_ptr) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const bool f = starts_run(i, n, shift, code, order);
    const unsigned rank = tile_sort::scanned(flag, ftot, (size_t)i) + (f ? 1u : 0u) - 1u;
    const long long p = order[i];
    if (!row_ok(p, n) || (unsigned long)rank >= (unsigned long)n) return;   // (never taken for a permutation)
    cluster[p] = (long long)rank;
    if (f) idx_ptr[rank] = (int)i;
    if (i == n - 1) idx_ptr[rank + 1] = (int)n;
}

// position i of the serialized order -> its row's place among the rows of its run, by row index (runs are short: <= 8^pooling_depth
// distinct sites, more only among duplicated sites)
__global__ __launch_bounds__(TB) void k_rows(long n, const long long *__restrict__ order, const long long *__restrict__ cluster,
                                             const int *__restrict__ idx_ptr, int *__restrict__ sorted, long long *__restrict__ head) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const long long p = order[i];
    if (!row_ok(p, n)) return;
    const long long rank = cluster[p];
    if (rank < 0 || rank >= (long long)n) return;
    const int a = idx_ptr[rank], z = idx_ptr[rank + 1];
    if (a < 0 || z > n || a > i || z <= i) return;
    int before = 0;
    for (int t = a; t < z; ++t) before += order[t] < p ? 1 : 0;
    sorted[a + before] = (int)p;
    if (before == 0) head[rank] = p;
}

struct Workspace {
    unsigned *k32[2], *khi, *pay[2], *hist, *gtot, *flag, *ftot;
};

size_t carve(void *base, long n, Workspace &w) {
    PdfCarver cv{static_cast<char *>(base)};
    const size_t nt = (size_t)((n + tile_sort::TILE - 1) / tile_sort::TILE);
    w.k32[0] = cv.take<unsigned>((size_t)n);
    w.k32[1] = cv.take<unsigned>((size_t)n);
    w.khi = cv.take<unsigned>((size_t)n);
    w.pay[0] = cv.take<unsigned>((size_t)n);
    w.pay[1] = cv.take<unsigned>((size_t)n);
    w.hist = cv.take<unsigned>(nt * tile_sort::RADIX);
    w.gtot = cv.take<unsigned>(tile_sort::chunks(nt * tile_sort::RADIX));
    w.flag = cv.take<unsigned>((size_t)n);
    w.ftot = cv.take<unsigned>(tile_sort::chunks((size_t)n));
    return cv.off;
}

inline unsigned blocks(long total) { return (unsigned)((total + TB - 1) / TB); }

}  // namespace
}  // namespace sz

extern "C" long pdf_serial_workspace_bytes(long n) {
    if (n < 1 || n >= (1L << 31) - 2) return 0;
    sz::Workspace w;
    return (long)sz::carve(nullptr, n, w);
}

extern "C" int pdf_serial_codes(long n, int k, int orders, int depth, const int *grid_coord, const long long *batch, long long *code,
                                void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || n >= (1L << 31) - 2 || k < 1 || k > 8 || depth < 0 || depth > 16 || !grid_coord || !batch || !code) return PDF_ERR_BAD_ARG;
    for (int j = 0; j < k; ++j)
        if (((orders >> (4 * j)) & 15) > 3) return PDF_ERR_BAD_ARG;
    sz::k_codes<<<sz::blocks(n), sz::TB, 0, static_cast<hipStream_t>(stream)>>>(n, k, orders, depth, grid_coord, batch, code);
    return pdf_launch_status();
}

extern "C" int pdf_serial_sort(long n, int k, const long long *code, long long *order, long long *inverse, void *workspace, void *stream) {
    if (n < 1 || n >= (1L << 31) - 2 || k < 1 || !code || !order || !inverse || !workspace || ((uintptr_t)workspace % 256)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    sz::Workspace w;
    sz::carve(workspace, n, w);
    const unsigned nb = sz::blocks(n);
    for (int j = 0; j < k; ++j) {
        sz::k_split<<<nb, sz::TB, 0, s>>>(n, code + (size_t)j * n, w.k32[0], w.khi, w.pay[0]);
        int cur = tile_sort::sort<unsigned, true>(n, 1, w.k32, w.pay, w.hist, w.gtot, s);
        unsigned *k2[2] = {w.k32[cur ^ 1], w.k32[cur]};
        unsigned *p2[2] = {w.pay[cur], w.pay[cur ^ 1]};
        sz::k_gather_u32<<<nb, sz::TB, 0, s>>>(n, w.khi, p2[0], k2[0]);
        cur = tile_sort::sort<unsigned, true>(n, 1, k2, p2, w.hist, w.gtot, s);
        sz::k_order_out<<<nb, sz::TB, 0, s>>>(n, p2[cur], order + (size_t)j * n, inverse + (size_t)j * n);
    }
    return pdf_launch_status();
}

extern "C" int pdf_serial_pool_partition(long n, int shift, const long long *code0, const long long *order0, long long *cluster, int *sorted,
                                         int *idx_ptr, long long *head, int *count, void *workspace, void *stream) {
    if (n < 1 || n >= (1L << 31) - 2 || shift < 0 || shift > 62 || !code0 || !order0 || !cluster || !sorted || !idx_ptr || !head || !count
        || !workspace || ((uintptr_t)workspace % 256))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    sz::Workspace w;
    sz::carve(workspace, n, w);
    const unsigned nb = sz::blocks(n);
    sz::k_flags<<<nb, sz::TB, 0, s>>>(n, shift, code0, order0, w.flag);
    const long fchunks = (long)tile_sort::chunks((size_t)n);
    tile_sort::k_ts_scan_chunks<<<(unsigned)fchunks, tile_sort::LB, 0, s>>>(n, w.flag, w.ftot);
    tile_sort::k_ts_scan_short<<<1, tile_sort::LB, 0, s>>>((int)fchunks, w.ftot, reinterpret_cast<unsigned *>(count));
    sz::k_assign<<<nb, sz::TB, 0, s>>>(n, shift, code0, order0, w.flag, w.ftot, cluster, idx_ptr);
    sz::k_rows<<<nb, sz::TB, 0, s>>>(n, order0, cluster, idx_ptr, sorted, head);
    return pdf_launch_status();
}
