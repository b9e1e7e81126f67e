// Partition-based pooling of PointTransformer-V2 (point_transformer_v2m2_base.py:244-269, :308-309) as launches on the caller's stream:
// no float atomics, fixed summation orders, nothing allocated.
//
//   pdf_grid_pool_partition  keys -> stable sort -> run boundaries: cluster (rank of every point's cell among the distinct cells),
//                            the sort order, idx_ptr and the cluster count (one int the caller reads)
//   pdf_grid_pool_reduce     pooled coord = segment mean (rows added in ascending point order in fp32, one fp32 division by the count),
//                            pooled feat = segment max with the arg-max row saved (the first row in point order wins a tie)
//   pdf_grid_pool_max_backward   every fine row takes grad_out[cluster[i], c] where it is the saved arg-max, else 0 (a gather)
//   pdf_grid_unpool_forward      map unpooling: out[i] = x[cluster[i]] (its backward is pdf_seg_sum_rows over (idx_ptr, sort order))
//
// The key is the cell id of torch_geometric's voxel_grid on (coord - start[scene]) with start = 0 (stratified._voxel_grid): per axis
// cell = floor_divide(pos, size) in fp32 -- torch's floor division (c10::div_floor_floating: fmod, exact quotient of the remainder-free
// part, floor, round-up guard), restated below --, x fastest, the scene as the slowest axis, extents from the batch-wide maximum of pos.
// pos is monotone in the coordinate (one rounding), so that maximum is max over the scenes of hi[scene] - lo[scene]: no reduction over
// the points is needed.  The id is an int64 quantity (100 m at a 0.01 m cell: 10^12 cells): the stable sort runs as two stable 32-bit
// sorts (csrc/tile_sort.h), low word first.  This TU is compiled with -ffp-contract=off.
#include "tile_sort.h"

namespace gp {
namespace {

constexpr int TB = 256;

// torch.div(a, b, rounding_mode="floor") for floats (c10/util/generic_math.h: div_floor_floating), a >= 0 or not, b > 0
__device__ __forceinline__ float div_floor(float a, float b) {
    if (b == 0.f) return a / b;
    const float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.f;
    if (div != 0.f) {
        float fl = floorf(div);
        if (div - fl > 0.5f) fl += 1.f;
        return fl;
    }
    return copysignf(0.f, a / b);
}

// num[d] = max(1, floor_divide(max over the scenes of (hi - lo)[d], size) + 1), d = x, y, z
__global__ void k_extent(int scenes, const float *__restrict__ lo, const float *__restrict__ hi, float size, long long *__restrict__ num) {
    const int d = threadIdx.x;
    if (d >= 3) return;
    float e = -INFINITY;
    for (int b = 0; b < scenes; ++b) e = fmaxf(e, hi[b * 3 + d] - lo[b * 3 + d]);
    long long v = (long long)div_floor(e, size) + 1;
    num[d] = v < 1 ? 1 : v;
}

__global__ __launch_bounds__(TB) void k_keys(long n, const float *__restrict__ xyz, const int *__restrict__ ends, int scenes,
                                             const float *__restrict__ lo, float size, const long long *__restrict__ num,
                                             long long *__restrict__ key, unsigned *__restrict__ klo, unsigned *__restrict__ khi,
                                             unsigned *__restrict__ pay) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    int a = 0, z = scenes - 1;   // the scene of point i: the first b with i < ends[b]
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (i < (long)ends[mid]) z = mid; else a = mid + 1;
    }
    const long long nx = num[0], ny = num[1], nz = num[2];
    const long long cx = (long long)div_floor(xyz[i * 3 + 0] - lo[a * 3 + 0], size);
    const long long cy = (long long)div_floor(xyz[i * 3 + 1] - lo[a * 3 + 1], size);
    const long long cz = (long long)div_floor(xyz[i * 3 + 2] - lo[a * 3 + 2], size);
    const long long k = cx + cy * nx + cz * (nx * ny) + (long long)a * (nx * ny * nz);
    key[i] = k;
    klo[i] = (unsigned)((unsigned long long)k & 0xffffffffull);
    khi[i] = (unsigned)((unsigned long long)k >> 32);
    pay[i] = (unsigned)i;
}

__global__ __launch_bounds__(TB) void k_gather_u32(long n, const unsigned *__restrict__ src, const unsigned *__restrict__ order,
                                                   unsigned *__restrict__ out) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) { const unsigned j = order[i]; out[i] = j < (unsigned long)n ? src[j] : 0u; }
}

__device__ __forceinline__ bool starts_run(long i, const long long *key, const unsigned *order) {
    return i == 0 || key[order[i]] != key[order[i - 1]];
}

__global__ __launch_bounds__(TB) void k_flags(long n, const long long *__restrict__ key, const unsigned *__restrict__ order,
                                              unsigned *__restrict__ flag) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) flag[i] = starts_run(i, key, order) ? 1u : 0u;
}

// flag: exclusive prefix of the run starts (two-level scan of csrc/tile_sort.h) -> rank of position i = runs started before i + (i starts one) - 1
__global__ __launch_bounds__(TB) void k_assign(long n, const long long *__restrict__ key, const unsigned *__restrict__ order,
                                               const unsigned *__restrict__ flag, const unsigned *__restrict__ ftot,
                                               long long *__restrict__ cluster, int *__restrict__ sorted, int *__restrict__ idx_ptr) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const bool f = starts_run(i, key, order);
    const unsigned rank = tile_sort::scanned(flag, ftot, (size_t)i) + (f ? 1u : 0u) - 1u;
    const unsigned p = order[i];
    if ((unsigned long)p >= (unsigned long)n || (unsigned long)rank >= (unsigned long)n) return;   // (never taken)
    cluster[p] = (long long)rank;
    sorted[i] = (int)p;
    if (f) idx_ptr[rank] = (int)i;
    if (i == n - 1) idx_ptr[rank + 1] = (int)n;
}

// one thread per segment: the three coordinate sums in ascending sorted position, then one division
__global__ __launch_bounds__(TB) void k_mean3(long n, long m, const float *__restrict__ xyz, const int *__restrict__ idx_ptr,
                                              const int *__restrict__ sorted, float *__restrict__ out) {
    const long j = (long)blockIdx.x * TB + threadIdx.x;
    if (j >= m) return;
    const int a = idx_ptr[j], z = idx_ptr[j + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int t = a; t < z; ++t) {
        const long r = sorted[t];
        if (r < 0 || r >= n) continue;
        if (t == a) { sx = xyz[r * 3]; sy = xyz[r * 3 + 1]; sz = xyz[r * 3 + 2]; }
        else { sx += xyz[r * 3]; sy += xyz[r * 3 + 1]; sz += xyz[r * 3 + 2]; }
    }
    const float cnt = (float)(z - a);
    out[j * 3] = sx / cnt; out[j * 3 + 1] = sy / cnt; out[j * 3 + 2] = sz / cnt;
}

// one thread per (segment, channel), channel fastest: rows read coalesced
__global__ __launch_bounds__(TB) void k_max(long n, long total, int c, const float *__restrict__ feat, const int *__restrict__ idx_ptr,
                                            const int *__restrict__ sorted, float *__restrict__ out, int *__restrict__ arg) {
    for (long g = (long)blockIdx.x * TB + threadIdx.x; g < total; g += (long)gridDim.x * TB) {
        const long j = g / c;
        const int ch = (int)(g - j * c);
        const int a = idx_ptr[j], z = idx_ptr[j + 1];
        float best = 0.f;
        int who = -1;
        for (int t = a; t < z; ++t) {
            const long r = sorted[t];
            if (r < 0 || r >= n) continue;
            const float v = feat[r * c + ch];
            if (who < 0 || v > best) { best = v; who = (int)r; }
        }
        out[g] = best;
        arg[g] = who;
    }
}

__global__ __launch_bounds__(TB) void k_max_bwd(long total, long m, int c, const float *__restrict__ g_out, const long long *__restrict__ cluster,
                                                const int *__restrict__ arg, float *__restrict__ g_in) {
    for (long g = (long)blockIdx.x * TB + threadIdx.x; g < total; g += (long)gridDim.x * TB) {
        const long i = g / c;
        const int ch = (int)(g - i * c);
        const long long j = cluster[i];
        float v = 0.f;
        if (j >= 0 && j < m && (long)arg[j * c + ch] == i) v = g_out[j * c + ch];
        g_in[g] = v;
    }
}

__global__ __launch_bounds__(TB) void k_unpool(long total, long m, int c, const float *__restrict__ x, const long long *__restrict__ cluster,
                                               float *__restrict__ out) {
    for (long g = (long)blockIdx.x * TB + threadIdx.x; g < total; g += (long)gridDim.x * TB) {
        const long i = g / c;
        const int ch = (int)(g - i * c);
        const long long j = cluster[i];
        out[g] = (j >= 0 && j < m) ? x[j * c + ch] : 0.f;
    }
}

struct Workspace {
    long long *key, *num;
    unsigned *k32[2], *khi, *pay[2], *hist, *gtot, *flag, *ftot;
};

size_t carve(void *base, long n, Workspace &w) {
    PdfCarver cv{static_cast<char *>(base)};
    const size_t nt = (size_t)((n + tile_sort::TILE - 1) / tile_sort::TILE);
    w.key = cv.take<long long>((size_t)n);
    w.num = cv.take<long long>(4);
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
inline unsigned capped(long total) { const long b = (total + TB - 1) / TB; return (unsigned)(b < 8 * PDF_MAX_BLOCKS ? b : 8 * PDF_MAX_BLOCKS); }

}  // namespace
}  // namespace gp

extern "C" long pdf_grid_pool_workspace_bytes(long n) {
    if (n < 1 || n >= (1L << 31) - 2) return 0;
    gp::Workspace w;
    return (long)gp::carve(nullptr, n, w);
}

// xyz (n, 3); ends (scenes) ascending scene ends, the last one = n; lo / hi (scenes, 3): pdf_scene_bounds.  -> cluster (n) int64,
// sorted (n) int32 (stable ascending order of the keys), idx_ptr (n + 1) int32 of which the first count[0] + 1 entries are written,
// count (1) int32 = number of clusters.
extern "C" int pdf_grid_pool_partition(long n, const float *xyz, const int *ends, int scenes, const float *lo, const float *hi, float size,
                                       long long *cluster, int *sorted, int *idx_ptr, int *count, void *workspace, void *stream) {
    if (n < 1 || n >= (1L << 31) - 2 || scenes < 1 || !xyz || !ends || !lo || !hi || !cluster || !sorted || !idx_ptr || !count || !workspace
        || !(size > 0.f) || ((uintptr_t)workspace % 256))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    gp::Workspace w;
    gp::carve(workspace, n, w);
    const unsigned nb = gp::blocks(n);
    gp::k_extent<<<1, 64, 0, s>>>(scenes, lo, hi, size, w.num);
    gp::k_keys<<<nb, gp::TB, 0, s>>>(n, xyz, ends, scenes, lo, size, w.num, w.key, w.k32[0], w.khi, w.pay[0]);
    // low word: four passes, the result is back in buffer 0
    int cur = tile_sort::sort<unsigned, true>(n, 1, w.k32, w.pay, w.hist, w.gtot, s);
    // high word of the keys in that order, then the second stable sort (equal high words keep the low-word order)
    unsigned *k2[2] = {w.k32[cur ^ 1], w.k32[cur]};
    unsigned *p2[2] = {w.pay[cur], w.pay[cur ^ 1]};
    gp::k_gather_u32<<<nb, gp::TB, 0, s>>>(n, w.khi, p2[0], k2[0]);
    cur = tile_sort::sort<unsigned, true>(n, 1, k2, p2, w.hist, w.gtot, s);
    const unsigned *order = p2[cur];
    gp::k_flags<<<nb, gp::TB, 0, s>>>(n, w.key, order, w.flag);
    const long fchunks = (long)tile_sort::chunks((size_t)n);
    tile_sort::k_ts_scan_chunks<<<(unsigned)fchunks, tile_sort::LB, 0, s>>>(n, w.flag, w.ftot);
    tile_sort::k_ts_scan_short<<<1, tile_sort::LB, 0, s>>>((int)fchunks, w.ftot, reinterpret_cast<unsigned *>(count));
    gp::k_assign<<<nb, gp::TB, 0, s>>>(n, w.key, order, w.flag, w.ftot, cluster, sorted, idx_ptr);
    return pdf_launch_status();
}

// xyz (n, 3) -> coord_out (m, 3) (both or neither); feat (n, c) -> feat_out (m, c), arg_out (m, c) int32 = the fine row that holds the
// maximum (all three or none).
extern "C" int pdf_grid_pool_reduce(long n, long m, int c, const float *xyz, const float *feat, const int *idx_ptr, const int *sorted,
                                    float *coord_out, float *feat_out, int *arg_out, void *stream) {
    if (m == 0) return PDF_OK;
    if (n < 1 || m < 0 || m > n || !idx_ptr || !sorted || (!xyz != !coord_out) || (!feat != !feat_out) || (!feat != !arg_out) || (feat && c < 1))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (xyz) gp::k_mean3<<<gp::blocks(m), gp::TB, 0, s>>>(n, m, xyz, idx_ptr, sorted, coord_out);
    if (feat) gp::k_max<<<gp::capped(m * c), gp::TB, 0, s>>>(n, m * c, c, feat, idx_ptr, sorted, feat_out, arg_out);
    return pdf_launch_status();
}

extern "C" int pdf_grid_pool_max_backward(long n, long m, int c, const float *grad_out, const long long *cluster, const int *arg, float *grad_in,
                                          void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || m < 1 || c < 1 || !grad_out || !cluster || !arg || !grad_in) return PDF_ERR_BAD_ARG;
    gp::k_max_bwd<<<gp::capped(n * c), gp::TB, 0, static_cast<hipStream_t>(stream)>>>(n * c, m, c, grad_out, cluster, arg, grad_in);
    return pdf_launch_status();
}

extern "C" int pdf_grid_unpool_forward(long n, long m, int c, const float *x, const long long *cluster, float *out, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || m < 1 || c < 1 || !x || !cluster || !out) return PDF_ERR_BAD_ARG;
    gp::k_unpool<<<gp::capped(n * c), gp::TB, 0, static_cast<hipStream_t>(stream)>>>(n * c, m, c, x, cluster, out);
    return pdf_launch_status();
}
