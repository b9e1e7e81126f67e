// Test-time fragments of ONE augmented scene for gfx950 (pointcept/datasets/transform.py:858-887,
// pointcept/datasets/defaults.py:96-129, pointcept/engines/test.py:206-251) -- replaces, for a BATCH of G fragments per call, the
// per-fragment numpy gathers of GridSample(mode="test"), the post_transform shift + ToTensor + Collect of every fragment, collate_fn
// and the tester's per-fragment accumulation.
//
// All three entries read the fragment table of the scene (voxelize.fragment_table): order (N) = point ids, key-sorted, original order
// inside a voxel; vstart (V) / count (V) = every voxel's run in `order`; voxel_of (N) = the voxel of every sorted position.
// Fragment f holds the point  order[vstart[v] + f % count[v]]  of every voxel v, in voxel order (transform.py:861-863).
//   k_fragment_bounds_*  per-fragment min / max of the selected coordinates: a grid-stride pass per fragment into per-block slots and a
//                        one-block pass per fragment over the slots (min / max are exact: any order gives the same bits).
//   k_fragment_gather    row r = g V + v of the collated batch: index, coord - shift[g] (subtracted in the SOURCE dtype, rounded once
//                        to fp32: numpy's in-place `coord -= shift` followed by ToTensor's .float()), feat = the Collect.feat_keys
//                        concatenation, grid_coord.  One lane per row; coord and feat rows are staged in LDS and written by the whole
//                        workgroup as one contiguous run of floats (coalesced).  24 B read + (8 + 12 + 4 C + 24) B written per row.
//   k_fragment_vote      one lane per SORTED POSITION j (voxel v = voxel_of[j], slot s = j - vstart[v], point p = order[j]): the lane
//                        walks the batch's fragments f ascending and folds every f with f % count[v] == s into pred[p, :] / score_sum[p]
//                        / score_cnt[p] with pdf_vote_row (vote_row.h, the row function of k_vote).  A point is owned by one lane, so
//                        there are no atomics, every logits row is consumed exactly once, and a point's additions happen in ascending
//                        fragment order: bit-identical to G successive pdf_vote_accumulate calls.
// Bound: HBM / latency of the dependent gathers (order -> coord); nothing here has reuse.
#include "pdfops_common.h"
#include "vote_row.h"

namespace {

constexpr int LB = 256;
constexpr int PDF_FRAG_SLOTS = 128;     // per-fragment partial slots of the bounds pass
constexpr int PDF_FRAG_MAXC = 16;       // widest feat row (4 segments of at most 4 floats)

struct FeatSeg {           // one Collect.feat_keys entry: src == nullptr -> the shifted coordinate (w = 3), else an (N, w) fp32 array
    const float *src;
    int w;
};
struct FeatSegs {
    FeatSeg s[4];
};

template <typename T>
__global__ __launch_bounds__(LB) void k_fragment_bounds_part(long v, int f0, const T *__restrict__ coord, const long *__restrict__ order,
                                                             const long *__restrict__ vstart, const long *__restrict__ count,
                                                             double *__restrict__ part) {
    __shared__ double red[6][LB / 64];
    const int g = blockIdx.y;
    const long f = (long)f0 + g;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long i = (long)blockIdx.x * LB + threadIdx.x; i < v; i += (long)gridDim.x * LB) {
        const long p = order[vstart[i] + f % count[i]];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = (double)coord[3 * p + a];
            lo[a] = fmin(lo[a], x);
            hi[a] = fmax(hi[a], x);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], o, 64));
        }
        if ((threadIdx.x & 63) == 0) { red[a][threadIdx.x >> 6] = lo[a]; red[3 + a][threadIdx.x >> 6] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double r = red[threadIdx.x][0];
        for (int w = 1; w < LB / 64; ++w) r = threadIdx.x < 3 ? fmin(r, red[threadIdx.x][w]) : fmax(r, red[threadIdx.x][w]);
        part[((long)g * PDF_FRAG_SLOTS + blockIdx.x) * 6 + threadIdx.x] = r;
    }
}

// bounds[g, 0..2] = min, bounds[g, 3..5] = max over the `slots` partial rows of fragment g.  One 64-lane block per fragment.
__global__ __launch_bounds__(64) void k_fragment_bounds_final(int slots, const double *__restrict__ part, double *__restrict__ bounds) {
    const int g = blockIdx.x;
    for (int a = 0; a < 6; ++a) {
        double r = a < 3 ? (double)INFINITY : -(double)INFINITY;
        for (int s = threadIdx.x; s < slots; s += 64) {
            const double x = part[((long)g * PDF_FRAG_SLOTS + s) * 6 + a];
            r = a < 3 ? fmin(r, x) : fmax(r, x);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double y = __shfl_xor(r, o, 64);
            r = a < 3 ? fmin(r, y) : fmax(r, y);
        }
        if (threadIdx.x == 0) bounds[6 * g + a] = r;
    }
}

template <typename T>
__global__ __launch_bounds__(LB) void k_fragment_gather(long v, long rows, int f0, int g, const T *__restrict__ coord,
                                                        const long *__restrict__ order, const long *__restrict__ vstart,
                                                        const long *__restrict__ count, const T *__restrict__ shift, FeatSegs segs, int c,
                                                        const long long *__restrict__ grid_src, long *__restrict__ index,
                                                        float *__restrict__ out_coord, float *__restrict__ out_feat,
                                                        long long *__restrict__ out_grid, int *__restrict__ out_offset) {
    __shared__ float s_coord[LB * 3];
    __shared__ float s_feat[LB * PDF_FRAG_MAXC];
    const long r0 = (long)blockIdx.x * LB;
    const long r = r0 + threadIdx.x;
    if (blockIdx.x == 0 && (int)threadIdx.x < g) out_offset[threadIdx.x] = (int)((long)(threadIdx.x + 1) * v);
    if (r < rows) {
        const long gi = r / v, vi = r - gi * v;
        const long p = order[vstart[vi] + ((long)f0 + gi) % count[vi]];
        index[r] = p;
        float xyz[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xyz[a] = (float)(coord[3 * p + a] - shift[3 * gi + a]);   // the source dtype's subtraction, one rounding to fp32
            s_coord[3 * threadIdx.x + a] = xyz[a];
        }
        float *fr = s_feat + (long)threadIdx.x * c;
        int col = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int w = segs.s[k].w;
            const float *src = segs.s[k].src;
            for (int j = 0; j < w; ++j) fr[col + j] = src ? src[p * w + j] : xyz[j];
            col += w;
        }
        if (out_grid) {
#pragma unroll
            for (int a = 0; a < 3; ++a) out_grid[3 * r + a] = grid_src[3 * p + a];
        }
    }
    __syncthreads();
    const long live = rows - r0 < LB ? rows - r0 : LB;   // rows of this block
    for (long e = threadIdx.x; e < live * 3; e += LB) out_coord[r0 * 3 + e] = s_coord[e];
    for (long e = threadIdx.x; e < live * c; e += LB) out_feat[r0 * c + e] = s_feat[e];
}

__global__ __launch_bounds__(LB) void k_fragment_vote(long n, long v, int f0, int g, int c, const float *__restrict__ logits,
                                                      const float *__restrict__ score, const long *__restrict__ order,
                                                      const long *__restrict__ vstart, const long *__restrict__ count,
                                                      const long *__restrict__ voxel_of, float *__restrict__ pred,
                                                      float *__restrict__ score_sum, float *__restrict__ score_cnt) {
    for (long j = (long)blockIdx.x * LB + threadIdx.x; j < n; j += (long)gridDim.x * LB) {
        const long vi = voxel_of[j];
        const long cnt = count[vi], s = j - vstart[vi];
        // first fragment of the batch that selects slot s of this voxel, then every cnt-th one
        long f = (long)f0 + ((s - (long)f0 % cnt) + cnt) % cnt;
        if (f >= (long)f0 + g) continue;   // (a batch shorter than the voxel's count: this point is not visited)
        const long p = order[j];
        float *dst = pred + p * c;
        for (; f < (long)f0 + g; f += cnt) {
            const long r = (f - f0) * v + vi;
            pdf_vote_row(logits + r * c, c, dst);
            if (score) { score_sum[p] += score[r]; score_cnt[p] += 1.f; }
        }
    }
}

bool bad_table(long n, long v, int f0, int g, const void *order, const void *vstart, const void *count) {
    return n < 0 || v < 0 || v > n || f0 < 0 || g < 1 || !order || !vstart || !count;
}

}  // namespace

extern "C" long pdf_fragment_bounds_ws_doubles(int g) { return g < 1 ? 0 : (long)g * PDF_FRAG_SLOTS * 6; }

// bounds (g, 6) float64 = [min xyz | max xyz] of the coordinates fragments f0 .. f0 + g - 1 select (exact for fp32 sources as well:
// every fp32 value is a double).  coord (n, 3) of dtype fp32 (f64 = 0) or fp64 (f64 = 1); ws: pdf_fragment_bounds_ws_doubles(g) doubles.
extern "C" int pdf_fragment_bounds(long n, long v, int f0, int g, int f64, const void *coord, const long *order, const long *vstart,
                                   const long *count, double *ws, double *bounds, void *stream) {
    if (bad_table(n, v, f0, g, order, vstart, count) || !coord || !ws || !bounds || (f64 != 0 && f64 != 1)) return PDF_ERR_BAD_ARG;
    if (v == 0) return PDF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long slots = (v + LB - 1) / LB;
    if (slots > PDF_FRAG_SLOTS) slots = PDF_FRAG_SLOTS;
    const dim3 grid((unsigned)slots, (unsigned)g);
    if (f64) k_fragment_bounds_part<double><<<grid, LB, 0, s>>>(v, f0, static_cast<const double *>(coord), order, vstart, count, ws);
    else k_fragment_bounds_part<float><<<grid, LB, 0, s>>>(v, f0, static_cast<const float *>(coord), order, vstart, count, ws);
    k_fragment_bounds_final<<<(unsigned)g, 64, 0, s>>>((int)slots, ws, bounds);
    return pdf_launch_status();
}

// The collated batch of fragments f0 .. f0 + g - 1 (row r = (f - f0) v + voxel): index (g v) int64, out_coord (g v, 3) fp32 =
// coord[p] - shift[f - f0] (shift (g, 3) in the dtype of coord), out_feat (g v, c) fp32 = the nseg <= 4 segments side by side -- segment
// k is the shifted coordinate when seg_src[k] is NULL (then seg_w[k] must be 3), else the (n, seg_w[k] <= 4) fp32 array seg_src[k];
// c = sum of the widths -- out_grid (g v, 3) int64 = grid_src[p] (both NULL: not written), out_offset (g) int32 = (k + 1) v.
// seg_src / seg_w are HOST arrays (read before the launch).
extern "C" int pdf_fragment_gather(long n, long v, int f0, int g, int f64, const void *coord, const long *order, const long *vstart,
                                   const long *count, const void *shift, int nseg, const float *const *seg_src, const int *seg_w,
                                   const long long *grid_src, long *index, float *out_coord, float *out_feat, long long *out_grid,
                                   int *out_offset, void *stream) {
    if (bad_table(n, v, f0, g, order, vstart, count) || !coord || !shift || !index || !out_coord || !out_feat || !out_offset ||
        (f64 != 0 && f64 != 1) || nseg < 1 || nseg > 4 || !seg_src || !seg_w || (grid_src == nullptr) != (out_grid == nullptr) || g > LB)
        return PDF_ERR_BAD_ARG;
    if (v > 0x7fffffffL / g) return PDF_ERR_BAD_ARG;   // out_offset is int32: its last entry g v must fit
    FeatSegs segs{};
    int c = 0;
    for (int k = 0; k < nseg; ++k) {
        if (seg_w[k] < 1 || seg_w[k] > 4 || (!seg_src[k] && seg_w[k] != 3)) return PDF_ERR_BAD_ARG;
        segs.s[k].src = seg_src[k];
        segs.s[k].w = seg_w[k];
        c += seg_w[k];
    }
    if (v == 0) return PDF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long rows = (long)g * v;
    const unsigned blocks = (unsigned)((rows + LB - 1) / LB);
    if (f64)
        k_fragment_gather<double><<<blocks, LB, 0, s>>>(v, rows, f0, g, static_cast<const double *>(coord), order, vstart, count,
                                                        static_cast<const double *>(shift), segs, c, grid_src, index, out_coord, out_feat,
                                                        out_grid, out_offset);
    else
        k_fragment_gather<float><<<blocks, LB, 0, s>>>(v, rows, f0, g, static_cast<const float *>(coord), order, vstart, count,
                                                       static_cast<const float *>(shift), segs, c, grid_src, index, out_coord, out_feat,
                                                       out_grid, out_offset);
    return pdf_launch_status();
}

// Fold the batch of fragments f0 .. f0 + g - 1 into the running vote: logits (g v, c), score (g v) or NULL, rows in gather order;
// pred (n, c), score_sum / score_cnt (n) as pdf_vote_accumulate keeps them.  Bit-identical to g successive pdf_vote_accumulate calls.
extern "C" int pdf_fragment_vote(long n, long v, int f0, int g, int c, const float *logits, const float *score, const long *order,
                                 const long *vstart, const long *count, const long *voxel_of, float *pred, float *score_sum,
                                 float *score_cnt, void *stream) {
    if (bad_table(n, v, f0, g, order, vstart, count) || c < 1 || !logits || !voxel_of || !pred || (score && (!score_sum || !score_cnt)))
        return PDF_ERR_BAD_ARG;
    if (v == 0) return PDF_OK;
    long blocks = (n + LB - 1) / LB;
    if (blocks > PDF_MAX_BLOCKS) blocks = PDF_MAX_BLOCKS;
    k_fragment_vote<<<(unsigned)blocks, LB, 0, static_cast<hipStream_t>(stream)>>>(n, v, f0, g, c, logits, score, order, vstart, count,
                                                                                   voxel_of, pred, score_sum, score_cnt);
    return pdf_launch_status();
}
