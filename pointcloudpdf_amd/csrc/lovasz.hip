// Lovasz-softmax over (N, C <= 64) logits, multiclass, whole batch (pointcept/models/losses/lovasz.py:89-164, 241-257 with
// per_image=False), as a capturable pass: no host read (the reference loops over labels.unique() and tests fg.sum() == 0), no torch
// sort / cumsum / dot, no atomics on floats, nothing to zero beforehand, a fixed order for every sum (bit-reproducible).
//
//   k_lv_keys     lane = row: softmax in registers -> prob; per (class, row) the sort key ~bits(e), e = |fg - p| (a non-negative float:
//                 its bit pattern is monotone as an unsigned integer, the complement sorts descending; ignored rows get the last key
//                 0xFFFFFFFF) and the payload row | fg << 31, both class-major (C segments of N).
//   4 x (k_ts_hist, k_ts_scan_segments, k_ts_scatter)
//                 the batched stable radix sort of csrc/tile_sort.h, segment = class, one-level scan: equal keys keep ascending row order.
//   k_lv_fgcount, k_ts_scan_short
//                 foreground count of every tile of the sorted order, its exclusive scan and the class totals G.
//   k_lv_grad     F_i = inclusive foreground count, I = G - F_i, U = G + (i + 1) - F_i.  J_i - J_{i-1} from the integer counts in double
//                 without a difference of two nearly equal quotients: 1 / U on a foreground element, I / (U (U - 1)) on a background
//                 one (U_{i-1} = U or U - 1, I_{i-1} = I + 1 or I).  d loss / d P = sign(p - fg) grad / #classes, scattered to
//                 (row, class): every entry is written exactly once (zero for an absent or masked class, an ignored row or e == 0, where
//                 |.| has gradient 0).  The tile's sum of e * grad goes to its own slot, in double.
//   k_lv_loss     one workgroup: per class the tile sums in a fixed order, the classes in ascending order, / #classes; NaN when a label
//                 is neither `ignore` nor a class id.
//   k_lv_softmax_bwd
//                 dlogits[n, j] = P[n, j] (g[n, j] - sum_k g[n, k] P[n, k]), in place over the buffer that held d loss / d P.
// An element with key 0xFFFFFFFF is an ignored row or has e == 0: it contributes nothing either way, so the two may share the key
// (ignored rows are background, and every element with e > 0 sorts before them: no count that matters sees them).
// Bound: HBM (the sort moves 16 NC bytes per pass, four passes).
#include "slot_sum.h"
#include "tile_sort.h"

namespace {

using namespace tile_sort;   // LB, ITEMS, TILE, WAVES, RADIX, pos: the sort's tile geometry is this pass's too

constexpr int MAXC = 64;
constexpr unsigned LAST_KEY = 0xFFFFFFFFu;

template <int W>
__global__ __launch_bounds__(LB) void k_lv_keys(long n, int c, const float *__restrict__ logits, const long *__restrict__ target, long ignore,
                                                float *__restrict__ prob, unsigned *__restrict__ keys, unsigned *__restrict__ vals,
                                                unsigned *__restrict__ bad) {
    int anybad = 0;
    for (int k = 0; k < ITEMS; ++k) {
        const long r = (long)blockIdx.x * TILE + k * LB + threadIdx.x;
        if (r >= n) break;
        const float *x = logits + r * c;
        float a[W];
        float m = -__builtin_huge_valf();
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < c) { a[j] = x[j]; m = fmaxf(m, a[j]); }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < c) { a[j] = expf(a[j] - m); s += a[j]; }
        const long t = target[r];
        const bool ign = t == ignore;
        // a label that is neither the ignore value nor a class id poisons the loss (as csrc/loss.hip); its row counts as background
        if (!ign && (t < 0 || t >= c)) anybad = 1;
        float *p = prob + r * c;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (j < c) {
                const float pj = a[j] / s;
                const bool fg = !ign && j == t;
                const float e = fabsf((fg ? 1.f : 0.f) - pj);
                p[j] = pj;
                keys[(size_t)j * n + r] = ign ? LAST_KEY : ~__float_as_uint(e);
                vals[(size_t)j * n + r] = (unsigned)r | (fg ? 0x80000000u : 0u);
            }
        }
    }
    anybad = __syncthreads_or(anybad);
    if (threadIdx.x == 0) bad[blockIdx.x] = (unsigned)anybad;
}

// fgcnt[cls * ntiles + tile] = foreground elements among the tile's sorted positions
__global__ __launch_bounds__(LB) void k_lv_fgcount(long n, int ntiles, const unsigned *__restrict__ vals, unsigned *__restrict__ fgcnt) {
    const int tile = blockIdx.x, cls = blockIdx.y;
    const unsigned *v = vals + (size_t)cls * n;
    unsigned cntv[1] = {0u}, a[1];
    for (int i = 0; i < ITEMS; ++i) {
        const size_t p = (size_t)tile * TILE + i * LB + threadIdx.x;
        cntv[0] += (unsigned)__popcll(__ballot(p < (size_t)n && (v[p] >> 31)));   // (wave-uniform: already the wave's total)
    }
    if (block_sum_wave_totals<LB>(cntv, a)) fgcnt[(size_t)cls * ntiles + tile] = a[0];
}

// a class is averaged when it occurs among the kept rows and the caller's mask (class_seen) admits it
__device__ __forceinline__ bool lv_included(int j, int c, const unsigned *total, const unsigned char *mask) {
    return j < c && total[j] > 0u && (!mask || mask[j] != 0);
}

__global__ __launch_bounds__(LB) void k_lv_grad(long n, int c, int ntiles, const unsigned *__restrict__ keys, const unsigned *__restrict__ vals,
                                                const unsigned *__restrict__ fgoff, const unsigned *__restrict__ total,
                                                const unsigned char *__restrict__ mask, float *__restrict__ dprob, double *__restrict__ part) {
    __shared__ unsigned wtot[WAVES];
    const int tile = blockIdx.x, cls = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t seg = (size_t)cls * n;
    const int ncls = __popcll(__ballot(lv_included(lane, c, total, mask)));
    const bool inc = lv_included(cls, c, total, mask);
    unsigned key[ITEMS], val[ITEMS];
    unsigned long long fgm[ITEMS];
    unsigned mine = 0u;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const size_t p = pos(tile, w, r, lane);
        const bool valid = p < (size_t)n;
        key[r] = valid ? keys[seg + p] : LAST_KEY;
        val[r] = valid ? vals[seg + p] : 0u;
        fgm[r] = __ballot(val[r] >> 31);
        mine += (unsigned)__popcll(fgm[r]);
    }
    if (lane == 0) wtot[w] = mine;
    __syncthreads();
    unsigned run = fgoff[(size_t)cls * ntiles + tile];
    for (int i = 0; i < w; ++i) run += wtot[i];
    const double g = (double)total[cls], inv_ncls = inc ? 1.0 / (double)ncls : 0.0;
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    double acc[1] = {0.0};
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const size_t p = pos(tile, w, r, lane);
        const bool fg = val[r] >> 31;
        const double f = (double)(run + (unsigned)__popcll(fgm[r] & upto));
        run += (unsigned)__popcll(fgm[r]);
        if (p >= (size_t)n) continue;
        float out = 0.f;
        if (inc && key[r] != LAST_KEY) {   // (an absent class has g == 0: never divided by)
            const double i_ = g - f, u = g + (double)(p + 1) - f;
            const double gr = fg ? 1.0 / u : i_ / (u * (u - 1.0));
            acc[0] += (double)__uint_as_float(~key[r]) * gr;
            out = (float)((fg ? -gr : gr) * inv_ncls);
        }
        dprob[(size_t)(val[r] & 0x7FFFFFFFu) * c + cls] = out;
    }
    block_sum_by_waves<LB>(acc, part + (size_t)cls * ntiles + tile);
}

// out = [loss, number of classes averaged].  One workgroup; per class the slot_total of its tiles, the classes in ascending order.
__global__ __launch_bounds__(LB) void k_lv_loss(int c, int ntiles, const double *__restrict__ part, const unsigned *__restrict__ total,
                                                const unsigned char *__restrict__ mask, const unsigned *__restrict__ bad, float *__restrict__ out) {
    int anybad = 0;
    for (int t = threadIdx.x; t < ntiles; t += LB) anybad |= bad[t] != 0u;
    anybad = __syncthreads_or(anybad);
    double loss = 0.0;
    int ncls = 0;
    for (int j = 0; j < c; ++j) {
        if (!lv_included(j, c, total, mask)) continue;   // (workgroup-uniform)
        double b[1];
        if (slot_total<LB>(part + (size_t)j * ntiles, ntiles, b)) loss += b[0];
        ++ncls;
    }
    if (threadIdx.x != 0) return;
    out[0] = anybad ? __builtin_nanf("") : (ncls ? (float)(loss / (double)ncls) : 0.f);
    out[1] = (float)ncls;
}

template <int W>
__global__ __launch_bounds__(LB) void k_lv_softmax_bwd(long n, int c, const float *__restrict__ prob, float *__restrict__ g) {
    for (long r = (long)blockIdx.x * LB + threadIdx.x; r < n; r += (long)gridDim.x * LB) {
        const float *p = prob + r * c;
        float *gr = g + r * c;
        float a[W];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < c) { a[j] = gr[j]; dot += a[j] * p[j]; }
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < c) gr[j] = p[j] * (a[j] - dot);
    }
}

// grad_out = dlogits * gy * scale.  The forward's buffer is only READ (retain_graph: a second backward sees the same values).
__global__ __launch_bounds__(LB) void k_lv_bwd(long total, const float *__restrict__ dlogits, const float *__restrict__ gy, float scale,
                                               float *__restrict__ out) {
    pdf_scaled_copy<LB>(total, dlogits, gy[0] * scale, out);
}

struct LvWorkspace {
    unsigned *keys[2], *vals[2], *hist, *fgcnt, *total, *bad;
    double *part;
    size_t bytes;
};

LvWorkspace lv_carve(char *base, long n, int c) {
    const size_t nt = (size_t)((n + TILE - 1) / TILE), nc = (size_t)n * c;
    LvWorkspace w;
    PdfCarver ws{base};
    w.part = ws.take<double>(nt * c);
    for (int i = 0; i < 2; ++i) w.keys[i] = ws.take<unsigned>(nc);
    for (int i = 0; i < 2; ++i) w.vals[i] = ws.take<unsigned>(nc);
    w.hist = ws.take<unsigned>(nt * c * RADIX);
    w.fgcnt = ws.take<unsigned>(nt * c);
    w.total = ws.take<unsigned>((size_t)MAXC);
    w.bad = ws.take<unsigned>(nt);
    w.bytes = ws.off;
    return w;
}

bool lv_shape_ok(long n, int c) { return n >= 1 && n < 0x7FFFFFFFL && c >= 1; }

}  // namespace

extern "C" long pdf_lovasz_workspace_bytes(long n, int c) {
    if (!lv_shape_ok(n, c) || c > MAXC) return 0;
    return (long)lv_carve(nullptr, n, c).bytes;
}

extern "C" int pdf_lovasz_forward(long n, int c, const float *logits, const long *target, long ignore, const unsigned char *class_mask,
                                  float *prob, float *dlogits, float *loss, void *workspace, void *stream) {
    if (!lv_shape_ok(n, c) || !logits || !target || !prob || !dlogits || !loss || !workspace) return PDF_ERR_BAD_ARG;
    if (c > MAXC) return PDF_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LvWorkspace w = lv_carve(static_cast<char *>(workspace), n, c);
    const int nt = (int)((n + TILE - 1) / TILE);
    const dim3 grid((unsigned)nt, (unsigned)c);
    if (c <= 16) k_lv_keys<16><<<(unsigned)nt, LB, 0, s>>>(n, c, logits, target, ignore, prob, w.keys[0], w.vals[0], w.bad);
    else if (c <= 32) k_lv_keys<32><<<(unsigned)nt, LB, 0, s>>>(n, c, logits, target, ignore, prob, w.keys[0], w.vals[0], w.bad);
    else k_lv_keys<MAXC><<<(unsigned)nt, LB, 0, s>>>(n, c, logits, target, ignore, prob, w.keys[0], w.vals[0], w.bad);
    const int cur = sort<unsigned, false>(n, c, w.keys, w.vals, w.hist, nullptr, s);
    k_lv_fgcount<<<grid, LB, 0, s>>>(n, nt, w.vals[cur], w.fgcnt);
    k_ts_scan_short<<<(unsigned)c, LB, 0, s>>>(nt, w.fgcnt, w.total);   // -> foreground before the tile; total[cls] = G
    k_lv_grad<<<grid, LB, 0, s>>>(n, c, nt, w.keys[cur], w.vals[cur], w.fgcnt, w.total, class_mask, dlogits, w.part);
    k_lv_loss<<<1, LB, 0, s>>>(c, nt, w.part, w.total, class_mask, w.bad, loss);
    long g = (n + LB - 1) / LB;
    if (g > PDF_MAX_BLOCKS) g = PDF_MAX_BLOCKS;
    if (c <= 16) k_lv_softmax_bwd<16><<<(unsigned)g, LB, 0, s>>>(n, c, prob, dlogits);
    else if (c <= 32) k_lv_softmax_bwd<32><<<(unsigned)g, LB, 0, s>>>(n, c, prob, dlogits);
    else k_lv_softmax_bwd<MAXC><<<(unsigned)g, LB, 0, s>>>(n, c, prob, dlogits);
    return pdf_launch_status();
}

extern "C" int pdf_lovasz_backward(long n, int c, const float *dlogits, const float *gy, float scale, float *grad_out, void *stream) {
    if (n < 1 || c < 1 || !dlogits || !gy || !grad_out) return PDF_ERR_BAD_ARG;
    long g = (n * c + LB - 1) / LB;
    if (g > PDF_MAX_BLOCKS) g = PDF_MAX_BLOCKS;
    k_lv_bwd<<<(unsigned)g, LB, 0, static_cast<hipStream_t>(stream)>>>(n * c, dlogits, gy, scale, grad_out);
    return pdf_launch_status();
}
