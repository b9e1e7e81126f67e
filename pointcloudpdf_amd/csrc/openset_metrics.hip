// Open-set metrics of one call as a capturable pass: the class histograms of evaluator.intersection_and_union (exact integer counts) and
// AUPR / AUROC of evaluator.aupr_and_auroc (what sklearn's average_precision_score / roc_auc_score compute), over n rows.  No host read,
// no torch sort / cumsum / bincount, no atomics on floats, nothing to zero beforehand, a fixed order for every sum (bit-reproducible);
// kernel boundaries are the only synchronisation between workgroups.
//
//   k_om_keys     at most HB workgroups, each over tiles b, b + grid, ...: prediction (given, or the lowest index among the row's maximal
//                 logits, a NaN counting as maximal), the LDS histogram intersection | output | target of the rows with target != ignore
//                 plus the counts [positive, valid, NaN score], stored as the workgroup's own partial row; per row the sort key and one
//                 byte of payload (1 = positive: unknown[target]).  Key = ~ordered(score) with -0.0 folded onto +0.0: ascending keys are
//                 descending scores; +-inf are ordinary values.  Ignored rows get the last key 0xFFFFFFFF and payload 0: they sort behind
//                 every valid row (the only score with that key is one NaN pattern, and a NaN on a valid row makes both areas NaN anyway).
//   k_om_sums     one workgroup per class adds the partial rows: hist = intersection | output + target - intersection | target (int64);
//                 one more workgroup the three counts -> totals.
//   4 x (k_ts_hist, k_ts_scan_chunks, k_ts_scan_short, k_ts_scatter)
//                 the stable radix sort of csrc/tile_sort.h: ONE segment of up to 2^31 - 2 keys, so with its two-level scan.
//   k_om_ends     per tile of the sorted order: positives and group ends (a key that differs from its successor's; the last key of a
//                 tile reads the first key of the next tile) -> counts [positives (tiles) | ends (tiles)], scanned by the sort's two-level
//                 scan (k_ts_scan_chunks, k_ts_scan_short).
//   k_om_walk     tp (inclusive positives) at every group end, fp = min(position + 1, valid) - tp, stored COMPACTED by the group's rank:
//                 E[g] = (tp_g, fp_g).  A tie group may span any number of tiles; after the compaction the predecessor of group g is E[g-1].
//   k_om_area     per 2048 groups: sum of (tp_g - tp_{g-1}) / n_pos * tp_g / (tp_g + fp_g) in double and of the INTEGER
//                 (fp_g - fp_{g-1}) (tp_g + tp_{g-1}) in 64 bits (the whole sum is <= 2 n_pos n_neg < 2^63) -> one slot per workgroup.
//   k_om_final    one workgroup: the slots in a fixed order; aupr, auroc = S / (2 n_pos n_neg) (exact operands below 2^53, i.e. for any
//                 n below ~1.3e8 whatever the labels; one rounding each for operands beyond), n_pos, n_neg.
// Only (tp, fp) at group ends enter the areas, so the order inside a tie group is free and the payload is one bit.
// Bound: HBM (a pass of the sort moves 14 bytes per key; four passes + 8 bytes per group for the compaction).
#include "slot_sum.h"
#include "tile_sort.h"

namespace {

using namespace tile_sort;   // LB, ITEMS, TILE, WAVES, RADIX, pos, scanned, chunks: the sort's tile geometry is this pass's too

constexpr int HB = 512;                  // partial histogram rows (workgroups of k_om_keys)
constexpr int MAXK = 1024;               // classes: 3 k + 3 LDS counters
constexpr unsigned LAST_KEY = 0xFFFFFFFFu;
typedef unsigned long long u64;

__device__ __forceinline__ unsigned om_key(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;   // -0.0 == +0.0: one key
    return ~pdf_f32_ordered(__uint_as_float(u));
}

// part[col * HB + workgroup], col: [0, k) intersection | [k, 2k) output | [2k, 3k) target | 3k positives | 3k + 1 valid | 3k + 2 NaN score
__global__ __launch_bounds__(LB) void k_om_keys(long n, int c, int k, int ntiles, const float *__restrict__ logits, const long *__restrict__ pred,
                                                const float *__restrict__ score, const long *__restrict__ target, long ignore,
                                                const unsigned char *__restrict__ unknown, unsigned *__restrict__ keys,
                                                unsigned char *__restrict__ pay, unsigned *__restrict__ part) {
    __shared__ unsigned h[3 * MAXK + 3];
    const int ncol = 3 * k + 3;
    for (int col = threadIdx.x; col < ncol; col += LB) h[col] = 0u;
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int i = 0; i < ITEMS; ++i) {
            const long r = (long)tile * TILE + i * LB + threadIdx.x;
            if (r >= n) break;
            const long t = target[r];
            const bool valid = t != ignore, in_t = t >= 0 && t < k;
            if (valid) {
                long o;
                if (pred) {
                    o = pred[r];
                } else {   // torch.max(1)[1]: the first maximal value, a NaN being maximal
                    const float *x = logits + r * c;
                    float best = x[0];
                    int bi = 0;
                    for (int j = 1; j < c; ++j) {
                        const float v = x[j];
                        if (best == best && (v > best || v != v)) { best = v; bi = j; }
                    }
                    o = bi;
                }
                const bool in_o = o >= 0 && o < k;
                if (in_o) atomicAdd(&h[k + (int)o], 1u);
                if (in_t) atomicAdd(&h[2 * k + (int)t], 1u);
                if (in_o && o == t) atomicAdd(&h[(int)o], 1u);
                atomicAdd(&h[3 * k + 1], 1u);
            }
            if (score) {
                const float s = score[r];
                const bool pos = valid && in_t && unknown && unknown[t] != 0;
                if (pos) atomicAdd(&h[3 * k], 1u);
                if (valid && s != s) atomicOr(&h[3 * k + 2], 1u);
                keys[r] = valid ? om_key(s) : LAST_KEY;
                pay[r] = pos ? 1 : 0;
            }
        }
    }
    __syncthreads();
    for (int col = threadIdx.x; col < ncol; col += LB) part[(size_t)col * HB + blockIdx.x] = h[col];
}

// workgroup j < k: class j of the histogram; workgroup k: totals = [n_pos, n_valid, NaN seen], and the whole record when there is no score
__global__ __launch_bounds__(LB) void k_om_sums(int k, int nrows, const unsigned *__restrict__ part, long long *__restrict__ hist,
                                                u64 *__restrict__ totals, double *__restrict__ record, int has_score) {
    const int j = blockIdx.x;
    u64 a[3] = {0ull, 0ull, 0ull}, s[3];
    for (int q = 0; q < 3; ++q) {   // (the partial rows are column-major 32-bit counts: the lanes' sums are formed here, not by slot_total)
        const int col = j < k ? q * k + j : 3 * k + q;
        for (int b = threadIdx.x; b < nrows; b += LB) a[q] += part[(size_t)col * HB + b];
    }
    if (!block_sum_by_lanes<LB>(a, s)) return;
    if (j < k) {
        hist[j] = (long long)s[0];
        hist[k + j] = (long long)(s[1] + s[2] - s[0]);
        hist[2 * k + j] = (long long)s[2];
    } else {
        totals[0] = s[0]; totals[1] = s[1]; totals[2] = s[2]; totals[3] = 0ull;
        if (!has_score) {
            record[0] = record[1] = __builtin_nan("");
            record[2] = record[3] = 0.0;
        }
    }
}

// the last position of a group of equal keys (the array's last position is one)
__device__ __forceinline__ bool om_is_end(const unsigned *keys, size_t p, long n) { return p + 1 == (size_t)n || keys[p + 1] != keys[p]; }

// tcnt[tile] = positives among the tile's sorted positions, tcnt[ntiles + tile] = group ends among them
__global__ __launch_bounds__(LB) void k_om_ends(long n, int ntiles, const unsigned *__restrict__ keys, const unsigned char *__restrict__ pay,
                                                unsigned *__restrict__ tcnt) {
    const int tile = blockIdx.x;
    unsigned cnt[2] = {0u, 0u}, t[2];   // [positives, ends]
    for (int i = 0; i < ITEMS; ++i) {
        const size_t p = (size_t)tile * TILE + i * LB + threadIdx.x;
        const bool valid = p < (size_t)n;
        cnt[0] += (unsigned)__popcll(__ballot(valid && pay[p] != 0));   // (wave-uniform: already the wave's totals)
        cnt[1] += (unsigned)__popcll(__ballot(valid && om_is_end(keys, p, n)));
    }
    if (!block_sum_wave_totals<LB>(cnt, t)) return;
    tcnt[tile] = t[0];
    tcnt[(size_t)ntiles + tile] = t[1];
}

// E[rank of the group] = (tp, fp) at the group's end; totals[3] = number of groups.  tcnt / gtot: the scanned counts of k_om_ends (the
// ends follow the positives in ONE linear scan, so their prefix carries the total of the positives, n_pos).
__global__ __launch_bounds__(LB) void k_om_walk(long n, int ntiles, const unsigned *__restrict__ keys, const unsigned char *__restrict__ pay,
                                                const unsigned *__restrict__ tcnt, const unsigned *__restrict__ gtot, u64 *__restrict__ totals,
                                                uint2 *__restrict__ ends) {
    __shared__ unsigned wtot[2][WAVES];
    const int tile = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long posm[ITEMS], endm[ITEMS];
    unsigned mp = 0u, me = 0u;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const size_t p = pos(tile, w, r, lane);
        const bool valid = p < (size_t)n;
        posm[r] = __ballot(valid && pay[p] != 0);
        endm[r] = __ballot(valid && om_is_end(keys, p, n));
        mp += (unsigned)__popcll(posm[r]);
        me += (unsigned)__popcll(endm[r]);
    }
    if (lane == 0) { wtot[0][w] = mp; wtot[1][w] = me; }
    __syncthreads();
    const unsigned n_pos = (unsigned)totals[0], n_valid = (unsigned)totals[1];
    unsigned runp = scanned(tcnt, gtot, (size_t)tile), rune = scanned(tcnt, gtot, (size_t)ntiles + tile) - n_pos;
    for (int i = 0; i < w; ++i) { runp += wtot[0][i]; rune += wtot[1][i]; }
    const unsigned long long lower = (1ull << lane) - 1ull, upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        if ((endm[r] >> lane) & 1ull) {
            const size_t p = pos(tile, w, r, lane);
            const unsigned tp = runp + (unsigned)__popcll(posm[r] & upto), rank = rune + (unsigned)__popcll(endm[r] & lower);
            const unsigned seen = p + 1 < (size_t)n_valid ? (unsigned)(p + 1) : n_valid;   // the ignored rows sit behind the valid ones
            if ((size_t)rank < (size_t)n) ends[rank] = make_uint2(tp, seen - tp);           // (there are at most n groups)
            if (p + 1 == (size_t)n) totals[3] = (u64)rank + 1ull;
        }
        runp += (unsigned)__popcll(posm[r]);
        rune += (unsigned)__popcll(endm[r]);
    }
}

// per workgroup (2048 groups): pa[b] = its share of the average-precision sum, ps[b] = of the integer ROC sum
__global__ __launch_bounds__(LB) void k_om_area(long n, const uint2 *__restrict__ ends, const u64 *__restrict__ totals, double *__restrict__ pa,
                                                u64 *__restrict__ ps) {
    const u64 groups = totals[3] < (u64)n ? totals[3] : (u64)n;
    const double n_pos = (double)totals[0];
    double a[1] = {0.0};
    u64 s[1] = {0ull};
    for (int i = 0; i < ITEMS; ++i) {
        const u64 g = (u64)blockIdx.x * TILE + i * LB + threadIdx.x;
        if (g >= groups) break;
        const uint2 cur = ends[g], prev = g ? ends[g - 1] : make_uint2(0u, 0u);
        const unsigned dtp = cur.x - prev.x;
        if (dtp) a[0] += (double)dtp / n_pos * ((double)cur.x / ((double)cur.x + (double)cur.y));   // (a group of ignored rows adds nothing)
        s[0] += (u64)(cur.y - prev.y) * ((u64)cur.x + (u64)prev.x);
    }
    block_sum_by_waves<LB>(a, pa + blockIdx.x);   // (two element types: one call each)
    block_sum_by_waves<LB>(s, ps + blockIdx.x);
}

// record = [aupr, auroc, n_pos, n_neg].  One workgroup: the slot_total of either array.
__global__ __launch_bounds__(LB) void k_om_final(int ntiles, const double *__restrict__ pa, const u64 *__restrict__ ps,
                                                 const u64 *__restrict__ totals, double *__restrict__ record) {
    double xs[1];
    u64 ys[1];
    const bool t0 = slot_total<LB>(pa, ntiles, xs);   // (every thread makes both calls; both are true on thread 0 only)
    slot_total<LB>(ps, ntiles, ys);
    if (!t0) return;
    const double x = xs[0];
    const u64 y = ys[0];
    const u64 n_pos = totals[0], n_neg = totals[1] - totals[0];
    const bool bad = totals[2] != 0ull;
    const double nan = __builtin_nan("");
    record[0] = n_pos == 0ull || bad ? nan : x;
    record[1] = n_pos == 0ull || n_neg == 0ull || bad ? nan : (double)y / (2.0 * (double)n_pos * (double)n_neg);
    record[2] = (double)n_pos;
    record[3] = (double)n_neg;
}

struct OmWorkspace {
    unsigned *part, *keys[2], *hist, *gtot, *tcnt;
    unsigned char *pay[2];
    uint2 *ends;
    double *pa;
    u64 *ps, *totals;
    size_t bytes;
};

OmWorkspace om_carve(char *base, long n) {
    const size_t nt = (size_t)((n + TILE - 1) / TILE), nn = (size_t)n;
    OmWorkspace w;
    PdfCarver ws{base};
    w.totals = ws.take<u64>(4);
    w.pa = ws.take<double>(nt);
    w.ps = ws.take<u64>(nt);
    w.ends = ws.take<uint2>(nn);
    w.part = ws.take<unsigned>((size_t)(3 * MAXK + 3) * HB);
    for (int i = 0; i < 2; ++i) w.keys[i] = ws.take<unsigned>(nn);
    w.hist = ws.take<unsigned>(nt * RADIX);
    w.gtot = ws.take<unsigned>(chunks(nt * RADIX));   // (RADIX >= 2: covers the scan of the 2 * tiles end counts too)
    w.tcnt = ws.take<unsigned>(2 * nt);
    for (int i = 0; i < 2; ++i) w.pay[i] = ws.take<unsigned char>(nn);
    w.bytes = ws.off;
    return w;
}

bool om_shape_ok(long n) { return n >= 1 && n < 0x7FFFFFFFL; }

}  // namespace

extern "C" long pdf_openset_metrics_workspace_bytes(long n, int c) {
    if (!om_shape_ok(n) || c < 0) return 0;
    return (long)om_carve(nullptr, n).bytes;
}

extern "C" int pdf_openset_metrics(long n, int c, const float *logits, const long *pred, const float *score, const long *target, long ignore,
                                   const unsigned char *unknown, int k, long long *hist, double *record, void *workspace, void *stream) {
    if (!om_shape_ok(n) || k < 1 || (logits != nullptr) == (pred != nullptr) || (logits && c < 1) || !target || !hist || !record || !workspace)
        return PDF_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return PDF_ERR_BAD_ARG;
    if (k > MAXK) return PDF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const OmWorkspace w = om_carve(static_cast<char *>(workspace), n);
    const int nt = (int)((n + TILE - 1) / TILE);
    const int rows = nt < HB ? nt : HB;
    k_om_keys<<<(unsigned)rows, LB, 0, s>>>(n, c, k, nt, logits, pred, score, target, ignore, unknown, w.keys[0], w.pay[0], w.part);
    k_om_sums<<<(unsigned)(k + 1), LB, 0, s>>>(k, rows, w.part, hist, w.totals, record, score != nullptr);
    if (!score) return pdf_launch_status();
    const int cur = sort<unsigned char, true>(n, 1, w.keys, w.pay, w.hist, w.gtot, s);
    const long tlen = 2L * nt, tchunks = (long)chunks((size_t)tlen);
    k_om_ends<<<(unsigned)nt, LB, 0, s>>>(n, nt, w.keys[cur], w.pay[cur], w.tcnt);
    k_ts_scan_chunks<<<(unsigned)tchunks, LB, 0, s>>>(tlen, w.tcnt, w.gtot);
    k_ts_scan_short<<<1, LB, 0, s>>>((int)tchunks, w.gtot, nullptr);
    k_om_walk<<<(unsigned)nt, LB, 0, s>>>(n, nt, w.keys[cur], w.pay[cur], w.tcnt, w.gtot, w.totals, w.ends);
    k_om_area<<<(unsigned)nt, LB, 0, s>>>(n, w.ends, w.totals, w.pa, w.ps);
    k_om_final<<<1, LB, 0, s>>>(nt, w.pa, w.ps, w.totals, record);
    return pdf_launch_status();
}
