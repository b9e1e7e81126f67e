// The remaining criteria of pointcept/models/losses/misc.py as capturable passes: the full nn.CrossEntropyLoss (class weights, label
// smoothing, mean / sum / none, any class count), FocalLoss (:97-172), DiceLoss (:176-223) and BinaryFocalLoss (:60-93).  The plain
// cross-entropy of csrc/loss.hip is untouched.  Rules shared with loss.hip / lovasz.hip: fp32 logits, int64 labels, wave64; the slot
// sums of slot_sum.h in double (by waves into the workgroup's slot, one workgroup totals the slots); nothing needs zeroing; nothing is
// read back to the host (the reference selects rows with a boolean mask and branches on len(target) == 0).  Every forward leaves its
// UNSCALED gradient (dice: the softmax) in a buffer that the backward only reads, so retain_graph / a second backward see the same values.
//
//   acc = [sum, normaliser, scale, -] | per-workgroup [sum | normaliser] pairs of doubles            (CE, focal, binary focal)
//   acc = [loss, -, -, -] | coefficients (2, c): d loss / d p = ca[j] y + cb[j] p^(exponent - 1) | partial slabs (blocks, 3, c)   (dice)
//
// Row passes (CE, dice): c <= 64 one lane per row (as k_ce_fwd), above that one wave per row with strided columns and wave reductions.
// Bound: HBM for every kernel here (CE 8NC bytes forward, focal 8NC, dice 12NC).
#include "slot_sum.h"

namespace {

constexpr int LB = 256;
constexpr int HEAD = 4;
constexpr int MAX_BLOCKS = 1024;    // row / element passes: at most this many workgroups, one pair of doubles each
constexpr int DICE_BLOCKS = 512;    // dice column sums: at most this many row chunks, one (3, c) slab of floats each
enum { FIN_SUM = 0, FIN_MEAN = 1, FIN_MEAN_OR_ZERO = 2 };

__device__ __forceinline__ double *pair_slots(float *acc) { return reinterpret_cast<double *>(acc + HEAD); }

// the workgroup's [a | b] by waves into its own slot (every thread of the block calls it)
__device__ __forceinline__ void block_pair_store(double a, double b, float *acc) {
    double v[2] = {a, b};
    block_sum_by_waves<LB>(v, pair_slots(acc) + 2 * blockIdx.x);
}

// One workgroup: slot_total.  a = sum, b = normaliser.
//   FIN_SUM: loss = a, scale = 1;  FIN_MEAN: loss = a / (b per), scale = 1 / (b per) (NaN / inf when b == 0, as torch);
//   FIN_MEAN_OR_ZERO: the same, but loss = scale = 0 when b == 0 (every row ignored).
__global__ __launch_bounds__(LB) void k_finish(float *__restrict__ acc, int blocks, int mode, double per, float *__restrict__ loss) {
    double t[2];
    if (!slot_total<LB>(pair_slots(acc), blocks, t)) return;
    const double a = t[0], b = t[1];
    const bool zero = mode == FIN_MEAN_OR_ZERO && !(b > 0.0);
    const double denom = b * per;
    const double scale = mode == FIN_SUM ? 1.0 : zero ? 0.0 : 1.0 / denom;
    const double l = mode == FIN_SUM ? a : zero ? 0.0 : a / denom;
    acc[0] = (float)a; acc[1] = (float)b; acc[2] = (float)scale; acc[3] = 0.f;
    loss[0] = (float)l;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Extended cross-entropy.  WV = false: lane = row; WV = true: wave = row, lane j0 visits columns j0, j0 + 64, ...
template <bool WV>
__global__ __launch_bounds__(LB) void k_cex_fwd(long n, int c, const float *__restrict__ logits, const long *__restrict__ target,
                                                const float *__restrict__ weight, float eps, int reduction, long ignore,
                                                float *__restrict__ grad, float *__restrict__ acc, float *__restrict__ rowloss) {
    const int j0 = WV ? (int)(threadIdx.x & 63) : 0, js = WV ? 64 : 1;
    const long first = WV ? (long)blockIdx.x * (LB / 64) + (threadIdx.x >> 6) : (long)blockIdx.x * LB + threadIdx.x;
    const long stride = (long)gridDim.x * (WV ? LB / 64 : LB);
    const bool lead = !WV || j0 == 0;
    double loss = 0.0, wsum = 0.0;
    for (long r = first; r < n; r += stride) {   // (WV: the trip count, `counted` and every branch below are uniform over the wave)
        const float *x = logits + r * c;
        const long t = target[r];
        float m = -__builtin_huge_valf();
        for (int j = j0; j < c; j += js) m = fmaxf(m, x[j]);
        if (WV) m = pdf_wave_max_f32(m);
        float s = 0.f;
        for (int j = j0; j < c; j += js) s += expf(x[j] - m);
        if (WV) s = pdf_wave_sum_f32(s);
        const float lse = m + logf(s);
        const bool counted = t != ignore && t >= 0 && t < c;
        float l = 0.f, wt = 0.f, cp = 0.f, se = 0.f;
        if (counted) {
            wt = weight ? weight[t] : 1.f;
            float smooth = 0.f, wall = 0.f;
            if (eps > 0.f) {
                for (int j = j0; j < c; j += js) {
                    const float wj = weight ? weight[j] : 1.f;
                    smooth += wj * (lse - x[j]);
                    wall += wj;
                }
                if (WV) { smooth = pdf_wave_sum_f32(smooth); wall = pdf_wave_sum_f32(wall); }
                se = eps / (float)c;
            }
            l = (1.f - eps) * wt * (lse - x[t]) + se * smooth;
            cp = (1.f - eps) * wt + se * wall;
            if (lead) { loss += (double)l; wsum += (double)wt; }
        } else if (t != ignore) {
            // a label that is neither the ignore value nor a class id poisons the loss (as k_ce_fwd); its gradient row is 0
            l = __builtin_nanf("");
            if (lead) loss += (double)l;
        }
        if (rowloss && lead) rowloss[r] = l;
        float *g = grad + r * c;
        const float inv = 1.f / s, hot = (1.f - eps) * wt;
        for (int j = j0; j < c; j += js) {
            const float wj = se > 0.f ? se * (weight ? weight[j] : 1.f) : 0.f;
            g[j] = counted ? expf(x[j] - m) * inv * cp - (j == t ? hot : 0.f) - wj : 0.f;
        }
    }
    if (reduction != PDF_REDUCE_NONE) block_pair_store(loss, wsum, acc);
}

// out = d * gy[0] * acc[2]
__global__ __launch_bounds__(LB) void k_scale(long total, const float *__restrict__ d, const float *__restrict__ acc,
                                              const float *__restrict__ gy, float *__restrict__ out) {
    pdf_scaled_copy<LB>(total, d, gy[0] * acc[2], out);
}

// out[r, j] = d[r, j] * gy[r]
__global__ __launch_bounds__(LB) void k_scale_rows(long total, int c, const float *__restrict__ d, const float *__restrict__ gy,
                                                   float *__restrict__ out) {
    const bool narrow = total <= 0x7fffffffL;
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < total; e += (long)gridDim.x * LB) {
        const long r = c == 1 ? e : narrow ? (long)((unsigned)e / (unsigned)c) : e / c;
        out[e] = d[e] * gy[r];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Focal loss: one thread per ELEMENT (coalesced; the row's label comes from the cache).  With s = t ? -x : x the term is
// a sigmoid(s)^gamma softplus(s), a = t ? alpha : 1 - alpha: softplus(s) = max(s, 0) + log1p(exp(-|s|)) is torch's stable BCE_with_logits,
// sigmoid(s) = the reference's one_minus_pt.  d / ds = a sigmoid(s)^gamma (gamma (1 - sigmoid(s)) softplus(s) + sigmoid(s)).
__global__ __launch_bounds__(LB) void k_focal_fwd(long total, int c, const float *__restrict__ logits, const long *__restrict__ target,
                                                  const float *__restrict__ alpha_vec, float alpha, float gamma, long ignore,
                                                  float *__restrict__ grad, float *__restrict__ acc) {
    const bool narrow = total <= 0x7fffffffL;
    double loss = 0.0, cnt = 0.0;
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < total; e += (long)gridDim.x * LB) {
        const long r = narrow ? (long)((unsigned)e / (unsigned)c) : e / c;
        const int j = (int)(e - r * c);
        const long t = target[r];
        float g = 0.f;
        if (t != ignore) {
            if (j == 0) cnt += 1.0;   // valid rows, counted once each
            if (t < 0 || t >= c) {
                if (j == 0) loss += (double)__builtin_nanf("");
            } else {
                const float x = logits[e];
                const bool y = j == t;
                const float a = alpha_vec ? alpha_vec[j] : alpha, aw = y ? a : 1.f - a;
                const float s = y ? -x : x;
                const float ex = expf(-fabsf(s)), q = 1.f / (1.f + ex);
                const float sp = fmaxf(s, 0.f) + log1pf(ex);
                const float sig = s >= 0.f ? q : ex * q, one_m = s >= 0.f ? ex * q : q;
                const float pw = gamma == 2.f ? sig * sig : powf(sig, gamma);
                loss += (double)(aw * pw * sp);
                const float ds = aw * pw * (gamma * one_m * sp + sig);
                g = y ? -ds : ds;
            }
        }
        grad[e] = g;
    }
    block_pair_store(loss, cnt, acc);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Binary focal loss, elementwise.  om = 1 - exp(-bce) is formed as -expm1(-bce).
__global__ __launch_bounds__(LB) void k_bfocal_fwd(long n, const float *__restrict__ pred, const float *__restrict__ target, float alpha,
                                                   float gamma, int logits, int reduce, float *__restrict__ grad, float *__restrict__ acc,
                                                   float *__restrict__ out) {
    double loss = 0.0, cnt = 0.0;
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < n; e += (long)gridDim.x * LB) {
        const float x = pred[e], t = target[e];
        float bce, dbce;
        if (logits) {
            const float ex = expf(-fabsf(x)), q = 1.f / (1.f + ex);
            bce = fmaxf(x, 0.f) - x * t + log1pf(ex);
            dbce = (x >= 0.f ? q : ex * q) - t;
        } else {   // F.binary_cross_entropy: both logs clamped at -100, the gradient's denominator at 1e-12
            bce = (t - 1.f) * fmaxf(log1pf(-x), -100.f) - t * fmaxf(logf(x), -100.f);
            dbce = (x - t) / fmaxf((1.f - x) * x, 1e-12f);
        }
        const float pt = expf(-bce), om = -expm1f(-bce);
        const float aw = alpha * t + (1.f - alpha) * (1.f - t);
        const float pw = gamma == 2.f ? om * om : powf(om, gamma), pw1 = gamma == 2.f ? om : powf(om, gamma - 1.f);
        const float f = aw * pw * bce;
        grad[e] = aw * (gamma * pw1 * pt * bce + pw) * dbce;
        if (reduce) { loss += (double)f; cnt += 1.0; } else out[e] = f;
    }
    if (reduce) block_pair_store(loss, cnt, acc);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Dice loss.  k_dice_prob: softmax of every row -> prob.  k_dice_colsum: workgroup (b, y) owns a chunk of rows and the columns
// [256 y, 256 y + cw); thread = (row group, column), consecutive threads read consecutive floats; its sums over the chunk of
// [p y | p^exponent | y] go to slab (b, 3, c).  k_dice_finish: one workgroup adds the slabs per class in chunk order (double), forms the
// class terms and the coefficients of the backward.  k_dice_bwd: row pass, softmax backward of g_j = ca[j] y_j + cb[j] p_j^(exponent-1).
template <bool WV>
__global__ __launch_bounds__(LB) void k_dice_prob(long n, int c, const float *__restrict__ logits, float *__restrict__ prob) {
    const int j0 = WV ? (int)(threadIdx.x & 63) : 0, js = WV ? 64 : 1;
    const long first = WV ? (long)blockIdx.x * (LB / 64) + (threadIdx.x >> 6) : (long)blockIdx.x * LB + threadIdx.x;
    const long stride = (long)gridDim.x * (WV ? LB / 64 : LB);
    for (long r = first; r < n; r += stride) {
        const float *x = logits + r * c;
        float m = -__builtin_huge_valf();
        for (int j = j0; j < c; j += js) m = fmaxf(m, x[j]);
        if (WV) m = pdf_wave_max_f32(m);
        float s = 0.f;
        for (int j = j0; j < c; j += js) s += expf(x[j] - m);
        if (WV) s = pdf_wave_sum_f32(s);
        float *p = prob + r * c;
        for (int j = j0; j < c; j += js) p[j] = expf(x[j] - m) / s;
    }
}

__device__ __forceinline__ long dice_label(long t, int c) { return t < 0 ? 0 : t > c - 1 ? c - 1 : t; }   // the reference clamps

__global__ __launch_bounds__(LB) void k_dice_colsum(long n, int c, const float *__restrict__ prob, const long *__restrict__ target,
                                                    long ignore, float exponent, long rows_per_block, float *__restrict__ slab) {
    __shared__ float red[3][LB];
    const int jb = blockIdx.y * LB, cw = c - jb < LB ? c - jb : LB, groups = LB / cw;
    const int g = threadIdx.x / cw, j = threadIdx.x - g * cw;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    float a = 0.f, b = 0.f, y = 0.f;
    if (g < groups) {
        for (long r = r0 + g; r < r1; r += groups) {
            const long t = target[r];
            if (t == ignore) continue;
            const float p = prob[r * c + jb + j];
            const bool hot = dice_label(t, c) == jb + j;
            a += hot ? p : 0.f;
            b += exponent == 2.f ? p * p : powf(p, exponent);
            y += hot ? 1.f : 0.f;
        }
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = y;
    __syncthreads();
    if ((int)threadIdx.x < cw) {
        for (int q = 0; q < 3; ++q) {
            double s = 0.0;
            for (int k = 0; k < groups; ++k) s += (double)red[q][k * cw + threadIdx.x];
            slab[((size_t)blockIdx.x * 3 + q) * c + jb + threadIdx.x] = (float)s;
        }
    }
}

__global__ __launch_bounds__(LB) void k_dice_finish(int c, int blocks, const float *__restrict__ slab, float smooth, float exponent,
                                                    long ignore, float *__restrict__ acc, float *__restrict__ loss) {
    float *ca = acc + HEAD, *cb = ca + c;
    double terms = 0.0;
    for (int j = threadIdx.x; j < c; j += LB) {
        double a = 0.0, b = 0.0, y = 0.0;
        for (int k = 0; k < blocks; ++k) {
            const float *s = slab + (size_t)k * 3 * c;
            a += (double)s[j]; b += (double)s[c + j]; y += (double)s[2 * c + j];
        }
        const double num = 2.0 * a + (double)smooth, den = b + y + (double)smooth;
        const bool skip = (long)j == ignore;   // the reference leaves class `ignore_index` out of the sum; the divisor stays c
        terms += skip ? 0.0 : 1.0 - num / den;
        ca[j] = skip ? 0.f : (float)(-2.0 / (den * c));
        cb[j] = skip ? 0.f : (float)((double)exponent * num / (den * den * c));
    }
    const double mine[1] = {terms};
    double total[1];
    if (!block_sum_by_lanes<LB>(mine, total)) return;   // (the lanes' class terms in lane order)
    const float l = (float)(total[0] / c);
    acc[0] = l; acc[1] = 0.f; acc[2] = 1.f; acc[3] = 0.f;
    loss[0] = l;
}

template <bool WV>
__global__ __launch_bounds__(LB) void k_dice_bwd(long n, int c, const float *__restrict__ prob, const long *__restrict__ target, long ignore,
                                                 float exponent, const float *__restrict__ acc, const float *__restrict__ gy,
                                                 float *__restrict__ out) {
    const int j0 = WV ? (int)(threadIdx.x & 63) : 0, js = WV ? 64 : 1;
    const long first = WV ? (long)blockIdx.x * (LB / 64) + (threadIdx.x >> 6) : (long)blockIdx.x * LB + threadIdx.x;
    const long stride = (long)gridDim.x * (WV ? LB / 64 : LB);
    const float *ca = acc + HEAD, *cb = ca + c;
    const float g0 = gy[0];
    for (long r = first; r < n; r += stride) {   // (WV: uniform over the wave)
        const long t = target[r];
        const float *p = prob + r * c;
        float *o = out + r * c;
        if (t == ignore) {
            for (int j = j0; j < c; j += js) o[j] = 0.f;
            continue;
        }
        const long tc = dice_label(t, c);
        float dot = 0.f;
        for (int j = j0; j < c; j += js) {
            const float pj = p[j];
            const float gj = (j == tc ? ca[j] : 0.f) + cb[j] * (exponent == 2.f ? pj : powf(pj, exponent - 1.f));
            dot += gj * pj;
        }
        if (WV) dot = pdf_wave_sum_f32(dot);
        for (int j = j0; j < c; j += js) {
            const float pj = p[j];
            const float gj = (j == tc ? ca[j] : 0.f) + cb[j] * (exponent == 2.f ? pj : powf(pj, exponent - 1.f));
            o[j] = pj * (gj - dot) * g0;
        }
    }
}

inline unsigned row_blocks(long n, int c) {
    const long per = c <= 64 ? LB : LB / 64;
    const long g = (n + per - 1) / per;
    return (unsigned)(g > MAX_BLOCKS ? MAX_BLOCKS : g);
}
inline unsigned elem_blocks(long total, long cap) {
    const long g = (total + LB - 1) / LB;
    return (unsigned)(g > cap ? cap : g);
}
inline bool bad_reduction(int r) { return r != PDF_REDUCE_NONE && r != PDF_REDUCE_MEAN && r != PDF_REDUCE_SUM; }

}  // namespace

// floats of `acc` for any of the passes with c classes: the pairs of doubles of the row / element passes, or dice's coefficients + slabs
extern "C" long pdf_criteria_workspace_floats(int c) {
    if (c < 1) return 0;
    const long pairs = HEAD + 4L * MAX_BLOCKS, dice = HEAD + 2L * c + 3L * c * DICE_BLOCKS;
    return pairs > dice ? pairs : dice;
}

extern "C" int pdf_ce_ex_forward(long n, int c, const float *logits, const long *target, const float *weight, float label_smoothing,
                                 int reduction, long ignore, float *grad, float *acc, float *loss, void *stream) {
    if (n < 1 || c < 1 || !logits || !target || !grad || !acc || !loss || bad_reduction(reduction)
        || !(label_smoothing >= 0.f && label_smoothing <= 1.f))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = row_blocks(n, c);
    float *rowloss = reduction == PDF_REDUCE_NONE ? loss : nullptr;
    if (c <= 64) k_cex_fwd<false><<<g, LB, 0, s>>>(n, c, logits, target, weight, label_smoothing, reduction, ignore, grad, acc, rowloss);
    else k_cex_fwd<true><<<g, LB, 0, s>>>(n, c, logits, target, weight, label_smoothing, reduction, ignore, grad, acc, rowloss);
    if (reduction != PDF_REDUCE_NONE)
        k_finish<<<1, LB, 0, s>>>(acc, (int)g, reduction == PDF_REDUCE_MEAN ? FIN_MEAN : FIN_SUM, 1.0, loss);
    return pdf_launch_status();
}

extern "C" int pdf_ce_ex_backward(long n, int c, const float *dlogits, const float *acc, const float *gy, int reduction, float *grad_out,
                                  void *stream) {
    if (n < 1 || c < 1 || !dlogits || !acc || !gy || !grad_out || bad_reduction(reduction)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = elem_blocks(n * c, PDF_MAX_BLOCKS);
    if (reduction == PDF_REDUCE_NONE) k_scale_rows<<<g, LB, 0, s>>>(n * c, c, dlogits, gy, grad_out);
    else k_scale<<<g, LB, 0, s>>>(n * c, dlogits, acc, gy, grad_out);
    return pdf_launch_status();
}

extern "C" int pdf_focal_forward(long n, int c, const float *logits, const long *target, const float *alpha_vec, float alpha, float gamma,
                                 int reduction, long ignore, float *grad, float *acc, float *loss, void *stream) {
    if (n < 1 || c < 1 || !logits || !target || !grad || !acc || !loss || (reduction != PDF_REDUCE_MEAN && reduction != PDF_REDUCE_SUM))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = elem_blocks(n * c, MAX_BLOCKS);
    k_focal_fwd<<<g, LB, 0, s>>>(n * c, c, logits, target, alpha_vec, alpha, gamma, ignore, grad, acc);
    k_finish<<<1, LB, 0, s>>>(acc, (int)g, reduction == PDF_REDUCE_MEAN ? FIN_MEAN_OR_ZERO : FIN_SUM, (double)c, loss);
    return pdf_launch_status();
}

extern "C" int pdf_focal_backward(long n, int c, const float *dlogits, const float *acc, const float *gy, float *grad_out, void *stream) {
    if (n < 1 || c < 1 || !dlogits || !acc || !gy || !grad_out) return PDF_ERR_BAD_ARG;
    k_scale<<<elem_blocks(n * c, PDF_MAX_BLOCKS), LB, 0, static_cast<hipStream_t>(stream)>>>(n * c, dlogits, acc, gy, grad_out);
    return pdf_launch_status();
}

extern "C" int pdf_bfocal_forward(long n, const float *pred, const float *target, float alpha, float gamma, int logits, int reduce,
                                  float *grad, float *acc, float *loss, void *stream) {
    if (n < 1 || !pred || !target || !grad || !acc || !loss) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = elem_blocks(n, MAX_BLOCKS);
    k_bfocal_fwd<<<g, LB, 0, s>>>(n, pred, target, alpha, gamma, logits, reduce, grad, acc, loss);
    if (reduce) k_finish<<<1, LB, 0, s>>>(acc, (int)g, FIN_MEAN, 1.0, loss);
    return pdf_launch_status();
}

extern "C" int pdf_bfocal_backward(long n, const float *dpred, const float *acc, const float *gy, int reduce, float *grad_out, void *stream) {
    if (n < 1 || !dpred || !acc || !gy || !grad_out) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = elem_blocks(n, PDF_MAX_BLOCKS);
    if (reduce) k_scale<<<g, LB, 0, s>>>(n, dpred, acc, gy, grad_out);
    else k_scale_rows<<<g, LB, 0, s>>>(n, 1, dpred, gy, grad_out);
    return pdf_launch_status();
}

extern "C" int pdf_dice_forward(long n, int c, const float *logits, const long *target, float smooth, float exponent, long ignore,
                                float *prob, float *acc, float *loss, void *stream) {
    if (n < 1 || c < 1 || !logits || !target || !prob || !acc || !loss || !(exponent > 0.f)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = row_blocks(n, c);
    if (c <= 64) k_dice_prob<false><<<g, LB, 0, s>>>(n, c, logits, prob);
    else k_dice_prob<true><<<g, LB, 0, s>>>(n, c, logits, prob);
    long chunks = (n + 127) / 128;
    if (chunks > DICE_BLOCKS) chunks = DICE_BLOCKS;
    const long rows_per_block = (n + chunks - 1) / chunks;
    const int blocks = (int)((n + rows_per_block - 1) / rows_per_block);   // (no chunk is empty: every slab is written)
    float *slab = acc + HEAD + 2L * c;
    k_dice_colsum<<<dim3((unsigned)blocks, (unsigned)((c + LB - 1) / LB)), LB, 0, s>>>(n, c, prob, target, ignore, exponent, rows_per_block, slab);
    k_dice_finish<<<1, LB, 0, s>>>(c, blocks, slab, smooth, exponent, ignore, acc, loss);
    return pdf_launch_status();
}

extern "C" int pdf_dice_backward(long n, int c, const float *prob, const long *target, long ignore, float exponent, const float *acc,
                                 const float *gy, float *grad_out, void *stream) {
    if (n < 1 || c < 1 || !prob || !target || !acc || !gy || !grad_out || !(exponent > 0.f)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = row_blocks(n, c);
    if (c <= 64) k_dice_bwd<false><<<g, LB, 0, s>>>(n, c, prob, target, ignore, exponent, acc, gy, grad_out);
    else k_dice_bwd<true><<<g, LB, 0, s>>>(n, c, prob, target, ignore, exponent, acc, gy, grad_out);
    return pdf_launch_status();
}
