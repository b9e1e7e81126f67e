// Grouped vector attention core of PointTransformer-V2 (point_transformer_v2m2_base.py:109-129) as two nodes with hand-written backwards.
//
//   relation   rel[n,s,:] = (key[idx[n,s]] - query[n]) * pem[n,s] + peb[n,s]        (pem / peb optional; idx < 0 reads a zero key row);
//              the grouped (n, s, c) key is never materialised
//   attend     p = softmax over s of logits[n,:,g];  w = p * [idx >= 0]  (mask AFTER the softmax, no renormalisation);
//              out[n, g*i + j] = sum_s w[n,s,g] * (value[idx[n,s], g*i + j] + peb[n,s,g*i + j]),  i = c / groups = 8
//
// One thread per (point, channel), channel fastest; the eight channels of a group are eight neighbouring lanes (c % 8 == 0), so the
// per-group inner products of the backward are three lane exchanges.  Scatter-adds (g_key, g_value) are segmented sums over the inverse
// kNN table (csrc/seg_gather.hip's table form: ascending entry ids per destination) -- no float atomics, every sum in a fixed order.
// Sums over s and over a destination's entries are carried in double and rounded once.  The element-wise expressions are rounded as
// written (-ffp-contract=off), so the relation's forward is the torch composition's bit for bit.
#include "pdfops_common.h"

namespace gva {
namespace {

constexpr int TB = 256;
constexpr int GI = 8;        // channels per group of the fused attend class
constexpr int MAX_S = 64;

inline unsigned capped(long total) { const long b = (total + TB - 1) / TB; return (unsigned)(b < 8 * PDF_MAX_BLOCKS ? b : 8 * PDF_MAX_BLOCKS); }

__device__ __forceinline__ float key_at(const float *key, long nk, int j, int c, int ch) { return (j >= 0 && (long)j < nk) ? key[(size_t)j * c + ch] : 0.f; }

__global__ __launch_bounds__(TB) void k_rel_fwd(long total, long nk, int s, int c, const float *__restrict__ query, const float *__restrict__ key,
                                                const int *__restrict__ idx, const float *__restrict__ pem, const float *__restrict__ peb,
                                                float *__restrict__ rel) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < total; t += (long)gridDim.x * TB) {
        const long e = t / c;
        const int ch = (int)(t - e * c);
        const long nn = e / s;
        float r = key_at(key, nk, idx[e], c, ch) - query[nn * c + ch];
        if (pem) r = r * pem[t];
        if (peb) r = r + peb[t];
        rel[t] = r;
    }
}

// g_query[n] = - sum_s g_rel * pem;  g_pem = g_rel * (key[idx] - query)
__global__ __launch_bounds__(TB) void k_rel_bwd(long total, long nk, int s, int c, const float *__restrict__ g_rel, const float *__restrict__ query,
                                                const float *__restrict__ key, const int *__restrict__ idx, const float *__restrict__ pem,
                                                float *__restrict__ g_query, float *__restrict__ g_pem) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < total; t += (long)gridDim.x * TB) {
        const long nn = t / c;
        const int ch = (int)(t - nn * c);
        const float q = query[t];
        double acc = 0.0;
        for (int j = 0; j < s; ++j) {
            const long e = nn * s + j;
            const size_t at = (size_t)e * c + ch;
            const float g = g_rel[at];
            acc += pem ? (double)(g * pem[at]) : (double)g;
            if (g_pem) g_pem[at] = g * (key_at(key, nk, idx[e], c, ch) - q);
        }
        if (g_query) g_query[t] = -(float)acc;
    }
}

// out[v, ch] = sum over v's inverse segment of a[e, ch] * (b ? b[e, ch] : 1)
__global__ __launch_bounds__(TB) void k_seg_prod(long total, long entries, int c, const float *__restrict__ a, const float *__restrict__ b,
                                                 const int *__restrict__ inv_off, const int *__restrict__ inv_entry, float *__restrict__ out) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < total; t += (long)gridDim.x * TB) {
        const long v = t / c;
        const int ch = (int)(t - v * c);
        double acc = 0.0;
        const int end = inv_off[v + 1];
        for (int k = inv_off[v]; k < end; ++k) {
            const long e = inv_entry[k];
            if (e < 0 || e >= entries) continue;
            const size_t at = (size_t)e * c + ch;
            acc += b ? (double)(a[at] * b[at]) : (double)a[at];
        }
        out[t] = (float)acc;
    }
}

// out[v, ch] = sum over v's inverse segment of w[e, ch / GI] * src[e / s, ch]
__global__ __launch_bounds__(TB) void k_seg_weighted(long total, long entries, int s, int c, int groups, const float *__restrict__ w,
                                                     const float *__restrict__ src, const int *__restrict__ inv_off,
                                                     const int *__restrict__ inv_entry, float *__restrict__ out) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < total; t += (long)gridDim.x * TB) {
        const long v = t / c;
        const int ch = (int)(t - v * c), g = ch / GI;
        double acc = 0.0;
        const int end = inv_off[v + 1];
        for (int k = inv_off[v]; k < end; ++k) {
            const long e = inv_entry[k];
            if (e < 0 || e >= entries) continue;
            acc += (double)(w[(size_t)e * groups + g] * src[(size_t)(e / s) * c + ch]);
        }
        out[t] = (float)acc;
    }
}

// softmax statistics of logits[n, :, g]: the maximum and the sum of exp(l - max) (terms in fp32, sum in double, rounded once)
__device__ __forceinline__ void softmax_stats(const float *lg, int s, int groups, float &mx, float &den) {
    mx = lg[0];
    for (int j = 1; j < s; ++j) mx = fmaxf(mx, lg[(size_t)j * groups]);
    double d = 0.0;
    for (int j = 0; j < s; ++j) d += (double)expf(lg[(size_t)j * groups] - mx);
    den = (float)d;
}

__global__ __launch_bounds__(TB) void k_att_fwd(long total, long nv, int s, int c, int groups, const float *__restrict__ logits,
                                                const float *__restrict__ value, const float *__restrict__ peb, const int *__restrict__ idx,
                                                float *__restrict__ out, float *__restrict__ p) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < total; t += (long)gridDim.x * TB) {
        const long nn = t / c;
        const int ch = (int)(t - nn * c), g = ch / GI;
        const float *lg = logits + (size_t)nn * s * groups + g;
        float mx, den;
        softmax_stats(lg, s, groups, mx, den);
        double acc = 0.0;
        for (int j = 0; j < s; ++j) {
            const long e = nn * s + j;
            const float pj = expf(lg[(size_t)j * groups] - mx) / den;
            if ((ch & (GI - 1)) == 0) p[(size_t)e * groups + g] = pj;
            const int r = idx[e];
            if (r >= 0 && (long)r < nv) {
                float x = value[(size_t)r * c + ch];
                if (peb) x = x + peb[(size_t)e * c + ch];
                acc += (double)(pj * x);
            }
        }
        out[t] = (float)acc;
    }
}

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = 1; o < GI; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// g_logits[n,s,g] = p * (m * d - sum_t p_t m_t d_t),  d[s,g] = <g_out[n, group], value[idx] + peb>;  g_peb[n,s,ch] = p * m * g_out[n,ch].
// The index range is padded to a multiple of 64: every lane of a wave runs the exchanges; lanes past the end work on the last element
// with a zero gradient and store nothing (total is a multiple of 8, so a group is live or padded as a whole).
__global__ __launch_bounds__(TB) void k_att_bwd(long total, long nv, int s, int c, int groups, const float *__restrict__ g_out,
                                                const float *__restrict__ p, const float *__restrict__ value, const float *__restrict__ peb,
                                                const int *__restrict__ idx, float *__restrict__ g_logits, float *__restrict__ g_peb) {
    const long padded = (total + 63) / 64 * 64;
    for (long t0 = (long)blockIdx.x * TB + threadIdx.x; t0 < padded; t0 += (long)gridDim.x * TB) {
        const bool live = t0 < total;
        const long t = live ? t0 : total - 1;
        const long nn = t / c;
        const int ch = (int)(t - nn * c), g = ch / GI;
        const float go = live ? g_out[t] : 0.f;
        double S = 0.0;
        for (int j = 0; j < s; ++j) {
            const long e = nn * s + j;
            const int r = idx[e];
            const bool m = r >= 0 && (long)r < nv;
            float x = m ? value[(size_t)r * c + ch] : 0.f;
            if (peb) x = x + peb[(size_t)e * c + ch];
            const double d = group_sum((double)go * (double)x);
            if (m) S += (double)p[(size_t)e * groups + g] * d;
        }
        for (int j = 0; j < s; ++j) {
            const long e = nn * s + j;
            const int r = idx[e];
            const bool m = r >= 0 && (long)r < nv;
            float x = m ? value[(size_t)r * c + ch] : 0.f;
            if (peb) x = x + peb[(size_t)e * c + ch];
            const double d = group_sum((double)go * (double)x);
            const float pj = p[(size_t)e * groups + g];
            if (live) {
                if ((ch & (GI - 1)) == 0) g_logits[(size_t)e * groups + g] = (float)((double)pj * ((m ? d : 0.0) - S));
                if (g_peb) g_peb[(size_t)e * c + ch] = m ? pj * go : 0.f;
            }
        }
    }
}

}  // namespace
}  // namespace gva

// the fused attend class: c = 8 * groups, 1 <= s <= 64 (the relation node takes any c and s)
extern "C" int pdf_gva_supported(int c, int groups, int s) {
    return c >= 1 && groups >= 1 && c % groups == 0 && c / groups == gva::GI && s >= 1 && s <= gva::MAX_S;
}

// query (n, c), key (nk, c), idx (n, s) with values in [-1, nk), pem / peb (n, s, c) or NULL -> rel (n, s, c)
extern "C" int pdf_gva_relation_forward(long n, long nk, int s, int c, const float *query, const float *key, const int *idx, const float *pem,
                                        const float *peb, float *rel, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || nk < 1 || s < 1 || c < 1 || !query || !key || !idx || !rel) return PDF_ERR_BAD_ARG;
    gva::k_rel_fwd<<<gva::capped(n * s * c), gva::TB, 0, static_cast<hipStream_t>(stream)>>>(n * s * c, nk, s, c, query, key, idx, pem, peb, rel);
    return pdf_launch_status();
}

// inv_off (nk + 1) / inv_entry: the inverse of idx (pdf_seg_sum_rows' table form, entry_base 0).  g_query (n, c), g_key (nk, c),
// g_pem (n, s, c): each nullable (not asked for); g_peb is g_rel itself.
extern "C" int pdf_gva_relation_backward(long n, long nk, int s, int c, const float *g_rel, const float *query, const float *key, const int *idx,
                                         const float *pem, const int *inv_off, const int *inv_entry, float *g_query, float *g_key, float *g_pem,
                                         void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || nk < 1 || s < 1 || c < 1 || !g_rel || !query || !key || !idx || (g_key && (!inv_off || !inv_entry)) || (g_pem && !pem))
        return PDF_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (g_query || g_pem) gva::k_rel_bwd<<<gva::capped(n * c), gva::TB, 0, st>>>(n * c, nk, s, c, g_rel, query, key, idx, pem, g_query, g_pem);
    if (g_key) gva::k_seg_prod<<<gva::capped(nk * c), gva::TB, 0, st>>>(nk * c, n * s, c, g_rel, pem, inv_off, inv_entry, g_key);
    return pdf_launch_status();
}

// logits (n, s, groups), value (nv, c), peb (n, s, c) or NULL, idx (n, s) -> out (n, c), p (n, s, groups) = the softmax (saved for the backward)
extern "C" int pdf_gva_attend_forward(long n, long nv, int s, int c, int groups, const float *logits, const float *value, const float *peb,
                                      const int *idx, float *out, float *p, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || nv < 1 || !logits || !value || !idx || !out || !p) return PDF_ERR_BAD_ARG;
    if (!pdf_gva_supported(c, groups, s)) return PDF_ERR_UNSUPPORTED;
    gva::k_att_fwd<<<gva::capped(n * c), gva::TB, 0, static_cast<hipStream_t>(stream)>>>(n * c, nv, s, c, groups, logits, value, peb, idx, out, p);
    return pdf_launch_status();
}

// -> g_logits (n, s, groups), g_value (nv, c) (nullable), g_peb (n, s, c) (nullable; needs peb)
extern "C" int pdf_gva_attend_backward(long n, long nv, int s, int c, int groups, const float *g_out, const float *p, const float *value,
                                       const float *peb, const int *idx, const int *inv_off, const int *inv_entry, float *g_logits,
                                       float *g_value, float *g_peb, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || nv < 1 || !g_out || !p || !value || !idx || !g_logits || (g_value && (!inv_off || !inv_entry)) || (g_peb && !peb))
        return PDF_ERR_BAD_ARG;
    if (!pdf_gva_supported(c, groups, s)) return PDF_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    gva::k_att_bwd<<<gva::capped(n * c), gva::TB, 0, st>>>(n * c, nv, s, c, groups, g_out, p, value, peb, idx, g_logits, g_peb);
    if (g_value) gva::k_seg_weighted<<<gva::capped(nv * c), gva::TB, 0, st>>>(nv * c, n * s, s, c, groups, p, g_out, inv_off, inv_entry, g_value);
    return pdf_launch_status();
}
