// Patch attention of Point Transformer V3 over the serialized order (point_transformer_v3m1_base.py:172-216) without the K x K score
// tensor: flash-style passes in fp32 on v_mfma_f32_16x16x4_f32 (head width 16 = one 16 x 16 tile per side).
//
// Rows stay where the qkv Linear left them: (n, 3 c) in original order; a serialized position p reads row order[p].  The patch layout
// (the reference's pad / unpad) lives in two small tables built with the geometry:
//   qtab {q_start, q_len <= 64, k_start, k_len}                         a chunk of a patch's OWNED queries and the patch's key window
//   ktab {k_start, k_len <= 64, qa_start, qa_len, qb_start, qb_len, shared_from}
//                                                                      a chunk of keys, the owned queries of its own patch (a) and -- for
//                                                                      the keys at positions >= shared_from -- of the scene's last patch (b)
//
// Operand layout (lane l: li = l & 15, lg = l >> 4; A[row li][k lg], B[k lg][col li], C[row 4 lg + reg][col li]):
//   S^T = K Q^T   A = K[key 16 t + li][d 4 lg + e], B = Q[q li][d 4 lg + e], e = 0..3  ->  lane holds S[q li][key 16 t + 4 lg + r]
//   O^T = V^T P^T A = V[key 16 t + 4 lg + r][d li], B = that accumulator register r      ->  lane holds O[q li][d 4 lg + reg]
// so the probabilities go from one product into the next without leaving their registers, and a row's statistics are a reduction over
// the lane's 16 registers and two lane exchanges (xor 16, 32).  The backward passes use the same two shapes with the roles of queries and
// keys exchanged.  One workgroup = 4 waves = 64 stationary rows; the streamed side passes through LDS in tiles of 64 rows of 16 floats
// (row stride 20 floats: 16-byte aligned rows, the column reads of the second product hit 64 distinct banks).
//
//   k_fwd     query-stationary, online softmax (running maximum, partial sums per lane, one division at the end); writes out and the
//             row's log-sum-exp as the pair (m, l) = (maximum, sum of exp(s - m)): the rounded sum m + log l would cost every
//             probability of the row half an ulp of |lse| (2 ulps at lse = 5).
//   k_bwd_q   query-stationary: p = exp(s - m) / l, dP = dO V^T, dS = p (dP - delta), dQ = scale dS K; writes delta = <dO, O> and g_q.
//   k_bwd_kv  key-stationary over window a, then window b: dV = P^T dO, dK = dS^T (scale Q); writes g_k and g_v.
// No float atomics, a fixed order of every sum, every output element written once.
#include "pdfops_common.h"

namespace sa {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;      // threads per workgroup
constexpr int ROWS = 64;     // stationary rows per workgroup = streamed rows per LDS tile
constexpr int STR = 20;      // LDS row stride in floats
constexpr float LOG2E = 1.4426950408889634f;
constexpr float BIG = 1e30f;

#define SA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

__device__ __forceinline__ bool window_ok(int start, int len, long n) { return start >= 0 && len >= 0 && (long)start + (long)len <= n; }

// row of serialized position p, or -1
__device__ __forceinline__ long row_at(const long long *order, long p, long n) {
    const long long r = order[p];
    return (r >= 0 && r < (long long)n) ? (long)r : -1L;
}

// One LDS tile: rows [base, base + 64) of a window of `len` positions starting at `start`; columns col0 .. col0 + 15 of every row's
// (ld-strided) record into a (and col1 .. into b).  Rows outside the window are zero.  Thread t: row t >> 2, quarter t & 3.
__device__ __forceinline__ void load_tile(const float *__restrict__ src_a, const float *__restrict__ src_b, size_t ld_a, size_t ld_b, int col_a,
                                          int col_b, float mul_a, const long long *__restrict__ order, long n, int start, int len, int base,
                                          float *sa_, float *sb_) {
    const int r = threadIdx.x >> 2, qd = threadIdx.x & 3;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (base + r < len) {
        const long row = row_at(order, (long)start + base + r, n);
        if (row >= 0) {
            a = ld4(src_a + (size_t)row * ld_a + col_a + 4 * qd) * mul_a;
            b = ld4(src_b + (size_t)row * ld_b + col_b + 4 * qd);
        }
    }
    *reinterpret_cast<f32x4 *>(sa_ + r * STR + 4 * qd) = a;
    *reinterpret_cast<f32x4 *>(sb_ + r * STR + 4 * qd) = b;
}

__global__ __launch_bounds__(NT) void k_fwd(long n, int c, float scale, const float *__restrict__ qkv, const long long *__restrict__ order,
                                            const int4 *__restrict__ qtab, int h, float *__restrict__ out, float *__restrict__ lse) {
    __shared__ __attribute__((aligned(16))) float sK[ROWS * STR];
    __shared__ __attribute__((aligned(16))) float sV[ROWS * STR];
    const int4 it = qtab[blockIdx.x];
    const int head = blockIdx.y, q0 = it.x, ql = it.y, k0 = it.z, kl = it.w;
    if (ql < 1 || ql > ROWS || kl < 1 || !window_ok(q0, ql, n) || !window_ok(k0, kl, n)) return;   // (block-uniform)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const size_t ld = 3 * (size_t)c;
    const int qi = 16 * w + li;
    const bool active = 16 * w < ql;   // (wave-uniform)
    long qrow = qi < ql ? row_at(order, (long)q0 + qi, n) : -1L;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (qrow >= 0) q = ld4(qkv + (size_t)qrow * ld + head * 16 + 4 * lg) * scale;
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    float m = -BIG, l = 0.f;
    for (int kt = 0; kt < kl; kt += ROWS) {
        __syncthreads();
        load_tile(qkv, qkv, ld, ld, c + head * 16, 2 * c + head * 16, 1.f, order, n, k0, kl, kt, sK, sV);
        __syncthreads();
        if (!active) continue;
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 ka[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ka[t] = ld4(sK + (16 * t + li) * STR + 4 * lg);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = SA_MFMA(ka[t][e], q[e], s[t]);
        float mx = -BIG;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kt + 16 * t + 4 * lg + r >= kl) s[t][r] = -BIG;
                mx = fmaxf(mx, s[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = ex2((m - mn) * LOG2E);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (kt + 16 * t + 4 * lg + r < kl) ? ex2((s[t][r] - mn) * LOG2E) : 0.f;
                s[t][r] = p;
                ps += p;
            }
        l = l * alpha + ps;
        o0 *= alpha;
        o1 *= alpha;
#pragma unroll
        for (int t = 0; t < 4; t += 2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o0 = SA_MFMA(sV[(16 * t + 4 * lg + r) * STR + li], s[t][r], o0);
                o1 = SA_MFMA(sV[(16 * (t + 1) + 4 * lg + r) * STR + li], s[t + 1][r], o1);
            }
    }
    if (!active) return;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qrow >= 0) {
        const f32x4 o = (o0 + o1) / l;
        *reinterpret_cast<f32x4 *>(out + (size_t)qrow * c + head * 16 + 4 * lg) = o;
        if (lg == 0) *reinterpret_cast<float2 *>(lse + 2 * ((size_t)qrow * h + head)) = make_float2(m, l);
    }
}

__global__ __launch_bounds__(NT) void k_bwd_q(long n, int c, float scale, const float *__restrict__ qkv, const float *__restrict__ out,
                                              const float *__restrict__ lse, const float *__restrict__ gout,
                                              const long long *__restrict__ order, const int4 *__restrict__ qtab, int h,
                                              float *__restrict__ delta, float *__restrict__ gqkv) {
    __shared__ __attribute__((aligned(16))) float sK[ROWS * STR];
    __shared__ __attribute__((aligned(16))) float sV[ROWS * STR];
    const int4 it = qtab[blockIdx.x];
    const int head = blockIdx.y, q0 = it.x, ql = it.y, k0 = it.z, kl = it.w;
    if (ql < 1 || ql > ROWS || kl < 1 || !window_ok(q0, ql, n) || !window_ok(k0, kl, n)) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const size_t ld = 3 * (size_t)c;
    const int qi = 16 * w + li;
    const bool active = 16 * w < ql;
    long qrow = qi < ql ? row_at(order, (long)q0 + qi, n) : -1L;
    f32x4 q = {0.f, 0.f, 0.f, 0.f}, go = {0.f, 0.f, 0.f, 0.f};
    float L = BIG, il = 0.f, dl = 0.f;
    if (qrow >= 0) {
        q = ld4(qkv + (size_t)qrow * ld + head * 16 + 4 * lg) * scale;
        go = ld4(gout + (size_t)qrow * c + head * 16 + 4 * lg);
        const f32x4 oo = ld4(out + (size_t)qrow * c + head * 16 + 4 * lg);
        const float2 ml = *reinterpret_cast<const float2 *>(lse + 2 * ((size_t)qrow * h + head));
        L = ml.x;
        il = 1.f / ml.y;
        dl = go[0] * oo[0] + go[1] * oo[1] + go[2] * oo[2] + go[3] * oo[3];
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (qrow >= 0 && lg == 0) delta[(size_t)qrow * h + head] = dl;
    f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < kl; kt += ROWS) {
        __syncthreads();
        load_tile(qkv, qkv, ld, ld, c + head * 16, 2 * c + head * 16, 1.f, order, n, k0, kl, kt, sK, sV);
        __syncthreads();
        if (!active) continue;
        f32x4 s[4], dp[4], ka[4], va[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            ka[t] = ld4(sK + (16 * t + li) * STR + 4 * lg);
            va[t] = ld4(sV + (16 * t + li) * STR + 4 * lg);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = SA_MFMA(ka[t][e], q[e], s[t]);
                dp[t] = SA_MFMA(va[t][e], go[e], dp[t]);
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (kt + 16 * t + 4 * lg + r < kl) ? ex2((s[t][r] - L) * LOG2E) * il : 0.f;
                s[t][r] = p * (dp[t][r] - dl);
            }
#pragma unroll
        for (int t = 0; t < 4; t += 2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                g0 = SA_MFMA(sK[(16 * t + 4 * lg + r) * STR + li], s[t][r], g0);
                g1 = SA_MFMA(sK[(16 * (t + 1) + 4 * lg + r) * STR + li], s[t + 1][r], g1);
            }
    }
    if (active && qrow >= 0) *reinterpret_cast<f32x4 *>(gqkv + (size_t)qrow * ld + head * 16 + 4 * lg) = (g0 + g1) * scale;
}

struct KItem { int k0, kl, qa0, qal, qb0, qbl, shared_from, pad; };

__global__ __launch_bounds__(NT) void k_bwd_kv(long n, int c, float scale, const float *__restrict__ qkv, const float *__restrict__ lse,
                                               const float *__restrict__ delta, const float *__restrict__ gout,
                                               const long long *__restrict__ order, const KItem *__restrict__ ktab, int h,
                                               float *__restrict__ gqkv) {
    __shared__ __attribute__((aligned(16))) float sQ[ROWS * STR];
    __shared__ __attribute__((aligned(16))) float sG[ROWS * STR];
    __shared__ __attribute__((aligned(16))) float sL[ROWS];
    __shared__ __attribute__((aligned(16))) float sD[ROWS];
    __shared__ __attribute__((aligned(16))) float sI[ROWS];
    const KItem it = ktab[blockIdx.x];
    const int head = blockIdx.y;
    if (it.kl < 1 || it.kl > ROWS || !window_ok(it.k0, it.kl, n) || !window_ok(it.qa0, it.qal, n) || !window_ok(it.qb0, it.qbl, n)) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    const size_t ld = 3 * (size_t)c;
    const int ki = 16 * w + li;
    const bool active = 16 * w < it.kl;
    const long kpos = (long)it.k0 + ki;
    long krow = ki < it.kl ? row_at(order, kpos, n) : -1L;
    f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if (krow >= 0) {
        kk = ld4(qkv + (size_t)krow * ld + c + head * 16 + 4 * lg);
        vv = ld4(qkv + (size_t)krow * ld + 2 * c + head * 16 + 4 * lg);
    }
    f32x4 gk0 = {0.f, 0.f, 0.f, 0.f}, gk1 = {0.f, 0.f, 0.f, 0.f}, gv0 = {0.f, 0.f, 0.f, 0.f}, gv1 = {0.f, 0.f, 0.f, 0.f};
    for (int win = 0; win < 2; ++win) {
        const int qs = win ? it.qb0 : it.qa0, qlen = win ? it.qbl : it.qal;
        const bool live = krow >= 0 && (win == 0 || kpos >= (long)it.shared_from);   // this lane's key takes part in the window
        for (int qt = 0; qt < qlen; qt += ROWS) {
            __syncthreads();
            load_tile(qkv, gout, ld, (size_t)c, head * 16, head * 16, scale, order, n, qs, qlen, qt, sQ, sG);
            if (threadIdx.x < ROWS) {
                float L = BIG, il = 0.f, d = 0.f;
                if (qt + (int)threadIdx.x < qlen) {
                    const long row = row_at(order, (long)qs + qt + threadIdx.x, n);
                    if (row >= 0) {
                        const float2 ml = *reinterpret_cast<const float2 *>(lse + 2 * ((size_t)row * h + head));
                        L = ml.x;
                        il = 1.f / ml.y;
                        d = delta[(size_t)row * h + head];
                    }
                }
                sL[threadIdx.x] = L;
                sD[threadIdx.x] = d;
                sI[threadIdx.x] = il;
            }
            __syncthreads();
            if (!active) continue;
            f32x4 s[4], dp[4], qa[4], ga[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                qa[t] = ld4(sQ + (16 * t + li) * STR + 4 * lg);
                ga[t] = ld4(sG + (16 * t + li) * STR + 4 * lg);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s[t] = SA_MFMA(qa[t][e], kk[e], s[t]);      // S[q 16 t + 4 lg + r][key li]
                    dp[t] = SA_MFMA(ga[t][e], vv[e], dp[t]);    // dP, same places
                }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 Lq = ld4(sL + 16 * t + 4 * lg), Dq = ld4(sD + 16 * t + 4 * lg), Iq = ld4(sI + 16 * t + 4 * lg);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = live ? ex2((s[t][r] - Lq[r]) * LOG2E) * Iq[r] : 0.f;
                    s[t][r] = p;
                    dp[t][r] = p * (dp[t][r] - Dq[r]);
                }
            }
#pragma unroll
            for (int t = 0; t < 4; t += 2)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gv0 = SA_MFMA(sG[(16 * t + 4 * lg + r) * STR + li], s[t][r], gv0);
                    gk0 = SA_MFMA(sQ[(16 * t + 4 * lg + r) * STR + li], dp[t][r], gk0);
                    gv1 = SA_MFMA(sG[(16 * (t + 1) + 4 * lg + r) * STR + li], s[t + 1][r], gv1);
                    gk1 = SA_MFMA(sQ[(16 * (t + 1) + 4 * lg + r) * STR + li], dp[t + 1][r], gk1);
                }
        }
    }
    if (active && krow >= 0) {
        *reinterpret_cast<f32x4 *>(gqkv + (size_t)krow * ld + c + head * 16 + 4 * lg) = gk0 + gk1;
        *reinterpret_cast<f32x4 *>(gqkv + (size_t)krow * ld + 2 * c + head * 16 + 4 * lg) = gv0 + gv1;
    }
}

}  // namespace
}  // namespace sa

extern "C" int pdf_serial_attn_supported(int c, int h, int k) { return (h >= 1 && c == 16 * h && c <= 512 && k >= 1) ? 1 : 0; }

extern "C" int pdf_serial_attn_forward(long n, int c, int h, float scale, const float *qkv, const long long *order, const int *qtab, int nq,
                                       float *out, float *lse, void *stream) {
    if (n == 0 || nq == 0) return PDF_OK;
    if (n < 0 || n >= (1L << 31) - 2 || nq < 0 || !qkv || !order || !qtab || !out || !lse) return PDF_ERR_BAD_ARG;
    if (!pdf_serial_attn_supported(c, h, 1)) return PDF_ERR_UNSUPPORTED;
    sa::k_fwd<<<dim3((unsigned)nq, (unsigned)h), sa::NT, 0, static_cast<hipStream_t>(stream)>>>(
        n, c, scale, qkv, order, reinterpret_cast<const int4 *>(qtab), h, out, lse);
    return pdf_launch_status();
}

extern "C" int pdf_serial_attn_backward(long n, int c, int h, float scale, const float *qkv, const float *out, const float *lse,
                                        const float *g_out, const long long *order, const int *qtab, int nq, const int *ktab, int nk,
                                        float *delta, float *g_qkv, void *stream) {
    if (n == 0 || nq == 0) return PDF_OK;
    if (n < 0 || n >= (1L << 31) - 2 || nq < 0 || nk < 1 || !qkv || !out || !lse || !g_out || !order || !qtab || !ktab || !delta || !g_qkv)
        return PDF_ERR_BAD_ARG;
    if (!pdf_serial_attn_supported(c, h, 1)) return PDF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    sa::k_bwd_q<<<dim3((unsigned)nq, (unsigned)h), sa::NT, 0, s>>>(n, c, scale, qkv, out, lse, g_out, order,
                                                                    reinterpret_cast<const int4 *>(qtab), h, delta, g_qkv);
    sa::k_bwd_kv<<<dim3((unsigned)nk, (unsigned)h), sa::NT, 0, s>>>(n, c, scale, qkv, lse, delta, g_out, order,
                                                                     reinterpret_cast<const sa::KItem *>(ktab), h, g_qkv);
    return pdf_launch_status();
}
