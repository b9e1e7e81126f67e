// The head of the context-aware classifier (pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py) as
// capturable passes.  Rules shared with criteria.hip: fp32 data, int64 labels, int32 scene ends (`offset`) on the device, wave64; no float
// atomics -- every workgroup leaves its partial sums in its own slab and the slabs are added in a fixed order, so every pass is
// bit-reproducible; nothing needs zeroing; nothing is read back to the host; a grid is sized from n, K, c and the scene count alone.
//
// Rows are cut into chunks per scene: workgroup (ch, s) owns rows [a_s + ch len_s, a_s + (ch + 1) len_s) of scene s = [a_s, b_s), with
// len_s = ceil((b_s - a_s) / chunks) rounded up to the row step; chunks = cac_chunks(n, scenes).  A chunk never straddles a scene; a
// chunk without rows still writes its (zero) slab.
//
// Three shapes (K classes, c channels, CP = c + 4 padded columns, KP = K rounded up to 4):
//   class sums  k_class_sums<MODE>: slab[s][ch](K, CP) = sum_n w_nk [R_n | 1 0 0 0] over the chunk's rows; the weights are formed in the
//               pass -- SOFT: softmax(logits) * threshold mask (P is never materialised), ONEHOT: the label, GIVEN: a gradient matrix with
//               R_n the normalised row (the cosine's prototype gradient).  Steps of 32 rows are staged in LDS; a thread owns up to three
//               4 x 4 tiles of the (K, CP) result in registers.  k_class_finish (one wave per class row) adds the slabs in chunk order
//               (double) and applies the normaliser of the mode.
//   row passes  steps of 16 rows against the scene's (K, c) slab in LDS (38 KB at K = 200, c = 48): k_soft_bwd (gradient of the soft
//               prototypes into the features and, through the softmax and the normaliser, into the logits), k_cos_fwd, k_cos_bwd_x.
//   distillation loss: k_distill_row (one wave per row) leaves the unscaled gradient and [l e | e] per row, k_distill_class the per-class
//               triples per workgroup, k_distill_finish (one workgroup) the loss and the class coefficients the backward multiplies with.
// Bounds: none of these is HBM-bound at the recipe's size (4 N (K + c) algorithmic bytes next to 2 N K c fp32 flops); the products are
// LDS-fed FMA tiles (two 16-byte LDS reads per 16 FMAs).
#include "pdfops_common.h"

namespace {

constexpr int LB = 256;
constexpr int RS = 32;            // rows per step of the class sums
constexpr int RR = 16;            // rows per step of the row passes
constexpr int MAXT = 3;           // 4 x 4 register tiles per thread in the class sums
constexpr int MAX_CHUNKS = 128;
constexpr int CHUNK_ROWS = 512;   // a scene is cut into more chunks once the batch has more than this many rows per (scene, chunk)
constexpr int DIST_BLOCKS = 64;   // workgroups of the distillation loss's class pass
enum { W_SOFT = 0, W_ONEHOT = 1, W_GIVEN = 2 };
enum { FIN_SOFT = 0, FIN_LABEL = 1, FIN_COSGRAD = 2 };
constexpr float NORM_EPS = 1e-12f;   // F.normalize
constexpr long SOFT_BWD_LDS = 96 * 1024;

inline int kp_of(int K) { return (K + 3) & ~3; }
inline bool supported(int K, int c) {
    if (K < 1 || c < 4 || c > 64 || (c & 3) || K > 256) return false;
    if ((long)(kp_of(K) / 4) * (c / 4 + 1) > (long)LB * MAXT) return false;
    // LDS: the cosine backward (slab (KP, CP) + a row tile (RR, KP) + two (RR, CP)) stays inside the 64 KB every kernel may ask for; the
    // soft-prototype backward with the logits gradient holds a second (RR, KP) tile and asks for a raised limit (SOFT_BWD_LDS)
    const long KP = kp_of(K), CP = c + 4;
    return 4L * (KP * CP + RR * KP + 2L * RR * CP + 2 * RR) <= 64 * 1024 && 4L * (KP * CP + KP + 2L * RR * KP + RR * CP) <= SOFT_BWD_LDS;
}
inline int cac_chunks(long n, int scenes) {
    long g = (n + (long)scenes * CHUNK_ROWS - 1) / ((long)scenes * CHUNK_ROWS);
    return (int)(g < 1 ? 1 : g > MAX_CHUNKS ? MAX_CHUNKS : g);
}

// rows [r0, r1) of chunk ch of scene s (offset == nullptr: one scene of n rows); step = the pass's row step
__device__ __forceinline__ void chunk_rows(long n, const int *__restrict__ offset, int s, int ch, int nch, int step, long &r0, long &r1) {
    long a = 0, b = n;
    if (offset) {
        a = s ? (long)offset[s - 1] : 0;
        b = (long)offset[s];
        b = b < 0 ? 0 : b > n ? n : b;
        a = a < 0 ? 0 : a > b ? b : a;
    }
    long len = (b - a + nch - 1) / nch;
    len = (len + step - 1) / step * step;
    r0 = a + (long)ch * len;
    if (r0 > b) r0 = b;
    r1 = r0 + len < b ? r0 + len : b;
}

// softmax(x) * [max prob >= thresh] of one row by one wave -> w[0, KP) (zeros past K, or when the row does not exist)
__device__ __forceinline__ void soft_weights(const float *__restrict__ x, bool live, int K, int KP, float thresh, float *__restrict__ w) {
    const int lane = threadIdx.x & 63;
    if (!live) {
        for (int k = lane; k < KP; k += 64) w[k] = 0.f;
        return;
    }
    float m = -__builtin_huge_valf();
    for (int k = lane; k < K; k += 64) m = fmaxf(m, x[k]);
    m = pdf_wave_max_f32(m);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(x[k] - m);
    s = pdf_wave_sum_f32(s);
    const bool keep = !(thresh > 0.f) || 1.f / s >= thresh;   // the largest probability is exp(0) / s
    for (int k = lane; k < KP; k += 64) w[k] = k < K && keep ? expf(x[k] - m) / s : 0.f;
}

// acc[a][b] += sum_j X[r0 + a][j] S[k0 + b][j], j in [0, c): rows of X and S are 16-byte aligned
__device__ __forceinline__ void mac_xs(const float *__restrict__ X, int ldx, const float *__restrict__ S, int lds, int c, int r0, int k0,
                                       float (&acc)[4][4]) {
    for (int j = 0; j < c; j += 4) {
        float4 xa[4], sb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xa[a] = *reinterpret_cast<const float4 *>(X + (r0 + a) * ldx + j);
#pragma unroll
        for (int b = 0; b < 4; ++b) sb[b] = *reinterpret_cast<const float4 *>(S + (k0 + b) * lds + j);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] += xa[a].x * sb[b].x + xa[a].y * sb[b].y + xa[a].z * sb[b].z + xa[a].w * sb[b].w;
    }
}

// acc[a][0..3] += sum_k W[r0 + a][k] S[k][j0 .. j0 + 3], k in [0, K)
__device__ __forceinline__ void mac_ws(const float *__restrict__ W, int ldw, const float *__restrict__ S, int lds, int K, int r0, int j0,
                                       float (&acc)[4][4]) {
    for (int k = 0; k < K; ++k) {
        const float4 sv = *reinterpret_cast<const float4 *>(S + k * lds + j0);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float w = W[(r0 + a) * ldw + k];
            acc[a][0] += w * sv.x; acc[a][1] += w * sv.y; acc[a][2] += w * sv.z; acc[a][3] += w * sv.w;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Class sums.  grid (chunks, scenes); dynamic LDS: Wt (RS, KP) | Xt (RS, CP) | rinv (RS).
template <int MODE>
__global__ __launch_bounds__(LB) void k_class_sums(long n, int K, int c, const int *__restrict__ offset, const float *__restrict__ rows,
                                                   const float *__restrict__ wsrc, const long *__restrict__ target, float thresh,
                                                   float *__restrict__ slab) {
    extern __shared__ __align__(16) float lds[];
    const int KP = (K + 3) & ~3, CP = c + 4, JT = CP / 4, ntiles = (KP / 4) * JT;
    float *Wt = lds, *Xt = Wt + RS * KP, *rinv = Xt + RS * CP;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long r0, r1;
    chunk_rows(n, offset, blockIdx.y, blockIdx.x, gridDim.x, RS, r0, r1);
    float acc[MAXT][4][4];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[t][a][b] = 0.f;
    for (long r = r0; r < r1; r += RS) {   // (block-uniform trip count)
        const int live = r1 - r < RS ? (int)(r1 - r) : RS;
        for (int e = tid; e < RS * CP; e += LB) {
            const int rr = e / CP, j = e - rr * CP;
            Xt[e] = rr < live ? (j < c ? rows[(r + rr) * c + j] : j == c ? 1.f : 0.f) : 0.f;
        }
        if (MODE == W_SOFT) {
            for (int rr = wave; rr < RS; rr += LB / 64) soft_weights(wsrc + (r + rr) * K, rr < live, K, KP, thresh, Wt + rr * KP);
        } else if (MODE == W_ONEHOT) {
            for (int e = tid; e < RS * KP; e += LB) {
                const int rr = e / KP, k = e - rr * KP;
                Wt[e] = rr < live && target[r + rr] == (long)k && k < K ? 1.f : 0.f;
            }
        } else {
            __syncthreads();
            if (tid < RS) {   // 1 / max(|x|, eps) of the staged rows
                float q = 0.f;
                for (int j = 0; j < c; ++j) q += Xt[tid * CP + j] * Xt[tid * CP + j];
                rinv[tid] = 1.f / fmaxf(sqrtf(q), NORM_EPS);
            }
            __syncthreads();
            for (int e = tid; e < RS * KP; e += LB) {
                const int rr = e / KP, k = e - rr * KP;
                Wt[e] = rr < live && k < K ? wsrc[(r + rr) * K + k] * rinv[rr] : 0.f;
            }
        }
        __syncthreads();
        for (int rr = 0; rr < RS; ++rr) {
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                const int tile = tid + t * LB;
                if (tile < ntiles) {
                    const int kt = tile / JT, jt = tile - kt * JT;
                    const float4 w = *reinterpret_cast<const float4 *>(Wt + rr * KP + 4 * kt);
                    const float4 x = *reinterpret_cast<const float4 *>(Xt + rr * CP + 4 * jt);
                    const float wv[4] = {w.x, w.y, w.z, w.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[t][a][b] += wv[a] * xv[b];
                }
            }
        }
        __syncthreads();
    }
    float *out = slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)K * CP;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int tile = tid + t * LB;
        if (tile < ntiles) {
            const int kt = tile / JT, jt = tile - kt * JT;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (4 * kt + a < K)
                    *reinterpret_cast<float4 *>(out + (size_t)(4 * kt + a) * CP + 4 * jt) = make_float4(acc[t][a][0], acc[t][a][1], acc[t][a][2], acc[t][a][3]);
        }
    }
}

// One wave per class row (s, k): lane j < c adds column j of the chunk slabs in chunk order, every lane the mass column.
//   FIN_SOFT:    out[s, k, j] = sum / (mass + 1e-7), aux[s, k] = mass
//   FIN_LABEL:   out[k, j] = mass > 0 ? sum / (mass + 1e-4) : base[k, j], aux[k] = mass (the count)
//   FIN_COSGRAD: w = scale sum; with p = base[s, k, :]: out = (w - [|p| >= eps] p^ (p^ . w)) / max(|p|, eps)   (F.normalize's backward)
__global__ __launch_bounds__(LB) void k_class_finish(int K, int c, int scenes, int nch, int mode, const float *__restrict__ slab,
                                                     const float *__restrict__ base, float scale, float *__restrict__ out,
                                                     float *__restrict__ aux) {
    const int CP = c + 4, lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (LB / 64) + (threadIdx.x >> 6);   // (wave-uniform)
    if (row >= (long)scenes * K) return;
    const int s = (int)(row / K), k = (int)(row - (long)s * K);
    const bool col = lane < c;
    double sum = 0.0, mass = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
        const float *p = slab + (((size_t)s * nch + ch) * K + k) * CP;
        sum += col ? (double)p[lane] : 0.0;
        mass += (double)p[c];
    }
    float *o = out + (size_t)row * c;
    if (mode == FIN_SOFT) {
        if (col) o[lane] = (float)(sum / (mass + 1e-7));
        if (lane == 0) aux[row] = (float)mass;
    } else if (mode == FIN_LABEL) {
        if (col) o[lane] = mass > 0.0 ? (float)(sum / (mass + 1e-4)) : base[(size_t)row * c + lane];
        if (lane == 0) aux[row] = (float)mass;
    } else {
        const float p = col ? base[(size_t)row * c + lane] : 0.f, w = scale * (float)sum;
        const float norm = sqrtf(pdf_wave_sum_f32(p * p)), den = fmaxf(norm, NORM_EPS), ph = p / den;
        const float dot = pdf_wave_sum_f32(col ? ph * w : 0.f);
        if (col) o[lane] = (w - (norm >= NORM_EPS ? ph * dot : 0.f)) / den;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Backward of the soft prototypes.  With Q_k = G_k / (A_k + 1e-7), d_k = proto_k . Q_k, w_nk = m_n P_nk:
//   gfeat_n = sum_k w_nk Q_k;   glogits_nk = w_nk (u_nk - sum_j w_nj u_nj), u_nk = F_n . Q_k - d_k   (the mask is not differentiated).
// dynamic LDS: Qs (KP, CP) | dk (KP) | Wt (RR, KP) | Xt (RR, CP) | Tt (RR, KP), the last with LOGITS only
template <bool LOGITS>
__global__ __launch_bounds__(LB) void k_soft_bwd(long n, int K, int c, const int *__restrict__ offset, const float *__restrict__ feat,
                                                 const float *__restrict__ logits, float thresh, const float *__restrict__ proto,
                                                 const float *__restrict__ mass, const float *__restrict__ gproto,
                                                 float *__restrict__ gfeat, float *__restrict__ glogits) {
    extern __shared__ __align__(16) float lds[];
    const int KP = (K + 3) & ~3, CP = c + 4;
    float *Qs = lds, *dk = Qs + KP * CP, *Wt = dk + KP, *Xt = Wt + RR * KP, *Tt = Xt + RR * CP;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = blockIdx.y;
    long r0, r1;
    chunk_rows(n, offset, s, blockIdx.x, gridDim.x, RR, r0, r1);
    if (r0 >= r1) return;   // (block-uniform)
    for (int e = tid; e < KP * CP; e += LB) {
        const int k = e / CP, j = e - k * CP;
        Qs[e] = k < K && j < c ? gproto[((size_t)s * K + k) * c + j] / (mass[(size_t)s * K + k] + 1e-7f) : 0.f;
    }
    __syncthreads();
    for (int k = tid; k < KP; k += LB) {
        float d = 0.f;
        if (k < K)
            for (int j = 0; j < c; ++j) d += proto[((size_t)s * K + k) * c + j] * Qs[k * CP + j];
        dk[k] = d;
    }
    for (long r = r0; r < r1; r += RR) {
        const int live = r1 - r < RR ? (int)(r1 - r) : RR;
        __syncthreads();   // (dk on the first trip; the previous step's tiles afterwards)
        for (int e = tid; e < RR * CP; e += LB) {
            const int rr = e / CP, j = e - rr * CP;
            Xt[e] = rr < live && j < c ? feat[(r + rr) * c + j] : 0.f;
        }
        for (int rr = wave; rr < RR; rr += LB / 64) soft_weights(logits + (r + rr) * K, rr < live, K, KP, thresh, Wt + rr * KP);
        __syncthreads();
        if (LOGITS && tid < (RR / 4) * (KP / 4)) {   // Tt = X Q^T
            const int rt = tid / (KP / 4), kt = tid - rt * (KP / 4);
            float acc[4][4] = {};
            mac_xs(Xt, CP, Qs, CP, c, 4 * rt, 4 * kt, acc);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float4 *>(Tt + (4 * rt + a) * KP + 4 * kt) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        }
        if (tid < (RR / 4) * (c / 4)) {   // gfeat = W Q
            const int rt = tid / (c / 4), jt = tid - rt * (c / 4);
            float acc[4][4] = {};
            mac_ws(Wt, KP, Qs, CP, K, 4 * rt, 4 * jt, acc);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (4 * rt + a < live)
                    *reinterpret_cast<float4 *>(gfeat + (r + 4 * rt + a) * c + 4 * jt) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        }
        if (LOGITS) {
            __syncthreads();
            for (int rr = wave; rr < live; rr += LB / 64) {   // (wave-uniform)
                float dot = 0.f;
                for (int k = lane; k < K; k += 64) dot += Wt[rr * KP + k] * (Tt[rr * KP + k] - dk[k]);
                dot = pdf_wave_sum_f32(dot);
                for (int k = lane; k < K; k += 64) glogits[(r + rr) * K + k] = Wt[rr * KP + k] * (Tt[rr * KP + k] - dk[k] - dot);
            }
        }
    }
}

// gfeat[n] = G[t_n] / (count[t_n] + 1e-4) for labels in [0, K), else 0
__global__ __launch_bounds__(LB) void k_label_bwd(long total, int K, int c, const long *__restrict__ target, const float *__restrict__ count,
                                                  const float *__restrict__ gproto, float *__restrict__ gfeat) {
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < total; e += (long)gridDim.x * LB) {
        const long r = e / c;
        const int j = (int)(e - r * c);
        const long t = target[r];
        gfeat[e] = t >= 0 && t < K ? gproto[t * c + j] / (count[t] + 1e-4f) : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Cosine logits.  The scene's prototypes are normalised into LDS once per workgroup: one wave per row, lane = channel.
__device__ __forceinline__ void stage_unit_rows(const float *__restrict__ src, int nrows, int live, int c, int CP, float *__restrict__ dst,
                                                float *__restrict__ rinv, float *__restrict__ norms) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = wave; k < nrows; k += LB / 64) {   // (wave-uniform)
        const float v = k < live && lane < c ? src[(size_t)k * c + lane] : 0.f;
        const float norm = sqrtf(pdf_wave_sum_f32(v * v)), inv = 1.f / fmaxf(norm, NORM_EPS);
        if (lane < CP) dst[k * CP + lane] = v / fmaxf(norm, NORM_EPS);
        if (rinv && lane == 0) { rinv[k] = inv; norms[k] = norm; }
    }
}

// out[n, k] = scale x^_n . p^_k;   dynamic LDS: Ps (KP, CP) | Xt (RR, CP)
__global__ __launch_bounds__(LB) void k_cos_fwd(long n, int K, int c, const int *__restrict__ offset, const float *__restrict__ x,
                                                const float *__restrict__ proto, float scale, float *__restrict__ out) {
    extern __shared__ __align__(16) float lds[];
    const int KP = (K + 3) & ~3, CP = c + 4;
    float *Ps = lds, *Xt = Ps + KP * CP;
    const int tid = threadIdx.x, s = blockIdx.y;
    long r0, r1;
    chunk_rows(n, offset, s, blockIdx.x, gridDim.x, RR, r0, r1);
    if (r0 >= r1) return;
    stage_unit_rows(proto + (size_t)s * K * c, KP, K, c, CP, Ps, nullptr, nullptr);
    for (long r = r0; r < r1; r += RR) {
        const int live = r1 - r < RR ? (int)(r1 - r) : RR;
        __syncthreads();
        stage_unit_rows(x + r * c, RR, live, c, CP, Xt, nullptr, nullptr);
        __syncthreads();
        if (tid < (RR / 4) * (KP / 4)) {
            const int rt = tid / (KP / 4), kt = tid - rt * (KP / 4);
            float acc[4][4] = {};
            mac_xs(Xt, CP, Ps, CP, c, 4 * rt, 4 * kt, acc);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (4 * rt + a < live && 4 * kt + b < K) out[(r + 4 * rt + a) * K + 4 * kt + b] = scale * acc[a][b];
        }
    }
}

// gx_n = scale (v - [|x| >= eps] x^ (x^ . v)) / max(|x|, eps), v = sum_k g_nk p^_k;   dynamic LDS: Ps | Gt (RR, KP) | Xt | Vt (RR, CP) | rinv | norm
__global__ __launch_bounds__(LB) void k_cos_bwd_x(long n, int K, int c, const int *__restrict__ offset, const float *__restrict__ x,
                                                  const float *__restrict__ proto, float scale, const float *__restrict__ gout,
                                                  float *__restrict__ gx) {
    extern __shared__ __align__(16) float lds[];
    const int KP = (K + 3) & ~3, CP = c + 4;
    float *Ps = lds, *Gt = Ps + KP * CP, *Xt = Gt + RR * KP, *Vt = Xt + RR * CP, *rinv = Vt + RR * CP, *norms = rinv + RR;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = blockIdx.y;
    long r0, r1;
    chunk_rows(n, offset, s, blockIdx.x, gridDim.x, RR, r0, r1);
    if (r0 >= r1) return;
    stage_unit_rows(proto + (size_t)s * K * c, KP, K, c, CP, Ps, nullptr, nullptr);
    for (long r = r0; r < r1; r += RR) {
        const int live = r1 - r < RR ? (int)(r1 - r) : RR;
        __syncthreads();
        stage_unit_rows(x + r * c, RR, live, c, CP, Xt, rinv, norms);
        for (int e = tid; e < RR * KP; e += LB) {
            const int rr = e / KP, k = e - rr * KP;
            Gt[e] = rr < live && k < K ? gout[(r + rr) * K + k] : 0.f;
        }
        __syncthreads();
        if (tid < (RR / 4) * (c / 4)) {
            const int rt = tid / (c / 4), jt = tid - rt * (c / 4);
            float acc[4][4] = {};
            mac_ws(Gt, KP, Ps, CP, K, 4 * rt, 4 * jt, acc);
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float4 *>(Vt + (4 * rt + a) * CP + 4 * jt) = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        }
        __syncthreads();
        for (int rr = wave; rr < live; rr += LB / 64) {   // (wave-uniform)
            const float xh = lane < c ? Xt[rr * CP + lane] : 0.f, v = lane < c ? Vt[rr * CP + lane] : 0.f;
            const float dot = pdf_wave_sum_f32(xh * v);
            if (lane < c) gx[(r + rr) * c + lane] = scale * (v - (norms[rr] >= NORM_EPS ? xh * dot : 0.f)) * rinv[rr];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Distillation loss.  Row n (one wave): q = smooth softmax(soft) + (1 - smooth) onehot(t), l = -sum_k log_softmax(pred)_k q_k,
// e = -sum_k sm_k log(sm_k + 1e-4); grad[n] = e (softmax(pred) - q) (0 for ignored rows), rowbuf[n] = [l e | e].
__global__ __launch_bounds__(LB) void k_distill_row(long n, int K, const float *__restrict__ pred, const float *__restrict__ soft,
                                                    const long *__restrict__ target, float smooth, float *__restrict__ grad,
                                                    float *__restrict__ rowbuf) {
    const int lane = threadIdx.x & 63;
    for (long r = (long)blockIdx.x * (LB / 64) + (threadIdx.x >> 6); r < n; r += (long)gridDim.x * (LB / 64)) {   // (wave-uniform)
        const float *x = pred + r * K, *y = soft + r * K;
        const long t = target[r];
        const bool valid = t != -1, bad = valid && (t < 0 || t >= K);
        const long hot = valid ? t : 0;   // (the reference scatters ignored rows into class 0; their entropy weight is 0)
        float mx = -__builtin_huge_valf(), my = -__builtin_huge_valf();
        for (int k = lane; k < K; k += 64) { mx = fmaxf(mx, x[k]); my = fmaxf(my, y[k]); }
        mx = pdf_wave_max_f32(mx); my = pdf_wave_max_f32(my);
        float sx = 0.f, sy = 0.f;
        for (int k = lane; k < K; k += 64) { sx += expf(x[k] - mx); sy += expf(y[k] - my); }
        sx = pdf_wave_sum_f32(sx); sy = pdf_wave_sum_f32(sy);
        const float lse = mx + logf(sx);
        float l = 0.f, e = 0.f;
        for (int k = lane; k < K; k += 64) {
            const float sm = expf(y[k] - my) / sy;
            const float q = smooth * sm + (1.f - smooth) * (k == hot ? 1.f : 0.f);
            l += (lse - x[k]) * q;
            e -= sm * logf(sm + 1e-4f);
        }
        l = pdf_wave_sum_f32(l); e = pdf_wave_sum_f32(e);
        const bool counted = valid && !bad;
        for (int k = lane; k < K; k += 64) {
            const float sm = expf(y[k] - my) / sy;
            const float q = smooth * sm + (1.f - smooth) * (k == hot ? 1.f : 0.f);
            grad[r * K + k] = counted ? e * (expf(x[k] - mx) / sx - q) : 0.f;
        }
        if (lane == 0) {
            rowbuf[2 * r] = bad ? __builtin_nanf("") : counted ? l * e : 0.f;   // a bad label poisons the loss
            rowbuf[2 * r + 1] = counted ? e : 0.f;
        }
    }
}

// Workgroup b walks the 256-row chunks b, b + grid, ...: the chunk's labels and pairs go to LDS, thread k adds the rows of class k in
// row order (double) -> part[b][3][K] = [sum l e | sum e | count].  A bad label counts into class 0 (with its NaN).
__global__ __launch_bounds__(LB) void k_distill_class(long n, int K, const long *__restrict__ target, const float *__restrict__ rowbuf,
                                                      double *__restrict__ part) {
    __shared__ int tl[LB];
    __shared__ float le[LB], en[LB];
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (long r0 = (long)blockIdx.x * LB; r0 < n; r0 += (long)gridDim.x * LB) {   // (block-uniform)
        const long r = r0 + threadIdx.x;
        long t = r < n ? target[r] : -1;
        if (t != -1 && (t < 0 || t >= K)) t = 0;
        __syncthreads();
        tl[threadIdx.x] = (int)t;
        le[threadIdx.x] = r < n ? rowbuf[2 * r] : 0.f;
        en[threadIdx.x] = r < n ? rowbuf[2 * r + 1] : 0.f;
        __syncthreads();
        const int k = threadIdx.x;
        if (k < K)
            for (int i = 0; i < LB; ++i)
                if (tl[i] == k) { s1 += (double)le[i]; s2 += (double)en[i]; cnt += 1.0; }
    }
    if ((int)threadIdx.x < K) {
        double *p = part + (size_t)blockIdx.x * 3 * K;
        p[threadIdx.x] = s1; p[K + threadIdx.x] = s2; p[2 * K + threadIdx.x] = cnt;
    }
}

// One workgroup: class k's triple from the parts in workgroup order; loss = sum_present (S1 / (S2 + 1e-4)) / (#present + 1e-4), 0 when no
// class is present; coef[k] = 1 / ((S2_k + 1e-4) (#present + 1e-4)) for present classes, else 0.
__global__ __launch_bounds__(LB) void k_distill_finish(int K, int blocks, const double *__restrict__ part, float *__restrict__ coef,
                                                       float *__restrict__ loss) {
    __shared__ double term[LB], inv[LB];
    __shared__ int here[LB];
    const int k = threadIdx.x;
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    if (k < K)
        for (int b = 0; b < blocks; ++b) {
            const double *p = part + (size_t)b * 3 * K;
            s1 += p[k]; s2 += p[K + k]; cnt += p[2 * K + k];
        }
    here[k] = k < K && cnt > 0.0;
    inv[k] = 1.0 / (s2 + 1e-4);
    term[k] = s1 / (s2 + 1e-4);
    __syncthreads();
    double total = 0.0, present = 0.0;
    for (int i = 0; i < K; ++i)
        if (here[i]) { total += term[i]; present += 1.0; }   // (every thread: ascending class order)
    if (k < K) coef[k] = here[k] ? (float)(inv[k] / (present + 1e-4)) : 0.f;
    if (k == 0) loss[0] = present > 0.0 ? (float)(total / (present + 1e-4)) : 0.f;
}

__global__ __launch_bounds__(LB) void k_distill_bwd(long total, int K, const float *__restrict__ grad, const long *__restrict__ target,
                                                    const float *__restrict__ coef, const float *__restrict__ gy, float *__restrict__ out) {
    const float g0 = gy[0];
    for (long e = (long)blockIdx.x * LB + threadIdx.x; e < total; e += (long)gridDim.x * LB) {
        const long t = target[e / K];
        out[e] = t >= 0 && t < K ? grad[e] * (coef[t] * g0) : 0.f;
    }
}

inline unsigned elem_blocks(long total) {
    const long g = (total + LB - 1) / LB;
    return (unsigned)(g > PDF_MAX_BLOCKS ? PDF_MAX_BLOCKS : g < 1 ? 1 : g);
}
inline size_t sums_lds(int K, int c) { return sizeof(float) * ((size_t)RS * kp_of(K) + (size_t)RS * (c + 4) + RS); }
inline size_t slab_floats(long n, int K, int c, int scenes) { return (size_t)cac_chunks(n, scenes) * scenes * K * (c + 4); }
inline bool bad_shape(long n, int K, int c, int scenes) { return n < 1 || scenes < 1 || scenes > 65535 || !supported(K, c); }

}  // namespace

extern "C" int pdf_cac_supported(int K, int c) { return supported(K, c) ? 1 : 0; }

// floats of `ws` for any pass over n rows in `scenes` scenes: the chunk slabs of the class sums
extern "C" long pdf_cac_workspace_floats(long n, int K, int c, int scenes) {
    if (bad_shape(n, K, c, scenes)) return 0;
    return (long)slab_floats(n, K, c, scenes);
}

extern "C" int pdf_cac_soft_proto_forward(long n, int K, int c, int scenes, const float *feat, const float *logits, const int *offset,
                                          float conf_thresh, float *proto, float *mass, float *ws, void *stream) {
    if (bad_shape(n, K, c, scenes) || !feat || !logits || !offset || !proto || !mass || !ws) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nch = cac_chunks(n, scenes);
    k_class_sums<W_SOFT><<<dim3(nch, scenes), LB, sums_lds(K, c), s>>>(n, K, c, offset, feat, logits, nullptr, conf_thresh, ws);
    k_class_finish<<<pdf_divup((long)scenes * K, LB / 64), LB, 0, s>>>(K, c, scenes, nch, FIN_SOFT, ws, nullptr, 1.f, proto, mass);
    return pdf_launch_status();
}

extern "C" int pdf_cac_soft_proto_backward(long n, int K, int c, int scenes, const float *feat, const float *logits, const int *offset,
                                           float conf_thresh, const float *proto, const float *mass, const float *gproto, float *gfeat,
                                           float *glogits, void *stream) {
    if (bad_shape(n, K, c, scenes) || !feat || !logits || !offset || !proto || !mass || !gproto || !gfeat) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int KP = kp_of(K), CP = c + 4;
    const size_t lds = sizeof(float) * ((size_t)KP * CP + KP + (glogits ? 2 : 1) * (size_t)RR * KP + (size_t)RR * CP);
    const dim3 g(cac_chunks(n, scenes), scenes);
    static PdfLdsLimit site;   // per device (pdfops_common.h)
    if (lds > 64 * 1024 && !pdf_lds_limit_raised(site, reinterpret_cast<const void *>(&k_soft_bwd<true>), (int)SOFT_BWD_LDS)) return PDF_ERR_BAD_ARG;
    if (glogits) k_soft_bwd<true><<<g, LB, lds, s>>>(n, K, c, offset, feat, logits, conf_thresh, proto, mass, gproto, gfeat, glogits);
    else k_soft_bwd<false><<<g, LB, lds, s>>>(n, K, c, offset, feat, logits, conf_thresh, proto, mass, gproto, gfeat, nullptr);
    return pdf_launch_status();
}

extern "C" int pdf_cac_label_proto_forward(long n, int K, int c, const float *feat, const long *target, const float *base, float *proto,
                                           float *count, float *ws, void *stream) {
    if (bad_shape(n, K, c, 1) || !feat || !target || !base || !proto || !count || !ws) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nch = cac_chunks(n, 1);
    k_class_sums<W_ONEHOT><<<dim3(nch, 1), LB, sums_lds(K, c), s>>>(n, K, c, nullptr, feat, nullptr, target, 0.f, ws);
    k_class_finish<<<pdf_divup((long)K, LB / 64), LB, 0, s>>>(K, c, 1, nch, FIN_LABEL, ws, base, 1.f, proto, count);
    return pdf_launch_status();
}

extern "C" int pdf_cac_label_proto_backward(long n, int K, int c, const long *target, const float *count, const float *gproto,
                                            float *gfeat, void *stream) {
    if (bad_shape(n, K, c, 1) || !target || !count || !gproto || !gfeat) return PDF_ERR_BAD_ARG;
    k_label_bwd<<<elem_blocks(n * c), LB, 0, static_cast<hipStream_t>(stream)>>>(n * c, K, c, target, count, gproto, gfeat);
    return pdf_launch_status();
}

extern "C" int pdf_cac_cosine_forward(long n, int K, int c, int scenes, const float *x, const float *proto, const int *offset, float scale,
                                      float *out, void *stream) {
    if (bad_shape(n, K, c, scenes) || !x || !proto || !out || (scenes > 1 && !offset)) return PDF_ERR_BAD_ARG;
    const size_t lds = sizeof(float) * ((size_t)kp_of(K) * (c + 4) + (size_t)RR * (c + 4));
    k_cos_fwd<<<dim3(cac_chunks(n, scenes), scenes), LB, lds, static_cast<hipStream_t>(stream)>>>(n, K, c, offset, x, proto, scale, out);
    return pdf_launch_status();
}

extern "C" int pdf_cac_cosine_backward(long n, int K, int c, int scenes, const float *x, const float *proto, const int *offset, float scale,
                                       const float *gout, float *gx, float *gproto, float *ws, void *stream) {
    if (bad_shape(n, K, c, scenes) || !x || !proto || !gout || !gx || !gproto || !ws || (scenes > 1 && !offset)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int KP = kp_of(K), CP = c + 4, nch = cac_chunks(n, scenes);
    const size_t lds = sizeof(float) * ((size_t)KP * CP + (size_t)RR * KP + 2 * (size_t)RR * CP + 2 * RR);
    k_cos_bwd_x<<<dim3(nch, scenes), LB, lds, s>>>(n, K, c, offset, x, proto, scale, gout, gx);
    k_class_sums<W_GIVEN><<<dim3(nch, scenes), LB, sums_lds(K, c), s>>>(n, K, c, offset, x, gout, nullptr, 0.f, ws);
    k_class_finish<<<pdf_divup((long)scenes * K, LB / 64), LB, 0, s>>>(K, c, scenes, nch, FIN_COSGRAD, ws, proto, scale, gproto, nullptr);
    return pdf_launch_status();
}

// floats of `acc` of the distillation loss: the per-workgroup class triples (doubles, first: 8-byte aligned) and the K class coefficients
extern "C" long pdf_cac_distill_workspace_floats(int K) {
    if (K < 1 || K > LB) return 0;
    return 2L * DIST_BLOCKS * 3 * K + K;
}

extern "C" int pdf_cac_distill_forward(long n, int K, const float *pred, const float *soft, const long *target, float smoothness,
                                       float *grad, float *rowbuf, float *acc, float *loss, void *stream) {
    if (n < 1 || K < 1 || K > LB || !pred || !soft || !target || !grad || !rowbuf || !acc || !loss) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long rows = (n + LB / 64 - 1) / (LB / 64);
    k_distill_row<<<(unsigned)(rows > PDF_MAX_BLOCKS ? PDF_MAX_BLOCKS : rows), LB, 0, s>>>(n, K, pred, soft, target, smoothness, grad, rowbuf);
    const long chunks = (n + LB - 1) / LB;
    const int blocks = (int)(chunks > DIST_BLOCKS ? DIST_BLOCKS : chunks);
    double *part = reinterpret_cast<double *>(acc);
    k_distill_class<<<blocks, LB, 0, s>>>(n, K, target, rowbuf, part);
    k_distill_finish<<<1, LB, 0, s>>>(K, blocks, part, acc + 2L * DIST_BLOCKS * 3 * K, loss);
    return pdf_launch_status();
}

extern "C" int pdf_cac_distill_backward(long n, int K, const float *grad, const long *target, const float *acc, const float *gy,
                                        float *grad_out, void *stream) {
    if (n < 1 || K < 1 || K > LB || !grad || !target || !acc || !gy || !grad_out) return PDF_ERR_BAD_ARG;
    k_distill_bwd<<<elem_blocks(n * K), LB, 0, static_cast<hipStream_t>(stream)>>>(n * K, K, grad, target, acc + 2L * DIST_BLOCKS * 3 * K,
                                                                                    gy, grad_out);
    return pdf_launch_status();
}
