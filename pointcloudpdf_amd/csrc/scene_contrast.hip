// MSC-v1m1 (pointcept/models/masked_scene_contrast/masked_scene_contrast_v1m1_base.py) -- the two loss stages as HIP passes.
//
// Matched-pair InfoNCE (:174-203).  The reference gathers the P matched rows of both views, normalises them, forms the (P, P) similarity
// matrix, divides it by the temperature and runs cross-entropy against the diagonal.  Here no (P, P) array exists in either direction:
//
//   k_rows      a wave per pair: A^ = a / (|a| + 1e-7), B^ likewise (norm = fixed-order sum), padded with zero rows to a multiple of 128.
//   k_fwd       workgroup = 128 rows of A^ x a stretch of 128-column tiles of B^ (ascending).  A tile of S = A^ B^T is formed on the matrix
//               cores (v_mfma_f32_32x32x2_f32: fp32 in, fp32 out, staged through LDS in chunks of 32 channels, as spc::k_gconv does) and
//               folded into per-lane running (max, sum of exp) of s / t, the plain row sum of s and s_ii.  The columns are split over
//               grid.y as well (P = 8,192 has only 64 row tiles); the lanes' states are merged by a fixed butterfly.
//   k_fwd_fin   one workgroup: merges the splits' (max, sum, rowsum) in split order -> lse_i (kept for the backward), and the three means in
//               double in a fixed order.
//   k_bwd       G = g (softmax(S / t) - I) / (P t).  grid.z = 0: row-tile owners recompute their S tiles and accumulate dA^ = G B^;
//               grid.z = 1: column-tile owners recompute S^T = B^ A^T and accumulate dB^ = G^T A^.  The walked range is split over grid.y
//               into partial slabs.  No atomics: the order of every sum is a function of P and C.
//   k_adjoint   a wave per pair and side: sums the slabs in split order and applies the adjoint of the normalisation.
//   k_scatter   a thread per (row of the view, 4 channels): the pairs that point at the row are found by binary search in the stably sorted
//               indices (tile_sort.h) and added in ascending pair order; rows without a pair are written as zeros.
//
// Masked reconstruction heads (:274-307).  k_recon_fwd: 32 lanes per row; a masked row forms its three outputs and its loss term, the
// per-workgroup slots are totalled by one workgroup in double (slot_sum.h); the denominator is the masked count of the same pass.
// k_recon_bwd writes d feat (zero rows where unmasked) and per-workgroup slabs of d weight | d bias, summed in slab order.
#include "slot_sum.h"
#include "tile_sort.h"

namespace msc {
namespace {

constexpr int TB = 256;
constexpr int TR = 128;      // rows and columns of an S tile
constexpr int LS = 33;       // row stride of a staged 32-channel chunk in LDS (floats)
constexpr int MAXC = 256;
constexpr float EPS = 1e-7f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline long padded(long p) { return (p + TR - 1) / TR * TR; }
// column splits: fill ~512 workgroups, every split a stretch of `per` column tiles, none empty -- a function of P alone
inline int splits(long p) {
    const long tiles = padded(p) / TR;
    long ns = (512 + tiles - 1) / tiles;
    if (ns > tiles) ns = tiles;
    if (ns < 1) ns = 1;
    const long per = (tiles + ns - 1) / ns;
    return (int)((tiles + per - 1) / per);
}

struct Saved {   // the forward's state for the backward, one float array
    float *hat[2], *norm[2], *lse;
};
inline size_t carve_saved(float *base, long p, int c, Saved &s) {
    const size_t pp = (size_t)padded(p);
    if (base) {
        s.hat[0] = base; s.hat[1] = base + pp * c;
        s.norm[0] = base + 2 * pp * c; s.norm[1] = s.norm[0] + pp;
        s.lse = s.norm[1] + pp;
    }
    return 2 * pp * c + 3 * pp;
}

struct FwdWs { float *pm, *pl, *ps, *diag; };
inline size_t carve_fwd(void *base, long p, FwdWs &w) {
    PdfCarver cv{static_cast<char *>(base)};
    const size_t pp = (size_t)padded(p), ns = (size_t)splits(p);
    w.pm = cv.take<float>(ns * pp);
    w.pl = cv.take<float>(ns * pp);
    w.ps = cv.take<float>(ns * pp);
    w.diag = cv.take<float>(pp);
    return cv.off;
}

struct BwdWs { float *part, *da; unsigned *key[2], *pay[2], *hist; };
inline size_t carve_bwd(void *base, long p, int c, BwdWs &w) {
    PdfCarver cv{static_cast<char *>(base)};
    const size_t pp = (size_t)padded(p), ns = (size_t)splits(p);
    const size_t nt = (size_t)((p + tile_sort::TILE - 1) / tile_sort::TILE);
    w.part = cv.take<float>(2 * ns * pp * c);
    w.da = cv.take<float>(2 * (size_t)p * c);
    for (int k = 0; k < 2; ++k) w.key[k] = cv.take<unsigned>(2 * (size_t)p);
    for (int k = 0; k < 2; ++k) w.pay[k] = cv.take<unsigned>(2 * (size_t)p);
    w.hist = cv.take<unsigned>(2 * nt * tile_sort::RADIX);
    return cv.off;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// row pass
// ---------------------------------------------------------------------------------------------------------------------------------------
struct RowArgs {
    const float *feat[2]; long n[2];
    const long long *match; long p, pp; int c;
    float *hat[2], *norm[2];
};

__global__ __launch_bounds__(TB) void k_rows(RowArgs a) {
    const int lane = threadIdx.x & 63, side = blockIdx.y;
    const long i = (long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (i >= a.pp) return;   // (wave-uniform)
    float *dst = a.hat[side] + (size_t)i * a.c;
    long src = -1;
    if (i < a.p) {
        src = (long)a.match[2 * i + side];
        if (src < 0 || src >= a.n[side]) src = -1;   // (an index outside the view reads nothing: a zero row)
    }
    float v[MAXC / 64], ss = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC / 64; ++j) {
        const int ch = lane + 64 * j;
        v[j] = (src >= 0 && ch < a.c) ? a.feat[side][(size_t)src * a.c + ch] : 0.f;
        ss += v[j] * v[j];
    }
    ss = pdf_wave_sum_f32(ss);
    const float nrm = sqrtf(ss), den = nrm + EPS;
#pragma unroll
    for (int j = 0; j < MAXC / 64; ++j) {
        const int ch = lane + 64 * j;
        if (ch < a.c) dst[ch] = v[j] / den;
    }
    if (lane == 0) a.norm[side][i] = nrm;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// one 128 x 128 tile of X Y^T on the matrix cores: X rows [r0, r0 + 128), Y rows [c0, c0 + 128), both (pp, c) with pp a multiple of 128.
// Wave wv owns the rows [32 wv, 32 wv + 32); acc[nb][r] = the element at row 32 wv + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column
// 32 nb + (lane & 31).  Xs, Ys: TR * LS floats each.  Starts with a barrier (the buffers may still be read), ends without one.
// ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void s_tile(const float *__restrict__ X, const float *__restrict__ Y, int c, long r0, long c0, float *Xs, float *Ys,
                                       f32x16 (&acc)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    for (int k0 = 0; k0 < c; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = tid + TB * j, t = e >> 3, q = e & 7;
            const float4 xv = *reinterpret_cast<const float4 *>(X + (size_t)(r0 + t) * c + k0 + 4 * q);
            const float4 yv = *reinterpret_cast<const float4 *>(Y + (size_t)(c0 + t) * c + k0 + 4 * q);
            float *dx = Xs + t * LS + 4 * q, *dy = Ys + t * LS + 4 * q;
            dx[0] = xv.x; dx[1] = xv.y; dx[2] = xv.z; dx[3] = xv.w;
            dy[0] = yv.x; dy[1] = yv.y; dy[2] = yv.z; dy[3] = yv.w;
        }
        __syncthreads();
        const float *ap = Xs + (32 * wv + li) * LS + lh;
        const float *bp = Ys + li * LS + lh;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const float av = ap[2 * s];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[nb * 32 * LS + 2 * s], acc[nb], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ int row_of(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ---------------------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    const float *A, *B; long p, pp; int c, ns; float t;
    float *pm, *pl, *ps, *diag;
};

__global__ __launch_bounds__(TB) void k_fwd(FwdArgs a) {
    __shared__ float Xs[TR * LS];
    __shared__ float Ys[TR * LS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const long r0 = (long)blockIdx.x * TR;
    const int tiles = (int)(a.pp / TR), per = (tiles + a.ns - 1) / a.ns;
    const int z = blockIdx.y, t0 = z * per, t1 = min(tiles, t0 + per);
    float m[16], l[16], rs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { m[r] = -INFINITY; l[r] = 0.f; rs[r] = 0.f; }
    f32x16 acc[4];
    for (int ct = t0; ct < t1; ++ct) {
        const long c0 = (long)ct * TR;
        s_tile(a.A, a.B, a.c, r0, c0, Xs, Ys, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long grow = r0 + 32 * wv + row_of(r, lh);
            float v[4], mt = -INFINITY;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const long gcol = c0 + nb * 32 + li;
                const bool ok = gcol < a.p;
                const float s = acc[nb][r];
                rs[r] += ok ? s : 0.f;
                v[nb] = ok ? s / a.t : -INFINITY;
                mt = fmaxf(mt, v[nb]);
                if (ok && gcol == grow) a.diag[grow] = s;
            }
            if (mt > -INFINITY) {
                const float mn = fmaxf(m[r], mt);
                float e = 0.f;
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) e += expf(v[nb] - mn);
                l[r] = l[r] * expf(m[r] - mn) + e;
                m[r] = mn;
            }
        }
    }
    // the 32 lanes that share a row: fixed butterfly (both partners form the same sum)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 1; o <= 16; o <<= 1) {
            const float m2 = __shfl_xor(m[r], o, 64), l2 = __shfl_xor(l[r], o, 64), s2 = __shfl_xor(rs[r], o, 64);
            const float mn = fmaxf(m[r], m2);
            const float e1 = m[r] == mn ? 1.f : expf(m[r] - mn), e2 = m2 == mn ? 1.f : expf(m2 - mn);
            l[r] = l[r] * e1 + l2 * e2;
            m[r] = mn;
            rs[r] += s2;
        }
        if (li == 0) {
            const size_t at = (size_t)z * a.pp + (size_t)(r0 + 32 * wv + row_of(r, lh));
            a.pm[at] = m[r]; a.pl[at] = l[r]; a.ps[at] = rs[r];
        }
    }
}

// one workgroup: lse per row, the three means in double (lane-strided rows, then by lanes: slot_sum.h)
__global__ __launch_bounds__(TB) void k_fwd_fin(FwdArgs a, float *__restrict__ lse, float *__restrict__ out) {
    double s_loss = 0.0, s_pos = 0.0, s_all = 0.0;
    for (long i = threadIdx.x; i < a.p; i += TB) {
        float m = -INFINITY;
        for (int z = 0; z < a.ns; ++z) m = fmaxf(m, a.pm[(size_t)z * a.pp + i]);
        float l = 0.f, rs = 0.f;
        for (int z = 0; z < a.ns; ++z) {
            const float mz = a.pm[(size_t)z * a.pp + i];
            l += a.pl[(size_t)z * a.pp + i] * (mz == m ? 1.f : expf(mz - m));
            rs += a.ps[(size_t)z * a.pp + i];
        }
        const float e = m + logf(l), d = a.diag[i];
        lse[i] = e;
        s_loss += (double)(e - d / a.t);
        s_pos += (double)d;
        s_all += (double)rs / (double)a.p;
    }
    const double v[3] = {s_loss, s_pos, s_all};
    double t[3];
    if (!block_sum_by_lanes<TB>(v, t)) return;
    const double p = (double)a.p;
    out[0] = (float)(t[0] / p);
    out[1] = (float)(t[1] / p);
    out[2] = (float)(t[2] / p - (t[1] / p) / p);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    const float *hat[2], *lse, *gy; long p, pp; int c, ns, ys; float t;
    float *part;   // [2][ns][pp][c]
};

template <int NCB>
__global__ __launch_bounds__(TB) void k_bwd(BwdArgs a) {
    extern __shared__ float lds[];
    float *Xs = lds, *Ys = lds + TR * LS, *Yt = lds + 2 * TR * LS;   // G's 32-column strip takes Xs over once the tile is formed
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int dir = blockIdx.z, z = blockIdx.y, c = NCB * 32;
    const float *X = a.hat[dir], *Y = a.hat[dir ^ 1];
    const long r0 = (long)blockIdx.x * TR;
    const int tiles = (int)(a.pp / TR), per = (tiles + a.ns - 1) / a.ns;
    const int t0 = z * per, t1 = min(tiles, t0 + per);
    const float scale = a.gy[0] / ((float)a.p * a.t);
    f32x16 dx[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dx[cb][r] = 0.f;
    f32x16 acc[4];
    for (int wt = t0; wt < t1; ++wt) {
        const long w0 = (long)wt * TR;
        s_tile(X, Y, c, r0, w0, Xs, Ys, acc);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tr = 32 * wv + row_of(r, lh);
                const long orow = r0 + tr, wcol = w0 + nb * 32 + li;
                const long i = dir ? wcol : orow, j = dir ? orow : wcol;
                float g = 0.f;
                if (i < a.p && j < a.p) g = (expf(acc[nb][r] / a.t - a.lse[i]) - (i == j ? 1.f : 0.f)) * scale;
                Xs[tr * LS + li] = g;
            }
            for (int e = tid; e < 8 * c; e += TB) {
                const int t = e / (c / 4), q = e - t * (c / 4);
                const float4 yv = *reinterpret_cast<const float4 *>(Y + (size_t)(w0 + nb * 32 + t) * c + 4 * q);
                *reinterpret_cast<float4 *>(Yt + t * a.ys + 4 * q) = yv;
            }
            __syncthreads();
            const float *ap = Xs + (32 * wv + li) * LS + lh;
            const float *bp = Yt + lh * a.ys + li;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const float av = ap[2 * s];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) dx[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * s * a.ys + cb * 32], dx[cb], 0, 0, 0);
            }
        }
    }
    float *dst = a.part + ((size_t)(dir * a.ns + z) * a.pp + r0 + 32 * wv) * c;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(size_t)row_of(r, lh) * c + cb * 32 + li] = dx[cb][r];
}

template <int NCB>
int launch_bwd(const BwdArgs &a, hipStream_t s) {
    static PdfLdsLimit limit;
    const int bytes = (2 * TR * LS + 32 * a.ys) * (int)sizeof(float);
    if (bytes > 48 * 1024 && !pdf_lds_limit_raised(limit, reinterpret_cast<const void *>(&k_bwd<NCB>), bytes)) return PDF_ERR_UNSUPPORTED;
    k_bwd<NCB><<<dim3((unsigned)(a.pp / TR), (unsigned)a.ns, 2), TB, bytes, s>>>(a);
    return PDF_OK;
}

struct AdjArgs {
    const float *feat[2]; long n[2];
    const long long *match; long p, pp; int c, ns;
    const float *norm[2], *part; float *da;   // da [2][p][c]
};

__global__ __launch_bounds__(TB) void k_adjoint(AdjArgs a) {
    const int lane = threadIdx.x & 63, side = blockIdx.y;
    const long i = (long)blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (i >= a.p) return;   // (wave-uniform)
    long src = (long)a.match[2 * i + side];
    if (src < 0 || src >= a.n[side]) src = -1;
    float v[MAXC / 64], d[MAXC / 64], dot = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC / 64; ++j) {
        const int ch = lane + 64 * j;
        const bool ok = ch < a.c;
        v[j] = (ok && src >= 0) ? a.feat[side][(size_t)src * a.c + ch] : 0.f;
        float sum = 0.f;
        if (ok)
            for (int z = 0; z < a.ns; ++z) sum += a.part[((size_t)(side * a.ns + z) * a.pp + i) * a.c + ch];
        d[j] = sum;
        dot += v[j] * d[j];
    }
    dot = pdf_wave_sum_f32(dot);
    const float nrm = a.norm[side][i], den = nrm + EPS;
    const float k = nrm > 0.f ? dot / (nrm * den * den) : 0.f;   // (torch.norm's subgradient at a zero row is zero)
    float *dst = a.da + ((size_t)side * a.p + i) * a.c;
#pragma unroll
    for (int j = 0; j < MAXC / 64; ++j) {
        const int ch = lane + 64 * j;
        if (ch < a.c) dst[ch] = d[j] / den - v[j] * k;
    }
}

__global__ __launch_bounds__(TB) void k_keys(long p, long n1, long n2, const long long *__restrict__ match, unsigned *__restrict__ key,
                                             unsigned *__restrict__ pay) {
    const long e = (long)blockIdx.x * TB + threadIdx.x;
    if (e >= 2 * p) return;
    const int side = e >= p;
    const long i = e - (side ? p : 0);
    const long v = (long)match[2 * i + side];
    key[e] = (v < 0 || v >= (side ? n2 : n1)) ? 0xffffffffu : (unsigned)v;   // (never found by a row's search)
    pay[e] = (unsigned)i;
}

struct ScatterArgs {
    long n[2], p; int c;
    const unsigned *key, *pay;   // [2][p] sorted by index, equal indices in ascending pair order
    const float *da; float *g[2];
};

__global__ __launch_bounds__(TB) void k_scatter(ScatterArgs a) {
    const int q4 = a.c / 4;
    const long total = (a.n[0] + a.n[1]) * q4;
    for (long e = (long)blockIdx.x * TB + threadIdx.x; e < total; e += (long)gridDim.x * TB) {
        long row = e / q4;
        const int q = (int)(e - row * q4);
        const int side = row >= a.n[0];
        if (side) row -= a.n[0];
        const unsigned *key = a.key + (size_t)side * a.p, *pay = a.pay + (size_t)side * a.p;
        long lo = 0, hi = a.p;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if ((long)key[mid] < row) lo = mid + 1; else hi = mid;
        }
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (; lo < a.p && (long)key[lo] == row; ++lo) {
            const float4 v = *reinterpret_cast<const float4 *>(a.da + ((size_t)side * a.p + pay[lo]) * a.c + 4 * q);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4 *>(a.g[side] + (size_t)row * a.c + 4 * q) = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// reconstruction heads
// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int RG = TB / 32;        // rows in flight per workgroup (32 lanes each)
constexpr int RMAXB = 1024;        // workgroups at most: slots and slabs
constexpr int ACC_HEAD = 4;        // acc[0] = 1 / count (0 without a masked row), acc[1] = count; slots from acc[ACC_HEAD]

inline int recon_blocks(long n) {
    long b = (n + 8 * RG - 1) / (8 * RG);
    return (int)(b < 1 ? 1 : (b > RMAXB ? RMAXB : b));
}

struct ReconArgs {
    long n[2]; int c, kind;
    const float *feat[2], *target[2]; const unsigned char *mask[2];
    const float *w, *bias;
    float *dpred;    // (n1 + n2, 3): d term / d prediction of the masked rows
    double *acc;
    const float *gy; float *g[2]; float *slab;
};

__global__ __launch_bounds__(TB) void k_recon_fwd(ReconArgs a) {
    __shared__ double ssum[RG];
    __shared__ long long scnt[RG];
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const long total = a.n[0] + a.n[1], stride = (long)gridDim.x * RG;
    float w[3][MAXC / 32];
#pragma unroll
    for (int j = 0; j < MAXC / 32; ++j) {
        const int ch = lane + 32 * j;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k][j] = ch < a.c ? a.w[k * a.c + ch] : 0.f;
    }
    const float b0 = a.bias[0], b1 = a.bias[1], b2 = a.bias[2];
    double sum = 0.0;
    long long cnt = 0;
    for (long r = (long)blockIdx.x * RG + grp; r < total; r += stride) {
        const int side = r >= a.n[0];
        const long row = side ? r - a.n[0] : r;
        if (!a.mask[side][row]) continue;   // (uniform over the 32 lanes of the row)
        const float *f = a.feat[side] + (size_t)row * a.c;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
        for (int j = 0; j < MAXC / 32; ++j) {
            const int ch = lane + 32 * j;
            const float x = ch < a.c ? f[ch] : 0.f;
            p0 += x * w[0][j]; p1 += x * w[1][j]; p2 += x * w[2][j];
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) { p0 += __shfl_xor(p0, o, 64); p1 += __shfl_xor(p1, o, 64); p2 += __shfl_xor(p2, o, 64); }
        p0 += b0; p1 += b1; p2 += b2;
        const float *t = a.target[side] + (size_t)row * 3;
        const float t0 = t[0], t1 = t[1], t2 = t[2];
        float term, d0, d1, d2;
        if (a.kind == 0) {   // sum (pred - color)^2
            const float e0 = p0 - t0, e1 = p1 - t1, e2 = p2 - t2;
            term = e0 * e0 + e1 * e1 + e2 * e2;
            d0 = 2.f * e0; d1 = 2.f * e1; d2 = 2.f * e2;
        } else {             // sum (pred / (|pred| + 1e-10)) * normal
            const float nrm = sqrtf(p0 * p0 + p1 * p1 + p2 * p2), den = nrm + 1e-10f;
            const float dot = p0 * t0 + p1 * t1 + p2 * t2;
            term = (p0 / den) * t0 + (p1 / den) * t1 + (p2 / den) * t2;
            const float k = nrm > 0.f ? dot / (nrm * den * den) : 0.f;   // (the norm's subgradient at a zero prediction is zero)
            d0 = t0 / den - p0 * k; d1 = t1 / den - p1 * k; d2 = t2 / den - p2 * k;
        }
        if (lane == 0) {
            float *d = a.dpred + (size_t)r * 3;
            d[0] = d0; d[1] = d1; d[2] = d2;
        }
        sum += (double)term;
        cnt += 1;
    }
    if (lane == 0) { ssum[grp] = sum; scnt[grp] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        long long n = 0;
        for (int k = 0; k < RG; ++k) { s += ssum[k]; n += scnt[k]; }
        a.acc[ACC_HEAD + 2 * blockIdx.x] = s;
        a.acc[ACC_HEAD + 2 * blockIdx.x + 1] = (double)n;
    }
}

__global__ __launch_bounds__(TB) void k_recon_fwd_fin(int slots, double *__restrict__ acc, float *__restrict__ loss) {
    double t[2];   // [sum of terms, masked rows]
    if (!slot_total<TB>(acc + ACC_HEAD, slots, t)) return;
    loss[0] = (float)(t[0] / t[1]);             // 0 / 0 = NaN without a masked row, as upstream
    acc[0] = t[1] > 0.0 ? 1.0 / t[1] : 0.0;
    acc[1] = t[1];
}

__global__ __launch_bounds__(TB) void k_recon_bwd(ReconArgs a) {
    __shared__ float red[RG][3 * MAXC + 3];
    const int lane = threadIdx.x & 31, grp = threadIdx.x >> 5;
    const long total = a.n[0] + a.n[1], stride = (long)gridDim.x * RG;
    const float scale = a.gy[0] * (float)a.acc[0];
    float w[3][MAXC / 32], dw[3][MAXC / 32], db[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < MAXC / 32; ++j) {
        const int ch = lane + 32 * j;
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k][j] = ch < a.c ? a.w[k * a.c + ch] : 0.f; dw[k][j] = 0.f; }
    }
    for (long r = (long)blockIdx.x * RG + grp; r < total; r += stride) {
        const int side = r >= a.n[0];
        const long row = side ? r - a.n[0] : r;
        float *g = a.g[side] + (size_t)row * a.c;
        if (!a.mask[side][row]) {
#pragma unroll
            for (int j = 0; j < MAXC / 32; ++j)
                if (lane + 32 * j < a.c) g[lane + 32 * j] = 0.f;
            continue;
        }
        const float *d = a.dpred + (size_t)r * 3;
        const float d0 = d[0], d1 = d[1], d2 = d[2];
        const float *f = a.feat[side] + (size_t)row * a.c;
        db[0] += d0; db[1] += d1; db[2] += d2;
#pragma unroll
        for (int j = 0; j < MAXC / 32; ++j) {
            const int ch = lane + 32 * j;
            if (ch < a.c) {
                const float x = f[ch];
                g[ch] = scale * (d0 * w[0][j] + d1 * w[1][j] + d2 * w[2][j]);
                dw[0][j] += d0 * x; dw[1][j] += d1 * x; dw[2][j] += d2 * x;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MAXC / 32; ++j) {
        const int ch = lane + 32 * j;
        if (ch < a.c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) red[grp][k * a.c + ch] = dw[k][j];
        }
    }
    if (lane == 0) { red[grp][3 * a.c] = db[0]; red[grp][3 * a.c + 1] = db[1]; red[grp][3 * a.c + 2] = db[2]; }
    __syncthreads();
    const int width = 3 * a.c + 3;
    for (int e = threadIdx.x; e < width; e += TB) {
        float s = 0.f;
        for (int k = 0; k < RG; ++k) s += red[k][e];
        a.slab[(size_t)blockIdx.x * width + e] = s;
    }
}

__global__ __launch_bounds__(TB) void k_recon_bwd_fin(int slabs, int c, const float *__restrict__ slab, const double *__restrict__ acc,
                                                      const float *__restrict__ gy, float *__restrict__ gw, float *__restrict__ gb) {
    const int width = 3 * c + 3, e = blockIdx.x * TB + threadIdx.x;
    if (e >= width) return;
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += (double)slab[(size_t)k * width + e];
    const float v = (float)(s * (double)gy[0] * acc[0]);
    if (e < 3 * c) gw[e] = v; else gb[e - 3 * c] = v;
}

}  // namespace
}  // namespace msc

extern "C" {

int pdf_msc_nce_supported(int c) { return c >= 32 && c <= msc::MAXC && c % 32 == 0; }

long pdf_msc_nce_saved_floats(long p, int c) {
    if (p < 1 || !pdf_msc_nce_supported(c)) return 0;
    msc::Saved s;
    return (long)msc::carve_saved(nullptr, p, c, s);
}

long pdf_msc_nce_workspace_bytes(long p, int c, int backward) {
    if (p < 1 || !pdf_msc_nce_supported(c)) return 0;
    if (backward) { msc::BwdWs w; return (long)msc::carve_bwd(nullptr, p, c, w); }
    msc::FwdWs w;
    return (long)msc::carve_fwd(nullptr, p, w);
}

int pdf_msc_nce_forward(long p, int c, long n1, long n2, const float *feat1, const float *feat2, const long long *match, float temperature,
                        float *saved, float *out, void *workspace, long workspace_bytes, void *stream) {
    if (p < 1 || n1 < 0 || n2 < 0 || !feat1 || !feat2 || !match || !saved || !out || !workspace || !(temperature > 0.f)) return PDF_ERR_BAD_ARG;
    if (!pdf_msc_nce_supported(c) || p >= (1l << 31) - msc::TR || n1 >= (1l << 31) || n2 >= (1l << 31)) return PDF_ERR_UNSUPPORTED;
    if (workspace_bytes < pdf_msc_nce_workspace_bytes(p, c, 0) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    msc::Saved sv;
    msc::carve_saved(saved, p, c, sv);
    msc::FwdWs w;
    msc::carve_fwd(workspace, p, w);
    const long pp = msc::padded(p);
    msc::RowArgs ra{{feat1, feat2}, {n1, n2}, match, p, pp, c, {sv.hat[0], sv.hat[1]}, {sv.norm[0], sv.norm[1]}};
    msc::k_rows<<<dim3((unsigned)(pp / (msc::TB / 64)), 2), msc::TB, 0, s>>>(ra);
    msc::FwdArgs fa{sv.hat[0], sv.hat[1], p, pp, c, msc::splits(p), temperature, w.pm, w.pl, w.ps, w.diag};
    msc::k_fwd<<<dim3((unsigned)(pp / msc::TR), (unsigned)fa.ns), msc::TB, 0, s>>>(fa);
    msc::k_fwd_fin<<<1, msc::TB, 0, s>>>(fa, sv.lse, out);
    return pdf_launch_status();
}

int pdf_msc_nce_backward(long p, int c, long n1, long n2, const float *feat1, const float *feat2, const long long *match, float temperature,
                         const float *saved, const float *gy, float *g1, float *g2, void *workspace, long workspace_bytes, void *stream) {
    if (p < 1 || n1 < 0 || n2 < 0 || !feat1 || !feat2 || !match || !saved || !gy || !workspace || !(temperature > 0.f)) return PDF_ERR_BAD_ARG;
    if ((n1 > 0 && !g1) || (n2 > 0 && !g2)) return PDF_ERR_BAD_ARG;
    if (!pdf_msc_nce_supported(c) || p >= (1l << 31) - msc::TR || n1 >= (1l << 31) || n2 >= (1l << 31)) return PDF_ERR_UNSUPPORTED;
    if (workspace_bytes < pdf_msc_nce_workspace_bytes(p, c, 1) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    msc::Saved sv;
    msc::carve_saved(const_cast<float *>(saved), p, c, sv);
    msc::BwdWs w;
    msc::carve_bwd(workspace, p, c, w);
    const long pp = msc::padded(p);
    const int ns = msc::splits(p);
    msc::BwdArgs ba{{sv.hat[0], sv.hat[1]}, sv.lse, gy, p, pp, c, ns, (c % 64 == 32) ? c : c + 32, temperature, w.part};
    int rc = PDF_OK;
    switch (c / 32) {
        case 1: rc = msc::launch_bwd<1>(ba, s); break;
        case 2: rc = msc::launch_bwd<2>(ba, s); break;
        case 3: rc = msc::launch_bwd<3>(ba, s); break;
        case 4: rc = msc::launch_bwd<4>(ba, s); break;
        case 5: rc = msc::launch_bwd<5>(ba, s); break;
        case 6: rc = msc::launch_bwd<6>(ba, s); break;
        case 7: rc = msc::launch_bwd<7>(ba, s); break;
        default: rc = msc::launch_bwd<8>(ba, s); break;
    }
    if (rc != PDF_OK) return rc;
    msc::AdjArgs aa{{feat1, feat2}, {n1, n2}, match, p, pp, c, ns, {sv.norm[0], sv.norm[1]}, w.part, w.da};
    msc::k_adjoint<<<dim3((unsigned)pdf_divup(p, msc::TB / 64), 2), msc::TB, 0, s>>>(aa);
    msc::k_keys<<<(unsigned)pdf_divup(2 * p, msc::TB), msc::TB, 0, s>>>(p, n1, n2, match, w.key[0], w.pay[0]);
    const int cur = tile_sort::sort<unsigned, false>(p, 2, w.key, w.pay, w.hist, nullptr, s);
    if (n1 + n2 > 0) {
        msc::ScatterArgs sa{{n1, n2}, p, c, w.key[cur], w.pay[cur], w.da, {g1, g2}};
        const long b = ((n1 + n2) * (c / 4) + msc::TB - 1) / msc::TB;
        msc::k_scatter<<<(unsigned)(b < 8 * PDF_MAX_BLOCKS ? b : 8 * PDF_MAX_BLOCKS), msc::TB, 0, s>>>(sa);
    }
    return pdf_launch_status();
}

int pdf_msc_recon_supported(int c) { return c >= 32 && c <= msc::MAXC && c % 32 == 0; }
long pdf_msc_recon_acc_doubles(void) { return msc::ACC_HEAD + 2 * msc::RMAXB; }
long pdf_msc_recon_slab_floats(long n, int c) { return n < 0 || !pdf_msc_recon_supported(c) ? 0 : (long)msc::recon_blocks(n) * (3 * c + 3); }

int pdf_msc_recon_forward(long n1, long n2, int c, int kind, const float *feat1, const float *feat2, const unsigned char *mask1,
                          const unsigned char *mask2, const float *weight, const float *bias, const float *target1, const float *target2,
                          float *dpred, double *acc, float *loss, void *stream) {
    if (n1 < 0 || n2 < 0 || kind < 0 || kind > 1 || !weight || !bias || !acc || !loss) return PDF_ERR_BAD_ARG;
    if ((n1 > 0 && (!feat1 || !mask1 || !target1)) || (n2 > 0 && (!feat2 || !mask2 || !target2)) || (n1 + n2 > 0 && !dpred)) return PDF_ERR_BAD_ARG;
    if (!pdf_msc_recon_supported(c)) return PDF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = msc::recon_blocks(n1 + n2);
    msc::ReconArgs a{{n1, n2}, c, kind, {feat1, feat2}, {target1, target2}, {mask1, mask2}, weight, bias, dpred, acc, nullptr, {nullptr, nullptr}, nullptr};
    msc::k_recon_fwd<<<(unsigned)blocks, msc::TB, 0, s>>>(a);
    msc::k_recon_fwd_fin<<<1, msc::TB, 0, s>>>(blocks, acc, loss);
    return pdf_launch_status();
}

int pdf_msc_recon_backward(long n1, long n2, int c, const float *feat1, const float *feat2, const unsigned char *mask1, const unsigned char *mask2,
                           const float *weight, const float *dpred, const double *acc, const float *gy, float *g1, float *g2, float *gw, float *gb,
                           float *slab, void *stream) {
    if (n1 < 0 || n2 < 0 || !weight || !acc || !gy || !gw || !gb || !slab) return PDF_ERR_BAD_ARG;
    if ((n1 > 0 && (!feat1 || !mask1 || !g1)) || (n2 > 0 && (!feat2 || !mask2 || !g2)) || (n1 + n2 > 0 && !dpred)) return PDF_ERR_BAD_ARG;
    if (!pdf_msc_recon_supported(c)) return PDF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = msc::recon_blocks(n1 + n2);
    msc::ReconArgs a{{n1, n2}, c, 0, {feat1, feat2}, {nullptr, nullptr}, {mask1, mask2}, weight, nullptr, const_cast<float *>(dpred),
                     const_cast<double *>(acc), gy, {g1, g2}, slab};
    msc::k_recon_bwd<<<(unsigned)blocks, msc::TB, 0, s>>>(a);
    msc::k_recon_bwd_fin<<<(unsigned)pdf_divup(3 * c + 3, msc::TB), msc::TB, 0, s>>>(blocks, c, slab, acc, gy, gw, gb);
    return pdf_launch_status();
}

}  // extern "C"
