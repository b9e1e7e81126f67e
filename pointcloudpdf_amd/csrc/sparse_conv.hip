// Sparse 3-D convolutions (the three spconv operators SpUNet-v1m1 uses) as launches on the caller's stream: coordinate-only geometry
// and fp32 gather-convolutions on the matrix cores.  No float atomics, fixed summation orders (bit-reproducible), nothing allocated.
//
// Sites: indices (n, 4) int32 = [batch, d0, d1, d2].  Key of a site = batch << 48 | d0 << 32 | d1 << 16 | d2 (coordinates in [0, 2^16),
// batch in [0, 2^15)); the all-ones word is the "no site" sentinel and sorts last.  Ascending keys = ascending (batch, d0, d1, d2).
//
//   geometry   pdf_spconv_sort_sites   level 0: keys -> stable sort (csrc/tile_sort.h, two 32-bit sorts like csrc/grid_pool.hip) -> sorted
//                                      keys + order; status bits for a negative coordinate / a coordinate or batch outside the packing /
//                                      a duplicated site
//              pdf_spconv_subm_table   nbr (n, k^3): binary search of every neighbour's key in the sorted keys (the FIRST of equal keys =
//                                      the lowest row, the sort is stable), -1 where no site is
//              pdf_spconv_down         one stride-2 step: parent keys -> stable sort -> run starts -> parent, code, the coarse sites (in
//                                      ascending key order, so their sorted keys are themselves), the children table, and the rows
//                                      bucketed by code in tiles of 128 (perm + the tile's code) for the selected-weight product
//            Every array is sized by the FINE level; the count of a level lives on the device (counts[l]) and every kernel reads it there:
//            the caller reads counts + status once, after all levels are enqueued.
//   products   pdf_spconv_gather       out[r] = bias + sum_k x[tbl[r, k]] W[k] over a (rows, K) table, output-stationary: a workgroup owns
//                                      128 rows x <= 128 columns, wave w the rows [32 w, 32 w + 32), v_mfma_f32_32x32x2_f32 over chunks of
//                                      32 input channels staged in LDS (gathered rows, -1 reads zeros) with the weight chunk; a (tile, k)
//                                      without any neighbour is skipped.  Generic weight strides and an optional mirrored table column
//                                      (K - 1 - k) make it the SubM forward, the SubM input gradient, the strided forward (children table),
//                                      the inverse convolution's input gradient and -- with the bucketed row list and the tile's code as
//                                      the weight tap -- the selected-weight product out[i] = x[parent[i]] W[code[i]].
//              pdf_spconv_small_*      the stem (C_in <= 16, K <= 125, C_out 32 or 64): plain VALU kernels, forward and input gradient
//              pdf_spconv_wgrad        dW[k] = sum_r G[tbl[r, k]]^T D[r]: a workgroup owns (row chunk, k, 32 x <= 128 block), every wave a
//                                      quarter of each 128-row stage and writes its own partial slab; a fixed-order reduction of the slabs follows
//              pdf_spconv_colsum       bias gradient: chunk sums, then the chunks in order
#include "tile_sort.h"

namespace spc {
namespace {

constexpr int TB = 256;
constexpr int TR = 128;                       // rows per tile of the products and of the code buckets
constexpr unsigned long long SENT = ~0ull;
constexpr int ST_NEG = 1, ST_RANGE = 2, ST_DUP = 4;
constexpr int MAXC = 1 << 16, MAXBATCH = 1 << 15;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ unsigned long long pack(int b, int d0, int d1, int d2) {
    return ((unsigned long long)b << 48) | ((unsigned long long)d0 << 32) | ((unsigned long long)d1 << 16) | (unsigned long long)d2;
}

inline unsigned blocks(long total) { return (unsigned)((total + TB - 1) / TB); }

// ---------------------------------------------------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void k_site_keys(long n, const int *__restrict__ idx, unsigned long long *__restrict__ key,
                                                  unsigned *__restrict__ klo, unsigned *__restrict__ khi, unsigned *__restrict__ pay,
                                                  int *__restrict__ status) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int b = idx[i * 4], d0 = idx[i * 4 + 1], d1 = idx[i * 4 + 2], d2 = idx[i * 4 + 3];
    unsigned long long k = SENT;
    if (b < 0 || d0 < 0 || d1 < 0 || d2 < 0) atomicOr(status, ST_NEG);
    else if (b >= MAXBATCH || d0 >= MAXC || d1 >= MAXC || d2 >= MAXC) atomicOr(status, ST_RANGE);
    else k = pack(b, d0, d1, d2);
    key[i] = k;
    klo[i] = (unsigned)(k & 0xffffffffull);
    khi[i] = (unsigned)(k >> 32);
    pay[i] = (unsigned)i;
}

__global__ __launch_bounds__(TB) void k_gather_u32(long n, const unsigned *__restrict__ src, const unsigned *__restrict__ order,
                                                   unsigned *__restrict__ out) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) { const unsigned j = order[i]; out[i] = j < (unsigned long)n ? src[j] : 0u; }
}

__global__ __launch_bounds__(TB) void k_sorted_sites(long n, const unsigned long long *__restrict__ key, const unsigned *__restrict__ order,
                                                     unsigned long long *__restrict__ skey, int *__restrict__ order_out,
                                                     int *__restrict__ status) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const unsigned p = order[i] < (unsigned long)n ? order[i] : 0u;
    const unsigned long long k = key[p];
    skey[i] = k;
    order_out[i] = (int)p;
    if (i > 0 && k != SENT) {
        const unsigned q = order[i - 1] < (unsigned long)n ? order[i - 1] : 0u;
        if (key[q] == k) atomicOr(status, ST_DUP);
    }
}

// first position of `k` among skey[0, cnt), -1 when absent
__device__ __forceinline__ int find_key(const unsigned long long *__restrict__ skey, int cnt, unsigned long long k) {
    int a = 0, z = cnt;
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (skey[mid] < k) a = mid + 1; else z = mid;
    }
    return (a < cnt && skey[a] == k) ? a : -1;
}

__global__ __launch_bounds__(TB) void k_subm_table(long nmax, const int *__restrict__ cnt_p, const int *__restrict__ idx,
                                                   const unsigned long long *__restrict__ skey, const int *__restrict__ order, int ks,
                                                   int *__restrict__ nbr) {
    const int K = ks * ks * ks;
    const long cnt = min((long)cnt_p[0], nmax);
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < cnt * K; t += (long)gridDim.x * TB) {
        const long i = t / K;
        const int k = (int)(t - i * K);
        const int o0 = k / (ks * ks), o1 = (k / ks) % ks, o2 = k % ks, h = ks / 2;
        const int b = idx[i * 4], c0 = idx[i * 4 + 1] + o0 - h, c1 = idx[i * 4 + 2] + o1 - h, c2 = idx[i * 4 + 3] + o2 - h;
        int r = -1;
        if (b >= 0 && b < MAXBATCH && c0 >= 0 && c1 >= 0 && c2 >= 0 && c0 < MAXC && c1 < MAXC && c2 < MAXC) {
            const int p = find_key(skey, (int)cnt, pack(b, c0, c1, c2));
            if (p >= 0) r = order ? order[p] : p;
            if (r < 0 || r >= cnt) r = -1;
        }
        nbr[t] = r;
    }
}

// parent key and code of every fine row; rows past the level's count, rows whose parent lies outside `lim` (when lim[0] > 0) and rows
// whose own coordinates are outside the packing get the sentinel
__global__ __launch_bounds__(TB) void k_parent_keys(long nmax, const int *__restrict__ cnt_p, const int *__restrict__ idx, int l0, int l1, int l2,
                                                    unsigned long long *__restrict__ key, unsigned *__restrict__ klo, unsigned *__restrict__ khi,
                                                    unsigned *__restrict__ pay, int *__restrict__ code, unsigned *__restrict__ ckey) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= nmax) return;
    unsigned long long k = SENT;
    int c = 0;
    if (i < (long)cnt_p[0]) {
        const int b = idx[i * 4], d0 = idx[i * 4 + 1], d1 = idx[i * 4 + 2], d2 = idx[i * 4 + 3];
        const bool ok = b >= 0 && b < MAXBATCH && d0 >= 0 && d1 >= 0 && d2 >= 0 && d0 < MAXC && d1 < MAXC && d2 < MAXC;
        if (ok && !(l0 > 0 && ((d0 >> 1) >= l0 || (d1 >> 1) >= l1 || (d2 >> 1) >= l2))) {
            k = pack(b, d0 >> 1, d1 >> 1, d2 >> 1);
            c = ((d0 & 1) << 2) | ((d1 & 1) << 1) | (d2 & 1);
        }
    }
    key[i] = k;
    klo[i] = (unsigned)(k & 0xffffffffull);
    khi[i] = (unsigned)(k >> 32);
    pay[i] = (unsigned)i;
    code[i] = c;
    ckey[i] = k == SENT ? 8u : (unsigned)c;
}

__device__ __forceinline__ bool starts_run(long i, const unsigned long long *key, const unsigned *order) {
    const unsigned long long k = key[order[i]];
    return k != SENT && (i == 0 || k != key[order[i - 1]]);
}

__global__ __launch_bounds__(TB) void k_flags(long n, const unsigned long long *__restrict__ key, const unsigned *__restrict__ order,
                                              unsigned *__restrict__ flag) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) flag[i] = (order[i] < (unsigned long)n && (i == 0 || order[i - 1] < (unsigned long)n) && starts_run(i, key, order)) ? 1u : 0u;
}

__global__ __launch_bounds__(TB) void k_fill_i32(long n, int v, int *__restrict__ out) {
    for (long i = (long)blockIdx.x * TB + threadIdx.x; i < n; i += (long)gridDim.x * TB) out[i] = v;
}

__global__ __launch_bounds__(TB) void k_assign(long n, const unsigned long long *__restrict__ key, const unsigned *__restrict__ order,
                                               const unsigned *__restrict__ flag, const unsigned *__restrict__ ftot,
                                               const int *__restrict__ code, int *__restrict__ parent, int *__restrict__ cidx,
                                               unsigned long long *__restrict__ cskey, unsigned *__restrict__ children) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const unsigned p = order[i];
    if ((unsigned long)p >= (unsigned long)n) return;   // (never taken)
    const unsigned long long k = key[p];
    if (k == SENT) { parent[p] = -1; return; }
    const bool f = starts_run(i, key, order);
    const unsigned rank = tile_sort::scanned(flag, ftot, (size_t)i) + (f ? 1u : 0u) - 1u;
    if ((unsigned long)rank >= (unsigned long)n) return;   // (never taken)
    parent[p] = (int)rank;
    if (f) {
        cidx[(size_t)rank * 4 + 0] = (int)(k >> 48);
        cidx[(size_t)rank * 4 + 1] = (int)((k >> 32) & 0xffffull);
        cidx[(size_t)rank * 4 + 2] = (int)((k >> 16) & 0xffffull);
        cidx[(size_t)rank * 4 + 3] = (int)(k & 0xffffull);
        cskey[rank] = k;
    }
    atomicMin(children + (size_t)rank * 8 + code[p], p);   // the lowest row of a duplicated site; all-ones (= -1) stays where no child is
}

// ptr[c] = first position of code c among the sorted codes (c = 0..8; ptr[8] = rows that have a parent); astart[c] = start of bucket c
// in the layout where every bucket begins on a tile boundary
__global__ void k_bucket_ptr(long n, const unsigned *__restrict__ scode, int *__restrict__ ptr) {
    const int c = threadIdx.x;
    if (c <= 8) {
        long a = 0, z = n;
        while (a < z) {
            const long mid = (a + z) >> 1;
            if (scode[mid] < (unsigned)c) a = mid + 1; else z = mid;
        }
        ptr[c] = (int)a;
    }
    __syncthreads();
    if (c == 0) {
        int run = 0;
        for (int j = 0; j < 8; ++j) {
            ptr[9 + j] = run;
            run += (ptr[j + 1] - ptr[j] + TR - 1) / TR * TR;
        }
        ptr[17] = run;
    }
}

__global__ __launch_bounds__(TB) void k_bucket_fill(long padded, long n, const unsigned *__restrict__ srow, const int *__restrict__ ptr,
                                                    int *__restrict__ perm, int *__restrict__ tile_code) {
    const long q = (long)blockIdx.x * TB + threadIdx.x;
    if (q >= padded) return;
    int c = -1;
    for (int j = 0; j < 8; ++j) if (q >= ptr[9 + j] && q < ptr[9 + j + 1]) c = j;
    int r = -1;
    if (c >= 0) {
        const long j = q - ptr[9 + c], src = ptr[c] + j;
        if (src < ptr[c + 1] && src < n && srow[src] < (unsigned long)n) r = (int)srow[src];
    }
    perm[q] = r;
    if (q % TR == 0) tile_code[q / TR] = c;
}

__global__ __launch_bounds__(TB) void k_iota(long n, unsigned *__restrict__ out) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i < n) out[i] = (unsigned)i;
}

struct Workspace {
    unsigned long long *key;
    unsigned *k32[2], *khi, *pay[2], *hist, *gtot, *flag, *ftot, *ckey[2], *crow[2];
};

size_t carve(void *base, long n, Workspace &w) {
    PdfCarver cv{static_cast<char *>(base)};
    const size_t nt = (size_t)((n + tile_sort::TILE - 1) / tile_sort::TILE);
    w.key = cv.take<unsigned long long>((size_t)n);
    w.k32[0] = cv.take<unsigned>((size_t)n);
    w.k32[1] = cv.take<unsigned>((size_t)n);
    w.khi = cv.take<unsigned>((size_t)n);
    w.pay[0] = cv.take<unsigned>((size_t)n);
    w.pay[1] = cv.take<unsigned>((size_t)n);
    w.hist = cv.take<unsigned>(nt * tile_sort::RADIX);
    w.gtot = cv.take<unsigned>(tile_sort::chunks(nt * tile_sort::RADIX));
    w.flag = cv.take<unsigned>((size_t)n);
    w.ftot = cv.take<unsigned>(tile_sort::chunks((size_t)n));
    w.ckey[0] = cv.take<unsigned>((size_t)n);
    w.ckey[1] = cv.take<unsigned>((size_t)n);
    w.crow[0] = cv.take<unsigned>((size_t)n);
    w.crow[1] = cv.take<unsigned>((size_t)n);
    return cv.off;
}

// stable order of the 64-bit keys whose halves are in k32[0] / khi and whose payload (the row) is in pay[0]
const unsigned *sort64(long n, Workspace &w, hipStream_t s) {
    int cur = tile_sort::sort<unsigned, true>(n, 1, w.k32, w.pay, w.hist, w.gtot, s);
    unsigned *k2[2] = {w.k32[cur ^ 1], w.k32[cur]};
    unsigned *p2[2] = {w.pay[cur], w.pay[cur ^ 1]};
    k_gather_u32<<<blocks(n), TB, 0, s>>>(n, w.khi, p2[0], k2[0]);
    cur = tile_sort::sort<unsigned, true>(n, 1, k2, p2, w.hist, w.gtot, s);
    return p2[cur];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// gather-convolution on the matrix cores
// ---------------------------------------------------------------------------------------------------------------------------------------
struct GArgs {
    const float *x; long ldx; int cin;
    const int *tbl; int K, mirror;
    const int *perm; const int *tile_k; long rows, xrows;
    const float *w; long w_kk, w_k, w_col;
    const float *bias; float *out; long ldo; int cout; long orows;
};

constexpr int AS = 33;   // row stride of the gathered tile in LDS (floats)
constexpr int KMAX = 27;

template <int NB>
__global__ __launch_bounds__(TB) void k_gconv(GArgs a) {
    constexpr int BS = NB * 32 + 32;   // row stride of the weight chunk
    __shared__ int rowL[TR];
    __shared__ int tblL[TR * KMAX];
    __shared__ int anyk[32];
    __shared__ float As[TR * AS];
    __shared__ float Bs[32 * BS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long tile = blockIdx.x;
    const int col0 = blockIdx.y * NB * 32;
    int wk0 = 0;
    if (a.tile_k) { wk0 = a.tile_k[tile]; if (wk0 < 0 || wk0 >= 8) return; }   // (block-uniform)
    const int K = a.K;
    if (tid < TR) {
        const long r = tile * TR + tid;
        long row = r < a.rows ? (a.perm ? (long)a.perm[r] : r) : -1;
        if (row >= a.orows) row = -1;
        rowL[tid] = (int)row;
    }
    if (tid < 32) anyk[tid] = 0;
    __syncthreads();
    for (int e = tid; e < TR * K; e += TB) {
        const int t = e / K, k = e - t * K;
        const int row = rowL[t];
        int src = -1;
        if (row >= 0) src = a.tbl[(size_t)row * K + (a.mirror ? K - 1 - k : k)];
        if (src < 0 || src >= a.xrows) src = -1;
        tblL[e] = src;
        if (src >= 0) anyk[k] = 1;
    }
    __syncthreads();
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    const int li = lane & 31, lh = lane >> 5;
    for (int k = 0; k < K; ++k) {
        if (!anyk[k]) continue;   // (block-uniform: no row of the tile has this neighbour)
        const int wk = a.tile_k ? wk0 : k;
        for (int c0 = 0; c0 < a.cin; c0 += 32) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = tid + TB * j, t = e >> 3, q = e & 7;
                const int src = tblL[t * K + k];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (src >= 0) v = *reinterpret_cast<const float4 *>(a.x + (size_t)src * a.ldx + c0 + 4 * q);
                float *d = As + t * AS + 4 * q;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            const float *wb = a.w + (size_t)wk * a.w_k + (size_t)c0 * a.w_kk + (size_t)col0 * a.w_col;
            if (a.w_col == 1) {
                for (int e = tid; e < 32 * NB * 32; e += TB) {
                    const int kk = e / (NB * 32), col = e - kk * (NB * 32);
                    Bs[kk * BS + col] = wb[(size_t)kk * a.w_kk + col];
                }
            } else {
                for (int e = tid; e < 32 * NB * 32; e += TB) {
                    const int col = e >> 5, kk = e & 31;
                    Bs[kk * BS + col] = wb[(size_t)kk * a.w_kk + (size_t)col * a.w_col];
                }
            }
            __syncthreads();
            const float *ap = As + (32 * wv + li) * AS + lh;
            const float *bp = Bs + lh * BS + li;
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const float av = ap[2 * s];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * s * BS + nb * 32], acc[nb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = col0 + nb * 32 + li;
        const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int row = rowL[t];
            if (row >= 0) a.out[(size_t)row * a.ldo + col] = acc[nb][r] + bv;
        }
    }
}

template <int NB>
void launch_gconv(const GArgs &a, long tiles, hipStream_t s) {
    k_gconv<NB><<<dim3((unsigned)tiles, (unsigned)(a.cout / (NB * 32))), TB, 0, s>>>(a);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// small C_in (the stem): plain kernels.  Weight element (co, k, ci) at w[(co * K + k) * cin + ci].
// ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int SR = 64;   // rows per workgroup
constexpr int SMALL_CIN = 16, SMALL_COUT = 64;

__global__ __launch_bounds__(TB) void k_small_fwd(long rows, int cin, int cout, int K, const float *__restrict__ x, const int *__restrict__ tbl,
                                                  const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ out) {
    __shared__ float Ws[SMALL_CIN * SMALL_COUT];
    __shared__ int srcL[SR];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * SR;
    const int co = tid % cout, rl = tid / cout, rstep = TB / cout;   // cout divides 256 (32 or 64)
    float acc[SR / 4];   // rstep >= 4
#pragma unroll
    for (int j = 0; j < SR / 4; ++j) acc[j] = 0.f;
    for (int k = 0; k < K; ++k) {
        __syncthreads();
        int any = 0;
        if (tid < SR) {
            const long r = r0 + tid;
            int src = r < rows ? tbl[(size_t)r * K + k] : -1;
            if (src >= rows) src = -1;
            srcL[tid] = src;
            any = src >= 0;
        }
        if (!__syncthreads_or(any)) continue;
        for (int e = tid; e < cin * cout; e += TB) {
            const int c = e / cin, ci = e - c * cin;
            Ws[ci * cout + c] = w[((size_t)c * K + k) * cin + ci];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SR / 4; ++j) {
            const int t = rl + j * rstep;
            if (t < SR) {
                const int src = srcL[t];
                if (src >= 0) {
                    float v = acc[j];
                    for (int ci = 0; ci < cin; ++ci) v = fmaf(x[(size_t)src * cin + ci], Ws[ci * cout + co], v);
                    acc[j] = v;
                }
            }
        }
    }
    const float bv = bias ? bias[co] : 0.f;
#pragma unroll
    for (int j = 0; j < SR / 4; ++j) {
        const int t = rl + j * rstep;
        const long r = r0 + t;
        if (t < SR && r < rows) out[(size_t)r * cout + co] = acc[j] + bv;
    }
}

// dx[j, ci] = sum_k sum_co g[tbl[j, K - 1 - k], co] W[co, k, ci]: one thread per (row, ci)
__global__ __launch_bounds__(TB) void k_small_dgrad(long rows, int cin, int cout, int K, const float *__restrict__ g, const int *__restrict__ tbl,
                                                    const float *__restrict__ w, float *__restrict__ dx) {
    for (long t = (long)blockIdx.x * TB + threadIdx.x; t < rows * cin; t += (long)gridDim.x * TB) {
        const long j = t / cin;
        const int ci = (int)(t - j * cin);
        float v = 0.f;
        for (int k = 0; k < K; ++k) {
            const int src = tbl[(size_t)j * K + (K - 1 - k)];
            if (src < 0 || src >= rows) continue;
            for (int co = 0; co < cout; ++co) v = fmaf(g[(size_t)src * cout + co], w[((size_t)co * K + k) * cin + ci], v);
        }
        dx[t] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------------------------------
struct WArgs {
    const float *G; long ldg; int ca; long grows;   // gathered side (rows of G through the table), ca channels (padded to 32 with zeros)
    const float *D; long ldd; int cb;               // direct side, cb a multiple of 32
    const int *tbl; int K; long rows; long chunk;   // rows of the table; rows per chunk (a multiple of 128)
    float *ws;                                      // slabs [chunks * 4][K][CA][cb], CA = ca rounded up to 32
};

template <int NB>
__global__ __launch_bounds__(TB) void k_wgrad(WArgs a) {
    constexpr int DS = NB * 32 + 32;
    __shared__ float Gs[TR * AS];
    __shared__ __attribute__((aligned(16))) float Ds[TR * DS];
    __shared__ int srcL[TR];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int CA = (a.ca + 31) / 32 * 32, nbs = a.cb / (NB * 32);
    const int k = blockIdx.y, ab = blockIdx.z / nbs, bs = blockIdx.z - ab * nbs;
    const int a0 = ab * 32, b0 = bs * NB * 32;
    const long r_begin = (long)blockIdx.x * a.chunk, r_end = min(a.rows, r_begin + a.chunk);
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    for (long rs = r_begin; rs < r_end; rs += TR) {
        __syncthreads();
        int any = 0;
        if (tid < TR) {
            const long r = rs + tid;
            int src = r < r_end ? a.tbl[(size_t)r * a.K + k] : -1;
            if (src >= a.grows) src = -1;
            srcL[tid] = src;
            any = src >= 0;
        }
        if (!__syncthreads_or(any)) continue;   // (block-uniform)
        for (int e = tid; e < TR * 32; e += TB) {
            const int t = e >> 5, c = e & 31;
            const int src = srcL[t];
            Gs[t * AS + c] = (src >= 0 && a0 + c < a.ca) ? a.G[(size_t)src * a.ldg + a0 + c] : 0.f;
        }
        for (int e = tid; e < TR * NB * 8; e += TB) {
            const int t = e / (NB * 8), q = e - t * (NB * 8);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (srcL[t] >= 0) v = *reinterpret_cast<const float4 *>(a.D + (size_t)(rs + t) * a.ldd + b0 + 4 * q);
            *reinterpret_cast<float4 *>(Ds + t * DS + 4 * q) = v;
        }
        __syncthreads();
        const float *gp = Gs + (32 * wv + lh) * AS + li;
        const float *dp = Ds + (32 * wv + lh) * DS + li;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const float av = gp[2 * s * AS];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, dp[2 * s * DS + nb * 32], acc[nb], 0, 0, 0);
        }
    }
    float *slab = a.ws + (((size_t)blockIdx.x * 4 + wv) * a.K + k) * (size_t)CA * a.cb;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ar = a0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            slab[(size_t)ar * a.cb + b0 + nb * 32 + li] = acc[nb][r];
        }
}

// dW element (co, k, ci) = sum of the slabs' (k, a, b) in slab order; swap = 0: (a, b) = (ci, co); swap = 1: (a, b) = (co, ci)
__global__ __launch_bounds__(TB) void k_wreduce(int nslabs, int K, int ca, int cb, int swap, const float *__restrict__ ws, float *__restrict__ dw) {
    const int CA = (ca + 31) / 32 * 32;
    const long total = (long)K * ca * cb;
    for (long e = (long)blockIdx.x * TB + threadIdx.x; e < total; e += (long)gridDim.x * TB) {
        const int b = (int)(e % cb), ar = (int)((e / cb) % ca), k = (int)(e / ((long)cb * ca));
        const size_t off = ((size_t)k * CA + ar) * cb + b, stride = (size_t)K * CA * cb;
        float v = 0.f;
        for (int s = 0; s < nslabs; ++s) v += ws[s * stride + off];
        const int co = swap ? ar : b, ci = swap ? b : ar, cin = swap ? cb : ca;
        dw[((size_t)co * K + k) * cin + ci] = v;
    }
}

long wgrad_chunks(long rows, int K, int ca, int cb) {
    const long CA = (ca + 31) / 32 * 32;
    const long per = 4 * (long)K * CA * cb;
    long chunks = (rows + 511) / 512;
    const long cap = (16L << 20) / per;
    if (chunks > cap) chunks = cap;
    if (chunks > 64) chunks = 64;
    if (chunks < 1) chunks = 1;
    return chunks;
}

constexpr int CS_CHUNKS = 128;
__global__ __launch_bounds__(TB) void k_colsum_part(long rows, int c, const float *__restrict__ g, float *__restrict__ part) {
    const long per = (rows + CS_CHUNKS - 1) / CS_CHUNKS, r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
    for (int col = threadIdx.x; col < c; col += TB) {
        float v = 0.f;
        for (long r = r0; r < r1; ++r) v += g[(size_t)r * c + col];
        part[(size_t)blockIdx.x * c + col] = v;
    }
}
__global__ __launch_bounds__(TB) void k_colsum_fin(int c, const float *__restrict__ part, float *__restrict__ out) {
    const int col = blockIdx.x * TB + threadIdx.x;
    if (col >= c) return;
    float v = 0.f;
    for (int s = 0; s < CS_CHUNKS; ++s) v += part[(size_t)s * c + col];
    out[col] = v;
}

}  // namespace
}  // namespace spc

// ---------------------------------------------------------------------------------------------------------------------------------------
// entries
// ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" long pdf_spconv_geometry_workspace_bytes(long n) {
    if (n < 1 || n >= (1L << 31) - 2) return 0;
    spc::Workspace w;
    return (long)spc::carve(nullptr, n, w);
}

extern "C" long pdf_spconv_bucket_rows(long n) { return n < 0 ? 0 : (n + spc::TR - 1) / spc::TR * spc::TR + 8 * spc::TR; }

extern "C" int pdf_spconv_sort_sites(long n, const int *indices, unsigned long long *skey, int *order, int *status, void *workspace,
                                     void *stream) {
    if (n < 1 || n >= (1L << 31) - 2 || !indices || !skey || !order || !status || !workspace || ((uintptr_t)workspace % 256))
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    spc::Workspace w;
    spc::carve(workspace, n, w);
    const unsigned nb = spc::blocks(n);
    spc::k_site_keys<<<nb, spc::TB, 0, s>>>(n, indices, w.key, w.k32[0], w.khi, w.pay[0], status);
    const unsigned *ord = spc::sort64(n, w, s);
    spc::k_sorted_sites<<<nb, spc::TB, 0, s>>>(n, w.key, ord, skey, order, status);
    return pdf_launch_status();
}

extern "C" int pdf_spconv_subm_table(long nmax, const int *count, const int *indices, const unsigned long long *skey, const int *order,
                                     int ksize, int *nbr, void *stream) {
    if (nmax < 1 || nmax >= (1L << 31) - 2 || !count || !indices || !skey || !nbr || ksize < 1 || ksize > 5 || !(ksize & 1))
        return PDF_ERR_BAD_ARG;
    const long total = nmax * ksize * ksize * ksize;
    const long b = (total + spc::TB - 1) / spc::TB;
    spc::k_subm_table<<<(unsigned)(b < 64 * PDF_MAX_BLOCKS ? b : 64 * PDF_MAX_BLOCKS), spc::TB, 0, static_cast<hipStream_t>(stream)>>>(
        nmax, count, indices, skey, order, ksize, nbr);
    return pdf_launch_status();
}

// One stride-2 step.  indices (nmax, 4) of which count[0] rows are sites; limit: the coarse spatial shape (3 host ints) or NULL.
// -> parent (nmax), code (nmax), coarse_indices (nmax, 4), coarse_skey (nmax), children (nmax, 8), bucket_perm (pdf_spconv_bucket_rows(nmax)),
// tile_code (that / 128), bucket_ptr (18 ints), count_out[0] = the coarse sites.
extern "C" int pdf_spconv_down(long nmax, const int *count, const int *indices, const int *limit, int *parent, int *code, int *coarse_indices,
                               unsigned long long *coarse_skey, int *children, int *bucket_perm, int *tile_code, int *bucket_ptr,
                               int *count_out, void *workspace, void *stream) {
    if (nmax < 1 || nmax >= (1L << 31) - 2 || !count || !indices || !parent || !code || !coarse_indices || !coarse_skey || !children
        || !bucket_perm || !tile_code || !bucket_ptr || !count_out || !workspace || ((uintptr_t)workspace % 256))
        return PDF_ERR_BAD_ARG;
    if (limit && (limit[0] < 1 || limit[1] < 1 || limit[2] < 1)) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    spc::Workspace w;
    spc::carve(workspace, nmax, w);
    const unsigned nb = spc::blocks(nmax);
    spc::k_parent_keys<<<nb, spc::TB, 0, s>>>(nmax, count, indices, limit ? limit[0] : 0, limit ? limit[1] : 0, limit ? limit[2] : 0, w.key,
                                              w.k32[0], w.khi, w.pay[0], code, w.ckey[0]);
    spc::k_fill_i32<<<spc::blocks(nmax * 8 < 2048L * spc::TB ? nmax * 8 : 2048L * spc::TB), spc::TB, 0, s>>>(nmax * 8, -1, children);
    const unsigned *ord = spc::sort64(nmax, w, s);
    spc::k_flags<<<nb, spc::TB, 0, s>>>(nmax, w.key, ord, w.flag);
    const long fchunks = (long)tile_sort::chunks((size_t)nmax);
    tile_sort::k_ts_scan_chunks<<<(unsigned)fchunks, tile_sort::LB, 0, s>>>(nmax, w.flag, w.ftot);
    tile_sort::k_ts_scan_short<<<1, tile_sort::LB, 0, s>>>((int)fchunks, w.ftot, reinterpret_cast<unsigned *>(count_out));
    spc::k_assign<<<nb, spc::TB, 0, s>>>(nmax, w.key, ord, w.flag, w.ftot, code, parent, coarse_indices, coarse_skey,
                                         reinterpret_cast<unsigned *>(children));
    // rows bucketed by code: a stable sort of (code, row), then every bucket laid out from a tile boundary
    spc::k_iota<<<nb, spc::TB, 0, s>>>(nmax, w.crow[0]);
    const int cur = tile_sort::sort<unsigned, true>(nmax, 1, w.ckey, w.crow, w.hist, w.gtot, s);
    spc::k_bucket_ptr<<<1, 64, 0, s>>>(nmax, w.ckey[cur], bucket_ptr);
    const long padded = pdf_spconv_bucket_rows(nmax);
    spc::k_bucket_fill<<<spc::blocks(padded), spc::TB, 0, s>>>(padded, nmax, w.crow[cur], bucket_ptr, bucket_perm, tile_code);
    return pdf_launch_status();
}

static int spconv_nb(int cols) { return cols % 128 == 0 ? 4 : cols % 96 == 0 ? 3 : cols % 64 == 0 ? 2 : 1; }

/* 1: the matrix-core class, 2: the small-C_in class (the stem), 0: neither. */
extern "C" int pdf_spconv_supported(int k, int cin, int cout) {
    if (k < 1 || k > 5 || cin < 1 || cout < 1) return 0;
    if (cin % 32 == 0 && cout % 32 == 0 && cin <= 384 && cout <= 384 && k <= 3) return 1;
    if (cin <= spc::SMALL_CIN && (cout == 32 || cout == 64)) return 2;
    return 0;
}

extern "C" int pdf_spconv_gather(long rows, long orows, long xrows, int cin, int cout, int K, const float *x, const int *tbl, int mirror,
                                 const int *perm, const int *tile_k, const float *w, long w_kk, long w_k, long w_col, const float *bias,
                                 float *out, void *stream) {
    if (rows == 0 || orows == 0) return PDF_OK;
    if (rows < 0 || orows < 0 || xrows < 1 || !x || !tbl || !w || !out || K < 1 || K > spc::KMAX || (tile_k && (!perm || K != 1))
        || w_kk < 1 || w_k < 0 || w_col < 1 || ((uintptr_t)x % 16))
        return PDF_ERR_BAD_ARG;
    if (cin % 32 || cout % 32 || cin < 32 || cout < 32 || cin > 384 || cout > 384) return PDF_ERR_UNSUPPORTED;
    spc::GArgs a{x, (long)cin, cin, tbl, K, mirror ? 1 : 0, perm, tile_k, rows, xrows, w, w_kk, w_k, w_col, bias, out, (long)cout, cout};
    a.orows = orows;
    const long tiles = (rows + spc::TR - 1) / spc::TR;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (spconv_nb(cout)) {
        case 4: spc::launch_gconv<4>(a, tiles, s); break;
        case 3: spc::launch_gconv<3>(a, tiles, s); break;
        case 2: spc::launch_gconv<2>(a, tiles, s); break;
        default: spc::launch_gconv<1>(a, tiles, s); break;
    }
    return pdf_launch_status();
}

extern "C" int pdf_spconv_small_forward(long rows, int cin, int cout, int K, const float *x, const int *tbl, const float *w,
                                        const float *bias, float *out, void *stream) {
    if (rows == 0) return PDF_OK;
    if (rows < 0 || !x || !tbl || !w || !out || K < 1 || K > 125) return PDF_ERR_BAD_ARG;
    if (cin < 1 || cin > spc::SMALL_CIN || (cout != 32 && cout != 64)) return PDF_ERR_UNSUPPORTED;
    spc::k_small_fwd<<<(unsigned)((rows + spc::SR - 1) / spc::SR), spc::TB, 0, static_cast<hipStream_t>(stream)>>>(rows, cin, cout, K, x, tbl, w,
                                                                                                                  bias, out);
    return pdf_launch_status();
}

extern "C" int pdf_spconv_small_dgrad(long rows, int cin, int cout, int K, const float *g, const int *tbl, const float *w, float *dx,
                                      void *stream) {
    if (rows == 0) return PDF_OK;
    if (rows < 0 || !g || !tbl || !w || !dx || K < 1 || K > 125) return PDF_ERR_BAD_ARG;
    if (cin < 1 || cin > spc::SMALL_CIN || cout < 1) return PDF_ERR_UNSUPPORTED;
    const long b = (rows * cin + spc::TB - 1) / spc::TB;
    spc::k_small_dgrad<<<(unsigned)(b < 8 * PDF_MAX_BLOCKS ? b : 8 * PDF_MAX_BLOCKS), spc::TB, 0, static_cast<hipStream_t>(stream)>>>(
        rows, cin, cout, K, g, tbl, w, dx);
    return pdf_launch_status();
}

extern "C" long pdf_spconv_wgrad_ws_floats(long rows, int K, int ca, int cb) {
    if (rows < 1 || K < 1 || ca < 1 || cb < 1) return 0;
    const long CA = (ca + 31) / 32 * 32;
    return spc::wgrad_chunks(rows, K, ca, cb) * 4 * K * CA * cb;
}

/* dW (co, k, ci) from G (grows, ca) gathered through tbl (rows, K) and D (rows, cb): swap = 0: ca = C_in, cb = C_out; 1: ca = C_out, cb = C_in. */
extern "C" int pdf_spconv_wgrad(long rows, long grows, int K, int ca, int cb, const float *G, const float *D, const int *tbl, int swap,
                                float *ws, float *dw, void *stream) {
    if (rows < 1 || grows < 1 || K < 1 || K > 125 || !G || !D || !tbl || !ws || !dw || ((uintptr_t)D % 16)) return PDF_ERR_BAD_ARG;
    if (ca < 1 || ca > 384 || cb < 32 || cb > 384 || cb % 32) return PDF_ERR_UNSUPPORTED;
    const long chunks = spc::wgrad_chunks(rows, K, ca, cb);
    long chunk = (rows + chunks - 1) / chunks;
    chunk = (chunk + spc::TR - 1) / spc::TR * spc::TR;
    spc::WArgs a{G, (long)ca, ca, grows, D, (long)cb, cb, tbl, K, rows, chunk, ws};
    const int nb = spconv_nb(cb), nA = (ca + 31) / 32;
    const dim3 grid((unsigned)chunks, (unsigned)K, (unsigned)(nA * (cb / (nb * 32))));
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (nb) {
        case 4: spc::k_wgrad<4><<<grid, spc::TB, 0, s>>>(a); break;
        case 3: spc::k_wgrad<3><<<grid, spc::TB, 0, s>>>(a); break;
        case 2: spc::k_wgrad<2><<<grid, spc::TB, 0, s>>>(a); break;
        default: spc::k_wgrad<1><<<grid, spc::TB, 0, s>>>(a); break;
    }
    const long total = (long)K * ca * cb, b = (total + spc::TB - 1) / spc::TB;
    spc::k_wreduce<<<(unsigned)(b < 8 * PDF_MAX_BLOCKS ? b : 8 * PDF_MAX_BLOCKS), spc::TB, 0, s>>>((int)chunks * 4, K, ca, cb, swap ? 1 : 0, ws, dw);
    return pdf_launch_status();
}

extern "C" long pdf_spconv_colsum_ws_floats(int c) { return c < 1 ? 0 : (long)spc::CS_CHUNKS * c; }

extern "C" int pdf_spconv_colsum(long rows, int c, const float *g, float *ws, float *out, void *stream) {
    if (rows < 1 || c < 1 || !g || !ws || !out) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    spc::k_colsum_part<<<spc::CS_CHUNKS, spc::TB, 0, s>>>(rows, c, g, ws);
    spc::k_colsum_fin<<<spc::blocks(c), spc::TB, 0, s>>>(c, ws, out);
    return pdf_launch_status();
}
