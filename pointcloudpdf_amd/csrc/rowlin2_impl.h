// Streaming per-point Linear layers for channel widths 32..512 (second-generation kernels behind pdf_rowlin_*).
//
// The Bottleneck's Linear layers (point_transformer_seg.py:184-192, 45-78: linear1, linear_q/k/v, linear3) are skinny GEMMs:
// N = 10^5..10^3 rows, 32..512 channels, i.e. 16..256 FLOP per byte of activations -- HBM / latency bound, never
// MFMA bound.  The kernels therefore stream the activation rows exactly once and keep the whole weight slab in registers:
//
//   forward / input gradient (k_fwd):  Y_out[n, o] = sum_in sum_k f(X_in[n, k]) Wt_in/out(k, o) + bias[o]
//     one wave = 16 rows per trip; v_mfma_f32_16x16x4_f32 with A = W (rows = output channels) and B = X^T (cols = rows n):
//     lane (n = l & 15, kq = l >> 4) loads float4 X[n][16 j + 4 kq ..+4] (64 contiguous bytes per row and instruction) and
//     ends up with float4 Y[n][o0 + 4 (l >> 4) ..+4]: both sides are 16-byte accesses, no LDS, no barrier.
//     The reduction index is permuted (k = 16 j + 4 kq + c at MFMA step (j, c)), which a dot product does not mind.
//     f = identity or relu(x * scale[k] + shift[k]) (the BatchNorm + ReLU in front of the layer), optional epilogue =
//     per-column sum / sum of squares of Y for the BatchNorm behind it.  Up to three inputs (dX = sum G_i W_i) or three
//     outputs (q, k, v from one read of the activations).
//   weight gradient (k_wg):  dW[o, k] += sum_n G[n, o] f(X[n, k]),  db[o] += sum_n G[n, o]
//     reduction index = rows: lane (i = l & 15, nq = l >> 4) loads VW consecutive channels of row n0 + nq of G and of X;
//     MFMA (c, c') accumulates the 16x16 sub-block {o = VW i + c} x {k = VW j + c'}: VW^2 MFMAs per 4 rows cover a
//     (16 VW)^2 block of dW.  Waves reduce through LDS, every workgroup stores its block into its own SLAB of a caller-owned workspace,
//     and k_slab_reduce sums the slabs of a block in a fixed order (round 3: no float atomics -- bit-reproducible gradients; dW is
//     written, not accumulated).
//
// fp32 in / fp32 accumulate (bit-equal to an fmaf chain): the reference computes these layers in fp32.
//
// Layout: rowlin2.h declares the host interface (the problem structs Forward / Wgrad, RArgs, the try_* prototypes) for rowlin.hip.  This
// header is the implementation -- the kernels, then the host code that turns a described problem into kernel arguments and a launch:
// fwd_args (the one place a FwdArgs is validated and filled), wg_plan + wg_setup (the one place WArgs / RArgs / grid are made, from the
// plan that also sizes the workspace) and the try_*_mp<MP> templates.  It is compiled three times, once per input precision of the
// products (template parameter MP, see Mma below): rowlin2.hip (MP = 0, fp32 operands -- plus the precision-independent helpers,
// RL2_MAIN_TU, the paired products and the one dispatch on `mma_input`), rowlin2_f16.hip (MP = 1), rowlin2_bf16.hip (MP = 2).  Each
// translation unit instantiates its try_forward_mp / try_wgrad_mp / try_wgrad_pair_mp<MP> explicitly, one line each.
#pragma once
#include "rowlin2.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace rl2 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Input precision of the products (template parameter MP of the kernels; `mma_input` of the C entry points, include/pdfops.h):
//   0  fp32 operands, v_mfma_f32_16x16x4_f32 (bit-equal to an fmaf chain) -- the default and the parity path;
//   1  operands rounded to fp16 in registers, v_mfma_f32_16x16x16_f16;   2  the same with bfloat16, v_mfma_f32_16x16x16_bf16.
// Activations, weights and gradients stay fp32 in HBM and the accumulators are fp32: what torch.autocast does to an nn.Linear
// (engines/train.py:340-363, enable_amp) minus the half-precision rounding of the OUTPUT.  The lane layouts coincide: lane (i = l & 15,
// kq = l >> 4) holds reduction indices 4 kq .. 4 kq + 3 of a 16-wide step in both forms, so one 16x16x16 product replaces the four
// 16x16x4 products of a step.
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 b16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
template <int MP> struct Mma;
template <> struct Mma<0> {
    typedef f32x4 frag;
    static __device__ __forceinline__ frag cvt(f32x4 v) { return v; }
};
template <> struct Mma<1> {
    typedef h16x4 frag;
    static __device__ __forceinline__ frag cvt(f32x4 v) { return __builtin_convertvector(v, h16x4); }
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, acc, 0, 0, 0); }
};
template <> struct Mma<2> {
    typedef s16x4 frag;
    static __device__ __forceinline__ frag cvt(f32x4 v) { return __builtin_bit_cast(s16x4, __builtin_convertvector(v, b16x4)); }
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, acc, 0, 0, 0); }
};

struct FwdArgs {
    long N;
    int O;                   // width of ONE output tensor
    const float *X[3]; long ldx;
    const float *W[3]; long wso, wsk;   // Wt(k, o) = W[o * wso + k * wsk]; indexed by input (NIN > 1) or by output
    const float *bias[3];    // per output (nullable)
    const float *scale, *shift; int relu;
    float *Y[3]; long ldy;
    int accumulate;
    float *partial;          // [gridDim.x][2 * O] (ST != 0; single output)
    // ST == 2: the output is the gradient of a BatchNorm(+ReLU) OUTPUT; the partial rows then carry that BatchNorm's backward sums
    // [sum g' | sum g' xhat] (g' = output masked by the ReLU of bx * scale + shift, xhat = (bx - mean) * rstd) instead of [sum | sum of squares]
    const float *bx; long ldb; const float *bcoef; int brelu;   // bx (N, O; row stride ldb), bcoef = [scale | shift | mean | rstd] (4 O)
    const float *roww; long rws;   // optional per-row factor of the product (y = roww[n] * (f(x) Wt) + bias), element stride rws
    // ST == 1, optional: handoff scratch of the CONSUMER's in-kernel BatchNorm finalize (pdfops_common.h: PdfRowsBn) -- zeroed here
    unsigned long long *ho_gran; unsigned *ho_sync;
};

constexpr int FWD_CAP = 1024;   // row-blocks (4 waves each) of the persistent grid
static inline int fwd_row_blocks(long n) {
    const long tiles = (n + 15) / 16, b = (tiles + 3) / 4;
    return (int)(b < 1 ? 1 : (b > FWD_CAP ? FWD_CAP : b));
}

// One workgroup of k_fwd: (bx, by) = its block id in the grid of ITS problem, gdx = that grid's row blocks.  The kernels below hand it
// blockIdx / gridDim (single launch) or the coordinates of one of two problems that share a launch (k_fwd2).
template <int K, int NOB, int NIN, bool PRE, int ST, int MP>   // ST: 0 = no statistics, 1 = [sum | sum of squares] of the output, 2 = BatchNorm-backward sums (FwdArgs); MP: Mma
__device__ __forceinline__ void fwd_block(const FwdArgs &a, const unsigned bx, const unsigned by, const unsigned gdx) {
    typedef typename Mma<MP>::frag wfrag;
    constexpr bool STATS = ST != 0;
    constexpr int NJ = K / 16;
    constexpr bool COEF_REGS = K <= 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    if (ST == 1 && a.ho_gran && bx == 0 && by == 0) pdf_handoff_zero(a.ho_gran, a.O, a.ho_sync);
    const int gcol0 = (int)by * NOB * 16;   // column over the concatenated outputs; a 16-column block never straddles two
    int outi[NOB], colb[NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) { outi[ob] = (gcol0 + ob * 16) / a.O; colb[ob] = gcol0 + ob * 16 - outi[ob] * a.O; }
    wfrag Wr[NIN][NOB][NJ];
#pragma unroll
    for (int in = 0; in < NIN; ++in) {
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            const float *W = a.W[NIN > 1 ? in : outi[ob]];
            const long o = colb[ob] + li;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x4 w4;
                if (a.wsk == 1) {   // (out, in) row-major: four consecutive reduction indices in one 16-byte load
                    w4 = *reinterpret_cast<const f32x4 *>(W + o * a.wso + 16 * j + 4 * kq);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) w4[c] = W[o * a.wso + (long)(16 * j + 4 * kq + c) * a.wsk];
                }
                Wr[in][ob][j] = Mma<MP>::cvt(w4);
            }
        }
    }
    f32x4 bias4[NOB];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob) {
        const float *b = a.bias[NIN > 1 ? 0 : outi[ob]];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[ob][r] = b ? b[colb[ob] + 4 * kq + r] : 0.f;
    }
    f32x4 sc4[COEF_REGS && PRE ? NJ : 1], sh4[COEF_REGS && PRE ? NJ : 1];
    if (PRE && COEF_REGS) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            sc4[j] = *reinterpret_cast<const f32x4 *>(a.scale + 16 * j + 4 * kq);
            sh4[j] = *reinterpret_cast<const f32x4 *>(a.shift + 16 * j + 4 * kq);
        }
    }
    f32x4 s4[STATS ? NOB : 1], ss4[STATS ? NOB : 1];
    if (STATS) {
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) { s4[ob] = f32x4{0.f, 0.f, 0.f, 0.f}; ss4[ob] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
    // ST == 2: the BatchNorm coefficients of this workgroup's columns live in LDS (registers are full of weight fragments: 16 more per
    // column block would halve the occupancy of the three-input K = 256 kernel); rstd is applied once, to the finished sums.
    __shared__ float bco[ST == 2 ? 3 : 1][NOB * 16];   // scale | shift | mean
    if (ST == 2) {
        if (threadIdx.x < 3 * NOB * 16) {
            const int v = threadIdx.x / (NOB * 16), t = threadIdx.x % (NOB * 16);
            bco[ST == 2 ? v : 0][t] = a.bcoef[(long)v * a.O + gcol0 + t];
        }
        __syncthreads();
    }
    // Prologue coefficients of the wide shapes (K > 64) in LDS: read next to the row loads without a trip to L2.
    __shared__ float pco[PRE && !COEF_REGS ? 2 : 1][PRE && !COEF_REGS ? K : 1];
    if (PRE && !COEF_REGS) {
        for (int t = threadIdx.x; t < K; t += 256) { pco[0][t] = a.scale[t]; pco[PRE && !COEF_REGS ? 1 : 0][t] = a.shift[t]; }
        __syncthreads();
    }
    const float relu_lo = a.relu ? 0.f : -INFINITY;   // max(x, lo): no branch between the loads of a trip
    // Row loads of a tile are issued XB at a time ahead of the products that consume them.  Left to the compiler the K = 128 .. 512 shapes
    // compile to load -> s_waitcnt -> 8 products per 16 reduction indices (the weight fragments fill the register file): 16-48 dependent
    // trips to L2 per tile, which is what a level-4 / level-5 launch (one tile per wave) consists of.  XB is what the registers allow
    // next to the weights: the three-input K = 256 kernel holds 192 of them (VGPRs + AGPRs <= 256 keeps two waves per SIMD).
    // (with statistics and several column blocks per wave the accumulators of the sums take the room of half a batch)
    constexpr int XB0 = NJ < 16 ? NJ : 16;
    constexpr int XB = (K == 256 && NIN == 3) ? 4 : ((ST != 0 && NOB > 1 && NIN * NOB * NJ * 4 >= 128) ? ((PRE && K == 128) ? 2 : XB0 / 2) : XB0);
    const long ntiles = (a.N + 15) / 16;
    for (long tile = (long)bx * 4 + wave; tile < ntiles; tile += (long)gdx * 4) {
        const long n = tile * 16 + li;
        const bool valid = n < a.N;
        f32x4 acc[NOB];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int in = 0; in < NIN; ++in) {
            const float *xr = a.X[in] + (valid ? n : 0) * a.ldx + 4 * kq;   // (rows past the end read row 0: a column of the product depends on its own row only)
#pragma unroll
            for (int j0 = 0; j0 < NJ; j0 += XB) {
                f32x4 xb[XB];
#pragma unroll
                for (int t = 0; t < XB; ++t) xb[t] = *reinterpret_cast<const f32x4 *>(xr + 16 * (j0 + t));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < XB; ++t) {
                    const int j = j0 + t;
                    f32x4 x4 = xb[t];
                    if (PRE) {
                        const f32x4 sc = COEF_REGS ? sc4[COEF_REGS ? j : 0] : *reinterpret_cast<const f32x4 *>(&pco[0][16 * j + 4 * kq]);
                        const f32x4 sh = COEF_REGS ? sh4[COEF_REGS ? j : 0] : *reinterpret_cast<const f32x4 *>(&pco[PRE && !COEF_REGS ? 1 : 0][16 * j + 4 * kq]);
                        x4 = x4 * sc + sh;
#pragma unroll
                        for (int c = 0; c < 4; ++c) x4[c] = fmaxf(x4[c], relu_lo);
                    }
                    if constexpr (MP == 0) {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
#pragma unroll
                            for (int ob = 0; ob < NOB; ++ob)
                                acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(Wr[in][ob][j][c], x4[c], acc[ob], 0, 0, 0);
                    } else {
                        const wfrag xh = Mma<MP>::cvt(x4);
#pragma unroll
                        for (int ob = 0; ob < NOB; ++ob) acc[ob] = Mma<MP>::mma(Wr[in][ob][j], xh, acc[ob]);
                    }
                }
            }
        }
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            f32x4 v = acc[ob];
            if (a.roww) v *= a.roww[(valid ? n : 0) * a.rws];
            v += bias4[ob];
            float *dst = a.Y[outi[ob]] + (valid ? n : 0) * a.ldy + colb[ob] + 4 * kq;
            if (a.accumulate && valid) v += *reinterpret_cast<const f32x4 *>(dst);
            if (valid) *reinterpret_cast<f32x4 *>(dst) = v;
            if (ST == 1 && valid) { s4[ob] += v; ss4[ob] += v * v; }
            if (ST == 2) {
                const f32x4 x4 = *reinterpret_cast<const f32x4 *>(a.bx + (valid ? n : 0) * a.ldb + colb[ob] + 4 * kq);
                const f32x4 sc = *reinterpret_cast<const f32x4 *>(&bco[0][ob * 16 + 4 * kq]);
                const f32x4 sh = *reinterpret_cast<const f32x4 *>(&bco[ST == 2 ? 1 : 0][ob * 16 + 4 * kq]);
                const f32x4 mu = *reinterpret_cast<const f32x4 *>(&bco[ST == 2 ? 2 : 0][ob * 16 + 4 * kq]);
                const f32x4 pre = x4 * sc + sh;
                f32x4 gm;
#pragma unroll
                for (int c = 0; c < 4; ++c) gm[c] = (valid && (!a.brelu || pre[c] > 0.f)) ? v[c] : 0.f;
                s4[ob] += gm;
                ss4[ob] += gm * (x4 - mu);
            }
        }
    }
    if (STATS) {
        __shared__ float red[4][2][NOB * 16];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = s4[ob][r], ss = ss4[ob][r];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) { s += __shfl_xor(s, m, 64); ss += __shfl_xor(ss, m, 64); }
                if (li == 0) { red[wave][0][ob * 16 + 4 * kq + r] = s; red[wave][1][ob * 16 + 4 * kq + r] = ss; }
            }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < NOB * 16) {
            float *row = a.partial + (size_t)bx * 2 * a.O;
            row[gcol0 + t] = red[0][0][t] + red[1][0][t] + red[2][0][t] + red[3][0][t];      // STATS: single output, gcol0 == column
            const float ss = red[0][1][t] + red[1][1][t] + red[2][1][t] + red[3][1][t];
            row[a.O + gcol0 + t] = ST == 2 ? ss * a.bcoef[3 * (long)a.O + gcol0 + t] : ss;
        }
    }
}
template <int K, int NOB, int NIN, bool PRE, int ST, int MP>
__global__ __launch_bounds__(256) void k_fwd(FwdArgs a) {
    fwd_block<K, NOB, NIN, PRE, ST, MP>(a, blockIdx.x, blockIdx.y, gridDim.x);
}

// The group form of k_fwd, for launches with few row tiles and many column blocks (levels 3-5: the three-output q / k / v product, the
// three-input dX = sum G_i W_i, the c x c products with statistics).  Same row blocks, same tile-to-wave assignment, same products in the
// same order per output element (input, j, c: one accumulator chain) and the same epilogue as k_fwd -- bit-identical results and partial
// rows -- but a workgroup owns GN 16-column blocks instead of one slab of NOB:
//   - their weight fragments sit in LDS (dynamic, NIN x GN x K x 16 operands), filled once per workgroup by all four waves, instead of
//     once per wave in registers.  The image is in fragment order, [input][block][j][lane]: lane l of the read for (block, j) takes the
//     16 bytes at l, so a ds_read_b128 is contiguous over the wave (conflict-free without padding) and yields the A operands of the four
//     products of one step.  Reduced-precision operands are rounded once, at the fill (8 bytes per lane and step);
//   - a wave reads its row tile once per GN blocks and applies the prologue once: GN accumulators are live, the inputs are walked
//     outermost, rows arrive in double-buffered batches of XB steps.
// Nothing passes between waves through LDS except the fill (one barrier before the first tile) and the statistics sums (as in k_fwd).
//
// GROUP_GN, the 16-column blocks per workgroup.  Measured at 12,496 x 128, 3,124 x 256 and 780 x 512 (profiles/rowlin_group_probe.txt): two blocks beat four on
// every launch -- 16 / 32 / 64 KB of fp32 fragments per input leave several workgroups per CU, and the grid keeps twice the waves.
constexpr int GROUP_GN = 2;
template <int K, int GN, int NIN, int MP> constexpr int group_lds_bytes() { return NIN * GN * (K / 16) * 64 * (int)sizeof(typename Mma<MP>::frag); }

template <int K, int GN, int NIN, bool PRE, int ST, int MP>
__device__ __forceinline__ void fwd_group_block(const FwdArgs &a, const unsigned bx, const unsigned by, const unsigned gdx) {   // (block coordinates: as fwd_block)
    typedef typename Mma<MP>::frag wfrag;
    constexpr bool STATS = ST != 0;
    constexpr int NJ = K / 16;
    static_assert(K >= 128 && NJ % 8 == 0 && (NIN == 1 || NIN == 3), "group form: K = 128 / 256 / 512, one or three inputs");
    extern __shared__ __attribute__((aligned(16))) unsigned char group_lds[];
    wfrag *Wl = reinterpret_cast<wfrag *>(group_lds);   // [NIN][GN][NJ][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    if (ST == 1 && a.ho_gran && bx == 0 && by == 0) pdf_handoff_zero(a.ho_gran, a.O, a.ho_sync);
    const int gcol0 = (int)by * GN * 16;
    int outi[GN], colb[GN];
#pragma unroll
    for (int ob = 0; ob < GN; ++ob) { outi[ob] = (gcol0 + ob * 16) / a.O; colb[ob] = gcol0 + ob * 16 - outi[ob] * a.O; }
    {   // fill: fragment f = (input, block, j) goes to wave f & 3; all of a wave's global loads are in flight before its first LDS store
        constexpr int PER_WAVE = NIN * GN * NJ / 4;   // 4 .. 24 fragments, one float4 per lane each
        f32x4 w4[PER_WAVE];
#pragma unroll
        for (int t = 0; t < PER_WAVE; ++t) {
            const int f = t * 4 + wave;
            const int j = f % NJ, ob = (f / NJ) % GN, in = f / (NJ * GN);
            const int col = gcol0 + ob * 16, oi = col / a.O;
            const float *W = a.W[NIN > 1 ? in : oi];
            const long o = col - oi * a.O + li;
            if (a.wsk == 1) {
                w4[t] = *reinterpret_cast<const f32x4 *>(W + o * a.wso + 16 * j + 4 * kq);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) w4[t][c] = W[o * a.wso + (long)(16 * j + 4 * kq + c) * a.wsk];
            }
        }
#pragma unroll
        for (int t = 0; t < PER_WAVE; ++t) Wl[(t * 4 + wave) * 64 + lane] = Mma<MP>::cvt(w4[t]);
    }
    __shared__ float bco[ST == 2 ? 3 : 1][GN * 16];   // scale | shift | mean of this workgroup's columns (ST == 2)
    if (ST == 2 && threadIdx.x < 3 * GN * 16) {
        const int v = threadIdx.x / (GN * 16), t = threadIdx.x % (GN * 16);
        bco[ST == 2 ? v : 0][t] = a.bcoef[(long)v * a.O + gcol0 + t];
    }
    __shared__ float pco[PRE ? 2 : 1][PRE ? K : 1];
    if (PRE)
        for (int t = threadIdx.x; t < K; t += 256) { pco[0][t] = a.scale[t]; pco[PRE ? 1 : 0][t] = a.shift[t]; }
    __syncthreads();   // the weight image, bco and pco are complete before any wave's first tile
    f32x4 s4[STATS ? GN : 1], ss4[STATS ? GN : 1];
    if (STATS) {
#pragma unroll
        for (int ob = 0; ob < GN; ++ob) { s4[ob] = f32x4{0.f, 0.f, 0.f, 0.f}; ss4[ob] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
    const float relu_lo = a.relu ? 0.f : -INFINITY;
    constexpr int XB = 8, NBJ = NJ / XB, NB = NIN * NBJ;   // batches of XB steps; batch b + 1 is in flight while batch b is multiplied
    const long ntiles = (a.N + 15) / 16;
    for (long tile = (long)bx * 4 + wave; tile < ntiles; tile += (long)gdx * 4) {
        const long n = tile * 16 + li;
        const bool valid = n < a.N;
        const long row = valid ? n : 0;   // (rows past the end read row 0 and never store)
        f32x4 acc[GN];
#pragma unroll
        for (int ob = 0; ob < GN; ++ob) acc[ob] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 xb[2][XB];
#pragma unroll
        for (int t = 0; t < XB; ++t) xb[0][t] = *reinterpret_cast<const f32x4 *>(a.X[0] + row * a.ldx + 4 * kq + 16 * t);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) {
                const float *xr = a.X[(b + 1) / NBJ] + row * a.ldx + 4 * kq + 16 * ((b + 1) % NBJ) * XB;
#pragma unroll
                for (int t = 0; t < XB; ++t) xb[(b + 1) & 1][t] = *reinterpret_cast<const f32x4 *>(xr + 16 * t);
            }
            __builtin_amdgcn_sched_barrier(0);
            const int in = b / NBJ;
#pragma unroll
            for (int t = 0; t < XB; ++t) {
                const int j = (b % NBJ) * XB + t;
                f32x4 x4 = xb[b & 1][t];
                if (PRE) {
                    const f32x4 sc = *reinterpret_cast<const f32x4 *>(&pco[0][16 * j + 4 * kq]);
                    const f32x4 sh = *reinterpret_cast<const f32x4 *>(&pco[PRE ? 1 : 0][16 * j + 4 * kq]);
                    x4 = x4 * sc + sh;
#pragma unroll
                    for (int c = 0; c < 4; ++c) x4[c] = fmaxf(x4[c], relu_lo);
                }
                wfrag wa[GN];
#pragma unroll
                for (int ob = 0; ob < GN; ++ob) wa[ob] = Wl[((in * GN + ob) * NJ + j) * 64 + lane];
                if constexpr (MP == 0) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int ob = 0; ob < GN; ++ob)
                            acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ob][c], x4[c], acc[ob], 0, 0, 0);
                } else {
                    const wfrag xh = Mma<MP>::cvt(x4);
#pragma unroll
                    for (int ob = 0; ob < GN; ++ob) acc[ob] = Mma<MP>::mma(wa[ob], xh, acc[ob]);
                }
            }
        }
#pragma unroll
        for (int ob = 0; ob < GN; ++ob) {
            f32x4 v = acc[ob];
            if (a.roww) v *= a.roww[row * a.rws];
            const float *bp = a.bias[NIN > 1 ? 0 : outi[ob]];
            f32x4 bias4;
#pragma unroll
            for (int r = 0; r < 4; ++r) bias4[r] = bp ? bp[colb[ob] + 4 * kq + r] : 0.f;
            v += bias4;
            float *dst = a.Y[outi[ob]] + row * a.ldy + colb[ob] + 4 * kq;
            if (a.accumulate && valid) v += *reinterpret_cast<const f32x4 *>(dst);
            if (valid) *reinterpret_cast<f32x4 *>(dst) = v;
            if (ST == 1 && valid) { s4[ob] += v; ss4[ob] += v * v; }
            if (ST == 2) {
                const f32x4 x4 = *reinterpret_cast<const f32x4 *>(a.bx + row * a.ldb + colb[ob] + 4 * kq);
                const f32x4 sc = *reinterpret_cast<const f32x4 *>(&bco[0][ob * 16 + 4 * kq]);
                const f32x4 sh = *reinterpret_cast<const f32x4 *>(&bco[ST == 2 ? 1 : 0][ob * 16 + 4 * kq]);
                const f32x4 mu = *reinterpret_cast<const f32x4 *>(&bco[ST == 2 ? 2 : 0][ob * 16 + 4 * kq]);
                const f32x4 pre = x4 * sc + sh;
                f32x4 gm;
#pragma unroll
                for (int c = 0; c < 4; ++c) gm[c] = (valid && (!a.brelu || pre[c] > 0.f)) ? v[c] : 0.f;
                s4[ob] += gm;
                ss4[ob] += gm * (x4 - mu);
            }
        }
    }
    if (STATS) {
        __shared__ float red[4][2][GN * 16];
#pragma unroll
        for (int ob = 0; ob < GN; ++ob)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = s4[ob][r], ss = ss4[ob][r];
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) { s += __shfl_xor(s, m, 64); ss += __shfl_xor(ss, m, 64); }
                if (li == 0) { red[wave][0][ob * 16 + 4 * kq + r] = s; red[wave][1][ob * 16 + 4 * kq + r] = ss; }
            }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < GN * 16) {
            float *prow = a.partial + (size_t)bx * 2 * a.O;
            prow[gcol0 + t] = red[0][0][t] + red[1][0][t] + red[2][0][t] + red[3][0][t];
            const float ss = red[0][1][t] + red[1][1][t] + red[2][1][t] + red[3][1][t];
            prow[a.O + gcol0 + t] = ST == 2 ? ss * a.bcoef[3 * (long)a.O + gcol0 + t] : ss;
        }
    }
}
template <int K, int GN, int NIN, bool PRE, int ST, int MP>
__global__ __launch_bounds__(256, 2) void k_fwd_group(FwdArgs a) {   // (at least two waves per SIMD: the images of 16-96 KB leave room for two workgroups per CU)
    fwd_group_block<K, GN, NIN, PRE, ST, MP>(a, blockIdx.x, blockIdx.y, gridDim.x);
}

// Two plain products (one input, one output, no prologue, no statistics) of ONE reduction width in one launch: the input gradients
// gz_1 W_1 and gz_2 W_2 of a TransitionUp join reduce over the same o and differ in rows, output width and pointers only.  Workgroups
// below `split` are problem 0's grid (x fastest, as the hardware numbers a two-dimensional grid), the rest problem 1's; each runs
// fwd_block / fwd_group_block with the coordinates and the extent of its own grid.
struct FwdArgs2 { FwdArgs a[2]; unsigned gx[2], split; };
template <int K, int NOB, int MP>
__global__ __launch_bounds__(256) void k_fwd2(FwdArgs2 q) {
    const int i = blockIdx.x >= q.split ? 1 : 0;
    const unsigned b = blockIdx.x - (i ? q.split : 0u), gx = q.gx[i];
    fwd_block<K, NOB, 1, false, 0, MP>(q.a[i], b % gx, b / gx, gx);
}
template <int K, int GN, int MP>
__global__ __launch_bounds__(256, 2) void k_fwd_group2(FwdArgs2 q) {
    const int i = blockIdx.x >= q.split ? 1 : 0;
    const unsigned b = blockIdx.x - (i ? q.split : 0u), gx = q.gx[i];
    fwd_group_block<K, GN, 1, false, 0, MP>(q.a[i], b % gx, b / gx, gx);
}

// Two products with the statistics epilogue (one input, one output, bias, no prologue) of DIFFERENT reduction widths in one launch: the
// two Linear layers in front of a TransitionUp join's norms, x1 W1^T (K0) and x2 W2^T (K1).  Each problem runs the body of its own single
// launch -- slab form with NB column blocks per wave, or group form with NB blocks per workgroup -- over its own grid, problem 0's
// workgroups first (x fastest); the partial rows are indexed by each problem's own row block.  The branch is uniform per workgroup and
// every barrier stays inside one body.  Dynamic LDS: the larger weight image of the group-form problems.
template <int K, int NB, bool GROUP, int MP>
__device__ __forceinline__ void fwd_stats_block(const FwdArgs &a, unsigned bx, unsigned by, unsigned gdx) {
    if constexpr (GROUP) fwd_group_block<K, NB, 1, false, 1, MP>(a, bx, by, gdx);
    else fwd_block<K, NB, 1, false, 1, MP>(a, bx, by, gdx);
}
template <int K0, int NB0, bool G0, int K1, int NB1, bool G1, int MP>
__global__ __launch_bounds__(256, (G0 || G1) ? 2 : 1) void k_fwd_stats2(FwdArgs2 q) {
    if (blockIdx.x < q.split) {
        fwd_stats_block<K0, NB0, G0, MP>(q.a[0], blockIdx.x % q.gx[0], blockIdx.x / q.gx[0], q.gx[0]);
    } else {
        const unsigned b = blockIdx.x - q.split;
        fwd_stats_block<K1, NB1, G1, MP>(q.a[1], b % q.gx[1], b / q.gx[1], q.gx[1]);
    }
}

struct WArgs {
    long N;
    int K, O;
    const float *G[WG_MAXG]; long ldg;
    const float *X; long ldx;
    const float *scale, *shift; int relu;
    // per-matrix inputs (per_z != 0; kernels instantiated with PRE = true): its own X and, where scalez[z] is non-null, its own folded
    // BatchNorm + ReLU prologue (a null scalez[z] runs the prologue with scale 1, shift 0, no ReLU: x * 1 + 0 is x)
    int per_z; const float *Xz[WG_MAXG]; const float *scalez[WG_MAXG], *shiftz[WG_MAXG]; int reluz[WG_MAXG];
    float *dW[WG_MAXG], *db[WG_MAXG];
    long rows_per_block;     // multiple of 64
    const float *roww; long rws;   // optional per-row weight of G (dW = sum_n roww[n] G[n]^T f(X[n]))
    float *slab;             // [gridDim.z][gridDim.y][gridDim.x][(16 VW)^2]: one block of dW per workgroup
    float *bslab;            // [gridDim.z][O / (16 VW)][gridDim.x][16 VW]: the workgroup's column sums of G (bias gradient), k-block 0 only
};

template <int VW> struct Vec;
template <> struct Vec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Vec<4> { typedef float type __attribute__((ext_vector_type(4))); };

// One workgroup of k_wg: (bx, by, bz) = its block id in the grid of ITS problem, (gdx, gdy) = that grid's extents (block coordinates: as fwd_block).
// red [4][(16 VW)^2] and redb [4][16 VW] are the workgroup's LDS (wg_lds_floats<VW>() floats, redb behind red): one (16 VW)^2 block per
// wave -- plain stores, then a 4-way sum (LDS atomics cost 20 us here).  The caller owns them: a single launch passes static arrays, a
// launch shared with a product that keeps a weight image in dynamic LDS passes that image's bytes (the larger of the two sizes, not the sum).
template <int VW> constexpr int wg_lds_floats() { return 4 * (16 * VW) * (16 * VW) + 4 * (16 * VW); }
template <int VW, bool PRE, bool RW, int MP>   // RW: per-row weight of G (a.roww); MP: Mma
__device__ __forceinline__ void wg_block(const WArgs &a, const unsigned bx, const unsigned by, const unsigned bz, const unsigned gdx, const unsigned gdy,
                                         float *red, float *redb) {
    typedef typename Vec<VW>::type vec;
    constexpr int B = 16 * VW;   // block edge of dW
    constexpr int BB = B * B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, nq = lane >> 4;
    const int nkb = a.K / B;
    const int ob = ((int)by / nkb) * B, kb = ((int)by % nkb) * B;
    const float *G = a.G[bz];
    const float *X = (PRE && a.per_z) ? a.Xz[bz] : a.X;
    vec sc, sh;
    bool relu = a.relu != 0;
    if (PRE) {
        const float *scp = a.per_z ? a.scalez[bz] : a.scale, *shp = a.per_z ? a.shiftz[bz] : a.shift;
        if (a.per_z) relu = scp != nullptr && a.reluz[bz] != 0;
        if (scp) {   // (uniform per workgroup)
            sc = *reinterpret_cast<const vec *>(scp + kb + VW * li);
            sh = *reinterpret_cast<const vec *>(shp + kb + VW * li);
        } else {
#pragma unroll
            for (int c = 0; c < VW; ++c) { sc[c] = 1.f; sh[c] = 0.f; }
        }
    }
    const float relu_lo = relu ? 0.f : -INFINITY;
    f32x4 acc[VW][VW];
    float gsum[VW];
#pragma unroll
    for (int c = 0; c < VW; ++c) {
        gsum[c] = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < VW; ++c2) acc[c][c2] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const long rb = (long)bx * a.rows_per_block;
    const long re = rb + a.rows_per_block < a.N ? rb + a.rows_per_block : a.N;
    for (long r0 = rb + 16 * wave; r0 < re; r0 += 64) {
        // the eight (twelve) loads of a trip first, nothing conditional between them: with the row weight behind `if (a.roww)` and the
        // ReLU behind `if (a.relu)` the trip compiled to four dependent (g, x) round trips (k_wg<4, true>: 22.7 -> 17.7 us, <4, false>:
        // 14.9 -> 12.2 us per launch over a step).  (Issuing the next trip's loads ahead of this trip's products: the compiler merges the
        // two trips into one of 16 loads, 208 + 88 registers, one wave per SIMD.)
        vec gv[4], xv[4];
        float rw[RW ? 4 : 1];
        bool ok[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const long n = r0 + 4 * t + nq;
            ok[t] = n < re;
            const long nn = ok[t] ? n : rb;
            gv[t] = *reinterpret_cast<const vec *>(G + nn * a.ldg + ob + VW * li);
            xv[t] = *reinterpret_cast<const vec *>(X + nn * a.ldx + kb + VW * li);
            if (RW) rw[RW ? t : 0] = a.roww[nn * a.rws];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (RW) gv[t] *= rw[RW ? t : 0];
            if (PRE) {
                xv[t] = xv[t] * sc + sh;
#pragma unroll
                for (int c = 0; c < VW; ++c) xv[t][c] = fmaxf(xv[t][c], relu_lo);
            }
#pragma unroll
            for (int c = 0; c < VW; ++c) { gv[t][c] = ok[t] ? gv[t][c] : 0.f; xv[t][c] = ok[t] ? xv[t][c] : 0.f; }
        }
        if constexpr (MP == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int c = 0; c < VW; ++c) {
                    gsum[c] += gv[t][c];
#pragma unroll
                    for (int c2 = 0; c2 < VW; ++c2)
                        acc[c][c2] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[t][c], xv[t][c2], acc[c][c2], 0, 0, 0);
                }
        } else {   // reduction index of the 16x16x16 product = 4 nq + t  <->  row r0 + 4 t + nq (the same bijection on both operands)
            typename Mma<MP>::frag ga[VW], xa[VW];
#pragma unroll
            for (int c = 0; c < VW; ++c) {
                gsum[c] += (gv[0][c] + gv[1][c]) + (gv[2][c] + gv[3][c]);
                ga[c] = Mma<MP>::cvt(f32x4{gv[0][c], gv[1][c], gv[2][c], gv[3][c]});
                xa[c] = Mma<MP>::cvt(f32x4{xv[0][c], xv[1][c], xv[2][c], xv[3][c]});
            }
#pragma unroll
            for (int c = 0; c < VW; ++c)
#pragma unroll
                for (int c2 = 0; c2 < VW; ++c2) acc[c][c2] = Mma<MP>::mma(ga[c], xa[c2], acc[c][c2]);
        }
    }
    // D layout: acc[c][c2][r] = dW[ob + VW (4 nq + r) + c][kb + VW li + c2]
#pragma unroll
    for (int c = 0; c < VW; ++c)
#pragma unroll
        for (int c2 = 0; c2 < VW; ++c2)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave * BB + (VW * (4 * nq + r) + c) * B + VW * li + c2] = acc[c][c2][r];
    float *db = a.db[bz];
    const bool want_db = db && kb == 0;
    if (want_db) {
#pragma unroll
        for (int c = 0; c < VW; ++c) {
            float g = gsum[c];
            g += __shfl_xor(g, 16, 64);
            g += __shfl_xor(g, 32, 64);
            if (nq == 0) redb[wave * B + VW * li + c] = g;
        }
    }
    __syncthreads();
    float *slab = a.slab + (((size_t)bz * gdy + by) * gdx + bx) * (B * B);
    for (int e = threadIdx.x; e < BB; e += 256) slab[e] = (red[e] + red[BB + e]) + (red[2 * BB + e] + red[3 * BB + e]);
    if (want_db && threadIdx.x < B)
        a.bslab[(((size_t)bz * (a.O / B) + ob / B) * gdx + bx) * B + threadIdx.x] =
            (redb[threadIdx.x] + redb[B + threadIdx.x]) + (redb[2 * B + threadIdx.x] + redb[3 * B + threadIdx.x]);
}
template <int VW, bool PRE, bool RW, int MP>
__global__ __launch_bounds__(256) void k_wg(WArgs a) {
    __shared__ float red[wg_lds_floats<VW>()];
    wg_block<VW, PRE, RW, MP>(a, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y, red, red + 4 * (16 * VW) * (16 * VW));
}
// Two single-gradient products without prologue or row weight in one launch (the two weight gradients of a TransitionUp join): each
// problem with its own K, O, row split and workspace; workgroups below `split` are problem 0's grid (x fastest), the rest problem 1's.
struct WArgs2 { WArgs a[2]; unsigned gx[2], gy[2], split; };
template <int VW, int MP>
__global__ __launch_bounds__(256) void k_wg2(WArgs2 q) {
    const int i = blockIdx.x >= q.split ? 1 : 0;
    const unsigned b = blockIdx.x - (i ? q.split : 0u), gx = q.gx[i];
    __shared__ float red[wg_lds_floats<VW>()];
    wg_block<VW, false, false, MP>(q.a[i], b % gx, b / gx, 0u, gx, q.gy[i], red, red + 4 * (16 * VW) * (16 * VW));
}
// The same with a vector width per problem and a row weight on problem 0 (the two Gram products of a TransitionDown forward:
// x^T diag(cnt) x, cin wide, and [R | cnt]^T x, 32 wide).  One LDS block, the larger of the two bodies'.
template <int VW0, int VW1, int MP>
__global__ __launch_bounds__(256) void k_wg2_roww(WArgs2 q) {
    __shared__ float red[wg_lds_floats<(VW0 > VW1 ? VW0 : VW1)>()];
    if (blockIdx.x < q.split) {
        const unsigned gx = q.gx[0];
        wg_block<VW0, false, true, MP>(q.a[0], blockIdx.x % gx, blockIdx.x / gx, 0u, gx, q.gy[0], red, red + 4 * (16 * VW0) * (16 * VW0));
    } else {
        const unsigned b = blockIdx.x - q.split, gx = q.gx[1];
        wg_block<VW1, false, false, MP>(q.a[1], b % gx, b / gx, 0u, gx, q.gy[1], red, red + 4 * (16 * VW1) * (16 * VW1));
    }
}

// The grouped weight gradients of a Bottleneck (per-gradient inputs with prologue: k_wg<VW, true, false>) and ONE plain product (one input,
// one output, no prologue, no statistics: the block's gx += dy W1) in one launch.  The two are independent: the product reads dy and W1
// and reads / writes gx, the gradients read their inputs and write only the slab workspace.  Workgroups below `split` are the gradients'
// grid, flattened x fastest, then y, then z -- the longer problem first -- and the rest are the product's grid (x fastest); each runs the
// body of its single launch over the grid of its single launch: the same slabs and the same product bits.  The LDS of both bodies is ONE
// dynamic block sized as the larger of the two (wg_block's four dW blocks, the group form's weight image): added together, 66.5 KB + the
// image would leave one workgroup per CU.
struct WgFwdArgs { WArgs w; FwdArgs f; unsigned wgx, wgy, split, fgx; };
// Waves per SIMD asked of the compiler: the group forms as k_fwd_group; the slab forms what keeps the launch within the registers of the
// wider of its two single kernels.  Left alone (one wave per SIMD allowed) the compiler takes the larger VGPR count of one body plus the
// larger AGPR count of the other: 52 + 16 at K = 32 against k_fwd<32, 2>'s 50 + 12 and k_wg<2, true, false>'s 39 + 16, 120 + 88 at K = 64
// against k_fwd<64, 4>'s 118 + 24 and k_wg<4, true, false>'s 84 + 88.  With the bounds below: 58 and 134 registers, no AGPRs, no scratch
// (the group forms: 123 / 123 / 128; the table of every instantiation: profiles/paired_block_bench.json).
template <int K, bool GROUP> constexpr int wg_fwd_min_waves() { return GROUP ? 2 : (K == 32 ? 8 : 3); }
template <int VW, int K, int NB, bool GROUP, int MINW = wg_fwd_min_waves<K, GROUP>()>   // NB: 16-column blocks per wave (slab form) or per workgroup (group form)
__global__ __launch_bounds__(256, MINW) void k_wg_fwd(WgFwdArgs q) {
    if (blockIdx.x < q.split) {
        extern __shared__ __attribute__((aligned(16))) unsigned char wg_lds[];
        float *red = reinterpret_cast<float *>(wg_lds);
        const unsigned b = blockIdx.x, plane = q.wgx * q.wgy;
        wg_block<VW, true, false, 0>(q.w, b % q.wgx, (b % plane) / q.wgx, b / plane, q.wgx, q.wgy, red, red + 4 * (16 * VW) * (16 * VW));
    } else {
        const unsigned b = blockIdx.x - q.split;
        if constexpr (GROUP) fwd_group_block<K, NB, 1, false, 0, 0>(q.f, b % q.fgx, b / q.fgx, q.fgx);
        else fwd_block<K, NB, 1, false, 0, 0>(q.f, b % q.fgx, b / q.fgx, q.fgx);
    }
}
template <int VW, int K, int NB, bool GROUP> constexpr int wg_fwd_lds_bytes() {
    constexpr int w = wg_lds_floats<VW>() * (int)sizeof(float), g = GROUP ? group_lds_bytes<K, NB, 1, 0>() : 0;
    return w > g ? w : g;
}

// The slab reduction (RArgs and its order of summation: rowlin2.h).
// One workgroup of the reduction: (bx, by, z) = its block id in the grid of ITS problem; lanes 64 L and above of a wider workgroup (the
// two-problem launch, whose problems may differ in L) only take part in the barrier.
template <int L, bool WIDE>
__device__ __forceinline__ void slab_reduce_block(const RArgs &a, int bx, int by, int z, float (*red)[64]) {
    const int e = threadIdx.x & 63, l = threadIdx.x >> 6;
    const int ei = bx * 64 + e;
    const bool bias = by >= a.tiles;
    const int t = bias ? by - a.tiles : by;
    const int len = bias ? a.B : a.B * a.B;
    if (bias && bx * 64 >= len) return;   // (uniform per block)
    const float *src = bias ? a.bslab + ((size_t)z * a.otiles + t) * a.split * a.B : a.slab + ((size_t)z * a.tiles + t) * a.split * (size_t)(a.B * a.B);
    float s = 0.f;
    if (ei < len && (!WIDE || l < L)) {
        int k = l;
        for (; k + 3 * L < a.split; k += 4 * L) {   // four loads in flight per lane
            const float v0 = src[(size_t)k * len + ei], v1 = src[(size_t)(k + L) * len + ei];
            const float v2 = src[(size_t)(k + 2 * L) * len + ei], v3 = src[(size_t)(k + 3 * L) * len + ei];
            s = (((s + v0) + v1) + v2) + v3;
        }
        for (; k < a.split; k += L) s += src[(size_t)k * len + ei];
    }
    red[l][e] = s;
    __syncthreads();
    if (l != 0 || ei >= len) return;
#pragma unroll
    for (int k = 1; k < L; ++k) s += red[k][e];
    if (bias) {
        const int o = t * a.B + ei;
        if (a.db[z] && o < a.O) a.db[z][o] = s;
    } else {
        const int o = (t / a.tiles_k) * a.B + ei / a.B, kk = (t % a.tiles_k) * a.B + ei % a.B;
        if (o < a.O && kk < a.K) a.dW[z][(size_t)o * a.K + kk] = s;
    }
}
template <int L>
__global__ __launch_bounds__(64 * L) void k_slab_reduce(RArgs a) {
    __shared__ float red[L][64];
    slab_reduce_block<L, false>(a, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, red);
}
static inline int slab_reduce_lanes(int split) { return split > 32 ? 16 : (split > 4 ? 4 : 1); }   // L of a reduction over `split` slabs

// Two single-gradient reductions in ONE launch: grid rows below `ysplit` are problem 0's grid, the rest problem 1's.  Each problem is
// summed with the L (and so the order) of its own launch; the workgroup is as wide as the larger L needs.
struct RArgs2 { RArgs a[2]; int L[2], gx[2], ysplit; };
template <int LMAX>
__global__ __launch_bounds__(64 * LMAX) void k_slab_reduce2(RArgs2 q) {
    __shared__ float red[LMAX][64];
    const int i = (int)blockIdx.y >= q.ysplit ? 1 : 0;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y - (i ? q.ysplit : 0);
    if (bx >= q.gx[i]) return;   // (uniform per block: the x extent is the larger of the two)
    const int L = q.L[i];
    if (LMAX >= 16 && L == 16) slab_reduce_block<16, true>(q.a[i], bx, by, 0, red);
    else if (LMAX >= 4 && L == 4) slab_reduce_block<4, true>(q.a[i], bx, by, 0, red);
    else slab_reduce_block<1, true>(q.a[i], bx, by, 0, red);
}

#ifdef RL2_MAIN_TU
void launch_slab_reduce(const RArgs &a, int ng, bool any_bias, hipStream_t s) {
    const dim3 grid((unsigned)((a.B * a.B + 63) / 64), (unsigned)(a.tiles + (any_bias ? a.otiles : 0)), (unsigned)ng);
    if (a.split > 32) k_slab_reduce<16><<<grid, 64 * 16, 0, s>>>(a);
    else if (a.split > 4) k_slab_reduce<4><<<grid, 64 * 4, 0, s>>>(a);
    else k_slab_reduce<1><<<grid, 64, 0, s>>>(a);
}
void launch_slab_reduce2(const RArgs &a0, bool bias0, const RArgs &a1, bool bias1, hipStream_t s) {
    RArgs2 q;
    q.a[0] = a0; q.a[1] = a1;
    const bool bias[2] = {bias0, bias1};
    int gy[2];
    for (int i = 0; i < 2; ++i) {
        q.L[i] = slab_reduce_lanes(q.a[i].split);
        q.gx[i] = (q.a[i].B * q.a[i].B + 63) / 64;
        gy[i] = q.a[i].tiles + (bias[i] ? q.a[i].otiles : 0);
    }
    q.ysplit = gy[0];
    const dim3 grid((unsigned)std::max(q.gx[0], q.gx[1]), (unsigned)(gy[0] + gy[1]), 1u);
    const int lmax = std::max(q.L[0], q.L[1]);
    if (lmax == 16) k_slab_reduce2<16><<<grid, 64 * 16, 0, s>>>(q);
    else if (lmax == 4) k_slab_reduce2<4><<<grid, 64 * 4, 0, s>>>(q);
    else k_slab_reduce2<1><<<grid, 64, 0, s>>>(q);
}
#endif

// Split of the row range for (n, k, o, ng) -- workgroups in flight against rows per workgroup -- and the workspace that goes with it: ONE
// plan, from which wgrad_ws_floats takes the size and wg_setup the grid and the pointers.  Offsets and `floats` in floats from ws.
struct WgPlan { int vw, b, nblk; long split, rows_per_block, slab, bslab, floats; };
constexpr int WG_BLOCKS = 512;   // workgroups aimed at (256 and 1024 measured no better over a step: profiles/r03_knobs_ab.txt)
static WgPlan wg_plan(long n, int k, int o, int ng) {
    WgPlan p{};
    p.vw = (k % 64 == 0 && o % 64 == 0) ? 4 : ((k % 32 == 0 && o % 32 == 0) ? 2 : 0);
    p.b = 16 * p.vw;
    if (!p.vw) return p;
    p.nblk = (o / p.b) * (k / p.b) * ng;
    long split = (WG_BLOCKS + p.nblk - 1) / p.nblk;    // workgroups in flight
    const long max_split = (n + 255) / 256;            // at least 256 rows (4 trips per wave) per workgroup
    if (split > max_split) split = max_split;
    if (split < 1) split = 1;
    p.rows_per_block = ((n + split - 1) / split + 63) / 64 * 64;
    p.split = (n + p.rows_per_block - 1) / p.rows_per_block;
    p.bslab = (long)p.nblk * p.split * p.b * p.b;                      // slab [ng][blocks][split][b^2] at 0, then ...
    p.floats = p.bslab + (long)ng * (o / p.b) * p.split * p.b;         // ... bslab [ng][o / b][split][b]
    return p;
}
#ifdef RL2_MAIN_TU
long wgrad_ws_floats(long n, int k, int o, int ng) { return wg_plan(n, k, o, ng).floats; }
#endif

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Which form a launch takes (K >= 128, one or three inputs; `blocks` 16-column blocks).  PDFOPS_RL_FORM = auto | slab | group, read at
// every launch (a test drives both forms inside one process), forces a form wherever the group form supports the shape.  auto is the
// measured rule: at the row counts of levels 3-5 (12,496 x 128, 3,124 x 256, 780 x 512) every launch beat the slab form by more than its
// spread except the three-output product at K = 128 (28.2 against 29.0 us, spread 0.6-0.9: past its bound by 0.1-0.3 us in two probe runs,
// short of it in a third -- not told from noise), which stays on the slab form (profiles/rowlin_group_probe.txt);
// nothing larger was measured, and there a wave has enough tiles to amortise its fragments.
constexpr long GROUP_MAX_ROWS = 16384;
static bool group_form_wanted(const FwdArgs &a, int k, int blocks) {
    if (blocks % GROUP_GN) return false;
    if (const char *f = getenv("PDFOPS_RL_FORM")) {
        if (!strcmp(f, "slab")) return false;
        if (!strcmp(f, "group")) return true;
    }
    return a.N <= GROUP_MAX_ROWS && !(k == 128 && blocks * 16 > a.O);
}

template <int K, int GN, int NIN, bool PRE, int ST, int MP>
static bool launch_group_kernel(const FwdArgs &a, dim3 grid, hipStream_t s) {
    constexpr int lds = group_lds_bytes<K, GN, NIN, MP>();
    static PdfLdsLimit site;
    if (!pdf_lds_limit_raised(site, reinterpret_cast<const void *>(&k_fwd_group<K, GN, NIN, PRE, ST, MP>), lds)) return false;
    k_fwd_group<K, GN, NIN, PRE, ST, MP><<<grid, 256, lds, s>>>(a);
    return true;
}

// false: the dynamic LDS limit was refused, the caller launches the slab form
template <int K, int GN, int NIN, int MP>
static bool launch_fwd_group(const FwdArgs &a, int blocks, int gx, hipStream_t s) {
    const bool pre = a.scale != nullptr, stats = a.partial != nullptr, bst = stats && a.bx != nullptr;
    const dim3 grid((unsigned)gx, (unsigned)(blocks / GN));
    if (bst) return launch_group_kernel<K, GN, NIN, false, 2, MP>(a, grid, s);
    if constexpr (NIN == 1) {
        if (stats) return pre ? launch_group_kernel<K, GN, 1, true, 1, MP>(a, grid, s) : launch_group_kernel<K, GN, 1, false, 1, MP>(a, grid, s);
    }
    return pre ? launch_group_kernel<K, GN, NIN, true, 0, MP>(a, grid, s) : launch_group_kernel<K, GN, NIN, false, 0, MP>(a, grid, s);
}

// Row blocks of a launch with `nslabs` column slabs (launch_fwd below: what `capped` is for, and the measurements behind FWD_BLOCKS).
constexpr int FWD_BLOCKS = 512;   // total workgroups aimed at
static int fwd_grid_rows(long n, int nslabs, bool capped) {
    const int gx = fwd_row_blocks(n);
    return capped ? std::max(1, std::min(gx, std::max(8, FWD_BLOCKS / std::max(nslabs, 1)))) : gx;
}

template <int K, int NOB, int NIN, int MP>
static int launch_fwd(const FwdArgs &a, int nslabs, hipStream_t s) {   // returns the number of row blocks (= partial rows written)
    const bool pre = a.scale != nullptr, stats = a.partial != nullptr, bst = stats && a.bx != nullptr;
    // Every workgroup first loads its waves' weight fragments (16 NOB columns x K: 8-32 KB per wave).  With many column slabs and few
    // rows (levels 4-5: 3,124 / 780 rows, up to 96 slabs for the three-output q / k / v product) one row block per 64 rows means a wave
    // loads its fragment for a single 16-row tile; fewer row blocks amortise it over several tiles.  (Not with statistics: the partial
    // rows are indexed by row block and sized by pdf_rowlin_partial_rows.)
    // Measured (FWD_BLOCKS = total workgroups aimed at): 512 -> q / k / v product at 3,124 x 256: 41 -> 31 us, three-input dgrad 36 -> 30 us,
    // 780 x 512: 54 -> 46 us, single-slab shapes unchanged; 384 and below lose on the large levels, 1024 and above change nothing.
    const int gx = fwd_grid_rows(a.N, nslabs, !stats || bst);   // (bst: the caller is told the row count)
    if constexpr (K >= 128 && NIN != 2) {
        if (group_form_wanted(a, K, nslabs * NOB) && launch_fwd_group<K, GROUP_GN, NIN, MP>(a, nslabs * NOB, gx, s)) return gx;
    }
    const dim3 grid((unsigned)gx, (unsigned)nslabs);
    if (bst) {   // BatchNorm-backward sums of the output (dgrad kernels: no input prologue)
        k_fwd<K, NOB, NIN, false, 2, MP><<<grid, 256, 0, s>>>(a);
    } else if (NIN == 1 && stats) {
        if (pre) k_fwd<K, NOB, 1, true, 1, MP><<<grid, 256, 0, s>>>(a);
        else k_fwd<K, NOB, 1, false, 1, MP><<<grid, 256, 0, s>>>(a);
    } else {
        if (pre) k_fwd<K, NOB, NIN, true, 0, MP><<<grid, 256, 0, s>>>(a);
        else k_fwd<K, NOB, NIN, false, 0, MP><<<grid, 256, 0, s>>>(a);
    }
    return gx;
}

#ifdef RL2_MAIN_TU
int stats_rows(long n) { return fwd_row_blocks(n); }
long stats_rows_floats(long n, int o) { return (long)fwd_row_blocks(n) * 2 * o; }
#endif

// 16-column blocks per wave of the one-input kernels for (k, cols): the widest instantiated slab that divides the columns (0: k is not covered)
static int fwd_nob1(int k, int cols, bool stats, bool bst) {
    const auto fits = [cols](int nob) { return cols % (nob * 16) == 0; };
    switch (k) {
    case 32: return (!stats && fits(6)) ? 6 : (fits(2) ? 2 : 1);   // (statistics: at most 2 column blocks per wave)
    case 64: return fits(4) ? 4 : 1;
    case 128: { const int wide = bst ? 2 : 4; return fits(wide) ? wide : 1; }   // (ST == 2 with 4 column blocks: 305 registers, one wave per SIMD)
    case 256: return fits(2) ? 2 : 1;
    case 512: return 1;
    default: return 0;
    }
}

// THE place a forward problem is validated and its kernel arguments are made (every field of FwdArgs is set here and nowhere else);
// false: a form or an alignment the streaming kernels do not cover.
static bool fwd_args(const Forward &p, FwdArgs &a) {
    const int nin = p.nin, nout = p.nout, nw = nin > 1 ? nin : nout;
    if (nin < 1 || nout < 1 || (nin > 1 && nout > 1) || nin > 3 || nout > 3) return false;
    if (nin == 2 && (p.scale || p.bx)) return false;   // (the two-window form: plain product only)
    if (p.partial && !p.bx && (nin != 1 || nout != 1)) return false;
    if (p.bx && (!p.partial || nout != 1 || p.scale || !p.bcoef || (p.ldb & 3) || !aligned16(p.bx) || !aligned16(p.bcoef))) return false;
    if ((p.ldx & 3) || (p.ldy & 3) || (p.o & 15)) return false;
    for (int i = 0; i < nw; ++i) if (!aligned16(p.w[i])) return false;
    if (p.scale && (!aligned16(p.scale) || !aligned16(p.shift))) return false;
    for (int i = 0; i < nin; ++i) if (!aligned16(p.x[i])) return false;
    for (int i = 0; i < nout; ++i) if (!aligned16(p.y[i])) return false;
    a = FwdArgs{};
    a.N = p.n; a.O = p.o; a.ldx = p.ldx; a.ldy = p.ldy; a.scale = p.scale; a.shift = p.shift; a.relu = p.relu; a.accumulate = p.accumulate;
    a.partial = p.partial; a.roww = p.roww; a.rws = p.rws;
    a.bx = p.bx; a.ldb = p.ldb; a.bcoef = p.bcoef; a.brelu = p.brelu;
    a.ho_gran = static_cast<unsigned long long *>(p.handoff);
    a.ho_sync = p.handoff ? reinterpret_cast<unsigned *>(a.ho_gran + 2 * (size_t)p.o) : nullptr;
    a.wso = p.transpose_w ? 1 : (p.ldw ? p.ldw : p.k); a.wsk = p.transpose_w ? p.o : 1;
    for (int i = 0; i < nin; ++i) a.X[i] = p.x[i];
    for (int i = 0; i < nw; ++i) a.W[i] = p.w[i];
    for (int i = 0; i < nout; ++i) { a.bias[i] = p.bias[i]; a.Y[i] = p.y[i]; }
    return true;
}
static bool plain1(const Forward &p) { return p.nin == 1 && p.nout == 1 && !p.scale && !p.bx && !p.roww && !p.accumulate && !p.handoff; }   // what the paired kernels take

template <int MP>
int try_forward_mp(const Forward &p, hipStream_t s, int *partial_rows) {
    FwdArgs a;
    if (!fwd_args(p, a)) return 0;
    const int k = p.k, cols = p.o * p.nout;
#define PDF_RL2(K_, NOB_, NIN_) do { if (cols % (NOB_ * 16) == 0) { \
        const int r_ = launch_fwd<K_, NOB_, NIN_, MP>(a, cols / (NOB_ * 16), s); \
        if (partial_rows) *partial_rows = r_; \
        return 1; } } while (0)
    if (p.nin == 1) {
        switch (k * 8 + fwd_nob1(k, cols, p.partial != nullptr, p.bx != nullptr)) {
        case 32 * 8 + 6: PDF_RL2(32, 6, 1); break;
        case 32 * 8 + 2: PDF_RL2(32, 2, 1); break;
        case 32 * 8 + 1: PDF_RL2(32, 1, 1); break;
        case 64 * 8 + 4: PDF_RL2(64, 4, 1); break;
        case 64 * 8 + 1: PDF_RL2(64, 1, 1); break;
        case 128 * 8 + 4: PDF_RL2(128, 4, 1); break;
        case 128 * 8 + 2: PDF_RL2(128, 2, 1); break;
        case 128 * 8 + 1: PDF_RL2(128, 1, 1); break;
        case 256 * 8 + 2: PDF_RL2(256, 2, 1); break;
        case 256 * 8 + 1: PDF_RL2(256, 1, 1); break;
        case 512 * 8 + 1: PDF_RL2(512, 1, 1); break;
        default: break;
        }
    } else if (p.nin == 2) {   // two 512-wide column windows of one 1024-wide input (ldw): ONE accumulation chain over both, bias at the end
        if (k == 512) PDF_RL2(512, 1, 2);
    } else if (p.nin == 3) {
        switch (k) {
        case 32: PDF_RL2(32, 2, 3); break;
        case 64: PDF_RL2(64, 2, 3); break;
        case 128: PDF_RL2(128, 1, 3); break;
        case 256: PDF_RL2(256, 1, 3); break;
        default: break;
        }
    }
#undef PDF_RL2
    return 0;
}

template <int K, int MP>
static bool launch_fwd_group2(const FwdArgs2 &q, unsigned total, hipStream_t s) {
    constexpr int lds = group_lds_bytes<K, GROUP_GN, 1, MP>();
    static PdfLdsLimit site;
    if (!pdf_lds_limit_raised(site, reinterpret_cast<const void *>(&k_fwd_group2<K, GROUP_GN, MP>), lds)) return false;
    k_fwd_group2<K, GROUP_GN, MP><<<total, 256, lds, s>>>(q);
    return true;
}

// Two plain products Y_i (n_i, o_i) = X_i (n_i, k) Wt_i of ONE reduction width in one launch (k_fwd2 / k_fwd_group2).  Paired is what a
// TransitionUp join reaches: both problems on the same kernel, i.e. the same slab width and the same form, at the widths instantiated
// below.  Each problem keeps the row blocks and column slabs launch_fwd gives it; the workgroups of the problem with more tiles per
// workgroup come first.  Returns 1 when the pair was launched; 0 when nothing was launched -- the caller issues two single launches,
// which form the same bits.  Instantiated for fp32 operands only (rowlin2.hip: reduced-precision products take the two launches).
template <int MP>
int try_forward2_mp(const Forward (&p)[2], hipStream_t s) {
    const int k = p[0].k;
    if (p[1].k != k) return 0;
    FwdArgs u[2];
    int nob[2], gx[2], gy[2];
    bool group[2];
    long trips[2];
    for (int i = 0; i < 2; ++i) {
        if (!plain1(p[i]) || p[i].partial || !fwd_args(p[i], u[i])) return 0;
        const long n = p[i].n;
        const int o = p[i].o;
        nob[i] = fwd_nob1(k, o, false, false);
        if (!nob[i]) return 0;
        const int nslabs = o / (nob[i] * 16);
        gx[i] = fwd_grid_rows(n, nslabs, true);
        group[i] = k >= 128 && group_form_wanted(u[i], k, nslabs * nob[i]);
        gy[i] = group[i] ? nslabs * nob[i] / GROUP_GN : nslabs;
        trips[i] = ((n + 15) / 16 + 4L * gx[i] - 1) / (4L * gx[i]);
    }
    if (nob[0] != nob[1] || group[0] != group[1]) return 0;
    const int first = trips[1] > trips[0] ? 1 : 0;
    FwdArgs2 q;
    for (int j = 0; j < 2; ++j) { const int i = j ? 1 - first : first; q.a[j] = u[i]; q.gx[j] = (unsigned)gx[i]; }
    q.split = (unsigned)(gx[first] * gy[first]);
    const unsigned total = q.split + (unsigned)(gx[1 - first] * gy[1 - first]);
    if (group[0]) {
        switch (k) {
        case 128: return launch_fwd_group2<128, MP>(q, total, s) ? 1 : 0;
        case 256: return launch_fwd_group2<256, MP>(q, total, s) ? 1 : 0;
        case 512: return launch_fwd_group2<512, MP>(q, total, s) ? 1 : 0;
        default: return 0;
        }
    }
    switch (k * 8 + nob[0]) {   // (slab form: the joins at o = 32 and 64; wider joins reach the slab form only above GROUP_MAX_ROWS rows: two launches)
    case 32 * 8 + 2: k_fwd2<32, 2, MP><<<total, 256, 0, s>>>(q); return 1;
    case 64 * 8 + 4: k_fwd2<64, 4, MP><<<total, 256, 0, s>>>(q); return 1;
    default: return 0;
    }
}

template <int K0, int NB0, bool G0, int K1, int NB1, bool G1, int MP>
static bool launch_fwd_stats2(const FwdArgs2 &q, unsigned total, hipStream_t s) {
    constexpr int lds0 = G0 ? group_lds_bytes<K0, NB0, 1, MP>() : 0, lds1 = G1 ? group_lds_bytes<K1, NB1, 1, MP>() : 0, lds = lds0 > lds1 ? lds0 : lds1;
    if (lds) {
        static PdfLdsLimit site;
        if (!pdf_lds_limit_raised(site, reinterpret_cast<const void *>(&k_fwd_stats2<K0, NB0, G0, K1, NB1, G1, MP>), lds)) return false;
    }
    k_fwd_stats2<K0, NB0, G0, K1, NB1, G1, MP><<<total, 256, lds, s>>>(q);
    return true;
}

// Y_i (n_i, o) = X_i (n_i, k_i) W_i^T + bias_i with the statistics rows partial_i [fwd_row_blocks(n_i)][2 o], i = 0, 1, in ONE launch
// (k_fwd_stats2).  Paired are the width pairs of the model's joins -- (32, 64), (64, 128), (128, 256), (256, 512), (512, 512) -- in the forms
// launch_fwd gives those widths at the model's row counts.  Problem 0's workgroups always come first: the two problems are different
// template instantiations, so "the longer problem first" would take a mirrored kernel per pair; at levels 4-5, where problem 1 (K = 512)
// has the longer chain per workgroup, both grids together are under two workgroups per CU and start at once, so the order decides nothing
// there.  Returns 1 when the pair was launched; 0 when nothing was launched -- the caller issues two single launches, which form the
// same bits.  Instantiated for fp32 operands only (rowlin2.hip).
template <int MP>
int try_forward_stats2_mp(const Forward (&p)[2], hipStream_t s) {
    const int o = p[0].o;
    if (p[1].o != o) return 0;
    FwdArgs2 q;
    int k[2], nb[2], gy[2];
    bool group[2];
    for (int i = 0; i < 2; ++i) {
        if (!plain1(p[i]) || !p[i].partial || p[i].transpose_w || !fwd_args(p[i], q.a[i])) return 0;
        k[i] = p[i].k;
        const int nob = fwd_nob1(k[i], o, true, false);
        if (!nob) return 0;
        const int blocks = o / 16;
        q.gx[i] = (unsigned)fwd_grid_rows(p[i].n, blocks / nob, false);
        group[i] = k[i] >= 128 && group_form_wanted(q.a[i], k[i], blocks);
        nb[i] = group[i] ? GROUP_GN : nob;
        gy[i] = blocks / nb[i];
    }
    q.split = q.gx[0] * (unsigned)gy[0];
    const unsigned total = q.split + q.gx[1] * (unsigned)gy[1];
#define PDF_RL2S(K0_, NB0_, G0_, K1_, NB1_, G1_) \
    if (k[0] == K0_ && nb[0] == NB0_ && group[0] == G0_ && k[1] == K1_ && nb[1] == NB1_ && group[1] == G1_) \
        return launch_fwd_stats2<K0_, NB0_, G0_, K1_, NB1_, G1_, MP>(q, total, s) ? 1 : 0
    PDF_RL2S(32, 2, false, 64, 1, false);
    PDF_RL2S(64, 4, false, 128, GROUP_GN, true);
    PDF_RL2S(128, GROUP_GN, true, 256, GROUP_GN, true);
    PDF_RL2S(256, GROUP_GN, true, 512, GROUP_GN, true);
    PDF_RL2S(512, GROUP_GN, true, 512, GROUP_GN, true);
#undef PDF_RL2S
    return 0;
}

// THE place the arguments, grid and reduction of a k_wg launch are made, from the plan that sized the workspace (every field of WArgs
// and RArgs is set here and nowhere else); false: the shape or an alignment is not covered.
struct WgSetup { WArgs a; RArgs r; dim3 grid; int vw; bool any_bias; };
static bool wg_setup(const Wgrad &p, WgSetup &u) {
    const bool pz = p.per_gradient;
    if (p.ng < 1 || p.ng > (pz ? WG_MAXG : 3) || !p.ws) return false;
    const WgPlan pl = wg_plan(p.n, p.k, p.o, p.ng);
    const int vw = pl.vw, b = pl.b;
    if (!vw) return false;
    if ((p.ldg % vw) || (p.ldx % vw)) return false;
    if (pz) {
        if (p.roww) return false;   // (no kernel is instantiated for per-gradient inputs with a row weight)
    } else {
        if (!aligned16(p.x)) return false;
        if (p.scale && (!aligned16(p.scale) || !aligned16(p.shift))) return false;
    }
    for (int i = 0; i < p.ng; ++i) {
        if (!aligned16(p.g[i])) return false;
        if (pz && (!aligned16(p.xz[i]) || (p.scalez[i] && (!aligned16(p.scalez[i]) || !aligned16(p.shiftz[i]))))) return false;
    }
    u = WgSetup{};
    WArgs &a = u.a;
    a.N = p.n; a.K = p.k; a.O = p.o; a.ldg = p.ldg; a.ldx = p.ldx; a.roww = p.roww; a.rws = p.rws;
    a.per_z = pz ? 1 : 0;
    if (!pz) { a.X = p.x; a.scale = p.scale; a.shift = p.shift; a.relu = p.relu; }
    for (int i = 0; i < p.ng; ++i) {
        a.G[i] = p.g[i]; a.dW[i] = p.dw[i]; a.db[i] = p.db[i];
        if (pz) { a.Xz[i] = p.xz[i]; a.scalez[i] = p.scalez[i]; a.shiftz[i] = p.shiftz[i]; a.reluz[i] = p.reluz[i]; }
        u.any_bias = u.any_bias || a.db[i] != nullptr;
    }
    a.rows_per_block = pl.rows_per_block;
    a.slab = p.ws + pl.slab;
    a.bslab = p.ws + pl.bslab;
    u.vw = vw;
    u.grid = dim3((unsigned)pl.split, (unsigned)((p.o / b) * (p.k / b)), (unsigned)p.ng);
    RArgs &r = u.r;
    r.slab = a.slab; r.bslab = a.bslab; r.B = b; r.tiles_k = p.k / b; r.tiles = (p.o / b) * (p.k / b); r.otiles = p.o / b; r.split = (int)pl.split;
    r.K = p.k; r.O = p.o;
    for (int i = 0; i < WG_MAXG; ++i) { r.dW[i] = a.dW[i]; r.db[i] = a.db[i]; }
    return true;
}

// One k_wg launch + one slab reduction, for gradients that share the layer input and for up to WG_MAXG gradients of ONE shape with their
// OWN inputs (Wgrad::per_gradient; kernels with the prologue, which a null scalez[i] runs as the identity).  A Bottleneck's backward has
// five such products (linear3, q / k / v, linear1: all c x c over the block's n rows); issued one by one at levels 3-5 each of them is a
// launch that fills a fraction of the chip followed by its own reduction launch.
template <int MP>
int try_wgrad_mp(const Wgrad &p, hipStream_t s) {
    WgSetup u;
    if (!wg_setup(p, u)) return 0;
    const WArgs &a = u.a;
    const dim3 grid = u.grid;
    const bool pre = p.per_gradient || p.scale != nullptr;
#define PDF_WG(VW_) do { \
        if (p.roww) { if (pre) k_wg<VW_, true, true, MP><<<grid, 256, 0, s>>>(a); else k_wg<VW_, false, true, MP><<<grid, 256, 0, s>>>(a); } \
        else        { if (pre) k_wg<VW_, true, false, MP><<<grid, 256, 0, s>>>(a); else k_wg<VW_, false, false, MP><<<grid, 256, 0, s>>>(a); } } while (0)
    if (u.vw == 4) PDF_WG(4); else PDF_WG(2);
#undef PDF_WG
    launch_slab_reduce(u.r, p.ng, u.any_bias, s);
    return 1;
}

// Two single weight gradients dW_i (o_i, k_i) = G_i^T X_i (no prologue, own workspace each) whose slab reductions the caller launches
// (r[i]: launch_slab_reduce2).  pair: the two products as ONE launch -- k_wg2 where both take the same vector width, the workgroups of the
// problem with more rows per workgroup first; k_wg2_roww where problem 0 carries a row weight (problem 0 first, each with its own vector
// width) -- otherwise one launch each, as try_wgrad_mp issues them.  Either way every workgroup runs wg_block over the grid of its own
// problem: the same slabs.  Returns 2 for one launch, 1 for two; 0: a shape or an alignment is not covered, nothing was launched.
template <int MP>
int try_wgrad_pair_mp(const Wgrad (&p)[2], bool pair, hipStream_t s, RArgs *r) {
    WgSetup u[2];
    for (int i = 0; i < 2; ++i)
        if (p[i].ng != 1 || p[i].per_gradient || p[i].scale || (i == 1 && p[i].roww) || !wg_setup(p[i], u[i])) return 0;
    const bool rw = p[0].roww != nullptr;
    r[0] = u[0].r; r[1] = u[1].r;
    if constexpr (MP == 0) {   // (the paired kernels are built for fp32 operands only: reduced-precision products take one launch each)
        if (pair && (rw ? u[1].vw == 2 : u[0].vw == u[1].vw)) {
            const int first = !rw && u[1].a.rows_per_block > u[0].a.rows_per_block ? 1 : 0;
            WArgs2 q;
            for (int j = 0; j < 2; ++j) { const WgSetup &v = u[j ? 1 - first : first]; q.a[j] = v.a; q.gx[j] = v.grid.x; q.gy[j] = v.grid.y; }
            q.split = q.gx[0] * q.gy[0];
            const unsigned total = q.split + q.gx[1] * q.gy[1];
            if (rw) { if (u[0].vw == 4) k_wg2_roww<4, 2, 0><<<total, 256, 0, s>>>(q); else k_wg2_roww<2, 2, 0><<<total, 256, 0, s>>>(q); }
            else if (u[0].vw == 4) k_wg2<4, 0><<<total, 256, 0, s>>>(q);
            else k_wg2<2, 0><<<total, 256, 0, s>>>(q);
            return 2;
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (i == 0 && rw) { if (u[i].vw == 4) k_wg<4, false, true, MP><<<u[i].grid, 256, 0, s>>>(u[i].a); else k_wg<2, false, true, MP><<<u[i].grid, 256, 0, s>>>(u[i].a); }
        else if (u[i].vw == 4) k_wg<4, false, false, MP><<<u[i].grid, 256, 0, s>>>(u[i].a);
        else k_wg<2, false, false, MP><<<u[i].grid, 256, 0, s>>>(u[i].a);
    }
    return 1;
}

template <int VW, int K, int NB, bool GROUP>
static bool launch_wg_fwd(const WgFwdArgs &q, unsigned total, hipStream_t s) {
    constexpr int lds = wg_fwd_lds_bytes<VW, K, NB, GROUP>();
    static PdfLdsLimit site;
    if (!pdf_lds_limit_raised(site, reinterpret_cast<const void *>(&k_wg_fwd<VW, K, NB, GROUP>), lds)) return false;
    k_wg_fwd<VW, K, NB, GROUP><<<total, 256, lds, s>>>(q);
    return true;
}

// The grouped weight gradients w (per-gradient inputs: a Bottleneck's five c x c products) and the plain product f (one input, one
// output, no prologue, statistics or row weight; `accumulate` allowed: the block's gx += dy W1) as ONE launch (k_wg_fwd), followed by the
// gradients' slab reduction.  Paired are the forms the model's five levels reach: the slab products at K = 32 / 64 beside the VW = 2 / 4
// gradients, and the group-form products at K = 128 / 256 / 512 beside the VW = 4 gradients; each problem keeps the grid its single launch
// has (wg_setup; launch_fwd's row blocks, column slabs and choice of form).  Returns 1 when everything was launched; 0 when nothing was
// (another form, an alignment, a refused LDS limit) -- the caller issues the single launches, which form the same bits.  fp32 operands only.
template <int MP>
int try_wgrad_fwd_mp(const Wgrad &w, const Forward &f, hipStream_t s) {
    static_assert(MP == 0, "the paired kernel is built for fp32 operands only");
    WgFwdArgs q;
    WgSetup u;
    if (!w.per_gradient || f.nin != 1 || f.nout != 1 || f.scale || f.bx || f.roww || f.handoff || f.partial) return 0;
    if (!wg_setup(w, u) || !fwd_args(f, q.f)) return 0;
    const int k = f.k, nob = fwd_nob1(k, f.o, false, false);
    if (!nob) return 0;
    const int nslabs = f.o / (nob * 16);
    const int gx = fwd_grid_rows(f.n, nslabs, true);
    const bool group = k >= 128 && group_form_wanted(q.f, k, nslabs * nob);
    const int gy = group ? nslabs * nob / GROUP_GN : nslabs;
    q.w = u.a; q.wgx = u.grid.x; q.wgy = u.grid.y; q.split = u.grid.x * u.grid.y * u.grid.z; q.fgx = (unsigned)gx;
    const unsigned total = q.split + (unsigned)(gx * gy);
    bool ok = false;
    if (group && u.vw == 4) {
        if (k == 128) ok = launch_wg_fwd<4, 128, GROUP_GN, true>(q, total, s);
        else if (k == 256) ok = launch_wg_fwd<4, 256, GROUP_GN, true>(q, total, s);
        else if (k == 512) ok = launch_wg_fwd<4, 512, GROUP_GN, true>(q, total, s);
    } else if (!group) {
        if (k == 32 && nob == 2 && u.vw == 2) ok = launch_wg_fwd<2, 32, 2, false>(q, total, s);
        else if (k == 64 && nob == 4 && u.vw == 4) ok = launch_wg_fwd<4, 64, 4, false>(q, total, s);
    }
    if (!ok) return 0;
    launch_slab_reduce(u.r, w.ng, u.any_bias, s);
    return 1;
}

}  // namespace rl2
