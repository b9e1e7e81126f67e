// Host interface of the streaming per-point Linear kernels (namespace rl2): THE declaration of what rowlin.hip (the C entry points) calls
// and rowlin2_impl.h / rowlin2{,_f16,_bf16}.hip define.  A product is DESCRIBED -- a Forward or a Wgrad with default member
// initialisers, so a call site names only what it uses -- and handed to a try_* function, which returns 0 without launching anything
// when the streaming kernels do not cover the shape or an alignment (the caller then takes the tiled kernel or reports it).
#pragma once
#include "pdfops_common.h"

namespace rl2 {

constexpr int WG_MAXG = 5;   // weight gradients of one launch (blockIdx.z): q / k / v of one input, or the five c x c products of a Bottleneck

// `mma_input` of the C entry points (include/pdfops.h; rowlin2_impl.h: Mma): 0 fp32, 1 fp16, 2 bfloat16 product operands
static inline bool mma_input_ok(int mma) { return mma >= 0 && mma <= 2; }

// Forward product / input gradient, every form of k_fwd:
//   nin = 1, nout = 1..3 :  y[i] (n, o) (+)= roww .* (f(x[0]) Wt[i]) + bias[i]
//   nin = 1..3, nout = 1 :  y[0] (n, o) (+)= sum_i x[i] Wt[i] + bias[0]      (nin = 2: the two-window form, plain product only)
// f = relu?(x * scale[k] + shift[k]) where scale is non-null.  Callers have checked n, k, o >= 1.
struct Forward {
    long n = 0; int k = 0, o = 0, nin = 1, nout = 1;
    const float *x[3] = {}; long ldx = 0;
    const float *w[3] = {};            // per input (nin > 1) or per output
    long ldw = 0;                      // row stride of an (o, k) window of a wider weight matrix (0: k)
    int transpose_w = 0;               // 0: W is (o, k) row-major; 1: (k, o) row-major (the layer's own weight, for the input gradient)
    const float *bias[3] = {};         // per output (nullable)
    const float *scale = nullptr, *shift = nullptr; int relu = 0;   // prologue (k floats each)
    float *y[3] = {}; long ldy = 0;
    int accumulate = 0;
    float *partial = nullptr;          // statistics rows [row blocks][2 o] of the single output: [sum | sum of squares], or with bx ...
    const float *bx = nullptr; long ldb = 0; const float *bcoef = nullptr; int brelu = 0;   // ... the BatchNorm-backward sums (FwdArgs)
    const float *roww = nullptr; long rws = 0;   // per-row factor of the product, element stride rws
    void *handoff = nullptr;           // statistics only: the consumer's handoff scratch (pdfops_common.h: PdfRowsBn), zeroed by the launch
};

// Weight gradients dW_i (o, k) = G_i^T f(X), db_i (o) = column sums of G_i (null: not computed), i < ng; everything is WRITTEN.
//   shared input (per_gradient = false, ng <= 3):  x / scale / shift / relu, optional row weight of G
//   per-gradient inputs (per_gradient = true, ng <= WG_MAXG):  xz[i] and, where scalez[i] is non-null, its own prologue
// ws: wgrad_ws_floats(n, k, o, ng) floats.
struct Wgrad {
    long n = 0; int k = 0, o = 0, ng = 1;
    const float *g[WG_MAXG] = {}; long ldg = 0;
    long ldx = 0;
    const float *x = nullptr, *scale = nullptr, *shift = nullptr; int relu = 0;
    bool per_gradient = false;
    const float *xz[WG_MAXG] = {}, *scalez[WG_MAXG] = {}, *shiftz[WG_MAXG] = {}; int reluz[WG_MAXG] = {};
    float *dw[WG_MAXG] = {}, *db[WG_MAXG] = {};
    float *ws = nullptr;
    const float *roww = nullptr; long rws = 0;   // dW = sum_n roww[n] G[n]^T f(X[n])
};

// Sum of the `split` slabs of every dW block (and bias block) in a fixed order: lane l of an element adds slabs l, l + L, l + 2L, ...,
// the L partial sums are combined in lane order.  grid = (ceil(B^2 / 64), tiles + bias tiles, ng), 64 L threads.  Works for the tiled
// kernel of rowlin.hip as well (B = 32, edge blocks masked by O / K).  Passed to the kernel by value: value-initialise it (RArgs r{};)
// before filling it, so that every one of the WG_MAXG slots is defined.
struct RArgs {
    const float *slab, *bslab;
    float *dW[WG_MAXG], *db[WG_MAXG];
    int B, tiles_k, tiles, otiles, split, K, O;
};

// Each returns 1 when a streaming kernel took the job, 0 when the shape is not covered and nothing was launched.
int try_forward(const Forward &p, int mma, hipStream_t s, int *partial_rows = nullptr);   // partial_rows: receives the statistics rows written
// Two products in one launch; the caller issues two single launches on 0, which form the same bits.  fp32 operands only (mma != 0: 0).
int try_forward2(const Forward (&p)[2], int mma, hipStream_t s);         // plain products of ONE reduction width k (k_fwd2 / k_fwd_group2)
int try_forward_stats2(const Forward (&p)[2], int mma, hipStream_t s);   // one output width o, statistics epilogue (k_fwd_stats2)
int try_wgrad(const Wgrad &p, int mma, hipStream_t s);   // the product and its slab reduction
// Two single weight gradients without prologue whose reductions are left to the caller (r[2]: launch_slab_reduce2); p[0] may carry a row
// weight.  Returns 2: one launch, 1: two.
int try_wgrad_pair(const Wgrad (&p)[2], bool pair, int mma, hipStream_t s, RArgs *r);
// Grouped weight gradients (per_gradient) + their reduction with ONE plain product in the products' launch (k_wg_fwd): 1, or 0 and nothing launched.
int try_wgrad_fwd(const Wgrad &w, const Forward &f, int mma, hipStream_t s);
void launch_slab_reduce(const RArgs &a, int ng, bool any_bias, hipStream_t s);
void launch_slab_reduce2(const RArgs &a0, bool bias0, const RArgs &a1, bool bias1, hipStream_t s);
int stats_rows(long n);                  // rows of the statistics epilogue ...
long stats_rows_floats(long n, int o);   // ... and their floats, [row blocks][2 o]
long wgrad_ws_floats(long n, int k, int o, int ng);

}  // namespace rl2
