// Distillation loss of the incremental learner (pointcept/incrLearners/ours/pointpdf_incr_v1m1_base.py:62-87, IncrDistillKlLoss):
//   logp = log_softmax(pred / T_p) over the student's Cs classes;
//   t    = [softmax(teacher / T_t), 0 ... 0] (Ct -> Cs columns), or onehot(label) on the rows whose label is not `ignore`;
//   loss = sum_rows sum_j (xlogy(t_j, t_j) - t_j logp_j) / N       (F.kl_div(..., "batchmean"): the divisor is ALL N rows).
// The reference builds the target with a boolean-mask assignment (a nonzero: host sync) and ~10 torch kernels; here it is one
// launch per row block + one fixed-order sum per direction, nothing read back to the host, so the step stays capturable.
// One lane owns one row (Cs <= 64 logits and the target row in registers); the workgroup's sum goes by waves to its own slot and one
// workgroup totals the slots (slot_sum.h).  The forward leaves the row gradient  softmax(pred / T_p) * sum_j t_j - t  in `grad`; the
// backward scales it by gy / (T_p N) and only READS it.
// Bound: HBM ((Cs + Ct) * 4 + 8 bytes read, Cs * 4 written per row).
#include "slot_sum.h"

namespace {

constexpr int LB = 256;
constexpr int MAXC = 64;   // widest head served; the row kernel is instantiated for 16 / 32 / 64 columns (register footprint)
constexpr int PDF_KL_HEAD = 4, PDF_KL_MAX_BLOCKS = 1024;   // acc = [sum, scale, loss, -] + one partial sum per workgroup

template <int W>
__global__ __launch_bounds__(LB) void k_kl_fwd(long n, int cs, int ct, const float *__restrict__ student, const float *__restrict__ teacher,
                                               const long *__restrict__ labels, long ignore, float inv_tp, float inv_tt,
                                               float *__restrict__ grad, float *__restrict__ acc) {
    float loss = 0.f;
    for (long r = (long)blockIdx.x * LB + threadIdx.x; r < n; r += (long)gridDim.x * LB) {
        const float *x = student + r * cs;
        float a[W], t[W];
        float m = -__builtin_huge_valf();
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < cs) { a[j] = x[j] * inv_tp; m = fmaxf(m, a[j]); }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < cs) s += __expf(a[j] - m);
        const float lse = m + __logf(s);   // logp_j = a_j - lse
        const long lab = labels[r];
        float row = 0.f, tsum;
        if (lab != ignore) {   // onehot target: xlogy(1, 1) = 0, the other columns contribute exactly 0
            const bool ok = lab >= 0 && lab < cs;
            // a label that is neither the ignore value nor a class id poisons the loss (as csrc/loss.hip): a mis-sized head / label
            // map shows up as a NaN loss on the first step, without a host sync; the row's gradient stays 0
            float picked = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j) {   // (static indices only: the rows stay in registers)
                const bool hit = ok && j == lab;
                if (j < cs) t[j] = hit ? 1.f : 0.f;
                if (hit) picked = a[j];
            }
            row = ok ? lse - picked : __builtin_nanf("");
            tsum = ok ? 1.f : 0.f;
        } else {   // softmax(teacher / T_t) on the first Ct columns, zero padding after them
            const float *y = teacher + r * ct;
            float mt = -__builtin_huge_valf();
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j < ct) { t[j] = y[j] * inv_tt; mt = fmaxf(mt, t[j]); }
            float st = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (j < ct) st += __expf(t[j] - mt);
            const float lst = __logf(st), ist = 1.f / st;
            tsum = 0.f;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (j < ct) {
                    const float logt = t[j] - mt - lst;
                    const float tj = __expf(t[j] - mt) * ist;
                    row += tj > 0.f ? tj * (logt - (a[j] - lse)) : 0.f;   // xlogy(0, 0) = 0: an underflowed target adds nothing
                    t[j] = tj;
                    tsum += tj;
                } else if (j < cs) {
                    t[j] = 0.f;
                }
            }
        }
        loss += row;
        float *g = grad + r * cs;
        const float is = 1.f / s;
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (j < cs) g[j] = __expf(a[j] - m) * is * tsum - t[j];
    }
    float v[1] = {loss};
    block_sum_by_waves<LB>(v, acc + PDF_KL_HEAD + blockIdx.x);   // the workgroup's own slot
}

// acc[PDF_KL_HEAD + g] = the workgroups' sums -> acc[0] = total, acc[1] = 1 / (T_p N) (the backward's scale), out = total / N.
// One workgroup: slot_total.
__global__ __launch_bounds__(LB) void k_kl_mean(float *__restrict__ acc, int blocks, long n, float inv_tp, float *__restrict__ out) {
    float t[1];
    if (!slot_total<LB>(acc + PDF_KL_HEAD, blocks, t)) return;
    const float inv_n = 1.f / (float)n;
    acc[0] = t[0];
    acc[1] = inv_tp * inv_n;
    out[0] = t[0] * inv_n;
}

// grad_pred = dgrad * gy / (T_p N).  The forward's buffer is only READ: a second backward over the same graph (retain_graph) sees
// the unscaled values again.
__global__ __launch_bounds__(LB) void k_kl_bwd(long total, const float *__restrict__ dgrad, const float *__restrict__ acc,
                                               const float *__restrict__ gy, float *__restrict__ out) {
    pdf_scaled_copy<LB>(total, dgrad, gy[0] * acc[1], out);
}

}  // namespace

extern "C" long pdf_incr_kl_workspace_floats(void) { return PDF_KL_HEAD + (long)PDF_KL_MAX_BLOCKS; }

extern "C" int pdf_incr_kl_forward(long n, int cs, int ct, const float *student, const float *teacher, const long *labels, long ignore,
                                   float inv_tp, float inv_tt, float *grad, float *acc, float *loss, void *stream) {
    if (n < 1 || cs < 1 || ct < 1 || ct > cs || !student || !teacher || !labels || !grad || !acc || !loss) return PDF_ERR_BAD_ARG;
    if (cs > MAXC) return PDF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long g = (n + LB - 1) / LB;
    if (g > PDF_KL_MAX_BLOCKS) g = PDF_KL_MAX_BLOCKS;
    if (cs <= 16) k_kl_fwd<16><<<(unsigned)g, LB, 0, s>>>(n, cs, ct, student, teacher, labels, ignore, inv_tp, inv_tt, grad, acc);
    else if (cs <= 32) k_kl_fwd<32><<<(unsigned)g, LB, 0, s>>>(n, cs, ct, student, teacher, labels, ignore, inv_tp, inv_tt, grad, acc);
    else k_kl_fwd<MAXC><<<(unsigned)g, LB, 0, s>>>(n, cs, ct, student, teacher, labels, ignore, inv_tp, inv_tt, grad, acc);
    k_kl_mean<<<1, LB, 0, s>>>(acc, (int)g, n, inv_tp, loss);
    return pdf_launch_status();
}

extern "C" int pdf_incr_kl_backward(long n, int cs, const float *dgrad, const float *acc, const float *gy, float *out, void *stream) {
    if (n < 1 || cs < 1 || !dgrad || !acc || !gy || !out) return PDF_ERR_BAD_ARG;
    long g = (n * cs + LB - 1) / LB;
    if (g > 2048) g = 2048;
    k_kl_bwd<<<(unsigned)g, LB, 0, static_cast<hipStream_t>(stream)>>>(n * cs, dgrad, acc, gy, out);
    return pdf_launch_status();
}
