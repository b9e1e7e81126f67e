// SGD with momentum and weight decay over ALL parameter tensors of the model in ONE launch (torch.optim.SGD semantics, dampening = 0,
// no Nesterov: engines/defaults build the reference's optimizer from configs/_base_/default_runtime + the dataset config: SGD,
// momentum 0.9, weight_decay 1e-4):   g' = g + wd * p;   buf = momentum * buf + g';   p -= lr * buf.
// torch's fused multi-tensor SGD packs ~24 tensors per launch: 13 launches and 275 us per step for this model's 304 tensors (8.5 M
// values, 170 MB of traffic = 21 us at the HBM peak).  Here the host hands over a table of (param, grad, momentum, length) and a
// chunk list; one workgroup = one chunk of CH values of one tensor.  Bound: HBM.
#include "pdfops_common.h"

namespace {

constexpr int OB = 256, CH = 4096;   // threads per workgroup, values per chunk

struct SgdTensor { float *p; const float *g; float *m; long n; };

__global__ __launch_bounds__(OB) void k_sgd(const SgdTensor *__restrict__ tab, const int2 *__restrict__ chunks, float lr, float momentum,
                                            float wd, const float *__restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;        // (uniform: a GradScaler step with a non-finite gradient changes nothing)
    const int2 c = chunks[blockIdx.x];                 // (tensor, chunk inside the tensor)
    const SgdTensor t = tab[c.x];
    const long base = (long)c.y * CH;
    const long left = t.n - base;
    float *p = t.p + base, *m = t.m + base;
    const float *g = t.g + base;
    if (left >= CH && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m)) & 15) == 0) {
        float4 pv[CH / (4 * OB)], gv[CH / (4 * OB)], mv[CH / (4 * OB)];
#pragma unroll
        for (int k = 0; k < CH / (4 * OB); ++k) {
            const int e = threadIdx.x + k * OB;
            pv[k] = reinterpret_cast<const float4 *>(p)[e]; gv[k] = reinterpret_cast<const float4 *>(g)[e]; mv[k] = reinterpret_cast<const float4 *>(m)[e];
        }
#pragma unroll
        for (int k = 0; k < CH / (4 * OB); ++k) {
            const int e = threadIdx.x + k * OB;
            float4 b;
            b.x = momentum * mv[k].x + (gv[k].x + wd * pv[k].x); b.y = momentum * mv[k].y + (gv[k].y + wd * pv[k].y);
            b.z = momentum * mv[k].z + (gv[k].z + wd * pv[k].z); b.w = momentum * mv[k].w + (gv[k].w + wd * pv[k].w);
            reinterpret_cast<float4 *>(m)[e] = b;
            reinterpret_cast<float4 *>(p)[e] = make_float4(pv[k].x - lr * b.x, pv[k].y - lr * b.y, pv[k].z - lr * b.z, pv[k].w - lr * b.w);
        }
    } else {
        const long n = left < CH ? left : CH;
        for (long e = threadIdx.x; e < n; e += OB) {
            const float pe = p[e];
            const float b = momentum * m[e] + (g[e] + wd * pe);
            m[e] = b;
            p[e] = pe - lr * b;
        }
    }
}

// GradScaler.unscale_ (torch/amp/grad_scaler.py: _unscale_grads_ -> _amp_foreach_non_finite_check_and_unscale_) over the same tables:
// g *= inv_scale in place; found_inf = 1 if any gradient value is inf / nan (every workgroup that sees one stores the same 1.0f: no
// atomics, no ordering needed).  found_inf must be 0 on entry (pdf_scaler_update leaves it so).
template <class Tensor>   // (SgdTensor or AdamTensor: the record's grad pointer and length)
__global__ __launch_bounds__(OB) void k_unscale(const Tensor *__restrict__ tab, const int2 *__restrict__ chunks,
                                                const float *__restrict__ inv_scale, float *found_inf) {
    const int2 c = chunks[blockIdx.x];
    const float *tg = tab[c.x].g;
    const long tn = tab[c.x].n;
    const long base = (long)c.y * CH;
    const long left = tn - base;
    float *g = const_cast<float *>(tg) + base;
    const float is = *inv_scale;
    bool bad = false;
    if (left >= CH && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        float4 gv[CH / (4 * OB)];
#pragma unroll
        for (int k = 0; k < CH / (4 * OB); ++k) gv[k] = reinterpret_cast<const float4 *>(g)[threadIdx.x + k * OB];
#pragma unroll
        for (int k = 0; k < CH / (4 * OB); ++k) {
            bad = bad || !(isfinite(gv[k].x) && isfinite(gv[k].y) && isfinite(gv[k].z) && isfinite(gv[k].w));
            reinterpret_cast<float4 *>(g)[threadIdx.x + k * OB] = make_float4(gv[k].x * is, gv[k].y * is, gv[k].z * is, gv[k].w * is);
        }
    } else {
        const long n = left < CH ? left : CH;
        for (long e = threadIdx.x; e < n; e += OB) {
            const float v = g[e];
            bad = bad || !isfinite(v);
            g[e] = v * is;
        }
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) *found_inf = 1.f;
}

// GradScaler.update (torch/amp/grad_scaler.py: _amp_update_scale_): found_inf -> scale *= backoff, tracker = 0; else tracker += 1 and
// at `interval` consecutive clean steps scale *= growth, tracker = 0.  Leaves inv_scale = 1 / scale and found_inf = 0 for the next step.
__global__ void k_scaler_update(float *scale, float *inv_scale, int *tracker, float *found_inf, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = *scale;
    if (*found_inf != 0.f) {
        s *= backoff;
        *tracker = 0;
    } else {
        const int t = *tracker + 1;
        if (t >= interval) {
            const float grown = s * growth;
            if (isfinite(grown)) s = grown;   // (torch keeps the scale when growing would overflow)
            *tracker = 0;
        } else {
            *tracker = t;
        }
    }
    *scale = s;
    *inv_scale = 1.f / s;
    *found_inf = 0.f;
}

// Adam / AdamW (torch.optim.Adam / AdamW: the single-tensor, non-capturable form of torch/optim/adam.py; configs/scannet/openseg-pt-v1-0-*
// and the openseg-st-v1m1 configs build AdamW) over all tensors of one parameter group.  Same shape as k_sgd: a record table + a
// {tensor, chunk} list, one workgroup per chunk.  Reads p, g, m, v and writes p, m, v: 28 B per value.  Bound: HBM.
//   p *= 1 - lr wd (decoupled)  |  g += wd p (L2 form);   m += (1 - b1)(g - m);   v = b2 v + (1 - b2) g g;
//   p -= (lr / (1 - b1^step)) m / (sqrt(v) / sqrt(1 - b2^step) + eps)
// The scalars (1 - lr wd, lr / bc1, sqrt(bc2)) are formed in double from this call's hyper-parameters and this tensor's step count and
// rounded to float once, as torch's Python scalars are when they reach its kernels.  Every product and sum below rounds as torch's
// vectorised CPU kernels round it (lerp, addcmul and add-with-alpha are one fused multiply-add each; mul, sqrt, div and addcdiv's
// (value * m) / denom round every operation), so contraction is switched off and the fused operations are written out.
struct AdamTensor { float *p; const float *g; float *m; float *v; float *step; long n; long pad[2]; };   // 64 bytes
static_assert(sizeof(AdamTensor) == 64, "AdamTensor: the host writes 8 x int64 rows");

struct AdamScalars { float decay, w1, b2, w2, nstep, sqrt_bc2, eps, wd; };

// The per-tensor step counts advance in a launch of their own, ahead of k_adam: every chunk of a tensor reads the same, already
// advanced count (a chunk-0 increment would race with the other chunks' reads).  Guarded like the update itself.
__global__ void k_adam_tick(const AdamTensor *__restrict__ tab, int ntensors, const float *__restrict__ found_inf) {
    if (found_inf && *found_inf != 0.f) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ntensors) *tab[i].step += 1.f;
}

__device__ __forceinline__ void adam_value(const AdamScalars &s, int decoupled, float &p, float g, float &m, float &v) {
#pragma clang fp contract(off)
    if (decoupled) p = p * s.decay;
    else g = fmaf(s.wd, p, g);
    m = fmaf(s.w1, g - m, m);
    v = fmaf(s.w2 * g, g, v * s.b2);
    const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
    p = p + (s.nstep * m) / denom;
}

__global__ __launch_bounds__(OB) void k_adam(const AdamTensor *__restrict__ tab, const int2 *__restrict__ chunks, double lr, double beta1,
                                             double beta2, double eps, double wd, int decoupled, const float *__restrict__ found_inf) {
#pragma clang fp contract(off)                         // (the double scalars too: 1 - lr wd is Python's two operations)
    if (found_inf && *found_inf != 0.f) return;        // (uniform; the tick launch skipped the step counts too)
    __shared__ AdamScalars sh;
    const int2 c = chunks[blockIdx.x];
    const AdamTensor t = tab[c.x];
    const long base = (long)c.y * CH;
    const long left = t.n - base;
    float *p = t.p + base, *m = t.m + base, *v = t.v + base;
    const float *g = t.g + base;
    const bool wide = left >= CH && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                                     reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    constexpr int K = CH / (4 * OB);
    float4 pv[K], gv[K], mv[K], vv[K];
    if (wide) {   // (the loads are in flight while wave 0 forms the scalars)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = threadIdx.x + k * OB;
            pv[k] = reinterpret_cast<const float4 *>(p)[e]; gv[k] = reinterpret_cast<const float4 *>(g)[e];
            mv[k] = reinterpret_cast<const float4 *>(m)[e]; vv[k] = reinterpret_cast<const float4 *>(v)[e];
        }
    }
    if (threadIdx.x == 0) {
        const double step = (double)*t.step;
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
        AdamScalars s;
        s.decay = (float)(1.0 - lr * wd);
        s.w1 = (float)(1.0 - beta1);
        s.b2 = (float)beta2;
        s.w2 = (float)(1.0 - beta2);
        s.nstep = (float)(-(lr / bc1));
        s.sqrt_bc2 = (float)sqrt(bc2);
        s.eps = (float)eps;
        s.wd = (float)wd;
        sh = s;
    }
    __syncthreads();
    const AdamScalars s = sh;
    const int dec = decoupled || wd == 0.0;   // (torch skips the decay altogether at weight_decay == 0: p * 1 and g + 0 p change nothing)
    if (wide) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = threadIdx.x + k * OB;
            adam_value(s, dec, pv[k].x, gv[k].x, mv[k].x, vv[k].x);
            adam_value(s, dec, pv[k].y, gv[k].y, mv[k].y, vv[k].y);
            adam_value(s, dec, pv[k].z, gv[k].z, mv[k].z, vv[k].z);
            adam_value(s, dec, pv[k].w, gv[k].w, mv[k].w, vv[k].w);
            reinterpret_cast<float4 *>(m)[e] = mv[k];
            reinterpret_cast<float4 *>(v)[e] = vv[k];
            reinterpret_cast<float4 *>(p)[e] = pv[k];
        }
    } else {
        const long n = left < CH ? left : CH;
        for (long e = threadIdx.x; e < n; e += OB) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_value(s, dec, pe, g[e], me, ve);
            m[e] = me;
            v[e] = ve;
            p[e] = pe;
        }
    }
}

}  // namespace

extern "C" int pdf_sgd_chunk(void) { return CH; }

// tab: ntensors x {param*, grad*, momentum*, length} (device, 32 bytes each); chunks: nchunks x {tensor, chunk} int32 pairs (device).
// found_inf (device float, nullable): non-zero = the whole step is skipped (GradScaler.step with a non-finite gradient).
extern "C" int pdf_sgd_step(int nchunks, const void *tab, const int *chunks, float lr, float momentum, float weight_decay, const float *found_inf,
                            void *stream) {
    if (nchunks == 0) return PDF_OK;
    if (nchunks < 0 || !tab || !chunks) return PDF_ERR_BAD_ARG;
    k_sgd<<<nchunks, OB, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const SgdTensor *>(tab), reinterpret_cast<const int2 *>(chunks), lr, momentum,
                                                              weight_decay, found_inf);
    return pdf_launch_status();
}

extern "C" int pdf_grad_unscale(int nchunks, const void *tab, const int *chunks, const float *inv_scale, float *found_inf, void *stream) {
    if (nchunks == 0) return PDF_OK;
    if (nchunks < 0 || !tab || !chunks || !inv_scale || !found_inf) return PDF_ERR_BAD_ARG;
    k_unscale<SgdTensor><<<nchunks, OB, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const SgdTensor *>(tab), reinterpret_cast<const int2 *>(chunks), inv_scale,
                                                                  found_inf);
    return pdf_launch_status();
}

extern "C" int pdf_scaler_update(float *scale, float *inv_scale, int *growth_tracker, float *found_inf, float growth_factor, float backoff_factor,
                                 int growth_interval, void *stream) {
    if (!scale || !inv_scale || !growth_tracker || !found_inf || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f) ||
        growth_interval < 1)
        return PDF_ERR_BAD_ARG;
    k_scaler_update<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(scale, inv_scale, growth_tracker, found_inf, growth_factor, backoff_factor, growth_interval);
    return pdf_launch_status();
}

// tab: ntensors x {param*, grad*, exp_avg*, exp_avg_sq*, step*, length, 0, 0} (device, 64 bytes each; step: that tensor's own float32
// step count in device memory, advanced here); chunks as pdf_sgd_step's.  Two launches: the step counts, then the update.
extern "C" int pdf_adam_step(int nchunks, int ntensors, const void *tab, const int *chunks, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int decoupled, const float *found_inf, void *stream) {
    if (nchunks < 0 || ntensors < 0 || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
        !(weight_decay >= 0.0))
        return PDF_ERR_BAD_ARG;
    if (nchunks == 0) return PDF_OK;
    if (!tab || !chunks || ntensors == 0) return PDF_ERR_BAD_ARG;
    k_adam_tick<<<(ntensors + OB - 1) / OB, OB, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const AdamTensor *>(tab), ntensors, found_inf);
    k_adam<<<nchunks, OB, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const AdamTensor *>(tab), reinterpret_cast<const int2 *>(chunks), lr, beta1,
                                                               beta2, eps, weight_decay, decoupled != 0, found_inf);
    return pdf_launch_status();
}

extern "C" int pdf_adam_grad_unscale(int nchunks, const void *tab, const int *chunks, const float *inv_scale, float *found_inf, void *stream) {
    if (nchunks == 0) return PDF_OK;
    if (nchunks < 0 || !tab || !chunks || !inv_scale || !found_inf) return PDF_ERR_BAD_ARG;
    k_unscale<AdamTensor><<<nchunks, OB, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const AdamTensor *>(tab), reinterpret_cast<const int2 *>(chunks),
                                                                              inv_scale, found_inf);
    return pdf_launch_status();
}
