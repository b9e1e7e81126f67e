// PointGroup (PG-v1m1) on the device: the ball table and the clustering of libs/pointgroup_ops, the proposal stage and the bias losses of
// point_group_v1m1_base.py, and the intersection table of InsSegEvaluator.associate_instances.
//
// Ball table (ballquery_batch_p, bfs_cluster_kernel.cu:16-62).  Row p = the points k of p's scene in ascending k with d2 < radius^2 (strict,
// fp32, the as-written expression: pdf_sqdist3), cut after the first 1,000 hits.  CSR instead of the reference's allocate-and-retry loop:
//   k_ball_count : one wave per row over the 27 cells of the per-scene grid of knn_grid.hip (cell >= radius) -> hits (uncapped)
//   k_row_scan   : exclusive scan of min(hits, 1000) in ROW order (one workgroup) -> start_len (n, 2), total (64 bit): the starts are a
//                  function of the input alone (the reference's come from an atomicAdd)
//   k_ball_fill  : one wave per row.  A saturated row first finds T = the 1,000th smallest in-ball index by a radix select over the index
//                  (one byte per walk of the cells, a 256-bin LDS histogram each: 3 walks for a 150k-point scene; no assumption that a
//                  ball fits in LDS); every row then gathers its hits <= T (at most 1,000) into LDS and writes them by rank counting --
//                  ascending index, whatever order the cells hold them in.
// Clustering (bfs_cluster, bfs_cluster.cpp:53-100).  The reference's BFS from every unvisited i in ascending order puts w into the cluster
// of m(w) = min{ i : i reaches w over equal-label edges } ("PointGroup": proof), the least fixed point of
// L(v) = min(v, min over edges u -> v of L(u)).  k_round pushes L(u) along u's out-edges with atomicMin and shortcuts L(u) <- L(L(u))
// (valid: reachability is transitive; hooking ROOTS would compute weak components and is not done).  Labels only decrease and L(w) always
// reaches w, so a stale read inside a launch delays convergence and nothing else.  A round is a launch; "nothing lowered" is the sum of
// the comparisons old > new on the values the atomics RETURN, in the round's own counter; rounds are issued in batches with one host
// read per batch and bounded by n + 1.  Integer atomics only.  The clusters are read off L: class sizes, kept roots (>= threshold),
// rank by a prefix over the root flags (= ascending root index = the reference's order), members in ascending index (a stable sort by
// rank: pdf_serial_sort, driven by the caller).
// Bias losses (point_group_v1m1_base.py:74-86): per-row terms in the promoted type (fp32, or double with a float64 centroid), masked sums
// as the slot sums of slot_sum.h in double.  Nothing to zero, no host read, no float atomics.
#include "knn_grid.h"
#include "slot_sum.h"

namespace pg {
namespace {

constexpr int CAP = 1000;     // bfs_cluster_kernel.cu:22, int idx_temp[1000]
constexpr int WAVES = 4;      // rows per workgroup (one wave each)
constexpr int TB = 256;
constexpr int MAX_BATCH = 64; // rounds per host read, at most
constexpr int LOSS_BLOCKS = 1024;
constexpr int LOSS_HEAD = 4;  // doubles in front of the slots: [1 / denominator, sum l1, sum cosine, count]

// Calls f(hit, index) for the candidates of the ball around (qx, qy, qz), 64 at a time: EVERY lane calls f once per step (hit = false
// for the lanes past the end), so f may ballot.  The three x-cells of a (z, y) row are one range of the cell-sorted copy.
template <typename F>
__device__ __forceinline__ void for_ball(const kg::SceneGrid &g, const unsigned *__restrict__ cell_start, const float4 *__restrict__ sorted,
                                         float qx, float qy, float qz, float r2, int lane, F &&f) {
    const int cx = kg::cell_coord(qx, g.minx, g.inv_h, g.nx), cy = kg::cell_coord(qy, g.miny, g.inv_h, g.ny),
              cz = kg::cell_coord(qz, g.minz, g.inv_h, g.nz);
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = cy + dy, z = cz + dz;
            if (y < 0 || y >= g.ny || z < 0 || z >= g.nz) continue;
            const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
            const int c0 = g.cell_base + (z * g.ny + y) * g.nx + x0;
            const unsigned beg = cell_start[c0], end = cell_start[c0 + (x1 - x0) + 1];
            for (unsigned base = beg; base < end; base += 64) {
                const unsigned p = base + lane;
                bool ok = false;
                int id = -1;
                if (p < end) {
                    const float4 v = sorted[p];
                    id = __float_as_int(v.w);
                    ok = pdf_sqdist3(qx - v.x, qy - v.y, qz - v.z) < r2;
                }
                f(ok, id);
            }
        }
}

__global__ __launch_bounds__(64 * WAVES) void k_ball_count(int n, int b, float radius, const float *__restrict__ xyz, const int *__restrict__ offset,
                                                           const kg::SceneGrid *__restrict__ grids, const unsigned *__restrict__ cell_start,
                                                           const float4 *__restrict__ sorted, int *__restrict__ hits) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= n) return;
    const kg::SceneGrid g = grids[kg::scene_of(q, offset, b)];
    const float qx = xyz[3 * (size_t)q], qy = xyz[3 * (size_t)q + 1], qz = xyz[3 * (size_t)q + 2];
    int cnt = 0;
    for_ball(g, cell_start, sorted, qx, qy, qz, radius * radius, lane,
             [&](bool ok, int) { cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok)); });
    if (lane == 0) hits[q] = cnt;
}

// start_len[q] = {exclusive sum of min(hits, CAP) over the rows before q, min(hits[q], CAP)}; total = the sum over all rows (64 bit:
// a total >= 2^31 is the caller's error to report, the 32-bit starts are then meaningless and never used)
__global__ __launch_bounds__(1024) void k_row_scan(int n, const int *__restrict__ hits, int *__restrict__ start_len, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (int base = 0; base < n; base += 1024 * 4) {
        unsigned v[4];
        unsigned long long sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = base + t * 4 + u;
            v[u] = r < n ? (unsigned)min(max(hits[r], 0), CAP) : 0u;
            sum += v[u];
        }
        unsigned long long inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o, 64);
            if ((t & 63) >= o) inc += up;
        }
        if ((t & 63) == 63) wsum[t >> 6] = inc;
        __syncthreads();
        unsigned long long run = carry + inc - sum;
        for (int w = 0; w < (t >> 6); ++w) run += wsum[w];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = base + t * 4 + u;
            if (r < n) { start_len[2 * (size_t)r] = (int)run; start_len[2 * (size_t)r + 1] = (int)v[u]; }
            run += v[u];
        }
        __syncthreads();
        if (t == 1023) carry = run;
        __syncthreads();
    }
    if (t == 0) total[0] = carry;
}

__global__ __launch_bounds__(64 * WAVES) void k_ball_fill(int n, int b, float radius, long total, const float *__restrict__ xyz,
                                                          const int *__restrict__ offset, const kg::SceneGrid *__restrict__ grids,
                                                          const unsigned *__restrict__ cell_start, const float4 *__restrict__ sorted,
                                                          const int *__restrict__ hits, const int *__restrict__ start_len, int *__restrict__ idx) {
    __shared__ int s_idx[WAVES][CAP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x * WAVES + wave;
    if (q >= n) return;   // wave-uniform, no block barrier below
    int *ci = s_idx[wave];
    const kg::SceneGrid g = grids[kg::scene_of(q, offset, b)];
    const float qx = xyz[3 * (size_t)q], qy = xyz[3 * (size_t)q + 1], qz = xyz[3 * (size_t)q + 2];
    const float r2 = radius * radius;
    const int start = start_len[2 * (size_t)q], len = start_len[2 * (size_t)q + 1];
    if (len <= 0 || start < 0 || (long)start + len > total) return;
    int T = 0x7fffffff;
    if (hits[q] > CAP) {
        // T = the CAP-th smallest in-ball index (indices are unique), by a radix select over the index relative to the scene's start, one byte
        // per walk from the top: histogram (256 LDS counters, in the list's buffer) of the byte over the hits whose higher bytes equal the
        // prefix found so far, then the bucket that holds the want-th of them.  ceil(bits(n_scene) / 8) walks: 3 for a 150k-point scene.
        const int bits = 32 - __builtin_clz((unsigned)(g.n - 1) | 1u);
        unsigned prefix = 0u;
        int want = CAP;   // invariant: at least `want` hits carry the prefix
        bool found = true;
        for (int shift = ((bits - 1) / 8) * 8; shift >= 0 && found; shift -= 8) {
            for (int e = lane; e < 256; e += 64) ci[e] = 0;
            wave_sync();
            const unsigned high = shift + 8 >= 32 ? 0u : ~0u << (shift + 8);
            for_ball(g, cell_start, sorted, qx, qy, qz, r2, lane, [&](bool ok, int id) {
                const unsigned rel = (unsigned)(id - g.start);
                if (ok && (rel & high) == prefix) atomicAdd(&ci[(rel >> shift) & 255u], 1);
            });
            wave_sync();
            int h[4], sum = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) { h[u] = ci[4 * lane + u]; sum += h[u]; }
            int inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            int run = inc - sum, bucket = -1, below = 0;
            if (run < want && want <= inc) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (bucket < 0 && run + h[u] >= want) { bucket = 4 * lane + u; below = run; }
                    run += h[u];
                }
            }
            const unsigned long long who = __builtin_amdgcn_ballot_w64(bucket >= 0);
            found = who != 0ull;   // (always, by the invariant)
            if (found) {
                const int src = __builtin_ctzll(who);
                prefix |= (unsigned)__shfl(bucket, src, 64) << shift;
                want -= __shfl(below, src, 64);
            }
            wave_sync();
        }
        if (found) T = g.start + (int)prefix;
    }
    int cnt = 0;   // wave-uniform
    for_ball(g, cell_start, sorted, qx, qy, qz, r2, lane, [&](bool ok, int id) {
        ok = ok && id <= T;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(ok);
        const int pos = cnt + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (ok && pos < CAP) ci[pos] = id;
        cnt += __builtin_popcountll(mask);
    });
    cnt = min(cnt, CAP);
    wave_sync();
    int *out = idx + start;
    for (int c = lane; c < cnt; c += 64) {   // rank among the gathered indices = position in the row
        const int mine = ci[c];
        int rank = 0;
        for (int o = 0; o < cnt; ++o) rank += ci[o] < mine ? 1 : 0;
        if (rank < len) out[rank] = mine;
    }
}

// ---------------------------------------------------------------------------------------------------------------- clustering
__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(TB) void k_cluster_init(int n, int *__restrict__ L, int *__restrict__ size) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) { L[i] = i; size[i] = 0; }
}

__global__ __launch_bounds__(64) void k_zero_counters(unsigned *__restrict__ c, int k) {
    if ((int)threadIdx.x < k) c[threadIdx.x] = 0u;
}

// One round: row u lowers L(u) to L(L(u)), then lowers L(v) to L(u) for its out-edges u -> v of equal label.  The plain read before an
// atomicMin only SKIPS atomics that cannot lower (a stale value is never smaller than the current one); *lowered counts the atomics whose
// returned value was larger than what they wrote.
__global__ __launch_bounds__(64 * WAVES) void k_round(int n, long total, const int *__restrict__ label, const int *__restrict__ idx,
                                                      const int *__restrict__ start_len, int *__restrict__ L, unsigned *__restrict__ lowered) {
    const int lane = threadIdx.x & 63, u = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= n) return;
    unsigned low = 0;
    int lu = ld(L + u);
    const int r = ld(L + lu);   // (0 <= L <= own index < n, always)
    if (r < lu) {
        if (lane == 0 && atomicMin(L + u, r) > r) ++low;
        lu = r;
    }
    const int lab = label[u], s = start_len[2 * (size_t)u], len = start_len[2 * (size_t)u + 1];
    if (s >= 0 && len > 0 && (long)s + len <= total)
        for (int e = lane; e < len; e += 64) {
            const int v = idx[s + e];
            if ((unsigned)v >= (unsigned)n || label[v] != lab) continue;
            if (ld(L + v) > lu && atomicMin(L + v, lu) > lu) ++low;
        }
    low = pdf_wave_sum(low);
    if (lane == 0 && low) atomicAdd(lowered, low);
}

__global__ __launch_bounds__(TB) void k_class_sizes(int n, const int *__restrict__ L, int *__restrict__ size) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i < n) atomicAdd(size + L[i], 1);
}

// One workgroup, rows in order: flag[r] = keep(r); rank[r] = number of kept r' < r; offs[rank[r]] = sum of their sizes; offs[count] = sum of
// all; info = {count, sum}.  keep(r) = (root[r] == r or root == null) and size[r] >= lo  [clusters: >= threshold; proposals: > points].
__global__ __launch_bounds__(1024) void k_kept_scan(int n, const int *__restrict__ root, const int *__restrict__ size, const int *__restrict__ ends,
                                                    int lo, int *__restrict__ rank, int *__restrict__ offs, long long *__restrict__ info) {
    __shared__ unsigned long long wsum[16];
    __shared__ unsigned long long carry;   // count << 32 | sum (both < 2^31)
    const int t = threadIdx.x;
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int r = base + t;
        int sz = 0;
        bool keep = false;
        if (r < n) {
            sz = ends ? ends[r + 1] - ends[r] : size[r];
            keep = (!root || root[r] == r) && sz >= lo;
        }
        const unsigned long long mine = keep ? (1ull << 32) | (unsigned)sz : 0ull;
        unsigned long long inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o, 64);
            if ((t & 63) >= o) inc += up;
        }
        if ((t & 63) == 63) wsum[t >> 6] = inc;
        __syncthreads();
        unsigned long long run = carry + inc - mine;
        for (int w = 0; w < (t >> 6); ++w) run += wsum[w];
        if (r < n) {
            rank[r] = keep ? (int)(run >> 32) : -1;
            if (keep) offs[run >> 32] = (int)(run & 0xffffffffull);
        }
        __syncthreads();
        if (t == 1023) carry = run + mine;
        __syncthreads();
    }
    if (t == 0) {
        offs[carry >> 32] = (int)(carry & 0xffffffffull);
        info[0] = (long long)(carry >> 32);
        info[1] = (long long)(carry & 0xffffffffull);
    }
}

__global__ __launch_bounds__(TB) void k_cluster_code(int n, const int *__restrict__ L, const int *__restrict__ rank, long long *__restrict__ code) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const int k = rank[L[i]];
    code[i] = k >= 0 ? (long long)k : (long long)n;   // dropped points sort behind every cluster
}

__global__ __launch_bounds__(TB) void k_cluster_fill(long s, long n, const long long *__restrict__ code, const long long *__restrict__ order,
                                                     int *__restrict__ cluster_idxs) {
    const long i = (long)blockIdx.x * TB + threadIdx.x;
    if (i >= s) return;
    const long long w = order[i];
    if (w < 0 || w >= n) return;
    cluster_idxs[2 * i] = (int)code[w];
    cluster_idxs[2 * i + 1] = (int)w;
}

// ---------------------------------------------------------------------------------------------------------------- proposals
// One wave per cluster c with rank[c] = p >= 0: members mapped to the caller's point space (object_idxs), class = label of a member,
// score = mean of prob[member, class] (fp32 values, lane-strided double partial sums in ascending member order, combined by a fixed butterfly).
__global__ __launch_bounds__(64 * WAVES) void k_proposals_fill(int nc, long npts, int k, long ns, const int *__restrict__ cluster_idxs, const int *__restrict__ offs,
                                                               const int *__restrict__ rank, const int *__restrict__ new_offs,
                                                               const int *__restrict__ label, long nobj, const long long *__restrict__ object_idxs,
                                                               const float *__restrict__ prob, int *__restrict__ members, int *__restrict__ prop_of,
                                                               long long *__restrict__ classes, float *__restrict__ scores, int *__restrict__ masks) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (c >= nc) return;
    const int p = rank[c];
    if (p < 0) return;
    const int base = offs[c], cnt = offs[c + 1] - base, out = new_offs[p];
    if (base < 0 || cnt <= 0 || (long)base + cnt > ns) return;   // (offsets that do not describe cluster_idxs)
    const int first = cluster_idxs[2 * (size_t)base + 1];
    const int cls = (first >= 0 && first < nobj) ? label[first] : -1;
    double sum = 0.0;
    for (int e = lane; e < cnt; e += 64) {
        const int m = cluster_idxs[2 * (size_t)(base + e) + 1];
        long o = -1;
        if (m >= 0 && m < nobj) o = object_idxs ? (long)object_idxs[m] : (long)m;
        const bool ok = o >= 0 && o < npts;
        members[out + e] = ok ? (int)o : -1;
        if (!ok) continue;
        prop_of[o] = p;
        if (cls >= 0 && cls < k) sum += (double)prob[o * k + cls];
        if (masks) masks[(size_t)p * npts + o] = 1;
    }
    sum = pdf_wave_sum_f64(sum);
    if (lane == 0) {
        classes[p] = cls;
        scores[p] = (float)(sum / (double)cnt);
    }
}

// ---------------------------------------------------------------------------------------------------------------- intersection table
// Point j of the evaluated cloud lies in proposal p = prop_of[map ? map[j] : j] (or none: -1): table[p, slot[j]] += 1, vert[p] += 1,
// voidc[p] += isvoid[j].  Integer atomics (order-free).
__global__ __launch_bounds__(TB) void k_intersections(long m, long nsrc, int np, int g, const int *__restrict__ prop_of, const long long *__restrict__ map,
                                                      const int *__restrict__ slot, const unsigned char *__restrict__ isvoid, int *__restrict__ table,
                                                      int *__restrict__ vert, int *__restrict__ voidc) {
    const long j = (long)blockIdx.x * TB + threadIdx.x;
    if (j >= m) return;
    const long src = map ? (long)map[j] : j;
    if (src < 0 || src >= nsrc) return;
    const int p = prop_of[src];
    if (p < 0 || p >= np) return;
    atomicAdd(vert + p, 1);
    if (isvoid[j]) atomicAdd(voidc + p, 1);
    const int sl = slot[j];
    if (sl >= 0 && sl < g) atomicAdd(table + (size_t)p * g + sl, 1);
}

// ---------------------------------------------------------------------------------------------------------------- bias losses
__device__ __forceinline__ float tsqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double tsqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float tabs(float v) { return fabsf(v); }
__device__ __forceinline__ double tabs(double v) { return fabs(v); }

// Row i (point_group_v1m1_base.py:74-86, T = the promoted type): gt = centroid - coord; dist = sum |pred - gt|;
// cos = -sum (pred / (|pred| + 1e-8)) * (gt / (|gt| + 1e-8)), the pred factor in fp32 (bias_pred is fp32), the rest in T.
// d1 = mask * sign(pred - gt), d2 = mask * d cos / d pred (0 through |pred| at |pred| = 0, as torch.norm's backward): the unscaled gradients.
template <typename T>
__global__ __launch_bounds__(TB) void k_bias_fwd(long n, const float *__restrict__ pred, const float *__restrict__ coord, const T *__restrict__ centroid,
                                                 const long long *__restrict__ instance, long long ignore, float *__restrict__ d1,
                                                 float *__restrict__ d2, double *__restrict__ acc) {
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (long i = (long)blockIdx.x * TB + threadIdx.x; i < n; i += (long)gridDim.x * TB) {
        const bool on = instance[i] != ignore;
        const float p[3] = {pred[3 * i], pred[3 * i + 1], pred[3 * i + 2]};
        T g[3], diff[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { g[a] = centroid[3 * i + a] - (T)coord[3 * i + a]; diff[a] = (T)p[a] - g[a]; }
        const T dist = tabs(diff[0]) + tabs(diff[1]) + tabs(diff[2]);
        const float pn = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        const T gn = tsqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const float pden = pn + 1e-8f;
        const T gden = gn + (T)1e-8;
        T gu[3], dot = (T)0;
#pragma unroll
        for (int a = 0; a < 3; ++a) { gu[a] = g[a] / gden; dot += (T)(p[a] / pden) * gu[a]; }
        if (on) { s1 += (double)dist; s2 += (double)(-dot); cnt += 1.0; }
        // d(-sum_k p_k / (r + eps) gu_k) / d p_a = -(gu_a / (r + eps) - (p . gu) p_a / (r (r + eps)^2))
        double pg = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) pg += (double)p[a] * (double)gu[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double through_norm = pn > 0.f ? pg * (double)p[a] / ((double)pn * (double)pden * (double)pden) : 0.0;
            d1[3 * i + a] = on ? (diff[a] > (T)0 ? 1.f : (diff[a] < (T)0 ? -1.f : 0.f)) : 0.f;
            d2[3 * i + a] = on ? (float)(-((double)gu[a] / (double)pden - through_norm)) : 0.f;
        }
    }
    double v[3] = {s1, s2, cnt};
    block_sum_by_waves<TB>(v, acc + LOSS_HEAD + 3 * (size_t)blockIdx.x);   // the workgroup's own slot
}

// One workgroup totals the slots (slot_sum.h).  denominator = fp32(sum(mask) + 1e-8) as torch forms it (a 0-dim fp32 tensor plus a
// Python scalar stays fp32, also next to a float64 numerator); loss = {l1, cosine} in T.
template <typename T>
__global__ __launch_bounds__(TB) void k_bias_finish(int blocks, double *__restrict__ acc, T *__restrict__ loss) {
    double t[3];
    if (!slot_total<TB>(acc + LOSS_HEAD, blocks, t)) return;
    const double a = t[0], b = t[1], c = t[2];
    const float denom = (float)c + 1e-8f;
    acc[0] = 1.0 / (double)denom; acc[1] = a; acc[2] = b; acc[3] = c;
    loss[0] = (T)a / (T)denom;
    loss[1] = (T)b / (T)denom;
}

template <typename T>
__global__ __launch_bounds__(TB) void k_bias_bwd(long total, const float *__restrict__ d1, const float *__restrict__ d2, const double *__restrict__ acc,
                                                 const T *__restrict__ gy, float *__restrict__ grad) {
    const double a = (double)gy[0] * acc[0], b = (double)gy[1] * acc[0];
    for (long e = (long)blockIdx.x * TB + threadIdx.x; e < total; e += (long)gridDim.x * TB) grad[e] = (float)((double)d1[e] * a + (double)d2[e] * b);
}

// Cell bound of the ball table's grid.  A neighbour lies less than `radius` away along every axis, so with cells wider than that it sits in
// the 27 cells around the row's cell -- up to the rounding of (v - lo) * inv_h, ~2e-7 relative on each of the two points: 4e-4 of a cell at
// the 1,000 cells an axis can have.  The slack covers it.
inline float min_cell(float radius) { return fmaxf(radius, kg::RQ_MIN_REACH) * 1.001f; }

struct BallWs {
    kg::Layout L;
    size_t hits, total;
};
inline BallWs ball_ws(int b, int n) {
    BallWs w;
    w.L = kg::make_layout(b, n, 0);
    w.hits = w.L.total;
    w.total = kg::al(w.hits + (size_t)n * 4) + 256;
    return w;
}

}  // namespace
}  // namespace pg

extern "C" long pdf_pg_ball_workspace_bytes(int n, int b) {
    if (n < 0 || b < 1 || b > 64) return 0;
    return (long)pg::ball_ws(b, n).total;
}

extern "C" int pdf_pg_ball_count(int n, int b, float radius, const float *xyz, const int *offset, int *start_len, long long *total,
                                 void *workspace, long workspace_bytes, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || b < 1 || !xyz || !offset || !start_len || !total || !workspace || ((uintptr_t)workspace % 256) || !(radius > 0.f)) return PDF_ERR_BAD_ARG;
    if (b > 64) return PDF_ERR_UNSUPPORTED;
    const pg::BallWs w = pg::ball_ws(b, n);
    if (workspace_bytes < (long)w.total) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    const int rc = pdf_grid_build_min_cell(n, xyz, offset, b, pg::min_cell(radius), workspace, (long)w.L.total, stream);
    if (rc != PDF_OK) return rc;
    int *hits = reinterpret_cast<int *>(ws + w.hits);
    pg::k_ball_count<<<pdf_divup(n, pg::WAVES), 64 * pg::WAVES, 0, s>>>(n, b, radius, xyz, offset, reinterpret_cast<kg::SceneGrid *>(ws + w.L.grid),
                                                                       reinterpret_cast<unsigned *>(ws + w.L.cell_start),
                                                                       reinterpret_cast<float4 *>(ws + w.L.sorted), hits);
    pg::k_row_scan<<<1, 1024, 0, s>>>(n, hits, start_len, reinterpret_cast<unsigned long long *>(total));
    return pdf_launch_status();
}

extern "C" int pdf_pg_ball_fill(int n, int b, float radius, const float *xyz, const int *offset, const int *start_len, long total, int *idx,
                                void *workspace, long workspace_bytes, void *stream) {
    if (n == 0 || total == 0) return PDF_OK;
    if (n < 0 || total < 0 || b < 1 || !xyz || !offset || !start_len || !idx || !workspace || ((uintptr_t)workspace % 256) || !(radius > 0.f)) return PDF_ERR_BAD_ARG;
    if (b > 64 || total >= (1L << 31)) return PDF_ERR_UNSUPPORTED;   // start_len is int32 (as upstream)
    const pg::BallWs w = pg::ball_ws(b, n);
    if (workspace_bytes < (long)w.total) return PDF_ERR_BAD_ARG;
    char *ws = static_cast<char *>(workspace);
    pg::k_ball_fill<<<pdf_divup(n, pg::WAVES), 64 * pg::WAVES, 0, static_cast<hipStream_t>(stream)>>>(
        n, b, radius, total, xyz, offset, reinterpret_cast<kg::SceneGrid *>(ws + w.L.grid), reinterpret_cast<unsigned *>(ws + w.L.cell_start),
        reinterpret_cast<float4 *>(ws + w.L.sorted), reinterpret_cast<int *>(ws + w.hits), start_len, idx);
    return pdf_launch_status();
}

extern "C" int pdf_pg_cluster_labels(int n, const int *label, const int *idx, long total, const int *start_len, int threshold, int *L, int *size,
                                     int *rank, int *offs, long long *code, long long *info, unsigned *counters, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || total < 0 || total >= (1L << 31) || !label || (!idx && total > 0) || !start_len || !L || !size || !rank || !offs || !code || !info || !counters)
        return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = pdf_divup(n, pg::TB), rows = pdf_divup(n, pg::WAVES);
    pg::k_cluster_init<<<blocks, pg::TB, 0, s>>>(n, L, size);
    long rounds = 0;
    bool done = false;
    unsigned host[pg::MAX_BATCH];
    for (int batch = 4; !done; batch = batch * 2 < pg::MAX_BATCH ? batch * 2 : pg::MAX_BATCH) {
        if (rounds > (long)n) return PDF_ERR_NOT_CONVERGED;   // n - 1 lowering rounds + the one that finds nothing is the worst case
        pg::k_zero_counters<<<1, 64, 0, s>>>(counters, batch);
        for (int r = 0; r < batch; ++r) pg::k_round<<<rows, 64 * pg::WAVES, 0, s>>>(n, total, label, idx, start_len, L, counters + r);
        hipError_t e = hipMemcpyAsync(host, counters, sizeof(unsigned) * batch, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return (int)e;
        for (int r = 0; r < batch && !done; ++r) {
            ++rounds;
            done = host[r] == 0u;
        }
    }
    pg::k_class_sizes<<<blocks, pg::TB, 0, s>>>(n, L, size);
    pg::k_kept_scan<<<1, 1024, 0, s>>>(n, L, size, nullptr, threshold, rank, offs, info);
    pg::k_cluster_code<<<blocks, pg::TB, 0, s>>>(n, L, rank, code);
    hipError_t e = hipMemcpyAsync(info + 2, &rounds, sizeof(long long), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // (`rounds` lives on this frame)
    return e != hipSuccess ? (int)e : pdf_launch_status();
}

extern "C" int pdf_pg_cluster_fill(long n, long s, const long long *code, const long long *order, int *cluster_idxs, void *stream) {
    if (s == 0) return PDF_OK;
    if (n < 1 || s < 0 || s > n || !code || !order || !cluster_idxs) return PDF_ERR_BAD_ARG;
    pg::k_cluster_fill<<<pdf_divup(s, pg::TB), pg::TB, 0, static_cast<hipStream_t>(stream)>>>(s, n, code, order, cluster_idxs);
    return pdf_launch_status();
}

extern "C" int pdf_pg_proposals_select(int nc, const int *offs, int propose_points, int *rank, int *new_offs, long long *info, void *stream) {
    if (nc < 0 || !offs || !rank || !new_offs || !info || propose_points >= 0x7fffffff) return PDF_ERR_BAD_ARG;
    // (nc == 0 still writes new_offs[0] = 0 and info = {0, 0})
    pg::k_kept_scan<<<1, 1024, 0, static_cast<hipStream_t>(stream)>>>(nc, nullptr, nullptr, offs, propose_points + 1, rank, new_offs, info);
    return pdf_launch_status();
}

extern "C" int pdf_pg_proposals_fill(int nc, long npts, int k, long ns, const int *cluster_idxs, const int *offs, const int *rank, const int *new_offs,
                                     const int *label, long nobj, const long long *object_idxs, const float *prob, int *members, int *prop_of,
                                     long long *classes, float *scores, int *masks, void *stream) {
    if (nc == 0) return PDF_OK;
    if (nc < 0 || npts < 1 || npts >= (1L << 31) || k < 1 || ns < 1 || nobj < 1 || !cluster_idxs || !offs || !rank || !new_offs || !label || !prob || !members
        || !prop_of || !classes || !scores)
        return PDF_ERR_BAD_ARG;
    pg::k_proposals_fill<<<pdf_divup(nc, pg::WAVES), 64 * pg::WAVES, 0, static_cast<hipStream_t>(stream)>>>(
        nc, npts, k, ns, cluster_idxs, offs, rank, new_offs, label, nobj, object_idxs, prob, members, prop_of, classes, scores, masks);
    return pdf_launch_status();
}

extern "C" int pdf_pg_intersections(long m, long nsrc, int np, int g, const int *prop_of, const long long *map, const int *slot,
                                    const unsigned char *isvoid, int *table, int *vert, int *voidc, void *stream) {
    if (m == 0 || np == 0) return PDF_OK;
    if (m < 0 || nsrc < 1 || np < 0 || g < 0 || !prop_of || !slot || !isvoid || (!table && g > 0) || !vert || !voidc) return PDF_ERR_BAD_ARG;
    pg::k_intersections<<<pdf_divup(m, pg::TB), pg::TB, 0, static_cast<hipStream_t>(stream)>>>(m, nsrc, np, g, prop_of, map, slot, isvoid, table, vert, voidc);
    return pdf_launch_status();
}

extern "C" long pdf_pg_bias_loss_workspace_doubles(void) { return pg::LOSS_HEAD + 3L * pg::LOSS_BLOCKS; }

extern "C" int pdf_pg_bias_loss_forward(long n, const float *pred, const float *coord, const void *centroid, int centroid_f64,
                                        const long long *instance, long long ignore, float *d1, float *d2, double *acc, void *loss, void *stream) {
    if (n < 0 || !acc || !loss || (n > 0 && (!pred || !coord || !centroid || !instance || !d1 || !d2))) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = n == 0 ? 0 : (int)(pdf_divup(n, pg::TB) < pg::LOSS_BLOCKS ? pdf_divup(n, pg::TB) : pg::LOSS_BLOCKS);
    if (centroid_f64) {
        if (blocks) pg::k_bias_fwd<double><<<blocks, pg::TB, 0, s>>>(n, pred, coord, static_cast<const double *>(centroid), instance, ignore, d1, d2, acc);
        pg::k_bias_finish<double><<<1, pg::TB, 0, s>>>(blocks, acc, static_cast<double *>(loss));
    } else {
        if (blocks) pg::k_bias_fwd<float><<<blocks, pg::TB, 0, s>>>(n, pred, coord, static_cast<const float *>(centroid), instance, ignore, d1, d2, acc);
        pg::k_bias_finish<float><<<1, pg::TB, 0, s>>>(blocks, acc, static_cast<float *>(loss));
    }
    return pdf_launch_status();
}

extern "C" int pdf_pg_bias_loss_backward(long n, const float *d1, const float *d2, const double *acc, const void *gy, int f64, float *grad,
                                         void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || !d1 || !d2 || !acc || !gy || !grad) return PDF_ERR_BAD_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long total = 3 * n;
    const int blocks = (int)(pdf_divup(total, pg::TB) < PDF_MAX_BLOCKS ? pdf_divup(total, pg::TB) : PDF_MAX_BLOCKS);
    if (f64) pg::k_bias_bwd<double><<<blocks, pg::TB, 0, s>>>(total, d1, d2, acc, static_cast<const double *>(gy), grad);
    else pg::k_bias_bwd<float><<<blocks, pg::TB, 0, s>>>(total, d1, d2, acc, static_cast<const float *>(gy), grad);
    return pdf_launch_status();
}
