// Training augmentation of raw scenes for gfx950 -- the per-point half of the PDF configs' `data.train.transform` lists
// (pointcept/datasets/transform.py: CenterShift 147-161, RandomRotate 227-261, RandomScale 303-315, RandomFlip 318-334, RandomJitter
// 337-352, ChromaticAutoContrast 376-394, ChromaticTranslation 397-407, ChromaticJitter 410-423, HueSaturationTranslation 642-707,
// RandomColorDrop 710-724, ElasticDistortion 727-785, PositiveShift 138-144, NormalizeColor 112-123) for a whole batch of scenes.
//
// Working buffers are fp64 (N,3) rows.  NumPy's dtype of an array changes per scene with which steps fired (RandomRotate's np.dot with
// a float64 matrix promotes float32 coordinates), so the host keeps each scene's current dtype and every op row carries it: a float32
// array is reproduced by rounding through float after every NumPy statement (a double holds every float exactly, and one +, -, *, /
// of two floats rounded double -> float equals the float operation).  Compiled with -ffp-contract=off: every product and sum rounds as
// written, like NumPy's elementwise loops.
//
// Generator: Philox4x64-10 (Salmon et al., SC'11), the function behind numpy.random.Philox.  Per-point draws use key (scene key,
// stream id) and counter = the point's index in its scene, so a scene's draws do not depend on the batch it is in.
#include "pdfops_common.h"

namespace {

constexpr int ROW = 16;          // doubles per (scene, op) row of the parameter table
enum Op {
    OP_CENTER = 1, OP_ROTATE = 2, OP_SCALE = 3, OP_FLIP = 4, OP_JITTER = 5, OP_AUTOCONTRAST = 6, OP_CTRANS = 7, OP_CJITTER = 8,
    OP_HST = 9, OP_CDROP = 10, OP_POSSHIFT = 11, OP_NORMCOLOR = 12,
};
// row slots
constexpr int R_FIRED = 0, R_REC = 11, R_STREAM = 10, R_NF32 = 12, R_KF32 = 13, R_CF32 = 14, R_CODE = 15;
constexpr int NB = 12;           // bounds per scene: coord min (3), coord max (3), colour min (3), colour max (3)
constexpr int BCH = 64;          // workgroups per scene of the bounds pass

__device__ __forceinline__ void mulhilo(unsigned long long a, unsigned long long b, unsigned long long &hi, unsigned long long &lo) {
    lo = a * b;
    hi = __umul64hi(a, b);
}

// Philox4x64-10: ctr (4 words), key (2 words) -> 4 words
__host__ __device__ __forceinline__ void philox4x64(unsigned long long c[4], unsigned long long k0, unsigned long long k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
        unsigned long long h0, l0, h1, l1;
#ifdef __HIP_DEVICE_COMPILE__
        mulhilo(0xD2E7470EE14C6C93ull, c[0], h0, l0);
        mulhilo(0xCA5A826395121157ull, c[2], h1, l1);
#else
        { unsigned __int128 p = (unsigned __int128)0xD2E7470EE14C6C93ull * c[0]; h0 = (unsigned long long)(p >> 64); l0 = (unsigned long long)p; }
        { unsigned __int128 p = (unsigned __int128)0xCA5A826395121157ull * c[2]; h1 = (unsigned long long)(p >> 64); l1 = (unsigned long long)p; }
#endif
        const unsigned long long n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
    }
}

__device__ __forceinline__ double u53(unsigned long long w) { return (double)(w >> 11) * (1.0 / 9007199254740992.0); }

// three standard normals for point `i` of a scene (Box-Muller in fp64 on the four uniforms of one block)
__device__ __forceinline__ void normals3(unsigned long long key, unsigned long long stream, long i, double z[3]) {
    unsigned long long c[4] = {(unsigned long long)i, 0ull, 0ull, 0ull};
    philox4x64(c, key, stream);
    const double twopi = 6.283185307179586;
    const double r0 = sqrt(-2.0 * log(1.0 - u53(c[0]))), r1 = sqrt(-2.0 * log(1.0 - u53(c[2])));
    z[0] = r0 * cos(twopi * u53(c[1]));
    z[1] = r0 * sin(twopi * u53(c[1]));
    z[2] = r1 * cos(twopi * u53(c[3]));
}

__device__ __forceinline__ double rnd(double x, bool f32) { return f32 ? (double)(float)x : x; }

__device__ __forceinline__ int scene_of(long i, int b, const long long *__restrict__ off) {   // off: (b + 1) starts, off[0] = 0
    int lo = 0, hi = b - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)i >= off[mid]) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long bits_of(double d) { return __builtin_bit_cast(unsigned long long, d); }

// NumPy's float remainder (npy_remainder) with divisor 1: the sign of the divisor, +0 for an exact multiple
__device__ __forceinline__ double rem1(double a) {
    double m = fmod(a, 1.0);
    if (m != 0.0) { if (m < 0.0) m += 1.0; } else m = 0.0;
    return m;
}

template <typename T>
__device__ __forceinline__ void autocontrast(double c[3], const double lo[3], const double hi[3], double bf) {
    const T wa = (T)(1.0 - bf), wb = (T)bf;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const T l = (T)lo[a], scale = (T)255 / (T)((T)hi[a] - l);
        const T contrast = (T)((T)c[a] - l) * scale;
        c[a] = (double)(T)((T)(wa * (T)c[a]) + (T)(wb * contrast));
    }
}

template <typename T>
__device__ __forceinline__ void normcolor(double c[3], int zero_one) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = zero_one ? (double)((T)c[a] / (T)255) : (double)((T)((T)c[a] / (T)127.5) - (T)1);
}

// HueSaturationTranslation on one rgb triple (colour math in fp64, result truncated through uint8 like hsv_to_rgb's astype)
__device__ __forceinline__ void hst(double c[3], double hue_val, double sat_ratio) {
    const double r = c[0], g = c[1], bl = c[2];
    const double maxc = fmax(fmax(r, g), bl), minc = fmin(fmin(r, g), bl);
    const bool mask = maxc != minc;
    const double v = maxc;
    double s = mask ? (maxc - minc) / maxc : 0.0;
    const double rc = mask ? (maxc - r) / (maxc - minc) : 0.0, gc = mask ? (maxc - g) / (maxc - minc) : 0.0,
                 bc = mask ? (maxc - bl) / (maxc - minc) : 0.0;
    double h = r == maxc ? bc - gc : (g == maxc ? 2.0 + rc - bc : 4.0 + gc - rc);
    h = rem1(h / 6.0);
    h = rem1(hue_val + h + 1.0);
    s = sat_ratio * s;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double h6 = h * 6.0;
    int i = (int)(unsigned char)(int)h6;
    const double f = h6 - (double)i;
    const double p = v * (1.0 - s), q = v * (1.0 - s * f), t = v * (1.0 - s * (1.0 - f));
    i = i % 6;
    double o0, o1, o2;
    if (s == 0.0) { o0 = v; o1 = v; o2 = v; }
    else if (i == 1) { o0 = q; o1 = v; o2 = p; }
    else if (i == 2) { o0 = p; o1 = v; o2 = t; }
    else if (i == 3) { o0 = p; o1 = q; o2 = v; }
    else if (i == 4) { o0 = t; o1 = p; o2 = v; }
    else if (i == 5) { o0 = v; o1 = p; o2 = q; }
    else { o0 = v; o1 = t; o2 = p; }
    c[0] = (double)(unsigned char)(int)o0; c[1] = (double)(unsigned char)(int)o1; c[2] = (double)(unsigned char)(int)o2;
}

__device__ __forceinline__ double clip255(double x) { return x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x); }

// One segment of the transform list on every point of every scene.  table: (b, 1 + nop, ROW) doubles; row 0 of a scene holds its
// 64-bit key (bit pattern) in slot 0.  rec (optional): recorded per-point draws, (k, n, 3) doubles, op slot R_REC = k (or -1).
__global__ __launch_bounds__(256) void k_aug_points(int b, long n, const long long *__restrict__ off, int nop, const double *__restrict__ table,
                                                    const double *__restrict__ bounds, const double *__restrict__ rec,
                                                    double *__restrict__ coord, double *__restrict__ color, double *__restrict__ normal) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int s = scene_of(i, b, off);
        const long li = i - off[s];
        const double *srow = table + (long)s * (1 + nop) * ROW;
        const unsigned long long skey = bits_of(srow[0]);
        double c[3] = {0.0, 0.0, 0.0}, k[3] = {0.0, 0.0, 0.0}, nm[3] = {0.0, 0.0, 0.0};
        if (coord) { c[0] = coord[3 * i]; c[1] = coord[3 * i + 1]; c[2] = coord[3 * i + 2]; }
        if (color) { k[0] = color[3 * i]; k[1] = color[3 * i + 1]; k[2] = color[3 * i + 2]; }
        if (normal) { nm[0] = normal[3 * i]; nm[1] = normal[3 * i + 1]; nm[2] = normal[3 * i + 2]; }
        const double *bd = bounds ? bounds + (long)s * NB : nullptr;
        for (int o = 0; o < nop; ++o) {
            const double *p = srow + (long)(1 + o) * ROW;
            if (p[R_FIRED] == 0.0) continue;
            const int code = (int)p[R_CODE];
            const bool cf = p[R_CF32] != 0.0, kf = p[R_KF32] != 0.0, nf = p[R_NF32] != 0.0;
            const int rk = (int)p[R_REC];
            double z[3];
            if (code == OP_JITTER || code == OP_CJITTER) {
                if (rk >= 0 && rec) { const double *rr = rec + ((long)rk * n + i) * 3; z[0] = rr[0]; z[1] = rr[1]; z[2] = rr[2]; }
                else normals3(skey, (unsigned long long)p[R_STREAM], li, z);
            }
            switch (code) {
            case OP_CENTER: {   // shift = [(xmin + xmax) / 2, (ymin + ymax) / 2, zmin or 0] in the coordinate dtype
                const double sx = rnd(rnd(bd[0] + bd[3], cf) / 2.0, cf), sy = rnd(rnd(bd[1] + bd[4], cf) / 2.0, cf);
                const double sz = p[1] != 0.0 ? bd[2] : 0.0;
                c[0] = rnd(c[0] - sx, cf); c[1] = rnd(c[1] - sy, cf); c[2] = rnd(c[2] - sz, cf);
                break;
            }
            case OP_ROTATE: {   // coord -= center (coordinate dtype); coord = coord . R^T (float64); coord += center (float64)
                double ctr[3];
                if (p[4] != 0.0) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) ctr[a] = rnd(rnd(bd[a] + bd[3 + a], cf) / 2.0, cf);
                } else { ctr[0] = p[5]; ctr[1] = p[6]; ctr[2] = p[7]; }
                const double cs = p[1], sn = p[2];
                const int ax = (int)p[3];
                double R[3][3];   // rot_t as upstream builds it
                if (ax == 0) { R[0][0] = 1; R[0][1] = 0; R[0][2] = 0; R[1][0] = 0; R[1][1] = cs; R[1][2] = -sn; R[2][0] = 0; R[2][1] = sn; R[2][2] = cs; }
                else if (ax == 1) { R[0][0] = cs; R[0][1] = 0; R[0][2] = sn; R[1][0] = 0; R[1][1] = 1; R[1][2] = 0; R[2][0] = -sn; R[2][1] = 0; R[2][2] = cs; }
                else { R[0][0] = cs; R[0][1] = -sn; R[0][2] = 0; R[1][0] = sn; R[1][1] = cs; R[1][2] = 0; R[2][0] = 0; R[2][1] = 0; R[2][2] = 1; }
                if (coord) {
                    double d[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) d[a] = rnd(c[a] - ctr[a], cf);
#pragma unroll
                    for (int j = 0; j < 3; ++j) c[j] = (d[0] * R[j][0] + d[1] * R[j][1] + d[2] * R[j][2]) + ctr[j];
                }
                if (normal) {
                    const double m0 = nm[0], m1 = nm[1], m2 = nm[2];
#pragma unroll
                    for (int j = 0; j < 3; ++j) nm[j] = m0 * R[j][0] + m1 * R[j][1] + m2 * R[j][2];
                }
                break;
            }
            case OP_SCALE:
#pragma unroll
                for (int a = 0; a < 3; ++a) c[a] = rnd(c[a] * p[1 + a], cf);
                break;
            case OP_FLIP:
                if (p[1] != 0.0) { c[0] = -c[0]; nm[0] = -nm[0]; }
                if (p[2] != 0.0) { c[1] = -c[1]; nm[1] = -nm[1]; }
                break;
            case OP_JITTER: {
                const double sigma = p[1], cl = p[2];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    double j = sigma * z[a];
                    j = j < -cl ? -cl : (j > cl ? cl : j);
                    c[a] = rnd(c[a] + j, cf);
                }
                break;
            }
            case OP_AUTOCONTRAST:
                if (kf) autocontrast<float>(k, bd + 6, bd + 9, p[1]);
                else autocontrast<double>(k, bd + 6, bd + 9, p[1]);
                break;
            case OP_CTRANS:
#pragma unroll
                for (int a = 0; a < 3; ++a) k[a] = rnd(clip255(p[1 + a] + k[a]), kf);
                break;
            case OP_CJITTER:
#pragma unroll
                for (int a = 0; a < 3; ++a) k[a] = rnd(clip255(z[a] * p[1] + k[a]), kf);
                break;
            case OP_HST:
                hst(k, p[1], p[2]);
                break;
            case OP_CDROP:
#pragma unroll
                for (int a = 0; a < 3; ++a) k[a] = rnd(k[a] * rnd(p[1], kf), kf);
                break;
            case OP_POSSHIFT:
#pragma unroll
                for (int a = 0; a < 3; ++a) c[a] = rnd(c[a] - bd[a], cf);
                break;
            case OP_NORMCOLOR:
                if (kf) normcolor<float>(k, (int)p[1]);
                else normcolor<double>(k, (int)p[1]);
                break;
            default:
                break;
            }
            (void)nf;
        }
        if (coord) { coord[3 * i] = c[0]; coord[3 * i + 1] = c[1]; coord[3 * i + 2] = c[2]; }
        if (color) { color[3 * i] = k[0]; color[3 * i + 1] = k[1]; color[3 * i + 2] = k[2]; }
        if (normal) { normal[3 * i] = nm[0]; normal[3 * i + 1] = nm[1]; normal[3 * i + 2] = nm[2]; }
    }
}

// Segmented min / max, stage 1: workgroup (s, ch) strides over scene s; writes one partial row of NB values.  Order-free: no atomics.
__global__ __launch_bounds__(256) void k_aug_bounds_part(int b, const long long *__restrict__ off, const double *__restrict__ coord,
                                                         const double *__restrict__ color, double *__restrict__ part) {
    const int s = blockIdx.x / BCH, ch = blockIdx.x % BCH;
    double v[NB];
#pragma unroll
    for (int a = 0; a < 3; ++a) { v[a] = INFINITY; v[3 + a] = -INFINITY; v[6 + a] = INFINITY; v[9 + a] = -INFINITY; }
    for (long i = off[s] + (long)ch * 256 + threadIdx.x; i < off[s + 1]; i += (long)BCH * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = coord[3 * i + a];
            v[a] = fmin(v[a], x); v[3 + a] = fmax(v[3 + a], x);
            if (color) { const double y = color[3 * i + a]; v[6 + a] = fmin(v[6 + a], y); v[9 + a] = fmax(v[9 + a], y); }
        }
    }
    __shared__ double red[NB][4];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        double x = v[q];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double y = __shfl_xor(x, o, 64);
            x = (q % 6) < 3 ? fmin(x, y) : fmax(x, y);
        }
        if (pdf_lane() == 0) red[q][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < NB) {
        const int q = threadIdx.x;
        double x = red[q][0];
        for (int w = 1; w < 4; ++w) x = (q % 6) < 3 ? fmin(x, red[q][w]) : fmax(x, red[q][w]);
        part[(long)blockIdx.x * NB + q] = x;
    }
}

__global__ __launch_bounds__(64) void k_aug_bounds_final(int b, const double *__restrict__ part, double *__restrict__ bounds) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= b * NB) return;
    const int s = t / NB, q = t % NB;
    double x = part[((long)s * BCH) * NB + q];
    for (int c = 1; c < BCH; ++c) {
        const double y = part[((long)s * BCH + c) * NB + q];
        x = (q % 6) < 3 ? fmin(x, y) : fmax(x, y);
    }
    bounds[t] = x;
}

__global__ __launch_bounds__(256) void k_philox(long n, unsigned long long k0, unsigned long long k1, unsigned long long c0,
                                                unsigned long long *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        unsigned long long c[4] = {c0 + (unsigned long long)i, 0ull, 0ull, 0ull};
        if (c[0] < c0) c[1] = 1ull;   // carry into the second counter word
        philox4x64(c, k0, k1);
        ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 4 * i);
        o[0] = make_ulonglong2(c[0], c[1]);
        o[1] = make_ulonglong2(c[2], c[3]);
    }
}

// one 64-bit random key per point: word 0 of block (scene key, stream; counter = index in the scene)
__global__ __launch_bounds__(256) void k_aug_keys(int b, long n, const long long *__restrict__ off, const unsigned long long *__restrict__ skeys,
                                                  unsigned long long stream, unsigned long long *__restrict__ out) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int s = scene_of(i, b, off);
        unsigned long long c[4] = {(unsigned long long)(i - off[s]), 0ull, 0ull, 0ull};
        philox4x64(c, skeys[s], stream);
        out[i] = c[0];
    }
}

// GridSample keys on float64 coordinates (voxel_hash.hip for float32): floor(coord / grid_size) in float64, minus the scene's minimum
__global__ __launch_bounds__(256) void k_grid_hash_f64(long n, int b, const double *__restrict__ coord, const int *__restrict__ offset,
                                                       double gx, double gy, double gz, const long long *__restrict__ min_grid,
                                                       long long *__restrict__ grid, unsigned long long *__restrict__ key) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int s = 0;
        while (s < b - 1 && i >= offset[s]) ++s;
        long long g[3] = {(long long)floor(coord[3 * i] / gx), (long long)floor(coord[3 * i + 1] / gy), (long long)floor(coord[3 * i + 2] / gz)};
        unsigned long long h = 14695981039346656037ull;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            g[a] -= min_grid[3 * s + a];
            grid[3 * i + a] = g[a];
            h *= 1099511628211ull;
            h ^= (unsigned long long)g[a];
        }
        key[i] = h;
    }
}


// ---- ElasticDistortion (transform.py:727-785), one (granularity, magnitude) stage.  vinfo (int64): voff (b + 1) voxel starts of the
// scenes' noise volumes, dims (b, 3), aoff (b + 1) starts of the scenes' axes (dx + dy + dz values each).  Volumes are C order
// (dx, dy, dz, 3) float32, like upstream's `np.random.randn(*noise_dim, 3).astype(np.float32)`.
__device__ __forceinline__ int seg_of(long i, int b, const long long *__restrict__ starts) { return scene_of(i, b, starts); }

// float32 standard normals for every voxel: Box-Muller in fp64 on block (scene key, stream; counter = voxel index in the scene)
__global__ __launch_bounds__(256) void k_elastic_noise(int b, long total, const long long *__restrict__ vinfo,
                                                       const unsigned long long *__restrict__ skeys, unsigned long long stream,
                                                       float *__restrict__ vol) {
    for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (long)gridDim.x * blockDim.x) {
        const int s = seg_of(v, b, vinfo);
        double z[3];
        normals3(skeys[s], stream, v - vinfo[s], z);
        vol[3 * v] = (float)z[0]; vol[3 * v + 1] = (float)z[1]; vol[3 * v + 2] = (float)z[2];
    }
}

// one pass of the 3-tap 1/3 box filter along `axis` with zero boundary (scipy.ndimage.convolve, mode="constant"): the weight is the
// float32 1/3, the three products are summed in double in tap order and the sum is rounded to float32
__global__ __launch_bounds__(256) void k_elastic_blur(int b, long total, const long long *__restrict__ vinfo, const float *__restrict__ in,
                                                      float *__restrict__ out, int axis) {
    const double w = (double)(1.0f / 3.0f);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < 3 * total; e += (long)gridDim.x * blockDim.x) {
        const long v = e / 3;
        const int s = seg_of(v, b, vinfo);
        const long long *d = vinfo + (b + 1) + 3 * s;
        const long lv = v - vinfo[s];
        const long iz = lv % d[2], iy = (lv / d[2]) % d[1], ix = lv / (d[2] * d[1]);
        const long pos = axis == 0 ? ix : (axis == 1 ? iy : iz), len = d[axis];
        const long stride = 3 * (axis == 0 ? d[1] * d[2] : (axis == 1 ? d[2] : 1));
        const double a = pos > 0 ? (double)in[e - stride] : 0.0, c = pos + 1 < len ? (double)in[e + stride] : 0.0;
        out[e] = (float)((a * w + (double)in[e] * w) + c * w);
    }
}

// largest i in [0, n - 2] with g[i] <= x (scipy's find_interval_ascending for x inside [g[0], g[n - 1]])
__device__ __forceinline__ int cell_of(const double *__restrict__ g, int n, double x) {
    int lo = 0, hi = n - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// coords += RegularGridInterpolator(axes, vol, linear, fill 0)(coords) * magnitude: the eight corner terms value * ((w0 * w1) * w2) in
// fp64, added in scipy's hypercube order (last axis fastest); the sum rounded to the coordinate dtype.  params (b, 2): fired, float32.
__global__ __launch_bounds__(256) void k_elastic_apply(int b, long n, const long long *__restrict__ off, const long long *__restrict__ vinfo,
                                                       const double *__restrict__ axes, const float *__restrict__ vol,
                                                       const double *__restrict__ params, double magnitude, double *__restrict__ coord,
                                                       double *__restrict__ disp) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int s = scene_of(i, b, off);
        if (params[2 * s] == 0.0) continue;
        const bool cf = params[2 * s + 1] != 0.0;
        const long long *d = vinfo + (b + 1) + 3 * s;
        const double *g[3];
        g[0] = axes + vinfo[4 * b + 1 + s]; g[1] = g[0] + d[0]; g[2] = g[1] + d[1];
        double x[3] = {coord[3 * i], coord[3 * i + 1], coord[3 * i + 2]};
        int idx[3];
        double y[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int na = (int)d[a];
            inside = inside && !(x[a] < g[a][0]) && !(x[a] > g[a][na - 1]);
            idx[a] = cell_of(g[a], na, x[a]);
            y[a] = (x[a] - g[a][idx[a]]) / (g[a][idx[a] + 1] - g[a][idx[a]]);
        }
        double val[3] = {0.0, 0.0, 0.0};
        if (inside) {
            const float *base = vol + 3 * vinfo[s];
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const int u0 = (h >> 2) & 1, u1 = (h >> 1) & 1, u2 = h & 1;
                const double wt = ((u0 ? y[0] : 1.0 - y[0]) * (u1 ? y[1] : 1.0 - y[1])) * (u2 ? y[2] : 1.0 - y[2]);
                const long vox = ((long)(idx[0] + u0) * d[1] + (idx[1] + u1)) * d[2] + (idx[2] + u2);
#pragma unroll
                for (int c = 0; c < 3; ++c) val[c] = val[c] + (double)base[3 * vox + c] * wt;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (disp) disp[3 * i + c] = val[c];
            coord[3 * i + c] = rnd(x[c] + val[c] * magnitude, cf);
        }
    }
}

inline int grid_for(long n) { const long g = (n + 255) / 256; return (int)(g < PDF_MAX_BLOCKS ? (g > 0 ? g : 1) : PDF_MAX_BLOCKS); }

}  // namespace

extern "C" int pdf_philox4x64(long n, long key0, long key1, long ctr0, unsigned long long *out, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || !out) return PDF_ERR_BAD_ARG;
    k_philox<<<grid_for(n), 256, 0, static_cast<hipStream_t>(stream)>>>(n, (unsigned long long)key0, (unsigned long long)key1,
                                                                      (unsigned long long)ctr0, out);
    return pdf_launch_status();
}

extern "C" int pdf_aug_bounds_workspace_doubles(int b) { return b < 0 ? 0 : b * BCH * NB; }

extern "C" int pdf_aug_bounds(int b, const long long *offset, const double *coord, const double *color, double *part, double *bounds,
                              void *stream) {
    if (b == 0) return PDF_OK;
    if (b < 0 || !offset || !coord || !part || !bounds) return PDF_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    k_aug_bounds_part<<<b * BCH, 256, 0, st>>>(b, offset, coord, color, part);
    k_aug_bounds_final<<<pdf_divup((long)b * NB, 64), 64, 0, st>>>(b, part, bounds);
    return pdf_launch_status();
}

extern "C" int pdf_aug_points(int b, long n, const long long *offset, int nop, const double *table, const double *bounds, const double *rec,
                              double *coord, double *color, double *normal, void *stream) {
    if (n == 0 || nop == 0) return PDF_OK;
    if (b < 1 || n < 0 || nop < 0 || !offset || !table || (!coord && !color)) return PDF_ERR_BAD_ARG;
    k_aug_points<<<grid_for(n), 256, 0, static_cast<hipStream_t>(stream)>>>(b, n, offset, nop, table, bounds, rec, coord, color, normal);
    return pdf_launch_status();
}

extern "C" int pdf_aug_keys(int b, long n, const long long *offset, const unsigned long long *scene_keys, long stream_id,
                            unsigned long long *out, void *stream) {
    if (n == 0) return PDF_OK;
    if (b < 1 || n < 0 || !offset || !scene_keys || !out) return PDF_ERR_BAD_ARG;
    k_aug_keys<<<grid_for(n), 256, 0, static_cast<hipStream_t>(stream)>>>(b, n, offset, scene_keys, (unsigned long long)stream_id, out);
    return pdf_launch_status();
}

extern "C" int pdf_grid_hash_f64(long n, int b, const double *coord, const int *offset, double gx, double gy, double gz,
                                 const long long *min_grid, long long *grid, unsigned long long *key, void *stream) {
    if (n == 0) return PDF_OK;
    if (n < 0 || b < 1 || !coord || !offset || !min_grid || !grid || !key || !(gx > 0.0) || !(gy > 0.0) || !(gz > 0.0)) return PDF_ERR_BAD_ARG;
    k_grid_hash_f64<<<grid_for(n), 256, 0, static_cast<hipStream_t>(stream)>>>(n, b, coord, offset, gx, gy, gz, min_grid, grid, key);
    return pdf_launch_status();
}

extern "C" int pdf_aug_elastic_noise(int b, long total, const long long *vinfo, const unsigned long long *scene_keys, long stream_id, float *vol,
                                     void *stream) {
    if (total == 0) return PDF_OK;
    if (b < 1 || total < 0 || !vinfo || !scene_keys || !vol) return PDF_ERR_BAD_ARG;
    k_elastic_noise<<<grid_for(total), 256, 0, static_cast<hipStream_t>(stream)>>>(b, total, vinfo, scene_keys, (unsigned long long)stream_id, vol);
    return pdf_launch_status();
}

extern "C" int pdf_aug_elastic_blur(int b, long total, const long long *vinfo, const float *in, float *out, int axis, void *stream) {
    if (total == 0) return PDF_OK;
    if (b < 1 || total < 0 || !vinfo || !in || !out || in == out || axis < 0 || axis > 2) return PDF_ERR_BAD_ARG;
    k_elastic_blur<<<grid_for(3 * total), 256, 0, static_cast<hipStream_t>(stream)>>>(b, total, vinfo, in, out, axis);
    return pdf_launch_status();
}

extern "C" int pdf_aug_elastic_apply(int b, long n, const long long *offset, const long long *vinfo, const double *axes, const float *vol,
                                     const double *params, double magnitude, double *coord, double *disp, void *stream) {
    if (n == 0) return PDF_OK;
    if (b < 1 || n < 0 || !offset || !vinfo || !axes || !vol || !params || !coord) return PDF_ERR_BAD_ARG;
    k_elastic_apply<<<grid_for(n), 256, 0, static_cast<hipStream_t>(stream)>>>(b, n, offset, vinfo, axes, vol, params, magnitude, coord, disp);
    return pdf_launch_status();
}
