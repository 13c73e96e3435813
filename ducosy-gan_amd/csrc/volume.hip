// Volume post-processing of generate.py's synthesis stage on gfx950 (modules/postprocess.py and
// modules/inference.py::synthesize / smooth_volume on the host): separable Gaussian along one
// axis, z median, z Kalman, exact min/max, the fused unsharp mask + threshold restore + int16
// cast, the HU-range merge and the enhancement-difference merge (synthesize_enhancement).  Dense
// [D][H][W] volumes, x fastest.
//
// Every kernel reproduces the host arithmetic bit for bit: scipy's correlate1d (symmetric
// weights) runs in double as  tmp = x[l]*w[r];  tmp += (x[l+ii] + x[l-ii]) * w[ii+r]  for
// ii = -r..-1, and stores in the array's dtype; numpy's elementwise chain is one IEEE operation
// per step.  Neither contracts a multiply and an add, so contraction is off for this whole file.
//
// All kernels are HBM-bound streams: one thread owns one 16-byte vector of the input along x
// (4 float, 2 double, 8 int16) when W allows it and the pointers are aligned, else one element.
// The z and y passes read their 2r+1 taps straight from global memory: the taps of neighbouring
// outputs are the same lines, so they come from L2 / Infinity Cache and HBM sees the input about
// once.  The x pass stages a row segment and its halo in LDS.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int VT = 256;            // threads per block of the streaming kernels
constexpr int XT = 128;            // threads per block of the x pass
constexpr int XHALO = DCS_VOL_MAX_RADIUS;

template <typename T, int N>
struct alignas(sizeof(T) * N) Vec {
    T v[N];
};

struct GaussW {
    double w[DCS_VOL_MAX_RADIUS + 1];  // w[0..r]: the first r+1 weights, w[r] the centre
};

// scipy 'reflect' (half-sample symmetric, d c b a | a b c d | d c b a), repeated for any i
__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// Gaussian along z (S = H*W, L = D) or y (S = W, L = H): element e of the flat volume lies at
// position (e / S) % L of its line, and its taps at e + (p - l) * S.
template <typename TI, typename TO, int VEC>
__global__ void __launch_bounds__(VT) gauss_strided_kernel(const TI* __restrict__ in, TO* __restrict__ out,
                                                           int64_t nvec, int L, int64_t S, int r, GaussW gw) {
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int l = (int)((e / S) % L);
    using VI = Vec<TI, VEC>;
    const VI c = *reinterpret_cast<const VI*>(in + e);
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = (double)c.v[v] * gw.w[r];
    for (int k = 0; k < r; ++k) {
        const int ii = k - r;
        const VI a = *reinterpret_cast<const VI*>(in + (e + (int64_t)(reflect_idx(l + ii, L) - l) * S));
        const VI b = *reinterpret_cast<const VI*>(in + (e + (int64_t)(reflect_idx(l - ii, L) - l) * S));
        const double wk = gw.w[k];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += ((double)a.v[v] + (double)b.v[v]) * wk;
    }
    Vec<TO, VEC> o;
#pragma unroll
    for (int v = 0; v < VEC; ++v) o.v[v] = (TO)acc[v];
    *reinterpret_cast<Vec<TO, VEC>*>(out + e) = o;
}

// Gaussian along x: one block per segment of XT*VEC elements of one row; the segment and r
// reflected elements on each side are staged in LDS as the input type.
template <typename TI, typename TO, int VEC>
__global__ void __launch_bounds__(XT) gauss_x_kernel(const TI* __restrict__ in, TO* __restrict__ out, int W,
                                                     int nseg, int r, GaussW gw) {
    constexpr int SEG = XT * VEC;
    __shared__ alignas(16) TI buf[SEG + 2 * XHALO];
    const int64_t row = (int64_t)(blockIdx.x / (unsigned)nseg);
    const int x0 = (int)(blockIdx.x % (unsigned)nseg) * SEG;
    const TI* __restrict__ src = in + row * W;
    const int xend = min(x0 + SEG, W);  // one past the last element this block writes
    const int xt = x0 + (int)threadIdx.x * VEC;
    using VI = Vec<TI, VEC>;
    if (xt < xend)  // W % VEC == 0 on the vector path: the whole vector lies inside the row
        *reinterpret_cast<VI*>(&buf[XHALO + threadIdx.x * VEC]) = *reinterpret_cast<const VI*>(src + xt);
    for (int p = threadIdx.x; p < SEG + 2 * XHALO; p += XT) {
        const int x = x0 - XHALO + p;
        if (x < x0 - r || x >= xend + r || (x >= x0 && x < xend)) continue;
        buf[p] = src[reflect_idx(x, W)];
    }
    __syncthreads();
    if (xt >= xend) return;
    const int l = XHALO + (int)threadIdx.x * VEC;
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = (double)buf[l + v] * gw.w[r];
    for (int k = 0; k < r; ++k) {
        const int ii = k - r;
        const double wk = gw.w[k];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += ((double)buf[l + v + ii] + (double)buf[l + v - ii]) * wk;
    }
    Vec<TO, VEC> o;
#pragma unroll
    for (int v = 0; v < VEC; ++v) o.v[v] = (TO)acc[v];
    *reinterpret_cast<Vec<TO, VEC>*>(out + row * W + xt) = o;
}

// z median of odd size K (rank K/2), reflect boundary: insertion sort of the K taps in registers
template <int K, int VEC>
__global__ void __launch_bounds__(VT) median_z_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      int64_t nvec, int D, int64_t S) {
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int l = (int)(e / S);
    using VF = Vec<float, VEC>;
    float t[VEC][K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const VF a = *reinterpret_cast<const VF*>(in + (e + (int64_t)(reflect_idx(l + k - K / 2, D) - l) * S));
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v][k] = a.v[v];
    }
    VF o;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
#pragma unroll
        for (int a = 1; a < K; ++a)
#pragma unroll
            for (int b = a; b > 0; --b) {
                const float lo = fminf(t[v][b - 1], t[v][b]), hi = fmaxf(t[v][b - 1], t[v][b]);
                t[v][b - 1] = lo;
                t[v][b] = hi;
            }
        o.v[v] = t[v][K / 2];
    }
    *reinterpret_cast<VF*>(out + e) = o;
}

// scalar Kalman filter along z for every column: x = x + gain[k] * (z[k] - x), x0 = z[0], double
template <int VEC>
__global__ void __launch_bounds__(VT) kalman_z_kernel(const float* __restrict__ in, const double* __restrict__ gain,
                                                      double* __restrict__ out, int D, int64_t S) {
    const int64_t e = ((int64_t)blockIdx.x * VT + threadIdx.x) * VEC;
    if (e >= S) return;
    using VF = Vec<float, VEC>;
    using VD = Vec<double, VEC>;
    VD x;
    {
        const VF z0 = *reinterpret_cast<const VF*>(in + e);
#pragma unroll
        for (int v = 0; v < VEC; ++v) x.v[v] = (double)z0.v[v];
    }
    for (int k = 0; k < D; ++k) {
        const VF z = *reinterpret_cast<const VF*>(in + (e + (int64_t)k * S));
        const double g = gain[k];
#pragma unroll
        for (int v = 0; v < VEC; ++v) x.v[v] = x.v[v] + g * ((double)z.v[v] - x.v[v]);
        *reinterpret_cast<VD*>(out + (e + (int64_t)k * S)) = x;
    }
}

// exact min / max of a float array (finite values): per-block partials, then one block folds them
__global__ void __launch_bounds__(VT) minmax_part_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
    __shared__ float smn[VT / WAVE], smx[VT / WAVE];
    float mn = INFINITY, mx = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * VT;
    const int64_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * VT + threadIdx.x; i < n; i += stride) {
        mn = fminf(mn, x[i]);
        mx = fmaxf(mx, x[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VT / WAVE; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
        }
        part[2 * blockIdx.x] = mn;
        part[2 * blockIdx.x + 1] = mx;
    }
}

__global__ void __launch_bounds__(VT) minmax_fold_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out) {
    __shared__ float smn[VT / WAVE], smx[VT / WAVE];
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += VT) {
        mn = fminf(mn, part[2 * i]);
        mx = fmaxf(mx, part[2 * i + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn;
        smx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < VT / WAVE; ++w) {
            mn = fminf(mn, smn[w]);
            mx = fmaxf(mx, smx[w]);
        }
        out[0] = mn;
        out[1] = mx;
    }
}

// numpy astype(int16) of a double on the host: truncation toward zero to 32 bits, low 16 kept
__device__ __forceinline__ int16_t to_i16(double v) { return (int16_t)(int32_t)v; }

// unsharp_mask + threshold restore + int16 (postprocess_ct_volume's tail), elementwise in the
// host's operation order.  UNSHARP = false: restore + cast only.
template <typename TS, int VEC, bool UNSHARP>
__global__ void __launch_bounds__(VT) finish_kernel(const TS* __restrict__ sm, const double* __restrict__ blur_sm,
                                                    const double* __restrict__ blur_og,
                                                    const float* __restrict__ orig, const float* __restrict__ mm,
                                                    int64_t nvec, double one_minus_amount, double amount, float thr,
                                                    int16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const Vec<TS, VEC> s = *reinterpret_cast<const Vec<TS, VEC>*>(sm + e);
    const Vec<float, VEC> og = *reinterpret_cast<const Vec<float, VEC>*>(orig + e);
    Vec<double, VEC> bs, bo;
    double lo = 0.0, hi = 0.0;
    if (UNSHARP) {
        bs = *reinterpret_cast<const Vec<double, VEC>*>(blur_sm + e);
        bo = *reinterpret_cast<const Vec<double, VEC>*>(blur_og + e);
        lo = (double)mm[0];
        hi = (double)mm[1];
    }
    Vec<int16_t, VEC> o;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        double r = (double)s.v[v];
        if (UNSHARP) {
            const double g = (double)og.v[v];
            const double detail = one_minus_amount * (r - bs.v[v]) + amount * (g - bo.v[v]);
            r = r + detail * amount;
            r = r < lo ? lo : r;
            r = r > hi ? hi : r;
        }
        if (og.v[v] >= thr) r = (double)og.v[v];
        o.v[v] = to_i16(r);
    }
    *reinterpret_cast<Vec<int16_t, VEC>*>(out + e) = o;
}

// HU-range merge (inference.synthesize on every slice): hu = f32(raw) * slope[z] + intercept[z]
// as two float32 roundings; soft range first, lung second; both bounds inclusive.
template <typename TP, int VEC>
__global__ void __launch_bounds__(VT) merge_kernel(const TP* __restrict__ raw, const TP* __restrict__ soft,
                                                   const TP* __restrict__ lung, const float* __restrict__ slope,
                                                   const float* __restrict__ intercept, int64_t nvec, int64_t S,
                                                   float slo, float shi, float llo, float lhi,
                                                   TP* __restrict__ out, float* __restrict__ out_f32) {
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int64_t z = e / S;
    const float a = slope[z], b = intercept[z];
    using VP = Vec<TP, VEC>;
    const VP r = *reinterpret_cast<const VP*>(raw + e);
    const VP s = *reinterpret_cast<const VP*>(soft + e);
    const VP g = *reinterpret_cast<const VP*>(lung + e);
    VP o;
    Vec<float, VEC> f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const float hu = (float)r.v[v] * a + b;
        TP m = r.v[v];
        if (hu >= slo && hu <= shi) m = s.v[v];
        if (hu >= llo && hu <= lhi) m = g.v[v];
        o.v[v] = m;
        f.v[v] = (float)m;
    }
    if (out) *reinterpret_cast<VP*>(out + e) = o;
    if (out_f32) *reinterpret_cast<Vec<float, VEC>*>(out_f32 + e) = f;
}

// Enhancement-difference merge (inference.synthesize_enhancement on every slice), float32, one
// IEEE operation per step: the NCCT value plus each translation's HU gain over it, where that gain
// exceeds thr and the NCCT HU exceeds min_hu (both strict); soft tissue first, then lung.
template <typename TP, int VEC>
__global__ void __launch_bounds__(VT) merge_enhance_kernel(const TP* __restrict__ raw, const TP* __restrict__ soft,
                                                           const TP* __restrict__ lung,
                                                           const float* __restrict__ slope,
                                                           const float* __restrict__ intercept, int64_t nvec,
                                                           int64_t S, float thr, float min_hu,
                                                           float* __restrict__ out_f32) {
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int64_t z = e / S;
    const float a = slope[z], b = intercept[z];
    using VP = Vec<TP, VEC>;
    const VP r = *reinterpret_cast<const VP*>(raw + e);
    const VP s = *reinterpret_cast<const VP*>(soft + e);
    const VP g = *reinterpret_cast<const VP*>(lung + e);
    Vec<float, VEC> f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const float rv = (float)r.v[v];
        const float hr = rv * a + b;
        const float es = ((float)s.v[v] * a + b) - hr;
        const float el = ((float)g.v[v] * a + b) - hr;
        const bool valid = hr > min_hu;
        float m = rv;
        if (es > thr && valid) m = m + __fdiv_rn(es, a);
        if (el > thr && valid) m = m + __fdiv_rn(el, a);
        f.v[v] = m;
    }
    *reinterpret_cast<Vec<float, VEC>*>(out_f32 + e) = f;
}

static bool aligned(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// dims accepted by every volume entry point: positive, each < 2^30 (reflect_idx doubles one),
// and few enough elements that a grid of one thread per element fits
static bool dims_ok(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0 || D >= (1 << 30) || H >= (1 << 30) || W >= (1 << 30)) return false;
    return (long double)D * H * W < (long double)(1ll << 38);
}
static unsigned blocks_for(int64_t n) { return (unsigned)cdiv(n, VT); }

template <typename TI, typename TO>
static void launch_gauss(const void* in, void* out, int D, int H, int W, int axis, int r, const GaussW& gw,
                         hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(TI);
    const int64_t n = (int64_t)D * H * W;
    const bool vec = W % VEC == 0 && aligned(in, sizeof(TI) * VEC) && aligned(out, sizeof(TO) * VEC);
    const TI* i = static_cast<const TI*>(in);
    TO* o = static_cast<TO*>(out);
    if (axis == 2) {
        const int64_t rows = (int64_t)D * H;
        if (vec) {
            const int nseg = (int)cdiv(W, XT * VEC);
            hipLaunchKernelGGL((gauss_x_kernel<TI, TO, VEC>), dim3((unsigned)(rows * nseg)), dim3(XT), 0, s, i, o, W,
                               nseg, r, gw);
        } else {
            const int nseg = (int)cdiv(W, XT);
            hipLaunchKernelGGL((gauss_x_kernel<TI, TO, 1>), dim3((unsigned)(rows * nseg)), dim3(XT), 0, s, i, o, W,
                               nseg, r, gw);
        }
        return;
    }
    const int L = axis == 0 ? D : H;
    const int64_t S = axis == 0 ? (int64_t)H * W : (int64_t)W;
    if (vec)
        hipLaunchKernelGGL((gauss_strided_kernel<TI, TO, VEC>), dim3(blocks_for(n / VEC)), dim3(VT), 0, s, i, o,
                           n / VEC, L, S, r, gw);
    else
        hipLaunchKernelGGL((gauss_strided_kernel<TI, TO, 1>), dim3(blocks_for(n)), dim3(VT), 0, s, i, o, n, L, S, r,
                           gw);
}

template <int K>
static void launch_median(const float* in, float* out, int64_t n, int D, int64_t S, bool vec, hipStream_t s) {
    if (vec)
        hipLaunchKernelGGL((median_z_kernel<K, 4>), dim3(blocks_for(n / 4)), dim3(VT), 0, s, in, out, n / 4, D, S);
    else
        hipLaunchKernelGGL((median_z_kernel<K, 1>), dim3(blocks_for(n)), dim3(VT), 0, s, in, out, n, D, S);
}

template <typename TS, bool UNSHARP>
static void launch_finish(const void* sm, const double* bs, const double* bo, const float* orig, const float* mm,
                          int64_t n, double oma, double amount, float thr, int16_t* out, hipStream_t s) {
    const bool vec = n % 4 == 0 && aligned(sm, sizeof(TS) * 4) && aligned(bs, 32) && aligned(bo, 32) &&
                     aligned(orig, 16) && aligned(out, 8);
    const TS* p = static_cast<const TS*>(sm);
    if (vec)
        hipLaunchKernelGGL((finish_kernel<TS, 4, UNSHARP>), dim3(blocks_for(n / 4)), dim3(VT), 0, s, p, bs, bo, orig,
                           mm, n / 4, oma, amount, thr, out);
    else
        hipLaunchKernelGGL((finish_kernel<TS, 1, UNSHARP>), dim3(blocks_for(n)), dim3(VT), 0, s, p, bs, bo, orig, mm,
                           n, oma, amount, thr, out);
}

template <typename TP>
static void launch_merge(const void* raw, const void* soft, const void* lung, const float* slope,
                         const float* intercept, int64_t n, int64_t S, float slo, float shi, float llo, float lhi,
                         void* out, float* out_f32, hipStream_t s) {
    const bool vec = S % 8 == 0 && aligned(raw, 16) && aligned(soft, 16) && aligned(lung, 16) && aligned(out, 16) &&
                     aligned(out_f32, 32);
    const TP *r = static_cast<const TP*>(raw), *so = static_cast<const TP*>(soft), *lu = static_cast<const TP*>(lung);
    if (vec)
        hipLaunchKernelGGL((merge_kernel<TP, 8>), dim3(blocks_for(n / 8)), dim3(VT), 0, s, r, so, lu, slope,
                           intercept, n / 8, S, slo, shi, llo, lhi, static_cast<TP*>(out), out_f32);
    else
        hipLaunchKernelGGL((merge_kernel<TP, 1>), dim3(blocks_for(n)), dim3(VT), 0, s, r, so, lu, slope, intercept, n,
                           S, slo, shi, llo, lhi, static_cast<TP*>(out), out_f32);
}

// one 16-byte float vector of the output per thread: 4 stored values (8 bytes) of each input
template <typename TP>
static void launch_merge_enhance(const void* raw, const void* soft, const void* lung, const float* slope,
                                 const float* intercept, int64_t n, int64_t S, float thr, float min_hu, float* out_f32,
                                 hipStream_t s) {
    const bool vec = S % 4 == 0 && aligned(raw, 8) && aligned(soft, 8) && aligned(lung, 8) && aligned(out_f32, 16);
    const TP *r = static_cast<const TP*>(raw), *so = static_cast<const TP*>(soft), *lu = static_cast<const TP*>(lung);
    if (vec)
        hipLaunchKernelGGL((merge_enhance_kernel<TP, 4>), dim3(blocks_for(n / 4)), dim3(VT), 0, s, r, so, lu, slope,
                           intercept, n / 4, S, thr, min_hu, out_f32);
    else
        hipLaunchKernelGGL((merge_enhance_kernel<TP, 1>), dim3(blocks_for(n)), dim3(VT), 0, s, r, so, lu, slope,
                           intercept, n, S, thr, min_hu, out_f32);
}

}  // namespace dcs

using namespace dcs;

extern "C" int dcs_vol_gauss1d(const void* in, int in_dtype, void* out, int out_dtype, int D, int H, int W, int axis,
                               int radius, const double* weights, void* stream) {
    if (!in || !out || !weights || in == out) return fail(DCS_E_INVALID, "vol_gauss1d: null or aliased pointers");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "vol_gauss1d: bad dimensions");
    if (axis < 0 || axis > 2) return fail(DCS_E_INVALID, "vol_gauss1d: axis must be 0 (z), 1 (y) or 2 (x)");
    if (radius < 0 || radius > DCS_VOL_MAX_RADIUS) return fail(DCS_E_INVALID, "vol_gauss1d: radius must be in [0, 16]");
    const bool ff = in_dtype == DCS_VOL_F32 && out_dtype == DCS_VOL_F32;
    const bool fd = in_dtype == DCS_VOL_F32 && out_dtype == DCS_VOL_F64;
    const bool dd = in_dtype == DCS_VOL_F64 && out_dtype == DCS_VOL_F64;
    if (!ff && !fd && !dd) return fail(DCS_E_INVALID, "vol_gauss1d: dtypes must be f32->f32, f32->f64 or f64->f64");
    if (!aligned(in, in_dtype == DCS_VOL_F32 ? 4 : 8) || !aligned(out, out_dtype == DCS_VOL_F32 ? 4 : 8))
        return fail(DCS_E_INVALID, "vol_gauss1d: misaligned pointer");
    if (axis == 2 && (long double)D * H * cdiv(W, XT) >= (long double)(1ll << 31))
        return fail(DCS_E_INVALID, "vol_gauss1d: too many rows");
    GaussW gw;
    for (int k = 0; k <= DCS_VOL_MAX_RADIUS; ++k) gw.w[k] = k <= radius ? weights[k] : 0.0;
    hipStream_t s = as_stream(stream);
    if (ff)
        launch_gauss<float, float>(in, out, D, H, W, axis, radius, gw, s);
    else if (fd)
        launch_gauss<float, double>(in, out, D, H, W, axis, radius, gw, s);
    else
        launch_gauss<double, double>(in, out, D, H, W, axis, radius, gw, s);
    return check_launch("vol_gauss1d");
}

extern "C" int dcs_vol_median_z(const float* in, float* out, int D, int H, int W, int k, void* stream) {
    if (!in || !out || in == out) return fail(DCS_E_INVALID, "vol_median_z: null or aliased pointers");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "vol_median_z: bad dimensions");
    if (k < 1 || k > DCS_VOL_MAX_MEDIAN || (k & 1) == 0)
        return fail(DCS_E_INVALID, "vol_median_z: kernel size must be odd and at most 9");
    if (!aligned(in, 4) || !aligned(out, 4)) return fail(DCS_E_INVALID, "vol_median_z: misaligned pointer");
    const int64_t S = (int64_t)H * W, n = S * D;
    const bool vec = S % 4 == 0 && aligned(in, 16) && aligned(out, 16);
    hipStream_t s = as_stream(stream);
    switch (k) {
        case 1: launch_median<1>(in, out, n, D, S, vec, s); break;
        case 3: launch_median<3>(in, out, n, D, S, vec, s); break;
        case 5: launch_median<5>(in, out, n, D, S, vec, s); break;
        case 7: launch_median<7>(in, out, n, D, S, vec, s); break;
        default: launch_median<9>(in, out, n, D, S, vec, s); break;
    }
    return check_launch("vol_median_z");
}

extern "C" int dcs_vol_kalman_z(const float* in, const double* gain, double* out, int D, int H, int W, void* stream) {
    if (!in || !gain || !out) return fail(DCS_E_INVALID, "vol_kalman_z: null pointer");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "vol_kalman_z: bad dimensions");
    if (!aligned(in, 4) || !aligned(out, 8) || !aligned(gain, 8))
        return fail(DCS_E_INVALID, "vol_kalman_z: misaligned pointer");
    const int64_t S = (int64_t)H * W;
    hipStream_t s = as_stream(stream);
    if (S % 4 == 0 && aligned(in, 16) && aligned(out, 32))
        hipLaunchKernelGGL(kalman_z_kernel<4>, dim3(blocks_for(S / 4)), dim3(VT), 0, s, in, gain, out, D, S);
    else
        hipLaunchKernelGGL(kalman_z_kernel<1>, dim3(blocks_for(S)), dim3(VT), 0, s, in, gain, out, D, S);
    return check_launch("vol_kalman_z");
}

extern "C" int dcs_vol_minmax(const float* x, int64_t n, float* out, float* ws, void* stream) {
    if (!x || !out || !ws) return fail(DCS_E_INVALID, "vol_minmax: null pointer");
    if (n <= 0 || n >= (1ll << 38)) return fail(DCS_E_INVALID, "vol_minmax: bad element count");
    if (!aligned(x, 4) || !aligned(out, 4) || !aligned(ws, 4)) return fail(DCS_E_INVALID, "vol_minmax: misaligned pointer");
    const int parts = (int)(cdiv(n, VT * 4) < DCS_VOL_MINMAX_PARTS ? cdiv(n, VT * 4) : DCS_VOL_MINMAX_PARTS);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(minmax_part_kernel, dim3((unsigned)parts), dim3(VT), 0, s, x, n, ws);
    hipLaunchKernelGGL(minmax_fold_kernel, dim3(1), dim3(VT), 0, s, ws, parts, out);
    return check_launch("vol_minmax");
}

extern "C" int dcs_vol_unsharp_finish(const void* sm, int sm_dtype, const double* blur_sm, const double* blur_og,
                                      const float* original, const float* minmax, int64_t n, double one_minus_amount,
                                      double amount, float hu_threshold, int16_t* out, void* stream) {
    if (!sm || !blur_sm || !blur_og || !original || !minmax || !out)
        return fail(DCS_E_INVALID, "vol_unsharp_finish: null pointer");
    if (n <= 0 || n >= (1ll << 38)) return fail(DCS_E_INVALID, "vol_unsharp_finish: bad element count");
    if (sm_dtype != DCS_VOL_F32 && sm_dtype != DCS_VOL_F64) return fail(DCS_E_INVALID, "vol_unsharp_finish: bad dtype");
    if (!aligned(sm, sm_dtype == DCS_VOL_F32 ? 4 : 8) || !aligned(blur_sm, 8) || !aligned(blur_og, 8) ||
        !aligned(original, 4) || !aligned(minmax, 4) || !aligned(out, 2))
        return fail(DCS_E_INVALID, "vol_unsharp_finish: misaligned pointer");
    hipStream_t s = as_stream(stream);
    if (sm_dtype == DCS_VOL_F32)
        launch_finish<float, true>(sm, blur_sm, blur_og, original, minmax, n, one_minus_amount, amount, hu_threshold,
                                   out, s);
    else
        launch_finish<double, true>(sm, blur_sm, blur_og, original, minmax, n, one_minus_amount, amount, hu_threshold,
                                    out, s);
    return check_launch("vol_unsharp_finish");
}

extern "C" int dcs_vol_finish(const void* sm, int sm_dtype, const float* original, int64_t n, float hu_threshold,
                              int16_t* out, void* stream) {
    if (!sm || !original || !out) return fail(DCS_E_INVALID, "vol_finish: null pointer");
    if (n <= 0 || n >= (1ll << 38)) return fail(DCS_E_INVALID, "vol_finish: bad element count");
    if (sm_dtype != DCS_VOL_F32 && sm_dtype != DCS_VOL_F64) return fail(DCS_E_INVALID, "vol_finish: bad dtype");
    if (!aligned(sm, sm_dtype == DCS_VOL_F32 ? 4 : 8) || !aligned(original, 4) || !aligned(out, 2))
        return fail(DCS_E_INVALID, "vol_finish: misaligned pointer");
    hipStream_t s = as_stream(stream);
    if (sm_dtype == DCS_VOL_F32)
        launch_finish<float, false>(sm, nullptr, nullptr, original, nullptr, n, 0.0, 0.0, hu_threshold, out, s);
    else
        launch_finish<double, false>(sm, nullptr, nullptr, original, nullptr, n, 0.0, 0.0, hu_threshold, out, s);
    return check_launch("vol_finish");
}

extern "C" int dcs_vol_merge(const void* raw, const void* soft, const void* lung, int stored_dtype, const float* slope,
                             const float* intercept, int D, int H, int W, float soft_lo, float soft_hi, float lung_lo,
                             float lung_hi, void* out, float* out_f32, void* stream) {
    if (!raw || !soft || !lung || !slope || !intercept || (!out && !out_f32))
        return fail(DCS_E_INVALID, "vol_merge: null pointer");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "vol_merge: bad dimensions");
    if (stored_dtype != DCS_VOL_I16 && stored_dtype != DCS_VOL_U16)
        return fail(DCS_E_INVALID, "vol_merge: stored dtype must be int16 or uint16");
    if (!aligned(raw, 2) || !aligned(soft, 2) || !aligned(lung, 2) || !aligned(out, 2) || !aligned(out_f32, 4) ||
        !aligned(slope, 4) || !aligned(intercept, 4))
        return fail(DCS_E_INVALID, "vol_merge: misaligned pointer");
    const int64_t S = (int64_t)H * W, n = S * D;
    hipStream_t s = as_stream(stream);
    if (stored_dtype == DCS_VOL_I16)
        launch_merge<int16_t>(raw, soft, lung, slope, intercept, n, S, soft_lo, soft_hi, lung_lo, lung_hi, out, out_f32,
                              s);
    else
        launch_merge<uint16_t>(raw, soft, lung, slope, intercept, n, S, soft_lo, soft_hi, lung_lo, lung_hi, out,
                               out_f32, s);
    return check_launch("vol_merge");
}

extern "C" int dcs_vol_merge_enhance(const void* raw, const void* soft, const void* lung, int stored_dtype,
                                     const float* slope, const float* intercept, int D, int H, int W, float threshold,
                                     float min_hu, float* out_f32, void* stream) {
    if (!raw || !soft || !lung || !slope || !intercept || !out_f32)
        return fail(DCS_E_INVALID, "vol_merge_enhance: null pointer");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "vol_merge_enhance: bad dimensions");
    if (stored_dtype != DCS_VOL_I16 && stored_dtype != DCS_VOL_U16)
        return fail(DCS_E_INVALID, "vol_merge_enhance: stored dtype must be int16 or uint16");
    if (!aligned(raw, 2) || !aligned(soft, 2) || !aligned(lung, 2) || !aligned(out_f32, 4) || !aligned(slope, 4) ||
        !aligned(intercept, 4))
        return fail(DCS_E_INVALID, "vol_merge_enhance: misaligned pointer");
    if (out_f32 == raw || out_f32 == soft || out_f32 == lung)
        return fail(DCS_E_INVALID, "vol_merge_enhance: the output aliases an input");
    const int64_t S = (int64_t)H * W, n = S * D;
    hipStream_t s = as_stream(stream);
    if (stored_dtype == DCS_VOL_I16)
        launch_merge_enhance<int16_t>(raw, soft, lung, slope, intercept, n, S, threshold, min_hu, out_f32, s);
    else
        launch_merge_enhance<uint16_t>(raw, soft, lung, slope, intercept, n, S, threshold, min_hu, out_f32, s);
    return check_launch("vol_merge_enhance");
}
