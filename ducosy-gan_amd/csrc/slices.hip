// Slice-series kernels of the resident inference path (generate.py --pipeline resident,
// modules/inference.py::translate_volume_device) on gfx950: the map from the two Generators'
// outputs to stored values fused with the HU-range merge (translate_merge) or with the
// enhancement-difference merge (translate_enhance), and the two resizes of series whose slice size
// differs from the network's (antialiased bilinear for images, nearest for masks).
//
// translate_merge and translate_enhance repeat the host's float32 operations one IEEE operation
// per step (inference.stored_from_output, inference.synthesize, inference.synthesize_enhancement),
// and the antialiased resize accumulates acc = acc + x * w in tap order as two roundings, so
// contraction is off for this whole file.
//
// All kernels are HBM-bound streams.  The two merges and the vertical resize pass own one 16-byte
// vector of float32 along x per thread when the row length (the plane size for translate_enhance)
// and the pointers allow it, else one element.  The vertical pass reads its taps straight from global memory (neighbouring outputs
// share the lines, which come from L2); the horizontal pass stages the input segment of a run of
// output columns in LDS.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int ST = 256;                          // threads per block of the streaming kernels
constexpr int HT = 128;                          // output columns per block of the horizontal pass
constexpr int HCAP = HT * 8 + 2 * DCS_RESIZE_MAX_TAPS;  // staged input columns (in/out <= 8)

template <typename T, int N>
struct alignas(sizeof(T) * N) SVec {
    T v[N];
};

// numpy astype of a float32 on the host: truncation toward zero to 32 bits, low 16 kept
template <typename TP>
__device__ __forceinline__ TP to_stored(float v) {
    return (TP)(int32_t)v;
}

template <typename TP, int VEC>
__global__ void __launch_bounds__(ST) translate_merge_kernel(
    const TP* __restrict__ raw, const float* __restrict__ slope, const float* __restrict__ intercept,
    const float* __restrict__ ys, const float* __restrict__ yl, int64_t nvec, int64_t S, float slo, float shi,
    float sspan, float llo, float lhi, float lspan, TP* __restrict__ soft_out, TP* __restrict__ lung_out,
    TP* __restrict__ merged, float* __restrict__ merged_f32) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int64_t z = e / S;
    const float a = slope[z], b = intercept[z];
    using VP = SVec<TP, VEC>;
    using VF = SVec<float, VEC>;
    const VP r = *reinterpret_cast<const VP*>(raw + e);
    const VF s = *reinterpret_cast<const VF*>(ys + e);
    const VF g = *reinterpret_cast<const VF*>(yl + e);
    VP so, lo, mo;
    VF mf;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const float hs = ((s.v[v] + 1.0f) / 2.0f) * sspan + slo;
        const float hl = ((g.v[v] + 1.0f) / 2.0f) * lspan + llo;
        const TP ps = to_stored<TP>(__fdiv_rn(hs - b, a));
        const TP pl = to_stored<TP>(__fdiv_rn(hl - b, a));
        const float hu = (float)r.v[v] * a + b;
        TP m = r.v[v];
        if (hu >= slo && hu <= shi) m = ps;
        if (hu >= llo && hu <= lhi) m = pl;
        so.v[v] = ps;
        lo.v[v] = pl;
        mo.v[v] = m;
        mf.v[v] = (float)m;
    }
    if (soft_out) *reinterpret_cast<VP*>(soft_out + e) = so;
    if (lung_out) *reinterpret_cast<VP*>(lung_out + e) = lo;
    if (merged) *reinterpret_cast<VP*>(merged + e) = mo;
    if (merged_f32) *reinterpret_cast<VF*>(merged_f32 + e) = mf;
}

// inference.synthesize_enhancement for one voxel (the same rule as volume.hip's): r = f32(raw),
// hs / hl the HU of the two translations.  Both comparisons strict; soft tissue first, then lung.
__device__ __forceinline__ float enhance(float r, float hs, float hl, float a, float b, float thr, float min_hu) {
    const float hr = r * a + b;
    const float es = hs - hr, el = hl - hr;
    const bool valid = hr > min_hu;
    float m = r;
    if (es > thr && valid) m = m + __fdiv_rn(es, a);
    if (el > thr && valid) m = m + __fdiv_rn(el, a);
    return m;
}

// translate_merge_kernel's map to stored values, then the enhancement rule on the HU of those
// stored values (what the staged path reads back from its working series).
template <typename TP, int VEC>
__global__ void __launch_bounds__(ST) translate_enhance_kernel(
    const TP* __restrict__ raw, const float* __restrict__ slope, const float* __restrict__ intercept,
    const float* __restrict__ ys, const float* __restrict__ yl, int64_t nvec, int64_t S, float slo, float sspan,
    float llo, float lspan, float thr, float min_hu, TP* __restrict__ soft_out, TP* __restrict__ lung_out,
    float* __restrict__ merged_f32) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int64_t z = e / S;
    const float a = slope[z], b = intercept[z];
    using VP = SVec<TP, VEC>;
    using VF = SVec<float, VEC>;
    const VP r = *reinterpret_cast<const VP*>(raw + e);
    const VF s = *reinterpret_cast<const VF*>(ys + e);
    const VF g = *reinterpret_cast<const VF*>(yl + e);
    VP so, lo;
    VF mf;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const float hs = ((s.v[v] + 1.0f) / 2.0f) * sspan + slo;
        const float hl = ((g.v[v] + 1.0f) / 2.0f) * lspan + llo;
        const TP ps = to_stored<TP>(__fdiv_rn(hs - b, a));
        const TP pl = to_stored<TP>(__fdiv_rn(hl - b, a));
        so.v[v] = ps;
        lo.v[v] = pl;
        mf.v[v] = enhance((float)r.v[v], (float)ps * a + b, (float)pl * a + b, a, b, thr, min_hu);
    }
    if (soft_out) *reinterpret_cast<VP*>(soft_out + e) = so;
    if (lung_out) *reinterpret_cast<VP*>(lung_out + e) = lo;
    *reinterpret_cast<VF*>(merged_f32 + e) = mf;
}

// Horizontal pass of the antialiased resize: one block per run of HT output columns of one row.
// The tables come from the caller, so every index read from them is clamped into the row.
__global__ void __launch_bounds__(HT) resize_aa_h_kernel(const float* __restrict__ in, float* __restrict__ out, int W,
                                                         int ow, int nseg, const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ count,
                                                         const float* __restrict__ wt, int taps) {
    __shared__ float buf[HCAP];
    const int64_t row = (int64_t)(blockIdx.x / (unsigned)nseg);
    const int o0 = (int)(blockIdx.x % (unsigned)nseg) * HT;
    const int o1 = min(o0 + HT, ow) - 1;  // last output column of this block
    const float* __restrict__ src = in + row * W;
    const int lo = min(max(start[o0], 0), W - 1);
    const int hi = min(max(start[o1], 0) + max(count[o1], 0), W);  // one past the last staged column
    const bool staged = hi - lo <= HCAP;
    if (staged)
        for (int p = threadIdx.x; p < hi - lo; p += HT) buf[p] = src[lo + p];
    __syncthreads();
    const int o = o0 + (int)threadIdx.x;
    if (o > o1) return;
    const int x0 = min(max(start[o], 0), W - 1);
    const int n = min(min(max(count[o], 0), taps), W - x0);
    const float* __restrict__ w = wt + (int64_t)o * taps;
    float acc = 0.0f;
    if (staged && x0 >= lo && x0 + n <= hi) {
        for (int t = 0; t < n; ++t) acc = acc + buf[x0 - lo + t] * w[t];
    } else {
        for (int t = 0; t < n; ++t) acc = acc + src[x0 + t] * w[t];
    }
    out[row * ow + o] = acc;
}

// Vertical pass: element e of the [NC][oh][W] output takes its taps at rows start[y] .. of plane e / (oh*W)
template <int VEC>
__global__ void __launch_bounds__(ST) resize_aa_v_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                         int64_t nvec, int H, int oh, int W,
                                                         const int32_t* __restrict__ start,
                                                         const int32_t* __restrict__ count,
                                                         const float* __restrict__ wt, int taps) {
    const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (i >= nvec) return;
    const int64_t e = i * VEC;
    const int64_t rowo = e / W;  // plane * oh + y
    const int x = (int)(e - rowo * W);
    const int64_t plane = rowo / oh;
    const int y = (int)(rowo - plane * oh);
    const int y0 = min(max(start[y], 0), H - 1);
    const int n = min(min(max(count[y], 0), taps), H - y0);
    const float* __restrict__ w = wt + (int64_t)y * taps;
    const float* __restrict__ src = in + (plane * H + y0) * W + x;
    using VF = SVec<float, VEC>;
    VF acc;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc.v[v] = 0.0f;
    for (int t = 0; t < n; ++t) {
        const VF a = *reinterpret_cast<const VF*>(src + (int64_t)t * W);
        const float wk = w[t];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc.v[v] = acc.v[v] + a.v[v] * wk;
    }
    *reinterpret_cast<VF*>(out + e) = acc;
}

// torch 'nearest': src = min(int(floorf(dst * scale)), in - 1) per axis
__global__ void __launch_bounds__(ST) resize_nearest_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int64_t n, int H, int W, int oh, int ow, float sy,
                                                            float sx) {
    const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
    if (e >= n) return;
    const int64_t rowo = e / ow;
    const int x = (int)(e - rowo * ow);
    const int64_t plane = rowo / oh;
    const int y = (int)(rowo - plane * oh);
    const int iy = min((int)floorf((float)y * sy), H - 1);
    const int ix = min((int)floorf((float)x * sx), W - 1);
    out[e] = in[(plane * H + iy) * W + ix];
}

static bool al(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// [NC][H][W] -> [NC][oh][ow]: positive sizes, each below 2^20, a grid of one thread per element fits
static bool resize_dims_ok(int NC, int H, int W, int oh, int ow) {
    const int lim = 1 << 20;
    if (NC <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return false;
    if (NC >= (1 << 30) || H >= lim || W >= lim || oh >= lim || ow >= lim) return false;
    const long double cap = (long double)(1ll << 38);
    return (long double)NC * H * W < cap && (long double)NC * oh * ow < cap && (long double)NC * H * ow < cap;
}
static unsigned sblocks(int64_t n) { return (unsigned)cdiv(n, ST); }

template <typename TP>
static void launch_translate_merge(const void* raw, const float* slope, const float* intercept, const float* ys,
                                   const float* yl, int64_t n, int64_t S, int W, const float* rg, void* so, void* lo,
                                   void* mo, float* mf, hipStream_t s) {
    const bool vec = W % 4 == 0 && al(raw, 8) && al(ys, 16) && al(yl, 16) && al(so, 8) && al(lo, 8) && al(mo, 8) &&
                     al(mf, 16);
    const TP* r = static_cast<const TP*>(raw);
    if (vec)
        hipLaunchKernelGGL((translate_merge_kernel<TP, 4>), dim3(sblocks(n / 4)), dim3(ST), 0, s, r, slope, intercept,
                           ys, yl, n / 4, S, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], static_cast<TP*>(so),
                           static_cast<TP*>(lo), static_cast<TP*>(mo), mf);
    else
        hipLaunchKernelGGL((translate_merge_kernel<TP, 1>), dim3(sblocks(n)), dim3(ST), 0, s, r, slope, intercept, ys,
                           yl, n, S, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], static_cast<TP*>(so),
                           static_cast<TP*>(lo), static_cast<TP*>(mo), mf);
}

template <typename TP>
static void launch_translate_enhance(const void* raw, const float* slope, const float* intercept, const float* ys,
                                     const float* yl, int64_t n, int64_t S, const float* rg, void* so, void* lo,
                                     float* mf, hipStream_t s) {
    const bool vec = S % 4 == 0 && al(raw, 8) && al(ys, 16) && al(yl, 16) && al(so, 8) && al(lo, 8) && al(mf, 16);
    const TP* r = static_cast<const TP*>(raw);
    if (vec)
        hipLaunchKernelGGL((translate_enhance_kernel<TP, 4>), dim3(sblocks(n / 4)), dim3(ST), 0, s, r, slope, intercept,
                           ys, yl, n / 4, S, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], static_cast<TP*>(so),
                           static_cast<TP*>(lo), mf);
    else
        hipLaunchKernelGGL((translate_enhance_kernel<TP, 1>), dim3(sblocks(n)), dim3(ST), 0, s, r, slope, intercept,
                           ys, yl, n, S, rg[0], rg[1], rg[2], rg[3], rg[4], rg[5], static_cast<TP*>(so),
                           static_cast<TP*>(lo), mf);
}

}  // namespace dcs

using namespace dcs;

extern "C" int dcs_vol_translate_merge(const void* raw, int stored_dtype, const float* slope, const float* intercept,
                                       const float* y_soft, const float* y_lung, int D, int H, int W, float soft_lo,
                                       float soft_hi, float soft_span, float lung_lo, float lung_hi, float lung_span,
                                       void* soft_stored, void* lung_stored, void* merged, float* merged_f32,
                                       void* stream) {
    if (!raw || !slope || !intercept || !y_soft || !y_lung) return fail(DCS_E_INVALID, "vol_translate_merge: null pointer");
    if (!soft_stored && !lung_stored && !merged && !merged_f32)
        return fail(DCS_E_INVALID, "vol_translate_merge: no output requested");
    if (D <= 0 || H <= 0 || W <= 0 || D >= (1 << 30) || H >= (1 << 30) || W >= (1 << 30) ||
        (long double)D * H * W >= (long double)(1ll << 38))
        return fail(DCS_E_INVALID, "vol_translate_merge: bad dimensions");
    if (stored_dtype != DCS_VOL_I16 && stored_dtype != DCS_VOL_U16)
        return fail(DCS_E_INVALID, "vol_translate_merge: stored dtype must be int16 or uint16");
    if (!al(raw, 2) || !al(soft_stored, 2) || !al(lung_stored, 2) || !al(merged, 2) || !al(merged_f32, 4) ||
        !al(y_soft, 4) || !al(y_lung, 4) || !al(slope, 4) || !al(intercept, 4))
        return fail(DCS_E_INVALID, "vol_translate_merge: misaligned pointer");
    const void* outs[4] = {soft_stored, lung_stored, merged, merged_f32};
    for (const void* o : outs)
        if (o && (o == raw || o == y_soft || o == y_lung))
            return fail(DCS_E_INVALID, "vol_translate_merge: an output aliases an input");
    const int64_t S = (int64_t)H * W, n = S * D;
    const float rg[6] = {soft_lo, soft_hi, soft_span, lung_lo, lung_hi, lung_span};
    hipStream_t s = as_stream(stream);
    if (stored_dtype == DCS_VOL_I16)
        launch_translate_merge<int16_t>(raw, slope, intercept, y_soft, y_lung, n, S, W, rg, soft_stored, lung_stored,
                                        merged, merged_f32, s);
    else
        launch_translate_merge<uint16_t>(raw, slope, intercept, y_soft, y_lung, n, S, W, rg, soft_stored, lung_stored,
                                         merged, merged_f32, s);
    return check_launch("vol_translate_merge");
}

extern "C" int dcs_vol_translate_enhance(const void* raw, int stored_dtype, const float* slope, const float* intercept,
                                         const float* y_soft, const float* y_lung, int D, int H, int W, float soft_lo,
                                         float soft_span, float lung_lo, float lung_span, float threshold,
                                         float min_hu, void* soft_stored, void* lung_stored, float* merged_f32,
                                         void* stream) {
    if (!raw || !slope || !intercept || !y_soft || !y_lung || !merged_f32)
        return fail(DCS_E_INVALID, "vol_translate_enhance: null pointer");
    if (D <= 0 || H <= 0 || W <= 0 || D >= (1 << 30) || H >= (1 << 30) || W >= (1 << 30) ||
        (long double)D * H * W >= (long double)(1ll << 38))
        return fail(DCS_E_INVALID, "vol_translate_enhance: bad dimensions");
    if (stored_dtype != DCS_VOL_I16 && stored_dtype != DCS_VOL_U16)
        return fail(DCS_E_INVALID, "vol_translate_enhance: stored dtype must be int16 or uint16");
    if (!al(raw, 2) || !al(soft_stored, 2) || !al(lung_stored, 2) || !al(merged_f32, 4) || !al(y_soft, 4) ||
        !al(y_lung, 4) || !al(slope, 4) || !al(intercept, 4))
        return fail(DCS_E_INVALID, "vol_translate_enhance: misaligned pointer");
    const void* outs[3] = {soft_stored, lung_stored, merged_f32};
    for (const void* o : outs)
        if (o && (o == raw || o == y_soft || o == y_lung))
            return fail(DCS_E_INVALID, "vol_translate_enhance: an output aliases an input");
    const int64_t S = (int64_t)H * W, n = S * D;
    const float rg[6] = {soft_lo, soft_span, lung_lo, lung_span, threshold, min_hu};
    hipStream_t s = as_stream(stream);
    if (stored_dtype == DCS_VOL_I16)
        launch_translate_enhance<int16_t>(raw, slope, intercept, y_soft, y_lung, n, S, rg, soft_stored, lung_stored,
                                          merged_f32, s);
    else
        launch_translate_enhance<uint16_t>(raw, slope, intercept, y_soft, y_lung, n, S, rg, soft_stored, lung_stored,
                                           merged_f32, s);
    return check_launch("vol_translate_enhance");
}

extern "C" int dcs_resize_aa(const float* in, float* out, float* tmp, int NC, int H, int W, int oh, int ow,
                             const int32_t* x_start, const int32_t* x_count, const float* x_weights, int x_taps,
                             const int32_t* y_start, const int32_t* y_count, const float* y_weights, int y_taps,
                             void* stream) {
    if (!in || !out || in == out) return fail(DCS_E_INVALID, "resize_aa: null or aliased pointers");
    if (!resize_dims_ok(NC, H, W, oh, ow)) return fail(DCS_E_INVALID, "resize_aa: bad dimensions");
    const bool horiz = W != ow, vert = H != oh;
    if (!horiz && !vert) return fail(DCS_E_INVALID, "resize_aa: equal sizes (nothing to resize)");
    if ((int64_t)W > 8 * (int64_t)ow || (int64_t)H > 8 * (int64_t)oh)
        return fail(DCS_E_INVALID, "resize_aa: in/out above 8 is not supported");
    if (horiz && (!x_start || !x_count || !x_weights || x_taps < 1 || x_taps > DCS_RESIZE_MAX_TAPS))
        return fail(DCS_E_INVALID, "resize_aa: bad horizontal tables");
    if (vert && (!y_start || !y_count || !y_weights || y_taps < 1 || y_taps > DCS_RESIZE_MAX_TAPS))
        return fail(DCS_E_INVALID, "resize_aa: bad vertical tables");
    if (horiz && vert && (!tmp || tmp == in || tmp == out))
        return fail(DCS_E_INVALID, "resize_aa: a separate [NC][H][ow] buffer is required when both axes change");
    if (!al(in, 4) || !al(out, 4) || !al(tmp, 4) || !al(x_start, 4) || !al(x_count, 4) || !al(x_weights, 4) ||
        !al(y_start, 4) || !al(y_count, 4) || !al(y_weights, 4))
        return fail(DCS_E_INVALID, "resize_aa: misaligned pointer");
    const int nseg = (int)cdiv(ow, HT);
    if (horiz && (long double)NC * H * nseg >= (long double)(1ll << 31))
        return fail(DCS_E_INVALID, "resize_aa: too many rows");
    hipStream_t s = as_stream(stream);
    const float* mid = in;
    if (horiz) {
        float* h_out = vert ? tmp : out;
        hipLaunchKernelGGL(resize_aa_h_kernel, dim3((unsigned)((int64_t)NC * H * nseg)), dim3(HT), 0, s, in, h_out, W,
                           ow, nseg, x_start, x_count, x_weights, x_taps);
        mid = h_out;
    }
    if (vert) {
        const int64_t n = (int64_t)NC * oh * ow;
        if (ow % 4 == 0 && al(mid, 16) && al(out, 16))
            hipLaunchKernelGGL(resize_aa_v_kernel<4>, dim3(sblocks(n / 4)), dim3(ST), 0, s, mid, out, n / 4, H, oh, ow,
                               y_start, y_count, y_weights, y_taps);
        else
            hipLaunchKernelGGL(resize_aa_v_kernel<1>, dim3(sblocks(n)), dim3(ST), 0, s, mid, out, n, H, oh, ow,
                               y_start, y_count, y_weights, y_taps);
    }
    return check_launch("resize_aa");
}

extern "C" int dcs_resize_nearest(const float* in, float* out, int NC, int H, int W, int oh, int ow, void* stream) {
    if (!in || !out || in == out) return fail(DCS_E_INVALID, "resize_nearest: null or aliased pointers");
    if (!resize_dims_ok(NC, H, W, oh, ow)) return fail(DCS_E_INVALID, "resize_nearest: bad dimensions");
    if (!al(in, 4) || !al(out, 4)) return fail(DCS_E_INVALID, "resize_nearest: misaligned pointer");
    const int64_t n = (int64_t)NC * oh * ow;
    const float sy = (float)((double)H / oh), sx = (float)((double)W / ow);
    hipLaunchKernelGGL(resize_nearest_kernel, dim3(sblocks(n)), dim3(ST), 0, as_stream(stream), in, out, n, H, W, oh,
                       ow, sy, sx);
    return check_launch("resize_nearest");
}
