// The passes of the difference-map stage between the U-Net's convolutions on gfx950 (modules/nmodel
// on the host: the normal-map U-Net run one slice at a time, then modules/postprocess.py::
// apply_diffmap): HU normalisation, folded BatchNorm + ReLU + 2x2 max pool, bilinear x2 upsample
// with the skip's pad split, and the tail (1x1 projection, denormalisation, threshold, uint8 cast,
// add into the merged volume).  Activations are NHWC float32; the 3x3 convolutions themselves run
// on the rows pass (conv.hip).
//
// The normalisation and the tail reproduce the host's numpy chain bit for bit: one IEEE float32
// operation per step, so contraction is off for this whole file.
//
// All kernels are HBM-bound streams: one thread owns one 16-byte vector of 4 channels (or 4
// pixels of a one-channel volume); every store is a vector store to an address no other thread
// writes, so results do not depend on the launch.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int UT = 256;  // threads per block

static bool aligned_to(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }
static unsigned ublocks(int64_t n) { return (unsigned)cdiv(n, UT); }
constexpr int64_t MAX_THREADS = (int64_t)1 << 38;  // one thread per vector: the grid stays below 2^31 blocks

// numpy's clip keeps a NaN; the two divisions and the multiply are single float32 roundings
__device__ __forceinline__ float normalize_hu(float v) {
    v = v < -1024.f ? -1024.f : (v > 3071.f ? 3071.f : v);
    v = (v + 1024.f) / 4095.f;
    return v * 2.f - 1.f;
}

template <int VEC>
__global__ void __launch_bounds__(UT) normalize_dense_kernel(const float* __restrict__ hu, int64_t nvec,
                                                             float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= nvec) return;
    if (VEC == 4) {
        float4 v = reinterpret_cast<const float4*>(hu)[i];
        v.x = normalize_hu(v.x);
        v.y = normalize_hu(v.y);
        v.z = normalize_hu(v.z);
        v.w = normalize_hu(v.w);
        reinterpret_cast<float4*>(out)[i] = v;
    } else {
        out[i] = normalize_hu(hu[i]);
    }
}

__global__ void __launch_bounds__(UT) normalize_c4_kernel(const float* __restrict__ hu, int64_t n,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= n) return;
    reinterpret_cast<float4*>(out)[i] = make_float4(normalize_hu(hu[i]), 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float4 affine_relu4(const float4& v, const float4& sc, const float4& sh) {
    float4 a;
    a.x = v.x * sc.x + sh.x;
    a.y = v.y * sc.y + sh.y;
    a.z = v.z * sc.z + sh.z;
    a.w = v.w * sc.w + sh.w;
    a.x = a.x > 0.f ? a.x : 0.f;
    a.y = a.y > 0.f ? a.y : 0.f;
    a.z = a.z > 0.f ? a.z : 0.f;
    a.w = a.w > 0.f ? a.w : 0.f;
    return a;
}

// One thread: 4 channels of one 2x2 quad of y (the quads cover ceil(H/2) x ceil(W/2), so an odd
// last row / column is read and written to skip but forms no pooled pixel).
__global__ void __launch_bounds__(UT) affine_relu_pool_kernel(const float* __restrict__ y,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int64_t nthreads,
                                                              int H, int W, int C, float* __restrict__ skip,
                                                              int skip_cstride, float* __restrict__ pooled) {
    const int64_t i = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= nthreads) return;
    const int C4 = C >> 2, Hq = (H + 1) >> 1, Wq = (W + 1) >> 1, Hp = H >> 1, Wp = W >> 1;
    const int c = (int)(i % C4) * 4;
    int64_t r = i / C4;
    const int qx = (int)(r % Wq);
    r /= Wq;
    const int qy = (int)(r % Hq);
    const int64_t n = r / Hq;
    const float4 sc = *reinterpret_cast<const float4*>(scale + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + c);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);  // relu output: 0 is the identity of the maximum
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int h = 2 * qy + dy;
        if (h >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int w = 2 * qx + dx;
            if (w >= W) continue;
            const int64_t pix = (n * H + h) * W + w;
            const float4 a = affine_relu4(*reinterpret_cast<const float4*>(y + pix * C + c), sc, sh);
            *reinterpret_cast<float4*>(skip + pix * skip_cstride + c) = a;
            m.x = fmaxf(m.x, a.x);
            m.y = fmaxf(m.y, a.y);
            m.z = fmaxf(m.z, a.z);
            m.w = fmaxf(m.w, a.w);
        }
    }
    if (qy < Hp && qx < Wp)
        *reinterpret_cast<float4*>(pooled + ((n * Hp + qy) * Wp + qx) * C + c) = m;
}

// One thread: 4 channels of one output pixel.  ry / rx: float32(in - 1) / float32(2 in - 1), 0 for
// a 1-pixel axis; AFFINE: the source is read as relu(x * scale + shift).
template <bool AFFINE>
__global__ void __launch_bounds__(UT) upsample2_pad_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int64_t nthreads, int h,
                                                           int w, int C, int Ho, int Wo, int pt, int pl, float ry,
                                                           float rx, float* __restrict__ out, int out_cstride) {
    const int64_t i = (int64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= nthreads) return;
    const int C4 = C >> 2;
    const int c = (int)(i % C4) * 4;
    int64_t r = i / C4;
    const int X = (int)(r % Wo);
    r /= Wo;
    const int Y = (int)(r % Ho);
    const int64_t n = r / Ho;
    float4* dst = reinterpret_cast<float4*>(out + ((n * Ho + Y) * Wo + X) * out_cstride + c);
    const int uy = Y - pt, ux = X - pl;
    if (uy < 0 || uy >= 2 * h || ux < 0 || ux >= 2 * w) {
        *dst = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float sy = ry * (float)uy, sx = rx * (float)ux;
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 > h - 1 ? h - 1 : y0;
    x0 = x0 > w - 1 ? w - 1 : x0;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = sy - (float)y0, lx1 = sx - (float)x0;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* base = x + n * h * w * C + c;
    float4 a00 = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * w + x0) * C);
    float4 a01 = *reinterpret_cast<const float4*>(base + ((int64_t)y0 * w + x1) * C);
    float4 a10 = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * w + x0) * C);
    float4 a11 = *reinterpret_cast<const float4*>(base + ((int64_t)y1 * w + x1) * C);
    if (AFFINE) {
        const float4 sc = *reinterpret_cast<const float4*>(scale + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c);
        a00 = affine_relu4(a00, sc, sh);
        a01 = affine_relu4(a01, sc, sh);
        a10 = affine_relu4(a10, sc, sh);
        a11 = affine_relu4(a11, sc, sh);
    }
    float4 o;
    o.x = ly0 * (lx0 * a00.x + lx1 * a01.x) + ly1 * (lx0 * a10.x + lx1 * a11.x);
    o.y = ly0 * (lx0 * a00.y + lx1 * a01.y) + ly1 * (lx0 * a10.y + lx1 * a11.y);
    o.z = ly0 * (lx0 * a00.z + lx1 * a01.z) + ly1 * (lx0 * a10.z + lx1 * a11.z);
    o.w = ly0 * (lx0 * a00.w + lx1 * a01.w) + ly1 * (lx0 * a10.w + lx1 * a11.w);
    *dst = o;
}

// numpy astype(uint8) of a float32 on the host: truncation toward zero to 32 bits, low 8 kept
__device__ __forceinline__ float diff_as_u8(float d, float thr) {
    const float m = d < thr ? 0.f : d;
    return (float)(uint8_t)(int32_t)m;
}

// LP lanes: one pixel, each lane C / LP consecutive channels (64 bytes a lane at LP = C / 16, so a
// wave reads whole lines); the lanes' partial sums are added by an xor butterfly, the same value in
// every lane and the same from run to run.  PROJ: d comes from the last conv output (affine + ReLU,
// 1x1 projection, denormalize_diff); else from diff_in (LP = 1).
template <bool PROJ, int LP>
__global__ void __launch_bounds__(UT) out_diffmap_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const float* __restrict__ wproj, float bias, int64_t P, int C,
                                                         float thr, const float* __restrict__ diff_in,
                                                         const float* vol_in, float* vol_out,
                                                         float* __restrict__ diff_out) {
    const int64_t t = (int64_t)blockIdx.x * UT + threadIdx.x;
    const int64_t p = t / LP;
    const bool live = p < P;  // a lane past the end still takes part in the butterfly
    float d;
    if (PROJ) {
        const int CL = C / LP, c0 = (int)(t % LP) * CL;
        float acc = 0.f;
        if (live) {
            const float* row = y + p * C;
            for (int c = c0; c < c0 + CL; c += 4) {
                const float4 a = affine_relu4(*reinterpret_cast<const float4*>(row + c),
                                              *reinterpret_cast<const float4*>(scale + c),
                                              *reinterpret_cast<const float4*>(shift + c));
                const float4 wv = *reinterpret_cast<const float4*>(wproj + c);
                acc = acc + a.x * wv.x;
                acc = acc + a.y * wv.y;
                acc = acc + a.z * wv.z;
                acc = acc + a.w * wv.w;
            }
        }
#pragma unroll
        for (int o = LP / 2; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
        if (!live || (LP > 1 && t % LP != 0)) return;
        d = (acc + bias + 1.f) / 2.f * 4000.f;
        if (diff_out) diff_out[p] = d;
    } else {
        if (!live) return;
        d = diff_in[p];
    }
    if (vol_in) vol_out[p] = vol_in[p] + diff_as_u8(d, thr);
}

template <int LP>
static void launch_out_proj(const float* y, const float* scale, const float* shift, const float* w, float bias,
                            int64_t P, int C, float thr, const float* vol_in, float* vol_out, float* diff,
                            hipStream_t s) {
    hipLaunchKernelGGL((out_diffmap_kernel<true, LP>), dim3(ublocks(P * LP)), dim3(UT), 0, s, y, scale, shift, w, bias,
                       P, C, thr, (const float*)nullptr, vol_in, vol_out, diff);
}

}  // namespace dcs

using namespace dcs;

extern "C" int dcs_unet_normalize_hu(const float* hu, int64_t n, int cstride, float* out, void* stream) {
    if (!hu || !out || hu == out) return fail(DCS_E_INVALID, "unet_normalize_hu: null or aliased pointers");
    if (n <= 0 || n >= MAX_THREADS) return fail(DCS_E_INVALID, "unet_normalize_hu: bad element count");
    if (cstride != 1 && cstride != 4) return fail(DCS_E_INVALID, "unet_normalize_hu: cstride must be 1 or 4");
    if (!aligned_to(hu, 4) || !aligned_to(out, cstride == 4 ? 16 : 4))
        return fail(DCS_E_INVALID, "unet_normalize_hu: misaligned pointer");
    hipStream_t s = as_stream(stream);
    if (cstride == 4)
        hipLaunchKernelGGL(normalize_c4_kernel, dim3(ublocks(n)), dim3(UT), 0, s, hu, n, out);
    else if (n % 4 == 0 && aligned_to(hu, 16) && aligned_to(out, 16))
        hipLaunchKernelGGL(normalize_dense_kernel<4>, dim3(ublocks(n / 4)), dim3(UT), 0, s, hu, n / 4, out);
    else
        hipLaunchKernelGGL(normalize_dense_kernel<1>, dim3(ublocks(n)), dim3(UT), 0, s, hu, n, out);
    return check_launch("unet_normalize_hu");
}

// N, H, W, C of an NHWC activation: positive, C % 4 == 0, few enough vectors for one grid
static bool act_dims_ok(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return false;
    return (long double)N * H * W * C < (long double)MAX_THREADS;
}

extern "C" int dcs_unet_affine_relu_pool(const float* y, const float* scale, const float* shift, int N, int H, int W,
                                         int C, float* skip, int skip_cstride, float* pooled, void* stream) {
    if (!y || !scale || !shift || !skip || !pooled) return fail(DCS_E_INVALID, "unet_affine_relu_pool: null pointer");
    if (!act_dims_ok(N, H, W, C)) return fail(DCS_E_INVALID, "unet_affine_relu_pool: bad dimensions (C % 4 == 0)");
    if (skip_cstride < C || skip_cstride % 4 != 0 || (long double)N * H * W * skip_cstride >= (long double)MAX_THREADS)
        return fail(DCS_E_INVALID, "unet_affine_relu_pool: skip_cstride must be >= C and a multiple of 4");
    if (H < 2 || W < 2) return fail(DCS_E_INVALID, "unet_affine_relu_pool: nothing to pool (H, W >= 2)");
    if (y == skip || y == pooled || skip == pooled) return fail(DCS_E_INVALID, "unet_affine_relu_pool: aliased pointers");
    if (!aligned_to(y, 16) || !aligned_to(scale, 16) || !aligned_to(shift, 16) || !aligned_to(skip, 16) ||
        !aligned_to(pooled, 16))
        return fail(DCS_E_INVALID, "unet_affine_relu_pool: pointers must be 16-byte aligned");
    const int64_t nthreads = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    hipLaunchKernelGGL(affine_relu_pool_kernel, dim3(ublocks(nthreads)), dim3(UT), 0, as_stream(stream), y, scale,
                       shift, nthreads, H, W, C, skip, skip_cstride, pooled);
    return check_launch("unet_affine_relu_pool");
}

extern "C" int dcs_unet_upsample2_pad(const float* x, const float* scale, const float* shift, int N, int h, int w,
                                      int C, int Ho, int Wo, float* out, int out_cstride, void* stream) {
    if (!x || !out || x == out) return fail(DCS_E_INVALID, "unet_upsample2_pad: null or aliased pointers");
    if ((scale == nullptr) != (shift == nullptr))
        return fail(DCS_E_INVALID, "unet_upsample2_pad: scale and shift come together");
    if (!act_dims_ok(N, h, w, C) || h >= (1 << 29) || w >= (1 << 29))
        return fail(DCS_E_INVALID, "unet_upsample2_pad: bad dimensions (C % 4 == 0)");
    if (Ho < 2 * h || Wo < 2 * w) return fail(DCS_E_INVALID, "unet_upsample2_pad: the target is smaller than 2h x 2w");
    if (out_cstride < C || out_cstride % 4 != 0 || !act_dims_ok(N, Ho, Wo, out_cstride))
        return fail(DCS_E_INVALID, "unet_upsample2_pad: out_cstride must be >= C and a multiple of 4");
    if (!aligned_to(x, 16) || !aligned_to(scale, 16) || !aligned_to(shift, 16) || !aligned_to(out, 16))
        return fail(DCS_E_INVALID, "unet_upsample2_pad: pointers must be 16-byte aligned");
    const int64_t nthreads = (int64_t)N * Ho * Wo * (C / 4);
    const int pt = (Ho - 2 * h) / 2, pl = (Wo - 2 * w) / 2;
    const float ry = h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.f;
    const float rx = w > 1 ? (float)(w - 1) / (float)(2 * w - 1) : 0.f;
    hipStream_t s = as_stream(stream);
    if (scale)
        hipLaunchKernelGGL(upsample2_pad_kernel<true>, dim3(ublocks(nthreads)), dim3(UT), 0, s, x, scale, shift,
                           nthreads, h, w, C, Ho, Wo, pt, pl, ry, rx, out, out_cstride);
    else
        hipLaunchKernelGGL(upsample2_pad_kernel<false>, dim3(ublocks(nthreads)), dim3(UT), 0, s, x, scale, shift,
                           nthreads, h, w, C, Ho, Wo, pt, pl, ry, rx, out, out_cstride);
    return check_launch("unet_upsample2_pad");
}

extern "C" int dcs_unet_out_diffmap(const float* y, const float* scale, const float* shift, const float* w, float bias,
                                    int64_t P, int C, float threshold, const float* vol_in, float* vol_out, float* diff,
                                    void* stream) {
    if (!y || !scale || !shift || !w) return fail(DCS_E_INVALID, "unet_out_diffmap: null pointer");
    if ((vol_in == nullptr) != (vol_out == nullptr))
        return fail(DCS_E_INVALID, "unet_out_diffmap: vol_in and vol_out come together");
    if (!vol_out && !diff) return fail(DCS_E_INVALID, "unet_out_diffmap: nothing to compute");
    if (P <= 0 || P >= MAX_THREADS / 16 || C <= 0 || C > 256 || C % 4 != 0)
        return fail(DCS_E_INVALID, "unet_out_diffmap: bad dimensions (C % 4 == 0, C <= 256)");
    if (diff && (diff == vol_out || diff == vol_in)) return fail(DCS_E_INVALID, "unet_out_diffmap: diff aliases the volume");
    if (!aligned_to(y, 16) || !aligned_to(scale, 16) || !aligned_to(shift, 16) || !aligned_to(w, 16) ||
        !aligned_to(vol_in, 4) || !aligned_to(vol_out, 4) || !aligned_to(diff, 4))
        return fail(DCS_E_INVALID, "unet_out_diffmap: misaligned pointer");
    hipStream_t s = as_stream(stream);
    switch (C % 16 == 0 ? C / 16 : 1) {  // lanes per pixel: 16 channels a lane where that is a power of two
        case 2: launch_out_proj<2>(y, scale, shift, w, bias, P, C, threshold, vol_in, vol_out, diff, s); break;
        case 4: launch_out_proj<4>(y, scale, shift, w, bias, P, C, threshold, vol_in, vol_out, diff, s); break;
        case 8: launch_out_proj<8>(y, scale, shift, w, bias, P, C, threshold, vol_in, vol_out, diff, s); break;
        case 16: launch_out_proj<16>(y, scale, shift, w, bias, P, C, threshold, vol_in, vol_out, diff, s); break;
        default: launch_out_proj<1>(y, scale, shift, w, bias, P, C, threshold, vol_in, vol_out, diff, s); break;
    }
    return check_launch("unet_out_diffmap");
}

extern "C" int dcs_unet_apply_diffmap(const float* diff, int64_t n, float threshold, const float* vol_in,
                                      float* vol_out, void* stream) {
    if (!diff || !vol_in || !vol_out) return fail(DCS_E_INVALID, "unet_apply_diffmap: null pointer");
    if (diff == vol_out) return fail(DCS_E_INVALID, "unet_apply_diffmap: diff aliases the output");
    if (n <= 0 || n >= MAX_THREADS) return fail(DCS_E_INVALID, "unet_apply_diffmap: bad element count");
    if (!aligned_to(diff, 4) || !aligned_to(vol_in, 4) || !aligned_to(vol_out, 4))
        return fail(DCS_E_INVALID, "unet_apply_diffmap: misaligned pointer");
    hipLaunchKernelGGL((out_diffmap_kernel<false, 1>), dim3(ublocks(n)), dim3(UT), 0, as_stream(stream),
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0.f,
                       n, 0, threshold, diff, vol_in, vol_out, (float*)nullptr);
    return check_launch("unet_apply_diffmap");
}
