// LPIPS (lpips 0.1.4, net='alex') of calculate.py on gfx950: the pieces the convolution passes of
// conv.hip do not cover (modules/metrics.py::lpips_taps states the metric; modules/hip/lpips.py
// drives the layers).  Activations are NHWC float32.
//
//   lpips_stem_kernel  AlexNet's first layer (11x11 stride 4 pad 2, 3 -> 64) + bias + ReLU straight
//                      from the float32 [N][H][W] volume.  The input chain is folded in: the
//                      re-normalisation (x - off) / div, t * 2 - 1, and the scaling layer on three
//                      equal channels, which makes the layer a 2-channel convolution over (x, 1)
//                      (modules/lpips_weights.py::stem_fold).  The constant channel is zero in the
//                      padding, so its sum depends on which kernel rows and columns lie inside the
//                      image: 4 x 4 classes (top cut, whole, bottom cut by 1 or 2; the same across),
//                      summed per class on the host in float64 and added to the bias (cb).
//   lpips_tap_kernel   one read of a tap's ReLU maps of both volumes: per pixel the channel norms,
//                      the lin-weighted squared difference of the unit-normalised features (float64
//                      on the float32 samples), the per-slice spatial sum, and the 3x3 stride-2 max
//                      pool of both maps that feeds the next layer.
//
// No floating-point atomics: a workgroup sums its pixels in a fixed order and writes one float64
// partial, lpips_fold_kernel adds the partials of a slice in index order.  A slice's result
// depends on that slice alone, whatever the call's N.
#include "common.hpp"

// no contracted multiply-add: a * ia - b * ib must be exactly 0 for equal maps (the stem's
// multiply-adds are explicit fmaf)
#pragma clang fp contract(off)

namespace dcs {

constexpr int LT = 256;                 // threads per block
constexpr int SK = 11, SS = 4, SP = 2;  // the stem's kernel, stride and padding
constexpr int SCO = 64;                 // its output channels
constexpr int STO = 8;                  // output tile side: one pixel per lane of a wave
constexpr int SPW = SS * STO + SK - SS; // input patch side: 39
constexpr int SLD = 40;                 // patch rows / row stride after the stride-4 de-interleave
constexpr int TAP_PARTS_MAX = 256, TAP_PIX = 64;

// Row or column i of the patch is kept at (i % 4) * 10 + i / 4: the lanes of a wave read inputs 4
// apart, which land on consecutive LDS words this way (32 lanes on 32 banks).
__device__ __forceinline__ int deint(int i) { return (i & 3) * 10 + (i >> 2); }

// which kernel rows (or columns) of output o lie inside an image of n inputs:
// 0 = the first SP are cut, 1 = all, 2 / 3 = the last one / two are cut
__device__ __forceinline__ int edge_class(int o, int n) {
    if (o * SS - SP < 0) return 0;
    const int over = o * SS - SP + SK - n;
    return over <= 0 ? 1 : 1 + over;
}

__global__ void __launch_bounds__(LT) lpips_stem_kernel(const float* __restrict__ x, int H, int W, int Ho, int Wo,
                                                        int ntx, float off, float div, const float* __restrict__ wx,
                                                        const float* __restrict__ cb, float* __restrict__ out) {
    __shared__ float4 wl[SK * SK * SCO / 4];  // [tap][channel]
    __shared__ float patch[SLD * SLD];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int oy0 = (blockIdx.x / ntx) * STO, ox0 = (blockIdx.x % ntx) * STO;
    const float4* __restrict__ wx4 = reinterpret_cast<const float4*>(wx);
    for (int i = tid; i < SK * SK * SCO / 4; i += LT) wl[i] = wx4[i];
    const float* __restrict__ xs = x + (int64_t)n * H * W;
    const int iy0 = oy0 * SS - SP, ix0 = ox0 * SS - SP;
    for (int i = tid; i < SPW * SPW; i += LT) {
        const int r = i / SPW, c = i - r * SPW;
        const int iy = iy0 + r, ix = ix0 + c;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = (xs[(int64_t)iy * W + ix] - off) / div * 2.f - 1.f;
        patch[deint(r) * SLD + deint(c)] = v;
    }
    __syncthreads();
    const int p = tid & 63, g = tid >> 6;  // one wave per 16 output channels: its weight reads broadcast
    const int py = p >> 3, px = p & 7;
    const int oy = oy0 + py, ox = ox0 + px;
    const bool live = oy < Ho && ox < Wo;
    float acc[16];
    {
        const int cls = live ? edge_class(oy, H) * 4 + edge_class(ox, W) : 5;
        const float4* __restrict__ c4 = reinterpret_cast<const float4*>(cb + cls * SCO + g * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 v = c4[j];
            acc[4 * j] = v.x, acc[4 * j + 1] = v.y, acc[4 * j + 2] = v.z, acc[4 * j + 3] = v.w;
        }
    }
    for (int ky = 0; ky < SK; ++ky) {
        const float* __restrict__ prow = patch + (deint(ky) + py) * SLD + px;
#pragma unroll
        for (int kx = 0; kx < SK; ++kx) {
            const float xv = prow[deint(kx)];
            const float4* __restrict__ wt = wl + ((ky * SK + kx) * SCO + g * 16) / 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 w4 = wt[j];
                acc[4 * j] = fmaf(w4.x, xv, acc[4 * j]);
                acc[4 * j + 1] = fmaf(w4.y, xv, acc[4 * j + 1]);
                acc[4 * j + 2] = fmaf(w4.z, xv, acc[4 * j + 2]);
                acc[4 * j + 3] = fmaf(w4.w, xv, acc[4 * j + 3]);
            }
        }
    }
    if (!live) return;
    float4* __restrict__ o4 = reinterpret_cast<float4*>(out + (((int64_t)n * Ho + oy) * Wo + ox) * SCO + g * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        o4[j] = make_float4(fmaxf(acc[4 * j], 0.f), fmaxf(acc[4 * j + 1], 0.f), fmaxf(acc[4 * j + 2], 0.f),
                            fmaxf(acc[4 * j + 3], 0.f));
}

// sum over the 16 lanes that share a pixel
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
    return v;
}

__device__ __forceinline__ float4 max4(const float4& a, const float4& b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// Block (t, n) takes pixels [t * per, (t + 1) * per) of slice n, 16 lanes per pixel with IT float4
// of channels each (C = 64 * IT), and then its share of the pooled outputs (pa != nullptr).
template <int IT>
__global__ void __launch_bounds__(LT) lpips_tap_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                       const float* __restrict__ lin, int h, int w, int T,
                                                       float* __restrict__ pa, float* __restrict__ pb, int hp, int wp,
                                                       double* __restrict__ ws) {
    constexpr int C4 = 16 * IT;
    __shared__ double red[LT / 16];
    const int tid = threadIdx.x, grp = tid >> 4, l = tid & 15;
    const int n = blockIdx.y, t = blockIdx.x;
    const int npx = h * w;
    const int per = (npx + T - 1) / T;
    const int p0 = t * per, p1 = min(npx, p0 + per);
    const float4* __restrict__ a4 = reinterpret_cast<const float4*>(fa) + (int64_t)n * npx * C4;
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(fb) + (int64_t)n * npx * C4;
    float4 lw[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) lw[i] = reinterpret_cast<const float4*>(lin)[l + 16 * i];
    double acc = 0.0;
    for (int base = p0; base < p1; base += LT / 16) {  // the same trip count for every lane of the block
        const int p = base + grp;
        const bool live = p < p1;
        float4 va[IT], vb[IT];
        double na = 0.0, nb = 0.0;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            va[i] = live ? a4[(int64_t)p * C4 + l + 16 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
            vb[i] = live ? b4[(int64_t)p * C4 + l + 16 * i] : make_float4(0.f, 0.f, 0.f, 0.f);
            na += (double)va[i].x * va[i].x + (double)va[i].y * va[i].y + (double)va[i].z * va[i].z +
                  (double)va[i].w * va[i].w;
            nb += (double)vb[i].x * vb[i].x + (double)vb[i].y * vb[i].y + (double)vb[i].z * vb[i].z +
                  (double)vb[i].w * vb[i].w;
        }
        const double ia = 1.0 / (sqrt(group_sum(na)) + 1e-10), ib = 1.0 / (sqrt(group_sum(nb)) + 1e-10);
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const double dx = va[i].x * ia - vb[i].x * ib, dy = va[i].y * ia - vb[i].y * ib;
            const double dz = va[i].z * ia - vb[i].z * ib, dw = va[i].w * ia - vb[i].w * ib;
            s += (double)lw[i].x * (dx * dx) + (double)lw[i].y * (dy * dy) + (double)lw[i].z * (dz * dz) +
                 (double)lw[i].w * (dw * dw);
        }
        acc += group_sum(s);  // 0 for a pixel past the range
    }
    if (l == 0) red[grp] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < LT / 16; ++i) s += red[i];
        ws[(int64_t)n * T + t] = s;
    }
    if (!pa) return;  // kernel argument: uniform
    const int tot = hp * wp * C4;
    const int per2 = (tot + T - 1) / T;
    const int e1 = min(tot, (t + 1) * per2);
    float4* __restrict__ oa = reinterpret_cast<float4*>(pa) + (int64_t)n * tot;
    float4* __restrict__ ob = reinterpret_cast<float4*>(pb) + (int64_t)n * tot;
    for (int e = t * per2 + tid; e < e1; e += LT) {
        const int c4 = e % C4, q = e / C4;
        const int qx = q % wp, qy = q / wp;
        const int64_t src = ((int64_t)(2 * qy) * w + 2 * qx) * C4 + c4;  // rows 2qy .. 2qy+2 < h, the same across
        float4 ma = a4[src], mb = b4[src];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int64_t o = src + ((int64_t)dy * w + dx) * C4;
                ma = max4(ma, a4[o]);
                mb = max4(mb, b4[o]);
            }
        oa[e] = ma;
        ob[e] = mb;
    }
}

__global__ void lpips_fold_kernel(const double* __restrict__ ws, int N, int T, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += ws[(int64_t)n * T + t];
    out[n] = s;
}

static int tap_parts(int h, int w) {
    const int64_t t = cdiv((int64_t)h * w, TAP_PIX);
    return (int)(t > TAP_PARTS_MAX ? TAP_PARTS_MAX : t);
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool finite(float v) { return v - v == 0.f; }

}  // namespace dcs

using namespace dcs;

extern "C" int dcs_lpips_stem(const float* x, int N, int H, int W, float off, float div, const float* wx,
                              const float* cb, float* out, void* stream) {
    if (!x || !wx || !cb || !out) return fail(DCS_E_INVALID, "lpips_stem: null pointer");
    if (N <= 0 || N > 65535 || H < SK || W < SK || (int64_t)H * W >= (1ll << 31) / SCO)
        return fail(DCS_E_INVALID, "lpips_stem: 1..65535 slices with sides of at least 11 are required");
    if (!aligned16(wx) || !aligned16(cb) || !aligned16(out) || (reinterpret_cast<uintptr_t>(x) & 3))
        return fail(DCS_E_INVALID, "lpips_stem: misaligned pointer");
    if (!finite(off) || !finite(div) || !(div > 0.f)) return fail(DCS_E_INVALID, "lpips_stem: off must be finite, div finite and positive");
    const int Ho = (H + 2 * SP - SK) / SS + 1, Wo = (W + 2 * SP - SK) / SS + 1;
    const int ntx = (int)cdiv(Wo, STO), nty = (int)cdiv(Ho, STO);
    hipLaunchKernelGGL(lpips_stem_kernel, dim3((unsigned)(ntx * nty), (unsigned)N), dim3(LT), 0, as_stream(stream), x, H,
                       W, Ho, Wo, ntx, off, div, wx, cb, out);
    return check_launch("lpips_stem");
}

extern "C" size_t dcs_lpips_tap_workspace_size(int N, int h, int w) {
    if (N <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)N * tap_parts(h, w) * sizeof(double);
}

extern "C" int dcs_lpips_tap(const float* fa, const float* fb, int N, int h, int w, int C, const float* lin,
                             float* pool_a, float* pool_b, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (!fa || !fb || !lin || !out || !ws) return fail(DCS_E_INVALID, "lpips_tap: null pointer");
    if (N <= 0 || N > 65535 || h <= 0 || w <= 0 || (int64_t)h * w * C >= (1ll << 31))
        return fail(DCS_E_INVALID, "lpips_tap: bad dimensions");
    if (C != 64 && C != 192 && C != 256 && C != 384) return fail(DCS_E_INVALID, "lpips_tap: C must be 64, 192, 256 or 384");
    if ((pool_a == nullptr) != (pool_b == nullptr)) return fail(DCS_E_INVALID, "lpips_tap: the pooled outputs come together");
    if (pool_a && (h < 3 || w < 3)) return fail(DCS_E_INVALID, "lpips_tap: a map below 3x3 has no 3x3 pool");
    if (pool_a && (pool_a == pool_b || pool_a == fa || pool_a == fb || pool_b == fa || pool_b == fb))
        return fail(DCS_E_INVALID, "lpips_tap: the pooled outputs must not alias each other or the inputs");
    if (!aligned16(fa) || !aligned16(fb) || !aligned16(lin) || !aligned16(pool_a) || !aligned16(pool_b) ||
        (reinterpret_cast<uintptr_t>(out) & 7) || (reinterpret_cast<uintptr_t>(ws) & 7))
        return fail(DCS_E_INVALID, "lpips_tap: misaligned pointer");
    if (ws_bytes < dcs_lpips_tap_workspace_size(N, h, w)) return fail(DCS_E_WORKSPACE, "lpips_tap: workspace too small");
    const int T = tap_parts(h, w);
    const int hp = pool_a ? (h - 3) / 2 + 1 : 0, wp = pool_a ? (w - 3) / 2 + 1 : 0;
    const dim3 grid((unsigned)T, (unsigned)N);
    hipStream_t s = as_stream(stream);
    double* wsd = static_cast<double*>(ws);
#define DCS_LPIPS_TAP(IT) \
    hipLaunchKernelGGL(lpips_tap_kernel<IT>, grid, dim3(LT), 0, s, fa, fb, lin, h, w, T, pool_a, pool_b, hp, wp, wsd)
    if (C == 64) DCS_LPIPS_TAP(1);
    else if (C == 192) DCS_LPIPS_TAP(3);
    else if (C == 256) DCS_LPIPS_TAP(4);
    else DCS_LPIPS_TAP(6);
#undef DCS_LPIPS_TAP
    if (int rc = check_launch("lpips_tap")) return rc;
    hipLaunchKernelGGL(lpips_fold_kernel, dim3((unsigned)cdiv(N, LT)), dim3(LT), 0, s, wsd, N, T, out);
    return check_launch("lpips_tap");
}
