// The passes between the convolutions of the normal-map U-Net's TRAINING step on gfx950
// (modules/hip/unet_train.py; the 3x3 convolutions, their data and weight gradients run on the rows
// pass, conv.hip): BatchNorm batch statistics, the backward of BatchNorm + ReLU (+ 2x2 max pool, +
// the 1x1 output projection), the L1 tail, the adjoint of the bilinear x2 upsample with the pad
// split, and the gradient norm with its clip coefficient.
//
// Activations are NHWC float32; one thread owns one 16-byte vector of 4 channels.  Every reduction
// has two stages and a fixed order: a thread walks its pixels in ascending order and adds in
// float64, a block merges its threads by a tree in LDS whose shape depends on the launch geometry
// only, and a second kernel adds the per-block partials in index order.  No atomics: a step gives
// the same bits from run to run.
//
// The affine map relu(y * scale + shift) is the one of unet.hip (one float32 rounding per step,
// contraction off), so the ReLU mask and the pool's argmax recomputed here are the forward's.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int TT = 256;           // threads per block
constexpr int TR_MAX_CHUNKS = 1024;  // per-block partials of one reduction
constexpr int64_t TR_MAX_THREADS = (int64_t)1 << 38;

static bool al16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % 16) == 0; }
static bool al4(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % 4) == 0; }

// Launch geometry of a per-channel reduction over ``items`` (pixels or 2x2 quads) of a C-channel
// tensor: thread t owns channel vector t % CV and walks items pl, pl + PL, ... of its block's
// ``per`` items (pl = t / CV < PL).
struct RedGeom {
    int CV, PL, nchunk;
    int64_t per;
};

static RedGeom red_geom(int64_t items, int C) {
    RedGeom g;
    g.CV = C / 4;
    g.PL = TT / g.CV;
    int64_t per = cdiv(items, TR_MAX_CHUNKS);
    const int64_t least = (int64_t)g.PL * 8;
    per = per < least ? least : per;
    g.per = cdiv(per, g.PL) * g.PL;
    g.nchunk = (int)cdiv(items, g.per);
    return g;
}

// N, H, W, C of an NHWC activation a per-channel reduction covers
static bool red_dims_ok(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || C > 4 * TT) return false;
    return (long double)N * H * W * C < (long double)TR_MAX_THREADS;
}

// Tree merge of K x 4 float64 accumulators per thread over the pl index (t = pl * CV + cv); the
// totals end in lds[kj * TT + cv] (threads t < CV).  lds: K * 4 * TT doubles.
template <int K>
__device__ __forceinline__ void block_tree(const double (&acc)[K][4], int CV, int PL, double* lds) {
    const int t = threadIdx.x;
    const int pl = t / CV;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) lds[(k * 4 + j) * TT + t] = acc[k][j];
    __syncthreads();
    int s = 1;
    while (s < PL) s <<= 1;
    for (s >>= 1; s > 0; s >>= 1) {
        if (pl < s && pl + s < PL) {
#pragma unroll
            for (int kj = 0; kj < K * 4; ++kj) lds[kj * TT + t] += lds[kj * TT + t + s * CV];
        }
        __syncthreads();
    }
}

// Sum of the per-block partials parts[(chunk * C + c) * K + k] of channel c = blockIdx.x in chunk
// order: thread t adds chunks t, t + TT, ..., then a fixed tree; the totals are valid in thread 0.
template <int K>
__device__ __forceinline__ void channel_total(const double* __restrict__ parts, int nchunk, int C, double (&tot)[K],
                                              double* lds /* K * TT */) {
    const int t = threadIdx.x, c = blockIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] = 0.0;
    for (int ch = t; ch < nchunk; ch += TT)
#pragma unroll
        for (int k = 0; k < K; ++k) tot[k] += parts[((int64_t)ch * C + c) * K + k];
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k * TT + t] = tot[k];
    __syncthreads();
    for (int s = TT / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < K; ++k) lds[k * TT + t] += lds[k * TT + t + s];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] = lds[k * TT];
}

// Sum of n float64 partials in index order by one block; valid in every thread.
__device__ __forceinline__ double partials_total(const double* __restrict__ parts, int64_t n, double* lds /* TT */) {
    const int t = threadIdx.x;
    double s = 0.0;
    const int64_t per = (n + TT - 1) / TT;  // thread t: a contiguous run, so the order is the index order
    const int64_t i0 = t * per, i1 = i0 + per < n ? i0 + per : n;
    for (int64_t i = i0; i < i1; ++i) s += parts[i];
    lds[t] = s;
    __syncthreads();
    for (int st = TT / 2; st > 0; st >>= 1) {
        if (t < st) lds[t] += lds[t + st];
        __syncthreads();
    }
    return lds[0];
}

// ---------------------------------------------------------------------------------------
// BatchNorm batch statistics
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TT) bn_stats_partial_kernel(const float* __restrict__ y, int64_t M, int C, int CV,
                                                              int PL, int64_t per, double* __restrict__ parts) {
    __shared__ double lds[2 * 4 * TT];
    const int t = threadIdx.x, cv = t % CV, pl = t / CV;
    double acc[2][4] = {};
    if (pl < PL) {
        // sums of x - k and (x - k)^2 with k the channel's first value: exact differences in float64, and
        // no cancellation in the variance however far the mean lies from zero
        const float4 kv = *reinterpret_cast<const float4*>(y + cv * 4);
        const double k0[4] = {(double)kv.x, (double)kv.y, (double)kv.z, (double)kv.w};
        const int64_t p0 = (int64_t)blockIdx.x * per;
        const int64_t p1 = p0 + per < M ? p0 + per : M;
        for (int64_t p = p0 + pl; p < p1; p += PL) {
            const float4 v = *reinterpret_cast<const float4*>(y + p * C + cv * 4);
            const double d[4] = {(double)v.x - k0[0], (double)v.y - k0[1], (double)v.z - k0[2], (double)v.w - k0[3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] += d[j];
                acc[1][j] += d[j] * d[j];
            }
        }
    }
    block_tree<2>(acc, CV, PL, lds);
    if (t < CV) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 2; ++k)
                parts[((int64_t)blockIdx.x * C + cv * 4 + j) * 2 + k] = lds[(k * 4 + j) * TT + t];
    }
}

// One block per channel: mean and biased variance from the float64 sums (shifted by y[0][c]), the folded pair
// scale = gamma * invstd, shift = beta - mean * scale (nrep copies: the rows pass reads its
// prologue per image), and the running statistics (unbiased variance, momentum).
__global__ void __launch_bounds__(TT) bn_stats_finish_kernel(const double* __restrict__ parts, int nchunk, int C,
                                                             int64_t M, const float* __restrict__ y, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float momentum,
                                                             int nrep, float* __restrict__ scale,
                                                             float* __restrict__ shift, float* __restrict__ mean,
                                                             float* __restrict__ invstd, float* running_mean,
                                                             float* running_var) {
    __shared__ double lds[2 * TT];
    double tot[2];
    channel_total<2>(parts, nchunk, C, tot, lds);
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    const double dm = tot[0] / (double)M;  // mean - k
    const double m = (double)y[c] + dm;
    double var = tot[1] / (double)M - dm * dm;
    var = var > 0.0 ? var : 0.0;
    const double is = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * is;
    const double sh = (double)beta[c] - m * sc;
    for (int r = 0; r < nrep; ++r) {
        scale[(int64_t)r * C + c] = (float)sc;
        shift[(int64_t)r * C + c] = (float)sh;
    }
    mean[c] = (float)m;
    invstd[c] = (float)is;
    if (running_mean) running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * m);
    if (running_var)
        running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] +
                                 (double)momentum * var * ((double)M / (double)(M - 1)));
}

// ---------------------------------------------------------------------------------------
// backward of a = relu(BatchNorm(y)) (+ 2x2 max pool of a, + the 1x1 projection of a)
// ---------------------------------------------------------------------------------------
// The gradient reaching a, in one of three forms:
//   A  da: a channel slice of an [N,H,W,da_cstride] tensor
//   B  A + dpool [N,H/2,W/2,C] routed to the first maximum (row-major) of each 2x2 window of a
//   C  da[p,c] = dout[p] * wout[c]
struct BwdArgs {
    const float* da;
    int da_cstride;
    const float* dpool;
    const float* dout;
    const float* wout;
    const float* y;
    const float* scale;
    const float* shift;
    const float* mean;
    const float* invstd;
    int H, W, C, Hq, Wq;
};

__device__ __forceinline__ void ld4(float (&d)[4], const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}

// 4 channels (from c) of quad q = (n, qy, qx): for its up to 4 pixels (k = 2 dy + dx) the pixel
// index, y, a = relu(y * scale + shift) and g = da * [a's pre-activation > 0].
template <int FORM>
__device__ __forceinline__ void quad_grad(const BwdArgs& A, int64_t q, int c, int64_t (&pix)[4], float (&yv)[4][4],
                                          float (&av)[4][4], float (&g)[4][4], float (&dov)[4]) {
    const int qx = (int)(q % A.Wq);
    int64_t r = q / A.Wq;
    const int qy = (int)(r % A.Hq);
    const int64_t n = r / A.Hq;
    float sc[4], sh[4];
    ld4(sc, A.scale + c);
    ld4(sh, A.shift + c);
    float pre[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int h = 2 * qy + (k >> 1), w = 2 * qx + (k & 1);
        pix[k] = (h < A.H && w < A.W) ? (n * A.H + h) * A.W + w : -1;
        dov[k] = 0.f;
        if (pix[k] < 0) continue;
        ld4(yv[k], A.y + pix[k] * A.C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pre[k][j] = yv[k][j] * sc[j] + sh[j];
            av[k][j] = pre[k][j] > 0.f ? pre[k][j] : 0.f;
        }
        if (FORM == 2) {
            float wv[4];
            ld4(wv, A.wout + c);
            dov[k] = A.dout[pix[k]];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] = dov[k] * wv[j];
        } else {
            ld4(g[k], A.da + pix[k] * A.da_cstride + c);
        }
    }
    if (FORM == 1 && 2 * qy + 1 < A.H && 2 * qx + 1 < A.W) {  // a whole window: it formed a pooled pixel
        float dp[4];
        ld4(dp, A.dpool + ((n * (A.H >> 1) + qy) * (A.W >> 1) + qx) * A.C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int best = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (av[k][j] > av[best][j]) best = k;  // strict: the first maximum keeps the gradient
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k == best) g[k][j] = g[k][j] + dp[j];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (pix[k] < 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) g[k][j] = pre[k][j] > 0.f ? g[k][j] : 0.f;
    }
}

// Partials per block and channel: sum g, sum g * xhat; form C also sum dout * a and sum dout.
template <int FORM>
__global__ void __launch_bounds__(TT) bn_bwd_sums_kernel(BwdArgs A, int64_t Q, int CV, int PL, int64_t per,
                                                         double* __restrict__ parts) {
    constexpr int K = FORM == 2 ? 4 : 2;
    __shared__ double lds[K * 4 * TT];
    const int t = threadIdx.x, cv = t % CV, pl = t / CV;
    double acc[K][4] = {};
    if (pl < PL) {
        const int c = cv * 4;
        float mu[4], is[4];
        ld4(mu, A.mean + c);
        ld4(is, A.invstd + c);
        const int64_t q0 = (int64_t)blockIdx.x * per;
        const int64_t q1 = q0 + per < Q ? q0 + per : Q;
        for (int64_t q = q0 + pl; q < q1; q += PL) {
            int64_t pix[4];
            float yv[4][4], av[4][4], g[4][4], dov[4];
            quad_grad<FORM>(A, q, c, pix, yv, av, g, dov);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (pix[k] < 0) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xh = (yv[k][j] - mu[j]) * is[j];
                    acc[0][j] += (double)g[k][j];
                    acc[1][j] += (double)g[k][j] * (double)xh;
                    if (FORM == 2) {
                        acc[2][j] += (double)dov[k] * (double)av[k][j];
                        acc[3][j] += (double)dov[k];
                    }
                }
            }
        }
    }
    block_tree<K>(acc, CV, PL, lds);
    if (t < CV) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k)
                parts[((int64_t)blockIdx.x * A.C + cv * 4 + j) * K + k] = lds[(k * 4 + j) * TT + t];
    }
}

template <int K>
__global__ void __launch_bounds__(TT) bn_bwd_finish_kernel(const double* __restrict__ parts, int nchunk, int C,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ dwout, float* __restrict__ dbias) {
    __shared__ double lds[K * TT];
    double tot[K];
    channel_total<K>(parts, nchunk, C, tot, lds);
    if (threadIdx.x != 0) return;
    const int c = blockIdx.x;
    dbeta[c] = (float)tot[0];
    dgamma[c] = (float)tot[1];
    if (K == 4) {
        dwout[c] = (float)tot[2];
        if (c == 0) dbias[0] = (float)tot[3];
    }
}

// dy = scale * (g - dbeta / M - xhat * dgamma / M), scale = gamma * invstd.  One thread: 4 channels
// of one quad.
template <int FORM>
__global__ void __launch_bounds__(TT) bn_bwd_apply_kernel(BwdArgs A, int64_t nthreads, float inv_m,
                                                          const float* __restrict__ dgamma,
                                                          const float* __restrict__ dbeta, float* __restrict__ dy) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= nthreads) return;
    const int C4 = A.C >> 2;
    const int c = (int)(i % C4) * 4;
    const int64_t q = i / C4;
    int64_t pix[4];
    float yv[4][4], av[4][4], g[4][4], dov[4];
    quad_grad<FORM>(A, q, c, pix, yv, av, g, dov);
    float mu[4], is[4], sc[4], dg[4], db[4];
    ld4(mu, A.mean + c);
    ld4(is, A.invstd + c);
    ld4(sc, A.scale + c);
    ld4(dg, dgamma + c);
    ld4(db, dbeta + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (pix[k] < 0) continue;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (yv[k][j] - mu[j]) * is[j];
            o[j] = sc[j] * (g[k][j] - db[j] * inv_m - xh * (dg[j] * inv_m));
        }
        *reinterpret_cast<float4*>(dy + pix[k] * A.C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---------------------------------------------------------------------------------------
// the training tail: projection, L1 loss, d loss / d o
// ---------------------------------------------------------------------------------------
// LP lanes per pixel as unet.hip's output kernel.  Each block writes the float64 sum of |o - t| of
// its pixels (an xor butterfly and a 4-wave sum: fixed order).
template <int LP>
__global__ void __launch_bounds__(TT) l1_out_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, const float* __restrict__ wout,
                                                    const float* __restrict__ bias, const float* __restrict__ target,
                                                    int64_t P, int C, float k, float* __restrict__ o_out,
                                                    float* __restrict__ dout, double* __restrict__ parts) {
    __shared__ double red[4];
    const int64_t t = (int64_t)blockIdx.x * TT + threadIdx.x;
    const int64_t p = t / LP;
    const bool live = p < P;  // a lane past the end still takes part in the reductions
    const int CL = C / LP, c0 = (int)(t % LP) * CL;
    float acc = 0.f;
    if (live) {
        const float* row = y + p * C;
        for (int c = c0; c < c0 + CL; c += 4) {
            float yv[4], sc[4], sh[4], wv[4];
            ld4(yv, row + c);
            ld4(sc, scale + c);
            ld4(sh, shift + c);
            ld4(wv, wout + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = yv[j] * sc[j] + sh[j];
                a = a > 0.f ? a : 0.f;
                acc = acc + a * wv[j];
            }
        }
    }
#pragma unroll
    for (int s = LP / 2; s > 0; s >>= 1) acc = acc + __shfl_xor(acc, s, 64);
    double l = 0.0;
    if (live && t % LP == 0) {
        const float o = acc + bias[0];
        const float d = o - target[p];
        if (o_out) o_out[p] = o;
        dout[p] = k * sgnf(d);
        l = (double)fabsf(d);
    }
    l = block_sum_256_d(l, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = l;
}

__global__ void __launch_bounds__(TT) l1_finish_kernel(const double* __restrict__ parts, int64_t n, double mul,
                                                       float* __restrict__ loss) {
    __shared__ double lds[TT];
    const double s = partials_total(parts, n, lds);
    if (threadIdx.x == 0) loss[0] = (float)(s * mul);
}

// ---------------------------------------------------------------------------------------
// adjoint of unet.hip's upsample2_pad (bilinear x2, align_corners, centred by the pad split)
// ---------------------------------------------------------------------------------------
// weight of source index s in output index u of one axis: the forward's own arithmetic
__device__ __forceinline__ float up_weight(int u, int s, int n, float r) {
    const float f = r * (float)u;
    int i0 = (int)f;
    i0 = i0 > n - 1 ? n - 1 : i0;
    const int i1 = i0 + (i0 < n - 1 ? 1 : 0);
    const float l1 = f - (float)i0, l0 = 1.f - l1;
    float wgt = 0.f;
    if (i0 == s) wgt = wgt + l0;
    if (i1 == s) wgt = wgt + l1;
    return wgt;
}

// One thread: 4 channels of one source pixel; it gathers the outputs 2 s - 2 .. 2 s + 3 per axis
// (every output whose two taps can reach s) in ascending order.
__global__ void __launch_bounds__(TT) upsample2_pad_bwd_kernel(const float* __restrict__ dcat, int cstride,
                                                               int64_t nthreads, int h, int w, int C, int Ho, int Wo,
                                                               int pt, int pl, float ry, float rx,
                                                               float* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * TT + threadIdx.x;
    if (i >= nthreads) return;
    const int C4 = C >> 2;
    const int c = (int)(i % C4) * 4;
    int64_t r = i / C4;
    const int x = (int)(r % w);
    r /= w;
    const int yy = (int)(r % h);
    const int64_t n = r / h;
    float wy[6], wx[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int uy = 2 * yy - 2 + k, ux = 2 * x - 2 + k;
        wy[k] = (uy >= 0 && uy < 2 * h) ? up_weight(uy, yy, h, ry) : 0.f;
        wx[k] = (ux >= 0 && ux < 2 * w) ? up_weight(ux, x, w, rx) : 0.f;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 6; ++ky) {
        if (wy[ky] == 0.f) continue;
        const int Y = 2 * yy - 2 + ky + pt;  // inside [pt, pt + 2h) within [0, Ho)
#pragma unroll
        for (int kx = 0; kx < 6; ++kx) {
            if (wx[kx] == 0.f) continue;
            const int X = 2 * x - 2 + kx + pl;
            float g[4];
            ld4(g, dcat + ((n * Ho + Y) * Wo + X) * cstride + c);
            const float wgt = wy[ky] * wx[kx];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + wgt * g[j];
        }
    }
    *reinterpret_cast<float4*>(dx + ((n * h + yy) * w + x) * C + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// ---------------------------------------------------------------------------------------
// gradient norm and clip coefficient
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TT) sumsq_partial_kernel(const float* __restrict__ g, int64_t n, int64_t per,
                                                           double* __restrict__ parts) {
    __shared__ double red[4];
    const int64_t i0 = (int64_t)blockIdx.x * per;
    const int64_t i1 = i0 + per < n ? i0 + per : n;
    double s = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += TT) {
        const double v = (double)g[i];
        s += v * v;
    }
    s = block_sum_256_d(s, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}

// out[0] = the L2 norm, out[1] = min(1, clip / (norm + 1e-6)) (1 where clip <= 0: no clipping)
__global__ void __launch_bounds__(TT) sumsq_finish_kernel(const double* __restrict__ parts, int64_t nparts, float clip,
                                                          float* __restrict__ out) {
    __shared__ double lds[TT];
    const double s = partials_total(parts, nparts, lds);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(s);
    float coef = 1.f;
    if (clip > 0.f) {
        coef = clip / (norm + 1e-6f);
        coef = coef < 1.f ? coef : 1.f;
    }
    out[0] = norm;
    out[1] = coef;
}

static int64_t sumsq_per(int64_t n) {
    int64_t per = cdiv(n, TR_MAX_CHUNKS);
    per = per < 8 * TT ? 8 * TT : per;
    return cdiv(per, TT) * TT;
}

static int l1_lanes(int C) {
    const int lp = C % 16 == 0 ? C / 16 : 1;
    return (lp == 2 || lp == 4 || lp == 8 || lp == 16) ? lp : 1;
}

static size_t bwd_ws_bytes(int N, int H, int W, int C) {
    const int64_t Q = (int64_t)N * ((H + 1) / 2) * ((W + 1) / 2);
    return (size_t)red_geom(Q, C).nchunk * C * 4 * sizeof(double);
}

static int bwd_check(const char* who, const float* da, int da_cstride, const float* dpool, const float* dout,
                     const float* wout, const float* y, const float* scale, const float* shift, const float* mean,
                     const float* invstd, int N, int H, int W, int C) {
    if (!y || !scale || !shift || !mean || !invstd) return fail(DCS_E_INVALID, who);
    if (!red_dims_ok(N, H, W, C)) return fail(DCS_E_INVALID, who);
    if (dout) {
        if (da || dpool || !wout) return fail(DCS_E_INVALID, who);
    } else {
        if (!da || wout) return fail(DCS_E_INVALID, who);
        if (da_cstride < C || da_cstride % 4 != 0 || (long double)N * H * W * da_cstride >= (long double)TR_MAX_THREADS)
            return fail(DCS_E_INVALID, who);
        if (dpool && (H < 2 || W < 2)) return fail(DCS_E_INVALID, who);
    }
    if (!al16(da) || !al16(dpool) || !al4(dout) || !al16(wout) || !al16(y) || !al16(scale) || !al16(shift) ||
        !al16(mean) || !al16(invstd))
        return fail(DCS_E_INVALID, who);
    return DCS_OK;
}

static BwdArgs bwd_args(const float* da, int da_cstride, const float* dpool, const float* dout, const float* wout,
                        const float* y, const float* scale, const float* shift, const float* mean,
                        const float* invstd, int H, int W, int C) {
    BwdArgs A;
    A.da = da, A.da_cstride = da_cstride, A.dpool = dpool, A.dout = dout, A.wout = wout, A.y = y;
    A.scale = scale, A.shift = shift, A.mean = mean, A.invstd = invstd;
    A.H = H, A.W = W, A.C = C, A.Hq = (H + 1) / 2, A.Wq = (W + 1) / 2;
    return A;
}

}  // namespace dcs

using namespace dcs;

extern "C" size_t dcs_unet_bn_stats_workspace_size(int64_t M, int C) {
    if (M <= 0 || C <= 0 || C % 4 != 0 || C > 4 * TT) return 0;
    return (size_t)red_geom(M, C).nchunk * C * 2 * sizeof(double);
}

extern "C" int dcs_unet_bn_stats(const float* y, int64_t M, int C, const float* gamma, const float* beta, float eps,
                                 float momentum, int nrep, float* scale, float* shift, float* mean, float* invstd,
                                 float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream) {
    if (!y || !gamma || !beta || !scale || !shift || !mean || !invstd || !ws)
        return fail(DCS_E_INVALID, "unet_bn_stats: null pointer");
    if (C <= 0 || C % 4 != 0 || C > 4 * TT || M < 2 || (long double)M * C >= (long double)TR_MAX_THREADS)
        return fail(DCS_E_INVALID, "unet_bn_stats: bad dimensions (C % 4 == 0, C <= 1024, at least 2 values per channel)");
    if (nrep < 1 || !(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f))
        return fail(DCS_E_INVALID, "unet_bn_stats: bad nrep, eps or momentum");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(DCS_E_INVALID, "unet_bn_stats: the running statistics come together");
    if (!al16(y) || !al4(gamma) || !al4(beta) || !al4(scale) || !al4(shift) || !al4(mean) || !al4(invstd) ||
        !al4(running_mean) || !al4(running_var) || (reinterpret_cast<uintptr_t>(ws) % 8) != 0)
        return fail(DCS_E_INVALID, "unet_bn_stats: misaligned pointer");
    if (ws_bytes < dcs_unet_bn_stats_workspace_size(M, C)) return fail(DCS_E_WORKSPACE, "unet_bn_stats: workspace too small");
    const RedGeom g = red_geom(M, C);
    hipStream_t s = as_stream(stream);
    double* parts = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)g.nchunk), dim3(TT), 0, s, y, M, C, g.CV, g.PL, g.per,
                       parts);
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)C), dim3(TT), 0, s, parts, g.nchunk, C, M, y, gamma, beta,
                       eps, momentum, nrep, scale, shift, mean, invstd, running_mean, running_var);
    return check_launch("unet_bn_stats");
}

extern "C" size_t dcs_unet_bn_relu_backward_workspace_size(int N, int H, int W, int C) {
    if (!red_dims_ok(N, H, W, C)) return 0;
    return bwd_ws_bytes(N, H, W, C);
}

extern "C" int dcs_unet_bn_relu_backward_sums(const float* da, int da_cstride, const float* dpool, const float* dout,
                                              const float* wout, const float* y, const float* scale,
                                              const float* shift, const float* mean, const float* invstd, int N, int H,
                                              int W, int C, float* dgamma, float* dbeta, float* dwout, float* dbias,
                                              void* ws, size_t ws_bytes, void* stream) {
    int e = bwd_check("unet_bn_relu_backward_sums: bad arguments", da, da_cstride, dpool, dout, wout, y, scale, shift,
                      mean, invstd, N, H, W, C);
    if (e) return e;
    if (!dgamma || !dbeta || !ws || (dout && (!dwout || !dbias)))
        return fail(DCS_E_INVALID, "unet_bn_relu_backward_sums: null output");
    if (!al4(dgamma) || !al4(dbeta) || !al4(dwout) || !al4(dbias) || (reinterpret_cast<uintptr_t>(ws) % 8) != 0)
        return fail(DCS_E_INVALID, "unet_bn_relu_backward_sums: misaligned pointer");
    if (ws_bytes < bwd_ws_bytes(N, H, W, C))
        return fail(DCS_E_WORKSPACE, "unet_bn_relu_backward_sums: workspace too small");
    const BwdArgs A = bwd_args(da, da_cstride, dpool, dout, wout, y, scale, shift, mean, invstd, H, W, C);
    const int64_t Q = (int64_t)N * A.Hq * A.Wq;
    const RedGeom g = red_geom(Q, C);
    hipStream_t s = as_stream(stream);
    double* parts = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)g.nchunk), blk(TT);
    if (dout) {
        hipLaunchKernelGGL(bn_bwd_sums_kernel<2>, grid, blk, 0, s, A, Q, g.CV, g.PL, g.per, parts);
        hipLaunchKernelGGL(bn_bwd_finish_kernel<4>, dim3((unsigned)C), blk, 0, s, parts, g.nchunk, C, dgamma, dbeta,
                           dwout, dbias);
    } else {
        if (dpool) hipLaunchKernelGGL(bn_bwd_sums_kernel<1>, grid, blk, 0, s, A, Q, g.CV, g.PL, g.per, parts);
        else hipLaunchKernelGGL(bn_bwd_sums_kernel<0>, grid, blk, 0, s, A, Q, g.CV, g.PL, g.per, parts);
        hipLaunchKernelGGL(bn_bwd_finish_kernel<2>, dim3((unsigned)C), blk, 0, s, parts, g.nchunk, C, dgamma, dbeta,
                           (float*)nullptr, (float*)nullptr);
    }
    return check_launch("unet_bn_relu_backward_sums");
}

extern "C" int dcs_unet_bn_relu_backward_apply(const float* da, int da_cstride, const float* dpool, const float* dout,
                                               const float* wout, const float* y, const float* scale,
                                               const float* shift, const float* mean, const float* invstd, int N,
                                               int H, int W, int C, const float* dgamma, const float* dbeta, float* dy,
                                               void* stream) {
    int e = bwd_check("unet_bn_relu_backward_apply: bad arguments", da, da_cstride, dpool, dout, wout, y, scale, shift,
                      mean, invstd, N, H, W, C);
    if (e) return e;
    if (!dgamma || !dbeta || !dy) return fail(DCS_E_INVALID, "unet_bn_relu_backward_apply: null pointer");
    if (dy == y || dy == da || dy == dpool) return fail(DCS_E_INVALID, "unet_bn_relu_backward_apply: dy aliases an input");
    if (!al16(dgamma) || !al16(dbeta) || !al16(dy))
        return fail(DCS_E_INVALID, "unet_bn_relu_backward_apply: pointers must be 16-byte aligned");
    const BwdArgs A = bwd_args(da, da_cstride, dpool, dout, wout, y, scale, shift, mean, invstd, H, W, C);
    const int64_t nthreads = (int64_t)N * A.Hq * A.Wq * (C / 4);
    const float inv_m = (float)(1.0 / ((double)N * H * W));
    const dim3 grid((unsigned)cdiv(nthreads, TT)), blk(TT);
    hipStream_t s = as_stream(stream);
    if (dout) hipLaunchKernelGGL(bn_bwd_apply_kernel<2>, grid, blk, 0, s, A, nthreads, inv_m, dgamma, dbeta, dy);
    else if (dpool) hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, grid, blk, 0, s, A, nthreads, inv_m, dgamma, dbeta, dy);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<0>, grid, blk, 0, s, A, nthreads, inv_m, dgamma, dbeta, dy);
    return check_launch("unet_bn_relu_backward_apply");
}

extern "C" size_t dcs_unet_l1_out_workspace_size(int64_t P, int C) {
    if (P <= 0 || C <= 0 || C % 4 != 0 || C > 256 || P >= TR_MAX_THREADS / 16) return 0;
    return (size_t)cdiv(P * l1_lanes(C), TT) * sizeof(double);
}

extern "C" int dcs_unet_l1_out(const float* y, const float* scale, const float* shift, const float* wout,
                               const float* bias, const float* target, int64_t P, int C, float gscale, float* o,
                               float* dout, float* loss, void* ws, size_t ws_bytes, void* stream) {
    if (!y || !scale || !shift || !wout || !bias || !target || !dout || !loss || !ws)
        return fail(DCS_E_INVALID, "unet_l1_out: null pointer");
    if (P <= 0 || P >= TR_MAX_THREADS / 16 || C <= 0 || C > 256 || C % 4 != 0)
        return fail(DCS_E_INVALID, "unet_l1_out: bad dimensions (C % 4 == 0, C <= 256)");
    if (!al16(y) || !al16(scale) || !al16(shift) || !al16(wout) || !al4(bias) || !al4(target) || !al4(o) ||
        !al4(dout) || !al4(loss) || (reinterpret_cast<uintptr_t>(ws) % 8) != 0)
        return fail(DCS_E_INVALID, "unet_l1_out: misaligned pointer");
    if (ws_bytes < dcs_unet_l1_out_workspace_size(P, C)) return fail(DCS_E_WORKSPACE, "unet_l1_out: workspace too small");
    const int lp = l1_lanes(C);
    const int64_t nblk = cdiv(P * lp, TT);
    const float k = (float)((double)gscale / (double)P);
    hipStream_t s = as_stream(stream);
    double* parts = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)nblk), blk(TT);
    switch (lp) {
        case 2: hipLaunchKernelGGL(l1_out_kernel<2>, grid, blk, 0, s, y, scale, shift, wout, bias, target, P, C, k, o, dout, parts); break;
        case 4: hipLaunchKernelGGL(l1_out_kernel<4>, grid, blk, 0, s, y, scale, shift, wout, bias, target, P, C, k, o, dout, parts); break;
        case 8: hipLaunchKernelGGL(l1_out_kernel<8>, grid, blk, 0, s, y, scale, shift, wout, bias, target, P, C, k, o, dout, parts); break;
        case 16: hipLaunchKernelGGL(l1_out_kernel<16>, grid, blk, 0, s, y, scale, shift, wout, bias, target, P, C, k, o, dout, parts); break;
        default: hipLaunchKernelGGL(l1_out_kernel<1>, grid, blk, 0, s, y, scale, shift, wout, bias, target, P, C, k, o, dout, parts); break;
    }
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), blk, 0, s, parts, nblk, (double)gscale / (double)P, loss);
    return check_launch("unet_l1_out");
}

extern "C" int dcs_unet_upsample2_pad_backward(const float* dcat, int cstride, int N, int h, int w, int C, int Ho,
                                               int Wo, float* dx, void* stream) {
    if (!dcat || !dx || dcat == dx) return fail(DCS_E_INVALID, "unet_upsample2_pad_backward: null or aliased pointers");
    if (N <= 0 || h <= 0 || w <= 0 || C <= 0 || C % 4 != 0 || h >= (1 << 29) || w >= (1 << 29) ||
        (long double)N * h * w * C >= (long double)TR_MAX_THREADS)
        return fail(DCS_E_INVALID, "unet_upsample2_pad_backward: bad dimensions (C % 4 == 0)");
    if (Ho < 2 * h || Wo < 2 * w)
        return fail(DCS_E_INVALID, "unet_upsample2_pad_backward: the upsampled map is larger than the gradient");
    if (cstride < C || cstride % 4 != 0 || (long double)N * Ho * Wo * cstride >= (long double)TR_MAX_THREADS)
        return fail(DCS_E_INVALID, "unet_upsample2_pad_backward: cstride must be >= C and a multiple of 4");
    if (!al16(dcat) || !al16(dx)) return fail(DCS_E_INVALID, "unet_upsample2_pad_backward: pointers must be 16-byte aligned");
    const int64_t nthreads = (int64_t)N * h * w * (C / 4);
    const int pt = (Ho - 2 * h) / 2, pl = (Wo - 2 * w) / 2;
    const float ry = h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.f;
    const float rx = w > 1 ? (float)(w - 1) / (float)(2 * w - 1) : 0.f;
    hipLaunchKernelGGL(upsample2_pad_bwd_kernel, dim3((unsigned)cdiv(nthreads, TT)), dim3(TT), 0, as_stream(stream),
                       dcat, cstride, nthreads, h, w, C, Ho, Wo, pt, pl, ry, rx, dx);
    return check_launch("unet_upsample2_pad_backward");
}

extern "C" size_t dcs_unet_sumsq_workspace_size(int64_t n) {
    if (n <= 0) return 0;
    return (size_t)cdiv(n, sumsq_per(n)) * sizeof(double);
}

extern "C" int dcs_unet_sumsq(const float* g, int64_t n, float clip, float* out, void* ws, size_t ws_bytes,
                              void* stream) {
    if (!g || !out || !ws || n <= 0) return fail(DCS_E_INVALID, "unet_sumsq: bad arguments");
    if (!al4(g) || !al4(out) || (reinterpret_cast<uintptr_t>(ws) % 8) != 0)
        return fail(DCS_E_INVALID, "unet_sumsq: misaligned pointer");
    if (ws_bytes < dcs_unet_sumsq_workspace_size(n)) return fail(DCS_E_WORKSPACE, "unet_sumsq: workspace too small");
    const int64_t per = sumsq_per(n);
    const int64_t nblk = cdiv(n, per);
    hipStream_t s = as_stream(stream);
    double* parts = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)nblk), dim3(TT), 0, s, g, n, per, parts);
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(TT), 0, s, parts, nblk, clip, out);
    return check_launch("unet_sumsq");
}
