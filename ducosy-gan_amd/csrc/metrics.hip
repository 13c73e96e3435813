// Evaluation metrics of calculate.py on gfx950 (modules/metrics.py on the host): MAE, PSNR, cosine
// similarity and the min/max of a volume pair from one pass, per-slice SSIM, the Sobel texture
// similarity, the per-slice normalised Euclidean distance and the L1 distance of two row-sorted
// volumes (the Wasserstein-1 distance of EMD), and the levels of MS-SSIM (the per-slice sums of one
// level and the 2x2 pooling between levels), and the region-wise sums of calculate.py --regions
// (per HU-range owner and over the true enhancement: counts, error sums, the SSIM map).  Dense
// float32 [D][H][W] volumes, x fastest; every result is float64 per slice.
//
// Arithmetic (the spec modules/metrics.py follows too): the reference's numpy elementwise
// expressions stay in float32, one IEEE operation per step (a - b, its square, the (x - off) / div
// normalisations), every sum accumulates in float64, SSIM and Sobel run in float64 on the float32
// samples.  No multiply-add is contracted in this file.
//
// No floating-point atomics: a workgroup reduces its chunk or tile in a fixed order and writes
// float64 partials to the caller's workspace, fold_kernel combines the partials of one slice in
// index order.  Results are bit-identical from run to run.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int MT = 256;        // threads per block of every kernel here
constexpr int PCH = DCS_MET_PAIR_CHUNK;  // elements of one slice per block of the pair kernels
constexpr int TX = DCS_MET_TILE_X, TY = DCS_MET_TILE_Y;  // output tile of the SSIM and Sobel kernels
constexpr int SR = TY / (MT / TX);                       // output rows per thread: 4 strips of 8
constexpr int NSTAT = DCS_MET_NSTATS;
static_assert(PCH % (MT * 4) == 0, "whole vectors per chunk");
static_assert(TX == 64 && MT % TX == 0 && TY % (MT / TX) == 0, "one wave per strip of the tile");

// x -> (x - off) / div in float32 (numpy's normalisations); div == 0 gives 0 (normalize() of a
// constant volume); ident skips the arithmetic
struct Aff {
    float off, div;
    int ident;
};
__device__ __forceinline__ float aff(float x, const Aff& t) {
    if (t.ident) return x;  // kernel argument: wave-uniform
    return t.div == 0.f ? 0.f : (x - t.off) / t.div;
}

enum { OP_ADD = 0, OP_MIN = 1, OP_MAX = 2 };
template <int OP>
__device__ __forceinline__ double comb(double a, double b) {
    return OP == OP_ADD ? a + b : (OP == OP_MIN ? fmin(a, b) : fmax(a, b));
}
// block-wide reduction in a fixed order; red: MT / WAVE doubles; the result is valid in every thread
template <int OP>
__device__ __forceinline__ double block_red(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = comb<OP>(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return comb<OP>(comb<OP>(red[0], red[1]), comb<OP>(red[2], red[3]));
}

// scipy 'reflect' (d c b a | a b c d | d c b a), repeated for any i
__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// One pass over chunk p of slice z of both volumes.
//   PM_STATS: sum|a-b|, sum (a-b)^2, sum ab, sum a^2, sum b^2, min a, max a, min b, max b
//   PM_L1:    sum|a-b|
//   PM_ED:    sum (a_n - b_n)^2 with each slice normalised by its own min / max + 1e-8f, read
//             from the PM_STATS record of the slice
enum { PM_STATS = 0, PM_L1 = 1, PM_ED = 2 };
template <int MODE, int VEC>
__global__ void __launch_bounds__(MT) pair_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t S,
                                                  int P, Aff ta, Aff tb, const double* __restrict__ stats,
                                                  double* __restrict__ ws) {
    __shared__ double red[MT / WAVE];
    const int64_t z = blockIdx.x / (unsigned)P;
    const int p = (int)(blockIdx.x % (unsigned)P);
    if (MODE == PM_ED) {
        const double* st = stats + z * NSTAT;
        ta.off = (float)st[5];
        ta.div = (float)st[6] - ta.off + 1e-8f;
        tb.off = (float)st[7];
        tb.div = (float)st[8] - tb.off + 1e-8f;
        ta.ident = tb.ident = 0;
    }
    const float* __restrict__ pa = a + z * S;
    const float* __restrict__ pb = b + z * S;
    const int64_t start = (int64_t)p * PCH;
    const int64_t end = start + PCH < S ? start + PCH : S;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    float mna = INFINITY, mxa = -INFINITY, mnb = INFINITY, mxb = -INFINITY;
    using VF = float __attribute__((ext_vector_type(VEC)));
#pragma unroll 2
    for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += MT * VEC) {  // S % VEC == 0
        float va[VEC], vb[VEC];
        if (VEC == 1) {
            va[0] = pa[i];
            vb[0] = pb[i];
        } else {
            const VF qa = *reinterpret_cast<const VF*>(pa + i);
            const VF qb = *reinterpret_cast<const VF*>(pb + i);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                va[v] = qa[v];
                vb[v] = qb[v];
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float x = aff(va[v], ta), y = aff(vb[v], tb);
            const float d = x - y;
            if (MODE == PM_ED) {
                s0 += (double)d * (double)d;
            } else {
                s0 += (double)fabsf(d);
            }
            if (MODE == PM_STATS) {
                const float q = d * d;
                s1 += (double)q;
                s2 += (double)x * (double)y;
                s3 += (double)x * (double)x;
                s4 += (double)y * (double)y;
                mna = fminf(mna, x);
                mxa = fmaxf(mxa, x);
                mnb = fminf(mnb, y);
                mxb = fmaxf(mxb, y);
            }
        }
    }
    double* out = ws + (int64_t)blockIdx.x * (MODE == PM_STATS ? NSTAT : 1);
    s0 = block_red<OP_ADD>(s0, red);
    if (MODE == PM_STATS) {
        s1 = block_red<OP_ADD>(s1, red);
        s2 = block_red<OP_ADD>(s2, red);
        s3 = block_red<OP_ADD>(s3, red);
        s4 = block_red<OP_ADD>(s4, red);
        const double r5 = block_red<OP_MIN>((double)mna, red), r6 = block_red<OP_MAX>((double)mxa, red);
        const double r7 = block_red<OP_MIN>((double)mnb, red), r8 = block_red<OP_MAX>((double)mxb, red);
        if (threadIdx.x == 0) {
            out[1] = s1, out[2] = s2, out[3] = s3, out[4] = s4;
            out[5] = r5, out[6] = r6, out[7] = r7, out[8] = r8;
        }
    }
    if (threadIdx.x == 0) out[0] = s0;
}

// out[z][k] = the partials ws[z][0..P)[k] combined in index order; ops holds two bits per k (K <= 32)
__global__ void __launch_bounds__(MT) fold_kernel(const double* __restrict__ ws, int D, int P, int K, uint64_t ops,
                                                  double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= (int64_t)D * K) return;
    const int64_t z = i / K;
    const int k = (int)(i % K);
    const int op = (int)((ops >> (2 * k)) & 3u);
    const double* w = ws + z * P * K + k;
    double v = w[0];
    for (int p = 1; p < P; ++p) {
        const double u = w[(int64_t)p * K];
        v = op == OP_ADD ? v + u : (op == OP_MIN ? fmin(v, u) : fmax(v, u));
    }
    out[i] = v;
}

// The SSIM map of one TX x TY tile of the interior (H-6) x (W-6) of a slice.  The interior's 7x7
// windows lie inside the image, so the 'reflect' border of the filters is never read.  The tile
// and its 6-pixel halo are staged in LDS (ssim_stage); a thread owns one column of a strip of SR
// rows, walks down SR + 6 input rows, forms the five horizontal 7-sums of each once and keeps the
// last seven in registers (the column sums are reused by seven outputs), and hands every map value
// of its column to emit(row in the strip, value).
// With N = 49 and the window sums sx, sy, sxx, syy, sxy (float64) the factors N^2 cancel in
//   S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  v = N/(N-1) (u.. - u.u.):
//   S = ((2 sx sy + c1)((N sxy - sx sy) 49/24 + c2)) / ((sx^2 + sy^2 + c1)((N (sxx + syy) - sx^2 - sy^2) 49/48 + c2))
// with c1 = C1 N^2, c2 = C2 N^2: one division per pixel, and exact on integer-valued data.
// ssim_kernel sums the map over the tile, region_ssim_kernel per region: both read this map.
using SsimTile = float[TY + 6][TX + 6];
__device__ __forceinline__ void ssim_stage(const float* __restrict__ pa, const float* __restrict__ pb, int H, int W,
                                           int tx0, int ty0, const Aff& ta, const Aff& tb, SsimTile& sa, SsimTile& sb) {
    for (int i = threadIdx.x; i < (TY + 6) * (TX + 6); i += MT) {
        const int r = i / (TX + 6), c = i % (TX + 6);
        const int y = ty0 + r, x = tx0 + c;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            va = aff(pa[(int64_t)y * W + x], ta);
            vb = aff(pb[(int64_t)y * W + x], tb);
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
}
template <class Emit>
__device__ __forceinline__ void ssim_strip(const SsimTile& sa, const SsimTile& sb, int r0, int cx, double c1, double c2,
                                           Emit&& emit) {
    double ring[7][5];
#pragma unroll
    for (int i = 0; i < SR + 6; ++i) {
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double x = (double)sa[r0 + i][cx + k], y = (double)sb[r0 + i][cx + k];
            m0 += x;
            m1 += y;
            m2 += x * x;
            m3 += y * y;
            m4 += x * y;
        }
        ring[i % 7][0] = m0, ring[i % 7][1] = m1, ring[i % 7][2] = m2, ring[i % 7][3] = m3, ring[i % 7][4] = m4;
        if (i >= 6) {
            double s[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                s[q] = ring[(i - 6) % 7][q];
#pragma unroll
                for (int j = i - 5; j <= i; ++j) s[q] += ring[j % 7][q];
            }
            const double sxsy = s[0] * s[1], sx2 = s[0] * s[0], sy2 = s[1] * s[1];
            const double A1 = 2.0 * sxsy + c1;
            const double A2 = (49.0 * s[4] - sxsy) * (49.0 / 24.0) + c2;
            const double B1 = sx2 + sy2 + c1;
            const double B2 = (49.0 * (s[2] + s[3]) - sx2 - sy2) * (49.0 / 48.0) + c2;
            emit(i - 6, (A1 * A2) / (B1 * B2));
        }
    }
}

// Sum of the SSIM map over one tile of the interior of slice z.
__global__ void __launch_bounds__(MT) ssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                  int ntx, int nty, Aff ta, Aff tb, double c1, double c2,
                                                  double* __restrict__ ws) {
    __shared__ SsimTile sa, sb;
    __shared__ double red[MT / WAVE];
    const unsigned ntile = (unsigned)(ntx * nty);
    const int64_t z = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x % ntile);
    const int tx0 = (tile % ntx) * TX, ty0 = (tile / ntx) * TY;
    ssim_stage(a + z * H * W, b + z * H * W, H, W, tx0, ty0, ta, tb, sa, sb);
    __syncthreads();
    const int Ho = H - 6, Wo = W - 6;
    const int cx = threadIdx.x & (TX - 1), r0 = (int)(threadIdx.x / TX) * SR;
    const bool col_ok = tx0 + cx < Wo;
    double acc = 0.0;
    if (ty0 + r0 < Ho)  // wave-uniform: a strip is one wave
        ssim_strip(sa, sb, r0, cx, c1, c2, [&](int j, double v) {
            if (col_ok && ty0 + r0 + j < Ho) acc += v;
        });
    acc = block_red<OP_ADD>(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
}

// Region-wise evaluation (calculate.py --regions; modules/metrics.py::region_sums states it).  A
// voxel's owner follows synthesis(): lung where lung_min <= vue <= lung_max, else soft where
// soft_min <= vue <= soft_max, else rest; over these lies the true enhancement (std - vue) > thr
// and vue > min_hu, and the predicted one with gen in place of std.  float32 comparisons on
// float32 differences, as synthesize_enhancement takes them.
constexpr int NREG = 4, NRS = DCS_MET_REGION_NSUMS, NRSS = DCS_MET_REGION_NSSIM;
enum { RG_LUNG = 0, RG_SOFT = 1, RG_REST = 2, RG_ENH = 3, RG_ENH_BIT = 4 };  // map byte: owner | RG_ENH_BIT
static_assert(NRS == 4 * NREG + 5 && NRSS == 2 * NREG && NRS <= MT && NRS <= 32, "one thread and two fold bits per column");
struct RegionRanges {
    float lung_min, lung_max, soft_min, soft_max, thr, min_hu;
};

// the N sums of a block in a fixed order: lanes by shuffles, then the four waves through LDS;
// thread k < N writes out[k]
template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N], double (*red)[MT / WAVE], double* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const double* r = red[threadIdx.x];
        out[threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// One pass over chunk p of slice z of the three series, 12 bytes per voxel.  Writes the block's
// record of NRS sums: per region n, sum|std-gen|, sum f32((std-gen)^2), sum (gen-std), then TP,
// FP, FN of the predicted against the true enhancement and sum (std-vue), sum (gen-vue) over the
// true one; and, if asked, one byte per voxel (owner | RG_ENH_BIT) for region_ssim_kernel.
template <int VEC>
__global__ void __launch_bounds__(MT) region_kernel(const float* __restrict__ vue, const float* __restrict__ std_,
                                                    const float* __restrict__ gen, int64_t S, int P, RegionRanges rr,
                                                    unsigned char* __restrict__ map, double* __restrict__ ws) {
    __shared__ double red[NRS][MT / WAVE];
    const int64_t z = blockIdx.x / (unsigned)P;
    const int p = (int)(blockIdx.x % (unsigned)P);
    const float* __restrict__ pv = vue + z * S;
    const float* __restrict__ ps = std_ + z * S;
    const float* __restrict__ pg = gen + z * S;
    unsigned char* __restrict__ pm = map ? map + z * S : nullptr;  // kernel argument: wave-uniform
    const int64_t start = (int64_t)p * PCH;
    const int64_t end = start + PCH < S ? start + PCH : S;
    int cnt[NREG] = {0, 0, 0, 0}, tp = 0, fp = 0, fn = 0;
    double sab[NREG] = {0.0, 0.0, 0.0, 0.0}, ssq[NREG] = {0.0, 0.0, 0.0, 0.0}, sbi[NREG] = {0.0, 0.0, 0.0, 0.0};
    double set = 0.0, sep = 0.0;
    using VF = float __attribute__((ext_vector_type(VEC)));
    using VB = unsigned char __attribute__((ext_vector_type(VEC)));
#pragma unroll 1
    for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += MT * VEC) {  // S % VEC == 0
        float vv[VEC], vs[VEC], vg[VEC];
        unsigned char mb[VEC];
        if (VEC == 1) {
            vv[0] = pv[i];
            vs[0] = ps[i];
            vg[0] = pg[i];
        } else {
            const VF qv = *reinterpret_cast<const VF*>(pv + i);
            const VF qs = *reinterpret_cast<const VF*>(ps + i);
            const VF qg = *reinterpret_cast<const VF*>(pg + i);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                vv[v] = qv[v];
                vs[v] = qs[v];
                vg[v] = qg[v];
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float x = vv[v], s = vs[v], g = vg[v];
            const float d = s - g, q = d * d, b = g - s;
            const float et = s - x, ep = g - x;
            const bool lung = x >= rr.lung_min && x <= rr.lung_max;
            const bool soft = !lung && x >= rr.soft_min && x <= rr.soft_max;
            const int own = lung ? RG_LUNG : (soft ? RG_SOFT : RG_REST);
            const bool valid = x > rr.min_hu;
            const bool te = et > rr.thr && valid, pe = ep > rr.thr && valid;
            mb[v] = (unsigned char)(own | (te ? RG_ENH_BIT : 0));
            const double da = (double)fabsf(d), dq = (double)q, db = (double)b;
#pragma unroll
            for (int r = 0; r < NREG; ++r) {
                const bool in = r == RG_ENH ? te : own == r;
                cnt[r] += in ? 1 : 0;
                sab[r] += in ? da : 0.0;
                ssq[r] += in ? dq : 0.0;
                sbi[r] += in ? db : 0.0;
            }
            tp += (te && pe) ? 1 : 0;
            fp += (!te && pe) ? 1 : 0;
            fn += (te && !pe) ? 1 : 0;
            set += te ? (double)et : 0.0;
            sep += te ? (double)ep : 0.0;
        }
        if (pm) {
            if (VEC == 1) {
                pm[i] = mb[0];
            } else {
                VB qm;
#pragma unroll
                for (int v = 0; v < VEC; ++v) qm[v] = mb[v];
                *reinterpret_cast<VB*>(pm + i) = qm;
            }
        }
    }
    double rec[NRS];  // a thread counts at most PCH / MT voxels: exact in int and in double
#pragma unroll
    for (int r = 0; r < NREG; ++r) rec[4 * r] = (double)cnt[r], rec[4 * r + 1] = sab[r], rec[4 * r + 2] = ssq[r], rec[4 * r + 3] = sbi[r];
    rec[16] = (double)tp, rec[17] = (double)fp, rec[18] = (double)fn, rec[19] = set, rec[20] = sep;
    block_sum_n<NRS>(rec, red, ws + (int64_t)blockIdx.x * NRS);
}

// The SSIM map of (std, gen) over one tile of the interior of slice z, as ssim_kernel forms it,
// summed per region: the block's record is {count, sum} of lung, soft, rest and the true
// enhancement.  A pixel's regions come from the byte region_kernel wrote for it (1 byte read per
// output pixel; no halo: only the outputs are classified).
__global__ void __launch_bounds__(MT) region_ssim_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         const unsigned char* __restrict__ map, int H, int W, int ntx,
                                                         int nty, double c1, double c2, double* __restrict__ ws) {
    __shared__ SsimTile sa, sb;
    __shared__ double red[NRSS][MT / WAVE];
    const unsigned ntile = (unsigned)(ntx * nty);
    const int64_t z = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x % ntile);
    const int tx0 = (tile % ntx) * TX, ty0 = (tile / ntx) * TY;
    const int Ho = H - 6, Wo = W - 6;
    const int cx = threadIdx.x & (TX - 1), r0 = (int)(threadIdx.x / TX) * SR;
    const bool col_ok = tx0 + cx < Wo;
    // output (y, x) of the interior is pixel (y + 3, x + 3) of the slice
    const unsigned char* __restrict__ pm = map + z * H * W + (int64_t)(ty0 + r0 + 3) * W + (tx0 + cx + 3);
    unsigned char mb[SR];
#pragma unroll
    for (int j = 0; j < SR; ++j) mb[j] = (col_ok && ty0 + r0 + j < Ho) ? pm[(int64_t)j * W] : (unsigned char)0xff;
    Aff id;
    id.off = 0.f, id.div = 1.f, id.ident = 1;
    ssim_stage(a + z * H * W, b + z * H * W, H, W, tx0, ty0, id, id, sa, sb);
    __syncthreads();
    double rec[NRSS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ty0 + r0 < Ho)  // wave-uniform: a strip is one wave
        ssim_strip(sa, sb, r0, cx, c1, c2, [&](int j, double v) {
            const int m = mb[j];  // 0xff outside the interior: no owner, and skipped
            if (m != 0xff) {
#pragma unroll
                for (int r = 0; r < NREG; ++r) {
                    const bool in = r == RG_ENH ? (m & RG_ENH_BIT) != 0 : (m & 3) == r;
                    rec[2 * r] += in ? 1.0 : 0.0;
                    rec[2 * r + 1] += in ? v : 0.0;
                }
            }
        });
    block_sum_n<NRSS>(rec, red, ws + (int64_t)blockIdx.x * NRSS);
}

// skimage.filters.sobel of both slices on the fly over one TX x TY tile, 'reflect' border:
// h = ([1,2,1]/4 along x)([1,0,-1] along y), v its transpose, g = sqrt((h^2 + v^2) / 2) in
// float64.  Writes sum|g1 - g2|, max g1, max g2 of the tile; no gradient plane goes to memory.
// A thread walks down SR + 2 rows of its column and keeps the x-smoothed and x-differenced
// values of the last three.
__global__ void __launch_bounds__(MT) sobel_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                   int ntx, int nty, double* __restrict__ ws) {
    __shared__ float sa[TY + 2][TX + 2], sb[TY + 2][TX + 2];
    __shared__ double red[MT / WAVE];
    const unsigned ntile = (unsigned)(ntx * nty);
    const int64_t z = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x % ntile);
    const int tx0 = (tile % ntx) * TX, ty0 = (tile / ntx) * TY;
    const float* __restrict__ pa = a + z * H * W;
    const float* __restrict__ pb = b + z * H * W;
    for (int i = threadIdx.x; i < (TY + 2) * (TX + 2); i += MT) {
        const int r = i / (TX + 2), c = i % (TX + 2);
        const int64_t src = (int64_t)reflect_idx(ty0 - 1 + r, H) * W + reflect_idx(tx0 - 1 + c, W);
        sa[r][c] = pa[src];
        sb[r][c] = pb[src];
    }
    __syncthreads();
    const int cx = threadIdx.x & (TX - 1), r0 = (int)(threadIdx.x / TX) * SR;
    const bool col_ok = tx0 + cx < W;
    double acc = 0.0, mx1 = 0.0, mx2 = 0.0;
    if (ty0 + r0 < H) {  // wave-uniform
        double sm1[3], df1[3], sm2[3], df2[3];
#pragma unroll
        for (int i = 0; i < SR + 2; ++i) {
            {
                const double l = (double)sa[r0 + i][cx], c = (double)sa[r0 + i][cx + 1], r = (double)sa[r0 + i][cx + 2];
                sm1[i % 3] = c * 0.5 + (l + r) * 0.25;
                df1[i % 3] = l - r;
            }
            {
                const double l = (double)sb[r0 + i][cx], c = (double)sb[r0 + i][cx + 1], r = (double)sb[r0 + i][cx + 2];
                sm2[i % 3] = c * 0.5 + (l + r) * 0.25;
                df2[i % 3] = l - r;
            }
            if (i >= 2) {
                const int u = (i - 2) % 3, m = (i - 1) % 3, d = i % 3;
                const double h1 = sm1[u] - sm1[d], v1 = df1[m] * 0.5 + (df1[u] + df1[d]) * 0.25;
                const double h2 = sm2[u] - sm2[d], v2 = df2[m] * 0.5 + (df2[u] + df2[d]) * 0.25;
                const double g1 = sqrt((h1 * h1 + v1 * v1) * 0.5), g2 = sqrt((h2 * h2 + v2 * v2) * 0.5);
                if (col_ok && ty0 + r0 + i - 2 < H) {
                    acc += fabs(g1 - g2);
                    mx1 = fmax(mx1, g1);
                    mx2 = fmax(mx2, g2);
                }
            }
        }
    }
    acc = block_red<OP_ADD>(acc, red);
    mx1 = block_red<OP_MAX>(mx1, red);
    mx2 = block_red<OP_MAX>(mx2, red);
    if (threadIdx.x == 0) {
        double* out = ws + (int64_t)blockIdx.x * 3;
        out[0] = acc, out[1] = mx1, out[2] = mx2;
    }
}

// One level of MS-SSIM (torchmetrics' defaults, restated in modules/metrics.py::ms_ssim_levels):
// the sums of the SSIM map and of its contrast-structure factor over one TX x TY tile of the
// interior (H-10) x (W-10) of slice z, whose 11x11 windows lie inside the image.  The tile and its
// 10-pixel halo are staged in LDS; a thread owns one column of a strip of SR rows, walks down
// SR + 10 input rows, filters x, y, x^2, y^2 and xy of each along the row once (taps in ascending
// order, float64) and keeps the last eleven rows' values in registers, which the column filter
// of eleven outputs reuses.  The window comes from the host as eleven doubles, so both paths
// filter with the same bits.
//   cs = (2 sxy + c2) / (sx2 + sy2 + c2),  sim = ((2 ux uy + c1)(2 sxy + c2)) / ((ux^2 + uy^2 + c1)(sx2 + sy2 + c2))
// with sx2 = E[x^2] - ux^2 and so on (no N/(N-1) factor).  Writes {sum sim, sum cs} of the tile.
constexpr int MSW = DCS_MET_MSSSIM_TAPS, MSH = MSW - 1;  // window taps and halo
struct MsWin {
    double g[MSW];
};
__global__ void __launch_bounds__(MT) msssim_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                    int ntx, int nty, MsWin win, double c1, double c2,
                                                    double* __restrict__ ws) {
    __shared__ float sa[TY + MSH][TX + MSH], sb[TY + MSH][TX + MSH];
    __shared__ double red[MT / WAVE];
    const unsigned ntile = (unsigned)(ntx * nty);
    const int64_t z = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x % ntile);
    const int tx0 = (tile % ntx) * TX, ty0 = (tile / ntx) * TY;
    const float* __restrict__ pa = a + z * H * W;
    const float* __restrict__ pb = b + z * H * W;
    for (int i = threadIdx.x; i < (TY + MSH) * (TX + MSH); i += MT) {
        const int r = i / (TX + MSH), c = i % (TX + MSH);
        const int y = ty0 + r, x = tx0 + c;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {
            va = pa[(int64_t)y * W + x];
            vb = pb[(int64_t)y * W + x];
        }
        sa[r][c] = va;
        sb[r][c] = vb;
    }
    __syncthreads();
    const int Ho = H - MSH, Wo = W - MSH;
    const int cx = threadIdx.x & (TX - 1), r0 = (int)(threadIdx.x / TX) * SR;
    const bool col_ok = tx0 + cx < Wo;
    double acc_sim = 0.0, acc_cs = 0.0;
    if (ty0 + r0 < Ho) {  // wave-uniform: a strip is one wave
        double ring[MSW][5];
#pragma unroll
        for (int i = 0; i < SR + MSH; ++i) {
            double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
            for (int k = 0; k < MSW; ++k) {
                const double x = (double)sa[r0 + i][cx + k], y = (double)sb[r0 + i][cx + k];
                const double g = win.g[k];
                m0 += g * x;
                m1 += g * y;
                m2 += g * (x * x);
                m3 += g * (y * y);
                m4 += g * (x * y);
            }
            ring[i % MSW][0] = m0, ring[i % MSW][1] = m1, ring[i % MSW][2] = m2, ring[i % MSW][3] = m3,
                          ring[i % MSW][4] = m4;
            if (i >= MSH) {
                double s[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    s[q] = 0.0;
#pragma unroll
                    for (int j = 0; j < MSW; ++j) s[q] += win.g[j] * ring[(i - MSH + j) % MSW][q];
                }
                const double uxuy = s[0] * s[1], ux2 = s[0] * s[0], uy2 = s[1] * s[1];
                const double upper = 2.0 * (s[4] - uxuy) + c2;
                const double lower = (s[2] - ux2) + (s[3] - uy2) + c2;
                const double cs = upper / lower;
                const double sim = ((2.0 * uxuy + c1) * upper) / ((ux2 + uy2 + c1) * lower);
                if (col_ok && ty0 + r0 + i - MSH < Ho) {
                    acc_sim += sim;
                    acc_cs += cs;
                }
            }
        }
    }
    acc_sim = block_red<OP_ADD>(acc_sim, red);
    acc_cs = block_red<OP_ADD>(acc_cs, red);
    if (threadIdx.x == 0) {
        double* out = ws + (int64_t)blockIdx.x * 2;
        out[0] = acc_sim, out[1] = acc_cs;
    }
}

// The next MS-SSIM level of both volumes: the 2x2 average with floor sizes (an odd last row or
// column is dropped), float32(((a + b) + c) + d) * 0.25) with the sum in float64.
__global__ void __launch_bounds__(MT) pool2_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                   int Ho, int Wo, int64_t n, float* __restrict__ oa,
                                                   float* __restrict__ ob) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= n) return;
    const int xo = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int yo = (int)(t % Ho);
    const int64_t z = t / Ho;
    const int64_t src = (z * H + 2 * yo) * W + 2 * xo;
    oa[i] = (float)(((((double)a[src] + (double)a[src + 1]) + (double)a[src + W]) + (double)a[src + W + 1]) * 0.25);
    ob[i] = (float)(((((double)b[src] + (double)b[src + 1]) + (double)b[src + W]) + (double)b[src + W + 1]) * 0.25);
}

template <int VEC>
__global__ void __launch_bounds__(MT) normalize_kernel(const float* __restrict__ x, int64_t nvec, Aff t,
                                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x;
    if (i >= nvec) return;
    using VF = float __attribute__((ext_vector_type(VEC)));
    if (VEC == 1) {
        out[i] = aff(x[i], t);
    } else {
        VF q = reinterpret_cast<const VF*>(x)[i];
#pragma unroll
        for (int v = 0; v < VEC; ++v) q[v] = aff(q[v], t);
        reinterpret_cast<VF*>(out)[i] = q;
    }
}

}  // namespace dcs

// Host side: argument checks, workspace sizing and launches.
namespace dcs {

static bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// positive, one slice indexable by int, at most 2^38 voxels, every grid below 2^31 blocks
static bool dims_ok(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return false;
    if ((int64_t)H * W >= (1ll << 30)) return false;
    if ((long double)D * H * W >= (long double)(1ll << 38)) return false;
    return (int64_t)D * cdiv((int64_t)H * W, PCH) < (1ll << 31) && (int64_t)D * cdiv(H, TY) * cdiv(W, TX) < (1ll << 31);
}
static int pair_parts(int H, int W) { return (int)cdiv((int64_t)H * W, PCH); }
static int64_t tiles(int h, int w) { return cdiv(h, TY) * cdiv(w, TX); }

static Aff make_aff(const float* affine, int which) {
    Aff t;
    t.off = affine ? affine[2 * which] : 0.f;
    t.div = affine ? affine[2 * which + 1] : 1.f;
    t.ident = affine ? 0 : 1;
    return t;
}
static bool aff_ok(const float* affine) {
    if (!affine) return true;
    for (int i = 0; i < 4; ++i)
        if (!(affine[i] - affine[i] == 0.f)) return false;  // finite
    return true;
}

static int fold(const double* ws, int D, int P, int K, uint64_t ops, double* out, hipStream_t s, const char* what) {
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)cdiv((int64_t)D * K, MT)), dim3(MT), 0, s, ws, D, P, K, ops, out);
    return check_launch(what);
}

template <int MODE>
static void launch_pair(const float* a, const float* b, int D, int H, int W, Aff ta, Aff tb, const double* stats,
                        double* ws, hipStream_t s) {
    const int64_t S = (int64_t)H * W;
    const int P = pair_parts(H, W);
    const dim3 grid((unsigned)((int64_t)D * P));
    if (S % 4 == 0 && aligned(a, 16) && aligned(b, 16))
        hipLaunchKernelGGL((pair_kernel<MODE, 4>), grid, dim3(MT), 0, s, a, b, S, P, ta, tb, stats, ws);
    else
        hipLaunchKernelGGL((pair_kernel<MODE, 1>), grid, dim3(MT), 0, s, a, b, S, P, ta, tb, stats, ws);
}

// the checks every pair entry point shares; DCS_OK when the call is good
static int pair_args(const char* name, const float* a, const float* b, int D, int H, int W, const double* out,
                     const void* ws, size_t ws_bytes, int64_t parts_per_slice, int K) {
    const char* bad = nullptr;
    int code = DCS_E_INVALID;
    if (!a || !b || !out || !ws)
        bad = ": null pointer";
    else if (!dims_ok(D, H, W))
        bad = ": bad dimensions";
    else if (!aligned(a, 4) || !aligned(b, 4) || !aligned(out, 8) || !aligned(ws, 8))
        bad = ": misaligned pointer";
    else if (ws_bytes < sizeof(double) * (size_t)K * (size_t)D * (size_t)parts_per_slice)
        bad = ": workspace too small", code = DCS_E_WORKSPACE;
    if (!bad) return DCS_OK;
    set_error(std::string(name) + bad);
    return code;
}

}  // namespace dcs

using namespace dcs;

extern "C" size_t dcs_met_workspace_size(int D, int H, int W) {
    if (!dims_ok(D, H, W)) return 0;
    const int64_t pair = (int64_t)pair_parts(H, W) * NSTAT, tile = tiles(H, W) * 3;
    return (size_t)((pair > tile ? pair : tile) * D) * sizeof(double);
}

extern "C" int dcs_met_pair_stats(const float* a, const float* b, int D, int H, int W, const float* affine,
                                  double* out, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = pair_args("met_pair_stats", a, b, D, H, W, out, ws, ws_bytes, cdiv((int64_t)H * W, PCH), NSTAT)) return rc;
    if (!aff_ok(affine)) return fail(DCS_E_INVALID, "met_pair_stats: affine must be finite");
    hipStream_t s = as_stream(stream);
    launch_pair<PM_STATS>(a, b, D, H, W, make_aff(affine, 0), make_aff(affine, 1), nullptr, static_cast<double*>(ws), s);
    // five sums, then min a, max a, min b, max b
    const unsigned ops = (OP_MIN << 10) | (OP_MAX << 12) | (OP_MIN << 14) | (OP_MAX << 16);
    return fold(static_cast<const double*>(ws), D, pair_parts(H, W), NSTAT, ops, out, s, "met_pair_stats");
}

extern "C" int dcs_met_sorted_l1(const float* a, const float* b, int D, int H, int W, const float* affine, double* out,
                                 void* ws, size_t ws_bytes, void* stream) {
    if (int rc = pair_args("met_sorted_l1", a, b, D, H, W, out, ws, ws_bytes, cdiv((int64_t)H * W, PCH), 1)) return rc;
    if (!aff_ok(affine)) return fail(DCS_E_INVALID, "met_sorted_l1: affine must be finite");
    hipStream_t s = as_stream(stream);
    launch_pair<PM_L1>(a, b, D, H, W, make_aff(affine, 0), make_aff(affine, 1), nullptr, static_cast<double*>(ws), s);
    return fold(static_cast<const double*>(ws), D, pair_parts(H, W), 1, OP_ADD, out, s, "met_sorted_l1");
}

extern "C" int dcs_met_ed(const float* a, const float* b, int D, int H, int W, const double* stats, double* out,
                          void* ws, size_t ws_bytes, void* stream) {
    if (int rc = pair_args("met_ed", a, b, D, H, W, out, ws, ws_bytes, cdiv((int64_t)H * W, PCH), 1)) return rc;
    if (!stats || !aligned(stats, 8) || stats == out) return fail(DCS_E_INVALID, "met_ed: bad stats pointer");
    hipStream_t s = as_stream(stream);
    const Aff id = make_aff(nullptr, 0);
    launch_pair<PM_ED>(a, b, D, H, W, id, id, stats, static_cast<double*>(ws), s);
    return fold(static_cast<const double*>(ws), D, pair_parts(H, W), 1, OP_ADD, out, s, "met_ed");
}

extern "C" int dcs_met_ssim(const float* a, const float* b, int D, int H, int W, const float* affine, double data_range,
                            double* out, void* ws, size_t ws_bytes, void* stream) {
    if (H < 7 || W < 7) return fail(DCS_E_INVALID, "met_ssim: the 7x7 window exceeds the image");
    if (int rc = pair_args("met_ssim", a, b, D, H, W, out, ws, ws_bytes, tiles(H - 6, W - 6), 1)) return rc;
    if (!aff_ok(affine) || !(data_range - data_range == 0.0) || data_range < 0.0)
        return fail(DCS_E_INVALID, "met_ssim: affine and data_range must be finite, data_range >= 0");
    const int ntx = (int)cdiv(W - 6, TX), nty = (int)cdiv(H - 6, TY);
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)((int64_t)D * ntx * nty)), dim3(MT), 0, s, a, b, H, W, ntx, nty,
                       make_aff(affine, 0), make_aff(affine, 1), C1 * 2401.0, C2 * 2401.0, static_cast<double*>(ws));
    // out[z] = the sum of the map; the caller divides by (H-6)(W-6)
    return fold(static_cast<const double*>(ws), D, ntx * nty, 1, OP_ADD, out, s, "met_ssim");
}

// region records per slice: NRS per chunk of the one-pass kernel, NRSS per SSIM tile (none below 7)
static int64_t region_parts(int H, int W) {
    const int64_t pair = (int64_t)pair_parts(H, W) * NRS, tile = (H < 7 || W < 7) ? 0 : tiles(H - 6, W - 6) * NRSS;
    return pair > tile ? pair : tile;
}

extern "C" size_t dcs_met_region_workspace_size(int D, int H, int W) {
    if (!dims_ok(D, H, W)) return 0;
    return (size_t)(region_parts(H, W) * D) * sizeof(double);
}

extern "C" int dcs_met_region_sums(const float* vue, const float* std_, const float* gen, int D, int H, int W,
                                   const float* ranges, double* out, unsigned char* region_map, void* ws,
                                   size_t ws_bytes, void* stream) {
    if (!vue) return fail(DCS_E_INVALID, "met_region_sums: null pointer");
    if (int rc = pair_args("met_region_sums", std_, gen, D, H, W, out, ws, ws_bytes, pair_parts(H, W), NRS)) return rc;
    if (!aligned(vue, 4)) return fail(DCS_E_INVALID, "met_region_sums: misaligned pointer");
    if (!ranges) return fail(DCS_E_INVALID, "met_region_sums: null ranges");
    for (int i = 0; i < 6; ++i)
        if (!(ranges[i] - ranges[i] == 0.f)) return fail(DCS_E_INVALID, "met_region_sums: the ranges must be finite");
    const RegionRanges rr = {ranges[0], ranges[1], ranges[2], ranges[3], ranges[4], ranges[5]};
    const int64_t S = (int64_t)H * W;
    const int P = pair_parts(H, W);
    const dim3 grid((unsigned)((int64_t)D * P));
    hipStream_t s = as_stream(stream);
    if (S % 4 == 0 && aligned(vue, 16) && aligned(std_, 16) && aligned(gen, 16) && aligned(region_map, 4))
        hipLaunchKernelGGL(region_kernel<4>, grid, dim3(MT), 0, s, vue, std_, gen, S, P, rr, region_map,
                           static_cast<double*>(ws));
    else
        hipLaunchKernelGGL(region_kernel<1>, grid, dim3(MT), 0, s, vue, std_, gen, S, P, rr, region_map,
                           static_cast<double*>(ws));
    return fold(static_cast<const double*>(ws), D, P, NRS, OP_ADD, out, s, "met_region_sums");
}

extern "C" int dcs_met_region_ssim(const float* std_, const float* gen, const unsigned char* region_map, int D, int H,
                                   int W, double data_range, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (H < 7 || W < 7) return fail(DCS_E_INVALID, "met_region_ssim: the 7x7 window exceeds the image");
    if (int rc = pair_args("met_region_ssim", std_, gen, D, H, W, out, ws, ws_bytes, tiles(H - 6, W - 6), NRSS)) return rc;
    if (!region_map) return fail(DCS_E_INVALID, "met_region_ssim: null region map");
    if (!(data_range - data_range == 0.0) || data_range < 0.0)
        return fail(DCS_E_INVALID, "met_region_ssim: data_range must be finite and not negative");
    const int ntx = (int)cdiv(W - 6, TX), nty = (int)cdiv(H - 6, TY);
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(region_ssim_kernel, dim3((unsigned)((int64_t)D * ntx * nty)), dim3(MT), 0, s, std_, gen, region_map,
                       H, W, ntx, nty, C1 * 2401.0, C2 * 2401.0, static_cast<double*>(ws));
    // out[z] = {count, sum of the map} per region; the caller divides
    return fold(static_cast<const double*>(ws), D, ntx * nty, NRSS, OP_ADD, out, s, "met_region_ssim");
}

extern "C" int dcs_met_sobel_ts(const float* a, const float* b, int D, int H, int W, double* out, void* ws,
                                size_t ws_bytes, void* stream) {
    if (int rc = pair_args("met_sobel_ts", a, b, D, H, W, out, ws, ws_bytes, tiles(H, W), 3)) return rc;
    const int ntx = (int)cdiv(W, TX), nty = (int)cdiv(H, TY);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(sobel_kernel, dim3((unsigned)((int64_t)D * ntx * nty)), dim3(MT), 0, s, a, b, H, W, ntx, nty,
                       static_cast<double*>(ws));
    return fold(static_cast<const double*>(ws), D, ntx * nty, 3, (OP_MAX << 2) | (OP_MAX << 4), out, s, "met_sobel_ts");
}

extern "C" int dcs_met_msssim_level(const float* a, const float* b, int D, int H, int W, const double* window, double c1,
                                    double c2, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (H < MSW || W < MSW) return fail(DCS_E_INVALID, "met_msssim_level: the 11x11 window exceeds the image");
    if (int rc = pair_args("met_msssim_level", a, b, D, H, W, out, ws, ws_bytes, tiles(H - MSH, W - MSH), 2)) return rc;
    if (!window) return fail(DCS_E_INVALID, "met_msssim_level: null window");
    MsWin win;
    for (int k = 0; k < MSW; ++k) {
        win.g[k] = window[k];
        if (!(win.g[k] - win.g[k] == 0.0)) return fail(DCS_E_INVALID, "met_msssim_level: the window must be finite");
    }
    if (!(c1 - c1 == 0.0) || !(c2 - c2 == 0.0) || c1 < 0.0 || c2 < 0.0)
        return fail(DCS_E_INVALID, "met_msssim_level: c1 and c2 must be finite and not negative");
    const int ntx = (int)cdiv(W - MSH, TX), nty = (int)cdiv(H - MSH, TY);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(msssim_kernel, dim3((unsigned)((int64_t)D * ntx * nty)), dim3(MT), 0, s, a, b, H, W, ntx, nty, win,
                       c1, c2, static_cast<double*>(ws));
    // out[z] = {sum sim, sum cs}; the caller divides by (H-10)(W-10)
    return fold(static_cast<const double*>(ws), D, ntx * nty, 2, OP_ADD, out, s, "met_msssim_level");
}

extern "C" int dcs_met_pool2(const float* a, const float* b, float* out_a, float* out_b, int D, int H, int W,
                             void* stream) {
    if (!a || !b || !out_a || !out_b) return fail(DCS_E_INVALID, "met_pool2: null pointer");
    if (!dims_ok(D, H, W) || H < 2 || W < 2) return fail(DCS_E_INVALID, "met_pool2: bad dimensions");
    if (!aligned(a, 4) || !aligned(b, 4) || !aligned(out_a, 4) || !aligned(out_b, 4))
        return fail(DCS_E_INVALID, "met_pool2: misaligned pointer");
    if (out_a == out_b || out_a == a || out_a == b || out_b == a || out_b == b)
        return fail(DCS_E_INVALID, "met_pool2: the outputs must not alias each other or the inputs");
    const int Ho = H / 2, Wo = W / 2;
    const int64_t n = (int64_t)D * Ho * Wo;
    hipLaunchKernelGGL(pool2_kernel, dim3((unsigned)cdiv(n, MT)), dim3(MT), 0, as_stream(stream), a, b, H, W, Ho, Wo, n,
                       out_a, out_b);
    return check_launch("met_pool2");
}

extern "C" int dcs_met_normalize(const float* x, int64_t n, float off, float div, float* out, void* stream) {
    if (!x || !out) return fail(DCS_E_INVALID, "met_normalize: null pointer");
    if (n <= 0 || n >= (1ll << 38)) return fail(DCS_E_INVALID, "met_normalize: bad element count");
    if (!aligned(x, 4) || !aligned(out, 4)) return fail(DCS_E_INVALID, "met_normalize: misaligned pointer");
    if (!(off - off == 0.f) || !(div - div == 0.f)) return fail(DCS_E_INVALID, "met_normalize: off and div must be finite");
    Aff t;
    t.off = off, t.div = div, t.ident = 0;
    hipStream_t s = as_stream(stream);
    if (n % 4 == 0 && aligned(x, 16) && aligned(out, 16))
        hipLaunchKernelGGL(normalize_kernel<4>, dim3((unsigned)cdiv(n / 4, MT)), dim3(MT), 0, s, x, n / 4, t, out);
    else
        hipLaunchKernelGGL(normalize_kernel<1>, dim3((unsigned)cdiv(n, MT)), dim3(MT), 0, s, x, n, t, out);
    return check_launch("met_normalize");
}
