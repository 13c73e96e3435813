// Training targets of the normal-map U-Net from a voxel-aligned NCCT / CECT pair on gfx950
// (prepare_nmodel_data.py; modules/nmodel/prepare.py::residual_targets states it on the host).
// One pass over the patient: per voxel two 16-bit stored values and, when the sCECT is given, one
// float32 are read and two float32 written (16 bytes, 12 without the sCECT), and the slice's
// statistics are reduced on the way.
//
// Arithmetic: float32, one IEEE operation per step, in the host's order, the division correctly
// rounded; no multiply-add is contracted in this file, so vue and diff equal the host's bit for bit.
// The sums accumulate in float64 (x and y widened before they are multiplied), the counts are exact.
//
// Statistics follow the fixed-order scheme of csrc/metrics.hip: one workgroup per DCS_MET_PAIR_CHUNK
// voxels of a slice reduces its chunk (lanes by shuffles, the four waves through LDS) and writes one
// record of float64 partials to the caller's workspace; a second launch folds the records of a
// slice in index order.  No atomics: results are bit-identical from run to run.
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {

constexpr int NT = 256;                  // threads per block
constexpr int NCH = DCS_MET_PAIR_CHUNK;  // voxels of one slice per block
constexpr int NS = DCS_NMODEL_NSTATS;
constexpr float DIFF_MAX = 4000.0f;      // modules/nmodel/dataset.py DIFF_RANGE[1]
static_assert(NCH % (NT * 4) == 0, "whole vectors per chunk");
static_assert(NS == 11 && NS <= NT, "one thread per column of a record");

template <typename T, int N>
struct alignas(sizeof(T) * N) NVec {
    T v[N];
};

// a stored value as float32: the 16 bits read as uint16 or int16 (numpy astype(float32), exact)
__device__ __forceinline__ float stored_f32(uint16_t bits, int is_unsigned) {
    return is_unsigned ? (float)bits : (float)(int16_t)bits;  // kernel argument: wave-uniform
}

// the N sums of a block in a fixed order: lanes by shuffles, then the four waves through LDS;
// thread k < N writes out[k]
template <int N>
__device__ __forceinline__ void nmodel_block_sums(double (&v)[N], double (*red)[NT / WAVE], double* __restrict__ out) {
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

// Chunk p of slice z.  x = f32(ncct) sn + in (vue); y = f32(cect) sc + ic; g = merged sn + in, or x
// without merged; diff = (y - g) / sn.  The block's record: n, n(diff >= thr), n(diff < 0),
// n(diff > 4000), sum clip(diff, 0, 4000), sum |diff|, sum x, sum y, sum x^2, sum y^2, sum xy.
template <int VEC, bool HAS_M>
__global__ void __launch_bounds__(NT) nmodel_targets_kernel(const uint16_t* __restrict__ ncct, int n_unsigned,
                                                     const float* __restrict__ sn, const float* __restrict__ in_,
                                                     const uint16_t* __restrict__ cect, int c_unsigned,
                                                     const float* __restrict__ sc, const float* __restrict__ ic,
                                                     const float* __restrict__ merged, int64_t S, int P, float thr,
                                                     float* __restrict__ vue, float* __restrict__ diff,
                                                     double* __restrict__ ws) {
    __shared__ double red[NS][NT / WAVE];
    const int64_t z = blockIdx.x / (unsigned)P;
    const int p = (int)(blockIdx.x % (unsigned)P);
    const float an = sn[z], bn = in_[z], ac = sc[z], bc = ic[z];
    const uint16_t* __restrict__ pn = ncct + z * S;
    const uint16_t* __restrict__ pc = cect + z * S;
    const float* __restrict__ pm = HAS_M ? merged + z * S : nullptr;
    float* __restrict__ pv = vue + z * S;
    float* __restrict__ pd = diff + z * S;
    const int64_t start = (int64_t)p * NCH;
    const int64_t end = start + NCH < S ? start + NCH : S;
    int cnt = 0, n_apply = 0, n_neg = 0, n_over = 0;
    double s_clip = 0.0, s_abs = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    using VP = NVec<uint16_t, VEC>;
    using VF = NVec<float, VEC>;
#pragma unroll 2
    for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += NT * VEC) {  // S % VEC == 0
        const VP qn = *reinterpret_cast<const VP*>(pn + i);
        const VP qc = *reinterpret_cast<const VP*>(pc + i);
        VF qm, ov, od;
        if (HAS_M) qm = *reinterpret_cast<const VF*>(pm + i);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float x = stored_f32(qn.v[v], n_unsigned) * an + bn;
            const float y = stored_f32(qc.v[v], c_unsigned) * ac + bc;
            const float g = HAS_M ? qm.v[v] * an + bn : x;
            const float d = __fdiv_rn(y - g, an);
            ov.v[v] = x;
            od.v[v] = d;
            cnt += 1;
            n_apply += d >= thr ? 1 : 0;
            n_neg += d < 0.0f ? 1 : 0;
            n_over += d > DIFF_MAX ? 1 : 0;
            s_clip += (double)fminf(fmaxf(d, 0.0f), DIFF_MAX);
            s_abs += (double)fabsf(d);
            const double dx = (double)x, dy = (double)y;
            sx += dx;
            sy += dy;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
        }
        *reinterpret_cast<VF*>(pv + i) = ov;
        *reinterpret_cast<VF*>(pd + i) = od;
    }
    // a thread counts at most NCH / NT voxels: exact in int and in double
    double rec[NS] = {(double)cnt, (double)n_apply, (double)n_neg, (double)n_over, s_clip, s_abs, sx, sy, sxx, syy, sxy};
    nmodel_block_sums<NS>(rec, red, ws + (int64_t)blockIdx.x * NS);
}

// out[z][k] = the sum of the partials ws[z][0..P)[k] in index order
__global__ void __launch_bounds__(NT) nmodel_targets_fold_kernel(const double* __restrict__ ws, int D, int P,
                                                          double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)D * NS) return;
    const int64_t z = i / NS;
    const int k = (int)(i % NS);
    const double* w = ws + z * P * NS + k;
    double v = w[0];
    for (int p = 1; p < P; ++p) v += w[(int64_t)p * NS];
    out[i] = v;
}

static bool al(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

static int parts(int H, int W) { return (int)cdiv((int64_t)H * W, NCH); }

// positive, one slice indexable by int, at most 2^38 voxels, the grid below 2^31 blocks
static bool dims_ok(int D, int H, int W) {
    if (D <= 0 || H <= 0 || W <= 0) return false;
    if ((int64_t)H * W >= (1ll << 30)) return false;
    if ((long double)D * H * W >= (long double)(1ll << 38)) return false;
    return (int64_t)D * parts(H, W) < (1ll << 31);
}

}  // namespace dcs

using namespace dcs;

extern "C" size_t dcs_nmodel_targets_workspace_size(int D, int H, int W) {
    if (!dims_ok(D, H, W)) return 0;
    return sizeof(double) * (size_t)NS * (size_t)D * (size_t)parts(H, W);
}

extern "C" int dcs_nmodel_targets(const void* ncct, int ncct_unsigned, const float* ncct_slope,
                                  const float* ncct_intercept, const void* cect, int cect_unsigned,
                                  const float* cect_slope, const float* cect_intercept, const float* merged, int D,
                                  int H, int W, float threshold, float* vue_out, float* diff_out, double* stats_out,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (!ncct || !ncct_slope || !ncct_intercept || !cect || !cect_slope || !cect_intercept || !vue_out || !diff_out ||
        !stats_out || !ws)
        return fail(DCS_E_INVALID, "nmodel_targets: null pointer");
    if (!dims_ok(D, H, W)) return fail(DCS_E_INVALID, "nmodel_targets: bad dimensions");
    if (!(threshold - threshold == 0.f)) return fail(DCS_E_INVALID, "nmodel_targets: the threshold must be finite");
    if (!al(ncct, 2) || !al(cect, 2) || !al(merged, 4) || !al(vue_out, 4) || !al(diff_out, 4) || !al(ncct_slope, 4) ||
        !al(ncct_intercept, 4) || !al(cect_slope, 4) || !al(cect_intercept, 4) || !al(stats_out, 8) || !al(ws, 8))
        return fail(DCS_E_INVALID, "nmodel_targets: misaligned pointer");
    const void* ins[3] = {ncct, cect, merged};
    for (const void* i : ins)
        if (i && (i == (const void*)vue_out || i == (const void*)diff_out))
            return fail(DCS_E_INVALID, "nmodel_targets: an output aliases an input");
    if (vue_out == diff_out) return fail(DCS_E_INVALID, "nmodel_targets: the two outputs alias each other");
    const int P = parts(H, W);
    if (ws_bytes < sizeof(double) * (size_t)NS * (size_t)D * (size_t)P)
        return fail(DCS_E_WORKSPACE, "nmodel_targets: workspace too small");
    const int64_t S = (int64_t)H * W;
    const dim3 grid((unsigned)((int64_t)D * P));
    hipStream_t s = as_stream(stream);
    const uint16_t* pn = static_cast<const uint16_t*>(ncct);
    const uint16_t* pc = static_cast<const uint16_t*>(cect);
    double* w = static_cast<double*>(ws);
    const bool vec = S % 4 == 0 && al(ncct, 8) && al(cect, 8) && al(merged, 16) && al(vue_out, 16) && al(diff_out, 16);
#define DCS_ND_LAUNCH(VEC, HAS_M)                                                                                  \
    hipLaunchKernelGGL((nmodel_targets_kernel<VEC, HAS_M>), grid, dim3(NT), 0, s, pn, ncct_unsigned ? 1 : 0, ncct_slope, \
                       ncct_intercept, pc, cect_unsigned ? 1 : 0, cect_slope, cect_intercept, merged, S, P,       \
                       threshold, vue_out, diff_out, w)
    if (vec && merged)
        DCS_ND_LAUNCH(4, true);
    else if (vec)
        DCS_ND_LAUNCH(4, false);
    else if (merged)
        DCS_ND_LAUNCH(1, true);
    else
        DCS_ND_LAUNCH(1, false);
#undef DCS_ND_LAUNCH
    if (int rc = check_launch("nmodel_targets")) return rc;
    hipLaunchKernelGGL(nmodel_targets_fold_kernel, dim3((unsigned)cdiv((int64_t)D * NS, NT)), dim3(NT), 0, s, w, D, P,
                       stats_out);
    return check_launch("nmodel_targets");
}
