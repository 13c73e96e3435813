// Heart-mask clean-up and organ masking of the masked evaluation on gfx950
// (modules/organ_masks.py is the definition; reference modify_heart_mask.py:87-198 and
// masking.py:455-541).  Volumes are dense [D][H][W] bytes, x fastest: a NIfTI file's own order,
// so nibabel's [x, y, z] is (x = W index, y = H index, z = D index).
//
// All of it is integer / byte work bounded by HBM and atomics:
//   * 3-D connected components (scipy.ndimage.label, 6-connectivity) are the lock-free union-find
//     of masks.hip in three dimensions: a 16x16x16 brick in LDS (one x-row of 16 voxels per thread,
//     the row's occupancy as one 16-bit word), then only the faces that cross into an earlier brick
//     in global memory, then path compression and per-component statistics aggregated over runs
//     of equal roots within the wave (voxel count, int64 coordinate sums, minimum [x,y,z] key);
//   * the heart clean-up keeps everything between the upload of the label volume and the download
//     of the modified one on the device: the lowest component (stable sort by the centre's z,
//     ties by ndimage.label's numbering) is selected by three small passes over the roots;
//   * the distance test is float64, one rounding per numpy operation (contraction is off for this
//     file; sqrt and division are correctly rounded), so `>= max_distance` decides like numpy;
//   * the organ mask runs the 2-D union-find on the complement of a batch of binary
//     (slice, label) images; a pair that the presence table does not hold exits before any pixel
//     pass.  The filled set, its outer boundary and the brush stamps are one tiled LDS pass.
// Every atomic is an integer min / max / add, so results are order-independent and bit-identical
// from run to run.  This file is self-contained (it shares no kernel with masks.hip).
#include "common.hpp"

#pragma clang fp contract(off)

namespace dcs {
namespace {

constexpr int OT = 256;

__device__ __forceinline__ int om_ld(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int om_find(const int* L, int x) {
    int p = om_ld(L + x);
    while (p != x) {
        x = p;
        p = om_ld(L + x);
    }
    return x;
}

// parents only ever decrease (atomicMin): a stale read is safe, the loop retries from what the
// atomic returned
__device__ __forceinline__ void om_union(int* L, int a, int b) {
    bool done;
    do {
        a = om_find(L, a);
        b = om_find(L, b);
        if (a < b) {
            const int old = atomicMin(L + b, a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(L + a, b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

__device__ __forceinline__ int om_lds_find(int* lab, int x) {
    int p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != x) {
        x = p;
        p = __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    return x;
}

__device__ __forceinline__ void om_lds_union(int* lab, int a, int b) {
    bool done;
    do {
        a = om_lds_find(lab, a);
        b = om_lds_find(lab, b);
        if (a < b) {
            const int old = atomicMin(lab + b, a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(lab + a, b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

// The edge from j to its neighbour in the previous row (or slice) is implied when j's left
// neighbour and that neighbour's counterpart are both set: the two x-runs and the left pair's own
// edge already connect them.
__device__ __forceinline__ bool om_need(bool left, bool diag) { return !(left && diag); }

// ---------------------------------------------------------------------------------------
// 3-D connected components, 6-connectivity
// ---------------------------------------------------------------------------------------
constexpr int BR = 16;                 // brick edge
constexpr int BRV = BR * BR * BR;      // voxels of a brick (one workgroup, 16 per thread)

struct Vol3 {
    int D, H, W, HW, np;
    int bx, by, bz;  // bricks per axis
};

// A workgroup labels one brick in LDS and writes, per voxel, the global index of its brick-local
// root (-1 for background).  Thread t owns the x-row (ly = t & 15, lz = t >> 4) of the brick.
// The brick-local order (lz, ly, lx) is the global order restricted to the brick, so a local root
// is also the smallest global index of its part: parents never exceed children.
__global__ __launch_bounds__(OT) void cc3_local_kernel(const uint8_t* __restrict__ V, int match, int* __restrict__ L,
                                                       Vol3 v) {
    __shared__ int lab[BRV];
    __shared__ unsigned short rows[OT];
    const int b = blockIdx.x;
    const int bxi = b % v.bx, byi = (b / v.bx) % v.by, bzi = b / (v.bx * v.by);
    const int t = threadIdx.x, ly = t & 15, lz = t >> 4;
    const int x0 = bxi * BR, y = byi * BR + ly, z = bzi * BR + lz;
    const bool inrow = y < v.H && z < v.D;
    const int base = inrow ? (z * v.H + y) * v.W + x0 : 0;
    unsigned bits = 0;
    if (inrow) {
#pragma unroll
        for (int e = 0; e < BR; ++e)
            if (x0 + e < v.W && V[base + e] == match) bits |= 1u << e;
    }
    rows[t] = (unsigned short)bits;
    int run = -1;
#pragma unroll
    for (int e = 0; e < BR; ++e) {
        const int j = t * BR + e;
        if (!((bits >> e) & 1u)) { lab[j] = -1; run = -1; continue; }
        if (run < 0) run = j;
        lab[j] = run;
    }
    __syncthreads();
    const unsigned up = ly > 0 ? rows[t - 1] : 0u, dn = lz > 0 ? rows[t - BR] : 0u;
#pragma unroll
    for (int e = 0; e < BR; ++e) {
        if (!((bits >> e) & 1u)) continue;
        const int j = t * BR + e;
        const bool left = e > 0 && ((bits >> (e - 1)) & 1u);
        if (((up >> e) & 1u) && om_need(left, e > 0 && ((up >> (e - 1)) & 1u))) om_lds_union(lab, j, j - BR);
        if (((dn >> e) & 1u) && om_need(left, e > 0 && ((dn >> (e - 1)) & 1u))) om_lds_union(lab, j, j - BR * BR);
    }
    __syncthreads();
    if (!inrow) return;
#pragma unroll
    for (int e = 0; e < BR; ++e) {
        if (x0 + e >= v.W) continue;
        int out = -1;
        if ((bits >> e) & 1u) {
            const int r = om_lds_find(lab, t * BR + e);
            out = ((bzi * BR + (r >> 8)) * v.H + byi * BR + ((r >> 4) & 15)) * v.W + x0 + (r & 15);
        }
        L[base + e] = out;
    }
}

// the edges that cross a brick face into an earlier brick
__global__ __launch_bounds__(OT) void cc3_border_kernel(const uint8_t* __restrict__ V, int match, int* L, Vol3 v) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= v.np) return;
    const int x = i % v.W, y = (i / v.W) % v.H, z = i / v.HW;
    const bool fx = x > 0 && (x & (BR - 1)) == 0, fy = y > 0 && (y & (BR - 1)) == 0, fz = z > 0 && (z & (BR - 1)) == 0;
    if (!(fx || fy || fz) || V[i] != match) return;
    const bool left = x > 0 && V[i - 1] == match;
    if (fx && left) om_union(L, i, i - 1);
    if (fy && V[i - v.W] == match && om_need(left, x > 0 && V[i - 1 - v.W] == match)) om_union(L, i, i - v.W);
    if (fz && V[i - v.HW] == match && om_need(left, x > 0 && V[i - 1 - v.HW] == match)) om_union(L, i, i - v.HW);
}

// L[i] = root; a root resets its own statistics (no memset of the per-root arrays)
__global__ __launch_bounds__(OT) void cc3_compress_kernel(int* L, int* __restrict__ C, long long* __restrict__ S,
                                                          unsigned* __restrict__ K, int np) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= np || om_ld(L + i) < 0) return;
    const int r = om_find(L, i);
    if (r != i) {
        L[i] = r;
        return;
    }
    C[i] = 0;
    if (S) {
        S[i] = 0;
        S[(size_t)np + i] = 0;
        S[2 * (size_t)np + i] = 0;
    }
    if (K) K[i] = 0xffffffffu;
}

// Per component: voxel count, coordinate sums (S[0] = x, S[1] = y, S[2] = z planes of np int64)
// and the minimum of the [x, y, z]-lexicographic key (x * H + y) * D + z, reduced over runs of
// equal roots within the wave before one atomic per run (a 100k-voxel component would otherwise
// serialise 100k atomics on one address).
__global__ __launch_bounds__(OT) void cc3_stats_kernel(const int* __restrict__ L, int* __restrict__ C,
                                                       long long* __restrict__ S, unsigned* __restrict__ K, Vol3 v) {
    const int i = blockIdx.x * OT + threadIdx.x;
    const int r = i < v.np ? L[i] : -1;
    const bool fg = r >= 0;
    if (!__ballot(fg)) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(r, 1, 64);
    const bool head = fg && (lane == 0 || prev != r);
    const unsigned long long heads = __ballot(head);
    const unsigned long long below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
    const int seg = fg && below ? 63 - __clzll((long long)below) : -1 - lane;
    int c = fg ? 1 : 0;
    if (!S) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int os = __shfl_down(seg, o, 64), oc = __shfl_down(c, o, 64);
            if (lane + o < 64 && os == seg) c += oc;
        }
        if (head) atomicAdd(C + r, c);
        return;
    }
    const int ii = fg ? i : 0;
    const int x = ii % v.W, y = (ii / v.W) % v.H, z = ii / v.HW;
    long long sx = x, sy = y, sz = z;
    unsigned key = ((unsigned)x * (unsigned)v.H + (unsigned)y) * (unsigned)v.D + (unsigned)z;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int os = __shfl_down(seg, o, 64), oc = __shfl_down(c, o, 64);
        const long long ox = __shfl_down(sx, o, 64), oy = __shfl_down(sy, o, 64), oz = __shfl_down(sz, o, 64);
        const unsigned ok = __shfl_down(key, o, 64);
        if (lane + o < 64 && os == seg) {
            c += oc;
            sx += ox;
            sy += oy;
            sz += oz;
            key = min(key, ok);
        }
    }
    if (head) {
        atomicAdd(C + r, c);
        atomicAdd(reinterpret_cast<unsigned long long*>(S) + r, (unsigned long long)sx);
        atomicAdd(reinterpret_cast<unsigned long long*>(S) + (size_t)v.np + r, (unsigned long long)sy);
        atomicAdd(reinterpret_cast<unsigned long long*>(S) + 2 * (size_t)v.np + r, (unsigned long long)sz);
        atomicMin(K + r, key);
    }
}

Vol3 make_vol(int D, int H, int W) {
    Vol3 v;
    v.D = D; v.H = H; v.W = W; v.HW = H * W; v.np = D * H * W;
    v.bx = (int)cdiv(W, BR); v.by = (int)cdiv(H, BR); v.bz = (int)cdiv(D, BR);
    return v;
}

int run_cc3(const uint8_t* V, int match, const Vol3& v, int* L, int* C, long long* S, unsigned* K, hipStream_t s) {
    const dim3 g((unsigned)cdiv(v.np, OT));
    hipLaunchKernelGGL(cc3_local_kernel, dim3((unsigned)(v.bx * v.by * v.bz)), dim3(OT), 0, s, V, match, L, v);
    if (v.bx * v.by * v.bz > 1) hipLaunchKernelGGL(cc3_border_kernel, g, dim3(OT), 0, s, V, match, L, v);
    hipLaunchKernelGGL(cc3_compress_kernel, g, dim3(OT), 0, s, L, C, S, K, v.np);
    hipLaunchKernelGGL(cc3_stats_kernel, g, dim3(OT), 0, s, L, C, S, K, v);
    return check_launch("organ_masks: 3-D connected components");
}

// ---------------------------------------------------------------------------------------
// heart clean-up
// ---------------------------------------------------------------------------------------
struct HeartState {
    unsigned long long min_cz;  // bits of the smallest centre z (non-negative doubles order as integers)
    unsigned long long max_plane, max_adx;  // bits of max (dx^2 + dy^2) on the centre's slice, max |dx|
    double cx, cy, cz;
    unsigned min_key;
    int found, start_z, zc, plane_any, pad;
};

struct HeartArgs {
    int gap, min_region, label;
    double offset, oyb_m1, offset_z;
};

__global__ void heart_init_kernel(HeartState* st, int D) {
    st->min_cz = ~0ull;
    st->max_plane = 0;
    st->max_adx = 0;
    st->cx = st->cy = st->cz = 0.0;
    st->min_key = 0xffffffffu;
    st->found = 0;
    st->start_z = D;
    st->zc = 0;
    st->plane_any = 0;
    st->pad = 0;
}

__global__ __launch_bounds__(OT) void heart_extract_kernel(const uint8_t* __restrict__ V, int label,
                                                           uint8_t* __restrict__ HM, int np) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i < np) HM[i] = V[i] == label;
}

// centers.sort(key = z), stable: the smallest centre z, then the smallest first-voxel key
__global__ __launch_bounds__(OT) void heart_select_kernel(const int* __restrict__ L, const int* __restrict__ C,
                                                          const long long* __restrict__ S,
                                                          const unsigned* __restrict__ K, Vol3 v, int pass,
                                                          HeartState* st) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= v.np || L[i] != i) return;
    const double cnt = (double)C[i];
    const double cz = (double)S[2 * (size_t)v.np + i] / cnt;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(cz);
    if (pass == 0) {
        atomicMin(&st->min_cz, bits);
    } else if (pass == 1) {
        if (bits == st->min_cz) atomicMin(&st->min_key, K[i]);
    } else if (bits == st->min_cz && K[i] == st->min_key) {  // exactly one root
        st->cx = (double)S[i] / cnt;
        st->cy = (double)S[(size_t)v.np + i] / cnt;
        st->cz = cz;
        st->start_z = (int)cz;
        st->zc = (int)cz;
        st->found = 1;
    }
}

// One thread per (x, y) column, serial in z; consecutive threads take consecutive x.
__global__ __launch_bounds__(OT) void heart_gap_kernel(uint8_t* HM, Vol3 v, int gap, const HeartState* st) {
    const int c = blockIdx.x * OT + threadIdx.x;
    if (c >= v.HW || !st->found) return;
    int run = 0;
    for (int z = st->start_z; z < v.D; ++z) {
        run = HM[z * v.HW + c] ? 0 : run + 1;
        if (run >= gap) {
            for (int zz = z - run + 1; zz < v.D; ++zz) HM[zz * v.HW + c] = 0;
            return;
        }
    }
}

__device__ __forceinline__ double wave_max_d(double m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    return m;
}

// max |dx| over the cut mask and max (dx^2 + dy^2) over its slice int(cz); a maximum has no
// order dependence, and sqrt is monotone and correctly rounded, so sqrt(max) == max(sqrt)
__global__ __launch_bounds__(OT) void heart_extent_kernel(const uint8_t* __restrict__ HM, Vol3 v, HeartState* st) {
    if (!st->found) return;
    const double cx = st->cx, cy = st->cy;
    const int zc = st->zc;
    double adx = -1.0, pl = -1.0;
    for (int i = blockIdx.x * OT + threadIdx.x; i < v.np; i += gridDim.x * OT) {
        if (!HM[i]) continue;
        const int x = i % v.W, y = (i / v.W) % v.H, z = i / v.HW;
        const double dx = (double)x - cx;
        adx = fmax(adx, fabs(dx));
        if (z == zc) {
            const double dy = (double)y - cy;
            pl = fmax(pl, dx * dx + dy * dy);
        }
    }
    adx = wave_max_d(adx);
    pl = wave_max_d(pl);
    if ((threadIdx.x & 63) == 0) {
        if (adx >= 0.0) atomicMax(&st->max_adx, (unsigned long long)__double_as_longlong(adx));
        if (pl >= 0.0) {
            atomicMax(&st->max_plane, (unsigned long long)__double_as_longlong(pl));
            st->plane_any = 1;
        }
    }
}

// modify_heart_mask.py:149-156, one rounding per numpy operation, the sum left to right
__global__ __launch_bounds__(OT) void heart_distance_kernel(uint8_t* HM, Vol3 v, HeartArgs a, const HeartState* st) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= v.np || !st->found || !st->plane_any || !HM[i]) return;
    const double max_distance = __dsqrt_rn(__longlong_as_double((long long)st->max_plane)) * a.offset;
    const double den = __longlong_as_double((long long)st->max_adx) + 1e-5;
    const int x = i % v.W, y = (i / v.W) % v.H, z = i / v.HW;
    const double dx = (double)x - st->cx, dy = (double)y - st->cy, dz = (double)z - st->cz;
    const double oyv = 1.0 + (a.oyb_m1 * fabs(dx)) / den;
    const double sy = dy * oyv, sz = dz * a.offset_z;
    const double ty = (dy > 0.0 && dz > 0.0) ? sy * sy : dy * dy;
    const double tz = dz > 0.0 ? sz * sz : dz * dz;
    const double d = __dsqrt_rn((dx * dx + ty) + tz);
    if (d >= max_distance) HM[i] = 0;
}

// regions below min_region go; the surviving heart is written back into the other labels
__global__ __launch_bounds__(OT) void heart_finish_kernel(const uint8_t* __restrict__ V, const uint8_t* __restrict__ HM,
                                                          const int* __restrict__ L, const int* __restrict__ C,
                                                          HeartArgs a, uint8_t* __restrict__ out, int np) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= np) return;
    const uint8_t val = V[i];
    uint8_t o = val == a.label ? 0 : val;
    if (HM[i] && C[L[i]] >= a.min_region) o = (uint8_t)a.label;
    out[i] = o;
}

struct HeartWs {
    int* L;
    int* C;
    long long* S;
    unsigned* K;
    uint8_t* HM;
    HeartState* st;
    size_t bytes;
};

HeartWs heart_carve(void* base, int D, int H, int W) {
    HeartWs w;
    const size_t np = (size_t)D * H * W;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t b) {
        char* q = p ? p + off : nullptr;
        off = align_up(off + b, 256);
        return q;
    };
    w.S = reinterpret_cast<long long*>(take(np * 24));
    w.L = reinterpret_cast<int*>(take(np * 4));
    w.C = reinterpret_cast<int*>(take(np * 4));
    w.K = reinterpret_cast<unsigned*>(take(np * 4));
    w.HM = reinterpret_cast<uint8_t*>(take(np));
    w.st = reinterpret_cast<HeartState*>(take(sizeof(HeartState)));
    w.bytes = off;
    return w;
}

bool vol_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && (long long)D * H * W < (1ll << 31);
}

// ---------------------------------------------------------------------------------------
// organ mask: batch of binary (slice, label) images, 2-D union-find on the complement
// ---------------------------------------------------------------------------------------
constexpr int OM_TILE = 4096;            // consecutive pixels per workgroup of the local labelling
constexpr int OM_SEG = OM_TILE / OT;     // per thread
constexpr int ST = 32;                   // output tile edge of the stamp pass
constexpr int OM_MAX_R = 2;              // largest brush radius
constexpr int OM_MAX_BRUSH = 25;
constexpr int HALO = OM_MAX_R + 1;
constexpr int SA = ST + 2 * HALO;        // edge of the state region (tile + brush + one neighbour)
constexpr int SB = ST + 2 * OM_MAX_R;    // edge of the boundary region

struct OmArgs {
    int H, W, HW, tiles;
    int nl, S, z0, fill;  // labels, slices of this chunk, its first slice, stage-1 fill
    uint8_t lab[256];
};

struct Brush {
    int n;
    signed char dy[OM_MAX_BRUSH], dx[OM_MAX_BRUSH];
};

// pres[z][value] = 1 for the values slice z holds
__global__ __launch_bounds__(OT) void om_presence_kernel(const uint8_t* __restrict__ V, int HW, int per_slice,
                                                         uint8_t* __restrict__ pres) {
    __shared__ int seen[256];
    seen[threadIdx.x] = 0;
    __syncthreads();
    const int z = blockIdx.x / per_slice, b = blockIdx.x - z * per_slice;
    const uint8_t* src = V + (size_t)z * HW;
    for (int p = b * OT + threadIdx.x; p < HW; p += per_slice * OT) seen[src[p]] = 1;
    __syncthreads();
    if (seen[threadIdx.x]) pres[z * 256 + threadIdx.x] = 1;
}

// background (src != label) of image `slot` = (slice s, label li) of the chunk, tile-local
// (the tile also clears its outside flags E, so an absent pair costs not even a memset)
__global__ __launch_bounds__(OT) void om_local_kernel(const uint8_t* __restrict__ V, const uint8_t* __restrict__ pres,
                                                      OmArgs a, int* __restrict__ L, uint8_t* __restrict__ E) {
    __shared__ int lab[OM_TILE];
    __shared__ uint8_t fgm[OM_TILE];
    const int slot = blockIdx.x / a.tiles, t = blockIdx.x - slot * a.tiles;
    const int s = slot / a.nl, label = a.lab[slot - s * a.nl];
    if (!pres[(a.z0 + s) * 256 + label]) return;  // absent pair: no pixel pass
    const uint8_t* src = V + (size_t)(a.z0 + s) * a.HW;
    const int W = a.W, p0 = t * OM_TILE, cnt = min(OM_TILE, a.HW - p0);
    const int g0 = slot * a.HW + p0;
    for (int j = threadIdx.x; j < OM_TILE; j += OT) fgm[j] = j < cnt ? src[p0 + j] != label : 0;
    __syncthreads();
    const int j0 = threadIdx.x * OM_SEG;
    int x = (p0 + j0) % W;
    int run = -1;
#pragma unroll
    for (int e = 0; e < OM_SEG; ++e) {
        const int j = j0 + e;
        if (e > 0 && ++x == W) x = 0;
        if (!fgm[j]) { lab[j] = -1; run = -1; continue; }
        if (run < 0 || x == 0) run = j;
        lab[j] = run;
    }
    __syncthreads();
    x = (p0 + j0) % W;
#pragma unroll
    for (int e = 0; e < OM_SEG; ++e) {
        const int j = j0 + e;
        if (e > 0 && ++x == W) x = 0;
        if (j >= cnt || !fgm[j]) continue;
        const bool left = x > 0 && j > 0 && fgm[j - 1];
        if (e == 0 && left) om_lds_union(lab, j, j - 1);
        // (a diagonal neighbour in the previous tile is not in fgm: the edge is then kept)
        if (j >= W && fgm[j - W] && om_need(left, x > 0 && j > W && fgm[j - 1 - W])) om_lds_union(lab, j, j - W);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += OT) {
        L[g0 + j] = fgm[j] ? g0 + om_lds_find(lab, j) : -1;
        E[g0 + j] = 0;
    }
}

// edges from tile t >= 1 into earlier tiles: its first min(W, OM_TILE) pixels (upper neighbour)
// and its first pixel (left neighbour, when the tile starts mid-row)
__global__ __launch_bounds__(OT) void om_border_kernel(const uint8_t* __restrict__ V, const uint8_t* __restrict__ pres,
                                                       OmArgs a, int* L, int span, int total) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= total) return;
    const int per = (a.tiles - 1) * span;
    const int slot = i / per, r = i - slot * per;
    const int t = 1 + r / span, k = r - (t - 1) * span;
    const int p = t * OM_TILE + k;
    if (p >= a.HW) return;
    const int s = slot / a.nl, label = a.lab[slot - s * a.nl];
    if (!pres[(a.z0 + s) * 256 + label]) return;
    const uint8_t* src = V + (size_t)(a.z0 + s) * a.HW;
    if (src[p] == label) return;
    const int W = a.W, g = slot * a.HW + p, x = p % W;
    const bool left = x > 0 && src[p - 1] != label;
    if (p >= W && src[p - W] != label && om_need(left, x > 0 && src[p - 1 - W] != label)) om_union(L, g, g - W);
    if (k == 0 && left) om_union(L, g, g - 1);
}

// L[i] = root; E[root] = 1 for the background components that touch an image edge (the outside:
// the part of the background a 4-connected path joins to the padded border)
__global__ __launch_bounds__(OT) void om_compress_kernel(const uint8_t* __restrict__ pres, OmArgs a, int* L,
                                                         uint8_t* __restrict__ E, int total) {
    const int i = blockIdx.x * OT + threadIdx.x;
    if (i >= total) return;
    const int slot = i / a.HW, p = i - slot * a.HW;
    const int s = slot / a.nl, label = a.lab[slot - s * a.nl];
    if (!pres[(a.z0 + s) * 256 + label] || om_ld(L + i) < 0) return;
    const int r = om_find(L, i);
    L[i] = r;
    const int y = p / a.W, x = p - y * a.W;
    if (x == 0 || y == 0 || x == a.W - 1 || y == a.H - 1) E[r] = 1;
}

// One 32x32 tile of one (slice, label) image: state (in the set / outside) over the tile and a
// halo of brush radius + 1, the outer boundary over tile + brush radius, then
// out = in-set | brush stamped at the boundary pixels.  fill: the holes (background that is not
// outside) belong to the set (stage 1); otherwise they are left alone (stage 2 draws a line only).
__global__ __launch_bounds__(OT) void om_stamp_kernel(const uint8_t* __restrict__ V, const uint8_t* __restrict__ pres,
                                                      OmArgs a, Brush br, const int* __restrict__ L,
                                                      const uint8_t* __restrict__ E, uint8_t* __restrict__ out) {
    __shared__ uint8_t st[SA * SA];
    __shared__ uint8_t bnd[SB * SB];
    const int slot = blockIdx.y, s = slot / a.nl, label = a.lab[slot - s * a.nl];
    if (!pres[(a.z0 + s) * 256 + label]) return;
    const uint8_t* src = V + (size_t)(a.z0 + s) * a.HW;
    const int tx_n = (a.W + ST - 1) / ST;
    const int ty0 = (blockIdx.x / tx_n) * ST, tx0 = (blockIdx.x % tx_n) * ST;
    const int base = slot * a.HW;
    for (int k = threadIdx.x; k < SA * SA; k += OT) {
        const int yy = ty0 - HALO + k / SA, xx = tx0 - HALO + k % SA;
        uint8_t code = 2;  // beyond the image: outside
        if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
            const int p = yy * a.W + xx;
            if (src[p] == label) code = 1;
            else code = E[L[base + p]] ? 2 : (a.fill ? 1 : 0);
        }
        st[k] = code;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SB * SB; k += OT) {
        const int c = (k / SB + 1) * SA + k % SB + 1;
        bnd[k] = (st[c] & 1) && ((st[c - SA] | st[c + SA] | st[c - 1] | st[c + 1]) & 2);
    }
    __syncthreads();
    uint8_t* dst = out + (size_t)(a.z0 + s) * a.HW;
    for (int k = threadIdx.x; k < ST * ST; k += OT) {
        const int ly = k / ST, lx = k % ST;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= a.H || x >= a.W) continue;
        int on = st[(ly + HALO) * SA + lx + HALO] & 1;
        for (int q = 0; q < br.n && !on; ++q) on = bnd[(ly + OM_MAX_R - br.dy[q]) * SB + lx + OM_MAX_R - br.dx[q]];
        if (on) dst[y * a.W + x] = 1;  // every label's writer stores the same value
    }
}

struct OmWs {
    int* L;
    uint8_t* E;
    uint8_t* U;
    uint8_t* pres;
    size_t bytes;
};

OmWs om_carve(void* base, int N, int H, int W, int nl, int chunk) {
    OmWs w;
    const size_t img = (size_t)chunk * nl * H * W;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t b) {
        char* q = p ? p + off : nullptr;
        off = align_up(off + b, 256);
        return q;
    };
    w.L = reinterpret_cast<int*>(take(img * 4));
    w.E = reinterpret_cast<uint8_t*>(take(img));
    w.U = reinterpret_cast<uint8_t*>(take((size_t)N * H * W));
    w.pres = reinterpret_cast<uint8_t*>(take((size_t)N * 256));
    w.bytes = off;
    return w;
}

bool om_dims_ok(int N, int H, int W, int nl, int chunk) {
    // chunk * nl images: their pixels (plus one tile of slack for the border pass's thread count)
    // index in 31 bits, and they are the y extent of the stamp pass's grid
    return vol_ok(N, H, W) && nl >= 1 && nl <= 255 && chunk >= 1 && (long long)chunk * nl <= 65535 &&
           (long long)chunk * nl * ((long long)H * W + OM_TILE) < (1ll << 31);
}

// one stage over N slices of V, `per` slices at a time: out[z][p] = 1 where the stage sets it
int om_stage(const uint8_t* V, int N, OmArgs a, const Brush& br, int per, const OmWs& w, uint8_t* out, hipStream_t s) {
    const int HW = a.HW;
    if (hipMemsetAsync(w.pres, 0, (size_t)N * 256, s) != hipSuccess) return fail(DCS_E_INVALID, "organ_mask: memset failed");
    const int pb = (int)(cdiv(HW, OT) < 32 ? cdiv(HW, OT) : 32);
    hipLaunchKernelGGL(om_presence_kernel, dim3((unsigned)((int64_t)N * pb)), dim3(OT), 0, s, V, HW, pb, w.pres);
    const int st_tiles = (int)(cdiv(a.H, ST) * cdiv(a.W, ST));
    for (int z0 = 0; z0 < N; z0 += per) {
        a.z0 = z0;
        a.S = N - z0 < per ? N - z0 : per;
        const int slots = a.S * a.nl, total = slots * HW;
        hipLaunchKernelGGL(om_local_kernel, dim3((unsigned)(slots * a.tiles)), dim3(OT), 0, s, V, w.pres, a, w.L, w.E);
        if (a.tiles > 1) {
            const int span = a.W < OM_TILE ? a.W : OM_TILE;
            const int tot = slots * (a.tiles - 1) * span;
            hipLaunchKernelGGL(om_border_kernel, dim3((unsigned)cdiv(tot, OT)), dim3(OT), 0, s, V, w.pres, a, w.L, span, tot);
        }
        hipLaunchKernelGGL(om_compress_kernel, dim3((unsigned)cdiv(total, OT)), dim3(OT), 0, s, w.pres, a, w.L, w.E, total);
        hipLaunchKernelGGL(om_stamp_kernel, dim3((unsigned)st_tiles, (unsigned)slots), dim3(OT), 0, s, V, w.pres, a, br, w.L,
                           w.E, out);
        const int e = check_launch("organ_mask: stage");
        if (e) return e;
    }
    return DCS_OK;
}

int make_brush(const int8_t* pairs, int n, Brush* br) {
    if (!pairs || n < 1 || n > OM_MAX_BRUSH) return 1;
    br->n = n;
    for (int q = 0; q < n; ++q) {
        const int dy = pairs[2 * q], dx = pairs[2 * q + 1];
        if (dy < -OM_MAX_R || dy > OM_MAX_R || dx < -OM_MAX_R || dx > OM_MAX_R) return 1;
        br->dy[q] = (signed char)dy;
        br->dx[q] = (signed char)dx;
    }
    return 0;
}

__global__ __launch_bounds__(OT) void om_apply_kernel(const int16_t* __restrict__ a, const int16_t* __restrict__ b,
                                                      const int16_t* __restrict__ c, const uint8_t* __restrict__ m,
                                                      long long n, int16_t fill, int16_t* __restrict__ oa,
                                                      int16_t* __restrict__ ob, int16_t* __restrict__ oc) {
    for (long long i = (long long)blockIdx.x * OT + threadIdx.x; i < n; i += (long long)gridDim.x * OT) {
        const bool on = m[i] != 0;
        oa[i] = on ? fill : a[i];
        ob[i] = on ? fill : b[i];
        oc[i] = on ? fill : c[i];
    }
}

}  // namespace
}  // namespace dcs

using namespace dcs;

extern "C" int dcs_cc3_label(const uint8_t* vol, int match, int D, int H, int W, int32_t* labels, int32_t* count,
                             int64_t* sums, uint32_t* keys, void* stream) {
    if (!vol || !labels || !count || (sums == nullptr) != (keys == nullptr) || match < 0 || match > 255)
        return fail(DCS_E_INVALID, "cc3_label: bad arguments");
    if (!vol_ok(D, H, W)) return fail(DCS_E_INVALID, "cc3_label: volume too large or empty (0 < D*H*W < 2^31)");
    return run_cc3(vol, match, make_vol(D, H, W), labels, count, reinterpret_cast<long long*>(sums), keys,
                   as_stream(stream));
}

extern "C" size_t dcs_heart_workspace_size(int D, int H, int W) {
    if (!vol_ok(D, H, W)) return 0;
    return heart_carve(nullptr, D, H, W).bytes;
}

extern "C" int dcs_heart_modify(const uint8_t* vol, int D, int H, int W, int heart_label, int gap_threshold,
                                double offset, double offset_y_base_m1, double offset_z, int min_region, uint8_t* out,
                                void* ws, size_t ws_bytes, void* stream) {
    if (!vol || !out || !ws || vol == out || gap_threshold < 1)
        return fail(DCS_E_INVALID, "heart_modify: bad arguments");
    if (heart_label < 0 || heart_label > 255) return fail(DCS_E_INVALID, "heart_modify: labels must be < 256");
    if (!vol_ok(D, H, W)) return fail(DCS_E_INVALID, "heart_modify: volume too large or empty (0 < D*H*W < 2^31)");
    if (ws_bytes < dcs_heart_workspace_size(D, H, W)) return fail(DCS_E_WORKSPACE, "heart_modify: workspace too small");
    const HeartWs w = heart_carve(ws, D, H, W);
    const Vol3 v = make_vol(D, H, W);
    HeartArgs a;
    a.gap = gap_threshold; a.min_region = min_region; a.label = heart_label;
    a.offset = offset; a.oyb_m1 = offset_y_base_m1; a.offset_z = offset_z;
    hipStream_t s = as_stream(stream);
    const dim3 g((unsigned)cdiv(v.np, OT));
    int e;
    hipLaunchKernelGGL(heart_init_kernel, dim3(1), dim3(1), 0, s, w.st, D);
    hipLaunchKernelGGL(heart_extract_kernel, g, dim3(OT), 0, s, vol, heart_label, w.HM, v.np);
    if ((e = run_cc3(w.HM, 1, v, w.L, w.C, w.S, w.K, s))) return e;
    for (int pass = 0; pass < 3; ++pass)
        hipLaunchKernelGGL(heart_select_kernel, g, dim3(OT), 0, s, w.L, w.C, w.S, w.K, v, pass, w.st);
    hipLaunchKernelGGL(heart_gap_kernel, dim3((unsigned)cdiv(v.HW, OT)), dim3(OT), 0, s, w.HM, v, a.gap, w.st);
    const unsigned eb = (unsigned)(cdiv(v.np, OT) < 2048 ? cdiv(v.np, OT) : 2048);
    hipLaunchKernelGGL(heart_extent_kernel, dim3(eb), dim3(OT), 0, s, w.HM, v, w.st);
    hipLaunchKernelGGL(heart_distance_kernel, g, dim3(OT), 0, s, w.HM, v, a, w.st);
    if ((e = check_launch("heart_modify: cut"))) return e;
    if ((e = run_cc3(w.HM, 1, v, w.L, w.C, nullptr, nullptr, s))) return e;
    hipLaunchKernelGGL(heart_finish_kernel, g, dim3(OT), 0, s, vol, w.HM, w.L, w.C, a, out, v.np);
    return check_launch("heart_modify: finish");
}

extern "C" size_t dcs_organ_mask_workspace_size(int N, int H, int W, int nlabels, int chunk) {
    if (!om_dims_ok(N, H, W, nlabels, chunk)) return 0;
    return om_carve(nullptr, N, H, W, nlabels, chunk).bytes;
}

extern "C" int dcs_organ_mask(const uint8_t* labels, int N, int H, int W, const int32_t* target, int nlabels,
                              const int8_t* brush1, int nbrush1, const int8_t* brush2, int nbrush2, int chunk,
                              uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !target || !out || !ws || labels == out) return fail(DCS_E_INVALID, "organ_mask: bad arguments");
    if (!om_dims_ok(N, H, W, nlabels, chunk))
        return fail(DCS_E_INVALID, "organ_mask: bad dimensions (0 < N*H*W < 2^31, chunk*nlabels*H*W < 2^31, 1..255 labels)");
    Brush b1, b2;
    if (make_brush(brush1, nbrush1, &b1) || make_brush(brush2, nbrush2, &b2))
        return fail(DCS_E_INVALID, "organ_mask: brush (1..25 offsets within radius 2)");
    OmArgs a;
    a.H = H; a.W = W; a.HW = H * W; a.tiles = (int)cdiv(a.HW, OM_TILE);
    a.nl = nlabels; a.S = 0; a.z0 = 0; a.fill = 1;
    for (int q = 0; q < 256; ++q) a.lab[q] = 0;
    for (int q = 0; q < nlabels; ++q) {
        if (target[q] < 0 || target[q] > 255) return fail(DCS_E_INVALID, "organ_mask: labels must be < 256");
        a.lab[q] = (uint8_t)target[q];
    }
    if (ws_bytes < dcs_organ_mask_workspace_size(N, H, W, nlabels, chunk))
        return fail(DCS_E_WORKSPACE, "organ_mask: workspace too small");
    const OmWs w = om_carve(ws, N, H, W, nlabels, chunk);
    hipStream_t s = as_stream(stream);
    const size_t np = (size_t)N * H * W;
    if (hipMemsetAsync(w.U, 0, np, s) != hipSuccess || hipMemsetAsync(out, 0, np, s) != hipSuccess)
        return fail(DCS_E_INVALID, "organ_mask: memset failed");
    int e;
    // stage 1: per label, external contours filled and drawn with the first brush, united in U
    if ((e = om_stage(labels, N, a, b1, chunk, w, w.U, s))) return e;
    // stage 2: the external contours of U drawn with the second brush: U is a one-label volume
    a.nl = 1; a.fill = 0; a.lab[0] = 1;
    if ((e = om_stage(w.U, N, a, b2, chunk * nlabels, w, out, s))) return e;
    return DCS_OK;
}

extern "C" int dcs_organ_apply(const int16_t* a, const int16_t* b, const int16_t* c, const uint8_t* mask, int64_t n,
                               int fill, int16_t* out_a, int16_t* out_b, int16_t* out_c, void* stream) {
    if (!a || !b || !c || !mask || !out_a || !out_b || !out_c || n <= 0 || fill < -32768 || fill > 32767)
        return fail(DCS_E_INVALID, "organ_apply: bad arguments");
    const int64_t blocks = cdiv(n, OT) < 8192 ? cdiv(n, OT) : 8192;
    hipLaunchKernelGGL(om_apply_kernel, dim3((unsigned)blocks), dim3(OT), 0, as_stream(stream), a, b, c, mask,
                       (long long)n, (int16_t)fill, out_a, out_b, out_c);
    return check_launch("organ_apply");
}
