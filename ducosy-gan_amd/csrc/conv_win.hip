// 3x3 stride-1 'same' convolution over whole image rows on f16x3 operands, the source window of a
// tile staged once per 16-channel slice (the residual-block convolutions of modules/model.py:72-80:
// forward with reflection padding, and the interior of the data gradient with zero padding over
// flipped weights).
//
// conv.hip's rows pass gathers A[pixel][(tap, channel)] into LDS per k-tile: every source value is
// fetched, split into hi/lo fp16 and stored nine times (once per tap).  Here a workgroup owns 256
// consecutive pixels of one image (R = 256 / W whole rows) x 128 output channels, and per 16-channel
// slice stages the (R + 2) x (W + 2) source window once (520 pixels at W = 128: 2.0 values per output
// pixel instead of 9); the nine taps read their MFMA fragments from the window at a per-tap pixel
// offset.  The weights arrive pre-split (dcs_pack_weights_h3: hi / lo fp16 planes, slice-major K), so
// their k-steps are copied to LDS without arithmetic (LDS-DMA, win_glds).
// 8 waves = 4 (pixels) x 2 (channels) of 64 x 64; one workgroup per CU.
//
// The MFMA is v_mfma_f32_16x16x32_f16 (conv3_win16_kernel).  It does the same MACs per fragment byte
// as the 32x32x16 form, but under the package power limit sustains ~12 % more FLOP/s: 1758 against
// 1562 TFLOP/s of f16x3 products in a bare LDS-read + MFMA loop with every CU busy on random operands
// (scripts/probes/mfma_shape_power.hip, profiles/r06b/; MI355X_MICROARCH.md, DVFS item 7).
//
// K = 32 per MFMA = two (slice, tap) units of 16 channels: the fragments' k groups 0, 1 (lanes 0-31)
// take unit 2j, k groups 2, 3 (lanes 32-63) unit 2j + 1 -- the packed B's k = 16 unit + channel, so a
// k-step is 32 consecutive packed k.  A slice has nine taps: the k-steps walk the 18 units of a PAIR
// of slices, 9 k-steps, k-step 4 taking tap 8 of the even slice and tap 0 of the odd one.  The even
// slice of a pair sits in window buffer 0, the odd one in buffer 1; the next odd slice is staged
// during k-steps 0-3 (buffer 1 is free after the previous pair's k-step 8), the next even slice
// during k-steps 5-8 (buffer 0 is free after k-step 4), one staging unit in flight per thread: only
// one unit's eight floats are live at a time.  Only the window's interior columns are loaded (two
// units per thread); the halo columns are written by the units of source columns 1 and W - 2
// (reflection) or zeroed once (zero padding).  Waves 4-7 (the partners of waves 0-3 on their SIMDs)
// store their staging unit at the top of the next k-step instead of after their MFMAs, so the two
// waves of a SIMD are not in the same phase.
// One barrier per k-step: B (128 output-channel rows x 32 k x 2 planes, 16 KB) by LDS-DMA into the
// other of the B buffers.  Per k-step and wave: 4 x 4 blocks of 16 x 16 x 3 products = 48 MFMAs.
// Row block i of wave wm holds the 16 consecutive tile pixels wm * 64 + 16 i + (lane & 15) (W >= 16:
// a block never crosses an image row), so the window needs no swizzle: the 16 lanes of a
// ds_read_b128 lane group read 16 distinct 16-byte bank groups (pixel stride 32 B, the two channel
// halves on odd / even groups).  A B row (output channel co) holds its four 8-k groups rotated by
// 2 * ((co >> 2) & 3), which makes the B reads conflict-free too.  Two-level accumulation: chains of
// 5 and 4 k-steps (160 / 128 k), added to the running sum.
#include "common.hpp"
#include "conv_common.hpp"
#include <type_traits>


namespace dcs {
namespace {

constexpr int WIN_BN = 128, WIN_NT = 512;  // tiles: 256 pixels (whole rows) x WIN_BN channels
constexpr int WIN_PIX = 520;             // window pixels for W <= 128: (256 / W + 2) * (W + 2) <= 520
// window staging units (pixel, 8-channel half) per thread: the interior columns only, (256 / W + 2) x W
// pixels x 2 halves <= 1024 for W <= 128
constexpr int WIN_UNITS = 2;

struct WinArgs {
    int N, H, W, C, Co;  // source NHWC [N][H][W][C]; output NHWC [N][H][W][Co]
    int reflect;         // 1: reflection padding (forward), 0: zero padding (data gradient interior)
    int R, tiles;        // image rows per tile (256 / W), tiles per image (H / R)
    int gy;              // column tiles (Co / 128)
    int rng_n;           // partial maxima of the source range record
};

// one global_load_lds_dwordx4: lane L's 16 bytes land at LDS byte address lds + 16 L.  Inline asm: a
// compiler-emitted LDS-DMA makes hipcc wait for it before every later LDS read it cannot tell apart
// from the DMA's destination.  The kernel retires these itself (s_waitcnt vmcnt before the barrier
// that publishes the buffer); the compiler's own vmcnt waits only grow more conservative beside them.
__device__ __forceinline__ void win_glds(const void* base, unsigned voff, unsigned lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(base), "s"(lds)
                 : "memory");
}

// The InstanceNorm backward's partial sums over a data-gradient tile (IBW instances): the output is
// da of a layer a = act(IN(y)); per channel sum g and sum g * xhat with xhat = y * sc + sh and
// g = da * act'(xhat), over the tile's pixels except the ones the reflection ring fold still adds to
// (rows 1, H - 2 and columns 1, W - 2: the fold kernel sums those with their final values).
struct IbwArgs {
    const float* y;
    const float* sc;
    const float* sh;
    Sum2* parts;  // [N][nchunk][Co]
    int act, nchunk;
};

constexpr int W16_BSLOT = 128 * 32;  // halves per B plane and k-step

__device__ __forceinline__ int w16_off(int buf, int pl, int wpix, int h) {
    return ((buf * 2 + pl) * WIN_PIX + wpix) * 16 + 8 * h;
}

// IN statistics of the tile from the 16x16 accumulator layout (lane: column lane & 15 of each block,
// rows 4 (lane >> 4) + r): per column over the lane's 16 pixels, merged with lanes ^ 16 and ^ 32, then
// over the four pixel waves in a fixed order (the tile's count / mean / M2 / max / first argmax per
// column, as conv.hip rows_in_stats with BM 256 x BN 128)
__device__ __forceinline__ void win16_stats(const f32x4v (&acc)[4][4], int p0, int n0, int Co, int wm, int wn,
                                            int lane, int tid, float* lds, Part* __restrict__ parts, long long chunk) {
    Part* sp = reinterpret_cast<Part*>(lds);  // [4][128]
    const int g = lane >> 4, m16 = lane & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = 0.f, mx = -INFINITY;
        int am = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)  // increasing pixel order (first maximum)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[i][j][r];
                s += v;
                if (v > mx) { mx = v; am = p0 + wm * 64 + 16 * i + 4 * g + r; }
            }
        float mean = s * (1.f / 16.f), m2 = 0.f, cnt = 16.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dv = acc[i][j][r] - mean;
                m2 = fmaf(dv, dv, m2);
            }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {  // equal counts on both sides
            const float mb = __shfl_xor(mean, o, 64), m2b = __shfl_xor(m2, o, 64), mxb = __shfl_xor(mx, o, 64);
            const int amb = __shfl_xor(am, o, 64);
            const float dl = mb - mean;
            m2 = m2 + m2b + dl * dl * (0.5f * cnt);
            mean = mean + 0.5f * dl;
            cnt *= 2.f;
            if (mxb > mx || (mxb == mx && amb < am)) { mx = mxb; am = amb; }
        }
        if (g == 0) {
            Part p;
            p.cnt = cnt;
            p.mean = mean;
            p.m2 = m2;
            p.mx = mx;
            p.amax = am;
            p.pad[0] = p.pad[1] = p.pad[2] = 0;
            sp[wm * WIN_BN + wn * 64 + j * 16 + m16] = p;
        }
    }
    __syncthreads();
    if (tid < WIN_BN && n0 + tid < Co) {
        Part a = sp[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const Part b = sp[w * WIN_BN + tid];
            const float tot = a.cnt + b.cnt, dl = b.mean - a.mean;
            a.mean += dl * (b.cnt / tot);
            a.m2 += b.m2 + dl * dl * (a.cnt * b.cnt / tot);
            a.cnt = tot;
            if (b.mx > a.mx || (b.mx == a.mx && b.amax < a.amax)) { a.mx = b.mx; a.amax = b.amax; }
        }
        parts[chunk * Co + n0 + tid] = a;
    }
}

// the IbwArgs partial sums of the tile from the 16x16 accumulator layout (yv: y at the tile's outputs)
__device__ __forceinline__ void win16_ibw(const f32x4v (&acc)[4][4], const float (&yv)[4][4][4], const IbwArgs& ib,
                                          int n, int p0, int H, int W, int Co, int n0, int wm, int wn, int lane,
                                          int tid, int tile, float* lds) {
    const int g = lane >> 4, m16 = lane & 15;
    Sum2* sp = reinterpret_cast<Sum2*>(lds);  // [4][128]; the k-loop's last barrier freed the LDS
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + j * 16 + m16;
        const float s = ib.sc[(long long)n * Co + col], b = ib.sh[(long long)n * Co + col];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pix = p0 + wm * 64 + 16 * i + 4 * g + r;
                const int py = pix >> __builtin_ctz(W), px = pix & (W - 1);  // (W is a power of two)
                if (py == 1 || py == H - 2 || px == 1 || px == W - 2) continue;  // the ring fold's pixels
                const float xh = fmaf(yv[i][j][r], s, b);
                const float gg = acc[i][j][r] * act_grad(xh, ib.act);
                sa += gg;
                sb = fmaf(gg, xh, sb);
            }
        sa += __shfl_xor(sa, 16, 64);  // the same operand pair on both lanes: order-free
        sb += __shfl_xor(sb, 16, 64);
        sa += __shfl_xor(sa, 32, 64);
        sb += __shfl_xor(sb, 32, 64);
        if (g == 0) sp[wm * 128 + wn * 64 + j * 16 + m16] = Sum2{sa, sb};
    }
    __syncthreads();
    if (tid < 128 && n0 + tid < Co) {
        Sum2 t = sp[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            t.a += sp[w * 128 + tid].a;
            t.b += sp[w * 128 + tid].b;
        }
        ib.parts[((long long)n * ib.nchunk + tile) * Co + n0 + tid] = t;
    }
}

template <int NP, bool IBW, bool WIDE>  // NP: products (3: f16x3, 1: f16, hi planes only); WIDE: W >= 64
__global__ __launch_bounds__(WIN_NT, 1) void conv3_win16_kernel(WinArgs a, const float* __restrict__ src,
                                                                const _Float16* __restrict__ wh,
                                                                const _Float16* __restrict__ wl,
                                                                const float* __restrict__ rng,
                                                                const int* __restrict__ wexp,
                                                                const float* __restrict__ addend,
                                                                float* __restrict__ out, Part* __restrict__ parts,
                                                                IbwArgs ib) {
    // B buffers: the k-step in use's fragments are in registers; the next one's are read during it, so its
    // DMA must have landed by the barrier before: three buffers, the DMA two k-steps ahead, and vmcnt(0) per k-step
    constexpr int NBUF = 3;
    // G3 (NP 1): three k-steps per barrier, nine single-plane B buffers (one per k-step of a pair)
    constexpr bool G3 = NP == 1;
    constexpr int BSLOTS = G3 ? 9 : NBUF * 2;
    __shared__ __attribute__((aligned(16))) _Float16 smem[2 * 2 * WIN_PIX * 16 + BSLOTS * W16_BSLOT + 8];
    _Float16* const Wn = smem;                        // [2 buffers][2 planes][WIN_PIX][16]
    _Float16* const Bs = smem + 2 * 2 * WIN_PIX * 16;  // [3 buffers][2 planes][128 rows][32 k]
    _Float16* const Wspare = Bs + BSLOTS * W16_BSLOT;  // 16 bytes nobody reads

    const int T = gridDim.x;
    const int L = xcd_remap(blockIdx.x, T);
    const int ntile = L % a.gy, mt = L / a.gy;
    const int n = mt / a.tiles, tile = mt - n * a.tiles;
    const int n0 = ntile * WIN_BN;
    const int y0 = tile * a.R;
    const int W = a.W, WP = a.W + 2, C = a.C;
    const int K = 9 * C;
    const int npair = C / 32;
    const int lw = __builtin_ctz(W);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int m16 = lane & 15, g = lane >> 4;

    int ea = 0;
    float asc = 1.f;
    const int eb = __builtin_amdgcn_readfirstlane(wexp[0]);

    // window staging units of this thread: (pixel, 8-channel half) of the window's interior columns
    // ((R + 2) x W pixels: 2 units per thread at W <= 128).  uoff: byte offset of the unit's source
    // channel 0 (-1: zero padding); uwd: its window pixel (bits 0-15) and the halo pixel it also writes
    // (bits 16-31), each + 1 (0: none)
    const int nint = (a.R + 2) * W;
    int uoff[WIN_UNITS], uwd[WIN_UNITS];
#pragma unroll
    for (int q = 0; q < WIN_UNITS; ++q) {
        const int u = tid + q * WIN_NT;
        const int ip = u >> 1, h = u & 1;
        uoff[q] = -1;
        uwd[q] = 0;
        if (ip < nint) {
            const int wr = ip >> lw, sx = ip & (W - 1);
            int dup = -1;
            int sy = y0 - 1 + wr;
            bool ok = true;
            if (a.reflect) {
                sy = sy < 0 ? -sy : (sy >= a.H ? 2 * a.H - 2 - sy : sy);
                if (sx == 1) dup = wr * WP;
                else if (sx == W - 2) dup = wr * WP + W + 1;
            } else {
                ok = sy >= 0 && sy < a.H;
            }
            uwd[q] = (wr * WP + sx + 2) | ((dup + 1) << 16);
            if (ok) uoff[q] = (((n * a.H + sy) * W + sx) * C + 8 * h) * 4;
        }
    }
    if (!a.reflect) {  // zero halo columns of both buffers and planes
        for (int i = tid; i < 2 * 2 * (a.R + 2) * 2 * 2; i += WIN_NT) {
            const int h = i & 1, side = (i >> 1) & 1, rest = i >> 2;
            const int wr = rest % (a.R + 2), bp = rest / (a.R + 2);
            *reinterpret_cast<f16x8*>(Wn + w16_off(bp >> 1, bp & 1, wr * WP + side * (W + 1), h)) = f16x8{};
        }
    }
    const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), (short)0, 0x7fffff00, 0x00020000);
    f32x4v wq_[2];  // the unit in flight (ext vectors: tied operands of the wait below)
    // every global load is unconditional (a unit outside the source reads at a clamped offset, zeros):
    // a load under a branch makes the compiler wait for all outstanding loads (vmcnt(0)) at the next
    // consumer
    auto win_load_into = [&](int q, int s, f32x4v (&dst)[2]) {
        const int off = uoff[q] >= 0 ? uoff[q] + s * 64 : 0x7fffffbf;  // 16 channels = 64 B per slice
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(srsrc, off, 0, 0);
        u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(srsrc, off + 16, 0, 0);
        __builtin_memcpy(&dst[0], &v0, 16);
        __builtin_memcpy(&dst[1], &v1, 16);
    };
    auto win_load_u = [&](int q, int s) { win_load_into(q, s, wq_); };
    // unconditional store (a unit past the window writes the spare slot): a store under a branch lets
    // the compiler sink the unit's load into the branch, next to its use
    auto win_store_u = [&](int q, int buf) {
        const int h = (tid + q * WIN_NT) & 1;
        const int wp = (uwd[q] & 0xffff) - 1, wd = (uwd[q] >> 16) - 1;
        f16x8 hi, lo;
        split8h(make_float4(wq_[0][0], wq_[0][1], wq_[0][2], wq_[0][3]),
                make_float4(wq_[1][0], wq_[1][1], wq_[1][2], wq_[1][3]), asc, hi, lo);
        *reinterpret_cast<f16x8*>(wp >= 0 ? Wn + w16_off(buf, 0, wp, h) : Wspare) = hi;
        if constexpr (NP == 3) *reinterpret_cast<f16x8*>(wp >= 0 ? Wn + w16_off(buf, 1, wp, h) : Wspare) = lo;
        if (wd >= 0) {
            *reinterpret_cast<f16x8*>(Wn + w16_off(buf, 0, wd, h)) = hi;
            if constexpr (NP == 3) *reinterpret_cast<f16x8*>(Wn + w16_off(buf, 1, wd, h)) = lo;
        }
    };

    // B k-step by LDS-DMA: 16 blocks of 1 KB (plane, 16-row block), blocks 2w and 2w + 1 of wave w.  Lane
    // L of a block lands at row L / 4, 16-byte slot L % 4, which holds the row's k group
    // (L % 4 - 2 ((row >> 2) & 3)) & 3 (the rotation above; (row >> 2) & 3 = (L >> 4) & 3)
    unsigned dsu[2], ddst[2];
    const _Float16* dbase[2];
    const unsigned dlane = 2u * (unsigned)((n0 + (lane >> 2)) * K + 8 * (((lane & 3) - 2 * ((lane >> 4) & 3)) & 3));
    {
        const unsigned bs_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) _Float16*)Bs;
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // (NP 1: the hi plane's 8 blocks, block w of wave w)
            const int b = NP == 3 ? __builtin_amdgcn_readfirstlane(wid) * 2 + i : __builtin_amdgcn_readfirstlane(wid);
            const int pl = b >> 3, rb = b & 7;
            dsu[i] = 2u * (unsigned)(rb * 16 * K);
            dbase[i] = pl ? wl : wh;
            ddst[i] = __builtin_amdgcn_readfirstlane(bs_lds + 2u * (unsigned)(pl * W16_BSLOT + rb * 16 * 32));
        }
    }
    auto b_dma = [&](int j, int buf) {  // k-step j (packed k 32 j .. 32 j + 31) into B buffer buf
        const unsigned kb = 2u * (unsigned)(j * 32);
#pragma unroll
        for (int i = 0; i < (NP == 3 ? 2 : 1); ++i)
            win_glds(dbase[i], dlane + (dsu[i] + kb), ddst[i] + 2u * (unsigned)(buf * 2 * W16_BSLOT));
    };

    // fragment offsets (halves).  A: window pixel of row block i at tap (0, 0) = ublk[i] + m16 (wave-
    // uniform block part); k group g reads channel half g & 1 of the unit of its lane half.  B: row
    // wn * 64 + 16 j + m16, k group g in slot (g + 2 ((m16 >> 2) & 3)) & 3.
    // (W >= 64: the wave's four blocks are consecutive pixels of one row, block offsets 256 i halves
    // fold into the reads' immediate offsets; narrower images add a uniform offset per block)
    int ublk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = wm * 64 + 16 * i;
        ublk[i] = __builtin_amdgcn_readfirstlane(((q >> lw) * WP + (q & (W - 1))) * 16);
    }
    const int alane = ublk[0] + m16 * 16 + 8 * (g & 1);
    const int blane = (wn * 64 + m16) * 32 + 8 * ((g + 2 * ((m16 >> 2) & 3)) & 3);
    const bool hiu = g >= 2;  // this lane's k groups take the k-step's second unit

    f32x4v acc[4][4], t[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f}; t[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f}; }

    if constexpr (G3) {
    // NP 1 (f16 operands, hi planes only): one product per fragment pair leaves 16 MFMAs per wave and k-step,
    // so the k-steps of a pair run in three groups of three between barriers (48 MFMAs per wave per barrier,
    // as one f16x3 k-step).  B: one single-plane buffer per k-step of a pair (buffer = js), the DMA for group
    // g + 2 issued at the top of group g.  Window: the lo-plane slots are free, so slices rotate through four
    // single-plane slots (slice s in slot s & 3): the next pair's even slice is loaded in group 0 and stored at
    // the top of group 1 (published before group 2 reads its first fragments for the next pair), the odd one
    // loaded in group 1 and stored at the top of group 2 (published before the next pair's group 1).
    const unsigned bsl = (unsigned)(uintptr_t)(__attribute__((address_space(3))) _Float16*)Bs;
    const unsigned ddst1 = __builtin_amdgcn_readfirstlane(bsl + 2u * (unsigned)(wid * 16 * 32));
    auto dma1 = [&](int j, int buf) {  // k-step j (packed k 32 j ..) into single-plane buffer buf
        win_glds(dbase[0], dlane + (dsu[0] + 2u * (unsigned)(j * 32)), ddst1 + 2u * (unsigned)(buf * W16_BSLOT));
    };
    auto dma_group = [&](int p_, int g_) {  // group g_ of pair p_
#pragma unroll
        for (int k = 0; k < 3; ++k) dma1(9 * p_ + 3 * g_ + k, 3 * g_ + k);
    };
    f32x4v wq1[2];
    auto store_slot = [&](int q, int slot, const f32x4v (&v)[2]) {
        const int h = (tid + q * WIN_NT) & 1;
        const int wp = (uwd[q] & 0xffff) - 1, wd = (uwd[q] >> 16) - 1;
        f16x8 hi, lo;
        split8h(make_float4(v[0][0], v[0][1], v[0][2], v[0][3]), make_float4(v[1][0], v[1][1], v[1][2], v[1][3]),
                asc, hi, lo);
        *reinterpret_cast<f16x8*>(wp >= 0 ? Wn + (slot * WIN_PIX + wp) * 16 + 8 * h : Wspare) = hi;
        if (wd >= 0) *reinterpret_cast<f16x8*>(Wn + (slot * WIN_PIX + wd) * 16 + 8 * h) = hi;
    };
    auto load_slice = [&](int sl) {  // both units of slice sl: unit 0 into wq_, unit 1 into wq1
        win_load_into(0, sl, wq_);
        win_load_into(1, sl, wq1);
    };
    auto store_slice = [&](int sl) {
        store_slot(0, sl & 3, wq_);
        store_slot(1, sl & 3, wq1);
    };
    // prologue: B groups 0 and 1 of pair 0, slices 0 and 1, the exponent
    dma_group(0, 0);
    dma_group(0, 1);
    load_slice(0);
    ea = f16x3_exp(rng, a.rng_n);
    asc = __builtin_ldexpf(1.f, ea);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(wq_[0]), "+v"(wq_[1]), "+v"(wq1[0]), "+v"(wq1[1]) : : "memory");
    store_slice(0);
    load_slice(1);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(wq_[0]), "+v"(wq_[1]), "+v"(wq1[0]), "+v"(wq1[1]) : : "memory");
    store_slice(1);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();

    f16x8 bh[4], ah[2];
    auto a_base1 = [&](int js_, int podd) {  // A base of k-step js_ (units 2 js_, 2 js_ + 1) of a pair
        const int u0 = 2 * js_, u1 = 2 * js_ + 1;
        const int t0 = u0 % 9, t1 = u1 % 9;
        const int o0 = (2 * podd + u0 / 9) * WIN_PIX * 16 + ((t0 / 3) * WP + t0 % 3) * 16;
        const int o1 = (2 * podd + u1 / 9) * WIN_PIX * 16 + ((t1 / 3) * WP + t1 % 3) * 16;
        int al_ = alane;
        asm volatile("" : "+v"(al_));
        return Wn + al_ + (hiu ? o1 : o0);
    };
    auto b_base1 = [&](int buf) {
        int bl_ = blane;
        asm volatile("" : "+v"(bl_));
        return Bs + buf * W16_BSLOT + bl_;
    };
    auto rd_a1 = [&](const _Float16* Ak, int i, int slot) {
        const int bo = WIDE ? 256 * i : ublk[i] - ublk[0];
        ah[slot] = *reinterpret_cast<const f16x8*>(Ak + bo);
    };
    {  // k-step 0's fragments
        rd_a1(a_base1(0, 0), 0, 0);
        const _Float16* const B0 = b_base1(0);
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) bh[jb] = *reinterpret_cast<const f16x8*>(B0 + jb * 16 * 32);
    }
    for (int p = 0; p < npair; ++p) {
        const int podd = p & 1;
        const bool more = p + 1 < npair;  // (block-uniform)
#pragma unroll
        for (int g_ = 0; g_ < 3; ++g_) {
            // group top: the staging of the next pair's slices, and the B DMA two groups ahead
            if (g_ == 0) {
                dma_group(p, 2);
                if (more) load_slice(2 * p + 2);
            } else if (g_ == 1) {
                if (more) {
                    store_slice(2 * p + 2);
                    dma_group(p + 1, 0);
                    load_slice(2 * p + 3);
                }
            } else {
                if (more) {
                    store_slice(2 * p + 3);
                    dma_group(p + 1, 1);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const int js = 3 * g_ + kk;
                const _Float16* const Ak = a_base1(js, podd);
                const _Float16* const An = js < 8 ? a_base1(js + 1, podd) : a_base1(0, podd ^ 1);
                const _Float16* const Bn = b_base1(js < 8 ? js + 1 : 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < 3) rd_a1(Ak, i + 1, (i + 1) & 1);
                    else rd_a1(An, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) {
                        t[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i & 1], bh[jb], t[i][jb], 0, 0, 0);
                        if (i == 3) bh[jb] = *reinterpret_cast<const f16x8*>(Bn + jb * 16 * 32);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (js == 4 || js == 8) {  // close the accumulation chain (160 / 128 k)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            acc[i][jj] += t[i][jj];
                            asm volatile("" : "+v"(acc[i][jj]));
                            t[i][jj] = f32x4v{0.f, 0.f, 0.f, 0.f};
                        }
                }
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the group's DMAs and stores landed
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    } else {
    // prologue: window of slice 0 (buffer 0) and B k-steps 0 and 1, every load (and the exponent's) in
    // flight before the first store
    b_dma(0, 0);
    b_dma(1, 1);
    f32x4v wp1[2];
    win_load_into(1, 0, wp1);
    win_load_u(0, 0);
    ea = f16x3_exp(rng, a.rng_n);
    asc = __builtin_ldexpf(1.f, ea);
    // vmcnt(0): the units (asm, tied to their registers)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(wq_[0]), "+v"(wq_[1]), "+v"(wp1[0]), "+v"(wp1[1]) : : "memory");
    win_store_u(0, 0);
    wq_[0] = wp1[0];
    wq_[1] = wp1[1];
    win_store_u(1, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the DMAs have landed (asm: kept)
    __syncthreads();

    const int nstep = 9 * npair;
    // fragments carried across k-steps: the k-step's B (four column blocks) and the A row block in use
    // plus the next one.  Row block i's MFMAs run with block i + 1's A (or, at i = 3, the next k-step's
    // block 0) in flight, and during i = 3 each column block's B is replaced by the next k-step's right
    // after its last MFMA: the reads a k-step needs are issued during the previous one, so no wave
    // starts a k-step with its LDS reads queued behind eight waves' bursts.  That needs B k-step j + 1
    // readable during k-step j: three B buffers (k-step j in buffer j % 3 = js % 3, the DMA for j + 2
    // issued at the top of j), and each window slice published one k-step before its first fragment
    // read (see the staging windows below).
    f16x8 bh[4], bl[4], ah[2], al[2];
    auto a_base = [&](int js_) {  // this lane's A base of k-step js_ of a pair (units 2 js_, 2 js_ + 1)
        const int u0 = 2 * js_, u1 = 2 * js_ + 1;
        const int t0 = u0 % 9, t1 = u1 % 9;
        const int o0 = (u0 / 9) * 2 * WIN_PIX * 16 + ((t0 / 3) * WP + t0 % 3) * 16;
        const int o1 = (u1 / 9) * 2 * WIN_PIX * 16 + ((t1 / 3) * WP + t1 % 3) * 16;
        // (through an empty asm: hoisted out of the loop, the nine k-steps' bases stayed live and spilled)
        int al_ = alane;
        asm volatile("" : "+v"(al_));
        return Wn + al_ + (hiu ? o1 : o0);
    };
    auto b_base = [&](int buf) {
        int bl_ = blane;
        asm volatile("" : "+v"(bl_));
        return Bs + buf * 2 * W16_BSLOT + bl_;
    };
    auto rd_a = [&](const _Float16* Ak, int i, int slot) {
        const int bo = WIDE ? 256 * i : ublk[i] - ublk[0];
        if constexpr (NP == 3) al[slot] = *reinterpret_cast<const f16x8*>(Ak + bo + WIN_PIX * 16);
        ah[slot] = *reinterpret_cast<const f16x8*>(Ak + bo);
    };
    auto rd_b = [&](const _Float16* Bk, int jb) {
        bh[jb] = *reinterpret_cast<const f16x8*>(Bk + jb * 16 * 32);
        if constexpr (NP == 3) bl[jb] = *reinterpret_cast<const f16x8*>(Bk + jb * 16 * 32 + W16_BSLOT);
    };
    {  // k-step 0's fragments (published by the prologue's barrier)
        rd_a(a_base(0), 0, 0);
        const _Float16* const B0 = b_base(0);
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) rd_b(B0, jb);
    }
    auto kloop = [&](auto role_tag) {
        constexpr int ROLE = decltype(role_tag)::value;
        for (int p = 0; p < npair; ++p) {
            // staging windows (one unit in flight per thread): the odd slice 2p + 1 into window buffer 1 in
            // k-steps 0-2 (buffer 1's previous slice had its last fragment read in the previous pair's
            // k-step 8; its first read is k-step 4's block 0, issued in k-step 3), the next even slice into
            // buffer 0 in k-steps 5-7 (last read of slice 2p in k-step 4; first read of slice 2p + 2 in
            // k-step 8 for the next pair's k-step 0)
            const int s_odd = 2 * p + 1;
            const int s_even = 2 * p + 2 < 2 * npair ? 2 * p + 2 : 2 * p;  // past the end a repeat nobody reads
#pragma unroll
            for (int js = 0; js < 9; ++js) {
                const int j = 9 * p + js;
                const int ph = js < 3 ? js : (js >= 5 && js < 8 ? js - 5 : -1);  // position in a staging window
                const int sbuf = js < 3 ? 1 : 0, ssl = js < 3 ? s_odd : s_even;
                if constexpr (ROLE == 1) {  // unit ph - 1 stored at the top of the next k-step
                    if (ph == 1 || ph == 2) win_store_u(ph - 1, sbuf);
                }
                if (ph == 0 || ph == 1) win_load_u(ph, ssl);
                b_dma(j + NBUF - 1 < nstep ? j + NBUF - 1 : nstep - 1, (j + NBUF - 1) % NBUF);
                __builtin_amdgcn_sched_barrier(0);  // the loads stay at the top of the k-step
                const _Float16* const Ak = a_base(js);
                const _Float16* const An = a_base((js + 1) % 9);
                const _Float16* const Bn = b_base((j + 1) % NBUF);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < 3) rd_a(Ak, i + 1, (i + 1) & 1);
                    else rd_a(An, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int jb = 0; jb < 4; ++jb) {
                        const int sl = i & 1;
                        if constexpr (NP == 3) {
                            t[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[sl], bh[jb], t[i][jb], 0, 0, 0);
                            t[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[sl], bl[jb], t[i][jb], 0, 0, 0);
                        }
                        t[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[sl], bh[jb], t[i][jb], 0, 0, 0);
                        if (i == 3) rd_b(Bn, jb);  // the next k-step's column block jb
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (ROLE == 0) {
                    if (ph == 0 || ph == 1) win_store_u(ph, sbuf);
                }
                if (js == 4 || js == 8) {  // close the accumulation chain (160 / 128 k)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            acc[i][jj] += t[i][jj];
                            // (pinned here: sunk to the next closure, the sum kept both chains live and spilled)
                            asm volatile("" : "+v"(acc[i][jj]));
                            t[i][jj] = f32x4v{0.f, 0.f, 0.f, 0.f};
                        }
                }
                __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0): this wave's DMAs (and window loads) landed
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (wid >= 4) kloop(std::integral_constant<int, 1>{});  // (wave-uniform branch)
    else kloop(std::integral_constant<int, 0>{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last (repeat) DMAs landed before the epilogue
    }

    // epilogue: undo the operand scales, + addend, NHWC store, IN statistics
    const int eab = -(ea + eb);
    const int p0 = y0 * W;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = __builtin_ldexpf(acc[i][j][r], eab);
    const long long obase = (long long)n * a.H * W * a.Co;
    auto ooff = [&](int i, int j, int r) {
        const int pix = p0 + wm * 64 + 16 * i + 4 * g + r;
        return obase + (long long)pix * a.Co + n0 + wn * 64 + j * 16 + m16;
    };
    if (addend) {  // wave-uniform: all 64 addend loads issued before the first use
        float ad[4][4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) ad[i][j][r] = addend[ooff(i, j, r)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[ooff(i, j, r)] = acc[i][j][r] + ad[i][j][r];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) out[ooff(i, j, r)] = acc[i][j][r];
    }
    if (parts) win16_stats(acc, p0, n0, a.Co, wm, wn, lane, tid, reinterpret_cast<float*>(smem), parts,
                           (long long)n * a.tiles + tile);
    if constexpr (IBW) {
        float yv[4][4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) yv[i][j][r] = ib.y[ooff(i, j, r)];
        win16_ibw(acc, yv, ib, n, p0, a.H, W, a.Co, n0, wm, wn, lane, tid, tile, reinterpret_cast<float*>(smem));
    }
}

// pre-split weight pack (dcs_pack_weights_h3): the range of the raw weights first, then every block
// derives the same exponent and writes hi / lo fp16 planes of the slice-major B
__global__ __launch_bounds__(256) void wrange_kernel(const float* __restrict__ w, long long n, float* __restrict__ parts) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        m = fmaxf(m, fabsf(w[i]));
    __shared__ float red[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (blockIdx.x == 0)  // a grid smaller than the record: the remaining partial maxima are zero
        for (int i = gridDim.x + threadIdx.x; i < DCS_RANGE_PARTS; i += blockDim.x) parts[i] = 0.f;
}

__global__ __launch_bounds__(256) void pack_h3_kernel(const float* __restrict__ w, int Cout, int Cin, int flip,
                                                      int ncols, const float* __restrict__ parts, int nparts,
                                                      _Float16* __restrict__ oh, _Float16* __restrict__ ol,
                                                      int* __restrict__ wexp) {
    const int e = f16x3_exp(parts, nparts);  // every wave derives the same exponent
    const float sc = __builtin_ldexpf(1.f, e);
    if (blockIdx.x == 0 && threadIdx.x == 0) wexp[0] = e;
    const int C = flip ? Cout : Cin;  // reduction channels per tap
    const int K = 9 * C;
    const long long total = (long long)ncols * K;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int col = (int)(idx / K), k = (int)(idx - (long long)col * K);
        const int slice = k / 144, rem = k - slice * 144;
        const int tap = rem >> 4, c = slice * 16 + (rem & 15);
        int ty = tap / 3, tx = tap - 3 * (tap / 3);
        float v = 0.f;
        if (!flip) {  // forward: B[k][co] = W[co][c][ty][tx]
            if (col < Cout) v = w[(((long long)col * Cin + c) * 3 + ty) * 3 + tx];
        } else {      // data gradient: B[k][ci] = W[c][ci][2-ty][2-tx] (c = output channel of the forward)
            if (col < Cin) v = w[(((long long)c * Cin + col) * 3 + (2 - ty)) * 3 + (2 - tx)];
        }
        const float f = v * sc;
        const _Float16 h = (_Float16)f, l = (_Float16)(f - (float)h);
        oh[idx] = h;
        ol[idx] = l;
        if (flip) {  // the tap-major copy behind the planes (k = tap * C + c: the ring kernel's B)
            const long long t = total + (long long)col * K + tap * C + c;
            oh[t] = h;
            ol[t] = l;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Weight gradient of the residual 3x3 convs on a rolling source window (the f16 mode: wgrad3_win_h3_kernel,
// hi planes only; f16x3 runs the same design on the 16x16x32 MFMA, wgrad3_win16_kernel below):
//   dW[co][ci][ty][tx] = sum_p dy[p][co] * xpad[p + (ty - 1, tx - 1)][ci]
// conv.hip's conv_wgrad_x6_kernel owns a 128 (co) x 128 ((tap, ci)) tile and gathers the source at
// each tap's offset: every source value is fetched, split and staged once per tap column group
// (nine times).  Here a workgroup owns 64 co x 64 ci x all nine taps and walks one 64-pixel-wide
// strip of an image row by row: per row it stages the dy row segment (64 px x 64 co) and ONE new
// source row segment (66 px with the halo x 64 ci) into a ring of rows, converted to fp16 once; the
// nine taps read their fragments from the ring at a per-tap (row slot, pixel) offset.
// MFMA shape: M = co (32), N = ci (32), K = 16 pixels of the row; both operands pixel-major in LDS,
// fragments by ds_read_b64_tr_b16 (8 consecutive pixels of one channel per lane).  8 waves, two per
// SIMD: waves w and w + 4 (same SIMD) own co block (w & 1) x ci block ((w >> 1) & 1), wave w taps
// 0..3 and wave w + 4 taps 5..8, tap 4 split between them by pixel sub-tile (ww_k / ww_tap), so each
// SIMD carries all nine taps of one 32 x 32 (co, ci) block, 18 MFMA groups per wave, and each wave
// five accumulators (two-level: a chain of two rows = 128 pixels, then added to
// the running sum), leaving registers for fragment reads ahead and a second wave to cover LDS
// latency.  Per row and SIMD: 4 pixel sub-tiles x 9 taps = 36 MFMAs, two rows between barriers.
// LDS (halves): ring [8 slots][66 px][64 ch], dy [4 buffers][64 px][64 ch];
// 16-byte channel units swizzled by bit 1 of the pixel index (unit ^ 4), so the four consecutive
// pixels of a transposed read land on the four 64-byte quarters of the banks at any tap offset.
// Partial sums per (image, strip, row chunk) go to slabs [split][co][tap * C + ci] (the layout of
// conv.hip's split-K weight gradient), summed by its reduce kernel.
constexpr int WW_NT = 512, WW_SW = 64, WW_WP = WW_SW + 2;
constexpr int WW_XU = (WW_WP * 8 + WW_NT - 1) / WW_NT;  // source-row (pixel, 8-channel unit)s per thread: 2
constexpr int WW_TPW = 5;                                // taps per wave (5 + 4)

struct WWArgs {
    int N, H, W, C, Co;  // source NHWC [N][H][W][C]; dy NHWC [N][H][W][Co]
    int reflect;         // 1: reflection padding, 0: zero padding
    int strips, rchunks, rows_per;  // 64-pixel strips per row, row chunks per strip, rows per chunk
    int gco, gci;        // 64-channel tiles of co / ci
    int rng_a_n, rng_b_n;
};

__device__ __forceinline__ int ww_swz(int pix) { return ((pix >> 1) & 1) << 2; }

typedef short wshortx4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) wshortx4 lds_wshortx4;

__device__ __forceinline__ f16x8 ww_frag(const _Float16* p) {
    const wshortx4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_wshortx4*)(p));
    const wshortx4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_wshortx4*)(p + 4 * 64));
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// (sub-tile k, tap) of a wave's j-th MFMA group in a row: the 36 pairs of a SIMD split 18 / 18
// between its two waves, tap 4 shared (role 0: taps 0..4 on sub-tiles 0, 1 and taps 0..3 on 2, 3;
// role 1: taps 5..8 on sub-tiles 0, 1 and taps 4..8 on 2, 3), so neither wave runs alone at the
// row's end; the two partial sums of tap 4 meet in the epilogue
__host__ __device__ constexpr int ww_k(int r, int j) { return r == 0 ? (j < 10 ? j / 5 : 2 + (j - 10) / 4) : (j < 8 ? j / 4 : 2 + (j - 8) / 5); }
__host__ __device__ constexpr int ww_tap(int r, int j) { return r == 0 ? (j < 10 ? j % 5 : (j - 10) % 4) : (j < 8 ? 5 + j % 4 : 4 + (j - 8) % 5); }
__host__ __device__ constexpr int ww_acc(int r, int tap) { return r == 0 ? tap : (tap == 4 ? 4 : tap - 5); }

template <int NP>  // (kept so the kernel's symbol stays wgrad3_win_h3_kernel<1>, which the profile tables key on)
__global__ __launch_bounds__(WW_NT, 1) void wgrad3_win_h3_kernel(WWArgs a, const float* __restrict__ dy,
                                                                 const float* __restrict__ src,
                                                                 const float* __restrict__ rnga,
                                                                 const float* __restrict__ rngb,
                                                                 float* __restrict__ ws) {
    static_assert(NP == 1, "the f16 mode's kernel; f16x3 runs wgrad3_win16_kernel");
    // f16 (hi planes only): one product per fragment pair leaves 36 MFMAs per SIMD and row, so two rows run
    // per barrier: a ring of 8 source rows [66][64] and 4 dy buffers [64][64].
    constexpr int RPB = 2;             // image rows per barrier
    constexpr int NXS = 8;             // source-row ring slots
    constexpr int NDB = 4;             // dy buffers
    constexpr int XROW = WW_WP * 64;   // halves per ring slot
    constexpr int DROW = WW_SW * 64;   // halves per dy buffer
    __shared__ __attribute__((aligned(16))) _Float16 smem[NXS * XROW + NDB * DROW];
    _Float16* const Xr = smem;                 // [NXS][66][64]
    _Float16* const Dy = smem + NXS * XROW;    // [NDB][64][64]

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int ntile = a.gco * a.gci;
    const int tile = L % ntile, split = L / ntile;
    const int co0 = (tile % a.gco) * 64, ci0 = (tile / a.gco) * 64;
    const int rc = split % a.rchunks, rest = split / a.rchunks;
    const int strip = rest % a.strips, n = rest / a.strips;
    const int x0 = strip * WW_SW;
    const int H = a.H, W = a.W, C = a.C, Co = a.Co;
    const int y_beg = rc * a.rows_per;
    const int y_end = y_beg + a.rows_per < H ? y_beg + a.rows_per : H;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cob = wid & 1, cib = (wid >> 1) & 1, half = wid >> 2;

    // the operand exponents are read in the prologue, beside the first rows' loads
    int ea = 0, eb = 0;
    float asc = 1.f, bsc = 1.f;

    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), (short)0, 0x7fffff00, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), (short)0, 0x7fffff00, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr int OOB = 0x7fffffbf;

    // dy row segment: 64 px x 8 units, one per thread; byte offset within the row
    int doff, dls;
    {
        const int pix = tid >> 3, cu = tid & 7;
        doff = ((x0 + pix) * Co + co0 + 8 * cu) * 4;
        dls = pix * 64 + 8 * (cu ^ ww_swz(pix));
    }
    // source row segment: 66 px (halo included) x 8 units; byte offset within the row (-1: none)
    int xoff[WW_XU], xls[WW_XU];
#pragma unroll
    for (int q = 0; q < WW_XU; ++q) {
        const int u = tid + q * WW_NT, wc = u >> 3, cu = u & 7;
        xoff[q] = -1;
        xls[q] = -1;
        if (wc < WW_WP) {
            int sx = x0 - 1 + wc;
            bool ok = true;
            if (a.reflect) sx = sx < 0 ? -sx : (sx >= W ? 2 * W - 2 - sx : sx);
            else ok = sx >= 0 && sx < W;
            if (ok) xoff[q] = (sx * C + ci0 + 8 * cu) * 4;
            xls[q] = wc * 64 + 8 * (cu ^ ww_swz(wc));
        }
    }
    float4 dr[2], xr[WW_XU][2];  // the row in flight
    auto ld_dy = [&](int y) {
        const int rb = ((n * H + y) * W) * Co * 4;
        u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(drs, rb + doff, 0, 0);
        u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(drs, rb + doff + 16, 0, 0);
        __builtin_memcpy(&dr[0], &v0, 16);
        __builtin_memcpy(&dr[1], &v1, 16);
    };
    auto ld_x = [&](int r) {  // logical source row r in [-1, H]
        int sy = r;
        bool ok = true;
        if (a.reflect) sy = sy < 0 ? -sy : (sy >= H ? 2 * H - 2 - sy : sy);
        else ok = sy >= 0 && sy < H;
        const int rb = ((n * H + sy) * W) * C * 4;
#pragma unroll
        for (int q = 0; q < WW_XU; ++q) {
            const int off = (ok && xoff[q] >= 0) ? rb + xoff[q] : OOB;
            u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0);
            u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(xrs, off + 16, 0, 0);
            __builtin_memcpy(&xr[q][0], &v0, 16);
            __builtin_memcpy(&xr[q][1], &v1, 16);
        }
    };
    auto st_dy = [&](int buf) {
        f16x8 hi, lo;
        split8h(dr[0], dr[1], asc, hi, lo);
        *reinterpret_cast<f16x8*>(Dy + buf * DROW + dls) = hi;
    };
    auto st_x = [&](int slot) {
#pragma unroll
        for (int q = 0; q < WW_XU; ++q) {
            if (xls[q] >= 0) {
                f16x8 hi, lo;
                split8h(xr[q][0], xr[q][1], bsc, hi, lo);
                *reinterpret_cast<f16x8*>(Xr + slot * XROW + xls[q]) = hi;
            }
        }
    };

    // transposed-read lane offsets (halves): lane (r, h) of a fragment gets pixels 8h .. 8h+7 of
    // channel r of its 32-channel block; in a 16-lane group lane 4q+p reads pixel row q (+4: second
    // read), channels 4p .. 4p+3
    const int g16 = lane >> 4;
    const int rpix = 8 * (g16 >> 1) + ((lane & 15) >> 2);
    const int rcol = 16 * (g16 & 1) + 4 * (lane & 3);
    int aoff, boff[3];
    {
        const int c = 32 * cob + rcol;
        aoff = rpix * 64 + 8 * ((c >> 3) ^ ww_swz(rpix)) + (c & 7);
        const int cb = 32 * cib + rcol;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            const int p = rpix + tx;
            boff[tx] = p * 64 + 8 * ((cb >> 3) ^ ww_swz(p)) + (cb & 7);
        }
    }

    floatx16 acc[WW_TPW], t[WW_TPW];
#pragma unroll
    for (int i = 0; i < WW_TPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; t[i][r] = 0.f; }

    // prologue: source rows y_beg - 1 .. y_beg + RPB into their ring slots, dy rows y_beg .. y_beg + RPB - 1;
    // every row's loads (and the exponents') in flight before the first store
    {
        float4 px_[RPB + 2][WW_XU][2], pd_[RPB][2];
#pragma unroll
        for (int i = 0; i < RPB + 2; ++i) {
            const int r = y_beg - 1 + i;
            ld_x(r <= H ? r : H);
#pragma unroll
            for (int q = 0; q < WW_XU; ++q) { px_[i][q][0] = xr[q][0]; px_[i][q][1] = xr[q][1]; }
        }
#pragma unroll
        for (int i = 0; i < RPB; ++i) {
            const int r = y_beg + i;
            ld_dy(r < y_end ? r : y_end - 1);
            pd_[i][0] = dr[0];
            pd_[i][1] = dr[1];
        }
        ea = f16x3_exp(rnga, a.rng_a_n);
        eb = f16x3_exp(rngb, a.rng_b_n);
        asc = __builtin_ldexpf(1.f, ea);
        bsc = __builtin_ldexpf(1.f, eb);
#pragma unroll
        for (int i = 0; i < RPB + 2; ++i) {
#pragma unroll
            for (int q = 0; q < WW_XU; ++q) { xr[q][0] = px_[i][q][0]; xr[q][1] = px_[i][q][1]; }
            st_x((y_beg - 1 + i) & (NXS - 1));
        }
#pragma unroll
        for (int i = 0; i < RPB; ++i) {
            dr[0] = pd_[i][0];
            dr[1] = pd_[i][1];
            st_dy((y_beg + i) & (NDB - 1));
        }
    }
    __syncthreads();

    // one row of this wave's taps T0 .. T0 + NT_ - 1: 4 pixel sub-tiles x NT_ taps, the fragments of
    // the next (sub-tile, tap) read before the MFMAs of the current one
    auto row = [&](int y, auto tag) {
        constexpr int R = decltype(tag)::value;
        constexpr int NJ = 18;  // (sub-tile, tap) pairs of this wave
        const _Float16* const Db = Dy + (y & (NDB - 1)) * DROW;
        const _Float16* Xs[3];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) Xs[ty] = Xr + ((y + NXS - 1 + ty) & (NXS - 1)) * XROW;  // row y - 1 + ty
        auto rdA = [&](int k) { return ww_frag(Db + aoff + k * 16 * 64); };
        auto rdB = [&](int j) {
            const int k = ww_k(R, j), tap = ww_tap(R, j), ty = tap / 3, tx = tap % 3;
            return ww_frag(Xs[ty] + boff[tx] + k * 16 * 64);
        };
        f16x8 ah = rdA(0), bh = rdB(0), nah, nbh;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j + 1 < NJ) {
                if (ww_k(R, j + 1) != ww_k(R, j)) nah = rdA(ww_k(R, j + 1));
                nbh = rdB(j + 1);
            }
            floatx16& tt = t[ww_acc(R, ww_tap(R, j))];
            tt = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, tt, 0, 0, 0);
            // stage the row loaded above into the buffers no row of this barrier reads, at the row's end
            // (mid-row hid too little of the loads' latency)
            if (j == NJ - 1) {
                st_dy((y + RPB) & (NDB - 1));
                st_x((y + RPB + 1) & (NXS - 1));
            }
            bh = nbh;
            if (j + 1 < NJ && ww_k(R, j + 1) != ww_k(R, j)) ah = nah;
        }
    };

#pragma unroll 1
    for (int y = y_beg; y < y_end; y += 2) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int yr = y + q;
            if (yr < y_end) {  // (block-uniform)
                // next rows in flight, staged at the row's end into the buffers no row of this barrier reads
                ld_dy(yr + 2 < y_end ? yr + 2 : y_end - 1);
                ld_x(yr + 3 <= H ? yr + 3 : H);
                if (half == 0) row(yr, std::integral_constant<int, 0>{});
                else row(yr, std::integral_constant<int, 1>{});
            }
        }
#pragma unroll
        for (int i = 0; i < WW_TPW; ++i) {  // chains of two rows
            acc[i] += t[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) t[i][r] = 0.f;
        }
        __syncthreads();
    }

    // epilogue: the two halves of tap 4 summed through LDS (free after the loop's last barrier), then
    // undo the operand scales, slab [split][co][tap * C + ci]
    float* const t4 = reinterpret_cast<float*>(smem) + (wid & 3) * 64 * 16 + lane;
    if (half == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) t4[r * 64] = acc[4][r];
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[4][r] += t4[r * 64];
    }
    const int eab = -(ea + eb);
    float* const slab = ws + (long long)split * Co * 9 * C;
    const int col = ci0 + 32 * cib + (lane & 31);
#pragma unroll
    for (int i = 0; i < WW_TPW; ++i) {
        const int tap = half == 0 ? i : (i == 4 ? 9 : 5 + i);
        if (tap < 9) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = co0 + 32 * cob + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                slab[(long long)row * 9 * C + tap * C + col] = __builtin_ldexpf(acc[i][r], eab);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// The residual weight gradient on v_mfma_f32_16x16x32_f16 (f16x3; same workgroup, rolling window,
// staging and slabs as wgrad3_win_h3_kernel above, the MFMA shape the window conv moved to for the
// power-limited clock, conv3_win16_kernel).  M = 16 output channels, N = 16 input channels, K = 32
// pixels of the row: two k-steps per 64-pixel row.  A SIMD's waves w and w + 4 still share one
// 32 x 32 (co, ci) block = 2 x 2 sub-blocks of 16 x 16; wave w takes taps 0-3 on all four
// sub-blocks and tap 4 on the co sub-block 0, wave w + 4 taps 5-8 and tap 4 on co sub-block 1: 18
// accumulators each, no shared accumulator to merge.  Fragments by ds_read_b64_tr_b16 (lane group
// g = lane >> 4 takes pixels 8 g .. 8 g + 7 of the k-step, lane 4 q + p of the group addresses pixel
// row q (+ 4 for the second read), channels 4 p .. 4 p + 3).  The 16-byte channel units of a pixel
// row are XOR-swizzled by bits 1 and 3 of the pixel (ww16_swz), which spreads the eight pixel rows
// of a 32-lane read group (rows r .. r + 3 and r + 8 .. r + 11) over all 64 banks at any tap offset;
// the unit index's bit 1 is the 16-channel sub-block, so the second sub-block's fragment is the first
// one's offset XOR 16 halves.
__device__ __forceinline__ int ww16_swz(int pix) { return (((pix >> 1) & 1) << 2) | (((pix >> 3) & 1) << 1); }

__device__ __forceinline__ f16x8 ww16_frag(const _Float16* p1, const _Float16* p2) {
    const wshortx4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_wshortx4*)(p1));
    const wshortx4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_wshortx4*)(p2));
    return __builtin_bit_cast(f16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int NP>  // (kept so the kernel's symbol stays wgrad3_win16_kernel<3>, which the profile tables key on)
__global__ __launch_bounds__(WW_NT, 1) void wgrad3_win16_kernel(WWArgs a, const float* __restrict__ dy,
                                                                const float* __restrict__ src,
                                                                const float* __restrict__ rnga,
                                                                const float* __restrict__ rngb,
                                                                float* __restrict__ ws) {
    static_assert(NP == 3, "the f16x3 mode's kernel; f16 runs wgrad3_win_h3_kernel");
    constexpr int RPB = 1;  // image rows per barrier
    constexpr int NXS = 4;  // source-row ring slots
    constexpr int NDB = 2;  // dy buffers
    constexpr int XROW = 2 * WW_WP * 64;  // halves per ring slot (hi and lo planes)
    constexpr int DROW = 2 * WW_SW * 64;  // halves per dy buffer
    __shared__ __attribute__((aligned(16))) _Float16 smem[NXS * XROW + NDB * DROW];
    _Float16* const Xr = smem;                 // [NXS slots][planes][66][64]
    _Float16* const Dy = smem + NXS * XROW;    // [NDB buffers][planes][64][64]

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int ntile = a.gco * a.gci;
    const int tile = L % ntile, split = L / ntile;
    const int co0 = (tile % a.gco) * 64, ci0 = (tile / a.gco) * 64;
    const int rc = split % a.rchunks, rest = split / a.rchunks;
    const int strip = rest % a.strips, n = rest / a.strips;
    const int x0 = strip * WW_SW;
    const int H = a.H, W = a.W, C = a.C, Co = a.Co;
    const int y_beg = rc * a.rows_per;
    const int y_end = y_beg + a.rows_per < H ? y_beg + a.rows_per : H;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cob = wid & 1, cib = (wid >> 1) & 1, half = wid >> 2;

    int ea = 0, eb = 0;
    float asc = 1.f, bsc = 1.f;

    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), (short)0, 0x7fffff00, 0x00020000);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), (short)0, 0x7fffff00, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr int OOB = 0x7fffffbf;

    int doff, dls;
    {
        const int pix = tid >> 3, cu = tid & 7;
        doff = ((x0 + pix) * Co + co0 + 8 * cu) * 4;
        dls = pix * 64 + 8 * (cu ^ ww16_swz(pix));
    }
    int xoff[WW_XU], xls[WW_XU];
#pragma unroll
    for (int q = 0; q < WW_XU; ++q) {
        const int u = tid + q * WW_NT, wc = u >> 3, cu = u & 7;
        xoff[q] = -1;
        xls[q] = -1;
        if (wc < WW_WP) {
            int sx = x0 - 1 + wc;
            bool ok = true;
            if (a.reflect) sx = sx < 0 ? -sx : (sx >= W ? 2 * W - 2 - sx : sx);
            else ok = sx >= 0 && sx < W;
            if (ok) xoff[q] = (sx * C + ci0 + 8 * cu) * 4;
            xls[q] = wc * 64 + 8 * (cu ^ ww16_swz(wc));
        }
    }
    float4 dr[2], xr[WW_XU][2];  // the row in flight
    auto ld_dy = [&](int y) {
        const int rb = ((n * H + y) * W) * Co * 4;
        u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(drs, rb + doff, 0, 0);
        u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(drs, rb + doff + 16, 0, 0);
        __builtin_memcpy(&dr[0], &v0, 16);
        __builtin_memcpy(&dr[1], &v1, 16);
    };
    auto ld_x = [&](int r) {  // logical source row r in [-1, H]
        int sy = r;
        bool ok = true;
        if (a.reflect) sy = sy < 0 ? -sy : (sy >= H ? 2 * H - 2 - sy : sy);
        else ok = sy >= 0 && sy < H;
        const int rb = ((n * H + sy) * W) * C * 4;
#pragma unroll
        for (int q = 0; q < WW_XU; ++q) {
            const int off = (ok && xoff[q] >= 0) ? rb + xoff[q] : OOB;
            u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(xrs, off, 0, 0);
            u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(xrs, off + 16, 0, 0);
            __builtin_memcpy(&xr[q][0], &v0, 16);
            __builtin_memcpy(&xr[q][1], &v1, 16);
        }
    };
    auto st_dy = [&](int buf) {
        f16x8 hi, lo;
        split8h(dr[0], dr[1], asc, hi, lo);
        *reinterpret_cast<f16x8*>(Dy + buf * DROW + dls) = hi;
        *reinterpret_cast<f16x8*>(Dy + buf * DROW + WW_SW * 64 + dls) = lo;
    };
    auto st_xq = [&](int slot, int q) {
        if (q == 0 || xls[q] >= 0) {  // (unit 0 covers pixels 0..63 of the 66: always inside)
            f16x8 hi, lo;
            split8h(xr[q][0], xr[q][1], bsc, hi, lo);
            *reinterpret_cast<f16x8*>(Xr + slot * XROW + xls[q]) = hi;
            *reinterpret_cast<f16x8*>(Xr + slot * XROW + WW_WP * 64 + xls[q]) = lo;
        }
    };
    auto st_x = [&](int slot) {
#pragma unroll
        for (int q = 0; q < WW_XU; ++q) st_xq(slot, q);
    };
    // staging piece p (0: the dy row, 1 / 2: source units 0 / 1) of the row loaded for the next barrier
    auto st_piece = [&](int p, int y) {
        if (p == 0) st_dy((y + 1) & 1);
        else st_xq((y + 2) & 3, p - 1);
    };

    // transposed-read lane offsets (halves) of k-step 0 and the first sub-block: A (dy) at pixel row
    // 8 g + q (+ 4: the second read, same swizzle), channel 32 cob + 4 p; B (source) at pixel row
    // 8 g + q + tx, whose second read can carry into bit 3 (its own offset)
    const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
    int aoff, boff1[3], boff2[3];
    {
        const int r = 8 * g + q, c = 32 * cob + 4 * pp;
        aoff = r * 64 + 8 * ((c >> 3) ^ ww16_swz(r)) + (c & 7);
        const int cb = 32 * cib + 4 * pp;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            const int p1 = r + tx, p2 = r + 4 + tx;
            boff1[tx] = p1 * 64 + 8 * ((cb >> 3) ^ ww16_swz(p1)) + (cb & 7);
            boff2[tx] = p2 * 64 + 8 * ((cb >> 3) ^ ww16_swz(p2)) + (cb & 7);
        }
    }

    f32x4v acc[18], t[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) { acc[i] = f32x4v{0.f, 0.f, 0.f, 0.f}; t[i] = f32x4v{0.f, 0.f, 0.f, 0.f}; }

    // prologue: source rows y_beg - 1 .. y_beg + RPB into their ring slots, dy rows y_beg .. y_beg + RPB - 1;
    // every row's loads (and the exponents') in flight before the first store
    {
        float4 px_[RPB + 2][WW_XU][2], pd_[RPB][2];
#pragma unroll
        for (int i = 0; i < RPB + 2; ++i) {
            const int r = y_beg - 1 + i;
            ld_x(r <= H ? r : H);
#pragma unroll
            for (int u = 0; u < WW_XU; ++u) { px_[i][u][0] = xr[u][0]; px_[i][u][1] = xr[u][1]; }
        }
#pragma unroll
        for (int i = 0; i < RPB; ++i) {
            const int r = y_beg + i;
            ld_dy(r < y_end ? r : y_end - 1);
            pd_[i][0] = dr[0];
            pd_[i][1] = dr[1];
        }
        ea = f16x3_exp(rnga, a.rng_a_n);
        eb = f16x3_exp(rngb, a.rng_b_n);
        asc = __builtin_ldexpf(1.f, ea);
        bsc = __builtin_ldexpf(1.f, eb);
#pragma unroll
        for (int i = 0; i < RPB + 2; ++i) {
#pragma unroll
            for (int u = 0; u < WW_XU; ++u) { xr[u][0] = px_[i][u][0]; xr[u][1] = px_[i][u][1]; }
            st_x((y_beg - 1 + i) & (NXS - 1));
        }
#pragma unroll
        for (int i = 0; i < RPB; ++i) {
            dr[0] = pd_[i][0];
            dr[1] = pd_[i][1];
            st_dy((y_beg + i) & (NDB - 1));
        }
    }
    __syncthreads();

    // one row: two k-steps of 32 pixels; per k-step the A fragments of both co sub-blocks, then the
    // wave's five taps with the next tap's B fragments read ahead of the current one's MFMAs
    auto row = [&](int y, auto tag) {
        constexpr int R = decltype(tag)::value;
        const _Float16* const Db = Dy + (y & (NDB - 1)) * DROW;
        const _Float16* Xs[3];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) Xs[ty] = Xr + ((y + NXS - 1 + ty) & (NXS - 1)) * XROW;  // row y - 1 + ty
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 ah[2], al[2];
#pragma unroll
            for (int cs = 0; cs < 2; ++cs) {
                const int o = (aoff ^ (16 * cs)) + kk * 32 * 64;
                ah[cs] = ww16_frag(Db + o, Db + o + 4 * 64);
                al[cs] = ww16_frag(Db + WW_SW * 64 + o, Db + WW_SW * 64 + o + 4 * 64);
            }
            // (tap, ci sub-block) pairs of the wave: the next pair's B fragments read ahead of this one's MFMAs
            f16x8 bh[2], bl[2];
            auto rd_b = [&](int jp, int slot) {
                const int tt = jp >> 1, ns = jp & 1;
                const int tap = R == 0 ? tt : (tt < 4 ? 5 + tt : 4);
                const int ty = tap / 3, tx = tap % 3;
                const int o1 = (boff1[tx] ^ (16 * ns)) + kk * 32 * 64, o2 = (boff2[tx] ^ (16 * ns)) + kk * 32 * 64;
                bh[slot] = ww16_frag(Xs[ty] + o1, Xs[ty] + o2);
                bl[slot] = ww16_frag(Xs[ty] + WW_WP * 64 + o1, Xs[ty] + WW_WP * 64 + o2);
            };
            rd_b(0, 0);
#pragma unroll
            for (int jp = 0; jp < 10; ++jp) {
                if (jp < 9) rd_b(jp + 1, (jp + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
                // the three staging pieces inside the second k-step's pair iterations 1, 3, 5 (their split VALU
                // beside MFMAs instead of a block between the k-steps)
                if (kk == 1 && (jp == 1 || jp == 3 || jp == 5)) st_piece((jp - 1) >> 1, y);
                const int tt = jp >> 1, ns = jp & 1;
                const int tap = R == 0 ? tt : (tt < 4 ? 5 + tt : 4);
                const int sl = jp & 1;
#pragma unroll
                for (int cs = 0; cs < 2; ++cs) {
                    if (tap == 4 && cs != R) continue;  // tap 4: co sub-block R only
                    const int idx = tap == 4 ? 16 + ns : (R == 0 ? tap : tap - 5) * 4 + cs * 2 + ns;
                    t[idx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[cs], bh[sl], t[idx], 0, 0, 0);
                    t[idx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[cs], bl[sl], t[idx], 0, 0, 0);
                    t[idx] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[cs], bh[sl], t[idx], 0, 0, 0);
                }
            }
        }
    };

#pragma unroll 1
    for (int y = y_beg; y < y_end; ++y) {
        // the next row in flight (clamped past the chunk, reflected / zero past the image)
        ld_dy(y + 1 < y_end ? y + 1 : y);
        ld_x(y + 2 <= H ? y + 2 : H);
        if (half == 0) row(y, std::integral_constant<int, 0>{});
        else row(y, std::integral_constant<int, 1>{});
        if (((y - y_beg) & 1) == 1 || y + 1 == y_end) {  // chains of two rows (128 pixels)
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                acc[i] += t[i];
                asm volatile("" : "+v"(acc[i]));  // (pinned: see conv3_win16_kernel)
                t[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();
    }

    // epilogue: undo the operand scales, slab [split][co][tap * C + ci]; lane holds rows 4 g + r (co)
    // and column lane & 15 (ci) of each 16 x 16 sub-block
    const int eab = -(ea + eb);
    float* const slab = ws + (long long)split * Co * 9 * C;
#pragma unroll
    for (int i = 0; i < 18; ++i) {
        int tap, cs, ns;
        if (i >= 16) { tap = 4; cs = half; ns = i - 16; }
        else { tap = (half == 0 ? 0 : 5) + i / 4; cs = (i >> 1) & 1; ns = i & 1; }
        const int col = ci0 + 32 * cib + 16 * ns + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rowc = co0 + 32 * cob + 16 * cs + 4 * g + r;
            slab[(long long)rowc * 9 * C + tap * C + col] = __builtin_ldexpf(acc[i][r], eab);
        }
    }
}

// ---------------------------------------------------------------------------------------
// The one-pixel ring of the residual data gradient's padded grid (dcs_conv_dgrad_reflect_win).  Over the
// (H + 2) x (W + 2) grid dx_pad[q] = sum_t B_t^T dy[q + (ty - 2, tx - 2)] (B: the window kernel's flipped
// pack, dcs_pack_weights_h3), and a ring position is reached by the three taps of one kernel row (top
// ring row: ty = 2, bottom: ty = 0) or column (left: tx = 2, right: tx = 0) only.  One GEMM per ring
// segment and tap, so B is uniform over a workgroup: M = the segment's positions over the batch (the
// top rows of all images, ...), N = the output channels, K = C; the three taps' products go to three ring
// copies (RG_COPIES), summed by the fold in tap order, so each position's sum has one fixed order
// whatever the batch.  A workgroup owns 64 positions x 256 channels: four waves of 64 x 64 (4 x 4 blocks
// of v_mfma_f32_16x16x32_f16).  A (the gathered dy pixels, fp32) arrives by LDS-DMA (the eight 16-byte
// chunks of a row rotated by bits 1-3 of the row: conflict-free fragment reads) and is split into hi / lo
// fp16 at the fragment read, where pixels outside the image are masked to zero (their DMA reads pixel 0).
// B fragments come straight from the pack's tap-major copy (L2) into registers.  RG_D = 2 of the 8 k-steps
// (C = 256) are in flight, in RG_D + 1 LDS buffers and register sets (140 VGPRs: three waves per SIMD).  The B loads are inline asm like the DMA, so the compiler inserts no wait of its
// own for them (it cannot count the DMAs, and its waits for the registers would drain later k-steps'
// loads); the one wait per k-step (vmcnt: all but the loads of the k-steps after the next) covers both.
// The tap split triples the workgroups (more waves per SIMD to overlap the fetch latency of these short
// K loops).  The generic rows pass this replaces ran the ring as 128-row tiles with K split
// over up to eight ring copies.
constexpr int RG_NT = 256, RG_BM = 64;
constexpr int RG_D = 2;  // k-steps in flight (RG_D + 1 register sets and LDS buffers; 4 measured slower: 202 VGPRs)

template <int... I, class F>
__device__ __forceinline__ void rg_unroll(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

struct RingArgs {
    int N, H, W, C, Co;
    int tiles_tb, tiles_lr;  // 64-position tiles of the top / bottom segments and of the left / right ones
    int rng_n;
};

// 16 bytes per lane through the buffer descriptor, untracked by the compiler (see ring16_kernel)
__device__ __forceinline__ f16x8 rg_bload(__amdgpu_buffer_rsrc_t r, int off) {
    f16x8 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(r) : "memory");
    return v;
}

template <int NP, int NK>  // NK: k-steps (C / 32)
__global__ __launch_bounds__(RG_NT) void ring16_kernel(RingArgs a, const float* __restrict__ dy,
                                                      const _Float16* __restrict__ wh,
                                                      const _Float16* __restrict__ wl,
                                                      const float* __restrict__ rng,
                                                      const int* __restrict__ wexp, float* __restrict__ ring) {
    __shared__ __attribute__((aligned(16))) float Ar[(RG_D + 1) * RG_BM * 32];  // [buffer][row][32 floats]
    const int gco = a.Co >> 8;
    const int L = blockIdx.x;
    const int ct = L % gco, jt = (L / gco) % 3, mt = L / (3 * gco);
    const int n0 = ct * 256;
    int seg, tm;
    if (mt < 2 * a.tiles_tb) {
        seg = mt >= a.tiles_tb;
        tm = mt - seg * a.tiles_tb;
    } else {
        const int r = mt - 2 * a.tiles_tb;
        seg = 2 + (r >= a.tiles_lr);
        tm = r - (seg - 2) * a.tiles_lr;
    }
    const int H = a.H, W = a.W, C = a.C, Wp = W + 2, K = 9 * C;
    const int seglen = seg < 2 ? Wp : H;  // positions per image
    const int segM = a.N * seglen, m0 = tm * RG_BM;
    const int ringlen = 2 * Wp + 2 * H;
    // the workgroup's tap (t0 + jt tstep); dy pixel of a position at tap jt: (py0 + jt sy, px0 + jt sx)
    const int t0 = seg == 0 ? 6 : (seg == 2 ? 2 : 0), tstep = seg < 2 ? 1 : 3;
    const int sy = seg < 2 ? 0 : jt, sx = seg < 2 ? jt : 0;
    auto locate = [&](int m, int& n, int& py, int& px, int& ri) {
        n = m / seglen;
        const int p = m - n * seglen;
        if (seg == 0) { py = 0; px = p - 2; ri = p; }
        else if (seg == 1) { py = H - 1; px = p - 2; ri = Wp + p; }
        else if (seg == 2) { py = p - 1; px = 0; ri = 2 * Wp + 2 * p; }  // padded row p + 1
        else { py = p - 1; px = W - 1; ri = 2 * Wp + 2 * p + 1; }
        py += sy;
        px += sx;
    };
    auto inimg = [&](int py, int px) { return py >= 0 && py < H && px >= 0 && px < W; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int m16 = lane & 15, g = lane >> 4;

    // A by LDS-DMA: wave w's instructions i = 0, 1 move chunks u = (2 w + i) * 64 + lane: row u >> 3,
    // LDS slot u & 7 holding channel chunk (u & 7) ^ ((row >> 1) & 7) of the k-step's 32 channels
    unsigned doff[2], dlds[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int u = (2 * wid + i) * 64 + lane, row = u >> 3, chunk = (u & 7) ^ ((row >> 1) & 7);
        int n = 0, py = 0, px = 0, ri = 0;
        if (m0 + row < segM) locate(m0 + row, n, py, px, ri);
        const bool ok = m0 + row < segM && inimg(py, px);
        doff[i] = (unsigned)((ok ? ((n * H + py) * W + px) * C * 4 : 0) + chunk * 16);
        dlds[i] = (unsigned)__builtin_amdgcn_readfirstlane((2 * wid + i) * 64 * 16);
    }
    const unsigned ar_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)Ar;
    auto a_dma = [&](int ks, int buf) {
        const unsigned base = ar_lds + (unsigned)(buf * RG_BM * 32 * 4);
#pragma unroll
        for (int i = 0; i < 2; ++i) win_glds(dy, doff[i] + (unsigned)(ks * 128), base + dlds[i]);
    };
    // fragment rows 16 i + m16 inside the image at this tap (bit i)
    int vmask = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * i + m16;
        if (m < segM) {
            int n, py, px, ri;
            locate(m, n, py, px, ri);
            if (inimg(py, px)) vmask |= 1 << i;
        }
    }
    // B: lane (m16, g) of column block jb reads column n0 + 64 wid + 16 jb + m16, the k-step's channels
    // 8 g .. 8 g + 7 of the workgroup's tap, from the pack's tap-major copy (behind its Co x 9C planes:
    // the four lanes of a column read 64 contiguous bytes; the slice-major planes interleave the taps)
    const __amdgpu_buffer_rsrc_t bhr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(wh), (short)0, 0x7fffff00, 0x00020000);
    const __amdgpu_buffer_rsrc_t blr = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(NP == 3 ? wl : wh), (short)0, 0x7fffff00, 0x00020000);
    const int blane = (a.Co * K + (n0 + 64 * wid + m16) * K + (t0 + jt * tstep) * C + 8 * g) * 2;
    f16x8 bq[RG_D + 1][4][2];
    auto b_load = [&](int ks, auto setc) {
        constexpr int S = decltype(setc)::value;
        const int kb = blane + ks * 32 * 2;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            bq[S][jb][0] = rg_bload(bhr, kb + jb * 16 * K * 2);
            if constexpr (NP == 3) bq[S][jb][1] = rg_bload(blr, kb + jb * 16 * K * 2);
        }
    };

    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[i][jb] = f32x4v{0.f, 0.f, 0.f, 0.f};

    // vmcnt(n) with the other counters left alone
    auto wait_vm = [](auto nc) {
        constexpr int n = decltype(nc)::value;
        __builtin_amdgcn_s_waitcnt(0x0F70 | (n & 15) | ((n >> 4) << 14));
    };
    constexpr int PER = NP == 3 ? 10 : 6;  // loads per k-step and lane: 2 DMA + 4 or 8 B

    // prologue: the exponents first (their loads are the compiler's to wait for), then k-steps
    // 0 .. RG_D - 1 in flight, k-step 0 waited for
    const int ea = f16x3_exp(rng, a.rng_n);
    const int eb = __builtin_amdgcn_readfirstlane(wexp[0]);
    const float asc = __builtin_ldexpf(1.f, ea);
    __builtin_amdgcn_sched_barrier(0);
    rg_unroll(std::make_integer_sequence<int, (RG_D < NK ? RG_D : NK)>{}, [&](auto kc) {
        constexpr int k = decltype(kc)::value;
        a_dma(k, k);
        b_load(k, std::integral_constant<int, k>{});
    });
    wait_vm(std::integral_constant<int, ((RG_D < NK ? RG_D : NK) - 1) * PER>{});
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);

    // per lane: A rows 16 i + m16, floats 8 g .. 8 g + 7 = chunks 2 g, 2 g + 1
    int aoff[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 16 * i + m16, f = (row >> 1) & 7;
        aoff[i][0] = row * 32 + 4 * ((2 * g) ^ f);
        aoff[i][1] = row * 32 + 4 * ((2 * g + 1) ^ f);
    }
    auto step = [&](auto ksc) {
        constexpr int ks = decltype(ksc)::value, S = ks % (RG_D + 1);
        // no load past the end (its dead destination registers the compiler would hand to other values)
        if constexpr (ks + RG_D < NK) {
            a_dma(ks + RG_D, (ks + RG_D) % (RG_D + 1));
            b_load(ks + RG_D, std::integral_constant<int, (ks + RG_D) % (RG_D + 1)>{});
        }
        __builtin_amdgcn_sched_barrier(0);
        const float* const Ab = Ar + S * RG_BM * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 r0 = *reinterpret_cast<const float4*>(Ab + aoff[i][0]);
            const float4 r1 = *reinterpret_cast<const float4*>(Ab + aoff[i][1]);
            const float sc = (vmask >> i) & 1 ? asc : 0.f;  // pixels outside the image: zero
            f16x8 ah, al;
            split8h(r0, r1, sc, ah, al);
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                if constexpr (NP == 3) {
                    acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bq[S][jb][0], acc[i][jb], 0, 0, 0);
                    acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bq[S][jb][1], acc[i][jb], 0, 0, 0);
                }
                acc[i][jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bq[S][jb][0], acc[i][jb], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // k-step ks + 1 has landed once only the loads of the k-steps after it are in flight
        constexpr int last = ks + RG_D < NK - 1 ? ks + RG_D : NK - 1;
        wait_vm(std::integral_constant<int, (last > ks + 1 ? last - ks - 1 : 0) * PER>{});
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    };
    // fully unrolled (NK = C / 32 k-steps): the registers the asm loads fill must not meet a control-flow
    // merge, where the compiler could copy them before the data lands
    rg_unroll(std::make_integer_sequence<int, NK>{}, step);

    // epilogue: undo the scales into ring copy jt; lane (m16, g) holds rows 16 i + 4 g + r, column
    // 16 jb + m16
    const int eab = -(ea + eb);
    float* const rc = ring + (long long)jt * a.N * ringlen * a.Co;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * i + 4 * g + r;
            if (m >= segM) continue;
            int n, py, px, ri;
            locate(m, n, py, px, ri);
            float* const o = rc + ((long long)n * ringlen + ri) * a.Co + n0 + 64 * wid + m16;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) o[16 * jb] = __builtin_ldexpf(acc[i][jb][r], eab);
        }
}

struct WWPlan {
    int strips, rchunks, rows_per, nsplit;
};
WWPlan ww_plan(const dcs_conv_desc& d) {
    WWPlan p;
    p.strips = d.Ws / WW_SW;
    const long long base = (long long)d.N * p.strips * (d.Co / 64) * (d.Cs / 64);
    int rch = (int)cdiv(256, base);  // at least one workgroup per CU
    const int maxch = d.Hs / 8 > 0 ? d.Hs / 8 : 1;  // >= 8 rows per chunk
    rch = rch < 1 ? 1 : (rch > maxch ? maxch : rch);
    p.rows_per = (int)cdiv(d.Hs, rch);
    p.rchunks = (int)cdiv(d.Hs, p.rows_per);
    p.nsplit = d.N * p.strips * p.rchunks;
    return p;
}

}  // namespace

// d describes the FORWARD conv (source x, output dy)
bool wgrad_win_check(const dcs_conv_desc& d) {
    return (d.mma == DCS_MMA_F16X3 || d.mma == DCS_MMA_F16) && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.up == 1 &&
           d.parity == 0 &&
           d.pt == 1 && d.pl == 1 && d.Ho == d.Hs && d.Wo == d.Ws && d.Cs % 64 == 0 && d.Co % 64 == 0 &&
           d.Ws % WW_SW == 0 && d.Hs >= 2 && d.s_c == 1 && d.s_w == d.Cs && d.s_h == (long long)d.Ws * d.Cs &&
           d.s_n == (long long)d.Hs * d.Ws * d.Cs && d.csplit == d.Cs && (d.cw == 0 || d.cw == d.Cs) &&
           d.pro_act == DCS_ACT_NONE && d.rng_a && d.rng_b && d.rng_a_n > 0 && d.rng_a_n <= 1024 &&
           d.rng_b_n > 0 && d.rng_b_n <= 1024 && (long long)d.N * d.Hs * d.Ws * d.Cs * 4 < 0x7fffff00LL - 64 &&
           (long long)d.N * d.Hs * d.Ws * d.Co * 4 < 0x7fffff00LL - 64;
}

size_t wgrad_win_workspace_size(const dcs_conv_desc& d) {
    const WWPlan p = ww_plan(d);
    return (size_t)p.nsplit * d.Co * 9 * d.Cs * sizeof(float);
}

// partial slabs into ws (wgrad_win_workspace_size bytes); returns the split count (< 0: error)
int wgrad_win_launch(const dcs_conv_desc& d, const float* dy, const float* x, float* ws, hipStream_t s) {
    const WWPlan p = ww_plan(d);
    WWArgs a;
    a.N = d.N; a.H = d.Hs; a.W = d.Ws; a.C = d.Cs; a.Co = d.Co;
    a.reflect = d.pad_mode == DCS_PAD_REFLECT;
    a.strips = p.strips; a.rchunks = p.rchunks; a.rows_per = p.rows_per;
    a.gco = d.Co / 64; a.gci = d.Cs / 64;
    a.rng_a_n = d.rng_a_n; a.rng_b_n = d.rng_b_n;
    const unsigned blocks = (unsigned)((long long)p.nsplit * a.gco * a.gci);
    if (d.mma == DCS_MMA_F16)
        hipLaunchKernelGGL(wgrad3_win_h3_kernel<1>, dim3(blocks), dim3(WW_NT), 0, s, a, dy, x, d.rng_a, d.rng_b, ws);
    else
        hipLaunchKernelGGL(wgrad3_win16_kernel<3>, dim3(blocks), dim3(WW_NT), 0, s, a, dy, x, d.rng_a, d.rng_b, ws);
    const int e = check_launch("wgrad3_win");
    return e ? -e : p.nsplit;
}

namespace {

// the padded-grid ring on ring16_kernel (d: the data gradient's descriptor): RG_COPIES ring copies (one
// per tap)
bool ring16_ok(const dcs_conv_desc& d) {
    return d.Cs == 256 && d.Co % 256 == 0 && d.Hs >= 2 && d.Ws >= 2;
}

// the one place that decides whether the window kernels take a descriptor (dcs_conv3_win_ok): forward,
// conv3_win16_kernel; data gradient, conv3_win16_kernel for the interior and ring16_kernel for the ring
int win_check(const dcs_conv_desc& d, bool fwd) {
    const bool geom = d.KH == 3 && d.KW == 3 && d.stride == 1 && d.up == 1 && !d.parity && d.Cs % 32 == 0 &&
                      d.Co % WIN_BN == 0 && d.Ws >= 16 && d.Ws <= 128 && 256 % d.Ws == 0 && d.Hs % (256 / d.Ws) == 0 &&
                      d.s_c == 1 && d.s_w == d.Cs && d.s_h == (long long)d.Ws * d.Cs &&
                      d.s_n == (long long)d.Hs * d.Ws * d.Cs && d.csplit == d.Cs &&
                      d.epi_act == DCS_ACT_NONE && (d.mma == DCS_MMA_F16X3 || d.mma == DCS_MMA_F16) && d.rng_a && d.rng_a_n > 0 &&
                      d.rng_a_n <= 1024 && (long long)d.N * d.Hs * d.Ws * d.Cs * 4 < 0x7fffff00LL &&
                      d.pro_act == DCS_ACT_NONE;
    if (!geom) return 0;
    if (fwd) return d.Ho == d.Hs && d.Wo == d.Ws && d.pt == 1 && d.pl == 1;
    return d.Ho == d.Hs + 2 && d.Wo == d.Ws + 2 && d.pt == 2 && d.pl == 2 && d.pad_mode == DCS_PAD_ZERO &&
           ring16_ok(d);
}

int launch_win(const dcs_conv_desc& d, int H, int W, int reflect, const float* src, const void* wh, const void* wl,
               const int* wexp, const float* addend, float* out, Part* parts, hipStream_t s,
               const IbwArgs* ibw = nullptr) {
    WinArgs a;
    a.N = d.N; a.H = H; a.W = W; a.C = d.Cs; a.Co = d.Co; a.reflect = reflect;
    a.R = 256 / W; a.tiles = H / a.R; a.gy = d.Co / WIN_BN; a.rng_n = d.rng_a_n;
    const unsigned blocks = (unsigned)(a.N * a.tiles * a.gy);
    const IbwArgs ib = ibw ? *ibw : IbwArgs{nullptr, nullptr, nullptr, nullptr, 0, 0};
    const _Float16* h = reinterpret_cast<const _Float16*>(wh);
    const _Float16* l = reinterpret_cast<const _Float16*>(wl);
#define DCS_WIN16_LAUNCH(IBW_, WIDE_)                                                                              \
    if (d.mma == DCS_MMA_F16X3)                                                                                \
        hipLaunchKernelGGL((conv3_win16_kernel<3, IBW_, WIDE_>), dim3(blocks), dim3(WIN_NT), 0, s, a, src, h, l,   \
                           d.rng_a, wexp, addend, out, parts, ib);                                                 \
    else                                                                                                        \
        hipLaunchKernelGGL((conv3_win16_kernel<1, IBW_, WIDE_>), dim3(blocks), dim3(WIN_NT), 0, s, a, src, h, l,   \
                           d.rng_a, wexp, addend, out, parts, ib);
    if (W >= 64) {
        if (ibw) { DCS_WIN16_LAUNCH(true, true) } else { DCS_WIN16_LAUNCH(false, true) }
    } else {
        if (ibw) { DCS_WIN16_LAUNCH(true, false) } else { DCS_WIN16_LAUNCH(false, false) }
    }
#undef DCS_WIN16_LAUNCH
    return check_launch("conv3_win16");
}

int launch_ring16(const dcs_conv_desc& d, const float* dy, const void* wh, const void* wl, const int* wexp, float* ring,
                  hipStream_t s) {
    RingArgs a;
    a.N = d.N; a.H = d.Hs; a.W = d.Ws; a.C = d.Cs; a.Co = d.Co; a.rng_n = d.rng_a_n;
    a.tiles_tb = (int)cdiv((long long)d.N * (d.Ws + 2), RG_BM);
    a.tiles_lr = (int)cdiv((long long)d.N * d.Hs, RG_BM);
    const unsigned blocks = (unsigned)((2 * a.tiles_tb + 2 * a.tiles_lr) * 3 * (d.Co / 256));
    const _Float16* h = reinterpret_cast<const _Float16*>(wh);
    const _Float16* l = reinterpret_cast<const _Float16*>(wl);
    if (d.mma == DCS_MMA_F16)
        hipLaunchKernelGGL((ring16_kernel<1, 8>), dim3(blocks), dim3(RG_NT), 0, s, a, dy, h, l, d.rng_a, wexp, ring);
    else
        hipLaunchKernelGGL((ring16_kernel<3, 8>), dim3(blocks), dim3(RG_NT), 0, s, a, dy, h, l, d.rng_a, wexp, ring);
    return check_launch("ring16");
}

}  // namespace

// conv.hip: the ring fold
int reflect_ring_fold(const float* ring, float* dx, int N, int H, int W, int C, int nsplit, hipStream_t s);
int reflect_ring_fold_ibw(const float* ring, float* dx, int N, int H, int W, int C, int nsplit, const float* y,
                          const float* sc, const float* sh, int act, Sum2* parts, int nchunk, int chunk0, int nfc,
                          hipStream_t s);
constexpr int IBW_FOLD_CHUNKS = 64;  // partial-sum chunks of the ring fold per image (its blocks: 64 per image)

}  // namespace dcs

using namespace dcs;

extern "C" size_t dcs_pack_weights_h3_scratch_size(void) { return DCS_RANGE_PARTS * sizeof(float); }

extern "C" int dcs_pack_weights_h3(const float* w, int Cout, int Cin, int flip, int ncols, void* out_hi, void* out_lo,
                                   float* scratch, int* wexp, void* stream) {
    if (!w || !out_hi || !out_lo || !scratch || !wexp || Cout <= 0 || Cin <= 0 || ncols <= 0 ||
        (flip ? Cout : Cin) % 16 != 0 || ncols < (flip ? Cin : Cout))
        return fail(DCS_E_INVALID, "pack_weights_h3: bad arguments (3x3, reduction channels % 16 == 0)");
    hipStream_t s = as_stream(stream);
    const long long nw = (long long)Cout * Cin * 9;
    const long long rb = cdiv(nw, 2048) < DCS_RANGE_PARTS ? cdiv(nw, 2048) : DCS_RANGE_PARTS;  // ~8 weights per thread
    hipLaunchKernelGGL(wrange_kernel, dim3((unsigned)(rb < 1 ? 1 : rb)), dim3(256), 0, s, w, nw, scratch);
    int e = check_launch("pack_weights_h3 range");
    if (e) return e;
    const long long pb = cdiv((long long)ncols * 9 * (flip ? Cout : Cin), 2048);
    hipLaunchKernelGGL(pack_h3_kernel, dim3((unsigned)(pb < 1 ? 1 : (pb > 256 ? 256 : pb))), dim3(256), 0, s, w, Cout, Cin, flip, ncols, scratch,
                       (int)DCS_RANGE_PARTS, reinterpret_cast<_Float16*>(out_hi), reinterpret_cast<_Float16*>(out_lo),
                       wexp);
    return check_launch("pack_weights_h3");
}


extern "C" int dcs_conv3_win_ok(const dcs_conv_desc* dp, int dgrad) { return dp ? win_check(*dp, !dgrad) : 0; }

extern "C" int dcs_conv3_win_in_stats(const dcs_conv_desc* dp, const float* src, const void* w_hi, const void* w_lo,
                                      const int* wexp, float* out, void* parts, size_t parts_bytes, int* nchunk,
                                      void* stream) {
    if (!dp || !src || !w_hi || !w_lo || !wexp || !out) return fail(DCS_E_INVALID, "conv3_win: null pointer");
    const dcs_conv_desc& d = *dp;
    if (!win_check(d, true))
        return fail(DCS_E_INVALID, "conv3_win: needs a 3x3 stride-1 'same' f16x3 conv over contiguous NHWC rows "
                                   "(16 <= W <= 128, 256 % W == 0, H % (256 / W) == 0, Cs % 32 == 0, Co % 128 == 0, "
                                   "no prologue)");
    const int tiles = d.Hs / (256 / d.Ws);
    if (parts) {
        if (!nchunk || parts_bytes < (size_t)d.N * tiles * d.Co * sizeof(Part))
            return fail(DCS_E_WORKSPACE, "conv3_win: parts buffer too small");
        *nchunk = tiles;
    }
    return launch_win(d, d.Hs, d.Ws, d.pad_mode == DCS_PAD_REFLECT, src, w_hi, w_lo, wexp, nullptr, out,
                      reinterpret_cast<Part*>(parts), as_stream(stream));
}

extern "C" int dcs_conv_dgrad_reflect_win(const dcs_conv_desc* dp, const float* dy, const float* wpack,
                                          const void* w_hi, const void* w_lo, const int* wexp, const float* addend,
                                          float* dx, float* ring, void* stream) {
    (void)wpack;  // unused by the window route
    if (!dp || !dy || !w_hi || !w_lo || !wexp || !dx || !ring)
        return fail(DCS_E_INVALID, "conv_dgrad_reflect_win: null pointer");
    const dcs_conv_desc& d = *dp;
    if (!win_check(d, false) || d.Co % 4 != 0 || d.Hs < 4 || d.Ws < 4)
        return fail(DCS_E_INVALID, "conv_dgrad_reflect_win: the padded-grid data gradient of a 3x3 reflect-pad-1 conv "
                                   "(dcs_conv_dgrad_reflect's descriptor) with an f16x3 window geometry expected");
    hipStream_t s = as_stream(stream);
    // interior: a 'same' zero-pad conv of dy over the flipped weights, straight into dx (+ addend)
    int e = launch_win(d, d.Hs, d.Ws, 0, dy, w_hi, w_lo, wexp, addend, dx, nullptr, s);
    if (e) return e;
    // the padded grid's one-pixel ring (ring16_kernel), folded onto the border
    if ((e = launch_ring16(d, dy, w_hi, w_lo, wexp, ring, s))) return e;
    return reflect_ring_fold(ring, dx, d.N, d.Ho - 2, d.Wo - 2, d.Co, RG_COPIES, s);
}

extern "C" size_t dcs_conv_dgrad_reflect_win_inbwd_parts_size(const dcs_conv_desc* dp) {
    if (!dp || dp->Ws <= 0 || 256 % dp->Ws) return 0;
    const int H = dp->Ho - 2, W = dp->Wo - 2;
    if (H <= 0 || W <= 0 || (long long)H * W % 256) return 0;
    return (size_t)dp->N * (H * W / 256 + IBW_FOLD_CHUNKS) * dp->Co * sizeof(Sum2);
}

extern "C" int dcs_conv_dgrad_reflect_win_inbwd(const dcs_conv_desc* dp, const float* dy, const float* wpack,
                                                const void* w_hi, const void* w_lo, const int* wexp, float* dx,
                                                float* ring, const float* y, const float* scale, const float* shift,
                                                int act, void* parts, size_t parts_bytes, int* nchunk, void* stream) {
    (void)wpack;  // unused by the window route
    if (!dp || !dy || !w_hi || !w_lo || !wexp || !dx || !ring || !y || !scale || !shift || !parts || !nchunk)
        return fail(DCS_E_INVALID, "conv_dgrad_reflect_win_inbwd: null pointer");
    const dcs_conv_desc& d = *dp;
    if (!win_check(d, false) || d.Co % 4 != 0 || 256 % (d.Co / 4) || d.Hs < 4 || d.Ws < 4)
        return fail(DCS_E_INVALID, "conv_dgrad_reflect_win_inbwd: a dcs_conv_dgrad_reflect_win geometry with Co / 4 "
                                   "dividing 256 expected");
    if (act != DCS_ACT_AFFINE && act != DCS_ACT_RELU && act != DCS_ACT_LRELU)
        return fail(DCS_E_INVALID, "conv_dgrad_reflect_win_inbwd: act must be DCS_ACT_AFFINE / _RELU / _LRELU");
    if (parts_bytes < dcs_conv_dgrad_reflect_win_inbwd_parts_size(dp))
        return fail(DCS_E_WORKSPACE, "conv_dgrad_reflect_win_inbwd: parts buffer too small");
    hipStream_t s = as_stream(stream);
    const int tiles = d.Hs * d.Ws / 256;
    const int nch = tiles + IBW_FOLD_CHUNKS;
    const IbwArgs ib{y, scale, shift, reinterpret_cast<Sum2*>(parts), act, nch};
    int e = launch_win(d, d.Hs, d.Ws, 0, dy, w_hi, w_lo, wexp, nullptr, dx, nullptr, s, &ib);
    if (e) return e;
    if ((e = launch_ring16(d, dy, w_hi, w_lo, wexp, ring, s))) return e;
    *nchunk = nch;
    return reflect_ring_fold_ibw(ring, dx, d.N, d.Hs, d.Ws, d.Co, RG_COPIES, y, scale, shift, act,
                                 reinterpret_cast<Sum2*>(parts), nch, tiles, IBW_FOLD_CHUNKS, s);
}
