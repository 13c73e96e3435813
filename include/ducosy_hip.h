/*
 * ducosy_hip.h — C-ABI of the MI355X (gfx950) kernel library behind the DuCoSy-GAN
 * CycleGAN training hot path.
 *
 * The reference has no FFI: its de-facto operator boundary is the Python nn.Module /
 * loss-module API of modules/model.py and modules/trainer.py, which reach ATen/cuDNN
 * kernels through torch.nn.  Every entry point below replaces one such group of ATen
 * calls (cited per function, paths relative to the reference repo).  The host side
 * (ducosy-gan_amd/modules/hip/ Python modules) binds them with ctypes.
 *
 * Conventions
 *   - Plain device pointers + int sizes; no torch types.  Activations are NHWC fp32
 *     (channels innermost); single-channel planes are NCHW == NHWC.
 *   - The caller owns every buffer (including workspaces, sized by *_workspace_size).
 *     The library never allocates or frees device memory and never synchronises.
 *   - Every call is enqueued on `stream` (a hipStream_t passed as void*).
 *   - Every call returns 0 on success, a DCS_E_* code on an invalid argument, or the
 *     hipError_t of a failed launch; dcs_last_error() returns a thread-local message.
 */
#ifndef DUCOSY_HIP_H
#define DUCOSY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCS_OK 0
#define DCS_E_INVALID 1001
#define DCS_E_WORKSPACE 1002

#define DCS_PAD_ZERO 0
#define DCS_PAD_REFLECT 1

/* per-channel prologue transform applied to gathered source values:
 * v -> act(v * scale[n,c] + shift[n,c]); padding stays zero (or mirrors transformed values) */
#define DCS_ACT_NONE 0     /* no transform at all */
#define DCS_ACT_AFFINE 1   /* affine only (InstanceNorm apply) */
#define DCS_ACT_RELU 2     /* affine + ReLU                    */
#define DCS_ACT_LRELU 3    /* affine + LeakyReLU(0.2)          */
#define DCS_ACT_TANH 4     /* epilogue only                    */

/*
 * Geometry of one implicit-GEMM convolution pass.
 *   source  : the tensor gathered into the GEMM reduction (forward: x, dgrad: dy)
 *   output  : NHWC [N, Ho, Wo, Co]
 * Regular rows (parity = 0): output pixel (oy, ox) reads virtual source coordinate
 *   (oy*stride + ty - pt, ox*stride + tx - pl) for tap (ty, tx); the virtual source is
 *   the source upsampled (nearest) by `up`, padded by pad_mode.
 * Parity rows (parity = 1): stride-2 transposed convolution (dgrad of a stride-2
 *   forward conv with kernel KH x KW and padding pt/pl): output pixel (2qy+ry, 2qx+rx)
 *   reads dy at (qy + (ry+pt-ty)/2, qx + (rx+pl-tx)/2) for the taps of its parity class.
 */
typedef struct dcs_conv_desc {
    int32_t N;
    int32_t Hs, Ws, Cs;             /* source dims (Cs = reduction channels per tap)      */
    int64_t s_n, s_c, s_h, s_w;     /* source element strides                             */
    int32_t csplit;                 /* channels >= csplit come from src2 (concat fusion)  */
    int32_t cw;                     /* weight input channels if < Cs (zero-padded source  */
                                    /* channels, e.g. the 3-channel stem packed to 4); 0 = Cs */
    int64_t s2_n, s2_c, s2_h, s2_w; /* src2 strides (channel index relative to csplit)   */
    int32_t up;                     /* nearest-upsample factor of the source (1 or 2)     */
    int32_t pad_mode;               /* DCS_PAD_ZERO / DCS_PAD_REFLECT                     */
    int32_t KH, KW, pt, pl;         /* kernel, top/left padding                           */
    int32_t stride;                 /* forward stride (1 or 2)                            */
    int32_t parity;                 /* 0 regular rows, 1 stride-2 transposed parity rows  */
    int32_t Ho, Wo, Co;             /* output dims                                        */
    int32_t ldb;                    /* packed weights: Kpad (rows pass) / ncols (narrow)  */
    int32_t pro_act;                /* DCS_ACT_* prologue on the source                   */
    int32_t epi_act;                /* DCS_ACT_NONE / DCS_ACT_TANH / DCS_ACT_LRELU        */
    int32_t mma;                    /* MFMA operands: DCS_MMA_F32 (exact; 0 = zeroed desc) */
                                    /* or DCS_MMA_BF16 / _BF16X3 / _BF16X6 (f32 accum.)   */
    int32_t korder;                 /* GEMM K order of the rows pass (and of its packed    */
                                    /* weights): DCS_KORDER_TAP (tap-major) or            */
                                    /* DCS_KORDER_SLICE (16-channel slices, taps inside)  */
    int32_t rng_a_n, rng_b_n;       /* DCS_MMA_F16X3: counts of the partial maxima below   */
    const float* rng_a;             /* F16X3: partial maxima of |gathered operand| (rows:  */
                                    /* the source after its prologue; wgrad: dy), their   */
                                    /* max an upper bound of every value (dcs_range_parts) */
    const float* rng_b;             /* F16X3: the same for the other operand (rows: the   */
                                    /* packed weights, dcs_pack_weights_r; wgrad: source) */
    const void* b_h3;               /* F16X3 / F16 rows pass, optional: the packed weights */
                                    /* pre-split by dcs_pack_split_h3 (B staged without a */
                                    /* split); NULL: split at staging                     */
} dcs_conv_desc;

/* K order of the rows pass.  TAP: k = tap * Cs + c.  SLICE: k = (c / 16) * taps * 16 + tap * 16 +
 * c % 16 — every tap of a 16-channel slice before the next slice, so the gathered source rows
 * of a slice are re-read from L2 / L1 by the next taps instead of after a whole tap sweep
 * (regular stride-1 rows, Cs % 16 == 0; pack the weights with DCS_PACK_KSLICE). */
#define DCS_KORDER_TAP 0
#define DCS_KORDER_SLICE 1
#define DCS_PACK_KSLICE 8

/* MFMA operand modes of the MFMA convolution passes (dcs_conv_desc.mma).  F32 is exact fp32
 * (the reference's precision).  BF16 rounds both GEMM operands to bf16 (BASELINE config 5's
 * half-precision path).  BF16X3 splits each operand into hi + lo bf16 and sums three
 * products (~2^-16 relative error per product).  Shapes without a bf16 variant run F32. */
#define DCS_MMA_F32 0
#define DCS_MMA_BF16 1
#define DCS_MMA_BF16X3 3
/* BF16X6: three-way split (hi + mid + lo bf16), six products, ~2^-24 relative error per
 * product (fp32-class); 128-column tiles only, other shapes run F32. */
#define DCS_MMA_BF16X6 6
/* F16X3: each fp32 operand, scaled by a power of two 2^s (max|operand| * 2^s < 2^15, from the
 * descriptor's rng_a / rng_b partial maxima), is split into hi + lo fp16 (22 significant bits:
 * |v - hi - lo| <= 2^-22 |v|); three products hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16,
 * fp32 two-level accumulation, the result scaled back by 2^-(s_a + s_b) (exact).  Measured
 * error against float64 at or below the exact-f32 path's on every layer geometry
 * (tests/test_gpu_mma.py): fp32-class at half the MFMAs of BF16X6.  Shapes without an F16X3
 * variant run BF16X6. */
#define DCS_MMA_F16X3 7
/* F16: BASELINE config 5's fp16 MFMA path.  Each fp32 operand, scaled by the same power of two as
 * F16X3 (from rng_a / rng_b), is rounded to fp16 (11 significant bits, no overflow or underflow
 * from the scale); one product per fragment pair on v_mfma_f32_32x32x16_f16, fp32 accumulation and
 * storage, the result scaled back exactly.  Shapes without an F16 variant run BF16X6. */
#define DCS_MMA_F16 8
/* partial maxima the F16X3 kernels reduce (dcs_range_parts writes this many).  The producers of
 * conv operands (dcs_in_apply, dcs_in_act_backward, dcs_cbam_forward, dcs_cbam_backward,
 * dcs_act_backward, dcs_pack_nhwc4) take an optional `rng` (DCS_RANGE_PARTS floats, or NULL):
 * they zero it and fold the max |value| they write into it, so an F16X3 pass over their output
 * needs no separate dcs_range_parts read. */
#define DCS_RANGE_PARTS 512

const char* dcs_last_error(void);
int dcs_version(void);


/* ---- convolution family (modules/model.py:61-63,74-79,94-112,122-129 → aten conv) ---- */

/* Pack OIHW weights into the GEMM B operand, logically [Kpad][ncols] (zero padded), stored
 * N-major ([ncols][Kpad]; nmajor=1, for dcs_conv_rows, ldb = Kpad) or K-major ([Kpad][ncols];
 * nmajor=0, for the narrow kernels, ldb = ncols).
 * kind 0 forward   : B[(ty*KW+tx)*Cin + ci][co] = W[co][ci][ty][tx]
 * kind 1 dgrad-flip: B[(ty*KW+tx)*Cout + co][ci] = W[co][ci][KH-1-ty][KW-1-tx]  (stride-1 dgrad)
 * kind 2 dgrad     : B[(ty*KW+tx)*Cout + co][ci] = W[co][ci][ty][tx]              (stride-2 dgrad)
 * kind 3 / 4      : sub-pixel forward / data gradient of nearest-x2 upsample + 3x3 conv
 * kind 5 fwd-pad  : B[(ty*KW+tx)*ci_count + ci][co] = ci < Cin ? W[co][ci][ty][tx] : 0
 *                   (forward over a source whose channels are zero-padded to ci_count)
 * kind | DCS_PACK_KSLICE (kinds 0 and 1): the same B with its K rows in DCS_KORDER_SLICE order
 * ci_count limits the packed input channels (dgrad of a concat input needs only the first). */
int dcs_pack_weights(const float* w, int Cout, int Cin, int KH, int KW, int kind, int ci_count,
                     int Kpad, int ncols, int nmajor, float* out, void* stream);
/* The same, and DCS_RANGE_PARTS partial maxima of |packed value| into rng (the rng_b of an
 * F16X3 rows pass over these weights). */
int dcs_pack_weights_r(const float* w, int Cout, int Cin, int KH, int KW, int kind, int ci_count,
                       int Kpad, int ncols, int nmajor, float* out, float* rng, void* stream);

/* Fused G-step loss planes (the north star's fused cycle / identity / SSIM / gradient /
 * contrast-loss kernel; replaces the per-term calls of modules/trainer.py:469-512).  One job per
 * (pred, target) plane set of n_img single-channel H x W planes; flags select its terms:
 *   DCS_GL_L1 nn.L1Loss, DCS_GL_GRAD GradientLoss (trainer.py:22-40), DCS_GL_SSIM
 *   pytorch_msssim.SSIM (11-tap sigma 1.5 valid gaussian, size_average), DCS_GL_CA
 *   ContrastAttentionLoss with a 7x7 box (trainer.py:43-86; needs source), DCS_GL_MSEC
 *   nn.MSELoss against the constant t_const (target unused).
 * grad (optional) receives c_l1 d(L1)/dpred + c_grad d(Grad)/dpred + c_ssim d(SSIM)/dpred +
 * c_ca d(CA)/dpred + c_mse d(MSE)/dpred + c_add0 add0 + c_add1 add1 in one write per pixel
 * (add0 / add1: optional planes of the same shape, e.g. the batch-coupled terms' gradients).
 * Term values (means) val[5 j + q], q = 0 L1, 1 gradient-loss x part, 2 y part, 3 SSIM, 4 CA or
 * MSE, are composed into out[o] = bias[o] + sum_k coef[o * 5 njobs + k] val[k]
 *                                 + sum_x coefx[o * 4 + x] extra[x][0]  (o < nout <= 12)
 * (extra: up to 4 device scalars, NULL entries skipped).  Two launches; deterministic. */
#define DCS_GL_L1 1
#define DCS_GL_GRAD 2
#define DCS_GL_SSIM 4
#define DCS_GL_CA 8
#define DCS_GL_MSEC 16
typedef struct dcs_gl_job {
    const float* pred;
    const float* target;
    const float* source;
    const float* add0;
    const float* add1;
    float* grad;
    int32_t n_img, H, W, flags;
    float c_l1, c_grad, c_ssim, c_ca, c_mse, t_const, c_add0, c_add1;
} dcs_gl_job;
size_t dcs_gen_loss_fused_ws(const dcs_gl_job* jobs, int njobs);
int dcs_gen_loss_fused(const dcs_gl_job* jobs, int njobs, float ssim_data_range, float ca_sigma, float ca_min_w,
                       float ca_max_w, const float* bias, const float* coef, const float* coefx,
                       const float* const* extra, int nout, float* out, void* ws, size_t ws_bytes, void* stream);

/* Range-record arena: records (DCS_RANGE_PARTS floats each) inside [base, base + bytes) are zeroed
 * by the caller, in bulk, before each reuse of the arena; the producers that fold a record's maxima
 * then skip their own per-record memset.  Host-side registry of the calling process. */
int dcs_range_arena_register(const void* base, size_t bytes);
int dcs_range_arena_unregister(const void* base);

/* Partial maxima of |act(x * scale[n][c] + shift[n][c])| (or |x| when act == DCS_ACT_NONE and
 * scale == NULL) over an NHWC tensor of n_img images of `per_img` elements, C channels
 * innermost: DCS_RANGE_PARTS floats into parts, whose max bounds every value (the rng_a / rng_b
 * of an F16X3 pass).  per_img % 4 == 0, C % 4 == 0 with a prologue. */
int dcs_range_parts(const float* x, int n_img, int64_t per_img, int C, const float* scale,
                    const float* shift, int act, float* parts, void* stream);

/* ---- f16x3 window convolution: the residual-block 3x3 convs (modules/model.py:72-80) ----
 * A workgroup owns 256 consecutive pixels of one image (256 / W whole rows) x 128 output channels
 * and stages the (rows + 2) x (W + 2) source window once per 16-channel slice, split into hi / lo
 * fp16; the nine taps read MFMA fragments from it at a per-tap offset (csrc/conv_win.hip).
 *
 * dcs_pack_weights_h3: pre-split weights of a 3x3 conv, hi / lo fp16 planes [ncols][9 * C] in the
 * slice-major K order (k = (c / 16) * 144 + tap * 16 + c % 16), C = Cin for the forward (flip = 0) or
 * Cout for the data gradient over flipped taps (flip = 1); the values are scaled by 2^wexp[0]
 * (max |w| * 2^wexp < 2^15), written to *wexp on the device.  With flip = 1 out_hi / out_lo hold
 * 2 * ncols * 9 * Cout halves: the planes, then a tap-major copy (k = tap * Cout + c) that the data
 * gradient's ring reads.  scratch: DCS_RANGE_PARTS floats (dcs_pack_weights_h3_scratch_size bytes).
 * dcs_conv3_win_ok(d, dgrad): 1 if d is a geometry these passes cover: dgrad = 0, the forward of a
 * 3x3 stride-1 pad-1 conv (d as for dcs_conv_rows_in_stats); dgrad = 1, the padded-grid data gradient
 * (d as for dcs_conv_dgrad_reflect); both with mma = DCS_MMA_F16X3 and rng_a set, contiguous NHWC,
 * 16 <= W <= 128, 256 % W == 0, H % (256 / W) == 0, Cs % 32 == 0, Co % 128 == 0; the data gradient
 * also Cs == 256 and Co % 256 == 0 (its ring kernel).  It is the single place that decides: every
 * other geometry takes the rows pass (dcs_conv_rows_in_stats / dcs_conv_dgrad_reflect).
 * dcs_conv3_win_in_stats: forward + IN statistics partials (as dcs_conv_rows_in_stats; parts = NULL
 * for none; *nchunk = H * W / 256).
 * dcs_conv_dgrad_reflect_win: the data gradient of a ReflectionPad2d(1) + 3x3 conv
 * (dcs_conv_dgrad_reflect's contract, plus the pre-split flipped weights): the interior by the
 * window pass (+ addend), the padded grid's one-pixel ring into ring (dcs_conv_dgrad_reflect_ring_size
 * bytes, any allocation) and folded onto dx's border; w_hi / w_lo: a flip = 1 pack with ncols == d->Co.
 * The ring: one GEMM per ring segment and tap over the pack's tap-major copy (csrc/conv_win.hip
 * ring16_kernel: three ring copies summed in tap order, independent of the batch).  wpack is unused by
 * the window route (may be NULL); the parameter stays for the ABI. */
size_t dcs_pack_weights_h3_scratch_size(void);
int dcs_pack_weights_h3(const float* w, int Cout, int Cin, int flip, int ncols, void* out_hi, void* out_lo,
                        float* scratch, int* wexp, void* stream);
int dcs_conv3_win_ok(const dcs_conv_desc* d, int dgrad);
int dcs_conv3_win_in_stats(const dcs_conv_desc* d, const float* src, const void* w_hi, const void* w_lo,
                           const int* wexp, float* out, void* parts, size_t parts_bytes, int* nchunk, void* stream);
int dcs_conv_dgrad_reflect_win(const dcs_conv_desc* d, const float* dy, const float* wpack, const void* w_hi,
                               const void* w_lo, const int* wexp, const float* addend, float* dx, float* ring,
                               void* stream);
/* ---- f16x3 window convolution: the Generator's up-convolutions (modules/model.py:112-120) ----
 * nearest-x2 upsample + 3x3 zero-pad-1 conv as four 2x2 phase convolutions of the low-resolution
 * source (csrc/conv_subpix.hip): a workgroup owns 256 source pixels x 128 virtual columns (one column
 * phase, a 64-channel block, both row phases) and stages the source window once per 16-channel slice.
 * dcs_pack_subpix_h3: the phase weights (sums of the 3x3 taps that land on one source pixel) pre-split
 * into hi / lo fp16 planes, scaled by 2^wexp[0] of their own range; scratch: DCS_RANGE_PARTS floats.
 * kind 0: [4 Cout][4 Cin] (row = ((px * Cout / 64 + co / 64) * 2 + py) * 64 + co % 64, k = (c / 16) * 64 +
 * (u * 2 + t) * 16 + c % 16 for source offset (u, t)); Cout % 64 == 0, Cin % 16 == 0.  kind 1: the
 * transposed phase weights of the data gradient [Cin][16 Cout] (row = input channel, k = ((py * 2 + px) *
 * Cout / 16 + co / 16) * 64 + ((1 - u) * 2 + (1 - t)) * 16 + co % 16); Cout % 16 == 0, Cin % 128 == 0.
 * kinds 2 and 3: the stride-2 3x3 convolution's taps in kind 0's layout over dx's parity classes (its
 * data gradient, [4 Cin][4 Cout]; Cin % 64 == 0, Cout % 16 == 0) and in kind 1's layout over the source's
 * parity classes (its forward, [Cout][16 Cin]; Cout % 128 == 0, Cin % 16 == 0), zero where no tap lands;
 * kinds 5 and 4: the same for a 4x4 stride-2 convolution (w [Cout][Cin][4][4]).
 * dcs_subpix_win_ok(d): 1 if d is a sub-pixel rows descriptor (parity 2, as the rows pass takes it:
 * up = 1, Ho = 2 Hs) these kernels cover (contiguous NHWC, Cs % 16 == 0, Co % 64 == 0, min(Ws, 128)
 * dividing 256 and Ws, Hs % (256 / min(Ws, 128)) == 0, f16x3 / f16 with rng_a set, no prologue).
 * dcs_subpix_win: forward (+ IN statistics partials as dcs_conv_rows_in_stats when parts != NULL,
 * dcs_subpix_win_parts_size bytes; *nchunk = 4 x tiles per image). */
int dcs_pack_subpix_h3(const float* w, int Cout, int Cin, int kind, void* out_hi, void* out_lo, float* scratch,
                       int* wexp, void* stream);
int dcs_subpix_win_ok(const dcs_conv_desc* d);
size_t dcs_subpix_win_parts_size(const dcs_conv_desc* d);
int dcs_subpix_win(const dcs_conv_desc* d, const float* src, const void* w_hi, const void* w_lo, const int* wexp,
                   float* out, void* parts, size_t parts_bytes, int* nchunk, void* stream);
/* The data gradient of the same up-convolution (the adjoint: per phase a 2x2 conv of dy's phase sub-grid
 * with the transposed phase weights, dcs_pack_subpix_h3 with dgrad = 1).  d: the descriptor the rows pass
 * takes for it (source dy [N][Hs][Ws][Cs] contiguous, KH = KW = 4, stride 2, pt = pl = 1, zero pad, Ho = Hs / 2,
 * Wo = Ws / 2, Co = input channels of the forward, rng_a = dy's range record); dcs_subpix_win_dgrad_ok
 * checks it (Co % 128 == 0, min(Wo, 128) dividing 256 and Wo, Ho % (256 / min(Wo, 128)) == 0). */
int dcs_subpix_win_dgrad_ok(const dcs_conv_desc* d);
int dcs_subpix_win_dgrad(const dcs_conv_desc* d, const float* dy, const void* w_hi, const void* w_lo, const int* wexp,
                         float* dx, void* stream);
/* The down-convolutions (stride-2 3x3 zero-pad-1, modules/model.py:100-106) and the PatchGAN's stride-2
 * 4x4 zero-pad-1 layers (modules/model.py:118-131; every class offset a tap) on the same two kernels: the
 * forward as a sum over the source's four parity classes of <= 2x2 convolutions of the class sub-grids
 * (the sub-pixel data gradient's kernel; + IN statistics partials when parts != NULL,
 * dcs_stride2_win_parts_size bytes, *nchunk = tiles per image), the data gradient as four <= 2x2 phase
 * convolutions of dy onto dx's parity classes (the sub-pixel forward's kernel); the (class, offset) pairs
 * no tap reaches are skipped.  d: the rows pass's descriptor (parity 0: forward, Hs = 2 Ho, Co % 128 == 0;
 * parity 1: data gradient, Ho = 2 Hs, Co % 64 == 0), planes from dcs_pack_subpix_h3 kind 3 / 2 (3x3) or
 * 4 / 5 (4x4).  The forward takes the rows pass's prologue (d.pro_act AFFINE / RELU / LRELU with
 * pro_scale / pro_shift [N][Cs], Cs <= 512): a = act(y * scale + shift) staged, zero in the padding. */
/* Either data gradient (subpixel = 1: dcs_subpix_win_dgrad's descriptor and planes; 0: dcs_stride2_win's
 * parity-1 descriptor and planes) with the InstanceNorm backward's partial sums of its output fused, for
 * dx = da of a layer a = act(InstanceNorm(y)) (the down-convs' and up2's inputs): per (chunk, channel)
 * sum g and sum g * xhat, g = da * act'(xhat), xhat = y * scale + shift, into parts (Sum2 {float a, b}
 * [N][*nchunk][Co], dcs_phase_win_dgrad_inbwd_parts_size bytes) for dcs_in_act_backward_parts;
 * act DCS_ACT_AFFINE / _RELU / _LRELU, y NHWC like dx. */
size_t dcs_phase_win_dgrad_inbwd_parts_size(const dcs_conv_desc* d, int subpixel);
int dcs_phase_win_dgrad_inbwd(const dcs_conv_desc* d, int subpixel, const float* dy, const void* w_hi,
                              const void* w_lo, const int* wexp, float* dx, const float* y, const float* scale,
                              const float* shift, int act, void* parts, size_t parts_bytes, int* nchunk,
                              void* stream);
int dcs_stride2_win_ok(const dcs_conv_desc* d);
size_t dcs_stride2_win_parts_size(const dcs_conv_desc* d);
int dcs_stride2_win(const dcs_conv_desc* d, const float* src, const float* pro_scale, const float* pro_shift,
                    const void* w_hi, const void* w_lo, const int* wexp, float* out, void* parts, size_t parts_bytes,
                    int* nchunk, void* stream);
/* The same data gradient dx = da of a layer a = act(InstanceNorm(y)) (the first conv of a residual
 * block, modules/model.py:74-76), with the InstanceNorm backward's partial sums fused: the window
 * epilogue sums g = da * act'(xhat) and g * xhat (xhat = y * scale + shift) per (256-pixel tile,
 * channel) over the pixels the ring fold does not touch, and the fold sums its pixels with their final
 * values, into parts (Sum2 {float a, b} [N][*nchunk][Co], dcs_conv_dgrad_reflect_win_inbwd_parts_size
 * bytes) for dcs_in_act_backward_parts.  No addend; act DCS_ACT_AFFINE / _RELU / _LRELU; Co / 4
 * divides 256. */
size_t dcs_conv_dgrad_reflect_win_inbwd_parts_size(const dcs_conv_desc* d);
int dcs_conv_dgrad_reflect_win_inbwd(const dcs_conv_desc* d, const float* dy, const float* wpack, const void* w_hi,
                                     const void* w_lo, const int* wexp, float* dx, float* ring, const float* y,
                                     const float* scale, const float* shift, int act, void* parts, size_t parts_bytes,
                                     int* nchunk, void* stream);

/* Forward / data-gradient pass: out = gather(src) x B (+ bias, epilogue act). */
int dcs_conv_rows(const dcs_conv_desc* d, const float* src, const float* src2, const float* wpack,
                  const float* bias, const float* pro_scale, const float* pro_shift, float* out,
                  void* stream);

/* Forward pass with the InstanceNorm statistics of its output fused into the epilogue
 * (modules/model.py:94-111 — every conv that an InstanceNorm2d follows; aten convolution +
 * the statistics half of instance_norm): `out` as dcs_conv_rows, and per (row tile, channel) the
 * tile's count / mean / M2 / max / first argmax into `parts` (tiles never straddle images).
 * Needs parity 0 (or the sub-pixel forward, parity 2: per phase), Co > 4 and rows per image
 * % 128 == 0 (parts: dcs_conv_rows_in_stats_parts_size(d)
 * bytes; 0 = not applicable).  *nchunk receives the tiles per image, the `nchunk` of
 * dcs_in_stats_finish, which turns the partials into the scale / shift (and max / argmax) of
 * dcs_in_stats. */
size_t dcs_conv_rows_in_stats_parts_size(const dcs_conv_desc* d);
int dcs_conv_rows_in_stats(const dcs_conv_desc* d, const float* src, const float* src2, const float* wpack,
                           const float* bias, const float* pro_scale, const float* pro_shift, float* out, void* parts,
                           size_t parts_bytes, int* nchunk, void* stream);

/* Weight gradient: dw (OIHW) = sum_pixels dy^T x gather(x).  `d` describes the FORWARD conv
 * (source = x, output = dy).  ws must hold dcs_conv_wgrad_workspace_size(d) bytes. */
size_t dcs_conv_wgrad_workspace_size(const dcs_conv_desc* d);
int dcs_conv_wgrad(const dcs_conv_desc* d, const float* dy, const float* x, const float* x2,
                   const float* pro_scale, const float* pro_shift, float* dw, void* ws,
                   size_t ws_bytes, void* stream);

/* Data gradient of a 'same' K x K stride-1 convolution with ONE output channel (the Generator
 * head, modules/model.py:112: ReflectionPad(3) + Conv 7x7 64->1; aten convolution_backward
 * grad_input + reflection_pad2d_backward) onto its unpadded NHWC input:
 *   dx[n][y][x][c] = sum_{ty,tx} W[0][c][ty][tx] * sum_{(a,b) padding to (y,x)} dy[n][a-ty][b-tx]
 * dy: [N][H][W] (one channel); wk: the forward K-major pack ([(ty*K+tx)*C + c], dcs_pack_weights
 * kind 0, nmajor 0, ncols 1); dx: NHWC [N][H][W][C], C = 32 or 64; K = 3 or 7; 2*pad == K-1. */
int dcs_conv_dgrad_c1(const float* dy, int N, int H, int W, const float* wk, int C, int K, int pad, int pad_mode,
                      float* dx, void* stream);

/* Data gradient onto ONE input channel from C = 64 output channels: the image channel of the
 * Generator stem (modules/model.py:96-97, ReflectionPad(3) + Conv 7x7, stride 1) and the
 * PatchGAN's first layer (modules/model.py:121, Conv 4x4 stride 2 padding 1); aten
 * convolution_backward grad_input (+ reflection_pad2d_backward for the stem).  Two passes:
 *   z[q][t] = sum_c W[c][0][t] * dy[q][c]                                  (per dy pixel q)
 *   dx[n][y][x] = sum over padded positions (a,b) of (y,x) and taps t with (a-ty), (b-tx)
 *                 divisible by `stride` of z[n][(a-ty)/stride][(b-tx)/stride][t]
 * dy: NHWC [N][Hy][Wy][C]; wk[(ty*K+tx)*C + c] = W[c][0][ty][tx] (dcs_pack_weights kind 2, nmajor 0,
 * ncols 1, ci_count 1); (K, stride) = (7, 1) or (4, 2); pt/pl: top/left padding of pad_mode (reflect:
 * symmetric); dx: [N][H][W]; ws: dcs_conv_dgrad_to1_workspace_size(N, Hy, Wy, K) bytes. */
size_t dcs_conv_dgrad_to1_workspace_size(int N, int Hy, int Wy, int K);
int dcs_conv_dgrad_to1(const float* dy, int N, int Hy, int Wy, int C, const float* wk, int K, int stride, int pt,
                       int pl, int pad_mode, int H, int W, float* dx, void* ws, size_t ws_bytes, void* stream);

/* Pack up to 4 NCHW planes (x: [N][c1][H][W], x2: [N][c2][H][W] or NULL) into one NHWC
 * [N][H][W][4] tensor with zero channels after c1+c2 (c1 + c2 <= 4): the 4-channel layout the
 * vectorised stem convolution gathers (modules/model.py:94 input, trainer.py:451 concat). */
int dcs_pack_nhwc4(const float* x, int c1, const float* x2, int c2, int N, int H, int W, float* out,
                   float* rng,
                   void* stream);

/* Fold the gradient of a reflection-padded tensor back onto the tensor:
 * dx[n,i,j,c] = addend[n,i,j,c] + sum over padded positions mirroring to (i,j). */
/* Stride-1 data gradient of a ReflectionPad(1) + conv layer straight onto the unpadded grid
 * (modules/model.py:72-79 backward: aten convolution_backward + reflection_pad2d_backward, and
 * the residual add of the block when addend != NULL):
 *   dx[n][y][x][c] = addend[n][y][x][c] + sum over padded pixels (yp, xp) reflecting onto
 *                    (y, x) of (dy (*) flipped W)[n][yp][xp][c].
 * d describes the rows pass over the (H+2) x (W+2) padded grid exactly as for dcs_conv_rows
 * (pt = pl = KH-1, Ho = H+2, Wo = W+2, zero pad, stride 1).  The
 * conv epilogue writes interior pixels (plus the addend) into dx and the one-pixel ring into
 * ring (dcs_conv_dgrad_reflect_ring_size bytes); a small kernel then folds the ring in. */
size_t dcs_conv_dgrad_reflect_ring_size(const dcs_conv_desc* d);
int dcs_conv_dgrad_reflect(const dcs_conv_desc* d, const float* dy, const float* wpack, const float* addend,
                           float* dx, float* ring, void* stream);
int dcs_reflect_fold(const float* dxpad, const float* addend, float* dx, int N, int H, int W, int C,
                     int pad, void* stream);

/* Gradient of nearest x2 upsampling: dx[n,i,j,c] = sum_{a,b<2} dup[n,2i+a,2j+b,c]. */
int dcs_upsample2_grad(const float* dup, float* dx, int N, int H, int W, int C, void* stream);

/* ---- InstanceNorm2d(affine=False) (modules/model.py:61,94,97,110,124 → aten native_batch_norm) ---- */

/* Per-(n,c) statistics of an NHWC tensor: scale = 1/sqrt(var+eps), shift = -mean*scale
 * (so IN(x) = x*scale + shift), optional per-(n,c) max and argmax (pixel index) of x. */
size_t dcs_in_stats_workspace_size(int N, int HW, int C);
int dcs_in_stats(const float* x, int N, int HW, int C, float eps, float* scale, float* shift,
                 float* xmax, int32_t* xargmax, void* ws, size_t ws_bytes, void* stream);

/* The second half of dcs_in_stats over partials a producer wrote (dcs_conv_rows_in_stats):
 * parts [N][nchunk][C] chunk records, merged per (n,c) in a fixed order (deterministic). */
int dcs_in_stats_finish(const void* parts, int N, int C, int nchunk, float eps, float* scale, float* shift,
                        float* xmax, int32_t* xargmax, void* stream);

/* out = act(x*scale + shift) */
int dcs_in_apply(const float* x, const float* scale, const float* shift, float* out, int N, int HW,
                 int C, int act, float* rng,
                 void* stream);

/* Backward of a = act(IN(y)) given da: dy = scale*(g - mean(g) - xh*mean(g*xh)),
 * g = da*act'(xh), xh = y*scale+shift.  ws: dcs_in_stats_workspace_size(N,HW,C). */
int dcs_in_act_backward(const float* da, const float* y, const float* scale, const float* shift,
                        float* dy, int N, int HW, int C, int act, void* ws, size_t ws_bytes,
                        float* rng,
                        void* stream);
/* The same, its partial sums written by the producer of da (parts [N][nchunk][C] Sum2 records,
 * dcs_conv_dgrad_reflect_win_inbwd): merged per (n,c) in a fixed order, then applied.  ws: N*C*8 bytes. */
int dcs_in_act_backward_parts(const float* da, const float* y, const float* scale, const float* shift, float* dy,
                              int N, int HW, int C, int act, const void* parts, int nchunk, void* ws,
                              size_t ws_bytes, float* rng, void* stream);

/* ---- narrow-output convolutions (Co <= 4: Generator head, PatchGAN last layer, and the
 *      input-image gradients of the stem and the first PatchGAN layer) ---- */
int dcs_conv_rows_narrow(const dcs_conv_desc* d, const float* src, const float* src2,
                         const float* wpack, const float* bias, const float* pro_scale,
                         const float* pro_shift, float* out, void* stream);
/* The Generator head (modules/model.py:112: ReflectionPad2d(3) + Conv 7x7 64 -> 1 (+ bias) + Tanh) forward
 * in the fp16 operand modes, by tap projection on the MFMA pipe: z = a W (a = relu(src * pro_scale +
 * pro_shift) per (image, channel), W [64][49] from wpack = the narrow pack, K-major (tap * 64 + c) * ldb),
 * then a fixed-order 49-tap gather per output pixel.  d: the head's forward descriptor with pro_act =
 * DCS_ACT_RELU, epi_act DCS_ACT_NONE / _TANH, mma DCS_MMA_F16X3 / _F16 (dcs_head_fwd_proj_ok).  xmax:
 * [N][64] max of src per (image, channel) (dcs_in_stats_finish), for the operand scale.  out: [N][H][W]. */
int dcs_head_fwd_proj_ok(const dcs_conv_desc* d);
int dcs_head_fwd_proj(const dcs_conv_desc* d, const float* src, const float* wpack, const float* bias,
                      const float* pro_scale, const float* pro_shift, const float* xmax, float* out, void* stream);
/* The head's weight gradient in the same modes, by the transposed projection: dW[c][t] = sum_p a[p + off_t][c]
 * dy[p] as an MFMA GEMM (M = 64 channels, N = 49 taps, K = source columns) per workgroup band, the
 * workgroups' partials summed in a fixed order.  d, src, pro_scale, pro_shift, xmax as dcs_head_fwd_proj;
 * dy: [N][H][W] gradient at the conv output (before the bias); dw: [1][64][7][7] (OIHW).
 * ws: dcs_head_wgrad_proj_workspace_size(d) bytes. */
size_t dcs_head_wgrad_proj_workspace_size(const dcs_conv_desc* d);
int dcs_head_wgrad_proj(const dcs_conv_desc* d, const float* dy, const float* src, const float* pro_scale,
                        const float* pro_shift, const float* xmax, float* dw, void* ws, size_t ws_bytes,
                        void* stream);
/* The head's data gradient fused with the InstanceNorm + ReLU backward of its input (modules/model.py:110-112
 * backward) in the fp16 operand modes: da = the 7x7 reflect-pad-3 adjoint of dy_out onto 64 channels, on MFMA
 * (never written), then dy = IN-ReLU-backward(da) given y (the IN input, NHWC [N][H][W][64]) and its
 * per-(image, channel) scale / shift.  dy_out: [N][H][W] gradient at the head conv's output; wk: the weights
 * K-major, wk[(ty * 7 + tx) * 64 + c] = W[0][c][ty][tx].  act: DCS_ACT_RELU; mma: DCS_MMA_F16X3 / _F16;
 * H, W >= 8.  dy_rng: the range record of dy_out (dy_rng_n partial maxima, dcs_range_parts); rng: optional
 * range record of dy.  ws: dcs_head_dgrad_in_workspace_size(N, H, W) bytes. */
size_t dcs_head_dgrad_in_workspace_size(int N, int H, int W);
int dcs_head_dgrad_in(const float* dy_out, const float* dy_rng, int dy_rng_n, const float* wk, int N, int H, int W,
                      const float* y, const float* scale, const float* shift, int act, int mma, float* dy, void* ws,
                      size_t ws_bytes, float* rng, void* stream);
/* The Generator stem (modules/model.py:96-98: ReflectionPad2d(3) + Conv 7x7 cin -> 64 over the NHWC x 4
 * packed image, dcs_pack_nhwc4) forward in the f16x3 / f16 operand modes, on MFMA with the weights resident
 * in LDS.  d: the rows-pass descriptor of that conv (Cs = 4, pro_act / epi_act none, mma F16X3 / F16 with
 * both range records, ldb the packed weights' Kpad; dcs_stem_fwd_ok).  wpack: the rows pack (tap * 4 + c
 * K order).  parts (optional): per-(image, tile, channel) InstanceNorm partials for dcs_in_stats_finish
 * (dcs_stem_fwd_parts_size bytes; *nchunk receives the tiles per image). */
int dcs_stem_fwd_ok(const dcs_conv_desc* d);
size_t dcs_stem_fwd_parts_size(const dcs_conv_desc* d);
int dcs_stem_fwd(const dcs_conv_desc* d, const float* src, const float* wpack, float* out, void* parts,
                 size_t parts_bytes, int* nchunk, void* stream);
/* The stem's weight gradient in the same modes (rows pass over 64 output channels x 7 kernel-row blocks,
 * K = output pixels, on MFMA): d as for dcs_stem_fwd with cw = the weights' input channels (<= 4), rng_a
 * the range record of dy and rng_b that of the source; dw: [64][cw][7][7] (OIHW).
 * ws: dcs_stem_wgrad_workspace_size(d) bytes. */
int dcs_stem_wgrad_ok(const dcs_conv_desc* d);
size_t dcs_stem_wgrad_workspace_size(const dcs_conv_desc* d);
int dcs_stem_wgrad(const dcs_conv_desc* d, const float* dy, const float* src, float* dw, void* ws, size_t ws_bytes,
                   void* stream);
/* Pre-split fp16 planes of an N-major packed weight tensor for the f16x3 / f16 rows pass (dcs_conv_desc.b_h3):
 * out[r][0][k] = hi, out[r][1][k] = lo of wpack[r][k] * 2^e (fp16), e the operand exponent of the pack's range
 * record rng (dcs_pack_weights_r).  out: rows * 2 * ldb halves. */
int dcs_pack_split_h3(const float* wpack, int rows, int ldb, const float* rng, int rng_n, void* out, void* stream);
/* Every weight pack of a training step in two launches (instead of one or two small launches per pack).
 * A job is either a dcs_pack_weights_r pack (kind >= 0: w, Cout .. nmajor, out, rng as there; planes:
 * optional dcs_pack_split_h3 output of that pack, rows = ncols) or, with h3 = 1, a dcs_pack_weights_h3
 * pack (w, Cout, Cin, h3_flip, h3_ncols, h3_hi, h3_lo, h3_wexp, h3_scratch as there) or, with h3 = 2, a
 * dcs_pack_subpix_h3 pack (w, Cout, Cin, h3_flip = kind, h3_hi, h3_lo, h3_wexp, h3_scratch).  Results are
 * bit-identical to the per-pack calls.  jobs_dev: device copy of jobs[0 .. njobs) (the caller stages it;
 * jobs only supplies the host-side block counts); the b0 / b1 / p0 / p1 fields are filled here. */
typedef struct dcs_pack_job {
    const float* w;
    int32_t Cout, Cin, KH, KW, kind, ci_count, Kpad, ncols, nmajor, h3, h3_flip, h3_ncols;
    float* out;
    float* rng;
    void* planes;
    void* h3_hi;
    void* h3_lo;
    int32_t* h3_wexp;
    float* h3_scratch;
    int32_t b0, b1, p0, p1;  /* first block and block count of the job in the two launches (set by dcs_pack_plan) */
} dcs_pack_job;
/* Fills each job's block ranges and returns the grid sizes of the two launches (*g1, *g2). */
int dcs_pack_plan(dcs_pack_job* jobs, int njobs, int* g1, int* g2);
int dcs_pack_batch(const dcs_pack_job* jobs_dev, int njobs, int g1, int g2, void* stream);
size_t dcs_conv_wgrad_narrow_workspace_size(const dcs_conv_desc* d);
int dcs_conv_wgrad_narrow(const dcs_conv_desc* d, const float* dy, const float* x, const float* x2,
                          const float* pro_scale, const float* pro_shift, float* dw, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- CBAM tail of ResidualBlockWithCBAM (modules/model.py:6-52, 83-87) ----
 * out = x + CBAM(IN(y)):  y is the raw conv2 output NHWC [N,H*W,C] with its InstanceNorm
 * coefficients (scale, shift) and the per-(n,c) max / argmax of y from dcs_in_stats.
 * w1: fc.0 [Cr][C], w2: fc.2 [C][Cr], wsa: [2][ksa][ksa] (spatial-attention conv, no bias).
 * Saved for backward: ca [N][C], sin_ [N][HW][2] (channel mean/max), sarg [N][HW] (argmax
 * channel), sa [N][HW]. */
int dcs_cbam_forward(const float* x, const float* y, const float* scale, const float* shift,
                     const float* ymax, const float* w1, const float* w2, const float* wsa,
                     int N, int H, int W, int C, int Cr, int ksa,
                     float* ca, float* sin_, int32_t* sarg, float* sa, float* out, float* rng,
                     void* stream);
size_t dcs_cbam_backward_workspace_size(int N, int H, int W, int C, int Cr, int ksa);
/* Given dout = dL/d(out): dy (gradient of the raw conv2 output y, InstanceNorm backward
 * included) and the gradients of w1, w2, wsa (overwritten).  The residual gradient (dout
 * itself, for x) is NOT added here. */
int dcs_cbam_backward(const float* dout, const float* y, const float* scale, const float* shift,
                      const float* ymax, const int32_t* yargmax, const float* w1, const float* w2,
                      const float* wsa, const float* ca, const float* sin_, const int32_t* sarg,
                      const float* sa, int N, int H, int W, int C, int Cr, int ksa, float* dy,
                      float* dw1, float* dw2, float* dwsa, void* ws, size_t ws_bytes, float* rng,
                      void* stream);

/* Global statistics of the batch-coupled losses over data-parallel ranks (SURVEY.md §8e
 * option ii; replaces the whole-batch reductions of modules/trainer.py:126-128 and :170-180
 * when the batch is sharded).  Phase functions: each leaves this shard's partial sums in a
 * caller buffer (red: double, histograms: uint32[512]) that the caller sums over ranks (one
 * all-reduce) before the next phase reads it.  All ranks then finish with the loss of the whole
 * batch; d loss / d pred of the local shard is multiplied by grad_scale (the world size, so
 * that the all-reduce-MEAN of parameter gradients equals the whole-batch gradient).  With one
 * rank and no reduction the result equals dcs_loss_contrast_region / _edge.  ws: the same
 * dcs_loss_workspace_size(N, H, W) buffer for every phase of one loss evaluation.
 *   region: partial -> sum red[0..6] -> finish
 *   edge:   partial -> sum red[0..4] -> for pass 0..3 { hist -> sum hist[0..511] -> select }
 *           -> topk -> sum red[5..8] -> finish                                           */
int dcs_loss_contrast_region_partial(const float* pred, const float* target, const float* source, int N, int H,
                                     int W, float threshold, double* red, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_region_finish(const float* pred, int N, int H, int W, float weight, const double* red,
                                    float grad_scale, float* out, float* grad, void* ws, size_t ws_bytes,
                                    void* stream);
int dcs_loss_contrast_edge_partial(const float* pred, const float* target, int N, int H, int W, double* red,
                                   void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_edge_hist(int N, int H, int W, int pass, const double* red, uint32_t* hist, void* ws,
                                size_t ws_bytes, void* stream);
int dcs_loss_contrast_edge_select(int pass, const uint32_t* hist, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_edge_topk(int N, int H, int W, double* red, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_edge_finish(const float* pred, int N, int H, int W, const double* red, float grad_scale,
                                  float* out, float* grad, void* ws, size_t ws_bytes, void* stream);

/* ---- losses (modules/trainer.py:22-184, 347-351; pytorch_msssim.SSIM) ----
 * All take single-channel planes [N,1,H,W]; each writes the loss value to out[0] and the
 * gradient d(loss)/d(pred) (unscaled) to grad (may be NULL for value only). */
size_t dcs_loss_workspace_size(int N, int H, int W);
int dcs_loss_l1(const float* pred, const float* target, int64_t n, float* out, float* grad,
                void* ws, size_t ws_bytes, void* stream);
int dcs_loss_mse(const float* pred, const float* target, int64_t n, float* out, float* grad,
                 void* ws, size_t ws_bytes, void* stream);
int dcs_loss_mse_const(const float* pred, float target, int64_t n, float* out, float* grad,
                       void* ws, size_t ws_bytes, void* stream);
int dcs_loss_gradient(const float* pred, const float* target, int N, int H, int W, float* out,
                      float* grad, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_attention(const float* pred, const float* target, const float* source, int N,
                                int H, int W, float sigma, float min_w, float max_w, int k,
                                float* out, float* grad, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_region(const float* pred, const float* target, const float* source, int N,
                             int H, int W, float threshold, float weight, float* out, float* grad,
                             void* ws, size_t ws_bytes, void* stream);
int dcs_loss_contrast_edge(const float* pred, const float* target, int N, int H, int W, float* out,
                           float* grad, void* ws, size_t ws_bytes, void* stream);
int dcs_loss_ssim(const float* X, const float* Y, int N, int H, int W, float data_range,
                  int win, float sigma, float k1, float k2, float* out, float* grad, void* ws,
                  size_t ws_bytes, void* stream);

/* ---- optimizer (torch.optim.Adam, modules/trainer.py:360-362, 514, 520, 525) ----
 * One launch over a flat parameter buffer. */
int dcs_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float bias_c1, float bias_c2, void* stream);

/* ---- input pipeline (modules/preprocess.py:6-55, modules/mask_generator.py:11-347, as used by
 *      modules/dataset.py:109-181 for every training slice) ---- */

/* HU transform of N stored-pixel slices [N][H][W]: hu = f32(raw)*slope[n] + intercept[n]
 * (preprocess.py:45-46); img = [-1,1] image of clip(hu, hu_min, hu_max), soft-squeezed
 * (apply_soft_squeezing, preprocess.py:6-40, k = 10/sigma, threshold 0.9) when soft != 0, else
 * linear (preprocess.py:53).  raw_dtype: 0 int16, 1 uint16, 2 float32.  slope/intercept are
 * device arrays [N].  hu or img may be NULL (not written).  float32 op order as numpy. */
int dcs_hu_transform(const void* raw, int raw_dtype, const float* slope, const float* intercept, int N,
                     int H, int W, float hu_min, float hu_max, int soft, float sigma, float* hu,
                     float* img, void* stream);

/* Anatomical masks of N HU slices [N][H][W] (generate_anatomical_masks, 2-D path per slice):
 * lung (detect_lung), mediastinum (detect_mediastinum), bone (detect_bone), lung_vessel
 * (detect_lung_vessels).  Host arrays:
 *   thresholds[7] = {lung_lower, lung_upper, vessel_lower, vessel_upper, mediastinum_lower,
 *                    mediastinum_upper, bone_threshold}        (reference defaults -1000, -300,
 *                    -300, 600, -300, 450, 200)
 *   iparams[3]    = {min_size, border_margin, spine_start}     (64, 32, int(H*(1-0.25)))
 *   chan[4]       = output channel of {lung, mediastinum, bone, lung_vessel}, -1 = not wanted
 * out: float32 [N][nout][H][W] in {0,1} (the channel concat of dataset.py:135-158).
 * lung_in: optional device uint8 [N][H][W] binary lung mask used instead of detect_lung (the
 *   lung_mask argument of detect_mediastinum / detect_bone / detect_lung_vessels); NULL =
 *   computed from hu.
 * ws: dcs_masks_workspace_size(N, H, W) bytes.  H, W <= 1024.  Bit-exact with the reference. */
size_t dcs_masks_workspace_size(int N, int H, int W);
int dcs_anatomical_masks(const float* hu, const uint8_t* lung_in, int N, int H, int W, const float* thresholds,
                         const int32_t* iparams, const int32_t* chan, int nout, float* out, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- volume post-processing of the synthesis stage (modules/postprocess.py:6-301,
 *      generate.py:212-254) ----
 * Dense [D][H][W] device volumes, x fastest.  Every entry point checks its arguments on the
 * host before any launch (null pointers, D/H/W <= 0, radius, kernel size, axis, dtype) and
 * returns DCS_E_INVALID on a bad call.  Results are bit-identical to scipy / numpy on the host:
 * double accumulation in the host's operation order, no fused multiply-add. */
#define DCS_VOL_F32 0
#define DCS_VOL_F64 1
#define DCS_VOL_I16 2
#define DCS_VOL_U16 3
#define DCS_VOL_MAX_RADIUS 16
#define DCS_VOL_MAX_MEDIAN 9
#define DCS_VOL_MINMAX_PARTS 1024

/* scipy.ndimage.gaussian_filter1d(mode='reflect') along axis 0 (z), 1 (y) or 2 (x).
 * weights: HOST array of radius+1 doubles, the first half of the normalised kernel including
 * its centre (weights[radius]); radius <= DCS_VOL_MAX_RADIUS.  (in_dtype, out_dtype) is
 * (F32,F32), (F32,F64) [= filtering in.astype(float64)] or (F64,F64).  in != out. */
int dcs_vol_gauss1d(const void* in, int in_dtype, void* out, int out_dtype, int D, int H, int W, int axis,
                    int radius, const double* weights, void* stream);
/* scipy.ndimage.median_filter(size=(k,1,1), mode='reflect') on float32; k odd, <= DCS_VOL_MAX_MEDIAN */
int dcs_vol_median_z(const float* in, float* out, int D, int H, int W, int k, void* stream);
/* scalar Kalman filter along z of every pixel: x = x + gain[k]*(in[k] - x), x0 = in[0], in double.
 * gain: DEVICE array [D] (the gain sequence depends only on the two variances). */
int dcs_vol_kalman_z(const float* in, const double* gain, double* out, int D, int H, int W, void* stream);
/* out[0] = min, out[1] = max of n finite floats.  ws: 2*DCS_VOL_MINMAX_PARTS floats. */
int dcs_vol_minmax(const float* x, int64_t n, float* out, float* ws, void* stream);
/* unsharp_mask + threshold restore + int16 cast over n voxels:
 *   detail = one_minus_amount*(sm - blur_sm) + amount*(og - blur_og), og = (double)original
 *   v = clip(sm + detail*amount, minmax[0], minmax[1]);  original >= hu_threshold keeps original;
 *   out = int16 truncated toward zero.  sm_dtype: DCS_VOL_F32 or DCS_VOL_F64.
 * minmax: device float[2] of dcs_vol_minmax over the whole original volume. */
int dcs_vol_unsharp_finish(const void* sm, int sm_dtype, const double* blur_sm, const double* blur_og,
                           const float* original, const float* minmax, int64_t n, double one_minus_amount,
                           double amount, float hu_threshold, int16_t* out, void* stream);
/* the same without sharpening: threshold restore + int16 cast */
int dcs_vol_finish(const void* sm, int sm_dtype, const float* original, int64_t n, float hu_threshold,
                   int16_t* out, void* stream);
/* HU-range merge of three stored-value series (generate.py:212-236): hu = f32(raw)*slope[z] +
 * intercept[z]; voxels with soft_lo <= hu <= soft_hi take soft, then lung_lo <= hu <= lung_hi
 * take lung.  stored_dtype: DCS_VOL_I16 or DCS_VOL_U16.  out (stored dtype) and out_f32 (the
 * merged values as float32) are optional, at least one is required. */
int dcs_vol_merge(const void* raw, const void* soft, const void* lung, int stored_dtype, const float* slope,
                  const float* intercept, int D, int H, int W, float soft_lo, float soft_hi, float lung_lo,
                  float lung_hi, void* out, float* out_f32, void* stream);
/* Enhancement-difference merge of three stored-value series (the reference's synthesis_test,
 * generate.py:302-477; modules/inference.py::synthesize_enhancement on every slice).  Per voxel,
 * with a = slope[z], b = intercept[z], in float32, one IEEE operation per step (no fused
 * multiply-add, the division correctly rounded):
 *   r  = f32(raw);  hr = r*a + b;  hs = f32(soft)*a + b;  hl = f32(lung)*a + b
 *   es = hs - hr;   el = hl - hr;  valid = hr > min_hu
 *   m  = r;  if (es > threshold && valid) m = m + es / a;  if (el > threshold && valid) m = m + el / a
 * Both comparisons are strict; a voxel can take both additions, soft tissue first.  out_f32 = m
 * (float32, generally not integral).  stored_dtype: DCS_VOL_I16 or DCS_VOL_U16. */
int dcs_vol_merge_enhance(const void* raw, const void* soft, const void* lung, int stored_dtype, const float* slope,
                          const float* intercept, int D, int H, int W, float threshold, float min_hu,
                          float* out_f32, void* stream);

/* ---- slice series of the resident inference path (generate.py --pipeline resident:
 *      modules/inference.py::stored_from_output + synthesize, torchvision Resize) ---- */
#define DCS_RESIZE_MAX_TAPS 18 /* taps of one output sample of dcs_resize_aa (in/out <= 8) */

/* Model outputs -> stored values -> HU-range merge in one pass over a [D][H][W] series.
 *   y_soft, y_lung: the two Generators' outputs, float32 in [-1, 1]
 *   raw: the NCCT stored values, stored_dtype DCS_VOL_I16 or DCS_VOL_U16; slope/intercept: device [D]
 * Per element, in float32 and in the host's operation order (no fused multiply-add):
 *   hu = ((y + 1) / 2) * span + lo;  px = (hu - intercept[z]) / slope[z]
 *   stored = px cast to the stored dtype by truncation toward zero (numpy astype)
 * with span = hi - lo formed by the caller.  Then dcs_vol_merge's rule on hu_raw = f32(raw) *
 * slope[z] + intercept[z]: soft_lo <= hu_raw <= soft_hi takes the soft value, then lung_lo <=
 * hu_raw <= lung_hi takes the lung value.  A px that does not fit the stored dtype is not pinned:
 * numpy's cast is undefined there, and this kernel keeps the low 16 bits of the saturating
 * float32 -> int32 conversion.
 * Outputs, each optional (NULL = not written), at least one required: soft_stored, lung_stored and
 * merged in the stored dtype; merged_f32 = the merged values as float32. */
int dcs_vol_translate_merge(const void* raw, int stored_dtype, const float* slope, const float* intercept,
                            const float* y_soft, const float* y_lung, int D, int H, int W, float soft_lo,
                            float soft_hi, float soft_span, float lung_lo, float lung_hi, float lung_span,
                            void* soft_stored, void* lung_stored, void* merged, float* merged_f32, void* stream);
/* Model outputs -> stored values -> enhancement-difference merge in one pass.  ps and pl are
 * dcs_vol_translate_merge's stored values of the two outputs (same operations, same truncating
 * cast); then dcs_vol_merge_enhance's rule per voxel with a = slope[z], b = intercept[z]:
 *   r  = f32(raw);  hr = r*a + b;  hs = f32(ps)*a + b;  hl = f32(pl)*a + b
 *   es = hs - hr;   el = hl - hr;  valid = hr > min_hu
 *   m  = r;  if (es > threshold && valid) m = m + es / a;  if (el > threshold && valid) m = m + el / a
 * so merged_f32 equals dcs_vol_merge_enhance of the stored series bit for bit.  merged_f32 is
 * required; soft_stored and lung_stored (stored dtype) are optional. */
int dcs_vol_translate_enhance(const void* raw, int stored_dtype, const float* slope, const float* intercept,
                              const float* y_soft, const float* y_lung, int D, int H, int W, float soft_lo,
                              float soft_span, float lung_lo, float lung_span, float threshold, float min_hu,
                              void* soft_stored, void* lung_stored, float* merged_f32, void* stream);
/* Antialiased bilinear resize (F.interpolate(mode="bilinear", align_corners=False, antialias=True))
 * of NC planes [H][W] -> [oh][ow], separable: horizontal pass, then vertical pass.  The caller
 * builds the weights (modules/hip/slices.py::aa_tables) and passes them as DEVICE tables, one set
 * per axis: start[o] = first input sample of output o, count[o] <= taps its tap count,
 * weights[o][taps] padded with zeros.  The kernels accumulate acc = acc + x * w from zero in tap
 * order, in float32 without fused multiply-add; table entries are clamped into the input.
 * An axis whose size does not change is skipped and its tables may be NULL; both sizes equal is
 * DCS_E_INVALID (return the input instead), and so is in/out > 8 on either axis (more than
 * DCS_RESIZE_MAX_TAPS taps).  tmp: [NC][H][ow] floats, required when both axes change. */
int dcs_resize_aa(const float* in, float* out, float* tmp, int NC, int H, int W, int oh, int ow,
                  const int32_t* x_start, const int32_t* x_count, const float* x_weights, int x_taps,
                  const int32_t* y_start, const int32_t* y_count, const float* y_weights, int y_taps,
                  void* stream);
/* F.interpolate(mode="nearest") of NC planes: src = min(int(floorf(dst * float32(in / out))), in - 1)
 * per axis; exact. */
int dcs_resize_nearest(const float* in, float* out, int NC, int H, int W, int oh, int ow, void* stream);

/* ---- evaluation metrics (calculate.py's MAE, PSNR, SSIM, MS-SSIM, EMD, texture similarity, cosine
 *      similarity and Euclidean distance; modules/metrics.py on the host) ----
 * a (target) and b (prediction): dense float32 [D][H][W] device volumes, x fastest.  Every result
 * is float64 per slice.  Arithmetic: the float32 elementwise steps of the numpy expressions
 * (a - b, its square, (x - off) / div), float64 accumulation of every sum, SSIM and Sobel in
 * float64.  No floating-point atomics: per-workgroup float64 partials go to the caller's
 * workspace ws (dcs_met_workspace_size bytes serve every entry point but the two region ones,
 * which have dcs_met_region_workspace_size) and are folded in a fixed
 * order, so results are bit-identical from run to run.  Every entry point checks its arguments on
 * the host before any launch and returns DCS_E_INVALID (DCS_E_WORKSPACE for a short workspace).
 * affine: optional HOST array {a_off, a_div, b_off, b_div}; the kernels then read
 * (x - off) / div in float32 (0 where div == 0) in place of x, which is calculate.py's
 * normalize() for off = min, div = max - min.  NULL reads the volumes as they are. */
#define DCS_MET_NSTATS 9
#define DCS_MET_TILE_X 64 /* output tile of dcs_met_ssim and dcs_met_sobel_ts */
#define DCS_MET_TILE_Y 32
#define DCS_MET_PAIR_CHUNK 8192 /* voxels of one slice per workgroup of the pair passes */
/* bytes of workspace for a [D][H][W] pair; 0 for dimensions the entry points refuse */
size_t dcs_met_workspace_size(int D, int H, int W);
/* one pass over both volumes: out[z][0..8] = sum|a-b|, sum f32((a-b)^2), sum ab, sum a^2,
 * sum b^2, min a, max a, min b, max b of slice z (MAE, PSNR, cosine similarity, global range) */
int dcs_met_pair_stats(const float* a, const float* b, int D, int H, int W, const float* affine, double* out,
                       void* ws, size_t ws_bytes, void* stream);
/* out[z] = the SUM of skimage's structural_similarity map (7x7 uniform window, sample covariance,
 * K1 0.01, K2 0.03) over the interior cropped by 3; the mean divides by (H-6)(W-6).  H, W >= 7. */
int dcs_met_ssim(const float* a, const float* b, int D, int H, int W, const float* affine, double data_range,
                 double* out, void* ws, size_t ws_bytes, void* stream);
/* skimage.filters.sobel (mode reflect) of both slices on the fly:
 * out[z][0..2] = sum|g1 - g2|, max g1, max g2 */
int dcs_met_sobel_ts(const float* a, const float* b, int D, int H, int W, double* out, void* ws, size_t ws_bytes,
                     void* stream);
/* out[z] = sum (a_n - b_n)^2, each slice normalised in float32 by its own (x - min) / (max - min + 1e-8f);
 * stats: the device result of dcs_met_pair_stats on the same pair without affine */
int dcs_met_ed(const float* a, const float* b, int D, int H, int W, const double* stats, double* out, void* ws,
               size_t ws_bytes, void* stream);
/* out[z] = sum|a_n - b_n| of two volumes whose slices are sorted (EMD: the Wasserstein-1 distance
 * of equal-sized samples is the mean of this) */
int dcs_met_sorted_l1(const float* a, const float* b, int D, int H, int W, const float* affine, double* out,
                      void* ws, size_t ws_bytes, void* stream);
/* out = (x - off) / div in float32, 0 where div == 0 (calculate.py's normalize) */
int dcs_met_normalize(const float* x, int64_t n, float off, float div, float* out, void* stream);
/* One level of MS-SSIM (torchmetrics' MultiScaleStructuralSimilarityIndexMeasure defaults, restated
 * in modules/metrics.py): out[z][0..1] = the SUMS of the SSIM map and of its contrast-structure
 * factor (2 sxy + c2) / (sx2 + sy2 + c2) over the (H-10) x (W-10) windows that lie inside slice z;
 * the means divide by (H-10)(W-10).  window: HOST array of the DCS_MET_MSSSIM_TAPS float64 taps of
 * the separable filter (x, y, x^2, y^2, xy in float64 along W, then along H); no N/(N-1) factor.
 * H, W >= 11; c1, c2 >= 0; dcs_met_workspace_size bytes of workspace suffice. */
#define DCS_MET_MSSSIM_TAPS 11
int dcs_met_msssim_level(const float* a, const float* b, int D, int H, int W, const double* window, double c1,
                         double c2, double* out, void* ws, size_t ws_bytes, void* stream);
/* The next MS-SSIM level of both volumes, [D][H/2][W/2] (an odd last row or column is dropped):
 * out[i][j] = float32((((x[2i][2j] + x[2i][2j+1]) + x[2i+1][2j]) + x[2i+1][2j+1]) * 0.25), the sum
 * in float64.  H, W >= 2; the outputs alias nothing. */
int dcs_met_pool2(const float* a, const float* b, float* out_a, float* out_b, int D, int H, int W, void* stream);
/* Region-wise evaluation (calculate.py --regions; modules/metrics.py::region_sums states it) of the
 * three series vue (NCCT), std (CECT, the target) and gen (sCECT).  ranges: HOST array {lung_min,
 * lung_max, soft_min, soft_max, thr, min_hu}, finite.  A voxel's owner is lung where lung_min <= vue
 * <= lung_max, else soft where soft_min <= vue <= soft_max, else rest; the true enhancement is
 * f32(std - vue) > thr && vue > min_hu, the predicted one the same with gen for std.
 * out[z][0..20]: for lung, soft, rest and the true enhancement in turn n, sum|std-gen|,
 * sum f32((std-gen)^2), sum f32(gen-std); then TP, FP, FN of the predicted against the true
 * enhancement; then sum f32(std-vue) and sum f32(gen-vue) over the true enhancement.  Counts are exact.
 * region_map: optional device [D][H][W] bytes, owner (0 lung, 1 soft, 2 rest) | 4 where the true
 * enhancement holds, the input of dcs_met_region_ssim.  One pass, 12 bytes read per voxel. */
#define DCS_MET_REGION_NSUMS 21
#define DCS_MET_REGION_NSSIM 8
/* bytes of workspace of the two region entry points; 0 for dimensions they refuse */
size_t dcs_met_region_workspace_size(int D, int H, int W);
int dcs_met_region_sums(const float* vue, const float* std_, const float* gen, int D, int H, int W,
                        const float* ranges, double* out, unsigned char* region_map, void* ws, size_t ws_bytes,
                        void* stream);
/* out[z][0..7] = {number of region pixels inside the interior cropped by 3, SUM of dcs_met_ssim's
 * map of (std, gen) over them} for lung, soft, rest and the true enhancement, read from region_map
 * (dcs_met_region_sums wrote it).  H, W >= 7. */
int dcs_met_region_ssim(const float* std_, const float* gen, const unsigned char* region_map, int D, int H, int W,
                        double data_range, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- LPIPS of calculate.py (lpips 0.1.4, net='alex'; modules/metrics.py::lpips_taps states it) ----
 * Activations are NHWC float32.  Layers 2-5 of the AlexNet trunk run on dcs_conv_rows (bias + ReLU
 * in its epilogue); these are the first layer and the pass between the convolutions.  A slice's
 * result depends on that slice alone, whatever N is.  No atomics; bit-identical from run to run. */
/* AlexNet's first layer (11x11 stride 4 pad 2 -> 64 channels) + ReLU of N slices x [N][H][W],
 * H, W >= 11, read as t = ((x - off) / div) * 2 - 1 in float32 (div > 0) and, folded in, the scaling
 * layer on three equal channels: out[N][Ho][Wo][64], Ho = (H - 7) / 4 + 1.  wx: device [121][64], the
 * tap-major weights of t (sum_c w[o][c] / scale_c).  cb: device [16][64], the bias plus the constant
 * channel's weights (-sum_c w[o][c] shift_c / scale_c) summed over the taps inside the image, per
 * class y * 4 + x with 0 = the first two kernel rows (columns) cut, 1 = none, 2 / 3 = the last one /
 * two cut: the padding is zero AFTER the scaling layer, so the constant is not a bias. */
int dcs_lpips_stem(const float* x, int N, int H, int W, float off, float div, const float* wx, const float* cb,
                   float* out, void* stream);
/* bytes of workspace of dcs_lpips_tap for N slices of h x w maps; 0 for bad dimensions */
size_t dcs_lpips_tap_workspace_size(int N, int h, int w);
/* One tap from one read of the ReLU maps fa, fb [N][h][w][C] (C = 64, 192, 256 or 384) of both
 * volumes: out[n] = sum over the pixels of sum_c lin[c] * (fa_c / (|fa| + 1e-10) - fb_c / (|fb| + 1e-10))^2
 * with |f| = sqrt(sum_c f_c^2), in float64 on the float32 samples (the mean divides by h * w); and,
 * where pool_a / pool_b are given, the 3x3 stride-2 max pool (floor sizes, h, w >= 3) of both maps,
 * [N][(h-3)/2+1][(w-3)/2+1][C].  lin: device [C]. */
int dcs_lpips_tap(const float* fa, const float* fb, int N, int h, int w, int C, const float* lin, float* pool_a,
                  float* pool_b, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- difference-map stage (modules/nmodel: the normal-map U-Net run one slice at a time, then
 *      modules/postprocess.py::apply_diffmap) ----
 * Activations are NHWC float32.  The U-Net's 3x3 convolutions run on dcs_conv_rows; these are the
 * passes between them.  scale / shift: the eval-mode BatchNorm folded per channel (device [C],
 * scale of either sign).  Float32 arithmetic without fused multiply-add; vector stores only, no
 * atomics, results bit-identical from run to run.  Arguments are checked on the host before any
 * launch (DCS_E_INVALID). */
/* out[i * cstride] = ((clip(hu[i], -1024, 3071) + 1024) / 4095) * 2 - 1 (modules/nmodel's
 * normalize_hu, bit for bit).  cstride 1: dense; cstride 4: pixels of 4 channels, channels 1..3
 * written as zero (the first convolution's 16-byte source). */
int dcs_unet_normalize_hu(const float* hu, int64_t n, int cstride, float* out, void* stream);
/* a = relu(y * scale[c] + shift[c]) of y [N][H][W][C], C % 4 == 0, read once:
 *   skip[((n*H + h)*W + w) * skip_cstride + c] = a   (skip_cstride >= C, % 4 == 0: the leading
 *       channels of a concatenated tensor, or C for a dense one)
 *   pooled [N][H/2][W/2][C] = the 2x2 maximum of a (floor sizes: an odd last row / column is dropped);
 *       H, W >= 2. */
int dcs_unet_affine_relu_pool(const float* y, const float* scale, const float* shift, int N, int H, int W, int C,
                              float* skip, int skip_cstride, float* pooled, void* stream);
/* Bilinear x2 upsample with align_corners=True of x [N][h][w][C] (C % 4 == 0), placed inside an
 * Ho x Wo map (Ho >= 2h, Wo >= 2w) with (Ho - 2h) / 2 zero rows before it and the rest after, the
 * same split along x:  out[((n*Ho + Y)*Wo + X) * out_cstride + c], out_cstride >= C, % 4 == 0
 * (pass the pointer of the first channel slot behind the skip).  With scale / shift (both or
 * neither) the source is read as relu(x * scale[c] + shift[c]).  A 1-pixel source axis repeats
 * that pixel.  Source coordinate: float32(o) * (float32(in - 1) / float32(2 in - 1)), as ATen. */
int dcs_unet_upsample2_pad(const float* x, const float* scale, const float* shift, int N, int h, int w, int C,
                           int Ho, int Wo, float* out, int out_cstride, void* stream);
/* The U-Net's tail and apply_diffmap in one pass over P pixels of y [P][C] (C % 4 == 0, <= 256):
 *   o = sum_c relu(y[p][c] * scale[c] + shift[c]) * w[c] + bias     (1x1 convolution: c ascending;
 *       for C = 32, 64, 128, 256 per group of 16 channels, the group sums added pairwise)
 *   d = ((o + 1) / 2) * 4000                                         (denormalize_diff)
 *   diff[p] = d                     when diff != NULL
 *   m = d < threshold ? 0 : d;  vol_out[p] = vol_in[p] + float32(uint8(m))   when vol_in != NULL
 * uint8(m): truncation to a 32-bit integer (saturating), low 8 bits kept, as numpy's astype on the
 * host for every m below 2^31.  vol_out may alias vol_in; at least one output is required. */
int dcs_unet_out_diffmap(const float* y, const float* scale, const float* shift, const float* w, float bias,
                         int64_t P, int C, float threshold, const float* vol_in, float* vol_out, float* diff,
                         void* stream);
/* apply_diffmap for a difference map that already exists: vol_out[i] = vol_in[i] +
 * float32(uint8(diff[i] < threshold ? 0 : diff[i])); diff is not modified; vol_out may alias vol_in. */
int dcs_unet_apply_diffmap(const float* diff, int64_t n, float threshold, const float* vol_in, float* vol_out,
                           void* stream);

/* ---- training the normal-map U-Net on depth-1 patches (modules/hip/unet_train.py) ----
 * The passes between the convolutions of a training step.  Activations are NHWC float32, C % 4 == 0.
 * Every reduction is two-stage with a fixed order (float64 partials per block, added in block
 * order; no atomics): the same inputs give the same bits from run to run.  ws: 8-byte aligned. */
/* BatchNorm in training mode over the M = N*H*W values per channel of y [M][C] (M >= 2, C <= 1024):
 *   mean[c], invstd[c] = 1 / sqrt(biased variance + eps)          (from float64 sums)
 *   scale[r*C + c] = gamma[c] * invstd[c], shift[r*C + c] = beta[c] - mean[c] * scale, r < nrep
 *       (the pair dcs_conv_rows' prologue, dcs_unet_affine_relu_pool and dcs_unet_upsample2_pad read)
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var + momentum * variance * M / (M - 1)   (both or NULL) */
size_t dcs_unet_bn_stats_workspace_size(int64_t M, int C);
int dcs_unet_bn_stats(const float* y, int64_t M, int C, const float* gamma, const float* beta, float eps,
                      float momentum, int nrep, float* scale, float* shift, float* mean, float* invstd,
                      float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
/* Backward of a = relu(y * scale + shift) with batch statistics, y [N][H][W][C]:
 *   g = da * [y * scale + shift > 0],  xhat = (y - mean) * invstd
 *   sums:  dbeta[c] = sum g,  dgamma[c] = sum g * xhat
 *   apply: dy = scale[c] * (g - dbeta[c] / M - xhat * dgamma[c] / M)      (scale = gamma * invstd)
 * The gradient da reaching a comes in one of three forms:
 *   A  da[((n*H + h)*W + w) * da_cstride + c]: a channel slice of a wider tensor (pass the pointer
 *      of its first channel; da_cstride >= C, % 4 == 0);  dpool = dout = wout = NULL
 *   B  A plus dpool [N][H/2][W/2][C], the gradient of the 2x2 max pool of a, added at the first
 *      maximum of each window in row-major order (recomputed from y; an odd last row / column is in
 *      no window);  H, W >= 2
 *   C  da[p][c] = dout[p] * wout[c] (the 1x1 output projection; da = dpool = NULL); sums also writes
 *      dwout[c] = sum_p dout[p] * a[p][c] and dbias[0] = sum_p dout[p]. */
size_t dcs_unet_bn_relu_backward_workspace_size(int N, int H, int W, int C);
int dcs_unet_bn_relu_backward_sums(const float* da, int da_cstride, const float* dpool, const float* dout,
                                   const float* wout, const float* y, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, int N, int H, int W, int C, float* dgamma,
                                   float* dbeta, float* dwout, float* dbias, void* ws, size_t ws_bytes, void* stream);
int dcs_unet_bn_relu_backward_apply(const float* da, int da_cstride, const float* dpool, const float* dout,
                                    const float* wout, const float* y, const float* scale, const float* shift,
                                    const float* mean, const float* invstd, int N, int H, int W, int C,
                                    const float* dgamma, const float* dbeta, float* dy, void* stream);
/* The training tail over P pixels of y [P][C] (C <= 256):
 *   o[p] = sum_c relu(y[p][c] * scale[c] + shift[c]) * wout[c] + bias[0]   (written when o != NULL)
 *   loss[0] = gscale * sum_p |o[p] - target[p]| / P
 *   dout[p] = gscale * sign(o[p] - target[p]) / P,  sign(0) = 0 */
size_t dcs_unet_l1_out_workspace_size(int64_t P, int C);
int dcs_unet_l1_out(const float* y, const float* scale, const float* shift, const float* wout, const float* bias,
                    const float* target, int64_t P, int C, float gscale, float* o, float* dout, float* loss, void* ws,
                    size_t ws_bytes, void* stream);
/* Adjoint of dcs_unet_upsample2_pad: dx [N][h][w][C] from the gradient of the padded Ho x Wo map,
 * dcat[((n*Ho + Y)*Wo + X) * cstride + c] (pass the pointer of the first upsampled channel).  A
 * gather in ascending output order with the forward's own weights. */
int dcs_unet_upsample2_pad_backward(const float* dcat, int cstride, int N, int h, int w, int C, int Ho, int Wo,
                                    float* dx, void* stream);
/* out[0] = sqrt(sum g[i]^2), out[1] = min(1, clip / (out[0] + 1e-6)) (1 for clip <= 0): the
 * coefficient of clip_grad_norm_, left on the device for dcs_scale_dev. */
size_t dcs_unet_sumsq_workspace_size(int64_t n);
int dcs_unet_sumsq(const float* g, int64_t n, float clip, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- training targets of the normal-map U-Net from a voxel-aligned NCCT / CECT pair
 *      (prepare_nmodel_data.py; modules/nmodel/prepare.py::residual_targets on the host) ----
 * ncct, cect: device [D][H][W] stored values, 16 bits each, read as uint16 where the series' flag
 * is set and as int16 otherwise, independently.  ncct_slope .. cect_intercept: device float32 [D],
 * one rescale pair per slice and series.  merged: optional device float32 [D][H][W], the merged
 * sCECT before the smoothing in stored-value units of the NCCT series
 * (modules/inference.py::translate_volume_device); read only.  Per voxel with sn, in, sc, ic the
 * slice's pairs, in float32, one IEEE operation per step (no fused multiply-add, the division
 * correctly rounded):
 *   x = f32(ncct) * sn + in          -> vue_out   (the NCCT in HU)
 *   y = f32(cect) * sc + ic
 *   g = merged * sn + in             (g = x when merged is NULL, which is then not read)
 *   d = (y - g) / sn                 -> diff_out  (stored-value units of the NCCT: what apply_diffmap adds)
 * so both outputs equal the host's bit for bit.  stats_out[z][0..10], float64: n, n(d >= threshold),
 * n(d < 0), n(d > 4000), sum clip(d, 0, 4000), sum |d|, sum x, sum y, sum x^2, sum y^2, sum xy (x, y
 * widened to float64 before they are multiplied).  Counts are exact.  One pass, 16 bytes per voxel
 * (12 without merged), 16-byte float32 accesses when H * W % 4 == 0 and the pointers allow it.
 * One workgroup per DCS_MET_PAIR_CHUNK voxels of a slice writes a record of DCS_NMODEL_NSTATS
 * float64 partials to ws, a second launch folds a slice's records in index order: no atomics,
 * bit-identical from run to run.  Arguments are checked on the host before any launch
 * (DCS_E_INVALID; DCS_E_WORKSPACE for a short workspace); no output may alias an input. */
#define DCS_NMODEL_NSTATS 11
/* bytes of workspace; 0 for dimensions the entry point refuses */
size_t dcs_nmodel_targets_workspace_size(int D, int H, int W);
int dcs_nmodel_targets(const void* ncct, int ncct_unsigned, const float* ncct_slope, const float* ncct_intercept,
                       const void* cect, int cect_unsigned, const float* cect_slope, const float* cect_intercept,
                       const float* merged, int D, int H, int W, float threshold, float* vue_out, float* diff_out,
                       double* stats_out, void* ws, size_t ws_bytes, void* stream);

/* ---- heart-mask clean-up and organ masking (organ_masks.hip; modules/organ_masks.py is the
 *      definition; reference modify_heart_mask.py:87-198, masking.py:455-541) ----
 * Dense [D][H][W] uint8 label volumes, x fastest (a NIfTI file's own order: nibabel's [x, y, z] is
 * x = W index, y = H index, z = D index).  Integer atomics only (min / max / add), so every result is
 * order-independent and bit-identical from run to run, and equal to the host functions bit for bit.
 * Arguments are checked on the host before any launch: DCS_E_INVALID for null pointers, an empty
 * volume, D*H*W >= 2^31 or a label >= 256; DCS_E_WORKSPACE for a short workspace. */
/* 3-D connected components of {vol == match}, 6-connectivity (scipy.ndimage.label's default
 * structure up to renumbering).  labels[i]: the smallest voxel index of i's component, -1 for
 * background.  At every root r (labels[r] == r): count[r] voxels; with sums and keys (both or
 * neither) also sums[r], sums[np + r], sums[2 np + r] = the sums of the x, y, z coordinates and
 * keys[r] = the minimum of (x * H + y) * D + z, the component's first voxel in [x, y, z] raster
 * order.  Entries of count / sums / keys that are not at a root are left untouched. */
int dcs_cc3_label(const uint8_t* vol, int match, int D, int H, int W, int32_t* labels, int32_t* count,
                  int64_t* sums, uint32_t* keys, void* stream);
/* bytes of workspace; 0 for dimensions the entry point refuses */
size_t dcs_heart_workspace_size(int D, int H, int W);
/* modules/organ_masks.py::modify_heart_label: the lowest heart component (centre z, ties by first
 * voxel) is chosen on the device, the column gap cut, the float64 distance test (one rounding per
 * numpy operation, offset_y_base_m1 = offset_y_base - 1 as the host computes it), the size filter
 * and the write-back follow without a host wait.  out must not alias vol. */
int dcs_heart_modify(const uint8_t* vol, int D, int H, int W, int heart_label, int gap_threshold, double offset,
                     double offset_y_base_m1, double offset_z, int min_region, uint8_t* out, void* ws,
                     size_t ws_bytes, void* stream);
/* bytes of workspace for N slices handled `chunk` slices at a time (chunk * nlabels binary images
 * of 5 bytes per pixel, plus N*H*W + 256 N); 0 for dimensions the entry point refuses
 * (chunk * nlabels > 65535 or chunk * nlabels * (H*W + 4096) >= 2^31 among them) */
size_t dcs_organ_mask_workspace_size(int N, int H, int W, int nlabels, int chunk);
/* modules/organ_masks.py::organ_mask.  target: HOST array of nlabels labels (each < 256).
 * brush1 / brush2: HOST arrays of (dy, dx) int8 pairs, 1..25 offsets within radius 2 (the
 * thickness-2 and thickness-4 line brushes).  A (slice, label) pair the slice does not hold costs
 * no pixel pass.  out: uint8 0/1 [N][H][W], must not alias labels. */
int dcs_organ_mask(const uint8_t* labels, int N, int H, int W, const int32_t* target, int nlabels,
                   const int8_t* brush1, int nbrush1, const int8_t* brush2, int nbrush2, int chunk, uint8_t* out,
                   void* ws, size_t ws_bytes, void* stream);
/* out_k[i] = mask[i] ? fill : k[i] for three int16 series of n values in one pass; no output may alias an input */
int dcs_organ_apply(const int16_t* a, const int16_t* b, const int16_t* c, const uint8_t* mask, int64_t n, int fill,
                    int16_t* out_a, int16_t* out_b, int16_t* out_c, void* stream);

/* small utilities */
int dcs_scale_add(float* y, const float* x, float a, int64_t n, void* stream); /* y += a*x */
/* out = x * (*s) with s a device scalar (loss backward without a host sync) */
int dcs_scale_dev(const float* x, const float* s, float* out, int64_t n, void* stream);
/* dst[i][k] += src[i][k], k < n[i], for count tensors in one launch (host arrays of device
 * pointers; chunks of 64 tensors per launch). */
int dcs_multi_add(int count, const float* const* src, float* const* dst, const int64_t* n, void* stream);
/* dy = da * act'(y): relu/lrelu given the pre-activation y; tanh given the output y */
int dcs_act_backward(const float* da, const float* y, float* dy, int64_t n, int act, float* rng,
                     void* stream);
/* out[c] = sum_p x[p][c] (conv bias gradients) */
size_t dcs_channel_sum_workspace_size(int64_t P, int C);
int dcs_channel_sum(const float* x, int64_t P, int C, float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DUCOSY_HIP_H */
