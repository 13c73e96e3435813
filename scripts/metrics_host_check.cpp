// Host-side check of csrc/metrics.hip's argument validation and workspace sizing, for a sanitizer
// build on the CPU.  No kernel is launched: every call below is refused by the checks, or only
// sizes a workspace.  Build and run from the repository root (no GPU needed):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I include scripts/metrics_host_check.cpp \
//       -o /tmp/metrics_host_check && /tmp/metrics_host_check
#include "../ducosy-gan_amd/csrc/metrics.hip"

#include <cmath>
#include <cstdlib>
#include <limits>
#include <vector>

namespace dcs {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
bool in_range_arena(const void*) { return false; }
}  // namespace dcs

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, dcs::g_error.c_str()); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

int main() {
    // stand-ins for device pointers: never dereferenced on the host
    alignas(16) static float fa[8], fb[8];
    alignas(16) static double out[32], ws[32], stats[32];
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int big = std::numeric_limits<int>::max();

    // workspace sizing: bad and boundary dimensions
    EXPECT(dcs_met_workspace_size(0, 8, 8) == 0 && dcs_met_workspace_size(1, 0, 8) == 0);
    EXPECT(dcs_met_workspace_size(-1, 8, 8) == 0 && dcs_met_workspace_size(1, 8, -8) == 0);
    EXPECT(dcs_met_workspace_size(big, big, big) == 0 && dcs_met_workspace_size(1, big, big) == 0);
    EXPECT(dcs_met_workspace_size(1, 1 << 15, 1 << 15) == 0);             // one slice of 2^30 voxels
    EXPECT(dcs_met_workspace_size(1, 1 << 15, (1 << 15) - 1) > 0);         // just below
    EXPECT(dcs_met_workspace_size(big, 1, 1) == (size_t)big * 9 * sizeof(double));  // the largest grid
    EXPECT(dcs_met_workspace_size(1 << 20, 512, 512) == 0);                // 2^38 voxels
    EXPECT(dcs_met_workspace_size(1, 1, 1) == 9 * sizeof(double));
    EXPECT(dcs_met_workspace_size(2, 8, 70) == 2 * 9 * sizeof(double));
    EXPECT(dcs_met_workspace_size(128, 512, 512) == 128 * 128 * 3 * sizeof(double));
    EXPECT(dcs_met_workspace_size(3, 33, 4097) == 3 * 2 * 65 * 3 * sizeof(double));  // tiles outgrow the chunks
    for (int d = 1; d < 40; d += 7)
        for (int h = 1; h < 200; h += 13)
            for (int w = 1; w < 9000; w += 997) {
                const size_t n = dcs_met_workspace_size(d, h, w);
                const size_t pair = (size_t)d * (((size_t)h * w + DCS_MET_PAIR_CHUNK - 1) / DCS_MET_PAIR_CHUNK) * 9 * sizeof(double);
                const size_t tile = (size_t)d * ((h + 31) / 32) * ((w + 63) / 64) * 3 * sizeof(double);
                EXPECT(n >= pair && n >= tile && (n == pair || n == tile));
            }

    const size_t need = dcs_met_workspace_size(2, 8, 8);
    EXPECT(need <= sizeof(ws));
    // null, misaligned, bad dimensions, short workspace: every pair entry point
    EXPECT(dcs_met_pair_stats(nullptr, fb, 2, 8, 8, nullptr, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pair_stats(fa, fb, 2, 8, 8, nullptr, nullptr, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pair_stats(fa, fb, 2, 8, 8, nullptr, out, nullptr, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pair_stats(reinterpret_cast<float*>(reinterpret_cast<char*>(fa) + 1), fb, 2, 8, 8, nullptr, out, ws,
                              need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pair_stats(fa, fb, 0, 8, 8, nullptr, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pair_stats(fa, fb, 2, 8, 8, nullptr, out, ws, need - 1, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_pair_stats(fa, fb, 2, 8, 8, nullptr, out, ws, 0, nullptr) == DCS_E_WORKSPACE);
    const float bad1[4] = {0.f, nan, 0.f, 1.f}, bad2[4] = {inf, 1.f, 0.f, 1.f};
    EXPECT(dcs_met_pair_stats(fa, fb, 2, 8, 8, bad1, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_sorted_l1(fa, fb, 2, 8, 8, bad2, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_sorted_l1(fa, fb, 2, big, big, nullptr, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_sorted_l1(fa, fb, 2, 8, 8, nullptr, out, ws, 8, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_ed(fa, fb, 2, 8, 8, nullptr, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ed(fa, fb, 2, 8, 8, out, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ed(fa, fb, 2, 8, 8, stats, out, ws, 8, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_ed(fa, fb, -2, 8, 8, stats, out, ws, need, nullptr) == DCS_E_INVALID);
    // SSIM: the window, data_range
    EXPECT(dcs_met_ssim(fa, fb, 2, 6, 8, nullptr, 1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, 8, 6, nullptr, 1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, -8, 8, nullptr, 1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, 8, 8, nullptr, (double)nan, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, 8, 8, nullptr, -1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, 8, 8, bad1, 1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_ssim(fa, fb, 2, 8, 8, nullptr, 1.0, out, ws, 8, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_ssim(fa, fb, big, big, big, nullptr, 1.0, out, ws, need, nullptr) == DCS_E_INVALID);
    // Sobel
    EXPECT(dcs_met_sobel_ts(fa, nullptr, 2, 8, 8, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_sobel_ts(fa, fb, 2, 8, 0, out, ws, need, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_sobel_ts(fa, fb, 2, 8, 8, out, ws, 2 * 3 * sizeof(double) - 1, nullptr) == DCS_E_WORKSPACE);
    // normalize
    EXPECT(dcs_met_normalize(nullptr, 8, 0.f, 1.f, fb, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_normalize(fa, 0, 0.f, 1.f, fb, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_normalize(fa, -5, 0.f, 1.f, fb, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_normalize(fa, 1ll << 38, 0.f, 1.f, fb, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_normalize(fa, 8, nan, 1.f, fb, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_normalize(fa, 8, 0.f, inf, fb, nullptr) == DCS_E_INVALID);
    // MS-SSIM level: the window, its taps, c1 / c2, two partials per tile
    double win[DCS_MET_MSSSIM_TAPS], badwin[DCS_MET_MSSSIM_TAPS];
    for (int k = 0; k < DCS_MET_MSSSIM_TAPS; ++k) win[k] = badwin[k] = 1.0 / DCS_MET_MSSSIM_TAPS;
    const double c1 = 1e-4, c2 = 9e-4;
    const size_t need11 = dcs_met_workspace_size(2, 11, 11);
    EXPECT(need11 >= 2 * 2 * sizeof(double) && need11 <= sizeof(ws));
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 10, 11, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 10, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, -11, 11, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 0, 11, 11, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, big, big, big, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(nullptr, fb, 2, 11, 11, win, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, c1, c2, nullptr, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, c1, c2, out, nullptr, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, nullptr, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(reinterpret_cast<float*>(reinterpret_cast<char*>(fa) + 2), fb, 2, 11, 11, win, c1, c2, out,
                                ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, c1, c2, out, ws, 2 * 2 * sizeof(double) - 1, nullptr) ==
           DCS_E_WORKSPACE);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, c1, c2, out, ws, 0, nullptr) == DCS_E_WORKSPACE);
    badwin[10] = (double)nan;
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, badwin, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    badwin[10] = (double)inf, badwin[0] = 0.0;
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, badwin, c1, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, (double)nan, c2, out, ws, need11, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_msssim_level(fa, fb, 2, 11, 11, win, c1, -1.0, out, ws, need11, nullptr) == DCS_E_INVALID);
    // the existing workspace size covers two partials per tile of the (H-10) x (W-10) interior
    for (int d = 1; d < 40; d += 7)
        for (int h = 11; h < 700; h += 53)
            for (int w = 11; w < 9000; w += 997) {
                const size_t tile = (size_t)d * ((h - 10 + 31) / 32) * ((w - 10 + 63) / 64) * 2 * sizeof(double);
                EXPECT(dcs_met_workspace_size(d, h, w) >= tile);
            }
    // 2x2 pooling
    static float oa[8], ob[8];
    EXPECT(dcs_met_pool2(nullptr, fb, oa, ob, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, nullptr, oa, ob, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, nullptr, ob, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, nullptr, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, 2, 1, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, 2, 2, 1, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, 0, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, 2, -2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, big, big, big, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, ob, 1 << 20, 512, 512, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, reinterpret_cast<float*>(reinterpret_cast<char*>(oa) + 1), ob, 2, 2, 2, nullptr) ==
           DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, oa, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, fa, ob, 2, 2, 2, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_pool2(fa, fb, oa, fb, 2, 2, 2, nullptr) == DCS_E_INVALID);
    // region-wise evaluation: its own workspace (21 per chunk or 8 per tile of the interior)
    static unsigned char rmap[8];
    const float ranges[6] = {-1000.f, -150.f, -150.f, 250.f, 5.f, -400.f};
    float badr[6] = {-1000.f, -150.f, -150.f, 250.f, 5.f, nan};
    EXPECT(dcs_met_region_workspace_size(0, 8, 8) == 0 && dcs_met_region_workspace_size(big, big, big) == 0);
    EXPECT(dcs_met_region_workspace_size(1, 1, 1) == 21 * sizeof(double));
    EXPECT(dcs_met_region_workspace_size(3, 33, 65) == 3 * 21 * sizeof(double));
    EXPECT(dcs_met_region_workspace_size(2, 70, 300) == 2 * 10 * 8 * sizeof(double));   // the tiles outgrow 3 chunks
    EXPECT(dcs_met_region_workspace_size(128, 512, 512) == 128 * 128 * 8 * sizeof(double));
    EXPECT(dcs_met_region_workspace_size(big, 1, 1) == (size_t)big * 21 * sizeof(double));
    const size_t needr = dcs_met_region_workspace_size(2, 8, 8);
    EXPECT(needr == 2 * 21 * sizeof(double));
    EXPECT(dcs_met_region_sums(nullptr, fa, fb, 2, 8, 8, ranges, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, nullptr, fb, 2, 8, 8, ranges, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, nullptr, 2, 8, 8, ranges, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, 8, 8, nullptr, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, 8, 8, badr, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    badr[5] = -400.f, badr[0] = -inf;
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, 8, 8, badr, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, 8, 8, ranges, nullptr, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 0, 8, 8, ranges, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, big, big, ranges, out, rmap, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(reinterpret_cast<float*>(reinterpret_cast<char*>(fa) + 2), fa, fb, 2, 8, 8, ranges, out, rmap,
                               ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_sums(fa, fa, fb, 2, 8, 8, ranges, out, rmap, ws, needr - 1, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, 2, 6, 8, 1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, 2, 8, 6, 1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(fa, fb, nullptr, 2, 8, 8, 1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(nullptr, fb, rmap, 2, 8, 8, 1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, 2, 8, 8, (double)nan, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, 2, 8, 8, -1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, 2, 8, 8, 1.0, out, ws, 2 * 8 * sizeof(double) - 1, nullptr) == DCS_E_WORKSPACE);
    EXPECT(dcs_met_region_ssim(fa, fb, rmap, big, big, big, 1.0, out, ws, needr, nullptr) == DCS_E_INVALID);
    for (int d = 1; d < 40; d += 7)
        for (int h = 7; h < 700; h += 53)
            for (int w = 7; w < 9000; w += 997) {
                const size_t tile = (size_t)d * ((h - 6 + 31) / 32) * ((w - 6 + 63) / 64) * 8 * sizeof(double);
                const size_t pair = (size_t)d * (((size_t)h * w + DCS_MET_PAIR_CHUNK - 1) / DCS_MET_PAIR_CHUNK) * 21 * sizeof(double);
                EXPECT(dcs_met_region_workspace_size(d, h, w) == (tile > pair ? tile : pair));
            }
    std::printf(failures ? "metrics host check: %d FAILED\n" : "metrics host check: ok\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
