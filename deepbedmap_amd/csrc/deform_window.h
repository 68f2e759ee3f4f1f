// What the launchers of deform_fwd.hip need of the two LDS-window kernels (deform_window.hip): the constants their form choice reads, the
// plane limits, and one launch function per kernel.
#pragma once
#include <hip/hip_runtime.h>

// deform_conv64_fusedw_kernel (fp32): a workgroup owns DWF_POS consecutive positions of one image
constexpr int DWF_R = 2;
constexpr int DWF_POS = 128;
constexpr int DWF_MAXPIX = 528;               // window pixels the LDS layout is sized for (36-wide planes: 12 rows x 43 = 516)
// deform_conv64_x3w_kernel (split bf16): a workgroup owns a DW_T x DW_T tile of positions
constexpr int DW_T = 16;                          // tile edge (positions)

// (these three cross a file boundary only since the fused kernels were split by pass: hidden, so that libdbm.so exports what it did)
#define DBM_WINDOW_LOCAL __attribute__((visibility("hidden")))

// plane limits of both kernels (see deform_window.hip); past them the launchers take the gathering kernels
DBM_WINDOW_LOCAL bool deform_window_plane_ok(int H, int W);
#define DBM_DEFORM_WINDOW_LIMITS "H <= 32765, W <= 65533, H * W < 2^24"

// Each sets its kernel's dynamic-LDS attribute once and launches; arguments as the launchers of deform_fwd.hip receive them
// (wx: launch_pack_deform_x3's image; N * tilesX * tilesY workgroups).  No checks, no profiler bracket: the callers' own.
DBM_WINDOW_LOCAL void launch_deform_conv64_fusedw(const float* xt, const float* off, const float* wf, const float* bias, float* y, float* yt, int N, int H, int W,
                                 long offsn, int act, float slope, hipStream_t s);
DBM_WINDOW_LOCAL void launch_deform_conv64_x3w(const float* xt, const float* off, const void* wx, const float* bias, float* y, float* yt, int N, int H, int W,
                              long offsn, int act, float slope, int tilesX, int tilesY, hipStream_t s);
