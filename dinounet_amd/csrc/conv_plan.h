// The dispatch plans of the direct 3x3 convolution (conv_strip.hip, conv_halo.hip): everything that is decided about a call, decided once
// and before anything launches.
//
// du_conv3x3_plan / du_conv3x3_wgrad_plan (conv_halo.hip) are the only functions that choose a kernel.  du_conv3x3_halo, du_conv3x3_strip and
// du_conv3x3_wgrad_halo execute the plan; du_conv3x3_halo_parts, du_conv3x3_wgrad_halo_blocks and the two *_plan_describe entries read it --
// so the reported kernel, statistics rows and slab count are the executed ones by construction.  The launchers take the plan's decision as
// a parameter.  Pure host functions: operand addresses are looked at for alignment only.
#pragma once
#include "common.h"

enum { DU_CONV_NONE = 0, DU_CONV_STRIP = 1, DU_CONV_HALO = 2 };          // Conv3x3Plan::kernel
enum { DU_WGRAD_NONE = 0, DU_WGRAD_ROWS = 1, DU_WGRAD_ROUND3 = 2 };      // Conv3x3WgradPlan::kernel

struct Conv3x3Plan {
  int rc;             // DU_OK, or what du_conv3x3_halo returns without launching: DU_ERR_BAD_ARG / DU_ERR_UNSUPPORTED
  int kernel;         // DU_CONV_*
  int variant;        // strip: NP * 10 + NCO (planes of 32 input channels, 32-channel output halves); halo: CK * 10 + TN (chunk, Cout / 32)
  int strip_rows;     // strip: image rows per segment
  int stats_parts;    // rows of the partial-statistics array this kernel writes; 0 = this call emits no statistics (not asked for, or a
                      // strip shape whose byte sizes the strip kernel declines: the tile kernel runs it without statistics)
};
Conv3x3Plan du_conv3x3_plan(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H, int W,
                            const void* w, const void* y, int64_t ldy, bool want_stats);

struct Conv3x3WgradPlan {
  int rc;
  int kernel;         // DU_WGRAD_*: conv3x3_wgrad_rows_kernel, or the round-3 conv3x3_wgrad_halo_kernel
  int variant;        // CK * 10 + MT (chunk, Cout / 32)
  int blocks;         // workgroups = partial dW slabs
};
Conv3x3WgradPlan du_conv3x3_wgrad_plan(const void* x, int64_t ldx, const void* x2, int64_t ldx2, int C1, int Cin, int Cout, int B, int H,
                                       int W, const void* dy, int64_t lddy);

// conv_strip.hip: the strip kernel's rules and its launcher.  du_conv3x3_strip_kind: NP * 10 + NCO and the rows per segment of a shape
// it serves (0 = none); du_conv3x3_strip_fits: the byte sizes its 32-bit DMA offsets reach
int du_conv3x3_strip_kind(int C1, int Cin, int Cout, bool concat, int B, int H, int W, int* rows);
bool du_conv3x3_strip_fits(int B, int H, int W, int64_t ldmax, int64_t ldy);
int du_conv3x3_strip_run(const Conv3x3Plan& plan, const void* x, int64_t ldx, const void* x2, int64_t ldx2, int Cout, int B, int H, int W,
                         const void* w, const float* bias, void* y, int64_t ldy, float* stats_part, void* stream);
