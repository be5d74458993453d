// The dispatch plan of the depthwise 3x3 (elementwise.hip: the row kernels; dwconv.hip: the band kernels): everything that is decided
// about a call, decided once and before anything launches.
//
// du_dwconv_plan (dwconv.hip) is the only function that chooses a kernel.  du_dwconv3x3_fwd and du_dwconv3x3_bwd execute the plan;
// du_dwconv3x3_bwd_ws_elems and du_dwconv3x3_plan_describe read it -- so the reported kernel, band height, partial rows and scratch size
// are the executed ones by construction.  The launchers take the plan's decision as a parameter.  A pure host function of the call's
// numbers: no operand is looked at.
//
// The rules.  Band family (dwconv_band_*): bf16, C % 8 == 0, every grid width even, the work-item count within 2^30, option key 19 != 0
// (band_shape_ok), ld % 8 == 0 and bs % 8 == 0 -- for the token pyramid with any activation, for one NHWC segment with DU_ACT_NONE only.
// Row family otherwise: C, ld, bs multiples of the vector width (8 bf16 / 4 fp32), H and W even for the pyramid; the 4-pixel kernels
// (dwconv_row4_kernel, dwconv_bwd_weight_kernel<bf16, true, true>) for the bf16 pyramid with W % 8 == 0, dwconv_kernel /
// dwconv_bwd_weight_kernel<T, PYR> for the rest.  A pyramid call is a contiguous (B, 21 n, C) tensor: ld == C, bs == 21 n C.  The row
// family's activation derivative is a separate act_bwd_kernel launch over B * pixels * C contiguous elements: a strided tensor with an
// activation is DU_ERR_UNSUPPORTED there.
#pragma once
#include "common.h"

enum { DU_DW_NONE = 0, DU_DW_ROW = 1, DU_DW_ROW4 = 2, DU_DW_BAND = 3 };                              // DwconvPlan::kernel
enum { DU_DW_ACT_NONE = 0, DU_DW_ACT_PASS = 1, DU_DW_ACT_ON_LOAD = 2 };                              // DwconvPlan::act_bwd
enum { DU_DWW_NONE = 0, DU_DWW_ROW = 1, DU_DWW_PYR = 2, DU_DWW_PYR_ROW4 = 3, DU_DWW_BAND = 4 };      // DwconvPlan::wgrad

struct DwconvPlan {
  int rc;             // DU_OK, or what du_dwconv3x3_fwd / _bwd return without launching: DU_ERR_BAD_ARG / DU_ERR_UNSUPPORTED
  int kernel;         // forward and data gradient: dwconv_kernel, dwconv_row4_kernel or dwconv_band_kernel (DU_DW_*).  kernel, wgrad, rows
                      // and ws_elems follow from (dtype, B, H, W, C, pyramid, act) and the strides' alignment; rc judges the rest
  int R;              // band height of forward and data gradient; 0 for the row kernels
  int act_bwd;        // DU_DW_ACT_*: no activation; act_bwd_kernel in a launch of its own; applied on load by dwconv_band_dgrad_act_kernel
  int wgrad;          // DU_DWW_*: dwconv_bwd_weight_kernel<T, false>, <T, true>, <bf16, true, true> or dwconv_band_wgrad_kernel
  int wgrad_R;        // band height of the weight gradient; 0 for the row kernels
  int strip;          // row kernels: pixels per workgroup of the weight gradient; 0 for the band kernel
  int rows;           // partial rows (= workgroups of the row kernels) the weight gradient writes; the finalize kernel sums them
  int64_t ws_elems;   // fp32 scratch of the backward: rows * 10 * C
};
DwconvPlan du_dwconv_plan(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act);

// elementwise.hip: the row family's launchers.  du_dwconv_row_run: forward (flip = false) or data gradient (flip = true: the caller passes
// no bias, no z and DU_ACT_NONE); du_dwconv_row_wgrad: partial rows into `part`, then dwconv_wgrad_finalize_kernel OVERWRITES dw / db
void du_dwconv_row_run(const DwconvPlan& plan, int dtype, const void* x, const float* w, const float* bias, void* y, void* z, int64_t ld,
                       int64_t bs, int B, int H, int W, int C, int pyramid, int act, bool flip, hipStream_t st);
void du_dwconv_row_wgrad(const DwconvPlan& plan, int dtype, const void* x, const void* dz, float* dw, float* db, int64_t ld, int64_t bs,
                         int B, int H, int W, int C, float* part, hipStream_t st);
