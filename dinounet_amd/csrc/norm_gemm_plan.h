// The plan of du_layernorm_bwd_prod (norm_gemm.hip): whether the row-owning "LayerNorm backward of a product" kernel serves a call and
// how the call is cut, decided once and before anything launches.  du_ln_bwd_prod_plan is the only function that decides;
// du_layernorm_bwd_prod executes the plan, du_layernorm_bwd_prod_plan reports it -- callers (ops.py) ask the latter and run the unfused
// pair (data-gradient product + du_layernorm_bwd) for every call it declines.
//
// Served: bf16, D == 1024, K % 64 == 0 with K <= 256 (the 64 x K block of G and the 64 x 1024 block of dy share the CU's 160 KB of LDS),
// ldg and ldw multiples of 8 and >= K, x / G / Wt / dx / dres 16-byte aligned (dres may be NULL).  x, dx and dres are dense (rows, D).
#pragma once
#include "common.h"

struct LnProdPlan {
  int rc;             // DU_OK; DU_ERR_UNSUPPORTED: declined (run the unfused pair); DU_ERR_BAD_ARG: a NULL operand or a non-positive size
  int served;         // 1 exactly when rc == DU_OK
  int block_rows;     // rows whose dy is formed and consumed at a time (64)
  int wgs;            // workgroups = partial rows of the dw / db reduction
  int rows_per_wg;    // contiguous rows a workgroup owns: max(64, ceil(rows / 256))
  int lds_bytes;      // dynamic LDS of the launch
  int64_t ws_elems;   // fp32 scratch: wgs * D * 2
};
LnProdPlan du_ln_bwd_prod_plan(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K, const void* dx,
                               const void* dres, int64_t rows, int D);
