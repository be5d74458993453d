// du_gemm's dispatch plan: everything that is decided about a product, decided once and before anything launches.
//
// du_gemm_plan (gemm.hip) is the only function that chooses a kernel family.  du_gemm executes the plan; du_gemm_route, du_gemm_ws_elems,
// du_gemm_ks_ws_bytes and du_gemm_plan_describe read it -- so the reported route is the executed one by construction.  The rules of each
// family stay beside its kernels, in the predicates below, and the launchers take the plan's decision as a parameter.
#pragma once
#include "common.h"

// how the rows behind the last full tile row of a tall bf16 NT product are computed (du_gemm_ragged_rows)
enum { DU_TAIL_NONE = 0, DU_TAIL_RIDES = 1, DU_TAIL_SKINNY_FUSED = 2, DU_TAIL_SKINNY_PAIR = 3, DU_TAIL_TILE_ENGINE = 4 };

struct GemmPlan {
  int rc;               // DU_OK, or what du_gemm returns without launching: DU_ERR_BAD_ARG / DU_ERR_UNSUPPORTED
  int family;           // du_gemm_route's number (include/dinounet_hip.h): 0 .. 8
  int variant;          // gemm_p8.hip NT kernels (families 3, 4, 6, 8 and the 4-wave kernel): du_gemm_p8_choice's 1 .. 5; 0 elsewhere
  int gather;           // the ConvTranspose2d k2 s2 operand is gathered from dY in place (gemm_p8.hip's GA forms, gemm_rk.hip)
  int tail_rows;        // rows that leave the head's tile grid (0 .. 64); the head is M - tail_rows rows
  int tail_form;        // DU_TAIL_*: in the head's launch, the skinny kernels (one launch, or partial + finish through ws), the bf16 tile engine
  int tn_splits;        // family 5 (weight gradients): K splits
  int64_t ws_elems;     // scratch the product wants, whether or not it was passed: du_gemm_ws_elems / du_gemm_ks_ws_bytes
  int64_t ks_ws_bytes;
};

GemmPlan du_gemm_plan(const du_gemm_args& a);

// ---- each family's rules (pure host functions) and its launcher ----
// gemm_bf16.hip: the bf16 tile engine; rows of a tall NT product that should leave the tile grid
bool du_gemm_modes_served(int a_mode, int b_mode);
int du_gemm_bf16_tiles(const du_gemm_args& a, hipStream_t st);
int du_gemm_ragged_rows(const du_gemm_args& a);
// gemm_glds.hip
bool du_gemm_glds_serves(const du_gemm_args& a);
int du_gemm_nt_glds(const du_gemm_args& a, hipStream_t st);
// gemm_rk.hip
bool du_gemm_rk_serves(const du_gemm_args& a);
int du_gemm_nt_rk(const du_gemm_args& a, hipStream_t st);
// gemm_p8.hip: `choice` is du_gemm_p8_choice's (or 2 where only these kernels have the epilogue); tail_rows > 0 needs du_gemm_p8_tail_ok
bool p8_legal(const du_gemm_args& a);
int du_gemm_p8_choice(const du_gemm_args& a);
bool du_gemm_p8_tail_ok(const du_gemm_args& whole, int r);
long du_gemm_p8_ks_bytes(const du_gemm_args& a);
long du_gemm_p8_tail_bytes(const du_gemm_args& whole);
int du_gemm_nt_p8(const du_gemm_args& a, hipStream_t st, int choice, int tail_rows);
int du_gemm_tn_p8_splits(const du_gemm_args& a);
int du_gemm_tn_p8(const du_gemm_args& a, hipStream_t st, int splits);
// gemm_skinny.hip: `form` is du_gemm_skinny_form's: 0 = not served, DU_TAIL_SKINNY_FUSED, DU_TAIL_SKINNY_PAIR (needs a.ws)
int du_gemm_skinny_form(const du_gemm_args& a);
int64_t du_gemm_skinny_ws_elems(int N, int K);
int du_gemm_skinny(const du_gemm_args& a, hipStream_t st, int form);
