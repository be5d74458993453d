// LayerNorm backward whose incoming gradient is a narrow product: dy = bf16(G Wt^T), G (rows, K) bf16, Wt (D, K) bf16, D = 1024,
// K <= 256 -- the adapter's query_norm -> offsets | weights product (K = 192) and ffn_norm -> ConvFFN.fc1 (K = 256), dinov3/adapter.py.
// The unfused chain writes dy (rows x 1024 bf16, 88 MB at 43008 rows) with a data-gradient GEMM only for layernorm_bwd_fused_kernel
// (norm.hip) to read it back at once.  Here dy never leaves the CU.
//
// A workgroup (8 waves) owns a contiguous run of rows (LnProdPlan::rows_per_wg >= 64: no row's sums cross workgroups; kernel boundaries
// are the only synchronisation) and walks it in blocks of 64 rows.  Per block:
//   1. G's 64 x K block is staged into LDS (16-byte row-coalesced loads; 16-byte chunks XOR-swizzled by row & 7).
//   2. product: wave v forms columns [128 v, 128 v + 128) of the 64 x 1024 dy block in two passes of 64 columns, v_mfma_f32_32x32x16_bf16
//      fed with (Wt fragment, G fragment) as gemm_p8.hip does, so a lane holds ONE output row.  The Wt fragments come straight from
//      global memory (Wt is 384-512 KB: L2 resident, read once per block); Wt ROW perm(i) = 16 (i >> 2 & 1) + 4 (i >> 3) + (i & 3) is fed as
//      operand row i, which makes the lane's 16 accumulators 16 CONSECUTIVE columns: one rounding to bf16 and two ds_write_b128 per
//      32 x 32 block into the row-major dy block in LDS (chunks swizzled by row & 7).  The K-sum runs as in gemm_nt_rk_kernel and
//      gemm_nt_pp_kernel -- the kernels of the unfused data gradient at these shapes: k-steps of 16 in ascending order into one
//      accumulator, lane half h holding k = 16 s + 8 h -- so dy has the SAME BITS as the matrix those kernels write.
//   3. the row program of layernorm_bwd_fused_kernel on the same fp32 operations (ln_bwd_row.h), one wave per row, two rows of a wave at a time: x and dres from
//      global memory (16 bytes per lane, whole rows per wave; requested one row pair ahead, x of a block's first pair before its
//      product), dy from LDS; dx written the same way; every lane accumulates the dw / db terms of ITS columns over the rows its
//      wave visits.
// At the end the eight waves' column sums meet through LDS and leave as ONE partial row per workgroup, part[workgroup][D][2], the layout
// finalize_kernel (norm.hip) sums.
//
// LDS: dy block 64 x 1024 bf16 = 128 KB + G block 64 x K bf16 (24 / 32 KB) = 152 / 160 KB: one workgroup per CU, two waves per SIMD.
#include "common.h"
#include "ln_bwd_row.h"
#include "norm_gemm_plan.h"

int du_norm_finalize_planar(const float* part, float* out, int strips, int C, hipStream_t st);   // norm.hip

namespace {

constexpr int LP_D = 1024;          // the one row width served
constexpr int LP_BM = 64;           // rows per block
constexpr int LP_WGS = 256;         // workgroups a large launch is cut into: one per CU of the MI355X
constexpr int LP_DY_BYTES = LP_BM * LP_D * 2;

struct LnProdParams {
  const bf16_t* x; const bf16_t* G; const bf16_t* Wt; const bf16_t* dres; bf16_t* dx;
  const float* w; const float* mean; const float* rstd; float* part;
  long rows, ldg, ldw;
  int rows_per_wg;
};

template <int KT>     // K = 64 KT
__global__ __launch_bounds__(512) void layernorm_bwd_prod_kernel(const LnProdParams P) {
  constexpr int K = 64 * KT, KC = K / 8, D = LP_D, VI = 8, MAXV = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char lp_smem[];
  bf16_t* dyl = (bf16_t*)lp_smem;                          // [64][1024], 16-byte chunk c of row r at chunk c ^ (r & 7)
  bf16_t* gl = (bf16_t*)(lp_smem + LP_DY_BYTES);           // [64][K], likewise
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: row addresses are SGPR bases + one lane offset
  const int lr = lane & 31, lh = lane >> 5;
  const long r_begin = (long)blockIdx.x * P.rows_per_wg;
  const long r_end = r_begin + P.rows_per_wg < P.rows ? r_begin + P.rows_per_wg : P.rows;
  float wv[MAXV][VI], sa[MAXV][VI], sb[MAXV][VI];
#pragma unroll
  for (int i = 0; i < MAXV; i++) {
    const int vi = lane + i * 64;
#pragma unroll
    for (int j = 0; j < VI; j++) { wv[i][j] = P.w[vi * VI + j]; sa[i][j] = 0.f; sb[i][j] = 0.f; }
  }
  const int wperm = 16 * ((lr >> 2) & 1) + 4 * (lr >> 3) + (lr & 3);      // Wt row (inside a 32-column block) this lane feeds
  const int ldg = (int)P.ldg, ldw = (int)P.ldw;
  const unsigned woff = (unsigned)(wperm * ldw + 8 * lh);                 // ... and its first element there
  // the row pair (l0, l0 + 8) of the block at b0: x and the statistics (and dres), requested ahead of their use
  uint4 nx[2][MAXV], nr[2][MAXV];
  float nmu[2], nrs[2];
  auto request = [&](long b0, int nrows, int l0, bool with_dres) {
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int l = l0 + 8 * u;
      const bool live = l < nrows;
      const long row = b0 + l;
      nmu[u] = live ? P.mean[row] : 0.f; nrs[u] = live ? P.rstd[row] : 0.f;
#pragma unroll
      for (int i = 0; i < MAXV; i++) {
        const int vi = lane + i * 64;
        nx[u][i] = make_uint4(0, 0, 0, 0);
        if (live) nx[u][i] = *(const uint4*)((P.x + row * (long)D) + (unsigned)(vi * VI));
        if (with_dres) {
          nr[u][i] = make_uint4(0, 0, 0, 0);
          if (live && P.dres) nr[u][i] = *(const uint4*)((P.dres + row * (long)D) + (unsigned)(vi * VI));
        }
      }
    }
  };
  // rows l0 and l0 + 8 of the block at b0, their dy in LDS: the row terms, dx, and this lane's share of the column sums -- the row
  // program of layernorm_bwd_fused_kernel (norm.hip) on the shared fp32 operations of ln_bwd_row.h: the same dy gives the same dx bits
  auto process = [&](long b0, int nrows, int l0, const uint4 (&rx)[2][MAXV], const uint4 (&rr)[2][MAXV], const float (&mu)[2], const float (&rs)[2]) {
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int l = l0 + 8 * u;
      if (l >= nrows) break;
      const long row = b0 + l;
      float xh[MAXV][VI], g[MAXV][VI];
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int i = 0; i < MAXV; i++) {
        const int vi = lane + i * 64;
        ln_bwd_row_terms<bf16_t>(rx[u][i], *(const uint4*)(dyl + l * D + ((vi ^ (l & 7)) << 3)), mu[u], rs[u], wv[i], xh[i], g[i], c1, c2, sa[i], sb[i]);
      }
      c1 = wave_sum(c1) / (float)D;
      c2 = wave_sum(c2) / (float)D;
#pragma unroll
      for (int i = 0; i < MAXV; i++) {
        const int vi = lane + i * 64;
        uint4 o;
        if (P.dres) o = ln_bwd_row_dx<bf16_t, true>(xh[i], g[i], c1, c2, rs[u], rr[u][i]);
        else o = ln_bwd_row_dx<bf16_t, false>(xh[i], g[i], c1, c2, rs[u], rr[u][i]);
        *(uint4*)((P.dx + row * (long)D) + (unsigned)(vi * VI)) = o;
      }
    }
  };
  request(r_begin, (int)(r_end - r_begin < LP_BM ? r_end - r_begin : LP_BM), wave, false);
  for (long b0 = r_begin; b0 < r_end; b0 += LP_BM) {
    const int nrows = (int)(r_end - b0 < LP_BM ? r_end - b0 : LP_BM);
    // ---- 1. G block -> LDS (rows past the block read as zeros) ----
    const bf16_t* gbase = P.G + b0 * P.ldg;             // (scalar base + a 32-bit lane offset: LnProdPlan bounds ldg and ldw)
    int stid = tid;
    asm volatile("" : "+v"(stid));        // the staging offsets are recomputed per block: hoisted, they are eight more live registers
#pragma unroll
    for (int i = 0; i < LP_BM * KC / 512; i++) {
      const int idx = stid + i * 512, row = idx / KC, c = idx - row * KC;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < nrows) v = *(const uint4*)(gbase + (unsigned)(row * ldg + c * 8));
      *(uint4*)(gl + row * K + ((c ^ (row & 7)) << 3)) = v;
    }
    __syncthreads();
    // ---- 2. dy block = bf16(G Wt^T) -> LDS ----
    const bool two = nrows > 32;          // the second 32-row half holds live rows (uniform over the workgroup)
#pragma unroll 1
    for (int sp = 0; sp < 2; sp++) {
      const int nb = wave * 128 + sp * 64;
      f32x16 acc[2][2];
#pragma unroll
      for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int e = 0; e < 16; e++) acc[mb][j][e] = 0.f;
      const bf16_t* wrow0 = P.Wt + (long)nb * P.ldw + woff;
      const bf16_t* wrow1 = wrow0 + 32 * P.ldw;
#pragma unroll
      for (int t = 0; t < KT; t++) {
        bf16x8 bw[2][4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          bw[0][s] = *(const bf16x8*)(wrow0 + 64 * t + 16 * s);
          bw[1][s] = *(const bf16x8*)(wrow1 + 64 * t + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int c = 8 * t + 2 * s + lh;
          const bf16x8 g0 = *(const bf16x8*)(gl + lr * K + ((c ^ (lr & 7)) << 3));
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[0][s], g0, acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[1][s], g0, acc[0][1], 0, 0, 0);
          if (two) {
            const bf16x8 g1 = *(const bf16x8*)(gl + (32 + lr) * K + ((c ^ (lr & 7)) << 3));
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[0][s], g1, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[1][s], g1, acc[1][1], 0, 0, 0);
          }
        }
      }
      // register e of the lane = column nb + 32 j + 16 lh + e of row 32 mb + lr: the ONE rounding to bf16, two 16-byte pieces
#pragma unroll
      for (int mb = 0; mb < 2; mb++) {
        const int m = 32 * mb + lr;
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int q = 0; q < 2; q++) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] = (bf16_t)acc[mb][j][8 * q + e];
            const int cc = ((nb + 32 * j + 16 * lh) >> 3) + q;
            *(bf16x8*)(dyl + m * D + ((cc ^ (m & 7)) << 3)) = o;
          }
      }
    }
    __syncthreads();
    // ---- 3. layernorm_bwd_fused_kernel's row program; wave v takes rows v, v + 8, ... of the block, two at a time.  A pair's x and
    // statistics were requested a pair ahead -- the block's first pair before the product, so its HBM latency passes under the MFMAs;
    // its dres is requested here (sixteen registers the product has no room for), the later pairs' dres with their x ----
    if (wave < nrows) {
      uint4 rx[2][MAXV], rr[2][MAXV];
      float mu[2], rs[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        mu[u] = nmu[u]; rs[u] = nrs[u];
        const int l = wave + 8 * u;
#pragma unroll
        for (int i = 0; i < MAXV; i++) {
          rx[u][i] = nx[u][i];
          rr[u][i] = make_uint4(0, 0, 0, 0);
          if (P.dres && l < nrows) rr[u][i] = *(const uint4*)((P.dres + (b0 + l) * (long)D) + (unsigned)((lane + i * 64) * VI));
        }
      }
      if (wave + 16 < nrows) request(b0, nrows, wave + 16, true);
      else if (b0 + LP_BM < r_end) request(b0 + LP_BM, (int)(r_end - b0 - LP_BM < LP_BM ? r_end - b0 - LP_BM : LP_BM), wave, false);
      process(b0, nrows, wave, rx, rr, mu, rs);
    }
    for (int l0 = wave + 16; l0 < nrows; l0 += 16) {
      uint4 rx[2][MAXV], rr[2][MAXV];
      float mu[2], rs[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        mu[u] = nmu[u]; rs[u] = nrs[u];
#pragma unroll
        for (int i = 0; i < MAXV; i++) { rx[u][i] = nx[u][i]; rr[u][i] = nr[u][i]; }
      }
      if (l0 + 16 < nrows) request(b0, nrows, l0 + 16, true);
      else if (b0 + LP_BM < r_end) request(b0 + LP_BM, (int)(r_end - b0 - LP_BM < LP_BM ? r_end - b0 - LP_BM : LP_BM), wave, false);
      process(b0, nrows, l0, rx, rr, mu, rs);
    }
    __syncthreads();        // the next block's G and dy overwrite what this one read
  }
  // ---- the eight waves' column sums -> one partial row of this workgroup ----
  float* red = (float*)lp_smem;                           // [7][D][2]: the sums of waves 1-7 (56 KB of the dy block's space)
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < MAXV; i++) {
      const int vi = lane + i * 64;
#pragma unroll
      for (int j = 0; j < VI; j += 2)
        *(float4*)(red + ((long)(wave - 1) * D + vi * VI + j) * 2) = make_float4(sa[i][j], sb[i][j], sa[i][j + 1], sb[i][j + 1]);
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < MAXV; i++) {
      const int vi = lane + i * 64;
#pragma unroll
      for (int j = 0; j < VI; j += 2) {
        float4 t = make_float4(sa[i][j], sb[i][j], sa[i][j + 1], sb[i][j + 1]);
#pragma unroll
        for (int q = 0; q < 7; q++) {
          const float4 u = *(const float4*)(red + ((long)q * D + vi * VI + j) * 2);
          t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        *(float4*)(P.part + ((long)blockIdx.x * D + vi * VI + j) * 2) = t;
      }
    }
  }
}

template <int KT>
int lp_launch(const LnProdPlan& plan, const LnProdParams& P, hipStream_t st) {
  auto kfn = layernorm_bwd_prod_kernel<KT>;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, plan.lds_bytes) != hipSuccess) return DU_ERR_LAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)plan.wgs), dim3(512), (size_t)plan.lds_bytes, st, P);
  return du_check_launch();
}

}  // namespace

// The only place that decides whether a call is served and how it is cut.  A pure host function of the call's numbers (pointers are
// looked at for their alignment only).
LnProdPlan du_ln_bwd_prod_plan(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K, const void* dx,
                               const void* dres, int64_t rows, int D) {
  LnProdPlan p = {};
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  p.rc = DU_ERR_UNSUPPORTED;
  if (rows <= 0 || D <= 0 || K <= 0 || !x || !G || !Wt || !dx) { p.rc = DU_ERR_BAD_ARG; return p; }
  if (dtype != DU_BF16 || D != LP_D) return p;
  if (K % 64 != 0 || K > 256) return p;
  if (ldg < K || ldw < K || ldg % 8 != 0 || ldw % 8 != 0) return p;
  if (!al16(x) || !al16(G) || !al16(Wt) || !al16(dx) || !al16(dres)) return p;
  if (rows > (int64_t)LP_WGS * 65536 || ldg > 65536 || ldw > 65536) return p;      // (32-bit lane offsets inside a block)
  p.rc = DU_OK;
  p.served = 1;
  p.block_rows = LP_BM;
  int64_t per = (rows + LP_WGS - 1) / LP_WGS;
  if (per < LP_BM) per = LP_BM;
  p.rows_per_wg = (int)per;
  p.wgs = (int)((rows + per - 1) / per);
  p.ws_elems = (int64_t)p.wgs * LP_D * 2;
  p.lds_bytes = LP_DY_BYTES + LP_BM * K * 2;
  return p;
}

extern "C" int du_layernorm_bwd_prod_plan(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K,
                                          const void* dx, const void* dres, int64_t rows, int D, int64_t* out, int n) {
  if (!out || n < 6) return DU_ERR_BAD_ARG;
  const LnProdPlan p = du_ln_bwd_prod_plan(dtype, x, G, ldg, Wt, ldw, K, dx, dres, rows, D);
  out[0] = p.served; out[1] = p.block_rows; out[2] = p.wgs; out[3] = p.rows_per_wg; out[4] = p.ws_elems; out[5] = p.lds_bytes;
  return 6;
}

extern "C" int du_layernorm_bwd_prod(int dtype, const void* x, const void* G, int64_t ldg, const void* Wt, int64_t ldw, int K, const float* w,
                                     const float* mean, const float* rstd, void* dx, float* dwdb, int64_t rows, int D, float* ws,
                                     int64_t ws_elems, const void* dres, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const LnProdPlan plan = du_ln_bwd_prod_plan(dtype, x, G, ldg, Wt, ldw, K, dx, dres, rows, D);
  if (plan.rc != DU_OK) return plan.rc;
  if (!w || !mean || !rstd || !dwdb || !ws || ws_elems < plan.ws_elems) return DU_ERR_BAD_ARG;
  LnProdParams P;
  P.x = (const bf16_t*)x; P.G = (const bf16_t*)G; P.Wt = (const bf16_t*)Wt; P.dres = (const bf16_t*)dres; P.dx = (bf16_t*)dx;
  P.w = w; P.mean = mean; P.rstd = rstd; P.part = ws;
  P.rows = rows; P.ldg = ldg; P.ldw = ldw; P.rows_per_wg = plan.rows_per_wg;
  int rc;
  switch (K / 64) {
    case 1: rc = lp_launch<1>(plan, P, st); break;
    case 2: rc = lp_launch<2>(plan, P, st); break;
    case 3: rc = lp_launch<3>(plan, P, st); break;
    default: rc = lp_launch<4>(plan, P, st); break;
  }
  if (rc != DU_OK) return rc;
  return du_norm_finalize_planar(ws, dwdb, plan.wgs, D, st);      // planar dw[D] then db[D], as du_layernorm_bwd with scratch
}
