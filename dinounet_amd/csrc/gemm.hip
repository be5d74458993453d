// MFMA GEMM / implicit-convolution engine for gfx950.
//
//   C[m][n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )
//
// One kernel template serves every dense contraction of the Dino U-Net hot path: linear layers and 1x1 convs
// (PLAIN_ROW x PLAIN_ROW), their data gradients (PLAIN_ROW x PLAIN_COL), weight gradients (PLAIN_COL x PLAIN_COL,
// split-K + fp32 atomics), 3x3 / strided / transposed-stride convolutions as implicit GEMM (IM2COL_ROW gather of
// an NHWC tensor, optionally from two tensors = fused channel concat), conv weight gradients (PLAIN_COL x
// IM2COL_COL) and ConvTranspose2d k2s2 (GEMM + pixel-shuffle store).
//
// Tiling (wave64): 256 threads = WM x WN waves, each wave owns TM x TN MFMA tiles of 32x32
// (v_mfma_f32_32x32x16_bf16 for bf16 inputs, v_mfma_f32_32x32x2_f32 for the fp32 parity mode), fp32 accumulate.
// Operand tiles are staged global -> registers -> LDS as S[outer][k] (k contiguous, one 16-byte vector of
// padding per row); the next tile's global loads are issued before the current tile's MFMAs so HBM/L2 latency
// hides under the matrix pipe.
#include "common.h"
#include "gemm_params.h"
#include "gemm_plan.h"

namespace {

// ------------------------------------------------------------------------------------------------------------
// Tile loader: OUTER x BK tile of one operand -> registers -> LDS S[OUTER][BK + VEC]
// ------------------------------------------------------------------------------------------------------------
template <typename T, int MODE, int OUTER, int BK, int NT>
struct TileLoader {
  static constexpr int VEC = Elem<T>::VEC;
  static constexpr int LDS_LD = BK + VEC;
  static constexpr int TOTAL = OUTER * BK / VEC;
  static constexpr int NV = (TOTAL + NT - 1) / NT;
  static constexpr bool ROWMODE = (MODE == DU_PLAIN_ROW || MODE == DU_IM2COL_ROW);
  static constexpr int KV = BK / VEC;      // vectors per row (ROW modes)
  static constexpr int OV = OUTER / VEC;   // vectors per k-row (COL modes)

  uint4 regs[NV];
  // per-slot cached pixel coordinates for the IM2COL modes
  int pb[NV], py[NV], px[NV];

  __device__ __forceinline__ void init(const Operand& op, int tid, int o0, int outer_dim, int kbeg) {
    if constexpr (MODE == DU_IM2COL_ROW) {
#pragma unroll
      for (int i = 0; i < NV; i++) {
        int v = tid + i * NT;
        int o = o0 + v / KV;
        if (o >= outer_dim) o = outer_dim - 1;
        int xo = o % op.Wo; int t = o / op.Wo;
        px[i] = xo; py[i] = t % op.Ho; pb[i] = t / op.Ho;
      }
    } else if constexpr (MODE == DU_IM2COL_COL) {
#pragma unroll
      for (int i = 0; i < NV; i++) {
        int v = tid + i * NT;
        long pix = (long)kbeg + v / OV;
        int xo = pix % op.Wo; long t = pix / op.Wo;
        px[i] = xo; py[i] = (int)(t % op.Ho); pb[i] = (int)(t / op.Ho);
      }
    }
  }

  // advance cached pixel coordinates by BK pixels (IM2COL_COL: contraction runs over pixels)
  __device__ __forceinline__ void advance(const Operand& op) {
    if constexpr (MODE == DU_IM2COL_COL) {
#pragma unroll
      for (int i = 0; i < NV; i++) {
        px[i] += BK;
        while (px[i] >= op.Wo) { px[i] -= op.Wo; py[i]++; }
        while (py[i] >= op.Ho) { py[i] -= op.Ho; pb[i]++; }
      }
    }
  }

  __device__ __forceinline__ void load(const Operand& op, int tid, int o0, int outer_dim, int k0, int kend) {
#pragma unroll
    for (int i = 0; i < NV; i++) {
      int v = tid + i * NT;
      uint4 r = make_uint4(0, 0, 0, 0);
      if (TOTAL % NT == 0 || v < TOTAL) {
        if constexpr (MODE == DU_PLAIN_ROW) {
          int o = o0 + v / KV, k = k0 + (v % KV) * VEC;
          if (o < outer_dim && k < kend) r = *(const uint4*)((const T*)op.p + (long)o * op.ld + k);
        } else if constexpr (MODE == DU_PLAIN_COL) {
          int k = k0 + v / OV, o = o0 + (v % OV) * VEC;
          if (o < outer_dim && k < kend) r = *(const uint4*)((const T*)op.p + (long)k * op.ld + o);
        } else if constexpr (MODE == DU_IM2COL_ROW) {
          int o = o0 + v / KV, k = k0 + (v % KV) * VEC;
          if (o < outer_dim && k < kend) {
            const T* q = im2col_ptr<T>(op, pb[i], py[i], px[i], k);
            if (q) r = *(const uint4*)q;
          }
        } else {  // IM2COL_COL: row = pixel (contraction), column vector = (tap, ci..ci+VEC)
          int k = k0 + v / OV, o = o0 + (v % OV) * VEC;
          if (o < outer_dim && k < kend) {
            const T* q = im2col_ptr<T>(op, pb[i], py[i], px[i], o);
            if (q) r = *(const uint4*)q;
          }
        }
      }
      regs[i] = r;
    }
  }

  __device__ __forceinline__ void store(T* S, int tid) {
#pragma unroll
    for (int i = 0; i < NV; i++) {
      int v = tid + i * NT;
      if (TOTAL % NT == 0 || v < TOTAL) {
        if constexpr (ROWMODE) {
          int o = v / KV, kv = v % KV;
          *(uint4*)(S + o * LDS_LD + kv * VEC) = regs[i];
        } else {
          int k = v / OV, ov = v % OV;
          Vec16<T> e = as_vec<T>(regs[i]);
#pragma unroll
          for (int j = 0; j < VEC; j++) S[(ov * VEC + j) * LDS_LD + k] = e.v[j];
        }
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------------------
// MFMA micro-kernels
// ------------------------------------------------------------------------------------------------------------
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  static constexpr int K = 16;  // contraction per instruction
  typedef bf16x8 Frag;
  // lane l supplies row (l&31), k-slice (l>>5)*8 .. +8
  static __device__ __forceinline__ Frag load(const bf16_t* S, int ld, int row, int kk, int lane) {
    return *(const bf16x8*)(S + row * ld + kk * 16 + (lane >> 5) * 8);
  }
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  static constexpr int K = 2;
  typedef float Frag;
  // lane l supplies row (l&31), k = (l>>5)
  static __device__ __forceinline__ Frag load(const float* S, int ld, int row, int kk, int lane) {
    return S[row * ld + kk * 2 + (lane >> 5)];
  }
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }
};

template <typename T> struct TileK;
template <> struct TileK<bf16_t> { static constexpr int BK = 64; };
template <> struct TileK<float> { static constexpr int BK = 16; };

template <typename T, typename TC, int AMODE, int BMODE, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void gemm_kernel(GemmParams P) {
  constexpr int NT = 256;
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, BK = TileK<T>::BK;
  constexpr int VEC = Elem<T>::VEC;
  constexpr int LDS_LD = BK + VEC;
  static_assert(WM * WN == 4, "4 waves");
  __shared__ __attribute__((aligned(16))) T smem[(BM + BN) * LDS_LD];
  T* As = smem;
  T* Bs = smem + BM * LDS_LD;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tile = blockIdx.x;
  const int tm_idx = tile / P.tiles_n, tn_idx = tile % P.tiles_n;
  const int m0 = tm_idx * BM, n0 = tn_idx * BN;
  const int z = blockIdx.y;
  const int batch = z / P.split_k, split = z % P.split_k;
  const int kbeg = split * P.k_per_split;
  const int kend = min(P.K, kbeg + P.k_per_split);

  Operand opa = P.a, opb = P.b;
  opa.p = (const T*)opa.p + (long)batch * opa.bstride;
  opb.p = (const T*)opb.p + (long)batch * opb.bstride;

  TileLoader<T, AMODE, BM, BK, NT> la;
  TileLoader<T, BMODE, BN, BK, NT> lb;
  la.init(opa, tid, m0, P.M, kbeg);
  lb.init(opb, tid, n0, P.N, kbeg);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; i++)
#pragma unroll
    for (int j = 0; j < TN; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  const int nk = (kend - kbeg + BK - 1) / BK;
  if (nk > 0) {
    la.load(opa, tid, m0, P.M, kbeg, kend);
    lb.load(opb, tid, n0, P.N, kbeg, kend);
    la.store(As, tid);
    lb.store(Bs, tid);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const bool more = (kt + 1 < nk);
    if (more) {
      la.advance(opa); lb.advance(opb);
      la.load(opa, tid, m0, P.M, kbeg + (kt + 1) * BK, kend);
      lb.load(opb, tid, n0, P.N, kbeg + (kt + 1) * BK, kend);
    }
#pragma unroll
    for (int kk = 0; kk < BK / Mma<T>::K; kk++) {
      typename Mma<T>::Frag fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; i++) fa[i] = Mma<T>::load(As, LDS_LD, (wm * TM + i) * 32 + (lane & 31), kk, lane);
#pragma unroll
      for (int j = 0; j < TN; j++) fb[j] = Mma<T>::load(Bs, LDS_LD, (wn * TN + j) * 32 + (lane & 31), kk, lane);
#pragma unroll
      for (int i = 0; i < TM; i++)
#pragma unroll
        for (int j = 0; j < TN; j++) acc[i][j] = Mma<T>::mma(fa[i], fb[j], acc[i][j]);
    }
    __syncthreads();
    if (more) {
      la.store(As, tid);
      lb.store(Bs, tid);
    }
    __syncthreads();
  }

  // ---- epilogue: lane holds column (lane&31), rows (r&3) + 8*(r>>2) + 4*(lane>>5) of each 32x32 tile ----
  TC* Cb = (TC*)P.C + (long)batch * P.cbs;
  const TC* Rb = (const TC*)P.residual;
  if (Rb) Rb += (long)batch * P.cbs;
#pragma unroll
  for (int j = 0; j < TN; j++) {
    const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
    if (n >= P.N) continue;
    const float bias = P.bias ? P.bias[n] : 0.f;
    const float gam = P.gamma ? P.gamma[n] : 1.f;
    int ps_q = 0, ps_co = n;
    if (P.store_mode == DU_STORE_PIXEL_SHUFFLE2) { ps_q = n / P.ps_C; ps_co = n - ps_q * P.ps_C; }
#pragma unroll
    for (int i = 0; i < TM; i++) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= P.M) continue;
        float v = acc[i][j][r] * P.alpha;
        if (P.split_k > 1) { atomic_add_f32((float*)Cb + (long)m * P.ldc + n, v); continue; }
        v += bias;
        v = apply_act(v, P.act);
        v *= gam;
        if (P.row_scale) v *= P.row_scale[m / P.rs_rows];
        long off;
        if (P.store_mode == DU_STORE_PIXEL_SHUFFLE2) {
          int x = m % P.ps_W; int t = m / P.ps_W; int y = t % P.ps_H; int b = t / P.ps_H;
          off = (((long)b * 2 * P.ps_H + 2 * y + (ps_q >> 1)) * (2 * P.ps_W) + 2 * x + (ps_q & 1)) * P.ldc + ps_co;
        } else {
          off = (long)m * P.ldc + n;
        }
        if (Rb) v += to_f32(Rb[P.store_mode == DU_STORE_PIXEL_SHUFFLE2 ? (off / P.ldc) * P.ldr + ps_co : (long)m * P.ldr + n]);
        Cb[off] = from_f32<TC>(v);
      }
    }
  }
}

template <typename T, typename TC, int AMODE, int BMODE, int WM, int WN, int TM, int TN>
int launch_cfg(const du_gemm_args& a, hipStream_t st) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, BK = TileK<T>::BK;
  GemmParams P = make_params(a, AMODE, BMODE, BM, BN, BK);
  int tiles_m = (a.M + BM - 1) / BM;
  // when the caller asked for split-K but it collapsed to one split the epilogue must still accumulate
  // (C was zero-filled, no epilogue ops) -- plain store of alpha*acc is equivalent.
  dim3 grid(tiles_m * P.tiles_n, (a.batch < 1 ? 1 : a.batch) * P.split_k);
  hipLaunchKernelGGL((gemm_kernel<T, TC, AMODE, BMODE, WM, WN, TM, TN>), grid, dim3(256), 0, st, P);
  return du_check_launch();
}

template <typename T, typename TC, int AMODE, int BMODE>
int launch_modes(const du_gemm_args& a, hipStream_t st) {
  if (a.N <= 32) return launch_cfg<T, TC, AMODE, BMODE, 4, 1, 2, 1>(a, st);   // 256 x 32
  if (a.N <= 64) return launch_cfg<T, TC, AMODE, BMODE, 2, 2, 2, 1>(a, st);   // 128 x 64
  return launch_cfg<T, TC, AMODE, BMODE, 2, 2, 2, 2>(a, st);                   // 128 x 128
}

template <typename T, typename TC>
int launch_dtype(const du_gemm_args& a, hipStream_t st) {
  const int am = a.a_mode, bm = a.b_mode;
  if (am == DU_PLAIN_ROW && bm == DU_PLAIN_ROW) return launch_modes<T, TC, DU_PLAIN_ROW, DU_PLAIN_ROW>(a, st);
  if (am == DU_PLAIN_ROW && bm == DU_PLAIN_COL) return launch_modes<T, TC, DU_PLAIN_ROW, DU_PLAIN_COL>(a, st);
  if (am == DU_PLAIN_COL && bm == DU_PLAIN_COL) return launch_modes<T, TC, DU_PLAIN_COL, DU_PLAIN_COL>(a, st);
  if (am == DU_IM2COL_ROW && bm == DU_PLAIN_ROW) return launch_modes<T, TC, DU_IM2COL_ROW, DU_PLAIN_ROW>(a, st);
  if (am == DU_PLAIN_COL && bm == DU_IM2COL_COL) return launch_modes<T, TC, DU_PLAIN_COL, DU_IM2COL_COL>(a, st);
  return DU_ERR_UNSUPPORTED;
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the exact-fp32 / any-alignment engine above: bf16 or fp32 operands, fp32 results for fp32 operands
int launch_generic(const du_gemm_args& a, hipStream_t st) {
  if (a.dtype == DU_BF16) {
    if (a.out_dtype == DU_BF16) return launch_dtype<bf16_t, bf16_t>(a, st);
    return launch_dtype<bf16_t, float>(a, st);
  }
  return launch_dtype<float, float>(a, st);
}

// the last r rows of `a` as a product of their own; the head keeps the operands and M - r rows
void split_rows(const du_gemm_args& a, int r, du_gemm_args& head, du_gemm_args& tail) {
  const long m0 = a.M - r;
  const long osz = a.out_dtype == DU_BF16 ? 2 : 4;
  head = a;
  head.M = (int)m0;
  tail = a;
  tail.M = r;
  tail.A = (const char*)a.A + m0 * a.lda * 2;
  tail.C = (char*)a.C + m0 * a.ldc * osz;
  if (a.residual) tail.residual = (const char*)a.residual + m0 * a.ldr * osz;
  if (a.row_scale) tail.row_scale = a.row_scale + m0 / a.rs_rows;
}

// ---- the plan, step 1: which kernels run.  p.rc = DU_ERR_UNSUPPORTED where none does ----
void plan_kernels(const du_gemm_args& a, bool generic_only, GemmPlan& p) {
  p.rc = DU_OK;
  auto multi_phase = [&](const du_gemm_args& head, int choice, int riding) {     // gemm_p8.hip NT kernels (2 + choice = 7 is the resident-weights kernel)
    p.family = choice == 5 ? 8 : 2 + choice;
    p.variant = choice;
    p.gather = head.a_mode == DU_IM2COL_ROW;
    if (riding) { p.tail_rows = riding; p.tail_form = DU_TAIL_RIDES; }
  };
  // stores and the gate that exist in the multi-phase kernels' epilogues only: those kernels or nothing (callers fall back to a plain
  // product + du_msda_prep / du_qkv_rope_split / du_swiglu_pairs)
  if (a.store_mode == DU_STORE_MSDA_PREP || a.store_mode == DU_STORE_QKV_HEADS || a.store_mode == DU_STORE_QKV_ROPE) {
    p.rc = DU_ERR_UNSUPPORTED;
    if (a.dtype != DU_BF16 || a.a_mode != DU_PLAIN_ROW || a.b_mode != DU_PLAIN_ROW || a.split_k > 1) return;
    du_gemm_args head = a;
    int r = 0;
    if (a.store_mode == DU_STORE_QKV_HEADS) {      // head-major planes from the persistent kernel's drain: whole 256-row tiles, ragged rows in the same launch
      r = du_gemm_ragged_rows(a);
      head.M = a.M - r;
      if (head.M % 256) return;
    }
    const int c = du_gemm_p8_choice(head);
    if (c) { p.rc = DU_OK; multi_phase(head, c, r); }
    return;
  }
  if (a.act == DU_ACT_SWIGLU) {
    p.rc = DU_ERR_UNSUPPORTED;
    if (a.dtype != DU_BF16 || a.N % 2) return;
    int c = du_gemm_p8_choice(a);
    if (!c && p8_legal(a)) c = 2;      // the narrow tile where the heuristic would have preferred another family
    if (c) { p.rc = DU_OK; multi_phase(a, c, 0); }
    return;
  }
  // the bf16 kernel families: 16-byte epilogue vectors
  bool fast = a.dtype == DU_BF16 && !generic_only && a.N % 4 == 0 && a.ldc % 4 == 0 && aligned16(a.C) && a.c_batch_stride % 4 == 0;
  if (a.bias && !aligned16(a.bias)) fast = false;
  if (a.gamma && !aligned16(a.gamma)) fast = false;
  if (a.residual && (a.ldr % 4 || !aligned16(a.residual))) fast = false;
  if (a.store_mode == DU_STORE_PIXEL_SHUFFLE2 && a.ps_C % 4) fast = false;
  if (!fast) {
    if (!du_gemm_modes_served(a.a_mode, a.b_mode) || (a.dtype != DU_BF16 && a.out_dtype != DU_F32)) p.rc = DU_ERR_UNSUPPORTED;
    return;       // family 0
  }
  if (a.a_mode == DU_PLAIN_COL && (a.b_mode == DU_PLAIN_COL || a.b_mode == DU_IM2COL_COL)) {     // weight gradients: the multi-phase kernel where it is legal
    p.tn_splits = du_gemm_tn_p8_splits(a);
    if (p.tn_splits) { p.family = 5; p.gather = a.b_mode == DU_IM2COL_COL; return; }
  }
  if (du_gemm_rk_serves(a)) {        // K <= 256, tall M: the streaming kernel (any M: rows past the last full block are masked)
    p.family = 7; p.gather = a.a_mode == DU_IM2COL_ROW;
    return;
  }
  // large contraction-contiguous products: the multi-phase kernels where they pay, else the 128 x 128 direct-to-LDS kernel
  const int r = du_gemm_ragged_rows(a);
  if (r > 0 && a.ws && a.ws_elems >= du_gemm_skinny_ws_elems(a.N, a.K)) {
    // exact part on the tile kernels; the short ragged tail rides in a multi-phase kernel's launch (extra workgroups behind the tiles), or
    // runs on the K-parallel skinny kernels (gemm_skinny.hip) behind it
    // (forking the tail onto a side stream with event edges measured slower both times it was tried, inside the hipGraph: round 1 beside
    // the 128 x 128 kernels 191.6 vs 194.0 slices/s; round 2 beside the multi-phase kernels, 8 KB-LDS tail form, 33.9 vs 33.2 ms per step)
    du_gemm_args head, tail;
    split_rows(a, r, head, tail);
    const int c = du_gemm_p8_choice(head);
    if (c && du_gemm_p8_tail_ok(a, r)) { multi_phase(head, c, r); return; }
    if (c || du_gemm_glds_serves(head)) {
      if (c) multi_phase(head, c, 0); else p.family = 2;
      const int form = du_gemm_skinny_form(tail);
      p.tail_rows = r;
      p.tail_form = form ? form : DU_TAIL_TILE_ENGINE;
      return;
    }
  }
  const int c = du_gemm_p8_choice(a);
  if (c) { multi_phase(a, c, 0); return; }
  if (du_gemm_glds_serves(a)) { p.family = 2; return; }
  if (du_gemm_modes_served(a.a_mode, a.b_mode)) p.family = 1; else p.rc = DU_ERR_UNSUPPORTED;
}

// ---- step 2: the scratch the product wants (asked before any is passed: a.ws / a.ks_ws do not count) ----
int64_t plan_ks_bytes(const du_gemm_args& a) {
  if (a.dtype != DU_BF16 || a.a_mode != DU_PLAIN_ROW || a.b_mode != DU_PLAIN_ROW) return 0;
  du_gemm_args head = a;
  head.ks_ws = nullptr; head.ks_ws_bytes = 0;      // (the ragged-row rule must not depend on the scratch being asked about)
  int r = a.M % 256;
  if (r < 1 || r > 64 || !du_gemm_p8_tail_ok(a, r)) r = 0;
  head.M = a.M - r;
  const long pair = du_gemm_p8_ks_bytes(head);
  // (the sliced units exist in the one-shot tile kernels' launches: choice 1 / 2)
  const int c = r > 0 ? du_gemm_p8_choice(head) : 0;
  const long tail = (c == 1 || c == 2) ? du_gemm_p8_tail_bytes(a) : 0;
  return pair > tail ? pair : tail;
}

// ---- step 3: du_gemm's argument checks, in the order their codes take precedence; `family` is what step 1 chose ----
int plan_check(const du_gemm_args& a, int family) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return DU_ERR_BAD_ARG;
  if (!a.A || !a.B || !a.C) return DU_ERR_BAD_ARG;
  const int vec = a.dtype == DU_BF16 ? 8 : 4;
  if (a.dtype != DU_BF16 && a.dtype != DU_F32) return DU_ERR_BAD_ARG;
  if (a.out_dtype != DU_BF16 && a.out_dtype != DU_F32) return DU_ERR_BAD_ARG;
  // 16-byte vector access requirements
  if (!aligned16(a.A) || !aligned16(a.B)) return DU_ERR_BAD_ARG;
  auto chk = [&](int mode, long ld, int outer, long bs) {
    if (ld % vec || bs % vec) return false;
    if (mode == DU_PLAIN_ROW) return a.K % vec == 0;
    if (mode == DU_PLAIN_COL) return outer % vec == 0;
    return true;
  };
  if (!chk(a.a_mode, a.lda, a.M, a.a_batch_stride) || !chk(a.b_mode, a.ldb, a.N, a.b_batch_stride)) return DU_ERR_BAD_ARG;
  const bool a_i2c = (a.a_mode == DU_IM2COL_ROW), b_i2c = (a.b_mode == DU_IM2COL_COL);
  if (a_i2c || b_i2c) {
    const du_conv_geom& g = a.geom;
    if (g.C % vec || g.KH <= 0 || g.KW <= 0 || g.stride <= 0) return DU_ERR_BAD_ARG;
    if (g.p2 && (g.C1 % vec || g.ld2 % vec || !aligned16(g.p2))) return DU_ERR_BAD_ARG;
    if (a_i2c && a.K != g.KH * g.KW * g.C) return DU_ERR_BAD_ARG;
    if (b_i2c && a.N != g.KH * g.KW * g.C) return DU_ERR_BAD_ARG;
  }
  // weight-gradient form (A contraction-major): row_scale scales the CONTRACTION rows (per-sample DropPath scale on dY); only the bf16
  // tile engine implements it, and only for K tiles that lie inside one sample
  const bool k_scale = a.row_scale && a.a_mode == DU_PLAIN_COL;
  if (k_scale && (family != 1 || a.rs_rows <= 0 || a.rs_rows % 64 || a.bias || a.act || a.gamma || a.residual || a.store_mode)) return DU_ERR_UNSUPPORTED;
  if (a.split_k > 1 && (a.out_dtype != DU_F32 || a.bias || a.act || a.gamma || (a.row_scale && !k_scale) || a.residual ||
                        (a.store_mode && a.store_mode != DU_STORE_SLABS))) return DU_ERR_BAD_ARG;
  // one slab per K range instead of atomics: the bf16 tile engine's split-K epilogue only
  if (a.store_mode == DU_STORE_SLABS && (a.split_k <= 1 || a.batch > 1 || family != 1)) return DU_ERR_UNSUPPORTED;
  if (a.store_mode == DU_STORE_PIXEL_SHUFFLE2 && (a.ps_C <= 0 || a.N != 4 * a.ps_C || a.ps_H <= 0 || a.ps_W <= 0 || a.M % (a.ps_H * a.ps_W))) return DU_ERR_BAD_ARG;
  // bias-gradient side sums (a_colsum; b_colsum: ConvT, from the gathered dY operand): only the bf16 weight-gradient kernels accumulate them
  const bool wgrad = a.a_mode == DU_PLAIN_COL && (family == 1 || family == 5);
  if (a.b_colsum && (!wgrad || a.b_mode != DU_IM2COL_COL || a.geom.C <= 0 || a.N % a.geom.C)) return DU_ERR_UNSUPPORTED;
  if (a.a_colsum && !wgrad) return DU_ERR_UNSUPPORTED;
  return DU_OK;
}

}  // namespace

GemmPlan du_gemm_plan(const du_gemm_args& a) {
  static const bool generic_only = DU_GETENV("DU_GEMM_GENERIC") != nullptr;   // debugging aid: force the generic kernel
  GemmPlan p{};
  plan_kernels(a, generic_only, p);
  if (!generic_only) {
    p.ws_elems = du_gemm_ragged_rows(a) > 0 ? du_gemm_skinny_ws_elems(a.N, a.K) : 0;
    p.ks_ws_bytes = plan_ks_bytes(a);
  }
  const int rc = plan_check(a, p.family);
  if (rc != DU_OK) p.rc = rc;
  return p;
}

extern "C" int du_gemm_route(const du_gemm_args* pa) { return pa ? du_gemm_plan(*pa).family : DU_ERR_BAD_ARG; }
extern "C" int64_t du_gemm_ws_elems(const du_gemm_args* pa) { return pa ? du_gemm_plan(*pa).ws_elems : 0; }
extern "C" int64_t du_gemm_ks_ws_bytes(const du_gemm_args* pa) { return pa ? du_gemm_plan(*pa).ks_ws_bytes : 0; }

extern "C" int du_gemm_plan_describe(const du_gemm_args* pa, int64_t* out, int n) {
  if (!pa || !out || n < 9) return DU_ERR_BAD_ARG;
  const GemmPlan p = du_gemm_plan(*pa);
  const int64_t v[9] = {p.rc, p.family, p.variant, p.gather, p.tail_rows, p.tail_form, p.tn_splits, p.ws_elems, p.ks_ws_bytes};
  for (int i = 0; i < 9; i++) out[i] = v[i];
  return 9;
}

extern "C" int du_gemm(const du_gemm_args* pa, void* stream) {
  if (!pa) return DU_ERR_BAD_ARG;
  const GemmPlan p = du_gemm_plan(*pa);
  if (p.rc != DU_OK) return p.rc;
  hipStream_t st = (hipStream_t)stream;
  du_gemm_args head = *pa, tail = *pa;
  if (p.tail_rows) split_rows(*pa, p.tail_rows, head, tail);
  int rc;
  if (p.variant) rc = du_gemm_nt_p8(head, st, p.variant, p.tail_form == DU_TAIL_RIDES ? p.tail_rows : 0);
  else switch (p.family) {
    case 0: rc = launch_generic(head, st); break;
    case 1: rc = du_gemm_bf16_tiles(head, st); break;
    case 2: rc = du_gemm_nt_glds(head, st); break;
    case 5: rc = du_gemm_tn_p8(head, st, p.tn_splits); break;
    default: rc = du_gemm_nt_rk(head, st); break;      // 7
  }
  if (rc != DU_OK) return rc;
  switch (p.tail_form) {
    case DU_TAIL_SKINNY_FUSED: case DU_TAIL_SKINNY_PAIR: return du_gemm_skinny(tail, st, p.tail_form);
    case DU_TAIL_TILE_ENGINE: tail.ws = nullptr; tail.ws_elems = 0; return du_gemm_bf16_tiles(tail, st);
  }
  return rc;
}
