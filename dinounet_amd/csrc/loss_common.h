// Everything the fused segmentation losses share (loss.hip: Dice + CE with an ignore label, Dice + BCE for regions, deep supervision and
// their validation twins; loss_topk.hip: top-k CE and Dice + top-k): the 4-pixels-per-lane loads and stores, the softmax forward body of one
// pixel and the sigmoid bodies of one element (forward sums, backward gradient), the two stages of the sums, the finish arithmetic with the Dice coefficients, the
// class switch and the launch grids.  One copy of each: a kernel of the family chooses where its labels, its mask and its CE scale come
// from, never the arithmetic.  The exceptions are the four plain-label kernels at the top of loss.hip (dice_ce_partial / sum / coef /
// bwd_kernel), which keep their own one-pixel-per-lane bodies, sums layout and Dice-mean rounding; a later change can retire them in
// favour of the masked kernels with an ignore value no label takes, at the price of different result bits for the plain loss.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void ld4f(const float* __restrict__ p, bool vec, int n, float o[4]) {
  if (vec) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = j < n ? p[j] : 0.f;
  }
}
__device__ __forceinline__ void st4f(float* __restrict__ p, bool vec, int n, const float o[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < n) p[j] = o[j];
  }
}
__device__ __forceinline__ void ld4l(const int64_t* __restrict__ p, bool vec, int n, int64_t fill, int64_t o[4]) {
  if (vec) {
    const longlong2 a = reinterpret_cast<const longlong2*>(p)[0], b = reinterpret_cast<const longlong2*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = j < n ? p[j] : fill;
  }
}
// 4 uint8 of one plane in one dword (byte j = pixel j)
__device__ __forceinline__ uint32_t ld4b(const uint8_t* __restrict__ p, bool vec, int n) {
  if (vec) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) if (j < n) w |= (uint32_t)p[j] << (8 * j);
  return w;
}
__device__ __forceinline__ void st4b(uint8_t* __restrict__ p, bool vec, int n, uint32_t w) {
  if (vec) {
    *reinterpret_cast<uint32_t*>(p) = w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) if (j < n) p[j] = (uint8_t)(w >> (8 * j));
  }
}

// -log p_t of one pixel from the softmax pass: mx = max_k x_k, xt = the target's logit, se = sum_k exp(x_k - mx) in [1, K].  The order is
// log_softmax's: mx - xt is exact or rounds once at its own size and log se <= log K, so the error does not grow with a common offset
// of the logits ((mx + log se) - xt rounds at |mx|), and a target far below the maximum gives its gap, not a saturated -log of an
// underflowed p.  Every softmax body of the loss family goes through this one line.
__device__ __forceinline__ float softmax_nll(float mx, float xt, float se) { return (mx - xt) + __logf(se); }

// Softmax forward of one pixel: x = its K logits, t = its label, valid = it counts (not ignored, not the padding of a partial quad).
// Adds the pixel to the accumulator row [CE sum, n_valid, (I_c, P_c, G_c) c = 1..K-1] and returns its CE term.  The CE term is the
// caller's: ce_term(-log p_t) is valid ? nll : 0 in the Dice + CE losses, and the top-k loss clamps it to +0 as well.  Two things here
// are shaped by the compiler, which optimises this function alone before it inlines it: the pixel comes as its own array, not as slot j
// of the lane's quad (an index that is not a compile-time one in here keeps the whole quad in a vector alloca in the caller, +10 to 20
// VGPRs), and the CE term is added in here, in the statement order the kernels always had (added by the caller after the call, the
// log moves behind the Dice sums and the sums kernels of 6 and 8 classes lose a wave per SIMD).
template <int K, int NS, typename F>
__device__ __forceinline__ float softmax_pixel_fwd(const float (&x)[K], int64_t t, bool valid, float (&acc)[NS], F&& ce_term) {
  static_assert(NS == 2 + 3 * (K - 1), "accumulator row of the masked softmax sums");
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; k++) mx = fmaxf(mx, x[k]);
  float e[K], se = 0.f, xt = mx;
#pragma unroll
  for (int k = 0; k < K; k++) { e[k] = __expf(x[k] - mx); se += e[k]; if (k == t) xt = x[k]; }
  const float inv = 1.f / se;
  const float ce = ce_term(softmax_nll(mx, xt, se));
  acc[0] += ce;
  acc[1] += valid ? 1.f : 0.f;
#pragma unroll
  for (int k = 1; k < K; k++) {
    const float pk = e[k] * inv;
    const bool hit = valid && k == t;
    acc[2 + 3 * (k - 1)] += hit ? pk : 0.f;
    acc[2 + 3 * (k - 1) + 1] += valid ? pk : 0.f;
    acc[2 + 3 * (k - 1) + 2] += hit ? 1.f : 0.f;
  }
  return ce;
}

// The softmax BACKWARD of a pixel is not in here: dice_ce_masked_bwd_kernel, the softmax branch of ds_bwd_kernel and topk_bwd_kernel each
// keep the same text, which differs only in where the pixel's CE scale comes from.  Every shared form that was tried moved the
// compiler's choice of which products of (p - onehot) scale + p (g - p . g) and of the p . g chain it fuses (per pixel of the quad or
// packed over two classes) in the 3-class kernels, so their gradients differed from the un-shared text's in the last bit, or it cost
// the 5- to 8-class kernels a wave per SIMD.  A shared body needs that arithmetic pinned in the source first (explicit fused and
// unfused operations), which changes result bits once, for every class count.

// sigmoid and the stable BCE-with-logits from one exponential: e = exp(-|x|), bce = max(x, 0) - x y + log(1 + e).  The reciprocal is
// v_rcp_f32 (1 ulp; 1 + e lies in [1, 2]): an IEEE division is a ~10-instruction sequence per element, and at R elements per pixel it
// made the region kernels VALU-bound
__device__ __forceinline__ void sigmoid_bce(float x, float y, float& s, float& bce) {
  const float e = __expf(-fabsf(x));
  const float inv = __builtin_amdgcn_rcpf(1.f + e);
  s = x >= 0.f ? inv : e * inv;
  bce = fmaxf(x, 0.f) - x * y + __logf(1.f + e);
}

// Sigmoid forward of one element: logit x of region r, y = its target (0 / 1), m = its pixel counts.  Adds the BCE and the Dice triple of
// the region to the accumulator row [BCE sum, n_valid, (I_r, P_r, G_r) r < R]; n_valid is per pixel and stays with the caller.
template <int NS>
__device__ __forceinline__ void sigmoid_elem_fwd(float x, float y, bool m, int r, float (&acc)[NS]) {
  float s, bce;
  sigmoid_bce(x, y, s, bce);
  acc[0] += m ? bce : 0.f;
  acc[2 + 3 * r] += m ? s * y : 0.f;
  acc[2 + 3 * r + 1] += m ? s : 0.f;
  acc[2 + 3 * r + 2] += m ? y : 0.f;
}

// Sigmoid backward of the same element -> go d loss / d x = go ((s - y) bce_scale + (ca y + cb) s (1 - s)); the caller writes 0 where
// the pixel does not count
__device__ __forceinline__ float sigmoid_elem_bwd(float x, float y, float ca, float cb, float bce_scale, float go) {
  float s, bce;
  sigmoid_bce(x, y, s, bce);
  return go * ((s - y) * bce_scale + (ca * y + cb) * s * (1.f - s));
}

// the Dice backward coefficients of the N outputs from coef = [(ca_c, cb_c) c < CD]: CD = N for regions, N - 1 for softmax classes
// (class 0, the background, has no Dice term)
template <int N, int CD>
__device__ __forceinline__ void load_dice_coefs(const float* coef, float (&ca)[N], float (&cb)[N]) {
#pragma unroll
  for (int c = 0; c < N; c++) {
    const int q = c - (N - CD);
    ca[c] = q >= 0 ? coef[2 * q] : 0.f;
    cb[c] = q >= 0 ? coef[2 * q + 1] : 0.f;
  }
}

// first stage of a sums pass: the block's sum of every accumulator column (DPP wave tree, then waves 0..3); thread i < NS stores column
// i to *dst(i)
template <int NS, typename F>
__device__ __forceinline__ void block_columns_store(float (&acc)[NS], F&& dst) {
  __shared__ float red[4][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) *dst((int)threadIdx.x) = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
// ... to row blockIdx.x of the partial rows (blocks x NS)
template <int NS>
__device__ __forceinline__ void block_partial_store(float (&acc)[NS], float* __restrict__ part) {
  block_columns_store<NS>(acc, [&](int i) { return part + (long)blockIdx.x * NS + i; });
}

// second stage: ONE block adds the per-block partial rows (blocks x NS).  Every thread loads all NS columns of its rows at once, so the
// block waits for one memory round trip instead of NS dependent ones (dice_ce_sum_kernel of the plain loss walks the columns one at a
// time, with a strided load and an eight-barrier tree each: ~2 us per column, two thirds of a 512^2 batch-8 sums pass).  Fixed order
// (rows t, t + 256, ... per thread, then block_columns_store): bit-reproducible.
template <int NS>
__device__ __forceinline__ void thread_rows_sum(const float* __restrict__ part, int blocks, float (&acc)[NS]) {
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  for (int b = threadIdx.x; b < blocks; b += 256) {
    const float* row = part + (long)b * NS;
#pragma unroll
    for (int i = 0; i < NS; i++) acc[i] += row[i];
  }
}
template <int NS>
__global__ __launch_bounds__(256) void partial_rows_sum_kernel(const float* __restrict__ part, float* __restrict__ sums, int blocks) {
  float acc[NS];
  thread_rows_sum<NS>(part, blocks, acc);
  block_partial_store<NS>(acc, sums);     // gridDim.x == 1: row 0 of `sums`
}

// per-class dice coefficients shared by both configurations: loss -= mean_c dc_c; d loss / d q_c(pixel) = m (ca_c y_c + cb_c), q = the
// probability the dice terms see.  dc_c is summed before the division so an all-ignored batch gives exactly 1 (s / s) per class.
__device__ float dice_coefs(const float* __restrict__ s3, float* __restrict__ coef, int C, float smooth, float grad_mult) {
  float dc_sum = 0.f;
  const float invc = 1.f / (float)C;
  for (int c = 0; c < C; c++) {
    const float I = s3[3 * c], P = s3[3 * c + 1], G = s3[3 * c + 2];
    const float num = 2.f * I + smooth;
    const float raw = G + P + smooth;
    const float den = fmaxf(raw, 1e-8f);
    dc_sum += num / den;
    coef[2 * c] = -2.f * invc / den * grad_mult;
    coef[2 * c + 1] = (raw > 1e-8f ? num / (den * den) * invc : 0.f) * grad_mult;
  }
  return dc_sum / (float)C;
}

// The finish of one loss from its sums: ce_nv = [CE or BCE sum, n_valid], s3 = its C Dice triples, w = the weight folded into the
// backward coefficients (a deep-supervision scale's, else 1).  The CE / BCE scale is 1 / n_valid (per_elem: 1 / (n_valid C), the mean
// over every element of C regions), exactly 0 when nothing is valid.  coef <- [(ca_c, cb_c) c < C, scale] w; returns the loss.
__device__ __forceinline__ float loss_finish(const float* __restrict__ ce_nv, const float* __restrict__ s3, float* __restrict__ coef, int C,
                                             bool per_elem, float smooth, float grad_mult, float w) {
  const float dc = dice_coefs(s3, coef, C, smooth, grad_mult * w);
  const float nv = ce_nv[1];
  const float scale = nv > 0.f ? 1.f / (per_elem ? nv * (float)C : nv) : 0.f;
  coef[2 * C] = scale * w;
  return ce_nv[0] * scale - dc;
}

long quad_items(int B, int64_t HW) { return (long)B * ((HW + 3) / 4); }
// two quads per lane in the sums pass; the partial count is a function of the shape only (same reduction order on every call)
int masked_grid(long items) { long g = (items + 511) / 512; if (g < 1) g = 1; if (g > 2048) g = 2048; return (int)g; }
int elem_grid(long items) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > 8192) g = 8192; return (int)g; }
// the 4-pixel vector loads / stores: every row (plane of one image) starts on a 16 B (fp32, int64) / 4 B (uint8) boundary
bool al(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace

// CALL(n) for n = C in MIN..8 (MIN = 2: softmax classes, 1: regions): one kernel instantiation per count; any other C is unsupported
#define LOSS_SWITCH(C, MIN, CALL) \
  switch (C) { case 1: { if (MIN != 1) return DU_ERR_UNSUPPORTED; CALL(MIN); break; } \
               case 2: { CALL(2); break; } case 3: { CALL(3); break; } case 4: { CALL(4); break; } case 5: { CALL(5); break; } \
               case 6: { CALL(6); break; } case 7: { CALL(7); break; } case 8: { CALL(8); break; } default: return DU_ERR_UNSUPPORTED; }
