// Helpers shared by the fused segmentation losses (loss.hip: Dice + CE with an ignore label, Dice + BCE for regions, deep supervision;
// loss_topk.hip: top-k CE and Dice + top-k): the 4-pixels-per-lane loads and stores, the per-block partial row of a two-stage sum, the
// Dice coefficients and the launch grids.  One copy, so the Dice term of every loss is the same formula.
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

template <int NS>
__device__ __forceinline__ void block_partial_store(float (&acc)[NS], float* __restrict__ part) {
  __shared__ float red[4][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) part[(long)blockIdx.x * NS + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
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

long quad_items(int B, int64_t HW) { return (long)B * ((HW + 3) / 4); }
// two quads per lane in the sums pass; the partial count is a function of the shape only (same reduction order on every call)
int masked_grid(long items) { long g = (items + 511) / 512; if (g < 1) g = 1; if (g > 2048) g = 2048; return (int)g; }
int elem_grid(long items) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > 8192) g = 8192; return (int)g; }
// the 4-pixel vector loads / stores: every row (plane of one image) starts on a 16 B (fp32, int64) / 4 B (uint8) boundary
bool al(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace
