// Export tail of the sliding-window predictor: the accumulators of du_window_accumulate_cases go straight to the label map of the
// case's original geometry, and two label maps go to the per-case counts.
//   convert_predicted_logits_to_segmentation_with_correct_shape (dinounet/inference/export_prediction.py:15-68):
//     resample the logits in-plane to shape_after_cropping_and_before_resampling (order 1, edge clamp, half-pixel centres),
//     softmax + argmax / sigmoid + region paint loop (label_handling.py:128-175), paste into shape_before_cropping at the bbox (:44-48),
//     probabilities with the background convention outside the bbox (label_handling.py:185-209).
//   compute_metrics (dinounet/evaluation/evaluate_predictions.py:75-94, 176-186): tp / fp / fn / tn per label or region.
// Both are streaming passes.  du_export_seg reads 4 K bytes per window voxel (+ 4 for n_predictions where the normalised value is needed:
// resampling or probabilities) and writes 1 byte per output voxel (+ 4 K with probabilities); the normalised logits are never stored.
// du_seg_counts reads 2 bytes per voxel.  No float atomics; the counts are integers, two stages, fixed order.
#include "common.h"

namespace {

constexpr int MAXC = 8;

struct ExportGeom {
  int D, Hp, Wp;          // accumulator planes
  int y0, x0, Hc, Wc;     // un-padding window inside (Hp, Wp)
  int Ho, Wo;             // in-plane size after resampling = bbox size
  int D0, H0, W0;         // destination volume
  int bd, by, bx;         // low corner of the bbox in the destination
  int pad, nq;            // a row is cut into nq quads of 4 columns starting at column -pad: the quads' source columns start on multiples of 4
};

__device__ __forceinline__ bool finite_f(float x) { return __builtin_isfinite(x); }

// order-1 source position of output index `dst` from integers: n = (2 dst + 1) S - O, tap floor(n / 2O), weight (n mod 2O) / 2O with one
// rounded division; taps clamped to [0, S - 1].  n > -2O, so the floor is -1 exactly when n < 0.
__device__ __forceinline__ void src_taps(int dst, int S, int O, int& a, int& b, float& w) {
  const long n = (2L * dst + 1) * S - O, den = 2L * O;
  long i, rem;
  if (n < 0) { i = -1; rem = n + den; } else { i = n / den; rem = n - i * den; }
  w = (float)rem / (float)den;
  a = i < 0 ? 0 : (int)i;
  b = i + 1 > S - 1 ? S - 1 : (int)(i + 1);
}

// One lane: 4 adjacent output columns of one output row.  C = classes (softmax, argmax with the lowest index among equal maxima) or
// regions (REGION: label order[i] of the LARGEST i with logit_i > 0, else 0).  !RESAMPLE: the label comes from the raw sums (the positive
// factor 1 / n_predictions changes neither the argmax nor a sign); RESAMPLE: from the 4-tap interpolation of sums / n_predictions.
// flag = 1 when a value read for a window voxel is not finite (same value from every lane that sees one: a plain store).
template <int C, bool REGION, bool RESAMPLE>
__global__ __launch_bounds__(256) void export_seg_kernel(const float* __restrict__ sums, const float* __restrict__ npred,
                                                         uint8_t* __restrict__ seg, float* __restrict__ probs, int* __restrict__ flag,
                                                         ExportGeom g, uint64_t order, bool vec_in, bool vec_seg, bool vec_probs) {
  const long plane_in = (long)g.D * g.Hp * g.Wp, plane_out = (long)g.D0 * g.H0 * g.W0;
  const long items = (long)g.D0 * g.H0 * g.nq;
  bool bad = false;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long row = it / g.nq;
    const int q = (int)(it - row * g.nq);
    const int d = (int)(row / g.H0), y = (int)(row - (long)d * g.H0);
    const int xs = 4 * q - g.pad;
    const int dd = d - g.bd, yo = y - g.by;
    const bool row_in = dd >= 0 && dd < g.D && yo >= 0 && yo < g.Ho;
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int xo = xs + j - g.bx; in[j] = row_in && xo >= 0 && xo < g.Wo; }
    float v[C][4];
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
      for (int j = 0; j < 4; j++) v[c][j] = 0.f;
    float nrm[4] = {1.f, 1.f, 1.f, 1.f};

    if constexpr (!RESAMPLE) {
      // bbox size == window size: output column x reads window column x - bx, accumulator column x0 + x - bx
      const long src = row_in ? ((long)dd * g.Hp + g.y0 + yo) * g.Wp + g.x0 + (xs - g.bx) : 0;
      const bool full = in[0] && in[3];
      if (full && vec_in) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          const float4 t = *reinterpret_cast<const float4*>(sums + c * plane_in + src);
          v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        }
        if (probs && npred) {
          const float4 t = *reinterpret_cast<const float4*>(npred + src);
          nrm[0] = t.x; nrm[1] = t.y; nrm[2] = t.z; nrm[3] = t.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (in[j]) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c][j] = sums[c * plane_in + src + j];
            if (probs && npred) nrm[j] = npred[src + j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bad |= !finite_f(nrm[j]);
#pragma unroll
        for (int c = 0; c < C; c++) bad |= !finite_f(v[c][j]);
      }
    } else {
      if (row_in) {
        int ya, yb;
        float wy;
        src_taps(yo, g.Hc, g.Ho, ya, yb, wy);
        const long ra = ((long)dd * g.Hp + g.y0 + ya) * g.Wp + g.x0, rb = ((long)dd * g.Hp + g.y0 + yb) * g.Wp + g.x0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (in[j]) {
            int xa, xb;
            float wx;
            src_taps(xs + j - g.bx, g.Wc, g.Wo, xa, xb, wx);
            float n00 = 1.f, n01 = 1.f, n10 = 1.f, n11 = 1.f;
            if (npred) { n00 = npred[ra + xa]; n01 = npred[ra + xb]; n10 = npred[rb + xa]; n11 = npred[rb + xb]; }
            bad |= !(finite_f(n00) && finite_f(n01) && finite_f(n10) && finite_f(n11));
#pragma unroll
            for (int c = 0; c < C; c++) {
              const float* p = sums + c * plane_in;
              const float s00 = p[ra + xa], s01 = p[ra + xb], s10 = p[rb + xa], s11 = p[rb + xb];
              bad |= !(finite_f(s00) && finite_f(s01) && finite_f(s10) && finite_f(s11));
              const float a = s00 / n00, b = s01 / n01, cc = s10 / n10, e = s11 / n11;
              const float top = fmaf(wx, b - a, a), bot = fmaf(wx, e - cc, cc);
              v[c][j] = fmaf(wy, bot - top, top);
            }
          }
        }
      }
    }

    uint32_t lab = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int l = 0;
      if constexpr (REGION) {
#pragma unroll
        for (int c = 0; c < C; c++) if (v[c][j] > 0.f) l = (int)((order >> (8 * c)) & 0xffull);
      } else {
        float best = v[0][j];
#pragma unroll
        for (int c = 1; c < C; c++) if (v[c][j] > best) { best = v[c][j]; l = c; }
      }
      lab |= in[j] ? ((uint32_t)l << (8 * j)) : 0u;
    }
    uint8_t* sp = seg + row * g.W0 + xs;
    if (vec_seg) {
      *reinterpret_cast<uint32_t*>(sp) = lab;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (xs + j >= 0 && xs + j < g.W0) sp[j] = (uint8_t)(lab >> (8 * j));
    }

    if (probs) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (in[j]) {
          if constexpr (!RESAMPLE) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c][j] = v[c][j] / nrm[j];
          }
          if constexpr (REGION) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c][j] = 1.f / (1.f + expf(-v[c][j]));
          } else {
            float mx = v[0][j];
#pragma unroll
            for (int c = 1; c < C; c++) mx = fmaxf(mx, v[c][j]);
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < C; c++) { v[c][j] = expf(v[c][j] - mx); se += v[c][j]; }
#pragma unroll
            for (int c = 0; c < C; c++) v[c][j] = v[c][j] / se;
          }
        } else {
          // revert_cropping_on_probabilities: background probability 1 outside the bbox (softmax), all 0 (regions)
#pragma unroll
          for (int c = 0; c < C; c++) v[c][j] = (!REGION && c == 0) ? 1.f : 0.f;
        }
      }
      float* pp = probs + row * g.W0 + xs;
#pragma unroll
      for (int c = 0; c < C; c++) {
        if (vec_probs) {
          *reinterpret_cast<float4*>(pp + c * plane_out) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) if (xs + j >= 0 && xs + j < g.W0) pp[c * plane_out + j] = v[c][j];
        }
      }
    }
  }
  if (bad) *flag = 1;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Stage 1 of the per-case counts: per region three int32 lane counters (hits, predicted, labelled) and one for the valid voxels, over
// 16 voxels per lane and step; added over the wave and the block as integers into one row of 3R + 1 int32 per block.
template <int R>
__global__ __launch_bounds__(256) void seg_counts_partial_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ ref,
                                                                 const int64_t* __restrict__ masks, int* __restrict__ cpart, long n,
                                                                 int has_ignore, int ignore, bool vec) {
  constexpr int NC = 3 * R + 1;
  uint64_t tb[R];
#pragma unroll
  for (int r = 0; r < R; r++) tb[r] = (uint64_t)masks[r];
  int cnt[NC];
#pragma unroll
  for (int i = 0; i < NC; i++) cnt[i] = 0;
  const long items = (n + 15) >> 4;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long base = it << 4;
    const int m = (int)(n - base < 16 ? n - base : 16);
    uint32_t pw[4] = {0u, 0u, 0u, 0u}, gw[4] = {0u, 0u, 0u, 0u};
    if (vec && m == 16) {
      const uint4 a = *reinterpret_cast<const uint4*>(pred + base), b = *reinterpret_cast<const uint4*>(ref + base);
      pw[0] = a.x; pw[1] = a.y; pw[2] = a.z; pw[3] = a.w;
      gw[0] = b.x; gw[1] = b.y; gw[2] = b.z; gw[3] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if (j < m) {
          pw[j >> 2] |= (uint32_t)pred[base + j] << (8 * (j & 3));
          gw[j >> 2] |= (uint32_t)ref[base + j] << (8 * (j & 3));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t pl = (pw[j >> 2] >> (8 * (j & 3))) & 255u, gl = (gw[j >> 2] >> (8 * (j & 3))) & 255u;
      const int valid = (j < m && !(has_ignore && (int)gl == ignore)) ? 1 : 0;
      cnt[3 * R] += valid;
#pragma unroll
      for (int r = 0; r < R; r++) {
        const int p = (pl < 64u && ((tb[r] >> pl) & 1ull)) ? valid : 0;
        const int t = (gl < 64u && ((tb[r] >> gl) & 1ull)) ? valid : 0;
        cnt[r] += p & t;
        cnt[R + r] += p;
        cnt[2 * R + r] += t;
      }
    }
  }
  __shared__ int cred[4][NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NC; i++) {
    const int s = wave_sum_i32(cnt[i]);
    if (lane == 0) cred[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NC) cpart[(long)blockIdx.x * NC + threadIdx.x] = (cred[0][threadIdx.x] + cred[1][threadIdx.x]) + (cred[2][threadIdx.x] + cred[3][threadIdx.x]);
}

// Stage 2: ONE block adds the rows in int64, fixed order; counts (4, R) = tp | fp | fn | tn
__global__ __launch_bounds__(256) void seg_counts_sum_kernel(const int* __restrict__ cpart, int64_t* __restrict__ counts, int blocks, int R) {
  __shared__ long long red[3 * MAXC + 1][4];
  __shared__ long long tot[3 * MAXC + 1];
  const int NC = 3 * R + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < NC; i++) {
    long long a = 0;
    for (int b = threadIdx.x; b < blocks; b += 256) a += (long long)cpart[(long)b * NC + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) red[i][wave] = a;
  }
  __syncthreads();
  if (threadIdx.x < NC) tot[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
  __syncthreads();
  if (threadIdx.x < R) {
    const int r = threadIdx.x;
    const long long h = tot[r], p = tot[R + r], t = tot[2 * R + r], valid = tot[3 * R];
    counts[r] = (int64_t)h;
    counts[R + r] = (int64_t)(p - h);
    counts[2 * R + r] = (int64_t)(t - h);
    counts[3 * R + r] = (int64_t)(valid - p - t + h);
  }
}

int export_grid(long items) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > 4096) g = 4096; return (int)g; }
// 16 voxels per lane; the partial count is a function of n only (same reduction order on every call)
int counts_grid(int64_t n) { long g = (((long)n + 15) / 16 + 255) / 256; if (g < 1) g = 1; if (g > 1024) g = 1024; return (int)g; }
bool aligned_to(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace

#define EXPORT_C_SWITCH(C, CALL) \
  switch (C) { case 1: { CALL(1); break; } case 2: { CALL(2); break; } case 3: { CALL(3); break; } case 4: { CALL(4); break; } \
               case 5: { CALL(5); break; } case 6: { CALL(6); break; } case 7: { CALL(7); break; } case 8: { CALL(8); break; } \
               default: return DU_ERR_UNSUPPORTED; }

extern "C" int du_export_seg(const float* sums, const float* npred, uint8_t* seg, float* probs, int32_t* flag, int K, int D, int Hp, int Wp,
                             int y0, int x0, int Hc, int Wc, int Ho, int Wo, int D0, int H0, int W0, int bd, int by, int bx, int mode,
                             int64_t region_order, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !seg || !flag || (mode != DU_EXPORT_SOFTMAX && mode != DU_EXPORT_REGIONS)) return DU_ERR_BAD_ARG;
  if (K < (mode == DU_EXPORT_SOFTMAX ? 2 : 1) || K > MAXC) return DU_ERR_UNSUPPORTED;
  if (D <= 0 || Hp <= 0 || Wp <= 0 || Hc <= 0 || Wc <= 0 || Ho <= 0 || Wo <= 0 || D0 <= 0 || H0 <= 0 || W0 <= 0) return DU_ERR_BAD_ARG;
  if (y0 < 0 || x0 < 0 || y0 > Hp - Hc || x0 > Wp - Wc) return DU_ERR_BAD_ARG;                    // the window lies inside the accumulators
  if (bd < 0 || by < 0 || bx < 0 || bd > D0 - D || by > H0 - Ho || bx > W0 - Wo) return DU_ERR_BAD_ARG;   // the bbox (D, Ho, Wo) fits the destination
  const int lim = 1 << 22;                                                                       // tap weights: integers below 2^24 in fp32
  if (Hc > lim || Wc > lim || Ho > lim || Wo > lim) return DU_ERR_UNSUPPORTED;
  const bool resample = Ho != Hc || Wo != Wc;
  ExportGeom g;
  g.D = D; g.Hp = Hp; g.Wp = Wp; g.y0 = y0; g.x0 = x0; g.Hc = Hc; g.Wc = Wc; g.Ho = Ho; g.Wo = Wo;
  g.D0 = D0; g.H0 = H0; g.W0 = W0; g.bd = bd; g.by = by; g.bx = bx;
  // vector loads: rows of the accumulators start on 16 bytes (Wp % 4 == 0, aligned base) and the quads are shifted by `pad` columns so that
  // output column -pad reads an accumulator column that is a multiple of 4; otherwise every load is a guarded scalar one
  const bool vec_in = !resample && Wp % 4 == 0 && aligned_to(sums, 16) && (!npred || aligned_to(npred, 16));
  g.pad = vec_in ? (((x0 - bx) % 4) + 4) % 4 : 0;
  g.nq = (W0 + g.pad + 3) / 4;
  const bool vec_out = g.pad == 0 && W0 % 4 == 0;
  const bool vec_seg = vec_out && aligned_to(seg, 4), vec_probs = vec_out && probs && aligned_to(probs, 16);
  const int grid = export_grid((long)D0 * H0 * g.nq);
  const uint64_t order = (uint64_t)region_order;
#define CALL(CC)                                                                                                                            \
  if (mode == DU_EXPORT_REGIONS) {                                                                                                          \
    if (resample) hipLaunchKernelGGL((export_seg_kernel<CC, true, true>), dim3(grid), dim3(256), 0, st, sums, npred, seg, probs, (int*)flag, g, order, vec_in, vec_seg, vec_probs); \
    else hipLaunchKernelGGL((export_seg_kernel<CC, true, false>), dim3(grid), dim3(256), 0, st, sums, npred, seg, probs, (int*)flag, g, order, vec_in, vec_seg, vec_probs); \
  } else {                                                                                                                                  \
    if (resample) hipLaunchKernelGGL((export_seg_kernel<CC, false, true>), dim3(grid), dim3(256), 0, st, sums, npred, seg, probs, (int*)flag, g, order, vec_in, vec_seg, vec_probs); \
    else hipLaunchKernelGGL((export_seg_kernel<CC, false, false>), dim3(grid), dim3(256), 0, st, sums, npred, seg, probs, (int*)flag, g, order, vec_in, vec_seg, vec_probs); \
  }
  EXPORT_C_SWITCH(K, CALL)
#undef CALL
  return du_check_launch();
}

extern "C" int64_t du_seg_counts_ws_elems(int64_t n, int R) {
  if (n <= 0 || R < 1 || R > MAXC) return 0;
  return (int64_t)counts_grid(n) * (3 * R + 1);
}

extern "C" int du_seg_counts(const uint8_t* pred, const uint8_t* ref, const int64_t* masks, int64_t* counts, int64_t n, int R,
                             int has_ignore, int ignore_label, int32_t* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!pred || !ref || !masks || !counts || !ws || n <= 0 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXC || n >= ((int64_t)1 << 31)) return DU_ERR_UNSUPPORTED;                  // int32 block partials
  const int grid = counts_grid(n);
  if (ws_elems < (int64_t)grid * (3 * R + 1)) return DU_ERR_BAD_ARG;
  const bool vec = aligned_to(pred, 16) && aligned_to(ref, 16);
#define CALL(RR) hipLaunchKernelGGL(seg_counts_partial_kernel<RR>, dim3(grid), dim3(256), 0, st, pred, ref, masks, (int*)ws, (long)n, has_ignore, ignore_label, vec)
  EXPORT_C_SWITCH(R, CALL)
#undef CALL
  hipLaunchKernelGGL(seg_counts_sum_kernel, dim3(1), dim3(256), 0, st, (const int*)ws, counts, grid, R);
  return du_check_launch();
}
