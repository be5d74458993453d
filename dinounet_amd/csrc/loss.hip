// Fused soft-Dice + cross-entropy loss of the reference trainer on fp32 NCHW logits:
//   DC_and_CE_loss (dinounet/training/loss/compound_losses.py:8-56) = RobustCrossEntropyLoss (mean over pixels)
//   + MemoryEfficientSoftDiceLoss(batch_dice=True, do_bg=False, smooth=1e-5) (dice.py:58-119):
//       dc_c = (2 I_c + s) / clip(G_c + P_c + s, 1e-8),   I_c = sum p_c [t = c],  P_c = sum p_c,  G_c = sum [t = c]   (c >= 1)
//       loss = CE - mean_c dc_c
// One pass over the logits produces the softmax-dependent sums (stock torch needs ~25 launches and several full-size temporaries and
// its multi-block reductions misbehave under hipGraph replay); the backward pass recomputes the softmax and writes d loss / d logits.
// HBM-bound: forward reads K*4 + 8 bytes per pixel, backward reads the same and writes K*4.
#include "common.h"
#include "loss_common.h"

namespace {

constexpr int MAXK = 16;

// Validation counts (COUNTS instantiations of the partial kernels; nnUNetTrainer.validation_step, nnUNetTrainer.py:971-994 with
// get_tp_fp_fn_tn, dice.py:122-167): per class / region three int32 lane counters (hits, predicted, labelled) over the valid pixels, added
// over the wave and the block as integers into one row of 3C int32 per block (cpart).  counts_sum_kernel adds the rows in int64 and turns
// them into tp = hits, fp = predicted - hits, fn = labelled - hits.  The float code of a COUNTS instantiation is the text of the COUNTS =
// false one, so the sums (and the loss `finish` makes of them) are the training forward's, bit for bit.
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int NC>
__device__ __forceinline__ void block_counts_store(int (&cnt)[NC], int* __restrict__ cpart) {
  __shared__ int cred[4][NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NC; i++) {
    const int s = wave_sum_i(cnt[i]);
    if (lane == 0) cred[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NC) cpart[(long)blockIdx.x * NC + threadIdx.x] = cred[0][threadIdx.x] + cred[1][threadIdx.x] + cred[2][threadIdx.x] + cred[3][threadIdx.x];
}
// torch.argmax over the class axis: the lowest index among equal maxima (finite logits)
template <int K, typename F>
__device__ __forceinline__ int argmax_first(F&& x) {
  int pred = 0;
  float best = x(0);
#pragma unroll
  for (int k = 1; k < K; k++) { const float xk = x(k); if (xk > best) { best = xk; pred = k; } }
  return pred;
}

// second stage of the counts: ONE block adds the per-block rows (blocks x 3C int32) in int64, fixed order; counts (3, C) int64 =
// this step's (tp, fp, fn), accum (3, C) int64 += the same (NULL: skipped)
__global__ __launch_bounds__(256) void counts_sum_kernel(const int* __restrict__ cpart, int64_t* __restrict__ counts,
                                                         int64_t* __restrict__ accum, int blocks, int C) {
  __shared__ long long red[3 * 8][4];
  __shared__ long long tot[3 * 8];
  const int NC = 3 * C;
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
  if (threadIdx.x < NC) {
    const int row = threadIdx.x / C, c = threadIdx.x - row * C;
    const long long v = row == 0 ? tot[c] : tot[row * C + c] - tot[c];
    counts[threadIdx.x] = (int64_t)v;
    if (accum) accum[threadIdx.x] += (int64_t)v;
  }
}

// sums layout: [0] = sum of -log p_target, then for c = 1..K-1: [1 + 3(c-1) + {0,1,2}] = (I_c, P_c, G_c)
template <int K, bool COUNTS>
__global__ __launch_bounds__(256) void dice_ce_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                              float* __restrict__ part, int* __restrict__ cpart, int B, long HW) {
  constexpr int NS = 1 + 3 * (K - 1);
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  int cnt[COUNTS ? 3 * K : 1];
#pragma unroll
  for (int i = 0; i < (COUNTS ? 3 * K : 1); i++) cnt[i] = 0;
  const long npix = (long)B * HW;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long b = p / HW, r = p - b * HW;
    const float* lp = logits + b * K * HW + r;
    float v[K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; k++) { v[k] = lp[(long)k * HW]; mx = fmaxf(mx, v[k]); }
    const int t = (int)target[p];
    if constexpr (COUNTS) {
      const int pred = argmax_first<K>([&](int k) { return v[k]; });
#pragma unroll
      for (int k = 0; k < K; k++) {
        cnt[k] += (pred == k && t == k) ? 1 : 0;
        cnt[K + k] += pred == k ? 1 : 0;
        cnt[2 * K + k] += t == k ? 1 : 0;
      }
    }
    float se = 0.f, xt = mx;
#pragma unroll
    for (int k = 0; k < K; k++) { if (k == t) xt = v[k]; v[k] = __expf(v[k] - mx); se += v[k]; }
    const float inv = 1.f / se;
    if (t >= 0 && t < K) acc[0] += softmax_nll(mx, xt, se);     // shared with the COUNTS twin: this is its text
#pragma unroll
    for (int k = 0; k < K; k++) {
      const float pk = v[k] * inv;
      if (k >= 1) {
        acc[1 + 3 * (k - 1) + 1] += pk;
        if (k == t) { acc[1 + 3 * (k - 1)] += pk; acc[1 + 3 * (k - 1) + 2] += 1.f; }
      }
    }
  }
  __shared__ float red[4][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NS; i++) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NS) part[(long)blockIdx.x * NS + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  if constexpr (COUNTS) block_counts_store<3 * K>(cnt, cpart);
}

__global__ __launch_bounds__(256) void dice_ce_sum_kernel(const float* __restrict__ part, float* __restrict__ sums, int blocks, int NS) {
  __shared__ float red[256];
  for (int i = 0; i < NS; i++) {
    float a = 0.f;
    for (int b = threadIdx.x; b < blocks; b += 256) a += part[(long)b * NS + i];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[i] = red[0];
    __syncthreads();
  }
}

// loss and the per-class backward coefficients: d loss / d p_c(pixel) = coef[2(c-1)] * [t = c] + coef[2(c-1) + 1]
__global__ void dice_ce_coef_kernel(const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef, int K,
                                    float inv_npix, float smooth, float grad_mult) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float dc_mean = 0.f;
  const float invc = 1.f / (float)(K - 1);
  for (int c = 1; c < K; c++) {
    const float I = sums[1 + 3 * (c - 1)], P = sums[1 + 3 * (c - 1) + 1], G = sums[1 + 3 * (c - 1) + 2];
    const float num = 2.f * I + smooth;
    const float raw = G + P + smooth;
    const float den = fmaxf(raw, 1e-8f);
    dc_mean += num / den * invc;
    coef[2 * (c - 1)] = -2.f * invc / den * grad_mult;
    coef[2 * (c - 1) + 1] = (raw > 1e-8f ? num / (den * den) * invc : 0.f) * grad_mult;
  }
  loss[0] = sums[0] * inv_npix - dc_mean;
}

template <int K>
__global__ __launch_bounds__(256) void dice_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          const float* __restrict__ coef, const float* __restrict__ gout,
                                                          float* __restrict__ dlogits, int B, long HW, float inv_npix) {
  float ca[K], cb[K];
  ca[0] = 0.f; cb[0] = 0.f;
#pragma unroll
  for (int c = 1; c < K; c++) { ca[c] = coef[2 * (c - 1)]; cb[c] = coef[2 * (c - 1) + 1]; }
  const float go = gout ? gout[0] : 1.f;
  const long npix = (long)B * HW;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const long b = p / HW, r = p - b * HW;
    const float* lp = logits + b * K * HW + r;
    float v[K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; k++) { v[k] = lp[(long)k * HW]; mx = fmaxf(mx, v[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) { v[k] = __expf(v[k] - mx); se += v[k]; }
    const float inv = 1.f / se;
    const int t = (int)target[p];
    float g[K], dot = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) {
      v[k] *= inv;
      g[k] = (k == t ? ca[k] : 0.f) + cb[k];
      dot += g[k] * v[k];
    }
    float* dp = dlogits + b * K * HW + r;
#pragma unroll
    for (int k = 0; k < K; k++) dp[(long)k * HW] = go * ((v[k] - (k == t ? 1.f : 0.f)) * inv_npix + v[k] * (g[k] - dot));
  }
}

int loss_grid(long npix) { long g = (npix + 255) / 256 / 4; if (g < 1) g = 1; if (g > 2048) g = 2048; return (int)g; }

}  // namespace

extern "C" int64_t du_dice_ce_ws_elems(int B, int K, int64_t HW) {
  if (B <= 0 || K < 2 || K > 8 || HW <= 0) return 0;       // what du_dice_ce_sums launches: 0 is the wrapper's "unsupported"
  return (int64_t)loss_grid((long)B * HW) * (1 + 3 * (K - 1));
}

// sums (1 + 3(K-1)) fp32 <- per-pixel softmax sums of this rank's batch
extern "C" int du_dice_ce_sums(const float* logits, const int64_t* target, float* sums, int B, int K, int64_t HW, float* ws,
                               int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !ws || B <= 0 || K < 2 || HW <= 0) return DU_ERR_BAD_ARG;
  const int grid = loss_grid((long)B * HW);
  const int NS = 1 + 3 * (K - 1);
  if (ws_elems < (int64_t)grid * NS) return DU_ERR_BAD_ARG;
#define CALL(KK) hipLaunchKernelGGL((dice_ce_partial_kernel<KK, false>), dim3(grid), dim3(256), 0, st, logits, target, ws, (int*)nullptr, B, (long)HW)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  hipLaunchKernelGGL(dice_ce_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, sums, grid, NS);
  return du_check_launch();
}

// loss (1) and coef (2(K-1)) from (possibly all-reduced) sums; npix = pixels of THIS rank (the CE term is a local mean);
// grad_mult = world size when the dice sums were all-reduced (backward of the all-gather sums the identical coefficient over ranks)
extern "C" int du_dice_ce_finish(const float* sums, float* loss, float* coef, int K, int64_t npix, float smooth, float grad_mult,
                                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !loss || !coef || K < 2 || K > MAXK || npix <= 0) return DU_ERR_BAD_ARG;
  hipLaunchKernelGGL(dice_ce_coef_kernel, dim3(1), dim3(64), 0, st, sums, loss, coef, K, 1.f / (float)npix, smooth, grad_mult);
  return du_check_launch();
}

// dlogits = grad_out[0] * d loss / d logits   (grad_out: device scalar, NULL = 1)
extern "C" int du_dice_ce_bwd(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float* dlogits,
                              int B, int K, int64_t HW, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !coef || !dlogits || B <= 0 || K < 2 || HW <= 0) return DU_ERR_BAD_ARG;
  const long npix = (long)B * HW;
  long g = (npix + 255) / 256; if (g > 8192) g = 8192;
#define CALL(KK) hipLaunchKernelGGL(dice_ce_bwd_kernel<KK>, dim3((unsigned)g), dim3(256), 0, st, logits, target, coef, grad_out, dlogits, B, (long)HW, 1.f / (float)npix)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  return du_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The other two label configurations of the reference trainer (nnUNetTrainer._build_loss, nnUNetTrainer.py:355-365):
//  * ignore label (sparse annotation): DC_and_CE_loss(ignore_label) (compound_losses.py:31-56, dice.py:72-119 with loss_mask):
//      m = [t != ignore];  CE = sum m (-log p_t) / n_valid, exactly 0 when n_valid = 0 (compound_losses.py:52-53, decided on the device);
//      Dice over classes 1..K-1 with p and the one-hot target multiplied by m.
//  * regions (sigmoid outputs, overlapping classes): DC_and_BCE_loss (compound_losses.py:83-99), MemoryEfficientSoftDiceLoss(sigmoid,
//      do_bg=True); target = uint8 one-hot planes (B, R + u, HW), u = 1 with an ignore label, m = 1 - target[:, R]:
//      BCE = sum m bce / clip(n_valid, 1e-8) with n_valid counted in PIXELS (the (B,1,H,W) mask broadcast over R, :95), else the mean
//      over all B R HW elements; Dice over all R regions on sigmoid(x).
// Sums layouts: masked softmax [CE_sum, n_valid, (I_c, P_c, G_c) c = 1..K-1], regions [BCE_sum, n_valid, (I_r, P_r, G_r) r = 0..R-1]:
// under data parallelism only sums[2:] are all-reduced.  `finish` also writes the CE / BCE scale (1/n_valid or 0) after the 2(K-1) /
// 2R dice coefficients, so the backward pass needs no host value.  Each lane handles 4 consecutive pixels of one image (16 B per fp32
// logits plane, one dword per uint8 plane, 32 B of int64 labels); when HW % 4 != 0 the rows are not 16 B aligned and every quad takes
// the guarded scalar path (the last quad of an image is partial).  Reductions are two-stage, per-block partial rows + one block adding
// them (partial_rows_sum_kernel, loss_common.h): no float atomics, bit-reproducible across calls and graph replays.
namespace {

constexpr int MAXR = 8;

template <int K, bool COUNTS>
__global__ __launch_bounds__(256) void dice_ce_masked_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                     float* __restrict__ part, int* __restrict__ cpart, int B, long HW,
                                                                     int64_t ignore, bool vec) {
  constexpr int NS = 2 + 3 * (K - 1);
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  int cnt[COUNTS ? 3 * K : 1];
#pragma unroll
  for (int i = 0; i < (COUNTS ? 3 * K : 1); i++) cnt[i] = 0;
  const long nq = (HW + 3) >> 2, items = (long)B * nq;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = logits + b * K * HW + r0;
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; k++) ld4f(lp + (long)k * HW, vec, n, v[k]);
    int64_t t[4];
    ld4l(target + b * HW + r0, vec, n, ignore, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool valid = t[j] != ignore;
      if constexpr (COUNTS) {       // an ignored pixel (and the padding of a partial quad) adds to no count
        const int pred = argmax_first<K>([&](int k) { return v[k][j]; });
#pragma unroll
        for (int k = 0; k < K; k++) {
          cnt[k] += (valid && pred == k && t[j] == k) ? 1 : 0;
          cnt[K + k] += (valid && pred == k) ? 1 : 0;
          cnt[2 * K + k] += (valid && t[j] == k) ? 1 : 0;
        }
      }
      float x[K];
#pragma unroll
      for (int k = 0; k < K; k++) x[k] = v[k][j];
      softmax_pixel_fwd<K>(x, t[j], valid, acc, [&](float nll) { return valid ? nll : 0.f; });
    }
  }
  block_partial_store<NS>(acc, part);
  if constexpr (COUNTS) block_counts_store<3 * K>(cnt, cpart);
}

// coef = [(ca_c, cb_c) c = 1..K-1, ce_scale]
__global__ void dice_ce_masked_coef_kernel(const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef, int K,
                                           float smooth, float grad_mult) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  loss[0] = loss_finish(sums, sums + 2, coef, K - 1, false, smooth, grad_mult, 1.f);
}

template <int K>
__global__ __launch_bounds__(256) void dice_ce_masked_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 const float* __restrict__ coef, const float* __restrict__ gout,
                                                                 float* __restrict__ dlogits, int B, long HW, int64_t ignore, bool vec) {
  float ca[K], cb[K];
  load_dice_coefs<K, K - 1>(coef, ca, cb);
  const float ce_scale = coef[2 * (K - 1)];
  const float go = gout ? gout[0] : 1.f;
  const long nq = (HW + 3) >> 2, items = (long)B * nq;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = logits + b * K * HW + r0;
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; k++) ld4f(lp + (long)k * HW, vec, n, v[k]);
    int64_t t[4];
    ld4l(target + b * HW + r0, vec, n, ignore, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool valid = t[j] != ignore;
      const float ce_scale_j = ce_scale;
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; k++) mx = fmaxf(mx, v[k][j]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) { v[k][j] = __expf(v[k][j] - mx); se += v[k][j]; }
      const float inv = 1.f / se;
      float g[K], dot = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) {
        v[k][j] *= inv;
        g[k] = (k == t[j] ? ca[k] : 0.f) + cb[k];
        dot += g[k] * v[k][j];
      }
#pragma unroll
      for (int k = 0; k < K; k++)
        v[k][j] = valid ? go * ((v[k][j] - (k == t[j] ? 1.f : 0.f)) * ce_scale_j + v[k][j] * (g[k] - dot)) : 0.f;
    }
    float* dp = dlogits + b * K * HW + r0;
#pragma unroll
    for (int k = 0; k < K; k++) st4f(dp + (long)k * HW, vec, n, v[k]);
  }
}

// COUNTS: region r is predicted where x > 0.  The reference thresholds sigmoid(x) > 0.5 (nnUNetTrainer.py:974); torch's fp32 sigmoid
// rounds to exactly 0.5 for 0 < x < ~1.2e-7, so the two predicates differ only inside that band (and agree at x = 0: not predicted)
template <int R, bool COUNTS>
__global__ __launch_bounds__(256) void dice_bce_partial_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ target,
                                                               float* __restrict__ part, int* __restrict__ cpart, int B, long HW, int ign,
                                                               bool vec) {
  constexpr int NS = 2 + 3 * R;
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  int cnt[COUNTS ? 3 * R : 1];
#pragma unroll
  for (int i = 0; i < (COUNTS ? 3 * R : 1); i++) cnt[i] = 0;
  const long nq = (HW + 3) >> 2, items = (long)B * nq;
  const int T = R + ign;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = logits + b * R * HW + r0;
    const uint8_t* tp = target + b * T * HW + r0;
    const uint32_t iw = ign ? ld4b(tp + (long)R * HW, vec, n) : 0u;
    bool m[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { m[j] = j < n && ((iw >> (8 * j)) & 0xffu) == 0u; acc[1] += m[j] ? 1.f : 0.f; }
#pragma unroll
    for (int r = 0; r < R; r++) {
      float x[4];
      ld4f(lp + (long)r * HW, vec, n, x);
      const uint32_t yw = ld4b(tp + (long)r * HW, vec, n);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float y = ((yw >> (8 * j)) & 0xffu) ? 1.f : 0.f;
        if constexpr (COUNTS) {
          const bool pred = x[j] > 0.f, lab = ((yw >> (8 * j)) & 0xffu) != 0u;
          cnt[r] += (m[j] && pred && lab) ? 1 : 0;
          cnt[R + r] += (m[j] && pred) ? 1 : 0;
          cnt[2 * R + r] += (m[j] && lab) ? 1 : 0;
        }
        sigmoid_elem_fwd(x[j], y, m[j], r, acc);
      }
    }
  }
  block_partial_store<NS>(acc, part);
  if constexpr (COUNTS) block_counts_store<3 * R>(cnt, cpart);
}

// coef = [(ca_r, cb_r) r = 0..R-1, bce_scale]; bce_scale = 1 / n_valid with an ignore channel (pixels, not pixel x region), else
// 1 / (n_valid R) = the mean over every element; 0 when nothing is valid
__global__ void dice_bce_coef_kernel(const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef, int R, int ign,
                                     float smooth, float grad_mult) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  loss[0] = loss_finish(sums, sums + 2, coef, R, !ign, smooth, grad_mult, 1.f);
}

template <int R>
__global__ __launch_bounds__(256) void dice_bce_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ target,
                                                           const float* __restrict__ coef, const float* __restrict__ gout,
                                                           float* __restrict__ dlogits, int B, long HW, int ign, bool vec) {
  const float bce_scale = coef[2 * R];
  const float go = gout ? gout[0] : 1.f;
  const long nq = (HW + 3) >> 2, items = (long)B * nq;
  const int T = R + ign;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = logits + b * R * HW + r0;
    float* dp = dlogits + b * R * HW + r0;
    const uint8_t* tp = target + b * T * HW + r0;
    const uint32_t iw = ign ? ld4b(tp + (long)R * HW, vec, n) : 0u;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float ca = coef[2 * r], cb = coef[2 * r + 1];
      float x[4];
      ld4f(lp + (long)r * HW, vec, n, x);
      const uint32_t yw = ld4b(tp + (long)r * HW, vec, n);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool m = ((iw >> (8 * j)) & 0xffu) == 0u;
        const float y = ((yw >> (8 * j)) & 0xffu) ? 1.f : 0.f;
        x[j] = m ? sigmoid_elem_bwd(x[j], y, ca, cb, bce_scale, go) : 0.f;
      }
      st4f(dp + (long)r * HW, vec, n, x);
    }
  }
}

// out (B, R + ign, HW) uint8: plane r = [0 <= label < 64 and bit label of table[r]], plane R = [label == ignore_label]
__global__ __launch_bounds__(256) void labels_to_regions_kernel(const int64_t* __restrict__ seg, const int64_t* __restrict__ table,
                                                                uint8_t* __restrict__ out, int B, int R, long HW, int ign, int64_t ignore, bool vec) {
  uint64_t tb[MAXR];
#pragma unroll
  for (int r = 0; r < MAXR; r++) tb[r] = r < R ? (uint64_t)table[r] : 0ull;
  const long nq = (HW + 3) >> 2, items = (long)B * nq;
  const int T = R + ign;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    int64_t l[4];
    ld4l(seg + b * HW + r0, vec, n, -1, l);
    uint8_t* op = out + b * T * HW + r0;
#pragma unroll
    for (int r = 0; r < MAXR; r++) {
      if (r < R) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) w |= (l[j] >= 0 && l[j] < 64 && ((tb[r] >> l[j]) & 1ull)) ? (1u << (8 * j)) : 0u;
        st4b(op + (long)r * HW, vec, n, w);
      }
    }
    if (ign) {
      uint32_t w = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) w |= l[j] == ignore ? (1u << (8 * j)) : 0u;
      st4b(op + (long)R * HW, vec, n, w);
    }
  }
}

bool counts_fit(int B, int64_t HW) { return (int64_t)B * HW < ((int64_t)1 << 31); }

// The sums pass of a training loss (COUNTS = false) and of its validation twin (COUNTS = true: the same float code, plus the int32 count
// rows behind the float rows of ws and counts_sum_kernel).  The entries check their arguments; these check the workspace and launch.
template <bool COUNTS>
int masked_sums_launch(const float* logits, const int64_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int K, int64_t HW,
                       int64_t ignore_label, float* ws, int64_t ws_elems, hipStream_t st) {
  const int grid = masked_grid(quad_items(B, HW));
  const int NS = 2 + 3 * (K - 1);
  if (ws_elems < (int64_t)grid * (NS + (COUNTS ? 3 * K : 0))) return DU_ERR_BAD_ARG;
  int* cws = COUNTS ? reinterpret_cast<int*>(ws + (long)grid * NS) : nullptr;
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 16);
#define CALL(KK) hipLaunchKernelGGL((dice_ce_masked_partial_kernel<KK, COUNTS>), dim3(grid), dim3(256), 0, st, logits, target, ws, cws, B, (long)HW, ignore_label, vec); \
                 hipLaunchKernelGGL(partial_rows_sum_kernel<2 + 3 * (KK - 1)>, dim3(1), dim3(256), 0, st, (const float*)ws, sums, grid)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  if (COUNTS) hipLaunchKernelGGL(counts_sum_kernel, dim3(1), dim3(256), 0, st, (const int*)cws, counts, accum, grid, K);
  return du_check_launch();
}

template <bool COUNTS>
int bce_sums_launch(const float* logits, const uint8_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int R, int64_t HW,
                    int has_ignore, float* ws, int64_t ws_elems, hipStream_t st) {
  const int grid = masked_grid(quad_items(B, HW));
  const int NS = 2 + 3 * R;
  if (ws_elems < (int64_t)grid * (NS + (COUNTS ? 3 * R : 0))) return DU_ERR_BAD_ARG;
  int* cws = COUNTS ? reinterpret_cast<int*>(ws + (long)grid * NS) : nullptr;
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 4);
#define CALL(RR) hipLaunchKernelGGL((dice_bce_partial_kernel<RR, COUNTS>), dim3(grid), dim3(256), 0, st, logits, target, ws, cws, B, (long)HW, has_ignore, vec); \
                 hipLaunchKernelGGL(partial_rows_sum_kernel<2 + 3 * RR>, dim3(1), dim3(256), 0, st, (const float*)ws, sums, grid)
  LOSS_SWITCH(R, 1, CALL)
#undef CALL
  if (COUNTS) hipLaunchKernelGGL(counts_sum_kernel, dim3(1), dim3(256), 0, st, (const int*)cws, counts, accum, grid, R);
  return du_check_launch();
}

}  // namespace

extern "C" int64_t du_dice_ce_masked_ws_elems(int B, int K, int64_t HW) {
  if (B <= 0 || K < 2 || K > 8 || HW <= 0) return 0;
  return (int64_t)masked_grid(quad_items(B, HW)) * (2 + 3 * (K - 1));
}

extern "C" int du_dice_ce_masked_sums(const float* logits, const int64_t* target, float* sums, int B, int K, int64_t HW,
                                      int64_t ignore_label, float* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !ws || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  return masked_sums_launch<false>(logits, target, sums, nullptr, nullptr, B, K, HW, ignore_label, ws, ws_elems, st);
}

extern "C" int du_dice_ce_masked_finish(const float* sums, float* loss, float* coef, int K, float smooth, float grad_mult, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !loss || !coef) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dice_ce_masked_coef_kernel, dim3(1), dim3(64), 0, st, sums, loss, coef, K, smooth, grad_mult);
  return du_check_launch();
}

extern "C" int du_dice_ce_masked_bwd(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float* dlogits,
                                     int B, int K, int64_t HW, int64_t ignore_label, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !coef || !dlogits || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  const int g = elem_grid(quad_items(B, HW));
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 16) && al(dlogits, 16);
#define CALL(KK) hipLaunchKernelGGL(dice_ce_masked_bwd_kernel<KK>, dim3(g), dim3(256), 0, st, logits, target, coef, grad_out, dlogits, B, (long)HW, ignore_label, vec)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  return du_check_launch();
}

extern "C" int64_t du_dice_bce_ws_elems(int B, int R, int64_t HW) {
  if (B <= 0 || R < 1 || R > MAXR || HW <= 0) return 0;
  return (int64_t)masked_grid(quad_items(B, HW)) * (2 + 3 * R);
}

extern "C" int du_dice_bce_sums(const float* logits, const uint8_t* target, float* sums, int B, int R, int64_t HW, int has_ignore, float* ws,
                                int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !ws || B <= 0 || HW <= 0 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR) return DU_ERR_UNSUPPORTED;
  return bce_sums_launch<false>(logits, target, sums, nullptr, nullptr, B, R, HW, has_ignore, ws, ws_elems, st);
}

extern "C" int du_dice_bce_finish(const float* sums, float* loss, float* coef, int R, int has_ignore, float smooth, float grad_mult,
                                  void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !loss || !coef || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR) return DU_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dice_bce_coef_kernel, dim3(1), dim3(64), 0, st, sums, loss, coef, R, has_ignore, smooth, grad_mult);
  return du_check_launch();
}

extern "C" int du_dice_bce_bwd(const float* logits, const uint8_t* target, const float* coef, const float* grad_out, float* dlogits, int B,
                               int R, int64_t HW, int has_ignore, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !coef || !dlogits || B <= 0 || HW <= 0 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR) return DU_ERR_UNSUPPORTED;
  const int g = elem_grid(quad_items(B, HW));
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 4) && al(dlogits, 16);
#define CALL(RR) hipLaunchKernelGGL(dice_bce_bwd_kernel<RR>, dim3(g), dim3(256), 0, st, logits, target, coef, grad_out, dlogits, B, (long)HW, has_ignore, vec)
  LOSS_SWITCH(R, 1, CALL)
#undef CALL
  return du_check_launch();
}

extern "C" int du_labels_to_regions(const int64_t* seg, const int64_t* table, uint8_t* out, int B, int R, int64_t HW, int has_ignore,
                                    int64_t ignore_label, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!seg || !table || !out || B <= 0 || HW <= 0 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR) return DU_ERR_UNSUPPORTED;
  const bool vec = HW % 4 == 0 && al(seg, 16) && al(out, 4);
  hipLaunchKernelGGL(labels_to_regions_kernel, dim3(elem_grid(quad_items(B, HW))), dim3(256), 0, st, seg, table, out, B, R, (long)HW,
                     has_ignore, ignore_label, vec);
  return du_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Validation pass (nnUNetTrainer.validation_step, nnUNetTrainer.py:946-1008): the sums of the matching training loss (same layout, same
// bits: the COUNTS instantiations share the float code; the caller runs the matching *_finish on them) and the exact tp / fp / fn of the
// hard prediction, from ONE read of the logits.  counts (3, C) int64 = this step's [tp | fp | fn] over all C = K classes / R regions
// (the host drops the background, :999-1006); accum (3, C) int64 += counts (NULL: none).  ws: the float partial rows, then the int32 count
// rows (4-byte elements both).  int32 block partials: B * HW < 2^31.
extern "C" int64_t du_val_dice_ce_ws_elems(int B, int K, int64_t HW) {
  if (B <= 0 || K < 2 || K > 8 || HW <= 0) return 0;
  return (int64_t)loss_grid((long)B * HW) * (1 + 3 * (K - 1) + 3 * K);
}

extern "C" int du_val_dice_ce(const float* logits, const int64_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int K,
                              int64_t HW, float* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !counts || !ws || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8 || !counts_fit(B, HW)) return DU_ERR_UNSUPPORTED;
  const int grid = loss_grid((long)B * HW);
  const int NS = 1 + 3 * (K - 1);
  if (ws_elems < (int64_t)grid * (NS + 3 * K)) return DU_ERR_BAD_ARG;
  int* cws = reinterpret_cast<int*>(ws + (long)grid * NS);
#define CALL(KK) hipLaunchKernelGGL((dice_ce_partial_kernel<KK, true>), dim3(grid), dim3(256), 0, st, logits, target, ws, cws, B, (long)HW)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  hipLaunchKernelGGL(dice_ce_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, sums, grid, NS);
  hipLaunchKernelGGL(counts_sum_kernel, dim3(1), dim3(256), 0, st, (const int*)cws, counts, accum, grid, K);
  return du_check_launch();
}

extern "C" int64_t du_val_dice_ce_masked_ws_elems(int B, int K, int64_t HW) {
  if (B <= 0 || K < 2 || K > 8 || HW <= 0) return 0;
  return (int64_t)masked_grid(quad_items(B, HW)) * (2 + 3 * (K - 1) + 3 * K);
}

extern "C" int du_val_dice_ce_masked(const float* logits, const int64_t* target, float* sums, int64_t* counts, int64_t* accum, int B,
                                     int K, int64_t HW, int64_t ignore_label, float* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !counts || !ws || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8 || !counts_fit(B, HW)) return DU_ERR_UNSUPPORTED;
  return masked_sums_launch<true>(logits, target, sums, counts, accum, B, K, HW, ignore_label, ws, ws_elems, st);
}

extern "C" int64_t du_val_dice_bce_ws_elems(int B, int R, int64_t HW) {
  if (B <= 0 || R < 1 || R > MAXR || HW <= 0) return 0;
  return (int64_t)masked_grid(quad_items(B, HW)) * (2 + 3 * R + 3 * R);
}

extern "C" int du_val_dice_bce(const float* logits, const uint8_t* target, float* sums, int64_t* counts, int64_t* accum, int B, int R,
                               int64_t HW, int has_ignore, float* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !counts || !ws || B <= 0 || HW <= 0 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR || !counts_fit(B, HW)) return DU_ERR_UNSUPPORTED;
  return bce_sums_launch<true>(logits, target, sums, counts, accum, B, R, HW, has_ignore, ws, ws_elems, st);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Deep supervision (DeepSupervisionWrapper, training/loss/deep_supervision.py, around the three losses above with the weights of
// nnUNetTrainer._build_loss, nnUNetTrainer.py:373-387): total = sum_s w_s loss_s over the S <= 4 logits tensors of the decoder, largest
// first, each against the full-resolution label map resampled to its size.  The lower-scale targets of the reference
// (DownsampleSegForDSTransform2: resize_segmentation(order=0) = skimage resize(order=0, mode="edge", anti_aliasing=False) =
// scipy.ndimage.zoom(order=0, mode="nearest", grid_mode=True)) are index arithmetic on the full-resolution map,
//     target_s(y, x) = target(src(y, H / h_s, H), src(x, W / w_s, W)),   src(i, z, n) = floor(clamp((i + 0.5) z - 0.5, 0, n - 1) + 0.5),
// evaluated in fp64 operation by operation as scipy's NI_ZoomShift does (ds_src_index: the exact value is ((2i + 1) n) div (2 m), but where
// n / m is not a binary fraction scipy's rounding decides the ties, e.g. 148 -> 18 at i = 13, and the reference's target is scipy's),
// so they are gathered in the kernels and never stored; region membership is decided from the gathered int64 label and the 64-bit region
// table (the du_labels_to_regions convention), so no one-hot plane exists at any scale either.  Four launches whatever S is: partial
// rows (every block serves one scale, found in a by-value descriptor table), one block per scale adding its rows in a fixed order,
// finish (per-scale losses, total, backward coefficients with w_s folded in), backward of every active scale.  A scale with w_s == 0 is
// inactive, as in the wrapper: no block is assigned to it, its logits are never read and it gets no gradient.
// Two per-pixel bodies serve the three label configurations: softmax (plain labels = masked with an ignore value no label takes) and
// sigmoid regions.  sums (S (2 + 3 C) floats, C = K - 1 or R): [(CE or BCE sum, n_valid) s = 0..S-1 | (I_c, P_c, G_c) c < C, s = 0..S-1]:
// the Dice slices of all scales are contiguous (sums[2 S:]), one all-reduce covers them under data parallelism.
namespace {

constexpr int DS_MAX = 4;
constexpr int64_t DS_NO_IGNORE = INT64_MIN;

struct DsScale {
  const float* x;       // logits (B, N, h, w) fp32
  float* dx;            // their gradient (backward launch)
  int h, w;
  int first, nblk;      // this scale's blocks: first .. first + nblk - 1 (nblk == 0: inactive)
  int vec;              // the 4-pixel vector path
  double zy, zx;        // (double)H / h, (double)W / w: scipy's zoom of the two axes
};
struct DsTable {
  DsScale s[DS_MAX];
  float wgt[DS_MAX];
  int S, B, H, W;
};

// kernel-argument structs are indexed with compile-time indices only (a run-time index would move the table to scratch)
__device__ __forceinline__ DsScale ds_scale_of_block(const DsTable& d, int& si) {
  DsScale sc = d.s[0];
  si = 0;
#pragma unroll
  for (int i = 1; i < DS_MAX; i++)
    if (i < d.S && d.s[i].nblk > 0 && (int)blockIdx.x >= d.s[i].first) { sc = d.s[i]; si = i; }
  return sc;
}
__device__ __forceinline__ float ds_weight(const DsTable& d, int s) {
  float w = d.wgt[0];
#pragma unroll
  for (int i = 1; i < DS_MAX; i++) if (s == i) w = d.wgt[i];
  return w;
}

// source index of output position i along an axis of n input and n / zoom output positions: scipy.ndimage.zoom(order=0, mode="nearest",
// grid_mode=True), NI_ZoomShift's arithmetic step by step in fp64 (no contraction: a fused multiply-add would round differently)
__device__ __forceinline__ int ds_src_index(int i, double zoom, int n) {
#pragma clang fp contract(off)
  double cc = ((double)i + 0.5) * zoom;
  cc = cc - 0.5;
  cc = fmin(fmax(cc, 0.0), (double)(n - 1));
  return (int)floor(cc + 0.5);
}

// labels of the 4 pixels r0 .. r0 + 3 of image b at a scale of (h, w); tb = target + b H W.  Pixels past the image get `fill`
// (and are not loaded: their source row would lie past the map)
__device__ __forceinline__ void ds_labels(const int64_t* __restrict__ tb, long r0, int n, bool full, bool vec, const DsScale& sc, int H, int W,
                                          int64_t fill, int64_t t[4]) {
  if (full) { ld4l(tb + r0, vec, n, fill, t); return; }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    t[j] = fill;
    if (j < n) {
      const int r = (int)r0 + j, y = r / sc.w, x = r - y * sc.w;
      t[j] = tb[(long)ds_src_index(y, sc.zy, H) * W + ds_src_index(x, sc.zx, W)];
    }
  }
}

template <bool SIG, int N>
__global__ __launch_bounds__(256) void ds_partial_kernel(DsTable d, const int64_t* __restrict__ target, const int64_t* __restrict__ table,
                                                         float* __restrict__ part, int64_t ignore) {
  constexpr int CD = SIG ? N : N - 1, NS = 2 + 3 * CD;
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  int si;
  const DsScale sc = ds_scale_of_block(d, si);
  const long HW = (long)sc.h * sc.w, HWf = (long)d.H * d.W;
  const bool full = sc.h == d.H && sc.w == d.W, vec = sc.vec != 0;
  const long nq = (HW + 3) >> 2, items = (long)d.B * nq;
  uint64_t tb[SIG ? N : 1];
  if constexpr (SIG) {
#pragma unroll
    for (int r = 0; r < N; r++) tb[r] = (uint64_t)table[r];
  }
  for (long it = (long)((int)blockIdx.x - sc.first) * 256 + threadIdx.x; it < items; it += (long)sc.nblk * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = sc.x + b * N * HW + r0;
    int64_t t[4];
    ds_labels(target + b * HWf, r0, n, full, vec, sc, d.H, d.W, ignore, t);
    if constexpr (SIG) {
      bool m[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { m[j] = j < n && t[j] != ignore; acc[1] += m[j] ? 1.f : 0.f; }
#pragma unroll
      for (int r = 0; r < N; r++) {
        float x[4];
        ld4f(lp + (long)r * HW, vec, n, x);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float y = (t[j] >= 0 && t[j] < 64 && ((tb[r] >> t[j]) & 1ull)) ? 1.f : 0.f;
          sigmoid_elem_fwd(x[j], y, m[j], r, acc);
        }
      }
    } else {
      float v[N][4];
#pragma unroll
      for (int k = 0; k < N; k++) ld4f(lp + (long)k * HW, vec, n, v[k]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool valid = j < n && t[j] != ignore;
        float x[N];
#pragma unroll
        for (int k = 0; k < N; k++) x[k] = v[k][j];
        softmax_pixel_fwd<N>(x, t[j], valid, acc, [&](float nll) { return valid ? nll : 0.f; });
      }
    }
  }
  block_partial_store<NS>(acc, part);      // row blockIdx.x: the rows of one scale are consecutive
}

// second stage: block s adds the partial rows of scale s (rows t, t + 256, ... per thread, wave tree, waves 0..3: a fixed order) and
// scatters them into the sums layout above; an inactive scale gets zeros
template <int CD>
__global__ __launch_bounds__(256) void ds_rows_sum_kernel(DsTable d, const float* __restrict__ part, float* __restrict__ sums) {
  constexpr int NS = 2 + 3 * CD;
  const int s = blockIdx.x;
  int first = d.s[0].first, nblk = d.s[0].nblk;
#pragma unroll
  for (int i = 1; i < DS_MAX; i++) if (s == i) { first = d.s[i].first; nblk = d.s[i].nblk; }
  float acc[NS];
  thread_rows_sum<NS>(part + (long)first * NS, nblk, acc);
  block_columns_store<NS>(acc, [&](int i) { return sums + (i < 2 ? 2 * s + i : 2 * d.S + 3 * CD * s + (i - 2)); });
}

// loss = [total, loss_0 .. loss_{S-1}] (0 for an inactive scale); coef (S, 2 CD + 1) = per scale [(ca_c, cb_c) c < CD, CE / BCE scale],
// all multiplied by w_s, so the backward pass writes d total / d logits_s.  total = sum of w_s loss_s over the active scales in scale order
__global__ void ds_finish_kernel(DsTable d, const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef, int CD,
                                 int sig, int ign, float smooth, float grad_mult) {
  __shared__ float ls[DS_MAX];
  const int s = threadIdx.x;
  if (s < d.S) {
    const float w = ds_weight(d, s);
    float* cf = coef + s * (2 * CD + 1);
    float l = 0.f;
    if (w != 0.f) {
      l = loss_finish(sums + 2 * s, sums + 2 * d.S + 3 * CD * s, cf, CD, sig && !ign, smooth, grad_mult, w);
    } else {
      for (int i = 0; i < 2 * CD + 1; i++) cf[i] = 0.f;
    }
    ls[s] = l;
    loss[1 + s] = l;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < d.S; i++) {
      const float w = ds_weight(d, i);
      if (w != 0.f) tot += w * ls[i];
    }
    loss[0] = tot;
  }
}

template <bool SIG, int N>
__global__ __launch_bounds__(256) void ds_bwd_kernel(DsTable d, const int64_t* __restrict__ target, const int64_t* __restrict__ table,
                                                     const float* __restrict__ coef, const float* __restrict__ gout, int64_t ignore) {
  constexpr int CD = SIG ? N : N - 1;
  int si;
  const DsScale sc = ds_scale_of_block(d, si);
  const float* cf = coef + si * (2 * CD + 1);
  float ca[N], cb[N];
  load_dice_coefs<N, CD>(cf, ca, cb);
  const float scale = cf[2 * CD];
  const float go = gout ? gout[0] : 1.f;
  const long HW = (long)sc.h * sc.w, HWf = (long)d.H * d.W;
  const bool full = sc.h == d.H && sc.w == d.W, vec = sc.vec != 0;
  const long nq = (HW + 3) >> 2, items = (long)d.B * nq;
  uint64_t tb[SIG ? N : 1];
  if constexpr (SIG) {
#pragma unroll
    for (int r = 0; r < N; r++) tb[r] = (uint64_t)table[r];
  }
  for (long it = (long)((int)blockIdx.x - sc.first) * 256 + threadIdx.x; it < items; it += (long)sc.nblk * 256) {
    const long b = it / nq, r0 = (it - b * nq) * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const float* lp = sc.x + b * N * HW + r0;
    float* dp = sc.dx + b * N * HW + r0;
    int64_t t[4];
    ds_labels(target + b * HWf, r0, n, full, vec, sc, d.H, d.W, ignore, t);
    if constexpr (SIG) {
#pragma unroll
      for (int r = 0; r < N; r++) {
        float x[4];
        ld4f(lp + (long)r * HW, vec, n, x);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bool m = t[j] != ignore;
          const float y = (t[j] >= 0 && t[j] < 64 && ((tb[r] >> t[j]) & 1ull)) ? 1.f : 0.f;
          x[j] = m ? sigmoid_elem_bwd(x[j], y, ca[r], cb[r], scale, go) : 0.f;
        }
        st4f(dp + (long)r * HW, vec, n, x);
      }
    } else {
      float v[N][4];
#pragma unroll
      for (int k = 0; k < N; k++) ld4f(lp + (long)k * HW, vec, n, v[k]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool valid = t[j] != ignore;
        const float ce_scale_j = scale;
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < N; k++) mx = fmaxf(mx, v[k][j]);
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < N; k++) { v[k][j] = __expf(v[k][j] - mx); se += v[k][j]; }
        const float inv = 1.f / se;
        float g[N], dot = 0.f;
#pragma unroll
        for (int k = 0; k < N; k++) {
          v[k][j] *= inv;
          g[k] = (k == t[j] ? ca[k] : 0.f) + cb[k];
          dot += g[k] * v[k][j];
        }
#pragma unroll
        for (int k = 0; k < N; k++)
          v[k][j] = valid ? go * ((v[k][j] - (k == t[j] ? 1.f : 0.f)) * ce_scale_j + v[k][j] * (g[k] - dot)) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < N; k++) st4f(dp + (long)k * HW, vec, n, v[k]);
    }
  }
}

// DownsampleSegForDSTransform2 on the device: every requested map in one launch, one output pixel per lane
struct DsSegTable {
  int64_t* out[DS_MAX];
  int h[DS_MAX], w[DS_MAX];
  double zy[DS_MAX], zx[DS_MAX];
  long end[DS_MAX];      // exclusive end of map s in the concatenated output index space (B h w pixels each)
  int S, H, W;
};
__global__ __launch_bounds__(256) void ds_downsample_seg_kernel(DsSegTable d, const int64_t* __restrict__ seg) {
  const long total = d.end[DS_MAX - 1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int64_t* out = d.out[0];
    int h = d.h[0], w = d.w[0];
    double zy = d.zy[0], zx = d.zx[0];
    long base = 0;
#pragma unroll
    for (int s = 1; s < DS_MAX; s++)
      if (i >= d.end[s - 1]) { out = d.out[s]; h = d.h[s]; w = d.w[s]; zy = d.zy[s]; zx = d.zx[s]; base = d.end[s - 1]; }
    const long li = i - base, hw = (long)h * w;
    const long b = li / hw;
    const int r = (int)(li - b * hw), y = r / w, x = r - y * w;
    out[li] = seg[b * (long)d.H * d.W + (long)ds_src_index(y, zy, d.H) * d.W + ds_src_index(x, zx, d.W)];
  }
}

// host side of the descriptor table.  bwd: the backward launch's grids and the gradient pointers.  Returns 0 or a DU_ERR_*
int ds_table(DsTable& d, const float* const* logits, float* const* dlogits, const void* target, int B, int H, int W, int S, const int* hs,
             const int* wd, const float* weights, bool bwd, int& total) {
  total = 0;
  if (S < 1 || !hs || !wd || !weights || B <= 0 || H <= 0 || W <= 0) return DU_ERR_BAD_ARG;
  if (S > DS_MAX || H > 32768 || W > 32768) return DU_ERR_UNSUPPORTED;       // pixel indices of a map in 32 bits
  d.S = S; d.B = B; d.H = H; d.W = W;
  bool any = false;
  for (int s = 0; s < DS_MAX; s++) {
    DsScale& sc = d.s[s];
    sc = DsScale{nullptr, nullptr, 1, 1, 0, 0, 0, 1.0, 1.0};
    d.wgt[s] = 0.f;
    if (s >= S) continue;
    if (hs[s] <= 0 || wd[s] <= 0 || hs[s] > H || wd[s] > W) return DU_ERR_BAD_ARG;      // a scale larger than the target
    sc.h = hs[s]; sc.w = wd[s];
    sc.zy = (double)H / (double)sc.h; sc.zx = (double)W / (double)sc.w;
    if (!(weights[s] == weights[s])) return DU_ERR_BAD_ARG;
    d.wgt[s] = weights[s];
    if (weights[s] == 0.f) continue;
    any = true;
    if (logits) {
      if (!logits[s] || (bwd && (!dlogits || !dlogits[s]))) return DU_ERR_BAD_ARG;
      sc.x = logits[s];
      sc.dx = bwd ? dlogits[s] : nullptr;
    }
    const int64_t HW = (int64_t)sc.h * sc.w;
    const long items = quad_items(B, HW);
    if (items >= (1L << 31)) return DU_ERR_UNSUPPORTED;
    const bool full = sc.h == H && sc.w == W;
    sc.vec = HW % 4 == 0 && al(sc.x, 16) && (!bwd || al(sc.dx, 16)) && (!full || al(target, 16));
    sc.first = total;
    sc.nblk = bwd ? elem_grid(items) : masked_grid(items);
    total += sc.nblk;
  }
  return any ? 0 : DU_ERR_BAD_ARG;         // the wrapper asserts at least one weight != 0
}

// mode 0: softmax over C = K classes (2..8), mode 1: sigmoid over C = R regions (1..8)
int ds_mode_ok(int mode, int C) {
  if (mode != 0 && mode != 1) return DU_ERR_BAD_ARG;
  if (mode == 0 ? (C < 2 || C > 8) : (C < 1 || C > MAXR)) return DU_ERR_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" int64_t du_ds_loss_ws_elems(int mode, int B, int C, int H, int W, int S, const int* hs, const int* wd, const float* weights) {
  if (ds_mode_ok(mode, C) != 0) return 0;
  DsTable d;
  int total;
  if (ds_table(d, nullptr, nullptr, nullptr, B, H, W, S, hs, wd, weights, false, total) != 0) return 0;
  return (int64_t)total * (2 + 3 * (mode == 0 ? C - 1 : C));
}

extern "C" int du_ds_loss_sums(int mode, const float* const* logits, const int64_t* target, const int64_t* table, float* sums, int B, int C,
                               int H, int W, int S, const int* hs, const int* wd, const float* weights, int has_ignore,
                               int64_t ignore_label, float* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sums || !ws || (has_ignore != 0 && has_ignore != 1) || (mode == 1 && !table)) return DU_ERR_BAD_ARG;
  if (int rc = ds_mode_ok(mode, C)) return rc;
  DsTable d;
  int total;
  if (int rc = ds_table(d, logits, nullptr, target, B, H, W, S, hs, wd, weights, false, total)) return rc;
  const int CD = mode == 0 ? C - 1 : C;
  if (ws_elems < (int64_t)total * (2 + 3 * CD)) return DU_ERR_BAD_ARG;
  const int64_t ignore = has_ignore ? ignore_label : DS_NO_IGNORE;
  if (mode == 0) {
#define CALL(KK) hipLaunchKernelGGL((ds_partial_kernel<false, KK>), dim3(total), dim3(256), 0, st, d, target, table, ws, ignore); \
                 hipLaunchKernelGGL(ds_rows_sum_kernel<KK - 1>, dim3(S), dim3(256), 0, st, d, (const float*)ws, sums)
    LOSS_SWITCH(C, 2, CALL)
#undef CALL
  } else {
#define CALL(RR) hipLaunchKernelGGL((ds_partial_kernel<true, RR>), dim3(total), dim3(256), 0, st, d, target, table, ws, ignore); \
                 hipLaunchKernelGGL(ds_rows_sum_kernel<RR>, dim3(S), dim3(256), 0, st, d, (const float*)ws, sums)
    LOSS_SWITCH(C, 1, CALL)
#undef CALL
  }
  return du_check_launch();
}

extern "C" int du_ds_loss_finish(int mode, const float* sums, float* loss, float* coef, int C, int S, const float* weights, int has_ignore,
                                 float smooth, float grad_mult, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !loss || !coef || !weights || S < 1 || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (S > DS_MAX) return DU_ERR_UNSUPPORTED;
  if (int rc = ds_mode_ok(mode, C)) return rc;
  DsTable d;
  d.S = S; d.B = 0; d.H = 0; d.W = 0;
  bool any = false;
  for (int s = 0; s < DS_MAX; s++) {
    d.s[s] = DsScale{nullptr, nullptr, 1, 1, 0, 0, 0, 1.0, 1.0};
    d.wgt[s] = s < S ? weights[s] : 0.f;
    any = any || d.wgt[s] != 0.f;
  }
  if (!any) return DU_ERR_BAD_ARG;
  hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(64), 0, st, d, sums, loss, coef, mode == 0 ? C - 1 : C, mode, has_ignore, smooth,
                     grad_mult);
  return du_check_launch();
}

extern "C" int du_ds_loss_bwd(int mode, const float* const* logits, const int64_t* target, const int64_t* table, const float* coef,
                              const float* grad_out, float* const* dlogits, int B, int C, int H, int W, int S, const int* hs, const int* wd,
                              const float* weights, int has_ignore, int64_t ignore_label, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !dlogits || !target || !coef || (has_ignore != 0 && has_ignore != 1) || (mode == 1 && !table)) return DU_ERR_BAD_ARG;
  if (int rc = ds_mode_ok(mode, C)) return rc;
  DsTable d;
  int total;
  if (int rc = ds_table(d, logits, dlogits, target, B, H, W, S, hs, wd, weights, true, total)) return rc;
  const int64_t ignore = has_ignore ? ignore_label : DS_NO_IGNORE;
  if (mode == 0) {
#define CALL(KK) hipLaunchKernelGGL((ds_bwd_kernel<false, KK>), dim3(total), dim3(256), 0, st, d, target, table, coef, grad_out, ignore)
    LOSS_SWITCH(C, 2, CALL)
#undef CALL
  } else {
#define CALL(RR) hipLaunchKernelGGL((ds_bwd_kernel<true, RR>), dim3(total), dim3(256), 0, st, d, target, table, coef, grad_out, ignore)
    LOSS_SWITCH(C, 1, CALL)
#undef CALL
  }
  return du_check_launch();
}

extern "C" int du_downsample_seg(const int64_t* seg, int64_t* const* outs, int B, int H, int W, int S, const int* hs, const int* wd,
                                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!seg || !outs || !hs || !wd || B <= 0 || H <= 0 || W <= 0 || S < 1) return DU_ERR_BAD_ARG;
  if (S > DS_MAX || H > 32768 || W > 32768) return DU_ERR_UNSUPPORTED;
  DsSegTable d;
  d.S = S; d.H = H; d.W = W;
  long end = 0;
  for (int s = 0; s < DS_MAX; s++) {
    d.out[s] = nullptr; d.h[s] = 1; d.w[s] = 1; d.zy[s] = 1.0; d.zx[s] = 1.0;
    if (s < S) {
      if (!outs[s] || hs[s] <= 0 || wd[s] <= 0 || hs[s] > H || wd[s] > W) return DU_ERR_BAD_ARG;
      d.out[s] = outs[s]; d.h[s] = hs[s]; d.w[s] = wd[s];
      d.zy[s] = (double)H / (double)hs[s]; d.zx[s] = (double)W / (double)wd[s];
      end += (long)B * hs[s] * wd[s];
    }
    d.end[s] = end;
  }
  hipLaunchKernelGGL(ds_downsample_seg_kernel, dim3(elem_grid(end)), dim3(256), 0, st, d, seg);
  return du_check_launch();
}
