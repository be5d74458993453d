// The fused segmentation losses with the options of the reference's loss classes (DC_and_CE_loss / DC_and_BCE_loss weight_ce and
// weight_dice, compound_losses.py:8-99; MemoryEfficientSoftDiceLoss batch_dice and do_bg, dice.py:58-119; RobustCrossEntropyLoss
// weight = nn.CrossEntropyLoss's class weights, robust_ce_loss.py).  The trainer's defaults keep the kernels of loss.hip; these serve
// every other setting, softmax (2..8 classes) and sigmoid regions (1..8), each with and without an ignore label:
//   CE   = sum_valid w_t (-log p_t) / sum_valid w_t       (w = 1 without class weights: the mean over the valid pixels; exactly 0 when
//          the denominator is 0, decided on the device);  regions: the BCE of loss.hip
//   Dice = mean over (rows, Dice classes) of (2 I + s) / clip(G + P + s, 1e-8), rows = 1 (batch Dice: the sums run over the batch) or B
//          (per-sample Dice: one row per image); the Dice classes are 1..K-1, 0..K-1 with do_bg, or the R regions
//   loss = weight_ce CE - weight_dice Dice
// Layout.  Every block works inside ONE image: image b owns the blocks b G .. b G + G - 1, G = blocks per image = a function of the
// shape alone.  First stage: one partial row per block, [sum w_t nll, sum w_t (regions: n_valid), (I_c, P_c, G_c) c < CD].  Second stage:
// per-sample Dice: block b adds the G rows of image b -> sums (B, NS); batch Dice: one block adds all B G rows -> sums (1, NS)
// (thread_rows_sum's fixed order in both).  No float atomics, so the result is bit-reproducible across calls and graph replays.
// Finish: coef = [rows][(ca_c, cb_c) c < CD] then the CE scale.  weight_dice and the mean divisor (CD rows) are folded into ca / cb,
// weight_ce into the CE scale, so the backward pass knows nothing of the weights; a weight of 0 writes exact zeros.  Backward: one
// pass, a block reads the coefficient row of its image (uniform loads) and the pixel's CE scale is the scale times w_t.
#include "common.h"
#include "loss_common.h"

namespace {

constexpr int OPT_SUMS_CAP = 2048;     // blocks of a sums pass over all images (masked_grid's cap), shared out per image
constexpr int OPT_BWD_CAP = 8192;      // ... of a backward pass (elem_grid's cap)

// blocks per image: `per_block` quads each (512 sums: two per lane, 256 backward) until the cap / B binds
int opt_img_blocks(int B, int64_t HW, int per_block, int cap) {
  const long nq = (HW + 3) / 4;
  long g = (nq + per_block - 1) / per_block, c = cap / B;
  if (c < 1) c = 1;
  if (g < 1) g = 1;
  if (g > c) g = c;
  return (int)g;
}

template <int K, bool BG>
__global__ __launch_bounds__(256) void opt_softmax_partial_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                  const float* __restrict__ class_w, float* __restrict__ part, int G,
                                                                  long HW, int has_ignore, int64_t ignore, bool vec) {
  constexpr int CD = BG ? K : K - 1, NS = 2 + 3 * CD, C0 = K - CD;
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  float w[K];
#pragma unroll
  for (int k = 0; k < K; k++) w[k] = class_w ? class_w[k] : 1.f;
  const int b = (int)blockIdx.x / G, g = (int)blockIdx.x - b * G;
  const long nq = (HW + 3) >> 2;
  const float* lb = logits + (long)b * K * HW;
  const int64_t* tb = target + (long)b * HW;
  for (long q = (long)g * 256 + threadIdx.x; q < nq; q += (long)G * 256) {
    const long r0 = q * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; k++) ld4f(lb + (long)k * HW + r0, vec, n, v[k]);
    int64_t t[4];
    ld4l(tb + r0, vec, n, 0, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool valid = j < n && !(has_ignore && t[j] == ignore);
      float x[K];
#pragma unroll
      for (int k = 0; k < K; k++) x[k] = v[k][j];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; k++) mx = fmaxf(mx, x[k]);
      float e[K], se = 0.f, xt = mx, wt = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) { e[k] = __expf(x[k] - mx); se += e[k]; if (k == t[j]) { xt = x[k]; wt = w[k]; } }
      const float inv = 1.f / se;
      const float wv = valid ? wt : 0.f;
      acc[0] += valid ? wt * softmax_nll(mx, xt, se) : 0.f;
      acc[1] += wv;
#pragma unroll
      for (int k = C0; k < K; k++) {
        const float pk = e[k] * inv;
        const bool hit = valid && k == t[j];
        acc[2 + 3 * (k - C0)] += hit ? pk : 0.f;
        acc[2 + 3 * (k - C0) + 1] += valid ? pk : 0.f;
        acc[2 + 3 * (k - C0) + 2] += hit ? 1.f : 0.f;
      }
    }
  }
  block_partial_store<NS>(acc, part);
}

template <int R>
__global__ __launch_bounds__(256) void opt_sigmoid_partial_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                  float* __restrict__ part, int G, long HW, int ign, bool vec) {
  constexpr int NS = 2 + 3 * R;
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
  const int b = (int)blockIdx.x / G, g = (int)blockIdx.x - b * G;
  const long nq = (HW + 3) >> 2;
  const int T = R + ign;
  const float* lb = logits + (long)b * R * HW;
  const uint8_t* tb = target + (long)b * T * HW;
  for (long q = (long)g * 256 + threadIdx.x; q < nq; q += (long)G * 256) {
    const long r0 = q * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const uint32_t iw = ign ? ld4b(tb + (long)R * HW + r0, vec, n) : 0u;
    bool m[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { m[j] = j < n && ((iw >> (8 * j)) & 0xffu) == 0u; acc[1] += m[j] ? 1.f : 0.f; }
#pragma unroll
    for (int r = 0; r < R; r++) {
      float x[4];
      ld4f(lb + (long)r * HW + r0, vec, n, x);
      const uint32_t yw = ld4b(tb + (long)r * HW + r0, vec, n);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float y = ((yw >> (8 * j)) & 0xffu) ? 1.f : 0.f;
        sigmoid_elem_fwd(x[j], y, m[j], r, acc);
      }
    }
  }
  block_partial_store<NS>(acc, part);
}

// second stage of per-sample Dice: block b adds the G partial rows of image b -> row b of sums (thread_rows_sum's fixed order)
template <int NS>
__global__ __launch_bounds__(256) void opt_image_rows_sum_kernel(const float* __restrict__ part, float* __restrict__ sums, int G) {
  float acc[NS];
  thread_rows_sum<NS>(part + (long)blockIdx.x * G * NS, G, acc);
  block_partial_store<NS>(acc, sums);
}

// ONE block.  sums (rows, NS) -> loss, coef = [rows][(ca_c, cb_c) c < CD], CE scale.  Thread t takes the rows t, t + 256, .. and thread 0
// adds the 256 per-thread terms in thread order: up to 256 rows that is the index order of the rows; a fixed order for any count.
// wd / (CD rows) and grad_mult go into ca / cb, wce into the scale; wd == 0 / wce == 0 write exact zeros and leave the term out of the loss.
__global__ __launch_bounds__(256) void opt_finish_kernel(const float* __restrict__ sums, float* __restrict__ loss, float* __restrict__ coef,
                                                         int rows, int CD, int per_elem, float wce, float wd, float smooth,
                                                         float grad_mult) {
  __shared__ float sdc[256], sce[256], snv[256];
  const int NS = 2 + 3 * CD;
  const float cnt = (float)CD * (float)rows;
  const float invc = wd / cnt;
  float dc = 0.f, ce = 0.f, nv = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* s = sums + (long)r * NS;
    float* cf = coef + (long)r * 2 * CD;
    ce += s[0];
    nv += s[1];
    for (int c = 0; c < CD; c++) {
      const float I = s[2 + 3 * c], P = s[2 + 3 * c + 1], G = s[2 + 3 * c + 2];
      const float num = 2.f * I + smooth;
      const float raw = G + P + smooth;
      const float den = fmaxf(raw, 1e-8f);
      dc += num / den;
      cf[2 * c] = wd != 0.f ? -2.f * invc / den * grad_mult : 0.f;
      cf[2 * c + 1] = (wd != 0.f && raw > 1e-8f) ? num / (den * den) * invc * grad_mult : 0.f;
    }
  }
  sdc[threadIdx.x] = dc; sce[threadIdx.x] = ce; snv[threadIdx.x] = nv;
  __syncthreads();
  if (threadIdx.x == 0) {
    float dct = 0.f, cet = 0.f, nvt = 0.f;
    const int nt = rows < 256 ? rows : 256;
    for (int i = 0; i < nt; i++) { dct += sdc[i]; cet += sce[i]; nvt += snv[i]; }
    const float scale = nvt > 0.f ? 1.f / (per_elem ? nvt * (float)CD : nvt) : 0.f;
    coef[(long)rows * 2 * CD] = wce != 0.f ? scale * wce : 0.f;
    const float lce = wce != 0.f ? wce * (cet * scale) : 0.f;
    const float ldc = wd != 0.f ? wd * (dct / cnt) : 0.f;
    loss[0] = lce - ldc;
  }
}

// the softmax backward text of dice_ce_masked_bwd_kernel (loss.hip); the pixel's CE scale is the scale times w_t, the Dice coefficients
// are the row of the block's image (cstride = 2 CD per-sample, 0 batch Dice), cd of the K classes have a Dice term (the last cd)
template <int K>
__global__ __launch_bounds__(256) void opt_softmax_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                              const float* __restrict__ class_w, const float* __restrict__ coef,
                                                              const float* __restrict__ gout, float* __restrict__ dlogits, int G, long HW,
                                                              int has_ignore, int64_t ignore, int cd, int cstride, long scale_at, bool vec) {
  const int b = (int)blockIdx.x / G, g = (int)blockIdx.x - b * G;
  const float* cf = coef + (long)b * cstride;
  float ca[K], cb[K], w[K];
#pragma unroll
  for (int c = 0; c < K; c++) {
    const int q = c - (K - cd);
    ca[c] = q >= 0 ? cf[2 * q] : 0.f;
    cb[c] = q >= 0 ? cf[2 * q + 1] : 0.f;
    w[c] = class_w ? class_w[c] : 1.f;
  }
  const float ce_scale = coef[scale_at];
  const float go = gout ? gout[0] : 1.f;
  const long nq = (HW + 3) >> 2;
  const float* lb = logits + (long)b * K * HW;
  float* db = dlogits + (long)b * K * HW;
  const int64_t* tb = target + (long)b * HW;
  for (long q = (long)g * 256 + threadIdx.x; q < nq; q += (long)G * 256) {
    const long r0 = q * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    float v[K][4];
#pragma unroll
    for (int k = 0; k < K; k++) ld4f(lb + (long)k * HW + r0, vec, n, v[k]);
    int64_t t[4];
    ld4l(tb + r0, vec, n, 0, t);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool valid = !(has_ignore && t[j] == ignore);
      float wt = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) if (k == t[j]) wt = w[k];
      const float ce_scale_j = ce_scale * wt;
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; k++) mx = fmaxf(mx, v[k][j]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) { v[k][j] = __expf(v[k][j] - mx); se += v[k][j]; }
      const float inv = 1.f / se;
      float gg[K], dot = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) {
        v[k][j] *= inv;
        gg[k] = (k == t[j] ? ca[k] : 0.f) + cb[k];
        dot += gg[k] * v[k][j];
      }
#pragma unroll
      for (int k = 0; k < K; k++)
        v[k][j] = valid ? go * ((v[k][j] - (k == t[j] ? 1.f : 0.f)) * ce_scale_j + v[k][j] * (gg[k] - dot)) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; k++) st4f(db + (long)k * HW + r0, vec, n, v[k]);
  }
}

template <int R>
__global__ __launch_bounds__(256) void opt_sigmoid_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ target,
                                                              const float* __restrict__ coef, const float* __restrict__ gout,
                                                              float* __restrict__ dlogits, int G, long HW, int ign, int cstride,
                                                              long scale_at, bool vec) {
  const int b = (int)blockIdx.x / G, g = (int)blockIdx.x - b * G;
  const float* cf = coef + (long)b * cstride;
  const float bce_scale = coef[scale_at];
  const float go = gout ? gout[0] : 1.f;
  const long nq = (HW + 3) >> 2;
  const int T = R + ign;
  const float* lb = logits + (long)b * R * HW;
  float* db = dlogits + (long)b * R * HW;
  const uint8_t* tb = target + (long)b * T * HW;
  for (long q = (long)g * 256 + threadIdx.x; q < nq; q += (long)G * 256) {
    const long r0 = q * 4;
    const int n = vec ? 4 : (int)min(4L, HW - r0);
    const uint32_t iw = ign ? ld4b(tb + (long)R * HW + r0, vec, n) : 0u;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float ca = cf[2 * r], cb = cf[2 * r + 1];
      float x[4];
      ld4f(lb + (long)r * HW + r0, vec, n, x);
      const uint32_t yw = ld4b(tb + (long)r * HW + r0, vec, n);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool m = ((iw >> (8 * j)) & 0xffu) == 0u;
        const float y = ((yw >> (8 * j)) & 0xffu) ? 1.f : 0.f;
        x[j] = m ? sigmoid_elem_bwd(x[j], y, ca, cb, bce_scale, go) : 0.f;
      }
      st4f(db + (long)r * HW + r0, vec, n, x);
    }
  }
}

bool flag01(int v) { return v == 0 || v == 1; }
bool weight_ok(float w) { return w >= 0.f && w <= 3.0e38f; }      // finite and not negative (a NaN fails both comparisons)

// the option block alone: DU_OK, DU_ERR_BAD_ARG (a contradiction) or DU_ERR_UNSUPPORTED (a class / region count without a kernel)
int opt_check(const du_loss_opt* o) {
  if (!o) return DU_ERR_BAD_ARG;
  if (!flag01(o->regions) || !flag01(o->has_ignore) || !flag01(o->do_bg) || !flag01(o->batch_dice)) return DU_ERR_BAD_ARG;
  if (!weight_ok(o->weight_ce) || !weight_ok(o->weight_dice) || (o->weight_ce == 0.f && o->weight_dice == 0.f)) return DU_ERR_BAD_ARG;
  if (o->regions && (o->class_w || !o->do_bg)) return DU_ERR_BAD_ARG;
  if (o->regions ? (o->n < 1 || o->n > 8) : (o->n < 2 || o->n > 8)) return DU_ERR_UNSUPPORTED;
  return DU_OK;
}
int opt_cd(const du_loss_opt* o) { return (o->regions || o->do_bg) ? o->n : o->n - 1; }

}  // namespace

extern "C" int64_t du_loss_opt_ws_elems(const du_loss_opt* o, int B, int64_t HW) {
  if (opt_check(o) != DU_OK || B <= 0 || HW <= 0) return 0;
  return (int64_t)B * opt_img_blocks(B, HW, 512, OPT_SUMS_CAP) * (2 + 3 * opt_cd(o));
}

// sums (rows, 2 + 3 CD) fp32, rows = 1 (batch_dice) or B
extern "C" int du_loss_opt_sums(const du_loss_opt* o, const float* logits, const void* target, float* sums, int B, int64_t HW, float* ws,
                                int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!o || !logits || !target || !sums || !ws || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  const int rc = opt_check(o);
  if (rc != DU_OK) return rc;
  const int G = opt_img_blocks(B, HW, 512, OPT_SUMS_CAP), grid = B * G;
  if (ws_elems < (int64_t)grid * (2 + 3 * opt_cd(o))) return DU_ERR_BAD_ARG;
  const int batch = o->batch_dice;
#define SECOND(NSV) if (batch) hipLaunchKernelGGL(partial_rows_sum_kernel<NSV>, dim3(1), dim3(256), 0, st, (const float*)ws, sums, grid); \
                    else hipLaunchKernelGGL(opt_image_rows_sum_kernel<NSV>, dim3(B), dim3(256), 0, st, (const float*)ws, sums, G)
  if (o->regions) {
    const uint8_t* tg = (const uint8_t*)target;
    const bool vec = HW % 4 == 0 && al(logits, 16) && al(tg, 4);
    const int ign = o->has_ignore;
#define CALL(RR) hipLaunchKernelGGL(opt_sigmoid_partial_kernel<RR>, dim3(grid), dim3(256), 0, st, logits, tg, ws, G, (long)HW, ign, vec); \
                 SECOND(2 + 3 * RR)
    LOSS_SWITCH(o->n, 1, CALL)
#undef CALL
  } else {
    const int64_t* tg = (const int64_t*)target;
    const bool vec = HW % 4 == 0 && al(logits, 16) && al(tg, 16);
    const float* cw = o->class_w;
    const int ign = o->has_ignore;
    const int64_t ignore = o->ignore;
    if (o->do_bg) {
#define CALL(KK) hipLaunchKernelGGL((opt_softmax_partial_kernel<KK, true>), dim3(grid), dim3(256), 0, st, logits, tg, cw, ws, G, (long)HW, ign, ignore, vec); \
                 SECOND(2 + 3 * KK)
      LOSS_SWITCH(o->n, 2, CALL)
#undef CALL
    } else {
#define CALL(KK) hipLaunchKernelGGL((opt_softmax_partial_kernel<KK, false>), dim3(grid), dim3(256), 0, st, logits, tg, cw, ws, G, (long)HW, ign, ignore, vec); \
                 SECOND(2 + 3 * (KK - 1))
      LOSS_SWITCH(o->n, 2, CALL)
#undef CALL
    }
  }
#undef SECOND
  return du_check_launch();
}

// loss (1 float); coef (rows 2 CD + 1 floats); grad_mult = world size when the Dice columns of a batch-Dice sums row were all-reduced
extern "C" int du_loss_opt_finish(const du_loss_opt* o, const float* sums, float* loss, float* coef, int B, float smooth, float grad_mult,
                                  void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!o || !sums || !loss || !coef || B <= 0) return DU_ERR_BAD_ARG;
  const int rc = opt_check(o);
  if (rc != DU_OK) return rc;
  const int rows = o->batch_dice ? 1 : B;
  hipLaunchKernelGGL(opt_finish_kernel, dim3(1), dim3(256), 0, st, sums, loss, coef, rows, opt_cd(o), (o->regions && !o->has_ignore) ? 1 : 0,
                     o->weight_ce, o->weight_dice, smooth, grad_mult);
  return du_check_launch();
}

// dlogits = grad_out[0] * d loss / d logits (grad_out: device scalar, NULL = 1); exactly 0 in every channel of an ignored pixel
extern "C" int du_loss_opt_bwd(const du_loss_opt* o, const float* logits, const void* target, const float* coef, const float* grad_out,
                               float* dlogits, int B, int64_t HW, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!o || !logits || !target || !coef || !dlogits || B <= 0 || HW <= 0) return DU_ERR_BAD_ARG;
  const int rc = opt_check(o);
  if (rc != DU_OK) return rc;
  const int G = opt_img_blocks(B, HW, 256, OPT_BWD_CAP), grid = B * G;
  const int cd = opt_cd(o), rows = o->batch_dice ? 1 : B;
  const int cstride = o->batch_dice ? 0 : 2 * cd;
  const long scale_at = (long)rows * 2 * cd;
  if (o->regions) {
    const uint8_t* tg = (const uint8_t*)target;
    const bool vec = HW % 4 == 0 && al(logits, 16) && al(tg, 4) && al(dlogits, 16);
#define CALL(RR) hipLaunchKernelGGL(opt_sigmoid_bwd_kernel<RR>, dim3(grid), dim3(256), 0, st, logits, tg, coef, grad_out, dlogits, G, (long)HW, o->has_ignore, cstride, scale_at, vec)
    LOSS_SWITCH(o->n, 1, CALL)
#undef CALL
  } else {
    const int64_t* tg = (const int64_t*)target;
    const bool vec = HW % 4 == 0 && al(logits, 16) && al(tg, 16) && al(dlogits, 16);
#define CALL(KK) hipLaunchKernelGGL(opt_softmax_bwd_kernel<KK>, dim3(grid), dim3(256), 0, st, logits, tg, o->class_w, coef, grad_out, dlogits, G, (long)HW, o->has_ignore, o->ignore, cd, cstride, scale_at, vec)
    LOSS_SWITCH(o->n, 2, CALL)
#undef CALL
  }
  return du_check_launch();
}
