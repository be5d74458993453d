// Top-k cross-entropy and Dice + top-k of the reference's loss package on fp32 NCHW logits:
//   TopKLoss (dinounet/training/loss/robust_ce_loss.py:19-32): v = cross_entropy(reduction="none", ignore_index), the mean of the
//     k_vox = int(N k / 100) largest v over all N = B HW voxels (an ignored voxel has v = 0 and counts in N);
//   DC_and_topk_loss (compound_losses.py:102-150) = TopKLoss + SoftDiceLoss(softmax, batch_dice, do_bg=False, smooth), the Dice sums
//     multiplied by the mask m = [t != ignore]: 2tp + fp + fn = P_c + G_c, so the Dice term is the (I_c, P_c, G_c) sums and coefficients
//     of the masked Dice + CE loss (csrc/loss.hip), same layout, same all-reduce of sums[2:], same grad_mult.
// The k largest are found by a radix select on the raw bits of v (v >= +0, so the bits order as unsigned integers), as the dataset
// fingerprint's order statistics do (csrc/fingerprint.hip): no sort, no read-back, k_vox is a launch argument, the whole loss captures.
//   values   one pass over the logits (the 4-pixels-per-lane structure of the masked kernels): v -> values (B HW) fp32, the per-block
//            partial rows of the sums, the histogram of key >> 20 (2048 bins; LDS counters, integer atomics to global)
//   sweep    twice over the values alone (4 B per voxel): every workgroup first picks the digit of the k-th largest key from the previous
//            level's histogram (one scan over 2048 / 1024 bins, the same result in every workgroup; workgroup 0 records it), then counts
//            the next 10 bits of the keys that carry the prefix
//   count    picks the last digit -> T = the k-th largest value, cnt_gt = #{v > T}, need = k_vox - cnt_gt; per wave, over its contiguous
//            range of the flat index: sum of v > T (fixed order) and the number of v == T
//   finish   ONE workgroup: exclusive scan of the per-wave tie counts, the wave sums added in fp64 in fixed order,
//            loss = (sum_{v > T} v + need T) / k_vox - mean_c dice_c, the Dice backward coefficients
//   select   uint8 map (B HW): [v > T] or (v == T and fewer than `need` ties at lower flat indices): exactly k_vox voxels, ties to the
//            lowest index (b, y, x order).  torch.topk leaves that choice open; the loss value does not depend on it.
//   backward one pass, softmax recomputed: dlogits = go ((p - onehot) sel / k_vox + the masked Dice term); the selection is READ from the
//            map, never recomputed, so it cannot round differently from the forward pass.
// Integer sums do not depend on order and every float sum has a fixed order: no float atomics, bit-reproducible across calls and replays.
#include "common.h"
#include "loss_common.h"

namespace {

constexpr int L1_BINS = 2048, LX_BINS = 1024;        // key >> 20 (sign bit 0: 11 significant bits), then 10 + 10 bits
constexpr int HIST_WORDS = L1_BINS + 2 * LX_BINS;
constexpr int STATE_WORDS = 16;                      // three slots of (prefix, rem, cnt_gt, -), one per pick
constexpr int MAX_WAVES = 4096;                      // waves of a sweep launch (1024 workgroups); the finish kernel stages one entry per wave in LDS

// 4 consecutive keys of the flat values buffer from index i (a multiple of 4); n = how many of them exist
__device__ __forceinline__ void ld4k(const uint32_t* __restrict__ keys, long i, int n, bool vec, uint32_t o[4]) {
  if (vec && n == 4) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + i);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = j < n ? keys[i + j] : 0u;
  }
}

__global__ __launch_bounds__(256) void topk_init_kernel(uint32_t* __restrict__ hist_state, int words) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) hist_state[i] = 0u;
}

// sums layout of the masked loss: [sum of v, n_valid, (I_c, P_c, G_c) c = 1..K-1]
template <int K>
__global__ __launch_bounds__(256) void topk_values_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                          float* __restrict__ values, float* __restrict__ part,
                                                          uint32_t* __restrict__ hist1, int B, long HW, int64_t ignore, bool vec) {
  constexpr int NS = 2 + 3 * (K - 1);
  __shared__ uint32_t h[L1_BINS];
  for (int i = threadIdx.x; i < L1_BINS; i += 256) h[i] = 0u;
  __syncthreads();
  float acc[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) acc[i] = 0.f;
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
    float ce[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float x[K];
#pragma unroll
      for (int k = 0; k < K; k++) x[k] = v[k][j];
      const bool valid = t[j] != ignore;
      // +0 for an ignored voxel, for -0 and for a nan: the bits order as integers
      ce[j] = softmax_pixel_fwd<K>(x, t[j], valid, acc, [&](float nll) { return (nll > 0.f && valid) ? nll : 0.f; });
    }
    st4f(values + b * HW + r0, vec, n, ce);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < n) atomicAdd(&h[__builtin_bit_cast(uint32_t, ce[j]) >> 20], 1u);      // the padding of a partial quad is no voxel
  }
  block_partial_store<NS>(acc, part);                     // (its barrier also ends the LDS counting)
  for (int i = threadIdx.x; i < L1_BINS; i += 256) {
    const uint32_t s = h[i];
    if (s) atomicAdd(&hist1[i], s);
  }
}

// inclusive scan over the 256 threads of the workgroup; *total = the sum of all 256
__device__ __forceinline__ int block_scan(int v, int* red, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();                                        // the previous round's reads of red are over
  if (lane == 63) red[w] = v;
  __syncthreads();
  const int a = red[0], b = red[1], c = red[2], d = red[3];
  *total = a + b + c + d;
  return v + (w > 0 ? a : 0) + (w > 1 ? b : 0) + (w > 2 ? c : 0);
}

struct Pick { uint32_t prefix, rem, gt; };

// One radix step by the whole workgroup (every workgroup of a launch computes the same): among the keys that carry `in.prefix`, counted
// per next digit in hist (NB bins), the digit d of the in.rem-th largest -> prefix = (prefix << log2 NB) | d, rem and gt moved past the
// `above` keys with a larger digit.  Thread t holds the NB / 256 bins from the top down, bin = NB - 1 - (t PER + i).
template <int NB>
__device__ __forceinline__ Pick pick_digit(const uint32_t* __restrict__ hist, Pick in, int* red, uint32_t* res) {
  constexpr int PER = NB / 256;
  constexpr int BITS = NB == 2048 ? 11 : 10;
  const int t = threadIdx.x;
  int c[PER], s = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) { c[i] = (int)hist[NB - 1 - (t * PER + i)]; s += c[i]; }
  if (t == 0) { res[0] = 0u; res[1] = 0u; }
  int total;
  const int inc = block_scan(s, red, &total), exc = inc - s;      // (two barriers: res is cleared before anyone writes it)
  const int rem = (int)in.rem;
  if (s > 0 && exc < rem && rem <= inc) {                          // exactly one thread while 1 <= rem <= total
    int run = exc;
    bool done = false;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (!done && run + c[i] >= rem) { res[0] = (uint32_t)(NB - 1 - (t * PER + i)); res[1] = (uint32_t)run; done = true; }
      if (!done) run += c[i];
    }
  }
  __syncthreads();
  Pick out;
  out.prefix = (in.prefix << BITS) | res[0];
  out.rem = in.rem - res[1];
  out.gt = in.gt + res[1];
  __syncthreads();                                                 // res may be reused
  return out;
}

__device__ __forceinline__ Pick load_pick(const uint32_t* __restrict__ state, int slot) {
  Pick p;
  p.prefix = state[slot * 4]; p.rem = state[slot * 4 + 1]; p.gt = state[slot * 4 + 2];
  return p;
}
__device__ __forceinline__ void store_pick(uint32_t* __restrict__ state, int slot, Pick p) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { state[slot * 4] = p.prefix; state[slot * 4 + 1] = p.rem; state[slot * 4 + 2] = p.gt; }
}

// LVL 2: pick the first digit from hist1, count bits 19..10 of the keys with key >> 20 == prefix into hist2;
// LVL 3: pick the second digit from hist2, count bits 9..0 of the keys with key >> 10 == prefix into hist3.
// Wave w of the launch sweeps the flat range [w CW, min(N, (w + 1) CW)), CW a multiple of 256, 4 keys per lane and step.
template <int LVL>
__global__ __launch_bounds__(256) void topk_sweep_kernel(const uint32_t* __restrict__ keys, long N, long CW, uint32_t* __restrict__ hist,
                                                         uint32_t* __restrict__ state, uint32_t k_vox, bool vec) {
  __shared__ uint32_t h[LX_BINS];
  __shared__ int red[4];
  __shared__ uint32_t res[2];
  Pick p;
  if constexpr (LVL == 2) {
    Pick in; in.prefix = 0u; in.rem = k_vox; in.gt = 0u;
    p = pick_digit<L1_BINS>(hist, in, red, res);
  } else {
    p = pick_digit<LX_BINS>(hist + L1_BINS, load_pick(state, 0), red, res);
  }
  store_pick(state, LVL - 2, p);
  uint32_t* hout = hist + (LVL == 2 ? L1_BINS : L1_BINS + LX_BINS);
  constexpr int HI = LVL == 2 ? 20 : 10, LO = LVL == 2 ? 10 : 0;
  for (int i = threadIdx.x; i < LX_BINS; i += 256) h[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long lo = w * CW, hi = min(N, lo + CW);
  for (long i = lo + lane * 4; i < hi; i += 256) {
    const int n = (int)min(4L, hi - i);
    uint32_t k4[4];
    ld4k(keys, i, n, vec, k4);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < n && (k4[j] >> HI) == p.prefix) atomicAdd(&h[(k4[j] >> LO) & (LX_BINS - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LX_BINS; i += 256) {
    const uint32_t s = h[i];
    if (s) atomicAdd(&hout[i], s);
  }
}

// picks the last digit (T = the k-th largest key; state slot 2 = (T, need, cnt_gt)); per wave: sum of the values above T, number equal to T
__global__ __launch_bounds__(256) void topk_count_kernel(const uint32_t* __restrict__ keys, long N, long CW, const uint32_t* __restrict__ hist,
                                                         uint32_t* __restrict__ state, float* __restrict__ wsum, int* __restrict__ wtie,
                                                         bool vec) {
  __shared__ int red[4];
  __shared__ uint32_t res[2];
  const Pick p = pick_digit<LX_BINS>(hist + L1_BINS + LX_BINS, load_pick(state, 1), red, res);
  store_pick(state, 2, p);
  const uint32_t T = p.prefix;
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long lo = w * CW, hi = min(N, lo + CW);
  float s = 0.f;
  int ties = 0;
  for (long i = lo + lane * 4; i < hi; i += 256) {
    const int n = (int)min(4L, hi - i);
    uint32_t k4[4];
    ld4k(keys, i, n, vec, k4);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s += (j < n && k4[j] > T) ? __builtin_bit_cast(float, k4[j]) : 0.f;
      ties += (j < n && k4[j] == T) ? 1 : 0;
    }
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ties += __shfl_xor(ties, o, 64);
  if (lane == 0) { wsum[w] = s; wtie[w] = ties; }
}

// ONE workgroup.  woff = exclusive scan of wtie (thread t owns the PERW consecutive waves from t PERW); the wave sums in fp64, fixed order;
// coef = [(ca_c, cb_c) c = 1..K-1, 1 / k_vox]; info = (T bits, need, cnt_gt, 0)
__global__ __launch_bounds__(256) void topk_finish_kernel(const float* __restrict__ sums, const uint32_t* __restrict__ state,
                                                          const float* __restrict__ wsum, const int* __restrict__ wtie,
                                                          int* __restrict__ woff, int Wn, float* __restrict__ loss, float* __restrict__ coef,
                                                          int32_t* __restrict__ info, int K, uint32_t k_vox, int dice, float smooth,
                                                          float grad_mult) {
  __shared__ int red[4];
  __shared__ double dred[4];
  __shared__ int tie_s[MAX_WAVES + MAX_WAVES / 32];        // entry e at e + e / 32: a thread's consecutive entries fall into different banks
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // every entry is loaded once, coalesced and all loads in flight together (a thread walking its own consecutive entries paid one memory
  // round trip per entry); the fp64 sum needs no contiguity: thread t adds the entries t, t + 256, ... in that order
  double s = 0.0;
  {
    int c[MAX_WAVES / 256];
    float f[MAX_WAVES / 256];
#pragma unroll
    for (int i = 0; i < MAX_WAVES / 256; i++) {
      const int e = i * 256 + t;
      c[i] = e < Wn ? wtie[e] : 0;
      f[i] = e < Wn ? wsum[e] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MAX_WAVES / 256; i++) {
      const int e = i * 256 + t;
      tie_s[e + (e >> 5)] = c[i];
      s += (double)f[i];
    }
  }
  __syncthreads();
  const int PERW = (Wn + 255) / 256;
  const int w0 = t * PERW, w1 = min(Wn, w0 + PERW);
  int cnt = 0;
  for (int w = w0; w < w1; w++) cnt += tie_s[w + (w >> 5)];
  int total;
  int run = block_scan(cnt, red, &total) - cnt;
  for (int w = w0; w < w1; w++) { woff[w] = run; run += tie_s[w + (w >> 5)]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) dred[wave] = s;
  __syncthreads();
  if (t != 0) return;
  const uint32_t T = state[8], need = state[9], gt = state[10];
  const double S = (dred[0] + dred[1]) + (dred[2] + dred[3]);
  const float ce = (float)((S + (double)need * (double)__builtin_bit_cast(float, T)) / (double)k_vox);
  float dc = 0.f;
  if (dice) {
    dc = dice_coefs(sums + 2, coef, K - 1, smooth, grad_mult);
  } else {
    for (int c = 0; c < 2 * (K - 1); c++) coef[c] = 0.f;
  }
  coef[2 * (K - 1)] = 1.f / (float)k_vox;
  loss[0] = ce - dc;
  info[0] = (int32_t)T; info[1] = (int32_t)need; info[2] = (int32_t)gt; info[3] = 0;
}

// sel[i] = [v_i > T] or (v_i == T and rank of i among the ties, by flat index, < need).  The wave ranges are those of the count kernel;
// inside a step the flat order is lane-major (lane l holds i .. i + 3), so the rank is woff + ties of the earlier steps + of the lower lanes
// + of the lane's own earlier keys.
__global__ __launch_bounds__(256) void topk_select_kernel(const uint32_t* __restrict__ keys, long N, long CW, const uint32_t* __restrict__ state,
                                                          const int* __restrict__ woff, uint8_t* __restrict__ sel, bool vec) {
  const uint32_t T = state[8];
  const int need = (int)state[9];
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long lo = w * CW, hi = min(N, lo + CW);
  if (lo >= hi) return;
  int off = woff[w];
  for (long i0 = lo; i0 < hi; i0 += 256) {                          // uniform trip count in the wave
    const long i = i0 + lane * 4;
    const int n = (int)max(0L, min(4L, hi - i));
    uint32_t k4[4] = {0u, 0u, 0u, 0u};
    if (n > 0) ld4k(keys, i, n, vec, k4);
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) c += (j < n && k4[j] == T) ? 1 : 0;
    int pre = 0, tot = 0;
    if (__ballot(c > 0) != 0ull) {                                  // wave-uniform
      int inc = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
      }
      pre = inc - c;
      tot = __shfl(inc, 63, 64);
    }
    int rank = off + pre;
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool tie = j < n && k4[j] == T;
      const bool s = j < n && (k4[j] > T || (tie && rank < need));
      rank += tie ? 1 : 0;
      word |= s ? (1u << (8 * j)) : 0u;
    }
    if (n == 4 && vec) {
      *reinterpret_cast<uint32_t*>(sel + i) = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) if (j < n) sel[i + j] = (uint8_t)(word >> (8 * j));
    }
    off += tot;
  }
}

template <int K>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                       const uint8_t* __restrict__ sel, const float* __restrict__ coef,
                                                       const float* __restrict__ gout, float* __restrict__ dlogits, int B, long HW,
                                                       int64_t ignore, bool vec) {
  float ca[K], cb[K];
  load_dice_coefs<K, K - 1>(coef, ca, cb);
  const float inv_k = coef[2 * (K - 1)];
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
    const uint32_t sw = ld4b(sel + b * HW + r0, vec, n);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool valid = t[j] != ignore;
      const float ce_scale_j = ((sw >> (8 * j)) & 0xffu) ? inv_k : 0.f;
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

// the sweeps over the flat values: G workgroups of 4 waves, wave w owns [w CW, (w + 1) CW), CW a multiple of 256
struct Sweep { int G; int Wn; long CW; };
Sweep sweep_of(int64_t N) {
  Sweep s;
  long g = (long)((N + 1023) / 1024);
  if (g < 1) g = 1;
  if (g > MAX_WAVES / 4) g = MAX_WAVES / 4;
  s.G = (int)g; s.Wn = s.G * 4;
  const long per = (long)((N + s.Wn - 1) / s.Wn);
  s.CW = (per + 255) / 256 * 256;
  return s;
}

// scratch, in 4-byte words: [values-pass partial rows | hist 2048 + 1024 + 1024 | state 16 | wsum Wn | wtie Wn | woff Wn]
struct Layout { int64_t part, hist, state, wsum, wtie, woff, total; };
Layout layout_of(int B, int K, int64_t HW) {
  Layout l;
  const Sweep s = sweep_of((int64_t)B * HW);
  l.part = 0;
  l.hist = (int64_t)masked_grid(quad_items(B, HW)) * (2 + 3 * (K - 1));
  l.hist = (l.hist + 3) / 4 * 4;
  l.state = l.hist + HIST_WORDS;
  l.wsum = l.state + STATE_WORDS;
  l.wtie = l.wsum + s.Wn;
  l.woff = l.wtie + s.Wn;
  l.total = l.woff + s.Wn;
  return l;
}

bool shape_ok(int B, int64_t HW) { return B > 0 && HW > 0 && (int64_t)B * HW < ((int64_t)1 << 31) && HW <= ((int64_t)1 << 31) / B; }

}  // namespace

extern "C" int64_t du_topk_loss_ws_elems(int B, int K, int64_t HW) {
  if (K < 2 || K > 8 || !shape_ok(B, HW)) return 0;
  return layout_of(B, K, HW).total;
}

extern "C" int du_topk_loss_fwd(const float* logits, const int64_t* target, float* values, float* sums, int B, int K, int64_t HW,
                                int has_ignore, int64_t ignore_label, int64_t k_vox, int32_t* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !values || !sums || !ws || !shape_ok(B, HW) || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  const int64_t N = (int64_t)B * HW;
  if (k_vox < 1 || k_vox > N) return DU_ERR_BAD_ARG;
  const Layout l = layout_of(B, K, HW);
  if (ws_elems < l.total || !al(ws, 16)) return DU_ERR_BAD_ARG;
  const int64_t ignore = has_ignore ? ignore_label : INT64_MIN;     // no label equals it; the padding of a partial quad carries it
  const int grid = masked_grid(quad_items(B, HW));
  const Sweep s = sweep_of(N);
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 16) && al(values, 16);
  const bool kvec = al(values, 16);
  float* part = (float*)ws + l.part;
  uint32_t* hist = (uint32_t*)ws + l.hist;
  uint32_t* state = (uint32_t*)ws + l.state;
  const uint32_t* keys = (const uint32_t*)values;
  hipLaunchKernelGGL(topk_init_kernel, dim3(4), dim3(256), 0, st, hist, HIST_WORDS + STATE_WORDS);
#define CALL(KK) hipLaunchKernelGGL(topk_values_kernel<KK>, dim3(grid), dim3(256), 0, st, logits, target, values, part, hist, B, (long)HW, ignore, vec); \
                 hipLaunchKernelGGL(partial_rows_sum_kernel<2 + 3 * (KK - 1)>, dim3(1), dim3(256), 0, st, (const float*)part, sums, grid)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  hipLaunchKernelGGL(topk_sweep_kernel<2>, dim3(s.G), dim3(256), 0, st, keys, (long)N, s.CW, hist, state, (uint32_t)k_vox, kvec);
  hipLaunchKernelGGL(topk_sweep_kernel<3>, dim3(s.G), dim3(256), 0, st, keys, (long)N, s.CW, hist, state, (uint32_t)k_vox, kvec);
  hipLaunchKernelGGL(topk_count_kernel, dim3(s.G), dim3(256), 0, st, keys, (long)N, s.CW, (const uint32_t*)hist, state,
                     (float*)ws + l.wsum, (int*)ws + l.wtie, kvec);
  return du_check_launch();
}

extern "C" int du_topk_loss_finish(const float* sums, const float* values, int32_t* ws, int64_t ws_elems, uint8_t* sel, float* loss,
                                   float* coef, int32_t* info, int B, int K, int64_t HW, int64_t k_vox, int dice, float smooth,
                                   float grad_mult, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sums || !values || !ws || !sel || !loss || !coef || !info || !shape_ok(B, HW) || (dice != 0 && dice != 1)) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  const int64_t N = (int64_t)B * HW;
  if (k_vox < 1 || k_vox > N) return DU_ERR_BAD_ARG;
  const Layout l = layout_of(B, K, HW);
  if (ws_elems < l.total || !al(ws, 16)) return DU_ERR_BAD_ARG;
  const Sweep s = sweep_of(N);
  const uint32_t* state = (const uint32_t*)ws + l.state;
  hipLaunchKernelGGL(topk_finish_kernel, dim3(1), dim3(256), 0, st, sums, state, (const float*)ws + l.wsum, (const int*)ws + l.wtie,
                     (int*)ws + l.woff, s.Wn, loss, coef, info, K, (uint32_t)k_vox, dice, smooth, grad_mult);
  hipLaunchKernelGGL(topk_select_kernel, dim3(s.G), dim3(256), 0, st, (const uint32_t*)values, (long)N, s.CW, state,
                     (const int*)ws + l.woff, sel, al(values, 16) && al(sel, 4));
  return du_check_launch();
}

extern "C" int du_topk_loss_bwd(const float* logits, const int64_t* target, const uint8_t* sel, const float* coef, const float* grad_out,
                                float* dlogits, int B, int K, int64_t HW, int has_ignore, int64_t ignore_label, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !target || !sel || !coef || !dlogits || !shape_ok(B, HW) || (has_ignore != 0 && has_ignore != 1)) return DU_ERR_BAD_ARG;
  if (K < 2 || K > 8) return DU_ERR_UNSUPPORTED;
  const int64_t ignore = has_ignore ? ignore_label : INT64_MIN;
  const int g = elem_grid(quad_items(B, HW));
  const bool vec = HW % 4 == 0 && al(logits, 16) && al(target, 16) && al(dlogits, 16) && al(sel, 4);
#define CALL(KK) hipLaunchKernelGGL(topk_bwd_kernel<KK>, dim3(g), dim3(256), 0, st, logits, target, sel, coef, grad_out, dlogits, B, (long)HW, ignore, vec)
  LOSS_SWITCH(K, 2, CALL)
#undef CALL
  return du_check_launch();
}
