// Sliding-window inference over a LIST of cases: the two passes around the network's forward when one window batch holds
// windows of several cases (inference._window_loop_cases).
//   du_window_gather: the window batch x (slots, C, ph, pw) straight from the cases' (C, D, H, W) volumes.  pad_nd_image's centred zero padding
//     (predict_from_raw_data.py:680-727) is folded in -- a source position outside the image reads as 0 -- so no padded copy of a case exists;
//     slots nb .. slots-1 (the ragged tail of a captured forward's static buffer) are written as zeros.  A pure copy.
//     Per window: reads at most C ph pw 4 bytes, writes C ph pw 4 bytes; 16 bytes per lane where the source row position is on 16 bytes and
//     inside the image, guarded elements otherwise (odd W, shifted x0, the padding's edge).
//   du_window_accumulate_cases: predicted_logits[sl] += prediction * gaussian; n_predictions[sl] += gaussian (:607-610) for every window of the
//     batch, WITHOUT float atomics.  An accumulator element is owned by the lane of the lowest slot of the launch that covers it; that lane reads
//     it once, adds the contributions of all covering slots in slot order -- acc = fadd(acc, fmul(logit, g)), never fused -- and writes it once.
//     Launches of one stream are ordered and the slots of a launch are in the reference's window order, so every element sees the additions of
//     the reference's sequential loop, in its order, in fp32: equal to the bit, whatever other cases share the batch.
//     Per window: reads K ph pw 4 (logits) + ph pw 4 (importance map, cache resident) and reads + writes (K + 1) ph pw 4 bytes of accumulators
//     (less where windows of one launch overlap: the element moves once for all of them).  The descriptors (<= 64 x 16 bytes) sit in LDS; which
//     slots can meet this block's window at all is one wave ballot, so a lane tests 0-8 rectangles, not 64.
#include "common.h"

// The product is rounded, then added: the reference's two torch ops, never a fused multiply-add.  The header's __fmul_rn / __fadd_rn are
// compiled under the default contraction mode and fuse once inlined, hence these two, under the pragma (and -ffp-contract=off, _build.py).
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

constexpr int MAX_NB = 64;       // one ballot bit per slot

// pointers out of a device table: global address space by hand (the compiler would emit flat accesses, csrc/ensemble.hip)
#define DU_GLOBAL __attribute__((address_space(1)))
typedef float f32x4g __attribute__((ext_vector_type(4)));

// One lane: V adjacent columns of one row of one channel of one slot.  VEC (pw % 4 == 0, x on 16 bytes): a 16-byte store, and a 16-byte load
// where the four source columns are inside the image and on 16 bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const void* const* __restrict__ cases, const int* __restrict__ geom,
                                                            const int4* __restrict__ desc, float* __restrict__ x, int ncases, int nb, int slots,
                                                            int C, int ph, int pw) {
  constexpr int V = VEC ? 4 : 1;
  const int qw = pw / V;
  const long per_c = (long)ph * qw, per_slot = per_c * C, total = per_slot * slots;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int s = (int)(i / per_slot);
    const long r = i - (long)s * per_slot;
    const int c = (int)(r / per_c);
    const int r2 = (int)(r - (long)c * per_c);
    const int y = r2 / qw, xo = (r2 - y * qw) * V;
    float v[V];
#pragma unroll
    for (int j = 0; j < V; j++) v[j] = 0.f;
    if (s < nb) {
      const int4 w = desc[s];                                             // (case, d, y0, x0), the origin in the padded frame
      if ((unsigned)w.x < (unsigned)ncases) {
        const int D = geom[3 * w.x], H = geom[3 * w.x + 1], W = geom[3 * w.x + 2];
        const int lo_y = ((H > ph ? H : ph) - H) / 2, lo_x = ((W > pw ? W : pw) - W) / 2;
        const int sy = w.z + y - lo_y, sx = w.w + xo - lo_x;
        if ((unsigned)w.y < (unsigned)D && (unsigned)sy < (unsigned)H) {
          const DU_GLOBAL float* row = (const DU_GLOBAL float*)cases[w.x] + (((long)c * D + w.y) * H + sy) * W;
          if (VEC && sx >= 0 && sx + V <= W && (reinterpret_cast<uintptr_t>(row + sx) & 15) == 0) {
            const f32x4g t = *reinterpret_cast<const DU_GLOBAL f32x4g*>(row + sx);
#pragma unroll
            for (int j = 0; j < V; j++) v[j] = t[j];
          } else {
#pragma unroll
            for (int j = 0; j < V; j++) v[j] = (unsigned)(sx + j) < (unsigned)W ? row[sx + j] : 0.f;
          }
        }
      }
    }
    float* o = x + (((long)s * C + c) * ph + y) * pw + xo;
    if constexpr (VEC) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else o[0] = v[0];
  }
}

__device__ __forceinline__ bool desc_ok(const int4 w, const int* __restrict__ geom, int ncases, int ph, int pw) {
  if ((unsigned)w.x >= (unsigned)ncases) return false;
  const int D = geom[3 * w.x], H = geom[3 * w.x + 1], W = geom[3 * w.x + 2];
  const int Hp = H > ph ? H : ph, Wp = W > pw ? W : pw;
  return (unsigned)w.y < (unsigned)D && w.z >= 0 && w.z <= Hp - ph && w.w >= 0 && w.w <= Wp - pw;
}

// blockIdx.y = slot b, blockIdx.x strides over the window's ph pw elements; one lane per element, all K planes and the weight plane.
// A slot whose descriptor does not fit its case is skipped, as owner and as contributor: nothing is read or written through it.
__global__ __launch_bounds__(256) void window_accumulate_cases_kernel(const float* __restrict__ logits, const float* __restrict__ gauss,
                                                                      const int4* __restrict__ desc, const int* __restrict__ geom,
                                                                      float* const* __restrict__ preds, float* const* __restrict__ npreds,
                                                                      int ncases, int nb, int K, int ph, int pw) {
  __shared__ int4 sd[MAX_NB];
  if (threadIdx.x < MAX_NB) {
    int4 w = make_int4(-1, 0, 0, 0);
    if ((int)threadIdx.x < nb) {
      w = desc[threadIdx.x];
      if (!desc_ok(w, geom, ncases, ph, pw)) w.x = -1;
    }
    sd[threadIdx.x] = w;
  }
  __syncthreads();
  const int b = blockIdx.y;
  const int4 me = sd[b];
  if (me.x < 0) return;
  // the slots that can meet this window: same case and slice, rectangles overlap.  One bit per slot, the same in every wave.
  const int lane = threadIdx.x & 63;
  const int4 ot = sd[lane];
  const bool meets = lane != b && ot.x == me.x && ot.y == me.y && abs(ot.z - me.z) < ph && abs(ot.w - me.w) < pw;
  const unsigned long long mask = __ballot(meets);
  const unsigned long long before = mask & ((1ull << b) - 1ull), after = mask & ~((2ull << b) - 1ull);

  const int D = geom[3 * me.x], H = geom[3 * me.x + 1], W = geom[3 * me.x + 2];
  const int Hp = H > ph ? H : ph, Wp = W > pw ? W : pw;
  const long plane = (long)D * Hp * Wp;
  const int per = ph * pw;
  DU_GLOBAL float* pred = (DU_GLOBAL float*)preds[me.x];
  DU_GLOBAL float* npred = (DU_GLOBAL float*)npreds[me.x];
  for (int r = blockIdx.x * 256 + threadIdx.x; r < per; r += gridDim.x * 256) {
    const int y = r / pw, x = r - y * pw;
    const int Y = me.z + y, X = me.w + x;
    bool owned = true;
    for (unsigned long long m = before; m; m &= m - 1) {                  // a lower slot covers the element: its lane owns it
      const int4 o = sd[__builtin_ctzll(m)];
      if ((unsigned)(Y - o.z) < (unsigned)ph && (unsigned)(X - o.w) < (unsigned)pw) { owned = false; break; }
    }
    if (!owned) continue;
    unsigned long long cover = 0;                                        // the later slots that cover it, added after this one in slot order
    for (unsigned long long m = after; m; m &= m - 1) {
      const int j = __builtin_ctzll(m);
      const int4 o = sd[j];
      if ((unsigned)(Y - o.z) < (unsigned)ph && (unsigned)(X - o.w) < (unsigned)pw) cover |= 1ull << j;
    }
    const long e = ((long)me.y * Hp + Y) * Wp + X;
    const float g = gauss[r];
    {
      float acc = add_rn(npred[e], g);
      for (unsigned long long m = cover; m; m &= m - 1) {
        const int4 o = sd[__builtin_ctzll(m)];
        acc = add_rn(acc, gauss[(Y - o.z) * pw + (X - o.w)]);
      }
      npred[e] = acc;
    }
    for (int k = 0; k < K; k++) {
      float acc = pred[(long)k * plane + e];
      acc = add_rn(acc, mul_rn(logits[((long)b * K + k) * per + r], g));
      for (unsigned long long m = cover; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        const int4 o = sd[j];
        const int rj = (Y - o.z) * pw + (X - o.w);
        acc = add_rn(acc, mul_rn(logits[((long)j * K + k) * per + rj], gauss[rj]));
      }
      pred[(long)k * plane + e] = acc;
    }
  }
}

int grid_for(long items, int cap) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > cap) g = cap; return (int)g; }

}  // namespace

extern "C" int du_window_gather(const void* const* cases, const int32_t* geom, const int32_t* desc, float* x, int ncases, int nb, int slots,
                                int C, int ph, int pw, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!cases || !geom || !desc || !x || ncases <= 0 || nb <= 0 || slots < nb || C <= 0 || ph <= 0 || pw <= 0) return DU_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(desc) & 15) return DU_ERR_BAD_ARG;
  if ((long)ph * pw >= (1l << 31) / 4) return DU_ERR_UNSUPPORTED;
  const bool vec = pw % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const long items = (long)slots * C * ph * (vec ? pw / 4 : pw);
  const int grid = grid_for(items, 8192);
  if (vec) hipLaunchKernelGGL(window_gather_kernel<true>, dim3(grid), dim3(256), 0, st, cases, (const int*)geom, (const int4*)desc, x, ncases, nb, slots, C, ph, pw);
  else hipLaunchKernelGGL(window_gather_kernel<false>, dim3(grid), dim3(256), 0, st, cases, (const int*)geom, (const int4*)desc, x, ncases, nb, slots, C, ph, pw);
  return du_check_launch();
}

extern "C" int du_window_accumulate_cases(const float* logits, const float* gauss, const int32_t* desc, const int32_t* geom, float* const* preds,
                                          float* const* npreds, int ncases, int nb, int K, int ph, int pw, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!logits || !gauss || !desc || !geom || !preds || !npreds || ncases <= 0 || nb <= 0 || K <= 0 || ph <= 0 || pw <= 0) return DU_ERR_BAD_ARG;
  if (reinterpret_cast<uintptr_t>(desc) & 15) return DU_ERR_BAD_ARG;
  if (nb > MAX_NB || (long)ph * pw >= (1l << 31) / 4) return DU_ERR_UNSUPPORTED;
  const int gx = grid_for((long)ph * pw, 1024);
  hipLaunchKernelGGL(window_accumulate_cases_kernel, dim3(gx, nb), dim3(256), 0, st, logits, gauss, (const int4*)desc, (const int*)geom, preds, npreds,
                     ncases, nb, K, ph, pw);
  return du_check_launch();
}
