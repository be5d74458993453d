// Ensembling: M member probability volumes -> the label map, optionally the averaged probabilities, in ONE streaming pass.
//   average_probabilities (dinounet/ensembling/ensemble.py:17-29): avg = p0 (widened to fp32); avg += p_m in the given order; avg /= M
//   merge_files (:32-46): the label map of that average (label_handling.py:128-175: argmax | region paint loop)
// mean[k][i] = (((p0 + p1) + p2) + ...) / M in fp32: the members in their order, one IEEE division (no reciprocal, no pairwise sum), so the
// result equals numpy's to the bit for every finite input; fp16 members widen exactly, as numpy widens them in the add.
// Reads M K 4 (fp32) or M K 2 (fp16) bytes per voxel, each member once; writes 1 byte per voxel (+ 4 K with the mean, which is never
// written when not asked for).  No LDS, no scratch, no atomics: the flag is a plain store of 1.
#include "common.h"

namespace {

constexpr int MAXC = 8, MAXM = 16;

// The member pointers come out of a table, so the compiler cannot tell their address space and would emit flat loads (an aperture check,
// and a share of the LGKM counter) for the very loads the kernel lives on: they are cast to global pointers by hand.
#define DU_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// One lane: V = 16 / sizeof(T) adjacent voxels of all C planes.  VEC: every plane of every member starts on 16 bytes and n % V == 0 (no tail):
// one 16-byte load per member and plane, word stores.  !VEC: guarded element loads and stores (members that are views starting at any
// element, n that is no multiple of V).
template <typename T, int C, bool REGION, bool VEC>
__device__ __forceinline__ void merge_body(const void* const* __restrict__ members, int M, long n, uint8_t* __restrict__ seg,
                                           float* __restrict__ mean, int* __restrict__ flag, uint64_t order) {
  constexpr int V = 16 / (int)sizeof(T);
  const long items = (n + V - 1) / V;
  const float fm = (float)M;
  bool bad = false;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long base = it * V;
    const int cnt = VEC ? V : (int)(n - base < V ? n - base : V);
    float v[C][V];
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
      for (int j = 0; j < V; j++) v[c][j] = 0.f;
    for (int m = 0; m < M; m++) {
      const DU_GLOBAL T* p = (const DU_GLOBAL T*)members[m] + base;
      float x[C][V];
#pragma unroll
      for (int c = 0; c < C; c++) {
        if constexpr (VEC) {
          const Vec16<T> t = __builtin_bit_cast(Vec16<T>, *reinterpret_cast<const DU_GLOBAL u32x4_t*>(p + c * n));
#pragma unroll
          for (int j = 0; j < V; j++) x[c][j] = (float)t.v[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; j++) x[c][j] = j < cnt ? (float)p[c * n + j] : 0.f;
        }
      }
#pragma unroll
      for (int c = 0; c < C; c++)
#pragma unroll
        for (int j = 0; j < V; j++) v[c][j] = m == 0 ? x[c][j] : v[c][j] + x[c][j];      // avg = p0, then avg += p_m
    }
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
      for (int j = 0; j < V; j++) {
        v[c][j] = v[c][j] / fm;                                                         // avg /= M: a true division
        bad |= !__builtin_isfinite(v[c][j]);                                            // a non-finite member or sum stays non-finite
      }

    if (seg) {
      uint32_t lab[V / 4];
#pragma unroll
      for (int w = 0; w < V / 4; w++) lab[w] = 0u;
#pragma unroll
      for (int j = 0; j < V; j++) {
        int l = 0;
        if constexpr (REGION) {
#pragma unroll
          for (int c = 0; c < C; c++) if (v[c][j] > 0.5f) l = (int)((order >> (8 * c)) & 0xffull);
        } else {
          float best = v[0][j];
#pragma unroll
          for (int c = 1; c < C; c++) if (v[c][j] > best) { best = v[c][j]; l = c; }
        }
        lab[j >> 2] |= (uint32_t)l << (8 * (j & 3));
      }
      if constexpr (VEC) {
        if constexpr (V == 4) *reinterpret_cast<uint32_t*>(seg + base) = lab[0];
        else *reinterpret_cast<uint2*>(seg + base) = make_uint2(lab[0], lab[1]);
      } else {
#pragma unroll
        for (int j = 0; j < V; j++) if (j < cnt) seg[base + j] = (uint8_t)(lab[j >> 2] >> (8 * (j & 3)));
      }
    }

    if (mean) {
#pragma unroll
      for (int c = 0; c < C; c++) {
        float* mp = mean + c * n + base;
        if constexpr (VEC) {
#pragma unroll
          for (int w = 0; w < V / 4; w++)
            *reinterpret_cast<float4*>(mp + 4 * w) = make_float4(v[c][4 * w], v[c][4 * w + 1], v[c][4 * w + 2], v[c][4 * w + 3]);
        } else {
#pragma unroll
          for (int j = 0; j < V; j++) if (j < cnt) mp[j] = v[c][j];
        }
      }
    }
  }
  if (bad) *flag = 1;
}

// The member pointers live in a device table, so the kernel itself decides between the two bodies: the same answer in every lane of the
// grid (a scalar branch).  out_vec: what the host knows -- seg and mean are aligned for the word stores.
template <typename T, int C, bool REGION>
__global__ __launch_bounds__(256) void ensemble_merge_kernel(const void* const* __restrict__ members, int M, long n, uint8_t* __restrict__ seg,
                                                             float* __restrict__ mean, int* __restrict__ flag, uint64_t order, bool out_vec) {
  constexpr int V = 16 / (int)sizeof(T);
  uintptr_t bits = 0;
  for (int m = 0; m < M; m++) bits |= reinterpret_cast<uintptr_t>(members[m]);
  if (out_vec && (bits & 15) == 0 && n % V == 0) merge_body<T, C, REGION, true>(members, M, n, seg, mean, flag, order);
  else merge_body<T, C, REGION, false>(members, M, n, seg, mean, flag, order);
}

int merge_grid(long items) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > 4096) g = 4096; return (int)g; }
bool aligned_to(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace

#define ENSEMBLE_C_SWITCH(C, CALL) \
  switch (C) { case 1: { CALL(1); break; } case 2: { CALL(2); break; } case 3: { CALL(3); break; } case 4: { CALL(4); break; } \
               case 5: { CALL(5); break; } case 6: { CALL(6); break; } case 7: { CALL(7); break; } case 8: { CALL(8); break; } \
               default: return DU_ERR_UNSUPPORTED; }

extern "C" int du_ensemble_merge(const void* const* members, int M, int elem_size, int K, int64_t n, int mode, int64_t region_order,
                                 uint8_t* seg, float* mean, int32_t* flag, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (M < 1 || M > MAXM || n < 0 || (elem_size != 4 && elem_size != 2)) return DU_ERR_UNSUPPORTED;
  if (mode != DU_EXPORT_SOFTMAX && mode != DU_EXPORT_REGIONS) return DU_ERR_BAD_ARG;
  // the label map of a softmax needs two classes; without a label map (seg == NULL: the mean alone) any 1..8 planes
  if (K < ((seg && mode == DU_EXPORT_SOFTMAX) ? 2 : 1) || K > MAXC) return DU_ERR_UNSUPPORTED;
  if (!members || !flag || (!seg && !mean)) return DU_ERR_BAD_ARG;
  if (n == 0) return DU_OK;
  const int V = 16 / elem_size;
  const bool out_vec = (!seg || aligned_to(seg, V)) && (!mean || aligned_to(mean, 16));
  const int grid = merge_grid((long)((n + V - 1) / V));
  const uint64_t order = (uint64_t)region_order;
  const bool region = mode == DU_EXPORT_REGIONS;
#define CALL(CC)                                                                                                                          \
  if (elem_size == 4) {                                                                                                                   \
    if (region) hipLaunchKernelGGL((ensemble_merge_kernel<float, CC, true>), dim3(grid), dim3(256), 0, st, members, M, (long)n, seg, mean, (int*)flag, order, out_vec); \
    else hipLaunchKernelGGL((ensemble_merge_kernel<float, CC, false>), dim3(grid), dim3(256), 0, st, members, M, (long)n, seg, mean, (int*)flag, order, out_vec); \
  } else {                                                                                                                                \
    if (region) hipLaunchKernelGGL((ensemble_merge_kernel<_Float16, CC, true>), dim3(grid), dim3(256), 0, st, members, M, (long)n, seg, mean, (int*)flag, order, out_vec); \
    else hipLaunchKernelGGL((ensemble_merge_kernel<_Float16, CC, false>), dim3(grid), dim3(256), 0, st, members, M, (long)n, seg, mean, (int*)flag, order, out_vec); \
  }
  ENSEMBLE_C_SWITCH(K, CALL)
#undef CALL
  return du_check_launch();
}
