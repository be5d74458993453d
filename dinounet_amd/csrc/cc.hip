// Connected components of one binary mask of a uint8 label map, and "keep only the largest" (remove_all_but_largest_component_from_segmentation,
// dinounet/postprocessing/remove_connected_components.py:22-34, which labels with full connectivity: 26 neighbours in 3-D).
//   mask(v) = label(v) < 64 and bit label(v) of mask_bits (the du_labels_to_regions convention)
//   id(component) = the smallest linear index (z H + y) W + x of its voxels: a function of the input alone, whatever the schedule
//   largest = the maximum voxel count, on a tie the smallest id (the first component in raster order)
// Union-find with the invariant parent[i] <= i, in separate launches on the caller's stream:
//   tile     one workgroup per 4 x 8 x 64 tile (z, y, x), one wave per row: the row's mask is one ballot, a voxel starts at the first voxel of
//            its row run (count leading zeros), rows are united through the 4 backward rows with integer atomics in LDS; writes
//            parent[v] = the global index of the tile-local root (-1 outside the mask) and size[v] = the tile-local voxel count at that
//            root, 0 elsewhere.  Tile raster order agrees with global order, so the local minimum is the global minimum of the tile component
//   merge    voxels on tile faces unite with those of their 13 forward neighbours that lie in another tile: returning atomicMin on the
//            larger root, retried from the value the atomic returns
//   flatten  ids[v] = root of v (reads parent only); every tile root that is not the global root adds its tile size to size[global root]:
//            one integer atomic per tile component, not per voxel
//   select   roots: key = size << 31 | (2^31 - 1 - id), one uint64 atomicMax and one count per workgroup; then stats
//   apply    out = (in the mask and ids != largest id) ? background_label : seg, 16 voxels per lane
// No kernel waits for another workgroup.  Every loop ends by itself: a find walks strictly decreasing parents, a union retry continues from
// a strictly smaller value.  Words another workgroup may write during a launch (parent in merge, size at global roots in flatten, the key
// and the count in select) are touched in that launch by atomics and agent-scope relaxed atomic loads only; everything read with plain
// loads was finished by an earlier launch.  Integer atomics only: bit-identical run to run.  No float, no scratch.
#include "common.h"

namespace {

constexpr int TX = 64, TY = 8, TZ = 4, ROWS = TY * TZ, TV = TX * ROWS;   // a tile: 2048 voxels, 32 rows of one wave each
constexpr int WS_HEAD = 4;                                             // int32 words in front of the arrays: key (uint64), count, spare
constexpr unsigned long long ID_MASK = 0x7FFFFFFFull;

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int agent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parents strictly decrease along the walk (L[i] <= i), so it ends at a root
__device__ __forceinline__ int lds_find(const int* L, int i) {
  int p = lds_load(L + i);
  while (p != i) { i = p; p = lds_load(L + i); }
  return i;
}
// every retry continues from `old` < a: ends.  A lost link a -> old is restored by uniting old with b.
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  a = lds_find(L, a); b = lds_find(L, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) break;
    a = old;
  }
}
__device__ __forceinline__ int global_find(const int* parent, int i) {
  int p = agent_load(parent + i);
  while (p != i) { i = p; p = agent_load(parent + i); }
  return i;
}
__device__ __forceinline__ void global_union(int* parent, int a, int b) {
  a = global_find(parent, a); b = global_find(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    a = old;
  }
}

struct Tiling {
  int ntx, nty;
  long ntiles;
};
__device__ __forceinline__ void tile_origin(const Tiling& tl, long t, int& x0, int& y0, int& z0) {
  const long ty = t / tl.ntx;
  x0 = (int)(t - ty * tl.ntx) * TX;
  const long tz = ty / tl.nty;
  y0 = (int)(ty - tz * tl.nty) * TY;
  z0 = (int)tz * TZ;
}

// the voxel of row `nb` (a ballot) that lane must unite with, given its own row ballot `own`: the voxel above it if set (its row
// neighbours are then in that voxel's run), else the diagonal ones.  A lane whose left neighbour is in its run and sits under the same
// run of `nb` leaves the union to that neighbour.
__device__ __forceinline__ void unite_rows(int* L, unsigned long long own, unsigned long long nb, int lane, int v, int nrow) {
  if (!((own >> lane) & 1ull) || nb == 0ull) return;
  const bool c = (nb >> lane) & 1ull, l = lane > 0 && ((nb >> (lane - 1)) & 1ull), r = lane < 63 && ((nb >> (lane + 1)) & 1ull);
  const bool left_own = lane > 0 && ((own >> (lane - 1)) & 1ull);
  if (c) {
    if (!(left_own && l)) lds_union(L, v, nrow * TX + lane);
  } else {
    if (l && !left_own) lds_union(L, v, nrow * TX + lane - 1);     // with left_own, the left neighbour has that voxel above it
    if (r) lds_union(L, v, nrow * TX + lane + 1);
  }
}

__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ seg, unsigned long long bits, int* __restrict__ parent,
                                                      int* __restrict__ size, int D, int H, int W, Tiling tl) {
  __shared__ int L[TV];
  __shared__ int cnt[TV];
  __shared__ unsigned long long rowbal[ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long t = blockIdx.x; t < tl.ntiles; t += gridDim.x) {
    int x0, y0, z0;
    tile_origin(tl, t, x0, y0, z0);
    const int x = x0 + lane;
#pragma unroll
    for (int k = 0; k < ROWS / 4; k++) {
      const int r = k * 4 + wave, y = y0 + (r & (TY - 1)), z = z0 + (r >> 3);
      bool m = false;
      if (z < D && y < H && x < W) {
        const unsigned l = seg[((long)z * H + y) * W + x];
        m = l < 64u && ((bits >> l) & 1ull);
      }
      const unsigned long long bal = __ballot(m);
      if (lane == 0) rowbal[r] = bal;
      const unsigned long long below = ~bal & ((1ull << lane) - 1ull);      // zeros left of this lane
      const int start = below ? 64 - __builtin_clzll(below) : 0;            // first voxel of this lane's run
      L[r * TX + lane] = m ? r * TX + start : -1;
      cnt[r * TX + lane] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROWS / 4; k++) {
      const int r = k * 4 + wave, ly = r & (TY - 1), lz = r >> 3, v = r * TX + lane;
      const unsigned long long own = rowbal[r];
      if (ly > 0) unite_rows(L, own, rowbal[r - 1], lane, v, r - 1);
      if (lz > 0) {
        unite_rows(L, own, rowbal[r - TY], lane, v, r - TY);
        if (ly > 0) unite_rows(L, own, rowbal[r - TY - 1], lane, v, r - TY - 1);
        if (ly < TY - 1) unite_rows(L, own, rowbal[r - TY + 1], lane, v, r - TY + 1);
      }
    }
    __syncthreads();
    int root[ROWS / 4];
#pragma unroll
    for (int k = 0; k < ROWS / 4; k++) {
      const int r = k * 4 + wave, v = r * TX + lane;
      const unsigned long long own = rowbal[r];
      root[k] = -1;
      if ((own >> lane) & 1ull) {
        root[k] = lds_find(L, v);
        if (lane == 0 || !((own >> (lane - 1)) & 1ull)) {                   // the first voxel of a run adds the run
          const unsigned long long rest = ~(own >> lane);
          atomicAdd(cnt + root[k], rest ? __builtin_ctzll(rest) : 64);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ROWS / 4; k++) {
      const int r = k * 4 + wave, y = y0 + (r & (TY - 1)), z = z0 + (r >> 3), v = r * TX + lane;
      if (z < D && y < H && x < W) {
        const long g = ((long)z * H + y) * W + x;
        const int rt = root[k];
        int pg = -1;
        if (rt >= 0) pg = (int)(((long)(z0 + (rt >> 9)) * H + y0 + ((rt >> 6) & (TY - 1))) * W + x0 + (rt & (TX - 1)));
        parent[g] = pg;
        size[g] = rt == v ? cnt[v] : 0;
      }
    }
    __syncthreads();
  }
}

// forward neighbours of the voxel (x, y, z) in row (y + dy, z + dz); only those in another tile are united here
__device__ __forceinline__ void merge_row(int* parent, int g, int x, int y, int z, int dy, int dz, int H, int W, int D) {
  const int ny = y + dy, nz = z + dz;
  if (ny < 0 || ny >= H || nz >= D) return;
  const bool row_other = (ny >> 3) != (y >> 3) || (nz >> 2) != (z >> 2);
  const int lx = x & (TX - 1);
  if (!row_other && lx != 0 && lx != TX - 1) return;
  const int ng = (int)(((long)nz * H + ny) * W + x);
  if (agent_load(parent + ng) >= 0) {            // the voxel straight across: its row neighbours are in its run
    if (row_other) global_union(parent, g, ng);
    return;
  }
  if (x > 0 && (row_other || lx == 0) && agent_load(parent + ng - 1) >= 0) global_union(parent, g, ng - 1);
  if (x < W - 1 && (row_other || lx == TX - 1) && agent_load(parent + ng + 1) >= 0) global_union(parent, g, ng + 1);
}

__global__ __launch_bounds__(256) void cc_merge_kernel(int* __restrict__ parent, int D, int H, int W, Tiling tl) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long t = blockIdx.x; t < tl.ntiles; t += gridDim.x) {
    int x0, y0, z0;
    tile_origin(tl, t, x0, y0, z0);
    const int x = x0 + lane;
    if (x >= W) continue;
    for (int r = wave; r < ROWS; r += 4) {
      const int ly = r & (TY - 1), lz = r >> 3, y = y0 + ly, z = z0 + lz;
      if (y >= H || z >= D) continue;
      if (lane != 0 && lane != TX - 1 && ly != 0 && ly != TY - 1 && lz != TZ - 1) continue;   // no forward neighbour in another tile
      const int g = (int)(((long)z * H + y) * W + x);
      if (agent_load(parent + g) < 0) continue;
      if (lane == TX - 1 && x < W - 1 && agent_load(parent + g + 1) >= 0) global_union(parent, g, g + 1);
      merge_row(parent, g, x, y, z, 1, 0, H, W, D);
      merge_row(parent, g, x, y, z, -1, 1, H, W, D);
      merge_row(parent, g, x, y, z, 0, 1, H, W, D);
      merge_row(parent, g, x, y, z, 1, 1, H, W, D);
    }
  }
}

// parent is final here (plain loads).  size[i] of a voxel that is not a global root is written by nobody in this launch.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ size, int* __restrict__ ids, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    int r = parent[i];
    if (r >= 0) {
      int q = parent[r];
      while (q != r) { r = q; q = parent[r]; }
      if (r != (int)i) {
        const int s = size[i];
        if (s > 0) atomicAdd(size + r, s);
      }
    }
    ids[i] = r;
  }
}

__global__ __launch_bounds__(256) void cc_select_kernel(const int* __restrict__ ids, const int* __restrict__ size, unsigned long long* key,
                                                        int* count, long n) {
  unsigned long long best = 0ull;
  int roots = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    if (ids[i] == (int)i) {
      const unsigned long long k = ((unsigned long long)size[i] << 31) | (ID_MASK - (unsigned long long)i);
      best = k > best ? k : best;
      roots++;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = __shfl_xor(best, o, 64);
    best = ob > best ? ob : best;
    roots += __shfl_xor(roots, o, 64);
  }
  __shared__ unsigned long long sb[4];
  __shared__ int sr[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sb[wave] = best; sr[wave] = roots; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { best = sb[w] > best ? sb[w] : best; roots += sr[w]; }
    if (roots > 0) { atomicMax(key, best); atomicAdd(count, roots); }
  }
}

// stats = {n_components, largest size, largest id or -1}
__global__ void cc_stats_kernel(const unsigned long long* __restrict__ key, const int* __restrict__ count, int64_t* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const unsigned long long k = *key;
    stats[0] = *count;
    stats[1] = (int64_t)(k >> 31);
    stats[2] = k ? (int64_t)(ID_MASK - (k & ID_MASK)) : -1;
  }
}

__global__ __launch_bounds__(256) void cc_apply_kernel(const uint8_t* __restrict__ seg, const int* __restrict__ ids,
                                                       const unsigned long long* __restrict__ key, uint8_t* __restrict__ out,
                                                       unsigned long long bits, int background, long n, bool vec) {
  const unsigned long long k = *key;
  const int best = k ? (int)(ID_MASK - (k & ID_MASK)) : -1;
  const long items = (n + 15) >> 4;
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
    const long base = it << 4;
    const int m = (int)(n - base < 16 ? n - base : 16);
    if (vec && m == 16) {
      const uint4 a = *reinterpret_cast<const uint4*>(seg + base);
      uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int4 id = *reinterpret_cast<const int4*>(ids + base + 4 * q);
        const int idv[4] = {id.x, id.y, id.z, id.w};
        uint32_t o = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint32_t l = (w[q] >> (8 * j)) & 255u;
          const bool drop = l < 64u && ((bits >> l) & 1ull) && idv[j] != best;
          o |= (drop ? (uint32_t)background : l) << (8 * j);
        }
        w[q] = o;
      }
      *reinterpret_cast<uint4*>(out + base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int j = 0; j < m; j++) {
        const uint32_t l = seg[base + j];
        const bool drop = l < 64u && ((bits >> l) & 1ull) && ids[base + j] != best;
        out[base + j] = (uint8_t)(drop ? (uint32_t)background : l);
      }
    }
  }
}

struct CcWs {
  unsigned long long* key;
  int* count;
  int *parent, *size, *ids;
  int64_t elems;
};
// 4 head words, then parent | size (| ids) of n rounded up to 4 voxels each: every array starts 16-byte aligned
CcWs carve(int32_t* ws, int64_t n, int keep) {
  const int64_t nn = (n + 3) & ~(int64_t)3;
  CcWs s;
  s.key = (unsigned long long*)ws;
  s.count = ws + 2;
  s.parent = ws + WS_HEAD;
  s.size = ws + WS_HEAD + nn;
  s.ids = keep ? ws + WS_HEAD + 2 * nn : nullptr;
  s.elems = WS_HEAD + (keep ? 3 : 2) * nn;
  return s;
}
int grid_for(long items, long cap) { long g = (items + 255) / 256; if (g < 1) g = 1; if (g > cap) g = cap; return (int)g; }

// 0, or the error of the shape
int shape_error(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return DU_ERR_BAD_ARG;
  const int64_t lim = (int64_t)1 << 31, dh = (int64_t)D * H;
  if (dh >= lim || dh * W >= lim) return DU_ERR_UNSUPPORTED;
  return DU_OK;
}

// tile, merge, flatten, select, stats.  ids: where the flattened labels go
int label_launches(const uint8_t* seg, uint64_t bits, int* ids, int64_t* stats, const CcWs& s, int D, int H, int W, hipStream_t st) {
  const long n = (long)D * H * W;
  Tiling tl;
  tl.ntx = (W + TX - 1) / TX; tl.nty = (H + TY - 1) / TY;
  tl.ntiles = (long)tl.ntx * tl.nty * ((D + TZ - 1) / TZ);
  const int tgrid = (int)(tl.ntiles < 262144 ? tl.ntiles : 262144);
  if (hipMemsetAsync(s.key, 0, WS_HEAD * sizeof(int32_t), st) != hipSuccess) return DU_ERR_LAUNCH;
  hipLaunchKernelGGL(cc_tile_kernel, dim3(tgrid), dim3(256), 0, st, seg, (unsigned long long)bits, s.parent, s.size, D, H, W, tl);
  hipLaunchKernelGGL(cc_merge_kernel, dim3(tgrid), dim3(256), 0, st, s.parent, D, H, W, tl);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for(n, 65536)), dim3(256), 0, st, (const int*)s.parent, s.size, ids, n);
  hipLaunchKernelGGL(cc_select_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, st, (const int*)ids, (const int*)s.size, s.key, s.count, n);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)s.key, (const int*)s.count, stats);
  return DU_OK;
}

}  // namespace

extern "C" int64_t du_cc_ws_elems(int D, int H, int W, int keep) {
  if (shape_error(D, H, W) != DU_OK) return 0;
  return carve(nullptr, (int64_t)D * H * W, keep).elems;
}

extern "C" int du_cc_label(const uint8_t* seg, int64_t mask_bits, int32_t* ids, int64_t* stats, int D, int H, int W, int32_t* ws,
                           int64_t ws_elems, void* stream) {
  if (!seg || !ids || !stats || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)ids & 3)) return DU_ERR_BAD_ARG;
  const int e = shape_error(D, H, W);
  if (e != DU_OK) return e;
  const CcWs s = carve(ws, (int64_t)D * H * W, 0);
  if (ws_elems < s.elems) return DU_ERR_BAD_ARG;
  const int rc = label_launches(seg, (uint64_t)mask_bits, ids, stats, s, D, H, W, (hipStream_t)stream);
  return rc != DU_OK ? rc : du_check_launch();
}

extern "C" int du_cc_keep_largest(const uint8_t* seg, int64_t mask_bits, int background_label, uint8_t* out, int64_t* stats, int D, int H,
                                  int W, int32_t* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!seg || !out || !stats || !ws || ((uintptr_t)ws & 15) || out == seg || background_label < 0 || background_label > 255) return DU_ERR_BAD_ARG;
  const int e = shape_error(D, H, W);
  if (e != DU_OK) return e;
  const int64_t n = (int64_t)D * H * W;
  if (out < seg + n && seg < out + n) return DU_ERR_BAD_ARG;               // out must not overlap seg
  const CcWs s = carve(ws, n, 1);
  if (ws_elems < s.elems) return DU_ERR_BAD_ARG;
  const int rc = label_launches(seg, (uint64_t)mask_bits, s.ids, stats, s, D, H, W, st);
  if (rc != DU_OK) return rc;
  const bool vec = (((uintptr_t)seg | (uintptr_t)out) & 15) == 0;
  hipLaunchKernelGGL(cc_apply_kernel, dim3(grid_for((n + 15) / 16, 8192)), dim3(256), 0, st, seg, (const int*)s.ids,
                     (const unsigned long long*)s.key, out, (unsigned long long)(uint64_t)mask_bits, background_label, (long)n, vec);
  return du_check_launch();
}
