// Surface metrics of the per-case table (HD95 / ASD of compute_metrics, dinounet/evaluation/evaluate_predictions.py:97-149, 212-226, which
// calls medpy.metric.hd95 / asd): the border voxels of every label or region of two uint8 label maps, and the exact Euclidean distance
// transform of the complement of each border set, sampled at the other map's border voxels.
//   border(m) = m ^ binary_erosion(m, 6-neighbourhood, border_value = 0): a mask voxel with a face neighbour outside the mask or the volume
//   dt(q)     = min over border voxels p of (dz sz)^2 + (dy sy)^2 + (dx sx)^2, the three squares added in that order, fp64, never rooted here
// One field (side x region) at a time, three passes over the volume:
//   x  every voxel gets |dx| to the nearest border voxel of its row (uint16, NONE16 = none in this row): ballots + count-leading-zeros
//   y  lower envelope (Felzenszwalb & Huttenlocher) of the parabolas (dx sx)^2 + ((y - y') sy)^2 down every column; writes the WINNER's integer
//      offsets |dy| | |dx| packed in 32 bits (NONE32 = no border voxel in this slice), not a distance
//   z  the same down z over (dy sy)^2 + (dx sx)^2; the winner's three integer offsets give the value, evaluated directly.  The value goes to
//      the dense field (FIELD) or, where the other map's border bit is set, to a compacted segment (GATHER) with sqrt summed per block
// A lane owns a column: consecutive lanes are consecutive x, so every global access of the y and z passes is a row segment.  The envelope is
// a stack of 4-byte entries (index | offsets) in LDS; intersections are recomputed from two entries where needed and never stored.
// A candidate without a border voxel is never pushed: no infinity enters an intersection, an empty stack is +inf for the whole column.
// No float atomics: the compacted slot comes from an integer counter (order inside a segment is free), the ASD sum from per-block
// partials added in a fixed order by a second kernel.
#include "common.h"

#pragma clang fp contract(off)   // the three squares are rounded one by one and added in the stated order: no fused multiply-add

namespace {

constexpr int MAXR = 8;
constexpr int MAX_EXTENT = 1024;          // offsets and indices are 10-bit fields of a stack entry
constexpr uint32_t NONE16 = 0xFFFFu, NONE32 = 0xFFFFFFFFu;
constexpr int SCAN_LDS_BYTES = 65536;     // the stacks of one workgroup: columns * n * 4 bytes
constexpr int BATCH = 8;                  // rows loaded ahead of the serial scan

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int R>
__device__ __forceinline__ uint32_t membership(const uint64_t (&tb)[R], uint32_t l) {
  uint32_t m = 0;
  const uint32_t s = l & 63u;
#pragma unroll
  for (int r = 0; r < R; r++) m |= (uint32_t)((tb[r] >> s) & 1ull) << r;
  return l < 64u ? m : 0u;
}

// Border bits and counts.  bits[i]: bit r = voxel i is a border voxel of region r of pred, bit 8 + r = of ref.  cpart: one row of 4R int32
// per block = mask voxels pred | mask voxels ref | border voxels pred | border voxels ref.
template <int R>
__global__ __launch_bounds__(256) void surface_border_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ ref,
                                                             const int64_t* __restrict__ masks, uint16_t* __restrict__ bits,
                                                             int* __restrict__ cpart, int D, int H, int W) {
  constexpr int NC = 4 * R;
  uint64_t tb[R];
#pragma unroll
  for (int r = 0; r < R; r++) tb[r] = (uint64_t)masks[r];
  int cnt[NC];
#pragma unroll
  for (int i = 0; i < NC; i++) cnt[i] = 0;
  const long HW = (long)H * W, n = (long)D * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / W;
    const int x = (int)(i - row * W);
    const int z = (int)(row / H), y = (int)(row - (long)z * H);
    const uint32_t pc = membership<R>(tb, pred[i]), rc = membership<R>(tb, ref[i]);
    uint32_t pn = 0, rn = 0;                      // regions whose six neighbours are all inside the mask and the volume
    if ((pc | rc) != 0u && x > 0 && x < W - 1 && y > 0 && y < H - 1 && z > 0 && z < D - 1) {
      pn = pc; rn = rc;
      pn &= membership<R>(tb, pred[i - 1]);  rn &= membership<R>(tb, ref[i - 1]);
      pn &= membership<R>(tb, pred[i + 1]);  rn &= membership<R>(tb, ref[i + 1]);
      pn &= membership<R>(tb, pred[i - W]);  rn &= membership<R>(tb, ref[i - W]);
      pn &= membership<R>(tb, pred[i + W]);  rn &= membership<R>(tb, ref[i + W]);
      pn &= membership<R>(tb, pred[i - HW]); rn &= membership<R>(tb, ref[i - HW]);
      pn &= membership<R>(tb, pred[i + HW]); rn &= membership<R>(tb, ref[i + HW]);
    }
    const uint32_t pb = pc & ~pn, rb = rc & ~rn;
    bits[i] = (uint16_t)(pb | (rb << 8));
#pragma unroll
    for (int r = 0; r < R; r++) {
      cnt[r] += (int)((pc >> r) & 1u);
      cnt[R + r] += (int)((rc >> r) & 1u);
      cnt[2 * R + r] += (int)((pb >> r) & 1u);
      cnt[3 * R + r] += (int)((rb >> r) & 1u);
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

// ONE block adds the rows of the block partials in int64, fixed order: counts (4, R)
__global__ __launch_bounds__(256) void surface_counts_sum_kernel(const int* __restrict__ cpart, int64_t* __restrict__ counts, int blocks, int NC) {
  __shared__ long long red[4 * MAXR][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < NC; i++) {
    long long a = 0;
    for (int b = threadIdx.x; b < blocks; b += 256) a += (long long)cpart[(long)b * NC + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) red[i][wave] = a;
  }
  __syncthreads();
  if (threadIdx.x < NC) counts[threadIdx.x] = (int64_t)((red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]));
}

// x pass: one wave per row.  The row's border bits of field `bit` become one 64-bit ballot per 64 columns, ballot c kept by lane c; the
// nearest set bit at or left of a column is in its own ballot (count leading zeros) or is the last set bit of the chunks before, the
// nearest at or right likewise.  Every loop has the same trip count in all lanes: the shuffles read active lanes only.
__global__ __launch_bounds__(256) void surface_xpass_kernel(const uint16_t* __restrict__ bits, uint16_t* __restrict__ gx, long rows, int W, int bit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = (W + 63) >> 6;
  constexpr int FAR = 1 << 20;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    const uint16_t* b = bits + row * W;
    unsigned long long mine = 0ull;
    for (int c = 0; c < nch; c++) {
      const int x = c * 64 + lane;
      const bool s = x < W && ((b[x] >> bit) & 1);
      const unsigned long long bal = __ballot(s);
      if (lane == c) mine = bal;
    }
    int nxt = -1, run = -1;                       // lane c: first set column in the chunks after c
    for (int c = nch - 1; c >= 0; c--) {
      const unsigned long long w = __shfl(mine, c, 64);
      if (lane == c) nxt = run;
      if (w) run = c * 64 + __builtin_ctzll(w);
    }
    int last = -1;                                // last set column in the chunks before c
    for (int c = 0; c < nch; c++) {
      const unsigned long long w = __shfl(mine, c, 64);
      const int np = __shfl(nxt, c, 64);
      const int x = c * 64 + lane;
      const unsigned long long ml = w & (~0ull >> (63 - lane)), mr = w & (~0ull << lane);
      const int dl = ml ? lane - (63 - __builtin_clzll(ml)) : (last >= 0 ? x - last : FAR);
      const int dr = mr ? __builtin_ctzll(mr) - lane : (np >= 0 ? np - x : FAR);
      const int d = dl < dr ? dl : dr;
      if (x < W) gx[row * W + x] = d >= FAR ? (uint16_t)NONE16 : (uint16_t)d;
      if (w) last = c * 64 + 63 - __builtin_clzll(w);
    }
  }
}

// ---- the lower-envelope scan of the y and z passes.  A stack entry is index << 20 | a << 10 | b: y pass a = 0, b = |dx|; z pass a = |dy|,
// b = |dx|.  cost of entry e at position q = base(e) + ((q - index) w)^2.
template <bool ZP>
__host__ __device__ __forceinline__ double base_cost(uint32_t e, double sy, double sx) {
  const double dx = (double)(e & 1023u) * sx;
  if constexpr (ZP) {
    const double dy = (double)((e >> 10) & 1023u) * sy;
    return dy * dy + dx * dx;
  } else {
    return dx * dx;
  }
}

// where the parabolas of candidates i < j (base costs fi, fj, both finite) meet: left of it i is lower, right of it j
__host__ __device__ __forceinline__ double meet(int i, double fi, int j, double fj, double w2) {
  return ((fj - fi) / (w2 * (double)(j - i)) + (double)(i + j)) * 0.5;
}

// Build the envelope of one column.  load(q) returns the raw element of position q (NONE = no candidate).  st: this lane's stack, entry k at
// st[k * C].  Returns the number of entries.  The top's index, base cost and the start of its interval stay in registers.
template <bool ZP, typename Load>
__host__ __device__ __forceinline__ int envelope_build(uint32_t* st, int C, int n, double sy, double sx, double w2, bool active, Load load) {
  int k = 0, ti = 0;
  double tf = 0.0, tz = 0.0;
  const double NEG = -__builtin_inf();
  for (int q0 = 0; q0 < n; q0 += BATCH) {
    uint32_t raw[BATCH];
#pragma unroll
    for (int j = 0; j < BATCH; j++) raw[j] = (active && q0 + j < n) ? load(q0 + j) : NONE32;
#pragma unroll
    for (int j = 0; j < BATCH; j++) {
      if (raw[j] != NONE32) {
        const int q = q0 + j;
        const uint32_t e = ((uint32_t)q << 20) | raw[j];
        const double f = base_cost<ZP>(e, sy, sx);
        double s = NEG;
        if (k > 0) {
          s = meet(ti, tf, q, f, w2);
          while (s <= tz) {                        // the top is nowhere lowest: drop it.  tz = -inf for the last entry, s is finite
            k--;
            const uint32_t te = st[(k - 1) * C];
            ti = (int)(te >> 20); tf = base_cost<ZP>(te, sy, sx);
            if (k >= 2) { const uint32_t pe = st[(k - 2) * C]; tz = meet((int)(pe >> 20), base_cost<ZP>(pe, sy, sx), ti, tf, w2); }
            else tz = NEG;
            s = meet(ti, tf, q, f, w2);
          }
        }
        st[k * C] = e;
        k++; ti = q; tf = f; tz = s;
      }
    }
  }
  return k;
}

// Walk the envelope: calls emit(q, e) with the entry that is lowest at q, for q = 0 .. n - 1 (k > 0)
struct EnvelopeWalk {
  uint32_t cur, nxt;
  double zn;
  int c;
};
template <bool ZP>
__host__ __device__ __forceinline__ void walk_start(EnvelopeWalk& wk, const uint32_t* st, int C, int k, double sy, double sx, double w2) {
  wk.c = 0; wk.cur = st[0]; wk.nxt = 0; wk.zn = __builtin_inf();
  if (k > 1) {
    wk.nxt = st[C];
    wk.zn = meet((int)(wk.cur >> 20), base_cost<ZP>(wk.cur, sy, sx), (int)(wk.nxt >> 20), base_cost<ZP>(wk.nxt, sy, sx), w2);
  }
}
template <bool ZP>
__host__ __device__ __forceinline__ void walk_to(EnvelopeWalk& wk, const uint32_t* st, int C, int k, int q, double sy, double sx, double w2) {
  while (wk.zn < (double)q) {
    wk.c++; wk.cur = wk.nxt; wk.zn = __builtin_inf();
    if (wk.c + 1 < k) {
      wk.nxt = st[(wk.c + 1) * C];
      wk.zn = meet((int)(wk.cur >> 20), base_cost<ZP>(wk.cur, sy, sx), (int)(wk.nxt >> 20), base_cost<ZP>(wk.nxt, sy, sx), w2);
    }
  }
}

// y pass.  One 64-lane workgroup: slice blockIdx.y, columns blockIdx.x * C .. + C - 1 (lanes >= C idle); rows 0 .. H - 1 down the column.
__global__ __launch_bounds__(64) void surface_ypass_kernel(const uint16_t* __restrict__ gx, uint32_t* __restrict__ gyx, int H, int W, int C,
                                                           double sy, double sx) {
  extern __shared__ uint32_t lds_stack[];
  const int lane = threadIdx.x;
  const int x = blockIdx.x * C + lane;
  const bool active = lane < C && x < W;
  if (!active) return;                              // no barrier below: a lane's stack is its own
  uint32_t* st = lds_stack + lane;
  const long base = (long)blockIdx.y * H * W + x;
  const double w2 = sy * sy;
  const int k = envelope_build<false>(st, C, H, sy, sx, w2, active, [&](int q) -> uint32_t {
    const uint32_t v = gx[base + (long)q * W];
    return v == NONE16 ? NONE32 : v;
  });
  if (k == 0) {
    for (int q = 0; q < H; q++) gyx[base + (long)q * W] = NONE32;
    return;
  }
  EnvelopeWalk wk;
  walk_start<false>(wk, st, C, k, sy, sx, w2);
  for (int q = 0; q < H; q++) {
    walk_to<false>(wk, st, C, k, q, sy, sx, w2);
    const int i = (int)(wk.cur >> 20);
    const uint32_t dy = (uint32_t)(q > i ? q - i : i - q);
    gyx[base + (long)q * W] = (dy << 10) | (wk.cur & 1023u);
  }
}

// z pass.  Workgroup: row blockIdx.y of every slice, columns blockIdx.x * C ..; positions 0 .. D - 1 down z.
// GATHER = false: field[voxel] = the squared distance (+inf without any border voxel).
// GATHER = true: where bits has `other_bit`, the value is appended to seg[0 .. seg_len) (slot from the integer counter `cursor`); with
// part != null the lane adds sqrt(value) over its column in z order, the wave adds its lanes in a fixed tree, part[block] = that sum.
template <bool GATHER>
__global__ __launch_bounds__(64) void surface_zpass_kernel(const uint32_t* __restrict__ gyx, const uint16_t* __restrict__ bits,
                                                           double* __restrict__ field, double* __restrict__ seg, long seg_len,
                                                           int* __restrict__ cursor, double* __restrict__ part, int other_bit, int D, int H,
                                                           int W, int C, double sz, double sy, double sx) {
  extern __shared__ uint32_t lds_stack[];
  const int lane = threadIdx.x;
  const int x = blockIdx.x * C + lane;
  const bool active = lane < C && x < W;
  const long HW = (long)H * W;
  const long base = (long)blockIdx.y * W + (active ? x : 0);
  const double w2 = sz * sz;
  double sum = 0.0;
  if (active) {
    uint32_t* st = lds_stack + lane;
    const int k = envelope_build<true>(st, C, D, sy, sx, w2, active, [&](int q) -> uint32_t { return gyx[base + (long)q * HW]; });
    EnvelopeWalk wk;
    if (k > 0) walk_start<true>(wk, st, C, k, sy, sx, w2);
    for (int q0 = 0; q0 < D; q0 += BATCH) {
      bool hit[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; j++) hit[j] = GATHER && q0 + j < D && ((bits[base + (long)(q0 + j) * HW] >> other_bit) & 1);
#pragma unroll
      for (int j = 0; j < BATCH; j++) {
        const int q = q0 + j;
        if (q < D && (!GATHER || hit[j])) {
          double v = __builtin_inf();
          if (k > 0) {
            walk_to<true>(wk, st, C, k, q, sy, sx, w2);
            const uint32_t e = wk.cur;
            const int i = (int)(e >> 20);
            const double dz = (double)(q > i ? q - i : i - q) * sz, dy = (double)((e >> 10) & 1023u) * sy, dx = (double)(e & 1023u) * sx;
            v = (dz * dz + dy * dy) + dx * dx;
          }
          if constexpr (GATHER) {
            const int slot = atomicAdd(cursor, 1);
            if ((long)slot < seg_len) seg[slot] = v;
            sum += sqrt(v);
          } else {
            field[base + (long)q * HW] = v;
          }
        }
      }
    }
  }
  if constexpr (GATHER) {
    if (part) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
      if (lane == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = sum;
    }
  }
}

// ONE block adds the per-block sqrt sums in a fixed order
__global__ __launch_bounds__(256) void surface_sqrt_sum_kernel(const double* __restrict__ part, double* __restrict__ out, int blocks) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += part[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

int border_grid(int64_t n) { long g = ((long)n + 255) / 256; if (g < 1) g = 1; if (g > 2048) g = 2048; return (int)g; }
// columns per workgroup of a scan over n positions: the largest power of two <= 64 whose stacks fit SCAN_LDS_BYTES
int scan_columns(int n) { int c = 64; while (c > 1 && (long)c * n * 4 > SCAN_LDS_BYTES) c >>= 1; return c; }
bool extents_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT; }
bool spacing_ok(double s) { return s > 0.0 && s < 1e100; }

struct SurfaceWs {
  uint16_t* gx;      // (D, H, W) uint16
  uint32_t* gyx;     // (D, H, W) uint32
  double* part;      // z-pass blocks
  int* cursor;       // 2 * MAXR
  int zblocks;
  int64_t elems;     // 8-byte elements
};
SurfaceWs carve(void* ws, int D, int H, int W) {
  const int64_t n = (int64_t)D * H * W;
  const int Cz = scan_columns(D);
  SurfaceWs s;
  s.zblocks = H * ((W + Cz - 1) / Cz);
  const int64_t e_gx = (n + 3) / 4, e_gyx = (n + 1) / 2, e_part = s.zblocks, e_cur = MAXR;
  char* p = (char*)ws;
  s.gx = (uint16_t*)p;
  s.gyx = (uint32_t*)(p + 8 * e_gx);
  s.part = (double*)(p + 8 * (e_gx + e_gyx));
  s.cursor = (int*)(p + 8 * (e_gx + e_gyx + e_part));
  s.elems = e_gx + e_gyx + e_part + e_cur;
  return s;
}

// x and y passes of the field `bit` of `bits` into the workspace
void launch_xy(const uint16_t* bits, const SurfaceWs& s, int D, int H, int W, int bit, double sy, double sx, hipStream_t st) {
  const long rows = (long)D * H;
  long gxb = (rows + 3) / 4; if (gxb > 4096) gxb = 4096;
  hipLaunchKernelGGL(surface_xpass_kernel, dim3((int)gxb), dim3(256), 0, st, bits, s.gx, rows, W, bit);
  const int Cy = scan_columns(H);
  hipLaunchKernelGGL(surface_ypass_kernel, dim3((W + Cy - 1) / Cy, D), dim3(64), (size_t)Cy * H * 4, st, (const uint16_t*)s.gx, s.gyx, H, W, Cy, sy, sx);
}

}  // namespace

#define SURFACE_R_SWITCH(R, CALL) \
  switch (R) { case 1: { CALL(1); break; } case 2: { CALL(2); break; } case 3: { CALL(3); break; } case 4: { CALL(4); break; } \
               case 5: { CALL(5); break; } case 6: { CALL(6); break; } case 7: { CALL(7); break; } case 8: { CALL(8); break; } \
               default: return DU_ERR_UNSUPPORTED; }

extern "C" int64_t du_surface_border_ws_elems(int64_t n, int R) {
  if (n <= 0 || R < 1 || R > MAXR) return 0;
  return (int64_t)border_grid(n) * 4 * R;
}

extern "C" int du_surface_border(const uint8_t* pred, const uint8_t* ref, const int64_t* masks, uint16_t* bits, int64_t* counts, int D, int H,
                                 int W, int R, int32_t* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!pred || !ref || !masks || !bits || !counts || !ws) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR || !extents_ok(D, H, W)) return DU_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)D * H * W;
  const int grid = border_grid(n);
  if (ws_elems < (int64_t)grid * 4 * R) return DU_ERR_BAD_ARG;
#define CALL(RR) hipLaunchKernelGGL(surface_border_kernel<RR>, dim3(grid), dim3(256), 0, st, pred, ref, masks, bits, (int*)ws, D, H, W)
  SURFACE_R_SWITCH(R, CALL)
#undef CALL
  hipLaunchKernelGGL(surface_counts_sum_kernel, dim3(1), dim3(256), 0, st, (const int*)ws, counts, grid, 4 * R);
  return du_check_launch();
}

extern "C" int64_t du_surface_ws_elems(int D, int H, int W) {
  if (!extents_ok(D, H, W)) return 0;
  return carve(nullptr, D, H, W).elems;
}

extern "C" int du_surface_field(const uint16_t* bits, double* field, int D, int H, int W, int bit, double sz, double sy, double sx, void* ws,
                                int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!bits || !field || !ws || bit < 0 || bit > 15 || ((uintptr_t)ws & 7)) return DU_ERR_BAD_ARG;
  if (!extents_ok(D, H, W)) return DU_ERR_UNSUPPORTED;
  if (!spacing_ok(sz) || !spacing_ok(sy) || !spacing_ok(sx)) return DU_ERR_BAD_ARG;
  const SurfaceWs s = carve(ws, D, H, W);
  if (ws_elems < s.elems) return DU_ERR_BAD_ARG;
  launch_xy(bits, s, D, H, W, bit, sy, sx, st);
  const int Cz = scan_columns(D);
  hipLaunchKernelGGL(surface_zpass_kernel<false>, dim3((W + Cz - 1) / Cz, H), dim3(64), (size_t)Cz * D * 4, st, (const uint32_t*)s.gyx, bits, field,
                     (double*)nullptr, 0L, (int*)nullptr, (double*)nullptr, 0, D, H, W, Cz, sz, sy, sx);
  return du_check_launch();
}

extern "C" int du_surface_gather(const uint16_t* bits, int D, int H, int W, int R, int active, double sz, double sy, double sx,
                                 const int64_t* seg_off_host, double* dist_sq, double* sqrt_sums, void* ws, int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!bits || !seg_off_host || !dist_sq || !sqrt_sums || !ws || ((uintptr_t)ws & 7)) return DU_ERR_BAD_ARG;
  if (R < 1 || R > MAXR || !extents_ok(D, H, W)) return DU_ERR_UNSUPPORTED;
  if (!spacing_ok(sz) || !spacing_ok(sy) || !spacing_ok(sx)) return DU_ERR_BAD_ARG;
  for (int i = 0; i < 2 * R; i++) if (seg_off_host[i] < 0 || seg_off_host[i + 1] < seg_off_host[i]) return DU_ERR_BAD_ARG;
  const SurfaceWs s = carve(ws, D, H, W);
  if (ws_elems < s.elems) return DU_ERR_BAD_ARG;
  if (hipMemsetAsync(s.cursor, 0, 2 * MAXR * sizeof(int), st) != hipSuccess) return DU_ERR_LAUNCH;
  const int Cz = scan_columns(D);
  for (int r = 0; r < R; r++) {
    if (!((active >> r) & 1)) continue;
    for (int dir = 0; dir < 2; dir++) {
      // dir 0: the ref field sampled at the pred border (d_pr, with the sqrt sum); dir 1: the pred field at the ref border (d_rp)
      const int field_bit = dir == 0 ? 8 + r : r, other_bit = dir == 0 ? r : 8 + r;
      const int64_t off = seg_off_host[2 * r + dir], len = seg_off_host[2 * r + dir + 1] - off;
      launch_xy(bits, s, D, H, W, field_bit, sy, sx, st);
      hipLaunchKernelGGL(surface_zpass_kernel<true>, dim3((W + Cz - 1) / Cz, H), dim3(64), (size_t)Cz * D * 4, st, (const uint32_t*)s.gyx, bits,
                         (double*)nullptr, dist_sq + off, (long)len, s.cursor + 2 * r + dir, dir == 0 ? s.part : (double*)nullptr, other_bit, D,
                         H, W, Cz, sz, sy, sx);
      if (dir == 0) hipLaunchKernelGGL(surface_sqrt_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)s.part, sqrt_sums + r, s.zblocks);
    }
  }
  return du_check_launch();
}
