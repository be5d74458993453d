// Band-tiled depthwise 3x3 (stride 1, pad 1) for bf16 channel-last tensors on gfx950: forward, data gradient (with the activation's
// derivative applied on load) and weight / bias gradient.  Serves ConvFFN's DWConv + GELU over the token pyramid (dinov3_adapter.py:87-109)
// and DepthwiseSeparableConv.depthwise (dinounet_training.py:235); every call du_dwconv_plan (below; dwconv_plan.h) does not give to them stays on elementwise.hip.
//
// Decomposition.  The row kernels of elementwise.hip give a workgroup 32 consecutive pixels of ONE row: rows y - 1 and y + 1 belong to
// workgroups the dispatcher deals to other XCDs, so every input row is fetched by three L2s and a thread issues 18 loads per 4 outputs.
// Here a thread owns XT = 2 adjacent columns of one 8-channel vector and walks down a band of R rows with a three-row window of packed
// inputs in registers: each input row is loaded once per band (the two halo rows of a band are the only re-reads, (R + 2) / R), and the
// row below is requested before the current one is consumed.  A work item = (image, band, column group), column groups fastest; a
// workgroup = 32 consecutive items x a slab of 64 channels (8 vectors: one 128-byte line per pixel).  Workgroup indices are ordered
// level -> slab -> item block and mapped through xcd_linear_index(), so the bands of one (image, grid, slab) are neighbours on one XCD
// and a halo row is found in the L2 that fetched it.  Placement affects speed only: every output element is written by exactly one thread
// and every sum inside a thread has a fixed order.
//
// Results.  y, z and dx have the bits of dwconv_row4_kernel / dwconv_kernel: accumulator = bias, then the taps row-major, one fp32 fma per
// tap, taps outside the grid contribute x = +0 (an fma with +0 leaves the accumulator as it is), bf16 rounding at the same points.
// dz = bf16(dy * act'(z)) is formed with act_bwd_kernel's expression.  dw / db are fp32 sums over another partition of the pixels.
#include "common.h"
#include "dwconv_plan.h"

int g_dwconv_band = 1;    // du_set_option key 19: 0 = the kernels of elementwise.hip everywhere, 1 = the band kernels where du_dwconv_plan
                          // says so (default); tuning aid: bits 0-7 >= 2 = bands of that many rows in forward and data gradient, bits 8-15 >= 2 =
                          // in the weight gradient (0 there: the rule of band_geom)

namespace {

constexpr int XT = 2;       // columns per thread
constexpr int CVB = 8;      // channel vectors per workgroup (a slab of 64 channels)
constexpr int NL = 32;      // work items per workgroup
constexpr int V = 8;        // bf16 per 16-byte vector

struct BandGeom {
  long ld, bs;              // pixel and image stride in elements
  int C, R, nlev, nslab;
  int Hs[3], Ws[3], s0[3];  // the grids of one image: height, width, first pixel
  int ncg[3], nbands[3], nitems[3], nblk[3];
  int wg0[4];               // first workgroup (linear index) of a level; wg0[nlev] = all
  int row0[3];              // first partial row of a level (weight gradient)
};

// workgroups are dealt round-robin to the 8 XCDs: the index under which consecutive values share an XCD (gemm_p8.hip)
__device__ __forceinline__ int xcd_linear_index() {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

#define LEV(a, l) ((l) == 0 ? (a)[0] : ((l) == 1 ? (a)[1] : (a)[2]))

struct Item {
  bool on;                  // this thread has work (an item and a channel vector)
  int y0, y1, x0, Hs, Ws, cg, ncg, c0, prow, slab;
  long base;                // element offset of (image, grid, channel vector)
};

__device__ __forceinline__ Item band_item(const BandGeom& G) {
  const int lin = xcd_linear_index();
  int l = 0;
  if (G.nlev > 1 && lin >= G.wg0[1]) l = 1;
  if (G.nlev > 2 && lin >= G.wg0[2]) l = 2;
  const int nblk = LEV(G.nblk, l), r = lin - LEV(G.wg0, l);
  const int slab = r / nblk, blk = r - slab * nblk;
  const int lane = threadIdx.x / CVB, tcv = threadIdx.x % CVB;
  const int item = blk * NL + lane, cv = slab * CVB + tcv;
  Item it;
  it.ncg = LEV(G.ncg, l);
  it.Hs = LEV(G.Hs, l);
  it.Ws = LEV(G.Ws, l);
  it.prow = LEV(G.row0, l) + blk;
  it.slab = slab;
  it.on = item < LEV(G.nitems, l) && cv * V < G.C;
  const int nb = LEV(G.nbands, l);
  const int t = item / it.ncg, b = t / nb, band = t - b * nb;
  it.cg = item - t * it.ncg;
  it.x0 = it.cg * XT;
  it.y0 = it.on ? band * G.R : 0;
  it.y1 = it.on ? min(it.Hs, it.y0 + G.R) : 0;
  it.c0 = cv * V;
  it.base = it.on ? (long)b * G.bs + (long)LEV(G.s0, l) * G.ld + it.c0 : 0;
  return it;
}

struct Row { uint4 c[XT + 2]; };      // columns x0 - 1 .. x0 + XT of one row, packed

__device__ __forceinline__ Row zero_row() {
  Row r;
#pragma unroll
  for (int c = 0; c < XT + 2; c++) r.c[c] = make_uint4(0, 0, 0, 0);
  return r;
}

// row yi of the item's grid; zeros outside the grid
__device__ __forceinline__ Row load_row(const bf16_t* __restrict__ p, const Item& it, long ld, int yi, bool want) {
  Row r;
  const bool rv = want && yi >= 0 && yi < it.Hs;
  const bf16_t* row = p + it.base + (long)yi * it.Ws * ld;
#pragma unroll
  for (int c = 0; c < XT + 2; c++) {
    const int xi = it.x0 - 1 + c;
    r.c[c] = (rv && xi >= 0 && xi < it.Ws) ? *(const uint4*)(row + (long)xi * ld) : make_uint4(0, 0, 0, 0);
  }
  return r;
}

__device__ __forceinline__ void load_taps(const float* __restrict__ w, const float* __restrict__ bias, int c0, bool flip, float (&wt)[9][V],
                                          float (&bs)[V]) {
#pragma unroll
  for (int j = 0; j < V; j++) {
    bs[j] = bias ? bias[c0 + j] : 0.f;
#pragma unroll
    for (int t = 0; t < 9; t++) wt[t][j] = w[(c0 + j) * 9 + (flip ? 8 - t : t)];
  }
}

// XT outputs from the three window rows: bias, then taps row-major (the order of dwconv_row4_kernel)
__device__ __forceinline__ void stencil(const Row& a, const Row& b, const Row& c, const float (&wt)[9][V], const float (&bs)[V],
                                        float (&acc)[XT][V]) {
#pragma unroll
  for (int t = 0; t < XT; t++)
#pragma unroll
    for (int j = 0; j < V; j++) acc[t][j] = bs[j];
#pragma unroll
  for (int dy = 0; dy < 3; dy++) {
    const Row& r = dy == 0 ? a : (dy == 1 ? b : c);
#pragma unroll
    for (int cc = 0; cc < XT + 2; cc++) {
      const Vec16<bf16_t> v = as_vec<bf16_t>(r.c[cc]);
      float f[V];
#pragma unroll
      for (int j = 0; j < V; j++) f[j] = to_f32(v.v[j]);
#pragma unroll
      for (int dx = 0; dx < 3; dx++) {
        const int t = cc - dx;                      // column cc is tap dx of output t = cc - dx
        if (t >= 0 && t < XT) {
#pragma unroll
          for (int j = 0; j < V; j++) acc[t][j] += f[j] * wt[dy * 3 + dx][j];
        }
      }
    }
  }
}

// forward (FLIP = false: y = act(conv + bias), z = the pre-activation when given) and plain data gradient (FLIP = true, no bias, no act).
// ACT >= 0: the activation at compile time (apply_act's switch inside the element loop is a chain of scalar branches that keeps the
// compiler from interleaving the erf polynomials of a row's 16 elements; one or two waves per SIMD have nothing else to hide them
// behind), ACT < 0: the runtime argument.
template <bool FLIP, int ACT>
__global__ __launch_bounds__(256) void dwconv_band_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, bf16_t* __restrict__ y, bf16_t* __restrict__ z,
                                                          BandGeom G, int act_rt) {
  const int act = ACT >= 0 ? ACT : act_rt;
  const Item it = band_item(G);
  if (!it.on) return;
  float wt[9][V], bs[V];
  load_taps(w, bias, it.c0, FLIP, wt, bs);
  Row a = load_row(x, it, G.ld, it.y0 - 1, true), b = load_row(x, it, G.ld, it.y0, true), c = load_row(x, it, G.ld, it.y0 + 1, true);
  for (int yo = it.y0; yo < it.y1; yo++) {
    const Row n = load_row(x, it, G.ld, yo + 2, yo + 2 <= it.y1);      // the row below, requested before this one is consumed
    float acc[XT][V];
    stencil(a, b, c, wt, bs, acc);
    const long off = it.base + ((long)yo * it.Ws + it.x0) * G.ld;
#pragma unroll
    for (int t = 0; t < XT; t++) {
      Vec16<bf16_t> o;
      if (!FLIP && z) {
#pragma unroll
        for (int j = 0; j < V; j++) o.v[j] = from_f32<bf16_t>(acc[t][j]);
        *(uint4*)(z + off + (long)t * G.ld) = as_u4(o);
      }
#pragma unroll
      for (int j = 0; j < V; j++) o.v[j] = from_f32<bf16_t>(FLIP ? acc[t][j] : apply_act(acc[t][j], act));
      *(uint4*)(y + off + (long)t * G.ld) = as_u4(o);
    }
    a = b; b = c; c = n;
  }
}

// dz = bf16(dy * act'(z)) of one pixel vector: act_bwd_kernel's expression
__device__ __forceinline__ uint4 act_dz(uint4 zr, uint4 gr, int act) {
  const Vec16<bf16_t> a = as_vec<bf16_t>(zr), g = as_vec<bf16_t>(gr);
  Vec16<bf16_t> o;
#pragma unroll
  for (int j = 0; j < V; j++) o.v[j] = from_f32<bf16_t>(to_f32(g.v[j]) * act_grad(to_f32(a.v[j]), act));
  return as_u4(o);
}

// Data gradient with the activation's derivative applied on load: dz = bf16(dy * act'(z)) is formed once per pixel of the band and its
// two halo rows (a thread forms its own XT columns and hands its edge columns to its neighbours through LDS: erff + exp per element are
// the cost of this kernel, not the bytes), written out for the weight gradient (own rows only), and dx = dz (*) flipped filter.
// Every thread of the workgroup walks R + 2 rows -- one __syncthreads per row, two LDS buffers -- whether it has work or not.
// SELF: some row is cut by a workgroup boundary (a grid wider than 64 columns, a width / XT that does not divide 32): the edge threads
// then form the neighbour column themselves.  Compile-time, because the compiler evaluates both act_dz of that path for every thread.
template <int ACT, bool SELF>
__global__ __launch_bounds__(256) void dwconv_band_dgrad_act_kernel(const bf16_t* __restrict__ z, const bf16_t* __restrict__ dy,
                                                                    const float* __restrict__ w, bf16_t* __restrict__ dx,
                                                                    bf16_t* __restrict__ dzo, BandGeom G, int act_rt) {
  __shared__ uint4 edge[2][256][2];
  const int act = ACT >= 0 ? ACT : act_rt;
  const Item it = band_item(G);
  const int tid = threadIdx.x, lane = tid / CVB;
  float wt[9][V], bs[V];
  if (it.on) load_taps(w, nullptr, it.c0, true, wt, bs);
  else {
#pragma unroll
    for (int j = 0; j < V; j++) {
      bs[j] = 0.f;
#pragma unroll
      for (int t = 0; t < 9; t++) wt[t][j] = 0.f;
    }
  }
  // the neighbour column comes from the neighbouring thread when that thread works on the same row; a row cut by the workgroup's
  // boundary (grids wider than 64 columns, widths that do not divide 64) makes the edge thread form that column itself
  const bool lz = it.cg == 0, rz = it.cg == it.ncg - 1;
  const bool lself = SELF && !lz && lane == 0, rself = SELF && !rz && lane == NL - 1;
  Row a = zero_row(), b = zero_row(), c = zero_row();
  uint4 zc[XT], gc[XT];
  {
    const int yi = it.y0 - 1;
    const bool rv = it.on && yi >= 0;
    const long off = it.base + ((long)yi * it.Ws + it.x0) * G.ld;
#pragma unroll
    for (int t = 0; t < XT; t++) {
      zc[t] = rv ? *(const uint4*)(z + off + (long)t * G.ld) : make_uint4(0, 0, 0, 0);
      gc[t] = rv ? *(const uint4*)(dy + off + (long)t * G.ld) : make_uint4(0, 0, 0, 0);
    }
  }
  for (int i = 0; i < G.R + 2; i++) {
    const int yi = it.y0 - 1 + i, p = i & 1;
    const bool rv = it.on && yi >= 0 && yi < it.Hs && yi <= it.y1;
    // request row yi + 1 before row yi is consumed
    uint4 zn[XT], gn[XT];
    {
      const bool nv = it.on && yi + 1 < it.Hs && yi + 1 <= it.y1;
      const long off = it.base + ((long)(yi + 1) * it.Ws + it.x0) * G.ld;
#pragma unroll
      for (int t = 0; t < XT; t++) {
        zn[t] = nv ? *(const uint4*)(z + off + (long)t * G.ld) : make_uint4(0, 0, 0, 0);
        gn[t] = nv ? *(const uint4*)(dy + off + (long)t * G.ld) : make_uint4(0, 0, 0, 0);
      }
    }
    Row n;
    const long roff = it.base + ((long)yi * it.Ws + it.x0) * G.ld;
#pragma unroll
    for (int t = 0; t < XT; t++) n.c[1 + t] = rv ? act_dz(zc[t], gc[t], act) : make_uint4(0, 0, 0, 0);
    if (rv && yi >= it.y0 && yi < it.y1) {
#pragma unroll
      for (int t = 0; t < XT; t++) *(uint4*)(dzo + roff + (long)t * G.ld) = n.c[1 + t];
    }
    edge[p][tid][0] = n.c[1];
    edge[p][tid][1] = n.c[XT];
    __syncthreads();
    n.c[0] = make_uint4(0, 0, 0, 0);
    n.c[XT + 1] = make_uint4(0, 0, 0, 0);
    if (rv) {
      if (lself) n.c[0] = act_dz(*(const uint4*)(z + roff - G.ld), *(const uint4*)(dy + roff - G.ld), act);
      else if (!lz) n.c[0] = edge[p][tid - CVB][1];
      if (rself) n.c[XT + 1] = act_dz(*(const uint4*)(z + roff + (long)XT * G.ld), *(const uint4*)(dy + roff + (long)XT * G.ld), act);
      else if (!rz) n.c[XT + 1] = edge[p][tid + CVB][0];
    }
    a = b; b = c; c = n;
    const int yo = yi - 1;
    if (i >= 2 && it.on && yo < it.y1) {
      float acc[XT][V];
      stencil(a, b, c, wt, bs, acc);
      const long off = it.base + ((long)yo * it.Ws + it.x0) * G.ld;
#pragma unroll
      for (int t = 0; t < XT; t++) {
        Vec16<bf16_t> o;
#pragma unroll
        for (int j = 0; j < V; j++) o.v[j] = from_f32<bf16_t>(acc[t][j]);
        *(uint4*)(dx + off + (long)t * G.ld) = as_u4(o);
      }
    }
#pragma unroll
    for (int t = 0; t < XT; t++) { zc[t] = zn[t]; gc[t] = gn[t]; }
  }
}

// dw[c][tap] = sum_pix x[pix + tap][c] * dz[pix][c], db[c] = sum_pix dz[pix][c]: 10 x 8 fp32 partials per thread over its band (x through
// the same three-row window, dz at the centre), ONE block reduction through LDS (two passes of five taps), one partial row per workgroup:
// part[row][tap][C], row = (level, item block); the slabs of a block write disjoint channel ranges of the same row.
__global__ __launch_bounds__(256) void dwconv_band_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dz,
                                                                float* __restrict__ part, BandGeom G) {
  __shared__ float red[5][256 * V];
  const Item it = band_item(G);
  float aw[10][V];
#pragma unroll
  for (int k = 0; k < 10; k++)
#pragma unroll
    for (int j = 0; j < V; j++) aw[k][j] = 0.f;
  if (it.on) {
    Row a = load_row(x, it, G.ld, it.y0 - 1, true), b = load_row(x, it, G.ld, it.y0, true), c = load_row(x, it, G.ld, it.y0 + 1, true);
    uint4 gc[XT];
#pragma unroll
    for (int t = 0; t < XT; t++) gc[t] = *(const uint4*)(dz + it.base + ((long)it.y0 * it.Ws + it.x0 + t) * G.ld);
    for (int yo = it.y0; yo < it.y1; yo++) {
      const Row n = load_row(x, it, G.ld, yo + 2, yo + 2 <= it.y1);
      uint4 gn[XT];
#pragma unroll
      for (int t = 0; t < XT; t++)
        gn[t] = yo + 1 < it.y1 ? *(const uint4*)(dz + it.base + ((long)(yo + 1) * it.Ws + it.x0 + t) * G.ld) : make_uint4(0, 0, 0, 0);
      float gf[XT][V];
#pragma unroll
      for (int t = 0; t < XT; t++) {
        const Vec16<bf16_t> g = as_vec<bf16_t>(gc[t]);
#pragma unroll
        for (int j = 0; j < V; j++) { gf[t][j] = to_f32(g.v[j]); aw[9][j] += gf[t][j]; }
      }
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        const Row& r = ky == 0 ? a : (ky == 1 ? b : c);
#pragma unroll
        for (int cc = 0; cc < XT + 2; cc++) {
          const Vec16<bf16_t> v = as_vec<bf16_t>(r.c[cc]);
          float f[V];
#pragma unroll
          for (int j = 0; j < V; j++) f[j] = to_f32(v.v[j]);
#pragma unroll
          for (int kx = 0; kx < 3; kx++) {
            const int t = cc - kx;                   // input column cc is tap kx of output pixel t
            if (t >= 0 && t < XT) {
#pragma unroll
              for (int j = 0; j < V; j++) aw[ky * 3 + kx][j] += f[j] * gf[t][j];
            }
          }
        }
      }
      a = b; b = c; c = n;
#pragma unroll
      for (int t = 0; t < XT; t++) gc[t] = gn[t];
    }
  }
  const int slab = it.slab;
  constexpr int NCOL = CVB * V;                      // channel columns of a slab
#pragma unroll
  for (int half = 0; half < 2; half++) {
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
      for (int j = 0; j < V; j++) red[k][threadIdx.x * V + j] = aw[half * 5 + k][j];
    __syncthreads();
    for (int o = threadIdx.x; o < 5 * NCOL; o += 256) {
      const int k5 = o / NCOL, ci = o - k5 * NCOL;
      const int ch = slab * NCOL + ci;
      if (ch >= G.C) continue;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int q = 0; q < NL; q += 4) {
        s0 += red[k5][q * NCOL + ci];
        s1 += red[k5][(q + 1) * NCOL + ci];
        s2 += red[k5][(q + 2) * NCOL + ci];
        s3 += red[k5][(q + 3) * NCOL + ci];
      }
      part[((long)it.prow * 10 + half * 5 + k5) * G.C + ch] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
  }
}

// second stage: dw[c][k] (+)= sum_rows part[row][k][c], db[c] (+)= sum_rows part[row][9][c].  Workgroup = 32 columns x 8 row lanes: a
// thread adds every eighth row of its column (coalesced 128-byte reads, four independent accumulators: at most 64 loads, none waiting
// for another), the eight lanes meet in LDS.  A few hundred rows at most.
__global__ __launch_bounds__(256) void dwconv_band_finalize_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                   float* __restrict__ db, int rows, int C, int accum) {
  __shared__ float red[8][33];
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + col, n = C * 10;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n) {
    int r = sl;
    for (; r + 24 < rows; r += 32) {
      s0 += part[(long)r * n + i];
      s1 += part[(long)(r + 8) * n + i];
      s2 += part[(long)(r + 16) * n + i];
      s3 += part[(long)(r + 24) * n + i];
    }
    for (; r < rows; r += 8) s0 += part[(long)r * n + i];
  }
  red[sl][col] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 8; q++) t += red[q][col];
    const int k = i / C, c = i - k * C;
    if (k < 9) dw[c * 9 + k] = accum ? dw[c * 9 + k] + t : t;
    else if (db) db[c] = accum ? db[c] + t : t;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
bool band_shape_ok(int dtype, int B, int H, int W, int C, int pyramid) {
  if (!g_dwconv_band || dtype != DU_BF16 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % V) return false;
  if (pyramid) {
    if ((H & 1) || (W & 1) || (W / 2) % XT) return false;
    if ((long)B * 21 * ((long)H * W / 4) * ((C + 63) / 64) > 0x3fffffffL) return false;
  } else {
    if (W % XT) return false;
    if ((long)B * H * W * ((C + 63) / 64) > 0x3fffffffL) return false;
  }
  return true;
}

// workgroups and partial rows of a launch with bands of G.R rows
void band_count(BandGeom& G, int B) {
  int wg = 0, row = 0;
  for (int l = 0; l < G.nlev; l++) {
    G.ncg[l] = G.Ws[l] / XT;
    G.nbands[l] = (G.Hs[l] + G.R - 1) / G.R;
    G.nitems[l] = B * G.nbands[l] * G.ncg[l];
    G.nblk[l] = (G.nitems[l] + NL - 1) / NL;
    G.wg0[l] = wg; G.row0[l] = row;
    wg += G.nblk[l] * G.nslab; row += G.nblk[l];
  }
  G.wg0[G.nlev] = wg;
}

int band_rows(const BandGeom& G) { return G.row0[G.nlev - 1] + G.nblk[G.nlev - 1]; }

// The geometry of a launch with bands of R rows.
BandGeom band_geom(int B, int H, int W, int C, int pyramid, long ld, long bs, int R) {
  BandGeom G{};
  G.ld = ld; G.bs = bs; G.C = C; G.R = R;
  G.nslab = (C + CVB * V - 1) / (CVB * V);
  if (pyramid) {
    const int n = (H * W) >> 2;
    G.nlev = 3;
    G.Hs[0] = 2 * H; G.Ws[0] = 2 * W; G.s0[0] = 0;
    G.Hs[1] = H; G.Ws[1] = W; G.s0[1] = 16 * n;
    G.Hs[2] = H >> 1; G.Ws[2] = W >> 1; G.s0[2] = 20 * n;
  } else {
    G.nlev = 1;
    G.Hs[0] = H; G.Ws[0] = W; G.s0[0] = 0;
  }
  band_count(G, B);
  return G;
}

// The band height.  Every workgroup walks R rows (plus a prologue worth about a row and a half: item decode, 72 taps, the
// first three rows), all workgroups start together, and the kernels are bound by their own instructions (the erf of GELU and its
// derivative: ~550 of the forward's ~800 VALU instructions per row) and by the latency of a row's loads, not by bytes: with 210-230
// registers two workgroups share a CU, and a launch takes as long as the CU with the most rounds of two.  So R is the band height in
// 4 .. 16 with the least (workgroups / 512, rounded up) x (R + 1.5): at the token pyramid of the train step 6 rows = 472 workgroups
// (measured: forward 25.7 us, 8 rows = 336 workgroups 30.1, 11 rows = 256 workgroups 29.0, 16 rows 38.8).
// rows_cap > 0 (weight gradient): taller bands until at most that many partial rows.
int band_height(int B, int H, int W, int C, int pyramid, int rows_cap) {
  BandGeom G = band_geom(B, H, W, C, pyramid, C, 0, 4);
  const int forced = rows_cap > 0 ? (g_dwconv_band >> 8) & 0xff : (g_dwconv_band >= 2 ? g_dwconv_band & 0xff : 0);
  if (forced >= 2) G.R = forced;
  else {
    const int slots = 512;                     // the CUs of the MI355X x two workgroups side by side
    long best = 0;
    int pick = 4;
    for (int r = 4; r <= 16; r++) {            // (the first, shortest band among equal costs)
      G.R = r;
      band_count(G, B);
      const long cost = (long)((G.wg0[G.nlev] + slots - 1) / slots) * (2 * r + 3);
      if (r == 4 || cost < best) { best = cost; pick = r; }
    }
    G.R = pick;
  }
  for (;;) {
    band_count(G, B);
    if (rows_cap <= 0 || band_rows(G) <= rows_cap || G.R >= G.Hs[0]) break;
    G.R *= 2;
  }
  return G.R;
}

constexpr int WGRAD_ROWS_CAP = 512;

void band_forward(const bf16_t* x, const float* w, const float* bias, bf16_t* y, bf16_t* z, const BandGeom& G, int act, hipStream_t st) {
  const dim3 grid(G.wg0[G.nlev]), block(256);
  if (act == DU_ACT_GELU) hipLaunchKernelGGL((dwconv_band_kernel<false, DU_ACT_GELU>), grid, block, 0, st, x, w, bias, y, z, G, act);
  else if (act == DU_ACT_NONE) hipLaunchKernelGGL((dwconv_band_kernel<false, DU_ACT_NONE>), grid, block, 0, st, x, w, bias, y, z, G, act);
  else hipLaunchKernelGGL((dwconv_band_kernel<false, -1>), grid, block, 0, st, x, w, bias, y, z, G, act);
}

// data gradient (the activation's derivative on load: dz is written for the weight gradient), weight gradient, second stage
void band_backward(const DwconvPlan& plan, const bf16_t* z, const bf16_t* dy, const bf16_t* x, const float* w, bf16_t* dx, float* dw,
                   float* db, bf16_t* dz, int B, int H, int W, int C, int pyramid, long ld, long bs, int act, float* ws, hipStream_t st) {
  const BandGeom G = band_geom(B, H, W, C, pyramid, ld, bs, plan.R);
  const bf16_t* g = dy;
  if (plan.act_bwd == DU_DW_ACT_ON_LOAD) {
    bool cut = false;                          // a row shared by two workgroups
    for (int l = 0; l < G.nlev; l++) cut = cut || NL % G.ncg[l] != 0;
    const dim3 grid(G.wg0[G.nlev]), block(256);
    if (act == DU_ACT_GELU && !cut) hipLaunchKernelGGL((dwconv_band_dgrad_act_kernel<DU_ACT_GELU, false>), grid, block, 0, st, z, dy, w, dx, dz, G, act);
    else if (act == DU_ACT_GELU) hipLaunchKernelGGL((dwconv_band_dgrad_act_kernel<DU_ACT_GELU, true>), grid, block, 0, st, z, dy, w, dx, dz, G, act);
    else hipLaunchKernelGGL((dwconv_band_dgrad_act_kernel<-1, true>), grid, block, 0, st, z, dy, w, dx, dz, G, act);
    g = dz;
  } else {
    hipLaunchKernelGGL((dwconv_band_kernel<true, DU_ACT_NONE>), dim3(G.wg0[G.nlev]), dim3(256), 0, st, dy, w, (const float*)nullptr, dx,
                       (bf16_t*)nullptr, G, (int)DU_ACT_NONE);
  }
  const BandGeom GW = band_geom(B, H, W, C, pyramid, ld, bs, plan.wgrad_R);
  hipLaunchKernelGGL(dwconv_band_wgrad_kernel, dim3(GW.wg0[GW.nlev]), dim3(256), 0, st, x, g, ws, GW);
  hipLaunchKernelGGL(dwconv_band_finalize_kernel, dim3((C * 10 + 31) / 32), dim3(256), 0, st, (const float*)ws, dw, db, plan.rows, C, 0);
}

// the 4-pixel row kernels need every grid of the token pyramid -- widths 2W, W, W / 2 -- to be a multiple of 4
bool row4_ok(int W) {
  static const bool off = DU_GETENV("DU_DWCONV_NO_ROW4") != nullptr;      // debugging / A-B aid
  return !off && W % 8 == 0;
}

// pixels per workgroup of the row family's weight gradient
int row_wgrad_strip(long npix, int C, int v) {
  // ~512 workgroups per launch, but at least 4 pixels per pixel lane so the LDS reduction stays amortised
  const int cvb = (C / v) < 256 ? (C / v) : 256;
  const int np = 256 / cvb;
  long strip = (npix + 511) / 512;           // 512 strips: the partial buffer the finalize kernel re-reads halves (measured vs 1024)
  if (strip < (long)np * 4) strip = (long)np * 4;
  return (int)((strip + 3) / 4 * 4);         // whole 4-pixel groups (row form of the kernel)
}

}  // namespace

DwconvPlan du_dwconv_plan(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act) {
  DwconvPlan p{};
  p.rc = DU_ERR_BAD_ARG;
  const int v = dtype == DU_BF16 ? 8 : 4;
  if ((dtype != DU_BF16 && dtype != DU_F32) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % v) return p;
  const long pix = pyramid ? 21L * (((long)H * W) >> 2) : (long)H * W;      // of one image
  const bool dense = ld == C && bs == pix * C;
  p.act_bwd = act == DU_ACT_NONE ? DU_DW_ACT_NONE : DU_DW_ACT_PASS;
  if (band_shape_ok(dtype, B, H, W, C, pyramid) && ld % V == 0 && bs % V == 0 && (pyramid || act == DU_ACT_NONE)) {
    p.kernel = DU_DW_BAND;
    p.R = band_height(B, H, W, C, pyramid, 0);
    if (act != DU_ACT_NONE) p.act_bwd = DU_DW_ACT_ON_LOAD;
    p.wgrad = DU_DWW_BAND;
    p.wgrad_R = band_height(B, H, W, C, pyramid, WGRAD_ROWS_CAP);
    p.rows = band_rows(band_geom(B, H, W, C, pyramid, ld, bs, p.wgrad_R));      // one per item block: its slabs share the row
    p.ws_elems = (int64_t)p.rows * 10 * C;
    p.rc = pyramid && !dense ? DU_ERR_BAD_ARG : DU_OK;
    return p;
  }
  const bool four = pyramid && dtype == DU_BF16 && row4_ok(W);
  p.kernel = four ? DU_DW_ROW4 : DU_DW_ROW;
  p.strip = row_wgrad_strip((long)B * pix, C, v);
  p.wgrad = !pyramid ? DU_DWW_ROW : (four && p.strip % 4 == 0 ? DU_DWW_PYR_ROW4 : DU_DWW_PYR);
  p.rows = (int)(((long)B * pix + p.strip - 1) / p.strip);
  p.ws_elems = (int64_t)p.rows * 10 * C;
  if (ld % v || bs % v || (pyramid && ((H & 1) || (W & 1) || !dense))) p.rc = DU_ERR_BAD_ARG;
  else if (act != DU_ACT_NONE && !dense) p.rc = DU_ERR_UNSUPPORTED;      // act_bwd_kernel is one launch over contiguous elements
  else p.rc = DU_OK;
  return p;
}

extern "C" int du_dwconv3x3_plan_describe(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act, int64_t* out,
                                          int n) {
  if (!out || n < 7) return DU_ERR_BAD_ARG;
  const DwconvPlan p = du_dwconv_plan(dtype, ld, bs, B, H, W, C, pyramid, act);
  out[0] = p.rc; out[1] = p.kernel; out[2] = p.R; out[3] = p.act_bwd; out[4] = p.wgrad; out[5] = p.rows; out[6] = p.ws_elems;
  return 7;
}

extern "C" int64_t du_dwconv3x3_bwd_ws_elems(int dtype, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act) {
  return du_dwconv_plan(dtype, ld, bs, B, H, W, C, pyramid, act).ws_elems;
}

extern "C" int du_dwconv3x3_fwd(int dtype, const void* x, const float* w, const float* bias, void* y, void* z, int64_t ld, int64_t bs, int B,
                                int H, int W, int C, int pyramid, int act, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const DwconvPlan p = du_dwconv_plan(dtype, ld, bs, B, H, W, C, pyramid, act);
  if (p.rc != DU_OK) return p.rc;
  if (!x || !w || !y) return DU_ERR_BAD_ARG;
  if (p.kernel == DU_DW_BAND)
    band_forward((const bf16_t*)x, w, bias, (bf16_t*)y, (bf16_t*)z, band_geom(B, H, W, C, pyramid, ld, bs, p.R), act, st);
  else du_dwconv_row_run(p, dtype, x, w, bias, y, z, ld, bs, B, H, W, C, pyramid, act, false, st);
  return du_check_launch();
}

extern "C" int du_dwconv3x3_bwd(int dtype, const void* z, const void* dy, const void* x, const float* w, void* dx, float* dw, float* db,
                                void* dz, int64_t ld, int64_t bs, int B, int H, int W, int C, int pyramid, int act, float* ws,
                                int64_t ws_elems, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const DwconvPlan p = du_dwconv_plan(dtype, ld, bs, B, H, W, C, pyramid, act);
  if (p.rc != DU_OK) return p.rc;
  if (!dy || !x || !w || !dx || !dw || !ws || ws_elems < p.ws_elems) return DU_ERR_BAD_ARG;
  if (p.act_bwd != DU_DW_ACT_NONE && (!z || !dz)) return DU_ERR_BAD_ARG;
  if (p.kernel == DU_DW_BAND) {
    band_backward(p, (const bf16_t*)z, (const bf16_t*)dy, (const bf16_t*)x, w, (bf16_t*)dx, dw, db, (bf16_t*)dz, B, H, W, C, pyramid, ld, bs,
                  act, ws, st);
    return du_check_launch();
  }
  const void* g = dy;
  if (p.act_bwd == DU_DW_ACT_PASS) {
    const long pix = pyramid ? 21L * (((long)H * W) >> 2) : (long)H * W;
    const int rc = du_act_bwd(dtype, z, dy, dz, (int64_t)B * pix * C, act, stream);
    if (rc != DU_OK) return rc;
    g = dz;
  }
  du_dwconv_row_run(p, dtype, g, w, nullptr, dx, nullptr, ld, bs, B, H, W, C, pyramid, DU_ACT_NONE, true, st);
  du_dwconv_row_wgrad(p, dtype, x, g, dw, db, ld, bs, B, H, W, C, ws, st);
  return du_check_launch();
}
