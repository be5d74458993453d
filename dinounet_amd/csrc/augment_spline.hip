// The training augmentation with the interpolation batchgenerators itself uses (GPUAugment2D(interpolation="spline")):
// scipy.ndimage.map_coordinates(order=3, mode="constant", cval=0) for the image of SpatialTransform, the order-1 label rule with -1 as a
// label of its own, skimage's resize (scipy.ndimage.zoom(order=3, mode="nearest", grid_mode=True) + clip) for the up-sampling half of
// SimulateLowResolutionTransform, and MaskTransform + RemoveLabelTransform(-1, 0) as the last pass.  Everything a pixel value goes through
// is fp64 with one rounding to fp32 at the store, which is what scipy does for float32 input.
//
//   du_aug_spline_coeffs    cubic B-spline coefficients of the listed planes with whole-sample mirror boundaries and no padding
//                           (spline_filter(mode="mirror")).  The prefilter is the two-sided sequence sqrt(3) z^|k|, z = sqrt(3) - 2, cut at
//                           |k| <= 32 (|z|^33 < 2e-19) as in preprocess.hip: no recurrence, no state.  Rows first (a 256-sample segment
//                           and its 32-sample halos staged in LDS, every global sample read once per workgroup), then columns (32 x 64
//                           tiles with their halo rows in LDS, eight consecutive rows per thread over a 72-row register window).
//   du_aug_spatial_spline   image and labels of the whole batch in one launch, 16 x 16 output tiles.  A sample whose matrix is exactly
//                           [1, 0, 0, 1] is batchgenerators' integer centre crop (bits copied); every other pixel outside [0, n - 1] is 0,
//                           inside it is the 4 x 4 sum over coefficients whose tap indices are MIRRORED at the border.
//   du_aug_lowres_spline    low grid by nearest source pixel, its min / max per plane, then the two up-sampling passes of
//                           preprocess.hip's spline_axis_kernel with per-plane sizes from a device array, clipped to that min / max
//   du_aug_mask             label < 0: the masked channels become 0 and the label becomes 0
#include "common.h"

namespace {

constexpr int HZ = 32;                            // prefilter horizon
constexpr double SQRT3 = 1.7320508075688772, POLE = SQRT3 - 2.0;

// scipy "mirror" (d c b | a b c d | c b a): period 2 (n - 1), any distance from the line
__device__ __forceinline__ int mirror(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i = (i < 0 ? -i : i) % p;
  return i >= n ? p - i : i;
}

// cubic B-spline weights of the taps floor - 1 .. floor + 2 at the fraction t
__device__ __forceinline__ void bspline_weights(double t, double* w) {
  const double u = 1.0 - t;
  w[0] = u * u * u * (1.0 / 6.0);
  w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) * (1.0 / 6.0);
  w[2] = (4.0 - 6.0 * u * u + 3.0 * u * u * u) * (1.0 / 6.0);
  w[3] = t * t * t * (1.0 / 6.0);
}

// ------------------------------------------------------------------------------------------------------------- coefficients
constexpr int SEG = 256;                          // row pass: outputs of one workgroup
// out[j] (H, W) fp64 = rows of plane plane_idx[j] filtered along x.  One work item = one segment of one row.
__global__ __launch_bounds__(256) void coef_rows_kernel(const float* __restrict__ in, const int* __restrict__ plane_idx, double* __restrict__ out,
                                                        int in_planes, int H, int W, int nseg, long items) {
  __shared__ double s[SEG + 2 * HZ];
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int sg = (int)(item % nseg);
    const long r = item / nseg;
    const int y = (int)(r % H);
    const long j = r / H;
    const int pi = plane_idx[j];
    const bool known = pi >= 0 && pi < in_planes;               // an index outside the input reads as a plane of zeros
    const float* line = in + ((long)(known ? pi : 0) * H + y) * W;
    const int x0 = sg * SEG;
    __syncthreads();                              // the previous item's reads of s
    for (int i = threadIdx.x; i < SEG + 2 * HZ; i += 256) s[i] = known ? (double)line[mirror(x0 - HZ + i, W)] : 0.0;
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x < W) {
      const double* c = s + threadIdx.x + HZ;
      double acc = SQRT3 * c[0], w = SQRT3;
#pragma unroll
      for (int k = 1; k <= HZ; k++) {
        w *= POLE;
        acc += w * (c[-k] + c[k]);
      }
      out[(j * H + y) * W + x] = W == 1 ? c[0] : acc;           // a line of length 1 is its own coefficient
    }
  }
}

constexpr int CX = 32, CY = 64, CR = CY + 2 * HZ, CQ = 8;        // column pass: tile, staged rows, rows per thread
// out[j] = in[j] filtered along y, both (H, W) fp64.  One work item = one 32 x 64 tile.
__global__ __launch_bounds__(256) void coef_cols_kernel(const double* __restrict__ in, double* __restrict__ out, int H, int W, int ntx, int nty,
                                                        long items) {
  __shared__ double s[CR][CX];
  const int tx = threadIdx.x & (CX - 1), ty = threadIdx.x / CX;
  double w[HZ + 1];
  w[0] = SQRT3;
#pragma unroll
  for (int k = 1; k <= HZ; k++) w[k] = w[k - 1] * POLE;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int bx = (int)(item % ntx);
    const long r = item / ntx;
    const int by = (int)(r % nty);
    const long j = r / nty;
    const double* pl = in + j * H * W;
    const int x = bx * CX + tx, y0 = by * CY;
    __syncthreads();
    for (int rr = ty; rr < CR; rr += 256 / CX) s[rr][tx] = x < W ? pl[(long)mirror(y0 - HZ + rr, H) * W + x] : 0.0;
    __syncthreads();
    double acc[CQ];
#pragma unroll
    for (int q = 0; q < CQ; q++) acc[q] = 0.0;
#pragma unroll
    for (int k = 0; k < CQ + 2 * HZ; k++) {                     // staged row ty * 8 + k is HZ - k + q rows above output q
      const double v = s[ty * CQ + k][tx];
#pragma unroll
      for (int q = 0; q < CQ; q++) {
        const int d = k - q - HZ;
        if (d >= -HZ && d <= HZ) acc[q] += w[d < 0 ? -d : d] * v;
      }
    }
#pragma unroll
    for (int q = 0; q < CQ; q++) {
      const int y = y0 + ty * CQ + q;
      if (x < W && y < H) out[(j * H + y) * W + x] = H == 1 ? s[HZ + ty * CQ + q][tx] : acc[q];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- spatial
constexpr int ST = 16;                            // output tile edge
// params per sample as in du_aug_spatial; slot[b * C + c] = which of the `coef_planes` planes of `coef` holds that plane's coefficients
// (not read for a sample whose matrix is the identity; a slot outside the scratch gives zeros)
__global__ __launch_bounds__(256) void spatial_spline_kernel(const float* __restrict__ din, const float* __restrict__ sin_, const float* __restrict__ prm,
                                                             const double* __restrict__ coef, const int* __restrict__ slot, float* __restrict__ dout,
                                                             float* __restrict__ sout, int coef_planes, int C, int Hi, int Wi, int Ho, int Wo,
                                                             int ntx, int nty, long items) {
  const int lx = threadIdx.x & (ST - 1), ly = threadIdx.x / ST;
  const long ni = (long)Hi * Wi, no = (long)Ho * Wo;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int bx = (int)(item % ntx);
    const long r = item / ntx;
    const int by = (int)(r % nty);
    const long b = r / nty;
    const int xo = bx * ST + lx, yo = by * ST + ly;
    if (xo >= Wo || yo >= Ho) continue;
    const float* q = prm + b * 6;
    const int ys = q[4] != 0.f ? Ho - 1 - yo : yo, xs = q[5] != 0.f ? Wo - 1 - xo : xo;      // MirrorTransform flips the output arrays
    const long o = (long)yo * Wo + xo;
    float* dq = dout + b * C * no + o;
    if (q[0] == 1.f && q[1] == 0.f && q[2] == 0.f && q[3] == 1.f) {
      // no rotation and no scale drawn: the centre crop with integer lower bounds (Hi - Ho) // 2, (Wi - Wo) // 2, nothing interpolated
      const int dy = Hi - Ho, dx = Wi - Wo;
      const int yi = ys + (dy >= 0 ? dy / 2 : -((1 - dy) / 2)), xi = xs + (dx >= 0 ? dx / 2 : -((1 - dx) / 2));
      const bool in = yi >= 0 && yi < Hi && xi >= 0 && xi < Wi;
      const long src = (long)yi * Wi + xi;
      for (int c = 0; c < C; c++) dq[c * no] = in ? din[(b * C + c) * ni + src] : 0.f;
      if (sin_) sout[b * no + o] = in ? sin_[b * ni + src] : 0.f;
      continue;
    }
    // numpy's fp64 expression m0 * cy + m1 * cx + centre with each product and sum rounded on its own: no FMA
    const double cy = (double)ys - 0.5 * (double)(Ho - 1), cx = (double)xs - 0.5 * (double)(Wo - 1);
    const double y = __dadd_rn(__dadd_rn(__dmul_rn((double)q[0], cy), __dmul_rn((double)q[1], cx)), (double)Hi / 2.0 - 0.5);
    const double x = __dadd_rn(__dadd_rn(__dmul_rn((double)q[2], cy), __dmul_rn((double)q[3], cx)), (double)Wi / 2.0 - 0.5);
    if (!(y >= 0.0 && y <= (double)(Hi - 1) && x >= 0.0 && x <= (double)(Wi - 1))) {        // mode "constant": exactly cval
      for (int c = 0; c < C; c++) dq[c * no] = 0.f;
      if (sin_) sout[b * no + o] = 0.f;
      continue;
    }
    const int y0 = (int)floor(y), x0 = (int)floor(x);
    const double fy = y - (double)y0, fx = x - (double)x0;
    double wy[4], wx[4];
    bspline_weights(fy, wy);
    bspline_weights(fx, wx);
    long iy[4];
    int ix[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      iy[k] = (long)mirror(y0 - 1 + k, Hi) * Wi;
      ix[k] = mirror(x0 - 1 + k, Wi);
    }
    for (int c = 0; c < C; c++) {
      const int sl = slot[b * C + c];
      if (sl < 0 || sl >= coef_planes) { dq[c * no] = 0.f; continue; }
      const double* cp = coef + (long)sl * ni;
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const double* row = cp + iy[k];
        acc += wy[k] * (wx[0] * row[ix[0]] + wx[1] * row[ix[1]] + wx[2] * row[ix[2]] + wx[3] * row[ix[3]]);
      }
      dq[c * no] = (float)acc;
    }
    if (sin_) {
      // order 1, every label (-1 included) on its own one-hot map: the largest label whose bilinear weight reaches 1/2, else 0.  A tap
      // beyond the last row / column has weight exactly 0 (the coordinate is the last index itself) and is read from the edge.
      const float* sp = sin_ + b * ni;
      const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
      const double w4[4] = {(1.0 - fy) * (1.0 - fx), (1.0 - fy) * fx, fy * (1.0 - fx), fy * fx};
      const float lab[4] = {sp[(long)y0 * Wi + x0], sp[(long)y0 * Wi + x1], sp[(long)y1 * Wi + x0], sp[(long)y1 * Wi + x1]};
      float best = 0.f;
      bool found = false;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        double sum = 0.0;
#pragma unroll
        for (int m = 0; m < 4; m++) sum += lab[m] == lab[k] ? w4[m] : 0.0;
        if (sum >= 0.5 && (!found || lab[k] > best)) { best = lab[k]; found = true; }
      }
      sout[b * no + o] = best;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- low resolution
constexpr int SPL_PAD = 12;                       // edge padding of scipy.ndimage.zoom(mode='nearest') for order 3
constexpr int SPL_TAB = 2 * (HZ + 3) + 1;

// nearest source pixel of low-grid sample i, ratio = n / nl: floor((i + 1/2) n / nl), evaluated as scipy's zoom(order=0, grid_mode=True)
// evaluates it -- floor(((i + 1/2) ratio - 1/2) + 1/2) in fp64, every operation rounded on its own (no FMA) -- because where
// (i + 1/2) n / nl is an integer (64 -> 49: i = 24) the rounding of the ratio decides between the two equally near pixels
__device__ __forceinline__ int nearest_src(int i, double ratio, int n) {
  const double cc = __dadd_rn(__dsub_rn(__dmul_rn((double)i + 0.5, ratio), 0.5), 0.5);
  return min(max((int)floor(cc), 0), n - 1);
}

constexpr int BPARTS = 32;                        // workgroups per plane of the min / max pass
// sizes (P, 2) = (Hl, Wl) <= (H, W), (0, 0) for a plane that is left alone; bounds[p][part] = (min, max) of the low grid's rows part,
// part + 32, ...: the up-sampling pass takes the min / max over the 32 parts
__global__ __launch_bounds__(256) void lowres_bounds_kernel(const float* __restrict__ x, const int* __restrict__ sizes, float* __restrict__ bounds,
                                                            int H, int W) {
  __shared__ float red[2][4];
  const int p = blockIdx.y, Hl = min(sizes[p * 2], H), Wl = min(sizes[p * 2 + 1], W);
  if (Hl <= 0 || Wl <= 0) return;
  const float* q = x + (long)p * H * W;
  float mn = 3.4e38f, mx = -3.4e38f;                            // a part without rows keeps these: neutral in the final min / max
  const double ry = __ddiv_rn((double)H, (double)Hl), rx = __ddiv_rn((double)W, (double)Wl);
  for (int yl = blockIdx.x; yl < Hl; yl += BPARTS) {
    const float* line = q + (long)nearest_src(yl, ry, H) * W;
    for (int xl = threadIdx.x; xl < Wl; xl += 256) {
      const float v = line[nearest_src(xl, rx, W)];
      mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = bounds + ((long)p * BPARTS + blockIdx.x) * 2;
    o[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    o[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__device__ __forceinline__ void fill_tab(double* tab) {          // tab[35 + d] = sqrt(3) z^|d| for |d| <= 32, else 0
  if (threadIdx.x < SPL_TAB) {
    const int d = (int)threadIdx.x - (HZ + 3), ad = d < 0 ? -d : d;
    double v = 0.0;
    if (ad <= HZ) {
      v = SQRT3;
      for (int k = 0; k < ad; k++) v *= POLE;
    }
    tab[threadIdx.x] = v;
  }
  __syncthreads();
}

// output sample o of a line of n_in samples (sample(m), 0 <= m < n_in) resampled to n_out: spline_axis_kernel's arithmetic (12 edge samples
// of padding, mirror prefilter over the padded line, four taps at the unclamped coordinate (o + 1/2) n_in / n_out - 1/2 from integers)
template <typename F>
__device__ __forceinline__ double resample_at(F sample, const double* tab, int n_in, int n_out, int o) {
  const int npad = n_in + 2 * SPL_PAD;
  const long num = (2l * o + 1) * n_in - n_out, den = 2l * n_out;
  long f = num / den;
  if (num - f * den < 0) f--;
  double w[4];
  bspline_weights((double)(num - f * den) / (double)den, w);
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  const int base = (int)f + SPL_PAD - 1;
#pragma unroll 4
  for (int k = -HZ; k <= HZ + 3; k++) {
    int m = base + k;
    m = m < 0 ? -m : m;
    m = m >= npad ? 2 * npad - 2 - m : m;
    m -= SPL_PAD;
    m = m < 0 ? 0 : (m > n_in - 1 ? n_in - 1 : m);
    const double v = sample(m);
    const double* h = tab + (k + HZ + 3);
    c0 += h[0] * v; c1 += h[-1] * v; c2 += h[-2] * v; c3 += h[-3] * v;
  }
  return w[0] * c0 + w[1] * c1 + w[2] * c2 + w[3] * c3;
}

// tmp[p] rows 0 .. Hl - 1, W samples each (row stride W) = the low grid's rows resampled along x
__global__ __launch_bounds__(256) void lowres_x_kernel(const float* __restrict__ x, const int* __restrict__ sizes, double* __restrict__ tmp, int H, int W) {
  __shared__ double tab[SPL_TAB];
  fill_tab(tab);
  const int p = blockIdx.y, Hl = min(sizes[p * 2], H), Wl = min(sizes[p * 2 + 1], W);
  if (Hl <= 0 || Wl <= 0) return;
  const float* q = x + (long)p * H * W;
  double* t = tmp + (long)p * H * W;
  const double ry = __ddiv_rn((double)H, (double)Hl), rx = __ddiv_rn((double)W, (double)Wl);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)Hl * W; i += (long)gridDim.x * 256) {
    const int yl = (int)(i / W), xo = (int)(i % W);
    const float* line = q + (long)nearest_src(yl, ry, H) * W;
    t[i] = Wl == W ? (double)line[xo] : resample_at([&](int m) { return (double)line[nearest_src(m, rx, W)]; }, tab, Wl, W, xo);
  }
}

// y[p] = tmp[p] resampled along y, clipped to the low grid's range, rounded once; a plane that is left alone is copied
__global__ __launch_bounds__(256) void lowres_y_kernel(const float* __restrict__ x, const int* __restrict__ sizes, const float* __restrict__ bounds,
                                                       const double* __restrict__ tmp, float* __restrict__ y, int H, int W) {
  __shared__ double tab[SPL_TAB];
  fill_tab(tab);
  const int p = blockIdx.y, Hl = sizes[p * 2 + 1] > 0 ? min(sizes[p * 2], H) : 0;
  const long n = (long)H * W;
  const float* q = x + (long)p * n;
  const double* t = tmp + (long)p * n;
  float* out = y + (long)p * n;
  float fmn = 3.4e38f, fmx = -3.4e38f;
  if (Hl > 0)
    for (int k = 0; k < BPARTS; k++) {
      fmn = fminf(fmn, bounds[((long)p * BPARTS + k) * 2]);
      fmx = fmaxf(fmx, bounds[((long)p * BPARTS + k) * 2 + 1]);
    }
  const double lo = (double)fmn, hi = (double)fmx;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    if (Hl <= 0) { out[i] = q[i]; continue; }
    const int yo = (int)(i / W), xo = (int)(i % W);
    double v = Hl == H ? t[i] : resample_at([&](int m) { return t[(long)m * W + xo]; }, tab, Hl, H, yo);
    v = v < lo ? lo : (v > hi ? hi : v);
    out[i] = (float)v;
  }
}

// ------------------------------------------------------------------------------------------------------------- mask
__global__ __launch_bounds__(256) void mask_kernel(float* __restrict__ data, float* __restrict__ labels, unsigned long long bits, int C, long n,
                                                   long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    if (!(labels[i] < 0.f)) continue;
    const long b = i / n, o = i - b * n;
    for (int c = 0; c < C && c < 63; c++)
      if ((bits >> c) & 1ull) data[(b * C + c) * n + o] = 0.f;
    labels[i] = 0.f;
  }
}

inline unsigned grid_cap(long items, long cap) { return (unsigned)(items < cap ? items : cap); }
constexpr int64_t PLANE_LIMIT = (int64_t)1 << 31;

}  // namespace

extern "C" int64_t du_aug_spline_ws_elems(int planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0) return DU_ERR_BAD_ARG;
  if ((int64_t)H * W >= PLANE_LIMIT) return DU_ERR_UNSUPPORTED;
  return 2 * (int64_t)planes * H * W;
}

extern "C" int du_aug_spline_coeffs(const float* x, int in_planes, const int32_t* plane_idx, int planes, int H, int W, double* ws, int64_t ws_elems,
                                    void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!x || !plane_idx || !ws || in_planes <= 0 || planes <= 0 || H <= 0 || W <= 0) return DU_ERR_BAD_ARG;
  if ((int64_t)H * W >= PLANE_LIMIT) return DU_ERR_UNSUPPORTED;
  if (ws_elems < du_aug_spline_ws_elems(planes, H, W)) return DU_ERR_BAD_ARG;
  double* rows = ws + (long)planes * H * W;                     // second half: the row pass's result
  const int nseg = (W + SEG - 1) / SEG;
  const long ritems = (long)planes * H * nseg;
  hipLaunchKernelGGL(coef_rows_kernel, dim3(grid_cap(ritems, 1 << 16)), dim3(256), 0, st, x, plane_idx, rows, in_planes, H, W, nseg, ritems);
  const int ntx = (W + CX - 1) / CX, nty = (H + CY - 1) / CY;
  const long citems = (long)planes * ntx * nty;
  hipLaunchKernelGGL(coef_cols_kernel, dim3(grid_cap(citems, 1 << 16)), dim3(256), 0, st, (const double*)rows, ws, H, W, ntx, nty, citems);
  return du_check_launch();
}

extern "C" int du_aug_spatial_spline(const float* data, const float* seg, const float* params, const double* coef, int coef_planes,
                                     const int32_t* slots, float* data_out, float* seg_out, int B, int C, int Hi, int Wi, int Ho, int Wo, void* stream) {
  if (!data || !params || !coef || coef_planes < 0 || !slots || !data_out || (seg && !seg_out) || B <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0)
    return DU_ERR_BAD_ARG;
  if ((int64_t)Hi * Wi >= PLANE_LIMIT || (int64_t)Ho * Wo >= PLANE_LIMIT) return DU_ERR_UNSUPPORTED;
  const int ntx = (Wo + ST - 1) / ST, nty = (Ho + ST - 1) / ST;
  const long items = (long)B * ntx * nty;
  hipLaunchKernelGGL(spatial_spline_kernel, dim3(grid_cap(items, 1 << 16)), dim3(256), 0, (hipStream_t)stream, data, seg, params, coef, slots,
                     data_out, seg_out, coef_planes, C, Hi, Wi, Ho, Wo, ntx, nty, items);
  return du_check_launch();
}

extern "C" int du_aug_lowres_spline(const float* x, float* y, const int32_t* sizes, float* bounds, double* tmp, int planes, int H, int W,
                                    void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!x || !y || x == y || !sizes || !bounds || !tmp || planes <= 0 || H <= 0 || W <= 0) return DU_ERR_BAD_ARG;
  if ((int64_t)H * W >= PLANE_LIMIT || planes > 65535) return DU_ERR_UNSUPPORTED;
  const long n = (long)H * W;
  const dim3 grid(grid_cap((n + 255) / 256, 1024), (unsigned)planes);
  hipLaunchKernelGGL(lowres_bounds_kernel, dim3(BPARTS, (unsigned)planes), dim3(256), 0, st, x, sizes, bounds, H, W);
  hipLaunchKernelGGL(lowres_x_kernel, grid, dim3(256), 0, st, x, sizes, tmp, H, W);
  hipLaunchKernelGGL(lowres_y_kernel, grid, dim3(256), 0, st, x, sizes, (const float*)bounds, (const double*)tmp, y, H, W);
  return du_check_launch();
}

extern "C" int du_aug_mask(float* data, float* labels, int64_t channel_bits, int B, int C, int64_t n, void* stream) {
  if (!data || !labels || B <= 0 || C <= 0 || n <= 0 || channel_bits < 0 || (C < 63 && (channel_bits >> C) != 0)) return DU_ERR_BAD_ARG;
  if (n >= PLANE_LIMIT) return DU_ERR_UNSUPPORTED;
  const long total = (long)B * n;
  hipLaunchKernelGGL(mask_kernel, dim3(grid_cap((total + 255) / 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, data, labels,
                     (unsigned long long)channel_bits, C, (long)n, total);
  return du_check_launch();
}
