// Training batches on the device: the class-location tables of a preprocessed case (DefaultPreprocessor._sample_foreground_locations,
// dinounet/preprocessing/preprocessors/default_preprocessor.py:157-181) and the batch gather of nnUNetDataLoader2D.generate_train_batch
// (dinounet/training/dataloading/data_loader_2d.py:46-85).
//   member(v, mask) = 0 <= seg[v] <= 63 and bit seg[v] of mask (the du_labels_to_regions convention; any other label is in no mask)
//   raster order    v = (z H + y) W + x: the order np.argwhere lists the members in
// counts   one wave per chunk of 1024 consecutive voxels: 16 coalesced steps of 64 int16, kept in registers; per mask the chunk's member
//          count is the sum of 16 popcounts of 64-bit ballots (the ballot lives in scalar registers, the count costs no vector work).
//          Every (mask, chunk) word is written by exactly one lane: no atomics.
// scan     one workgroup per mask turns the chunk counts into their exclusive prefix in place (256 chunks a round, shuffles inside a
//          wave, four wave totals through LDS, the carry in a register) and writes the mask's total.
// select   one wave per query r: binary search for the chunk with prefix <= r < prefix + count, then the chunk 64 voxels at a time:
//          ballot, popcount, and in the step that holds the member the lane whose prefix popcount equals the remainder writes
//          {0, z, y, x}.  No list of n entries exists anywhere; the queries come in any order.
// gather   grid.x = one (sample, plane) pair, plane C = the segmentation, so the job row is uniform in a workgroup; lanes run along x:
//          reads and writes are contiguous 4-byte (2-byte for the labels) accesses.  The window may lie anywhere: outside the image the
//          image planes read 0 and the segmentation -1.
// Integer work only; nothing depends on the schedule, so results are identical from run to run.  No scratch.
#include "common.h"

namespace {

constexpr int CHUNK = 1024, STEPS = CHUNK / 64;

__device__ __forceinline__ bool member(int label, unsigned long long bits) {
  return (unsigned)label < 64u && ((bits >> (unsigned)label) & 1ull);
}

__global__ __launch_bounds__(256) void dl_count_kernel(const int16_t* __restrict__ seg, const unsigned long long* __restrict__ masks, int G,
                                                       int* __restrict__ counts, int n, int nchunks) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);                  // uniform in the wave
  if (chunk >= nchunks) return;
  const int base = chunk * CHUNK;                                         // < n < 2^31
  int lab[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const int off = s * 64 + lane;
    lab[s] = off < n - base ? (int)seg[base + off] : -1;                  // past the end: in no mask
  }
  for (int g = 0; g < G; g++) {
    const unsigned long long bits = masks[g];
    int c = 0;
#pragma unroll
    for (int s = 0; s < STEPS; s++) c += __popcll(__ballot(member(lab[s], bits)));
    if (lane == 0) counts[(long)g * nchunks + chunk] = c;
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
  __syncthreads();                                                        // the previous round's reads of red are over
  if (lane == 63) red[w] = v;
  __syncthreads();
  const int a = red[0], b = red[1], c = red[2], d = red[3];
  *total = a + b + c + d;
  return v + (w > 0 ? a : 0) + (w > 1 ? b : 0) + (w > 2 ? c : 0);
}

__global__ __launch_bounds__(256) void dl_scan_kernel(int* __restrict__ counts, long long* __restrict__ totals, int nchunks) {
  __shared__ int red[4];
  int* row = counts + (long)blockIdx.x * nchunks;
  int carry = 0;                                                          // < n < 2^31
  for (int c0 = 0; c0 < nchunks; c0 += 256) {                             // uniform trip count: the barriers inside are reached by all
    const int c = c0 + (int)threadIdx.x;
    const int v = c < nchunks ? row[c] : 0;
    int total;
    const int inc = block_scan(v, red, &total);
    if (c < nchunks) row[c] = carry + inc - v;
    carry += total;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void dl_select_kernel(const int16_t* __restrict__ seg, const unsigned long long* __restrict__ masks, int g,
                                                        const int* __restrict__ prefix, const long long* __restrict__ ranks, long m,
                                                        int* __restrict__ out, int n, int nchunks, int H, int W) {
  const int lane = threadIdx.x & 63;
  const unsigned long long bits = masks[g];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6); q < m; q += (long)gridDim.x * 4) {     // q is uniform in the wave
    const long long r = ranks[q];
    int found = -1;
    if (r >= 0 && r < (long long)n) {
      int lo = 0, hi = nchunks - 1;                                       // the largest chunk with prefix <= r; prefix[0] = 0
      while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if ((long long)prefix[mid] <= r) lo = mid; else hi = mid - 1;
      }
      int rem = (int)(r - prefix[lo]);
      const int base = lo * CHUNK;
      for (int s = 0; s < STEPS; s++) {
        const int off = s * 64 + lane;
        const int l = off < n - base ? (int)seg[base + off] : -1;
        const bool in = member(l, bits);
        const unsigned long long b = __ballot(in);
        const int cnt = __popcll(b);
        if (rem < cnt) {
          if (in && __popcll(b & below) == rem) found = base + off;       // exactly one lane
          break;                                                          // rem and cnt are uniform: the whole wave leaves
        }
        rem -= cnt;
      }
    }
    const unsigned long long hit = __ballot(found >= 0);
    if (hit) {
      if (found >= 0) {
        const int x = found % W, t = found / W;
        int* o = out + q * 4;
        o[0] = 0; o[1] = t / H; o[2] = t % H; o[3] = x;
      }
    } else if (lane < 4) {
      out[q * 4 + lane] = lane == 0 ? 0 : -1;                             // a rank outside [0, total): no voxel
    }
  }
}

// jobs (B, 8) int64: {data pointer, seg pointer, D, H, W, slice, y0, x0}
__global__ __launch_bounds__(256) void dl_gather_kernel(const long long* __restrict__ jobs, int C, int ph, int pw, float* __restrict__ data_out,
                                                        void* __restrict__ seg_out, int seg_f32) {
  const int plane = blockIdx.x % (C + 1), b = blockIdx.x / (C + 1);
  const long long* job = jobs + (long)b * 8;
  const float* data = (const float*)(uintptr_t)job[0];
  const int16_t* seg = (const int16_t*)(uintptr_t)job[1];
  const long long D = job[2], H = job[3], W = job[4], z = job[5], y0 = job[6], x0 = job[7];
  const bool is_seg = plane == C;
  const bool live = z >= 0 && z < D && H > 0 && W > 0 && (is_seg ? seg != nullptr : data != nullptr);
  const long npix = (long)ph * pw;
  const long long src_plane = ((is_seg ? 0 : (long long)plane * D) + z) * H;          // rows in front of this slice
  float* dout = data_out + ((long)b * C + (is_seg ? 0 : plane)) * npix;               // not used for the segmentation plane
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < npix; i += (long)gridDim.y * 256) {
    const int xo = (int)(i % pw), yo = (int)(i / pw);
    const long long y = y0 + yo, x = x0 + xo;
    const bool in = live && y >= 0 && y < H && x >= 0 && x < W;
    const long long src = (src_plane + y) * W + x;
    if (!is_seg) {
      dout[i] = in ? data[src] : 0.f;
    } else {
      const int l = in ? (int)seg[src] : -1;
      if (seg_f32) ((float*)seg_out)[(long)b * npix + i] = (float)l;
      else ((int16_t*)seg_out)[(long)b * npix + i] = (int16_t)l;
    }
  }
}

// 0, or the error of the shape
int shape_error(int D, int H, int W, int G) {
  if (D < 1 || H < 1 || W < 1 || G < 1) return DU_ERR_BAD_ARG;
  const int64_t lim = (int64_t)1 << 31, dh = (int64_t)D * H;
  if (dh >= lim || dh * W >= lim) return DU_ERR_UNSUPPORTED;
  return DU_OK;
}
int64_t chunks_of(int64_t n) { return (n + CHUNK - 1) / CHUNK; }
int64_t ws_need(int64_t n, int G) { return (chunks_of(n) * G + 3) & ~(int64_t)3; }

}  // namespace

extern "C" int64_t du_dl_ws_elems(int D, int H, int W, int G) {
  const int e = shape_error(D, H, W, G);
  if (e != DU_OK) return e;                                               // negative: the DU_ERR_* code of the shape
  return ws_need((int64_t)D * H * W, G);
}

extern "C" int du_dl_class_counts(const int16_t* seg, const int64_t* masks, int G, int D, int H, int W, int32_t* ws, int64_t ws_elems,
                                  int64_t* totals, void* stream) {
  if (!seg || !masks || !ws || !totals || ((uintptr_t)ws & 15) || ((uintptr_t)seg & 1) || ((uintptr_t)masks & 7) || ((uintptr_t)totals & 7))
    return DU_ERR_BAD_ARG;
  const int e = shape_error(D, H, W, G);
  if (e != DU_OK) return e;
  const int64_t n = (int64_t)D * H * W;
  if (ws_elems < ws_need(n, G)) return DU_ERR_BAD_ARG;
  const int nchunks = (int)chunks_of(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dl_count_kernel, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, st, seg, (const unsigned long long*)masks, G, ws, (int)n,
                     nchunks);
  hipLaunchKernelGGL(dl_scan_kernel, dim3((unsigned)G), dim3(256), 0, st, ws, (long long*)totals, nchunks);
  return du_check_launch();
}

extern "C" int du_dl_select(const int16_t* seg, const int64_t* masks, int G, int g, int D, int H, int W, const int32_t* ws, int64_t ws_elems,
                            const int64_t* ranks, int64_t m, int32_t* out, void* stream) {
  if (!seg || !masks || !ws || !ranks || !out || ((uintptr_t)ws & 15) || ((uintptr_t)seg & 1) || ((uintptr_t)masks & 7) ||
      ((uintptr_t)ranks & 7) || ((uintptr_t)out & 3) || m < 1 || g < 0)
    return DU_ERR_BAD_ARG;
  const int e = shape_error(D, H, W, G);
  if (e != DU_OK) return e;
  if (g >= G) return DU_ERR_BAD_ARG;
  const int64_t n = (int64_t)D * H * W;
  if (ws_elems < ws_need(n, G)) return DU_ERR_BAD_ARG;
  if (m > n) return DU_ERR_BAD_ARG;                                       // more ranks than voxels: not ranks of distinct members
  const int nchunks = (int)chunks_of(n);
  int64_t grid = (m + 3) / 4;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(dl_select_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, seg, (const unsigned long long*)masks, g,
                     ws + (int64_t)g * nchunks, (const long long*)ranks, (long)m, out, (int)n, nchunks, H, W);
  return du_check_launch();
}

extern "C" int du_dl_gather(const int64_t* jobs, int B, int C, int ph, int pw, float* data_out, void* seg_out, int seg_f32, void* stream) {
  if (!jobs || !data_out || !seg_out || ((uintptr_t)jobs & 7) || ((uintptr_t)data_out & 3) || ((uintptr_t)seg_out & (seg_f32 ? 3 : 1)) ||
      B < 1 || C < 1 || ph < 1 || pw < 1)
    return DU_ERR_BAD_ARG;
  const int64_t planes = (int64_t)B * ((int64_t)C + 1);
  if (planes >= ((int64_t)1 << 31)) return DU_ERR_UNSUPPORTED;
  const int64_t npix = (int64_t)ph * pw;
  int64_t gy = (npix + 1023) / 1024;                                      // about four pixels a lane
  if (gy > 1024) gy = 1024;
  hipLaunchKernelGGL(dl_gather_kernel, dim3((unsigned)planes, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (const long long*)jobs, C, ph, pw,
                     data_out, seg_out, seg_f32 ? 1 : 0);
  return du_check_launch();
}
