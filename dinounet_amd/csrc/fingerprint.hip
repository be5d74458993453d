// Dataset fingerprint on the device: what DatasetFingerprintExtractor.collect_foreground_intensities and .run
// (dinounet/experiment_planning/dataset_fingerprint/fingerprint_extractor.py:42-80, :156-177) compute from the foreground voxels of a case,
// and from the concatenated samples of a dataset, without ever listing those voxels.
//   member(v)  = seg[v] > 0; every element without seg (the dataset-level form over the concatenated samples)
//   key(x)     = the fp32 bits with all bits flipped for a negative, the sign bit set for the rest: unsigned order = numeric order,
//                -0.0 directly below +0.0
// moments      one workgroup per stretch of a channel: per lane a sequential fp64 sum, lanes by the xor tree, the four waves in order; one
//              wave per channel then adds the stretches in lane order, again by the xor tree: a fixed order, no atomics.  A second mode
//              sums (x - sum / count)^2 the same way.
// order stats  radix select, 8 bits a pass from the top: a sweep over img and seg counts, for every distinct prefix among the R targets of the
//              channel, the members whose higher key bits equal that prefix by their next 8 bits; a one-workgroup kernel per channel scans
//              the 256 counts, picks the bin that holds the rank, extends the prefix, reduces the rank and groups the targets whose new
//              prefixes agree (they share one histogram in the next sweep).  Four sweeps, nothing read back between them.
//              The sweep's counters live in LDS as [prefix][bin][4 copies], the copy chosen by lane & 3, so equal keys in neighbouring
//              lanes land in different banks; before that the lanes of a wave that share the first matching lane's bin are counted by one
//              ballot and added once (CT foregrounds and every top-byte pass put most of a wave in one bin).  Flush: one integer atomicAdd
//              per non-empty bin per workgroup.
// sample       the counts / exclusive prefix / select-by-ballot scheme of dataload.hip with the predicate seg > 0 (its masks cover the
//              labels 0..63 only), the select fused with the gather of the member's value from every channel's own rank list.  The chunk
//              is found 64 ways a round (three rounds for 2^15 chunks, not fifteen dependent loads) and loaded in one go.
//              Streaming loads are unconditional at a clamped index throughout, so a lane has 8 to 16 of them in flight.
// Integer atomics only; nothing depends on the schedule, so results are identical from run to run.  No kernel waits for another
// workgroup.  No scratch.
#include "common.h"

namespace {

constexpr int CHUNK = 1024, STEPS = CHUNK / 64;                           // sample: voxels per member count
constexpr int MOM_CHUNK = 16384, MOM_MAX_BLOCKS = 2048;                   // moments: the shortest stretch, the most stretches of a channel
constexpr int MOM_STEPS = 8;                                              // loads a lane has in flight
constexpr int RMAX = 8, BINS = 256, COPIES = 4;
constexpr int TILE_STEPS = 8, TILE = 256 * TILE_STEPS;                    // order stats: elements a workgroup takes per round
constexpr int HIST_MAX_BLOCKS = 1024;
// select state of a channel, int32 words: the targets' prefix, remaining rank, bad flag and histogram slot, then the distinct prefixes
constexpr int ST_PREFIX = 0, ST_REM = 8, ST_BAD = 16, ST_SLOT = 24, ST_NLEAD = 32, ST_LEAD = 40, STATE = 64;
constexpr int MOM = 6;                                                    // doubles of a stats row

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned b = __builtin_bit_cast(unsigned, v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __shfl_xor((int)(b & 0xffffffffll), o, 64), hi = __shfl_xor((int)(b >> 32), o, 64);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

// ---------------------------------------------------------------------------------------------------------------- moments
// partial (C, nblk, 5) fp64 = {count, min, max, sum, NaN count} of a stretch; SQ: sum = the squared deviations from sum / count of the channel
// Loads are unconditional at a clamped index (a conditional load waits for the one before it): MOM_STEPS of them are issued back to back.
template <bool SQ, bool SEG>
__global__ __launch_bounds__(256) void mom_partial_kernel(const float* __restrict__ img, const int16_t* __restrict__ seg,
                                                          const double* __restrict__ stats, double* __restrict__ partial, long n, long len,
                                                          int nblk) {
  const int c = blockIdx.y, k = blockIdx.x;
  const float* x = img + (long)c * n;
  const long a = (long)k * len, b = a + len < n ? a + len : n;
  double mean = 0.0;
  if (SQ) { const double cnt = stats[c * MOM]; mean = cnt > 0.0 ? stats[c * MOM + 3] / cnt : 0.0; }
  float mn = INFINITY, mx = -INFINITY;
  double sum = 0.0;
  int cnt = 0, nan = 0;
  for (long i0 = a + threadIdx.x; i0 < b; i0 += 256 * MOM_STEPS) {            // a < b: every stretch has an element
    float v[MOM_STEPS];
    bool in[MOM_STEPS];
#pragma unroll
    for (int u = 0; u < MOM_STEPS; u++) {
      const long i = i0 + u * 256;
      const bool ok = i < b;
      const long ic = ok ? i : b - 1;
      v[u] = x[ic];
      const int l = SEG ? (int)seg[ic] : 1;
      in[u] = ok & (l > 0);
    }
#pragma unroll
    for (int u = 0; u < MOM_STEPS; u++) {                                   // the lane's elements in ascending order, as a plain loop would
      if (in[u]) {
        if (SQ) {
          const double dv = (double)v[u] - mean;
          sum += dv * dv;
        } else {
          mn = fminf(mn, v[u]); mx = fmaxf(mx, v[u]);
          sum += (double)v[u];
          cnt++;
          nan += v[u] != v[u];
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    sum += shfl_xor_f64(sum, o);
    cnt += __shfl_xor(cnt, o, 64); nan += __shfl_xor(nan, o, 64);
  }
  __shared__ double sh[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[wave][0] = cnt; sh[wave][1] = mn; sh[wave][2] = mx; sh[wave][3] = sum; sh[wave][4] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = sh[0][0], r1 = sh[0][1], r2 = sh[0][2], r3 = sh[0][3], r4 = sh[0][4];
    for (int q = 1; q < 4; q++) { r0 += sh[q][0]; r1 = fmin(r1, sh[q][1]); r2 = fmax(r2, sh[q][2]); r3 += sh[q][3]; r4 += sh[q][4]; }
    double* o = partial + ((long)c * nblk + k) * 5;
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
  }
}

// one workgroup of one wave per channel: the stretches in lane order, lanes by the xor tree: a fixed order
template <bool SQ>
__global__ __launch_bounds__(64) void mom_final_kernel(const double* __restrict__ partial, double* __restrict__ stats, int nblk) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double cnt = 0.0, mn = INFINITY, mx = -INFINITY, sum = 0.0, nan = 0.0;
  for (int k = lane; k < nblk; k += 64) {
    const double* q = partial + ((long)c * nblk + k) * 5;
    cnt += q[0]; mn = fmin(mn, q[1]); mx = fmax(mx, q[2]); sum += q[3]; nan += q[4];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += shfl_xor_f64(cnt, o); mn = fmin(mn, shfl_xor_f64(mn, o)); mx = fmax(mx, shfl_xor_f64(mx, o));
    sum += shfl_xor_f64(sum, o); nan += shfl_xor_f64(nan, o);
  }
  if (lane == 0) {
    double* o = stats + c * MOM;
    if (SQ) { o[5] = sum; }
    else { o[0] = cnt; o[1] = mn; o[2] = mx; o[3] = sum; o[4] = nan; o[5] = 0.0; }
  }
}

// ---------------------------------------------------------------------------------------------------------------- order statistics
__global__ __launch_bounds__(256) void os_init_kernel(const long long* __restrict__ ranks, int R, long n, unsigned* __restrict__ state,
                                                      unsigned* __restrict__ hist) {
  const int c = blockIdx.x, t = threadIdx.x;
  unsigned* st = state + c * STATE;
  unsigned* hc = hist + (long)c * RMAX * BINS;
  for (int i = t; i < RMAX * BINS; i += 256) hc[i] = 0u;
  if (t < STATE) {
    unsigned v = 0u;
    const int w = t & 7;
    if (t >= ST_REM && t < ST_REM + RMAX && w < R) v = (unsigned)ranks[(long)c * R + w];
    if (t >= ST_BAD && t < ST_BAD + RMAX) { v = 1u; if (w < R) { const long long r = ranks[(long)c * R + w]; v = (r < 0 || r >= n) ? 1u : 0u; } }
    if (t == ST_NLEAD) v = 1u;                                            // one prefix, the empty one, shared by every target
    st[t] = v;
  }
}

// called by the lanes whose element matches a prefix, i = slot * BINS + bin: the lanes that share the first such lane's counter add once,
// the rest one by one
__device__ __forceinline__ void add_bin(unsigned* h, int i, int lane) {
  const int first = __builtin_amdgcn_readfirstlane(i);
  if (i == first) {
    const unsigned long long b = __ballot(1);
    if (lane == __ffsll((long long)b) - 1) atomicAdd(&h[first * COPIES + (lane & (COPIES - 1))], (unsigned)__popcll(b));
  } else {
    atomicAdd(&h[i * COPIES + (lane & (COPIES - 1))], 1u);
  }
}

template <bool SEG>
__global__ __launch_bounds__(256) void os_hist_kernel(const float* __restrict__ img, const int16_t* __restrict__ seg, long n,
                                                      const unsigned* __restrict__ state, unsigned* __restrict__ hist, int shift, int ntiles) {
  __shared__ unsigned h[RMAX * BINS * COPIES];                            // 32 KiB
  const int c = blockIdx.y, lane = threadIdx.x & 63;
  const unsigned* st = state + c * STATE;
  const int nlead = (int)st[ST_NLEAD];                                    // uniform: 1..RMAX
  unsigned lp[RMAX];
#pragma unroll
  for (int j = 0; j < RMAX; j++) lp[j] = st[ST_LEAD + j];
  for (int i = threadIdx.x; i < nlead * BINS * COPIES; i += 256) h[i] = 0u;
  __syncthreads();
  const float* x = img + (long)c * n;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long base = (long)t * TILE + threadIdx.x;
    float v[TILE_STEPS];
    bool in[TILE_STEPS];
#pragma unroll
    for (int u = 0; u < TILE_STEPS; u++) {
      const long i = base + u * 256;
      const bool ok = i < n;
      const long ic = ok ? i : n - 1;                                      // unconditional loads at a clamped index: all in flight at once
      v[u] = x[ic];
      const int l = SEG ? (int)seg[ic] : 1;
      in[u] = ok & (l > 0);
    }
#pragma unroll
    for (int u = 0; u < TILE_STEPS; u++) {
      if (in[u]) {
        const unsigned key = key_of(v[u]);
        const unsigned hi = shift == 24 ? 0u : key >> (shift + 8);
        const int d = (int)((key >> shift) & 255u);
        int j = RMAX;                                                     // the prefixes are distinct: at most one slot below nlead matches
#pragma unroll
        for (int t = RMAX - 1; t >= 0; t--) j = hi == lp[t] ? t : j;      // selects, no branches; the lowest slot wins over stale ones
        if (j < nlead) add_bin(h, j * BINS + d, lane);
      }
    }
  }
  __syncthreads();
  unsigned* hc = hist + (long)c * RMAX * BINS;
  for (int i = threadIdx.x; i < nlead * BINS; i += 256) {
    const unsigned s = h[i * COPIES] + h[i * COPIES + 1] + h[i * COPIES + 2] + h[i * COPIES + 3];
    if (s) atomicAdd(&hc[i], s);
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

// one workgroup per channel, thread = bin: per target the bin with prefix sum <= rank < prefix sum + count
__global__ __launch_bounds__(256) void os_pick_kernel(unsigned* __restrict__ state, unsigned* __restrict__ hist, int R, int last,
                                                      float* __restrict__ out) {
  __shared__ int red[4];
  __shared__ unsigned np[RMAX], nr[RMAX], nb[RMAX], lead[RMAX];
  const int c = blockIdx.x, tid = threadIdx.x;
  unsigned* st = state + c * STATE;
  unsigned* hc = hist + (long)c * RMAX * BINS;
  if (tid < RMAX) { np[tid] = st[ST_PREFIX + tid]; nr[tid] = st[ST_REM + tid]; nb[tid] = 1u; }          // bad until a bin takes the rank
  for (int t = 0; t < R; t++) {                                           // uniform trip count: the barriers inside are reached by all
    const int j = (int)st[ST_SLOT + t];
    const int cnt = (int)hc[j * BINS + tid];                              // <= n < 2^31
    int total;
    const int inc = block_scan(cnt, red, &total);
    const unsigned r = st[ST_REM + t], exc = (unsigned)(inc - cnt);
    if (cnt > 0 && exc <= r && r < (unsigned)inc) {                       // at most one thread
      np[t] = (st[ST_PREFIX + t] << 8) | (unsigned)tid;
      nr[t] = r - exc;
      nb[t] = st[ST_BAD + t];
    }
  }
  __syncthreads();                                                        // every read of the state and of the histograms is over
  for (int i = tid; i < RMAX * BINS; i += 256) hc[i] = 0u;
  if (tid == 0) {
    int nl = 0;
    for (int t = 0; t < R; t++) {
      st[ST_PREFIX + t] = np[t]; st[ST_REM + t] = nr[t]; st[ST_BAD + t] = nb[t];
      int j = 0;
      while (j < nl && lead[j] != np[t]) j++;
      if (j == nl) { lead[nl] = np[t]; st[ST_LEAD + nl] = np[t]; nl++; }
      st[ST_SLOT + t] = (unsigned)j;
      if (last) out[(long)c * R + t] = nb[t] ? __builtin_nanf("") : value_of(np[t]);
    }
    st[ST_NLEAD] = (unsigned)nl;
  }
}

// ---------------------------------------------------------------------------------------------------------------- sample
__global__ __launch_bounds__(256) void sm_count_kernel(const int16_t* __restrict__ seg, int* __restrict__ counts, int n, int nchunks) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);                  // uniform in the wave
  if (chunk >= nchunks) return;
  const int base = chunk * CHUNK;                                         // < n < 2^31
  int c = 0;
#pragma unroll
  for (int s = 0; s < STEPS; s++) {
    const int off = s * 64 + lane;
    const int l = off < n - base ? (int)seg[base + off] : 0;              // past the end: no member
    c += __popcll(__ballot(l > 0));
  }
  if (lane == 0) counts[chunk] = c;
}

// one workgroup; a thread takes SCAN_RUN consecutive counts a round, the workgroup scans the 256 run sums
constexpr int SCAN_RUN = 16;
__global__ __launch_bounds__(256) void sm_scan_kernel(int* __restrict__ counts, long long* __restrict__ total, int nchunks) {
  __shared__ int red[4];
  int carry = 0;                                                          // < n < 2^31
  for (int c0 = 0; c0 < nchunks; c0 += 256 * SCAN_RUN) {                  // uniform trip count: the barriers inside are reached by all
    const int first = c0 + (int)threadIdx.x * SCAN_RUN;
    int v[SCAN_RUN], run = 0;
#pragma unroll
    for (int k = 0; k < SCAN_RUN; k++) {
      v[k] = first + k < nchunks ? counts[first + k] : 0;
      run += v[k];
    }
    int tot;
    int at = carry + block_scan(run, red, &tot) - run;                    // the exclusive prefix of this thread's first count
#pragma unroll
    for (int k = 0; k < SCAN_RUN; k++) {
      if (first + k < nchunks) counts[first + k] = at;
      at += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// one wave per (channel, j): the member of rank ranks[c][j], its value in channel c
__global__ __launch_bounds__(256) void sm_select_kernel(const float* __restrict__ img, const int16_t* __restrict__ seg,
                                                        const int* __restrict__ prefix, const long long* __restrict__ total,
                                                        const long long* __restrict__ ranks, long m, long cm, float* __restrict__ out, int n,
                                                        int nchunks) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long members = *total;
  for (long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6); q < cm; q += (long)gridDim.x * 4) {      // q is uniform in the wave
    const long long r = ranks[q];
    int found = -1;
    if (r >= 0 && r < members) {
      // the largest chunk with prefix <= r, 64 ways a round: lane l looks at lo + l stride, the prefix is non-decreasing and
      // prefix[lo] <= r holds throughout (prefix[0] = 0), so the lanes that say yes are a run from lane 0
      int lo = 0, len = nchunks;
      while (len > 1) {                                                   // lo and len are uniform
        const int stride = (len + 63) / 64;
        const int idx = lo + lane * stride;
        const bool le = idx < lo + len && (long long)prefix[idx] <= r;
        const int k = __popcll(__ballot(le)) - 1;
        const int end = lo + len;
        lo += k * stride;
        len = end - lo < stride ? end - lo : stride;
      }
      int rem = (int)(r - prefix[lo]);
      const int base = lo * CHUNK;
      int lab[STEPS];
#pragma unroll
      for (int s = 0; s < STEPS; s++) {                                   // the whole chunk at once: unconditional loads at a clamped index
        const int off = s * 64 + lane;
        const int l = seg[base + (off < n - base ? off : n - base - 1)];
        lab[s] = off < n - base ? l : 0;
      }
      bool open = true;                                                   // uniform
#pragma unroll
      for (int s = 0; s < STEPS; s++) {
        const bool in = lab[s] > 0;
        const unsigned long long b = __ballot(in);
        const int cnt = __popcll(b);
        if (open && rem < cnt) {
          if (in && __popcll(b & below) == rem) found = base + s * 64 + lane;          // exactly one lane
          open = false;
        }
        if (open) rem -= cnt;
      }
    }
    const unsigned long long hit = __ballot(found >= 0);
    if (hit) {
      if (found >= 0) out[q] = img[(q / m) * (long)n + found];
    } else if (lane == 0) {
      out[q] = __builtin_nanf("");                                        // a rank outside [0, members): no voxel
    }
  }
}

// without seg every element is a member: the rank is the index
__global__ __launch_bounds__(256) void sm_gather_kernel(const float* __restrict__ img, const long long* __restrict__ ranks, long m, long cm,
                                                        float* __restrict__ out, long n) {
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < cm; q += (long)gridDim.x * 256) {
    const long long r = ranks[q];
    out[q] = (r >= 0 && r < n) ? img[(q / m) * n + r] : __builtin_nanf("");
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
// 0, or the error of the shape
int shape_error(int C, int64_t n) {
  if (C < 1 || n < 1) return DU_ERR_BAD_ARG;
  if (n >= ((int64_t)1 << 31) || C > 65535) return DU_ERR_UNSUPPORTED;    // channels are grid.y
  return DU_OK;
}
struct MomPlan {
  int nblk;
  long len;
};
MomPlan mom_plan(int64_t n) {
  MomPlan p;
  int64_t nb = cdiv64(n, MOM_CHUNK);
  if (nb > MOM_MAX_BLOCKS) nb = MOM_MAX_BLOCKS;
  p.len = (long)cdiv64(n, nb);
  p.nblk = (int)cdiv64(n, p.len);
  return p;
}
int64_t chunks_of(int64_t n) { return (n + CHUNK - 1) / CHUNK; }
int64_t mom_words(int C, int64_t n) { return 2 * (int64_t)C * mom_plan(n).nblk * 5; }
int64_t os_words(int C) { return (int64_t)C * (STATE + RMAX * BINS); }
int64_t sm_words(int64_t n) { return 4 + chunks_of(n); }
int64_t ws_need(int C, int64_t n) {
  int64_t w = mom_words(C, n);
  if (os_words(C) > w) w = os_words(C);
  if (sm_words(n) > w) w = sm_words(n);
  return (w + 3) & ~(int64_t)3;
}
bool bad_inputs(const float* img, const int16_t* seg, const int32_t* ws) {
  return !img || !ws || ((uintptr_t)img & 3) || ((uintptr_t)seg & 1) || ((uintptr_t)ws & 15);
}

}  // namespace

extern "C" int64_t du_fp_ws_elems(int C, int64_t n) {
  const int e = shape_error(C, n);
  if (e != DU_OK) return e;                                               // negative: the DU_ERR_* code of the shape
  return ws_need(C, n);
}

extern "C" int du_fp_moments(const float* img, const int16_t* seg, int C, int64_t n, int mode, double* stats, int32_t* ws, int64_t ws_elems,
                             void* stream) {
  if (bad_inputs(img, seg, ws) || !stats || ((uintptr_t)stats & 7) || (mode != 0 && mode != 1)) return DU_ERR_BAD_ARG;
  const int e = shape_error(C, n);
  if (e != DU_OK) return e;
  if (ws_elems < ws_need(C, n)) return DU_ERR_BAD_ARG;
  const MomPlan p = mom_plan(n);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)ws;
  auto partial_kernel = mode == 0 ? (seg ? mom_partial_kernel<false, true> : mom_partial_kernel<false, false>)
                                  : (seg ? mom_partial_kernel<true, true> : mom_partial_kernel<true, false>);
  hipLaunchKernelGGL(partial_kernel, dim3(p.nblk, C), dim3(256), 0, st, img, seg, (const double*)stats, partial, (long)n, p.len, p.nblk);
  if (mode == 0) hipLaunchKernelGGL(mom_final_kernel<false>, dim3(C), dim3(64), 0, st, (const double*)partial, stats, p.nblk);
  else hipLaunchKernelGGL(mom_final_kernel<true>, dim3(C), dim3(64), 0, st, (const double*)partial, stats, p.nblk);
  return du_check_launch();
}

extern "C" int du_fp_order_stats(const float* img, const int16_t* seg, int C, int64_t n, const int64_t* ranks, int R, float* out, int32_t* ws,
                                 int64_t ws_elems, void* stream) {
  if (bad_inputs(img, seg, ws) || !ranks || !out || ((uintptr_t)ranks & 7) || ((uintptr_t)out & 3) || R < 1 || R > RMAX) return DU_ERR_BAD_ARG;
  const int e = shape_error(C, n);
  if (e != DU_OK) return e;
  if (ws_elems < ws_need(C, n)) return DU_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned* state = (unsigned*)ws;
  unsigned* hist = state + (int64_t)C * STATE;
  const int ntiles = (int)cdiv64(n, TILE);
  const int gx = ntiles < HIST_MAX_BLOCKS ? ntiles : HIST_MAX_BLOCKS;
  hipLaunchKernelGGL(os_init_kernel, dim3(C), dim3(256), 0, st, (const long long*)ranks, R, (long)n, state, hist);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(seg ? os_hist_kernel<true> : os_hist_kernel<false>, dim3(gx, C), dim3(256), 0, st, img, seg, (long)n,
                       (const unsigned*)state, hist, shift, ntiles);
    hipLaunchKernelGGL(os_pick_kernel, dim3(C), dim3(256), 0, st, state, hist, R, shift == 0 ? 1 : 0, out);
  }
  return du_check_launch();
}

extern "C" int du_fp_sample(const float* img, const int16_t* seg, int C, int64_t n, const int64_t* ranks, int64_t m, float* out, int32_t* ws,
                            int64_t ws_elems, void* stream) {
  if (bad_inputs(img, seg, ws) || !ranks || !out || ((uintptr_t)ranks & 7) || ((uintptr_t)out & 3) || m < 1) return DU_ERR_BAD_ARG;
  const int e = shape_error(C, n);
  if (e != DU_OK) return e;
  if (m >= ((int64_t)1 << 40)) return DU_ERR_UNSUPPORTED;
  if (ws_elems < ws_need(C, n)) return DU_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t cm = (int64_t)C * m;
  if (!seg) {
    int64_t grid = (cm + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(sm_gather_kernel, dim3((unsigned)grid), dim3(256), 0, st, img, (const long long*)ranks, (long)m, (long)cm, out, (long)n);
    return du_check_launch();
  }
  const int nchunks = (int)chunks_of(n);
  long long* total = (long long*)ws;
  int* prefix = (int*)ws + 4;
  hipLaunchKernelGGL(sm_count_kernel, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, st, seg, prefix, (int)n, nchunks);
  hipLaunchKernelGGL(sm_scan_kernel, dim3(1), dim3(256), 0, st, prefix, total, nchunks);
  int64_t grid = (cm + 3) / 4;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(sm_select_kernel, dim3((unsigned)grid), dim3(256), 0, st, img, seg, (const int*)prefix, (const long long*)total,
                     (const long long*)ranks, (long)m, (long)cm, out, (int)n, nchunks);
  return du_check_launch();
}
