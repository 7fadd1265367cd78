// fps.hip - farthest point sampling on a ragged batch: points fp32 [N, 3], cu int32 [B + 1] on the device, K samples per
// segment, idx int32 [B, K] of global rows (reference: csrc/farthest_point_sampling.cu, which enqueues 2 (K - 1) + 1 launches
// and re-reads coordinates and running distances from global memory in every step).
//
// The contract: sample 0 of segment b is row cu[b] + start[b]; sample k is the row with the largest running
// distance t[i] = min over the earlier samples s of d(i, s), of equal ones the lowest row; d = (dx dx + dy dy) + dz dz in
// fp32 with every operation rounded once (no FMA contraction); t starts at +inf and takes d where d < t; the selection starts
// from (-1, first row) and replaces on a larger t.  So t lies in [0, +inf] and is never a NaN, and a result is always a row of
// its segment.  An empty segment gets -1 in all its K entries.
//
// The order "larger t, then lower row" is ONE unsigned 64-bit comparison: key = (bits of t) << 32 | ~(local row).  The bits of
// a non-negative float ascend with its value, and key 0 (no row) loses to every row.  Every reduction below is a maximum of
// keys, so no result depends on which lane or workgroup held what.
//
//   resident tier   a segment of at most kFpsMaxP * kFpsThreads points: ONE workgroup keeps P points and their t per thread in
//                   registers (arrays indexed by compile-time constants only) and runs the whole K-loop in one launch.  A
//                   step: update the P distances and the thread's best (its coordinates ride along), maximum across the wave,
//                   the owning lane of each wave publishes key + coordinates to LDS, one barrier, every wave takes the
//                   maximum of the 16 wave results (one per lane) and reads the winner's coordinates from LDS.  The LDS
//                   slots alternate by step parity, which is what lets one barrier per step do.
//   streamed tier   a longer segment: kFpsBlocksPerSeg workgroups and one launch per step, back to back.  The workgroups of
//                   step k reduce the partials of step k - 1 (one per workgroup, read by every wave), workgroup 0 writes that
//                   winner to idx, every workgroup updates its slice of t (an fp32 [N] workspace) and writes its partial.
//                   The partials alternate by step parity; a last small launch writes sample K - 1.  Kernel boundaries are
//                   the only synchronisation.
//
// cu, seg_ids and start come from the device unchecked: a segment id outside [0, B) is skipped, a span is clamped to [0, n]
// (and to the capacity of the resident instantiation), start to the segment.
#include <limits.h>
#include <math.h>

#include "wcn_common.h"

namespace wcn {

constexpr int kFpsThreads = 1024;        // threads of a workgroup, both tiers
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsMaxP = 16;             // points per thread of the largest resident instantiation
constexpr int kFpsBlocksPerSeg = 64;     // streamed tier: workgroups of one segment = lanes of the wave that reduces them
constexpr int kFpsMaxGrid = 1024;        // segments of one grid; more are strided over

static_assert(kFpsBlocksPerSeg == 64, "one lane per partial");

struct FpsArgs {
  const float* pts;
  const int32_t* cu;
  const int32_t* seg_ids;  // null: the segments 0 .. nseg - 1
  const int32_t* start;    // null: 0
  int32_t* idx;
  int64_t n;
  int nseg, total_segs, K;
};

// rows [lo, hi) of segment b, inside [0, n] whatever cu holds
__device__ __forceinline__ void fps_span(const int32_t* __restrict__ cu, int b, int64_t n, int64_t& lo, int64_t& hi) {
  lo = cu[b];
  hi = cu[b + 1];
  lo = lo < 0 ? 0 : lo > n ? n : lo;
  hi = hi < lo ? lo : hi > n ? n : hi;
}

// segment of slot sg; false: the slot names none
__device__ __forceinline__ bool fps_segment(const FpsArgs& a, int sg, int& b) {
  b = a.seg_ids ? a.seg_ids[sg] : sg;
  return b >= 0 && b < a.total_segs;
}

__device__ __forceinline__ int fps_start(const FpsArgs& a, int b, int len) {
  int s = a.start ? a.start[b] : 0;
  return s < 0 ? 0 : s >= len ? len - 1 : s;
}

// the contract's distance: three differences, three squares, two sums, each rounded on its own
__device__ __forceinline__ float fps_dist(float x, float y, float z, float sx, float sy, float sz) {
#pragma clang fp contract(off)
  const float dx = x - sx, dy = y - sy, dz = z - sz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

__device__ __forceinline__ unsigned long long fps_key(float t, unsigned local_row) {
  return ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(0xFFFFFFFFu - local_row);
}
__device__ __forceinline__ int64_t fps_key_row(unsigned long long key, int64_t lo) {
  return key == 0ull ? lo : lo + (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}

// v against the key that a DPP move brings from another lane; a lane that the move leaves out receives 0, the key that loses
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long fps_dpp_max(unsigned long long v) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
  return o > v ? o : v;
}

// a running maximum along each row of 16 lanes: lane 15 of a row ends with the row's maximum
__device__ __forceinline__ unsigned long long fps_row_scan(unsigned long long v) {
  v = fps_dpp_max<0x111, 0xf>(v);  // row_shr:1
  v = fps_dpp_max<0x112, 0xf>(v);  // row_shr:2
  v = fps_dpp_max<0x114, 0xf>(v);  // row_shr:4
  return fps_dpp_max<0x118, 0xf>(v);  // row_shr:8
}

// the largest key of the wave, in every lane; all 64 lanes call it.  Register moves only (the shuffles of __shfl_xor go
// through the LDS path): the rows' maxima, the rows' last lanes handed on, lane 63 read out.
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v) {
  v = fps_row_scan(v);
  v = fps_dpp_max<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = fps_dpp_max<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

// the largest key of the first 16 lanes, in every lane; all 64 lanes call it
__device__ __forceinline__ unsigned long long fps_row0_max(unsigned long long v) {
  v = fps_row_scan(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 15);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 15);
  return ((unsigned long long)hi << 32) | lo;
}

// ---- resident tier ---------------------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kFpsThreads) void fps_resident_kernel(const FpsArgs a) {
  __shared__ unsigned long long s_key[2][kFpsWaves];
  __shared__ float4 s_xyz[2][kFpsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ pts = a.pts;
  const int K = a.K;

  for (int sg = blockIdx.x; sg < a.nseg; sg += gridDim.x) {
    int b;
    if (!fps_segment(a, sg, b)) continue;
    int64_t lo, hi;
    fps_span(a.cu, b, a.n, lo, hi);
    const int len = (int)(hi - lo < (int64_t)P * kFpsThreads ? hi - lo : (int64_t)P * kFpsThreads);
    int32_t* __restrict__ out = a.idx + (int64_t)b * K;
    if (len == 0) {
      for (int k0 = 0; k0 < K; k0 += kFpsThreads)
        if (k0 + tid < K) out[k0 + tid] = -1;
      continue;
    }

    // slot j of thread tid = local row j * kFpsThreads + tid; a slot without a row holds t = -1, which no update lowers
    // and no selection takes
    float px[P], py[P], pz[P], t[P];
    const float* __restrict__ mine = pts + (lo + tid) * 3;  // one address per thread; the slots lie at constant distances
#pragma unroll
    for (int j = 0; j < P; ++j) {
      px[j] = py[j] = pz[j] = 0.f;
      t[j] = -1.f;
      if (tid < len - j * kFpsThreads) {
        const float* p = mine + j * (kFpsThreads * 3);
        px[j] = p[0];
        py[j] = p[1];
        pz[j] = p[2];
        t[j] = INFINITY;
      }
    }
    const int s0 = fps_start(a, b, len);
    float sx = pts[(lo + s0) * 3], sy = pts[(lo + s0) * 3 + 1], sz = pts[(lo + s0) * 3 + 2];
    if (tid == 0) out[0] = (int32_t)(lo + s0);

    for (int k = 1; k < K; ++k) {
      float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
      int bj = 0;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float d = fps_dist(px[j], py[j], pz[j], sx, sy, sz);
        const float tj = d < t[j] ? d : t[j];
        t[j] = tj;
        const bool up = tj > best;  // local rows ascend with j: a strict comparison keeps the lowest
        best = up ? tj : best;
        bj = up ? j : bj;
        bx = up ? px[j] : bx;
        by = up ? py[j] : by;
        bz = up ? pz[j] : bz;
      }
      const unsigned long long key = best < 0.f ? 0ull : fps_key(best, (unsigned)(bj * kFpsThreads + tid));
      const unsigned long long wkey = fps_wave_max(key);
      const int par = k & 1;
      if (key == wkey && (key != 0ull || lane == 0)) {  // a row has one owner; a wave without rows: its lane 0
        s_key[par][wave] = wkey;
        s_xyz[par][wave] = make_float4(bx, by, bz, 0.f);
      }
      __syncthreads();
      // lane l of every wave holds the key of wave l % 16: the first row of lanes sees each wave once
      const unsigned long long kw = s_key[par][lane & (kFpsWaves - 1)];
      const unsigned long long top = fps_row0_max(kw);
      const int tw = __ffsll((long long)__ballot(kw == top)) - 1;  // the lowest lane that holds it: below 16, a wave
      const float4 c = s_xyz[par][tw];
      sx = c.x;
      sy = c.y;
      sz = c.z;
      if (tid == 0) out[k] = (int32_t)fps_key_row(top, lo);
      // no second barrier: step k + 1 writes the other parity, and a thread reaches the writes of step k + 2 only through
      // the barrier of step k + 1, which every thread passes after these reads
    }
    __syncthreads();  // the next segment starts at parity 1 again
  }
}

// ---- streamed tier ---------------------------------------------------------------------------------------------------------
struct FpsStream {
  float* t;                    // [n] running distances, by global row; first written in step 1
  unsigned long long* keys;    // [2][nseg][kFpsBlocksPerSeg]
  float4* xyz;                 // [2][nseg][kFpsBlocksPerSeg] coordinates of the row of a key
};

// the winner among the partials of one step of slot sg, in every lane of the calling wave
__device__ __forceinline__ unsigned long long fps_reduce_partials(const FpsStream& w, int parity, int nseg, int sg, float& x,
                                                                  float& y, float& z) {
  const int lane = threadIdx.x & 63;
  const int64_t at = ((int64_t)parity * nseg + sg) * kFpsBlocksPerSeg + lane;
  const unsigned long long key = w.keys[at];
  const float4 c = w.xyz[at];
  const unsigned long long top = fps_wave_max(key);
  const int src = __ffsll((long long)__ballot(key == top)) - 1;  // keys differ unless they are 0
  x = __shfl(c.x, src);
  y = __shfl(c.y, src);
  z = __shfl(c.z, src);
  return top;
}

// step = 1 .. K - 1: writes sample step - 1, updates t against it, leaves the partials of sample `step`
__global__ __launch_bounds__(kFpsThreads) void fps_step_kernel(const FpsArgs a, const FpsStream w, const int step) {
  __shared__ unsigned long long s_key[kFpsWaves];
  __shared__ float4 s_xyz[kFpsWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ pts = a.pts;

  for (int sg = blockIdx.y; sg < a.nseg; sg += gridDim.y) {
    int b;
    if (!fps_segment(a, sg, b)) continue;
    int64_t lo, hi;
    fps_span(a.cu, b, a.n, lo, hi);
    const int64_t len = hi - lo;
    if (len == 0) continue;  // the last launch writes its -1

    float sx, sy, sz;
    int64_t prev;
    if (step == 1) {
      prev = lo + fps_start(a, b, (int)len);
      sx = pts[prev * 3];
      sy = pts[prev * 3 + 1];
      sz = pts[prev * 3 + 2];
    } else {
      prev = fps_key_row(fps_reduce_partials(w, (step - 1) & 1, a.nseg, sg, sx, sy, sz), lo);
    }
    if (blockIdx.x == 0 && tid == 0) a.idx[(int64_t)b * a.K + step - 1] = (int32_t)prev;

    float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    unsigned bi = 0;
    for (int64_t base = (int64_t)blockIdx.x * kFpsThreads; base < len; base += (int64_t)kFpsBlocksPerSeg * kFpsThreads) {
      const int64_t i = base + tid;
      if (i < len) {
        const float* p = pts + (lo + i) * 3;
        const float x = p[0], y = p[1], z = p[2];
        const float d = fps_dist(x, y, z, sx, sy, sz);
        const float told = step == 1 ? INFINITY : w.t[lo + i];
        const float tn = d < told ? d : told;
        w.t[lo + i] = tn;
        if (tn > best) {  // i ascends: a strict comparison keeps the lowest
          best = tn;
          bi = (unsigned)i;
          bx = x;
          by = y;
          bz = z;
        }
      }
    }
    const unsigned long long key = best < 0.f ? 0ull : fps_key(best, bi);
    const unsigned long long wkey = fps_wave_max(key);
    if (key == wkey && (key != 0ull || lane == 0)) {
      s_key[wave] = wkey;
      s_xyz[wave] = make_float4(bx, by, bz, 0.f);
    }
    __syncthreads();
    if (wave == 0) {
      const unsigned long long kw = lane < kFpsWaves ? s_key[lane] : 0ull;
      const unsigned long long top = fps_wave_max(kw);
      const int src = __ffsll((long long)__ballot(lane < kFpsWaves && kw == top)) - 1;
      if (lane == src) {
        const int64_t at = ((int64_t)(step & 1) * a.nseg + sg) * kFpsBlocksPerSeg + blockIdx.x;
        w.keys[at] = top;
        w.xyz[at] = s_xyz[src];
      }
    }
    __syncthreads();  // the LDS slots are rewritten by the next trip
  }
}

// sample K - 1 from the partials of the last step, sample 0 where K = 1, -1 for an empty segment.  One wave per segment.
__global__ __launch_bounds__(64) void fps_last_kernel(const FpsArgs a, const FpsStream w) {
  const int lane = threadIdx.x;
  const int K = a.K;
  for (int sg = blockIdx.x; sg < a.nseg; sg += gridDim.x) {
    int b;
    if (!fps_segment(a, sg, b)) continue;
    int64_t lo, hi;
    fps_span(a.cu, b, a.n, lo, hi);
    int32_t* __restrict__ out = a.idx + (int64_t)b * K;
    if (hi == lo) {
      for (int k0 = 0; k0 < K; k0 += 64)
        if (k0 + lane < K) out[k0 + lane] = -1;
    } else if (K == 1) {
      if (lane == 0) out[0] = (int32_t)(lo + fps_start(a, b, (int)(hi - lo)));
    } else {
      float x, y, z;
      const unsigned long long top = fps_reduce_partials(w, (K - 1) & 1, a.nseg, sg, x, y, z);
      if (lane == 0) out[K - 1] = (int32_t)fps_key_row(top, lo);
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static size_t fps_t_bytes(int64_t n) { return align256((size_t)n * sizeof(float)); }
static size_t fps_key_bytes(int64_t num_segs) { return align256((size_t)2 * num_segs * kFpsBlocksPerSeg * sizeof(unsigned long long)); }
static size_t fps_xyz_bytes(int64_t num_segs) { return align256((size_t)2 * num_segs * kFpsBlocksPerSeg * sizeof(float4)); }

static unsigned fps_grid(int64_t segs) { return (unsigned)(segs < kFpsMaxGrid ? segs : kFpsMaxGrid); }

template <int P>
static void fps_resident_launch(const FpsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fps_resident_kernel<P>, dim3(fps_grid(a.nseg)), dim3(kFpsThreads), 0, s, a);
}

}  // namespace wcn

using namespace wcn;

int64_t wcn_fps_resident_max_points(void) { return (int64_t)kFpsMaxP * kFpsThreads; }
int32_t wcn_fps_block_threads(void) { return kFpsThreads; }
int32_t wcn_fps_blocks_per_segment(void) { return kFpsBlocksPerSeg; }
int32_t wcn_fps_max_grid(void) { return kFpsMaxGrid; }

size_t wcn_fps_workspace_bytes(int64_t n, int64_t num_segs, int32_t k) {
  if (n <= 0 || num_segs <= 0 || k < 1) return 0;
  return fps_t_bytes(n) + fps_key_bytes(num_segs) + fps_xyz_bytes(num_segs);
}

int wcn_fps(const float* points, const int32_t* cu, int64_t total_segs, const int32_t* seg_ids, int64_t num_segs, int64_t n,
            int32_t k, int64_t max_len, const int32_t* start, int32_t tier, void* workspace, size_t workspace_bytes,
            int32_t* idx, wcn_stream_t stream) {
  if (n < 0 || total_segs < 0 || num_segs < 0 || max_len < 0 || k < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (n > INT32_MAX || total_segs > INT32_MAX - 1 || num_segs > INT32_MAX - 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (tier < WCN_FPS_AUTO || tier > WCN_FPS_STREAMED) return WCN_ERROR_INVALID_PARAMETERS;
  if (!seg_ids && num_segs > total_segs) return WCN_ERROR_INVALID_PARAMETERS;
  if (num_segs == 0) return WCN_SUCCESS;
  if (!cu || !idx || (n > 0 && !points)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(points, 4) || !aligned_to(cu, 4) || !aligned_to(seg_ids, 4) || !aligned_to(start, 4) || !aligned_to(idx, 4))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (max_len > n) max_len = n;
  const int64_t cap = wcn_fps_resident_max_points();
  if (tier == WCN_FPS_RESIDENT && max_len > cap) return WCN_ERROR_INVALID_PARAMETERS;
  const bool resident = tier == WCN_FPS_RESIDENT || (tier == WCN_FPS_AUTO && max_len <= cap);

  FpsArgs a;
  a.pts = points;
  a.cu = cu;
  a.seg_ids = seg_ids;
  a.start = start;
  a.idx = idx;
  a.n = n;
  a.nseg = (int)num_segs;
  a.total_segs = (int)total_segs;
  a.K = k;
  hipStream_t s = (hipStream_t)stream;

  if (resident) {
    if (max_len <= 1 * kFpsThreads) fps_resident_launch<1>(a, s);
    else if (max_len <= 2 * kFpsThreads) fps_resident_launch<2>(a, s);
    else if (max_len <= 4 * kFpsThreads) fps_resident_launch<4>(a, s);
    else if (max_len <= 8 * kFpsThreads) fps_resident_launch<8>(a, s);
    else fps_resident_launch<16>(a, s);
    return launch_status();
  }

  FpsStream w;
  w.t = nullptr;
  w.keys = nullptr;
  w.xyz = nullptr;
  if (n > 0) {  // without a row every segment is empty and the last launch alone writes the -1
    if (!workspace || !aligned_to(workspace, 16) || workspace_bytes < wcn_fps_workspace_bytes(n, num_segs, k))
      return WCN_ERROR_INVALID_PARAMETERS;
    w.t = (float*)workspace;
    w.keys = (unsigned long long*)((char*)workspace + fps_t_bytes(n));
    w.xyz = (float4*)((char*)workspace + fps_t_bytes(n) + fps_key_bytes(num_segs));
    const dim3 grid(kFpsBlocksPerSeg, fps_grid(num_segs));
    for (int step = 1; step < k; ++step) hipLaunchKernelGGL(fps_step_kernel, grid, dim3(kFpsThreads), 0, s, a, w, step);
  }
  hipLaunchKernelGGL(fps_last_kernel, dim3(fps_grid(num_segs)), dim3(64), 0, s, a, w);
  return launch_status();
}
