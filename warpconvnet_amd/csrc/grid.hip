// grid.hip - dense grids and point clouds (Grid / FactorGrid geometry).
//
//   a. keys      every point's flat cell id over the grid's cells (points -> grid pooling), or its base cell over the
//                (dims - 1) cell grid of trilinear interpolation together with the three fractions
//   b. sample    out[p, col0 + c] = sum over the 8 corners of w * grid[b, x, y, z, c]; the grid is read through five element
//                strides (b, x, y, z, c), so every memory format and every permuted view is read in place
//   c. backward  d_grid through the same strides, every element written exactly once: a vertex sums over its at most 8
//                adjacent cells in a fixed order and inside a cell over the points in the map's (stable-sorted) order.  A
//                cell of more than kRowChunk points is cut into chunks whose corner sums are formed by gs_bwd_chunk_kernel and
//                added in chunk order: the chunk rule of row_lists.h, with slots derived from the sorted position instead of
//                a list.
// No float atomics: the bits of a result depend on the map alone.  Every grid is capped at kRowMaxGrid workgroups and strides.
#include "row_lists.h"

namespace wcn {

constexpr int kGsPlanarCh = 8;  // channels of one thread of the planar forward kernel

struct GsShape {
  int32_t dims[3];   // vertices per axis
  int32_t cells[3];  // max(dims - 1, 1): base cells of the interpolation
  int64_t stride[5]; // element strides of (b, x, y, z, c)
  int32_t channels;
};

struct GsBounds {
  float lo[3];
  float scale[3];
};

// ---- a. keys ----------------------------------------------------------------------------------------------------------------
// batch element of row i: the last b with offsets[b] <= i (empty elements in between are skipped)
__device__ __forceinline__ int gs_batch_of(const int64_t* __restrict__ offsets, int num_batches, int64_t i) {
  int lo = 0, hi = num_batches;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// NaN -> 0: fmaxf returns the other operand
__device__ __forceinline__ float gs_clamp(float v, float hi) { return fminf(fmaxf(v, 0.0f), hi); }

template <bool CORNER>
__global__ __launch_bounds__(kRowThreads) void gs_keys_kernel(const float* __restrict__ pos, int64_t n,
                                                             const int64_t* __restrict__ offsets, int num_batches, GsShape sh,
                                                             GsBounds bd, int64_t* __restrict__ keys,
                                                             float* __restrict__ frac) {
  for (int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowThreads) {
    const int b = gs_batch_of(offsets, num_batches, i);
    int64_t flat = b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float d = pos[i * 3 + a] - bd.lo[a];
      const float u = gs_clamp(d * bd.scale[a], (float)(sh.dims[a] - 1));
      if (CORNER) {
        const int top = sh.dims[a] - 2 > 0 ? sh.dims[a] - 2 : 0;
        int i0 = (int)floorf(u);
        i0 = i0 < top ? i0 : top;
        frac[i * 3 + a] = u - (float)i0;
        flat = flat * sh.cells[a] + i0;
      } else {
        flat = flat * sh.dims[a] + (int)u;
      }
    }
    keys[i] = flat;
  }
}

// ---- b. sample --------------------------------------------------------------------------------------------------------------
struct GsPoint {
  int64_t off[8];  // element offsets of the 8 corners (channel 0), order (dx, dy, dz), dz fastest
  float w[8];
};

// weights: w = wx * wy * wz multiplied in that order, w_a in {1 - f_a, f_a}
__device__ __forceinline__ void gs_weights(float fx, float fy, float fz, float* w) {
  const float ax[2] = {1.0f - fx, fx}, ay[2] = {1.0f - fy, fy}, az[2] = {1.0f - fz, fz};
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = ax[k >> 2] * ay[(k >> 1) & 1] * az[k & 1];
}

__device__ __forceinline__ void gs_cell_of(const GsShape& sh, int64_t key, int& b, int& cx, int& cy, int& cz) {
  cz = (int)(key % sh.cells[2]);
  key /= sh.cells[2];
  cy = (int)(key % sh.cells[1]);
  key /= sh.cells[1];
  cx = (int)(key % sh.cells[0]);
  b = (int)(key / sh.cells[0]);
}

__device__ __forceinline__ void gs_point(const GsShape& sh, int64_t key, const float* __restrict__ f, GsPoint& pt) {
  int b, c0[3];
  gs_cell_of(sh, key, b, c0[0], c0[1], c0[2]);
  int64_t o[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int hi = c0[a] + 1 < sh.dims[a] ? c0[a] + 1 : sh.dims[a] - 1;  // an axis of one vertex: both corners are vertex 0
    o[a][0] = c0[a] * sh.stride[1 + a];
    o[a][1] = hi * sh.stride[1 + a];
  }
  const int64_t ob = b * sh.stride[0];
#pragma unroll
  for (int k = 0; k < 8; ++k) pt.off[k] = ob + o[0][k >> 2] + o[1][(k >> 1) & 1] + o[2][k & 1];
  gs_weights(f[0], f[1], f[2], pt.w);
}

// channel stride 1: `lanes` lanes (a power of two, <= 64) per point, VEC channels per access
template <typename T, int VEC>
__global__ __launch_bounds__(kRowThreads) void gs_fwd_rows_kernel(GsShape sh, const T* __restrict__ grid,
                                                                 const int64_t* __restrict__ keys,
                                                                 const int64_t* __restrict__ perm,
                                                                 const float* __restrict__ frac, int64_t n, T* __restrict__ out,
                                                                 int64_t pitch, int64_t col0, int lanes) {
  const int per_block = kRowThreads / lanes, group = threadIdx.x / lanes, lane = threadIdx.x % lanes;
  for (int64_t j = (int64_t)blockIdx.x * per_block + group; j < n; j += (int64_t)gridDim.x * per_block) {
    const int64_t p = perm[j];
    GsPoint pt;
    gs_point(sh, keys[j], frac + p * 3, pt);
    T* __restrict__ row = out + p * pitch + col0;
    for (int c = lane * VEC; c < sh.channels; c += lanes * VEC) {
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const Vec<T, VEC> x = *reinterpret_cast<const Vec<T, VEC>*>(grid + pt.off[k] + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = fmaf(pt.w[k], (float)x.v[i], acc[i]);
      }
      Vec<T, VEC> y;
#pragma unroll
      for (int i = 0; i < VEC; ++i) y.v[i] = (T)acc[i];
      *reinterpret_cast<Vec<T, VEC>*>(row + c) = y;
    }
  }
}

// planar channels: one thread per (point, kGsPlanarCh channels), points fastest, so that the lanes of a wave read
// neighbouring cells of one channel plane
template <typename T>
__global__ __launch_bounds__(kRowThreads) void gs_fwd_planar_kernel(GsShape sh, const T* __restrict__ grid,
                                                                   const int64_t* __restrict__ keys,
                                                                   const int64_t* __restrict__ perm,
                                                                   const float* __restrict__ frac, int64_t n,
                                                                   T* __restrict__ out, int64_t pitch, int64_t col0) {
  const int64_t pieces = (sh.channels + kGsPlanarCh - 1) / kGsPlanarCh, items = pieces * n;
  for (int64_t it = (int64_t)blockIdx.x * kRowThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kRowThreads) {
    const int64_t j = it % n;
    const int cb = (int)(it / n) * kGsPlanarCh;
    const int64_t p = perm[j];
    GsPoint pt;
    gs_point(sh, keys[j], frac + p * 3, pt);
    T* __restrict__ row = out + p * pitch + col0;
    const int ce = cb + kGsPlanarCh < sh.channels ? cb + kGsPlanarCh : sh.channels;
    for (int c = cb; c < ce; ++c) {
      const int64_t oc = c * sh.stride[4];
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fmaf(pt.w[k], (float)(grid[pt.off[k] + oc]), acc);
      row[c] = (T)acc;
    }
  }
}

// ---- c. backward ------------------------------------------------------------------------------------------------------------
// slot of the chunk of a crowded cell that starts at sorted position `start`: two slots per kRowChunk positions, the odd one
// for a cell's first chunk.  Crowded cells are longer than kRowChunk, so no two first chunks and no two later chunks start
// inside the same kRowChunk positions.
__device__ __forceinline__ int64_t gs_chunk_slot(int64_t start, bool first) {
  return 2 * (start / kRowChunk) + (first ? 1 : 0);
}

// one workgroup per kRowChunk sorted positions: the (at most two) chunk heads among them, then the 8 corner sums of each
// chunk, one channel per thread, over the chunk's points in order
template <typename T>
__global__ __launch_bounds__(kRowThreads) void gs_bwd_chunk_kernel(int channels, const T* __restrict__ dy, int64_t pitch,
                                                                  int64_t col0, const int64_t* __restrict__ keys,
                                                                  const int64_t* __restrict__ perm,
                                                                  const int64_t* __restrict__ cell_offsets,
                                                                  const float* __restrict__ frac, int64_t n,
                                                                  float* __restrict__ partials) {
  static_assert(kRowThreads == kRowChunk, "one thread per sorted position of a tile");
  __shared__ int64_t s_start[2];
  __shared__ int s_len[2], s_first[2], s_heads;
  const int64_t tiles = (n + kRowChunk - 1) / kRowChunk;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    if (threadIdx.x == 0) s_heads = 0;
    __syncthreads();
    const int64_t x = t * kRowChunk + threadIdx.x;
    if (x < n) {
      const int64_t key = keys[x], o0 = cell_offsets[key], o1 = cell_offsets[key + 1];
      if (o1 - o0 > kRowChunk && (x - o0) % kRowChunk == 0) {
        const int h = atomicAdd(&s_heads, 1);  // at most two heads: one first chunk, one later chunk
        if (h < 2) {
          s_start[h] = x;
          s_len[h] = (int)(o1 - x < kRowChunk ? o1 - x : kRowChunk);
          s_first[h] = x == o0;
        }
      }
    }
    __syncthreads();
    const int heads = s_heads < 2 ? s_heads : 2;
    for (int h = 0; h < heads; ++h) {
      const int64_t start = s_start[h];
      const int len = s_len[h];
      float* __restrict__ dst = partials + gs_chunk_slot(start, s_first[h]) * 8 * channels;
      for (int c = threadIdx.x; c < channels; c += kRowThreads) {
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
        for (int i = 0; i < len; ++i) {
          const int64_t p = perm[start + i];
          float w[8];
          gs_weights(frac[p * 3], frac[p * 3 + 1], frac[p * 3 + 2], w);
          const float g = (float)dy[p * pitch + col0 + c];
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] = fmaf(w[k], g, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k * channels + c] = acc[k];
      }
    }
    __syncthreads();  // the head list is rewritten by the next trip
  }
}

// `lanes` lanes (a power of two, <= 64) per vertex, lanes over channels: the rows of dy are read 4 bytes a lane, coalesced
template <typename T>
__global__ __launch_bounds__(kRowThreads) void gs_bwd_vertex_kernel(GsShape sh, int64_t vertices, const T* __restrict__ dy,
                                                                   int64_t pitch, int64_t col0,
                                                                   const int64_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ cell_offsets,
                                                                   const float* __restrict__ frac,
                                                                   const float* __restrict__ partials, T* __restrict__ dgrid,
                                                                   int lanes) {
  const int per_block = kRowThreads / lanes, group = threadIdx.x / lanes, lane = threadIdx.x % lanes;
  const int C = sh.channels;
  for (int64_t v = (int64_t)blockIdx.x * per_block + group; v < vertices; v += (int64_t)gridDim.x * per_block) {
    int64_t r = v;
    const int z = (int)(r % sh.dims[2]);
    r /= sh.dims[2];
    const int y = (int)(r % sh.dims[1]);
    r /= sh.dims[1];
    const int x = (int)(r % sh.dims[0]);
    const int64_t b = r / sh.dims[0];
    T* __restrict__ dst = dgrid + b * sh.stride[0] + x * sh.stride[1] + y * sh.stride[2] + z * sh.stride[3];
    for (int c = lane; c < C; c += lanes) {
      float acc = 0.0f;
      for (int a = 0; a < 8; ++a) {  // adjacent cells in the order (x - 1, x) x (y - 1, y) x (z - 1, z), z fastest
        const int cx = x - 1 + (a >> 2), cy = y - 1 + ((a >> 1) & 1), cz = z - 1 + (a & 1);
        if (cx < 0 || cy < 0 || cz < 0 || cx >= sh.cells[0] || cy >= sh.cells[1] || cz >= sh.cells[2]) continue;
        const int corner = 7 - a;  // the vertex is corner (1 - ax, 1 - ay, 1 - az) of that cell
        // an axis of one vertex has one cell whose two corners are both vertex 0: the upper one weighs exactly 0
        const int64_t cell = ((b * sh.cells[0] + cx) * sh.cells[1] + cy) * sh.cells[2] + cz;
        const int64_t o0 = cell_offsets[cell], o1 = cell_offsets[cell + 1];
        if (partials && o1 - o0 > kRowChunk) {  // no partials: the caller vouched for short cells
          for (int64_t s = o0; s < o1; s += kRowChunk)
            acc += partials[(gs_chunk_slot(s, s == o0) * 8 + corner) * C + c];
        } else {
          for (int64_t j = o0; j < o1; ++j) {
            const int64_t p = perm[j];
            const float fx = frac[p * 3], fy = frac[p * 3 + 1], fz = frac[p * 3 + 2];
            const float wx = (corner & 4) ? fx : 1.0f - fx, wy = (corner & 2) ? fy : 1.0f - fy,
                        wz = (corner & 1) ? fz : 1.0f - fz;
            acc = fmaf(wx * wy * wz, (float)dy[p * pitch + col0 + c], acc);
          }
        }
      }
      dst[c * sh.stride[4]] = (T)acc;
    }
  }
}

// dims >= 1, their product and the batch count inside int32 where indices are 32-bit
static bool gs_shape_ok(const int32_t* dims, int64_t num_batches, int64_t* vertices) {
  if (!dims || num_batches < 0) return false;
  int64_t v = num_batches > 0 ? num_batches : 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) return false;
    v *= dims[a];
    if (v > INT32_MAX) return false;
  }
  *vertices = num_batches > 0 ? v : 0;
  return true;
}

static GsShape gs_shape(const int32_t* dims, const int64_t* strides, int32_t channels) {
  GsShape sh;
  for (int a = 0; a < 3; ++a) {
    sh.dims[a] = dims[a];
    sh.cells[a] = dims[a] > 1 ? dims[a] - 1 : 1;
  }
  for (int a = 0; a < 5; ++a) sh.stride[a] = strides ? strides[a] : 0;
  sh.channels = channels;
  return sh;
}

template <typename T>
static void gs_launch_forward(const GsShape& sh, const void* grid, const int64_t* keys, const int64_t* perm, const float* frac,
                              int64_t n, void* out, int64_t pitch, int64_t col0, hipStream_t s) {
  constexpr int V = 16 / sizeof(T);
  const T* g = (const T*)grid;
  T* o = (T*)out;
  if (sh.stride[4] == 1) {
    const bool wide = sh.channels % V == 0 && pitch % V == 0 && col0 % V == 0 && aligned_to(g, 16) && aligned_to(o, 16) &&
                      sh.stride[0] % V == 0 && sh.stride[1] % V == 0 && sh.stride[2] % V == 0 && sh.stride[3] % V == 0;
    const int lanes = row_lanes(wide ? sh.channels / V : sh.channels);
    const unsigned blocks = capped_grid(ceil_div(n, kRowThreads / lanes));
    if (wide) gs_fwd_rows_kernel<T, V><<<blocks, kRowThreads, 0, s>>>(sh, g, keys, perm, frac, n, o, pitch, col0, lanes);
    else gs_fwd_rows_kernel<T, 1><<<blocks, kRowThreads, 0, s>>>(sh, g, keys, perm, frac, n, o, pitch, col0, lanes);
  } else {
    const int64_t items = ceil_div(sh.channels, kGsPlanarCh) * n;
    gs_fwd_planar_kernel<T><<<capped_grid(ceil_div(items, kRowThreads)), kRowThreads, 0, s>>>(sh, g, keys, perm, frac, n, o, pitch, col0);
  }
}

template <typename T>
static void gs_launch_backward(const GsShape& sh, int64_t vertices, const void* dy, int64_t pitch, int64_t col0,
                               const int64_t* keys, const int64_t* perm, const int64_t* cell_offsets, const float* frac,
                               int64_t n, bool chunks, float* partials, void* dgrid, hipStream_t s) {
  if (chunks)
    gs_bwd_chunk_kernel<T><<<capped_grid(ceil_div(n, kRowChunk)), kRowThreads, 0, s>>>(
        sh.channels, (const T*)dy, pitch, col0, keys, perm, cell_offsets, frac, n, partials);
  const int lanes = row_lanes(sh.channels);
  gs_bwd_vertex_kernel<T><<<capped_grid(ceil_div(vertices, kRowThreads / lanes)), kRowThreads, 0, s>>>(
      sh, vertices, (const T*)dy, pitch, col0, perm, cell_offsets, frac, partials, (T*)dgrid, lanes);
}

static size_t gs_partial_bytes(int64_t n, int32_t channels) {
  return (size_t)(2 * ceil_div(n, kRowChunk) + 2) * 8 * (size_t)channels * sizeof(float);
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int32_t wcn_grid_max_grid(void) { return kRowMaxGrid; }
int32_t wcn_grid_chunk_points(void) { return kRowChunk; }

int wcn_grid_point_keys(const float* points, int64_t n, const int64_t* point_offsets, int32_t num_batches, const int32_t* dims,
                        const float* lo, const float* scale, int32_t mode, int64_t* keys, float* fractions,
                        wcn_stream_t stream) {
  int64_t vertices;
  if (n < 0 || n > INT32_MAX || num_batches < 1 || !gs_shape_ok(dims, num_batches, &vertices) || !lo || !scale)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (mode != WCN_GRID_KEY_CELL && mode != WCN_GRID_KEY_CORNER) return WCN_ERROR_INVALID_PARAMETERS;
  if (n == 0) return WCN_SUCCESS;
  if (!points || !point_offsets || !keys || (mode == WCN_GRID_KEY_CORNER && !fractions)) return WCN_ERROR_INVALID_PARAMETERS;
  const GsShape sh = gs_shape(dims, nullptr, 0);
  GsBounds bd;
  for (int a = 0; a < 3; ++a) {
    bd.lo[a] = lo[a];
    bd.scale[a] = scale[a];
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = capped_grid(ceil_div(n, kRowThreads));
  if (mode == WCN_GRID_KEY_CORNER)
    gs_keys_kernel<true><<<g, kRowThreads, 0, s>>>(points, n, point_offsets, num_batches, sh, bd, keys, fractions);
  else
    gs_keys_kernel<false><<<g, kRowThreads, 0, s>>>(points, n, point_offsets, num_batches, sh, bd, keys, fractions);
  return launch_status();
}

static int gs_sample_args(const int64_t* strides, const int32_t* dims, int32_t channels, int32_t dtype,
                          int64_t num_batches, int64_t n, int64_t pitch, int64_t col0, int64_t* vertices) {
  if (n < 0 || n > INT32_MAX || channels < 0 || !gs_shape_ok(dims, num_batches, vertices) || !strides || pitch < 0 ||
      col0 < 0 || col0 + channels > pitch)
    return WCN_ERROR_INVALID_PARAMETERS;
  for (int a = 0; a < 5; ++a)
    if (strides[a] < 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (!dtype_ok(dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return WCN_SUCCESS;
}

int wcn_grid_sample(const void* grid, const int64_t* strides, const int32_t* dims, int32_t channels, int32_t dtype,
                    int64_t num_batches, const int64_t* sorted_keys, const int64_t* perm, const float* fractions, int64_t n,
                    void* out, int64_t out_pitch, int64_t col0, wcn_stream_t stream) {
  int64_t vertices;
  const int st = gs_sample_args(strides, dims, channels, dtype, num_batches, n, out_pitch, col0, &vertices);
  if (st != WCN_SUCCESS) return st;
  if (n == 0 || channels == 0) return WCN_SUCCESS;
  if (!grid || !sorted_keys || !perm || !fractions || !out || vertices == 0) return WCN_ERROR_INVALID_PARAMETERS;
  const GsShape sh = gs_shape(dims, strides, channels);
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    gs_launch_forward<decltype(t)>(sh, grid, sorted_keys, perm, fractions, n, out, out_pitch, col0, s);
    return launch_status();
  });
}

size_t wcn_grid_sample_backward_workspace_bytes(int64_t n, int32_t channels) {
  if (n < 0 || channels < 0) return 0;
  return gs_partial_bytes(n, channels);
}

int wcn_grid_sample_backward(const void* dy, int64_t dy_pitch, int64_t col0, const int64_t* strides, const int32_t* dims,
                             int32_t channels, int32_t dtype, int64_t num_batches, const int64_t* sorted_keys,
                             const int64_t* perm, const int64_t* cell_offsets, const float* fractions, int64_t n,
                             int64_t max_cell_points, void* d_grid, void* workspace, size_t workspace_bytes,
                             wcn_stream_t stream) {
  int64_t vertices;
  const int st = gs_sample_args(strides, dims, channels, dtype, num_batches, n, dy_pitch, col0, &vertices);
  if (st != WCN_SUCCESS) return st;
  if (vertices == 0 || channels == 0) return WCN_SUCCESS;
  if (!d_grid || !cell_offsets || (n > 0 && (!dy || !sorted_keys || !perm || !fractions))) return WCN_ERROR_INVALID_PARAMETERS;
  const bool chunks = n > kRowChunk && (max_cell_points < 0 || max_cell_points > kRowChunk);
  if (chunks && (!workspace || workspace_bytes < gs_partial_bytes(n, channels))) return WCN_ERROR_INVALID_PARAMETERS;
  const GsShape sh = gs_shape(dims, strides, channels);
  hipStream_t s = (hipStream_t)stream;
  float* part = chunks ? (float*)workspace : nullptr;
  return with_dtype(dtype, [&](auto t) {
    gs_launch_backward<decltype(t)>(sh, vertices, dy, dy_pitch, col0, sorted_keys, perm, cell_offsets, fractions, n, chunks, part,
                                    d_grid, s);
    return launch_status();
  });
}

}  // extern "C"
