// dual_grid.hip - flexible-dual-grid -> triangle-mesh extraction.
//
// Every voxel carries one dual vertex and three flags: flag a says the surface crosses the primal edge along axis a through
// the voxel's maximum corner.  A flagged edge whose four surrounding voxels all exist yields one quad (two triangles); the
// others are dropped.  The four voxels are columns of the kernel map of the voxel set onto itself with kernel_size (2, 2, 2):
// column 4 i + 2 j + l of the row-major table is the voxel at +(i, j, l) (include/wcn.h, "kernel map"), so no search
// structure is built here.
//
//   wcn_fdg_count   kept (row, axis) pairs per row and per 256-row tile, then one workgroup scans the tiles and writes
//                   quad_offsets [B + 1] (quads in front of every scene; the last entry is the total)
//   wcn_fdg_emit    one lane per voxel: its vertex, and for each kept axis the quad and its two faces at the rank the scan
//                   gives - quads are ordered by (row, axis), nothing is atomic, the result does not depend on the launch
//
// The fp32 arithmetic is fixed operation by operation (no contraction), so that the torch backend
// (nn/functional/dual_grid.py) picks the same split on every quad, exact ties included.

#include "wcn_common.h"

namespace wcn {

constexpr int kFdgThreads = 256;

// ---- the three tables of the definition (nn/functional/dual_grid.py holds the same data) -----------------------------------
// kFdgQuadCols[a][i]: kernel-map column of corner q_i of the quad around the edge along axis a, in cyclic order
//   x: (0,0,0) (0,0,1) (0,1,1) (0,1,0)    y: (0,0,0) (1,0,0) (1,0,1) (0,0,1)    z: (0,0,0) (0,1,0) (1,1,0) (1,0,0)
__device__ constexpr int kFdgQuadCols[3][4] = {{0, 1, 3, 2}, {0, 4, 5, 1}, {0, 2, 6, 4}};
// corners of the two triangles of either split
__device__ constexpr int kFdgSplit1[2][3] = {{0, 1, 2}, {0, 2, 3}};
__device__ constexpr int kFdgSplit2[2][3] = {{0, 1, 3}, {3, 1, 2}};

struct FdgWs {
  uint8_t* cnt;   // [N]      kept axes of every row
  int32_t* tile;  // [T + 1]  quads in front of every 256-row tile, the last entry their total
};
static inline int64_t fdg_tiles(int64_t n) { return ceil_div(n > 0 ? n : 0, kFdgThreads); }
static inline FdgWs carve_fdg(void* ws, int64_t n) {
  FdgWs w;
  w.cnt = (uint8_t*)ws;
  w.tile = (int32_t*)((uint8_t*)ws + ((n + 15) & ~(int64_t)15));
  return w;
}

// the row's eight neighbours: one 32-B access
struct FdgRow {
  int32_t c[8];
};
__device__ __forceinline__ FdgRow fdg_row(const int32_t* __restrict__ nbr, int64_t p) {
  const int4 lo = *reinterpret_cast<const int4*>(nbr + p * 8);
  const int4 hi = *reinterpret_cast<const int4*>(nbr + p * 8 + 4);
  FdgRow r;
  r.c[0] = lo.x; r.c[1] = lo.y; r.c[2] = lo.z; r.c[3] = lo.w;
  r.c[4] = hi.x; r.c[5] = hi.y; r.c[6] = hi.z; r.c[7] = hi.w;
  return r;
}

// bit a = axis a yields a quad: flagged, and the three other voxels around the edge exist (corner 0 is the row itself)
__device__ __forceinline__ int fdg_kept(const FdgRow& r, const uint8_t* __restrict__ flags, int64_t p, int64_t n) {
  int kept = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bool ok = flags[p * 3 + a] != 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const int32_t q = r.c[kFdgQuadCols[a][i]];
      ok = ok && q >= 0 && q < n;
    }
    kept |= ok ? 1 << a : 0;
  }
  return kept;
}

__global__ __launch_bounds__(kFdgThreads) void fdg_count_kernel(const int32_t* __restrict__ nbr,
                                                                const uint8_t* __restrict__ flags, int64_t n,
                                                                uint8_t* __restrict__ cnt, int32_t* __restrict__ tile) {
  const int64_t p = (int64_t)blockIdx.x * kFdgThreads + threadIdx.x;
  int c = 0;
  if (p < n) {
    c = __popc(fdg_kept(fdg_row(nbr, p), flags, p, n));
    cnt[p] = (uint8_t)c;
  }
  __shared__ int s_w[kFdgThreads / 64];
  int total;
  block_excl_scan<kFdgThreads>(c, s_w, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// one workgroup: tile counts -> exclusive prefix in place (tile[T] = total); quad_offsets[b] = quads of the rows in front of
// row offsets[b] (the prefix of its tile plus the counts of the tile's rows in front of it)
__global__ __launch_bounds__(kFdgThreads) void fdg_scan_kernel(int32_t* __restrict__ tile, int64_t T,
                                                               const uint8_t* __restrict__ cnt, int64_t n,
                                                               const int32_t* __restrict__ offsets, int num_batches,
                                                               int32_t* __restrict__ quad_offsets) {
  __shared__ int s_w[kFdgThreads / 64];
  int carry = 0;
  for (int64_t base = 0; base < T; base += kFdgThreads) {
    const int64_t e = base + threadIdx.x;
    const int v = e < T ? tile[e] : 0;
    int total;
    const int excl = block_excl_scan<kFdgThreads>(v, s_w, &total);
    if (e < T) tile[e] = carry + excl;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) tile[T] = carry;
  __syncthreads();
  for (int b = threadIdx.x; b <= num_batches; b += kFdgThreads) {
    int64_t r = b >= num_batches ? n : (int64_t)offsets[b];
    r = r < 0 ? 0 : r > n ? n : r;
    int v = carry;
    if (r < n) {
      const int64_t t = r / kFdgThreads;
      v = tile[t];
      for (int64_t i = t * kFdgThreads; i < r; ++i) v += cnt[i];
    }
    quad_offsets[b] = v;
  }
}

// One fp32 operation, rounded once: plain operators under `fp contract(off)`, as in fps.hip.  (__fmul_rn / __fadd_rn are
// inline functions compiled with contraction allowed: once inlined next to each other their product and sum become one FMA,
// which shows as soon as the voxel size is no power of two.)
__device__ __forceinline__ float fdg_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float fdg_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float fdg_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

struct FdgGeom {
  float vs, lx, ly, lz;  // voxel size, lower corner of the box
};
struct FdgVec {
  float x, y, z;
};

// V = ((float(c) + d) * voxel_size) + lo: three operations, each rounded
template <typename T>
__device__ __forceinline__ FdgVec fdg_vertex(const int4* __restrict__ coords, const T* __restrict__ dual, int64_t row,
                                             const FdgGeom& g) {
  const int4 c = coords[row];
  const float dx = (float)dual[row * 3], dy = (float)dual[row * 3 + 1], dz = (float)dual[row * 3 + 2];
  FdgVec v;
  v.x = fdg_add(fdg_mul(fdg_add((float)c.y, dx), g.vs), g.lx);
  v.y = fdg_add(fdg_mul(fdg_add((float)c.z, dy), g.vs), g.ly);
  v.z = fdg_add(fdg_mul(fdg_add((float)c.w, dz), g.vs), g.lz);
  return v;
}

// cross(b - a, c - a): differences, then every component as mul, mul, sub
__device__ __forceinline__ FdgVec fdg_normal(const FdgVec& a, const FdgVec& b, const FdgVec& c) {
  const float ux = fdg_sub(b.x, a.x), uy = fdg_sub(b.y, a.y), uz = fdg_sub(b.z, a.z);
  const float vx = fdg_sub(c.x, a.x), vy = fdg_sub(c.y, a.y), vz = fdg_sub(c.z, a.z);
  FdgVec n;
  n.x = fdg_sub(fdg_mul(uy, vz), fdg_mul(uz, vy));
  n.y = fdg_sub(fdg_mul(uz, vx), fdg_mul(ux, vz));
  n.z = fdg_sub(fdg_mul(ux, vy), fdg_mul(uy, vx));
  return n;
}
// |(x x' + y y') + z z'|
__device__ __forceinline__ float fdg_align(const FdgVec& m, const FdgVec& n) {
  return fabsf(fdg_add(fdg_add(fdg_mul(m.x, n.x), fdg_mul(m.y, n.y)), fdg_mul(m.z, n.z)));
}

// TV / TW: element types of the dual offsets and of the split weights; GEOM: no weights, the split compares the normals
template <typename TV, typename TW, bool GEOM>
__global__ __launch_bounds__(kFdgThreads) void fdg_emit_kernel(const int32_t* __restrict__ nbr, const uint8_t* __restrict__ flags,
                                                               const int4* __restrict__ coords,
                                                               const int32_t* __restrict__ offsets, int num_batches,
                                                               const TV* __restrict__ dual, const TW* __restrict__ lerp,
                                                               int64_t n, FdgGeom g, const int32_t* __restrict__ tile,
                                                               int64_t capacity, float* __restrict__ verts,
                                                               int4* __restrict__ quads, int32_t* __restrict__ faces) {
  const int64_t p = (int64_t)blockIdx.x * kFdgThreads + threadIdx.x;
  FdgRow r;
  int kept = 0;
  if (p < n) {
    r = fdg_row(nbr, p);
    kept = fdg_kept(r, flags, p, n);
  }
  __shared__ int s_w[kFdgThreads / 64];
  int total;
  int64_t pos = (int64_t)tile[blockIdx.x] + block_excl_scan<kFdgThreads>(__popc(kept), s_w, &total);
  if (p >= n) return;
  FdgVec v0 = {0.f, 0.f, 0.f};
  if (dual) {
    v0 = fdg_vertex(coords, dual, p, g);
    if (verts) {
      verts[p * 3] = v0.x;
      verts[p * 3 + 1] = v0.y;
      verts[p * 3 + 2] = v0.z;
    }
  }
  if (!kept || (!quads && !faces)) return;
  const int b = coords[p].x;
  const int32_t first = b >= 0 && b < num_batches ? offsets[b] : 0;  // indices are local to the scene
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(kept >> a & 1)) continue;
    if (pos >= capacity) return;
    int32_t q[4];
    q[0] = (int32_t)p;
#pragma unroll
    for (int i = 1; i < 4; ++i) q[i] = r.c[kFdgQuadCols[a][i]];
    if (quads) quads[pos] = make_int4(q[0] - first, q[1] - first, q[2] - first, q[3] - first);
    if (faces) {
      bool split1;
      if constexpr (GEOM) {
        const FdgVec v1 = fdg_vertex(coords, dual, q[1], g), v2 = fdg_vertex(coords, dual, q[2], g),
                     v3 = fdg_vertex(coords, dual, q[3], g);
        const float align1 = fdg_align(fdg_normal(v0, v1, v2), fdg_normal(v0, v2, v3));
        const float align2 = fdg_align(fdg_normal(v0, v1, v3), fdg_normal(v3, v1, v2));
        split1 = align1 > align2;
      } else {
        const float w0 = (float)lerp[q[0]], w1 = (float)lerp[q[1]], w2 = (float)lerp[q[2]], w3 = (float)lerp[q[3]];
        split1 = fdg_mul(w0, w2) > fdg_mul(w1, w3);
      }
      int32_t f[6];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 3; ++j) f[t * 3 + j] = (split1 ? q[kFdgSplit1[t][j]] : q[kFdgSplit2[t][j]]) - first;
      int2* dst = reinterpret_cast<int2*>(faces + pos * 6);  // 24 B per quad: 8-B aligned
      dst[0] = make_int2(f[0], f[1]);
      dst[1] = make_int2(f[2], f[3]);
      dst[2] = make_int2(f[4], f[5]);
    }
    ++pos;
  }
}

template <typename TV, typename TW, bool GEOM>
static void fdg_launch_emit(int64_t T, hipStream_t s, const int32_t* nbr, const uint8_t* flags, const int32_t* coords,
                            const int32_t* offsets, int num_batches, const void* dual, const void* lerp, int64_t n,
                            const FdgGeom& g, const int32_t* tile, int64_t capacity, float* verts, int32_t* quads,
                            int32_t* faces) {
  hipLaunchKernelGGL((fdg_emit_kernel<TV, TW, GEOM>), dim3((unsigned)T), dim3(kFdgThreads), 0, s, nbr, flags,
                     (const int4*)coords, offsets, num_batches, (const TV*)dual, (const TW*)lerp, n, g, tile, capacity, verts,
                     (int4*)quads, faces);
}

}  // namespace wcn

using namespace wcn;

extern "C" {

int wcn_fdg_supported(int32_t dual_dtype, int32_t lerp_dtype) {
  return dtype_ok(dual_dtype) && (lerp_dtype < 0 || dtype_ok(lerp_dtype)) ? 1 : 0;
}

size_t wcn_fdg_workspace(int64_t n) {
  const int64_t N = n > 0 ? n : 0;
  return (size_t)((N + 15) & ~(int64_t)15) + (size_t)(fdg_tiles(N) + 4) * sizeof(int32_t);
}

int wcn_fdg_count(const int32_t* nbr, int32_t pitch, const uint8_t* flags, int64_t n, const int32_t* offsets,
                  int32_t num_batches, void* workspace, size_t workspace_bytes, int32_t* quad_offsets, wcn_stream_t stream) {
  if (n < 0 || num_batches < 0 || n >= (1ll << 31) / 6 || pitch != 8) return WCN_ERROR_INVALID_PARAMETERS;
  if (!workspace || workspace_bytes < wcn_fdg_workspace(n) || !quad_offsets || !aligned_to(workspace, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  if ((num_batches > 0 && !offsets) || (n > 0 && (!nbr || !flags || !aligned_to(nbr, 16)))) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  const FdgWs w = carve_fdg(workspace, n);
  const int64_t T = fdg_tiles(n);
  if (T > 0) hipLaunchKernelGGL(fdg_count_kernel, dim3((unsigned)T), dim3(kFdgThreads), 0, s, nbr, flags, n, w.cnt, w.tile);
  hipLaunchKernelGGL(fdg_scan_kernel, dim3(1), dim3(kFdgThreads), 0, s, w.tile, T, w.cnt, n, offsets, (int)num_batches,
                     quad_offsets);
  return launch_status();
}

int wcn_fdg_emit(const int32_t* nbr, int32_t pitch, const uint8_t* flags, const int32_t* coords, int64_t n,
                 const int32_t* offsets, int32_t num_batches, const void* dual, int32_t dual_dtype, const void* lerp,
                 int32_t lerp_dtype, float voxel_size, const float lo[3], const void* workspace, size_t workspace_bytes,
                 int64_t capacity, float* verts, int32_t* quads, int32_t* faces, wcn_stream_t stream) {
  if (n < 0 || num_batches < 0 || capacity < 0 || n >= (1ll << 31) / 6 || pitch != 8) return WCN_ERROR_INVALID_PARAMETERS;
  if (dual && !dtype_ok(dual_dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (lerp && !dtype_ok(lerp_dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!workspace || workspace_bytes < wcn_fdg_workspace(n) || !aligned_to(workspace, 16)) return WCN_ERROR_INVALID_PARAMETERS;
  if ((verts && !dual) || (faces && !dual && !lerp) || (dual && !lo)) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(quads, 16) || !aligned_to(faces, 8)) return WCN_ERROR_INVALID_PARAMETERS;
  if (n == 0) return WCN_SUCCESS;
  if (!nbr || !flags || !coords || !aligned_to(nbr, 16) || !aligned_to(coords, 16) || (num_batches > 0 && !offsets))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!verts && !quads && !faces) return WCN_SUCCESS;
  hipStream_t s = (hipStream_t)stream;
  const FdgWs w = carve_fdg(const_cast<void*>(workspace), n);
  const int64_t T = fdg_tiles(n);
  FdgGeom g = {voxel_size, 0.f, 0.f, 0.f};
  if (lo) g.lx = lo[0], g.ly = lo[1], g.lz = lo[2];
  const int dd = dual ? dual_dtype : WCN_F32;
  with_dtype(dd, [&](auto tv) {
    using TV = decltype(tv);
    if (!lerp) {
      fdg_launch_emit<TV, float, true>(T, s, nbr, flags, coords, offsets, num_batches, dual, nullptr, n, g, w.tile, capacity,
                                       verts, quads, faces);
      return 0;
    }
    return with_dtype(lerp_dtype, [&](auto tw) {
      using TW = decltype(tw);
      fdg_launch_emit<TV, TW, false>(T, s, nbr, flags, coords, offsets, num_batches, dual, lerp, n, g, w.tile, capacity, verts,
                                     quads, faces);
      return 0;
    });
  });
  return launch_status();
}

}  // extern "C"
