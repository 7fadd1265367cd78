// seg_bmm.hip - per-segment GEMM over the contiguous rows of a ragged batch (reference: nn/functional/bmm.py, which pads to
// [B, M, Cin], calls torch.bmm and unpads):
//
//   wcn_seg_bmm        y[r, :] = x[r, :] @ W[seg(r)]       W [K, cin, cout]; with transpose_w  y[r, :] = x[r, :] @ W[seg(r)]^T
//   wcn_seg_bmm_wgrad  dW[b]   = X_b^T dY_b                 (rows of segment b)
//
// f32 / f16 / bf16, all operands in one dtype, fp32 accumulation, one rounding.  fp32 runs on v_mfma_f32_16x16x4_f32 (exact
// fp32 operands, an fmaf chain), the half types on v_mfma_f32_16x16x32_{f16,bf16}.  Channel counts from 1 to kBmmMaxC: what
// lies off the 16-wide tiles or the k step is zero in registers, never in memory.
//
// Forward / dX.  A workgroup owns one (segment, tile of kBmmTile rows counted from the segment's first row), so a tile never
// straddles two weights; a wave owns 32 of its rows and walks the output columns 64 at a time, over the whole reduction each
// time.  The reduction order of a row is k-step by k-step and fixed by (cin, cout, dtype) alone: a row's result depends bit for
// bit on that row and its weight.  A lane brings E = 16 B of a row (4 floats / 8 halves): its k's are k0 + E * (lane / 16) + e,
// the weight fragment is read at the same k's (the order of k inside a product is free as long as both operands agree).
//
// dW.  A segment is cut into chunks of kBmmChunk rows counted from its own first row; one workgroup reduces one chunk into an
// fp32 [cin, cout] workspace slot (its waves share the 16 x 64 output blocks), and a second launch adds a segment's slots in
// chunk order and rounds once.  No float atomics; the result does not depend on the launch or on the rest of the batch; a
// segment without rows gets exact zeros.
//
// Neither needs a host read: one workgroup scans ceil(len / tile) into ts [K + 1] (and the chunks into cs), the grid is the
// upper bound ceil(rows / tile) + K, every workgroup bisects the scan and the surplus ones leave at once.  cu comes from the
// device unchecked: spans are clamped to [0, rows], slots to the slots there are.
#include "gather_gemm.h"

namespace wcn {

constexpr int kBmmThreads = 256;
constexpr int kBmmTile = 128;    // rows of a forward workgroup: 4 waves x 2 row tiles of 16
constexpr int kBmmChunk = 512;   // rows of one dW chunk
constexpr int kBmmMaxC = 256;    // channel cap of either side

template <typename T> struct BmmOp;
template <> struct BmmOp<float> {
  static constexpr int E = 4;  // four 16x16x4 products a macro step, product e takes element e of every lane
  static __device__ __forceinline__ f32x4 mma(const float (&a)[4], const float (&b)[4], f32x4 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], c, 0, 0, 0);
    return c;
  }
};
template <typename T> struct BmmOp16 {
  static constexpr int E = 8;  // one 16x16x32 product a macro step
  static __device__ __forceinline__ f32x4 mma(const T (&a)[8], const T (&b)[8], f32x4 c) {
    typename Mfma16<T>::type av, bv;
#pragma unroll
    for (int e = 0; e < 8; ++e) { av[e] = a[e]; bv[e] = b[e]; }
    return Mfma16<T>::mfma(av, bv, c);
  }
};
template <> struct BmmOp<__bf16> : BmmOp16<__bf16> {};
template <> struct BmmOp<_Float16> : BmmOp16<_Float16> {};

// rows [lo, hi) of segment k, inside [0, rows] whatever cu holds
__device__ __forceinline__ void bmm_span(const int32_t* __restrict__ cu, int k, int64_t rows, int64_t& lo, int64_t& hi) {
  lo = cu[k];
  hi = cu[k + 1];
  lo = lo < 0 ? 0 : lo > rows ? rows : lo;
  hi = hi < lo ? lo : hi > rows ? rows : hi;
}

// ts[k] = first tile of segment k, ts[K] = tiles in all; cs the same for the dW chunks (null = not wanted).  ONE workgroup.
__global__ __launch_bounds__(kBmmThreads) void bmm_plan_kernel(const int32_t* __restrict__ cu, int K, int64_t rows,
                                                               int64_t tcap, int64_t ccap, int32_t* __restrict__ ts,
                                                               int32_t* __restrict__ cs) {
  __shared__ int s_wave[kBmmThreads / 64];
  int64_t tcarry = 0, ccarry = 0;
  for (int64_t base = 0; base < K; base += kBmmThreads) {
    const int64_t i = base + threadIdx.x;
    int64_t len = 0;
    if (i < K) {
      int64_t lo, hi;
      bmm_span(cu, (int)i, rows, lo, hi);
      len = hi - lo;
    }
    int tot;
    const int te = block_excl_scan<kBmmThreads>((int)((len + kBmmTile - 1) / kBmmTile), s_wave, &tot);
    if (i < K) {
      const int64_t at = tcarry + te;
      ts[i] = (int32_t)(at < tcap ? at : tcap);
    }
    tcarry += tot;
    __syncthreads();
    if (cs) {
      const int ce = block_excl_scan<kBmmThreads>((int)((len + kBmmChunk - 1) / kBmmChunk), s_wave, &tot);
      if (i < K) {
        const int64_t at = ccarry + ce;
        cs[i] = (int32_t)(at < ccap ? at : ccap);
      }
      ccarry += tot;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    ts[K] = (int32_t)(tcarry < tcap ? tcarry : tcap);
    if (cs) cs[K] = (int32_t)(ccarry < ccap ? ccarry : ccap);
  }
}

// y [rows, cn] = x [rows, ck] @ W'[seg]; W'(k, n) = w[seg * ck * cn + k * wsk + n * wsn]
template <typename T>
__global__ __launch_bounds__(kBmmThreads) void seg_bmm_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                              T* __restrict__ y, const int32_t* __restrict__ cu,
                                                              const int32_t* __restrict__ ts, int K, int64_t rows, int ck,
                                                              int cn, int wsk, int wsn, int xvec) {
  constexpr int E = BmmOp<T>::E;
  const int tile = blockIdx.x;
  if (tile >= ts[K]) return;
  const int b = last_offset_not_above(ts, K, tile);
  int64_t lo, hi;
  bmm_span(cu, b, rows, lo, hi);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, kq = lane >> 4;
  const int64_t w0 = lo + (int64_t)(tile - ts[b]) * kBmmTile + wave * 32;  // the wave's first row
  if (w0 >= hi) return;
  const T* __restrict__ wb = w + (int64_t)b * ck * cn;

  for (int n0 = 0; n0 < cn; n0 += 64) {
    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ck; k0 += 4 * E) {
      const int k = k0 + E * kq;
      T a[2][E];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int64_t row = w0 + rt * 16 + r;
        const bool live = row < hi;
        if (xvec) {  // ck a multiple of E and x 16-B aligned: k < ck means the whole piece is there
          Vec<T, E> v;
#pragma unroll
          for (int e = 0; e < E; ++e) v.v[e] = (T)0.f;
          if (live && k < ck) v = *reinterpret_cast<const Vec<T, E>*>(x + row * ck + k);
#pragma unroll
          for (int e = 0; e < E; ++e) a[rt][e] = v.v[e];
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) a[rt][e] = live && k + e < ck ? x[row * ck + k + e] : (T)0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (n0 + 16 * t >= cn) break;  // wave-uniform
        const int n = n0 + 16 * t + r;
        T bf[E];
#pragma unroll
        for (int e = 0; e < E; ++e) bf[e] = n < cn && k + e < ck ? wb[(int64_t)(k + e) * wsk + (int64_t)n * wsn] : (T)0.f;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc[rt][t] = BmmOp<T>::mma(a[rt], bf, acc[rt][t]);
      }
    }
    // result tile: column lane % 16, rows 4 (lane / 16) + reg
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int n = n0 + 16 * t + r;
        if (n >= cn) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t row = w0 + rt * 16 + 4 * kq + g;
          if (row < hi) y[row * cn + n] = (T)acc[rt][t][g];
        }
      }
  }
}

// part [chunk][cin][cout] = X_chunk^T dY_chunk
template <typename T>
__global__ __launch_bounds__(kBmmThreads) void seg_bmm_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                    float* __restrict__ part, const int32_t* __restrict__ cu,
                                                                    const int32_t* __restrict__ cs, int K, int64_t rows,
                                                                    int cin, int cout) {
  constexpr int E = BmmOp<T>::E;
  const int chunk = blockIdx.x;
  if (chunk >= cs[K]) return;
  const int b = last_offset_not_above(cs, K, chunk);
  int64_t lo, hi;
  bmm_span(cu, b, rows, lo, hi);
  const int64_t c_lo = lo + (int64_t)(chunk - cs[b]) * kBmmChunk;
  const int64_t c_hi = c_lo + kBmmChunk < hi ? c_lo + kBmmChunk : hi;
  float* __restrict__ out = part + (int64_t)chunk * cin * cout;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, kq = lane >> 4;
  const int nti = (cin + 15) / 16, ntj = (cout + 63) / 64;

  for (int item = wave; item < nti * ntj; item += kBmmThreads / 64) {
    const int i0 = (item / ntj) * 16, j0 = (item % ntj) * 64;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ci = i0 + r;
    for (int64_t r0 = c_lo; r0 < c_hi; r0 += 4 * E) {
      const int64_t rr = r0 + E * kq;
      T a[E];
#pragma unroll
      for (int e = 0; e < E; ++e) a[e] = ci < cin && rr + e < c_hi ? x[(rr + e) * cin + ci] : (T)0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (j0 + 16 * t >= cout) break;  // wave-uniform
        const int co = j0 + 16 * t + r;
        T bf[E];
#pragma unroll
        for (int e = 0; e < E; ++e) bf[e] = co < cout && rr + e < c_hi ? dy[(rr + e) * cout + co] : (T)0.f;
        acc[t] = BmmOp<T>::mma(a, bf, acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int co = j0 + 16 * t + r;
      if (co >= cout) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int i = i0 + 4 * kq + g;
        if (i < cin) out[(int64_t)i * cout + co] = acc[t][g];
      }
    }
  }
}

// dW[b] = the segment's slots added in chunk order, rounded once
template <typename T>
__global__ __launch_bounds__(kBmmThreads) void seg_bmm_wgrad_merge_kernel(const float* __restrict__ part,
                                                                          const int32_t* __restrict__ cs, int K, int cells,
                                                                          T* __restrict__ dw) {
  const int b = blockIdx.y;
  const int c0 = cs[b], c1 = cs[b + 1];
  for (int e = blockIdx.x * kBmmThreads + threadIdx.x; e < cells; e += gridDim.x * kBmmThreads) {
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += part[(int64_t)c * cells + e];
    dw[(int64_t)b * cells + e] = (T)s;
  }
}

static size_t bmm_plan_bytes(int64_t num_segs) { return align256((size_t)(num_segs + 1) * sizeof(int32_t)); }

// WCN_SUCCESS, an error, or 1 = valid but nothing to launch
static int bmm_check(int64_t rows, int64_t num_segs, int32_t cin, int32_t cout, int32_t dtype) {
  if (rows < 0 || num_segs < 0 || cin < 1 || cout < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (rows > INT32_MAX || num_segs > 65535) return WCN_ERROR_INVALID_PARAMETERS;  // int32 row offsets; grid.y of the merge
  if (!dtype_ok(dtype) || cin > kBmmMaxC || cout > kBmmMaxC) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return rows == 0 || num_segs == 0 ? 1 : WCN_SUCCESS;
}

}  // namespace wcn

using namespace wcn;

int32_t wcn_seg_bmm_max_channels(void) { return kBmmMaxC; }
int32_t wcn_seg_bmm_tile_rows(void) { return kBmmTile; }
int32_t wcn_seg_bmm_chunk_rows(void) { return kBmmChunk; }

size_t wcn_seg_bmm_workspace_bytes(int64_t rows, int64_t num_segs, int32_t cin, int32_t cout, int32_t wgrad) {
  if (rows <= 0 || num_segs <= 0 || cin < 1 || cout < 1) return 0;
  if (!wgrad) return bmm_plan_bytes(num_segs);
  return 2 * bmm_plan_bytes(num_segs) + (size_t)(ceil_div(rows, kBmmChunk) + num_segs) * (size_t)cin * (size_t)cout * sizeof(float);
}

int wcn_seg_bmm(const void* x, const void* w, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t cin, int32_t cout,
                int32_t transpose_w, int32_t dtype, void* y, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  const int st = bmm_check(rows, num_segs, cin, cout, dtype);
  if (st != WCN_SUCCESS) return st == 1 ? WCN_SUCCESS : st;
  if (!x || !w || !cu || !y || !workspace) return WCN_ERROR_INVALID_PARAMETERS;
  const size_t el = dtype_bytes(dtype);
  if (!aligned_to(x, el) || !aligned_to(w, el) || !aligned_to(y, el) || !aligned_to(cu, 4) || !aligned_to(workspace, 16) ||
      workspace_bytes < wcn_seg_bmm_workspace_bytes(rows, num_segs, cin, cout, 0))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  int32_t* ts = (int32_t*)workspace;
  const int64_t tcap = ceil_div(rows, kBmmTile) + num_segs;
  hipLaunchKernelGGL(bmm_plan_kernel, dim3(1), dim3(kBmmThreads), 0, s, cu, (int)num_segs, rows, tcap, (int64_t)0, ts,
                     (int32_t*)nullptr);
  // the reduction runs over ck, the output over cn; the weight is [cin, cout] either way
  const int ck = transpose_w ? cout : cin, cn = transpose_w ? cin : cout;
  const int wsk = transpose_w ? 1 : cout, wsn = transpose_w ? cout : 1;
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = ck % BmmOp<T>::E == 0 && aligned_to(x, 16);
    hipLaunchKernelGGL(seg_bmm_kernel<T>, dim3((unsigned)tcap), dim3(kBmmThreads), 0, s, (const T*)x, (const T*)w, (T*)y, cu,
                       (const int32_t*)ts, (int)num_segs, rows, ck, cn, wsk, wsn, xvec);
    return 0;
  });
  return launch_status();
}

int wcn_seg_bmm_wgrad(const void* x, const void* dy, const int32_t* cu, int64_t num_segs, int64_t rows, int32_t cin,
                      int32_t cout, int32_t dtype, void* dw, void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  const int st = bmm_check(rows, num_segs, cin, cout, dtype);
  if (st != WCN_SUCCESS && st != 1) return st;
  const size_t el = dtype_bytes(dtype);
  if (num_segs > 0 && (!dw || !aligned_to(dw, el))) return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  if (st == 1) {  // no rows: exact zeros, without a kernel
    const size_t bytes = (size_t)num_segs * (size_t)cin * (size_t)cout * el;
    if (bytes > 0 && hipMemsetAsync(dw, 0, bytes, s) != hipSuccess) return WCN_ERROR_KERNEL_EXECUTION;
    return WCN_SUCCESS;
  }
  if (!x || !dy || !cu || !workspace) return WCN_ERROR_INVALID_PARAMETERS;
  if (!aligned_to(x, el) || !aligned_to(dy, el) || !aligned_to(cu, 4) || !aligned_to(workspace, 16) ||
      workspace_bytes < wcn_seg_bmm_workspace_bytes(rows, num_segs, cin, cout, 1))
    return WCN_ERROR_INVALID_PARAMETERS;
  int32_t* ts = (int32_t*)workspace;
  int32_t* cs = (int32_t*)((char*)workspace + bmm_plan_bytes(num_segs));
  float* part = (float*)((char*)workspace + 2 * bmm_plan_bytes(num_segs));
  const int64_t tcap = ceil_div(rows, kBmmTile) + num_segs, ccap = ceil_div(rows, kBmmChunk) + num_segs;
  hipLaunchKernelGGL(bmm_plan_kernel, dim3(1), dim3(kBmmThreads), 0, s, cu, (int)num_segs, rows, tcap, ccap, ts, cs);
  const int cells = cin * cout;
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(seg_bmm_wgrad_kernel<T>, dim3((unsigned)ccap), dim3(kBmmThreads), 0, s, (const T*)x, (const T*)dy, part, cu,
                       (const int32_t*)cs, (int)num_segs, rows, cin, cout);
    const dim3 mgrid((unsigned)ceil_div(cells, kBmmThreads), (unsigned)num_segs);
    hipLaunchKernelGGL(seg_bmm_wgrad_merge_kernel<T>, mgrid, dim3(kBmmThreads), 0, s, (const float*)part, (const int32_t*)cs,
                       (int)num_segs, cells, (T*)dw);
    return 0;
  });
  return launch_status();
}
