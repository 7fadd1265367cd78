// pad.hip - ragged row repack between the three layouts of a batch of K segments of rows (reference:
// geometry/features/ops/convert.py, features/batch_copy.py, features/patch.py, which loop over the batch in Python with one
// device read per element).  Every layout gives segment b a first row and the same length len_b = cu[b + 1] - cu[b]:
//
//   cat    first row cu[b]                 rows = cu[K]
//   pad    first row b * M                 rows = K * M
//   patch  first row patch_offsets[b]      rows = patch_offsets[K]
//
// A layout is (starts, pitch): `starts` int32 [K + 1] on the device (cu or patch_offsets), or null with the pitch M.  ONE
// kernel serves every ordered pair: a thread owns one piece of one DESTINATION row, finds the row's segment (a division for
// pad, a bisection of `starts` otherwise) and its place j in it, and writes the source row's piece if j < len_b, the fill
// otherwise.  Every destination piece is written exactly once: no prior zero fill, no atomics, nothing depends on the launch.
// With src null it is the fill-only pass of clear_padding: rows with j < len_b are left alone.
//
// It is a byte copy: rows of `row_bytes` bytes of elements of 1, 2, 4 or 8 bytes, moved in the widest piece of 16, 8, 4, 2
// or 1 bytes that divides the row and that both pointers are aligned to.  The offsets come from the device unchecked: a
// source row outside [0, src_rows) reads nothing and gives the fill.
#include "row_lists.h"

namespace wcn {

constexpr int kPadThreads = 256;

struct PadLayout {
  const int32_t* starts;  // [K + 1] or null
  int64_t pitch;          // rows of a segment's slot when starts is null
  int64_t rows;           // rows of the tensor
};

struct PadArgs {
  const void* src;  // null: fill only
  void* dst;
  const int32_t* cu;
  PadLayout s, d;
  int64_t items;  // dst rows * pieces
  int pieces;     // row_bytes / PB
  int num_segs;
  uint64_t fill[2];  // the fill element repeated over 16 bytes
};

template <int PB>
__global__ __launch_bounds__(kPadThreads) void pad_repack_kernel(const PadArgs p) {
  typedef Vec<uint8_t, PB> Piece;
  const Piece* __restrict__ src = (const Piece*)p.src;
  Piece* __restrict__ dst = (Piece*)p.dst;
  const int K = p.num_segs;
  Piece fill;
  {
    const uint8_t* fb = (const uint8_t*)p.fill;
#pragma unroll
    for (int i = 0; i < PB; ++i) fill.v[i] = fb[i];
  }
  for (int64_t it = (int64_t)blockIdx.x * kPadThreads + threadIdx.x; it < p.items; it += (int64_t)gridDim.x * kPadThreads) {
    const int64_t row = it / p.pieces;
    const int piece = (int)(it - row * p.pieces);
    int b;
    int64_t first;
    if (p.d.starts) {
      b = last_offset_not_above(p.d.starts, K, row);
      first = p.d.starts[b];
    } else {
      const int64_t q = row / p.d.pitch;
      b = (int)(q < K ? q : K - 1);
      first = (int64_t)b * p.d.pitch;
    }
    const int64_t j = row - first;
    const int64_t len = (int64_t)p.cu[b + 1] - (int64_t)p.cu[b];
    const bool inside = j >= 0 && j < len;
    if (!src) {
      if (!inside) dst[it] = fill;
      continue;
    }
    Piece v = fill;
    if (inside) {
      const int64_t sr = (p.s.starts ? (int64_t)p.s.starts[b] : (int64_t)b * p.s.pitch) + j;
      if (sr >= 0 && sr < p.s.rows) v = src[sr * p.pieces + piece];
    }
    dst[it] = v;
  }
}

static bool pad_layout_ok(const int32_t* starts, int64_t pitch, int64_t rows, int64_t num_segs) {
  if (rows < 0 || !aligned_to(starts, 4)) return false;
  if (!starts && (pitch < 0 || rows != num_segs * pitch)) return false;
  return true;
}

}  // namespace wcn

using namespace wcn;

int32_t wcn_pad_max_grid(void) { return kRowMaxGrid; }
int32_t wcn_pad_block_threads(void) { return kPadThreads; }

int wcn_pad_repack(const void* src, void* dst, const int32_t* cu, int64_t num_segs, const int32_t* src_starts, int64_t src_pitch,
                   int64_t src_rows, const int32_t* dst_starts, int64_t dst_pitch, int64_t dst_rows, int64_t row_bytes,
                   int32_t elem_bytes, uint64_t fill_bits, wcn_stream_t stream) {
  if (num_segs < 0 || num_segs > INT32_MAX || row_bytes < 1 || row_bytes > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (row_bytes % elem_bytes != 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (!pad_layout_ok(dst_starts, dst_pitch, dst_rows, num_segs)) return WCN_ERROR_INVALID_PARAMETERS;
  if (src && !pad_layout_ok(src_starts, src_pitch, src_rows, num_segs)) return WCN_ERROR_INVALID_PARAMETERS;
  if (dst_rows > INT32_MAX || (src && src_rows > INT32_MAX)) return WCN_ERROR_INVALID_PARAMETERS;  // int32 starts
  if (dst_rows == 0) return WCN_SUCCESS;
  if (num_segs == 0) return WCN_ERROR_INVALID_PARAMETERS;  // rows without a segment to own them
  if (!dst || !cu || !aligned_to(cu, 4) || !aligned_to(dst, elem_bytes) || !aligned_to(src, elem_bytes))
    return WCN_ERROR_INVALID_PARAMETERS;

  int pb = 16;
  while (pb > elem_bytes && (row_bytes % pb != 0 || !aligned_to(dst, pb) || !aligned_to(src, pb))) pb >>= 1;

  PadArgs a;
  a.src = src;
  a.dst = dst;
  a.cu = cu;
  a.s = PadLayout{src_starts, src_pitch, src_rows};
  a.d = PadLayout{dst_starts, dst_pitch, dst_rows};
  a.pieces = (int)(row_bytes / pb);
  a.items = dst_rows * a.pieces;
  a.num_segs = (int)num_segs;
  uint64_t pattern = 0;  // little endian: byte i of the pattern is byte i % elem_bytes of the element
  for (int i = 0; i < 8; ++i) pattern |= ((fill_bits >> (8 * (i % elem_bytes))) & 0xffull) << (8 * i);
  a.fill[0] = a.fill[1] = pattern;

  const dim3 grid(capped_grid(ceil_div(a.items, kPadThreads))), block(kPadThreads);
  hipStream_t s = (hipStream_t)stream;
  switch (pb) {
    case 16: hipLaunchKernelGGL(pad_repack_kernel<16>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(pad_repack_kernel<8>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(pad_repack_kernel<4>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(pad_repack_kernel<2>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(pad_repack_kernel<1>, grid, block, 0, s, a); break;
  }
  return launch_status();
}
