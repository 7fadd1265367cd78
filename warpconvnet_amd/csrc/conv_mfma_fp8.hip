// conv_mfma_fp8.hip - inference sparse convolution on FP8 (OCP E4M3) operands: v_mfma_f32_32x32x64_f8f6f4, fp32 accumulation,
// one rounding to fp16 / bf16 / fp32 ("hip_mfma_fp8", WCN_ALGO_MFMA_FP8).  Forward only.  No float atomics anywhere: two runs
// give the same bits.
//
//   y[m, c] = (s_x * s_w[c]) * sum_k sum_ci Xq[nbr[m][k], ci] * Wq[k, ci, c]  (+ bias[c])
//   Xq = rne_e4m3(x / s_x), s_x = amax|x| / 448 (one scale per tensor); Wq = rne_e4m3(w / s_w[c]), s_w[c] = amax|w[:, :, c]| / 448.
//   A product of two E4M3 values has 8 significant bits and is exact in fp32; the sums are fp32.
//
// ---- quantiser ---------------------------------------------------------------------------------------------------------------
//   fp8_amax_scale_kernel    |x| maximum of a tensor -> *scale.  Every workgroup leaves its partial in the workspace, takes a
//                            ticket (an INTEGER atomic) and the last one reduces the partials in index order; max is exact and
//                            commutative, so the value does not depend on which workgroup is last.  scale = amax / 448, IEEE
//                            division; 1 for an all-zero tensor.  The ticket word is zero before and after.
//   fp8_quant_rows_kernel    out[r][c] = e4m3(x[r][c] / *scale) for c < C, 0 for C <= c < C_pad: rows of C_pad bytes (the pitch
//                            the convolution reads, so there is no padding pass).  16 output bytes per thread.  IEEE division,
//                            not a reciprocal multiply: ties between two E4M3 neighbours have to fall as the framework's cast
//                            of x / scale does.  v_cvt_pk_fp8_f32 is OCP E4M3 on gfx950 and rounds to nearest even, subnormals
//                            included; |x / scale| <= 448 (1 + 2^-22) < 464, so nothing it is given overflows.
//   fp8_weight_scale_kernel  s_w[c] for 32 output channels per workgroup: 8 row strands per channel, LDS tree in a fixed order.
//   fp8_weight_pack_kernel   the weight image below from the plain [K, cin, cout] tensor (zero bytes for padded channels).
//
// ---- weight image ------------------------------------------------------------------------------------------------------------
//   One B fragment = (offset k, 64-channel chunk q, 32-column block cb) = 2 KiB = [j = 0, 1][lane = 32 h + n][16 bytes b]:
//     byte = Wq[k][64 q + 32 h + 16 j + b][32 cb + n]
//   fragments in the order [k][q][cb].  A wave reads a fragment as two global_load_dwordx4, 1 KiB of consecutive bytes each.
//   The order of the reduction inside an MFMA is free as long as A and B agree (the hardware maps byte i of lane half h of A and
//   of B to the same k index), so the A operand of lane (h, n) is bytes 32 h + 16 j + b of the 64-byte piece of row n: two whole
//   ds_read_b128 of consecutive addresses.
//
// ---- gather GEMM (gather_gemm_fp8_kernel) --------------------------------------------------------------------------------------
//   * why 32x32x64: a 64-channel step of a 32 x 32 block is ONE instruction of 16 passes (64 cycles, 131 072 flop) where
//     v_mfma_f32_32x32x16_fp8_fp8 takes four of 8 passes and the bf16 32x32x16 chain four of 8: half the matrix-core time per
//     step.  Cin is a multiple of 64 after padding, so there is one shape class.  (Pass counts: from the published peak rates
//     of the part - 2x the 16-bit rate for the f8f6f4 instruction, 1x for the x16 fp8 one - and the LLVM AMDGPU scheduling
//     model; not timed here.)
//   * tile: 256 threads own 128 output rows (through the mask-sorted permutation) x CB = 32 NCW columns; grid.y walks the
//     column blocks.  NCW = 4 (cout % 128 == 0): wave w owns columns 32 w .. + 31 of ALL four 32-row blocks - four accumulators,
//     one B fragment feeds four MFMAs.  NCW = 2 (cout % 64 == 0): two column waves x two row halves.  NCW = 1: one row block per
//     wave, one column block; cout = 96, 160 run as 32-wide blocks (each gathers its rows again).
//   * step = (offset k, 64-channel chunk).  Rows: FOUR adjacent lanes move the 64-B piece of a row (16 B each), 64 rows per
//     pass, two passes; an absent neighbour issues no load and stores zeros.  Registers first, LDS after the MFMAs of the step
//     before: loads of step s + 1 fly under the MFMAs of step s; two LDS stages, one barrier a step.  (LDS-DMA cannot write a
//     padded pitch.)  Weights never touch LDS: each wave loads its fragment L2 -> VGPR one step ahead (two register buffers).
//   * LDS pitch 80 B = 20 words (64 banks of 4 B; a 16-B read is served 16 lanes at a time).  The 16 lanes of a pass read rows
//     n .. n + 15 at one byte offset: first bank (20 n + c) % 64 = 4 (5 n % 16) + c, and 5 n % 16 is a permutation of 0 .. 15 -
//     sixteen disjoint 4-bank groups, every bank once.  (Any pitch of 4 * odd words; 20 is the smallest above 16.)  The
//     commits are NOT conflict-free: 16 lanes write 4 rows x 4 pieces, first banks 20 r + 4 p, and (r, p) = (3, 1) meets (0, 0)
//     and so on - 2-way on 6 of 16 pieces; there is one commit for NCW reads of a row.  Derived, not measured with a counter.
//   * a wave skips the MFMA of a row block none of whose rows has the offset, the workgroup skips the step of an offset none
//     of its rows has (gather_gemm.h); K > 32 runs one pass per mask word.
//   * epilogue: lane (h, n) holds column n of rows 8 v + 4 h + q of a block: acc * (s_x * s_w[col]) + bias[col] in fp32, one
//     rounding, 32 lanes store one 32-column row piece (128 B fp32, 64 B 16-bit) - with NCW = 4 the four waves write the four
//     pieces of a 128-column row.
//
// Shapes: cin % 64 == 0, cout % 32 == 0, any K <= 4096 (the caller zero-pads everything else).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch must stay 0) is in
// DESIGN.md 4.36.
#include "gather_gemm.h"

namespace wcn {

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int kCIC = 64;        // reduction channels (= bytes of a row piece) per step
constexpr int kPitch = 80;      // bytes: LDS pitch of a staged row piece (see the header)
constexpr int kTile = 128;      // output rows per workgroup
constexpr int kWordCols = 32;   // table columns per mask word
constexpr float kE4M3Max = 448.f;
constexpr int kAmaxBlocks = 256;  // partials of the tensor-wide maximum

// cbsz = blgp = 0: E4M3 for both operands; scale arguments constant 0: the unscaled instruction
__device__ __forceinline__ f32x16 mfma_fp8(i32x8 a, i32x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}

// four floats -> four E4M3 bytes (ascending addresses), round to nearest even
__device__ __forceinline__ uint32_t pack_e4m3(float a, float b, float c, float d) {
  int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  return (uint32_t)v;
}

__device__ __forceinline__ float block_max_256(float m, float* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// ---- quantiser ---------------------------------------------------------------------------------------------------------------
// ws: [kAmaxBlocks] partials (float bits), then the ticket word
template <typename T>
__global__ __launch_bounds__(256) void fp8_amax_scale_kernel(const T* __restrict__ x, int64_t count, uint32_t* __restrict__ ws,
                                                             float* __restrict__ scale) {
  __shared__ float s_red[4];
  __shared__ int s_last;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf((float)x[i]));
  m = block_max_256(m, s_red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&ws[blockIdx.x], __float_as_uint(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    s_last = atomicAdd(&ws[kAmaxBlocks], 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  float p = 0.f;
  if (threadIdx.x < gridDim.x)
    p = __uint_as_float(__hip_atomic_load(&ws[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();  // s_red is rewritten
  p = block_max_256(p, s_red);
  if (threadIdx.x == 0) {
    *scale = p == 0.f ? 1.f : p / kE4M3Max;
    ws[kAmaxBlocks] = 0u;
  }
}

// one thread: 16 bytes of an output row
template <typename T>
__global__ __launch_bounds__(256) void fp8_quant_rows_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                             uint8_t* __restrict__ out, int64_t n, int c, int c_pad) {
  const int per_row = c_pad / 16;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * per_row) return;
  const int64_t r = e / per_row;
  const int c0 = (int)(e - r * per_row) * 16;
  const float s = *scale;
  const T* src = x + r * c + c0;
  uint4 o;
  uint32_t* ow = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (c % 4 == 0) {  // (uniform) whole 4-element pieces, aligned
      if (c0 + 4 * g < c) ld_vec<T, 4>(src + 4 * g, f);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + 4 * g + q < c) f[q] = (float)src[4 * g + q];
    }
    ow[g] = pack_e4m3(f[0] / s, f[1] / s, f[2] / s, f[3] / s);
  }
  *reinterpret_cast<uint4*>(out + r * c_pad + c0) = o;
}

// s_w of 32 output channels per workgroup; w [rows = K * cin][cout]; channels >= cout (padding) get 1
template <typename T>
__global__ __launch_bounds__(256) void fp8_weight_scale_kernel(const T* __restrict__ w, int64_t rows, int cout,
                                                               float* __restrict__ w_scale) {
  __shared__ float s_m[8][32];
  const int n = threadIdx.x & 31, strand = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + n;
  float m = 0.f;
  if (col < cout)
    for (int64_t r = strand; r < rows; r += 8) m = fmaxf(m, fabsf((float)w[r * cout + col]));
  s_m[strand][n] = m;
  __syncthreads();
  if (strand == 0) {
#pragma unroll
    for (int q = 1; q < 8; ++q) m = fmaxf(m, s_m[q][n]);
    w_scale[col] = m == 0.f ? 1.f : m / kE4M3Max;
  }
}

// one thread: 16 bytes of the image = 16 consecutive input channels of one output column
template <typename T>
__global__ __launch_bounds__(256) void fp8_weight_pack_kernel(const T* __restrict__ w, const float* __restrict__ w_scale,
                                                              uint8_t* __restrict__ image, int K, int cin, int cout, int cin_p,
                                                              int cout_p) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // 16-B piece of the image
  if (e >= (int64_t)K * cin_p * cout_p / 16) return;
  const int lane = (int)(e & 63), j = (int)((e >> 6) & 1);
  int64_t frag = e >> 7;
  const int nb = cout_p / 32, nq = cin_p / kCIC;
  const int cb = (int)(frag % nb);
  frag /= nb;
  const int q = (int)(frag % nq), k = (int)(frag / nq);
  const int col = 32 * cb + (lane & 31), ci0 = kCIC * q + 32 * (lane >> 5) + 16 * j;
  const float s = w_scale[col];
  float f[16];
#pragma unroll
  for (int b = 0; b < 16; ++b)
    f[b] = (col < cout && ci0 + b < cin) ? (float)w[((int64_t)k * cin + ci0 + b) * cout + col] / s : 0.f;
  uint4 o;
  o.x = pack_e4m3(f[0], f[1], f[2], f[3]);
  o.y = pack_e4m3(f[4], f[5], f[6], f[7]);
  o.z = pack_e4m3(f[8], f[9], f[10], f[11]);
  o.w = pack_e4m3(f[12], f[13], f[14], f[15]);
  reinterpret_cast<uint4*>(image)[e] = o;
}

// ---- gather GEMM -------------------------------------------------------------------------------------------------------------
// NCW waves along the columns (32 each); a wave owns NCW of the tile's four 32-row blocks
template <int NCW, typename TO>
__global__ __launch_bounds__(256) void gather_gemm_fp8_kernel(const uint8_t* __restrict__ xq, const float* __restrict__ x_scale,
                                                              const uint8_t* __restrict__ wq, const float* __restrict__ w_scale,
                                                              TO* __restrict__ out, const int32_t* __restrict__ nbr,
                                                              const uint32_t* __restrict__ mask, const int32_t* __restrict__ perm,
                                                              const float* __restrict__ bias, int64_t n_out, int cin, int cout,
                                                              int kp, int mw) {
  __shared__ __attribute__((aligned(16))) uint8_t s_stage[2][kTile * kPitch];
  __shared__ int32_t s_nbr[kTile * kWordCols];  // the columns of one mask word
  __shared__ int32_t s_rows[kTile];
  __shared__ uint32_t s_wmask[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, n = lane & 31;
  const int wc = wave % NCW, rb0 = (wave / NCW) * NCW;  // the wave's column slice and first row block
  const int nchunk = cin / kCIC, nb = cout / 32;
  const int cb = blockIdx.y * NCW + wc;                 // 32-column block of the output
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int piece = tid & 3, prow = tid >> 2;           // row gather: 4 lanes a row piece

  stage_row_ids<kTile>(s_rows, perm, row0, n_out);
  __syncthreads();

  f32x16 acc[NCW];
#pragma unroll
  for (int i = 0; i < NCW; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

  for (int word = 0; word < mw; ++word) {
    const int kbase = word * kWordCols;
    const int kpw = (kp - kbase) < kWordCols ? (kp - kbase) : kWordCols;
    uint32_t my_mask = 0;
    if (tid < kTile) {
      const int32_t r = s_rows[tid];
      if (r >= 0) my_mask = mask[(int64_t)r * mw + word];
    }
    for (int e = tid; e < kTile * kpw; e += 256) {
      const int i = e / kpw, c = e - i * kpw;
      const int32_t r = s_rows[i];
      s_nbr[i * kWordCols + c] = r >= 0 ? nbr[(int64_t)r * kp + kbase + c] : -1;
    }
    if (tid < 4) s_wmask[tid] = 0;
    __syncthreads();
    or_row_mask<kTile, 32>(s_wmask, my_mask);
    __syncthreads();
    uint32_t rb_mask[NCW];
#pragma unroll
    for (int i = 0; i < NCW; ++i) rb_mask[i] = __builtin_amdgcn_readfirstlane(s_wmask[rb0 + i]);
    const uint32_t block_mask = tile_mask<4>(s_wmask);

    if (block_mask != 0u) {
      uint4 ra[2];
      i32x8 b_cur, b_next;
      // row pieces and the wave's weight fragment of step (k, chunk) -> registers
      auto fetch = [&](int k, int chunk, i32x8& b) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int32_t idx = s_nbr[(prow + 64 * i) * kWordCols + k];
          ra[i] = make_uint4(0u, 0u, 0u, 0u);
          if (idx >= 0) ra[i] = *reinterpret_cast<const uint4*>(xq + (int64_t)idx * cin + chunk * kCIC + piece * 16);
        }
        const uint8_t* f = wq + ((((int64_t)(kbase + k) * nchunk + chunk) * nb + cb) * 128 + lane) * 16;
        const int4 lo = *reinterpret_cast<const int4*>(f), hi = *reinterpret_cast<const int4*>(f + 1024);
        b = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      };
      auto commit = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(&s_stage[buf][(prow + 64 * i) * kPitch + piece * 16]) = ra[i];
      };
      auto compute = [&](int buf, int k, const i32x8& b) {
#pragma unroll
        for (int i = 0; i < NCW; ++i) {
          if (!((rb_mask[i] >> k) & 1u)) continue;  // wave-uniform: none of the block's rows has the offset
          const uint8_t* sa = &s_stage[buf][((rb0 + i) * 32 + n) * kPitch + 32 * h];
          const int4 lo = *reinterpret_cast<const int4*>(sa), hi = *reinterpret_cast<const int4*>(sa + 16);
          acc[i] = mfma_fp8(i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}, b, acc[i]);
        }
      };
      StepIter steps{block_mask, nchunk};
      int k = -1, c = 0, buf = 0;
      steps.next(k, c);
      fetch(k, c, b_cur);
      commit(0);
      __syncthreads();
      for (;;) {
        int k2 = k, c2 = c;
        const bool has = steps.next(k2, c2);
        if (has) fetch(k2, c2, b_next);  // in flight under the MFMAs below
        compute(buf, k, b_cur);
        if (!has) break;
        commit(buf ^ 1);                 // last read before the barrier of the step before
        __syncthreads();
        buf ^= 1; k = k2; c = c2; b_cur = b_next;
      }
    }
    __syncthreads();  // stages, index slab and mask words are rewritten by the next pass
  }

  const int col = 32 * cb + n;
  const float sc = *x_scale * w_scale[col];
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int i = 0; i < NCW; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int32_t r = s_rows[(rb0 + i) * 32 + 8 * v + 4 * h + q];
        if (r >= 0) out[(int64_t)r * cout + col] = (TO)(acc[i][4 * v + q] * sc + bv);
      }
}

template <int NCW>
int launch_gather_fp8(const void* xq, const float* x_scale, const void* wq, const float* w_scale, void* out, const int32_t* nbr,
                      const uint32_t* mask, const int32_t* perm, const float* bias, int64_t n_out, int cin, int cout, int K,
                      int out_dtype, hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(n_out, kTile), (unsigned)(cout / (32 * NCW)));
  return with_dtype(out_dtype, [&](auto t) {
    typedef decltype(t) TO;
    hipLaunchKernelGGL((gather_gemm_fp8_kernel<NCW, TO>), grid, dim3(256), 0, s, (const uint8_t*)xq, x_scale, (const uint8_t*)wq,
                       w_scale, (TO*)out, nbr, mask, perm, bias, n_out, cin, cout, wcn_kmap_row_pitch(K), wcn_kmap_mask_words(K));
    return launch_status();
  });
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool conv_fp8_supported(int cin, int cout, int K) {
  return cin >= 64 && cin % 64 == 0 && cin <= (1 << 20) && cout >= 32 && cout % 32 == 0 && cout / 32 <= 65535 && valid_k(K);
}
size_t fp8_packed_weight_bytes(int K, int cin, int cout) { return (size_t)K * cin * cout; }
size_t fp8_amax_workspace() { return (kAmaxBlocks + 1) * sizeof(uint32_t); }

int fp8_amax_scale(const void* x, int64_t count, int dtype, void* workspace, float* scale, hipStream_t s) {
  const unsigned blocks = (unsigned)(count < 1 ? 1 : ceil_div(count, 256 * 16) < kAmaxBlocks ? ceil_div(count, 256 * 16) : kAmaxBlocks);
  return with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(fp8_amax_scale_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)x, count, (uint32_t*)workspace, scale);
    return launch_status();
  });
}

int fp8_quantize_rows(const void* x, int64_t n, int c, int dtype, const float* scale, void* out, int c_pad, hipStream_t s) {
  const int64_t pieces = n * (c_pad / 16);
  if (ceil_div(pieces, 256) > 0x7fffffff) return WCN_ERROR_INVALID_PARAMETERS;
  return with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(fp8_quant_rows_kernel<T>, dim3((unsigned)ceil_div(pieces, 256)), dim3(256), 0, s, (const T*)x, scale,
                       (uint8_t*)out, n, c, c_pad);
    return launch_status();
  });
}

int fp8_pack_weight(const void* w, int K, int cin, int cout, int dtype, int cin_p, int cout_p, void* image, float* w_scale,
                    hipStream_t s) {
  return with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(fp8_weight_scale_kernel<T>, dim3(cout_p / 32), dim3(256), 0, s, (const T*)w, (int64_t)K * cin, cout, w_scale);
    const int64_t pieces = (int64_t)K * cin_p * cout_p / 16;
    hipLaunchKernelGGL(fp8_weight_pack_kernel<T>, dim3((unsigned)ceil_div(pieces, 256)), dim3(256), 0, s, (const T*)w, w_scale,
                       (uint8_t*)image, K, cin, cout, cin_p, cout_p);
    return launch_status();
  });
}

int conv_gather_gemm_fp8(const void* xq, const float* x_scale, const void* wq, const float* w_scale, void* out, const int32_t* nbr,
                         const uint32_t* mask, const int32_t* perm, const float* bias, int64_t n_out, int cin, int cout, int K,
                         int out_dtype, hipStream_t s) {
  if (ceil_div(n_out, kTile) > 0x7fffffff) return WCN_ERROR_INVALID_PARAMETERS;
  if (cout % 128 == 0)
    return launch_gather_fp8<4>(xq, x_scale, wq, w_scale, out, nbr, mask, perm, bias, n_out, cin, cout, K, out_dtype, s);
  if (cout % 64 == 0)
    return launch_gather_fp8<2>(xq, x_scale, wq, w_scale, out, nbr, mask, perm, bias, n_out, cin, cout, K, out_dtype, s);
  return launch_gather_fp8<1>(xq, x_scale, wq, w_scale, out, nbr, mask, perm, bias, n_out, cin, cout, K, out_dtype, s);
}

}  // namespace wcn
