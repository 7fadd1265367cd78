// conv_mfma_f32.hip - the three sparse-conv products on TRUE fp32 operands: v_mfma_f32_32x32x2_f32, fp32 accumulation,
// fp32 results ("hip_mfma_f32", WCN_ALGO_MFMA_F32).  No float atomics anywhere: two runs give the same bits.
//
// Why 32x32x2: one instruction does 2048 MACs on the 64 + 64 operand values the lanes supply, 16x16x4 half that.  What an
// fp32 MFMA loop pays for is the LDS -> register traffic per flop, so the larger shape.
//
// ---- forward / dgrad gather-GEMM (gather_gemm_f32_kernel) ------------------------------------------------------------------
//   out[r] = sum_k in[nbr[r][k]] . W[k'] (+ bias), k' = k or K - 1 - k (k_flip); W[k'] is the weight AS STORED: [cin, cout]
//   row-major, or [cout, cin] with w_transposed (the dgrad reads the forward tensor down its columns).  No packed image, no
//   pack launch, nothing to cache (csrc/dense_rows.hip is the precedent).
//   * tile: 256 threads own TILE output rows (through the mask-sorted permutation) x CB output columns, grid.y walks the
//     column blocks.  CB = 128 (cout % 128 == 0; TILE 64: wave = 32 rows x 64 columns, two accumulators), 64 (cout % 64 == 0;
//     TILE 64: 32 x 32 per wave) or 32 (TILE 128: four row blocks).  A column block gathers its rows again - cout = 96 runs
//     as three 32-wide blocks.
//   * step = (offset k, 64-channel chunk of the reduction; the last chunk may hold 16, 32 or 48).  The rows of a step are
//     gathered by GROUPS OF 16 LANES PER ROW - sixteen 16-B loads, one 256-B row piece, coalesced - never one lane per row;
//     the weight slab of the step is read the same way, whole rows of it.  Both go to registers first and to LDS after the
//     MFMAs of the step before: the loads of step s + 1 are in flight under the MFMAs of step s, two LDS stages, one barrier a
//     step.  (LDS-DMA cannot write a padded pitch: one instruction fills 1 KiB of consecutive LDS.)
//   * fragments: lane l = 32 h + n of the A operand holds A[row n][k = h].  The order of the reduction is free, so of the
//     eight channels 8 j .. 8 j + 7 half-wave h owns 8 j + 4 h .. + 3: ONE 16-B LDS read feeds four consecutive MFMAs
//     (MFMA e multiplies channels 8 j + e and 8 j + 4 + e).  The B operand uses the same assignment: with w_transposed its
//     four values are one 16-B read too, forward they are four 4-B reads of rows 8 j + 4 h + e at column n.
//   * LDS pitches (64 banks of 4 B; a 16-B read is served 16 lanes at a time, a 4-B read 64 lanes at a time):
//       rows [TILE][64] and transposed slab [CB][64]: pitch 68 floats.  The 16 lanes of a pass read rows n .. n + 15 at one
//         channel offset: bank (68 n + c) % 64 = (4 n + c) % 64 - sixteen 4-bank groups, all 64 banks once.  (Any pitch
//         4 * odd does it; 68 is the smallest above 64.)
//       forward slab [64][CB]: pitch CB + 8 floats.  32 lanes of a half-wave read 32 consecutive columns of one row = 32
//         consecutive banks; the other half-wave reads 4 rows further down: 4 (CB + 8) % 64 = 32, the other 32 banks.
//     One stage = TILE * 68 + max(64 (CB + 8), 68 CB) floats: 52 224 B at CB = 128; two stages + index slab = 112 960 B of
//     the 160 KiB, one workgroup per CU.
//   * a wave skips the MFMAs of an offset none of its 32 rows has, the workgroup skips the step of an offset none of its
//     rows has (stage_row_ids / or_row_mask / tile_mask / StepIter of gather_gemm.h); K > 32 runs one pass per mask word.
//   * epilogue: lane (h, n) holds column n of rows 8 v + 4 h + q of its block: a store instruction writes two 128-B row
//     pieces, straight from the accumulators, + bias[column].
//
// ---- weight gradient (wgrad_f32_kernel + wgrad_f32_reduce_kernel) ----------------------------------------------------------
//   dw[k] = sum_{p in bucket k} x[in_maps[p]]^T . dy[out_maps[p]].  With 32x32x2 the A fragment is x[pair 2 s + h][ci n] and
//   the B fragment dy[pair 2 s + h][co n]: plain row reads of the staged rows, no transpose; one MFMA consumes two pairs.
//   * a workgroup owns (pair range g of the global pair list, one 64 x 128 block of the [cin, cout] plane: four waves =
//     2 x 2 sub-tiles of 32 x 64).  kWgradRanges ranges of equal length (a multiple of the 32-pair step; the length comes
//     from offsets[K] on the device, no host sync).  Steps of 32 pairs, rows through registers into two LDS stages as above.
//   * a range may span several buckets: the partial tile is flushed to workspace slab (g + k) when the bucket changes.  Slab
//     ids are unique; the reduce kernel adds the slabs of bucket k in ascending g and writes zeros for an empty bucket.  The
//     result does not depend on timing.
//   * LDS pitch: x rows 96 floats, dy rows 160: both % 64 == 32, so the two half-waves (pairs 2 s and 2 s + 1, 32 consecutive
//     channels each) hit disjoint halves of the 64 banks.  Two stages: 65 536 B, two workgroups per CU.
//
// Shapes: cin % 16 == 0, cout % 32 == 0, any K (the caller zero-pads everything else).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch must stay 0):
//   kernel                                   VGPRs  AGPRs  SGPRs  scratch  LDS (dynamic)  workgroups / CU (LDS-bound)
//   gather_gemm_f32_kernel<2, 2, false>      130    32     78     0        112 960 B      1
//   gather_gemm_f32_kernel<2, 2, true>       120    32     64     0        112 960 B      1
//   gather_gemm_f32_kernel<1, 2, false>       88    16     70     0         80 192 B      2
//   gather_gemm_f32_kernel<1, 2, true>        84    16     64     0         80 192 B      2
//   gather_gemm_f32_kernel<1, 1, false>       82    16     66     0        107 072 B      1
//   gather_gemm_f32_kernel<1, 1, true>        82    16     64     0        107 072 B      1
//   wgrad_f32_kernel                         136    32    106     0         65 536 B      2
//   wgrad_f32_reduce_kernel                   14     0     26     0              0        8 waves / SIMD
// (the registers alone would allow 3 - 4 waves per SIMD; the LDS stages decide)
#include "gather_gemm.h"

namespace wcn {

namespace {

constexpr int kCIC = 64;        // reduction channels per step
constexpr int kPitchA = 68;     // floats: gathered rows and the transposed weight slab (see the header)
constexpr int kWordCols = 32;   // table columns per mask word

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// NB 32-column blocks per wave, WC waves along the columns
template <int NB, int WC>
struct GatherF32 {
  static constexpr int CB = 32 * NB * WC;            // columns per workgroup
  static constexpr int RBW = 4 / WC;                 // 32-row blocks per workgroup
  static constexpr int TILE = 32 * RBW;
  static constexpr int PITCH_W = CB + 8;             // forward slab
  static constexpr int A_FLOATS = TILE * kPitchA;
  static constexpr int W_FLOATS = kCIC * PITCH_W > CB * kPitchA ? kCIC * PITCH_W : CB * kPitchA;
  static constexpr int STAGE_FLOATS = A_FLOATS + W_FLOATS;
  static constexpr int A_VEC = TILE / 16;            // 16-B pieces per thread and step: rows
  static constexpr int W_VEC = CB / 16;              //                                  weight slab
  static constexpr size_t LDS_BYTES = 2 * (size_t)STAGE_FLOATS * 4 + (size_t)TILE * kWordCols * 4 + (size_t)TILE * 4 + 64;
};

template <int NB, int WC, bool WT>
__global__ __launch_bounds__(256) void gather_gemm_f32_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                              float* __restrict__ out, const int32_t* __restrict__ nbr,
                                                              const uint32_t* __restrict__ mask,
                                                              const int32_t* __restrict__ perm, const float* __restrict__ bias,
                                                              int64_t n_out, int cin, int cout, int K, int kp, int mw,
                                                              int k_flip) {
  typedef GatherF32<NB, WC> G;
  constexpr int CB = G::CB, RBW = G::RBW, TILE = G::TILE, PW = G::PITCH_W;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_stage = reinterpret_cast<float*>(smem);                               // [2][rows | slab]
  int32_t* s_nbr = reinterpret_cast<int32_t*>(s_stage + 2 * G::STAGE_FLOATS);    // [TILE][32]: the columns of one mask word
  int32_t* s_rows = s_nbr + TILE * kWordCols;                                    // [TILE]
  uint32_t* s_wmask = reinterpret_cast<uint32_t*>(s_rows + TILE);                // [RBW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, n = lane & 31;
  const int rb = wave % RBW, wc = wave / RBW;      // the wave's row block and column share
  const int nchunk = (cin + kCIC - 1) / kCIC;
  const int64_t row0 = (int64_t)blockIdx.x * TILE;
  const int co0 = blockIdx.y * CB;
  const int piece = tid & 15, prow = tid >> 4;     // row gather: 16 lanes a row

  stage_row_ids<TILE>(s_rows, perm, row0, n_out);
  __syncthreads();

  f32x16 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;

  for (int word = 0; word < mw; ++word) {
    const int kbase = word * kWordCols;
    const int kpw = (kp - kbase) < kWordCols ? (kp - kbase) : kWordCols;
    uint32_t my_mask = 0;
    if (tid < TILE) {
      const int32_t r = s_rows[tid];
      if (r >= 0) my_mask = mask[(int64_t)r * mw + word];
    }
    for (int e = tid; e < TILE * kpw; e += 256) {
      const int i = e / kpw, c = e - i * kpw;
      const int32_t r = s_rows[i];
      s_nbr[i * kWordCols + c] = r >= 0 ? nbr[(int64_t)r * kp + kbase + c] : -1;
    }
    if (tid < RBW) s_wmask[tid] = 0;
    __syncthreads();
    or_row_mask<TILE, 32>(s_wmask, my_mask);
    __syncthreads();
    const uint32_t rb_mask = __builtin_amdgcn_readfirstlane(s_wmask[rb]);
    const uint32_t block_mask = tile_mask<RBW>(s_wmask);

    if (block_mask != 0u) {
      float4 ra[G::A_VEC], rw[G::W_VEC];
      // rows and weight slab of step (k, chunk) -> registers
      auto fetch = [&](int k, int chunk) {
        const int c0 = chunk * kCIC;
        const int cw = cin - c0 < kCIC ? cin - c0 : kCIC;
#pragma unroll
        for (int i = 0; i < G::A_VEC; ++i) {
          const int32_t idx = s_nbr[(prow + 16 * i) * kWordCols + k];
          ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (idx >= 0 && piece * 4 < cw) ra[i] = *reinterpret_cast<const float4*>(in + (int64_t)idx * cin + c0 + piece * 4);
        }
        const int kw = k_flip ? K - 1 - (kbase + k) : kbase + k;
#pragma unroll
        for (int i = 0; i < G::W_VEC; ++i) {
          const int e = tid + 256 * i;
          rw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (WT) {  // [cout][cin]: CB rows of this column block, the chunk's channels of each
            const int row = e >> 4, p = e & 15;
            if (p * 4 < cw) rw[i] = *reinterpret_cast<const float4*>(w + ((int64_t)kw * cout + co0 + row) * cin + c0 + p * 4);
          } else {   // [cin][cout]: the chunk's rows, CB columns of each
            const int row = e / (CB / 4), p = e - row * (CB / 4);
            if (row < cw) rw[i] = *reinterpret_cast<const float4*>(w + ((int64_t)kw * cin + c0 + row) * cout + co0 + p * 4);
          }
        }
      };
      auto commit = [&](int buf) {
        float* sa = s_stage + buf * G::STAGE_FLOATS;
        float* sw = sa + G::A_FLOATS;
#pragma unroll
        for (int i = 0; i < G::A_VEC; ++i) *reinterpret_cast<float4*>(sa + (prow + 16 * i) * kPitchA + piece * 4) = ra[i];
#pragma unroll
        for (int i = 0; i < G::W_VEC; ++i) {
          const int e = tid + 256 * i;
          if (WT) *reinterpret_cast<float4*>(sw + (e >> 4) * kPitchA + (e & 15) * 4) = rw[i];
          else *reinterpret_cast<float4*>(sw + (e / (CB / 4)) * PW + (e % (CB / 4)) * 4) = rw[i];
        }
      };
      auto compute = [&](int buf, int k, int chunk) {
        if (!((rb_mask >> k) & 1u)) return;  // wave-uniform: none of the wave's rows has the offset
        const int cw = cin - chunk * kCIC < kCIC ? cin - chunk * kCIC : kCIC;
        const float* sa = s_stage + buf * G::STAGE_FLOATS + (rb * 32 + n) * kPitchA + 4 * h;
        const float* sw = s_stage + buf * G::STAGE_FLOATS + G::A_FLOATS;
        const int col = wc * NB * 32 + n;
        for (int j = 0; j < cw / 8; ++j) {
          const float4 a = *reinterpret_cast<const float4*>(sa + 8 * j);
          float4 bq[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if (WT) {
              bq[b] = *reinterpret_cast<const float4*>(sw + (col + 32 * b) * kPitchA + 8 * j + 4 * h);
            } else {
              const float* p = sw + (8 * j + 4 * h) * PW + col + 32 * b;
              bq[b] = make_float4(p[0], p[PW], p[2 * PW], p[3 * PW]);
            }
          }
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] = mfma_f32(a.x, bq[b].x, acc[b]);
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] = mfma_f32(a.y, bq[b].y, acc[b]);
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] = mfma_f32(a.z, bq[b].z, acc[b]);
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] = mfma_f32(a.w, bq[b].w, acc[b]);
        }
      };
      StepIter steps{block_mask, nchunk};
      int k = -1, c = 0, buf = 0;
      steps.next(k, c);
      fetch(k, c);
      commit(0);
      __syncthreads();
      for (;;) {
        int k2 = k, c2 = c;
        const bool has = steps.next(k2, c2);
        if (has) fetch(k2, c2);   // in flight under the MFMAs below
        compute(buf, k, c);
        if (!has) break;
        commit(buf ^ 1);          // last read before the barrier of the step before
        __syncthreads();
        buf ^= 1; k = k2; c = c2;
      }
    }
    __syncthreads();  // stages, index slab and mask words are rewritten by the next pass
  }

#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int col = co0 + wc * NB * 32 + 32 * b + n;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float4 o = epi_bias(acc4(acc[b], v), make_float4(bv, bv, bv, bv));
      const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int32_t r = s_rows[rb * 32 + 8 * v + 4 * h + q];
        if (r >= 0) out[(int64_t)r * cout + col] = ov[q];
      }
    }
  }
}

template <int NB, int WC, bool WT>
int launch_gather_f32(const float* in, const float* w, float* out, const int32_t* nbr, const uint32_t* mask,
                      const int32_t* perm, const float* bias, int64_t n_out, int cin, int cout, int K, int k_flip,
                      hipStream_t s) {
  typedef GatherF32<NB, WC> G;
  static unsigned long long attr_done = 0ull;  // per device (wcn_common.h)
  const int rc = once_per_device(attr_done, [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(gather_gemm_f32_kernel<NB, WC, WT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES) == hipSuccess;
  });
  if (rc != WCN_SUCCESS) return rc;
  const dim3 grid((unsigned)ceil_div(n_out, G::TILE), (unsigned)(cout / G::CB));
  hipLaunchKernelGGL((gather_gemm_f32_kernel<NB, WC, WT>), grid, dim3(256), G::LDS_BYTES, s, in, w, out, nbr, mask, perm, bias,
                     n_out, cin, cout, K, wcn_kmap_row_pitch(K), wcn_kmap_mask_words(K), k_flip);
  return launch_status();
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
constexpr int kWgradRanges = 256;  // pair ranges of the global pair list (one per CU and plane block)
constexpr int kWgradPairs = 32;    // pairs per step
constexpr int kWgradCI = 64, kWgradCO = 128;   // block of the [cin, cout] plane per workgroup
constexpr int kPitchX = kWgradCI + 32, kPitchY = kWgradCO + 32;
constexpr int kWgradStage = kWgradPairs * (kPitchX + kPitchY);  // floats
constexpr size_t kWgradLds = 2 * (size_t)kWgradStage * 4;

// pairs per range: the same in both kernels
__device__ __forceinline__ int wgrad_f32_range(int total) {
  const int per = (total + kWgradRanges - 1) / kWgradRanges;
  const int steps = (per + kWgradPairs - 1) / kWgradPairs;
  return (steps > 0 ? steps : 1) * kWgradPairs;
}

__global__ __launch_bounds__(256) void wgrad_f32_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        const int32_t* __restrict__ in_maps,
                                                        const int32_t* __restrict__ out_maps,
                                                        const int32_t* __restrict__ offsets, float* __restrict__ slabs, int cin,
                                                        int cout, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_stage = reinterpret_cast<float*>(smem);  // [2][x rows | dy rows]

  const int total = offsets[K];
  const int per = wgrad_f32_range(total);
  const int g = blockIdx.x;
  const int64_t r0 = (int64_t)g * per;
  if (r0 >= total) return;  // (uniform)
  const int r1 = r0 + per < total ? (int)(r0 + per) : total;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, n = lane & 31;
  const int wi = wave & 1, wo = wave >> 1;  // 2 x 2 sub-tiles of 32 x 64
  const int nco = (cout + kWgradCO - 1) / kWgradCO;
  const int ci0 = (blockIdx.y / nco) * kWgradCI, co0 = (blockIdx.y % nco) * kWgradCO;
  const bool a_on = ci0 + 32 * wi < cin;                                  // (wave-uniform) the wave's blocks inside the plane
  const bool b_on[2] = {co0 + 64 * wo < cout, co0 + 64 * wo + 32 < cout};
  const size_t plane = (size_t)cin * cout;

  f32x16 acc[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;

  int k = last_offset_not_above(offsets, K, r0);
  int p = (int)r0;
  while (p < r1) {
    const int next = offsets[k + 1];
    const int end = next < r1 ? next : r1;
    if (end > p) {
      float4 rx[2], ry[4];
      auto fetch = [&](int base) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {  // 16 lanes a row piece of 64 channels
          const int e = tid + 256 * i, q = base + (e >> 4), c = ci0 + (e & 15) * 4;
          rx[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (q < end && c < cin) rx[i] = *reinterpret_cast<const float4*>(x + (int64_t)in_maps[q] * cin + c);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // 32 lanes a row piece of 128 channels
          const int e = tid + 256 * i, q = base + (e >> 5), c = co0 + (e & 31) * 4;
          ry[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (q < end && c < cout) ry[i] = *reinterpret_cast<const float4*>(dy + (int64_t)out_maps[q] * cout + c);
        }
      };
      auto commit = [&](int buf) {
        float* sx = s_stage + buf * kWgradStage;
        float* sy = sx + kWgradPairs * kPitchX;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int e = tid + 256 * i;
          *reinterpret_cast<float4*>(sx + (e >> 4) * kPitchX + (e & 15) * 4) = rx[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = tid + 256 * i;
          *reinterpret_cast<float4*>(sy + (e >> 5) * kPitchY + (e & 31) * 4) = ry[i];
        }
      };
      auto compute = [&](int buf) {
        if (!a_on || !b_on[0]) return;
        const float* sx = s_stage + buf * kWgradStage + h * kPitchX + 32 * wi + n;
        const float* sy = s_stage + buf * kWgradStage + kWgradPairs * kPitchX + h * kPitchY + 64 * wo + n;
#pragma unroll
        for (int s = 0; s < kWgradPairs / 2; ++s) {
          const float a = sx[2 * s * kPitchX];
          acc[0] = mfma_f32(a, sy[2 * s * kPitchY], acc[0]);
          if (b_on[1]) acc[1] = mfma_f32(a, sy[2 * s * kPitchY + 32], acc[1]);
        }
      };
      int buf = 0;
      fetch(p);
      commit(0);
      __syncthreads();
      for (int base = p; base < end; base += kWgradPairs) {
        const bool has = base + kWgradPairs < end;
        if (has) fetch(base + kWgradPairs);
        compute(buf);
        if (!has) break;
        commit(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
      // flush: lane (h, n) holds column n of rows 8 v + 4 h + q of its blocks
      float* slab = slabs + (size_t)(g + k) * plane;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = co0 + 64 * wo + 32 * b + n;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int ci = ci0 + 32 * wi + 8 * (q >> 2) + 4 * h + (q & 3);
          if (a_on && b_on[b] && ci < cin) slab[(size_t)ci * cout + col] = acc[b][q];
          acc[b][q] = 0.f;
        }
      }
      __syncthreads();  // the stages are rewritten by the next bucket
    }
    p = end;
    ++k;
  }
}

// dw[k] = the slabs of bucket k in ascending range order; zeros for an empty bucket.  One thread per 16-B piece.
__global__ __launch_bounds__(256) void wgrad_f32_reduce_kernel(const float4* __restrict__ slabs, const int32_t* __restrict__ offsets,
                                                               float4* __restrict__ dw, int plane4, int K) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)K * plane4) return;
  const int k = (int)(e / plane4), i = (int)(e - (int64_t)k * plane4);
  const int per = wgrad_f32_range(offsets[K]);
  const int o0 = offsets[k], o1 = offsets[k + 1];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (o1 > o0) {
    for (int g = o0 / per; g <= (o1 - 1) / per; ++g) s = epi_bias(s, slabs[(size_t)(g + k) * plane4 + i]);
  }
  dw[e] = s;
}

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool mfma_f32_gather_supported(int cin, int cout, int K) {
  return cin >= 16 && cin % 16 == 0 && cout >= 32 && cout % 32 == 0 && cout / 32 <= 65535 && valid_k(K);
}
bool mfma_f32_wgrad_supported(int cin, int cout) {
  return cin >= 16 && cin % 16 == 0 && cout >= 32 && cout % 32 == 0 && (int64_t)cin * cout <= (1 << 24);
}
size_t wgrad_f32_workspace(int K, int cin, int cout) {
  return (size_t)(kWgradRanges + K) * cin * cout * sizeof(float);
}

int conv_gather_gemm_f32(const float* in, const float* w, float* out, const int32_t* nbr, const uint32_t* mask,
                         const int32_t* perm, const float* bias, int64_t n_out, int cin, int cout, int K, int w_transposed,
                         int k_flip, hipStream_t s) {
  if (!mfma_f32_gather_supported(cin, cout, K)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!mask || !aligned_to(in, 16) || !aligned_to(w, 16) || ceil_div(n_out, 64) > 0x7fffffff) return WCN_ERROR_INVALID_PARAMETERS;
  auto go = [&](auto nb, auto wcols) {
    constexpr int NB = decltype(nb)::value, WC = decltype(wcols)::value;
    return w_transposed ? launch_gather_f32<NB, WC, true>(in, w, out, nbr, mask, perm, bias, n_out, cin, cout, K, k_flip, s)
                        : launch_gather_f32<NB, WC, false>(in, w, out, nbr, mask, perm, bias, n_out, cin, cout, K, k_flip, s);
  };
  typedef std::integral_constant<int, 1> I1;
  typedef std::integral_constant<int, 2> I2;
  if (cout % 128 == 0) return go(I2{}, I2{});
  if (cout % 64 == 0) return go(I1{}, I2{});
  return go(I1{}, I1{});
}

int conv_wgrad_f32(const float* x, const float* dy, float* dw, const int32_t* in_maps, const int32_t* out_maps,
                   const int32_t* offsets, int cin, int cout, int K, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (!mfma_f32_wgrad_supported(cin, cout) || !valid_k(K)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!workspace || workspace_bytes < wgrad_f32_workspace(K, cin, cout) || !aligned_to(workspace, 16) || !aligned_to(dw, 16) ||
      !aligned_to(x, 16) || !aligned_to(dy, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  static unsigned long long attr_done = 0ull;  // per device (wcn_common.h)
  const int rc = once_per_device(attr_done, [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(wgrad_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kWgradLds) == hipSuccess;
  });
  if (rc != WCN_SUCCESS) return rc;
  const int blocks = (int)(ceil_div(cin, kWgradCI) * ceil_div(cout, kWgradCO));
  hipLaunchKernelGGL(wgrad_f32_kernel, dim3(kWgradRanges, blocks), dim3(256), kWgradLds, s, x, dy, in_maps, out_maps, offsets,
                     (float*)workspace, cin, cout, K);
  const int plane4 = cin * cout / 4;
  hipLaunchKernelGGL(wgrad_f32_reduce_kernel, dim3((unsigned)ceil_div((int64_t)K * plane4, 256)), dim3(256), 0, s,
                     (const float4*)workspace, offsets, (float4*)dw, plane4, K);
  return launch_status();
}

}  // namespace wcn
