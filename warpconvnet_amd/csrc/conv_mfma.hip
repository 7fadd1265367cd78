// conv_mfma.hip - fused gather -> MFMA -> store kernel for the AB (forward) and ABt (dgrad) sparse-conv GEMMs.
//
// Design (gfx950, wave64):
//   * output-stationary: a workgroup of 4 waves owns TILE = 4*32*RB output rows (taken through the
//     mask-sorted permutation) and all CO output channels; fp32 accumulators live in registers.
//   * the MFMA is issued "transposed": A operand = weight fragment (M = 32 output channels),
//     B operand = 32 gathered feature rows (N = rows).  With the row/column permutations folded into
//     the PACKED weight image (wcn_pack_weight) every lane (a) gathers CIC/2 CONTIGUOUS channels of one
//     input row straight from HBM into its B registers - no LDS hop, no transpose - and (b) ends up
//     holding CO/2 contiguous output channels of one output row, stored with 16-B writes.
//   * weights: the [CIC x CO] slab of the current (offset, channel-chunk) step is streamed into LDS by
//     LDS-DMA (global_load_lds, 16 B/lane) in exactly the order the A fragments are read back
//     (lane-linear => conflict-free ds_read_b128), double buffered, one barrier per step.  The DMA goes through
//     inline asm and the per-step drain through the s_waitcnt BUILTIN: with the DMA builtin hipcc drains vmcnt(0)
//     in front of the first LDS read of every step (i.e. in front of the MFMAs), and with an asm s_waitcnt its own
//     scoreboard still believes the gathered registers are in flight and waits again - either way gather latency
//     and math serialise.
//   * the tile's neighbour rows (TILE x 32 int32) are staged in LDS once ("index slab").
//   * offsets absent from every row of the workgroup are skipped (bitmask OR), and a wave skips the
//     gather + MFMA of an offset none of its own rows has.
//   * epilogue: + bias in fp32, round, transpose 32 rows at a time through a wave-private LDS stage and write whole
//     rows with adjacent lanes (full-line writes instead of 8 partial-line write requests per 128 B).
//
// Math: out[r] = sum_k in[nbr[r][k]] . Wp[k]  (fp32 accumulate), Wp = packed image of w (forward),
// or of w^T with k reversed (dgrad of a submanifold map), or of w^T (dgrad with a reverse table).
// Reference semantics: warpconvnet/nn/functional/sparse_conv/detail/explicit.py:22-57, 60-92; role of
// _C.mask_gemm.fwd/.dgrad (warpconvnet/csrc/bindings/mask_gemm_bindings.cu:2074-2101).
#include "gather_gemm.h"

namespace wcn {

constexpr int kWaves = 4;
constexpr int kMaxKp = 32;  // table columns staged per pass (one mask word)
constexpr int kMaxK = 1024;  // kernel volumes up to 32 mask words (5^3 = 125 and 7^3 = 343 included)

// ---- main kernel -------------------------------------------------------------------------------------
template <typename T, int CIC, int CO, int RB>
struct GatherGemm {
  static constexpr int NS = CIC / 16;
  static constexpr int NB = CO / 32;
  static constexpr int ROWS_PER_WAVE = 32 * RB;
  static constexpr int TILE = kWaves * ROWS_PER_WAVE;
  static constexpr int SLAB_ELEMS = CIC * CO;
  static constexpr int SLAB_BYTES = SLAB_ELEMS * 2;
  static constexpr size_t LDS_BYTES = 2 * (size_t)SLAB_BYTES + (size_t)TILE * kMaxKp * 4 + (size_t)TILE * 4 + 64;
  typedef typename Mfma32<T>::type frag_t;
};

template <typename T, int CIC, int CO, int RB, bool MULTI>
__global__ __launch_bounds__(256, 2) void gather_gemm_mfma_kernel(const T* __restrict__ in, const T* __restrict__ wp,
                                                               T* __restrict__ out, const int32_t* __restrict__ nbr,
                                                               const uint32_t* __restrict__ mask,
                                                               const int32_t* __restrict__ perm,
                                                               ConvEpilogue epi, int64_t n_out, int cin,
                                                               int K, int kp, int mw, float* __restrict__ out32,
                                                               int in_stride, int out_stride) {
  // Channel groups (weight [K, G, Cin/G, Cout/G], reference MaskGemm_forward_64x64x32_1s_flat.h:117-123): ONE launch, the
  // group on grid.y.  `cin` / CO are the PER-GROUP widths, rows are in_stride / out_stride elements apart, group g reads
  // channels [g*cin, (g+1)*cin) and writes [g*CO, (g+1)*CO); the packed weight images of the groups follow each other.
  {
    const int grp = blockIdx.y;
    in += (int64_t)grp * cin;
    wp += (int64_t)grp * K * cin * CO;
    if (out) out += (int64_t)grp * CO;
    if (out32) out32 += (int64_t)grp * CO;
    if (epi.bias) epi.bias += grp * CO;
    if (epi.scale) { epi.scale += grp * CO; epi.shift += grp * CO; }
    if (epi.residual) epi.residual = reinterpret_cast<const T*>(epi.residual) + (int64_t)grp * CO;
  }
  typedef GatherGemm<T, CIC, CO, RB> G;
  typedef typename G::frag_t frag_t;
  constexpr int NS = G::NS, NB = G::NB, RPW = G::ROWS_PER_WAVE, TILE = G::TILE;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* s_w = reinterpret_cast<T*>(smem);                                        // [2][SLAB_ELEMS]
  int32_t* s_nbr = reinterpret_cast<int32_t*>(smem + 2 * G::SLAB_BYTES);      // [TILE][kp]
  int32_t* s_rows = s_nbr + TILE * kMaxKp;                                    // [TILE]
  uint32_t* s_wmask = reinterpret_cast<uint32_t*>(s_rows + TILE);             // [4]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, n = lane & 31;
  const int nchunk = cin / CIC;
  const int64_t row0 = (int64_t)blockIdx.x * TILE;

  stage_row_ids<TILE>(s_rows, perm, row0, n_out);
  __syncthreads();

  f32x16 acc[NB][RB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[b][rb][q] = 0.f;

  // Kernel volumes above 32 offsets: one pass per 32-bit mask word - the index slab holds the 32 table columns of the
  // current word, the accumulators persist across words.  (K <= 32: a single pass, as before.)
  const int nwords = MULTI ? mw : 1;  // compile-time 1 for K <= 32: the accumulators are then not live during staging
  for (int word = 0; word < nwords; ++word) {
  const int kbase = word * 32;
  const int kpw = (kp - kbase) < kMaxKp ? (kp - kbase) : kMaxKp;  // table columns staged for this word
  uint32_t my_mask = 0;
  if (tid < TILE) {
    const int32_t r = s_rows[tid];
    if (r >= 0) my_mask = mask[(int64_t)r * mw + word];  // thread tid stages row tid, which belongs to wave tid / RPW
  }
  {
    // all row ids first, then all table loads, then all LDS writes: written as one loop, every s_rows read is ordered
    // behind the previous s_nbr write (same LDS array) and the global round trips serialise
    const int vec_per_row = kpw >> 2;
    constexpr int kIter = TILE * (kMaxKp / 4) / 256;
    int32_t rr[kIter];
    int4 vv[kIter];
#pragma unroll
    for (int t = 0; t < kIter; ++t) {
      const int e = tid + t * 256;
      rr[t] = (e < TILE * vec_per_row) ? s_rows[e / vec_per_row] : -1;
    }
#pragma unroll
    for (int t = 0; t < kIter; ++t) {
      const int e = tid + t * 256;
      const int i = e / vec_per_row, c = e - i * vec_per_row;
      vv[t] = make_int4(-1, -1, -1, -1);
      if (rr[t] >= 0) {  // read once: non-temporal
        typedef __attribute__((ext_vector_type(4))) int i32x4;
        const i32x4 q = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(nbr + (int64_t)rr[t] * kp + kbase) + c);
        vv[t] = make_int4(q.x, q.y, q.z, q.w);
      }
    }
#pragma unroll
    for (int t = 0; t < kIter; ++t) {
      const int e = tid + t * 256;
      const int i = e / vec_per_row, c = e - i * vec_per_row;
      if (e < TILE * vec_per_row) reinterpret_cast<int4*>(s_nbr + i * kpw)[c] = vv[t];
    }
  }
  // OR-reduce masks: rows of wave w are [w*RPW, (w+1)*RPW)
  // (one word per 32-row block: a wave also skips the MFMAs of a row block that has no row with the offset)
  if (tid < kWaves * RB) s_wmask[tid] = 0;
  __syncthreads();
  or_row_mask<TILE, 32>(s_wmask, my_mask);
  __syncthreads();
  uint32_t rb_mask[RB];
  uint32_t wave_mask = 0u;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    rb_mask[rb] = __builtin_amdgcn_readfirstlane(s_wmask[wave * RB + rb]);  // wave-uniform: keep it in an SGPR
    wave_mask |= rb_mask[rb];
  }
  const uint32_t block_mask = tile_mask<kWaves * RB>(s_wmask);

  if (block_mask != 0u) {
    // weight slab of the step by LDS-DMA, then the rows: lane (h, n) pulls its half of the chunk's channels of row n
    auto fetch = [&](int buf, frag_t (&bf)[RB][NS], int k, int chunk) {
      const T* slab = wp + ((int64_t)(kbase + k) * nchunk + chunk) * G::SLAB_ELEMS;
      dma_weights<G::SLAB_BYTES, kWaves>(reinterpret_cast<const char*>(slab),
                                         reinterpret_cast<char*>(s_w) + (size_t)buf * G::SLAB_BYTES, wave, lane);
      if (!((wave_mask >> k) & 1u)) return;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int i = wave * RPW + rb * 32 + n;
        const int32_t idx = s_nbr[i * kpw + k];
        const T* p = in + (int64_t)idx * in_stride + chunk * CIC + h * (CIC / 2);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          frag_t v;
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = (T)0.f;
          if (idx >= 0) v = *reinterpret_cast<const frag_t*>(p + s * 8);
          bf[rb][s] = v;
        }
      }
    };
    auto compute = [&](const frag_t (&bf)[RB][NS], int buf, int k) {
      if (!((wave_mask >> k) & 1u)) return;
      const frag_t* wl = reinterpret_cast<const frag_t*>(reinterpret_cast<const char*>(s_w) + (size_t)buf * G::SLAB_BYTES);
      // the NB weight fragments of channel slice s+1 are read from LDS while the NB*RB MFMAs of slice s run
      frag_t a_cur[NB], a_nxt[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) a_cur[b] = wl[(b * NS) * 64 + lane];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) {
#pragma unroll
          for (int b = 0; b < NB; ++b) a_nxt[b] = wl[(b * NS + s + 1) * 64 + lane];
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          if (RB > 1 && !((rb_mask[rb] >> k) & 1u)) continue;  // wave-uniform: no row of this block has offset k
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b][rb] = Mfma32<T>::mfma(a_cur[b], bf[rb][s], acc[b][rb]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) a_cur[b] = a_nxt[b];
      }
    };
    // double buffered: while step i multiplies from weight buffer b and row registers Bb, the slab and the rows of step i + 1
    // are in flight into buffer 1 - b; one barrier per step
    StepIter steps{block_mask, nchunk};
    frag_t B0[RB][NS], B1[RB][NS];
    int k0 = -1, c0 = 0, k1 = -1, c1 = 0;
    steps.next(k0, c0);
    fetch(0, B0, k0, c0);
    sync_step();
    bool more = true;
    while (more) {
      // even half-iteration: compute (k0,c0) from buffer 0 while fetching (k1,c1) into buffer 1
      k1 = k0; c1 = c0;
      const bool has1 = steps.next(k1, c1);
      if (has1) fetch(1, B1, k1, c1);
      compute(B0, 0, k0);
      sync_step();
      if (!has1) break;
      // odd half-iteration
      k0 = k1; c0 = c1;
      const bool has0 = steps.next(k0, c0);
      if (has0) fetch(0, B0, k0, c0);
      compute(B1, 1, k1);
      sync_step();
      more = has0;
    }
  }
  __syncthreads();  // the slab and the mask words are rewritten by the next pass
  }  // word

  // ---- epilogue: lane (h, n) holds out channels h*CO/2 + 16*b + q of row (rb, n).  Storing that straight to HBM
  // makes every lane write 16-B pieces of its own row (8 partial-line write requests per 128-B line); instead each
  // wave transposes 32 rows at a time through its own LDS stage and writes whole rows with adjacent lanes. ----
  constexpr int kPitch = CO * 2 + 16;               // bytes; +16 keeps the b128 stage writes conflict-free
  constexpr int kStage = 32 * kPitch;               // one 32-row block per wave
  constexpr bool kStaged = (size_t)kWaves * kStage <= 2 * (size_t)G::SLAB_BYTES + (size_t)TILE * kMaxKp * 4;
  if (out32) {
    // fp32 output (the fp32-feature path: fp16 operands, fp32 accumulate, unrounded result): every lane stores its
    // 16 contiguous channels per block straight from the accumulators
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int32_t r = s_rows[wave * RPW + rb * 32 + n];
      if (r < 0) continue;
      float* dst = out32 + (int64_t)r * out_stride + h * (CO / 2);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float4 o = make_float4(acc[b][rb][4 * v + 0], acc[b][rb][4 * v + 1], acc[b][rb][4 * v + 2], acc[b][rb][4 * v + 3]);
          if (epi.bias) {
            const float4 bv = reinterpret_cast<const float4*>(epi.bias + h * (CO / 2) + 16 * b)[v];
            o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
          }
          reinterpret_cast<float4*>(dst + 16 * b)[v] = o;
        }
      }
    }
    return;
  }
  if (kStaged) __syncthreads();  // the weight / index slabs are dead from here on: reuse them as the stage
  char* stage = smem + wave * kStage;
  constexpr int kLanesPerRow = CO / 8;              // 16-B pieces per output row
  constexpr int kRowsPerInstr = 64 / kLanesPerRow;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int i = wave * RPW + rb * 32 + n;
    const int32_t r = s_rows[i];
    T* dst = out + (int64_t)r * out_stride + h * (CO / 2);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      frag_t lo, hi;
      if (epi.bias) {  // fused epilogue: + bias[co] in fp32 before the rounding to the storage dtype
        const float4* bp = reinterpret_cast<const float4*>(epi.bias + h * (CO / 2) + 16 * b);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float4 bv = bp[v];
          acc[b][rb][4 * v + 0] += bv.x; acc[b][rb][4 * v + 1] += bv.y;
          acc[b][rb][4 * v + 2] += bv.z; acc[b][rb][4 * v + 3] += bv.w;
        }
      }
      if (epi.scale) {  // per-channel affine (BatchNorm in inference mode)
        const float4* sp4 = reinterpret_cast<const float4*>(epi.scale + h * (CO / 2) + 16 * b);
        const float4* tp4 = reinterpret_cast<const float4*>(epi.shift + h * (CO / 2) + 16 * b);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float4 sv = sp4[v], tv = tp4[v];
          acc[b][rb][4 * v + 0] = acc[b][rb][4 * v + 0] * sv.x + tv.x; acc[b][rb][4 * v + 1] = acc[b][rb][4 * v + 1] * sv.y + tv.y;
          acc[b][rb][4 * v + 2] = acc[b][rb][4 * v + 2] * sv.z + tv.z; acc[b][rb][4 * v + 3] = acc[b][rb][4 * v + 3] * sv.w + tv.w;
        }
      }
      if (!kStaged && epi.residual && r >= 0) {  // direct path: the lane owns 16 contiguous channels of its row
        const T* rp = reinterpret_cast<const T*>(epi.residual) + (int64_t)r * out_stride + h * (CO / 2) + 16 * b;
        const frag_t r0 = *reinterpret_cast<const frag_t*>(rp), r1 = *reinterpret_cast<const frag_t*>(rp + 8);
#pragma unroll
        for (int q = 0; q < 8; ++q) { acc[b][rb][q] += (float)r0[q]; acc[b][rb][8 + q] += (float)r1[q]; }
      }
      if (epi.relu && !(kStaged && epi.residual)) {  // (with a staged residual the activation follows the add below)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][rb][q] = fmaxf(acc[b][rb][q], 0.f);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        lo[q] = (T)acc[b][rb][q];
        hi[q] = (T)acc[b][rb][8 + q];
      }
      if (kStaged) {
        frag_t* sp = reinterpret_cast<frag_t*>(stage + n * kPitch + (h * (CO / 2) + 16 * b) * 2);
        sp[0] = lo;
        sp[1] = hi;
      } else if (r >= 0) {
        *reinterpret_cast<frag_t*>(dst + 16 * b) = lo;
        *reinterpret_cast<frag_t*>(dst + 16 * b + 8) = hi;
      }
    }
    if (kStaged) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // stage is wave-private: LDS ops of one wave execute in order
      const int piece = lane % kLanesPerRow, rsub = lane / kLanesPerRow;
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += kRowsPerInstr) {
        const int row = r0 + rsub;
        if (rsub < kRowsPerInstr && row < 32) {
          const int32_t rr = s_rows[wave * RPW + rb * 32 + row];
          if (rr >= 0) {
            frag_t o = *reinterpret_cast<const frag_t*>(stage + row * kPitch + piece * 16);
            if (epi.residual) {
              const frag_t rv = __builtin_nontemporal_load(
                  reinterpret_cast<const frag_t*>(reinterpret_cast<const T*>(epi.residual) + (int64_t)rr * out_stride + piece * 8));
              o = add_residual<T>(o, rv, epi.relu);
            }
            __builtin_nontemporal_store(o, reinterpret_cast<frag_t*>(out + (int64_t)rr * out_stride + piece * 8));
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // next block overwrites the stage
    }
  }
}

template <typename T, int CIC, int CO, int RB>
static int launch_gather_gemm(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                              const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int K, float* out32,
                              hipStream_t s, int groups = 1) {
  typedef GatherGemm<T, CIC, CO, RB> G;
  const int kp = wcn_kmap_row_pitch(K);
  const int mw = wcn_kmap_mask_words(K);
  const dim3 grid((unsigned)ceil_div(n_out, G::TILE), (unsigned)groups);
  const int in_stride = cin * groups, out_stride = CO * groups;
  return launch_multi<gather_gemm_mfma_kernel<T, CIC, CO, RB, false>, gather_gemm_mfma_kernel<T, CIC, CO, RB, true>>(
      mw != 1, grid, G::LDS_BYTES, s, (const T*)in, (const T*)wp, (T*)out, nbr, mask, perm, epi, n_out, cin, K, kp, mw,
      out32, in_stride, out_stride);
}

// Output widths 96 / 128 run 32 rows per wave (128-row tiles, 64 / 48 accumulator registers, three workgroups per CU
// instead of two): 4-6 % faster than 64 rows per wave on both scene types (round 2).  Width 64 keeps 64 rows per wave.
template <typename T, int CIC>
static int dispatch_co(int cout, const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                       const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int K, float* out32,
                       hipStream_t s, int groups) {
  switch (cout) {
    case 32: return launch_gather_gemm<T, CIC, 32, 2>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 64: return launch_gather_gemm<T, CIC, 64, 2>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 96: return launch_gather_gemm<T, CIC, 96, 1>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 128: return launch_gather_gemm<T, CIC, 128, 1>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 192: return launch_gather_gemm<T, CIC, 192, 1>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 256: return launch_gather_gemm<T, CIC, 256, 1>(in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    default: return WCN_ERROR_UNSUPPORTED_CONFIG;
  }
}

// reduction chunk per step: 64 channels when they divide cin (measured optimum between loads in flight per wave and steps
// per tile: a 128 -> 64 dgrad with one 128-channel step per offset 317 us, with 32-channel steps 314 us, vs 265 us)
static int mfma32_chunk(int cin) {
  if (cin % 64 == 0) return 64;
  if (cin % 32 == 0) return 32;
  if (cin % 16 == 0) return 16;
  return 0;
}

// channel shapes of the 32x32x16 kernels in this file
bool mfma32_shape(int cin, int cout) {
  if (mfma32_chunk(cin) == 0) return false;
  return cout == 32 || cout == 64 || cout == 96 || cout == 128 || cout == 192 || cout == 256;
}

// The family a shape goes to: channel-split where it applies (incl. outputs in column blocks: 320 = 5 x 64, 384, 512 ...),
// else the 16x16x32 kernels (which leave the 32x32x16 shapes alone), else the 32x32x16 kernels of this file.
GemmFamily gather_gemm_family(int cin, int cout, int K, int dtype) {
  if (gather_gemm_cs_supported(cin, cout, K, dtype)) return GemmFamily::ChannelSplit;
  if (mfma16_supported(cin, cout, K, dtype)) return GemmFamily::Mfma16;
  if (dtype != WCN_F16 && dtype != WCN_BF16) return GemmFamily::None;
  if (K < 1 || K > kMaxK) return GemmFamily::None;
  return mfma32_shape(cin, cout) ? GemmFamily::Mfma32 : GemmFamily::None;
}

bool mfma_gather_supported(int cin, int cout, int K, int dtype) {
  return gather_gemm_family(cin, cout, K, dtype) != GemmFamily::None;
}

template <typename T>
static int dispatch_cic(int cin, int cout, const void* in, const void* wp, void* out, const int32_t* nbr,
                        const uint32_t* mask, const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int K, float* out32,
                        hipStream_t s, int groups = 1) {
  switch (mfma32_chunk(cin)) {
    case 64: return dispatch_co<T, 64>(cout, in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 32: return dispatch_co<T, 32>(cout, in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    case 16: return dispatch_co<T, 16>(cout, in, wp, out, nbr, mask, perm, epi, n_out, cin, K, out32, s, groups);
    default: return WCN_ERROR_UNSUPPORTED_CONFIG;
  }
}

// channel groups in ONE launch: per-group widths cin x cout, the 32x32x16 kernels (group index on grid.y)
bool mfma_grouped_supported(int cin, int cout, int K, int dtype) {
  return (dtype == WCN_F16 || dtype == WCN_BF16) && K >= 1 && K <= kMaxK && mfma32_shape(cin, cout);
}
int conv_gather_gemm_grouped(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                             const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int groups,
                             int K, int dtype, hipStream_t s) {
  if (groups < 1 || groups > 65535 || !mfma_grouped_supported(cin, cout, K, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return with_dtype16(dtype, [&](auto t) {
    return dispatch_cic<decltype(t)>(cin, cout, in, wp, out, nbr, mask, perm, epi, n_out, K, nullptr, s, groups);
  });
}

int conv_gather_gemm_mfma(const void* in, const void* wp, void* out, const int32_t* nbr, const uint32_t* mask,
                          const int32_t* perm, const ConvEpilogue& epi, int64_t n_out, int cin, int cout, int K, int dtype,
                          float* out32, hipStream_t s) {
  switch (gather_gemm_family(cin, cout, K, dtype)) {
    case GemmFamily::ChannelSplit:
      return conv_gather_gemm_cs(in, wp, out, nbr, mask, perm, epi, n_out, cin, cout, K, dtype, out32, s);
    case GemmFamily::Mfma16:
      return conv_gather_gemm16(in, wp, out, nbr, mask, perm, epi, n_out, cin, cout, K, dtype, out32, s);
    case GemmFamily::Mfma32:
      return with_dtype16(dtype, [&](auto t) {
        return dispatch_cic<decltype(t)>(cin, cout, in, wp, out, nbr, mask, perm, epi, n_out, K, out32, s);
      });
    case GemmFamily::None: break;
  }
  return WCN_ERROR_UNSUPPORTED_CONFIG;
}

// ---- weight packing (all three families) ---------------------------------------------------------------------------------
// A packed image is a permutation of the weight (plus zero padding, channel-split family) in the order the consuming
// kernel reads its A fragments.  A Layout knows the element count of its image and, for packed element e, the weight
// element it holds: offset k, group, input channel ci, output channel co (kernel-side roles: reduce over ci, produce co),
// and whether it exists at all.  Source: w[K][groups][cin][cout], or [K][groups][cout][cin] with `transpose` (the forward
// weight, packed for a dgrad); `flip` reverses k (dgrad of a submanifold map).
struct PackIndex { int k, grp, ci, co; bool valid; };
struct PackShape { int K, cin, cout, groups; };

// 32x32x16 kernels (this file): per group packed[k][chunk][b][s][lane][j], lane = (h<<5)|m:
//   ci = chunk*CIC + h*(CIC/2) + 8*s + j
//   co = ((m>>2)&1)*(CO/2) + 16*b + 4*(m>>3) + (m&3)
// so that the C fragment of lane (h', n) holds out channels h'*(CO/2) + 16*b + reg, reg = 0..15.
// Grouped weights (cin / cout per group): the images of the groups back to back.
struct Pack32 : PackShape {
  int cic;
  __host__ __device__ int64_t elements() const { return (int64_t)groups * K * cin * cout; }
  __device__ PackIndex at(int64_t e) const {
    const int64_t per_group = (int64_t)K * cin * cout;
    const int NS = cic / 16, NB = cout / 32, nchunk = cin / cic;
    PackIndex x;
    x.grp = (int)(e / per_group);
    int64_t t = e - (int64_t)x.grp * per_group;
    const int j = (int)(t % 8); t /= 8;
    const int lane = (int)(t % 64); t /= 64;
    const int s = (int)(t % NS); t /= NS;
    const int b = (int)(t % NB); t /= NB;
    const int chunk = (int)(t % nchunk); t /= nchunk;
    x.k = (int)t;
    const int h = lane >> 5, m = lane & 31;
    x.ci = chunk * cic + h * (cic / 2) + 8 * s + j;
    x.co = ((m >> 2) & 1) * (cout / 2) + 16 * b + 4 * (m >> 3) + (m & 3);
    x.valid = true;
    return x;
  }
};

// 16x16x32 kernels (conv_mfma16.hip): packed[k][chunk][c][cb][lane][j], lane = (g<<4)|n:
//   ci = chunk*CIC + 32*c + 8*g + j          co = (n >> 2)*(CO/4) + 4*cb + (n & 3)
// so the D fragments of lane (g, n) over cb = 0..CO/16-1 are the CO/4 contiguous output channels [g*CO/4, (g+1)*CO/4).
struct Pack16 : PackShape {
  int cic;
  __host__ __device__ int64_t elements() const { return (int64_t)K * cin * cout; }
  __device__ PackIndex at(int64_t e) const {
    const int NC = cic / 32, NCB = cout / 16, nchunk = cin / cic;
    int64_t t = e;
    const int j = (int)(t % 8); t /= 8;
    const int lane = (int)(t % 64); t /= 64;
    const int cb = (int)(t % NCB); t /= NCB;
    const int c = (int)(t % NC); t /= NC;
    const int chunk = (int)(t % nchunk); t /= nchunk;
    const int g = lane >> 4, n = lane & 15;
    PackIndex x;
    x.k = (int)t;
    x.grp = 0;
    x.ci = chunk * cic + 32 * c + 8 * g + j;
    x.co = (n >> 2) * (cout / 4) + 4 * cb + (n & 3);
    x.valid = true;
    return x;
  }
};

// channel-split kernels (conv_mfma_cs.hip): packed[k][chunk][cs][s][lane][j], lane = (h << 5) | m:
//   ci = chunk*64 + 16*s + 8*h + j                      (the K index of the MFMA: natural channel order)
//   co = cs*32 + 16*((m >> 2) & 1) + 4*(m >> 3) + (m & 3)
// so that the C fragment of lane (h', n) holds output channels cs*32 + 16*h' + reg, reg = 0..15, of row n.  A last chunk
// of 32 channels is zero-padded to 64.  Outputs wider than 128 channels: `cout / cob` images of `cob` channels behind
// each other (column block on grid.y of the main kernel), each the image of w[:, :, cb * cob : (cb + 1) * cob].
struct PackCs : PackShape {
  int cob;
  __host__ __device__ int nchunk() const { return (cin + kCsCIC - 1) / kCsCIC; }
  __host__ __device__ int64_t elements() const { return (int64_t)K * nchunk() * kCsCIC * cout; }
  __device__ PackIndex at(int64_t e) const {
    const int WC = cob / 32;
    const int64_t image = (int64_t)K * nchunk() * kCsCIC * cob;
    const int cb = (int)(e / image);
    int64_t t = e - cb * image;
    const int j = (int)(t % 8); t /= 8;
    const int lane = (int)(t % 64); t /= 64;
    const int s = (int)(t % 4); t /= 4;
    const int cs = (int)(t % WC); t /= WC;
    const int chunk = (int)(t % nchunk()); t /= nchunk();
    const int h = lane >> 5, m = lane & 31;
    PackIndex x;
    x.k = (int)t;
    x.grp = 0;
    x.ci = chunk * kCsCIC + 16 * s + 8 * h + j;
    x.co = cb * cob + cs * 32 + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
    x.valid = x.ci < cin;
    return x;
  }
};

// TS -> TD: fp32 master weights are rounded to nearest even (what `.to(bf16 / f16)` does) while they are packed - one
// launch instead of a cast kernel plus a pack kernel per convolution and direction
template <typename Layout, typename TS, typename TD>
__device__ __forceinline__ void pack_element(const Layout& L, const TS* __restrict__ w, TD* __restrict__ packed, int64_t e,
                                             int transpose, int flip) {
  if (e >= L.elements()) return;
  const PackIndex x = L.at(e);
  const int64_t kg = (int64_t)(flip ? (L.K - 1 - x.k) : x.k) * L.groups + x.grp;
  const int64_t src = transpose ? ((kg * L.cout + x.co) * L.cin + x.ci) : ((kg * L.cin + x.ci) * L.cout + x.co);
  packed[e] = x.valid ? (TD)w[src] : (TD)0;
}

template <typename Layout, typename TS, typename TD>
__global__ void pack_weight_kernel(const Layout L, const TS* __restrict__ w, TD* __restrict__ packed, int transpose, int flip) {
  pack_element(L, w, packed, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, transpose, flip);
}

// Both images of a training step in ONE launch: blockIdx.y = 0 the forward image of w [K, cin, cout], 1 the dgrad image
// (kernel-side roles exchanged: reduce over cout, produce cin; transposed, k-flipped for a submanifold map).  An optimizer step
// invalidates both at once, so every layer of a network saves a launch per iteration.
template <typename TD>
__global__ void pack_weight_cs_pair_kernel(const PackCs fwd, const PackCs dgrad, const float* __restrict__ w,
                                           TD* __restrict__ packed_fwd, TD* __restrict__ packed_dgrad, int flip_dgrad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.y == 0) pack_element(fwd, w, packed_fwd, e, 0, 0);
  else pack_element(dgrad, w, packed_dgrad, e, 1, flip_dgrad);
}

template <typename Layout>
static int launch_pack(const Layout& L, const void* w, int w_is_f32, int dtype, int transpose, int flip, void* packed,
                       hipStream_t s) {
  const dim3 grid((unsigned)ceil_div(L.elements(), 256)), block(256);
  if (!w_is_f32) {  // bf16 and f16 are both 2-byte moves
    hipLaunchKernelGGL((pack_weight_kernel<Layout, uint16_t, uint16_t>), grid, block, 0, s, L, (const uint16_t*)w,
                       (uint16_t*)packed, transpose, flip);
    return launch_status();
  }
  return with_dtype16(dtype, [&](auto t) {
    typedef decltype(t) TD;
    hipLaunchKernelGGL((pack_weight_kernel<Layout, float, TD>), grid, block, 0, s, L, (const float*)w, (TD*)packed,
                       transpose, flip);
    return launch_status();
  });
}

// the layout of the packed image follows the kernel that will consume it (a pure function of the shape)
int pack_weight_mfma(const void* w, int w_is_f32, int K, int cin, int cout, int dtype, int transpose, int flip, void* packed,
                     hipStream_t s) {
  switch (gather_gemm_family(cin, cout, K, dtype)) {
    case GemmFamily::ChannelSplit:
      return launch_pack(PackCs{{K, cin, cout, 1}, cs_col_block(cout)}, w, w_is_f32, dtype, transpose, flip, packed, s);
    case GemmFamily::Mfma16:
      return launch_pack(Pack16{{K, cin, cout, 1}, mfma16_chunk(cin, cout)}, w, w_is_f32, dtype, transpose, flip, packed, s);
    case GemmFamily::Mfma32:
    case GemmFamily::None: {
      // (None: a shape no kernel takes - K above the limit, an output width that is not instantiated - is still packed
      // in the 32x32x16 layout where that layout exists, as it always was; the launcher refuses it.)
      const int cic = mfma32_chunk(cin);
      if (cic == 0 || cout % 32 != 0 || (dtype != WCN_F16 && dtype != WCN_BF16)) return WCN_ERROR_UNSUPPORTED_CONFIG;
      return launch_pack(Pack32{{K, cin, cout, 1}, cic}, w, w_is_f32, dtype, transpose, flip, packed, s);
    }
  }
  return WCN_ERROR_UNSUPPORTED_CONFIG;  // (not reached: the switch names every family)
}

// grouped weights [K, G, cin, cout] (forward layout; cin / cout per group): always the 32x32x16 layout, one launch
int pack_weight_grouped(const void* w, int w_is_f32, int K, int groups, int cin, int cout, int dtype, int transpose, int flip,
                        void* packed, hipStream_t s) {
  if (groups < 1 || !mfma32_shape(cin, cout) || (dtype != WCN_F16 && dtype != WCN_BF16)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  return launch_pack(Pack32{{K, cin, cout, groups}, mfma32_chunk(cin)}, w, w_is_f32, dtype, transpose, flip, packed, s);
}

// forward + dgrad images of an fp32 master weight in one launch; both directions must be the channel-split family's shapes
int pack_weight_cs_pair(const float* w, int K, int cin, int cout, int dtype, int flip_dgrad, void* packed_fwd,
                        void* packed_dgrad, hipStream_t s) {
  if (!gather_gemm_cs_supported(cin, cout, K, dtype) || !gather_gemm_cs_supported(cout, cin, K, dtype))
    return WCN_ERROR_UNSUPPORTED_CONFIG;
  const PackCs fwd{{K, cin, cout, 1}, cs_col_block(cout)}, dgrad{{K, cout, cin, 1}, cs_col_block(cin)};
  const int64_t total = fwd.elements() > dgrad.elements() ? fwd.elements() : dgrad.elements();
  const dim3 grid((unsigned)ceil_div(total, 256), 2), block(256);
  return with_dtype16(dtype, [&](auto t) {
    typedef decltype(t) TD;
    hipLaunchKernelGGL((pack_weight_cs_pair_kernel<TD>), grid, block, 0, s, fwd, dgrad, w, (TD*)packed_fwd, (TD*)packed_dgrad,
                       flip_dgrad);
    return launch_status();
  });
}

}  // namespace wcn
