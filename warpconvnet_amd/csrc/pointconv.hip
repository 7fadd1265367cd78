// pointconv.hip - the PointConv edge pipeline in one pass (gfx950, fp32 on the matrix cores).
//
// Reference: warpconvnet/nn/modules/point_conv.py:231-273 (gather neighbour / query features, concatenate, edge MLP,
// reduce over the neighbours of a query) with the edge MLP of warpconvnet/nn/modules/mlp.py:124-177
// (Linear - LayerNorm - ReLU - Linear - LayerNorm, + identity shortcut).  The reference materialises the
// [M*k, C] edge tensors in HBM between every one of those steps; here an edge never leaves the chip:
//
//   x_e = [in_feats[nbr[e]] | q_feats[q(e)] | in_xyz[nbr[e]] - q_xyz[q(e)]]          gathered into registers
//   h   = ReLU(LN1(W1 x_e + b1)),  o = LN2(W2 h + b2) + shortcut(x_e),  out[q] = sum|mean_e o   (forward)
//   and the whole backward of that chain, recomputing the forward per tile                       (backward)
//
// Both kernels walk 32-edge tiles, for uniform lists (1 << log2k edges a query) and ragged ones (a query id per edge).
// All GEMMs are v_mfma_f32_32x32x2_f32 in the TRANSPOSED form (rows = channels, columns = the 32 edges):
//   * a result tile puts edge e in lane e / e+32 and 16 channels in registers, channel sigma(r, h) = 8*(r/4) + 4*h + r%4;
//   * that is exactly a B operand (k-pair = channels sigma(r,0), sigma(r,1)) of the next GEMM, so GEMM1 -> LN -> ReLU ->
//     GEMM2 and the whole data-gradient chain run register to register, the permutation folded into the packed weights.
//
// pointconv_fwd_wave_kernel - the forward of every list kind.  One tile per WAVE: a wave owns all hidden channels of its
//   tile, LayerNorm reduces over registers + one lane swap, nothing is exchanged between the waves.  The operand images
//   (P1, P2, tables, Linear shortcut) sit in LDS once per persistent workgroup.
// pointconv_bwd_kernel - the backward of every list kind ("tensor parallel workgroup").  One tile per workgroup of 4
//   waves: every wave holds the tile's x, wave w owns hidden channels [w*HID/4, (w+1)*HID/4) through the whole chain, so
//   the weight-gradient blocks it accumulates (its rows of dW1 / dW2) live in registers for the lifetime of the kernel.
//   * LayerNorm reduces over registers + one lane swap + a 1.5-KiB exchange between the waves;
//   * only the weight-gradient GEMMs (reduction over edges) need the other orientation: the operands take one trip
//     through a wave-private LDS tile [channel][edge];
//   * the forward operands (P1, P2) stay in registers, the transposed images (P2T, P1T) in LDS; the Linear shortcut's
//     transposed image is read from global memory (L1/L2 resident, 16 B per lane).
//
// LayerNorm variance.  Never sum(v * v) / n - mu * mu: with a mean far from zero (a large Linear bias, W1 rows with a common
// component) that difference of two large numbers loses the variance - at mean / sigma = 30 the normalised value is off by
// 5e-4 in fp32, at 1000 by its own size.  Both kernels take the mean first and then sum the squared deviations, which are
// differences of nearby numbers.  Padded channels hold exact zeros, not the mean, so they are kept out of that sum by
// comparing the (compile-time) channel index with hid_t / co_t (a uniform branch skips the comparisons when the width is
// the padded one); subtracting n_pad * mu^2 afterwards would bring the cancellation back.  Where one wave holds all channels of an edge (forward, LayerNorm 2 of the backward) this is a second
// pass over the registers and one lane swap.  LayerNorm 1 of the backward spans the four waves and keeps its single
// barrier: wave w deviates from its OWN mean m_w (of its n_w true channels) and sends m_w, q_w = sum (v - m_w)^2 and
// r_w = sum (v - m_w), which is zero but for the rounding of m_w.  Every lane then merges, with mu = sum (n_w m_w + r_w) / n:
//   sum (v - mu)^2 = sum_w [ q_w + 2 (m_w - mu) r_w + n_w (m_w - mu)^2 ]
// (Chan's merge, with the r_w term the identity holds for ANY m_w, so the rounding of the wave means does not enter the
// between-waves term in first order).
#include <type_traits>

#include "wcn_common.h"

namespace wcn {
namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kPcWaves = 4;  // waves of a backward workgroup
constexpr int kPcMaxGrid = 256;  // persistent workgroups of either kernel, one per CU (pinned in tests/test_grid_cap_constants.py)
constexpr int kPitch = 36;  // floats per row of the [channel][32 edges] LDS tiles: b128 reads of 8 lanes hit 32 banks

__host__ __device__ constexpr int sigma(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float half_swap(float v) { return __shfl_xor(v, 32, 64); }
__device__ __forceinline__ float half_sum32(float v) {  // sum over the 32 lanes of a half
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Compile-time shape of one kernel instance (channel counts padded with zeros up to it) and the packed-image layout.
template <int EIN_, int HID_, int CO_>
struct PC {
  static constexpr int EIN = EIN_, HID = HID_, CO = CO_;
  static constexpr int KS1 = EIN / 2;   // x registers per lane: lane half h holds channels [h*KS1, (h+1)*KS1)
  static constexpr int HB = HID / 128;  // hidden 32-blocks per wave
  static constexpr int NB1 = HID / 32, NB2 = CO / 32, NBX = EIN / 32;
  static constexpr int NBP = NB2 > NBX ? NB2 : NBX;
  static_assert(EIN % 32 == 0 && HID % 128 == 0 && CO % 32 == 0, "tile shape");
  // packed image (floats)
  static constexpr int OFF_P1 = 0;                    // [NB1][KS1/4][64][4]      GEMM1 A: W1[c = h*KS1+s][hid = 32blk+i]
  static constexpr int OFF_P2 = OFF_P1 + EIN * HID;   // [NB1][NB2][4][64][4]     GEMM2 A: W2[hid = 32blk+sigma(r,h)][out = 32b+i]
  static constexpr int OFF_P2T = OFF_P2 + HID * CO;   // [NB1][NB2][4][64][4]     dH A:    W2[hid = 32blk+i][out = 32b+sigma(r,h)]
  static constexpr int OFF_P1T = OFF_P2T + HID * CO;  // [NB1][NBX][4][64][4]     dX A:    W1[c = 32cb+i][hid = 32blk+sigma(r,h)]
  static constexpr int OFF_T1 = OFF_P1T + EIN * HID;  // [NB1][3][2][16]          b1, g1, be1 at channel 32blk+sigma(r,h)
  static constexpr int OFF_T2 = OFF_T1 + NB1 * 96;    // [NB2][3][2][16]          b2, g2, be2
  static constexpr int OFF_PS = OFF_T2 + NB2 * 96;    // [NB2][KS1/4][64][4]      shortcut A: Ws[c = h*KS1+s][out = 32b+i]
  static constexpr int OFF_PST = OFF_PS + EIN * CO;   // [NBX][NB2][4][64][4]     dX A:       Ws[c = 32cb+i][out = 32b+sigma(r,h)]
  static constexpr int OFF_TS = OFF_PST + EIN * CO;   // [NB2][2][16]             bs
  static constexpr int PACKED = OFF_TS + NB2 * 32;
  // LDS of the forward (floats): the images it reads, P1 | P2 | T1 | T2 | PS | TS
  static constexpr int LDS_FLOATS_WAVE = OFF_P2T + (NB1 + NB2) * 96 + EIN * CO + NB2 * 32;
  static constexpr int WSB = (NBX * NB2 + kPcWaves - 1) / kPcWaves;  // backward: dWs blocks per wave
  // LDS of the backward (floats)
  static constexpr int L_TAB = 0;                             // [NB1 + NB2][3][2][16] bias / LayerNorm tables (copy of T1, T2)
  static constexpr int L_TX = (NB1 + NB2) * 96;               // [EIN][kPitch]      x, channel-major (dW1 / dWs A)
  static constexpr int L_TH = L_TX + EIN * kPitch;            // [HID][kPitch]      per wave: H, later dHpre, channel-major
  static constexpr int L_TB = L_TH + HID * kPitch;            // [CO][kPitch]       dOpre channel-major
  static constexpr int L_PO = L_TB + CO * kPitch;             // [4][NBP][16][64]   partial tiles exchanged between the waves
  static constexpr int L_ST = L_PO + kPcWaves * NBP * 1024;   // [4][32][3] LayerNorm 1 statistics | [4][32][2] its backward sums
  static constexpr int ST_LN1 = kPcWaves * 32 * 3;            //                    offset of the second part inside st
  static constexpr int L_DXT = L_ST + kPcWaves * 32 * 5;      // [32][EIN+1]        dX, edge-major; before that dy channel-major [CO][kPitch]
  static constexpr int DXT_FLOATS = ((32 * (EIN + 1) > CO * kPitch ? 32 * (EIN + 1) : CO * kPitch) + 3) & ~3;
  static constexpr int L_DOUT = L_DXT + DXT_FLOATS;           // [32][CO] grad_out rows of the tile's queries ([32][CO+1] per edge when ragged)
  static constexpr int L_JT = L_DOUT + 32 * (CO + 1);         // [32] int           neighbour ids, then [32] int query ids (ragged lists)
  static constexpr int L_WT = L_JT + 64;                      // [HID*CO + EIN*HID]  P2T | P1T operand images
  static constexpr int LDS_FLOATS = L_WT + HID * CO + EIN * HID;
  static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};
// the two layouts of the instantiated shape, pinned: a slip in an offset above fails here
static_assert(PC<64, 128, 64>::LDS_FLOATS * 4 == 157824, "backward LDS layout");
static_assert(PC<64, 128, 64>::LDS_FLOATS_WAVE * 4 == 84480, "forward LDS layout");

struct PcArgs {
  const float* in_feats;  // [n_in][cin]
  const float* q_feats;   // [n_query][cq]
  const float* in_xyz;    // [n_in][3]     (nrel == 3)
  const float* q_xyz;     // [n_query][3]
  const int32_t* nbr;     // [n_query * k]
  int64_t n_query;
  int32_t log2k, cin, cq, nrel;
  const float* packed;
  int32_t ein_t, hid_t, co_t;  // true channel counts
  float eps1, eps2, scale;     // scale: 1 (sum) or 1/k (mean)
  int32_t lin_sc;              // 0: identity shortcut (ein == cout), 1: Linear shortcut
  // ragged neighbour lists (radius search): query id of every edge, per-query reduction scale (1 / count for mean, NULL = 1),
  // number of edges; edge_q == NULL: uniform lists of 1 << log2k edges
  const int32_t* edge_q;
  const float* q_scale;
  int64_t n_edges;
  float* out;                  // forward:  [n_query][co_t]
  const float* grad_out;       // backward: [n_query][co_t]
  float* d_in;                 //           [n_in][cin], zero-filled by the caller (accumulated with atomics)
  float* d_edge;               //           deterministic mode (uniform lists): [n_edges][cin] per-edge input gradients, plain
                               //           stores instead of the atomics on d_in; the caller sums them per input row
  float* d_q;                  //           [n_query][cq]
  float* partial;              //           [grid][grad floats] per-workgroup parameter-gradient partials
};

// gradient blob (floats, torch layouts): dW1 [hid][ein] | db1 | dg1 | dbe1 | dW2 [co][hid] | db2 | dg2 | dbe2
//                                         (+ dWs [co][ein] | dbs with a Linear shortcut)
__host__ __device__ inline int64_t grad_floats(int ein_t, int hid_t, int co_t, int lin_sc) {
  return (int64_t)hid_t * ein_t + 3 * hid_t + (int64_t)co_t * hid_t + 3 * co_t + (lin_sc ? (int64_t)co_t * ein_t + co_t : 0);
}

template <int EIN, int HID, int CO, bool LIN, bool RAG>
__global__ __launch_bounds__(256, 1) void pointconv_bwd_kernel(const PcArgs a) {
  typedef PC<EIN, HID, CO> P;
  constexpr int KS1 = P::KS1, HB = P::HB, NB2 = P::NB2, NBX = P::NBX, NBP = P::NBP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tX = smem + P::L_TX;
  float* tH = smem + P::L_TH;
  float* tB = smem + P::L_TB;
  float* po = smem + P::L_PO;
  float* st = smem + P::L_ST;
  float* dxt = smem + P::L_DXT;
  float* tD = dxt;  // dy channel-major (Linear shortcut), dead before dxt is written
  float* dout = smem + P::L_DOUT;
  int32_t* jt = reinterpret_cast<int32_t*>(smem + P::L_JT);
  int32_t* qt = jt + 32;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, e = lane & 31;
  const int k = 1 << a.log2k, nq = 32 >> a.log2k;
  constexpr bool ragged = RAG;  // neighbour lists of any length (per-edge query ids) instead of uniform 1 << log2k
  const int64_t n_edges = ragged ? a.n_edges : (a.n_query << a.log2k);
  const int64_t ntiles = (n_edges + 31) >> 5;
  const float inv_hid = 1.f / (float)a.hid_t, inv_co = 1.f / (float)a.co_t;
  const bool full1 = a.hid_t == HID, full2 = a.co_t == CO;  // no padded channels: the LayerNorm sums take every register
  const f32x4* pk4 = reinterpret_cast<const f32x4*>(a.packed);
  float* thw = tH + w * HB * 32 * kPitch;  // this wave's rows of tH
  const float* tab = smem + P::L_TAB;
  // true (not padded) hidden channels among the HB * 32 that wave ww owns
  auto true_channels = [&](int hid_t, int ww) { return min(max(hid_t - 32 * HB * ww, 0), 32 * HB); };
  for (int i = tid; i < (P::NB1 + NB2) * 96; i += 256) smem[P::L_TAB + i] = a.packed[P::OFF_T1 + i];
  // the transposed weight images (A operands of the dH and dX GEMMs) live in LDS: no global round trip per tile
  for (int i = tid; i < (P::OFF_T1 - P::OFF_P2T) / 4; i += 256)
    reinterpret_cast<f32x4*>(smem + P::L_WT)[i] = pk4[P::OFF_P2T / 4 + i];
  __syncthreads();
  const f32x4* pkT4 = reinterpret_cast<const f32x4*>(smem + P::L_WT) - P::OFF_P2T / 4;  // same indexing as pk4

  // persistent parameter-gradient accumulators
  f32x16 dW1a[NBX][HB], dW2a[HB][NB2];
  float dg1a[HB][16], dbe1a[HB][16], db1a[HB][16];
  float dg2a[NB2 * 4], dbe2a[NB2 * 4], db2a[NB2 * 4];  // this wave's quarter: items (b*16 + r) with (b*16+r) % 4 == w
  f32x16 dWsa[LIN ? P::WSB : 1];                                 // Linear shortcut: blocks (cb, b) with (cb*NB2 + b) % 4 == w
#pragma unroll
  for (int cb = 0; cb < NBX; ++cb)
#pragma unroll
    for (int t = 0; t < HB; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) dW1a[cb][t][q] = 0.f;
#pragma unroll
  for (int t = 0; t < HB; ++t)
#pragma unroll
    for (int b = 0; b < NB2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) dW2a[t][b][q] = 0.f;
#pragma unroll
  for (int t = 0; t < HB; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dg1a[t][r] = dbe1a[t][r] = db1a[t][r] = 0.f;
#pragma unroll
  for (int i = 0; i < NB2 * 4; ++i) dg2a[i] = dbe2a[i] = db2a[i] = 0.f;
#pragma unroll
  for (int jb = 0; jb < (LIN ? P::WSB : 1); ++jb)
#pragma unroll
    for (int q = 0; q < 16; ++q) dWsa[jb][q] = 0.f;

  // ---- this wave's forward weight operands never change: they stay in registers for the whole kernel ----
  float wA1[HB][KS1], wA2[HB][NB2][16];
#pragma unroll
  for (int t = 0; t < HB; ++t) {
    const int blk = w * HB + t;
    const f32x4* pa = pk4 + P::OFF_P1 / 4 + (blk * (KS1 / 4)) * 64 + lane;
#pragma unroll
    for (int s4 = 0; s4 < KS1 / 4; ++s4) {
      const f32x4 av = pa[s4 * 64];
#pragma unroll
      for (int d = 0; d < 4; ++d) wA1[t][4 * s4 + d] = av[d];
    }
#pragma unroll
    for (int b = 0; b < NB2; ++b)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const f32x4 av = pk4[P::OFF_P2 / 4 + ((blk * NB2 + b) * 4 + r4) * 64 + lane];
#pragma unroll
        for (int d = 0; d < 4; ++d) wA2[t][b][4 * r4 + d] = av[d];
      }
  }

  // ---- software pipeline over tiles: the rows of tile i+1 are requested right after GEMM1 of tile i has consumed x,
  // the neighbour ids of tile i+2 with them ----
  auto load_ids = [&](int64_t tile, bool& valid, int64_t& q, int32_t& j) {
    const int64_t E = tile * 32 + e;
    valid = tile < ntiles && E < n_edges;
    q = valid ? (ragged ? (int64_t)a.edge_q[E] : (E >> a.log2k)) : 0;
    j = valid ? a.nbr[E] : 0;
  };
  float x[KS1];
  // x_e of one edge: 16-B loads where four channels lie inside one feature row, else channel by channel (row tails,
  // relative positions).  Written out here and in the wave kernel: as one shared function it changes the register
  // allocation of all eight instances (docs/OPTIMISATION_LOG.md, section P).
  auto gather_x = [&](bool valid, int64_t q, int32_t j) {
    const float* fi = a.in_feats + (int64_t)j * a.cin;
    const float* fq = a.q_feats + q * a.cq;
    const bool vec = ((a.cin | a.cq) & 3) == 0;
#pragma unroll
    for (int u = 0; u < KS1 / 4; ++u) {
      const int c4 = h * KS1 + 4 * u;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid) {
        if (vec && c4 + 4 <= a.cin) {
          v = *reinterpret_cast<const f32x4*>(fi + c4);
        } else if (vec && c4 >= a.cin && c4 + 4 <= a.cin + a.cq) {
          v = *reinterpret_cast<const f32x4*>(fq + (c4 - a.cin));
        } else {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int c = c4 + d;
            float sv = 0.f;
            if (c < a.cin) sv = fi[c];
            else if (c < a.cin + a.cq) sv = fq[c - a.cin];
            else if (c < a.cin + a.cq + a.nrel) sv = a.in_xyz[(int64_t)j * 3 + (c - a.cin - a.cq)] - a.q_xyz[q * 3 + (c - a.cin - a.cq)];
            v[d] = sv;
          }
        }
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) x[4 * u + d] = v[d];
    }
  };
  bool v_cur, v_nxt;
  int64_t q_cur, q_nxt;
  int32_t j_cur, j_nxt;
  load_ids(blockIdx.x, v_cur, q_cur, j_cur);
  gather_x(v_cur, q_cur, j_cur);
  load_ids((int64_t)blockIdx.x + gridDim.x, v_nxt, q_nxt, j_nxt);

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---- A. stage the tile: neighbour ids, grad_out rows, channel-major copy of x ----
    const bool valid = v_cur;
    if (w == 0 && h == 0) qt[e] = valid ? (int32_t)q_cur : -1;
    if (w == 0 && h == 0) jt[e] = valid ? j_cur : -1;
    if (ragged) {  // grad_out row of every edge's query, scaled (pitch CO + 1: lanes = edges read one column)
      for (int i = tid; i < 32 * CO; i += 256) {
        const int ee = i / CO, ch = i - ee * CO;
        const int64_t Ee = tile * 32 + ee;
        float v = 0.f;
        if (Ee < n_edges && ch < a.co_t) {
          const int64_t qv = a.edge_q[Ee];
          v = a.grad_out[qv * a.co_t + ch] * (a.q_scale ? a.q_scale[qv] : a.scale);
        }
        dout[ee * (CO + 1) + ch] = v;
      }
    } else {
      for (int i = tid; i < nq * CO; i += 256) {
        const int ql = i / CO, ch = i - ql * CO;
        const int64_t qq = tile * nq + ql;
        dout[i] = (qq < a.n_query && ch < a.co_t) ? a.grad_out[qq * a.co_t + ch] * a.scale : 0.f;
      }
    }
#pragma unroll
    for (int s = 0; s < KS1; ++s)  // every wave writes a quarter of the registers
      if ((s & 3) == w) tX[(h * KS1 + s) * kPitch + e] = x[s];

    // ---- GEMM1 (this wave's hidden blocks): Hpre^T = W1^T x^T + b1 ----
    f32x16 acc1[HB];
#pragma unroll
    for (int t = 0; t < HB; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[t][r] = 0.f;
#pragma unroll
      for (int s = 0; s < KS1; ++s) acc1[t] = mfma(wA1[t][s], x[s], acc1[t]);
    }
    // x is consumed: next tile's rows, and the ids of the tile after it
    v_cur = v_nxt; q_cur = q_nxt; j_cur = j_nxt;
    gather_x(v_cur, q_cur, j_cur);
    load_ids(tile + 2 * (int64_t)gridDim.x, v_nxt, q_nxt, j_nxt);

    // LayerNorm 1 statistics over the four waves with one exchange: wave w sends the mean m_w of its n_w true channels,
    // q_w = sum (v - m_w)^2 and r_w = sum (v - m_w) over them; the header comment has the merge.
    const int nw1 = true_channels(a.hid_t, w);
    {
      float s1 = 0.f;
#pragma unroll
      for (int t = 0; t < HB; ++t) {
        const float* t1 = tab + (w * HB + t) * 96 + h * 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc1[t][r] += t1[r];
          s1 += acc1[t][r];
        }
      }
      s1 += half_swap(s1);
      const float mw = nw1 > 0 ? s1 / (float)nw1 : 0.f;
      const int lim = a.hid_t - 32 * HB * w - 4 * h;  // channel 32 (w HB + t) + sigma(r, h) is a true one: 32 t + sigma(r, 0) < lim
      float qw = 0.f, rw = 0.f;
      if (full1) {  // no padded channel (a uniform branch): every register counts
#pragma unroll
        for (int t = 0; t < HB; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float d = acc1[t][r] - mw;
            rw += d;
            qw = fmaf(d, d, qw);
          }
      } else {
#pragma unroll
        for (int t = 0; t < HB; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float d = (32 * t + sigma(r, 0) < lim) ? acc1[t][r] - mw : 0.f;
            rw += d;
            qw = fmaf(d, d, qw);
          }
      }
      qw += half_swap(qw);
      rw += half_swap(rw);
      if (h == 0) {
        st[(w * 32 + e) * 3 + 0] = mw;
        st[(w * 32 + e) * 3 + 1] = qw;
        st[(w * 32 + e) * 3 + 2] = rw;
      }
    }
    __syncthreads();  // 1: tX, st[0], (jt, dout)

    float mu1, rstd1;
    {
      float S1 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kPcWaves; ++ww)
        S1 += (float)true_channels(a.hid_t, ww) * st[(ww * 32 + e) * 3 + 0] + st[(ww * 32 + e) * 3 + 2];
      mu1 = S1 * inv_hid;
      float M2 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kPcWaves; ++ww) {
        const float dm = st[(ww * 32 + e) * 3 + 0] - mu1;
        M2 += st[(ww * 32 + e) * 3 + 1] + dm * (2.f * st[(ww * 32 + e) * 3 + 2] + (float)true_channels(a.hid_t, ww) * dm);
      }
      rstd1 = rsqrtf(fmaxf(M2, 0.f) * inv_hid + a.eps1);
    }
    float xh1[HB][16], H[HB][16];
#pragma unroll
    for (int t = 0; t < HB; ++t) {
      const float* t1 = tab + (w * HB + t) * 96 + h * 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        xh1[t][r] = (acc1[t][r] - mu1) * rstd1;
        H[t][r] = fmaxf(xh1[t][r] * t1[32 + r] + t1[64 + r], 0.f);
        thw[(t * 32 + sigma(r, h)) * kPitch + e] = H[t][r];
      }
    }

    // ---- GEMM2, partial over this wave's hidden channels; the waves exchange partial tiles through LDS ----
    {
      f32x16 o[NB2];
#pragma unroll
      for (int b = 0; b < NB2; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
#pragma unroll
        for (int t = 0; t < HB; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[b] = mfma(wA2[t][b][r], H[t][r], o[b]);
        f32x4* pw = reinterpret_cast<f32x4*>(po) + ((w * NBP + b) * 4) * 64 + lane;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f32x4 v = {o[b][4 * r4], o[b][4 * r4 + 1], o[b][4 * r4 + 2], o[b][4 * r4 + 3]};
          pw[r4 * 64] = v;
        }
      }
    }
    __syncthreads();  // 2: po

    float xh2[NB2][16];  // normalised GEMM2 output
    float mu2, rstd2;
    {
      float s1b = 0.f;
#pragma unroll
      for (int b = 0; b < NB2; ++b) {
        const float* t2 = tab + (P::NB1 + b) * 96 + h * 16;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ww = 0; ww < kPcWaves; ++ww) v += reinterpret_cast<const f32x4*>(po)[((ww * NBP + b) * 4 + r4) * 64 + lane];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int r = 4 * r4 + d;
            const float ov = v[d] + t2[r];
            xh2[b][r] = ov;
            s1b += ov;
          }
        }
      }
      s1b += half_swap(s1b);
      mu2 = s1b * inv_co;
      const int lim = a.co_t - 4 * h;  // channel 32 b + sigma(r, h) is a true one: 32 b + sigma(r, 0) < lim
      float s2b = 0.f;  // squared deviations of the true channels (the padded ones hold 0, not the mean)
      if (full2) {
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) s2b = fmaf(xh2[b][r] - mu2, xh2[b][r] - mu2, s2b);
      } else {
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float d = (32 * b + sigma(r, 0) < lim) ? xh2[b][r] - mu2 : 0.f;
            s2b = fmaf(d, d, s2b);
          }
      }
      s2b += half_swap(s2b);
      rstd2 = rsqrtf(s2b * inv_co + a.eps2);
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) xh2[b][r] = (xh2[b][r] - mu2) * rstd2;
    }

    // ---- the forward is recomputed; from here on backward: dy -> LayerNorm2 -> dOpre ----
    float dOpre[NB2][16], dy[NB2][16];
    {
      const int ql = e >> a.log2k;
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dy[b][r] = !valid ? 0.f : ragged ? dout[e * (CO + 1) + 32 * b + sigma(r, h)] : dout[ql * CO + 32 * b + sigma(r, h)];
          const float gd = dy[b][r] * tab[(P::NB1 + b) * 96 + 32 + h * 16 + r];
          m1 += gd;
          m2 += gd * xh2[b][r];
        }
      m1 += half_swap(m1);
      m2 += half_swap(m2);
      m1 *= inv_co;
      m2 *= inv_co;
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dOpre[b][r] = rstd2 * (dy[b][r] * tab[(P::NB1 + b) * 96 + 32 + h * 16 + r] - m1 - xh2[b][r] * m2);
          if (((b * 16 + r) & 3) == w) {
            const int i = (b * 16 + r) >> 2;
            dg2a[i] += dy[b][r] * xh2[b][r];
            dbe2a[i] += dy[b][r];
            db2a[i] += dOpre[b][r];
            tB[(32 * b + sigma(r, h)) * kPitch + e] = dOpre[b][r];
            if (LIN) tD[(32 * b + sigma(r, h)) * kPitch + e] = dy[b][r];
          }
        }
    }
    // ---- dH (this wave's hidden blocks) = W2 dOpre, ReLU mask, LayerNorm1 backward (sums exchanged between the waves) ----
    float gg[HB][16];
    {
      float p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int t = 0; t < HB; ++t) {
        f32x16 dh;
#pragma unroll
        for (int r = 0; r < 16; ++r) dh[r] = 0.f;
#pragma unroll
        for (int b = 0; b < NB2; ++b) {
          const f32x4* pa = pkT4 + P::OFF_P2T / 4 + (((w * HB + t) * NB2 + b) * 4) * 64 + lane;
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 av = pa[r4 * 64];
#pragma unroll
            for (int d = 0; d < 4; ++d) dh = mfma(av[d], dOpre[b][4 * r4 + d], dh);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float g = H[t][r] > 0.f ? dh[r] : 0.f;
          dg1a[t][r] += g * xh1[t][r];
          dbe1a[t][r] += g;
          gg[t][r] = g * tab[(w * HB + t) * 96 + 32 + h * 16 + r];
          p1 += gg[t][r];
          p2 += gg[t][r] * xh1[t][r];
        }
      }
      p1 += half_swap(p1);
      p2 += half_swap(p2);
      if (h == 0) {
        st[P::ST_LN1 + (w * 32 + e) * 2 + 0] = p1;
        st[P::ST_LN1 + (w * 32 + e) * 2 + 1] = p2;
      }
    }
    __syncthreads();  // 3: st[1], tB

    float dHpre[HB][16];
    {
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kPcWaves; ++ww) {
        m1 += st[P::ST_LN1 + (ww * 32 + e) * 2 + 0];
        m2 += st[P::ST_LN1 + (ww * 32 + e) * 2 + 1];
      }
      m1 *= inv_hid;
      m2 *= inv_hid;
#pragma unroll
      for (int t = 0; t < HB; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dHpre[t][r] = rstd1 * (gg[t][r] - m1 - xh1[t][r] * m2);
          db1a[t][r] += dHpre[t][r];
        }
    }
    // ---- dW2 (rows of this wave) += H^T dOpre: the reduction runs over edges, operands channel-major from LDS ----
#pragma unroll
    for (int t = 0; t < HB; ++t)
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(thw + (t * 32 + e) * kPitch + 16 * h + 4 * s4);
          const f32x4 bv = *reinterpret_cast<const f32x4*>(tB + (32 * b + e) * kPitch + 16 * h + 4 * s4);
#pragma unroll
          for (int d = 0; d < 4; ++d) dW2a[t][b] = mfma(av[d], bv[d], dW2a[t][b]);
        }
    // the wave's tile now takes dHpre (LDS operations of one wave execute in order)
#pragma unroll
    for (int t = 0; t < HB; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) thw[(t * 32 + sigma(r, h)) * kPitch + e] = dHpre[t][r];
    // ---- dX partial = W1 dHpre over this wave's hidden channels ----
#pragma unroll
    for (int cb = 0; cb < NBX; ++cb) {
      f32x16 dx;
#pragma unroll
      for (int r = 0; r < 16; ++r) dx[r] = 0.f;
#pragma unroll
      for (int t = 0; t < HB; ++t) {
        const f32x4* pa = pkT4 + P::OFF_P1T / 4 + (((w * HB + t) * NBX + cb) * 4) * 64 + lane;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4 av = pa[r4 * 64];
#pragma unroll
          for (int d = 0; d < 4; ++d) dx = mfma(av[d], dHpre[t][4 * r4 + d], dx);
        }
      }
      if (LIN) {  // + Ws dy: the (cb, b) blocks are spread over the waves, the partial-tile sum adds them up
#pragma unroll
        for (int b = 0; b < NB2; ++b)
          if (((cb * NB2 + b) & 3) == w) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
              const f32x4 av = pk4[P::OFF_PST / 4 + ((cb * NB2 + b) * 4 + r4) * 64 + lane];
#pragma unroll
              for (int d = 0; d < 4; ++d) dx = mfma(av[d], dy[b][4 * r4 + d], dx);
            }
          }
      }
      f32x4* pw = reinterpret_cast<f32x4*>(po) + ((w * NBP + cb) * 4) * 64 + lane;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        f32x4 v = {dx[4 * r4], dx[4 * r4 + 1], dx[4 * r4 + 2], dx[4 * r4 + 3]};
        pw[r4 * 64] = v;
      }
    }
    // ---- dW1 (columns of this wave) += x^T dHpre ----
#pragma unroll
    for (int cb = 0; cb < NBX; ++cb)
#pragma unroll
      for (int t = 0; t < HB; ++t)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const f32x4 av = *reinterpret_cast<const f32x4*>(tX + (32 * cb + e) * kPitch + 16 * h + 4 * s4);
          const f32x4 bv = *reinterpret_cast<const f32x4*>(thw + (t * 32 + e) * kPitch + 16 * h + 4 * s4);
#pragma unroll
          for (int d = 0; d < 4; ++d) dW1a[cb][t] = mfma(av[d], bv[d], dW1a[cb][t]);
        }
    if (LIN) {  // dWs (this wave's blocks) += x^T dy
#pragma unroll
      for (int jb = 0; jb < P::WSB; ++jb) {
        const int id = jb * kPcWaves + w;
        if (id < NBX * NB2) {
          const int cb = id / NB2, b = id - cb * NB2;
#pragma unroll
          for (int s4 = 0; s4 < 4; ++s4) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(tX + (32 * cb + e) * kPitch + 16 * h + 4 * s4);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(tD + (32 * b + e) * kPitch + 16 * h + 4 * s4);
#pragma unroll
            for (int d = 0; d < 4; ++d) dWsa[jb] = mfma(av[d], bv[d], dWsa[jb]);
          }
        }
      }
    }
    __syncthreads();  // 4: po (dX partials); tD is dead

    // ---- dX: sum the partials (+ dy through the identity shortcut), edge-major tile, then scatter ----
#pragma unroll
    for (int cb = 0; cb < NBX; ++cb)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        if (((cb * 4 + r4) & 3) == w) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ww = 0; ww < kPcWaves; ++ww) v += reinterpret_cast<const f32x4*>(po)[((ww * NBP + cb) * 4 + r4) * 64 + lane];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int r = 4 * r4 + d;
            float s = v[d];
            if (!LIN && cb < NB2) s += dy[cb < NB2 ? cb : 0][r];  // identity shortcut: output channel c is x channel c
            dxt[e * (EIN + 1) + 32 * cb + sigma(r, h)] = s;
          }
        }
    __syncthreads();  // 5: dxt
    if (a.d_edge) {  // deterministic mode: the tile's 32 rows, whole rows by adjacent lanes
      for (int i = tid; i < 32 * a.cin; i += 256) {
        const int ee = i / a.cin, c = i - ee * a.cin;
        const int64_t E = tile * 32 + ee;
        if (E < n_edges) a.d_edge[E * a.cin + c] = jt[ee] >= 0 ? dxt[ee * (EIN + 1) + c] : 0.f;
      }
    } else {
      for (int i = tid; i < 32 * a.cin; i += 256) {
        const int ee = i / a.cin, c = i - ee * a.cin;
        const int32_t jj = jt[ee];
        if (jj >= 0) unsafeAtomicAdd(a.d_in + (int64_t)jj * a.cin + c, dxt[ee * (EIN + 1) + c]);  // hardware fp32 add, no CAS loop
      }
    }
    if (ragged) {
      // query-side gradient: segments of equal query id inside the tile; a list may continue in the next tile, so every
      // segment is ADDED to its (zero-filled) row.  Thread (part, c): 8 consecutive edges, flush when the query changes.
      for (int i = tid; i < 4 * a.cq; i += 256) {
        const int part = i / a.cq, c = i - part * a.cq;
        float acc = 0.f;
        int32_t qprev = -1;
        for (int ee = part * 8; ee < part * 8 + 8; ++ee) {
          const int32_t qv = qt[ee];
          if (qv != qprev) {
            if (qprev >= 0) unsafeAtomicAdd(a.d_q + (int64_t)qprev * a.cq + c, acc);
            acc = 0.f;
            qprev = qv;
          }
          if (qv >= 0) acc += dxt[ee * (EIN + 1) + a.cin + c];
        }
        if (qprev >= 0) unsafeAtomicAdd(a.d_q + (int64_t)qprev * a.cq + c, acc);
      }
    } else {
      for (int i = tid; i < nq * a.cq; i += 256) {
        const int ql = i / a.cq, c = i - ql * a.cq;
        const int64_t qq = tile * nq + ql;
        float s = 0.f;
        for (int kk = 0; kk < k; ++kk) s += dxt[(ql * k + kk) * (EIN + 1) + a.cin + c];
        if (qq < a.n_query) a.d_q[qq * a.cq + c] = s;
      }
    }
    __syncthreads();  // 6: LDS is rewritten by the next tile
  }

  // ---- this workgroup's parameter-gradient partials (every true element is written: the reduce kernel sums them) ----
  float* base = a.partial + (int64_t)blockIdx.x * grad_floats(a.ein_t, a.hid_t, a.co_t, LIN);
  float* pW1 = base;
  float* pb1 = pW1 + (int64_t)a.hid_t * a.ein_t;
  float* pg1 = pb1 + a.hid_t;
  float* pbe1 = pg1 + a.hid_t;
  float* pW2 = pbe1 + a.hid_t;
  float* pb2 = pW2 + (int64_t)a.co_t * a.hid_t;
  float* pg2 = pb2 + a.co_t;
  float* pbe2 = pg2 + a.co_t;
  float* pWs = pbe2 + a.co_t;  // [co][ein], then dbs [co]  (Linear shortcut)
  float* pbs = pWs + (int64_t)a.co_t * a.ein_t;
#pragma unroll
  for (int t = 0; t < HB; ++t) {
    const int hid0 = 32 * (w * HB + t);
#pragma unroll
    for (int cb = 0; cb < NBX; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // dW1a[cb][t][r] at lane (h, e): W1 grad (c = 32cb + sigma(r,h), hid = hid0 + e)
        const int c = 32 * cb + sigma(r, h), hid = hid0 + e;
        if (c < a.ein_t && hid < a.hid_t) pW1[(int64_t)hid * a.ein_t + c] = dW1a[cb][t][r];
      }
#pragma unroll
    for (int b = 0; b < NB2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {  // dW2a[t][b][r] at lane (h, e): W2 grad (hid = hid0 + sigma(r,h), out = 32b + e)
        const int hid = hid0 + sigma(r, h), oc = 32 * b + e;
        if (hid < a.hid_t && oc < a.co_t) pW2[(int64_t)oc * a.hid_t + hid] = dW2a[t][b][r];
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float vg = half_sum32(dg1a[t][r]), vb = half_sum32(dbe1a[t][r]), vc = half_sum32(db1a[t][r]);
      const int hid = hid0 + sigma(r, h);
      if (e == 0 && hid < a.hid_t) {
        pg1[hid] = vg;
        pbe1[hid] = vb;
        pb1[hid] = vc;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (((b * 16 + r) & 3) == w) {
        const int i = (b * 16 + r) >> 2;
        const float vg = half_sum32(dg2a[i]), vb = half_sum32(dbe2a[i]), vc = half_sum32(db2a[i]);
        const int oc = 32 * b + sigma(r, h);
        if (e == 0 && oc < a.co_t) {
          pg2[oc] = vg;
          pbe2[oc] = vb;
          pb2[oc] = vc;
          if (LIN) pbs[oc] = vb;  // d bs = sum of dy = d LN2.bias
        }
      }
  if (LIN) {
#pragma unroll
    for (int jb = 0; jb < P::WSB; ++jb) {
      const int id = jb * kPcWaves + w;
      if (id < NBX * NB2) {
        const int cb = id / NB2, b = id - cb * NB2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // dWsa[jb][r] at lane (h, e): Ws grad (c = 32cb + sigma(r,h), out = 32b + e)
          const int c = 32 * cb + sigma(r, h), oc = 32 * b + e;
          if (c < a.ein_t && oc < a.co_t) pWs[(int64_t)oc * a.ein_t + c] = dWsa[jb][r];
        }
      }
    }
  }
}

// Forward for uniform and ragged lists, one 32-edge tile per WAVE: nothing to exchange between the waves of a workgroup
// (every wave owns all hidden channels of its tile), so there is no barrier in the loop and two waves per SIMD overlap each
// other's gathers, LayerNorm arithmetic and MFMA chains.  The operand images sit in LDS once per (persistent) workgroup.
// The tensor-parallel decomposition above is the backward's alone: its point is the register-resident weight gradients.
// EIN = 64: lane half h holds x channels [32h, 32h + 32), so the identity shortcut is one lane swap.
template <int EIN, int HID, int CO, bool LIN, bool RAG>
__global__ __launch_bounds__(512, 1) void pointconv_fwd_wave_kernel(const PcArgs a) {
  typedef PC<EIN, HID, CO> P;
  constexpr int KS1 = P::KS1, NB1 = P::NB1, NB2 = P::NB2;
  static_assert(KS1 == 32 && CO <= EIN, "identity shortcut by lane swap");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sP = smem;                          // P1 | P2 (packed image prefix)
  float* sTab = sP + P::OFF_P2T;             // T1 | T2
  float* sPS = sTab + (NB1 + NB2) * 96;      // PS (Linear shortcut)
  float* sTS = sPS + EIN * CO;               // bs
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, e = lane & 31;
  for (int i = tid; i < P::OFF_P2T / 4; i += 512) reinterpret_cast<f32x4*>(sP)[i] = reinterpret_cast<const f32x4*>(a.packed)[i];
  for (int i = tid; i < (NB1 + NB2) * 96; i += 512) sTab[i] = a.packed[P::OFF_T1 + i];
  if (LIN) {
    for (int i = tid; i < EIN * CO / 4; i += 512)
      reinterpret_cast<f32x4*>(sPS)[i] = reinterpret_cast<const f32x4*>(a.packed + P::OFF_PS)[i];
    for (int i = tid; i < NB2 * 32; i += 512) sTS[i] = a.packed[P::OFF_TS + i];
  }
  __syncthreads();  // the only barrier: the waves are independent from here on

  const int k = 1 << a.log2k;
  const int64_t n_edges = RAG ? a.n_edges : (a.n_query << a.log2k);
  const int64_t ntiles = (n_edges + 31) >> 5;
  const float inv_hid = 1.f / (float)a.hid_t, inv_co = 1.f / (float)a.co_t;
  const bool full1 = a.hid_t == HID, full2 = a.co_t == CO;  // no padded channels: the LayerNorm sums take every register
  const int64_t nwaves = (int64_t)gridDim.x * 8;
  int64_t tile = (int64_t)blockIdx.x * 8 + (tid >> 6);
  // neighbour id of the first tile; the next tile's id is requested while the current tile is computed
  int32_t j_nxt = 0;
  if (tile < ntiles && tile * 32 + e < n_edges) j_nxt = a.nbr[tile * 32 + e];
  for (; tile < ntiles; tile += nwaves) {
    // the operand images never change, so the compiler would hoist all 512 registers' worth of LDS reads out of the tile
    // loop (and spill them): the LDS offsets are laundered per tile
    uint32_t o1 = (uint32_t)(P::OFF_P1 * 4 + lane * 16), o2 = (uint32_t)(P::OFF_P2 * 4 + lane * 16), ot = 0u;
    asm volatile("" : "+v"(o1), "+v"(o2), "+v"(ot));
    const f32x4* p1 = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(sP) + o1);
    const f32x4* p2 = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(sP) + o2);
    const float* sTabL = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sTab) + ot);
    const float* sPSL = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sPS) + ot);
    const float* sTSL = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sTS) + ot);
    const int64_t E = tile * 32 + e;
    const bool valid = E < n_edges;
    const int64_t q = valid ? (RAG ? (int64_t)a.edge_q[E] : (E >> a.log2k)) : -1;
    const int32_t j = j_nxt;
    {
      const int64_t En = (tile + nwaves) * 32 + e;
      j_nxt = (tile + nwaves < ntiles && En < n_edges) ? a.nbr[En] : 0;
    }
    float x[KS1];
    {  // the gather of the backward kernel (gather_x), q clamped for the lanes past the last edge
      const float* fi = a.in_feats + (int64_t)j * a.cin;
      const float* fq = a.q_feats + (q < 0 ? 0 : q) * a.cq;
      const bool vec = ((a.cin | a.cq) & 3) == 0;
#pragma unroll
      for (int u = 0; u < KS1 / 4; ++u) {
        const int c4 = h * KS1 + 4 * u;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
          if (vec && c4 + 4 <= a.cin) {
            v = *reinterpret_cast<const f32x4*>(fi + c4);
          } else if (vec && c4 >= a.cin && c4 + 4 <= a.cin + a.cq) {
            v = *reinterpret_cast<const f32x4*>(fq + (c4 - a.cin));
          } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              const int c = c4 + d;
              float sv = 0.f;
              if (c < a.cin) sv = fi[c];
              else if (c < a.cin + a.cq) sv = fq[c - a.cin];
              else if (c < a.cin + a.cq + a.nrel) sv = a.in_xyz[(int64_t)j * 3 + (c - a.cin - a.cq)] - a.q_xyz[q * 3 + (c - a.cin - a.cq)];
              v[d] = sv;
            }
          }
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) x[4 * u + d] = v[d];
      }
    }
    // ---- GEMM1 (all hidden blocks) + LayerNorm1 + ReLU ----
    f32x16 hb[NB1];
    float s1 = 0.f;
#pragma unroll
    for (int blk = 0; blk < NB1; ++blk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) hb[blk][r] = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KS1 / 4; ++s4) {
        const f32x4 av = p1[(blk * (KS1 / 4) + s4) * 64];
#pragma unroll
        for (int d = 0; d < 4; ++d) hb[blk] = mfma(av[d], x[4 * s4 + d], hb[blk]);
      }
      const float* t1 = sTabL + blk * 96 + h * 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        hb[blk][r] += t1[r];
        s1 += hb[blk][r];
      }
    }
    s1 += half_swap(s1);
    const float mu1 = s1 * inv_hid;
    const int lim1 = a.hid_t - 4 * h;  // channel 32 blk + sigma(r, h) is a true one: 32 blk + sigma(r, 0) < lim1
    float s2 = 0.f;  // squared deviations of the true channels (the padded ones hold 0, not the mean)
    if (full1) {  // no padded channel (a uniform branch): every register counts
#pragma unroll
      for (int blk = 0; blk < NB1; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) s2 = fmaf(hb[blk][r] - mu1, hb[blk][r] - mu1, s2);
    } else {
#pragma unroll
      for (int blk = 0; blk < NB1; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = (32 * blk + sigma(r, 0) < lim1) ? hb[blk][r] - mu1 : 0.f;
          s2 = fmaf(d, d, s2);
        }
    }
    s2 += half_swap(s2);
    const float rstd1 = rsqrtf(s2 * inv_hid + a.eps1);
#pragma unroll
    for (int blk = 0; blk < NB1; ++blk) {
      const float* t1 = sTabL + blk * 96 + h * 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) hb[blk][r] = fmaxf((hb[blk][r] - mu1) * rstd1 * t1[32 + r] + t1[64 + r], 0.f);
    }
    // ---- GEMM2 + LayerNorm2 + shortcut ----
    f32x16 o[NB2];
    float u1 = 0.f;
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[b][r] = 0.f;
#pragma unroll
      for (int blk = 0; blk < NB1; ++blk)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4 av = p2[((blk * NB2 + b) * 4 + r4) * 64];
#pragma unroll
          for (int d = 0; d < 4; ++d) o[b] = mfma(av[d], hb[blk][4 * r4 + d], o[b]);
        }
      const float* t2 = sTabL + (NB1 + b) * 96 + h * 16;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[b][r] += t2[r];
        u1 += o[b][r];
      }
    }
    u1 += half_swap(u1);
    const float mu2 = u1 * inv_co;
    const int lim2 = a.co_t - 4 * h;
    float u2 = 0.f;
    if (full2) {
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) u2 = fmaf(o[b][r] - mu2, o[b][r] - mu2, u2);
    } else {
#pragma unroll
      for (int b = 0; b < NB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = (32 * b + sigma(r, 0) < lim2) ? o[b][r] - mu2 : 0.f;
          u2 = fmaf(d, d, u2);
        }
    }
    u2 += half_swap(u2);
    const float rstd2 = rsqrtf(u2 * inv_co + a.eps2);
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
      const float* t2 = sTabL + (NB1 + b) * 96 + h * 16;
      f32x16 sc;
      if (LIN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s4 = 0; s4 < KS1 / 4; ++s4) {
          const f32x4 av = reinterpret_cast<const f32x4*>(sPSL)[(b * (KS1 / 4) + s4) * 64 + lane];
#pragma unroll
          for (int d = 0; d < 4; ++d) sc = mfma(av[d], x[4 * s4 + d], sc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] += sTSL[b * 32 + h * 16 + r];
      } else {
        // identity: output channel 32b + sigma(r, h) is x channel sigma(r, h) of lane half b (own half or the partner's)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float own = x[sigma(r, b)], other = half_swap(x[sigma(r, 1 - b)]);
          sc[r] = (h == b) ? own : other;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) o[b][r] = (o[b][r] - mu2) * rstd2 * t2[32 + r] + t2[64 + r] + sc[r];
    }
    if (RAG) {
      // ragged lists: segmented inclusive scan over the lanes of the tile (equal query ids are adjacent); the last lane
      // of every segment ADDS its total to the (zero-filled) output row - a list may continue in the next tile
      const int qi = (int)q;
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) {
        const int qo = __shfl_up(qi, off, 32);
        const bool take = e >= off && qo == qi && qi >= 0;
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = __shfl_up(o[b][r], off, 32);
            if (take) o[b][r] += v;
          }
      }
      const int qn = __shfl_down(qi, 1, 32);
      if (valid && (e == 31 || qn != qi)) {
        const float sc = a.q_scale ? a.q_scale[q] : a.scale;
        float* dst = a.out + q * a.co_t;
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = 32 * b + sigma(r, h);
            if (ch < a.co_t) unsafeAtomicAdd(dst + ch, o[b][r] * sc);
          }
      }
    } else {
      // ---- reduction over the k edges of a query (adjacent lanes), one store per query and channel ----
      for (int m = k >> 1; m >= 1; m >>= 1) {
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[b][r] += __shfl_xor(o[b][r], m, 64);
      }
      if (valid && (e & (k - 1)) == 0) {
        float* dst = a.out + q * a.co_t;
#pragma unroll
        for (int b = 0; b < NB2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = 32 * b + sigma(r, h);
            if (ch < a.co_t) dst[ch] = o[b][r] * a.scale;
          }
      }
    }
  }
}

// packs the torch-layout parameters into the operand images of PC<EIN, HID, CO>
struct PackArgs {
  const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2;  // w1 [hid][ein], w2 [co][hid]
  const float *ws, *bs;                                  // Linear shortcut [co][ein] / bias, or NULL
  int ein_t, hid_t, co_t;
  float* packed;
};
// One element of a packed image, decoded from its offset inside the image.  `i` is the MFMA row of the A operand (lane
// % 32), `blk` the index over the leading dimensions; the k index of the operand is
//   TFrag  [blk][r4][lane][4]:     channel sigma(4*r4 + d, lane / 32) of a 32-block - a result register of the GEMM in front
//   KFrag  [blk][s4][lane][4]:     channel (lane / 32) * KS1 + 4*s4 + d            - an x register
struct TFrag { int i, sg, blk; };
struct KFrag { int i, c, blk; };
__device__ __forceinline__ TFrag decode_tfrag(int o) {
  const int d = o & 3, lane = (o >> 2) & 63, r4 = (o >> 8) & 3;
  return {lane & 31, sigma(4 * r4 + d, lane >> 5), o >> 10};
}
template <int KS1>
__device__ __forceinline__ KFrag decode_kfrag(int o) {
  const int d = o & 3, lane = (o >> 2) & 63, rest = o >> 8;
  return {lane & 31, (lane >> 5) * KS1 + 4 * (rest % (KS1 / 4)) + d, rest / (KS1 / 4)};
}
// [blk][ROWS][2][16] table (ROWS = 3: bias, LayerNorm weight, LayerNorm bias): row and channel 32*blk + sigma(r, h)
struct TabElem { int row, ch; };
template <int ROWS>
__device__ __forceinline__ TabElem decode_tab(int o) {
  const int r = o & 15, hh = (o >> 4) & 1, rows = o >> 5;
  return {rows % ROWS, 32 * (rows / ROWS) + sigma(r, hh)};
}

template <int EIN, int HID, int CO>
__global__ void pointconv_pack_kernel(const PackArgs p) {
  typedef PC<EIN, HID, CO> P;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P::PACKED) return;
  auto W1 = [&](int c, int hid) { return (c < p.ein_t && hid < p.hid_t) ? p.w1[(int64_t)hid * p.ein_t + c] : 0.f; };
  auto W2 = [&](int hid, int oc) { return (hid < p.hid_t && oc < p.co_t) ? p.w2[(int64_t)oc * p.hid_t + hid] : 0.f; };
  auto WS = [&](int c, int oc) { return (p.ws && c < p.ein_t && oc < p.co_t) ? p.ws[(int64_t)oc * p.ein_t + c] : 0.f; };
  auto tab = [&](const float* src, int ch, int width) { return (ch < width && src) ? src[ch] : 0.f; };
  float v = 0.f;
  if (idx < P::OFF_P2) {  // P1 [blk][s4][lane][4]
    const KFrag f = decode_kfrag<P::KS1>(idx - P::OFF_P1);
    v = W1(f.c, 32 * f.blk + f.i);
  } else if (idx < P::OFF_P2T) {  // P2 [blk][b][r4][lane][4]
    const TFrag f = decode_tfrag(idx - P::OFF_P2);
    v = W2(32 * (f.blk / P::NB2) + f.sg, 32 * (f.blk % P::NB2) + f.i);
  } else if (idx < P::OFF_P1T) {  // P2T [blk][b][r4][lane][4]
    const TFrag f = decode_tfrag(idx - P::OFF_P2T);
    v = W2(32 * (f.blk / P::NB2) + f.i, 32 * (f.blk % P::NB2) + f.sg);
  } else if (idx < P::OFF_T1) {  // P1T [blk][cb][r4][lane][4]
    const TFrag f = decode_tfrag(idx - P::OFF_P1T);
    v = W1(32 * (f.blk % P::NBX) + f.i, 32 * (f.blk / P::NBX) + f.sg);
  } else if (idx < P::OFF_T2) {  // T1 [blk][3][2][16]
    const TabElem t = decode_tab<3>(idx - P::OFF_T1);
    v = tab(t.row == 0 ? p.b1 : t.row == 1 ? p.g1 : p.be1, t.ch, p.hid_t);
  } else if (idx < P::OFF_PS) {  // T2 [b][3][2][16]
    const TabElem t = decode_tab<3>(idx - P::OFF_T2);
    v = tab(t.row == 0 ? p.b2 : t.row == 1 ? p.g2 : p.be2, t.ch, p.co_t);
  } else if (idx < P::OFF_PST) {  // PS [b][s4][lane][4]
    const KFrag f = decode_kfrag<P::KS1>(idx - P::OFF_PS);
    v = WS(f.c, 32 * f.blk + f.i);
  } else if (idx < P::OFF_TS) {  // PST [cb][b][r4][lane][4]
    const TFrag f = decode_tfrag(idx - P::OFF_PST);
    v = WS(32 * (f.blk / P::NB2) + f.i, 32 * (f.blk % P::NB2) + f.sg);
  } else {  // TS [b][2][16]
    const TabElem t = decode_tab<1>(idx - P::OFF_TS);
    v = tab(p.bs, t.ch, p.co_t);
  }
  p.packed[idx] = v;
}

__global__ void pointconv_grad_reduce_kernel(const float* __restrict__ partial, int grid, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int g = 0; g < grid; ++g) s += partial[(int64_t)g * n + i];  // fixed order: deterministic
  out[i] = s;
}

// Instantiated shapes (EIN, HID, CO), one line each: f(PC<..>{}) for the shape of that index, false past the last one.
template <typename F>
bool with_shape(int index, F&& f) {
  switch (index) {
    case 0: f(PC<64, 128, 64>{}); return true;
    default: return false;
  }
}
// channel counts are zero-padded up to the first shape that fits; -1: none does
int pick_shape(int ein_t, int hid_t, int co_t) {
  bool fits = false;
  for (int i = 0; with_shape(i, [&](auto p) { fits = ein_t <= p.EIN && hid_t <= p.HID && co_t <= p.CO; }); ++i)
    if (fits) return i;
  return -1;
}
int log2_exact(int k) {
  for (int l = 0; l <= 5; ++l)
    if ((1 << l) == k) return l;
  return -1;
}
int bwd_grid(int64_t n_query, int k) {
  const int64_t tiles = (n_query * k + 31) / 32;
  return (int)(tiles < kPcMaxGrid ? tiles : kPcMaxGrid);  // one persistent workgroup per CU
}

// The two runtime flags of a launch as template flags: f(bool_constant<LIN>, bool_constant<RAG>).
template <typename F>
int with_lin_rag(const PcArgs& a, F&& f) {
  if (a.edge_q) return a.lin_sc ? f(std::true_type{}, std::true_type{}) : f(std::false_type{}, std::true_type{});
  return a.lin_sc ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{});
}

// Launches kernel_of(lin, rag), the <LIN, RAG> instance of a kernel for the flags of `a`; the instance's dynamic-LDS limit
// is raised on its first launch on a device (the static below exists once per instance).
template <typename KernelOf>
int launch_lin_rag(const PcArgs& a, KernelOf kernel_of, int grid, int threads, int lds_bytes, hipStream_t s) {
  return with_lin_rag(a, [&](auto lin, auto rag) {
    void (*const kernel)(PcArgs) = kernel_of(lin, rag);
    static unsigned long long attr_done = 0ull;
    const int rc = once_per_device(attr_done, [&] {
      return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 lds_bytes) == hipSuccess;
    });
    if (rc != WCN_SUCCESS) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds_bytes, s, a);
    return launch_status();
  });
}

template <typename P>
int launch_fwd_wave(const PcArgs& a, hipStream_t s) {
  const int64_t edges = a.edge_q ? a.n_edges : (a.n_query << a.log2k);
  const int64_t tiles = (edges + 31) / 32;
  const int64_t wgs = (tiles + 7) / 8;
  const int grid = (int)(wgs < kPcMaxGrid ? wgs : kPcMaxGrid);  // one persistent 8-wave workgroup per CU
  const auto kernel_of = [](auto lin, auto rag) {
    return pointconv_fwd_wave_kernel<P::EIN, P::HID, P::CO, decltype(lin)::value, decltype(rag)::value>;
  };
  return launch_lin_rag(a, kernel_of, grid, 512, P::LDS_FLOATS_WAVE * 4, s);
}

template <typename P>
int launch_bwd(const PcArgs& a, int grid, hipStream_t s) {
  const auto kernel_of = [](auto lin, auto rag) {
    return pointconv_bwd_kernel<P::EIN, P::HID, P::CO, decltype(lin)::value, decltype(rag)::value>;
  };
  return launch_lin_rag(a, kernel_of, grid, 256, P::LDS_FLOATS * 4, s);
}

}  // namespace
}  // namespace wcn

using namespace wcn;

extern "C" {

int wcn_pointconv_supported(int32_t cin, int32_t cq, int32_t nrel, int32_t hidden, int32_t cout, int32_t k,
                            int32_t linear_shortcut) {
  if (cin < 1 || cq < 0 || (nrel != 0 && nrel != 3) || hidden < 1 || cout < 1) return 0;
  if (!linear_shortcut && cin + cq + nrel != cout) return 0;  // identity shortcut needs equal widths (mlp.py:141)
  return (log2_exact(k) >= 0 && pick_shape(cin + cq + nrel, hidden, cout) >= 0) ? 1 : 0;
}

int64_t wcn_pointconv_packed_floats(int32_t ein, int32_t hidden, int32_t cout) {
  int64_t floats = 0;
  with_shape(pick_shape(ein, hidden, cout), [&](auto p) { floats = p.PACKED; });
  return floats;
}

int64_t wcn_pointconv_grad_floats(int32_t ein, int32_t hidden, int32_t cout, int32_t linear_shortcut) {
  return grad_floats(ein, hidden, cout, linear_shortcut);
}

size_t wcn_pointconv_backward_workspace(int64_t n_query, int32_t k, int32_t ein, int32_t hidden, int32_t cout,
                                        int32_t linear_shortcut) {
  return (size_t)bwd_grid(n_query, k) * (size_t)grad_floats(ein, hidden, cout, linear_shortcut) * sizeof(float);
}

int wcn_pointconv_pack(const float* w1, const float* b1, const float* g1, const float* be1, const float* w2,
                       const float* b2, const float* g2, const float* be2, const float* ws, const float* bs, int32_t ein,
                       int32_t hidden, int32_t cout, float* packed, void* stream) {
  if (!w1 || !w2 || !packed) return WCN_ERROR_INVALID_PARAMETERS;
  const PackArgs p{w1, b1, g1, be1, w2, b2, g2, be2, ws, bs, ein, hidden, cout, packed};
  hipStream_t s = (hipStream_t)stream;
  const bool launched = with_shape(pick_shape(ein, hidden, cout), [&](auto shape) {
    typedef decltype(shape) P;
    hipLaunchKernelGGL((pointconv_pack_kernel<P::EIN, P::HID, P::CO>), dim3((P::PACKED + 255) / 256), dim3(256), 0, s, p);
  });
  return launched ? launch_status() : WCN_ERROR_UNSUPPORTED_CONFIG;
}

static int fill_args(PcArgs& a, const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                     const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                     const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                     int32_t linear_shortcut) {
  if (!wcn_pointconv_supported(cin, cq, nrel, hidden, cout, k, linear_shortcut)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!in_feats || (cq > 0 && !q_feats) || !nbr || !packed || (nrel && (!in_xyz || !q_xyz)) || n_query < 0)
    return WCN_ERROR_INVALID_PARAMETERS;
  a = PcArgs{};
  a.in_feats = in_feats; a.q_feats = q_feats; a.in_xyz = in_xyz; a.q_xyz = q_xyz; a.nbr = nbr;
  a.n_query = n_query; a.log2k = log2_exact(k); a.cin = cin; a.cq = cq; a.nrel = nrel;
  a.packed = packed; a.ein_t = cin + cq + nrel; a.hid_t = hidden; a.co_t = cout;
  a.eps1 = eps1; a.eps2 = eps2; a.scale = mean ? 1.f / (float)k : 1.f; a.lin_sc = linear_shortcut ? 1 : 0;
  a.d_edge = nullptr;
  return WCN_SUCCESS;
}

// ragged lists: the query of every edge, the per-query reduction scale (or NULL) and the number of edges
static int set_ragged(PcArgs& a, const int32_t* edge_q, const float* q_scale, int64_t n_edges) {
  if (!edge_q || n_edges < 0) return WCN_ERROR_INVALID_PARAMETERS;
  a.edge_q = edge_q; a.q_scale = q_scale; a.n_edges = n_edges;
  return WCN_SUCCESS;
}

static int run_forward(PcArgs& a, float* out, hipStream_t s) {
  if (!out) return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t edges = a.edge_q ? a.n_edges : (a.n_query << a.log2k);
  if (a.n_query == 0 || edges == 0) return WCN_SUCCESS;
  a.out = out;
  int rc = WCN_ERROR_UNSUPPORTED_CONFIG;
  with_shape(pick_shape(a.ein_t, a.hid_t, a.co_t), [&](auto shape) { rc = launch_fwd_wave<decltype(shape)>(a, s); });
  return rc;
}

static int run_backward(PcArgs& a, const float* grad_out, float* d_in, float* d_q, float* d_params, void* workspace,
                        size_t workspace_bytes, hipStream_t s) {
  const int64_t edges = a.edge_q ? a.n_edges : (a.n_query << a.log2k);
  if (!grad_out || !d_in || (a.cq > 0 && !d_q) || !d_params || !workspace ||
      workspace_bytes < wcn_pointconv_backward_workspace(edges, 1, a.ein_t, a.hid_t, a.co_t, a.lin_sc))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t gf = grad_floats(a.ein_t, a.hid_t, a.co_t, a.lin_sc);
  if (a.n_query == 0 || edges == 0)
    return hipMemsetAsync(d_params, 0, gf * sizeof(float), s) == hipSuccess ? WCN_SUCCESS : WCN_ERROR_KERNEL_EXECUTION;
  a.grad_out = grad_out; a.d_in = d_in; a.d_q = d_q; a.partial = (float*)workspace;
  const int grid = bwd_grid(edges, 1);
  int rc = WCN_ERROR_UNSUPPORTED_CONFIG;
  with_shape(pick_shape(a.ein_t, a.hid_t, a.co_t), [&](auto shape) { rc = launch_bwd<decltype(shape)>(a, grid, s); });
  if (rc != WCN_SUCCESS) return rc;
  hipLaunchKernelGGL(pointconv_grad_reduce_kernel, dim3((unsigned)((gf + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, grid, gf, d_params);
  return launch_status();
}

int wcn_pointconv_edge_forward(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                               const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                               const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                               int32_t linear_shortcut, float* out, void* stream) {
  PcArgs a;
  const int rc = fill_args(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, k, cin, cq, nrel, packed, hidden, cout, eps1,
                           eps2, mean, linear_shortcut);
  if (rc != WCN_SUCCESS) return rc;
  return run_forward(a, out, (hipStream_t)stream);
}

int wcn_pointconv_edge_backward(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                int32_t linear_shortcut, const float* grad_out, float* d_in, float* d_q, float* d_params,
                                void* workspace, size_t workspace_bytes, void* stream) {
  PcArgs a;
  const int rc = fill_args(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, k, cin, cq, nrel, packed, hidden, cout, eps1,
                           eps2, mean, linear_shortcut);
  if (rc != WCN_SUCCESS) return rc;
  return run_backward(a, grad_out, d_in, d_q, d_params, workspace, workspace_bytes, (hipStream_t)stream);
}

// Bitwise-reproducible variant for uniform lists: the input gradient of every EDGE goes to `d_edge` [n_query * k][cin] with
// plain stores (no atomics; `d_in` is not touched), the caller adds the rows of each input point in a fixed order (sorted
// edge ids).  Everything else - d_q, the parameter gradients - is deterministic in both variants.
int wcn_pointconv_edge_backward_peredge(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                        const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                        const float* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                        int32_t linear_shortcut, const float* grad_out, float* d_edge, float* d_q,
                                        float* d_params, void* workspace, size_t workspace_bytes, void* stream) {
  PcArgs a;
  const int rc = fill_args(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, k, cin, cq, nrel, packed, hidden, cout, eps1,
                           eps2, mean, linear_shortcut);
  if (rc != WCN_SUCCESS) return rc;
  if (!d_edge) return WCN_ERROR_INVALID_PARAMETERS;
  a.d_edge = d_edge;
  return run_backward(a, grad_out, d_edge, d_q, d_params, workspace, workspace_bytes, (hipStream_t)stream);
}

// Ragged neighbour lists (radius search): `nbr` [n_edges] with the lists of the queries behind each other, `edge_q`
// [n_edges] the query of every edge (non-decreasing), `q_scale` [n_query] the reduction scale per query (1 / list length for
// mean; NULL = sum).  `out` (forward) and `d_q` (backward) must be ZERO-FILLED: a list may straddle two 32-edge tiles, so
// list segments are added to their rows.
int wcn_pointconv_edge_forward_ragged(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                      const int32_t* nbr, const int32_t* edge_q, const float* q_scale, int64_t n_edges,
                                      int64_t n_query, int32_t cin, int32_t cq, int32_t nrel, const float* packed,
                                      int32_t hidden, int32_t cout, float eps1, float eps2, int32_t linear_shortcut,
                                      float* out, void* stream) {
  PcArgs a;
  const int rc = fill_args(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, 1, cin, cq, nrel, packed, hidden, cout, eps1,
                           eps2, 0, linear_shortcut);
  if (rc != WCN_SUCCESS) return rc;
  if (const int rr = set_ragged(a, edge_q, q_scale, n_edges)) return rr;
  return run_forward(a, out, (hipStream_t)stream);
}

int wcn_pointconv_edge_backward_ragged(const float* in_feats, const float* q_feats, const float* in_xyz, const float* q_xyz,
                                       const int32_t* nbr, const int32_t* edge_q, const float* q_scale, int64_t n_edges,
                                       int64_t n_query, int32_t cin, int32_t cq, int32_t nrel, const float* packed,
                                       int32_t hidden, int32_t cout, float eps1, float eps2, int32_t linear_shortcut,
                                       const float* grad_out, float* d_in, float* d_q, float* d_params, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  PcArgs a;
  const int rc = fill_args(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, 1, cin, cq, nrel, packed, hidden, cout, eps1,
                           eps2, 0, linear_shortcut);
  if (rc != WCN_SUCCESS) return rc;
  if (const int rr = set_ragged(a, edge_q, q_scale, n_edges)) return rr;
  return run_backward(a, grad_out, d_in, d_q, d_params, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
