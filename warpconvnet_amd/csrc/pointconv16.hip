// pointconv16.hip - the PointConv edge pipeline under autocast: bf16 / f16 GEMM operands on v_mfma_f32_32x32x16_{bf16,f16},
// fp32 accumulators, fp32 LayerNorm / ReLU / shortcut add / reduction (gfx950).  DESIGN.md section 4.39.
//
// Same chain as pointconv.hip (reference: warpconvnet/nn/modules/point_conv.py:231-273 with the MLPBlock of
// warpconvnet/nn/modules/mlp.py:124-177), other arithmetic contract and other data movement:
//
//   x_e = T([in_feats[nbr[e]] | q_feats[q(e)] | in_xyz[nbr[e]] - q_xyz[q(e)]])     rows stored in T, rel-pos formed in fp32
//   h   = ReLU(LN1(W1_T x_e + b1)),  o = LN2(W2_T T(h) + b2) + (x_e | Ws_T x_e + bs),  out[q] = scale * sum_e o
//
// W1_T, W2_T, Ws_T are the fp32 parameters rounded to T once (pack kernel); T(h) is the only intermediate rounding.
// Uniform lists of 1 << log2k edges; an entry of -1 is an edge that contributes nothing (forward and backward).
//
// Operand layout.  All GEMMs are TRANSPOSED (A = weights, rows = output channels; B = data, columns = the 32 edges of a
// tile), K = 16 per instruction: lane (h, i) of A holds row i, k-slots 8h .. 8h+7 (one 16-B fragment), lane (h, e) of B holds
// edge e, the same k-slots.  A result tile puts edge e in lanes e / e+32 and channel sigma(r, h) = 8*(r/4) + 4h + r%4 in
// register r, so registers 8b .. 8b+7 of the two halves, converted to T, ARE the B fragment of K-block b of the next GEMM:
// k-slot 8h + j is channel tau(b, h, j) = sigma(8b + j, h), and that permutation is folded into the packed A images.  The
// gathered row is the natural layout: K-block kb, lane half h = channels 16kb + 8h .. + 7, one 16-B load where the widths allow.
//
// pointconv16_fwd_kernel - one tile per wave, 4-wave persistent workgroups, the images P1 | P2 | PS in 43 520 B of LDS, two
//   workgroups per CU (two waves per SIMD, 256 registers each), no barrier in the loop.  The loop is written for
//   kFwdTiles tiles per wave (every A fragment read from LDS then feeds that many MFMAs); two spill at 256 registers.
// pointconv16_bwd_kernel - one tile per 4-wave workgroup, wave w owns hidden channels [32w, 32w+32) through the chain (the
//   split of pointconv.hip).  At 2 bytes ALL operand images (P1, P2, the transposed P2T, P1T and the shortcut's PST) fit the
//   LDS next to the per-tile data, 153 600 B, one workgroup per CU: a wave reads the 16 fragments of its hidden block per
//   tile (16 KiB of LDS reads per wave and tile) and no weight occupies a register between tiles - with them resident
//   (64 VGPRs) the kernel spilled.  The channel-major tiles for the weight-gradient GEMMs are 2-byte with a pitch of 40
//   elements (80 B).  Every wave gathers the whole tile's x (GEMM1 needs all of it): four requests per row, three served by L2.
#include "gather_gemm.h"

namespace wcn {
namespace {

constexpr int kEin = 64, kHid = 128, kCo = 64;             // the one instantiated (padded) shape
constexpr int kKB = kEin / 16;                              // K-blocks of a gathered row
constexpr int kNB1 = kHid / 32, kNB2 = kCo / 32, kNBX = kEin / 32;
constexpr int kWaves = 4;
constexpr int kFwdTiles = 1;                                // tiles per wave and trip of the forward (2 spills at 256 VGPRs)
constexpr int kFwdMaxGrid = 512, kBwdMaxGrid = 256;         // persistent workgroups: two per CU forward, one per CU backward
constexpr int kPitch16 = 40;  // elements per row of the [channel][32 edges] tiles: 80 B = 5 x 16 B, odd, so the 16-B reads of
                              // 8 (16) lanes = 8 (16) consecutive rows fall into 8 (16) different 16-B bank groups

// packed image: 16-B fragments [unit][64 lanes], then the fp32 tables
constexpr int F_P1 = 0;                          // [blk][kb][64]       GEMM1 A:  W1[hid 32blk+i][c 16kb+8h+j]
constexpr int F_P2 = F_P1 + kNB1 * kKB * 64;     // [blk][b2][kb][64]   GEMM2 A:  W2[out 32b2+i][hid 32blk+tau]
constexpr int F_P2T = F_P2 + kNB1 * kNB2 * 128;  // [blk][b2][kb][64]   dH A:     W2[out 32b2+tau][hid 32blk+i]
constexpr int F_P1T = F_P2T + kNB1 * kNB2 * 128; // [blk][cb][kb][64]   dX A:     W1[hid 32blk+tau][c 32cb+i]
constexpr int F_PS = F_P1T + kNB1 * kNBX * 128;  // [b2][kb][64]        shortcut: Ws[out 32b2+i][c 16kb+8h+j]
constexpr int F_PST = F_PS + kNB2 * kKB * 64;    // [cb][b2][kb][64]    dX A:     Ws[out 32b2+tau][c 32cb+i]
constexpr int F_END = F_PST + kNBX * kNB2 * 128;
constexpr int T_1 = 0;                           // [blk][3][2][16]  b1, g1, be1 at channel 32blk + sigma(r, h)
constexpr int T_2 = T_1 + kNB1 * 96;             // [b2][3][2][16]   b2, g2, be2
constexpr int T_S = T_2 + kNB2 * 96;             // [b2][2][16]      bs
constexpr int T_END = T_S + kNB2 * 32;
constexpr int kPackedBytes = F_END * 16 + T_END * 4;
static_assert(kPackedBytes == 84480, "packed image");

constexpr int kFwdLds = (F_P2T + kNB2 * kKB * 64) * 16 + T_END * 4;  // P1 | P2 | PS | tables
static_assert(kFwdLds == 43520, "forward LDS layout");
// backward LDS (bytes)
constexpr int B_TAB = 0;                                   // T1 | T2
constexpr int B_TX = B_TAB + T_S * 4;                      // T [64][40]   x, channel-major (dW1 / dWs A)
constexpr int B_TH = B_TX + kEin * kPitch16 * 2;           // T [128][40]  H, later dHpre (wave w: rows 32w ..)
constexpr int B_TB = B_TH + kHid * kPitch16 * 2;           // T [64][40]   dOpre
constexpr int B_TD = B_TB + kCo * kPitch16 * 2;            // T [64][40]   dy (Linear shortcut)
constexpr int B_PO = B_TD + kCo * kPitch16 * 2;            // f32 [4][2][16][64] partial tiles exchanged between the waves
constexpr int B_ST = B_PO + kWaves * 2 * 1024 * 4;         // f32 [4][32][3] LayerNorm 1 statistics | [4][32][2] backward sums
constexpr int B_DXT = B_ST + kWaves * 32 * 5 * 4;          // f32 [32][65] dX edge-major
constexpr int B_DOUT = B_DXT + 32 * (kEin + 1) * 4;        // f32 [32][64] scaled grad_out rows of the tile's queries
constexpr int B_JT = B_DOUT + 32 * kCo * 4;                // int [32] neighbour ids
constexpr int B_WT = B_JT + 32 * 4;                        // frag [F_PS] the images P1 | P2 | P2T | P1T
constexpr int B_WS = B_WT + F_PS * 16;                     // frag [F_END - F_PST] the image PST (Linear shortcut)
constexpr int kBwdLds = B_WS + (F_END - F_PST) * 16;
static_assert(kBwdLds == 153600, "backward LDS layout");
static_assert(kBwdLds <= 160 * 1024, "one workgroup per CU (the register file decides: DESIGN 4.39)");

__host__ __device__ constexpr int sigma(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

__device__ __forceinline__ float half_swap(float v) { return __shfl_xor(v, 32, 64); }
__device__ __forceinline__ float half_sum32(float v) {
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

struct Pc16Args {
  const void* in_feats;   // T [n_in][cin]
  const void* q_feats;    // T [n_query][cq]
  const float* in_xyz;    // [n_in][3]   (nrel == 3)
  const float* q_xyz;     // [n_query][3]
  const int32_t* nbr;     // [n_query << log2k], -1 = no edge
  int64_t n_query;
  int32_t log2k, cin, cq, nrel, vec;  // vec: widths multiples of 8 and 16-B aligned rows
  const void* packed;
  int32_t ein_t, hid_t, co_t;
  float eps1, eps2, scale;
  float* out;             // forward:  [n_query][co_t]
  const float* grad_out;  // backward: [n_query][co_t]
  float* d_in;            //           fp32 [n_in][cin], zero-filled by the caller
  float* d_q;             //           fp32 [n_query][cq], every row stored once
  float* partial;         //           [grid][grad floats]
};

__host__ __device__ inline int64_t grad_floats16(int ein_t, int hid_t, int co_t, int lin) {
  return (int64_t)hid_t * ein_t + 3 * hid_t + (int64_t)co_t * hid_t + 3 * co_t + (lin ? (int64_t)co_t * ein_t + co_t : 0);
}

// registers 8b .. 8b+7 of a result tile -> the B fragment of K-block b (the one intermediate rounding where v is H)
template <typename T>
__device__ __forceinline__ typename Mfma32<T>::type to_frag(const float (&v)[16], int b) {
  typename Mfma32<T>::type f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (T)v[8 * b + j];
  return f;
}

// x_e of one edge as kKB fragments: one 16-B load where eight channels lie inside one feature row, else element by element
// (row tails, relative positions: fp32 difference, then rounded)
template <typename T>
__device__ __forceinline__ void gather16(const Pc16Args& a, bool valid, int64_t q, int32_t j, int h,
                                         typename Mfma32<T>::type (&x)[kKB]) {
  typedef typename Mfma32<T>::type frag;
  const T* fi = reinterpret_cast<const T*>(a.in_feats) + (int64_t)j * a.cin;
  const T* fq = reinterpret_cast<const T*>(a.q_feats) + q * a.cq;
#pragma unroll
  for (int kb = 0; kb < kKB; ++kb) {
    const int c0 = 16 * kb + 8 * h;
    frag v;
#pragma unroll
    for (int d = 0; d < 8; ++d) v[d] = (T)0.f;
    if (valid) {
      if (a.vec && c0 + 8 <= a.cin) {
        v = *reinterpret_cast<const frag*>(fi + c0);
      } else if (a.vec && c0 >= a.cin && c0 + 8 <= a.cin + a.cq) {
        v = *reinterpret_cast<const frag*>(fq + (c0 - a.cin));
      } else {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          const int c = c0 + d;
          if (c < a.cin) v[d] = fi[c];
          else if (c < a.cin + a.cq) v[d] = fq[c - a.cin];
          else if (c < a.cin + a.cq + a.nrel)
            v[d] = (T)(a.in_xyz[(int64_t)j * 3 + (c - a.cin - a.cq)] - a.q_xyz[q * 3 + (c - a.cin - a.cq)]);
        }
      }
    }
    x[kb] = v;
  }
}

// mean, then the squared deviations of the TRUE channels (padded ones hold 0, not the mean) of NB result tiles held by one
// wave: returns (mu, rstd).  lim = width - 4h: channel 32b + sigma(r, h) is a true one iff 32b + sigma(r, 0) < lim.
template <int NB>
__device__ __forceinline__ void wave_layer_norm(const float (&v)[NB][16], int width, int padded, int h, float eps, float& mu,
                                                float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += v[b][r];
  s += half_swap(s);
  mu = s / (float)width;
  const int lim = width - 4 * h;
  float q = 0.f;
  if (width == padded) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) q = fmaf(v[b][r] - mu, v[b][r] - mu, q);
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = (32 * b + sigma(r, 0) < lim) ? v[b][r] - mu : 0.f;
        q = fmaf(d, d, q);
      }
  }
  q += half_swap(q);
  rstd = rsqrtf(q / (float)width + eps);
}

template <typename T, bool LIN>
__global__ __launch_bounds__(256, 2) void pointconv16_fwd_kernel(const Pc16Args a) {
  typedef typename Mfma32<T>::type frag;
  constexpr int TPW = kFwdTiles;
  extern __shared__ __attribute__((aligned(16))) char smem16[];
  frag* sP1 = reinterpret_cast<frag*>(smem16);
  frag* sP2 = sP1 + (F_P2 - F_P1);
  frag* sPS = sP2 + (F_P2T - F_P2);
  float* sTab = reinterpret_cast<float*>(sPS + (F_PST - F_PS));
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, e = lane & 31;
  const frag* pk = reinterpret_cast<const frag*>(a.packed);
  for (int i = tid; i < F_P2T; i += 256) sP1[i] = pk[i];  // P1 | P2
  if (LIN)
    for (int i = tid; i < F_PST - F_PS; i += 256) sPS[i] = pk[F_PS + i];
  for (int i = tid; i < T_END; i += 256) sTab[i] = reinterpret_cast<const float*>(pk + F_END)[i];
  __syncthreads();  // the only barrier: the waves are independent from here on

  const int k = 1 << a.log2k;
  const int64_t n_edges = a.n_query << a.log2k;
  const int64_t ntiles = (n_edges + 31) >> 5;
  const int64_t stride = (int64_t)gridDim.x * kWaves * TPW;
  for (int64_t t0 = ((int64_t)blockIdx.x * kWaves + (tid >> 6)) * TPW; t0 < ntiles; t0 += stride) {
    // the images never change: without this the compiler hoists their LDS reads out of the loop and spills them
    uint32_t z = 0u;
    asm volatile("" : "+v"(z));
    const frag* p1 = reinterpret_cast<const frag*>(reinterpret_cast<const char*>(sP1) + z) + lane;
    const frag* p2 = reinterpret_cast<const frag*>(reinterpret_cast<const char*>(sP2) + z) + lane;
    const frag* ps = reinterpret_cast<const frag*>(reinterpret_cast<const char*>(sPS) + z) + lane;
    const float* tab = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sTab) + z);

    frag x[TPW][kKB];
    bool valid[TPW];
    int64_t qid[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      const int64_t E = (t0 + u) * 32 + e;
      const int32_t j = E < n_edges ? a.nbr[E] : -1;
      valid[u] = j >= 0;
      qid[u] = E < n_edges ? (E >> a.log2k) : -1;
      gather16<T>(a, valid[u], valid[u] ? qid[u] : 0, j, h, x[u]);
    }
    // ---- GEMM1: every A fragment feeds both tiles ----
    float hb[TPW][kNB1][16];
#pragma unroll
    for (int blk = 0; blk < kNB1; ++blk) {
      f32x16 acc[TPW];
#pragma unroll
      for (int u = 0; u < TPW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        const frag av = p1[(blk * kKB + kb) * 64];
#pragma unroll
        for (int u = 0; u < TPW; ++u) acc[u] = Mfma32<T>::mfma(av, x[u][kb], acc[u]);
      }
      const float* t1 = tab + T_1 + blk * 96 + h * 16;
#pragma unroll
      for (int u = 0; u < TPW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) hb[u][blk][r] = acc[u][r] + t1[r];
    }
    // ---- LayerNorm1 + ReLU in fp32, then the one rounding: H as B fragments ----
    frag Hb[TPW][kNB1][2];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      float mu, rstd;
      wave_layer_norm<kNB1>(hb[u], a.hid_t, kHid, h, a.eps1, mu, rstd);
#pragma unroll
      for (int blk = 0; blk < kNB1; ++blk) {
        const float* t1 = tab + T_1 + blk * 96 + h * 16;
#pragma unroll
        for (int r = 0; r < 16; ++r) hb[u][blk][r] = fmaxf((hb[u][blk][r] - mu) * rstd * t1[32 + r] + t1[64 + r], 0.f);
        Hb[u][blk][0] = to_frag<T>(hb[u][blk], 0);
        Hb[u][blk][1] = to_frag<T>(hb[u][blk], 1);
      }
    }
    // ---- GEMM2 + LayerNorm2 + shortcut ----
    float o[TPW][kNB2][16];
#pragma unroll
    for (int b2 = 0; b2 < kNB2; ++b2) {
      f32x16 acc[TPW];
#pragma unroll
      for (int u = 0; u < TPW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
#pragma unroll
      for (int blk = 0; blk < kNB1; ++blk)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const frag av = p2[((blk * kNB2 + b2) * 2 + kb) * 64];
#pragma unroll
          for (int u = 0; u < TPW; ++u) acc[u] = Mfma32<T>::mfma(av, Hb[u][blk][kb], acc[u]);
        }
      const float* t2 = tab + T_2 + b2 * 96 + h * 16;
#pragma unroll
      for (int u = 0; u < TPW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[u][b2][r] = acc[u][r] + t2[r];
    }
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
      float mu, rstd;
      wave_layer_norm<kNB2>(o[u], a.co_t, kCo, h, a.eps2, mu, rstd);
#pragma unroll
      for (int b2 = 0; b2 < kNB2; ++b2) {
        const float* t2 = tab + T_2 + b2 * 96 + h * 16;
        float sc[16];
        if (LIN) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
          for (int kb = 0; kb < kKB; ++kb) acc = Mfma32<T>::mfma(ps[(b2 * kKB + kb) * 64], x[u][kb], acc);
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[r] = acc[r] + tab[T_S + b2 * 32 + h * 16 + r];
        } else {
          // identity: output channel 32 b2 + sigma(r, h) = 16 kb + 8 hh + 4h + m with kb = 2 b2 + r/8, hh = (r/4) % 2,
          // m = r % 4 is k-slot 4h + m of K-block kb in lane half hh: the own fragment, or the partner's by one lane swap
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kb = 2 * b2 + (r >> 3), m = r & 3;
            const float lo = (float)x[u][kb][m], hi = (float)x[u][kb][4 + m];
            const float other = half_swap(h ? lo : hi);
            sc[r] = (((r >> 2) & 1) == h) ? (h ? hi : lo) : other;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
          o[u][b2][r] = valid[u] ? (o[u][b2][r] - mu) * rstd * t2[32 + r] + t2[64 + r] + sc[r] : 0.f;
      }
      // ---- reduction over the k edges of a query (adjacent lanes), one store per query and channel ----
      for (int m = k >> 1; m >= 1; m >>= 1) {
#pragma unroll
        for (int b2 = 0; b2 < kNB2; ++b2)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[u][b2][r] += __shfl_xor(o[u][b2][r], m, 64);
      }
      if (qid[u] >= 0 && (e & (k - 1)) == 0) {
        float* dst = a.out + qid[u] * a.co_t;
#pragma unroll
        for (int b2 = 0; b2 < kNB2; ++b2)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = 32 * b2 + sigma(r, h);
            if (ch < a.co_t) dst[ch] = o[u][b2][r] * a.scale;
          }
      }
    }
  }
}

template <typename T, bool LIN>
__global__ __launch_bounds__(256, 1) void pointconv16_bwd_kernel(const Pc16Args a) {
  typedef typename Mfma32<T>::type frag;
  extern __shared__ __attribute__((aligned(16))) char smem16[];
  T* tX = reinterpret_cast<T*>(smem16 + B_TX);
  T* tH = reinterpret_cast<T*>(smem16 + B_TH);
  T* tB = reinterpret_cast<T*>(smem16 + B_TB);
  T* tD = reinterpret_cast<T*>(smem16 + B_TD);
  float* po = reinterpret_cast<float*>(smem16 + B_PO);
  float* st = reinterpret_cast<float*>(smem16 + B_ST);
  float* dxt = reinterpret_cast<float*>(smem16 + B_DXT);
  float* dout = reinterpret_cast<float*>(smem16 + B_DOUT);
  int32_t* jt = reinterpret_cast<int32_t*>(smem16 + B_JT);
  constexpr int ST_LN1 = kWaves * 32 * 3;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, e = lane & 31;
  const int k = 1 << a.log2k, nq = 32 >> a.log2k;
  const int64_t n_edges = a.n_query << a.log2k;
  const int64_t ntiles = (n_edges + 31) >> 5;
  const float inv_hid = 1.f / (float)a.hid_t, inv_co = 1.f / (float)a.co_t;
  const frag* pk = reinterpret_cast<const frag*>(a.packed);
  T* thw = tH + w * 32 * kPitch16;  // this wave's rows of tH
  auto true_channels = [&](int ww) { return min(max(a.hid_t - 32 * ww, 0), 32); };
  for (int i = tid; i < T_S; i += 256) reinterpret_cast<float*>(smem16 + B_TAB)[i] = reinterpret_cast<const float*>(pk + F_END)[i];
  // the operand images live in LDS once per persistent workgroup; a wave reads the 16 fragments of its hidden block per tile
  for (int i = tid; i < F_PS; i += 256) reinterpret_cast<frag*>(smem16 + B_WT)[i] = pk[i];
  if (LIN)
    for (int i = tid; i < F_END - F_PST; i += 256) reinterpret_cast<frag*>(smem16 + B_WS)[i] = pk[F_PST + i];
  __syncthreads();

  // persistent parameter-gradient accumulators
  f32x16 dW1a[kNBX], dW2a[kNB2], dWsa;  // dWs: block (cb, b2) = (w / 2, w % 2)
  float dg1a[16], dbe1a[16], db1a[16];
  float dg2a[8], dbe2a[8], db2a[8];     // this wave's quarter: items (b2*16 + r) with r % 4 == w
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dW1a[0][r] = dW1a[1][r] = dW2a[0][r] = dW2a[1][r] = dWsa[r] = 0.f;
    dg1a[r] = dbe1a[r] = db1a[r] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) dg2a[i] = dbe2a[i] = db2a[i] = 0.f;

  // ---- software pipeline: rows of tile i+1 requested once GEMM1 of tile i has consumed x, ids of tile i+2 with them ----
  auto load_ids = [&](int64_t tile, bool& valid, int64_t& q, int32_t& j) {
    const int64_t E = tile * 32 + e;
    j = (tile < ntiles && E < n_edges) ? a.nbr[E] : -1;
    valid = j >= 0;
    q = valid ? (E >> a.log2k) : 0;
  };
  frag x[kKB];
  bool v_cur, v_nxt;
  int64_t q_cur, q_nxt;
  int32_t j_cur, j_nxt;
  load_ids(blockIdx.x, v_cur, q_cur, j_cur);
  gather16<T>(a, v_cur, q_cur, j_cur, h, x);
  load_ids((int64_t)blockIdx.x + gridDim.x, v_nxt, q_nxt, j_nxt);

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---- A. stage the tile: neighbour ids, grad_out rows, this wave's K-block of x channel-major ----
    uint32_t z = 0u;  // the tables never change: keep their reads inside the tile (hoisted, they are 144 registers)
    asm volatile("" : "+v"(z));
    const float* tab = reinterpret_cast<const float*>(smem16 + B_TAB + z);
    const frag* wimg = reinterpret_cast<const frag*>(smem16 + B_WT + z) + lane;  // (the images likewise: 64 registers)
    auto wA1 = [&](int kb) { return wimg[F_P1 + (w * kKB + kb) * 64]; };
    auto wA2 = [&](int b, int kb) { return wimg[F_P2 + ((w * kNB2 + b) * 2 + kb) * 64]; };
    auto wA2T = [&](int b, int kb) { return wimg[F_P2T + ((w * kNB2 + b) * 2 + kb) * 64]; };
    auto wA1T = [&](int cb, int kb) { return wimg[F_P1T + ((w * kNBX + cb) * 2 + kb) * 64]; };
    const bool valid = v_cur;
    if (w == 0 && h == 0) jt[e] = valid ? j_cur : -1;
    for (int i = tid; i < nq * kCo; i += 256) {
      const int ql = i / kCo, ch = i - ql * kCo;
      const int64_t qq = tile * nq + ql;
      dout[i] = (qq < a.n_query && ch < a.co_t) ? a.grad_out[qq * a.co_t + ch] * a.scale : 0.f;
    }
#pragma unroll
    for (int kb = 0; kb < kKB; ++kb)
      if (kb == w) {
#pragma unroll
        for (int j = 0; j < 8; ++j) tX[(16 * kb + 8 * h + j) * kPitch16 + e] = x[kb][j];
      }

    // ---- GEMM1 (this wave's hidden block) ----
    float acc1[16];
    {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) acc = Mfma32<T>::mfma(wA1(kb), x[kb], acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[r] = acc[r] + tab[T_1 + w * 96 + h * 16 + r];
    }
    // x is consumed (its channel-major copy is in tX): next tile's rows, and the ids of the tile after it
    v_cur = v_nxt; q_cur = q_nxt; j_cur = j_nxt;
    gather16<T>(a, v_cur, q_cur, j_cur, h, x);
    load_ids(tile + 2 * (int64_t)gridDim.x, v_nxt, q_nxt, j_nxt);

    // LayerNorm 1 over the four waves with one exchange: wave w sends the mean m_w of its n_w true channels,
    // q_w = sum (v - m_w)^2 and r_w = sum (v - m_w); merged as in pointconv.hip (Chan, with the r_w term)
    {
      const int nw1 = true_channels(w);
      float s1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s1 += acc1[r];
      s1 += half_swap(s1);
      const float mw = nw1 > 0 ? s1 / (float)nw1 : 0.f;
      const int lim = a.hid_t - 32 * w - 4 * h;
      float qw = 0.f, rw = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = (sigma(r, 0) < lim) ? acc1[r] - mw : 0.f;
        rw += d;
        qw = fmaf(d, d, qw);
      }
      qw += half_swap(qw);
      rw += half_swap(rw);
      if (h == 0) {
        st[(w * 32 + e) * 3 + 0] = mw;
        st[(w * 32 + e) * 3 + 1] = qw;
        st[(w * 32 + e) * 3 + 2] = rw;
      }
    }
    __syncthreads();  // 1: tX, st[0], jt, dout

    float rstd1;
    float xh1[16];
    uint32_t relu = 0u;  // bit r: H[r] > 0
    {
      float S1 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) S1 += (float)true_channels(ww) * st[(ww * 32 + e) * 3 + 0] + st[(ww * 32 + e) * 3 + 2];
      const float mu1 = S1 * inv_hid;
      float M2 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) {
        const float dm = st[(ww * 32 + e) * 3 + 0] - mu1;
        M2 += st[(ww * 32 + e) * 3 + 1] + dm * (2.f * st[(ww * 32 + e) * 3 + 2] + (float)true_channels(ww) * dm);
      }
      rstd1 = rsqrtf(fmaxf(M2, 0.f) * inv_hid + a.eps1);
      float H[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        xh1[r] = (acc1[r] - mu1) * rstd1;
        H[r] = fmaxf(xh1[r] * tab[T_1 + w * 96 + 32 + h * 16 + r] + tab[T_1 + w * 96 + 64 + h * 16 + r], 0.f);
        relu |= (H[r] > 0.f ? 1u : 0u) << r;
        thw[sigma(r, h) * kPitch16 + e] = (T)H[r];
      }
      // ---- GEMM2, partial over this wave's hidden channels; the waves exchange fp32 partial tiles through LDS ----
      const frag Hb0 = to_frag<T>(H, 0), Hb1 = to_frag<T>(H, 1);
#pragma unroll
      for (int b = 0; b < kNB2; ++b) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        o = Mfma32<T>::mfma(wA2(b, 0), Hb0, o);
        o = Mfma32<T>::mfma(wA2(b, 1), Hb1, o);
        f32x4* pw = reinterpret_cast<f32x4*>(po) + ((w * 2 + b) * 4) * 64 + lane;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4 v = {o[4 * r4], o[4 * r4 + 1], o[4 * r4 + 2], o[4 * r4 + 3]};
          pw[r4 * 64] = v;
        }
      }
    }
    __syncthreads();  // 2: po

    float xh2[kNB2][16];
    float rstd2;
    {
#pragma unroll
      for (int b = 0; b < kNB2; ++b)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ww = 0; ww < kWaves; ++ww) v += reinterpret_cast<const f32x4*>(po)[((ww * 2 + b) * 4 + r4) * 64 + lane];
#pragma unroll
          for (int d = 0; d < 4; ++d) xh2[b][4 * r4 + d] = v[d] + tab[T_2 + b * 96 + h * 16 + 4 * r4 + d];
        }
      float mu2;
      wave_layer_norm<kNB2>(xh2, a.co_t, kCo, h, a.eps2, mu2, rstd2);
#pragma unroll
      for (int b = 0; b < kNB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) xh2[b][r] = (xh2[b][r] - mu2) * rstd2;
    }

    // ---- the forward is recomputed; backward: dy -> LayerNorm2 -> dOpre ----
    const int ql = e >> a.log2k;
    frag dOb[kNB2][2];  // dOpre as B fragments
    {
      float dOpre[kNB2][16], dy[kNB2][16];
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int b = 0; b < kNB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dy[b][r] = valid ? dout[ql * kCo + 32 * b + sigma(r, h)] : 0.f;
          const float gd = dy[b][r] * tab[T_2 + b * 96 + 32 + h * 16 + r];
          m1 += gd;
          m2 += gd * xh2[b][r];
        }
      m1 += half_swap(m1);
      m2 += half_swap(m2);
      m1 *= inv_co;
      m2 *= inv_co;
#pragma unroll
      for (int b = 0; b < kNB2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          dOpre[b][r] = rstd2 * (dy[b][r] * tab[T_2 + b * 96 + 32 + h * 16 + r] - m1 - xh2[b][r] * m2);
          if ((r & 3) == w) {
            const int i = (b * 16 + r) >> 2;
            dg2a[i] += dy[b][r] * xh2[b][r];
            dbe2a[i] += dy[b][r];
            db2a[i] += dOpre[b][r];
            tB[(32 * b + sigma(r, h)) * kPitch16 + e] = (T)dOpre[b][r];
            if (LIN) tD[(32 * b + sigma(r, h)) * kPitch16 + e] = (T)dy[b][r];
          }
        }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        dOb[0][kb] = to_frag<T>(dOpre[0], kb);
        dOb[1][kb] = to_frag<T>(dOpre[1], kb);
      }
    }
    // ---- dH (this wave's hidden block) = W2 dOpre, ReLU mask, LayerNorm1 backward sums ----
    float gg[16];
    {
      f32x16 dh;
#pragma unroll
      for (int r = 0; r < 16; ++r) dh[r] = 0.f;
#pragma unroll
      for (int b = 0; b < kNB2; ++b) {
        dh = Mfma32<T>::mfma(wA2T(b, 0), dOb[b][0], dh);
        dh = Mfma32<T>::mfma(wA2T(b, 1), dOb[b][1], dh);
      }
      float p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float g = ((relu >> r) & 1u) ? dh[r] : 0.f;
        dg1a[r] += g * xh1[r];
        dbe1a[r] += g;
        gg[r] = g * tab[T_1 + w * 96 + 32 + h * 16 + r];
        p1 += gg[r];
        p2 += gg[r] * xh1[r];
      }
      p1 += half_swap(p1);
      p2 += half_swap(p2);
      if (h == 0) {
        st[ST_LN1 + (w * 32 + e) * 2 + 0] = p1;
        st[ST_LN1 + (w * 32 + e) * 2 + 1] = p2;
      }
    }
    __syncthreads();  // 3: st[1], tB, tD

    float dHpre[16];
    {
      float m1 = 0.f, m2 = 0.f;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) {
        m1 += st[ST_LN1 + (ww * 32 + e) * 2 + 0];
        m2 += st[ST_LN1 + (ww * 32 + e) * 2 + 1];
      }
      m1 *= inv_hid;
      m2 *= inv_hid;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dHpre[r] = rstd1 * (gg[r] - m1 - xh1[r] * m2);
        db1a[r] += dHpre[r];
      }
    }
    // ---- weight gradients: the reduction runs over the 32 edges = two K-blocks; A and B fragments are 16-B reads of
    // eight consecutive edges of one channel row (row = lane % 32, edges 16 kb + 8h ..) ----
    auto tile_frag = [&](const T* t, int row0, int kb) {
      return *reinterpret_cast<const frag*>(t + (row0 + e) * kPitch16 + 16 * kb + 8 * h);
    };
    // dW2 (rows of this wave) += H^T dOpre
#pragma unroll
    for (int b = 0; b < kNB2; ++b)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) dW2a[b] = Mfma32<T>::mfma(tile_frag(thw, 0, kb), tile_frag(tB, 32 * b, kb), dW2a[b]);
    // the wave's tile now takes dHpre (LDS operations of one wave execute in order)
#pragma unroll
    for (int r = 0; r < 16; ++r) thw[sigma(r, h) * kPitch16 + e] = (T)dHpre[r];
    // ---- dX partial = W1 dHpre over this wave's hidden channels (+ Ws dy: block (cb, b) by wave (2 cb + b)) ----
    {
      const frag dHb0 = to_frag<T>(dHpre, 0), dHb1 = to_frag<T>(dHpre, 1);
#pragma unroll
      for (int cb = 0; cb < kNBX; ++cb) {
        f32x16 dx;
#pragma unroll
        for (int r = 0; r < 16; ++r) dx[r] = 0.f;
        dx = Mfma32<T>::mfma(wA1T(cb, 0), dHb0, dx);
        dx = Mfma32<T>::mfma(wA1T(cb, 1), dHb1, dx);
        if (LIN) {
#pragma unroll
          for (int b = 0; b < kNB2; ++b)
            if (cb * kNB2 + b == w) {
#pragma unroll
              for (int kb = 0; kb < 2; ++kb) {  // dy of output block b, K-block kb, read back from the staged grad_out rows
                frag dyb;
#pragma unroll
                for (int j = 0; j < 8; ++j) dyb[j] = (T)(valid ? dout[ql * kCo + 32 * b + sigma(8 * kb + j, h)] : 0.f);
                const frag* ws = reinterpret_cast<const frag*>(smem16 + B_WS + z) + lane;
                dx = Mfma32<T>::mfma(ws[((cb * kNB2 + b) * 2 + kb) * 64], dyb, dx);
              }
            }
        }
        f32x4* pw = reinterpret_cast<f32x4*>(po) + ((w * 2 + cb) * 4) * 64 + lane;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f32x4 v = {dx[4 * r4], dx[4 * r4 + 1], dx[4 * r4 + 2], dx[4 * r4 + 3]};
          pw[r4 * 64] = v;
        }
      }
    }
    // dW1 (columns of this wave) += x^T dHpre;  dWs (this wave's block) += x^T dy
#pragma unroll
    for (int cb = 0; cb < kNBX; ++cb)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) dW1a[cb] = Mfma32<T>::mfma(tile_frag(tX, 32 * cb, kb), tile_frag(thw, 0, kb), dW1a[cb]);
    if (LIN) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        dWsa = Mfma32<T>::mfma(tile_frag(tX, 32 * (w >> 1), kb), tile_frag(tD, 32 * (w & 1), kb), dWsa);
    }
    __syncthreads();  // 4: po (dX partials)

    // ---- dX: sum the partials (+ dy through the identity shortcut), edge-major tile, then scatter ----
#pragma unroll
    for (int cb = 0; cb < kNBX; ++cb)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        if (r4 == w) {
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ww = 0; ww < kWaves; ++ww) v += reinterpret_cast<const f32x4*>(po)[((ww * 2 + cb) * 4 + r4) * 64 + lane];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int r = 4 * r4 + d;
            const int c = 32 * cb + sigma(r, h);  // identity shortcut: + dy, output channel c is x channel c
            dxt[e * (kEin + 1) + c] = (LIN || !valid) ? v[d] : v[d] + dout[ql * kCo + c];
          }
        }
    __syncthreads();  // 5: dxt
    for (int i = tid; i < 32 * a.cin; i += 256) {
      const int ee = i / a.cin, c = i - ee * a.cin;
      const int32_t jj = jt[ee];
      if (jj >= 0) unsafeAtomicAdd(a.d_in + (int64_t)jj * a.cin + c, dxt[ee * (kEin + 1) + c]);  // hardware fp32 add
    }
    for (int i = tid; i < nq * a.cq; i += 256) {
      const int ql = i / a.cq, c = i - ql * a.cq;
      const int64_t qq = tile * nq + ql;
      float s = 0.f;
      for (int kk = 0; kk < k; ++kk) s += dxt[(ql * k + kk) * (kEin + 1) + a.cin + c];
      if (qq < a.n_query) a.d_q[qq * a.cq + c] = s;
    }
    __syncthreads();  // 6: LDS is rewritten by the next tile
  }

  // ---- this workgroup's parameter-gradient partials (every true element is written: the reduce kernel sums them) ----
  float* pW1 = a.partial + (int64_t)blockIdx.x * grad_floats16(a.ein_t, a.hid_t, a.co_t, LIN);
  float* pb1 = pW1 + (int64_t)a.hid_t * a.ein_t;
  float* pg1 = pb1 + a.hid_t;
  float* pbe1 = pg1 + a.hid_t;
  float* pW2 = pbe1 + a.hid_t;
  float* pb2 = pW2 + (int64_t)a.co_t * a.hid_t;
  float* pg2 = pb2 + a.co_t;
  float* pbe2 = pg2 + a.co_t;
  float* pWs = pbe2 + a.co_t;
  float* pbs = pWs + (int64_t)a.co_t * a.ein_t;
  const int hid0 = 32 * w;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int cb = 0; cb < kNBX; ++cb) {  // dW1a[cb][r] at lane (h, e): (c = 32cb + sigma(r, h), hid = hid0 + e)
      const int c = 32 * cb + sigma(r, h), hid = hid0 + e;
      if (c < a.ein_t && hid < a.hid_t) pW1[(int64_t)hid * a.ein_t + c] = dW1a[cb][r];
    }
#pragma unroll
    for (int b = 0; b < kNB2; ++b) {  // dW2a[b][r] at lane (h, e): (hid = hid0 + sigma(r, h), out = 32b + e)
      const int hid = hid0 + sigma(r, h), oc = 32 * b + e;
      if (hid < a.hid_t && oc < a.co_t) pW2[(int64_t)oc * a.hid_t + hid] = dW2a[b][r];
    }
    const float vg = half_sum32(dg1a[r]), vb = half_sum32(dbe1a[r]), vc = half_sum32(db1a[r]);
    const int hid = hid0 + sigma(r, h);
    if (e == 0 && hid < a.hid_t) {
      pg1[hid] = vg;
      pbe1[hid] = vb;
      pb1[hid] = vc;
    }
  }
#pragma unroll
  for (int b = 0; b < kNB2; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((r & 3) == w) {
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
    for (int r = 0; r < 16; ++r) {  // dWsa[r] at lane (h, e): (c = 32 (w/2) + sigma(r, h), out = 32 (w%2) + e)
      const int c = 32 * (w >> 1) + sigma(r, h), oc = 32 * (w & 1) + e;
      if (c < a.ein_t && oc < a.co_t) pWs[(int64_t)oc * a.ein_t + c] = dWsa[r];
    }
  }
}

struct Pack16Args {
  const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *ws, *bs;  // torch layouts, fp32; ws / bs NULL: identity shortcut
  int ein_t, hid_t, co_t;
  void* packed;
};

// one thread per element of the image: 16-bit weights (rounded to T here, once), then the fp32 tables
template <typename T>
__global__ void pointconv16_pack_kernel(const Pack16Args p) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  auto W1 = [&](int c, int hid) { return (c < p.ein_t && hid < p.hid_t) ? p.w1[(int64_t)hid * p.ein_t + c] : 0.f; };
  auto W2 = [&](int hid, int oc) { return (hid < p.hid_t && oc < p.co_t) ? p.w2[(int64_t)oc * p.hid_t + hid] : 0.f; };
  auto WS = [&](int c, int oc) { return (p.ws && c < p.ein_t && oc < p.co_t) ? p.ws[(int64_t)oc * p.ein_t + c] : 0.f; };
  if (idx < F_END * 8) {
    const int j = idx & 7, lane = (idx >> 3) & 63, unit = idx >> 9, h = lane >> 5, i = lane & 31;
    float v;
    if (unit < F_P2 / 64) {  // P1 [blk][kb]
      const int u = unit - F_P1 / 64, blk = u / kKB, kb = u % kKB;
      v = W1(16 * kb + 8 * h + j, 32 * blk + i);
    } else if (unit < F_PS / 64) {  // P2 | P2T | P1T [blk][b][kb]
      const int u = (unit - F_P2 / 64) & 15, blk = u >> 2, b = (u >> 1) & 1, tau = sigma(8 * (u & 1) + j, h);
      v = unit < F_P2T / 64 ? W2(32 * blk + tau, 32 * b + i)
          : unit < F_P1T / 64 ? W2(32 * blk + i, 32 * b + tau) : W1(32 * b + i, 32 * blk + tau);
    } else if (unit < F_PST / 64) {  // PS [b2][kb]
      const int u = unit - F_PS / 64, b2 = u / kKB, kb = u % kKB;
      v = WS(16 * kb + 8 * h + j, 32 * b2 + i);
    } else {  // PST [cb][b2][kb]
      const int u = unit - F_PST / 64, cb = u >> 2, b2 = (u >> 1) & 1, tau = sigma(8 * (u & 1) + j, h);
      v = WS(32 * cb + i, 32 * b2 + tau);
    }
    reinterpret_cast<T*>(p.packed)[idx] = (T)v;
    return;
  }
  const int o = idx - F_END * 8;
  if (o >= T_END) return;
  // [blk][ROWS][2][16] tables: row and channel 32 blk + sigma(r, h)
  const int r = o & 15, hh = (o >> 4) & 1;
  const float* src;
  int ch, width;
  if (o < T_2) {
    const int rows = o >> 5;
    src = rows % 3 == 0 ? p.b1 : rows % 3 == 1 ? p.g1 : p.be1;
    ch = 32 * (rows / 3) + sigma(r, hh);
    width = p.hid_t;
  } else if (o < T_S) {
    const int rows = (o - T_2) >> 5;
    src = rows % 3 == 0 ? p.b2 : rows % 3 == 1 ? p.g2 : p.be2;
    ch = 32 * (rows / 3) + sigma(r, hh);
    width = p.co_t;
  } else {
    src = p.bs;
    ch = 32 * ((o - T_S) >> 5) + sigma(r, hh);
    width = p.co_t;
  }
  reinterpret_cast<float*>(reinterpret_cast<char*>(p.packed) + F_END * 16)[o] = (src && ch < width) ? src[ch] : 0.f;
}

// fixed order over the workgroups: bitwise repeatable (grid == 0 writes zeros)
__global__ void pointconv16_grad_reduce_kernel(const float* __restrict__ partial, int grid, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int g = 0; g < grid; ++g) s += partial[(int64_t)g * n + i];
  out[i] = s;
}

int log2_exact16(int k) {
  for (int l = 0; l <= 5; ++l)
    if ((1 << l) == k) return l;
  return -1;
}
int bwd_grid16(int64_t n_query, int k) {
  const int64_t tiles = (n_query * k + 31) / 32;
  return (int)(tiles < kBwdMaxGrid ? tiles : kBwdMaxGrid);
}

// f(T{}, bool_constant<LIN>{}) for a 16-bit dtype code and the shortcut flag
template <typename F>
int with_type_lin(int dtype, int lin, F&& f) {
  return with_dtype16(dtype, [&](auto t) { return lin ? f(t, std::true_type{}) : f(t, std::false_type{}); });
}

}  // namespace
}  // namespace wcn

using namespace wcn;

extern "C" {

int wcn_pointconv16_supported(int32_t cin, int32_t cq, int32_t nrel, int32_t hidden, int32_t cout, int32_t k,
                              int32_t linear_shortcut, int32_t dtype) {
  if (dtype != WCN_F16 && dtype != WCN_BF16) return 0;
  if (cin < 1 || cq < 0 || (nrel != 0 && nrel != 3) || hidden < 1 || cout < 1) return 0;
  if (!linear_shortcut && cin + cq + nrel != cout) return 0;  // identity shortcut needs equal widths
  return (log2_exact16(k) >= 0 && cin + cq + nrel <= kEin && hidden <= kHid && cout <= kCo) ? 1 : 0;
}

int64_t wcn_pointconv16_packed_bytes(int32_t ein, int32_t hidden, int32_t cout) {
  return (ein >= 1 && ein <= kEin && hidden >= 1 && hidden <= kHid && cout >= 1 && cout <= kCo) ? kPackedBytes : 0;
}

int64_t wcn_pointconv16_grad_floats(int32_t ein, int32_t hidden, int32_t cout, int32_t linear_shortcut) {
  return grad_floats16(ein, hidden, cout, linear_shortcut);
}

size_t wcn_pointconv16_backward_workspace(int64_t n_query, int32_t k, int32_t ein, int32_t hidden, int32_t cout,
                                          int32_t linear_shortcut) {
  return (size_t)bwd_grid16(n_query, k) * (size_t)grad_floats16(ein, hidden, cout, linear_shortcut) * sizeof(float);
}

int wcn_pointconv16_pack(const float* w1, const float* b1, const float* g1, const float* be1, const float* w2,
                         const float* b2, const float* g2, const float* be2, const float* ws, const float* bs, int32_t ein,
                         int32_t hidden, int32_t cout, int32_t dtype, void* packed, void* stream) {
  if (!w1 || !w2 || !packed) return WCN_ERROR_INVALID_PARAMETERS;
  if ((dtype != WCN_F16 && dtype != WCN_BF16) || !wcn_pointconv16_packed_bytes(ein, hidden, cout))
    return WCN_ERROR_UNSUPPORTED_CONFIG;
  const Pack16Args p{w1, b1, g1, be1, w2, b2, g2, be2, ws, bs, ein, hidden, cout, packed};
  return with_dtype16(dtype, [&](auto t) {
    hipLaunchKernelGGL(pointconv16_pack_kernel<decltype(t)>, dim3((F_END * 8 + T_END + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, p);
    return launch_status();
  });
}

static int fill_args16(Pc16Args& a, const void* in_feats, const void* q_feats, const float* in_xyz, const float* q_xyz,
                       const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel, const void* packed,
                       int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean, int32_t lin, int32_t dtype) {
  if (!wcn_pointconv16_supported(cin, cq, nrel, hidden, cout, k, lin, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!in_feats || (cq > 0 && !q_feats) || !nbr || !packed || (nrel && (!in_xyz || !q_xyz)) || n_query < 0 ||
      !aligned_to(packed, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  a = Pc16Args{};
  a.in_feats = in_feats; a.q_feats = q_feats; a.in_xyz = in_xyz; a.q_xyz = q_xyz; a.nbr = nbr;
  a.n_query = n_query; a.log2k = log2_exact16(k); a.cin = cin; a.cq = cq; a.nrel = nrel;
  a.vec = (cin % 8 == 0 && cq % 8 == 0 && aligned_to(in_feats, 16) && aligned_to(q_feats, 16)) ? 1 : 0;
  a.packed = packed; a.ein_t = cin + cq + nrel; a.hid_t = hidden; a.co_t = cout;
  a.eps1 = eps1; a.eps2 = eps2; a.scale = mean ? 1.f / (float)k : 1.f;
  return WCN_SUCCESS;
}

int wcn_pointconv16_edge_forward(const void* in_feats, const void* q_feats, const float* in_xyz, const float* q_xyz,
                                 const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                 const void* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                 int32_t linear_shortcut, int32_t dtype, float* out, void* stream) {
  Pc16Args a;
  const int rc = fill_args16(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, k, cin, cq, nrel, packed, hidden, cout, eps1,
                             eps2, mean, linear_shortcut, dtype);
  if (rc != WCN_SUCCESS) return rc;
  if (!out) return WCN_ERROR_INVALID_PARAMETERS;
  if (n_query == 0) return WCN_SUCCESS;
  a.out = out;
  const int64_t tiles = (n_query * k + 31) / 32, wgs = ceil_div(tiles, kWaves * kFwdTiles);
  const int grid = (int)(wgs < kFwdMaxGrid ? wgs : kFwdMaxGrid);
  return with_type_lin(dtype, linear_shortcut, [&](auto t, auto lin) {
    hipLaunchKernelGGL((pointconv16_fwd_kernel<decltype(t), decltype(lin)::value>), dim3(grid), dim3(256), kFwdLds,
                       (hipStream_t)stream, a);
    return launch_status();
  });
}

int wcn_pointconv16_edge_backward(const void* in_feats, const void* q_feats, const float* in_xyz, const float* q_xyz,
                                  const int32_t* nbr, int64_t n_query, int32_t k, int32_t cin, int32_t cq, int32_t nrel,
                                  const void* packed, int32_t hidden, int32_t cout, float eps1, float eps2, int32_t mean,
                                  int32_t linear_shortcut, int32_t dtype, const float* grad_out, float* d_in, float* d_q,
                                  float* d_params, void* workspace, size_t workspace_bytes, void* stream) {
  Pc16Args a;
  const int rc = fill_args16(a, in_feats, q_feats, in_xyz, q_xyz, nbr, n_query, k, cin, cq, nrel, packed, hidden, cout, eps1,
                             eps2, mean, linear_shortcut, dtype);
  if (rc != WCN_SUCCESS) return rc;
  if (!grad_out || !d_in || (cq > 0 && !d_q) || !d_params || !workspace ||
      workspace_bytes < wcn_pointconv16_backward_workspace(n_query, k, a.ein_t, hidden, cout, linear_shortcut))
    return WCN_ERROR_INVALID_PARAMETERS;
  hipStream_t s = (hipStream_t)stream;
  a.grad_out = grad_out; a.d_in = d_in; a.d_q = d_q; a.partial = (float*)workspace;
  const int grid = bwd_grid16(n_query, k);
  if (grid > 0) {
    const int lrc = with_type_lin(dtype, linear_shortcut, [&](auto t, auto lin) {
      void (*const kernel)(Pc16Args) = pointconv16_bwd_kernel<decltype(t), decltype(lin)::value>;
      static unsigned long long attr_done = 0ull;  // once per instance and device: more than 64 KiB of dynamic LDS
      const int arc = once_per_device(attr_done, [&] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kBwdLds) == hipSuccess;
      });
      if (arc != WCN_SUCCESS) return arc;
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), kBwdLds, s, a);
      return launch_status();
    });
    if (lrc != WCN_SUCCESS) return lrc;
  }
  const int64_t gf = grad_floats16(a.ein_t, hidden, cout, linear_shortcut);
  hipLaunchKernelGGL(pointconv16_grad_reduce_kernel, dim3((unsigned)((gf + 255) / 256)), dim3(256), 0, s,
                     (const float*)workspace, grid, gf, d_params);
  return launch_status();
}

}  // extern "C"
