// dense_conv2d.hip - dense 2-D convolution on channels-last images (FIGConvNet's folded grids: nn.Conv2d with kernel 1 / 3 / 5,
// padding (k - 1) / 2, stride 1 or 2, and nn.ConvTranspose2d with stride 2, on [B, H, W, C] memory).  f32 / f16 / bf16, fp32
// accumulation, no float atomics: every result depends bit for bit on its operands alone.
//
//   wcn_dense_conv2d        y[o, :] = sum_delta x[s * o + delta - pad, :] @ W[delta] (+ bias).  Also the input gradient of a
//                           stride-1 convolution (flipped, transposed pack) and of the transposed convolution (s = 2).
//   wcn_dense_conv2d_frac   y[2 i + delta - pad, :] += x[i, :] @ W[delta] (+ bias): the forward of ConvTranspose2d(stride 2) and
//                           the input gradient of the stride-2 convolution, without zero-stuffing.
//   wcn_dense_conv2d_wgrad  dW[co, ci, delta] = sum_o x[s * o + delta - pad, ci] * dy[o, co], dbias = column sums.
//
// Strided forward.  A workgroup of four waves owns 8 x 16 output pixels (128 GEMM rows) and a block of 64 or 128 output
// channels, and walks tiles t = blockIdx.x, + gridDim.x, ... (the grid is capped).  Input channels go by chunks of 128 B per
// pixel at stride 1 and 64 B at stride 2: per chunk the workgroup stages the tile's input halo ((s 8 + k - s) x (s 16 + k - s)
// pixels; zeros outside the image - that IS the padding, coordinates are compared per axis and nothing wraps into the next row
// or batch element) into LDS once and runs all k^2 offsets against it: the A fragment of output pixel (ty, tx) at offset
// (ky, kx) is the 16-B LDS read at halo pixel (s ty + ky, s tx + kx), the B fragment a 16-B read of the packed weight
// (L2-resident; the image of the NEXT offset is fetched while the current one multiplies).  The waves sit 2 x 2 on the tile:
// four output rows (two fragments of 2 x 16 pixels) by 32 or 64 channels each.  The LDS pitch is the chunk + 16 B.
//
// Fractionally-strided form.  The parity (oy & 1, ox & 1) of an output pixel decides which taps reach it: ky = oy + pad mod 2,
// kx likewise, so every tap belongs to exactly one of the four parity classes and a class of a k = 3 kernel has 1, 2, 2 or 4
// taps (k = 5: 9, 6, 6, 4; k = 1: 1, 0, 0, 0).  A workgroup owns 8 x 32 output pixels = 4 x 16 pixels of every class and stages
// the COARSE image's halo of that tile ((4 + e) x (16 + e) pixels, e = 0 / 1 / 2 for k = 1 / 3 / 5).  An MFMA fragment holds 32
// pixels of ONE class (two class rows of 16), so a product is issued only for a tap its rows really have; every wave owns one
// fragment of each of the four classes (waves 2 x 2: class rows x channels), so all waves issue the same k^2 products per
// chunk however unequal the classes are.  Output pixels no tap reaches are stored as bias (or an exact 0).
//
// Packed weight: [k^2][Kpad / S][Npad][S] as in dense_conv3d.hip, Kpad a multiple of the 128-B chunk; padded lanes are zero.
// Epilogue in fp32: acc + bias is one fp32 add, rounded once to the storage type.
//
// Weight gradient.  Grid = pixel slab x (Cin block x Cout block of 64 x 64) x offset, the staged tiles, K-major reads
// (ds_read_b64_tr_b16 for the 16-bit types), fp32 partials and ordered reduce of dense_conv.h.  Slabs run over OUTPUT pixels;
// the x row of output pixel o at offset delta is s o + delta - pad (zeros outside the image).  The bias gradient sums the
// rows of dy or, for the transposed module (whose x and dy are exchanged), of x.
#include "dense_conv.h"

namespace wcn {

constexpr int kC2TH = 8, kC2TW = 16;  // output tile of a strided-forward workgroup
constexpr int kC2FH = 4, kC2FW = 16;  // fractionally-strided: pixels of one parity class per workgroup (8 x 32 outputs)
constexpr int kC2MaxGrid = 1024;      // workgroups of a forward / fractional launch (four per CU); the rest is walked

template <int V> using c2_int = std::integral_constant<int, V>;

// ---- weight pack -----------------------------------------------------------------------------------------------------------
// w [Cout, Cin, kv] -> packed [kv][kpad / S][npad][S].  mode 0: K = Cin, N = Cout.  mode 1: K = Cout, N = Cin, offsets
// reversed (stride-1 input gradient).  mode 2: K = Cout, N = Cin, offsets as they are (fractionally-strided form).
template <typename T>
__global__ __launch_bounds__(kDcThreads) void dense_conv2d_pack_kernel(const T* __restrict__ w, T* __restrict__ packed, int cin,
                                                                       int cout, int kv, int kpad, int npad, int mode) {
  constexpr int S = 2 * DcOp<T>::E;
  const int64_t total = (int64_t)kv * kpad * npad;
  for (int64_t i = (int64_t)blockIdx.x * kDcThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kDcThreads) {
    const int kk = (int)(i % S);
    int64_t t = i / S;
    const int n = (int)(t % npad);
    t /= npad;
    const int sg = (int)(t % (kpad / S));
    const int delta = (int)(t / (kpad / S));
    const int k = sg * S + kk;
    T v = (T)0.f;
    if (mode == 0) {
      if (k < cin && n < cout) v = w[((int64_t)n * cin + k) * kv + delta];
    } else {
      if (k < cout && n < cin) v = w[((int64_t)k * cin + n) * kv + (mode == 1 ? kv - 1 - delta : delta)];
    }
    packed[i] = v;
  }
}

// B fragments of one offset and chunk: STEPS x NB 16-B pieces of the lane's columns
template <typename T, int STEPS, int NB>
__device__ __forceinline__ void c2_load_b(Vec<T, DcOp<T>::E> (&b)[STEPS][NB], const T* __restrict__ wlane, int64_t wstep) {
  constexpr int S = 2 * DcOp<T>::E;
#pragma unroll
  for (int s = 0; s < STEPS; ++s)
#pragma unroll
    for (int j = 0; j < NB; ++j) b[s][j] = *reinterpret_cast<const Vec<T, DcOp<T>::E>*>(wlane + s * wstep + (int64_t)j * 32 * S);
}

// the staged halo: HH x HW pixels from (gy0, gx0) of image `b` (ih x iw pixels of `cin` channels), channels from `k0`
template <typename T, int HH, int HW, int PIECES, int PITCH>
__device__ __forceinline__ void c2_stage_halo(char* s_halo, const T* __restrict__ x, int64_t b, int gy0, int gx0, int ih, int iw,
                                              int cin, int k0, int xvec) {
  constexpr int E = DcOp<T>::E;
  for (int p = threadIdx.x; p < HH * HW * PIECES; p += kDcThreads) {
    const int hv = p / PIECES, piece = p % PIECES;
    const int gy = gy0 + hv / HW, gx = gx0 + hv % HW;
    Vec<T, E> v = dc_zero<T, E>();
    if ((unsigned)gy < (unsigned)ih && (unsigned)gx < (unsigned)iw)
      v = dc_load_piece<T, E>(x + (((int64_t)b * ih + gy) * iw + gx) * cin, k0 + piece * E, cin, xvec);
    *reinterpret_cast<Vec<T, E>*>(s_halo + hv * PITCH + piece * 16) = v;
  }
}

// ---- strided forward / input gradient of stride 1 and of the transposed convolution ----------------------------------------
template <typename T, int KS, int ST, int NB>
__global__ __launch_bounds__(kDcThreads) void dense_conv2d_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                                  const T* __restrict__ bias, T* __restrict__ y, int64_t tiles,
                                                                  int H, int W, int Ho, int Wo, int cin, int cout, int kpad,
                                                                  int npad, int xvec) {
  constexpr int RB = ST == 1 ? 128 : 64, PITCH = RB + 16;
  constexpr int E = DcOp<T>::E, S = 2 * E, CK = RB / (int)sizeof(T), STEPS = RB / 32, PIECES = RB / 16;
  constexpr int PAD = (KS - 1) / 2, KV = KS * KS;
  constexpr int HH = ST * kC2TH + KS - ST, HW = ST * kC2TW + KS - ST;
  __shared__ __attribute__((aligned(16))) char s_halo[HH * HW * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, r = lane & 31;
  const int ntw = (Wo + kC2TW - 1) / kC2TW, nth = (Ho + kC2TH - 1) / kC2TH;
  const int ncol0 = blockIdx.y * (64 * NB) + wn * (32 * NB) + r;  // the lane's column of block j: ncol0 + 32 j (< npad)
  const int nchunk = (cin + CK - 1) / CK;
  const int nsteps = kpad / S;  // fragment steps of the whole reduction
  const int64_t wstep = (int64_t)npad * S;

  // the lane's two A rows: output pixel (4 wm + 2 i + r / 16, r % 16) of the tile
  int hbase[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) hbase[i] = ST * ((4 * wm + 2 * i + (r >> 4)) * HW + (r & 15));

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ox0 = (int)(tile % ntw) * kC2TW;
    const int oy0 = (int)((tile / ntw) % nth) * kC2TH;
    const int64_t b = tile / ((int64_t)ntw * nth);

    f32x16 acc[2][NB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    for (int chunk = 0; chunk < nchunk; ++chunk) {
      __syncthreads();  // the sweep of the chunk (or tile) before is over
      c2_stage_halo<T, HH, HW, PIECES, PITCH>(s_halo, x, b, ST * oy0 - PAD, ST * ox0 - PAD, H, W, cin, chunk * CK, xvec);
      __syncthreads();

      // B fragments of (delta, chunk): wp + ((delta * nsteps + chunk * STEPS + s) * npad + n) * S + E * half
      const T* wlane = wp + ((int64_t)chunk * STEPS * npad + ncol0) * S + E * half;
      Vec<T, E> bcur[STEPS][NB], bnxt[STEPS][NB];
      c2_load_b<T, STEPS, NB>(bcur, wlane, wstep);
      for (int delta = 0; delta < KV; ++delta) {
        if (delta + 1 < KV) c2_load_b<T, STEPS, NB>(bnxt, wlane + (int64_t)(delta + 1) * nsteps * wstep, wstep);
        const int hoff = (delta / KS) * HW + delta % KS;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
          Vec<T, E> af[2];
#pragma unroll
          for (int i = 0; i < 2; ++i)
            af[i] = *reinterpret_cast<const Vec<T, E>*>(s_halo + (hbase[i] + hoff) * PITCH + s * 32 + half * 16);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = DcOp<T>::mma(af[i], bcur[s][j], acc[i][j]);
        }
        if (delta + 1 < KV) {
#pragma unroll
          for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int j = 0; j < NB; ++j) bcur[s][j] = bnxt[s][j];
        }
      }
    }

    // result block: column lane % 32, rows 8 (q / 4) + 4 (lane / 32) + q % 4
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int n = ncol0 + 32 * j;
        if (n >= cout) continue;
        const float bv = bias ? (float)bias[n] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = 8 * (q >> 2) + 4 * half + (q & 3);
          const int oy = oy0 + 4 * wm + 2 * i + (row >> 4), ox = ox0 + (row & 15);
          if (oy >= Ho || ox >= Wo) continue;
          y[(((int64_t)b * Ho + oy) * Wo + ox) * cout + n] = (T)(acc[i][j][q] + bv);
        }
      }
    }
  }
}

// ---- fractionally-strided form (stride 2) ----------------------------------------------------------------------------------
template <typename T, int KS, int NB>
__global__ __launch_bounds__(kDcThreads) void dense_conv2d_frac_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                                       const T* __restrict__ bias, T* __restrict__ y,
                                                                       int64_t tiles, int Hc, int Wc, int Ho, int Wo, int cin,
                                                                       int cout, int kpad, int npad, int xvec) {
  constexpr int RB = 128, PITCH = RB + 16;
  constexpr int E = DcOp<T>::E, S = 2 * E, CK = RB / (int)sizeof(T), STEPS = RB / 32, PIECES = RB / 16;
  constexpr int PAD = (KS - 1) / 2;
  // output o = 2 a + c (class c, class pixel a) takes tap k = c + PAD mod 2 from coarse pixel a + e, e = (c + PAD - k) / 2
  constexpr int EMIN = -(PAD / 2), EMAX = (1 + PAD) / 2;
  constexpr int HH = kC2FH + EMAX - EMIN, HW = kC2FW + EMAX - EMIN;
  __shared__ __attribute__((aligned(16))) char s_halo[HH * HW * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, r = lane & 31;
  const int ntw = (Wo + 2 * kC2FW - 1) / (2 * kC2FW), nth = (Ho + 2 * kC2FH - 1) / (2 * kC2FH);
  const int ncol0 = blockIdx.y * (64 * NB) + wn * (32 * NB) + r;
  const int nchunk = (cin + CK - 1) / CK;
  const int nsteps = kpad / S;
  const int64_t wstep = (int64_t)npad * S;
  const int hbase = (2 * wm + (r >> 4)) * HW + (r & 15);  // the lane's class pixel (2 wm + r / 16, r % 16), in every class

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ox0 = (int)(tile % ntw) * (2 * kC2FW);
    const int oy0 = (int)((tile / ntw) % nth) * (2 * kC2FH);
    const int64_t b = tile / ((int64_t)ntw * nth);

    f32x16 acc[4][NB];  // one fragment per parity class
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[c][j][q] = 0.f;

    for (int chunk = 0; chunk < nchunk; ++chunk) {
      __syncthreads();
      c2_stage_halo<T, HH, HW, PIECES, PITCH>(s_halo, x, b, oy0 / 2 + EMIN, ox0 / 2 + EMIN, Hc, Wc, cin, chunk * CK, xvec);
      __syncthreads();

      const T* wlane = wp + ((int64_t)chunk * STEPS * npad + ncol0) * S + E * half;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int cy = c >> 1, cx = c & 1;
        const int ky0 = (cy + PAD) & 1, kx0 = (cx + PAD) & 1;          // the class's first tap per axis; the others 2 apart
        const int nky = (KS - ky0 + 1) / 2, nkx = (KS - kx0 + 1) / 2;  // taps per axis: only these reach the class
        const int ntap = nky * nkx;
        if (ntap == 0) continue;
        Vec<T, E> bcur[STEPS][NB], bnxt[STEPS][NB];
        c2_load_b<T, STEPS, NB>(bcur, wlane + (int64_t)(ky0 * KS + kx0) * nsteps * wstep, wstep);
        for (int t = 0; t < ntap; ++t) {
          const int ky = ky0 + 2 * (t / nkx), kx = kx0 + 2 * (t % nkx);
          if (t + 1 < ntap) {
            const int ky1 = ky0 + 2 * ((t + 1) / nkx), kx1 = kx0 + 2 * ((t + 1) % nkx);
            c2_load_b<T, STEPS, NB>(bnxt, wlane + (int64_t)(ky1 * KS + kx1) * nsteps * wstep, wstep);
          }
          const int hoff = ((cy + PAD - ky) / 2 - EMIN) * HW + (cx + PAD - kx) / 2 - EMIN;
#pragma unroll
          for (int s = 0; s < STEPS; ++s) {
            const Vec<T, E> af = *reinterpret_cast<const Vec<T, E>*>(s_halo + (hbase + hoff) * PITCH + s * 32 + half * 16);
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[c][j] = DcOp<T>::mma(af, bcur[s][j], acc[c][j]);
          }
          if (t + 1 < ntap) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s)
#pragma unroll
              for (int j = 0; j < NB; ++j) bcur[s][j] = bnxt[s][j];
          }
        }
      }
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int n = ncol0 + 32 * j;
        if (n >= cout) continue;
        const float bv = bias ? (float)bias[n] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = 8 * (q >> 2) + 4 * half + (q & 3);
          const int oy = oy0 + 2 * (2 * wm + (row >> 4)) + (c >> 1), ox = ox0 + 2 * (row & 15) + (c & 1);
          if (oy >= Ho || ox >= Wo) continue;
          y[(((int64_t)b * Ho + oy) * Wo + ox) * cout + n] = (T)(acc[c][j][q] + bv);
        }
      }
    }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
template <typename T, int KS>
__global__ __launch_bounds__(kDcThreads) void dense_conv2d_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                        float* __restrict__ part, int H, int W, int Ho, int Wo,
                                                                        int st, int cin, int cout, int64_t npix,
                                                                        int64_t slab_pix, int xvec, int yvec) {
  typedef DwTile<T> TL;
  constexpr int E = TL::E, PAD = (KS - 1) / 2, KV = KS * KS;
  __shared__ __attribute__((aligned(16))) char s_x[TL::BYTES];
  __shared__ __attribute__((aligned(16))) char s_y[TL::BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, half = lane >> 5, r = lane & 31;
  const int nco = (cout + kDwTile - 1) / kDwTile;
  const int ci0 = (blockIdx.y / nco) * kDwTile, co0 = (blockIdx.y % nco) * kDwTile;
  const int delta = blockIdx.z;
  const int dh = delta / KS - PAD, dw = delta % KS - PAD;
  const int64_t v_begin = (int64_t)blockIdx.x * slab_pix;
  const int64_t v_end = v_begin + slab_pix < npix ? v_begin + slab_pix : npix;
  const int nstep = (int)((v_end - v_begin + TL::VSTEP - 1) / TL::VSTEP);  // >= 1: the host launches no empty slab

  Vec<T, E> px[TL::PER], py[TL::PER];
  auto fetch = [&](int step) {
#pragma unroll
    for (int i = 0; i < TL::PER; ++i) {
      const int p = tid + kDcThreads * i;
      const int lv = p / TL::PPR, piece = p % TL::PPR;
      const int64_t v = v_begin + (int64_t)step * TL::VSTEP + lv;
      px[i] = dc_zero<T, E>();
      py[i] = dc_zero<T, E>();
      if (v < v_end) {
        py[i] = dc_load_piece<T, E>(dy + v * cout, co0 + piece * E, cout, yvec);
        const int ox = (int)(v % Wo);
        const int64_t q = v / Wo;
        const int oy = (int)(q % Ho);
        const int64_t b = q / Ho;
        const int iy = st * oy + dh, ix = st * ox + dw;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
          px[i] = dc_load_piece<T, E>(x + ((b * H + iy) * W + ix) * cin, ci0 + piece * E, cin, xvec);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < TL::PER; ++i) {
      const int p = tid + kDcThreads * i;
      const int at = dw_piece_at<T>(p / TL::PPR, p % TL::PPR);
      *reinterpret_cast<Vec<T, E>*>(s_x + at) = px[i];
      *reinterpret_cast<Vec<T, E>*>(s_y + at) = py[i];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  fetch(0);
  stage();
  __syncthreads();
  for (int step = 0; step < nstep; ++step) {
    if (step + 1 < nstep) fetch(step + 1);
    acc = dw_step_mma<T>(s_x, s_y, wi, wj, lane, acc);
    __syncthreads();
    if (step + 1 < nstep) stage();
    __syncthreads();
  }

  float* __restrict__ out = part + ((int64_t)blockIdx.x * KV + delta) * cin * cout;
  const int co = co0 + 32 * wj + r;
  if (co < cout) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int ci = ci0 + 32 * wi + 8 * (q >> 2) + 4 * half + (q & 3);
      if (ci < cin) out[(int64_t)ci * cout + co] = acc[q];
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static bool c2_ks_ok(int ks) { return ks == 1 || ks == 3 || ks == 5; }
static bool c2_shape_ok(int cin, int cout, int ks, int stride, int dtype) {
  return dtype_ok(dtype) && c2_ks_ok(ks) && (stride == 1 || stride == 2) && cin >= 1 && cout >= 1 && cin <= 8192 &&
         cout <= 8192;  // (grid.y of dW)
}
static int c2_kpad(int k, int dtype) { return dc_round(k, 128 / dtype_bytes(dtype)); }  // whole 128-B chunks
static int c2_npad(int n) { return dc_round(n, 64 * dc_nb(n)); }
static int c2_out(int size, int stride) { return (size - 1) / stride + 1; }

// f(c2_int<KS>{}) for ks in {1, 3, 5}
template <typename F>
static void c2_with_ks(int ks, F&& f) {
  if (ks == 1) f(c2_int<1>{});
  else if (ks == 3) f(c2_int<3>{});
  else f(c2_int<5>{});
}

}  // namespace wcn

using namespace wcn;

int wcn_dense_conv2d_supported(int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t dtype) {
  return c2_shape_ok(cin, cout, ks, stride, dtype) ? 1 : 0;
}

size_t wcn_dense_conv2d_packed_bytes(int32_t cin, int32_t cout, int32_t ks, int32_t dtype, int32_t mode) {
  if (!c2_shape_ok(cin, cout, ks, 1, dtype) || mode < 0 || mode > 2) return 0;
  const int k = mode ? cout : cin, n = mode ? cin : cout;
  return (size_t)ks * ks * c2_kpad(k, dtype) * c2_npad(n) * dtype_bytes(dtype);
}

int wcn_dense_conv2d_pack(const void* w, int32_t cin, int32_t cout, int32_t ks, int32_t dtype, int32_t mode, void* packed,
                          size_t packed_bytes, wcn_stream_t stream) {
  if (cin < 1 || cout < 1 || mode < 0 || mode > 2) return WCN_ERROR_INVALID_PARAMETERS;
  if (!c2_shape_ok(cin, cout, ks, 1, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!w || !packed || !aligned_to(w, dtype_bytes(dtype)) || !aligned_to(packed, 16) ||
      packed_bytes < wcn_dense_conv2d_packed_bytes(cin, cout, ks, dtype, mode))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int k = mode ? cout : cin, n = mode ? cin : cout, kv = ks * ks;
  const int kpad = c2_kpad(k, dtype), npad = c2_npad(n);
  const int64_t total = (int64_t)kv * kpad * npad;
  const unsigned grid = (unsigned)(ceil_div(total, kDcThreads) < 4096 ? ceil_div(total, kDcThreads) : 4096);
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(dense_conv2d_pack_kernel<T>, dim3(grid), dim3(kDcThreads), 0, (hipStream_t)stream, (const T*)w, (T*)packed,
                       cin, cout, kv, kpad, npad, mode);
    return 0;
  });
  return launch_status();
}

// the checks the two image launches share; *tiles = workgroup tiles of th x tw output pixels
static int c2_check_launch(const void* x, const void* packed, const void* bias, const void* y, int64_t batch, int Ho, int Wo,
                           int th, int tw, int dtype, int64_t* tiles) {
  const size_t el = dtype_bytes(dtype);
  if (!x || !packed || !y || !aligned_to(x, el) || !aligned_to(y, el) || !aligned_to(bias, el) || !aligned_to(packed, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  *tiles = batch * ceil_div(Ho, th) * ceil_div(Wo, tw);
  return WCN_SUCCESS;
}

int wcn_dense_conv2d(const void* x, const void* packed, const void* bias, void* y, int64_t batch, int32_t H, int32_t W,
                     int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t dtype, wcn_stream_t stream) {
  if (batch < 0 || H < 0 || W < 0 || cin < 1 || cout < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (!c2_shape_ok(cin, cout, ks, stride, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (batch == 0 || H == 0 || W == 0) return WCN_SUCCESS;  // no pixels, no launch
  const int Ho = c2_out(H, stride), Wo = c2_out(W, stride);
  int64_t tiles;
  const int rc = c2_check_launch(x, packed, bias, y, batch, Ho, Wo, kC2TH, kC2TW, dtype, &tiles);
  if (rc != WCN_SUCCESS) return rc;
  const int nb = dc_nb(cout), kpad = c2_kpad(cin, dtype), npad = c2_npad(cout);
  const dim3 grid((unsigned)(tiles < kC2MaxGrid ? tiles : kC2MaxGrid), (unsigned)(npad / (64 * nb)));
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = cin % DcOp<T>::E == 0 && aligned_to(x, 16);
    c2_with_ks(ks, [&](auto kc) {
      constexpr int KS = decltype(kc)::value;
      auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kDcThreads), 0, (hipStream_t)stream, (const T*)x, (const T*)packed, (const T*)bias,
                           (T*)y, tiles, H, W, Ho, Wo, cin, cout, kpad, npad, xvec);
      };
      if (stride == 1) { if (nb == 2) go(dense_conv2d_kernel<T, KS, 1, 2>); else go(dense_conv2d_kernel<T, KS, 1, 1>); }
      else { if (nb == 2) go(dense_conv2d_kernel<T, KS, 2, 2>); else go(dense_conv2d_kernel<T, KS, 2, 1>); }
    });
    return 0;
  });
  return launch_status();
}

int wcn_dense_conv2d_frac(const void* x, const void* packed, const void* bias, void* y, int64_t batch, int32_t Hc, int32_t Wc,
                          int32_t Ho, int32_t Wo, int32_t cin, int32_t cout, int32_t ks, int32_t dtype, wcn_stream_t stream) {
  if (batch < 0 || Hc < 0 || Wc < 0 || Ho < 0 || Wo < 0 || cin < 1 || cout < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (!c2_shape_ok(cin, cout, ks, 2, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (batch == 0 || Ho == 0 || Wo == 0) return WCN_SUCCESS;  // no output pixels, no launch
  int64_t tiles;
  const int rc = c2_check_launch(x, packed, bias, y, batch, Ho, Wo, 2 * kC2FH, 2 * kC2FW, dtype, &tiles);
  if (rc != WCN_SUCCESS) return rc;
  const int nb = dc_nb(cout), kpad = c2_kpad(cin, dtype), npad = c2_npad(cout);
  const dim3 grid((unsigned)(tiles < kC2MaxGrid ? tiles : kC2MaxGrid), (unsigned)(npad / (64 * nb)));
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = cin % DcOp<T>::E == 0 && aligned_to(x, 16);
    c2_with_ks(ks, [&](auto kc) {
      constexpr int KS = decltype(kc)::value;
      auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kDcThreads), 0, (hipStream_t)stream, (const T*)x, (const T*)packed, (const T*)bias,
                           (T*)y, tiles, Hc, Wc, Ho, Wo, cin, cout, kpad, npad, xvec);
      };
      if (nb == 2) go(dense_conv2d_frac_kernel<T, KS, 2>); else go(dense_conv2d_frac_kernel<T, KS, 1>);
    });
    return 0;
  });
  return launch_status();
}

int32_t wcn_dense_conv2d_wgrad_slabs(int64_t pixels, int32_t cin, int32_t cout, int32_t ks, int32_t dtype) {
  if (pixels <= 0 || !c2_shape_ok(cin, cout, ks, 1, dtype)) return 0;
  return dw_slabs(pixels, cin, cout, ks * ks, dtype);
}

size_t wcn_dense_conv2d_wgrad_workspace(int32_t cin, int32_t cout, int32_t ks, int32_t slabs) {
  if (cin < 1 || cout < 1 || slabs < 1 || !c2_ks_ok(ks)) return 0;
  return align256((size_t)slabs * ks * ks * cin * cout * sizeof(float)) +
         (size_t)kDwBiasParts * (cin > cout ? cin : cout) * sizeof(float);
}

int wcn_dense_conv2d_wgrad(const void* x, const void* dy, int64_t batch, int32_t H, int32_t W, int32_t cin, int32_t cout,
                           int32_t ks, int32_t stride, int32_t dtype, int32_t slabs, int32_t dbias_from_x, void* dw, void* dbias,
                           void* workspace, size_t workspace_bytes, wcn_stream_t stream) {
  if (batch < 0 || H < 0 || W < 0 || cin < 1 || cout < 1 || slabs < 0 || slabs > kDwMaxSlabs)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!c2_shape_ok(cin, cout, ks, stride, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (batch == 0 || H == 0 || W == 0) return WCN_SUCCESS;  // no pixels, no launch: the caller's zeros stand
  const int Ho = c2_out(H, stride), Wo = c2_out(W, stride);
  const int64_t npix = batch * Ho * Wo;
  if (slabs == 0) slabs = wcn_dense_conv2d_wgrad_slabs(npix, cin, cout, ks, dtype);
  const size_t el = dtype_bytes(dtype);
  if (!x || !dy || !dw || !workspace || !aligned_to(x, el) || !aligned_to(dy, el) || !aligned_to(dw, el) ||
      !aligned_to(dbias, el) || !aligned_to(workspace, 256) ||
      workspace_bytes < wcn_dense_conv2d_wgrad_workspace(cin, cout, ks, slabs))
    return WCN_ERROR_INVALID_PARAMETERS;
  int64_t slab_pix;
  int used;
  dw_plan(npix, slabs, dtype, &slab_pix, &used);
  const int kv = ks * ks;
  float* part = (float*)workspace;
  float* bpart = (float*)((char*)workspace + align256((size_t)slabs * kv * cin * cout * sizeof(float)));
  const dim3 grid((unsigned)used, (unsigned)(ceil_div(cin, kDwTile) * ceil_div(cout, kDwTile)), (unsigned)kv);
  hipStream_t s = (hipStream_t)stream;
  const int nbias = dbias_from_x ? cin : cout;
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = cin % DcOp<T>::E == 0 && aligned_to(x, 16), yvec = cout % DcOp<T>::E == 0 && aligned_to(dy, 16);
    c2_with_ks(ks, [&](auto kc) {
      constexpr int KS = decltype(kc)::value;
      hipLaunchKernelGGL((dense_conv2d_wgrad_kernel<T, KS>), grid, dim3(kDcThreads), 0, s, (const T*)x, (const T*)dy, part, H, W,
                         Ho, Wo, stride, cin, cout, npix, slab_pix, xvec, yvec);
    });
    if (dbias)
      hipLaunchKernelGGL(dense_conv_dbias_kernel<T>, dim3(kDwBiasParts), dim3(kDcThreads), 0, s,
                         (const T*)(dbias_from_x ? x : dy), bpart, dbias_from_x ? batch * H * W : npix, nbias);
    const int64_t total = (int64_t)kv * cin * cout + nbias;
    const unsigned rgrid = (unsigned)(ceil_div(total, kDcThreads) < 8192 ? ceil_div(total, kDcThreads) : 8192);
    hipLaunchKernelGGL(dense_conv_wgrad_reduce_kernel<T>, dim3(rgrid), dim3(kDcThreads), 0, s, (const float*)part,
                       (const float*)bpart, used, kv, cin, cout, nbias, (T*)dw, (T*)dbias);
    return 0;
  });
  return launch_status();
}
