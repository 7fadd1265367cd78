// dense_conv3d.hip - dense 3-D "brick" convolution on channels-last cubes (the TRELLIS.2 sparse-structure VAE: nn.Conv3d with
// kernel 3 / padding 1 or kernel 1, stride 1, on [B, D, H, W, C] memory).  f32 / f16 / bf16, fp32 accumulation, no float
// atomics: every result depends bit for bit on its operands alone.
//
//   wcn_dense_conv3d        y[v, :] = sum_delta x[v + delta - pad, :] @ W[delta]  (+ bias) (+ residual), optionally stored
//                           through a factor-2 pixel shuffle.  The input gradient is the same launch on dY with the flipped,
//                           transposed weight image (wcn_dense_conv3d_pack with dgrad = 1).
//   wcn_dense_conv3d_wgrad  dW[delta, ci, co] = sum_v x[v + delta - pad, ci] * dy[v, co], dbias = column sums of dy.
//
// Forward / dgrad.  A workgroup of four waves owns a tile of 4 x 4 x 8 output voxels (128 GEMM rows) and a block of 64 or 128
// output channels.  Input channels go by chunks of 128 B per voxel (64 halves / 32 floats): per chunk the workgroup stages the
// tile's halo ((4 + KS - 1) x (4 + KS - 1) x (8 + KS - 1) voxels, zeros outside the volume - that IS the padding, nothing
// wraps into a neighbouring row, plane or batch element) into LDS once and runs all KS^3 offsets against it: the A fragment
// of output voxel m at offset delta is the 16-B LDS read at halo_index(m) + delta, the B fragment a 16-B read of the packed
// weight (L2-resident; the image of the NEXT offset is fetched while the current one multiplies).  The waves sit 2 x 2 on the
// tile: 64 voxels (two d-planes) by 32 or 64 channels each, v_mfma_f32_32x32x16_{f16,bf16} or, for fp32 tensors,
// v_mfma_f32_32x32x2f32 on exact fp32 operands.  LDS rows have a pitch of 144 B so that the eight voxels of a w-run fall
// into different banks.
//
// Packed weight: [KS^3][Kpad / S][Npad][S] with S = the reduction step of one fragment pair (16 halves / 8 floats), Kpad a
// multiple of the chunk and Npad of the channel block; everything off the real [K, N] is zero, and so is whatever the
// staging reads past the last input channel: padded lanes contribute exact zeros.
//
// Epilogue in fp32, one rounding to the storage type: acc + bias is one fp32 add.  With a residual two fp32 adds would round
// twice, f |acc + bias| + f |acc + bias + residual|, which counts the bias twice and leaves f (n + 2) A + f |bias| + f |residual|
// where |bias| > A; so the three-term sum alone is formed in fp64 and rounded to fp32 once.
//
// Weight gradient.  Grid = spatial slab x (Cin block x Cout block of 64 x 64) x offset.  A workgroup sweeps its slab in
// steps of 128 voxels (64 for fp32): the shifted x rows (zeros where v + delta leaves the volume) and the dy rows go through
// registers into two row-major LDS tiles (the next step's loads are in flight during the products) and are read K-major:
// ds_read_b64_tr_b16 for the 16-bit types (with the chunk swizzle of wgrad_mfma.hip), plain 4-B reads for fp32.  fp32
// partials [slab][delta][ci][co] are added in slab order by the reduce kernel, which writes nn.Conv3d's [Cout, Cin, k, k, k]
// in the weight's type and adds the 64 row-range partials of dbias in order.  The slab count is a function of the shape.
#include "dense_conv.h"

namespace wcn {

constexpr int kDcTD = 4, kDcTH = 4, kDcTW = 8;  // output tile of a forward workgroup
constexpr int kDcRowBytes = 128;                // input channels of one chunk, in bytes per voxel
constexpr int kDcPitch = kDcRowBytes + 16;      // LDS pitch of a staged voxel

// ---- weight pack -----------------------------------------------------------------------------------------------------------
// w [Cout, Cin, kv] -> packed [kv][kpad / S][npad][S].  Forward: K = Cin, N = Cout.  dgrad: K = Cout, N = Cin, offsets reversed.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void dense_conv3d_pack_kernel(const T* __restrict__ w, T* __restrict__ packed, int cin,
                                                                       int cout, int kv, int kpad, int npad, int dgrad) {
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
    if (!dgrad) {
      if (k < cin && n < cout) v = w[((int64_t)n * cin + k) * kv + delta];
    } else {
      if (k < cout && n < cin) v = w[((int64_t)k * cin + n) * kv + (kv - 1 - delta)];
    }
    packed[i] = v;
  }
}

// ---- forward / input gradient ----------------------------------------------------------------------------------------------
template <typename T, int KS, int NB>
__global__ __launch_bounds__(kDcThreads) void dense_conv3d_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                                  const T* __restrict__ bias, const T* __restrict__ res,
                                                                  T* __restrict__ y, int D, int H, int W, int cin, int cout,
                                                                  int kpad, int npad, int ps, int xvec) {
  constexpr int E = DcOp<T>::E, S = 2 * E, CK = kDcRowBytes / (int)sizeof(T), STEPS = CK / S;
  constexpr int PAD = (KS - 1) / 2, KV = KS * KS * KS;
  constexpr int HD = kDcTD + KS - 1, HH = kDcTH + KS - 1, HW = kDcTW + KS - 1, HALO = HD * HH * HW;
  constexpr int PIECES = kDcRowBytes / 16;
  static_assert(STEPS == 4 && PIECES == 8, "a chunk is four fragment steps of 32 B");
  __shared__ __attribute__((aligned(16))) char s_halo[HALO * kDcPitch];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, r = lane & 31;
  const int ntw = (W + kDcTW - 1) / kDcTW, nth = (H + kDcTH - 1) / kDcTH, ntd = (D + kDcTD - 1) / kDcTD;
  int t = blockIdx.x;
  const int w0 = (t % ntw) * kDcTW;
  t /= ntw;
  const int h0 = (t % nth) * kDcTH;
  t /= nth;
  const int d0 = (t % ntd) * kDcTD;
  const int64_t b = t / ntd;
  const int ncol0 = blockIdx.y * (64 * NB) + wn * (32 * NB) + r;  // the lane's column of block j: ncol0 + 32 j (< npad)

  // the lane's two A rows: voxel (2 wm + i, r / 8, r % 8) of the tile
  int hbase[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) hbase[i] = ((2 * wm + i) * HH + (r >> 3)) * HW + (r & 7);

  f32x16 acc[2][NB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  const int nsteps = kpad / S;  // fragment steps of the whole reduction
  const int64_t wstep = (int64_t)npad * S;
  for (int chunk = 0; chunk < kpad / CK; ++chunk) {
    __syncthreads();  // the sweep of the chunk before is over
    for (int p = tid; p < HALO * PIECES; p += kDcThreads) {
      const int hv = p >> 3, piece = p & 7;
      const int gw = w0 - PAD + hv % HW, gh = h0 - PAD + (hv / HW) % HH, gd = d0 - PAD + hv / (HW * HH);
      Vec<T, E> v = dc_zero<T, E>();
      if ((unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W)
        v = dc_load_piece<T, E>(x + ((((int64_t)b * D + gd) * H + gh) * W + gw) * cin, chunk * CK + piece * E, cin, xvec);
      *reinterpret_cast<Vec<T, E>*>(s_halo + hv * kDcPitch + piece * 16) = v;
    }
    __syncthreads();

    // B fragments of (delta, chunk): wp + ((delta * nsteps + chunk * STEPS + s) * npad + n) * S + E * half
    const T* wlane = wp + ((int64_t)chunk * STEPS * npad + ncol0) * S + E * half;
    Vec<T, E> bcur[STEPS][NB], bnxt[STEPS][NB];
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
#pragma unroll
      for (int j = 0; j < NB; ++j) bcur[s][j] = *reinterpret_cast<const Vec<T, E>*>(wlane + s * wstep + (int64_t)j * 32 * S);
    for (int delta = 0; delta < KV; ++delta) {
      if (delta + 1 < KV) {
        const T* wnext = wlane + (int64_t)(delta + 1) * nsteps * wstep;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
          for (int j = 0; j < NB; ++j) bnxt[s][j] = *reinterpret_cast<const Vec<T, E>*>(wnext + s * wstep + (int64_t)j * 32 * S);
      }
      const int hoff = ((delta / (KS * KS)) * HH + (delta / KS) % KS) * HW + delta % KS;
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        Vec<T, E> af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
          af[i] = *reinterpret_cast<const Vec<T, E>*>(s_halo + (hbase[i] + hoff) * kDcPitch + s * 32 + half * 16);
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
  const int cfine = cout >> 3;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int d = d0 + 2 * wm + i;
    if (d >= D) continue;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = ncol0 + 32 * j;
      if (n >= cout) continue;
      const float bv = bias ? (float)bias[n] : 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 8 * (q >> 2) + 4 * half + (q & 3);
        const int h = h0 + (row >> 3), w = w0 + (row & 7);
        if (h >= H || w >= W) continue;
        int64_t idx;
        if (ps) {  // channel c * 8 + (sd, sh, sw) of the coarse voxel -> channel c of fine voxel (2d + sd, 2h + sh, 2w + sw)
          const int sub = n & 7;
          idx = ((((int64_t)b * (2 * D) + 2 * d + (sub >> 2)) * (2 * H) + 2 * h + ((sub >> 1) & 1)) * (2 * W) + 2 * w + (sub & 1)) *
                    cfine + (n >> 3);
        } else {
          idx = ((((int64_t)b * D + d) * H + h) * W + w) * cout + n;
        }
        float o = acc[i][j][q] + bv;
        if (res) o = (float)((double)acc[i][j][q] + (double)bv + (double)(float)res[idx]);
        y[idx] = (T)o;
      }
    }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
template <typename T, int KS>
__global__ __launch_bounds__(kDcThreads) void dense_conv3d_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                        float* __restrict__ part, int D, int H, int W, int cin,
                                                                        int cout, int64_t nvox, int64_t slab_vox, int xvec,
                                                                        int yvec) {
  typedef DwTile<T> TL;
  constexpr int E = TL::E, PAD = (KS - 1) / 2, KV = KS * KS * KS;
  __shared__ __attribute__((aligned(16))) char s_x[TL::BYTES];
  __shared__ __attribute__((aligned(16))) char s_y[TL::BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, half = lane >> 5, r = lane & 31;
  const int nco = (cout + kDwTile - 1) / kDwTile;
  const int ci0 = (blockIdx.y / nco) * kDwTile, co0 = (blockIdx.y % nco) * kDwTile;
  const int delta = blockIdx.z;
  const int dd = delta / (KS * KS) - PAD, dh = (delta / KS) % KS - PAD, dw = delta % KS - PAD;
  const int64_t dlin = ((int64_t)dd * H + dh) * W + dw;
  const int64_t v_begin = (int64_t)blockIdx.x * slab_vox;
  const int64_t v_end = v_begin + slab_vox < nvox ? v_begin + slab_vox : nvox;
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
        const int w = (int)(v % W);
        const int64_t q = v / W;
        const int h = (int)(q % H), d = (int)((q / H) % D);
        if ((unsigned)(d + dd) < (unsigned)D && (unsigned)(h + dh) < (unsigned)H && (unsigned)(w + dw) < (unsigned)W)
          px[i] = dc_load_piece<T, E>(x + (v + dlin) * cin, ci0 + piece * E, cin, xvec);
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
static bool dc_shape_ok(int cin, int cout, int ks, int dtype) {
  return dtype_ok(dtype) && (ks == 1 || ks == 3) && cin >= 1 && cout >= 1 && cin <= 8192 && cout <= 8192;  // (grid.y of dW)
}
static int dc_chunk(int dtype) { return kDcRowBytes / dtype_bytes(dtype); }   // input channels of a staged chunk

}  // namespace wcn

using namespace wcn;

int wcn_dense_conv3d_supported(int32_t cin, int32_t cout, int32_t ks, int32_t dtype) {
  return dc_shape_ok(cin, cout, ks, dtype) ? 1 : 0;
}

size_t wcn_dense_conv3d_packed_bytes(int32_t cin, int32_t cout, int32_t ks, int32_t dtype, int32_t dgrad) {
  if (!dc_shape_ok(cin, cout, ks, dtype)) return 0;
  const int k = dgrad ? cout : cin, n = dgrad ? cin : cout;
  return (size_t)ks * ks * ks * dc_round(k, dc_chunk(dtype)) * dc_round(n, 64 * dc_nb(n)) * dtype_bytes(dtype);
}

int wcn_dense_conv3d_pack(const void* w, int32_t cin, int32_t cout, int32_t ks, int32_t dtype, int32_t dgrad, void* packed,
                          size_t packed_bytes, wcn_stream_t stream) {
  if (cin < 1 || cout < 1) return WCN_ERROR_INVALID_PARAMETERS;
  if (!dc_shape_ok(cin, cout, ks, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (!w || !packed || !aligned_to(w, dtype_bytes(dtype)) || !aligned_to(packed, 16) ||
      packed_bytes < wcn_dense_conv3d_packed_bytes(cin, cout, ks, dtype, dgrad))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int k = dgrad ? cout : cin, n = dgrad ? cin : cout, kv = ks * ks * ks;
  const int kpad = dc_round(k, dc_chunk(dtype)), npad = dc_round(n, 64 * dc_nb(n));
  const int64_t total = (int64_t)kv * kpad * npad;
  const unsigned grid = (unsigned)(ceil_div(total, kDcThreads) < 4096 ? ceil_div(total, kDcThreads) : 4096);
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL(dense_conv3d_pack_kernel<T>, dim3(grid), dim3(kDcThreads), 0, (hipStream_t)stream, (const T*)w, (T*)packed,
                       cin, cout, kv, kpad, npad, dgrad ? 1 : 0);
    return 0;
  });
  return launch_status();
}

int wcn_dense_conv3d(const void* x, const void* packed, const void* bias, const void* residual, void* y, int64_t batch,
                     int32_t D, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks, int32_t pixel_shuffle,
                     int32_t dtype, wcn_stream_t stream) {
  if (batch < 0 || D < 0 || H < 0 || W < 0 || cin < 1 || cout < 1 || (pixel_shuffle != 1 && pixel_shuffle != 2))
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!dc_shape_ok(cin, cout, ks, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  if (pixel_shuffle == 2 && cout % 8 != 0) return WCN_ERROR_INVALID_PARAMETERS;
  if (batch == 0 || D == 0 || H == 0 || W == 0) return WCN_SUCCESS;  // no voxels, no launch
  const size_t el = dtype_bytes(dtype);
  if (!x || !packed || !y || y == residual || !aligned_to(x, el) || !aligned_to(y, el) || !aligned_to(bias, el) ||
      !aligned_to(residual, el) || !aligned_to(packed, 16))
    return WCN_ERROR_INVALID_PARAMETERS;
  const int64_t tiles = batch * ceil_div(D, kDcTD) * ceil_div(H, kDcTH) * ceil_div(W, kDcTW);
  if (tiles > INT32_MAX) return WCN_ERROR_INVALID_PARAMETERS;
  const int nb = dc_nb(cout), kpad = dc_round(cin, dc_chunk(dtype)), npad = dc_round(cout, 64 * nb);
  const dim3 grid((unsigned)tiles, (unsigned)(npad / (64 * nb)));
  const int ps = pixel_shuffle == 2;
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = cin % DcOp<T>::E == 0 && aligned_to(x, 16);
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(kDcThreads), 0, (hipStream_t)stream, (const T*)x, (const T*)packed, (const T*)bias,
                         (const T*)residual, (T*)y, D, H, W, cin, cout, kpad, npad, ps, xvec);
    };
    if (ks == 3) { if (nb == 2) go(dense_conv3d_kernel<T, 3, 2>); else go(dense_conv3d_kernel<T, 3, 1>); }
    else { if (nb == 2) go(dense_conv3d_kernel<T, 1, 2>); else go(dense_conv3d_kernel<T, 1, 1>); }
    return 0;
  });
  return launch_status();
}

int32_t wcn_dense_conv3d_wgrad_slabs(int64_t voxels, int32_t cin, int32_t cout, int32_t ks, int32_t dtype) {
  if (voxels <= 0 || !dc_shape_ok(cin, cout, ks, dtype)) return 0;
  return dw_slabs(voxels, cin, cout, ks * ks * ks, dtype);
}

size_t wcn_dense_conv3d_wgrad_workspace(int32_t cin, int32_t cout, int32_t ks, int32_t slabs) {
  if (cin < 1 || cout < 1 || slabs < 1 || (ks != 1 && ks != 3)) return 0;
  return align256((size_t)slabs * ks * ks * ks * cin * cout * sizeof(float)) + (size_t)kDwBiasParts * cout * sizeof(float);
}

int wcn_dense_conv3d_wgrad(const void* x, const void* dy, int64_t batch, int32_t D, int32_t H, int32_t W, int32_t cin,
                           int32_t cout, int32_t ks, int32_t dtype, int32_t slabs, void* dw, void* dbias, void* workspace,
                           size_t workspace_bytes, wcn_stream_t stream) {
  if (batch < 0 || D < 0 || H < 0 || W < 0 || cin < 1 || cout < 1 || slabs < 0 || slabs > kDwMaxSlabs)
    return WCN_ERROR_INVALID_PARAMETERS;
  if (!dc_shape_ok(cin, cout, ks, dtype)) return WCN_ERROR_UNSUPPORTED_CONFIG;
  const int64_t nvox = batch * D * H * W;
  if (nvox == 0) return WCN_SUCCESS;  // no voxels, no launch: the caller's zeros stand
  if (slabs == 0) slabs = wcn_dense_conv3d_wgrad_slabs(nvox, cin, cout, ks, dtype);
  const size_t el = dtype_bytes(dtype);
  if (!x || !dy || !dw || !workspace || !aligned_to(x, el) || !aligned_to(dy, el) || !aligned_to(dw, el) ||
      !aligned_to(dbias, el) || !aligned_to(workspace, 256) ||
      workspace_bytes < wcn_dense_conv3d_wgrad_workspace(cin, cout, ks, slabs))
    return WCN_ERROR_INVALID_PARAMETERS;
  int64_t slab_vox;
  int used;
  dw_plan(nvox, slabs, dtype, &slab_vox, &used);
  const int kv = ks * ks * ks;
  float* part = (float*)workspace;
  float* bpart = (float*)((char*)workspace + align256((size_t)slabs * kv * cin * cout * sizeof(float)));
  const dim3 grid((unsigned)used, (unsigned)(ceil_div(cin, kDwTile) * ceil_div(cout, kDwTile)), (unsigned)kv);
  hipStream_t s = (hipStream_t)stream;
  with_dtype(dtype, [&](auto t) {
    typedef decltype(t) T;
    const int xvec = cin % DcOp<T>::E == 0 && aligned_to(x, 16), yvec = cout % DcOp<T>::E == 0 && aligned_to(dy, 16);
    if (ks == 3)
      hipLaunchKernelGGL((dense_conv3d_wgrad_kernel<T, 3>), grid, dim3(kDcThreads), 0, s, (const T*)x, (const T*)dy, part, D, H, W,
                         cin, cout, nvox, slab_vox, xvec, yvec);
    else
      hipLaunchKernelGGL((dense_conv3d_wgrad_kernel<T, 1>), grid, dim3(kDcThreads), 0, s, (const T*)x, (const T*)dy, part, D, H, W,
                         cin, cout, nvox, slab_vox, xvec, yvec);
    if (dbias)
      hipLaunchKernelGGL(dense_conv_dbias_kernel<T>, dim3(kDwBiasParts), dim3(kDcThreads), 0, s, (const T*)dy, bpart, nvox, cout);
    const int64_t total = (int64_t)kv * cin * cout + cout;
    const unsigned rgrid = (unsigned)(ceil_div(total, kDcThreads) < 8192 ? ceil_div(total, kDcThreads) : 8192);
    hipLaunchKernelGGL(dense_conv_wgrad_reduce_kernel<T>, dim3(rgrid), dim3(kDcThreads), 0, s, (const float*)part,
                       (const float*)bpart, used, kv, cin, cout, cout, (T*)dw, (T*)dbias);
    return 0;
  });
  return launch_status();
}
