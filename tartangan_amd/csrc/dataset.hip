// Building the training archive on the device (tartangan_amd/image_folder_dataset.py): Pillow's two-pass separable resampler for
// 8-bit interleaved images (Resample.c, the 8bpc path) with the fixed-point taps computed on the host.  Per output sample
//   acc = 2^21 + sum_j pixel[first + j] * k[j]        (32-bit, unsigned wrap-around)
//   out = clip((int32)acc >> 22, 0, 255)
// Integer sums do not depend on their order, so the result is bit-identical to Pillow's whatever the decomposition.  Horizontal
// first into a uint8 intermediate (clipped, as Pillow does), then vertical.  No atomics, 64-bit addressing throughout.
//
// Horizontal: a workgroup takes 64 output columns of up to 4 image rows.  Neighbouring outputs share most of their taps (all but
// `scale` of `6 scale` pixels), so the rows' input span -- the columns the tile's bounds reach, halo included -- is staged in LDS
// once (dword loads where the row's address allows, bytes at its ragged ends) and every tap is an LDS byte read.  Lanes are
// adjacent outputs: their windows start `scale * C` bytes apart, an odd dword stride for the common integer ratios with C = 3,
// and overlapping windows (up-scaling) are broadcasts.  Vertical: a thread owns 4 consecutive bytes of an output row (one dword
// load per tap row when rows are dword-aligned, else one byte), coalesced along the row; the taps are wave-uniform.
#include <vector>

#include "common.h"

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_TX = 64;                  // output columns per workgroup: one wave per staged row
constexpr int RS_MAX_ROWS = RS_BLOCK / RS_TX;
constexpr int RS_LDS_MAX = 64 * 1024;      // dynamic LDS a launch may ask for without opting in to more

__device__ __forceinline__ uint8_t clip8(uint32_t acc) {
  const int32_t v = (int32_t)acc >> 22;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// rows = N * H image rows of W pixels -> rows of OW pixels.  stride: LDS bytes per staged row (a multiple of 4, >= span * C + 3).
template <int C>
__global__ void __launch_bounds__(RS_BLOCK) resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int32_t* __restrict__ kx, const int32_t* __restrict__ bx,
                                                              int64_t rows, int W, int OW, int ks, int tile_rows, int stride) {
  extern __shared__ __align__(16) uint8_t staged[];
  const int ox0 = blockIdx.x * RS_TX;
  const int nox = min(RS_TX, OW - ox0);
  int lo = bx[2 * ox0], hi = lo + bx[2 * ox0 + 1];
  for (int i = 1; i < nox; ++i) {           // the same addresses in every thread: uniform loads
    const int a = bx[2 * (ox0 + i)], b = a + bx[2 * (ox0 + i) + 1];
    lo = min(lo, a);
    hi = max(hi, b);
  }
  const int nbytes = (hi - lo) * C;
  const int col = threadIdx.x % RS_TX, rr = threadIdx.x / RS_TX;
  for (int64_t r0 = (int64_t)blockIdx.y * tile_rows; r0 < rows; r0 += (int64_t)gridDim.y * tile_rows) {
    const int nr = (int)min((int64_t)tile_rows, rows - r0);
    __syncthreads();                         // the previous group's reads are done
    for (int r = 0; r < nr; ++r) {
      const uint8_t* g = src + ((r0 + r) * W + lo) * C;
      const int pad = (int)((uintptr_t)g & 3);                      // LDS keeps the row's alignment: dwords map onto dwords
      uint8_t* l = staged + r * stride + pad;
      const int head = min((4 - pad) & 3, nbytes);
      const int nw = (nbytes - head) >> 2;
      for (int i = threadIdx.x; i < head; i += RS_BLOCK) l[i] = g[i];
      for (int i = threadIdx.x; i < nw; i += RS_BLOCK)
        *reinterpret_cast<uint32_t*>(l + head + 4 * i) = *reinterpret_cast<const uint32_t*>(g + head + 4 * i);
      for (int i = head + 4 * nw + threadIdx.x; i < nbytes; i += RS_BLOCK) l[i] = g[i];
    }
    __syncthreads();
    if (col < nox && rr < nr) {
      const int ox = ox0 + col;
      const int first = bx[2 * ox], count = bx[2 * ox + 1];
      const int32_t* k = kx + (int64_t)ox * ks;
      const int pad = (int)((uintptr_t)(src + ((r0 + rr) * W + lo) * C) & 3);
      const uint8_t* l = staged + rr * stride + pad + (first - lo) * C;
      uint32_t acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 1u << 21;
      for (int j = 0; j < count; ++j) {
        const uint32_t kj = (uint32_t)k[j];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (uint32_t)l[j * C + c] * kj;
      }
      uint8_t* o = dst + ((r0 + rr) * OW + ox) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = clip8(acc[c]);
    }
  }
}

// (N, H, RB) bytes -> (N, OH, RB) bytes, RB = row bytes (pixels * C).  V = 4: every row of src and dst starts dword-aligned and RB % 4 == 0.
template <int V>
__global__ void __launch_bounds__(RS_BLOCK) resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                              const int32_t* __restrict__ ky, const int32_t* __restrict__ by, int N,
                                                              int H, int OH, int64_t RB, int ks) {
  for (int n = blockIdx.z; n < N; n += gridDim.z) {
    for (int oy = blockIdx.y; oy < OH; oy += gridDim.y) {
      const int first = by[2 * oy], count = by[2 * oy + 1];
      const int32_t* k = ky + (int64_t)oy * ks;
      const uint8_t* in = src + ((int64_t)n * H + first) * RB;
      uint8_t* out = dst + ((int64_t)n * OH + oy) * RB;
      for (int64_t b = ((int64_t)blockIdx.x * RS_BLOCK + threadIdx.x) * V; b < RB; b += (int64_t)gridDim.x * RS_BLOCK * V) {
        uint32_t acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 1u << 21;
        for (int j = 0; j < count; ++j) {
          const uint32_t kj = (uint32_t)k[j];
          if (V == 4) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(in + j * RB + b);
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] += ((w >> (8 * i)) & 255u) * kj;
          } else {
            acc[0] += (uint32_t)in[j * RB + b] * kj;
          }
        }
        if (V == 4) {
          *reinterpret_cast<uint32_t*>(out + b) = (uint32_t)clip8(acc[0]) | ((uint32_t)clip8(acc[V > 1 ? 1 : 0]) << 8) |
                                                  ((uint32_t)clip8(acc[V > 2 ? 2 : 0]) << 16) | ((uint32_t)clip8(acc[V > 3 ? 3 : 0]) << 24);
        } else {
          out[b] = clip8(acc[0]);
        }
      }
    }
  }
}

// The bounds live on the device and decide what the kernels read: they are fetched and checked before anything is launched.
// -> TG_OK / TG_EINVAL / a HIP error; *span = the widest input span of one 64-output tile (horizontal staging).
static int check_bounds(const int32_t* bounds_dev, int n_out, int n_in, int ks, hipStream_t st, int* span) {
  std::vector<int32_t> b((size_t)n_out * 2);
  hipError_t e = hipMemcpyAsync(b.data(), bounds_dev, b.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  int widest = 0;
  for (int t0 = 0; t0 < n_out; t0 += RS_TX) {
    int lo = n_in, hi = 0;
    for (int i = t0; i < n_out && i < t0 + RS_TX; ++i) {
      const int64_t first = b[2 * (size_t)i], count = b[2 * (size_t)i + 1];
      if (first < 0 || count < 0 || count > ks || first + count > n_in) return TG_EINVAL;
      lo = first < lo ? (int)first : lo;
      hi = first + count > hi ? (int)(first + count) : hi;
    }
    widest = hi - lo > widest ? hi - lo : widest;
  }
  *span = widest;
  return TG_OK;
}

}  // namespace

extern "C" int tg_resample_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp, const int32_t* kx, const int32_t* bx, const int32_t* ky,
                              const int32_t* by, int N, int H, int W, int C, int OH, int OW, int ksx, int ksy, void* stream) {
  TG_CHECK_PTR(src); TG_CHECK_PTR(dst);
  TG_CHECK_POS(N); TG_CHECK_POS(H); TG_CHECK_POS(W); TG_CHECK_POS(OH); TG_CHECK_POS(OW);
  if (C != 1 && C != 3) return TG_EUNSUPPORTED;
  if (kx == nullptr && ky == nullptr) return TG_EINVAL;             // nothing to do: the caller copies
  if (kx ? (bx == nullptr || ksx <= 0) : (W != OW)) return TG_EINVAL;
  if (ky ? (by == nullptr || ksy <= 0) : (H != OH)) return TG_EINVAL;
  if (kx && ky && tmp == nullptr) return TG_EINVAL;
  hipStream_t st = tg_stream(stream);
  int span = 0, unused = 0, rc;
  if (kx && (rc = check_bounds(bx, OW, W, ksx, st, &span)) != TG_OK) return rc;
  if (ky && (rc = check_bounds(by, OH, H, ksy, st, &unused)) != TG_OK) return rc;
  if (kx) {
    const int64_t stride64 = ((int64_t)span * C + 3 + 3) / 4 * 4;
    if (stride64 > RS_LDS_MAX) return TG_EUNSUPPORTED;              // one row's tile span does not fit: the caller resizes on the host
    const int stride = (int)stride64;
    int tile_rows = RS_MAX_ROWS;
    while (tile_rows > 1 && tile_rows * stride > RS_LDS_MAX) tile_rows >>= 1;
    const int64_t rows = (int64_t)N * H, groups = (rows + tile_rows - 1) / tile_rows;
    const dim3 grid((unsigned)tg_div_up(OW, RS_TX), (unsigned)(groups > 65535 ? 65535 : groups));
    uint8_t* out = ky ? tmp : dst;
    const size_t lds = (size_t)tile_rows * stride;
    if (C == 3) resample_h_kernel<3><<<grid, RS_BLOCK, lds, st>>>(src, out, kx, bx, rows, W, OW, ksx, tile_rows, stride);
    else resample_h_kernel<1><<<grid, RS_BLOCK, lds, st>>>(src, out, kx, bx, rows, W, OW, ksx, tile_rows, stride);
    if ((rc = tg_launch_status()) != TG_OK) return rc;
  }
  if (ky) {
    const uint8_t* in = kx ? tmp : src;
    const int64_t RB = (int64_t)OW * C;
    const bool vec = RB % 4 == 0 && (((uintptr_t)in | (uintptr_t)dst) & 3) == 0;
    const int64_t per_block = (int64_t)RS_BLOCK * (vec ? 4 : 1);
    const dim3 grid((unsigned)((RB + per_block - 1) / per_block), (unsigned)(OH > 65535 ? 65535 : OH), (unsigned)(N > 65535 ? 65535 : N));
    if (vec) resample_v_kernel<4><<<grid, RS_BLOCK, 0, st>>>(in, dst, ky, by, N, H, OH, RB, ksy);
    else resample_v_kernel<1><<<grid, RS_BLOCK, 0, st>>>(in, dst, ky, by, N, H, OH, RB, ksy);
    if ((rc = tg_launch_status()) != TG_OK) return rc;
  }
  return TG_OK;
}
