// Inception-v3 forward (the network between tg_inception_preprocess and the FID / Inception-score math) on gfx950.
//
// One 299 x 299 image is 5.71 GMAC, all but 2 MMAC of it in 94 convolutions, each followed by an eval-mode BatchNorm and a
// ReLU.  The BatchNorm is folded into the filter and a per-channel bias by the host, so a layer is ONE launch of
// inc_conv_kernel: an NCHW fp32 implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 operands and accumulation),
//     M = Cout,  N = B * OH * OW (flattened across the batch, so the 17 x 17 and 8 x 8 planes still fill tiles),
//     K = Cin * KH * KW  in the filter's own (ci, kh, kw) order.
// Tiling: 256 threads = 2 x 2 waves, K in steps of 16, two LDS buffers, one barrier per step:
//     gather(step 0) -> LDS;  for s: { global loads of step s + 1 into registers;  MFMAs on step s;  registers -> other
//     LDS buffer;  barrier }
//   * 128 x 128 tiles (a wave owns 64 x 64 = 2 x 2 MFMA tiles, 64 accumulator registers, 32 KB of LDS) where they give
//     every CU a workgroup, 64 x 64 tiles (one MFMA tile per wave, 16 KB) for the small-plane layers otherwise;
//   * the filter arrives packed by the host as wp[Kp][CoutP] (K-major, Kp = K rounded up to 16, CoutP = Cout rounded up
//     to 128, zero filled): a K step of the A panel is float4 loads with no bounds test, stored as the [k][m] LDS image
//     the MFMA A operand reads conflict-free;
//   * the B panel is the im2col gather, global -> registers -> LDS: a thread keeps ONE output pixel (its (b, oh, ow)
//     split is done once) and walks k; which k rows a wave loads is wave-uniform, so the (ci, kh, kw) split of k is
//     scalar arithmetic.  Lanes of a wave read consecutive ow: coalesced for stride 1.  Stride 2, 1 x 7 / 7 x 1 and the
//     per-axis zero padding are just that address arithmetic plus a bounds test;
//   * channel-slice addressing on both sides: the input is channels [x_coff, x_coff + Cin) of a tensor with x_ctot
//     channels, the output channels [y_coff, y_coff + Cout) of one with y_ctot.  A Mixed block's branches write straight
//     into the block's concatenated output (no torch.cat pass), and 1 x 1 branches that share an input run as one stacked
//     launch whose result is read back by slices.
//   * summation: the MFMA is a k-ordered fp32 fma chain, whose rounding error grows with its length (K reaches 4032); after
//     every IC_KC = 256 values of k the chain is closed and added to a second accumulator, so the error is that of a
//     256-long chain plus K / 256 additions -- what blocked fp32 summation (ATen on a CPU) gives.
// No atomics and no K split across workgroups: every output element is summed by one wave in a fixed order, so results are
// bit-identical from run to run.  The pools (3 x 3 stride 2 max, 3 x 3 stride 1 pad 1 average with count_include_pad) are
// bandwidth-bound one-thread-per-output kernels with the same slice addressing.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int IC_T = 256, IC_BK = 16, IC_MPAD = 128, IC_KC = 256;

struct IcShape {
  int B, Cin, Cout, H, W, KH, KW, stride, ph, pw, OH, OW, relu;
  int x_ctot, x_coff, y_ctot, y_coff;
  int K, CoutP, N;       // Cin * KH * KW; padded row length of wp; B * OH * OW
};

template <int BM, int BN>
__global__ void __launch_bounds__(IC_T)
inc_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y,
                const IcShape s) {
  constexpr int WM = BM / 2, WN = BN / 2, MT = WM / 32, NT = WN / 32;
  constexpr int ACH = IC_BK * BM / 4, NVA = ACH / IC_T;           // float4 chunks of an A step; per thread
  constexpr int KR = IC_T / BN, NVB = IC_BK / KR;                 // k rows the block gathers per pass; passes
  static_assert(ACH % IC_T == 0 && IC_BK % KR == 0 && BN % 64 == 0, "whole passes, wave-uniform k rows");
  __shared__ __attribute__((aligned(16))) float As[2][IC_BK * BM];
  __shared__ __attribute__((aligned(16))) float Bs[2][IC_BK * BN];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_m = (s.Cout + BM - 1) / BM;
  const int m0 = (blockIdx.x % tiles_m) * BM, n0 = (blockIdx.x / tiles_m) * BN;   // m fastest: neighbours share the gather in L2
  const int HW = s.H * s.W, OHW = s.OH * s.OW, taps = s.KH * s.KW;

  // the pixel this thread gathers for
  const int col = tid % BN, krow0 = wave / (BN / 64);
  const float* xb = x;
  int ih0 = -(1 << 20), iw0 = 0;                                  // n >= N: every bounds test fails
  {
    const int n = n0 + col;
    if (n < s.N) {
      const int b = n / OHW, p = n - b * OHW, oh = p / s.OW, ow = p - oh * s.OW;
      ih0 = oh * s.stride - s.ph;
      iw0 = ow * s.stride - s.pw;
      xb = x + ((int64_t)b * s.x_ctot + s.x_coff) * HW;
    }
  }
  const float* wa = wp + m0;

  f32x4 ra[NVA];
  float rb[NVB];
  auto load = [&](int k0) {
#pragma unroll
    for (int v = 0; v < NVA; ++v) {
      const int e = v * IC_T + tid, row = e / (BM / 4), q = e % (BM / 4);
      ra[v] = *reinterpret_cast<const f32x4*>(wa + (int64_t)(k0 + row) * s.CoutP + 4 * q);
    }
#pragma unroll
    for (int v = 0; v < NVB; ++v) {
      const int k = k0 + krow0 + v * KR;                          // wave-uniform
      const int ci = k / taps, t = k - ci * taps, kh = t / s.KW, kw = t - kh * s.KW;
      const int ih = ih0 + kh, iw = iw0 + kw;
      const bool ok = (ci < s.Cin) && ((unsigned)ih < (unsigned)s.H) && ((unsigned)iw < (unsigned)s.W);
      rb[v] = ok ? xb[(int64_t)ci * HW + ih * s.W + iw] : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < NVA; ++v) *reinterpret_cast<f32x4*>(&As[buf][(v * IC_T + tid) * 4]) = ra[v];
#pragma unroll
    for (int v = 0; v < NVB; ++v) Bs[buf][(krow0 + v * KR) * BN + col] = rb[v];
  };

  f32x16 acc[MT][NT], tot[MT][NT];                               // the running chain; the closed chains
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[a][b][r] = 0.f; tot[a][b][r] = 0.f; }

  const int la = h * BM + wm * WM + i, lb = h * BN + wn * WN + i;
  load(0);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < s.K; k0 += IC_BK) {
    const bool more = k0 + IC_BK < s.K;
    if (more) load(k0 + IC_BK);
    const float* al = As[buf];
    const float* bl = Bs[buf];
#pragma unroll
    for (int kk = 0; kk < IC_BK / 2; ++kk) {
      float a[MT], b[NT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = al[la + (2 * kk) * BM + t * 32];
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t] = bl[lb + (2 * kk) * BN + t * 32];
#pragma unroll
      for (int u = 0; u < MT; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[u][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[t], acc[u][t], 0, 0, 0);
    }
    if (((k0 + IC_BK) % IC_KC == 0) || !more) {
#pragma unroll
      for (int u = 0; u < MT; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) { tot[u][t][r] += acc[u][t][r]; acc[u][t][r] = 0.f; }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  // D[row][col]: lane (col = i, h), register r -> row (r & 3) + 8 (r >> 2) + 4 h
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + wn * WN + t * 32 + i;
    if (n >= s.N) continue;
    const int b = n / OHW, p = n - b * OHW;
    float* yb = y + ((int64_t)b * s.y_ctot + s.y_coff) * OHW + p;
#pragma unroll
    for (int u = 0; u < MT; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WM + u * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < s.Cout) {
          float v = tot[u][t][r] + (bias ? bias[m] : 0.f);
          if (s.relu) v = fmaxf(v, 0.f);
          yb[(int64_t)m * OHW] = v;
        }
      }
  }
}

// F.max_pool2d(x, 3, stride=2): every window lies inside the plane
__global__ void __launch_bounds__(256)
inc_maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total, int C, int H, int W, int OH, int OW,
                      int x_ctot, int x_coff, int y_ctot, int y_coff) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += stride) {
    const int ow = (int)(e % OW), oh = (int)((e / OW) % OH), c = (int)((e / ((int64_t)OW * OH)) % C);
    const int64_t b = e / ((int64_t)OW * OH * C);
    const float* p = x + ((b * x_ctot + x_coff + c) * H + 2 * oh) * (int64_t)W + 2 * ow;
    float m = p[0];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const float q = p[u * W + v];
        m = (q > m || q != q) ? q : m;                            // NaN propagates, like ATen's max_pool2d
      }
    y[((b * y_ctot + y_coff + c) * OH + oh) * (int64_t)OW + ow] = m;
  }
}

// F.avg_pool2d(x, 3, stride=1, padding=1) with count_include_pad: the sum of the taps inside the plane, over 9 everywhere
__global__ void __launch_bounds__(256)
inc_avgpool3_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total, int C, int H, int W, int x_ctot, int x_coff,
                    int y_ctot, int y_coff) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += stride) {
    const int w = (int)(e % W), hh = (int)((e / W) % H), c = (int)((e / ((int64_t)W * H)) % C);
    const int64_t b = e / ((int64_t)W * H * C);
    const float* p = x + (b * x_ctot + x_coff + c) * (int64_t)H * W;
    float sum = 0.f;
#pragma unroll
    for (int u = -1; u <= 1; ++u)
#pragma unroll
      for (int v = -1; v <= 1; ++v) {
        const int ih = hh + u, iw = w + v;
        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) sum += p[ih * W + iw];
      }
    y[((b * y_ctot + y_coff + c) * H + hh) * (int64_t)W + w] = sum / 9.f;
  }
}

bool slices_ok(int C, int x_ctot, int x_coff, int y_ctot, int y_coff, int Cy) {
  return x_coff >= 0 && y_coff >= 0 && (int64_t)x_coff + C <= x_ctot && (int64_t)y_coff + Cy <= y_ctot;
}

}  // namespace

extern "C" {

size_t tg_inception_conv_weight_floats(int Cin, int Cout, int KH, int KW) {
  if (Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0) return 0;
  const int64_t K = (int64_t)Cin * KH * KW;
  const int64_t Kp = (K + IC_BK - 1) / IC_BK * IC_BK, CoutP = ((int64_t)Cout + IC_MPAD - 1) / IC_MPAD * IC_MPAD;
  return (size_t)(Kp * CoutP);
}

int tg_inception_conv_supported(int B, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int ph, int pw, int x_ctot,
                                int y_ctot) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || ph < 0 || pw < 0) return 0;
  if (stride != 1 && stride != 2) return 0;
  if (KH > 64 || KW > 64 || ph >= (1 << 16) || pw >= (1 << 16)) return 0;
  if (H + 2 * ph < KH || W + 2 * pw < KW) return 0;
  const int64_t OH = (H + 2 * ph - KH) / stride + 1, OW = (W + 2 * pw - KW) / stride + 1;
  // 32-bit index arithmetic inside the kernel: pixels, one image of either tensor, the reduction length
  if ((int64_t)B * OH * OW >= (1ll << 30) || (int64_t)Cin * KH * KW >= (1ll << 30)) return 0;
  if ((int64_t)H * W >= (1ll << 30) || x_ctot < Cin || y_ctot < Cout) return 0;
  if ((((int64_t)Cout + 63) / 64) * (((int64_t)B * OH * OW + 63) / 64) >= (1ll << 31) - 1) return 0;   // gridDim.x of the small tiles
  return 1;
}

int tg_inception_conv_fwd(const float* x, const float* wp, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                          int KH, int KW, int stride, int ph, int pw, int relu, int x_ctot, int x_coff, int y_ctot, int y_coff,
                          void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(wp); TG_CHECK_PTR(y);
  TG_CHECK_POS(B); TG_CHECK_POS(Cin); TG_CHECK_POS(Cout); TG_CHECK_POS(H); TG_CHECK_POS(W); TG_CHECK_POS(KH); TG_CHECK_POS(KW);
  if (ph < 0 || pw < 0 || !slices_ok(Cin, x_ctot, x_coff, y_ctot, y_coff, Cout)) return TG_EINVAL;
  if (!tg_inception_conv_supported(B, Cin, Cout, H, W, KH, KW, stride, ph, pw, x_ctot, y_ctot) || !tg_aligned16(wp)) return TG_EUNSUPPORTED;
  IcShape s;
  s.B = B; s.Cin = Cin; s.Cout = Cout; s.H = H; s.W = W; s.KH = KH; s.KW = KW; s.stride = stride; s.ph = ph; s.pw = pw;
  s.OH = (H + 2 * ph - KH) / stride + 1;
  s.OW = (W + 2 * pw - KW) / stride + 1;
  s.relu = relu;
  s.x_ctot = x_ctot; s.x_coff = x_coff; s.y_ctot = y_ctot; s.y_coff = y_coff;
  s.K = Cin * KH * KW;
  s.CoutP = (Cout + IC_MPAD - 1) / IC_MPAD * IC_MPAD;
  s.N = B * s.OH * s.OW;
  hipStream_t st = tg_stream(stream);
  const int64_t big = (int64_t)((Cout + 127) / 128) * ((s.N + 127) / 128);
  if (big >= 256) {
    inc_conv_kernel<128, 128><<<(int)big, IC_T, 0, st>>>(x, wp, bias, y, s);
  } else {
    const int tiles = ((Cout + 63) / 64) * ((s.N + 63) / 64);
    inc_conv_kernel<64, 64><<<tiles, IC_T, 0, st>>>(x, wp, bias, y, s);
  }
  return tg_launch_status();
}

int tg_inception_maxpool3s2(const float* x, float* y, int B, int C, int H, int W, int x_ctot, int x_coff, int y_ctot, int y_coff,
                            void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(y); TG_CHECK_POS(B); TG_CHECK_POS(C);
  if (H < 3 || W < 3 || !slices_ok(C, x_ctot, x_coff, y_ctot, y_coff, C)) return TG_EINVAL;
  const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  const int64_t total = (int64_t)B * C * OH * OW;
  inc_maxpool3s2_kernel<<<tg_ew_grid(total, 256), 256, 0, tg_stream(stream)>>>(x, y, total, C, H, W, OH, OW, x_ctot, x_coff, y_ctot, y_coff);
  return tg_launch_status();
}

int tg_inception_avgpool3(const float* x, float* y, int B, int C, int H, int W, int x_ctot, int x_coff, int y_ctot, int y_coff,
                          void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(y); TG_CHECK_POS(B); TG_CHECK_POS(C); TG_CHECK_POS(H); TG_CHECK_POS(W);
  if (!slices_ok(C, x_ctot, x_coff, y_ctot, y_coff, C)) return TG_EINVAL;
  const int64_t total = (int64_t)B * C * H * W;
  inc_avgpool3_kernel<<<tg_ew_grid(total, 256), 256, 0, tg_stream(stream)>>>(x, y, total, C, H, W, x_ctot, x_coff, y_ctot, y_coff);
  return tg_launch_status();
}

}  // extern "C"
