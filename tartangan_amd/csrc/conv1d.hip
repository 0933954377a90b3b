// 1-D convolutions of the text trainer (nn.Conv1d, ks in {1, 3}, stride 1, zero padding ks / 2) and the 1-D resampling
// pair, on gfx950.
//
// G and D of trainers/text_cnn.py are the residual blocks of the image trainers with conv_factory = nn.Conv1d over
// (B, C, L), L = 4 .. 64 tokens.  A 2-D image tile has nothing to hold on to at H = 1, so the three passes are implicit
// GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32 operands, a k-ordered fp32 fma chain) whose long axis is the
// batch-flattened token axis:
//     forward   y  (Cout x B*L)    = w  (Cout x Cin*ks)  . im2col(x)  (Cin*ks x B*L)       k = (ci, tap)
//     dgrad     gx (Cin  x B*L)    = w' (Cin  x Cout*ks) . im2col(gy) (Cout*ks x B*L)      k = (co, flipped tap)
//     wgrad     gw (Cout x Cin*ks) = gy (Cout x B*L)     . im2col(x)^T (B*L x Cin*ks)      k = (b, l)
// A tile of 64 columns spans several sequences when L < 64: a column is split into (b, l) once, and a tap whose token
// l + tap - ks / 2 falls outside [0, L) of ITS OWN sequence contributes zero, never the neighbouring sequence's token.
// One kernel serves all three: 64 x 64 tiles, 256 threads = 2 x 2 waves of one 32 x 32 MFMA tile each, K in steps of 32
// through two LDS buffers with one barrier per step (global -> registers -> LDS, loads of step s + 1 issued before the
// MFMAs of step s).  Each operand is described by a small gather object; its lanes run along whichever index is
// contiguous in memory (the columns for activations in forward / dgrad, k for the filter in forward and for both
// operands in wgrad).  After every K step (32 values of k) the fma chain is closed into a second accumulator (16 adds per 16
// MFMAs), so the rounding error is that of blocked summation, as ATen's own convolution has it, not of one K-long chain.
// wgrad splits K = B*L over gridDim.y workgroups (a fixed function of the shape), each writing its partial
// (Cout x Cin*ks + 1) block into the workspace -- the extra column multiplies gy by one, which is the bias gradient --
// and a second launch adds the partials in split order: no atomics, bit-identical from run to run.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int C1_T = 256, C1_BK = 32, C1_NV = C1_BK / 4, C1_BM = 64, C1_BN = 64, C1_P = 68, C1_MAXSPLIT = 64;

// ---- gather objects: prep(column) once per thread and column, get(info, k) per element; out-of-range -> 0
struct ColInfo {
  const float* base;
  int pos;          // token position (activations) / tap shift (wgrad x)
  int flag;         // 0: out of range, 1: data, 2: the all-ones bias column of wgrad
};

// activations of forward / dgrad: column n = (b, l), k = (c, tap); reads act[b][c][l + tap - KS / 2]
template <int KS>
struct ActCols {
  const float* act; int C, L, N;
  __device__ ColInfo prep(int n) const {
    ColInfo ci; ci.base = act; ci.pos = 0; ci.flag = 0;
    if (n < N) { const int b = n / L; ci.pos = n - b * L; ci.base = act + (int64_t)b * C * L; ci.flag = 1; }
    return ci;
  }
  __device__ float get(const ColInfo& ci, int k) const {
    const int c = k / KS, t = k - c * KS, j = ci.pos + t - KS / 2;
    return (ci.flag && c < C && (unsigned)j < (unsigned)L) ? ci.base[c * L + j] : 0.f;
  }
};
// forward filter: row m = co, k = (ci, tap): w[co][k]
struct FilterRows {
  const float* w; int M, K;
  __device__ ColInfo prep(int m) const { ColInfo ci; ci.base = w + (int64_t)(m < M ? m : 0) * K; ci.pos = 0; ci.flag = m < M; return ci; }
  __device__ float get(const ColInfo& ci, int k) const { return (ci.flag && k < K) ? ci.base[k] : 0.f; }
};
// dgrad filter: row m = ci, k = (co, t'): w[co][ci][KS - 1 - t']
template <int KS>
struct FilterRowsT {
  const float* w; int Cin, Cout;
  __device__ ColInfo prep(int m) const { ColInfo ci; ci.base = w + (int64_t)(m < Cin ? m : 0) * KS; ci.pos = 0; ci.flag = m < Cin; return ci; }
  __device__ float get(const ColInfo& ci, int k) const {
    const int co = k / KS, t = k - co * KS;
    return (ci.flag && co < Cout) ? ci.base[(int64_t)co * Cin * KS + (KS - 1 - t)] : 0.f;
  }
};
// wgrad: rows m = co of gy, k = (b, l): gy[b][co][l]
struct GyRows {
  const float* gy; int Cout, L, Ktot;
  __device__ ColInfo prep(int m) const { ColInfo ci; ci.base = gy + (int64_t)(m < Cout ? m : 0) * L; ci.pos = 0; ci.flag = m < Cout; return ci; }
  __device__ float get(const ColInfo& ci, int k) const {
    if (!ci.flag || k >= Ktot) return 0.f;
    const int b = k / L, l = k - b * L;
    return ci.base[(int64_t)b * Cout * L + l];
  }
};
// wgrad: columns n = (ci, tap) of im2col(x)^T, plus the all-ones column n = Cin * KS; k = (b, l): x[b][ci][l + tap - KS / 2]
template <int KS>
struct XColsT {
  const float* x; int Cin, L, Ktot;
  __device__ ColInfo prep(int n) const {
    ColInfo ci; ci.base = x; ci.pos = 0; ci.flag = 0;
    if (n < Cin * KS) { const int c = n / KS; ci.pos = n - c * KS - KS / 2; ci.base = x + (int64_t)c * L; ci.flag = 1; }
    else if (n == Cin * KS) ci.flag = 2;
    return ci;
  }
  __device__ float get(const ColInfo& ci, int k) const {
    if (!ci.flag || k >= Ktot) return 0.f;
    if (ci.flag == 2) return 1.f;
    const int b = k / L, l = k - b * L, j = l + ci.pos;
    return ((unsigned)j < (unsigned)L) ? ci.base[(int64_t)b * Cin * L + j] : 0.f;
  }
};

// ---- epilogues: element (m, n) of the tile
struct ActOut {        // y[b][m][l] = v + bias[m] + residual[b][m][l]
  float* y; const float* bias; const float* residual; int M, L, N;
  __device__ void put(int m, int n, float v, int) const {
    if (m >= M || n >= N) return;
    const int b = n / L, l = n - b * L;
    const int64_t o = ((int64_t)b * M + m) * L + l;
    if (bias) v += bias[m];
    if (residual) v += residual[o];
    y[o] = v;
  }
};
struct PartialOut {    // ws[split][m][n]
  float* ws; int M, Ncols;
  __device__ void put(int m, int n, float v, int split) const {
    if (m < M && n < Ncols) ws[((int64_t)split * M + m) * Ncols + n] = v;
  }
};

// AK / BK: lanes of the loading pass run along k (true) or along the operand's rows / columns (false)
template <bool AK, bool BK, class AG, class BG, class OUT>
__global__ void __launch_bounds__(C1_T)
conv1d_gemm_kernel(const AG ag, const BG bg, const OUT out, int tiles_m, int K, int kchunk) {
  __shared__ float As[2][C1_BK * C1_P];
  __shared__ float Bs[2][C1_BK * C1_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int m0 = (blockIdx.x % tiles_m) * C1_BM, n0 = (blockIdx.x / tiles_m) * C1_BN;
  const int kbeg = blockIdx.y * kchunk, kend = min(K, kbeg + kchunk);

  // col-fast: one column, k rows tid / 64 + 4 v;  k-fast: k row tid % C1_BK, columns tid / C1_BK + (256 / C1_BK) v
  constexpr int CS = C1_T / C1_BK;                  // column stride of the k-fast pass
  ColInfo ia[C1_NV], ib[C1_NV];
  if (AK) {
#pragma unroll
    for (int v = 0; v < C1_NV; ++v) ia[v] = ag.prep(m0 + tid / C1_BK + CS * v);
  } else {
    ia[0] = ag.prep(m0 + (tid & 63));
  }
  if (BK) {
#pragma unroll
    for (int v = 0; v < C1_NV; ++v) ib[v] = bg.prep(n0 + tid / C1_BK + CS * v);
  } else {
    ib[0] = bg.prep(n0 + (tid & 63));
  }
  float ra[C1_NV], rb[C1_NV];
  auto load = [&](int k0) {
#pragma unroll
    for (int v = 0; v < C1_NV; ++v) {
      const int ka = AK ? k0 + tid % C1_BK : k0 + (tid >> 6) + 4 * v;
      ra[v] = ka < kend ? ag.get(ia[AK ? v : 0], ka) : 0.f;
      const int kb = BK ? k0 + tid % C1_BK : k0 + (tid >> 6) + 4 * v;
      rb[v] = kb < kend ? bg.get(ib[BK ? v : 0], kb) : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int v = 0; v < C1_NV; ++v) {
      if (AK) As[buf][(tid % C1_BK) * C1_P + tid / C1_BK + CS * v] = ra[v];
      else As[buf][((tid >> 6) + 4 * v) * C1_P + (tid & 63)] = ra[v];
      if (BK) Bs[buf][(tid % C1_BK) * C1_P + tid / C1_BK + CS * v] = rb[v];
      else Bs[buf][((tid >> 6) + 4 * v) * C1_P + (tid & 63)] = rb[v];
    }
  };

  f32x16 acc, tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.f; }
  const int la = h * C1_P + wm * 32 + i, lb = h * C1_P + wn * 32 + i;
  load(kbeg);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += C1_BK) {
    const bool more = k0 + C1_BK < kend;
    if (more) load(k0 + C1_BK);
    const float* al = As[buf];
    const float* bl = Bs[buf];
#pragma unroll
    for (int kk = 0; kk < C1_BK / 2; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[la + 2 * kk * C1_P], bl[lb + 2 * kk * C1_P], acc, 0, 0, 0);
    // close the fma chain of this step (32 values of k) into the running total
#pragma unroll
    for (int r = 0; r < 16; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // D[row][col]: lane (col = i, h), register r -> row (r & 3) + 8 (r >> 2) + 4 h
  const int n = n0 + wn * 32 + i;
#pragma unroll
  for (int r = 0; r < 16; ++r) out.put(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, n, tot[r], blockIdx.y);
}

// stage 2 of wgrad: gw[m][n] (+)= sum_s ws[s][m][n], gbias[m] (+)= sum_s ws[s][m][Cin*ks], in split order
__global__ void __launch_bounds__(256)
conv1d_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, float* __restrict__ gbias, int M, int Ncols,
                           int splits, int accumulate) {
  const int64_t total = (int64_t)M * Ncols, stride = (int64_t)gridDim.x * 256;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += stride) {
    const int m = (int)(e / Ncols), n = (int)(e - (int64_t)m * Ncols);
    float s = 0.f;
    for (int p = 0; p < splits; ++p) s += ws[(int64_t)p * total + e];
    if (n < Ncols - 1) {
      float* o = gw + (int64_t)m * (Ncols - 1) + n;
      *o = accumulate ? *o + s : s;
    } else if (gbias) {
      gbias[m] = accumulate ? gbias[m] + s : s;
    }
  }
}

__global__ void __launch_bounds__(256) up2x1d_kernel(const float* __restrict__ x, float* __restrict__ y, float alpha, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += stride) y[e] = alpha * x[e >> 1];
}

__global__ void __launch_bounds__(256)
pool2_1d_kernel(const float* __restrict__ x, const float* __restrict__ residual, float* __restrict__ y, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < total; e += stride) {
    const float p = 0.5f * (x[2 * e] + x[2 * e + 1]);
    y[e] = residual ? residual[e] + p : p;
  }
}

// the kernels index one sequence set with 32-bit integers: columns, one sample of either tensor, either reduction length
bool conv1d_shape_ok(int B, int Cin, int Cout, int L, int ks) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || L <= 0 || (ks != 1 && ks != 3)) return false;
  const int64_t lim = 1ll << 30;
  if ((int64_t)B * L >= lim || (int64_t)Cin * L >= lim || (int64_t)Cout * L >= lim) return false;
  if ((int64_t)Cin * ks + 1 >= lim || (int64_t)Cout * ks >= lim || (int64_t)Cout * Cin * ks >= lim) return false;
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  if (((cmax + 63) / 64) * (((int64_t)B * L + 63) / 64) >= (1ll << 31) - 1) return false;                       // gridDim.x, forward / dgrad
  if ((((int64_t)Cout + 63) / 64) * (((int64_t)Cin * ks + 1 + 63) / 64) >= (1ll << 31) - 1) return false;     // gridDim.x, wgrad
  return true;
}

// K = B * L in `splits` chunks of whole K steps (C1_BK): about 512 workgroups over the output tiles (two per CU), at most C1_MAXSPLIT
void wgrad_split(int B, int Cin, int Cout, int L, int ks, int* splits, int* kchunk) {
  const int64_t tiles = (int64_t)((Cout + 63) / 64) * ((Cin * ks + 1 + 63) / 64);
  const int64_t steps = ((int64_t)B * L + C1_BK - 1) / C1_BK;
  int64_t s = (512 + tiles - 1) / tiles;
  if (s > C1_MAXSPLIT) s = C1_MAXSPLIT;
  if (s > steps) s = steps;
  if (s < 1) s = 1;
  const int64_t per = (steps + s - 1) / s;
  *splits = (int)((steps + per - 1) / per);
  *kchunk = (int)(per * C1_BK);
}

template <int KS>
int launch_act(const float* act, const float* w, const float* bias, const float* residual, float* out, int B, int Cact, int Cres,
               int L, bool transposed, hipStream_t st) {
  const int N = B * L, tiles_m = (Cres + 63) / 64, tiles_n = (N + 63) / 64, K = Cact * KS;
  const ActCols<KS> bg{act, Cact, L, N};
  const ActOut o{out, bias, residual, Cres, L, N};
  const dim3 grid(tiles_m * tiles_n, 1);
  if (!transposed) {
    const FilterRows ag{w, Cres, K};
    conv1d_gemm_kernel<true, false><<<grid, C1_T, 0, st>>>(ag, bg, o, tiles_m, K, K);
  } else {
    const FilterRowsT<KS> ag{w, Cres, Cact};
    conv1d_gemm_kernel<false, false><<<grid, C1_T, 0, st>>>(ag, bg, o, tiles_m, K, K);
  }
  return tg_launch_status();
}

template <int KS>
int launch_wgrad(const float* x, const float* gy, float* ws, int B, int Cin, int Cout, int L, int splits, int kchunk, hipStream_t st) {
  const int Ktot = B * L, Ncols = Cin * KS + 1, tiles_m = (Cout + 63) / 64, tiles_n = (Ncols + 63) / 64;
  const GyRows ag{gy, Cout, L, Ktot};
  const XColsT<KS> bg{x, Cin, L, Ktot};
  const PartialOut o{ws, Cout, Ncols};
  conv1d_gemm_kernel<true, true><<<dim3(tiles_m * tiles_n, splits), C1_T, 0, st>>>(ag, bg, o, tiles_m, Ktot, kchunk);
  return tg_launch_status();
}

}  // namespace

extern "C" {

int tg_conv1d_supported(int B, int Cin, int Cout, int L, int ks) { return conv1d_shape_ok(B, Cin, Cout, L, ks) ? 1 : 0; }

int tg_conv1d_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int Cin, int Cout, int L,
                  int ks, void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(w); TG_CHECK_PTR(y);
  TG_CHECK_POS(B); TG_CHECK_POS(Cin); TG_CHECK_POS(Cout); TG_CHECK_POS(L); TG_CHECK_POS(ks);
  if (!conv1d_shape_ok(B, Cin, Cout, L, ks)) return TG_EUNSUPPORTED;
  return ks == 3 ? launch_act<3>(x, w, bias, residual, y, B, Cin, Cout, L, false, tg_stream(stream))
                 : launch_act<1>(x, w, bias, residual, y, B, Cin, Cout, L, false, tg_stream(stream));
}

int tg_conv1d_dgrad(const float* gy, const float* w, float* gx, int B, int Cin, int Cout, int L, int ks, void* stream) {
  TG_CHECK_PTR(gy); TG_CHECK_PTR(w); TG_CHECK_PTR(gx);
  TG_CHECK_POS(B); TG_CHECK_POS(Cin); TG_CHECK_POS(Cout); TG_CHECK_POS(L); TG_CHECK_POS(ks);
  if (!conv1d_shape_ok(B, Cin, Cout, L, ks)) return TG_EUNSUPPORTED;
  return ks == 3 ? launch_act<3>(gy, w, nullptr, nullptr, gx, B, Cout, Cin, L, true, tg_stream(stream))
                 : launch_act<1>(gy, w, nullptr, nullptr, gx, B, Cout, Cin, L, true, tg_stream(stream));
}

size_t tg_conv1d_wgrad_workspace(int B, int Cin, int Cout, int L, int ks) {
  if (!conv1d_shape_ok(B, Cin, Cout, L, ks)) return 0;
  int splits, kchunk;
  wgrad_split(B, Cin, Cout, L, ks, &splits, &kchunk);
  return (size_t)splits * (size_t)Cout * ((size_t)Cin * ks + 1) * sizeof(float);
}

int tg_conv1d_wgrad(const float* x, const float* gy, float* gw, float* gbias, float* workspace, size_t workspace_bytes, int B, int Cin,
                    int Cout, int L, int ks, int accumulate, void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(gy); TG_CHECK_PTR(gw); TG_CHECK_PTR(workspace);
  TG_CHECK_POS(B); TG_CHECK_POS(Cin); TG_CHECK_POS(Cout); TG_CHECK_POS(L); TG_CHECK_POS(ks);
  if (!conv1d_shape_ok(B, Cin, Cout, L, ks)) return TG_EUNSUPPORTED;
  if (workspace_bytes < tg_conv1d_wgrad_workspace(B, Cin, Cout, L, ks)) return TG_EWORKSPACE;
  int splits, kchunk;
  wgrad_split(B, Cin, Cout, L, ks, &splits, &kchunk);
  hipStream_t st = tg_stream(stream);
  const int rc = ks == 3 ? launch_wgrad<3>(x, gy, workspace, B, Cin, Cout, L, splits, kchunk, st)
                         : launch_wgrad<1>(x, gy, workspace, B, Cin, Cout, L, splits, kchunk, st);
  if (rc != TG_OK) return rc;
  const int Ncols = Cin * ks + 1;
  conv1d_wgrad_reduce_kernel<<<tg_ew_grid((int64_t)Cout * Ncols, 256), 256, 0, st>>>(workspace, gw, gbias, Cout, Ncols, splits, accumulate);
  return tg_launch_status();
}

int tg_up2x1d(const float* x, float* y, float alpha, int BC, int L, void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(y); TG_CHECK_POS(BC); TG_CHECK_POS(L);
  const int64_t total = 2ll * BC * L;
  up2x1d_kernel<<<tg_ew_grid(total, 256), 256, 0, tg_stream(stream)>>>(x, y, alpha, total);
  return tg_launch_status();
}

int tg_pool2_1d(const float* x, const float* residual, float* y, int BC, int L, void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(y); TG_CHECK_POS(BC); TG_CHECK_POS(L);
  const int64_t total = (int64_t)BC * L;
  pool2_1d_kernel<<<tg_ew_grid(total, 256), 256, 0, tg_stream(stream)>>>(x, residual, y, total);
  return tg_launch_status();
}

}  // extern "C"
