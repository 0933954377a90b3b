// The explore apps' own kernels (tartangan_amd/explore/): the find-image reconstruction loss with its image gradient, the whole
// latent update of a find-image step in one launch, and continuous-interp's mosaic gather.  All three are latency kernels at the
// sizes the apps use (a batch of 2 images, a few hundred latents, one 256 x 256 mosaic): plain 4-byte loads that take any
// alignment, fp32 throughout, fixed-order sums (a serial grid-stride sum per thread, a shuffle tree per wave, the waves in order),
// no atomics -- two runs give the same bits.
#include "common.h"

namespace {

constexpr int EX_BLOCK = 256;
constexpr int RECON_MAX_BLOCKS = 256;      // one per CU; the second stage reads them with one 256-thread block, one each
constexpr int RECON_PER_THREAD = 4;

// torchvision's Normalize(mean, std) for ImageNet, the constants of find_image.py:99-100
__device__ __constant__ float kMean[3] = {0.485f, 0.456f, 0.406f};
__device__ __constant__ float kStd[3] = {0.229f, 0.224f, 0.225f};

static inline int recon_grid(int64_t n) {
  int64_t g = (n + (int64_t)EX_BLOCK * RECON_PER_THREAD - 1) / ((int64_t)EX_BLOCK * RECON_PER_THREAD);
  return (int)(g < 1 ? 1 : (g > RECON_MAX_BLOCKS ? RECON_MAX_BLOCKS : g));
}

// d = ((x + 1) / 2 - mean_c) / std_c - t;  kind 0: d^2, kind 1: SmoothL1(beta = 1);  grad = rho'(d) / (2 std_c)
template <int KIND>
__global__ void __launch_bounds__(EX_BLOCK) recon_loss_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                              float* __restrict__ grad, float* __restrict__ partial,
                                                              float* __restrict__ loss, int64_t n, int64_t HW) {
  __shared__ float scratch[32];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)EX_BLOCK + threadIdx.x; i < n; i += gridDim.x * (int64_t)EX_BLOCK) {
    const int c = (int)((i / HW) % 3);
    const float sd = kStd[c];
    const float d = ((x[i] + 1.f) * 0.5f - kMean[c]) / sd - t[i];
    float term, slope;
    if (KIND == 0) {
      term = d * d;
      slope = 2.f * d;
    } else {
      const float a = fabsf(d);
      const bool quad = a < 1.f;
      term = quad ? 0.5f * d * d : a - 0.5f;
      slope = quad ? d : (d > 0.f ? 1.f : -1.f);          // (NaN: a < 1 is false and d > 0 is false; term is NaN, as it must be)
      if (d != d) slope = d;
    }
    acc += term;
    if (grad) grad[i] = slope / (2.f * sd);
  }
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) *loss = acc;
    else partial[blockIdx.x] = acc;
  }
}

__global__ void __launch_bounds__(EX_BLOCK) recon_finish_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ loss) {
  __shared__ float scratch[32];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += EX_BLOCK) acc += partial[i];
  acc = block_sum(acc, scratch);
  if (threadIdx.x == 0) *loss = acc;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float block_min(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_min(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = scratch[0];
  for (int i = 1; i < nw; ++i) r = fminf(r, scratch[i]);
  return r;
}

struct LatentHyper {
  float lr, b2, omb1, omb2, eps, l2, g_coef;      // g_coef = 2 l2 / n
  double beta1, beta2, lr_d;
};

// ONE workgroup walks the n latents three times (they stay in L1/L2: n is a few hundred to a few thousand).
// opt 0 Adam, 1 SGD, 2 clip only.
__global__ void __launch_bounds__(EX_BLOCK) latent_step_kernel(float* __restrict__ z, const float* __restrict__ gz, float* __restrict__ m,
                                                               float* __restrict__ v, int64_t* __restrict__ step,
                                                               const float* __restrict__ noise, float* __restrict__ stats,
                                                               const float* __restrict__ recon, int64_t n, int opt, LatentHyper h) {
  __shared__ float scratch[32];
  const int tid = threadIdx.x;
  if (opt != 2) {
    // 1. the reported loss, from z BEFORE the update
    float sq = 0.f;
    for (int64_t i = tid; i < n; i += EX_BLOCK) sq += z[i] * z[i];
    sq = block_sum(sq, scratch);
    if (tid == 0) stats[0] = *recon + h.l2 * (sq / (float)n);
    // 2.-4. the update
    float step_size = h.lr, bc2_sqrt = 1.f;
    if (opt == 0) {
      const int64_t t = step[0] + 1;                 // every thread reads it; thread 0 writes it back behind the barrier below
      const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
      step_size = (float)(h.lr_d / bc1);
      bc2_sqrt = (float)sqrt(bc2);
    }
    float mn = INFINITY, mx = -INFINITY, sum = 0.f, nans = 0.f;
    for (int64_t i = tid; i < n; i += EX_BLOCK) {
      float zi = z[i];
      const float gi = gz[i] + h.g_coef * zi;
      if (opt == 0) {
        float mi = m[i], vi = v[i];
        const float d = gi - mi;                     // torch.lerp(m, g, 1 - beta1), as tg_adam_step
        mi = (h.omb1 < 0.5f) ? (mi + h.omb1 * d) : (gi - d * (1.f - h.omb1));
        vi = vi * h.b2;
        vi = vi + (h.omb2 * gi) * gi;
        zi = zi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + h.eps));
        m[i] = mi;
        v[i] = vi;
      } else {
        zi = zi - h.lr * gi;
      }
      z[i] = zi;
      // 5. statistics of the updated z; torch's min / max return NaN when there is one, fminf / fmaxf skip it
      mn = fminf(mn, zi);
      mx = fmaxf(mx, zi);
      sum += zi;
      nans += (zi != zi) ? 1.f : 0.f;
    }
    mn = block_min(mn, scratch);
    mx = block_max(mx, scratch);
    sum = block_sum(sum, scratch);
    nans = block_sum(nans, scratch);                  // (its first barrier is also the one between the reads and the write of *step)
    if (tid == 0) {
      const float nan = __int_as_float(0x7fc00000);
      stats[1] = nans > 0.f ? nan : mn;
      stats[2] = sum / (float)n;
      stats[3] = nans > 0.f ? nan : mx;
      if (opt == 0) step[0] = step[0] + 1;
    }
  }
  // 6. stochastic clipping (find_image.py:77-81): strictly outside [-3, 3] -> the noise; NaN compares false and stays
  if (noise) {
    for (int64_t i = tid; i < n; i += EX_BLOCK) {     // each thread rereads only what it wrote itself
      const float zi = z[i];
      if (zi > 3.f || zi < -3.f) z[i] = noise[i];
    }
  }
}

__global__ void __launch_bounds__(EX_BLOCK) mosaic_gather_kernel(const float* __restrict__ imgs, float* __restrict__ out, int rows, int cols,
                                                                 int C, int h, int w, int S) {
  const int64_t total = (int64_t)C * S * S;
  for (int64_t i = blockIdx.x * (int64_t)EX_BLOCK + threadIdx.x; i < total; i += gridDim.x * (int64_t)EX_BLOCK) {
    const int x = (int)(i % S), y = (int)((i / S) % S), c = (int)(i / ((int64_t)S * S));
    const int64_t gy = ((int64_t)y * rows) / S, gx = ((int64_t)x * cols) / S;
    const int64_t iy = ((int64_t)y * h) / S, ix = ((int64_t)x * w) / S;
    out[i] = imgs[(((gy * cols + gx) * C + c) * h + iy) * w + ix];
  }
}

}  // namespace

extern "C" {

size_t tg_recon_loss_workspace(int B, int C, int HW) {
  if (B <= 0 || C != 3 || HW <= 0) return 0;
  return sizeof(float) * (size_t)recon_grid((int64_t)B * C * HW);
}

int tg_recon_loss(const float* imgs, const float* target, float* grad_imgs, float* loss_out, float* workspace, size_t workspace_bytes,
                  int B, int C, int HW, int kind, void* stream) {
  TG_CHECK_PTR(imgs); TG_CHECK_PTR(target); TG_CHECK_PTR(loss_out);
  TG_CHECK_POS(B); TG_CHECK_POS(HW);
  if (C != 3 || (kind != 0 && kind != 1)) return TG_EINVAL;
  const int64_t n = (int64_t)B * C * HW;
  const int g = recon_grid(n);
  if (g > 1 && (workspace == nullptr || workspace_bytes < sizeof(float) * (size_t)g)) return TG_EWORKSPACE;
  hipStream_t st = tg_stream(stream);
  if (kind == 0) recon_loss_kernel<0><<<g, EX_BLOCK, 0, st>>>(imgs, target, grad_imgs, workspace, loss_out, n, HW);
  else recon_loss_kernel<1><<<g, EX_BLOCK, 0, st>>>(imgs, target, grad_imgs, workspace, loss_out, n, HW);
  if (g > 1) recon_finish_kernel<<<1, EX_BLOCK, 0, st>>>(workspace, g, loss_out);
  return tg_launch_status();
}

int tg_latent_step(float* z, const float* gz, float* m, float* v, int64_t* step, const float* noise_next, float* stats,
                   const float* recon_loss, int64_t n, int opt, double lr, double beta1, double beta2, double eps, double l2,
                   void* stream) {
  TG_CHECK_PTR(z);
  if (n <= 0 || opt < 0 || opt > 2) return TG_EINVAL;
  if (opt == 2) {
    TG_CHECK_PTR(noise_next);
  } else {
    TG_CHECK_PTR(gz); TG_CHECK_PTR(stats); TG_CHECK_PTR(recon_loss);
    if (opt == 0) {
      TG_CHECK_PTR(m); TG_CHECK_PTR(v); TG_CHECK_PTR(step);
      if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return TG_EINVAL;
    }
  }
  LatentHyper h;
  h.lr = (float)lr; h.b2 = (float)beta2; h.omb1 = (float)(1.0 - beta1); h.omb2 = (float)(1.0 - beta2); h.eps = (float)eps;
  h.l2 = (float)l2; h.g_coef = (float)(2.0 * l2 / (double)n);
  h.beta1 = beta1; h.beta2 = beta2; h.lr_d = lr;
  latent_step_kernel<<<1, EX_BLOCK, 0, tg_stream(stream)>>>(z, gz, m, v, step, noise_next, stats, recon_loss, n, opt, h);
  return tg_launch_status();
}

int tg_mosaic_gather(const float* imgs, float* out, int rows, int cols, int C, int h, int w, int S, void* stream) {
  TG_CHECK_PTR(imgs); TG_CHECK_PTR(out);
  TG_CHECK_POS(rows); TG_CHECK_POS(cols); TG_CHECK_POS(C); TG_CHECK_POS(h); TG_CHECK_POS(w); TG_CHECK_POS(S);
  mosaic_gather_kernel<<<tg_ew_grid((int64_t)C * S * S, EX_BLOCK), EX_BLOCK, 0, tg_stream(stream)>>>(imgs, out, rows, cols, C, h, w, S);
  return tg_launch_status();
}

}  // extern "C"
