// The IQN head behind the pooled features, fused (include/tartangan_amd.h: tg_iqn_head_fwd / tg_iqn_head_bwd).
//
// The composed head is ~35 launches of a few microseconds of work each (cosine embedding, two Linear layers, tanh, the mix, the
// quantile mean and the Huber loss with their backwards).  The whole of it is ~3e6 multiply-adds at B = 64, C = 128: latency,
// not throughput, so the kernels here are plain VALU code (the cosine embedding in fp32, in tg_iqn_cos_embed's evaluation order;
// the pre-activation, exp, tanh and its derivative, and every sum in double) whose only concern is to sum in a fixed order.
//   forward : one workgroup per (g, b); its waves take the Q rows of that image in turn, the lanes of a wave the channels.  The
//             quantile mean and the image's share of the loss are complete inside the workgroup; the G*B shares are summed by a
//             one-workgroup second launch.
//   backward: one workgroup per slab of HB_WAVES channels, one wave per channel; a lane owns the images gb = lane, lane + 64, ...
//             and walks their Q rows, so df[gb][c] is complete in a lane and the parameter gradients of a channel in a wave.
//             The cosine embedding of 64 rows at a time is computed once per workgroup into LDS and shared by its channels.
// s = tanh(b1 + e . W1) is never stored: the backward recomputes it with the forward's own code (head_s).
#include "common.h"

namespace {

constexpr int HF_BLOCK = 256;                 // forward: 4 waves
constexpr int HF_WAVES = HF_BLOCK / TG_WAVE;
constexpr int HB_WAVES = 8;                   // backward: 8 channels per workgroup
constexpr int HB_BLOCK = HB_WAVES * TG_WAVE;
constexpr int HEAD_MAX_D = 20;                // embedding dims the kernels hold in registers (the reference's quantile_dims)

// A double kept in the float workspace as two 32-bit words: the workspace, like every pointer here, may sit at any multiple of 4 bytes
__device__ __forceinline__ void put_double(float* ws, int i, double v) {
  const long long bits = __double_as_longlong(v);
  ws[2 * i] = __int_as_float((int)(bits & 0xffffffffll));
  ws[2 * i + 1] = __int_as_float((int)(bits >> 32));
}
__device__ __forceinline__ double get_double(const float* ws, int i) {
  const unsigned long long lo = (unsigned int)__float_as_int(ws[2 * i]), hi = (unsigned int)__float_as_int(ws[2 * i + 1]);
  return __longlong_as_double((long long)(lo | (hi << 32)));
}

__device__ __forceinline__ float head_cos(float tau, float range) {
  const float pi = 3.14159265358979323846f;   // np.pi rounded to fp32, as tg_iqn_cos_embed
  return cosf((tau * pi) * range);
}

// s = tanh(a) and 1 - s^2 for a = b1[c] + sum_j e[j] W1[c][j] (fp32 e, summed in double, j ascending): the one definition both
// directions use.  From u = exp(-2|a|) in double: s = (1 - u) / (1 + u), 1 - s^2 = 4u / (1 + u)^2.  The second has no cancellation where s is next
// to +-1 -- 1 - s*s of an fp32 tanh loses every digit there, and the parameter gradients are sums of such terms -- and one double
// exp per element costs nothing at this size.
struct HeadS {
  double s, om;
};
template <int DCAP>
__device__ __forceinline__ HeadS head_s(const float* e, const float* __restrict__ w1c, float b1c, int D) {
  double a = (double)b1c;
#pragma unroll
  for (int j = 0; j < DCAP; ++j)
    if (j < D) a = fma((double)e[j], (double)w1c[j], a);
  const double u = exp(-2.0 * fabs(a)), d = 1.0 / (1.0 + u);
  const double sa = (1.0 - u) * d;
  return HeadS{a < 0.0 ? -sa : sa, 4.0 * u * d * d};
}

template <int DCAP>
__global__ void __launch_bounds__(HF_BLOCK) iqn_head_fwd_kernel(const float* __restrict__ f, const float* __restrict__ taus,
                                                                const float* __restrict__ target, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, const float* __restrict__ range,
                                                                float k, float* __restrict__ pt, float* __restrict__ loss,
                                                                float* __restrict__ dpreds, float* __restrict__ partial,
                                                                int G, int B, int Q, int C, int D) {
  __shared__ float se[HF_WAVES][DCAP];
  __shared__ float sp[HF_WAVES];
  const int gb = blockIdx.x, g = gb / B, b = gb - g * B;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float* frow = f + (int64_t)gb * C;
  const float bias2 = b2 ? b2[0] : 0.f;
  const float tgt = target ? target[gb] : 0.f;
  const float inv_b = 1.f / (float)B;
  double psum = 0.0;         // thread 0 only: sum_q p, q ascending
  double lsum = 0.0;         // thread 0 only: this image's share of the loss
  for (int q0 = 0; q0 < Q; q0 += HF_WAVES) {
    const int q = q0 + wid;
    const int r = g * Q * B + q * B + b;
    if (q < Q && lane < D) se[wid][lane] = head_cos(taus[r], range[lane]);
    __syncthreads();
    if (q < Q) {
      float e[DCAP];
#pragma unroll
      for (int j = 0; j < DCAP; ++j) e[j] = j < D ? se[wid][j] : 0.f;
      double acc = 0.0;          // (sums in double throughout: a fixed order AND no rounding of its own to speak of)
      for (int c = lane; c < C; c += TG_WAVE) acc += ((double)frow[c] * head_s<DCAP>(e, W1 + (int64_t)c * D, b1[c], D).s) * (double)w2[c];
      acc = wave_sum_d(acc);
      if (lane == 0) sp[wid] = (float)(acc + (double)bias2);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < HF_WAVES && q0 + w < Q; ++w) {
        const float p = sp[w];
        psum += (double)p;
        if (target) {
          const int rr = g * Q * B + (q0 + w) * B + b;
          const float err = tgt - p;
          const float a = fabsf(err);
          const bool quad = a <= k;
          const float hub = quad ? 0.5f * err * err : k * (a - 0.5f * k);
          const float dh = quad ? err : (err > 0.f ? k : (err < 0.f ? -k : 0.f));
          const float wq = fabsf(taus[rr] - (err < 0.f ? 1.f : 0.f));
          lsum += (double)(wq * hub);
          dpreds[rr] = -wq * dh * inv_b;
        }
      }
    }
  }
  if (threadIdx.x == 0) {
    pt[gb] = (float)(psum / (double)Q);
    if (target) {
      if (G * B == 1) loss[0] = (float)(lsum / (double)B);
      else put_double(partial, gb, lsum);
    }
  }
}

// *loss = (1 / B) * sum of the n per-image shares, in a fixed order
__global__ void __launch_bounds__(HF_BLOCK) iqn_head_loss_finish(const float* __restrict__ partial, int n, double inv_b,
                                                                 float* __restrict__ loss) {
  __shared__ double scratch[32];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += HF_BLOCK) acc += get_double(partial, i);
  acc = block_sum_d(acc, scratch);
  if (threadIdx.x == 0) loss[0] = (float)(acc * inv_b);
}

template <int DCAP>
__global__ void __launch_bounds__(HB_BLOCK) iqn_head_bwd_kernel(const float* __restrict__ gl, const float* __restrict__ gpt,
                                                                const float* __restrict__ dpreds, const float* __restrict__ f,
                                                                const float* __restrict__ taus, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ range, float* __restrict__ df,
                                                                float* __restrict__ dW1, float* __restrict__ db1,
                                                                float* __restrict__ dw2, float* __restrict__ db2, int G, int B,
                                                                int Q, int C, int D, int accumulate) {
  __shared__ float se[TG_WAVE][DCAP + 1];          // (+1: a lane reads its own row, consecutive rows in consecutive banks)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = blockIdx.x * HB_WAVES + wid;
  const bool active = c < C;
  const bool params = dW1 || db1 || dw2;
  const bool first = blockIdx.x == 0 && wid == 0;  // (channel 0 exists: C >= 1) this wave also sums delta for db2
  const int GB = G * B;
  const double glv = gl ? (double)gl[0] : 0.0;
  float w1c[DCAP];
#pragma unroll
  for (int j = 0; j < DCAP; ++j) w1c[j] = (active && j < D) ? W1[(int64_t)c * D + j] : 0.f;
  const float b1c = active ? b1[c] : 0.f, w2c = active ? w2[c] : 0.f;
  double a_w1[DCAP];         // (sums in double: see the forward)
#pragma unroll
  for (int j = 0; j < DCAP; ++j) a_w1[j] = 0.0;
  double a_b1 = 0.0, a_w2 = 0.0, a_b2 = 0.0;
  for (int gb0 = 0; gb0 < GB; gb0 += TG_WAVE) {
    const int gb = gb0 + lane;
    const bool row_ok = gb < GB;
    const int g = row_ok ? gb / B : 0, b = row_ok ? gb - g * B : 0;
    const float fv = (active && row_ok) ? f[(int64_t)gb * C + c] : 0.f;
    const double gp = (gpt && row_ok) ? (double)gpt[gb] / (double)Q : 0.0;
    double a_f = 0.0;
    for (int q = 0; q < Q; ++q) {
      __syncthreads();                              // the previous tile has been read
      for (int i = threadIdx.x; i < TG_WAVE * D; i += HB_BLOCK) {
        const int l = i / D, j = i - l * D;
        const int gbl = gb0 + l;
        if (gbl < GB) {
          const int gl_ = gbl / B;
          se[l][j] = head_cos(taus[gl_ * Q * B + q * B + (gbl - gl_ * B)], range[j]);
        }
      }
      __syncthreads();
      if (active && row_ok) {
        const int r = g * Q * B + q * B + b;
        float e[DCAP];
#pragma unroll
        for (int j = 0; j < DCAP; ++j) e[j] = j < D ? se[lane][j] : 0.f;
        const double delta = (gl ? glv * (double)dpreds[r] : 0.0) + gp;
        const HeadS h = head_s<DCAP>(e, w1c, b1c, D);
        a_f += delta * h.s;
        if (first) a_b2 += delta;
        if (params) {
          const double t = delta * (double)fv;
          a_w2 += t * h.s;
          const double da = (t * (double)w2c) * h.om;
          a_b1 += da;
#pragma unroll
          for (int j = 0; j < DCAP; ++j) a_w1[j] = fma(da, (double)e[j], a_w1[j]);
        }
      }
    }
    if (df && active && row_ok) df[(int64_t)gb * C + c] = (float)((double)w2c * a_f);
  }
  // the lanes' sums of one channel: a fixed butterfly
  if (params) {
    a_w2 = wave_sum_d(a_w2);
    a_b1 = wave_sum_d(a_b1);
#pragma unroll
    for (int j = 0; j < DCAP; ++j) a_w1[j] = wave_sum_d(a_w1[j]);
    if (active && lane == 0) {
      if (dw2) dw2[c] = (accumulate ? dw2[c] : 0.f) + (float)a_w2;
      if (db1) db1[c] = (accumulate ? db1[c] : 0.f) + (float)a_b1;
    }
    if (active && dW1) {
#pragma unroll
      for (int j = 0; j < DCAP; ++j)
        if (lane == j && j < D) dW1[(int64_t)c * D + j] = (accumulate ? dW1[(int64_t)c * D + j] : 0.f) + (float)a_w1[j];
    }
  }
  if (db2 && blockIdx.x == 0 && wid == 0) {
    a_b2 = wave_sum_d(a_b2);
    if (lane == 0) db2[0] = (accumulate ? db2[0] : 0.f) + (float)a_b2;
  }
}

}  // namespace

extern "C" {

size_t tg_iqn_head_workspace(int G, int B) {
  if (G < 1 || B < 1) return 0;
  return (size_t)G * (size_t)B * sizeof(double);
}

int tg_iqn_head_fwd(const float* f, const float* taus, const float* target, const float* W1, const float* b1, const float* w2,
                    const float* b2, const float* range, float k, float* pt, float* loss, float* dpreds, float* workspace,
                    int G, int B, int Q, int C, int D, void* stream) {
  TG_CHECK_PTR(f); TG_CHECK_PTR(taus); TG_CHECK_PTR(W1); TG_CHECK_PTR(b1); TG_CHECK_PTR(w2); TG_CHECK_PTR(range); TG_CHECK_PTR(pt);
  TG_CHECK_POS(B); TG_CHECK_POS(Q); TG_CHECK_POS(C); TG_CHECK_POS(D);
  if (G != 1 && G != 2) return TG_EINVAL;
  if (target && (!loss || !dpreds || !workspace)) return TG_EINVAL;
  if (D > HEAD_MAX_D) return TG_EUNSUPPORTED;
  if (!target) loss = nullptr, dpreds = nullptr;
  const int GB = G * B;
  iqn_head_fwd_kernel<HEAD_MAX_D><<<GB, HF_BLOCK, 0, tg_stream(stream)>>>(f, taus, target, W1, b1, w2, b2, range, k, pt, loss, dpreds,
                                                                          workspace, G, B, Q, C, D);
  if (target && GB > 1) iqn_head_loss_finish<<<1, HF_BLOCK, 0, tg_stream(stream)>>>(workspace, GB, 1.0 / (double)B, loss);
  return tg_launch_status();
}

int tg_iqn_head_bwd(const float* gl, const float* gpt, const float* dpreds, const float* f, const float* taus, const float* W1,
                    const float* b1, const float* w2, const float* range, float* df, float* dW1, float* db1, float* dw2,
                    float* db2, int G, int B, int Q, int C, int D, int accumulate, void* stream) {
  TG_CHECK_PTR(f); TG_CHECK_PTR(taus); TG_CHECK_PTR(W1); TG_CHECK_PTR(b1); TG_CHECK_PTR(w2); TG_CHECK_PTR(range);
  TG_CHECK_POS(B); TG_CHECK_POS(Q); TG_CHECK_POS(C); TG_CHECK_POS(D);
  if (G != 1 && G != 2) return TG_EINVAL;
  if (gl && !dpreds) return TG_EINVAL;
  if (D > HEAD_MAX_D) return TG_EUNSUPPORTED;
  if (!df && !dW1 && !db1 && !dw2 && !db2) return TG_OK;          // nothing asked for
  const int grid = tg_div_up(C, HB_WAVES);
  iqn_head_bwd_kernel<HEAD_MAX_D><<<grid, HB_BLOCK, 0, tg_stream(stream)>>>(gl, gpt, dpreds, f, taus, W1, b1, w2, range, df, dW1, db1,
                                                                            dw2, db2, G, B, Q, C, D, accumulate);
  return tg_launch_status();
}

}  // extern "C"
