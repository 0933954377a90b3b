// Scene structure stage (models/blocks/scene.py:127-155): P small opacity patches per image, each placed on an S x S canvas by
// its own affine transform.  The reference loops over the patches in Python -- F.affine_grid(align_corners=False),
// F.grid_sample(bilinear, zeros, align_corners=False), a mask multiply, a squeeze, then stack + permute: some hundred tiny
// launches forward and more backward.  Here it is one launch each way.
//
// One workgroup of 4 waves per (b, p) plane.  theta's six floats and the <= 256 finished texel values
//     m[v][u] = (logits ? 1 - sigmoid(l) : 1) * (noise ? noise[v][u] : 1)
// live in LDS; the threads stride over the S*S pixels.  Per pixel, as ATen computes it:
//     x = (2j+1)/S - 1, y = (2i+1)/S - 1;  gx = t00 x + t01 y + t02, gy = t10 x + t11 y + t12
//     ix = ((gx+1) patch - 1)/2, iy alike;  x0 = floor(ix), corner weights (x0+1 - ix), (ix - x0), zero outside the patch.
// Backward: the six theta sums are per-thread partials reduced by wave shuffles and across the waves through LDS (a fixed
// tree).  The texel gradients are GATHERED, not scattered: the pixels are staged through LDS 256 at a time (the sample
// coordinate, its floor, the incoming gradient) and the thread that owns texel (v, u) walks them in pixel order, so every texel sum has one
// fixed order -- no atomics of any kind, two runs are bit-identical.  The work is tiny and latency-bound (a batch of 64 at the
// default geometry: 1280 planes of 256 pixels); nothing here is tuned for bandwidth.
#include "common.h"

namespace {

constexpr int SC_T = 256;        // threads per workgroup = pixels staged per round = the most texels a patch may have
constexpr int SC_MAX_PATCH = 16;

__device__ __forceinline__ float sc_sigmoid(float l) { return 1.f / (1.f + expf(-l)); }

struct ScSample {
  float x, y;          // base grid
  float ix, iy;        // sample coordinate in texels
  float x0, y0;        // its floor (kept as floats: compared with texel indices, converted only after a range check)
};

// ix is clamped to [-2, patch + 1] first: outside (-1, patch) every corner is outside the patch whatever the exact value, and
// the clamp keeps floor() of an overflowing or NaN coordinate a small number.
__device__ __forceinline__ ScSample sc_sample(const float* th, int64_t pix, int S, int patch) {
  ScSample s;
  const int i = (int)(pix / S), j = (int)(pix - (int64_t)i * S);
  s.x = (float)(2 * j + 1) / (float)S - 1.f;
  s.y = (float)(2 * i + 1) / (float)S - 1.f;
  const float gx = th[0] * s.x + th[1] * s.y + th[2];
  const float gy = th[3] * s.x + th[4] * s.y + th[5];
  float ix = ((gx + 1.f) * (float)patch - 1.f) * 0.5f;
  float iy = ((gy + 1.f) * (float)patch - 1.f) * 0.5f;
  ix = fminf(fmaxf(ix, -2.f), (float)patch + 1.f);
  iy = fminf(fmaxf(iy, -2.f), (float)patch + 1.f);
  s.ix = ix;
  s.iy = iy;
  s.x0 = floorf(ix);
  s.y0 = floorf(iy);
  return s;
}

// texel (yy, xx) of the LDS patch, zero outside (grid_sample's padding_mode='zeros')
__device__ __forceinline__ float sc_texel(const float* m, float yy, float xx, int patch) {
  const bool in = xx >= 0.f && xx <= (float)(patch - 1) && yy >= 0.f && yy <= (float)(patch - 1);
  return in ? m[(int)yy * patch + (int)xx] : 0.f;
}

__device__ __forceinline__ void sc_load_patch(float* m, float* th, const float* theta, const float* logits, const float* noise,
                                              int64_t plane, int patch) {
  const int T = patch * patch, tid = threadIdx.x;
  if (tid < T) {
    float v = logits != nullptr ? 1.f - sc_sigmoid(logits[plane * T + tid]) : 1.f;
    if (noise != nullptr) v *= noise[tid];
    m[tid] = v;
  }
  if (tid < 6) th[tid] = theta[plane * 6 + tid];
  __syncthreads();
}

__global__ void __launch_bounds__(SC_T) scene_patches_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ logits,
                                                                 const float* __restrict__ noise, float* __restrict__ out,
                                                                 int patch, int S) {
  __shared__ float m[SC_T];
  __shared__ float th[6];
  const int64_t plane = blockIdx.x, npix = (int64_t)S * S;
  sc_load_patch(m, th, theta, logits, noise, plane, patch);
  for (int64_t pix = threadIdx.x; pix < npix; pix += SC_T) {
    const ScSample s = sc_sample(th, pix, S, patch);
    const float wx1 = s.ix - s.x0, wx0 = (s.x0 + 1.f) - s.ix, wy1 = s.iy - s.y0, wy0 = (s.y0 + 1.f) - s.iy;
    const float v00 = sc_texel(m, s.y0, s.x0, patch), v01 = sc_texel(m, s.y0, s.x0 + 1.f, patch);
    const float v10 = sc_texel(m, s.y0 + 1.f, s.x0, patch), v11 = sc_texel(m, s.y0 + 1.f, s.x0 + 1.f, patch);
    out[plane * npix + pix] = v00 * (wx0 * wy0) + v01 * (wx1 * wy0) + v10 * (wx0 * wy1) + v11 * (wx1 * wy1);
  }
}

__global__ void __launch_bounds__(SC_T) scene_patches_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ theta,
                                                                 const float* __restrict__ logits, const float* __restrict__ noise,
                                                                 float* __restrict__ gtheta, float* __restrict__ glogits,
                                                                 int patch, int S) {
  __shared__ float m[SC_T];
  __shared__ float th[6];
  __shared__ float st_x0[SC_T], st_y0[SC_T], st_ix[SC_T], st_iy[SC_T], st_g[SC_T];
  __shared__ float scratch[32];
  const int64_t plane = blockIdx.x, npix = (int64_t)S * S;
  const int tid = threadIdx.x, T = patch * patch;
  sc_load_patch(m, th, theta, logits, noise, plane, patch);
  const float tu = (float)(tid % patch), tv = (float)(tid / patch);      // the texel this thread owns (tid < T)
  const float half = 0.5f * (float)patch;                                 // d ix / d gx
  float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gm = 0.f;
  for (int64_t base = 0; base < npix; base += SC_T) {
    const int64_t pix = base + tid;
    float g = 0.f, x0 = -2.f, y0 = -2.f, ix = -2.f, iy = -2.f;              // a slot past the last pixel touches nothing
    if (pix < npix) {
      const ScSample s = sc_sample(th, pix, S, patch);
      g = gout[plane * npix + pix];
      x0 = s.x0; y0 = s.y0; ix = s.ix; iy = s.iy;
      const float wx1 = ix - x0, wx0 = (x0 + 1.f) - ix, wy1 = iy - y0, wy0 = (y0 + 1.f) - iy;
      const float v00 = sc_texel(m, y0, x0, patch), v01 = sc_texel(m, y0, x0 + 1.f, patch);
      const float v10 = sc_texel(m, y0 + 1.f, x0, patch), v11 = sc_texel(m, y0 + 1.f, x0 + 1.f, patch);
      const float gix = g * half * ((v01 - v00) * wy0 + (v11 - v10) * wy1);
      const float giy = g * half * ((v10 - v00) * wx0 + (v11 - v01) * wx1);
      a[0] = fmaf(gix, s.x, a[0]); a[1] = fmaf(gix, s.y, a[1]); a[2] += gix;
      a[3] = fmaf(giy, s.x, a[3]); a[4] = fmaf(giy, s.y, a[4]); a[5] += giy;
    }
    if (glogits != nullptr) {          // (uniform over the workgroup)
      st_x0[tid] = x0; st_y0[tid] = y0; st_ix[tid] = ix; st_iy[tid] = iy; st_g[tid] = g;
      __syncthreads();
      if (tid < T) {
        const int n = (int)((npix - base) < (int64_t)SC_T ? (npix - base) : (int64_t)SC_T);
        for (int k = 0; k < n; ++k) {          // every lane reads the same slot: an LDS broadcast
          const float kx0 = st_x0[k], ky0 = st_y0[k], kix = st_ix[k], kiy = st_iy[k];
          const float cx = tu == kx0 ? (kx0 + 1.f) - kix : (tu == kx0 + 1.f ? kix - kx0 : 0.f);
          const float cy = tv == ky0 ? (ky0 + 1.f) - kiy : (tv == ky0 + 1.f ? kiy - ky0 : 0.f);
          gm = fmaf(st_g[k], cx * cy, gm);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float r = block_sum(a[k], scratch);
    if (tid == 0) gtheta[plane * 6 + k] = r;
  }
  if (glogits != nullptr && tid < T) {
    const float sg = sc_sigmoid(logits[plane * T + tid]);
    if (noise != nullptr) gm *= noise[tid];
    glogits[plane * T + tid] = -gm * ((1.f - sg) * sg);
  }
}

int sc_check(int B, int P, int patch, int S) {
  if (B <= 0 || P <= 0 || S <= 0 || patch <= 0) return TG_EINVAL;
  if (patch > SC_MAX_PATCH) return TG_EUNSUPPORTED;
  if ((int64_t)B * P > 0x7fffffffll || S > (1 << 30)) return TG_EUNSUPPORTED;       // the grid; 2j+1 as an int
  return TG_OK;
}

}  // namespace

extern "C" {

int tg_scene_patches_fwd(const float* theta, const float* mask_logits, const float* noise, float* out, int B, int P, int patch,
                         int S, void* stream) {
  TG_CHECK_PTR(theta); TG_CHECK_PTR(out);
  const int rc = sc_check(B, P, patch, S);
  if (rc != TG_OK) return rc;
  scene_patches_fwd_kernel<<<B * P, SC_T, 0, tg_stream(stream)>>>(theta, mask_logits, noise, out, patch, S);
  return tg_launch_status();
}

int tg_scene_patches_bwd(const float* gout, const float* theta, const float* mask_logits, const float* noise, float* gtheta,
                         float* gmask_logits, int B, int P, int patch, int S, void* stream) {
  TG_CHECK_PTR(gout); TG_CHECK_PTR(theta); TG_CHECK_PTR(gtheta);
  if ((mask_logits == nullptr) != (gmask_logits == nullptr)) return TG_EINVAL;
  const int rc = sc_check(B, P, patch, S);
  if (rc != TG_OK) return rc;
  scene_patches_bwd_kernel<<<B * P, SC_T, 0, tg_stream(stream)>>>(gout, theta, mask_logits, noise, gtheta, gmask_logits, patch, S);
  return tg_launch_status();
}

}  // extern "C"
