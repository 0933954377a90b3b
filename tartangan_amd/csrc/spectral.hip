// Spectral norm (north_star item a15; the reference's only trace is prep4web.py:33-51 which strips
// torch.nn.utils.spectral_norm from a checkpoint, so the semantics pinned here are torch's):
//     v <- normalize(W^T u, eps),  u <- normalize(W v, eps)   (in place),   sigma = u^T W v,   W_sn = W / sigma
// W is rows x cols (Cout x Cin*k*k).  Two forms:
//   * tg_sn_power_iter: ONE workgroup of 16 waves per matrix, n_iter iterations, sigma only.  The per-layer route of
//     models/layers.SpectralNormConv2d outside a spectral scope; any size is computed correctly, but a 1024 x 9216 filter of
//     '128big' streams 37.7 MB x 3 through a single CU.
//   * tg_sn_batch_fwd / tg_sn_batch_bwd: every layer of a network per call, one iteration, the grid spread over (layer, tile), the
//     stages ordered by launch boundaries alone (no atomics, no flags, no grid barrier); what the trainers' --spectral-norm uses.
//     forward: (1) W^T u partials per (layer, 64-row slab, 256-column chunk)  (2) per layer: sum the slabs, norm, v
//              (3) W v, one wave per row, wavefront-shuffle sum, into a scratch u'  (4) per (layer, 2048-element chunk): |u'| and sigma
//              recomputed locally in one fixed order, W_sn written; the layer's first workgroup writes u and sigma.
//     backward: (1) <g_sn, w_sn> partials per chunk  (2) per chunk: sum the partials in one fixed order, apply.
//     The vector (float4) and scalar paths of every stage add in the same order: their results are bit-identical.
// W^T u runs over columns in a lane (coalesced along the row), W v one row per wave with a wavefront-shuffle reduction; the norms are
// block reductions (in double for the batched form: a few thousand terms per layer).
#include "common.h"

namespace {

constexpr int SNB = 1024;

__device__ __forceinline__ float block_sum_1024(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < SNB / 64; ++i) r += scratch[i];
  return r;
}

__global__ void __launch_bounds__(SNB) sn_power_iter_kernel(const float* __restrict__ W, float* __restrict__ u, float* __restrict__ v,
                                                            float* __restrict__ sigma, int rows, int cols, int n_iter, float eps) {
  __shared__ float scratch[32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int it = 0; it < n_iter; ++it) {
    // v = W^T u
    float nrm = 0.f;
    for (int j = threadIdx.x; j < cols; j += SNB) {
      float acc = 0.f;
      for (int i = 0; i < rows; ++i) acc = fmaf(W[(int64_t)i * cols + j], u[i], acc);
      v[j] = acc;
      nrm = fmaf(acc, acc, nrm);
    }
    nrm = sqrtf(block_sum_1024(nrm, scratch));
    const float inv = 1.f / fmaxf(nrm, eps);
    for (int j = threadIdx.x; j < cols; j += SNB) v[j] *= inv;
    __syncthreads();
    // u = W v
    for (int i = wave; i < rows; i += SNB / 64) {
      float acc = 0.f;
      for (int j = lane; j < cols; j += 64) acc = fmaf(W[(int64_t)i * cols + j], v[j], acc);
      acc = wave_sum(acc);
      if (lane == 0) u[i] = acc;
    }
    __syncthreads();
    float un = 0.f;
    for (int i = threadIdx.x; i < rows; i += SNB) un = fmaf(u[i], u[i], un);
    un = sqrtf(block_sum_1024(un, scratch));
    const float uinv = 1.f / fmaxf(un, eps);
    for (int i = threadIdx.x; i < rows; i += SNB) u[i] *= uinv;
    __syncthreads();
  }
  if (sigma != nullptr) {
    float part = 0.f;
    for (int i = wave; i < rows; i += SNB / 64) {
      float acc = 0.f;
      for (int j = lane; j < cols; j += 64) acc = fmaf(W[(int64_t)i * cols + j], v[j], acc);
      acc = wave_sum(acc);
      if (lane == 0) part = fmaf(u[i], acc, part);
    }
    part = block_sum_1024(part, scratch);
    if (threadIdx.x == 0) *sigma = part;
  }
}

__global__ void recip_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n) {
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) out[i] = 1.f / x[i];
}

// =========================================================================== the batched form
constexpr int SN_MAX_ITEMS = 48;      // layers per group of launches (the table travels by value: 48 x 72 bytes of kernel arguments)
constexpr int SN_SLAB = 64;           // rows per W^T u partial (4 waves x 16 rows)
constexpr int SN_COLS = 256;          // columns per W^T u workgroup (64 lanes x 4)
constexpr int SN_ELEMS = 2048;        // flat elements per workgroup of the element-wise stages (256 threads x 2 x 4)
constexpr int SN_WAVES = 4;           // rows per workgroup of W v

struct SnItem {
  const float* w; float* u; float* v; float* wsn; float* gsn; float* gorig;
  int rows, cols;
  int t1_end, t3_end, ch_end;         // running ends of this layer's tiles in the three grids (stage 1, stage 3, element-wise)
  int ws_off;                         // this layer's first float in the workspace: [slabs x cols | rows | chunks]
};
struct SnBatch { SnItem it[SN_MAX_ITEMS]; int n, base; };

__device__ __forceinline__ int sn_slabs(int rows) { return (rows + SN_SLAB - 1) / SN_SLAB; }
__device__ __forceinline__ int sn_chunks(int rows, int cols) { return (int)(((int64_t)rows * cols + SN_ELEMS - 1) / SN_ELEMS); }
__device__ __forceinline__ bool sn_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// stage 1: part[slab][j] = sum over the slab's rows of W[i][j] u[i]; rows in order inside a wave, then the four waves in order
__global__ void __launch_bounds__(256) sn_wtu_kernel(SnBatch b, float* __restrict__ ws) {
  __shared__ float red[SN_WAVES][SN_COLS];
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].t1_end) ++i;            // (block-uniform)
  const SnItem& it = b.it[i];
  const int t = (int)blockIdx.x - (i == 0 ? 0 : b.it[i - 1].t1_end);
  const int rows = it.rows, cols = it.cols, nch = (cols + SN_COLS - 1) / SN_COLS;
  const int slab = t / nch, chunk = t - slab * nch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = chunk * SN_COLS + lane * 4;
  const int r0 = slab * SN_SLAB + wave * (SN_SLAB / SN_WAVES);
  const int r1 = min(r0 + SN_SLAB / SN_WAVES, rows);
  const float* __restrict__ w = it.w;
  const float* __restrict__ u = it.u;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (sn_al16(w) && (cols & 3) == 0) {
    if (j0 < cols) {
#pragma unroll 8
      for (int r = r0; r < r1; ++r) {
        const float4 x = *reinterpret_cast<const float4*>(w + (int64_t)r * cols + j0);
        const float ur = u[r];
        a[0] = fmaf(x.x, ur, a[0]); a[1] = fmaf(x.y, ur, a[1]); a[2] = fmaf(x.z, ur, a[2]); a[3] = fmaf(x.w, ur, a[3]);
      }
    }
  } else {
    for (int r = r0; r < r1; ++r) {
      const float ur = u[r];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k < cols) a[k] = fmaf(w[(int64_t)r * cols + j0 + k], ur, a[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[wave][lane * 4 + k] = a[k];
  __syncthreads();
  const int j = chunk * SN_COLS + (int)threadIdx.x;
  if (j < cols) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < SN_WAVES; ++q) s += red[q][threadIdx.x];
    ws[it.ws_off + (int64_t)slab * cols + j] = s;
  }
}

// stage 2, one workgroup per layer: t[j] = sum of the slabs in order, v = t / max(|t|, eps)
__global__ void __launch_bounds__(1024) sn_v_kernel(SnBatch b, const float* __restrict__ ws, float eps) {
  __shared__ double scratch[32];
  const SnItem& it = b.it[blockIdx.x];
  const int cols = it.cols, slabs = sn_slabs(it.rows);
  const float* __restrict__ part = ws + it.ws_off;
  float* __restrict__ v = it.v;
  double nrm = 0.0;
  for (int j = threadIdx.x; j < cols; j += 1024) {
    float acc = part[j];
    for (int s = 1; s < slabs; ++s) acc += part[(int64_t)s * cols + j];
    v[j] = acc;
    nrm = fma((double)acc, (double)acc, nrm);
  }
  nrm = block_sum_d(nrm, scratch);
  const float den = fmaxf((float)sqrt(nrm), eps);
  for (int j = threadIdx.x; j < cols; j += 1024) v[j] = v[j] / den;          // the element this thread wrote above
}

// stage 3: u'[i] = sum_j W[i][j] v[j], one wave per row; a lane adds its columns in order, then the wavefront-shuffle tree
__global__ void __launch_bounds__(64 * SN_WAVES) sn_wv_kernel(SnBatch b, float* __restrict__ ws) {
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].t3_end) ++i;
  const SnItem& it = b.it[i];
  const int t = (int)blockIdx.x - (i == 0 ? 0 : b.it[i - 1].t3_end);
  const int rows = it.rows, cols = it.cols;
  const int lane = threadIdx.x & 63, row = t * SN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                                                   // (wave-uniform; no barrier below)
  const float* __restrict__ w = it.w + (int64_t)row * cols;
  const float* __restrict__ v = it.v;
  float acc = 0.f;
  if (sn_al16(it.w) && sn_al16(v) && (cols & 3) == 0) {
#pragma unroll 4
    for (int j = lane * 4; j < cols; j += 256) {
      const float4 x = *reinterpret_cast<const float4*>(w + j);
      const float4 y = *reinterpret_cast<const float4*>(v + j);
      acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
    }
  } else {
    for (int j = lane * 4; j < cols; j += 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < cols) acc = fmaf(w[j + k], v[j + k], acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) ws[it.ws_off + (int64_t)sn_slabs(rows) * cols + row] = acc;
}

// What every workgroup of a layer derives from u' (and, without an update, u) in the same order, hence bit-identically:
// the denominator of u = u' / max(|u'|, eps) and sigma = u^T u'.
__device__ __forceinline__ void sn_sigma(const float* __restrict__ up, const float* __restrict__ u, int rows, int update, float eps,
                                         double* scratch, float& den, float& sigma) {
  den = 1.f;
  if (update) {
    double nrm = 0.0;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) nrm = fma((double)up[r], (double)up[r], nrm);
    den = fmaxf((float)sqrt(block_sum_d(nrm, scratch)), eps);
  }
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) s = fma((double)(update ? up[r] / den : u[r]), (double)up[r], s);
  sigma = (float)block_sum_d(s, scratch);
}

// stage 4 per (layer, chunk): W_sn = W / sigma; the layer's first workgroup also writes u and sigma[layer]
__global__ void __launch_bounds__(256) sn_scale_kernel(SnBatch b, const float* __restrict__ ws, float* __restrict__ sigma_out, int update,
                                                       float eps) {
  __shared__ double scratch[32];
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].ch_end) ++i;
  const SnItem& it = b.it[i];
  const int t = (int)blockIdx.x - (i == 0 ? 0 : b.it[i - 1].ch_end);
  const int rows = it.rows, cols = it.cols;
  const float* __restrict__ up = ws + it.ws_off + (int64_t)sn_slabs(rows) * cols;
  float den, sigma;
  sn_sigma(up, it.u, rows, update, eps, scratch, den, sigma);
  const int64_t n = (int64_t)rows * cols, e0 = (int64_t)t * SN_ELEMS;
  const float* __restrict__ w = it.w;
  float* __restrict__ o = it.wsn;
  if (sn_al16(w) && sn_al16(o)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t e = e0 + q * 1024 + threadIdx.x * 4;
      if (e + 3 < n) {
        float4 x = *reinterpret_cast<const float4*>(w + e);
        x.x /= sigma; x.y /= sigma; x.z /= sigma; x.w /= sigma;
        *reinterpret_cast<float4*>(o + e) = x;
      } else {
        for (int64_t k = e; k < n; ++k) o[k] = w[k] / sigma;
      }
    }
  } else {
    for (int q = 0; q < SN_ELEMS / 256; ++q) {
      const int64_t e = e0 + q * 256 + threadIdx.x;
      if (e < n) o[e] = w[e] / sigma;
    }
  }
  if (t == 0) {
    if (update) {
      float* __restrict__ u = it.u;
      for (int r = threadIdx.x; r < rows; r += 256) u[r] = up[r] / den;
    }
    if (threadIdx.x == 0) sigma_out[b.base + i] = sigma;
  }
}

// backward stage 1 per (layer, chunk): <g_sn, w_sn> over the chunk
__global__ void __launch_bounds__(256) sn_dot_kernel(SnBatch b, float* __restrict__ ws) {
  __shared__ double scratch[32];
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].ch_end) ++i;
  const SnItem& it = b.it[i];
  const int t = (int)blockIdx.x - (i == 0 ? 0 : b.it[i - 1].ch_end);
  const int rows = it.rows, cols = it.cols;
  const int64_t n = (int64_t)rows * cols, e0 = (int64_t)t * SN_ELEMS;
  const float* __restrict__ g = it.gsn;
  const float* __restrict__ w = it.wsn;
  float acc = 0.f;
  if (sn_al16(g) && sn_al16(w)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t e = e0 + q * 1024 + threadIdx.x * 4;
      if (e + 3 < n) {
        const float4 x = *reinterpret_cast<const float4*>(g + e);
        const float4 y = *reinterpret_cast<const float4*>(w + e);
        acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
      } else {
        for (int64_t k = e; k < n; ++k) acc = fmaf(g[k], w[k], acc);
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t e = e0 + q * 1024 + threadIdx.x * 4;
      for (int64_t k = e; k < e + 4 && k < n; ++k) acc = fmaf(g[k], w[k], acc);
    }
  }
  const double s = block_sum_d((double)acc, scratch);
  if (threadIdx.x == 0) ws[it.ws_off + (int64_t)sn_slabs(rows) * cols + rows + t] = (float)s;
}

// backward stage 2 per (layer, chunk): d = the layer's partials in order; g_orig += (g_sn - d u v^T) / sigma; clear: g_sn = 0
__global__ void __launch_bounds__(256) sn_apply_kernel(SnBatch b, const float* __restrict__ ws, const float* __restrict__ sigma_in, int clear) {
  __shared__ double scratch[32];
  int i = 0;
  while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].ch_end) ++i;
  const SnItem& it = b.it[i];
  const int t = (int)blockIdx.x - (i == 0 ? 0 : b.it[i - 1].ch_end);
  const int rows = it.rows, cols = it.cols, nchunks = sn_chunks(rows, cols);
  const float* __restrict__ dots = ws + it.ws_off + (int64_t)sn_slabs(rows) * cols + rows;
  double dd = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += 256) dd += (double)dots[c];
  const float d = (float)block_sum_d(dd, scratch);
  const float sigma = sigma_in[b.base + i];
  const int64_t n = (int64_t)rows * cols, e0 = (int64_t)t * SN_ELEMS;
  float* __restrict__ g = it.gsn;
  float* __restrict__ o = it.gorig;
  const float* __restrict__ u = it.u;
  const float* __restrict__ v = it.v;
  if (sn_al16(g) && sn_al16(o) && (cols & 3) == 0) {           // four elements of a float4 share a row
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t e = e0 + q * 1024 + threadIdx.x * 4;
      if (e < n) {
        const int r = (int)(e / cols), j = (int)(e - (int64_t)r * cols);
        const float du = d * u[r];
        const float4 x = *reinterpret_cast<const float4*>(g + e);
        float4 y = *reinterpret_cast<const float4*>(o + e);
        y.x += fmaf(-du, v[j], x.x) / sigma; y.y += fmaf(-du, v[j + 1], x.y) / sigma;
        y.z += fmaf(-du, v[j + 2], x.z) / sigma; y.w += fmaf(-du, v[j + 3], x.w) / sigma;
        *reinterpret_cast<float4*>(o + e) = y;
        if (clear) *reinterpret_cast<float4*>(g + e) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  } else {
    for (int q = 0; q < SN_ELEMS / 256; ++q) {
      const int64_t e = e0 + q * 256 + threadIdx.x;
      if (e < n) {
        const int r = (int)(e / cols), j = (int)(e - (int64_t)r * cols);
        o[e] += fmaf(-(d * u[r]), v[j], g[e]) / sigma;
        if (clear) g[e] = 0.f;
      }
    }
  }
}

// ---- host side: the table, checked and laid out before anything is launched
struct SnPlan { int t1, t3, ch; };
static inline int64_t sn_item_floats(int64_t rows, int64_t cols) {
  const int64_t f = ((rows + SN_SLAB - 1) / SN_SLAB) * cols + rows + (rows * cols + SN_ELEMS - 1) / SN_ELEMS;
  return (f + 3) / 4 * 4;
}
// -> TG_OK / TG_EINVAL / TG_EUNSUPPORTED; *floats = the workspace of all items
static int sn_check(const tg_host_i64* items, int n_items, int need_grads, int64_t* floats) {
  if (n_items < 1 || items == nullptr) return TG_EINVAL;
  int64_t total = 0;
  for (int i = 0; i < n_items; ++i) {
    const tg_host_i64* it = items + (size_t)i * TG_SN_ITEM_FIELDS;
    for (int f = 0; f < 6; ++f) {
      if (it[f] == 0 && (f < 4 || need_grads)) return TG_EINVAL;
      if (it[f] & 3) return TG_EINVAL;
    }
    if (it[6] < 1 || it[7] < 1) return TG_EINVAL;
  }
  for (int i = 0; i < n_items; ++i) {
    const tg_host_i64* it = items + (size_t)i * TG_SN_ITEM_FIELDS;
    if (it[6] >= (1ll << 31) || it[7] >= (1ll << 31) || it[6] * it[7] >= (1ll << 31)) return TG_EUNSUPPORTED;
    total += sn_item_floats(it[6], it[7]);
    if (total >= (1ll << 31)) return TG_EUNSUPPORTED;
  }
  *floats = total;
  return TG_OK;
}
// the group of at most SN_MAX_ITEMS layers that starts at `base`; ws_off continues from *off
static SnPlan sn_group(const tg_host_i64* items, int n_items, int base, int64_t* off, SnBatch* b) {
  SnPlan p{0, 0, 0};
  b->n = n_items - base < SN_MAX_ITEMS ? n_items - base : SN_MAX_ITEMS;
  b->base = base;
  for (int i = 0; i < b->n; ++i) {
    const tg_host_i64* it = items + (size_t)(base + i) * TG_SN_ITEM_FIELDS;
    const int rows = (int)it[6], cols = (int)it[7];
    p.t1 += ((rows + SN_SLAB - 1) / SN_SLAB) * ((cols + SN_COLS - 1) / SN_COLS);
    p.t3 += (rows + SN_WAVES - 1) / SN_WAVES;
    p.ch += (int)(((int64_t)rows * cols + SN_ELEMS - 1) / SN_ELEMS);
    b->it[i] = SnItem{reinterpret_cast<const float*>(it[0]), reinterpret_cast<float*>(it[1]), reinterpret_cast<float*>(it[2]),
                      reinterpret_cast<float*>(it[3]), reinterpret_cast<float*>(it[4]), reinterpret_cast<float*>(it[5]),
                      rows, cols, p.t1, p.t3, p.ch, (int)*off};
    *off += sn_item_floats(rows, cols);
  }
  for (int i = b->n; i < SN_MAX_ITEMS; ++i) b->it[i] = b->it[0];
  return p;
}

}  // namespace

extern "C" {

int tg_sn_power_iter(const float* W, float* u, float* v, float* sigma, int rows, int cols, int n_iter, float eps, void* stream) {
  TG_CHECK_PTR(W); TG_CHECK_PTR(u); TG_CHECK_PTR(v);
  TG_CHECK_POS(rows); TG_CHECK_POS(cols);
  if (n_iter < 0) return TG_EINVAL;
  sn_power_iter_kernel<<<1, SNB, 0, tg_stream(stream)>>>(W, u, v, sigma, rows, cols, n_iter, eps);
  return tg_launch_status();
}

int tg_recip(const float* x, float* out, int64_t n, void* stream) {
  TG_CHECK_PTR(x); TG_CHECK_PTR(out);
  if (n <= 0) return TG_EINVAL;
  recip_kernel<<<tg_ew_grid(n, 256), 256, 0, tg_stream(stream)>>>(x, out, n);
  return tg_launch_status();
}

size_t tg_sn_batch_workspace(const tg_host_i64* items, int n_items) {
  int64_t floats = 0;
  return sn_check(items, n_items, 0, &floats) == TG_OK ? (size_t)floats * sizeof(float) : 0;
}

int tg_sn_batch_fwd(const tg_host_i64* items, int n_items, float* sigma, float* workspace, size_t workspace_bytes, int update, float eps,
                    void* stream) {
  int64_t floats = 0;
  if (int rc = sn_check(items, n_items, 0, &floats)) return rc;
  TG_CHECK_PTR(sigma); TG_CHECK_PTR(workspace);
  if (workspace_bytes < (size_t)floats * sizeof(float)) return TG_EWORKSPACE;
  hipStream_t st = tg_stream(stream);
  int64_t off = 0;
  for (int base = 0; base < n_items; base += SN_MAX_ITEMS) {
    SnBatch b;
    const SnPlan p = sn_group(items, n_items, base, &off, &b);
    if (update) {
      sn_wtu_kernel<<<p.t1, 256, 0, st>>>(b, workspace);
      sn_v_kernel<<<b.n, 1024, 0, st>>>(b, workspace, eps);
    }
    sn_wv_kernel<<<p.t3, 64 * SN_WAVES, 0, st>>>(b, workspace);
    sn_scale_kernel<<<p.ch, 256, 0, st>>>(b, workspace, sigma, update, eps);
  }
  return tg_launch_status();
}

int tg_sn_batch_bwd(const tg_host_i64* items, int n_items, const float* sigma, float* workspace, size_t workspace_bytes, int clear,
                    void* stream) {
  int64_t floats = 0;
  if (int rc = sn_check(items, n_items, 1, &floats)) return rc;
  TG_CHECK_PTR(sigma); TG_CHECK_PTR(workspace);
  if (workspace_bytes < (size_t)floats * sizeof(float)) return TG_EWORKSPACE;
  hipStream_t st = tg_stream(stream);
  int64_t off = 0;
  for (int base = 0; base < n_items; base += SN_MAX_ITEMS) {
    SnBatch b;
    const SnPlan p = sn_group(items, n_items, base, &off, &b);
    sn_dot_kernel<<<p.ch, 256, 0, st>>>(b, workspace);
    sn_apply_kernel<<<p.ch, 256, 0, st>>>(b, workspace, sigma, clear);
  }
  return tg_launch_status();
}

}  // extern "C"
