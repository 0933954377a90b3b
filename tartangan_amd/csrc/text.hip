// The text trainer's embedding side on gfx950: the fused skip-gram step (models/text.py:42-55 + its sparse backward,
// coalesce and torch.optim.SGD, trainers/text_cnn.py:162-182), embedding(x).permute(0, 2, 1) and SkipGram.lookup.
//
// tg_skipgram_step is two launches over tables that are updated IN PLACE, arranged so that neither launch reads a table
// element another workgroup may already have updated:
//   1. sg_scores_kernel, one wave per batch row b: u = U[w_b]; for every context / negative j the score V[.] . u, its
//      log-sigmoid term and the score gradient (-sigmoid(-s) / B, sigmoid(s) / B).  It leaves in the workspace the row's loss,
//      the 2 C2 score gradients, a COPY of u and the finished gradient of u (sum_j coefficient * V row): everything launch 2
//      needs from the tables as they were on entry.
//   2. sg_update_kernel, one wave per index slot (B word slots for U; 2 B C2 context-then-negative slots for V) plus one for
//      the loss.  A wave walks its table's slot list in order; if an EARLIER slot names the same row it is not the owner and
//      leaves, otherwise it sums the contributions of every slot naming its row in slot order -- the reference's
//      coalesce -- and applies T[r] -= lr * g[r].  Every row has exactly one writer, which reads only its own row and the
//      workspace.  Rows equal to padding_idx have no owner; rows no index names are never touched.
// No atomics, fixed summation orders: bit-identical from run to run.
// An index outside [0, vocab) is never dereferenced: its row reads as zeros and gets no update (the reference raises
// instead; models/text.py of this package checks the indexes on the host, where they come from).
#include "common.h"

namespace {

constexpr int SG_MAXE = 1024, SG_MAXSLOTS = 1 << 16;

__device__ __forceinline__ float sg_logsigmoid(float s) { return fminf(s, 0.f) - log1pf(expf(-fabsf(s))); }
__device__ __forceinline__ float sg_sigmoid(float s) {
  const float e = expf(-fabsf(s));
  return s >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

struct SgWs {      // views into the workspace
  float* lossb;    // [B]
  float* coef;     // [2][B * C2]: contexts, then negatives
  float* ucopy;    // [B][E]
  float* du;       // [B][E]
};
__host__ __device__ inline SgWs sg_ws(float* ws, int B, int C2, int E) {
  SgWs v;
  v.lossb = ws;
  v.coef = ws + B;
  v.ucopy = v.coef + 2 * (int64_t)B * C2;
  v.du = v.ucopy + (int64_t)B * E;
  return v;
}

// NQ: 64-wide chunks of E a lane holds (E <= 64 NQ); the host picks the smallest of 1, 2, 4, 8, 16
template <int NQ>
__global__ void __launch_bounds__(64)
sg_scores_kernel(const float* __restrict__ U, const float* __restrict__ V, const int64_t* __restrict__ words,
                 const int64_t* __restrict__ contexts, const int64_t* __restrict__ negatives, float* ws, int B, int C2, int E, int vocab) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const SgWs w = sg_ws(ws, B, C2, E);
  const int64_t wi = words[b];
  const float* urow = ((uint64_t)wi < (uint64_t)vocab) ? U + wi * E : nullptr;
  float u[NQ], g[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = lane + 64 * q;
    u[q] = (urow && e < E) ? urow[e] : 0.f;
    g[q] = 0.f;
  }
  float loss = 0.f;
  for (int half = 0; half < 2; ++half) {
    const int64_t* idx = half ? negatives : contexts;
    for (int j = 0; j < C2; ++j) {
      const int64_t vi = idx[(int64_t)b * C2 + j];
      const float* vrow = ((uint64_t)vi < (uint64_t)vocab) ? V + vi * E : nullptr;
      float v[NQ], dot = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int e = lane + 64 * q;
        v[q] = (vrow && e < E) ? vrow[e] : 0.f;
        dot += v[q] * u[q];
      }
      const float s = wave_sum(dot);
      // -(log sigmoid(s)) for a context, -(log sigmoid(-s)) for a negative; d/ds = -sigmoid(-s) and sigmoid(s)
      loss -= half ? sg_logsigmoid(-s) : sg_logsigmoid(s);
      const float c = (half ? sg_sigmoid(s) : -sg_sigmoid(-s)) / (float)B;
      if (lane == 0) w.coef[(int64_t)half * B * C2 + (int64_t)b * C2 + j] = c;
#pragma unroll
      for (int q = 0; q < NQ; ++q) g[q] += c * v[q];
    }
  }
  if (lane == 0) w.lossb[b] = loss;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = lane + 64 * q;
    if (e < E) {
      w.ucopy[(int64_t)b * E + e] = u[q];
      w.du[(int64_t)b * E + e] = g[q];
    }
  }
}

template <int NQ>
__global__ void __launch_bounds__(64)
sg_update_kernel(float* U, float* V, const int64_t* __restrict__ words, const int64_t* __restrict__ contexts,
                 const int64_t* __restrict__ negatives, float lr, int64_t padding_idx, float* loss_out, const float* ws, int B, int C2,
                 int E, int vocab) {
  const int lane = threadIdx.x;
  const SgWs w = sg_ws(const_cast<float*>(ws), B, C2, E);
  const int nv = 2 * B * C2;
  int slot = blockIdx.x;
  if (slot == B + nv) {                                 // the loss: rows in order, one lane chain per 64, fixed tree
    float s = 0.f;
    for (int b = lane; b < B; b += 64) s += w.lossb[b];
    s = wave_sum(s);
    if (lane == 0) loss_out[0] = s / (float)B;
    return;
  }
  const bool isu = slot < B;
  if (!isu) slot -= B;
  const int nslots = isu ? B : nv;
  auto index_of = [&](int p) -> int64_t { return isu ? words[p] : (p < B * C2 ? contexts[p] : negatives[p - B * C2]); };
  const int64_t r = index_of(slot);
  if ((uint64_t)r >= (uint64_t)vocab || r == padding_idx) return;
  float acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
  for (int p0 = 0; p0 < nslots; p0 += 64) {
    const int p = p0 + lane;
    const bool hit = p < nslots && index_of(p) == r;
    unsigned long long m = __ballot(hit);
    if (p0 <= slot && (m & ((p0 + 64 <= slot) ? ~0ull : ((1ull << (slot - p0)) - 1ull)))) return;   // an earlier slot owns the row
    while (m) {
      const int q0 = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int pp = p0 + q0;
      const float* src;
      float c;
      if (isu) { src = w.du + (int64_t)pp * E; c = 1.f; }
      else { src = w.ucopy + (int64_t)((pp % (B * C2)) / C2) * E; c = w.coef[pp]; }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int e = lane + 64 * q;
        if (e < E) acc[q] += c * src[e];
      }
    }
  }
  float* row = (isu ? U : V) + r * E;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int e = lane + 64 * q;
    if (e < E) row[e] -= lr * acc[q];
  }
}

// out[b][e][l] = U[idx[b][l]][e]: a 32 (tokens) x 32 (dims) tile through LDS; rows are read along e, written along l
__global__ void __launch_bounds__(256)
embed_gather_t_kernel(const float* __restrict__ U, const int64_t* __restrict__ idx, float* __restrict__ out, int L, int E, int vocab,
                      int tl, int te) {
  __shared__ float tile[32][33];
  const int bid = blockIdx.x, b = bid / (tl * te), rem = bid - b * (tl * te), l0 = (rem / te) * 32, e0 = (rem % te) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int l = l0 + ty + 8 * v, e = e0 + tx;
    float val = 0.f;
    if (l < L && e < E) {
      const int64_t r = idx[(int64_t)b * L + l];
      if ((uint64_t)r < (uint64_t)vocab) val = U[r * E + e];
    }
    tile[ty + 8 * v][tx] = val;
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = e0 + ty + 8 * v, l = l0 + tx;
    if (l < L && e < E) out[((int64_t)b * E + e) * L + l] = tile[tx][ty + 8 * v];
  }
}

// SkipGram.lookup (models/text.py:57-69): one workgroup per column z[b, :, l]; thread t scores rows 1 + t, 1 + t + 256, ...
__global__ void __launch_bounds__(256)
embed_lookup_kernel(const float* __restrict__ U, const float* __restrict__ z, int64_t* __restrict__ out, int L, int E, int vocab) {
  __shared__ float zc[SG_MAXE];
  __shared__ float bs[256];
  __shared__ int bi[256];
  const int col = blockIdx.x, b = col / L, l = col - b * L, tid = threadIdx.x;
  for (int e = tid; e < E; e += 256) zc[e] = z[((int64_t)b * E + e) * L + l];
  __syncthreads();
  float best = 0.f;
  int besti = -1;
  for (int i = 1 + tid; i < vocab; i += 256) {
    const float* row = U + (int64_t)i * E;
    float dot = 0.f, sq = 0.f;
    for (int e = 0; e < E; ++e) { const float w = row[e]; dot += w * zc[e]; sq += w * w; }
    const float s = dot / sqrtf(sq);
    // the first maximum; NaN (a zero row) counts as the largest value, as torch.argmax has it
    if (besti < 0 || (s > best) || (s != s && best == best)) { best = s; besti = i; }
  }
  bs[tid] = best;
  bi[tid] = besti;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) {
      if (bi[t] < 0) continue;
      const float s = bs[t];
      const bool better = besti < 0 || (s > best) || (s != s && best == best) || (s == best && bi[t] < besti) ||
                          (s != s && best != best && bi[t] < besti);
      if (better) { best = s; besti = bi[t]; }
    }
    out[col] = besti - 1;                               // the reference's quirk: the index counts from row 1
  }
}

template <int NQ>
int sg_launch(float* U, float* V, const int64_t* words, const int64_t* contexts, const int64_t* negatives, float lr, int padding_idx,
              float* loss_out, float* workspace, int B, int C2, int E, int vocab, hipStream_t st) {
  sg_scores_kernel<NQ><<<B, 64, 0, st>>>(U, V, words, contexts, negatives, workspace, B, C2, E, vocab);
  const int rc = tg_launch_status();
  if (rc != TG_OK) return rc;
  sg_update_kernel<NQ><<<B + 2 * B * C2 + 1, 64, 0, st>>>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab);
  return tg_launch_status();
}

bool sg_shape_ok(int B, int C2, int E) { return E <= SG_MAXE && 2 * (int64_t)B * C2 <= SG_MAXSLOTS; }

}  // namespace

extern "C" {

size_t tg_skipgram_workspace(int B, int C2, int E) {
  if (B <= 0 || C2 <= 0 || E <= 0 || !sg_shape_ok(B, C2, E)) return 0;
  return ((size_t)B + 2 * (size_t)B * C2 + 2 * (size_t)B * E) * sizeof(float);
}

int tg_skipgram_step(float* U, float* V, const int64_t* words, const int64_t* contexts, const int64_t* negatives, float lr,
                     int padding_idx, float* loss_out, float* workspace, size_t workspace_bytes, int B, int C2, int E, int vocab,
                     void* stream) {
  TG_CHECK_PTR(U); TG_CHECK_PTR(V); TG_CHECK_PTR(words); TG_CHECK_PTR(contexts); TG_CHECK_PTR(negatives); TG_CHECK_PTR(loss_out);
  TG_CHECK_PTR(workspace);
  TG_CHECK_POS(B); TG_CHECK_POS(C2); TG_CHECK_POS(E); TG_CHECK_POS(vocab);
  if (U == V) return TG_EINVAL;
  if (!sg_shape_ok(B, C2, E) || (int64_t)vocab * E >= (1ll << 40)) return TG_EUNSUPPORTED;
  if (workspace_bytes < tg_skipgram_workspace(B, C2, E)) return TG_EWORKSPACE;
  hipStream_t st = tg_stream(stream);
  return E <= 64    ? sg_launch<1>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab, st)
         : E <= 128 ? sg_launch<2>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab, st)
         : E <= 256 ? sg_launch<4>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab, st)
         : E <= 512 ? sg_launch<8>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab, st)
                    : sg_launch<16>(U, V, words, contexts, negatives, lr, padding_idx, loss_out, workspace, B, C2, E, vocab, st);
}

int tg_embed_gather_t(const float* U, const int64_t* idx, float* out, int B, int L, int E, int vocab, void* stream) {
  TG_CHECK_PTR(U); TG_CHECK_PTR(idx); TG_CHECK_PTR(out);
  TG_CHECK_POS(B); TG_CHECK_POS(L); TG_CHECK_POS(E); TG_CHECK_POS(vocab);
  const int tl = (L + 31) / 32, te = (E + 31) / 32;
  if ((int64_t)B * tl * te >= (1ll << 31) - 1) return TG_EUNSUPPORTED;
  embed_gather_t_kernel<<<B * tl * te, 256, 0, tg_stream(stream)>>>(U, idx, out, L, E, vocab, tl, te);
  return tg_launch_status();
}

int tg_embed_lookup(const float* U, const float* z, int64_t* out, int B, int L, int E, int vocab, void* stream) {
  TG_CHECK_PTR(U); TG_CHECK_PTR(z); TG_CHECK_PTR(out);
  TG_CHECK_POS(B); TG_CHECK_POS(L); TG_CHECK_POS(E);
  if (vocab < 2) return TG_EINVAL;
  if (E > SG_MAXE || (int64_t)B * L >= (1ll << 31) - 1) return TG_EUNSUPPORTED;
  embed_lookup_kernel<<<B * L, 256, 0, tg_stream(stream)>>>(U, z, out, L, E, vocab);
  return tg_launch_status();
}

}  // extern "C"
