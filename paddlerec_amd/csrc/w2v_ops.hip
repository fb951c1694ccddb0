// word2vec (models/recall/word2vec), skip-gram with negative sampling, on gfx950: the model's own hot path.
//
//   rec_w2v_sgns_fwd_bwd   <- word2vec/net.py:57-81 Word2VecLayer.forward and dygraph_model.py:53-69 create_loss: the three
//                             lookups, the 1 + neg dots, sigmoid then BCE on probabilities (two stages, Paddle's clamps),
//                             g = d loss / d logit and d_in = sum_j g_j emb_w[target_j] in ONE launch, then the loss fold
//   rec_w2v_target_update  <- the SGD step (dygraph_model.py:72-76) of embedding_w / embedding_b: the gradient of a target
//                             row, sum_k g[pos_k] emb[in_ids[b_k]], is formed from g and the input table WHILE it is
//                             reduced; the [B, 1 + neg, D] gradient of the torch chain is never written
//   rec_w2v_analogy_topk   <- net.py:100-110 Word2VecInferLayer.forward: target = e_b - e_a + e_c, every vocabulary row
//                             divided by max(|row|, 1e-12), the scores and the top k, without the [Q, V] matrix
//
// Mapping.  fwd_bwd gives one 64-lane WAVE to a sample, four samples to a block.  A lane owns the column chunks lane,
// lane + 64, ... (VEC floats each) of its sample's rows; the input row, the target row in flight and the d_in accumulator
// live in the wave's slice of dynamic LDS, and a lane only ever reads what it wrote there itself, so the kernel has no
// barrier.  Every global row is read once.  A dot is the lane's partial in ascending column order, then an xor butterfly.
// The loss is folded by a second, single-block kernel of the same entry that evaluates the loss terms again from the
// logits just written: thread t sums the terms t, t + 1024, ... in ascending order, then a fixed tree over LDS.
//
// target_update runs two kernels over the grouping of target_ids.  A segment of at most kLongSeg occurrences is one wave's
// loop in ascending order (its g and input ids are loaded once, one per lane, and broadcast by shuffles).  A longer one
// (the reference reader hands every sample the SAME negatives: neg rows with B occurrences each) is cut into column slices
// of kSliceLanes chunks, one 1024-thread block per (row, slice): occurrence i goes to partial i % 64 (16 waves x 4 lane
// groups), each partial adds its occurrences in ascending order, the 4 groups of a wave fold by two xor steps and the 16
// waves in ascending order over LDS.  One block owns a (row, slice), so no float atomics and no scratch buffer.  The blocks
// find the long rows themselves: a block scans 1024 unique rows a step, a thread each, and kLongSplit z-blocks share what
// a step finds (row u goes to z-block u % kLongSplit), so hot rows that are neighbours in the sorted order run side by side.
//
// analogy_topk: a block takes one tile of REC_W2V_TOPK_TILE_ROWS vocabulary rows and walks ALL queries, 64 at a time, as a
// register-tiled product (8 rows x 4 queries per thread, 32-column steps staged through LDS; the query vectors are built
// from the three rows while they are staged, the rows divided by their norm), then picks its k best per query; a second kernel merges the tiles'
// candidates, one wave per query.  Order everywhere: higher score first, equal scores by lower id.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kLongSeg = 16;       // occurrences above which a target row takes the block-per-slice kernel
constexpr int kSliceLanes = 16;    // column chunks of one slice of that kernel
constexpr int kLongBlock = 1024;
constexpr int kLongSplit = 4;     // z-blocks that share the long rows of one scan step
constexpr int kFoldBlock = 1024;
constexpr int kTile = REC_W2V_TOPK_TILE_ROWS;
constexpr int kQTile = 64;         // queries of one pass of the search
constexpr int kDK = 32;            // columns staged per step
constexpr int kLdR = kTile + 1, kLdQ = kQTile + 1, kLdS = kTile + 1;

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  return x;
}

// dygraph_model.py:60-66 for one logit: p = sigmoid(z), then BCE on the probability with Paddle's clamps [EXT]: the log at
// -100, the backward's denominator at 1e-12.  y is 1 for the true column and 0 for a negative.
__device__ __forceinline__ float sgns_prob(const float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float sgns_loss(const float p, const bool is_true) {
  return -fmaxf(logf(is_true ? p : 1.f - p), -100.f);
}
__device__ __forceinline__ float sgns_grad(const float p, const bool is_true, const float scale) {
  const float y = is_true ? 1.f : 0.f;
  return (p - y) / fmaxf((1.f - p) * p, 1e-12f) * scale * (1.f - p) * p;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void w2v_sgns_kernel(const int64_t batch, const int D, const int neg, const int64_t V,
                                                          const int per_wave, const int64_t* in_ids, const int64_t* target_ids,
                                                          const float* emb, const int64_t ld_emb, const float* emb_w,
                                                          const int64_t ld_w, const float* emb_b, const int64_t ld_b,
                                                          const float scale_true, const float scale_neg, float* true_logits,
                                                          float* neg_logits, float* g, float* d_in, const int64_t ld_din,
                                                          int32_t* status) {
  extern __shared__ __align__(16) float smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int64_t b = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (b >= batch) return;                             // no barrier below
  const int Dp = per_wave / 3;
  float* sx = smem + (size_t)wave * per_wave;         // the input row | the target row in flight | d_in
  float* sw = sx + Dp;
  float* sa = sw + Dp;
  const int chunks = D / VEC;
  const int64_t in = in_ids[b];
  const bool in_ok = in >= 0 && in < V;
  bool bad = !in_ok;
  for (int c = lane; c < chunks; c += kWave) {
    float x[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[v] = 0.f;
    if (in_ok) vload<VEC>(x, emb + in * ld_emb + (int64_t)c * VEC);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      sx[c * VEC + v] = x[v];
      sa[c * VEC + v] = 0.f;
    }
  }
  const int tw = 1 + neg;
  for (int j = 0; j < tw; ++j) {
    const int64_t t = target_ids[b * tw + j];
    const bool t_ok = t >= 0 && t < V;
    bad |= !t_ok;
    const bool ok = in_ok && t_ok;                    // wave-uniform
    float dot = 0.f;
    if (ok)
      for (int c = lane; c < chunks; c += kWave) {
        float w[VEC];
        vload<VEC>(w, emb_w + t * ld_w + (int64_t)c * VEC);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          dot += sx[c * VEC + v] * w[v];
          sw[c * VEC + v] = w[v];
        }
      }
    dot = wave_sum(dot);
    float z = 0.f, gj = 0.f;
    if (ok) {
      z = dot + emb_b[t * ld_b];
      gj = sgns_grad(sgns_prob(z), j == 0, j == 0 ? scale_true : scale_neg);
      for (int c = lane; c < chunks; c += kWave)
#pragma unroll
        for (int v = 0; v < VEC; ++v) sa[c * VEC + v] += gj * sw[c * VEC + v];
    }
    if (lane == 0) {
      if (j == 0)
        true_logits[b] = z;
      else
        neg_logits[b * neg + (j - 1)] = z;
      g[b * tw + j] = gj;
    }
  }
  for (int c = lane; c < chunks; c += kWave) {
    float a[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) a[v] = sa[c * VEC + v];
    vstore<VEC>(d_in + b * ld_din + (int64_t)c * VEC, a);
  }
  if (bad && lane == 0 && status) atomicOr(status, REC_FLAG_INDEX_OOB);
}

// loss = mean over B of the true terms + mean over B neg of the negative terms, the terms evaluated again from the logits
__global__ __launch_bounds__(kFoldBlock) void w2v_loss_fold_kernel(const int64_t batch, const int neg, const int64_t V,
                                                                   const int64_t* in_ids, const int64_t* target_ids,
                                                                   const float* true_logits, const float* neg_logits,
                                                                   float* loss) {
  __shared__ float st[kFoldBlock], sn[kFoldBlock];
  const int tw = 1 + neg;
  const int64_t n = batch * tw;
  float at = 0.f, an = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kFoldBlock) {
    const int64_t b = i / tw;
    const int j = (int)(i - b * tw);
    const int64_t in = in_ids[b], t = target_ids[i];
    if (in < 0 || in >= V || t < 0 || t >= V) continue;
    if (j == 0)
      at += sgns_loss(sgns_prob(true_logits[b]), true);
    else
      an += sgns_loss(sgns_prob(neg_logits[b * neg + (j - 1)]), false);
  }
  st[threadIdx.x] = at;
  sn[threadIdx.x] = an;
  __syncthreads();
  for (int o = kFoldBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      st[threadIdx.x] += st[threadIdx.x + o];
      sn[threadIdx.x] += sn[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = st[0] / (float)batch + sn[0] / ((float)batch * (float)neg);
}

// segments of at most kLongSeg occurrences: one wave per unique row, occurrences in ascending order
template <int VEC>
__global__ __launch_bounds__(kBlock) void w2v_update_short_kernel(const int64_t n, const int D, const int tw, const int64_t V,
                                                                  const int32_t* n_uniq, const int64_t* uniq_rows,
                                                                  const int32_t* seg_offset, const int32_t* sorted_pos,
                                                                  const float* g, const int64_t* in_ids, const float* emb,
                                                                  const int64_t ld_emb, float* emb_w, const int64_t ld_w,
                                                                  float* emb_b, const int64_t ld_b, const float lr,
                                                                  float* d_w_rows, const int64_t ld_dw, float* d_b_rows) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int64_t U = n_uniq[0] < n ? n_uniq[0] : n;
  const int chunks = D / VEC;
  for (int64_t u = (int64_t)blockIdx.x * (kBlock / kWave) + wave; u < U; u += (int64_t)gridDim.x * (kBlock / kWave)) {
    const int s0 = seg_offset[u], len = seg_offset[u + 1] - s0;
    const int64_t r = uniq_rows[u];
    if (len <= 0 || len > kLongSeg || r < 0 || r >= V) continue;             // wave-uniform
    float my_g = 0.f;
    long long my_in = -1;
    if (lane < len) {
      const int64_t pos = sorted_pos[s0 + lane];
      if (pos >= 0 && pos < n) {
        const int64_t in = in_ids[pos / tw];
        if (in >= 0 && in < V) {
          my_in = in;
          my_g = g[pos];
        }
      }
    }
    float gs = 0.f;
    for (int k = 0; k < len; ++k) gs += __shfl(my_g, k, kWave);
    for (int c0 = 0; c0 < chunks; c0 += kWave) {
      const int c = c0 + lane;
      const bool live = c < chunks;
      float acc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      for (int k = 0; k < len; ++k) {
        const float gk = __shfl(my_g, k, kWave);
        const long long in = __shfl(my_in, k, kWave);
        if (live && in >= 0) {
          float x[VEC];
          vload<VEC>(x, emb + in * ld_emb + (int64_t)c * VEC);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += gk * x[v];
        }
      }
      if (live) {
        float w[VEC];
        float* dst = emb_w + r * ld_w + (int64_t)c * VEC;
        vload<VEC>(w, dst);
#pragma unroll
        for (int v = 0; v < VEC; ++v) w[v] -= lr * acc[v];
        vstore<VEC>(dst, w);
        if (d_w_rows) vstore<VEC>(d_w_rows + u * ld_dw + (int64_t)c * VEC, acc);
      }
    }
    if (lane == 0) {
      emb_b[r * ld_b] -= lr * gs;
      if (d_b_rows) d_b_rows[u] = gs;
    }
  }
}

// longer segments: one block per (unique row, column slice); 64 partials folded in a fixed order
template <int VEC>
__global__ __launch_bounds__(kLongBlock) void w2v_update_long_kernel(const int64_t n, const int D, const int tw, const int64_t V,
                                                                     const int32_t* n_uniq, const int64_t* uniq_rows,
                                                                     const int32_t* seg_offset, const int32_t* sorted_pos,
                                                                     const float* g, const int64_t* in_ids, const float* emb,
                                                                     const int64_t ld_emb, float* emb_w, const int64_t ld_w,
                                                                     float* emb_b, const int64_t ld_b, const float lr,
                                                                     float* d_w_rows, const int64_t ld_dw, float* d_b_rows) {
  constexpr int kWaves = kLongBlock / kWave, kSubs = kWave / kSliceLanes;
  __shared__ float sp[kWaves][kSliceLanes * VEC];
  __shared__ float sg[kWaves];
  __shared__ int s_cnt, s_list[kLongBlock];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int sub = lane / kSliceLanes, cl = lane % kSliceLanes;
  const int col = ((int)blockIdx.y * kSliceLanes + cl) * VEC;
  const bool live = col < D;                          // D % VEC == 0: a live chunk is whole
  const int64_t U = n_uniq[0] < n ? n_uniq[0] : n;
  // the block scans kLongBlock unique rows a step, a thread each, and lists the long ones that are its own: row u belongs to
  // the z-block u % gridDim.z, so hot rows that are neighbours in the sorted order spread over the z-blocks
  for (int64_t base = (int64_t)blockIdx.x * kLongBlock; base < U; base += (int64_t)gridDim.x * kLongBlock) {
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    {
      const int64_t u = base + threadIdx.x;
      if (u < U && u % gridDim.z == blockIdx.z && seg_offset[u + 1] - seg_offset[u] > kLongSeg) {
        const int64_t r = uniq_rows[u];
        if (r >= 0 && r < V) s_list[atomicAdd(&s_cnt, 1)] = (int)threadIdx.x;      // the list's order changes no result
      }
    }
    __syncthreads();
    const int cnt = s_cnt;
    for (int e = 0; e < cnt; ++e) {
    const int64_t u = base + s_list[e];
    const int s0 = seg_offset[u], s1 = seg_offset[u + 1];
    const int64_t r = uniq_rows[u];
    float acc[VEC], gs = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    for (int k = s0 + wave * kSubs + sub; k < s1; k += kWaves * kSubs) {
      const int64_t pos = sorted_pos[k];
      float gk = 0.f;
      int64_t in = -1;
      if (pos >= 0 && pos < n) {
        in = in_ids[pos / tw];
        if (in >= 0 && in < V) gk = g[pos];
      }
      if (in >= 0 && in < V) {
        gs += gk;
        if (live) {
          float x[VEC];
          vload<VEC>(x, emb + in * ld_emb + col);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += gk * x[v];
        }
      }
    }
#pragma unroll
    for (int o = kSliceLanes; o < kWave; o <<= 1) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o, kWave);
      gs += __shfl_xor(gs, o, kWave);
    }
    if (sub == 0) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) sp[wave][cl * VEC + v] = acc[v];
      if (cl == 0) sg[wave] = gs;
    }
    __syncthreads();
    if (wave == 0 && sub == 0) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = sp[0][cl * VEC + v];
      gs = sg[0];
      for (int w = 1; w < kWaves; ++w) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += sp[w][cl * VEC + v];
        gs += sg[w];
      }
      if (live) {
        float w[VEC];
        float* dst = emb_w + r * ld_w + col;
        vload<VEC>(w, dst);
#pragma unroll
        for (int v = 0; v < VEC; ++v) w[v] -= lr * acc[v];
        vstore<VEC>(dst, w);
        if (d_w_rows) vstore<VEC>(d_w_rows + u * ld_dw + col, acc);
      }
      if (blockIdx.y == 0 && cl == 0) {
        emb_b[r * ld_b] -= lr * gs;
        if (d_b_rows) d_b_rows[u] = gs;
      }
    }
    __syncthreads();
    }
    __syncthreads();                                  // s_cnt and s_list are free again
  }
}

// (s, i) comes before (s2, i2): the higher score, equal scores by the lower id
__device__ __forceinline__ bool before(const float s, const int64_t i, const float s2, const int64_t i2) {
  return s > s2 || (s == s2 && i < i2);
}

// one tile of kTile vocabulary rows against all queries -> the tile's k candidates per query
template <int VEC>
__global__ __launch_bounds__(kBlock) void w2v_topk_tile_kernel(const int64_t Q, const int D, const int64_t ld, const int64_t V,
                                                               const int k, const int64_t* ida, const int64_t* idb,
                                                               const int64_t* idc, const float* W, float* cand_values,
                                                               int64_t* cand_ids, int32_t* status) {
  constexpr int kStage = kDK * kLdR + kDK * kLdQ, kScore = kQTile * kLdS;
  __shared__ float sm[kStage > kScore ? kStage : kScore];
  __shared__ float s_norm[kTile];
  float* sR = sm;                                     // [kDK][kLdR]: column d of the tile's rows
  float* sQ = sm + kDK * kLdR;                        // [kDK][kLdQ]: column d of the pass's query vectors
  float* sS = sm;                                     // [kQTile][kLdS]: the pass's scores (after the product)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (kWave - 1);
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  // |row| of the tile's rows: a wave per row, lanes over the columns in ascending order, then a butterfly
  for (int r = wave; r < kTile; r += kBlock / kWave) {
    const int64_t row = row0 + r;
    float s = 0.f;
    if (row < V)
      for (int d = lane; d < D; d += kWave) {
        const float x = W[row * ld + d];
        s += x * x;
      }
    s = wave_sum(s);
    if (lane == 0) s_norm[r] = fmaxf(sqrtf(s), 1e-12f);
  }
  bool bad = false;
  for (int64_t q0 = 0; q0 < Q; q0 += kQTile) {
    float acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += kDK) {
      __syncthreads();                                // the last step's (or pass's) readers are done
      constexpr int kPer = kDK / VEC;                 // chunks of a staged row
      for (int i = tid; i < kTile * kPer; i += kBlock) {
        const int r = i / kPer, d = (i - r * kPer) * VEC;
        float x[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) x[v] = 0.f;
        if (row0 + r < V && d0 + d < D) vload<VEC>(x, W + (row0 + r) * ld + d0 + d);
        const float nr = s_norm[r];                   // net.py:107: the ROW is normalised, then multiplied
#pragma unroll
        for (int v = 0; v < VEC; ++v) sR[(d + v) * kLdR + r] = x[v] / nr;
      }
      for (int i = tid; i < kQTile * kPer; i += kBlock) {
        const int q = i / kPer, d = (i - q * kPer) * VEC;
        float t[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) t[v] = 0.f;
        if (q0 + q < Q && d0 + d < D) {
          const int64_t a = ida[q0 + q], b = idb[q0 + q], c = idc[q0 + q];
          float ea[VEC], eb[VEC], ec[VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v) ea[v] = eb[v] = ec[v] = 0.f;
          if (a >= 0 && a < V) vload<VEC>(ea, W + a * ld + d0 + d); else bad = true;
          if (b >= 0 && b < V) vload<VEC>(eb, W + b * ld + d0 + d); else bad = true;
          if (c >= 0 && c < V) vload<VEC>(ec, W + c * ld + d0 + d); else bad = true;
#pragma unroll
          for (int v = 0; v < VEC; ++v) t[v] = eb[v] - ea[v] + ec[v];     // net.py:106
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) sQ[(d + v) * kLdQ + q] = t[v];
      }
      __syncthreads();
#pragma unroll 4
      for (int d = 0; d < kDK; ++d) {
        float rr[8], qq[4];
#pragma unroll
        for (int i = 0; i < 8; ++i) rr[i] = sR[d * kLdR + tx + 16 * i];
#pragma unroll
        for (int j = 0; j < 4; ++j) qq[j] = sQ[d * kLdQ + ty + 16 * j];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] += rr[i] * qq[j];
      }
    }
    __syncthreads();                                  // the staging area becomes the score tile
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = tx + 16 * i;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        sS[(ty + 16 * j) * kLdS + r] = row0 + r < V ? acc[i][j] : -INFINITY;
    }
    __syncthreads();
    if (tid < kQTile && q0 + tid < Q) {                // a thread per query: k passes over the tile's scores
      const float* s = sS + tid * kLdS;
      float ls = INFINITY;
      int li = -1;
      for (int m = 0; m < k; ++m) {
        float bs = -INFINITY;
        int bi = kTile;                                // nothing left: -inf with an id behind the vocabulary
        for (int r = 0; r < kTile; ++r) {
          const float x = s[r];
          const bool after = x < ls || (x == ls && r > li);
          if (after && (x > bs || (x == bs && r < bi))) {
            bs = x;
            bi = r;
          }
        }
        const int64_t o = ((int64_t)blockIdx.x * Q + q0 + tid) * k + m;
        cand_values[o] = bs;
        cand_ids[o] = bi < kTile && row0 + bi < V ? row0 + bi : INT64_MAX;
        ls = bs;
        li = bi;
      }
    }
  }
  if (bad && status) atomicOr(status, REC_FLAG_INDEX_OOB);
}

// the tiles' candidates of one query -> its k best; one wave per query
__global__ __launch_bounds__(kBlock) void w2v_topk_merge_kernel(const int64_t Q, const int64_t tiles, const int k,
                                                                const float* cand_values, const int64_t* cand_ids, float* values,
                                                                int64_t* ids) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int64_t q = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (q >= Q) return;
  const int64_t total = tiles * k;
  float ls = INFINITY;
  int64_t li = -1;
  for (int m = 0; m < k; ++m) {
    float bs = -INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t e = lane; e < total; e += kWave) {
      const int64_t t = e / k, o = (t * Q + q) * k + (e - t * k);
      const float x = cand_values[o];
      const int64_t id = cand_ids[o];
      if (before(ls, li, x, id) && before(x, id, bs, bi)) {
        bs = x;
        bi = id;
      }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const float xs = __shfl_xor(bs, o, kWave);
      const long long xi = __shfl_xor((long long)bi, o, kWave);
      if (before(xs, xi, bs, bi)) {
        bs = xs;
        bi = xi;
      }
    }
    if (lane == 0) {
      values[q * k + m] = bs;
      ids[q * k + m] = bi;
    }
    ls = bs;
    li = bi;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace rec

using namespace rec;

// the size checks the two training entry points share; -> 0 or the error
static int sgns_check(const char* what, int64_t batch, int32_t D, int32_t neg, int64_t V) {
  REC_REQUIRE(batch >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)batch);
  REC_REQUIRE(D >= 1 && D <= REC_W2V_MAX_DIM, REC_EINVAL, "%s: bad emb_dim %d (1..%d)", what, D, REC_W2V_MAX_DIM);
  REC_REQUIRE(neg >= 1 && neg <= REC_W2V_MAX_NEG, REC_EINVAL, "%s: bad neg %d (1..%d)", what, neg, REC_W2V_MAX_NEG);
  REC_REQUIRE(V >= 1, REC_EINVAL, "%s: bad num_rows %lld", what, (long long)V);
  REC_REQUIRE(batch * (1 + (int64_t)neg) < (1ll << 31), REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

#define W2V_STRIDE(ld, width, what, name)                                                                             \
  do {                                                                                                                \
    if ((ld) == 0) (ld) = (width);                                                                                    \
    REC_REQUIRE((ld) >= (width), REC_EINVAL, "%s: bad %s %lld: below the packed width %d", what, name, (long long)(ld), \
                (int)(width));                                                                                        \
  } while (0)

extern "C" int rec_w2v_sgns_fwd_bwd(int64_t batch, int32_t emb_dim, int32_t neg, int64_t num_rows, const int64_t* in_ids,
                                    const int64_t* target_ids, const float* emb, int64_t ld_emb, const float* emb_w,
                                    int64_t ld_w, const float* emb_b, int64_t ld_b, float grad_scale, float* true_logits,
                                    float* neg_logits, float* g, float* d_in, int64_t ld_din, float* loss, int32_t* status,
                                    void* stream) {
  static const char* what = "rec_w2v_sgns_fwd_bwd";
  const int D = emb_dim;
  if (int rc = sgns_check(what, batch, D, neg, num_rows)) return rc;
  W2V_STRIDE(ld_emb, D, what, "ld_emb");
  W2V_STRIDE(ld_w, D, what, "ld_w");
  W2V_STRIDE(ld_b, 1, what, "ld_b");
  W2V_STRIDE(ld_din, D, what, "ld_din");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(in_ids && target_ids && emb && emb_w && emb_b && true_logits && neg_logits && g && d_in && loss, REC_EINVAL,
              "%s: null pointer argument", what);
  const int rows = kBlock / kWave;
  const int64_t grid = (batch + rows - 1) / rows;
  const int per_wave = 3 * ((D + 3) / 4 * 4);         // three rows, each a multiple of 16 bytes; at most 12 KiB
  const size_t lds = (size_t)rows * per_wave * sizeof(float);
  const float st = grad_scale / (float)batch, sn = grad_scale / ((float)batch * (float)neg);
  const bool vec = D % 4 == 0 && ld_emb % 4 == 0 && ld_w % 4 == 0 && ld_din % 4 == 0 && aligned16(emb) && aligned16(emb_w) &&
                   aligned16(d_in);
  if (vec)
    hipLaunchKernelGGL(w2v_sgns_kernel<4>, dim3((unsigned)grid), dim3(kBlock), lds, (hipStream_t)stream, batch, D, (int)neg,
                       num_rows, per_wave, in_ids, target_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, st, sn, true_logits,
                       neg_logits, g, d_in, ld_din, status);
  else
    hipLaunchKernelGGL(w2v_sgns_kernel<1>, dim3((unsigned)grid), dim3(kBlock), lds, (hipStream_t)stream, batch, D, (int)neg,
                       num_rows, per_wave, in_ids, target_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, st, sn, true_logits,
                       neg_logits, g, d_in, ld_din, status);
  hipLaunchKernelGGL(w2v_loss_fold_kernel, dim3(1), dim3(kFoldBlock), 0, (hipStream_t)stream, batch, (int)neg, num_rows, in_ids,
                     target_ids, true_logits, neg_logits, loss);
  return check_launch(what);
}

extern "C" int rec_w2v_target_update(int64_t batch, int32_t emb_dim, int32_t neg, int64_t num_rows, const int32_t* n_uniq,
                                     const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos,
                                     const float* g, const int64_t* in_ids, const float* emb, int64_t ld_emb, float* emb_w,
                                     int64_t ld_w, float* emb_b, int64_t ld_b, float lr, float* d_w_rows, int64_t ld_dw,
                                     float* d_b_rows, void* stream) {
  static const char* what = "rec_w2v_target_update";
  const int D = emb_dim;
  if (int rc = sgns_check(what, batch, D, neg, num_rows)) return rc;
  W2V_STRIDE(ld_emb, D, what, "ld_emb");
  W2V_STRIDE(ld_w, D, what, "ld_w");
  W2V_STRIDE(ld_b, 1, what, "ld_b");
  W2V_STRIDE(ld_dw, D, what, "ld_dw");
  if (emb && emb_w) {                                 // emb is read while emb_w is written: they may not share a float
    const uintptr_t a0 = (uintptr_t)emb, a1 = a0 + (size_t)num_rows * ld_emb * sizeof(float);
    const uintptr_t b0 = (uintptr_t)emb_w, b1 = b0 + (size_t)num_rows * ld_w * sizeof(float);
    REC_REQUIRE(a1 <= b0 || b1 <= a0, REC_EINVAL, "%s: emb aliases emb_w (the input table is read while the rows are updated)",
                what);
  }
  if (batch == 0) return REC_OK;
  REC_REQUIRE(n_uniq && uniq_rows && seg_offset && sorted_pos && g && in_ids && emb && emb_w && emb_b, REC_EINVAL,
              "%s: null pointer argument", what);
  const int tw = 1 + neg;
  const int64_t n = batch * tw;
  const bool vec = D % 4 == 0 && ld_emb % 4 == 0 && ld_w % 4 == 0 && ld_dw % 4 == 0 && aligned16(emb) && aligned16(emb_w) &&
                   (!d_w_rows || aligned16(d_w_rows));
  const int rows = kBlock / kWave;
  int64_t grid = (n + rows - 1) / rows;
  grid = grid > 8 * kNumCU ? 8 * kNumCU : grid;
  const int chunks = vec ? D / 4 : D;
  int64_t lx = (n + kLongBlock - 1) / kLongBlock;
  lx = lx > 4 * kNumCU ? 4 * kNumCU : lx;
  const dim3 lgrid((unsigned)lx, (unsigned)((chunks + kSliceLanes - 1) / kSliceLanes), kLongSplit);
  if (vec) {
    hipLaunchKernelGGL(w2v_update_short_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, n, D, tw, num_rows,
                       n_uniq, uniq_rows, seg_offset, sorted_pos, g, in_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, lr, d_w_rows,
                       ld_dw, d_b_rows);
    hipLaunchKernelGGL(w2v_update_long_kernel<4>, lgrid, dim3(kLongBlock), 0, (hipStream_t)stream, n, D, tw, num_rows, n_uniq,
                       uniq_rows, seg_offset, sorted_pos, g, in_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, lr, d_w_rows, ld_dw,
                       d_b_rows);
  } else {
    hipLaunchKernelGGL(w2v_update_short_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, n, D, tw, num_rows,
                       n_uniq, uniq_rows, seg_offset, sorted_pos, g, in_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, lr, d_w_rows,
                       ld_dw, d_b_rows);
    hipLaunchKernelGGL(w2v_update_long_kernel<1>, lgrid, dim3(kLongBlock), 0, (hipStream_t)stream, n, D, tw, num_rows, n_uniq,
                       uniq_rows, seg_offset, sorted_pos, g, in_ids, emb, ld_emb, emb_w, ld_w, emb_b, ld_b, lr, d_w_rows, ld_dw,
                       d_b_rows);
  }
  return check_launch(what);
}

extern "C" int rec_w2v_analogy_topk(int64_t n_query, int32_t emb_dim, int64_t row_stride, int64_t num_rows, int32_t k,
                                    const int64_t* a, const int64_t* b, const int64_t* c, const float* W, float* cand_values,
                                    int64_t* cand_ids, int64_t n_tiles, float* values, int64_t* ids, int32_t* status,
                                    void* stream) {
  static const char* what = "rec_w2v_analogy_topk";
  const int D = emb_dim;
  REC_REQUIRE(n_query >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)n_query);
  REC_REQUIRE(D >= 1 && D <= REC_W2V_MAX_DIM, REC_EINVAL, "%s: bad emb_dim %d (1..%d)", what, D, REC_W2V_MAX_DIM);
  REC_REQUIRE(k >= 1 && k <= REC_W2V_MAX_TOPK, REC_EINVAL, "%s: bad k %d (1..%d)", what, k, REC_W2V_MAX_TOPK);
  REC_REQUIRE(num_rows >= k, REC_EINVAL, "%s: bad num_rows %lld: fewer rows than k %d", what, (long long)num_rows, k);
  W2V_STRIDE(row_stride, D, what, "row_stride");
  const int64_t tiles = (num_rows + kTile - 1) / kTile;
  REC_REQUIRE(n_tiles == tiles, REC_EINVAL, "%s: bad n_tiles %lld: %lld rows are %lld tiles of %d", what, (long long)n_tiles,
              (long long)num_rows, (long long)tiles, kTile);
  REC_REQUIRE(tiles < (1ll << 31) && n_query < (1ll << 31), REC_ESHAPE, "%s: too many rows", what);
  if (n_query == 0) return REC_OK;
  REC_REQUIRE(a && b && c && W && cand_values && cand_ids && values && ids, REC_EINVAL, "%s: null pointer argument", what);
  if (D % 4 == 0 && row_stride % 4 == 0 && aligned16(W))
    hipLaunchKernelGGL(w2v_topk_tile_kernel<4>, dim3((unsigned)tiles), dim3(kBlock), 0, (hipStream_t)stream, n_query, D,
                       row_stride, num_rows, (int)k, a, b, c, W, cand_values, cand_ids, status);
  else
    hipLaunchKernelGGL(w2v_topk_tile_kernel<1>, dim3((unsigned)tiles), dim3(kBlock), 0, (hipStream_t)stream, n_query, D,
                       row_stride, num_rows, (int)k, a, b, c, W, cand_values, cand_ids, status);
  const int rows = kBlock / kWave;
  hipLaunchKernelGGL(w2v_topk_merge_kernel, dim3((unsigned)((n_query + rows - 1) / rows)), dim3(kBlock), 0, (hipStream_t)stream,
                     n_query, tiles, (int)k, cand_values, cand_ids, values, ids);
  return check_launch(what);
}
