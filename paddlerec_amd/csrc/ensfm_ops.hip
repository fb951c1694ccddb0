// ENSFM (models/recall/ensfm): the non-sampling factorization machine, trained on ALL user-item pairs.
//
// The reference builds dot = einsum('ac,bc->abc', p_emb, q_emb), a [B, I+1, C] tensor, on every step (net.py:87-88) and three
// [B, P, C] tensors for the positives (net.py:92-97).  The step needs two [n, C] tower outputs, two C x C Gram matrices and
// one scalar per (b, j); that is what these kernels move.  C = D + 2.
//
//   ef_tower_fwd_kernel      one wave per row: the field sum, the FM cross score against H_s, the bias sum -> [n, C]
//   ef_tower_bwd_kernel      the per-lookup gradient rows, d score per row and per-block partials of dH_s / d bias
//   ef_fold_cols_kernel      the fixed-order fold of those partials (one block per column)
//   ef_gram_kernel / ef_gram_fold_kernel   G = X^T X: 64-row LDS tiles, 4 x 4 entries per thread, per-block partials, an
//                            ascending fold
//   ef_pos_user_kernel       one block per user: gathers q[ur[b, j]] from L2, forward and backward of the positives in one
//                            pass (g, the user's loss share, dP, the user's dH_i partial)
//   ef_item_gram_kernel      dQ[i] = 2 w Q[i] (G_p o h h^T) for all I + 1 rows
//   ef_pos_item_kernel       one block per item that has positives: dQ[i] += h o sum g[b, j] P[b], 16 interleaved partials
//   ef_loss_kernel           the loss and dH_i folds with their Gram shares
//   ef_score_kernel          pre [B, I+1] for --infer, LDS-tiled; dot is never formed
//
// No float atomics: the only atomic is the OR into the integer status word.  Every sum has a fixed order.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kEfRows = kBlock / kWave;                      // rows (waves) per block
constexpr int kEfKC = (REC_ENSFM_MAX_DIM + 2 + kWave - 1) / kWave;   // columns of a [., C] row per lane
constexpr int kEfKD = (REC_ENSFM_MAX_DIM + kWave - 1) / kWave;       // columns of a [., D] row per lane
constexpr int kEfCMax = REC_ENSFM_MAX_DIM + 2;
constexpr int kEfGramTile = 64;
constexpr int kEfScoreUsers = 16, kEfScoreItems = 64;

__device__ __forceinline__ float ef_h(const float* __restrict__ Hi, int c, int D) { return c < D ? Hi[c] : 1.f; }

// s^2 - sum e^2 with every product rounded on its own (no contraction into an fma): with one field, or one valid id, the
// cross term is then exactly 0, as in the reference's float32 evaluation, and not the rounding residue of e^2
__device__ __forceinline__ float ef_sq(float e) {
#pragma clang fp contract(off)
  return e * e;
}
__device__ __forceinline__ float ef_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float ef_cross(float s, float sq) { return ef_add(ef_sq(s), -sq); }

// ---------------------------------------------------------------- towers
// out[r] = [s, score + bias sum (+ bias), 1] (user layout) or [s, 1, score + bias sum] (item layout), net.py:65-83
__global__ __launch_bounds__(kBlock) void ef_tower_fwd_kernel(int64_t n, int F, int D, int64_t num_rows, int64_t bias_rows,
                                                              const int64_t* __restrict__ ids,
                                                              const float* __restrict__ table, int64_t ldt,
                                                              const float* __restrict__ bias_table,
                                                              const float* __restrict__ Hs, const float* __restrict__ bias,
                                                              int item_layout, float* __restrict__ out, int64_t ldo,
                                                              int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * kEfRows + (threadIdx.x >> 6);
  if (r >= n) return;
  float s[kEfKD], sq[kEfKD];
#pragma unroll
  for (int k = 0; k < kEfKD; ++k) s[k] = sq[k] = 0.f;
  float bsum = 0.f;
  bool bad = false;
  for (int f = 0; f < F; ++f) {
    const int64_t id = ids[r * F + f];
    const bool ok = id >= 0 && id < num_rows;
    const bool okb = id >= 0 && id < bias_rows;
    bad |= !ok || !okb;
    if (okb) bsum += bias_table[id];
    if (ok) {
#pragma unroll
      for (int k = 0; k < kEfKD; ++k) {
        const int c = lane + k * kWave;
        if (c < D) {
          const float e = table[id * ldt + c];
          s[k] += e;
          sq[k] = ef_add(sq[k], ef_sq(e));
        }
      }
    }
  }
  if (bad && lane == 0 && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
  float cross = 0.f;
#pragma unroll
  for (int k = 0; k < kEfKD; ++k) {
    const int c = lane + k * kWave;
    if (c < D) {
      cross = fmaf(0.5f * ef_cross(s[k], sq[k]), Hs[c], cross);
      out[r * ldo + c] = s[k];
    }
  }
  cross = group_sum<kWave>(cross);
  if (lane == 0) {
    const float score = cross + bsum + (bias != nullptr ? bias[0] : 0.f);
    out[r * ldo + D] = item_layout ? 1.f : score;
    out[r * ldo + D + 1] = item_layout ? score : 1.f;
  }
}

// rows[r * F + f] = ds + dscore H_s o (s - e_f); dscore[r]; partials[block] = [sum_r dscore_r cross_r (D), sum_r dscore_r]
__global__ __launch_bounds__(kBlock) void ef_tower_bwd_kernel(int64_t n, int rows_per_block, int F, int D, int64_t num_rows,
                                                              const int64_t* __restrict__ ids,
                                                              const float* __restrict__ table, int64_t ldt,
                                                              const float* __restrict__ Hs, const float* __restrict__ dout,
                                                              int64_t lddo, int item_layout, float* __restrict__ rows,
                                                              int64_t ldr, float* __restrict__ dscore,
                                                              float* __restrict__ partials) {
  __shared__ float part[kEfRows][REC_ENSFM_MAX_DIM + 1];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  float hacc[kEfKD], hs[kEfKD];
#pragma unroll
  for (int k = 0; k < kEfKD; ++k) {
    const int c = lane + k * kWave;
    hacc[k] = 0.f;
    hs[k] = c < D ? Hs[c] : 0.f;
  }
  float bacc = 0.f;
  for (int64_t r = r0 + wave; r < r1; r += kEfRows) {
    const float dsc = dout[r * lddo + (item_layout ? D + 1 : D)];
    float s[kEfKD], sq[kEfKD], ds[kEfKD];
#pragma unroll
    for (int k = 0; k < kEfKD; ++k) {
      const int c = lane + k * kWave;
      s[k] = sq[k] = 0.f;
      ds[k] = c < D ? dout[r * lddo + c] : 0.f;
    }
    for (int f = 0; f < F; ++f) {
      const int64_t id = ids[r * F + f];
      if (id < 0 || id >= num_rows) continue;
#pragma unroll
      for (int k = 0; k < kEfKD; ++k) {
        const int c = lane + k * kWave;
        if (c < D) {
          const float e = table[id * ldt + c];
          s[k] += e;
          sq[k] = ef_add(sq[k], ef_sq(e));
        }
      }
    }
    for (int f = 0; f < F; ++f) {
      const int64_t id = ids[r * F + f];
      const bool ok = id >= 0 && id < num_rows;
#pragma unroll
      for (int k = 0; k < kEfKD; ++k) {
        const int c = lane + k * kWave;
        if (c < D) {
          const float e = ok ? table[id * ldt + c] : 0.f;
          rows[(r * F + f) * ldr + c] = ok ? fmaf(dsc * hs[k], s[k] - e, ds[k]) : 0.f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kEfKD; ++k) hacc[k] = fmaf(dsc, 0.5f * ef_cross(s[k], sq[k]), hacc[k]);
    bacc += dsc;
    if (lane == 0) dscore[r] = dsc;
  }
#pragma unroll
  for (int k = 0; k < kEfKD; ++k) {
    const int c = lane + k * kWave;
    if (c < D) part[wave][c] = hacc[k];
  }
  if (lane == 0) part[wave][D] = bacc;
  __syncthreads();
  for (int c = threadIdx.x; c <= D; c += kBlock)
    partials[(int64_t)blockIdx.x * (D + 1) + c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// out[c] (+)= sum_p partials[p, c]: one block per column, the partials strided over its threads, then a tree.  Column
// `split` and beyond go to out1 (may be NULL: dropped).
__global__ __launch_bounds__(kBlock) void ef_fold_cols_kernel(int nparts, int width, int split,
                                                              const float* __restrict__ partials, float* __restrict__ out0,
                                                              float* __restrict__ out1, int accumulate) {
  __shared__ float red[kBlock];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < nparts; p += kBlock) s += partials[(int64_t)p * width + c];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float* dst = c < split ? out0 + c : (out1 != nullptr ? out1 + (c - split) : nullptr);
    if (dst != nullptr) *dst = accumulate ? *dst + red[0] : red[0];
  }
}

// ---------------------------------------------------------------- Gram
// block b owns the tiles [b * tiles_per_block, ...) of 64 rows; partials[b] = sum over its rows of x x^T (ascending rows)
__global__ __launch_bounds__(kBlock) void ef_gram_kernel(int64_t n, int C, int64_t tiles_per_block,
                                                         const float* __restrict__ X, int64_t ldx,
                                                         float* __restrict__ partials) {
  extern __shared__ float tile[];                            // [kEfGramTile][C]
  const int CC = C * C, nt = (C + 3) / 4;
  float* __restrict__ mine = partials + (int64_t)blockIdx.x * CC;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
  for (int64_t t = t0; t < t0 + tiles_per_block; ++t) {
    const int64_t r0 = t * kEfGramTile;
    if (r0 >= n && t > t0) break;
    const int rows = r0 >= n ? 0 : (int)(n - r0 < kEfGramTile ? n - r0 : kEfGramTile);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * C; e += kBlock) tile[e] = X[(r0 + e / C) * ldx + e % C];
    __syncthreads();
    // a thread owns 4 x 4 entries at a time: 8 LDS reads feed 16 independent fma chains per row (one entry per thread
    // left every fma waiting for its own two reads; 8 to 58 blocks cannot hide that with occupancy)
    for (int st = threadIdx.x; st < nt * nt; st += kBlock) {
      const int a0 = (st / nt) * 4, b0 = (st % nt) * 4;
      int ai[4], bi[4];
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ai[i] = a0 + i < C ? a0 + i : C - 1;                  // clamped: always a column of the row; such entries are not stored
        bi[i] = b0 + i < C ? b0 + i : C - 1;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)                           // an overhanging entry starts at 0: another thread owns what its clamp names
          acc[i][j] = t > t0 && a0 + i < C && b0 + j < C ? mine[(a0 + i) * C + b0 + j] : 0.f;
      for (int r = 0; r < rows; ++r) {
        const float* __restrict__ row = tile + r * C;
        float av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          av[i] = row[ai[i]];
          bv[i] = row[bi[i]];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (a0 + i < C && b0 + j < C) mine[(a0 + i) * C + b0 + j] = acc[i][j];
    }
  }
}

__global__ __launch_bounds__(kBlock) void ef_gram_fold_kernel(int nparts, int CC, const float* __restrict__ partials,
                                                              float* __restrict__ G) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= CC) return;
  float s = 0.f;
  int p = 0;
  for (; p + 4 <= nparts; p += 4) {                           // four loads in flight, added in ascending p
    const float a = partials[(int64_t)p * CC + e], b = partials[(int64_t)(p + 1) * CC + e];
    const float c = partials[(int64_t)(p + 2) * CC + e], d = partials[(int64_t)(p + 3) * CC + e];
    s = (((s + a) + b) + c) + d;
  }
  for (; p < nparts; ++p) s += partials[(int64_t)p * CC + e];
  G[e] = s;
}

// ---------------------------------------------------------------- positives, user-owned
// One block per user; wave w takes the list positions 16 t + 4 w .. + 3 (four gathers in flight), each wave in ascending
// j, the four waves folded in ascending order.  net.py:92-97 and dygraph_model.py:50 with their backward.
__global__ __launch_bounds__(kBlock) void ef_pos_user_kernel(int P, int D, int64_t I, float w,
                                                             const int64_t* __restrict__ ur, const float* __restrict__ p,
                                                             int64_t ldp, const float* __restrict__ q, int64_t ldq,
                                                             const float* __restrict__ Hi, const float* __restrict__ Gq,
                                                             float* __restrict__ g, float* __restrict__ pos_r,
                                                             float* __restrict__ dP, int64_t lddp,
                                                             float* __restrict__ loss_part, float* __restrict__ dHi_part,
                                                             int32_t* __restrict__ status) {
  __shared__ float ph_s[kEfCMax];
  __shared__ float acc_s[kEfRows][kEfCMax];
  __shared__ float loss_s[kEfRows];
  const int C = D + 2;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x;
  for (int c = threadIdx.x; c < C; c += kBlock) ph_s[c] = p[b * ldp + c] * ef_h(Hi, c, D);
  __syncthreads();
  float ph[kEfKC], acc[kEfKC];
#pragma unroll
  for (int k = 0; k < kEfKC; ++k) {
    const int c = lane + k * kWave;
    ph[k] = c < C ? ph_s[c] : 0.f;
    acc[k] = 0.f;
  }
  float lsum = 0.f;
  bool bad = false;
  const float w1 = 1.f - w;
  for (int j0 = wave * 4; j0 < P; j0 += 4 * kEfRows) {
    float qv[4][kEfKC], dot[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      const int64_t id = j < P ? ur[b * P + j] : I;
      ok[u] = id >= 0 && id < I;                             // id == I is the padding of the list (net.py:93)
      bad |= !ok[u] && id != I;
      dot[u] = 0.f;
#pragma unroll
      for (int k = 0; k < kEfKC; ++k) {
        const int c = lane + k * kWave;
        qv[u][k] = ok[u] && c < C ? q[id * ldq + c] : 0.f;
        dot[u] = fmaf(ph[k], qv[u][k], dot[u]);
      }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
      for (int u = 0; u < 4; ++u) dot[u] += __shfl_xor(dot[u], o, kWave);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      const float pr = ok[u] ? dot[u] : 0.f;
      const float gg = ok[u] ? 2.f * w1 * pr - 2.f : 0.f;
      lsum += w1 * pr * pr - 2.f * pr;
      if (lane == 0 && j < P) {
        g[b * P + j] = gg;
        if (pos_r != nullptr) pos_r[b * P + j] = pr;
      }
#pragma unroll
      for (int k = 0; k < kEfKC; ++k) acc[k] = fmaf(gg, qv[u][k], acc[k]);
    }
  }
  if (bad && lane == 0 && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
#pragma unroll
  for (int k = 0; k < kEfKC; ++k) {
    const int c = lane + k * kWave;
    if (c < C) acc_s[wave][c] = acc[k];
  }
  if (lane == 0) loss_s[wave] = lsum;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kBlock) {
    const float a = ((acc_s[0][c] + acc_s[1][c]) + acc_s[2][c]) + acc_s[3][c];
    if (c < D) dHi_part[b * D + c] = p[b * ldp + c] * a;
    float t = 0.f;                                          // sum_c' P[b, c'] h[c'] G_q[c, c'] (G_q is symmetric)
    for (int c2 = 0; c2 < C; ++c2) t = fmaf(ph_s[c2], Gq[c2 * C + c], t);
    const float h = ef_h(Hi, c, D);
    dP[b * lddp + c] = fmaf(h, a, 2.f * w * h * t);
  }
  if (threadIdx.x == 0) loss_part[b] = ((loss_s[0] + loss_s[1]) + loss_s[2]) + loss_s[3];
}

// ---------------------------------------------------------------- positives, item-owned
// dQ[i] = 2 w h o (G_p (Q[i] o h)) for every row: the whole-data term of the loss reaches all I + 1 items
__global__ __launch_bounds__(kBlock) void ef_item_gram_kernel(int64_t rows, int D, float w, const float* __restrict__ q,
                                                              int64_t ldq, const float* __restrict__ Hi,
                                                              const float* __restrict__ Gp, float* __restrict__ dQ,
                                                              int64_t lddq) {
  __shared__ float qh[kEfRows][kEfCMax];
  const int C = D + 2;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kEfRows + wave;
  if (i < rows)
    for (int c = lane; c < C; c += kWave) qh[wave][c] = q[i * ldq + c] * ef_h(Hi, c, D);
  __syncthreads();
  if (i >= rows) return;
  for (int c = lane; c < C; c += kWave) {
    float t = 0.f;
    for (int c2 = 0; c2 < C; ++c2) t = fmaf(qh[wave][c2], Gp[c2 * C + c], t);
    dQ[i * lddq + c] = 2.f * w * ef_h(Hi, c, D) * t;
  }
}

// One block per unique item of the grouping.  Occurrence i of its segment goes to partial i % 16 (wave (i % 16) / 4,
// accumulator i % 4), each partial in ascending i, folded in a fixed tree: a hot item is 16 chains, never one.
__global__ __launch_bounds__(kBlock) void ef_pos_item_kernel(int64_t n_pos, int P, int D, int64_t I,
                                                             const int32_t* __restrict__ n_uniq,
                                                             const int64_t* __restrict__ uniq_rows,
                                                             const int32_t* __restrict__ seg_offset,
                                                             const int32_t* __restrict__ sorted_pos,
                                                             const float* __restrict__ g, const float* __restrict__ p,
                                                             int64_t ldp, const float* __restrict__ Hi,
                                                             float* __restrict__ dQ, int64_t lddq) {
  __shared__ float acc_s[kEfRows][kEfCMax];
  const int C = D + 2;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if ((int)blockIdx.x >= n_uniq[0]) return;
  const int64_t row = uniq_rows[blockIdx.x];
  const int beg = seg_offset[blockIdx.x], end = seg_offset[blockIdx.x + 1];
  if (row < 0 || row > I || beg < 0 || end > n_pos) return;       // never true for a grouping of ur; no write without it
  float a[4][kEfKC];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int k = 0; k < kEfKC; ++k) a[u][k] = 0.f;
  for (int i0 = beg + wave * 4; i0 < end; i0 += 4 * kEfRows) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u;
      const int pos = i < end ? sorted_pos[i] : -1;
      const bool ok = pos >= 0 && pos < n_pos;
      const float gg = ok ? g[pos] : 0.f;
      const int64_t b = ok ? pos / P : 0;
#pragma unroll
      for (int k = 0; k < kEfKC; ++k) {
        const int c = lane + k * kWave;
        const float pv = ok && c < C ? p[b * ldp + c] : 0.f;
        a[u][k] = fmaf(gg, pv, a[u][k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kEfKC; ++k) {
    const int c = lane + k * kWave;
    if (c < C) acc_s[wave][c] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kBlock) {
    const float s = ((acc_s[0][c] + acc_s[1][c]) + acc_s[2][c]) + acc_s[3][c];
    dQ[row * lddq + c] = fmaf(ef_h(Hi, c, D), s, dQ[row * lddq + c]);
  }
}

// ---------------------------------------------------------------- loss and dH_i
// block d < D: dH_i[d] = sum_b dHi_part[b, d] + 2 w sum_c' G_q[d, c'] G_p[d, c'] h[c'];
// block D: loss = w sum_{c, c'} G_q G_p h h + sum_b loss_part[b]   (dygraph_model.py:40-51)
__global__ __launch_bounds__(kBlock) void ef_loss_kernel(int64_t B, int D, float w, const float* __restrict__ Gp,
                                                         const float* __restrict__ Gq, const float* __restrict__ Hi,
                                                         const float* __restrict__ loss_part,
                                                         const float* __restrict__ dHi_part, float* __restrict__ loss,
                                                         float* __restrict__ dHi) {
  __shared__ float red[kBlock], red2[kBlock];
  const int C = D + 2, d = blockIdx.x;
  float s = 0.f, t = 0.f;
  if (d < D) {
    for (int64_t b = threadIdx.x; b < B; b += kBlock) s += dHi_part[b * D + d];
    for (int c = threadIdx.x; c < C; c += kBlock) t = fmaf(Gq[d * C + c] * Gp[d * C + c], ef_h(Hi, c, D), t);
  } else {
    for (int64_t b = threadIdx.x; b < B; b += kBlock) s += loss_part[b];
    for (int e = threadIdx.x; e < C * C; e += kBlock)
      t = fmaf(Gq[e] * Gp[e], ef_h(Hi, e / C, D) * ef_h(Hi, e % C, D), t);
  }
  red[threadIdx.x] = s;
  red2[threadIdx.x] = t;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[threadIdx.x] += red[threadIdx.x + o];
      red2[threadIdx.x] += red2[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (d < D) dHi[d] = fmaf(2.f * w, red2[0], red[0]);
    else loss[0] = fmaf(w, red2[0], red[0]);
  }
}

// ---------------------------------------------------------------- scores for --infer
// pre[b, i] = sum_c p[b, c] h[c] q[i, c]: a 16-user x 64-item tile per block, both operands staged in LDS
__global__ __launch_bounds__(kBlock) void ef_score_kernel(int64_t B, int64_t rows, int D, const float* __restrict__ p,
                                                          int64_t ldp, const float* __restrict__ q, int64_t ldq,
                                                          const float* __restrict__ Hi, float* __restrict__ pre,
                                                          int64_t ldpre) {
  extern __shared__ float sm[];
  const int C = D + 2, CP = C | 1;                            // odd pitch: 64 item rows fall on distinct banks
  float* __restrict__ qs = sm;                                // [kEfScoreItems][CP]
  float* __restrict__ ps = sm + kEfScoreItems * CP;           // [kEfScoreUsers][C]
  const int64_t i0 = (int64_t)blockIdx.x * kEfScoreItems, b0 = (int64_t)blockIdx.y * kEfScoreUsers;
  for (int e = threadIdx.x; e < kEfScoreItems * C; e += kBlock) {
    const int r = e / C, c = e - r * C;
    qs[r * CP + c] = i0 + r < rows ? q[(i0 + r) * ldq + c] : 0.f;
  }
  for (int e = threadIdx.x; e < kEfScoreUsers * C; e += kBlock) {
    const int r = e / C, c = e - r * C;
    ps[e] = b0 + r < B ? p[(b0 + r) * ldp + c] * ef_h(Hi, c, D) : 0.f;
  }
  __syncthreads();
  const int it = threadIdx.x & (kEfScoreItems - 1), ug = threadIdx.x >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const float qv = qs[it * CP + c];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(ps[(ug * 4 + u) * C + c], qv, acc[u]);
  }
  if (i0 + it < rows) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (b0 + ug * 4 + u < B) pre[(b0 + ug * 4 + u) * ldpre + i0 + it] = acc[u];
  }
}

bool ef_dim_ok(int32_t D) { return D >= 1 && D <= REC_ENSFM_MAX_DIM; }

int64_t ef_tower_blocks(int64_t n, int* rows_per_block) {
  int64_t rpb = (n + REC_ENSFM_MAX_PARTIALS - 1) / REC_ENSFM_MAX_PARTIALS;
  rpb = (rpb + kEfRows - 1) / kEfRows * kEfRows;
  if (rpb < kEfRows) rpb = kEfRows;
  *rows_per_block = (int)rpb;
  return (n + rpb - 1) / rpb;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_ensfm_tower_fwd(int64_t n, int32_t num_fields, int32_t emb_dim, int64_t num_rows, int64_t bias_rows,
                                   const int64_t* ids, const float* table, int64_t ld_table, const float* bias_table,
                                   const float* H_s, const float* bias, int32_t item_layout, float* out, int64_t ld_out,
                                   int32_t* status, void* stream) {
  const char* what = "rec_ensfm_tower_fwd";
  REC_REQUIRE(n >= 0 && num_fields >= 1 && num_rows >= 1 && bias_rows >= 1, REC_EINVAL,
              "%s: bad sizes (n %lld, num_fields %d, num_rows %lld, bias_rows %lld)", what, (long long)n, num_fields,
              (long long)num_rows, (long long)bias_rows);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(n * num_fields < (1ll << 31), REC_EINVAL, "%s: n * num_fields too large", what);
  REC_REQUIRE(ld_table >= emb_dim && ld_out >= emb_dim + 2, REC_EINVAL, "%s: a row stride is smaller than its row", what);
  if (n == 0) return REC_OK;
  REC_REQUIRE(ids && table && bias_table && H_s && out, REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(out != table && out != bias_table && out != H_s && out != bias, REC_EINVAL, "%s: out aliases an input", what);
  hipLaunchKernelGGL(ef_tower_fwd_kernel, dim3((unsigned)((n + kEfRows - 1) / kEfRows)), dim3(kBlock), 0, (hipStream_t)stream,
                     n, (int)num_fields, (int)emb_dim, num_rows, bias_rows, ids, table, ld_table, bias_table, H_s, bias,
                     (int)item_layout, out, ld_out, status);
  return check_launch(what);
}

extern "C" int rec_ensfm_tower_bwd(int64_t n, int32_t num_fields, int32_t emb_dim, int64_t num_rows, const int64_t* ids,
                                   const float* table, int64_t ld_table, const float* H_s, const float* d_out, int64_t ld_dout,
                                   int32_t item_layout, float* rows, int64_t ld_rows, float* dscore, float* partials,
                                   float* dH_s, float* dbias, int32_t accumulate, void* stream) {
  const char* what = "rec_ensfm_tower_bwd";
  REC_REQUIRE(n >= 0 && num_fields >= 1 && num_rows >= 1, REC_EINVAL, "%s: bad sizes (n %lld, num_fields %d, num_rows %lld)",
              what, (long long)n, num_fields, (long long)num_rows);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(n * num_fields < (1ll << 31), REC_EINVAL, "%s: n * num_fields too large", what);
  REC_REQUIRE(ld_table >= emb_dim && ld_dout >= emb_dim + 2 && ld_rows >= emb_dim, REC_EINVAL,
              "%s: a row stride is smaller than its row", what);
  REC_REQUIRE(dH_s && dH_s != H_s && dH_s != dbias, REC_EINVAL, "%s: dH_s is null, H_s or dbias", what);
  if (n == 0) return REC_OK;
  REC_REQUIRE(ids && table && H_s && d_out && rows && dscore && partials, REC_EINVAL, "%s: null pointer argument", what);
  for (const float* o : {(const float*)rows, (const float*)dscore, (const float*)partials, (const float*)dH_s})
    REC_REQUIRE(o != table && o != d_out && o != H_s, REC_EINVAL, "%s: an output aliases an input", what);
  REC_REQUIRE(rows != dscore && rows != partials && dscore != partials && rows != dH_s && dscore != dH_s && partials != dH_s &&
                  (dbias == nullptr || (dbias != rows && dbias != dscore && dbias != partials)),
              REC_EINVAL, "%s: the outputs alias each other", what);
  int rpb = 0;
  const int64_t blocks = ef_tower_blocks(n, &rpb);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ef_tower_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, n, rpb, (int)num_fields, (int)emb_dim,
                     num_rows, ids, table, ld_table, H_s, d_out, ld_dout, (int)item_layout, rows, ld_rows, dscore, partials);
  int rc = check_launch(what);
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(ef_fold_cols_kernel, dim3((unsigned)(emb_dim + 1)), dim3(kBlock), 0, st, (int)blocks, (int)emb_dim + 1,
                     (int)emb_dim, (const float*)partials, dH_s, dbias, (int)accumulate);
  return check_launch("rec_ensfm_tower_bwd (fold)");
}

extern "C" int rec_ensfm_gram(int64_t n, int32_t cols, const float* X, int64_t ldx, float* partials, float* G, void* stream) {
  const char* what = "rec_ensfm_gram";
  REC_REQUIRE(n >= 0 && cols >= 1 && cols <= REC_ENSFM_MAX_DIM + 2, REC_EINVAL, "%s: bad sizes (n %lld, cols %d; cols <= %d)",
              what, (long long)n, cols, REC_ENSFM_MAX_DIM + 2);
  REC_REQUIRE(ldx >= cols, REC_EINVAL, "%s: ldx is smaller than cols", what);
  REC_REQUIRE(G && partials && G != partials, REC_EINVAL, "%s: G / partials null or the same", what);
  if (n == 0) return REC_OK;
  REC_REQUIRE(X && X != G && X != partials, REC_EINVAL, "%s: X is null or aliases an output", what);
  const int64_t tiles = (n + kEfGramTile - 1) / kEfGramTile;
  int64_t blocks = tiles < REC_ENSFM_GRAM_MAX_BLOCKS ? tiles : REC_ENSFM_GRAM_MAX_BLOCKS;
  const int64_t tpb = (tiles + blocks - 1) / blocks;
  blocks = (tiles + tpb - 1) / tpb;                           // every block owns at least one tile
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ef_gram_kernel, dim3((unsigned)blocks), dim3(kBlock), (size_t)kEfGramTile * cols * sizeof(float), st, n,
                     (int)cols, tpb, X, ldx, partials);
  int rc = check_launch(what);
  if (rc != REC_OK) return rc;
  const int CC = cols * cols;
  hipLaunchKernelGGL(ef_gram_fold_kernel, dim3((unsigned)((CC + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (int)blocks, CC,
                     (const float*)partials, G);
  return check_launch("rec_ensfm_gram (fold)");
}

extern "C" int rec_ensfm_pos_user(int64_t batch, int32_t max_pos, int32_t emb_dim, int64_t num_items, float neg_weight,
                                  const int64_t* ur, const float* p, int64_t ld_p, const float* q, int64_t ld_q,
                                  const float* H_i, const float* G_q, float* g, float* pos_r, float* dP, int64_t ld_dp,
                                  float* loss_part, float* dHi_part, int32_t* status, void* stream) {
  const char* what = "rec_ensfm_pos_user";
  REC_REQUIRE(batch >= 0 && max_pos >= 1 && num_items >= 1, REC_EINVAL, "%s: bad sizes (batch %lld, max_pos %d, num_items %lld)",
              what, (long long)batch, max_pos, (long long)num_items);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(isfinite(neg_weight), REC_EINVAL, "%s: neg_weight must be finite", what);
  REC_REQUIRE(batch * max_pos < (1ll << 31), REC_EINVAL, "%s: batch * max_pos too large", what);
  REC_REQUIRE(ld_p >= emb_dim + 2 && ld_q >= emb_dim + 2 && ld_dp >= emb_dim + 2, REC_EINVAL,
              "%s: a row stride is smaller than emb_dim + 2", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(ur && p && q && H_i && G_q && g && dP && loss_part && dHi_part, REC_EINVAL, "%s: null pointer argument", what);
  for (const float* o : {(const float*)g, (const float*)pos_r, (const float*)dP, (const float*)loss_part, (const float*)dHi_part})
    REC_REQUIRE(o != p && o != q && o != H_i && o != G_q, REC_EINVAL, "%s: an output aliases an input", what);
  REC_REQUIRE(g != dP && g != loss_part && g != dHi_part && dP != loss_part && dP != dHi_part && loss_part != dHi_part &&
                  pos_r != g && pos_r != dP && pos_r != loss_part && pos_r != dHi_part,
              REC_EINVAL, "%s: the outputs alias each other", what);
  hipLaunchKernelGGL(ef_pos_user_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, (int)max_pos, (int)emb_dim,
                     num_items, neg_weight, ur, p, ld_p, q, ld_q, H_i, G_q, g, pos_r, dP, ld_dp, loss_part, dHi_part, status);
  return check_launch(what);
}

extern "C" int rec_ensfm_pos_item(int64_t batch, int32_t max_pos, int32_t emb_dim, int64_t num_items, float neg_weight,
                                  const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                                  const int32_t* sorted_pos, const float* g, const float* p, int64_t ld_p, const float* q,
                                  int64_t ld_q, const float* H_i, const float* G_p, float* dQ, int64_t ld_dq, void* stream) {
  const char* what = "rec_ensfm_pos_item";
  REC_REQUIRE(batch >= 0 && max_pos >= 1 && num_items >= 1 && num_items < (1ll << 31) - 1, REC_EINVAL,
              "%s: bad sizes (batch %lld, max_pos %d, num_items %lld)", what, (long long)batch, max_pos, (long long)num_items);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(isfinite(neg_weight), REC_EINVAL, "%s: neg_weight must be finite", what);
  REC_REQUIRE(batch * max_pos < (1ll << 31), REC_EINVAL, "%s: batch * max_pos too large", what);
  REC_REQUIRE(ld_p >= emb_dim + 2 && ld_q >= emb_dim + 2 && ld_dq >= emb_dim + 2, REC_EINVAL,
              "%s: a row stride is smaller than emb_dim + 2", what);
  REC_REQUIRE(q && H_i && G_p && dQ, REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(dQ != q && dQ != H_i && dQ != G_p && dQ != p && dQ != g, REC_EINVAL, "%s: dQ aliases an input", what);
  REC_REQUIRE(batch == 0 || (n_uniq && uniq_rows && seg_offset && sorted_pos && g && p), REC_EINVAL, "%s: null pointer argument",
              what);
  if (batch == 0) return REC_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = num_items + 1;                          // the padding row too (movielens_reader.py:66-68)
  hipLaunchKernelGGL(ef_item_gram_kernel, dim3((unsigned)((rows + kEfRows - 1) / kEfRows)), dim3(kBlock), 0, st, rows,
                     (int)emb_dim, neg_weight, q, ld_q, H_i, G_p, dQ, ld_dq);
  int rc = check_launch("rec_ensfm_pos_item (Gram term)");
  if (rc != REC_OK) return rc;
  const int64_t n_pos = batch * max_pos;
  const int64_t blocks = n_pos < num_items ? n_pos : num_items;   // an upper bound of the unique non-padding items
  hipLaunchKernelGGL(ef_pos_item_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, n_pos, (int)max_pos, (int)emb_dim,
                     num_items, n_uniq, uniq_rows, seg_offset, sorted_pos, g, p, ld_p, H_i, dQ, ld_dq);
  return check_launch(what);
}

extern "C" int rec_ensfm_loss(int64_t batch, int32_t emb_dim, float neg_weight, const float* G_p, const float* G_q,
                              const float* H_i, const float* loss_part, const float* dHi_part, float* loss, float* dH_i,
                              void* stream) {
  const char* what = "rec_ensfm_loss";
  REC_REQUIRE(batch >= 0, REC_EINVAL, "%s: batch %lld", what, (long long)batch);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(isfinite(neg_weight), REC_EINVAL, "%s: neg_weight must be finite", what);
  REC_REQUIRE(G_p && G_q && H_i && loss && dH_i, REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(batch == 0 || (loss_part && dHi_part), REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(loss != dH_i && dH_i != H_i && dH_i != G_p && dH_i != G_q && loss != G_p && loss != G_q && loss != H_i &&
                  dH_i != dHi_part && dH_i != loss_part && loss != loss_part && loss != dHi_part,
              REC_EINVAL, "%s: an output aliases an input or the other output", what);
  if (batch == 0) return REC_OK;
  hipLaunchKernelGGL(ef_loss_kernel, dim3((unsigned)(emb_dim + 1)), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)emb_dim,
                     neg_weight, G_p, G_q, H_i, loss_part, dHi_part, loss, dH_i);
  return check_launch(what);
}

extern "C" int rec_ensfm_score(int64_t batch, int64_t num_rows, int32_t emb_dim, const float* p, int64_t ld_p, const float* q,
                               int64_t ld_q, const float* H_i, float* pre, int64_t ld_pre, void* stream) {
  const char* what = "rec_ensfm_score";
  REC_REQUIRE(batch >= 0 && num_rows >= 1, REC_EINVAL, "%s: bad sizes (batch %lld, num_rows %lld)", what, (long long)batch,
              (long long)num_rows);
  REC_REQUIRE(ef_dim_ok(emb_dim), REC_EINVAL, "%s: emb_dim %d outside 1..%d", what, emb_dim, REC_ENSFM_MAX_DIM);
  REC_REQUIRE(ld_p >= emb_dim + 2 && ld_q >= emb_dim + 2 && ld_pre >= num_rows, REC_EINVAL,
              "%s: a row stride is smaller than its row", what);
  const int64_t gx = (num_rows + kEfScoreItems - 1) / kEfScoreItems, gy = (batch + kEfScoreUsers - 1) / kEfScoreUsers;
  REC_REQUIRE(gx < (1ll << 31) && gy < 65536, REC_EINVAL, "%s: batch %lld / num_rows %lld too large (batch <= %d)", what,
              (long long)batch, (long long)num_rows, 65535 * kEfScoreUsers);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(p && q && H_i && pre, REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(pre != p && pre != q && pre != H_i, REC_EINVAL, "%s: pre aliases an input", what);
  const int C = emb_dim + 2;
  const size_t lds = ((size_t)kEfScoreItems * (C | 1) + (size_t)kEfScoreUsers * C) * sizeof(float);
  hipLaunchKernelGGL(ef_score_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), lds, (hipStream_t)stream, batch, num_rows,
                     (int)emb_dim, p, ld_p, q, ld_q, H_i, pre, ld_pre);
  return check_launch(what);
}
