// AutoFIS (rank/autofis), gfx950: the gated, batch-normalised pair term fused into the lookup, its backward in place on the
// layer-0 dX, and the GRDA rule of the gate.
//
//   rec_autofis_plan  <- host only: checks a pair list (0 <= cols[p] < rows[p] < S) and lays out its device image:
//                        cols | rows | per-field adjacency offsets | adjacency entries (partner + 256 * pair), in pair order
//   rec_autofis_fwd   <- X0 = [v_0 | .. | v_{S-1}] (the DNN input), lin = sum_s w[ids], L[b,p] = <v[b,c_p], v[b,r_p]>,
//                        s[b] = lin[b] + sum_p mask_p * BN_p(L[.,p])[b]                            (autofis/net.py:78-99)
//   rec_autofis_bwd   <- d mask, d gamma, d beta of the pair BatchNorm and dX0 += the pair term's gradient, in place
//   rec_grda_step     <- SimpleGrda.step() on one parameter                                     (autofis/optimizer.py:39-60)
// All float32, no float atomics, every reduction in a fixed order: two runs on the same inputs give the same bits.
//
// Forward, training: a block owns a fixed set of chunks of `sb` samples (chunk c of block k: c = k, k + grid, ..).  It
// gathers the chunk's rows into X0 and into an LDS tile of odd pitch, then one thread per pair forms the dot products from
// the tile, writes L and folds them into its column's running (mean, M2) with Welford's update; the blocks' partials are
// merged with Chan's formula in block order.  The variance never passes through sum x^2 - mean^2.  The BatchNorm output is
// not materialised: s[b] = lin[b] + sum_p a_p (L[b,p] - mean_p) + sum_p mask_p beta_p with a_p = mask_p gamma_p invstd_p —
// the centred form of the issue's a_p L + c, which cancels nothing when a column's mean is large against its spread.
// Eval: one launch, the same kernel with the running statistics; the block sums the pair terms itself.
// Backward: T_p = sum_b dz[b] (L[b,p] - mean_p) and S0 = sum_b dz[b] by row blocks, folded in block order; a row kernel
// forms dL in LDS and adds, for every field in its fixed partner order, dL * (the partner's row of X0) onto dX0.
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kAfMaxFields = REC_AUTOFIS_MAX_FIELDS;
constexpr int kAfMaxDim = REC_AUTOFIS_MAX_DIM;
constexpr int kAfMaxPairs = REC_AUTOFIS_MAX_PAIRS;
constexpr int kAfLdsFloats = 4864;                 // 19 KB of dynamic LDS per block: 8 blocks share a CU's 160 KB
constexpr int kAfBwdLdsFloats = 6656;              // 26 KB for the backward's row kernel: 6 blocks per CU
constexpr int kAfBwdMaxBlocks = kNumCU * 6;
constexpr int kAfMaxSb = 4;                        // samples of a chunk
constexpr int kAfFwdMaxBlocks = kNumCU * 8;        // 8 blocks per CU; at most 2048 partial statistics per column
constexpr int kAfColTile = 64;
constexpr int kAfRowLanes = kBlock / kAfColTile;
constexpr int kAfMergeCols = 32;                   // columns of a merge block; kBlock / 32 = 8 groups share the partials
constexpr int kAfMergeGroups = kBlock / kAfMergeCols;
constexpr int kAfMaxRowBlocks = 128;
static_assert(kAfMaxFields <= 256 && kAfMaxPairs == kAfMaxFields * (kAfMaxFields - 1) / 2, "adjacency entry packing");

// fixed-order sum of one value per thread; every thread gets the result (red: kBlock floats)
__device__ __forceinline__ float block_sum(float x, float* red) {
  __syncthreads();
  red[threadIdx.x] = x;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

struct AfFwd {
  int64_t B, N;
  int S, D, P, stride, w_stride, sb, want_L;
  const int64_t* ids;
  const float* V;
  const float* W1;
  const int32_t* plan;          // cols | rows | ..
  const float* gamma;
  const float* beta;
  const float* mask;
  const float* rmean;
  const float* rvar;
  float eps;
  float* X0;
  int64_t ldx;
  float* L;
  int64_t ldl;
  float* s;                     // eval: the result; training: lin
  float* pmean;                 // training: [grid][P] partial means, [grid][P] partial M2, [grid] counts
  float* pm2;
  float* pcnt;
  int32_t* status;
};

template <int VEC, int LANES, bool TRAIN>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(96))) void autofis_fwd_kernel(AfFwd a) {
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[kBlock];
  constexpr int R = kBlock / LANES;
  const int S = a.S, D = a.D, P = a.P, DP = a.D | 1, sb_max = a.sb;
  float* tile = smem;                          // [sb][S][DP]: the chunk's rows, odd pitch
  float* wv = tile + sb_max * S * DP;          // [sb][S]: its first-order weights
  float* st0 = wv + sb_max * S;                // [P]: training: the block's running mean; eval: a_p
  float* st1 = st0 + P;                        // [P]: training: its running M2;           eval: the running mean
  const int32_t* __restrict__ cols = a.plan;
  const int32_t* __restrict__ rows = a.plan + P;
  float cb = 0.f;
  for (int p = threadIdx.x; p < P; p += kBlock) {
    if (TRAIN) {
      st0[p] = 0.f;
      st1[p] = 0.f;
    } else {
      st0[p] = a.mask[p] * a.gamma[p] * (1.f / sqrtf(a.rvar[p] + a.eps));
      st1[p] = a.rmean[p];
      cb += a.mask[p] * a.beta[p];
    }
  }
  if (!TRAIN) cb = block_sum(cb, red);
  const int r = threadIdx.x / LANES, lg = threadIdx.x % LANES;
  const int d0 = lg * VEC;
  const int64_t chunks = (a.B + sb_max - 1) / sb_max;
  int seen = 0;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t b0 = c * sb_max;
    const int nb = (int)(a.B - b0 < sb_max ? a.B - b0 : sb_max);
    if (d0 < D) {
      for (int q = r; q < nb * S; q += R) {
        const int64_t id = a.ids[b0 * S + q];
        float e[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) e[v] = 0.f;
        const bool live = id >= 0 && id < a.N;
        if (live)
          vload<VEC>(e, a.V + id * a.stride + d0);
        else if (lg == 0)
          atomicOr(a.status, REC_FLAG_INDEX_OOB);
        if (lg == 0) wv[q] = live ? a.W1[id * a.w_stride] : 0.f;
        const int k = q / S, s = q - k * S;
        vstore<VEC>(a.X0 + (b0 + k) * a.ldx + (int64_t)s * D + d0, e);
#pragma unroll
        for (int v = 0; v < VEC; ++v) tile[q * DP + d0 + v] = e[v];
      }
    }
    __syncthreads();
    float acc[kAfMaxSb], rcount[kAfMaxSb];
#pragma unroll
    for (int k = 0; k < kAfMaxSb; ++k) {
      acc[k] = 0.f;
      rcount[k] = 1.f / (float)(seen + k + 1);     // uniform: one division per sample, not per pair
    }
    for (int p = threadIdx.x; p < P; p += kBlock) {
      const float* x = tile + cols[p] * DP;
      const float* y = tile + rows[p] * DP;
      float m = st0[p], m2 = st1[p];
#pragma unroll
      for (int k = 0; k < kAfMaxSb; ++k) {
        if (k < nb) {
          float dot = 0.f;
#pragma unroll 4
          for (int d = 0; d < D; ++d) dot += x[k * S * DP + d] * y[k * S * DP + d];
          if (TRAIN || a.want_L) a.L[(b0 + k) * a.ldl + p] = dot;
          if (TRAIN) {                         // Welford: the (seen + k + 1)-th value of this block's column
            const float delta = dot - m;
            m += delta * rcount[k];
            m2 += delta * (dot - m);
          } else {
            acc[k] += m * (dot - m2);
          }
        }
      }
      if (TRAIN) {
        st0[p] = m;
        st1[p] = m2;
      }
    }
    if (TRAIN) {
      if ((int)threadIdx.x < nb) {
        float lin = 0.f;
        for (int s = 0; s < S; ++s) lin += wv[threadIdx.x * S + s];
        a.s[b0 + threadIdx.x] = lin;
      }
    } else {
#pragma unroll
      for (int k = 0; k < kAfMaxSb; ++k) {
        if (k < nb) {                          // uniform
          const float fm = block_sum(acc[k], red);
          if (threadIdx.x == 0) {
            float lin = 0.f;
            for (int s = 0; s < S; ++s) lin += wv[k * S + s];
            a.s[b0 + k] = lin + fm + cb;
          }
        }
      }
    }
    seen += nb;
    __syncthreads();                           // the next chunk overwrites the tile
  }
  if (TRAIN) {
    for (int p = threadIdx.x; p < P; p += kBlock) {
      a.pmean[(int64_t)blockIdx.x * P + p] = st0[p];
      a.pm2[(int64_t)blockIdx.x * P + p] = st1[p];
    }
    if (threadIdx.x == 0) a.pcnt[blockIdx.x] = (float)seen;
  }
}

// Chan, Golub & LeVeque: (n, mean, M2) of the union of two sample sets
__device__ __forceinline__ void chan_merge(float& n, float& m, float& M2, float nb, float mb, float M2b) {
  if (nb == 0.f) return;
  const float nn = n + nb, delta = mb - m, f = nb / nn;
  m += delta * f;
  M2 += M2b + delta * delta * n * f;
  n = nn;
}

// Column p: the blocks' partials merged in block order (8 contiguous runs, then the runs in order) -> save_mean,
// save_invstd, the running statistics, a_p = mask gamma invstd; block 0 also writes c = sum_p mask_p beta_p.
__global__ __launch_bounds__(kBlock) void autofis_merge_kernel(int64_t B, int P, int G, const float* __restrict__ pmean,
                                                               const float* __restrict__ pm2,
                                                               const float* __restrict__ pcnt,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               const float* __restrict__ mask, float* rmean, float* rvar,
                                                               float momentum, float eps, float* __restrict__ save_mean,
                                                               float* __restrict__ save_invstd, float* __restrict__ coef_a,
                                                               float* __restrict__ cval) {
  __shared__ float sn[kAfMergeGroups][kAfMergeCols], sm[kAfMergeGroups][kAfMergeCols], s2[kAfMergeGroups][kAfMergeCols];
  __shared__ float red[kBlock];
  const int pl = threadIdx.x % kAfMergeCols, grp = threadIdx.x / kAfMergeCols;
  const int p = blockIdx.x * kAfMergeCols + pl;
  const int per = (G + kAfMergeGroups - 1) / kAfMergeGroups;
  float n = 0.f, m = 0.f, M2 = 0.f;
  if (p < P) {
    const int g1 = (grp + 1) * per < G ? (grp + 1) * per : G;
#pragma unroll 4
    for (int g = grp * per; g < g1; ++g) chan_merge(n, m, M2, pcnt[g], pmean[(int64_t)g * P + p], pm2[(int64_t)g * P + p]);
  }
  sn[grp][pl] = n;
  sm[grp][pl] = m;
  s2[grp][pl] = M2;
  __syncthreads();
  if (grp == 0 && p < P) {
    for (int i = 1; i < kAfMergeGroups; ++i) chan_merge(n, m, M2, sn[i][pl], sm[i][pl], s2[i][pl]);
    const float var = M2 / (float)B;                     // biased
    const float is = 1.f / sqrtf(var + eps);
    save_mean[p] = m;
    save_invstd[p] = is;
    if (rmean) rmean[p] = momentum * rmean[p] + (1.f - momentum) * m;
    if (rvar) rvar[p] = momentum * rvar[p] + (1.f - momentum) * var;
    coef_a[p] = mask[p] * gamma[p] * is;
  }
  if (blockIdx.x == 0) {
    float cb = 0.f;
    for (int q = threadIdx.x; q < P; q += kBlock) cb += mask[q] * beta[q];
    cb = block_sum(cb, red);
    if (threadIdx.x == 0) cval[0] = cb;
  }
}

// s[b] = lin[b] + sum_p a_p (L[b,p] - mean_p) + c, in place on s: one wave per row, lanes stride the row
__global__ __launch_bounds__(kBlock) void autofis_rows_kernel(int64_t B, int P, const float* __restrict__ L, int64_t ldl,
                                                              const float* __restrict__ coef_a,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ cval, float* __restrict__ s) {
  const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= B) return;
  const float* l = L + row * ldl;
  float acc = 0.f;
  for (int p = lane; p < P; p += kWave) acc += coef_a[p] * (l[p] - mean[p]);
  acc = group_sum<kWave>(acc);
  if (lane == 0) s[row] = s[row] + acc + cval[0];
}

// part[y][p] = sum over row block y of dz[b] (L[b,p] - mean_p); ps0[y] = its sum of dz
__global__ __launch_bounds__(kBlock) void autofis_bwd_reduce_kernel(int64_t B, int P, const float* __restrict__ L,
                                                                    int64_t ldl, const float* __restrict__ dz,
                                                                    const float* __restrict__ mean,
                                                                    float* __restrict__ part, float* __restrict__ ps0) {
  __shared__ float red[2][kAfRowLanes][kAfColTile];
  const int pl = threadIdx.x % kAfColTile, rl = threadIdx.x / kAfColTile;
  const int p = blockIdx.x * kAfColTile + pl;
  const bool on = p < P;
  const float mu = on ? mean[p] : 0.f;
  const int64_t per = (B + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < B ? r0 + per : B;
  float t[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t r = r0 + rl;
  for (; r + 3 * kAfRowLanes < r1; r += 4 * kAfRowLanes) {
    float x[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = on ? L[(r + u * kAfRowLanes) * ldl + p] : 0.f;
      g[u] = dz[r + u * kAfRowLanes];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      t[u] += g[u] * (x[u] - mu);
      z[u] += g[u];
    }
  }
  for (int u = 0; r < r1; r += kAfRowLanes, ++u) {
    const float g = dz[r];
    t[u] += g * ((on ? L[r * ldl + p] : 0.f) - mu);
    z[u] += g;
  }
  red[0][rl][pl] = (t[0] + t[1]) + (t[2] + t[3]);
  red[1][rl][pl] = (z[0] + z[1]) + (z[2] + z[3]);
  __syncthreads();
  if (rl == 0) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < kAfRowLanes; ++i) {
      s0 += red[0][i][pl];
      s1 += red[1][i][pl];
    }
    if (on) part[(int64_t)blockIdx.y * P + p] = s0;
    if (blockIdx.x == 0 && pl == 0) ps0[blockIdx.y] = s1;
  }
}

// The row blocks' partials added in block order -> d mask, d gamma, d beta and the row kernel's coefficients:
// a_p = gamma invstd mask, q_p = invstd S1_p / B, cz = S0 / B.   GY == 0 (an empty batch) writes zero gradients.
__global__ __launch_bounds__(kBlock) void autofis_bwd_finalize_kernel(int64_t B, int P, int GY,
                                                                      const float* __restrict__ part,
                                                                      const float* __restrict__ ps0,
                                                                      const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta,
                                                                      const float* __restrict__ mask,
                                                                      const float* __restrict__ invstd,
                                                                      float* __restrict__ d_mask, float* __restrict__ d_gamma,
                                                                      float* __restrict__ d_beta, float* __restrict__ coef_a,
                                                                      float* __restrict__ coef_q, float* __restrict__ cz) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  float T = 0.f, S0 = 0.f;
  for (int g = 0; g < GY; ++g) {
    T += part[(int64_t)g * P + p];
    S0 += ps0[g];
  }
  const float is = GY > 0 ? invstd[p] : 0.f;
  const float S1 = is * T;
  d_mask[p] = gamma[p] * S1 + beta[p] * S0;
  d_gamma[p] = mask[p] * S1;
  d_beta[p] = mask[p] * S0;
  if (GY > 0) {
    coef_a[p] = gamma[p] * is * mask[p];
    coef_q[p] = is * S1 / (float)B;
    if (p == 0) cz[0] = S0 / (float)B;
  }
}

// dL[b,p] = a_p (dz[b] - cz - (L[b,p] - mean_p) q_p) in LDS, then for every float of a field f of the block's samples
// dX[b,f,d] += sum over f's pairs, in pair order, of dL[b,pair] * X0[b,partner,d].  A field in no pair is not written.
// The adjacency is copied to LDS once per block; a thread owns the floats d, d + DQ, d + 2 DQ, d + 3 DQ (DQ = ceil(D / 4))
// of one field, so an adjacency entry and a dL value are read once for four products.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(96))) void autofis_bwd_rows_kernel(
    int64_t B, int S, int D, int P, int sb_max,
                                                                  const int32_t* __restrict__ plan,
                                                                  const float* __restrict__ X0, int64_t ldx,
                                                                  const float* __restrict__ L, int64_t ldl,
                                                                  const float* __restrict__ dz,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ coef_a,
                                                                  const float* __restrict__ coef_q,
                                                                  const float* __restrict__ cz, float* __restrict__ dX,
                                                                  int64_t lddx) {
  extern __shared__ __align__(16) float smem[];
  const int DP = D | 1, SD = S * D, DQ = (D + 3) / 4;
  float* tile = smem;                          // [sb][S][DP]
  float* dl = tile + sb_max * S * DP;          // [sb][P]
  int* sadj = (int*)(dl + sb_max * P);         // [2P]: partner + 256 * pair, by field
  int* soff = sadj + 2 * P;                    // [S + 1]
  for (int i = threadIdx.x; i < 2 * P; i += kBlock) sadj[i] = plan[2 * P + S + 1 + i];
  for (int i = threadIdx.x; i <= S; i += kBlock) soff[i] = plan[2 * P + i];
  const float c0 = cz[0];
  const int64_t chunks = (B + sb_max - 1) / sb_max;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t b0 = c * sb_max;
    const int nb = (int)(B - b0 < sb_max ? B - b0 : sb_max);
    for (int it = threadIdx.x; it < nb * SD; it += kBlock) {
      const int k = it / SD, rem = it - k * SD;
      const int f = rem / D, d = rem - f * D;
      tile[(k * S + f) * DP + d] = X0[(b0 + k) * ldx + rem];
    }
    for (int it = threadIdx.x; it < nb * P; it += kBlock) {
      const int k = it / P, p = it - k * P;
      dl[it] = coef_a[p] * (dz[b0 + k] - c0 - (L[(b0 + k) * ldl + p] - mean[p]) * coef_q[p]);
    }
    __syncthreads();                           // also orders the adjacency's stores before their first use
    for (int it = threadIdx.x; it < nb * S * DQ; it += kBlock) {
      const int k = it / (S * DQ), rem = it - k * S * DQ;
      const int f = rem / DQ, q = rem - f * DQ;
      const int e0 = soff[f], e1 = soff[f + 1];
      if (e0 == e1) continue;
      const float* t = tile + k * S * DP + q;  // t[.. + 3 DQ] may pass the row's D floats by at most 2: still inside smem
      const float* g = dl + k * P;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int e = e0; e < e1; ++e) {
        const int w = sadj[e];
        const float gv = g[w >> 8];
        const float* tp = t + (w & 255) * DP;
        a0 += gv * tp[0];
        a1 += gv * tp[DQ];
        a2 += gv * tp[2 * DQ];
        a3 += gv * tp[3 * DQ];
      }
      float* o = dX + (b0 + k) * lddx + f * D + q;
      o[0] += a0;
      if (q + DQ < D) o[DQ] += a1;
      if (q + 2 * DQ < D) o[2 * DQ] += a2;
      if (q + 3 * DQ < D) o[3 * DQ] += a3;
    }
    __syncthreads();                           // the next chunk overwrites the LDS
  }
}

// SimpleGrda.step() on one element (optimizer.py:47-55), rounding points pinned:
//   a <- a + first_iter * p - lr * g;  p <- sign(a) * max(|a| - l1, 0)
__global__ __launch_bounds__(kBlock) void grda_kernel(int64_t n, float* __restrict__ p, float* __restrict__ acc,
                                                      const float* __restrict__ g, float lr, float l1, float first_iter) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float fp = first_iter * p[i];
  const float lg = lr * g[i];
  const float a = (acc[i] + fp) - lg;
  const float sh = fmaxf(fabsf(a) - l1, 0.f);
  acc[i] = a;
  p[i] = (a > 0.f ? 1.f : a < 0.f ? -1.f : 0.f) * sh;
}

int af_fwd_sb(int S, int D, int P) {
  const int per = S * (D | 1) + S;
  const int room = kAfLdsFloats - 2 * P;
  const int sb = room > 0 ? room / per : 0;
  return sb < 1 ? 1 : sb > kAfMaxSb ? kAfMaxSb : sb;
}

int af_bwd_sb(int S, int D, int P) {
  const int room = kAfBwdLdsFloats - 2 * P - S - 1;
  const int sb = room > 0 ? room / (S * (D | 1) + P) : 0;
  return sb < 1 ? 1 : sb > kAfMaxSb ? kAfMaxSb : sb;
}

int64_t af_fwd_grid(int64_t B, int sb) {           // a function of the shape alone: the sample sets of the partials are fixed
  const int64_t chunks = (B + sb - 1) / sb;
  return chunks < kAfFwdMaxBlocks ? chunks : kAfFwdMaxBlocks;
}

int af_row_blocks(int64_t B) {
  const int64_t g = (B + 127) / 128;
  return (int)(g < 1 ? 1 : g > kAfMaxRowBlocks ? kAfMaxRowBlocks : g);
}

int af_check_sizes(int64_t B, int32_t S, int32_t D, int32_t P) {
  REC_REQUIRE(B >= 0 && S >= 2 && S <= kAfMaxFields && D >= 1 && D <= kAfMaxDim, REC_EINVAL,
              "autofis: bad sizes (batch %lld, num_fields %d (2..%d), emb_dim %d (1..%d))", (long long)B, S, kAfMaxFields,
              D, kAfMaxDim);
  REC_REQUIRE(P >= 1 && P <= kAfMaxPairs && P <= S * (S - 1) / 2, REC_EINVAL,
              "autofis: num_pairs %d must be 1 .. min(%d, num_fields (num_fields - 1) / 2 = %d)", P, kAfMaxPairs,
              S * (S - 1) / 2);
  REC_REQUIRE(B * (int64_t)(S > P ? S : P) < (1ll << 31), REC_ESHAPE, "autofis: batch * max(num_fields, num_pairs) too large");
  return REC_OK;
}

int af_check_pairs(int32_t S, int32_t P, const int32_t* cols, const int32_t* rows) {
  REC_REQUIRE(cols && rows, REC_EINVAL, "autofis: cols / rows is null");
  for (int p = 0; p < P; ++p)
    REC_REQUIRE(cols[p] >= 0 && cols[p] < rows[p] && rows[p] < S, REC_EINVAL,
                "autofis: pair %d = (%d, %d) must satisfy 0 <= col < row < num_fields = %d", p, cols[p], rows[p], S);
  return REC_OK;
}

size_t af_fwd_ws_floats(int64_t B, int S, int D, int P) {
  const int64_t grid = af_fwd_grid(B, af_fwd_sb(S, D, P));
  return (size_t)grid * (2 * (size_t)P + 1) + (size_t)P + 4;      // partial means, M2, counts | a_p | c
}

size_t af_bwd_ws_floats(int64_t B, int P) {
  return (size_t)af_row_blocks(B) * ((size_t)P + 1) + 2 * (size_t)P + 4;      // partials, dz partials | a_p, q_p | cz
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_autofis_plan_ints(int32_t num_fields, int32_t num_pairs, size_t* ints) {
  REC_REQUIRE(ints, REC_EINVAL, "null pointer argument");
  int rc = af_check_sizes(0, num_fields, 1, num_pairs);
  if (rc != REC_OK) return rc;
  *ints = 4 * (size_t)num_pairs + (size_t)num_fields + 1;
  return REC_OK;
}

extern "C" int rec_autofis_plan(int32_t num_fields, int32_t num_pairs, const int32_t* cols, const int32_t* rows,
                                int32_t* plan) {
  int rc = af_check_sizes(0, num_fields, 1, num_pairs);
  if (rc != REC_OK) return rc;
  rc = af_check_pairs(num_fields, num_pairs, cols, rows);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(plan, REC_EINVAL, "null pointer argument");
  const int S = num_fields, P = num_pairs;
  int32_t* off = plan + 2 * P;
  int32_t* adj = off + S + 1;
  for (int p = 0; p < P; ++p) {
    plan[p] = cols[p];
    plan[P + p] = rows[p];
  }
  for (int f = 0; f <= S; ++f) off[f] = 0;
  for (int p = 0; p < P; ++p) {
    ++off[cols[p] + 1];
    ++off[rows[p] + 1];
  }
  for (int f = 0; f < S; ++f) off[f + 1] += off[f];
  int32_t fill[kAfMaxFields];
  for (int f = 0; f < S; ++f) fill[f] = off[f];
  for (int p = 0; p < P; ++p) {                      // pair order = the partner order of every field
    adj[fill[cols[p]]++] = rows[p] + 256 * p;
    adj[fill[rows[p]]++] = cols[p] + 256 * p;
  }
  return REC_OK;
}

extern "C" int rec_autofis_fwd_workspace_bytes(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs,
                                               size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = af_check_sizes(batch, num_fields, emb_dim, num_pairs);
  if (rc != REC_OK) return rc;
  *bytes = af_fwd_ws_floats(batch, num_fields, emb_dim, num_pairs) * sizeof(float);
  return REC_OK;
}

extern "C" int rec_autofis_fwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int32_t w_stride,
                               int64_t num_rows, const int64_t* ids, const float* V, const float* W1, int32_t num_pairs,
                               const int32_t* cols, const int32_t* rows, const int32_t* plan_dev, const float* gamma,
                               const float* beta, const float* mask, float* running_mean, float* running_var,
                               float momentum, float eps, int32_t training, int32_t want_L, float* X0, int64_t x0_stride,
                               float* L, int64_t l_stride, float* s, float* save_mean, float* save_invstd,
                               int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = af_check_sizes(batch, num_fields, emb_dim, num_pairs);
  if (rc != REC_OK) return rc;
  rc = af_check_pairs(num_fields, num_pairs, cols, rows);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(row_stride >= emb_dim && w_stride >= 1 && num_rows > 0, REC_EINVAL,
              "autofis: bad tables (row_stride %d, w_stride %d, num_rows %lld)", row_stride, w_stride, (long long)num_rows);
  REC_REQUIRE(x0_stride >= (int64_t)num_fields * emb_dim, REC_EINVAL, "autofis: x0_stride %lld < num_fields * emb_dim",
              (long long)x0_stride);
  const bool writes_L = training || want_L;
  REC_REQUIRE(!writes_L || l_stride >= num_pairs, REC_EINVAL, "autofis: l_stride %lld < num_pairs %d", (long long)l_stride,
              num_pairs);
  REC_REQUIRE(eps > 0.f, REC_EINVAL, "autofis: eps %g must be positive", (double)eps);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(ids && V && W1 && plan_dev && gamma && beta && mask && X0 && s && status, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(!writes_L || L, REC_EINVAL, "autofis: L is null");
  REC_REQUIRE(running_mean && running_var, REC_EINVAL, "autofis: the running statistics are null");
  const int S = num_fields, D = emb_dim, P = num_pairs;
  const int sb = af_fwd_sb(S, D, P);
  const size_t lds = ((size_t)sb * (S * (D | 1) + S) + 2 * (size_t)P) * sizeof(float);
  REC_REQUIRE(lds <= 64 * 1024, REC_ESHAPE, "autofis: %zu bytes of LDS for one sample exceed 64 KB", lds);
  hipStream_t st = (hipStream_t)stream;
  AfFwd a;
  a.B = batch; a.N = num_rows; a.S = S; a.D = D; a.P = P; a.stride = row_stride; a.w_stride = w_stride; a.sb = sb;
  a.want_L = want_L; a.ids = ids; a.V = V; a.W1 = W1; a.plan = plan_dev; a.gamma = gamma; a.beta = beta; a.mask = mask;
  a.rmean = running_mean; a.rvar = running_var; a.eps = eps; a.X0 = X0; a.ldx = x0_stride; a.L = L; a.ldl = l_stride;
  a.s = s; a.pmean = a.pm2 = a.pcnt = nullptr; a.status = status;
  const bool vec = ((uintptr_t)V) % 16 == 0 && row_stride % 4 == 0 && ((uintptr_t)X0) % 16 == 0 && x0_stride % 4 == 0;
  const int64_t chunks = (batch + sb - 1) / sb;
  if (!training) {
    return dispatch_row_shape(D, vec ? row_stride : row_stride | 1, [&](auto vec_, auto lanes) -> int {
      constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
      const int64_t grid = chunks < kNumCU * 8 ? chunks : kNumCU * 8;
      hipLaunchKernelGGL((autofis_fwd_kernel<VEC, LANES, false>), dim3((unsigned)grid), dim3(kBlock), lds, st, a);
      return check_launch("rec_autofis_fwd (eval)");
    });
  }
  REC_REQUIRE(save_mean && save_invstd, REC_EINVAL, "null pointer argument");
  const int64_t grid = af_fwd_grid(batch, sb);
  const size_t need = af_fwd_ws_floats(batch, S, D, P) * sizeof(float);
  REC_REQUIRE(workspace && workspace_bytes >= need, REC_EWORKSPACE, "autofis fwd workspace %zu < %zu bytes",
              workspace_bytes, need);
  float* w = (float*)workspace;
  a.pmean = w;
  a.pm2 = w + (size_t)grid * P;
  a.pcnt = w + (size_t)grid * 2 * P;
  float* coef_a = a.pcnt + grid;
  float* cval = coef_a + P;
  rc = dispatch_row_shape(D, vec ? row_stride : row_stride | 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    hipLaunchKernelGGL((autofis_fwd_kernel<VEC, LANES, true>), dim3((unsigned)grid), dim3(kBlock), lds, st, a);
    return check_launch("rec_autofis_fwd");
  });
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(autofis_merge_kernel, dim3((P + kAfMergeCols - 1) / kAfMergeCols), dim3(kBlock), 0, st, batch, P,
                     (int)grid, a.pmean, a.pm2, a.pcnt, gamma, beta, mask, running_mean, running_var, momentum, eps,
                     save_mean, save_invstd, coef_a, cval);
  const int64_t rb = (batch + kBlock / kWave - 1) / (kBlock / kWave);
  hipLaunchKernelGGL(autofis_rows_kernel, dim3((unsigned)rb), dim3(kBlock), 0, st, batch, P, L, l_stride, coef_a,
                     save_mean, cval, s);
  return check_launch("rec_autofis_fwd (rows)");
}

extern "C" int rec_autofis_bwd_workspace_bytes(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs,
                                               size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = af_check_sizes(batch, num_fields, emb_dim, num_pairs);
  if (rc != REC_OK) return rc;
  *bytes = af_bwd_ws_floats(batch, num_pairs) * sizeof(float);
  return REC_OK;
}

extern "C" int rec_autofis_bwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs, const int32_t* cols,
                               const int32_t* rows, const int32_t* plan_dev, const float* dz, const float* L,
                               int64_t l_stride, const float* X0, int64_t x0_stride, const float* save_mean,
                               const float* save_invstd, const float* gamma, const float* beta, const float* mask,
                               float* dX, int64_t dx_stride, float* d_mask, float* d_gamma, float* d_beta, void* workspace,
                               size_t workspace_bytes, void* stream) {
  int rc = af_check_sizes(batch, num_fields, emb_dim, num_pairs);
  if (rc != REC_OK) return rc;
  rc = af_check_pairs(num_fields, num_pairs, cols, rows);
  if (rc != REC_OK) return rc;
  const int S = num_fields, D = emb_dim, P = num_pairs;
  REC_REQUIRE(l_stride >= P && x0_stride >= (int64_t)S * D && dx_stride >= (int64_t)S * D, REC_EINVAL,
              "autofis: l_stride %lld < num_pairs, or x0_stride %lld / dx_stride %lld < num_fields * emb_dim",
              (long long)l_stride, (long long)x0_stride, (long long)dx_stride);
  REC_REQUIRE(gamma && beta && mask && d_mask && d_gamma && d_beta, REC_EINVAL, "null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  const unsigned fb = (P + kBlock - 1) / kBlock;
  if (batch == 0) {                                  // empty batch sums
    hipLaunchKernelGGL(autofis_bwd_finalize_kernel, dim3(fb), dim3(kBlock), 0, st, batch, P, 0, (const float*)nullptr,
                       (const float*)nullptr, gamma, beta, mask, (const float*)nullptr, d_mask, d_gamma, d_beta,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr);
    return check_launch("rec_autofis_bwd (finalize)");
  }
  REC_REQUIRE(plan_dev && dz && L && X0 && save_mean && save_invstd && dX, REC_EINVAL, "null pointer argument");
  REC_REQUIRE((const float*)dX != X0 && (const float*)dX != L, REC_EINVAL, "autofis: dX must not be X0 or L");
  const size_t need = af_bwd_ws_floats(batch, P) * sizeof(float);
  REC_REQUIRE(workspace && workspace_bytes >= need, REC_EWORKSPACE, "autofis bwd workspace %zu < %zu bytes",
              workspace_bytes, need);
  const int sb = af_bwd_sb(S, D, P);
  const size_t lds = ((size_t)sb * (S * (D | 1) + P) + 2 * (size_t)P + S + 1) * sizeof(float);
  REC_REQUIRE(lds <= 64 * 1024, REC_ESHAPE, "autofis: %zu bytes of LDS for one sample exceed 64 KB", lds);
  const int gy = af_row_blocks(batch);
  float* part = (float*)workspace;
  float* ps0 = part + (size_t)gy * P;
  float* coef_a = ps0 + gy;
  float* coef_q = coef_a + P;
  float* cz = coef_q + P;
  hipLaunchKernelGGL(autofis_bwd_reduce_kernel, dim3((P + kAfColTile - 1) / kAfColTile, gy), dim3(kBlock), 0, st, batch, P,
                     L, l_stride, dz, save_mean, part, ps0);
  hipLaunchKernelGGL(autofis_bwd_finalize_kernel, dim3(fb), dim3(kBlock), 0, st, batch, P, gy, part, ps0, gamma, beta, mask,
                     save_invstd, d_mask, d_gamma, d_beta, coef_a, coef_q, cz);
  const int64_t bchunks = (batch + sb - 1) / sb;
  const int64_t grid = bchunks < kAfBwdMaxBlocks ? bchunks : kAfBwdMaxBlocks;
  hipLaunchKernelGGL(autofis_bwd_rows_kernel, dim3((unsigned)grid), dim3(kBlock), lds, st, batch, S, D, P, sb, plan_dev, X0,
                     x0_stride, L, l_stride, dz, save_mean, coef_a, coef_q, cz, dX, dx_stride);
  return check_launch("rec_autofis_bwd");
}

extern "C" int rec_grda_step(int64_t n, float* p, float* acc, const float* g, float lr, float l1_accumulation,
                             int32_t first_iter, void* stream) {
  REC_REQUIRE(n >= 0 && l1_accumulation >= 0.f && (first_iter == 0 || first_iter == 1), REC_EINVAL,
              "rec_grda_step: bad arguments (n %lld, l1_accumulation %g, first_iter %d)", (long long)n,
              (double)l1_accumulation, first_iter);
  if (n == 0) return REC_OK;
  REC_REQUIRE(p && acc && g, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(p != acc && (const float*)p != g && (const float*)acc != g, REC_EINVAL,
              "rec_grda_step: p, acc and g must be three buffers");
  const int64_t grid = (n + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_grda_step: n too large");
  hipLaunchKernelGGL(grda_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, n, p, acc, g, lr,
                     l1_accumulation, (float)first_iter);
  return check_launch("rec_grda_step");
}
