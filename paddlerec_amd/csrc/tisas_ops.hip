// TiSASRec (recall/tisas, time-interval-aware self-attention) on gfx950.
//
//   rec_tisas_attn_fwd / _bwd            <- tisas/net.py:85-164 TimeAwareMultiHeadAttention after Q_w / K_w / V_w: every score
//                                           and every output carries a row of a small table picked by tm[b,i,j].  The
//                                           reference gathers the tables into two [B, L, L, D] tensors; here the rows are
//                                           read from the tables per (i, j) (51 KB each at the shipped shape: they stay in
//                                           L2), forward and backward.
//   rec_affine_layer_norm_fwd / _bwd     <- paddle.nn.LayerNorm(hidden, epsilon=1e-8) with the residual add and the
//                                           padding mask in front of it (net.py:273-287)
//   rec_tisas_embed_fwd / _bwd           <- net.py:245-247,263: item_emb * sqrt(D), dropout, * (log_seqs != 0)
//   rec_tisas_head                       <- net.py:305-308, dygraph_model.py:42-53: both dots, the masked BCE means, d(feats)
//
// Attention.  A block is 16 query rows of one (sample, head); the head's keys and values of the sample, position rows
// added (after their dropout), sit in LDS, rows padded to an odd stride.  A wave takes one query row at a time in two
// roles: lane = key j for the scores (a dot product per lane, no cross-lane sum; the time row of (i, j) is gathered by the
// lane), then lane = feature d for the output (the weights are broadcast from LDS, keys ascending).  The backward has the
// same shape: the query pass recomputes the weights from lse, renormalises them by their own sum (lse of a padded row is
// -2^32 + log L, which rounds to -2^32), and writes dQ and the two score-shaped arrays gs = scale dS and ga = dropped
// weights; the key pass forms dK and dV from them (queries ascending); the position tables sum dK / dV over the batch in
// ascending sample order; the time tables take LDS tiles: a block owns a range of samples and a head, its wave w owns the
// table rows t with t % 4 == w and adds the hits of its rows in ascending (b, i, j), then one fold adds the blocks' tiles
// in ascending order.  No float atomics anywhere: a rerun is bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kTsRows = 16;                        // query (key) rows of a block
constexpr int kTsWaves = kBlock / kWave;           // 4
constexpr int kTsRowsPerWave = kTsRows / kTsWaves;
constexpr int kTsMaxL = REC_TISAS_MAX_L;
constexpr int kTsKeysPerLane = kTsMaxL / kWave;    // 2
constexpr int kTsMaxHead = REC_TISAS_MAX_HEAD;
constexpr float kTsNeg = -4294967295.0f;           // -2**32 + 1 in float32 (net.py:141)
constexpr int kLnRows = kBlock / kWave;

struct TsArgs {
  int L, H, hd, D, T;
  const float* q;
  const float* k;
  const float* v;
  int64_t ldq, ldk, ldv;
  const float* pos_k;
  const float* pos_v;
  const float* time_k;
  const float* time_v;
  const int64_t* tm;
  const int64_t* log_seqs;
  float scale;
  int drop_a, drop_p, drop_t;
  uint32_t th_a, th_p, th_t;
  float ik_a, ik_p, ik_t;
  uint64_t key_a, key_pk, key_pv, key_tk, key_tv;
};

__device__ __forceinline__ bool ts_keep(uint64_t key, uint32_t thresh, uint64_t e) {
  return (uint32_t)(mix64(key + e) >> 32) >= thresh;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, kWave));
  return x;
}

// keys + dropped position rows of (sample b, head h) -> sK, sV [L][ldt]
__device__ __forceinline__ void ts_stage_kv(const TsArgs& a, int b, int h, int ldt, float* sK, float* sV) {
  const int64_t row0 = (int64_t)b * a.L;
  for (int idx = threadIdx.x; idx < a.L * a.hd; idx += kBlock) {
    const int j = idx / a.hd, d = idx - j * a.hd, col = h * a.hd + d;
    float pk = a.pos_k[j * a.D + col], pv = a.pos_v[j * a.D + col];
    if (a.drop_p) {
      const uint64_t e = (uint64_t)(row0 + j) * a.D + col;
      pk = ts_keep(a.key_pk, a.th_p, e) ? pk * a.ik_p : 0.f;
      pv = ts_keep(a.key_pv, a.th_p, e) ? pv * a.ik_p : 0.f;
    }
    sK[j * ldt + d] = a.k[(row0 + j) * a.ldk + col] + pk;
    sV[j * ldt + d] = a.v[(row0 + j) * a.ldv + col] + pv;
  }
}

// one element of a dropped time row: table[t, col] through the mask of element ((b L + i) L + j, col)
__device__ __forceinline__ float ts_time(const TsArgs& a, const float* table, uint64_t key, int t, uint64_t pair, int col) {
  float x = table[(int64_t)t * a.D + col];
  if (a.drop_t) x = ts_keep(key, a.th_t, pair * a.D + col) ? x * a.ik_t : 0.f;
  return x;
}

// the same from an LDS copy [T][hd] of the head's slice (REC_TISAS_TIME_LDS, a measurement build of the forward: DESIGN.md)
__device__ __forceinline__ float ts_time_lds(const TsArgs& a, const float* tile, uint64_t key, int t, uint64_t pair, int d, int col) {
  float x = tile[t * a.hd + d];
  if (a.drop_t) x = ts_keep(key, a.th_t, pair * a.D + col) ? x * a.ik_t : 0.f;
  return x;
}

// LDS of the two query-row kernels: sK, sV [L][ldt], then per wave q [64], g [64], weights [kTsMaxL], tm ids [kTsMaxL]
__host__ __device__ inline size_t ts_lds_bytes(int L, int hd) {
  return ((size_t)2 * L * (hd | 1) + (size_t)kTsWaves * (2 * kTsMaxHead + 2 * kTsMaxL)) * sizeof(float);
}

// grid (B H, ceil(L / 16))
__global__ __launch_bounds__(kBlock) void ts_attn_fwd_kernel(TsArgs a, float* __restrict__ out, int64_t ldo,
                                                             float* __restrict__ lse, int32_t* __restrict__ status) {
  extern __shared__ float smem[];
  const int ldt = a.hd | 1;
  float* sK = smem;
  float* sV = sK + a.L * ldt;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  float* sQ = sV + a.L * ldt + w * kTsMaxHead;
  float* sA = sV + a.L * ldt + kTsWaves * 2 * kTsMaxHead + w * kTsMaxL;
  int* sT = reinterpret_cast<int*>(sV + a.L * ldt + kTsWaves * 2 * kTsMaxHead + kTsWaves * kTsMaxL) + w * kTsMaxL;
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int64_t row0 = (int64_t)b * a.L;
  ts_stage_kv(a, b, h, ldt, sK, sV);
#ifdef REC_TISAS_TIME_LDS                                        // measurement build: the head's slice of both time tables in LDS
  float* sTK = reinterpret_cast<float*>(sT - w * kTsMaxL + kTsWaves * kTsMaxL);
  float* sTV = sTK + a.T * a.hd;
  for (int idx = threadIdx.x; idx < a.T * a.hd; idx += kBlock) {
    const int t = idx / a.hd, d = idx - t * a.hd;
    sTK[idx] = a.time_k[(int64_t)t * a.D + h * a.hd + d];
    sTV[idx] = a.time_v[(int64_t)t * a.D + h * a.hd + d];
  }
#define TS_FWD_TK(t, pair, d) ts_time_lds(a, sTK, a.key_tk, t, pair, d, h * a.hd + (d))
#define TS_FWD_TV(t, pair, d) ts_time_lds(a, sTV, a.key_tv, t, pair, d, h * a.hd + (d))
#else
#define TS_FWD_TK(t, pair, d) ts_time(a, a.time_k, a.key_tk, t, pair, h * a.hd + (d))
#define TS_FWD_TV(t, pair, d) ts_time(a, a.time_v, a.key_tv, t, pair, h * a.hd + (d))
#endif
  bool bad = false;
  for (int r = 0; r < kTsRowsPerWave; ++r) {
    const int i = blockIdx.y * kTsRows + w * kTsRowsPerWave + r;
    const bool valid = i < a.L;
    const int ic = valid ? i : a.L - 1;                       // a row past L repeats row L-1 and stores nothing
    __syncthreads();                                          // the stage above / the previous row's reads
    if (lane < a.hd) sQ[lane] = a.q[(row0 + ic) * a.ldq + h * a.hd + lane];
    const uint64_t pair0 = (uint64_t)(row0 + ic) * a.L;
    for (int j = lane; j < a.L; j += kWave) {
      const int64_t t = a.tm[pair0 + j];
      const bool ok = t >= 0 && t < a.T;
      bad |= !ok;
      sT[j] = ok ? (int)t : 0;
    }
    __syncthreads();
    const bool padded = a.log_seqs[row0 + ic] == 0;
    float sc[kTsKeysPerLane];
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      const int j = lane + kWave * u;
      float s = -INFINITY;
      if (j < a.L) {
        if (padded || j > ic) {
          s = kTsNeg;
        } else {
          const int t = sT[j];
          s = 0.f;
          for (int d = 0; d < a.hd; ++d)
            s = fmaf(sQ[d], sK[j * ldt + d] + TS_FWD_TK(t, pair0 + j, d), s);
          s *= a.scale;
        }
      }
      sc[u] = s;
    }
    float m = sc[0];
#pragma unroll
    for (int u = 1; u < kTsKeysPerLane; ++u) m = fmaxf(m, sc[u]);
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      sc[u] = expf(sc[u] - m);                                // 0 past L
      sum += sc[u];
    }
    sum = group_sum<kWave>(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      const int j = lane + kWave * u;
      if (j < a.L) {
        float p = sc[u] * inv;
        if (a.drop_a) p = ts_keep(a.key_a, a.th_a, ((uint64_t)bh * a.L + ic) * a.L + j) ? p * a.ik_a : 0.f;
        sA[j] = p;
      }
    }
    __syncthreads();
    if (valid && lane < a.hd) {
      const int col = h * a.hd + lane;
      const int nj = padded ? a.L : ic + 1;                   // exp(-2^32 - m) is exactly 0 behind the diagonal
      float acc = 0.f;
      for (int j = 0; j < nj; ++j) {
        const float p = sA[j];
        if (p == 0.f) continue;                               // wave-uniform: a dropped weight costs no gather
        acc = fmaf(p, sV[j * ldt + lane] + TS_FWD_TV(sT[j], pair0 + j, lane), acc);
      }
      out[(row0 + i) * ldo + col] = acc;
    }
    if (valid && lane == 0) lse[bh * a.L + i] = m + logf(sum);
  }
  if (bad && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
}

// grid (B H, ceil(L / 16)) over QUERY rows: gs, ga [B H, L, L] and dQ
__global__ __launch_bounds__(kBlock) void ts_attn_bwd_q_kernel(TsArgs a, const float* __restrict__ dout, int64_t lddo,
                                                               const float* __restrict__ lse, float* __restrict__ gs,
                                                               float* __restrict__ ga, float* __restrict__ dq, int64_t lddq) {
  extern __shared__ float smem[];
  const int ldt = a.hd | 1;
  float* sK = smem;
  float* sV = sK + a.L * ldt;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  float* sQ = sV + a.L * ldt + w * kTsMaxHead;
  float* sG = sV + a.L * ldt + kTsWaves * kTsMaxHead + w * kTsMaxHead;
  float* sA = sV + a.L * ldt + kTsWaves * 2 * kTsMaxHead + w * kTsMaxL;
  int* sT = reinterpret_cast<int*>(sV + a.L * ldt + kTsWaves * 2 * kTsMaxHead + kTsWaves * kTsMaxL) + w * kTsMaxL;
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int64_t row0 = (int64_t)b * a.L;
  ts_stage_kv(a, b, h, ldt, sK, sV);
  for (int r = 0; r < kTsRowsPerWave; ++r) {
    const int i = blockIdx.y * kTsRows + w * kTsRowsPerWave + r;
    const bool valid = i < a.L;
    const int ic = valid ? i : a.L - 1;
    __syncthreads();
    if (lane < a.hd) {
      sQ[lane] = a.q[(row0 + ic) * a.ldq + h * a.hd + lane];
      sG[lane] = dout[(row0 + ic) * lddo + h * a.hd + lane];
    }
    const uint64_t pair0 = (uint64_t)(row0 + ic) * a.L;
    for (int j = lane; j < a.L; j += kWave) {
      const int64_t t = a.tm[pair0 + j];
      sT[j] = t >= 0 && t < a.T ? (int)t : 0;
    }
    __syncthreads();
    const bool padded = a.log_seqs[row0 + ic] == 0;
    const float li = lse[bh * a.L + ic];
    float pw[kTsKeysPerLane], da[kTsKeysPerLane], keep_w[kTsKeysPerLane];
    float z = 0.f;
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      const int j = lane + kWave * u;
      pw[u] = da[u] = 0.f;
      keep_w[u] = 1.f;
      if (j < a.L) {
        const bool masked = padded || j > ic;
        float s = kTsNeg;
        if (!masked) {
          s = 0.f;
          const int t = sT[j];
          for (int d = 0; d < a.hd; ++d)
            s = fmaf(sQ[d], sK[j * ldt + d] + ts_time(a, a.time_k, a.key_tk, t, pair0 + j, h * a.hd + d), s);
          s *= a.scale;
        }
        pw[u] = expf(s - li);
        if (padded || j <= ic) {                              // behind the diagonal the weight is exactly 0
          const int t = sT[j];
          float g = 0.f;
          for (int d = 0; d < a.hd; ++d)
            g = fmaf(sG[d], sV[j * ldt + d] + ts_time(a, a.time_v, a.key_tv, t, pair0 + j, h * a.hd + d), g);
          da[u] = g;
        }
        z += pw[u];
      }
    }
    z = group_sum<kWave>(z);
    const float inv = 1.f / z;
    float dl = 0.f;
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      const int j = lane + kWave * u;
      pw[u] *= inv;
      if (a.drop_a) {                                         // da becomes d(weight): 0 where the weight was dropped
        const bool keep = j < a.L && ts_keep(a.key_a, a.th_a, ((uint64_t)bh * a.L + ic) * a.L + j);
        da[u] = keep ? da[u] * a.ik_a : 0.f;
        keep_w[u] = keep ? a.ik_a : 0.f;
      }
      dl = fmaf(pw[u], da[u], dl);
    }
    dl = group_sum<kWave>(dl);
#pragma unroll
    for (int u = 0; u < kTsKeysPerLane; ++u) {
      const int j = lane + kWave * u;
      if (j < a.L) {
        const float dae = da[u];
        const float ad = pw[u] * keep_w[u];
        const float ds = (padded || j > ic) ? 0.f : pw[u] * (dae - dl) * a.scale;   // a replaced score has no gradient
        sA[j] = ds;
        if (valid) {
          gs[((uint64_t)bh * a.L + i) * a.L + j] = ds;
          ga[((uint64_t)bh * a.L + i) * a.L + j] = ad;
        }
      }
    }
    __syncthreads();
    if (valid && lane < a.hd) {
      const int col = h * a.hd + lane;
      float acc = 0.f;
      if (!padded)
        for (int j = 0; j <= ic; ++j) {
          const float ds = sA[j];
          if (ds == 0.f) continue;
          acc = fmaf(ds, sK[j * ldt + lane] + ts_time(a, a.time_k, a.key_tk, sT[j], pair0 + j, col), acc);
        }
      dq[(row0 + i) * lddq + col] = acc;
    }
  }
}

// grid (B H, ceil(L / 16)) over KEY rows: dK_j = sum_i gs_ij q_i, dV_j = sum_i ga_ij dO_i, i ascending
__global__ __launch_bounds__(kBlock) void ts_attn_bwd_kv_kernel(TsArgs a, const float* __restrict__ dout, int64_t lddo,
                                                                const float* __restrict__ gs, const float* __restrict__ ga,
                                                                float* __restrict__ dk, int64_t lddk, float* __restrict__ dv,
                                                                int64_t lddv) {
  extern __shared__ float smem[];
  float* sQ = smem;                                           // [L][hd]
  float* sG = smem + a.L * a.hd;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int64_t row0 = (int64_t)b * a.L;
  for (int idx = threadIdx.x; idx < a.L * a.hd; idx += kBlock) {
    const int i = idx / a.hd, d = idx - i * a.hd;
    sQ[idx] = a.q[(row0 + i) * a.ldq + h * a.hd + d];
    sG[idx] = dout[(row0 + i) * lddo + h * a.hd + d];
  }
  __syncthreads();
  for (int r = 0; r < kTsRowsPerWave; ++r) {
    const int j = blockIdx.y * kTsRows + w * kTsRowsPerWave + r;
    if (j >= a.L || lane >= a.hd) continue;
    float ak = 0.f, av = 0.f;
    const float* gsj = gs + (uint64_t)bh * a.L * a.L + j;
    const float* gaj = ga + (uint64_t)bh * a.L * a.L + j;
    for (int i = 0; i < a.L; ++i) {
      ak = fmaf(gsj[(int64_t)i * a.L], sQ[i * a.hd + lane], ak);
      av = fmaf(gaj[(int64_t)i * a.L], sG[i * a.hd + lane], av);
    }
    dk[(row0 + j) * lddk + h * a.hd + lane] = ak;
    dv[(row0 + j) * lddv + h * a.hd + lane] = av;
  }
}

// d_pos_k[j, c] (+)= sum_b mask_bjc dk[b, j, c], the same for v: samples ascending
__global__ __launch_bounds__(kBlock) void ts_pos_grad_kernel(TsArgs a, int64_t B, const float* __restrict__ dk, int64_t lddk,
                                                             const float* __restrict__ dv, int64_t lddv,
                                                             float* __restrict__ d_pos_k, float* __restrict__ d_pos_v,
                                                             int accumulate) {
  const int total = a.L * a.D;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < total; e += gridDim.x * kBlock) {
    const int j = e / a.D, c = e - j * a.D;
    float sk = 0.f, sv = 0.f;
    for (int64_t b = 0; b < B; ++b) {
      const int64_t row = b * a.L + j;
      float gk = dk[row * lddk + c], gv = dv[row * lddv + c];
      if (a.drop_p) {
        const uint64_t m = (uint64_t)row * a.D + c;
        gk = ts_keep(a.key_pk, a.th_p, m) ? gk * a.ik_p : 0.f;
        gv = ts_keep(a.key_pv, a.th_p, m) ? gv * a.ik_p : 0.f;
      }
      sk += gk;
      sv += gv;
    }
    d_pos_k[e] = accumulate ? d_pos_k[e] + sk : sk;
    d_pos_v[e] = accumulate ? d_pos_v[e] + sv : sv;
  }
}

// grid (P, H, 2): z = 0 the key side (coefficients gs, vectors q), z = 1 the value side (ga, dO).  Dynamic LDS: [T][hd].
__global__ __launch_bounds__(kBlock) void ts_time_partial_kernel(TsArgs a, int64_t B, int per_block,
                                                                 const float* __restrict__ dout, int64_t lddo,
                                                                 const float* __restrict__ gs, const float* __restrict__ ga,
                                                                 float* __restrict__ partials) {
  extern __shared__ float tile[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int h = blockIdx.y, side = blockIdx.z;
  for (int idx = threadIdx.x; idx < a.T * a.hd; idx += kBlock) tile[idx] = 0.f;
  __syncthreads();
  const float* coef = side == 0 ? gs : ga;
  const float* vec = side == 0 ? a.q : dout;
  const int64_t ldvec = side == 0 ? a.ldq : lddo;
  const uint64_t key = side == 0 ? a.key_tk : a.key_tv;
  const int LL = a.L * a.L;
  const int64_t b0 = (int64_t)blockIdx.x * per_block;
  const int64_t b1 = b0 + per_block < B ? b0 + per_block : B;
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t* tmb = a.tm + b * LL;
    const float* cb = coef + (b * a.H + h) * LL;
    for (int f0 = 0; f0 < LL; f0 += kWave) {
      const int f = f0 + lane;
      int t = 0;
      float c = 0.f;
      if (f < LL) {
        const int64_t tt = tmb[f];
        t = tt >= 0 && tt < a.T ? (int)tt : 0;
        c = cb[f];
      }
      unsigned long long todo = __ballot(c != 0.f && (t & (kTsWaves - 1)) == w);
      while (todo) {                                          // ascending (b, i, j): a fixed order per table row
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int tl = __shfl(t, l, kWave);
        const float cl = __shfl(c, l, kWave);
        const int fl = f0 + l, i = fl / a.L;
        if (lane < a.hd) {
          const int col = h * a.hd + lane;
          float x = vec[(b * a.L + i) * ldvec + col];
          if (a.drop_t) x = ts_keep(key, a.th_t, ((uint64_t)b * LL + fl) * a.D + col) ? x * a.ik_t : 0.f;
          tile[tl * a.hd + lane] = fmaf(cl, x, tile[tl * a.hd + lane]);
        }
      }
    }
  }
  __syncthreads();
  float* dst = partials + ((int64_t)blockIdx.x * 2 + side) * a.T * a.D;
  for (int idx = threadIdx.x; idx < a.T * a.hd; idx += kBlock) {
    const int t = idx / a.hd, d = idx - t * a.hd;
    dst[(int64_t)t * a.D + h * a.hd + d] = tile[idx];
  }
}

__global__ __launch_bounds__(kBlock) void ts_time_fold_kernel(int64_t TD, int P, const float* __restrict__ partials,
                                                              float* __restrict__ d_time_k, float* __restrict__ d_time_v,
                                                              int accumulate) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < 2 * TD; e += (int64_t)gridDim.x * kBlock) {
    const int side = e >= TD;
    const int64_t o = e - side * TD;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += partials[((int64_t)p * 2 + side) * TD + o];
    float* dst = side ? d_time_v : d_time_k;
    dst[o] = accumulate ? dst[o] + s : s;
  }
}

// ---------------------------------------------------------------- affine layer norm, one wave per row
__global__ __launch_bounds__(kBlock) void aln_fwd_kernel(int64_t m, int n, const float* x, int64_t ldx, const float* r,
                                                         int64_t ldr, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         const int64_t* __restrict__ row_ids, float* sum_out, int64_t lds,
                                                         float* y, int64_t ldy, float* __restrict__ mean,
                                                         float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
  if (row >= m) return;
  const bool off = row_ids != nullptr && row_ids[row] == 0;
  const float* xr = x + row * ldx;
  const float* rr = r != nullptr ? r + row * ldr : nullptr;
  auto at = [&](int c) { return off ? 0.f : (rr != nullptr ? xr[c] + rr[c] : xr[c]); };
  float s = 0.f;
  for (int c = lane; c < n; c += kWave) s += at(c);
  const float mu = group_sum<kWave>(s) / (float)n;
  float v = 0.f;
  for (int c = lane; c < n; c += kWave) {
    const float t = at(c) - mu;
    v = fmaf(t, t, v);
  }
  const float rs = 1.f / sqrtf(group_sum<kWave>(v) / (float)n + eps);
  float* yr = y + row * ldy;
  float* sr = sum_out != nullptr ? sum_out + row * lds : nullptr;
  for (int c = lane; c < n; c += kWave) {
    const float t = at(c);                                    // read before either store: sum_out may be x
    yr[c] = (t - mu) * rs * gamma[c] + beta[c];
    if (sr != nullptr) sr[c] = t;
  }
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

__global__ __launch_bounds__(kBlock) void aln_bwd_kernel(int64_t m, int n, const float* __restrict__ t, int64_t ldt,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* dy, int64_t lddy,
                                                         const float* dy2, int64_t lddy2, const float* e1, int64_t lde1,
                                                         const float* e2, int64_t lde2, const int64_t* __restrict__ row_ids,
                                                         float* dx, int64_t lddx) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
  if (row >= m) return;
  float* dr = dx + row * lddx;
  if (row_ids != nullptr && row_ids[row] == 0) {
    for (int c = lane; c < n; c += kWave) dr[c] = 0.f;
    return;
  }
  const float mu = mean[row], rs = rstd[row];
  const float* tr = t + row * ldt;
  const float* g1 = dy + row * lddy;
  const float* g2 = dy2 != nullptr ? dy2 + row * lddy2 : nullptr;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < n; c += kWave) {
    const float g = (g2 != nullptr ? g1[c] + g2[c] : g1[c]) * gamma[c];
    s1 += g;
    s2 = fmaf(g, (tr[c] - mu) * rs, s2);
  }
  const float c1 = group_sum<kWave>(s1) / (float)n, c2 = group_sum<kWave>(s2) / (float)n;
  for (int c = lane; c < n; c += kWave) {
    const float g = (g2 != nullptr ? g1[c] + g2[c] : g1[c]) * gamma[c];
    float d = rs * (g - c1 - (tr[c] - mu) * rs * c2);
    if (e1 != nullptr) d += e1[row * lde1 + c];
    if (e2 != nullptr) d += e2[row * lde2 + c];
    dr[c] = d;
  }
}

// one block per column: dgamma[c] = sum_rows g xhat, dbeta[c] = sum_rows g (rows strided over the threads, then the tree)
__global__ __launch_bounds__(kBlock) void aln_param_kernel(int64_t m, const float* __restrict__ t, int64_t ldt,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ dy, int64_t lddy,
                                                           const float* __restrict__ dy2, int64_t lddy2,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float rg[kBlock];
  __shared__ float rb[kBlock];
  const int c = blockIdx.x;
  float sg = 0.f, sb = 0.f;
  for (int64_t row = threadIdx.x; row < m; row += kBlock) {
    const float g = dy2 != nullptr ? dy[row * lddy + c] + dy2[row * lddy2 + c] : dy[row * lddy + c];
    sg = fmaf(g, (t[row * ldt + c] - mean[row]) * rstd[row], sg);
    sb += g;
  }
  rg[threadIdx.x] = sg;
  rb[threadIdx.x] = sb;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      rg[threadIdx.x] += rg[threadIdx.x + o];
      rb[threadIdx.x] += rb[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dgamma[c] = rg[0];
    dbeta[c] = rb[0];
  }
}

// ---------------------------------------------------------------- embedding of the sequence
// bwd == 0: out[r] = drop(table[ids[r]] * scale), zero for id 0;  bwd != 0: src is d_out and no table is read
__global__ __launch_bounds__(kBlock) void ts_embed_kernel(int64_t n, int dim, int64_t num_rows,
                                                          const int64_t* __restrict__ ids, const float* __restrict__ src,
                                                          int64_t ld_src, float scale, int drop, uint32_t thresh, float ik,
                                                          uint64_t key, float* __restrict__ out, int64_t ldo, int bwd,
                                                          int32_t* __restrict__ status) {
  const int64_t total = n * dim;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / dim;
    const int c = (int)(e - r * dim);
    const int64_t id = ids[r];
    const bool ok = id >= 0 && id < num_rows;
    bad |= !ok;
    float x = 0.f;
    if (ok && id != 0) {
      x = (bwd ? src[r * ld_src + c] : src[id * ld_src + c]) * scale;
      if (drop) x = ts_keep(key, thresh, (uint64_t)e) ? x * ik : 0.f;
    }
    out[r * ldo + c] = x;
  }
  if (bad && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
}

// ---------------------------------------------------------------- head
__global__ __launch_bounds__(kBlock) void ts_head_count_kernel(int64_t n, const int64_t* __restrict__ pos,
                                                               float* __restrict__ loss2) {
  __shared__ int red[kBlock];
  int c = 0;
  for (int64_t r = threadIdx.x; r < n; r += kBlock) c += pos[r] != 0;
  red[threadIdx.x] = c;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss2[1] = (float)red[0];
}

__device__ __forceinline__ float softplusf(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoidf(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// one wave per position
__global__ __launch_bounds__(kBlock) void ts_head_rows_kernel(int64_t n, int dim, int64_t num_rows,
                                                              const float* __restrict__ feats, int64_t ldf,
                                                              const int64_t* __restrict__ pos, const int64_t* __restrict__ neg,
                                                              const float* __restrict__ table, int64_t ldt,
                                                              const float* __restrict__ loss2, float* __restrict__ row_loss,
                                                              float* __restrict__ pos_logits, float* __restrict__ neg_logits,
                                                              float* __restrict__ coef_pos, float* __restrict__ coef_neg,
                                                              float* __restrict__ d_feats, int64_t lddf,
                                                              float* __restrict__ d_pos_rows, int64_t ldp,
                                                              float* __restrict__ d_neg_rows, int64_t ldn,
                                                              int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t ip = pos[r], in = neg[r];
  const bool okp = ip >= 0 && ip < num_rows, okn = in >= 0 && in < num_rows;
  if ((!okp || !okn) && lane == 0 && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
  const float* fr = feats + r * ldf;
  const float* ep = table + (okp ? ip : 0) * ldt;
  const float* en = table + (okn ? in : 0) * ldt;
  float pl = 0.f, nl = 0.f;
  for (int c = lane; c < dim; c += kWave) {
    pl = fmaf(fr[c], okp ? ep[c] : 0.f, pl);
    nl = fmaf(fr[c], okn ? en[c] : 0.f, nl);
  }
  pl = group_sum<kWave>(pl);
  nl = group_sum<kWave>(nl);
  const bool sel = ip != 0;
  const float cnt = loss2[1];
  const float cp = sel ? (sigmoidf(pl) - 1.f) / cnt : 0.f;
  const float cn = sel ? sigmoidf(nl) / cnt : 0.f;
  if (lane == 0) {
    row_loss[r] = sel ? softplusf(-pl) + softplusf(nl) : 0.f;
    coef_pos[r] = cp;
    coef_neg[r] = cn;
    if (pos_logits != nullptr) pos_logits[r] = pl;
    if (neg_logits != nullptr) neg_logits[r] = nl;
  }
  for (int c = lane; c < dim; c += kWave) {
    const float f = fr[c];
    d_feats[r * lddf + c] = fmaf(cp, okp ? ep[c] : 0.f, cn * (okn ? en[c] : 0.f));
    if (d_pos_rows != nullptr) d_pos_rows[r * ldp + c] = cp * f;
    if (d_neg_rows != nullptr) d_neg_rows[r * ldn + c] = cn * f;
  }
}

__global__ __launch_bounds__(kBlock) void ts_head_loss_kernel(int64_t n, const float* __restrict__ row_loss,
                                                              float* __restrict__ loss2) {
  __shared__ float red[kBlock];
  float s = 0.f;
  for (int64_t r = threadIdx.x; r < n; r += kBlock) s += row_loss[r];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss2[0] = red[0] / loss2[1];        // an empty selection: 0 / 0 = NaN, as the reference's mean
}

int64_t ts_grid(int64_t total) {
  int64_t grid = (total + kBlock - 1) / kBlock;
  if (grid > kNumCU * 8) grid = kNumCU * 8;
  return grid < 1 ? 1 : grid;
}

uint64_t ts_key(uint64_t seed, uint64_t stream_id) { return mix64(seed ^ mix64(stream_id + 0x9E3779B97F4A7C15ull)); }
uint32_t ts_thresh(float p) { return (uint32_t)((double)p * 4294967296.0); }

int ts_check(const char* what, int64_t batch, int32_t L, int32_t H, int32_t D, int32_t T, const float* q, int64_t ldq,
             const float* k, int64_t ldk, const float* v, int64_t ldv, const float* const* tables, const int64_t* tm,
             const int64_t* log_seqs, float scale, const float* probs, uint64_t seed, const uint64_t* streams, TsArgs* a) {
  REC_REQUIRE(batch >= 0 && L >= 1 && H >= 1 && D >= 1 && T >= 1, REC_EINVAL,
              "%s: bad sizes (batch %lld, seq_len %d, heads %d, hidden %d, time_rows %d)", what, (long long)batch, L, H, D, T);
  REC_REQUIRE(D % H == 0, REC_EINVAL, "%s: hidden %d is not a multiple of n_head %d", what, D, H);
  const int hd = D / H;
  REC_REQUIRE(L <= REC_TISAS_MAX_L && hd <= REC_TISAS_MAX_HEAD && L * (hd | 1) <= REC_TISAS_MAX_TILE, REC_EINVAL,
              "%s: seq_len %d / head %d beyond the limits (seq_len <= %d, head <= %d, seq_len * (head | 1) <= %d)", what, L,
              hd, REC_TISAS_MAX_L, REC_TISAS_MAX_HEAD, REC_TISAS_MAX_TILE);
  REC_REQUIRE(batch * H < (1ll << 31) && batch * L * L < (1ll << 40), REC_EINVAL, "%s: batch too large", what);
  REC_REQUIRE(probs && streams && tables, REC_EINVAL, "%s: null pointer argument (tables, probs or streams)", what);
  for (int i = 0; i < 3; ++i)
    REC_REQUIRE(probs[i] >= 0.f && probs[i] < 1.f, REC_EINVAL, "%s: probs[%d] must be in [0, 1)", what, i);
  REC_REQUIRE(isfinite(scale), REC_EINVAL, "%s: scale must be finite", what);
  for (int i = 0; i < 4; ++i) REC_REQUIRE(tables[i], REC_EINVAL, "%s: tables[%d] is null", what, i);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(q && k && v && tm && log_seqs, REC_EINVAL, "%s: null pointer argument", what);
  REC_REQUIRE(ldq >= D && ldk >= D && ldv >= D, REC_EINVAL, "%s: a row stride of q, k, v is smaller than hidden", what);
  a->L = L;
  a->H = H;
  a->hd = hd;
  a->D = D;
  a->T = T;
  a->q = q;
  a->k = k;
  a->v = v;
  a->ldq = ldq;
  a->ldk = ldk;
  a->ldv = ldv;
  a->pos_k = tables[0];
  a->pos_v = tables[1];
  a->time_k = tables[2];
  a->time_v = tables[3];
  a->tm = tm;
  a->log_seqs = log_seqs;
  a->scale = scale;
  a->drop_a = probs[0] > 0.f;
  a->drop_p = probs[1] > 0.f;
  a->drop_t = probs[2] > 0.f;
  a->th_a = ts_thresh(probs[0]);
  a->th_p = ts_thresh(probs[1]);
  a->th_t = ts_thresh(probs[2]);
  a->ik_a = 1.f / (1.f - probs[0]);
  a->ik_p = 1.f / (1.f - probs[1]);
  a->ik_t = 1.f / (1.f - probs[2]);
  a->key_a = ts_key(seed, streams[0]);
  a->key_pk = ts_key(seed, streams[1]);
  a->key_pv = ts_key(seed, streams[2]);
  a->key_tk = ts_key(seed, streams[3]);
  a->key_tv = ts_key(seed, streams[4]);
  return REC_OK;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_tisas_attn_fwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t hidden, int32_t time_rows,
                                  const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                  const float* const* tables, const int64_t* tm, const int64_t* log_seqs, float scale,
                                  const float* probs, uint64_t seed, const uint64_t* streams, float* out, int64_t ldo,
                                  float* lse, int32_t* status, void* stream) {
  TsArgs a;
  int rc = ts_check("rec_tisas_attn_fwd", batch, seq_len, n_head, hidden, time_rows, q, ldq, k, ldk, v, ldv, tables, tm,
                    log_seqs, scale, probs, seed, streams, &a);
  if (rc != REC_OK || batch == 0) return rc;
  REC_REQUIRE(out && lse && ldo >= hidden, REC_EINVAL, "rec_tisas_attn_fwd: out / lse null, or ldo smaller than hidden");
  REC_REQUIRE(out != q && out != k && out != v, REC_EINVAL, "rec_tisas_attn_fwd: out aliases no input");
  const dim3 grid((unsigned)(batch * n_head), (unsigned)((seq_len + kTsRows - 1) / kTsRows));
  size_t lds = ts_lds_bytes(seq_len, a.hd);
#ifdef REC_TISAS_TIME_LDS
  lds += (size_t)2 * time_rows * a.hd * sizeof(float);
  REC_REQUIRE(lds <= 160 * 1024, REC_EINVAL, "rec_tisas_attn_fwd (REC_TISAS_TIME_LDS): %zu bytes of LDS", lds);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ts_attn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return check_launch("rec_tisas_attn_fwd (LDS attribute)");
#endif
  hipLaunchKernelGGL(ts_attn_fwd_kernel, grid, dim3(kBlock), lds, (hipStream_t)stream, a, out, ldo, lse, status);
  return check_launch("rec_tisas_attn_fwd");
}

extern "C" int rec_tisas_attn_bwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t hidden, int32_t time_rows,
                                  const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                  const float* const* tables, const int64_t* tm, const int64_t* log_seqs, float scale,
                                  const float* probs, uint64_t seed, const uint64_t* streams, const float* d_out,
                                  int64_t ld_dout, const float* lse, float* gs, float* ga, float* dq, int64_t lddq, float* dk,
                                  int64_t lddk, float* dv, int64_t lddv, float* const* d_tables, float* partials,
                                  int32_t accumulate, void* stream) {
  TsArgs a;
  int rc = ts_check("rec_tisas_attn_bwd", batch, seq_len, n_head, hidden, time_rows, q, ldq, k, ldk, v, ldv, tables, tm,
                    log_seqs, scale, probs, seed, streams, &a);
  if (rc != REC_OK) return rc;
  REC_REQUIRE((int64_t)time_rows * (hidden / n_head) <= REC_TISAS_MAX_TIME_TILE, REC_EINVAL,
              "rec_tisas_attn_bwd: time_rows %d * head %d > %d", time_rows, hidden / n_head, REC_TISAS_MAX_TIME_TILE);
  REC_REQUIRE(d_tables, REC_EINVAL, "rec_tisas_attn_bwd: d_tables is null");
  for (int i = 0; i < 4; ++i)
    REC_REQUIRE(d_tables[i] && d_tables[i] != tables[i], REC_EINVAL, "rec_tisas_attn_bwd: d_tables[%d] is null or its table", i);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(d_out && lse && gs && ga && dq && dk && dv && partials, REC_EINVAL, "rec_tisas_attn_bwd: null pointer argument");
  REC_REQUIRE(ld_dout >= hidden && lddq >= hidden && lddk >= hidden && lddv >= hidden, REC_EINVAL,
              "rec_tisas_attn_bwd: a row stride is smaller than hidden");
  for (const float* g : {(const float*)dq, (const float*)dk, (const float*)dv, (const float*)gs, (const float*)ga})
    REC_REQUIRE(g != q && g != k && g != v && g != d_out && g != lse, REC_EINVAL, "rec_tisas_attn_bwd: an output aliases an input");
  REC_REQUIRE(dq != dk && dq != dv && dk != dv && gs != ga, REC_EINVAL, "rec_tisas_attn_bwd: the outputs alias each other");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(batch * n_head), (unsigned)((seq_len + kTsRows - 1) / kTsRows));
  hipLaunchKernelGGL(ts_attn_bwd_q_kernel, grid, dim3(kBlock), ts_lds_bytes(seq_len, a.hd), st, a, d_out, ld_dout, lse, gs, ga,
                     dq, lddq);
  if ((rc = check_launch("rec_tisas_attn_bwd (dQ)")) != REC_OK) return rc;
  hipLaunchKernelGGL(ts_attn_bwd_kv_kernel, grid, dim3(kBlock), (size_t)2 * seq_len * a.hd * sizeof(float), st, a, d_out,
                     ld_dout, (const float*)gs, (const float*)ga, dk, lddk, dv, lddv);
  if ((rc = check_launch("rec_tisas_attn_bwd (dK, dV)")) != REC_OK) return rc;
  hipLaunchKernelGGL(ts_pos_grad_kernel, dim3((unsigned)ts_grid((int64_t)seq_len * hidden)), dim3(kBlock), 0, st, a, batch,
                     (const float*)dk, lddk, (const float*)dv, lddv, d_tables[0], d_tables[1], (int)accumulate);
  if ((rc = check_launch("rec_tisas_attn_bwd (positions)")) != REC_OK) return rc;
  const int P = (int)(batch < REC_TISAS_MAX_PARTIALS ? batch : REC_TISAS_MAX_PARTIALS);
  const int per_block = (int)((batch + P - 1) / P);
  const int used = (int)((batch + per_block - 1) / per_block);          // blocks that own at least one sample
  hipLaunchKernelGGL(ts_time_partial_kernel, dim3((unsigned)used, (unsigned)n_head, 2u), dim3(kBlock),
                     (size_t)time_rows * a.hd * sizeof(float), st, a, batch, per_block, d_out, ld_dout, (const float*)gs,
                     (const float*)ga, partials);
  if ((rc = check_launch("rec_tisas_attn_bwd (time tiles)")) != REC_OK) return rc;
  const int64_t TD = (int64_t)time_rows * hidden;
  hipLaunchKernelGGL(ts_time_fold_kernel, dim3((unsigned)ts_grid(2 * TD)), dim3(kBlock), 0, st, TD, used,
                     (const float*)partials, d_tables[2], d_tables[3], (int)accumulate);
  return check_launch("rec_tisas_attn_bwd (time fold)");
}

extern "C" int rec_affine_layer_norm_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, const float* r, int64_t ldr,
                                         const float* gamma, const float* beta, float eps, const int64_t* row_ids,
                                         float* sum_out, int64_t ld_sum, float* y, int64_t ldy, float* mean, float* rstd,
                                         void* stream) {
  REC_REQUIRE(m >= 0 && n > 0 && eps >= 0.f, REC_EINVAL, "rec_affine_layer_norm_fwd: bad sizes (m %lld, n %d)", (long long)m, n);
  REC_REQUIRE(gamma && beta, REC_EINVAL, "rec_affine_layer_norm_fwd: gamma / beta null");
  if (m == 0) return REC_OK;
  REC_REQUIRE(x && y && mean && rstd, REC_EINVAL, "rec_affine_layer_norm_fwd: null pointer argument");
  REC_REQUIRE(ldx >= n && ldy >= n && (r == nullptr || ldr >= n) && (sum_out == nullptr || ld_sum >= n), REC_EINVAL,
              "rec_affine_layer_norm_fwd: a row stride is smaller than n");
  REC_REQUIRE(y != x && y != r && y != sum_out && (sum_out == nullptr || sum_out != r), REC_EINVAL,
              "rec_affine_layer_norm_fwd: y aliases no operand and sum_out may only be x");
  const int64_t grid = (m + kLnRows - 1) / kLnRows;
  REC_REQUIRE(grid < (1ll << 31), REC_EINVAL, "rec_affine_layer_norm_fwd: too many rows");
  hipLaunchKernelGGL(aln_fwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, m, n, x, ldx, r, ldr, gamma,
                     beta, eps, row_ids, sum_out, ld_sum, y, ldy, mean, rstd);
  return check_launch("rec_affine_layer_norm_fwd");
}

extern "C" int rec_affine_layer_norm_bwd(int64_t m, int32_t n, const float* t, int64_t ldt, const float* mean,
                                         const float* rstd, const float* gamma, const float* dy, int64_t lddy,
                                         const float* dy2, int64_t lddy2, const float* e1, int64_t lde1, const float* e2,
                                         int64_t lde2, const int64_t* row_ids, float* dx, int64_t lddx, float* dgamma,
                                         float* dbeta, void* stream) {
  REC_REQUIRE(m >= 0 && n > 0, REC_EINVAL, "rec_affine_layer_norm_bwd: bad sizes (m %lld, n %d)", (long long)m, n);
  REC_REQUIRE(gamma && dgamma && dbeta && dgamma != dbeta, REC_EINVAL, "rec_affine_layer_norm_bwd: gamma / dgamma / dbeta null");
  REC_REQUIRE(m == 0 || (t && mean && rstd && dy && dx), REC_EINVAL, "rec_affine_layer_norm_bwd: null pointer argument");
  REC_REQUIRE(m == 0 || (ldt >= n && lddy >= n && lddx >= n && (dy2 == nullptr || lddy2 >= n) && (e1 == nullptr || lde1 >= n) &&
                         (e2 == nullptr || lde2 >= n)),
              REC_EINVAL, "rec_affine_layer_norm_bwd: a row stride is smaller than n");
  REC_REQUIRE(m == 0 || (dx != t && dx != dy2 && dx != e1 && dx != e2), REC_EINVAL,
              "rec_affine_layer_norm_bwd: dx may alias dy only");
  const int64_t grid = (m + kLnRows - 1) / kLnRows;
  REC_REQUIRE(grid < (1ll << 31), REC_EINVAL, "rec_affine_layer_norm_bwd: too many rows");
  hipStream_t st = (hipStream_t)stream;
  // the parameter sums first: they read dy, which dx may overwrite
  hipLaunchKernelGGL(aln_param_kernel, dim3((unsigned)n), dim3(kBlock), 0, st, m, t, ldt, mean, rstd, dy, lddy, dy2, lddy2,
                     dgamma, dbeta);
  int rc = check_launch("rec_affine_layer_norm_bwd (gamma, beta)");
  if (rc != REC_OK || m == 0) return rc;
  hipLaunchKernelGGL(aln_bwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, m, n, t, ldt, mean, rstd, gamma, dy, lddy, dy2,
                     lddy2, e1, lde1, e2, lde2, row_ids, dx, lddx);
  return check_launch("rec_affine_layer_norm_bwd");
}

static int ts_embed(const char* what, int64_t n, int32_t dim, int64_t num_rows, const int64_t* ids, const float* src,
                    int64_t ld_src, float scale, float p, uint64_t seed, uint64_t stream_id, float* out, int64_t ldo, int bwd,
                    int32_t* status, void* stream) {
  REC_REQUIRE(n >= 0 && dim > 0 && num_rows > 0, REC_EINVAL, "%s: bad sizes (n %lld, dim %d, num_rows %lld)", what, (long long)n,
              dim, (long long)num_rows);
  REC_REQUIRE(p >= 0.f && p < 1.f && isfinite(scale), REC_EINVAL, "%s: p must be in [0, 1) and scale finite", what);
  if (n == 0) return REC_OK;
  REC_REQUIRE(ids && src && out && out != src, REC_EINVAL, "%s: null pointer argument, or the output is the input", what);
  REC_REQUIRE(ld_src >= dim && ldo >= dim, REC_EINVAL, "%s: a row stride is smaller than dim", what);
  hipLaunchKernelGGL(ts_embed_kernel, dim3((unsigned)ts_grid(n * dim)), dim3(kBlock), 0, (hipStream_t)stream, n, dim, num_rows,
                     ids, src, ld_src, scale, (int)(p > 0.f), ts_thresh(p), 1.f / (1.f - p), ts_key(seed, stream_id), out, ldo,
                     bwd, status);
  return check_launch(what);
}

extern "C" int rec_tisas_embed_fwd(int64_t n, int32_t dim, int64_t num_rows, const int64_t* ids, const float* table,
                                   int64_t ld_table, float scale, float p, uint64_t seed, uint64_t stream_id, float* out,
                                   int64_t ldo, int32_t* status, void* stream) {
  return ts_embed("rec_tisas_embed_fwd", n, dim, num_rows, ids, table, ld_table, scale, p, seed, stream_id, out, ldo, 0, status,
                  stream);
}

extern "C" int rec_tisas_embed_bwd(int64_t n, int32_t dim, int64_t num_rows, const int64_t* ids, const float* d_out,
                                   int64_t ld_dout, float scale, float p, uint64_t seed, uint64_t stream_id, float* rows,
                                   int64_t ld_rows, void* stream) {
  return ts_embed("rec_tisas_embed_bwd", n, dim, num_rows, ids, d_out, ld_dout, scale, p, seed, stream_id, rows, ld_rows, 1,
                  nullptr, stream);
}

extern "C" int rec_tisas_head(int64_t n, int32_t dim, int64_t num_rows, const float* feats, int64_t ld_feats, const int64_t* pos,
                              const int64_t* neg, const float* table, int64_t ld_table, float* loss2, float* row_loss,
                              float* pos_logits, float* neg_logits, float* coef_pos, float* coef_neg, float* d_feats, int64_t ld_dfeats, float* d_pos_rows,
                              int64_t ld_dpos, float* d_neg_rows, int64_t ld_dneg, int32_t* status, void* stream) {
  REC_REQUIRE(n >= 0 && dim > 0 && dim <= REC_TISAS_HEAD_MAX_DIM && num_rows > 0, REC_EINVAL,
              "rec_tisas_head: bad sizes (n %lld, dim %d, num_rows %lld)", (long long)n, dim, (long long)num_rows);
  REC_REQUIRE(loss2, REC_EINVAL, "rec_tisas_head: loss2 is null");
  REC_REQUIRE(n == 0 || (feats && pos && neg && table && row_loss && coef_pos && coef_neg && d_feats), REC_EINVAL,
              "rec_tisas_head: null pointer argument");
  REC_REQUIRE(n == 0 || (ld_feats >= dim && ld_table >= dim && ld_dfeats >= dim && (d_pos_rows == nullptr || ld_dpos >= dim) &&
                         (d_neg_rows == nullptr || ld_dneg >= dim)),
              REC_EINVAL, "rec_tisas_head: a row stride is smaller than dim");
  REC_REQUIRE(n == 0 || (d_feats != feats && d_pos_rows != feats && d_neg_rows != feats), REC_EINVAL,
              "rec_tisas_head: an output is feats");
  const int64_t grid = (n + kLnRows - 1) / kLnRows;
  REC_REQUIRE(grid < (1ll << 31), REC_EINVAL, "rec_tisas_head: too many rows");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ts_head_count_kernel, dim3(1), dim3(kBlock), 0, st, n, pos, loss2);
  int rc = check_launch("rec_tisas_head (count)");
  if (rc != REC_OK) return rc;
  if (n > 0) {
    hipLaunchKernelGGL(ts_head_rows_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, n, dim, num_rows, feats, ld_feats, pos,
                       neg, table, ld_table, (const float*)loss2, row_loss, pos_logits, neg_logits, coef_pos, coef_neg, d_feats, ld_dfeats, d_pos_rows,
                       ld_dpos, d_neg_rows, ld_dneg, status);
    if ((rc = check_launch("rec_tisas_head (rows)")) != REC_OK) return rc;
  }
  hipLaunchKernelGGL(ts_head_loss_kernel, dim3(1), dim3(kBlock), 0, st, n, (const float*)row_loss, loss2);
  return check_launch("rec_tisas_head (loss)");
}
