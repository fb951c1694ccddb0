// DMR (rank/dmr, Deep Match to Rank) on gfx950: the causal masked-softmax pooling of its user-to-item net, PReLU, the
// full-softmax cross-entropy of its auxiliary match loss, and the glue of its tower input.
//
//   rec_dmr_prefix_pool_fwd / _bwd  <- dmr/net.py:259-281 (u2i: mask, the [B,T,T] lower-triangular tile, softmax over
//                                      each full row, matmul with the history) for a short LIST of rows, and
//                                      net.py:338-350 (i2i: the same with the one row T-1, plus the sum of the raw
//                                      scores at valid positions).  O(R T D) per sample, no T x T buffer.
//   rec_prelu_fwd / _bwd            <- paddle.nn.PReLU: channel = column (the tower, [B, n]) or channel = base +
//                                      row % period (axis 1 of a [B, T, n] input given as [B*T, n])
//   rec_dmr_match_loss_fwd / _bwd   <- net.py:298-301: logits = U V^T + bias over ALL classes, mean softmax
//                                      cross-entropy.  No [B, C] buffer: the classes are cut into at most 64 chunks, a
//                                      chunk's (max, sum exp) / dU partial is folded in chunk order; the backward
//                                      recomputes the logits.  dV is dense (every class row).
//   rec_dmr_tail_fwd / _bwd_match / _bwd_hist <- net.py:471,289-291,512-516,526: sum_t hist, item_eb * that sum, the
//                                      rel_u2i dot product and user_vector2 = row T-2 * match_mask, written straight
//                                      into column ranges of the tower input; their backward.
//
// Match-loss kernels.  Products are plain f32 FMAs.  Forward and dU: a THREAD owns a batch row (U_b in registers, K / 4
// float4) and walks the classes of its chunk; the class row V_c is the same for every lane (a uniform address: scalar
// loads, no LDS).  dV: a thread owns a CLASS (V_c and its K accumulators in registers) and walks the rows of one of at
// most 16 batch chunks, U_b uniform.  A logit is four k-strided FMA chains added as (x + y) + (z + w) — the same
// in all three kernels, so exp(logit - lse) in the backward is the forward's value.  K is a multiple of 4, at most 64;
// the register arrays are sized by the template argument (K / 4 rounded up to 1, 2, 4, 8, 12 or 16) and indexed by
// fully unrolled loops only.
// Every sum has a fixed order and there are no float atomics: a rerun is bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr float kDmrPad = -4294967295.0f;          // float32(-2**32 + 1) = -4294967296 (net.py:262,274,340)
constexpr int kPoolMaxRows = 8;                    // query positions per call
constexpr int kPoolMaxSteps = 4096;                // backward: 2 * T floats of LDS
constexpr int kPreluRows = 16;                     // rows of a backward block
constexpr int kMatchChunks = 64;                   // class chunks (forward, dU)
constexpr int kMatchBatchChunks = 16;              // batch chunks (dV)
constexpr int kMatchMaxK = 64;

__device__ __forceinline__ float dmr_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ float dmr_block_max(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

struct PoolRows {
  int n;
  int r[kPoolMaxRows];
};

// ---------------------------------------------------------------- prefix pool, one block per sample
// v_{r,j} = (j <= r && mask_j == 1) ? score_j : P for ALL j < T; w_r = softmax(v_r); out[b,r,:] = sum_j w_{r,j} hist[b,j,:]
// (ascending j).  A prefix without a valid position has max = P: exp(0) = 1 everywhere, w = 1 / T over all T entries.
__global__ __launch_bounds__(kBlock) void dmr_prefix_pool_fwd_kernel(int T, int D, const float* __restrict__ score,
                                                                     const int64_t* __restrict__ mask, int64_t ldm,
                                                                     const float* __restrict__ hist, int64_t ldh,
                                                                     PoolRows rows, float* __restrict__ out, int64_t ldo,
                                                                     float* __restrict__ rel, int64_t ld_rel,
                                                                     float* __restrict__ w) {
  __shared__ float red[kBlock];
  const int64_t b = blockIdx.x;
  const float* s = score + b * T;
  const int64_t* mk = mask + b * ldm;
  const float* h = hist + b * T * ldh;
  float* wb = w + b * rows.n * T;
  for (int q = 0; q < rows.n; ++q) {
    const int r = rows.r[q];
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < T; j += kBlock) mx = fmaxf(mx, (j <= r && mk[j] == 1) ? s[j] : kDmrPad);
    mx = dmr_block_max(mx, red);
    float sum = 0.f;
    for (int j = threadIdx.x; j < T; j += kBlock) sum += expf(((j <= r && mk[j] == 1) ? s[j] : kDmrPad) - mx);
    sum = dmr_block_sum(sum, red);
    for (int j = threadIdx.x; j < T; j += kBlock)
      wb[q * T + j] = expf(((j <= r && mk[j] == 1) ? s[j] : kDmrPad) - mx) / sum;
  }
  if (rel != nullptr) {
    float sr = 0.f;
    for (int j = threadIdx.x; j < T; j += kBlock) sr += mk[j] == 1 ? s[j] : 0.f;
    sr = dmr_block_sum(sr, red);
    if (threadIdx.x == 0) rel[b * ld_rel] = sr;
  }
  __syncthreads();                                         // w of this sample: written by this block, read below
  for (int i = threadIdx.x; i < rows.n * D; i += kBlock) {
    const int q = i / D, d = i % D;
    float acc = 0.f;
    for (int j = 0; j < T; ++j) acc = fmaf(wb[q * T + j], h[j * ldh + d], acc);
    out[b * ldo + i] = acc;
  }
}

// g_{r,j} = d_out[b,r] . hist[b,j];  dv_{r,j} = w_{r,j} (g_{r,j} - sum_s w_{r,s} g_{r,s});
// dscore[b,j] = sum_r [j <= r && mask_j == 1] dv_{r,j} + [mask_j == 1] d_rel[b];  d_hist[b,j,:] (+)= sum_r w_{r,j} d_out[b,r,:]
__global__ __launch_bounds__(kBlock) void dmr_prefix_pool_bwd_kernel(int T, int D, const int64_t* __restrict__ mask,
                                                                     int64_t ldm, const float* __restrict__ hist,
                                                                     int64_t ldh, PoolRows rows,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ d_out, int64_t lddo,
                                                                     const float* __restrict__ d_rel, int64_t ld_drel,
                                                                     float* __restrict__ dscore,
                                                                     float* __restrict__ d_hist, int64_t lddh,
                                                                     int accumulate) {
  __shared__ float red[kBlock];
  extern __shared__ float pool_lds[];                      // g [T] | acc [T]
  float* g = pool_lds;
  float* acc = pool_lds + T;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t* mk = mask + b * ldm;
  const float* h = hist + b * T * ldh;
  const float* wb = w + b * rows.n * T;
  const float* dob = d_out + b * lddo;
  for (int j = threadIdx.x; j < T; j += kBlock) acc[j] = 0.f;
  for (int q = 0; q < rows.n; ++q) {
    const int r = rows.r[q];
    for (int j = wave; j < T; j += kBlock / kWave) {
      float s = 0.f;
      for (int d = lane; d < D; d += kWave) s = fmaf(dob[q * D + d], h[j * ldh + d], s);
      s = group_sum<kWave>(s);
      if (lane == 0) g[j] = s;
    }
    __syncthreads();
    float sum = 0.f;
    for (int j = threadIdx.x; j < T; j += kBlock) sum = fmaf(wb[q * T + j], g[j], sum);
    sum = dmr_block_sum(sum, red);
    for (int j = threadIdx.x; j < T; j += kBlock)          // entry j has one owner thread: no race, fixed order over q
      if (j <= r && mk[j] == 1) acc[j] += wb[q * T + j] * (g[j] - sum);
    __syncthreads();
  }
  const float dr = d_rel != nullptr ? d_rel[b * ld_drel] : 0.f;
  for (int j = threadIdx.x; j < T; j += kBlock) dscore[b * T + j] = acc[j] + (mk[j] == 1 ? dr : 0.f);
  float* dh = d_hist + b * T * lddh;
  for (int i = threadIdx.x; i < T * D; i += kBlock) {
    const int j = i / D, d = i % D;
    float a = 0.f;
    for (int q = 0; q < rows.n; ++q) a = fmaf(wb[q * T + j], dob[q * D + d], a);
    dh[j * lddh + d] = accumulate ? dh[j * lddh + d] + a : a;
  }
}

// ---------------------------------------------------------------- PReLU
// Both channel rules are one "virtual matrix" [mv, nv] whose channel is cbase + column / cgroup: column mode mv = m,
// nv = n, cgroup 1; row mode (channel = base + row % period) mv = ceil(m / period), nv = period * n, cgroup n — virtual
// element (rv, cv) is X[rv * period + cv / n, cv % n].
struct PreluShape {
  int64_t m;
  int n, period, cgroup, cbase;
  int64_t mv, nv;
};

__device__ __forceinline__ bool prelu_at(const PreluShape& s, int64_t rv, int64_t cv, int64_t& row, int& col) {
  if (s.period > 1 || s.cgroup > 1) {
    row = rv * s.period + cv / s.n;
    col = (int)(cv % s.n);
  } else {
    row = rv;
    col = (int)cv;
  }
  return row < s.m;
}

__global__ __launch_bounds__(kBlock) void prelu_fwd_kernel(PreluShape s, const float* __restrict__ X, int64_t ldx,
                                                           const float* __restrict__ alpha, float* __restrict__ Y,
                                                           int64_t ldy) {
  const int64_t cv = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (cv >= s.nv) return;
  const float a = alpha[s.cbase + cv / s.cgroup];
  const int64_t r0 = (int64_t)blockIdx.y * kPreluRows;
  for (int64_t rv = r0; rv < r0 + kPreluRows && rv < s.mv; ++rv) {
    int64_t row;
    int col;
    if (!prelu_at(s, rv, cv, row, col)) continue;
    const float x = X[row * ldx + col];
    Y[row * ldy + col] = x > 0.f ? x : a * x;
  }
}

// dX = x > 0 ? dy : a dy;  part[blockIdx.y, cv] = sum over the block's rows (ascending) of dy x where x <= 0
__global__ __launch_bounds__(kBlock) void prelu_bwd_kernel(PreluShape s, const float* __restrict__ X, int64_t ldx,
                                                           const float* __restrict__ dY, int64_t lddy,
                                                           const float* __restrict__ alpha, float* __restrict__ dX,
                                                           int64_t lddx, float* __restrict__ part) {
  const int64_t cv = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (cv >= s.nv) return;
  const float a = alpha[s.cbase + cv / s.cgroup];
  const int64_t r0 = (int64_t)blockIdx.y * kPreluRows;
  float sum = 0.f;
  for (int64_t rv = r0; rv < r0 + kPreluRows && rv < s.mv; ++rv) {
    int64_t row;
    int col;
    if (!prelu_at(s, rv, cv, row, col)) continue;
    const float x = X[row * ldx + col], dy = dY[row * lddy + col];
    dX[row * lddx + col] = x > 0.f ? dy : a * dy;
    sum += x > 0.f ? 0.f : dy * x;
  }
  part[(int64_t)blockIdx.y * s.nv + cv] = sum;
}

// one block per channel of dalpha [num_alpha]: the channel's nblk * cgroup partials, thread-strided then the fixed tree;
// a channel outside [cbase, cbase + nv / cgroup) gets 0
__global__ __launch_bounds__(kBlock) void prelu_fold_kernel(PreluShape s, int64_t nblk, const float* __restrict__ part,
                                                            float* __restrict__ dalpha) {
  __shared__ float red[kBlock];
  const int ch = (int)blockIdx.x - s.cbase;
  float sum = 0.f;
  if (ch >= 0 && (int64_t)ch * s.cgroup < s.nv) {
    const int64_t items = nblk * s.cgroup;
    for (int64_t i = threadIdx.x; i < items; i += kBlock)
      sum += part[(i / s.cgroup) * s.nv + (int64_t)ch * s.cgroup + i % s.cgroup];
  }
  sum = dmr_block_sum(sum, red);
  if (threadIdx.x == 0) dalpha[blockIdx.x] = sum;
}

// ---------------------------------------------------------------- match loss
struct MatchArgs {
  int64_t B, C;
  int k4;                       // K / 4
  const float* U;
  int64_t ldu;
  const float* V;
  int64_t ldv;
  const float* bias;
  const int64_t* label;
  int64_t ldl;
  int64_t chunk;                // classes per chunk (forward, dU) / rows per chunk (dV)
  int nch;
};

__device__ __forceinline__ float4 ld4u(const float* p) { return *reinterpret_cast<const float4*>(p); }

// logit = U_b . V_c: four k-strided chains, (x + y) + (z + w)
template <int K4>
__device__ __forceinline__ float match_logit(const float4 (&a)[K4], const float* __restrict__ v, int k4) {
  float zx = 0.f, zy = 0.f, zz = 0.f, zw = 0.f;
#pragma unroll
  for (int i = 0; i < K4; ++i)
    if (i < k4) {
      zx = fmaf(a[i].x, v[4 * i], zx);
      zy = fmaf(a[i].y, v[4 * i + 1], zy);
      zz = fmaf(a[i].z, v[4 * i + 2], zz);
      zw = fmaf(a[i].w, v[4 * i + 3], zw);
    }
  return (zx + zy) + (zz + zw);
}

template <int K4>
__device__ __forceinline__ float match_logit_reg(const float4 (&a)[K4], const float4 (&v)[K4]) {
  float zx = 0.f, zy = 0.f, zz = 0.f, zw = 0.f;
#pragma unroll
  for (int i = 0; i < K4; ++i) {                            // registers behind k4 hold zeros
    zx = fmaf(a[i].x, v[i].x, zx);
    zy = fmaf(a[i].y, v[i].y, zy);
    zz = fmaf(a[i].z, v[i].z, zz);
    zw = fmaf(a[i].w, v[i].w, zw);
  }
  return (zx + zy) + (zz + zw);
}

template <int K4>
__device__ __forceinline__ void match_load_row(float4 (&a)[K4], const float* __restrict__ p, int k4) {
#pragma unroll
  for (int i = 0; i < K4; ++i) a[i] = i < k4 ? ld4u(p + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// thread = batch row, block (x = class chunk, y = 256 rows): the chunk's running (max, sum exp) and the label's logit
template <int K4>
__global__ __launch_bounds__(kBlock) void match_fwd_kernel(MatchArgs a, float* __restrict__ pm, float* __restrict__ ps,
                                                           float* __restrict__ lab) {
  const int64_t b = (int64_t)blockIdx.y * kBlock + threadIdx.x;
  const bool live = b < a.B;
  const int64_t bb = live ? b : a.B - 1;
  float4 u[K4];
  match_load_row<K4>(u, a.U + bb * a.ldu, a.k4);
  const int64_t lb = a.label[bb * a.ldl];
  const int64_t c0 = (int64_t)blockIdx.x * a.chunk, c1 = c0 + a.chunk < a.C ? c0 + a.chunk : a.C;
  float m = -INFINITY, s = 0.f, zl = 0.f;
  for (int64_t c = c0; c < c1; ++c) {
    float z = match_logit<K4>(u, a.V + c * a.ldv, a.k4);
    if (a.bias != nullptr) z += a.bias[c];
    const float d = z - m, e = expf(-fabsf(d));             // the first class: d = +inf, e = 0, s = 0 * 0 + 1
    s = d > 0.f ? fmaf(s, e, 1.f) : s + e;
    m = fmaxf(m, z);
    if (c == lb) zl = z;
  }
  if (!live) return;
  pm[b * a.nch + blockIdx.x] = m;
  ps[b * a.nch + blockIdx.x] = s;
  if (lb >= c0 && lb < c1) lab[b] = zl;
}

// thread = batch row: lse over the chunks in chunk order, term[b] = lse - logit[b, label]
__global__ __launch_bounds__(kBlock) void match_lse_kernel(int64_t B, int64_t C, int nch, const float* __restrict__ pm,
                                                           const float* __restrict__ ps, const float* __restrict__ lab,
                                                           const int64_t* __restrict__ label, int64_t ldl,
                                                           float* __restrict__ lse, float* __restrict__ term,
                                                           int32_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  float m = -INFINITY;
  for (int c = 0; c < nch; ++c) m = fmaxf(m, pm[b * nch + c]);
  float s = 0.f;
  for (int c = 0; c < nch; ++c) s = fmaf(ps[b * nch + c], expf(pm[b * nch + c] - m), s);
  const float l = m + logf(s);
  lse[b] = l;
  const int64_t lb = label[b * ldl];
  if (lb < 0 || lb >= C) {                                  // no class: the row contributes its lse alone
    atomicOr(status, REC_FLAG_INDEX_OOB);
    term[b] = l;
  } else {
    term[b] = l - lab[b];
  }
}

__global__ __launch_bounds__(kBlock) void match_mean_kernel(int64_t n, const float* __restrict__ term, float scale,
                                                            float* __restrict__ out) {
  __shared__ float red[kBlock];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) s += term[i];
  s = dmr_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// thread = batch row: dUp[b, chunk, :] = sum_{c in chunk} G[b,c] V_c (ascending c), G = scale (exp(z - lse_b) - [c == label_b])
template <int K4>
__global__ __launch_bounds__(kBlock) void match_du_kernel(MatchArgs a, const float* __restrict__ lse, float scale,
                                                          float* __restrict__ dUp) {
  const int64_t b = (int64_t)blockIdx.y * kBlock + threadIdx.x;
  const bool live = b < a.B;
  const int64_t bb = live ? b : a.B - 1;
  float4 u[K4], du[K4];
  match_load_row<K4>(u, a.U + bb * a.ldu, a.k4);
#pragma unroll
  for (int i = 0; i < K4; ++i) du[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t lb = a.label[bb * a.ldl];
  const float l = lse[bb];
  const int64_t c0 = (int64_t)blockIdx.x * a.chunk, c1 = c0 + a.chunk < a.C ? c0 + a.chunk : a.C;
  for (int64_t c = c0; c < c1; ++c) {
    const float* v = a.V + c * a.ldv;
    float z = match_logit<K4>(u, v, a.k4);
    if (a.bias != nullptr) z += a.bias[c];
    const float g = scale * (expf(z - l) - (c == lb ? 1.f : 0.f));
#pragma unroll
    for (int i = 0; i < K4; ++i)
      if (i < a.k4) {
        du[i].x = fmaf(g, v[4 * i], du[i].x);
        du[i].y = fmaf(g, v[4 * i + 1], du[i].y);
        du[i].z = fmaf(g, v[4 * i + 2], du[i].z);
        du[i].w = fmaf(g, v[4 * i + 3], du[i].w);
      }
  }
  if (!live) return;
  float4* o = reinterpret_cast<float4*>(dUp + (b * a.nch + blockIdx.x) * 4 * a.k4);
#pragma unroll
  for (int i = 0; i < K4; ++i)
    if (i < a.k4) o[i] = du[i];
}

// dU[b, k] = sum over the chunks, in chunk order
__global__ __launch_bounds__(kBlock) void match_du_fold_kernel(int64_t total, int K, int nch, const float* __restrict__ dUp,
                                                               float* __restrict__ dU, int64_t lddu) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / K;
  const int k = (int)(idx % K);
  float s = 0.f;
  for (int c = 0; c < nch; ++c) s += dUp[(b * nch + c) * K + k];
  dU[b * lddu + k] = s;
}

// thread = class, block (x = 256 classes, y = batch chunk): dVp[chunk, c, :] = sum_{b in chunk} G[b,c] U_b (ascending b)
template <int K4>
__global__ __launch_bounds__(kBlock) void match_dv_kernel(MatchArgs a, const float* __restrict__ lse, float scale,
                                                          float* __restrict__ dVp) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = c < a.C;
  const int64_t cc = live ? c : a.C - 1;
  float4 v[K4], dv[K4];
  match_load_row<K4>(v, a.V + cc * a.ldv, a.k4);
#pragma unroll
  for (int i = 0; i < K4; ++i) dv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float bc = a.bias != nullptr ? a.bias[cc] : 0.f;
  const int64_t b0 = (int64_t)blockIdx.y * a.chunk, b1 = b0 + a.chunk < a.B ? b0 + a.chunk : a.B;
  for (int64_t b = b0; b < b1; ++b) {
    const float* up = a.U + b * a.ldu;
    float4 u[K4];
    match_load_row<K4>(u, up, a.k4);
    float z = match_logit_reg<K4>(u, v);
    if (a.bias != nullptr) z += bc;
    const float g = scale * (expf(z - lse[b]) - (cc == a.label[b * a.ldl] ? 1.f : 0.f));
#pragma unroll
    for (int i = 0; i < K4; ++i) {
      dv[i].x = fmaf(g, u[i].x, dv[i].x);
      dv[i].y = fmaf(g, u[i].y, dv[i].y);
      dv[i].z = fmaf(g, u[i].z, dv[i].z);
      dv[i].w = fmaf(g, u[i].w, dv[i].w);
    }
  }
  if (!live) return;
  float4* o = reinterpret_cast<float4*>(dVp + ((int64_t)blockIdx.y * a.C + c) * 4 * a.k4);
#pragma unroll
  for (int i = 0; i < K4; ++i)
    if (i < a.k4) o[i] = dv[i];
}

// dV[c, k] (+)= sum over the batch chunks, in chunk order
__global__ __launch_bounds__(kBlock) void match_dv_fold_kernel(int64_t C, int K, int nbch, const float* __restrict__ dVp,
                                                               float* __restrict__ dV, int64_t lddv, int accumulate) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= C * K) return;
  const int64_t c = idx / K;
  const int k = (int)(idx % K);
  float s = 0.f;
  for (int q = 0; q < nbch; ++q) s += dVp[((int64_t)q * C + c) * K + k];
  dV[c * lddv + k] = accumulate ? dV[c * lddv + k] + s : s;
}

// ---------------------------------------------------------------- tail glue, one block per sample
// hist_sum[b,:] = sum_t hist[b,t,:] (ALL t: the reference ignores the mask, net.py:471); prod = item_eb * hist_sum;
// rel_u2i[b] = uv[b,1,:] . V[cate_id[b]];  U2[b,:] = uv[b,0,:] * float(match_mask[b])
__global__ __launch_bounds__(kBlock) void dmr_tail_fwd_kernel(int T, int D, const float* __restrict__ hist, int64_t ldh,
                                                              const float* __restrict__ item_eb, int64_t ld_item,
                                                              const float* __restrict__ uv,
                                                              const int64_t* __restrict__ match_mask, int64_t ldm,
                                                              const float* __restrict__ V, int64_t ldv, int64_t C,
                                                              const int64_t* __restrict__ cate_id,
                                                              float* __restrict__ hist_sum, int64_t ld_sum,
                                                              float* __restrict__ prod, int64_t ld_prod,
                                                              float* __restrict__ rel, int64_t ld_rel,
                                                              float* __restrict__ U2, int32_t* __restrict__ status) {
  __shared__ float red[kBlock];
  const int64_t b = blockIdx.x;
  const int E = D / 2;
  const float* h = hist + b * T * ldh;
  for (int d = threadIdx.x; d < D; d += kBlock) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += h[t * ldh + d];
    hist_sum[b * ld_sum + d] = s;
    prod[b * ld_prod + d] = item_eb[b * ld_item + d] * s;
  }
  const int64_t cid = cate_id[b];
  const bool ok = cid >= 0 && cid < C;
  if (!ok && threadIdx.x == 0) atomicOr(status, REC_FLAG_INDEX_OOB);
  const float mm = (float)match_mask[b * ldm];
  float s = 0.f;
  for (int e = threadIdx.x; e < E; e += kBlock) {
    s = fmaf(uv[(b * 2 + 1) * E + e], ok ? V[cid * ldv + e] : 0.f, s);
    U2[b * E + e] = uv[(b * 2) * E + e] * mm;
  }
  s = dmr_block_sum(s, red);
  if (threadIdx.x == 0) rel[b * ld_rel] = s;
}

// d_uv[b,0,:] = dU2[b,:] * match_mask[b];  d_uv[b,1,:] = d_rel[b] V[cate_id[b]];  dV_rows[b,:] = d_rel[b] uv[b,1,:]
__global__ __launch_bounds__(kBlock) void dmr_tail_bwd_match_kernel(int64_t total, int E, const float* __restrict__ dU2,
                                                                    const float* __restrict__ d_rel, int64_t ld_drel,
                                                                    const float* __restrict__ uv,
                                                                    const int64_t* __restrict__ match_mask, int64_t ldm,
                                                                    const float* __restrict__ V, int64_t ldv, int64_t C,
                                                                    const int64_t* __restrict__ cate_id,
                                                                    float* __restrict__ d_uv,
                                                                    float* __restrict__ dV_rows, int64_t ld_dvr) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / E;
  const int e = (int)(idx % E);
  const int64_t cid = cate_id[b];
  const float dr = d_rel[b * ld_drel];
  d_uv[(b * 2) * E + e] = dU2 != nullptr ? dU2[idx] * (float)match_mask[b * ldm] : 0.f;
  d_uv[(b * 2 + 1) * E + e] = (cid >= 0 && cid < C) ? dr * V[cid * ldv + e] : 0.f;
  dV_rows[b * ld_dvr + e] = dr * uv[(b * 2 + 1) * E + e];
}

// d_hist[b,t,:] += f1[b,t,:] + f2[b,t,:] + d_sum[b,:] + d_prod[b,:] * item_eb[b,:]   (f1, f2 nullable)
// d_item[b,:] = d_item_direct[b,:] + d_prod[b,:] * hist_sum[b,:] + sum_t d_ctx[b,t,:]   (ascending t)
__global__ __launch_bounds__(kBlock) void dmr_tail_bwd_hist_kernel(int T, int D, const float* __restrict__ f1,
                                                                   const float* __restrict__ f2,
                                                                   const float* __restrict__ d_sum, int64_t ld_dsum,
                                                                   const float* __restrict__ d_prod, int64_t ld_dprod,
                                                                   const float* __restrict__ item_eb, int64_t ld_item,
                                                                   const float* __restrict__ hist_sum, int64_t ld_sum,
                                                                   const float* __restrict__ d_item_direct, int64_t ld_did,
                                                                   const float* __restrict__ d_ctx, int64_t ld_ctx,
                                                                   float* __restrict__ d_hist, int64_t lddh,
                                                                   float* __restrict__ d_item, int64_t ld_ditem) {
  const int64_t b = blockIdx.x;
  for (int i = threadIdx.x; i < T * D; i += kBlock) {
    const int t = i / D, d = i % D;
    float a = d_sum[b * ld_dsum + d] + d_prod[b * ld_dprod + d] * item_eb[b * ld_item + d];
    if (f1 != nullptr) a += f1[(b * T + t) * D + d];
    if (f2 != nullptr) a += f2[(b * T + t) * D + d];
    d_hist[(b * T + t) * lddh + d] += a;
  }
  for (int d = threadIdx.x; d < D; d += kBlock) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += d_ctx[(b * T + t) * ld_ctx + d];
    d_item[b * ld_ditem + d] = (d_item_direct[b * ld_did + d] + d_prod[b * ld_dprod + d] * hist_sum[b * ld_sum + d]) + s;
  }
}

int pool_check(int64_t B, int32_t T, int32_t D, int32_t R, const int32_t* rows, PoolRows* out, const char* what) {
  REC_REQUIRE(B >= 0 && T > 0 && D > 0, REC_EINVAL, "%s: bad sizes (batch %lld, steps %d, dim %d)", what, (long long)B, T, D);
  REC_REQUIRE(rows != nullptr && R > 0 && R <= kPoolMaxRows, REC_EINVAL, "%s: num_rows %d must be in [1, %d]", what, R,
              kPoolMaxRows);
  REC_REQUIRE(B < (1ll << 31), REC_ESHAPE, "%s: batch too large", what);
  REC_REQUIRE((int64_t)T * D < (1ll << 31) / kPoolMaxRows, REC_ESHAPE, "%s: steps * dim too large", what);
  out->n = R;
  for (int i = 0; i < kPoolMaxRows; ++i) out->r[i] = 0;
  for (int i = 0; i < R; ++i) {
    REC_REQUIRE(rows[i] >= 0 && rows[i] < T, REC_EINVAL, "%s: rows[%d] = %d is outside [0, %d)", what, i, rows[i], T);
    out->r[i] = rows[i];
  }
  return REC_OK;
}

int prelu_shape(int64_t m, int32_t n, int32_t num_alpha, int32_t row_mode, int32_t period, int32_t base, PreluShape* s,
                const char* what) {
  REC_REQUIRE(m >= 0 && n > 0 && num_alpha > 0, REC_EINVAL, "%s: bad sizes (m %lld, n %d, num_alpha %d)", what,
              (long long)m, n, num_alpha);
  if (row_mode) {
    REC_REQUIRE(period > 0 && base >= 0 && (int64_t)base + period <= num_alpha, REC_EINVAL,
                "%s: row mode needs period > 0 and base + period <= num_alpha (period %d, base %d, num_alpha %d)", what,
                period, base, num_alpha);
    REC_REQUIRE((int64_t)period * n < (1ll << 31), REC_ESHAPE, "%s: period * n too large", what);
    *s = PreluShape{m, n, period, n, base, (m + period - 1) / period, (int64_t)period * n};
  } else {
    REC_REQUIRE(num_alpha == n, REC_EINVAL, "%s: column mode needs num_alpha == n (%d != %d)", what, num_alpha, n);
    *s = PreluShape{m, n, 1, 1, 0, m, n};
  }
  REC_REQUIRE((s->mv + kPreluRows - 1) / kPreluRows < 65536, REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

struct MatchPlan {
  int64_t chunk;     // classes per chunk
  int nch;
  int64_t bchunk;    // rows per batch chunk
  int nbch;
};

int match_check(int64_t B, int64_t C, int32_t K, const float* U, int64_t ldu, const float* V, int64_t ldv, MatchPlan* p,
                const char* what) {
  REC_REQUIRE(B >= 0 && C > 0 && K > 0, REC_EINVAL, "%s: bad sizes (batch %lld, classes %lld, k %d)", what, (long long)B,
              (long long)C, K);
  REC_REQUIRE(K % 4 == 0 && K <= kMatchMaxK, REC_ESHAPE, "%s: k %d unsupported (need a multiple of 4, <= %d)", what, K,
              kMatchMaxK);
  REC_REQUIRE(ldu >= K && ldv >= K && ldu % 4 == 0 && ldv % 4 == 0, REC_EINVAL,
              "%s: the row strides of U and V must be multiples of 4, >= k", what);
  REC_REQUIRE(((uintptr_t)U) % 16 == 0 && ((uintptr_t)V) % 16 == 0, REC_EINVAL, "%s: U and V must be 16-byte aligned", what);
  REC_REQUIRE((B + kBlock - 1) / kBlock < 65536 && (C + kBlock - 1) / kBlock < (1ll << 31), REC_ESHAPE,
              "%s: batch or classes too large", what);
  p->chunk = (C + kMatchChunks - 1) / kMatchChunks;
  p->nch = (int)((C + p->chunk - 1) / p->chunk);
  p->bchunk = B > 0 ? (B + kMatchBatchChunks - 1) / kMatchBatchChunks : 1;
  p->nbch = B > 0 ? (int)((B + p->bchunk - 1) / p->bchunk) : 0;
  return REC_OK;
}

size_t match_fwd_bytes(int64_t B) { return (size_t)B * (2 * kMatchChunks + 2) * sizeof(float); }
size_t match_bwd_bytes(int64_t B, int64_t C, int K) {
  const size_t du = (size_t)B * kMatchChunks * K, dv = (size_t)kMatchBatchChunks * (size_t)C * K;
  return (du > dv ? du : dv) * sizeof(float);
}

// K / 4 -> the register-array size of the instantiation
#define DMR_MATCH_DISPATCH(k4, CALL) \
  do {                               \
    if ((k4) <= 1) { CALL(1); }      \
    else if ((k4) <= 2) { CALL(2); } \
    else if ((k4) <= 4) { CALL(4); } \
    else if ((k4) <= 8) { CALL(8); } \
    else if ((k4) <= 12) { CALL(12); } \
    else { CALL(16); }               \
  } while (0)

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_dmr_prefix_pool_fwd(int64_t batch, int32_t steps, int32_t dim, const float* score, const int64_t* mask,
                                       int64_t ld_mask, const float* hist, int64_t ld_hist, int32_t num_rows,
                                       const int32_t* rows, float* out, int64_t ld_out, float* rel, int64_t ld_rel,
                                       float* w, void* stream) {
  PoolRows pr;
  int rc = pool_check(batch, steps, dim, num_rows, rows, &pr, "rec_dmr_prefix_pool_fwd");
  if (rc != REC_OK) return rc;
  if (batch == 0) return REC_OK;
  REC_REQUIRE(score && mask && hist && out && w, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ld_mask >= steps && ld_hist >= dim && ld_out >= (int64_t)num_rows * dim && (rel == nullptr || ld_rel >= 1),
              REC_EINVAL, "rec_dmr_prefix_pool_fwd: a stride is smaller than its row");
  hipLaunchKernelGGL(dmr_prefix_pool_fwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps, dim,
                     score, mask, ld_mask, hist, ld_hist, pr, out, ld_out, rel, ld_rel, w);
  return check_launch("rec_dmr_prefix_pool_fwd");
}

extern "C" int rec_dmr_prefix_pool_bwd(int64_t batch, int32_t steps, int32_t dim, const int64_t* mask, int64_t ld_mask,
                                       const float* hist, int64_t ld_hist, int32_t num_rows, const int32_t* rows,
                                       const float* w, const float* d_out, int64_t ld_dout, const float* d_rel,
                                       int64_t ld_drel, float* dscore, float* d_hist, int64_t ld_dhist,
                                       int32_t accumulate_hist, void* stream) {
  PoolRows pr;
  int rc = pool_check(batch, steps, dim, num_rows, rows, &pr, "rec_dmr_prefix_pool_bwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(steps <= kPoolMaxSteps, REC_ESHAPE, "rec_dmr_prefix_pool_bwd: steps %d > %d", steps, kPoolMaxSteps);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(mask && hist && w && d_out && dscore && d_hist, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ld_mask >= steps && ld_hist >= dim && ld_dhist >= dim && ld_dout >= (int64_t)num_rows * dim &&
                  (d_rel == nullptr || ld_drel >= 1),
              REC_EINVAL, "rec_dmr_prefix_pool_bwd: a stride is smaller than its row");
  REC_REQUIRE(d_hist != hist && d_hist != d_out && dscore != w, REC_EINVAL,
              "rec_dmr_prefix_pool_bwd: the gradients alias no input");
  hipLaunchKernelGGL(dmr_prefix_pool_bwd_kernel, dim3((unsigned)batch), dim3(kBlock), (size_t)2 * steps * sizeof(float),
                     (hipStream_t)stream, steps, dim, mask, ld_mask, hist, ld_hist, pr, w, d_out, ld_dout, d_rel, ld_drel,
                     dscore, d_hist, ld_dhist, accumulate_hist);
  return check_launch("rec_dmr_prefix_pool_bwd");
}

extern "C" int rec_prelu_fwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* alpha, int32_t num_alpha,
                             int32_t row_mode, int32_t period, int32_t base, float* Y, int64_t ldy, void* stream) {
  PreluShape s;
  int rc = prelu_shape(m, n, num_alpha, row_mode, period, base, &s, "rec_prelu_fwd");
  if (rc != REC_OK) return rc;
  if (m == 0) return REC_OK;
  REC_REQUIRE(X && alpha && Y, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ldx >= n && ldy >= n, REC_EINVAL, "rec_prelu_fwd: a row stride is smaller than n");
  const dim3 grid((unsigned)((s.nv + kBlock - 1) / kBlock), (unsigned)((s.mv + kPreluRows - 1) / kPreluRows));
  hipLaunchKernelGGL(prelu_fwd_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, s, X, ldx, alpha, Y, ldy);
  return check_launch("rec_prelu_fwd");
}

extern "C" int rec_prelu_workspace_bytes(int64_t m, int32_t n, int32_t row_mode, int32_t period, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  PreluShape s;
  int rc = prelu_shape(m, n, row_mode ? period : n, row_mode, period, 0, &s, "rec_prelu_workspace_bytes");
  if (rc != REC_OK) return rc;
  *bytes = (size_t)((s.mv + kPreluRows - 1) / kPreluRows) * (size_t)s.nv * sizeof(float);
  return REC_OK;
}

extern "C" int rec_prelu_bwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* dY, int64_t lddy,
                             const float* alpha, int32_t num_alpha, int32_t row_mode, int32_t period, int32_t base,
                             float* dX, int64_t lddx, float* dalpha, void* workspace, size_t workspace_bytes,
                             void* stream) {
  PreluShape s;
  int rc = prelu_shape(m, n, num_alpha, row_mode, period, base, &s, "rec_prelu_bwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(alpha && dalpha, REC_EINVAL, "null pointer argument");
  const int64_t nblk = (s.mv + kPreluRows - 1) / kPreluRows;
  hipStream_t st = (hipStream_t)stream;
  if (m > 0) {
    REC_REQUIRE(X && dY && dX, REC_EINVAL, "null pointer argument");
    REC_REQUIRE(ldx >= n && lddy >= n && lddx >= n, REC_EINVAL, "rec_prelu_bwd: a row stride is smaller than n");
    REC_REQUIRE(dX != X, REC_EINVAL, "rec_prelu_bwd: dX must not be X");
    const size_t need = (size_t)nblk * (size_t)s.nv * sizeof(float);
    REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "prelu workspace %zu < %zu bytes", workspace_bytes, need);
    REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
    const dim3 grid((unsigned)((s.nv + kBlock - 1) / kBlock), (unsigned)nblk);
    hipLaunchKernelGGL(prelu_bwd_kernel, grid, dim3(kBlock), 0, st, s, X, ldx, dY, lddy, alpha, dX, lddx,
                       (float*)workspace);
    rc = check_launch("rec_prelu_bwd");
    if (rc != REC_OK) return rc;
  }
  hipLaunchKernelGGL(prelu_fold_kernel, dim3((unsigned)num_alpha), dim3(kBlock), 0, st, s, nblk, (const float*)workspace,
                     dalpha);
  return check_launch("rec_prelu_bwd (fold)");
}

extern "C" int rec_dmr_match_loss_workspace_bytes(int64_t batch, int64_t classes, int32_t k, size_t* fwd_bytes,
                                                  size_t* bwd_bytes) {
  REC_REQUIRE(fwd_bytes && bwd_bytes, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(batch >= 0 && classes > 0 && k > 0, REC_EINVAL, "dmr match loss: bad sizes (batch %lld, classes %lld, k %d)",
              (long long)batch, (long long)classes, k);
  *fwd_bytes = match_fwd_bytes(batch);
  *bwd_bytes = match_bwd_bytes(batch, classes, k);
  return REC_OK;
}

extern "C" int rec_dmr_match_loss_fwd(int64_t batch, int64_t classes, int32_t k, const float* U, int64_t ldu,
                                      const float* V, int64_t ldv, const float* bias, const int64_t* label,
                                      int64_t ld_label, float* loss, float* lse, int32_t* status, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  REC_REQUIRE(batch == 0 || (U && V), REC_EINVAL, "null pointer argument");
  MatchPlan p;
  int rc = match_check(batch, classes, k, U, ldu, V, ldv, &p, "rec_dmr_match_loss_fwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(loss, REC_EINVAL, "null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  float* term = nullptr;
  if (batch > 0) {
    REC_REQUIRE(label && lse && status, REC_EINVAL, "null pointer argument");
    REC_REQUIRE(ld_label >= 1, REC_EINVAL, "rec_dmr_match_loss_fwd: ld_label must be >= 1");
    REC_REQUIRE(workspace_bytes >= match_fwd_bytes(batch), REC_EWORKSPACE, "dmr match loss workspace %zu < %zu bytes",
                workspace_bytes, match_fwd_bytes(batch));
    REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
    float* pm = (float*)workspace;
    float* ps = pm + batch * kMatchChunks;
    float* lab = ps + batch * kMatchChunks;
    term = lab + batch;
    const MatchArgs a{batch, classes, k / 4, U, ldu, V, ldv, bias, label, ld_label, p.chunk, p.nch};
    const dim3 grid((unsigned)p.nch, (unsigned)((batch + kBlock - 1) / kBlock));
#define DMR_CALL(N) hipLaunchKernelGGL(match_fwd_kernel<N>, grid, dim3(kBlock), 0, st, a, pm, ps, lab)
    DMR_MATCH_DISPATCH(k / 4, DMR_CALL);
#undef DMR_CALL
    rc = check_launch("rec_dmr_match_loss_fwd");
    if (rc != REC_OK) return rc;
    hipLaunchKernelGGL(match_lse_kernel, dim3((unsigned)((batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, batch,
                       classes, p.nch, pm, ps, lab, label, ld_label, lse, term, status);
    rc = check_launch("rec_dmr_match_loss_fwd (lse)");
    if (rc != REC_OK) return rc;
  }
  hipLaunchKernelGGL(match_mean_kernel, dim3(1), dim3(kBlock), 0, st, batch, (const float*)term,
                     batch > 0 ? 1.f / (float)batch : 0.f, loss);
  return check_launch("rec_dmr_match_loss_fwd (mean)");
}

extern "C" int rec_dmr_match_loss_bwd(int64_t batch, int64_t classes, int32_t k, const float* U, int64_t ldu,
                                      const float* V, int64_t ldv, const float* bias, const int64_t* label,
                                      int64_t ld_label, const float* lse, float d_loss, float* dU, int64_t lddu,
                                      float* dV, int64_t lddv, int32_t accumulate_dv, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  REC_REQUIRE(batch == 0 || (U && V), REC_EINVAL, "null pointer argument");
  MatchPlan p;
  int rc = match_check(batch, classes, k, U, ldu, V, ldv, &p, "rec_dmr_match_loss_bwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(dV && lddv >= k, REC_EINVAL, "rec_dmr_match_loss_bwd: dV is null or its row stride is smaller than k");
  REC_REQUIRE(dV != V, REC_EINVAL, "rec_dmr_match_loss_bwd: dV must not be V");
  hipStream_t st = (hipStream_t)stream;
  const int64_t cgrid = (classes * k + kBlock - 1) / kBlock;
  REC_REQUIRE(cgrid < (1ll << 31), REC_ESHAPE, "rec_dmr_match_loss_bwd: classes * k too large");
  if (batch > 0) {
    REC_REQUIRE(label && lse && dU, REC_EINVAL, "null pointer argument");
    REC_REQUIRE(ld_label >= 1 && lddu >= k, REC_EINVAL, "rec_dmr_match_loss_bwd: a stride is smaller than its row");
    REC_REQUIRE(dU != U, REC_EINVAL, "rec_dmr_match_loss_bwd: dU must not be U");
    const size_t need = match_bwd_bytes(batch, classes, k);
    REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "dmr match loss workspace %zu < %zu bytes", workspace_bytes, need);
    REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
    REC_REQUIRE(((uintptr_t)workspace) % 16 == 0, REC_EINVAL, "rec_dmr_match_loss_bwd: workspace must be 16-byte aligned");
    const float scale = d_loss / (float)batch;
    float* part = (float*)workspace;
    MatchArgs a{batch, classes, k / 4, U, ldu, V, ldv, bias, label, ld_label, p.chunk, p.nch};
    const dim3 grid((unsigned)p.nch, (unsigned)((batch + kBlock - 1) / kBlock));
#define DMR_CALL(N) hipLaunchKernelGGL(match_du_kernel<N>, grid, dim3(kBlock), 0, st, a, lse, scale, part)
    DMR_MATCH_DISPATCH(k / 4, DMR_CALL);
#undef DMR_CALL
    rc = check_launch("rec_dmr_match_loss_bwd (dU)");
    if (rc != REC_OK) return rc;
    const int64_t total = batch * k;
    hipLaunchKernelGGL(match_du_fold_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, total, k,
                       p.nch, (const float*)part, dU, lddu);
    rc = check_launch("rec_dmr_match_loss_bwd (dU fold)");
    if (rc != REC_OK) return rc;
    a.chunk = p.bchunk;
    a.nch = p.nbch;
    const dim3 vgrid((unsigned)((classes + kBlock - 1) / kBlock), (unsigned)p.nbch);
#define DMR_CALL(N) hipLaunchKernelGGL(match_dv_kernel<N>, vgrid, dim3(kBlock), 0, st, a, lse, scale, part)
    DMR_MATCH_DISPATCH(k / 4, DMR_CALL);
#undef DMR_CALL
    rc = check_launch("rec_dmr_match_loss_bwd (dV)");
    if (rc != REC_OK) return rc;
  }
  hipLaunchKernelGGL(match_dv_fold_kernel, dim3((unsigned)cgrid), dim3(kBlock), 0, st, classes, k, p.nbch,
                     (const float*)workspace, dV, lddv, accumulate_dv);
  return check_launch("rec_dmr_match_loss_bwd (dV fold)");
}

extern "C" int rec_dmr_tail_fwd(int64_t batch, int32_t steps, int32_t dim, const float* hist, int64_t ld_hist,
                                const float* item_eb, int64_t ld_item, const float* uv, const int64_t* match_mask,
                                int64_t ld_mm, const float* V, int64_t ldv, int64_t classes, const int64_t* cate_id,
                                float* hist_sum, int64_t ld_sum, float* prod, int64_t ld_prod, float* rel_u2i,
                                int64_t ld_rel, float* U2, int32_t* status, void* stream) {
  REC_REQUIRE(batch >= 0 && steps > 0 && dim > 0 && dim % 2 == 0 && classes > 0, REC_EINVAL,
              "rec_dmr_tail_fwd: bad sizes (batch %lld, steps %d, dim %d, classes %lld)", (long long)batch, steps, dim,
              (long long)classes);
  REC_REQUIRE(batch < (1ll << 31), REC_ESHAPE, "rec_dmr_tail_fwd: batch too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(hist && item_eb && uv && match_mask && V && cate_id && hist_sum && prod && rel_u2i && U2 && status,
              REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ld_hist >= dim && ld_item >= dim && ld_sum >= dim && ld_prod >= dim && ldv >= dim / 2 && ld_mm >= 1 &&
                  ld_rel >= 1,
              REC_EINVAL, "rec_dmr_tail_fwd: a stride is smaller than its row");
  hipLaunchKernelGGL(dmr_tail_fwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps, dim, hist,
                     ld_hist, item_eb, ld_item, uv, match_mask, ld_mm, V, ldv, classes, cate_id, hist_sum, ld_sum, prod,
                     ld_prod, rel_u2i, ld_rel, U2, status);
  return check_launch("rec_dmr_tail_fwd");
}

extern "C" int rec_dmr_tail_bwd_match(int64_t batch, int32_t half_dim, const float* dU2, const float* d_rel,
                                      int64_t ld_drel, const float* uv, const int64_t* match_mask, int64_t ld_mm,
                                      const float* V, int64_t ldv, int64_t classes, const int64_t* cate_id, float* d_uv,
                                      float* dV_rows, int64_t ld_dvr, void* stream) {
  REC_REQUIRE(batch >= 0 && half_dim > 0 && classes > 0, REC_EINVAL, "rec_dmr_tail_bwd_match: bad sizes (batch %lld, dim %d)",
              (long long)batch, half_dim);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(d_rel && uv && match_mask && V && cate_id && d_uv && dV_rows, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ld_drel >= 1 && ld_mm >= 1 && ldv >= half_dim && ld_dvr >= half_dim, REC_EINVAL,
              "rec_dmr_tail_bwd_match: a stride is smaller than its row");
  const int64_t total = batch * half_dim, grid = (total + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_dmr_tail_bwd_match: batch too large");
  hipLaunchKernelGGL(dmr_tail_bwd_match_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, total, half_dim,
                     dU2, d_rel, ld_drel, uv, match_mask, ld_mm, V, ldv, classes, cate_id, d_uv, dV_rows, ld_dvr);
  return check_launch("rec_dmr_tail_bwd_match");
}

extern "C" int rec_dmr_tail_bwd_hist(int64_t batch, int32_t steps, int32_t dim, const float* f1, const float* f2,
                                     const float* d_sum, int64_t ld_dsum, const float* d_prod, int64_t ld_dprod,
                                     const float* item_eb, int64_t ld_item, const float* hist_sum, int64_t ld_sum,
                                     const float* d_item_direct, int64_t ld_did, const float* d_ctx, int64_t ld_ctx,
                                     float* d_hist, int64_t ld_dhist, float* d_item, int64_t ld_ditem, void* stream) {
  REC_REQUIRE(batch >= 0 && steps > 0 && dim > 0, REC_EINVAL, "rec_dmr_tail_bwd_hist: bad sizes (batch %lld, steps %d, dim %d)",
              (long long)batch, steps, dim);
  REC_REQUIRE(batch < (1ll << 31) && (int64_t)steps * dim < (1ll << 31), REC_ESHAPE, "rec_dmr_tail_bwd_hist: too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(d_sum && d_prod && item_eb && hist_sum && d_item_direct && d_ctx && d_hist && d_item, REC_EINVAL,
              "null pointer argument");
  REC_REQUIRE(ld_dsum >= dim && ld_dprod >= dim && ld_item >= dim && ld_sum >= dim && ld_did >= dim && ld_ctx >= dim &&
                  ld_dhist >= dim && ld_ditem >= dim,
              REC_EINVAL, "rec_dmr_tail_bwd_hist: a stride is smaller than its row");
  hipLaunchKernelGGL(dmr_tail_bwd_hist_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps, dim, f1,
                     f2, d_sum, ld_dsum, d_prod, ld_dprod, item_eb, ld_item, hist_sum, ld_sum, d_item_direct, ld_did, d_ctx,
                     ld_ctx, d_hist, ld_dhist, d_item, ld_ditem);
  return check_launch("rec_dmr_tail_bwd_hist");
}
