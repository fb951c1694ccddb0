// BST (rank/bst, Behavior Sequence Transformer) on gfx950: the Transformer encoder block of the sequence line — multi-head
// self-attention, add + layer norm, LeakyReLU — and the glue of its input and tail.
//
//   rec_mha_fwd / rec_mha_bwd             <- bst/net.py:362-372 scaled_dot_product_attention between __split_heads_qkv and
//                                            __combine_heads: out[b,i,h] = sum_j drop(softmax_j(scale q_i . k_j)) v_j.
//                                            No [B,H,L,L] array: keys / values are walked in LDS tiles of 64 with the
//                                            running maximum subtracted (forward), the weights are recomputed from the
//                                            saved log-sum-exp (backward).
//   rec_add_layer_norm_fwd / _bwd         <- net.py:283-290: paddle.add + paddle.static.nn.layer_norm with fresh scale 1 /
//                                            bias 0, i.e. a parameter-free layer norm over the last axis
//   rec_leaky_relu_fwd / _bwd             <- paddle.nn.LeakyReLU (net.py:190,207)
//   rec_bst_embed_fwd / _bwd, rec_bst_possum_fwd / _bwd, rec_bst_add <- net.py:421-442 (seven lookups, two concats),
//                                            net.py:456 + 74 (sum over the positions, + bias), paddle.add of net.py:283
//
// Attention kernels.  Products are plain f32 FMAs.  A block is 64 rows of one (sample, head) x 4 lanes per row; lane c of a
// row owns the float4 chunks c, c + 4, c + 8, c + 12 of the head width (d_k, d_v multiples of 4, at most 64), so a dot
// product is a per-lane FMA chain over its chunks and one 4-lane butterfly — the same chain in all three kernels, so the
// backward's exp(s - lse) sees the forward's s.  The other side of the product (keys and values in the forward and the
// dQ pass, queries and dO in the dK / dV pass) sits in LDS, 64 rows a tile; every lane of a wave reads the same tile row
// (4 distinct float4: a broadcast).  The forward keeps (m, l, acc) per row and rescales per key.  The backward is two
// passes without atomics: blocks over query tiles write D_i and dQ, blocks over key tiles write dK and dV.  D_i = sum_j
// P_ij dP_ij / sum_j P_ij (dP_ij = keep_ij / (1 - p) dO_i . v_j) is a sweep of its own over the recomputed weights.  It equals dO_i . O_i
// with the DROPPED output O, dropout or not, but only in exact arithmetic: the forward's weights differ from exp(s - lse)
// by a rounding, and dS_ij = P_ij (dP_ij - D_i) has to sum to zero over j to rounding — dQ_i = sum_j dS_ij k_j cancels
// against the part the keys have in common (DESIGN.md has what was measured with either form).
// The keep rule is rec_dropout's: element e of the virtual [B H L, L] matrix is kept iff bits 32.. of mix64(key + e) are
// >= p 2^32, key = mix64(seed ^ mix64(stream + golden)).
// Every sum has a fixed order and there are no atomics on floats: a rerun is bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kMhaTile = 64;                       // rows of a block (queries, or keys in the dK / dV pass) and of an LDS tile
constexpr int kMhaLanes = 4;                       // lanes of a row
constexpr int kMhaChunks = 16;                     // float4 of an LDS tile row: head widths up to 64
constexpr int kMhaMaxD = 64;
constexpr int kMhaMaxL = 8192;                     // grid.y = L / 64 and an O(L^2) walk per (sample, head)
constexpr int kLnRows = kBlock / kWave;            // layer norm: one wave per row

struct MhaArgs {
  int L, H, dk4, dv4;
  const float* q;
  const float* k;
  const float* v;
  int64_t ldq, ldk, ldv;
  float scale, inv_keep;
  uint32_t thresh;
  uint64_t key;
  int drop;
};

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float s) {
  s = fmaf(a.x, b.x, s);
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

__device__ __forceinline__ void axpy4(float4& y, float a, const float4& x) {
  y.x = fmaf(a, x.x, y.x);
  y.y = fmaf(a, x.y, y.y);
  y.z = fmaf(a, x.z, y.z);
  y.w = fmaf(a, x.w, y.w);
}

__device__ __forceinline__ bool mha_keep(const MhaArgs& a, uint64_t e) {
  return (uint32_t)(mix64(a.key + e) >> 32) >= a.thresh;
}

// rows j0 .. j0 + 63 of one head of a [B L, ld] matrix -> tile[row][chunk]; rows past L and chunks past d4 keep their zeros
__device__ __forceinline__ void mha_load_tile(float4* tile, const float* src, int64_t ld, int64_t row0, int j0, int L, int col0,
                                              int d4) {
  for (int idx = threadIdx.x; idx < kMhaTile * d4; idx += kBlock) {
    const int r = idx / d4, ch = idx - r * d4;
    if (j0 + r < L)
      tile[r * kMhaChunks + ch] = *reinterpret_cast<const float4*>(src + (row0 + j0 + r) * ld + col0 + ch * 4);
  }
}

__device__ __forceinline__ void mha_load_row(float4 (&reg)[4], const float* src, int c, int d4) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ch = c + kMhaLanes * u;
    reg[u] = ch < d4 ? *reinterpret_cast<const float4*>(src + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void mha_store_row(float* dst, const float4 (&reg)[4], float f, int c, int d4) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ch = c + kMhaLanes * u;
    if (ch < d4)
      *reinterpret_cast<float4*>(dst + ch * 4) = make_float4(reg[u].x * f, reg[u].y * f, reg[u].z * f, reg[u].w * f);
  }
}

__device__ __forceinline__ void mha_zero_tiles(float4* t0, float4* t1) {
  for (int idx = threadIdx.x; idx < kMhaTile * kMhaChunks; idx += kBlock)
    t0[idx] = t1[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid (B H, ceil(L / 64)).  out [B L, H d_v] (row stride ldo), lse [B H, L]
__global__ __launch_bounds__(kBlock) void mha_fwd_kernel(MhaArgs a, float* __restrict__ out, int64_t ldo,
                                                         float* __restrict__ lse) {
  __shared__ float4 sK[kMhaTile * kMhaChunks];
  __shared__ float4 sV[kMhaTile * kMhaChunks];
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int c = threadIdx.x & (kMhaLanes - 1);
  const int i = blockIdx.y * kMhaTile + (threadIdx.x >> 2);
  const bool valid = i < a.L;
  const int ic = valid ? i : a.L - 1;                      // a row past L computes a copy of row L-1 and stores nothing
  const int64_t row0 = (int64_t)b * a.L;
  float4 q[4], acc[4];
  mha_load_row(q, a.q + (row0 + ic) * a.ldq + h * a.dk4 * 4, c, a.dk4);
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, l = 0.f;
  const uint64_t e0 = ((uint64_t)bh * a.L + ic) * a.L;
  mha_zero_tiles(sK, sV);
  for (int j0 = 0; j0 < a.L; j0 += kMhaTile) {
    __syncthreads();
    mha_load_tile(sK, a.k, a.ldk, row0, j0, a.L, h * a.dk4 * 4, a.dk4);
    mha_load_tile(sV, a.v, a.ldv, row0, j0, a.L, h * a.dv4 * 4, a.dv4);
    __syncthreads();
    const int nj = min(kMhaTile, a.L - j0);
    for (int jj = 0; jj < nj; ++jj) {
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) s = dot4(q[u], sK[jj * kMhaChunks + c + kMhaLanes * u], s);
      s = group_sum<kMhaLanes>(s) * a.scale;
      const float mn = fmaxf(m, s);
      const float corr = expf(m - mn), p = expf(s - mn);
      l = fmaf(l, corr, p);
      float pd = p;
      if (a.drop) pd = mha_keep(a, e0 + (uint64_t)(j0 + jj)) ? p * a.inv_keep : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dv4) {
          const float4 vv = sV[jj * kMhaChunks + c + kMhaLanes * u];
          acc[u].x = fmaf(pd, vv.x, acc[u].x * corr);
          acc[u].y = fmaf(pd, vv.y, acc[u].y * corr);
          acc[u].z = fmaf(pd, vv.z, acc[u].z * corr);
          acc[u].w = fmaf(pd, vv.w, acc[u].w * corr);
        }
      m = mn;
    }
  }
  if (valid) {
    mha_store_row(out + (row0 + i) * ldo + h * a.dv4 * 4, acc, 1.f / l, c, a.dv4);
    if (c == 0) lse[bh * a.L + i] = m + logf(l);
  }
}

// grid (B H, ceil(L / 64)) over QUERY tiles: delta[b,h,i] = sum_j P_ij dP_ij;  dQ_i = scale sum_j P_ij (dP_ij - delta_i) k_j
__global__ __launch_bounds__(kBlock) void mha_dq_kernel(MhaArgs a, const float* __restrict__ dout, int64_t lddo,
                                                        const float* __restrict__ lse, float* __restrict__ delta,
                                                        float* __restrict__ dq, int64_t lddq) {
  __shared__ float4 sK[kMhaTile * kMhaChunks];
  __shared__ float4 sV[kMhaTile * kMhaChunks];
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int c = threadIdx.x & (kMhaLanes - 1);
  const int i = blockIdx.y * kMhaTile + (threadIdx.x >> 2);
  const bool valid = i < a.L;
  const int ic = valid ? i : a.L - 1;
  const int64_t row0 = (int64_t)b * a.L;
  float4 q[4], go[4], acc[4];
  mha_load_row(q, a.q + (row0 + ic) * a.ldq + h * a.dk4 * 4, c, a.dk4);
  mha_load_row(go, dout + (row0 + ic) * lddo + h * a.dv4 * 4, c, a.dv4);
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float li = lse[bh * a.L + ic];
  const uint64_t e0 = ((uint64_t)bh * a.L + ic) * a.L;
  mha_zero_tiles(sK, sV);
  // sweep 1: D_i = sum_j P_ij dP_ij / sum_j P_ij over the RECOMPUTED weights.  exp(s - lse) sums to 1 only to the rounding
  // of lse (an absolute 1e-7 at lse = 2), and sum_j P_ij (dP_ij - D_i) must cancel against the large part the keys share:
  // dividing by the weights' own sum makes it cancel by construction (dO_i . O_i does not)
  float dl = 0.f, z = 0.f;
  for (int j0 = 0; j0 < a.L; j0 += kMhaTile) {
    __syncthreads();
    mha_load_tile(sK, a.k, a.ldk, row0, j0, a.L, h * a.dk4 * 4, a.dk4);
    mha_load_tile(sV, a.v, a.ldv, row0, j0, a.L, h * a.dv4 * 4, a.dv4);
    __syncthreads();
    const int nj = min(kMhaTile, a.L - j0);
    for (int jj = 0; jj < nj; ++jj) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) s = dot4(q[u], sK[jj * kMhaChunks + c + kMhaLanes * u], s);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dv4) dp = dot4(go[u], sV[jj * kMhaChunks + c + kMhaLanes * u], dp);
      s = group_sum<kMhaLanes>(s) * a.scale;
      dp = group_sum<kMhaLanes>(dp);
      if (a.drop) dp = mha_keep(a, e0 + (uint64_t)(j0 + jj)) ? dp * a.inv_keep : 0.f;
      const float p = expf(s - li);
      z += p;
      dl = fmaf(p, dp, dl);
    }
  }
  dl /= z;                                                   // sum_j P_ij (dP_ij - D_i) = 0 whatever lse's rounding
  if (valid && c == 0) delta[bh * a.L + i] = dl;
  // sweep 2: dQ
  for (int j0 = 0; j0 < a.L; j0 += kMhaTile) {
    __syncthreads();
    mha_load_tile(sK, a.k, a.ldk, row0, j0, a.L, h * a.dk4 * 4, a.dk4);
    mha_load_tile(sV, a.v, a.ldv, row0, j0, a.L, h * a.dv4 * 4, a.dv4);
    __syncthreads();
    const int nj = min(kMhaTile, a.L - j0);
    for (int jj = 0; jj < nj; ++jj) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) s = dot4(q[u], sK[jj * kMhaChunks + c + kMhaLanes * u], s);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dv4) dp = dot4(go[u], sV[jj * kMhaChunks + c + kMhaLanes * u], dp);
      s = group_sum<kMhaLanes>(s) * a.scale;
      dp = group_sum<kMhaLanes>(dp);
      const float p = expf(s - li);
      if (a.drop) dp = mha_keep(a, e0 + (uint64_t)(j0 + jj)) ? dp * a.inv_keep : 0.f;
      const float ds = p * (dp - dl);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) axpy4(acc[u], ds, sK[jj * kMhaChunks + c + kMhaLanes * u]);
    }
  }
  if (valid) mha_store_row(dq + (row0 + i) * lddq + h * a.dk4 * 4, acc, a.scale, c, a.dk4);
}

// grid (B H, ceil(L / 64)) over KEY tiles: dV_j = sum_i Pd_ij dO_i;  dK_j = scale sum_i P_ij (dP_ij - delta_i) q_i (ascending i)
__global__ __launch_bounds__(kBlock) void mha_dkv_kernel(MhaArgs a, const float* __restrict__ dout, int64_t lddo,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         float* __restrict__ dk, int64_t lddk, float* __restrict__ dv,
                                                         int64_t lddv) {
  __shared__ float4 sQ[kMhaTile * kMhaChunks];
  __shared__ float4 sG[kMhaTile * kMhaChunks];
  __shared__ float sL[kMhaTile];
  __shared__ float sD[kMhaTile];
  const int64_t bh = blockIdx.x;
  const int b = (int)(bh / a.H), h = (int)(bh - (int64_t)b * a.H);
  const int c = threadIdx.x & (kMhaLanes - 1);
  const int j = blockIdx.y * kMhaTile + (threadIdx.x >> 2);
  const bool valid = j < a.L;
  const int jc = valid ? j : a.L - 1;
  const int64_t row0 = (int64_t)b * a.L;
  float4 kk[4], vv[4], ak[4], av[4];
  mha_load_row(kk, a.k + (row0 + jc) * a.ldk + h * a.dk4 * 4, c, a.dk4);
  mha_load_row(vv, a.v + (row0 + jc) * a.ldv + h * a.dv4 * 4, c, a.dv4);
#pragma unroll
  for (int u = 0; u < 4; ++u) ak[u] = av[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  mha_zero_tiles(sQ, sG);
  for (int i0 = 0; i0 < a.L; i0 += kMhaTile) {
    __syncthreads();
    mha_load_tile(sQ, a.q, a.ldq, row0, i0, a.L, h * a.dk4 * 4, a.dk4);
    mha_load_tile(sG, dout, lddo, row0, i0, a.L, h * a.dv4 * 4, a.dv4);
    if ((int)threadIdx.x < kMhaTile && i0 + (int)threadIdx.x < a.L) {
      sL[threadIdx.x] = lse[bh * a.L + i0 + threadIdx.x];
      sD[threadIdx.x] = delta[bh * a.L + i0 + threadIdx.x];
    }
    __syncthreads();
    const int ni = min(kMhaTile, a.L - i0);
    for (int ii = 0; ii < ni; ++ii) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) s = dot4(sQ[ii * kMhaChunks + c + kMhaLanes * u], kk[u], s);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dv4) dp = dot4(sG[ii * kMhaChunks + c + kMhaLanes * u], vv[u], dp);
      s = group_sum<kMhaLanes>(s) * a.scale;
      dp = group_sum<kMhaLanes>(dp);
      const float p = expf(s - sL[ii]);
      float pd = p;
      if (a.drop) {
        const bool keep = mha_keep(a, ((uint64_t)bh * a.L + (uint64_t)(i0 + ii)) * a.L + jc);
        pd = keep ? p * a.inv_keep : 0.f;
        dp = keep ? dp * a.inv_keep : 0.f;
      }
      const float ds = p * (dp - sD[ii]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dv4) axpy4(av[u], pd, sG[ii * kMhaChunks + c + kMhaLanes * u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (kMhaLanes * u < a.dk4) axpy4(ak[u], ds, sQ[ii * kMhaChunks + c + kMhaLanes * u]);
    }
  }
  if (valid) {
    mha_store_row(dk + (row0 + j) * lddk + h * a.dk4 * 4, ak, a.scale, c, a.dk4);
    mha_store_row(dv + (row0 + j) * lddv + h * a.dv4 * 4, av, 1.f, c, a.dv4);
  }
}

// ---------------------------------------------------------------- add + layer norm, one wave per row
// row r of y sits at (r / yg) * ldyg + (r % yg) * ldy when yg > 0 (rows 1.. of each sample of the tower input), else r * ldy
__device__ __forceinline__ int64_t ln_row(int64_t r, int64_t ld, int64_t g, int64_t ldg) {
  return g > 0 ? (r / g) * ldg + (r % g) * ld : r * ld;
}

__global__ __launch_bounds__(kBlock) void add_ln_fwd_kernel(int64_t m, int n, const float* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ r, int64_t ldr, float eps, float* y,
                                                            int64_t ldy, int64_t yg, int64_t ldyg, float* __restrict__ mean,
                                                            float* __restrict__ rstd) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
  if (row >= m) return;
  const float* xr = x + row * ldx;
  const float* rr = r != nullptr ? r + row * ldr : nullptr;
  float s = 0.f;
  for (int c = lane; c < n; c += kWave) s += rr != nullptr ? xr[c] + rr[c] : xr[c];
  const float mu = group_sum<kWave>(s) / (float)n;
  float v = 0.f;
  for (int c = lane; c < n; c += kWave) {
    const float t = (rr != nullptr ? xr[c] + rr[c] : xr[c]) - mu;
    v = fmaf(t, t, v);
  }
  const float rs = 1.f / sqrtf(group_sum<kWave>(v) / (float)n + eps);
  float* yr = y + ln_row(row, ldy, yg, ldyg);
  for (int c = lane; c < n; c += kWave) yr[c] = ((rr != nullptr ? xr[c] + rr[c] : xr[c]) - mu) * rs;   // y may be x or r
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

// no affine parameters: y IS the normalised row.  dx = rstd (dy - mean(dy) - y mean(dy y)); dx may be dy
__global__ __launch_bounds__(kBlock) void add_ln_bwd_kernel(int64_t m, int n, const float* __restrict__ y, int64_t ldy,
                                                            int64_t yg, int64_t ldyg, const float* __restrict__ rstd,
                                                            const float* dy, int64_t lddy, float* dx, int64_t lddx) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kLnRows + (threadIdx.x >> 6);
  if (row >= m) return;
  const float* yr = y + ln_row(row, ldy, yg, ldyg);
  const float* gr = dy + row * lddy;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < n; c += kWave) {
    s1 += gr[c];
    s2 = fmaf(gr[c], yr[c], s2);
  }
  const float c1 = group_sum<kWave>(s1) / (float)n, c2 = group_sum<kWave>(s2) / (float)n;
  const float rs = rstd[row];
  float* dr = dx + row * lddx;
  for (int c = lane; c < n; c += kWave) dr[c] = rs * (gr[c] - c1 - yr[c] * c2);
}

// ---------------------------------------------------------------- elementwise
__global__ __launch_bounds__(kBlock) void leaky_relu_fwd_kernel(int64_t m, int n, const float* x, int64_t ldx, float slope,
                                                                float* y, int64_t ldy) {
  const int64_t total = m * n;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / n;
    const int c = (int)(e - r * n);
    const float t = x[r * ldx + c];
    y[r * ldy + c] = t > 0.f ? t : slope * t;
  }
}

// reads the OUTPUT's sign (slope > 0: the input's sign; at +-0 the gradient takes the slope, as x > 0 ? 1 : slope)
__global__ __launch_bounds__(kBlock) void leaky_relu_bwd_kernel(int64_t m, int n, const float* __restrict__ y, int64_t ldy,
                                                                const float* dy, int64_t lddy, float slope, float* dx,
                                                                int64_t lddx) {
  const int64_t total = m * n;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t r = e / n;
    const int c = (int)(e - r * n);
    const float g = dy[r * lddy + c];
    dx[r * lddx + c] = y[r * ldy + c] > 0.f ? g : slope * g;
  }
}

__global__ __launch_bounds__(kBlock) void bst_add_kernel(int64_t m, int64_t n, const float* x, int64_t ldx, const float* r,
                                                         int64_t ldr, float* y, int64_t ldy) {
  const int64_t total = m * n;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
    const int64_t row = e / n, c = e - row * n;
    const float t = x[row * ldx + c];
    y[row * ldy + c] = r != nullptr ? t + r[row * ldr + c] : t;
  }
}

// ---------------------------------------------------------------- input and tail glue
// lookups 0..2: hist item / cat / position ([B, T] ids, row stride ld); 3..5: target item / cat / position; 6: user
// ([B] ids, element stride ld).  Tables are contiguous rows of their own width.
struct BstEmbed {
  const int64_t* ids[7];
  int64_t ld[7];
  const float* table[7];
  int64_t rows[7];
  int w[3];
};

__global__ __launch_bounds__(kBlock) void bst_embed_fwd_kernel(int T, BstEmbed a, float* __restrict__ X, int64_t ldx,
                                                               float* __restrict__ user_out, int64_t ld_user,
                                                               int32_t* __restrict__ status) {
  const int64_t b = blockIdx.x;
  const int L = T + 1, dm = a.w[0] + a.w[1] + a.w[2];
  bool bad = false;
  for (int e = threadIdx.x; e < L * dm; e += kBlock) {
    const int l = e / dm, c = e - l * dm;
    const int seg = c < a.w[0] ? 0 : (c < a.w[0] + a.w[1] ? 1 : 2);
    const int col = c - (seg == 0 ? 0 : (seg == 1 ? a.w[0] : a.w[0] + a.w[1]));
    const int t = l < T ? seg : seg + 3;
    const int64_t id = l < T ? a.ids[t][b * a.ld[t] + l] : a.ids[t][b * a.ld[t]];
    const bool ok = id >= 0 && id < a.rows[t];
    bad |= !ok;
    X[(b * L + l) * ldx + c] = ok ? a.table[t][id * a.w[seg] + col] : 0.f;
  }
  const int64_t uid = a.ids[6][b * a.ld[6]];
  const bool uok = uid >= 0 && uid < a.rows[6];
  bad |= !uok;
  for (int c = threadIdx.x; c < dm; c += kBlock) user_out[b * ld_user + c] = uok ? a.table[6][uid * dm + c] : 0.f;
  if (bad) atomicOr(status, REC_FLAG_INDEX_OOB);
}

struct BstSplit {
  float* g[6];
  int w[3];
};

// dX [B L, dm] -> the gradient rows of the six lookups: g[0..2] [B T, w], g[3..5] [B, w], contiguous
__global__ __launch_bounds__(kBlock) void bst_embed_bwd_kernel(int T, const float* __restrict__ dX, int64_t lddx, BstSplit a) {
  const int64_t b = blockIdx.x;
  const int L = T + 1, dm = a.w[0] + a.w[1] + a.w[2];
  for (int e = threadIdx.x; e < L * dm; e += kBlock) {
    const int l = e / dm, c = e - l * dm;
    const int seg = c < a.w[0] ? 0 : (c < a.w[0] + a.w[1] ? 1 : 2);
    const int col = c - (seg == 0 ? 0 : (seg == 1 ? a.w[0] : a.w[0] + a.w[1]));
    const float g = dX[(b * L + l) * lddx + c];
    if (l < T)
      a.g[seg][(b * T + l) * a.w[seg] + col] = g;
    else
      a.g[seg + 3][b * a.w[seg] + col] = g;
  }
}

// y[b] = sum_l z[b P + l] (lane-strided, then the butterfly) + bias[0]; one wave per sample
__global__ __launch_bounds__(kBlock) void bst_possum_fwd_kernel(int64_t B, int P, const float* __restrict__ z,
                                                                const float* __restrict__ bias, float* __restrict__ y) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (b >= B) return;
  float s = 0.f;
  for (int l = lane; l < P; l += kWave) s += z[b * P + l];
  s = group_sum<kWave>(s);
  if (lane == 0) y[b] = s + bias[0];
}

// dz[b P + l] = dy[b];  block 0 also folds dbias = sum_b dy[b] (thread-strided, then the tree)
__global__ __launch_bounds__(kBlock) void bst_possum_bwd_kernel(int64_t B, int P, const float* __restrict__ dy,
                                                                float* __restrict__ dz, float* __restrict__ dbias) {
  __shared__ float red[kBlock];
  const int64_t total = B * P;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) dz[e] = dy[e / P];
  if (blockIdx.x != 0) return;
  float s = 0.f;
  for (int64_t b = threadIdx.x; b < B; b += kBlock) s += dy[b];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dbias[0] = red[0];
}

int mha_check(int64_t batch, int32_t L, int32_t n_head, int32_t d_k, int32_t d_v, const float* q, int64_t ldq, const float* k,
              int64_t ldk, const float* v, int64_t ldv, float scale, float p, uint64_t seed, uint64_t stream_id, MhaArgs* a,
              const char* what) {
  REC_REQUIRE(batch >= 0 && L >= 1 && n_head >= 1, REC_EINVAL, "%s: bad sizes (batch %lld, L %d, heads %d)", what,
              (long long)batch, L, n_head);
  REC_REQUIRE(L <= kMhaMaxL, REC_ESHAPE, "%s: L %d > %d", what, L, kMhaMaxL);
  REC_REQUIRE(d_k >= 4 && d_v >= 4 && d_k % 4 == 0 && d_v % 4 == 0 && d_k <= kMhaMaxD && d_v <= kMhaMaxD, REC_ESHAPE,
              "%s: d_k %d / d_v %d unsupported (need multiples of 4, <= %d)", what, d_k, d_v, kMhaMaxD);
  REC_REQUIRE(batch * n_head < (1ll << 31), REC_ESHAPE, "%s: batch * heads too large", what);
  REC_REQUIRE(p >= 0.f && p < 1.f && isfinite(scale), REC_EINVAL, "%s: p must be in [0, 1) and scale finite", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(q && k && v, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ldq >= (int64_t)n_head * d_k && ldk >= (int64_t)n_head * d_k && ldv >= (int64_t)n_head * d_v && ldq % 4 == 0 &&
                  ldk % 4 == 0 && ldv % 4 == 0,
              REC_EINVAL, "%s: the row strides of q, k, v must be multiples of 4, >= heads * width", what);
  REC_REQUIRE(((uintptr_t)q) % 16 == 0 && ((uintptr_t)k) % 16 == 0 && ((uintptr_t)v) % 16 == 0, REC_EINVAL,
              "%s: q, k, v must be 16-byte aligned", what);
  a->L = L;
  a->H = n_head;
  a->dk4 = d_k / 4;
  a->dv4 = d_v / 4;
  a->q = q;
  a->k = k;
  a->v = v;
  a->ldq = ldq;
  a->ldk = ldk;
  a->ldv = ldv;
  a->scale = scale;
  a->drop = p > 0.f;                                        // p = 0: no hashing at all
  a->inv_keep = 1.f / (1.f - p);
  a->thresh = (uint32_t)((double)p * 4294967296.0);
  a->key = mix64(seed ^ mix64(stream_id + 0x9E3779B97F4A7C15ull));
  return REC_OK;
}

bool mha_mat_ok(const float* p, int64_t ld, int64_t cols) { return p && ld >= cols && ld % 4 == 0 && ((uintptr_t)p) % 16 == 0; }

int64_t stream_grid(int64_t total) {
  int64_t grid = (total + kBlock - 1) / kBlock;
  if (grid > kNumCU * 16) grid = kNumCU * 16;
  return grid < 1 ? 1 : grid;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_mha_fwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t d_k, int32_t d_v, const float* q,
                           int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float scale, float p,
                           uint64_t seed, uint64_t stream_id, float* out, int64_t ldo, float* lse, void* stream) {
  MhaArgs a;
  int rc = mha_check(batch, seq_len, n_head, d_k, d_v, q, ldq, k, ldk, v, ldv, scale, p, seed, stream_id, &a, "rec_mha_fwd");
  if (rc != REC_OK) return rc;
  if (batch == 0) return REC_OK;
  REC_REQUIRE(lse && mha_mat_ok(out, ldo, (int64_t)n_head * d_v), REC_EINVAL,
              "rec_mha_fwd: out must be 16-byte aligned with a row stride that is a multiple of 4, >= heads * d_v");
  REC_REQUIRE(out != q && out != k && out != v, REC_EINVAL, "rec_mha_fwd: out aliases no input");
  const dim3 grid((unsigned)(batch * n_head), (unsigned)((seq_len + kMhaTile - 1) / kMhaTile));
  hipLaunchKernelGGL(mha_fwd_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, a, out, ldo, lse);
  return check_launch("rec_mha_fwd");
}

extern "C" int rec_mha_bwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t d_k, int32_t d_v, const float* q,
                           int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float scale, float p,
                           uint64_t seed, uint64_t stream_id, const float* out, int64_t ldo, const float* d_out,
                           int64_t ld_dout, const float* lse, float* delta, float* dq, int64_t lddq, float* dk, int64_t lddk,
                           float* dv, int64_t lddv, void* stream) {
  MhaArgs a;
  int rc = mha_check(batch, seq_len, n_head, d_k, d_v, q, ldq, k, ldk, v, ldv, scale, p, seed, stream_id, &a, "rec_mha_bwd");
  if (rc != REC_OK) return rc;
  if (batch == 0) return REC_OK;
  const int64_t wk = (int64_t)n_head * d_k, wv = (int64_t)n_head * d_v;
  REC_REQUIRE(lse && delta, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(mha_mat_ok(out, ldo, wv) && mha_mat_ok(d_out, ld_dout, wv) && mha_mat_ok(dq, lddq, wk) &&
                  mha_mat_ok(dk, lddk, wk) && mha_mat_ok(dv, lddv, wv),
              REC_EINVAL, "rec_mha_bwd: every matrix must be 16-byte aligned with a row stride that is a multiple of 4, >= its width");
  for (const float* g : {(const float*)dq, (const float*)dk, (const float*)dv})
    REC_REQUIRE(g != q && g != k && g != v && g != out && g != d_out, REC_EINVAL, "rec_mha_bwd: the gradients alias no input");
  REC_REQUIRE(dq != dk && dq != dv && dk != dv && delta != lse, REC_EINVAL, "rec_mha_bwd: the gradients alias each other");
  const dim3 grid((unsigned)(batch * n_head), (unsigned)((seq_len + kMhaTile - 1) / kMhaTile));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mha_dq_kernel, grid, dim3(kBlock), 0, st, a, d_out, ld_dout, lse, delta, dq, lddq);
  rc = check_launch("rec_mha_bwd (dQ)");
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(mha_dkv_kernel, grid, dim3(kBlock), 0, st, a, d_out, ld_dout, lse, (const float*)delta, dk, lddk, dv,
                     lddv);
  return check_launch("rec_mha_bwd (dK, dV)");
}

extern "C" int rec_add_layer_norm_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, const float* r, int64_t ldr, float eps,
                                      float* y, int64_t ldy, int64_t y_group, int64_t ldy_group, float* mean, float* rstd,
                                      void* stream) {
  REC_REQUIRE(m >= 0 && n > 0 && eps >= 0.f, REC_EINVAL, "rec_add_layer_norm_fwd: bad sizes (m %lld, n %d)", (long long)m, n);
  if (m == 0) return REC_OK;
  REC_REQUIRE(x && y && mean && rstd, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ldx >= n && ldy >= n && (r == nullptr || ldr >= n), REC_EINVAL, "rec_add_layer_norm_fwd: a row stride is smaller than n");
  REC_REQUIRE(y_group >= 0 && (y_group == 0 || ldy_group >= y_group * ldy), REC_EINVAL,
              "rec_add_layer_norm_fwd: ldy_group is smaller than a group of rows");
  const int64_t grid = (m + kLnRows - 1) / kLnRows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_add_layer_norm_fwd: too many rows");
  hipLaunchKernelGGL(add_ln_fwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, m, n, x, ldx, r, ldr, eps,
                     y, ldy, y_group, ldy_group, mean, rstd);
  return check_launch("rec_add_layer_norm_fwd");
}

extern "C" int rec_add_layer_norm_bwd(int64_t m, int32_t n, const float* y, int64_t ldy, int64_t y_group, int64_t ldy_group,
                                      const float* rstd, const float* dy, int64_t lddy, float* dx, int64_t lddx, void* stream) {
  REC_REQUIRE(m >= 0 && n > 0, REC_EINVAL, "rec_add_layer_norm_bwd: bad sizes (m %lld, n %d)", (long long)m, n);
  if (m == 0) return REC_OK;
  REC_REQUIRE(y && rstd && dy && dx, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(ldy >= n && lddy >= n && lddx >= n, REC_EINVAL, "rec_add_layer_norm_bwd: a row stride is smaller than n");
  REC_REQUIRE(y_group >= 0 && (y_group == 0 || ldy_group >= y_group * ldy), REC_EINVAL,
              "rec_add_layer_norm_bwd: ldy_group is smaller than a group of rows");
  REC_REQUIRE(dx != y, REC_EINVAL, "rec_add_layer_norm_bwd: dx must not be y");
  const int64_t grid = (m + kLnRows - 1) / kLnRows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_add_layer_norm_bwd: too many rows");
  hipLaunchKernelGGL(add_ln_bwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, m, n, y, ldy, y_group,
                     ldy_group, rstd, dy, lddy, dx, lddx);
  return check_launch("rec_add_layer_norm_bwd");
}

extern "C" int rec_leaky_relu_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, float slope, float* y, int64_t ldy,
                                  void* stream) {
  REC_REQUIRE(m >= 0 && n > 0 && slope >= 0.f, REC_EINVAL, "rec_leaky_relu_fwd: bad arguments");
  if (m == 0) return REC_OK;
  REC_REQUIRE(x && y && ldx >= n && ldy >= n, REC_EINVAL, "rec_leaky_relu_fwd: null pointer or a row stride smaller than n");
  hipLaunchKernelGGL(leaky_relu_fwd_kernel, dim3((unsigned)stream_grid(m * n)), dim3(kBlock), 0, (hipStream_t)stream, m, n, x,
                     ldx, slope, y, ldy);
  return check_launch("rec_leaky_relu_fwd");
}

extern "C" int rec_leaky_relu_bwd(int64_t m, int32_t n, const float* y, int64_t ldy, const float* dy, int64_t lddy, float slope,
                                  float* dx, int64_t lddx, void* stream) {
  REC_REQUIRE(m >= 0 && n > 0 && slope >= 0.f, REC_EINVAL, "rec_leaky_relu_bwd: bad arguments");
  if (m == 0) return REC_OK;
  REC_REQUIRE(y && dy && dx && ldy >= n && lddy >= n && lddx >= n, REC_EINVAL,
              "rec_leaky_relu_bwd: null pointer or a row stride smaller than n");
  REC_REQUIRE(dx != y, REC_EINVAL, "rec_leaky_relu_bwd: dx must not be y");
  hipLaunchKernelGGL(leaky_relu_bwd_kernel, dim3((unsigned)stream_grid(m * n)), dim3(kBlock), 0, (hipStream_t)stream, m, n, y,
                     ldy, dy, lddy, slope, dx, lddx);
  return check_launch("rec_leaky_relu_bwd");
}

extern "C" int rec_bst_add(int64_t m, int64_t n, const float* x, int64_t ldx, const float* r, int64_t ldr, float* y, int64_t ldy,
                           void* stream) {
  REC_REQUIRE(m >= 0 && n > 0, REC_EINVAL, "rec_bst_add: bad sizes");
  if (m == 0) return REC_OK;
  REC_REQUIRE(x && y && ldx >= n && ldy >= n && (r == nullptr || ldr >= n), REC_EINVAL,
              "rec_bst_add: null pointer or a row stride smaller than n");
  hipLaunchKernelGGL(bst_add_kernel, dim3((unsigned)stream_grid(m * n)), dim3(kBlock), 0, (hipStream_t)stream, m, n, x, ldx, r,
                     ldr, y, ldy);
  return check_launch("rec_bst_add");
}

extern "C" int rec_bst_embed_fwd(int64_t batch, int32_t steps, const int64_t* const* ids, const int64_t* id_ld,
                                 const float* const* tables, const int64_t* table_rows, const int32_t* widths, float* X,
                                 int64_t ldx, float* user_out, int64_t ld_user, int32_t* status, void* stream) {
  REC_REQUIRE(batch >= 0 && steps >= 1 && ids && id_ld && tables && table_rows && widths, REC_EINVAL,
              "rec_bst_embed_fwd: bad arguments");
  REC_REQUIRE(widths[0] > 0 && widths[1] > 0 && widths[2] > 0, REC_EINVAL, "rec_bst_embed_fwd: widths must be positive");
  const int64_t dm = (int64_t)widths[0] + widths[1] + widths[2];
  REC_REQUIRE(batch < (1ll << 31) && (int64_t)(steps + 1) * dm < (1ll << 31), REC_ESHAPE, "rec_bst_embed_fwd: too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(X && user_out && status && ldx >= dm && ld_user >= dm, REC_EINVAL,
              "rec_bst_embed_fwd: null pointer or a row stride smaller than d_model");
  BstEmbed a;
  for (int t = 0; t < 7; ++t) {
    REC_REQUIRE(ids[t] && tables[t] && table_rows[t] > 0 && id_ld[t] >= (t < 3 ? steps : 1), REC_EINVAL,
                "rec_bst_embed_fwd: lookup %d: null pointer, empty table or an id stride smaller than its row", t);
    a.ids[t] = ids[t];
    a.ld[t] = id_ld[t];
    a.table[t] = tables[t];
    a.rows[t] = table_rows[t];
  }
  for (int s = 0; s < 3; ++s) a.w[s] = widths[s];
  hipLaunchKernelGGL(bst_embed_fwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps, a, X, ldx,
                     user_out, ld_user, status);
  return check_launch("rec_bst_embed_fwd");
}

extern "C" int rec_bst_embed_bwd(int64_t batch, int32_t steps, const int32_t* widths, const float* dX, int64_t lddx,
                                 float* const* grads, void* stream) {
  REC_REQUIRE(batch >= 0 && steps >= 1 && widths && grads, REC_EINVAL, "rec_bst_embed_bwd: bad arguments");
  REC_REQUIRE(widths[0] > 0 && widths[1] > 0 && widths[2] > 0, REC_EINVAL, "rec_bst_embed_bwd: widths must be positive");
  const int64_t dm = (int64_t)widths[0] + widths[1] + widths[2];
  REC_REQUIRE(batch < (1ll << 31) && (int64_t)(steps + 1) * dm < (1ll << 31), REC_ESHAPE, "rec_bst_embed_bwd: too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(dX && lddx >= dm, REC_EINVAL, "rec_bst_embed_bwd: null pointer or a row stride smaller than d_model");
  BstSplit a;
  for (int t = 0; t < 6; ++t) {
    REC_REQUIRE(grads[t] && grads[t] != dX, REC_EINVAL, "rec_bst_embed_bwd: gradient buffer %d is null or dX", t);
    a.g[t] = grads[t];
  }
  for (int s = 0; s < 3; ++s) a.w[s] = widths[s];
  hipLaunchKernelGGL(bst_embed_bwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps, dX, lddx, a);
  return check_launch("rec_bst_embed_bwd");
}

extern "C" int rec_bst_possum_fwd(int64_t batch, int32_t positions, const float* z, const float* bias, float* y, void* stream) {
  REC_REQUIRE(batch >= 0 && positions >= 1, REC_EINVAL, "rec_bst_possum_fwd: bad sizes");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(z && bias && y, REC_EINVAL, "null pointer argument");
  const int64_t grid = (batch + kBlock / kWave - 1) / (kBlock / kWave);
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_bst_possum_fwd: batch too large");
  hipLaunchKernelGGL(bst_possum_fwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, positions, z,
                     bias, y);
  return check_launch("rec_bst_possum_fwd");
}

extern "C" int rec_bst_possum_bwd(int64_t batch, int32_t positions, const float* dy, float* dz, float* dbias, void* stream) {
  REC_REQUIRE(batch >= 0 && positions >= 1 && dbias, REC_EINVAL, "rec_bst_possum_bwd: bad arguments");
  REC_REQUIRE(batch == 0 || (dy && dz && dz != dy), REC_EINVAL, "rec_bst_possum_bwd: null pointer, or dz is dy");
  hipLaunchKernelGGL(bst_possum_bwd_kernel, dim3((unsigned)stream_grid(batch * positions)), dim3(kBlock), 0,
                     (hipStream_t)stream, batch, positions, dy, dz, dbias);
  return check_launch("rec_bst_possum_bwd");
}
