// DSSM (models/match/dssm): two towers over bags of letter trigrams, a cosine head.  A tower input is a float vector of 2 900
// entries of which a dozen are set, so the first Linear — 87 % of a tower's multiply-adds when run dense — is a short list of
// weight rows to add up, and its weight gradient is nonzero only in the rows the batch touched:
//
//   dssm_lod_rows_kernel     row_of[j] = the row of CSR entry j (what the backward reads)
//   dssm_sparse_fwd_kernel   Y[r, :] = act(bias + sum_j vals[j] W[cols[j], :]); a thread owns VEC columns of one row and walks
//                            the row's entries in stored order
//   dssm_sparse_bwd_kernel   dW[c, :] for EVERY column c, one block per column: the block finds c among the grouped columns
//                            (binary search of uniq_rows), wave w sums the w-th part of the column's entries in ascending
//                            order, the parts meet in LDS and are folded in ascending w; a column nobody holds gets zeros
//   dssm_head_kernel         one wave per sample: the 1 + neg cosines (lane k keeps those of document k), the softmax over
//                            the lanes, -log of the positive's share, and dq / dd by the two-branch cosine gradient
//   dssm_loss_fold_kernel    the mean of the first M loss terms, one wave, fixed order
//   dssm_cos_kernel          the positive cosine alone (inference)
//
// No float atomics: the only atomic is the OR into the integer status word.  No per-lane arrays, no scratch.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr float kCosEps = 1e-8f;                              // Paddle's cosine_similarity epsilon
constexpr int kBwdWaves = REC_DSSM_BWD_WAVES;
constexpr int kBwdBlock = kBwdWaves * kWave;

__device__ __forceinline__ float wave_sum(float x) { return group_sum<kWave>(x); }

// x held to [lo, hi]
__device__ __forceinline__ int64_t clamp_i64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, kWave));
  return x;
}

__global__ __launch_bounds__(kBlock) void dssm_lod_rows_kernel(int64_t rows, int64_t nnz, const int64_t* __restrict__ lod,
                                                               int32_t* __restrict__ row_of) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;
  const int64_t beg = clamp_i64(lod[r], 0, nnz), end = clamp_i64(lod[r + 1], beg, nnz);
  for (int64_t j = beg; j < end; ++j) row_of[j] = (int32_t)r;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void dssm_sparse_fwd_kernel(int64_t total, int chunks, int64_t nnz, int64_t in_dim, int n,
                                                                 int relu, const int64_t* __restrict__ cols,
                                                                 const float* __restrict__ vals, const int64_t* __restrict__ lod,
                                                                 const float* __restrict__ W, int64_t ldw,
                                                                 const float* __restrict__ bias, float* __restrict__ Y,
                                                                 int64_t ldy, int32_t* status) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / chunks;
  const int c0 = (int)(e - r * chunks) * VEC;                 // c0 + VEC <= n: VEC 4 runs only where n % 4 == 0
  const int64_t beg = clamp_i64(lod[r], 0, nnz), end = clamp_i64(lod[r + 1], beg, nnz);
  float acc[VEC], w[VEC];
  vload<VEC>(acc, bias + c0);
  bool oob = false;
  for (int64_t j = beg; j < end; ++j) {
    const int64_t c = cols[j];
    if (c < 0 || c >= in_dim) {
      oob = true;
      continue;
    }
    const float v = vals[j];
    vload<VEC>(w, W + c * ldw + c0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = fmaf(v, w[i], acc[i]);
  }
  if (oob && c0 == 0 && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
  if (relu) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = fmaxf(acc[i], 0.f);
  }
  vstore<VEC>(Y + r * ldy + c0, acc);
}

// One block per column c of dW.  part [kBwdWaves, n] in dynamic LDS.  8 waves per SIMD: the walk of a column is a chain of
// dependent loads, hidden by other waves and not by registers.
template <int VEC>
__global__ __launch_bounds__(kBwdBlock, 8) void dssm_sparse_bwd_kernel(int64_t rows, int64_t nnz, int64_t in_dim, int n,
                                                                    const float* __restrict__ vals,
                                                                    const int32_t* __restrict__ row_of,
                                                                    const int32_t* __restrict__ sorted_pos,
                                                                    const int64_t* __restrict__ uniq_rows,
                                                                    const int32_t* __restrict__ seg_offset,
                                                                    const int32_t* __restrict__ n_uniq,
                                                                    const float* __restrict__ dY, int64_t lddy,
                                                                    float* __restrict__ dW, int64_t lddw) {
  extern __shared__ __attribute__((aligned(16))) float part[];
  const int64_t c = blockIdx.x;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  // the segment of column c: uniq_rows[0 .. U) is ascending
  const int64_t U = clamp_i64(n_uniq[0], 0, nnz < in_dim ? nnz : in_dim);
  int64_t lo = 0, hi = U;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (uniq_rows[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  int64_t beg = 0, end = 0;
  if (lo < U && uniq_rows[lo] == c) {
    beg = clamp_i64(seg_offset[lo], 0, nnz);
    end = clamp_i64(seg_offset[lo + 1], beg, nnz);
  }
  const int64_t len = end - beg, per = (len + kBwdWaves - 1) / kBwdWaves;
  const int64_t wbeg = clamp_i64(beg + wave * per, beg, end), wend = clamp_i64(wbeg + per, wbeg, end);
  const int chunks = n / VEC;
  for (int ch = lane; ch < chunks; ch += kWave) {
    const int c0 = ch * VEC;
    float acc[VEC], g[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    for (int64_t k = wbeg; k < wend; ++k) {
      const int64_t j = sorted_pos[k];
      if (j < 0 || j >= nnz) continue;
      const int64_t r = row_of[j];
      if (r < 0 || r >= rows) continue;
      const float v = vals[j];
      vload<VEC>(g, dY + r * lddy + c0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = fmaf(v, g[i], acc[i]);
    }
    vstore<VEC>(part + wave * n + c0, acc);
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < chunks; ch += kBwdBlock) {
    const int c0 = ch * VEC;
    float acc[VEC], p[VEC];
    vload<VEC>(acc, part + c0);
    for (int w = 1; w < kBwdWaves; ++w) {
      vload<VEC>(p, part + w * n + c0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] += p[i];
    }
    vstore<VEC>(dW + c * lddw + c0, acc);
  }
}

// cos = w12 / sqrt(max(w1 w2, eps^2)); `inv` = 1 / that root, `open` = the product is not clamped
__device__ __forceinline__ float dssm_cosine(float w12, float w1, float w2, float* inv, bool* open) {
  const float prod = w1 * w2;
  *open = prod >= kCosEps * kCosEps;
  *inv = *open ? 1.f / sqrtf(prod) : 1.f / kCosEps;
  return w12 * *inv;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void dssm_head_kernel(int64_t batch, int docs, int n, int64_t m_rows, int relu_mask,
                                                           const float* __restrict__ q, int64_t ldq,
                                                           const float* __restrict__ d, int64_t ldd, float* __restrict__ cosv,
                                                           float* __restrict__ hit_prob, float* __restrict__ loss_terms,
                                                           float* __restrict__ dq, int64_t lddq, float* __restrict__ dd,
                                                           int64_t lddd) {
  const int lane = threadIdx.x % kWave;
  const int64_t b = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (b >= batch) return;                                     // whole waves leave; nothing below synchronises a block
  const float* qb = q + b * ldq;
  float x[VEC], y[VEC];
  float w1 = 0.f;
  for (int c0 = lane * VEC; c0 < n; c0 += kWave * VEC) {
    vload<VEC>(x, qb + c0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) w1 = fmaf(x[i], x[i], w1);
  }
  w1 = wave_sum(w1);
  // lane k keeps document k's cosine, its squared norm, 1 / root and branch
  float my_cos = -INFINITY, my_w2 = 0.f, my_inv = 0.f;
  int my_open = 0;
  for (int k = 0; k < docs; ++k) {
    const float* dk = d + ((int64_t)k * batch + b) * ldd;
    float w12 = 0.f, w2 = 0.f;
    for (int c0 = lane * VEC; c0 < n; c0 += kWave * VEC) {
      vload<VEC>(x, qb + c0);
      vload<VEC>(y, dk + c0);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        w12 = fmaf(x[i], y[i], w12);
        w2 = fmaf(y[i], y[i], w2);
      }
    }
    w12 = wave_sum(w12);
    w2 = wave_sum(w2);
    float inv;
    bool open;
    const float cs = dssm_cosine(w12, w1, w2, &inv, &open);
    if (lane == k) {
      my_cos = cs;
      my_w2 = w2;
      my_inv = inv;
      my_open = open;
    }
  }
  const float mx = wave_max(my_cos);
  const float ex = lane < docs ? expf(my_cos - mx) : 0.f;
  const float prob = ex / wave_sum(ex);
  if (lane < docs) cosv[b * docs + lane] = my_cos;
  if (lane == 0) {
    hit_prob[b] = prob;
    loss_terms[b] = -logf(prob);
  }
  // d loss / d cos_k = (prob_k - [k == 0]) / M for the first M rows, 0 beyond
  const float my_g = b < m_rows && lane < docs ? (prob - (lane == 0 ? 1.f : 0.f)) / (float)m_rows : 0.f;
  float* dqb = dq + b * lddq;
  for (int c0 = lane * VEC; c0 < n; c0 += kWave * VEC) {
    vload<VEC>(x, qb + c0);
    float aq[VEC], ad[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) aq[i] = 0.f;
    for (int k = 0; k < docs; ++k) {
      const float g = __shfl(my_g, k, kWave), cs = __shfl(my_cos, k, kWave), w2 = __shfl(my_w2, k, kWave),
                  inv = __shfl(my_inv, k, kWave);
      const int open = __shfl(my_open, k, kWave);
      const int64_t row = (int64_t)k * batch + b;
      vload<VEC>(y, d + row * ldd + c0);
      // open: d cos / dx = y / root - cos x / w1 (w1, w2 > 0 there); clamped: y / eps
      const float sq = open ? cs / w1 : 0.f, sd = open ? cs / w2 : 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        aq[i] += g * (y[i] * inv - sq * x[i]);
        ad[i] = g * (x[i] * inv - sd * y[i]);
        if (relu_mask && !(y[i] > 0.f)) ad[i] = 0.f;
      }
      vstore<VEC>(dd + row * lddd + c0, ad);
    }
    if (relu_mask) {
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        if (!(x[i] > 0.f)) aq[i] = 0.f;
    }
    vstore<VEC>(dqb + c0, aq);
  }
}

__global__ __launch_bounds__(kWave) void dssm_loss_fold_kernel(int64_t m_rows, const float* __restrict__ loss_terms,
                                                               float* __restrict__ loss) {
  float s = 0.f;
  for (int64_t b = threadIdx.x; b < m_rows; b += kWave) s += loss_terms[b];
  s = wave_sum(s);
  if (threadIdx.x == 0) loss[0] = s / (float)m_rows;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void dssm_cos_kernel(int64_t batch, int n, const float* __restrict__ q, int64_t ldq,
                                                          const float* __restrict__ d, int64_t ldd, float* __restrict__ cosv) {
  const int lane = threadIdx.x % kWave;
  const int64_t b = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (b >= batch) return;
  float x[VEC], y[VEC];
  float w1 = 0.f, w2 = 0.f, w12 = 0.f;
  for (int c0 = lane * VEC; c0 < n; c0 += kWave * VEC) {
    vload<VEC>(x, q + b * ldq + c0);
    vload<VEC>(y, d + b * ldd + c0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      w1 = fmaf(x[i], x[i], w1);
      w12 = fmaf(x[i], y[i], w12);
      w2 = fmaf(y[i], y[i], w2);
    }
  }
  w1 = wave_sum(w1);
  w12 = wave_sum(w12);
  w2 = wave_sum(w2);
  float inv;
  bool open;
  const float cs = dssm_cosine(w12, w1, w2, &inv, &open);
  if (lane == 0) cosv[b] = cs;
}

// float4 lanes: the width and every row stride a multiple of 4 floats, every base 16-byte aligned
inline bool vec4_ok(int n, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
  if (n % 4) return false;
  for (int64_t ld : lds)
    if (ld % 4) return false;
  for (const void* p : ptrs)
    if ((uintptr_t)p % 16) return false;
  return true;
}

}  // namespace
}  // namespace rec

using namespace rec;

#define DSSM_CSR_SIZES()                                                                                              \
  REC_REQUIRE(rows >= 0 && rows < (1ll << 31), REC_EINVAL, "%s: rows %lld outside 0..2^31", what, (long long)rows);   \
  REC_REQUIRE(nnz >= 0 && nnz < (1ll << 31), REC_EINVAL, "%s: nnz %lld outside 0..2^31", what, (long long)nnz);

extern "C" int rec_dssm_lod_rows(int64_t rows, int64_t nnz, const int64_t* lod, int32_t* row_of, void* stream) {
  const char* what = "rec_dssm_lod_rows";
  DSSM_CSR_SIZES();
  if (rows == 0 || nnz == 0) return REC_OK;
  REC_REQUIRE(lod && row_of, REC_EINVAL, "%s: lod / row_of is null", what);
  REC_REQUIRE((const void*)lod != (const void*)row_of, REC_EINVAL, "%s: row_of aliases lod", what);
  hipLaunchKernelGGL(dssm_lod_rows_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     rows, nnz, lod, row_of);
  return check_launch(what);
}

extern "C" int rec_dssm_sparse_linear_fwd(int64_t rows, int64_t nnz, int64_t in_dim, int32_t n, int32_t relu, const int64_t* cols,
                                          const float* vals, const int64_t* lod, const float* W, int64_t ld_w, const float* bias,
                                          float* Y, int64_t ld_y, int32_t* status, void* stream) {
  const char* what = "rec_dssm_sparse_linear_fwd";
  DSSM_CSR_SIZES();
  REC_REQUIRE(in_dim >= 1, REC_EINVAL, "%s: in_dim %lld is not positive", what, (long long)in_dim);
  REC_REQUIRE(n >= 1 && n <= REC_DSSM_MAX_WIDTH, REC_EINVAL, "%s: n %d outside 1..REC_DSSM_MAX_WIDTH %d", what, n,
              REC_DSSM_MAX_WIDTH);
  REC_REQUIRE(ld_w >= n && ld_y >= n, REC_EINVAL, "%s: ld_w / ld_y smaller than n (%d)", what, n);
  if (rows == 0) return REC_OK;
  REC_REQUIRE(lod && W && bias && Y, REC_EINVAL, "%s: lod / W / bias / Y is null", what);
  REC_REQUIRE(nnz == 0 || (cols && vals), REC_EINVAL, "%s: cols / vals is null", what);
  REC_REQUIRE(Y != W && Y != bias && Y != vals, REC_EINVAL, "%s: Y aliases an input", what);
  const bool v4 = vec4_ok(n, {ld_w, ld_y}, {W, bias, Y});
  const int chunks = v4 ? n / 4 : n;
  const int64_t total = rows * chunks, blocks = (total + kBlock - 1) / kBlock;
  REC_REQUIRE(blocks < (1ll << 31), REC_EINVAL, "%s: rows * n too large for one launch", what);
  hipStream_t st = (hipStream_t)stream;
  if (v4)
    hipLaunchKernelGGL(dssm_sparse_fwd_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, st, total, chunks, nnz, in_dim, n, relu,
                       cols, vals, lod, W, ld_w, bias, Y, ld_y, status);
  else
    hipLaunchKernelGGL(dssm_sparse_fwd_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, total, chunks, nnz, in_dim, n, relu,
                       cols, vals, lod, W, ld_w, bias, Y, ld_y, status);
  return check_launch(what);
}

extern "C" int rec_dssm_sparse_linear_bwd(int64_t rows, int64_t nnz, int64_t in_dim, int32_t n, const float* vals,
                                          const int32_t* row_of, const int32_t* sorted_pos, const int64_t* uniq_rows,
                                          const int32_t* seg_offset, const int32_t* n_uniq, const float* dY, int64_t ld_dy,
                                          float* dW, int64_t ld_dw, void* stream) {
  const char* what = "rec_dssm_sparse_linear_bwd";
  DSSM_CSR_SIZES();
  REC_REQUIRE(in_dim >= 1 && in_dim < (1ll << 31), REC_EINVAL, "%s: in_dim %lld outside 1..2^31", what, (long long)in_dim);
  REC_REQUIRE(n >= 1 && n <= REC_DSSM_MAX_WIDTH, REC_EINVAL, "%s: n %d outside 1..REC_DSSM_MAX_WIDTH %d", what, n,
              REC_DSSM_MAX_WIDTH);
  REC_REQUIRE(ld_dy >= n && ld_dw >= n, REC_EINVAL, "%s: ld_dy / ld_dw smaller than n (%d)", what, n);
  REC_REQUIRE(dW != nullptr, REC_EINVAL, "%s: dW is null", what);
  REC_REQUIRE(sorted_pos && uniq_rows && seg_offset && n_uniq, REC_EINVAL,
              "%s: sorted_pos / uniq_rows / seg_offset / n_uniq is null", what);
  REC_REQUIRE(nnz == 0 || rows == 0 || (vals && row_of && dY), REC_EINVAL, "%s: vals / row_of / dY is null", what);
  REC_REQUIRE(dW != dY && dW != vals, REC_EINVAL, "%s: dW aliases an input", what);
  const bool v4 = vec4_ok(n, {ld_dy, ld_dw}, {dY, dW});
  const size_t lds = (size_t)kBwdWaves * n * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (v4)
    hipLaunchKernelGGL(dssm_sparse_bwd_kernel<4>, dim3((unsigned)in_dim), dim3(kBwdBlock), lds, st, rows, nnz, in_dim, n, vals,
                       row_of, sorted_pos, uniq_rows, seg_offset, n_uniq, dY, ld_dy, dW, ld_dw);
  else
    hipLaunchKernelGGL(dssm_sparse_bwd_kernel<1>, dim3((unsigned)in_dim), dim3(kBwdBlock), lds, st, rows, nnz, in_dim, n, vals,
                       row_of, sorted_pos, uniq_rows, seg_offset, n_uniq, dY, ld_dy, dW, ld_dw);
  return check_launch(what);
}

extern "C" int rec_dssm_head_step(int64_t batch, int32_t neg, int32_t n, int64_t slice_end, int32_t relu_mask, const float* q,
                                  int64_t ld_q, const float* d, int64_t ld_d, float* cosv, float* hit_prob, float* loss_terms,
                                  float* loss, float* dq, int64_t ld_dq, float* dd, int64_t ld_dd, void* stream) {
  const char* what = "rec_dssm_head_step";
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31) / REC_DSSM_MAX_DOCS, REC_EINVAL, "%s: batch %lld outside 0..2^25", what,
              (long long)batch);
  REC_REQUIRE(neg >= 0 && neg < REC_DSSM_MAX_DOCS, REC_EINVAL, "%s: neg %d outside 0..REC_DSSM_MAX_DOCS - 1 (%d)", what, neg,
              REC_DSSM_MAX_DOCS - 1);
  REC_REQUIRE(n >= 1, REC_EINVAL, "%s: n %d is not positive", what, n);
  REC_REQUIRE(slice_end >= 1, REC_EINVAL, "%s: slice_end %lld is not positive", what, (long long)slice_end);
  REC_REQUIRE(ld_q >= n && ld_d >= n && ld_dq >= n && ld_dd >= n, REC_EINVAL, "%s: ld_q / ld_d / ld_dq / ld_dd smaller than n (%d)",
              what, n);
  REC_REQUIRE(loss != nullptr, REC_EINVAL, "%s: loss is null", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(q && d, REC_EINVAL, "%s: q / d is null", what);
  REC_REQUIRE(cosv && hit_prob && loss_terms && dq && dd, REC_EINVAL, "%s: cos / hit_prob / loss_terms / dq / dd is null", what);
  for (const float* o : {(const float*)cosv, (const float*)hit_prob, (const float*)loss_terms, (const float*)loss,
                         (const float*)dq, (const float*)dd})
    REC_REQUIRE(o != q && o != d, REC_EINVAL, "%s: an output aliases an input", what);
  REC_REQUIRE(dq != dd, REC_EINVAL, "%s: dq and dd are the same", what);
  const int64_t m_rows = slice_end < batch ? slice_end : batch;
  const int64_t blocks = (batch + kBlock / kWave - 1) / (kBlock / kWave);
  hipStream_t st = (hipStream_t)stream;
  if (vec4_ok(n, {ld_q, ld_d, ld_dq, ld_dd}, {q, d, dq, dd}))
    hipLaunchKernelGGL(dssm_head_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, st, batch, neg + 1, n, m_rows, relu_mask, q,
                       ld_q, d, ld_d, cosv, hit_prob, loss_terms, dq, ld_dq, dd, ld_dd);
  else
    hipLaunchKernelGGL(dssm_head_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, batch, neg + 1, n, m_rows, relu_mask, q,
                       ld_q, d, ld_d, cosv, hit_prob, loss_terms, dq, ld_dq, dd, ld_dd);
  int rc = check_launch(what);
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(dssm_loss_fold_kernel, dim3(1), dim3(kWave), 0, st, m_rows, (const float*)loss_terms, loss);
  return check_launch("rec_dssm_head_step (fold)");
}

extern "C" int rec_dssm_cos(int64_t batch, int32_t n, const float* q, int64_t ld_q, const float* d, int64_t ld_d, float* cosv,
                            void* stream) {
  const char* what = "rec_dssm_cos";
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31), REC_EINVAL, "%s: batch %lld outside 0..2^31", what, (long long)batch);
  REC_REQUIRE(n >= 1, REC_EINVAL, "%s: n %d is not positive", what, n);
  REC_REQUIRE(ld_q >= n && ld_d >= n, REC_EINVAL, "%s: ld_q / ld_d smaller than n (%d)", what, n);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(q && d && cosv, REC_EINVAL, "%s: q / d / cos is null", what);
  REC_REQUIRE(cosv != q && cosv != d, REC_EINVAL, "%s: cos aliases an input", what);
  const int64_t blocks = (batch + kBlock / kWave - 1) / (kBlock / kWave);
  if (vec4_ok(n, {ld_q, ld_d}, {q, d}))
    hipLaunchKernelGGL(dssm_cos_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, batch, n, q, ld_q, d, ld_d,
                       cosv);
  else
    hipLaunchKernelGGL(dssm_cos_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, batch, n, q, ld_q, d, ld_d,
                       cosv);
  return check_launch(what);
}
