// AITM (models/multitask/aitm) on gfx950: the pieces its hot path lacks.
//
//   rec_field_gather_fwd    <- aitm/net.py:97-105: one nn.Embedding per field (tables of unequal size, no padding id) and the
//                              concat — out [B, F * D] from ONE table buffer and field_begin [F + 1]; an id is checked against
//                              ITS OWN field's row count, so it can never read (or, through rows_out, train) a neighbouring table
//   rec_ait_fwd / _bwd      <- aitm/net.py:53-60 Attention.forward: per-token self score <Q_t, K_t> / sqrt(d), softmax over the
//                              tokens, sum_t a_t V_t, and its backward to d(QKV)
//   rec_aitm_head           <- aitm/net.py:112-113 + dygraph_model.py:41-55: the two Linear(d, 1) + sigmoid, both
//                              binary_cross_entropy terms, the hinge max(pCVR - pCTR, 0) and d(logits) in one launch
//   rec_auc_histogram_wide  <- dygraph_model.py:71-73: paddle.metric.Auc(num_thresholds = 100000) — the bucket arithmetic of
//                              auc_hist_kernel (head_ops.hip) with the histograms in global memory
//
// Mapping.  Gather, AIT and head share one layout: a ROW GROUP of 2^k lanes (k from the host: the smallest power of two
// covering the row's VEC-wide column chunks, at most 64) owns one (sample, field) pair / one sample, and a 256-thread block
// holds 256 >> k of them; lane l owns the chunks l, l + 2^k, ...: a row is read as contiguous 16-byte pieces (VEC 4) or
// floats (VEC 1).  What every lane of a group needs of its row's scalars (the id, the field's bounds) it loads itself:
// one address per group, a broadcast.  A dot product is each lane's partial over its chunks in ascending order, then an
// xor butterfly over the group from offset 2^(k-1) down to 1: a fixed order, and every lane of the group ends with the
// same float.  The per-token values of the AIT block live in registers (loops over REC_AIT_MAX_TOKENS fully unrolled and
// guarded by t < tokens, never an array indexed by a runtime value).  No LDS, no workspace, no float atomics, one writer
// per output element: a rerun is bit-identical.  The gather's status word is ORed with a plain load and store (every
// writer stores the same bit).  The wide AUC histogram uses 64-bit INTEGER global atomics only: sums of integers are
// exact in any order.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kAitMaxTokens = REC_AIT_MAX_TOKENS;

__device__ __forceinline__ float lanes_sum(float x, const int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  return x;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void field_gather_fwd_kernel(const int64_t pairs, const int num_fields, const int D,
                                                                  const int64_t row_stride, const int lane_shift,
                                                                  const int64_t* field_begin, const int64_t* ids, const float* W,
                                                                  float* out, const int64_t ld_out, int64_t* rows_out,
                                                                  int32_t* status) {
  const int lanes = 1 << lane_shift;
  const int64_t pair = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (pair >= pairs) return;
  const int lane = threadIdx.x & (lanes - 1);
  const int64_t b = pair / num_fields;
  const int f = (int)(pair - b * num_fields);
  const int64_t begin = field_begin[f], id = ids[pair];
  const bool ok = id >= 0 && id < field_begin[f + 1] - begin;
  const int64_t row = ok ? begin + id : -1;
  float* o = out + b * ld_out + (int64_t)f * D;
  for (int c = lane * VEC; c < D; c += lanes * VEC) {
    float w[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) w[v] = 0.f;
    if (ok) vload<VEC>(w, W + row * row_stride + c);
    vstore<VEC>(o + c, w);
  }
  if (lane == 0) {
    if (rows_out != nullptr) rows_out[pair] = row;
    if (!ok && status != nullptr) *status = *status | REC_FLAG_INDEX_OOB;
  }
}

// one row group per sample; QKV rows b * T + t, columns Q | K | V
template <int VEC>
__global__ __launch_bounds__(kBlock) void ait_fwd_kernel(const int64_t batch, const int T, const int d, const int lane_shift,
                                                         const float scale, const float* QKV, const int64_t ld_qkv, float* out,
                                                         const int64_t ld_out, float* prob) {
  const int lanes = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const float* x = QKV + b * T * ld_qkv;
  float s[kAitMaxTokens];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < kAitMaxTokens; ++t) {
    s[t] = 0.f;
    if (t < T) {
      const float* r = x + t * ld_qkv;
      float acc = 0.f;
      for (int c = lane * VEC; c < d; c += lanes * VEC) {
        float q[VEC], k[VEC];
        vload<VEC>(q, r + c);
        vload<VEC>(k, r + d + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc += q[v] * k[v];
      }
      s[t] = lanes_sum(acc, lanes) * scale;
      m = fmaxf(m, s[t]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < kAitMaxTokens; ++t)
    if (t < T) {
      s[t] = expf(s[t] - m);
      sum += s[t];
    }
#pragma unroll
  for (int t = 0; t < kAitMaxTokens; ++t)
    if (t < T) {
      s[t] = s[t] / sum;
      if (lane == 0) prob[b * T + t] = s[t];
    }
  for (int c = lane * VEC; c < d; c += lanes * VEC) {
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
#pragma unroll
    for (int t = 0; t < kAitMaxTokens; ++t)
      if (t < T) {
        float vv[VEC];
        vload<VEC>(vv, x + t * ld_qkv + 2 * d + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += s[t] * vv[v];
      }
    vstore<VEC>(out + b * ld_out + c, acc);
  }
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void ait_bwd_kernel(const int64_t batch, const int T, const int d, const int lane_shift,
                                                         const float scale, const float* QKV, const int64_t ld_qkv,
                                                         const float* prob, const float* d_out, const int64_t ld_dout,
                                                         float* dQKV, const int64_t ld_dqkv) {
  const int lanes = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const float* x = QKV + b * T * ld_qkv;
  const float* g = d_out + b * ld_dout;
  float a[kAitMaxTokens], ds[kAitMaxTokens];
  float dot = 0.f;                                   // sum_u a_u da_u, u ascending
#pragma unroll
  for (int t = 0; t < kAitMaxTokens; ++t) {
    a[t] = ds[t] = 0.f;
    if (t < T) {
      float acc = 0.f;
      for (int c = lane * VEC; c < d; c += lanes * VEC) {
        float gg[VEC], vv[VEC];
        vload<VEC>(gg, g + c);
        vload<VEC>(vv, x + t * ld_qkv + 2 * d + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc += gg[v] * vv[v];
      }
      a[t] = prob[b * T + t];
      ds[t] = lanes_sum(acc, lanes);                 // da_t
      dot += a[t] * ds[t];
    }
  }
#pragma unroll
  for (int t = 0; t < kAitMaxTokens; ++t)
    if (t < T) {
      const float w = a[t] * (ds[t] - dot) * scale;  // ds_t / sqrt(d); one token: a = 1 and da - 1 * da = 0 exactly
      const float* r = x + t * ld_qkv;
      float* o = dQKV + (b * T + t) * ld_dqkv;
      for (int c = lane * VEC; c < d; c += lanes * VEC) {
        float q[VEC], k[VEC], gg[VEC], dq[VEC], dk[VEC], dv[VEC];
        vload<VEC>(q, r + c);
        vload<VEC>(k, r + d + c);
        vload<VEC>(gg, g + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          dq[v] = w * k[v];
          dk[v] = w * q[v];
          dv[v] = a[t] * gg[v];
        }
        vstore<VEC>(o + c, dq);
        vstore<VEC>(o + d + c, dk);
        vstore<VEC>(o + 2 * d + c, dv);
      }
    }
}

__device__ __forceinline__ float bce(const float p, const float y) {
  return -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(logf(1.f - p), -100.f));
}

// one row group per sample: both dots, then lane 0 finishes the sample
template <int VEC>
__global__ __launch_bounds__(kBlock) void aitm_head_kernel(const rec_aitm_head_desc d, const int lane_shift, const float* click_in,
                                                           const float* ait, const float* w_click, const float* b_click,
                                                           const float* w_conv, const float* b_conv, const int64_t* click,
                                                           const int64_t* buy, float* pred, float* cost, float* dz) {
  const int lanes = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= d.batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const float* xc = click_in + b * d.ld_click;
  const float* xa = ait + b * d.ld_ait;
  float acc0 = 0.f, acc1 = 0.f;
  for (int c = lane * VEC; c < d.dim; c += lanes * VEC) {
    float x0[VEC], w0[VEC], x1[VEC], w1[VEC];
    vload<VEC>(x0, xc + c);
    vload<VEC>(w0, w_click + c);
    vload<VEC>(x1, xa + c);
    vload<VEC>(w1, w_conv + c);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      acc0 += x0[v] * w0[v];
      acc1 += x1[v] * w1[v];
    }
  }
  acc0 = lanes_sum(acc0, lanes);
  acc1 = lanes_sum(acc1, lanes);
  if (lane != 0) return;
  const float p0 = 1.f / (1.f + expf(-(acc0 + b_click[0])));      // pCTR
  const float p1 = 1.f / (1.f + expf(-(acc1 + b_conv[0])));       // pCVR
  const float y = (float)click[b], t = (float)buy[b];
  pred[b * 2] = p0;
  pred[b * 2 + 1] = p1;
  const bool over = p1 > p0;                                        // strictly: a tie carries no hinge gradient
  cost[b * 3] = bce(p0, y);
  cost[b * 3 + 1] = bce(p1, t);
  cost[b * 3 + 2] = over ? p1 - p0 : 0.f;
  if (dz == nullptr) return;
  const float s0 = p0 * (1.f - p0), s1 = p1 * (1.f - p1);
  float g0 = d.grad_scale * ((p0 - y) / fmaxf(s0, 1e-12f));
  float g1 = d.grad_scale * ((p1 - t) / fmaxf(s1, 1e-12f));
  if (over) {                                                       // the hinge is a batch SUM: not scaled by grad_scale
    g0 -= d.constraint_w;
    g1 += d.constraint_w;
  }
  dz[b * 2] = g0 * s0;
  dz[b * 2 + 1] = g1 * s1;
}

__global__ __launch_bounds__(kBlock) void auc_hist_wide_kernel(const int64_t B, const float* pred, const int64_t ld_pred,
                                                               const int64_t* label, const int T, unsigned long long* pos,
                                                               unsigned long long* neg) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
    int bucket = (int)(pred[i * ld_pred] * (float)T);
    bucket = bucket < 0 ? 0 : (bucket > T ? T : bucket);
    atomicAdd((label[i] != 0 ? pos : neg) + bucket, 1ull);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// lanes of a row group, as a shift: the smallest power of two covering `chunks`, at most 64
inline int group_shift(const int chunks) {
  int shift = 0;
  while ((1 << shift) < chunks && shift < 6) ++shift;
  return shift;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_field_gather_fwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t row_stride,
                                    const int64_t* field_begin, const int64_t* ids, const float* W, float* out, int64_t ld_out,
                                    int64_t* rows_out, int32_t* status, void* stream) {
  REC_REQUIRE(batch >= 0 && num_fields >= 1, REC_EINVAL, "rec_field_gather_fwd: bad sizes (batch %lld, num_fields %d)",
              (long long)batch, num_fields);
  REC_REQUIRE(emb_dim >= 1 && emb_dim <= REC_FIELD_GATHER_MAX_DIM, REC_EINVAL, "rec_field_gather_fwd: bad emb_dim %d (1..%d)",
              emb_dim, REC_FIELD_GATHER_MAX_DIM);
  REC_REQUIRE(row_stride >= emb_dim, REC_EINVAL, "rec_field_gather_fwd: bad table (row_stride %d below emb_dim %d)", row_stride,
              emb_dim);
  const int64_t packed = (int64_t)num_fields * emb_dim;
  if (ld_out == 0) ld_out = packed;
  REC_REQUIRE(ld_out >= packed, REC_EINVAL, "rec_field_gather_fwd: bad ld_out %lld: below the packed width %lld",
              (long long)ld_out, (long long)packed);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(field_begin && ids && W && out, REC_EINVAL, "rec_field_gather_fwd: null pointer argument");
  const bool vec = emb_dim % 4 == 0 && row_stride % 4 == 0 && ld_out % 4 == 0 && aligned16(W) && aligned16(out);
  const int shift = group_shift(vec ? emb_dim / 4 : emb_dim);
  const int rows = kBlock >> shift;
  REC_REQUIRE(batch <= (1ll << 62) / num_fields, REC_ESHAPE, "rec_field_gather_fwd: too many lookups");
  const int64_t pairs = batch * num_fields;
  const int64_t grid = (pairs + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_field_gather_fwd: too many rows");
  if (vec)
    hipLaunchKernelGGL(field_gather_fwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, pairs,
                       (int)num_fields, (int)emb_dim, (int64_t)row_stride, shift, field_begin, ids, W, out, ld_out, rows_out,
                       status);
  else
    hipLaunchKernelGGL(field_gather_fwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, pairs,
                       (int)num_fields, (int)emb_dim, (int64_t)row_stride, shift, field_begin, ids, W, out, ld_out, rows_out,
                       status);
  return check_launch("rec_field_gather_fwd");
}

// the checks rec_ait_fwd and rec_ait_bwd share; -> 0 or the error
static int ait_check(const char* what, int64_t batch, int32_t tokens, int32_t dim, int64_t* ld_qkv) {
  REC_REQUIRE(batch >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)batch);
  REC_REQUIRE(tokens >= 1 && tokens <= REC_AIT_MAX_TOKENS, REC_EINVAL, "%s: bad tokens %d (1..%d)", what, tokens,
              REC_AIT_MAX_TOKENS);
  REC_REQUIRE(dim >= 1 && dim <= REC_AIT_MAX_DIM, REC_EINVAL, "%s: bad dim %d (1..%d)", what, dim, REC_AIT_MAX_DIM);
  if (*ld_qkv == 0) *ld_qkv = 3 * (int64_t)dim;
  REC_REQUIRE(*ld_qkv >= 3 * (int64_t)dim, REC_EINVAL, "%s: bad ld_qkv %lld: below the packed width %d", what,
              (long long)*ld_qkv, 3 * dim);
  REC_REQUIRE(batch <= (1ll << 40), REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

extern "C" int rec_ait_fwd(int64_t batch, int32_t tokens, int32_t dim, const float* QKV, int64_t ld_qkv, float* out,
                           int64_t ld_out, float* prob, void* stream) {
  if (int rc = ait_check("rec_ait_fwd", batch, tokens, dim, &ld_qkv)) return rc;
  if (ld_out == 0) ld_out = dim;
  REC_REQUIRE(ld_out >= dim, REC_EINVAL, "rec_ait_fwd: bad ld_out %lld: below the packed width %d", (long long)ld_out, dim);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(QKV && out && prob, REC_EINVAL, "rec_ait_fwd: null pointer argument");
  const bool vec = dim % 4 == 0 && ld_qkv % 4 == 0 && ld_out % 4 == 0 && aligned16(QKV) && aligned16(out);
  const int shift = group_shift(vec ? dim / 4 : dim);
  const int rows = kBlock >> shift;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_ait_fwd: too many rows");
  const float scale = 1.0f / sqrtf((float)dim);
  if (vec)
    hipLaunchKernelGGL(ait_fwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)tokens,
                       (int)dim, shift, scale, QKV, ld_qkv, out, ld_out, prob);
  else
    hipLaunchKernelGGL(ait_fwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)tokens,
                       (int)dim, shift, scale, QKV, ld_qkv, out, ld_out, prob);
  return check_launch("rec_ait_fwd");
}

extern "C" int rec_ait_bwd(int64_t batch, int32_t tokens, int32_t dim, const float* QKV, int64_t ld_qkv, const float* prob,
                           const float* d_out, int64_t ld_dout, float* dQKV, int64_t ld_dqkv, void* stream) {
  if (int rc = ait_check("rec_ait_bwd", batch, tokens, dim, &ld_qkv)) return rc;
  if (ld_dout == 0) ld_dout = dim;
  REC_REQUIRE(ld_dout >= dim, REC_EINVAL, "rec_ait_bwd: bad ld_dout %lld: below the packed width %d", (long long)ld_dout, dim);
  if (ld_dqkv == 0) ld_dqkv = 3 * (int64_t)dim;
  REC_REQUIRE(ld_dqkv >= 3 * (int64_t)dim, REC_EINVAL, "rec_ait_bwd: bad ld_dqkv %lld: below the packed width %d",
              (long long)ld_dqkv, 3 * dim);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(QKV && prob && d_out && dQKV, REC_EINVAL, "rec_ait_bwd: null pointer argument");
  const bool vec = dim % 4 == 0 && ld_qkv % 4 == 0 && ld_dout % 4 == 0 && ld_dqkv % 4 == 0 && aligned16(QKV) &&
                   aligned16(d_out) && aligned16(dQKV);
  const int shift = group_shift(vec ? dim / 4 : dim);
  const int rows = kBlock >> shift;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_ait_bwd: too many rows");
  const float scale = 1.0f / sqrtf((float)dim);
  if (vec)
    hipLaunchKernelGGL(ait_bwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)tokens,
                       (int)dim, shift, scale, QKV, ld_qkv, prob, d_out, ld_dout, dQKV, ld_dqkv);
  else
    hipLaunchKernelGGL(ait_bwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)tokens,
                       (int)dim, shift, scale, QKV, ld_qkv, prob, d_out, ld_dout, dQKV, ld_dqkv);
  return check_launch("rec_ait_bwd");
}

extern "C" int rec_aitm_head(const rec_aitm_head_desc* desc, const float* tower_click, const float* ait, const float* w_click,
                             const float* b_click, const float* w_conv, const float* b_conv, const int64_t* click,
                             const int64_t* buy, float* pred, float* cost, float* dz, void* stream) {
  REC_REQUIRE(desc != nullptr, REC_EINVAL, "rec_aitm_head: null descriptor");
  rec_aitm_head_desc d = *desc;
  REC_REQUIRE(d.batch >= 0, REC_EINVAL, "rec_aitm_head: bad batch %lld", (long long)d.batch);
  REC_REQUIRE(d.dim >= 1 && d.dim <= REC_AITM_HEAD_MAX_DIM, REC_EINVAL, "rec_aitm_head: bad dim %d (1..%d)", d.dim,
              REC_AITM_HEAD_MAX_DIM);
  if (d.ld_click == 0) d.ld_click = d.dim;
  if (d.ld_ait == 0) d.ld_ait = d.dim;
  REC_REQUIRE(d.ld_click >= d.dim && d.ld_ait >= d.dim, REC_EINVAL,
              "rec_aitm_head: bad ld_click %lld / ld_ait %lld: below the packed width %d", (long long)d.ld_click,
              (long long)d.ld_ait, d.dim);
  if (d.batch == 0) return REC_OK;
  REC_REQUIRE(tower_click && ait && w_click && b_click && w_conv && b_conv && click && buy && pred && cost, REC_EINVAL,
              "rec_aitm_head: null pointer argument");
  const bool vec = d.dim % 4 == 0 && d.ld_click % 4 == 0 && d.ld_ait % 4 == 0 && aligned16(tower_click) && aligned16(ait) &&
                   aligned16(w_click) && aligned16(w_conv);
  const int shift = group_shift(vec ? d.dim / 4 : d.dim);
  const int rows = kBlock >> shift;
  const int64_t grid = (d.batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_aitm_head: too many rows");
  if (vec)
    hipLaunchKernelGGL(aitm_head_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, d, shift, tower_click,
                       ait, w_click, b_click, w_conv, b_conv, click, buy, pred, cost, dz);
  else
    hipLaunchKernelGGL(aitm_head_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, d, shift, tower_click,
                       ait, w_click, b_click, w_conv, b_conv, click, buy, pred, cost, dz);
  return check_launch("rec_aitm_head");
}

extern "C" int rec_auc_histogram_wide(int64_t batch, const float* pred, int64_t ld_pred, const int64_t* label,
                                      int32_t num_thresholds, int64_t* stat_pos, int64_t* stat_neg, void* stream) {
  REC_REQUIRE(batch >= 0, REC_EINVAL, "rec_auc_histogram_wide: bad batch %lld", (long long)batch);
  REC_REQUIRE(num_thresholds >= 1 && num_thresholds <= REC_AUC_WIDE_MAX_THRESHOLDS, REC_EINVAL,
              "rec_auc_histogram_wide: bad num_thresholds %d (1..%d)", num_thresholds, REC_AUC_WIDE_MAX_THRESHOLDS);
  if (ld_pred == 0) ld_pred = 1;
  REC_REQUIRE(ld_pred >= 1, REC_EINVAL, "rec_auc_histogram_wide: bad ld_pred %lld: below the packed width 1", (long long)ld_pred);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(pred && label && stat_pos && stat_neg, REC_EINVAL, "rec_auc_histogram_wide: null pointer argument");
  int64_t grid = (batch + kBlock - 1) / kBlock;
  if (grid > kNumCU * 8) grid = kNumCU * 8;
  hipLaunchKernelGGL(auc_hist_wide_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, pred, ld_pred,
                     label, (int)num_thresholds, (unsigned long long*)stat_pos, (unsigned long long*)stat_neg);
  return check_launch("rec_auc_histogram_wide");
}
