// The entire-space multitask nets (models/multitask: ESMM, ESCM2) on gfx950: the two pieces their hot path lacks.
//
//   rec_field_sumpool_fwd  <- esmm/net.py:84-91, escm2/net.py:108-115: Embedding(padding_idx) on ids [B, F, L], sum over L per
//                             field, concat over the fields — out [B, F * D], written through a row stride so that it can
//                             be the feature buffer of the packed first GEMM
//   rec_esm_head           <- esmm/net.py:97-111 + dygraph_model.py:57-67, escm2/net.py:135-160 + dygraph_model.py:67-148: two
//                             or three two-class softmaxes (ESCM2: clipped), pCTCVR = pCTR pCVR, the log losses, the IPW /
//                             DR counterfactual CVR term (its propensity factor under stop-gradient) and d(logits)
//
// Mapping.  Pool: a ROW GROUP of 2^k lanes (k from the host: the smallest power of two covering D / VEC column chunks, at most
// 64) owns one (sample, field) pair and a 256-thread block holds 256 >> k pairs; lane l owns the VEC-wide chunks l, l + 2^k,
// ...; every lane of the group reads the pair's ids itself (one address per group: a broadcast) and adds its chunk of the
// rows in l order, starting from +0.  An id equal to padding_idx is skipped; an id outside [0, num_rows) is skipped too,
// its row is never addressed, and lane 0 of the group ORs REC_FLAG_INDEX_OOB into the status word with a plain load and
// store (every writer stores the same bit: the race has one outcome).  Head: one thread per sample, tens of bytes each.
// The click count of the IPW mode is one workgroup: thread t adds click[t], click[t + 256], ... in int64 (four partial
// sums, so four loads are in flight), a butterfly over the wave, the four wave sums through LDS — integer sums, exact in
// any order.  Nothing is atomic, no kernel takes a
// workspace, every output element has one writer: a rerun is bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

template <int VEC>
__global__ __launch_bounds__(kBlock) void field_sumpool_fwd_kernel(const int64_t pairs, const int num_fields, const int max_len,
                                                                   const int D, const int64_t row_stride, const int64_t num_rows,
                                                                   const int64_t padding_idx, const int lane_shift,
                                                                   const int64_t* ids, const float* W, float* out,
                                                                   const int64_t ld_out, int32_t* status) {
  const int lanes = 1 << lane_shift;
  const int64_t pair = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (pair >= pairs) return;
  const int lane = threadIdx.x & (lanes - 1);
  const int64_t b = pair / num_fields;
  const int f = (int)(pair - b * num_fields);
  const int64_t* id = ids + pair * max_len;
  float* o = out + b * ld_out + (int64_t)f * D;
  bool oob = false;
  for (int c = lane * VEC; c < D; c += lanes * VEC) {
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    for (int l = 0; l < max_len; ++l) {
      const int64_t r = id[l];
      if (r == padding_idx) continue;
      if (r < 0 || r >= num_rows) {
        oob = true;
        continue;
      }
      float w[VEC];
      vload<VEC>(w, W + r * row_stride + c);
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += w[v];
    }
    vstore<VEC>(o + c, acc);
  }
  if (lane == 0) {                       // c = 0 < D: lane 0 has walked the ids
    if (oob && status != nullptr) *status = *status | REC_FLAG_INDEX_OOB;
  }
}

// click_count[0] = sum of click[0 .. batch): ONE block
__global__ __launch_bounds__(kBlock) void esm_click_count_kernel(const int64_t batch, const int64_t* click, int64_t* click_count) {
  __shared__ int64_t part[kBlock / kWave];
  int64_t s = 0, s1 = 0, s2 = 0, s3 = 0;      // four loads in flight per thread: the fold is one block's latency chain
  int64_t i = threadIdx.x;
  for (; i + 3 * kBlock < batch; i += 4 * kBlock) {
    s += click[i];
    s1 += click[i + kBlock];
    s2 += click[i + 2 * kBlock];
    s3 += click[i + 3 * kBlock];
  }
  for (; i < batch; i += kBlock) s += click[i];
  s = (s + s1) + (s2 + s3);
  for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int w = 0; w < kBlock / kWave; ++w) t += part[w];
    click_count[0] = t;
  }
}

struct Soft2 {
  float p0, p1;      // the softmax
  float q0, q1;      // what the net returns: clipped (ESCM2) or p itself (ESMM)
  bool open;         // the clip passes the gradient of column 1
};

__device__ __forceinline__ Soft2 soft2(const float x0, const float x1, const bool clip) {
  const float lo = 1e-15f, hi = 1.0f - 1e-15f;     // paddle.clip's bounds as a float32 tensor sees them (hi is 1)
  const float m = fmaxf(x0, x1);
  const float e0 = expf(x0 - m), e1 = expf(x1 - m);
  const float s = e0 + e1;
  Soft2 r;
  r.p0 = e0 / s;
  r.p1 = e1 / s;
  r.q0 = clip ? fminf(fmaxf(r.p0, lo), hi) : r.p0;
  r.q1 = clip ? fminf(fmaxf(r.p1, lo), hi) : r.p1;
  r.open = !clip || (r.p1 >= lo && r.p1 <= hi);
  return r;
}

__device__ __forceinline__ float log_loss(const float x, const float lab) {
  const float eps = 1e-4f;
  return -lab * logf(x + eps) - (1.f - lab) * logf(1.f - x + eps);
}

__device__ __forceinline__ float d_log_loss(const float x, const float lab) {
  const float eps = 1e-4f;
  return (1.f - lab) / (1.f - x + eps) - lab / (x + eps);
}

// one thread per sample
__global__ __launch_bounds__(kBlock) void esm_head_kernel(const rec_esm_head_desc d, const float* logits, const int64_t* click,
                                                          const int64_t* buy, const int64_t* click_count, float* pred,
                                                          float* cost, float* dlogits) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= d.batch) return;
  const int mode = d.mode;
  const int G = mode == REC_ESM_DR ? 3 : 2;
  const bool clip = mode != REC_ESM_ESMM;
  const float* x = logits + b * d.ld_logit;
  const Soft2 ctr = soft2(x[0], x[1], clip), cvr = soft2(x[2], x[3], clip);
  const float y = (float)click[b], t = (float)buy[b], o = y;
  const float p1 = ctr.q1, q1 = cvr.q1;
  const float r = p1 * q1;
  float* pr = pred + b * (2 * G + 2);
  pr[0] = ctr.q0;
  pr[1] = ctr.q1;
  pr[2] = cvr.q0;
  pr[3] = cvr.q1;
  pr[2 * G] = 1.f - r;
  pr[2 * G + 1] = r;
  const float c0 = log_loss(p1, y), c2 = log_loss(r, t);
  float c1 = 0.f, dq_cf = 0.f, di = 0.f;      // the counterfactual term and its derivatives by q1 and i1
  Soft2 imp = ctr;
  if (mode == REC_ESM_IPW) {
    float ips = 1.f / fmaxf(p1 * (float)click_count[0], 1e-6f);
    ips = fminf(fmaxf(ips, -15.f), 15.f) * (float)d.batch;
    c1 = log_loss(q1, t) * ips * o;
    dq_cf = d_log_loss(q1, t) * ips * o;
  } else if (mode == REC_ESM_DR) {
    imp = soft2(x[4], x[5], true);
    pr[4] = imp.q0;
    pr[5] = imp.q1;
    const float i1 = imp.q1;
    const float e = log_loss(q1, t) - i1;
    const float ips = fminf(fmaxf(o / fmaxf(p1, 1e-6f), -15.f), 15.f);
    c1 = i1 + e * ips + e * e * ips;
    const float de = ips + 2.f * e * ips;     // d c1 / d e
    dq_cf = d_log_loss(q1, t) * de;
    di = 1.f - de;
  }
  cost[b * 3] = c0;
  cost[b * 3 + 1] = c1;
  cost[b * 3 + 2] = c2;
  if (dlogits == nullptr) return;
  const float gs = d.grad_scale, gw = d.global_w, cw = d.counterfactual_w;
  const float dr = gw * d_log_loss(r, t);      // by the product r = p1 q1
  float dp = gs * (d_log_loss(p1, y) + dr * q1);
  float dq = gs * (dr * p1 + cw * dq_cf);
  if (!ctr.open) dp = 0.f;                     // torch.clamp: the gradient passes where lo <= p <= hi
  if (!cvr.open) dq = 0.f;
  float* dl = dlogits + b * (2 * G);
  // softmax: d p1 / d x1 = p0 p1, d p1 / d x0 = -p0 p1 — ONE product per task, negated for column 0: d z0 = -d z1 exactly
  const float w0 = ctr.p0 * ctr.p1 * dp, w1 = cvr.p0 * cvr.p1 * dq;
  dl[0] = -w0;
  dl[1] = w0;
  dl[2] = -w1;
  dl[3] = w1;
  if (mode == REC_ESM_DR) {
    float dim = gs * cw * di;
    if (!imp.open) dim = 0.f;
    const float w2 = imp.p0 * imp.p1 * dim;
    dl[4] = -w2;
    dl[5] = w2;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_field_sumpool_fwd(int64_t batch, int32_t num_fields, int32_t max_len, int32_t emb_dim, int32_t row_stride,
                                     int64_t num_rows, int64_t padding_idx, const int64_t* ids, const float* W, float* out,
                                     int64_t ld_out, int32_t* status, void* stream) {
  REC_REQUIRE(batch >= 0 && num_fields >= 1, REC_EINVAL, "rec_field_sumpool_fwd: bad sizes (batch %lld, num_fields %d)",
              (long long)batch, num_fields);
  REC_REQUIRE(max_len >= 1 && max_len <= REC_FIELD_SUMPOOL_MAX_LEN, REC_EINVAL, "rec_field_sumpool_fwd: bad max_len %d (1..%d)",
              max_len, REC_FIELD_SUMPOOL_MAX_LEN);
  REC_REQUIRE(emb_dim >= 1 && emb_dim <= REC_FIELD_SUMPOOL_MAX_DIM, REC_EINVAL, "rec_field_sumpool_fwd: bad emb_dim %d (1..%d)",
              emb_dim, REC_FIELD_SUMPOOL_MAX_DIM);
  REC_REQUIRE(row_stride >= emb_dim && num_rows >= 1, REC_EINVAL,
              "rec_field_sumpool_fwd: bad table (row_stride %d below emb_dim %d, or num_rows %lld)", row_stride, emb_dim,
              (long long)num_rows);
  const int64_t packed = (int64_t)num_fields * emb_dim;
  if (ld_out == 0) ld_out = packed;
  REC_REQUIRE(ld_out >= packed, REC_EINVAL, "rec_field_sumpool_fwd: bad ld_out %lld: below the packed width %lld",
              (long long)ld_out, (long long)packed);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && out, REC_EINVAL, "rec_field_sumpool_fwd: null pointer argument");
  const bool vec = emb_dim % 4 == 0 && row_stride % 4 == 0 && ld_out % 4 == 0 && aligned16(W) && aligned16(out);
  const int cols = vec ? emb_dim / 4 : emb_dim;
  int shift = 0;
  while ((1 << shift) < cols && shift < 6) ++shift;
  const int rows = kBlock >> shift;
  REC_REQUIRE(batch <= ((1ll << 62) / num_fields) / max_len, REC_ESHAPE, "rec_field_sumpool_fwd: too many lookups");
  const int64_t pairs = batch * num_fields;
  const int64_t grid = (pairs + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_field_sumpool_fwd: too many rows");
  if (vec)
    hipLaunchKernelGGL(field_sumpool_fwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, pairs,
                       (int)num_fields, (int)max_len, (int)emb_dim, (int64_t)row_stride, num_rows, padding_idx, shift, ids, W, out,
                       ld_out, status);
  else
    hipLaunchKernelGGL(field_sumpool_fwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, pairs,
                       (int)num_fields, (int)max_len, (int)emb_dim, (int64_t)row_stride, num_rows, padding_idx, shift, ids, W, out,
                       ld_out, status);
  return check_launch("rec_field_sumpool_fwd");
}

extern "C" int rec_esm_head(const rec_esm_head_desc* desc, const float* logits, const int64_t* click, const int64_t* buy,
                            int64_t* click_count, float* pred, float* cost, float* dlogits, void* stream) {
  REC_REQUIRE(desc != nullptr, REC_EINVAL, "rec_esm_head: null descriptor");
  rec_esm_head_desc d = *desc;
  REC_REQUIRE(d.batch >= 0, REC_EINVAL, "rec_esm_head: bad batch %lld", (long long)d.batch);
  REC_REQUIRE(d.mode == REC_ESM_ESMM || d.mode == REC_ESM_IPW || d.mode == REC_ESM_DR, REC_EINVAL,
              "rec_esm_head: bad mode %d (0 ESMM, 1 IPW, 2 DR)", d.mode);
  const int64_t packed = d.mode == REC_ESM_DR ? 6 : 4;
  if (d.ld_logit == 0) d.ld_logit = packed;
  REC_REQUIRE(d.ld_logit >= packed, REC_EINVAL, "rec_esm_head: bad ld_logit %lld: below the packed width %lld",
              (long long)d.ld_logit, (long long)packed);
  REC_REQUIRE(d.mode != REC_ESM_IPW || click_count != nullptr, REC_EINVAL,
              "rec_esm_head: null click_count (the IPW mode needs the batch's click count)");
  if (d.batch == 0) return REC_OK;
  REC_REQUIRE(logits && click && buy && pred && cost, REC_EINVAL, "rec_esm_head: null pointer argument");
  const int64_t grid = (d.batch + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_esm_head: too many rows");
  if (click_count != nullptr) {
    hipLaunchKernelGGL(esm_click_count_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, d.batch, click, click_count);
    if (int rc = check_launch("rec_esm_head (click count)")) return rc;
  }
  hipLaunchKernelGGL(esm_head_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, d, logits, click, buy,
                     click_count, pred, cost, dlogits);
  return check_launch("rec_esm_head");
}
