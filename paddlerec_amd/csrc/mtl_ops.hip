// The multitask family (models/multitask: MMoE, PLE) on gfx950: what sits between the packed expert / gate GEMM and the
// towers, and the head every net of the family ends in.
//
//   rec_mtl_mix_fwd   <- mmoe/net.py:96-101, ple/net.py:194-222: per gate a softmax over its experts and the weighted sum
//                        of their (post-ReLU) outputs
//   rec_mtl_mix_bwd   <- the backward of both, with the experts' ReLU folded in: dH | dlogits in the column layout of the
//                        packed image, so one weight-gradient GEMM follows
//   rec_mtl_head      <- net.py: softmax over two classes, paddle.clip(1e-15, 1 - 1e-15); dygraph_model.py create_loss:
//                        slice column 1, log_loss (epsilon 1e-4) — predictions, per-sample cost and d(logits)
//
// Mapping.  A row of H is n_slots * S floats, at most a few hundred in practice, so a ROW GROUP of 2^k lanes (k chosen on the
// host: the smallest power of two that covers S / VEC columns, at most 64) owns one sample and a 256-thread block holds
// 256 >> k samples.  Lane l of a group owns the VEC-wide column chunks l, l + 2^k, ... of every expert slot; VEC is 4
// (float4 accesses) when S, the strides and the addresses allow it and 1 otherwise.  A gate has at most 64 experts: every
// lane of the group walks the gate's logits itself (the loads are one address per group, a broadcast), so the softmax
// needs no cross-lane step and no LDS, and every lane holds the same probabilities bit for bit (where a whole wave owns the
// row and makes several column passes, lane j keeps p_j and the passes shuffle it: expf is not called per pass).  The
// backward's dot products over s are a per-lane chain over the lane's chunks followed by a butterfly over the group.
// Every sum has a fixed order, nothing is atomic and no kernel takes a workspace: a rerun is bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

// slot of expert j of gate g (j < count0 + count1)
__device__ __forceinline__ int mix_slot(const rec_mtl_mix_desc& d, int g, int j) {
  const int n0 = d.count0[g];
  return j < n0 ? d.first0[g] + j : d.first1[g] + (j - n0);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void mtl_mix_fwd_kernel(const rec_mtl_mix_desc d, const int lane_shift, const float* H,
                                                             const float* logits, float* prob, float* mix) {
  const int lanes = 1 << lane_shift;
  const int64_t row = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (row >= d.batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const int S = d.expert_size;
  const float* h = H + row * d.ld_h;
  const float* lg = logits + row * d.ld_logit;
  float* pr = prob + row * d.ld_prob;
  float* mo = mix + row * d.ld_out;
  for (int g = 0; g < d.n_gates; ++g) {
    const int n = d.count0[g] + d.count1[g];
    float m = lg[0];
    for (int j = 1; j < n; ++j) m = fmaxf(m, lg[j]);
    float sum = 0.f;
    for (int j = 0; j < n; ++j) sum += expf(lg[j] - m);
    const float inv = 1.f / sum;
    if (lanes == kWave) {
      // a whole wave on the row (more than 32 column chunks, possibly several passes): lane j keeps p_j, n <= 64, and
      // the passes fetch it with a shuffle instead of calling expf again; the pass count is wave-uniform
      const float mine = lane < n ? expf(lg[lane] - m) * inv : 0.f;
      for (int c0 = 0; c0 < S; c0 += kWave * VEC) {
        const int c = c0 + lane * VEC;
        const bool on = c < S;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int j = 0; j < n; ++j) {
          const float p = __shfl(mine, j, kWave);
          if (on) {
            float hv[VEC];
            vload<VEC>(hv, h + (int64_t)mix_slot(d, g, j) * S + c);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = fmaf(p, hv[v], acc[v]);
          }
        }
        if (on) vstore<VEC>(mo + (int64_t)g * S + c, acc);
      }
      if (lane < n) pr[lane] = mine;
    } else {
      const int c = lane * VEC;                    // fewer than 64 lanes cover S in one pass
      if (c < S) {
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int j = 0; j < n; ++j) {
          const float p = expf(lg[j] - m) * inv;
          float hv[VEC];
          vload<VEC>(hv, h + (int64_t)mix_slot(d, g, j) * S + c);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = fmaf(p, hv[v], acc[v]);
        }
        vstore<VEC>(mo + (int64_t)g * S + c, acc);
      }
      for (int j = lane; j < n; j += lanes) pr[j] = expf(lg[j] - m) * inv;
    }
    lg += n;
    pr += n;
  }
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void mtl_mix_bwd_kernel(const rec_mtl_mix_desc d, const int lane_shift, const int relu,
                                                             const float* H, const float* prob, const float* dmix, float* dH,
                                                             float* dlogits) {
  const int lanes = 1 << lane_shift;
  int64_t row = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  const bool valid = row < d.batch;      // a group past the end reads the last row and stores nothing: its lanes stay
  if (!valid) row = d.batch - 1;         // in the butterflies of the wave
  const int lane = threadIdx.x & (lanes - 1);
  const int S = d.expert_size;
  const float* h = H + row * d.ld_h;
  const float* pr = prob + row * d.ld_prob;
  const float* dm = dmix + row * d.ld_out;
  float* dh = dH + row * d.ld_dh;
  float* dl = dlogits + row * d.ld_dlogit;
  // dlogits[g, j] = p_j (dp_j - sum_k p_k dp_k), dp_j = dmix[g, :] . H[slot(g, j), :]
  int col0 = 0;
  for (int g = 0; g < d.n_gates; ++g) {
    const int n = d.count0[g] + d.count1[g];
    const float* dmg = dm + (int64_t)g * S;
    float t = 0.f;
    for (int j = 0; j < n; ++j) {
      const float* hs = h + (int64_t)mix_slot(d, g, j) * S;
      float part = 0.f;
      for (int c = lane * VEC; c < S; c += lanes * VEC) {
        float a[VEC], b[VEC];
        vload<VEC>(a, dmg + c);
        vload<VEC>(b, hs + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) part = fmaf(a[v], b[v], part);
      }
      for (int o = lanes >> 1; o > 0; o >>= 1) part += __shfl_xor(part, o, kWave);
      t = fmaf(pr[col0 + j], part, t);
      if (valid && lane == 0) dl[col0 + j] = part;          // dp_j, finished below by the lane that wrote it
    }
    if (valid && lane == 0)
      for (int j = 0; j < n; ++j) dl[col0 + j] = pr[col0 + j] * (dl[col0 + j] - t);
    col0 += n;
  }
  // dH[e, :] = sum over the gates that select slot e, g ascending, of p[g, j(e)] dmix[g, :]
  for (int c = lane * VEC; c < S; c += lanes * VEC) {
    for (int e = 0; e < d.n_slots; ++e) {
      float acc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      int base = 0;
      for (int g = 0; g < d.n_gates; ++g) {
        const int n0 = d.count0[g], n1 = d.count1[g];
        int j = -1;
        if (e >= d.first0[g] && e < d.first0[g] + n0) j = e - d.first0[g];
        else if (e >= d.first1[g] && e < d.first1[g] + n1) j = n0 + e - d.first1[g];
        if (j >= 0) {
          const float p = pr[base + j];
          float a[VEC];
          vload<VEC>(a, dm + (int64_t)g * S + c);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] = fmaf(p, a[v], acc[v]);
        }
        base += n0 + n1;
      }
      if (relu) {
        float hv[VEC];
        vload<VEC>(hv, h + (int64_t)e * S + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = hv[v] > 0.f ? acc[v] : 0.f;
      }
      if (valid) vstore<VEC>(dh + (int64_t)e * S + c, acc);
    }
  }
}

// one thread per (sample, task)
__global__ __launch_bounds__(kBlock) void mtl_head_kernel(const int64_t batch, const int n_tasks, const float* logits,
                                                          const int64_t ld, const float* label, const int64_t ld_label,
                                                          const float grad_scale, float* pred, float* cost, float* dlogits) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= batch * n_tasks) return;
  const int64_t b = i / n_tasks;
  const int t = (int)(i - b * n_tasks);
  const float lo = 1e-15f, hi = 1.0f - 1e-15f;     // paddle.clip's bounds as a float32 tensor sees them (hi is 1)
  const float eps = 1e-4f;
  const float x0 = logits[b * ld + 2 * t], x1 = logits[b * ld + 2 * t + 1];
  const float m = fmaxf(x0, x1);
  const float e0 = expf(x0 - m), e1 = expf(x1 - m);
  const float s = e0 + e1;
  const float p0 = e0 / s, p1 = e1 / s;
  const float q0 = fminf(fmaxf(p0, lo), hi), q1 = fminf(fmaxf(p1, lo), hi);
  const float y = label[b * ld_label + t];
  pred[i * 2] = q0;
  pred[i * 2 + 1] = q1;
  cost[i] = -y * logf(q1 + eps) - (1.f - y) * logf(1.f - q1 + eps);
  if (dlogits != nullptr) {
    float dq = grad_scale * ((1.f - y) / (1.f - q1 + eps) - y / (q1 + eps));
    if (!(p1 >= lo && p1 <= hi)) dq = 0.f;         // torch.clamp: the gradient passes where lo <= p <= hi
    const float w = p0 * p1 * dq;                  // softmax: d p1 / d x1 = p1 (1 - p1) = p0 p1, d p1 / d x0 = -p0 p1
    dlogits[i * 2] = -w;
    dlogits[i * 2 + 1] = w;
  }
}

struct MixPlan {
  int vec, lane_shift;
  int64_t grid;
  int n_logit;
};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Every check of the descriptor; fills the packed strides into *d.  No device call.
int mix_check(const char* what, rec_mtl_mix_desc* d, int* n_logit) {
  REC_REQUIRE(d->batch >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)d->batch);
  REC_REQUIRE(d->expert_size >= 1 && d->expert_size <= REC_MTL_MAX_EXPERT_SIZE, REC_EINVAL, "%s: bad expert_size %d (1..%d)",
              what, d->expert_size, REC_MTL_MAX_EXPERT_SIZE);
  REC_REQUIRE(d->n_slots >= 1 && d->n_slots <= REC_MTL_MAX_SLOTS, REC_EINVAL, "%s: bad n_slots %d (1..%d)", what, d->n_slots,
              REC_MTL_MAX_SLOTS);
  REC_REQUIRE(d->n_gates >= 1 && d->n_gates <= REC_MTL_MAX_GATES, REC_EINVAL, "%s: bad n_gates %d (1..%d)", what, d->n_gates,
              REC_MTL_MAX_GATES);
  int total = 0;
  for (int g = 0; g < d->n_gates; ++g) {
    const int f0 = d->first0[g], n0 = d->count0[g], f1 = d->first1[g], n1 = d->count1[g];
    REC_REQUIRE(n0 >= 1 && n1 >= 0 && n0 + n1 <= REC_MTL_MAX_PER_GATE, REC_EINVAL,
                "%s: bad expert counts of gate %d (%d + %d; count0 >= 1, count1 >= 0, at most %d together)", what, g, n0, n1,
                REC_MTL_MAX_PER_GATE);
    REC_REQUIRE(f0 >= 0 && f0 + n0 <= d->n_slots, REC_EINVAL, "%s: bad first range of gate %d ([%d, %d) of %d slots)", what,
                g, f0, f0 + n0, d->n_slots);
    if (n1 > 0) {
      REC_REQUIRE(f1 >= 0 && f1 + n1 <= d->n_slots, REC_EINVAL, "%s: bad second range of gate %d ([%d, %d) of %d slots)",
                  what, g, f1, f1 + n1, d->n_slots);
      REC_REQUIRE(f1 >= f0 + n0 || f1 + n1 <= f0, REC_EINVAL, "%s: bad ranges of gate %d: [%d, %d) and [%d, %d) overlap", what,
                  g, f0, f0 + n0, f1, f1 + n1);
    }
    total += n0 + n1;
  }
  const int64_t w_h = (int64_t)d->n_slots * d->expert_size, w_out = (int64_t)d->n_gates * d->expert_size;
  int64_t* ld[6] = {&d->ld_h, &d->ld_logit, &d->ld_prob, &d->ld_out, &d->ld_dh, &d->ld_dlogit};
  const int64_t packed[6] = {w_h, total, total, w_out, w_h, total};
  const char* names[6] = {"ld_h", "ld_logit", "ld_prob", "ld_out", "ld_dh", "ld_dlogit"};
  for (int i = 0; i < 6; ++i) {
    if (*ld[i] == 0) *ld[i] = packed[i];
    REC_REQUIRE(*ld[i] >= packed[i], REC_EINVAL, "%s: bad %s %lld: below the packed width %lld", what, names[i],
                (long long)*ld[i], (long long)packed[i]);
  }
  *n_logit = total;
  return REC_OK;
}

int mix_plan(const char* what, const rec_mtl_mix_desc& d, bool vec_ok, MixPlan* p) {
  p->vec = vec_ok && d.expert_size % 4 == 0 ? 4 : 1;
  const int cols = d.expert_size / p->vec;
  int shift = 0;
  while ((1 << shift) < cols && shift < 6) ++shift;
  p->lane_shift = shift;
  const int rows = kBlock >> shift;
  p->grid = (d.batch + rows - 1) / rows;
  REC_REQUIRE(p->grid < (1ll << 31), REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_mtl_mix_fwd(const rec_mtl_mix_desc* desc, const float* H, const float* logits, float* prob, float* mix,
                               void* stream) {
  REC_REQUIRE(desc != nullptr, REC_EINVAL, "rec_mtl_mix_fwd: null descriptor");
  rec_mtl_mix_desc d = *desc;
  int n_logit = 0;
  if (int rc = mix_check("rec_mtl_mix_fwd", &d, &n_logit)) return rc;
  if (d.batch == 0) return REC_OK;
  REC_REQUIRE(H && logits && prob && mix, REC_EINVAL, "rec_mtl_mix_fwd: null pointer argument");
  REC_REQUIRE(prob != logits && mix != H, REC_EINVAL, "rec_mtl_mix_fwd: an output aliases an input");
  const bool vec_ok = d.ld_h % 4 == 0 && d.ld_out % 4 == 0 && aligned16(H) && aligned16(mix);
  MixPlan p;
  if (int rc = mix_plan("rec_mtl_mix_fwd", d, vec_ok, &p)) return rc;
  if (p.vec == 4)
    hipLaunchKernelGGL(mtl_mix_fwd_kernel<4>, dim3((unsigned)p.grid), dim3(kBlock), 0, (hipStream_t)stream, d, p.lane_shift, H,
                       logits, prob, mix);
  else
    hipLaunchKernelGGL(mtl_mix_fwd_kernel<1>, dim3((unsigned)p.grid), dim3(kBlock), 0, (hipStream_t)stream, d, p.lane_shift, H,
                       logits, prob, mix);
  return check_launch("rec_mtl_mix_fwd");
}

extern "C" int rec_mtl_mix_bwd(const rec_mtl_mix_desc* desc, const float* H, const float* prob, const float* dmix, int32_t relu,
                               float* dH, float* dlogits, void* stream) {
  REC_REQUIRE(desc != nullptr, REC_EINVAL, "rec_mtl_mix_bwd: null descriptor");
  rec_mtl_mix_desc d = *desc;
  int n_logit = 0;
  if (int rc = mix_check("rec_mtl_mix_bwd", &d, &n_logit)) return rc;
  if (d.batch == 0) return REC_OK;
  REC_REQUIRE(H && prob && dmix && dH && dlogits, REC_EINVAL, "rec_mtl_mix_bwd: null pointer argument");
  REC_REQUIRE(dH != H && dH != dmix && dlogits != prob, REC_EINVAL, "rec_mtl_mix_bwd: an output aliases an input");
  const bool vec_ok = d.ld_h % 4 == 0 && d.ld_out % 4 == 0 && d.ld_dh % 4 == 0 && aligned16(H) && aligned16(dmix) && aligned16(dH);
  MixPlan p;
  if (int rc = mix_plan("rec_mtl_mix_bwd", d, vec_ok, &p)) return rc;
  if (p.vec == 4)
    hipLaunchKernelGGL(mtl_mix_bwd_kernel<4>, dim3((unsigned)p.grid), dim3(kBlock), 0, (hipStream_t)stream, d, p.lane_shift,
                       relu != 0, H, prob, dmix, dH, dlogits);
  else
    hipLaunchKernelGGL(mtl_mix_bwd_kernel<1>, dim3((unsigned)p.grid), dim3(kBlock), 0, (hipStream_t)stream, d, p.lane_shift,
                       relu != 0, H, prob, dmix, dH, dlogits);
  return check_launch("rec_mtl_mix_bwd");
}

extern "C" int rec_mtl_head(int64_t batch, int32_t n_tasks, const float* logits, int64_t ld, const float* label,
                            int64_t ld_label, float grad_scale, float* pred, float* cost, float* dlogits, void* stream) {
  REC_REQUIRE(batch >= 0 && n_tasks >= 1 && n_tasks <= REC_MTL_MAX_TASKS, REC_EINVAL,
              "rec_mtl_head: bad sizes (batch %lld, n_tasks %d; 1..%d tasks)", (long long)batch, n_tasks, REC_MTL_MAX_TASKS);
  if (ld == 0) ld = 2 * n_tasks;
  if (ld_label == 0) ld_label = n_tasks;
  REC_REQUIRE(ld >= 2 * n_tasks && ld_label >= n_tasks, REC_EINVAL,
              "rec_mtl_head: bad row stride (ld %lld, ld_label %lld): below the packed width", (long long)ld, (long long)ld_label);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(logits && label && pred && cost, REC_EINVAL, "rec_mtl_head: null pointer argument");
  const int64_t grid = (batch * n_tasks + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mtl_head: too many rows");
  hipLaunchKernelGGL(mtl_head_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, (int)n_tasks, logits, ld,
                     label, ld_label, grad_scale, pred, cost, dlogits);
  return check_launch("rec_mtl_head");
}
