// MIND (models/recall/mind) on gfx950: the pieces its hot path lacks.
//
//   rec_mind_routing_fwd / _bwd    <- mind/net.py:178-234 Mind_Capsual_Layer.forward: the dynamic (B2I) routing over the mapped
//                                     history low [B, T, H] — iters - 1 rounds of masked softmax over T, W x low, squash,
//                                     low x caps^T, then the final softmax over K — and the backward of its last product
//   rec_mind_label_attn_fwd / _bwd <- mind/net.py:284-297 label_aware_attention: <caps2_k, target>, pow, softmax over K, the
//                                     weighted sum of the capsules, and its backward to d(caps2) and d(target)
//   rec_mind_ssm_head              <- mind/net.py:63-113 Mind_SampledSoftmaxLoss_Layer.forward after the gathers: true logit,
//                                     accidental-hit mask, both log_q subtractions, log-sum-exp over 1 + n columns, the loss and
//                                     d(sample logits), d(true logit) in one launch
//
// Mapping.  Routing and head give one 64-lane WAVE to a sample; a block holds up to four of them.  The routing forward reads
// low[b] from global memory ONCE into the wave's own LDS slice [T][H | 1] (an odd row stride: the column walk of the
// B_delta product, lane = t, meets 32 different banks) and keeps it there for every round; the [B, K, T, H] tile of the
// reference is never formed.  The coupling weights and the squashed capsules sit beside it TRANSPOSED, W^T [T][8] and
// caps^T [H][8], so that all k_max values of a position or a column are one 16-byte LDS broadcast (two above four capsules).  Lane t owns the routing logits B[k][t] of all K capsules in registers (loops over
// REC_MIND_MAX_K fully unrolled and guarded by k < K, never an array indexed by a runtime value): the softmax over T is a
// butterfly over the wave, the final softmax over K is lane-local.  In the W x low product lane c owns the columns c and
// c + 64 of all K capsules and walks t in ascending order.  Waves of a block
// never exchange data; __syncthreads() only orders a wave's own LDS writes before its reads, and a wave past the batch
// repeats the last sample without storing, so every wave reaches every barrier.  The label attention uses the row-group
// layout of aitm_ops.hip (2^k lanes per sample, VEC-wide column chunks).  Every sum is a lane's partial in ascending order
// followed by an xor butterfly: a fixed order.  No workspace, no float atomics, one writer per output element: a rerun is
// bit-identical.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kMaxK = REC_MIND_MAX_K;
constexpr float kPad = -4294967295.0f;            // net.py:189: -2**32 + 1 (float32 rounds it to -2^32)

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, kWave));
  return x;
}
__device__ __forceinline__ float lanes_sum(float x, const int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  return x;
}

// net.py:155-162: n2 / (1 + n2) / sqrt(n2 + 1e-8)
__device__ __forceinline__ float squash_scale(const float n2) { return n2 / (1.f + n2) / sqrtf(n2 + 1e-8f); }

constexpr int kCapStride = 8;                     // floats per LDS row of W^T [T][8] and caps^T [H][8]: two 16-byte reads

// the k_max values of one row of W^T or caps^T: one 16-byte LDS broadcast, two above four capsules
__device__ __forceinline__ void load_caps_row(const float* row, const int K, float (&w)[kMaxK]) {
  const float4 a = *reinterpret_cast<const float4*>(row);
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (K > 4) b = *reinterpret_cast<const float4*>(row + 4);
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void store_caps_row(float* row, const int K, const float (&w)[kMaxK]) {
  *reinterpret_cast<float4*>(row) = make_float4(w[0], w[1], w[2], w[3]);
  if (K > 4) *reinterpret_cast<float4*>(row + 4) = make_float4(w[4], w[5], w[6], w[7]);
}

// Z[k][c] = sum_t W^T[t][k] * sl[t][c] for the lane's two columns (c = lane, lane + 64), t ascending
__device__ __forceinline__ void mix_low(const int T, const int K, const int H, const int ldh, const int lane, const float* sl,
                                        const float* sw, float (&z)[kMaxK][2]) {
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) z[k][0] = z[k][1] = 0.f;
  const bool c0 = lane < H, c1 = lane + kWave < H;
  const bool wide = H > kWave;                        // wave-uniform: the second column pass exists at all
  for (int t = 0; t < T; ++t) {
    const float l0 = c0 ? sl[t * ldh + lane] : 0.f;
    float l1 = 0.f;
    if (wide) l1 = c1 ? sl[t * ldh + lane + kWave] : 0.f;
    float w[kMaxK];
    load_caps_row(sw + t * kCapStride, K, w);
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        z[k][0] += w[k] * l0;
        z[k][1] += w[k] * l1;
      }
  }
}

// one wave per sample; dynamic LDS: per wave W^T [T][8], caps^T [H][8], low [T][H | 1]
template <int VEC>
__global__ __launch_bounds__(kBlock) void mind_routing_fwd_kernel(const int64_t batch, const int T, const int K, const int H,
                                                                  const int iters, const int per_wave, const float* low,
                                                                  const int64_t ld_low, const int64_t* seq_len,
                                                                  const float* logits, float* W, float* Z, float* caps) {
  extern __shared__ __align__(16) float smem[];
  const int ldh = H | 1;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = b < batch;
  if (!live) b = batch - 1;
  float* sw = smem + (size_t)wave * per_wave;          // per_wave is a multiple of 4 floats: every slice is 16-byte aligned
  float* sc = sw + T * kCapStride;
  float* sl = sc + H * kCapStride;
  {
    const float* src = low + b * T * ld_low;
    const int chunks = H / VEC;
    for (int i = lane; i < T * chunks; i += kWave) {
      const int t = i / chunks, c = (i - t * chunks) * VEC;
      float v[VEC];
      vload<VEC>(v, src + (int64_t)t * ld_low + c);
#pragma unroll
      for (int j = 0; j < VEC; ++j) sl[t * ldh + c + j] = v[j];
    }
  }
  const bool mine = lane < T;
  const bool valid = (int64_t)lane < seq_len[b];          // net.py:175: row_vector < lengths
  float bl[kMaxK], w[kMaxK];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) bl[k] = (k < K && mine) ? logits[k * T + lane] : 0.f;
  float z[kMaxK][2];
  __syncthreads();
  for (int r = 0; r + 1 < iters; ++r) {
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      w[k] = 0.f;
      if (k < K) {                                         // softmax over T of where(mask, B, pad)
        const float x = mine ? (valid ? bl[k] : kPad) : -INFINITY;
        const float m = wave_max(x);
        const float e = mine ? expf(x - m) : 0.f;
        w[k] = e / wave_sum(e);
      }
    }
    if (mine) store_caps_row(sw + lane * kCapStride, K, w);
    __syncthreads();
    mix_low(T, K, H, ldh, lane, sl, sw, z);
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      w[k] = 0.f;
      if (k < K) {
        const float f = squash_scale(wave_sum(z[k][0] * z[k][0] + z[k][1] * z[k][1]));
        w[k] = f * z[k][0];
        z[k][1] *= f;
      }
    }
    if (lane < H) store_caps_row(sc + lane * kCapStride, K, w);
    if (lane + kWave < H) {
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) w[k] = z[k][1];
      store_caps_row(sc + (lane + kWave) * kCapStride, K, w);
    }
    __syncthreads();
    if (mine) {                                            // B += low x caps^T, padded positions too
      float d[kMaxK];
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) d[k] = 0.f;
      for (int h = 0; h < H; ++h) {
        const float l = sl[lane * ldh + h];
        load_caps_row(sc + h * kCapStride, K, w);
#pragma unroll
        for (int k = 0; k < kMaxK; ++k)
          if (k < K) d[k] += l * w[k];
      }
#pragma unroll
      for (int k = 0; k < kMaxK; ++k) bl[k] += d[k];
    }
  }
  if (mine) {                                              // net.py:226: the final softmax runs over K
    float m = -INFINITY, s = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        bl[k] = valid ? bl[k] : kPad;
        m = fmaxf(m, bl[k]);
      }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        bl[k] = expf(bl[k] - m);
        s += bl[k];
      }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      w[k] = 0.f;
      if (k < K) {
        w[k] = bl[k] / s;
        if (live) W[(b * K + k) * T + lane] = w[k];
      }
    }
    store_caps_row(sw + lane * kCapStride, K, w);
  }
  __syncthreads();
  mix_low(T, K, H, ldh, lane, sl, sw, z);
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K) {
      const float f = squash_scale(wave_sum(z[k][0] * z[k][0] + z[k][1] * z[k][1]));
      if (live) {
        const int64_t o = (b * K + k) * H;
        if (lane < H) {
          Z[o + lane] = z[k][0];
          caps[o + lane] = f * z[k][0];
        }
        if (lane + kWave < H) {
          Z[o + lane + kWave] = z[k][1];
          caps[o + lane + kWave] = f * z[k][1];
        }
      }
    }
}

// one wave per sample: dZ through squash, then d_low[t] = sum_k W[k][t] dZ[k]
__global__ __launch_bounds__(kBlock) void mind_routing_bwd_kernel(const int64_t batch, const int T, const int K, const int H,
                                                                  const float* d_caps, const float* Z, const float* W,
                                                                  float* d_low, const int64_t ld_dlow) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  const bool c0 = lane < H, c1 = lane + kWave < H;
  float dz[kMaxK][2], w[kMaxK];
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    dz[k][0] = dz[k][1] = w[k] = 0.f;
    if (k < K) {
      const int64_t o = (b * K + k) * H;
      const float z0 = c0 ? Z[o + lane] : 0.f, z1 = c1 ? Z[o + lane + kWave] : 0.f;
      const float g0 = c0 ? d_caps[o + lane] : 0.f, g1 = c1 ? d_caps[o + lane + kWave] : 0.f;
      const float n2 = wave_sum(z0 * z0 + z1 * z1);
      const float dot = wave_sum(z0 * g0 + z1 * g1);
      const float q = sqrtf(n2 + 1e-8f), p1 = 1.f + n2;
      const float f = n2 / p1 / q;                                           // caps = f Z
      const float df = 1.f / (p1 * p1) / q - 0.5f * (n2 / p1) / ((n2 + 1e-8f) * q);   // d f / d n2
      const float a = 2.f * df * dot;
      dz[k][0] = f * g0 + a * z0;
      dz[k][1] = f * g1 + a * z1;
      if (lane < T) w[k] = W[(b * K + k) * T + lane];
    }
  }
  for (int t = 0; t < T; ++t) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        const float wt = __shfl(w[k], t, kWave);
        a0 += wt * dz[k][0];
        a1 += wt * dz[k][1];
      }
    float* o = d_low + (b * T + t) * ld_dlow;
    if (c0) o[lane] = a0;
    if (c1) o[lane + kWave] = a1;
  }
}

// one row group per sample; caps2 rows b * K + k
template <int VEC>
__global__ __launch_bounds__(kBlock) void mind_label_attn_fwd_kernel(const int64_t batch, const int K, const int H,
                                                                     const int lane_shift, const float pow_p, const int unit_pow,
                                                                     const float* caps2, const int64_t ld_caps,
                                                                     const float* target, const int64_t ld_target, float* user,
                                                                     const int64_t ld_user, float* attn) {
  const int lanes = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const float* x = caps2 + b * K * ld_caps;
  const float* q = target + b * ld_target;
  float s[kMaxK];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    s[k] = 0.f;
    if (k < K) {
      float acc = 0.f;
      for (int c = lane * VEC; c < H; c += lanes * VEC) {
        float a[VEC], t[VEC];
        vload<VEC>(a, x + k * ld_caps + c);
        vload<VEC>(t, q + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc += a[v] * t[v];
      }
      acc = lanes_sum(acc, lanes);
      s[k] = unit_pow ? acc : powf(acc, pow_p);
      m = fmaxf(m, s[k]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K) {
      s[k] = expf(s[k] - m);
      sum += s[k];
    }
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K) {
      s[k] = s[k] / sum;
      if (lane == 0) attn[b * K + k] = s[k];
    }
  for (int c = lane * VEC; c < H; c += lanes * VEC) {
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        float a[VEC];
        vload<VEC>(a, x + k * ld_caps + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += s[k] * a[v];
      }
    vstore<VEC>(user + b * ld_user + c, acc);
  }
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void mind_label_attn_bwd_kernel(const int64_t batch, const int K, const int H,
                                                                     const int lane_shift, const float pow_p, const int unit_pow,
                                                                     const float* caps2, const int64_t ld_caps,
                                                                     const float* target, const int64_t ld_target,
                                                                     const float* attn, const float* d_user,
                                                                     const int64_t ld_duser, float* d_caps2,
                                                                     const int64_t ld_dcaps, float* d_target,
                                                                     const int64_t ld_dtarget) {
  const int lanes = 1 << lane_shift;
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> lane_shift) + (threadIdx.x >> lane_shift);
  if (b >= batch) return;
  const int lane = threadIdx.x & (lanes - 1);
  const float* x = caps2 + b * K * ld_caps;
  const float* q = target + b * ld_target;
  const float* g = d_user + b * ld_duser;
  float a[kMaxK], ds[kMaxK], dp[kMaxK];
  float dot = 0.f;                                   // sum_j a_j da_j, j ascending
#pragma unroll
  for (int k = 0; k < kMaxK; ++k) {
    a[k] = ds[k] = dp[k] = 0.f;
    if (k < K) {
      float acc = 0.f, sc = 0.f;
      for (int c = lane * VEC; c < H; c += lanes * VEC) {
        float xv[VEC], gv[VEC], tv[VEC];
        vload<VEC>(xv, x + k * ld_caps + c);
        vload<VEC>(gv, g + c);
        vload<VEC>(tv, q + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc += gv[v] * xv[v];
          sc += tv[v] * xv[v];
        }
      }
      a[k] = attn[b * K + k];
      ds[k] = lanes_sum(acc, lanes);                 // da_k
      dot += a[k] * ds[k];
      // d pow(s, p) / ds = p s^(p - 1) of the score s = <caps2_k, target>; p == 1 keeps the factor at exactly one
      dp[k] = unit_pow ? 1.f : pow_p * powf(lanes_sum(sc, lanes), pow_p - 1.f);
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxK; ++k)
    if (k < K) ds[k] = a[k] * (ds[k] - dot) * dp[k];  // d(score_k); one capsule: a = 1 and da - 1 * da = 0 exactly
  for (int c = lane * VEC; c < H; c += lanes * VEC) {
    float gv[VEC], tv[VEC], dt[VEC];
    vload<VEC>(gv, g + c);
    vload<VEC>(tv, q + c);
#pragma unroll
    for (int v = 0; v < VEC; ++v) dt[v] = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K) {
        float xv[VEC], dx[VEC];
        vload<VEC>(xv, x + k * ld_caps + c);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          dx[v] = a[k] * gv[v] + ds[k] * tv[v];
          dt[v] += ds[k] * xv[v];
        }
        vstore<VEC>(d_caps2 + (b * K + k) * ld_dcaps + c, dx);
      }
    vstore<VEC>(d_target + b * ld_dtarget + c, dt);
  }
}

// one wave per sample: the true logit, then three passes over the sample's n logits (maximum, sum, gradient)
__global__ __launch_bounds__(kBlock) void mind_ssm_head_kernel(const int64_t batch, const int H, const int n, const float* user,
                                                               const int64_t ld_user, const float* true_w, const int64_t ld_true,
                                                               const float* true_b, float* S, const int64_t ld_s,
                                                               const float* sample_b, const int64_t* labels, const int64_t* neg,
                                                               const float* logq_true, const float* logq_neg,
                                                               const float grad_scale, float* loss, float* d_true,
                                                               float* d_true_w, const int64_t ld_dtw, float* d_user0,
                                                               const int64_t ld_du0) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = (int64_t)blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  float acc = 0.f;
  for (int c = lane; c < H; c += kWave) acc += user[b * ld_user + c] * true_w[b * ld_true + c];
  const float x0 = wave_sum(acc) + true_b[b] - logq_true[b];
  const int64_t label = labels[b];
  float* s = S + b * ld_s;
  // net.py:94-101: the accidental-hit mask goes in BEFORE log_q comes off
  auto logit = [&](const int j) { return (neg[j] == label ? -1e30f : s[j] + sample_b[j]) - logq_neg[j]; };
  float m = x0;
  for (int j = lane; j < n; j += kWave) m = fmaxf(m, logit(j));
  m = wave_max(m);
  float sum = 0.f;
  for (int j = lane; j < n; j += kWave) sum += expf(logit(j) - m);
  const float e0 = expf(x0 - m);
  const float total = e0 + wave_sum(sum);
  for (int j = lane; j < n; j += kWave) s[j] = grad_scale * (expf(logit(j) - m) / total);
  const float dt = grad_scale * (e0 / total - 1.f);
  if (lane == 0) {
    loss[b] = m + logf(total) - x0;                  // -log_softmax[0]
    d_true[b] = dt;
  }
  // the two row scalings of the true column's backward: d(true_w) = d_true user, and d_true true_w, the term of d(user)
  // that the caller's dS x sample_w GEMM adds to
  for (int c = lane; c < H; c += kWave) {
    if (d_true_w != nullptr) d_true_w[b * ld_dtw + c] = dt * user[b * ld_user + c];
    if (d_user0 != nullptr) d_user0[b * ld_du0 + c] = dt * true_w[b * ld_true + c];
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

// the size checks the routing entry points share; -> 0 or the error
static int routing_check(const char* what, int64_t batch, int32_t T, int32_t K, int32_t H) {
  REC_REQUIRE(batch >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)batch);
  REC_REQUIRE(T >= 1 && T <= REC_MIND_MAX_T, REC_EINVAL, "%s: bad seq_len_max %d (1..%d)", what, T, REC_MIND_MAX_T);
  REC_REQUIRE(K >= 1 && K <= REC_MIND_MAX_K, REC_EINVAL, "%s: bad k_max %d (1..%d)", what, K, REC_MIND_MAX_K);
  REC_REQUIRE(H >= 1 && H <= REC_MIND_MAX_H, REC_EINVAL, "%s: bad hidden %d (1..%d)", what, H, REC_MIND_MAX_H);
  REC_REQUIRE(batch <= (1ll << 40), REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

extern "C" int rec_mind_routing_fwd(int64_t batch, int32_t seq_len_max, int32_t k_max, int32_t hidden, int32_t iters,
                                    const float* low, int64_t ld_low, const int64_t* seq_len, const float* routing_logits,
                                    float* W, float* Z, float* caps, void* stream) {
  const int T = seq_len_max, K = k_max, H = hidden;
  if (int rc = routing_check("rec_mind_routing_fwd", batch, T, K, H)) return rc;
  REC_REQUIRE(iters >= 1 && iters <= REC_MIND_MAX_ITERS, REC_EINVAL, "rec_mind_routing_fwd: bad iters %d (1..%d)", iters,
              REC_MIND_MAX_ITERS);
  if (ld_low == 0) ld_low = H;
  REC_REQUIRE(ld_low >= H, REC_EINVAL, "rec_mind_routing_fwd: bad ld_low %lld: below the packed width %d", (long long)ld_low, H);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(low && seq_len && routing_logits && W && Z && caps, REC_EINVAL, "rec_mind_routing_fwd: null pointer argument");
  // per wave: W^T [T][8], caps^T [H][8] and low [T][H | 1], rounded up to 16 bytes; at most 39184 bytes
  const int per_wave = (int)(((size_t)(T + H) * 8 + (size_t)T * (H | 1) + 3) / 4 * 4);
  const size_t per = (size_t)per_wave * sizeof(float);
  int waves = (int)((64u << 10) / per);               // stay within the 64 KiB a launch gets without an opt-in
  waves = waves > kBlock / kWave ? kBlock / kWave : waves;
  const int64_t grid = (batch + waves - 1) / waves;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mind_routing_fwd: too many rows");
  if (H % 4 == 0 && ld_low % 4 == 0 && aligned16(low))
    hipLaunchKernelGGL(mind_routing_fwd_kernel<4>, dim3((unsigned)grid), dim3(waves * kWave), waves * per, (hipStream_t)stream,
                       batch, T, K, H, (int)iters, per_wave, low, ld_low, seq_len, routing_logits, W, Z, caps);
  else
    hipLaunchKernelGGL(mind_routing_fwd_kernel<1>, dim3((unsigned)grid), dim3(waves * kWave), waves * per, (hipStream_t)stream,
                       batch, T, K, H, (int)iters, per_wave, low, ld_low, seq_len, routing_logits, W, Z, caps);
  return check_launch("rec_mind_routing_fwd");
}

extern "C" int rec_mind_routing_bwd(int64_t batch, int32_t seq_len_max, int32_t k_max, int32_t hidden, const float* d_caps,
                                    const float* Z, const float* W, float* d_low, int64_t ld_dlow, void* stream) {
  const int T = seq_len_max, K = k_max, H = hidden;
  if (int rc = routing_check("rec_mind_routing_bwd", batch, T, K, H)) return rc;
  if (ld_dlow == 0) ld_dlow = H;
  REC_REQUIRE(ld_dlow >= H, REC_EINVAL, "rec_mind_routing_bwd: bad ld_dlow %lld: below the packed width %d", (long long)ld_dlow,
              H);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(d_caps && Z && W && d_low, REC_EINVAL, "rec_mind_routing_bwd: null pointer argument");
  const int rows = kBlock / kWave;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mind_routing_bwd: too many rows");
  hipLaunchKernelGGL(mind_routing_bwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, T, K, H, d_caps,
                     Z, W, d_low, ld_dlow);
  return check_launch("rec_mind_routing_bwd");
}

// the checks rec_mind_label_attn_fwd and _bwd share; -> 0 or the error
static int label_attn_check(const char* what, int64_t batch, int32_t K, int32_t H, int64_t* ld_caps, int64_t* ld_target) {
  REC_REQUIRE(batch >= 0, REC_EINVAL, "%s: bad batch %lld", what, (long long)batch);
  REC_REQUIRE(K >= 1 && K <= REC_MIND_MAX_K, REC_EINVAL, "%s: bad k_max %d (1..%d)", what, K, REC_MIND_MAX_K);
  REC_REQUIRE(H >= 1 && H <= REC_MIND_MAX_H, REC_EINVAL, "%s: bad hidden %d (1..%d)", what, H, REC_MIND_MAX_H);
  if (*ld_caps == 0) *ld_caps = H;
  if (*ld_target == 0) *ld_target = H;
  REC_REQUIRE(*ld_caps >= H && *ld_target >= H, REC_EINVAL, "%s: bad ld_caps %lld / ld_target %lld: below the packed width %d",
              what, (long long)*ld_caps, (long long)*ld_target, H);
  REC_REQUIRE(batch <= (1ll << 40), REC_ESHAPE, "%s: too many rows", what);
  return REC_OK;
}

extern "C" int rec_mind_label_attn_fwd(int64_t batch, int32_t k_max, int32_t hidden, float pow_p, const float* caps2,
                                       int64_t ld_caps, const float* target, int64_t ld_target, float* user, int64_t ld_user,
                                       float* attn, void* stream) {
  const int K = k_max, H = hidden;
  if (int rc = label_attn_check("rec_mind_label_attn_fwd", batch, K, H, &ld_caps, &ld_target)) return rc;
  if (ld_user == 0) ld_user = H;
  REC_REQUIRE(ld_user >= H, REC_EINVAL, "rec_mind_label_attn_fwd: bad ld_user %lld: below the packed width %d",
              (long long)ld_user, H);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(caps2 && target && user && attn, REC_EINVAL, "rec_mind_label_attn_fwd: null pointer argument");
  const bool vec = H % 4 == 0 && ld_caps % 4 == 0 && ld_target % 4 == 0 && ld_user % 4 == 0 && aligned16(caps2) &&
                   aligned16(target) && aligned16(user);
  const int shift = group_shift(vec ? H / 4 : H);
  const int rows = kBlock >> shift;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mind_label_attn_fwd: too many rows");
  const int unit = pow_p == 1.0f;
  if (vec)
    hipLaunchKernelGGL(mind_label_attn_fwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, K, H,
                       shift, pow_p, unit, caps2, ld_caps, target, ld_target, user, ld_user, attn);
  else
    hipLaunchKernelGGL(mind_label_attn_fwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, K, H,
                       shift, pow_p, unit, caps2, ld_caps, target, ld_target, user, ld_user, attn);
  return check_launch("rec_mind_label_attn_fwd");
}

extern "C" int rec_mind_label_attn_bwd(int64_t batch, int32_t k_max, int32_t hidden, float pow_p, const float* caps2,
                                       int64_t ld_caps, const float* target, int64_t ld_target, const float* attn,
                                       const float* d_user, int64_t ld_duser, float* d_caps2, int64_t ld_dcaps, float* d_target,
                                       int64_t ld_dtarget, void* stream) {
  const int K = k_max, H = hidden;
  if (int rc = label_attn_check("rec_mind_label_attn_bwd", batch, K, H, &ld_caps, &ld_target)) return rc;
  if (ld_duser == 0) ld_duser = H;
  if (ld_dcaps == 0) ld_dcaps = H;
  if (ld_dtarget == 0) ld_dtarget = H;
  REC_REQUIRE(ld_duser >= H && ld_dcaps >= H && ld_dtarget >= H, REC_EINVAL,
              "rec_mind_label_attn_bwd: bad ld_duser %lld / ld_dcaps %lld / ld_dtarget %lld: below the packed width %d",
              (long long)ld_duser, (long long)ld_dcaps, (long long)ld_dtarget, H);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(caps2 && target && attn && d_user && d_caps2 && d_target, REC_EINVAL,
              "rec_mind_label_attn_bwd: null pointer argument");
  const bool vec = H % 4 == 0 && ld_caps % 4 == 0 && ld_target % 4 == 0 && ld_duser % 4 == 0 && ld_dcaps % 4 == 0 &&
                   ld_dtarget % 4 == 0 && aligned16(caps2) && aligned16(target) && aligned16(d_user) && aligned16(d_caps2) &&
                   aligned16(d_target);
  const int shift = group_shift(vec ? H / 4 : H);
  const int rows = kBlock >> shift;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mind_label_attn_bwd: too many rows");
  const int unit = pow_p == 1.0f;
  if (vec)
    hipLaunchKernelGGL(mind_label_attn_bwd_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, K, H,
                       shift, pow_p, unit, caps2, ld_caps, target, ld_target, attn, d_user, ld_duser, d_caps2, ld_dcaps, d_target,
                       ld_dtarget);
  else
    hipLaunchKernelGGL(mind_label_attn_bwd_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, K, H,
                       shift, pow_p, unit, caps2, ld_caps, target, ld_target, attn, d_user, ld_duser, d_caps2, ld_dcaps, d_target,
                       ld_dtarget);
  return check_launch("rec_mind_label_attn_bwd");
}

extern "C" int rec_mind_ssm_head(int64_t batch, int32_t hidden, int32_t n_sample, const float* user, int64_t ld_user,
                                 const float* true_w, int64_t ld_true, const float* true_b, float* S, int64_t ld_s,
                                 const float* sample_b, const int64_t* labels, const int64_t* neg, const float* logq_true,
                                 const float* logq_neg, float grad_scale, float* loss, float* d_true, float* d_true_w,
                                 int64_t ld_dtw, float* d_user0, int64_t ld_du0, void* stream) {
  const int H = hidden, n = n_sample;
  REC_REQUIRE(batch >= 0, REC_EINVAL, "rec_mind_ssm_head: bad batch %lld", (long long)batch);
  REC_REQUIRE(H >= 1 && H <= REC_MIND_HEAD_MAX_DIM, REC_EINVAL, "rec_mind_ssm_head: bad hidden %d (1..%d)", H,
              REC_MIND_HEAD_MAX_DIM);
  REC_REQUIRE(n >= 1 && n <= REC_MIND_MAX_NEG, REC_EINVAL, "rec_mind_ssm_head: bad n_sample %d (1..%d)", n, REC_MIND_MAX_NEG);
  if (ld_user == 0) ld_user = H;
  if (ld_true == 0) ld_true = H;
  if (ld_s == 0) ld_s = n;
  REC_REQUIRE(ld_user >= H && ld_true >= H, REC_EINVAL,
              "rec_mind_ssm_head: bad ld_user %lld / ld_true %lld: below the packed width %d", (long long)ld_user,
              (long long)ld_true, H);
  REC_REQUIRE(ld_s >= n, REC_EINVAL, "rec_mind_ssm_head: bad ld_s %lld: below the packed width %d", (long long)ld_s, n);
  if (ld_dtw == 0) ld_dtw = H;
  if (ld_du0 == 0) ld_du0 = H;
  REC_REQUIRE(ld_dtw >= H && ld_du0 >= H, REC_EINVAL,
              "rec_mind_ssm_head: bad ld_dtw %lld / ld_du0 %lld: below the packed width %d", (long long)ld_dtw,
              (long long)ld_du0, H);
  REC_REQUIRE(batch <= (1ll << 40), REC_ESHAPE, "rec_mind_ssm_head: too many rows");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(user && true_w && true_b && S && sample_b && labels && neg && logq_true && logq_neg && loss && d_true, REC_EINVAL,
              "rec_mind_ssm_head: null pointer argument");
  const int rows = kBlock / kWave;
  const int64_t grid = (batch + rows - 1) / rows;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "rec_mind_ssm_head: too many rows");
  hipLaunchKernelGGL(mind_ssm_head_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, batch, H, n, user, ld_user,
                     true_w, ld_true, true_b, S, ld_s, sample_b, labels, neg, logq_true, logq_neg, grad_scale, loss, d_true,
                     d_true_w, ld_dtw, d_user0, ld_du0);
  return check_launch("rec_mind_ssm_head");
}
