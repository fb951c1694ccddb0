// GateNet (rank/gatenet) gates, gfx950: the embedding gate fused into the lookup, and the elementwise passes around the
// hidden gate's GEMMs.
//
//   rec_gate_emb_fwd      <- emb = embedding(ids[s]); emb * sigmoid(sum(emb * w_s))   (gatenet/net.py:88-103; w_s is ONE
//                            scalar per field, so the gate's argument is w_s * sum_k e_k)
//   rec_gate_emb_bwd      <- its backward, in place on the layer-0 dX: g -> d e, and d w_s summed over the batch
//   rec_gate_hidden_fwd   <- y * tanh(y @ G) given t = y @ G                         (gatenet/net.py:114-118)
//   rec_gate_hidden_bwd   <- d t = u * y * (1 - h^2) and the direct term u * h for upstream u, h = tanh(t)
//   rec_relu_mask_inplace <- dy *= (y > 0): the ReLU in front of the gate (the mask is y's, not the gated output's)
// The lookups use the row groups of emb_ops.hip: LANES lanes per lookup, VEC floats per lane.  The row sum t and
// <g, e> are reduced over the group's lanes by shuffle, so every lane of a group ends up with the same a = sigmoid(w t);
// no lane leaves before the shuffles.  d w_s is summed without float atomics: a block walks a fixed set of lookup
// chunks, adds the chunk's contributions per field in lookup order, and a fold kernel adds the blocks' partials in
// block order, so two runs on the same inputs give the same bits.
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kGateMaxFields = 1024;            // the per-block field sums live in LDS
constexpr int kGateBwdMaxBlocks = kNumCU * 8;   // 8 blocks of 256 threads per CU: 8 waves per SIMD
constexpr int kGateFoldCols = 16;

__device__ __forceinline__ float gate_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

template <int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void gate_emb_fwd_kernel(
    int64_t n, int S, int D, int stride, int64_t N, int64_t pad, const int64_t* __restrict__ ids,
    const float* __restrict__ W, const float* __restrict__ gate_w, float* __restrict__ out, int64_t out_stride,
    int32_t* __restrict__ status) {
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
  const int lg = threadIdx.x % LANES;
  const int d0 = lg * VEC;
  const bool live = i < n && d0 < D;
  float e[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) e[v] = 0.f;
  if (i < n) {
    const int64_t id = ids[i];
    if (id != pad || pad < 0) {
      if (id >= 0 && id < N) {
        if (live) vload<VEC>(e, W + id * stride + d0);
      } else if (lg == 0) {
        atomicOr(status, REC_FLAG_INDEX_OOB);
      }
    }
  }
  float ts = 0.f;
#pragma unroll
  for (int v = 0; v < VEC; ++v) ts += e[v];
  const float t = group_sum<LANES>(ts);
  if (!live) return;
  const int s = (int)(i % S);
  const float a = gate_sigmoid(gate_w[s] * t);
#pragma unroll
  for (int v = 0; v < VEC; ++v) e[v] *= a;
  vstore<VEC>(out + (i / S) * out_stride + (int64_t)s * D + d0, e);
}

// A block takes the chunks blockIdx.x, blockIdx.x + gridDim.x, .. of kBlock / LANES consecutive lookups.  Per chunk the
// group leaders leave d p * t in LDS and thread s adds the entries of field s in lookup order to its running sum; the two
// LDS rows alternate so that one barrier per chunk is enough.
template <int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void gate_emb_bwd_kernel(
    int64_t n, int S, int D, int stride, int64_t N, int64_t pad, const int64_t* __restrict__ ids,
    const float* __restrict__ W, const float* __restrict__ gate_w, float* __restrict__ g, int64_t g_stride,
    float* __restrict__ part, int32_t* __restrict__ status) {
  constexpr int G = kBlock / LANES;
  __shared__ float contrib[2][G];
  __shared__ float acc[kGateMaxFields];
  for (int s = threadIdx.x; s < S; s += kBlock) acc[s] = 0.f;      // thread s is the only one that touches acc[s]
  const int grp = threadIdx.x / LANES, lg = threadIdx.x % LANES;
  const int d0 = lg * VEC;
  const bool col = d0 < D;
  const int64_t chunks = (n + G - 1) / G;
  int buf = 0;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x, buf ^= 1) {
    const int64_t i0 = c * G, i = i0 + grp;
    float e[VEC], gr[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) e[v] = gr[v] = 0.f;
    bool row = false;
    float w = 0.f;
    float* slot = nullptr;
    if (i < n) {
      const int64_t id = ids[i];
      const int s = (int)(i % S);
      slot = g + (i / S) * g_stride + (int64_t)s * D + d0;
      if (id != pad || pad < 0) {
        if (id >= 0 && id < N) {
          row = true;
          w = gate_w[s];
          if (col) {
            vload<VEC>(e, W + id * stride + d0);
            vload<VEC>(gr, slot);
          }
        } else if (lg == 0) {
          atomicOr(status, REC_FLAG_INDEX_OOB);
        }
      }
    }
    float ts = 0.f, ds = 0.f;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      ts += e[v];
      ds += gr[v] * e[v];
    }
    const float t = group_sum<LANES>(ts);
    const float da = group_sum<LANES>(ds);
    const float a = gate_sigmoid(w * t);
    const float dp = da * a * (1.f - a);
    if (i < n && col) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) gr[v] = row ? gr[v] * a + dp * w : 0.f;
      vstore<VEC>(slot, gr);
    }
    if (lg == 0) contrib[buf][grp] = row ? dp * t : 0.f;
    __syncthreads();
    const int first = (int)(i0 % S);
    for (int s = threadIdx.x; s < S; s += kBlock) {
      int j = s - first;
      if (j < 0) j += S;
      float sum = acc[s];
      for (; j < G; j += S) sum += contrib[buf][j];
      acc[s] = sum;
    }
  }
  float* __restrict__ mine = part + (int64_t)blockIdx.x * S;
  for (int s = threadIdx.x; s < S; s += kBlock) mine[s] = acc[s];
}

// d_w[s] = part[0][s] + part[1][s] + ..: 16 groups take every 16th block in order, then the groups add up in order
// (blocks == 0 writes zeros)
__global__ __launch_bounds__(kBlock) void gate_fold_kernel(int blocks, int S, const float* __restrict__ part,
                                                           float* __restrict__ d_w) {
  constexpr int kGroups = kBlock / kGateFoldCols;
  __shared__ float red[kGroups][kGateFoldCols];
  const int ci = threadIdx.x % kGateFoldCols, grp = threadIdx.x / kGateFoldCols;
  const int s = blockIdx.x * kGateFoldCols + ci;
  float sum = 0.f;
  if (s < S)
    for (int p = grp; p < blocks; p += kGroups) sum += part[(int64_t)p * S + s];
  red[grp][ci] = sum;
  __syncthreads();
  if (grp == 0 && s < S) {
    float t = red[0][ci];
    for (int i = 1; i < kGroups; ++i) t += red[i][ci];
    d_w[s] = t;
  }
}

// elementwise over [B, n] with row strides: thread idx owns VEC consecutive columns of one row
template <int VEC>
__global__ __launch_bounds__(kBlock) void gate_hidden_fwd_kernel(int64_t total, int nv, const float* __restrict__ y,
                                                                 int64_t ld_y, float* __restrict__ t, int64_t ld_t,
                                                                 float* __restrict__ x, int64_t ld_x) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx / nv;
  const int c = (int)(idx % nv) * VEC;
  float yv[VEC], tv[VEC], xv[VEC];
  vload<VEC>(yv, y + r * ld_y + c);
  vload<VEC>(tv, t + r * ld_t + c);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    tv[v] = tanhf(tv[v]);
    xv[v] = yv[v] * tv[v];
  }
  vstore<VEC>(t + r * ld_t + c, tv);
  vstore<VEC>(x + r * ld_x + c, xv);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void gate_hidden_bwd_kernel(int64_t total, int nv, const float* __restrict__ u,
                                                                 int64_t ld_u, const float* __restrict__ y, int64_t ld_y,
                                                                 const float* __restrict__ h, int64_t ld_h,
                                                                 float* __restrict__ dt, int64_t ld_dt,
                                                                 float* __restrict__ uh, int64_t ld_uh) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx / nv;
  const int c = (int)(idx % nv) * VEC;
  float uv[VEC], yv[VEC], hv[VEC], a[VEC], b[VEC];
  vload<VEC>(uv, u + r * ld_u + c);
  vload<VEC>(yv, y + r * ld_y + c);
  vload<VEC>(hv, h + r * ld_h + c);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    a[v] = uv[v] * yv[v] * (1.f - hv[v] * hv[v]);
    b[v] = uv[v] * hv[v];
  }
  vstore<VEC>(dt + r * ld_dt + c, a);
  vstore<VEC>(uh + r * ld_uh + c, b);
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void gate_relu_mask_kernel(int64_t total, int nv, float* __restrict__ dy,
                                                                int64_t ld_dy, const float* __restrict__ y,
                                                                int64_t ld_y) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t r = idx / nv;
  const int c = (int)(idx % nv) * VEC;
  float dv[VEC], yv[VEC];
  vload<VEC>(dv, dy + r * ld_dy + c);
  vload<VEC>(yv, y + r * ld_y + c);
#pragma unroll
  for (int v = 0; v < VEC; ++v) dv[v] = yv[v] > 0.f ? dv[v] : 0.f;
  vstore<VEC>(dy + r * ld_dy + c, dv);
}

int gate_emb_check(int64_t n, int32_t S, int32_t D, int32_t row_stride, int64_t N, int64_t ld, const char* ld_name) {
  REC_REQUIRE(n >= 0 && S > 0 && D > 0 && row_stride >= D && N > 0, REC_EINVAL,
              "gate emb: bad sizes (n %lld, num_fields %d, emb_dim %d, row_stride %d, num_rows %lld)", (long long)n, S, D,
              row_stride, (long long)N);
  REC_REQUIRE(n % S == 0, REC_EINVAL, "gate emb: n %lld is not a multiple of num_fields %d", (long long)n, S);
  REC_REQUIRE(ld >= (int64_t)S * D, REC_EINVAL, "gate emb: %s %lld < num_fields * emb_dim = %lld", ld_name, (long long)ld,
              (long long)S * D);
  return REC_OK;
}

bool gate_vec_ok(const void* p, int64_t ld) { return ((uintptr_t)p) % 16 == 0 && ld % 4 == 0; }

int64_t gate_bwd_grid(int64_t n, int lanes) {       // a function of the shape alone: the chunk sets of the partials are fixed
  const int64_t per = kBlock / lanes, chunks = (n + per - 1) / per;
  return chunks < kGateBwdMaxBlocks ? chunks : kGateBwdMaxBlocks;
}

int gate_rows_check(int64_t B, int32_t n, const char* what) {
  REC_REQUIRE(B >= 0 && n > 0, REC_EINVAL, "%s: bad sizes (batch %lld, n %d)", what, (long long)B, n);
  return REC_OK;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_gate_emb_fwd(int64_t n, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                                int64_t padding_idx, const int64_t* ids, const float* W, const float* gate_w,
                                float* out, int64_t out_stride, int32_t* status, void* stream) {
  int rc = gate_emb_check(n, num_fields, emb_dim, row_stride, num_rows, out_stride, "out_stride");
  if (rc != REC_OK) return rc;
  if (n == 0) return REC_OK;
  REC_REQUIRE(ids && W && gate_w && out && status, REC_EINVAL, "null pointer argument");
  // float4 loads and stores need 16-byte aligned rows on both sides: fall back to scalar lanes otherwise
  const bool vec = gate_vec_ok(W, row_stride) && gate_vec_ok(out, out_stride);
  return dispatch_row_shape(emb_dim, vec ? row_stride : row_stride | 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    const int64_t grid = (n * LANES + kBlock - 1) / kBlock;
    REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "n too large");
    hipLaunchKernelGGL((gate_emb_fwd_kernel<VEC, LANES>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, n,
                       num_fields, emb_dim, row_stride, num_rows, padding_idx, ids, W, gate_w, out, out_stride, status);
    return check_launch("rec_gate_emb_fwd");
  });
}

extern "C" int rec_gate_emb_bwd_workspace_bytes(int64_t n, int32_t num_fields, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(n >= 0 && num_fields > 0, REC_EINVAL, "gate emb: bad sizes (n %lld, num_fields %d)", (long long)n,
              num_fields);
  *bytes = (size_t)gate_bwd_grid(n, kWave) * (size_t)num_fields * sizeof(float);  // 64-lane groups: the most blocks
  return REC_OK;
}

extern "C" int rec_gate_emb_bwd(int64_t n, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                                int64_t padding_idx, const int64_t* ids, const float* W, const float* gate_w, float* g,
                                int64_t g_stride, float* d_gate_w, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream) {
  int rc = gate_emb_check(n, num_fields, emb_dim, row_stride, num_rows, g_stride, "g_stride");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(num_fields <= kGateMaxFields, REC_ESHAPE, "gate emb: num_fields %d unsupported (need <= %d)", num_fields,
              kGateMaxFields);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {                                      // an empty batch sum
    if (!d_gate_w) return REC_OK;
    hipLaunchKernelGGL(gate_fold_kernel, dim3((num_fields + kGateFoldCols - 1) / kGateFoldCols), dim3(kBlock), 0, st, 0,
                       num_fields, (const float*)nullptr, d_gate_w);
    return check_launch("rec_gate_emb_bwd (fold)");
  }
  REC_REQUIRE(ids && W && gate_w && g && d_gate_w && status, REC_EINVAL, "null pointer argument");
  {   // the caller is held to the ONE figure of the query (the lane shape with the most blocks), whatever shape runs
    size_t owed = 0;
    rec_gate_emb_bwd_workspace_bytes(n, num_fields, &owed);
    REC_REQUIRE(workspace_bytes >= owed, REC_EWORKSPACE, "gate emb bwd workspace %zu < %zu bytes", workspace_bytes, owed);
    REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
  }
  const bool vec = gate_vec_ok(W, row_stride) && gate_vec_ok(g, g_stride);
  float* part = (float*)workspace;
  int grid = 0;
  rc = dispatch_row_shape(emb_dim, vec ? row_stride : row_stride | 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    grid = (int)gate_bwd_grid(n, LANES);
    const size_t need = (size_t)grid * (size_t)num_fields * sizeof(float);
    REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "gate emb bwd workspace %zu < %zu bytes", workspace_bytes, need);
    hipLaunchKernelGGL((gate_emb_bwd_kernel<VEC, LANES>), dim3((unsigned)grid), dim3(kBlock), 0, st, n, num_fields,
                       emb_dim, row_stride, num_rows, padding_idx, ids, W, gate_w, g, g_stride, part, status);
    return check_launch("rec_gate_emb_bwd");
  });
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(gate_fold_kernel, dim3((num_fields + kGateFoldCols - 1) / kGateFoldCols), dim3(kBlock), 0, st, grid,
                     num_fields, part, d_gate_w);
  return check_launch("rec_gate_emb_bwd (fold)");
}

#define REC_GATE_ROWS(kernel, what, vec, ...)                                                                          \
  do {                                                                                                                 \
    const int nv = (vec) ? n / 4 : n;                                                                                  \
    const int64_t total = batch * nv, grid = (total + kBlock - 1) / kBlock;                                            \
    REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "%s: batch too large", what);                                          \
    if (vec)                                                                                                           \
      hipLaunchKernelGGL((kernel<4>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, total, nv, __VA_ARGS__); \
    else                                                                                                               \
      hipLaunchKernelGGL((kernel<1>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, total, nv, __VA_ARGS__); \
    return check_launch(what);                                                                                         \
  } while (0)

extern "C" int rec_gate_hidden_fwd(int64_t batch, int32_t n, const float* y, int64_t ld_y, float* t, int64_t ld_t,
                                   float* x, int64_t ld_x, void* stream) {
  int rc = gate_rows_check(batch, n, "rec_gate_hidden_fwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(ld_y >= n && ld_t >= n && ld_x >= n, REC_EINVAL, "rec_gate_hidden_fwd: a row stride is below n %d", n);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(y && t && x, REC_EINVAL, "null pointer argument");
  const bool vec = n % 4 == 0 && gate_vec_ok(y, ld_y) && gate_vec_ok(t, ld_t) && gate_vec_ok(x, ld_x);
  REC_GATE_ROWS(gate_hidden_fwd_kernel, "rec_gate_hidden_fwd", vec, y, ld_y, t, ld_t, x, ld_x);
}

extern "C" int rec_gate_hidden_bwd(int64_t batch, int32_t n, const float* u, int64_t ld_u, const float* y, int64_t ld_y,
                                   const float* h, int64_t ld_h, float* dt, int64_t ld_dt, float* uh, int64_t ld_uh,
                                   void* stream) {
  int rc = gate_rows_check(batch, n, "rec_gate_hidden_bwd");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(ld_u >= n && ld_y >= n && ld_h >= n && ld_dt >= n && ld_uh >= n, REC_EINVAL,
              "rec_gate_hidden_bwd: a row stride is below n %d", n);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(u && y && h && dt && uh, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(dt != u && dt != y && dt != h && uh != u && uh != y && uh != h && dt != uh, REC_EINVAL,
              "rec_gate_hidden_bwd: the outputs must not alias an input or each other");
  const bool vec = n % 4 == 0 && gate_vec_ok(u, ld_u) && gate_vec_ok(y, ld_y) && gate_vec_ok(h, ld_h) &&
                   gate_vec_ok(dt, ld_dt) && gate_vec_ok(uh, ld_uh);
  REC_GATE_ROWS(gate_hidden_bwd_kernel, "rec_gate_hidden_bwd", vec, u, ld_u, y, ld_y, h, ld_h, dt, ld_dt, uh, ld_uh);
}

extern "C" int rec_relu_mask_inplace(int64_t batch, int32_t n, float* dy, int64_t ld_dy, const float* y, int64_t ld_y,
                                     void* stream) {
  int rc = gate_rows_check(batch, n, "rec_relu_mask_inplace");
  if (rc != REC_OK) return rc;
  REC_REQUIRE(ld_dy >= n && ld_y >= n, REC_EINVAL, "rec_relu_mask_inplace: a row stride is below n %d", n);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(dy && y, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(dy != y, REC_EINVAL, "rec_relu_mask_inplace: dy must not be y");
  const bool vec = n % 4 == 0 && gate_vec_ok(dy, ld_dy) && gate_vec_ok(y, ld_y);
  REC_GATE_ROWS(gate_relu_mask_kernel, "rec_relu_mask_inplace", vec, dy, ld_dy, y, ld_y);
}
#undef REC_GATE_ROWS
