// Deep & Cross, the vector-form cross network (models/rank/dcn/net.py:117-135): L layers that share ONE weight w [d]
// and ONE bias b [d],
//     s_l = <x_l, w>            x_{l+1} = x_0 * s_l + b + x_l            l2 += sum (x_l * w)^2
// and their backward, each as one pass over the rows.  A layer is a dot product and an axpy per row, so the whole stack
// needs x_0, w, b and L scalars: one 64-lane wave owns a row, keeps x_0, the running x_l, w and b in registers (4 floats
// per lane at d <= 256, 8 at d <= 512), reduces the dot product across its lanes and never touches LDS or scratch for the
// rows.  The forward streams x_0 in and x_L out; the backward streams x_0 and dL/dx_L in and dL/dx_0 out and rebuilds
// x_l = x_0 * (1 + s_0 + .. + s_{l-1}) + l * b from the saved scalars.
//
// Column layout of a lane's registers.  Vector form (row base addresses and strides multiples of 16 bytes): register
// (j, e) of lane i is column (j * 64 + i) * 4 + e, one 16-byte access per j.  Scalar form (anything else, e.g. rows
// of 247 floats back to back): column (j * 4 + e) * 64 + i, 64 consecutive floats per wave access.  Columns >= d are
// never read or written and hold 0 in registers, so they drop out of every sum.
//
// d_w / d_b are batch sums: every wave accumulates its rows (a fixed set: row = wave + k * waves) in registers, the waves
// of a block add up in wave order through LDS, and dcn_fold_kernel adds the blocks' partials in block order.
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kDcnMaxD = 512;
constexpr int kDcnMaxLayers = kWave;           // the saved scalars of a row sit one per lane
constexpr int kDcnFwdBlock = 256;              // 4 rows in flight per block
constexpr int kDcnFwdGrid = 8 * kNumCU;        // 8 blocks per CU = 8 waves per SIMD: the grid-stride loop covers more rows
// The backward writes ONE d_w / d_b partial per block, so its blocks are large.  d <= 256 (4 floats per lane): 768
// threads = 12 rows in flight, 2 blocks per CU = 6 waves per SIMD (80 VGPRs); d <= 512 (8 floats per lane): 1024
// threads = 16 rows, 1 block per CU = 4 waves per SIMD (128 VGPRs).
constexpr int dcn_bwd_block(int nv) { return nv == 1 ? 768 : 1024; }
constexpr int dcn_bwd_waves_per_simd(int nv) { return nv == 1 ? 6 : 4; }
constexpr int kDcnFoldCols = 16;               // dcn_fold_kernel: 16 columns x 16 partial groups per 256-thread block

struct DcnArgs {
  int64_t B;
  int d, L;
  int64_t ld_x0, ld_out, ld_dxl, ld_dx0;
  float coeff;
  bool accumulate;
};

template <int NV, bool VEC>
__device__ __forceinline__ int dcn_col(int j, int e, int lane) {
  return VEC ? (j * kWave + lane) * 4 + e : (j * 4 + e) * kWave + lane;
}

// w / b / u: tiny, L2-resident, of unknown alignment — element loads in the lane's column layout, once per wave
template <int NV, bool VEC>
__device__ __forceinline__ void dcn_load_param(float (&r)[4 * NV], const float* __restrict__ p, int d, int lane) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = dcn_col<NV, VEC>(j, e, lane);
      r[j * 4 + e] = c < d ? p[c] : 0.f;
    }
}

template <int NV, bool VEC>
__device__ __forceinline__ void dcn_load_row(float (&r)[4 * NV], const float* __restrict__ p, int d, int lane) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = dcn_col<NV, VEC>(j, 0, lane);
    if (VEC && c0 + 3 < d) {
      float t[4];
      vload<4>(t, p + c0);
#pragma unroll
      for (int e = 0; e < 4; ++e) r[j * 4 + e] = t[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = dcn_col<NV, VEC>(j, e, lane);
        r[j * 4 + e] = c < d ? p[c] : 0.f;
      }
    }
  }
}

template <int NV, bool VEC>
__device__ __forceinline__ void dcn_store_row(float* __restrict__ p, const float (&r)[4 * NV], int d, int lane) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c0 = dcn_col<NV, VEC>(j, 0, lane);
    if (VEC && c0 + 3 < d) {
      const float t[4] = {r[j * 4], r[j * 4 + 1], r[j * 4 + 2], r[j * 4 + 3]};
      vstore<4>(p + c0, t);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = dcn_col<NV, VEC>(j, e, lane);
        if (c < d) p[c] = r[j * 4 + e];
      }
    }
  }
}

template <int NV, bool VEC>
__global__ __launch_bounds__(kDcnFwdBlock) void dcn_cross_fwd_kernel(DcnArgs a, const float* __restrict__ X0,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ b, float* __restrict__ XL,
                                                                     float* __restrict__ saved,
                                                                     float* __restrict__ l2_part) {
  constexpr int E = 4 * NV;
  constexpr int kWaves = kDcnFwdBlock / kWave;
  __shared__ float red[kWaves];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  float wr[E], br[E];
  dcn_load_param<NV, VEC>(wr, w, a.d, lane);
  dcn_load_param<NV, VEC>(br, b, a.d, lane);
  const bool want_l2 = l2_part != nullptr;
  float l2 = 0.f;
  const int64_t step = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.B; r += step) {
    float x0[E], x[E];
    dcn_load_row<NV, VEC>(x0, X0 + r * a.ld_x0, a.d, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) x[e] = x0[e];
    for (int l = 0; l < a.L; ++l) {
      float p = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float xw = x[e] * wr[e];                      // net.py:118 input_w
        p += xw;
        if (want_l2) l2 += xw * xw;                         // net.py:137-138 _l2_loss
      }
      const float s = group_sum<kWave>(p);                  // net.py:119 input_w1
      if (saved && lane == 0) saved[r * a.L + l] = s;
#pragma unroll
      for (int e = 0; e < E; ++e) x[e] = (x0[e] * s + br[e]) + x[e];   // net.py:121-124
    }
    dcn_store_row<NV, VEC>(XL + r * a.ld_out, x, a.d, lane);
  }
  if (want_l2) {                                            // fixed order: lanes (butterfly), waves, then the blocks
    l2 = group_sum<kWave>(l2);
    if (lane == 0) red[wave] = l2;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = red[0];
      for (int i = 1; i < kWaves; ++i) s += red[i];
      l2_part[blockIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(kBlock) void dcn_l2_fold_kernel(int n, float coeff, const float* __restrict__ part,
                                                             float* __restrict__ out) {
  __shared__ float red[kBlock];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kBlock) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = coeff * red[0];
}

// RANK1: the upstream gradient is dz[r] * u[k] (u in registers) instead of a [B, d] matrix
template <int NV, bool VEC, bool RANK1>
__global__ __launch_bounds__(dcn_bwd_block(NV), dcn_bwd_waves_per_simd(NV)) void dcn_cross_bwd_kernel(DcnArgs a, const float* __restrict__ X0,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ b,
                                                                     const float* __restrict__ saved,
                                                                     const float* __restrict__ dXL,
                                                                     const float* __restrict__ dz,
                                                                     const float* __restrict__ u, float* __restrict__ dX0,
                                                                     float* __restrict__ part) {
  constexpr int E = 4 * NV;
  constexpr int kWaves = dcn_bwd_block(NV) / kWave;
  __shared__ float red[2][kDcnMaxD];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  float wr[E], br[E], ur[RANK1 ? E : 1], dw[E], db[E];
  dcn_load_param<NV, VEC>(wr, w, a.d, lane);
  dcn_load_param<NV, VEC>(br, b, a.d, lane);
  if constexpr (RANK1) dcn_load_param<NV, VEC>(ur, u, a.d, lane);
#pragma unroll
  for (int e = 0; e < E; ++e) dw[e] = db[e] = 0.f;
  const float c2 = 2.f * a.coeff;
  const int64_t step = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.B; r += step) {
    float x0[E], g[E], acc[E];
    dcn_load_row<NV, VEC>(x0, X0 + r * a.ld_x0, a.d, lane);
    if constexpr (RANK1) {
      const float z = dz[r];
#pragma unroll
      for (int e = 0; e < E; ++e) g[e] = z * ur[e];
    } else {
      dcn_load_row<NV, VEC>(g, dXL + r * a.ld_dxl, a.d, lane);
    }
    // lane l holds s_l; pre = s_0 + .. + s_{l-1} (shuffle scan, additions only), so x_l = x_0 * (1 + pre_l) + l * b
    const float sv = lane < a.L ? saved[r * a.L + lane] : 0.f;
    float inc = sv;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const float t = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += t;
    }
    float pre = __shfl_up(inc, 1, kWave);
    if (lane == 0) pre = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    for (int l = a.L - 1; l >= 0; --l) {
      const float s = __shfl(sv, l, kWave);
      const float A = 1.f + __shfl(pre, l, kWave);
      const float fl = (float)l;
      float p = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) p += g[e] * x0[e];
      const float t = group_sum<kWave>(p);                  // dL / d s_l
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float xl = x0[e] * A + fl * br[e];
        const float xw = xl * wr[e];
        acc[e] += g[e] * s;                                 // x_0's own factor in x_0 * s_l
        db[e] += g[e];
        dw[e] += t * xl + c2 * xw * xl;                     // s_l = <x_l, w>; l2: d/dw (x_l w)^2
        g[e] += t * wr[e] + c2 * xw * wr[e];                // dL / d x_l
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] += g[e];             // x_0 is also the stack's first input
    float* __restrict__ o = dX0 + r * a.ld_dx0;
    if (a.accumulate) {
      float old[E];
      dcn_load_row<NV, VEC>(old, o, a.d, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] += old[e];
    }
    dcn_store_row<NV, VEC>(o, acc, a.d, lane);
  }
  // the block's partial: the waves add up in wave order
  for (int wv = 0; wv < kWaves; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = dcn_col<NV, VEC>(j, e, lane);
          red[0][c] = wv == 0 ? dw[j * 4 + e] : red[0][c] + dw[j * 4 + e];
          red[1][c] = wv == 0 ? db[j * 4 + e] : red[1][c] + db[j * 4 + e];
        }
    }
    __syncthreads();
  }
  float* __restrict__ mine = part + (int64_t)blockIdx.x * 2 * a.d;
  for (int c = threadIdx.x; c < a.d; c += dcn_bwd_block(NV)) {
    mine[c] = red[0][c];
    mine[a.d + c] = red[1][c];
  }
}

// out[c] = part[0][c] + part[1][c] + ..: 16 groups take every 16th block in order, then the groups add up in order
__global__ __launch_bounds__(kBlock) void dcn_fold_kernel(int blocks, int d, const float* __restrict__ part,
                                                          float* __restrict__ d_w, float* __restrict__ d_b) {
  constexpr int kGroups = kBlock / kDcnFoldCols;
  __shared__ float red[kGroups][kDcnFoldCols];
  const int ci = threadIdx.x % kDcnFoldCols, grp = threadIdx.x / kDcnFoldCols;
  const int c = blockIdx.x * kDcnFoldCols + ci;
  const int W = 2 * d;
  float s = 0.f;
  if (c < W)
    for (int p = grp; p < blocks; p += kGroups) s += part[(int64_t)p * W + c];
  red[grp][ci] = s;
  __syncthreads();
  if (grp == 0 && c < W) {
    float t = red[0][ci];
    for (int i = 1; i < kGroups; ++i) t += red[i][ci];
    if (c < d) d_w[c] = t;
    else d_b[c - d] = t;
  }
}

int dcn_check(const rec_dcn_cross_desc* d) {
  REC_REQUIRE(d, REC_EINVAL, "null desc");
  REC_REQUIRE(d->batch >= 0, REC_EINVAL, "dcn cross: bad sizes (batch %lld)", (long long)d->batch);
  REC_REQUIRE(d->d >= 1 && d->d <= kDcnMaxD, REC_EINVAL, "dcn cross: d %d unsupported (need 1 <= d <= %d)", d->d, kDcnMaxD);
  REC_REQUIRE(d->num_layers >= 1 && d->num_layers <= kDcnMaxLayers, REC_EINVAL,
              "dcn cross: %d layers unsupported (need 1 <= num_layers <= %d)", d->num_layers, kDcnMaxLayers);
  REC_REQUIRE(d->ld_x0 >= d->d, REC_EINVAL, "dcn cross: row stride ld_x0 %lld < d %d", (long long)d->ld_x0, d->d);
  REC_REQUIRE(d->l2_coeff == d->l2_coeff && d->l2_coeff >= 0.f, REC_EINVAL, "dcn cross: l2_coeff must be >= 0");
  return REC_OK;
}

int dcn_fwd_grid(int64_t B) {
  const int64_t waves = kDcnFwdBlock / kWave, g = (B + waves - 1) / waves;
  return (int)(g < kDcnFwdGrid ? g : kDcnFwdGrid);
}

int dcn_bwd_grid(int64_t B, int d) {          // a function of the shape alone: the row sets of the partials are fixed
  const int nv = d <= 4 * kWave ? 1 : 2;
  const int64_t waves = dcn_bwd_block(nv) / kWave, g = (B + waves - 1) / waves;
  const int64_t resident = (int64_t)kNumCU * dcn_bwd_waves_per_simd(nv) * 4 / waves;
  return (int)(g < resident ? g : resident);
}

DcnArgs dcn_args(const rec_dcn_cross_desc* d) {
  DcnArgs a;
  a.B = d->batch; a.d = d->d; a.L = d->num_layers;
  a.ld_x0 = d->ld_x0; a.ld_out = d->ld_out; a.ld_dxl = d->ld_dxl; a.ld_dx0 = d->ld_dx0;
  a.coeff = d->l2_coeff; a.accumulate = d->accumulate_dx0 != 0;
  return a;
}

bool dcn_vec_ok(const void* p, int64_t ld) { return ((uintptr_t)p) % 16 == 0 && ld % 4 == 0; }

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_dcn_cross_bwd_workspace_bytes(const rec_dcn_cross_desc* desc, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = dcn_check(desc);
  if (rc != REC_OK) return rc;
  const size_t bwd = (size_t)dcn_bwd_grid(desc->batch, desc->d) * 2 * (size_t)desc->d * sizeof(float);
  const size_t fwd = (size_t)dcn_fwd_grid(desc->batch) * sizeof(float);
  *bytes = bwd > fwd ? bwd : fwd;
  return REC_OK;
}

extern "C" int rec_dcn_cross_fwd(const rec_dcn_cross_desc* desc, const float* X0, const float* w, const float* b,
                                 float* XL, float* saved, float* l2_out, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  int rc = dcn_check(desc);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(desc->ld_out >= desc->d, REC_EINVAL, "dcn cross: row stride ld_out %lld < d %d", (long long)desc->ld_out,
              desc->d);
  const int grid = dcn_fwd_grid(desc->batch);
  if (l2_out) {
    size_t need = 0;                                  // the ONE figure of the query, as the backward: a caller sizes once
    rec_dcn_cross_bwd_workspace_bytes(desc, &need);
    REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE,
                "dcn cross fwd workspace %zu < %zu bytes", workspace_bytes, need);
    REC_REQUIRE(workspace || need == 0, REC_EINVAL, "null pointer argument");
  }
  if (desc->batch == 0) return REC_OK;
  hipStream_t st = (hipStream_t)stream;
  REC_REQUIRE(X0 && w && b && XL, REC_EINVAL, "null pointer argument");
  const DcnArgs a = dcn_args(desc);
  float* part = l2_out ? (float*)workspace : nullptr;
  const bool vec = dcn_vec_ok(X0, a.ld_x0) && dcn_vec_ok(XL, a.ld_out);
#define REC_DCN_FWD(NV, VEC)                                                                                           \
  hipLaunchKernelGGL((dcn_cross_fwd_kernel<NV, VEC>), dim3(grid), dim3(kDcnFwdBlock), 0, st, a, X0, w, b, XL, saved, part)
  if (a.d <= 4 * kWave) {
    if (vec) REC_DCN_FWD(1, true);
    else REC_DCN_FWD(1, false);
  } else {
    if (vec) REC_DCN_FWD(2, true);
    else REC_DCN_FWD(2, false);
  }
#undef REC_DCN_FWD
  rc = check_launch("rec_dcn_cross_fwd");
  if (rc != REC_OK || !l2_out) return rc;
  hipLaunchKernelGGL(dcn_l2_fold_kernel, dim3(1), dim3(kBlock), 0, st, grid, a.coeff, part, l2_out);
  return check_launch("rec_dcn_cross_fwd (l2 fold)");
}

extern "C" int rec_dcn_cross_bwd(const rec_dcn_cross_desc* desc, const float* X0, const float* w, const float* b,
                                 const float* saved, const float* dXL, const float* dz, const float* u, float* dX0,
                                 float* d_w, float* d_b, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = dcn_check(desc);
  if (rc != REC_OK) return rc;
  const bool rank1 = dXL == nullptr && dz != nullptr && u != nullptr;
  REC_REQUIRE(desc->ld_dx0 >= desc->d, REC_EINVAL, "dcn cross: row stride ld_dx0 %lld < d %d", (long long)desc->ld_dx0,
              desc->d);
  REC_REQUIRE(rank1 || desc->ld_dxl >= desc->d, REC_EINVAL, "dcn cross: row stride ld_dxl %lld < d %d",
              (long long)desc->ld_dxl, desc->d);
  const int grid = dcn_bwd_grid(desc->batch, desc->d);
  size_t need = 0;                                    // the query's figure (it also covers the forward's partials)
  rec_dcn_cross_bwd_workspace_bytes(desc, &need);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE,
              "dcn cross bwd workspace %zu < %zu bytes", workspace_bytes, need);
  REC_REQUIRE(workspace || need == 0, REC_EINVAL, "null pointer argument");
  if (desc->batch == 0) return REC_OK;
  hipStream_t st = (hipStream_t)stream;
  REC_REQUIRE(X0 && w && b && saved && (dXL || rank1) && dX0 && d_w && d_b, REC_EINVAL,
              "null pointer argument");
  const DcnArgs a = dcn_args(desc);
  float* part = (float*)workspace;
  const bool vec = dcn_vec_ok(X0, a.ld_x0) && dcn_vec_ok(dX0, a.ld_dx0) && (rank1 || dcn_vec_ok(dXL, a.ld_dxl));
#define REC_DCN_BWD(NV, VEC, R1)                                                                                       \
  hipLaunchKernelGGL((dcn_cross_bwd_kernel<NV, VEC, R1>), dim3(grid), dim3(dcn_bwd_block(NV)), 0, st, a, X0, w, b, saved,   \
                     dXL, dz, u, dX0, part)
#define REC_DCN_BWD_R1(NV, VEC) \
  if (rank1) REC_DCN_BWD(NV, VEC, true); else REC_DCN_BWD(NV, VEC, false)
  if (a.d <= 4 * kWave) {
    if (vec) { REC_DCN_BWD_R1(1, true); } else { REC_DCN_BWD_R1(1, false); }
  } else {
    if (vec) { REC_DCN_BWD_R1(2, true); } else { REC_DCN_BWD_R1(2, false); }
  }
#undef REC_DCN_BWD_R1
#undef REC_DCN_BWD
  rc = check_launch("rec_dcn_cross_bwd");
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(dcn_fold_kernel, dim3((2 * a.d + kDcnFoldCols - 1) / kDcnFoldCols), dim3(kBlock), 0, st, grid, a.d,
                     part, d_w, d_b);
  return check_launch("rec_dcn_cross_bwd (fold)");
}
