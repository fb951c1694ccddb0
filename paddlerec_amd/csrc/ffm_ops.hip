// Field-aware factorisation machine (models/rank/ffm/net.py:76-133): first-order term + the field-aware pairwise
// interaction  y2[b] = sum_{i<j} <E[i, j, :], E[j, i, :]>  over the per-sample feature cube E [F, F, D], whose field f
// is the R = F*D wide row W[id_f] (f < S) or dense[b, f-S] * dense_w[f-S, :] (f >= S), and its backward.
//
// Every element E[i, j, :] (i != j) is read exactly once by the forward, and the partner of a contiguous run of row i
// is a D-float piece of another row.  The fast path therefore gathers a sample's S table rows once, coalesced, into an
// LDS image of the cube and pairs there; the LDS pitch P satisfies P = D (mod 32), so the transposed piece reads of a
// wave, E[j*P + i*D + d] over consecutive c = j*D + d, fall on consecutive banks.  Cubes larger than kFfmLdsMax (D 16 at
// F 39: 97 KB) take the same code with the partners read from the table itself (through L2).  The dense rows are
// products computed where they are needed; they are never stored outside LDS.
#include "ffm_cube.h"

namespace rec {
namespace {

template <bool LDS>
__global__ __launch_bounds__(kBlock) void ffm_fwd_kernel(FfmArgs a, float* __restrict__ y1, float* __restrict__ y2) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  __shared__ float red[kBlock / kWave + 2];
  const int64_t chunk = (a.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    ffm_rows(a, b, rows);
    for (int k = threadIdx.x; k < a.Dn; k += kBlock) dval[k] = a.dense[b * a.Dn + k];
    __syncthreads();
    if constexpr (LDS) {
      ffm_stage(a, b, rows, img);
      __syncthreads();
    }
    // first order (wave 0): sum_s W1[id_s] + sum_k dense_k * dense_w_one[k]          net.py:101-108
    if (threadIdx.x < kWave) {
      const int l = threadIdx.x;
      float s1 = 0.f, s2 = 0.f;
      if (l < a.S && rows[l] >= 0) s1 = a.W1[rows[l]];
      if (l < a.Dn) s2 = dval[l] * a.dense_w_one[l];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, kWave);
        s2 += __shfl_xor(s2, o, kWave);
      }
      if (l == 0) red[kBlock / kWave] = s1 + s2;
    }
    // field-aware second order: row i against the partner pieces of its columns j > i      net.py:121-132
    float acc = 0.f;
    for (int i = 0; i + 1 < a.F; ++i) {
      for (int c = (i + 1) * a.D + threadIdx.x; c < a.R; c += kBlock) {
        const int j = c / a.D, d = c - j * a.D;
        acc += ffm_e<LDS>(a, img, rows, dval, i, c) * ffm_e<LDS>(a, img, rows, dval, j, i * a.D + d);
      }
    }
    const float s = ffm_block_sum(acc, red);
    if (threadIdx.x == 0) {
      y1[b] = red[kBlock / kWave];
      y2[b] = s;
    }
    __syncthreads();                           // rows / dval / img / red are rewritten by the next sample
  }
}

// Backward.  dE[i, j, :] = dz * E[j, i, :] (j != i), dE[i, i, :] = 0.  Sparse field i < S: row_grad[b*S + i, c] =
// dE[i][c] for c < R, 0 on the pad columns [R, grad_stride).  Dense field k: d dense_w[k, c] += dense[b,k] * dE[S+k][c];
// d dense_w_one[k] += dz * dense[b,k].  Both batch sums are per-block partials over a fixed sample range (registers on
// the fast path, the block's own workspace slice otherwise), folded in block order by ffm_fold_kernel.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void ffm_bwd_kernel(FfmArgs a, const float* __restrict__ dz,
                                                         float* __restrict__ row_grad, float* __restrict__ part) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  const int DnR = a.Dn * a.R;
  float* __restrict__ mine = part + (int64_t)blockIdx.x * (DnR + a.Dn);
  float acc[kFfmAccRegs];
  float acc1 = 0.f;
  if constexpr (LDS) {
#pragma unroll
    for (int r = 0; r < kFfmAccRegs; ++r) acc[r] = 0.f;
  } else {
    for (int e = threadIdx.x; e < DnR; e += kBlock) mine[e] = 0.f;
  }
  const bool v4 = a.gstride % 4 == 0 && ((uintptr_t)row_grad) % 16 == 0;
  const int64_t chunk = (a.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    ffm_rows(a, b, rows);
    for (int k = threadIdx.x; k < a.Dn; k += kBlock) dval[k] = a.dense[b * a.Dn + k];
    __syncthreads();
    if constexpr (LDS) {
      ffm_stage(a, b, rows, img);
      __syncthreads();
    }
    const float g = dz[b];
    auto de = [&](int i, int c) -> float {     // dE[i][c]
      if (c >= a.R) return 0.f;
      const int j = c / a.D, d = c - j * a.D;
      return j == i ? 0.f : g * ffm_e<LDS>(a, img, rows, dval, j, i * a.D + d);
    };
    float* __restrict__ out = row_grad + b * a.S * (int64_t)a.gstride;
    if (v4) {
      const int G4 = a.gstride >> 2, n = a.S * G4;
      for (int q = threadIdx.x; q < n; q += kBlock) {
        const int i = q / G4, c = (q - i * G4) * 4;
        const float t[4] = {de(i, c), de(i, c + 1), de(i, c + 2), de(i, c + 3)};
        vstore_nt<4>(out + (int64_t)i * a.gstride + c, t);
      }
    } else {
      const int n = a.S * a.gstride;
      for (int q = threadIdx.x; q < n; q += kBlock) {
        const int i = q / a.gstride, c = q - i * a.gstride;
        __builtin_nontemporal_store(de(i, c), out + q);
      }
    }
    if constexpr (LDS) {
#pragma unroll
      for (int r = 0; r < kFfmAccRegs; ++r) {
        const int e = threadIdx.x + r * kBlock;
        if (e < DnR) {
          const int k = e / a.R;
          acc[r] += dval[k] * de(a.S + k, e - k * a.R);
        }
      }
    } else {
      for (int e = threadIdx.x; e < DnR; e += kBlock) {
        const int k = e / a.R;
        mine[e] += dval[k] * de(a.S + k, e - k * a.R);
      }
    }
    if (threadIdx.x < a.Dn) acc1 += g * dval[threadIdx.x];
    __syncthreads();
  }
  if constexpr (LDS) {
#pragma unroll
    for (int r = 0; r < kFfmAccRegs; ++r) {
      const int e = threadIdx.x + r * kBlock;
      if (e < DnR) mine[e] = acc[r];
    }
  }
  if (threadIdx.x < a.Dn) mine[DnR + threadIdx.x] = acc1;
}

__global__ __launch_bounds__(kBlock) void ffm_fold_kernel(int grid, int DnR, int Dn, const float* __restrict__ part,
                                                          float* __restrict__ d_dense_w,
                                                          float* __restrict__ d_dense_w_one) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  const int W = DnR + Dn;
  if (e >= W) return;
  float s = 0.f;
  for (int g = 0; g < grid; ++g) s += part[(int64_t)g * W + e];
  if (e < DnR) d_dense_w[e] = s;
  else d_dense_w_one[e - DnR] = s;
}

int ffm_check(const rec_ffm_desc* d) {
  REC_REQUIRE(d, REC_EINVAL, "null desc");
  REC_REQUIRE(d->batch >= 0 && d->num_rows >= 1 && d->num_slots >= 1 && d->num_dense >= 0 && d->dim >= 1, REC_EINVAL,
              "bad sizes");
  const int F = d->num_slots + d->num_dense;
  REC_REQUIRE(F <= kFfmMaxFields && d->dim <= kFfmMaxDim, REC_ESHAPE,
              "ffm: %d fields x dim %d unsupported (need fields <= %d, dim <= %d)", F, d->dim, kFfmMaxFields,
              kFfmMaxDim);
  const int R = F * d->dim;
  REC_REQUIRE(d->row_stride >= R, REC_EINVAL, "row_stride %d < fields x dim %d", d->row_stride, R);
  return REC_OK;
}

FfmArgs ffm_args(const rec_ffm_desc* d, const int64_t* ids, const float* dense, const float* W, const float* W1,
                 const float* dense_w, const float* dense_w_one, int32_t* status) {
  FfmArgs a;
  a.B = d->batch; a.N = d->num_rows;
  a.S = d->num_slots; a.Dn = d->num_dense; a.D = d->dim; a.F = a.S + a.Dn; a.R = a.F * a.D;
  a.stride = d->row_stride; a.gstride = d->grad_stride; a.P = ffm_pitch(a.R, a.D);
  a.wvec = a.stride % 4 == 0 && ((uintptr_t)W) % 16 == 0;
  a.ids = ids; a.dense = dense; a.W = W; a.W1 = W1; a.dense_w = dense_w; a.dense_w_one = dense_w_one;
  a.status = status;
  return a;
}

size_t ffm_lds_bytes(const FfmArgs& a) { return (size_t)a.F * a.P * sizeof(float); }

int ffm_grid(int64_t B) { return (int)(B < kFfmGrid ? B : kFfmGrid); }

template <class K>
void ffm_allow_lds(K kern) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFfmLdsMax);
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_ffm_fwd(const rec_ffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                           const float* W1, const float* dense_w, const float* dense_w_one, float* y1, float* y2,
                           int32_t* status, void* stream) {
  int rc = ffm_check(desc);
  if (rc != REC_OK) return rc;
  if (desc->batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && W1 && y1 && y2 && (desc->num_dense == 0 || (dense && dense_w && dense_w_one)), REC_EINVAL,
              "null pointer argument");
  const FfmArgs a = ffm_args(desc, ids, dense, W, W1, dense_w, dense_w_one, status);
  const int grid = ffm_grid(a.B);
  const size_t lds = ffm_lds_bytes(a);
  hipStream_t st = (hipStream_t)stream;
  if (lds <= kFfmLdsMax) {
    static const bool once = (ffm_allow_lds(ffm_fwd_kernel<true>), true);
    (void)once;
    hipLaunchKernelGGL(ffm_fwd_kernel<true>, dim3(grid), dim3(kBlock), lds, st, a, y1, y2);
  } else {
    hipLaunchKernelGGL(ffm_fwd_kernel<false>, dim3(grid), dim3(kBlock), 0, st, a, y1, y2);
  }
  return check_launch("rec_ffm_fwd");
}

extern "C" int rec_ffm_bwd_workspace_bytes(const rec_ffm_desc* desc, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = ffm_check(desc);
  if (rc != REC_OK) return rc;
  const int64_t R = (int64_t)(desc->num_slots + desc->num_dense) * desc->dim;
  *bytes = (size_t)ffm_grid(desc->batch) * (size_t)(desc->num_dense * R + desc->num_dense) * sizeof(float);
  return REC_OK;
}

extern "C" int rec_ffm_bwd(const rec_ffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                           const float* dense_w, const float* dz, float* row_grad, float* d_dense_w,
                           float* d_dense_w_one, void* workspace, size_t workspace_bytes, int32_t* status,
                           void* stream) {
  int rc = ffm_check(desc);
  if (rc != REC_OK) return rc;
  const int R = (desc->num_slots + desc->num_dense) * desc->dim;
  REC_REQUIRE(desc->grad_stride >= R, REC_EINVAL, "grad_stride %d < fields x dim %d", desc->grad_stride, R);
  size_t need = 0;
  rec_ffm_bwd_workspace_bytes(desc, &need);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "ffm bwd workspace %zu < %zu bytes", workspace_bytes, need);
  if (desc->batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && dz && row_grad && (desc->num_dense == 0 || (dense && dense_w && d_dense_w &&
              d_dense_w_one && workspace)), REC_EINVAL, "null pointer argument");
  const FfmArgs a = ffm_args(desc, ids, dense, W, nullptr, dense_w, nullptr, status);
  const int grid = ffm_grid(a.B);
  const size_t lds = ffm_lds_bytes(a);
  const int DnR = a.Dn * a.R;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (lds <= kFfmLdsMax && DnR <= kFfmAccRegs * kBlock) {
    static const bool once = (ffm_allow_lds(ffm_bwd_kernel<true>), true);
    (void)once;
    hipLaunchKernelGGL(ffm_bwd_kernel<true>, dim3(grid), dim3(kBlock), lds, st, a, dz, row_grad, part);
  } else {
    hipLaunchKernelGGL(ffm_bwd_kernel<false>, dim3(grid), dim3(kBlock), 0, st, a, dz, row_grad, part);
  }
  rc = check_launch("rec_ffm_bwd");
  if (rc != REC_OK || a.Dn == 0) return rc;
  hipLaunchKernelGGL(ffm_fold_kernel, dim3((DnR + a.Dn + kBlock - 1) / kBlock), dim3(kBlock), 0, st, grid, DnR, a.Dn,
                     part, d_dense_w, d_dense_w_one);
  return check_launch("rec_ffm_bwd (fold)");
}
