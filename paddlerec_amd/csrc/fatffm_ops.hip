// FAT-DeepFFM (models/rank/fat_deepffm/net.py): the CENet attention over the F*F slices of the per-sample feature cube
// E [F, F, D] (csrc/ffm_cube.h) and the attention-scaled field-pair Hadamard features that feed the DNN.  With
// q = i*F + j, q' = j*F + i and p the index of the pair (i < j) in nested-loop order:
//   pooled[q]    = max_d E[q, d]                                        AdaptiveMaxPool1D(1), net.py:126
//   a            = relu(relu(pooled @ W_red + b_red) @ W_add + b_add)   two GEMMs of the caller, net.py:98-103
//   y1           = sum_q a[q] * sum_d E[q, d]                            net.py:221-222 (the diagonal slices included)
//   H[p*D + d]   = a[q] E[q, d] * a[q'] E[q', d]                         net.py:231-249 (is_H)
// and, for dz = dloss/dlogit and dH = dloss/dH:
//   t[q, d]      = dz + dH[p*D + d] * a[q'] * E[q', d]  (i != j),  dz  (i == j)
//   d_a[q]       = sum_d E[q, d] * t[q, d]  =  dz * sum_d E[q, d] + a[q'] * G[p],  G[p] = sum_d dH[p*D+d] E[q,d] E[q',d]
//   dE[q, d]     = a[q] * t[q, d] + (d == argmax_d E[q, :]) * d_pooled[q]
// The argmax is the smallest d among equal maxima (what the max pool's backward of the reference picks) and is
// recomputed from the cube: no index tensor is stored.  Every kernel is one persistent grid of 256-thread blocks; a block
// gathers its sample's rows once into the LDS cube and produces everything from there (the cube is never written to
// memory).  Behind the cube the dynamic LDS holds the sample's a [F*F] and F*F floats of scratch.  All sums are in a
// fixed order; there are no float atomics.
#include "ffm_cube.h"

namespace rec {
namespace {

struct FatArgs {
  FfmArgs f;
  int64_t lda, ldh;                            // floats between the rows of pooled / a / d_a / d_pooled, of H / dH
  int F2, NP, PD;                              // F*F slices, F(F-1)/2 pairs, pairs x D
  int cube;                                    // floats of the LDS cube image (0 on the table path)
};

// index of the pair (i < j) in nested-loop order
__device__ __forceinline__ int fat_pair(int F, int i, int j) { return (i * (2 * F - i - 1)) / 2 + j - i - 1; }

__device__ __forceinline__ int fat_opaque(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// rows / dval / av (the sample's attention row, where A is given) / the LDS cube of sample b
template <bool LDS>
__device__ inline void fat_load(const FatArgs& a, int64_t b, int64_t* rows, float* dval, float* img, float* av,
                                const float* __restrict__ A) {
  ffm_rows(a.f, b, rows);
  for (int k = threadIdx.x; k < a.f.Dn; k += kBlock) dval[k] = a.f.dense[b * a.f.Dn + k];
  if (A)
    for (int q = threadIdx.x; q < a.F2; q += kBlock) av[q] = A[b * a.lda + q];
  __syncthreads();
  if constexpr (LDS) {
    ffm_stage(a.f, b, rows, img);
    __syncthreads();
  }
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void fatffm_pool_fwd_kernel(FatArgs a, float* __restrict__ pooled) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  const int F = a.f.F, D = a.f.D;
  const int64_t chunk = (a.f.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.f.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    fat_load<LDS>(a, b, rows, dval, img, nullptr, nullptr);
    for (int q = threadIdx.x; q < a.F2; q += kBlock) {
      const int i = q / F, c0 = (q - i * F) * D;
      float m = ffm_e<LDS>(a.f, img, rows, dval, i, c0);
      for (int d = 1; d < D; ++d) {
        const float v = ffm_e<LDS>(a.f, img, rows, dval, i, c0 + d);
        m = v > m ? v : m;
      }
      pooled[b * a.lda + q] = m;
    }
    __syncthreads();                           // rows / dval / img are rewritten by the next sample
  }
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void fatffm_inter_fwd_kernel(FatArgs a, const float* __restrict__ A,
                                                                  float* __restrict__ H, float* __restrict__ y1) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  __shared__ float red[kBlock / kWave];
  float* av = img + a.cube;
  const int F = a.f.F, D = a.f.D;
  const int64_t chunk = (a.f.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.f.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    fat_load<LDS>(a, b, rows, dval, img, av, A);
    // the pairs of row i are the (F-1-i)*D consecutive floats of H from `off` on; every off-diagonal element of the
    // scaled cube is met exactly once here, so the first-order sum rides along
    float acc = 0.f;
    float* __restrict__ h = H + b * a.ldh;
    int i = 0, off = 0, next = (F - 1) * D;
    for (int idx = threadIdx.x; idx < a.PD; idx += kBlock) {
      while (idx >= next) {
        ++i;
        off = next;
        next += (F - 1 - i) * D;
      }
      const int c = (i + 1) * D + (idx - off);
      const int j = c / D, d = c - j * D;
      const float x = av[i * F + j] * ffm_e<LDS>(a.f, img, rows, dval, i, c);
      const float y = av[j * F + i] * ffm_e<LDS>(a.f, img, rows, dval, j, i * D + d);
      h[idx] = x * y;
      acc += x + y;
    }
    for (int idx = threadIdx.x; idx < F * D; idx += kBlock) {        // the diagonal slices
      const int f = idx / D;
      acc += av[f * F + f] * ffm_e<LDS>(a.f, img, rows, dval, f, f * D + (idx - f * D));
    }
    const float s = ffm_block_sum(acc, red);
    if (threadIdx.x == 0) y1[b] = s;
    __syncthreads();
  }
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void fatffm_attn_bwd_kernel(FatArgs a, const float* __restrict__ A,
                                                                 const float* __restrict__ dH,
                                                                 const float* __restrict__ dz,
                                                                 float* __restrict__ d_a) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  float* av = img + a.cube;
  float* G = av + a.F2;                        // NP <= F2 floats
  const int F = a.f.F, D = a.f.D;
  const int64_t chunk = (a.f.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.f.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    fat_load<LDS>(a, b, rows, dval, img, av, A);
    const float g = dz[b];
    const float* __restrict__ dh = dH + b * a.ldh;
    int i = 0, off = 0, next = F - 1;
    for (int p = threadIdx.x; p < a.NP; p += kBlock) {
      while (p >= next) {
        ++i;
        off = next;
        next += F - 1 - i;
      }
      const int j = i + 1 + (p - off);
      float s = 0.f;
      for (int d = 0; d < D; ++d)
        s += dh[p * D + d] * ffm_e<LDS>(a.f, img, rows, dval, i, j * D + d) *
             ffm_e<LDS>(a.f, img, rows, dval, j, i * D + d);
      G[p] = s;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < a.F2; q += kBlock) {
      const int f = q / F, j = q - f * F;
      float se = 0.f;
      for (int d = 0; d < D; ++d) se += ffm_e<LDS>(a.f, img, rows, dval, f, j * D + d);
      float r = g * se;
      if (f != j) r += av[j * F + f] * G[f < j ? fat_pair(F, f, j) : fat_pair(F, j, f)];
      d_a[b * a.lda + q] = r;
    }
    __syncthreads();
  }
}

// Sparse field i < S: row_grad[b*S + i, c] = dE[i][c] for c < R, 0 on the pad columns [R, grad_stride), written once,
// complete.  Dense field k: d dense_w[k, c] = sum_b dense[b,k] * dE_b[S+k][c] as per-block partials over a fixed sample
// range (registers on the fast path, the block's own workspace slice otherwise), folded in block order.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void fatffm_bwd_kernel(FatArgs a, const float* __restrict__ A,
                                                            const float* __restrict__ dH,
                                                            const float* __restrict__ dz,
                                                            const float* __restrict__ d_pooled,
                                                            float* __restrict__ row_grad, float* __restrict__ part) {
  extern __shared__ float img[];
  __shared__ int64_t rows[kFfmMaxFields];
  __shared__ float dval[kFfmMaxFields];
  float* av = img + a.cube;
  uint8_t* am = reinterpret_cast<uint8_t*>(av + a.F2);     // argmax_d of every slice: F2 bytes
  const int F = a.f.F, D = a.f.D, R = a.f.R, S = a.f.S;
  const int DnR = a.f.Dn * R;
  float* __restrict__ mine = part + (int64_t)blockIdx.x * DnR;
  float acc[kFfmAccRegs];
  if constexpr (LDS) {
#pragma unroll
    for (int r = 0; r < kFfmAccRegs; ++r) acc[r] = 0.f;
  } else {
    for (int e = threadIdx.x; e < DnR; e += kBlock) mine[e] = 0.f;
  }
  const bool v4 = a.f.gstride % 4 == 0 && ((uintptr_t)row_grad) % 16 == 0;
  const int64_t chunk = (a.f.B + gridDim.x - 1) / gridDim.x;
  const int64_t b0 = (int64_t)blockIdx.x * chunk, b1 = min(a.f.B, b0 + chunk);
  for (int64_t b = b0; b < b1; ++b) {
    fat_load<LDS>(a, b, rows, dval, img, av, A);
    for (int q = threadIdx.x; q < a.F2; q += kBlock) {     // first index among equal maxima
      const int i = q / F, c0 = (q - i * F) * D;
      float m = ffm_e<LDS>(a.f, img, rows, dval, i, c0);
      int best = 0;
      for (int d = 1; d < D; ++d) {
        const float v = ffm_e<LDS>(a.f, img, rows, dval, i, c0 + d);
        if (v > m) {
          m = v;
          best = d;
        }
      }
      am[q] = (uint8_t)best;
    }
    __syncthreads();
    const float g = dz[b];
    const float* __restrict__ dh = dH + b * a.ldh;
    const float* __restrict__ dp = d_pooled + b * a.lda;
    auto de = [&](int i, int c) -> float {     // dE[i][c]
      if (c >= R) return 0.f;
      const int j = c / D, d = c - j * D;
      const int q = i * F + j;
      float t = g;
      if (j != i) {
        const int p = i < j ? fat_pair(F, i, j) : fat_pair(F, j, i);
        t += dh[p * D + d] * av[j * F + i] * ffm_e<LDS>(a.f, img, rows, dval, j, i * D + d);
      }
      float r = av[q] * t;
      if (d == (int)am[q]) r += dp[q];
      return r;
    };
    float* __restrict__ out = row_grad + b * S * (int64_t)a.f.gstride;
    if (v4) {
      const int G4 = a.f.gstride >> 2, n = S * G4;
      for (int q = threadIdx.x; q < n; q += kBlock) {
        const int i = q / G4, c = (q - i * G4) * 4;
        const float t[4] = {de(i, c), de(i, c + 1), de(i, c + 2), de(i, c + 3)};
        vstore_nt<4>(out + (int64_t)i * a.f.gstride + c, t);
      }
    } else {
      const int n = S * a.f.gstride;
      for (int q = threadIdx.x; q < n; q += kBlock) {
        const int i = q / a.f.gstride, c = q - i * a.f.gstride;
        __builtin_nontemporal_store(de(i, c), out + q);
      }
    }
    if constexpr (LDS) {
#pragma unroll
      for (int r = 0; r < kFfmAccRegs; ++r) {
        // e does not depend on the sample: hidden from the optimiser, or it keeps the index arithmetic of all 24
        // elements in registers across the sample loop (> 256 VGPRs: one block per CU instead of two)
        const int e = fat_opaque(threadIdx.x + r * kBlock);
        if (e < DnR) {
          const int k = e / R;
          acc[r] += dval[k] * de(S + k, e - k * R);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      for (int e = threadIdx.x; e < DnR; e += kBlock) {
        const int k = e / R;
        mine[e] += dval[k] * de(S + k, e - k * R);
      }
    }
    __syncthreads();
  }
  if constexpr (LDS) {
#pragma unroll
    for (int r = 0; r < kFfmAccRegs; ++r) {
      const int e = threadIdx.x + r * kBlock;
      if (e < DnR) mine[e] = acc[r];
    }
  }
}

__global__ __launch_bounds__(kBlock) void fatffm_fold_kernel(int grid, int DnR, const float* __restrict__ part,
                                                             float* __restrict__ d_dense_w) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= DnR) return;
  float s = 0.f;
  for (int g = 0; g < grid; ++g) s += part[(int64_t)g * DnR + e];
  d_dense_w[e] = s;
}

int fat_check(const rec_fatffm_desc* d, bool attn, bool pair) {
  REC_REQUIRE(d, REC_EINVAL, "null desc");
  const rec_ffm_desc& f = d->ffm;
  REC_REQUIRE(f.batch >= 0 && f.num_rows >= 1 && f.num_slots >= 1 && f.num_dense >= 0 && f.dim >= 1, REC_EINVAL,
              "bad sizes");
  const int F = f.num_slots + f.num_dense;
  REC_REQUIRE(F <= kFfmMaxFields && f.dim <= kFfmMaxDim, REC_ESHAPE,
              "fatffm: %d fields x dim %d unsupported (need fields <= %d, dim <= %d)", F, f.dim, kFfmMaxFields,
              kFfmMaxDim);
  const int R = F * f.dim;
  REC_REQUIRE(f.row_stride >= R, REC_EINVAL, "row_stride %d < fields x dim %d", f.row_stride, R);
  const int64_t F2 = (int64_t)F * F, PD = (int64_t)F * (F - 1) / 2 * f.dim;
  REC_REQUIRE(!attn || d->ld_attn >= F2, REC_EINVAL, "ld_attn %lld < fields^2 %lld", (long long)d->ld_attn,
              (long long)F2);
  REC_REQUIRE(!pair || d->ld_pair >= PD, REC_EINVAL, "ld_pair %lld < pairs x dim %lld", (long long)d->ld_pair,
              (long long)PD);
  return REC_OK;
}

FatArgs fat_args(const rec_fatffm_desc* d, const int64_t* ids, const float* dense, const float* W,
                 const float* dense_w, int32_t* status) {
  FatArgs a;
  const rec_ffm_desc& f = d->ffm;
  a.f.B = f.batch; a.f.N = f.num_rows;
  a.f.S = f.num_slots; a.f.Dn = f.num_dense; a.f.D = f.dim; a.f.F = a.f.S + a.f.Dn; a.f.R = a.f.F * a.f.D;
  a.f.stride = f.row_stride; a.f.gstride = f.grad_stride; a.f.P = ffm_pitch(a.f.R, a.f.D);
  a.f.wvec = a.f.stride % 4 == 0 && ((uintptr_t)W) % 16 == 0;
  a.f.ids = ids; a.f.dense = dense; a.f.W = W; a.f.W1 = nullptr; a.f.dense_w = dense_w; a.f.dense_w_one = nullptr;
  a.f.status = status;
  a.lda = d->ld_attn; a.ldh = d->ld_pair;
  a.F2 = a.f.F * a.f.F; a.NP = a.f.F * (a.f.F - 1) / 2; a.PD = a.NP * a.f.D;
  const size_t cube = (size_t)a.f.F * a.f.P;
  a.cube = cube * sizeof(float) <= kFfmLdsMax ? (int)cube : 0;
  return a;
}

// dynamic LDS: the cube image (fast path), a [F2], F2 floats of scratch
size_t fat_lds_bytes(const FatArgs& a) { return ((size_t)a.cube + 2 * (size_t)a.F2) * sizeof(float); }

int fat_grid(int64_t B) { return (int)(B < kFfmGrid ? B : kFfmGrid); }

template <class K>
void fat_allow_lds(K kern) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(kFfmLdsMax + 2 * kFfmMaxFields * kFfmMaxFields * sizeof(float)));
}

}  // namespace
}  // namespace rec

using namespace rec;

#define FAT_LAUNCH(kernel, what, ...)                                                                   \
  do {                                                                                                  \
    const int grid = fat_grid(a.f.B);                                                                   \
    const size_t lds = fat_lds_bytes(a);                                                                \
    hipStream_t st = (hipStream_t)stream;                                                               \
    if (a.cube) {                                                                                       \
      static const bool once = (fat_allow_lds(kernel<true>), true);                                     \
      (void)once;                                                                                       \
      hipLaunchKernelGGL(kernel<true>, dim3(grid), dim3(kBlock), lds, st, a, __VA_ARGS__);              \
    } else {                                                                                            \
      hipLaunchKernelGGL(kernel<false>, dim3(grid), dim3(kBlock), lds, st, a, __VA_ARGS__);             \
    }                                                                                                   \
    rc = check_launch(what);                                                                            \
  } while (0)

extern "C" int rec_fatffm_pool_fwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense,
                                   const float* W, const float* dense_w, float* pooled, int32_t* status,
                                   void* stream) {
  int rc = fat_check(desc, true, false);
  if (rc != REC_OK) return rc;
  if (desc->ffm.batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && pooled && (desc->ffm.num_dense == 0 || (dense && dense_w)), REC_EINVAL,
              "null pointer argument");
  const FatArgs a = fat_args(desc, ids, dense, W, dense_w, status);
  FAT_LAUNCH(fatffm_pool_fwd_kernel, "rec_fatffm_pool_fwd", pooled);
  return rc;
}

extern "C" int rec_fatffm_inter_fwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense,
                                    const float* W, const float* dense_w, const float* a_attn, float* H, float* y1,
                                    int32_t* status, void* stream) {
  int rc = fat_check(desc, true, true);
  if (rc != REC_OK) return rc;
  if (desc->ffm.batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && a_attn && y1 && (H || desc->ffm.num_slots + desc->ffm.num_dense < 2) &&
              (desc->ffm.num_dense == 0 || (dense && dense_w)), REC_EINVAL, "null pointer argument");
  const FatArgs a = fat_args(desc, ids, dense, W, dense_w, status);
  FAT_LAUNCH(fatffm_inter_fwd_kernel, "rec_fatffm_inter_fwd", a_attn, H, y1);
  return rc;
}

extern "C" int rec_fatffm_attn_bwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense,
                                   const float* W, const float* dense_w, const float* a_attn, const float* dH,
                                   const float* dz, float* d_a, int32_t* status, void* stream) {
  int rc = fat_check(desc, true, true);
  if (rc != REC_OK) return rc;
  if (desc->ffm.batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && a_attn && dz && d_a && (dH || desc->ffm.num_slots + desc->ffm.num_dense < 2) &&
              (desc->ffm.num_dense == 0 || (dense && dense_w)), REC_EINVAL, "null pointer argument");
  const FatArgs a = fat_args(desc, ids, dense, W, dense_w, status);
  FAT_LAUNCH(fatffm_attn_bwd_kernel, "rec_fatffm_attn_bwd", a_attn, dH, dz, d_a);
  return rc;
}

extern "C" int rec_fatffm_bwd_workspace_bytes(const rec_fatffm_desc* desc, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = fat_check(desc, false, false);
  if (rc != REC_OK) return rc;
  const int64_t R = (int64_t)(desc->ffm.num_slots + desc->ffm.num_dense) * desc->ffm.dim;
  *bytes = (size_t)fat_grid(desc->ffm.batch) * (size_t)(desc->ffm.num_dense * R) * sizeof(float);
  return REC_OK;
}

extern "C" int rec_fatffm_bwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                              const float* dense_w, const float* a_attn, const float* dH, const float* dz,
                              const float* d_pooled, float* row_grad, float* d_dense_w, void* workspace,
                              size_t workspace_bytes, int32_t* status, void* stream) {
  int rc = fat_check(desc, true, true);
  if (rc != REC_OK) return rc;
  const rec_ffm_desc& f = desc->ffm;
  const int R = (f.num_slots + f.num_dense) * f.dim;
  REC_REQUIRE(f.grad_stride >= R, REC_EINVAL, "grad_stride %d < fields x dim %d", f.grad_stride, R);
  size_t need = 0;
  rec_fatffm_bwd_workspace_bytes(desc, &need);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "fatffm bwd workspace %zu < %zu bytes", workspace_bytes, need);
  if (f.batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && a_attn && dz && d_pooled && row_grad && (dH || f.num_slots + f.num_dense < 2) &&
              (f.num_dense == 0 || (dense && dense_w && d_dense_w && workspace)), REC_EINVAL,
              "null pointer argument");
  FatArgs a = fat_args(desc, ids, dense, W, dense_w, status);
  const int DnR = a.f.Dn * a.f.R;
  if (DnR > kFfmAccRegs * kBlock) a.cube = 0;  // the partial does not fit the registers: the table path keeps it in memory
  float* part = (float*)workspace;
  FAT_LAUNCH(fatffm_bwd_kernel, "rec_fatffm_bwd", a_attn, dH, dz, d_pooled, row_grad, part);
  if (rc != REC_OK || a.f.Dn == 0) return rc;
  hipLaunchKernelGGL(fatffm_fold_kernel, dim3((DnR + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream,
                     fat_grid(a.f.B), DnR, part, d_dense_w);
  return check_launch("rec_fatffm_bwd (fold)");
}
