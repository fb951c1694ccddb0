// The per-sample feature cube of the field-aware nets (csrc/ffm_ops.hip, csrc/fatffm_ops.hip): field f of sample b is the
// R = F*D wide row W[id_f] (f < S) or dense[b, f-S] * dense_w[f-S, :] (f >= S), and E[i, j, :] is block j of row i.  A
// block gathers a sample's S table rows once, coalesced, into an LDS image of the cube; the LDS pitch P satisfies
// P = D (mod 32), so the transposed piece reads of a wave, E[j*P + i*D + d] over consecutive c = j*D + d, fall on
// consecutive banks.  Cubes larger than kFfmLdsMax are read from the table itself (through L2).
#pragma once
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kFfmMaxFields = 64;
constexpr int kFfmMaxDim = 32;
constexpr int kFfmGrid = 2 * kNumCU;           // persistent grid (two 256-thread blocks per CU on the fast path)
constexpr size_t kFfmLdsMax = 76 * 1024;       // cube image per block: two blocks (+ static LDS) per CU in 160 KiB
constexpr int kFfmAccRegs = 24;                // d_dense_w partial per thread in registers: Dn*R <= 24*256

struct FfmArgs {
  int64_t B, N;
  int S, Dn, D, F, R, stride, gstride, P;
  bool wvec;                                   // W rows 16-B aligned and row_stride % 4 == 0: float4 staging
  const int64_t* ids;
  const float* dense;
  const float* W;
  const float* W1;
  const float* dense_w;
  const float* dense_w_one;
  int32_t* status;
};

__host__ __device__ inline int ffm_pitch(int R, int D) {
  const int Rp = (R + 3) & ~3;                 // float4 staging writes up to the padded width
  return Rp + (((D - Rp) % 32) + 32) % 32;     // smallest P >= Rp with P = D (mod 32)
}

// rows[f] = table row of field f of sample b (f < S), -1 for an id outside [0, N) (flagged, read as zeros)
__device__ inline void ffm_rows(const FfmArgs& a, int64_t b, int64_t* rows) {
  for (int s = threadIdx.x; s < a.S; s += kBlock) {
    const int64_t id = a.ids[b * a.S + s];
    const bool ok = id >= 0 && id < a.N;
    if (!ok && a.status) atomicOr(a.status, REC_FLAG_INDEX_OOB);
    rows[s] = ok ? id : -1;
  }
}

// element (f, c) of sample b's cube, from the LDS image or from the table
template <bool LDS>
__device__ __forceinline__ float ffm_e(const FfmArgs& a, const float* img, const int64_t* rows, const float* dval,
                                       int f, int c) {
  if constexpr (LDS) {
    return img[f * a.P + c];
  } else {
    if (f < a.S) {
      const int64_t r = rows[f];
      return r < 0 ? 0.f : a.W[r * a.stride + c];
    }
    return dval[f - a.S] * a.dense_w[(int64_t)(f - a.S) * a.R + c];
  }
}

__device__ inline void ffm_stage(const FfmArgs& a, int64_t b, const int64_t* rows, float* img) {
  if (a.wvec) {                                // (R + 3) / 4 float4 per row; the pad floats are never read back
    const int R4 = (a.R + 3) >> 2;
    const int n = a.S * R4;
    for (int q = threadIdx.x; q < n; q += kBlock) {
      const int f = q / R4, c = (q - f * R4) * 4;
      const int64_t r = rows[f];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r >= 0) v = *reinterpret_cast<const float4*>(a.W + r * a.stride + c);
      float* o = img + f * a.P + c;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
  } else {
    const int n = a.S * a.R;
    for (int q = threadIdx.x; q < n; q += kBlock) {
      const int f = q / a.R, c = q - f * a.R;
      const int64_t r = rows[f];
      img[f * a.P + c] = r < 0 ? 0.f : a.W[r * a.stride + c];
    }
  }
  const int n = a.Dn * a.R;
  for (int q = threadIdx.x; q < n; q += kBlock) {
    const int k = q / a.R, c = q - k * a.R;
    img[(a.S + k) * a.P + c] = a.dense[b * a.Dn + k] * a.dense_w[q];
  }
}

// fixed-order block sum (deterministic): wave butterflies, then wave 0 adds the four wave sums
__device__ inline float ffm_block_sum(float x, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = x;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) s = ((red[0] + red[1]) + red[2]) + red[3];
  return s;
}

}  // namespace
}  // namespace rec
