// The merged gradient of one table row, shared by the row-update kernels (sparse_update.hip, flen_ops.hip): where the
// gradient row of a lookup position lives (rec_grad_layout) and the fixed-order sum of a row's duplicates.
#pragma once
#include "rec_common.h"

namespace rec {

constexpr int kSegTile = REC_SEG_TILE, kSegLong = REC_SEG_LONG;

// element offset of the gradient row of lookup position `pos` (see rec_grad_layout)
__device__ __forceinline__ int64_t grad_offset(const rec_grad_layout& gl, int pos, int D) {
  const int p = gl.index ? gl.index[pos] : pos;   // multi-slot CSR: value k -> its (sample, slot) segment
  const int q = gl.div > 1 ? p / gl.div : p;
  return gl.group > 0 ? (int64_t)(q / gl.group) * gl.group_stride + (int64_t)(q % gl.group) * D
                      : (int64_t)q * D;
}
// ... of SORTED position k: the k-th row of grad when the producer wrote its rows in sorted order (rec_grad_layout.sorted:
// rec_deepfm_fm_bwd_sorted through the rank of rec_ids_group_slots) — consecutive segments then read consecutive
// memory and the dependent sorted_pos read drops out of the chain
__device__ __forceinline__ int64_t grad_at(const rec_grad_layout& gl, const int32_t* __restrict__ spos, int k, int D) {
  return gl.sorted ? (int64_t)k * D : grad_offset(gl, spos[k], D);
}

// g += the gradient rows of sorted positions [beg,end) (ascending; four loads in flight), through the
// tile partials when the segment is long and the caller supplied them
template <int VEC>
__device__ __forceinline__ void segment_sum(float (&g)[VEC], int beg, int end,
                                            const int32_t* __restrict__ spos,
                                            const float* __restrict__ grad,
                                            const rec_grad_layout& gl, int D, int d0) {
  if (gl.partials && end - beg >= kSegLong) {
    const float* __restrict__ pp = gl.partials;
    const int t1 = (end - 1) / kSegTile;
    int t = beg / kSegTile;
    auto at = [&](int tt) {
      return pp + ((int64_t)tt * 2 + (beg <= tt * kSegTile ? 0 : 1)) * D + d0;
    };
    for (; t + 4 <= t1 + 1; t += 4) {
      float a[VEC], b[VEC], c[VEC], d[VEC];
      vload<VEC>(a, at(t)); vload<VEC>(b, at(t + 1)); vload<VEC>(c, at(t + 2)); vload<VEC>(d, at(t + 3));
#pragma unroll
      for (int i = 0; i < VEC; ++i) g[i] = (((g[i] + a[i]) + b[i]) + c[i]) + d[i];
    }
    for (; t <= t1; ++t) {
      float a[VEC];
      vload<VEC>(a, at(t));
#pragma unroll
      for (int i = 0; i < VEC; ++i) g[i] += a[i];
    }
    return;
  }
  int k = beg;
  if (end - beg >= 8)   // short rows (the common case) stay on the plain loop: no divergence inside a wave
  for (; k + 4 <= end; k += 4) {
    float a[VEC], b[VEC], c[VEC], d[VEC];
    vload<VEC>(a, grad + grad_at(gl, spos, k, D) + d0);
    vload<VEC>(b, grad + grad_at(gl, spos, k + 1, D) + d0);
    vload<VEC>(c, grad + grad_at(gl, spos, k + 2, D) + d0);
    vload<VEC>(d, grad + grad_at(gl, spos, k + 3, D) + d0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] = (((g[i] + a[i]) + b[i]) + c[i]) + d[i];
  }
  for (; k < end; ++k) {
    float a[VEC];
    vload<VEC>(a, grad + grad_at(gl, spos, k, D) + d0);
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] += a[i];
  }
}

}  // namespace rec
