// Field-embedded factorisation machine (models/rank/deepfefm/net.py:118-187, FEFM.forward) and its backward.
//   x[b, f, :] = W[id[b,f], :]  (0 where id == 0), id of a dense field = int64(dense * 1e5 + 1e6 + 2)   net.py:135-146
//   t[b, p]    = x_i^T (FE_p + FE_p^T) x_j,  p = (i, j), i < j in itertools.combinations order            net.py:149-169
// Cut: a block owns a tile of TS samples whose F embedding rows it gathers once into LDS (sample-major, odd pitch: the
// lanes of a wave are the samples and read the same (field, d) of different samples from different banks).  The pair
// matrices are symmetrised once per call into the workspace (fefm_sym_kernel) and read at wave-uniform addresses: a
// wave walks its share of the pairs (forward) or of the target fields (backward) with every lane on its own sample.
// At dim 9 everything is unrolled: x_i, x_j in registers, the 81 matrix elements through the scalar cache, 90 FMAs per
// pair and lane.  Other dims take the generic path: TS shrinks until the tile fits and the 64 / TS lanes of a sample
// split the rows of the matrix.  A batch with fewer tiles than the chip has CUs gives each tile to several blocks, which
// share its pairs (forward: y2 as per-block partials folded in order) or its target fields (backward).  Exact f32
// throughout (these sums cancel).
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kFefmMaxFields = 64;
constexpr int kFefmMaxDim = 64;
constexpr size_t kFefmLdsMax = 128 * 1024;     // dynamic LDS of a block (one block per CU; static arrays on top)
constexpr int kFefmGrid = 2 * kNumCU;          // cap of the persistent grids (fixed: the partial sums depend on it)
constexpr int kFefmFeSplitMax = 32;            // sample splits of the d_FE pass
constexpr int kFefmFeRegs = 16;                // d_FE elements per thread: dim^2 <= 16 * 256
constexpr int kFefmFwdSplitMax = 8;            // blocks that share a tile's pairs when the batch has few tiles
constexpr int kFefmRows = 16;                  // generic path: matrix rows a lane keeps in registers at a time

struct FefmArgs {
  int64_t B, N;
  int S, Dn, D, F, P, FD, stride, gstride, ld;
  int TS, NQ, pitch, nw;                       // samples per tile, lanes per sample, LDS floats per sample, waves
  int per;                                     // generic path: matrix rows per lane of a sample (a multiple of 4 when v4)
  bool v4;                                     // dim % 4 == 0: the symmetrised rows load as float4
  const int64_t* ids;                          // fwd: [B,S]; bwd: ids_all [B,F]
  const float* dense;
  const float* W;
  const float* W1;
  const float* dense_w_one;
  int32_t* status;
};

// id of a dense field (net.py:138): three separately rounded f32 operations, truncation toward zero.  A value whose
// result is not a finite number inside int64 gives -1 (out of range: flagged by the caller, never an index).
__device__ __forceinline__ int64_t fefm_dense_id(float v) {
#pragma clang fp contract(off)
  const float a = v * 1e5f;
  const float b = a + 1e6f;
  const float c = b + 2.f;
  if (!(c > -9.0e18f && c < 9.0e18f)) return -1;
  return (int64_t)c;
}

// rows[s*F + f] = table row of field f of sample b0 + s, -1 = zero vector (padding id 0, out of range, past the batch)
template <bool FWD>
__device__ inline void fefm_rows(const FefmArgs& a, int64_t b0, int* rows, int64_t* __restrict__ ids_all,
                                 bool write_ids = false) {
  const int n = a.TS * a.F;
  for (int q = threadIdx.x; q < n; q += blockDim.x) {
    const int s = q / a.F, f = q - s * a.F;
    const int64_t b = b0 + s;
    int r = -1;
    if (b < a.B) {
      int64_t id;
      if constexpr (FWD) {
        id = f < a.S ? a.ids[b * a.S + f] : fefm_dense_id(a.dense[b * a.Dn + (f - a.S)]);
        if (write_ids) ids_all[b * a.F + f] = id;
      } else {
        id = a.ids[b * a.F + f];
      }
      const bool ok = id >= 0 && id < a.N;
      if (!ok && a.status) atomicOr(a.status, REC_FLAG_INDEX_OOB);
      if (ok && id != 0) r = (int)id;
    }
    rows[q] = r;
  }
}

__device__ inline void fefm_stage(const FefmArgs& a, const int* rows, float* xs) {
  const int n = a.TS * a.FD;
  for (int q = threadIdx.x; q < n; q += blockDim.x) {
    const int s = q / a.FD, c = q - s * a.FD;
    const int f = c / a.D, d = c - f * a.D;
    const int r = rows[s * a.F + f];
    xs[s * a.pitch + c] = r < 0 ? 0.f : a.W[(int64_t)r * a.stride + d];
  }
}

// the pair after `step` more pairs in combinations order (wave-uniform)
__device__ __forceinline__ void fefm_next_pair(int F, int step, int& i, int& j) {
  j += step;
  while (j >= F && i < F) {
    const int over = j - F;
    ++i;
    j = i + 1 + over;
  }
}

// u[k] += M[r0 + k, c] * x for the nr (<= kFefmRows) rows of a lane: M is symmetric, so column c of those rows is the
// contiguous run mc = M + c * D + r0 (float4 loads when v4: D, r0 and nr are then multiples of 4)
__device__ __forceinline__ void fefm_axpy_rows(float (&u)[kFefmRows], const float* __restrict__ mc, float x, int nr,
                                               bool v4) {
  if (v4) {
#pragma unroll
    for (int g = 0; g < kFefmRows / 4; ++g) {
      if (g * 4 < nr) {
        const float4 t = *reinterpret_cast<const float4*>(mc + g * 4);
        u[g * 4] += t.x * x; u[g * 4 + 1] += t.y * x; u[g * 4 + 2] += t.z * x; u[g * 4 + 3] += t.w * x;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kFefmRows; ++k)
      if (k < nr) u[k] += mc[k] * x;
  }
}

// index of pair (i, j), i < j
__device__ __forceinline__ int fefm_pair(int F, int i, int j) { return i * F - i * (i + 1) / 2 + (j - i - 1); }

template <int DT>
__global__ __launch_bounds__(1024) void fefm_fwd_kernel(FefmArgs a, const float* __restrict__ sym,
                                                        float* __restrict__ y1, float* __restrict__ y2,
                                                        float* __restrict__ dnn_in, int64_t* __restrict__ ids_all,
                                                        float* __restrict__ y2_part) {
  // gridDim.y > 1 (few tiles): the blocks (x, 0 .. gridDim.y) stage the same tile and share its pairs; block y writes
  // its sum to y2_part[y * B + b] (folded in order by the caller), block 0 writes everything else
  extern __shared__ float xs[];
  __shared__ int rows[64 * kFefmMaxFields];
  __shared__ float red[16 * 64];
  const int lane = threadIdx.x % kWave;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int SD = a.S * a.D;
  const int64_t tiles = (a.B + a.TS - 1) / a.TS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b0 = tile * a.TS;
    const bool first = blockIdx.y == 0;
    fefm_rows<true>(a, b0, rows, ids_all, first);
    __syncthreads();
    fefm_stage(a, rows, xs);
    __syncthreads();
    // dnn_in = [ x[0:S] flattened | d1 | t ]                                                             net.py:179-185
    for (int q = threadIdx.x; first && q < a.TS * SD; q += blockDim.x) {
      const int s = q / SD, c = q - s * SD;
      if (b0 + s < a.B) dnn_in[(b0 + s) * a.ld + c] = xs[s * a.pitch + c];
    }
    for (int q = threadIdx.x; first && q < a.TS * a.Dn; q += blockDim.x) {
      const int s = q / a.Dn, k = q - s * a.Dn;
      if (b0 + s < a.B) dnn_in[(b0 + s) * a.ld + SD + k] = a.dense[(b0 + s) * a.Dn + k] * a.dense_w_one[k];
    }
    const int s = lane % a.TS, q = lane / a.TS;
    const int64_t b = b0 + s;
    const float* __restrict__ xb = xs + s * a.pitch;
    float acc = 0.f;
    int i = 0, j = 1;
    const int p0 = w + a.nw * (int)blockIdx.y, pstep = a.nw * (int)gridDim.y;
    fefm_next_pair(a.F, p0, i, j);
    for (int p = p0; p < a.P; p += pstep) {
      float t = 0.f;
      if constexpr (DT > 0) {
        const float* __restrict__ m = sym + (int64_t)p * (DT * DT);
        float xi[DT], xj[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          xi[d] = xb[i * DT + d];
          xj[d] = xb[j * DT + d];
        }
#pragma unroll
        for (int r = 0; r < DT; ++r) {
          float u = 0.f;
#pragma unroll
          for (int c = 0; c < DT; ++c) u += m[r * DT + c] * xj[c];
          t += xi[r] * u;
        }
      } else {
        const float* __restrict__ m = sym + (int64_t)p * (a.D * a.D);
        const float* __restrict__ xi = xb + i * a.D;
        const float* __restrict__ xj = xb + j * a.D;
        const int r1 = min(a.D, (q + 1) * a.per);
        for (int r0 = q * a.per; r0 < r1; r0 += kFefmRows) {
          const int nr = min(kFefmRows, r1 - r0);
          float u[kFefmRows];
#pragma unroll
          for (int k = 0; k < kFefmRows; ++k) u[k] = 0.f;
          for (int c = 0; c < a.D; ++c) fefm_axpy_rows(u, m + c * a.D + r0, xj[c], nr, a.v4);
#pragma unroll
          for (int k = 0; k < kFefmRows; ++k)
            if (k < nr) t += xi[r0 + k] * u[k];
        }
        for (int o = a.TS; o < kWave; o <<= 1) t += __shfl_xor(t, o, kWave);
      }
      acc += t;
      if (q == 0 && b < a.B) dnn_in[b * a.ld + SD + a.Dn + p] = t;
      fefm_next_pair(a.F, pstep, i, j);
    }
    red[w * kWave + lane] = acc;
    __syncthreads();
    if (threadIdx.x < a.TS && b0 + threadIdx.x < a.B) {
      const int ss = threadIdx.x;
      float s2 = 0.f;
      for (int ww = 0; ww < a.nw; ++ww) s2 += red[ww * kWave + ss];
      if (gridDim.y > 1) y2_part[(int64_t)blockIdx.y * a.B + b0 + ss] = s2;
      else y2[b0 + ss] = s2;
      if (first) {
        float s1 = 0.f;                                    // net.py:120-132
        for (int f = 0; f < a.S; ++f) {
          const int r = rows[ss * a.F + f];
          if (r >= 0) s1 += a.W1[r];
        }
        float sd = 0.f;
        for (int k = 0; k < a.Dn; ++k) sd += a.dense[(b0 + ss) * a.Dn + k] * a.dense_w_one[k];
        y1[b0 + ss] = s1 + sd;
      }
    }
    __syncthreads();                                       // rows / xs / red are rewritten by the next tile
  }
}

// dx[b,i,:] = sum_{j != i} g[b,p(i,j)] * (FE_p + FE_p^T) x[b,j,:]  (+ d_dnn_in[b, i*D ..] for i < S): a wave owns a
// target field, a lane a sample.  d_dense_w_one: threads k < Dn walk the tile's samples in order; one partial per block.
template <int DT>
__global__ __launch_bounds__(1024) void fefm_bwd_kernel(FefmArgs a, const float* __restrict__ sym,
                                                        const float* __restrict__ dz,
                                                        const float* __restrict__ d_dnn_in,
                                                        float* __restrict__ row_grad, float* __restrict__ part) {
  extern __shared__ float xs[];
  __shared__ int rows[64 * kFefmMaxFields];
  const int lane = threadIdx.x % kWave;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int SD = a.S * a.D;
  const int toff = SD + a.Dn;
  float acc1 = 0.f;
  const int64_t tiles = (a.B + a.TS - 1) / a.TS;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t b0 = tile * a.TS;
    fefm_rows<false>(a, b0, rows, nullptr);
    __syncthreads();
    fefm_stage(a, rows, xs);
    __syncthreads();
    if ((int)threadIdx.x < a.Dn && blockIdx.y == 0) {
      const int k = threadIdx.x;
      for (int s = 0; s < a.TS && b0 + s < a.B; ++s)
        acc1 += (dz[b0 + s] + d_dnn_in[(b0 + s) * a.ld + SD + k]) * a.dense[(b0 + s) * a.Dn + k];
    }
    const int s = lane % a.TS, q = lane / a.TS;
    const int64_t b = b0 + s;
    const bool live = b < a.B;
    const float* __restrict__ xb = xs + s * a.pitch;
    const float* __restrict__ gb = d_dnn_in + (live ? b : 0) * a.ld;
    const float dzb = live ? dz[b] : 0.f;
    // gridDim.y > 1 (few tiles): the blocks (x, 0 .. gridDim.y) stage the same tile and share its target fields
    for (int i = w + a.nw * (int)blockIdx.y; i < a.F; i += a.nw * (int)gridDim.y) {
      float* __restrict__ out = row_grad + ((live ? b : 0) * a.F + i) * (int64_t)a.gstride;
      const bool pad = rows[s * a.F + i] < 0;              // padding position: a zero row
      if constexpr (DT > 0) {
        float dx[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) dx[d] = 0.f;
        for (int j = 0; j < a.F; ++j) {
          if (j == i) continue;
          const int p = j > i ? fefm_pair(a.F, i, j) : fefm_pair(a.F, j, i);
          const float* __restrict__ m = sym + (int64_t)p * (DT * DT);
          const float g = dzb + gb[toff + p];
          float xj[DT];
#pragma unroll
          for (int d = 0; d < DT; ++d) xj[d] = g * xb[j * DT + d];
#pragma unroll
          for (int r = 0; r < DT; ++r) {
#pragma unroll
            for (int c = 0; c < DT; ++c) dx[r] += m[r * DT + c] * xj[c];
          }
        }
        if (live) {
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            float v = dx[d];
            if (i < a.S) v += gb[i * DT + d];
            out[d] = pad ? 0.f : v;
          }
          for (int d = DT; d < a.gstride; ++d) out[d] = 0.f;
        }
      } else {
        const int r1 = min(a.D, (q + 1) * a.per);
        for (int r0 = q * a.per; r0 < r1; r0 += kFefmRows) {
          const int nr = min(kFefmRows, r1 - r0);
          float dx[kFefmRows];
#pragma unroll
          for (int k = 0; k < kFefmRows; ++k) dx[k] = 0.f;
          for (int j = 0; j < a.F; ++j) {
            if (j == i) continue;
            const int p = j > i ? fefm_pair(a.F, i, j) : fefm_pair(a.F, j, i);
            const float* __restrict__ m = sym + (int64_t)p * (a.D * a.D) + r0;
            const float* __restrict__ xj = xb + j * a.D;
            const float g = dzb + gb[toff + p];
            float u[kFefmRows];                            // per partner, then dx += g * u: short sums (these terms cancel)
#pragma unroll
            for (int k = 0; k < kFefmRows; ++k) u[k] = 0.f;
            for (int c = 0; c < a.D; ++c) fefm_axpy_rows(u, m + c * a.D, xj[c], nr, a.v4);
#pragma unroll
            for (int k = 0; k < kFefmRows; ++k) dx[k] += g * u[k];
          }
#pragma unroll
          for (int k = 0; k < kFefmRows; ++k) {
            if (k < nr && live) {
              float v = dx[k];
              if (i < a.S) v += gb[i * a.D + r0 + k];
              out[r0 + k] = pad ? 0.f : v;
            }
          }
        }
        if (live)
          for (int d = a.D + q; d < a.gstride; d += a.NQ) out[d] = 0.f;
      }
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < a.Dn && blockIdx.y == 0) part[(int64_t)blockIdx.x * a.Dn + threadIdx.x] = acc1;
}

__global__ __launch_bounds__(kBlock) void fefm_sym_kernel(int P, int D, const float* __restrict__ FE,
                                                          float* __restrict__ sym) {
  const int DD = D * D;
  const int64_t n = (int64_t)P * DD;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
    const int64_t p = e / DD;
    const int r = (int)(e - p * DD) / D, c = (int)(e - p * DD) % D;
    sym[e] = FE[e] + FE[p * DD + c * D + r];
  }
}

// out[e] = sum over g < n of part[g * width + e], in order
__global__ __launch_bounds__(kBlock) void fefm_fold_kernel(int n, int64_t width, const float* __restrict__ part,
                                                           float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= width) return;
  float s = 0.f;
  for (int g = 0; g < n; ++g) s += part[(int64_t)g * width + e];
  out[e] = s;
}

// d_FE_p = sum_b g[b,p] * (x_i x_j^T + x_j x_i^T): block (p, split) walks its sample range 64 at a time (rows gathered
// through ids_all into LDS); thread (q, e) sums the samples s = q (mod nq) of element e, the nq sums are added in order.
__global__ __launch_bounds__(kBlock) void fefm_dfe_kernel(FefmArgs a, const float* __restrict__ dz,
                                                          const float* __restrict__ d_dnn_in, int64_t per_split,
                                                          float* __restrict__ part) {
  __shared__ float xi[64 * kFefmMaxDim], xj[64 * kFefmMaxDim], g[64];
  __shared__ float red[kBlock];
  const int p = blockIdx.x;
  int i = 0, j = 1;
  fefm_next_pair(a.F, p, i, j);
  const int D = a.D, DD = D * D;
  const int nq = DD >= kBlock / 2 ? 1 : kBlock / DD;
  const int q = nq == 1 ? 0 : threadIdx.x / DD;
  const int e0 = nq == 1 ? threadIdx.x : threadIdx.x - q * DD;
  const int toff = a.S * D + a.Dn;
  float acc[kFefmFeRegs];
#pragma unroll
  for (int r = 0; r < kFefmFeRegs; ++r) acc[r] = 0.f;
  const int64_t b0 = (int64_t)blockIdx.y * per_split, b1 = min(a.B, b0 + per_split);
  for (int64_t bb = b0; bb < b1; bb += 64) {
    const int ns = (int)min((int64_t)64, b1 - bb);
    for (int t = threadIdx.x; t < ns * D; t += kBlock) {
      const int s = t / D, d = t - s * D;
      const int64_t ri = a.ids[(bb + s) * a.F + i], rj = a.ids[(bb + s) * a.F + j];
      xi[s * D + d] = (ri > 0 && ri < a.N) ? a.W[ri * a.stride + d] : 0.f;
      xj[s * D + d] = (rj > 0 && rj < a.N) ? a.W[rj * a.stride + d] : 0.f;
    }
    for (int s = threadIdx.x; s < ns; s += kBlock) g[s] = dz[bb + s] + d_dnn_in[(bb + s) * a.ld + toff + p];
    __syncthreads();
    if (q < nq) {
#pragma unroll
      for (int r = 0; r < kFefmFeRegs; ++r) {
        const int e = e0 + r * kBlock;
        if (e < DD && (r == 0 || nq == 1)) {
          const int ra = e / D, cb = e - ra * D;
          for (int s = q; s < ns; s += nq)
            acc[r] += g[s] * (xi[s * D + ra] * xj[s * D + cb] + xi[s * D + cb] * xj[s * D + ra]);
        }
      }
    }
    __syncthreads();
  }
  float* __restrict__ mine = part + ((int64_t)blockIdx.y * a.P + p) * DD;
  if (nq == 1) {
#pragma unroll
    for (int r = 0; r < kFefmFeRegs; ++r) {
      const int e = e0 + r * kBlock;
      if (e < DD) mine[e] = acc[r];
    }
  } else {
    red[threadIdx.x] = acc[0];
    __syncthreads();
    if ((int)threadIdx.x < DD) {
      float s = 0.f;
      for (int k = 0; k < nq; ++k) s += red[k * DD + threadIdx.x];
      mine[threadIdx.x] = s;
    }
  }
}

int fefm_check(const rec_fefm_desc* d) {
  REC_REQUIRE(d, REC_EINVAL, "null desc");
  REC_REQUIRE(d->batch >= 0 && d->num_rows >= 1 && d->num_slots >= 0 && d->num_dense >= 0 && d->dim >= 1, REC_EINVAL,
              "bad sizes");
  const int F = d->num_slots + d->num_dense;
  REC_REQUIRE(F >= 2 && F <= kFefmMaxFields && d->dim <= kFefmMaxDim, REC_ESHAPE,
              "fefm: %d fields x dim %d unsupported (need 2 <= fields <= %d, dim <= %d)", F, d->dim, kFefmMaxFields,
              kFefmMaxDim);
  REC_REQUIRE(d->num_rows <= 0x7fffffffll, REC_ESHAPE, "fefm: more than 2^31 - 1 table rows");
  REC_REQUIRE(d->row_stride >= d->dim, REC_EINVAL, "row_stride %d < dim %d", d->row_stride, d->dim);
  REC_REQUIRE(d->ld <= 0x7fffffffll, REC_ESHAPE, "fefm: ld %lld exceeds 2^31 - 1", (long long)d->ld);
  REC_REQUIRE(d->ld >= d->num_slots * d->dim + d->num_dense + F * (F - 1) / 2, REC_EINVAL,
              "ld %lld < the %d columns of dnn_in", (long long)d->ld, d->num_slots * d->dim + d->num_dense + F * (F - 1) / 2);
  return REC_OK;
}

// waves of the backward's block: the count in [8, 16] that wastes the fewest wave slots on `items` target fields
int fefm_waves(int items) {
  int best = 16, best_waste = 1 << 30;
  for (int nw = 16; nw >= 8; --nw) {
    const int waste = (items + nw - 1) / nw * nw - items;
    if (waste < best_waste) { best = nw; best_waste = waste; }
  }
  return best;
}

FefmArgs fefm_args(const rec_fefm_desc* d, const int64_t* ids, const float* dense, const float* W, const float* W1,
                   const float* dense_w_one, int32_t* status) {
  FefmArgs a;
  a.B = d->batch; a.N = d->num_rows;
  a.S = d->num_slots; a.Dn = d->num_dense; a.D = d->dim; a.F = a.S + a.Dn; a.P = a.F * (a.F - 1) / 2;
  a.FD = a.F * a.D; a.stride = d->row_stride; a.gstride = d->grad_stride; a.ld = (int)d->ld;
  a.pitch = a.FD | 1;
  a.TS = 64;
  while ((size_t)a.TS * a.pitch * sizeof(float) > kFefmLdsMax) a.TS >>= 1;
  a.NQ = 64 / a.TS;
  a.v4 = a.D % 4 == 0;
  a.per = (a.D + a.NQ - 1) / a.NQ;
  if (a.v4) a.per = (a.per + 3) & ~3;
  a.nw = 16;
  a.ids = ids; a.dense = dense; a.W = W; a.W1 = W1; a.dense_w_one = dense_w_one; a.status = status;
  return a;
}

int fefm_grid(const FefmArgs& a) {
  const int64_t tiles = (a.B + a.TS - 1) / a.TS;
  return (int)(tiles < kFefmGrid ? tiles : kFefmGrid);
}

// blocks per tile: 1 once the tiles fill the chip, else enough to, up to `most` (a function of the shape only)
int fefm_tile_split(const FefmArgs& a, int most) {
  const int64_t tiles = (a.B + a.TS - 1) / a.TS;
  if (tiles >= kNumCU || tiles < 1) return 1;
  const int64_t n = kNumCU / tiles;
  return (int)(n < most ? n : most);
}

int fefm_fe_splits(const rec_fefm_desc* d) {
  const int F = d->num_slots + d->num_dense;
  const int64_t per = (int64_t)(F * (F - 1) / 2) * d->dim * d->dim * sizeof(float);
  int64_t n = (d->batch + 255) / 256;
  if (n > kFefmFeSplitMax) n = kFefmFeSplitMax;
  const int64_t cap = (64ll << 20) / per;                  // partials of at most 64 MiB
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

// Lets kernel Kern take up to kFefmLdsMax of dynamic LDS: once per kernel and device; a failure is reported here, with
// its cause, instead of as a launch error later.
constexpr int kFefmMaxDevices = 64;
template <auto Kern>
int fefm_allow_lds(const char* what) {
  static bool done[kFefmMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const bool known = dev >= 0 && dev < kFefmMaxDevices;
  if (known && done[dev]) return REC_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kFefmLdsMax);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit to %zu bytes: %s", what, kFefmLdsMax, hipGetErrorString(e));
    return REC_EHIP;
  }
  if (known) done[dev] = true;
  return REC_OK;
}

int fefm_sym(const FefmArgs& a, const float* FE, float* sym, hipStream_t st) {
  const int64_t n = (int64_t)a.P * a.D * a.D;
  const int grid = (int)min((int64_t)kNumCU * 4, (n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(fefm_sym_kernel, dim3(grid), dim3(kBlock), 0, st, a.P, a.D, FE, sym);
  return check_launch("rec_fefm (symmetrise)");
}

size_t fefm_sym_bytes(const rec_fefm_desc* d) {
  const int F = d->num_slots + d->num_dense;
  return align_up((size_t)(F * (F - 1) / 2) * d->dim * d->dim * sizeof(float), 256);
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_fefm_fwd_workspace_bytes(const rec_fefm_desc* desc, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = fefm_check(desc);
  if (rc != REC_OK) return rc;
  const FefmArgs a = fefm_args(desc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  const int split = fefm_tile_split(a, kFefmFwdSplitMax);
  *bytes = fefm_sym_bytes(desc) + (split > 1 ? (size_t)split * (size_t)a.B * sizeof(float) : 0);
  return REC_OK;
}

extern "C" int rec_fefm_fwd(const rec_fefm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                            const float* W1, const float* dense_w_one, const float* FE, float* y1, float* y2,
                            float* dnn_in, int64_t* ids_all, void* workspace, size_t workspace_bytes, int32_t* status,
                            void* stream) {
  int rc = fefm_check(desc);
  if (rc != REC_OK) return rc;
  size_t need = 0;
  rec_fefm_fwd_workspace_bytes(desc, &need);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "fefm fwd workspace %zu < %zu bytes", workspace_bytes, need);
  if (desc->batch == 0) return REC_OK;
  REC_REQUIRE((desc->num_slots == 0 || ids) && (desc->num_dense == 0 || (dense && dense_w_one)) && W && W1 && FE && y1 &&
              y2 && dnn_in && ids_all && workspace, REC_EINVAL, "null pointer argument");
  float* sym = (float*)workspace;
  FefmArgs a = fefm_args(desc, ids, dense, W, W1, dense_w_one, status);   // 16 waves: P pairs are many rounds
  hipStream_t st = (hipStream_t)stream;
  rc = fefm_sym(a, FE, sym, st);
  if (rc != REC_OK) return rc;
  const size_t lds = (size_t)a.TS * a.pitch * sizeof(float);
  const int grid = fefm_grid(a);
  const int split = fefm_tile_split(a, kFefmFwdSplitMax);
  float* y2_part = (float*)((char*)workspace + fefm_sym_bytes(desc));
  if (a.D == 9 && a.TS == 64) {
    if ((rc = fefm_allow_lds<fefm_fwd_kernel<9>>("rec_fefm_fwd")) != REC_OK) return rc;
    hipLaunchKernelGGL(fefm_fwd_kernel<9>, dim3(grid, split), dim3(a.nw * kWave), lds, st, a, sym, y1, y2, dnn_in,
                       ids_all, y2_part);
  } else {
    if ((rc = fefm_allow_lds<fefm_fwd_kernel<0>>("rec_fefm_fwd")) != REC_OK) return rc;
    hipLaunchKernelGGL(fefm_fwd_kernel<0>, dim3(grid, split), dim3(a.nw * kWave), lds, st, a, sym, y1, y2, dnn_in,
                       ids_all, y2_part);
  }
  rc = check_launch("rec_fefm_fwd");
  if (rc != REC_OK || split == 1) return rc;
  hipLaunchKernelGGL(fefm_fold_kernel, dim3((unsigned)((a.B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, split, a.B,
                     y2_part, y2);
  return check_launch("rec_fefm_fwd (fold)");
}

extern "C" int rec_fefm_bwd_workspace_bytes(const rec_fefm_desc* desc, int32_t want_d_fe, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  int rc = fefm_check(desc);
  if (rc != REC_OK) return rc;
  size_t n = fefm_sym_bytes(desc);
  n += align_up((size_t)kFefmGrid * (size_t)(desc->num_dense > 0 ? desc->num_dense : 1) * sizeof(float), 256);
  if (want_d_fe) n += (size_t)fefm_fe_splits(desc) * fefm_sym_bytes(desc);
  *bytes = n;
  return REC_OK;
}

extern "C" int rec_fefm_bwd(const rec_fefm_desc* desc, const int64_t* ids_all, const float* dense, const float* W,
                            const float* FE, const float* dz, const float* d_dnn_in, float* row_grad,
                            float* d_dense_w_one, float* d_FE, void* workspace, size_t workspace_bytes,
                            int32_t* status, void* stream) {
  int rc = fefm_check(desc);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(desc->grad_stride >= desc->dim, REC_EINVAL, "grad_stride %d < dim %d", desc->grad_stride, desc->dim);
  size_t need = 0;
  rec_fefm_bwd_workspace_bytes(desc, d_FE != nullptr, &need);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "fefm bwd workspace %zu < %zu bytes", workspace_bytes, need);
  REC_REQUIRE(ids_all && W && FE && dz && d_dnn_in && row_grad && workspace &&
              (desc->num_dense == 0 || (dense && d_dense_w_one)), REC_EINVAL, "null pointer argument");
  hipStream_t st = (hipStream_t)stream;
  float* sym = (float*)workspace;
  float* part1 = (float*)((char*)workspace + fefm_sym_bytes(desc));
  float* part_fe = (float*)((char*)part1 + align_up((size_t)kFefmGrid * (size_t)(desc->num_dense > 0 ? desc->num_dense : 1) *
                                                    sizeof(float), 256));
  FefmArgs a = fefm_args(desc, ids_all, dense, W, nullptr, nullptr, status);
  const int64_t fe_n = (int64_t)a.P * a.D * a.D;
  if (desc->batch == 0) {                                  // empty sums
    if (a.Dn > 0) (void)hipMemsetAsync(d_dense_w_one, 0, a.Dn * sizeof(float), st);
    if (d_FE) (void)hipMemsetAsync(d_FE, 0, fe_n * sizeof(float), st);
    return check_launch("rec_fefm_bwd (empty)");
  }
  a.nw = fefm_waves(a.F);
  rc = fefm_sym(a, FE, sym, st);
  if (rc != REC_OK) return rc;
  const size_t lds = (size_t)a.TS * a.pitch * sizeof(float);
  const int grid = fefm_grid(a);
  const dim3 grid2(grid, fefm_tile_split(a, (a.F + a.nw - 1) / a.nw));
  if (a.D == 9 && a.TS == 64) {
    if ((rc = fefm_allow_lds<fefm_bwd_kernel<9>>("rec_fefm_bwd")) != REC_OK) return rc;
    hipLaunchKernelGGL(fefm_bwd_kernel<9>, grid2, dim3(a.nw * kWave), lds, st, a, sym, dz, d_dnn_in, row_grad, part1);
  } else {
    if ((rc = fefm_allow_lds<fefm_bwd_kernel<0>>("rec_fefm_bwd")) != REC_OK) return rc;
    hipLaunchKernelGGL(fefm_bwd_kernel<0>, grid2, dim3(a.nw * kWave), lds, st, a, sym, dz, d_dnn_in, row_grad, part1);
  }
  rc = check_launch("rec_fefm_bwd");
  if (rc != REC_OK) return rc;
  if (a.Dn > 0) {
    hipLaunchKernelGGL(fefm_fold_kernel, dim3((a.Dn + kBlock - 1) / kBlock), dim3(kBlock), 0, st, grid, (int64_t)a.Dn,
                       part1, d_dense_w_one);
    rc = check_launch("rec_fefm_bwd (fold)");
    if (rc != REC_OK) return rc;
  }
  if (!d_FE) return REC_OK;
  const int splits = fefm_fe_splits(desc);
  const int64_t per_split = ((a.B + splits - 1) / splits + 63) / 64 * 64;
  hipLaunchKernelGGL(fefm_dfe_kernel, dim3(a.P, splits), dim3(kBlock), 0, st, a, dz, d_dnn_in, per_split, part_fe);
  rc = check_launch("rec_fefm_bwd (d_FE)");
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(fefm_fold_kernel, dim3((unsigned)((fe_n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, splits, fe_n,
                     part_fe, d_FE);
  return check_launch("rec_fefm_bwd (d_FE fold)");
}
