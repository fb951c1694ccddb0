// MatchPyramid (models/match/match-pyramid): the word-by-word interaction image of two sentences, convolved, rectified and
// max-pooled.  The reference runs matmul -> Conv2D("SAME") -> relu -> max_pool2d("VALID") and keeps [B, 1, Ll, Lr] once and
// [B, K, Ll, Lr] twice; here the image never leaves the chip:
//
//   mpyr_fwd_kernel     one block per (sample, pool-row band).  The band — the ph + kh - 1 image rows one row of pool windows
//                       reads, with a zero halo of kw - 1 columns — is computed into LDS (mpyr_cross_band), then one wave per
//                       pool window scans its cells, eight channels at a time, and keeps the first maximum: pooled + argmax
//   mpyr_gate_kernel    the same band again (the image is recomputed, not stored), then per window the winner's
//                       pre-activation (the ReLU gate) -> gated = the gradient that passes, and the block's share of d_conv_w /
//                       d_conv_b as one row of `partials`
//   mpyr_fold_kernel    d_conv_w / d_conv_b = the partial rows summed in a fixed order, 16 lanes an element
//   mpyr_dcross_kernel  d_cross in GATHER form: a cell adds up the windows whose winner's tap footprint reaches it, in a fixed
//                       order (a cell that won several windows of a channel sums their gradients first).  Two kinds of block per sample, each complete in its outputs, so nothing is folded across
//                       blocks: kRT image rows x all columns -> those rows of dL; all rows x kBT columns -> those rows of dR
//   mpyr_hinge_kernel   the pairwise hinge over the first 2 * pairs rows and d_pred, one block, fixed-order fold
//
// mpyr_cross_band: a thread owns one image column of a kBlock-wide tile and kRT band rows; the right sentence's rows are staged
// kEC embedding columns at a time through LDS (pitch kEC + 1: lane j reads word j * 17 + e, conflict-free), the left rows
// beside them, read as broadcasts.  No float atomics: the only atomic is the OR into the status word.  No scratch.
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kRT = 8;                                        // band / image rows a thread accumulates at once
constexpr int kEC = 16;                                       // embedding columns staged per pass
constexpr int kKC = 8;                                        // channels a lane convolves at once
constexpr int kGC = 4;                                        // channels of a block of the channel-group split (measurement)
constexpr int kBT = 128;                                      // image columns of a dR block
constexpr int kWaves = kBlock / kWave;

struct Geo {
  int Ll, Lr, E, K, kh, kw, ph, pw, sh, sw, relu;
  int PH, PW, pt, pl;                                         // pooled size; SAME padding in front (rows, columns)
  int nrows, bp, Kp;                                          // band rows, band pitch, K rounded up to kKC
  int64_t V, ldt, pad;
};

__device__ __forceinline__ bool row_ok(int64_t id, const Geo& g) { return id >= 0 && id < g.V && id != g.pad; }

// band[t * bp + pl + j] = <emb(left[r0 + t]), emb(right[j])> for t < nrows, j < Lr; rows outside the image, padding ids and
// out-of-range ids give zeros, and so does the halo.  oob: the caller has seen an id out of range already; with the ones met
// here it sets the status bit.  Ends with a barrier.
__device__ void mpyr_cross_band(const Geo& g, float* band, int r0, const int64_t* __restrict__ lid,
                                const int64_t* __restrict__ rid, const float* __restrict__ table, int32_t* status,
                                bool oob) {
  __shared__ float Rt[kBlock][kEC + 1];
  __shared__ float Lc[kRT][kEC];
  __shared__ int64_t Rid[kBlock];
  const int tid = threadIdx.x;
  for (int i = tid; i < g.nrows * g.bp; i += kBlock) band[i] = 0.f;
  for (int j0 = 0; j0 < g.Lr; j0 += kBlock) {
    __syncthreads();
    {
      int64_t id = -1;
      if (j0 + tid < g.Lr) {
        id = rid[j0 + tid];
        if (id < 0 || id >= g.V) oob = true;
        if (!row_ok(id, g)) id = -1;
      }
      Rid[tid] = id;
    }
    for (int t0 = 0; t0 < g.nrows; t0 += kRT) {
      float acc[kRT];
#pragma unroll
      for (int t = 0; t < kRT; ++t) acc[t] = 0.f;
      for (int e0 = 0; e0 < g.E; e0 += kEC) {
        __syncthreads();
        for (int idx = tid; idx < kBlock * kEC; idx += kBlock) {
          const int jj = idx / kEC, ee = idx % kEC;
          const int64_t id = Rid[jj];
          Rt[jj][ee] = (id >= 0 && e0 + ee < g.E) ? table[id * g.ldt + e0 + ee] : 0.f;
        }
        if (tid < kRT * kEC) {
          const int t = tid / kEC, ee = tid % kEC, i = r0 + t0 + t;
          float v = 0.f;
          if (t0 + t < g.nrows && i >= 0 && i < g.Ll) {
            const int64_t id = lid[i];
            if (id < 0 || id >= g.V) oob = true;
            if (row_ok(id, g) && e0 + ee < g.E) v = table[id * g.ldt + e0 + ee];
          }
          Lc[t][ee] = v;
        }
        __syncthreads();
#pragma unroll
        for (int ee = 0; ee < kEC; ++ee) {
          const float rv = Rt[tid][ee];
#pragma unroll
          for (int t = 0; t < kRT; ++t) acc[t] = fmaf(Lc[t][ee], rv, acc[t]);
        }
      }
      if (j0 + tid < g.Lr) {
#pragma unroll
        for (int t = 0; t < kRT; ++t)
          if (t0 + t < g.nrows) band[(t0 + t) * g.bp + g.pl + j0 + tid] = acc[t];
      }
    }
  }
  if (oob && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
  __syncthreads();
}

// wl[tap * Kp + k] = w[k, tap] (zeros for k >= K), bl[k] = bias[k] (zeros for k >= K)
__device__ __forceinline__ void mpyr_stage_weights(const Geo& g, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* wl, float* bl) {
  const int taps = g.kh * g.kw;
  for (int i = threadIdx.x; i < taps * g.Kp; i += kBlock) {
    const int tap = i / g.Kp, k = i % g.Kp;
    wl[i] = k < g.K ? w[k * taps + tap] : 0.f;
  }
  for (int k = threadIdx.x; k < g.Kp; k += kBlock) bl[k] = k < g.K ? bias[k] : 0.f;
}

// The pool windows of band p (in LDS) for the channels [k_begin, k_end): one wave per window, a lane a cell, KC channels at a
// time; the first maximum in row-major order wins.
template <int KC>
__device__ __forceinline__ void mpyr_pool_band(const Geo& g, const float* band, const float* wl, const float* bl, int64_t b, int p,
                                               int k_begin, int k_end, float* __restrict__ pooled, int64_t ldp,
                                               int32_t* __restrict__ argmax, int64_t lda) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int cells = g.ph * g.pw, plane = g.PH * g.PW;
  for (int q = wave; q < g.PW; q += kWaves) {
    for (int k0 = k_begin; k0 < k_end; k0 += KC) {
      float best[KC];
      int bidx[KC];
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        best[kk] = -INFINITY;
        bidx[kk] = INT_MAX;
      }
      for (int c = lane; c < cells; c += kWave) {
        const int ci = c / g.pw, cj = c - ci * g.pw;
        float acc[KC];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) acc[kk] = bl[k0 + kk];
        for (int a = 0; a < g.kh; ++a) {
          const float* row = band + (ci + a) * g.bp + q * g.sw + cj;
          const float* wr = wl + a * g.kw * g.Kp + k0;
          for (int bb = 0; bb < g.kw; ++bb) {
            const float x = row[bb];
            float wv[KC];
#pragma unroll
            for (int v = 0; v < KC; v += 4) vload<4>(*reinterpret_cast<float(*)[4]>(&wv[v]), wr + bb * g.Kp + v);
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) acc[kk] = fmaf(x, wv[kk], acc[kk]);
          }
        }
        const int cell = (p * g.sh + ci) * g.Lr + q * g.sw + cj;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
          const float v = g.relu ? fmaxf(acc[kk], 0.f) : acc[kk];
          if (v > best[kk]) {                                 // a lane's cells ascend: the first of equals stays
            best[kk] = v;
            bidx[kk] = cell;
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < KC; ++kk) {
        float v = best[kk];
        int id = bidx[kk];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
          const float ov = __shfl_xor(v, o, kWave);
          const int oid = __shfl_xor(id, o, kWave);
          if (ov > v || (ov == v && oid < id)) {              // ties: the smaller cell index = the first in row-major order
            v = ov;
            id = oid;
          }
        }
        if (lane == kk && k0 + kk < k_end) {
          const int64_t n = (int64_t)(k0 + kk) * plane + p * g.PW + q;
          pooled[b * ldp + n] = v;
          argmax[b * lda + n] = id;
        }
      }
    }
  }
}

// Every left id is looked at once per sample: the rows below the last pool window's reach belong to no band.
__device__ __forceinline__ bool mpyr_left_oob(const Geo& g, const int64_t* __restrict__ lid) {
  bool oob = false;
  for (int i = threadIdx.x; i < g.Ll; i += kBlock) oob |= lid[i] < 0 || lid[i] >= g.V;
  return oob;
}

// One block per (sample, pool-row band), all channels: the split that is used.
__global__ __launch_bounds__(kBlock) void mpyr_fwd_kernel(Geo g, const int64_t* __restrict__ left,
                                                          const int64_t* __restrict__ right, const float* __restrict__ table,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ pooled, int64_t ldp, int32_t* __restrict__ argmax,
                                                          int64_t lda, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int64_t b = blockIdx.x / g.PH;
  const int p = (int)(blockIdx.x % g.PH);
  float* wl = lds;                                            // [taps, Kp]
  float* bl = wl + g.kh * g.kw * g.Kp;                        // [Kp]
  float* band = bl + g.Kp;                                    // [nrows, bp]
  mpyr_stage_weights(g, w, bias, wl, bl);
  const bool oob = p == 0 && mpyr_left_oob(g, left + b * g.Ll);
  mpyr_cross_band(g, band, p * g.sh - g.pt, left + b * g.Ll, right + b * g.Lr, table, status, oob);
  mpyr_pool_band<kKC>(g, band, wl, bl, b, p, 0, g.K, pooled, ldp, argmax, lda);
}

// The split by channel group, kept for measurement only (REC_MPYR_SPLIT=channel): one block per (sample, group of kGC
// channels) that walks every band, so the image is computed once per group.  Same outputs, bit for bit.
__global__ __launch_bounds__(kBlock, 4) void mpyr_fwd_channel_kernel(Geo g, int groups, const int64_t* __restrict__ left,
                                                                  const int64_t* __restrict__ right,
                                                                  const float* __restrict__ table, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, float* __restrict__ pooled,
                                                                  int64_t ldp, int32_t* __restrict__ argmax, int64_t lda,
                                                                  int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int64_t b = blockIdx.x / groups;
  const int grp = (int)(blockIdx.x % groups);
  float* wl = lds;
  float* bl = wl + g.kh * g.kw * g.Kp;
  float* band = bl + g.Kp;
  mpyr_stage_weights(g, w, bias, wl, bl);
  const bool oob = grp == 0 && mpyr_left_oob(g, left + b * g.Ll);
  const int k_begin = grp * kGC, k_end = k_begin + kGC < g.K ? k_begin + kGC : g.K;
  for (int p = 0; p < g.PH; ++p) {
    __syncthreads();                                          // the band's readers are done before it is filled again
    mpyr_cross_band(g, band, p * g.sh - g.pt, left + b * g.Ll, right + b * g.Lr, table, status, oob);
    mpyr_pool_band<kGC>(g, band, wl, bl, b, p, k_begin, k_end, pooled, ldp, argmax, lda);
  }
}

// One block per (sample, pool-row band): gated [B, K * PH * PW] and the block's row of partials [B * PH, K * taps + K].
__global__ __launch_bounds__(kBlock) void mpyr_gate_kernel(Geo g, const int64_t* __restrict__ left,
                                                           const int64_t* __restrict__ right, const float* __restrict__ table,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ d_pooled, int64_t lddp,
                                                           const int32_t* __restrict__ argmax, int64_t lda,
                                                           float* __restrict__ gated, float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int64_t b = blockIdx.x / g.PH;
  const int p = (int)(blockIdx.x % g.PH);
  const int taps = g.kh * g.kw, plane = g.PH * g.PW, nwin = g.K * g.PW;
  float* wl = lds;
  float* bl = wl + taps * g.Kp;
  float* gl = bl + g.Kp;                                      // [K, PW] the gradient that passes
  int* off = reinterpret_cast<int*>(gl + nwin);               // [K, PW] the winner's first tap in the band
  float* band = reinterpret_cast<float*>(off + nwin);
  mpyr_stage_weights(g, w, bias, wl, bl);
  mpyr_cross_band(g, band, p * g.sh - g.pt, left + b * g.Ll, right + b * g.Lr, table, nullptr, false);
  for (int n = threadIdx.x; n < nwin; n += kBlock) {
    const int k = n / g.PW, q = n - k * g.PW;
    const int64_t m = (int64_t)k * plane + p * g.PW + q;
    const int am = argmax[b * lda + m];
    const int wi = am / g.Lr - p * g.sh, wj = am % g.Lr;
    float gv = 0.f;
    int o = 0;
    if (am >= 0 && wi >= 0 && wi < g.ph && wj >= q * g.sw && wj < q * g.sw + g.pw) {   // anything else is not a winner
      o = wi * g.bp + wj;
      float pre = bl[k];
      for (int a = 0; a < g.kh; ++a)
        for (int bb = 0; bb < g.kw; ++bb) pre = fmaf(band[o + a * g.bp + bb], wl[(a * g.kw + bb) * g.Kp + k], pre);
      gv = (g.relu && !(pre > 0.f)) ? 0.f : d_pooled[b * lddp + m];
    }
    gl[n] = gv;
    off[n] = o;
    gated[b * (int64_t)g.K * plane + m] = gv;
  }
  __syncthreads();
  float* part = partials + (int64_t)blockIdx.x * (g.K * taps + g.K);
  for (int i = threadIdx.x; i < g.K * taps; i += kBlock) {
    const int k = i / taps, tap = i - k * taps;
    const int o = (tap / g.kw) * g.bp + tap % g.kw;
    float s = 0.f;
    for (int q = 0; q < g.PW; ++q) s = fmaf(gl[k * g.PW + q], band[off[k * g.PW + q] + o], s);
    part[i] = s;
  }
  for (int k = threadIdx.x; k < g.K; k += kBlock) {
    float s = 0.f;
    for (int q = 0; q < g.PW; ++q) s += gl[k * g.PW + q];
    part[g.K * taps + k] = s;
  }
}

constexpr int kFoldLanes = 16;                                // lanes that share one element of the fold

// 16 lanes per element: lane s sums the rows s, s + 16, ... in ascending order, the 16 sums meet in a fixed shuffle tree
__global__ __launch_bounds__(kBlock) void mpyr_fold_kernel(int64_t blocks, int n, int split, const float* __restrict__ partials,
                                                           float* __restrict__ d_w, float* __restrict__ d_b) {
  const int i = blockIdx.x * (kBlock / kFoldLanes) + threadIdx.x / kFoldLanes, lane = threadIdx.x % kFoldLanes;
  float s = 0.f;
  if (i < n)
    for (int64_t r = lane; r < blocks; r += kFoldLanes) s += partials[r * n + i];
  s = group_sum<kFoldLanes>(s);                               // every lane of the wave takes part
  if (i >= n || lane != 0) return;
  if (i < split) d_w[i] = s;
  else d_b[i - split] = s;
}

// d_cross[i, j]: the windows whose rows can hold a winner within tap reach of (i, j), ascending (p, q, k)
__device__ __forceinline__ float mpyr_dcross_cell(const Geo& g, int i, int j, const int* wi_l, const int* wj_l, const float* gl,
                                                  const float* wl) {
  const int rlo = i + g.pt - (g.kh - 1) - g.ph + 1, clo = j + g.pl - (g.kw - 1) - g.pw + 1;
  const int p_lo = rlo <= 0 ? 0 : (rlo + g.sh - 1) / g.sh, q_lo = clo <= 0 ? 0 : (clo + g.sw - 1) / g.sw;
  int p_hi = (i + g.pt) / g.sh, q_hi = (j + g.pl) / g.sw;
  if (p_hi > g.PH - 1) p_hi = g.PH - 1;
  if (q_hi > g.PW - 1) q_hi = g.PW - 1;
  float s = 0.f;
  for (int p = p_lo; p <= p_hi; ++p)
    for (int q = q_lo; q <= q_hi; ++q)
      for (int k = 0; k < g.K; ++k) {
        const int n = (k * g.PH + p) * g.PW + q;
        const int a = i - wi_l[n] + g.pt, bb = j - wj_l[n] + g.pl;
        if ((unsigned)a < (unsigned)g.kh && (unsigned)bb < (unsigned)g.kw) s = fmaf(gl[n], wl[(k * g.kh + a) * g.kw + bb], s);
      }
  return s;
}

__global__ __launch_bounds__(kBlock) void mpyr_dcross_kernel(Geo g, int nL, int nR, int dc_floats, const int64_t* __restrict__ left,
                                                             const int64_t* __restrict__ right, const float* __restrict__ table,
                                                             const float* __restrict__ w, const float* __restrict__ gated,
                                                             const int32_t* __restrict__ argmax, int64_t lda,
                                                             float* __restrict__ dL, int64_t lddl, float* __restrict__ dR,
                                                             int64_t lddr) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float part[kWaves][kRT][kWave];
  const int64_t b = blockIdx.x / (nL + nR);
  const int role = (int)(blockIdx.x % (nL + nR));
  const int taps = g.kh * g.kw, N = g.K * g.PH * g.PW;
  float* dc = lds;                                            // dL block: [Lr, kRT]; dR block: [Ll, kBT] then L [Ll, E]
  float* wl = dc + dc_floats;                                 // [K, taps]
  float* gl = wl + g.K * taps;                                // [N]
  int* wi_l = reinterpret_cast<int*>(gl + N);                 // [N]
  int* wj_l = wi_l + N;                                       // [N]
  const int64_t* lid = left + b * g.Ll;
  const int64_t* rid = right + b * g.Lr;
  for (int i = threadIdx.x; i < g.K * taps; i += kBlock) wl[i] = w[i];
  for (int n = threadIdx.x; n < N; n += kBlock) {
    const int am = argmax[b * lda + n];
    const bool ok = am >= 0 && am < g.Ll * g.Lr;
    gl[n] = ok ? gated[b * (int64_t)N + n] : 0.f;
    wi_l[n] = ok ? am / g.Lr : -(1 << 20);
    wj_l[n] = ok ? am % g.Lr : -(1 << 20);
  }
  __syncthreads();
  // Overlapping windows: a cell may win several windows of a channel.  Their gradients are summed FIRST, in ascending window
  // order, at the first of them (the others pass nothing), as the framework's pool backward does before the convolution's: two
  // gradients that cancel then leave their exact difference instead of the rounding of two products.
  if (g.sh < g.ph || g.sw < g.pw) {
    float* gm = reinterpret_cast<float*>(wj_l + N);           // [N]
    const int rp = (g.ph - 1) / g.sh, rq = (g.pw - 1) / g.sw;
    for (int n = threadIdx.x; n < N; n += kBlock) {
      const int k = n / (g.PH * g.PW), r = n - k * g.PH * g.PW, p = r / g.PW, q = r - p * g.PW;
      const int p0 = p - rp < 0 ? 0 : p - rp, p1 = p + rp > g.PH - 1 ? g.PH - 1 : p + rp;
      const int q0 = q - rq < 0 ? 0 : q - rq, q1 = q + rq > g.PW - 1 ? g.PW - 1 : q + rq;
      float s = 0.f;
      bool first = true;
      for (int pp = p0; pp <= p1; ++pp)
        for (int qq = q0; qq <= q1; ++qq) {
          const int m = (k * g.PH + pp) * g.PW + qq;
          if (wi_l[m] != wi_l[n] || wj_l[m] != wj_l[n]) continue;
          if (m < n) first = false;
          s += gl[m];
        }
      gm[n] = first ? s : 0.f;
    }
    __syncthreads();
    gl = gm;
  }
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (role < nL) {
    const int i0 = role * kRT;
    for (int idx = threadIdx.x; idx < g.Lr * kRT; idx += kBlock) {
      const int j = idx / kRT, t = idx % kRT;
      dc[idx] = i0 + t < g.Ll ? mpyr_dcross_cell(g, i0 + t, j, wi_l, wj_l, gl, wl) : 0.f;
    }
    __syncthreads();
    const int seg = (g.Lr + kWaves - 1) / kWaves;
    const int jb = wave * seg, je = jb + seg < g.Lr ? jb + seg : g.Lr;
    for (int e0 = 0; e0 < g.E; e0 += kWave) {
      const int e = e0 + lane;
      float acc[kRT];
#pragma unroll
      for (int t = 0; t < kRT; ++t) acc[t] = 0.f;
      for (int j = jb; j < je; ++j) {
        const int64_t id = rid[j];
        if (!row_ok(id, g)) continue;
        const float rv = e < g.E ? table[id * g.ldt + e] : 0.f;
        float d[kRT];
        vload<4>(*reinterpret_cast<float(*)[4]>(&d[0]), dc + j * kRT);
        vload<4>(*reinterpret_cast<float(*)[4]>(&d[4]), dc + j * kRT + 4);
#pragma unroll
        for (int t = 0; t < kRT; ++t) acc[t] = fmaf(d[t], rv, acc[t]);
      }
#pragma unroll
      for (int t = 0; t < kRT; ++t) part[wave][t][lane] = acc[t];
      __syncthreads();
      for (int idx = threadIdx.x; idx < kRT * kWave; idx += kBlock) {
        const int t = idx / kWave, l = idx % kWave;
        float s = part[0][t][l];
#pragma unroll
        for (int v = 1; v < kWaves; ++v) s += part[v][t][l];
        if (i0 + t < g.Ll && e0 + l < g.E)
          dL[(b * g.Ll + i0 + t) * lddl + e0 + l] = row_ok(lid[i0 + t], g) ? s : 0.f;
      }
      __syncthreads();
    }
  } else {
    const int j0 = (role - nL) * kBT;
    float* Lrow = dc + g.Ll * kBT;
    for (int idx = threadIdx.x; idx < g.Ll * g.E; idx += kBlock) {
      const int64_t id = lid[idx / g.E];
      Lrow[idx] = row_ok(id, g) ? table[id * g.ldt + idx % g.E] : 0.f;
    }
    for (int idx = threadIdx.x; idx < g.Ll * kBT; idx += kBlock) {
      const int i = idx / kBT, jj = idx % kBT;
      dc[idx] = j0 + jj < g.Lr ? mpyr_dcross_cell(g, i, j0 + jj, wi_l, wj_l, gl, wl) : 0.f;
    }
    __syncthreads();
    for (int e0 = 0; e0 < g.E; e0 += kWave) {
      const int e = e0 + lane;
      if (e >= g.E) continue;
      for (int jj = wave; jj < kBT && j0 + jj < g.Lr; jj += kWaves) {
        float s = 0.f;
        for (int i = 0; i < g.Ll; ++i) s = fmaf(dc[i * kBT + jj], Lrow[i * g.E + e], s);
        dR[(b * g.Lr + j0 + jj) * lddr + e] = row_ok(rid[j0 + jj], g) ? s : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void mpyr_hinge_kernel(int64_t batch, int64_t pairs, const float* __restrict__ pred,
                                                            float* __restrict__ loss, float* __restrict__ d_pred) {
  __shared__ float part[kBlock];
  const float inv = 1.f / (float)pairs;
  float s = 0.f;
  for (int64_t r = threadIdx.x; r < pairs; r += kBlock) {
    const float x = 1.f - pred[r] + pred[pairs + r];
    const bool open = 0.f <= x;                               // the gradient flows at a hinge of exactly 0
    s += open ? x : 0.f;
    d_pred[r] = open ? -inv : 0.f;
    d_pred[pairs + r] = open ? inv : 0.f;
  }
  for (int64_t r = 2 * pairs + threadIdx.x; r < batch; r += kBlock) d_pred[r] = 0.f;
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] * inv;
}

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

}  // namespace
}  // namespace rec

using namespace rec;

// The checks every entry shares -> the geometry.  `what` names the entry.
struct MpyrShape {
  int32_t left_len, right_len, emb_dim, channels, filter_h, filter_w, pool_h, pool_w, stride_h, stride_w, relu;
};
static_assert(sizeof(MpyrShape) == REC_MPYR_SHAPE_LEN * sizeof(int32_t), "shape is REC_MPYR_SHAPE_LEN int32");

static int mpyr_geometry(const char* what, int64_t batch, const int32_t* shape, int64_t vocab, int64_t ld_table,
                         int64_t padding_idx, Geo* g) {
  REC_REQUIRE(shape != nullptr, REC_EINVAL, "%s: shape is null", what);
  const MpyrShape* d = reinterpret_cast<const MpyrShape*>(shape);
  REC_REQUIRE(batch >= 0 && batch < (1ll << 24), REC_EINVAL, "%s: batch %lld outside 0..2^24", what, (long long)batch);
  REC_REQUIRE(d->left_len >= 1 && d->left_len <= REC_MPYR_MAX_LEFT, REC_EINVAL, "%s: left_len %d outside 1..REC_MPYR_MAX_LEFT %d",
              what, d->left_len, REC_MPYR_MAX_LEFT);
  REC_REQUIRE(d->right_len >= 1 && d->right_len <= REC_MPYR_MAX_RIGHT, REC_EINVAL,
              "%s: right_len %d outside 1..REC_MPYR_MAX_RIGHT %d", what, d->right_len, REC_MPYR_MAX_RIGHT);
  REC_REQUIRE(d->emb_dim >= 1 && d->emb_dim <= REC_MPYR_MAX_EMB, REC_EINVAL, "%s: emb_dim %d outside 1..REC_MPYR_MAX_EMB %d", what,
              d->emb_dim, REC_MPYR_MAX_EMB);
  REC_REQUIRE(d->channels >= 1, REC_EINVAL, "%s: channels %d is not positive", what, d->channels);
  REC_REQUIRE(d->filter_h >= 1 && d->filter_w >= 1 && d->filter_h <= d->left_len && d->filter_w <= d->right_len, REC_EINVAL,
              "%s: filter [%d, %d] outside 1..the image [%d, %d]", what, d->filter_h, d->filter_w, d->left_len, d->right_len);
  REC_REQUIRE(d->pool_h >= 1 && d->pool_w >= 1 && d->pool_h <= d->left_len && d->pool_w <= d->right_len, REC_EINVAL,
              "%s: pool [%d, %d] outside 1..the image [%d, %d]", what, d->pool_h, d->pool_w, d->left_len, d->right_len);
  REC_REQUIRE(d->stride_h >= 1 && d->stride_w >= 1, REC_EINVAL, "%s: pool stride [%d, %d] is not positive", what, d->stride_h,
              d->stride_w);
  REC_REQUIRE(vocab >= 1, REC_EINVAL, "%s: vocab %lld is not positive", what, (long long)vocab);
  REC_REQUIRE(ld_table >= d->emb_dim, REC_EINVAL, "%s: ld_table %lld smaller than emb_dim %d", what, (long long)ld_table,
              d->emb_dim);
  g->Ll = d->left_len, g->Lr = d->right_len, g->E = d->emb_dim, g->K = d->channels, g->kh = d->filter_h, g->kw = d->filter_w;
  g->ph = d->pool_h, g->pw = d->pool_w, g->sh = d->stride_h, g->sw = d->stride_w, g->relu = d->relu != 0;
  g->PH = (g->Ll - g->ph) / g->sh + 1, g->PW = (g->Lr - g->pw) / g->sw + 1;
  g->pt = (g->kh - 1) / 2, g->pl = (g->kw - 1) / 2;
  g->nrows = g->ph + g->kh - 1, g->bp = g->Lr + g->kw - 1, g->Kp = round_up(g->K, kKC);
  g->V = vocab, g->ldt = ld_table, g->pad = padding_idx;
  REC_REQUIRE((int64_t)g->kh * g->kw * g->Kp <= REC_MPYR_MAX_WEIGHTS, REC_EINVAL,
              "%s: filter_h * filter_w * channels (rounded up to 8) = %lld above REC_MPYR_MAX_WEIGHTS %d", what,
              (long long)g->kh * g->kw * g->Kp, REC_MPYR_MAX_WEIGHTS);
  REC_REQUIRE((int64_t)g->nrows * g->bp <= REC_MPYR_MAX_BAND, REC_EINVAL,
              "%s: (pool_h + filter_h - 1) * (right_len + filter_w - 1) = %lld above REC_MPYR_MAX_BAND %d", what,
              (long long)g->nrows * g->bp, REC_MPYR_MAX_BAND);
  REC_REQUIRE((int64_t)g->K * g->PH * g->PW <= REC_MPYR_MAX_POOLED, REC_EINVAL,
              "%s: channels * PH * PW = %lld above REC_MPYR_MAX_POOLED %d", what, (long long)g->K * g->PH * g->PW,
              REC_MPYR_MAX_POOLED);
  return REC_OK;
}

extern "C" int rec_mpyr_fwd(int64_t batch, const int32_t* shape, int64_t vocab, int64_t ld_table, int64_t padding_idx,
                            const int64_t* left, const int64_t* right,
                            const float* table, const float* conv_w, const float* conv_b, float* pooled, int64_t ld_pooled,
                            int32_t* argmax, int64_t ld_argmax, int32_t* status, void* stream) {
  const char* what = "rec_mpyr_fwd";
  Geo g;
  int rc = mpyr_geometry(what, batch, shape, vocab, ld_table, padding_idx, &g);
  if (rc != REC_OK) return rc;
  const int64_t N = (int64_t)g.K * g.PH * g.PW;
  REC_REQUIRE(ld_pooled >= N && ld_argmax >= N, REC_EINVAL, "%s: ld_pooled / ld_argmax smaller than K * PH * PW (%lld)", what,
              (long long)N);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(left && right && table && conv_w && conv_b, REC_EINVAL, "%s: left / right / table / conv_w / conv_b is null", what);
  REC_REQUIRE(pooled && argmax, REC_EINVAL, "%s: pooled / argmax is null", what);
  REC_REQUIRE(pooled != table && pooled != conv_w && pooled != conv_b, REC_EINVAL, "%s: pooled aliases an input", what);
  const size_t lds = ((size_t)g.kh * g.kw * g.Kp + g.Kp + (size_t)g.nrows * g.bp) * sizeof(float);
  // REC_MPYR_SPLIT=channel (read once): the split by channel group, for tools/match_pyramid_bench.py; anything else: by band
  static const bool by_channel = [] {
    const char* e = getenv("REC_MPYR_SPLIT");
    return e != nullptr && strcmp(e, "channel") == 0;
  }();
  if (by_channel) {
    const int groups = (g.K + kGC - 1) / kGC;
    hipLaunchKernelGGL(mpyr_fwd_channel_kernel, dim3((unsigned)(batch * groups)), dim3(kBlock), lds, (hipStream_t)stream, g, groups,
                       left, right, table, conv_w, conv_b, pooled, ld_pooled, argmax, ld_argmax, status);
    return check_launch(what);
  }
  hipLaunchKernelGGL(mpyr_fwd_kernel, dim3((unsigned)(batch * g.PH)), dim3(kBlock), lds, (hipStream_t)stream, g, left, right, table,
                     conv_w, conv_b, pooled, ld_pooled, argmax, ld_argmax, status);
  return check_launch(what);
}

extern "C" int rec_mpyr_bwd(int64_t batch, const int32_t* shape, int64_t vocab, int64_t ld_table, int64_t padding_idx,
                            const int64_t* left, const int64_t* right,
                            const float* table, const float* conv_w, const float* conv_b, const float* d_pooled,
                            int64_t ld_dpooled, const int32_t* argmax, int64_t ld_argmax, float* gated, float* partials, float* dL,
                            int64_t ld_dl, float* dR, int64_t ld_dr, float* d_conv_w, float* d_conv_b, void* stream) {
  const char* what = "rec_mpyr_bwd";
  Geo g;
  int rc = mpyr_geometry(what, batch, shape, vocab, ld_table, padding_idx, &g);
  if (rc != REC_OK) return rc;
  const int64_t N = (int64_t)g.K * g.PH * g.PW;
  REC_REQUIRE(ld_dpooled >= N && ld_argmax >= N, REC_EINVAL, "%s: ld_dpooled / ld_argmax smaller than K * PH * PW (%lld)", what,
              (long long)N);
  REC_REQUIRE(ld_dl >= g.E && ld_dr >= g.E, REC_EINVAL, "%s: ld_dl / ld_dr smaller than emb_dim (%d)", what, g.E);
  REC_REQUIRE(d_conv_w && d_conv_b, REC_EINVAL, "%s: d_conv_w / d_conv_b is null", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(left && right && table && conv_w && conv_b, REC_EINVAL, "%s: left / right / table / conv_w / conv_b is null", what);
  REC_REQUIRE(d_pooled && argmax, REC_EINVAL, "%s: d_pooled / argmax is null", what);
  REC_REQUIRE(gated && partials && dL && dR, REC_EINVAL, "%s: gated / partials / dL / dR is null", what);
  for (const float* o : {(const float*)gated, (const float*)partials, (const float*)dL, (const float*)dR, (const float*)d_conv_w,
                         (const float*)d_conv_b})
    REC_REQUIRE(o != table && o != conv_w && o != conv_b && o != d_pooled, REC_EINVAL, "%s: an output aliases an input", what);
  REC_REQUIRE(dL != dR, REC_EINVAL, "%s: dL and dR are the same", what);
  hipStream_t st = (hipStream_t)stream;
  const int taps = g.kh * g.kw, nwin = g.K * g.PW, n = g.K * taps + g.K;
  const size_t lds_gate = ((size_t)taps * g.Kp + g.Kp + 2 * (size_t)nwin + (size_t)g.nrows * g.bp) * sizeof(float);
  hipLaunchKernelGGL(mpyr_gate_kernel, dim3((unsigned)(batch * g.PH)), dim3(kBlock), lds_gate, st, g, left, right, table, conv_w,
                     conv_b, d_pooled, ld_dpooled, argmax, ld_argmax, gated, partials);
  rc = check_launch("rec_mpyr_bwd (gate)");
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(mpyr_fold_kernel, dim3((unsigned)((n + kBlock / kFoldLanes - 1) / (kBlock / kFoldLanes))), dim3(kBlock), 0, st,
                     batch * g.PH, n,
                     g.K * taps, (const float*)partials, d_conv_w, d_conv_b);
  rc = check_launch("rec_mpyr_bwd (fold)");
  if (rc != REC_OK) return rc;
  const int nL = (g.Ll + kRT - 1) / kRT, nR = (g.Lr + kBT - 1) / kBT;
  const size_t cells_l = (size_t)g.Lr * kRT, cells_r = (size_t)g.Ll * kBT + (size_t)g.Ll * g.E;
  const int dc_floats = round_up((int)(cells_l > cells_r ? cells_l : cells_r), 4);
  const size_t lds_dc = ((size_t)g.K * taps + 4 * (size_t)N + dc_floats) * sizeof(float);
  hipLaunchKernelGGL(mpyr_dcross_kernel, dim3((unsigned)(batch * (nL + nR))), dim3(kBlock), lds_dc, st, g, nL, nR, dc_floats, left, right,
                     table, conv_w, (const float*)gated, argmax, ld_argmax, dL, ld_dl, dR, ld_dr);
  return check_launch("rec_mpyr_bwd (dcross)");
}

extern "C" int rec_mpyr_hinge(int64_t batch, int64_t pairs, const float* pred, float* loss, float* d_pred, void* stream) {
  const char* what = "rec_mpyr_hinge";
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31), REC_EINVAL, "%s: batch %lld outside 0..2^31", what, (long long)batch);
  REC_REQUIRE(pairs >= 1, REC_EINVAL, "%s: pairs %lld is not positive", what, (long long)pairs);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(2 * pairs <= batch, REC_EINVAL, "%s: 2 * pairs (%lld) above batch %lld", what, (long long)(2 * pairs),
              (long long)batch);
  REC_REQUIRE(pred && loss && d_pred, REC_EINVAL, "%s: pred / loss / d_pred is null", what);
  REC_REQUIRE(d_pred != pred && loss != pred, REC_EINVAL, "%s: an output aliases pred", what);
  hipLaunchKernelGGL(mpyr_hinge_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, batch, pairs, pred, loss, d_pred);
  return check_launch(what);
}
