// DIEN (rank/dien) on gfx950: the GRU recurrence as ONE launch per layer and direction, the auxiliary loss, and the
// position-wise attention of dien/net.py:192-209.
//
//   rec_gru_seq_fwd / _bwd            <- paddle.nn.GRU / GRUCell stepped over T (net.py:153-159,190,266-271): the host
//                                        computes Gi = X W_ih^T + b_ih for all B*T rows with rec_gemm_f32; the kernel walks
//                                        the time loop with h on chip
//   rec_dien_aux_fwd / _bwd           <- net.py:219-254 (no length mask, no minus sign, sigma(n) not 1 - sigma(n))
//   rec_dien_att_feat_fwd / _bwd      <- [h, q, h - q, h * q] (net.py:193-199) around the attention MLP's GEMMs
//   rec_dien_attention_seq_fwd / _bwd <- (score + mask) * E^-0.5, softmax over T, x_att = w * hist (net.py:203-209)
//
// Recurrent kernels.  A block of 8 waves owns 16 batch rows (the M of v_mfma_f32_16x16x4_f32) for the whole time loop.
// Forward: wave w owns the hidden columns of the 16-column tiles w, w + 8 and there the r, z and c columns of
// h W_hh^T: three independent accumulator chains of one A fragment, and the gate arithmetic of an element (row, j)
// needs nothing from another lane.  h_{t-1} is the A operand, read from LDS (two buffers: one barrier per step); the
// k index is permuted as in gemm_direct.h (k-block of 16: lane (r, g) holds k = 16 kb + 4 g + s for MFMA s), the same
// on both operands, so that a lane's four k of a block are ONE float4 of an h row / a W_hh row.
// Backward: dh_t lives in the accumulator layout in registers; a step writes dGi / dGh, leaves dGh in LDS and carries
// dh_{t-1} = dGh W_hh + dh_t * z_t (K = 3H, two accumulator chains per tile: even and odd k-blocks, added once).
// Where W_hh lives (DESIGN.md "DIEN"): at H 128 the slice a wave needs — 3 gates x 16 columns x 128 k forward, 384 k x
// 16 columns backward — is 96 floats per lane, 192 KB over the block's 512 lanes: held in REGISTERS for the whole loop
// (REGW).  Any other H re-reads W_hh from L2 every step (at most 768 KB, resident in an XCD's L2).  Both forms issue
// the same MFMAs in the same order: bit-identical results.
// Every sum has a fixed order and there are no float atomics: a rerun is bit-identical.
#include "rec_common.h"

namespace rec {
namespace {

constexpr int kGruRows = 16;                      // batch rows of a block
constexpr int kGruWaves = 8;
constexpr int kGruThreads = kGruWaves * kWave;    // one block per CU, 2 waves per SIMD: 256 VGPRs a lane
constexpr int kGruMaxH = 256;                     // the DIN kernels' limit on E
constexpr int kGruTiles = kGruMaxH / 16 / kGruWaves;   // column tiles per wave
constexpr int kGruPad = 4;                        // floats behind an LDS row (rows stay 16-byte aligned)
constexpr int kGruRegH = 128;                     // REGW: this H exactly

__device__ __forceinline__ float dien_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float f4(const float4& v, int s) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; }

// Gi [B,T,3H] (r | z | c columns), W_hh [3H,H], b_hh [3H] -> H_out [B,T,H]; saved (nullable) [B,T,5H] = r | z | c | hc | hp
// with hc = W_hc h + b_hc (the backward's d r needs it) and hp = h_{t-1} (the B operand of the caller's dW_hh GEMM)
template <bool REGW>
__global__ __launch_bounds__(kGruThreads) void gru_seq_fwd_kernel(int64_t B, int T, int H, const float* __restrict__ Gi,
                                                                  const float* __restrict__ Whh,
                                                                  const float* __restrict__ bhh,
                                                                  float* __restrict__ Hout, float* __restrict__ saved) {
  extern __shared__ float4 gru_lds4[];
  float* hs = reinterpret_cast<float*>(gru_lds4);            // [2][16][H + pad]
  const int ld = H + kGruPad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int64_t b0 = (int64_t)blockIdx.x * kGruRows;
  const int nt = (H + 15) / 16, nkb = (H + 15) / 16;
  for (int i = threadIdx.x; i < 2 * kGruRows * ld; i += kGruThreads) hs[i] = 0.f;      // h_0 = 0 (net.py:190)
  float4 wreg[REGW ? 3 : 1][REGW ? kGruRegH / 16 : 1];
  if constexpr (REGW) {
    const int j = wave * 16 + r;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int kb = 0; kb < kGruRegH / 16; ++kb) wreg[q][kb] = ld4(Whh + ((int64_t)q * H + j) * H + 16 * kb + 4 * g);
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float* cur = hs + (t & 1) * kGruRows * ld;
    float* nxt = hs + ((t + 1) & 1) * kGruRows * ld;
#pragma unroll
    for (int i = 0; i < (REGW ? 1 : kGruTiles); ++i) {
      const int jt = wave + i * kGruWaves;
      if (jt >= nt) continue;                               // wave-uniform
      const int j = jt * 16 + r, jc = j < H ? j : H - 1;    // columns behind H are computed on column H-1 and dropped
      float gi[3][4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t b = b0 + 4 * g + v, bc = b < B ? b : B - 1;
        const float* p = Gi + (bc * T + t) * 3 * H + jc;
#pragma unroll
        for (int q = 0; q < 3; ++q) gi[q][v] = p[(int64_t)q * H];
      }
      f32x4 acc[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      auto kblock = [&](int kb, const float4 (&w)[3]) {
        const int kk = 16 * kb + 4 * g;
        const float4 a = kk < H ? ld4(cur + r * ld + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4(a, s), f4(w[q], s), acc[q], 0, 0, 0);
      };
      if constexpr (REGW) {
#pragma unroll
        for (int kb = 0; kb < kGruRegH / 16; ++kb) {
          const float4 w[3] = {wreg[0][kb], wreg[1][kb], wreg[2][kb]};
          kblock(kb, w);
        }
      } else {
        for (int kb = 0; kb < nkb; ++kb) {
          const int kk = 16 * kb + 4 * g;
          float4 w[3];
#pragma unroll
          for (int q = 0; q < 3; ++q)
            w[q] = kk < H ? ld4(Whh + ((int64_t)q * H + jc) * H + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
          kblock(kb, w);
        }
      }
      const float br = bhh[jc], bz = bhh[H + jc], bc_ = bhh[2 * H + jc];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 4 * g + v;
        const float hp = cur[row * ld + jc];
        const float rr = dien_sigmoid(gi[0][v] + (acc[0][v] + br));
        const float zz = dien_sigmoid(gi[1][v] + (acc[1][v] + bz));
        const float hc = acc[2][v] + bc_;
        const float cc = tanhf(gi[2][v] + rr * hc);
        const float hn = zz * hp + (1.f - zz) * cc;
        if (j < H) {
          nxt[row * ld + j] = hn;
          const int64_t b = b0 + row;
          if (b < B) {
            Hout[(b * T + t) * H + j] = hn;
            if (saved) {
              float* sp = saved + (b * T + t) * 5 * H + j;
              sp[0] = rr;
              sp[H] = zz;
              sp[2 * (int64_t)H] = cc;
              sp[3 * (int64_t)H] = hc;
              sp[4 * (int64_t)H] = hp;
            }
          }
        }
      }
    }
    __syncthreads();      // h_t complete before step t+1 reads it; every read of h_{t-1} was issued before
  }
}

// saved [B,T,5H] (the forward's), W_hh [3H,H], dH_out [B,T,H] and dh_T [B,H] (both nullable)
// -> dGi, dGh [B,T,3H]
template <bool REGW>
__global__ __launch_bounds__(kGruThreads) void gru_seq_bwd_kernel(int64_t B, int T, int H, const float* __restrict__ saved,
                                                                  const float* __restrict__ Whh,
                                                                  const float* __restrict__ dHout,
                                                                  const float* __restrict__ dhT, float* __restrict__ dGi,
                                                                  float* __restrict__ dGh) {
  extern __shared__ float4 gru_lds4[];
  float* dg = reinterpret_cast<float*>(gru_lds4);            // [16][3H + pad]: dGh of the step, the A operand
  const int K3 = 3 * H, ld = K3 + kGruPad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int64_t b0 = (int64_t)blockIdx.x * kGruRows;
  const int nt = (H + 15) / 16, nkb = (K3 + 15) / 16;
  constexpr int NT = REGW ? 1 : kGruTiles;
  constexpr int RKB = 3 * kGruRegH / 16;
  float wreg[REGW ? RKB : 1][REGW ? 4 : 1];
  if constexpr (REGW) {
    const int j = wave * 16 + r;
#pragma unroll
    for (int kb = 0; kb < RKB; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) wreg[kb][s] = Whh[(int64_t)(16 * kb + 4 * g + s) * H + j];
  }
  float dh[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = (wave + i * kGruWaves) * 16 + r;
      const int64_t b = b0 + 4 * g + v;
      dh[i][v] = (dhT && j < H && b < B) ? dhT[b * H + j] : 0.f;
    }
  for (int t = T - 1; t >= 0; --t) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int jt = wave + i * kGruWaves;
      if (jt >= nt) continue;
      const int j = jt * 16 + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 4 * g + v;
        const int64_t b = b0 + row, bt = b * T + t;
        const bool live = j < H && b < B;
        float rr = 0.f, zz = 0.f, cc = 0.f, hc = 0.f, hp = 0.f, d = dh[i][v];
        if (live) {
          const float* sp = saved + bt * 5 * H + j;
          rr = sp[0];
          zz = sp[H];
          cc = sp[2 * (int64_t)H];
          hc = sp[3 * (int64_t)H];
          hp = sp[4 * (int64_t)H];
          if (dHout) d += dHout[bt * H + j];
        }
        const float dz = d * (hp - cc) * zz * (1.f - zz);      // through z
        const float dc = d * (1.f - zz) * (1.f - cc * cc);     // through tanh: the c columns of dGi
        const float dr = dc * hc * rr * (1.f - rr);            // through r
        const float dchh = dc * rr;                            // the c columns of dGh
        if (live) {
          float* pi = dGi + bt * K3 + j;
          float* ph = dGh + bt * K3 + j;
          pi[0] = dr;
          pi[H] = dz;
          pi[2 * (int64_t)H] = dc;
          ph[0] = dr;
          ph[H] = dz;
          ph[2 * (int64_t)H] = dchh;
        }
        if (j < H) {                                           // rows behind B hold zeros
          dg[row * ld + j] = dr;
          dg[row * ld + H + j] = dz;
          dg[row * ld + 2 * H + j] = dchh;
        }
        dh[i][v] = d * zz;
      }
    }
    __syncthreads();
    if (t > 0) {                                               // dh_{t-1} = dGh_t W_hh + dh_t * z_t
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const int jt = wave + i * kGruWaves;
        if (jt >= nt) continue;
        const int j = jt * 16 + r, jc = j < H ? j : H - 1;
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        auto kblock = [&](int kb, const float (&w)[4], f32x4& a_) {
          const int kk = 16 * kb + 4 * g;
          const float4 a = kk < K3 ? ld4(dg + r * ld + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int s = 0; s < 4; ++s) a_ = __builtin_amdgcn_mfma_f32_16x16x4f32(f4(a, s), w[s], a_, 0, 0, 0);
        };
        if constexpr (REGW) {
#pragma unroll
          for (int kb = 0; kb < RKB; ++kb) kblock(kb, wreg[kb], acc[kb & 1]);
        } else {
          for (int kb = 0; kb < nkb; kb += 2) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              if (kb + u >= nkb) break;
              const int kk = 16 * (kb + u) + 4 * g;
              float w[4];
#pragma unroll
              for (int s = 0; s < 4; ++s) w[s] = kk < K3 ? Whh[(int64_t)(kk + s) * H + jc] : 0.f;
              kblock(kb + u, w, acc[u]);
            }
          }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) dh[i][v] += acc[0][v] + acc[1][v];
      }
    }
    __syncthreads();      // the MFMAs' reads of dg are done before the next step overwrites it
  }
}

// ---------------------------------------------------------------- fixed-order block sum (kBlock threads)
__device__ __forceinline__ float dien_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float dien_block_max(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const float s = red[0];
  __syncthreads();
  return s;
}

// ---------------------------------------------------------------- auxiliary loss
struct AuxArgs {
  int64_t n;                    // B * T
  int T, H, Ei;
  const float* gru_out;         // [B,T,H]
  const float* hist;            // [B,T,H] gathered rows
  const int64_t* neg_item;      // [B,T]
  const int64_t* neg_cat;
  const float* Wi; int si; int64_t Ni;
  const float* Wc; int sc; int64_t Nc;
  int64_t pad;
  int32_t* status;
};

// row of id in a table, or nullptr where the id reads as zero (padding row, or out of range: flagged)
__device__ __forceinline__ const float* aux_row(int64_t id, const float* W, int stride, int64_t N, int64_t pad, int lane,
                                                int32_t* status) {
  if (id == pad && pad >= 0) return nullptr;
  if (id < 0 || id >= N) {
    if (lane == 0) atomicOr(status, REC_FLAG_INDEX_OOB);
    return nullptr;
  }
  return W + id * stride;
}

// one wave per (b, t): p = gru_out[b,t] . hist[b,t+1], n = gru_out[b,t] . neg[b,t+1]; every lane returns both
__device__ __forceinline__ void aux_dots(const AuxArgs& a, int64_t idx, int lane, const float*& ri, const float*& rc, float& p,
                                         float& n) {
  ri = aux_row(a.neg_item[idx + 1], a.Wi, a.si, a.Ni, a.pad, lane, a.status);
  rc = aux_row(a.neg_cat[idx + 1], a.Wc, a.sc, a.Nc, a.pad, lane, a.status);
  float sp = 0.f, sn = 0.f;
  for (int j = lane; j < a.H; j += kWave) {
    const float go = a.gru_out[idx * a.H + j];
    const float nv = j < a.Ei ? (ri ? ri[j] : 0.f) : (rc ? rc[j - a.Ei] : 0.f);
    sp += go * a.hist[(idx + 1) * a.H + j];
    sn += go * nv;
  }
  p = group_sum<kWave>(sp);
  n = group_sum<kWave>(sn);
}

__global__ __launch_bounds__(kBlock) void dien_aux_fwd_kernel(AuxArgs a, float* __restrict__ term) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (idx >= a.n) return;
  if ((int)(idx % a.T) == a.T - 1) {
    if (lane == 0) term[idx] = 0.f;
    return;
  }
  const float *ri, *rc;
  float p, n;
  aux_dots(a, idx, lane, ri, rc, p, n);
  const float nc = fminf(fmaxf(n, -15.f), 15.f);             // net.py:243-249; the clip on p has no bounds (net.py:235)
  if (lane == 0) term[idx] = logf(1e-8f + dien_sigmoid(nc)) + logf(1e-8f + dien_sigmoid(p));
}

// out[0] = scale * sum(term[0 .. n)): thread i adds term[i], term[i + 256], .. in order, then the fixed tree
__global__ __launch_bounds__(kBlock) void dien_aux_reduce_kernel(int64_t n, const float* __restrict__ term, float scale,
                                                                 float* __restrict__ out) {
  __shared__ float red[kBlock];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) s += term[i];
  s = dien_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// wave (b, t), t < T-1: d_gru_out[b,t] = dp hist[b,t+1] + dn neg[b,t+1]; d_hist[b,t+1] (+)= dp gru_out[b,t];
// d_neg[b,t+1] = dn gru_out[b,t].  Wave (b, T-1): d_gru_out[b,T-1] = 0, d_neg[b,0] = 0 (and d_hist[b,0] = 0 unless
// accumulating).  Every element has one writer.
__global__ __launch_bounds__(kBlock) void dien_aux_bwd_kernel(AuxArgs a, float scale, float* __restrict__ d_gru_out,
                                                              float* __restrict__ d_hist, int accumulate,
                                                              float* __restrict__ d_neg) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (idx >= a.n) return;
  const int H = a.H;
  if ((int)(idx % a.T) == a.T - 1) {
    const int64_t first = idx - (a.T - 1);
    for (int j = lane; j < H; j += kWave) {
      d_gru_out[idx * H + j] = 0.f;
      d_neg[first * H + j] = 0.f;
      if (!accumulate) d_hist[first * H + j] = 0.f;
    }
    return;
  }
  const float *ri, *rc;
  float p, n;
  aux_dots(a, idx, lane, ri, rc, p, n);
  const float sp = dien_sigmoid(p), sn = dien_sigmoid(n);
  const float dp = scale * sp * (1.f - sp) / (1e-8f + sp);
  const float dn = (n > -15.f && n < 15.f) ? scale * sn * (1.f - sn) / (1e-8f + sn) : 0.f;
  for (int j = lane; j < H; j += kWave) {
    const float go = a.gru_out[idx * H + j];
    const float nv = j < a.Ei ? (ri ? ri[j] : 0.f) : (rc ? rc[j - a.Ei] : 0.f);
    d_gru_out[idx * H + j] = dp * a.hist[(idx + 1) * H + j] + dn * nv;
    const float dh = dp * go;
    d_hist[(idx + 1) * H + j] = accumulate ? d_hist[(idx + 1) * H + j] + dh : dh;
    d_neg[(idx + 1) * H + j] = dn * go;
  }
}

// ---------------------------------------------------------------- attention features
__global__ __launch_bounds__(kBlock) void dien_att_feat_fwd_kernel(int64_t total, int E, const float* __restrict__ hist,
                                                                   const float* __restrict__ q, float* __restrict__ feat) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t i = idx / E;
  const int e = (int)(idx % E);
  const float h = hist[idx], qq = q[idx];
  float* f = feat + i * 4 * E + e;
  f[0] = h;
  f[E] = qq;
  f[2 * E] = h - qq;
  f[3 * E] = h * qq;
}

__global__ __launch_bounds__(kBlock) void dien_att_feat_bwd_kernel(int64_t total, int E, const float* __restrict__ hist,
                                                                   const float* __restrict__ q,
                                                                   const float* __restrict__ dfeat,
                                                                   float* __restrict__ d_hist, int accumulate,
                                                                   float* __restrict__ d_q) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int64_t i = idx / E;
  const int e = (int)(idx % E);
  const float* f = dfeat + i * 4 * E + e;
  const float d0 = f[0], d1 = f[E], d2 = f[2 * E], d3 = f[3 * E];
  const float dh = (d0 + d2) + d3 * q[idx];
  d_hist[idx] = accumulate ? d_hist[idx] + dh : dh;
  d_q[idx] = (d1 - d2) + d3 * hist[idx];
}

// ---------------------------------------------------------------- softmax over T and the weighting, one block per sample
__global__ __launch_bounds__(kBlock) void dien_attention_seq_fwd_kernel(int T, int E, const float* __restrict__ score,
                                                                        const float* __restrict__ mask,
                                                                        const float* __restrict__ hist, float scale,
                                                                        float* __restrict__ w, float* __restrict__ x_att) {
  __shared__ float red[kBlock];
  const int64_t b = blockIdx.x;
  const float* s = score + b * T;
  const float* m = mask + b * T;
  float mx = -INFINITY;
  for (int t = threadIdx.x; t < T; t += kBlock) mx = fmaxf(mx, (s[t] + m[t]) * scale);
  mx = dien_block_max(mx, red);
  float sum = 0.f;
  for (int t = threadIdx.x; t < T; t += kBlock) sum += expf((s[t] + m[t]) * scale - mx);
  sum = dien_block_sum(sum, red);
  for (int t = threadIdx.x; t < T; t += kBlock) w[b * T + t] = expf((s[t] + m[t]) * scale - mx) / sum;
  __syncthreads();                                         // w of this sample: written by this block, read below
  const int64_t n = (int64_t)T * E;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) x_att[b * n + i] = w[b * T + i / E] * hist[b * n + i];
}

// g_t = dx_att[b,t] . hist[b,t]; dscore_t = scale * w_t (g_t - sum_s w_s g_s); d_hist[b,t] (+)= w_t dx_att[b,t]
__global__ __launch_bounds__(kBlock) void dien_attention_seq_bwd_kernel(int T, int E, const float* __restrict__ w,
                                                                        const float* __restrict__ hist,
                                                                        const float* __restrict__ dx_att, float scale,
                                                                        float* __restrict__ dscore,
                                                                        float* __restrict__ d_hist, int accumulate) {
  __shared__ float red[kBlock];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = (int64_t)T * E;
  for (int t = wave; t < T; t += kBlock / kWave) {
    float s = 0.f;
    for (int e = lane; e < E; e += kWave) s += dx_att[b * n + (int64_t)t * E + e] * hist[b * n + (int64_t)t * E + e];
    s = group_sum<kWave>(s);
    if (lane == 0) dscore[b * T + t] = s;                  // g_t, replaced below
  }
  __syncthreads();
  float sum = 0.f;
  for (int t = threadIdx.x; t < T; t += kBlock) sum += w[b * T + t] * dscore[b * T + t];
  sum = dien_block_sum(sum, red);                          // (its barriers separate the reads of g from the writes below)
  for (int t = threadIdx.x; t < T; t += kBlock) dscore[b * T + t] = scale * (w[b * T + t] * (dscore[b * T + t] - sum));
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {
    const float dh = w[b * T + i / E] * dx_att[b * n + i];
    d_hist[b * n + i] = accumulate ? d_hist[b * n + i] + dh : dh;
  }
}

bool gru_regw(int H) {
  static const bool on = [] { const char* v = getenv("REC_GRU_REGW"); return !(v && *v == '0'); }();
  return on && H == kGruRegH;
}

int gru_check(int64_t B, int32_t T, int32_t H, const char* what) {
  REC_REQUIRE(B >= 0 && T > 0 && H > 0, REC_EINVAL, "%s: bad sizes (batch %lld, steps %d, hidden %d)", what, (long long)B, T,
              H);
  REC_REQUIRE(H % 4 == 0 && H <= kGruMaxH, REC_ESHAPE, "%s: hidden %d unsupported (need a multiple of 4, <= %d)", what, H,
              kGruMaxH);
  REC_REQUIRE((B + kGruRows - 1) / kGruRows < (1ll << 31), REC_ESHAPE, "%s: batch too large", what);
  return REC_OK;
}

int aux_check(int64_t B, int32_t T, int32_t Ei, int32_t Ec, int32_t si, int64_t Ni, int32_t sc, int64_t Nc) {
  REC_REQUIRE(B >= 0 && T > 0 && Ei > 0 && Ec > 0 && si >= Ei && sc >= Ec && Ni > 0 && Nc > 0, REC_EINVAL,
              "dien aux: bad sizes (batch %lld, steps %d, item_dim %d, cat_dim %d, strides %d %d, rows %lld %lld)",
              (long long)B, T, Ei, Ec, si, sc, (long long)Ni, (long long)Nc);
  REC_REQUIRE((B * T + 3) / 4 < (1ll << 31), REC_ESHAPE, "dien aux: batch * steps too large");
  return REC_OK;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_gru_seq_fwd(int64_t batch, int32_t steps, int32_t hidden, const float* Gi, const float* W_hh,
                               const float* b_hh, float* H_out, float* saved, void* stream) {
  int rc = gru_check(batch, steps, hidden, "rec_gru_seq_fwd");
  if (rc != REC_OK) return rc;
  if (batch == 0) return REC_OK;
  REC_REQUIRE(Gi && W_hh && b_hh && H_out, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(((uintptr_t)W_hh) % 16 == 0, REC_EINVAL, "rec_gru_seq_fwd: W_hh must be 16-byte aligned");
  const unsigned grid = (unsigned)((batch + kGruRows - 1) / kGruRows);
  const size_t lds = (size_t)2 * kGruRows * (hidden + kGruPad) * sizeof(float);
  if (gru_regw(hidden))
    hipLaunchKernelGGL(gru_seq_fwd_kernel<true>, dim3(grid), dim3(kGruThreads), lds, (hipStream_t)stream, batch, steps,
                       hidden, Gi, W_hh, b_hh, H_out, saved);
  else
    hipLaunchKernelGGL(gru_seq_fwd_kernel<false>, dim3(grid), dim3(kGruThreads), lds, (hipStream_t)stream, batch, steps,
                       hidden, Gi, W_hh, b_hh, H_out, saved);
  return check_launch("rec_gru_seq_fwd");
}

extern "C" int rec_gru_seq_bwd(int64_t batch, int32_t steps, int32_t hidden, const float* saved, const float* W_hh,
                               const float* dH_out, const float* dh_T, float* dGi, float* dGh, void* stream) {
  int rc = gru_check(batch, steps, hidden, "rec_gru_seq_bwd");
  if (rc != REC_OK) return rc;
  if (batch == 0) return REC_OK;
  REC_REQUIRE(saved && W_hh && dGi && dGh, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(dGi != dGh, REC_EINVAL, "rec_gru_seq_bwd: dGi and dGh are two buffers");
  const unsigned grid = (unsigned)((batch + kGruRows - 1) / kGruRows);
  const size_t lds = (size_t)kGruRows * (3 * hidden + kGruPad) * sizeof(float);
  if (gru_regw(hidden))
    hipLaunchKernelGGL(gru_seq_bwd_kernel<true>, dim3(grid), dim3(kGruThreads), lds, (hipStream_t)stream, batch, steps,
                       hidden, saved, W_hh, dH_out, dh_T, dGi, dGh);
  else
    hipLaunchKernelGGL(gru_seq_bwd_kernel<false>, dim3(grid), dim3(kGruThreads), lds, (hipStream_t)stream, batch, steps,
                       hidden, saved, W_hh, dH_out, dh_T, dGi, dGh);
  return check_launch("rec_gru_seq_bwd");
}

extern "C" int rec_dien_aux_workspace_bytes(int64_t batch, int32_t steps, size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(batch >= 0 && steps > 0, REC_EINVAL, "dien aux: bad sizes (batch %lld, steps %d)", (long long)batch, steps);
  *bytes = (size_t)batch * (size_t)steps * sizeof(float);
  return REC_OK;
}

extern "C" int rec_dien_aux_fwd(int64_t batch, int32_t steps, int32_t item_dim, int32_t cat_dim, const float* gru_out,
                                const float* hist, const int64_t* neg_item, const int64_t* neg_cat, const float* W_neg_item,
                                int32_t item_stride, int64_t item_rows, const float* W_neg_cat, int32_t cat_stride,
                                int64_t cat_rows, int64_t padding_idx, float* aux, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream) {
  int rc = aux_check(batch, steps, item_dim, cat_dim, item_stride, item_rows, cat_stride, cat_rows);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(aux, REC_EINVAL, "null pointer argument");
  const int64_t n = batch * steps;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    REC_REQUIRE(gru_out && hist && neg_item && neg_cat && W_neg_item && W_neg_cat && status, REC_EINVAL,
                "null pointer argument");
    REC_REQUIRE(workspace_bytes >= (size_t)n * sizeof(float), REC_EWORKSPACE, "dien aux workspace %zu < %zu bytes",
                workspace_bytes, (size_t)n * sizeof(float));
    REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
    const AuxArgs a{n, steps, item_dim + cat_dim, item_dim, gru_out, hist, neg_item, neg_cat, W_neg_item, item_stride,
                    item_rows, W_neg_cat, cat_stride, cat_rows, padding_idx, status};
    hipLaunchKernelGGL(dien_aux_fwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kBlock), 0, st, a, (float*)workspace);
    rc = check_launch("rec_dien_aux_fwd");
    if (rc != REC_OK) return rc;
  }
  hipLaunchKernelGGL(dien_aux_reduce_kernel, dim3(1), dim3(kBlock), 0, st, n, (const float*)workspace,
                     batch > 0 ? 1.f / (float)batch : 0.f, aux);
  return check_launch("rec_dien_aux_fwd (reduce)");
}

extern "C" int rec_dien_aux_bwd(int64_t batch, int32_t steps, int32_t item_dim, int32_t cat_dim, const float* gru_out,
                                const float* hist, const int64_t* neg_item, const int64_t* neg_cat, const float* W_neg_item,
                                int32_t item_stride, int64_t item_rows, const float* W_neg_cat, int32_t cat_stride,
                                int64_t cat_rows, int64_t padding_idx, float d_aux, float* d_gru_out, float* d_hist,
                                int32_t accumulate_hist, float* d_neg, int32_t* status, void* stream) {
  int rc = aux_check(batch, steps, item_dim, cat_dim, item_stride, item_rows, cat_stride, cat_rows);
  if (rc != REC_OK) return rc;
  const int64_t n = batch * steps;
  if (n == 0) return REC_OK;
  REC_REQUIRE(gru_out && hist && neg_item && neg_cat && W_neg_item && W_neg_cat && status && d_gru_out && d_hist && d_neg,
              REC_EINVAL, "null pointer argument");
  REC_REQUIRE(d_gru_out != d_hist && d_gru_out != d_neg && d_hist != d_neg, REC_EINVAL,
              "rec_dien_aux_bwd: the three gradients are three buffers");
  const AuxArgs a{n, steps, item_dim + cat_dim, item_dim, gru_out, hist, neg_item, neg_cat, W_neg_item, item_stride,
                  item_rows, W_neg_cat, cat_stride, cat_rows, padding_idx, status};
  hipLaunchKernelGGL(dien_aux_bwd_kernel, dim3((unsigned)((n + 3) / 4)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     d_aux / (float)batch, d_gru_out, d_hist, accumulate_hist, d_neg);
  return check_launch("rec_dien_aux_bwd");
}

extern "C" int rec_dien_att_feat_fwd(int64_t n, int32_t emb_dim, const float* hist, const float* q, float* feat,
                                     void* stream) {
  REC_REQUIRE(n >= 0 && emb_dim > 0, REC_EINVAL, "dien att feat: bad sizes (n %lld, emb_dim %d)", (long long)n, emb_dim);
  if (n == 0) return REC_OK;
  REC_REQUIRE(hist && q && feat, REC_EINVAL, "null pointer argument");
  const int64_t total = n * emb_dim, grid = (total + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "dien att feat: n too large");
  hipLaunchKernelGGL(dien_att_feat_fwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, total, emb_dim,
                     hist, q, feat);
  return check_launch("rec_dien_att_feat_fwd");
}

extern "C" int rec_dien_att_feat_bwd(int64_t n, int32_t emb_dim, const float* hist, const float* q, const float* dfeat,
                                     float* d_hist, int32_t accumulate_hist, float* d_q, void* stream) {
  REC_REQUIRE(n >= 0 && emb_dim > 0, REC_EINVAL, "dien att feat: bad sizes (n %lld, emb_dim %d)", (long long)n, emb_dim);
  if (n == 0) return REC_OK;
  REC_REQUIRE(hist && q && dfeat && d_hist && d_q, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(d_hist != d_q, REC_EINVAL, "rec_dien_att_feat_bwd: d_hist and d_q are two buffers");
  const int64_t total = n * emb_dim, grid = (total + kBlock - 1) / kBlock;
  REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "dien att feat: n too large");
  hipLaunchKernelGGL(dien_att_feat_bwd_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, total, emb_dim,
                     hist, q, dfeat, d_hist, accumulate_hist, d_q);
  return check_launch("rec_dien_att_feat_bwd");
}

extern "C" int rec_dien_attention_seq_fwd(int64_t batch, int32_t steps, int32_t emb_dim, const float* score,
                                          const float* mask, const float* hist, float scale, float* w, float* x_att,
                                          void* stream) {
  REC_REQUIRE(batch >= 0 && steps > 0 && emb_dim > 0, REC_EINVAL, "dien attention seq: bad sizes (batch %lld, steps %d, emb_dim %d)",
              (long long)batch, steps, emb_dim);
  REC_REQUIRE(batch < (1ll << 31), REC_ESHAPE, "dien attention seq: batch too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(score && mask && hist && w && x_att, REC_EINVAL, "null pointer argument");
  hipLaunchKernelGGL(dien_attention_seq_fwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps,
                     emb_dim, score, mask, hist, scale, w, x_att);
  return check_launch("rec_dien_attention_seq_fwd");
}

extern "C" int rec_dien_attention_seq_bwd(int64_t batch, int32_t steps, int32_t emb_dim, const float* w, const float* hist,
                                          const float* dx_att, float scale, float* dscore, float* d_hist,
                                          int32_t accumulate_hist, void* stream) {
  REC_REQUIRE(batch >= 0 && steps > 0 && emb_dim > 0, REC_EINVAL, "dien attention seq: bad sizes (batch %lld, steps %d, emb_dim %d)",
              (long long)batch, steps, emb_dim);
  REC_REQUIRE(batch < (1ll << 31), REC_ESHAPE, "dien attention seq: batch too large");
  if (batch == 0) return REC_OK;
  REC_REQUIRE(w && hist && dx_att && dscore && d_hist, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(d_hist != dx_att, REC_EINVAL, "rec_dien_attention_seq_bwd: d_hist must not be dx_att");
  hipLaunchKernelGGL(dien_attention_seq_bwd_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, steps,
                     emb_dim, w, hist, dx_att, scale, dscore, d_hist, accumulate_hist);
  return check_launch("rec_dien_attention_seq_bwd");
}
