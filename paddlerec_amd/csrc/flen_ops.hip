// FLEN (rank/flen), gfx950: the field-wise bi-interaction fused into the lookup, its backward in place on the layer-0 dX,
// and paddle.optimizer.Adagrad for sparse rows and for the flat dense buffer.
//
//   rec_flen_fwd      <- X0 = [E_0 | .. | E_{S-1}] (the DNN input), FW[g] = sum of the lookups of field group g and
//                        h_mf = sum over the group pairs i < j of kernel_mf[p] * FW[i] * FW[j]   (flen/net.py:79, 205-229)
//   rec_flen_bwd      <- rg[b,s] = dX0[b,s] + dH[b] * sum_{g' != g(s)} kernel_mf[pair] * FW[b,g'], in place on dX0, and
//                        d_kernel_mf[p] = sum_{b,d} dH * FW_i * FW_j
//   rec_adagrad_rows  <- acc += g*g; p -= lr * g / (sqrt(acc) + eps) on the MERGED gradient of every touched row
//   rec_adagrad_dense <- the same rule over a flat buffer
// A block owns whole samples: it takes `sb` consecutive samples at a time, so the group sums of a sample never leave the
// block.  The lookups use the row groups of emb_ops.hip (LANES lanes per lookup, VEC floats per lane: a D = 32 row is eight
// 16-byte loads); every row goes to X0 and to an LDS tile, and the group sums, the pair products and the backward's
// per-group factor are then formed from LDS by one thread per output float in slot order.  The partition of the slots is
// a launch argument; a thread never indexes registers by group (the bounds are copied to LDS once), so the kernels keep
// no scratch.  d_kernel_mf is summed without float atomics: a thread owns (pair, one of kFlenSub column subsets), walks
// the block's fixed set of sample chunks in order, the subsets add up in order, and a fold kernel adds the blocks'
// partials in block order: two runs on the same inputs give the same bits.
#include "rec_common.h"
#include "segment_sum.h"

namespace rec {
namespace {

constexpr int kFlenMaxGroups = REC_FLEN_MAX_GROUPS;
constexpr int kFlenMaxPairs = kFlenMaxGroups * (kFlenMaxGroups - 1) / 2;
constexpr int kFlenSub = 8;                        // column subsets per pair: kFlenMaxPairs * kFlenSub <= kBlock
constexpr int kFlenBwdMaxBlocks = kNumCU * 8;      // 8 blocks of 256 threads per CU: 8 waves per SIMD
constexpr int kFlenTileFloats = 4096;              // 16 KB of LDS per block for the tile and the group sums
constexpr int kFlenFoldGroups = kBlock / 32;
static_assert(kFlenMaxPairs * kFlenSub <= kBlock && kFlenMaxPairs <= 32, "one thread per (pair, subset)");

struct FlenBounds {
  int b[kFlenMaxGroups + 1];
};

// the bounds and kernel_mf into LDS (the caller's barrier follows)
__device__ __forceinline__ void flen_load_consts(int G, const FlenBounds& gb, const float* __restrict__ kmf, int* sgb,
                                                 float* skmf) {
  if (threadIdx.x <= kFlenMaxGroups) {
    int v = 0;
#pragma unroll
    for (int k = 0; k <= kFlenMaxGroups; ++k)
      if ((int)threadIdx.x == k) v = gb.b[k];
    sgb[threadIdx.x] = v;
  }
  if ((int)threadIdx.x < G * (G - 1) / 2) skmf[threadIdx.x] = kmf[threadIdx.x];
}

__device__ __forceinline__ int flen_pair(int i, int j, int G) { return i * (2 * G - i - 1) / 2 + (j - i - 1); }  // i < j

template <int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void flen_fwd_kernel(
    int64_t B, int S, int G, int D, int stride, int64_t N, int sb_max, FlenBounds gb, const int64_t* __restrict__ ids,
    const float* __restrict__ W, const float* __restrict__ kmf, float* __restrict__ X0, int64_t ld_x0,
    float* __restrict__ H, int64_t ld_h, float* __restrict__ FW, int32_t* __restrict__ status) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sgb[kFlenMaxGroups + 1];
  __shared__ float skmf[kFlenMaxPairs];
  constexpr int R = kBlock / LANES;
  float* tile = smem;                          // [sb][S][D]: the chunk's lookups
  float* fw = smem + sb_max * S * D;           // [sb][G][D]: its group sums
  flen_load_consts(G, gb, kmf, sgb, skmf);
  const int64_t b0 = (int64_t)blockIdx.x * sb_max;
  const int nb = (int)(B - b0 < sb_max ? B - b0 : sb_max);
  const int r = threadIdx.x / LANES, lg = threadIdx.x % LANES;
  const int d0 = lg * VEC;
  if (d0 < D) {
    for (int q = r; q < nb * S; q += R) {
      const int64_t id = ids[b0 * S + q];
      float e[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) e[v] = 0.f;
      if (id >= 0 && id < N)
        vload<VEC>(e, W + id * stride + d0);
      else if (lg == 0)
        atomicOr(status, REC_FLAG_INDEX_OOB);
      const int sb = q / S, s = q - sb * S;
      vstore<VEC>(X0 + (b0 + sb) * ld_x0 + (int64_t)s * D + d0, e);
      vstore<VEC>(tile + q * D + d0, e);
    }
  }
  __syncthreads();
  for (int it = threadIdx.x; it < nb * G * D; it += kBlock) {      // it = (sb * G + g) * D + d
    const int d = it % D, g = (it / D) % G, sb = it / (D * G);
    const float* col = tile + sb * S * D + d;
    float sum = 0.f;
    for (int s = sgb[g]; s < sgb[g + 1]; ++s) sum += col[s * D];
    fw[it] = sum;
    FW[b0 * G * D + it] = sum;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < nb * D; it += kBlock) {
    const int d = it % D, sb = it / D;
    const float* f = fw + sb * G * D + d;
    float h = 0.f;
    int p = 0;
    for (int i = 0; i < G; ++i)
      for (int j = i + 1; j < G; ++j, ++p) h += skmf[p] * f[i * D] * f[j * D];
    H[(b0 + sb) * ld_h + d] = h;
  }
}

// A block takes the chunks blockIdx.x, blockIdx.x + gridDim.x, .. of sb_max samples.  The many uniform values (bounds,
// eight pointers, strides) would take 106 SGPRs, which is 7 waves per SIMD; capped at 96 the surplus lives in VGPR lanes
// (no scratch) and the kernel keeps the 8 waves of the other lookup kernels.
template <int VEC, int LANES>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(96))) void flen_bwd_kernel(
    int64_t B, int S, int G, int D, int64_t N, int sb_max, FlenBounds gb, const int64_t* __restrict__ ids,
    const float* __restrict__ FW, const float* __restrict__ kmf, const float* __restrict__ dH, int64_t ld_dh,
    float* __restrict__ g, int64_t g_stride, float* __restrict__ part, int32_t* __restrict__ status) {
  extern __shared__ __align__(16) float smem[];
  __shared__ int sgb[kFlenMaxGroups + 1];
  __shared__ float skmf[kFlenMaxPairs];
  __shared__ float red[kFlenMaxPairs * kFlenSub];
  constexpr int R = kBlock / LANES;
  float* fw = smem;                            // [sb][G][D]
  float* tf = fw + sb_max * G * D;             // [sb][G][D]: sum over g' != g of kernel_mf[pair] * FW[g']
  float* dh = tf + sb_max * G * D;             // [sb][D]
  flen_load_consts(G, gb, kmf, sgb, skmf);
  const int P = G * (G - 1) / 2;
  const int p = threadIdx.x / kFlenSub, sub = threadIdx.x % kFlenSub;
  int pi = 0, pj = 1;                          // the groups of pair p
  for (int k = 0; k < p && p < P; ++k)
    if (++pj == G) pj = ++pi + 1;
  float acc = 0.f;
  const int r = threadIdx.x / LANES, lg = threadIdx.x % LANES;
  const int d0 = lg * VEC;
  const int64_t chunks = (B + sb_max - 1) / sb_max;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t b0 = c * sb_max;
    const int nb = (int)(B - b0 < sb_max ? B - b0 : sb_max);
    for (int it = threadIdx.x; it < nb * G * D; it += kBlock) fw[it] = FW[b0 * G * D + it];
    for (int it = threadIdx.x; it < nb * D; it += kBlock) dh[it] = dH[(b0 + it / D) * ld_dh + it % D];
    __syncthreads();                           // also orders the constants' stores before their first use
    for (int it = threadIdx.x; it < nb * G * D; it += kBlock) {
      const int d = it % D, gi = (it / D) % G, sb = it / (D * G);
      const float* f = fw + sb * G * D + d;
      float sum = 0.f;
      for (int o = 0; o < G; ++o)
        if (o != gi) sum += skmf[o < gi ? flen_pair(o, gi, G) : flen_pair(gi, o, G)] * f[o * D];
      tf[it] = sum;
    }
    if (p < P)
      for (int j = sub; j < nb * D; j += kFlenSub) {
        const float* f = fw + (j / D) * G * D + j % D;
        acc += dh[j] * f[pi * D] * f[pj * D];
      }
    __syncthreads();
    if (d0 < D) {
      for (int q = r; q < nb * S; q += R) {
        const int64_t id = ids[b0 * S + q];
        const int sb = q / S, s = q - sb * S;
        int gi = 0;
        for (int k = 1; k < G; ++k) gi += s >= sgb[k];
        float* slot = g + (b0 + sb) * g_stride + (int64_t)s * D + d0;
        float gr[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) gr[v] = 0.f;
        if (id >= 0 && id < N) {
          float a[VEC], t[VEC];
          vload<VEC>(gr, slot);
          vload<VEC>(a, dh + sb * D + d0);
          vload<VEC>(t, tf + (sb * G + gi) * D + d0);
#pragma unroll
          for (int v = 0; v < VEC; ++v) gr[v] += a[v] * t[v];
        } else if (lg == 0) {
          atomicOr(status, REC_FLAG_INDEX_OOB);
        }
        vstore<VEC>(slot, gr);
      }
    }
    __syncthreads();                           // the next chunk overwrites the LDS
  }
  if (p < P) red[threadIdx.x] = acc;
  __syncthreads();
  if ((int)threadIdx.x < P) {
    float t = red[threadIdx.x * kFlenSub];
    for (int k = 1; k < kFlenSub; ++k) t += red[threadIdx.x * kFlenSub + k];
    part[(int64_t)blockIdx.x * P + threadIdx.x] = t;
  }
}

// d_kmf[p] = part[0][p] + part[1][p] + ..: 8 groups take every 8th block in order, then the groups add up in order
// (blocks == 0 writes zeros)
__global__ __launch_bounds__(kBlock) void flen_fold_kernel(int blocks, int P, const float* __restrict__ part,
                                                           float* __restrict__ d_kmf) {
  __shared__ float red[kFlenFoldGroups][32];
  const int p = threadIdx.x % 32, grp = threadIdx.x / 32;
  float sum = 0.f;
  if (p < P)
    for (int b = grp; b < blocks; b += kFlenFoldGroups) sum += part[(int64_t)b * P + p];
  red[grp][p] = sum;
  __syncthreads();
  if (grp == 0 && p < P) {
    float t = red[0][p];
    for (int i = 1; i < kFlenFoldGroups; ++i) t += red[i][p];
    d_kmf[p] = t;
  }
}

// paddle.optimizer.Adagrad on one element, rounding points pinned (no compiler-chosen fma contraction).  g == 0 leaves
// both values bit-unchanged.
__device__ __forceinline__ void adagrad_elem(float& p, float& a, float g, float lr, float eps) {
#pragma clang fp contract(off)
  const float g2 = g * g;
  a = a + g2;
  const float num = lr * g;
  const float den = sqrtf(a) + eps;
  p = p - num / den;
}

template <int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void adagrad_rows_kernel(
    int D, int stride, int sstride, const int32_t* __restrict__ n_uniq, const int64_t* __restrict__ uniq,
    const int32_t* __restrict__ seg_off, const int32_t* __restrict__ spos, const float* __restrict__ grad,
    rec_grad_layout gl, float* __restrict__ P, float* __restrict__ A, float lr, float eps) {
  constexpr int WL = row_lanes<LANES>();
  const int64_t u = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / WL;
  const int dl = (threadIdx.x % WL) * VEC;
  if (u >= n_uniq[0] || dl >= D) return;
  const int64_t row = uniq[u];
  const int beg = seg_off[u], end = seg_off[u + 1];
#pragma unroll
  for (int pass = 0; pass < row_passes<LANES>(); ++pass) {
    const int d0 = dl + pass * WL * VEC;
    if (pass > 0 && d0 >= D) return;
    float p[VEC], a[VEC], g[VEC];
    const int64_t ro = row * stride + d0, so = row * sstride + d0;
    vload<VEC>(p, P + ro);
    vload<VEC>(a, A + so);
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] = 0.f;
    segment_sum<VEC>(g, beg, end, spos, grad, gl, D, d0);      // the merged gradient: (sum g)^2, not sum g^2
#pragma unroll
    for (int i = 0; i < VEC; ++i) adagrad_elem(p[i], a[i], g[i], lr, eps);
    vstore<VEC>(P + ro, p);
    vstore<VEC>(A + so, a);
  }
}

__global__ __launch_bounds__(kBlock) void adagrad_dense_kernel(int64_t n, float* __restrict__ p, float* __restrict__ a,
                                                               const float* __restrict__ g, float lr, float eps) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    float pv = p[i], av = a[i];
    adagrad_elem(pv, av, g[i], lr, eps);
    p[i] = pv;
    a[i] = av;
  }
}

// samples a block takes at a time: as many as fit kFlenTileFloats of LDS, at most 8; 0 = one sample does not fit 64 KB
int flen_sb(int S, int G, int D) {
  const int64_t per = (int64_t)(S + G + 1) * D;      // forward: tile + group sums; the backward's (2G + 1) * D is no more
  if (per * (int64_t)sizeof(float) > 64 * 1024) return 0;
  const int64_t sb = kFlenTileFloats / per;
  return sb < 1 ? 1 : sb > 8 ? 8 : (int)sb;
}

int flen_check(int64_t B, int32_t S, int32_t G, int32_t D, const int32_t* group_begin, FlenBounds* gb, int* sb) {
  REC_REQUIRE(B >= 0 && D > 0 && G >= 2 && G <= kFlenMaxGroups && S >= G, REC_EINVAL,
              "flen: bad sizes (batch %lld, num_slots %d, num_groups %d (2..%d), emb_dim %d)", (long long)B, S, G,
              kFlenMaxGroups, D);
  REC_REQUIRE(group_begin, REC_EINVAL, "flen: group_begin is null");
  REC_REQUIRE(group_begin[0] == 0 && group_begin[G] == S, REC_EINVAL,
              "flen: group_begin must run from 0 to num_slots %d (got %d .. %d)", S, group_begin[0], group_begin[G]);
  for (int k = 0; k <= kFlenMaxGroups; ++k) gb->b[k] = k <= G ? group_begin[k] : S;
  for (int k = 0; k < G; ++k)
    REC_REQUIRE(group_begin[k] < group_begin[k + 1], REC_EINVAL, "flen: group %d is empty or group_begin decreases", k);
  *sb = flen_sb(S, G, D);
  REC_REQUIRE(*sb > 0, REC_ESHAPE, "flen: (num_slots + num_groups + 1) * emb_dim = %lld floats of one sample exceed 64 KB",
              (long long)(S + G + 1) * D);
  REC_REQUIRE(B * S < (1ll << 31), REC_ESHAPE, "flen: batch * num_slots too large");
  return REC_OK;
}

bool flen_vec_ok(const void* p, int64_t ld) { return ((uintptr_t)p) % 16 == 0 && ld % 4 == 0; }

int64_t flen_bwd_grid(int64_t B, int sb) {            // a function of the shape alone: the chunk sets of the partials are fixed
  const int64_t chunks = (B + sb - 1) / sb;
  return chunks < kFlenBwdMaxBlocks ? chunks : kFlenBwdMaxBlocks;
}

}  // namespace
}  // namespace rec

using namespace rec;

extern "C" int rec_flen_fwd(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim, int32_t row_stride,
                            int64_t num_rows, const int64_t* ids, const float* W, const int32_t* group_begin,
                            const float* kernel_mf, float* X0, int64_t x0_stride, float* h_mf, int64_t h_stride, float* FW,
                            int32_t* status, void* stream) {
  FlenBounds gb;
  int sb = 0;
  int rc = flen_check(batch, num_slots, num_groups, emb_dim, group_begin, &gb, &sb);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(row_stride >= emb_dim && num_rows > 0, REC_EINVAL, "flen: bad table (row_stride %d, num_rows %lld)",
              row_stride, (long long)num_rows);
  REC_REQUIRE(x0_stride >= (int64_t)num_slots * emb_dim && h_stride >= emb_dim, REC_EINVAL,
              "flen: x0_stride %lld < num_slots * emb_dim or h_stride %lld < emb_dim", (long long)x0_stride,
              (long long)h_stride);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(ids && W && kernel_mf && X0 && h_mf && FW && status, REC_EINVAL, "null pointer argument");
  const bool vec = flen_vec_ok(W, row_stride) && flen_vec_ok(X0, x0_stride);
  return dispatch_row_shape(emb_dim, vec ? row_stride : row_stride | 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    const int64_t grid = (batch + sb - 1) / sb;
    const size_t lds = (size_t)sb * (num_slots + num_groups) * emb_dim * sizeof(float);
    hipLaunchKernelGGL((flen_fwd_kernel<VEC, LANES>), dim3((unsigned)grid), dim3(kBlock), lds, (hipStream_t)stream, batch,
                       num_slots, num_groups, emb_dim, row_stride, num_rows, sb, gb, ids, W, kernel_mf, X0, x0_stride,
                       h_mf, h_stride, FW, status);
    return check_launch("rec_flen_fwd");
  });
}

extern "C" int rec_flen_bwd_workspace_bytes(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim,
                                            size_t* bytes) {
  REC_REQUIRE(bytes, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(batch >= 0 && emb_dim > 0 && num_groups >= 2 && num_groups <= kFlenMaxGroups && num_slots >= num_groups,
              REC_EINVAL, "flen: bad sizes (batch %lld, num_slots %d, num_groups %d, emb_dim %d)", (long long)batch,
              num_slots, num_groups, emb_dim);
  const int sb = flen_sb(num_slots, num_groups, emb_dim);
  REC_REQUIRE(sb > 0, REC_ESHAPE, "flen: one sample exceeds 64 KB of LDS");
  *bytes = (size_t)flen_bwd_grid(batch, sb) * (size_t)(num_groups * (num_groups - 1) / 2) * sizeof(float);
  return REC_OK;
}

extern "C" int rec_flen_bwd(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim, int64_t num_rows,
                            const int64_t* ids, const int32_t* group_begin, const float* kernel_mf, const float* FW,
                            const float* dH, int64_t dh_stride, float* g, int64_t g_stride, float* d_kernel_mf,
                            int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  FlenBounds gb;
  int sb = 0;
  int rc = flen_check(batch, num_slots, num_groups, emb_dim, group_begin, &gb, &sb);
  if (rc != REC_OK) return rc;
  REC_REQUIRE(num_rows > 0 && g_stride >= (int64_t)num_slots * emb_dim && dh_stride >= emb_dim, REC_EINVAL,
              "flen: num_rows %lld, g_stride %lld < num_slots * emb_dim or dh_stride %lld < emb_dim", (long long)num_rows,
              (long long)g_stride, (long long)dh_stride);
  REC_REQUIRE(d_kernel_mf, REC_EINVAL, "null pointer argument");
  const int P = num_groups * (num_groups - 1) / 2;
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {                                  // an empty batch sum
    hipLaunchKernelGGL(flen_fold_kernel, dim3(1), dim3(kBlock), 0, st, 0, P, (const float*)nullptr, d_kernel_mf);
    return check_launch("rec_flen_bwd (fold)");
  }
  REC_REQUIRE(ids && kernel_mf && FW && dH && g && status, REC_EINVAL, "null pointer argument");
  REC_REQUIRE((const float*)g != FW && (const float*)g != dH, REC_EINVAL, "flen: g must not be FW or dH");
  const int grid = (int)flen_bwd_grid(batch, sb);
  const size_t need = (size_t)grid * (size_t)P * sizeof(float);
  REC_REQUIRE(workspace_bytes >= need, REC_EWORKSPACE, "flen bwd workspace %zu < %zu bytes", workspace_bytes, need);
  REC_REQUIRE(workspace, REC_EINVAL, "null pointer argument");
  float* part = (float*)workspace;
  const bool vec = flen_vec_ok(g, g_stride);
  rc = dispatch_row_shape(emb_dim, vec ? 4 : 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    const size_t lds = (size_t)sb * (2 * num_groups + 1) * emb_dim * sizeof(float);
    hipLaunchKernelGGL((flen_bwd_kernel<VEC, LANES>), dim3((unsigned)grid), dim3(kBlock), lds, st, batch, num_slots,
                       num_groups, emb_dim, num_rows, sb, gb, ids, FW, kernel_mf, dH, dh_stride, g, g_stride, part, status);
    return check_launch("rec_flen_bwd");
  });
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(flen_fold_kernel, dim3(1), dim3(kBlock), 0, st, grid, P, part, d_kernel_mf);
  return check_launch("rec_flen_bwd (fold)");
}

extern "C" int rec_adagrad_rows(int64_t n_max, int32_t emb_dim, int32_t row_stride, int32_t state_stride,
                                const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                                const int32_t* sorted_pos, const float* grad, const rec_grad_layout* grad_layout, float* P,
                                float* A, float lr, float epsilon, void* stream) {
  rec_grad_layout gl = {1, 0, 0, nullptr, nullptr};
  if (grad_layout) gl = *grad_layout;
  REC_REQUIRE(n_max >= 0 && emb_dim > 0 && row_stride >= emb_dim && gl.div >= 1, REC_EINVAL, "bad sizes");
  REC_REQUIRE(gl.group <= 0 || gl.group_stride >= (int64_t)gl.group * emb_dim, REC_EINVAL, "grad group_stride too small");
  REC_REQUIRE(((uintptr_t)gl.partials) % 16 == 0, REC_EINVAL, "grad_layout.partials must be 16-byte aligned");
  if (state_stride <= 0) state_stride = row_stride;
  REC_REQUIRE(state_stride >= emb_dim, REC_EINVAL, "state_stride < emb_dim");
  REC_REQUIRE(n_uniq && uniq_rows && seg_offset && sorted_pos && grad && P && A, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(P != A, REC_EINVAL, "rec_adagrad_rows: the accumulator must not be the table");
  REC_REQUIRE(epsilon >= 0.f, REC_EINVAL, "rec_adagrad_rows: epsilon %g < 0", (double)epsilon);
  if (n_max == 0) return REC_OK;
  // float4 rows need 16-byte aligned gradient, table and accumulator rows
  const bool gvec = ((uintptr_t)grad) % 16 == 0 && (gl.group <= 0 || gl.group_stride % 4 == 0);
  const bool vec = gvec && flen_vec_ok(P, row_stride) && flen_vec_ok(A, state_stride);
  return dispatch_row_shape_wide(emb_dim, vec ? 4 : 1, [&](auto vec_, auto lanes) -> int {
    constexpr int VEC = decltype(vec_)::value, LANES = decltype(lanes)::value;
    const int64_t grid = (n_max * row_lanes<LANES>() + kBlock - 1) / kBlock;
    REC_REQUIRE(grid < (1ll << 31), REC_ESHAPE, "too many rows");
    hipLaunchKernelGGL((adagrad_rows_kernel<VEC, LANES>), dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream,
                       emb_dim, row_stride, state_stride, n_uniq, uniq_rows, seg_offset, sorted_pos, grad, gl, P, A, lr,
                       epsilon);
    return check_launch("rec_adagrad_rows");
  });
}

extern "C" int rec_adagrad_dense(int64_t n, float* p, float* acc, const float* g, float lr, float epsilon, void* stream) {
  REC_REQUIRE(n >= 0 && epsilon >= 0.f, REC_EINVAL, "rec_adagrad_dense: bad arguments (n %lld, epsilon %g)", (long long)n,
              (double)epsilon);
  if (n == 0) return REC_OK;
  REC_REQUIRE(p && acc && g, REC_EINVAL, "null pointer argument");
  REC_REQUIRE(p != acc && (const float*)p != g && (const float*)acc != g, REC_EINVAL,
              "rec_adagrad_dense: p, acc and g must be three buffers");
  int64_t grid = (n + kBlock - 1) / kBlock;
  if (grid > kNumCU * 8) grid = kNumCU * 8;
  hipLaunchKernelGGL(adagrad_dense_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, n, p, acc, g, lr,
                     epsilon);
  return check_launch("rec_adagrad_dense");
}
