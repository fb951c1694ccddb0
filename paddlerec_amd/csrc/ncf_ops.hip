// NCF (models/recall/ncf): NeuMF, GMF and MLP.  The dense side of the shipped net is 2 761 floats and a sample reads 40 floats
// from each of two tables, so a step made of gathers, GEMMs, a head and their backward is a chain of launches that each do
// microseconds of work.  Here the whole net lives in LDS and a step is ONE launch (plus a small fold):
//
//   ncf_net_kernel<true>    stages all weights in LDS once per block; per tile of REC_NCF_TILE samples: gathers the two packed
//                           rows, runs the tower, the head, the log loss and the whole backward from LDS, writes pred and the
//                           per-sample row gradients, and accumulates the dense gradients in LDS (one owner thread per
//                           element, samples in ascending order).  Block b takes the tiles b, b + G, ...; at the end it
//                           writes its accumulators and its loss sum as partials[b].
//   ncf_fold_kernel         g_dense and the loss: the partials added in ascending block order
//   ncf_net_kernel<false>   the forward alone (rec_ncf_score)
//   ncf_gather_fwd_kernel / ncf_gather_bwd_kernel   the glue of the general route (towers the LDS cannot hold)
//
// LDS: the weights keep the dense buffer's flat layout ([in, out] rows), a tile's activations and deltas have an ODD pitch.
// Forward and dW run with the output column fastest over the lanes (weights: consecutive banks; activations: a broadcast),
// the delta pass with the sample fastest (weights: a broadcast; deltas: an odd pitch, distinct banks).
// No float atomics: the only atomic is the OR into the integer status word.
#include <math.h>

#include "rec_common.h"

namespace rec {
namespace {

constexpr int kNcfTile = REC_NCF_TILE;
constexpr int kNcfMaxWidths = REC_NCF_MAX_FC + 1;

// The five "desc" arguments of every entry, gathered (widths: as many as the entry reads)
struct rec_ncf_desc {
  int32_t mf_dim, n_fc;
  int32_t widths[kNcfMaxWidths];
  int64_t num_users, num_items;
};
constexpr float kNcfEps = 1e-4f;                              // Paddle's log_loss epsilon

// Where everything is, worked out on the host from a rec_ncf_desc (ncf_plan) and passed to the kernels by value.
struct NcfPlan {
  int mf, nfc, half, cu;                                      // cu = mf + half: the width of a packed row (users and items)
  int w[kNcfMaxWidths];
  int woff[kNcfMaxWidths], boff[kNcfMaxWidths];     // dense buffer: W_l and b_l, l = 1..nfc
  int poff, pboff, pw, P;                                     // prediction.weight, .bias, its width; the buffer's length
  int apitch[kNcfMaxWidths], aoff[kNcfMaxWidths];   // tile: activations a_l [T][apitch], l = 0..nfc
  int doff[kNcfMaxWidths];                               // tile: deltas d_l [T][apitch[l]], l = 1..nfc
  int mfpitch, mfu_off, mfi_off, dz_off, cost_off, id_off;    // tile: MF rows, dz [T], cost [T], ids [2][T] int64
  int tile_floats;
};

inline int pad4(int n) { return (n + 3) & ~3; }

// The layout of include/recengine.h.  Returns NULL or the name of what is wrong with the desc.
const char* ncf_plan(const rec_ncf_desc* d, NcfPlan* p, bool gather_only) {
  if (d->mf_dim < 0 || d->n_fc < 0) return "mf_dim / n_fc negative";
  if (d->mf_dim == 0 && d->n_fc == 0) return "mf_dim and n_fc both 0";
  if (d->num_users < 1 || d->num_items < 1) return "num_users / num_items";
  p->mf = d->mf_dim;
  p->nfc = d->n_fc;
  p->half = 0;
  if (d->n_fc > 0) {
    if (d->widths[0] < 2 || d->widths[0] % 2 != 0) return "widths[0] must be even and positive";
    p->half = d->widths[0] / 2;
  }
  p->cu = p->mf + p->half;
  if (gather_only) return nullptr;
  if (d->n_fc > REC_NCF_MAX_FC) return nullptr;               // not malformed: ineligible (ncf_eligible)
  int64_t off = 0;
  int tile = 0;
  p->w[0] = d->n_fc > 0 ? d->widths[0] : 0;
  for (int l = 1; l <= d->n_fc; ++l) {
    if (d->widths[l] < 1) return "a width is not positive";
    p->w[l] = d->widths[l];
  }
  for (int l = 0; l <= d->n_fc; ++l) {
    if (d->n_fc == 0) break;
    p->apitch[l] = p->w[l] | 1;
    p->aoff[l] = tile;
    tile += kNcfTile * p->apitch[l];
  }
  for (int l = 1; l <= d->n_fc; ++l) {
    p->woff[l] = (int)off;
    off += pad4(p->w[l - 1] * p->w[l]);
    p->boff[l] = (int)off;
    off += pad4(p->w[l]);
    p->doff[l] = tile;
    tile += kNcfTile * p->apitch[l];
    if (off > (1 << 24)) return nullptr;                      // far beyond any LDS: ineligible
  }
  p->pw = p->mf + (d->n_fc > 0 ? p->w[d->n_fc] : 0);
  p->poff = (int)off;
  off += pad4(p->pw);
  p->pboff = (int)off;
  off += 4;
  p->P = (int)off;
  p->mfpitch = p->mf | 1;
  p->mfu_off = tile;
  tile += p->mf > 0 ? kNcfTile * p->mfpitch : 0;
  p->mfi_off = tile;
  tile += p->mf > 0 ? kNcfTile * p->mfpitch : 0;
  p->dz_off = tile;
  tile += kNcfTile;
  p->cost_off = tile;
  tile += kNcfTile;
  p->id_off = tile;                                           // even: every term above is a multiple of kNcfTile
  tile += 4 * kNcfTile;
  p->tile_floats = tile;
  return nullptr;
}

// The fused kernels' LDS in bytes: weights + accumulators + one tile (the score kernel uses the same figure less the accumulators)
inline int64_t ncf_lds_bytes(const NcfPlan& p, bool train) { return 4ll * ((train ? 2 : 1) * (int64_t)p.P + p.tile_floats); }

bool ncf_eligible(const rec_ncf_desc* d, const NcfPlan& p) {
  if (d->n_fc > REC_NCF_MAX_FC || d->mf_dim > REC_NCF_MAX_WIDTH) return false;
  for (int l = 0; l <= d->n_fc && d->n_fc > 0; ++l)
    if (d->widths[l] > REC_NCF_MAX_WIDTH) return false;
  return ncf_lds_bytes(p, true) <= REC_NCF_LDS_BYTES;
}

// ---------------------------------------------------------------- the whole net
template <bool TRAIN>
__global__ __launch_bounds__(kBlock) void ncf_net_kernel(NcfPlan p, int64_t B, float inv_mean, int64_t num_users,
                                                         int64_t num_items, const int64_t* __restrict__ users,
                                                         const int64_t* __restrict__ items,
                                                         const int64_t* __restrict__ labels,
                                                         const float* __restrict__ utab, int64_t ldu,
                                                         const float* __restrict__ itab, int64_t ldi,
                                                         const float* __restrict__ dense, float* __restrict__ pred,
                                                         float* __restrict__ gu, int64_t ldgu, float* __restrict__ gi,
                                                         int64_t ldgi, float* __restrict__ partials,
                                                         int32_t* __restrict__ status) {
  extern __shared__ float sm[];
  float* __restrict__ W = sm;
  float* __restrict__ acc = sm + p.P;                         // TRAIN only
  float* __restrict__ tile = sm + (TRAIN ? 2 * p.P : p.P);
  int64_t* __restrict__ sid = reinterpret_cast<int64_t*>(tile + p.id_off);   // [2][T]: the validated ids, -1 = none
  const int tid = threadIdx.x, nfc = p.nfc, mf = p.mf, half = p.half;
  for (int e = tid; e < p.P; e += kBlock) {
    W[e] = dense[e];
    if (TRAIN) acc[e] = 0.f;
  }
  float loss_sum = 0.f;                                       // thread 0's
  const int64_t ntiles = (B + kNcfTile - 1) / kNcfTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t s0 = t * kNcfTile;
    const int rows = (int)(B - s0 < kNcfTile ? B - s0 : kNcfTile);
    __syncthreads();                                          // the weights; the previous tile's readers
    if (tid < 2 * rows) {
      const int side = tid >= rows, s = side ? tid - rows : tid;
      const int64_t id = side ? items[s0 + s] : users[s0 + s];
      const bool ok = id >= 0 && id < (side ? num_items : num_users);
      if (!ok && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
      sid[side * kNcfTile + s] = ok ? id : -1;
    }
    __syncthreads();
    // the two packed rows of every sample: MF columns to mfu / mfi, MLP columns to the halves of a_0
    for (int e = tid; e < 2 * rows * p.cu; e += kBlock) {
      const int side = e >= rows * p.cu, r = side ? e - rows * p.cu : e;
      const int s = r / p.cu, c = r - s * p.cu;
      const int64_t id = sid[side * kNcfTile + s];
      const float v = id < 0 ? 0.f : (side ? itab[id * ldi + c] : utab[id * ldu + c]);
      if (c < mf) tile[(side ? p.mfi_off : p.mfu_off) + s * p.mfpitch + c] = v;
      else tile[p.aoff[0] + s * p.apitch[0] + side * half + (c - mf)] = v;
    }
    __syncthreads();
    for (int l = 1; l <= nfc; ++l) {                          // a_l = relu(a_{l-1} W_l + b_l)
      const int in = p.w[l - 1], out = p.w[l];
      const float* __restrict__ Wl = W + p.woff[l];
      const float* __restrict__ a_in = tile + p.aoff[l - 1];
      for (int o = tid; o < rows * out; o += kBlock) {
        const int s = o / out, j = o - s * out;
        float z = W[p.boff[l] + j];
        for (int i = 0; i < in; ++i) z = fmaf(a_in[s * p.apitch[l - 1] + i], Wl[i * out + j], z);
        tile[p.aoff[l] + s * p.apitch[l] + j] = fmaxf(z, 0.f);
      }
      __syncthreads();
    }
    if (tid < rows) {                                         // the head, the loss and dz: one thread per sample
      const int s = tid;
      float z = W[p.pboff];
      for (int c = 0; c < mf; ++c)
        z = fmaf(tile[p.mfu_off + s * p.mfpitch + c] * tile[p.mfi_off + s * p.mfpitch + c], W[p.poff + c], z);
      if (nfc > 0)
        for (int j = 0; j < p.w[nfc]; ++j) z = fmaf(tile[p.aoff[nfc] + s * p.apitch[nfc] + j], W[p.poff + mf + j], z);
      const float pr = 1.f / (1.f + expf(-z));
      pred[s0 + s] = pr;
      if (TRAIN) {
        const float y = (float)labels[s0 + s];
        tile[p.cost_off + s] = -y * logf(pr + kNcfEps) - (1.f - y) * logf(1.f - pr + kNcfEps);
        tile[p.dz_off + s] = (-y / (pr + kNcfEps) + (1.f - y) / (1.f - pr + kNcfEps)) * inv_mean * (pr * (1.f - pr));
      }
    }
    if (!TRAIN) continue;
    __syncthreads();
    if (tid == 0)
      for (int s = 0; s < rows; ++s) loss_sum += tile[p.cost_off + s];
    // the MF halves of the two gradient rows: dz w_c mf_i, dz w_c mf_u
    for (int e = tid; e < 2 * rows * mf; e += kBlock) {
      const int side = e >= rows * mf, r = side ? e - rows * mf : e;
      const int s = r / mf, c = r - s * mf;
      const float other = tile[(side ? p.mfu_off : p.mfi_off) + s * p.mfpitch + c];
      const float g = sid[side * kNcfTile + s] < 0 ? 0.f : tile[p.dz_off + s] * W[p.poff + c] * other;
      if (side) gi[(s0 + s) * ldgi + c] = g;
      else gu[(s0 + s) * ldgu + c] = g;
    }
    if (nfc > 0) {                                            // d_nfc = dz w o relu'(a_nfc); the mask is the stored activation
      const int out = p.w[nfc];
      for (int o = tid; o < rows * out; o += kBlock) {
        const int s = o / out, j = o - s * out;
        tile[p.doff[nfc] + s * p.apitch[nfc] + j] =
            tile[p.aoff[nfc] + s * p.apitch[nfc] + j] > 0.f ? tile[p.dz_off + s] * W[p.poff + mf + j] : 0.f;
      }
    }
    __syncthreads();
    for (int l = nfc; l >= 1; --l) {                          // d_{l-1} = (d_l W_l^T) o relu'(a_{l-1}); l == 1: the MLP halves of the rows
      const int in = p.w[l - 1], out = p.w[l];
      const float* __restrict__ Wl = W + p.woff[l];
      const float* __restrict__ dl = tile + p.doff[l];
      for (int o = tid; o < in * kNcfTile; o += kBlock) {
        const int i = o / kNcfTile, s = o - i * kNcfTile;     // the sample fastest: W_l[i, :] is a broadcast
        if (s >= rows) continue;
        float x = 0.f;
        for (int j = 0; j < out; ++j) x = fmaf(dl[s * p.apitch[l] + j], Wl[i * out + j], x);
        if (l > 1) {
          tile[p.doff[l - 1] + s * p.apitch[l - 1] + i] = tile[p.aoff[l - 1] + s * p.apitch[l - 1] + i] > 0.f ? x : 0.f;
        } else {
          const int side = i >= half, c = mf + (side ? i - half : i);
          if (sid[side * kNcfTile + s] < 0) x = 0.f;
          if (side) gi[(s0 + s) * ldgi + c] = x;
          else gu[(s0 + s) * ldgu + c] = x;
        }
      }
      __syncthreads();
    }
    // the dense gradients: element e has ONE owner, which adds the tile's samples in ascending order
    for (int e = tid; e < p.P; e += kBlock) {
      float a = acc[e];
      if (e >= p.poff) {
        const int c = e - p.poff;
        if (e == p.pboff) {
          for (int s = 0; s < rows; ++s) a += tile[p.dz_off + s];
        } else if (c < mf) {
          for (int s = 0; s < rows; ++s)
            a = fmaf(tile[p.dz_off + s], tile[p.mfu_off + s * p.mfpitch + c] * tile[p.mfi_off + s * p.mfpitch + c], a);
        } else if (c < p.pw) {
          for (int s = 0; s < rows; ++s) a = fmaf(tile[p.dz_off + s], tile[p.aoff[nfc] + s * p.apitch[nfc] + c - mf], a);
        }
      } else {
        int l = 1;
        while (l < nfc && e >= p.woff[l + 1]) ++l;
        const int out = p.w[l];
        const float* __restrict__ dl = tile + p.doff[l];
        if (e >= p.boff[l]) {
          const int j = e - p.boff[l];
          if (j < out)
            for (int s = 0; s < rows; ++s) a += dl[s * p.apitch[l] + j];
        } else {
          const int r = e - p.woff[l], i = r / out, j = r - i * out;
          if (i < p.w[l - 1]) {
            const float* __restrict__ a_in = tile + p.aoff[l - 1] + i;
            for (int s = 0; s < rows; ++s) a = fmaf(a_in[s * p.apitch[l - 1]], dl[s * p.apitch[l] + j], a);
          }
        }
      }
      acc[e] = a;
    }
  }
  if (TRAIN) {
    __syncthreads();
    float* __restrict__ mine = partials + (int64_t)blockIdx.x * (p.P + 1);
    for (int e = tid; e < p.P; e += kBlock) mine[e] = acc[e];
    if (tid == 0) mine[p.P] = loss_sum;
  }
}

// g_dense[e] = sum_b partials[b, e] in ascending b (four loads in flight); element P is the loss
__global__ __launch_bounds__(kBlock) void ncf_fold_kernel(int nparts, int P, float inv_mean,
                                                          const float* __restrict__ partials,
                                                          float* __restrict__ g_dense, float* __restrict__ loss) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e > P) return;
  const int64_t W = P + 1;
  float s = 0.f;
  int b = 0;
  for (; b + 4 <= nparts; b += 4) {
    const float x0 = partials[b * W + e], x1 = partials[(b + 1) * W + e];
    const float x2 = partials[(b + 2) * W + e], x3 = partials[(b + 3) * W + e];
    s = (((s + x0) + x1) + x2) + x3;
  }
  for (; b < nparts; ++b) s += partials[b * W + e];
  if (e < P) g_dense[e] = s;
  else loss[0] = s * inv_mean;
}

// ---------------------------------------------------------------- the general route's glue
__global__ __launch_bounds__(kBlock) void ncf_gather_fwd_kernel(int64_t n, int mf, int half, int64_t num_users,
                                                                int64_t num_items, const int64_t* __restrict__ users,
                                                                const int64_t* __restrict__ items,
                                                                const float* __restrict__ utab, int64_t ldu,
                                                                const float* __restrict__ itab, int64_t ldi,
                                                                float* __restrict__ pred_in, int64_t ldp,
                                                                float* __restrict__ mlp_in, int64_t ldm,
                                                                int32_t* __restrict__ status) {
  const int cols = mf + 2 * half;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  const int64_t s = e / cols;
  const int c = (int)(e - s * cols);
  const int64_t u = users[s], it = items[s];
  const bool uok = u >= 0 && u < num_users, iok = it >= 0 && it < num_items;
  if (c == 0 && !(uok && iok) && status != nullptr) atomicOr(status, REC_FLAG_INDEX_OOB);
  if (c < mf) {
    pred_in[s * ldp + c] = uok && iok ? utab[u * ldu + c] * itab[it * ldi + c] : 0.f;
  } else {
    const int k = c - mf;
    mlp_in[s * ldm + k] = k < half ? (uok ? utab[u * ldu + mf + k] : 0.f) : (iok ? itab[it * ldi + mf + k - half] : 0.f);
  }
}

__global__ __launch_bounds__(kBlock) void ncf_gather_bwd_kernel(int64_t n, int mf, int half, int64_t num_users,
                                                                int64_t num_items, const int64_t* __restrict__ users,
                                                                const int64_t* __restrict__ items,
                                                                const float* __restrict__ utab, int64_t ldu,
                                                                const float* __restrict__ itab, int64_t ldi,
                                                                const float* __restrict__ dpi, int64_t lddp,
                                                                const float* __restrict__ dmi, int64_t lddm,
                                                                float* __restrict__ gu, int64_t ldgu,
                                                                float* __restrict__ gi, int64_t ldgi) {
  const int cu = mf + half;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  const int64_t s = e / (2 * cu);
  const int r = (int)(e - s * 2 * cu), side = r >= cu, c = side ? r - cu : r;
  const int64_t u = users[s], it = items[s];
  const bool uok = u >= 0 && u < num_users, iok = it >= 0 && it < num_items;
  float g = 0.f;
  if (side ? iok : uok) {
    if (c < mf) g = uok && iok ? dpi[s * lddp + c] * (side ? utab[u * ldu + c] : itab[it * ldi + c]) : 0.f;
    else g = dmi[s * lddm + side * half + (c - mf)];
  }
  if (side) gi[s * ldgi + c] = g;
  else gu[s * ldgu + c] = g;
}

}  // namespace
}  // namespace rec

using namespace rec;

#define NCF_DESC_ARGS int32_t mf_dim, int32_t n_fc, const int32_t *widths, int64_t num_users, int64_t num_items
#define NCF_PLAN(gather_only)                                                           \
  NcfPlan p;                                                                            \
  rec_ncf_desc desc_v = {mf_dim, n_fc, {0}, num_users, num_items};                      \
  const rec_ncf_desc* desc = &desc_v;                                                   \
  REC_REQUIRE(n_fc <= 0 || widths != nullptr, REC_EINVAL, "%s: widths is null", what);  \
  for (int l = 0; n_fc > 0 && l <= (gather_only ? 0 : n_fc) && l < kNcfMaxWidths; ++l) desc_v.widths[l] = widths[l]; \
  {                                                                                     \
    const char* bad = ncf_plan(desc, &p, gather_only);                                  \
    REC_REQUIRE(bad == nullptr, REC_EINVAL, "%s: desc: %s", what, bad);                 \
  }

extern "C" int rec_ncf_dense_numel(NCF_DESC_ARGS, int64_t* numel) {
  const char* what = "rec_ncf_dense_numel";
  REC_REQUIRE(numel != nullptr, REC_EINVAL, "%s: numel is null", what);
  NCF_PLAN(false);
  REC_REQUIRE(desc->n_fc <= REC_NCF_MAX_FC, REC_EINVAL, "%s: n_fc %d above REC_NCF_MAX_FC %d (the layout is the fused kernels')",
              what, desc->n_fc, REC_NCF_MAX_FC);
  *numel = p.P;
  return REC_OK;
}

extern "C" int rec_ncf_fused_eligible(NCF_DESC_ARGS, int32_t* eligible) {
  const char* what = "rec_ncf_fused_eligible";
  REC_REQUIRE(eligible != nullptr, REC_EINVAL, "%s: eligible is null", what);
  NCF_PLAN(false);
  *eligible = ncf_eligible(desc, p) ? 1 : 0;
  return REC_OK;
}

extern "C" int rec_ncf_step(NCF_DESC_ARGS, int64_t batch, int64_t mean_over, const int64_t* users,
                            const int64_t* items, const int64_t* labels, const float* user_table, int64_t ld_user,
                            const float* item_table, int64_t ld_item, const float* dense, float* pred, float* g_user,
                            int64_t ld_gu, float* g_item, int64_t ld_gi, float* partials, float* g_dense, float* loss,
                            int32_t* status, void* stream) {
  const char* what = "rec_ncf_step";
  NCF_PLAN(false);
  REC_REQUIRE(ncf_eligible(desc, p), REC_EINVAL,
              "%s: desc: the net is not eligible for the fused kernels (rec_ncf_fused_eligible): n_fc <= %d, widths <= %d, %d "
              "bytes of LDS", what, REC_NCF_MAX_FC, REC_NCF_MAX_WIDTH, REC_NCF_LDS_BYTES);
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31), REC_EINVAL, "%s: batch %lld outside 0..2^31", what, (long long)batch);
  REC_REQUIRE(mean_over >= 0, REC_EINVAL, "%s: mean_over %lld is negative", what, (long long)mean_over);
  REC_REQUIRE(ld_user >= p.cu && ld_item >= p.cu, REC_EINVAL, "%s: ld_user / ld_item smaller than the packed row (%d)", what, p.cu);
  REC_REQUIRE(ld_gu >= p.cu && ld_gi >= p.cu, REC_EINVAL, "%s: ld_gu / ld_gi smaller than the packed row (%d)", what, p.cu);
  REC_REQUIRE(g_dense && loss, REC_EINVAL, "%s: g_dense / loss is null", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(users && items && labels, REC_EINVAL, "%s: users / items / labels is null", what);
  REC_REQUIRE(user_table && item_table && dense, REC_EINVAL, "%s: user_table / item_table / dense is null", what);
  REC_REQUIRE(pred && g_user && g_item && partials, REC_EINVAL, "%s: pred / g_user / g_item / partials is null", what);
  for (const float* o : {(const float*)pred, (const float*)g_user, (const float*)g_item, (const float*)partials,
                         (const float*)g_dense, (const float*)loss})
    REC_REQUIRE(o != user_table && o != item_table && o != dense, REC_EINVAL, "%s: an output aliases an input", what);
  const int64_t ntiles = (batch + kNcfTile - 1) / kNcfTile;
  const int G = (int)(ntiles < REC_NCF_MAX_BLOCKS ? ntiles : REC_NCF_MAX_BLOCKS);
  const float inv_mean = 1.f / (float)(mean_over > 0 ? mean_over : batch);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ncf_net_kernel<true>, dim3((unsigned)G), dim3(kBlock), (size_t)ncf_lds_bytes(p, true), st, p, batch,
                     inv_mean, desc->num_users, desc->num_items, users, items, labels, user_table, ld_user, item_table,
                     ld_item, dense, pred, g_user, ld_gu, g_item, ld_gi, partials, status);
  int rc = check_launch(what);
  if (rc != REC_OK) return rc;
  hipLaunchKernelGGL(ncf_fold_kernel, dim3((unsigned)((p.P + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, G, p.P, inv_mean,
                     (const float*)partials, g_dense, loss);
  return check_launch("rec_ncf_step (fold)");
}

extern "C" int rec_ncf_score(NCF_DESC_ARGS, int64_t batch, const int64_t* users, const int64_t* items,
                             const float* user_table, int64_t ld_user, const float* item_table, int64_t ld_item,
                             const float* dense, float* pred, int32_t* status, void* stream) {
  const char* what = "rec_ncf_score";
  NCF_PLAN(false);
  REC_REQUIRE(ncf_eligible(desc, p), REC_EINVAL,
              "%s: desc: the net is not eligible for the fused kernels (rec_ncf_fused_eligible): n_fc <= %d, widths <= %d, %d "
              "bytes of LDS", what, REC_NCF_MAX_FC, REC_NCF_MAX_WIDTH, REC_NCF_LDS_BYTES);
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31), REC_EINVAL, "%s: batch %lld outside 0..2^31", what, (long long)batch);
  REC_REQUIRE(ld_user >= p.cu && ld_item >= p.cu, REC_EINVAL, "%s: ld_user / ld_item smaller than the packed row (%d)", what, p.cu);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(users && items, REC_EINVAL, "%s: users / items is null", what);
  REC_REQUIRE(user_table && item_table && dense, REC_EINVAL, "%s: user_table / item_table / dense is null", what);
  REC_REQUIRE(pred && pred != user_table && pred != item_table && pred != dense, REC_EINVAL,
              "%s: pred is null or aliases an input", what);
  const int64_t ntiles = (batch + kNcfTile - 1) / kNcfTile;
  const int G = (int)(ntiles < REC_NCF_MAX_BLOCKS ? ntiles : REC_NCF_MAX_BLOCKS);
  hipLaunchKernelGGL(ncf_net_kernel<false>, dim3((unsigned)G), dim3(kBlock), (size_t)ncf_lds_bytes(p, false),
                     (hipStream_t)stream, p, batch, 0.f, desc->num_users, desc->num_items, users, items,
                     (const int64_t*)nullptr, user_table, ld_user, item_table, ld_item, dense, pred, (float*)nullptr,
                     (int64_t)0, (float*)nullptr, (int64_t)0, (float*)nullptr, status);
  return check_launch(what);
}

extern "C" int rec_ncf_gather_fwd(NCF_DESC_ARGS, int64_t batch, const int64_t* users, const int64_t* items,
                                  const float* user_table, int64_t ld_user, const float* item_table, int64_t ld_item,
                                  float* pred_in, int64_t ld_pred_in, float* mlp_in, int64_t ld_mlp_in, int32_t* status,
                                  void* stream) {
  const char* what = "rec_ncf_gather_fwd";
  NCF_PLAN(true);
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31) / (2 * p.cu), REC_EINVAL, "%s: batch %lld negative or too large", what,
              (long long)batch);
  REC_REQUIRE(ld_user >= p.cu && ld_item >= p.cu, REC_EINVAL, "%s: ld_user / ld_item smaller than the packed row (%d)", what, p.cu);
  REC_REQUIRE(p.mf == 0 || ld_pred_in >= p.mf, REC_EINVAL, "%s: ld_pred_in smaller than mf_dim", what);
  REC_REQUIRE(p.half == 0 || ld_mlp_in >= 2 * p.half, REC_EINVAL, "%s: ld_mlp_in smaller than widths[0]", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(users && items && user_table && item_table, REC_EINVAL, "%s: users / items / user_table / item_table is null", what);
  REC_REQUIRE((p.mf == 0 || pred_in) && (p.half == 0 || mlp_in), REC_EINVAL, "%s: pred_in / mlp_in is null", what);
  REC_REQUIRE(pred_in != user_table && pred_in != item_table && mlp_in != user_table && mlp_in != item_table, REC_EINVAL,
              "%s: an output aliases a table", what);
  const int64_t n = batch * (p.mf + 2 * p.half);
  hipLaunchKernelGGL(ncf_gather_fwd_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n,
                     p.mf, p.half, desc->num_users, desc->num_items, users, items, user_table, ld_user, item_table, ld_item,
                     pred_in, ld_pred_in, mlp_in, ld_mlp_in, status);
  return check_launch(what);
}

extern "C" int rec_ncf_gather_bwd(NCF_DESC_ARGS, int64_t batch, const int64_t* users, const int64_t* items,
                                  const float* user_table, int64_t ld_user, const float* item_table, int64_t ld_item,
                                  const float* d_pred_in, int64_t ld_dpred_in, const float* d_mlp_in, int64_t ld_dmlp_in,
                                  float* g_user, int64_t ld_gu, float* g_item, int64_t ld_gi, void* stream) {
  const char* what = "rec_ncf_gather_bwd";
  NCF_PLAN(true);
  REC_REQUIRE(batch >= 0 && batch < (1ll << 31) / (2 * p.cu), REC_EINVAL, "%s: batch %lld negative or too large", what,
              (long long)batch);
  REC_REQUIRE(ld_user >= p.cu && ld_item >= p.cu, REC_EINVAL, "%s: ld_user / ld_item smaller than the packed row (%d)", what, p.cu);
  REC_REQUIRE(ld_gu >= p.cu && ld_gi >= p.cu, REC_EINVAL, "%s: ld_gu / ld_gi smaller than the packed row (%d)", what, p.cu);
  REC_REQUIRE(p.mf == 0 || ld_dpred_in >= p.mf, REC_EINVAL, "%s: ld_dpred_in smaller than mf_dim", what);
  REC_REQUIRE(p.half == 0 || ld_dmlp_in >= 2 * p.half, REC_EINVAL, "%s: ld_dmlp_in smaller than widths[0]", what);
  if (batch == 0) return REC_OK;
  REC_REQUIRE(users && items && user_table && item_table, REC_EINVAL, "%s: users / items / user_table / item_table is null", what);
  REC_REQUIRE((p.mf == 0 || d_pred_in) && (p.half == 0 || d_mlp_in), REC_EINVAL, "%s: d_pred_in / d_mlp_in is null", what);
  REC_REQUIRE(g_user && g_item && g_user != g_item, REC_EINVAL, "%s: g_user / g_item is null or the same", what);
  for (const float* o : {(const float*)g_user, (const float*)g_item})
    REC_REQUIRE(o != user_table && o != item_table && o != d_pred_in && o != d_mlp_in, REC_EINVAL,
                "%s: an output aliases an input", what);
  const int64_t n = batch * 2 * p.cu;
  hipLaunchKernelGGL(ncf_gather_bwd_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n,
                     p.mf, p.half, desc->num_users, desc->num_items, users, items, user_table, ld_user, item_table, ld_item,
                     d_pred_in, ld_dpred_in, d_mlp_in, ld_dmlp_in, g_user, ld_gu, g_item, ld_gi);
  return check_launch(what);
}
