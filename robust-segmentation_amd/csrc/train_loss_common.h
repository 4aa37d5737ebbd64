// Shared pieces of the training-criterion translation units (train_loss.hip: T2 on full-resolution logits and the OHEM
// select; train_loss_up.hip: T2u on low-resolution logits): the per-block record, the 64 bytes of device words, the
// workspace layout that sea_train_ohem_select reads, and the one-block kernel that sums the records in a fixed order.
#pragma once
#include "sea_common.h"

namespace sea {

struct __attribute__((aligned(8))) TrainRecord {
  double loss, w, hard;
  int n_valid, n_hard;
};
static_assert(sizeof(TrainRecord) == 32, "TrainRecord");

// the device words (64 bytes; mirrored by semseg/_native.py: TRAIN_WORDS)
struct __attribute__((aligned(8))) TrainWords {
  double sum_sel;   // sum of the selected losses (CrossEntropy: of all valid ones)
  double sum_w;     // sum of w[y] over the valid pixels
  double sum_loss;  // sum of all per-pixel losses
  float loss;       // the criterion's value
  float coef;       // 1 / sum_w (CrossEntropy) or 1 / n_sel (OHEM): the backward's normalisation
  uint32_t t_bits;  // OHEM: selection threshold (float bits): selected = loss > t, plus `take` ties at t
  int take;         // OHEM top-k mode: number of pixels with loss == t to take, in ascending flat index
  int n_sel;        // OHEM: number of selected pixels
  int n_valid, n_hard, n_min;
  int mode;         // OHEM: 0 = threshold mode (n_hard >= n_min), 1 = top-k mode
  int err;          // 1 if a label outside [0, C) other than ignore_label was seen (treated as ignored)
};
static_assert(sizeof(TrainWords) == 64, "TrainWords");

constexpr int kSelMaxBlocks = 1024;  // blocks of the select passes (G)
constexpr float kUnselected = -1.f;  // written into the loss plane by the select for pixels the backward skips
// workspace: [hist 4 x 256 int][blk_sum G double][blk_ties G int][tie_base G int][records]
constexpr size_t kOffHist = 0, kOffBlkSum = 4096, kOffBlkTies = kOffBlkSum + 8 * kSelMaxBlocks,
                 kOffTieBase = kOffBlkTies + 4 * kSelMaxBlocks, kOffRecords = kOffTieBase + 4 * kSelMaxBlocks;
static_assert(kOffRecords % 32 == 0, "records are 8-byte aligned");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// label of a pixel as the kernels use it: class index, or -1 for ignore_label and for anything outside [0, C)
__device__ __forceinline__ int train_label(long long v, long long ignore, int C, bool& counted, bool& bad) {
  counted = v != ignore;  // what losses.py:48 counts for n_min
  bad = counted && (v < 0 || v >= (long long)C);
  return (!counted || bad) ? -1 : (int)v;
}

// ---- fixed-order sum of the records; decides the OHEM regime ----------------------------------------------------------
// one block.  ohem = 0: CrossEntropy (mean over the valid pixels, weighted); 1: first stage of the OHEM select.
static __global__ __launch_bounds__(256) void train_reduce_k(const TrainRecord* __restrict__ rec, int n_rec, int ohem,
                                                      float thresh, int* __restrict__ hist,
                                                      TrainWords* __restrict__ words) {
  __shared__ double s_d[3][256];
  __shared__ long long s_i[2][256];
  const int t = threadIdx.x;
  double l = 0.0, ww = 0.0, h = 0.0;
  long long nv = 0, nh = 0;
  for (int i = t; i < n_rec; i += 256) {
    const TrainRecord r = rec[i];
    l += r.loss;
    ww += r.w;
    h += r.hard;
    nv += r.n_valid;
    nh += r.n_hard;
  }
  s_d[0][t] = l;
  s_d[1][t] = ww;
  s_d[2][t] = h;
  s_i[0][t] = nv;
  s_i[1][t] = nh;
  if (ohem)
    for (int i = t; i < 4 * 256; i += 256) hist[i] = 0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_d[k][t] += s_d[k][t + o];
      s_i[0][t] += s_i[0][t + o];
      s_i[1][t] += s_i[1][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double sl = s_d[0][0], sw = s_d[1][0], sh = s_d[2][0];
    const int n_valid = (int)s_i[0][0], n_hard = (int)s_i[1][0];
    words->sum_loss = sl;
    words->sum_w = sw;
    words->n_valid = n_valid;
    words->n_hard = n_hard;
    if (!ohem) {
      words->sum_sel = sl;
      words->loss = (float)(sl / sw);  // 0 / 0 = NaN when every label is ignored, as torch
      words->coef = (float)(1.0 / sw);
      words->n_min = 0;
      words->mode = 0;
      words->n_sel = n_valid;
      words->take = 0;
      words->t_bits = 0;
    } else {
      const int n_min = n_valid / 16;  // losses.py:48
      words->n_min = n_min;
      const int mode = (n_hard < n_min) ? 1 : 0;  // losses.py:52
      words->mode = mode;
      if (mode == 0) {
        words->t_bits = __float_as_uint(thresh);
        words->take = 0;
        words->n_sel = n_hard;
        words->sum_sel = sh;
        words->loss = (float)(sh / (double)n_hard);  // torch.mean of an empty tensor: NaN
        words->coef = (float)(1.0 / (double)n_hard);
      }
    }
  }
}

}  // namespace sea
