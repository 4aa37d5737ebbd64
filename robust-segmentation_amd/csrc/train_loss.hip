// T2: the training criteria of the PIR-AT outer step on the device (reference semseg/losses.py:6-63): CrossEntropy and
// OhemCrossEntropy, forward + hard-pixel selection + backward, without a host read anywhere.
//
// Roofline: HBM.  Bytes per pixel, s = bytes per logit: forward C*s (logits) + 8 (int64 label) + 4 (loss plane);
// backward 2*C*s + 8 + 4 while the class vector fits the registers (C <= 32), 3*C*s + 8 + 4 beyond (the logits are
// read twice: soft-max statistics, then the gradient).  The log-softmax is never materialised: between forward and
// backward only the per-pixel loss plane (B*H*W floats) and 64 bytes of device words live.
//
// Layout NCHW as in K2 (loss_kernels.hip): lane l owns VEC consecutive pixels, for every class the wave reads one
// contiguous segment of that class plane (16 bytes per lane in the streaming kernels).  The class reduction is within
// a lane, so no LDS is needed for it.
//
// Sums: every block writes one record {sum loss, sum w[y], sum hard loss, n_valid, n_hard} reduced wave -> block in a
// fixed order in double; one block adds the records in a fixed order.  The radix select counts with INTEGER atomics
// only (the counts do not depend on the order of arrival).  No float atomics => bitwise reproducible run to run.
//
// exp is the accurate library version, not the hardware approximation K2 uses, the soft-max denominator is summed in
// double and the per-pixel log is taken in double: the criterion's value and gradient are compared with torch's own to
// the last bits (tests/test_train_loss_gpu.py), an attack direction is not.  The two extra double operations per logit
// and one double log per pixel are the price; the rescale of the online soft-max stays a float exp (exact 1 whenever
// the running maximum did not move).
#include "loss_common.h"
#include "train_loss_common.h"

namespace sea {

// ---- soft-max statistics of VEC pixels, streaming over the class planes (any C) ------------------------------------
// Online maximum and rescaled sum, four planes per trip (their loads are independent and in flight together).
// p0: the lane's first pixel in class plane 0.  On return m = max_c z, s = sum_c exp(z - m), zy = z[lab] (0 if none).
template <typename T, int VEC>
__device__ __forceinline__ void class_stats(const T* __restrict__ p0, int C, int64_t HW, const int (&lab)[VEC],
                                            float (&m)[VEC], double (&s)[VEC], float (&zy)[VEC]) {
  using R = typename Elem<T>::raw;
  using P = typename RawVec<R, VEC>::type;
  constexpr int CH = 4;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    m[v] = -INFINITY;
    s[v] = 0.0;
    zy[v] = 0.f;
  }
  const R* base = reinterpret_cast<const R*>(p0);
  for (int c0 = 0; c0 < C; c0 += CH) {
    P p[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (c0 + j < C) p[j] = __builtin_nontemporal_load(reinterpret_cast<const P*>(base + (int64_t)(c0 + j) * HW));
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float z[CH];
      float mm = m[v];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        z[j] = (c0 + j < C) ? Elem<T>::to_f(vec_get<R, VEC>(p[j], v)) : -INFINITY;
        mm = fmaxf(mm, z[j]);
        zy[v] = (lab[v] == c0 + j) ? z[j] : zy[v];
      }
      // a running maximum of -inf (nothing finite seen yet) must not turn exp(-inf - -inf) into NaN
      const float me = (mm == -INFINITY) ? -3.0e38f : mm;
      const float mo = (m[v] == -INFINITY) ? -3.0e38f : m[v];
      double acc = (mo == me) ? s[v] : s[v] * (double)expf(mo - me);
#pragma unroll
      for (int j = 0; j < CH; ++j) acc += (double)expf(z[j] - me);
      m[v] = mm;
      s[v] = acc;
    }
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------
// grid = (tiles per image, B), block = 256, tile = 256*VEC consecutive pixels of one image.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void train_ce_fwd_k(const T* __restrict__ logits, const long long* __restrict__ y,
                                                      const float* __restrict__ w, long long ignore, float thresh, int C,
                                                      int64_t HW, float* __restrict__ loss_px,
                                                      TrainRecord* __restrict__ rec, TrainWords* __restrict__ words) {
  const int b = blockIdx.y;
  const int64_t px0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  const bool active = px0 < HW;  // HW % VEC == 0 is guaranteed by the launcher
  double lsum = 0.0, wsum = 0.0, hsum = 0.0;
  int nvalid = 0, nhard = 0;
  if (active) {
    int lab[VEC];
    bool any_bad = false;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      bool counted, bad;
      lab[v] = train_label(y[(int64_t)b * HW + px0 + v], ignore, C, counted, bad);
      nvalid += counted ? 1 : 0;
      any_bad |= bad;
    }
    if (any_bad) words->err = 1;  // every writer stores the same value
    float m[VEC], zy[VEC];
    double s[VEC];
    class_stats<T, VEC>(logits + (int64_t)b * C * HW + px0, C, HW, lab, m, s, zy);
    float lv[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      // -log_softmax(z)[y] = log(sum exp(z - m)) - (z_y - m), rounded to float once
      const float ce = (float)(log(s[v]) - ((double)zy[v] - (double)m[v]));
      const bool valid = lab[v] >= 0;
      const float wy = (valid && w != nullptr) ? w[lab[v]] : 1.f;
      lv[v] = valid ? wy * ce : 0.f;
      lsum += (double)lv[v];
      wsum += valid ? (double)wy : 0.0;
      const bool hard = lv[v] > thresh;
      nhard += hard ? 1 : 0;
      hsum += hard ? (double)lv[v] : 0.0;
    }
    using LP = typename RawVec<float, VEC>::type;
    LP out;
#pragma unroll
    for (int v = 0; v < VEC; ++v) vec_set<float, VEC>(out, v, lv[v]);
    *reinterpret_cast<LP*>(loss_px + (int64_t)b * HW + px0) = out;
  }
  __shared__ double s_d[3][4];
  __shared__ int s_i[2][4];
  lsum = wave_sum_d(lsum);
  wsum = wave_sum_d(wsum);
  hsum = wave_sum_d(hsum);
  nvalid = wave_sum_i(nvalid);
  nhard = wave_sum_i(nhard);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    s_d[0][wave] = lsum;
    s_d[1][wave] = wsum;
    s_d[2][wave] = hsum;
    s_i[0][wave] = nvalid;
    s_i[1][wave] = nhard;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TrainRecord r;
    r.loss = (s_d[0][0] + s_d[0][1]) + (s_d[0][2] + s_d[0][3]);
    r.w = (s_d[1][0] + s_d[1][1]) + (s_d[1][2] + s_d[1][3]);
    r.hard = (s_d[2][0] + s_d[2][1]) + (s_d[2][2] + s_d[2][3]);
    r.n_valid = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3];
    r.n_hard = s_i[1][0] + s_i[1][1] + s_i[1][2] + s_i[1][3];
    rec[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// ---- radix select over the float bits of the loss plane ------------------------------------------------------------
// losses are >= 0, so the bit pattern orders like the value (anything with the sign bit set counts as 0)
__device__ __forceinline__ uint32_t loss_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? 0u : u;
}

// From the histograms of passes 0 .. npass-1 (one byte each, most significant first): the bytes of the n_min-th largest
// key fixed so far, and how many of the keys that share them are still to be taken.  Called by every thread of a block.
__device__ __forceinline__ void select_resolve(const int* __restrict__ hist, int npass, int n_min, uint32_t& prefix,
                                               int& k) {
  __shared__ int sh[256];
  __shared__ uint32_t s_pref;
  __shared__ int s_k;
  const int t = threadIdx.x;
  if (t == 0) {
    s_pref = 0;
    s_k = n_min;
  }
  for (int q = 0; q < npass; ++q) {
    __syncthreads();
    sh[t] = hist[q * 256 + t];
    __syncthreads();
    int above = 0;
    for (int j = t + 1; j < 256; ++j) above += sh[j];
    const int kk = s_k;
    __syncthreads();
    if (above < kk && kk <= above + sh[t]) {  // exactly one digit holds the kk-th largest
      s_pref |= (uint32_t)t << (24 - 8 * q);
      s_k = kk - above;
    }
  }
  __syncthreads();
  prefix = s_pref;
  k = s_k;
}

static inline int sel_blocks(int64_t N) {
  int64_t g = (N + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > kSelMaxBlocks ? kSelMaxBlocks : g));
}
static inline int64_t sel_chunk(int64_t N) {
  const int g = sel_blocks(N);
  return ((N + g - 1) / g + 255) / 256 * 256;
}

// pass `pass` (0 .. 3): byte histogram of the keys that share the bytes fixed so far.  Leaves at once in threshold mode.
__global__ __launch_bounds__(256) void ohem_hist_k(const float* __restrict__ px, int64_t N, int64_t chunk, int pass,
                                                   int* __restrict__ hist, const TrainWords* __restrict__ words) {
  if (words->mode == 0) return;
  __shared__ int h[256];
  uint32_t prefix;
  int k;
  select_resolve(hist, pass, words->n_min, prefix, k);
  h[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = (start + chunk < N) ? start + chunk : N;
  for (int64_t i = start + threadIdx.x; i < end; i += 256) {
    const uint32_t key = loss_key(px[i]);
    const bool match = (pass == 0) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
    if (match) atomicAdd(&h[(key >> shift) & 255u], 1);
  }
  __syncthreads();
  const int c = h[threadIdx.x];
  if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);
}

// top-k mode: per block, the sum of the losses above t and the number of ties at t
__global__ __launch_bounds__(256) void ohem_sum_k(const float* __restrict__ px, int64_t N, int64_t chunk,
                                                  const int* __restrict__ hist, double* __restrict__ blk_sum,
                                                  int* __restrict__ blk_ties, const TrainWords* __restrict__ words) {
  if (words->mode == 0) return;
  uint32_t t_bits;
  int take;
  select_resolve(hist, 4, words->n_min, t_bits, take);
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = (start + chunk < N) ? start + chunk : N;
  double s = 0.0;
  int ties = 0;
  for (int64_t i = start + threadIdx.x; i < end; i += 256) {
    const float v = px[i];
    const uint32_t key = loss_key(v);
    s += (key > t_bits) ? (double)v : 0.0;
    ties += (key == t_bits) ? 1 : 0;
  }
  __shared__ double s_s[4];
  __shared__ int s_t[4];
  s = wave_sum_d(s);
  ties = wave_sum_i(ties);
  if ((threadIdx.x & 63) == 0) {
    s_s[threadIdx.x >> 6] = s;
    s_t[threadIdx.x >> 6] = ties;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_sum[blockIdx.x] = (s_s[0] + s_s[1]) + (s_s[2] + s_s[3]);
    blk_ties[blockIdx.x] = s_t[0] + s_t[1] + s_t[2] + s_t[3];
  }
}

// top-k mode, one block: the words, and the fixed-order prefix over the per-block tie counts
__global__ __launch_bounds__(256) void ohem_finish_k(int G, const int* __restrict__ hist,
                                                     const double* __restrict__ blk_sum,
                                                     const int* __restrict__ blk_ties, int* __restrict__ tie_base,
                                                     TrainWords* __restrict__ words) {
  if (words->mode == 0) return;
  uint32_t t_bits;
  int take;
  const int n_min = words->n_min;
  select_resolve(hist, 4, n_min, t_bits, take);
  if (threadIdx.x == 0) {
    double s = 0.0;
    int base = 0;
    for (int g = 0; g < G; ++g) {
      s += blk_sum[g];
      tie_base[g] = base;
      base += blk_ties[g];
    }
    s += (double)take * (double)__uint_as_float(t_bits);
    words->t_bits = t_bits;
    words->take = take;
    words->n_sel = n_min;
    words->sum_sel = s;
    words->loss = (float)(s / (double)n_min);
    words->coef = (float)(1.0 / (double)n_min);
  }
}

// both modes: overwrite the loss of every pixel that is NOT selected with kUnselected.  Ties at t are taken in
// ascending flat pixel index: rank = ties in earlier blocks + ties earlier in this block's chunk.
__global__ __launch_bounds__(256) void ohem_mark_k(float* __restrict__ px, int64_t N, int64_t chunk,
                                                   const int* __restrict__ tie_base,
                                                   const TrainWords* __restrict__ words) {
  const int mode = words->mode, take = words->take;
  const uint32_t t_bits = words->t_bits;
  const float t = __uint_as_float(t_bits);
  __shared__ int s_w[4];
  int base = (mode && take > 0) ? tie_base[blockIdx.x] : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = (start + chunk < N) ? start + chunk : N;
  for (int64_t i0 = start; i0 < end; i0 += 256) {
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < end;
    const float v = in ? px[i] : 0.f;
    const uint32_t key = loss_key(v);
    bool sel = in && (mode ? key > t_bits : v > t);
    if (mode && take > 0) {  // block-uniform
      const bool tie = in && key == t_bits;
      const unsigned long long mask = __ballot(tie);
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      if (lane == 0) s_w[wave] = __popcll(mask);
      __syncthreads();
      int wbase = 0, total = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wbase += (k < wave) ? s_w[k] : 0;
        total += s_w[k];
      }
      sel = sel || (tie && (base + wbase + before) < take);
      base += total;
      __syncthreads();
    }
    if (in && !sel) px[i] = kUnselected;
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------
// dlogits = g * coef * w[y] * (softmax - onehot) for selected pixels, 0 elsewhere.  g: the upstream gradient, a device
// float.  A pixel is selected if its label is valid and (OHEM) the select left its loss in the plane.
template <int VEC>
__device__ __forceinline__ bool bwd_labels(const long long* __restrict__ y, const float* __restrict__ loss_px,
                                           const float* __restrict__ w, int64_t i0, long long ignore, int C, int ohem,
                                           float gc, int (&lab)[VEC], float (&K)[VEC]) {
  bool any = false;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    bool counted, bad;
    lab[v] = train_label(y[i0 + v], ignore, C, counted, bad);
    bool sel = lab[v] >= 0;
    if (ohem) sel = sel && (loss_px[i0 + v] != kUnselected);
    lab[v] = sel ? lab[v] : -1;
    const float wy = (sel && w != nullptr) ? w[lab[v]] : 1.f;
    K[v] = sel ? gc * wy : 0.f;
    any |= sel;
  }
  return any;
}

// class vector in registers (C <= CPAD <= 32): the logits are read once
template <typename T, int CPAD, int VEC>
__global__ __launch_bounds__(256) void train_ce_bwd_reg_k(const T* __restrict__ logits, const long long* __restrict__ y,
                                                          const float* __restrict__ w, long long ignore, int C,
                                                          int64_t HW, const float* __restrict__ loss_px, int ohem,
                                                          const float* __restrict__ g,
                                                          const TrainWords* __restrict__ words,
                                                          T* __restrict__ dlogits) {
  using R = typename Elem<T>::raw;
  using P = typename RawVec<R, VEC>::type;
  const int b = blockIdx.y;
  const int64_t px0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (px0 >= HW) return;
  const float gc = g[0] * words->coef;
  int lab[VEC];
  float K[VEC];
  const bool any = bwd_labels<VEC>(y, loss_px, w, (int64_t)b * HW + px0, ignore, C, ohem, gc, lab, K);
  const R* src = reinterpret_cast<const R*>(logits) + (int64_t)b * C * HW + px0;
  R* dst = reinterpret_cast<R*>(dlogits) + (int64_t)b * C * HW + px0;
  float z[CPAD][VEC];
  float A[VEC];
  if (any) {  // a lane whose pixels are all unselected reads no logits
#pragma unroll
    for (int c = 0; c < CPAD; ++c) {
      if (c < C) {
        const P p = __builtin_nontemporal_load(reinterpret_cast<const P*>(src + (int64_t)c * HW));
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[c][v] = Elem<T>::to_f(vec_get<R, VEC>(p, v));
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[c][v] = -INFINITY;
      }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float m = z[0][v];
#pragma unroll
      for (int c = 1; c < CPAD; ++c) m = fmaxf(m, z[c][v]);
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < CPAD; ++c) {
        const float e = expf(z[c][v] - m);  // padded classes: exp(-inf) = 0
        z[c][v] = e;
        s += (double)e;
      }
      A[v] = (float)((double)K[v] / s);
    }
  }
#pragma unroll
  for (int c = 0; c < CPAD; ++c) {
    if (c < C) {
      P p;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float gr = 0.f;
        if (any && lab[v] >= 0) {
          const float t = A[v] * z[c][v];
          gr = (lab[v] == c) ? t - K[v] : t;
        }
        vec_set<R, VEC>(p, v, Elem<T>::from_f(gr));
      }
      __builtin_nontemporal_store(p, reinterpret_cast<P*>(dst + (int64_t)c * HW));
    }
  }
}

// any C: soft-max statistics from a first pass over the class planes, the gradient from a second
template <typename T, int VEC>
__global__ __launch_bounds__(256) void train_ce_bwd_stream_k(const T* __restrict__ logits,
                                                             const long long* __restrict__ y,
                                                             const float* __restrict__ w, long long ignore, int C,
                                                             int64_t HW, const float* __restrict__ loss_px, int ohem,
                                                             const float* __restrict__ g,
                                                             const TrainWords* __restrict__ words,
                                                             T* __restrict__ dlogits) {
  using R = typename Elem<T>::raw;
  using P = typename RawVec<R, VEC>::type;
  constexpr int CH = 4;
  const int b = blockIdx.y;
  const int64_t px0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (px0 >= HW) return;
  const float gc = g[0] * words->coef;
  int lab[VEC];
  float K[VEC];
  const bool any = bwd_labels<VEC>(y, loss_px, w, (int64_t)b * HW + px0, ignore, C, ohem, gc, lab, K);
  const R* src = reinterpret_cast<const R*>(logits) + (int64_t)b * C * HW + px0;
  R* dst = reinterpret_cast<R*>(dlogits) + (int64_t)b * C * HW + px0;
  if (!any) {  // nothing selected in this lane: zeros, no logits read
    P zero;
#pragma unroll
    for (int v = 0; v < VEC; ++v) vec_set<R, VEC>(zero, v, Elem<T>::from_f(0.f));
    for (int c = 0; c < C; ++c) __builtin_nontemporal_store(zero, reinterpret_cast<P*>(dst + (int64_t)c * HW));
    return;
  }
  float m[VEC], zy[VEC], A[VEC];
  double s[VEC];
  class_stats<T, VEC>(logits + (int64_t)b * C * HW + px0, C, HW, lab, m, s, zy);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    A[v] = (float)((double)K[v] / s[v]);
    m[v] = (m[v] == -INFINITY) ? -3.0e38f : m[v];
  }
  for (int c0 = 0; c0 < C; c0 += CH) {
    P p[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (c0 + j < C) p[j] = *reinterpret_cast<const P*>(src + (int64_t)(c0 + j) * HW);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      if (c0 + j < C) {
        P o;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          float gr = 0.f;
          if (lab[v] >= 0) {
            const float t = A[v] * expf(Elem<T>::to_f(vec_get<R, VEC>(p[j], v)) - m[v]);
            gr = (lab[v] == c0 + j) ? t - K[v] : t;
          }
          vec_set<R, VEC>(o, v, Elem<T>::from_f(gr));
        }
        __builtin_nontemporal_store(o, reinterpret_cast<P*>(dst + (int64_t)(c0 + j) * HW));
      }
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static inline bool aligned_for(const void* p, size_t bytes) { return (((uintptr_t)p) % bytes) == 0; }

template <typename T>
static int fwd_launch(const void* logits, const void* y, const float* w, long long ignore, float thresh, int B, int C,
                      int64_t HW, float* loss_px, TrainRecord* rec, TrainWords* words, hipStream_t s, int* n_rec) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = (HW % V) == 0 && aligned_for(logits, 16) && aligned_for(loss_px, 4 * V);
  if (vec) {
    dim3 grid(tiles_for(HW, V), B);
    hipLaunchKernelGGL((train_ce_fwd_k<T, V>), grid, dim3(256), 0, s, (const T*)logits, (const long long*)y, w, ignore,
                       thresh, C, HW, loss_px, rec, words);
    *n_rec = (int)grid.x * B;
  } else {
    dim3 grid(tiles_for(HW, 1), B);
    hipLaunchKernelGGL((train_ce_fwd_k<T, 1>), grid, dim3(256), 0, s, (const T*)logits, (const long long*)y, w, ignore,
                       thresh, C, HW, loss_px, rec, words);
    *n_rec = (int)grid.x * B;
  }
  return 0;
}

template <typename T, int VEC>
static void bwd_launch_reg(const void* logits, const void* y, const float* w, long long ignore, int B, int C, int64_t HW,
                           const float* loss_px, int ohem, const float* g, const TrainWords* words, void* dlogits,
                           hipStream_t s) {
  dim3 grid(tiles_for(HW, VEC), B), block(256);
#define SEA_T2_REG(CP)                                                                                               \
  hipLaunchKernelGGL((train_ce_bwd_reg_k<T, CP, VEC>), grid, block, 0, s, (const T*)logits, (const long long*)y, w, \
                     ignore, C, HW, loss_px, ohem, g, words, (T*)dlogits)
  if (C <= 8)
    SEA_T2_REG(8);
  else if (C <= 16)
    SEA_T2_REG(16);
  else if (C <= 24)
    SEA_T2_REG(24);
  else
    SEA_T2_REG(32);
#undef SEA_T2_REG
}

template <typename T>
static int bwd_launch(const void* logits, const void* y, const float* w, long long ignore, int B, int C, int64_t HW,
                      const float* loss_px, int ohem, const float* g, const TrainWords* words, void* dlogits,
                      hipStream_t s) {
  if (C <= 32) {
    const bool vec = (HW % 4) == 0 && aligned_for(logits, 4 * sizeof(T)) && aligned_for(dlogits, 4 * sizeof(T));
    if (vec)
      bwd_launch_reg<T, 4>(logits, y, w, ignore, B, C, HW, loss_px, ohem, g, words, dlogits, s);
    else
      bwd_launch_reg<T, 1>(logits, y, w, ignore, B, C, HW, loss_px, ohem, g, words, dlogits, s);
    return 0;
  }
  constexpr int V = 16 / (int)sizeof(T);
  const bool vec = (HW % V) == 0 && aligned_for(logits, 16) && aligned_for(dlogits, 16);
#define SEA_T2_STREAM(VV)                                                                                            \
  hipLaunchKernelGGL((train_ce_bwd_stream_k<T, VV>), dim3(tiles_for(HW, VV), B), dim3(256), 0, s, (const T*)logits, \
                     (const long long*)y, w, ignore, C, HW, loss_px, ohem, g, words, (T*)dlogits)
  if (vec)
    SEA_T2_STREAM(V);
  else
    SEA_T2_STREAM(1);
#undef SEA_T2_STREAM
  return 0;
}

}  // namespace sea

using namespace sea;

extern "C" size_t sea_train_ce_workspace_bytes(int B, int64_t HW) {
  if (B <= 0 || HW <= 0) return 0;
  return kOffRecords + (size_t)B * (size_t)tiles_for(HW, 1) * sizeof(TrainRecord);
}

extern "C" int sea_train_ce_fwd(const void* logits, int dtype, const int64_t* y, const float* w, int64_t ignore_label,
                                float thresh, int reduce_mean, int B, int C, int64_t HW, float* loss_px, void* workspace,
                                size_t workspace_bytes, void* words, void* stream) {
  SEA_CHECK_ARG(logits && y && loss_px && workspace && words);
  SEA_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && HW > 0 && (int64_t)B * HW < ((int64_t)1 << 31));
  SEA_CHECK_ARG(dtype == SEA_DTYPE_F32 || dtype == SEA_DTYPE_BF16);
  SEA_CHECK_ARG(workspace_bytes >= sea_train_ce_workspace_bytes(B, HW));
  SEA_CHECK_ARG(aligned_for(workspace, 16) && aligned_for(words, 8) && aligned_for(y, 8));
  TrainRecord* rec = (TrainRecord*)((char*)workspace + kOffRecords);
  hipStream_t s = (hipStream_t)stream;
  int n_rec = 0;
  if (dtype == SEA_DTYPE_F32)
    fwd_launch<float>(logits, y, w, ignore_label, thresh, B, C, HW, loss_px, rec, (TrainWords*)words, s, &n_rec);
  else
    fwd_launch<__hip_bfloat16>(logits, y, w, ignore_label, thresh, B, C, HW, loss_px, rec, (TrainWords*)words, s, &n_rec);
  hipLaunchKernelGGL(train_reduce_k, dim3(1), dim3(256), 0, s, (const TrainRecord*)rec, n_rec, reduce_mean ? 0 : 1,
                     thresh, (int*)((char*)workspace + kOffHist), (TrainWords*)words);
  SEA_RETURN_LAST();
}

extern "C" int sea_train_ohem_select(float* loss_px, int64_t N, void* workspace, size_t workspace_bytes, void* words,
                                     void* stream) {
  SEA_CHECK_ARG(loss_px && workspace && words && N > 0 && N < ((int64_t)1 << 31));
  SEA_CHECK_ARG(workspace_bytes >= kOffRecords && aligned_for(workspace, 16) && aligned_for(words, 8));
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* hist = (int*)(ws + kOffHist);
  double* blk_sum = (double*)(ws + kOffBlkSum);
  int* blk_ties = (int*)(ws + kOffBlkTies);
  int* tie_base = (int*)(ws + kOffTieBase);
  const int G = sel_blocks(N);
  const int64_t chunk = sel_chunk(N);
  // every pass is launched unconditionally; in threshold mode the device flag makes the first five leave at once
  for (int pass = 0; pass < 4; ++pass)
    hipLaunchKernelGGL(ohem_hist_k, dim3(G), dim3(256), 0, s, (const float*)loss_px, N, chunk, pass, hist,
                       (const TrainWords*)words);
  hipLaunchKernelGGL(ohem_sum_k, dim3(G), dim3(256), 0, s, (const float*)loss_px, N, chunk, (const int*)hist, blk_sum,
                     blk_ties, (const TrainWords*)words);
  hipLaunchKernelGGL(ohem_finish_k, dim3(1), dim3(256), 0, s, G, (const int*)hist, (const double*)blk_sum,
                     (const int*)blk_ties, tie_base, (TrainWords*)words);
  hipLaunchKernelGGL(ohem_mark_k, dim3(G), dim3(256), 0, s, loss_px, N, chunk, (const int*)tie_base,
                     (const TrainWords*)words);
  SEA_RETURN_LAST();
}

extern "C" int sea_train_ce_bwd(const void* logits, int dtype, const int64_t* y, const float* w, int64_t ignore_label,
                                int ohem, int B, int C, int64_t HW, const float* loss_px, const float* g,
                                const void* words, void* dlogits, void* stream) {
  SEA_CHECK_ARG(logits && y && loss_px && g && words && dlogits);
  SEA_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && HW > 0 && (int64_t)B * HW < ((int64_t)1 << 31));
  SEA_CHECK_ARG(dtype == SEA_DTYPE_F32 || dtype == SEA_DTYPE_BF16);
  SEA_CHECK_ARG(aligned_for(words, 8) && aligned_for(y, 8));
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SEA_DTYPE_F32)
    bwd_launch<float>(logits, y, w, ignore_label, B, C, HW, loss_px, ohem, g, (const TrainWords*)words, dlogits, s);
  else
    bwd_launch<__hip_bfloat16>(logits, y, w, ignore_label, B, C, HW, loss_px, ohem, g, (const TrainWords*)words, dlogits, s);
  SEA_RETURN_LAST();
}
