// K2: fused per-pixel SEA loss forward + logit gradient + tracking loss + accuracy + argmax.
//
// Roofline: HBM.  Algorithmic bytes per pixel (fp32, with gradient): 2*C*4 (read logits, write
// dlogits) + label + pred.  One pass: every logit is loaded from HBM exactly once, kept in
// registers (class vector of a pixel = CPAD registers per lane, VEC pixels per lane), and its
// gradient is written exactly once.
//
// Layout NCHW ("class planes"): lane l of a wave owns VEC consecutive pixels; for every class c the
// wave reads one contiguous 64*VEC*4-byte segment of plane c -> perfectly coalesced
// global_load_dwordx4 (VEC=4) with C independent loads in flight per lane (latency hiding by ILP,
// no LDS needed because there is no reuse across lanes: the class reduction is within a lane).
//
// Per-image sums (loss, tracking loss, #correct) are reduced wave -> block with shuffles + LDS and
// written as one record per block; a second tiny kernel sums the records of an image in a fixed
// order in double precision.  No float atomics => bitwise run-to-run determinism.
#include "loss_common.h"

namespace sea {

// ---- NCHW, class vector in registers ---------------------------------------------------------
// grid = (tiles per image, B); block = 256 threads; tile = 256*VEC consecutive pixels of one image.
// CPAD = number of class registers; EXACT means C == CPAD (no per-class guards at all).
//
// Codegen notes (each one was a measured register-file problem):
//  * planes are addressed as ONE wave-uniform 64-bit pointer (SGPR pair, global address space)
//    advanced by HW per class, plus a 32-bit per-lane byte offset -> `global_load_dwordx4 v, v_off,
//    s[ptr:ptr+1]`.  The empty asm keeps the running pointer opaque so that the compiler does not
//    materialise C separate 64-bit plane addresses.
//  * argmax is computed as max-chain followed by a descending "first index equal to the max" scan;
//    the textbook `if (z > m) { m = z; arg = c; }` makes the compiler keep C 64-bit lane masks alive
//    (one per compare) and spill them.
//  * the label compares of the gradient pass use an opaque copy of the label so they are not CSE'd
//    with those of the z_y select (same reason).
// TUNE bits (benchmark variants): 1 = non-temporal gradient stores, 2 = non-temporal logit loads,
// 4 = ask for 4 waves/SIMD (<= 128 VGPRs)
template <typename T, int CPAD, int VEC, bool GRAD, bool EXACT, int TUNE = 0>
__global__ __launch_bounds__(256, (TUNE & 4) ? 4 : 1) void loss_nchw_reg(const T* __restrict__ logits, const void* __restrict__ y,
                                                     int y_bytes, const float* __restrict__ w, int mode,
                                                     int track_mode, int C, int64_t HW, float gscale,
                                                     T* __restrict__ dlogits, void* __restrict__ pred,
                                                     int pred_bytes, float* __restrict__ loss_px,
    BlockPartial* __restrict__ partials) {
  using R = typename Elem<T>::raw;
  using P = typename RawVec<R, VEC>::type;
  const int b = blockIdx.y;
  const int64_t px0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  const bool active = px0 < HW;  // HW % VEC == 0 is guaranteed by the launcher
  const uint32_t lane_off = (uint32_t)(threadIdx.x * VEC * sizeof(T));
  if (EXACT) C = CPAD;

  float z[CPAD][VEC];
  int lab[VEC];
#pragma unroll
  for (int c = 0; c < CPAD; ++c)
#pragma unroll
    for (int v = 0; v < VEC; ++v) z[c][v] = -INFINITY;
#pragma unroll
  for (int v = 0; v < VEC; ++v) lab[v] = -1;

  if (active) {
    // labels first: their latency hides under the C plane loads issued right after
    load_labels<VEC>(y, y_bytes, (int64_t)b * HW + px0, lab);
    gptr<char> plane = (gptr<char>)(logits + (int64_t)b * C * HW + (int64_t)blockIdx.x * 256 * VEC);
    const int64_t plane_bytes = HW * (int64_t)sizeof(T);
#pragma unroll
    for (int c = 0; c < CPAD; ++c) {
      if (EXACT || c < C) {
        P p;
        if (TUNE & 2)
          p = __builtin_nontemporal_load(reinterpret_cast<gptr<P>>(plane + lane_off));
        else
          p = *reinterpret_cast<gptr<P>>(plane + lane_off);
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[c][v] = Elem<T>::to_f(vec_get<R, VEC>(p, v));
      }
      plane += plane_bytes;
      asm volatile("" : "+s"(plane));
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) lab[v] = (lab[v] < 0 || lab[v] >= C) ? -1 : lab[v];
  }

  float lsum = 0.f, tsum = 0.f;
  int ncorr = 0;
  float K[VEC];  // gradient = K * (p_c - [c == y])
  float A[VEC];  // K / sum_exp
  int amax[VEC];
  float lpx[VEC];

#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    float m = z[0][v];
#pragma unroll
    for (int c = 1; c < CPAD; ++c) m = fmaxf(m, z[c][v]);
    // first index attaining the maximum (torch.max tie-break): descending scan, last write wins
    int arg = 0;
    float zy = 0.f;
#pragma unroll
    for (int c = CPAD - 1; c >= 0; --c) {
      const float zc = z[c][v];
      arg = (zc == m) ? c : arg;
      zy = (lab[v] == c) ? zc : zy;
    }
    // Order fence (no instruction): the exp pass below overwrites z in place, so the scan above must
    // be complete first; without it the compiler runs exp early into fresh registers and keeps
    // BOTH z and exp(z-m) alive (2x the register file, half the occupancy).
    asm volatile("" : "+v"(m) : "v"(arg), "v"(zy));
    // From here on the maximum is kept finite (any finite maximum is unchanged).  Under a maximum of +-inf exp(z - m) would
    // be NaN at the +-inf logits themselves (inf - inf); with the clamp it is +inf or 0 there and NaN at NaN logits only.
    m = fminf(fmaxf(m, -3.402823466e38f), 3.402823466e38f);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CPAD; ++c) {
      const float e = __expf(z[c][v] - m);  // padded classes: exp(-inf) = 0
      z[c][v] = e;
      s += e;
    }
    // torch.max semantics for non-finite logits (reference attacker.py:145, 370, 485): the first NaN wins, else the
    // first maximum.  The fmaxf chain above ignores NaNs and the scan gives the first maximum, +-inf included; exp(z - m)
    // with the clamped m is NaN exactly at the NaN logits, so the sum flags them and the first NaN among the e's is
    // torch's index.  (Without the clamp a +inf ahead of a NaN was a NaN too and won.)  Never taken for finite logits.
    if (__builtin_expect(s != s, 0)) {
#pragma unroll
      for (int c = CPAD - 1; c >= 0; --c) arg = (z[c][v] != z[c][v]) ? c : arg;
    }
    const bool valid = active && lab[v] >= 0;
    const bool correct = valid && (arg == lab[v]);
    const float lse = m + __logf(s);
    const float ce = lse - zy;
    const float logp = zy - lse;
    const bool need_js = (mode == SEA_MODE_JS) || (track_mode == SEA_MODE_JS);
    float py = 0.f, l1p = 0.f;
    if (need_js) {
      py = __expf(logp);
      l1p = __logf(1.f + py);
    }
    const bool need_w = (mode == SEA_MODE_MASK_CE_BAL) || (track_mode == SEA_MODE_MASK_CE_BAL);
    const float wy = (need_w && valid) ? w[lab[v]] : 1.f;
    const float lv = loss_value(mode, valid, correct, ce, logp, py, l1p, wy);
    lsum += lv;
    lpx[v] = lv;
    tsum += (track_mode == mode) ? lv : loss_value(track_mode, valid, correct, ce, logp, py, l1p, wy);
    ncorr += correct ? 1 : 0;
    amax[v] = arg;
    if (GRAD) {
      K[v] = grad_coef(mode, valid, correct, logp, py, l1p, wy) * gscale;
      A[v] = K[v] / s;
    }
  }

  if (active) {
    if (pred != nullptr) {
      store_indices<VEC>(pred, pred_bytes, (int64_t)b * HW + px0, amax);
    }
    if (loss_px != nullptr) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) loss_px[(int64_t)b * HW + px0 + v] = lpx[v];
    }
    if (GRAD) {
      gptr_w<char> gplane = (gptr_w<char>)(dlogits + (int64_t)b * C * HW + (int64_t)blockIdx.x * 256 * VEC);
      const int64_t plane_bytes = HW * (int64_t)sizeof(T);
      int lab2[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        lab2[v] = lab[v];
        asm volatile("" : "+v"(lab2[v]));
      }
#pragma unroll
      for (int c = 0; c < CPAD; ++c) {
        if (EXACT || c < C) {
          P p;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            // K*(e_c/s - [c==y]) = A*e_c - (c==y ? K : 0)
            const float g = A[v] * z[c][v];
            vec_set<R, VEC>(p, v, Elem<T>::from_f((lab2[v] == c) ? g - K[v] : g));
          }
          if (TUNE & 1)
            __builtin_nontemporal_store(p, reinterpret_cast<gptr_w<P>>(gplane + lane_off));
          else
            *reinterpret_cast<gptr_w<P>>(gplane + lane_off) = p;
        }
        gplane += plane_bytes;
        asm volatile("" : "+s"(gplane));
      }
    }
  }
  block_reduce_store(lsum, tsum, ncorr, partials);
}

// ---- NCHW, any C: two passes over the class planes (second pass re-reads; used only when the class
// vector does not fit the register file) ---------------------------------------------------------------
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void loss_nchw_stream(const T* __restrict__ logits, const void* __restrict__ y,
                                                        int y_bytes, const float* __restrict__ w, int mode,
                                                        int track_mode, int C, int64_t HW, float gscale,
                                                        T* __restrict__ dlogits, void* __restrict__ pred,
                                                        int pred_bytes, float* __restrict__ loss_px,
    BlockPartial* __restrict__ partials) {
  const int b = blockIdx.y;
  const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool active = px < HW;
  using R = typename Elem<T>::raw;
  const R* lbase = reinterpret_cast<const R*>(logits) + (int64_t)b * C * HW + px;
  float lsum = 0.f, tsum = 0.f;
  int ncorr = 0;
  if (active) {
    int lab = load_label_rt(y, y_bytes, (int64_t)b * HW + px);
    lab = (lab < 0 || lab >= C) ? -1 : lab;
    // online max / sum-exp: one read of every plane
    float m = Elem<T>::to_f(lbase[0]);
    int arg = 0;
    float s = 1.f;
    float zy = (lab == 0) ? m : 0.f;
    for (int c = 1; c < C; ++c) {
      const float zc = Elem<T>::to_f(lbase[(int64_t)c * HW]);
      zy = (lab == c) ? zc : zy;
      if (!(zc <= m) && !(m != m)) {  // zc > m, or zc is the first NaN (torch.max: a NaN wins and stays)
        s = s * __expf(m - zc) + 1.f;
        m = zc;
        arg = c;
      } else {
        // a -inf logit adds nothing; under a running maximum of -inf (masked leading classes) exp(-inf - -inf) would be NaN
        s += (zc == -INFINITY) ? 0.f : __expf(zc - m);
      }
    }
    const bool valid = lab >= 0;
    const bool correct = valid && arg == lab;
    const float lse = m + __logf(s);
    const float ce = lse - zy, logp = zy - lse;
    const float py = __expf(logp), l1p = __logf(1.f + py);
    const bool need_w = (mode == SEA_MODE_MASK_CE_BAL) || (track_mode == SEA_MODE_MASK_CE_BAL);
    const float wy = (need_w && valid) ? w[lab] : 1.f;
    lsum = loss_value(mode, valid, correct, ce, logp, py, l1p, wy);
    tsum = (track_mode == mode) ? lsum : loss_value(track_mode, valid, correct, ce, logp, py, l1p, wy);
    ncorr = correct ? 1 : 0;
    if (pred != nullptr) store_index_rt(pred, pred_bytes, (int64_t)b * HW + px, arg);
    if (loss_px != nullptr) loss_px[(int64_t)b * HW + px] = lsum;
    if (GRAD) {
      const float k = grad_coef(mode, valid, correct, logp, py, l1p, wy) * gscale;
      R* gbase = reinterpret_cast<R*>(dlogits) + (int64_t)b * C * HW + px;
      if (k == 0.f) {
        for (int c = 0; c < C; ++c) gbase[(int64_t)c * HW] = Elem<T>::from_f(0.f);
      } else {
        for (int c = 0; c < C; ++c) {
          const float pc = __expf(Elem<T>::to_f(lbase[(int64_t)c * HW]) - lse);
          gbase[(int64_t)c * HW] = Elem<T>::from_f(k * (pc - ((lab == c) ? 1.f : 0.f)));
        }
      }
    }
  }
  block_reduce_store(lsum, tsum, ncorr, partials);
}

// ---- NHWC (channels_last logits): the class vector of a pixel is contiguous -----------------------
// A block stages 256 pixels x C classes through LDS with coalesced accesses, each lane then walks its
// pixel's row in LDS (row stride padded to an odd number of dwords -> bank-conflict free).
template <typename T, bool GRAD>
__global__ __launch_bounds__(256) void loss_nhwc_lds(const T* __restrict__ logits, const void* __restrict__ y,
                                                     int y_bytes, const float* __restrict__ w, int mode,
                                                     int track_mode, int C, int CS /*row stride, floats*/,
                                                     int64_t HW, float gscale, T* __restrict__ dlogits,
                                                     void* __restrict__ pred, int pred_bytes, float* __restrict__ loss_px,
                                                     BlockPartial* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [256][CS]
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * 256;
  const int npx = (int)min((int64_t)256, HW - p0);
  using R = typename Elem<T>::raw;
  const R* src = reinterpret_cast<const R*>(logits) + ((int64_t)b * HW + p0) * C;
  const int total = npx * C;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int p = i / C, c = i - p * C;
    tile[p * CS + c] = Elem<T>::to_f(src[i]);
  }
  __syncthreads();
  float lsum = 0.f, tsum = 0.f;
  int ncorr = 0;
  const int t = threadIdx.x;
  if (t < npx) {
    float* row = tile + t * CS;
    int lab = load_label_rt(y, y_bytes, (int64_t)b * HW + p0 + t);
    lab = (lab < 0 || lab >= C) ? -1 : lab;
    float m = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float zc = row[c];
      if (!(zc <= m) && !(m != m)) {  // zc > m, or zc is the first NaN (torch.max semantics)
        m = zc;
        arg = c;
      }
    }
    const float zy = lab >= 0 ? row[lab] : 0.f;
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = __expf(row[c] - m);
      row[c] = e;
      s += e;
    }
    const bool valid = lab >= 0;
    const bool correct = valid && arg == lab;
    const float lse = m + __logf(s);
    const float ce = lse - zy, logp = zy - lse;
    const float py = __expf(logp), l1p = __logf(1.f + py);
    const bool need_w = (mode == SEA_MODE_MASK_CE_BAL) || (track_mode == SEA_MODE_MASK_CE_BAL);
    const float wy = (need_w && valid) ? w[lab] : 1.f;
    lsum = loss_value(mode, valid, correct, ce, logp, py, l1p, wy);
    tsum = (track_mode == mode) ? lsum : loss_value(track_mode, valid, correct, ce, logp, py, l1p, wy);
    ncorr = correct ? 1 : 0;
    if (pred != nullptr) store_index_rt(pred, pred_bytes, (int64_t)b * HW + p0 + t, arg);
    if (loss_px != nullptr) loss_px[(int64_t)b * HW + p0 + t] = lsum;
    if (GRAD) {
      const float k = grad_coef(mode, valid, correct, logp, py, l1p, wy) * gscale;
      const float a = k / s;
      for (int c = 0; c < C; ++c) {
        const float g = a * row[c];
        row[c] = (lab == c) ? g - k : g;
      }
    }
  }
  if (GRAD) {
    __syncthreads();
    R* dst = reinterpret_cast<R*>(dlogits) + ((int64_t)b * HW + p0) * C;
    for (int i = threadIdx.x; i < total; i += 256) {
      const int p = i / C, c = i - p * C;
      dst[i] = Elem<T>::from_f(tile[p * CS + c]);
    }
  }
  block_reduce_store(lsum, tsum, ncorr, partials);
}

// ---- second stage: fixed-order sum of the per-block records of each image ------------------------
__global__ __launch_bounds__(256) void loss_finalize(const BlockPartial* __restrict__ partials, int tiles,
                                                     float* __restrict__ loss_sum, float* __restrict__ track_sum,
                                                     int32_t* __restrict__ n_correct) {
  __shared__ double s_l[256], s_t[256];
  __shared__ int s_n[256];
  const int b = blockIdx.x;
  double l = 0.0, t = 0.0;
  int n = 0;
  for (int i = threadIdx.x; i < tiles; i += 256) {
    const BlockPartial p = partials[1 + (int64_t)b * tiles + i];
    l += (double)p.loss;
    t += (double)p.track;
    n += p.n_correct;
  }
  s_l[threadIdx.x] = l;
  s_t[threadIdx.x] = t;
  s_n[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s_l[threadIdx.x] += s_l[threadIdx.x + o];
      s_t[threadIdx.x] += s_t[threadIdx.x + o];
      s_n[threadIdx.x] += s_n[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_sum[b] = (float)s_l[0];
    track_sum[b] = (float)s_t[0];
    n_correct[b] = s_n[0];
  }
}

// ---- launch ----------------------------------------------------------------------------------------
// The launchers decide nothing: kernel, template parameters and grid come from the plan (loss_plan.h).
#define SEA_K2_ARGS(T) \
  (const T*)a.logits, a.y, a.y_bytes, a.w, a.mode, a.track_mode, a.C, a.HW, a.gscale, (T*)a.dlogits, a.pred, a.pred_bytes

template <typename T, int CPAD, int VEC>
static int launch_reg_as(const LossArgs& a, const LossPlan& p) {
  const bool g = a.dlogits != nullptr;
  auto k = g ? (p.exact ? loss_nchw_reg<T, CPAD, VEC, true, true> : loss_nchw_reg<T, CPAD, VEC, true, false>)
             : (p.exact ? loss_nchw_reg<T, CPAD, VEC, false, true> : loss_nchw_reg<T, CPAD, VEC, false, false>);
  // the three fp32 TUNE instantiations that ship (loss_plan.h), each of them EXACT; 0 elsewhere = the kernels above
  constexpr bool voc = sizeof(T) == 4 && CPAD == 21 && VEC == 4, ade = sizeof(T) == 4 && CPAD == 151;
  if (p.tune) k = g ? loss_nchw_reg<T, CPAD, VEC, true, true, voc ? 7 : ade ? 2 : 0> : loss_nchw_reg<T, CPAD, VEC, false, true, voc ? 6 : 0>;
  hipLaunchKernelGGL(k, dim3(p.tiles, a.B), dim3(256), 0, a.s, SEA_K2_ARGS(T), a.loss_px, a.partials);
  return 0;
}

template <typename T>
static int launch_reg(const LossArgs& a, const LossPlan& p) {
  switch (p.cpad * 8 + p.vec) {
#define SEA_REG(CP, V) \
  case CP * 8 + V: return launch_reg_as<T, CP, V>(a, p);
    SEA_K2_REG_INSTANCES(SEA_REG)
#undef SEA_REG
  }
  return SEA_ERR_ARG;
}

template <typename T>
static int launch_stream(const LossArgs& a, const LossPlan& p) {
  auto k = a.dlogits ? loss_nchw_stream<T, true> : loss_nchw_stream<T, false>;
  hipLaunchKernelGGL(k, dim3(p.tiles, a.B), dim3(256), 0, a.s, SEA_K2_ARGS(T), a.loss_px, a.partials);
  return 0;
}

template <typename T>
static int launch_nhwc(const LossArgs& a, const LossPlan& p) {
  auto k = a.dlogits ? loss_nhwc_lds<T, true> : loss_nhwc_lds<T, false>;
  if (p.lds > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL(k, dim3(p.tiles, a.B), dim3(256), p.lds, a.s, (const T*)a.logits, a.y, a.y_bytes, a.w, a.mode,
                     a.track_mode, a.C, a.C | 1, a.HW, a.gscale, (T*)a.dlogits, a.pred, a.pred_bytes, a.loss_px, a.partials);
  return 0;
}
#undef SEA_K2_ARGS

template <typename T>
static int launch(const LossArgs& a, const LossPlan& p) {
  constexpr int (*by_kernel[])(const LossArgs&, const LossPlan&) = {  // in K2Kernel's order
      launch_reg<T>, launch_stream<T>, launch_fwd<T>, launch_split<T>, launch_nhwc<T>};
  return by_kernel[p.kernel](a, p);
}

static int elem_bytes_of(int dtype) { return dtype == SEA_DTYPE_F32 ? 4 : (dtype == SEA_DTYPE_BF16 || dtype == SEA_DTYPE_F16) ? 2 : 0; }

}  // namespace sea

using namespace sea;

extern "C" size_t sea_loss_workspace_bytes(int B, int64_t HW) {
  if (B <= 0 || HW <= 0) return 0;
  return ((size_t)B * (size_t)max_tiles(HW) + 1) * sizeof(BlockPartial);
}

// check the arguments, plan, launch the plan, finalize.  `variant`: a SEA_K2_* word that pins a kernel (tests, A/B runs)
extern "C" int sea_loss_fwd_bwd_tuned(const void* logits, int dtype, int layout, const void* y, int y_bytes,
                                      const float* w, int mode, int track_mode, int B, int C, int64_t HW,
                                      float grad_scale, void* dlogits, void* pred, int pred_bytes, float* loss_px,
                                      void* workspace, size_t workspace_bytes, float* loss_sum, float* track_sum,
                                      int32_t* n_correct, void* stream, int variant) {
  SEA_CHECK_ARG(logits && y && workspace);
  // loss_sum == track_sum == n_correct == NULL: leave the per-block records in the workspace for
  // sea_apgd_track (one launch less in the APGD loop)
  const bool deferred = !loss_sum && !track_sum && !n_correct;
  SEA_CHECK_ARG(deferred || (loss_sum && track_sum && n_correct));
  SEA_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && HW > 0);
  SEA_CHECK_ARG(mode >= 0 && mode <= 3 && track_mode >= 0 && track_mode <= 3);
  SEA_CHECK_ARG(!((mode == SEA_MODE_MASK_CE_BAL || track_mode == SEA_MODE_MASK_CE_BAL) && w == nullptr));
  SEA_CHECK_ARG(y_bytes == 8 || y_bytes == 4 || y_bytes == 2 || y_bytes == 1);
  SEA_CHECK_ARG(pred == nullptr || pred_bytes == 8 || pred_bytes == 4 || pred_bytes == 2 || pred_bytes == 1);
  SEA_CHECK_ARG(!(pred && pred_bytes == 1 && C > 255) && !(pred && pred_bytes == 2 && C > 32767));
  SEA_CHECK_ARG(!(y_bytes == 1 && C > 255));
  SEA_CHECK_ARG(workspace_bytes >= sea_loss_workspace_bytes(B, HW));
  SEA_CHECK_ARG((((uintptr_t)workspace) & 15) == 0);
  LossPlan plan;
  int rc = loss_plan(LossQuery{elem_bytes_of(dtype), layout, C, HW, dlogits != nullptr, (uintptr_t)logits,
                               (uintptr_t)dlogits, (unsigned)variant}, &plan);
  if (rc) return rc;
  const LossArgs a{logits, y, y_bytes, w, mode, track_mode, B, C, HW, grad_scale, dlogits, pred, pred_bytes,
                   loss_px, (BlockPartial*)workspace, (hipStream_t)stream};
  switch (dtype) {
    case SEA_DTYPE_F32: rc = launch<float>(a, plan); break;
    case SEA_DTYPE_BF16: rc = launch<__hip_bfloat16>(a, plan); break;
    default: rc = launch<__half>(a, plan); break;
  }
  if (rc) return rc;
  if (!deferred)
    hipLaunchKernelGGL(loss_finalize, dim3(B), dim3(256), 0, a.s, (const BlockPartial*)workspace, plan.tiles, loss_sum,
                       track_sum, n_correct);
  SEA_RETURN_LAST();
}

extern "C" int sea_loss_fwd_bwd(const void* logits, int dtype, int layout, const void* y, int y_bytes,
                                const float* w, int mode, int track_mode, int B, int C, int64_t HW,
                                float grad_scale, void* dlogits, void* pred, int pred_bytes, float* loss_px,
                                void* workspace, size_t workspace_bytes, float* loss_sum, float* track_sum, int32_t* n_correct,
                                void* stream) {
  return sea_loss_fwd_bwd_tuned(logits, dtype, layout, y, y_bytes, w, mode, track_mode, B, C, HW, grad_scale, dlogits, pred,
                                pred_bytes, loss_px, workspace, workspace_bytes, loss_sum, track_sum, n_correct, stream,
                                SEA_K2_VARIANT_DEFAULT);
}

// host only: the plan of a call, without the call
extern "C" int sea_loss_plan(int dtype, int layout, int C, int64_t HW, int want_grad, size_t logits_addr,
                             size_t dlogits_addr, unsigned variant, int32_t out[8]) {
  SEA_CHECK_ARG(out != nullptr);
  LossPlan p;
  const int rc = loss_plan(LossQuery{elem_bytes_of(dtype), layout, C, HW, want_grad != 0, logits_addr, dlogits_addr,
                                     variant}, &p);
  const int v[8] = {p.kernel, p.cpad, p.exact, p.vec, p.tune, p.ch, p.waves, p.tiles};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return rc;
}
