// T1: train-mode BatchNorm2d (batch statistics) of PSPNet-ResNet50's outer PIR-AT step (reference
// tools/train_rob_seg.py:338-340 trains every nn.BatchNorm2d of backbones/resnet_ddcat.py and ddcat_psp.py on its batch),
// with the ReLU / residual-add + ReLU that follows each of them fused into the apply pass.
//
// Layout: fp32 dense NHWC, i.e. an (M, C) row-major matrix with M = B*H*W rows, C % 4 == 0; every lane moves one float4
// of channels (16-byte loads and stores).
//
// Forward (three launches):
//   bn_stats_partial  grid (chunks, channel tiles): a block owns a contiguous run of `rows_per_chunk` rows and a tile of
//                     up to 64 float4 columns; its 256 lanes are (column, row-slot) pairs, each keeping a Welford
//                     (count, mean, M2) over the rows r = row-slot (mod row-slots).  The row-slots are merged in
//                     increasing order through LDS with Chan's combine and the block writes its chunk's (mean, M2).
//   bn_stats_final    one lane per channel merges the chunks in increasing order (Chan) -> mean, invstd =
//                     1/sqrt(var_biased + eps), scale = gamma*invstd, and the running statistics exactly as torch:
//                     running <- (1-m)*running + m*batch, the variance unbiased (var * M/(M-1)); lane 0 adds 1 to
//                     num_batches_tracked.
//   bn_apply          y = (x - mean)*scale + beta, optionally + r, optionally ReLU.  (Not the folded x*scale + shift:
//                     where var << eps, as on the 2-row maps of the PPM's bin-1 branch, scale reaches gamma/sqrt(eps)
//                     and x*scale and shift cancel to ~1e-4 absolute; torch's own order does not.)
// Backward (three launches):
//   bn_bwd_partial    the same grid and order as the statistics: sums of g' and g'*xhat per chunk, g' = y > 0 ? g : 0
//                     for the ReLU epilogues (g' = g without), xhat = (x - mean)*invstd.
//   bn_bwd_final      chunks merged in increasing order -> dbeta = sum g', dgamma = sum g'*xhat.
//   bn_bwd_dx         dx = scale*(g' - dbeta/M - xhat*dgamma/M); the residual variant also writes g' (the gradient of r).
// The chunking depends on (M, C) alone and no float atomics are used: results are bitwise reproducible.
#include "sea_common.h"

namespace sea {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kBnThreads = 256;
constexpr int kBnTileC4 = 64;          // float4 columns per block: 1 KiB per row and load instruction
constexpr int kBnTargetBlocks = 1024;  // 4 blocks per CU
constexpr int kBnMaxChunks = 128;      // the final merges walk the chunks serially: at 900 chunks (C = 256, B = 8, 60^2)
                                       // that walk alone took longer than the whole statistics pass
constexpr int kBnMinRowsPerLane = 8;

struct BnGrid {
  int tc4, ry, ctiles, chunks;
  int64_t rpc;  // rows per chunk
};

static BnGrid bn_grid(int64_t M, int C) {
  BnGrid g;
  const int C4 = C / 4;
  g.tc4 = C4 < kBnTileC4 ? C4 : kBnTileC4;
  g.ry = kBnThreads / g.tc4;
  g.ctiles = (C4 + g.tc4 - 1) / g.tc4;
  int want = kBnTargetBlocks / g.ctiles;
  if (want > kBnMaxChunks) want = kBnMaxChunks;
  if (want < 1) want = 1;
  int64_t rpc = (M + want - 1) / want;
  const int64_t min_rpc = (int64_t)g.ry * kBnMinRowsPerLane;
  if (rpc < min_rpc) rpc = min_rpc;
  g.rpc = rpc;
  g.chunks = (int)((M + rpc - 1) / rpc);
  return g;
}

__device__ __forceinline__ void chan_merge(float& n, f4& mean, f4& m2, float nb, const f4& meanb, const f4& m2b) {
  if (nb == 0.f) return;
  const float nn = n + nb;
  const float wb = nb / nn;
  const f4 d = meanb - mean;
  mean = mean + d * wb;
  m2 = m2 + m2b + d * d * (n * wb);
  n = nn;
}

__global__ __launch_bounds__(kBnThreads) void bn_stats_partial_kernel(const f4* __restrict__ x, float* __restrict__ pmean,
                                                                      float* __restrict__ pm2, int64_t M, int C4, int tc4,
                                                                      int ry, int64_t rpc) {
  __shared__ f4 s_mean[kBnThreads];
  __shared__ f4 s_m2[kBnThreads];
  __shared__ float s_n[kBnThreads];
  const int tid = threadIdx.x;
  const int tx = tid % tc4, ty = tid / tc4;
  const int c4 = blockIdx.y * tc4 + tx;
  const int64_t r0 = (int64_t)blockIdx.x * rpc;
  const int64_t r1 = r0 + rpc < M ? r0 + rpc : M;
  float n = 0.f;
  f4 mean = {0.f, 0.f, 0.f, 0.f}, m2 = {0.f, 0.f, 0.f, 0.f};
  if (ty < ry && c4 < C4) {
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += ry) {
      const f4 v = x[r * C4 + c4];
      n += 1.f;
      const float inv = 1.f / n;
      const f4 d = v - mean;
      mean = mean + d * inv;
      m2 = m2 + d * (v - mean);
    }
  }
  s_mean[tid] = mean;
  s_m2[tid] = m2;
  s_n[tid] = n;
  __syncthreads();
  if (ty == 0 && c4 < C4) {
    for (int k = 1; k < ry; ++k) {
      const int o = k * tc4 + tx;
      chan_merge(n, mean, m2, s_n[o], s_mean[o], s_m2[o]);
    }
    float* pm = pmean + (int64_t)blockIdx.x * C4 * 4 + 4 * c4;
    float* pq = pm2 + (int64_t)blockIdx.x * C4 * 4 + 4 * c4;
    *(f4*)pm = mean;
    *(f4*)pq = m2;
  }
}

__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ pmean,
                                                             const float* __restrict__ pm2, const float* __restrict__ gamma,
                                                             float* __restrict__ mean_out,
                                                             float* __restrict__ invstd_out, float* __restrict__ scale_out,
                                                             float* __restrict__ rmean,
                                                             float* __restrict__ rvar, int64_t* __restrict__ nbt, int64_t M,
                                                             int C, int chunks, int64_t rpc, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) nbt[0] = nbt[0] + 1;
  if (c >= C) return;
  float n = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll 8
  for (int k = 0; k < chunks; ++k) {
    const int64_t r0 = (int64_t)k * rpc;
    const float nb = (float)((r0 + rpc < M ? r0 + rpc : M) - r0);
    const float mb = pmean[(int64_t)k * C + c], qb = pm2[(int64_t)k * C + c];
    const float nn = n + nb;
    const float wb = nb / nn;
    const float d = mb - mean;
    mean = mean + d * wb;
    m2 = m2 + qb + d * d * (n * wb);
    n = nn;
  }
  const float var = m2 / (float)M;
  const float invstd = 1.f / sqrtf(var + eps);
  const float scale = gamma[c] * invstd;
  mean_out[c] = mean;
  invstd_out[c] = invstd;
  scale_out[c] = scale;
  if (rmean) rmean[c] = momentum * mean + (1.f - momentum) * rmean[c];
  if (rvar) rvar[c] = momentum * (m2 / (float)(M - 1)) + (1.f - momentum) * rvar[c];
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const f4* __restrict__ x, const f4* __restrict__ r,
                                                       const f4* __restrict__ mean, const f4* __restrict__ scale,
                                                       const f4* __restrict__ beta, f4* __restrict__ y, int64_t n4,
                                                       int C4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    f4 v = (x[i] - mean[c]) * scale[c] + beta[c];
    if (RES) v = v + r[i];
    if (RELU) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
    }
    y[i] = v;
  }
}

template <bool RELU>
__device__ __forceinline__ f4 gate(const f4& g, const f4* __restrict__ y, int64_t i) {
  if (!RELU) return g;
  const f4 yv = y[i];
  f4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = yv[k] > 0.f ? g[k] : 0.f;
  return o;
}

template <bool RELU>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_partial_kernel(const f4* __restrict__ g, const f4* __restrict__ y,
                                                                    const f4* __restrict__ x, const f4* __restrict__ mean,
                                                                    const f4* __restrict__ invstd, float* __restrict__ psg,
                                                                    float* __restrict__ psgx, int64_t M, int C4, int tc4,
                                                                    int ry, int64_t rpc) {
  __shared__ f4 s_a[kBnThreads];
  __shared__ f4 s_b[kBnThreads];
  const int tid = threadIdx.x;
  const int tx = tid % tc4, ty = tid / tc4;
  const int c4 = blockIdx.y * tc4 + tx;
  const int64_t r0 = (int64_t)blockIdx.x * rpc;
  const int64_t r1 = r0 + rpc < M ? r0 + rpc : M;
  f4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
  if (ty < ry && c4 < C4) {
    const f4 mu = mean[c4], is = invstd[c4];
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += ry) {
      const int64_t i = r * C4 + c4;
      const f4 gv = gate<RELU>(g[i], y, i);
      sa = sa + gv;
      sb = sb + gv * ((x[i] - mu) * is);
    }
  }
  s_a[tid] = sa;
  s_b[tid] = sb;
  __syncthreads();
  if (ty == 0 && c4 < C4) {
    for (int k = 1; k < ry; ++k) {
      sa = sa + s_a[k * tc4 + tx];
      sb = sb + s_b[k * tc4 + tx];
    }
    *(f4*)(psg + (int64_t)blockIdx.x * C4 * 4 + 4 * c4) = sa;
    *(f4*)(psgx + (int64_t)blockIdx.x * C4 * 4 + 4 * c4) = sb;
  }
}

__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ psg, const float* __restrict__ psgx,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int C,
                                                           int chunks) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
#pragma unroll 8
  for (int k = 0; k < chunks; ++k) {
    a += psg[(int64_t)k * C + c];
    b += psgx[(int64_t)k * C + c];
  }
  dbeta[c] = a;
  dgamma[c] = b;
}

template <bool RELU, bool RES>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const f4* __restrict__ g, const f4* __restrict__ y,
                                                        const f4* __restrict__ x, const f4* __restrict__ mean,
                                                        const f4* __restrict__ invstd, const f4* __restrict__ scale,
                                                        const f4* __restrict__ dgamma, const f4* __restrict__ dbeta,
                                                        f4* __restrict__ dx, f4* __restrict__ gr, int64_t n4, int C4,
                                                        float inv_m) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const f4 gv = gate<RELU>(g[i], y, i);
    const f4 xh = (x[i] - mean[c]) * invstd[c];
    dx[i] = scale[c] * (gv - dbeta[c] * inv_m - xh * (dgamma[c] * inv_m));
    if (RES) gr[i] = gv;
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace sea

using namespace sea;

extern "C" int64_t sea_bn_train_workspace_floats(int64_t M, int C) {
  if (M < 1 || C < 4 || C % 4) return -1;
  const BnGrid g = bn_grid(M, C);
  return 2 * (int64_t)g.chunks * C;
}

extern "C" int sea_bn_train_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* y,
                                float* mean, float* invstd, float* scale, float* running_mean,
                                float* running_var, int64_t* num_batches_tracked, float* work, int64_t M, int C,
                                float eps, float momentum, int relu, void* stream) {
  SEA_CHECK_ARG(x && gamma && beta && y && mean && invstd && scale && work && x != y && M >= 2 && C >= 4 &&
                C % 4 == 0 && (C / 4) < 65536 * kBnTileC4 && M * (C / 4) < (1ll << 40) && aligned16(x) &&
                aligned16(y) && aligned16(mean) && aligned16(scale) && aligned16(beta) && aligned16(work) &&
                (!r || aligned16(r)) &&
                (!r || r != y));
  const hipStream_t s = (hipStream_t)stream;
  const BnGrid g = bn_grid(M, C);
  const int C4 = C / 4;
  float* pmean = work;
  float* pm2 = work + (int64_t)g.chunks * C;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(g.chunks, g.ctiles), dim3(kBnThreads), 0, s, (const f4*)x, pmean,
                     pm2, M, C4, g.tc4, g.ry, g.rpc);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, pmean, pm2, gamma, mean,
                     invstd, scale, running_mean, running_var, num_batches_tracked, M, C, g.chunks, g.rpc, eps,
                     momentum);
  const int64_t n4 = M * C4;
  const dim3 grid(grid_for(n4, 256));
  if (r) {
    if (relu)
      hipLaunchKernelGGL((bn_apply_kernel<true, true>), grid, dim3(256), 0, s, (const f4*)x, (const f4*)r,
                         (const f4*)mean, (const f4*)scale, (const f4*)beta, (f4*)y, n4, C4);
    else
      hipLaunchKernelGGL((bn_apply_kernel<false, true>), grid, dim3(256), 0, s, (const f4*)x, (const f4*)r,
                         (const f4*)mean, (const f4*)scale, (const f4*)beta, (f4*)y, n4, C4);
  } else {
    if (relu)
      hipLaunchKernelGGL((bn_apply_kernel<true, false>), grid, dim3(256), 0, s, (const f4*)x, (const f4*)nullptr,
                         (const f4*)mean, (const f4*)scale, (const f4*)beta, (f4*)y, n4, C4);
    else
      hipLaunchKernelGGL((bn_apply_kernel<false, false>), grid, dim3(256), 0, s, (const f4*)x, (const f4*)nullptr,
                         (const f4*)mean, (const f4*)scale, (const f4*)beta, (f4*)y, n4, C4);
  }
  SEA_RETURN_LAST();
}

extern "C" int sea_bn_train_bwd(const float* g, const float* x, const float* y, const float* mean, const float* invstd,
                                const float* scale, float* dx, float* dgamma, float* dbeta, float* gr, float* work,
                                int64_t M, int C, int relu, void* stream) {
  SEA_CHECK_ARG(g && x && mean && invstd && scale && dx && dgamma && dbeta && work && (!relu || y) && (!gr || relu) &&
                M >= 2 && C >= 4 && C % 4 == 0 && (C / 4) < 65536 * kBnTileC4 && M * (C / 4) < (1ll << 40) &&
                dx != g && dx != x && (!y || dx != y) && aligned16(g) && aligned16(x) && (!y || aligned16(y)) &&
                aligned16(mean) && aligned16(invstd) && aligned16(scale) && aligned16(dx) && aligned16(dgamma) &&
                aligned16(dbeta) && aligned16(work) && (!gr || (aligned16(gr) && gr != dx && gr != g)));
  const hipStream_t s = (hipStream_t)stream;
  const BnGrid gd = bn_grid(M, C);
  const int C4 = C / 4;
  float* psg = work;
  float* psgx = work + (int64_t)gd.chunks * C;
  const dim3 pgrid(gd.chunks, gd.ctiles);
  if (relu)
    hipLaunchKernelGGL(bn_bwd_partial_kernel<true>, pgrid, dim3(kBnThreads), 0, s, (const f4*)g, (const f4*)y,
                       (const f4*)x, (const f4*)mean, (const f4*)invstd, psg, psgx, M, C4, gd.tc4, gd.ry, gd.rpc);
  else
    hipLaunchKernelGGL(bn_bwd_partial_kernel<false>, pgrid, dim3(kBnThreads), 0, s, (const f4*)g, (const f4*)nullptr,
                       (const f4*)x, (const f4*)mean, (const f4*)invstd, psg, psgx, M, C4, gd.tc4, gd.ry, gd.rpc);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, psg, psgx, dgamma, dbeta, C,
                     gd.chunks);
  const int64_t n4 = M * C4;
  const dim3 grid(grid_for(n4, 256));
  const float inv_m = 1.f / (float)M;
  if (gr)
    hipLaunchKernelGGL((bn_bwd_dx_kernel<true, true>), grid, dim3(256), 0, s, (const f4*)g, (const f4*)y, (const f4*)x,
                       (const f4*)mean, (const f4*)invstd, (const f4*)scale, (const f4*)dgamma, (const f4*)dbeta,
                       (f4*)dx, (f4*)gr, n4, C4, inv_m);
  else if (relu)
    hipLaunchKernelGGL((bn_bwd_dx_kernel<true, false>), grid, dim3(256), 0, s, (const f4*)g, (const f4*)y,
                       (const f4*)x, (const f4*)mean, (const f4*)invstd, (const f4*)scale, (const f4*)dgamma,
                       (const f4*)dbeta, (f4*)dx, (f4*)nullptr, n4, C4, inv_m);
  else
    hipLaunchKernelGGL((bn_bwd_dx_kernel<false, false>), grid, dim3(256), 0, s, (const f4*)g, (const f4*)nullptr,
                       (const f4*)x, (const f4*)mean, (const f4*)invstd, (const f4*)scale, (const f4*)dgamma,
                       (const f4*)dbeta, (f4*)dx, (f4*)nullptr, n4, C4, inv_m);
  SEA_RETURN_LAST();
}
