// M7b: the attention of M7 (csrc/attention.hip) on the 16-bit matrix cores by operand splitting (see csrc/gemm_split.hip).
// Two arithmetics, one kernel body per pass, templated on an operand policy:
//
//   Bf16Terms<3 | 2>  an fp32 number is the exact sum of three bf16 numbers; six v_mfma_f32_32x32x16_bf16 products accumulated
//       in fp32 give fp32-level accuracy, three products with two terms give 16 significant bits per operand.  No scaling:
//       bf16 has fp32's exponent range.
//   F16x2  22 significant bits per operand in THREE v_mfma_f32_32x32x16_f16 products per pair, where three bf16 terms need
//       six: hi = fp16(a s), mid = fp16(a s - hi) with a power-of-two scale s per operand GROUP that puts the group's largest
//       magnitude below 2^14; fp16's 5 exponent bits then leave 17 binades under that maximum at full 22-bit precision and an
//       absolute floor of 2^-38 of it below -- wide enough for scales that are BOUNDS rather than exact maxima:
//         * row fragments (the lane's own Q / K / V / dO row, the B operand of the first products): the row's exact maximum,
//           computed in the lane; the accumulator is multiplied back by the exact inverse;
//         * staged 64 x 64 tiles (K, V in forward and dQ; Q, dO in dK / dV): ONE scale per (image, head) from a pre-pass over
//           the four tensors (attn_amax_bh_kernel): a tile's rows are the CONTRACTION index of the transposed products, so
//           their scale must be uniform over everything an accumulator sums -- all tiles of the (image, head);
//         * the accumulator operands of the transposed products: P <= 1 takes 2^14; dS = P (dP - delta) scale takes the bound
//           2 x 64 max|dO| max|V| scale (|dP| and |delta| are both 64-term dot products of dO with V rows resp. their convex
//           combination), per query row in dQ (the lane's own max|dO_i|), per (image, head) in dK / dV.
//       Everything that exists only for these scales sits behind `if constexpr (P::kScaled)`.
//
// Same three kernels, same flash formulation, same "first product transposed" register trick and the same outputs as
// the fp32 kernels (reference semseg/models/backbones/vit_encoder.py:106-127); what changes is how a 64 x 64 tile is staged
// and multiplied.  The fp32 MFMA (v_mfma_f32_32x32x2_f32) needs 64 cycles per 2048 MACs; six 16-bit products of the same
// 32x32 block over K = 16 need 6 x 32 cycles per 16384 MACs: 2.7 x fewer matrix-core cycles with six products, 5.3 x fewer
// with three.
//
// Two tile images in LDS, per term (64 rows x 128 B each):
//   RM  [row][64 d]  (d contiguous)   A operand of   acc[row][lane] += sum_d  tile[row][d] * reg_of_lane[d]
//   TR  [d][64 rows] (rows contiguous) A operand of  out[d][lane]  += sum_row tile[row][d] * X[row][lane],  X = an
//       accumulator tile (rows on the registers): its registers 8u..8u+7 ARE the B fragment of k step u, with the k order
//       k(j, half) = 16u + 8 (j >> 2) + 4 half + (j & 3) (MI355X guide, "an accumulator tile as the next MFMA's operand"),
//       so the A fragment reads the same rows: two 8-byte pieces of the TR image.
// Swizzles (conflict-free for the lane groups of ds_read_b128 / ds_read_b64): RM 16-byte chunk ^ ((row >> 1) & 7),
// TR 8-byte slot ^ ((d >> 1) & 15).  The head dimension is walked as d = 32 half + 8 s + j (a lane's operands contiguous).
#include "attention_common.h"

namespace sea {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));  // a 16-byte MFMA fragment of either 16-bit format
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kImg = 64 * 128;  // bytes of one term image

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {  // low half = a
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ uint32_t pack_f16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}

// ---- operand policies: kTerms packed words per pair of floats, and the product chain of two split operands -------------------
template <int TERMS>
struct Bf16Terms {
  static constexpr int kTerms = TERMS;
  static constexpr bool kScaled = false;
  // w[t] = the pair's t-th residual term (low half = a)
  static __device__ __forceinline__ void split2(float a, float b, uint32_t (&w)[TERMS]) {
#pragma unroll
    for (int t = 0; t < TERMS; ++t) {
      w[t] = pack_bf16(a, b);
      if (t + 1 < TERMS) {
        a -= __uint_as_float(w[t] << 16);
        b -= __uint_as_float(w[t] & 0xffff0000u);
      }
    }
  }
  static __device__ __forceinline__ f32x16 products(const bf16x8 (&a)[TERMS], const bf16x8 (&b)[TERMS], f32x16 c) {
    if constexpr (TERMS == 3) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
    return c;
  }
};

struct F16x2 {
  static constexpr int kTerms = 2;
  static constexpr bool kScaled = true;
  // (a, b) already scaled -> w[0] = hi, w[1] = mid.  (Scalars, not a 2-vector of packed words: hipcc 7.2 folds
  // bit_cast<f16x2>(v[1]) of a uint2 to v[0]'s halves.)
  static __device__ __forceinline__ void split2(float a, float b, uint32_t (&w)[2]) {
    w[0] = pack_f16(a, b);
    const f32x2 f = __builtin_convertvector(__builtin_bit_cast(f16x2, w[0]), f32x2);
    w[1] = pack_f16(a - f[0], b - f[1]);
  }
  static __device__ __forceinline__ f32x16 products(const bf16x8 (&a)[2], const bf16x8 (&b)[2], f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[1]), __builtin_bit_cast(f16x8, b[0]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[1]), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[0]), __builtin_bit_cast(f16x8, b[0]), c, 0, 0, 0);
    return c;
  }
};

// power-of-two scale for a group whose largest |value| has the float bits `amax_bits`: amax * scale in [2^13, 2^14)
__device__ __forceinline__ void attn_pow2_scale(uint32_t amax_bits, float& scale, float& inv) {
  int E = (int)((amax_bits >> 23) & 0xffu);
  E = E < 14 ? 14 : (E > 253 ? 253 : E);
  scale = __uint_as_float((uint32_t)(267 - E) << 23);
  inv = __uint_as_float((uint32_t)(E - 13) << 23);
}

// 8 floats -> kTerms fragments of 8 (element j of the fragment = v[j])
template <class P>
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&out)[P::kTerms]) {
  uint32_t w[4][P::kTerms];
#pragma unroll
  for (int i = 0; i < 4; ++i) P::split2(v[2 * i], v[2 * i + 1], w[i]);
#pragma unroll
  for (int t = 0; t < P::kTerms; ++t) out[t] = __builtin_bit_cast(bf16x8, u32x4{w[0][t], w[1][t], w[2][t], w[3][t]});
}

// registers of load_tile_regs (times the power of two `sc` when the policy scales) -> the term images (RM and / or TR) of the tile
template <class P, bool RM, bool TR>
__device__ __forceinline__ void stage_tile(char* __restrict__ rm, char* __restrict__ tr, const f32x4 (&r)[4], float sc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (int)threadIdx.x + 256 * i;
    const int row = e >> 4, d4 = e & 15;
    float x0 = r[i][0], x1 = r[i][1], x2 = r[i][2], x3 = r[i][3];
    if constexpr (P::kScaled) {
      x0 *= sc;
      x1 *= sc;
      x2 *= sc;
      x3 *= sc;
    }
    uint32_t w0[P::kTerms], w1[P::kTerms];
    P::split2(x0, x1, w0);
    P::split2(x2, x3, w1);
#pragma unroll
    for (int t = 0; t < P::kTerms; ++t) {
      const uint32_t p0 = w0[t], p1 = w1[t];
      if (RM) *reinterpret_cast<u32x2*>(rm + t * kImg + row * 128 + (((d4 >> 1) ^ ((row >> 1) & 7)) << 4) + (d4 & 1) * 8) = u32x2{p0, p1};
      if (TR) {
        // element c of the float4 is head-dim index d = 4 d4 + c: row d of the TR image, 2 bytes at tile row `row`
        const int d = 4 * d4;
        char* q = tr + t * kImg + (row & 3) * 2;
        const int slot = row >> 2;
        *reinterpret_cast<uint16_t*>(q + (d + 0) * 128 + ((slot ^ (((d + 0) >> 1) & 15)) << 3)) = (uint16_t)(p0 & 0xffffu);
        *reinterpret_cast<uint16_t*>(q + (d + 1) * 128 + ((slot ^ (((d + 1) >> 1) & 15)) << 3)) = (uint16_t)(p0 >> 16);
        *reinterpret_cast<uint16_t*>(q + (d + 2) * 128 + ((slot ^ (((d + 2) >> 1) & 15)) << 3)) = (uint16_t)(p1 & 0xffffu);
        *reinterpret_cast<uint16_t*>(q + (d + 3) * 128 + ((slot ^ (((d + 3) >> 1) & 15)) << 3)) = (uint16_t)(p1 >> 16);
      }
    }
  }
}

// a lane's 32 head-dim values (d = 32 half + i) times `mul`, as the B fragments of the four 16-deep k steps.  A scaling policy
// also multiplies by the ROW's own power of two (both halves of the row agree on it through one shuffle) and keeps the inverse
// of that scale and the row's max |value * mul|
template <class P>
struct RowFrag {
  bf16x8 f[4][P::kTerms];
  float inv, amax;  // set only when P::kScaled
};
template <class P>
__device__ __forceinline__ void load_row_frag(const float* __restrict__ base, int64_t row_stride, int row, int half, float mul,
                                              RowFrag<P>& out) {
  const float* p = base + (int64_t)row * row_stride + 32 * half;
  f32x4 a[8];
  uint32_t mb = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    a[s] = *reinterpret_cast<const f32x4*>(p + 4 * s);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[s][e] *= mul;
      if constexpr (P::kScaled) {
        const uint32_t b = __float_as_uint(a[s][e]) & 0x7fffffffu;
        mb = b > mb ? b : mb;
      }
    }
  }
  if constexpr (P::kScaled) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mb, 32, 64);
    mb = other > mb ? other : mb;
    float sc;
    attn_pow2_scale(mb, sc, out.inv);
    out.amax = __uint_as_float(mb);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[s][e] = a[s][e] * sc;
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float v[8] = {a[2 * s][0], a[2 * s][1], a[2 * s][2], a[2 * s][3], a[2 * s + 1][0], a[2 * s + 1][1], a[2 * s + 1][2], a[2 * s + 1][3]};
    split8<P>(v, out.f[s]);
  }
}

// acc[row r of sub-block rb][column = lane & 31] += sum_d tile[32 rb + r][d] * frag_of_lane_column[d]
template <class P>
__device__ __forceinline__ f32x16 rm_times_frag(const char* __restrict__ rm, int rb, int lane, const RowFrag<P>& q, f32x16 acc) {
  const int row = 32 * rb + (lane & 31), half = lane >> 5;
  const char* p = rm + row * 128;
  const int sw = (row >> 1) & 7;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    bf16x8 a[P::kTerms];
#pragma unroll
    for (int t = 0; t < P::kTerms; ++t) a[t] = *reinterpret_cast<const bf16x8*>(p + t * kImg + (((4 * half + s) ^ sw) << 4));
    acc = P::products(a, q.f[s], acc);
  }
  return acc;
}

// out_dt[d = 32 dt + (lane & 31)][column] += sum_{r in sub-block rb} tile[32 rb + r][d] * X[r][column], dt = 0, 1; a scaling
// policy multiplies X by `bsc` (a power of two) before the split
template <class P>
__device__ __forceinline__ void tr_times_acc(const char* __restrict__ tr, int rb, int lane, const f32x16& x, float bsc, f32x16& o0,
                                             f32x16& o1) {
  const int half = lane >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (P::kScaled)
        v[j] = x[8 * u + j] * bsc;
      else
        v[j] = x[8 * u + j];
    }
    bf16x8 b[P::kTerms];
    split8<P>(v, b);
    const int slot = 8 * rb + 4 * u + half;  // rows 32 rb + 16 u + 4 half .. +3; the second piece is 8 rows further (slot + 2)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int d = 32 * dt + (lane & 31);
      const char* p = tr + d * 128;
      const int sw = (d >> 1) & 15;
      bf16x8 a[P::kTerms];
#pragma unroll
      for (int t = 0; t < P::kTerms; ++t) {
        const u32x2 lo = *reinterpret_cast<const u32x2*>(p + t * kImg + ((slot ^ sw) << 3));
        const u32x2 hi = *reinterpret_cast<const u32x2*>(p + t * kImg + (((slot + 2) ^ sw) << 3));
        a[t] = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
      }
      if (dt == 0)
        o0 = P::products(a, b, o0);
      else
        o1 = P::products(a, b, o1);
    }
  }
}

// float bits of max |q|, |k|, |v|, |dO| over the T rows of every (image, head): out[(b H + h) 4 + {0, 1, 2, 3}].
// grid (H, B, Z): block z takes rows [z T / Z, (z + 1) T / Z) and merges its maxima with atomicMax (float bits of
// non-negative values order like unsigned integers), so `out` is zeroed by attn_zero_words_kernel first.  (Round 5's first
// version ran ONE block per (image, head): 48 blocks on 256 CUs, 35 us per launch, 28 launches per Segmenter step = 7 % of it.)
__global__ void attn_zero_words_kernel(uint32_t* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0u;
}

template <int NT>   // 3: q, k, v (forward); 4: + dO
__global__ __launch_bounds__(256) void attn_amax_bh_kernel(AttnPtrs p, int T, int H, const float* __restrict__ go,
                                                           uint32_t* __restrict__ out) {
  const int b = blockIdx.y, h = blockIdx.x;
  const int r0 = (int)((int64_t)T * blockIdx.z / gridDim.z), r1 = (int)((int64_t)T * (blockIdx.z + 1) / gridDim.z);
  const float* src[4] = {p.q + (int64_t)b * p.sb + (int64_t)h * p.sh, p.k + (int64_t)b * p.sb + (int64_t)h * p.sh,
                         p.v + (int64_t)b * p.sb + (int64_t)h * p.sh,
                         NT == 4 ? go + ((int64_t)b * T) * (H * kD) + h * kD : nullptr};
  const int64_t stride[4] = {p.st, p.st, p.st, (int64_t)H * kD};
  uint32_t m[4] = {0, 0, 0, 0};
  const int d4 = threadIdx.x & 15;
  for (int row = r0 + (threadIdx.x >> 4); row < r1; row += 16) {
#pragma unroll
    for (int w = 0; w < NT; ++w) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src[w] + (int64_t)row * stride[w] + 4 * d4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t bits = __float_as_uint(v[e]) & 0x7fffffffu;
        m[w] = bits > m[w] ? bits : m[w];
      }
    }
  }
  __shared__ uint32_t part[4][4];
#pragma unroll
  for (int w = 0; w < NT; ++w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)m[w], o, 64);
      m[w] = other > m[w] ? other : m[w];
    }
    if ((threadIdx.x & 63) == 0) part[w][threadIdx.x >> 6] = m[w];
  }
  __syncthreads();
  if (threadIdx.x < NT) {
    const int w = threadIdx.x;
    uint32_t r = part[w][0];
    for (int i = 1; i < 4; ++i) r = part[w][i] > r ? part[w][i] : r;
    atomicMax(out + ((int64_t)b * H + h) * 4 + w, r);
  }
}

static inline void attn_amax_launch(const AttnPtrs& p, int B, int H, int T, const float* grad_out, uint32_t* amax_ws,
                                    hipStream_t stream) {
  const int words = 4 * B * H;
  int Z = (T + 63) / 64;                 // >= 64 rows per block
  Z = Z < 1 ? 1 : (Z > 16 ? 16 : Z);
  hipLaunchKernelGGL(attn_zero_words_kernel, dim3((words + 255) / 256), dim3(256), 0, stream, amax_ws, words);
  if (grad_out)
    hipLaunchKernelGGL(attn_amax_bh_kernel<4>, dim3(H, B, Z), dim3(256), 0, stream, p, T, H, grad_out, amax_ws);
  else
    hipLaunchKernelGGL(attn_amax_bh_kernel<3>, dim3(H, B, Z), dim3(256), 0, stream, p, T, H, grad_out, amax_ws);
}

// ---- forward: wave = 32 query rows, loop over 64-key tiles: S^T = K Q^T, online soft-max, O^T += V^T P^T ----------------
// (amax_bh, in all three kernels: the words of attn_amax_bh_kernel; only a scaling policy reads them)
template <class P>
__global__ __launch_bounds__(256, 2) void attn_fwd_split_kernel(AttnPtrs p, int T, int H, float scale,
                                                                const uint32_t* __restrict__ amax_bh, float* __restrict__ out,
                                                                float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) char k_rm[P::kTerms * kImg];
  __shared__ __attribute__((aligned(16))) char v_tr[P::kTerms * kImg];
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int q_row = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const bool q_ok = q_row < T;
  const bool wave_rows = blockIdx.x * 128 + wave * 32 < T;
  const float* qb = p.q + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* kb = p.k + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* vb = p.v + (int64_t)b * p.sb + (int64_t)h * p.sh;

  RowFrag<P> qf;  // Q[q_row][.] * scale * log2(e): scores come out in the log2 domain
  load_row_frag<P>(qb, p.st, q_ok ? q_row : T - 1, half, scale * kLog2e, qf);
  float sK = 1.f, sV = 1.f, invV = 1.f, c_s = 1.f;
  const float s_p = 16384.f;                                           // P = exp2(s - max) <= 1
  if constexpr (P::kScaled) {
    const uint32_t* aw = amax_bh + ((int64_t)b * H + h) * 4;
    float invK;
    attn_pow2_scale(aw[1], sK, invK);
    attn_pow2_scale(aw[2], sV, invV);
    c_s = invK * qf.inv;
  }
  f32x16 o0 = zero16(), o1 = zero16();
  float m_run = -INFINITY, l_run = 0.f;
  const int n_tiles = (T + kTile - 1) / kTile;
  f32x4 kr[4], vr[4];
  load_tile_regs(kb, p.st, 0, T, kr);
  load_tile_regs(vb, p.st, 0, T, vr);
  for (int j = 0; j < n_tiles; ++j) {
    __syncthreads();
    stage_tile<P, true, false>(k_rm, nullptr, kr, sK);
    stage_tile<P, false, true>(nullptr, v_tr, vr, sV);
    __syncthreads();
    if (j + 1 < n_tiles) {
      load_tile_regs(kb, p.st, (j + 1) * kTile, T, kr);
      load_tile_regs(vb, p.st, (j + 1) * kTile, T, vr);
    }
    if (!wave_rows) continue;
    f32x16 s0 = rm_times_frag<P>(k_rm, 0, lane, qf, zero16());
    f32x16 s1 = rm_times_frag<P>(k_rm, 1, lane, qf, zero16());
    const int key0 = j * kTile;
    if constexpr (P::kScaled) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        s0[t] *= c_s;
        s1[t] *= c_s;
      }
    }
    if (key0 + kTile > T) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        if (key0 + acc_row(t, half) >= T) s0[t] = -INFINITY;
        if (key0 + 32 + acc_row(t, half) >= T) s1[t] = -INFINITY;
      }
    }
    float m_t = s0[0];
#pragma unroll
    for (int t = 1; t < 16; ++t) m_t = fmaxf(m_t, s0[t]);
#pragma unroll
    for (int t = 0; t < 16; ++t) m_t = fmaxf(m_t, s1[t]);
    m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
    const float m_new = fmaxf(m_run, m_t);
    const float alpha = fast_exp2(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      s0[t] = fast_exp2(s0[t] - m_new);
      s1[t] = fast_exp2(s1[t] - m_new);
      psum += s0[t] + s1[t];
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      o0[t] *= alpha;
      o1[t] *= alpha;
    }
    tr_times_acc<P>(v_tr, 0, lane, s0, s_p, o0, o1);
    tr_times_acc<P>(v_tr, 1, lane, s1, s_p, o0, o1);
  }
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  float o_mul = 1.f / l_tot;
  if constexpr (P::kScaled) o_mul = invV * (1.f / 16384.f) / l_tot;
  store_rows_t(out + ((int64_t)b * T) * (H * kD) + h * kD, (int64_t)H * kD, q_row, q_ok, lane, o0, o1, o_mul);
  if (q_ok && half == 0) lse[((int64_t)b * H + h) * T + q_row] = (m_run + log2f(l_tot)) * kLn2;
}

// ---- dQ: wave = 32 query rows, loop over 64-key tiles: S^T, dP^T = V dO^T, dS^T, dQ^T += K^T dS^T -------------------------
template <class P>
__global__ __launch_bounds__(256, 2) void attn_dq_split_kernel(AttnPtrs p, int T, int H, float scale, const float* __restrict__ go,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               const uint32_t* __restrict__ amax_bh, float* __restrict__ dq,
                                                               int64_t gsb, int64_t gsh, int64_t gst) {
  extern __shared__ __attribute__((aligned(16))) char smem_dq[];
  char* k_rm = smem_dq;
  char* k_tr = k_rm + P::kTerms * kImg;
  char* v_rm = k_tr + P::kTerms * kImg;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int q_row = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const bool q_ok = q_row < T;
  const int q_ld = q_ok ? q_row : T - 1;
  const float* qb = p.q + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* kb = p.k + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* vb = p.v + (int64_t)b * p.sb + (int64_t)h * p.sh;
  RowFrag<P> qf, gf;
  load_row_frag<P>(qb, p.st, q_ld, half, scale * kLog2e, qf);
  load_row_frag<P>(go + ((int64_t)b * T) * (H * kD) + h * kD, (int64_t)H * kD, q_ld, half, 1.f, gf);
  float sK = 1.f, sV = 1.f, c_s = 1.f, c_dp = 1.f, s_ds = 1.f, dq_mul = 1.f;
  if constexpr (P::kScaled) {
    const uint32_t* aw = amax_bh + ((int64_t)b * H + h) * 4;
    float invK, invV, inv_ds;
    attn_pow2_scale(aw[1], sK, invK);
    attn_pow2_scale(aw[2], sV, invV);
    // |dS| <= (|dP| + |delta|) scale <= 2 x 64 max|dO_i| max|V| scale
    attn_pow2_scale(__float_as_uint(128.f * gf.amax * __uint_as_float(aw[2]) * scale), s_ds, inv_ds);
    c_s = invK * qf.inv, c_dp = invV * gf.inv;
    dq_mul = invK * inv_ds;
  }
  const float lse2 = lse[((int64_t)b * H + h) * T + q_ld] * kLog2e;
  const float dlt = delta[((int64_t)b * H + h) * T + q_ld];
  f32x16 dq0 = zero16(), dq1 = zero16();
  const int n_tiles = (T + kTile - 1) / kTile;
  f32x4 kr[4], vr[4];
  load_tile_regs(kb, p.st, 0, T, kr);
  load_tile_regs(vb, p.st, 0, T, vr);
  for (int j = 0; j < n_tiles; ++j) {
    __syncthreads();
    stage_tile<P, true, true>(k_rm, k_tr, kr, sK);
    stage_tile<P, true, false>(v_rm, nullptr, vr, sV);
    __syncthreads();
    if (j + 1 < n_tiles) {
      load_tile_regs(kb, p.st, (j + 1) * kTile, T, kr);
      load_tile_regs(vb, p.st, (j + 1) * kTile, T, vr);
    }
    if (blockIdx.x * 128 + wave * 32 >= T) continue;
    const int key0 = j * kTile;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      f32x16 s = rm_times_frag<P>(k_rm, rb, lane, qf, zero16());    // S^T (log2 domain); scaled: S^T sK sq
      f32x16 dp = rm_times_frag<P>(v_rm, rb, lane, gf, zero16());   // dP^T = V dO^T;      scaled: dP^T sV sg
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const bool exists = key0 + 32 * rb + acc_row(t, half) < T;
        if constexpr (P::kScaled) {
          const float pr = exists ? fast_exp2(s[t] * c_s - lse2) : 0.f;
          s[t] = pr * (dp[t] * c_dp - dlt) * scale;                   // dS^T
        } else {
          const float pr = exists ? fast_exp2(s[t] - lse2) : 0.f;
          s[t] = pr * (dp[t] - dlt) * scale;                          // dS^T
        }
      }
      tr_times_acc<P>(k_tr, rb, lane, s, s_ds, dq0, dq1);            // dQ^T += K^T dS^T;   scaled: dQ^T sK s_ds
    }
  }
  store_rows_t(dq + (int64_t)b * gsb + (int64_t)h * gsh, gst, q_row, q_ok, lane, dq0, dq1, dq_mul);
}

// ---- dK, dV: wave = 32 KEY rows, loop over 64-query tiles: S, dP = dO V^T, dS, dV^T += dO^T P, dK^T += Q^T dS -------------
template <class P>
__global__ __launch_bounds__(256, P::kTerms == 2 ? 2 : 1) void attn_dkv_split_kernel(
    AttnPtrs p, int T, int H, float scale, const float* __restrict__ go, const float* __restrict__ lse,
    const float* __restrict__ delta, const uint32_t* __restrict__ amax_bh, float* __restrict__ dk, float* __restrict__ dv,
    int64_t gsb, int64_t gsh, int64_t gst) {
  extern __shared__ __attribute__((aligned(16))) char smem_dkv[];
  char* q_rm = smem_dkv;
  char* q_tr = q_rm + P::kTerms * kImg;
  char* g_rm = q_tr + P::kTerms * kImg;
  char* g_tr = g_rm + P::kTerms * kImg;
  float* lse_s = reinterpret_cast<float*>(g_tr + P::kTerms * kImg);
  float* dlt_s = lse_s + kTile;
  const int b = blockIdx.z, h = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int k_row = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const bool k_ok = k_row < T;
  const int k_ld = k_ok ? k_row : T - 1;
  const float* qb = p.q + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* kb = p.k + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* vb = p.v + (int64_t)b * p.sb + (int64_t)h * p.sh;
  const float* gb = go + ((int64_t)b * T) * (H * kD) + h * kD;
  const int64_t gst_o = (int64_t)H * kD;
  RowFrag<P> kf, vf;
  load_row_frag<P>(kb, p.st, k_ld, half, scale * kLog2e, kf);   // S = Q K^T in the log2 domain
  load_row_frag<P>(vb, p.st, k_ld, half, 1.f, vf);
  float sQ = 1.f, sG = 1.f, c_s = 1.f, c_dp = 1.f, s_ds = 1.f, dk_mul = 1.f, dv_mul = 1.f;
  const float s_p = 16384.f, inv_p = 1.f / 16384.f;                   // P <= 1
  if constexpr (P::kScaled) {
    const uint32_t* aw = amax_bh + ((int64_t)b * H + h) * 4;
    float invQ, invG, inv_ds;
    attn_pow2_scale(aw[0], sQ, invQ);
    attn_pow2_scale(aw[3], sG, invG);
    // |dS| <= 2 x 64 max|dO| max|V| scale over the (image, head): the delta of a query is not bounded by THIS key's V row
    attn_pow2_scale(__float_as_uint(128.f * __uint_as_float(aw[3]) * __uint_as_float(aw[2]) * scale), s_ds, inv_ds);
    c_s = invQ * kf.inv, c_dp = invG * vf.inv;
    dk_mul = invQ * inv_ds, dv_mul = invG * inv_p;
  }
  f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  const int n_tiles = (T + kTile - 1) / kTile;
  for (int j = 0; j < n_tiles; ++j) {
    // no register prefetch here: four accumulators, two row fragments and the soft-max tiles leave no room for 32
    // staging registers across the products (they would spill); the second resident block covers the load latency
    f32x4 qr[4], gr[4];
    load_tile_regs(qb, p.st, j * kTile, T, qr);
    load_tile_regs(gb, gst_o, j * kTile, T, gr);
    __syncthreads();
    stage_tile<P, true, true>(q_rm, q_tr, qr, sQ);
    stage_tile<P, true, true>(g_rm, g_tr, gr, sG);
    if (threadIdx.x < kTile) {
      const int qq = j * kTile + (int)threadIdx.x;
      const int ql = qq < T ? qq : T - 1;
      lse_s[threadIdx.x] = lse[((int64_t)b * H + h) * T + ql] * kLog2e;
      dlt_s[threadIdx.x] = delta[((int64_t)b * H + h) * T + ql];
    }
    __syncthreads();
    if (blockIdx.x * 128 + wave * 32 >= T) continue;
    const int q0 = j * kTile;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      f32x16 pr = rm_times_frag<P>(q_rm, rb, lane, kf, zero16());   // S[q on registers][key on the lane]; scaled: S sQ sk
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int ql = 32 * rb + acc_row(t, half);
        const bool exists = (q0 + ql < T) && k_ok;
        if constexpr (P::kScaled)
          pr[t] = exists ? fast_exp2(pr[t] * c_s - lse_s[ql]) : 0.f;    // P
        else
          pr[t] = exists ? fast_exp2(pr[t] - lse_s[ql]) : 0.f;          // P
      }
      tr_times_acc<P>(g_tr, rb, lane, pr, s_p, dv0, dv1);             // dV^T += dO^T P;  scaled: dV^T sG s_p
      f32x16 dp = rm_times_frag<P>(g_rm, rb, lane, vf, zero16());     // dP = dO V^T;     scaled: dP sG sv
#pragma unroll
      for (int t = 0; t < 16; ++t) {                                  // dS (in place)
        if constexpr (P::kScaled)
          pr[t] = pr[t] * (dp[t] * c_dp - dlt_s[32 * rb + acc_row(t, half)]) * scale;
        else
          pr[t] = pr[t] * (dp[t] - dlt_s[32 * rb + acc_row(t, half)]) * scale;
      }
      tr_times_acc<P>(q_tr, rb, lane, pr, s_ds, dk0, dk1);            // dK^T += Q^T dS;  scaled: dK^T sQ s_ds
    }
  }
  store_rows_t(dk + (int64_t)b * gsb + (int64_t)h * gsh, gst, k_row, k_ok, lane, dk0, dk1, dk_mul);
  store_rows_t(dv + (int64_t)b * gsb + (int64_t)h * gsh, gst, k_row, k_ok, lane, dv0, dv1, dv_mul);
}

// ---- launch: one place for the grid and the dynamic LDS of the three kernels ------------------------------------------------------
static inline dim3 attn_grid(int B, int H, int T) { return dim3((T + 127) / 128, H, B); }
constexpr size_t attn_lds_dq(int terms) { return (size_t)3 * terms * kImg; }                                 // K RM + TR, V RM
constexpr size_t attn_lds_dkv(int terms) { return (size_t)4 * terms * kImg + 2 * kTile * sizeof(float); }   // Q, dO RM + TR, lse, delta

// f(policy) for the arithmetic: 22 = fp16 x 2, 3 / 2 = bf16 terms
template <typename F>
static inline void with_policy(int arith, F&& f) {
  if (arith == 22)
    f(F16x2{});
  else if (arith == 3)
    f(Bf16Terms<3>{});
  else
    f(Bf16Terms<2>{});
}

template <class P>
static void attn_bwd_lds_opt_in() {
  (void)hipFuncSetAttribute((const void*)attn_dq_split_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds_dq(P::kTerms));
  (void)hipFuncSetAttribute((const void*)attn_dkv_split_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds_dkv(P::kTerms));
}

}  // namespace sea

using namespace sea;

int sea_attention_fwd_split(const AttnPtrs& p, int B, int H, int T, float scale, float* out, float* lse, int arith,
                            uint32_t* amax_ws, hipStream_t stream) {
  if (arith == 22) attn_amax_launch(p, B, H, T, nullptr, amax_ws, stream);
  with_policy(arith, [&](auto pol) {
    hipLaunchKernelGGL(attn_fwd_split_kernel<decltype(pol)>, attn_grid(B, H, T), dim3(256), 0, stream, p, T, H, scale, amax_ws, out, lse);
  });
  return (int)hipGetLastError();
}

int sea_attention_bwd_split(const AttnPtrs& p, int B, int H, int T, float scale, const float* grad_out, const float* lse,
                            const float* delta, float* dq, float* dk, float* dv, int64_t gsb, int64_t gsh, int64_t gst, int arith,
                            uint32_t* amax_ws, hipStream_t stream) {
  // up to 4 x 3 x 8 KB = 96 KB of dynamic LDS (dK / dV at three terms): opt in once per DEVICE (the attribute is per device; a
  // process that drives a second GPU would otherwise fail its first dkv launch there)
  static bool attr_set_dev[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!attr_set_dev[dev & 63]) {
    attn_bwd_lds_opt_in<F16x2>();
    attn_bwd_lds_opt_in<Bf16Terms<3>>();
    attn_bwd_lds_opt_in<Bf16Terms<2>>();
    attr_set_dev[dev & 63] = true;
  }
  if (arith == 22) attn_amax_launch(p, B, H, T, grad_out, amax_ws, stream);
  with_policy(arith, [&](auto pol) {
    using P = decltype(pol);
    hipLaunchKernelGGL(attn_dq_split_kernel<P>, attn_grid(B, H, T), dim3(256), attn_lds_dq(P::kTerms), stream, p, T, H, scale, grad_out,
                       lse, delta, amax_ws, dq, gsb, gsh, gst);
    hipLaunchKernelGGL(attn_dkv_split_kernel<P>, attn_grid(B, H, T), dim3(256), attn_lds_dkv(P::kTerms), stream, p, T, H, scale,
                       grad_out, lse, delta, amax_ws, dk, dv, gsb, gsh, gst);
  });
  return (int)hipGetLastError();
}
