// DQN gradient step on gfx950 (src/agents/dqn/dqn.py:403-451):
// double-DQN TD target + MSE / Huber gradient, MPNN weight gradients
// (split-K reductions over every node of the minibatch on bf16x3-split v_mfma_f32_32x32x16_bf16,
// per-wave partial slabs reduced in a fixed order -> bitwise reproducible), gradient-norm clipping, Adam, and the
// MPNN backward / gradient entries that end in the weight-gradient tail.  The replay rings are in eco_replay.hip.
#include <cmath>

#include "eco_mpnn.h"

namespace eco {

// ------------------------------------------------------------ weight grads ----
// dW[o][i] = sum_r dY[r][o] * X[r][i]  with X = [X1 (K1 cols) | X2 (K2 cols)]
struct WJob {
  const float* dY;   // [R][64]
  const float* X1;
  const float* X2;
  int ld1, K1, ld2, K2;
  int R;
  int nO;            // rows of dW (64, or 63 for the edge-embedding Wx)
  int out_off;       // flat offset of dW[0][0]
  int out_ld;        // row stride in the flat buffer
  int out_col0;      // first column in the flat buffer
};
constexpr int MAX_JOBS = 10;
#ifndef WGRAD_NT
#define WGRAD_NT 0  // A/B: nontemporal (streaming) loads of the dY / X rows
#endif
constexpr int WGRAD_WG_X = 3;  // workgroups per CU over all jobs (46 KB LDS each: 3 resident per CU)
constexpr int WG_PER_JOB = 128;
constexpr int SLABS_PER_JOB = WG_PER_JOB;  // one [64][128] partial per workgroup
constexpr int SLAB = 64 * 128;
constexpr int WROWS = 32;                  // rows per LDS tile

struct WJobs {
  WJob j[MAX_JOBS];
  int n;
  int nwgj[MAX_JOBS];     // wgrad_bf3_kernel / reduce: workgroups (= slabs) of job j, <= WG_PER_JOB
  int first[MAX_JOBS + 1];  // wgrad_bf3_kernel: first flat block of job j (1-D grid of first[n] blocks)
};


// Same reduction on 32x32x16 bf16 MFMAs: dY and X are split EXACTLY into three bf16 pieces while a
// 32-row tile is staged (split3_bits), and the six products above 2^-24 relative are accumulated in
// f32 (as mm_bf3_lean does for the forward Linears), so the sums keep f32 accuracy at ~2.7x the f32-MFMA
// rate.  Staging transposes through registers: thread t loads column (t & 63) of 8 consecutive rows
// (each wave-level load is one contiguous 256-B row segment), splits, and writes the three 8-row
// pieces as 16-B LDS stores into [p][column][row] planes, which are exactly the MFMA fragments
// (lane l: column l & 31, rows 8 (l >> 5) .. +7 of a 16-row k-step).
constexpr int WB_LD = 40;  // bf16 per plane column (32 rows + 8 pad: 80-B stride, conflict-light 16-B reads)
typedef short bf16x8w __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4w __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split8_store(uint16_t* base, int plane_stride, const float (&v)[8]) {
  u32x4w p1, p2, p3;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    uint16_t a0, b0, c0, a1, b1, c1;
    split3_bits(v[2 * t], a0, b0, c0);
    split3_bits(v[2 * t + 1], a1, b1, c1);
    p1[t] = a0 | (uint32_t)a1 << 16;
    p2[t] = b0 | (uint32_t)b1 << 16;
    p3[t] = c0 | (uint32_t)c1 << 16;
  }
  *reinterpret_cast<u32x4w*>(base) = p1;
  *reinterpret_cast<u32x4w*>(base + plane_stride) = p2;
  *reinterpret_cast<u32x4w*>(base + 2 * plane_stride) = p3;
}

// WIDE: X of up to 128 columns (two 64-column groups per thread); narrow jobs (K <= 64: Wf, W0, Wx, Wp) stage one
// group of 8 rows x 1 column per thread and issue half the X loads.
template <bool WIDE>
__device__ __forceinline__ void wgrad_bf3_job(const WJobs& jobs, float* slabs, int jb, uint16_t* sY, uint16_t* sX) {
  constexpr int PY = 64 * WB_LD, PX = 128 * WB_LD;  // plane strides (bf16)
  constexpr int XU = WIDE ? 2 : 1;                  // X row groups per thread
  const int wg = (int)blockIdx.x - jobs.first[jb], nwg = jobs.nwgj[jb];
  const WJob& J = jobs.j[jb];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int jj = lane & 31, h = lane >> 5;
  const int K = J.K1 + J.K2;
  const int ntile = 2 * ((K + 31) / 32);
  const int chunk = ((J.R + nwg - 1) / nwg + WROWS - 1) / WROWS * WROWS;
  const int r0 = wg * chunk;
  const int r1 = min(J.R, r0 + chunk);
  // staging roles: dY column yc of rows 8 yg .. +7; X columns xc (+ 0 / 1 x 128 units) of rows 8 xg .. +7
  const int yc = threadIdx.x & 63, yg = threadIdx.x >> 6;
  // X: WIDE: column t & 127 of row groups (t >> 7) + 2u, u < 2; narrow: column t & 63 of row group t >> 6
  const int xc = WIDE ? threadIdx.x & 127 : threadIdx.x & 63, xg0 = WIDE ? threadIdx.x >> 7 : threadIdx.x >> 6;
  constexpr int XG = WIDE ? 2 : 4;  // row-group step between a thread's X units
  typedef const __attribute__((address_space(1))) float gfloat;
  // loads are unconditional (rows clamped to r1 - 1, dead columns read column 0) and masked after:
  // predicated loads compiled to one branch + vmcnt(0) wait per row, serialising the whole tile
  const bool xlive = xc < K;
  gfloat* ysrc = (gfloat*)(J.dY + yc);
  const float* xsrc = !xlive ? J.X1 : (xc < J.K1 ? J.X1 + xc : J.X2 + (xc - J.K1));
  int xld = xlive && xc >= J.K1 ? J.ld2 : J.ld1;
  uint32_t xmask = xlive ? 0xFFFFFFFFu : 0u;
  // keep the per-lane source and mask opaque (otherwise the select is sunk into every load as a branch)
  asm volatile("" : "+v"(xsrc), "+v"(xld), "+v"(xmask));
  gfloat* xg = (gfloat*)xsrc;
  const int rlast = r1 - 1;
  f32x16 acc[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[q][k] = 0.f;
  // two register buffers: tiles i+1 and i+2 are in flight while tile i is split and multiplied
  // (one tile in flight held the reduction at ~4 TB/s: too few bytes outstanding per CU)
  struct Regs {
    float y[8], x[XU][8];
  };
  // raw loads only; the row / column masks are applied when the tile is stored (masking at load
  // time makes the compiler wait for every load before the multiply it should overlap)
  auto load_tile = [&](Regs& R, int rb) {
#if WGRAD_NT
#pragma unroll
    for (int k = 0; k < 8; ++k) R.y[k] = __builtin_nontemporal_load(&ysrc[(size_t)min(rb + 8 * yg + k, rlast) * 64]);
#pragma unroll
    for (int u = 0; u < XU; ++u)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        R.x[u][k] = __builtin_nontemporal_load(&xg[(size_t)min(rb + 8 * (xg0 + XG * u) + k, rlast) * (size_t)xld]);
#else
#pragma unroll
    for (int k = 0; k < 8; ++k) R.y[k] = ysrc[(size_t)min(rb + 8 * yg + k, rlast) * 64];
#pragma unroll
    for (int u = 0; u < XU; ++u)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        R.x[u][k] = xg[(size_t)min(rb + 8 * (xg0 + XG * u) + k, rlast) * (size_t)xld];
#endif
  };
  auto store_tile = [&](Regs& R, int rb) {
    asm volatile("" : "+s"(rb));  // keeps the masking (and this tile's wait) at the store
#pragma unroll
    for (int k = 0; k < 8; ++k) R.y[k] = rb + 8 * yg + k < r1 ? R.y[k] : 0.f;
    split8_store(sY + yc * WB_LD + 8 * yg, PY, R.y);
#pragma unroll
    for (int u = 0; u < XU; ++u) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        R.x[u][k] = rb + 8 * (xg0 + XG * u) + k < r1 ? __uint_as_float(__float_as_uint(R.x[u][k]) & xmask) : 0.f;
      split8_store(sX + xc * WB_LD + 8 * (xg0 + XG * u), PX, R.x[u]);
    }
  };
  // this wave's output tiles: t = w + 4q -> o-tile w & 1, i-tiles (w >> 1) and (w >> 1) + 2
  const int ot = w & 1;
  const bool live0 = w < ntile, live1 = w + 4 < ntile;
  const uint16_t* ya = sY + (32 * ot + jj) * WB_LD + 8 * h;
  const uint16_t* xb0 = sX + (32 * (w >> 1) + jj) * WB_LD + 8 * h;
  const uint16_t* xb1 = xb0 + 64 * WB_LD;
  auto compute = [&]() {
  if (live0) {
#pragma unroll
    for (int s = 0; s < WROWS / 16; ++s) {
      const bf16x8w a1 = *reinterpret_cast<const bf16x8w*>(ya + 16 * s);
      const bf16x8w a2 = *reinterpret_cast<const bf16x8w*>(ya + PY + 16 * s);
      const bf16x8w a3 = *reinterpret_cast<const bf16x8w*>(ya + 2 * PY + 16 * s);
      const bf16x8w b1 = *reinterpret_cast<const bf16x8w*>(xb0 + 16 * s);
      const bf16x8w b2 = *reinterpret_cast<const bf16x8w*>(xb0 + PX + 16 * s);
      const bf16x8w b3 = *reinterpret_cast<const bf16x8w*>(xb0 + 2 * PX + 16 * s);
      if (live1) {
        const bf16x8w c1 = *reinterpret_cast<const bf16x8w*>(xb1 + 16 * s);
        const bf16x8w c2 = *reinterpret_cast<const bf16x8w*>(xb1 + PX + 16 * s);
        const bf16x8w c3 = *reinterpret_cast<const bf16x8w*>(xb1 + 2 * PX + 16 * s);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, c1, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, c2, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, c3, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, c1, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, c2, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, c1, acc[1], 0, 0, 0);
      } else {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[0], 0, 0, 0);
      }
    }
  }
  };
  // loads are issued unconditionally (rows past r1 clamp to r1 - 1 and are masked at the store): a
  // conditional load makes the compiler drain every tile in flight at the join (vmcnt(0))
  if (r0 < r1) {
    Regs RA, RB;
    load_tile(RA, r0);
    load_tile(RB, r0 + WROWS);
    for (int rb = r0; rb < r1; rb += 2 * WROWS) {
      store_tile(RA, rb);
      __syncthreads();
      load_tile(RA, rb + 2 * WROWS);
      compute();
      __syncthreads();
      if (rb + WROWS >= r1) break;
      store_tile(RB, rb + WROWS);
      __syncthreads();
      load_tile(RB, rb + 3 * WROWS);
      compute();
      __syncthreads();
    }
  }
  float* slab = slabs + ((size_t)jb * SLABS_PER_JOB + wg) * SLAB;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int t = w + 4 * q;
    if (t < ntile) {
      const int it = t >> 1;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int o = 32 * ot + (k & 3) + 8 * (k >> 2) + 4 * h;  // 32x32 C/D layout
        slab[o * 128 + 32 * it + jj] = acc[q][k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_bf3_kernel(WJobs jobs, float* slabs) {
  __shared__ __attribute__((aligned(16))) uint16_t sY[3 * 64 * WB_LD];
  __shared__ __attribute__((aligned(16))) uint16_t sX[3 * 128 * WB_LD];
  int jb = 0;
  while (jb + 1 < jobs.n && (int)blockIdx.x >= jobs.first[jb + 1]) ++jb;
  if (jobs.j[jb].K1 + jobs.j[jb].K2 > 64) wgrad_bf3_job<true>(jobs, slabs, jb, sY, sX);
  else wgrad_bf3_job<false>(jobs, slabs, jb, sY, sX);
}


// fixed-order sum of the slabs of every job into the flat gradient
__global__ void wgrad_reduce_kernel(WJobs jobs, const float* slabs, float* grad) {
  const WJob& J = jobs.j[blockIdx.y];
  const int K = J.K1 + J.K2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int o = idx / 128, i = idx % 128;
  if (o >= J.nO || i >= K) return;
  const float* s = slabs + (size_t)blockIdx.y * SLABS_PER_JOB * SLAB + o * 128 + i;
  float acc = 0.f;
  const int nk = jobs.nwgj[blockIdx.y];
  int k = 0;
  for (; k + 8 <= nk; k += 8) {  // eight slab loads in flight, summed in slab order (same result as one by one)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(k + u) * SLAB];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; k < nk; ++k) acc += s[(size_t)k * SLAB];
  grad[J.out_off + o * J.out_ld + J.out_col0 + i] = acc;
}

// the readout / edge-weight column sums of one backward in ONE launch: one workgroup per output column, blocks
// dealt to the four jobs in order; a fixed-order sum per column (256 strided partials, then a tree)
struct ColJob {
  const float* X;
  int R, ld, C;
  float* out;
  int out_stride;
};
struct ColJobs {
  ColJob j[4];
  int first[5];
};
__global__ void colsum_jobs_kernel(ColJobs jobs) {
  int jb = 0;
  while (jb < 3 && (int)blockIdx.x >= jobs.first[jb + 1]) ++jb;
  const ColJob& J = jobs.j[jb];
  __shared__ float red[256];
  const int c = (int)blockIdx.x - jobs.first[jb];
  float acc = 0.f;
  for (int r = threadIdx.x; r < J.R; r += 256) acc += J.X[(size_t)r * J.ld + c];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) red[threadIdx.x] += red[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) J.out[(size_t)c * J.out_stride] = red[0];
}

// ---------------------------------------------------------------------- TD ----
// dqn.py:403-440 for a reversible env: q_t = target(s')[argmax online(s')] (double DQN),
// td = r + (1 - done) * gamma * q_t, loss = mean((q(s,a) - td)^2), dq = dloss/dq.
// One thread per element of dq[B][N]: the element of the taken action gets the TD gradient (and its row's
// squared error), every other element zero -- the zero-fill of loss.backward()'s dQ and the TD step in one pass.
// HUBER: smooth_l1_loss(beta = 1) instead of mse_loss (dqn.py:172): per-sample loss 0.5 d^2 for |d| < 1, else
// |d| - 0.5; gradient d / B clamped to +-1 / B.  The comparisons are torch's own (x < -beta, x > beta, else
// x), so a NaN d stays NaN in dq and in the loss.
// PRIO (eco_dqn_td_weighted, prioritised replay): the per-sample loss and the gradient are multiplied by the
// importance weight is_w[b] (nullable: 1) -- the gradient as (w * g) / B, one rounding after an exact product when
// w and g are short -- and abs_td[b] (nullable) receives |q(s,a) - td| whatever the loss kind.  PRIO = false is
// the kernel as it was: eco_dqn_td_loss and a weighted call without weights and abs_td launch that instantiation.
template <bool HUBER, bool PRIO>
__global__ void td_kernel(const float* q_s, const float* q_tn, const int32_t* a_star, const int32_t* actions,
                          const float* rewards, const float* dones, int B, int N, float gamma, int clip,
                          float* dq, float* sqerr, const float* is_w, float* abs_td) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * N) return;
  const int b = (int)(i / N), j = (int)(i - (size_t)b * N);
  int a = actions[b];
  if ((unsigned)a >= (unsigned)N) a = 0;
  if (j != a) {
    dq[i] = 0.f;
    return;
  }
  int as = a_star[b];
  if ((unsigned)as >= (unsigned)N) as = 0;  // never index outside the row (all-masked argmax is 0)
  float qt = q_tn[(size_t)b * N + as];
  if (clip && qt < 0.f) qt = 0.f;  // clip_Q_targets (dqn.py:431-432)
  const float td = rewards[b] + (1.f - dones[b]) * gamma * qt;
  const float q = q_s[i];
  const float diff = q - td;
  if (PRIO) {
    const float w = is_w ? is_w[b] : 1.f;
    const float ad = fabsf(diff);
    if (abs_td) abs_td[b] = ad;
    if (HUBER) {
      dq[i] = w * (diff < -1.f ? -1.f : diff > 1.f ? 1.f : diff) / (float)B;
      sqerr[b] = w * (ad < 1.f ? 0.5f * diff * diff : ad - 0.5f);
    } else {
      dq[i] = w * (2.f * diff) / (float)B;
      sqerr[b] = w * (diff * diff);
    }
    return;
  }
  if (HUBER) {
    const float ad = fabsf(diff);
    dq[i] = (diff < -1.f ? -1.f : diff > 1.f ? 1.f : diff) / (float)B;  // smooth_l1_loss(reduction='mean') backward
    sqerr[b] = ad < 1.f ? 0.5f * diff * diff : ad - 0.5f;
  } else {
    dq[i] = 2.f * diff / (float)B;  // mse_loss(reduction='mean') backward
    sqerr[b] = diff * diff;
  }
}

__global__ void mean_kernel(const float* v, int n, float* out) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0] / (float)n;
}

// -------------------------------------------------------------------- Adam ----
// torch.optim.Adam (amsgrad=False): m.lerp_(g, 1-b1); v = b2 v + (1-b2) g^2;
// p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)      (dqn.py:212, :443-449)
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, int n, float b1, float b2, float step_size,
                            float bc2_sqrt, float eps, float wd, float gscale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gi = gscale == 1.f ? g[i] : g[i] * gscale;
  if (wd != 0.f) gi = fmaf(wd, p[i], gi);
  const float mi = m[i] + (1.f - b1) * (gi - m[i]);
  const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = p[i] - step_size * (mi / denom);
}

// --------------------------------------------------------------- grad clip ----
// torch.nn.utils.clip_grad_norm_(parameters, max_norm), norm type 2, over the flat gradient (dqn.py:446-447).
// Three launches, no atomics and no host read: (1) each workgroup sums g^2 over its chunks of GC_CHUNK elements
// in float64 (per thread in index order, then the wave butterfly, then the four waves in order) into its slot of
// the library's partial buffer; (2) one workgroup sums the partials the same way and writes {total_norm, coef};
// (3) grad *= coef.  The grid depends on n alone, so the result is bitwise reproducible run to run.
constexpr int GC_CHUNK = 2048;       // elements per workgroup pass: 8 per thread
constexpr int GC_MAX_BLOCKS = 1024;  // partial slots; above GC_CHUNK * GC_MAX_BLOCKS elements workgroups take more chunks
__device__ double g_clip_partial[GC_MAX_BLOCKS];

// fixed-order sum over the 256 threads of a workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* g, int n) {
  __shared__ double red[4];
  const long long nchunk = ((long long)n + GC_CHUNK - 1) / GC_CHUNK;
  double acc = 0.0;
  for (long long c = blockIdx.x; c < nchunk; c += gridDim.x) {
#pragma unroll
    for (int k = 0; k < GC_CHUNK / 256; ++k) {
      const long long i = c * GC_CHUNK + k * 256 + threadIdx.x;
      const double v = i < n ? (double)g[i] : 0.0;
      acc += v * v;
    }
  }
  const double s = block_sum_d(acc, red);
  if (threadIdx.x == 0) g_clip_partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_norm_kernel(int nblk, double grad_scale, double max_norm, float* norm_out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) acc += g_clip_partial[k];
  const double s = block_sum_d(acc, red);
  if (threadIdx.x == 0) {
    const double total = grad_scale * sqrt(s);
    const double c = max_norm / (total + 1e-6);
    norm_out[0] = (float)total;
    norm_out[1] = (float)(c > 1.0 ? 1.0 : c);  // clamp(max = 1); a NaN norm stays NaN
  }
}

__global__ void grad_scale_kernel(float* g, int n, const float* norm_out) {
  const float coef = norm_out[1];
  if (coef == 1.f) return;  // x * 1.0f is x: nothing to write
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)n) g[i] *= coef;
}

static size_t slab_bytes() { return (size_t)MAX_JOBS * SLABS_PER_JOB * SLAB * sizeof(float); }

}  // namespace eco

using namespace eco;

extern "C" size_t eco_mpnn_backward_workspace_bytes(int32_t n_spins, int32_t batch) {
  const size_t g = mpnn_grad_ws_bytes(n_spins, batch);
  if (!g) return 0;
  return align_up(g, 256) + slab_bytes();
}

// The weight-gradient tail shared by eco_mpnn_backward and grad_rows: dW = sum_nodes dY^T X for every Linear
// from the saved activations `sv` and the activation gradients `gr` (both [tensor][R][64] then per graph, R = batch * N
// rows), split-K into `slabs` and reduced in a fixed order into grad; then the column sums of the per-graph /
// per-block partials (nblk rows of DWA).
static int wgrad_tail(const float* sv, const float* gr, int32_t n_obs_in, int N, int32_t batch, int nblk,
                      const float* obs_x, float* slabs, float* grad, hipStream_t st) {
  const size_t RT = (size_t)batch * N;
  auto SV = [&](int t) { return sv + (size_t)t * RT * 64; };
  auto GR = [&](int t) { return gr + (size_t)t * RT * 64; };
  const float* MEAN = sv + (size_t)SV_NODE_TENSORS * RT * 64;
  const float* DP = gr + (size_t)GR_NODE_TENSORS * RT * 64;
  const float* DWRA = DP + (size_t)batch * 64;
  const float* DWRB = DWRA + (size_t)batch * 64;
  const float* DBR = DWRB + (size_t)batch * 64;
  const float* DWA = DBR + (((size_t)batch + 63) & ~63ull);
  const FlatOffsets fo = flat_offsets(n_obs_in);
  WJobs J{};
  int n = 0;
  const int R = (int)RT;
  for (int l = 0; l < 3; ++l) {
    J.j[n++] = WJob{GR(GR_DUM0 + l), SV(SV_AGG0 + l), SV(SV_E), 64, 64, 64, 64, R, 64, fo.L + l * 16384, 128, 0};
    J.j[n++] = WJob{GR(GR_DUU0 + l), SV(SV_H0 + l), SV(SV_M0 + l), 64, 64, 64, 64, R, 64, fo.L + l * 16384 + 8192,
                    128, 0};
  }
  J.j[n++] = WJob{GR(GR_DUE), SV(SV_EAGG), nullptr, 64, 64, 0, 0, R, 64, fo.Wf, 64, 0};
  const int xw = ECO_OBS_X_STRIDE(n_obs_in);
  J.j[n++] = WJob{GR(GR_DU0), obs_x, nullptr, xw, n_obs_in, 0, 0, R, 64, fo.W0, n_obs_in, 0};
  J.j[n++] = WJob{GR(GR_DZ), obs_x, nullptr, xw, n_obs_in, 0, 0, R, 63, fo.We, 1 + n_obs_in, 1};
  J.j[n++] = WJob{DP, MEAN, nullptr, 64, 64, 0, 0, batch, 64, fo.Wp, 64, 0};
  J.n = n;
  {
    // one resident wave of workgroups over the 256 CUs (46 KB LDS: 3 per CU for bf16x3; 27 KB and 168 VGPRs:
    // 3 per CU for fp16x2).  Measured splits (M = 2048 ER-200): in proportion to the bytes each job reads,
    // 1.28 vs 1.05 ms per gradient step of backward + weight gradients against an even split; more workgroups
    // for the K = 128 jobs at the others' expense (96 / 112 each) slower again (9.25 / 12.1 vs 8.66 ms
    // per vector step): the K <= 64 jobs cost as much per row.  The fp16x2 variant (round 3)
    // measured 0.62 vs 0.52 ms per launch: its per-fragment scales and splits sit after the barrier, on the
    // critical path.
    const int total = WGRAD_WG_X * 256;
    double rows = 0.0;
    for (int j = 0; j < n; ++j) rows += J.j[j].R;
    J.first[0] = 0;
    for (int j = 0; j < n; ++j) {
      // in proportion to the job's rows (a row costs about the same in every job); the per-graph readout job
      // (R = batch) gets one
      const int g = (int)(total * (double)J.j[j].R / rows);
      J.nwgj[j] = std::max(1, std::min(WG_PER_JOB, g));
      J.first[j + 1] = J.first[j] + J.nwgj[j];
    }
    wgrad_bf3_kernel<<<J.first[n], 256, 0, st>>>(J, slabs);
  }
  wgrad_reduce_kernel<<<dim3(64 * 128 / 256, n), 256, 0, st>>>(J, slabs, grad);
  ColJobs CJ{};
  CJ.j[0] = ColJob{DWRA, batch, 64, 64, grad + fo.Wr, 1};
  CJ.j[1] = ColJob{DWRB, batch, 64, 64, grad + fo.Wr + 64, 1};
  CJ.j[2] = ColJob{DBR, batch, 1, 1, grad + fo.Br, 1};
  CJ.j[3] = ColJob{DWA, nblk, 64, 63, grad + fo.We, 1 + n_obs_in};
  CJ.first[0] = 0;
  for (int k = 0; k < 4; ++k) CJ.first[k + 1] = CJ.first[k] + CJ.j[k].C;
  colsum_jobs_kernel<<<CJ.first[4], 256, 0, st>>>(CJ);
  return check_launch("mpnn_backward_wgrad");
}

extern "C" int eco_mpnn_backward(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                                 const int32_t* graph_ids, int32_t batch, const float* obs_x, const void* saved,
                                 const float* dq, float* grad, void* workspace, eco_stream_t stream) {
  if (!grad || !workspace) return fail(ECO_ERR_ARG, "null grad/workspace");
  hipStream_t st = (hipStream_t)stream;
  int rc = mpnn_backward_launch(packed, n_obs_in, gs, graph_ids, batch, obs_x, saved, dq, workspace, st);
  if (rc) return rc;
  const int N = gs->n_spins;
  if ((size_t)batch * N > (size_t)INT32_MAX / 64) return fail(ECO_ERR_ARG, "batch * n_spins too large");
  const int gpb = graphs_per_block(N, batch);
  float* slabs = (float*)((char*)workspace + align_up(mpnn_grad_ws_bytes(N, batch), 256));
  return wgrad_tail((const float*)saved, (const float*)workspace, n_obs_in, N, batch, (batch + gpb - 1) / gpb, obs_x,
                    slabs, grad, st);
}

// eco_mpnn_grad_large and eco_mpnn_grad_wg: the gradient on global-memory rows of the range r (RowsRange, eco_mpnn.h).
// Everything is checked before the first launch; then the call's max degree, the saving forward and the backward
// (mpnn_grad_rows_launch), then the weight-gradient tail, one DWA row per episode.
static int grad_rows(const RowsRange& r, const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                     const int32_t* graph_ids, int32_t batch, const float* obs_x, const float* dq, float* grad,
                     void* workspace, eco_stream_t stream) {
  if (!packed || !gs || !graph_ids || !obs_x || !dq || !grad || !workspace)
    return fail(ECO_ERR_ARG, rows_message(r, "grad", "null argument"));
  if (const int rc = mpnn_rows_check(r, "grad", gs, n_obs_in, batch)) return rc;
  const int N = gs->n_spins;
  const GradRowsLayout L = mpnn_grad_rows_layout(r, N, batch, slab_bytes());
  if (!L.total)
    return fail(ECO_ERR_ARG, rows_message(r, "grad", "batch * n_spins beyond the 32-bit row index ((2^31 - 1) / 64)"));
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = mpnn_grad_rows_launch(r, packed, n_obs_in, gs, graph_ids, batch, obs_x, dq, workspace, L, st))
    return rc;
  char* ws = (char*)workspace;
  return wgrad_tail((const float*)(ws + L.sv), (const float*)(ws + L.gr), n_obs_in, N, batch, batch, obs_x,
                    (float*)(ws + L.slabs), grad, st);
}

extern "C" size_t eco_mpnn_grad_large_workspace_bytes(int32_t n_spins, int32_t batch) {
  return mpnn_grad_rows_layout(kRowsLarge, n_spins, batch, slab_bytes()).total;
}

extern "C" int eco_mpnn_grad_large(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                                   const int32_t* graph_ids, int32_t batch, const float* obs_x, const float* dq,
                                   float* grad, void* workspace, eco_stream_t stream) {
  return grad_rows(kRowsLarge, packed, n_obs_in, gs, graph_ids, batch, obs_x, dq, grad, workspace, stream);
}

extern "C" size_t eco_mpnn_grad_wg_workspace_bytes(int32_t n_spins, int32_t batch) {
  return mpnn_grad_rows_layout(kRowsWg, n_spins, batch, slab_bytes()).total;
}

extern "C" int eco_mpnn_grad_wg(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                                const int32_t* graph_ids, int32_t batch, const float* obs_x, const float* dq,
                                float* grad, void* workspace, eco_stream_t stream) {
  return grad_rows(kRowsWg, packed, n_obs_in, gs, graph_ids, batch, obs_x, dq, grad, workspace, stream);
}

extern "C" int eco_dqn_td_weighted(const float* q_s, const float* q_target_next, const int32_t* a_star,
                                   const int32_t* actions, const float* rewards, const float* dones, int32_t batch,
                                   int32_t n_spins, float gamma, int32_t clip_q_targets, int32_t loss_kind, float* dq,
                                   float* sqerr, float* loss, const float* is_weights, float* abs_td,
                                   eco_stream_t stream) {
  if (!q_s || !q_target_next || !a_star || !actions || !rewards || !dones || !dq || !sqerr || !loss)
    return fail(ECO_ERR_ARG, "null argument");
  if (batch < 1 || n_spins < 1) return fail(ECO_ERR_ARG, "bad batch/n_spins");
  if (loss_kind != ECO_LOSS_MSE && loss_kind != ECO_LOSS_HUBER)
    return fail(ECO_ERR_ARG, "loss_kind must be ECO_LOSS_MSE or ECO_LOSS_HUBER");
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)batch * n_spins;
  const unsigned nblk = (unsigned)((n + 255) / 256);
  const bool prio = is_weights || abs_td;
#define ECO_TD_LAUNCH(H, P)                                                                                          \
  td_kernel<H, P><<<nblk, 256, 0, st>>>(q_s, q_target_next, a_star, actions, rewards, dones, batch, n_spins, gamma, \
                                        clip_q_targets, dq, sqerr, is_weights, abs_td)
  if (loss_kind == ECO_LOSS_HUBER) {
    if (prio) ECO_TD_LAUNCH(true, true);
    else ECO_TD_LAUNCH(true, false);
  } else {
    if (prio) ECO_TD_LAUNCH(false, true);
    else ECO_TD_LAUNCH(false, false);
  }
#undef ECO_TD_LAUNCH
  mean_kernel<<<1, 256, 0, st>>>(sqerr, batch, loss);
  return check_launch("dqn_td");
}

extern "C" int eco_dqn_td_loss(const float* q_s, const float* q_target_next, const int32_t* a_star,
                               const int32_t* actions, const float* rewards, const float* dones, int32_t batch,
                               int32_t n_spins, float gamma, int32_t clip_q_targets, int32_t loss_kind, float* dq,
                               float* sqerr, float* loss, eco_stream_t stream) {
  return eco_dqn_td_weighted(q_s, q_target_next, a_star, actions, rewards, dones, batch, n_spins, gamma,
                             clip_q_targets, loss_kind, dq, sqerr, loss, nullptr, nullptr, stream);
}

extern "C" int eco_dqn_td(const float* q_s, const float* q_target_next, const int32_t* a_star,
                          const int32_t* actions, const float* rewards, const float* dones, int32_t batch,
                          int32_t n_spins, float gamma, int32_t clip_q_targets, float* dq, float* sqerr,
                          float* loss, eco_stream_t stream) {
  return eco_dqn_td_loss(q_s, q_target_next, a_star, actions, rewards, dones, batch, n_spins, gamma, clip_q_targets,
                         ECO_LOSS_MSE, dq, sqerr, loss, stream);
}

extern "C" int eco_grad_clip(float* grad, int32_t n, double grad_scale, double max_norm, float* norm_out,
                             eco_stream_t stream) {
  if (!grad || !norm_out) return fail(ECO_ERR_ARG, "null argument");
  if (n < 1) return fail(ECO_ERR_ARG, "grad clip: n must be positive");
  if (!(max_norm > 0.0) || !std::isfinite(max_norm)) return fail(ECO_ERR_ARG, "grad clip: max_norm must be finite and positive");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)std::min<long long>(GC_MAX_BLOCKS, ((long long)n + GC_CHUNK - 1) / GC_CHUNK);
  grad_sumsq_kernel<<<nblk, 256, 0, st>>>(grad, n);
  grad_norm_kernel<<<1, 256, 0, st>>>(nblk, grad_scale, max_norm, norm_out);
  grad_scale_kernel<<<(unsigned)(((size_t)n + 255) / 256), 256, 0, st>>>(grad, n, norm_out);
  return check_launch("grad_clip");
}

extern "C" int eco_adam(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int32_t n, double lr,
                        double beta1, double beta2, double eps, double weight_decay, double grad_scale, int64_t step,
                        eco_stream_t stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || n < 1 || step < 1) return fail(ECO_ERR_ARG, "bad adam args");
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  adam_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(params, grad, exp_avg, exp_avg_sq, n, (float)beta1,
                                                               (float)beta2, (float)(lr / bc1),
                                                               (float)std::sqrt(bc2), (float)eps,
                                                               (float)weight_decay, (float)grad_scale);
  return check_launch("adam");
}
