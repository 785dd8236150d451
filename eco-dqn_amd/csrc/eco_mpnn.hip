// MPNN Q-network (src/networks/mpnn.py) forward + backward, fused per graph block on
// gfx950, with the epsilon-greedy act (dqn.py:453-465, :490-512) fused into the readout.
//
// One 256-thread workgroup (4 waves) owns a block of whole graphs (graphs_per_block
// = max(1, 256/N)); the block's node embeddings H [rows][64] fp32 live in LDS for
// the whole forward.  Every stage runs on the same layout:
//   * message aggregation (A.H / deg and the edge embedding) is a sparse gather over
//     the CSR rows from LDS, accumulated DIRECTLY in the MFMA A-operand layout (lane l:
//     node l&15, features 16c + 4(l>>4) + 0..3), so no transpose is needed;
//   * every per-node Linear (128->64, 64->64) is v_mfma_f32_16x16x4_f32 (exact f32,
//     no TF32 on gfx950) with the k index permuted so that both operands are single
//     16-byte loads: MFMA kk of a 16-wide k chunk takes k = 16c + 4(l>>4) + kk;
//   * the edge layer never builds the [N,N,63] edge tensor (mpnn.py:90-100): with
//     Z = Wx.x per node in LDS, relu(We.[A_ij, x_j]) = relu(A_ij*w_a + Z_j) per edge.
// The backward (autograd of the same graph, dqn.py:440-449) mirrors it: activation
// gradients per block (A^T.x aggregations are gathers because A is symmetric), weight
// gradients as separate split-K reductions over all nodes (eco_train.hip).
#include "eco_common.h"
#include "eco_mpnn.h"
#include "eco_mpnn_dev.h"

#include <atomic>
#include <cstdlib>

namespace eco {

// Optional per-phase wall-clock stamps (make timing -> libecohip_timing.so; tools/phase_timing.py).
// Slots [blk][0..15] forward, [blk][16..31] backward, first ECO_TS_BLOCKS blocks only.
#ifdef ECO_PHASE_TIMING
constexpr int ECO_TS_BLOCKS = 8192;
__device__ unsigned long long eco_phase_ts[ECO_TS_BLOCKS * 32];
#define ECO_TS(k)                                                                                           \
  do {                                                                                                      \
    if (threadIdx.x == 0 && blockIdx.x < ECO_TS_BLOCKS) eco_phase_ts[blockIdx.x * 32 + (k)] = wall_clock64(); \
  } while (0)
// stamps of logical block b (persistent kernels: one workgroup walks several blocks)
#define ECO_TSB(k, b)                                                                       \
  do {                                                                                      \
    if (threadIdx.x == 0 && (b) < ECO_TS_BLOCKS) eco_phase_ts[(b) * 32 + (k)] = wall_clock64(); \
  } while (0)
#else
#define ECO_TS(k) \
  do {            \
  } while (0)
#define ECO_TSB(k, b) \
  do {                \
  } while (0)
#endif


}  // namespace eco
#include "eco_mpnn_dense.h"  // dense-aggregation kernels (after the phase-timing buffer)
#include "eco_mpnn_dense2.h"  // their fp16x2 successors
#include "eco_mpnn_dense3.h"  // the fp16x2 forward, two tiles per wave
#include "eco_mpnn_dl.h"      // one graph of 224 < N <= 512 per workgroup
#include "eco_mpnn_shared.h"  // many episodes on one shared large graph (G22)
namespace eco {

// Per-matrix power-of-two scale of the fp16x2 Linear pieces (PK_FHS, eco_mpnn.h): one block per matrix
// (Wf, then Wm / Wu of each layer); kw puts max |w| 2^kw into [2^14, 2^15).
__device__ __forceinline__ float wave_fmax(float v) {  // fmaxf over the wave (NaNs dropped, as fmaxf does)
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x128, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x124, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x122, 0xF, 0xF, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x121, 0xF, 0xF, false)));
  auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(s16[0]), __uint_as_float(s16[1]));
  auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(s32[0]), __uint_as_float(s32[1]));
}

// Per-matrix power-of-two scale of the fp16x2 Linear pieces (PK_FHS, eco_mpnn.h): one block per matrix
// (Wf, then Wm / Wu of each layer); kw puts max |w| 2^kw into [2^14, 2^15).  1024 threads, wave maxima.
constexpr int PS_THREADS = 1024;
__global__ __launch_bounds__(PS_THREADS) void pack_scale_kernel(const float* __restrict__ f, int nobs,
                                                                 float* __restrict__ p) {
  const FlatOffsets o = flat_offsets(nobs);
  const int m = blockIdx.x;
  const float* W = m == 0 ? f + o.Wf : f + o.L + (m - 1) * 8192;
  const int n = m == 0 ? 4096 : 8192;
  float mx = 0.f;
  for (int i = threadIdx.x; i < n; i += PS_THREADS) mx = fmaxf(mx, fabsf(W[i]));
  mx = wave_fmax(mx);
  __shared__ float red[PS_THREADS / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int k = 0; k < PS_THREADS / 64; ++k) v = fmaxf(v, red[k]);
    const int kw = (v > 0.f && v < INFINITY) ? 15 - __builtin_amdgcn_frexp_expf(v) : 0;
    p[PK_FHS + m] = __int_as_float(kw);
  }
}

__global__ void pack_kernel(const float* __restrict__ f, int nobs, float* __restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= PK_TOTAL) return;
  const FlatOffsets o = flat_offsets(nobs);
  float v = 0.f;
  if (i >= PK_FHS && i < PK_FH) return;  // scale exponents: pack_scale_kernel
  if (i >= PK_FH) {  // fp16x2 pieces, two fp16 per float slot
    uint16_t h[2];
    for (int t = 0; t < 2; ++t) {
      const int e = 2 * (i - PK_FH) + t;
      const bool tr = e >= FH_FWD_END;
      const int et = tr ? e - FH_FWD_END : e;
      const float* W;
      int in_dim, lin, mat;
      if (et < FH_LAYER) {
        W = f + o.Wf;
        in_dim = 64;
        lin = et;
        mat = 0;
      } else {
        const int e2 = et - FH_LAYER;
        const int l = e2 / FH_LAYER_STRIDE, r = e2 % FH_LAYER_STRIDE;
        const int which = r / (2 * FH_HALF);
        W = f + o.L + l * 16384 + which * 8192;
        in_dim = 128;
        lin = r % (2 * FH_HALF);
        mat = 1 + 2 * l + which;
      }
      const int frag = lin / FH_FRAG, within = lin % FH_FRAG;
      const int ln = within >> 3, jj = within & 7;
      const int kc2 = frag & 1, nt = (frag >> 1) & 3, pl = (frag >> 3) & 1, half = frag >> 4;
      const int kp = 64 * half + 32 * kc2 + 8 * (ln >> 4) + jj;
      const float wv = tr ? W[bf16_kprime_feature(kp & 63) * in_dim + 64 * half + 16 * nt + (ln & 15)]
                          : W[(16 * nt + (ln & 15)) * in_dim + bf16_kprime_feature(kp)];
      const float s = ldexpf(wv, __float_as_int(p[PK_FHS + mat]));
      const _Float16 h1 = (_Float16)s;
      const _Float16 h2 = (_Float16)(s - (float)h1);
      h[t] = __builtin_bit_cast(uint16_t, pl == 0 ? h1 : h2);
    }
    v = __uint_as_float((uint32_t)h[0] | ((uint32_t)h[1] << 16));
  } else if (i >= PK_W0H) {  // feature columns 8..15
    const bool wx = i >= PK_WXH;
    const int j = i - (wx ? PK_WXH : PK_W0H);
    const int r = j >> 3, c = 8 + (j & 7);
    if (!wx) v = c < nobs ? f[o.W0 + r * nobs + c] : 0.f;
    else v = (r < 63 && c < nobs) ? f[o.We + r * (1 + nobs) + 1 + c] : 0.f;
  } else if (i < PK_WX) {
    const int r = i >> 3, c = i & 7;
    v = c < nobs ? f[o.W0 + r * nobs + c] : 0.f;
  } else if (i < PK_WA) {
    const int r = (i - PK_WX) >> 3, c = (i - PK_WX) & 7;
    v = (r < 63 && c < nobs) ? f[o.We + r * (1 + nobs) + 1 + c] : 0.f;
  } else if (i < PK_WF) {
    const int r = i - PK_WA;
    v = r < 63 ? f[o.We + r * (1 + nobs)] : 0.f;
  } else if (i < PK_LAYER) {
    v = f[o.Wf + (i - PK_WF)];
  } else if (i < PK_WP) {
    v = f[o.L + (i - PK_LAYER)];  // message0, update0, message1, ... same order as state_dict
  } else if (i < PK_WR) {
    v = f[o.Wp + (i - PK_WP)];
  } else if (i < PK_BR) {
    v = f[o.Wr + (i - PK_WR)];
  } else if (i == PK_BR) {
    v = f[o.Br];
  } else if (i >= PK_WFT && i < PK_LAYERT) {
    const int j = i - PK_WFT;  // WfT[in][out] = Wf[out][in]
    v = f[o.Wf + (j & 63) * 64 + (j >> 6)];
  } else if (i >= PK_LAYERT && i < PK_LAYERT + 3 * 16384) {
    const int l = (i - PK_LAYERT) / 16384;
    const int j = (i - PK_LAYERT) % 16384;
    const int which = j / 8192;  // 0: message, 1: update
    const int jj = j % 8192;     // T[in (128)][out (64)]
    v = f[o.L + l * 16384 + which * 8192 + (jj & 63) * 128 + (jj >> 6)];
  } else if (i >= PK_BF) {
    // two bf16 plane elements per float slot
    uint16_t h[2];
    for (int t = 0; t < 2; ++t) {
      const int e = 2 * (i - PK_BF) + t;
      const float* W;
      int in_dim, lin;
      const bool tr = e >= BF_FWD_END;  // transposed fragments of the backward
      const int et = tr ? e - BF_FWD_END : e;
      if (et < BF_LAYER) {
        W = f + o.Wf;
        in_dim = 64;
        lin = et;
      } else {
        const int e2 = et - BF_LAYER;
        const int l = e2 / BF_LAYER_STRIDE, r = e2 % BF_LAYER_STRIDE;
        W = f + o.L + l * 16384 + (r / (2 * BF_HALF)) * 8192;
        in_dim = 128;
        lin = r % (2 * BF_HALF);
      }
      const int frag = lin / BF_FRAG, within = lin % BF_FRAG;
      const int ln = within >> 3, jj = within & 7;
      const int kc2 = frag & 1, nt = (frag >> 1) & 3, pl = (frag >> 3) % 3, half = frag / 24;
      const int kp = 64 * half + 32 * kc2 + 8 * (ln >> 4) + jj;
      // forward: W[16nt + (l&15)][feature(kp)];  transposed: W^T[64 half + 16nt + (l&15)][feature(kp & 63)]
      const float wv = tr ? W[bf16_kprime_feature(kp & 63) * in_dim + 64 * half + 16 * nt + (ln & 15)]
                          : W[(16 * nt + (ln & 15)) * in_dim + bf16_kprime_feature(kp)];
      uint16_t p1, p2, p3;
      split3_bits(wv, p1, p2, p3);
      h[t] = pl == 0 ? p1 : (pl == 1 ? p2 : p3);
    }
    v = __uint_as_float((uint32_t)h[0] | ((uint32_t)h[1] << 16));
  }
  p[i] = v;
}

// MAXT: max 16-node tiles per wave; NW: waves per workgroup; WLDS: stage each layer's weights in
// LDS (one copy per workgroup, read as conflict-free ds_read_b128 B operands) instead of
// streaming them from L2 in every wave.
// LDS: Hs [rows_pad][LDH] | Wl [2][64][LDW] (WLDS) | Xs [rows_pad][8] (WLDS) or readout scratch |
//      RI [rows_pad] int2 | GB [gpb] i64 | MD [gpb]
// FW: float-weighted graph set (gs.edge_weights): every gather reads (float)edge_weights[q] instead of the packed byte
template <int MAXT, bool SAVE, int NW, bool WLDS, bool FW = false>
__global__ __launch_bounds__(64 * NW, (NW == 8 && WLDS ? 2 : 1)) void mpnn_forward_kernel(MpnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ECO_TS(0);
  constexpr int NT = 64 * NW;
  const int lane = threadIdx.x & 63;
  const int w = uniform_i(threadIdx.x >> 6);
  const int blk = blockIdx.x;
  const int N = a.N;
  const int g_valid = min(a.gpb, a.B - blk * a.gpb);
  const int rows_valid = g_valid * N;
  const int rows_pad = (a.gpb * N + 15) & ~15;
  const int ntiles = rows_pad >> 4;
  float* Hs = lds;
  float* Wl = lds + rows_pad * LDH;
  float* Mreg = Wl + (WLDS ? 2 * 64 * LDW : 0);
  float* Xs = Mreg;                 // [rows_pad][8] node features (WLDS; else x is read from global)
  int2* RI = reinterpret_cast<int2*>(Mreg + fwd_mreg_floats(rows_pad, a.gpb, NW, WLDS));
  int64_t* GB = reinterpret_cast<int64_t*>(RI + rows_pad);  // [gpb] per-graph edge base
  int* MD = reinterpret_cast<int*>(GB + a.gpb);               // [gpb] per-graph max degree
  int* SCH = MD + ((a.gpb + 1) & ~1);                           // [64] tile schedule
  float* Es = WLDS ? Wl : Mreg;     // phase-E scratch
  const size_t R0 = (size_t)blk * a.gpb * N;
  const size_t RT = (size_t)a.B * N;
  const float* P = a.P;
  const uint16_t* BFP = reinterpret_cast<const uint16_t*>(P + PK_BF);
  const int s4 = lane >> 4;
  const int c16 = lane & 15;
  const uint32_t* __restrict__ edges = a.gs.edges;
  const double* __restrict__ ewts = a.gs.edge_weights;  // FW only
  if constexpr (!SAVE) {  // every graph of the block explores: the draw alone, no forward
    if (act_skip_block<NW>(a, blk, g_valid, R0)) return;
  }

  // ---- staging: x rows (WLDS, 8-float rows), row info, Wf ----
  const bool xwide = a.xw == 16;  // features 8..15 (read from global memory, never staged)
  if (WLDS && !xwide) {
    for (int i = threadIdx.x; i < rows_pad * 2; i += NT) {
      const int r = i >> 1;
      float4 v = zero4();
      if (r < rows_valid) v = f4(a.x + (R0 + r) * 8 + 4 * (i & 1));
      st4(Xs + 8 * r + 4 * (i & 1), v);
    }
  }
  // node features 0..7 of row r (zero for padding rows)
  auto xrow = [&](int r, float4& x0, float4& x1) {
    if (WLDS && !xwide) {
      x0 = f4(Xs + 8 * r);
      x1 = f4(Xs + 8 * r + 4);
    } else {
      x0 = r < rows_valid ? f4(a.x + (R0 + r) * a.xw) : zero4();
      x1 = r < rows_valid ? f4(a.x + (R0 + r) * a.xw + 4) : zero4();
    }
  };
  // w . x over features 8..15 (wide rows only)
  auto xdot_hi = [&](int r, const float* wh) {
    if (!xwide || r >= rows_valid) return 0.f;
    const float4 x2 = f4(a.x + (R0 + r) * 16 + 8), x3 = f4(a.x + (R0 + r) * 16 + 12);
    return wh[0] * x2.x + wh[1] * x2.y + wh[2] * x2.z + wh[3] * x2.w + wh[4] * x3.x + wh[5] * x3.y + wh[6] * x3.z +
           wh[7] * x3.w;
  };
  for (int r = threadIdx.x; r < rows_pad; r += NT) RI[r] = pack_row_info(a, blk, r, rows_valid);
  for (int gl = threadIdx.x; gl < g_valid; gl += NT) {
    const int gid = a.gids[blk * a.gpb + gl];
    GB[gl] = a.gs.edge_base[gid];
    MD[gl] = a.gs.max_deg[gid];
  }
  if constexpr (WLDS) stage_rows<NT>(Wl, LDH, P + PK_WF, 64, 64, 64);
  __syncthreads();
  if (w == 0) build_tile_schedule(SCH, RI, ntiles, NW, MAXT);  // published by the barrier after phase A
  ECO_TS(1);

  // ---- phase A: Z = Wx . x  (edge-embedding node term) into Hs ----
  {
    float wx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wx[k] = P[PK_WX + lane * 8 + k];
    for (int r = w; r < rows_pad; r += NW) {
      float4 x0, x1;
      xrow(r, x0, x1);
      Hs[r * LDH + lane] = wx[0] * x0.x + wx[1] * x0.y + wx[2] * x0.z + wx[3] * x0.w + wx[4] * x1.x +
                           wx[5] * x1.y + wx[6] * x1.z + wx[7] * x1.w + xdot_hi(r, P + PK_WXH + lane * 8);
    }
  }
  __syncthreads();
  ECO_TS(2);

  // ---- phase B: edge embedding (mpnn.py:89-104) -> e (registers, operand layout) ----
  float4 ereg[MAXT][4];
  {
    const int maxdeg_call = a.norm_scope == ECO_NORM_PER_CALL ? *a.call_maxdeg : 0;
    float wa[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) wa[c * 4 + i] = P[PK_WA + 16 * c + 4 * s4 + i];
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NW];
      if (t >= ntiles) break;
      const int r = t * 16 + c16;
      const RowInfo ri = row_info(RI, r);
      const bool valid = r < rows_valid;
      const int rbase = (r / N) * N;
      float4 acc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = zero4();
      const size_t gb = valid ? GB[r / N] : 0;
      for_edges(edges + gb, ri.e0, ri.e1, [&](uint32_t ex, int q) {
        const float wv = edge_wf<FW>(ex, ewts + gb, q);
        const float* zr = Hs + (rbase + edge_col(ex)) * LDH + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 z = f4(zr + 16 * c);
          acc[c].x += relu(fmaf(wv, wa[4 * c + 0], z.x));
          acc[c].y += relu(fmaf(wv, wa[4 * c + 1], z.y));
          acc[c].z += relu(fmaf(wv, wa[4 * c + 2], z.z));
          acc[c].w += relu(fmaf(wv, wa[4 * c + 3], z.w));
        }
      });
      const float nf = (float)ri.norm;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[c].x = acc[c].x / nf; acc[c].y = acc[c].y / nf; acc[c].z = acc[c].z / nf; acc[c].w = acc[c].w / nf;
      }
      // feature 63 = norm / norm.max()  (mpnn.py:102)
      const int md = a.norm_scope == ECO_NORM_PER_CALL ? maxdeg_call : (valid ? MD[r / N] : 1);
      if (s4 == 3) acc[3].w = nf / (float)md;
      if (!valid) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = zero4();
      } else if (SAVE) {
        float* ea = a.sv + (size_t)SV_EAGG * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) st4(ea + 16 * c, acc[c]);
      }
      f32x4 d[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (WLDS) mm_k<4, 4, true>(d, acc, Wl, LDH, lane);
      else mm_bf3_lean(d, acc, BFP + BF_WF, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        ereg[ti][nt] = relu4(d[nt]);  // the tile's e rows stay in this wave's registers for the layers
        if (SAVE && valid) st4(a.sv + (size_t)SV_E * RT * 64 + (R0 + r) * 64 + 16 * nt + 4 * s4, ereg[ti][nt]);
      }
    }
  }
  __syncthreads();
  ECO_TS(3);

  // ---- phase C: h0 = relu(W0 . x) (mpnn.py:20-23, :55) into Hs ----
  {
    float w0[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w0[k] = P[PK_W0 + lane * 8 + k];
    for (int r = w; r < rows_pad; r += NW) {
      float4 x0, x1;
      xrow(r, x0, x1);
      const float z = relu(w0[0] * x0.x + w0[1] * x0.y + w0[2] * x0.z + w0[3] * x0.w + w0[4] * x1.x +
                           w0[5] * x1.y + w0[6] * x1.z + w0[7] * x1.w + xdot_hi(r, P + PK_W0H + lane * 8));
      if (SAVE && r < rows_valid) a.sv[(size_t)SV_H0 * RT * 64 + (R0 + r) * 64 + lane] = z;
      Hs[r * LDH + lane] = z;
    }
  }
  __syncthreads();
  ECO_TS(4);

  // ---- phase D: 3 x UpdateNodeEmbeddingLayer (mpnn.py:114-120) ----
  for (int layer = 0; layer < 3; ++layer) {
    const float* Wm = P + PK_LAYER + layer * 16384;
    const float* Wu = Wm + 8192;
    if constexpr (WLDS) {  // the previous readers of Wl finished at the last barrier
      stage_rows<NT>(Wl, LDW, Wm, 128, 64, 128);
      stage_rows<NT>(Wl + 64 * LDW, LDW, Wu, 128, 64, 128);
      __syncthreads();
    }
    if (layer == 0) ECO_TS(10);
    // Half of each tile's MFMAs do not depend on the aggregation: Wm[:, 64:].e and Wu[:, :64].h.
    // Waves with (w >> 2) even issue that half BEFORE their gather, the others after it, so each
    // SIMD's MFMA pipe has work while its other waves gather from LDS (waves w, w+4 share a SIMD).
    const bool mfma_first = ((w >> 2) & 1) == 0;
    const float* WmL = WLDS ? Wl : Wm;
    const float* WuL = WLDS ? Wl + 64 * LDW : Wu;
    // weights from L2 (no LDS staging): the exact bf16x3-split fragments of the dense path (six products
    // above 2^-24, f32-accurate) -- 2.7x the f32 MFMA rate, and no f32 weight double buffer in registers
    const uint16_t* BFL = BFP + BF_LAYER + layer * BF_LAYER_STRIDE;  // message halves, then update halves
    constexpr int ldw = WLDS ? LDW : 128;
    f32x4 hn[MAXT][4];
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NW];
      if (t < ntiles) {
        const int r = t * 16 + c16;
        const RowInfo ri = row_info(RI, r);
        const bool valid = r < rows_valid;
        float4 agg[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) agg[c] = zero4();
        const size_t gb = valid ? GB[r / N] : 0;
        const uint32_t* eg = edges + gb;
        if (!mfma_first) gather_ri<FW>(ri, eg, Hs, (r / N) * N, s4, agg, ewts + gb);
        // gather-independent half: d = Wm[:, 64:] . e ; hn = Wu[:, :64] . h
        f32x4 d[4];
        float4 hcur[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
          hn[ti][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
          hcur[nt] = f4(Hs + r * LDH + 16 * nt + 4 * s4);
        }
        if constexpr (WLDS) {
          mm_k<4, 4, true>(d, ereg[ti], WmL + 64, ldw, lane);
          mm_k<4, 4, true>(hn[ti], hcur, WuL, ldw, lane);
        } else {
          mm_bf3_lean(d, ereg[ti], BFL + BF_HALF, lane);
          mm_bf3_lean(hn[ti], hcur, BFL + 2 * BF_HALF, lane);
        }
        if (layer == 0 && ti == 0) ECO_TS(11);
        if (mfma_first) gather_ri<FW>(ri, eg, Hs, (r / N) * N, s4, agg, ewts + gb);
        if (layer == 0 && ti == 0) ECO_TS(12);
        // aggregation (A . h) / norm (mpnn.py:118), already in operand layout
        const float nf = (float)ri.norm;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          agg[c].x = agg[c].x / nf; agg[c].y = agg[c].y / nf; agg[c].z = agg[c].z / nf; agg[c].w = agg[c].w / nf;
        }
        if (SAVE && valid) {
          float* sa = a.sv + (size_t)(SV_AGG0 + layer) * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(sa + 16 * c, agg[c]);
        }
        // message = relu(Wm . [agg, e]) (mpnn.py:119)
        if constexpr (WLDS) mm_k<4, 4, true>(d, agg, WmL, ldw, lane);
        else mm_bf3_lean(d, agg, BFL, lane);
        float4 mrel[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) mrel[c] = relu4(d[c]);
        if (SAVE && valid) {
          float* sm = a.sv + (size_t)(SV_M0 + layer) * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(sm + 16 * c, mrel[c]);
        }
        // h' = relu(Wu . [h, m]) (mpnn.py:120)
        if constexpr (WLDS) mm_k<4, 4, true>(hn[ti], mrel, WuL + 64, ldw, lane);
        else mm_bf3_lean(hn[ti], mrel, BFL + 3 * BF_HALF, lane);
        if (layer == 0 && ti == 0) {
          ECO_TS(13);
#ifdef ECO_PHASE_TIMING
#ifdef ECO_PHASE_TIMING
          asm volatile("" ::"v"(hn[ti][3][3]));  // wait for the tile's last MFMA
#endif
#endif
          ECO_TS(14);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NW];
      if (t < ntiles) {
        const int r = t * 16 + c16;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float4 hv = relu4(hn[ti][nt]);
          st4(Hs + r * LDH + 16 * nt + 4 * s4, hv);
          if (SAVE && r < rows_valid) st4(a.sv + (size_t)(SV_H0 + layer + 1) * RT * 64 + (R0 + r) * 64 + 16 * nt + 4 * s4, hv);
        }
      }
    }
    __syncthreads();
    ECO_TS(5 + layer);
  }

  // ---- phase E: ReadoutLayer (mpnn.py:143-159) + epsilon-greedy act, spread over all waves ----
  readout_act<SAVE, NW>(a, Hs, LDH, Es, a.gpb < NW, blk, g_valid, rows_valid, R0, RT);
  ECO_TS(8);
  ECO_TS(9);
}

// ============================================================== backward ====
// y[0..127] += W^T x for one 64-input transposed Linear from its two bf16x3 output-half fragment sets
__device__ __forceinline__ void bf3_t2(f32x4 (&d8)[8], const float4 (&x)[4], const uint16_t* WT, int lane) {
  f32x4 lo[4], hi[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) { lo[nt] = d8[nt]; hi[nt] = d8[4 + nt]; }
  mm_bf3_lean(lo, x, WT, lane);
  mm_bf3_lean(hi, x, WT + BF_HALF, lane);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) { d8[nt] = lo[nt]; d8[4 + nt] = hi[nt]; }
}

// Gradient of loss w.r.t. all MPNN parameters given dq = dLoss/dQ [B][N], for the
// forward saved in a.sv.  This kernel produces the activation gradients (the
// pre-activation gradients dY of every Linear, stored [R][64]) and the small
// per-graph / per-block partials; eco_train.hip reduces dW = sum_nodes dY^T X.
// LDS: G [rows_pad][LDH] (dq rows at the start) | Wl [2][128][LDH] (WLDS: Wu^T, Wm^T) | Xs [rows_pad][8] (WLDS) |
//      RI [rows_pad] int2 | GB [gpb] i64 | DMEAN [gpb][64] | RED [(gpb < NW ? gpb : 1)][NW][64]
template <int MAXT, int NW, bool WLDS, bool FW = false>
__global__ __launch_bounds__(64 * NW, (NW == 8 && WLDS ? 2 : 1)) void mpnn_backward_kernel(MpnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ECO_TS(16);
  constexpr int NWAVE = NW;
  constexpr int NT = 64 * NW;
  const int lane = threadIdx.x & 63;
  const int w = uniform_i(threadIdx.x >> 6);
  const int blk = blockIdx.x;
  const int N = a.N;
  const int g_valid = min(a.gpb, a.B - blk * a.gpb);
  const int rows_valid = g_valid * N;
  const int rows_pad = (a.gpb * N + 15) & ~15;
  const int ntiles = rows_pad >> 4;
  const bool split = a.gpb < NW;  // readout: all waves per graph
  float* G = lds;                                   // gathered-gradient source rows
  float* DQ = G;                                    // [rows_pad] dq of the block's rows (start only)
  float* Wl = G + rows_pad * LDH;                   // staged Wu^T | Wm^T, [128][LDH] each (WLDS)
  float* Xs = Wl + (WLDS ? 2 * 128 * LDH : 0);      // [rows_pad][8] (WLDS)
  int2* RI = reinterpret_cast<int2*>(Xs + (WLDS ? rows_pad * 8 : 0));
  int64_t* GB = reinterpret_cast<int64_t*>(RI + rows_pad);
  float* DMEAN = reinterpret_cast<float*>(GB + a.gpb);
  float* RED = DMEAN + a.gpb * 64;
  int* SCH = reinterpret_cast<int*>(RED + (a.gpb < NW ? a.gpb : 1) * NW * 64);  // [64] tile schedule
  const size_t R0 = (size_t)blk * a.gpb * N;
  const size_t RT = (size_t)a.B * N;
  const float* P = a.P;
  const float* sv = a.sv;
  float* gr = a.gr;
  const int s4 = lane >> 4;
  const int c16 = lane & 15;
  const uint32_t* __restrict__ edges = a.gs.edges;
  auto SV = [&](int t) { return sv + (size_t)t * RT * 64; };
  auto GR = [&](int t) { return gr + (size_t)t * RT * 64; };
  const float* MEAN = sv + (size_t)SV_NODE_TENSORS * RT * 64;
  const float* PP = MEAN + (size_t)a.B * 64;
  float* DP = gr + (size_t)GR_NODE_TENSORS * RT * 64;
  float* DWRA = DP + (size_t)a.B * 64;
  float* DWRB = DWRA + (size_t)a.B * 64;
  float* DBR = DWRB + (size_t)a.B * 64;
  float* DWA = DBR + ((a.B + 63) & ~63);  // [nblocks][64]

  // ---- staging: dq rows, row info, edge bases, x rows ----
  for (int r = threadIdx.x; r < rows_pad; r += NT) {
    DQ[r] = r < rows_valid ? a.dq[R0 + r] : 0.f;
    RI[r] = pack_row_info(a, blk, r, rows_valid);
  }
  for (int gl = threadIdx.x; gl < g_valid; gl += NT) GB[gl] = a.gs.edge_base[a.gids[blk * a.gpb + gl]];
  const bool xwide = a.xw == 16;  // features 8..15: read from global memory
  if (WLDS && !xwide) {
    for (int i = threadIdx.x; i < rows_pad * 2; i += NT) {
      const int r = i >> 1;
      st4(Xs + 8 * r + 4 * (i & 1), r < rows_valid ? f4(a.x + (R0 + r) * 8 + 4 * (i & 1)) : zero4());
    }
  }
  __syncthreads();
  if (w == 0) build_tile_schedule(SCH, RI, ntiles, NWAVE, MAXT);  // published by the barrier after the readout
  ECO_TS(17);

  // ---- readout backward (mpnn.py:143-159) ----
  // dWr[64:] = sum_v dq_v h3_v: spread over all waves when the block holds fewer graphs than waves
  if (split) {
    for (int gl = 0; gl < g_valid; ++gl) {
      const float* h3 = SV(SV_H3) + (R0 + (size_t)gl * N) * 64;
      float dwb = 0.f;
      for (int v = w; v < N; v += NWAVE) {
        const float dv = DQ[gl * N + v];
        if (dv != 0.f) dwb = fmaf(dv, h3[(size_t)v * 64 + lane], dwb);
      }
      RED[(gl * NWAVE + w) * 64 + lane] = dwb;
    }
    __syncthreads();
  }
  for (int gl = w; gl < g_valid; gl += NWAVE) {
    const int e = blk * a.gpb + gl;
    float s = 0.f;
    for (int v = lane; v < N; v += 64) s += DQ[gl * N + v];
    const float S = wave_sum_f(s);                       // d(sum_i q_i) / d br ...
    const float p = PP[(size_t)e * 64 + lane];
    const float wr = P[PK_WR + lane];
    const float dp = wr * S * (p > 0.f ? 1.f : 0.f);
    DP[(size_t)e * 64 + lane] = dp;
    DWRA[(size_t)e * 64 + lane] = relu(p) * S;
    if (lane == 0) DBR[e] = S;
    float dmean = 0.f;
#pragma unroll 16
    for (int k = 0; k < 64; ++k) dmean = fmaf(P[PK_WP + k * 64 + lane], __shfl(dp, k, 64), dmean);
    DMEAN[gl * 64 + lane] = dmean / (float)N;
    float dwb = 0.f;
    if (split) {
#pragma unroll
      for (int k = 0; k < NWAVE; ++k) dwb += RED[(gl * NWAVE + k) * 64 + lane];  // fixed order
    } else {
      const float* h3 = SV(SV_H3) + (R0 + (size_t)gl * N) * 64;
      for (int v = 0; v < N; ++v) {
        const float dv = DQ[gl * N + v];
        if (dv != 0.f) dwb = fmaf(dv, h3[(size_t)v * 64 + lane], dwb);
      }
    }
    DWRB[(size_t)e * 64 + lane] = dwb;
  }
  __syncthreads();
  ECO_TS(18);

  // dh3 (A layout): dq_i * wr[64+f] + dmean_f / N
  float4 dh[MAXT][4];
#pragma unroll
  for (int ti = 0; ti < MAXT; ++ti) {
    const int t = SCH[w + ti * NWAVE];
    const int r = t * 16 + c16;
#pragma unroll
    for (int c = 0; c < 4; ++c) dh[ti][c] = zero4();
    if (t < ntiles && r < rows_valid) {
      const int gl = r / N;
      const float dqi = DQ[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int f = 16 * c + 4 * s4;
        const float4 dm = f4(DMEAN + gl * 64 + f);
        dh[ti][c] = make_float4(fmaf(dqi, P[PK_WR + 64 + f + 0], dm.x), fmaf(dqi, P[PK_WR + 64 + f + 1], dm.y),
                                fmaf(dqi, P[PK_WR + 64 + f + 2], dm.z), fmaf(dqi, P[PK_WR + 64 + f + 3], dm.w));
      }
    }
  }
  // DQ (aliasing Mreg) is dead from here on; the next barrier orders it before the Z tiles

  // ---- update layers in reverse (mpnn.py:114-120) ----
  // Every Linear runs with the weight as the MFMA A operand (mm_k<.., true>): outputs arrive in the
  // node-operand layout (lane: node l&15, features 16c + 4(l>>4) + i), so the chain
  // duu -> [dh_direct, dm] -> dum -> [dagg, de] needs no transpose and rows are stored as float4.
  const uint16_t* BFP = reinterpret_cast<const uint16_t*>(P + PK_BF);
  for (int layer = 2; layer >= 0; --layer) {
    const float* WmT = P + PK_LAYERT + layer * 16384;  // [128][64]
    const float* WuT = WmT + 8192;                      // [128][64]
    // weights from L2 (no LDS staging): bf16x3-split transposed fragments, [out half][p][nt][kc2]
    const uint16_t* BFT = BFP + BFT_LAYER + layer * BF_LAYER_STRIDE;  // Wm^T halves, then Wu^T halves
    if constexpr (WLDS) {  // previous readers of Wl finished at the last barrier
      stage_rows<NT>(Wl, LDH, WuT, 64, 128, 64);
      stage_rows<NT>(Wl + 128 * LDH, LDH, WmT, 64, 128, 64);
      __syncthreads();
    }
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NWAVE];
      if (t < ntiles) {
        const int r = t * 16 + c16;
        const bool valid = r < rows_valid;
        const size_t ro = (R0 + r) * 64 + 4 * s4;
        // duu = dh' * [h' > 0]
        float4 duu[4], mv[4];
        const float* hnext = SV(SV_H0 + layer + 1) + ro;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 hv = valid ? f4(hnext + 16 * c) : zero4();
          mv[c] = valid ? f4(SV(SV_M0 + layer) + ro + 16 * c) : zero4();
          duu[c] = make_float4(hv.x > 0.f ? dh[ti][c].x : 0.f, hv.y > 0.f ? dh[ti][c].y : 0.f,
                               hv.z > 0.f ? dh[ti][c].z : 0.f, hv.w > 0.f ? dh[ti][c].w : 0.f);
          if (valid) st4(GR(GR_DUU0 + layer) + ro + 16 * c, duu[c]);
        }
        // [dh_direct, dm] = duu . Wu
        f32x4 d8[8];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) d8[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (WLDS) mm_k<8, 4, true>(d8, duu, Wl, LDH, lane);
        else bf3_t2(d8, duu, BFT + 2 * BF_HALF, lane);
        // dum = dm * [m > 0]
        float4 dum[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          dum[c] = make_float4(mv[c].x > 0.f ? d8[4 + c][0] : 0.f, mv[c].y > 0.f ? d8[4 + c][1] : 0.f,
                               mv[c].z > 0.f ? d8[4 + c][2] : 0.f, mv[c].w > 0.f ? d8[4 + c][3] : 0.f);
          if (valid) {
            st4(GR(GR_DUM0 + layer) + ro + 16 * c, dum[c]);
            st4(GR(GR_DH) + ro + 16 * c, make_float4(d8[c][0], d8[c][1], d8[c][2], d8[c][3]));
          }
        }
        // [dagg, de] = dum . Wm;  G rows <- dagg / norm  (d(agg)/d(A.h) = 1/norm)
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) d8[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (WLDS) mm_k<8, 4, true>(d8, dum, Wl + 128 * LDH, LDH, lane);
        else bf3_t2(d8, dum, BFT, lane);
        const float nf = (float)row_info(RI, r).norm;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          st4(G + r * LDH + 16 * c + 4 * s4,
              valid ? make_float4(d8[c][0] / nf, d8[c][1] / nf, d8[c][2] / nf, d8[c][3] / nf) : zero4());
          if (valid) {
            float* de = GR(GR_DE) + ro + 16 * c;
            const float4 prev = layer == 2 ? zero4() : f4(de);
            st4(de, make_float4(prev.x + d8[4 + c][0], prev.y + d8[4 + c][1], prev.z + d8[4 + c][2],
                                prev.w + d8[4 + c][3]));
          }
        }
      }
    }
    __syncthreads();
    // dh_l = dh_direct + A^T . (dagg / norm)   (A symmetric: a gather over the node's own row)
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NWAVE];
      if (t < ntiles) {
        const int r = t * 16 + c16;
        const bool valid = r < rows_valid;
        const RowInfo ri = row_info(RI, r);
        float4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = valid ? f4(GR(GR_DH) + (R0 + r) * 64 + 16 * c + 4 * s4) : zero4();
        const size_t gb = valid ? GB[r / N] : 0;
        gather_ri<FW>(ri, edges + gb, G, (r / N) * N, s4, acc, a.gs.edge_weights + gb);
#pragma unroll
        for (int c = 0; c < 4; ++c) dh[ti][c] = acc[c];
      }
    }
    __syncthreads();
    ECO_TS(21 - layer);
  }

  // ---- h0 = relu(W0.x): du0 ----
#pragma unroll
  for (int ti = 0; ti < MAXT; ++ti) {
    const int t = SCH[w + ti * NWAVE];
    const int r = t * 16 + c16;
    if (t < ntiles && r < rows_valid) {
      const float* h0 = SV(SV_H0) + (R0 + r) * 64 + 4 * s4;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 hv = f4(h0 + 16 * c);
        st4(GR(GR_DU0) + (R0 + r) * 64 + 4 * s4 + 16 * c,
            make_float4(hv.x > 0.f ? dh[ti][c].x : 0.f, hv.y > 0.f ? dh[ti][c].y : 0.f,
                        hv.z > 0.f ? dh[ti][c].z : 0.f, hv.w > 0.f ? dh[ti][c].w : 0.f));
      }
    }
  }

  // ---- edge embedding (mpnn.py:89-104): due, dEagg ----
  if constexpr (WLDS) {  // Wf^T; the last layer's readers finished at the barrier above
    stage_rows<NT>(Wl, LDH, P + PK_WFT, 64, 64, 64);
    __syncthreads();
  }
#pragma unroll
  for (int ti = 0; ti < MAXT; ++ti) {
    const int t = SCH[w + ti * NWAVE];
    if (t < ntiles) {
      const int r = t * 16 + c16;
      const bool valid = r < rows_valid;
      float4 due[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t off = (R0 + r) * 64 + 16 * c + 4 * s4;
        const float4 ev = valid ? f4(SV(SV_E) + off) : zero4();
        const float4 dv = valid ? f4(GR(GR_DE) + off) : zero4();
        due[c] = make_float4(ev.x > 0.f ? dv.x : 0.f, ev.y > 0.f ? dv.y : 0.f, ev.z > 0.f ? dv.z : 0.f,
                             ev.w > 0.f ? dv.w : 0.f);
        if (valid) st4(GR(GR_DUE) + off, due[c]);
      }
      f32x4 d4[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d4[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (WLDS) mm_k<4, 4, true>(d4, due, Wl, LDH, lane);
      else mm_bf3_lean(d4, due, reinterpret_cast<const uint16_t*>(P + PK_BF) + BFT_WF, lane);
      const float nf = (float)row_info(RI, r).norm;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        st4(G + r * LDH + 16 * c + 4 * s4,
            valid ? make_float4(d4[c][0] / nf, d4[c][1] / nf, d4[c][2] / nf, d4[c][3] / nf) : zero4());
    }
  }
  __syncthreads();
  ECO_TS(22);
  // dz_j = sum_{i in N(j)} G_i * [w_ij wa + z_j > 0];  dwa += same * w_ij
  {
    float wa[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) wa[4 * c + i] = P[PK_WA + 16 * c + 4 * s4 + i];
    float dwa[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dwa[i] = 0.f;
#pragma unroll
    for (int ti = 0; ti < MAXT; ++ti) {
      const int t = SCH[w + ti * NWAVE];
      if (t < ntiles) {
        const int r = t * 16 + c16;
        const bool valid = r < rows_valid;
        const RowInfo ri = row_info(RI, r);
        // z = Wx.x of the lane's node for its 16 features (same expression as forward phase A)
        float4 x0 = zero4(), x1 = zero4(), x2 = zero4(), x3 = zero4();
        if (valid) {
          const float* xr = (WLDS && !xwide) ? Xs + 8 * r : a.x + (R0 + r) * a.xw;
          x0 = f4(xr);
          x1 = f4(xr + 4);
          if (xwide) { x2 = f4(xr + 8); x3 = f4(xr + 12); }
        }
        float z[16], dz[16];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float* wx = P + PK_WX + (16 * c + 4 * s4 + i) * 8;
            const float4 w0 = f4(wx), w1 = f4(wx + 4);
            z[4 * c + i] = w0.x * x0.x + w0.y * x0.y + w0.z * x0.z + w0.w * x0.w + w1.x * x1.x + w1.y * x1.y +
                           w1.z * x1.z + w1.w * x1.w;
            if (xwide) {  // same left-to-right order as the forward's xdot_hi term
              const float* wh = P + PK_WXH + (16 * c + 4 * s4 + i) * 8;
              const float4 h0 = f4(wh), h1 = f4(wh + 4);
              z[4 * c + i] += h0.x * x2.x + h0.y * x2.y + h0.z * x2.z + h0.w * x2.w + h1.x * x3.x + h1.y * x3.y +
                              h1.z * x3.z + h1.w * x3.w;
            }
          }
#pragma unroll
        for (int i = 0; i < 16; ++i) dz[i] = 0.f;
        const int rbase = (r / N) * N;
        const size_t gb = valid ? GB[r / N] : 0;
        for_edges(edges + gb, ri.e0, ri.e1, [&](uint32_t ex, int q) {
          const float wv = edge_wf<FW>(ex, a.gs.edge_weights + gb, q);
          const float* gi = G + (rbase + edge_col(ex)) * LDH + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float4 gv = f4(gi + 16 * c);
            const float g4[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int kk = 4 * c + i;
              const float gm = fmaf(wv, wa[kk], z[kk]) > 0.f ? g4[i] : 0.f;
              dz[kk] += gm;
              dwa[kk] = fmaf(gm, wv, dwa[kk]);
            }
          }
        });
        if (valid) {
          float* dzp = GR(GR_DZ) + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(dzp + 16 * c, make_float4(dz[4 * c], dz[4 * c + 1], dz[4 * c + 2], dz[4 * c + 3]));
        }
      }
    }
    // reduce dwa over the 16 node lanes sharing s4, then over waves (fixed order)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = dwa[i];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      dwa[i] = v;
    }
    if (c16 == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) RED[w * 64 + 16 * c + 4 * s4 + i] = dwa[4 * c + i];
    }
    __syncthreads();
    if (w == 0) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NWAVE; ++k) s += RED[k * 64 + lane];
      DWA[(size_t)blk * 64 + lane] = s;
    }
  }
  ECO_TS(23);
}

// ======================================================== large graphs ====
// N > 512 (GSet G22, N = 2000; inference / best-cut search, and the forward inside eco_mpnn_grad_large): the node embeddings no longer fit
// LDS, so each episode's Z / h rows live in global memory (two ping-pong [rows][64] f32 buffers and the
// edge embedding e, in the forward workspace: per episode 3 x rows x 256 B, L2/MALL-resident while the
// workgroup runs).  One workgroup per episode; waves take 16-node tiles round-robin; the
// aggregations are CSR gathers from global rows in the MFMA operand layout; the Linears are the same
// exact-f32 MFMA tiles as the LDS kernels with both layer weights staged in LDS (8 waves: the gathers
// and the 8-chunk Linears need more than the 128 VGPRs of a 16-wave workgroup).
// LDS: Wl [2][64][LDW] | readout scratch
// XW: floats per observation row, 8 or 16 (n_obs_in > 8, MAIN_OBSERVABLES).  The wide instance adds features
// 8..15 to the two 8-input Linears from PK_WXH / PK_W0H in the summation order of mpnn_forward_kernel's xdot_hi:
// the low eight products, then the high eight as one term.
// SAVE: the forward inside eco_mpnn_grad_large -- every activation mpnn_backward_large_kernel and the weight-gradient
// jobs read goes to a.sv ([tensor][B N][64], the layout of the N <= 512 training forward) at the point it exists in
// registers, MEAN and P through readout_act<true>.  The non-saving instances are unchanged by the parameter.
template <int NW, bool FW = false, int XW = 8, bool SAVE = false>
__global__ __launch_bounds__(64 * NW, 2) void mpnn_forward_large_kernel(MpnnArgs a, float* hbuf) {
  static_assert(XW == 8 || XW == 16, "observation rows are 8 or 16 floats");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ws_invalidate_key(a.call_maxdeg);  // hbuf overwrites the cached shared-graph tables
  const int lane = threadIdx.x & 63;
  const int w = uniform_i(threadIdx.x >> 6);
  const int e = blockIdx.x;
  const int N = a.N;
  const int rows_pad = (N + 15) & ~15;
  const int ntiles = rows_pad >> 4;
  const size_t R0 = (size_t)e * N;
  const size_t RT = (size_t)a.B * N;
  if constexpr (!SAVE) {  // the episode explores: the draw alone, no forward
    if (act_skip_block<NW>(a, e, 1, R0)) return;
  }
  // Linears on the exact bf16x3-split weight fragments streamed from L2 (no LDS weight staging: the
  // LDS holds only the readout scratch, so two episodes share a CU and hide each other's gathers)
  const uint16_t* BFP = reinterpret_cast<const uint16_t*>(a.P + PK_BF);
  float* Scr = lds;
  float* HA = hbuf + (size_t)e * rows_pad * 64 * 3;
  float* HB = HA + (size_t)rows_pad * 64;
  float* EB = HB + (size_t)rows_pad * 64;
  const float* P = a.P;
  const int s4 = lane >> 4;
  const int c16 = lane & 15;
  const int gid = a.gids[e];
  const uint32_t* __restrict__ eg = a.gs.edges + a.gs.edge_base[gid];
  const double* __restrict__ ewg = a.gs.edge_weights + a.gs.edge_base[gid];  // FW only
  const float* x = a.x + R0 * XW;
  auto rinfo = [&](int r) { return row_info_packed(pack_row_info(a, e, r, N)); };
  // w . x over features 8..15 of row r (wide rows)
  auto xdot_hi = [&](int r, const float (&wh)[8]) {
    const float4 x2 = f4(x + r * XW + 8), x3 = f4(x + r * XW + 12);
    return wh[0] * x2.x + wh[1] * x2.y + wh[2] * x2.z + wh[3] * x2.w + wh[4] * x3.x + wh[5] * x3.y + wh[6] * x3.z +
           wh[7] * x3.w;
  };

  // ---- phase A: Z = Wx . x into HB ----
  {
    float wx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wx[k] = P[PK_WX + lane * 8 + k];
    float wxh[8];
    if constexpr (XW == 16) {
#pragma unroll
      for (int k = 0; k < 8; ++k) wxh[k] = P[PK_WXH + lane * 8 + k];
    }
    for (int r = w; r < rows_pad; r += NW) {
      float z = 0.f;
      if (r < N) {
        const float4 x0 = f4(x + r * XW), x1 = f4(x + r * XW + 4);
        z = wx[0] * x0.x + wx[1] * x0.y + wx[2] * x0.z + wx[3] * x0.w + wx[4] * x1.x + wx[5] * x1.y +
            wx[6] * x1.z + wx[7] * x1.w;
        if constexpr (XW == 16) z = z + xdot_hi(r, wxh);
      }
      HB[(size_t)r * 64 + lane] = z;
    }
  }
  __threadfence();
  __syncthreads();
  // ---- phase B: edge embedding (mpnn.py:89-104) -> EB; phase C: h0 = relu(W0 . x) -> HA ----
  {
    const int maxdeg_call = a.norm_scope == ECO_NORM_PER_CALL ? *a.call_maxdeg : a.gs.max_deg[gid];
    float wa[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) wa[c * 4 + i] = P[PK_WA + 16 * c + 4 * s4 + i];
    for (int t = w; t < ntiles; t += NW) {
      const int r = t * 16 + c16;
      const bool valid = r < N;
      const RowInfo ri = rinfo(r);
      float4 acc[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = zero4();
      for_edges(eg, ri.e0, ri.e1, [&](uint32_t ex, int q) {
        const float wv = edge_wf<FW>(ex, ewg, q);
        const float* zr = HB + (size_t)edge_col(ex) * 64 + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 z = f4(zr + 16 * c);
          acc[c].x += relu(fmaf(wv, wa[4 * c + 0], z.x));
          acc[c].y += relu(fmaf(wv, wa[4 * c + 1], z.y));
          acc[c].z += relu(fmaf(wv, wa[4 * c + 2], z.z));
          acc[c].w += relu(fmaf(wv, wa[4 * c + 3], z.w));
        }
      });
      const float nf = (float)ri.norm;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[c].x = acc[c].x / nf; acc[c].y = acc[c].y / nf; acc[c].z = acc[c].z / nf; acc[c].w = acc[c].w / nf;
      }
      if (s4 == 3) acc[3].w = nf / (float)maxdeg_call;  // norm / norm.max() (mpnn.py:102)
      if (!valid) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = zero4();
      }
      if constexpr (SAVE) {
        if (valid) {
          float* ea = a.sv + (size_t)SV_EAGG * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(ea + 16 * c, acc[c]);
        }
      }
      f32x4 d[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      mm_bf3_lean(d, acc, BFP + BF_WF, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        st4(EB + (size_t)r * 64 + 16 * nt + 4 * s4, relu4(d[nt]));
        if constexpr (SAVE) {
          if (valid) st4(a.sv + (size_t)SV_E * RT * 64 + (R0 + r) * 64 + 16 * nt + 4 * s4, relu4(d[nt]));
        }
      }
    }
    float w0[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w0[k] = P[PK_W0 + lane * 8 + k];
    float w0h[8];
    if constexpr (XW == 16) {
#pragma unroll
      for (int k = 0; k < 8; ++k) w0h[k] = P[PK_W0H + lane * 8 + k];
    }
    for (int r = w; r < rows_pad; r += NW) {
      float h0 = 0.f;
      if (r < N) {
        const float4 x0 = f4(x + r * XW), x1 = f4(x + r * XW + 4);
        if constexpr (XW == 16)
          h0 = relu(w0[0] * x0.x + w0[1] * x0.y + w0[2] * x0.z + w0[3] * x0.w + w0[4] * x1.x + w0[5] * x1.y +
                    w0[6] * x1.z + w0[7] * x1.w + xdot_hi(r, w0h));
        else
          h0 = relu(w0[0] * x0.x + w0[1] * x0.y + w0[2] * x0.z + w0[3] * x0.w + w0[4] * x1.x + w0[5] * x1.y +
                    w0[6] * x1.z + w0[7] * x1.w);
      }
      HA[(size_t)r * 64 + lane] = h0;
      if constexpr (SAVE) {
        if (r < N) a.sv[(size_t)SV_H0 * RT * 64 + (R0 + r) * 64 + lane] = h0;
      }
    }
  }
  __threadfence();
  __syncthreads();
  // ---- phase D: 3 x UpdateNodeEmbeddingLayer (mpnn.py:114-120), HA <-> HB ----
  float* Hc = HA;
  float* Hn = HB;
  for (int layer = 0; layer < 3; ++layer) {
    const uint16_t* BFL = BFP + BF_LAYER + layer * BF_LAYER_STRIDE;  // message halves, then update halves
    for (int t = w; t < ntiles; t += NW) {
      const int r = t * 16 + c16;
      const bool valid = r < N;
      const RowInfo ri = rinfo(r);
      float4 am[4], ev[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) am[c] = zero4();
      for_edges(eg, ri.e0, ri.e1, [&](uint32_t ex, int q) {
        const float wv = edge_wf<FW>(ex, ewg, q);
        const float* hr = Hc + (size_t)edge_col(ex) * 64 + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 hv = f4(hr + 16 * c);
          am[c].x = fmaf(wv, hv.x, am[c].x);
          am[c].y = fmaf(wv, hv.y, am[c].y);
          am[c].z = fmaf(wv, hv.z, am[c].z);
          am[c].w = fmaf(wv, hv.w, am[c].w);
        }
      });
      const float nf = (float)ri.norm;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        am[c].x = am[c].x / nf; am[c].y = am[c].y / nf; am[c].z = am[c].z / nf; am[c].w = am[c].w / nf;
        ev[c] = f4(EB + (size_t)r * 64 + 16 * c + 4 * s4);
      }
      if constexpr (SAVE) {
        if (valid) {
          float* sa = a.sv + (size_t)(SV_AGG0 + layer) * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(sa + 16 * c, am[c]);
        }
      }
      f32x4 d[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      mm_bf3_lean(d, am, BFL, lane);             // message = relu(Wm . [agg, e])
      mm_bf3_lean(d, ev, BFL + BF_HALF, lane);
      float4 hc[4], mr[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        hc[c] = f4(Hc + (size_t)r * 64 + 16 * c + 4 * s4);
        mr[c] = relu4(d[c]);
      }
      if constexpr (SAVE) {
        if (valid) {
          float* sm = a.sv + (size_t)(SV_M0 + layer) * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) st4(sm + 16 * c, mr[c]);
        }
      }
      f32x4 hn[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) hn[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      mm_bf3_lean(hn, hc, BFL + 2 * BF_HALF, lane);  // h' = relu(Wu . [h, m])
      mm_bf3_lean(hn, mr, BFL + 3 * BF_HALF, lane);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) st4(Hn + (size_t)r * 64 + 16 * nt + 4 * s4, valid ? relu4(hn[nt]) : zero4());
      if constexpr (SAVE) {
        if (valid) {
          float* sh = a.sv + (size_t)(SV_H0 + layer + 1) * RT * 64 + (R0 + r) * 64 + 4 * s4;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) st4(sh + 16 * nt, relu4(hn[nt]));
        }
      }
    }
    __threadfence();  // release the Hn rows and invalidate this CU's L1 before other waves read them
    __syncthreads();  // every wave done with Hc; Hn complete
    float* tmp = Hc;
    Hc = Hn;
    Hn = tmp;
  }
  // ---- phase E: readout + act over the h3 rows in global memory ----
  readout_act<SAVE, NW>(a, Hc, 64, Scr, true, e, 1, N, R0, RT);
}

// norm.max() of the call (mpnn.py:102 over every graph of the batch): ONE workgroup reduces all B graph
// ids and writes the result (no zeroing memset, no atomics)
__global__ __launch_bounds__(1024) void call_maxdeg_kernel(const eco_graph_set gs, const int32_t* gids, int B,
                                                           int* out) {
  __shared__ int red[16];
  int m = 1;
  for (int i = threadIdx.x; i < B; i += blockDim.x) m = max(m, gs.max_deg[gids[i]]);
  m = wave_max_i(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    int r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = max(r, red[w]);
    *out = r;
  }
}

// Backward over global-memory rows (512 < N <= 2048): mpnn_backward_kernel restated for one workgroup per episode,
// the saved activations a.sv of mpnn_forward_large_kernel<.., SAVE = true> and the gradient workspace a.gr in the
// layout of mpnn_grad_ws_bytes (graphs_per_block is 1 here: one DWA row per episode).  Waves own 16-node tiles
// round-robin (t = w; t += NW), the same tiles in every phase, so a row of GR_DH or GR_DE is only ever read by the
// thread that wrote it.  What the LDS kernel keeps in its array G (the rows other waves gather from) is the
// episode's [rows_pad][64] buffer in gbuf, with the forward's fence + barrier pair between writing and gathering;
// dh lives in the GR_DH rows instead of per-tile registers.  The Linears are the bf16x3 transposed fragments from
// L2 (the WLDS = false branch).  No atomics: every reduction runs in a fixed order.
// LDS: DQ [rows_pad] | DMEAN [64] | RED [NW][64]
// DQCAP: the capacity of DQ, rows_pad at the largest N of the entry that launches the instance (eco_mpnn_grad_large:
// 2048; eco_mpnn_grad_wg: ECO_MAX_SPINS_WG, 32 KB more static LDS under the same one-workgroup-per-CU bound).
template <int NW, bool FW = false, int DQCAP = MPNN_MAX_SPINS_LARGE>
__global__ __launch_bounds__(64 * NW, 1) void mpnn_backward_large_kernel(MpnnArgs a, float* gbuf) {
  static_assert(DQCAP % 16 == 0, "DQ holds rows_pad entries");
  __shared__ float DQ[DQCAP];
  __shared__ float DMEAN[64];
  __shared__ float RED[NW * 64];
  constexpr int NT = 64 * NW;
  const int lane = threadIdx.x & 63;
  const int w = uniform_i(threadIdx.x >> 6);
  const int e = blockIdx.x;
  const int N = a.N;
  const int rows_pad = (N + 15) & ~15;
  const int ntiles = rows_pad >> 4;
  const size_t R0 = (size_t)e * N;
  const size_t RT = (size_t)a.B * N;
  float* G = gbuf + (size_t)e * rows_pad * 64;  // gathered-gradient source rows
  const float* P = a.P;
  const float* sv = a.sv;
  float* gr = a.gr;
  const int s4 = lane >> 4;
  const int c16 = lane & 15;
  const int gid = a.gids[e];
  const uint32_t* __restrict__ eg = a.gs.edges + a.gs.edge_base[gid];
  const double* __restrict__ ewg = a.gs.edge_weights + a.gs.edge_base[gid];  // FW only
  auto rinfo = [&](int r) { return row_info_packed(pack_row_info(a, e, r, N)); };
  auto SV = [&](int t) { return sv + (size_t)t * RT * 64; };
  auto GR = [&](int t) { return gr + (size_t)t * RT * 64; };
  const float* MEAN = sv + (size_t)SV_NODE_TENSORS * RT * 64;
  const float* PP = MEAN + (size_t)a.B * 64;
  float* DP = gr + (size_t)GR_NODE_TENSORS * RT * 64;
  float* DWRA = DP + (size_t)a.B * 64;
  float* DWRB = DWRA + (size_t)a.B * 64;
  float* DBR = DWRB + (size_t)a.B * 64;
  float* DWA = DBR + ((a.B + 63) & ~63);  // [B][64]
  const bool xwide = a.xw == 16;

  for (int r = threadIdx.x; r < rows_pad; r += NT) DQ[r] = r < N ? a.dq[R0 + r] : 0.f;
  __syncthreads();

  // ---- readout backward (mpnn.py:143-159): dWr[64:] = sum_v dq_v h3_v over all waves, the rest on wave 0 ----
  {
    const float* h3 = SV(SV_H3) + R0 * 64;
    float dwb = 0.f;
    for (int v = w; v < N; v += NW) {
      const float dv = DQ[v];
      if (dv != 0.f) dwb = fmaf(dv, h3[(size_t)v * 64 + lane], dwb);
    }
    RED[w * 64 + lane] = dwb;
  }
  __syncthreads();
  if (w == 0) {
    float s = 0.f;
    for (int v = lane; v < N; v += 64) s += DQ[v];
    const float S = wave_sum_f(s);
    const float p = PP[(size_t)e * 64 + lane];
    const float wr = P[PK_WR + lane];
    const float dp = wr * S * (p > 0.f ? 1.f : 0.f);
    DP[(size_t)e * 64 + lane] = dp;
    DWRA[(size_t)e * 64 + lane] = relu(p) * S;
    if (lane == 0) DBR[e] = S;
    float dmean = 0.f;
#pragma unroll 16
    for (int k = 0; k < 64; ++k) dmean = fmaf(P[PK_WP + k * 64 + lane], __shfl(dp, k, 64), dmean);
    DMEAN[lane] = dmean / (float)N;
    float dwb = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) dwb += RED[k * 64 + lane];  // fixed order
    DWRB[(size_t)e * 64 + lane] = dwb;
  }
  __syncthreads();

  // dh3 (A layout): dq_i * wr[64+f] + dmean_f / N  -> GR_DH rows
  for (int t = w; t < ntiles; t += NW) {
    const int r = t * 16 + c16;
    if (r < N) {
      const float dqi = DQ[r];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int f = 16 * c + 4 * s4;
        const float4 dm = f4(DMEAN + f);
        st4(GR(GR_DH) + (R0 + r) * 64 + f,
            make_float4(fmaf(dqi, P[PK_WR + 64 + f + 0], dm.x), fmaf(dqi, P[PK_WR + 64 + f + 1], dm.y),
                        fmaf(dqi, P[PK_WR + 64 + f + 2], dm.z), fmaf(dqi, P[PK_WR + 64 + f + 3], dm.w)));
      }
    }
  }

  // ---- update layers in reverse (mpnn.py:114-120) ----
  const uint16_t* BFP = reinterpret_cast<const uint16_t*>(P + PK_BF);
  for (int layer = 2; layer >= 0; --layer) {
    const uint16_t* BFT = BFP + BFT_LAYER + layer * BF_LAYER_STRIDE;  // Wm^T halves, then Wu^T halves
    for (int t = w; t < ntiles; t += NW) {
      const int r = t * 16 + c16;
      const bool valid = r < N;
      const size_t ro = (R0 + r) * 64 + 4 * s4;
      // duu = dh' * [h' > 0]
      float4 duu[4], mv[4];
      const float* hnext = SV(SV_H0 + layer + 1) + ro;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 hv = valid ? f4(hnext + 16 * c) : zero4();
        const float4 dhv = valid ? f4(GR(GR_DH) + ro + 16 * c) : zero4();
        mv[c] = valid ? f4(SV(SV_M0 + layer) + ro + 16 * c) : zero4();
        duu[c] = make_float4(hv.x > 0.f ? dhv.x : 0.f, hv.y > 0.f ? dhv.y : 0.f, hv.z > 0.f ? dhv.z : 0.f,
                             hv.w > 0.f ? dhv.w : 0.f);
        if (valid) st4(GR(GR_DUU0 + layer) + ro + 16 * c, duu[c]);
      }
      // [dh_direct, dm] = duu . Wu
      f32x4 d8[8];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) d8[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf3_t2(d8, duu, BFT + 2 * BF_HALF, lane);
      // dum = dm * [m > 0]
      float4 dum[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dum[c] = make_float4(mv[c].x > 0.f ? d8[4 + c][0] : 0.f, mv[c].y > 0.f ? d8[4 + c][1] : 0.f,
                             mv[c].z > 0.f ? d8[4 + c][2] : 0.f, mv[c].w > 0.f ? d8[4 + c][3] : 0.f);
        if (valid) {
          st4(GR(GR_DUM0 + layer) + ro + 16 * c, dum[c]);
          st4(GR(GR_DH) + ro + 16 * c, make_float4(d8[c][0], d8[c][1], d8[c][2], d8[c][3]));
        }
      }
      // [dagg, de] = dum . Wm;  G rows <- dagg / norm  (d(agg)/d(A.h) = 1/norm)
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) d8[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf3_t2(d8, dum, BFT, lane);
      const float nf = (float)rinfo(r).norm;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        st4(G + (size_t)r * 64 + 16 * c + 4 * s4,
            valid ? make_float4(d8[c][0] / nf, d8[c][1] / nf, d8[c][2] / nf, d8[c][3] / nf) : zero4());
        if (valid) {
          float* de = GR(GR_DE) + ro + 16 * c;
          const float4 prev = layer == 2 ? zero4() : f4(de);
          st4(de, make_float4(prev.x + d8[4 + c][0], prev.y + d8[4 + c][1], prev.z + d8[4 + c][2],
                              prev.w + d8[4 + c][3]));
        }
      }
    }
    __threadfence();  // release the G rows and invalidate this CU's L1 before other waves gather them
    __syncthreads();
    // dh_l = dh_direct + A^T . (dagg / norm)   (A symmetric: a gather over the node's own row)
    for (int t = w; t < ntiles; t += NW) {
      const int r = t * 16 + c16;
      if (r < N) {
        const RowInfo ri = rinfo(r);
        float* dhp = GR(GR_DH) + (R0 + r) * 64 + 4 * s4;
        float4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f4(dhp + 16 * c);
        for_edges(eg, ri.e0, ri.e1, [&](uint32_t ex, int q) {
          const float wv = edge_wf<FW>(ex, ewg, q);
          const float* gv = G + (size_t)edge_col(ex) * 64 + 4 * s4;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float4 hv = f4(gv + 16 * c);
            acc[c].x = fmaf(wv, hv.x, acc[c].x);
            acc[c].y = fmaf(wv, hv.y, acc[c].y);
            acc[c].z = fmaf(wv, hv.z, acc[c].z);
            acc[c].w = fmaf(wv, hv.w, acc[c].w);
          }
        });
#pragma unroll
        for (int c = 0; c < 4; ++c) st4(dhp + 16 * c, acc[c]);
      }
    }
    __syncthreads();  // every wave done gathering before the next phase rewrites G
  }

  // ---- h0 = relu(W0.x): du0;  edge embedding (mpnn.py:89-104): due, G rows <- dEagg / norm ----
  for (int t = w; t < ntiles; t += NW) {
    const int r = t * 16 + c16;
    const bool valid = r < N;
    float4 due[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t off = (R0 + r) * 64 + 16 * c + 4 * s4;
      if (valid) {
        const float4 hv = f4(SV(SV_H0) + off);
        const float4 dhv = f4(GR(GR_DH) + off);
        st4(GR(GR_DU0) + off, make_float4(hv.x > 0.f ? dhv.x : 0.f, hv.y > 0.f ? dhv.y : 0.f,
                                          hv.z > 0.f ? dhv.z : 0.f, hv.w > 0.f ? dhv.w : 0.f));
      }
      const float4 ev = valid ? f4(SV(SV_E) + off) : zero4();
      const float4 dv = valid ? f4(GR(GR_DE) + off) : zero4();
      due[c] = make_float4(ev.x > 0.f ? dv.x : 0.f, ev.y > 0.f ? dv.y : 0.f, ev.z > 0.f ? dv.z : 0.f,
                           ev.w > 0.f ? dv.w : 0.f);
      if (valid) st4(GR(GR_DUE) + off, due[c]);
    }
    f32x4 d4[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) d4[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    mm_bf3_lean(d4, due, BFP + BFT_WF, lane);
    const float nf = (float)rinfo(r).norm;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      st4(G + (size_t)r * 64 + 16 * c + 4 * s4,
          valid ? make_float4(d4[c][0] / nf, d4[c][1] / nf, d4[c][2] / nf, d4[c][3] / nf) : zero4());
  }
  __threadfence();
  __syncthreads();
  // dz_j = sum_{i in N(j)} G_i * [w_ij wa + z_j > 0];  dwa += same * w_ij
  {
    float wa[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) wa[4 * c + i] = P[PK_WA + 16 * c + 4 * s4 + i];
    float dwa[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) dwa[i] = 0.f;
    for (int t = w; t < ntiles; t += NW) {
      const int r = t * 16 + c16;
      const bool valid = r < N;
      const RowInfo ri = rinfo(r);
      // z = Wx.x of the lane's node for its 16 features (same expression as forward phase A)
      float4 x0 = zero4(), x1 = zero4(), x2 = zero4(), x3 = zero4();
      if (valid) {
        const float* xr = a.x + (R0 + r) * a.xw;
        x0 = f4(xr);
        x1 = f4(xr + 4);
        if (xwide) { x2 = f4(xr + 8); x3 = f4(xr + 12); }
      }
      float z[16], dz[16];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float* wx = P + PK_WX + (16 * c + 4 * s4 + i) * 8;
          const float4 w0 = f4(wx), w1 = f4(wx + 4);
          z[4 * c + i] = w0.x * x0.x + w0.y * x0.y + w0.z * x0.z + w0.w * x0.w + w1.x * x1.x + w1.y * x1.y +
                         w1.z * x1.z + w1.w * x1.w;
          if (xwide) {  // same left-to-right order as the forward's xdot_hi term
            const float* wh = P + PK_WXH + (16 * c + 4 * s4 + i) * 8;
            const float4 h0 = f4(wh), h1 = f4(wh + 4);
            z[4 * c + i] += h0.x * x2.x + h0.y * x2.y + h0.z * x2.z + h0.w * x2.w + h1.x * x3.x + h1.y * x3.y +
                            h1.z * x3.z + h1.w * x3.w;
          }
        }
#pragma unroll
      for (int i = 0; i < 16; ++i) dz[i] = 0.f;
      for_edges(eg, ri.e0, ri.e1, [&](uint32_t ex, int q) {
        const float wv = edge_wf<FW>(ex, ewg, q);
        const float* gi = G + (size_t)edge_col(ex) * 64 + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 gv = f4(gi + 16 * c);
          const float g4[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int kk = 4 * c + i;
            const float gm = fmaf(wv, wa[kk], z[kk]) > 0.f ? g4[i] : 0.f;
            dz[kk] += gm;
            dwa[kk] = fmaf(gm, wv, dwa[kk]);
          }
        }
      });
      if (valid) {
        float* dzp = GR(GR_DZ) + (R0 + r) * 64 + 4 * s4;
#pragma unroll
        for (int c = 0; c < 4; ++c) st4(dzp + 16 * c, make_float4(dz[4 * c], dz[4 * c + 1], dz[4 * c + 2], dz[4 * c + 3]));
      }
    }
    // reduce dwa over the 16 node lanes sharing s4, then over waves (fixed order)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = dwa[i];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      dwa[i] = v;
    }
    if (c16 == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) RED[w * 64 + 16 * c + 4 * s4 + i] = dwa[4 * c + i];
    }
    __syncthreads();
    if (w == 0) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) s += RED[k * 64 + lane];
      DWA[(size_t)e * 64 + lane] = s;
    }
  }
}

// The MpnnArgs fields every launch fills the same way; the rest stay zero for the caller.  graphs_per_block is 1 from
// 208 vertices on, so on every global-row size.
static void fill_args(MpnnArgs& a, const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                      const int32_t* graph_ids, int32_t batch, const float* obs_x, int32_t norm_scope) {
  a = MpnnArgs{};
  a.P = packed; a.gs = *gs; a.gids = graph_ids; a.B = batch; a.N = gs->n_spins;
  a.gpb = graphs_per_block(a.N, batch);
  a.nobs = n_obs_in; a.xw = ECO_OBS_X_STRIDE(n_obs_in); a.x = obs_x; a.norm_scope = norm_scope;
  a.err = err_word();
}

// max_spins: MPNN_MAX_SPINS_LARGE but for eco_mpnn_forward_wg, which has checked its own range
static int prepare(MpnnArgs& a, const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                   const int32_t* graph_ids, int32_t batch, const float* obs_x, int32_t norm_scope,
                   int max_spins = MPNN_MAX_SPINS_LARGE) {
  if (!packed || !gs || !graph_ids || !obs_x) return fail(ECO_ERR_ARG, "null argument");
  if (n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS) return fail(ECO_ERR_ARG, "n_obs_in out of range [1, 16]");
  if (batch < 1) return fail(ECO_ERR_ARG, "batch must be >= 1");
  if (gs->n_spins < 1 || gs->n_spins > max_spins) return fail(ECO_ERR_ARG, "mpnn supports 1 <= N <= 2048");
  if (norm_scope != ECO_NORM_PER_GRAPH && norm_scope != ECO_NORM_PER_CALL)
    return fail(ECO_ERR_ARG, "bad norm_scope");
  // a float-weighted set runs the CSR-gather kernels only: unit_weights == 0 keeps it off the dense, DL, shared-graph
  // and fused-pair kernels (dense_eligible, dl_eligible and the shared-graph test all need unit_weights)
  if (gs->edge_weights && gs->unit_weights)
    return fail(ECO_ERR_ARG, "graph set has float edge_weights and unit_weights set");
  fill_args(a, packed, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope);
  return ECO_OK;
}

}  // namespace eco

using namespace eco;

#ifdef ECO_PHASE_TIMING
extern "C" int eco_debug_phase_ts(unsigned long long* host, int32_t n) {
  if (n > ECO_TS_BLOCKS * 32) n = ECO_TS_BLOCKS * 32;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(eco_phase_ts), n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" size_t eco_mpnn_param_count(int32_t n_obs_in) {
  if (n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS) return 0;
  return (size_t)flat_offsets(n_obs_in).total;
}

extern "C" size_t eco_mpnn_packed_count(void) { return (size_t)PK_TOTAL; }

extern "C" int eco_mpnn_pack(const float* params, int32_t n_obs_in, float* packed, eco_stream_t stream) {
  if (!params || !packed) return fail(ECO_ERR_ARG, "null params/packed");
  if (n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS) return fail(ECO_ERR_ARG, "n_obs_in out of range [1, 16]");
  pack_scale_kernel<<<FH_NMAT, PS_THREADS, 0, (hipStream_t)stream>>>(params, n_obs_in, packed);
  pack_kernel<<<(PK_TOTAL + 255) / 256, 256, 0, (hipStream_t)stream>>>(params, n_obs_in, packed);
  return check_launch("mpnn_pack");
}

extern "C" size_t eco_mpnn_workspace_bytes(int32_t n_spins, int32_t batch) {
  if (n_spins < 1 || batch < 1) return 0;
  if (n_spins > MPNN_MAX_SPINS) {  // + per episode Z/h ping-pong rows and e rows (mpnn_forward_large_kernel),
                                  // or the node-major buffers of the shared-graph path, whichever is larger
    const size_t per_ep = rows_buffer_bytes(n_spins, batch, 3);
    const size_t shared = shared_ws_bytes(n_spins, batch);
    return 256 + (per_ep > shared ? per_ep : shared);
  }
  if (n_spins > DN_MAX_ROWS)  // + the edge embeddings of the dense kernels for 224 < N <= 512
    return 256 + (size_t)batch * n_spins * 64 * sizeof(float);
  return 256;  // the call-scope norm.max() slot
}

extern "C" size_t eco_mpnn_saved_bytes(int32_t n_spins, int32_t batch) {
  if (n_spins < 1 || batch < 1) return 0;
  const size_t RT = (size_t)n_spins * batch;
  return sv_mask_offset_floats(RT, batch) * sizeof(float) + RT * 4 * SM_TENSORS * sizeof(uint16_t);
}

static std::atomic<int> g_kernel_paths{0};
int eco::kernel_paths() { return g_kernel_paths.load(std::memory_order_relaxed); }

extern "C" int32_t eco_set_kernel_paths(int32_t mask) {
  return g_kernel_paths.exchange(mask & (ECO_PATH_NO_DENSE | ECO_PATH_NO_DL | ECO_PATH_NO_SHARED | ECO_PATH_NO_PAIR |
                                         ECO_PATH_DENSE2_FWD | ECO_PATH_NO_ACT_SKIP));
}

// The kernel family of one MPNN call (ECO_ROUTE_* of include/eco_hip.h).  The forward, the pair forward and the
// backward all ask here, and nowhere else are the eligibility predicates and the family bits of ECO_PATH_* read: a
// training forward writes `saved` in the layout of the family named here, and the backward finds the family that
// reads it by the same call.  Pure: a function of a.gs (scalar fields, pointer null-ness), a.N, a.gpb, a.xw and
// the two other arguments.  training: the call writes or reads saved activations (training forward, backward),
// which no family has above MPNN_MAX_SPINS vertices: ECO_ROUTE_NONE there, and the caller names the limit.
static int mpnn_route(const MpnnArgs& a, int paths, bool training) {
  const eco_graph_set* gs = &a.gs;
  const bool rows8 = a.xw == 8;  // the dense-aggregation families take 8-float observation rows
  if (rows8 && dense_eligible(gs, a.gpb) && !(paths & ECO_PATH_NO_DENSE))
    return (paths & ECO_PATH_DENSE2_FWD) ? ECO_ROUTE_DENSE2 : ECO_ROUTE_DENSE3;
  if (rows8 && dl_eligible(gs, a.gpb) && !(paths & (ECO_PATH_NO_DL | ECO_PATH_NO_DENSE))) return ECO_ROUTE_DL;
  if (a.N <= MPNN_MAX_SPINS) return ECO_ROUTE_CSR;
  if (training) return ECO_ROUTE_NONE;  // global-memory embeddings: inference only
  // one graph shared by every episode (GSet best-cut search): node-major episode-batched kernels
  if (gs->n_graphs == 1 && gs->unit_weights && !(paths & ECO_PATH_NO_SHARED)) return ECO_ROUTE_SHARED;
  return ECO_ROUTE_LARGE;
}

// eco_mpnn_forward_pair runs both networks in ONE launch on one-graph dense blocks with a prepared gs.adjbits;
// any other pair call is two single forwards of `family`
static bool pair_fused(const MpnnArgs& a, int family, int paths) {
  return (family == ECO_ROUTE_DENSE3 || family == ECO_ROUTE_DENSE2) && a.gpb == 1 && a.gs.adjbits &&
         !(paths & ECO_PATH_NO_PAIR);
}

// Whether the blocks of a single forward whose graphs all drew "explore" return before their forward
// (act_skip_block): only where the actions are the launch's one output -- no Q, no saved activations -- and a draw
// can say "explore" at all (epsilon > 0: the greedy calls of the evaluator, the solvers and the train step never
// skip).  The shared-graph family runs every episode through common launches and has no per-episode forward to skip.
static bool act_skips(const MpnnArgs& a, int family, int paths, bool save) {
  return a.has_act && !a.q && !save && a.act.epsilon > 0.f && family != ECO_ROUTE_SHARED && family != ECO_ROUTE_NONE &&
         !(paths & ECO_PATH_NO_ACT_SKIP);
}

extern "C" int32_t eco_mpnn_route(const eco_graph_set* gs, int32_t n_obs_in, int32_t batch, int32_t gpb,
                                  int32_t training, int32_t pair) {
  // a call that prepare() rejects has no route
  if (!gs || n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS || batch < 1 || gs->n_spins < 1 ||
      gs->n_spins > MPNN_MAX_SPINS_LARGE || (gs->edge_weights && gs->unit_weights))
    return ECO_ROUTE_NONE;
  MpnnArgs a{};
  a.gs = *gs; a.B = batch; a.N = gs->n_spins; a.gpb = gpb > 0 ? gpb : graphs_per_block(a.N, batch);
  a.xw = ECO_OBS_X_STRIDE(n_obs_in);
  const int paths = kernel_paths();
  const int family = mpnn_route(a, paths, training && !pair);  // the pair forward never saves
  return pair && pair_fused(a, family, paths) ? family | ECO_ROUTE_PAIR_FUSED : family;
}

// The CSR-gather instantiation of a block: the kernels' MAXT (tiles per wave they are unrolled for; 0: the block
// is too large for any), waves per workgroup, weights staged in LDS or streamed from L2, dynamic LDS bytes.
struct KCfg {
  int mt, nw;
  bool wlds;
  size_t lds;
};
constexpr size_t LDS_MAX = 160 * 1024;

static size_t lds_bytes(int rows_pad, int gpb, int nw, bool wlds, bool backward) {
  size_t f = (size_t)rows_pad * LDH;
  if (backward) {
    if (wlds) f += (size_t)2 * 128 * LDH + (size_t)rows_pad * 8;  // Wu^T, Wm^T + x rows
    f += (size_t)rows_pad * 2 + 2 * (size_t)gpb;               // packed row info + per-graph edge base
    f += (size_t)gpb * 64 + (size_t)(gpb < nw ? gpb : 1) * nw * 64 + 64;  // + tile schedule
  } else {
    if (wlds) f += (size_t)2 * 64 * LDW;
    f += (size_t)fwd_mreg_floats(rows_pad, gpb, nw, wlds);
    f += (size_t)rows_pad * 2 + 3 * (size_t)gpb + 2 + 64;  // row info, edge base, max degree, tile schedule
  }
  return f * sizeof(float);
}

// 16 waves x 1 tile (forward) or 8 waves x 2 or 4 tiles with LDS-staged weights when the block fits, else weights
// from L2.
static KCfg pick_cfg(int N, int gpb, bool backward) {
  const int rows_pad = (gpb * N + 15) & ~15;
  const int ntiles = rows_pad / 16;
  auto cfg = [&](int nw, bool wlds) { return KCfg{0, nw, wlds, lds_bytes(rows_pad, gpb, nw, wlds, backward)}; };
  auto tiles = [&](int nw) { return (ntiles + nw - 1) / nw; };  // per wave
  for (int nw : {16, 8, 4}) {
    if (backward && nw == 16) continue;  // the backward's 8-wide weight fragments need > 128 VGPRs
    KCfg c = cfg(nw, true);
    if (c.lds <= LDS_MAX && tiles(nw) <= (nw == 16 ? 1 : 4)) {
      c.mt = nw == 16 ? 1 : (nw == 8 && tiles(nw) <= 2 ? 2 : 4);
      return c;
    }
  }
  // weights from L2, 8 waves (2 per SIMD: the block owns the CU through its LDS) when 4 tiles per
  // wave suffice; measured at BA-500: forward 15 % faster than 4 waves x 8 tiles, backward slower
  KCfg c = cfg(8, false);
  if (c.lds <= LDS_MAX && tiles(8) <= 4) {
    c.mt = 4;
    return c;
  }
  c = cfg(4, false);
  c.mt = tiles(4) <= 4 ? 4 : (tiles(4) <= 8 ? 8 : 0);
  return c;
}

// one launch of a kernel with dynamic LDS: its size attribute, then the kernel
template <class... Args>
static void launch_lds(void (*kern)(Args...), int blocks, int threads, size_t lds, hipStream_t st, Args... args) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<blocks, threads, lds, st>>>(args...);
}

// One row of the CSR-gather table: the forward (saving or not) or the backward of shape (MT, NW, WLDS); fw: the
// float-weighted instances.  The 16-wave shape has no backward (pick_cfg never returns it for one).
template <int MT, int NW, bool WL>
static void launch_csr_row(const KCfg& k, const MpnnArgs& a, bool backward, bool save, hipStream_t st) {
  const int blocks = (a.B + a.gpb - 1) / a.gpb;
  const bool fw = a.gs.edge_weights != nullptr;
  if (!backward) {
    if (fw && save) launch_lds(mpnn_forward_kernel<MT, true, NW, WL, true>, blocks, 64 * NW, k.lds, st, a);
    else if (fw) launch_lds(mpnn_forward_kernel<MT, false, NW, WL, true>, blocks, 64 * NW, k.lds, st, a);
    else if (save) launch_lds(mpnn_forward_kernel<MT, true, NW, WL, false>, blocks, 64 * NW, k.lds, st, a);
    else launch_lds(mpnn_forward_kernel<MT, false, NW, WL, false>, blocks, 64 * NW, k.lds, st, a);
  } else if constexpr (NW != 16) {
    if (fw) launch_lds(mpnn_backward_kernel<MT, NW, WL, true>, blocks, 64 * NW, k.lds, st, a);
    else launch_lds(mpnn_backward_kernel<MT, NW, WL, false>, blocks, 64 * NW, k.lds, st, a);
  }
}

// The CSR-gather launch of a call: the block configuration of pick_cfg, then its row of the table.
constexpr int cfg_key(int mt, int nw, bool wlds) { return mt * 64 + nw * 2 + (wlds ? 1 : 0); }
static int launch_csr(const MpnnArgs& a, bool backward, bool save, hipStream_t st) {
  const KCfg k = pick_cfg(a.N, a.gpb, backward);
  if (k.lds > LDS_MAX) return fail(ECO_ERR_ARG, "graph block exceeds the LDS budget");
  switch (cfg_key(k.mt, k.nw, k.wlds)) {
    case cfg_key(1, 16, true): launch_csr_row<1, 16, true>(k, a, backward, save, st); break;
    case cfg_key(2, 8, true): launch_csr_row<2, 8, true>(k, a, backward, save, st); break;
    case cfg_key(4, 8, true): launch_csr_row<4, 8, true>(k, a, backward, save, st); break;
    case cfg_key(4, 4, true): launch_csr_row<4, 4, true>(k, a, backward, save, st); break;
    case cfg_key(4, 8, false): launch_csr_row<4, 8, false>(k, a, backward, save, st); break;
    case cfg_key(4, 4, false): launch_csr_row<4, 4, false>(k, a, backward, save, st); break;
    case cfg_key(8, 4, false): launch_csr_row<8, 4, false>(k, a, backward, save, st); break;
    default: return fail(ECO_ERR_ARG, "graph block too large");
  }
  return check_launch(backward ? "mpnn_backward" : "mpnn_forward");
}

// The per-episode global-memory forward, one workgroup of 8 waves per episode with its three row buffers in hbuf:
// the instance of {float weights} x {8-, 16-float rows (more than 8 observables)} x {saving}.
static void launch_forward_large(const MpnnArgs& a, float* hbuf, bool save, hipStream_t st) {
  const int rows_pad = (a.N + 15) & ~15;
  const size_t lds = (size_t)readout_scratch_floats(rows_pad, 1, 8, true) * sizeof(float);
  static void (*const table[2][2][2])(MpnnArgs, float*) = {
      {{mpnn_forward_large_kernel<8, false, 8, false>, mpnn_forward_large_kernel<8, false, 8, true>},
       {mpnn_forward_large_kernel<8, false, 16, false>, mpnn_forward_large_kernel<8, false, 16, true>}},
      {{mpnn_forward_large_kernel<8, true, 8, false>, mpnn_forward_large_kernel<8, true, 8, true>},
       {mpnn_forward_large_kernel<8, true, 16, false>, mpnn_forward_large_kernel<8, true, 16, true>}}};
  launch_lds(table[a.gs.edge_weights != nullptr][a.xw == 16][save], a.B, 512, lds, st, a, hbuf);
}

// N > 512 inference: the non-saving forward on the row buffers after the workspace header
static int launch_large(const MpnnArgs& a, void* workspace, hipStream_t st) {
  launch_forward_large(a, (float*)((char*)workspace + 256), false, st);
  return check_launch("mpnn_forward_large");
}

// One network of a forward call: its packed weights and where its Q values / actions go.
struct FwdHead {
  const float* packed;
  float* q;
  const eco_act_config* act;
  int32_t* actions;
};

// Per-call set-up of eco_mpnn_forward, eco_mpnn_forward_wg (n = 1) and eco_mpnn_forward_pair (n = 2): folds
// ECO_NORM_PER_CALL_REUSE (the workspace already holds the call's max degree) into PER_CALL, validates, fills
// a[0 .. n) (which differ in P, q, act and actions only) and routes the call.  Unless a pair call falls back to two
// single forwards (fused false: nothing is launched, they do their own set-up), the call's norm.max() reduction is
// launched here.  wg: the call is eco_mpnn_forward_wg's, which has checked its range and runs ECO_ROUTE_LARGE alone.
static int forward_setup(MpnnArgs* a, const FwdHead* h, int n, int32_t n_obs_in, const eco_graph_set* gs,
                         const int32_t* graph_ids, int32_t batch, const float* obs_x, int32_t norm_scope, void* saved,
                         void* workspace, hipStream_t st, int& family, bool& fused, bool wg = false) {
  const bool reuse_maxdeg = norm_scope == ECO_NORM_PER_CALL_REUSE;
  if (reuse_maxdeg) norm_scope = ECO_NORM_PER_CALL;
  if (const int rc = prepare(a[0], h[0].packed, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope,
                             wg ? kRowsWg.hi : MPNN_MAX_SPINS_LARGE))
    return rc;
  if (!workspace) return fail(ECO_ERR_ARG, "null workspace");
  for (int i = 0; i < n; ++i)
    if (h[i].act && !h[i].actions) return fail(ECO_ERR_ARG, "act config without actions buffer");
  for (int i = 0; i < n; ++i)
    if (!h[i].q && !h[i].act) return fail(ECO_ERR_ARG, "nothing to compute (q and act both null)");
  a[0].call_maxdeg = (int*)workspace;
  a[0].sv = (float*)saved;
  for (int i = n - 1; i >= 0; --i) {
    a[i] = a[0];
    a[i].P = h[i].packed;
    a[i].q = h[i].q;
    a[i].has_act = h[i].act != nullptr;
    if (h[i].act) a[i].act = *h[i].act;
    a[i].actions = h[i].actions;
  }
  const int paths = kernel_paths();
  family = wg ? ECO_ROUTE_LARGE : mpnn_route(a[0], paths, saved != nullptr);
  fused = n == 2 && pair_fused(a[0], family, paths);
  if (n == 2 && !fused) return ECO_OK;
  if (n == 1) a[0].act_skip = act_skips(a[0], family, paths, saved != nullptr);  // the pair kernels never skip
  if (norm_scope == ECO_NORM_PER_CALL && !reuse_maxdeg)
    call_maxdeg_kernel<<<1, 1024, 0, st>>>(*gs, graph_ids, batch, (int*)workspace);
  return ECO_OK;
}

extern "C" int eco_mpnn_forward_pair(const float* packed_a, const float* packed_b, int32_t n_obs_in,
                                     const eco_graph_set* gs, const int32_t* graph_ids, int32_t batch,
                                     const float* obs_x, int32_t norm_scope, float* q_a, const eco_act_config* act_a,
                                     int32_t* actions_a, float* q_b, const eco_act_config* act_b, int32_t* actions_b,
                                     void* workspace, eco_stream_t stream) {
  if (!packed_b) return fail(ECO_ERR_ARG, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const FwdHead h[2] = {{packed_a, q_a, act_a, actions_a}, {packed_b, q_b, act_b, actions_b}};
  MpnnArgs a[2];
  int family;
  bool fused;
  if (const int rc = forward_setup(a, h, 2, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope, nullptr, workspace, st,
                                   family, fused))
    return rc;
  if (!fused) {  // the second forward reuses the first one's call-scope max degree
    if (const int rc = eco_mpnn_forward(packed_a, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope, q_a, act_a,
                                        actions_a, nullptr, workspace, stream))
      return rc;
    return eco_mpnn_forward(packed_b, n_obs_in, gs, graph_ids, batch, obs_x,
                            norm_scope == ECO_NORM_PER_GRAPH ? norm_scope : ECO_NORM_PER_CALL_REUSE, q_b, act_b,
                            actions_b, nullptr, workspace, stream);
  }
  if (family == ECO_ROUTE_DENSE2) return mpnn_forward_dense2_pair_launch(a[0], a[1], st);
  return mpnn_forward_dense3_pair_launch(a[0], a[1], st);
}

extern "C" int eco_mpnn_forward(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                                const int32_t* graph_ids, int32_t batch, const float* obs_x, int32_t norm_scope,
                                float* q, const eco_act_config* act, int32_t* actions, void* saved, void* workspace,
                                eco_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  const FwdHead h = {packed, q, act, actions};
  MpnnArgs a;
  int family;
  bool fused;
  if (const int rc = forward_setup(&a, &h, 1, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope, saved, workspace, st,
                                   family, fused))
    return rc;
  const bool save = saved != nullptr;
  switch (family) {
    case ECO_ROUTE_DENSE3: return mpnn_forward_dense3_launch(a, save, st);
    case ECO_ROUTE_DENSE2: return mpnn_forward_dense2_launch(a, save, st);
    case ECO_ROUTE_DL: return mpnn_forward_dl_launch(a, save, workspace, st);
    case ECO_ROUTE_SHARED: return mpnn_forward_shared_launch(a, workspace, st);
    case ECO_ROUTE_LARGE: return launch_large(a, workspace, st);
    case ECO_ROUTE_CSR: return launch_csr(a, false, save, st);
    default: return fail(ECO_ERR_ARG, "training forward (saved activations) supports N <= 512");
  }
}

// ---- inference above MPNN_MAX_SPINS_LARGE vertices: a self-contained entry on mpnn_forward_large_kernel ----
// The kernel keeps an episode's rows in global memory and walks them in loops bounded by N alone, so it runs
// 2048 < N <= ECO_MAX_SPINS_WG unchanged (DESIGN section 22 has the audit: pack_row_info's 16-bit row length and
// 15-bit norm hold up to 32767 neighbours; the readout scratch is 512 + 4 + rows_pad floats = 34.8 KB at 8192; every
// episode offset into the workspace, obs_x and q is a size_t product; per-episode row offsets r * 64 stay below
// 2^19).  eco_mpnn_forward and eco_mpnn_route keep their range: this entry has its own workspace layout -- the
// 256 B header (call max degree; the shared-graph key slot, zeroed by the kernel) and three [rows_pad][64] f32 row
// buffers per episode -- and never takes the shared-graph path, whose tables are one LDS block.

// What every entry of a global-row range asks of its graph set and sizes; what differs between the two ranges is in
// the RowsRange descriptor (eco_mpnn.h).
int eco::mpnn_rows_check(const RowsRange& r, const char* kind, const eco_graph_set* gs, int32_t n_obs_in,
                         int32_t batch) {
  auto no = [&](const std::string& reason) { return fail(ECO_ERR_ARG, rows_message(r, kind, reason)); };
  if (!gs->row_ptr || !gs->edge_base || !gs->edges || !gs->deg || !gs->max_deg) return no("incomplete graph set");
  if (!rows_in_range(r, gs->n_spins)) return no("got N = " + std::to_string(gs->n_spins));
  if (n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS) return no("n_obs_in out of range [1, 16]");
  if (batch < 1) return no("batch must be >= 1");
  if (gs->n_graphs < 1) return no("empty graph set");
  if (gs->edge_weights && !r.float_weights)
    return no("integer weights only (float-weighted sets run up to " + std::to_string(kRowsLarge.hi) + " vertices)");
  if (gs->edge_weights && gs->unit_weights) return no("graph set has float edge_weights and unit_weights set");
  return ECO_OK;
}

extern "C" size_t eco_mpnn_forward_wg_workspace_bytes(int32_t n_spins, int32_t batch, int32_t n_obs_in) {
  if (!rows_in_range(kRowsWg, n_spins) || batch < 1 || n_obs_in < 1 || n_obs_in > ECO_MPNN_MAX_OBS) return 0;
  if ((size_t)batch * padded_rows(n_spins) > (size_t)INT32_MAX / 64) return 0;  // the 32-bit row index
  return 256 + rows_buffer_bytes(n_spins, batch, 3);
}

extern "C" int eco_mpnn_forward_wg(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                                   const int32_t* graph_ids, int32_t batch, const float* obs_x, int32_t norm_scope,
                                   float* q, const eco_act_config* act, int32_t* actions, void* workspace,
                                   eco_stream_t stream) {
  if (!packed || !gs || !graph_ids || !obs_x || !workspace)
    return fail(ECO_ERR_ARG, rows_message(kRowsWg, "forward", "null argument"));
  if (const int rc = mpnn_rows_check(kRowsWg, "forward", gs, n_obs_in, batch)) return rc;
  if (eco_mpnn_forward_wg_workspace_bytes(gs->n_spins, batch, n_obs_in) == 0)
    return fail(ECO_ERR_ARG, rows_message(kRowsWg, "forward",
                                          "batch * rows beyond the 32-bit row index ((2^31 - 1) / 64)"));
  hipStream_t st = (hipStream_t)stream;
  const FwdHead h = {packed, q, act, actions};
  MpnnArgs a;
  int family;
  bool fused;
  if (const int rc = forward_setup(&a, &h, 1, n_obs_in, gs, graph_ids, batch, obs_x, norm_scope, nullptr, workspace,
                                   st, family, fused, true))
    return rc;
  return launch_large(a, workspace, st);
}

size_t eco::mpnn_grad_ws_bytes(int32_t n_spins, int32_t batch) {
  if (n_spins < 1 || batch < 1) return 0;
  const int gpb = graphs_per_block(n_spins, batch);
  const size_t nblk = (batch + gpb - 1) / gpb;
  return ((size_t)GR_NODE_TENSORS * n_spins * batch * 64 + 3 * (size_t)batch * 64 + (((size_t)batch + 63) & ~63ull) +
          nblk * 64) * sizeof(float);
}

int eco::mpnn_backward_launch(const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                              const int32_t* graph_ids, int32_t batch, const float* obs_x, const void* saved,
                              const float* dq, void* gradws, hipStream_t st) {
  MpnnArgs a;
  int rc = prepare(a, packed, n_obs_in, gs, graph_ids, batch, obs_x, ECO_NORM_PER_CALL);
  if (rc) return rc;
  if (!saved || !dq || !gradws) return fail(ECO_ERR_ARG, "null saved/dq/workspace");
  a.sv = (float*)saved;
  a.dq = dq;
  a.gr = (float*)gradws;
  switch (mpnn_route(a, kernel_paths(), true)) {
    case ECO_ROUTE_DENSE3: return mpnn_backward_dense3_launch(a, st);
    case ECO_ROUTE_DENSE2: return mpnn_backward_dense2_launch(a, st);
    case ECO_ROUTE_DL: return mpnn_backward_dl_launch(a, st);
    case ECO_ROUTE_CSR: return launch_csr(a, true, false, st);
    default: return fail(ECO_ERR_ARG, "MPNN backward supports N <= 512");
  }
}

// The workspace of eco_mpnn_grad_<r.name>: a 256 B header (the call's max degree), the SV_* node tensors + MEAN + P,
// the GR_* tensors + per-graph partials (mpnn_grad_ws_bytes), one [rows_pad][64] gather-source buffer per episode, the
// forward's three ping-pong row buffers, the weight-gradient slabs; every part 256 B aligned.  total = 0: no such
// call (N outside the range, batch < 1 or batch * n_spins rows beyond the 32-bit row index of the weight gradients:
// at most (2^31 - 1) / 64 rows, 4095 samples of 8192 vertices).
GradRowsLayout eco::mpnn_grad_rows_layout(const RowsRange& r, int32_t n_spins, int32_t batch, size_t slab_bytes) {
  GradRowsLayout L{};
  if (!rows_in_range(r, n_spins) || batch < 1) return L;
  const size_t RT = (size_t)n_spins * batch;
  if (RT > (size_t)INT32_MAX / 64) return L;
  L.sv = 256;
  L.gr = L.sv + align_up(sv_mask_offset_floats(RT, batch) * sizeof(float), 256);
  L.g = L.gr + align_up(mpnn_grad_ws_bytes(n_spins, batch), 256);
  L.hbuf = L.g + rows_buffer_bytes(n_spins, batch, 1);
  L.slabs = L.hbuf + rows_buffer_bytes(n_spins, batch, 3);
  L.total = L.slabs + slab_bytes;
  return L;
}

// The launches of eco_mpnn_grad_<r.name> before the weight-gradient tail: the call's max degree, the saving forward,
// the backward over global rows with a DQ of r.dqcap entries (the float-weight instance exists for the default DQCAP
// alone: the wg range takes integer weights only).  The kernels walk an episode's rows in loops bounded by N and index
// across episodes in size_t (DESIGN section 25 has the audit).  The caller has checked the pointers and the range
// (mpnn_rows_check) and computed the layout.
int eco::mpnn_grad_rows_launch(const RowsRange& r, const float* packed, int32_t n_obs_in, const eco_graph_set* gs,
                               const int32_t* graph_ids, int32_t batch, const float* obs_x, const float* dq,
                               void* workspace, const GradRowsLayout& L, hipStream_t st) {
  if (!L.total || !rows_in_range(r, gs->n_spins) || (gs->edge_weights && !r.float_weights))
    return fail(ECO_ERR_ARG, rows_message(r, "grad", "no such call"));
  static_assert(!kRowsWg.float_weights, "the backward with DQCAP = ECO_MAX_SPINS_WG has no float-weight instance");
  MpnnArgs a;
  fill_args(a, packed, n_obs_in, gs, graph_ids, batch, obs_x, ECO_NORM_PER_CALL);
  char* ws = (char*)workspace;
  a.call_maxdeg = (int*)ws;
  a.sv = (float*)(ws + L.sv);
  a.gr = (float*)(ws + L.gr);
  a.dq = dq;
  float* gbuf = (float*)(ws + L.g);
  call_maxdeg_kernel<<<1, 1024, 0, st>>>(*gs, graph_ids, batch, (int*)ws);
  launch_forward_large(a, (float*)(ws + L.hbuf), true, st);
  if (r.dqcap == ECO_MAX_SPINS_WG) mpnn_backward_large_kernel<8, false, ECO_MAX_SPINS_WG><<<a.B, 512, 0, st>>>(a, gbuf);
  else if (a.gs.edge_weights) mpnn_backward_large_kernel<8, true><<<a.B, 512, 0, st>>>(a, gbuf);
  else mpnn_backward_large_kernel<8, false><<<a.B, 512, 0, st>>>(a, gbuf);
  return check_launch("mpnn_grad_rows");
}

// ---- split2_pk hazard probe (the v_fma_mix inline asm carries its own wait states) ----
namespace eco {
// One wave per 64 x 32 block of activations: the lane's four float4 split by split2_pk (inline asm) and fed to
// MFMAs exactly as mm_fh feeds them (order 0), with the lo fragment consumed first, straight after the asm (order
// 1), or with the split and that first MFMA in one asm block, the MFMA reading the register the last v_fma_mixhi
// wrote right after the product's wait states (order 2: the only schedule where nothing else can supply them, so
// a build without them -- ECO_SPLIT2_NEGATIVE_CONTROL -- must fail); the same products from the plain-conversion
// split (split2_ref).  out[2][block][4 x 16 outputs][64 lanes] fp32 accumulators, compared bitwise by the test.
template <bool REF>
__device__ __forceinline__ void probe_split_fh(const float4& a, const float4& b, float sf, f16x8& hi, f16x8& lo) {
  uint32_t h[4], l[4];
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (REF) split2_ref(v[2 * t], v[2 * t + 1], sf, h[t], l[t]);
    else split2_pk(v[2 * t], v[2 * t + 1], sf, h[t], l[t]);
  }
  const u32x4v hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
  hi = __builtin_bit_cast(f16x8, hv);
  lo = __builtin_bit_cast(f16x8, lv);
}
template <bool REF, int ORDER>
__device__ __forceinline__ void probe_mm(f32x4 (&acc)[4], const float4 (&x)[4], float sf, const uint16_t* WH,
                                         int lane) {
  const uint16_t* wl = WH + lane * 8;
#pragma unroll
  for (int kc2 = 0; kc2 < 2; ++kc2) {
    f16x8 w1[4], w2[4];  // weight fragments read first: nothing but the split sits between it and the MFMAs
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      w1[nt] = *reinterpret_cast<const f16x8*>(wl + ((0 * 4 + nt) * 2 + kc2) * FH_FRAG);
      w2[nt] = *reinterpret_cast<const f16x8*>(wl + ((1 * 4 + nt) * 2 + kc2) * FH_FRAG);
    }
    if (ORDER >= 1) {
      // order 1 places the lo fragment's first reader straight after the split's last v_fma_mixhi: all loads
      // drained and earlier MFMAs retired first (nothing for the compiler to interleave), then that first
      // MFMA as inline asm (so no compiler-inserted wait state can separate it from the asm split), followed by
      // enough s_nop for every MFMA result hazard the recognizer cannot see through asm
      __builtin_amdgcn_s_waitcnt(0);
      asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    f16x8 xh, xl;
    if (ORDER == 2 && !REF) {
      // order 2: the split's eight v_fma_mix (the product's asm text and wait states, ECO_MIXLO / ECO_MIXHI /
      // ECO_SPLIT2_WAIT) and the first MFMA reading its lo fragment in ONE asm block with fixed registers, the MFMA
      // straight after the v_fma_mixhi that wrote its last operand register: nothing the compiler schedules can
      // separate them, so only ECO_SPLIT2_WAIT stands between the write and the read.  The lo pieces are then
      // copied out for the remaining MFMAs.
      const float v[8] = {x[2 * kc2].x, x[2 * kc2].y, x[2 * kc2].z, x[2 * kc2].w,
                          x[2 * kc2 + 1].x, x[2 * kc2 + 1].y, x[2 * kc2 + 1].z, x[2 * kc2 + 1].w};
      uint32_t h[4], l[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) h[t] = pk_f16(v[2 * t] * sf, v[2 * t + 1] * sf);
      asm volatile("s_nop 4\n\t"  // the compiler's VALU writes of h / v before this asm (reads by VALU: none needed)
                   ECO_MIXLO("v200", "%[a0]", "%[sf]", "%[h0]") "\n\t" ECO_MIXLO("v201", "%[a2]", "%[sf]", "%[h1]") "\n\t"
                   ECO_MIXLO("v202", "%[a4]", "%[sf]", "%[h2]") "\n\t" ECO_MIXLO("v203", "%[a6]", "%[sf]", "%[h3]") "\n\t"
                   ECO_MIXHI("v200", "%[a1]", "%[sf]", "%[h0]") "\n\t" ECO_MIXHI("v201", "%[a3]", "%[sf]", "%[h1]") "\n\t"
                   ECO_MIXHI("v202", "%[a5]", "%[sf]", "%[h2]") "\n\t" ECO_MIXHI("v203", "%[a7]", "%[sf]", "%[h3]")
                   ECO_SPLIT2_WAIT "\n\t"
                   "v_mfma_f32_16x16x32_f16 %[acc], %[w], v[200:203], %[acc]\n\t"
                   "v_mov_b32 %[l0], v200\n\tv_mov_b32 %[l1], v201\n\tv_mov_b32 %[l2], v202\n\tv_mov_b32 %[l3], v203\n\t"
                   "s_nop 7\n\ts_nop 7\n\ts_nop 3"
                   : [acc] "+v"(acc[0]), [l0] "=&v"(l[0]), [l1] "=&v"(l[1]), [l2] "=&v"(l[2]), [l3] "=&v"(l[3])
                   : [w] "v"(w1[0]), [sf] "v"(sf), [h0] "v"(h[0]), [h1] "v"(h[1]), [h2] "v"(h[2]), [h3] "v"(h[3]),
                     [a0] "v"(v[0]), [a1] "v"(v[1]), [a2] "v"(v[2]), [a3] "v"(v[3]), [a4] "v"(v[4]), [a5] "v"(v[5]),
                     [a6] "v"(v[6]), [a7] "v"(v[7])
                   : "v200", "v201", "v202", "v203");
      const u32x4v hv = {h[0], h[1], h[2], h[3]}, lv = {l[0], l[1], l[2], l[3]};
      xh = __builtin_bit_cast(f16x8, hv);
      xl = __builtin_bit_cast(f16x8, lv);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      probe_split_fh<REF>(x[2 * kc2], x[2 * kc2 + 1], sf, xh, xl);
    }
    if (ORDER == 2 && REF) {  // the same first product from the plain split (compiler VALU: wait states written out)
      asm volatile("s_nop 4\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\ts_nop 7\n\ts_nop 7\n\ts_nop 3"
                   : "+v"(acc[0])
                   : "v"(w1[0]), "v"(xl));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ORDER == 1) {
      // (the plain-conversion reference split is compiler VALU code: its wait states before this asm MFMA are
      // written out here, the recognizer not knowing the asm is an MFMA; the asm split carries its own)
      if (REF)
        asm volatile("s_nop 4\n\tv_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\ts_nop 7\n\ts_nop 7\n\ts_nop 3"
                     : "+v"(acc[0])
                     : "v"(w1[0]), "v"(xl));
      else
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0\n\ts_nop 7\n\ts_nop 7\n\ts_nop 3"
                     : "+v"(acc[0])
                     : "v"(w1[0]), "v"(xl));
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (ORDER >= 1 && nt == 0) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[0], xh, acc[0], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[0], xh, acc[0], 0, 0, 0);
      } else if (ORDER == 0) {  // mm_fh
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[nt], xh, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[nt], xl, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[nt], xh, acc[nt], 0, 0, 0);
      } else {
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[nt], xl, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2[nt], xh, acc[nt], 0, 0, 0);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[nt], xh, acc[nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int ORDER>
__global__ __launch_bounds__(256) void split2_probe_kernel(const float* x, const float* sf, const uint16_t* W,
                                                           float* out, int n_blocks) {
  __shared__ __attribute__((aligned(16))) uint16_t sWH[FH_HALF];
  for (int i = threadIdx.x; i < FH_HALF / 8; i += 256)
    reinterpret_cast<uint4*>(sWH)[i] = reinterpret_cast<const uint4*>(W)[i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= n_blocks) return;  // whole waves
  float4 xv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) xv[c] = f4(x + ((size_t)blk * 64 + lane) * 16 + 4 * c);
  const float s = sf[blk];
  f32x4 a[4], r[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) a[nt] = r[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  probe_mm<false, ORDER>(a, xv, s, sWH, lane);
  probe_mm<true, ORDER>(r, xv, s, sWH, lane);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      out[(((size_t)0 * n_blocks + blk) * 16 + nt * 4 + i) * 64 + lane] = a[nt][i];
      out[(((size_t)1 * n_blocks + blk) * 16 + nt * 4 + i) * 64 + lane] = r[nt][i];
    }
}
}  // namespace eco

extern "C" int eco_probe_split2_mfma(const float* x, const float* sf, const uint16_t* w_frags, int32_t n_blocks,
                                     int32_t order, float* out, eco_stream_t stream) {
  using namespace eco;
  if (!x || !sf || !w_frags || !out || n_blocks < 1 || order < 0 || order > 2)
    return fail(ECO_ERR_ARG, "eco_probe_split2_mfma: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int grid = (n_blocks + 3) / 4;
  if (order == 0) split2_probe_kernel<0><<<grid, 256, 0, st>>>(x, sf, w_frags, out, n_blocks);
  else if (order == 1) split2_probe_kernel<1><<<grid, 256, 0, st>>>(x, sf, w_frags, out, n_blocks);
  else split2_probe_kernel<2><<<grid, 256, 0, st>>>(x, sf, w_frags, out, n_blocks);
  return check_launch("split2_probe");
}
