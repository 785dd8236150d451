// MPNN forward for many episodes on ONE shared large graph (N > 512: GSet G22 best-cut search,
// configs[4]; src/networks/mpnn.py:40-159 batched as in experiments/utils.py:154-187).
//
// Every aggregation A.H (mpnn.py:100, :115) is the SAME sparse matrix applied to B episodes.  A per-edge
// gather of each episode's 256-B fp32 row re-reads nnz x B x 256 B per layer (10.5 GB at G22 x 1024), and
// served from L2 at its gather ceiling (~15 TB/s measured, MI355X_MICROARCH.md 'Indexed rows': 16.8-18.8)
// that was 0.84 ms per layer.  Here an aggregation launch stages ONE feature chunk of ONE episode -- the
// [N][8] fp32 block, 64 KB at N = 2000 -- in LDS with one contiguous read, and every node's neighbour sum
// is taken from LDS (ds_read_b128 per edge and lane pair), nodes in 16-node tiles of similar degree walking
// their CSR rows in lockstep.  The graph's CSR words (16-bit, interleaved per tile) are LDS-resident too, loaded
// once per persistent workgroup (85 KB on G22-like graphs; graphs whose table does not fit next to the block
// read it from L2): HBM/L2 traffic per layer is one read and one write of H (2 x 0.5 GB).
// The Linears then run as a streaming pass over rows (no gathers): 16-row MFMA tiles of 4 consecutive
// nodes x 4 episodes, weights LDS-DMA-staged once per persistent workgroup.
//
// Layout: every per-node buffer is [slice s][feature chunk c of 8][episode e of the slice][node][8 floats]:
// an aggregation item (s, c, e) is one contiguous N x 32 B block, and a Linear tile's rows of one chunk are
// SH_EPS runs of 4 consecutive nodes x 32 B = 128 B.
//
// Phases (one launch each; U = relu(Wx.x + w_a), V = relu(Wx.x - w_a) and h0 = relu(W0.x) are never stored:
// the aggregation launches build their blocks from the 32-B observation rows, the first update layer its
// own rows):
//   edge:    AG = A+.U (+ A-.V);  e = relu(Wf.[AG / deg, deg / norm.max()])   (mpnn.py:89-104, +-1 weights)
//   layers:  AG = A.h;  m = relu(Wm.[AG / deg, e]), h' = relu(Wu.[h, m])  (mpnn.py:114-120, x3)
//            the last layer writes no h3: it emits q_local = Wr[64:].h3 per node and episode and the
//            per-episode column sums of h3 (fixed-order partials per tile)
//   readout: mean -> p = Wp.mean -> q = relu(p).Wr[:64] + q_local + b, fused epsilon-greedy act
//            (mpnn.py:143-159, dqn.py:453-465, :490-512)
// Linears: the three-product fp16x2 MFMAs of eco_mpnn_dense2.h (f32-accurate; per-node scale over the Linear's
// inputs, pre-split weights PK_FH).  Integer weights must be
// +-1 (the edge phase sums U over +1 edges and V over -1 edges); other graphs take mpnn_forward_large_kernel.
#pragma once
#include "eco_mpnn_dense2.h"

namespace eco {

#ifndef SH_NW_X
#define SH_NW_X 16
#endif
constexpr int SH_EPS = 4;              // episodes per slice
constexpr int SH_NPT = 16 / SH_EPS;    // nodes per Linear tile: 16 MFMA rows = SH_NPT nodes x SH_EPS episodes
constexpr int SH_NW = SH_NW_X;         // waves per Linear workgroup (one workgroup per CU: <= 128 VGPRs at 16)
constexpr int SH_PART = SH_EPS * 64;   // floats of one column-sum partial
constexpr int SH_RUN = 8;              // consecutive tiles per wave item of the last Linear launch (one partial)
#ifndef AG_NW_X
#define AG_NW_X 16
#endif
constexpr int AG_NW = AG_NW_X;         // waves per aggregation workgroup (8: 256 VGPRs for the block prefetch)
#ifndef AG_TPW_X
#define AG_TPW_X 2
#endif
constexpr int AG_TPW = AG_TPW_X;       // aggregation tile pairs per wave in flight together
#ifndef AG_NW16_X
#define AG_NW16_X 8
#endif
#ifndef AG_TPW16_X
#define AG_TPW16_X 2
#endif
constexpr int AG_NW16 = AG_NW16_X;     // the same two for the x-build instances on 16-float observation rows: their
constexpr int AG_TPW16 = AG_TPW16_X;   // x values (32 per lane at 16 waves) do not fit 128 VGPRs beside the pair tables
constexpr int AG_UNROLL = 4;           // a tile's rows are padded to multiples of 4 edges (one 8-B word group)

struct SharedBufs {
  float* HA;      // [S][4][SH_EPS][N][16]: h2 (h0, U and V are never stored: the aggregation launches and the
  float* HB;      //  first update layer rebuild them from the observation rows, 32 B per node instead of 256 B)
  float* EB;
  float* AG;      // the aggregation of the current phase (raw neighbour sums, not yet divided by the degree)
  float* part;    // [2 x groups][SH_EPS][64] column-sum partials of h3: one per (group of SH_RUN consecutive Linear
                  // tiles, slice the group touches)
  float* ql;      // [Epad][N] Wr[64:] . h3
  int32_t* perm;  // [N] nodes by decreasing degree
  int32_t* tn;    // [nt16][16] aggregation tiles: node of each slot (-1: none), 16 ranked nodes per tile
  int32_t* tml;   // [nt16] the tile's longest CSR row, rounded up to AG_UNROLL
  uint32_t* et;   // [nt16][MD / 4][16][4] the tile's CSR rows interleaved, four consecutive edges of a slot in one
                  // 16-B word group (edge i of slot k at ((i >> 2) * 16 + k) * 4 + (i & 3); padding: 0)
  uint16_t* et16; // the same words packed (tile t from toff[t], tml[t] x 16 words each) as sh_w16
  int32_t* toff;  // [nt16 + 1] first 16-bit word of each tile in et16; toff[nt16] = the table's words
  const uint64_t* key;  // workspace header: [0] key of the cached perm / tile tables, [1] 1 = rebuild this call
  int Epad, S, ntiles, nt16, MD, N;
};

inline int shared_grid() {  // persistent Linear workgroups: one per CU
  static const int g = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                               hipSuccess || n < 1)
      n = 256;
    return n;
  }();
  return g;
}

inline size_t shared_part_slots(int N, int B) {  // two per group of SH_RUN tiles (a group spans <= 2 slices)
  const size_t S = ((size_t)B + SH_EPS - 1) / SH_EPS, nt = ((size_t)N + SH_NPT - 1) / SH_NPT;
  return 2 * ((S * nt + SH_RUN - 1) / SH_RUN);
}
inline size_t shared_ws_bytes(int N, int B) {
  const size_t S = ((size_t)B + SH_EPS - 1) / SH_EPS, Epad = S * SH_EPS;
  const size_t nt16 = ((size_t)N + 15) / 16, MD = ((size_t)N + 3) / 4 * 4 + AG_UNROLL;
  return (4 * (size_t)N * Epad * 64 + shared_part_slots(N, B) * SH_PART + Epad * (size_t)N + N + nt16 * 17 + 4 + nt16 * MD * 16 +
          nt16 * MD * 8 + nt16 + 1 + 4) *
         sizeof(float);
}

inline SharedBufs shared_carve(float* base, int N, int B) {
  SharedBufs sb;
  sb.S = (B + SH_EPS - 1) / SH_EPS;
  sb.Epad = sb.S * SH_EPS;
  sb.N = N;
  sb.ntiles = (N + SH_NPT - 1) / SH_NPT;
  const size_t T1 = (size_t)N * sb.Epad * 64;
  sb.HA = base;
  sb.HB = sb.HA + T1;
  sb.EB = sb.HB + T1;
  sb.AG = sb.EB + T1;
  sb.part = sb.AG + T1;
  sb.ql = sb.part + shared_part_slots(N, B) * SH_PART;

  sb.perm = reinterpret_cast<int32_t*>(sb.ql + (size_t)sb.Epad * N);
  sb.nt16 = (N + 15) / 16;
  sb.MD = (N + 3) / 4 * 4 + AG_UNROLL;
  sb.tn = sb.perm + N;
  sb.tml = sb.tn + (size_t)sb.nt16 * 16;
  sb.et = reinterpret_cast<uint32_t*>(((uintptr_t)(sb.tml + sb.nt16) + 15) & ~(uintptr_t)15);  // 16-B groups
  sb.et16 = reinterpret_cast<uint16_t*>(sb.et + (size_t)sb.nt16 * sb.MD * 16);
  sb.toff = reinterpret_cast<int32_t*>(sb.et16 + (size_t)sb.nt16 * sb.MD * 16);
  return sb;
}

constexpr int SH_FC = 8;  // features per chunk (8 chunks)
// float offset of features 4 q .. 4 q + 3 of row (slice s, episode eps of the slice, node n): chunk q / 2 of the
// 8-feature chunks; features 16 c + 4 q .. (the lane's float4 c of the node-operand layout) add c * sh_cs(N)
__device__ __forceinline__ size_t sh_row(int N, int s, int eps, int n, int q) {
  return (((size_t)s * 8 * SH_EPS + eps) * N + n) * SH_FC + (size_t)(q >> 1) * SH_EPS * N * SH_FC + 4 * (q & 1);
}
__device__ __forceinline__ size_t sh_cs(int N) { return (size_t)2 * SH_EPS * N * SH_FC; }

// streaming (non-temporal) row access: the layer's own e rows and its output rows are touched once, and
// should not push the gathered slice of H out of the L2
__device__ __forceinline__ float4 f4_nt(const float* p) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st4_nt(float* p, float4 x) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(v4{x.x, x.y, x.z, x.w}, reinterpret_cast<v4*>(p));
}

// mm_fh of eco_mpnn_dense2.h (fp16x2 operands: the 64-input half of x scaled by the node's 2^kx, hi / lo pieces, three
// products) with one output tile's fragments in flight at a time (the shared-graph layer runs four Linears back to
// back: unbounded, the compiler hoists all the fragment reads and spills)
__device__ __forceinline__ void mm_fh_seq(f32x4 (&acc)[4], const float4 (&x)[4], float sf, const uint16_t* WH,
                                          int lane) {
  const uint16_t* wl = WH + lane * 8;
#pragma unroll
  for (int kc2 = 0; kc2 < 2; ++kc2) {
    f16x8 xh, xl;
    split_fh(x[2 * kc2], x[2 * kc2 + 1], sf, xh, xl);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const f16x8 w1 = *reinterpret_cast<const f16x8*>(wl + ((0 * 4 + nt) * 2 + kc2) * FH_FRAG);
      const f16x8 w2 = *reinterpret_cast<const f16x8*>(wl + ((1 * 4 + nt) * 2 + kc2) * FH_FRAG);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w2, xh, acc[nt], 0, 0, 0);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, xl, acc[nt], 0, 0, 0);
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, xh, acc[nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// perm[rank] = node, nodes ranked by decreasing degree (index on ties).  A workgroup ranks 64 nodes with 4
// threads per node, each comparing against a quarter of the degrees (staged in LDS in chunks of 2048, read
// 4 at a time); the four partial counts are summed with shuffles.
// The degree ranking (perm) and the bank-aware tile tables depend on the graph alone (and on the workspace
// layout, i.e. N and B), while a G22 best-cut search runs hundreds of forwards on one graph: they are kept in
// the workspace across calls.  shared_key_kernel hashes (N, B, graph id, the graph's CSR row pointers and edge
// words) into a 64-bit key (sum of per-word SplitMix64 finalisers: order-aware through the word index) and
// compares it with the key in the workspace header: equal -> flag 0 (the perm / tiles launches return at once);
// otherwise the new key is stored and flag 1 rebuilds them in this call (stream order).  A call with another B
// or N writes its own key into the same header slot, so a layout whose tables it overwrote cannot match later.
__device__ __forceinline__ uint64_t sh_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr int SK_THREADS = 1024;
__global__ __launch_bounds__(SK_THREADS) void shared_key_kernel(MpnnArgs a, uint64_t* key) {
  __shared__ uint64_t red[SK_THREADS / 64];
  const int N = a.N;
  const int gid = a.gids[0];
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* eg = a.gs.edges + a.gs.edge_base[gid];
  const int e0 = rp[0], ne = rp[N] - rp[0];
  uint64_t h = 0;
  for (int i = threadIdx.x; i <= N; i += SK_THREADS) h += sh_mix64(((uint64_t)i << 32) ^ (uint32_t)rp[i]);
#pragma unroll 4
  for (int i = threadIdx.x; i < ne; i += SK_THREADS) h += sh_mix64(((uint64_t)(i + N + 1) << 32) ^ eg[e0 + i]);
  for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);  // sums mod 2^64: any order gives the same key
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int k = 0; k < SK_THREADS / 64; ++k) t += red[k];
    const uint64_t k = t + sh_mix64(((uint64_t)N << 40) ^ ((uint64_t)a.B << 8) ^ 0x5EC0ull) +
                       sh_mix64(0xC0FFEEull + (uint64_t)gid);
    const bool same = key[0] == k;
    key[0] = k;
    key[1] = same ? 0ull : 1ull;
  }
}

__global__ __launch_bounds__(256) void shared_perm_kernel(MpnnArgs a, SharedBufs sb) {
  if (sb.key[1] == 0ull) return;  // cached from an earlier call on this graph and layout
  __shared__ __attribute__((aligned(16))) int DG[2048];
  const int N = a.N;
  const int i = blockIdx.x * 64 + (threadIdx.x >> 2), part = threadIdx.x & 3;
  const int32_t* rp = a.gs.row_ptr + (size_t)a.gids[0] * (N + 1);
  const int di = i < N ? rp[i + 1] - rp[i] : 0;
  int r = 0;
  for (int j0 = 0; j0 < N; j0 += 2048) {
    const int nj = min(2048, N - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < 2048; j += 256) DG[j] = j < nj ? rp[j0 + j + 1] - rp[j0 + j] : -1;
    __syncthreads();
    const int q0 = part * 512;  // this thread's quarter of the chunk, 4 degrees per LDS read
    for (int j = q0; j < min(q0 + 512, nj); j += 4) {
      const int4 d = *reinterpret_cast<const int4*>(&DG[j]);
      const int jj = j0 + j;
      r += (d.x > di) || (d.x == di && jj < i);
      r += (d.y > di) || (d.y == di && jj + 1 < i);
      r += (d.z > di) || (d.z == di && jj + 2 < i);
      r += (d.w > di) || (d.w == di && jj + 3 < i);
    }
  }
  r += __shfl_xor(r, 1, 64);
  r += __shfl_xor(r, 2, 64);
  if (i < N && part == 0) sb.perm[r] = i;
}

// The 16-input form of lin8 (observation rows of 16 floats, n_obs_in > 8): the two K-steps of lin8 on W [64][8]
// (features 0..7), then two more on WH [64][8] (features 8..15: PK_W0H / PK_WXH) with xk2 = x[8 + (l >> 4)] and
// xk3 = x[12 + (l >> 4)].  shared_agg_kernel's wide x-build runs the same four MFMAs in the same order on its LDS
// copy of the weights, so the h0 rebuilt by the first update layer equals the h0 the aggregation summed.
__device__ __forceinline__ void lin16(f32x4 (&d)[4], const float* W, const float* WH, float xk0, float xk1, float xk2,
                                      float xk3, int lane) {
  const float* wl = W + (lane & 15) * 8 + (lane >> 4);
  const float* wh = WH + (lane & 15) * 8 + (lane >> 4);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[nt * 128], xk0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[nt * 128 + 4], xk1, d[nt], 0, 0, 0);
    d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[nt * 128], xk2, d[nt], 0, 0, 0);
    d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[nt * 128 + 4], xk3, d[nt], 0, 0, 0);
  }
}

// aggregation tile tables: tile t, slot k -> node perm[16 t + k]; the tile's CSR rows interleaved (padding words
// 0: column 0, weight 0) in a BANK-AWARE order, and the tile's longest row (slot 0: ranked first).
// In shared_agg_kernel lane 2k + q reads 16 B of the 32-B row col of slot k's current edge (a wave: slots 0..15
// of one tile, then of the pair's second tile): a ds_read_b128 serves the lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md LDS) = slots {0,1,6,7,10,11,12,13} and {2,3,4,5,8,9,14,15} of each
// tile, each group eight 32-B rows, whose bank eighth is col mod 8.  Random columns put ~2.4 LDS cycles on a group
// and step; so one thread per (tile, group) orders its eight rows greedily: at every step each slot (fewest residue
// classes left first) takes its next edge of an eighth no other slot of the group uses at that step -- the class
// with most edges left -- or, with none free, of the least-used eighth (most edges left on ties); no step is added:
// a row keeps its length.  The neighbour sums change summation order only.
__device__ __forceinline__ int sh_group_slot(int g, int j) {
  constexpr uint32_t tab[2] = {0xDCBA7610u, 0xFE985432u};  // slot of position j: nibble j
  return (tab[g] >> (4 * j)) & 0xF;
}
// One thread per (tile, group).  Every per-thread table the greedy indexes with a run-time slot / class lives
// in LDS (in registers such indexing compiles to scratch memory: 310-334 us per call on G22), and each thread
// first copies its eight rows into LDS (the first ST_CAP edges of each, independent loads), so the walk reads LDS;
// rows longer than ST_CAP (hub vertices) read their tail from global memory.
constexpr int ST_CAP = 64;
constexpr int ST_THREADS = 32;
constexpr int ST_LD = 65;  // ints per thread in the class tables (odd stride: no bank conflicts across threads)
constexpr int ST_SM = 33;
__global__ __launch_bounds__(ST_THREADS) void shared_tiles_kernel(MpnnArgs a, SharedBufs sb) {
  if (sb.key[1] == 0ull) return;  // cached
  __shared__ uint32_t rows[ST_THREADS][8][ST_CAP];
  __shared__ int s_cnt[ST_THREADS * ST_LD], s_cur[ST_THREADS * ST_LD], s_small[ST_THREADS * ST_SM];
  const int N = a.N;
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  const int t = i >> 1, g = i & 1;
  if (t >= sb.nt16) return;
  const int gid = a.gids[0];
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* eg = a.gs.edges + a.gs.edge_base[gid];
  const int n0 = sb.perm[t * 16];
  const int ml = (rp[n0 + 1] - rp[n0] + AG_UNROLL - 1) / AG_UNROLL * AG_UNROLL;
  if (g == 0) sb.tml[t] = ml;
  uint32_t (*my)[ST_CAP] = rows[threadIdx.x];
  int* cnt = s_cnt + threadIdx.x * ST_LD;  // [slot j][class r] at 8j + r: edges of the class left
  int* cur = s_cur + threadIdx.x * ST_LD;  // [j][r]: next position to scan for class r
  int* bj = s_small + threadIdx.x * ST_SM;  // [0..7] row start, [8..15] ncls, [16..23] ord, [24..31] used
  int* ncls = bj + 8;
  int* ord = bj + 16;
  int* used = bj + 24;
  int k[8], len[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k[j] = sh_group_slot(g, j);
    const int slot = t * 16 + k[j];
    const bool valid = slot < N;
    const int n = valid ? sb.perm[slot] : 0;
    bj[j] = valid ? rp[n] : 0;
    len[j] = valid ? rp[n + 1] - rp[n] : 0;
    sb.tn[slot] = valid ? n : -1;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int nl = min(len[j], ST_CAP);
    const int b = bj[j];
#pragma unroll 8
    for (int e = 0; e < nl; ++e) my[j][e] = eg[b + e];
  }
  auto edge_at = [&](int j, int e) -> uint32_t { return e < ST_CAP ? my[j][e] : eg[bj[j] + e]; };
  for (int j = 0; j < 8; ++j) {
    for (int r = 0; r < 8; ++r) cnt[8 * j + r] = cur[8 * j + r] = 0;
    for (int e = 0; e < len[j]; ++e) ++cnt[8 * j + (edge_col(edge_at(j, e)) & 7)];
  }
  uint32_t* et = sb.et + (size_t)t * sb.MD * 16;
  for (int q = 0; q < max(ml, AG_UNROLL); ++q) {
    for (int j = 0; j < 8; ++j) {
      int c = 0;
      for (int r = 0; r < 8; ++r) c += cnt[8 * j + r] > 0;
      ncls[j] = c;
      ord[j] = j;
      used[j] = 0;
    }
    for (int x = 1; x < 8; ++x)  // insertion sort of the eight slots by classes left (stable)
      for (int y = x; y > 0 && ncls[ord[y]] < ncls[ord[y - 1]]; --y) {
        const int tmp = ord[y]; ord[y] = ord[y - 1]; ord[y - 1] = tmp;
      }
    for (int x = 0; x < 8; ++x) {
      const int j = ord[x];
      uint32_t ex = 0u;  // padding
      if (ncls[j] > 0) {
        const int* cj = cnt + 8 * j;
        int best = -1;
        for (int r = 0; r < 8; ++r)  // a free class with the most edges left
          if (cj[r] > 0 && used[r] == 0 && (best < 0 || cj[r] > cj[best])) best = r;
        if (best < 0)
          for (int r = 0; r < 8; ++r)  // else the least-used class (most edges left on ties)
            if (cj[r] > 0 && (best < 0 || used[r] < used[best] || (used[r] == used[best] && cj[r] > cj[best])))
              best = r;
        ++used[best];
        --cnt[8 * j + best];
        int e = cur[8 * j + best];
        ex = edge_at(j, e);
        while ((edge_col(ex) & 7) != best) ex = edge_at(j, ++e);
        cur[8 * j + best] = e + 1;
      }
      et[((q >> 2) * 16 + sh_group_slot(g, j)) * 4 + (q & 3)] = ex;  // (no run-time index into k[])
    }
  }
}

// 16-bit form of an edge word for the packed table: the byte offset of the column's 32-B block row (col x 32, N <=
// 2048: bits 5..15) | the weight as a 2-bit signed field in bits 0..1 (+1: 01, -1: 11; the shared path has +-1
// weights).  A padding word (et word 0) has weight 0 and points at row N, which the aggregation keeps zero in its
// LDS block (N < 2048; row 0 at N = 2048): graphs without -1 edges then sum every word with weight 1.
__device__ __forceinline__ uint16_t sh_w16(uint32_t ex, int N) {
  if (ex == 0u) return (uint16_t)(N < 2048 ? N << 5 : 0);
  const int w = edge_w(ex);
  return (uint16_t)((edge_col(ex) << 5) | (w > 0 ? 1 : (w < 0 ? 3 : 0)));
}
// et -> et16 (rebuild calls only): tile t's first tml[t] x 16 interleaved words, tiles back to back (each a multiple
// of 64 words: 128-B aligned), toff[t] its first word
constexpr int SP_THREADS = 1024;
constexpr int AG_ZW = 64;  // zero words behind the packed table
__global__ __launch_bounds__(SP_THREADS) void shared_pack_kernel(SharedBufs sb) {
  if (sb.key[1] == 0ull) return;  // cached
  __shared__ int off[2049 / 16 + 2];
  if (threadIdx.x == 0) {
    int o = 0;
    for (int t = 0; t < sb.nt16; ++t) {
      off[t] = o;
      o += sb.tml[t] * 16;
    }
    off[sb.nt16] = o;
  }
  __syncthreads();
  for (int t = threadIdx.x; t <= sb.nt16; t += SP_THREADS) sb.toff[t] = off[t];
  for (int t = 0; t < sb.nt16; ++t) {
    const uint32_t* src = sb.et + (size_t)t * sb.MD * 16;
    uint16_t* dst = sb.et16 + off[t];
    const int n = sb.tml[t] * 16;
    for (int i = threadIdx.x; i < n; i += SP_THREADS) dst[i] = sh_w16(src[i], sb.N);
  }
  // 64 zero words behind the table: the reads of a lane past its row (and of padding pairs) point there
  for (int i = threadIdx.x; i < AG_ZW; i += SP_THREADS) sb.et16[off[sb.nt16] + i] = sh_w16(0u, sb.N);
}

// AG[item] (+)= A^(mode) . src[item] for the items = (slice, chunk, episode) blocks: an item's [N][8] block of src
// sits in LDS while every node's neighbour sum is taken from it.  Persistent workgroups (one per CU) walk items
// blockIdx.x, + grid, ...: the NEXT item's block is loaded into registers (4 float4 per thread) while the current
// one is aggregated, then written to LDS between two barriers.  The packed edge table (et16) is copied into the LDS
// behind the block once per workgroup when it fits (AG_LDS bytes in all), else read from L2.  Lane = (node slot
// k = lane >> 1 of two 16-node tiles, feature half q = lane & 1); pairs of tiles ranked by decreasing degree (the
// pair's first tile has the longer rows) walk their interleaved rows in lockstep, AG_TPW pairs per wave at a time,
// the next 4 edge words of each read one step ahead; each row is summed in the order of et16.
// mode 0: weight w (+-1); +1: edges with w > 0, weight 1; -1: edges with w < 0, weight 1.  accumulate: add
// to AG (the A- pass of the edge phase).
// XSRC 0: the block is read from src; 1 / 2 / 3: it is BUILT from the observation rows x (32 B per node) as
// U = relu(Wx.x + w_a) / V = relu(Wx.x - w_a) / h0 = relu(W0.x) (mpnn.py:89-104, :55) with lin8's two MFMAs per
// 16-feature chunk (d[c] of lin8, eco_mpnn_dense.h, so the rebuilt rows equal those of the dense kernels' form): the
// next item's x values are what is prefetched, the Linear runs when the block is written to LDS.
// XW: floats per observation row (XSRC 1..3).  16 (n_obs_in > 8): two more x values per tile are prefetched and the
// build runs four K-steps (lin16's order), its weight block AG_WL16 floats; the 8-wide instances are unchanged.
constexpr int AG_LDS = 160 * 1024;                               // dynamic LDS of the aggregation launches
constexpr int AG_WL = 576;                                        // floats of the x-build weights (64 x 8 + 64)
// 16-float observation rows (XW = 16): the weights of features 8..15 (64 x 8: PK_W0H / PK_WXH) follow the AG_WL block
constexpr int AG_WL16 = AG_WL + 512;
constexpr int AG_PF = (4096 + 64 * AG_NW - 1) / (64 * AG_NW);  // float4 per thread per block: 64 KB (N <= 2048)
// A wave's tile pairs are the same for every item: p = w + (r AG_TPW + j) AG_NW, rounds r < AG_R.  Their row
// lengths, table offsets and output nodes are read once per workgroup into registers (global loads inside the item
// loop would wait for the next block's prefetch too: vmcnt counts in order).
// TPW, NW: tile pairs in flight per wave and waves per workgroup of the instance (AG_TPW, AG_NW; the x-build on
// 16-float rows: AG_TPW16, AG_NW16)
template <int TPW, int NW>
struct AgPairs {
  static constexpr int R = (2048 / 32 + TPW * NW - 1) / (TPW * NW);
  int base[R][TPW], ml[R][TPW], mlw[R][TPW], nd[R][TPW];
};
template <int TPW, int NW>
__device__ __forceinline__ void sh_agg_pairs(const SharedBufs& sb, AgPairs<TPW, NW>& P, int w, int lane) {
  constexpr int AG_R = AgPairs<TPW, NW>::R;
  const int k = lane >> 1;
  const int jt = k >> 4, slot = k & 15;
#pragma unroll
  for (int r = 0; r < AG_R; ++r)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int p = w + (r * TPW + j) * NW;
      const int t = 2 * p + jt;
      const bool live = 2 * p < sb.nt16 && t < sb.nt16;
      P.ml[r][j] = live ? sb.tml[t] : 0;
      P.mlw[r][j] = 2 * p < sb.nt16 ? uniform_i(sb.tml[2 * p]) : 0;  // the pair's longest rows (its first tile)
      P.base[r][j] = (live ? sb.toff[t] : 0) + slot * 4;
      P.nd[r][j] = live ? sb.tn[t * 16 + slot] : -1;
    }
}
// one item: every node's sums over its row of the packed table, the block in LDS (HL); MODE 0: weights +-1,
// +1: the +1 edges with weight 1, -1: the -1 edges with weight 1
template <bool LDSW, int MODE, bool UNIT, int RB, int TPW, int NW>
__device__ __forceinline__ void sh_agg_item(const AgPairs<TPW, NW>& P, int nt16, const float4* HL, const uint16_t* tab,
                                            int zoff, float* dst, int accumulate, int w, int lane) {
  constexpr int AG_R = AgPairs<TPW, NW>::R;
  const int q = lane & 1;
  typedef uint16_t __attribute__((ext_vector_type(4))) u16x4;
  typedef float f2v __attribute__((ext_vector_type(2)));
  const char* hb = reinterpret_cast<const char*>(HL);
  const uint32_t qoff = 16u * (uint32_t)q;
#pragma unroll
  for (int r = 0; r < AG_R; ++r) {
    if (2 * (w + r * TPW * NW) >= nt16) break;  // wave-uniform
    u16x4 cur[TPW], nxt[TPW] = {};
    f2v a01[TPW], a23[TPW];  // the lane's four sums as two packed pairs (v_pk_fma_f32)
    // reads are never predicated: a lane past its row reads the zero words at zoff (a conditional select of the
    // loaded value would make the compiler wait for it at once)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      a01[j] = a23[j] = f2v{0.f, 0.f};
      cur[j] = *reinterpret_cast<const u16x4*>(tab + (P.ml[r][j] > 0 ? P.base[r][j] : zoff));
    }
    for (int i = 0; i < P.mlw[r][0]; i += 4) {
#pragma unroll
      for (int j = 0; j < TPW; ++j)
        if (i + 4 < P.mlw[r][j])  // wave-uniform
          nxt[j] = *reinterpret_cast<const u16x4*>(tab + (i + 4 < P.ml[r][j] ? P.base[r][j] + (i + 4) * 16 : zoff));
      // this step's row reads first (RB edges of each pair at a time), then the sums
#pragma unroll
      for (int u0 = 0; u0 < 4; u0 += RB) {
        float4 h[TPW][RB];
        float f[TPW][RB];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (i < P.mlw[r][j]) {  // wave-uniform
            const uint2 wd = __builtin_bit_cast(uint2, cur[j]);
#pragma unroll
            for (int v = 0; v < RB; ++v) {
              const int u = u0 + v;
              const uint32_t w32 = (u < 2 ? wd.x : wd.y) >> (16 * (u & 1));  // high half: masked below
              if (!UNIT) {
                const int code = ((int)(w32 << 30)) >> 30;                    // +1, -1, 0
                f[j][v] = (float)(MODE == 0 ? code : (MODE > 0 ? max(code, 0) : max(-code, 0)));
              }
              h[j][v] = *reinterpret_cast<const float4*>(hb + ((w32 & 0xFFE0u) | qoff));
            }
          }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
          if (i < P.mlw[r][j]) {
#pragma unroll
            for (int v = 0; v < RB; ++v) {
              if (UNIT) {  // every word weight 1 (padding reads the zero row): packed adds
                a01[j] += f2v{h[j][v].x, h[j][v].y};
                a23[j] += f2v{h[j][v].z, h[j][v].w};
              } else {
                a01[j] = __builtin_elementwise_fma(f2v{f[j][v], f[j][v]}, f2v{h[j][v].x, h[j][v].y}, a01[j]);
                a23[j] = __builtin_elementwise_fma(f2v{f[j][v], f[j][v]}, f2v{h[j][v].z, h[j][v].w}, a23[j]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        if (i < P.mlw[r][j]) {
          cur[j] = nxt[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (P.nd[r][j] >= 0) {
        float* d = dst + (size_t)P.nd[r][j] * SH_FC + 4 * q;
        float4 o = make_float4(a01[j].x, a01[j].y, a23[j].x, a23[j].y);
        if (accumulate) {
          const float4 pv = f4(d);
          o = make_float4(pv.x + o.x, pv.y + o.y, pv.z + o.z, pv.w + o.w);
        }
        st4(d, o);
      }
    }
  }
}
template <int XSRC, int XW = 8, int NW = (XW == 16 ? AG_NW16 : AG_NW)>
__global__ __launch_bounds__(64 * NW, 1) void shared_agg_kernel(MpnnArgs a, SharedBufs sb, const float* src,
                                                                   int mode, int accumulate, int items) {
  static_assert(XW == 8 || (XW == 16 && XSRC != 0), "observation rows are 8 or 16 floats");
  constexpr int WL = XW == 16 ? AG_WL16 : AG_WL;
  // mode (the host's +1 / -1 / 0 per launch) must match XSRC: 1 -> +1, 2 -> -1, 0 / 3 -> 0
  extern __shared__ __attribute__((aligned(16))) float4 HL[];  // [N][2], then the packed edge table
  const int N = a.N;
  if (mode < 0 && !(a.gs.meta[(size_t)a.gids[0] * 4 + 2] < 0.0)) return;  // no -1 edge: A- . V = 0
  const int n2 = N * 2;
  static_assert(XSRC != 0 || NW == AG_NW, "AG_PF is sized for AG_NW waves");
  constexpr int NPF = XSRC ? 1 : AG_PF;
  constexpr int NXT = XSRC ? (2048 / 16 + NW - 1) / NW : 1;  // 16-node x tiles per wave (N <= 2048)
  float4 pf[NPF];
  float xk0[NXT], xk1[NXT];
  float xk2[XW == 16 ? NXT : 1], xk3[XW == 16 ? NXT : 1];  // features 8..15 (wide rows)
  int pc = 0;  // chunk of the prefetched item (XSRC)
  // XSRC: the 8-input Linear (W0 or Wx: 64 x 8) and w_a sit at the end of the LDS (AG_WL floats), read per item
  // (global reads inside the build would expose an L2 round trip per item; registers would spill)
  float* WLs = reinterpret_cast<float*>(reinterpret_cast<char*>(HL) + AG_LDS) - WL;
  const int wv_ = threadIdx.x >> 6, ln = threadIdx.x & 63;
  // the k-th item of this workgroup (-1: none).  XSRC 0: items blockIdx.x + k grid.  XSRC 1..3: the workgroup
  // walks whole episodes, their 8 chunks in a row (episode blockIdx.x + (k / 8) grid, chunk k % 8), so an episode's
  // x rows are loaded once for its 8 blocks (one workgroup per episode, instead of 8 reading them from the MALL)
  auto item_of = [&](int k) -> int {
    if (XSRC == 0) {
      const int it = (int)blockIdx.x + k * (int)gridDim.x;
      return it < items ? it : -1;
    }
    const int ep = (int)blockIdx.x + (k >> 3) * (int)gridDim.x;
    if (ep >= items / 8) return -1;
    return ((ep / SH_EPS) * 8 + (k & 7)) * SH_EPS + ep % SH_EPS;
  };
  auto load_block = [&](int it, int k) {
    if (XSRC == 0) {
      const float* S = src + (size_t)it * N * SH_FC;
#pragma unroll
      for (int u = 0; u < NPF; ++u) {
        const int i = threadIdx.x + u * 64 * NW;
        pf[u] = f4_nt(S + 4 * (size_t)min(i, n2 - 1));
      }
    } else {
      const int e = it % SH_EPS, c = (it / SH_EPS) % 8, s = it / (8 * SH_EPS);
      const int ep = s * SH_EPS + e;
      pc = c;
      if ((k & 7) == 0)  // the episode's first chunk: its x rows (kept for the other 7)
#pragma unroll
      for (int j = 0; j < NXT; ++j) {
        // unpredicated loads (a predicated load compiles to a branch and a wait per load): a padding episode
        // reads episode B - 1's rows and reaches only its own rows; nodes past N are not stored
        const int n = min((wv_ + j * NW) * 16 + (ln & 15), N - 1);
        const float* xr = a.x + ((size_t)min(ep, a.B - 1) * N + n) * XW + (ln >> 4);
        xk0[j] = xr[0];
        xk1[j] = xr[4];
        if constexpr (XW == 16) {
          xk2[j] = xr[8];
          xk3[j] = xr[12];
        }
      }
    }
  };
  auto store_block = [&]() {
    if (XSRC == 0) {
#pragma unroll
      for (int u = 0; u < NPF; ++u) {
        const int i = threadIdx.x + u * 64 * NW;
        if (i < n2) HL[i] = pf[u];
      }
    } else {
      // chunk c of lin8 gives features 16c + 4 (ln >> 4) .. (c = pc / 2): the lanes of 8-feature chunk pc keep theirs
      const bool mine = (ln >> 5) == (pc & 1);
      const float* wl = WLs + (ln & 15) * 8 + (ln >> 4) + (pc >> 1) * 128;
      const float wv0 = wl[0], wv1 = wl[4];
      float wv2 = 0.f, wv3 = 0.f;
      if constexpr (XW == 16) {
        wv2 = wl[AG_WL];
        wv3 = wl[AG_WL + 4];
      }
      const float4 wa = XSRC == 3 ? make_float4(0.f, 0.f, 0.f, 0.f)
                                  : *reinterpret_cast<const float4*>(WLs + 512 + 16 * (pc >> 1) + 4 * (ln >> 4));
#pragma unroll
      for (int j = 0; j < NXT; ++j) {
        const int n = (wv_ + j * NW) * 16 + (ln & 15);
        if ((wv_ + j * NW) * 16 >= N) break;  // wave-uniform: MFMAs below run with EXEC all ones
        // lin8's chunk on the preloaded weights (the same two MFMAs)
        f32x4 z = __builtin_amdgcn_mfma_f32_16x16x4f32(wv0, xk0[j], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f32_16x16x4f32(wv1, xk1[j], z, 0, 0, 0);
        if constexpr (XW == 16) {  // features 8..15: lin16's third and fourth K-step
          z = __builtin_amdgcn_mfma_f32_16x16x4f32(wv2, xk2[j], z, 0, 0, 0);
          z = __builtin_amdgcn_mfma_f32_16x16x4f32(wv3, xk3[j], z, 0, 0, 0);
        }
        const float sg = XSRC == 2 ? -1.f : 1.f;
        float4 v = XSRC == 3 ? relu4(z)
                             : make_float4(relu(fmaf(sg, wa.x, z[0])), relu(fmaf(sg, wa.y, z[1])),
                                           relu(fmaf(sg, wa.z, z[2])), relu(fmaf(sg, wa.w, z[3])));
        if (mine && n < N) HL[n * 2 + ((ln >> 4) & 1)] = v;  // padding episodes (x = 0) only reach their own rows
      }
    }
  };
  int item = item_of(0);
  if (item < 0) return;
  const int nwords = sb.toff[sb.nt16];
  // LDS: the block's N rows, the zero row N, the packed table ... the x-build weights at the end
  const bool in_lds = (size_t)(n2 + 2) * 16 + (size_t)(nwords + AG_ZW) * 2 + WL * 4 <= (size_t)AG_LDS;  // uniform
  if (XSRC)
    for (int i = threadIdx.x; i < AG_WL; i += 64 * NW)
      WLs[i] = i < 512 ? a.P[(XSRC == 3 ? PK_W0 : PK_WX) + i] : (i < 576 ? a.P[PK_WA + i - 512] : 0.f);
  if constexpr (XW == 16)
    for (int i = threadIdx.x; i < 512; i += 64 * NW) WLs[AG_WL + i] = a.P[(XSRC == 3 ? PK_W0H : PK_WXH) + i];
  uint16_t* T16 = reinterpret_cast<uint16_t*>(HL + n2 + 2);                           // 16-B aligned
  // no -1 edge and N < 2048 (padding on the zero row): every word is a +1 edge (A+ = A; the A- pass returned above)
  const bool unit = N < 2048 && !(a.gs.meta[(size_t)a.gids[0] * 4 + 2] < 0.0);
  if (threadIdx.x < 2) HL[n2 + threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (in_lds) {
    const uint4* s4p = reinterpret_cast<const uint4*>(sb.et16);
    uint4* d4p = reinterpret_cast<uint4*>(T16);
    for (int i = threadIdx.x; i < (nwords + AG_ZW) / 8; i += 64 * NW) d4p[i] = s4p[i];  // multiples of 64
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // wide rows: AG_NW16 waves (twice the registers per lane for twice the x values), AG_TPW16 pairs in flight
  constexpr int TPW = XW == 16 ? AG_TPW16 : AG_TPW;
  AgPairs<TPW, NW> P;
  sh_agg_pairs<TPW, NW>(sb, P, w, lane);
  if (XSRC) __syncthreads();  // the x-build weights
  load_block(item, 0);
  store_block();
  __syncthreads();
  constexpr int MODE = XSRC == 1 ? 1 : (XSRC == 2 ? -1 : 0);  // U over +1 edges, V over -1 edges, else signed
  for (int k = 0; item >= 0; ++k) {
    const int next = item_of(k + 1);
    const bool more = next >= 0;
    if (more) load_block(next, k + 1);  // lands while this item is aggregated
    float* dst = sb.AG + (size_t)item * N * SH_FC;
    // row reads in flight per pair: 4 edges (2: measured slower where the x prefetch holds registers)
    constexpr int RB = 4;
    if (in_lds && unit) sh_agg_item<true, MODE, true, RB, TPW, NW>(P, sb.nt16, HL, T16, nwords, dst, accumulate, w, lane);
    else if (in_lds) sh_agg_item<true, MODE, false, RB, TPW, NW>(P, sb.nt16, HL, T16, nwords, dst, accumulate, w, lane);
    else sh_agg_item<false, MODE, false, RB, TPW, NW>(P, sb.nt16, HL, sb.et16, nwords, dst, accumulate, w, lane);
    __syncthreads();  // every wave is done with this block
    if (more) store_block();
    __syncthreads();
    item = next;
  }
}

// PHASE 0: edge embedding -> EB; 1: update layer Hc -> Hn; 2: last update layer -> q_local + column sums.
// Persistent workgroups (weights LDS-DMA-staged once); wave items = Linear tiles (slice-major, node tiles of
// SH_NPT consecutive nodes), lane row c16 = node kn x episode eps.  Rows of padding episodes and nodes are
// computed but stored as zeros / not stored.
// XW: floats per observation row (only layer 0 of PHASE 1, Hc == nullptr, reads x): 16 rebuilds h0 with lin16.
template <int PHASE, int XW = 8>
__global__ __launch_bounds__(64 * SH_NW, 1) void shared_lin_kernel(MpnnArgs a, SharedBufs sb, int layer,
                                                                   const float* Hc, float* Hn) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63;
  const int w = uniform_i(threadIdx.x >> 6);
  const int c16 = lane & 15, s4 = lane >> 4;
  const int kn = c16 / SH_EPS, eps = c16 % SH_EPS;
  uint16_t* WL = reinterpret_cast<uint16_t*>(lds);
  const uint16_t* PH = reinterpret_cast<const uint16_t*>(a.P + PK_FH);
  if (PHASE == 0) glds_frags<SH_NW>(WL, PH + FH_WF, 16, w, lane);
  else glds_frags<SH_NW>(WL, PH + FH_LAYER + layer * FH_LAYER_STRIDE, 64, w, lane);
  const int N = a.N;
  const int gid = a.gids[0];
  const float* P = a.P;
  const float md = PHASE == 0 ? (float)(a.norm_scope == ECO_NORM_PER_CALL ? *a.call_maxdeg : a.gs.max_deg[gid]) : 1.f;
  const size_t cs = sh_cs(N);
  glds_wait();
  __syncthreads();
  const int total = sb.S * sb.ntiles;
  // the rows of a tile: AG (all phases), e and h (update layers; layer 0 rebuilds h0 from x).  The NEXT
  // item's rows are loaded while the current one's Linears run.
  struct Rows {
    float4 ag[4], ev[4], hc[4];
    float xk0, xk1;
    float xh[XW == 16 ? 2 : 0];  // x[8 + s4], x[12 + s4] (wide rows)
  };
  auto load_rows = [&](Rows& R, int it) {
    const int s = it / sb.ntiles, t = it - s * sb.ntiles;
    const int ep = s * SH_EPS + eps;
    const int n = t * SH_NPT + kn;
    const int nc = min(n, N - 1);
    const size_t ro = sh_row(N, s, eps, nc, s4);
#pragma unroll
    for (int c = 0; c < 4; ++c) R.ag[c] = f4_nt(sb.AG + ro + c * cs);
    if (PHASE != 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) R.ev[c] = f4_nt(sb.EB + ro + c * cs);
      if (XW == 8 && Hc) {  // the wide instance is layer 0 only: it always rebuilds h0
#pragma unroll
        for (int c = 0; c < 4; ++c) R.hc[c] = f4_nt(Hc + ro + c * cs);
      } else {
        // unpredicated (clamped) loads: rows of padding episodes and nodes are stored as zeros
        const float* xr = a.x + ((size_t)min(ep, a.B - 1) * N + nc) * XW + s4;
        R.xk0 = xr[0];
        R.xk1 = xr[4];
        if constexpr (XW == 16) {
          R.xh[0] = xr[8];
          R.xh[1] = xr[12];
        }
      }
    }
  };
  // items strided over the waves; the last layer (PHASE 2) strides groups of SH_RUN consecutive tiles, so each
  // wave's column sums accumulate over a group in registers and leave as one partial per (group, slice it touches)
  const int wid = blockIdx.x * SH_NW + w;
  const int waves = gridDim.x * SH_NW;
  constexpr int RUN = PHASE == 2 ? SH_RUN : 1;
  float4 run[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) run[nt] = zero4();
  for (int it = wid * RUN; it < total; it += waves * RUN)
  for (int item = it; item < min(total, it + RUN); ++item) {
    Rows cu;
    load_rows(cu, item);
    const int s = item / sb.ntiles, t = item - s * sb.ntiles;
    const int ep = s * SH_EPS + eps;
    const bool evalid = ep < a.B;
    const int n = t * SH_NPT + kn;
    const bool nvalid = n < N;
    const int nc = min(n, N - 1);
    const float nf = (float)max(a.gs.deg[(size_t)gid * N + nc], 1);
    const size_t ro = sh_row(N, s, eps, nc, s4);
    float4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[c] = cu.ag[c];
      acc[c].x = acc[c].x / nf; acc[c].y = acc[c].y / nf; acc[c].z = acc[c].z / nf; acc[c].w = acc[c].w / nf;
    }
    const bool rvalid = nvalid && evalid;
    if (PHASE == 0) {
      if (s4 == 3) acc[3].w = nf / md;  // feature 63 = norm / norm.max() (mpnn.py:102)
      f32x4 d[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int kx = node_exp<4>(acc);
      mm_fh_seq(d, acc, exp2i(kx), WL, lane);
      unscale(d, kx + fh_kw(P, 0));
      if (nvalid) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st4_nt(sb.EB + ro + nt * cs, rvalid ? relu4(d[nt]) : zero4());
      }
    } else {
      f32x4 d[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) d[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      {  // message = relu(Wm . [agg, e]): one node scale over both halves, as the dense kernels
        const int kx = node_exp2(acc, cu.ev);
        const float sf = exp2i(kx);
        mm_fh_seq(d, cu.ev, sf, WL + FH_HALF, lane);
        mm_fh_seq(d, acc, sf, WL, lane);
        unscale(d, kx + fh_kw(P, 1 + 2 * layer));
      }
      float4 mr[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) mr[c] = relu4(d[c]);
      f32x4 hn[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) hn[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      float4 hc[4];
      if (XW == 8 && Hc) {
#pragma unroll
        for (int c = 0; c < 4; ++c) hc[c] = cu.hc[c];
      } else {  // layer 0: h0 = relu(W0 . x) of this lane's row (lin8, as the aggregation built it)
        f32x4 z[4];
        if constexpr (XW == 16) lin16(z, P + PK_W0, P + PK_W0H, cu.xk0, cu.xk1, cu.xh[0], cu.xh[1], lane);
        else lin8(z, P + PK_W0, cu.xk0, cu.xk1, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) hc[c] = relu4(z[c]);
      }
      {  // h' = relu(Wu . [h, m])
        const int kx = node_exp2(hc, mr);
        const float sf = exp2i(kx);
        mm_fh_seq(hn, hc, sf, WL + 2 * FH_HALF, lane);
        mm_fh_seq(hn, mr, sf, WL + 3 * FH_HALF, lane);
        unscale(hn, kx + fh_kw(P, 2 + 2 * layer));
      }
      if (PHASE == 1) {
        if (nvalid) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) st4_nt(Hn + ro + nt * cs, rvalid ? relu4(hn[nt]) : zero4());
        }
      } else {
        float qp = 0.f;
        const bool flush = item + 1 >= min(total, it + RUN) || (item + 1) / sb.ntiles != s;  // wave-uniform
        const int slot = 2 * (it / RUN) + (s - it / sb.ntiles);
        float* pt = sb.part + (size_t)slot * SH_PART + eps * 64 + 4 * s4;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float4 h3 = rvalid ? relu4(hn[nt]) : zero4();
          const int f = 16 * nt + 4 * s4;
          qp = fmaf(h3.x, P[PK_WR + 64 + f], qp);
          qp = fmaf(h3.y, P[PK_WR + 65 + f], qp);
          qp = fmaf(h3.z, P[PK_WR + 66 + f], qp);
          qp = fmaf(h3.w, P[PK_WR + 67 + f], qp);
          // the tile's column sums over its SH_NPT nodes (fixed butterfly order), added to the run's in tile order
          float4 csum = h3;
#pragma unroll
          for (int o = SH_EPS; o < 16; o <<= 1) {
            csum.x += __shfl_xor(csum.x, o, 64); csum.y += __shfl_xor(csum.y, o, 64);
            csum.z += __shfl_xor(csum.z, o, 64); csum.w += __shfl_xor(csum.w, o, 64);
          }
          run[nt] = make_float4(run[nt].x + csum.x, run[nt].y + csum.y, run[nt].z + csum.z, run[nt].w + csum.w);
          if (flush) {
            if (kn == 0) st4_nt(pt + 16 * nt, run[nt]);
            run[nt] = zero4();
          }
        }
        qp += __shfl_xor(qp, 16, 64);
        qp += __shfl_xor(qp, 32, 64);
        if (s4 == 0 && rvalid) sb.ql[(size_t)ep * N + n] = qp;
      }
    }
  }
}

// ReadoutLayer (mpnn.py:143-159) + epsilon-greedy act, one wave per episode: column sums from the
// partials (fixed order), p = Wp . mean, q = relu(p) . Wr[:64] + q_local + b, then the act of readout_act.
__global__ __launch_bounds__(256) void shared_readout_kernel(MpnnArgs a, SharedBufs sb) {
  __shared__ float red[4][64];
  const int e = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int N = a.N;
  const float* P = a.P;
  const int s = e / SH_EPS, er = e % SH_EPS;
  {  // the slice's column sums: the partials of the tile groups touching slice s (group g = tiles [g SH_RUN,
     // (g + 1) SH_RUN) of the slice-major order, partial 2 g + (s - first slice of g)); wave w of this block takes
     // groups g0 + w, + 4, ..., the four combined in order
    const int g0 = s * sb.ntiles / SH_RUN, g1 = ((s + 1) * sb.ntiles - 1) / SH_RUN;
    float c0 = 0.f;
    for (int g = g0 + w; g <= g1; g += 4) {
      const int slot = 2 * g + (s - g * SH_RUN / sb.ntiles);
      c0 += sb.part[(size_t)slot * SH_PART + er * 64 + lane];
    }
    red[w][lane] = c0;
  }
  __syncthreads();
  if (w != 0) return;
  const float cs = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  const float mean = cs / (float)N;
  const float* wp = P + PK_WP + lane * 64;
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float4 wr4 = f4(wp + 4 * k);
    p = fmaf(wr4.x, __shfl(mean, 4 * k + 0, 64), p);
    p = fmaf(wr4.y, __shfl(mean, 4 * k + 1, 64), p);
    p = fmaf(wr4.z, __shfl(mean, 4 * k + 2, 64), p);
    p = fmaf(wr4.w, __shfl(mean, 4 * k + 3, 64), p);
  }
  const float cg = wave_sum_f(relu(p) * P[PK_WR + lane]);
  const float br = P[PK_BR];
  const float* qloc = sb.ql + (size_t)e * N;
  const float* xe = a.x + (size_t)e * N * a.xw;
  float bestq = -INFINITY;
  int besti = 0x7fffffff;
  int n_allowed = 0;
  for (int v0 = 0; v0 < N; v0 += 64) {
    const int v = v0 + lane;
    bool allowed = false;
    float qv = -INFINITY;
    if (v < N) {
      qv = cg + qloc[v] + br;
      if (a.q) a.q[(size_t)e * N + v] = qv;
      allowed = a.has_act && (a.act.reversible || xe[(size_t)v * a.xw] == a.act.allowed_value);
    }
    n_allowed += __popcll(__ballot(allowed));
    if (allowed && (qv > bestq || (qv == bestq && v < besti))) { bestq = qv; besti = v; }
  }
  if (!a.has_act) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oq = __shfl_xor(bestq, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    if (oq > bestq || (oq == bestq && oi < besti)) { bestq = oq; besti = oi; }
  }
  int action = besti == 0x7fffffff ? 0 : besti;  // no allowed vertex: argmax of an all-masked row is 0
  const uint64_t r0 = rng3(a.act.seed, a.act.counter, (uint64_t)e);
  if (u01(r0) < a.act.epsilon && n_allowed > 0) {  // random.uniform(0,1) >= eps -> greedy
    const uint64_t r1 = rng3(a.act.seed ^ 0xA5A5A5A5ull, a.act.counter, (uint64_t)e);
    int k = (int)(r1 % (uint64_t)n_allowed);
    if (a.act.reversible) {
      action = k;
    } else {
      action = -1;  // k-th allowed vertex
      for (int v0 = 0; v0 < N && action < 0; v0 += 64) {
        const int v = v0 + lane;
        const bool al = v < N && xe[(size_t)v * a.xw] == a.act.allowed_value;
        const uint64_t bal = __ballot(al);
        const int c = __popcll(bal);
        if (k < c) {
          uint64_t b = bal;
          for (int i = 0; i < k; ++i) b &= b - 1;
          action = v0 + __ffsll((long long)b) - 1;
        } else {
          k -= c;
        }
      }
    }
  }
  if (lane == 0) a.actions[e] = action;
}

static int mpnn_forward_shared_launch(const MpnnArgs& a, void* workspace, hipStream_t st) {
  if (a.N > 2048) return fail(ECO_ERR_ARG, "shared-graph MPNN: N > 2048 does not fit one LDS block");
  SharedBufs sb = shared_carve((float*)((char*)workspace + 256), a.N, a.B);
  uint64_t* key = reinterpret_cast<uint64_t*>((char*)workspace + WS_KEY_OFFSET);
  sb.key = key;
  shared_key_kernel<<<1, SK_THREADS, 0, st>>>(a, key);
  shared_perm_kernel<<<(a.N + 63) / 64, 256, 0, st>>>(a, sb);
  shared_tiles_kernel<<<(sb.nt16 * 2 + ST_THREADS - 1) / ST_THREADS, ST_THREADS, 0, st>>>(a, sb);
  shared_pack_kernel<<<1, SP_THREADS, 0, st>>>(sb);
  const int items = sb.S * 8 * SH_EPS;  // (slice, chunk, episode) blocks
  const int agrid = std::min(items, shared_grid());
  const size_t lds_agg = AG_LDS;
  (void)hipFuncSetAttribute((const void*)shared_agg_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
  (void)hipFuncSetAttribute((const void*)shared_agg_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
  (void)hipFuncSetAttribute((const void*)shared_agg_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
  (void)hipFuncSetAttribute((const void*)shared_agg_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
  const bool wide = a.xw == 16;  // more than 8 observables: the x-build instances for 16-float rows
  if (wide) {
    (void)hipFuncSetAttribute((const void*)shared_agg_kernel<1, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
    (void)hipFuncSetAttribute((const void*)shared_agg_kernel<2, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
    (void)hipFuncSetAttribute((const void*)shared_agg_kernel<3, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_agg);
    (void)hipFuncSetAttribute((const void*)shared_lin_kernel<1, 16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(64 * FH_FRAG * 2));
  }
  const int grid = shared_grid();
  const size_t lds_edge = 16 * FH_FRAG * 2, lds_layer = 64 * FH_FRAG * 2;
  (void)hipFuncSetAttribute((const void*)shared_lin_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_edge);
  (void)hipFuncSetAttribute((const void*)shared_lin_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_layer);
  (void)hipFuncSetAttribute((const void*)shared_lin_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_layer);
  // edge phase: A+ . U (+ A- . V; that pass returns at once on graphs without -1 edges, meta[2] on the device)
  if (wide) {
    shared_agg_kernel<1, 16><<<agrid, 64 * AG_NW16, lds_agg, st>>>(a, sb, nullptr, 1, 0, items);
    shared_agg_kernel<2, 16><<<agrid, 64 * AG_NW16, lds_agg, st>>>(a, sb, nullptr, -1, 1, items);
  } else {
    shared_agg_kernel<1><<<agrid, 64 * AG_NW, lds_agg, st>>>(a, sb, nullptr, 1, 0, items);
    shared_agg_kernel<2><<<agrid, 64 * AG_NW, lds_agg, st>>>(a, sb, nullptr, -1, 1, items);
  }
  shared_lin_kernel<0><<<grid, 64 * SH_NW, lds_edge, st>>>(a, sb, 0, nullptr, nullptr);
  if (wide) {
    shared_agg_kernel<3, 16><<<agrid, 64 * AG_NW16, lds_agg, st>>>(a, sb, nullptr, 0, 0, items);   // A . h0
    shared_lin_kernel<1, 16><<<grid, 64 * SH_NW, lds_layer, st>>>(a, sb, 0, nullptr, sb.HB);     // h1
  } else {
    shared_agg_kernel<3><<<agrid, 64 * AG_NW, lds_agg, st>>>(a, sb, nullptr, 0, 0, items);       // A . h0
    shared_lin_kernel<1><<<grid, 64 * SH_NW, lds_layer, st>>>(a, sb, 0, nullptr, sb.HB);         // h1
  }
  shared_agg_kernel<0><<<agrid, 64 * AG_NW, lds_agg, st>>>(a, sb, sb.HB, 0, 0, items);
  shared_lin_kernel<1><<<grid, 64 * SH_NW, lds_layer, st>>>(a, sb, 1, sb.HB, sb.HA);             // h2
  shared_agg_kernel<0><<<agrid, 64 * AG_NW, lds_agg, st>>>(a, sb, sb.HA, 0, 0, items);
  shared_lin_kernel<2><<<grid, 64 * SH_NW, lds_layer, st>>>(a, sb, 2, sb.HA, nullptr);           // q_local, sums
  shared_readout_kernel<<<a.B, 256, 0, st>>>(a, sb);
  return check_launch("mpnn_forward_shared");
}

}  // namespace eco
