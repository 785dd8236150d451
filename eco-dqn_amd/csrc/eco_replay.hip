// Replay rings of the DQN agent on gfx950 (ReplayBuffer, src/agents/dqn/utils.py:28-83): the fp32 feature ring
// (push, uniform sample, gather by slot) and the compact integer-state ring in its two kinds, MaxCut (CutRing) and
// the five generic-scorer targets (ProbRing).  What the two kinds share -- slots, the Feistel draw, snapshot, push,
// the rebuild of s' and the read kernel -- is written once and instantiated per ring trait.
#include "eco_env_dev.h"

namespace eco {

// ------------------------------------------------------------ feature ring ----
// A device ring of transitions as fp32 feature rows:
// node features of s and s' ([N][x_stride] fp32), graph id, action, reward, done.
__device__ __forceinline__ int xstride(const eco_replay& rb) { return rb.x_stride == 16 ? 16 : 8; }

__global__ void replay_push_kernel(eco_replay rb, int pos, int B, const float* xs, const float* xn,
                                   const int32_t* gids, const int32_t* actions, const double* rewards,
                                   const uint8_t* dones) {
  const int b = blockIdx.y;
  if (b >= B) return;
  const int slot = (int)(((long long)pos + b) % rb.capacity);
  const int per = rb.n_spins * xstride(rb) / 4;  // float4s per state
  const float4* s4 = reinterpret_cast<const float4*>(xs + (size_t)b * rb.n_spins * xstride(rb));
  const float4* n4 = reinterpret_cast<const float4*>(xn + (size_t)b * rb.n_spins * xstride(rb));
  float4* ds = reinterpret_cast<float4*>(rb.xs + (size_t)slot * rb.n_spins * xstride(rb));
  float4* dn = reinterpret_cast<float4*>(rb.xn + (size_t)slot * rb.n_spins * xstride(rb));
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
    ds[i] = s4[i];
    dn[i] = n4[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rb.gid[slot] = gids[b];
    rb.act[slot] = actions[b];
    rb.rew[slot] = (float)rewards[b];  // torch.as_tensor([reward], dtype=torch.float) (dqn.py:299)
    rb.done[slot] = dones[b] ? 1.f : 0.f;
  }
}

// Feistel bijection on [0, 2^bits) with cycle walking into [0, n): distinct indices,
// i.e. sampling WITHOUT replacement like random.sample (dqn/utils.py:53).
__device__ __forceinline__ uint32_t feistel(uint32_t x, int half, uint64_t key) {
  const uint32_t mask = (1u << half) - 1u;
  uint32_t L = x >> half, R = x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint32_t F = (uint32_t)(rng3(key, (uint64_t)r, (uint64_t)R) & mask);
    const uint32_t nL = R;
    R = L ^ F;
    L = nL;
  }
  return (L << half) | R;
}

// the m-th of the distinct uniform positions in [0, size) drawn by `key`
__device__ __forceinline__ uint32_t feistel_draw(uint32_t m, int size, uint64_t key) {
  int bits = 2;
  while ((1 << bits) < size) ++bits;
  if (bits & 1) ++bits;
  const int half = bits / 2;
  uint32_t x = m;
  do { x = feistel(x, half, key); } while (x >= (uint32_t)size);
  return x;
}

// one workgroup copies the transition in `slot` to minibatch row m: float4 copies of the s / s' node-feature rows
// (HBM-bound: 2 x N x x_stride x 4 B per sample)
__device__ __forceinline__ void replay_copy(const eco_replay& rb, int slot, int m, float* xs, float* xn, int32_t* gid,
                                            int32_t* act, float* rew, float* done) {
  const int per = rb.n_spins * xstride(rb) / 4;
  const float4* s4 = reinterpret_cast<const float4*>(rb.xs + (size_t)slot * rb.n_spins * xstride(rb));
  const float4* n4 = reinterpret_cast<const float4*>(rb.xn + (size_t)slot * rb.n_spins * xstride(rb));
  float4* ds = reinterpret_cast<float4*>(xs + (size_t)m * rb.n_spins * xstride(rb));
  float4* dn = reinterpret_cast<float4*>(xn + (size_t)m * rb.n_spins * xstride(rb));
  for (int i = threadIdx.x; i < per; i += blockDim.x) {
    ds[i] = s4[i];
    dn[i] = n4[i];
  }
  if (threadIdx.x == 0) {
    gid[m] = rb.gid[slot];
    act[m] = rb.act[slot];
    rew[m] = rb.rew[slot];
    done[m] = rb.done[slot];
  }
}

// grid (1, M): the m-th of M distinct uniform slots
__global__ void replay_sample_kernel(eco_replay rb, int size, int M, uint64_t key, float* xs, float* xn,
                                     int32_t* gid, int32_t* act, float* rew, float* done) {
  const int m = blockIdx.y;
  if (m >= M) return;
  replay_copy(rb, (int)feistel_draw((uint32_t)m, size, key), m, xs, xn, gid, act, rew, done);
}

// grid M: the transition in slots[m] (the rank-based PER of eco_per.hip chooses the slots on the host)
__global__ __launch_bounds__(256) void replay_gather_kernel(eco_replay rb, int M, const int32_t* slots, float* xs,
                                                           float* xn, int32_t* gid, int32_t* act, float* rew,
                                                           float* done) {
  const int m = blockIdx.x;
  if (m >= M) return;
  const int slot = slots[m];
  if (slot < 0 || slot >= rb.capacity) return;  // rejected on the host; never read outside the ring
  replay_copy(rb, slot, m, xs, xn, gid, act, rew, done);
}

// ------------------------------------------------------------ compact replay ----
// ReplayBuffer of transitions as the env's integer state instead of fp32 feature rows.  A transition stores ONE
// state: s, per vertex one u32 {spin sign bit 31 | time-since-flip count bits 16..30 | an int16 field bits 0..15};
// s' is a deterministic function of s, the action and the graph (the env's step kernel: flip spin a, reset its
// count, count +1 elsewhere, the field += coef(w_aj) s_a over the CSR row of a), rebuilt on sample.  The read kernel
// rebuilds the fp32 feature rows with the env's own statements (the same float64 operations, so the features
// equal, bit for bit, the rows the env wrote).
// Ring of P = capacity + batch slots; transition k (k-th push, counted over the buffer's life) lives in slot
// k % P.  push(k0) writes the s' of episode e straight into slot (k0 + batch + e) % P as the s of that
// episode's next transition (a reset overwrites it through snapshot), so s is never copied; the `batch`
// slots ahead of the newest transition are never sampled (size <= capacity = P - batch).
// Layout: rows [P][N] u32 | ctx_s [P][CS] f64 | ctx_n [P][CS] f64 | gid | act | rew | done [P], CS scalars per state.
// act bit 30 marks a transition whose step left the state unchanged (an auto-masked finished episode).
// The entry points select the ring kind by cfg.optimisation_target:
//
// CutRing, OptimisationTarget.CUT (eco_env.hip): the field is the local field h = (J s)_v (|h| < 2^15, else
// ECO_ERR_GRAPH), updated with coef = -2 w.  Per state CS = 4 scalars {|score - best| / mlr, termination immanency,
// step t, Hamming distance to the best spins} (the Hamming distance needs the best spins, which are not kept).
// 4N + 80 B per transition (880 B at N=200) against 64N of the feature ring.  Expand LDS: N words (the state s').
//
// ProbRing, MIN_COVER, MIN_CUT, MAX_IND_SET, MAX_CLIQUE and MIN_DOM_SET (eco_env_problems.hip): every scorer keeps
// ONE integer neighbour sum F_v per vertex, updated along one CSR row per flip (field_coef), so a transition is
// again one integer state + the action; the field is F_v (|F_v| < 2^15, else ECO_ERR_GRAPH).
// Per state CS = PCS = 6 float64 scalars, the episode quantities of ProbObs that the row and the graph do not determine:
//   [0] step t            (episode time tab[t], termination immanency; t = 0 marks a reset state, whose rows count
//                          validity improvements with 'im > 0' and have zero distance / time scalars)
//   [1] distance from the best solution, |q - q(best)| / mlr (needs the best set's size)
//   [2] Hamming distance to the best spins (not kept)
//   [3] global validity difference (inv - inv(best)) / inorm (needs the best state's invalidity)
//   [4] invalidity normaliser the rows were written with: the graph's own for a stepped state, the PREVIOUS
//       reset's for a reset state (env_reset_problem_kernel's stale_inorm, kept per episode at EnvLayout.off_oinorm)
//   [5] max local reward mlr (a function of the graph alone, but a maximum over all its rows: one more pass over
//       the whole CSR per rebuilt state against 8 B)
// Recomputed on sample from the row and the graph: the set size n1, the invalidity degree inv (the reset kernel's
// closed forms), the validity bit, the per-vertex quality / invalidity / validity-change masks (vertex_masks; for
// MIN_DOM_SET one CSR pass per vertex over the mds_code bytes of the state, as mds_neighbour_counts) and the
// quality / validity improvement counts.  4N + 112 B per transition against 128N of 16-float feature rows.
// Expand LDS: N words (the state, s as well as s') + N bytes (MIN_DOM_SET codes).
constexpr uint32_t CR_NOFLIP = 0x40000000u;

struct CompactRing {
  uint32_t* rows;
  double *ctx_s, *ctx_n;
  int32_t *gid, *act;
  float *rew, *done;
};

// cs: f64 scalars per state (Ring::CS)
static CompactRing compact_carve(void* base, int N, long long P, int cs, size_t* bytes = nullptr) {
  CompactRing r;
  char* b = (char*)base;
  size_t o = 0;
  auto t = [&](size_t n) { void* p = b + o; o = align_up(o + n, 256); return p; };
  r.rows = (uint32_t*)t((size_t)P * N * 4);
  r.ctx_s = (double*)t((size_t)P * cs * 8);
  r.ctx_n = (double*)t((size_t)P * cs * 8);
  r.gid = (int32_t*)t((size_t)P * 4);
  r.act = (int32_t*)t((size_t)P * 4);
  r.rew = (float*)t((size_t)P * 4);
  r.done = (float*)t((size_t)P * 4);
  if (bytes) *bytes = o;
  return r;
}

template <class Ring>
static size_t compact_bytes(int N, long long P) {
  size_t o = 0;
  compact_carve(nullptr, N, P, Ring::CS, &o);
  return o;
}

// sums of a and b over the block (<= 4 waves) through red[8]; the barrier also publishes the caller's LDS writes
__device__ __forceinline__ void block_sum2(int& a, int& b, int* red) {
  a = wave_sum_i(a);
  b = wave_sum_i(b);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[4 + (threadIdx.x >> 6)] = b; }
  __syncthreads();
  a = 0; b = 0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { a += red[k]; b += red[4 + k]; }
}

// Ring traits.  CS: f64 scalars per state; LDS_PER_VERTEX: dynamic LDS bytes of the read kernel per vertex; RED: its
// static ints for expand's block sums; STAGE_S: s goes through LDS like s' (expand rewrites the state in place).
//   pack    episode e's current state (spins, field, time-since-flip counts, scalars) into rows / ctx (and ctx2 when
//           given: the same scalars as the s' of the transition just taken)
//   coef    what a flip of a adds to the field of a neighbour over an edge of weight w, per unit of s_a
//   expand  the feature rows of one compact state, written exactly as the env writes them
struct CutRing {
  static constexpr int CS = 4, LDS_PER_VERTEX = 4, RED = 4;
  static constexpr bool STAGE_S = false;

  static __device__ __forceinline__ void pack(const eco_env_config& cfg, const EnvLayout& L, const uint8_t* state, int e,
                                              uint32_t* rows, double* ctx, double* ctx2, int32_t* err) {
    const int N = L.N;
    const int8_t* sp = (const int8_t*)(state + L.off_spins) + (size_t)e * N;
    const int32_t* hf = (const int32_t*)(state + L.off_field) + (size_t)e * N;
    const int16_t* ts = (const int16_t*)(state + L.off_tsf) + (size_t)e * N;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const int h = hf[v];
      if (h < -32768 || h > 32767) atomicCAS(err, 0, ECO_ERR_GRAPH);  // compact rows need |J s| < 2^15
      rows[v] = (sp[v] < 0 ? 0x80000000u : 0u) | ((uint32_t)(ts[v] & 0x7FFF) << 16) | ((uint32_t)h & 0xFFFFu);
    }
    if (threadIdx.x < 4) {
      const EpScal* sc = (const EpScal*)(state + L.off_scal) + e;
      const int t = sc->t;
      double dist = 0.0, term = 0.0;  // a reset state's rows are 0 (_reset_state never sets them)
      if (t > 0) {
        dist = distance_from_best(sc->score, sc->best_score, sc->mlr);
        term = termination_immanency(cfg, t);
      }
      const double v = threadIdx.x == 0 ? dist : threadIdx.x == 1 ? term : threadIdx.x == 2 ? (double)t
                                                                                            : (double)sc->hamming;
      ctx[threadIdx.x] = v;
      if (ctx2) ctx2[threadIdx.x] = v;
    }
  }

  static __device__ __forceinline__ int coef(int, int w) { return -2 * w; }  // h_j -= 2 w_aj s_a (env_step_kernel)

  // as write_obs does (same obs_value, same casts)
  static __device__ __forceinline__ void expand(const eco_env_config& cfg, const uint32_t* rows, const double* ctx,
                                                const eco_graph_set& gs, int g, const double* tab, int N, float* out,
                                                int* red) {
    const double mlr = gs.meta[(size_t)g * 4];  // issued before the count, needed after it
    int cnt = 0;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const uint32_t w = rows[v];
      const int sv = (w >> 31) ? -1 : 1;
      const int h = (int)(int16_t)(w & 0xFFFFu);
      cnt += (sv * h > 0);
    }
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    int total = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) total += red[k];
    ObsCtx c;
    c.mlr = mlr; c.dist_best = ctx[0]; c.term = ctx[1]; c.hamming = ctx[3];
    const int t = (int)ctx[2];
    c.ep_time = tab[t];
    c.nqi = (double)total / (double)N;
    c.basis = cfg.spin_basis;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const uint32_t w = rows[v];
      const int sv = (w >> 31) ? -1 : 1;
      const int tsfk = (int)((w >> 16) & 0x7FFFu);
      const int h = (int)(int16_t)(w & 0xFFFFu);
      float xf[ECO_MAX_OBS];
#pragma unroll
      for (int i = 0; i < ECO_MAX_OBS; ++i) xf[i] = i < cfg.n_obs ? (float)obs_value(cfg.obs_ids[i], c, sv, h, tsfk, tab) : 0.f;
      store_obs_row(out, (size_t)v, cfg.n_obs, xf);
    }
  }
};

constexpr int PCS = 6;
enum { PC_T = 0, PC_DIST = 1, PC_HAM = 2, PC_GVD = 3, PC_INORM = 4, PC_MLR = 5 };

struct ProbRing {
  static constexpr int CS = PCS, LDS_PER_VERTEX = 5, RED = 16;
  static constexpr bool STAGE_S = true;

  static __device__ __forceinline__ void pack(const eco_env_config& cfg, const EnvLayout& L, const uint8_t* state, int e,
                                              uint32_t* rows, double* ctx, double* ctx2, int32_t* err) {
    const int N = L.N;
    const int8_t* sp = (const int8_t*)(state + L.off_spins) + (size_t)e * N;
    const int32_t* gF = (const int32_t*)(state + L.off_field) + (size_t)e * N;
    const int16_t* ts = (const int16_t*)(state + L.off_tsf) + (size_t)e * N;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const int f = gF[v];
      if (f < -32767 || f > 32767) atomicCAS(err, 0, ECO_ERR_GRAPH);  // F and the masks s F, -s F must fit an int16
      rows[v] = (sp[v] < 0 ? 0x80000000u : 0u) | ((uint32_t)(ts[v] & 0x7FFF) << 16) | ((uint32_t)f & 0xFFFFu);
    }
    if (threadIdx.x < PCS) {
      const EpScal* sc = (const EpScal*)(state + L.off_scal) + e;
      const int tgt = cfg.optimisation_target;
      const int t = sc->t;
      // a reset state's scalars are 0 and its normaliser is the previous reset's (env_reset_problem_kernel)
      double dist = 0.0, gvd = 0.0, inorm = ((const double*)(state + L.off_oinorm))[e];
      if (t > 0) {  // env_step_problem_kernel's statements on the values it left in the record
        inorm = sc->inorm;
        dist = tgt == ECO_TARGET_MIN_CUT ? distance_from_best(sc->score, sc->best_score, sc->mlr)
                                         : set_distance_from_best(tgt, sc->n1, sc->best_n1, N, sc->mlr);
        gvd = (double)(sc->inv - sc->best_inv) / inorm;
      }
      double v;
      switch (threadIdx.x) {
        case PC_T: v = (double)t; break;
        case PC_DIST: v = dist; break;
        case PC_HAM: v = (double)sc->hamming; break;
        case PC_GVD: v = gvd; break;
        case PC_INORM: v = inorm; break;
        default: v = sc->mlr; break;
      }
      ctx[threadIdx.x] = v;
      if (ctx2) ctx2[threadIdx.x] = v;
    }
  }

  static __device__ __forceinline__ int coef(int tgt, int w) { return field_coef(tgt, w); }

  // the state in LDS (st[N], each word read and rewritten by its own thread only, then N code bytes), written with
  // write_prob_obs's statements: vertex_masks, vm = (inv + im) == 0, prob_obs_value and the same casts
  static __device__ __forceinline__ void expand(const eco_env_config& cfg, uint32_t* st, const double* ctx,
                                                const eco_graph_set& gs, int g, const double* tab, int N, float* out,
                                                int* red) {
    uint8_t* code = reinterpret_cast<uint8_t*>(st + N);
    const int32_t* rp = gs.row_ptr + (size_t)g * (N + 1);
    const uint32_t* ed = gs.edges + gs.edge_base[g];
    const int tgt = cfg.optimisation_target;
    const bool cut_like = tgt == ECO_TARGET_MIN_CUT;
    const int t = (int)ctx[PC_T];
    // set size and invalidity degree (env_reset_problem_kernel's closed forms; the step's running inv equals them)
    int n1 = 0, isum = 0;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const uint32_t w = st[v];
      const int s = (w >> 31) ? -1 : 1;
      const int F = (int)(int16_t)(w & 0xFFFFu);
      n1 += s > 0;
      switch (tgt) {
        case ECO_TARGET_MIN_COVER: if (s < 0) isum += F; break;
        case ECO_TARGET_MIN_DOM_SET: isum += (s < 0 && F == 0); code[v] = mds_code(s, F); break;
        case ECO_TARGET_MIN_CUT: break;
        default: if (s > 0) isum += F; break;  // MAX_IND_SET / MAX_CLIQUE
      }
    }
    block_sum2(n1, isum, red);
    int inv = 0;
    switch (tgt) {
      case ECO_TARGET_MIN_COVER:
      case ECO_TARGET_MAX_IND_SET: inv = isum / 2; break;
      case ECO_TARGET_MAX_CLIQUE: inv = n1 * (n1 - 1) - isum; break;
      case ECO_TARGET_MIN_DOM_SET: inv = isum; break;
      default: break;
    }
    // masks; a set problem's im replaces F in the word (its qm is +-s), MIN_CUT keeps F (qm = -s F, im = 0)
    int nqi = 0, nvi = 0;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const uint32_t w = st[v];
      const int s = (w >> 31) ? -1 : 1;
      const int F = (int)(int16_t)(w & 0xFFFFu);
      int S0 = 0, S1 = 0;
      if (tgt == ECO_TARGET_MIN_DOM_SET) {
        const int q1 = rp[v + 1];
        int q = rp[v];
        for (; q + 4 <= q1; q += 4) {  // four independent edge loads in flight (mds_neighbour_counts)
          uint32_t x[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) x[u] = ed[q + u];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint8_t c = edge_w(x[u]) > 0 ? code[edge_col(x[u])] : (uint8_t)0;
            S0 += c & 1;
            S1 += c >> 1;
          }
        }
        for (; q < q1; ++q) {
          const uint32_t x = ed[q];
          const uint8_t c = edge_w(x) > 0 ? code[edge_col(x)] : (uint8_t)0;
          S0 += c & 1;
          S1 += c >> 1;
        }
      }
      int qm, im;
      vertex_masks(tgt, s, F, n1, S0, S1, qm, im);
      nqi += qm > 0;
      nvi += t == 0 ? im > 0 : im < 0;  // '> 0' at reset, '< 0' in step
      if (!cut_like) st[v] = (w & 0xFFFF0000u) | ((uint32_t)im & 0xFFFFu);
    }
    block_sum2(nqi, nvi, red + 8);
    ProbObs c;
    c.mlr = ctx[PC_MLR]; c.inorm = ctx[PC_INORM];
    c.dist_best = ctx[PC_DIST]; c.hamming = ctx[PC_HAM]; c.gvd = ctx[PC_GVD];
    c.nqi = (double)nqi / (double)N;
    c.nvi = (double)nvi / (double)N;
    c.term = 0.0; c.ep_time = 0.0;
    if (t > 0) {
      c.term = termination_immanency(cfg, t);
      c.ep_time = tab[t];
    }
    c.valid = inv == 0 ? 1.0 : 0.0;
    c.basis = cfg.spin_basis;
    for (int v = threadIdx.x; v < N; v += blockDim.x) {
      const uint32_t w = st[v];
      const int s = (w >> 31) ? -1 : 1;
      const int tsfk = (int)((w >> 16) & 0x7FFFu);
      const int lo = (int)(int16_t)(w & 0xFFFFu);
      int qm, im;
      vertex_masks(tgt, s, cut_like ? lo : 0, 0, 0, 0, qm, im);  // qm; a set problem's im is the stored one
      if (!cut_like) im = lo;
      const int vm = (inv + im) == 0;
      float xf[ECO_MAX_OBS];
#pragma unroll
      for (int i = 0; i < ECO_MAX_OBS; ++i)
        xf[i] = i < cfg.n_obs ? (float)prob_obs_value(cfg.obs_ids[i], c, s, qm, im, vm, tsfk, tab, cut_like) : 0.f;
      store_obs_row(out, (size_t)v, cfg.n_obs, xf);
    }
  }
};

__device__ __forceinline__ long long cr_slot(long long k, long long P) { return k % P; }

// The slot of the transition at LOGICAL position x: the slot the fp32 feature ring would read (replay_sample_kernel:
// slot x of a ring of `capacity` written at k % capacity); here it is resolved to the transition k == x (mod
// capacity) among the newest `size` and read from slot k % P.
__device__ __forceinline__ long long compact_slot_of(uint32_t x, int capacity, int size, long long pushed, long long P) {
  const long long base = pushed - size;  // oldest transition still held
  const long long k = base + (((long long)x - base % capacity) % capacity + capacity) % capacity;
  return cr_slot(k, P);
}

template <class Ring>
__global__ __launch_bounds__(256) void replay_compact_snapshot_kernel(eco_env_config cfg, EnvLayout L, const uint8_t* state,
                                                                      CompactRing r, long long P, long long pushed,
                                                                      const uint8_t* mask, int32_t* err) {
  const int e = blockIdx.x;
  if (mask && !mask[e]) return;
  const long long slot = cr_slot(pushed + e, P);
  Ring::pack(cfg, L, state, e, r.rows + slot * L.N, r.ctx_s + slot * Ring::CS, nullptr, err);
}

template <class Ring>
__global__ __launch_bounds__(256) void replay_compact_push_kernel(eco_env_config cfg, EnvLayout L, const uint8_t* state,
                                                                  CompactRing r, long long P, long long pushed, int B,
                                                                  const int32_t* actions, const double* rewards,
                                                                  const uint8_t* dones, int32_t* err) {
  const int e = blockIdx.x;
  const int N = L.N;
  const long long slot = cr_slot(pushed + e, P), next = cr_slot(pushed + B + e, P);
  if (threadIdx.x == 0) {
    const int a = actions[e];
    // did the step flip spin a (s' != s)?  An auto-masked finished episode returns its state unchanged.
    const bool flipped = a >= 0 && a < N &&
                         ((r.rows[slot * N + a] >> 31) != (uint32_t)(((const int8_t*)(state + L.off_spins))[(size_t)e * N + a] < 0));
    r.gid[slot] = ((const EpScal*)(state + L.off_scal) + e)->graph;
    r.act[slot] = (int32_t)((uint32_t)a | (flipped ? 0u : CR_NOFLIP));
    r.rew[slot] = (float)rewards[e];  // torch.as_tensor([reward], dtype=torch.float) (dqn.py:299)
    r.done[slot] = dones[e] ? 1.f : 0.f;
  }
  Ring::pack(cfg, L, state, e, r.rows + next * N, r.ctx_s + next * Ring::CS, r.ctx_n + slot * Ring::CS, err);
}

// The state `rows` into LDS st[N]; with `flip`, advanced by the env step of action a (env_step_kernel,
// spinsystem.py:397, :492-497; env_step_problem_kernel): flip a, reset its count, count +1 elsewhere (mod 2^15),
// then the field along the CSR row of a.  push sets CR_NOFLIP unless 0 <= a < N, so a is a vertex whenever flip is set.
template <class Ring>
__device__ __forceinline__ void compact_advance(int tgt, const uint32_t* rows, bool flip, int a,
                                                const eco_graph_set& gs, int g, int N, uint32_t* st) {
  for (int v = threadIdx.x; v < N; v += blockDim.x) {
    uint32_t w = rows[v];
    if (flip) {
      const uint32_t tsfk = v == a ? 0u : (((w >> 16) & 0x7FFFu) + 1u) & 0x7FFFu;
      w = ((v == a ? ~w : w) & 0x80000000u) | (tsfk << 16) | (w & 0xFFFFu);
    }
    st[v] = w;
  }
  __syncthreads();
  if (flip) {
    const int sa_old = (rows[a] >> 31) ? -1 : 1;
    const int32_t* rp = gs.row_ptr + (size_t)g * (N + 1);
    const uint32_t* ed = gs.edges + gs.edge_base[g];
    for (int q = rp[a] + threadIdx.x; q < rp[a + 1]; q += blockDim.x) {
      const uint32_t ex = ed[q];
      const int j = edge_col(ex);
      const uint32_t w = st[j];
      const int f = (int)(int16_t)(w & 0xFFFFu) + Ring::coef(tgt, edge_w(ex)) * sa_old;
      st[j] = (w & 0xFFFF0000u) | ((uint32_t)f & 0xFFFFu);
    }
    __syncthreads();
  }
}

// grid (2, M): blockIdx.x = 0 rebuilds s, 1 rebuilds s' of the m-th minibatch row.  GATHER: from the transition at
// logical position idx[m] (DEVICE int32, each in [0, size); others are skipped); else from the m-th of M distinct
// uniform positions (Feistel walk keyed by `key`, as replay_sample_kernel).
template <class Ring, bool GATHER>
__global__ __launch_bounds__(256) void replay_compact_read_kernel(eco_env_config cfg, CompactRing r, long long P,
                                                                  int capacity, int size, long long pushed, int M,
                                                                  const int32_t* idx, uint64_t key, const double* tab,
                                                                  eco_graph_set gs, float* xs, float* xn, int32_t* gid,
                                                                  int32_t* act, float* rew, float* done) {
  extern __shared__ uint32_t cr_lds[];
  __shared__ int red[Ring::RED];
  const int m = blockIdx.y;
  if (m >= M) return;
  uint32_t x;
  if (GATHER) {
    const int xi = idx[m];
    if ((unsigned)xi >= (unsigned)size) return;  // never read outside the stored transitions
    x = (uint32_t)xi;
  } else {
    x = feistel_draw((uint32_t)m, size, key);
  }
  const long long slot = compact_slot_of(x, capacity, size, pushed, P);
  const int N = cfg.n_spins;
  const int W = ECO_OBS_X_STRIDE(cfg.n_obs);
  const int g = r.gid[slot];
  const uint32_t* rows = r.rows + slot * N;
  const uint32_t av = (uint32_t)r.act[slot];
  const int a = (int)(av & ~CR_NOFLIP);
  const bool next = blockIdx.x == 1;
  if (!next && threadIdx.x == 0) { gid[m] = g; act[m] = a; rew[m] = r.rew[slot]; done[m] = r.done[slot]; }
  const double* ctx = (next ? r.ctx_n : r.ctx_s) + slot * Ring::CS;
  float* out = (next ? xn : xs) + (size_t)m * N * W;
  if (Ring::STAGE_S || next) {
    compact_advance<Ring>(cfg.optimisation_target, rows, next && !(av & CR_NOFLIP), a, gs, g, N, cr_lds);
    Ring::expand(cfg, cr_lds, ctx, gs, g, tab, N, out, red);
  } else if constexpr (!Ring::STAGE_S) {
    Ring::expand(cfg, rows, ctx, gs, g, tab, N, out, red);  // s straight from the ring rows: no LDS staging pass
  }
}

}  // namespace eco

using namespace eco;

extern "C" int eco_replay_push(const eco_replay* rb, int32_t pos, int32_t batch, const float* xs, const float* xn,
                               const int32_t* graph_ids, const int32_t* actions, const double* rewards,
                               const uint8_t* dones, eco_stream_t stream) {
  if (!rb || !xs || !xn || !graph_ids || !actions || !rewards || !dones) return fail(ECO_ERR_ARG, "null argument");
  if (rb->x_stride != 0 && rb->x_stride != 8 && rb->x_stride != 16) return fail(ECO_ERR_ARG, "x_stride must be 8 or 16");
  if (batch < 1 || rb->capacity < 1 || pos < 0) return fail(ECO_ERR_ARG, "bad batch/capacity/pos");
  if (batch > rb->capacity) return fail(ECO_ERR_ARG, "replay push: batch larger than the ring (slots would collide)");
  replay_push_kernel<<<dim3(1, batch), 256, 0, (hipStream_t)stream>>>(*rb, pos, batch, xs, xn, graph_ids, actions,
                                                                      rewards, dones);
  return check_launch("replay_push");
}

extern "C" int eco_replay_sample(const eco_replay* rb, int32_t size, int32_t m, uint64_t seed, uint64_t counter,
                                 float* xs, float* xn, int32_t* graph_ids, int32_t* actions, float* rewards,
                                 float* dones, eco_stream_t stream) {
  if (!rb || !xs || !xn || !graph_ids || !actions || !rewards || !dones) return fail(ECO_ERR_ARG, "null argument");
  if (rb->x_stride != 0 && rb->x_stride != 8 && rb->x_stride != 16) return fail(ECO_ERR_ARG, "x_stride must be 8 or 16");
  if (size < m || m < 1 || size > rb->capacity)
    return fail(ECO_ERR_ARG, "replay sample: need m <= size <= capacity (random.sample without replacement)");
  replay_sample_kernel<<<dim3(1, m), 256, 0, (hipStream_t)stream>>>(*rb, size, m, rng3(seed, counter, 0x5A5A),
                                                                    xs, xn, graph_ids, actions, rewards, dones);
  return check_launch("replay_sample");
}

// slots: DEVICE int32 [m], each in [0, capacity) (host-checked by the Python wrapper from the buffer
// positions eco_per_sample returned).
extern "C" int eco_replay_gather(const eco_replay* rb, int32_t m, const int32_t* slots, float* xs, float* xn,
                                 int32_t* graph_ids, int32_t* actions, float* rewards, float* dones,
                                 eco_stream_t stream) {
  if (m < 0 || rb->capacity < 1) return fail(ECO_ERR_ARG, "replay gather: bad size");
  if (m == 0) return ECO_OK;
  replay_gather_kernel<<<m, 256, 0, (hipStream_t)stream>>>(*rb, m, slots, xs, xn, graph_ids, actions, rewards, dones);
  return check_launch("replay_gather");
}

// the five generic-scorer targets of the compact ring (eco_env_problems.hip)
static bool compact_generic(const eco_env_config* cfg) {
  return cfg->optimisation_target >= ECO_TARGET_MIN_COVER && cfg->optimisation_target <= ECO_TARGET_MIN_DOM_SET;
}

static int compact_check(const eco_env_config* cfg, int32_t batch, int32_t capacity) {
  if (!cfg) return fail(ECO_ERR_ARG, "null config");
  const bool generic = compact_generic(cfg);
  if (cfg->optimisation_target != ECO_TARGET_CUT && !generic)
    return fail(ECO_ERR_TARGET, "compact replay: OptimisationTarget CUT, MIN_COVER, MIN_CUT, MAX_IND_SET, MAX_CLIQUE "
                                "or MIN_DOM_SET");
  if (cfg->float_weights)
    return fail(ECO_ERR_ARG, "compact replay: integer weights only (its local field is an int16); a float-weighted "
                             "env uses the feature ring (eco_replay_push / eco_replay_sample)");
  if (cfg->max_steps > 32767) return fail(ECO_ERR_ARG, "compact replay: max_steps must be < 32768");
  if (cfg->n_spins < 1 || cfg->n_spins > ECO_COMPACT_MAX_SPINS) return fail(ECO_ERR_ARG, "compact replay: n_spins out of range");
  if (generic && cfg->n_spins > ECO_MAX_SPINS)
    return fail(ECO_ERR_ARG, "compact replay: the generic-scorer targets take n_spins <= " + std::to_string(ECO_MAX_SPINS) +
                                 " (OptimisationTarget.CUT: " + std::to_string(ECO_COMPACT_MAX_SPINS) + ")");
  if (batch < 1 || capacity < 1) return fail(ECO_ERR_ARG, "bad batch/capacity");
  return ECO_OK;
}

// f(CutRing{}) or f(ProbRing{}), by the target of a checked config
template <class F>
static auto compact_dispatch(const eco_env_config* cfg, F&& f) {
  return compact_generic(cfg) ? f(ProbRing{}) : f(CutRing{});
}

// what every launch on a compact ring needs, from a checked config
struct CompactCtx {
  bool generic;
  EnvLayout L;
  long long P;        // ring slots
  const double* tab;  // the env's episode-time table
  CompactRing r;
  int nt;             // threads of the read kernel
  size_t lds;         // its dynamic LDS bytes
  hipStream_t st;
};

static CompactCtx compact_ctx(const eco_env_config* cfg, const void* env_state, const void* ring, int32_t capacity,
                              int32_t batch, eco_stream_t stream) {
  CompactCtx c;
  const int N = cfg->n_spins;
  c.generic = compact_generic(cfg);
  c.L = env_layout(N, cfg->max_steps, batch, 0, c.generic);
  c.P = (long long)capacity + batch;
  c.tab = (const double*)((const uint8_t*)env_state + c.L.off_tab + 256);
  c.r = compact_carve(const_cast<void*>(ring), N, c.P, c.generic ? ProbRing::CS : CutRing::CS);
  // threads per transition: 4096 workgroups of a few nodes' work each are latency chains (ring slot -> graph ->
  // rows -> count -> features); smaller workgroups keep more of them resident
  // (ER-200 x M = 2048: 30.6 / 24.2 / 21.0 us per call at 256 / 128 / 64 threads, profiles/r03/ab/sample_threads_*)
  c.nt = N <= 256 ? 64 : 128;
  c.lds = (size_t)N * (c.generic ? ProbRing::LDS_PER_VERTEX : CutRing::LDS_PER_VERTEX);
  c.st = (hipStream_t)stream;
  return c;
}

extern "C" size_t eco_replay_compact_bytes(int32_t n_spins, int32_t capacity, int32_t batch) {
  if (n_spins < 1 || n_spins > ECO_COMPACT_MAX_SPINS || capacity < 1 || batch < 1) return 0;
  return compact_bytes<CutRing>(n_spins, (long long)capacity + batch);
}

extern "C" size_t eco_replay_compact_bytes_cfg(const eco_env_config* cfg, int32_t capacity, int32_t batch) {
  if (compact_check(cfg, batch, capacity) != ECO_OK) return 0;
  return compact_dispatch(cfg, [&](auto ring) {
    return compact_bytes<decltype(ring)>(cfg->n_spins, (long long)capacity + batch);
  });
}

extern "C" int eco_replay_compact_snapshot(const eco_env_config* cfg, const void* env_state, int32_t batch, void* ring,
                                           int32_t capacity, int64_t pushed, const uint8_t* mask, eco_stream_t stream) {
  int rc = compact_check(cfg, batch, capacity);
  if (rc) return rc;
  if (!env_state || !ring || pushed < 0) return fail(ECO_ERR_ARG, "null state/ring or negative push count");
  const CompactCtx c = compact_ctx(cfg, env_state, ring, capacity, batch, stream);
  compact_dispatch(cfg, [&](auto ring_tag) {
    replay_compact_snapshot_kernel<decltype(ring_tag)><<<batch, 256, 0, c.st>>>(
        *cfg, c.L, (const uint8_t*)env_state, c.r, c.P, pushed, mask, err_word());
  });
  return check_launch(c.generic ? "replay_compact_snapshot (generic scorer)" : "replay_compact_snapshot");
}

extern "C" int eco_replay_compact_push(const eco_env_config* cfg, const void* env_state, int32_t batch, void* ring,
                                       int32_t capacity, int64_t pushed, const int32_t* actions, const double* rewards,
                                       const uint8_t* dones, eco_stream_t stream) {
  int rc = compact_check(cfg, batch, capacity);
  if (rc) return rc;
  if (!env_state || !ring || !actions || !rewards || !dones) return fail(ECO_ERR_ARG, "null argument");
  if (pushed < 0 || batch > capacity) return fail(ECO_ERR_ARG, "replay push: negative push count or batch larger than the ring");
  const CompactCtx c = compact_ctx(cfg, env_state, ring, capacity, batch, stream);
  compact_dispatch(cfg, [&](auto ring_tag) {
    replay_compact_push_kernel<decltype(ring_tag)><<<batch, 256, 0, c.st>>>(
        *cfg, c.L, (const uint8_t*)env_state, c.r, c.P, pushed, batch, actions, rewards, dones, err_word());
  });
  return check_launch(c.generic ? "replay_compact_push (generic scorer)" : "replay_compact_push");
}

// the checks shared by eco_replay_compact_sample and eco_replay_compact_gather
static int compact_read_check(const eco_env_config* cfg, const void* env_state, const eco_graph_set* gs,
                              int32_t env_batch, const void* ring, int32_t capacity, int32_t size, int64_t pushed,
                              int32_t m, float* xs, float* xn, int32_t* graph_ids, int32_t* actions, float* rewards,
                              float* dones) {
  int rc = compact_check(cfg, env_batch, capacity);
  if (rc) return rc;
  if (!env_state || !gs || !ring || !xs || !xn || !graph_ids || !actions || !rewards || !dones)
    return fail(ECO_ERR_ARG, "null argument");
  if (m < 1 || size < 1 || size > capacity || pushed < size)
    return fail(ECO_ERR_ARG, "replay sample: need m >= 1 and 1 <= size <= min(capacity, pushed)");
  if (gs->n_spins != cfg->n_spins) return fail(ECO_ERR_ARG, "replay sample: graph set / env size mismatch");
  if (gs->edge_weights) return fail(ECO_ERR_ARG, "compact replay: integer weights only (float-weighted graph set)");
  return ECO_OK;
}

extern "C" int eco_replay_compact_sample(const eco_env_config* cfg, const void* env_state, const eco_graph_set* gs,
                                         int32_t env_batch, const void* ring, int32_t capacity, int32_t size,
                                         int64_t pushed, int32_t m, uint64_t seed, uint64_t counter, float* xs,
                                         float* xn, int32_t* graph_ids, int32_t* actions, float* rewards, float* dones,
                                         eco_stream_t stream) {
  const int rc = compact_read_check(cfg, env_state, gs, env_batch, ring, capacity, size, pushed, m, xs, xn, graph_ids,
                                    actions, rewards, dones);
  if (rc) return rc;
  if (size < m)
    return fail(ECO_ERR_ARG, "replay sample: need m <= size <= min(capacity, pushed) (random.sample without replacement)");
  const CompactCtx c = compact_ctx(cfg, env_state, ring, capacity, env_batch, stream);
  compact_dispatch(cfg, [&](auto ring_tag) {
    replay_compact_read_kernel<decltype(ring_tag), false><<<dim3(2, m), c.nt, c.lds, c.st>>>(
        *cfg, c.r, c.P, capacity, size, pushed, m, nullptr, rng3(seed, counter, 0x5A5A), c.tab, *gs, xs, xn, graph_ids,
        actions, rewards, dones);
  });
  return check_launch(c.generic ? "replay_compact_sample (generic scorer)" : "replay_compact_sample");
}

extern "C" int eco_replay_compact_gather(const eco_env_config* cfg, const void* env_state, const eco_graph_set* gs,
                                         int32_t env_batch, const void* ring, int32_t capacity, int32_t size,
                                         int64_t pushed, int32_t m, const int32_t* idx, float* xs, float* xn,
                                         int32_t* graph_ids, int32_t* actions, float* rewards, float* dones,
                                         eco_stream_t stream) {
  if (!idx) return fail(ECO_ERR_ARG, "replay gather: null idx");
  const int rc = compact_read_check(cfg, env_state, gs, env_batch, ring, capacity, size, pushed, m, xs, xn, graph_ids,
                                    actions, rewards, dones);
  if (rc) return rc;
  const CompactCtx c = compact_ctx(cfg, env_state, ring, capacity, env_batch, stream);
  compact_dispatch(cfg, [&](auto ring_tag) {
    replay_compact_read_kernel<decltype(ring_tag), true><<<dim3(2, m), c.nt, c.lds, c.st>>>(
        *cfg, c.r, c.P, capacity, size, pushed, m, idx, 0, c.tab, *gs, xs, xn, graph_ids, actions, rewards, dones);
  });
  return check_launch(c.generic ? "replay_compact_gather (generic scorer)" : "replay_compact_gather");
}
