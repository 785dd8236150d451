// Batched MaxCut SpinSystem for ECO_MAX_SPINS < N <= ECO_MAX_SPINS_WG: the workgroup-per-episode kernels.
//
// The wave-per-episode kernels of eco_env.hip keep an episode in the registers of one 64-lane wave, 32 vertices
// per lane at most (N <= 2048).  Here ONE 256-thread workgroup (four waves) owns one episode: vertex v lives in
// thread v & 255, slot v >> 8, up to 32 slots (N <= 8192); spins, the local field h = J.s and the
// time-since-flip counters stay in registers exactly as there.  What was a wave ballot / popcount becomes two
// levels -- the wave's ballot, then the four wave results combined through a few words of LDS -- and the episode
// scalars, wave-uniform there, are block-uniform here: every thread computes them from the same inputs by the
// same f64 operations and thread 0 stores them.  Wave w's ballot of slot k covers vertices 256 k + 64 w ..
// + 63, i.e. it IS word 4 k + w of the visited-set state, so the visited set keeps its layout (words =
// ceil(N / 64) per state, Zobrist hash + full compare, initial state not inserted).
//
// The flip scatters the CSR row of the flipped vertex as int32 deltas into the LDS array d[N] (32 KB at
// N = 8192) and the owning threads add them.  OptimisationTarget.CUT with integer weights only (the host
// rejects float-weighted sets and the generic-scorer targets above ECO_MAX_SPINS); both spin bases, reversible and
// irreversible spins, every Stopping mode, the DEFAULT_OBSERVABLES fast write and the general observable write.
// Semantics: spinsystem.py:183-259, :283-330 (reset) and :355-559 (step); the episode logic (initial spin, reward,
// stopping, observation rows, the greedy compare) is the one copy of eco_env_dev.h that eco_env.hip calls too.  No
// atomics beyond the error word's atomicCAS the existing kernels use.
//
// Budget of env_step_wg_kernel<32> (N = 8192): dynamic LDS 4 N = 32 KB + 80 B static; per thread 32 slots x
// {s, h, tsf, best} = 128 VGPRs of state, the slot's g and the 64-bit ballots are transient (the build reports
// the totals: see DESIGN section 22).  One workgroup is one wave per SIMD, so up to four episodes share a CU by
// LDS (160 KB) and registers (512 per SIMD lane).
#include "eco_common.h"
#include "eco_env_dev.h"

namespace eco {
namespace {

constexpr int WG_NT = 256;  // threads per episode
constexpr int WG_NW = 4;    // waves per episode

// SpinSystemBase.reset (spinsystem.py:183-259) + _reset_state (:283-330); one workgroup per episode.
template <int VPT>
__global__ __launch_bounds__(WG_NT) void env_reset_wg_kernel(EnvArgs a) {
  extern __shared__ int8_t s_lds[];  // [N] spins staged for the J.s matvec
  __shared__ long long r_sg[WG_NW];
  __shared__ int r_cnt[WG_NW], r_n1[WG_NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int e = blockIdx.x;
  if (e >= a.B) return;
  if (a.mask && !a.mask[e]) return;
  const int N = a.cfg.n_spins;
  const EnvLayout& L = a.L;
  const int gid = uniform_i(a.graph_ids[e]);
  if (gid < 0 || gid >= a.gs.n_graphs || !a.gs.valid[gid]) {  // block-uniform: every thread returns
    if (tid == 0) atomicCAS(a.err, 0, ECO_ERR_GRAPH);
    return;
  }
  const double* meta = a.gs.meta + (size_t)gid * 4;
  const double mlr = meta[0], qn = meta[1], lb = meta[2];
  const long long sumJ = (long long)meta[3];
  int s[VPT], tsf[VPT], h[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    int sv = 0;
    if (v < N) {
      sv = initial_spin(a, e, v);
      s_lds[v] = (int8_t)sv;
    }
    s[k] = sv;
    tsf[k] = 0;
  }
  __syncthreads();
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* ed = a.gs.edges + a.gs.edge_base[gid];
  long long sg = 0;
  int cnt = 0, n1 = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    int hv = 0;
    if (v < N) {
      const int q1 = rp[v + 1];
      for (int q = rp[v]; q < q1; ++q) {
        const uint32_t x = ed[q];
        const int c = edge_col(x);
        if (c < N) hv += edge_w(x) * (int)s_lds[c];
      }
    }
    h[k] = hv;
    const int g = s[k] * hv;  // calculate_cut_changes: s * (J @ s)
    sg += g;
    cnt += (g > 0);
    n1 += (s[k] > 0);
  }
  sg = wave_sum_ll(sg);
  cnt = wave_sum_i(cnt);
  n1 = wave_sum_i(n1);
  if (lane == 0) { r_sg[wv] = sg; r_cnt[wv] = cnt; r_n1[wv] = n1; }
  __syncthreads();
  sg = r_sg[0] + r_sg[1] + r_sg[2] + r_sg[3];  // integers: exact in any order
  cnt = r_cnt[0] + r_cnt[1] + r_cnt[2] + r_cnt[3];
  n1 = r_n1[0] + r_n1[1] + r_n1[2] + r_n1[3];
  // calculate_cut = 1/4 sum J (1 - s s^T) = (sum J - s.Js)/4, exact integer for integer weights
  const double cut = (double)((sumJ - sg) / 4);
  const double lbabs = lb < 0.0 ? -lb : lb;
  const double score = cut + lbabs;   // MaximizationProblem.get_score (score_solver.py:182-188)
  const double nscore = score / qn;   // get_normalized_score (:190-194)
  const EpRows<int32_t> rows(a, e);
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    if (v < N) { rows.spins[v] = (int8_t)s[k]; rows.field[v] = h[k]; rows.tsf[v] = 0; rows.best[v] = (int8_t)s[k]; }
  }
  uint32_t* vidx = (uint32_t*)(a.state + L.off_vidx) + (size_t)e * L.cap;
  for (int i = tid; i < L.cap; i += WG_NT) vidx[i] = 0u;
  if (tid == 0) store_reset_scalars(scal_ptr(a) + e, score, nscore, cut, mlr, qn, lb, 1.0, gid, n1, 0);
  ObsCtx c;
  c.mlr = mlr; c.dist_best = 0.0; c.hamming = 0.0; c.nqi = (double)cnt / (double)N;
  c.term = 0.0; c.ep_time = 0.0; c.basis = a.cfg.spin_basis;
  write_obs<VPT, WG_NT, int>(a, e, tid, s, h, tsf, c);
}

// SpinSystemBase.step (spinsystem.py:355-559), ExtraAction.NONE, memory_length None; one workgroup per episode.
// FASTOBS: DEFAULT_OBSERVABLES, fp32 rows only.
template <int VPT, bool FASTOBS>
__global__ __launch_bounds__(WG_NT) void env_step_wg_kernel(EnvArgs a) {
  extern __shared__ int32_t d_lds[];  // [N] row deltas of the flip
  __shared__ int r_cnt[WG_NW], r_neg[WG_NW], r_ham[WG_NW];
  __shared__ int r_same[2][WG_NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int e = blockIdx.x;
  if (e >= a.B) return;
  const int N = a.cfg.n_spins;
  const int T = a.cfg.max_steps;
  const EnvLayout& L = a.L;
  EpScal* sc = scal_ptr(a) + e;
  const int act = uniform_i(a.actions[e]);
  // block-uniform exits: every thread of the episode takes them together, before the first barrier
  if (uniform_i(sc->done)) {  // auto-masked
    if (tid == 0) { a.rewards[e] = 0.0; a.dones[e] = 1; }
    return;
  }
  if (act < 0 || act >= N) {
    if (tid == 0) { atomicCAS(a.err, 0, ECO_ERR_ARG); a.rewards[e] = 0.0; a.dones[e] = 0; }
    return;
  }
  // the episode's scalars, read by every thread before the first barrier; thread 0 stores the new ones after the
  // last one
  const int t = sc->t + 1;  // :362
  const double qn = sc->qn, mlr = sc->mlr, lbabs = sc->lbabs;
  const double score0 = sc->score, nscore0 = sc->nscore;
  const double best_score = sc->best_score, best_nscore = sc->best_nscore;
  double best_solution = sc->best_solution;
  const uint64_t hash0 = sc->hash;
  const int early0 = sc->early, visits0 = sc->visit_count;
  const int gid = sc->graph;
  const EpRows<int32_t> rows(a, e);
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* ed = a.gs.edges + a.gs.edge_base[gid];
  const int q0 = rp[act], q1 = rp[act + 1];
  const int sa_old = rows.spins[act];  // pre-flip spin and field of the flipped vertex (one broadcast load each)
  const int ha = rows.field[act];
  int s[VPT], tsf[VPT], bs[VPT], h[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    if (v < N) { s[k] = rows.spins[v]; h[k] = rows.field[v]; tsf[k] = rows.tsf[v]; bs[k] = rows.best[v]; d_lds[v] = 0; }
    else { s[k] = 0; h[k] = 0; tsf[k] = 0; bs[k] = 0; }
  }
  const double delta = (double)sa_old * (double)ha;  // f64 product: keeps -0.0 like the reference
  const double delta_n = delta / qn;                 // get_normalized_score_mask(state)[action] (:394)
  const double score = score0 + delta;               // :399
  const double nscore = nscore0 + delta_n;           // :400 (accumulated)
  // step_outcome's `improved`, for the best-spins update inside the reduction loop only; after the call o.improved
  const bool improved_early = score > best_score;
  // incremental local field: h_j -= 2 w_aj s_a(old) over the CSR row of `act` (distinct columns: no collisions)
  __syncthreads();  // d zeroed; every load of the old state and scalars above has completed
  for (int q = q0 + tid; q < q1; q += WG_NT) {
    const uint32_t x = ed[q];
    const int c = edge_col(x);
    if (c < N) d_lds[c] = -2 * edge_w(x) * sa_old;
  }
  __syncthreads();
  // flip + time-since-flip counters (:397, :492-497), immediate changes (:414, :416), best tracking (:459-477)
  int cnt = 0, negs = 0, ham = 0;
  uint64_t words[VPT];  // words[k]: word 4 k + wv of the spin configuration
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    if (v < N) h[k] += d_lds[v];
    if (v == act) { s[k] = -s[k]; tsf[k] = 0; }
    else if (v < N) { tsf[k] = tsf[k] + 1; }
    const int g = s[k] * h[k];
    cnt += __popcll(__ballot(g > 0));
    words[k] = __ballot(s[k] > 0);
    negs += __popcll(__ballot(s[k] < 0));
    if (improved_early) bs[k] = s[k];
    ham += __popcll(__ballot(bs[k] != s[k]));
  }
  if (lane == 0) { r_cnt[wv] = cnt; r_neg[wv] = negs; r_ham[wv] = ham; }
  // HistoryBuffer.update (utils.py:444-464): is the flipped set (== spin configuration) new?  Every thread walks the
  // probe sequence on the same loads, so the loop and its barriers are block-uniform.
  const bool track = a.cfg.has_basin_reward || a.cfg.has_stag_punishment;
  bool isnew = true;
  const uint64_t hash = hash0 ^ zobrist(act);
  const int cap = L.cap;
  const int W = L.words;
  uint32_t* vidx = (uint32_t*)(a.state + L.off_vidx) + (size_t)e * cap;
  uint64_t* vh = (uint64_t*)(a.state + L.off_vhash) + (size_t)e * cap;
  uint64_t* vst = (uint64_t*)(a.state + L.off_vstates) + (size_t)e * (T + 1) * W;
  int slot = (int)(hash & (uint64_t)(cap - 1));
  if (track) {
    int it = 0;
    for (;;) {
      const uint32_t id = vidx[slot];
      const uint64_t hs = vh[slot];
      if (id == 0u) break;
      if (hs == hash) {  // full compare: each wave its own words, combined over the workgroup
        bool same = true;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
          const int wi = WG_NW * k + wv;
          if (wi < W) same = same && vst[(size_t)(id - 1) * W + wi] == words[k];
        }
        if (lane == 0) r_same[it & 1][wv] = same ? 1 : 0;
        __syncthreads();  // alternating buffers: a wave two compares ahead cannot exist (it needs this barrier twice)
        same = r_same[it & 1][0] && r_same[it & 1][1] && r_same[it & 1][2] && r_same[it & 1][3];
        ++it;
        if (same) { isnew = false; break; }
      }
      slot = (slot + 1) & (cap - 1);
    }
  }
  __syncthreads();  // the counts are in LDS; every wave has finished probing before the insertion below
  cnt = r_cnt[0] + r_cnt[1] + r_cnt[2] + r_cnt[3];
  negs = r_neg[0] + r_neg[1] + r_neg[2] + r_neg[3];
  ham = r_ham[0] + r_ham[1] + r_ham[2] + r_ham[3];
  if (track && isnew && lane == 0) {
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int wi = WG_NW * k + wv;
      if (wi < W) vst[(size_t)visits0 * W + wi] = words[k];
    }
  }
  // reward, best tracking, termination (:418-477, :541-556)
  const StepOutcome o = step_outcome(a.cfg, t, score, nscore, delta, delta_n, best_score, best_nscore, early0, isnew,
                                     cnt == 0, negs);
  if (o.improved) best_solution = cut_solution(score, lbabs);
  // write back
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = tid + WG_NT * k;
    if (v < N) {
      rows.spins[v] = (int8_t)s[k];
      rows.field[v] = h[k];
      rows.tsf[v] = (int16_t)tsf[k];
      if (o.improved) rows.best[v] = (int8_t)bs[k];
    }
  }
  if (tid == 0) {
    sc->score = score; sc->nscore = nscore;
    sc->best_score = o.best_score; sc->best_nscore = o.best_nscore; sc->best_solution = best_solution;
    sc->t = t; sc->hamming = ham; sc->done = o.done ? 1 : 0; sc->early = o.early;
    if (track) {
      sc->hash = hash;
      if (isnew) {
        vh[slot] = hash;
        vidx[slot] = (uint32_t)(visits0 + 1);
        sc->visit_count = visits0 + 1;
      }
    }
    a.rewards[e] = o.rew;
    a.dones[e] = o.done ? 1 : 0;
  }
  ObsCtx c;
  c.mlr = mlr;
  c.dist_best = distance_from_best(score, o.best_score, mlr);
  c.hamming = (double)ham;                                            // :526-527
  c.nqi = (double)cnt / (double)N;                                    // :513-514
  c.term = termination_immanency(a.cfg, t);
  c.ep_time = tab_ptr(a)[t];                                          // :506
  c.basis = a.cfg.spin_basis;
  if (FASTOBS) write_obs_default<VPT, WG_NT, int, false>(a, e, tid, s, h, tsf, c);
  else write_obs<VPT, WG_NT, int>(a, e, tid, s, h, tsf, c);
}

// Greedy solver action (src/agents/solver.py:100-131): first index of the largest g = s * (J s) over the allowed
// vertices, wave butterfly then the four waves through LDS; a negative best change (or no allowed vertex) finishes
// the episode.  Nothing is kept per vertex: the threads walk the state rows in global memory.
__global__ __launch_bounds__(WG_NT) void env_greedy_wg_kernel(EnvArgs a, int32_t* actions) {
  __shared__ int r_best[WG_NW], r_idx[WG_NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int e = blockIdx.x;
  if (e >= a.B) return;
  const int N = a.cfg.n_spins;
  EpScal* sc = scal_ptr(a) + e;
  if (uniform_i(sc->done)) {
    if (tid == 0) actions[e] = 0;
    return;
  }
  const EpRows<int32_t> rows(a, e);
  GreedyArgmax<int> m;
  for (int v = tid; v < N; v += WG_NT) {  // ascending v: a later equal value never replaces an earlier one
    const int s = rows.spins[v];
    if (a.cfg.reversible_spins || s < 0) m.offer(s * rows.field[v], v);
  }
  m.wave_reduce();
  if (lane == 0) { r_best[wv] = m.best; r_idx[wv] = m.idx; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < WG_NW; ++k) m.offer(r_best[k], r_idx[k]);
    m.finish(sc, actions, e);
  }
}

}  // namespace

// slots per thread: 16 up to 4096 vertices, 32 up to ECO_MAX_SPINS_WG
#define ECO_DISPATCH_WG(N, CALL)                          \
  do {                                                    \
    if ((N) <= 16 * WG_NT) { constexpr int V = 16; CALL; } \
    else { constexpr int V = 32; CALL; }                  \
  } while (0)

int env_reset_wg_launch(const EnvArgs& a, hipStream_t st) {
  const int N = a.cfg.n_spins;
  ECO_DISPATCH_WG(N, (env_reset_wg_kernel<V><<<a.B, WG_NT, (size_t)N, st>>>(a)));
  return check_launch("env_reset");
}

int env_step_wg_launch(const EnvArgs& a, bool fast, hipStream_t st) {
  const int N = a.cfg.n_spins;
  const size_t lds = (size_t)4 * N;  // <= 32 KB: within the default dynamic LDS limit
  if (fast) ECO_DISPATCH_WG(N, (env_step_wg_kernel<V, true><<<a.B, WG_NT, lds, st>>>(a)));
  else ECO_DISPATCH_WG(N, (env_step_wg_kernel<V, false><<<a.B, WG_NT, lds, st>>>(a)));
  return check_launch("env_step");
}

int env_greedy_wg_launch(const EnvArgs& a, int32_t* actions, hipStream_t st) {
  env_greedy_wg_kernel<<<a.B, WG_NT, 0, st>>>(a, actions);
  return check_launch("env_greedy");
}

}  // namespace eco
