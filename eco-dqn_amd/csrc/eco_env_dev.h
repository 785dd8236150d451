// Device-side pieces shared by the batched env kernels: the wave-per-episode MaxCut kernels (eco_env.hip), the
// generic-scorer kernels (eco_env_problems.hip), the workgroup-per-episode MaxCut kernels (eco_env_wg.hip), the
// trajectory recorder (eco_env_record.hip) and the compact replay rings (eco_replay.hip).
//
// Everything that happens to an episode's scalars is stated here once: the initial spin, the reset record, the
// step's reward / early-stop counter / stopping rule, the best-solution rule, the episode-level observables, the
// observation-row writers and the greedy argmax.  What the kernel families keep to themselves is how per-vertex
// state is held and reduced (a wave's registers and ballots, or a workgroup's plus four LDS words; the field h, or
// a neighbour sum F plus masks).
#pragma once
#include "eco_common.h"
#include <type_traits>

namespace eco {

struct EnvArgs {
  eco_env_config cfg;
  eco_graph_set gs;
  EnvLayout L;
  uint8_t* state;
  int B;
  const int32_t* graph_ids;
  const int8_t* spins_in;
  const uint8_t* mask;
  uint64_t seed;
  const int32_t* actions;
  double* rewards;
  uint8_t* dones;
  float* obs_x;
  double* obs_f64;
  int32_t* err;  // device error word (first error wins)
};

__device__ __forceinline__ EpScal* scal_ptr(const EnvArgs& a) { return (EpScal*)(a.state + a.L.off_scal); }
__device__ __forceinline__ const double* tab_ptr(const EnvArgs& a) { return (const double*)(a.state + a.L.off_tab + 256); }

// The four per-vertex state rows of episode e; F: the field type (int32, or f64 for float-weighted sets).
template <class F>
struct EpRows {
  int8_t* spins;
  F* field;
  int16_t* tsf;
  int8_t* best;
  __device__ __forceinline__ EpRows(const EnvArgs& a, int e) {
    const size_t o = (size_t)e * a.cfg.n_spins;
    spins = (int8_t*)(a.state + a.L.off_spins) + o;
    field = (F*)(a.state + a.L.off_field) + o;
    tsf = (int16_t*)(a.state + a.L.off_tsf) + o;
    best = (int8_t*)(a.state + a.L.off_best) + o;
  }
};

// Initial spin of vertex v of episode e (spinsystem.py:283-299): the caller's spins (anything but +-1 is reported
// as ECO_ERR_BASIS and taken as -1), a uniform draw 2*randint(2)-1, or all -1 in an irreversible env (:295-297).
__device__ __forceinline__ int initial_spin(const EnvArgs& a, int e, int v) {
  if (a.spins_in) {
    int sv = a.spins_in[(size_t)e * a.cfg.n_spins + v];
    if (sv != 1 && sv != -1) { atomicCAS(a.err, 0, ECO_ERR_BASIS); sv = -1; }
    return sv;
  }
  if (a.cfg.reversible_spins) return (int)(rng3(a.seed, (uint64_t)e, (uint64_t)v) >> 63) * 2 - 1;
  return -1;
}

// The scalar record of a freshly reset episode: the initial state is the best one, nothing visited, step 0.
// MaxCut has no invalidity: inorm = 1, inv = 0.
__device__ __forceinline__ void store_reset_scalars(EpScal* sc, double score, double nscore, double solution,
                                                    double mlr, double qn, double lb, double inorm, int gid, int n1,
                                                    int inv) {
  sc->score = score; sc->nscore = nscore;
  sc->best_score = score; sc->best_nscore = nscore; sc->best_solution = solution;
  sc->mlr = mlr; sc->qn = qn; sc->lbabs = lb < 0.0 ? -lb : lb;
  sc->hash = 0ull; sc->t = 0; sc->hamming = 0; sc->graph = gid; sc->done = 0; sc->early = 0;
  sc->visit_count = 0;
  sc->inorm = inorm; sc->lb = lb;
  sc->n1 = n1; sc->inv = inv; sc->best_n1 = n1; sc->best_inv = inv;
}

// one node's fp32 feature row: ECO_OBS_X_STRIDE(nobs) floats (8, or 16 beyond 8 observables)
__device__ __forceinline__ void store_obs_row(float* obs_x, size_t row, int nobs, const float (&xf)[ECO_MAX_OBS]) {
  if (nobs <= 8) {
    float4* dst = (float4*)(obs_x + row * 8);
    dst[0] = make_float4(xf[0], xf[1], xf[2], xf[3]);
    dst[1] = make_float4(xf[4], xf[5], xf[6], xf[7]);
  } else {
    float4* dst = (float4*)(obs_x + row * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = make_float4(xf[4 * i], xf[4 * i + 1], xf[4 * i + 2], xf[4 * i + 3]);
  }
}

// One observable row value, float64, exactly as spinsystem.py:303-328 / :486-535.
struct ObsCtx {
  double mlr, dist_best, hamming, nqi, term, ep_time;
  int basis;
};
// g is passed as the field h; the reference's g = s * (J@s) is a float64 product, so
// s = -1 with h = +0.0 gives -0.0 (kept: observations are compared bitwise).
// F: the field type, int (integer weights) or double (float-weighted sets: the same f64 operations).
template <class F>
__device__ __forceinline__ double obs_value(int id, const ObsCtx& c, int s, F h, int tsfk, const double* tab) {
  switch (id) {
    case ECO_OBS_SPIN_STATE: return c.basis == ECO_BASIS_BINARY ? (double)(1 - s) / 2.0 : (double)s;
    case ECO_OBS_IMMEDIATE_QUALITY_CHANGE: return ((double)s * (double)h) / c.mlr;
    case ECO_OBS_TIME_SINCE_FLIP: return tab[tsfk];
    case ECO_OBS_EPISODE_TIME: return c.ep_time;
    case ECO_OBS_TERMINATION_IMMANENCY: return c.term;
    case ECO_OBS_NUMBER_OF_QUALITY_IMPROVEMENTS: return c.nqi;
    case ECO_OBS_DISTANCE_FROM_BEST_SOLUTION: return c.dist_best;
    case ECO_OBS_DISTANCE_FROM_BEST_STATE: return c.hamming;
    case ECO_OBS_VALIDITY_BIT: return 1.0;  // MaxCut: every spin vector is valid
    default: return 0.0;  // GLOBAL_VALIDITY_DIFFERENCE: (0 - 0) / 1 (the mask observables are rejected)
  }
}

// ---- generic scorers (eco_env_problems.hip; the table of F_i, quality and invalidity masks is at its top) ----
// shared with the compact replay ring of eco_replay.hip, which rebuilds observation rows with these statements
__device__ __forceinline__ bool target_maximises(int t) {
  return t == ECO_TARGET_MAX_IND_SET || t == ECO_TARGET_MAX_CLIQUE;
}

__device__ __forceinline__ int field_coef(int t, int w) {
  switch (t) {
    case ECO_TARGET_MIN_CUT: return -2 * w;
    case ECO_TARGET_MIN_COVER: return w;
    case ECO_TARGET_MIN_DOM_SET: return w > 0 ? -1 : 0;
    default: return -w;
  }
}

// per-vertex quality / invalidity masks (table above)
__device__ __forceinline__ void vertex_masks(int t, int s, int F, int n1, int S0, int S1, int& qm, int& im) {
  switch (t) {
    case ECO_TARGET_MIN_COVER: qm = s; im = s * F; break;
    case ECO_TARGET_MAX_IND_SET: qm = -s; im = -s * F; break;
    case ECO_TARGET_MAX_CLIQUE: qm = -s; im = s > 0 ? 2 * (F - n1 + 1) : 2 * (n1 - F); break;
    case ECO_TARGET_MIN_DOM_SET: {
      const int alone = F == 0;
      qm = s; im = s > 0 ? alone + S1 : -alone - S0;
      break;
    }
    default: qm = -s * F; im = 0; break;  // MIN_CUT
  }
}

// solution quality (score_solver.py:196-200 / :224-228) of a set of size n1: measure n1, lower bound 0,
// quality normaliser N
__device__ __forceinline__ int set_quality(int t, int n1, int N) { return target_maximises(t) ? n1 : N - n1; }

// MinDomSet neighbour codes: bit0 = (x=0, P=0), bit1 = (x=0, P=1)
__device__ __forceinline__ uint8_t mds_code(int s, int F) {
  return s < 0 ? (uint8_t)((F == 0) | ((F == 1) << 1)) : (uint8_t)0;
}

// ---- episode logic of a step, after the family's own reductions ----
// The solution a state is worth (what best_solution holds once the state is the best one, and the recorder's
// `solution`): CUT calculate_cut = score - |lb| and MIN_CUT max(0, qn) - quality = qn - score, exact for integer
// weights; a set problem's set size if the set is valid, else the worst size (score_solver.py:196-200 / :224-228).
__device__ __forceinline__ double cut_solution(double score, double lbabs) { return score - lbabs; }
__device__ __forceinline__ double set_solution(int t, int n1, bool valid, int N) {
  return valid ? (double)n1 : (target_maximises(t) ? 0.0 : (double)N);
}
__device__ __forceinline__ double solution_of(int t, double score, double lbabs, double qn, int n1, bool valid, int N) {
  if (t == ECO_TARGET_CUT) return cut_solution(score, lbabs);
  if (t == ECO_TARGET_MIN_CUT) return qn - score;
  return set_solution(t, n1, valid, N);
}

// Reward (spinsystem.py:418-457), best score (:459-477) and termination (:541-556) of the step that took the
// episode to time t with score change d (normalised: dn).  score / nscore are the new ones, best_* and early the
// episode's old ones; isnew: the spin configuration was not visited before; basin: no flip raises the score
// (MaxCut: no g > 0; scorers: no positive score-mask entry); negs: spins still -1.
struct StepOutcome {
  double rew, best_score, best_nscore;
  int early;
  bool improved, done;
};
__device__ __forceinline__ StepOutcome step_outcome(const eco_env_config& cfg, int t, double score, double nscore,
                                                    double d, double dn, double best_score, double best_nscore,
                                                    int early, bool isnew, bool basin, int negs) {
  StepOutcome o;
  o.rew = 0.0;
  o.early = early + 1;
  o.improved = score > best_score;
  if (o.improved) {
    o.early = 0;
    if (cfg.reward_signal == ECO_REWARD_BLS) o.rew = cfg.norm_rewards ? nscore - best_nscore : score - best_score;
  }
  if (cfg.reward_signal == ECO_REWARD_DENSE) o.rew = cfg.norm_rewards ? dn : d;
  if (cfg.has_stag_punishment && !isnew) o.rew -= cfg.stag_punishment;
  if (cfg.has_basin_reward && basin && isnew) o.rew += cfg.basin_reward;
  o.best_score = o.improved ? score : best_score;
  o.best_nscore = o.improved ? nscore : best_nscore;
  const int T = cfg.max_steps;
  o.done = (t == T);
  if (cfg.stopping == ECO_STOP_EARLY && o.early == 15) o.done = true;
  if (cfg.stopping == ECO_STOP_QUARTER && t == T / 4) o.done = true;
  if (!cfg.reversible_spins && negs == 0) o.done = true;
  return o;
}

// TERMINATION_IMMANENCY (spinsystem.py:509-511) and DISTANCE_FROM_BEST_SOLUTION (:516-519) of a stepped state; the
// set problems measure the distance in solution quality (integers).  A reset state's rows hold 0 for both.
__device__ __forceinline__ double termination_immanency(const eco_env_config& cfg, int t) {
  const double x = (double)(t - cfg.max_steps) / (double)cfg.horizon_length + 1.0;
  return x > 0.0 ? x : 0.0;
}
__device__ __forceinline__ double distance_from_best(double score, double best_score, double mlr) {
  const double dsc = score - best_score;
  return (dsc < 0.0 ? -dsc : dsc) / mlr;
}
__device__ __forceinline__ double set_distance_from_best(int t, int n1, int best_n1, int N, double mlr) {
  const int dq = set_quality(t, n1, N) - set_quality(t, best_n1, N);
  return (double)(dq < 0 ? -dq : dq) / mlr;
}

// Episode quantities an observation row needs beyond the per-vertex masks.
struct ProbObs {
  double mlr, inorm, dist_best, hamming, nqi, nvi, term, ep_time, gvd, valid;
  int basis;
};

__device__ __forceinline__ double prob_obs_value(int id, const ProbObs& c, int s, int qm, int im, int vm, int tsfk,
                                                 const double* tab, bool cut_like) {
  switch (id) {
    case ECO_OBS_SPIN_STATE: return c.basis == ECO_BASIS_BINARY ? (double)(1 - s) / 2.0 : (double)s;
    case ECO_OBS_IMMEDIATE_QUALITY_CHANGE:
      // MIN_CUT: -(s * (J s)) in f64 (a zero product keeps its sign through the negation)
      return (cut_like ? -((double)s * (double)(-qm * s)) : (double)qm) / c.mlr;
    case ECO_OBS_IMMEDIATE_VALIDITY_DIFFERENCE: return (double)im / c.inorm;
    case ECO_OBS_IMMEDIATE_VALIDITY_CHANGE: return vm ? 1.0 : 0.0;
    case ECO_OBS_TIME_SINCE_FLIP: return tab[tsfk];
    case ECO_OBS_EPISODE_TIME: return c.ep_time;
    case ECO_OBS_TERMINATION_IMMANENCY: return c.term;
    case ECO_OBS_NUMBER_OF_QUALITY_IMPROVEMENTS: return c.nqi;
    case ECO_OBS_NUMBER_OF_VALIDITY_IMPROVEMENTS: return c.nvi;
    case ECO_OBS_DISTANCE_FROM_BEST_SOLUTION: return c.dist_best;
    case ECO_OBS_DISTANCE_FROM_BEST_STATE: return c.hamming;
    case ECO_OBS_GLOBAL_VALIDITY_DIFFERENCE: return c.gvd;
    default: return c.valid;  // ECO_OBS_VALIDITY_BIT
  }
}

// ---- observation rows ----
// The rows of the vertices first, first + STRIDE, ... (VPT slots; STRIDE 64: a wave's lanes, 256: a workgroup's
// threads) of episode e: value(k, id) is slot k's float64 value of observable id, stored to obs_f64 when that is
// given and rounded once to the fp32 feature row.
template <int VPT, int STRIDE, class ValueFn>
__device__ __forceinline__ void write_obs_rows(const EnvArgs& a, int e, int first, ValueFn value) {
  const int N = a.cfg.n_spins;
  const int nobs = a.cfg.n_obs;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = first + STRIDE * k;
    if (v >= N) continue;
    float xf[ECO_MAX_OBS];
#pragma unroll
    for (int i = 0; i < ECO_MAX_OBS; ++i) {
      double val = 0.0;
      if (i < nobs) {
        val = value(k, a.cfg.obs_ids[i]);
        if (a.obs_f64) a.obs_f64[((size_t)e * nobs + i) * N + v] = val;
      }
      xf[i] = (float)val;
    }
    if (a.obs_x) store_obs_row(a.obs_x, (size_t)e * N + v, nobs, xf);
  }
}

// MaxCut rows (both kernel families)
template <int VPT, int STRIDE, class F>
__device__ __forceinline__ void write_obs(const EnvArgs& a, int e, int first, const int (&s)[VPT], const F (&h)[VPT],
                                          const int (&tsf)[VPT], const ObsCtx& c) {
  const double* tab = tab_ptr(a);
  write_obs_rows<VPT, STRIDE>(a, e, first, [&](int k, int id) { return obs_value(id, c, s[k], h[k], tsf[k], tab); });
}

// write_obs for DEFAULT_OBSERVABLES (spinsystem.py:486-535 with the ECO training observables, the hot path) and no
// float64 rows: the fp32 feature rows directly.  Per vertex only three values vary -- the spin (basis-mapped), the
// immediate quality change g / mlr and the time since flip -- and the other four are episode-uniform, converted
// once.  -0.0 is kept (s = -1, h = 0 gives -0.0 in the float product as in the reference's float64 product).
// F32_QUOTIENT, the wave kernels with integer weights: g / mlr is the correctly rounded f32 quotient of the two
// integers (exact in f32: |g|, |mlr| < 2^18), which equals the reference's float64 quotient rounded to f32: the
// exact quotient of integers below 2^18 is never within 2^-53 of an f32 rounding midpoint without being one (its
// distance from any K / 2^j is at least 2^-42 relative), so rounding through float64 cannot change the f32
// result.  tests/test_env_gpu.py checks these rows bitwise against the general path.
// Otherwise s * h / mlr is computed in float64, as the general path does, and rounded once to f32.  None of the
// argument carries over to float weights (F = double), and the workgroup kernels cannot meet its bound: 8191
// neighbours of weight 127 exceed |g|, mlr < 2^18.
template <int VPT, int STRIDE, class F, bool F32_QUOTIENT>
__device__ __forceinline__ void write_obs_default(const EnvArgs& a, int e, int first, const int (&s)[VPT],
                                                  const F (&h)[VPT], const int (&tsf)[VPT], const ObsCtx& c) {
  static_assert(!F32_QUOTIENT || std::is_same_v<F, int>, "the f32 quotient is exact for integer fields only");
  const int N = a.cfg.n_spins;
  const double* tab = tab_ptr(a);
  const float mlrf = (float)c.mlr;
  const float u3 = (float)c.dist_best, u4 = (float)c.hamming, u5 = (float)c.nqi, u6 = (float)c.term;
  const bool binary = c.basis == ECO_BASIS_BINARY;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = first + STRIDE * k;
    if (v >= N) continue;
    const float sf = (float)s[k];
    const float x0 = binary ? (float)((1 - s[k]) / 2) : sf;  // (1 - s) / 2 is exact: 0 or 1
    float x1;
    if constexpr (F32_QUOTIENT) x1 = __fdiv_rn(sf * (float)h[k], mlrf);
    else x1 = (float)(((double)s[k] * (double)h[k]) / c.mlr);
    const float x2 = (float)tab[tsf[k]];
    float4* dst = (float4*)(a.obs_x + ((size_t)e * N + v) * 8);
    dst[0] = make_float4(x0, x1, x2, u3);
    dst[1] = make_float4(u4, u5, u6, 0.f);
  }
}

// ---- greedy argmax (src/agents/solver.py:110-127) ----
// The allowed vertex with the largest score change, the first index on ties.  V: int, or double (float weights).
template <class V>
struct GreedyArgmax {
  static constexpr int NONE = 0x7fffffff;  // no vertex offered
  V best;
  int idx = NONE;
  __device__ __forceinline__ GreedyArgmax() {
    if constexpr (std::is_same_v<V, double>) best = -INFINITY; else best = INT_MIN;
  }
  // larger value, or equal value and smaller index
  __device__ __forceinline__ void offer(V g, int v) {
    if (g > best || (g == best && v < idx)) { best = g; idx = v; }
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) offer(__shfl_xor(best, o, 64), __shfl_xor(idx, o, 64));
  }
  // one thread of the episode: a negative best change, or no allowed vertex, finishes the episode (the solver stops,
  // :124-127); it is marked done so later steps leave it unchanged
  __device__ __forceinline__ void finish(EpScal* sc, int32_t* actions, int e) const {
    if (best < 0 || idx == NONE) {
      sc->done = 1;
      actions[e] = 0;
    } else {
      actions[e] = idx;
    }
  }
};

// LDS written by a wave and read back by the same wave only: a wave-scope fence suffices
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int readlane_t(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double readlane_t(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// Pre-flip spin and field of vertex `act` (lane act & 63, slot act >> 6) from the wave's registers.
template <int VPT, class F>
__device__ __forceinline__ void read_vertex(const int (&s)[VPT], const F (&f)[VPT], int act, int& sa, F& fa) {
  const int kk = act >> 6, la = act & 63;
  sa = 0;
  fa = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k)
    if (k == kk) { sa = __builtin_amdgcn_readlane(s[k], la); fa = readlane_t(f[k], la); }
}

// f_j += coef(J_ja) for every neighbour j of `act`: the lanes load the CSR row in parallel and scatter the
// deltas through the wave's LDS slice dl[N] (a row has distinct columns, so the stores never collide) --
// one round of loads instead of deg(a) dependent ones.
struct NoIssue {
  __device__ void operator()() const {}
};
// coef takes the packed word's integer weight, or (float-weighted sets) the edge index q whose f64 weight it loads
template <class Coef>
__device__ __forceinline__ auto row_coef(Coef& coef, uint32_t x, int q) {
  if constexpr (std::is_invocable_v<Coef&, int, int>) return coef(edge_w(x), q);
  else return coef(edge_w(x));
}
// after_loads: issued right after the row's edge loads (the step's next loads, e.g. the visited-set probe)
template <int VPT, class F, class Coef, class After = NoIssue>
__device__ __forceinline__ void row_update(F* dl, const uint32_t* ed, int q0, int q1, int N, int lane,
                                           F (&f)[VPT], Coef coef, After after_loads = After()) {
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) dl[v] = 0;
  }
  wave_lds_sync();
  if (q1 - q0 <= 64) {  // one load per lane (every ER-200 / BA-500 row): the caller's next loads go out behind it
    const uint32_t x = q0 + lane < q1 ? ed[q0 + lane] : 0u;
    after_loads();
    if (q0 + lane < q1) dl[edge_col(x)] = row_coef(coef, x, q0 + lane);
  } else {
    after_loads();
    for (int q = q0 + lane; q < q1; q += 64) {
      const uint32_t x = ed[q];
      dl[edge_col(x)] = row_coef(coef, x, q);
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) f[k] += dl[v];
  }
}

// HistoryBuffer.update (src/envs/utils.py:438-464): is the flipped-vertex set after flipping `act` new?
// The set is identified by the spin configuration (words = ballot(s > 0) per 64 vertices); a Zobrist
// hash of the set indexes an open-addressing table of the episode's visited configurations.  The
// initial (empty) set is never inserted, as in the reference.
template <int VPT>
__device__ __forceinline__ bool history_update(const EnvArgs& a, int e, int lane, EpScal* sc, int act,
                                               const uint64_t (&words)[VPT]) {
  const EnvLayout& L = a.L;
  const int T = a.cfg.max_steps;
  const uint64_t hash = sc->hash ^ zobrist(act);
  const int cap = L.cap;
  const int W = L.words;
  uint32_t* vidx = (uint32_t*)(a.state + L.off_vidx) + (size_t)e * cap;
  uint64_t* vh = (uint64_t*)(a.state + L.off_vhash) + (size_t)e * cap;
  uint64_t* vst = (uint64_t*)(a.state + L.off_vstates) + (size_t)e * (T + 1) * W;
  bool isnew = true;
  int slot = (int)(hash & (uint64_t)(cap - 1));
  for (;;) {
    const uint32_t id = vidx[slot];
    const uint64_t hs = vh[slot];  // issued together with the index load
    if (id == 0u) break;
    if (hs == hash) {
      bool same = true;
#pragma unroll
      for (int k = 0; k < VPT; ++k) same = same && (k >= W || vst[(size_t)(id - 1) * W + k] == words[k]);
      if (same) { isnew = false; break; }
    }
    slot = (slot + 1) & (cap - 1);
  }
  if (lane == 0) {
    sc->hash = hash;
    if (isnew) {
      const int n = sc->visit_count;
#pragma unroll
      for (int k = 0; k < VPT; ++k)
        if (k < W) vst[(size_t)n * W + k] = words[k];  // VPT = next power of two >= W
      vh[slot] = hash;
      vidx[slot] = (uint32_t)(n + 1);
      sc->visit_count = n + 1;
    }
  }
  return isnew;
}

// The same update with the first probe slot loaded ahead by the caller (history_probe, issued right after the
// step's CSR-row loads so its latency runs under the field update and the ballots; vmcnt is in order, so issuing
// it before loads the step needs sooner would delay those instead).
struct HistProbe {
  uint64_t hash;
  int slot;
  uint32_t id;
  uint64_t hs;
};
__device__ __forceinline__ void history_probe(const EnvArgs& a, int e, uint64_t prev_hash, int act, HistProbe& p) {
  const EnvLayout& L = a.L;
  const int cap = L.cap;
  p.hash = prev_hash ^ zobrist(act);
  p.slot = (int)(p.hash & (uint64_t)(cap - 1));
  p.id = ((const uint32_t*)(a.state + L.off_vidx) + (size_t)e * cap)[p.slot];
  p.hs = ((const uint64_t*)(a.state + L.off_vhash) + (size_t)e * cap)[p.slot];
}
template <int VPT>
__device__ __forceinline__ bool history_update_from(const EnvArgs& a, int e, int lane, EpScal* sc, const HistProbe& p,
                                                    const uint64_t (&words)[VPT]) {
  const EnvLayout& L = a.L;
  const int T = a.cfg.max_steps;
  const int cap = L.cap;
  const int W = L.words;
  uint32_t* vidx = (uint32_t*)(a.state + L.off_vidx) + (size_t)e * cap;
  uint64_t* vh = (uint64_t*)(a.state + L.off_vhash) + (size_t)e * cap;
  uint64_t* vst = (uint64_t*)(a.state + L.off_vstates) + (size_t)e * (T + 1) * W;
  bool isnew = true;
  int slot = p.slot;
  uint32_t id = p.id;
  uint64_t hs = p.hs;
  for (;;) {
    if (id == 0u) break;
    if (hs == p.hash) {
      bool same = true;
#pragma unroll
      for (int k = 0; k < VPT; ++k) same = same && (k >= W || vst[(size_t)(id - 1) * W + k] == words[k]);
      if (same) { isnew = false; break; }
    }
    slot = (slot + 1) & (cap - 1);
    id = vidx[slot];
    hs = vh[slot];
  }
  if (lane == 0) {
    sc->hash = p.hash;
    if (isnew) {
      const int n = sc->visit_count;
#pragma unroll
      for (int k = 0; k < VPT; ++k)
        if (k < W) vst[(size_t)n * W + k] = words[k];
      vh[slot] = p.hash;
      vidx[slot] = (uint32_t)(n + 1);
      sc->visit_count = n + 1;
    }
  }
  return isnew;
}

// vertices per lane for N spins (one 64-lane wave per episode)
// dynamic LDS of the step kernels: int32 row deltas [4 waves][N], then MinDomSet codes [4][N]
// (the float-weighted CUT step: f64 row deltas [4 waves][N], 64 KB at N = 2048)
inline size_t env_step_lds(int N) { return (size_t)4 * N * 4 + (size_t)4 * N; }

#define ECO_DISPATCH_VPT(N, CALL)                                   \
  do {                                                              \
    if ((N) <= 64) { constexpr int V = 1; CALL; }                   \
    else if ((N) <= 128) { constexpr int V = 2; CALL; }             \
    else if ((N) <= 256) { constexpr int V = 4; CALL; }             \
    else if ((N) <= 512) { constexpr int V = 8; CALL; }             \
    else if ((N) <= 1024) { constexpr int V = 16; CALL; }           \
    else { constexpr int V = 32; CALL; }                            \
  } while (0)

// generic-scorer launches (eco_env_problems.hip): 4 episodes per 256-thread block, lds = env_step_lds(N)
int env_reset_problem_launch(const EnvArgs& a, int blocks, size_t lds, hipStream_t st);
int env_step_problem_launch(const EnvArgs& a, int blocks, size_t lds, hipStream_t st);
int env_greedy_problem_launch(const EnvArgs& a, int32_t* actions, int blocks, size_t lds, hipStream_t st);

// workgroup-per-episode launches (eco_env_wg.hip), ECO_MAX_SPINS < N <= ECO_MAX_SPINS_WG: one 256-thread block per
// episode, OptimisationTarget.CUT with integer weights; fast: the DEFAULT_OBSERVABLES fp32-only observation write
int env_reset_wg_launch(const EnvArgs& a, hipStream_t st);
int env_step_wg_launch(const EnvArgs& a, bool fast, hipStream_t st);
int env_greedy_wg_launch(const EnvArgs& a, int32_t* actions, hipStream_t st);

}  // namespace eco
