// Batched MaxCut SpinSystem on gfx950: graph preparation, reset, step, read-out.
//
// One 64-lane wave owns one episode; lane l owns vertices l, l+64, ... (VPT per
// lane), so every per-vertex reduction of the reference step (count of positive
// gains, all(g<=0), Hamming distance to best, the visited-state bitset) is a
// ballot/popcount and the episode scalars live in SGPRs.  The local field
// h = J.s is kept resident and updated by ONE CSR row per flip
// (h_j -= 2 w_aj s_a), so a step touches deg(a) edges instead of the reference's
// four dense J@s matvecs and two dense calculate_cut quadratic forms
// (spinsystem.py:393-416, 516-519).  All scores are exact integers in f64, and the
// f64 observation values are produced by the same IEEE operations as the
// reference, so rewards/observations match it bit for bit.
#include "eco_common.h"
#include "eco_mpnn.h"
#include "eco_env_dev.h"

namespace eco {

// ------------------------------------------------------------------ graphs ----
// score_solver.py:347-375 (normalisers) and mpnn.py:34-38 (degree norm).
// The graph's edge words are streamed ONCE, coalesced (thread t of the graph reads edges t, t + 64 WPG,
// ...), and each lane follows its edge's row through the row pointers staged in LDS (rows are contiguous, so a
// lane's row index only moves forward); per-vertex row sums and nonzero counts are LDS integer atomics (exact,
// order-free).  Walking one row per lane instead (each lane its own vertex's row) moved 3.58 GB for 8,192
// ER-200 graphs (18x their CSR): every load instruction touched 64 different lines.
constexpr int GP_WAVES = 4;
// WPG waves per graph: 1 for N <= 512 (four graphs per workgroup, wave-level sync only), all four for larger
// graphs (one graph per workgroup: a lone wave took 353 us over the 40 k edge words of a G22-like graph)
template <int WPG>
__global__ __launch_bounds__(64 * GP_WAVES) void graphs_prepare_kernel(eco_graph_set gs, int first, int count) {
  extern __shared__ int gp_lds[];  // per graph: rp [N + 1], rowsum [N], deg [N]
  constexpr int GPB = GP_WAVES / WPG;
  constexpr int NTG = 64 * WPG;  // threads per graph
  const int lane = threadIdx.x & 63;
  const int gl = (int)threadIdx.x / NTG;  // graph of the workgroup
  const int tg = (int)threadIdx.x % NTG;  // thread within the graph
  const int g = first + blockIdx.x * GPB + gl;
  const bool live = g < first + count;  // WPG == 1: wave-uniform; WPG > 1: one graph per workgroup
  if (WPG == 1 && !live) return;
  const int N = gs.n_spins;
  int* rpl = gp_lds + gl * (3 * N + 1);
  int* rsum = rpl + N + 1;
  int* dcnt = rsum + N;
  auto sync = [&]() {
    if (WPG == 1) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS operations done
      __builtin_amdgcn_wave_barrier();
    } else {
      __syncthreads();
    }
  };
  const int32_t* rp = gs.row_ptr + (size_t)g * (N + 1);
  const uint32_t* ed = gs.edges + gs.edge_base[live ? g : first];
  if (live) {
    for (int v = tg; v <= N; v += NTG) rpl[v] = rp[v];
    for (int v = tg; v < N; v += NTG) rsum[v] = dcnt[v] = 0;
  }
  sync();
  long long pos = 0, neg = 0;
  if (live) {
    const int e0 = rpl[0], e1 = rpl[N];
    int row = 0;
    for (int e = e0 + tg; e < e1; e += NTG) {
      while (rpl[row + 1] <= e) ++row;  // the row holding edge e (empty rows skipped)
      const int w = edge_w(ed[e]);
      if (w > 0) pos += w; else neg += w;
      if (w != 0) {
        atomicAdd(&rsum[row], w);
        atomicAdd(&dcnt[row], 1);
      }
    }
  }
  sync();
  long long sum = 0;
  int mdeg = 1;
  int best = INT_MIN;
  int has = 0;
  if (live) {
    for (int v = tg; v < N; v += NTG) {
      const int rs = rsum[v], d = dcnt[v];
      sum += rs;
      gs.deg[(size_t)g * N + v] = d;
      mdeg = max(mdeg, max(d, 1));
      // g(s=-1)_v = (-1) * (J.(-1))_v = row sum; mlr = max over NONZERO entries
      if (rs != 0) { has = 1; best = max(best, rs); }
    }
  }
  pos = wave_sum_ll(pos);
  neg = wave_sum_ll(neg);
  sum = wave_sum_ll(sum);
  mdeg = wave_max_i(mdeg);
  best = wave_max_i(best);
  has = wave_max_i(has);
  if (WPG > 1) {  // combine the graph's waves (fixed order: integer results, exact anyway)
    __shared__ long long rpos[GP_WAVES], rneg[GP_WAVES], rsm[GP_WAVES];
    __shared__ int rmd[GP_WAVES], rbest[GP_WAVES], rhas[GP_WAVES];
    const int wv = threadIdx.x >> 6;
    if (lane == 0) { rpos[wv] = pos; rneg[wv] = neg; rsm[wv] = sum; rmd[wv] = mdeg; rbest[wv] = best; rhas[wv] = has; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < WPG; ++k) {
      pos += rpos[k]; neg += rneg[k]; sum += rsm[k];
      mdeg = max(mdeg, rmd[k]); best = max(best, rbest[k]); has = max(has, rhas[k]);
    }
    if (!live) return;
  }
  if (lane == 0) {
    gs.max_deg[g] = mdeg;
    gs.valid[g] = has;
    double* m = gs.meta + (size_t)g * 4;
    m[0] = has ? (double)best : 1.0;
    const double q = (double)pos / 2.0;  // np.sum(J*(J>0))/2
    m[1] = q > 1.0 ? q : 1.0;            // max(1, .)
    const double lb = (double)neg / 2.0;
    m[2] = lb < 0.0 ? lb : 0.0;          // min(0, .)
    m[3] = (double)sum;
  }
}

// Float-weighted sets (gs.edge_weights, EdgeType.RANDOM): float64 sums must not depend on arrival order, so no
// atomics -- each row is summed by ONE lane in CSR order (lane t of the graph takes rows t, t + 64 WPG, ...), the
// lane partials are combined by the fixed xor butterfly and the graph's waves in wave order: bitwise reproducible
// run to run.  meta as score_solver.py:353-375: {max over nonzero row sums, max(1, sum_{w>0} w / 2),
// min(0, sum_{w<0} w / 2), sum w}.
template <int WPG>
__global__ __launch_bounds__(64 * GP_WAVES) void graphs_prepare_weighted_kernel(eco_graph_set gs, int first,
                                                                                int count) {
  constexpr int GPB = GP_WAVES / WPG;
  constexpr int NTG = 64 * WPG;
  const int lane = threadIdx.x & 63;
  const int gl = (int)threadIdx.x / NTG;
  const int tg = (int)threadIdx.x % NTG;
  const int g = first + blockIdx.x * GPB + gl;
  const bool live = g < first + count;
  if (WPG == 1 && !live) return;
  const int N = gs.n_spins;
  double pos = 0.0, neg = 0.0, sum = 0.0, best = -INFINITY;
  int mdeg = 1, has = 0;
  if (live) {
    const int32_t* rp = gs.row_ptr + (size_t)g * (N + 1);
    const double* ew = gs.edge_weights + gs.edge_base[g];
    for (int v = tg; v < N; v += NTG) {
      double rs = 0.0;
      int d = 0;
      const int q1 = rp[v + 1];
      for (int q = rp[v]; q < q1; ++q) {
        const double w = ew[q];
        rs += w;
        if (w > 0.0) pos += w; else neg += w;
        d += (w != 0.0);
      }
      sum += rs;
      gs.deg[(size_t)g * N + v] = d;
      mdeg = max(mdeg, max(d, 1));
      if (rs != 0.0) { has = 1; best = fmax(best, rs); }  // mlr = max over NONZERO entries
    }
  }
  pos = wave_sum_d(pos);
  neg = wave_sum_d(neg);
  sum = wave_sum_d(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, 64));
  mdeg = wave_max_i(mdeg);
  has = wave_max_i(has);
  if (WPG > 1) {  // combine the graph's waves in wave order
    __shared__ double rpos[GP_WAVES], rneg[GP_WAVES], rsm[GP_WAVES], rbest[GP_WAVES];
    __shared__ int rmd[GP_WAVES], rhas[GP_WAVES];
    const int wv = threadIdx.x >> 6;
    if (lane == 0) { rpos[wv] = pos; rneg[wv] = neg; rsm[wv] = sum; rbest[wv] = best; rmd[wv] = mdeg; rhas[wv] = has; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < WPG; ++k) {
      pos += rpos[k]; neg += rneg[k]; sum += rsm[k];
      best = fmax(best, rbest[k]); mdeg = max(mdeg, rmd[k]); has = max(has, rhas[k]);
    }
    if (!live) return;
  }
  if (lane == 0) {
    gs.max_deg[g] = mdeg;
    gs.valid[g] = has;
    double* m = gs.meta + (size_t)g * 4;
    m[0] = has ? best : 1.0;
    const double q = pos / 2.0;
    m[1] = q > 1.0 ? q : 1.0;
    const double lb = neg / 2.0;
    m[2] = lb < 0.0 ? lb : 0.0;
    m[3] = sum;
  }
}

// ------------------------------------------------------------- env kernels ----
// time table: tab[k] = running f64 sum of k additions of 1/T (spinsystem.py:493, :506)
__global__ void build_time_table_kernel(uint8_t* state, size_t off_tab, int T) {
  int* hdr = (int*)(state + off_tab);
  if (*hdr == T) return;
  double* tab = (double*)(state + off_tab + 256);
  double v = 0.0;
  const double inc = 1.0 / (double)T;
  tab[0] = 0.0;
  for (int k = 1; k <= T; ++k) { v += inc; tab[k] = v; }
  *hdr = T;
}

// SpinSystemBase.reset (spinsystem.py:183-259) + _reset_state (:283-330)
// F = int: integer weights (the packed byte); F = double: float-weighted sets (gs.edge_weights), every quantity the
// reference computes in float64 computed in float64 here.
template <int VPT, class F = int>
__global__ __launch_bounds__(256) void env_reset_kernel(EnvArgs a) {
  constexpr bool FW = std::is_same_v<F, double>;
  extern __shared__ int8_t s_lds[];  // [4 waves][N] spins staged for the J.s matvec
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int e = uniform_i(blockIdx.x * 4 + wv);
  if (e >= a.B) return;
  if (a.mask && !a.mask[e]) return;
  const int N = a.cfg.n_spins;
  const EnvLayout& L = a.L;
  int8_t* my_s = s_lds + wv * N;
  const int gid = uniform_i(a.graph_ids[e]);
  if (gid < 0 || gid >= a.gs.n_graphs || !a.gs.valid[gid]) {
    if (lane == 0) atomicCAS(a.err, 0, ECO_ERR_GRAPH);
    return;
  }
  const double* meta = a.gs.meta + (size_t)gid * 4;
  const double mlr = meta[0], qn = meta[1], lb = meta[2];
  const std::conditional_t<FW, double, long long> sumJ = (std::conditional_t<FW, double, long long>)meta[3];
  int s[VPT], tsf[VPT];
  F h[VPT], g[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    int sv = 0;
    if (v < N) {
      sv = initial_spin(a, e, v);
      my_s[v] = (int8_t)sv;
    }
    s[k] = sv;
    tsf[k] = 0;
  }
  wave_lds_sync();
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* ed = a.gs.edges + a.gs.edge_base[gid];
  std::conditional_t<FW, double, long long> sg = 0;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    F hv = 0;
    if (v < N) {
      if constexpr (FW) {
        const double* ew = a.gs.edge_weights + a.gs.edge_base[gid];
        for (int q = rp[v]; q < rp[v + 1]; ++q) hv += ew[q] * (double)my_s[edge_col(ed[q])];  // CSR order
      } else {
        for (int q = rp[v]; q < rp[v + 1]; ++q) {
          const uint32_t x = ed[q];
          hv += edge_w(x) * (int)my_s[edge_col(x)];
        }
      }
    }
    h[k] = hv;
    g[k] = s[k] * hv;  // calculate_cut_changes: s * (J @ s)
    sg += g[k];
    cnt += (g[k] > 0);
  }
  if constexpr (FW) sg = wave_sum_d(sg); else sg = wave_sum_ll(sg);
  cnt = wave_sum_i(cnt);
  // calculate_cut = 1/4 sum J (1 - s s^T) = (sum J - s.Js)/4, exact integer for integer weights
  double cut;
  if constexpr (FW) cut = (sumJ - sg) / 4.0; else cut = (double)((sumJ - sg) / 4);
  const double lbabs = lb < 0.0 ? -lb : lb;
  const double score = cut + lbabs;        // MaximizationProblem.get_score (score_solver.py:182-188)
  const double nscore = score / qn;        // get_normalized_score (:190-194)
  const EpRows<F> rows(a, e);
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) { rows.spins[v] = (int8_t)s[k]; rows.field[v] = h[k]; rows.tsf[v] = 0; rows.best[v] = (int8_t)s[k]; }
  }
  uint32_t* vidx = (uint32_t*)(a.state + L.off_vidx) + (size_t)e * L.cap;
  for (int i = lane; i < L.cap; i += 64) vidx[i] = 0u;
  int n1 = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) n1 += __popcll(__ballot(s[k] > 0));
  if (lane == 0) store_reset_scalars(scal_ptr(a) + e, score, nscore, cut, mlr, qn, lb, 1.0, gid, n1, 0);
  ObsCtx c;
  c.mlr = mlr; c.dist_best = 0.0; c.hamming = 0.0; c.nqi = (double)cnt / (double)N;
  c.term = 0.0; c.ep_time = 0.0; c.basis = a.cfg.spin_basis;
  write_obs<VPT, 64, F>(a, e, lane, s, h, tsf, c);
}

// Optional per-phase stamps of env_step_kernel (timing build only: make timing; tools/r04/env_timing.py):
// [episode][8] wall_clock64 values, first ECO_ENV_TS_EPS episodes.
#ifdef ECO_PHASE_TIMING
constexpr int ECO_ENV_TS_EPS = 16384;
__device__ unsigned long long eco_env_ts[ECO_ENV_TS_EPS * 8];
#define ECO_ENV_TS(k)                                                                                      \
  do {                                                                                                    \
    if (lane == 0 && e < ECO_ENV_TS_EPS) eco_env_ts[e * 8 + (k)] = wall_clock64();                        \
  } while (0)
#else
#define ECO_ENV_TS(k) \
  do {                \
  } while (0)
#endif

// SpinSystemBase.step (spinsystem.py:355-559), ExtraAction.NONE, memory_length None.
// FASTOBS: DEFAULT_OBSERVABLES, fp32 rows only (write_obs_default).
// F = double (float-weighted sets): h is an f64 register array updated along the CSR row of the flip as
// h_j -= 2 w_aj s_a, the LDS row-delta slice is f64 (8 N bytes per wave), and score / nscore / best_* / rewards /
// observation rows are the reference's float64 operations in its order (spinsystem.py:393-535).
template <int VPT, bool FASTOBS, class F = int>
__device__ __forceinline__ void env_step_body(const EnvArgs& a) {
  constexpr bool FW = std::is_same_v<F, double>;
  extern __shared__ int32_t d_lds[];  // [4 waves][N] row deltas (int32, or f64 for F = double)
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int e = uniform_i(blockIdx.x * 4 + wv);
  if (e >= a.B) return;
  ECO_ENV_TS(0);
  const int N = a.cfg.n_spins;
  EpScal* sc = scal_ptr(a) + e;
  const int act = uniform_i(a.actions[e]);  // loaded alongside the done flag
  if (sc->done) {  // auto-masked
    if (lane == 0) { a.rewards[e] = 0.0; a.dones[e] = 1; }
    return;
  }
  if (act < 0 || act >= N) {
    if (lane == 0) { atomicCAS(a.err, 0, ECO_ERR_ARG); a.rewards[e] = 0.0; a.dones[e] = 0; }
    return;
  }
  const int t = sc->t + 1;  // :362
  const EpRows<F> rows(a, e);
  const int gid = sc->graph;
  const int32_t* rp = a.gs.row_ptr + (size_t)gid * (N + 1);
  const uint32_t* ed = a.gs.edges + a.gs.edge_base[gid];
  const int q0 = rp[act], q1 = rp[act + 1];
  int s[VPT], tsf[VPT], bs[VPT];
  F h[VPT], g[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) { s[k] = rows.spins[v]; h[k] = rows.field[v]; tsf[k] = rows.tsf[v]; bs[k] = rows.best[v]; }
    else { s[k] = 0; h[k] = 0; tsf[k] = 0; bs[k] = 0; }
  }
  int sa_old;
  F ha;
  read_vertex<VPT>(s, h, act, sa_old, ha);
  ECO_ENV_TS(1);
  const double qn = sc->qn, mlr = sc->mlr;
  const double delta = (double)sa_old * (double)ha;  // f64 product: keeps -0.0 like the reference
  const double delta_n = delta / qn;     // get_normalized_score_mask(state)[action] (:394)
  const double score = sc->score + delta;           // :399
  const double nscore = sc->nscore + delta_n;       // :400 (accumulated)
  // incremental local field: h_j -= 2 w_aj s_a(old) over the CSR row of `act`
  const bool track = a.cfg.has_basin_reward || a.cfg.has_stag_punishment;
  HistProbe hp;
  if constexpr (FW) {
    const double* ew = a.gs.edge_weights + a.gs.edge_base[gid];
    const double m2s = -2.0 * (double)sa_old;
    // the same dynamic LDS seen as f64 [4 waves][N]: its own declaration carries the alignment of the 8-byte
    // accesses, whatever static LDS a later change may put in front of it
    extern __shared__ __attribute__((aligned(16))) double dd_lds[];
    row_update<VPT>(dd_lds + wv * N, ed, q0, q1, N, lane, h,
                    [&](int, int q) { return m2s * ew[q]; });
  } else {
    row_update<VPT>(d_lds + wv * N, ed, q0, q1, N, lane, h, [&](int w) { return -2 * w * sa_old; },
                    [&] { if (track) history_probe(a, e, sc->hash, act, hp); });
  }
  ECO_ENV_TS(2);
  // flip + time-since-flip counters (:397, :492-497)
  int cnt = 0;
  uint64_t words[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v == act) { s[k] = -s[k]; tsf[k] = 0; }
    else if (v < N) { tsf[k] = tsf[k] + 1; }
    g[k] = s[k] * h[k];  // immediate quality / score changes (:414, :416)
    cnt += __popcll(__ballot(g[k] > 0));
    words[k] = __ballot(s[k] > 0);
  }
  const int negs = [&] { int c = 0;
#pragma unroll
    for (int k = 0; k < VPT; ++k) c += __popcll(__ballot(s[k] < 0)); return c; }();
  // HistoryBuffer.update (utils.py:444-464): is the flipped set (== spin configuration) new?
  // (the f64 step probes the visited set here, without the early first-slot load of the integer kernels)
  bool isnew = true;
  if constexpr (FW) { if (track) isnew = history_update<VPT>(a, e, lane, sc, act, words); }
  else isnew = track ? history_update_from<VPT>(a, e, lane, sc, hp, words) : true;
  ECO_ENV_TS(3);
  // reward, best tracking, termination (:418-477, :541-556)
  const StepOutcome o = step_outcome(a.cfg, t, score, nscore, delta, delta_n, sc->best_score, sc->best_nscore,
                                     sc->early, isnew, cnt == 0, negs);
  double best_solution = sc->best_solution;
  if (o.improved) {
    best_solution = cut_solution(score, sc->lbabs);
#pragma unroll
    for (int k = 0; k < VPT; ++k) bs[k] = s[k];
  }
  int ham = 0;
#pragma unroll
  for (int k = 0; k < VPT; ++k) ham += __popcll(__ballot(bs[k] != s[k]));
  // write back
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) {
      rows.spins[v] = (int8_t)s[k];
      rows.field[v] = h[k];
      rows.tsf[v] = (int16_t)tsf[k];
      if (o.improved) rows.best[v] = (int8_t)bs[k];
    }
  }
  if (lane == 0) {
    sc->score = score; sc->nscore = nscore;
    sc->best_score = o.best_score; sc->best_nscore = o.best_nscore; sc->best_solution = best_solution;
    sc->t = t; sc->hamming = ham; sc->done = o.done ? 1 : 0; sc->early = o.early;
    a.rewards[e] = o.rew;
    a.dones[e] = o.done ? 1 : 0;
  }
  ECO_ENV_TS(4);
  ObsCtx c;
  c.mlr = mlr;
  c.dist_best = distance_from_best(score, o.best_score, mlr);
  c.hamming = (double)ham;                                            // :526-527
  c.nqi = (double)cnt / (double)N;                                    // :513-514
  c.term = termination_immanency(a.cfg, t);
  c.ep_time = tab_ptr(a)[t];                                          // :506
  c.basis = a.cfg.spin_basis;
  if (FASTOBS) write_obs_default<VPT, 64, F, !FW>(a, e, lane, s, h, tsf, c);
  else write_obs<VPT, 64, F>(a, e, lane, s, h, tsf, c);
  ECO_ENV_TS(5);
}
template <int VPT, bool FASTOBS, class F = int>
__global__ __launch_bounds__(256) void env_step_kernel(EnvArgs a) {
  env_step_body<VPT, FASTOBS, F>(a);
}
// The training / bench configuration up to N = 256 at 8 waves per SIMD (<= 64 VGPRs, no spills): all 8192
// ER-200 episodes of a step are resident at once (one wave each) instead of 6144 plus a second round of 2048
// (tools/r04/env_timing.py); above 4 vertices per lane that budget spills, so larger N runs env_step_kernel
template <int VPT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void env_step_fast_kernel(EnvArgs a) {
  env_step_body<VPT, true>(a);
}

// Greedy solver action (src/agents/solver.py:100-131): the vertex with the largest immediate
// cut change g = s * (J s) (first index on ties); an episode whose best change is negative is
// finished (the solver stops, :124-127) and is marked done so later steps leave it unchanged.
// Irreversible envs consider only still-flippable vertices (s == -1, :117-121).
template <int VPT, class F = int>
__global__ __launch_bounds__(256) void env_greedy_kernel(EnvArgs a, int32_t* actions) {
  const int lane = threadIdx.x & 63;
  const int e = uniform_i(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (e >= a.B) return;
  const int N = a.cfg.n_spins;
  EpScal* sc = scal_ptr(a) + e;
  if (sc->done) {
    if (lane == 0) actions[e] = 0;
    return;
  }
  const EpRows<F> rows(a, e);
  GreedyArgmax<F> m;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int v = lane + 64 * k;
    if (v < N) {
      const int s = rows.spins[v];
      if (a.cfg.reversible_spins || s < 0) m.offer(s * rows.field[v], v);
    }
  }
  m.wave_reduce();
  if (lane == 0) m.finish(sc, actions, e);
}

// read-out of episode scalars / spins
__global__ void env_read_kernel(EnvArgs a, double* scalars, int8_t* spins, int8_t* best) {
  const int e = blockIdx.x;
  if (e >= a.B) return;
  const int N = a.cfg.n_spins;
  const EpScal* sc = scal_ptr(a) + e;
  if (threadIdx.x == 0 && scalars) {
    double* o = scalars + (size_t)e * ECO_ENV_SCALARS;
    o[0] = sc->t; o[1] = sc->score; o[2] = sc->nscore; o[3] = sc->best_score;
    o[4] = sc->best_nscore; o[5] = sc->best_solution; o[6] = sc->hamming; o[7] = sc->done;
    o[8] = sc->mlr; o[9] = sc->qn; o[10] = sc->inorm > 0.0 ? sc->inorm : 1.0; o[11] = sc->lb;
    o[12] = sc->n1; o[13] = sc->inv; o[14] = sc->graph; o[15] = 0.0;
  }
  const int8_t* gsp = (const int8_t*)(a.state + a.L.off_spins) + (size_t)e * N;
  const int8_t* gb = (const int8_t*)(a.state + a.L.off_best) + (size_t)e * N;
  for (int v = threadIdx.x; v < N; v += blockDim.x) {
    if (spins) spins[(size_t)e * N + v] = gsp[v];
    if (best) best[(size_t)e * N + v] = gb[v];
  }
}

// ------------------------------------------------------------------ host ----
static int validate_cfg(const eco_env_config* c) {
  if (!c) return fail(ECO_ERR_ARG, "null env config");
  if (c->n_spins < 1 || c->n_spins > ECO_MAX_SPINS_WG)
    return fail(ECO_ERR_ARG, "n_spins out of range [1, " + std::to_string(ECO_MAX_SPINS_WG) + "]");
  if (c->max_steps < 1 || c->max_steps > 32767) return fail(ECO_ERR_ARG, "max_steps out of range [1, 32767]");
  if (c->n_obs < 1 || c->n_obs > 13) return fail(ECO_ERR_ARG, "n_obs out of range [1, 13]");
  if (c->obs_ids[0] != ECO_OBS_SPIN_STATE)
    return fail(ECO_ERR_OBSERVABLE, "First observable must be Observation.SPIN_STATE.");
  const int t = c->optimisation_target;
  if (t < ECO_TARGET_CUT || t > ECO_TARGET_MIN_DOM_SET || t == ECO_TARGET_ENERGY)
    return fail(ECO_ERR_TARGET, "Invalid optimization target: " + std::to_string(t) + " and biased False");
  for (int i = 0; i < c->n_obs; ++i) {
    const int id = c->obs_ids[i];
    if (id < 1 || id > 13) return fail(ECO_ERR_ARG, "unknown observable id");
    if ((t == ECO_TARGET_CUT || t == ECO_TARGET_MIN_CUT) &&
        (id == ECO_OBS_IMMEDIATE_VALIDITY_DIFFERENCE || id == ECO_OBS_IMMEDIATE_VALIDITY_CHANGE ||
         id == ECO_OBS_NUMBER_OF_VALIDITY_IMPROVEMENTS))
      return fail(ECO_ERR_OBSERVABLE, "validity-mask observables are undefined for cut targets (the "
                                      "reference's scorer returns a list: TypeError)");
  }
  if (c->spin_basis != ECO_BASIS_SIGNED && c->spin_basis != ECO_BASIS_BINARY)
    return fail(ECO_ERR_BASIS, "Unrecognised SpinBasis");
  if (c->horizon_length < 1) return fail(ECO_ERR_ARG, "horizon_length must be >= 1");
  if (c->float_weights != 0 && c->float_weights != 1) return fail(ECO_ERR_ARG, "float_weights must be 0 or 1");
  if (c->float_weights && t != ECO_TARGET_CUT)
    return fail(ECO_ERR_ARG, "float edge weights run OptimisationTarget.CUT only (the generic-scorer kernels are "
                             "integer)");
  // the workgroup-per-episode kernels (eco_env_wg.hip) are the integer MaxCut ones
  if (c->n_spins > ECO_MAX_SPINS && c->float_weights)
    return fail(ECO_ERR_ARG, "float edge weights run up to n_spins = " + std::to_string(ECO_MAX_SPINS) + " (" +
                                 std::to_string(ECO_MAX_SPINS) + " < N <= " + std::to_string(ECO_MAX_SPINS_WG) +
                                 " takes integer weights only)");
  if (c->n_spins > ECO_MAX_SPINS && t != ECO_TARGET_CUT)
    return fail(ECO_ERR_ARG, "the generic-scorer targets run up to n_spins = " + std::to_string(ECO_MAX_SPINS) + " (" +
                                 std::to_string(ECO_MAX_SPINS) + " < N <= " + std::to_string(ECO_MAX_SPINS_WG) +
                                 " runs OptimisationTarget.CUT only)");
  return ECO_OK;
}

static int validate_gs(const eco_graph_set* gs, int N) {
  if (!gs || !gs->row_ptr || !gs->edge_base || !gs->edges || !gs->deg || !gs->max_deg || !gs->meta || !gs->valid)
    return fail(ECO_ERR_ARG, "incomplete graph set");
  if (gs->n_spins != N) return fail(ECO_ERR_ARG, "graph set n_spins does not match the env");
  if (gs->n_graphs < 1) return fail(ECO_ERR_ARG, "empty graph set");
  if (gs->edge_weights && gs->unit_weights)
    return fail(ECO_ERR_ARG, "graph set has float edge_weights and unit_weights set");
  return ECO_OK;
}

// the env's field type must match the graph set's weight kind
static int check_weight_kind(const eco_env_config* c, const eco_graph_set* gs) {
  if ((c->float_weights != 0) != (gs->edge_weights != nullptr))
    return fail(ECO_ERR_ARG, c->float_weights ? "env configured with float_weights but the graph set has no edge_weights"
                                              : "float-weighted graph set needs an env configured with float_weights "
                                                "(OptimisationTarget.CUT only)");
  return ECO_OK;
}

int32_t* err_word() {
  static int32_t* w = nullptr;  // one device word per process (read back after each call)
  if (!w) {
    if (hipMalloc(&w, sizeof(int32_t)) != hipSuccess) return nullptr;
    (void)hipMemset(w, 0, sizeof(int32_t));
  }
  return w;
}

static int check_err_word(int32_t* w, hipStream_t st) {
  int32_t h = 0;
  if (hipMemcpyAsync(&h, w, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return fail(ECO_ERR_HIP, "error-word readback failed");
  if (h != 0) {
    (void)hipMemsetAsync(w, 0, sizeof(int32_t), st);
    (void)hipStreamSynchronize(st);
    switch (h) {
      case ECO_ERR_GRAPH: return fail(h, "graph has no nonzero local reward (empty graph) or bad graph id");
      case ECO_ERR_BASIS: return fail(h, "SpinSystem is configured for signed spins ([-1,1]).");
      case ECO_ERR_ARG: return fail(h, "action out of range [0, n_spins)");
      default: return fail(h, "device error");
    }
  }
  return ECO_OK;
}

static inline bool generic_target(const eco_env_config* c) { return c->optimisation_target != ECO_TARGET_CUT; }

}  // namespace eco

using namespace eco;

int eco::graphs_prepare_range(eco_graph_set* gs, int first, int count, hipStream_t st) {
  if (!gs || !gs->row_ptr || !gs->edge_base || !gs->edges || !gs->deg || !gs->max_deg || !gs->meta || !gs->valid)
    return fail(ECO_ERR_ARG, "incomplete graph set");
  if (gs->n_graphs < 1 || gs->n_spins < 1) return fail(ECO_ERR_ARG, "empty graph set");
  if (first < 0 || count < 1 || first + count > gs->n_graphs) return fail(ECO_ERR_ARG, "graph range out of set");
  if (gs->edge_weights) {
    if (gs->unit_weights) return fail(ECO_ERR_ARG, "graph set has float edge_weights and unit_weights set");
    if (gs->n_spins <= 512)
      graphs_prepare_weighted_kernel<1><<<(count + GP_WAVES - 1) / GP_WAVES, 64 * GP_WAVES, 0, st>>>(*gs, first, count);
    else
      graphs_prepare_weighted_kernel<GP_WAVES><<<count, 64 * GP_WAVES, 0, st>>>(*gs, first, count);
    return check_launch("graphs_prepare");
  }
  if (gs->n_spins <= 512) {
    const size_t lds = (size_t)GP_WAVES * (3 * gs->n_spins + 1) * sizeof(int);
    (void)hipFuncSetAttribute((const void*)graphs_prepare_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    graphs_prepare_kernel<1><<<(count + GP_WAVES - 1) / GP_WAVES, 64 * GP_WAVES, lds, st>>>(*gs, first, count);
  } else {
    // one workgroup per graph holds row pointers, row sums and nonzero counts in LDS: 12 B per vertex,
    // so the graph set may have at most 160 KB / 12 B = 13,653 vertices (every env kernel stops at
    // ECO_MAX_SPINS_WG = 8192 anyway: 96 KB); larger sets are rejected here rather than failing at launch
    const size_t lds = (size_t)(3 * gs->n_spins + 1) * sizeof(int);
    if (lds > (size_t)160 * 1024)
      return fail(ECO_ERR_ARG, "graphs_prepare: n_spins = " + std::to_string(gs->n_spins) +
                                   " needs " + std::to_string(lds) + " B of LDS (> 160 KB): at most 13653 vertices");
    if (hipFuncSetAttribute((const void*)graphs_prepare_kernel<GP_WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return fail(ECO_ERR_HIP, "graphs_prepare: cannot raise the dynamic LDS limit");
    graphs_prepare_kernel<GP_WAVES><<<count, 64 * GP_WAVES, lds, st>>>(*gs, first, count);
  }
  int rc = check_launch("graphs_prepare");
  if (rc) return rc;
  if (gs->adjbits && gs->unit_weights && adjbits_applies(gs->n_spins)) return adjbits_build(gs, first, count, st);
  return ECO_OK;
}

extern "C" int eco_graphs_prepare(eco_graph_set* gs, eco_stream_t stream) {
  if (!gs) return fail(ECO_ERR_ARG, "incomplete graph set");
  return graphs_prepare_range(gs, 0, gs->n_graphs, (hipStream_t)stream);
}

extern "C" size_t eco_graphs_adjbits_bytes(int32_t n_spins, int32_t n_graphs) {
  if (n_graphs < 1 || !adjbits_applies(n_spins)) return 0;
  return (size_t)n_graphs * n_spins * adjbits_words_per_node(n_spins) * 4;
}

extern "C" size_t eco_env_state_bytes(const eco_env_config* cfg, int32_t batch) {
  if (validate_cfg(cfg) != ECO_OK || batch < 1) return 0;
  return env_layout(cfg->n_spins, cfg->max_steps, batch, cfg->float_weights,
                    cfg->optimisation_target != ECO_TARGET_CUT).total;
}

static int make_args(EnvArgs& a, const eco_env_config* cfg, const eco_graph_set* gs, void* state, int32_t batch) {
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  if (gs) { rc = validate_gs(gs, cfg->n_spins); if (rc) return rc; }
  if (!state) return fail(ECO_ERR_ARG, "null state");
  if (batch < 1) return fail(ECO_ERR_ARG, "batch must be >= 1");
  a = EnvArgs{};
  a.cfg = *cfg;
  if (gs) a.gs = *gs;
  a.L = env_layout(cfg->n_spins, cfg->max_steps, batch, cfg->float_weights, cfg->optimisation_target != ECO_TARGET_CUT);
  a.state = (uint8_t*)state;
  a.B = batch;
  a.err = err_word();
  if (!a.err) return fail(ECO_ERR_HIP, "cannot allocate error word");
  return ECO_OK;
}

extern "C" int eco_env_reset(const eco_env_config* cfg, const eco_graph_set* gs, void* state, int32_t batch,
                             const int32_t* graph_ids, const int8_t* spins, const uint8_t* reset_mask, uint64_t seed,
                             float* obs_x, double* obs_f64, eco_stream_t stream) {
  EnvArgs a;
  int rc = make_args(a, cfg, gs, state, batch);
  if (rc) return rc;
  if (!gs) return fail(ECO_ERR_ARG, "null graph set");
  if (!graph_ids) return fail(ECO_ERR_ARG, "null graph_ids");
  rc = check_weight_kind(cfg, gs);
  if (rc) return rc;
  a.graph_ids = graph_ids; a.spins_in = spins; a.mask = reset_mask; a.seed = seed;
  a.obs_x = obs_x; a.obs_f64 = obs_f64;
  hipStream_t st = (hipStream_t)stream;
  build_time_table_kernel<<<1, 1, 0, st>>>(a.state, a.L.off_tab, cfg->max_steps);
  const int blocks = (batch + 3) / 4;
  const size_t lds = (size_t)4 * cfg->n_spins;
  if (generic_target(cfg)) return env_reset_problem_launch(a, blocks, lds, st);
  if (cfg->n_spins > ECO_MAX_SPINS) return env_reset_wg_launch(a, st);  // one workgroup per episode
  if (cfg->float_weights) ECO_DISPATCH_VPT(cfg->n_spins, (env_reset_kernel<V, double><<<blocks, 256, lds, st>>>(a)));
  else ECO_DISPATCH_VPT(cfg->n_spins, (env_reset_kernel<V><<<blocks, 256, lds, st>>>(a)));
  return check_launch("env_reset");
}

#ifdef ECO_PHASE_TIMING
extern "C" int eco_debug_env_ts(unsigned long long* host, int32_t n) {
  if (n > ECO_ENV_TS_EPS * 8) n = ECO_ENV_TS_EPS * 8;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(eco_env_ts), n * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" int eco_check_errors(eco_stream_t stream) {
  int32_t* w = err_word();
  if (!w) return fail(ECO_ERR_HIP, "cannot allocate error word");
  return check_err_word(w, (hipStream_t)stream);
}

extern "C" int eco_error_word_copy(int32_t* dst, eco_stream_t stream) {
  int32_t* w = err_word();
  if (!w) return fail(ECO_ERR_HIP, "cannot allocate error word");
  if (!dst) return fail(ECO_ERR_ARG, "null destination");
  if (hipMemcpyAsync(dst, w, sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream) != hipSuccess)
    return fail(ECO_ERR_HIP, "error-word copy failed");
  return ECO_OK;
}

extern "C" int eco_env_step(const eco_env_config* cfg, const eco_graph_set* gs, void* state, int32_t batch,
                            const int32_t* actions, double* rewards, uint8_t* dones, float* obs_x, double* obs_f64,
                            eco_stream_t stream) {
  EnvArgs a;
  int rc = make_args(a, cfg, gs, state, batch);
  if (rc) return rc;
  if (!gs) return fail(ECO_ERR_ARG, "null graph set");
  if (!actions || !rewards || !dones) return fail(ECO_ERR_ARG, "null actions/rewards/dones");
  rc = check_weight_kind(cfg, gs);
  if (rc) return rc;
  a.actions = actions; a.rewards = rewards; a.dones = dones; a.obs_x = obs_x; a.obs_f64 = obs_f64;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (batch + 3) / 4;
  if (generic_target(cfg)) return env_step_problem_launch(a, blocks, env_step_lds(cfg->n_spins), st);
  // the DEFAULT_OBSERVABLES fp32-only path (the training / bench configuration) or the general one
  const bool fast = !obs_f64 && obs_x && cfg->n_obs == 7 && cfg->obs_ids[0] == ECO_OBS_SPIN_STATE &&
                    cfg->obs_ids[1] == ECO_OBS_IMMEDIATE_QUALITY_CHANGE && cfg->obs_ids[2] == ECO_OBS_TIME_SINCE_FLIP &&
                    cfg->obs_ids[3] == ECO_OBS_DISTANCE_FROM_BEST_SOLUTION &&
                    cfg->obs_ids[4] == ECO_OBS_DISTANCE_FROM_BEST_STATE &&
                    cfg->obs_ids[5] == ECO_OBS_NUMBER_OF_QUALITY_IMPROVEMENTS &&
                    cfg->obs_ids[6] == ECO_OBS_TERMINATION_IMMANENCY;
  if (cfg->n_spins > ECO_MAX_SPINS) return env_step_wg_launch(a, fast, st);  // one workgroup per episode
  if (cfg->float_weights) {  // f64 field and row deltas: [4 waves][N] f64 of LDS (64 KB at N = 2048)
    const size_t ldsw = (size_t)32 * cfg->n_spins;  // <= 64 KB: within the default dynamic LDS limit
    if (fast) ECO_DISPATCH_VPT(cfg->n_spins, (env_step_kernel<V, true, double><<<blocks, 256, ldsw, st>>>(a)));
    else ECO_DISPATCH_VPT(cfg->n_spins, (env_step_kernel<V, false, double><<<blocks, 256, ldsw, st>>>(a)));
    return check_launch("env_step");
  }
  const size_t lds = (size_t)16 * cfg->n_spins;
  if (fast && cfg->n_spins <= 64) env_step_fast_kernel<1><<<blocks, 256, lds, st>>>(a);
  else if (fast && cfg->n_spins <= 128) env_step_fast_kernel<2><<<blocks, 256, lds, st>>>(a);
  else if (fast && cfg->n_spins <= 256) env_step_fast_kernel<4><<<blocks, 256, lds, st>>>(a);
  else if (fast) ECO_DISPATCH_VPT(cfg->n_spins, (env_step_kernel<V, true><<<blocks, 256, lds, st>>>(a)));
  else ECO_DISPATCH_VPT(cfg->n_spins, (env_step_kernel<V, false><<<blocks, 256, lds, st>>>(a)));
  return check_launch("env_step");
}

extern "C" int eco_env_greedy_actions(const eco_env_config* cfg, const eco_graph_set* gs, void* state,
                                      int32_t batch, int32_t* actions, eco_stream_t stream) {
  EnvArgs a;
  int rc = make_args(a, cfg, gs, state, batch);
  if (rc) return rc;
  if (!actions) return fail(ECO_ERR_ARG, "null actions");
  if (gs && (rc = check_weight_kind(cfg, gs))) return rc;
  if (cfg->optimisation_target == ECO_TARGET_MIN_DOM_SET && !gs)
    return fail(ECO_ERR_ARG, "MIN_DOM_SET greedy actions need the graph set");
  const int blocks = (batch + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  if (generic_target(cfg)) return env_greedy_problem_launch(a, actions, blocks, (size_t)4 * cfg->n_spins, st);
  if (cfg->n_spins > ECO_MAX_SPINS) return env_greedy_wg_launch(a, actions, st);  // one workgroup per episode
  if (cfg->float_weights)
    ECO_DISPATCH_VPT(cfg->n_spins, (env_greedy_kernel<V, double><<<blocks, 256, 0, st>>>(a, actions)));
  else
    ECO_DISPATCH_VPT(cfg->n_spins, (env_greedy_kernel<V><<<blocks, 256, 0, st>>>(a, actions)));
  return check_launch("env_greedy");
}

extern "C" int eco_env_read(const eco_env_config* cfg, const void* state, int32_t batch, double* scalars,
                            int8_t* spins, int8_t* best_spins, eco_stream_t stream) {
  EnvArgs a;
  int rc = make_args(a, cfg, nullptr, (void*)state, batch);
  if (rc) return rc;
  env_read_kernel<<<batch, 256, 0, (hipStream_t)stream>>>(a, scalars, spins, best_spins);
  return check_launch("env_read");
}
