// Trajectory histories of the batched SpinSystem: one record launch appends one row per episode
// (Network.reset / Network.step of src/agents/solver.py:198-216, :249-265).
//
// One 64-lane wave owns one episode, four episodes per workgroup, as in the env kernels; lane l walks
// vertices l, l + 64, ... in a loop, so one instantiation serves every N up to ECO_MAX_SPINS_WG (nothing is
// kept per vertex across the loop, unlike the step kernels' register-resident fields; the state layout is the same
// for the workgroup-per-episode env above ECO_MAX_SPINS, which is CUT with integer weights).  The kernel only
// reads the env state: the row's values are those the step kernels already keep --
//   solution    the value the step kernels store as best_solution when a state becomes the best one
//               (solution_of: CUT score - |lb|, MIN_CUT qn - score, set problems n1 if valid, else N / 0);
//   valid       inv == 0 (cut targets: always);
//   score_mask  every vertex's score change, from the resident neighbour sums with the arithmetic the greedy
//               kernels rank by (eco_env.hip env_greedy_kernel, eco_env_problems.hip
//               env_greedy_problem_kernel; the masks are vertex_masks, mds_code and set_quality of
//               eco_env_dev.h, as there) -- for ALL vertices: the reference records the unmasked
//               scorer.get_score_mask, also in irreversible envs.
// No atomics, no host read; every destination is optional (NULL = not recorded).
#include "eco_env_dev.h"

namespace eco {

struct RecordArgs {
  eco_env_history h;
  int row;
  const uint8_t* skip;
  const int32_t* actions;
  const double* rewards;
  const float* q;
};

template <class F>
__global__ __launch_bounds__(256) void env_record_kernel(EnvArgs a, RecordArgs r) {
  extern __shared__ uint8_t rc_lds[];  // MIN_DOM_SET: [4 waves][N] neighbour codes
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int e = uniform_i(blockIdx.x * 4 + wv);
  if (e >= a.B) return;
  if (r.skip && r.skip[e]) return;
  const int N = a.cfg.n_spins;
  const int B = a.B;
  const int tgt = a.cfg.optimisation_target;
  const EpScal* sc = scal_ptr(a) + e;
  const EpRows<F> rows(a, e);
  const size_t re = (size_t)r.row * B + e;  // [rows][B]
  const size_t rv = re * N;                 // [rows][B][N]
  const bool cut_like = tgt == ECO_TARGET_CUT || tgt == ECO_TARGET_MIN_CUT;
  const int n1 = sc->n1, inv = sc->inv;
  const bool valid = cut_like || inv == 0;
  if (lane == 0) {
    if (r.h.action) r.h.action[re] = (r.row > 0 && r.actions) ? (double)r.actions[e] : 0.0;
    if (r.h.reward) r.h.reward[re] = (r.row > 0 && r.rewards) ? r.rewards[e] : 0.0;
    if (r.h.solution) r.h.solution[re] = solution_of(tgt, sc->score, sc->lbabs, sc->qn, n1, valid, N);
    if (r.h.score) r.h.score[re] = sc->score;
    if (r.h.valid) r.h.valid[re] = valid ? 1 : 0;
    if (r.h.length) r.h.length[e] = r.row + 1;
  }
  if (r.h.qs) {
    const bool have = r.row > 0 && r.q;
    for (int v = lane; v < N; v += 64) r.h.qs[rv + v] = have ? r.q[(size_t)e * N + v] : 0.f;
  }
  if (r.h.spins)
    for (int v = lane; v < N; v += 64) r.h.spins[rv + v] = rows.spins[v];
  if (!r.h.score_mask) return;
  double* sm_out = r.h.score_mask + rv;
  if constexpr (std::is_same_v<F, double>) {  // float-weighted CUT: s * (J s) in float64
    for (int v = lane; v < N; v += 64) sm_out[v] = (double)rows.spins[v] * rows.field[v];
    return;
  } else {
    if (cut_like) {  // calculate_cut_changes: the f64 product s * (J s) (keeps -0.0), negated for MIN_CUT
      for (int v = lane; v < N; v += 64) {
        const double g = (double)rows.spins[v] * (double)rows.field[v];
        sm_out[v] = tgt == ECO_TARGET_CUT ? g : -g;
      }
      return;
    }
    const bool mds = tgt == ECO_TARGET_MIN_DOM_SET;
    uint8_t* code = rc_lds + (size_t)wv * N;
    const int32_t* rp = nullptr;
    const uint32_t* ed = nullptr;
    if (mds) {  // codes of the whole episode
      const int gid = sc->graph;
      rp = a.gs.row_ptr + (size_t)gid * (N + 1);
      ed = a.gs.edges + a.gs.edge_base[gid];
      for (int v = lane; v < N; v += 64) code[v] = mds_code(rows.spins[v], rows.field[v]);
      wave_lds_sync();
    }
    const int q = set_quality(tgt, n1, N);        // solution quality of the current set
    const int score = (inv == 0 ? q : 0) - inv;   // scorer.get_score (integer-valued)
    for (int v = lane; v < N; v += 64) {
      const int s = rows.spins[v], Fv = rows.field[v];
      int S0 = 0, S1 = 0;
      if (mds) {
        const int q1 = rp[v + 1];
        for (int k = rp[v]; k < q1; ++k) {
          const uint32_t x = ed[k];
          const int col = edge_col(x);
          const uint8_t c = (edge_w(x) > 0 && col < N) ? code[col] : (uint8_t)0;
          S0 += c & 1;
          S1 += c >> 1;
        }
      }
      int qm, im;
      vertex_masks(tgt, s, Fv, n1, S0, S1, qm, im);
      const int ui = inv + im;
      sm_out[v] = (double)((ui == 0 ? q + qm : 0) - ui - score);  // score_solver.py:310-324
    }
  }
}

}  // namespace eco

using namespace eco;

extern "C" int eco_env_record(const eco_env_config* cfg, const eco_graph_set* gs, const void* state, int32_t B,
                              int32_t row, const uint8_t* skip, const int32_t* actions, const double* rewards,
                              const float* q, const eco_env_history* hist, eco_stream_t stream) {
  if (!cfg) return fail(ECO_ERR_ARG, "null env config");
  if (!hist) return fail(ECO_ERR_ARG, "eco_env_record: null history");
  if (B < 1) return fail(ECO_ERR_ARG, "batch must be >= 1");
  if (!state) return fail(ECO_ERR_ARG, "null state");
  const int N = cfg->n_spins, tgt = cfg->optimisation_target;
  if (N < 1 || N > ECO_MAX_SPINS_WG)
    return fail(ECO_ERR_ARG, "n_spins out of range [1, " + std::to_string(ECO_MAX_SPINS_WG) + "]");
  // above ECO_MAX_SPINS the env is the integer MaxCut one (eco_env_wg.hip); the recorder's vertex loops take any N
  if (N > ECO_MAX_SPINS && (tgt != ECO_TARGET_CUT || cfg->float_weights || (gs && gs->edge_weights)))
    return fail(ECO_ERR_ARG, std::to_string(ECO_MAX_SPINS) + " < N <= " + std::to_string(ECO_MAX_SPINS_WG) +
                                 " runs OptimisationTarget.CUT with integer weights only");
  if (cfg->max_steps < 1 || cfg->max_steps > 32767) return fail(ECO_ERR_ARG, "max_steps out of range [1, 32767]");
  if (tgt < ECO_TARGET_CUT || tgt > ECO_TARGET_MIN_DOM_SET || tgt == ECO_TARGET_ENERGY)
    return fail(ECO_ERR_TARGET, "Invalid optimization target: " + std::to_string(tgt) + " and biased False");
  if (row < 0 || row >= hist->rows)
    return fail(ECO_ERR_ARG, "eco_env_record: row " + std::to_string(row) + " outside [0, " +
                                 std::to_string(hist->rows) + ")");
  const bool fw = cfg->float_weights != 0 || (gs && gs->edge_weights);
  if (fw && tgt != ECO_TARGET_CUT)
    return fail(ECO_ERR_ARG, "float edge weights run OptimisationTarget.CUT only (the generic-scorer kernels are "
                             "integer)");
  if (gs && (cfg->float_weights != 0) != (gs->edge_weights != nullptr))
    return fail(ECO_ERR_ARG, "env float_weights flag disagrees with the graph set");
  const bool mds_mask = tgt == ECO_TARGET_MIN_DOM_SET && hist->score_mask;
  if (mds_mask) {
    if (!gs || !gs->row_ptr || !gs->edge_base || !gs->edges)
      return fail(ECO_ERR_ARG, "MIN_DOM_SET score masks need the graph set");
    if (gs->n_spins != N) return fail(ECO_ERR_ARG, "graph set n_spins does not match the env");
  }
  EnvArgs a{};
  a.cfg = *cfg;
  if (gs) a.gs = *gs;
  a.L = env_layout(N, cfg->max_steps, B, cfg->float_weights);
  a.state = (uint8_t*)state;
  a.B = B;
  RecordArgs r;
  r.h = *hist;
  r.row = row;
  r.skip = skip;
  r.actions = actions;
  r.rewards = rewards;
  r.q = q;
  const int blocks = (B + 3) / 4;
  const size_t lds = mds_mask ? (size_t)4 * N : 0;
  hipStream_t st = (hipStream_t)stream;
  if (cfg->float_weights) env_record_kernel<double><<<blocks, 256, lds, st>>>(a, r);
  else env_record_kernel<int><<<blocks, 256, lds, st>>>(a, r);
  return check_launch("env_record");
}
