// On-device graph generation for training resets (reference:
// RandomErdosRenyiGraphGenerator / RandomBarabasiAlbertGraphGenerator, src/envs/utils.py:165-236,
// which draw a fresh networkx graph on the host for every episode).
//
// Graphs are written into fixed edge slots of a graph set (edge_base[g] .. + cap), so a
// pool can be regenerated in place, then eco_graphs_prepare computes the normalisers.
// ER: edge {i,j} present iff hash(seed, g, i, j) < p; the hash is symmetric by construction,
//     so each row is generated independently (wave per row: count pass, scan, ballot fill;
//     columns come out sorted).
// BA: preferential attachment exactly as networkx.barabasi_albert_graph (initial star of m
//     targets, repeated-nodes list, m distinct draws per new vertex); the process is
//     sequential per graph, so one wave owns one graph with its lists in LDS.
// REGULAR: d-regular by the pairing algorithm of networkx.random_regular_graph (RandomRegularGraphGenerator,
//     utils.py:238-275); sequential per graph with restarts, one wave per graph as BA (regular_kernel).
// WS: the ring lattice of networkx.watts_strogatz_graph(n, k, 0) (RandomWattsStrogatzGraphGenerator,
//     utils.py:277-314, which always passes p = 0); wave per row, no RNG.  Rewiring (p > 0) is not implemented.
// Weights: +-1 fair per edge (EdgeType.DISCRETE, symmetric hash), 1 (UNIFORM), or float64 uniform in (-1, 1)
// (EdgeType.RANDOM): w = 2u - 1, u the top 53 bits of the same symmetric hash, written to gs.edge_weights with
// sign(w) in the packed word.
// Parity with numpy/networkx is distributional only (different RNG streams).  What these kernels themselves draw is
// an exact function of (seed, slot, pair or draw number): oracle/graphgen_oracle.py restates it, and
// tests/test_graphgen_exact_gpu.py holds every edge word, weight and prepared field to it bit for bit.
#include "eco_common.h"

namespace eco {

__device__ __forceinline__ uint32_t pair_key(int i, int j, int N) {
  const int a = min(i, j), b = max(i, j);
  return (uint32_t)a * (uint32_t)N + (uint32_t)b;
}
__device__ __forceinline__ bool er_edge(uint64_t seed, int g, int i, int j, int N, float p) {
  return i != j && u01(rng3(seed, (uint64_t)g, pair_key(i, j, N))) < p;
}
__device__ __forceinline__ int edge_sign(uint64_t seed, int g, int i, int j, int N, int discrete) {
  if (!discrete) return 1;
  return (rng3(seed ^ 0x5157A3C1ull, (uint64_t)g, pair_key(i, j, N)) >> 63) ? 1 : -1;
}
// ECO_WEIGHTS_RANDOM: 2u - 1 with u a 53-bit draw keyed by (seed, graph, unordered pair); exact in float64.  A draw of
// exactly 0 (probability 2^-53) becomes 2^-53: stored weights are nonzero.
__device__ __forceinline__ double edge_weight_random(uint64_t seed, int g, int i, int j, int N) {
  const uint64_t r = rng3(seed ^ 0x5157A3C1ull, (uint64_t)g, pair_key(i, j, N));
  const double w = 2.0 * ((double)(r >> 11) * 0x1p-53) - 1.0;
  return w == 0.0 ? 0x1p-53 : w;
}
// packed word and (kind RANDOM) float64 weight of edge {i, j} stored at slot q of the graph's row data
__device__ __forceinline__ void store_edge(uint32_t* ed, double* ew, long long q, int col, uint64_t seed, int g, int i,
                                           int j, int N, int kind) {
  int w;
  if (kind == ECO_WEIGHTS_RANDOM) {
    const double wd = edge_weight_random(seed, g, i, j, N);
    ew[q] = wd;
    w = wd > 0.0 ? 1 : -1;
  } else {
    w = edge_sign(seed, g, i, j, N, kind);
  }
  ed[q] = (uint32_t)col | ((uint32_t)(uint8_t)(int8_t)w << 24);
}

// pass 1: per-row degree (wave per row)
__global__ void er_count_kernel(int first, int count, int N, float p, uint64_t seed, int32_t* row_cnt) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)count * N) return;
  const int g = first + (int)(row / N);
  const int i = (int)(row % N);
  int c = 0;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    c += __popcll(__ballot(j < N && er_edge(seed, g, i, j, N, p)));
  }
  if (lane == 0) row_cnt[row] = c;
}

// pass 2: per-graph exclusive scan into row_ptr (wave per graph); overflow -> error word
__global__ void er_scan_kernel(int first, int count, int N, const int32_t* row_cnt, int32_t* row_ptr, long long cap,
                               int32_t* err) {
  const int lane = threadIdx.x & 63;
  const int gi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gi >= count) return;
  const int g = first + gi;
  int32_t* rp = row_ptr + (size_t)g * (N + 1);
  const int32_t* rc = row_cnt + (size_t)gi * N;
  int total = 0;
  for (int i = lane; i < N; i += 64) total += rc[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (total > cap) {  // overflow: leave an empty graph (valid = 0 after prepare) and report it
    for (int i = lane; i <= N; i += 64) rp[i] = 0;
    if (lane == 0) atomicCAS(err, 0, ECO_ERR_GRAPH);
    return;
  }
  int base = 0;
  if (lane == 0) rp[0] = 0;
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    int v = i < N ? rc[i] : 0;
    // inclusive wave scan
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (i < N) rp[i + 1] = base + v;
    base += __shfl(v, 63, 64);
  }
}

// pass 3: fill sorted columns (wave per row)
__global__ void er_fill_kernel(int first, int count, int N, float p, uint64_t seed, int kind,
                               const int32_t* row_ptr, const int64_t* edge_base, uint32_t* edges, double* weights) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)count * N) return;
  const int g = first + (int)(row / N);
  const int i = (int)(row % N);
  const int32_t* rp = row_ptr + (size_t)g * (N + 1);
  // er_scan_kernel ran before on the same stream and wrote rp[N] for every graph of the call: 0 for a graph without
  // an edge and for one that overflowed its slot (whose whole row_ptr row it zeroed).  Either way there is nothing to
  // fill; going on would put every row of an overflowing graph at offset 0 of the slot, deg_i entries each, past the
  // slot's end when deg_i > cap.
  if (rp[N] == 0) return;
  uint32_t* ed = edges + edge_base[g];
  double* ew = weights ? weights + edge_base[g] : nullptr;
  int pos = rp[i];
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    const bool on = j < N && er_edge(seed, g, i, j, N, p);
    const uint64_t bal = __ballot(on);
    if (on) {
      const int k = __popcll(bal & ((1ull << lane) - 1ull));
      store_edge(ed, ew, pos + k, j, seed, g, i, j, N, kind);
    }
    pos += __popcll(bal);
  }
}

// Barabasi-Albert (networkx.barabasi_albert_graph semantics), one wave per graph.
// LDS per wave: repeated list [2 m (N - m)] int32, edge list [(N - m) m] x2 int16, degree [N], fill cursor [N]
__global__ void ba_kernel(int first, int count, int N, int m, uint64_t seed, int kind, int32_t* row_ptr,
                          const int64_t* edge_base, uint32_t* edges, double* weights, long long cap, int32_t* err) {
  extern __shared__ int32_t sm[];
  const int lane = threadIdx.x;
  const int gi = blockIdx.x;
  if (gi >= count) return;
  const int g = first + gi;
  const int E = (N - m) * m;
  int32_t* rep = sm;                    // [2E]
  int32_t* es = rep + 2 * E;            // [E] source
  int32_t* et = es + E;                 // [E] target
  int32_t* deg = et + E;                // [N]
  int32_t* cur = deg + N;               // [N]
  for (int i = lane; i < N; i += 64) deg[i] = 0;
  if (lane == 0) {
    int nrep = 0, ne = 0;
    int targets[64];
    for (int k = 0; k < m; ++k) targets[k] = k;
    uint64_t ctr = 0;
    for (int src = m; src < N; ++src) {
      for (int k = 0; k < m; ++k) {
        es[ne] = src;
        et[ne] = targets[k];
        ++ne;
        rep[nrep++] = targets[k];
      }
      for (int k = 0; k < m; ++k) rep[nrep++] = src;
      // m distinct uniform draws from the repeated list
      int got = 0;
      while (got < m) {
        const int x = rep[(int)(rng3(seed, (uint64_t)g, ctr++) % (uint64_t)nrep)];
        bool dup = false;
        for (int k = 0; k < got; ++k) dup = dup || (targets[k] == x);
        if (!dup) targets[got++] = x;
      }
    }
  }
  __syncthreads();
  for (int e = lane; e < E; e += 64) {
    atomicAdd(&deg[es[e]], 1);
    atomicAdd(&deg[et[e]], 1);
  }
  __syncthreads();
  int32_t* rp = row_ptr + (size_t)g * (N + 1);
  __shared__ int overflow;
  if (lane == 0) {
    int s = 0;
    for (int i = 0; i < N; ++i) {
      cur[i] = s;
      s += deg[i];
    }
    overflow = s > cap;
    if (overflow) atomicCAS(err, 0, ECO_ERR_GRAPH);
  }
  __syncthreads();
  for (int i = lane; i <= N; i += 64)  // overflow: an empty graph (valid = 0 after prepare)
    rp[i] = overflow ? 0 : (i == 0 ? 0 : cur[i - 1] + deg[i - 1]);
  if (overflow) return;
  __syncthreads();
  uint32_t* ed = edges + edge_base[g];
  double* ew = weights ? weights + edge_base[g] : nullptr;
  if (lane == 0) {  // deterministic fill order
    for (int e = 0; e < E; ++e) {
      const int a = es[e], b = et[e];
      store_edge(ed, ew, cur[a]++, b, seed, g, a, b, N, kind);
      store_edge(ed, ew, cur[b]++, a, seed, g, a, b, N, kind);
    }
  }
  __syncthreads();
  // sort each row by column (insertion sort; rows are short except hubs)
  for (int i = lane; i < N; i += 64) {
    for (int q = rp[i] + 1; q < rp[i + 1]; ++q) {
      const uint32_t x = ed[q];
      const double xw = ew ? ew[q] : 0.0;
      int r = q - 1;
      while (r >= rp[i] && (ed[r] & 0xFFFFFFu) > (x & 0xFFFFFFu)) {
        ed[r + 1] = ed[r];
        if (ew) ew[r + 1] = ew[r];
        --r;
      }
      ed[r + 1] = x;
      if (ew) ew[r + 1] = xw;
    }
  }
}

// Random d-regular graph (networkx.random_regular_graph: the pairing algorithm of Steger and Wormald), one wave
// per graph.  LDS per wave: stub list [N d], adjacency lists [N][d], degree [N], potential count [N], one word; int32.
// An attempt starts from the stub list (every vertex d times) and runs rounds: shuffle the stubs (Fisher-Yates),
// pair consecutive stubs, accept a pair that is neither a loop nor an edge already (edges of this round
// included), count the stubs of a rejected pair as potential.  No potential stubs: done.  No two distinct
// potential vertices that are not joined yet: the attempt failed and restarts from scratch.  Otherwise the stub
// list is rebuilt from the potential counts (in vertex order; the shuffle makes the order irrelevant).
// Lane 0 shuffles and pairs, as the definition is sequential in both; the wave fills and rebuilds the lists,
// tests the potential vertices, sorts the rows and writes them out.
// Termination: a round that adds an edge can happen N d / 2 times in an attempt; a round that adds none (every
// pair of a short stub list rejected although a joinable pair remains, e.g. a a b b shuffled to (a a)(b b)) is a
// stall, and an attempt with more than kRegularMaxStalls of them counts as failed; so an attempt has at most
// N d / 2 + kRegularMaxStalls + 1 rounds, and there are at most ECO_REGULAR_MAX_RESTARTS + 1 attempts.  Then the
// graph is left empty (valid = 0 after prepare) and ECO_ERR_GRAPH goes into the error word.
constexpr int kRegularMaxStalls = 64;

// uniform integer in [0, range) from a 64-bit draw (multiply-high; bias below range * 2^-64)
__device__ __forceinline__ int draw_below(uint64_t r, int range) { return (int)__umul64hi(r, (uint64_t)range); }

__global__ void regular_kernel(int first, int count, int N, int d, uint64_t seed, int kind, int32_t* row_ptr,
                               const int64_t* edge_base, uint32_t* edges, double* weights, int32_t* err) {
  extern __shared__ int32_t sm[];
  const int lane = threadIdx.x;
  const int gi = blockIdx.x;
  if (gi >= count) return;
  const int g = first + gi;
  const int S = N * d;
  int32_t* stubs = sm;        // [S]
  int32_t* adj = stubs + S;   // [N][d]
  int32_t* deg = adj + S;     // [N]
  int32_t* pot = deg + N;     // [N]
  int32_t& sh_added = pot[N]; // edges added by the round, lane 0 to the wave
  uint64_t ctr = 0;           // draw counter (used by lane 0 only)
  bool done = false;
  for (int attempt = 0; attempt <= ECO_REGULAR_MAX_RESTARTS && !done; ++attempt) {
    for (int i = lane; i < N; i += 64) deg[i] = 0;
    for (int s = lane; s < S; s += 64) stubs[s] = s % N;
    int ns = S, stalls = 0;  // wave-uniform
    __syncthreads();
    while (true) {  // one round per iteration: it adds an edge, or stalls, or ends the attempt
      if (ns == 0) {
        done = true;
        break;
      }
      for (int i = lane; i < N; i += 64) pot[i] = 0;
      __syncthreads();
      if (lane == 0) {
        for (int i = ns - 1; i > 0; --i) {
          const int j = draw_below(rng3(seed, (uint64_t)g, ctr++), i + 1);
          const int32_t t = stubs[i];
          stubs[i] = stubs[j];
          stubs[j] = t;
        }
        int added = 0;
        for (int p = 0; p < ns; p += 2) {
          const int a = stubs[p], b = stubs[p + 1];
          bool reject = a == b;
          for (int q = 0; q < deg[a] && !reject; ++q) reject = adj[a * d + q] == b;
          if (reject) {
            ++pot[a];
            ++pot[b];
          } else {  // deg <= d: every edge at a vertex consumed one of its d stubs
            adj[a * d + deg[a]++] = b;
            adj[b * d + deg[b]++] = a;
            ++added;
          }
        }
        sh_added = added;
      }
      __syncthreads();
      // potential vertices P; u can still be joined iff fewer than P - 1 of its neighbours are potential
      int np = 0;
      for (int i0 = 0; i0 < N; i0 += 64) np += __popcll(__ballot(i0 + lane < N && pot[i0 + lane] > 0));
      if (np == 0) {
        done = true;
        break;
      }
      bool open = false;
      for (int u = lane; u < N; u += 64) {
        if (pot[u] == 0) continue;
        int joined = 0;
        for (int q = 0; q < deg[u]; ++q) joined += pot[adj[u * d + q]] > 0;
        open = open || joined < np - 1;
      }
      const bool suitable = __ballot(open) != 0;
      if (uniform_i(sh_added) == 0) ++stalls;
      if (!suitable || stalls > kRegularMaxStalls) break;  // failed attempt
      // stub list of the next round: vertex i repeated pot[i] times (wave scan over the vertices)
      int base = 0;
      for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const int c = i < N ? pot[i] : 0;
        int v = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int u = __shfl_up(v, o, 64);
          if (lane >= o) v += u;
        }
        for (int q = 0; q < c; ++q) stubs[base + v - c + q] = i;  // total = 2 x rejected pairs <= ns
        base += __shfl(v, 63, 64);
      }
      ns = base;
      __syncthreads();
    }
    __syncthreads();
  }
  int32_t* rp = row_ptr + (size_t)g * (N + 1);
  if (!done) {  // restarts exhausted: an empty graph (valid = 0 after prepare)
    for (int i = lane; i <= N; i += 64) rp[i] = 0;
    if (lane == 0) atomicCAS(err, 0, ECO_ERR_GRAPH);
    return;
  }
  for (int i = lane; i <= N; i += 64) rp[i] = i * d;
  uint32_t* ed = edges + edge_base[g];
  double* ew = weights ? weights + edge_base[g] : nullptr;
  for (int i = lane; i < N; i += 64) {  // every row has d entries: sort by column, then store
    int32_t* row = adj + i * d;
    for (int q = 1; q < d; ++q) {
      const int32_t x = row[q];
      int r = q - 1;
      while (r >= 0 && row[r] > x) {
        row[r + 1] = row[r];
        --r;
      }
      row[r + 1] = x;
    }
    for (int q = 0; q < d; ++q) store_edge(ed, ew, (long long)i * d + q, row[q], seed, g, i, row[q], N, kind);
  }
}

// Ring lattice (networkx.watts_strogatz_graph(N, k, 0)): i ~ j iff 1 <= min(|i - j|, N - |i - j|) <= h, h = k / 2.
// No RNG in the structure; wave per row, ballot fill as er_fill_kernel, every row has rdeg = min(2 h, N - 1) entries.
__global__ void ws_kernel(int first, int count, int N, int h, int rdeg, uint64_t seed, int kind, int32_t* row_ptr,
                          const int64_t* edge_base, uint32_t* edges, double* weights) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)count * N) return;
  const int g = first + (int)(row / N);
  const int i = (int)(row % N);
  int32_t* rp = row_ptr + (size_t)g * (N + 1);
  if (lane == 0) {
    if (i == 0) rp[0] = 0;
    rp[i + 1] = (i + 1) * rdeg;
  }
  uint32_t* ed = edges + edge_base[g];
  double* ew = weights ? weights + edge_base[g] : nullptr;
  int pos = i * rdeg;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    const int dist = j > i ? j - i : i - j;
    const bool on = j < N && j != i && min(dist, N - dist) <= h;
    const uint64_t bal = __ballot(on);
    if (on) {
      const int k = __popcll(bal & ((1ull << lane) - 1ull));
      store_edge(ed, ew, pos + k, j, seed, g, i, j, N, kind);
    }
    pos += __popcll(bal);
  }
}

}  // namespace eco

using namespace eco;

extern "C" int eco_graphs_generate(eco_graph_set* gs, int32_t first, int32_t count, int32_t kind, double param,
                                   int32_t weight_kind, uint64_t seed, int64_t edge_cap, void* workspace,
                                   eco_stream_t stream) {
  if (!gs || !gs->row_ptr || !gs->edges || !gs->edge_base) return fail(ECO_ERR_ARG, "incomplete graph set");
  if (weight_kind < ECO_WEIGHTS_UNIFORM || weight_kind > ECO_WEIGHTS_RANDOM)
    return fail(ECO_ERR_ARG, "unknown weight kind (0 = all 1, 1 = +-1, 2 = uniform in (-1, 1))");
  if ((weight_kind == ECO_WEIGHTS_RANDOM) != (gs->edge_weights != nullptr))
    return fail(ECO_ERR_ARG, weight_kind == ECO_WEIGHTS_RANDOM
                                 ? "weight kind 2 (uniform in (-1, 1)) needs a graph set with edge_weights"
                                 : "integer weight kinds cannot be generated into a float-weighted graph set");
  if (gs->edge_weights && gs->unit_weights)
    return fail(ECO_ERR_ARG, "graph set has float edge_weights and unit_weights set");
  double* ewt = const_cast<double*>(gs->edge_weights);
  if (first < 0 || count < 1 || first + count > gs->n_graphs) return fail(ECO_ERR_ARG, "graph range out of set");
  const int N = gs->n_spins;
  hipStream_t st = (hipStream_t)stream;
  int32_t* err = err_word();  // read by eco_check_errors
  if (!err) return fail(ECO_ERR_HIP, "cannot allocate error word");
  if (!workspace) return fail(ECO_ERR_ARG, "null workspace (eco_graphs_generate_workspace_bytes)");
  int32_t* rp = const_cast<int32_t*>(gs->row_ptr);
  uint32_t* ed = const_cast<uint32_t*>(gs->edges);
  if (kind == ECO_GRAPH_ER) {
    if (!(param >= 0.0 && param <= 1.0)) return fail(ECO_ERR_ARG, "ER p must be in [0, 1]");
    int32_t* cnt = (int32_t*)((char*)workspace + 256);
    const long long rows = (long long)count * N;
    const int rblocks = (int)((rows + 3) / 4);
    er_count_kernel<<<rblocks, 256, 0, st>>>(first, count, N, (float)param, seed, cnt);
    er_scan_kernel<<<(count + 3) / 4, 256, 0, st>>>(first, count, N, cnt, rp, edge_cap, err);
    er_fill_kernel<<<rblocks, 256, 0, st>>>(first, count, N, (float)param, seed, weight_kind, rp, gs->edge_base,
                                            ed, ewt);
  } else if (kind == ECO_GRAPH_BA) {
    const int m = (int)param;
    if (m < 1 || m >= N || m > 64) return fail(ECO_ERR_ARG, "BA m must be in [1, min(N-1, 64)]");
    const size_t E = (size_t)(N - m) * m;
    const size_t lds = (4 * E + 2 * (size_t)N) * sizeof(int32_t);
    if (lds > 160 * 1024) return fail(ECO_ERR_ARG, "BA graph too large for one workgroup's LDS");
    (void)hipFuncSetAttribute((const void*)ba_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    ba_kernel<<<count, 64, lds, st>>>(first, count, N, m, seed, weight_kind, rp, gs->edge_base, ed, ewt, edge_cap,
                                      err);
  } else if (kind == ECO_GRAPH_REGULAR) {
    if (!(param >= 0.0 && param < (double)N) || param != (double)(int)param)
      return fail(ECO_ERR_ARG, "regular-graph degree d must be an integer in [0, N)");
    const int d = (int)param;
    const long long S = (long long)N * d;
    if (S & 1) return fail(ECO_ERR_ARG, "no d-regular graph on N vertices: N d must be even");
    const size_t lds = (2 * (size_t)S + 2 * (size_t)N + 1) * sizeof(int32_t);
    if (lds > 160 * 1024) return fail(ECO_ERR_ARG, "regular graph too large for one workgroup's LDS");
    if (edge_cap < S) return fail(ECO_ERR_ARG, "edge slot smaller than the N d entries of a d-regular graph");
    (void)hipFuncSetAttribute((const void*)regular_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    regular_kernel<<<count, 64, lds, st>>>(first, count, N, d, seed, weight_kind, rp, gs->edge_base, ed, ewt, err);
  } else if (kind == ECO_GRAPH_WS) {
    if (!(param >= 0.0 && param <= (double)N) || param != (double)(int)param)
      return fail(ECO_ERR_ARG, "ring-lattice k must be an integer in [0, N]");
    const int h = (int)param / 2;
    const int rdeg = 2 * h < N - 1 ? 2 * h : N - 1;  // h = N / 2 (N even): the antipode is one neighbour
    if (edge_cap < (long long)N * rdeg)
      return fail(ECO_ERR_ARG, "edge slot smaller than the N min(2 (k / 2), N - 1) entries of the ring lattice");
    const long long rows = (long long)count * N;
    ws_kernel<<<(int)((rows + 3) / 4), 256, 0, st>>>(first, count, N, h, rdeg, seed, weight_kind, rp, gs->edge_base,
                                                     ed, ewt);
  } else {
    return fail(ECO_ERR_ARG, "unknown graph kind");
  }
  int rc = check_launch("graphs_generate");
  if (rc) return rc;
  return graphs_prepare_range(gs, first, count, st);
}

extern "C" size_t eco_graphs_generate_workspace_bytes(int32_t n_spins, int32_t count) {
  return 256 + (size_t)n_spins * count * sizeof(int32_t);
}
