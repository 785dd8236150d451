// Proportional prioritised replay on the device (Schaul et al. 2016, the variant that needs sums and no sort).
// One uint32 `mass` per LOGICAL ring position x (transition k of the buffer's life sits at x = k % capacity: the
// index replay_sample_kernel / replay_compact_read_kernel of eco_replay.hip call x), so one index space serves the fp32 feature
// ring and the compact ring.  mass = clamp(rint((min(|d|, d_max) + eps)^alpha * 2^16), 1, 2^31 - 1) for a stored
// transition, 0 for a never-written slot; every sum is a uint64 (capacity * 2^31 < 2^63), so the sampler does not
// depend on the reduction order and is restated exactly on the CPU (tests/prio_common.py).  No atomics at all.
//
// sample = four launches, the block sums recomputed on every call (4 * size bytes read):
//   prio_block_kernel   per 1024-entry block: sum (uint64) and maximum (16-B loads, wave shuffles, LDS over 4 waves)
//   prio_scan_kernel    one workgroup: inclusive prefix of the block sums, total S, global maximum
//   prio_draw_kernel    one wave per sample: stratum, rng3 draw, binary search of the block prefix, then the block's
//                       four 256-entry segments by wave prefix + ballot
//   prio_weight_kernel  one workgroup: importance weights in float64, normalised by the minibatch maximum
// push = prio_block_kernel + a write of the current maximum; update = one thread per sampled transition.
#include <cmath>

#include "eco_common.h"

namespace eco {

constexpr int PRIO_BLOCK = 1024;        // mass entries per block sum: 256 threads x one 16-byte load
constexpr uint32_t PRIO_ONE = 1u << 16;  // the mass of priority p = 1 (fixed point with 16 fraction bits)
constexpr uint32_t PRIO_MAX = 0x7FFFFFFFu;

struct PrioWs {
  uint64_t* hdr;   // [0] = S, [1] = maximum mass (256 B)
  uint64_t* bsum;  // [nb]
  uint64_t* bpre;  // [nb] inclusive prefix of bsum
  uint32_t* bmax;  // [nb]
};

static int prio_nb(long long n) { return (int)((n + PRIO_BLOCK - 1) / PRIO_BLOCK); }

static PrioWs prio_carve(void* base, int capacity, size_t* bytes = nullptr) {
  const size_t nb = (size_t)prio_nb(capacity);
  char* b = (char*)base;
  size_t o = 0;
  auto t = [&](size_t n) { void* p = b + o; o = align_up(o + n, 256); return p; };
  PrioWs w;
  w.hdr = (uint64_t*)t(256);
  w.bsum = (uint64_t*)t(nb * 8);
  w.bpre = (uint64_t*)t(nb * 8);
  w.bmax = (uint32_t*)t(nb * 4);
  if (bytes) *bytes = o;
  return w;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
// inclusive prefix over the 64 lanes
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// entries e .. e + 3 (e a multiple of 4) of mass[0 .. size), zero beyond size; never reads at or beyond size
__device__ __forceinline__ uint4 load4(const uint32_t* mass, long long e, int size) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (e + 4 <= size) {
    v = *reinterpret_cast<const uint4*>(mass + e);
  } else {
    if (e < size) v.x = mass[e];
    if (e + 1 < size) v.y = mass[e + 1];
    if (e + 2 < size) v.z = mass[e + 2];
  }
  return v;
}

// grid = ceil(size / 1024): block sums and maxima of mass[0 .. size)
__global__ __launch_bounds__(256) void prio_block_kernel(const uint32_t* mass, int size, uint64_t* bsum, uint32_t* bmax) {
  __shared__ uint64_t rs[4];
  __shared__ uint32_t rm[4];
  const uint4 v = load4(mass, (long long)blockIdx.x * PRIO_BLOCK + 4 * (int)threadIdx.x, size);
  const uint64_t s = wave_sum_u64((uint64_t)v.x + v.y + v.z + v.w);
  const uint32_t mx = wave_max_u32(max(max(v.x, v.y), max(v.z, v.w)));
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rm[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = rs[0] + rs[1] + rs[2] + rs[3];
    bmax[blockIdx.x] = max(max(rm[0], rm[1]), max(rm[2], rm[3]));
  }
}

// one workgroup of 1024 threads: thread t owns the `chunk` consecutive block sums from t * chunk
__global__ __launch_bounds__(1024) void prio_scan_kernel(const uint64_t* bsum, const uint32_t* bmax, int nb, uint64_t* bpre,
                                                         uint64_t* hdr) {
  __shared__ uint64_t ws[16];
  __shared__ uint32_t wm[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int chunk = (nb + 1023) / 1024;
  const int b0 = min(nb, t * chunk), b1 = min(nb, b0 + chunk);
  uint64_t s = 0;
  uint32_t mx = 0;
  for (int b = b0; b < b1; ++b) {
    s += bsum[b];
    mx = max(mx, bmax[b]);
  }
  const uint64_t incl = wave_scan_u64(s, lane);
  mx = wave_max_u32(mx);
  if (lane == 63) ws[w] = incl;
  if (lane == 0) wm[w] = mx;
  __syncthreads();
  uint64_t acc = incl - s;  // exclusive prefix of this thread's chunk
  for (int k = 0; k < w; ++k) acc += ws[k];
  for (int b = b0; b < b1; ++b) {
    acc += bsum[b];
    bpre[b] = acc;
  }
  if (t == 0) {
    uint64_t S = 0;
    uint32_t g = 0;
    for (int k = 0; k < 16; ++k) {
      S += ws[k];
      g = max(g, wm[k]);
    }
    hdr[0] = S;
    hdr[1] = g;
  }
}

// Stratified proportional draw, one wave per sample k: stratum [lo_k, lo_{k+1}) of [0, S) with lo_k = q k + (r k) / m
// (q = S / m, r = S % m), u = lo_k + rng3(seed, counter, k) % max(1, lo_{k+1} - lo_k), idx[k] = the smallest x whose
// inclusive prefix sum exceeds u.  With S = 0 (no stored mass: a caller error) every draw is size - 1.
__global__ __launch_bounds__(256) void prio_draw_kernel(const uint32_t* mass, int size, int m, uint64_t seed,
                                                        uint64_t counter, const uint64_t* hdr, const uint64_t* bpre,
                                                        int nb, int32_t* idx_out) {
  const int lane = threadIdx.x & 63;
  const int k = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (k >= m) return;  // whole waves
  const uint64_t S = hdr[0];
  const uint64_t q = S / (uint64_t)m, r = S % (uint64_t)m;
  const uint64_t lo = q * (uint64_t)k + r * (uint64_t)k / (uint64_t)m;
  const uint64_t hi = q * (uint64_t)(k + 1) + r * (uint64_t)(k + 1) / (uint64_t)m;
  const uint64_t width = hi > lo ? hi - lo : 1;
  const uint64_t u = lo + rng3(seed, counter, (uint64_t)k) % width;
  int b = 0, bh = nb - 1;  // smallest block whose inclusive prefix exceeds u (the last one if none does)
  while (b < bh) {
    const int mid = (b + bh) >> 1;
    if (bpre[mid] > u) bh = mid;
    else b = mid + 1;
  }
  uint64_t ur = u - (b ? bpre[b - 1] : 0);
  uint4 v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = load4(mass, (long long)b * PRIO_BLOCK + 256 * j + 4 * lane, size);
  int x = size - 1;
  bool found = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (found) continue;  // wave-uniform
    const uint64_t own = (uint64_t)v[j].x + v[j].y + v[j].z + v[j].w;
    const uint64_t incl = wave_scan_u64(own, lane);
    const uint64_t total = __shfl(incl, 63, 64);
    if (ur < total) {
      const unsigned long long hit = __ballot(incl > ur);
      const int L = __ffsll((long long)hit) - 1;
      // lane L resolves its four entries; every lane computes, lane L's answer is broadcast
      uint64_t acc = incl - own;
      const uint32_t e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      int t = 3;
#pragma unroll
      for (int i = 3; i >= 0; --i) {
        uint64_t p = acc;
#pragma unroll
        for (int ii = 0; ii <= i; ++ii) p += e[ii];
        if (p > ur) t = i;
      }
      x = b * PRIO_BLOCK + 256 * j + 4 * L + __shfl(t, L, 64);
      found = true;
    } else {
      ur -= total;
    }
  }
  if (lane == 0) idx_out[k] = min(x, size - 1);
}

// w_k = (size * mass[x_k] / S)^(-beta) in float64, divided by the largest w of the minibatch, stored as float32.
// pow is monotone in its base, so the largest w is the w of the smallest sampled mass: an exact integer minimum,
// then ONE pow per sample and a divide.
__global__ __launch_bounds__(1024) void prio_weight_kernel(const uint32_t* mass, int size, int m, const uint64_t* hdr,
                                                           double beta, const int32_t* idx, float* weights) {
  __shared__ uint32_t red[16];
  uint32_t mn = 0xFFFFFFFFu;
  for (int k = threadIdx.x; k < m; k += 1024) mn = min(mn, mass[idx[k]]);
  mn = wave_min_u32(mn);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
  __syncthreads();
  mn = red[0];
  for (int k = 1; k < 16; ++k) mn = min(mn, red[k]);
  const double S = (double)hdr[0], n = (double)size;
  const double wmax = pow(n * (double)mn / S, -beta);
  for (int k = threadIdx.x; k < m; k += 1024)
    weights[k] = (float)(pow(n * (double)mass[idx[k]] / S, -beta) / wmax);
}

__device__ __forceinline__ uint32_t prio_mass(float abs_td, double alpha, double eps, double td_max) {
  const double t = (double)abs_td;
  const double p = (t < td_max ? t : td_max) + eps;  // a NaN |td| counts as td_max
  const double v = rint(pow(p, alpha) * 65536.0);
  return v < 1.0 ? 1u : v > 2147483647.0 ? PRIO_MAX : (uint32_t)v;
}

// duplicates in idx carry the same abs_td (the same transition under the same weights): both writers store one value
__global__ void prio_update_kernel(uint32_t* mass, int capacity, int m, const int32_t* idx, const float* abs_td,
                                   double alpha, double eps, double td_max) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int x = idx[k];
  if ((unsigned)x >= (unsigned)capacity) return;  // never write outside the ring
  mass[x] = prio_mass(abs_td[k], alpha, eps, td_max);
}

// mass[(pos + i) % capacity] = the maximum over the nb block maxima (PRIO_ONE when the buffer was empty: nb = 0)
__global__ __launch_bounds__(256) void prio_push_kernel(uint32_t* mass, int capacity, int pos, int batch,
                                                        const uint32_t* bmax, int nb) {
  __shared__ uint32_t red[4];
  uint32_t mx = 0;
  for (int b = threadIdx.x; b < nb; b += 256) mx = max(mx, bmax[b]);
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = max(max(red[0], red[1]), max(red[2], red[3]));
  if (mx == 0) mx = PRIO_ONE;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < batch) mass[(int)(((long long)pos + i) % capacity)] = mx;
}

static int prio_common_check(const uint32_t* mass, int32_t capacity, const void* workspace, const char* who) {
  if (!mass || !workspace) return fail(ECO_ERR_ARG, std::string(who) + ": null mass / workspace");
  if (capacity < 1) return fail(ECO_ERR_ARG, std::string(who) + ": capacity must be positive");
  if (((uintptr_t)mass & 15) || ((uintptr_t)workspace & 15))
    return fail(ECO_ERR_ARG, std::string(who) + ": mass and workspace must be 16-byte aligned");
  return ECO_OK;
}

}  // namespace eco

using namespace eco;

extern "C" size_t eco_prio_workspace_bytes(int32_t capacity) {
  if (capacity < 1) return 0;
  size_t bytes = 0;
  prio_carve(nullptr, capacity, &bytes);
  return bytes;
}

extern "C" int eco_prio_push(uint32_t* mass, int32_t capacity, int32_t pos, int32_t batch, int32_t size_before,
                             void* workspace, eco_stream_t stream) {
  if (const int rc = prio_common_check(mass, capacity, workspace, "prio push")) return rc;
  if (batch < 1 || batch > capacity || pos < 0 || pos >= capacity || size_before < 0 || size_before > capacity)
    return fail(ECO_ERR_ARG, "prio push: need 1 <= batch <= capacity, 0 <= pos < capacity, 0 <= size_before <= capacity");
  hipStream_t st = (hipStream_t)stream;
  const PrioWs w = prio_carve(workspace, capacity);
  const int nb = prio_nb(size_before);
  if (nb) prio_block_kernel<<<nb, 256, 0, st>>>(mass, size_before, w.bsum, w.bmax);
  prio_push_kernel<<<(batch + 255) / 256, 256, 0, st>>>(mass, capacity, pos, batch, w.bmax, nb);
  return check_launch("prio_push");
}

extern "C" int eco_prio_sample(const uint32_t* mass, int32_t capacity, int32_t size, int32_t m, uint64_t seed,
                               uint64_t counter, double beta, int32_t* idx_out, float* weights_out, void* workspace,
                               eco_stream_t stream) {
  if (size < 1 || m < 1 || m > 65536 || size > capacity)
    return fail(ECO_ERR_ARG, "prio sample: need 1 <= size <= capacity and 1 <= m <= 65536");
  if (const int rc = prio_common_check(mass, capacity, workspace, "prio sample")) return rc;
  if (!idx_out || !weights_out) return fail(ECO_ERR_ARG, "prio sample: null output");
  if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(ECO_ERR_ARG, "prio sample: beta must be finite and >= 0");
  hipStream_t st = (hipStream_t)stream;
  const PrioWs w = prio_carve(workspace, capacity);
  const int nb = prio_nb(size);
  prio_block_kernel<<<nb, 256, 0, st>>>(mass, size, w.bsum, w.bmax);
  prio_scan_kernel<<<1, 1024, 0, st>>>(w.bsum, w.bmax, nb, w.bpre, w.hdr);
  prio_draw_kernel<<<(m + 3) / 4, 256, 0, st>>>(mass, size, m, seed, counter, w.hdr, w.bpre, nb, idx_out);
  prio_weight_kernel<<<1, 1024, 0, st>>>(mass, size, m, w.hdr, beta, idx_out, weights_out);
  return check_launch("prio_sample");
}

extern "C" int eco_prio_update(uint32_t* mass, int32_t capacity, int32_t m, const int32_t* idx, const float* abs_td,
                               double alpha, double eps, double td_max, eco_stream_t stream) {
  if (!mass || !idx || !abs_td) return fail(ECO_ERR_ARG, "prio update: null argument");
  if (capacity < 1 || m < 1) return fail(ECO_ERR_ARG, "prio update: capacity and m must be positive");
  if (!(alpha >= 0.0) || !std::isfinite(alpha) || !(eps >= 0.0) || !std::isfinite(eps) || !(td_max > 0.0) ||
      !std::isfinite(td_max))
    return fail(ECO_ERR_ARG, "prio update: need finite alpha >= 0, eps >= 0, td_max > 0");
  prio_update_kernel<<<(m + 255) / 256, 256, 0, (hipStream_t)stream>>>(mass, capacity, m, idx, abs_td, alpha, eps, td_max);
  return check_launch("prio_update");
}
