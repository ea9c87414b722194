// sigma_cluster.hip -- the Wolff single-cluster update of the O(3) nonlinear sigma model (gfx950, wave64), on the unrotated
// lattice (mlmcpi_sigma_cluster_*) and on the levels of its CoarsenRotate hierarchy (mlmcpi_sigma_level_cluster_*; an unrotated
// level IS the lattice and takes its entry point).  One kernel per geometry, on the helpers of sigma_cluster_device.hpp: the
// two differ in the neighbour of a task and the name of its link.  One kernel instantiated on the geometry was built and
// withdrawn: the rotated wave-team instance with its bitmap in LDS went from 127 to 129 VGPRs, four waves per SIMD to three
// (EXPERIMENTS.md).  The plan, the attribute guard, the workspace and the launch exist once.
//
// NOT the reference's ClusterSampler for this action: ClusterSampler::single_cluster_update (sampler/clustersampler.cc:52-89)
// walks the eight entries of Lattice2D::neighbour_vertices (lattice2d.cc:135-155), the action couples four of them
// (nonlinearsigmaaction.hh:416-419); bonds across diagonals that carry no energy sample another model.  This is
// the same walk over the four links per vertex the action has, with the action's own new_reflection / S_ell / flip
// (nonlinearsigmaaction.cc:166-208).
//
// The update, restated (tests/sigma_cluster_model.py, tests/sigma_level_cluster_model.py).  A geometry has N
// vertices and 2 N links, every vertex four of them (where an extent is too small for four distinct neighbours, several links
// join one pair: distinct links with a uniform each, as the action counts each of those bonds).  With r the reflection normal
// and a_l = r . sigma_l of the field BEFORE the update, link (x, y) is bonded iff (a_x a_y) > 0 and its uniform
// < 1 - exp(min(0, -2 beta (a_x a_y)))  (the walk evaluates S_ell with one end already flipped: r . sigma' = -r . sigma).  The
// cluster is the connected component of the seed vertex in the graph of bonded links; every vertex of it is reflected once,
// sigma' = sigma - 2 a r, and stored in the canonical form (sigma2d.hip).  Every decision is a function of (link, chain,
// update counter, field before the update): the result does not depend on the order of the traversal.
//
// RNG contract, step = global update counter:
//   P_SIGMA_REFLECT  site 0, sub 0: (u, v) -> r_z = 1 - 2 u, azimuth 2 pi v - pi;  sub 1: u -> seed vertex min(floor(u N), N - 1)
//   P_SIGMA_BOND     unrotated: site l, sub 0: u decides link (l, 0), v decides link (l, 1)
//                    rotated:   site e (the E end), sub d >> 1: u decides link (e, d) for d even, v for d odd
#include "internal.hpp"

#include "sigma_cluster_device.hpp"  // the embedding and the geometries; fp contraction is off from here on

namespace mlmcpi {

constexpr uint32_t kScWaveChains = kClusterThreads / kWave;  // team = wave: chains per workgroup of 256 threads
constexpr uint32_t kScWaveLdsWords = 2048;     // team = wave: bitmap in LDS up to 8 KiB per chain (65 536 vertices)
constexpr uint32_t kScBlockLdsWords = 32768;   // team = workgroup: bitmap in LDS up to 128 KiB (2^20 vertices)

// n_updates updates of every chain, in place.  A chain belongs to a team of lanes: one wave (BLOCK = false, kScWaveChains
// chains per workgroup) or the whole workgroup (BLOCK = true).  Growth by frontier expansion: the vertices of the cluster
// are queued in the order they join, (vertex, a) pairs in the workspace; a level is the range [head, tail) of the queue.  A
// lane takes one (frontier vertex, direction) task: if the neighbour is not a member yet and the link is bonded, it claims
// the neighbour with an atomic OR on the membership bitmap, and the lane that set the bit appends it (one atomic add on the
// team's tail counter per wave and round).  Reflections are applied from the queue once growth has ended, so every bond test
// reads the field before the update; the same pass clears the bitmap words of the members.  Work per update is
// proportional to the cluster and its boundary; the bitmap is zeroed once per launch.
// The frontier loop ends after at most N levels (a vertex joins once, a level without a new member is the last one); `level <
// N` states that cap explicitly.  Queue positions are < N for the same reason; the store is guarded all the same.
template <bool BLOCK, bool LDS_MAP>
__global__ void __launch_bounds__(BLOCK ? kClusterBlockThreads : kClusterThreads)
    sigma_cluster_kernel(double2 *phi_all, uint32_t Mt, uint32_t Mx, double beta2, uint32_t B, uint32_t n_updates, RngKey key0,
                         uint32_t *queue_vertex, double *queue_a, uint32_t *map_all, uint32_t words, uint32_t *cluster_sites) {
  extern __shared__ uint32_t lds_map[];
  __shared__ uint32_t s_tail[kScWaveChains];
  const uint32_t T = BLOCK ? blockDim.x : (uint32_t)kWave;
  const uint32_t lane = BLOCK ? threadIdx.x : threadIdx.x & (kWave - 1);
  const uint32_t wave_lane = threadIdx.x & (kWave - 1);
  const uint32_t slot = BLOCK ? 0 : threadIdx.x >> 6;
  const uint32_t b = BLOCK ? blockIdx.x : blockIdx.x * kScWaveChains + slot;
  if (b >= B) return;                                    // team uniform (BLOCK: the grid has B workgroups)
  const uint32_t N = Mt * Mx;
  double2 *phi = phi_all + (size_t)b * N;
  uint32_t *qv = queue_vertex + (size_t)b * N;
  double *qa = queue_a + (size_t)b * N;
  uint32_t *map = LDS_MAP ? lds_map + slot * words : map_all + (size_t)b * words;
  for (uint32_t w = lane; w < words; w += T) map[w] = 0;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t total = 0;
  team_sync<BLOCK>();

  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    double u, v, us, unused;
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 0, u, v);
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 1, us, unused);
    const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
    double sa, ca;
    sincos(kTwoPi * v - kPi, &sa, &ca);
    const V3 r{rho * ca, rho * sa, rz};
    uint32_t seed = (uint32_t)(us * (double)N);
    seed = seed < N ? seed : N - 1;
    if (lane == 0) {
      qv[0] = seed;
      qa[0] = dot3(r, sigma_of(phi[seed]));
      map[seed >> 5] = 1u << (seed & 31u);
      s_tail[slot] = 1;
    }
    team_sync<BLOCK>();

    uint32_t head = 0, tail = 1;
    for (uint32_t level = 0; level < N && head < tail; ++level) {
      for (uint32_t base = head; base < tail; base += T / 4) {  // team uniform trip count: the ballot below sees whole waves
        const uint32_t q = base + (lane >> 2), d = lane & 3u;
        bool add = false;
        uint32_t y = 0;
        double ay = 0.0;
        if (q < tail) {
          const uint32_t x = qv[q];
          const double ax = qa[q];
          const uint32_t i = x % Mt, j = x / Mt;
          if (d == 0) y = i + 1 == Mt ? x - i : x + 1;
          else if (d == 1) y = i == 0 ? x + (Mt - 1) : x - 1;
          else if (d == 2) y = j + 1 == Mx ? i : x + Mt;
          else y = j == 0 ? x + (Mx - 1) * Mt : x - Mt;
          const uint32_t bit = 1u << (y & 31u);
          // a relaxed atomic load: other lanes set bits meanwhile; a stale 0 costs a test, the atomic OR below decides
          if (!(__hip_atomic_load(&map[y >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) {
            ay = dot3(r, sigma_of(phi[y]));
            const double prod = ax * ay;
            if (prod > 0.0) {                            // else p = 0: never bonded, no random number
              const double p = bond_probability(prod, beta2);
              // +i: link (x, 0), -i: link (y, 0), +j: link (x, 1), -j: link (y, 1)
              const U4 w = philox4x32_10((d & 1u) ? y : x, key.chain, key.step, (uint32_t)P_SIGMA_BOND << 24, key.k0, key.k1);
              const double uni = (d & 2u) ? u01(w.z, w.w) : u01(w.x, w.y);
              if (uni < p) add = !(atomicOr(&map[y >> 5], bit) & bit);
            }
          }
        }
        const unsigned long long joiners = __ballot(add);
        if (joiners) {                                   // wave uniform
          const uint32_t leader = (uint32_t)__builtin_ctzll(joiners);
          uint32_t first = 0;
          if (wave_lane == leader) first = atomicAdd(&s_tail[slot], (uint32_t)__builtin_popcountll(joiners));
          first = __shfl(first, leader);
          const uint32_t pos = first + (uint32_t)__builtin_popcountll(joiners & ((1ull << wave_lane) - 1ull));
          if (add && pos < N) {
            qv[pos] = y;
            qa[pos] = ay;
          }
        }
      }
      team_sync<BLOCK>();
      head = tail;
      tail = s_tail[slot];
      if (BLOCK) __syncthreads();                        // nobody appends to the next level before everybody has read the tail
    }

    for (uint32_t q = lane; q < tail; q += T) {
      const uint32_t x = qv[q];
      const double c = 2.0 * qa[q];
      const V3 s = sigma_of(phi[x]);
      phi[x] = angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
      map[x >> 5] = 0;                                   // every bit of the word that is set belongs to a member
    }
    total += tail;
    // the next update reads what this one stored (other lanes, other waves of the team): drain the stores first
    team_sync<BLOCK>();
  }
  if (cluster_sites && lane == 0) cluster_sites[b] += total;
}

// n_updates updates of every chain of a rotated level, in place: the algorithm of sigma_cluster_kernel (teams of one wave or
// one workgroup; frontier expansion over a queue of (vertex, a) pairs; a lane takes one (frontier vertex, direction) task,
// pre-checks the membership bitmap with a relaxed atomic load and claims the neighbour with an atomic OR; one ballot, one
// prefix count and one atomic add on the tail counter per wave and round; reflections from the queue once growth has ended,
// the same pass clearing the members' bitmap words) with the neighbour and the link of a task from the plane arithmetic of
// the rotated level (RotatedGeometry, sigma_cluster_device.hpp, names the links).  The queue carries the linear index: one
// division by ht per task (DESIGN.md 4.6a says why not (a, b, p) packed).
// The frontier loop ends after at most n levels (a vertex joins once, a level without a new member is the last one); `level <
// n` states that cap explicitly.  Queue positions are < n for the same reason; the store is guarded all the same.
template <bool BLOCK, bool LDS_MAP>
__global__ void __launch_bounds__(BLOCK ? kClusterBlockThreads : kClusterThreads)
    sigma_rot_cluster_kernel(double2 *phi_all, SigmaLevel L, double beta2, uint32_t B, uint32_t n_updates, RngKey key0,
                             uint32_t *queue_vertex, double *queue_a, uint32_t *map_all, uint32_t words, uint32_t *cluster_sites) {
  extern __shared__ uint32_t lds_map[];
  __shared__ uint32_t s_tail[kScWaveChains];
  const uint32_t T = BLOCK ? blockDim.x : (uint32_t)kWave;
  const uint32_t lane = BLOCK ? threadIdx.x : threadIdx.x & (kWave - 1);
  const uint32_t wave_lane = threadIdx.x & (kWave - 1);
  const uint32_t slot = BLOCK ? 0 : threadIdx.x >> 6;
  const uint32_t b = BLOCK ? blockIdx.x : blockIdx.x * kScWaveChains + slot;
  if (b >= B) return;                                    // team uniform (BLOCK: the grid has B workgroups)
  const uint32_t n = L.nvert(), ht = L.ht, hx = L.hx, nq = L.q;
  double2 *phi = phi_all + (size_t)b * n;
  uint32_t *qv = queue_vertex + (size_t)b * n;
  double *qa = queue_a + (size_t)b * n;
  uint32_t *map = LDS_MAP ? lds_map + slot * words : map_all + (size_t)b * words;
  for (uint32_t w = lane; w < words; w += T) map[w] = 0;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t total = 0;
  team_sync<BLOCK>();

  for (uint32_t k = 0; k < n_updates; ++k, ++key.step) {
    double u, v, us, unused;
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 0, u, v);
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 1, us, unused);
    const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
    double sa, ca;
    sincos(kTwoPi * v - kPi, &sa, &ca);
    const V3 r{rho * ca, rho * sa, rz};
    uint32_t seed = (uint32_t)(us * (double)n);
    seed = seed < n ? seed : n - 1;
    if (lane == 0) {
      qv[0] = seed;
      qa[0] = dot3(r, sigma_of(phi[seed]));
      map[seed >> 5] = 1u << (seed & 31u);
      s_tail[slot] = 1;
    }
    team_sync<BLOCK>();

    uint32_t head = 0, tail = 1;
    for (uint32_t level = 0; level < n && head < tail; ++level) {
      for (uint32_t base = head; base < tail; base += T / 4) {  // team uniform trip count: the ballot below sees whole waves
        const uint32_t q = base + (lane >> 2), d = lane & 3u;
        bool add = false;
        uint32_t y = 0;
        double ay = 0.0;
        if (q < tail) {
          const uint32_t x = qv[q];
          const double ax = qa[q];
          const bool odd = x >= nq;                      // plane O
          const uint32_t c = odd ? x - nq : x, cb = c / ht, ca_ = c - cb * ht;
          // E: d -> O(a - (d >> 1), b - (d & 1)); O: d' -> E(a + 1 - (d' >> 1), b + 1 - (d' & 1))
          uint32_t ya = ca_, yb = cb;
          if (odd) {
            if (!(d & 2u)) ya = ca_ + 1 == ht ? 0 : ca_ + 1;
            if (!(d & 1u)) yb = cb + 1 == hx ? 0 : cb + 1;
          } else {
            if (d & 2u) ya = ca_ == 0 ? ht - 1 : ca_ - 1;
            if (d & 1u) yb = cb == 0 ? hx - 1 : cb - 1;
          }
          const uint32_t yc = yb * ht + ya;              // < nq
          y = odd ? yc : nq + yc;
          const uint32_t bit = 1u << (y & 31u);
          // a relaxed atomic load: other lanes set bits meanwhile; a stale 0 costs a test, the atomic OR below decides
          if (!(__hip_atomic_load(&map[y >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) {
            ay = dot3(r, sigma_of(phi[y]));
            const double prod = ax * ay;
            if (prod > 0.0) {                            // else p = 0: never bonded, no random number
              const double p = bond_probability(prod, beta2);
              // the link's name from its E end: (x, d) from E, (y, 3 - d') from O
              const uint32_t e = odd ? yc : x, de = odd ? 3u - d : d;
              const U4 w = philox4x32_10(e, key.chain, key.step, ((uint32_t)P_SIGMA_BOND << 24) | (de >> 1), key.k0, key.k1);
              const double uni = (de & 1u) ? u01(w.z, w.w) : u01(w.x, w.y);
              if (uni < p) add = !(atomicOr(&map[y >> 5], bit) & bit);
            }
          }
        }
        const unsigned long long joiners = __ballot(add);
        if (joiners) {                                   // wave uniform
          const uint32_t leader = (uint32_t)__builtin_ctzll(joiners);
          uint32_t first = 0;
          if (wave_lane == leader) first = atomicAdd(&s_tail[slot], (uint32_t)__builtin_popcountll(joiners));
          first = __shfl(first, leader);
          const uint32_t pos = first + (uint32_t)__builtin_popcountll(joiners & ((1ull << wave_lane) - 1ull));
          if (add && pos < n) {
            qv[pos] = y;
            qa[pos] = ay;
          }
        }
      }
      team_sync<BLOCK>();
      head = tail;
      tail = s_tail[slot];
      tail = tail < n ? tail : n;                        // the queue holds n entries (a vertex joins once)
      if (BLOCK) __syncthreads();                        // nobody appends to the next level before everybody has read the tail
    }

    for (uint32_t q = lane; q < tail; q += T) {
      const uint32_t x = qv[q];
      const double c = 2.0 * qa[q];
      const V3 s = sigma_of(phi[x]);
      phi[x] = angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
      map[x >> 5] = 0;                                   // every bit of the word that is set belongs to a member
    }
    total += tail;
    // the next update reads what this one stored (other lanes, other waves of the team): drain the stores first
    team_sync<BLOCK>();
  }
  if (cluster_sites && lane == 0) cluster_sites[b] += total;
}

// ---- the improved draw (mlmcpi_sigma_level_cluster_improved_draw) ------------------------------------------
// What the improved kernel asks of a geometry: the neighbour across direction d of vertex x, the name of that link for its
// uniform (Philox site and sub-counter, and which of the call's two uniforms), and the slices of a vertex.  The two kernels
// above spell the same arithmetic out; they are not rebuilt on these, so that their instructions stay what they were.
struct WolffLatticeTasks {
  LatticeGeometry g;
  __device__ __forceinline__ uint32_t nvert() const { return g.nvert(); }
  __device__ __forceinline__ uint32_t position(uint32_t x, uint32_t d) const { return g.position(x, d); }
  __device__ __forceinline__ uint32_t neighbour(uint32_t x, uint32_t d, uint32_t &site, uint32_t &sub, bool &second) const {
    const uint32_t Mt = g.Mt, Mx = g.Mx, i = x % Mt, j = x / Mt;
    uint32_t y;
    if (d == 0) y = i + 1 == Mt ? x - i : x + 1;
    else if (d == 1) y = i == 0 ? x + (Mt - 1) : x - 1;
    else if (d == 2) y = j + 1 == Mx ? i : x + Mt;
    else y = j == 0 ? x + (Mx - 1) * Mt : x - Mt;
    site = (d & 1u) ? y : x;                             // +i: link (x, 0), -i: link (y, 0), +j: link (x, 1), -j: link (y, 1)
    sub = 0;
    second = d & 2u;
    return y;
  }
};

struct WolffRotatedTasks {
  RotatedGeometry g;
  __device__ __forceinline__ uint32_t nvert() const { return g.nvert(); }
  __device__ __forceinline__ uint32_t position(uint32_t x, uint32_t d) const { return g.position(x, d); }
  __device__ __forceinline__ uint32_t neighbour(uint32_t x, uint32_t d, uint32_t &site, uint32_t &sub, bool &second) const {
    const uint32_t ht = g.ht, hx = g.hx, nq = g.q;
    const bool odd = x >= nq;                            // plane O
    const uint32_t c = odd ? x - nq : x, cb = c / ht, ca = c - cb * ht;
    // E: d -> O(a - (d >> 1), b - (d & 1)); O: d' -> E(a + 1 - (d' >> 1), b + 1 - (d' & 1))
    uint32_t ya = ca, yb = cb;
    if (odd) {
      if (!(d & 2u)) ya = ca + 1 == ht ? 0 : ca + 1;
      if (!(d & 1u)) yb = cb + 1 == hx ? 0 : cb + 1;
    } else {
      if (d & 2u) ya = ca == 0 ? ht - 1 : ca - 1;
      if (d & 1u) yb = cb == 0 ? hx - 1 : cb - 1;
    }
    const uint32_t yc = yb * ht + ya;                    // < nq
    const uint32_t de = odd ? 3u - d : d;                // the link's name from its E end: (x, d) from E, (y, 3 - d') from O
    site = odd ? yc : x;
    sub = de >> 1;
    second = de & 1u;
    return odd ? yc : nq + yc;
  }
};

// ---- the improved estimators of the single-cluster update ---------------------------------------------------
// What the improved instances of the Wolff kernels carry beside the plain draw's arguments.  Per chain, in the workspace: the
// slice table P_d(i) = the sum of q(a) over the members in slice i of direction d, [M_0 + M_1] int64, t slices first; the list
// of the occupied slices of either direction, [M_0 + M_1] uint32; the accumulators, [kWolffSums + n_out] int64: A, Ac_0, As_0,
// Ac_1, As_1, then one per (d, tau) in the layout of mlmcpi_sigma_level_correlator; the weights (w^s, w^c) of every slice,
// [M_0 + M_1][2] double.  The kernel zeroes table and accumulators and forms the weights when it starts (sw_phase inside the
// update loop costs the registers of its expansion across the whole loop, as in sigma_sw_chain.hip), and every update leaves
// table and accumulators zero.  structure and corr may be NULL.
constexpr uint32_t kWolffSums = 5;

struct WolffImproved {
  long long *table, *acc;
  uint32_t *occupied;
  double *weights;
  double *improved, *structure, *corr;
  uint32_t M0, M1;
  double scale, inv_scale;   // 2^(s - 64) and 2^-s, s the fixed-point scale of the lag accumulators (sw_lag_scale)
  __device__ __forceinline__ uint32_t slots() const { return kWolffSums + M0 / 2 + M1 / 2 + 2; }
};

// the sum of v over the lanes of the wave (every lane of the wave calls it)
__device__ __forceinline__ long long wolff_wave_sum(long long v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the wave's sum of v onto *slot, one atomic per wave (every lane of the wave calls it)
__device__ __forceinline__ void wolff_wave_add(long long *slot, long long v) {
  v = wolff_wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0 && v) __hip_atomic_fetch_add(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void wolff_improved_clear(const WolffImproved &w, uint32_t b, uint32_t lane, uint32_t T) {
  const uint32_t M = w.M0 + w.M1, S = w.slots();
  for (uint32_t i = lane; i < M; i += T) w.table[(size_t)b * M + i] = 0;
  for (uint32_t k = lane; k < S; k += T) w.acc[(size_t)b * S + k] = 0;
  if (w.structure)
    for (uint32_t i = lane; i < M; i += T) {
      double ws, wc;
      sw_phase(i < w.M0 ? i : i - w.M0, i < w.M0 ? w.M0 : w.M1, ws, wc);
      w.weights[2 * ((size_t)b * M + i)] = ws;
      w.weights[2 * ((size_t)b * M + i) + 1] = wc;
    }
}

// a member at (x0, x1) with a = r . sigma before the update: q(a) onto its two slices
__device__ __forceinline__ void wolff_slice_add(const WolffImproved &w, uint32_t b, uint32_t x0, uint32_t x1, double a) {
  long long *tab = w.table + (size_t)b * (w.M0 + w.M1);
  const long long q = sw_fixed(a);
  if (x0 < w.M0) __hip_atomic_fetch_add(tab + x0, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (x1 < w.M1) __hip_atomic_fetch_add(tab + w.M0 + x1, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The epilogue of an update whose `size` members have been added to the table; every lane of the team calls it and `count`
// [2] is the team's in LDS.  Three phases with the team's fence between them; every sum is an integer sum and every output one
// fixed expression of such sums, so the outputs do not depend on the team, on the order of the queue or on who adds first.
// (1) Every slice of either direction: an occupied one (P != 0: the members of a cluster share the sign of a, so a slice with
//     members sums to 0 only where every q(a) is 0, and then it contributes 0 everywhere; it is then also missing from w_d of
//     (2), which can drop the largest lag of the slices either side of it: every member of such a slice has |a| < 2^-33, and a
//     vertex other than the seed joins across a bond of probability <= 2 beta |a| < beta 2^-32) joins the list of its direction and
//     adds P to A (direction t only) and llrint((double)P w) to Ac_d, As_d, (w^s, w^c) from sw_phase.
// (2) Every lag tau <= min(M_d / 2, w_d - 1), w_d the occupied slices (a link moves the slice index by at most 1, so the
//     occupied slices are an arc of the ring and larger lags pair nothing): the occupied slices i meet slice (i + tau) mod M_d
//     of the table, llrint(((double)P (double)P') 2^(s - 64)) summed per wave and added to the accumulator of (d, tau).
// (3) The outputs, each from its accumulator, which is zeroed again, and the occupied slices of the table back to 0.
template <bool BLOCK>
__device__ __forceinline__ void wolff_improved_finish(const WolffImproved &w, uint32_t b, uint32_t lane, uint32_t T, uint32_t size,
                                                      uint32_t *count) {
  const uint32_t M0 = w.M0, M1 = w.M1, M = M0 + M1, n_out = M0 / 2 + M1 / 2 + 2;
  long long *tab = w.table + (size_t)b * M;
  long long *acc = w.acc + (size_t)b * (kWolffSums + n_out);
  uint32_t *occ = w.occupied + (size_t)b * M;
  if (lane < 2) count[lane] = 0;
  team_sync<BLOCK>();                                    // and the adds of the reflection pass have landed

  long long sA = 0, c0 = 0, s0 = 0, c1 = 0, s1 = 0;
  for (uint32_t i = lane; i < M; i += T) {
    const long long P = __hip_atomic_load(tab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (P == 0) continue;
    const bool d = i >= M0;
    const uint32_t x = d ? i - M0 : i, Md = d ? M1 : M0;
    if (w.structure) {
      const double ws = w.weights[2 * ((size_t)b * M + i)], wc = w.weights[2 * ((size_t)b * M + i) + 1];
      const long long c = llrint((double)P * wc), s = llrint((double)P * ws);
      if (d) c1 += c, s1 += s;
      else c0 += c, s0 += s;
    }
    if (!d) sA += P;
    const uint32_t k = atomicAdd(count + (d ? 1 : 0), 1u);
    if (k < Md) occ[(d ? M0 : 0) + k] = x;
  }
  wolff_wave_add(acc + 0, sA);
  if (w.structure) {
    wolff_wave_add(acc + 1, c0);
    wolff_wave_add(acc + 2, s0);
    wolff_wave_add(acc + 3, c1);
    wolff_wave_add(acc + 4, s1);
  }
  team_sync<BLOCK>();

  const uint32_t w0 = count[0] < M0 ? count[0] : M0, w1 = count[1] < M1 ? count[1] : M1;
  if (w.corr) {
#pragma unroll 1
    for (uint32_t d = 0; d < 2; ++d) {
      const uint32_t Md = d ? M1 : M0, wd = d ? w1 : w0, base = d ? M0 : 0;
      long long *lag = acc + kWolffSums + (d ? M0 / 2 + 1 : 0);
      const uint32_t ntau = wd == 0 ? 0 : (wd - 1 < Md / 2 ? wd - 1 : Md / 2) + 1;   // team uniform: the wave sums see whole waves
      for (uint32_t tau = 0; tau < ntau; ++tau) {
        long long part = 0;
        for (uint32_t k = lane; k < wd; k += T) {
          const uint32_t i = occ[base + k];
          uint32_t j = i + tau;
          if (j >= Md) j -= Md;
          if (i < Md && j < Md) {
            const long long P = __hip_atomic_load(tab + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const long long Q = tau ? __hip_atomic_load(tab + base + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : P;
            part += llrint(((double)P * (double)Q) * w.scale);
          }
        }
        wolff_wave_add(lag + tau, part);
      }
    }
    team_sync<BLOCK>();
  }

  const double f = 3.0 / (double)size;
  if (w.corr)
    for (uint32_t k = lane; k < n_out; k += T) {
      const long long v = __hip_atomic_load(acc + kWolffSums + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (v) {
        w.corr[(size_t)b * n_out + k] += ((double)v * w.inv_scale) * f;
        acc[kWolffSums + k] = 0;
      }
    }
  for (uint32_t k = lane; k < w0; k += T) {
    const uint32_t i = occ[k];
    if (i < M0) tab[i] = 0;
  }
  for (uint32_t k = lane; k < w1; k += T) {
    const uint32_t i = occ[M0 + k];
    if (i < M1) tab[M0 + i] = 0;
  }
  if (lane == 0) {
    const double x = (double)__hip_atomic_load(acc + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) * (1.0 / kSwFix);
    w.improved[b] += (x * x) * f;
    acc[0] = 0;
    if (w.structure)
      for (uint32_t d = 0; d < 2; ++d) {
        const double xc = (double)__hip_atomic_load(acc + 1 + 2 * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) * (1.0 / kSwFix);
        const double xs = (double)__hip_atomic_load(acc + 2 + 2 * d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) * (1.0 / kSwFix);
        w.structure[(size_t)b * 2 + d] += (xc * xc) * f;
        w.structure[(size_t)b * 2 + d] += (xs * xs) * f;
        acc[1 + 2 * d] = 0;
        acc[2 + 2 * d] = 0;
      }
  }
}

// The update of the two kernels above, decision by decision (the same state and cluster_sites bits), on either geometry, with
// the improved estimators of wolff_improved_finish (above): the reflection pass adds q(a) of every member to
// the chain's slice table, the epilogue of the update turns the table into chi^W, F_d^W and C_d^W(tau) and leaves it zero.
template <class Tasks, bool BLOCK, bool LDS_MAP>
__global__ void __launch_bounds__(BLOCK ? kClusterBlockThreads : kClusterThreads)
    sigma_cluster_improved_kernel(double2 *phi_all, Tasks g, double beta2, uint32_t B, uint32_t n_updates, RngKey key0, uint32_t *queue_vertex,
                                  double *queue_a, uint32_t *map_all, uint32_t words, uint32_t *cluster_sites, WolffImproved imp) {
  extern __shared__ uint32_t lds_map[];
  __shared__ uint32_t s_tail[kScWaveChains];
  __shared__ uint32_t s_occupied[2 * kScWaveChains];
  const uint32_t T = BLOCK ? blockDim.x : (uint32_t)kWave;
  const uint32_t lane = BLOCK ? threadIdx.x : threadIdx.x & (kWave - 1);
  const uint32_t wave_lane = threadIdx.x & (kWave - 1);
  // the wave's number through readfirstlane: the chain and everything addressed through it are then scalars
  const uint32_t slot = BLOCK ? 0 : (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t b = BLOCK ? blockIdx.x : blockIdx.x * kScWaveChains + slot;
  if (b >= B) return;                                    // team uniform (BLOCK: the grid has B workgroups)
  const uint32_t N = g.nvert();
  double2 *phi = phi_all + (size_t)b * N;
  uint32_t *qv = queue_vertex + (size_t)b * N;
  double *qa = queue_a + (size_t)b * N;
  uint32_t *map = LDS_MAP ? lds_map + slot * words : map_all + (size_t)b * words;
  for (uint32_t w = lane; w < words; w += T) map[w] = 0;
  wolff_improved_clear(imp, b, lane, T);
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t total = 0;
  team_sync<BLOCK>();

  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    const V3 r = reflection_normal(key, P_SIGMA_REFLECT);
    double us, unused;
    rng_uniforms(key, 0, P_SIGMA_REFLECT, 1, us, unused);
    uint32_t seed = (uint32_t)(us * (double)N);
    seed = seed < N ? seed : N - 1;
    if (lane == 0) {
      qv[0] = seed;
      qa[0] = dot3(r, sigma_of(phi[seed]));
      map[seed >> 5] = 1u << (seed & 31u);
      s_tail[slot] = 1;
    }
    team_sync<BLOCK>();

    uint32_t head = 0, tail = 1;
    for (uint32_t level = 0; level < N && head < tail; ++level) {
      for (uint32_t base = head; base < tail; base += T / 4) {  // team uniform trip count: the ballot below sees whole waves
        const uint32_t q = base + (lane >> 2), d = lane & 3u;
        bool add = false;
        uint32_t y = 0;
        double ay = 0.0;
        if (q < tail) {
          const uint32_t x = qv[q];
          const double ax = qa[q];
          uint32_t site, sub;
          bool second;
          y = g.neighbour(x, d, site, sub, second);
          const uint32_t bit = 1u << (y & 31u);
          // a relaxed atomic load: other lanes set bits meanwhile; a stale 0 costs a test, the atomic OR below decides
          if (y < N && !(__hip_atomic_load(&map[y >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) {
            ay = dot3(r, sigma_of(phi[y]));
            const double prod = ax * ay;
            if (prod > 0.0) {                            // else p = 0: never bonded, no random number
              const double p = bond_probability(prod, beta2);
              const U4 w = philox4x32_10(site, key.chain, key.step, ((uint32_t)P_SIGMA_BOND << 24) | sub, key.k0, key.k1);
              const double uni = second ? u01(w.z, w.w) : u01(w.x, w.y);
              if (uni < p) add = !(atomicOr(&map[y >> 5], bit) & bit);
            }
          }
        }
        const unsigned long long joiners = __ballot(add);
        if (joiners) {                                   // wave uniform
          const uint32_t leader = (uint32_t)__builtin_ctzll(joiners);
          uint32_t first = 0;
          if (wave_lane == leader) first = atomicAdd(&s_tail[slot], (uint32_t)__builtin_popcountll(joiners));
          first = __shfl(first, leader);
          const uint32_t pos = first + (uint32_t)__builtin_popcountll(joiners & ((1ull << wave_lane) - 1ull));
          if (add && pos < N) {
            qv[pos] = y;
            qa[pos] = ay;
          }
        }
      }
      team_sync<BLOCK>();
      head = tail;
      tail = s_tail[slot];
      tail = tail < N ? tail : N;                        // the queue holds N entries (a vertex joins once)
      if (BLOCK) __syncthreads();                        // nobody appends to the next level before everybody has read the tail
    }

    for (uint32_t q = lane; q < tail; q += T) {
      const uint32_t x = qv[q];
      const double a = qa[q];
      phi[x] = reflected(sigma_of(phi[x]), a, r);
      map[x >> 5] = 0;                                   // every bit of the word that is set belongs to a member
      wolff_slice_add(imp, b, g.position(x, 0), g.position(x, 1), a);
    }
    wolff_improved_finish<BLOCK>(imp, b, lane, T, tail, s_occupied + 2 * slot);
    total += tail;
    // the next update reads what this one stored (other lanes, other waves of the team): drain the stores first
    team_sync<BLOCK>();
  }
  if (cluster_sites && lane == 0) cluster_sites[b] += total;
}

namespace {

struct ScPlan {
  bool block, lds_map;
  uint32_t threads, words, grid;
  size_t lds_bytes;
};

// Launch plan, a function of the number of vertices and the batch on either geometry.  A team is one wave
// when there are enough chains to give every SIMD of the device a wave (B >= 4 x kComputeUnits), the workgroup otherwise; the
// bitmap sits in LDS where it fits.  Knobs (bit-identical results): MLMCPI_SIGMA_CLUSTER_TEAM=wave|block,
// MLMCPI_SIGMA_CLUSTER_BITMAP=global|lds.
ScPlan sc_plan(uint32_t N, uint32_t B, const Tuning &tune) {
  ScPlan p;
  p.words = (N + 31) / 32;
  p.block = tune.sigma_cluster_team ? tune.sigma_cluster_team == 2 : B < 4 * kComputeUnits;
  p.lds_map = !tune.sigma_cluster_map_global && p.words <= (p.block ? kScBlockLdsWords : kScWaveLdsWords);
  p.threads = p.block ? (N >= 16384 ? kClusterBlockThreads : 256u) : kScWaveChains * kWave;
  p.grid = p.block ? B : (B + kScWaveChains - 1) / kScWaveChains;
  p.lds_bytes = p.lds_map ? (size_t)p.words * sizeof(uint32_t) * (p.block ? 1 : kScWaveChains) : 0;
  return p;
}

DeviceOnce g_sc_attr_once;

// dynamic LDS above 64 KiB: the workgroup team's bitmap up to its bound, on either geometry
int sc_init_attrs() {
  return once_per_device(g_sc_attr_once, []() -> int {
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cluster_kernel<true, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kScBlockLdsWords * sizeof(uint32_t)));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_cluster_kernel<true, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kScBlockLdsWords * sizeof(uint32_t)));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cluster_improved_kernel<WolffLatticeTasks, true, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kScBlockLdsWords * sizeof(uint32_t)));
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_cluster_improved_kernel<WolffRotatedTasks, true, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kScBlockLdsWords * sizeof(uint32_t)));
    return MLMCPI_OK;
  });
}

int sc_check(const mlmcpi_lattice_action *act, const char *what) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: the Wolff single-cluster update is built for the O(3) nonlinear sigma model only "
                "(action kind %d)", what, act->kind);
  if (int rc = check_lattice(act)) return rc;
  if (!(act->beta > 0.0)) return fail(MLMCPI_ERR_INVALID, "beta must be positive");
  return MLMCPI_OK;
}

// workspace sections: queue a [B N] double, queue vertex [B N] uint32, bitmap [B words] uint32
size_t sc_section_a(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(double)); }
size_t sc_section_v(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(uint32_t)); }
size_t sc_section_map(uint32_t N, uint32_t B) { return align256((size_t)B * ((N + 31) / 32) * sizeof(uint32_t)); }
size_t sc_workspace(uint32_t N, uint32_t B) { return sc_section_a(N, B) + sc_section_v(N, B) + sc_section_map(N, B); }

// The improved draw's part of the workspace, behind that of the plain draw, and its fixed-point scale.  Per chain the slice
// table [M0 + M1] int64, the accumulators [kWolffSums + n_out] int64, the occupied slices [M0 + M1] uint32 and the weights
// [M0 + M1][2] double.  In the workspace
// and not in LDS: at 1024 x 1024 the table is 16 KiB a chain beside the workgroup team's 128 KiB bitmap, and a
// wave-team workgroup would hold four of them beside its four bitmaps.  n_out and s from sw_lag_scale, where the bound is.
struct ScImprovedLayout {
  uint32_t M0, M1, n_out, s;
  size_t table_bytes, acc_bytes, occupied_bytes, weights_bytes;
  size_t bytes() const { return table_bytes + acc_bytes + occupied_bytes + weights_bytes; }
};

ScImprovedLayout sc_improved_layout(uint32_t N, uint32_t M0, uint32_t M1, uint32_t B) {
  ScImprovedLayout c{};
  c.M0 = M0;
  c.M1 = M1;
  const SwLagScale lags = sw_lag_scale(N, M0, M1);
  c.n_out = lags.n_out;
  c.s = lags.s;
  c.table_bytes = align256((size_t)B * (M0 + M1) * sizeof(long long));
  c.acc_bytes = align256((size_t)B * (kWolffSums + c.n_out) * sizeof(long long));
  c.occupied_bytes = align256((size_t)B * (M0 + M1) * sizeof(uint32_t));
  c.weights_bytes = align256((size_t)B * (M0 + M1) * 2 * sizeof(double));
  return c;
}

// the draw on either geometry, arguments checked; `rot` is the rotated level, NULL on the unrotated Mt x Mx lattice; with
// d_improved the improved instances, whose part of the workspace follows the plain draw's
int sc_draw(uint32_t Mt, uint32_t Mx, const SigmaLevel *rot, double beta, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed,
            uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *d_work, void *stream, double *d_improved = nullptr,
            double *d_structure = nullptr, double *d_corr = nullptr) {
  if (int rc = sc_init_attrs()) return rc;
  const uint32_t N = rot ? rot->nvert() : Mt * Mx;
  const ScPlan p = sc_plan(N, B, tuning());
  char *w = (char *)d_work;
  double *qa = (double *)w;
  uint32_t *qv = (uint32_t *)(w + sc_section_a(N, B));
  uint32_t *map = (uint32_t *)(w + sc_section_a(N, B) + sc_section_v(N, B));
  const RngKey key = make_key(seed, chain0, update0);
  const hipStream_t st = as_stream(stream);
#define MLMCPI_SC_LAUNCH(KERNEL, BLOCK, LDS, ...)                                                                              \
  hipLaunchKernelGGL((KERNEL<BLOCK, LDS>), dim3(p.grid), dim3(p.threads), p.lds_bytes, st, (double2 *)d_phi, __VA_ARGS__, 2.0 * beta, B, \
                     n_updates, key, qv, qa, map, p.words, d_cluster_sites)
#define MLMCPI_SC_DISPATCH(KERNEL, ...)                                                                                        \
  do {                                                                                                                         \
    if (p.block && p.lds_map) MLMCPI_SC_LAUNCH(KERNEL, true, true, __VA_ARGS__);                                               \
    else if (p.block) MLMCPI_SC_LAUNCH(KERNEL, true, false, __VA_ARGS__);                                                      \
    else if (p.lds_map) MLMCPI_SC_LAUNCH(KERNEL, false, true, __VA_ARGS__);                                                    \
    else MLMCPI_SC_LAUNCH(KERNEL, false, false, __VA_ARGS__);                                                                  \
  } while (0)
  if (d_improved) {
    const ScImprovedLayout c = rot ? sc_improved_layout(N, 2 * rot->ht, 2 * rot->hx, B) : sc_improved_layout(N, Mt, Mx, B);
    char *extra = w + sc_workspace(N, B);
    const WolffImproved imp{(long long *)extra, (long long *)(extra + c.table_bytes), (uint32_t *)(extra + c.table_bytes + c.acc_bytes),
                            (double *)(extra + c.table_bytes + c.acc_bytes + c.occupied_bytes), d_improved, d_structure, d_corr, c.M0, c.M1, ldexp(1.0, (int)c.s - 64), ldexp(1.0, -(int)c.s)};
#define MLMCPI_SC_LAUNCH_IMPROVED(TASKS, BLOCK, LDS, G)                                                                        \
  hipLaunchKernelGGL((sigma_cluster_improved_kernel<TASKS, BLOCK, LDS>), dim3(p.grid), dim3(p.threads), p.lds_bytes, st, (double2 *)d_phi, G, \
                     2.0 * beta, B, n_updates, key, qv, qa, map, p.words, d_cluster_sites, imp)
#define MLMCPI_SC_DISPATCH_IMPROVED(TASKS, G)                                                                                  \
  do {                                                                                                                         \
    if (p.block && p.lds_map) MLMCPI_SC_LAUNCH_IMPROVED(TASKS, true, true, G);                                                 \
    else if (p.block) MLMCPI_SC_LAUNCH_IMPROVED(TASKS, true, false, G);                                                        \
    else if (p.lds_map) MLMCPI_SC_LAUNCH_IMPROVED(TASKS, false, true, G);                                                      \
    else MLMCPI_SC_LAUNCH_IMPROVED(TASKS, false, false, G);                                                                    \
  } while (0)
    if (rot) MLMCPI_SC_DISPATCH_IMPROVED(WolffRotatedTasks, WolffRotatedTasks{RotatedGeometry(*rot)});
    else MLMCPI_SC_DISPATCH_IMPROVED(WolffLatticeTasks, (WolffLatticeTasks{LatticeGeometry{Mt, Mx}}));
    MLMCPI_LAUNCH_CHECK("sigma_cluster_improved_kernel");
#undef MLMCPI_SC_DISPATCH_IMPROVED
#undef MLMCPI_SC_LAUNCH_IMPROVED
  } else if (rot) {
    MLMCPI_SC_DISPATCH(sigma_rot_cluster_kernel, *rot);
    MLMCPI_LAUNCH_CHECK("sigma_rot_cluster_kernel");
  } else {
    MLMCPI_SC_DISPATCH(sigma_cluster_kernel, Mt, Mx);
    MLMCPI_LAUNCH_CHECK("sigma_cluster_kernel");
  }
#undef MLMCPI_SC_DISPATCH
#undef MLMCPI_SC_LAUNCH
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_cluster_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = sc_check(act, "mlmcpi_sigma_cluster_workspace_bytes")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  *bytes = sc_workspace(act->Mt * act->Mx, B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_cluster_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed,
                              uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *d_work, void *stream) {
  if (int rc = sc_check(act, "mlmcpi_sigma_cluster_draw")) return rc;
  MLMCPI_REQUIRE(d_phi && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  return sc_draw(act->Mt, act->Mx, nullptr, act->beta, d_phi, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream);
}

int mlmcpi_sigma_level_cluster_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    return mlmcpi_sigma_cluster_workspace_bytes(&act, B, bytes);
  }
  *bytes = sc_workspace(make_level(*level).nvert(), B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_cluster_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                    uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites, void *d_work,
                                    void *stream) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    return mlmcpi_sigma_cluster_draw(&act, d_state, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream);
  }
  const SigmaLevel L = make_level(*level);
  return sc_draw(0, 0, &L, level->beta, d_state, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream);
}

int mlmcpi_sigma_level_cluster_improved_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  size_t plain = 0;
  if (int rc = mlmcpi_sigma_level_cluster_workspace_bytes(level, B, &plain)) return rc;
  MLMCPI_REQUIRE(bytes, "bad arguments");
  const uint32_t N = level->rotated ? make_level(*level).nvert() : level->Mt * level->Mx;
  *bytes = plain + sc_improved_layout(N, level->Mt, level->Mx, B).bytes();
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_cluster_improved_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates,
                                             uint64_t seed, uint32_t chain0, uint32_t update0, uint32_t *d_cluster_sites,
                                             double *d_improved, double *d_structure, double *d_corr, void *d_work, size_t work_bytes,
                                             void *stream) {
  size_t need = 0;
  if (int rc = mlmcpi_sigma_level_cluster_improved_workspace_bytes(level, B ? B : 1, &need)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE(d_improved, "d_improved is NULL: mlmcpi_sigma_level_cluster_draw is the entry point without the improved estimators");
  MLMCPI_REQUIRE(work_bytes >= need, "the workspace is smaller than mlmcpi_sigma_level_cluster_improved_workspace_bytes asks for");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    if (int rc = sc_check(&act, "mlmcpi_sigma_level_cluster_improved_draw")) return rc;
    return sc_draw(act.Mt, act.Mx, nullptr, act.beta, d_state, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream,
                   d_improved, d_structure, d_corr);
  }
  const SigmaLevel L = make_level(*level);
  return sc_draw(0, 0, &L, level->beta, d_state, B, n_updates, seed, chain0, update0, d_cluster_sites, d_work, stream, d_improved,
                 d_structure, d_corr);
}

}  // extern "C"
