// sigma_cluster_device.hpp -- what the cluster samplers of the O(3) nonlinear sigma model share (sigma_cluster.hip: Wolff,
// sigma_sw.hip: Swendsen-Wang; each on the unrotated lattice and on the rotated level of the CoarsenRotate hierarchy): the
// embedding (normal, bond rule, reflection), the team's phase fence, the lock-free union-find and the fixed-order reduction of
// the improved estimator, and the two geometries the kernels are instantiated on.  Includes sigma_device.hpp (through
// sigma_level_device.hpp), so the including file is compiled without fp contraction.
#pragma once
#include "sigma_level_device.hpp"

namespace mlmcpi {

constexpr uint32_t kClusterThreads = 256;        // Wolff, team = wave: four chains per workgroup; SW tiled plan: every launch but the last
constexpr uint32_t kClusterBlockThreads = 1024;  // Wolff, team = workgroup; the fixed configuration of sw_finish; the SW chain plan's workgroup
// SW chain plan: a (8 B), the root's sum (8 B) and the parent (4 B) of every vertex in LDS beside the 12 KiB of sw_finish
constexpr uint32_t kSwChainBytesPerVertex = 20;
constexpr uint32_t kSwChainMaxN = (160 * 1024 - 12 * 1024 - 512) / kSwChainBytesPerVertex;  // 7552 vertices
constexpr double kSwFix = 4294967296.0;          // 2^32
constexpr int kUfPlain = -1;                     // uf_find: plain loads (nobody writes the parents any more)

// ---- host: what both samplers ask of a level ---------------------------------------------------------------------------------
inline int check_cluster_level(const mlmcpi_sigma_level *level) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(level->beta > 0.0, "beta must be positive");
  return MLMCPI_OK;
}

// an unrotated level IS the lattice and takes the lattice's entry point
inline mlmcpi_lattice_action level_as_lattice(const mlmcpi_sigma_level *l) {
  return mlmcpi_lattice_action{MLMCPI_NONLINEAR_SIGMA, l->Mt, l->Mx, l->beta, 0.0};
}

// ---- the embedding ---------------------------------------------------------------------------------------------------------
// the reflection normal of an update: (u, v) of (site 0, sub 0) -> r_z = 1 - 2 u, azimuth 2 pi v - pi.  Wolff draws it under
// P_SIGMA_REFLECT, Swendsen-Wang under P_SIGMA_SW_REFLECT.
__device__ __forceinline__ V3 reflection_normal(const RngKey &key, uint32_t purpose) {
  double u, v;
  rng_uniforms(key, 0, purpose, 0, u, v);
  const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
  double sa, ca;
  sincos(kTwoPi * v - kPi, &sa, &ca);
  return V3{rho * ca, rho * sa, rz};
}

// the bond probability of a link with prod = a_x a_y > 0 (prod <= 0: p = 0, never bonded, and no caller asks)
__device__ __forceinline__ double bond_probability(double prod, double beta2) { return 1.0 - exp(fmin(0.0, -(beta2 * prod))); }

// the product first: the same bits from either end of the link
__device__ __forceinline__ bool bonded(double ax, double ay, double beta2, double uni) {
  const double prod = ax * ay;
  if (!(prod > 0.0)) return false;                       // p = 0: never bonded
  return uni < bond_probability(prod, beta2);
}

// sigma' = sigma - 2 a r in the canonical form (sigma2d.hip)
__device__ __forceinline__ double2 reflected(const V3 &s, double a, const V3 &r) {
  const double c = 2.0 * a;
  return angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
}

// What orders one phase of a team behind the one before it: the phase's stores (state, queue, bitmap) drained and, for a
// team of several waves, the barrier.  A team of one wave runs in lockstep and needs the drain only.
template <bool BLOCK>
__device__ __forceinline__ void team_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  if (BLOCK) __syncthreads();
  else __builtin_amdgcn_wave_barrier();
}

// ---- the geometries ---------------------------------------------------------------------------------------------------------
// A geometry answers what the Swendsen-Wang kernels and the host ask and nothing else: the number of vertices, which vertices
// own links, how many each, their far ends and their bond bits.  The chain kernel of sigma_sw.hip is written once and
// instantiated on LatticeGeometry and RotatedGeometry; its tile front ends (bond + label, merge) differ for real and stay one
// per geometry, and so do the Wolff kernels of sigma_cluster.hip (the reason is given there), which walk the same links.

// The unrotated lattice: vertex l = Mt j + i; link (l, 0) joins l to its +i neighbour, link (l, 1) to its +j neighbour (periodic,
// 2 N links; on an extent of 2 the two links between a pair are two links with a uniform each).  One Philox call per vertex:
// site l, sub 0, u decides link (l, 0), v decides link (l, 1).
struct LatticeGeometry {
  uint32_t Mt, Mx;
  static constexpr uint32_t kOwnedLinks = 2;
  static constexpr bool kStructure = false;
  static constexpr bool kRoots = false;
  __host__ __device__ uint32_t nvert() const { return Mt * Mx; }
  __host__ __device__ uint32_t nowners() const { return Mt * Mx; }
  // the structure sums: the periodic extent of direction d (0: t, 1: x) and the position of vertex l along it, l at (i, j)
  __host__ __device__ uint32_t extent(uint32_t d) const { return d ? Mx : Mt; }
  __device__ __forceinline__ uint32_t position(uint32_t l, uint32_t d) const { return d ? l / Mt : l % Mt; }

  __device__ __forceinline__ void far_ends(uint32_t l, uint32_t (&y)[2]) const {
    const uint32_t i = l % Mt, j = l / Mt;
    y[0] = i + 1 == Mt ? l - i : l + 1;
    y[1] = j + 1 == Mx ? i : l + Mt;
  }

  // (bond of link (l, 0), bond of link (l, 1)) as bits 0 and 1
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t l, double a, double a_right, double a_up, double beta2) {
    const U4 w = philox4x32_10(l, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
    return (bonded(a, a_right, beta2, u01(w.x, w.y)) ? 1u : 0u) | (bonded(a, a_up, beta2, u01(w.z, w.w)) ? 2u : 0u);
  }
  // the form the chain kernel calls on either geometry: ay[d] = a of the far end of link (l, d).  The bond + label kernel keeps
  // the scalar form: built through this one it comes out with its LDS reads in another order.
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t l, double a, const double (&ay)[2], double beta2) {
    return bonds(key, l, a, ay[0], ay[1], beta2);
  }
};

// The rotated level (sigma_level_device.hpp): n = 2 q vertices, plane E then plane O of ht x hx each, index p q + ht b + a.  It is
// bipartite: every link has exactly one E end, so the 2 n links are named (e, d) with e an E vertex (e < q) and d its direction
// in the reference's order: E(a, b) -> O(a, b), O(a, b-1), O(a-1, b), O(a-1, b-1).  Seen from O(a, b), direction d' -> E(a+1, b+1),
// E(a+1, b), E(a, b+1), E(a, b) crosses link (neighbour, 3 - d').  Where a plane extent is 1 several of the four neighbours of a
// vertex are one vertex; those are distinct links with a uniform each.  Two Philox calls per E vertex: site e, sub d >> 1, u
// decides link (e, d) for d even, v for d odd.
struct RotatedGeometry {
  uint32_t ht, hx, q;  // q = ht hx
  static constexpr uint32_t kOwnedLinks = 4;
  static constexpr bool kStructure = false;
  static constexpr bool kRoots = false;
  explicit RotatedGeometry(const SigmaLevel &L) : ht(L.ht), hx(L.hx), q(L.q) {}
  __host__ __device__ uint32_t nvert() const { return 2 * q; }
  __host__ __device__ uint32_t nowners() const { return q; }
  // the structure sums: the level's extents Mt = 2 ht, Mx = 2 hx; plane p, cell (a, b) sits at (i, j) = (2 a + p, 2 b + p), the
  // slice assignment of mlmcpi_sigma_level_correlator
  __host__ __device__ uint32_t extent(uint32_t d) const { return 2 * (d ? hx : ht); }
  __device__ __forceinline__ uint32_t position(uint32_t l, uint32_t d) const {
    const uint32_t p = l >= q ? 1u : 0u, c = l - p * q;
    return 2 * (d ? c / ht : c % ht) + p;
  }

  __device__ __forceinline__ void far_ends(uint32_t e, uint32_t (&y)[4]) const {
    const uint32_t cb = e / ht, ca = e - cb * ht;
    const uint32_t am = ca == 0 ? ht - 1 : ca - 1, bm = cb == 0 ? hx - 1 : cb - 1;
    y[0] = q + cb * ht + ca;
    y[1] = q + bm * ht + ca;
    y[2] = q + cb * ht + am;
    y[3] = q + bm * ht + am;
  }

  // the bonds of the links (e, 0) .. (e, 3) as bits 0 .. 3; ao[d] = a of the O end of link (e, d)
  static __device__ __forceinline__ uint32_t bonds(const RngKey &key, uint32_t e, double a, const double (&ao)[4], double beta2) {
    const U4 w0 = philox4x32_10(e, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
    const U4 w1 = philox4x32_10(e, key.chain, key.step, ((uint32_t)P_SIGMA_SW_BOND << 24) | 1u, key.k0, key.k1);
    return (bonded(a, ao[0], beta2, u01(w0.x, w0.y)) ? 1u : 0u) | (bonded(a, ao[1], beta2, u01(w0.z, w0.w)) ? 2u : 0u) |
           (bonded(a, ao[2], beta2, u01(w1.x, w1.y)) ? 4u : 0u) | (bonded(a, ao[3], beta2, u01(w1.z, w1.w)) ? 8u : 0u);
  }
};

// A geometry whose kernels also form the structure sums (the improved structure factor, below): the compile-time option of the
// chain kernel.  It carries the caller's accumulator [B][2] and the chain kernel's table of weights [B][2 (M_0 + M_1)], so that
// the instances on the plain geometries keep their arguments.
template <class G>
struct WithStructure : G {
  double *structure, *weights;
  static constexpr bool kStructure = true;
  WithStructure(const G &g, double *s, double *w) : G(g), structure(s), weights(w) {}
};

// A geometry whose chain kernel also leaves every vertex's final root and q(a) of the field before the update in the workspace,
// [B][N] each, where the tiled plan has them after its resolve launch (the improved correlator, below, reads them from there
// under either plan).  The caller launches it with one update per launch.
template <class G>
struct WithRoots : G {
  uint32_t *roots;
  long long *qa;
  static constexpr bool kRoots = true;
  WithRoots(const G &g, uint32_t *r, long long *q) : G(g), roots(r), qa(q) {}
};

// ---- the union-find of the Swendsen-Wang labelling -------------------------------------------------------------------------
// The parent of a vertex is a vertex of its cluster with a smaller or equal index; a root is its own parent.  union(x, y): find
// both roots, hang the larger under the smaller with an atomic min on the parent word of the larger; if the word held
// something else meanwhile (another lane got there first), go on with (what it held, the smaller root): the edge the min may
// have replaced is the one that pair restores.  max(x, y) decreases with every retry, a path visits decreasing indices: the
// number of vertices bounds every loop, and the final root of a component is its smallest vertex whatever the order of
// arrival.  Every loop carries that bound as `cap`; a cap that is hit all the same sets `capped`, which the kernels turn into
// a status word the entry point returns as an error.  No loop waits on another lane's store.
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_parent(const uint32_t *parent, uint32_t x) {
  // other lanes (tiled plan: workgroups on other XCDs) lower parent words meanwhile: an atomic load of that scope, not a plain one
  if constexpr (SCOPE == kUfPlain) return parent[x];
  else return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
}

// the root above x; a path visits strictly decreasing indices, so `cap` >= the number of vertices bounds it
template <int SCOPE>
__device__ __forceinline__ uint32_t uf_find(const uint32_t *parent, uint32_t x, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {
    const uint32_t p = uf_parent<SCOPE>(parent, x);
    if (p == x) return x;
    x = p;
  }
  capped = true;
  return x;
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(uint32_t *parent, uint32_t x, uint32_t y, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {                // max(x, y) decreases with every retry
    x = uf_find<SCOPE>(parent, x, cap, capped);
    y = uf_find<SCOPE>(parent, y, cap, capped);
    if (x == y || capped) return;                        // x == y: also union(x, x), a no-op
    if (x < y) {
      const uint32_t t = x;
      x = y;
      y = t;
    }
    const uint32_t old = __hip_atomic_fetch_min(parent + x, y, __ATOMIC_RELAXED, SCOPE);
    if (old == x) return;                                // x was a root still: it hangs under y now
    x = old;                                             // somebody else hung x under `old`: unite that with y
  }
  capped = true;
}

// ---- Swendsen-Wang: the coin, the fixed point and the reductions -----------------------------------------------------------
__device__ __forceinline__ bool sw_coin(const RngKey &key, uint32_t root) {
  double u, unused;
  rng_uniforms(key, root, P_SIGMA_SW_FLIP, 0, u, unused);
  return u < 0.5;
}

__device__ __forceinline__ long long sw_fixed(double a) { return llrint(a * kSwFix); }

// sum over the roots of (A_C 2^-32)^2 and their number, in the fixed configuration (kClusterBlockThreads threads, every thread
// of the workgroup calls it); thread 0 adds 3 / N x the sum to *improved and the number to *clusters (either may be NULL)
__device__ __forceinline__ void sw_finish(const uint32_t *parent, const long long *sum, uint32_t N, double *red, uint32_t *redc,
                                          double *improved, uint32_t *clusters) {
  const uint32_t t = threadIdx.x;
  double s = 0.0;
  uint32_t c = 0;
  for (uint32_t l = t; l < N; l += kClusterBlockThreads)
    if (parent[l] == l) {
      const double A = (double)sum[l] * (1.0 / kSwFix);
      s += A * A;
      ++c;
    }
  red[t] = s;
  redc[t] = c;
  __syncthreads();
  for (uint32_t off = kClusterBlockThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
      red[t] += red[t + off];
      redc[t] += redc[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (improved) *improved += red[0] * (3.0 / (double)N);
    if (clusters) *clusters += redc[0];
  }
}

// ---- Swendsen-Wang: the structure sums (improved structure factor at the lowest momentum) ----------------------
// the weights of a vertex at position x of a periodic direction of extent M: s = sin(2 pi x / M), c = cos(2 pi x / M).  The one
// place that forms them, from the integers: both plans and both geometries get the same bits, and M = 2 gives exactly 0 and +-1.
__device__ __forceinline__ void sw_phase(uint32_t x, uint32_t M, double &s, double &c) { sincospi(2.0 * (double)x / (double)M, &s, &c); }

constexpr uint32_t kSwCombineRounds = 4;   // roots a wave combines for before its left-over lanes add one by one
constexpr uint32_t kSwCombineMin = 4;      // lanes that must share a root for the wave reduction to be the cheaper way

// v[0 .. NV) of every active lane added onto slot[root + k stride], k < NV.  Integer adds commute, so the lanes of a wave that share
// a root may add up first and send one atomic per value; the slots hold the same bits either way.  The percolating cluster
// otherwise serialises every lane of every wave on one address.  Every lane of the wave calls it: the loop's trip count comes
// from ballots and is uniform, the shuffles run with all lanes, and no lane waits on another lane's store.
template <int SCOPE, uint32_t NV>
__device__ __forceinline__ void sw_add_combined(long long *slot, size_t stride, uint32_t root, bool active, const long long (&v)[NV]) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  unsigned long long todo = __ballot(active);
  for (uint32_t round = 0; round < kSwCombineRounds && todo; ++round) {
    const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
    const bool same = ((todo >> lane) & 1ull) && root == (uint32_t)__shfl((int)root, (int)lead);
    const unsigned long long m = __ballot(same);
    todo &= ~m;
    if ((uint32_t)__builtin_popcountll(m) < kSwCombineMin) {
      if (same)
        for (uint32_t k = 0; k < NV; ++k) __hip_atomic_fetch_add(slot + root + k * stride, v[k], __ATOMIC_RELAXED, SCOPE);
      continue;
    }
    for (uint32_t k = 0; k < NV; ++k) {
      long long s = same ? v[k] : 0;
      for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == lead) __hip_atomic_fetch_add(slot + root + k * stride, s, __ATOMIC_RELAXED, SCOPE);
    }
  }
  if ((todo >> lane) & 1ull)
    for (uint32_t k = 0; k < NV; ++k) __hip_atomic_fetch_add(slot + root + k * stride, v[k], __ATOMIC_RELAXED, SCOPE);
}

// ---- Swendsen-Wang: the slice table of the improved correlator ---------------------------------------------------
// Per chain and direction an open-addressing table of 2^lg >= 2 N slots of 16 B: the key word ((root << 32) | (slice + 1); 0 =
// empty) and the value word, P_C,d(slice) = the sum of q(a) over the vertices of cluster `root` in that slice.  Linear probing
// from a multiplicative hash.  At most N keys of a direction exist, so the load stays <= 1/2 and an empty slot ends every probe;
// all the same every probe loop carries the capacity as its cap and reports a cap that is hit.  Nothing is ever removed from a
// table between its clear and its last reader, so a key, once stored, stays where it is.
__device__ __forceinline__ unsigned long long sw_slice_key(uint32_t root, uint32_t slice) {
  return ((unsigned long long)root << 32) | (unsigned long long)(slice + 1u);
}

__device__ __forceinline__ uint32_t sw_slice_hash(unsigned long long key, uint32_t lg) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - lg));
}

// v added onto the value of `key`, which is inserted first where it is missing: a 64-bit compare-and-swap on the key word
// claims an empty slot, the lane whose swap wins adds 1 to the occupied-slice count of its root.  A lane that loses a swap
// looks at what the winner stored and goes on; it never waits for a store.
__device__ __forceinline__ void sw_slice_add(unsigned long long *table, uint32_t lg, uint32_t *count, uint32_t root, uint32_t slice,
                                             long long v, bool &capped) {
  const unsigned long long key = sw_slice_key(root, slice);
  const uint32_t cap = 1u << lg;
  uint32_t slot = sw_slice_hash(key, lg);
  for (uint32_t it = 0; it < cap; ++it) {
    unsigned long long *kw = table + 2 * (size_t)slot;
    unsigned long long seen = __hip_atomic_load(kw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool created = false;
    if (seen == 0ull) {
      created = __hip_atomic_compare_exchange_strong(kw, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (created) seen = key;                             // else `seen` holds what the winner stored
    }
    if (seen == key) {
      __hip_atomic_fetch_add((long long *)(kw + 1), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (created) __hip_atomic_fetch_add(count + root, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    slot = (slot + 1u) & (cap - 1u);
  }
  capped = true;
}

// the value of (root, slice) in a table nobody writes any more; 0 where the key is absent
__device__ __forceinline__ long long sw_slice_lookup(const unsigned long long *table, uint32_t lg, uint32_t root, uint32_t slice,
                                                     bool &capped) {
  const unsigned long long key = sw_slice_key(root, slice);
  const uint32_t cap = 1u << lg;
  uint32_t slot = sw_slice_hash(key, lg);
  for (uint32_t it = 0; it < cap; ++it) {
    const unsigned long long seen = table[2 * (size_t)slot];
    if (seen == key) return (long long)table[2 * (size_t)slot + 1];
    if (seen == 0ull) return 0;
    slot = (slot + 1u) & (cap - 1u);
  }
  capped = true;
  return 0;
}

// v of every active lane added onto (root, slice), the lanes of a wave that share the key combined first as sw_add_combined
// combines them (in direction x whole runs of lanes share one).  Every lane of the wave calls it: the combining rounds take
// their trip count from ballots, the shuffles run with all lanes; the probe loop that follows has no ballot in it.
__device__ __forceinline__ void sw_slice_add_combined(unsigned long long *table, uint32_t lg, uint32_t *count, uint32_t root, uint32_t slice,
                                                      bool active, long long v, bool &capped) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  unsigned long long todo = __ballot(active);
  bool mine = active;
  for (uint32_t round = 0; round < kSwCombineRounds && todo; ++round) {
    const int lead = __builtin_ctzll(todo);
    const bool same = ((todo >> lane) & 1ull) && root == (uint32_t)__shfl((int)root, lead) && slice == (uint32_t)__shfl((int)slice, lead);
    const unsigned long long m = __ballot(same);
    todo &= ~m;
    if ((uint32_t)__builtin_popcountll(m) < kSwCombineMin) continue;   // too few: each of them adds its own
    long long s = same ? v : 0;
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (same) {
      mine = lane == (uint32_t)lead;
      v = s;
    }
  }
  if (mine) sw_slice_add(table, lg, count, root, slice, v, capped);
}

// ---- Wolff: the improved estimators of the single-cluster update ---------------------------------------------
// What the improved instances of the Wolff kernels carry beside the plain draw's arguments.  Per chain, in the workspace: the
// slice table P_d(i) = the sum of q(a) over the members in slice i of direction d, [M_0 + M_1] int64, t slices first; the list
// of the occupied slices of either direction, [M_0 + M_1] uint32; the accumulators, [kWolffSums + n_out] int64: A, Ac_0, As_0,
// Ac_1, As_1, then one per (d, tau) in the layout of mlmcpi_sigma_level_correlator; the weights (w^s, w^c) of every slice,
// [M_0 + M_1][2] double.  The kernel zeroes table and accumulators and forms the weights when it starts (sw_phase inside the
// update loop costs the registers of its expansion across the whole loop, as in sigma_sw.hip), and every update leaves table
// and accumulators zero.  structure and corr may be NULL.
constexpr uint32_t kWolffSums = 5;

struct WolffImproved {
  long long *table, *acc;
  uint32_t *occupied;
  double *weights;
  double *improved, *structure, *corr;
  uint32_t M0, M1;
  double scale, inv_scale;   // 2^(s - 64) and 2^-s, s the fixed-point scale of the lag accumulators (sigma_sw.hip: sw_corr)
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

// one atomic per wave: the lanes of the wave that flipped a vertex (every lane of the wave calls it)
__device__ __forceinline__ void sw_count_flips(bool flip, uint32_t *flipped_b) {
  const unsigned long long m = __ballot(flip);
  if (flipped_b && m && (threadIdx.x & (kWave - 1)) == (uint32_t)__builtin_ctzll(m)) atomicAdd(flipped_b, (uint32_t)__builtin_popcountll(m));
}

}  // namespace mlmcpi
