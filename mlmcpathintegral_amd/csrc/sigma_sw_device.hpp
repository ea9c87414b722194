// sigma_sw_device.hpp -- what the kernels of the Swendsen-Wang update share (sigma_sw_tiled.hip, sigma_sw_chain.hip,
// sigma_sw_correlator.hip) and nobody else reads: the chain plan's constants, the lock-free union-find, the coin, the
// fixed-order reduction of the improved estimator, the combined adds, the slice table of the improved correlator and the two
// options of the chain kernel.  On sigma_cluster_device.hpp, which has the embedding and the geometries.
#pragma once
#include "sigma_cluster_device.hpp"

namespace mlmcpi {

// SW chain plan: a (8 B), the root's sum (8 B) and the parent (4 B) of every vertex in LDS beside the 12 KiB of sw_finish
constexpr uint32_t kSwChainBytesPerVertex = 20;
constexpr uint32_t kSwChainMaxN = (160 * 1024 - 12 * 1024 - 512) / kSwChainBytesPerVertex;  // 7552 vertices
constexpr int kUfPlain = -1;                     // uf_find: plain loads (nobody writes the parents any more)

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

// ---- the coin and the reductions ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sw_coin(const RngKey &key, uint32_t root) {
  double u, unused;
  rng_uniforms(key, root, P_SIGMA_SW_FLIP, 0, u, unused);
  return u < 0.5;
}

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

// one atomic per wave: the lanes of the wave that flipped a vertex (every lane of the wave calls it)
__device__ __forceinline__ void sw_count_flips(bool flip, uint32_t *flipped_b) {
  const unsigned long long m = __ballot(flip);
  if (flipped_b && m && (threadIdx.x & (kWave - 1)) == (uint32_t)__builtin_ctzll(m)) atomicAdd(flipped_b, (uint32_t)__builtin_popcountll(m));
}

// ---- the structure sums (improved structure factor at the lowest momentum) -----------------------------------
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

// ---- the slice table of the improved correlator -------------------------------------------------------------
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

}  // namespace mlmcpi
