// sigma_level_sw.hip -- the Swendsen-Wang multi-cluster update of the O(3) nonlinear sigma model on the levels of its
// CoarsenRotate hierarchy (include/mlmcpi_hip.h: mlmcpi_sigma_level_sw_*).  An unrotated level is the lattice of
// sigma_sw.hip and delegates to mlmcpi_sigma_sw_*; this file adds the ROTATED level (geometry: sigma_level_device.hpp), where
// the coarse sampler of a two-level or hierarchical run with two levels lives.  The helpers of sigma_sw.hip are restated here
// (slsw_*): that unit is untouched.
//
// The update, restated (tests/sigma_level_sw_model.py).  The level has n = Mt Mx / 2 vertices, plane E then plane O of ht x hx =
// Mt/2 x Mx/2 each, index p ht hx + ht b + a.  It is bipartite: every link has exactly one E end, so the 2 n links are named
// (e, d) with e an E vertex (e < n / 2) and d its direction in the reference's order: E(a, b) -> O(a, b), O(a, b-1), O(a-1, b),
// O(a-1, b-1) -- the naming of sigma_level_cluster.hip.  Where a plane extent is 1 several of the four neighbours of a vertex
// are one vertex; those are distinct links with a uniform each.  With r the reflection normal and a_l = r . sigma_l of the field
// BEFORE the update, a link (x, y) is bonded iff a_x a_y > 0 and its uniform < 1 - exp(min(0, -2 beta (a_x a_y))) (the product
// first).  One update tests ALL 2 n links once, labels EVERY connected component of the graph of bonded links and reflects
// each component with probability 1/2: the root of a cluster is its smallest LEVEL index (also when the cluster is a lone O
// vertex), the cluster is reflected iff the root's coin says so, sigma' = sigma - 2 a r, stored in the canonical form.  Every
// decision is a function of (link or root, chain, update counter, field before the update): the state does not depend on the
// launch plan, the tile, the batch split or chain0.
//
// RNG contract, step = global update counter update0 + k, the purposes of sigma_sw.hip with the level's indices:
//   P_SIGMA_SW_REFLECT  site 0, sub 0: (u, v) -> r_z = 1 - 2 u, azimuth 2 pi v - pi
//   P_SIGMA_SW_BOND     site e, sub d >> 1: u decides link (e, d) for d even, v for d odd
//   P_SIGMA_SW_FLIP     site root, sub 0: reflected iff u < 0.5
//
// Improved estimator: 3 sum_C A_C^2 / n, A_C the sum of q(a) = llrint(a 2^32) over the cluster by integer atomic adds on the
// root's slot, the squares summed over the roots in the fixed configuration of slsw_finish (1024 threads, thread t takes the
// vertices t, t + 1024, .., then a fixed tree) and ADDED to the caller's accumulator update by update: 10 updates = 5 + 5.
//
// Labelling: the parent array and the union by atomic min of sigma_sw.hip.  The parent of a vertex is a vertex of its cluster
// with a smaller or equal index; union(x, y) finds both roots and hangs the larger under the smaller with an atomic min on the
// larger root's parent word; if the word held something else meanwhile it goes on with (what it held, the smaller root).
// max(x, y) decreases with every retry and a path visits decreasing indices: the number of vertices bounds every loop, every
// loop carries that cap, a cap that is hit sets a status word the entry point returns as an error.  No loop waits on another
// lane's store.  union(x, x) returns at once (level (2, 2): the four links of E(0, 0) all end at O(0, 0)).
#include <mutex>

#include "internal.hpp"

#include "sigma_device.hpp"  // fp contraction is off from here on
#include "sigma_level_device.hpp"

namespace mlmcpi {

constexpr uint32_t kSlswThreads = 256;         // tiled plan: bond + label, merge, resolve
constexpr uint32_t kSlswFinishThreads = 1024;  // the fixed configuration of slsw_finish; the chain plan's workgroup
// chain plan: a (8 B), the root's sum (8 B) and the parent (4 B) of every vertex in LDS beside the 12 KiB of slsw_finish
constexpr uint32_t kSlswChainBytesPerVertex = 20;
constexpr uint32_t kSlswChainMaxN = (160 * 1024 - 12 * 1024 - 512) / kSlswChainBytesPerVertex;  // 7552 vertices
constexpr uint32_t kSlswMaxTile = 64;          // the largest tile extent MLMCPI_SIGMA_SW_TILE admits, in cells
constexpr double kSlswFix = 4294967296.0;      // 2^32
constexpr int kSlswPlain = -1;                 // slsw_find: plain loads (nobody writes the parents any more)

// tiled plan, launch 1: a of the tile's E cells [W H], a of its O cells and their -a / -b halo [(W + 1)(H + 1)], the parents
// [2 W H] uint32, the bond bits [W H] uint8
__host__ __device__ constexpr size_t slsw_tile_lds(uint32_t W, uint32_t H) {
  return ((size_t)W * H + (size_t)(W + 1) * (H + 1)) * sizeof(double) + (size_t)2 * W * H * sizeof(uint32_t) + (size_t)W * H;
}

__device__ __forceinline__ double slsw_dot(const V3 &r, const V3 &s) { return (r.x * s.x + r.y * s.y) + r.z * s.z; }

__device__ __forceinline__ V3 slsw_normal(const RngKey &key) {
  double u, v;
  rng_uniforms(key, 0, P_SIGMA_SW_REFLECT, 0, u, v);
  const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
  double sa, ca;
  sincos(kTwoPi * v - kPi, &sa, &ca);
  return V3{rho * ca, rho * sa, rz};
}

__device__ __forceinline__ bool slsw_bonded(double ax, double ay, double beta2, double uni) {
  const double prod = ax * ay;
  if (!(prod > 0.0)) return false;                       // p = 0: never bonded
  return uni < 1.0 - exp(fmin(0.0, -(beta2 * prod)));
}

// the bonds of the links (e, 0) .. (e, 3) as bits 0 .. 3; ao[d] = a of the O end of link (e, d).  Two Philox calls.
__device__ __forceinline__ uint32_t slsw_bonds(const RngKey &key, uint32_t e, double a, const double (&ao)[4], double beta2) {
  const U4 w0 = philox4x32_10(e, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
  const U4 w1 = philox4x32_10(e, key.chain, key.step, ((uint32_t)P_SIGMA_SW_BOND << 24) | 1u, key.k0, key.k1);
  return (slsw_bonded(a, ao[0], beta2, u01(w0.x, w0.y)) ? 1u : 0u) | (slsw_bonded(a, ao[1], beta2, u01(w0.z, w0.w)) ? 2u : 0u) |
         (slsw_bonded(a, ao[2], beta2, u01(w1.x, w1.y)) ? 4u : 0u) | (slsw_bonded(a, ao[3], beta2, u01(w1.z, w1.w)) ? 8u : 0u);
}

__device__ __forceinline__ bool slsw_coin(const RngKey &key, uint32_t root) {
  double u, unused;
  rng_uniforms(key, root, P_SIGMA_SW_FLIP, 0, u, unused);
  return u < 0.5;
}

__device__ __forceinline__ double2 slsw_reflected(const V3 &s, double a, const V3 &r) {
  const double c = 2.0 * a;
  return angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
}

__device__ __forceinline__ long long slsw_fixed(double a) { return llrint(a * kSlswFix); }

template <int SCOPE>
__device__ __forceinline__ uint32_t slsw_parent(const uint32_t *parent, uint32_t x) {
  // other lanes (tiled plan: workgroups on other XCDs) lower parent words meanwhile: an atomic load of that scope, not a plain one
  if constexpr (SCOPE == kSlswPlain) return parent[x];
  else return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
}

// the root above x; a path visits strictly decreasing indices, so `cap` >= the number of vertices bounds it
template <int SCOPE>
__device__ __forceinline__ uint32_t slsw_find(const uint32_t *parent, uint32_t x, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {
    const uint32_t p = slsw_parent<SCOPE>(parent, x);
    if (p == x) return x;
    x = p;
  }
  capped = true;
  return x;
}

template <int SCOPE>
__device__ __forceinline__ void slsw_union(uint32_t *parent, uint32_t x, uint32_t y, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {                // max(x, y) decreases with every retry
    x = slsw_find<SCOPE>(parent, x, cap, capped);
    y = slsw_find<SCOPE>(parent, y, cap, capped);
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

// sum over the roots of (A_C 2^-32)^2 and their number, in the fixed configuration (kSlswFinishThreads threads, every thread
// of the workgroup calls it); thread 0 adds 3 / n x the sum to *improved and the number to *clusters (either may be NULL)
__device__ __forceinline__ void slsw_finish(const uint32_t *parent, const long long *sum, uint32_t n, double *red, uint32_t *redc,
                                            double *improved, uint32_t *clusters) {
  const uint32_t t = threadIdx.x;
  double s = 0.0;
  uint32_t c = 0;
  for (uint32_t l = t; l < n; l += kSlswFinishThreads)
    if (parent[l] == l) {
      const double A = (double)sum[l] * (1.0 / kSlswFix);
      s += A * A;
      ++c;
    }
  red[t] = s;
  redc[t] = c;
  __syncthreads();
  for (uint32_t off = kSlswFinishThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
      red[t] += red[t + off];
      redc[t] += redc[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    if (improved) *improved += red[0] * (3.0 / (double)n);
    if (clusters) *clusters += redc[0];
  }
}

// one atomic per wave: the lanes of the wave that flipped a vertex (every lane of the wave calls it)
__device__ __forceinline__ void slsw_count_flips(bool flip, uint32_t *flipped_b) {
  const unsigned long long m = __ballot(flip);
  if (flipped_b && m && (threadIdx.x & (kWave - 1)) == (uint32_t)__builtin_ctzll(m)) atomicAdd(flipped_b, (uint32_t)__builtin_popcountll(m));
}

// ---- tiled plan, launch 1: bonds of the tile's E vertices, union-find on the tile's interior links in LDS ----------------
// A workgroup takes a tile of W x H plane CELLS of one chain: cell (a, b) is the pair E(a, b), O(a, b) (w x h cells where the
// plane ends: masked, not padded).  The links (e, d) of E(a, b) end at O(a - (d >> 1), b - (d & 1)), so the tile needs a of its
// own cells and of the O vertices one column to the -a side and one row to the -b side: the O image is (w + 1) x (h + 1) with
// its row 0 and column 0 the halo.  A link is INTERIOR to the tile iff its O end is a cell of the tile without a periodic wrap:
// li >= (d >> 1) and lj >= (d & 1) in tile coordinates; every other link is a crossing link of launch 2 (also the wrap of a
// plane that one tile covers).
// Local order of the union-find: E cell (li, lj) -> W lj + li, O cell (li, lj) -> W H + W lj + li.  Inside a plane the level
// index is ht b + a, which orders the cells of a tile by (b, a) exactly as W lj + li orders them by (lj, li); and every E vertex
// of the level (index < n / 2) precedes every O vertex, as every local E index (< W H) precedes every local O index.  So the
// local order is the order of the level index restricted to the tile, and a local root -- the smallest local index of its
// component -- is the smallest level index of it.
__global__ void __launch_bounds__(kSlswThreads)
    sigma_rot_sw_bond_label_kernel(const double2 *phi_all, SigmaLevel L, double beta2, RngKey key0, uint32_t W, uint32_t H,
                                   uint32_t ntx, uint32_t nty, uint32_t *label_all, uint8_t *bits_all, long long *qa_all,
                                   long long *sum_all, uint32_t *status) {
  extern __shared__ double slsw_lds[];
  const uint32_t SA = W + 1, WH = W * H;
  double *aE = slsw_lds;
  double *aO = aE + WH;
  uint32_t *parent = (uint32_t *)(aO + (size_t)SA * (H + 1));
  uint8_t *lbits = (uint8_t *)(parent + 2 * WH);
  const uint32_t tiles = ntx * nty, b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const uint32_t a0 = (tile % ntx) * W, b0 = (tile / ntx) * H;
  const uint32_t ht = L.ht, hx = L.hx, q = L.q, n = 2 * q;
  const uint32_t w = ht - a0 < W ? ht - a0 : W, h = hx - b0 < H ? hx - b0 : H;
  const double2 *phi = phi_all + (size_t)b * n;
  RngKey key = key0;
  key.chain = key0.chain + b;
  const V3 r = slsw_normal(key);

  for (uint32_t p = threadIdx.x; p < (w + 1) * (h + 1); p += kSlswThreads) {
    const uint32_t li = p % (w + 1), lj = p / (w + 1);   // O image: (0, .) and (., 0) are the halo, (li, lj) is cell (li - 1, lj - 1)
    const uint32_t oa = a0 + li == 0 ? ht - 1 : a0 + li - 1, ob = b0 + lj == 0 ? hx - 1 : b0 + lj - 1;
    const uint32_t lo = q + ob * ht + oa;
    const double ao = slsw_dot(r, sigma_of(phi[lo]));
    aO[lj * SA + li] = ao;
    if (li > 0 && lj > 0) {                              // a cell of the tile: its O vertex and its E vertex
      const uint32_t le = lo - q;
      const double ae = slsw_dot(r, sigma_of(phi[le]));
      aE[(lj - 1) * W + li - 1] = ae;
      qa_all[(size_t)b * n + lo] = slsw_fixed(ao);
      qa_all[(size_t)b * n + le] = slsw_fixed(ae);
      if (sum_all) {
        sum_all[(size_t)b * n + lo] = 0;
        sum_all[(size_t)b * n + le] = 0;
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kSlswThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, e = (b0 + lj) * ht + a0 + li;
    const double ao[4] = {aO[(lj + 1) * SA + li + 1], aO[lj * SA + li + 1], aO[(lj + 1) * SA + li], aO[lj * SA + li]};
    const uint32_t bits = slsw_bonds(key, e, aE[loc], ao, beta2);
    bits_all[(size_t)b * q + e] = (uint8_t)bits;
    lbits[loc] = (uint8_t)bits;
    parent[loc] = loc;
    parent[WH + loc] = WH + loc;
  }
  __syncthreads();
  bool capped = false;
  for (uint32_t p = threadIdx.x; p < w * h; p += kSlswThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, bits = lbits[loc];
    if (bits & 1u) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc, 2 * WH, capped);
    if ((bits & 2u) && lj > 0) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - W, 2 * WH, capped);
    if ((bits & 4u) && li > 0) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - 1, 2 * WH, capped);
    if ((bits & 8u) && li > 0 && lj > 0) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - W - 1, 2 * WH, capped);
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < 2 * w * h; p += kSlswThreads) {
    const uint32_t plane = p >= w * h ? 1u : 0u, c = p - plane * w * h, li = c % w, lj = c / w;
    const uint32_t root = slsw_find<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, plane * WH + lj * W + li, 2 * WH, capped);
    const uint32_t rplane = root >= WH ? 1u : 0u, rc = root - rplane * WH;
    label_all[(size_t)b * n + plane * q + (b0 + lj) * ht + a0 + li] = rplane * q + (b0 + rc / W) * ht + a0 + rc % W;
  }
  if (capped) atomicOr(status, 1u);
}

// ---- launch 2: one lane per link that leaves its tile -------------------------------------------------------------------
// Per chain: 2 ntx hx lanes for the links d = 2, 3 of the E vertices in the first column of every tile column (their O end is
// one column to the -a side: another tile, or the wrap), then 2 nty ht lanes for the links d = 1, 3 of the E vertices in the
// first row of every tile row.  The d = 3 link of a tile's corner cell is in both sets: the lane of the second set returns, so
// it is crossed once.
__global__ void __launch_bounds__(kSlswThreads)
    sigma_rot_sw_merge_kernel(SigmaLevel L, uint32_t W, uint32_t H, uint32_t ntx, uint32_t nty, uint32_t blocks, uint32_t *label_all,
                              const uint8_t *bits_all, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, x = (blockIdx.x % blocks) * kSlswThreads + threadIdx.x;
  const uint32_t ht = L.ht, hx = L.hx, q = L.q, n = 2 * q, E0 = 2 * ntx * hx, E1 = 2 * nty * ht;
  if (x >= E0 + E1) return;
  uint32_t ca, cb, d;
  if (x < E0) {
    d = 2u + (x & 1u);
    ca = ((x >> 1) % ntx) * W;
    cb = (x >> 1) / ntx;
  } else {
    const uint32_t y = x - E0;
    d = 1u + ((y & 1u) << 1);
    ca = (y >> 1) % ht;
    cb = ((y >> 1) / ht) * H;
    if (d == 3u && ca % W == 0) return;                  // the corner cell's d = 3 link: the first set has it
  }
  const uint32_t e = cb * ht + ca;
  if (!(bits_all[(size_t)b * q + e] & (1u << d))) return;
  const uint32_t oa = (d & 2u) ? (ca == 0 ? ht - 1 : ca - 1) : ca, ob = (d & 1u) ? (cb == 0 ? hx - 1 : cb - 1) : cb;
  bool capped = false;
  slsw_union<__HIP_MEMORY_SCOPE_AGENT>(label_all + (size_t)b * n, e, q + ob * ht + oa, n, capped);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 3: every vertex follows its label to the final root, adds q(a) to the root's slot, evaluates the root's coin ----
// and, when the coin says so, stores its reflection (non-temporal; nothing is stored otherwise)
__global__ void __launch_bounds__(kSlswThreads)
    sigma_rot_sw_resolve_kernel(double2 *phi_all, uint32_t n, RngKey key0, uint32_t blocks, const uint32_t *label_all,
                                const long long *qa_all, long long *sum_all, uint32_t *flipped, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kSlswThreads + threadIdx.x;
  RngKey key = key0;
  key.chain = key0.chain + b;
  bool flip = false, capped = false;
  if (l < n) {
    const uint32_t root = slsw_find<kSlswPlain>(label_all + (size_t)b * n, l, n, capped);
    if (sum_all) atomicAdd((unsigned long long *)(sum_all + (size_t)b * n + root), (unsigned long long)qa_all[(size_t)b * n + l]);
    flip = !capped && slsw_coin(key, root);
    if (flip) {
      const V3 r = slsw_normal(key);
      double2 *p = phi_all + (size_t)b * n + l;
      const V3 s = sigma_of(*p);
      const double2 out = slsw_reflected(s, slsw_dot(r, s), r);
      __builtin_nontemporal_store(out.x, &p->x);
      __builtin_nontemporal_store(out.y, &p->y);
    }
  }
  slsw_count_flips(flip, flipped ? flipped + b : nullptr);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 4 (only when outputs are asked for): one workgroup per chain -------------------------------------------------
__global__ void __launch_bounds__(kSlswFinishThreads)
    sigma_rot_sw_finish_kernel(const uint32_t *label_all, const long long *sum_all, uint32_t n, double *improved, uint32_t *clusters) {
  __shared__ double red[kSlswFinishThreads];
  __shared__ uint32_t redc[kSlswFinishThreads];
  const uint32_t b = blockIdx.x;
  slsw_finish(label_all + (size_t)b * n, sum_all + (size_t)b * n, n, red, redc, improved ? improved + b : nullptr,
              clusters ? clusters + b : nullptr);
}

// ---- chain plan: one workgroup per chain, all n_updates updates in one launch, labels, sums and a in LDS -----------------
// Thread t owns the vertices t, t + 1024, ..: it alone reads and writes their angles, update after update.  Bonds are drawn
// and united from the E end: a lane with an E vertex makes two Philox calls and handles its four links, a lane with an O vertex
// makes none.
__global__ void __launch_bounds__(kSlswFinishThreads)
    sigma_rot_sw_chain_kernel(double2 *phi_all, SigmaLevel L, double beta2, uint32_t n_updates, RngKey key0, uint32_t *flipped,
                              uint32_t *clusters, double *improved, uint32_t *status) {
  extern __shared__ double slsw_lds[];
  __shared__ double red[kSlswFinishThreads];
  __shared__ uint32_t redc[kSlswFinishThreads];
  const uint32_t ht = L.ht, hx = L.hx, q = L.q, n = 2 * q, b = blockIdx.x, t = threadIdx.x;
  double *a = slsw_lds;
  long long *sum = (long long *)(a + n);
  uint32_t *parent = (uint32_t *)(sum + n);
  double2 *phi = phi_all + (size_t)b * n;
  const bool outputs = clusters || improved;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t nflip = 0;
  bool capped = false;
  for (uint32_t k = 0; k < n_updates; ++k, ++key.step) {
    const V3 r = slsw_normal(key);
    for (uint32_t l = t; l < n; l += kSlswFinishThreads) {
      a[l] = slsw_dot(r, sigma_of(phi[l]));
      sum[l] = 0;
      parent[l] = l;
    }
    __syncthreads();
    for (uint32_t e = t; e < q; e += kSlswFinishThreads) {
      const uint32_t cb = e / ht, ca = e - cb * ht;
      const uint32_t am = ca == 0 ? ht - 1 : ca - 1, bm = cb == 0 ? hx - 1 : cb - 1;
      const uint32_t y[4] = {q + cb * ht + ca, q + bm * ht + ca, q + cb * ht + am, q + bm * ht + am};
      const double ao[4] = {a[y[0]], a[y[1]], a[y[2]], a[y[3]]};
      const uint32_t bits = slsw_bonds(key, e, a[e], ao, beta2);
      if (bits & 1u) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, e, y[0], n, capped);
      if (bits & 2u) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, e, y[1], n, capped);
      if (bits & 4u) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, e, y[2], n, capped);
      if (bits & 8u) slsw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, e, y[3], n, capped);
    }
    __syncthreads();
    for (uint32_t l = t; l < n; l += kSlswFinishThreads) {
      const uint32_t root = slsw_find<kSlswPlain>(parent, l, n, capped);
      if (improved) atomicAdd((unsigned long long *)(sum + root), (unsigned long long)slsw_fixed(a[l]));
      if (!capped && slsw_coin(key, root)) {
        phi[l] = slsw_reflected(sigma_of(phi[l]), a[l], r);
        ++nflip;
      }
    }
    __syncthreads();
    if (outputs) slsw_finish(parent, sum, n, red, redc, improved ? improved + b : nullptr, clusters ? clusters + b : nullptr);
    __syncthreads();
  }
  if (flipped) {
    for (int off = kWave / 2; off > 0; off >>= 1) nflip += __shfl_down(nflip, off);
    if ((t & (kWave - 1)) == 0 && nflip) atomicAdd(flipped + b, nflip);
  }
  if (capped) atomicOr(status, 1u);
}

namespace {

struct SlswPlan {
  bool ok, chain;
  uint32_t W, H, ntx, nty;                // tiled: tile extents in cells, tiles per direction
  uint32_t merge_blocks, resolve_blocks;  // tiled: workgroups per chain of launches 2 and 3
  size_t lds_bytes;                       // dynamic LDS of the chain kernel / of launch 1
};

// Launch plan: sw_plan's rule with N replaced by n; it chooses and calls nothing.  The chain plan where a
// chain fits its LDS bound and one workgroup per chain fills the device (B >= kComputeUnits), the tiled plan otherwise.  The
// knobs MLMCPI_SIGMA_SW_PLAN=chain|tiled and MLMCPI_SIGMA_SW_TILE=WxH (here in cells) govern this unit too; ok = false: the
// chain plan was forced on a level beyond its bound.
// Default tile 32 x 32 cells, by LDS arithmetic and not by a timing sweep: a tile of W x H cells takes 25 W H + 8 (W + H + 1) B
// (slsw_tile_lds), so 32 x 32 takes 26 120 B = 25.5 KiB and six workgroups of four waves share the 160 KiB of a CU (24 of its
// 32 wave slots); it holds 2048 vertices, as the 64 x 32 vertex tile of the unrotated default does, the halo is 65 / 1024 = 6 %
// of the cells read, and among the tiles of that area the square one has the fewest crossing links (2 W + 2 H - 1 = 127 of
// 4096).  64 x 64 cells take 101 KiB: one workgroup per CU, and the attribute of slsw_init_attrs.
SlswPlan slsw_plan(const SigmaLevel &L, uint32_t B, const Tuning &tune) {
  SlswPlan p{};
  const uint32_t n = L.nvert();
  p.chain = tune.sigma_sw_plan ? tune.sigma_sw_plan == 1 : (n <= kSlswChainMaxN && B >= kComputeUnits);
  p.ok = !p.chain || n <= kSlswChainMaxN;
  p.W = tune.sigma_sw_tile_w ? tune.sigma_sw_tile_w : 32;
  p.H = tune.sigma_sw_tile_h ? tune.sigma_sw_tile_h : 32;
  p.ntx = (L.ht + p.W - 1) / p.W;
  p.nty = (L.hx + p.H - 1) / p.H;
  p.merge_blocks = (2 * p.ntx * L.hx + 2 * p.nty * L.ht + kSlswThreads - 1) / kSlswThreads;
  p.resolve_blocks = (n + kSlswThreads - 1) / kSlswThreads;
  p.lds_bytes = p.chain ? (size_t)n * kSlswChainBytesPerVertex : slsw_tile_lds(p.W, p.H);
  return p;
}

std::mutex g_slsw_attr_mutex;
bool g_slsw_attr_set[64] = {false};

// dynamic LDS above 64 KiB: the chain kernel up to its bound, launch 1 at the largest tile
int slsw_init_attrs() {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(MLMCPI_ERR_INVALID, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_slsw_attr_mutex);
  if (g_slsw_attr_set[dev]) return MLMCPI_OK;
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sw_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSlswChainMaxN * kSlswChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sw_bond_label_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)slsw_tile_lds(kSlswMaxTile, kSlswMaxTile)));
  g_slsw_attr_set[dev] = true;
  return MLMCPI_OK;
}

int slsw_check(const mlmcpi_sigma_level *level) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(level->beta > 0.0, "beta must be positive");
  return MLMCPI_OK;
}

mlmcpi_lattice_action slsw_as_lattice(const mlmcpi_sigma_level *l) {
  return mlmcpi_lattice_action{MLMCPI_NONLINEAR_SIGMA, l->Mt, l->Mx, l->beta, 0.0};
}

// workspace sections, the layout of sigma_sw.hip: status word (256 B), label [B n] uint32, q(a) [B n] int64, cluster sums [B n]
// int64, bond bits [B n / 2] uint8 (four bits per E vertex)
constexpr size_t kSlswStatusBytes = 256;
size_t slsw_section_label(uint32_t n, uint32_t B) { return align256((size_t)B * n * sizeof(uint32_t)); }
size_t slsw_section_fixed(uint32_t n, uint32_t B) { return align256((size_t)B * n * sizeof(long long)); }
size_t slsw_section_bits(uint32_t n, uint32_t B) { return align256((size_t)B * (n / 2)); }

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_sw_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = slsw_check(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = slsw_as_lattice(level);
    return mlmcpi_sigma_sw_workspace_bytes(&act, B, bytes);
  }
  const uint32_t n = make_level(*level).nvert();
  *bytes = kSlswStatusBytes + slsw_section_label(n, B) + 2 * slsw_section_fixed(n, B) + slsw_section_bits(n, B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_sw_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                               uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                               void *d_work, void *stream) {
  if (int rc = slsw_check(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = slsw_as_lattice(level);
    return mlmcpi_sigma_sw_draw(&act, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, d_work, stream);
  }
  const SigmaLevel L = make_level(*level);
  const uint32_t n = L.nvert();
  const SlswPlan p = slsw_plan(L, B, tuning());
  if (!p.ok)
    return fail(MLMCPI_ERR_UNSUPPORTED, "mlmcpi_sigma_level_sw_draw: MLMCPI_SIGMA_SW_PLAN=chain holds a chain of at most %u vertices in "
                "LDS, this level has %u", kSlswChainMaxN, n);
  const uint64_t widest = (uint64_t)B * (p.ntx * p.nty > p.resolve_blocks ? p.ntx * p.nty : p.resolve_blocks);
  MLMCPI_REQUIRE(p.chain || (widest < (1ull << 31) && (uint64_t)B * p.merge_blocks < (1ull << 31)), "too many workgroups for one launch: split the batch");
  if (n_updates == 0) return MLMCPI_OK;
  if (int rc = slsw_init_attrs()) return rc;
  char *w = (char *)d_work;
  uint32_t *status = (uint32_t *)w;
  uint32_t *label = (uint32_t *)(w + kSlswStatusBytes);
  long long *qa = (long long *)(w + kSlswStatusBytes + slsw_section_label(n, B));
  long long *sum = (long long *)(w + kSlswStatusBytes + slsw_section_label(n, B) + slsw_section_fixed(n, B));
  uint8_t *bits = (uint8_t *)(w + kSlswStatusBytes + slsw_section_label(n, B) + 2 * slsw_section_fixed(n, B));
  const hipStream_t st = as_stream(stream);
  const double beta2 = 2.0 * level->beta;
  MLMCPI_HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
  if (p.chain) {
    hipLaunchKernelGGL(sigma_rot_sw_chain_kernel, dim3(B), dim3(kSlswFinishThreads), p.lds_bytes, st, (double2 *)d_state, L, beta2,
                       n_updates, make_key(seed, chain0, update0), d_flipped, d_clusters, d_improved, status);
    MLMCPI_LAUNCH_CHECK("sigma_rot_sw_chain_kernel");
  } else {
    const bool outputs = d_clusters || d_improved;
    for (uint32_t k = 0; k < n_updates; ++k) {
      const RngKey key = make_key(seed, chain0, update0 + k);
      hipLaunchKernelGGL(sigma_rot_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kSlswThreads), p.lds_bytes, st,
                         (const double2 *)d_state, L, beta2, key, p.W, p.H, p.ntx, p.nty, label, bits, qa, d_improved ? sum : nullptr, status);
      MLMCPI_LAUNCH_CHECK("sigma_rot_sw_bond_label_kernel");
      hipLaunchKernelGGL(sigma_rot_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kSlswThreads), 0, st, L, p.W, p.H, p.ntx, p.nty,
                         p.merge_blocks, label, bits, status);
      MLMCPI_LAUNCH_CHECK("sigma_rot_sw_merge_kernel");
      hipLaunchKernelGGL(sigma_rot_sw_resolve_kernel, dim3(B * p.resolve_blocks), dim3(kSlswThreads), 0, st, (double2 *)d_state, n, key,
                         p.resolve_blocks, label, qa, d_improved ? sum : nullptr, d_flipped, status);
      MLMCPI_LAUNCH_CHECK("sigma_rot_sw_resolve_kernel");
      if (outputs) {
        hipLaunchKernelGGL(sigma_rot_sw_finish_kernel, dim3(B), dim3(kSlswFinishThreads), 0, st, label, sum, n, d_improved, d_clusters);
        MLMCPI_LAUNCH_CHECK("sigma_rot_sw_finish_kernel");
      }
    }
  }
  // a find or union loop that ran into its cap (it cannot, by the argument above): an error, never a hang
  uint32_t h_status = 0;
  MLMCPI_HIP_TRY(hipMemcpyAsync(&h_status, status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MLMCPI_HIP_TRY(hipStreamSynchronize(st));
  if (h_status) return fail(MLMCPI_ERR_HIP, "mlmcpi_sigma_level_sw_draw: a labelling loop reached its iteration cap (status %u); the state is undefined", h_status);
  return MLMCPI_OK;
}

}  // extern "C"
