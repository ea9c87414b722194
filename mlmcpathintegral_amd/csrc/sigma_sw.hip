// sigma_sw.hip -- the Swendsen-Wang multi-cluster update of the O(3) nonlinear sigma model (gfx950, wave64).
//
// The multi-cluster form of the embedding sigma_cluster.hip grows one cluster of: one update tests ALL 2 N links once, labels
// EVERY connected component of the graph of bonded links and reflects each component with probability 1/2.  The reference has
// no such sampler; like the Wolff update it is the project's own (tests/sigma_sw_model.py).
//
// The update, restated.  Vertex l = Mt j + i; link (l, 0) joins l to its +i neighbour, link (l, 1) to its +j neighbour
// (periodic, 2 N links; on an extent of 2 the two links between a pair are two links with a uniform each).  With r the
// reflection normal and a_l = r . sigma_l of the field BEFORE the update, a link (x, y) is bonded iff a_x a_y > 0 and its
// uniform < 1 - exp(min(0, -2 beta (a_x a_y))) (the product first: the same bits from either end).  The root of a cluster is
// its smallest vertex index; the cluster is reflected iff the root's coin says so, sigma' = sigma - 2 a r for every vertex of
// it, stored in the canonical form (sigma2d.hip).  Every decision is a function of (link or root, chain, update counter,
// field before the update): the state does not depend on the launch plan, the tile, the batch split or chain0.
//
// RNG contract, step = global update counter update0 + k:
//   P_SIGMA_SW_REFLECT  site 0, sub 0: (u, v) -> r_z = 1 - 2 u, azimuth 2 pi v - pi (the map of P_SIGMA_REFLECT sub 0)
//   P_SIGMA_SW_BOND     site l, sub 0: u decides link (l, 0), v decides link (l, 1)
//   P_SIGMA_SW_FLIP     site root, sub 0: reflected iff u < 0.5
//
// Improved estimator.  With A_C the sum of a_l over cluster C, 3 sum_C A_C^2 / N is an unbiased estimator of chi_m = <|M|^2> / N
// (the mean of (M . r)^2 over the coins is sum_C A_C^2, the mean over r is |M|^2 / 3).  A_C is summed in 64-bit fixed point,
// q(a) = llrint(a 2^32), with integer atomic adds on the root's slot (N <= 2^30 keeps it inside 63 bits), and (A_C 2^-32)^2 is
// summed over the roots by sw_finish: one workgroup of 1024 threads, thread t takes the vertices t, t + 1024, .. in ascending
// order, then a fixed tree.  That sum is the same bits under every plan, and it is ADDED to the caller's accumulator update by
// update, so that 10 updates equal 5 + 5 to the bit.
//
// Labelling.  The parent of a vertex is a vertex of its cluster with a smaller or equal index; a root is its own parent.
// union(x, y): find both roots, hang the larger under the smaller with an atomic min on the parent word of the larger; if
// the word held something else meanwhile (another lane got there first), go on with (what it held, the smaller root): the
// edge the min may have replaced is the one that pair restores.  max(x, y) decreases with every retry, a path visits
// decreasing indices: N iterations bound every loop, and the final root of a component is its smallest vertex whatever the
// order of arrival.  A cap that is hit all the same sets a status word the entry point returns as an error.
#include <mutex>

#include "internal.hpp"

#include "sigma_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

constexpr uint32_t kSwThreads = 256;         // tiled plan: bond + label, merge, resolve
constexpr uint32_t kSwFinishThreads = 1024;  // the fixed configuration of sw_finish; the chain plan's workgroup
// chain plan: a (8 B), the root's sum (8 B) and the parent (4 B) of every vertex in LDS beside the 12 KiB of sw_finish
constexpr uint32_t kSwChainBytesPerVertex = 20;
constexpr uint32_t kSwChainMaxN = (160 * 1024 - 12 * 1024 - 512) / kSwChainBytesPerVertex;  // 7552 vertices
constexpr double kSwFix = 4294967296.0;      // 2^32
constexpr int kSwPlain = -1;                 // sw_find: plain loads (nobody writes the parents any more)

__device__ __forceinline__ double sw_dot(const V3 &r, const V3 &s) { return (r.x * s.x + r.y * s.y) + r.z * s.z; }

__device__ __forceinline__ V3 sw_normal(const RngKey &key) {
  double u, v;
  rng_uniforms(key, 0, P_SIGMA_SW_REFLECT, 0, u, v);
  const double rz = 1.0 - 2.0 * u, t = 1.0 - rz * rz, rho = t > 0.0 ? sqrt(t) : 0.0;
  double sa, ca;
  sincos(kTwoPi * v - kPi, &sa, &ca);
  return V3{rho * ca, rho * sa, rz};
}

__device__ __forceinline__ bool sw_bonded(double ax, double ay, double beta2, double uni) {
  const double prod = ax * ay;
  if (!(prod > 0.0)) return false;                       // p = 0: never bonded
  return uni < 1.0 - exp(fmin(0.0, -(beta2 * prod)));
}

// (bond of link (l, 0), bond of link (l, 1)) as bits 0 and 1
__device__ __forceinline__ uint32_t sw_bonds(const RngKey &key, uint32_t l, double a, double a_right, double a_up, double beta2) {
  const U4 w = philox4x32_10(l, key.chain, key.step, (uint32_t)P_SIGMA_SW_BOND << 24, key.k0, key.k1);
  return (sw_bonded(a, a_right, beta2, u01(w.x, w.y)) ? 1u : 0u) | (sw_bonded(a, a_up, beta2, u01(w.z, w.w)) ? 2u : 0u);
}

__device__ __forceinline__ bool sw_coin(const RngKey &key, uint32_t root) {
  double u, unused;
  rng_uniforms(key, root, P_SIGMA_SW_FLIP, 0, u, unused);
  return u < 0.5;
}

__device__ __forceinline__ double2 sw_reflected(const V3 &s, double a, const V3 &r) {
  const double c = 2.0 * a;
  return angles_of(V3{s.x - c * r.x, s.y - c * r.y, s.z - c * r.z});
}

__device__ __forceinline__ long long sw_fixed(double a) { return llrint(a * kSwFix); }

template <int SCOPE>
__device__ __forceinline__ uint32_t sw_parent(const uint32_t *parent, uint32_t x) {
  // other lanes (tiled plan: workgroups on other XCDs) lower parent words meanwhile: an atomic load of that scope, not a plain one
  if constexpr (SCOPE == kSwPlain) return parent[x];
  else return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
}

// the root above x; a path visits strictly decreasing indices, so `cap` >= the number of vertices bounds it
template <int SCOPE>
__device__ __forceinline__ uint32_t sw_find(const uint32_t *parent, uint32_t x, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {
    const uint32_t p = sw_parent<SCOPE>(parent, x);
    if (p == x) return x;
    x = p;
  }
  capped = true;
  return x;
}

template <int SCOPE>
__device__ __forceinline__ void sw_union(uint32_t *parent, uint32_t x, uint32_t y, uint32_t cap, bool &capped) {
  for (uint32_t it = 0; it < cap; ++it) {                // max(x, y) decreases with every retry
    x = sw_find<SCOPE>(parent, x, cap, capped);
    y = sw_find<SCOPE>(parent, y, cap, capped);
    if (x == y || capped) return;
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

// sum over the roots of (A_C 2^-32)^2 and their number, in the fixed configuration (kSwFinishThreads threads, every thread of
// the workgroup calls it); thread 0 adds 3 / N x the sum to *improved and the number to *clusters (either may be NULL)
__device__ __forceinline__ void sw_finish(const uint32_t *parent, const long long *sum, uint32_t N, double *red, uint32_t *redc,
                                          double *improved, uint32_t *clusters) {
  const uint32_t t = threadIdx.x;
  double s = 0.0;
  uint32_t c = 0;
  for (uint32_t l = t; l < N; l += kSwFinishThreads)
    if (parent[l] == l) {
      const double A = (double)sum[l] * (1.0 / kSwFix);
      s += A * A;
      ++c;
    }
  red[t] = s;
  redc[t] = c;
  __syncthreads();
  for (uint32_t off = kSwFinishThreads / 2; off > 0; off >>= 1) {
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

// one atomic per wave: the lanes of the wave that flipped a vertex
__device__ __forceinline__ void sw_count_flips(bool flip, uint32_t *flipped_b) {
  const unsigned long long m = __ballot(flip);
  if (flipped_b && m && (threadIdx.x & (kWave - 1)) == (uint32_t)__builtin_ctzll(m)) atomicAdd(flipped_b, (uint32_t)__builtin_popcountll(m));
}

// ---- tiled plan, launch 1: bonds of the tile's vertices, union-find on the tile's interior links in LDS --------------------
// A workgroup takes a tile of W x H vertices (w x h where the lattice ends: masked, not padded) of one chain.  LDS: a of the
// tile and of its +i / +j halo [(H + 1)(W + 1)] double, the parents [H W] uint32 (local index W lj + li: the order of the
// global index inside a tile), the bond bits [H W] uint8.
__global__ void __launch_bounds__(kSwThreads)
    sigma_sw_bond_label_kernel(const double2 *phi_all, uint32_t Mt, uint32_t Mx, double beta2, RngKey key0, uint32_t W, uint32_t H,
                               uint32_t ntx, uint32_t nty, uint32_t *label_all, uint8_t *bits_all, long long *qa_all,
                               long long *sum_all, uint32_t *status) {
  extern __shared__ double sw_lds[];
  const uint32_t SA = W + 1;
  double *a = sw_lds;
  uint32_t *parent = (uint32_t *)(a + (size_t)SA * (H + 1));
  uint8_t *lbits = (uint8_t *)(parent + W * H);
  const uint32_t tiles = ntx * nty, b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const uint32_t i0 = (tile % ntx) * W, j0 = (tile / ntx) * H;
  const uint32_t w = Mt - i0 < W ? Mt - i0 : W, h = Mx - j0 < H ? Mx - j0 : H;
  const uint32_t N = Mt * Mx;
  const double2 *phi = phi_all + (size_t)b * N;
  RngKey key = key0;
  key.chain = key0.chain + b;
  const V3 r = sw_normal(key);

  for (uint32_t p = threadIdx.x; p < (w + 1) * (h + 1) - 1; p += kSwThreads) {   // - 1: the corner of the halo has no link
    const uint32_t li = p % (w + 1), lj = p / (w + 1);
    uint32_t gi = i0 + li, gj = j0 + lj;
    gi = gi == Mt ? 0 : gi;
    gj = gj == Mx ? 0 : gj;
    const uint32_t l = gj * Mt + gi;
    const double al = sw_dot(r, sigma_of(phi[l]));
    a[lj * SA + li] = al;
    if (li < w && lj < h) {
      qa_all[(size_t)b * N + l] = sw_fixed(al);
      if (sum_all) sum_all[(size_t)b * N + l] = 0;
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kSwThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, l = (j0 + lj) * Mt + i0 + li;
    const uint32_t bits = sw_bonds(key, l, a[lj * SA + li], a[lj * SA + li + 1], a[(lj + 1) * SA + li], beta2);
    bits_all[(size_t)b * N + l] = (uint8_t)bits;
    lbits[loc] = (uint8_t)bits;
    parent[loc] = loc;
  }
  __syncthreads();
  bool capped = false;
  for (uint32_t p = threadIdx.x; p < w * h; p += kSwThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, bits = lbits[loc];
    if ((bits & 1u) && li + 1 < w) sw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, loc + 1, W * H, capped);
    if ((bits & 2u) && lj + 1 < h) sw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, loc + W, W * H, capped);
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kSwThreads) {
    const uint32_t li = p % w, lj = p / w;
    const uint32_t root = sw_find<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, lj * W + li, W * H, capped);
    label_all[(size_t)b * N + (j0 + lj) * Mt + i0 + li] = (j0 + root / W) * Mt + i0 + root % W;
  }
  if (capped) atomicOr(status, 1u);
}

// ---- launch 2: one lane per link that leaves its tile (the periodic wrap and both links of an extent-2 pair included) -------
// per chain ntx Mx links of direction 0 (from the last column of every tile column) and nty Mt of direction 1
__global__ void __launch_bounds__(kSwThreads)
    sigma_sw_merge_kernel(uint32_t Mt, uint32_t Mx, uint32_t W, uint32_t H, uint32_t ntx, uint32_t nty, uint32_t blocks,
                          uint32_t *label_all, const uint8_t *bits_all, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, e = (blockIdx.x % blocks) * kSwThreads + threadIdx.x;
  const uint32_t N = Mt * Mx, E0 = ntx * Mx, E1 = nty * Mt;
  if (e >= E0 + E1) return;
  uint32_t l, y, bit;
  if (e < E0) {
    const uint32_t c = e % ntx, j = e / ntx;
    const uint32_t i = ((c + 1) * W < Mt ? (c + 1) * W : Mt) - 1;
    l = j * Mt + i;
    y = i + 1 == Mt ? l - i : l + 1;
    bit = 1u;
  } else {
    const uint32_t i = (e - E0) % Mt, c = (e - E0) / Mt;
    const uint32_t j = ((c + 1) * H < Mx ? (c + 1) * H : Mx) - 1;
    l = j * Mt + i;
    y = j + 1 == Mx ? i : l + Mt;
    bit = 2u;
  }
  if (!(bits_all[(size_t)b * N + l] & bit)) return;
  bool capped = false;
  sw_union<__HIP_MEMORY_SCOPE_AGENT>(label_all + (size_t)b * N, l, y, N, capped);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 3: every vertex follows its label to the final root, adds q(a) to the root's slot, evaluates the root's coin -----
// and, when the coin says so, stores its reflection (non-temporal; nothing is stored otherwise)
__global__ void __launch_bounds__(kSwThreads)
    sigma_sw_resolve_kernel(double2 *phi_all, uint32_t Mt, uint32_t Mx, RngKey key0, uint32_t blocks, const uint32_t *label_all,
                            const long long *qa_all, long long *sum_all, uint32_t *flipped, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kSwThreads + threadIdx.x;
  const uint32_t N = Mt * Mx;
  RngKey key = key0;
  key.chain = key0.chain + b;
  bool flip = false, capped = false;
  if (l < N) {
    const uint32_t root = sw_find<kSwPlain>(label_all + (size_t)b * N, l, N, capped);
    if (sum_all) atomicAdd((unsigned long long *)(sum_all + (size_t)b * N + root), (unsigned long long)qa_all[(size_t)b * N + l]);
    flip = !capped && sw_coin(key, root);
    if (flip) {
      const V3 r = sw_normal(key);
      double2 *p = phi_all + (size_t)b * N + l;
      const V3 s = sigma_of(*p);
      const double2 out = sw_reflected(s, sw_dot(r, s), r);
      __builtin_nontemporal_store(out.x, &p->x);
      __builtin_nontemporal_store(out.y, &p->y);
    }
  }
  sw_count_flips(flip, flipped ? flipped + b : nullptr);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 4 (only when outputs are asked for): one workgroup per chain --------------------------------------------------
__global__ void __launch_bounds__(kSwFinishThreads)
    sigma_sw_finish_kernel(const uint32_t *label_all, const long long *sum_all, uint32_t N, double *improved, uint32_t *clusters) {
  __shared__ double red[kSwFinishThreads];
  __shared__ uint32_t redc[kSwFinishThreads];
  const uint32_t b = blockIdx.x;
  sw_finish(label_all + (size_t)b * N, sum_all + (size_t)b * N, N, red, redc, improved ? improved + b : nullptr,
            clusters ? clusters + b : nullptr);
}

// ---- chain plan: one workgroup per chain, all n_updates updates in one launch, labels, sums and a in LDS ------------------
// Thread t owns the vertices t, t + 1024, ..: it alone reads and writes their angles, update after update.
__global__ void __launch_bounds__(kSwFinishThreads)
    sigma_sw_chain_kernel(double2 *phi_all, uint32_t Mt, uint32_t Mx, double beta2, uint32_t n_updates, RngKey key0, uint32_t *flipped,
                          uint32_t *clusters, double *improved, uint32_t *status) {
  extern __shared__ double sw_lds[];
  __shared__ double red[kSwFinishThreads];
  __shared__ uint32_t redc[kSwFinishThreads];
  const uint32_t N = Mt * Mx, b = blockIdx.x, t = threadIdx.x;
  double *a = sw_lds;
  long long *sum = (long long *)(a + N);
  uint32_t *parent = (uint32_t *)(sum + N);
  double2 *phi = phi_all + (size_t)b * N;
  const bool outputs = clusters || improved;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t nflip = 0;
  bool capped = false;
  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    const V3 r = sw_normal(key);
    for (uint32_t l = t; l < N; l += kSwFinishThreads) {
      a[l] = sw_dot(r, sigma_of(phi[l]));
      sum[l] = 0;
      parent[l] = l;
    }
    __syncthreads();
    for (uint32_t l = t; l < N; l += kSwFinishThreads) {
      const uint32_t i = l % Mt, j = l / Mt;
      const uint32_t right = i + 1 == Mt ? l - i : l + 1, up = j + 1 == Mx ? i : l + Mt;
      const uint32_t bits = sw_bonds(key, l, a[l], a[right], a[up], beta2);
      if (bits & 1u) sw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, l, right, N, capped);
      if (bits & 2u) sw_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, l, up, N, capped);
    }
    __syncthreads();
    for (uint32_t l = t; l < N; l += kSwFinishThreads) {
      const uint32_t root = sw_find<kSwPlain>(parent, l, N, capped);
      if (improved) atomicAdd((unsigned long long *)(sum + root), (unsigned long long)sw_fixed(a[l]));
      if (!capped && sw_coin(key, root)) {
        phi[l] = sw_reflected(sigma_of(phi[l]), a[l], r);
        ++nflip;
      }
    }
    __syncthreads();
    if (outputs) sw_finish(parent, sum, N, red, redc, improved ? improved + b : nullptr, clusters ? clusters + b : nullptr);
    __syncthreads();
  }
  if (flipped) {
    for (int off = kWave / 2; off > 0; off >>= 1) nflip += __shfl_down(nflip, off);
    if ((t & (kWave - 1)) == 0 && nflip) atomicAdd(flipped + b, nflip);
  }
  if (capped) atomicOr(status, 1u);
}

namespace {

struct SwPlan {
  bool ok, chain;
  uint32_t W, H, ntx, nty;          // tiled: tile extents, tiles per direction
  uint32_t merge_blocks, resolve_blocks;  // tiled: workgroups per chain of launches 2 and 3
  size_t lds_bytes;                 // dynamic LDS of the chain kernel / of launch 1
};

// Launch plan; it chooses and calls nothing.  The chain plan where a chain fits its LDS bound and one
// workgroup per chain fills the device (B >= kComputeUnits: a chain's workgroup is 16 waves and takes more than half a CU's
// LDS, so one is resident per CU), the tiled plan otherwise.  Knobs (bit-identical results): MLMCPI_SIGMA_SW_PLAN=chain|tiled,
// MLMCPI_SIGMA_SW_TILE=WxH.  ok = false: the chain plan was forced on a lattice beyond its bound.
SwPlan sw_plan(uint32_t Mt, uint32_t Mx, uint32_t B, const Tuning &tune) {
  SwPlan p{};
  const uint32_t N = Mt * Mx;
  p.chain = tune.sigma_sw_plan ? tune.sigma_sw_plan == 1 : (N <= kSwChainMaxN && B >= kComputeUnits);
  p.ok = !p.chain || N <= kSwChainMaxN;
  p.W = tune.sigma_sw_tile_w ? tune.sigma_sw_tile_w : 64;
  p.H = tune.sigma_sw_tile_h ? tune.sigma_sw_tile_h : 32;
  p.ntx = (Mt + p.W - 1) / p.W;
  p.nty = (Mx + p.H - 1) / p.H;
  p.merge_blocks = (p.ntx * Mx + p.nty * Mt + kSwThreads - 1) / kSwThreads;
  p.resolve_blocks = (N + kSwThreads - 1) / kSwThreads;
  p.lds_bytes = p.chain ? (size_t)N * kSwChainBytesPerVertex
                        : (size_t)(p.W + 1) * (p.H + 1) * sizeof(double) + (size_t)p.W * p.H * (sizeof(uint32_t) + sizeof(uint8_t));
  return p;
}

std::mutex g_sw_attr_mutex;
bool g_sw_attr_set[64] = {false};

int sw_init_attrs() {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(MLMCPI_ERR_INVALID, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_sw_attr_mutex);
  if (g_sw_attr_set[dev]) return MLMCPI_OK;
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSwChainMaxN * kSwChainBytesPerVertex));
  g_sw_attr_set[dev] = true;
  return MLMCPI_OK;
}

int sw_check(const mlmcpi_lattice_action *act, const char *what) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: the Swendsen-Wang update is built for the O(3) nonlinear sigma model only "
                "(action kind %d)", what, act->kind);
  if (int rc = check_lattice(act)) return rc;
  if (!(act->beta > 0.0)) return fail(MLMCPI_ERR_INVALID, "beta must be positive");
  return MLMCPI_OK;
}

// workspace sections: status word (256 B), label [B N] uint32, q(a) [B N] int64, cluster sums [B N] int64, bond bits [B N] uint8
constexpr size_t kSwStatusBytes = 256;
size_t sw_section_label(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(uint32_t)); }
size_t sw_section_fixed(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(long long)); }
size_t sw_section_bits(uint32_t N, uint32_t B) { return align256((size_t)B * N); }

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_sw_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_workspace_bytes")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  const uint32_t N = act->Mt * act->Mx;
  *bytes = kSwStatusBytes + sw_section_label(N, B) + 2 * sw_section_fixed(N, B) + sw_section_bits(N, B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_sw_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed, uint32_t chain0,
                         uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved, void *d_work, void *stream) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_draw")) return rc;
  MLMCPI_REQUIRE(d_phi && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  const uint32_t Mt = act->Mt, Mx = act->Mx, N = Mt * Mx;
  const SwPlan p = sw_plan(Mt, Mx, B, tuning());
  if (!p.ok)
    return fail(MLMCPI_ERR_UNSUPPORTED, "mlmcpi_sigma_sw_draw: MLMCPI_SIGMA_SW_PLAN=chain holds a chain of at most %u vertices in LDS, "
                "this lattice has %u", kSwChainMaxN, N);
  const uint64_t widest = (uint64_t)B * (p.ntx * p.nty > p.resolve_blocks ? p.ntx * p.nty : p.resolve_blocks);
  MLMCPI_REQUIRE(p.chain || (widest < (1ull << 31) && (uint64_t)B * p.merge_blocks < (1ull << 31)), "too many workgroups for one launch: split the batch");
  if (n_updates == 0) return MLMCPI_OK;
  if (int rc = sw_init_attrs()) return rc;
  char *w = (char *)d_work;
  uint32_t *status = (uint32_t *)w;
  uint32_t *label = (uint32_t *)(w + kSwStatusBytes);
  long long *qa = (long long *)(w + kSwStatusBytes + sw_section_label(N, B));
  long long *sum = (long long *)(w + kSwStatusBytes + sw_section_label(N, B) + sw_section_fixed(N, B));
  uint8_t *bits = (uint8_t *)(w + kSwStatusBytes + sw_section_label(N, B) + 2 * sw_section_fixed(N, B));
  const hipStream_t st = as_stream(stream);
  const double beta2 = 2.0 * act->beta;
  MLMCPI_HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
  if (p.chain) {
    hipLaunchKernelGGL(sigma_sw_chain_kernel, dim3(B), dim3(kSwFinishThreads), p.lds_bytes, st, (double2 *)d_phi, Mt, Mx, beta2, n_updates,
                       make_key(seed, chain0, update0), d_flipped, d_clusters, d_improved, status);
    MLMCPI_LAUNCH_CHECK("sigma_sw_chain_kernel");
  } else {
    const bool outputs = d_clusters || d_improved;
    for (uint32_t k = 0; k < n_updates; ++k) {
      const RngKey key = make_key(seed, chain0, update0 + k);
      hipLaunchKernelGGL(sigma_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kSwThreads), p.lds_bytes, st, (const double2 *)d_phi, Mt,
                         Mx, beta2, key, p.W, p.H, p.ntx, p.nty, label, bits, qa, d_improved ? sum : nullptr, status);
      MLMCPI_LAUNCH_CHECK("sigma_sw_bond_label_kernel");
      hipLaunchKernelGGL(sigma_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kSwThreads), 0, st, Mt, Mx, p.W, p.H, p.ntx, p.nty,
                         p.merge_blocks, label, bits, status);
      MLMCPI_LAUNCH_CHECK("sigma_sw_merge_kernel");
      hipLaunchKernelGGL(sigma_sw_resolve_kernel, dim3(B * p.resolve_blocks), dim3(kSwThreads), 0, st, (double2 *)d_phi, Mt, Mx, key,
                         p.resolve_blocks, label, qa, d_improved ? sum : nullptr, d_flipped, status);
      MLMCPI_LAUNCH_CHECK("sigma_sw_resolve_kernel");
      if (outputs) {
        hipLaunchKernelGGL(sigma_sw_finish_kernel, dim3(B), dim3(kSwFinishThreads), 0, st, label, sum, N, d_improved, d_clusters);
        MLMCPI_LAUNCH_CHECK("sigma_sw_finish_kernel");
      }
    }
  }
  // a find or union loop that ran into its cap (it cannot, by the argument above): an error, never a hang
  uint32_t h_status = 0;
  MLMCPI_HIP_TRY(hipMemcpyAsync(&h_status, status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MLMCPI_HIP_TRY(hipStreamSynchronize(st));
  if (h_status) return fail(MLMCPI_ERR_HIP, "mlmcpi_sigma_sw_draw: a labelling loop reached its iteration cap (status %u); the state is undefined", h_status);
  return MLMCPI_OK;
}

}  // extern "C"
