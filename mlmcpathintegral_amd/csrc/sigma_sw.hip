// sigma_sw.hip -- the Swendsen-Wang multi-cluster update of the O(3) nonlinear sigma model (gfx950, wave64), on the unrotated
// lattice (mlmcpi_sigma_sw_*) and on the levels of its CoarsenRotate hierarchy (mlmcpi_sigma_level_sw_*; an unrotated level IS
// the lattice and takes its entry point).  The geometry lives in sigma_cluster_device.hpp (LatticeGeometry, RotatedGeometry): the
// chain kernel is instantiated on it, the resolve and finish kernels use none, the two tile front ends (bond + label, merge)
// are written once per geometry.
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
// On a rotated level (tests/sigma_level_sw_model.py) the same update with the level's indices: n = Mt Mx / 2 vertices, plane E then
// plane O, the 2 n links named (e, d) from their E end (sigma_cluster_device.hpp), the root of a cluster its smallest LEVEL
// index (also when the cluster is a lone O vertex), P_SIGMA_SW_BOND at site e, sub d >> 1: u decides link (e, d) for d even, v
// for d odd.  union(x, x) returns at once (level (2, 2): the four links of E(0, 0) all end at O(0, 0)).
//
// Improved structure factor (mlmcpi_sigma_level_sw_structure_draw): per cluster and direction d the two sums
// of q(a_l w), w = cos, sin of 2 pi x_d(l) / M_d from sw_phase, on four further root slots; each is finished as A_C is and added
// to structure[b][d], cos then sin.  The structure instances: sigma_sw_resolve_structure_kernel<Geometry>,
// sigma_sw_finish_structure_kernel, sigma_sw_chain_kernel<WithStructure<Geometry>>; the instances of the plain draw are untouched.
//
// Improved correlator (mlmcpi_sigma_level_sw_correlator_draw): per cluster, direction and slice the sum of q(a)
// in a hash table keyed by (root, slice), per cluster and lag the products of those sums in a 64-bit fixed-point accumulator,
// added to corr[b][n_out] update by update.  The instances: sigma_sw_chain_kernel<WithRoots<Geometry>> (it leaves roots and q(a)
// where the tiled plan has them), sigma_sw_slice_sum_kernel<Geometry>, sigma_sw_slice_pair_kernel, sigma_sw_slice_finish_kernel;
// the instances of the plain and the structure draw are untouched.
//
// Labelling: the parent array and the union by atomic min of sigma_cluster_device.hpp (uf_*), where its termination argument
// is written out.
#include <mutex>

#include "internal.hpp"

#include "sigma_cluster_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

constexpr uint32_t kSwMaxTile = 64;          // the largest tile extent MLMCPI_SIGMA_SW_TILE admits, in cells

// rotated level, launch 1: a of the tile's E cells [W H], a of its O cells and their -a / -b halo [(W + 1)(H + 1)], the parents
// [2 W H] uint32, the bond bits [W H] uint8
__host__ __device__ constexpr size_t sw_rot_tile_lds(uint32_t W, uint32_t H) {
  return ((size_t)W * H + (size_t)(W + 1) * (H + 1)) * sizeof(double) + (size_t)2 * W * H * sizeof(uint32_t) + (size_t)W * H;
}

// ---- tiled plan, launch 1: bonds of the tile's vertices, union-find on the tile's interior links in LDS --------------------
// A workgroup takes a tile of W x H vertices (w x h where the lattice ends: masked, not padded) of one chain.  LDS: a of the
// tile and of its +i / +j halo [(H + 1)(W + 1)] double, the parents [H W] uint32 (local index W lj + li: the order of the
// global index inside a tile), the bond bits [H W] uint8.
__global__ void __launch_bounds__(kClusterThreads)
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
  const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);

  for (uint32_t p = threadIdx.x; p < (w + 1) * (h + 1) - 1; p += kClusterThreads) {   // - 1: the corner of the halo has no link
    const uint32_t li = p % (w + 1), lj = p / (w + 1);
    uint32_t gi = i0 + li, gj = j0 + lj;
    gi = gi == Mt ? 0 : gi;
    gj = gj == Mx ? 0 : gj;
    const uint32_t l = gj * Mt + gi;
    const double al = dot3(r, sigma_of(phi[l]));
    a[lj * SA + li] = al;
    if (li < w && lj < h) {
      qa_all[(size_t)b * N + l] = sw_fixed(al);
      if (sum_all) sum_all[(size_t)b * N + l] = 0;
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kClusterThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, l = (j0 + lj) * Mt + i0 + li;
    const uint32_t bits = LatticeGeometry::bonds(key, l, a[lj * SA + li], a[lj * SA + li + 1], a[(lj + 1) * SA + li], beta2);
    bits_all[(size_t)b * N + l] = (uint8_t)bits;
    lbits[loc] = (uint8_t)bits;
    parent[loc] = loc;
  }
  __syncthreads();
  bool capped = false;
  for (uint32_t p = threadIdx.x; p < w * h; p += kClusterThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, bits = lbits[loc];
    if ((bits & 1u) && li + 1 < w) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, loc + 1, W * H, capped);
    if ((bits & 2u) && lj + 1 < h) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, loc + W, W * H, capped);
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kClusterThreads) {
    const uint32_t li = p % w, lj = p / w;
    const uint32_t root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, lj * W + li, W * H, capped);
    label_all[(size_t)b * N + (j0 + lj) * Mt + i0 + li] = (j0 + root / W) * Mt + i0 + root % W;
  }
  if (capped) atomicOr(status, 1u);
}

// ---- launch 2: one lane per link that leaves its tile (the periodic wrap and both links of an extent-2 pair included) -------
// per chain ntx Mx links of direction 0 (from the last column of every tile column) and nty Mt of direction 1
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_merge_kernel(uint32_t Mt, uint32_t Mx, uint32_t W, uint32_t H, uint32_t ntx, uint32_t nty, uint32_t blocks,
                          uint32_t *label_all, const uint8_t *bits_all, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, e = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
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
  uf_union<__HIP_MEMORY_SCOPE_AGENT>(label_all + (size_t)b * N, l, y, N, capped);
  if (capped) atomicOr(status, 1u);
}

// ---- rotated level, launch 1: bonds of the tile's E vertices, union-find on the tile's interior links in LDS ----------------
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
__global__ void __launch_bounds__(kClusterThreads)
    sigma_rot_sw_bond_label_kernel(const double2 *phi_all, SigmaLevel L, double beta2, RngKey key0, uint32_t W, uint32_t H,
                                   uint32_t ntx, uint32_t nty, uint32_t *label_all, uint8_t *bits_all, long long *qa_all,
                                   long long *sum_all, uint32_t *status) {
  extern __shared__ double sw_lds[];
  const uint32_t SA = W + 1, WH = W * H;
  double *aE = sw_lds;
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
  const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);

  for (uint32_t p = threadIdx.x; p < (w + 1) * (h + 1); p += kClusterThreads) {
    const uint32_t li = p % (w + 1), lj = p / (w + 1);   // O image: (0, .) and (., 0) are the halo, (li, lj) is cell (li - 1, lj - 1)
    const uint32_t oa = a0 + li == 0 ? ht - 1 : a0 + li - 1, ob = b0 + lj == 0 ? hx - 1 : b0 + lj - 1;
    const uint32_t lo = q + ob * ht + oa;
    const double ao = dot3(r, sigma_of(phi[lo]));
    aO[lj * SA + li] = ao;
    if (li > 0 && lj > 0) {                              // a cell of the tile: its O vertex and its E vertex
      const uint32_t le = lo - q;
      const double ae = dot3(r, sigma_of(phi[le]));
      aE[(lj - 1) * W + li - 1] = ae;
      qa_all[(size_t)b * n + lo] = sw_fixed(ao);
      qa_all[(size_t)b * n + le] = sw_fixed(ae);
      if (sum_all) {
        sum_all[(size_t)b * n + lo] = 0;
        sum_all[(size_t)b * n + le] = 0;
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < w * h; p += kClusterThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, e = (b0 + lj) * ht + a0 + li;
    const double ao[4] = {aO[(lj + 1) * SA + li + 1], aO[lj * SA + li + 1], aO[(lj + 1) * SA + li], aO[lj * SA + li]};
    const uint32_t bits = RotatedGeometry::bonds(key, e, aE[loc], ao, beta2);
    bits_all[(size_t)b * q + e] = (uint8_t)bits;
    lbits[loc] = (uint8_t)bits;
    parent[loc] = loc;
    parent[WH + loc] = WH + loc;
  }
  __syncthreads();
  bool capped = false;
  for (uint32_t p = threadIdx.x; p < w * h; p += kClusterThreads) {
    const uint32_t li = p % w, lj = p / w, loc = lj * W + li, bits = lbits[loc];
    if (bits & 1u) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc, 2 * WH, capped);
    if ((bits & 2u) && lj > 0) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - W, 2 * WH, capped);
    if ((bits & 4u) && li > 0) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - 1, 2 * WH, capped);
    if ((bits & 8u) && li > 0 && lj > 0) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, loc, WH + loc - W - 1, 2 * WH, capped);
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < 2 * w * h; p += kClusterThreads) {
    const uint32_t plane = p >= w * h ? 1u : 0u, c = p - plane * w * h, li = c % w, lj = c / w;
    const uint32_t root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, plane * WH + lj * W + li, 2 * WH, capped);
    const uint32_t rplane = root >= WH ? 1u : 0u, rc = root - rplane * WH;
    label_all[(size_t)b * n + plane * q + (b0 + lj) * ht + a0 + li] = rplane * q + (b0 + rc / W) * ht + a0 + rc % W;
  }
  if (capped) atomicOr(status, 1u);
}

// ---- rotated level, launch 2: one lane per link that leaves its tile -------------------------------------------------------------------
// Per chain: 2 ntx hx lanes for the links d = 2, 3 of the E vertices in the first column of every tile column (their O end is
// one column to the -a side: another tile, or the wrap), then 2 nty ht lanes for the links d = 1, 3 of the E vertices in the
// first row of every tile row.  The d = 3 link of a tile's corner cell is in both sets: the lane of the second set returns, so
// it is crossed once.
__global__ void __launch_bounds__(kClusterThreads)
    sigma_rot_sw_merge_kernel(SigmaLevel L, uint32_t W, uint32_t H, uint32_t ntx, uint32_t nty, uint32_t blocks, uint32_t *label_all,
                              const uint8_t *bits_all, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, x = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
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
  uf_union<__HIP_MEMORY_SCOPE_AGENT>(label_all + (size_t)b * n, e, q + ob * ht + oa, n, capped);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 3: every vertex follows its label to the final root, adds q(a) to the root's slot, evaluates the root's coin -----
// and, when the coin says so, stores its reflection (non-temporal; nothing is stored otherwise)
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_resolve_kernel(double2 *phi_all, uint32_t N, RngKey key0, uint32_t blocks, const uint32_t *label_all,
                            const long long *qa_all, long long *sum_all, uint32_t *flipped, uint32_t *status) {
  const uint32_t b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
  RngKey key = key0;
  key.chain = key0.chain + b;
  bool flip = false, capped = false;
  if (l < N) {
    const uint32_t root = uf_find<kUfPlain>(label_all + (size_t)b * N, l, N, capped);
    if (sum_all) atomicAdd((unsigned long long *)(sum_all + (size_t)b * N + root), (unsigned long long)qa_all[(size_t)b * N + l]);
    flip = !capped && sw_coin(key, root);
    if (flip) {
      const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);
      double2 *p = phi_all + (size_t)b * N + l;
      const V3 s = sigma_of(*p);
      const double2 out = reflected(s, dot3(r, s), r);
      __builtin_nontemporal_store(out.x, &p->x);
      __builtin_nontemporal_store(out.y, &p->y);
    }
  }
  sw_count_flips(flip, flipped ? flipped + b : nullptr);
  if (capped) atomicOr(status, 1u);
}

// launch 3 with the structure sums: the same update, and q(a) and the four weighted values q(a w) go onto the root's five slots
// (`section` apart), the lanes of a wave that share a root combined first.  a is formed again from the field before the update
// (the same dot3 on the same bits as launch 1; nobody else stores this vertex).  Every lane stays to the end: the combining
// shuffles run with the whole wave.
template <class Geometry>
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_resolve_structure_kernel(double2 *phi_all, Geometry g, RngKey key0, uint32_t blocks, const uint32_t *label_all,
                                      const long long *qa_all, long long *sum_all, size_t section, uint32_t *flipped, uint32_t *status) {
  const uint32_t N = g.nvert(), b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
  const bool active = l < N;
  RngKey key = key0;
  key.chain = key0.chain + b;
  const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);
  bool flip = false, capped = false;
  uint32_t root = 0;
  long long v[5] = {0, 0, 0, 0, 0};
  V3 s{0.0, 0.0, 0.0};
  double a = 0.0;
  if (active) {
    root = uf_find<kUfPlain>(label_all + (size_t)b * N, l, N, capped);
    s = sigma_of(phi_all[(size_t)b * N + l]);
    a = dot3(r, s);
    v[0] = qa_all[(size_t)b * N + l];
#pragma unroll
    for (uint32_t d = 0; d < 2; ++d) {
      double ws, wc;
      sw_phase(g.position(l, d), g.extent(d), ws, wc);
      v[1 + 2 * d] = sw_fixed(a * wc);
      v[2 + 2 * d] = sw_fixed(a * ws);
    }
    flip = !capped && sw_coin(key, root);
  }
  sw_add_combined<__HIP_MEMORY_SCOPE_AGENT>(sum_all + (size_t)b * N, section, root, active, v);
  if (flip) {
    double2 *p = phi_all + (size_t)b * N + l;
    const double2 out = reflected(s, a, r);
    __builtin_nontemporal_store(out.x, &p->x);
    __builtin_nontemporal_store(out.y, &p->y);
  }
  sw_count_flips(flip, flipped ? flipped + b : nullptr);
  if (capped) atomicOr(status, 1u);
}

// ---- launch 4 (only when outputs are asked for): one workgroup per chain --------------------------------------------------
__global__ void __launch_bounds__(kClusterBlockThreads)
    sigma_sw_finish_kernel(const uint32_t *label_all, const long long *sum_all, uint32_t N, double *improved, uint32_t *clusters) {
  __shared__ double red[kClusterBlockThreads];
  __shared__ uint32_t redc[kClusterBlockThreads];
  const uint32_t b = blockIdx.x;
  sw_finish(label_all + (size_t)b * N, sum_all + (size_t)b * N, N, red, redc, improved ? improved + b : nullptr,
            clusters ? clusters + b : nullptr);
}

// launch 4 with the structure sums: what the plain one does and the same fixed-configuration finish of the four structure
// slots, cos then sin of direction d ADDED to structure[b][d] one after the other; the four slots of every root go back to
// zero as they are read (the resolve kernel adds to roots only)
__global__ void __launch_bounds__(kClusterBlockThreads)
    sigma_sw_finish_structure_kernel(const uint32_t *label_all, long long *sum_all, size_t section, uint32_t N, double *improved,
                                     uint32_t *clusters, double *structure) {
  __shared__ double red[kClusterBlockThreads];
  __shared__ uint32_t redc[kClusterBlockThreads];
  const uint32_t b = blockIdx.x;
  const uint32_t *label = label_all + (size_t)b * N;
  long long *sum = sum_all + (size_t)b * N;
  // one walk over the labels for the five slots: per slot the terms meet in the order of sw_finish (thread t takes t, t + 1024,
  // .., then the fixed tree), so every sum is the bits of a sw_finish of its own
  const uint32_t t = threadIdx.x;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t c = 0;
  for (uint32_t l = t; l < N; l += kClusterBlockThreads)
    if (label[l] == l) {
#pragma unroll
      for (uint32_t k = 0; k < 5; ++k) {
        const double S = (double)sum[k * section + l] * (1.0 / kSwFix);
        s[k] += S * S;
        if (k) sum[k * section + l] = 0;
      }
      ++c;
    }
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) {
    red[t] = s[k];
    if (k == 0) redc[t] = c;
    __syncthreads();
    for (uint32_t off = kClusterBlockThreads / 2; off > 0; off >>= 1) {
      if (t < off) {
        red[t] += red[t + off];
        if (k == 0) redc[t] += redc[t + off];
      }
      __syncthreads();
    }
    if (t == 0) {
      const double v = red[0] * (3.0 / (double)N);
      if (k) structure[2 * b + ((k - 1) >> 1)] += v;
      else if (improved) improved[b] += v;
      if (k == 0 && clusters) clusters[b] += redc[0];
    }
  }
}

// ---- chain plan: one workgroup per chain, all n_updates updates in one launch, labels, sums and a in LDS ------------------
// Thread t owns the vertices t, t + 1024, ..: it alone reads and writes their angles, update after update.  Bonds are drawn and
// united from the vertices that own links: every vertex its +i and +j link on the lattice; on a rotated level a lane with an E
// vertex makes two Philox calls and handles its four links, a lane with an O vertex makes none.
template <class Geometry>
__global__ void __launch_bounds__(kClusterBlockThreads)
    sigma_sw_chain_kernel(double2 *phi_all, Geometry g, double beta2, uint32_t n_updates, RngKey key0, uint32_t *flipped,
                          uint32_t *clusters, double *improved, uint32_t *status) {
  extern __shared__ double sw_lds[];
  __shared__ double red[kClusterBlockThreads];
  __shared__ uint32_t redc[kClusterBlockThreads];
  constexpr uint32_t NL = Geometry::kOwnedLinks;
  const uint32_t N = g.nvert(), owners = g.nowners(), b = blockIdx.x, t = threadIdx.x;
  double *a = sw_lds;
  long long *sum = (long long *)(a + N);
  uint32_t *parent = (uint32_t *)(sum + N);
  double2 *phi = phi_all + (size_t)b * N;
  const bool outputs = clusters || improved;
  RngKey key = key0;
  key.chain = key0.chain + b;
  uint32_t nflip = 0;
  bool capped = false;
  if constexpr (Geometry::kStructure) {
    // the weights of every position of both directions, once per launch, into this chain's table in the workspace: (cos, sin)
    // of position x of direction d at 2 (d M_0 + x).  Formed by sw_phase as everywhere; inside the update loop sincospi would
    // take the kernel beyond its 128 registers.  The barrier of the first update orders the table before its readers.
    const uint32_t M0 = g.extent(0), M1 = g.extent(1);
    double *table = g.weights + (size_t)b * 2 * (M0 + M1);
    for (uint32_t x = t; x < M0 + M1; x += kClusterBlockThreads) {
      const uint32_t d = x >= M0 ? 1u : 0u;
      double ws, wc;
      sw_phase(x - d * M0, d ? M1 : M0, ws, wc);
      table[2 * x] = wc;
      table[2 * x + 1] = ws;
    }
  }
  for (uint32_t n = 0; n < n_updates; ++n, ++key.step) {
    const V3 r = reflection_normal(key, P_SIGMA_SW_REFLECT);
    for (uint32_t l = t; l < N; l += kClusterBlockThreads) {
      a[l] = dot3(r, sigma_of(phi[l]));
      sum[l] = 0;
      parent[l] = l;
    }
    __syncthreads();
    for (uint32_t l = t; l < owners; l += kClusterBlockThreads) {
      uint32_t y[NL];
      g.far_ends(l, y);
      double ay[NL];
#pragma unroll
      for (uint32_t d = 0; d < NL; ++d) ay[d] = a[y[d]];
      const uint32_t bits = Geometry::bonds(key, l, a[l], ay, beta2);
#pragma unroll
      for (uint32_t d = 0; d < NL; ++d)
        if (bits & (1u << d)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent, l, y[d], N, capped);
    }
    __syncthreads();
    for (uint32_t l = t; l < N; l += kClusterBlockThreads) {
      // structure instance: the root is stored over the parent (a lane that reads the word meanwhile gets the old parent or the
      // root, both above it), so that the four passes below read it in one load.  A root stores itself over itself and no other
      // vertex can come to hold its own index, so parent[l] == l holds for the same l as before: sw_finish sees the same roots
      // and the same sums as the plain instance, and d_improved and d_clusters are its bits.
      const uint32_t root = uf_find<Geometry::kStructure ? __HIP_MEMORY_SCOPE_WORKGROUP : kUfPlain>(parent, l, N, capped);
      if constexpr (Geometry::kStructure) __hip_atomic_store(parent + l, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if constexpr (Geometry::kRoots) {                    // the improved correlator reads both from the workspace
        g.roots[(size_t)b * N + l] = root;
        g.qa[(size_t)b * N + l] = sw_fixed(a[l]);
      }
      if (improved) atomicAdd((unsigned long long *)(sum + root), (unsigned long long)sw_fixed(a[l]));
      if (!capped && sw_coin(key, root)) {
        phi[l] = reflected(sigma_of(phi[l]), a[l], r);
        ++nflip;
      }
    }
    __syncthreads();
    if constexpr (!Geometry::kStructure) {
      if (outputs) sw_finish(parent, sum, N, red, redc, improved ? improved + b : nullptr, clusters ? clusters + b : nullptr);
      __syncthreads();
    } else {
      // Pass 0 finishes the cluster sums as above.  Pass k = 1 + 2 d + (0: cos, 1: sin) takes the one slot per vertex again: zero,
      // add q(a w) onto the root's slot, finish into structure[b][d].  a is still the field's before the update, w comes from the
      // table; the trip counts are uniform (sw_add_combined shuffles).  One copy of the code serves the five passes.
      const double *table = g.weights + (size_t)b * 2 * (g.extent(0) + g.extent(1));
#pragma unroll 1
      for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t d = k ? (k - 1) >> 1 : 0;
        if (k > 0) {
          for (uint32_t l = t; l < N; l += kClusterBlockThreads) sum[l] = 0;
          __syncthreads();
#pragma unroll 1
          for (uint32_t base = 0; base < N; base += kClusterBlockThreads) {
            const uint32_t l = base + t;
            const bool active = l < N;
            const long long v[1] = {active ? sw_fixed(a[l] * table[2 * (d * g.extent(0) + g.position(l, d)) + ((k - 1) & 1u)]) : 0};
            sw_add_combined<__HIP_MEMORY_SCOPE_WORKGROUP>(sum, 0, active ? parent[l] : 0u, active, v);
          }
          __syncthreads();
        }
        if (k > 0 || outputs)
          sw_finish(parent, sum, N, red, redc, k ? g.structure + 2 * b + d : (improved ? improved + b : nullptr),
                    k || !clusters ? nullptr : clusters + b);
        __syncthreads();
      }
    }
  }
  if (flipped) {
    for (int off = kWave / 2; off > 0; off >>= 1) nflip += __shfl_down(nflip, off);
    if ((t & (kWave - 1)) == 0 && nflip) atomicAdd(flipped + b, nflip);
  }
  if (capped) atomicOr(status, 1u);
}

// ---- the improved correlator (mlmcpi_sigma_level_sw_correlator_draw) ------------------------------------------
// After an update of either plan the workspace holds a label array whose walk ends at every vertex's final root (tiled: the
// parents of launch 3; chain: the roots themselves) and q(a) of the field before the update.  Three launches follow, the same
// for both plans and both geometries, and every sum in them is an integer sum: no order matters.
//
// (1) one lane per vertex: q(a) onto P_C,d(x_d(l)) of the chain's table of either direction.  Every lane stays to the end.
template <class Geometry>
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_sum_kernel(Geometry g, uint32_t blocks, const uint32_t *label_all, const long long *qa_all, unsigned long long *table_all,
                              uint32_t lg, uint32_t *count_all, uint32_t *status) {
  const uint32_t N = g.nvert(), b = blockIdx.x / blocks, l = (blockIdx.x % blocks) * kClusterThreads + threadIdx.x;
  const bool active = l < N;
  bool capped = false;
  uint32_t root = 0;
  long long v = 0;
  if (active) {
    root = uf_find<kUfPlain>(label_all + (size_t)b * N, l, N, capped);
    v = qa_all[(size_t)b * N + l];
  }
#pragma unroll
  for (uint32_t d = 0; d < 2; ++d)
    sw_slice_add_combined(table_all + ((size_t)(2 * b + d) << (lg + 1)), lg, count_all + (size_t)(2 * b + d) * N, root,
                          active ? g.position(l, d) : 0u, active, v, capped);
  if (capped) atomicOr(status, 1u);
}

// (2) one lane per slot of the table of (chain, direction), kSwPairBatches slots in turn: an occupied slot (C, i, P) meets
// (C, (i + tau) mod M) for tau = 0 .. min(M / 2, w - 1), w the number of slices C occupies in that direction.  A larger lag finds
// nothing: a link changes the slice index by at most 1 on either geometry, so the slices of a cluster are an arc of the ring,
// and one that holds i and i + tau, tau <= M / 2, holds tau + 1 slices at least.  The term llrint(P P' 2^(s - 64)) (the product of
// the two integers in double, then the exact scale) goes onto acc[chain][direction][tau]: the lanes of a wave are added up
// first, the waves and batches of a workgroup meet in LDS for the lags below kSwPairLdsLags (where nearly every term falls:
// without that stage every wave of a chain sends its atomics to the same few words), and the workgroup sends one atomic per
// lag it holds; a lag beyond goes to the accumulator directly.  The loop over the lags runs to the wave's largest, so that its
// ballots and shuffles see all lanes.  Integer sums throughout: no order matters.
constexpr uint32_t kSwPairBatches = 16;    // slots a lane takes in turn
constexpr uint32_t kSwPairLdsLags = 128;   // lags a workgroup sums in LDS before it adds to the accumulator

__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_pair_kernel(const unsigned long long *table_all, uint32_t lg, const uint32_t *count_all, uint32_t N, uint32_t M0, uint32_t M1,
                               uint32_t blocks, double scale, long long *acc_all, uint32_t *status) {
  __shared__ long long part[kSwPairLdsLags];
  const uint32_t bd = blockIdx.x / blocks, d = bd & 1u, slot0 = (blockIdx.x % blocks) * (kClusterThreads * kSwPairBatches) + threadIdx.x;
  const uint32_t lane = threadIdx.x & (kWave - 1), M = d ? M1 : M0;
  const unsigned long long *table = table_all + ((size_t)bd << (lg + 1));
  long long *acc = acc_all + (size_t)(bd >> 1) * (M0 / 2 + M1 / 2 + 2) + (d ? M0 / 2 + 1 : 0);
  bool capped = false;
  if (threadIdx.x < kSwPairLdsLags) part[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t batch = 0; batch < kSwPairBatches; ++batch) {
    const uint32_t slot = slot0 + batch * kClusterThreads;
    const unsigned long long key = slot < (1u << lg) ? table[2 * (size_t)slot] : 0ull;
    const uint32_t root = (uint32_t)(key >> 32), i = (uint32_t)key - 1u;
    uint32_t ntau = 0;
    long long Pq = 0;
    if (key) {
      const uint32_t w = count_all[(size_t)bd * N + root];
      ntau = (w - 1u < M / 2 ? w - 1u : M / 2) + 1u;
      Pq = (long long)table[2 * (size_t)slot + 1];
    }
    const double P = (double)Pq;
    uint32_t tmax = ntau;
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)tmax, off);
      tmax = o > tmax ? o : tmax;
    }
    for (uint32_t tau = 0; tau < tmax; ++tau) {
      long long term = 0;
      if (tau < ntau) {
        uint32_t k = i + tau;
        if (k >= M) k -= M;
        const long long Q = tau ? sw_slice_lookup(table, lg, root, k, capped) : Pq;
        term = llrint((P * (double)Q) * scale);
      }
      const unsigned long long m = __ballot(term != 0);
      if (!m) continue;
      if (__builtin_popcountll(m) > 1) {
        for (int off = kWave / 2; off > 0; off >>= 1) term += __shfl_xor(term, off);
        if (lane != (uint32_t)__builtin_ctzll(m)) term = 0;
      }
      if (term) {
        if (tau < kSwPairLdsLags) __hip_atomic_fetch_add(part + tau, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(acc + tau, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kSwPairLdsLags && threadIdx.x <= M / 2 && part[threadIdx.x])
    __hip_atomic_fetch_add(acc + threadIdx.x, part[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (capped) atomicOr(status, 1u);
}

// (3) one lane per (chain, lag): corr[b][k] += (acc 2^-s) 3 / N
__global__ void __launch_bounds__(kClusterThreads)
    sigma_sw_slice_finish_kernel(const long long *acc_all, uint32_t total, double inv_scale, double three_over_n, double *corr) {
  const uint32_t k = blockIdx.x * kClusterThreads + threadIdx.x;
  if (k < total) corr[k] += ((double)acc_all[k] * inv_scale) * three_over_n;
}

namespace {

struct SwPlan {
  bool ok, chain;
  uint32_t W, H, ntx, nty;                // tiled: tile extents (vertices; on a rotated level cells), tiles per direction
  uint32_t merge_blocks, resolve_blocks;  // tiled: workgroups per chain of launches 2 and 3
  size_t lds_bytes;                       // dynamic LDS of the chain kernel / of launch 1
};

// what the tiled plan asks of a geometry: the plane the tiles divide, the default tile, the crossing links of launch 2 and the
// LDS of launch 1.
// Unrotated: tiles of 64 x 32 vertices; a tile holds a of its vertices and of the +i / +j halo, the parents and the bond bits.
inline void sw_tiling(const LatticeGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H) { pw = g.Mt, ph = g.Mx, W = 64, H = 32; }
inline uint32_t sw_crossing(const LatticeGeometry &g, const SwPlan &p) { return p.ntx * g.Mx + p.nty * g.Mt; }
inline size_t sw_tile_lds(const LatticeGeometry &, uint32_t W, uint32_t H) {
  return (size_t)(W + 1) * (H + 1) * sizeof(double) + (size_t)W * H * (sizeof(uint32_t) + sizeof(uint8_t));
}
// Rotated: default tile 32 x 32 cells, by LDS arithmetic and not by a timing sweep: a tile of W x H cells takes 25 W H + 8 (W + H
// + 1) B (sw_rot_tile_lds), so 32 x 32 takes 26 120 B = 25.5 KiB and six workgroups of four waves share the 160 KiB of a CU (24 of
// its 32 wave slots); it holds 2048 vertices, as the 64 x 32 vertex tile of the unrotated default does, the halo is 65 / 1024 =
// 6 % of the cells read, and among the tiles of that area the square one has the fewest crossing links (2 W + 2 H - 1 = 127 of
// 4096).  64 x 64 cells take 101 KiB: one workgroup per CU, and the attribute of sw_init_attrs.
inline void sw_tiling(const RotatedGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H) { pw = g.ht, ph = g.hx, W = 32, H = 32; }
inline uint32_t sw_crossing(const RotatedGeometry &g, const SwPlan &p) { return 2 * p.ntx * g.hx + 2 * p.nty * g.ht; }
inline size_t sw_tile_lds(const RotatedGeometry &, uint32_t W, uint32_t H) { return sw_rot_tile_lds(W, H); }

// Launch plan; it chooses and calls nothing.  The chain plan where a chain fits its LDS bound and one
// workgroup per chain fills the device (B >= kComputeUnits: a chain's workgroup is 16 waves and takes more than half a CU's
// LDS, so one is resident per CU), the tiled plan otherwise.  Knobs (bit-identical results): MLMCPI_SIGMA_SW_PLAN=chain|tiled,
// MLMCPI_SIGMA_SW_TILE=WxH (vertices; on a rotated level cells).  ok = false: the chain plan was forced beyond its bound.
template <class Geometry>
SwPlan sw_plan(const Geometry &g, uint32_t B, const Tuning &tune) {
  SwPlan p{};
  const uint32_t N = g.nvert();
  uint32_t pw, ph;
  sw_tiling(g, pw, ph, p.W, p.H);
  p.chain = tune.sigma_sw_plan ? tune.sigma_sw_plan == 1 : (N <= kSwChainMaxN && B >= kComputeUnits);
  p.ok = !p.chain || N <= kSwChainMaxN;
  if (tune.sigma_sw_tile_w) p.W = tune.sigma_sw_tile_w;
  if (tune.sigma_sw_tile_h) p.H = tune.sigma_sw_tile_h;
  p.ntx = (pw + p.W - 1) / p.W;
  p.nty = (ph + p.H - 1) / p.H;
  p.merge_blocks = (sw_crossing(g, p) + kClusterThreads - 1) / kClusterThreads;
  p.resolve_blocks = (N + kClusterThreads - 1) / kClusterThreads;
  p.lds_bytes = p.chain ? (size_t)N * kSwChainBytesPerVertex : sw_tile_lds(g, p.W, p.H);
  return p;
}

std::mutex g_sw_attr_mutex;
bool g_sw_attr_set[64] = {false};

// dynamic LDS above 64 KiB: the chain kernels up to their bound, the rotated launch 1 at the largest tile
int sw_init_attrs() {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(MLMCPI_ERR_INVALID, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_sw_attr_mutex);
  if (g_sw_attr_set[dev]) return MLMCPI_OK;
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<LatticeGeometry>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<RotatedGeometry>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<WithStructure<LatticeGeometry>>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<WithStructure<RotatedGeometry>>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<WithRoots<LatticeGeometry>>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_sw_chain_kernel<WithRoots<RotatedGeometry>>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kSwChainMaxN * kSwChainBytesPerVertex));
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sw_bond_label_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)sw_rot_tile_lds(kSwMaxTile, kSwMaxTile)));
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

// workspace sections: status word (256 B), label [B N] uint32, q(a) [B N] int64, cluster sums [B N] int64, bond bits [B owners]
// uint8 (two bits per vertex; on a rotated level four bits per E vertex).  With structure sums four more [B N] int64 sections
// follow the cluster sums (slot k of a root is k sections behind its cluster sum), before the bond bits.  The chain plan uses
// the status word only; with structure sums it also keeps its table of weights, 16 (M_0 + M_1) B per chain, from the start of the
// q(a) section on (sw_chain_table: the six int64 sections are contiguous, 48 B per vertex and chain, and 3 N >= M_0 + M_1).
constexpr uint32_t kSwStructureSlots = 4;
constexpr size_t kSwStatusBytes = 256;
size_t sw_section_label(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(uint32_t)); }
size_t sw_section_fixed(uint32_t N, uint32_t B) { return align256((size_t)B * N * sizeof(long long)); }
size_t sw_section_bits(uint32_t owners, uint32_t B) { return align256((size_t)B * owners); }
inline double *sw_chain_table(void *d_work, uint32_t N, uint32_t B) { return (double *)((char *)d_work + kSwStatusBytes + sw_section_label(N, B)); }
template <class Geometry>
size_t sw_workspace(const Geometry &g, uint32_t B, bool structure = false) {
  return kSwStatusBytes + sw_section_label(g.nvert(), B) + (2 + (structure ? kSwStructureSlots : 0)) * sw_section_fixed(g.nvert(), B) +
         sw_section_bits(g.nowners(), B);
}

// The improved correlator's part of the workspace, behind that of the plain draw: the tables [B][2][2^lg] of 16 B slots, the
// occupied-slice counts [B][2][N] uint32 and the accumulators [B][n_out] int64, contiguous, cleared by one memset per update.
// lg: the smallest with 2^lg >= 2 N.  s: the fixed-point scale of the accumulators, min(32, 62 - ceil(log2(N N_slice))) with
// N_slice = N / min(M_0, M_1) the vertices of the larger slice: sum_i sum_C |P(i)| |P(i + tau)| <= sum_i N_slice sum_C n_C(i)
// = N N_slice (|a| <= 1, n_C(i) the vertices of C in slice i), so |acc| <= 2^62 + N / 2 with the roundings of the terms.
struct SwCorr {
  double *corr;
  uint32_t lg, n_out, s;
  size_t table_bytes, count_bytes, acc_bytes;
  size_t bytes() const { return table_bytes + count_bytes + acc_bytes; }
};

template <class Geometry>
SwCorr sw_corr(const Geometry &g, uint32_t B, double *d_corr) {
  SwCorr c{};
  const uint32_t N = g.nvert(), M0 = g.extent(0), M1 = g.extent(1);
  c.corr = d_corr;
  c.lg = 1;
  while ((1ull << c.lg) < 2ull * N) ++c.lg;
  c.n_out = M0 / 2 + M1 / 2 + 2;
  const uint64_t bound = (uint64_t)N * (N / (M0 < M1 ? M0 : M1));
  uint32_t lb = 0;
  while ((1ull << lb) < bound) ++lb;
  c.s = 62 - lb < 32 ? 62 - lb : 32;
  c.table_bytes = align256(((size_t)2 * B << c.lg) * 16);
  c.count_bytes = align256((size_t)2 * B * N * sizeof(uint32_t));
  c.acc_bytes = align256((size_t)B * c.n_out * sizeof(long long));
  return c;
}

// the three launches of the improved correlator for the update whose roots and q(a) the workspace holds
template <class Geometry>
int sw_corr_update(const Geometry &g, const SwPlan &p, const SwCorr &c, uint32_t B, const uint32_t *label, const long long *qa, char *extra,
                   uint32_t *status, hipStream_t st) {
  const uint32_t N = g.nvert();
  unsigned long long *table = (unsigned long long *)extra;
  uint32_t *count = (uint32_t *)(extra + c.table_bytes);
  long long *acc = (long long *)(extra + c.table_bytes + c.count_bytes);
  MLMCPI_HIP_TRY(hipMemsetAsync(extra, 0, c.bytes(), st));
  hipLaunchKernelGGL(sigma_sw_slice_sum_kernel<Geometry>, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st, g, p.resolve_blocks, label,
                     qa, table, c.lg, count, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_sum_kernel");
  const uint32_t pair_blocks = ((1u << c.lg) + kClusterThreads * kSwPairBatches - 1) / (kClusterThreads * kSwPairBatches);
  hipLaunchKernelGGL(sigma_sw_slice_pair_kernel, dim3(2 * B * pair_blocks), dim3(kClusterThreads), 0, st, (const unsigned long long *)table,
                     c.lg, (const uint32_t *)count, N, g.extent(0), g.extent(1), pair_blocks, ldexp(1.0, (int)c.s - 64), acc, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_pair_kernel");
  const uint32_t total = B * c.n_out;
  hipLaunchKernelGGL(sigma_sw_slice_finish_kernel, dim3((total + kClusterThreads - 1) / kClusterThreads), dim3(kClusterThreads), 0, st,
                     (const long long *)acc, total, ldexp(1.0, -(int)c.s), 3.0 / (double)N, c.corr);
  MLMCPI_LAUNCH_CHECK("sigma_sw_slice_finish_kernel");
  return MLMCPI_OK;
}

// launches 1 and 2 of the tiled plan, one pair per geometry: the lattice's take its extents, the rotated level's the level
int sw_front_end(const LatticeGeometry &g, const SwPlan &p, const double2 *phi, double beta2, const RngKey &key, uint32_t B, uint32_t *label,
                 uint8_t *bits, long long *qa, long long *sum, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(sigma_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kClusterThreads), p.lds_bytes, st, phi, g.Mt, g.Mx, beta2,
                     key, p.W, p.H, p.ntx, p.nty, label, bits, qa, sum, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_bond_label_kernel");
  hipLaunchKernelGGL(sigma_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kClusterThreads), 0, st, g.Mt, g.Mx, p.W, p.H, p.ntx, p.nty,
                     p.merge_blocks, label, bits, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_merge_kernel");
  return MLMCPI_OK;
}

int sw_front_end(const SigmaLevel &L, const SwPlan &p, const double2 *phi, double beta2, const RngKey &key, uint32_t B, uint32_t *label,
                 uint8_t *bits, long long *qa, long long *sum, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(sigma_rot_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kClusterThreads), p.lds_bytes, st, phi, L, beta2, key,
                     p.W, p.H, p.ntx, p.nty, label, bits, qa, sum, status);
  MLMCPI_LAUNCH_CHECK("sigma_rot_sw_bond_label_kernel");
  hipLaunchKernelGGL(sigma_rot_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kClusterThreads), 0, st, L, p.W, p.H, p.ntx, p.nty,
                     p.merge_blocks, label, bits, status);
  MLMCPI_LAUNCH_CHECK("sigma_rot_sw_merge_kernel");
  return MLMCPI_OK;
}

// the draw on either geometry, arguments checked: the workspace laid out, the launches issued, the status word read back.
// `front` is what sw_front_end takes for this geometry, `what` the entry point, `where` the noun ("lattice", "level") of its
// messages and `chain_kernel` the name of the chain kernel's instance in a launch error.  d_structure != NULL: the structure
// instances of the kernels and the larger workspace (the caller has checked its size).
template <class Geometry, class Front>
int sw_draw(const Geometry &g, const Front &front, double beta, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed, uint32_t chain0, uint32_t update0,
            uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved, double *d_structure, void *d_work, void *stream, const char *what,
            const char *where, const char *chain_kernel, double *d_corr = nullptr) {
  const uint32_t N = g.nvert();
  const SwPlan p = sw_plan(g, B, tuning());
  if (!p.ok)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s: MLMCPI_SIGMA_SW_PLAN=chain holds a chain of at most %u vertices in LDS, this %s has %u", what,
                kSwChainMaxN, where, N);
  const uint64_t widest = (uint64_t)B * (p.ntx * p.nty > p.resolve_blocks ? p.ntx * p.nty : p.resolve_blocks);
  MLMCPI_REQUIRE(p.chain || (widest < (1ull << 31) && (uint64_t)B * p.merge_blocks < (1ull << 31)), "too many workgroups for one launch: split the batch");
  // d_corr != NULL (never with d_structure): the improved correlator's launches after every update, its workspace behind the plain draw's
  const SwCorr corr = sw_corr(g, B, d_corr);
  MLMCPI_REQUIRE(!d_corr || ((uint64_t)B * p.resolve_blocks < (1ull << 31) && ((uint64_t)2 * B << corr.lg) / kClusterThreads < (1ull << 31) &&
                             (uint64_t)B * corr.n_out < (1ull << 31)),
                 "too many workgroups for one launch: split the batch");
  if (n_updates == 0) return MLMCPI_OK;
  if (int rc = sw_init_attrs()) return rc;
  char *w = (char *)d_work;
  uint32_t *status = (uint32_t *)w;
  uint32_t *label = (uint32_t *)(w + kSwStatusBytes);
  long long *qa = (long long *)(w + kSwStatusBytes + sw_section_label(N, B));
  long long *sum = (long long *)(w + kSwStatusBytes + sw_section_label(N, B) + sw_section_fixed(N, B));
  uint8_t *bits = (uint8_t *)(w + kSwStatusBytes + sw_section_label(N, B) + (2 + (d_structure ? kSwStructureSlots : 0)) * sw_section_fixed(N, B));
  const size_t section = d_structure ? sw_section_fixed(N, B) / sizeof(long long) : 0;
  // the room of sw_chain_table (it holds on every level: both extents are even and >= 2)
  MLMCPI_REQUIRE(!d_structure || (uint64_t)3 * N >= (uint64_t)g.extent(0) + g.extent(1), "the table of weights does not fit the workspace");
  const hipStream_t st = as_stream(stream);
  const double beta2 = 2.0 * beta;
  char *extra = w + sw_workspace(g, B);
  MLMCPI_HIP_TRY(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
  if (p.chain && d_corr) {
    // one update per launch (the same bits as one launch of all: the call-split property), its roots and q(a) left in the workspace
    for (uint32_t k = 0; k < n_updates; ++k) {
      hipLaunchKernelGGL(sigma_sw_chain_kernel<WithRoots<Geometry>>, dim3(B), dim3(kClusterBlockThreads), p.lds_bytes, st, (double2 *)d_phi,
                         WithRoots<Geometry>(g, label, qa), beta2, 1u, make_key(seed, chain0, update0 + k), d_flipped, d_clusters, d_improved,
                         status);
      MLMCPI_LAUNCH_CHECK(chain_kernel);
      if (int rc = sw_corr_update(g, p, corr, B, label, qa, extra, status, st)) return rc;
    }
  } else if (p.chain && d_structure) {
    hipLaunchKernelGGL(sigma_sw_chain_kernel<WithStructure<Geometry>>, dim3(B), dim3(kClusterBlockThreads), p.lds_bytes, st, (double2 *)d_phi,
                       WithStructure<Geometry>(g, d_structure, sw_chain_table(d_work, N, B)), beta2, n_updates, make_key(seed, chain0, update0), d_flipped, d_clusters,
                       d_improved, status);
    MLMCPI_LAUNCH_CHECK(chain_kernel);
  } else if (p.chain) {
    hipLaunchKernelGGL(sigma_sw_chain_kernel<Geometry>, dim3(B), dim3(kClusterBlockThreads), p.lds_bytes, st, (double2 *)d_phi, g, beta2,
                       n_updates, make_key(seed, chain0, update0), d_flipped, d_clusters, d_improved, status);
    MLMCPI_LAUNCH_CHECK(chain_kernel);
  } else {
    const bool outputs = d_clusters || d_improved;
    // the bond + label kernels zero the cluster sum of every vertex and are the ones of the plain draw; the four structure slots
    // are zeroed here once, and after every update by the finish kernel at the roots it has read (nothing else was added to)
    if (d_structure) MLMCPI_HIP_TRY(hipMemsetAsync(sum + section, 0, kSwStructureSlots * sw_section_fixed(N, B), st));
    for (uint32_t k = 0; k < n_updates; ++k) {
      const RngKey key = make_key(seed, chain0, update0 + k);
      if (int rc = sw_front_end(front, p, (const double2 *)d_phi, beta2, key, B, label, bits, qa, d_improved || d_structure ? sum : nullptr, status, st))
        return rc;
      if (d_structure) {
        hipLaunchKernelGGL(sigma_sw_resolve_structure_kernel<Geometry>, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st,
                           (double2 *)d_phi, g, key, p.resolve_blocks, label, qa, sum, section, d_flipped, status);
        MLMCPI_LAUNCH_CHECK("sigma_sw_resolve_structure_kernel");
        hipLaunchKernelGGL(sigma_sw_finish_structure_kernel, dim3(B), dim3(kClusterBlockThreads), 0, st, label, sum, section, N, d_improved,
                           d_clusters, d_structure);
        MLMCPI_LAUNCH_CHECK("sigma_sw_finish_structure_kernel");
        continue;
      }
      hipLaunchKernelGGL(sigma_sw_resolve_kernel, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st, (double2 *)d_phi, N, key,
                         p.resolve_blocks, label, qa, d_improved ? sum : nullptr, d_flipped, status);
      MLMCPI_LAUNCH_CHECK("sigma_sw_resolve_kernel");
      if (outputs) {
        hipLaunchKernelGGL(sigma_sw_finish_kernel, dim3(B), dim3(kClusterBlockThreads), 0, st, label, sum, N, d_improved, d_clusters);
        MLMCPI_LAUNCH_CHECK("sigma_sw_finish_kernel");
      }
      if (d_corr)
        if (int rc = sw_corr_update(g, p, corr, B, label, qa, extra, status, st)) return rc;
    }
  }
  // a find or union loop that ran into its cap (it cannot, by the argument of sigma_cluster_device.hpp): an error, never a hang
  uint32_t h_status = 0;
  MLMCPI_HIP_TRY(hipMemcpyAsync(&h_status, status, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  MLMCPI_HIP_TRY(hipStreamSynchronize(st));
  if (h_status) return fail(MLMCPI_ERR_HIP, "%s: a labelling loop reached its iteration cap (status %u); the state is undefined", what, h_status);
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_sw_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_workspace_bytes")) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  *bytes = sw_workspace(LatticeGeometry{act->Mt, act->Mx}, B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_sw_draw(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint32_t n_updates, uint64_t seed, uint32_t chain0,
                         uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved, void *d_work, void *stream) {
  if (int rc = sw_check(act, "mlmcpi_sigma_sw_draw")) return rc;
  MLMCPI_REQUIRE(d_phi && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  const LatticeGeometry g{act->Mt, act->Mx};
  return sw_draw(g, g, act->beta, d_phi, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, nullptr, d_work, stream,
                 "mlmcpi_sigma_sw_draw", "lattice", "sigma_sw_chain_kernel");
}

int mlmcpi_sigma_level_sw_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    return mlmcpi_sigma_sw_workspace_bytes(&act, B, bytes);
  }
  *bytes = sw_workspace(RotatedGeometry(make_level(*level)), B);
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_sw_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                               uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                               void *d_work, void *stream) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    return mlmcpi_sigma_sw_draw(&act, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, d_work, stream);
  }
  const SigmaLevel L = make_level(*level);
  return sw_draw(RotatedGeometry(L), L, level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved,
                 nullptr, d_work, stream, "mlmcpi_sigma_level_sw_draw", "level", "sigma_rot_sw_chain_kernel");
}

int mlmcpi_sigma_level_sw_structure_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    if (int rc = sw_check(&act, "mlmcpi_sigma_level_sw_structure_workspace_bytes")) return rc;
    *bytes = sw_workspace(LatticeGeometry{act.Mt, act.Mx}, B, true);
  } else {
    *bytes = sw_workspace(RotatedGeometry(make_level(*level)), B, true);
  }
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_sw_structure_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                                         uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                                         double *d_structure, void *d_work, size_t work_bytes, void *stream) {
  size_t need = 0;
  if (int rc = mlmcpi_sigma_level_sw_structure_workspace_bytes(level, B ? B : 1, &need)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE(d_structure, "d_structure is NULL: mlmcpi_sigma_level_sw_draw is the entry point without structure sums");
  MLMCPI_REQUIRE(work_bytes >= need, "the workspace is smaller than mlmcpi_sigma_level_sw_structure_workspace_bytes asks for");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  const char *what = "mlmcpi_sigma_level_sw_structure_draw";
  if (!level->rotated) {
    const LatticeGeometry g{level->Mt, level->Mx};
    return sw_draw(g, g, level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, d_structure, d_work,
                   stream, what, "level", "sigma_sw_chain_kernel (structure)");
  }
  const SigmaLevel L = make_level(*level);
  return sw_draw(RotatedGeometry(L), L, level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved,
                 d_structure, d_work, stream, what, "level", "sigma_rot_sw_chain_kernel (structure)");
}

int mlmcpi_sigma_level_sw_correlator_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = check_cluster_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  if (!level->rotated) {
    const mlmcpi_lattice_action act = level_as_lattice(level);
    if (int rc = sw_check(&act, "mlmcpi_sigma_level_sw_correlator_workspace_bytes")) return rc;
    const LatticeGeometry g{act.Mt, act.Mx};
    *bytes = sw_workspace(g, B) + sw_corr(g, B, nullptr).bytes();
  } else {
    const RotatedGeometry g(make_level(*level));
    *bytes = sw_workspace(g, B) + sw_corr(g, B, nullptr).bytes();
  }
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_sw_correlator_draw(const mlmcpi_sigma_level *level, double *d_state, uint32_t B, uint32_t n_updates, uint64_t seed,
                                          uint32_t chain0, uint32_t update0, uint32_t *d_flipped, uint32_t *d_clusters, double *d_improved,
                                          double *d_corr, void *d_work, size_t work_bytes, void *stream) {
  size_t need = 0;
  if (int rc = mlmcpi_sigma_level_sw_correlator_workspace_bytes(level, B ? B : 1, &need)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE(d_corr, "d_corr is NULL: mlmcpi_sigma_level_sw_draw is the entry point without the improved correlator");
  MLMCPI_REQUIRE(work_bytes >= need, "the workspace is smaller than mlmcpi_sigma_level_sw_correlator_workspace_bytes asks for");
  MLMCPI_REQUIRE((uint64_t)update0 + n_updates <= 0xFFFFFFFFull, "update counter overflows");
  const char *what = "mlmcpi_sigma_level_sw_correlator_draw";
  if (!level->rotated) {
    const LatticeGeometry g{level->Mt, level->Mx};
    return sw_draw(g, g, level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved, nullptr, d_work,
                   stream, what, "level", "sigma_sw_chain_kernel (roots)", d_corr);
  }
  const SigmaLevel L = make_level(*level);
  return sw_draw(RotatedGeometry(L), L, level->beta, d_state, B, n_updates, seed, chain0, update0, d_flipped, d_clusters, d_improved,
                 nullptr, d_work, stream, what, "level", "sigma_rot_sw_chain_kernel (roots)", d_corr);
}

}  // extern "C"
