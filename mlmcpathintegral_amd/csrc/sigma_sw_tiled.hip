// sigma_sw_tiled.hip -- the tiled plan of the Swendsen-Wang update of the O(3) nonlinear sigma model (sigma_sw.hip has the
// update, the RNG contract and the plan that chooses between this and the chain plan of sigma_sw_chain.hip): three or four
// launches per update, on the unrotated lattice and on the rotated level.  The two tile front ends (bond + label, merge) are
// written once per geometry (sigma_cluster_device.hpp says why), the resolve and finish kernels use none or are instantiated
// on it.
//
// On a rotated level (tests/sigma_level_sw_model.py) the same update with the level's indices: n = Mt Mx / 2 vertices, plane E then
// plane O, the 2 n links named (e, d) from their E end (sigma_cluster_device.hpp), the root of a cluster its smallest LEVEL
// index (also when the cluster is a lone O vertex), P_SIGMA_SW_BOND at site e, sub d >> 1: u decides link (e, d) for d even, v
// for d odd.  union(x, x) returns at once (level (2, 2): the four links of E(0, 0) all end at O(0, 0)).
//
// Improved estimator.  With A_C the sum of a_l over cluster C, 3 sum_C A_C^2 / N is an unbiased estimator of chi_m = <|M|^2> / N
// (the mean of (M . r)^2 over the coins is sum_C A_C^2, the mean over r is |M|^2 / 3).  A_C is summed in 64-bit fixed point,
// q(a) = llrint(a 2^32), with integer atomic adds on the root's slot (N <= 2^30 keeps it inside 63 bits), and (A_C 2^-32)^2 is
// summed over the roots by sw_finish: one workgroup of 1024 threads, thread t takes the vertices t, t + 1024, .. in ascending
// order, then a fixed tree.  That sum is the same bits under every plan, and it is ADDED to the caller's accumulator update by
// update, so that 10 updates equal 5 + 5 to the bit.
//
// Improved structure factor (mlmcpi_sigma_level_sw_structure_draw): per cluster and direction d the two sums
// of q(a_l w), w = cos, sin of 2 pi x_d(l) / M_d from sw_phase, on four further root slots; each is finished as A_C is and added
// to structure[b][d], cos then sin.  The structure instances: sigma_sw_resolve_structure_kernel<Geometry>,
// sigma_sw_finish_structure_kernel (and sigma_sw_chain_kernel<WithStructure<Geometry>>); the instances of the plain draw are
// untouched.
//
// Labelling: the parent array and the union by atomic min of sigma_sw_device.hpp (uf_*), where its termination argument is
// written out.
#include "sigma_sw_host.hpp"

#include "sigma_sw_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

constexpr uint32_t kSwMaxTile = 64;          // the largest tile extent MLMCPI_SIGMA_SW_TILE admits, in cells

// rotated level, launch 1: a of the tile's E cells [W H], a of its O cells and their -a / -b halo [(W + 1)(H + 1)], the parents
// [2 W H] uint32, the bond bits [W H] uint8
__host__ __device__ constexpr size_t sw_rot_tile_lds(uint32_t W, uint32_t H) {
  return ((size_t)W * H + (size_t)(W + 1) * (H + 1)) * sizeof(double) + (size_t)2 * W * H * sizeof(uint32_t) + (size_t)W * H;
}

// ---- launch 1: bonds of the tile's vertices, union-find on the tile's interior links in LDS -------------------------------------
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

// ---- host ---------------------------------------------------------------------------------------------------------------------
// Unrotated: tiles of 64 x 32 vertices; a tile holds a of its vertices and of the +i / +j halo, the parents and the bond bits.
void sw_tiling(const LatticeGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H) { pw = g.Mt, ph = g.Mx, W = 64, H = 32; }
uint32_t sw_crossing(const LatticeGeometry &g, const SwPlan &p) { return p.ntx * g.Mx + p.nty * g.Mt; }
size_t sw_tile_lds(const LatticeGeometry &, uint32_t W, uint32_t H) {
  return (size_t)(W + 1) * (H + 1) * sizeof(double) + (size_t)W * H * (sizeof(uint32_t) + sizeof(uint8_t));
}
// Rotated: default tile 32 x 32 cells, by LDS arithmetic and not by a timing sweep: a tile of W x H cells takes 25 W H + 8 (W + H
// + 1) B (sw_rot_tile_lds), so 32 x 32 takes 26 120 B = 25.5 KiB and six workgroups of four waves share the 160 KiB of a CU (24 of
// its 32 wave slots); it holds 2048 vertices, as the 64 x 32 vertex tile of the unrotated default does, the halo is 65 / 1024 =
// 6 % of the cells read, and among the tiles of that area the square one has the fewest crossing links (2 W + 2 H - 1 = 127 of
// 4096).  64 x 64 cells take 101 KiB: one workgroup per CU, and the attribute of sw_tiled_init_attrs.
void sw_tiling(const RotatedGeometry &g, uint32_t &pw, uint32_t &ph, uint32_t &W, uint32_t &H) { pw = g.ht, ph = g.hx, W = 32, H = 32; }
uint32_t sw_crossing(const RotatedGeometry &g, const SwPlan &p) { return 2 * p.ntx * g.hx + 2 * p.nty * g.ht; }
size_t sw_tile_lds(const RotatedGeometry &, uint32_t W, uint32_t H) { return sw_rot_tile_lds(W, H); }

// dynamic LDS above 64 KiB: the rotated launch 1 at the largest tile
int sw_tiled_init_attrs() {
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)sigma_rot_sw_bond_label_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)sw_rot_tile_lds(kSwMaxTile, kSwMaxTile)));
  return MLMCPI_OK;
}

namespace {

// launches 1 and 2, one pair per geometry: the lattice's take its extents, the rotated level's the level
int sw_front_end(const LatticeGeometry &g, const SwPlan &p, const double2 *phi, double beta, const RngKey &key, uint32_t B, uint32_t *label,
                 uint8_t *bits, long long *qa, long long *sum, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(sigma_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kClusterThreads), p.lds_bytes, st, phi, g.Mt, g.Mx, 2.0 * beta,
                     key, p.W, p.H, p.ntx, p.nty, label, bits, qa, sum, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_bond_label_kernel");
  hipLaunchKernelGGL(sigma_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kClusterThreads), 0, st, g.Mt, g.Mx, p.W, p.H, p.ntx, p.nty,
                     p.merge_blocks, label, bits, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_merge_kernel");
  return MLMCPI_OK;
}

// L: the level the RotatedGeometry was built from, what make_level gives for it (a rotated level has even extents, so 2 ht and
// 2 hx are its Mt and Mx)
int sw_front_end(const RotatedGeometry &g, const SwPlan &p, const double2 *phi, double beta, const RngKey &key, uint32_t B, uint32_t *label,
                 uint8_t *bits, long long *qa, long long *sum, uint32_t *status, hipStream_t st) {
  const SigmaLevel L{2 * g.ht, 2 * g.hx, g.ht, g.hx, g.q, 1, beta};
  hipLaunchKernelGGL(sigma_rot_sw_bond_label_kernel, dim3(B * p.ntx * p.nty), dim3(kClusterThreads), p.lds_bytes, st, phi, L, 2.0 * beta, key,
                     p.W, p.H, p.ntx, p.nty, label, bits, qa, sum, status);
  MLMCPI_LAUNCH_CHECK("sigma_rot_sw_bond_label_kernel");
  hipLaunchKernelGGL(sigma_rot_sw_merge_kernel, dim3(B * p.merge_blocks), dim3(kClusterThreads), 0, st, L, p.W, p.H, p.ntx, p.nty,
                     p.merge_blocks, label, bits, status);
  MLMCPI_LAUNCH_CHECK("sigma_rot_sw_merge_kernel");
  return MLMCPI_OK;
}

}  // namespace

// The bond + label kernels zero the cluster sum of every vertex and are the ones of the plain draw; the four structure slots
// are zeroed by the draw once, and after every update by the finish kernel at the roots it has read (nothing else was added to).
template <class Geometry>
int sw_tiled_update(const Geometry &g, const SwPlan &p, const SwWorkspace &ws, const SwRequest &r, const RngKey &key) {
  const uint32_t N = g.nvert(), B = r.B;
  const hipStream_t st = as_stream(r.stream);
  uint32_t *status = ws.status.in<uint32_t>(r.d_work), *label = ws.label.in<uint32_t>(r.d_work);
  long long *qa = ws.qa.in<long long>(r.d_work), *sum = ws.sum.in<long long>(r.d_work);
  if (int rc = sw_front_end(g, p, (const double2 *)r.d_phi, r.beta, key, B, label, ws.bits.in<uint8_t>(r.d_work), qa,
                            r.d_improved || r.d_structure ? sum : nullptr, status, st))
    return rc;
  if (r.d_structure) {
    hipLaunchKernelGGL(sigma_sw_resolve_structure_kernel<Geometry>, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st,
                       (double2 *)r.d_phi, g, key, p.resolve_blocks, label, qa, sum, ws.slot_stride(), r.d_flipped, status);
    MLMCPI_LAUNCH_CHECK("sigma_sw_resolve_structure_kernel");
    hipLaunchKernelGGL(sigma_sw_finish_structure_kernel, dim3(B), dim3(kClusterBlockThreads), 0, st, label, sum, ws.slot_stride(), N,
                       r.d_improved, r.d_clusters, r.d_structure);
    MLMCPI_LAUNCH_CHECK("sigma_sw_finish_structure_kernel");
    return MLMCPI_OK;
  }
  hipLaunchKernelGGL(sigma_sw_resolve_kernel, dim3(B * p.resolve_blocks), dim3(kClusterThreads), 0, st, (double2 *)r.d_phi, N, key,
                     p.resolve_blocks, label, qa, r.d_improved ? sum : nullptr, r.d_flipped, status);
  MLMCPI_LAUNCH_CHECK("sigma_sw_resolve_kernel");
  if (r.d_clusters || r.d_improved) {
    hipLaunchKernelGGL(sigma_sw_finish_kernel, dim3(B), dim3(kClusterBlockThreads), 0, st, label, sum, N, r.d_improved, r.d_clusters);
    MLMCPI_LAUNCH_CHECK("sigma_sw_finish_kernel");
  }
  return MLMCPI_OK;
}

template int sw_tiled_update<LatticeGeometry>(const LatticeGeometry &, const SwPlan &, const SwWorkspace &, const SwRequest &, const RngKey &);
template int sw_tiled_update<RotatedGeometry>(const RotatedGeometry &, const SwPlan &, const SwWorkspace &, const SwRequest &, const RngKey &);

}  // namespace mlmcpi
