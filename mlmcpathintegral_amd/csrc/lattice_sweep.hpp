// lattice_sweep.hpp -- what the units of the 2-D sweep path share: lattice2d.hip (the launch plan and its executor),
// schwinger_sweeps.hip, gff_sweeps.hip and sigma2d.hip (each action's sweep kernels and their launcher).
// The device helpers both tile kernels use; the geometry the planner and the kernels agree on, each size defined once; and the
// launcher interface, one function per action.
#pragma once
#include <type_traits>

#include "internal.hpp"
#include "site_update.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- device helpers of the tile kernels ------------------------------------------------------------------------------------
// linear iteration of a workgroup over an nr x nc region without per-element division
template <int NT, class F>
__device__ __forceinline__ void for_region(uint32_t nr, uint32_t nc, F f) {
  const uint32_t total = nr * nc;
  uint32_t idx = threadIdx.x;
  if (idx >= total) return;
  uint32_t ri = idx / nc, ci = idx - ri * nc;
  uint32_t dr = NT / nc, dc = NT - dr * nc;
  for (; idx < total; idx += NT) {
    f(ri, ci);
    ri += dr;
    ci += dc;
    if (ci >= nc) {
      ci -= nc;
      ++ri;
    }
  }
}

// Staging loop for global -> LDS: the same traversal as for_region, but UNR independent loads are
// issued back to back before any of them is consumed, so a thread has UNR HBM requests in flight
// instead of one (a rolled load -> wait -> ds_write loop is latency bound: ~10 dependent round
// trips per tile).
template <int NT, int UNR, class T, class Load, class Store>
__device__ __forceinline__ void stage_region(uint32_t nr, uint32_t nc, Load load, Store store) {
  const uint32_t total = nr * nc;
  uint32_t idx = threadIdx.x;
  uint32_t ri = idx / nc, ci = idx - ri * nc;
  const uint32_t dr = NT / nc, dc = NT - dr * nc;
  while (idx < total) {
    T v[UNR];
    uint32_t rr[UNR], cc[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      rr[u] = ri;
      cc[u] = ci;
      if (idx + u * NT < total) v[u] = load(ri, ci);
      ri += dr;
      ci += dc;
      if (ci >= nc) {
        ci -= nc;
        ++ri;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (idx + u * NT < total) store(rr[u], cc[u], v[u]);
    idx += UNR * NT;
  }
}

struct TileGeom {
  uint32_t TW, TH;      // owned tile extent (even)
  uint32_t tiles_x;     // tiles per row of tiles
};

__device__ __forceinline__ uint32_t wrap_add(uint32_t base, uint32_t off, uint32_t n) {
  uint32_t v = base + off;
  while (v >= n) v -= n;
  return v;
}

// ---- site-at-a-time updates: Action::heatbath_update / overrelaxation_update(state, l), action/action.hh:73-96 -----------
// gffaction.cc:33-42,68-77; quenchedschwingeraction.cc:25-65.  One thread per chain walks the site list in order (the
// reference's own sequential semantics: every update sees the ones before it), straight on the state in global memory.
// Same arithmetic and the same random numbers -- Philox (site, chain, step) -- as the sweep kernels, so the sites of a
// colour class visited in any order with the sweep's step reproduce that colour phase of the sweep.
// One template, two launching units: <false> belongs to lattice2d.hip (mlmcpi_lattice_site_updates), <true> to
// schwinger_sweeps.hip (schwinger_site_updates).  vs_exact_pair (step_envelope.hpp) is not inlined, and without relocatable
// device code the compiler specialises it for the callers it has in a unit: the Schwinger sweep kernels hand it the table in
// LDS, this kernel in global memory.  Only with both in one unit are the function and the sweep kernels generated as
// tools/kernel_digest.py records them (EXPERIMENTS.md 0.9).
template <bool SCHW>
__global__ void __launch_bounds__(64)
    lattice_site_update_kernel(uint32_t Mt, uint32_t Mx, double coupling, double *__restrict__ state, uint32_t B,
                               const uint32_t *__restrict__ sites, uint32_t n, uint32_t single, int heat, RngKey key0,
                               const uint32_t *__restrict__ vs_table) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  RngKey key = key0;
  key.chain += b;
  if (SCHW) {
    double *th = state + (size_t)b * 2 * Mt * Mx;
    const bool step = 2. * coupling <= kVsKappaMax;
    const VsTable tab = VsTable::in_global(vs_table);
    for (uint32_t q = 0; q < n; ++q) schwinger_site_update(th, Mt, Mx, sites ? sites[q] : single, heat != 0, step, coupling, key, tab);
  } else {
    double *phi = state + (size_t)b * Mt * Mx;
    const double inv_kappa = 1. / (4. + coupling), two_over_kappa = 2. / (4. + coupling), sigma = 1. / sqrt(4. + coupling);
    for (uint32_t q = 0; q < n; ++q)
      gff_site_update(phi, Mt, Mx, sites ? sites[q] : single, heat != 0, inv_kappa, two_over_kappa, sigma, key);
  }
}

// ---- geometry: LDS sizes and workgroup shapes, read by the kernels and by next_launch ----------------------------------------
// LDS bytes in front of the tile image of a heat-bath launch of schwinger_sweep_kernel (kernel and host agree through this)
__host__ __device__ inline size_t sweep_pool_bytes(bool step, bool fixed, uint32_t cap) {
  const size_t b = step ? (fixed ? VsPool<uint16_t>::bytes(cap) : VsPool<uint32_t>::bytes(cap)) : HbPool::bytes(cap);
  return (b + 15) / 16 * 16;
}

// ---- Schwinger overrelaxation, 4 x 4 register blocks on 64 x 64 tiles ------------------------------------------
// A 2 x 2 block kernel on 64 x 32 tiles (retired; EXPERIMENTS 4.1) recomputes (64 + 4K)(32 + 4K) / (64 * 32) = 1.875 x
// the owned updates at K = 4 and moves 24 B through LDS per update.  Here a thread keeps a 4 x 4 block of vertices (32 link angles, 64 VGPRs) for all K sweeps and
// the tile is 64 x 64: redundancy (64 + 4K)^2 / 64^2 = 1.56 at K = 4 (1.72 at K = 5, which the 1024-thread limit of the
// 2 x 2 kernel could not reach), and LDS holds only the 20 values per block that a neighbouring block reads:
//   TOP0[a], TOP1[a]   both links of the top row        (read by the block above as its row -1)
//   BOT0[a]            mu = 0 links of the bottom row   (row PH of the block below)
//   LEFT1[c]           mu = 1 links of the left column  (column PW of the block to the left)
//   RIGHT0[c], RIGHT1[c]  both links of the right column (column -1 of the block to the right)
// with the four corner values that belong to two of these lists stored once.  Per sweep a thread reads 32 and writes
// 20 doubles for its 32 updates (13 B per update).  Planes are [value][block], so consecutive lanes touch consecutive
// doubles.  Same updates in the same colour order with the same arithmetic as every other overrelaxation kernel here:
// bit-identical results.  Block edges of the buffer read clamped neighbours: what they compute
// is wrong, and never reaches the owned tile (the exact region shrinks by 2 sites per sweep from a halo of 2K).
template <int K>
struct OrBlockGeom {
  static constexpr int TW = 64, TH = 64, PW = 4, PH = 4, H = 2 * K;
  static constexpr int BW = TW + 2 * H, BH = TH + 2 * H, NPX = BW / PW, NPY = BH / PH, NP = NPX * NPY;
  static constexpr int NT = (NP + 63) / 64 * 64;
  static constexpr int NPLANE = 3 * PW + 3 * PH - 4;
  static constexpr size_t lds_bytes = (size_t)NPLANE * NP * sizeof(double);
  // plane numbers (corner values stored once)
  static constexpr int top0(int a) { return a; }
  static constexpr int top1(int a) { return PW + a; }
  static constexpr int right0(int c) { return c == PH - 1 ? top0(PW - 1) : 3 * PW - 1 + (PH - 1) + c; }
  static constexpr int right1(int c) { return c == PH - 1 ? top1(PW - 1) : 3 * PW - 1 + 2 * (PH - 1) + c; }
  static constexpr int bot0(int a) { return a == PW - 1 ? right0(0) : 2 * PW + a; }
  static constexpr int left1(int c) { return c == PH - 1 ? top1(0) : 3 * PW - 1 + c; }
};

// ---- Schwinger: the heat-bath sweep on an LDS image, behind the overrelaxation sweeps of the same launch ------------------
// A draw ends "... K overrelaxation sweeps, heat bath, QoI".  As two launches the state makes two round trips through HBM,
// and the two kernels leave opposite halves of the CU idle: the overrelaxation launch is bound by its load / store phases
// and the latencies of its colour phases, the heat bath by vector issue with its memory traffic hidden.  In one launch
// (schwinger_perm_heat_kernel) the workgroup that has just swept a tile K times lays the tile and the two rings the heat
// bath reads down as an LDS image, runs the heat-bath sweep of schwinger_sweep_kernel<true, ., 64, 32, true> on it
// (schwinger_image_heat) -- same regions (the pruned last-sweep form), same cells, same Philox words, same arithmetic:
// bit-identical results -- sums the QoI and writes the tile out.  One round trip instead of two, and the two workgroups of
// a CU are in different phases most of the time: the loads of one run under the sampler arithmetic of the other.
// This struct holds the sizes of that image (a 64 x 64 tile and two rings) and of the sampler's list in front of it.
struct HeatImageGeom {
  static constexpr int HB = 2, IW = 64 + 2 * HB, IH = 64 + 2 * HB;
  static constexpr size_t image_bytes = (size_t)2 * IW * IH * sizeof(double);
  // in front of the image: the sampler's tables and the list of open cells -- a colour phase leaves about 5 % of its ~2200
  // cells on it at beta = 1 (110 entries on average; a list that overflows leaves cells to their own lanes, measured at
  // +20 % on the launch with 64 entries)
  static constexpr uint32_t pool_cap = 544, hb_pool_cap = 128;   // step-envelope list (r05: 256 -> 544 for concentrations up to 16: a phase leaves up to a fifth of its ~2200 cells there); wrapped-Cauchy pool (24 B per entry)
  static constexpr size_t vs_pool_bytes = VsPool<uint32_t>::bytes(pool_cap), hb_pool_bytes = HbPool::bytes(hb_pool_cap);
  static constexpr size_t pool_bytes = ((vs_pool_bytes > hb_pool_bytes ? vs_pool_bytes : hb_pool_bytes) + 15) / 16 * 16;
  static constexpr size_t hb_bytes = image_bytes + pool_bytes;
  static_assert(image_bytes == 73984 && pool_bytes == 3424 && hb_bytes == 77408, "LDS layout of the fused launch");
  static_assert(hb_bytes <= OrBlockGeom<6>::lds_bytes, "two workgroups per CU");
};

// ---- Schwinger overrelaxation in closed form (schwinger_perm_kernel, schwinger_perm_heat_kernel) ---------------------------
constexpr uint32_t kPermMaxK = 10;  // sweeps per launch

// K sweeps for the (64 + 2 RING) x (TH + 2 RING) vertices around a 64 x TH tile (RING = 0: the tile; RING = 2: what the heat
// bath behind the sweeps reads; TH = 32: lattices that 64 x 32 tiles divide and 64 x 64 ones do not), in two halves of
// HR = TH / 2 + RING rows.  NB = 1: one plane of 2 HR + 4 K rows serves both; NB = 2 (K
// sweeps reach 2 K rows up and down: beyond K = 6 the whole plane does not fit beside a second workgroup): a plane of
// HR + 4 K rows; for the second half its upper HR + 4 K - HR rows move down and HR new rows are built on top.
// Tasks of a half: (HR / 2) x OW column pairs (mu = 0), then HR x (OW / 2) row pairs (mu = 1); thread t takes t, t + NT, ...
template <int NT, int RING, int TH = 64>
struct PermGeom {
  static constexpr int OW = 64 + 2 * RING, HR = TH / 2 + RING, NTASK = HR * OW, NV = (NTASK + NT - 1) / NT;
  static constexpr int WP = OW + 4 * (int)kPermMaxK;   // the plane's pitch (PermPlane): the width of the deepest launch
  static_assert(HR % 2 == 0 && OW % 2 == 0, "parities of the output = parities of the lattice; the halves move by whole quadrant rows");
  static __host__ __device__ constexpr uint32_t width(uint32_t K) { return OW + 4 * K; }
  static __host__ __device__ constexpr uint32_t rows(uint32_t K, uint32_t NB) { return (NB == 2 ? HR : 2 * HR) + 4 * K; }
  static __host__ __device__ constexpr size_t plane_bytes(uint32_t K, uint32_t NB) { return (size_t)WP * rows(K, NB) * sizeof(double); }
};

// dynamic LDS of schwinger_perm_kernel<TH>
constexpr size_t kPermPlaneMax = 80 * 1024;  // two workgroups per CU
template <int TH>
__host__ __device__ constexpr size_t perm_lds_bytes(uint32_t K, uint32_t NB) {   // the plane; then the tile's image in its place
  return PermGeom<512, 0, TH>::plane_bytes(K, NB) > 2 * 64 * TH * sizeof(double) ? PermGeom<512, 0, TH>::plane_bytes(K, NB)
                                                                                   : 2 * 64 * TH * sizeof(double);
}

// ... and of schwinger_perm_heat_kernel.  LDS: tables + list | the plane, then the image in the same place.
template <int NT, bool STEP>
struct PermHeatGeom {
  using PG = PermGeom<NT, 2>;
  using OH = HeatImageGeom;
  static constexpr size_t lds_bytes(uint32_t K, uint32_t NB) {
    return OH::pool_bytes + (PG::plane_bytes(K, NB) > OH::image_bytes ? PG::plane_bytes(K, NB) : OH::image_bytes);
  }
};

// ---- GFF overrelaxation, 4 x 4 register blocks on 64 x 64 tiles ------------------------------------------------
// The construction of schwinger_or_block_kernel for the scalar field: a thread keeps 16 sites for all K sweeps, LDS
// carries the 12 sites on the rim of each block (TOP[a], BOT[a], LEFT[c], RIGHT[c], corners once), a colour phase reads
// the 8 neighbour values across the block's edges that belong to the other colour.  Redundancy (64 + 4K)^2 / 64^2
// (1.72 at K = 5) instead of 1.875 at K = 4 on 64 x 32 tiles, 1.75 LDS accesses per update instead of 3, three
// workgroups per CU.  Same sums in the same order as gff_sweep_kernel: bit-identical.
// T: tile extent.  64 is the default; 32 x 32 tiles (r04) serve the lattices 64 x 64 tiles do not divide or that are too
// small for the fused launch (96 x 96: 339 -> see DESIGN 7, fast_path_cliff) -- the halo recomputation is 2.6 x at K = 5
// instead of 1.7 x, but the launches are bound by their passes over the state, not by the sweeps.
template <int K, int T = 64>
struct GffBlockGeom {
  static constexpr int TW = T, TH = T, PW = 4, PH = 4, H = 2 * K;
  static constexpr int BW = TW + 2 * H, BH = TH + 2 * H, NPX = BW / PW, NPY = BH / PH, NP = NPX * NPY;
  static constexpr int NT = (NP + 63) / 64 * 64;
  static constexpr int NPLANE = 2 * PW + 2 * (PH - 2);
  static constexpr size_t lds_bytes = (size_t)NPLANE * NP * sizeof(double);
  static constexpr int top(int a) { return a; }
  static constexpr int bot(int a) { return PW + a; }
  static constexpr int left(int c) { return c == 0 ? bot(0) : c == PH - 1 ? top(0) : 2 * PW + (c - 1); }
  static constexpr int right(int c) { return c == 0 ? bot(PW - 1) : c == PH - 1 ? top(PW - 1) : 2 * PW + (PH - 2) + (c - 1); }
};

// gff_or_heat_kernel: the blocks with halo 2 K + 2, then the field on the tile and two rings as an LDS image in their place
template <int K, int T = 64>
struct GffHeatGeom {
  using G = GffBlockGeom<K + 1, T>;
  static constexpr int NT = G::NT, HB = 2, IW = G::TW + 2 * HB, IH = G::TH + 2 * HB;
  static constexpr size_t image_bytes = (size_t)IW * IH * sizeof(double);
  static constexpr size_t lds_bytes = G::lds_bytes > image_bytes ? G::lds_bytes : image_bytes;
};

// ---- host helpers ----------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, K>()) with the compile-time depth K = min(n, KMAX), n >= 1: one instantiation per depth
template <int KMAX, int K = 1, class F>
static int with_depth(uint32_t n, F &&f) {
  if constexpr (K < KMAX) {
    if (n > (uint32_t)K) return with_depth<KMAX, K + 1>(n, f);
  }
  return f(std::integral_constant<int, K>());
}

static int allow_lds(const void *kernel, size_t bytes) {
  MLMCPI_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return MLMCPI_OK;
}

// ---- launchers: one SweepLaunch each --------------------------------------------------------------------------------
// one launch of a draw, as lattice2d.hip's planner describes it (include/mlmcpi_hip.h: what mlmcpi_lattice_sweep_plan reports)
using SweepLaunch = mlmcpi_sweep_launch;

struct SweepArgs {  // what a launch needs beside its SweepLaunch
  uint32_t Mt, Mx, B;
  double coupling;                        // beta; GFF: mu2
  const double *src;
  double *dst;
  RngKey key;                             // of the launch's first sweep
  int qoi_op;                             // op != 0: the launch ends the draw and finishes the QoI of the final state ...
  double *d_qoi, *d_acc;                  // ... into d_qoi[b], and into the record_sample moments of d_acc where that is not NULL
  hipStream_t st;
  // filled in by the action's launcher for its kernels, not by the executor
  double *qoi_partial = nullptr;          // the QoI summed per tile: qoi_partial[b * grid.x + tile]
  const uint32_t *vs_table = nullptr;     // l.step: the step-envelope sampler's table
};

// The launch `l` of the action's draw: reads a.src, writes a.dst.  A launcher fetches what its kernels need (the sampler's table,
// the scratch for the QoI partials), launches the kernel and, where the launch carries the QoI, finishes it with one more launch.
// Kernels are launched only by the unit that defines them.
int schwinger_sweep_launch(const SweepLaunch &l, const SweepArgs &a);  // schwinger_sweeps.hip
int gff_sweep_launch(const SweepLaunch &l, const SweepArgs &a);        // gff_sweeps.hip
int sigma_sweep_launch(const SweepLaunch &l, const SweepArgs &a);      // sigma2d.hip
// The kernels of a unit whose LDS may exceed the 64 KiB default are allowed it, on the current device (init_sweep_kernels,
// lattice2d.hip, calls these once per device; the sigma model keeps its own once-per-device flag)
int schwinger_allow_lds();
int gff_allow_lds();
int sigma_init_sweep_kernels();
// mlmcpi_lattice_site_updates for the Schwinger action (arguments checked there), as sigma_site_updates (internal.hpp)
int schwinger_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites, uint32_t n,
                           uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, hipStream_t st);

}  // namespace mlmcpi
