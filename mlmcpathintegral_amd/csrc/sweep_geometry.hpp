// sweep_geometry.hpp -- the sizes the planner (lattice2d.hip) and the 2-D sweep kernels agree on that need no sampler, each
// defined once, and the description of a launch.  lattice_sweep.hpp includes it and adds what depends on a sampler; a unit that
// draws nothing (schwinger_or_block.hip) includes this header alone.
#pragma once
#include <type_traits>

#include "internal.hpp"

namespace mlmcpi {

// the tiles of the generic overlapped-tile kernels (schwinger_sweep_kernel, gff_sweep_kernel)
struct TileGeom {
  uint32_t TW, TH;      // owned tile extent (even)
  uint32_t tiles_x;     // tiles per row of tiles
};

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

// ---- Schwinger overrelaxation in closed form (schwinger_perm_kernel, schwinger_perm_heat_kernel) ---------------------------
constexpr uint32_t kPermMaxK = 10;  // sweeps per launch

// K sweeps for the (64 + 2 RING) x (TH + 2 RING) vertices around a 64 x TH tile (RING = 0: the tile; RING = 2: what the heat
// bath behind the sweeps reads; TH = 32: lattices that 64 x 32 tiles divide and 64 x 64 ones do not), in two halves of
// HR = TH / 2 + RING rows that share ONE plane of plaquettes.
// Tasks of a half: (HR / 2) x OW column pairs (mu = 0), then HR x (OW / 2) row pairs (mu = 1); thread t takes t, t + NT, ...
//
// The read set.  Plane coordinates: output vertex (c, r), 0 <= c < OW, 0 <= r < OH = 2 HR, is plane (C, R) = (c + 2 K, r + 2 K);
// all of 2 K, OW, HR and the tile origins are even, so plane, output and lattice parities agree.  From the two sums of
// schwinger_perm.hpp, with s = 0 .. K - 1:
//   mu = 0 task at (C, R), R even:   P(C + 2 s e_C, R - 1 - 2 s),  P(C + 2 s e_C, R + 2 s),  P(C + 2 s e_C, R + 2 + 2 s)
//   mu = 1 task at (C, R), C even:   P(C - 1 - 2 s, J_s),  P(C + 2 s, J_s),  P(C + 2 + 2 s, J_s),   J_s = R + 2 (s + 1) e_R.
// An index that is read at an even value only ever grows from where a task stands, one that is read at an odd value only falls:
//   even columns:  mu = 0, C even: C .. C + 2 K - 2;  mu = 1: C .. C + 2 K                ->  [2 K, OW + 4 K - 2]
//   odd columns:   mu = 0, C odd:  C - 2 K + 2 .. C;  mu = 1: C - 2 K + 1 .. C - 1         ->  [1, OW + 2 K - 1]
//   even rows:     mu = 0: R .. R + 2 K;              mu = 1, R even: R + 2 .. R + 2 K    ->  [2 K, OH + 4 K - 2]
//   odd rows:      mu = 0: R - 2 K + 1 .. R - 1;      mu = 1, R odd:  R - 2 K .. R - 2    ->  [1, OH + 2 K - 3]
// (C over [2 K, 2 K + OW), R over [2 K, 2 K + OH) of the task's parity).  That is OW / 2 + K columns of either parity and
// OH / 2 + K even, OH / 2 + K - 1 odd rows: each of the four (column parity, row parity) quadrants of the plane is read over
// about (OW / 2 + K) x (OH / 2 + K) plaquettes instead of the (OW / 2 + 2 K) x (OH / 2 + 2 K) of the rectangle around them.
// Packed (PermPlane) every quadrant is kQRows rows of kPitch values, the extents of the deepest launch: the four of them
// fit the LDS of the image that follows them at every depth, so one build serves both halves.
template <int NT, int RING, int TH = 64>
struct PermGeom {
  static constexpr int OW = 64 + 2 * RING, HR = TH / 2 + RING, OH = 2 * HR, NTASK = HR * OW, NV = (NTASK + NT - 1) / NT;
  static_assert(HR % 2 == 0 && OW % 2 == 0, "parities of the output = parities of the lattice");
  // the plaquettes a build has to cover: columns [0, width), rows [0, rows) around the read set
  static __host__ __device__ constexpr uint32_t width(uint32_t K) { return OW + 4 * K; }
  static __host__ __device__ constexpr uint32_t rows(uint32_t K) { return OH + 4 * K; }
  // first and last column / row of parity `par` that any task reads
  static __host__ __device__ constexpr uint32_t col_first(uint32_t K, uint32_t par) { return par ? 1 : 2 * K; }
  static __host__ __device__ constexpr uint32_t col_last(uint32_t K, uint32_t par) { return par ? OW + 2 * K - 1 : OW + 4 * K - 2; }
  static __host__ __device__ constexpr uint32_t row_first(uint32_t K, uint32_t par) { return par ? 1 : 2 * K; }
  static __host__ __device__ constexpr uint32_t row_last(uint32_t K, uint32_t par) { return par ? OH + 2 * K - 3 : OH + 4 * K - 2; }
  static __host__ __device__ constexpr uint32_t col_count(uint32_t K, uint32_t par) { return (col_last(K, par) - col_first(K, par)) / 2 + 1; }
  static __host__ __device__ constexpr uint32_t row_count(uint32_t K, uint32_t par) { return (row_last(K, par) - row_first(K, par)) / 2 + 1; }
  // a quadrant: kQRows rows of kPitch values (odd rows: one row of padding); the plane: four quadrants, whatever K
  static constexpr int kPitch = OW / 2 + (int)kPermMaxK, kQRows = OH / 2 + (int)kPermMaxK;
  static_assert(col_count(kPermMaxK, 0) == kPitch && col_count(kPermMaxK, 1) == kPitch, "the pitch: the columns of a parity at the deepest launch");
  static_assert(row_count(kPermMaxK, 0) == kQRows && row_count(kPermMaxK, 1) == kQRows - 1, "the rows of a quadrant at the deepest launch");
  static constexpr size_t plane_bytes = (size_t)4 * kQRows * kPitch * sizeof(double);
  // the value index of plaquette (C, R) of the read set of a launch of K sweeps: the odd index mirrored, so that a step of
  // any stream is (u, v) -> (u + 1, v + 1)
  static __host__ __device__ constexpr uint32_t col_u(uint32_t K, uint32_t C) { return (C & 1u) ? (col_last(K, 1) - C) / 2 : (C - col_first(K, 0)) / 2; }
  static __host__ __device__ constexpr uint32_t row_v(uint32_t K, uint32_t R) { return (R & 1u) ? (row_last(K, 1) - R) / 2 : (R - row_first(K, 0)) / 2; }
  static __host__ __device__ constexpr uint32_t offset(uint32_t K, uint32_t C, uint32_t R) {
    return ((R & 1u) * 2 + (C & 1u)) * (uint32_t)(kQRows * kPitch) + row_v(K, R) * (uint32_t)kPitch + col_u(K, C);
  }
  static constexpr uint32_t kStep = kPitch + 1;   // values per step of a stream
};

// dynamic LDS of schwinger_perm_kernel<TH>
constexpr size_t kPermPlaneMax = 80 * 1024;  // two workgroups per CU
template <int TH>
__host__ __device__ constexpr size_t perm_lds_bytes() {   // the plane; then the tile's image in its place
  return PermGeom<512, 0, TH>::plane_bytes > 2 * 64 * TH * sizeof(double) ? PermGeom<512, 0, TH>::plane_bytes : 2 * 64 * TH * sizeof(double);
}
static_assert(perm_lds_bytes<64>() <= kPermPlaneMax && perm_lds_bytes<32>() <= kPermPlaneMax, "the packed plane fits at every depth");

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

// ---- a launch ----------------------------------------------------------------------------------------------------------------
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

}  // namespace mlmcpi
