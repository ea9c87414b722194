// wilson_loops.hip -- Wilson loops W(r, s), 1 <= r <= R, 1 <= s <= S, of the quenched Schwinger model (include/mlmcpi_hip.h:
// mlmcpi_schwinger_wilson_loops*).
//
//   W(r, s) = (1 / (Mt Mx)) sum_{i,j} cos Theta(i, j; r, s),  Theta = the sum of the unreduced plaquette angles of the r x s cells
//   (i + k, j + l), k < r, l < s, all indices periodic (r links along direction 0, s along direction 1).
//
// e^{i Theta} is the product of the cell phases z = e^{i theta_p}: one sincos per plaquette, complex multiplies for the rest.
//   strip  U(i, j; r)    = U(i, j; r - 1) z(i + r - 1, j)          U(.; 0) = 1
//   loop   P(i, j; r, s) = P(i, j; r, s - 1) U(i, j + s - 1; r)    P(.; r, 0) = 1,   W(r, s) = (1/V) sum Re P
//
// A workgroup of 256 threads takes one tile of 32 x 32 base vertices of one chain (edge tiles are clipped to the lattice: tw x th).
//   1. Links: the (tw + R) x (th + S) vertices from the tile's corner on go into LDS as double2, one coalesced 16-byte load per
//      vertex, every periodic wrap resolved here (index mod extent, any number of wraps).
//   2. Phases: each thread forms the plaquette angles of its cells of the (tw + R - 1) x (th + S - 1) image in the order of
//      plaquette_angle (lattice_reduce.hip), takes their sincos into registers and, behind a barrier, writes (cos, sin) over the
//      links: one image, at most 48 x 48 x 16 B = 36 KiB, so that two workgroups share a CU within kWlLdsBytes = 64 KiB.
//      Row stride: tw + R slots of 16 bytes, no padding.  Thread t holds column t % 32 and the rows 4 (t / 32) .. + 3, so lanes l
//      and l + 32 of a wave read two rows and the lanes of a half wave 32 consecutive slots; each of the four 16-lane groups of a
//      16-byte LDS read (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) then covers 16 slots that are distinct
//      mod 16, i.e. every bank once, at ANY row stride.
//   3. For r = 1 .. R: the thread extends the strips of its window, the J + S - 1 = 4 + S - 1 rows from its first base row on,
//      in registers (one LDS read and one complex multiply per row), then walks s = 1 .. S for each of its J base rows from
//      registers: acc[s] += Re P, base rows ascending.  J S products for J + S - 1 LDS reads.
//   4. block_sum over the S accumulators (lane tree, then the four waves ascending); one partial per (chain, tile, r, s) goes to
//      the workspace.  wilson_loops_finish_kernel adds the tiles in ascending order, multiplies by 1 / V last, writes d_out and
//      with d_acc adds W and W^2.
// No atomics, no knob; the geometry is a function of (Mt, Mx, R, S) alone: a chain's output is the same bits for every B, every
// split of the chains over calls and every stream.  Complex multiplies are spelled (two products, two FMAs); the unit is compiled
// without fp contraction.
#include "internal.hpp"

#pragma clang fp contract(off)

namespace mlmcpi {

constexpr uint32_t kWlThreads = 256;
constexpr uint32_t kWlTile = 32;         // base vertices of a tile along either direction
constexpr uint32_t kWlJ = 4;             // consecutive base rows of one column per thread: 32 columns x 8 row groups
constexpr uint32_t kWlMax = MLMCPI_WILSON_LOOPS_MAX;  // cap on R and S
constexpr uint32_t kWlLdsBytes = 65536;  // LDS a workgroup may take (two workgroups per CU)
constexpr uint32_t kWlCells = ((kWlTile + kWlMax - 1) * (kWlTile + kWlMax - 1) + kWlThreads - 1) / kWlThreads;  // cells of the image per thread: 9
constexpr uint32_t kWlGridX = (1u << 31) / kWlThreads;  // workgroups along x of a launch; beyond, the grid grows along y
constexpr uint64_t kWlMaxBlocks = (uint64_t)kWlGridX * 65535;

struct WlPlan {
  uint32_t Mt, Mx, R, S;
  uint32_t ntx, nty;    // tiles along direction 0 and 1
  uint32_t lds_bytes;   // of the largest (unclipped) tile of this lattice
};

__host__ __device__ inline uint32_t wl_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

inline void wl_plan(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, WlPlan *pl) {
  WlPlan p;
  p.Mt = Mt;
  p.Mx = Mx;
  p.R = R;
  p.S = S;
  p.ntx = (Mt + kWlTile - 1) / kWlTile;
  p.nty = (Mx + kWlTile - 1) / kWlTile;
  p.lds_bytes = (wl_min(kWlTile, Mt) + R) * (wl_min(kWlTile, Mx) + S) * 16;
  *pl = p;
}

// (sin, cos)(x) for |x| <= 4 pi + a few ulp (an unreduced plaquette angle): two-term Cody-Waite reduction by quarter turns to
// |r| <= pi/4 (|n| <= 8; the FMA rounds the difference once), the Taylor kernels of sincos_2pi_unit (truncation < 5e-17 / 2e-18),
// rotation by the quadrant.  Absolute error of either component about 1 ulp of 1.
__device__ __forceinline__ void sincos_reduced(double x, double &sn, double &cs) {
  const double q = rint(x * 0.63661977236758134308);  // x / (pi/2)
  double r = __fma_rn(-q, 1.57079632679489655800e+00, x);  // pi/2, high part
  r = __fma_rn(-q, 6.12323399573676603587e-17, r);        // pi/2 - high part
  const double r2 = r * r;
  double sp = -7.6471637318198164759e-13;
  sp = __fma_rn(sp, r2, 1.6059043836821614599e-10);
  sp = __fma_rn(sp, r2, -2.5052108385441718775e-08);
  sp = __fma_rn(sp, r2, 2.7557319223985890653e-06);
  sp = __fma_rn(sp, r2, -1.9841269841269841270e-04);
  sp = __fma_rn(sp, r2, 8.3333333333333333333e-03);
  sp = __fma_rn(sp, r2, -1.6666666666666666667e-01);
  const double s0 = __fma_rn(r * r2, sp, r);
  double cp = 4.7794773323873852974e-14;
  cp = __fma_rn(cp, r2, -1.1470745597729724714e-11);
  cp = __fma_rn(cp, r2, 2.0876756987868098979e-09);
  cp = __fma_rn(cp, r2, -2.7557319223985890653e-07);
  cp = __fma_rn(cp, r2, 2.4801587301587301587e-05);
  cp = __fma_rn(cp, r2, -1.3888888888888888889e-03);
  cp = __fma_rn(cp, r2, 4.1666666666666666667e-02);
  cp = __fma_rn(cp, r2, -0.5);
  const double c0 = __fma_rn(cp, r2, 1.0);
  const int k = (int)q & 3;  // rotation by k quarter turns (two's complement: right for negative q as well)
  const double cr = (k & 1) ? -s0 : c0, sr = (k & 1) ? c0 : s0;
  cs = (k & 2) ? -cr : cr;
  sn = (k & 2) ? -sr : sr;
}

// a b of two complex numbers (x: real, y: imaginary part): two products, two FMAs
__device__ __forceinline__ double2 wl_cmul(double2 a, double2 b) {
  return make_double2(__fma_rn(a.x, b.x, -(a.y * b.y)), __fma_rn(a.x, b.y, a.y * b.x));
}

// workgroup w = blockIdx.y gridDim.x + blockIdx.x < nblocks: tile w mod (ntx nty) (tile = ty ntx + tx) of chain w / (ntx nty).
//   partial[((b ntiles + tile) R + r - 1) S + s - 1] = sum over the tile's base vertices of Re P(i, j; r, s)
// ST: the S of the call rounded up to 4, 8 or 16 (the register window and the accumulators are sized by it).
template <int ST>
__global__ void __launch_bounds__(kWlThreads)
    wilson_loops_kernel(WlPlan P, uint64_t nblocks, const double2 *__restrict__ theta, double *__restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double2 wl_img[];
  __shared__ double red[ST * (kWlThreads / kWave)];
  const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (wg >= nblocks) return;
  const uint32_t ntiles = P.ntx * P.nty, tile = (uint32_t)(wg % ntiles);
  const uint64_t b = wg / ntiles;
  const uint32_t i0 = (tile % P.ntx) * kWlTile, j0 = (tile / P.ntx) * kWlTile;
  const uint32_t tw = wl_min(kWlTile, P.Mt - i0), th = wl_min(kWlTile, P.Mx - j0);  // base vertices of this tile
  const uint32_t W = tw + P.R - 1, H = th + P.S - 1;                                // cells of its image
  const uint32_t LS = W + 1;                                                         // row stride; the link image has H + 1 rows
  const double2 *t = theta + (size_t)b * P.Mt * P.Mx;

  // 1. links
  for (uint32_t n = threadIdx.x; n < LS * (H + 1); n += kWlThreads) {
    const uint32_t cj = n / LS, ci = n - cj * LS;
    const uint32_t gi = (i0 + ci) % P.Mt, gj = (j0 + cj) % P.Mx;
    wl_img[n] = t[(size_t)gj * P.Mt + gi];
  }
  __syncthreads();
  // 2. phases, in place
  double2 z[kWlCells];
#pragma unroll
  for (uint32_t q = 0; q < kWlCells; ++q) {
    const uint32_t n = threadIdx.x + q * kWlThreads;
    z[q] = make_double2(1.0, 0.0);
    if (n < W * H) {
      const uint32_t cj = n / W, ci = n - cj * W;
      const double2 here = wl_img[cj * LS + ci];
      // theta(i,j,0) + theta(i+1,j,1) - theta(i,j+1,0) - theta(i,j,1): the order of plaquette_angle
      const double a = here.x + wl_img[cj * LS + ci + 1].y - wl_img[(cj + 1) * LS + ci].x - here.y;
      sincos_reduced(a, z[q].y, z[q].x);
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t q = 0; q < kWlCells; ++q) {
    const uint32_t n = threadIdx.x + q * kWlThreads;
    if (n < W * H) {
      const uint32_t cj = n / W, ci = n - cj * W;
      wl_img[cj * LS + ci] = z[q];
    }
  }
  __syncthreads();

  // 3. strips and loops
  const uint32_t col = threadIdx.x % kWlTile, row0 = (threadIdx.x / kWlTile) * kWlJ;
  const bool col_ok = col < tw;
  double2 U[kWlJ + ST - 1];
#pragma unroll
  for (int k = 0; k < (int)kWlJ + ST - 1; ++k) U[k] = make_double2(1.0, 0.0);
  double *out = partial + (wg * P.R) * P.S;
  for (uint32_t r = 1; r <= P.R; ++r) {
    if (col_ok) {
#pragma unroll
      for (int k = 0; k < (int)kWlJ + ST - 1; ++k)
        if (k < (int)(kWlJ + P.S - 1) && row0 + k < H) U[k] = wl_cmul(U[k], wl_img[(row0 + k) * LS + col + r - 1]);
    }
    double acc[ST];
#pragma unroll
    for (int s = 0; s < ST; ++s) acc[s] = 0.0;
    if (col_ok) {
#pragma unroll
      for (int jj = 0; jj < (int)kWlJ; ++jj) {
        if (row0 + jj < th) {
          double2 p = U[jj];
          acc[0] += p.x;
#pragma unroll
          for (int s = 1; s < ST; ++s) {
            if (s < (int)P.S) {
              p = wl_cmul(p, U[jj + s]);
              acc[s] += p.x;
            }
          }
        }
      }
    }
    block_sum<ST>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int s = 0; s < ST; ++s)
        if (s < (int)P.S) out[(size_t)(r - 1) * P.S + s] = acc[s];
    }
  }
}

// entry e < B R S (grid stride): the partials of its chain, r and s added in ascending tile order, then times 1 / V
__global__ void __launch_bounds__(kWlThreads)
    wilson_loops_finish_kernel(uint32_t RS, uint32_t ntiles, size_t n, double inv_V, const double *__restrict__ partial,
                               double *__restrict__ out, double *__restrict__ acc) {
  for (size_t e = (size_t)blockIdx.x * kWlThreads + threadIdx.x; e < n; e += (size_t)gridDim.x * kWlThreads) {
    const size_t b = e / RS, k = e % RS;
    const double *p = partial + b * ntiles * RS + k;
    double s = 0.0;
    for (uint32_t tl = 0; tl < ntiles; ++tl) s += p[(size_t)tl * RS];
    const double Wl = s * inv_V;
    out[e] = Wl;
    if (acc) {
      acc[2 * e] += Wl;
      acc[2 * e + 1] += Wl * Wl;
    }
  }
}

namespace {

// the checks every entry point shares; then the plan
int wl_check(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, uint32_t B, WlPlan *pl, uint64_t *blocks, size_t *work_bytes) {
  MLMCPI_REQUIRE(Mt >= 2 && Mx >= 2, "lattice %u x %u too small", Mt, Mx);
  MLMCPI_REQUIRE((uint64_t)Mt * Mx <= (1ull << 30), "lattice too large for 32-bit site indices");
  MLMCPI_REQUIRE(B > 0 && R > 0 && S > 0, "Wilson loops need B, R, S > 0 (got %u, %u, %u)", B, R, S);
  if (R > kWlMax || S > kWlMax)
    return fail(MLMCPI_ERR_UNSUPPORTED, "Wilson loops are built up to %u x %u (got %u x %u)", kWlMax, kWlMax, R, S);
  MLMCPI_REQUIRE(R <= Mt && S <= Mx, "Wilson loops of %u x %u do not fit the %u x %u lattice", R, S, Mt, Mx);
  wl_plan(Mt, Mx, R, S, pl);
  *blocks = (uint64_t)B * pl->ntx * pl->nty;
  MLMCPI_REQUIRE(*blocks <= kWlMaxBlocks, "Wilson loops take at most %llu workgroups per call (these chains need %llu)",
                 (unsigned long long)kWlMaxBlocks, (unsigned long long)*blocks);
  *work_bytes = align256((size_t)*blocks * R * S * sizeof(double));
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_schwinger_wilson_loops_workspace_bytes(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, uint32_t B, size_t *bytes) {
  WlPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = wl_check(Mt, Mx, R, S, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(bytes, "bad arguments");
  *bytes = wb;
  return MLMCPI_OK;
}

int mlmcpi_schwinger_wilson_loops_plan(uint32_t Mt, uint32_t Mx, uint32_t R, uint32_t S, uint32_t B, mlmcpi_wilson_loops_plan_info *out) {
  WlPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = wl_check(Mt, Mx, R, S, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(out, "bad arguments");
  out->work_bytes = wb;
  out->grid = blocks;
  out->workgroup = kWlThreads;
  out->tile_w = kWlTile;
  out->tile_h = kWlTile;
  out->halo_w = R - 1;
  out->halo_h = S - 1;
  out->J = kWlJ;
  out->tiles_w = pl.ntx;
  out->tiles_h = pl.nty;
  out->tiles = pl.ntx * pl.nty;
  out->lds_bytes = pl.lds_bytes;
  out->lds_limit = kWlLdsBytes;
  return MLMCPI_OK;
}

int mlmcpi_schwinger_wilson_loops(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, uint32_t R, uint32_t S, double *d_out,
                                  double *d_acc, void *d_work, size_t work_bytes, void *stream) {
  WlPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = wl_check(Mt, Mx, R, S, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(d_theta && d_out && d_work, "bad arguments");
  MLMCPI_REQUIRE(work_bytes >= wb, "the Wilson loops' workspace is too small (%zu bytes, needs %zu)", work_bytes, wb);
  hipStream_t st = as_stream(stream);
  const uint32_t gx = blocks < kWlGridX ? (uint32_t)blocks : kWlGridX;
  const dim3 grid(gx, (uint32_t)((blocks + gx - 1) / gx)), block(kWlThreads);
  const double2 *theta = (const double2 *)d_theta;
  double *partial = (double *)d_work;
  if (S <= 4)
    hipLaunchKernelGGL((wilson_loops_kernel<4>), grid, block, pl.lds_bytes, st, pl, blocks, theta, partial);
  else if (S <= 8)
    hipLaunchKernelGGL((wilson_loops_kernel<8>), grid, block, pl.lds_bytes, st, pl, blocks, theta, partial);
  else
    hipLaunchKernelGGL((wilson_loops_kernel<16>), grid, block, pl.lds_bytes, st, pl, blocks, theta, partial);
  MLMCPI_LAUNCH_CHECK("wilson_loops_kernel");
  const size_t n = (size_t)B * R * S;
  const size_t fb = (n + kWlThreads - 1) / kWlThreads;
  hipLaunchKernelGGL(wilson_loops_finish_kernel, dim3((uint32_t)(fb < 65536 ? fb : 65536)), block, 0, st, R * S, pl.ntx * pl.nty, n,
                     1.0 / ((double)Mx * Mt), (const double *)partial, d_out, d_acc);
  MLMCPI_LAUNCH_CHECK("wilson_loops_finish_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
