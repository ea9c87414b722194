// gff_correlator.hip -- the momentum-projected time-slice correlators of a Gaussian free field state on a level, rotated or not
// (include/mlmcpi_hip.h: mlmcpi_gff_correlator*).
//
//   S^t_i(q) = sum_j phi(i, j) e^{-2 pi i q j / Mx},   C_t(tau; q) = (1/N) sum_i Re[S^t_i(q) conj S^t_{(i + tau) mod Mt}(q)]
//   S^x_j(q) = sum_i phi(i, j) e^{-2 pi i q i / Mt},   C_x(tau; q) likewise along j;   q = 0 .. P - 1, tau = 0 .. M_d / 2
//
// A level is one plane (unrotated: W x H = Mt x Mx, index W r + c, vertex (c, r)) or two (rotated: E and O, W x H = Mt/2 x Mx/2
// each, plane p holds the vertices (2 c + p, 2 r + p)).  Four launches, the state is read ONCE:
//   0. gff_twiddle_kernel: the Mt-th and the Mx-th roots of unity into the workspace, one sincospi per entry.  The quarter turn
//      is split off in integers (4 k = n M + rem, |rem| <= M/2), so the argument rem / (2 M) of sincospi is within 1/4 and entry 0,
//      like every multiple of a quarter turn, is exact.
//   1. gff_project_kernel: a workgroup takes a band of kGcBand rows of a chunk of kGcTile columns of one plane of one chain, tile by
//      tile (kGcTile x kGcTile) through LDS.  Column task (q, c): the band's partial of S^t, rows ascending, one FMA per part and
//      vertex, kept in registers over the tiles of the band.  Row task (q, r): the chunk's partial of S^x, columns ascending.
//      The twiddle of (q, j) is the table entry (q j) mod M, the product reduced in integers; no twiddle is formed by recurrence.
//      LDS: the tile has a row stride of 65 doubles, so a column task (32 lanes of a ds_read_b64: 32 consecutive doubles) and a
//      row task (lane l: double 65 l + c, bank pair 2 (l + c) mod 64) both touch every bank pair once; the twiddle of a task's
//      step is one address for the whole wave (a wave holds 64 tasks of one q) and is broadcast.
//   2. gff_gather_kernel: adds a slice's partials in ascending band (S^t) / chunk (S^x) order.
//   3. gff_lags_kernel: one wave per (lag, q, direction, chain): lane l adds the slices l, l + 64, .. ascending, wave_sum, times
//      1 / N last; the same lane updates d_acc.
// Workgroups of every launch are one linear index (chain x tile, chain x block of lags) laid over grid x and past it y.  No atomics,
// no knob; the geometry is a function of (Mt, Mx, rotated, P) alone: a chain's output is the same bits for every batch size, every
// split of the chains over calls, every stream, and with or without d_acc.
#include "internal.hpp"

#pragma clang fp contract(off)

namespace mlmcpi {

constexpr uint32_t kGcThreads = 256;
constexpr uint32_t kGcTile = 64;          // rows and columns of a tile; columns of a chunk
constexpr uint32_t kGcLd = kGcTile + 1;   // row stride of the tile in LDS, doubles
constexpr uint32_t kGcBand = 256;         // rows of a band: four tiles
constexpr uint32_t kGcMaxP = MLMCPI_GFF_CORRELATOR_MAX_MOMENTA;
constexpr uint32_t kGcTasks = kGcTile * kGcMaxP / kGcThreads;  // column (row) tasks of a thread at P = kGcMaxP: 2
constexpr uint32_t kGcLagsPerBlock = 32;  // lags per workgroup of the lag pass, eight per wave
constexpr uint32_t kGcLdsBytes = 65536;   // LDS a workgroup may take
constexpr uint32_t kGcLdsExtent = kGcLdsBytes / sizeof(double2);  // the lag pass keeps the slice sums of an extent <= this in LDS
constexpr uint32_t kGcProjectLds = kGcTile * kGcLd * sizeof(double) + 2 * kGcMaxP * kGcTile * sizeof(double2);  // 49664
constexpr uint32_t kGcGridX = (1u << 31) / kGcThreads;  // workgroups along x of a launch; beyond, the grid grows along y
constexpr uint64_t kGcMaxBlocks = (uint64_t)kGcGridX * 65535;
static_assert(kGcProjectLds <= kGcLdsBytes, "the projection pass stays within 64 KiB of LDS");

struct GcPlan {
  uint32_t Mt, Mx, rot, P;
  uint32_t W, H, np;       // plane: W columns (the contiguous index), H rows; np planes
  uint32_t nchunk, nband;  // chunks of kGcTile columns, bands of kGcBand rows
  uint32_t vec;            // W even: every row of a chunk starts on 16 bytes, the tile is loaded as double2
  uint32_t nvert;          // N
};

inline GcPlan gc_plan(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t P) {
  GcPlan G;
  G.Mt = Mt;
  G.Mx = Mx;
  G.rot = rotated ? 1 : 0;
  G.P = P;
  G.W = G.rot ? Mt / 2 : Mt;
  G.H = G.rot ? Mx / 2 : Mx;
  G.np = G.rot ? 2 : 1;
  G.nchunk = (G.W + kGcTile - 1) / kGcTile;
  G.nband = (G.H + kGcBand - 1) / kGcBand;
  G.vec = G.W % 2 == 0;
  G.nvert = G.W * G.H * G.np;
  return G;
}

__device__ __forceinline__ uint64_t gc_block() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// ---- (0) the roots of unity ---------------------------------------------------------------------------------------------------
// tab[e], e < Mt: e^{+2 pi i e / Mt}; tab[Mt + e], e < Mx: e^{+2 pi i e / Mx}; (cos, sin)
__global__ void __launch_bounds__(kGcThreads) gff_twiddle_kernel(uint32_t Mt, uint32_t Mx, double2 *__restrict__ tab) {
  const uint64_t e = (uint64_t)blockIdx.x * kGcThreads + threadIdx.x;
  if (e >= (uint64_t)Mt + Mx) return;
  const uint64_t M = e < Mt ? Mt : Mx, k = e < Mt ? e : e - Mt;
  const uint64_t n = (4 * k + M / 2) / M;               // nearest quarter turn (M is even)
  const int64_t rem = (int64_t)(4 * k) - (int64_t)(n * M);  // -M/2 <= rem < M/2: the angle is (pi/2) (n + rem / M)
  double s0, c0;
  sincospi((double)rem / (2.0 * (double)M), &s0, &c0);
  const double cr = (n & 1) ? -s0 : c0, sr = (n & 1) ? c0 : s0;
  tab[e] = make_double2((n & 2) ? -cr : cr, (n & 2) ? -sr : sr);
}

// ---- (1) the projection pass --------------------------------------------------------------------------------------------------
// workgroup w < nblocks: x = w mod (np nband nchunk), chain b = w / (np nband nchunk); chunk = x mod nchunk, band = (x / nchunk) mod
// nband, plane p = x / (nchunk nband).
//   colpart[(((b np + p) nband + band) P + q) W + col]    the band's partial of S^t(q) of column col, rows ascending
//   rowpart[(((b np + p) nchunk + chunk) P + q) H + row]  the chunk's partial of S^x(q) of row `row`, columns ascending
// Task u = tid + 256 k < 64 P: momentum u / 64, column (row) u mod 64 of the tile; the row tasks start at the other half of the
// workgroup (tid ^ 128), so that at P <= 2 the two kinds run on different waves.
__global__ void __launch_bounds__(kGcThreads)
    gff_project_kernel(GcPlan G, uint64_t nblocks, const double *__restrict__ phi, const double2 *__restrict__ tab,
                       double2 *__restrict__ colpart, double2 *__restrict__ rowpart) {
  __shared__ double tile[kGcTile * kGcLd];
  __shared__ double2 twr[kGcMaxP * kGcTile];  // [q][row of the tile]: e^{-2 pi i q j / Mx}
  __shared__ double2 twc[kGcMaxP * kGcTile];  // [q][column of the tile]: e^{-2 pi i q i / Mt}
  const uint64_t wg = gc_block();
  if (wg >= nblocks) return;
  const uint32_t per = G.np * G.nband * G.nchunk, x = (uint32_t)(wg % per), tid = threadIdx.x;
  const uint64_t b = wg / per;
  const uint32_t chunk = x % G.nchunk, band = (x / G.nchunk) % G.nband, p = x / (G.nchunk * G.nband);
  const uint32_t c0 = chunk * kGcTile, nc = G.W - c0 < kGcTile ? G.W - c0 : kGcTile;
  const uint32_t r0 = band * kGcBand, r1 = G.H - r0 < kGcBand ? G.H : r0 + kGcBand;
  const uint32_t ntask = G.P * kGcTile;
  const double *s = phi + (size_t)b * G.nvert + (size_t)p * G.W * G.H;
  const double2 *tab_t = tab, *tab_x = tab + G.Mt;
  double2 *rp = rowpart + (((size_t)b * G.np + p) * G.nchunk + chunk) * G.P * G.H;

  for (uint32_t u = tid; u < ntask; u += kGcThreads) {
    const uint32_t q = u / kGcTile, lc = u % kGcTile;
    if (lc < nc) {
      const uint32_t i = G.rot ? 2 * (c0 + lc) + p : c0 + lc;
      const double2 t = tab_t[(uint32_t)(((uint64_t)q * i) % G.Mt)];
      twc[u] = make_double2(t.x, -t.y);
    }
  }
  double2 cacc[kGcTasks];
#pragma unroll
  for (uint32_t k = 0; k < kGcTasks; ++k) cacc[k] = make_double2(0.0, 0.0);

  for (uint32_t r = r0; r < r1; r += kGcTile) {
    const uint32_t nr = r1 - r < kGcTile ? r1 - r : kGcTile;
    if (G.vec) {
      for (uint32_t n = tid; n < kGcTile * kGcTile / 2; n += kGcThreads) {
        const uint32_t lr = n / (kGcTile / 2), lc = 2 * (n % (kGcTile / 2));
        if (lr < nr && lc < nc) {  // nc is even here
          const double2 v = *(const double2 *)(s + (size_t)(r + lr) * G.W + c0 + lc);
          tile[lr * kGcLd + lc] = v.x;
          tile[lr * kGcLd + lc + 1] = v.y;
        }
      }
    } else {
      for (uint32_t n = tid; n < kGcTile * kGcTile; n += kGcThreads) {
        const uint32_t lr = n / kGcTile, lc = n % kGcTile;
        if (lr < nr && lc < nc) tile[lr * kGcLd + lc] = s[(size_t)(r + lr) * G.W + c0 + lc];
      }
    }
    for (uint32_t u = tid; u < ntask; u += kGcThreads) {
      const uint32_t q = u / kGcTile, lr = u % kGcTile;
      if (lr < nr) {
        const uint32_t j = G.rot ? 2 * (r + lr) + p : r + lr;
        const double2 t = tab_x[(uint32_t)(((uint64_t)q * j) % G.Mx)];
        twr[u] = make_double2(t.x, -t.y);
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kGcTasks; ++k) {
      const uint32_t u = tid + k * kGcThreads, lc = u % kGcTile;
      if (u < ntask && lc < nc) {
        const double2 *t = twr + (u - lc);
        double2 a = cacc[k];
        for (uint32_t lr = 0; lr < nr; ++lr) {
          const double v = tile[lr * kGcLd + lc];
          a.x = __fma_rn(v, t[lr].x, a.x);
          a.y = __fma_rn(v, t[lr].y, a.y);
        }
        cacc[k] = a;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < kGcTasks; ++k) {
      const uint32_t u = (tid ^ (kGcThreads / 2)) + k * kGcThreads, lr = u % kGcTile;
      if (u < ntask && lr < nr) {
        const double2 *t = twc + (u - lr);
        const double *row = tile + lr * kGcLd;
        double2 a = make_double2(0.0, 0.0);
        for (uint32_t lc = 0; lc < nc; ++lc) {
          const double v = row[lc];
          a.x = __fma_rn(v, t[lc].x, a.x);
          a.y = __fma_rn(v, t[lc].y, a.y);
        }
        rp[(size_t)(u / kGcTile) * G.H + r + lr] = a;
      }
    }
    __syncthreads();
  }
  double2 *cp = colpart + (((size_t)b * G.np + p) * G.nband + band) * G.P * G.W;
#pragma unroll
  for (uint32_t k = 0; k < kGcTasks; ++k) {
    const uint32_t u = tid + k * kGcThreads, lc = u % kGcTile;
    if (u < ntask && lc < nc) cp[(size_t)(u / kGcTile) * G.W + c0 + lc] = cacc[k];
  }
}

// ---- (2) the gather -------------------------------------------------------------------------------------------------------------
// workgroup w < nblocks: chain w / per, tasks (w mod per) 256 .. + 255 of the chain's P (Mt + Mx).  S[b][P (Mt + Mx)]: S^t as P runs
// of Mt slices, then S^x as P runs of Mx.  The partials of a slice are added in ascending band (S^t) / chunk (S^x) order.
// Rotated: slice 2 a + p of direction t is column a of plane p, slice 2 r + p of direction x is row r of plane p.
__global__ void __launch_bounds__(kGcThreads)
    gff_gather_kernel(GcPlan G, uint64_t nblocks, uint32_t per, const double2 *__restrict__ colpart, const double2 *__restrict__ rowpart,
                      double2 *__restrict__ S) {
  const uint64_t wg = gc_block();
  if (wg >= nblocks) return;
  const uint64_t b = wg / per;
  const uint32_t u = (uint32_t)(wg % per) * kGcThreads + threadIdx.x, nt = G.P * G.Mt, ntot = G.P * (G.Mt + G.Mx);
  if (u >= ntot) return;
  double2 a = make_double2(0.0, 0.0);
  if (u < nt) {
    const uint32_t q = u / G.Mt, sl = u % G.Mt, p = G.rot ? sl & 1u : 0, col = G.rot ? sl >> 1 : sl;
    const double2 *cp = colpart + ((((size_t)b * G.np + p) * G.nband) * G.P + q) * G.W + col;
    for (uint32_t k = 0; k < G.nband; ++k) {
      const double2 v = cp[(size_t)k * G.P * G.W];
      a.x += v.x;
      a.y += v.y;
    }
  } else {
    const uint32_t v0 = u - nt, q = v0 / G.Mx, j = v0 % G.Mx, p = G.rot ? j & 1u : 0, row = G.rot ? j >> 1 : j;
    const double2 *rp = rowpart + ((((size_t)b * G.np + p) * G.nchunk) * G.P + q) * G.H + row;
    for (uint32_t k = 0; k < G.nchunk; ++k) {
      const double2 v = rp[(size_t)k * G.P * G.H];
      a.x += v.x;
      a.y += v.y;
    }
  }
  S[(size_t)b * ntot + u] = a;
}

// ---- (3) the lag pass -----------------------------------------------------------------------------------------------------------
// sum_i Re[S_i conj S_{(i + tau) mod M}] by one wave: lane l adds i = l, l + 64, .. ascending (a product and an FMA each), wave_sum
__device__ __forceinline__ double gc_lag(const double2 *g, uint32_t M, uint32_t tau, uint32_t lane) {
  double a = 0.0;
  for (uint32_t i = lane; i < M; i += kWave) {
    uint32_t k = i + tau;
    if (k >= M) k -= M;
    const double2 u = g[i], v = g[k];
    a += __fma_rn(u.y, v.y, u.x * v.x);
  }
  return wave_sum(a);
}

// workgroup w < nblocks: chain w / per, x = w mod per, per = P (nbt + nbx) with nb_d = ceil((M_d / 2 + 1) / 32) blocks of lags:
// direction t first, momentum-major, the block of lags fastest.  Wave w' takes the lags w', w' + 4, .. of the block.  LDS: the M_d
// slice sums of (direction, q) are copied to LDS first; else they are read where the gather left them.  out[b][n_out], C_t first,
// momentum-major, lag fastest; acc != NULL: acc[b][n_out][2] += (C, C C).
template <bool LDS>
__global__ void __launch_bounds__(kGcThreads)
    gff_lags_kernel(GcPlan G, uint64_t nblocks, double inv_n, const double2 *__restrict__ S, double *__restrict__ out,
                    double *__restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) double2 gc_lds[];
  const uint64_t wg = gc_block();
  if (wg >= nblocks) return;
  const uint32_t ntt = G.Mt / 2 + 1, ntx = G.Mx / 2 + 1;
  const uint32_t nbt = (ntt + kGcLagsPerBlock - 1) / kGcLagsPerBlock, nbx = (ntx + kGcLagsPerBlock - 1) / kGcLagsPerBlock;
  const uint32_t per = G.P * (nbt + nbx), x = (uint32_t)(wg % per);
  const uint64_t b = wg / per;
  const uint32_t d = x >= G.P * nbt, y = d ? x - G.P * nbt : x, nb = d ? nbx : nbt, q = y / nb, blk = y % nb;
  const uint32_t M = d ? G.Mx : G.Mt, ntau = d ? ntx : ntt, tau0 = blk * kGcLagsPerBlock;
  const uint32_t tau1 = tau0 + kGcLagsPerBlock < ntau ? tau0 + kGcLagsPerBlock : ntau;
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const double2 *g = S + (size_t)b * G.P * (G.Mt + G.Mx) + (d ? (size_t)G.P * G.Mt : 0) + (size_t)q * M;
  const size_t o = (size_t)b * G.P * (ntt + ntx) + (d ? (size_t)G.P * ntt : 0) + (size_t)q * ntau;
  if constexpr (LDS) {
    for (uint32_t k = threadIdx.x; k < M; k += kGcThreads) gc_lds[k] = g[k];
    __syncthreads();
  }
  for (uint32_t tau = tau0 + wave; tau < tau1; tau += kGcThreads / kWave) {
    const double v = gc_lag(LDS ? gc_lds : g, M, tau, lane);
    if (lane == 0) {
      const double C = v * inv_n;
      out[o + tau] = C;
      if (acc) {
        acc[2 * (o + tau)] += C;
        acc[2 * (o + tau) + 1] += C * C;
      }
    }
  }
}

namespace {

struct GcWork {
  size_t tab, colpart, rowpart, S, bytes;  // byte offsets of the four sections, and the total
};

struct GcLaunch {
  GcPlan G;
  GcWork w;
  uint64_t project_blocks, gather_blocks, lag_blocks;
  uint32_t gather_per;
};

// the checks every entry point shares; then the plan
int gc_check(uint32_t Mt, uint32_t Mx, uint32_t P) {
  MLMCPI_REQUIRE(Mt >= 2 && Mx >= 2 && Mt % 2 == 0 && Mx % 2 == 0, "the GFF correlator needs even extents >= 2 (got %u x %u)", Mt, Mx);
  MLMCPI_REQUIRE((uint64_t)Mt * Mx <= (1ull << 30), "lattice too large for 32-bit site indices");
  MLMCPI_REQUIRE(P > 0, "the GFF correlator needs at least one momentum");
  if (P > kGcMaxP) return fail(MLMCPI_ERR_UNSUPPORTED, "the GFF correlator is built for up to %u momenta (got %u)", kGcMaxP, P);
  MLMCPI_REQUIRE(P <= Mt / 2 + 1 && P <= Mx / 2 + 1, "%u momenta are more than the %u x %u lattice has up to its Nyquist momentum", P, Mt, Mx);
  return MLMCPI_OK;
}

int gc_launch(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t P, uint32_t B, GcLaunch *out) {
  if (int rc = gc_check(Mt, Mx, P)) return rc;
  MLMCPI_REQUIRE(B > 0, "the GFF correlator needs n_chains > 0");
  GcLaunch L;
  L.G = gc_plan(Mt, Mx, rotated, P);
  const GcPlan &G = L.G;
  L.project_blocks = (uint64_t)B * G.np * G.nband * G.nchunk;
  L.gather_per = (P * (Mt + Mx) + kGcThreads - 1) / kGcThreads;
  L.gather_blocks = (uint64_t)B * L.gather_per;
  const uint32_t nbt = (Mt / 2 + 1 + kGcLagsPerBlock - 1) / kGcLagsPerBlock, nbx = (Mx / 2 + 1 + kGcLagsPerBlock - 1) / kGcLagsPerBlock;
  L.lag_blocks = (uint64_t)B * P * (nbt + nbx);
  const uint64_t most = L.project_blocks > L.gather_blocks ? (L.project_blocks > L.lag_blocks ? L.project_blocks : L.lag_blocks)
                                                           : (L.gather_blocks > L.lag_blocks ? L.gather_blocks : L.lag_blocks);
  MLMCPI_REQUIRE(most <= kGcMaxBlocks, "the GFF correlator takes at most %llu workgroups per launch (these chains need %llu)",
                 (unsigned long long)kGcMaxBlocks, (unsigned long long)most);
  L.w.tab = 0;
  L.w.colpart = align256(((size_t)Mt + Mx) * sizeof(double2));
  L.w.rowpart = L.w.colpart + align256((size_t)B * G.np * G.nband * P * G.W * sizeof(double2));
  L.w.S = L.w.rowpart + align256((size_t)B * G.np * G.nchunk * P * G.H * sizeof(double2));
  L.w.bytes = L.w.S + align256((size_t)B * P * (Mt + Mx) * sizeof(double2));
  *out = L;
  return MLMCPI_OK;
}

inline dim3 gc_grid(uint64_t blocks) {
  const uint32_t gx = blocks < kGcGridX ? (uint32_t)blocks : kGcGridX;
  return dim3(gx, (uint32_t)((blocks + gx - 1) / gx));
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_gff_correlator_size(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t *n_out) {
  (void)rotated;
  if (int rc = gc_check(Mt, Mx, n_mom)) return rc;
  MLMCPI_REQUIRE(n_out, "bad arguments");
  *n_out = n_mom * (Mt / 2 + 1) + n_mom * (Mx / 2 + 1);
  return MLMCPI_OK;
}

int mlmcpi_gff_correlator_workspace_bytes(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t n_chains, size_t *bytes) {
  GcLaunch L;
  if (int rc = gc_launch(Mt, Mx, rotated, n_mom, n_chains, &L)) return rc;
  MLMCPI_REQUIRE(bytes, "bad arguments");
  *bytes = L.w.bytes;
  return MLMCPI_OK;
}

int mlmcpi_gff_correlator_plan(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, uint32_t n_chains,
                               mlmcpi_gff_correlator_plan_info *out) {
  GcLaunch L;
  if (int rc = gc_launch(Mt, Mx, rotated, n_mom, n_chains, &L)) return rc;
  MLMCPI_REQUIRE(out, "bad arguments");
  const uint32_t Mmax = Mt > Mx ? Mt : Mx;
  out->work_bytes = L.w.bytes;
  out->grid = L.project_blocks;
  out->gather_grid = L.gather_blocks;
  out->lag_grid = L.lag_blocks;
  out->workgroup = kGcThreads;
  out->tile = kGcTile;
  out->band_rows = kGcBand;
  out->planes = L.G.np;
  out->plane_w = L.G.W;
  out->plane_h = L.G.H;
  out->chunks = L.G.nchunk;
  out->bands = L.G.nband;
  out->vector_loads = L.G.vec;
  out->table_entries = Mt + Mx;
  out->lags_per_workgroup = kGcLagsPerBlock;
  out->lags_in_lds = Mmax <= kGcLdsExtent;
  out->lds_bytes = kGcProjectLds;
  out->lag_lds_bytes = Mmax <= kGcLdsExtent ? Mmax * (uint32_t)sizeof(double2) : 0;
  out->lds_limit = kGcLdsBytes;
  return MLMCPI_OK;
}

int mlmcpi_gff_correlator(uint32_t Mt, uint32_t Mx, int32_t rotated, uint32_t n_mom, const double *d_phi, uint32_t n_chains,
                          double *d_out, double *d_acc, void *d_work, size_t work_bytes, void *stream) {
  GcLaunch L;
  if (int rc = gc_launch(Mt, Mx, rotated, n_mom, n_chains, &L)) return rc;
  MLMCPI_REQUIRE(d_phi && d_out && d_work, "bad arguments");
  MLMCPI_REQUIRE(((uintptr_t)d_phi & 15) == 0 && ((uintptr_t)d_work & 15) == 0, "the GFF correlator needs d_phi and d_work on 16 bytes");
  MLMCPI_REQUIRE(work_bytes >= L.w.bytes, "the GFF correlator's workspace is too small (%zu bytes, needs %zu)", work_bytes, L.w.bytes);
  hipStream_t st = as_stream(stream);
  const GcPlan &G = L.G;
  double2 *tab = (double2 *)((char *)d_work + L.w.tab), *colpart = (double2 *)((char *)d_work + L.w.colpart);
  double2 *rowpart = (double2 *)((char *)d_work + L.w.rowpart), *S = (double2 *)((char *)d_work + L.w.S);
  const dim3 block(kGcThreads);
  hipLaunchKernelGGL(gff_twiddle_kernel, dim3((uint32_t)(((uint64_t)Mt + Mx + kGcThreads - 1) / kGcThreads)), block, 0, st, Mt, Mx, tab);
  MLMCPI_LAUNCH_CHECK("gff_twiddle_kernel");
  hipLaunchKernelGGL(gff_project_kernel, gc_grid(L.project_blocks), block, 0, st, G, L.project_blocks, d_phi, (const double2 *)tab,
                     colpart, rowpart);
  MLMCPI_LAUNCH_CHECK("gff_project_kernel");
  hipLaunchKernelGGL(gff_gather_kernel, gc_grid(L.gather_blocks), block, 0, st, G, L.gather_blocks, L.gather_per,
                     (const double2 *)colpart, (const double2 *)rowpart, S);
  MLMCPI_LAUNCH_CHECK("gff_gather_kernel");
  const uint32_t Mmax = Mt > Mx ? Mt : Mx;
  const double inv_n = 1.0 / (double)G.nvert;
  if (Mmax <= kGcLdsExtent)
    hipLaunchKernelGGL(gff_lags_kernel<true>, gc_grid(L.lag_blocks), block, (size_t)Mmax * sizeof(double2), st, G, L.lag_blocks, inv_n,
                       (const double2 *)S, d_out, d_acc);
  else
    hipLaunchKernelGGL(gff_lags_kernel<false>, gc_grid(L.lag_blocks), block, 0, st, G, L.lag_blocks, inv_n, (const double2 *)S, d_out, d_acc);
  MLMCPI_LAUNCH_CHECK("gff_lags_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
