// path_correlator.hip -- the time correlator C(tau) of the 1-D path actions (include/mlmcpi_hip.h: mlmcpi_path_correlator*;
// DESIGN.md 4.2a).
//
//   kinds 0, 1 (oscillators)  C(tau) = (1/M) sum_j x_j x_{(j + tau) mod M}
//   kind 2 (rotor)            C(tau) = (1/M) sum_j cos(x_j - x_{(j + tau) mod M}) = (1/M) sum_j (c_j c_{j+tau} + s_j s_{j+tau})
// for tau = 0 .. n_lag - 1: a circular autocorrelation of 1 or 2 components per site, (c, s) from one sincos per staged site.
//
// Sites and lags are cut into tiles of kPcJ = 8 sites and kPcT = 8 lags.  A segment of a path owns `own_tiles` site tiles from
// its first site seg0; its LDS image holds the own_tiles + lag_tiles tiles from seg0 on, every site of it a copy of
// x[(seg0 + i) mod M] (the wrap is resolved here, at load time), one fp64 plane per component, a tile at a stride of kPcStride =
// 10 doubles (80 bytes: the 16-byte slots of 16 lanes that read consecutive tiles are distinct, so the ds_read_b128 of a tile
// is conflict-free).  The pair (site tile s, lag tile q) needs the tile s (sites beyond the owned range count as zero) and the
// window of 15 sites from 8 (s + q) on -- the tiles s + q and s + q + 1 -- and is 64 FMAs per component into 8 accumulators:
//   acc[t] = fma(a_j, w_{j + t}, acc[t]),  j = 0 .. 7 ascending (rotor: the c term, then the s term, of each j)
// A group of G lanes (a power of two, <= 64) takes a lag tile q: lane g adds the site tiles g, g + G, .. ascending, then the
// lanes are added by the shuffle tree (offsets G/2, .., 1; wave_sum for G = 64).  A team of `wpc` waves serves one chain; its
// 64 wpc / G groups take the lag tiles round robin.  A path of one segment is finished there (C = sum / M); a longer path leaves
// partial[b][seg][n_lag] and path_correlator_finish_kernel adds the segments in ascending order.  The geometry (pc_plan) is a
// function of (kind, M, n_lag) alone and no sum is taken by atomics: a chain's output is the same bits whatever the batch, the
// split of the chains over calls and the stream.
#include "path_common.hpp"

#pragma clang fp contract(off)

namespace mlmcpi {

constexpr uint32_t kPcThreads = 256;      // workgroup of both kernels: four waves
constexpr uint32_t kPcJ = 8, kPcT = 8;    // sites x lags of a lane's register tile
constexpr uint32_t kPcStride = 10;        // doubles from a tile of the LDS image to the next
constexpr uint32_t kPcLdsBytes = 65536;   // LDS a workgroup may take (two workgroups per CU)
constexpr uint32_t kPcGridX = (1u << 31) / kPcThreads;  // workgroups along x of a launch; beyond, the grid grows along y
constexpr uint64_t kPcMaxBlocks = (uint64_t)kPcGridX * 65535;

struct PcPlan {
  uint32_t ncomp, M, n_lag;
  uint32_t lag_tiles, own_tiles, image_tiles, nseg;  // tiles of 8: lags, owned sites of a segment, its LDS image; segments
  uint32_t wpc, cpw, G;                              // waves per chain, chains per workgroup, lanes of a group
  uint32_t lds_bytes;
};

inline uint32_t pc_max_tiles(uint32_t ncomp) { return kPcLdsBytes / (kPcStride * 8 * ncomp); }  // 819, rotor 409

// MLMCPI_ERR_UNSUPPORTED: the halo of n_lag lags leaves no room for a site tile
inline int pc_plan(int kind, uint32_t M, uint32_t n_lag, PcPlan *pl) {
  PcPlan p;
  p.ncomp = kind == MLMCPI_ROTOR ? 2 : 1;
  p.M = M;
  p.n_lag = n_lag;
  const uint32_t max_tiles = pc_max_tiles(p.ncomp), tiles = (M + kPcJ - 1) / kPcJ;
  p.lag_tiles = (n_lag + kPcT - 1) / kPcT;
  if (p.lag_tiles + 1 > max_tiles)
    return fail(MLMCPI_ERR_UNSUPPORTED, "the path correlator takes at most %u lags of this action (got %u)", kPcT * (max_tiles - 1), n_lag);
  if (tiles + p.lag_tiles <= max_tiles) {
    p.nseg = 1;
    p.own_tiles = tiles;
  } else {
    const uint32_t own_max = max_tiles - p.lag_tiles, n = (tiles + own_max - 1) / own_max;
    p.own_tiles = (tiles + n - 1) / n;
    p.nseg = (tiles + p.own_tiles - 1) / p.own_tiles;
  }
  p.image_tiles = p.own_tiles + p.lag_tiles;
  const bool packed = p.nseg == 1 && p.own_tiles * p.lag_tiles <= 256 && p.image_tiles <= max_tiles / 4;
  p.wpc = packed ? 1 : 4;
  p.cpw = 4 / p.wpc;
  p.G = 1;
  while (p.G < 64 && p.G < p.own_tiles) p.G *= 2;
  p.lds_bytes = p.cpw * p.ncomp * p.image_tiles * kPcStride * 8;
  *pl = p;
  return MLMCPI_OK;
}

typedef double pc_d2 __attribute__((ext_vector_type(2)));

// the 8 doubles of a tile / the 16 of two consecutive tiles, as 16-byte reads
__device__ __forceinline__ void pc_read_tile(const double *t, double (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const pc_d2 u = *reinterpret_cast<const pc_d2 *>(t + 2 * k);
    v[2 * k] = u.x;
    v[2 * k + 1] = u.y;
  }
}
__device__ __forceinline__ void pc_read_window(const double *t, double (&w)[16]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const pc_d2 u = *reinterpret_cast<const pc_d2 *>(t + 2 * k), v = *reinterpret_cast<const pc_d2 *>(t + kPcStride + 2 * k);
    w[2 * k] = u.x;
    w[2 * k + 1] = u.y;
    w[8 + 2 * k] = v.x;
    w[8 + 2 * k + 1] = v.y;
  }
}

// workgroup w = blockIdx.y gridDim.x + blockIdx.x < nblocks: segment w mod nseg of the chains (w / nseg) cpw + team, team =
// thread / (64 wpc).
//   NSEG1: out[b][n_lag] = sum / M and, acc != NULL, acc[b][n_lag][2] += (C, C C); else partial[(b nseg + seg) n_lag + tau] = sum
template <int NCOMP, bool NSEG1>
__global__ void __launch_bounds__(kPcThreads)
    path_correlator_kernel(PcPlan P, uint64_t nblocks, const double *__restrict__ x, uint32_t B, double *__restrict__ out,
                           double *__restrict__ acc) {
  extern __shared__ __attribute__((aligned(16))) double pc_lds[];
  const uint64_t wg = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (wg >= nblocks) return;
  const uint32_t team_threads = P.wpc * kWave, team = threadIdx.x / team_threads, tl = threadIdx.x % team_threads;
  const uint32_t seg = NSEG1 ? 0 : (uint32_t)(wg % P.nseg);
  const uint64_t b = (NSEG1 ? wg : wg / P.nseg) * P.cpw + team;
  const uint32_t plane = P.image_tiles * kPcStride;
  double *img = pc_lds + (size_t)team * NCOMP * plane;
  const uint32_t seg0 = seg * P.own_tiles * kPcJ;
  const uint32_t own = P.M - seg0 < P.own_tiles * kPcJ ? P.M - seg0 : P.own_tiles * kPcJ;  // owned sites of this segment
  if (b < B) {
    const double *xb = x + (size_t)b * P.M;
    for (uint32_t i = tl; i < P.image_tiles * kPcJ; i += team_threads) {
      uint64_t k = (uint64_t)seg0 + i;
      if (k >= P.M) {
        k -= P.M;
        if (k >= P.M) k %= P.M;
      }
      const uint32_t q = (i / kPcJ) * kPcStride + i % kPcJ;
      if (NCOMP == 2) {
        double sn, cs;
        sincos(xb[k], &sn, &cs);
        img[q] = cs;
        img[plane + q] = sn;
      } else {
        img[q] = xb[k];
      }
    }
  }
  __syncthreads();
  if (b >= B) return;
  const uint32_t g = tl % P.G, grp = tl / P.G, ngrp = team_threads / P.G;
  for (uint32_t q = grp; q < P.lag_tiles; q += ngrp) {
    double a[kPcT];
#pragma unroll
    for (int t = 0; t < (int)kPcT; ++t) a[t] = 0.0;
    for (uint32_t s = g; s < P.own_tiles; s += P.G) {
      double u[NCOMP][8], w[NCOMP][16];
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) {
        pc_read_tile(img + c * plane + s * kPcStride, u[c]);
        pc_read_window(img + c * plane + (s + q) * kPcStride, w[c]);
      }
      if (s * kPcJ + kPcJ > own) {  // the last tile of the path: sites beyond it count as zero
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (s * kPcJ + j >= own) u[c][j] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
#pragma unroll
          for (int t = 0; t < 8; ++t) a[t] = __fma_rn(u[c][j], w[c][j + t], a[t]);
    }
#pragma unroll
    for (int t = 0; t < (int)kPcT; ++t) {
      if (P.G == kWave) {
        a[t] = wave_sum(a[t]);
      } else {
        for (uint32_t off = P.G / 2; off > 0; off >>= 1) a[t] += __shfl_down(a[t], off, kWave);
      }
    }
    if (g == 0) {
#pragma unroll
      for (int t = 0; t < (int)kPcT; ++t) {
        const uint32_t tau = q * kPcT + t;
        if (tau < P.n_lag) {
          if (NSEG1) {
            const size_t o = (size_t)b * P.n_lag + tau;
            const double C = a[t] / (double)P.M;
            out[o] = C;
            if (acc) {
              acc[2 * o] += C;
              acc[2 * o + 1] += C * C;
            }
          } else {
            out[((size_t)b * P.nseg + seg) * P.n_lag + tau] = a[t];
          }
        }
      }
    }
  }
}

// entry e < B n_lag (grid stride): the partials of its chain and lag added in ascending segment order, then / M
__global__ void __launch_bounds__(kPcThreads)
    path_correlator_finish_kernel(uint32_t M, uint32_t n_lag, uint32_t nseg, size_t n, const double *__restrict__ partial,
                                  double *__restrict__ out, double *__restrict__ acc) {
  for (size_t e = (size_t)blockIdx.x * kPcThreads + threadIdx.x; e < n; e += (size_t)gridDim.x * kPcThreads) {
    const size_t b = e / n_lag, tau = e % n_lag;
    const double *p = partial + b * nseg * n_lag + tau;
    double s = 0.0;
    for (uint32_t k = 0; k < nseg; ++k) s += p[(size_t)k * n_lag];
    const double C = s / (double)M;
    out[e] = C;
    if (acc) {
      acc[2 * e] += C;
      acc[2 * e + 1] += C * C;
    }
  }
}

namespace {

// the checks every entry point shares; then the plan
int pc_check(const mlmcpi_path_action *act, uint32_t n_lag, uint32_t B, PcPlan *pl, uint64_t *blocks, size_t *work_bytes) {
  MLMCPI_REQUIRE(act, "action is NULL");
  MLMCPI_REQUIRE(act->kind >= MLMCPI_HARMONIC && act->kind <= MLMCPI_ROTOR, "kind %d is not a 1-D path action", act->kind);
  MLMCPI_REQUIRE(act->M > 0 && B > 0 && n_lag > 0, "the path correlator needs M, B, n_lag > 0 (got %u, %u, %u)", act->M, B, n_lag);
  MLMCPI_REQUIRE(n_lag <= act->M / 2 + 1, "n_lag = %u beyond M / 2 + 1 = %u", n_lag, act->M / 2 + 1);
  if (int rc = pc_plan(act->kind, act->M, n_lag, pl)) return rc;
  *blocks = (uint64_t)((B + pl->cpw - 1) / pl->cpw) * pl->nseg;
  MLMCPI_REQUIRE(*blocks <= kPcMaxBlocks, "the path correlator takes at most %llu workgroups per call (these chains need %llu)",
                 (unsigned long long)kPcMaxBlocks, (unsigned long long)*blocks);
  *work_bytes = pl->nseg > 1 ? align256((size_t)B * pl->nseg * n_lag * sizeof(double)) : 256;
  return MLMCPI_OK;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_path_correlator_workspace_bytes(const mlmcpi_path_action *act, uint32_t n_lag, uint32_t B, size_t *bytes) {
  PcPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = pc_check(act, n_lag, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(bytes, "bad arguments");
  *bytes = wb;
  return MLMCPI_OK;
}

int mlmcpi_path_correlator_plan(const mlmcpi_path_action *act, uint32_t n_lag, uint32_t B, mlmcpi_path_correlator_plan_info *out) {
  PcPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = pc_check(act, n_lag, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(out, "bad arguments");
  out->work_bytes = wb;
  out->workgroup = kPcThreads;
  out->chains_per_workgroup = pl.cpw;
  out->waves_per_chain = pl.wpc;
  out->group = pl.G;
  out->owned = pl.nseg == 1 ? act->M : pl.own_tiles * kPcJ;
  out->nseg = pl.nseg;
  out->J = kPcJ;
  out->T = kPcT;
  out->lag_tiles = pl.lag_tiles;
  out->image_tiles = pl.image_tiles;
  out->components = pl.ncomp;
  out->lds_bytes = pl.lds_bytes;
  out->lds_limit = kPcLdsBytes;
  out->grid = blocks;
  return MLMCPI_OK;
}

int mlmcpi_path_correlator(const mlmcpi_path_action *act, const double *d_x, uint32_t B, uint32_t n_lag, double *d_out, double *d_acc,
                           void *d_work, size_t work_bytes, void *stream) {
  PcPlan pl;
  uint64_t blocks;
  size_t wb;
  if (int rc = pc_check(act, n_lag, B, &pl, &blocks, &wb)) return rc;
  MLMCPI_REQUIRE(d_x && d_out && d_work, "bad arguments");
  MLMCPI_REQUIRE(work_bytes >= wb, "the path correlator's workspace is too small (%zu bytes, needs %zu)", work_bytes, wb);
  hipStream_t st = as_stream(stream);
  const uint32_t gx = blocks < kPcGridX ? (uint32_t)blocks : kPcGridX;
  const dim3 grid(gx, (uint32_t)((blocks + gx - 1) / gx)), block(kPcThreads);
  if (pl.nseg == 1) {
    if (pl.ncomp == 1)
      hipLaunchKernelGGL((path_correlator_kernel<1, true>), grid, block, pl.lds_bytes, st, pl, blocks, d_x, B, d_out, d_acc);
    else
      hipLaunchKernelGGL((path_correlator_kernel<2, true>), grid, block, pl.lds_bytes, st, pl, blocks, d_x, B, d_out, d_acc);
    MLMCPI_LAUNCH_CHECK("path_correlator_kernel");
    return MLMCPI_OK;
  }
  double *partial = (double *)d_work;
  if (pl.ncomp == 1)
    hipLaunchKernelGGL((path_correlator_kernel<1, false>), grid, block, pl.lds_bytes, st, pl, blocks, d_x, B, partial, (double *)nullptr);
  else
    hipLaunchKernelGGL((path_correlator_kernel<2, false>), grid, block, pl.lds_bytes, st, pl, blocks, d_x, B, partial, (double *)nullptr);
  MLMCPI_LAUNCH_CHECK("path_correlator_kernel");
  const size_t n = (size_t)B * n_lag;
  const size_t fb = (n + kPcThreads - 1) / kPcThreads;
  hipLaunchKernelGGL(path_correlator_finish_kernel, dim3((uint32_t)(fb < 65536 ? fb : 65536)), block, 0, st, act->M, n_lag, pl.nseg, n,
                     (const double *)partial, d_out, d_acc);
  MLMCPI_LAUNCH_CHECK("path_correlator_finish_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
