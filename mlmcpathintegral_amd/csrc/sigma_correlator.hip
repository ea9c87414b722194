// sigma_correlator.hip -- the zero-momentum (time-slice) two-point function of the O(3) nonlinear sigma model on a level of
// its CoarsenRotate hierarchy (include/mlmcpi_hip.h: mlmcpi_sigma_level_correlator*).
//
//   S^t_i = sum_j sigma(i, j),  S^x_j = sum_i sigma(i, j)                      (slice sums over the vertices of the level)
//   C_t(tau) = (1/N) sum_i S^t_i . S^t_{(i + tau) mod Mt},  tau = 0 .. Mt/2;   C_x likewise along j
//
// Three launches.  (1) The slice-sum pass reads the state ONCE: a level is one plane (unrotated: W x H = Mt x Mx, index W r + c)
// or two (rotated: E and O, W x H = ht x hx each; plane p holds the vertices (2 c + p, 2 r + p)); a workgroup takes a band of
// kCorrBandRows rows of a chunk of cw columns of one plane of one chain, tile by tile through LDS, and leaves the column sums of
// its band and the row sums of its chunk.  (2) The gather adds a slice's partials in ascending band / chunk order.  (3) The
// correlator pass gives every tau to one wave.  The geometry (corr_geom) is a function of the level alone and no sum is taken
// by atomics, so every output is the same bits whatever the batch and however the chains are split over calls.
#include "internal.hpp"

#include "sigma_level_device.hpp"  // fp contraction is off from here on

namespace mlmcpi {

constexpr uint32_t kCorrThreads = 256;    // workgroup of all three kernels
constexpr uint32_t kCorrTile = 1024;      // vertices of a tile of the slice-sum pass: cw columns x kCorrTile / cw rows
constexpr uint32_t kCorrTileLds = 1088;   // doubles per component of the tile: rows of <= 32 columns are padded by one
constexpr uint32_t kCorrBandRows = 64;    // rows of a band (a multiple of every tile height)
constexpr uint32_t kCorrTauPerBlock = 32; // lags per workgroup of the correlator pass, eight per wave
constexpr uint32_t kCorrLdsExtent = 2048; // the correlator pass keeps the slice sums of an extent <= this in LDS (48 KiB)

struct CorrGeom {
  uint32_t W, H, np;        // plane: W columns (the contiguous index), H rows; np planes
  uint32_t cw, lg, tr, ld;  // tile: cw = 2^lg columns (16 .. 256), tr = kCorrTile / cw rows, ld = its row stride in LDS
  uint32_t nchunk, nband;   // chunks of cw columns, bands of kCorrBandRows rows
};

inline CorrGeom corr_geom(const SigmaLevel &L) {
  CorrGeom G;
  G.W = L.rot ? L.ht : L.Mt;
  G.H = L.rot ? L.hx : L.Mx;
  G.np = L.rot ? 2 : 1;
  G.lg = 4;
  while (G.lg < 8 && (1u << G.lg) < G.W) ++G.lg;
  G.cw = 1u << G.lg;
  G.tr = kCorrTile / G.cw;
  G.ld = G.cw <= 32 ? G.cw + 1 : G.cw;
  G.nchunk = (G.W + G.cw - 1) / G.cw;
  G.nband = (G.H + kCorrBandRows - 1) / kCorrBandRows;
  return G;
}

// ---- (1) the slice-sum pass --------------------------------------------------------------------------------------------
// workgroup x of chain blockIdx.y: chunk = x mod nchunk, band = (x / nchunk) mod nband, plane = x / (nchunk nband).
//   colpart[(((b np + p) nband + band) W + col) 3 + c]    the band's sum of column col, rows ascending
//   rowpart[(((b np + p) nchunk + chunk) H + row) 3 + c]  the chunk's sum of row `row`: cw <= 32: columns ascending; else lane l
//                                                         of a wave adds columns l, l + 64, .. ascending, then wave_sum
// A tile is loaded as coalesced double2 reads (thread t: entries t, t + 256, ..; a row of the tile is cw consecutive vertices)
// and stored as unit vectors, three SoA planes; entries beyond the plane are zero.
__global__ void __launch_bounds__(kCorrThreads)
    sigma_slice_sum_kernel(CorrGeom G, uint32_t nvert, const double2 *__restrict__ state, double *__restrict__ colpart,
                           double *__restrict__ rowpart) {
  __shared__ double tile[3][kCorrTileLds];
  const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave, b = blockIdx.y;
  const uint32_t chunk = blockIdx.x % G.nchunk, band = (blockIdx.x / G.nchunk) % G.nband, p = blockIdx.x / (G.nchunk * G.nband);
  const uint32_t c0 = chunk * G.cw, r0 = band * kCorrBandRows;
  const uint32_t r1 = r0 + kCorrBandRows < G.H ? r0 + kCorrBandRows : G.H;
  const double2 *s = state + (size_t)b * nvert + (size_t)p * G.W * G.H;
  double *rp = rowpart + (((size_t)b * G.np + p) * G.nchunk + chunk) * G.H * 3;

  double cacc[3] = {0.0, 0.0, 0.0};  // column task u = tid + 256 k < 3 cw: column u mod cw, component u / cw
  for (uint32_t r = r0; r < r1; r += G.tr) {
    const uint32_t nr = r1 - r < G.tr ? r1 - r : G.tr;
    for (uint32_t k = 0; k < kCorrTile / kCorrThreads; ++k) {
      const uint32_t idx = tid + k * kCorrThreads, lc = idx & (G.cw - 1), lr = idx >> G.lg;
      V3 v{0.0, 0.0, 0.0};
      if (c0 + lc < G.W && lr < nr) v = sigma_of(s[(size_t)(r + lr) * G.W + c0 + lc]);
      const uint32_t q = lr * G.ld + lc;
      tile[0][q] = v.x;
      tile[1][q] = v.y;
      tile[2][q] = v.z;
    }
    __syncthreads();
    for (uint32_t k = 0; k < 3; ++k) {
      const uint32_t u = tid + k * kCorrThreads;
      if (u < 3 * G.cw) {
        const double *t = tile[u >> G.lg] + (u & (G.cw - 1));
        double a = cacc[k];
        for (uint32_t lr = 0; lr < nr; ++lr) a += t[lr * G.ld];
        cacc[k] = a;
      }
    }
    if (G.cw <= 32) {  // row task tid < 3 tr: row tid mod tr, component tid / tr
      const uint32_t lr = tid % G.tr, c = tid / G.tr;
      if (c < 3 && lr < nr) {
        const double *t = tile[c] + lr * G.ld;
        double a = 0.0;
        for (uint32_t lc = 0; lc < G.cw; ++lc) a += t[lc];
        rp[(size_t)(r + lr) * 3 + c] = a;
      }
    } else {
      for (uint32_t lr = wave; lr < nr; lr += kCorrThreads / kWave)
        for (uint32_t c = 0; c < 3; ++c) {
          const double *t = tile[c] + lr * G.ld;
          double a = 0.0;
          for (uint32_t lc = lane; lc < G.cw; lc += kWave) a += t[lc];
          a = wave_sum(a);
          if (lane == 0) rp[(size_t)(r + lr) * 3 + c] = a;
        }
    }
    __syncthreads();
  }
  double *cp = colpart + (((size_t)b * G.np + p) * G.nband + band) * G.W * 3;
  for (uint32_t k = 0; k < 3; ++k) {
    const uint32_t u = tid + k * kCorrThreads, col = c0 + (u & (G.cw - 1));
    if (u < 3 * G.cw && col < G.W) cp[(size_t)col * 3 + (u >> G.lg)] = cacc[k];
  }
}

// ---- (2) the gather -----------------------------------------------------------------------------------------------------
// slice sums of chain blockIdx.y, S[b][3 (Mt + Mx)]: S^t as three runs of Mt (x, y, z), then S^x as three runs of Mx.  Task
// u < 3 (Mt + Mx): slice u / 3, component u mod 3; the partials of a slice are added in ascending band (S^t) / chunk (S^x)
// order.  Rotated: slice 2 a + p of direction t is column a of plane p, slice 2 r + p of direction x is row r of plane p.
__global__ void __launch_bounds__(kCorrThreads)
    sigma_slice_gather_kernel(CorrGeom G, uint32_t Mt, uint32_t Mx, const double *__restrict__ colpart,
                              const double *__restrict__ rowpart, double *__restrict__ S) {
  const uint32_t b = blockIdx.y, u = blockIdx.x * kCorrThreads + threadIdx.x;
  if (u >= 3 * (Mt + Mx)) return;
  const uint32_t sl = u / 3, c = u % 3;
  double *out = S + (size_t)b * 3 * (Mt + Mx);
  double a = 0.0;
  if (sl < Mt) {
    const uint32_t p = G.np == 2 ? sl & 1u : 0, col = G.np == 2 ? sl >> 1 : sl;
    const double *cp = colpart + ((size_t)b * G.np + p) * G.nband * G.W * 3 + (size_t)col * 3 + c;
    for (uint32_t k = 0; k < G.nband; ++k) a += cp[(size_t)k * G.W * 3];
    out[(size_t)c * Mt + sl] = a;
  } else {
    const uint32_t j = sl - Mt, p = G.np == 2 ? j & 1u : 0, row = G.np == 2 ? j >> 1 : j;
    const double *rp = rowpart + ((size_t)b * G.np + p) * G.nchunk * G.H * 3 + (size_t)row * 3 + c;
    for (uint32_t k = 0; k < G.nchunk; ++k) a += rp[(size_t)k * G.H * 3];
    out[(size_t)3 * Mt + (size_t)c * Mx + j] = a;
  }
}

// ---- (3) the correlator pass ----------------------------------------------------------------------------------------------
// sum_i S_i . S_{(i + tau) mod M} by one wave: lane l adds i = l, l + 64, .. ascending (dot3 each), then wave_sum
__device__ __forceinline__ double corr_lag(const double *sx, const double *sy, const double *sz, uint32_t M, uint32_t tau, uint32_t lane) {
  double a = 0.0;
  for (uint32_t i = lane; i < M; i += kWave) {
    uint32_t k = i + tau;
    if (k >= M) k -= M;
    a += dot3(V3{sx[i], sy[i], sz[i]}, V3{sx[k], sy[k], sz[k]});
  }
  return wave_sum(a);
}

// workgroup (x, d, b): lags [x kCorrTauPerBlock, (x + 1) kCorrTauPerBlock) of direction d (0: t, 1: x) of chain b, wave w the
// lags w, w + 4, .. of them.  LDS: the direction's slice sums are copied to LDS first (3 M doubles, dynamic); else they are read
// where the gather left them.  out[b][n_out], C_t first; the scale 1/N is applied last.  acc != NULL: acc[b][n_out][2] += (C, C C).
template <bool LDS>
__global__ void __launch_bounds__(kCorrThreads)
    sigma_correlator_kernel(uint32_t Mt, uint32_t Mx, double inv_n, const double *__restrict__ S, double *__restrict__ out,
                            double *__restrict__ acc) {
  extern __shared__ double corr_lds[];
  const uint32_t d = blockIdx.y, b = blockIdx.z, M = d ? Mx : Mt, ntau = M / 2 + 1, tau0 = blockIdx.x * kCorrTauPerBlock;
  if (tau0 >= ntau) return;  // the grid is sized for the longer direction
  const uint32_t tau1 = tau0 + kCorrTauPerBlock < ntau ? tau0 + kCorrTauPerBlock : ntau;
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave, n_out = Mt / 2 + Mx / 2 + 2;
  const double *g = S + (size_t)b * 3 * (Mt + Mx) + (d ? (size_t)3 * Mt : 0);
  const size_t o = (size_t)b * n_out + (d ? Mt / 2 + 1 : 0);
  if constexpr (LDS) {
    for (uint32_t k = threadIdx.x; k < 3 * M; k += kCorrThreads) corr_lds[k] = g[k];
    __syncthreads();
  }
  for (uint32_t tau = tau0 + wave; tau < tau1; tau += kCorrThreads / kWave) {
    double v;
    if constexpr (LDS) v = corr_lag(corr_lds, corr_lds + M, corr_lds + 2 * M, M, tau, lane);
    else v = corr_lag(g, g + M, g + 2 * (size_t)M, M, tau, lane);
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

struct CorrWork {
  size_t colpart, rowpart, S, bytes;  // byte offsets of the three sections, and the total
};

CorrWork corr_work(const SigmaLevel &L, const CorrGeom &G, uint32_t B) {
  CorrWork w;
  w.colpart = 0;
  w.rowpart = align256((size_t)B * G.np * G.nband * G.W * 3 * sizeof(double));
  w.S = w.rowpart + align256((size_t)B * G.np * G.nchunk * G.H * 3 * sizeof(double));
  w.bytes = w.S + align256((size_t)B * 3 * (L.Mt + L.Mx) * sizeof(double));
  return w;
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_sigma_level_correlator_size(const mlmcpi_sigma_level *level, uint32_t *n_out) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(n_out, "bad arguments");
  *n_out = level->Mt / 2 + level->Mx / 2 + 2;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_correlator_workspace_bytes(const mlmcpi_sigma_level *level, uint32_t B, size_t *bytes) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0 && B <= 65535, "bad arguments");
  const SigmaLevel L = make_level(*level);
  *bytes = corr_work(L, corr_geom(L), B).bytes;
  return MLMCPI_OK;
}

int mlmcpi_sigma_level_correlator(const mlmcpi_sigma_level *level, const double *d_state, uint32_t B, double *d_out, double *d_acc,
                                  void *d_work, size_t work_bytes, void *stream) {
  if (int rc = check_sigma_level(level)) return rc;
  MLMCPI_REQUIRE(d_state && d_out && d_work, "bad arguments");
  MLMCPI_REQUIRE(B > 0 && B <= 65535, "the correlator takes 1 .. 65535 chains per call (got %u)", B);
  const SigmaLevel L = make_level(*level);
  const CorrGeom G = corr_geom(L);
  const CorrWork w = corr_work(L, G, B);
  MLMCPI_REQUIRE(work_bytes >= w.bytes, "the correlator's workspace is too small (%zu bytes, needs %zu)", work_bytes, w.bytes);
  hipStream_t st = as_stream(stream);
  double *colpart = (double *)((char *)d_work + w.colpart), *rowpart = (double *)((char *)d_work + w.rowpart);
  double *S = (double *)((char *)d_work + w.S);
  hipLaunchKernelGGL(sigma_slice_sum_kernel, dim3(G.np * G.nband * G.nchunk, B), dim3(kCorrThreads), 0, st, G, L.nvert(),
                     (const double2 *)d_state, colpart, rowpart);
  MLMCPI_LAUNCH_CHECK("sigma_slice_sum_kernel");
  hipLaunchKernelGGL(sigma_slice_gather_kernel, dim3((3 * (L.Mt + L.Mx) + kCorrThreads - 1) / kCorrThreads, B), dim3(kCorrThreads), 0,
                     st, G, L.Mt, L.Mx, (const double *)colpart, (const double *)rowpart, S);
  MLMCPI_LAUNCH_CHECK("sigma_slice_gather_kernel");
  const uint32_t Mmax = L.Mt > L.Mx ? L.Mt : L.Mx;
  const dim3 grid((Mmax / 2 + 1 + kCorrTauPerBlock - 1) / kCorrTauPerBlock, 2, B);
  const double inv_n = 1.0 / (double)L.nvert();
  if (Mmax <= kCorrLdsExtent)
    hipLaunchKernelGGL(sigma_correlator_kernel<true>, grid, dim3(kCorrThreads), (size_t)3 * Mmax * sizeof(double), st, L.Mt, L.Mx, inv_n,
                       (const double *)S, d_out, d_acc);
  else
    hipLaunchKernelGGL(sigma_correlator_kernel<false>, grid, dim3(kCorrThreads), 0, st, L.Mt, L.Mx, inv_n, (const double *)S, d_out,
                       d_acc);
  MLMCPI_LAUNCH_CHECK("sigma_correlator_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
