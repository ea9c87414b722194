// lattice_reduce.hip -- the streaming side of the GFF and Schwinger lattices (lattice2d.hip and its kernel units hold the sweeps): per-chain
// reductions over a state (action, phi^2, average plaquette, topological charge), the final sum of per-tile partials,
// start states, the per-chain statistics, and the argument checks every lattice entry point shares.
#include "internal.hpp"

namespace mlmcpi {

__device__ __forceinline__ double plaquette_angle(const double2 *t, uint32_t Mt, uint32_t Mx, uint32_t i, uint32_t j) {
  const uint32_t ip = (i + 1 == Mt) ? 0 : i + 1, jp = (j + 1 == Mx) ? 0 : j + 1;
  // theta(i,j,0) + theta(i+1,j,1) - theta(i,j+1,0) - theta(i,j,1)   (quenchedschwingeraction.cc:14-17)
  const double2 here = t[(size_t)j * Mt + i];
  return here.x + t[(size_t)j * Mt + ip].y - t[(size_t)jp * Mt + i].x - here.y;
}

// grid (nrows_blocks, B): each workgroup strides over lattice rows j
template <int OP>
__global__ void __launch_bounds__(256) lattice_reduce_kernel(uint32_t Mt, uint32_t Mx, double mu2,
                                                             const double *__restrict__ state,
                                                             double *__restrict__ partial) {
  __shared__ double red[4];
  const uint32_t b = blockIdx.y;
  double acc[1] = {0.0};
  if (OP == L_GFF_ENERGY || OP == L_PHI2) {
    const double *phi = state + (size_t)b * Mt * Mx;
    const double kappa = 4. + mu2;
    for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x) {
      const uint32_t jm = j == 0 ? Mx - 1 : j - 1, jp = j + 1 == Mx ? 0 : j + 1;
      for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
        const double v = phi[(size_t)j * Mt + i];
        if (OP == L_PHI2) {
          acc[0] += v * v;
        } else {  // gffaction.cc:15-23
          const uint32_t im = i == 0 ? Mt - 1 : i - 1, ip = i + 1 == Mt ? 0 : i + 1;
          double loc = kappa * v;
          loc -= phi[(size_t)j * Mt + ip];
          loc -= phi[(size_t)j * Mt + im];
          loc -= phi[(size_t)jp * Mt + i];
          loc -= phi[(size_t)jm * Mt + i];
          acc[0] += v * loc;
        }
      }
    }
  } else {
    const double2 *t = (const double2 *)state + (size_t)b * Mt * Mx;
    for (uint32_t j = blockIdx.x; j < Mx; j += gridDim.x)
      for (uint32_t i = threadIdx.x; i < Mt; i += blockDim.x) {
        const double th = plaquette_angle(t, Mt, Mx, i, j);
        if (OP == L_SCHW_ENERGY) acc[0] += 1. - cos_reduced(th);
        if (OP == L_PLAQ) acc[0] += cos_reduced(th);
        if (OP == L_CHARGE) acc[0] += mod_2pi(th);
      }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
}

// Plaquette reductions (Schwinger energy, average plaquette, topological charge), one pass with ONE load per site.
// Grid (bands, B): a workgroup walks a band of consecutive rows bottom-up; a thread owns the columns tid + 256 c and
// keeps the current row of its columns in registers, so theta(i, j+1, 0) of this row is the `here` of the next one;
// theta(i+1, j, 1) comes from the neighbouring lane (the last lane of a wave loads it).  The generic kernel above issues
// three 16-byte loads per plaquette and runs at ~2.9 TB/s; this one is bound by the 16 B per site it has to read.
template <int OP, int NC>
__global__ void __launch_bounds__(256) schwinger_reduce_band_kernel(uint32_t Mt, uint32_t Mx, uint32_t rows_per_band,
                                                                    const double2 *__restrict__ state,
                                                                    double *__restrict__ partial) {
  __shared__ double red[4];
  const uint32_t b = blockIdx.y, j0 = blockIdx.x * rows_per_band;
  const uint32_t j1 = min(j0 + rows_per_band, Mx);
  const double2 *t = state + (size_t)b * Mt * Mx;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  double2 cur[NC], nxt[NC];
  uint32_t col[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    col[c] = threadIdx.x + 256u * c;
    cur[c] = col[c] < Mt ? t[(size_t)j0 * Mt + col[c]] : make_double2(0., 0.);
  }
  double acc[1] = {0.0};
  for (uint32_t j = j0; j < j1; ++j) {
    const uint32_t jp = j + 1 == Mx ? 0 : j + 1;
    double edge[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      nxt[c] = col[c] < Mt ? t[(size_t)jp * Mt + col[c]] : make_double2(0., 0.);
      // the right neighbour of a wave's last lane (or of the last column) lives in another wave / at column 0
      const uint32_t ip = col[c] + 1 == Mt ? 0 : col[c] + 1;
      edge[c] = (col[c] < Mt && (lane == kWave - 1 || col[c] + 1 == Mt)) ? t[(size_t)j * Mt + ip].y : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double from_lane = __shfl_down(cur[c].y, 1, kWave);
      const double right = (lane == kWave - 1 || col[c] + 1 == Mt) ? edge[c] : from_lane;
      if (col[c] < Mt) {
        // theta(i,j,0) + theta(i+1,j,1) - theta(i,j+1,0) - theta(i,j,1)   (quenchedschwingeraction.cc:14-17)
        const double th = cur[c].x + right - nxt[c].x - cur[c].y;
        if (OP == L_SCHW_ENERGY) acc[0] += 1. - cos_reduced(th);
        if (OP == L_PLAQ) acc[0] += cos_reduced(th);
        if (OP == L_CHARGE) acc[0] += mod_2pi(th);
      }
      cur[c] = nxt[c];
    }
  }
  block_sum<1>(acc, red);
  if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
}

__global__ void __launch_bounds__(256) lattice_finish_kernel(const double *__restrict__ partial, uint32_t nsplit, uint32_t B,
                                                              int op, double scale, double *__restrict__ out,
                                                              double *__restrict__ acc = nullptr) {
  // one wave per chain: lane l sums partials l, l + 64, ... in order, then a fixed shuffle tree -- the result depends on
  // nsplit only, never on the launch.  acc != NULL: stats->record_sample of the value as well (stats_accumulate_kernel's
  // recurrence), for callers that would launch that next.
  const uint32_t b = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (b >= B) return;
  double s = 0.0;
  for (uint32_t k = lane; k < nsplit; k += 64) s += partial[(size_t)b * nsplit + k];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    const double v = (op == L_CHARGE) ? (1. / (4. * kPi * kPi)) * s * s : scale * s;  // qoi2dsusceptibility.cc:26
    out[b] = v;
    if (acc) record_moments(acc + 5 * (size_t)b, v);
  }
}

__global__ void __launch_bounds__(256) lattice_init_kernel(int kind, uint32_t n, RngKey key0, double *__restrict__ x) {
  const uint32_t b = blockIdx.y;
  RngKey key = key0;
  key.chain += b;
  double *xb = x + (size_t)b * n;
  for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < n; l += gridDim.x * blockDim.x) {
    if (kind == MLMCPI_SCHWINGER) {
      double u, v;
      rng_uniforms(key, l, P_INIT, 0, u, v);
      xb[l] = -kPi + 2.0 * kPi * u;
    } else {
      xb[l] = rng_normal0(key, l, P_INIT, 0);
    }
  }
}

// Statistics::record_sample with its autocorrelation window (common/statistics.cc:4-27), one chain per thread: per chain
// [n, a1 = running average, S_0 .. S_{W-1} = running averages of Q_j Q_{j-k}, head, ring of the last W values].  The same
// recurrences as the reference: a1 <- ((n - 1) a1 + Q) / n; S_k <- ((N_k - 1) S_k + Q Q_{-k}) / N_k, N_k = n - k, over the k
// the window holds.  tau_int = max(1, 1 + 2 sum_{k >= 1} (1 - k / n) (S_k - a1^2) / (S_0 - a1^2)) is left to the caller
// (:38-61): the multilevel driver reads it between draws (montecarlomultilevel.cc:170-190).
__global__ void stats_window_record_kernel(double *__restrict__ state, const double *__restrict__ q, uint32_t B, uint32_t W) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double *st = state + (size_t)b * (2 * W + 3);
  double *S = st + 2, *ring = st + 3 + W;
  const double Q = q[b];
  const double n = st[0] + 1.0;
  uint32_t head = (uint32_t)st[2 + W];   // slot of the most recent value
  head = head + 1 == W ? 0 : head + 1;
  ring[head] = Q;
  st[2 + W] = (double)head;
  st[0] = n;
  st[1] = ((n - 1.0) * st[1] + Q) / n;
  const uint32_t filled = n < (double)W ? (uint32_t)n : W;
  uint32_t slot = head;
  for (uint32_t k = 0; k < filled; ++k) {
    const double Nk = n - (double)k;
    S[k] = ((Nk - 1.0) * S[k] + Q * ring[slot]) / Nk;
    slot = slot == 0 ? W - 1 : slot - 1;
  }
}

// packed per-chain sums for the cross-rank reduction: [n, sum q, sum q^2, sum q^3, sum q^4]
__global__ void stats_accumulate_kernel(double *__restrict__ acc, const double *__restrict__ q, uint32_t B) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  record_moments(acc + 5 * (size_t)b, q[b]);
}

// ---- host dispatch ----------------------------------------------------------------------------------------
int check_lattice(const mlmcpi_lattice_action *act, bool square_gff) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_GFF && act->kind != MLMCPI_SCHWINGER && act->kind != MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_INVALID, "kind %d is not a 2-D lattice action", act->kind);
  if (act->Mt < 2 || act->Mx < 2) return fail(MLMCPI_ERR_INVALID, "lattice %u x %u too small", act->Mt, act->Mx);
  if ((uint64_t)act->Mt * act->Mx > (1ull << 30)) return fail(MLMCPI_ERR_INVALID, "lattice too large for 32-bit site indices");
  // gffaction.hh:169-173: the GFF action requires a square lattice
  if (square_gff && act->kind == MLMCPI_GFF && act->Mt != act->Mx)
    return fail(MLMCPI_ERR_INVALID, "Lattice has to be squared for GFF action");
  return MLMCPI_OK;
}

// the entry points the O(3) sigma model does not take
int refuse_sigma(const mlmcpi_lattice_action *act, const char *what) {
  if (act && act->kind == MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "%s is not available for the O(3) nonlinear sigma model (DESIGN 8)", what);
  return MLMCPI_OK;
}

uint32_t row_blocks(uint32_t Mx, uint32_t B) {
  uint32_t want = (2048 + B - 1) / B;
  return want < Mx ? (want ? want : 1) : Mx;
}

int lattice_finish(const double *partial, uint32_t tiles, uint32_t B, int op, double scale, double *d_out, double *d_acc, hipStream_t st) {
  hipLaunchKernelGGL(lattice_finish_kernel, dim3((B + 3) / 4), dim3(256), 0, st, partial, tiles, B, op, scale, d_out, d_acc);
  MLMCPI_LAUNCH_CHECK("lattice_finish_kernel");
  return MLMCPI_OK;
}

template <int OP>
static int launch_lattice_reduce(uint32_t Mt, uint32_t Mx, double mu2, const double *d_state, uint32_t B, double scale,
                                 double *d_out, hipStream_t st) {
  uint32_t nsplit = row_blocks(Mx, B);
  constexpr bool plaquettes = OP == L_SCHW_ENERGY || OP == L_PLAQ || OP == L_CHARGE;
  // plaquette reductions on lattices up to 2048 columns: bands of consecutive rows, one load per site
  uint32_t rows_per_band = 0;
  if (plaquettes && Mt <= 2048 && Mt >= 64) {
    rows_per_band = (Mx + nsplit - 1) / nsplit;
    if (rows_per_band < 8) rows_per_band = Mx < 8 ? Mx : 8;  // the first row of a band is loaded twice: keep bands tall
    nsplit = (Mx + rows_per_band - 1) / rows_per_band;
  }
  void *ws = nullptr;
  if (int rc = scratch((size_t)B * nsplit * sizeof(double), &ws, st)) return rc;
  if constexpr (plaquettes) if (rows_per_band) {
    const double2 *t = (const double2 *)d_state;
    const int nc = (int)((Mt + 255) / 256);
#define MLMCPI_BAND(NC) hipLaunchKernelGGL((schwinger_reduce_band_kernel<OP, NC>), dim3(nsplit, B), dim3(256), 0, st, Mt, Mx, rows_per_band, t, (double *)ws)
    switch (nc) {
      case 1: MLMCPI_BAND(1); break;
      case 2: MLMCPI_BAND(2); break;
      case 3: MLMCPI_BAND(3); break;
      case 4: MLMCPI_BAND(4); break;
      case 5: MLMCPI_BAND(5); break;
      case 6: MLMCPI_BAND(6); break;
      case 7: MLMCPI_BAND(7); break;
      default: MLMCPI_BAND(8);
    }
#undef MLMCPI_BAND
    MLMCPI_LAUNCH_CHECK("schwinger_reduce_band_kernel");
  }
  if (!rows_per_band) {
    hipLaunchKernelGGL((lattice_reduce_kernel<OP>), dim3(nsplit, B), dim3(256), 0, st, Mt, Mx, mu2, d_state, (double *)ws);
    MLMCPI_LAUNCH_CHECK("lattice_reduce_kernel");
  }
  return lattice_finish((const double *)ws, nsplit, B, OP, scale, d_out, nullptr, st);
}

int lattice_energy(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S, hipStream_t st) {
  if (act->kind == MLMCPI_GFF)
    return launch_lattice_reduce<L_GFF_ENERGY>(act->Mt, act->Mx, gff_mu2(*act), d_phi, B, 0.5, d_S, st);
  return launch_lattice_reduce<L_SCHW_ENERGY>(act->Mt, act->Mx, 0.0, d_phi, B, act->beta, d_S, st);
}

int lattice_sum_squares(const double *d_x, uint32_t n, uint32_t B, double scale, double *d_out, hipStream_t st) {
  // treat the entries as a 1 x n strip, or as rows of the largest power of two in [64, 4096] that divides n: the
  // reduction does not need the geometry
  uint32_t w = n, h = 1;
  if (n > 4096)
    for (uint32_t c = 4096; c >= 64; c >>= 1)
      if (n % c == 0) { w = c; h = n / c; break; }
  return launch_lattice_reduce<L_PHI2>(w, h, 0.0, d_x, B, scale, d_out, st);
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_lattice_state_size(const mlmcpi_lattice_action *act, uint32_t *n) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(n, "n is NULL");
  *n = (act->kind == MLMCPI_GFF ? 1u : 2u) * act->Mt * act->Mx;
  return MLMCPI_OK;
}

int mlmcpi_lattice_evaluate(const mlmcpi_lattice_action *act, const double *d_phi, uint32_t B, double *d_S,
                            void *stream) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(d_phi && d_S && B > 0, "bad arguments");
  if (act->kind == MLMCPI_NONLINEAR_SIGMA) return sigma_evaluate(act, d_phi, B, d_S, as_stream(stream));
  return lattice_energy(act, d_phi, B, d_S, as_stream(stream));
}

int mlmcpi_lattice_initialise(const mlmcpi_lattice_action *act, double *d_phi, uint32_t B, uint64_t seed,
                              uint32_t chain0, void *stream) {
  if (int rc = check_lattice(act)) return rc;
  MLMCPI_REQUIRE(d_phi && B > 0, "bad arguments");
  if (act->kind == MLMCPI_GFF) return gff_initialise_exact(act, d_phi, B, seed, chain0, as_stream(stream));
  if (act->kind == MLMCPI_NONLINEAR_SIGMA) return sigma_initialise(act, d_phi, B, seed, chain0, as_stream(stream));
  uint32_t n = 0;
  mlmcpi_lattice_state_size(act, &n);
  hipLaunchKernelGGL(lattice_init_kernel, dim3(stream_blocks(n), B), dim3(256), 0, as_stream(stream), act->kind, n,
                     make_key(seed, chain0, 0), d_phi);
  MLMCPI_LAUNCH_CHECK("lattice_init_kernel");
  return MLMCPI_OK;
}

int mlmcpi_qoi_phi_squared(const double *d_phi, uint32_t n_vertices, uint32_t B, double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_phi && d_out && B > 0 && n_vertices > 0, "bad arguments");
  return lattice_sum_squares(d_phi, n_vertices, B, 1.0 / n_vertices, d_out, as_stream(stream));
}

int mlmcpi_qoi_avg_plaquette(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out,
                             void *stream) {
  MLMCPI_REQUIRE(d_theta && d_out && B > 0 && Mt > 1 && Mx > 1, "bad arguments");
  return launch_lattice_reduce<L_PLAQ>(Mt, Mx, 0.0, d_theta, B, 1.0 / ((double)Mx * Mt), d_out, as_stream(stream));
}

int mlmcpi_qoi_2d_susceptibility(const double *d_theta, uint32_t Mt, uint32_t Mx, uint32_t B, double *d_out,
                                 void *stream) {
  MLMCPI_REQUIRE(d_theta && d_out && B > 0 && Mt > 1 && Mx > 1, "bad arguments");
  return launch_lattice_reduce<L_CHARGE>(Mt, Mx, 0.0, d_theta, B, 1.0, d_out, as_stream(stream));
}

int mlmcpi_stats_window_record(double *d_state, const double *d_q, uint32_t B, uint32_t window, void *stream) {
  MLMCPI_REQUIRE(d_state && d_q && B > 0 && window > 0 && window <= 1024, "bad arguments");
  hipLaunchKernelGGL(stats_window_record_kernel, dim3((B + 255) / 256), dim3(256), 0, as_stream(stream), d_state, d_q, B, window);
  MLMCPI_LAUNCH_CHECK("stats_window_record_kernel");
  return MLMCPI_OK;
}

int mlmcpi_stats_accumulate(double *d_acc, const double *d_q, uint32_t B, void *stream) {
  MLMCPI_REQUIRE(d_acc && d_q && B > 0, "bad arguments");
  hipLaunchKernelGGL(stats_accumulate_kernel, dim3((B + 255) / 256), dim3(256), 0, as_stream(stream), d_acc, d_q, B);
  MLMCPI_LAUNCH_CHECK("stats_accumulate_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
