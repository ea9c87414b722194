// schwinger_sweeps.hip -- the sweep kernels of the quenched Schwinger model (U(1) link angles, plaquette action; one double2
// {theta_0, theta_1} per site) and their launcher: the generic overlapped-tile kernel, the 4 x 4 register blocks, the closed
// form of K overrelaxation sweeps and the launch that runs the heat bath behind it.  lattice2d.hip plans a draw and calls
// schwinger_sweep_launch once per launch; the sizes it plans with are in lattice_sweep.hpp.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include "lattice_sweep.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// Instrumentation build only (make EXTRA=-DMLMCPI_STAMPS): thread 0 of every workgroup of
// schwinger_perm_heat_kernel leaves the 100 MHz wall clock at ten points, plus the XCD / CU it ran on.
#ifdef MLMCPI_STAMPS
__device__ unsigned long long g_stamps[16 * 65536];
#define MLMCPI_STAMP(k)                                                                                            \
  do {                                                                                                             \
    if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 65536)                                           \
      g_stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (k)] = __builtin_amdgcn_s_memrealtime();               \
  } while (0)
#define MLMCPI_STAMP_WHERE()                                                                                       \
  do {                                                                                                             \
    if (threadIdx.x == 0 && blockIdx.y * gridDim.x + blockIdx.x < 65536)                                           \
      g_stamps[(blockIdx.y * gridDim.x + blockIdx.x) * 16 + 15] =                                                  \
          ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (31 << 11)) << 32) |         \
          __builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));                                        \
  } while (0)
// the stamps of the last launch of schwinger_perm_heat_kernel, 16 words per workgroup
extern "C" int mlmcpi_debug_read_stamps(unsigned long long *h_out, uint32_t n_workgroups) {
  MLMCPI_HIP_TRY(hipDeviceSynchronize());
  MLMCPI_HIP_TRY(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_stamps), (size_t)n_workgroups * 16 * sizeof(unsigned long long)));
  return MLMCPI_OK;
}
#else
#define MLMCPI_STAMP(k) do { } while (0)
#define MLMCPI_STAMP_WHERE() do { } while (0)
#endif

// region given as nr x nc with a runtime nc (generic kernels)
template <int NT, int S, bool DIRECT = false, class Setup, class Commit>
__device__ __forceinline__ void heatbath_region(uint32_t nr, uint32_t nc, const RngKey &key, HbPool &pool, Setup setup,
                                                Commit commit) {
  if (DIRECT) {  // nc is a compile-time constant at the call site: the division is a multiply and a shift
    heatbath_cells<NT, S>(nr * nc, key, pool,
                          [&](uint32_t idx, double &tau, double &centre, uint32_t &site, uint32_t &o) {
                            const uint32_t ri = idx / nc;
                            setup(ri, idx - ri * nc, tau, centre, site, o);
                          },
                          commit);
    return;
  }
  // (row, column) of a thread's cells without a division per cell: one division for the first cell, then steps of NT
  // (heatbath_cells asks for a thread's cells in increasing order: idx = tid, tid + NT, tid + 2 NT, ...)
  uint32_t cur = threadIdx.x, ri = cur / nc, ci = cur - ri * nc;
  const uint32_t dr = NT / nc, dc = NT - dr * nc;
  heatbath_cells<NT, S>(nr * nc, key, pool,
                        [&](uint32_t idx, double &tau, double &centre, uint32_t &site, uint32_t &o) {
                          while (cur < idx) {
                            cur += NT;
                            ri += dr;
                            ci += dc;
                            if (ci >= nc) {
                              ci -= nc;
                              ++ri;
                            }
                          }
                          setup(ri, ci, tau, centre, site, o);
                        },
                        commit);
}

// the same for the step-envelope sampler (step_envelope.hpp): cells are addressed by their LDS offset
// r0 * bw + c0 + (row step) * bw * ri + (column step) * ci
template <int NT, int S, bool DIRECT, class E, class Setup, class KappaExact, class Commit>
__device__ __forceinline__ void heatbath_region_step(uint32_t nr, uint32_t nc, uint32_t origin, uint32_t row_stride,
                                                     uint32_t col_stride, const RngKey &key, VsPool<E> &pool, Setup setup,
                                                     KappaExact kappa_exact, Commit commit) {
  if (DIRECT) {  // nc is a compile-time constant at the call site
    heatbath_cells_step<NT, S, E>(nr * nc, key, pool,
                                  [&](uint32_t idx) {
                                    const uint32_t ri = idx / nc;
                                    return origin + ri * row_stride + (idx - ri * nc) * col_stride;
                                  },
                                  setup, kappa_exact, commit);
    return;
  }
  // runtime nc: cells are handed out by a queue (heatbath_cells_step), in no particular order per thread, so (row, column)
  // come from a division -- by a reciprocal computed once, exact for the indices that occur (idx < 2^16 <= 2^24 / nc)
  const float rcp = 1.0f / (float)nc;
  heatbath_cells_step<NT, S, E>(nr * nc, key, pool,
                                [&](uint32_t idx) {
                                  uint32_t ri = (uint32_t)(((float)idx + 0.5f) * rcp);
                                  int32_t ci = (int32_t)(idx - ri * nc);
                                  if (ci < 0) { --ri; ci += (int32_t)nc; }
                                  else if (ci >= (int32_t)nc) { ++ri; ci -= (int32_t)nc; }
                                  return origin + ri * row_stride + (uint32_t)ci * col_stride;
                                },
                                setup, kappa_exact, commit);
}

// ---- Schwinger sweeps ----------------------------------------------------------------------------
// Colour order per sweep: (mu=0, j even), (mu=0, j odd), (mu=1, i even), (mu=1, i odd); links of one
// colour do not appear in each other's staples (quenchedschwingeraction.cc:25-43).  Every link whose
// six staple links lie inside the buffer is updated; the region of exact values shrinks by at most
// two sites per side per sweep, so a halo of 2*nsweeps keeps the owned tile exact (tile origins are
// even, which makes buffer parity equal lattice parity).
// TWC x THC > 0: single-sweep launch on a lattice that the TWC x THC tiles divide and that is wider than a buffer
// (Mt >= TWC + 4, Mx >= THC + 4): tile and buffer extents are compile-time constants (index arithmetic folds, cell
// coordinates come from divisions by constants) and a buffer coordinate wraps around the lattice at most once.  Same
// updates in the same order as the generic instantiation (TWC = THC = 0): bit-identical results.
// STEP: the heat-bath phases draw from the step envelope (2 beta <= kVsKappaMax; step_envelope.hpp) instead of the
// wrapped-Cauchy one; pool_cap then counts entries of VsPool.
template <bool HEAT, int NT, int TWC = 0, int THC = 0, bool STEP = false>
__global__ void __launch_bounds__(NT, HEAT ? (NT == 256 ? 4 : NT == 512 ? 2 : 1) : 1)
    schwinger_sweep_kernel(uint32_t Mt, uint32_t Mx, double beta, const double2 *__restrict__ in,
                           double2 *__restrict__ out, TileGeom tg, uint32_t nsweeps_arg, uint32_t kinds, RngKey key0,
                           uint32_t pool_cap, int qoi_op, double *__restrict__ qoi_partial, const uint32_t *__restrict__ vs_table) {
  extern __shared__ double lds[];
  __shared__ double qoi_red[NT / kWave];
  constexpr bool FIXED = TWC > 0;
  const uint32_t nsweeps = FIXED ? 1u : nsweeps_arg;
  const uint32_t H = 2 * nsweeps;
  const uint32_t tile = blockIdx.x, b = blockIdx.y;
  const uint32_t ty = tile / tg.tiles_x, tx = tile - ty * tg.tiles_x;
  const uint32_t i0 = tx * (FIXED ? TWC : tg.TW), j0 = ty * (FIXED ? THC : tg.TH);
  const uint32_t ow = FIXED ? TWC : min(tg.TW, Mt - i0), oh = FIXED ? THC : min(tg.TH, Mx - j0);
  const uint32_t bw = ow + 2 * H, bh = oh + 2 * H;
  // lattice coordinate of a buffer coordinate
  auto wrap = [&](uint32_t base, uint32_t off, uint32_t n) {
    if (FIXED) {
      const uint32_t v = base + off;
      return v >= n ? v - n : v;
    }
    return wrap_add(base, off, n);
  };
  // The sampler's tables and the list / pool of open cells of the heat-bath phases at the START of the LDS (table look-ups
  // are then instruction offsets; r04), the tile image behind them (launch_sweep_nt sizes the allocation the same way)
  using PoolEntry = typename std::conditional<FIXED, uint16_t, uint32_t>::type;   // 68 x 36 cells: 12 bits of offset
  double *pool_lds = lds;
  HbPool pool = HbPool::carve(pool_lds, HEAT && !STEP ? pool_cap : 0u);
  VsPool<PoolEntry> vpool = VsPool<PoolEntry>::carve(pool_lds, HEAT && STEP ? pool_cap : 0u, STEP ? vs_table : nullptr);
  double *th0 = lds + (HEAT ? sweep_pool_bytes(STEP, FIXED, pool_cap) / sizeof(double) : 0), *th1 = th0 + (size_t)bw * bh;
  const double beta2 = 2. * beta;
  const uint32_t sc = (uint32_t)(((uint64_t)i0 + Mt - (H % Mt)) % Mt);  // lattice column of buffer column 0
  const uint32_t sr = (uint32_t)(((uint64_t)j0 + Mx - (H % Mx)) % Mx);
  const double2 *src = in + (size_t)b * Mt * Mx;
  RngKey key = key0;
  key.chain += b;

  stage_region<NT, (NT >= 1024 ? 3 : 5), double2>(
      bh, bw, [&](uint32_t r, uint32_t c) { return src[(size_t)wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)]; },
      [&](uint32_t r, uint32_t c, double2 v) {
        th0[r * bw + c] = v.x;
        th1[r * bw + c] = v.y;
      });
  __syncthreads();

  for (uint32_t s = 0; s < nsweeps; ++s) {
    const bool heat = HEAT && (FIXED || ((kinds >> s) & 1u));
    RngKey skey = key;
    skey.step += s;
    // Update regions.  In general every link whose staple links lie inside the buffer is updated:
    //   mu = 0: rows [1, bh-2] of one parity, columns [0, bw-2];   mu = 1: columns [1, bw-2] of one parity, rows [0, bh-2].
    // The LAST sweep of a launch only has to be right on the owned tile (rows [H, H+oh), columns [H, H+ow)), so each
    // of its phases is cut down to what later phases still read:
    //   phase 3 (mu = 1, odd columns)   owned links;
    //   phase 2 (mu = 1, even columns)  + the column right of the tile (phase 3 reads theta_1(i+1, j));
    //   phases 0, 1 (mu = 0)            rows [H, H+oh], columns [H-1, H+ow] (phases 2, 3 read theta_0 at (i-1 .. i, j .. j+1)).
    // For a heat-bath launch (always a single sweep) that is 7 % fewer draws.
    const bool last = s + 1 == nsweeps;
    const uint32_t r_hi0 = last ? H + oh : bh - 2;                              // mu = 0 rows: upper end (inclusive)
    const uint32_t c_lo0 = last ? H - 1 : 0, c_hi0 = last ? H + ow : bw - 2;    // mu = 0 columns
    const uint32_t r_lo1 = last ? H : 0, r_hi1 = last ? H + oh - 1 : bh - 2;    // mu = 1 rows
    for (uint32_t par = 0; par < 2; ++par) {
      // even rows first; H is even, so H + par has the parity of this phase
      const uint32_t r_first = last ? H + par : (par ? 1 : 2);
      const uint32_t nr = r_first <= r_hi0 ? (r_hi0 - r_first) / 2 + 1 : 0;
      const uint32_t ncol = c_hi0 - c_lo0 + 1;
      if (heat && STEP) {
        heatbath_region_step<NT, 5, FIXED, PoolEntry>(
            nr, ncol, r_first * bw + c_lo0, 2 * bw, 1, skey, vpool,
            [&](uint32_t o, VsCell &cell) {
              const uint32_t r = o / bw, c = o - r * bw;
              vs_cell(beta2, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw], cell);
              cell.site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt));
            },
            [&](uint32_t o) {
              return vs_kappa_exact(beta2, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw]);
            },
            [&](uint32_t o, double v) { th0[o] = v; });
      } else if (heat) {
        heatbath_region<NT, 5, FIXED>(
            nr, ncol, skey, pool,
            [&](uint32_t ri, uint32_t ci, double &tau, double &centre, uint32_t &site, uint32_t &o) {
              const uint32_t r = r_first + 2 * ri, c = c_lo0 + ci;
              o = r * bw + c;
              const double tp = th0[o + bw] + th1[o] - th1[o + 1];  // staple angles, unwrapped (expcos_params)
              const double tm = th0[o - bw] + th1[o - bw + 1] - th1[o - bw];
              expcos_params(beta, tp, tm, tau, centre);
              site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt));
            },
            [&](uint32_t o, double v) { th0[o] = v; });
      } else
      for_region<NT>(nr, ncol, [&](uint32_t ri, uint32_t ci) {
        const uint32_t r = r_first + 2 * ri, o = r * bw + c_lo0 + ci;
        // overrelaxation: mod_2pi(theta+ + theta- - theta); the two staple angles need no wrap of their own here
        // (2 pi-periodicity of the final map), which drops two of the three mod_2pi per update
        const double tp = th0[o + bw] + th1[o] - th1[o + 1];
        const double tm = th0[o - bw] + th1[o - bw + 1] - th1[o - bw];
        th0[o] = mod_2pi_fast((tp + tm) - th0[o]);
      });
      __syncthreads();
    }
    for (uint32_t par = 0; par < 2; ++par) {
      const uint32_t c_first = last ? H + par : (par ? 1 : 2);
      // last sweep: even columns up to H + ow (one past the tile), odd columns up to H + ow - 1
      const uint32_t c_hi1 = last ? (par ? H + ow - 1 : H + ow) : bw - 2;
      const uint32_t nc = c_first <= c_hi1 ? (c_hi1 - c_first) / 2 + 1 : 0;
      const uint32_t nrow = r_hi1 - r_lo1 + 1;
      if (heat && STEP) {
        heatbath_region_step<NT, 5, FIXED, PoolEntry>(
            nrow, nc, r_lo1 * bw + c_first, bw, 2, skey, vpool,
            [&](uint32_t o, VsCell &cell) {
              const uint32_t r = o / bw, c = o - r * bw;
              vs_cell(beta2, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1], cell);
              cell.site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)) + 1;
            },
            [&](uint32_t o) {
              return vs_kappa_exact(beta2, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1]);
            },
            [&](uint32_t o, double v) { th1[o] = v; });
      } else if (heat) {
        heatbath_region<NT, 5, FIXED>(
            nrow, nc, skey, pool,
            [&](uint32_t ri, uint32_t ci, double &tau, double &centre, uint32_t &site, uint32_t &o) {
              const uint32_t r = r_lo1 + ri, c = c_first + 2 * ci;
              o = r * bw + c;
              const double tp = th0[o] + th1[o + 1] - th0[o + bw];
              const double tm = th0[o + bw - 1] + th1[o - 1] - th0[o - 1];
              expcos_params(beta, tp, tm, tau, centre);
              site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)) + 1;
            },
            [&](uint32_t o, double v) { th1[o] = v; });
      } else
      for_region<NT>(nrow, nc, [&](uint32_t ri, uint32_t ci) {
        const uint32_t r = r_lo1 + ri, c = c_first + 2 * ci, o = r * bw + c;
        const double tp = th0[o] + th1[o + 1] - th0[o + bw];
        const double tm = th0[o + bw - 1] + th1[o - 1] - th0[o - 1];
        th1[o] = mod_2pi_fast((tp + tm) - th1[o]);
      });
      __syncthreads();
    }
  }

  // Optional fused QoI of the final state (qoi/qft/qoiavgplaquette.cc:8-27, qoi2dsusceptibility.cc:8-27): the plaquette
  // (i, j) needs theta(i+1, j, 1) and theta(i, j+1, 0); for the owned tile those are the column right of it and the row
  // above it, which the last sweep's pruned regions bring to their final values (that is what they are for).  One
  // partial per tile; lattice_finish_kernel sums them in tile order.
  double acc[1] = {0.0};
  double2 *dst = out + (size_t)b * Mt * Mx;
  for_region<NT>(oh, ow, [&](uint32_t r, uint32_t c) {
    const uint32_t o = (r + H) * bw + (c + H);
    dst[(size_t)(j0 + r) * Mt + (i0 + c)] = make_double2(th0[o], th1[o]);
    if (qoi_op) {
      const double thp = th0[o] + th1[o + 1] - th0[o + bw] - th1[o];   // quenchedschwingeraction.cc:14-17
      acc[0] += qoi_op == 3 ? cos_reduced(thp) : mod_2pi(thp);         // 3 = L_PLAQ, 4 = L_CHARGE
    }
  });
  if (qoi_op) {
    block_sum<1>(acc, qoi_red);
    if (threadIdx.x == 0) qoi_partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
  }
}

// ---- Schwinger overrelaxation, 4 x 4 register blocks on 64 x 64 tiles (OrBlockGeom, lattice_sweep.hpp) -----------------------
// Measured on MI355X (1024 x 1024, 32 chains; timestamps taken inside the kernel): a sweep costs
// 0.028 ms of the launch, which is the fp64 issue time of its 9 instructions per update, and the rest of the launch
// (0.21 ms at K = 1, against 0.17 ms for a plain copy of the state) is the load and store phase of the workgroups,
// which the two workgroups a CU holds overlap only partly with each other's sweeps.  Persistent workgroups and an
// XCD-aware tile order changed nothing; writing the tile back in whole 1 KiB rows per wave instruction instead of
// 16 B per lane at a 64 B stride took 0.02-0.035 ms off every launch (see the end of the kernel); doing the same for
// the loads did not pay.  The K >= 4 launches run at the package power limit (1.37 kW, sclk 2.17-2.25 GHz).
// The buffer of geometry G (tile + halo G::H) into 4 x 4 register blocks, then KS <= G::H / 2 overrelaxation sweeps on it.
// Ends behind the barrier of the last colour phase: the plane area of the LDS is dead from there on.
template <class G, int KS>
__device__ __forceinline__ void or_block_sweeps(double *lds, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx,
                                                uint32_t i0, uint32_t j0, double (&t0)[G::PH][G::PW], double (&t1)[G::PH][G::PW]) {
  constexpr int PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NPY = G::NPY, NP = G::NP;
  static_assert(2 * KS <= H, "a sweep costs two sites of halo");
  auto pl = [&](int p) { return lds + p * NP; };
  const uint32_t tid = threadIdx.x;
  if (tid >= (uint32_t)G::NT) {  // waves beyond the blocks (a caller with a wider workgroup): only the barriers
    for (int i = 0; i < 1 + 4 * KS; ++i) __syncthreads();
    return;
  }
  const bool active = tid < NP;
  const int pj = active ? (int)tid / NPX : 0, pi = active ? (int)tid - pj * NPX : 0;
  const int me = active ? (int)tid : 0;  // idle threads of the last wave: every index is entry 0, nothing is written
  // neighbour blocks, clamped into the buffer
  const int dn = pj > 0 ? me - NPX : me, up = pj + 1 < NPY ? me + NPX : me;
  const int lf = pi > 0 ? me - 1 : me, rt = pi + 1 < NPX ? me + 1 : me;
  const int rtdn = (pi + 1 < NPX ? 1 : 0) + (pj > 0 ? -NPX : 0) + me;
  const int lfup = (pi > 0 ? -1 : 0) + (pj + 1 < NPY ? NPX : 0) + me;
  // t0, t1: [c][a] = links of vertex (PW pi + a, PH pj + c)

  // the block's columns in the lattice: H is even, so (gi, gi + 1) never straddles the wrap, (gi + 1, gi + 2) may
  {
    uint32_t gi[PW / 2], gj[PH];
    gi[0] = (uint32_t)(((uint64_t)i0 + Mt - (H % Mt) + PW * pi) % Mt);
    gj[0] = (uint32_t)(((uint64_t)j0 + Mx - (H % Mx) + PH * pj) % Mx);
#pragma unroll
    for (int a = 1; a < PW / 2; ++a) gi[a] = gi[a - 1] + 2 == Mt ? 0 : gi[a - 1] + 2;
#pragma unroll
    for (int c = 1; c < PH; ++c) gj[c] = gj[c - 1] + 1 == Mx ? 0 : gj[c - 1] + 1;
#pragma unroll
    for (int c = 0; c < PH; ++c)
#pragma unroll
      for (int a = 0; a < PW; a += 2) {
        double2 v0 = make_double2(0, 0), v1 = v0;
        if (active) {
          v0 = src[(size_t)gj[c] * Mt + gi[a / 2]];
          v1 = src[(size_t)gj[c] * Mt + gi[a / 2] + 1];
        }
        t0[c][a] = v0.x; t1[c][a] = v0.y; t0[c][a + 1] = v1.x; t1[c][a + 1] = v1.y;
      }
  }
  MLMCPI_STAMP(1);  // (the loads are issued; the first publish waits for their values)
  // what a neighbour reads of link mu at (a, c): up to three lists, a corner value once
  auto publish = [&](int mu, int a, int c, double v) {
    const int p1 = c == PH - 1 ? (mu ? G::top1(a) : G::top0(a)) : -1;
    const int p2 = mu == 0 ? (c == 0 ? G::bot0(a) : -1) : (a == 0 ? G::left1(c) : -1);
    const int p3 = a == PW - 1 ? (mu ? G::right1(c) : G::right0(c)) : -1;
    if (!active) return;
    if (p1 >= 0) pl(p1)[me] = v;
    if (p2 >= 0 && p2 != p1) pl(p2)[me] = v;
    if (p3 >= 0 && p3 != p1 && p3 != p2) pl(p3)[me] = v;
  };
#pragma unroll
  for (int c = 0; c < PH; ++c)
#pragma unroll
    for (int a = 0; a < PW; ++a) {
      publish(0, a, c, t0[c][a]);
      publish(1, a, c, t1[c][a]);
    }
  __syncthreads();
  MLMCPI_STAMP(2);  // buffer in registers, rims published

  for (int s = 0; s < KS; ++s) {
    // row -1: t0(a, -1), t1(a, -1) for a = 0 .. PW (the last from the block below to the right);
    // column PW: t1(PW, c) for c = -1 .. PH - 1 at index c + 1.  None of these changes during phases 0 and 1.
    double dn0[PW], dn1[PW + 1], rt1[PH + 1];
#pragma unroll
    for (int a = 0; a < PW; ++a) {
      dn0[a] = pl(G::top0(a))[dn];
      dn1[a] = pl(G::top1(a))[dn];
    }
    dn1[PW] = pl(G::top1(0))[rtdn];
    rt1[0] = dn1[PW];
#pragma unroll
    for (int c = 0; c < PH; ++c) rt1[c + 1] = pl(G::left1(c))[rt];
    // phases 0, 1: mu = 0, even rows then odd rows
    //   tp = t0(i, j+1) + t1(i, j) - t1(i+1, j),  tm = t0(i, j-1) + t1(i+1, j-1) - t1(i, j-1)
    double up0[PW + 1];  // row PH: t0(a, PH) for a = -1 .. PW - 1 at index a + 1 (final after phase 0)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      if (par == 1) {
#pragma unroll
        for (int a = 0; a < PW; ++a) up0[a + 1] = pl(G::bot0(a))[up];
        up0[0] = pl(G::bot0(PW - 1))[lfup];
      }
#pragma unroll
      for (int c = par; c < PH; c += 2)
#pragma unroll
        for (int a = 0; a < PW; ++a) {
          const double t0_up = c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a] : up0[a + 1];
          const double t0_dn = c > 0 ? t0[c > 0 ? c - 1 : 0][a] : dn0[a];
          const double t1_c = t1[c][a];
          const double t1_r = a + 1 < PW ? t1[c][a + 1 < PW ? a + 1 : 0] : rt1[c + 1];
          const double t1_dr = c > 0 ? (a + 1 < PW ? t1[c > 0 ? c - 1 : 0][a + 1 < PW ? a + 1 : 0] : rt1[c]) : dn1[a + 1];
          const double t1_dc = c > 0 ? t1[c > 0 ? c - 1 : 0][a] : dn1[a];
          const double tp = t0_up + t1_c - t1_r;
          const double tm = t0_dn + t1_dr - t1_dc;
          t0[c][a] = mod_2pi_fast((tp + tm) - t0[c][a]);
          publish(0, a, c, t0[c][a]);
        }
      __syncthreads();
    }
    // column -1: t0(-1, c) for c = 0 .. PH (the last is up0[0]), t1(-1, c); final after phase 1
    double lf0[PH + 1], lf1[PH];
#pragma unroll
    for (int c = 0; c < PH; ++c) {
      lf0[c] = pl(G::right0(c))[lf];
      lf1[c] = pl(G::right1(c))[lf];
    }
    lf0[PH] = up0[0];
    // phases 2, 3: mu = 1, even columns then odd columns
    //   tp = t0(i, j) + t1(i+1, j) - t0(i, j+1),  tm = t0(i-1, j+1) + t1(i-1, j) - t0(i-1, j)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      if (par == 1) {  // the right neighbour's column 0 changed in phase 2
#pragma unroll
        for (int c = 0; c < PH; ++c) rt1[c + 1] = pl(G::left1(c))[rt];
      }
#pragma unroll
      for (int a = par; a < PW; a += 2)
#pragma unroll
        for (int c = 0; c < PH; ++c) {
          const double t0_c = t0[c][a];
          const double t1_r = a + 1 < PW ? t1[c][a + 1 < PW ? a + 1 : 0] : rt1[c + 1];
          const double t0_u = c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a] : up0[a + 1];
          const double t0_lu = a > 0 ? (c + 1 < PH ? t0[c + 1 < PH ? c + 1 : 0][a > 0 ? a - 1 : 0] : up0[a]) : lf0[c + 1];
          const double t1_l = a > 0 ? t1[c][a > 0 ? a - 1 : 0] : lf1[c];
          const double t0_l = a > 0 ? t0[c][a > 0 ? a - 1 : 0] : lf0[c];
          const double tp = t0_c + t1_r - t0_u;
          const double tm = t0_lu + t1_l - t0_l;
          t1[c][a] = mod_2pi_fast((tp + tm) - t1[c][a]);
          publish(1, a, c, t1[c][a]);
        }
      __syncthreads();
    }
  }
}

template <int K>
__global__ void __launch_bounds__(OrBlockGeom<K>::NT)
    schwinger_or_block_kernel(uint32_t Mt, uint32_t Mx, const double2 *__restrict__ in, double2 *__restrict__ out,
                              uint32_t tiles_x) {
  using G = OrBlockGeom<K>;
  constexpr int TW = G::TW, TH = G::TH, PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NP = G::NP;
  extern __shared__ double lds[];
  const uint32_t tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * TW, j0 = ty * TH;
  double t0[PH][PW], t1[PH][PW];
  or_block_sweeps<G, K>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, t0, t1);

  // Owned vertices: buffer columns [H, H + TW), rows [H, H + TH).  A thread holds PW consecutive vertices of a row
  // (64 B), so storing block-wise would make every wave instruction write 64 x 16 B at a 64 B stride.  Instead each wave
  // transposes through LDS (the plane area is dead after the last barrier; wave-private staging, no workgroup barrier):
  // per block row c the owners put their four vertices down, and the wave writes the 256 vertices back as 4 coalesced
  // instructions -- lane l takes vertex l & 3 of block 16 i + (l >> 2), i = 0 .. 3.
  static_assert(PW == 4, "the coalesced side moves 4 vertices per block row");
  const uint32_t wave0 = tid & ~63u, lane = tid & 63u;
  double2 *stage = reinterpret_cast<double2 *>(lds) + (wave0 / 64) * (64 * PW);
  double2 *dst = out + (size_t)b * Mt * Mx;
  int uq[4], ur[4];  // tile coordinates of the vertex this lane writes for i = 0 .. 3 (row c = 0); uq < 0: none
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int bt = (int)wave0 + 16 * i + (int)(lane >> 2);
    const int bj = bt / NPX, bi = bt - bj * NPX;
    uq[i] = PW * bi + (int)(lane & 3) - H;
    ur[i] = PH * bj - H;
    if (bt >= NP || uq[i] >= TW) uq[i] = -1;
  }
#pragma unroll
  for (int c = 0; c < PH; ++c) {
#pragma unroll
    for (int a = 0; a < PW; ++a) stage[PW * lane + a] = make_double2(t0[c][a], t1[c][a]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double2 w = stage[64 * i + lane];
      const int r = ur[i] + c;
      // (non-temporal, r05: one sweep 0.231 -> 0.226 ms over three same-box pairs)
      if (uq[i] >= 0 && r >= 0 && r < TH) store_streaming(&dst[(size_t)(j0 + r) * Mt + (i0 + uq[i])], w.x, w.y);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// The tail of schwinger_perm_heat_kernel: the heat-bath sweep on the LDS image of a
// 64 x 64 tile and its two rings (theta_0 plane th0, theta_1 plane th1, IW = IH = 68), the optional QoI, the write-out.
template <int NT, bool STEP>
__device__ __forceinline__ void schwinger_image_heat(double *th0, double *th1, VsPool<uint32_t> &vpool, HbPool &hpool, uint32_t Mt,
                                                     uint32_t Mx, double beta, double2 *__restrict__ out, uint32_t i0, uint32_t j0,
                                                     uint32_t b, uint32_t tile, RngKey key0, int qoi_op,
                                                     double *__restrict__ qoi_partial, double *qoi_red) {
  constexpr int TW = 64, TH = 64, HB = 2, IW = TW + 2 * HB;
  // the heat-bath sweep: the last-sweep regions of schwinger_sweep_kernel with H = HB, bw = IW, oh = TH, ow = TW
  constexpr uint32_t bw = IW;
  const uint32_t sc = i0 >= (uint32_t)HB ? i0 - HB : i0 + Mt - HB;  // lattice column of image column 0
  const uint32_t sr = j0 >= (uint32_t)HB ? j0 - HB : j0 + Mx - HB;
  auto wrap = [](uint32_t base, uint32_t off, uint32_t n) {
    const uint32_t v = base + off;
    return v >= n ? v - n : v;
  };
  RngKey skey = key0;
  skey.chain += b;
  const double beta2 = 2. * beta;
  // Step-envelope phases with whole waves per round (NT = 512, 1024): the cells of pass 0 by a closed-form map
  // (heatbath_cells_step_mapped); other workgroup sizes and the wrapped-Cauchy sampler hand them out by linear index.
  constexpr bool kMapped = STEP && 32 % (NT / kWave) == 0;
  constexpr uint32_t NW = NT / kWave, NIT = kMapped ? 32 / NW : 1;
  // the stencil reads of the mapped phases go out as single ds_read_b64 at immediate offsets from one address (the compiler
  // pairs neighbouring doubles into ds_read2_b64: 8 LDS cycles against 2 + 2, MI355X_MICROARCH.md); th1 lies IW IH doubles
  // behind th0 at every call site
  constexpr int kT1 = IW * (TH + 2 * HB) * 8;
  const uint32_t lds_th0 = (uint32_t)(uintptr_t)th0;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  for (uint32_t par = 0; par < 2; ++par) {  // mu = 0: rows [HB, HB + TH] of one parity, columns [HB - 1, HB + TW]
    const uint32_t r_first = HB + par, nr = (HB + TH - r_first) / 2 + 1;
    constexpr uint32_t ncol = TW + 2;
    if (!STEP)
      heatbath_region<NT, 5, true>(
          nr, ncol, skey, hpool,
          [&](uint32_t ri, uint32_t ci, double &tau, double &centre, uint32_t &site, uint32_t &o) {
            const uint32_t r = r_first + 2 * ri, c = HB - 1 + ci;
            o = r * bw + c;
            expcos_params(beta, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw], tau, centre);
            site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt));
          },
          [&](uint32_t o, double v) { th0[o] = v; });
    else if constexpr (kMapped) {
      // pass 0: wave w takes rows ri = w + NW k (k < NIT: 32 of the 33 rows), lane l column ci = l (64 of the 66); the
      // row of the Philox site is a scalar, its column one register for the whole phase
      uint32_t o_next = (r_first + 2 * wave) * bw + (HB - 1) + lane;
      uint32_t srow = wrap(sr, r_first + 2 * wave, Mx);                  // (scalar)
      const uint32_t scol = wrap(sc, HB - 1 + lane, Mt), n_top = (nr - NIT * NW) * ncol;
      heatbath_cells_step_mapped<NT, NIT, uint32_t>(
          n_top + 2 * (NIT * NW), skey, vpool,
          [&](uint32_t &o, uint32_t &site) {
            o = o_next;
            site = (srow * Mt + scol) << 1;
            o_next += 2 * NW * bw;
            srow = wrap(srow, 2 * NW, Mx);
          },
          [&](uint32_t i) {   // left over: row ri = 32 of the even phase (66 cells), then columns 64, 65 of the rows before it
            const uint32_t j = i - n_top, ri = i < n_top ? (uint32_t)(NIT * NW) : j >> 1, ci = i < n_top ? i : 64 + (j & 1u);
            return (r_first + 2 * ri) * bw + (HB - 1) + ci;
          },
          [&](uint32_t o) {
            const uint32_t r = o / bw, c = o - r * bw;
            return 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt));
          },
          [&](uint32_t o, double (&v)[6]) {   // from the address of th0[o - bw]: offsets are unsigned
            const uint32_t a = lds_th0 + (o - bw) * 8u;
            v[0] = lds_read_f64<2 * bw * 8>(a);                 // th0[o + bw]
            v[1] = lds_read_f64<kT1 + bw * 8>(a);               // th1[o]
            v[2] = lds_read_f64<kT1 + bw * 8 + 8>(a);           // th1[o + 1]
            v[3] = lds_read_f64<0>(a);                          // th0[o - bw]
            v[4] = lds_read_f64<kT1 + 8>(a);                    // th1[o - bw + 1]
            v[5] = lds_read_f64<kT1>(a);                        // th1[o - bw]
          },
          [&](const double (&v)[6], VsCell &cell) { vs_cell(beta2, v[0] + v[1] - v[2], v[3] + v[4] - v[5], cell); },
          [&](uint32_t o) {
            return vs_kappa_exact(beta2, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw]);
          },
          [&](uint32_t o, double v) { th0[o] = v; });
    } else
    heatbath_region_step<NT, 5, true, uint32_t>(
        nr, ncol, r_first * bw + (HB - 1), 2 * bw, 1, skey, vpool,
        [&](uint32_t o, VsCell &cell) {
          const uint32_t r = o / bw, c = o - r * bw;
          vs_cell(beta2, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw], cell);
          cell.site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt));
        },
        [&](uint32_t o) {
          return vs_kappa_exact(beta2, th0[o + bw] + th1[o] - th1[o + 1], th0[o - bw] + th1[o - bw + 1] - th1[o - bw]);
        },
        [&](uint32_t o, double v) { th0[o] = v; });
    __syncthreads();
    MLMCPI_STAMP(5 + par);
  }
  for (uint32_t par = 0; par < 2; ++par) {  // mu = 1: rows [HB, HB + TH), even columns up to HB + TW, odd ones up to HB + TW - 1
    const uint32_t c_first = HB + par, c_hi1 = par ? HB + TW - 1 : HB + TW;
    const uint32_t nc = (c_hi1 - c_first) / 2 + 1;
    if (!STEP)
      heatbath_region<NT, 5, true>(
          TH, nc, skey, hpool,
          [&](uint32_t ri, uint32_t ci, double &tau, double &centre, uint32_t &site, uint32_t &o) {
            const uint32_t r = HB + ri, c = c_first + 2 * ci;
            o = r * bw + c;
            expcos_params(beta, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1], tau, centre);
            site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)) + 1;
          },
          [&](uint32_t o, double v) { th1[o] = v; });
    else if constexpr (kMapped) {
      // pass 0: a wave takes two rows and 32 columns per round -- lane l: row ri = 2 (w + NW k) + (l >> 5), column ci = l & 31;
      // the 33rd column of the even phase is left over
      const uint32_t r0 = HB + 2 * wave + (lane >> 5), c0 = c_first + 2 * (lane & 31u);
      uint32_t o_next = r0 * bw + c0;
      uint32_t rowmt = wrap(sr, r0, Mx) * Mt;
      const uint32_t scol = wrap(sc, c0, Mt), mxmt = Mx * Mt;
      heatbath_cells_step_mapped<NT, NIT, uint32_t>(
          (nc - 32) * (uint32_t)TH, skey, vpool,
          [&](uint32_t &o, uint32_t &site) {
            o = o_next;
            site = ((rowmt + scol) << 1) | 1u;
            o_next += 2 * NW * bw;
            rowmt += 2 * NW * Mt;
            rowmt = min(rowmt, rowmt - mxmt);   // (wraps once: the image is no taller than the lattice)
          },
          [&](uint32_t i) { return (HB + i) * bw + c_first + 64; },
          [&](uint32_t o) {
            const uint32_t r = o / bw, c = o - r * bw;
            return 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)) + 1;
          },
          [&](uint32_t o, double (&v)[6]) {   // from the address of th0[o - 1]
            const uint32_t a = lds_th0 + (o - 1) * 8u;
            v[0] = lds_read_f64<8>(a);                          // th0[o]
            v[1] = lds_read_f64<kT1 + 16>(a);                   // th1[o + 1]
            v[2] = lds_read_f64<bw * 8 + 8>(a);                 // th0[o + bw]
            v[3] = lds_read_f64<bw * 8>(a);                     // th0[o + bw - 1]
            v[4] = lds_read_f64<kT1>(a);                        // th1[o - 1]
            v[5] = lds_read_f64<0>(a);                          // th0[o - 1]
          },
          [&](const double (&v)[6], VsCell &cell) { vs_cell(beta2, v[0] + v[1] - v[2], v[3] + v[4] - v[5], cell); },
          [&](uint32_t o) {
            return vs_kappa_exact(beta2, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1]);
          },
          [&](uint32_t o, double v) { th1[o] = v; });
    } else
    heatbath_region_step<NT, 5, true, uint32_t>(
        TH, nc, HB * bw + c_first, bw, 2, skey, vpool,
        [&](uint32_t o, VsCell &cell) {
          const uint32_t r = o / bw, c = o - r * bw;
          vs_cell(beta2, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1], cell);
          cell.site = 2 * (wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)) + 1;
        },
        [&](uint32_t o) {
          return vs_kappa_exact(beta2, th0[o] + th1[o + 1] - th0[o + bw], th0[o + bw - 1] + th1[o - 1] - th0[o - 1]);
        },
        [&](uint32_t o, double v) { th1[o] = v; });
    __syncthreads();
    MLMCPI_STAMP(7 + par);
  }

  // write-out and the optional QoI, as in schwinger_sweep_kernel
  double acc[1] = {0.0};
  double2 *dst = out + (size_t)b * Mt * Mx;
  // (a tile on the upper / right edge of a lattice that 64 x 64 tiles do not divide reaches beyond it: those vertices are
  // periodic images of vertices another tile owns -- computed here like any halo, neither written nor counted)
  for_region<NT>(TH, TW, [&](uint32_t r, uint32_t c) {
    if (j0 + r >= Mx || i0 + c >= Mt) return;
    const uint32_t o = (r + HB) * bw + (c + HB);
    store_streaming(&dst[(size_t)(j0 + r) * Mt + (i0 + c)], th0[o], th1[o]);
    if (qoi_op) {
      const double thp = th0[o] + th1[o + 1] - th0[o + bw] - th1[o];
      acc[0] += qoi_op == 3 ? cos_reduced(thp) : mod_2pi(thp);
    }
  });
  if (qoi_op) {
    block_sum<1>(acc, qoi_red);
    if (threadIdx.x == 0) qoi_partial[(size_t)b * gridDim.x + tile] = acc[0];
  }
  MLMCPI_STAMP(9);
}

// ---- Schwinger overrelaxation in closed form: K sweeps are a fixed permutation of the plaquettes -----------------------
// With P(i, j) = theta_0(i, j) + theta_1(i+1, j) - theta_0(i, j+1) - theta_1(i, j) the two staple sums of the mu = 0 link at
// (i, j) are theta - P(i, j) and theta + P(i, j-1) (quenchedschwingeraction.cc:25-43), so its overrelaxation update
// (quenchedschwingeraction.cc:57-65) is
//     theta <- theta + P(i, j-1) - P(i, j)   (mod 2 pi),
// after which P(i, j) and P(i, j-1) have changed places; likewise theta_1(i, j) <- theta_1 + P(i, j) - P(i-1, j) swaps
// P(i, j) and P(i-1, j).  In the multicolour order of the sweeps here -- (mu = 0, j even), (mu = 0, j odd), (mu = 1, i even),
// (mu = 1, i odd) -- a colour phase therefore swaps whole rows (columns) of plaquettes pairwise, and one sweep moves the
// plaquette at an even row (column) index two rows (columns) down and the one at an odd index two up: after s sweeps
//     P_s(i, j) = P_0(i + 2 s e_i, j + 2 s e_j),   e_x = +1 for even x, -1 for odd x,
// whatever the field is.  Summing the increments of a link over K sweeps gives (s = 0 .. K - 1)
//     theta_0(i, j)  +=  sum_s  P_0(i + 2 s e_i, j - 1 - p_j - 2 s)  -  P_0(i + 2 s e_i, j + p_j + 2 s),        p_x = x mod 2,
//     theta_1(i, j)  +=  sum_s  P_0(i + p_i + 2 s, j + 2 (s + 1) e_j)  -  P_0(i - 1 - p_i - 2 s, j + 2 (s + 1) e_j),
// the same map as K sweeps of any other overrelaxation kernel here up to the rounding of 4 K additions (measured against
// them and against the oracle's sweeps: <= 3e-14 at K = 10).  A link costs 2 K LDS reads and 2 K additions instead of
// 9.3 K fp64 instructions, there is no halo recomputation (only the links that are wanted are computed), no colour
// phases and no barriers between sweeps; what remains is the halo of 2 K in the plaquettes a workgroup needs.
// Pairs: the two mu = 0 links of a column at rows (j, j + 1), j even, share their first stream (p_j cancels in it), and so
// do the two mu = 1 links of a row at columns (i, i + 1), i even, their second: a task is such a pair -- three streams of K
// plaquettes, two links.  With S, X, X' the sums over the shared stream and the two others (each in the order s = 0, 1, ...),
//     mu = 0:  theta_0(i, j) += S - X,  theta_0(i, j+1) += S - X';        mu = 1:  theta_1(i, j) += X - S,  theta_1(i+1, j) += X' - S.
// That order of operations is the definition: a result depends on the field and K only -- not on the tile, the batch, the
// workgroup size or the kernel (schwinger_perm_kernel == the first part of schwinger_perm_heat_kernel, bit for bit) -- but
// K sweeps in one launch and the same sweeps in two differ in the last bits.
//
// The plane: P_0 over `rows` x W vertices in LDS.  A wave takes 63 columns of a group of rows and walks up: lane l loads
// the double2 of column 63 cw + l, row by row -- the load of the next row is the theta_0(i, j+1) of this one, and
// theta_1(i+1, j) comes from lane l + 1 by DPP (lane 63 only serves lane 62): ONE coalesced 16-byte load per plaquette,
// U + 1 rows in flight per thread.  W + 1 <= Mt and rows + 1 <= Mx are not required: columns and rows wrap as often as
// needed (a 64 x 64 lattice is its own halo).
#ifndef MLMCPI_PERM_U
#define MLMCPI_PERM_U 0    // rows in flight per thread in the first plane build; 0 = all of a thread's rows at the deepest launch (19 at 512 threads; r05: one round trip to HBM instead of two, 10 + 9 rows: -4.2 % on the launch, same-box A/B)
#endif

// The plane in LDS.  Every stream of the closed form walks a diagonal of the plaquettes of ONE parity class: column and
// row parity do not change along it, the column moves by 2 e_c and the row by +-2 per step s.  So the plane is kept as four
// quadrants by (column parity, row parity), each Rh = rows / 2 rows of Wh = WP / 2 values, with the ODD index mirrored:
//     column C -> u = C / 2 (C even),  Wh - 1 - (C - 1) / 2 (C odd);      row R -> v = R / 2,  Rh - 1 - (R - 1) / 2 likewise.
// A step of any stream of any task is then (u, v) -> (u + 1, v + 1): ONE byte stride, kStep, for all of them -- whatever
// the parities, mu = 0 or 1 -- and with the pitch WP a compile-time constant (the width of the deepest launch, kPermMaxK
// sweeps; a shallower one leaves columns unused) the K reads of a stream are K immediate offsets from one address.  (The
// row-major plane this replaces cost 6.6 integer instructions of address arithmetic per read: a third of the launch's
// vector instructions outside the heat bath.)  Same values, same order of additions: results are bit for bit those of the
// row-major form.
template <int WP>
struct PermPlane {
  static constexpr int Wh = WP / 2, kRow = Wh * 8, kStep = kRow + 8;   // bytes
  uint32_t Rh, QB;                                                      // rows per quadrant; bytes per quadrant
  __device__ __forceinline__ explicit PermPlane(uint32_t rows) : Rh(rows / 2), QB((rows / 2) * (uint32_t)kRow) {}
  // byte offset of plaquette (C, R) = col(C) + row(R)
  __device__ __forceinline__ uint32_t col(uint32_t C) const { return (C & 1u) ? QB + (uint32_t)(Wh - 1 - (int)(C >> 1)) * 8u : (C >> 1) * 8u; }
  __device__ __forceinline__ uint32_t row(uint32_t R) const { return (R & 1u) ? 2u * QB + (Rh - 1u - (R >> 1)) * (uint32_t)kRow : (R >> 1) * (uint32_t)kRow; }
};

// where a thread stands in a build: its theta column, its rows [r, rend) of the `rows`, whether it owns a plaquette column
struct PermBuildPos {
  uint32_t c, r, rend, row_off, gj;   // row_off = gj Mt: the lattice row of build row r, in vertices (< 2^32: check_lattice)
  uint32_t cb;                        // PermPlane::col of the plaquette column
  const double2 *p;                   // src + the lattice column
  bool active, owns;
};
template <int NT, class PP>
__device__ __forceinline__ PermBuildPos perm_build_pos(const PP &P, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx, uint32_t gi0,
                                                       uint32_t gj0, uint32_t W, uint32_t rows) {
  PermBuildPos q;
  // (the wave index on the scalar side: rows, row offsets and the loop conditions of the build are then scalar too)
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  const uint32_t nwc = W > 63 ? 2 : 1;                                // column waves per row group (W <= 108: at most 2)
  const uint32_t groups = (NT / kWave) >> (nwc - 1);                   // row groups
  const uint32_t g = wave >> (nwc - 1), cw = wave & (nwc - 1);
  static_assert(((NT / kWave) & (NT / kWave - 1)) == 0, "waves per workgroup: a power of two (shifts for divisions)");
  const uint32_t rpg = groups == 4 ? (rows + 3) >> 2 : groups == 8 ? (rows + 7) >> 3 : (rows + groups - 1) / groups;
  q.c = 63 * cw + lane;                                                // theta column; the plaquette column of lanes 0 .. 62
  q.r = g * rpg;
  q.rend = g < groups ? min(rows, q.r + rpg) : 0;
  q.active = q.r < q.rend && q.c <= W;   // (not: whole waves, or the lanes beyond theta column W, which nobody reads)
  q.owns = lane < 63 && q.c < W;
  q.cb = P.col(q.c);
  q.p = src + wrap_add(gi0, q.c, Mt);
  q.gj = wrap_add(gj0, q.r, Mx);
  q.row_off = q.gj * Mt;
  return q;
}
// rows (q.r, min(q.r + U, q.rend)] of the thread's column into nxt[0 .. U); first: row q.r itself into cur
template <int U>
__device__ __forceinline__ void perm_rows_load(PermBuildPos &q, uint32_t Mt, uint32_t Mx, bool first, double2 &cur, double2 (&nxt)[U]) {
  if (!q.active) return;
  if (first) cur = q.p[q.row_off];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    q.gj = q.gj + 1 == Mx ? 0 : q.gj + 1;
    q.row_off = q.gj == 0 ? 0 : q.row_off + Mt;
    if (q.r + u < q.rend) nxt[u] = q.p[q.row_off];
  }
}
// their plaquettes into the plane (build row 0 = plane row R0); cur <- the last row, for the next chunk
template <int U, class PP>
__device__ __forceinline__ void perm_rows_store(PermBuildPos &q, const PP &P, double *plane, uint32_t R0, double2 &cur, const double2 (&nxt)[U]) {
  if (!q.active) return;
  char *const pb = reinterpret_cast<char *>(plane) + q.cb;
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (q.r + u < q.rend) {
      const double right = wave_rotate_down(cur.y);   // theta_1 of the next column
      if (q.owns) *reinterpret_cast<double *>(pb + P.row(R0 + q.r + u)) = ((cur.x + right) - nxt[u].x) - cur.y;   // (the row part is scalar)
      cur = nxt[u];
    }
  q.r += U;
}
template <int NT, int U, class PP>
__device__ __forceinline__ void perm_build_rows(const PP &P, double *plane, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx,
                                                uint32_t gi0, uint32_t gj0, uint32_t W, uint32_t rows) {
  PermBuildPos q = perm_build_pos<NT>(P, src, Mt, Mx, gi0, gj0, W, rows);
  double2 cur = make_double2(0., 0.);
  bool first = true;
  while (__builtin_amdgcn_readfirstlane(q.r) < __builtin_amdgcn_readfirstlane(q.rend)) {   // (uniform per wave)
    double2 nxt[U];
    perm_rows_load<U>(q, Mt, Mx, first, cur, nxt);
    perm_rows_store<U>(q, P, plane, 0u, cur, nxt);
    first = false;
  }
}

// The tasks of a half and who takes them.  A task is a column pair (mu = 0: rows r, r + 1 of column c) or a row pair
// (mu = 1: columns c, c + 1 of row r), coordinates inside the half.  r05: whole WAVES take whole rows -- wave-task m of a
// half is, for m < HR / 2, the mu = 0 tasks of row pair m in columns 0 .. 63 (lane l: the even columns on lanes 0 .. 31,
// the odd ones on 32 .. 63: a 32-lane group of a gather read stays inside one quadrant of the plane, contiguous banks),
// and for m >= HR / 2 the mu = 1 tasks of rows 2 (m - HR / 2) + (l >> 5) in column pairs l & 31; wave w takes m = w, w + NW,
// ... (slot k: m = w + NW k).  The kind of a slot and the row of its tasks are then wave-uniform and the column of a lane
// is the same in every slot: what was ~65 vector instructions of index arithmetic per task in the three places that need
// coordinates (own angles, gather, image) is scalar work plus a few additions.  The columns beyond 64 of the 68-wide
// output of the fused launch (4 x HR / 2 mu = 0 tasks, 2 x HR mu = 1 tasks) are left-over wave-tasks of one kind each, in
// the last slot of waves that have no main task there.  Which lane computes a task does not enter its result.
template <int NT, int RING, int TH = 64>
struct PermTasks {
  using PG = PermGeom<NT, RING, TH>;
  static constexpr int OW = PG::OW, HR = PG::HR, H2 = HR / 2, NW = NT / kWave, NS = (HR + NW - 1) / NW;
  static constexpr int XC = OW - 64;                                   // columns beyond a wave's 64 (0 or 4)
  static constexpr int L0 = XC * H2, L1 = (XC / 2) * HR;               // left-over tasks, mu = 0 and mu = 1
  static constexpr int NL0 = (L0 + 63) / 64, NL1 = (L1 + 63) / 64;     // ... as wave-tasks
  static constexpr int WF = HR - NW * (NS - 1);                        // the first wave without a main task in slot NS - 1
  static_assert(PG::NV == NS, "slots per thread");
  static_assert(NL0 + NL1 <= NW - WF, "the left-over wave-tasks fit the free last slots");
  uint32_t wave, lane, c_mu0, c_mu1, r_lo;
  __device__ PermTasks() {
    wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    lane = threadIdx.x % kWave;
    c_mu0 = lane < 32 ? 2 * lane : 2 * (lane - 32) + 1;
    c_mu1 = 2 * (lane & 31u);
    r_lo = lane >> 5;
  }
  // slot k of this thread: false when there is no task in it; mu1 is wave-uniform
  __device__ __forceinline__ bool task(int k, bool &mu1, uint32_t &r, uint32_t &c) const {
    const uint32_t m = wave + (uint32_t)(NW * k);
    mu1 = false; r = 0; c = 0;
    if (NW * k + NW - 1 < H2 || m < (uint32_t)H2) {            // (the first clause: known at compile time for the early slots)
      r = 2 * m;
      c = c_mu0;
      return true;
    }
    if (m < (uint32_t)HR) {
      mu1 = true;
      r = 2 * (m - H2) + r_lo;
      c = c_mu1;
      return true;
    }
    if (XC > 0 && k == NS - 1) {
      const uint32_t j = wave - (uint32_t)WF;
      if (j < (uint32_t)NL0) {                                // mu = 0, columns 64 ..: task L = row pair L / XC, column 64 + L % XC
        const uint32_t L = 64 * j + lane;
        r = 2 * (L / (XC ? XC : 1));
        c = 64 + L % (XC ? XC : 1);
        return L < (uint32_t)L0;
      }
      if (j < (uint32_t)(NL0 + NL1)) {                        // mu = 1, column pairs 32 ..: row L / (XC / 2), column 64 + 2 (L % (XC / 2))
        const uint32_t L = 64 * (j - NL0) + lane;
        mu1 = true;
        r = L / (XC > 1 ? XC / 2 : 1);
        c = 64 + 2 * (L % (XC > 1 ? XC / 2 : 1));
        return L < (uint32_t)L1;
      }
    }
    return false;
  }
  __device__ __forceinline__ bool valid(int k) const {
    bool mu1; uint32_t r, c;
    return task(k, mu1, r, c);
  }
  __device__ __forceinline__ bool is_mu1(int k) const {
    bool mu1; uint32_t r, c;
    task(k, mu1, r, c);
    return mu1;
  }
  __device__ __forceinline__ void coords(int k, uint32_t &r, uint32_t &c) const {
    bool mu1;
    task(k, mu1, r, c);
  }
};

// Five steps of the three streams of a task: fifteen 8-byte LDS reads at immediate offsets from three addresses, through
// inline asm (lds_read_f64: the compiler would pair the reads of a stream into ds_read2_b64, half the rate --
// MI355X_MICROARCH.md, LDS table), one wait naming all fifteen, then the additions in the order s = 0, 1, ...
template <int STEP>
__device__ __forceinline__ void perm_gather5(uint32_t pa, uint32_t px, uint32_t px2, double &S, double &X, double &X2) {
  double a0 = lds_read_f64<0>(pa), x0 = lds_read_f64<0>(px), y0 = lds_read_f64<0>(px2);
  double a1 = lds_read_f64<STEP>(pa), x1 = lds_read_f64<STEP>(px), y1 = lds_read_f64<STEP>(px2);
  double a2 = lds_read_f64<2 * STEP>(pa), x2 = lds_read_f64<2 * STEP>(px), y2 = lds_read_f64<2 * STEP>(px2);
  double a3 = lds_read_f64<3 * STEP>(pa), x3 = lds_read_f64<3 * STEP>(px), y3 = lds_read_f64<3 * STEP>(px2);
  double a4 = lds_read_f64<4 * STEP>(pa), x4 = lds_read_f64<4 * STEP>(px), y4 = lds_read_f64<4 * STEP>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a0), "+v"(x0), "+v"(y0), "+v"(a1), "+v"(x1), "+v"(y1), "+v"(a2), "+v"(x2), "+v"(y2), "+v"(a3), "+v"(x3), "+v"(y3),
                 "+v"(a4), "+v"(x4), "+v"(y4)
               :
               : "memory");
  S += a0; X += x0; X2 += y0;
  S += a1; X += x1; X2 += y1;
  S += a2; X += x2; X2 += y2;
  S += a3; X += x3; X2 += y3;
  S += a4; X += x4; X2 += y4;
}
__device__ __forceinline__ void perm_gather1(uint32_t pa, uint32_t px, uint32_t px2, double &S, double &X, double &X2) {
  double a0 = lds_read_f64<0>(pa), x0 = lds_read_f64<0>(px), y0 = lds_read_f64<0>(px2);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(x0), "+v"(y0) : : "memory");
  S += a0; X += x0; X2 += y0;
}

// res[h][k] = the new angles of the two links of task k of half h
template <int NT, int RING, int TH = 64>
__device__ __forceinline__ void perm_sweeps(double *plane, const double2 *__restrict__ src, uint32_t Mt, uint32_t Mx, uint32_t i0,
                                            uint32_t j0, uint32_t K, uint32_t NB, double2 (&res)[2][PermGeom<NT, RING, TH>::NV]) {
  using PG = PermGeom<NT, RING, TH>;
  using PP = PermPlane<PG::WP>;
  constexpr int HR = PG::HR, NV = PG::NV;
  // all of a thread's rows at the deepest launch: (HR + 4 kPermMaxK) rows over (NT / 64) / 2 row groups (W > 63: two column waves)
  constexpr int kGroups = NT / kWave / 2;
  constexpr int U = MLMCPI_PERM_U ? MLMCPI_PERM_U : (HR + 4 * (int)kPermMaxK + kGroups - 1) / kGroups, UB = (HR + kGroups - 1) / kGroups;   // rows in flight per thread: first build (nothing else is live yet), new rows of the second
  const uint32_t W = PG::width(K), rows = PG::rows(K, NB), H = RING + 2 * K;
  const PP P(rows);
  // lattice coordinates of plane (0, 0) of the first build, and of output vertex (0, 0)
  // (x - h) mod n for x < n: a comparison where h <= n -- the rule; the two modulo operations of the general form are ~80
  // instructions each in front of the first load of the workgroup
  auto back = [](uint32_t x, uint32_t h, uint32_t n) { return h <= n ? (x >= h ? x - h : x + n - h) : (x + n - h % n) % n; };
  const uint32_t gi0 = back(i0, H, Mt), gj0 = back(j0, H, Mx);
  const uint32_t oi0 = back(i0, RING, Mt), oj0 = back(j0, RING, Mx);
  const PermTasks<NT, RING, TH> tasks;
  // the links of a half as they are now (HR, RING, 2 K and the tile origins are even: output parity = plane parity = lattice parity)
  // (32-bit byte offsets from the chain's base pointer -- the host admits lattices of less than 2^28 vertices to these
  // kernels --, wraps by the unsigned-minimum trick: v >= n ? v - n : v = min(v, v - n); twice more for extents below
  // the output window's, a uniform branch.  The 64-bit pointer form this replaces cost 30 vector instructions per task.)
  const char *const src_b = reinterpret_cast<const char *>(src);
  const bool small_lattice = Mx < (uint32_t)(2 * HR + 2) || Mt < (uint32_t)(PG::OW + 2);   // (uniform: two copies of the loop)
  auto load_theta_of = [&](int h, double2 (&th)[NV], auto small) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (!tasks.valid(k)) continue;
      uint32_t r, c;
      tasks.coords(k, r, c);
      uint32_t gr = oj0 + r + h * HR, gc = oi0 + c;
      gr = min(gr, gr - Mx);
      gc = min(gc, gc - Mt);
      if ((bool)small) {
        gr = min(gr, gr - Mx); gr = min(gr, gr - Mx);
        gc = min(gc, gc - Mt); gc = min(gc, gc - Mt);
      }
      const uint32_t o = (gr * Mt + gc) * 16u;
      if (!tasks.is_mu1(k)) {
        const uint32_t o2 = gr + 1 == Mx ? o - gr * Mt * 16u : o + Mt * 16u;
        th[k] = make_double2(*reinterpret_cast<const double *>(src_b + o), *reinterpret_cast<const double *>(src_b + o2));
      } else {
        const uint32_t o2 = gc + 1 == Mt ? o - gc * 16u : o + 16u;
        th[k] = make_double2(*reinterpret_cast<const double *>(src_b + o + 8u), *reinterpret_cast<const double *>(src_b + o2 + 8u));
      }
    }
  };
  auto load_theta = [&](int h, double2 (&th)[NV]) {
    if (small_lattice) load_theta_of(h, th, std::true_type{}); else load_theta_of(h, th, std::false_type{});
  };
  // what K sweeps add to them
  auto gather = [&](int h, double2 (&d)[NV]) {
    const uint32_t row_off = 2 * K + (NB == 2 ? 0 : h * HR);  // plane row of output row 0 of this half (even)
    const uint32_t lds0 = (uint32_t)(uintptr_t)plane;   // the LDS byte address of the plane (lds_read_f64)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (!tasks.valid(k)) continue;
      uint32_t r, c;
      tasks.coords(k, r, c);
      // the shared stream, the first of the two others and the second, at s = 0 (plane coordinates C = c + 2 K, R = r + row_off):
      //   mu = 0 (R even): A_s = P(C + 2 s e_C, R - 1 - 2 s), B_s = P(C + 2 s e_C, R + 2 s), B'_s two rows above B_s;
      //   mu = 1 (C even): D_s = P(C - 1 - 2 s, J_s), J_s = R + 2 (s + 1) e_R, C_s = P(C + 2 s, J_s), C'_s two columns on;
      // in quadrant coordinates every one of them advances by (1, 1) per s
      const uint32_t C = c + 2 * K, R = r + row_off, Rq = R >> 1;
      uint32_t a, x, x2;
      if (!tasks.is_mu1(k)) {
        const uint32_t cb = P.col(C);
        x = cb + Rq * (uint32_t)PP::kRow;                       // row R, even: v = R / 2
        x2 = x + (uint32_t)PP::kRow;
        a = cb + 2u * P.QB + (P.Rh - Rq) * (uint32_t)PP::kRow;  // row R - 1, odd: v = Rh - 1 - (R / 2 - 1)
      } else {
        // J_0 = R + 2 (v = R / 2 + 1) for even R, R - 2 (v = Rh - 1 - ((R - 1) / 2 - 1)) for odd R
        const uint32_t rb = (R & 1u) ? 2u * P.QB + (P.Rh - Rq) * (uint32_t)PP::kRow : (Rq + 1u) * (uint32_t)PP::kRow;
        x = rb + (C >> 1) * 8u;                                  // column C, even: u = C / 2
        x2 = x + 8u;
        a = rb + P.QB + ((uint32_t)PP::Wh - (C >> 1)) * 8u;      // column C - 1, odd: u = Wh - 1 - (C / 2 - 1)
      }
      uint32_t pa = lds0 + a, px = lds0 + x, px2 = lds0 + x2;
      double S = 0.0, X = 0.0, X2 = 0.0;
      uint32_t s = 0;
      for (; s + 5 <= K; s += 5) {
        perm_gather5<PP::kStep>(pa, px, px2, S, X, X2);
        pa += 5 * PP::kStep;
        px += 5 * PP::kStep;
        px2 += 5 * PP::kStep;
      }
      for (; s < K; ++s) {
        perm_gather1(pa, px, px2, S, X, X2);
        pa += PP::kStep;
        px += PP::kStep;
        px2 += PP::kStep;
      }
      d[k] = tasks.is_mu1(k) ? make_double2(X - S, X2 - S) : make_double2(S - X, S - X2);
    }
  };
  auto finish = [&](const double2 (&th)[NV], double2 (&d)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (tasks.valid(k)) d[k] = make_double2(mod_2pi_fast(th[k].x + d[k].x), mod_2pi_fast(th[k].y + d[k].y));
  };

  perm_build_rows<NT, U>(P, plane, src, Mt, Mx, gi0, gj0, W, rows);
  double2 th[NV];
  if (NB == 1) {
    // one plane: first half (its angles are in flight across the barrier and the first reads of the plane), second half
    load_theta(0, th);
    __syncthreads();
    MLMCPI_STAMP(1);  // plane built
    gather(0, res[0]);
    finish(th, res[0]);
    MLMCPI_STAMP(2);  // first half gathered
    load_theta(1, th);
    gather(1, res[1]);
    finish(th, res[1]);
    return;
  }
  // NB = 2: the HR new rows of the second plane are loaded while the first half is gathered (at most UB rows per thread:
  // HR / 4 row groups); the angles of the first half only after it, so that the gather has the registers
  PermBuildPos qb = perm_build_pos<NT>(P, src, Mt, Mx, gi0, wrap_add(gj0, rows, Mx), W, HR);
  double2 curb = make_double2(0., 0.), vb[UB];
  __syncthreads();
  MLMCPI_STAMP(1);  // plane built
  perm_rows_load<UB>(qb, Mt, Mx, true, curb, vb);
  gather(0, res[0]);
  MLMCPI_STAMP(2);  // first half gathered
  // rows [HR, rows) of the plane become rows [0, rows - HR), the HR new rows go on top.  HR is even: a row keeps its parity
  // and moves by HR / 2 quadrant rows -- down in the quadrants of the even rows, up (mirrored) in those of the odd rows
  constexpr int NC = (4 * 2 * (int)kPermMaxK * PP::Wh + NT - 1) / NT;   // 4 quadrants x (rows - HR) / 2 = 2 K quadrant rows
  const uint32_t nkeep = (rows - HR) / 2 * (uint32_t)PP::Wh, shift = (uint32_t)(HR / 2) * (uint32_t)PP::kRow;
  {
    double keep[NC];
    char *const pbw = reinterpret_cast<char *>(plane);
    // (a thread reads what it moves as soon as its own gather is done -- reads beside the reads of the gathers still running
    // -- and ONE barrier separates every read of the old plane, the gathers' and these, from the writes; the barrier that
    // used to stand in front of these reads as well was worth 0.1 % of the launch, same-box A/B)
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const uint32_t idx = threadIdx.x + q * NT, e = idx >> 2, qd = idx & 3u;
      if (e < nkeep) keep[q] = *reinterpret_cast<const double *>(pbw + qd * P.QB + e * 8u + ((qd & 2u) ? 0u : shift));
    }
    __syncthreads();  // the first half has read its plane, and so have the threads that move its rows
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const uint32_t idx = threadIdx.x + q * NT, e = idx >> 2, qd = idx & 3u;
      if (e < nkeep) *reinterpret_cast<double *>(pbw + qd * P.QB + e * 8u + ((qd & 2u) ? shift : 0u)) = keep[q];
    }
  }
  perm_rows_store<UB>(qb, P, plane, rows - HR, curb, vb);
  load_theta(0, th);   // (earlier -- before the rows move, or before they are stored -- costs a spill or gains nothing: EXPERIMENTS 0.1, 0.6)
  double2 th1[NV];
  load_theta(1, th1);
  __syncthreads();
  MLMCPI_STAMP(10);  // second plane built
  finish(th, res[0]);   // (behind the gather instead: 48 bytes of spills)
  gather(1, res[1]);
  finish(th1, res[1]);
}

// the angles of perm_sweeps into the planes th0, th1 of an OW x 2 HR image (the caller puts barriers around it)
template <int NT, int RING, int TH = 64>
__device__ __forceinline__ void perm_store_image(double *th0, double *th1, const double2 (&res)[2][PermGeom<NT, RING, TH>::NV]) {
  using PG = PermGeom<NT, RING, TH>;
  constexpr int OW = PG::OW, HR = PG::HR, NV = PG::NV;
  const PermTasks<NT, RING, TH> tasks;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (!tasks.valid(k)) continue;
      uint32_t r, c;
      tasks.coords(k, r, c);
      const uint32_t o = (r + h * HR) * OW + c;
      if (!tasks.is_mu1(k)) {
        th0[o] = res[h][k].x;
        th0[o + OW] = res[h][k].y;
      } else {
        th1[o] = res[h][k].x;
        th1[o + 1] = res[h][k].y;
      }
    }
}

// K <= kPermMaxK overrelaxation sweeps of a 64 x TH tile per workgroup; lds = perm_lds_bytes<TH>(K, NB)
template <int TH>
__global__ void __launch_bounds__(512, 4)
    schwinger_perm_kernel(uint32_t Mt, uint32_t Mx, const double2 *__restrict__ in, double2 *__restrict__ out, uint32_t tiles_x,
                          uint32_t K, uint32_t NB) {
  constexpr int NT = 512;
  using PG = PermGeom<NT, 0, TH>;
  extern __shared__ double lds[];
  const uint32_t tile = blockIdx.x, b = blockIdx.y;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * 64, j0 = ty * TH;
  double2 res[2][PG::NV];
  perm_sweeps<NT, 0, TH>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, K, NB, res);
  double *th0 = lds, *th1 = lds + 64 * TH;
  __syncthreads();  // the plane is dead: the image takes its place
  perm_store_image<NT, 0, TH>(th0, th1, res);
  __syncthreads();
  double2 *dst = out + (size_t)b * Mt * Mx;
#pragma unroll
  for (int k = 0; k < 64 * TH / NT; ++k) {  // a wave writes a row of the tile
    const uint32_t v = threadIdx.x + k * NT, r = v / 64, c = v % 64;
    if (j0 + r < Mx && i0 + c < Mt)   // (an edge tile of a lattice the tiles do not divide: see schwinger_image_heat)
      store_streaming(&dst[(size_t)(j0 + r) * Mt + (i0 + c)], th0[v], th1[v]);
  }
}

// K overrelaxation sweeps in closed form, then the heat-bath sweep, the QoI and the write-out on the LDS image
// (schwinger_image_heat, HeatImageGeom): the whole draw of the reference's sampler (10 + 1 sweeps) is ONE launch with one
// round trip of the state through HBM.  LDS: tables + list | the plane, then the image in the same place.
template <int NT, bool STEP>
__global__ void __launch_bounds__(NT, 4)
    schwinger_perm_heat_kernel(uint32_t Mt, uint32_t Mx, double beta, const double2 *__restrict__ in, double2 *__restrict__ out,
                               uint32_t tiles_x, uint32_t K, uint32_t NB, RngKey key0, int qoi_op, double *__restrict__ qoi_partial,
                               const uint32_t *__restrict__ vs_table) {
  using PH = PermHeatGeom<NT, STEP>;
  using PG = typename PH::PG;
  using OH = typename PH::OH;
  constexpr int IW = OH::IW, IH = OH::IH;
  static_assert(PG::OW == IW && 2 * PG::HR == IH, "the closed-form stage fills the heat bath's image");
  extern __shared__ double lds[];
  __shared__ double qoi_red[NT / kWave];
  const uint32_t tile = blockIdx.x, b = blockIdx.y;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * 64, j0 = ty * 64;
  MLMCPI_STAMP(0);
  MLMCPI_STAMP_WHERE();
  // the sampler's table: one word per thread, fetched now, put down when the sweeps are done (nothing waits for it here;
  // staged at the start it cost a round trip in front of the plane's loads: 1 % of the launch)
  uint32_t tabw = 0;
  if (STEP && threadIdx.x < kVsTableBytes / 4) tabw = vs_table[threadIdx.x];
  HbPool hpool = HbPool::carve(lds, STEP ? 0u : OH::hb_pool_cap);
  double *th0 = lds + OH::pool_bytes / sizeof(double), *th1 = th0 + IW * IH;
  double2 res[2][PG::NV];
  perm_sweeps<NT, 2>(th0, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, K, NB, res);
  MLMCPI_STAMP(3);  // K sweeps done
  VsPool<uint32_t> vpool = VsPool<uint32_t>::carve(lds, OH::pool_cap, nullptr);
  if (STEP) {
    if (threadIdx.x < kVsTableBytes / 4) reinterpret_cast<uint32_t *>(lds)[threadIdx.x] = tabw;
    if (threadIdx.x < 2) vpool.count[threadIdx.x] = 0;
    vpool.tab = VsTable::at(lds, vs_table);
  }
  __syncthreads();  // the plane is dead: the image takes its place
  perm_store_image<NT, 2>(th0, th1, res);
  __syncthreads();
  MLMCPI_STAMP(4);  // image down
  schwinger_image_heat<NT, STEP>(th0, th1, vpool, hpool, Mt, Mx, beta, out, i0, j0, b, tile, key0, qoi_op, qoi_partial, qoi_red);
}

// ---- host side ----------------------------------------------------------------------------------------------------
template <bool HEAT, int NT>
static int allow_full_lds() {
  // tiles with deep halos may use the whole 160 KiB of LDS
  // (the kernels also hold NT / 64 doubles of static LDS for the fused QoI reduction)
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)schwinger_sweep_kernel<HEAT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
  if (HEAT)
    MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)schwinger_sweep_kernel<HEAT, NT, 0, 0, HEAT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
  return MLMCPI_OK;
}

int schwinger_allow_lds() {
  if (int rc = allow_full_lds<false, 256>()) return rc;
  if (int rc = allow_full_lds<true, 256>()) return rc;
  if (int rc = allow_full_lds<false, 512>()) return rc;
  if (int rc = allow_full_lds<true, 512>()) return rc;
  if (int rc = allow_full_lds<false, 1024>()) return rc;
  if (int rc = allow_full_lds<true, 1024>()) return rc;
  // kernels whose LDS may exceed the 64 KiB default
  if (int rc = allow_lds((const void *)schwinger_or_block_kernel<5>, OrBlockGeom<5>::lds_bytes)) return rc;
  if (int rc = allow_lds((const void *)schwinger_or_block_kernel<6>, OrBlockGeom<6>::lds_bytes)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_kernel<64>, kPermPlaneMax)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_kernel<32>, kPermPlaneMax)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_heat_kernel<512, true>, HeatImageGeom::hb_bytes)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_heat_kernel<512, false>, HeatImageGeom::hb_bytes)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_heat_kernel<1024, true>, 156 * 1024)) return rc;
  if (int rc = allow_lds((const void *)schwinger_perm_heat_kernel<1024, false>, 156 * 1024)) return rc;
  return MLMCPI_OK;
}

template <bool HEAT, int NT>
static void launch_tile_sweep_nt(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  const TileGeom tg{l.tile_w, l.tile_h, l.tiles_x};
  const uint32_t n = l.n_overrelax + l.n_heatbath;
#define MLMCPI_SCHW_SWEEP(...)                                                                                                       \
  hipLaunchKernelGGL((schwinger_sweep_kernel<__VA_ARGS__>), grid, dim3(NT), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, (const double2 *)a.src, \
                     (double2 *)a.dst, tg, n, l.kinds, a.key, l.pool_cap, a.qoi_op, a.qoi_partial, a.vs_table)
  if (l.fixed_tile && l.step) MLMCPI_SCHW_SWEEP(HEAT, NT, 64, 32, HEAT);
  else if (l.fixed_tile) MLMCPI_SCHW_SWEEP(HEAT, NT, 64, 32);
  else if (l.step) MLMCPI_SCHW_SWEEP(HEAT, NT, 0, 0, HEAT);
  else MLMCPI_SCHW_SWEEP(HEAT, NT);
#undef MLMCPI_SCHW_SWEEP
}

static int launch_tile_sweep(const SweepLaunch &l, const SweepArgs &a) {
  const bool heat = l.n_heatbath != 0;
  switch (l.threads) {
    case 1024: heat ? launch_tile_sweep_nt<true, 1024>(l, a) : launch_tile_sweep_nt<false, 1024>(l, a); break;
    case 512: heat ? launch_tile_sweep_nt<true, 512>(l, a) : launch_tile_sweep_nt<false, 512>(l, a); break;
    default: heat ? launch_tile_sweep_nt<true, 256>(l, a) : launch_tile_sweep_nt<false, 256>(l, a);
  }
  MLMCPI_LAUNCH_CHECK("lattice sweep kernel");
  return MLMCPI_OK;
}

// schwinger_or_block_kernel: the depth is the launch's overrelaxation count
static int launch_blocks(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  return with_depth<6>(l.n_overrelax, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    hipLaunchKernelGGL(schwinger_or_block_kernel<K>, grid, dim3(l.threads), l.lds_bytes, a.st, a.Mt, a.Mx, (const double2 *)a.src,
                       (double2 *)a.dst, l.tiles_x);
    MLMCPI_LAUNCH_CHECK("register-block overrelaxation kernel");
    return MLMCPI_OK;
  });
}

static int launch_perm(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  const double2 *in = (const double2 *)a.src;
  double2 *out = (double2 *)a.dst;
#define MLMCPI_PERM_HEAT(NT, STEP)                                                                                           \
  hipLaunchKernelGGL((schwinger_perm_heat_kernel<NT, STEP>), grid, dim3(NT), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, in, out, \
                     l.tiles_x, l.n_overrelax, l.planes, a.key, a.qoi_op, a.qoi_partial, a.vs_table)
  if (l.kernel == MLMCPI_K_SCHWINGER_PERM_HEAT) {
    if (l.threads == 1024 && l.step) MLMCPI_PERM_HEAT(1024, true);
    else if (l.threads == 1024) MLMCPI_PERM_HEAT(1024, false);
    else if (l.step) MLMCPI_PERM_HEAT(512, true);
    else MLMCPI_PERM_HEAT(512, false);
  } else if (l.tile_h == 64)
    hipLaunchKernelGGL(schwinger_perm_kernel<64>, grid, dim3(512), l.lds_bytes, a.st, a.Mt, a.Mx, in, out, l.tiles_x, l.n_overrelax, l.planes);
  else
    hipLaunchKernelGGL(schwinger_perm_kernel<32>, grid, dim3(512), l.lds_bytes, a.st, a.Mt, a.Mx, in, out, l.tiles_x, l.n_overrelax, l.planes);
#undef MLMCPI_PERM_HEAT
  MLMCPI_LAUNCH_CHECK("schwinger closed-form kernel");
  return MLMCPI_OK;
}

// The kernels take the key of the launch's heat-bath sweep, which stands behind its overrelaxation sweeps (a generic launch has
// one kind of sweep only: that is its first).
int schwinger_sweep_launch(const SweepLaunch &l, const SweepArgs &args) {
  SweepArgs a = args;
  if (l.n_heatbath) a.key.step += l.n_overrelax;
  void *partial = nullptr;
  if (l.step)
    if (int rc = vs_table_device(2. * a.coupling, &a.vs_table)) return rc;
  if (a.qoi_op)
    if (int rc = scratch((size_t)a.B * l.grid_x * sizeof(double), &partial, a.st)) return rc;
  a.qoi_partial = (double *)partial;
  int rc;
  switch (l.kernel) {
    case MLMCPI_K_SCHWINGER_PERM:
    case MLMCPI_K_SCHWINGER_PERM_HEAT: rc = launch_perm(l, a); break;
    case MLMCPI_K_SCHWINGER_OR_BLOCK: rc = launch_blocks(l, a); break;
    default: rc = launch_tile_sweep(l, a);
  }
  if (!rc && a.qoi_op) rc = lattice_finish(a.qoi_partial, l.grid_x, a.B, a.qoi_op, 1.0 / ((double)a.Mx * a.Mt), a.d_qoi, a.d_acc, a.st);
  return rc;
}

int schwinger_site_updates(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, const uint32_t *d_sites, uint32_t n,
                           uint32_t site, int32_t heat, uint64_t seed, uint32_t chain0, uint32_t step, hipStream_t st) {
  const uint32_t *vs_table = nullptr;
  if (heat && 2. * act->beta <= kVsKappaMax)
    if (int rc = vs_table_device(2. * act->beta, &vs_table)) return rc;
  hipLaunchKernelGGL((lattice_site_update_kernel<true>), dim3((B + 63) / 64), dim3(64), 0, st, act->Mt, act->Mx, act->beta, d_state, B,
                     d_sites, n, site, (int)heat, make_key(seed, chain0, step), vs_table);
  MLMCPI_LAUNCH_CHECK("lattice_site_update_kernel");
  return MLMCPI_OK;
}

}  // namespace mlmcpi
