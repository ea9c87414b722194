// schwinger_sweeps.hip -- the sweep kernels of the quenched Schwinger model (U(1) link angles, plaquette action; one double2
// {theta_0, theta_1} per site) that draw from a sampler, and the launcher of all of them: the generic overlapped-tile kernel, the
// closed form of K overrelaxation sweeps (schwinger_perm.hpp) and the launch that runs the heat bath behind it.  The 4 x 4 register
// blocks, which draw nothing, are in schwinger_or_block.hip.  lattice2d.hip plans a draw and calls schwinger_sweep_launch once per
// launch; the sizes it plans with are in lattice_sweep.hpp.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include "lattice_sweep.hpp"
#include "schwinger_perm.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

#ifdef MLMCPI_STAMPS
// the stamps of the last launch of schwinger_perm_heat_kernel, 16 words per workgroup
extern "C" int mlmcpi_debug_read_stamps(unsigned long long *h_out, uint32_t n_workgroups) {
  MLMCPI_HIP_TRY(hipDeviceSynchronize());
  MLMCPI_HIP_TRY(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_stamps), (size_t)n_workgroups * 16 * sizeof(unsigned long long)));
  return MLMCPI_OK;
}
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

// K <= kPermMaxK overrelaxation sweeps of a 64 x TH tile per workgroup; lds = perm_lds_bytes<TH>()
template <int TH>
__global__ void __launch_bounds__(512, 4)
    schwinger_perm_kernel(uint32_t Mt, uint32_t Mx, const double2 *__restrict__ in, double2 *__restrict__ out, uint32_t tiles_x,
                          uint32_t K) {
  constexpr int NT = 512;
  using PG = PermGeom<NT, 0, TH>;
  extern __shared__ double lds[];
  const uint32_t tile = blockIdx.x, b = blockIdx.y;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * 64, j0 = ty * TH;
  double2 res[2][PG::NV];
  perm_sweeps<NT, 0, TH>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, K, res);
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
                               uint32_t tiles_x, uint32_t K, RngKey key0, int qoi_op, double *__restrict__ qoi_partial,
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
  perm_sweeps<NT, 2>(th0, in + (size_t)b * Mt * Mx, Mt, Mx, i0, j0, K, res);
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
  if (int rc = schwinger_or_block_allow_lds()) return rc;
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

static int launch_perm(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  const double2 *in = (const double2 *)a.src;
  double2 *out = (double2 *)a.dst;
#define MLMCPI_PERM_HEAT(NT, STEP)                                                                                           \
  hipLaunchKernelGGL((schwinger_perm_heat_kernel<NT, STEP>), grid, dim3(NT), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, in, out, \
                     l.tiles_x, l.n_overrelax, a.key, a.qoi_op, a.qoi_partial, a.vs_table)
  if (l.kernel == MLMCPI_K_SCHWINGER_PERM_HEAT) {
    if (l.threads == 1024 && l.step) MLMCPI_PERM_HEAT(1024, true);
    else if (l.threads == 1024) MLMCPI_PERM_HEAT(1024, false);
    else if (l.step) MLMCPI_PERM_HEAT(512, true);
    else MLMCPI_PERM_HEAT(512, false);
  } else if (l.tile_h == 64)
    hipLaunchKernelGGL(schwinger_perm_kernel<64>, grid, dim3(512), l.lds_bytes, a.st, a.Mt, a.Mx, in, out, l.tiles_x, l.n_overrelax);
  else
    hipLaunchKernelGGL(schwinger_perm_kernel<32>, grid, dim3(512), l.lds_bytes, a.st, a.Mt, a.Mx, in, out, l.tiles_x, l.n_overrelax);
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
    case MLMCPI_K_SCHWINGER_OR_BLOCK: rc = schwinger_or_block_launch(l, a); break;
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
