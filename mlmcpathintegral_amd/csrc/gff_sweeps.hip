// gff_sweeps.hip -- the sweep kernels of the Gaussian free field (vertex field, 5-point stencil; one double per site) and their
// launcher: the generic overlapped-tile kernel, the 4 x 4 register blocks and the launch that runs the heat bath behind them.
// lattice2d.hip plans a draw and calls gff_sweep_launch once per launch; the sizes it plans with are in lattice_sweep.hpp.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include "lattice_sweep.hpp"

namespace mlmcpi {

// ---- GFF sweeps --------------------------------------------------------------------------------------
// Red/black order: (i+j) even, then odd.  gffaction.cc:33-42 (heat bath), :68-77 (overrelaxation);
// Delta is summed in the order of the reference's neighbour table (+i, -i, +j, -j).
// TWC x THC > 0: single-sweep launch on a lattice that the TWC x THC tiles divide and that is wider than a buffer: tile and
// buffer extents are compile-time constants, as in schwinger_sweep_kernel (same updates, bit-identical results).
template <bool HEAT, int NT, int TWC = 0, int THC = 0>
__global__ void __launch_bounds__(NT)
    gff_sweep_kernel(uint32_t Mt, uint32_t Mx, double mu2, const double *__restrict__ in, double *__restrict__ out,
                     TileGeom tg, uint32_t nsweeps_arg, uint32_t kinds, RngKey key0, int qoi_op = 0,
                     double *__restrict__ qoi_partial = nullptr) {
  extern __shared__ double lds[];
  __shared__ double qoi_red[NT / 64];
  constexpr bool FIXED = TWC > 0;
  const uint32_t nsweeps = FIXED ? 1u : nsweeps_arg;
  const uint32_t H = 2 * nsweeps;
  const uint32_t tile = blockIdx.x, b = blockIdx.y;
  const uint32_t ty = tile / tg.tiles_x, tx = tile - ty * tg.tiles_x;
  const uint32_t i0 = tx * (FIXED ? TWC : tg.TW), j0 = ty * (FIXED ? THC : tg.TH);
  const uint32_t ow = FIXED ? TWC : min(tg.TW, Mt - i0), oh = FIXED ? THC : min(tg.TH, Mx - j0);
  auto wrap = [&](uint32_t base, uint32_t off, uint32_t n) {  // lattice coordinate of a buffer coordinate
    if (FIXED) {
      const uint32_t v = base + off;
      return v >= n ? v - n : v;
    }
    return wrap_add(base, off, n);
  };
  const uint32_t bw = ow + 2 * H, bh = oh + 2 * H;
  double *phi = lds;
  double *nrm = lds + (size_t)bw * bh;  // HEAT only: the second normal of each Box-Muller pair, by cell
  const uint32_t sc = (uint32_t)(((uint64_t)i0 + Mt - (H % Mt)) % Mt);
  const uint32_t sr = (uint32_t)(((uint64_t)j0 + Mx - (H % Mx)) % Mx);
  const double *src = in + (size_t)b * Mt * Mx;
  RngKey key = key0;
  key.chain += b;
  const double inv_kappa = 1. / (4. + mu2), two_over_kappa = 2. / (4. + mu2), sigma = 1. / sqrt(4. + mu2);
  const PhiloxVKeys vk = philox_vkeys(key.k0, key.k1);

  stage_region<NT, (NT >= 1024 ? 3 : 5), double>(
      bh, bw, [&](uint32_t r, uint32_t c) { return src[(size_t)wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt)]; },
      [&](uint32_t r, uint32_t c, double v) { phi[r * bw + c] = v; });
  __syncthreads();

  for (uint32_t s = 0; s < nsweeps; ++s) {
    const bool heat = HEAT && (FIXED || ((kinds >> s) & 1u));
    RngKey skey = key;
    skey.step += s;
    for (uint32_t colour = 0; colour < 2; ++colour) {
      // One Philox call + one Box-Muller per vertex PAIR (l >> 1): the two vertices of a pair are horizontal
      // neighbours (c, c ^ 1), hence of opposite colour.  The colour-0 phase draws the pair and parks the
      // partner's normal in LDS; the colour-1 phase picks it up.  Only colour-1 cells whose partner sits in an
      // outermost buffer column (never updated, so nothing was parked) draw the pair themselves: exactly one
      // cell per row (column 1 or bw - 2).  They get a pass of their own, so that the waves of the main
      // colour-1 pass never execute the Philox + Box-Muller code (one boundary lane would drag its whole wave
      // through it).
      auto stencil = [&](uint32_t o) {
        double Delta = 0.0;
        Delta += phi[o + 1];
        Delta += phi[o - 1];
        Delta += phi[o + bw];
        Delta += phi[o - bw];
        return Delta;
      };
      auto draw_pair = [&](uint32_t r, uint32_t c, bool park) {  // returns this cell's normal
        const uint32_t ell = wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt);
        double n0, n1;
        rng_normals(skey, vk, ell >> 1, P_GFF_NORMAL, 0, n0, n1);
        if (park) nrm[r * bw + (c ^ 1u)] = (ell & 1u) ? n0 : n1;
        return (ell & 1u) ? n1 : n0;
      };
      // Update region of this phase: rows [r_lo, r_lo + nrow), columns [c_lo, c_lo + 2 nhalf), cells of the phase's
      // colour.  In general everything but the outermost ring of the buffer; the LAST sweep of a launch is cut down to
      // what is still read afterwards: colour 1 (last phase) the owned tile, colour 0 the tile plus one ring.
      const bool last = s + 1 == nsweeps;
      const uint32_t grow = colour == 0 ? 1u : 0u;  // rings around the owned tile in the last sweep
      const uint32_t r_lo = last ? H - grow : 1, nrow = last ? oh + 2 * grow : bh - 2;
      const uint32_t c_lo = last ? H - grow : 1, nhalf = last ? (ow + 2 * grow) / 2 : (bw - 2) / 2;
      auto column = [&](uint32_t r, uint32_t ci) { return c_lo + ((r + c_lo + colour) & 1u) + 2 * ci; };
      if (!heat) {
        for_region<NT>(nrow, nhalf, [&](uint32_t ri, uint32_t ci) {
          const uint32_t r = r_lo + ri;
          const uint32_t o = r * bw + column(r, ci);
          phi[o] = fma(two_over_kappa, stencil(o), -phi[o]);  // 2 Delta / kappa - phi without the fp64 division
        });
      } else if (colour == 0) {
        for_region<NT>(nrow, nhalf, [&](uint32_t ri, uint32_t ci) {
          const uint32_t r = r_lo + ri;
          const uint32_t c = column(r, ci);
          const uint32_t o = r * bw + c;
          phi[o] = fma(stencil(o), inv_kappa, sigma * draw_pair(r, c, true));
        });
      } else if (last) {
        // every colour-1 cell of the tile has its pair partner (c ^ 1, same row) inside the colour-0 region above
        for_region<NT>(nrow, nhalf, [&](uint32_t ri, uint32_t ci) {
          const uint32_t r = r_lo + ri;
          const uint32_t o = r * bw + column(r, ci);
          phi[o] = fma(stencil(o), inv_kappa, sigma * nrm[o]);
        });
      } else {
        for_region<NT>(nrow, nhalf, [&](uint32_t ri, uint32_t ci) {
          const uint32_t r = r_lo + ri;
          const uint32_t c = column(r, ci);
          if (c == 1 || c == bw - 2) return;  // boundary partners: next pass
          const uint32_t o = r * bw + c;
          phi[o] = fma(stencil(o), inv_kappa, sigma * nrm[o]);
        });
        for_region<NT>(bh - 2, 1, [&](uint32_t ri, uint32_t) {
          const uint32_t r = 1 + ri;
          const uint32_t c = (r & 1u) ? bw - 2 : 1;  // the colour-1 cell of this row next to an outermost column
          const uint32_t o = r * bw + c;
          phi[o] = fma(stencil(o), inv_kappa, sigma * draw_pair(r, c, false));
        });
      }
      __syncthreads();
    }
  }

  // Optional fused QoI of the final state (qoi/qft/qoi2dphisquared.cc:8-15): phi^2 summed over the owned sites while the
  // tile is in LDS, one partial per tile; lattice_finish_kernel sums them in tile order.
  double acc[1] = {0.0};
  double *dst = out + (size_t)b * Mt * Mx;
  for_region<NT>(oh, ow, [&](uint32_t r, uint32_t c) {
    const double v = phi[(r + H) * bw + (c + H)];
    dst[(size_t)(j0 + r) * Mt + (i0 + c)] = v;
    if (qoi_op) acc[0] += v * v;
  });
  if (qoi_op) {
    block_sum<1>(acc, qoi_red);
    if (threadIdx.x == 0) qoi_partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
  }
}

// ---- GFF overrelaxation, 4 x 4 register blocks on T x T tiles (GffBlockGeom, lattice_sweep.hpp) ----------------------------
// The buffer of geometry G (tile + halo G::H) into 4 x 4 register blocks, then KS <= G::H / 2 overrelaxation sweeps; ends
// behind the barrier of the last colour phase (the plane area is dead from there on).
template <class G, int KS>
__device__ __forceinline__ void gff_block_sweeps(double *lds, const double *__restrict__ src, uint32_t Mt, uint32_t Mx, double mu2,
                                                 uint32_t i0, uint32_t j0, double (&p)[G::PH][G::PW]) {
  constexpr int PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NPY = G::NPY, NP = G::NP;
  static_assert(2 * KS <= H, "a sweep costs two sites of halo");
  auto pl = [&](int p) { return lds + p * NP; };
  const uint32_t tid = threadIdx.x;
  const bool active = tid < NP;
  const int pj = active ? (int)tid / NPX : 0, pi = active ? (int)tid - pj * NPX : 0;
  const int me = active ? (int)tid : 0;  // idle threads of the last wave: every index is entry 0, nothing is written
  const int dn = pj > 0 ? me - NPX : me, up = pj + 1 < NPY ? me + NPX : me;
  const int lf = pi > 0 ? me - 1 : me, rt = pi + 1 < NPX ? me + 1 : me;
  const double two_over_kappa = 2. / (4. + mu2);
  // p: [c][a] = site (PW pi + a, PH pj + c)
  {
    uint32_t gi[PW / 2], gj[PH];  // H is even: a pair of sites (gi, gi + 1) never straddles the wrap
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
        const double2 v = active ? *(const double2 *)(src + (size_t)gj[c] * Mt + gi[a / 2]) : make_double2(0, 0);
        p[c][a] = v.x;
        p[c][a + 1] = v.y;
      }
  }
  auto publish = [&](int a, int c, double v) {  // rim sites: a corner belongs to a row and a column, stored once
    const int p1 = c == PH - 1 ? G::top(a) : c == 0 ? G::bot(a) : -1;
    const int p2 = a == 0 ? G::left(c) : a == PW - 1 ? G::right(c) : -1;
    if (!active) return;
    if (p1 >= 0) pl(p1)[me] = v;
    if (p2 >= 0 && p2 != p1) pl(p2)[me] = v;
  };
#pragma unroll
  for (int c = 0; c < PH; ++c)
#pragma unroll
    for (int a = 0; a < PW; ++a) publish(a, c, p[c][a]);
  __syncthreads();

  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int col = 0; col < 2; ++col) {
      // neighbour values across the block's edges (they have the other colour: unchanged during this phase)
      double e_lf[PH], e_rt[PH], e_dn[PW], e_up[PW];
#pragma unroll
      for (int c = 0; c < PH; ++c) {
        if (((0 + c) & 1) == col) e_lf[c] = pl(G::right(c))[lf];
        if (((PW - 1 + c) & 1) == col) e_rt[c] = pl(G::left(c))[rt];
      }
#pragma unroll
      for (int a = 0; a < PW; ++a) {
        if (((a + 0) & 1) == col) e_dn[a] = pl(G::top(a))[dn];
        if (((a + PH - 1) & 1) == col) e_up[a] = pl(G::bot(a))[up];
      }
#pragma unroll
      for (int c = 0; c < PH; ++c)
#pragma unroll
        for (int a = 0; a < PW; ++a) {
          if (((a + c) & 1) != col) continue;
          // gffaction.cc:68-77, Delta summed in the order of the reference's neighbour table (+i, -i, +j, -j)
          double Delta = 0.0;
          Delta += a + 1 < PW ? p[c][a + 1 < PW ? a + 1 : 0] : e_rt[c];
          Delta += a > 0 ? p[c][a > 0 ? a - 1 : 0] : e_lf[c];
          Delta += c + 1 < PH ? p[c + 1 < PH ? c + 1 : 0][a] : e_up[a];
          Delta += c > 0 ? p[c > 0 ? c - 1 : 0][a] : e_dn[a];
          p[c][a] = fma(two_over_kappa, Delta, -p[c][a]);
          publish(a, c, p[c][a]);
        }
      __syncthreads();
    }
  }
}

template <int K, int T = 64>
__global__ void __launch_bounds__((GffBlockGeom<K, T>::NT))
    gff_or_block_kernel(uint32_t Mt, uint32_t Mx, double mu2, const double *__restrict__ in, double *__restrict__ out,
                        uint32_t tiles_x) {
  using G = GffBlockGeom<K, T>;
  constexpr int TW = G::TW, TH = G::TH, PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NP = G::NP;
  static_assert(PW == 4 && PH == 4, "the write-back moves 4 sites per block row");
  extern __shared__ double lds[];
  const uint32_t tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * TW, j0 = ty * TH;
  double p[PH][PW];
  gff_block_sweeps<G, K>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, mu2, i0, j0, p);

  // Owned sites: buffer columns [H, H + TW), rows [H, H + TH), written back through a per-wave transposition in LDS (the
  // planes are dead after the last barrier) so that a wave instruction covers whole rows: per block row the owners put
  // their 4 sites down as two double2, and lane l writes the pair (l & 1) of block 32 i + (l >> 1), i = 0, 1.
  const uint32_t wave0 = tid & ~63u, lane = tid & 63u;
  double2 *stage = reinterpret_cast<double2 *>(lds) + (wave0 / 64) * 128;
  double *dst = out + (size_t)b * Mt * Mx;
  int uq[2], ur[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int bt = (int)wave0 + 32 * i + (int)(lane >> 1);
    const int bj = bt / NPX, bi = bt - bj * NPX;
    uq[i] = PW * bi + 2 * (int)(lane & 1) - H;  // even, and TW is even: the pair is owned as a whole or not at all
    ur[i] = PH * bj - H;
    if (bt >= NP || uq[i] >= TW) uq[i] = -1;
  }
#pragma unroll
  for (int c = 0; c < PH; ++c) {
    stage[2 * lane] = make_double2(p[c][0], p[c][1]);
    stage[2 * lane + 1] = make_double2(p[c][2], p[c][3]);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double2 w = stage[64 * i + lane];
      const int r = ur[i] + c;
      // (r05: an edge tile of a lattice the tiles do not divide reaches beyond it -- periodic images of sites other tiles
      // own, computed like any halo, not written; Mt is even, so a pair lies inside or outside as a whole)
      if (uq[i] >= 0 && r >= 0 && r < TH && j0 + (uint32_t)r < Mx && i0 + (uint32_t)uq[i] < Mt)
        *(double2 *)(dst + (size_t)(j0 + r) * Mt + (i0 + uq[i])) = w;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- GFF: K overrelaxation sweeps and the heat-bath sweep behind them in one launch ----------------------------------
// The construction of schwinger_perm_heat_kernel (HeatImageGeom) for the scalar field: gff_block_sweeps on the geometry with halo 2K + 2,
// then the field on the tile and two rings as an LDS image (with the plane of parked Box-Muller partners behind it), the
// heat-bath sweep of gff_sweep_kernel<true, 256, 64, 32> in its pruned last-sweep form -- same cells, same Philox
// words, same arithmetic: bit-identical -- the phi^2 sum and the write-out.  The second normal of a Box-Muller pair is
// not parked in LDS here: the thread that draws the pair for a colour-0 cell (r, c) also updates the colour-1 cell
// (r, c ^ 1) and keeps its normal in a register (the two phases walk the same compile-time index space), so the image is
// the field alone and three workgroups fit a CU.
template <int K, int T = 64>
__global__ void __launch_bounds__((GffHeatGeom<K, T>::NT), 4)
    gff_or_heat_kernel(uint32_t Mt, uint32_t Mx, double mu2, const double *__restrict__ in, double *__restrict__ out,
                       uint32_t tiles_x, RngKey key0, int qoi_op, double *__restrict__ qoi_partial) {
  using OH = GffHeatGeom<K, T>;
  using G = typename OH::G;
  constexpr int NT = OH::NT, TW = G::TW, TH = G::TH, PW = G::PW, PH = G::PH, H = G::H, NPX = G::NPX, NP = G::NP;
  constexpr int HB = OH::HB, IW = OH::IW, IH = OH::IH, O = H - HB;  // image (0, 0) = buffer (O, O)
  extern __shared__ double lds[];
  __shared__ double qoi_red[NT / kWave];
  const uint32_t tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const uint32_t i0 = tx * TW, j0 = ty * TH;
  double p[PH][PW];
  gff_block_sweeps<G, K>(lds, in + (size_t)b * Mt * Mx, Mt, Mx, mu2, i0, j0, p);

  double *phi = lds;
  if (tid < NP) {
    const int pj = (int)tid / NPX, pi = (int)tid - pj * NPX;
#pragma unroll
    for (int c = 0; c < PH; ++c) {
      const int r = PH * pj + c - O;
      if (r < 0 || r >= IH) continue;
#pragma unroll
      for (int a = 0; a < PW; ++a) {
        const int q = PW * pi + a - O;
        if (q >= 0 && q < IW) phi[r * IW + q] = p[c][a];
      }
    }
  }
  __syncthreads();

  // the heat-bath sweep: the last-sweep regions of gff_sweep_kernel with H = HB, bw = IW, oh = TH, ow = TW
  constexpr uint32_t bw = IW;
  const uint32_t sc = i0 >= (uint32_t)HB ? i0 - HB : i0 + Mt - HB;  // lattice column of image column 0 (even)
  const uint32_t sr = j0 >= (uint32_t)HB ? j0 - HB : j0 + Mx - HB;
  auto wrap = [](uint32_t base, uint32_t off, uint32_t n) {
    const uint32_t v = base + off;
    return v >= n ? v - n : v;
  };
  RngKey skey = key0;
  skey.chain += b;
  const double inv_kappa = 1. / (4. + mu2), sigma = 1. / sqrt(4. + mu2);
  // the four neighbours as single ds_read_b64 at immediate offsets from the address of phi[o - bw] (the compiler pairs
  // phi[o - 1], phi[o + 1] into a ds_read2_b64: 8 LDS cycles against 2 + 2, MI355X_MICROARCH.md); summed in the order of
  // the reference's neighbour table (+i, -i, +j, -j)
  const uint32_t lds_phi = (uint32_t)(uintptr_t)phi;
  auto stencil_load = [&](uint32_t o, double (&v)[4]) {
    const uint32_t a = lds_phi + (o - bw) * 8u;
    v[0] = lds_read_f64<bw * 8 + 8>(a);
    v[1] = lds_read_f64<bw * 8 - 8>(a);
    v[2] = lds_read_f64<2 * bw * 8>(a);
    v[3] = lds_read_f64<0>(a);
  };
  auto stencil_sum = [&](double (&v)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
    double Delta = 0.0;
    Delta += v[0];
    Delta += v[1];
    Delta += v[2];
    Delta += v[3];
    return Delta;
  };
  // colour 0: the tile plus one ring, (TH + 2) x (TW + 2) / 2 cells; cell idx = tid + k NT of the thread, k < CELLS
  constexpr uint32_t nrow = TH + 2, nhalf = (TW + 2) / 2, total = nrow * nhalf, CELLS = (total + NT - 1) / NT;
  double partner[CELLS];  // the normal of (r, c ^ 1), the colour-1 cell of the same Box-Muller pair
  const PhiloxVKeys vk = philox_vkeys(skey.k0, skey.k1);
  // one colour-0 cell (image row r, column c, offset o, lattice site ell) and the parked normal of its pair
  auto cell0 = [&](uint32_t o, uint32_t ell, double &parked) {
    double n0, n1, nb[4];
    stencil_load(o, nb);   // in flight under the Philox call and the Box-Muller transform
    rng_normals(skey, vk, ell >> 1, P_GFF_NORMAL, 0, n0, n1);
    parked = (ell & 1u) ? n0 : n1;
    phi[o] = fma(stencil_sum(nb), inv_kappa, sigma * ((ell & 1u) ? n1 : n0));
  };
  auto cell1 = [&](uint32_t o, double parked) {
    double nb[4];
    stencil_load(o, nb);
    phi[o] = fma(stencil_sum(nb), inv_kappa, sigma * parked);
  };
  if constexpr (NT == 512 && T == 64) {
    // r05: cells by a closed-form map instead of by linear index (a division by 33, the parity of the row, two wraps and a
    // multiplication per cell and colour: ~29 of the ~240 vector instructions of a pair): a wave takes two rows x 32 cells
    // per round -- lane l: row 1 + 2 (w + 8 k) + (l >> 5), column 1 + (l >> 5) + 2 (l & 31), the same in every round --, four
    // rounds cover rows 1 .. 64; rows 65, 66 and the 33rd cell of every row (130 cells) are a fifth round of 130 threads,
    // as many as the linear hand-out leaves for its last.  Which lane draws a pair does not enter the result.
    static_assert(CELLS == 5 && nhalf == 33 && nrow == 66, "64 x 64 tile, 512 threads");
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave), lane = tid % kWave, rr = lane >> 5;
    const uint32_t r0 = 1 + 2 * wave + rr, c0 = 1 + rr + 2 * (lane & 31u);
    const uint32_t colw = wrap(sc, c0, Mt), mxmt = Mx * Mt;
    uint32_t rowmt = wrap(sr, r0, Mx) * Mt, o = r0 * bw + c0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      cell0(o, rowmt + colw, partner[k]);
      o += 16 * bw;
      rowmt += 16 * Mt;
      rowmt = min(rowmt, rowmt - mxmt);   // (one wrap: the image is no taller than the lattice)
    }
    // the fifth round: t < 66: rows 65, 66, cell t % 33; 66 <= t < 130: row 1 + (t - 66), the 33rd cell
    const bool extra = tid < 130;
    const uint32_t xr = tid < 66 ? 65 + tid / 33 : 1 + (tid - 66), xci = tid < 66 ? tid % 33 : 32;
    const uint32_t xc = HB - 1 + ((xr + HB - 1) & 1u) + 2 * xci, xo = xr * bw + xc;
    partner[4] = 0.0;
    if (extra) cell0(xo, wrap(sr, xr, Mx) * Mt + wrap(sc, xc, Mt), partner[4]);
    __syncthreads();
    // colour 1: the cell (r, c ^ 1) of every colour-0 cell, where that lies inside the tile
    const uint32_t c1 = c0 ^ 1u;
    const bool col_in = c1 >= (uint32_t)HB && c1 < (uint32_t)(HB + TW);
    o = r0 * bw + c1;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t r = r0 + 16 * k;
      if (col_in && r >= (uint32_t)HB && r < (uint32_t)(HB + TH)) cell1(o, partner[k]);
      o += 16 * bw;
    }
    const uint32_t xc1 = xc ^ 1u;
    if (extra && xr >= (uint32_t)HB && xr < (uint32_t)(HB + TH) && xc1 >= (uint32_t)HB && xc1 < (uint32_t)(HB + TW))
      cell1(xr * bw + xc1, partner[4]);
    __syncthreads();
  } else {
#pragma unroll
  for (uint32_t k = 0; k < CELLS; ++k) {
    const uint32_t idx = tid + k * NT;
    partner[k] = 0.0;
    if (idx >= total) continue;
    const uint32_t ri = idx / nhalf, r = HB - 1 + ri;
    const uint32_t c = HB - 1 + ((r + HB - 1) & 1u) + 2 * (idx - ri * nhalf);
    cell0(r * bw + c, wrap(sr, r, Mx) * Mt + wrap(sc, c, Mt), partner[k]);
  }
  __syncthreads();
  // colour 1: the tile; the cell (r, c ^ 1) of every colour-0 cell, where that lies inside the tile
#pragma unroll
  for (uint32_t k = 0; k < CELLS; ++k) {
    const uint32_t idx = tid + k * NT;
    if (idx >= total) continue;
    const uint32_t ri = idx / nhalf, r = HB - 1 + ri;
    const uint32_t c = (HB - 1 + ((r + HB - 1) & 1u) + 2 * (idx - ri * nhalf)) ^ 1u;
    if (r < (uint32_t)HB || r >= (uint32_t)(HB + TH) || c < (uint32_t)HB || c >= (uint32_t)(HB + TW)) continue;
    cell1(r * bw + c, partner[k]);
  }
  __syncthreads();
  }

  double acc[1] = {0.0};
  double *dst = out + (size_t)b * Mt * Mx;
  for_region<NT>(TH, TW, [&](uint32_t r, uint32_t c) {
    if (j0 + r >= Mx || i0 + c >= Mt) return;   // (the part of an edge tile beyond the lattice: see gff_or_block_kernel)
    const double v = phi[(r + HB) * bw + (c + HB)];
    dst[(size_t)(j0 + r) * Mt + (i0 + c)] = v;
    if (qoi_op) acc[0] += v * v;
  });
  if (qoi_op) {
    block_sum<1>(acc, qoi_red);
    if (threadIdx.x == 0) qoi_partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
template <bool HEAT, int NT>
static int allow_full_lds() {
  // tiles with deep halos may use the whole 160 KiB of LDS
  // (the kernels also hold NT / 64 doubles of static LDS for the fused QoI reduction)
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)gff_sweep_kernel<HEAT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
  return MLMCPI_OK;
}

int gff_allow_lds() {
  if (int rc = allow_full_lds<false, 256>()) return rc;
  if (int rc = allow_full_lds<true, 256>()) return rc;
  if (int rc = allow_full_lds<false, 512>()) return rc;
  if (int rc = allow_full_lds<true, 512>()) return rc;
  if (int rc = allow_full_lds<false, 1024>()) return rc;
  if (int rc = allow_full_lds<true, 1024>()) return rc;
  // kernels whose LDS may exceed the 64 KiB default
  for (uint32_t k = 1; k <= 5; ++k)
    if (int rc = with_depth<5>(k, [](auto kc) {
          constexpr int K = decltype(kc)::value;
          return allow_lds((const void *)gff_or_heat_kernel<K>, GffHeatGeom<K>::lds_bytes);
        }))
      return rc;
  return MLMCPI_OK;
}

template <bool HEAT, int NT>
static void launch_tile_sweep_nt(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  const TileGeom tg{l.tile_w, l.tile_h, l.tiles_x};
  const uint32_t n = l.n_overrelax + l.n_heatbath;
#define MLMCPI_GFF_SWEEP(...)                                                                                               \
  hipLaunchKernelGGL((gff_sweep_kernel<__VA_ARGS__>), grid, dim3(NT), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, a.src, a.dst, \
                     tg, n, l.kinds, a.key, a.qoi_op, a.qoi_partial)
  if (l.fixed_tile) MLMCPI_GFF_SWEEP(HEAT, NT, 64, 32);
  else MLMCPI_GFF_SWEEP(HEAT, NT);
#undef MLMCPI_GFF_SWEEP
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

// gff_or_block_kernel, gff_or_heat_kernel: the depth is the launch's overrelaxation count
template <int T>
static int launch_blocks(const SweepLaunch &l, const SweepArgs &a) {
  const dim3 grid(l.grid_x, a.B);
  if (l.kernel == MLMCPI_K_GFF_OR_HEAT)
    return with_depth<5>(l.n_overrelax, [&](auto kc) -> int {
      constexpr int K = decltype(kc)::value;
      hipLaunchKernelGGL((gff_or_heat_kernel<K, T>), grid, dim3(l.threads), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, a.src, a.dst,
                         l.tiles_x, a.key, a.qoi_op, a.qoi_partial);
      MLMCPI_LAUNCH_CHECK("gff_or_heat_kernel");
      return MLMCPI_OK;
    });
  return with_depth<6>(l.n_overrelax, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    hipLaunchKernelGGL((gff_or_block_kernel<K, T>), grid, dim3(l.threads), l.lds_bytes, a.st, a.Mt, a.Mx, a.coupling, a.src, a.dst,
                       l.tiles_x);
    MLMCPI_LAUNCH_CHECK("register-block overrelaxation kernel");
    return MLMCPI_OK;
  });
}

// The kernels take the key of the launch's heat-bath sweep, which stands behind its overrelaxation sweeps (a generic launch has
// one kind of sweep only: that is its first).
int gff_sweep_launch(const SweepLaunch &l, const SweepArgs &args) {
  SweepArgs a = args;
  if (l.n_heatbath) a.key.step += l.n_overrelax;
  void *partial = nullptr;
  if (a.qoi_op)
    if (int rc = scratch((size_t)a.B * l.grid_x * sizeof(double), &partial, a.st)) return rc;
  a.qoi_partial = (double *)partial;
  int rc;
  switch (l.kernel) {
    case MLMCPI_K_GFF_OR_BLOCK:
    case MLMCPI_K_GFF_OR_HEAT: rc = l.tile_w == 32 ? launch_blocks<32>(l, a) : launch_blocks<64>(l, a); break;
    default: rc = launch_tile_sweep(l, a);
  }
  if (!rc && a.qoi_op) rc = lattice_finish(a.qoi_partial, l.grid_x, a.B, a.qoi_op, 1.0 / ((double)a.Mx * a.Mt), a.d_qoi, a.d_acc, a.st);
  return rc;
}

}  // namespace mlmcpi
