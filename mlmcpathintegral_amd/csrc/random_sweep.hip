// random_sweep.hip -- OverrelaxedHeatBathSampler::draw with random_order = true (sampler/overrelaxedheatbathsampler.cc:8-31:
// the index set is shuffled before every sweep, then one local update per index) for the 2-D actions, parallel within a chain
// and still EXACTLY the sequential sweep in that order.
//
// ORDER (P_SWEEP_ORDER, device_common.hpp).  Index l of a chain (Schwinger: the 2 Mt Mx links; GFF, sigma model:
// the Mt Mx vertices) takes word l & 3 of Philox (site l >> 2, chain, step of the sweep, purpose 18, sub 0) as its 32-bit key;
// the sweep visits the indices in ascending (key, l).  Every chain and every sweep has its own order.
//
// SCHEDULE.  Two updates conflict when one reads what the other writes: a link and the six links of its two staples, a
// vertex and its four neighbours (a symmetric relation).  Round of an index = 1 + the largest round among its conflict
// neighbours that precede it in the order (1 without any).  Two conflicting indices never share a round and every
// conflicting pair runs in the order's sequence, so running the rounds one after the other, each in parallel, gives what
// the sequential walk gives -- to the last bit, because the updates are the site-at-a-time kernels' own device functions.
//
// KERNEL.  One workgroup per chain; all sweeps of a draw in one launch.  Per sweep: keys (one Philox call per four
// indices); for every index the bit mask of its conflict neighbours that precede it; round numbers by the ready rule in
// integers (iteration k gives round k to the indices all of whose preceding neighbours have a smaller round: one barrier
// per iteration, byte reads only); a counting sort by round into a dense list that overlays the keys; then one barrier per
// round with the updates of that round on full lanes.  A pass schedules at most `chunk` (<= 254: the rounds are bytes)
// rounds of the indices not yet updated, runs them, and the next pass goes on from there: no cap on the number of rounds.
// HOME.  Lattices whose state, keys and two bytes per index fit the CU's LDS live there from the first load to the last
// store of the launch; beyond, the SAME body runs on the state in global memory with keys and bytes in the caller's
// workspace, and every barrier comes with a workgroup-scope fence.
#include <hipcub/hipcub.hpp>

#include "internal.hpp"
#include "site_update.hpp"
#include "step_envelope.hpp"

#include "sigma_device.hpp"  // fp contraction is off from here on (this file adds no floating-point arithmetic of its own)

namespace mlmcpi {

namespace {

enum RsAction : int { RS_GFF = 0, RS_SCHW = 1, RS_SIGMA = 2 };

constexpr uint32_t kRsHist = 256;                        // rounds of a pass are bytes: 1 .. 254 (0 pending, 255 updated)
constexpr uint32_t kRsDone = 255;
constexpr uint32_t kRsChunkMax = 254;
constexpr uint32_t kRsLdsMax = 160 * 1024 - 6 * 1024;    // dynamic LDS of a workgroup; static: three 1 KB tables + the sampler's

__host__ __device__ inline uint32_t rs_state_doubles(int act, uint32_t n) { return act == RS_SIGMA ? 2 * n : n; }
// keys (4 B, later the list), round byte, mask byte per index; multiples of 256 B per chain
__host__ __device__ inline size_t rs_work_stride(uint32_t n) { return ((size_t)6 * n + 255) / 256 * 256; }

// the conflict neighbours of index l, in a fixed order (bit c of the mask = neighbour c)
template <int ACT>
__device__ __forceinline__ void rs_neighbours(uint32_t Mt, uint32_t Mx, uint32_t l, uint32_t (&nb)[6]) {
  const uint32_t v = ACT == RS_SCHW ? l >> 1 : l, j = v / Mt, i = v - j * Mt;
  const uint32_t ip = i + 1 == Mt ? 0 : i + 1, im = i == 0 ? Mt - 1 : i - 1, jp = j + 1 == Mx ? 0 : j + 1, jm = j == 0 ? Mx - 1 : j - 1;
  if (ACT == RS_SCHW) {
    auto link = [&](uint32_t a, uint32_t c, uint32_t mu) { return 2 * (Mt * c + a) + mu; };
    if ((l & 1u) == 0) {  // the links schwinger_site_update reads for mu = 0 ...
      nb[0] = link(i, jp, 0); nb[1] = link(i, j, 1); nb[2] = link(ip, j, 1);
      nb[3] = link(i, jm, 0); nb[4] = link(ip, jm, 1); nb[5] = link(i, jm, 1);
    } else {              // ... and for mu = 1
      nb[0] = link(i, j, 0); nb[1] = link(ip, j, 1); nb[2] = link(i, jp, 0);
      nb[3] = link(im, jp, 0); nb[4] = link(im, j, 1); nb[5] = link(im, j, 0);
    }
  } else {
    nb[0] = Mt * j + ip; nb[1] = Mt * j + im; nb[2] = Mt * jp + i; nb[3] = Mt * jm + i;
    nb[4] = nb[5] = 0;
  }
}

template <bool LDS_HOME>
__device__ __forceinline__ void rs_barrier() {
  if (!LDS_HOME) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the other waves read what this one stored in global memory
  __syncthreads();
}

// state [B][ns] doubles; work: rs_work_stride(n) bytes per chain (global home; unused in the LDS home).  out_sortkey /
// out_round (either may be NULL): schedule only -- (key << 32 | l) and the round of every index of sweep key0.step, no updates.
template <int ACT, bool LDS_HOME, int NT>
__global__ void __launch_bounds__(NT)
    random_sweep_kernel(uint32_t Mt, uint32_t Mx, double coupling, double *state, uint32_t n_overrelax, uint32_t n_sweeps, RngKey key0,
                        const uint32_t *__restrict__ vs_table, uint8_t *work, uint32_t chunk, bool schedule_only,
                        uint64_t *__restrict__ out_sortkey, uint32_t *__restrict__ out_round) {
  extern __shared__ double rs_lds[];
  __shared__ uint32_t hist[kRsHist], start[kRsHist], cursor[kRsHist];
  __shared__ uint32_t vs_lds[kVsTableBytes / 4];
  constexpr uint32_t NC = ACT == RS_SCHW ? 6 : 4;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint32_t n = (ACT == RS_SCHW ? 2u : 1u) * Mt * Mx, ns = rs_state_doubles(ACT, n);
  double *const gst = state + (size_t)b * ns;
  double *st;
  uint32_t *keys;  // the keys of a sweep, then the list of a pass
  uint8_t *rb, *mask;
  if (LDS_HOME) {
    st = rs_lds;
    keys = (uint32_t *)(rs_lds + ns);
  } else {
    st = gst;
    keys = (uint32_t *)(work + (size_t)b * rs_work_stride(n));
  }
  rb = (uint8_t *)(keys + n);
  mask = rb + n;
  RngKey key = key0;
  key.chain += b;
  const VsTable tab = VsTable::stage(vs_lds, ACT == RS_SCHW ? vs_table : nullptr);
  const bool step = 2. * coupling <= kVsKappaMax;
  const double inv_kappa = 1. / (4. + coupling), two_over_kappa = 2. / (4. + coupling), sigma = 1. / sqrt(4. + coupling);
  if (LDS_HOME && !schedule_only)
    for (uint32_t e = tid; e < ns; e += NT) st[e] = gst[e];
  for (uint32_t h = tid; h < kRsHist; h += NT) hist[h] = 0;

  for (uint32_t s = 0; s < n_sweeps; ++s) {
    key.step = key0.step + s;
    const bool heat = s >= n_overrelax;
    for (uint32_t q = tid; q < (n + 3) / 4; q += NT) {
      const U4 r = philox4x32_10(q, key.chain, key.step, (uint32_t)P_SWEEP_ORDER << 24, key.k0, key.k1);
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c)
        if (4 * q + c < n) keys[4 * q + c] = w[c];
    }
    rs_barrier<LDS_HOME>();
    for (uint32_t l = tid; l < n; l += NT) {
      uint32_t nb[6];
      rs_neighbours<ACT>(Mt, Mx, l, nb);
      const uint32_t kl = keys[l];
      uint32_t m = 0;
#pragma unroll
      for (uint32_t c = 0; c < NC; ++c) {
        const uint32_t km = keys[nb[c]];
        if (km < kl || (km == kl && nb[c] < l)) m |= 1u << c;
      }
      mask[l] = (uint8_t)m;
      rb[l] = 0;
      if (out_sortkey) out_sortkey[(size_t)b * n + l] = ((uint64_t)kl << 32) | l;
    }
    rs_barrier<LDS_HOME>();

    uint32_t done = 0, base = 0;
    while (done < n) {  // a pass: schedule up to `chunk` rounds of the indices not yet updated, then run them
      uint32_t K = 0, assigned = done;
      while (K < chunk && assigned < n) {
        ++K;
        uint32_t mine = 0;
        for (uint32_t l = tid; l < n; l += NT) {
          if (rb[l] != 0) continue;
          const uint32_t m = mask[l];
          bool ready = true;
          if (m) {
            uint32_t nb[6];
            rs_neighbours<ACT>(Mt, Mx, l, nb);
#pragma unroll
            for (uint32_t c = 0; c < NC; ++c)
              if ((m >> c) & 1u) {
                const uint32_t r = rb[nb[c]];  // a byte another lane may be writing K into right now: 0 or K, not ready either way
                if (r == 0 || (r >= K && r != kRsDone)) ready = false;
              }
          }
          if (ready) {
            rb[l] = (uint8_t)K;
            ++mine;
          }
        }
        if (mine) atomicAdd(&hist[K], mine);
        rs_barrier<LDS_HOME>();
        assigned += hist[K];  // written in iteration K only
      }
      if (tid == 0) {
        uint32_t a = 0;
        for (uint32_t r = 1; r <= K; ++r) {
          start[r] = cursor[r] = a;
          a += hist[r];
        }
        start[K + 1] = a;
      }
      __syncthreads();
      for (uint32_t l = tid; l < n; l += NT) {  // counting sort by round; the order within a round does not matter
        const uint32_t r = rb[l];
        if (r == 0 || r == kRsDone) continue;
        keys[atomicAdd(&cursor[r], 1u)] = l;
        if (out_round) out_round[(size_t)b * n + l] = base + r;
      }
      rs_barrier<LDS_HOME>();
      if (!schedule_only)
        for (uint32_t r = 1; r <= K; ++r) {
          for (uint32_t t = start[r] + tid; t < start[r + 1]; t += NT) {
            const uint32_t l = keys[t];
            if (ACT == RS_SCHW) schwinger_site_update(st, Mt, Mx, l, heat, step, coupling, key, tab);
            else if (ACT == RS_GFF) gff_site_update(st, Mt, Mx, l, heat, inv_kappa, two_over_kappa, sigma, key);
            else sigma_site_update((double2 *)st, Mt, Mx, l, heat, coupling, key);
          }
          rs_barrier<LDS_HOME>();
        }
      for (uint32_t t = tid; t < start[K + 1]; t += NT) rb[keys[t]] = (uint8_t)kRsDone;
      for (uint32_t h = tid; h < kRsHist; h += NT) hist[h] = 0;
      done = assigned;
      base += K;
      rs_barrier<LDS_HOME>();
    }
  }
  if (LDS_HOME && !schedule_only)
    for (uint32_t e = tid; e < ns; e += NT) gst[e] = st[e];
}

__global__ void __launch_bounds__(256) rs_order_kernel(const uint64_t *__restrict__ sorted, uint32_t *__restrict__ order, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < total) order[t] = (uint32_t)sorted[t];
}

DeviceOnce g_rs_attr_once;

int rs_init_attrs() {
  return once_per_device(g_rs_attr_once, []() -> int {
#define RS_ATTR(ACT, NT) \
  MLMCPI_HIP_TRY(hipFuncSetAttribute((const void *)random_sweep_kernel<ACT, true, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, kRsLdsMax))
    RS_ATTR(RS_GFF, 256); RS_ATTR(RS_GFF, 1024);
    RS_ATTR(RS_SCHW, 256); RS_ATTR(RS_SCHW, 1024);
    RS_ATTR(RS_SIGMA, 256);  // the sigma model's update needs ~170 VGPRs: 256 threads (1024 would spill to scratch)
#undef RS_ATTR
    return MLMCPI_OK;
  });
}

// kind and extents; *act_out = the kernel's action, *n = the size of the index set
int rs_check(const mlmcpi_lattice_action *act, int *act_out, uint32_t *n) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind != MLMCPI_GFF && act->kind != MLMCPI_SCHWINGER && act->kind != MLMCPI_NONLINEAR_SIGMA)
    return fail(MLMCPI_ERR_UNSUPPORTED, "the parallel random-order sweep is built for the 2-D actions (GFF, Schwinger, sigma model), not kind %d",
                act->kind);
  if (int rc = check_lattice(act)) return rc;  // extents, as every other entry point
  *act_out = act->kind == MLMCPI_GFF ? RS_GFF : act->kind == MLMCPI_SCHWINGER ? RS_SCHW : RS_SIGMA;
  *n = (act->kind == MLMCPI_SCHWINGER ? 2u : 1u) * act->Mt * act->Mx;
  return MLMCPI_OK;
}

template <int ACT>
int rs_launch(const mlmcpi_lattice_action *act, uint32_t n, double *d_state, uint32_t B, uint32_t n_overrelax, uint32_t n_sweeps, RngKey key,
              const uint32_t *vs_table, void *d_work, bool schedule_only, uint64_t *out_sortkey, uint32_t *out_round, hipStream_t st) {
  const Tuning tune = tuning();
  const uint32_t chunk = tune.random_sweep_chunk ? tune.random_sweep_chunk : kRsChunkMax;
  const size_t lds = (size_t)8 * rs_state_doubles(ACT, n) + (size_t)6 * n;
  const double coupling = ACT == RS_GFF ? gff_mu2(*act) : act->beta;
#define RS_GO(HOME, NT, BYTES)                                                                                                        \
  hipLaunchKernelGGL((random_sweep_kernel<ACT, HOME, NT>), dim3(B), dim3(NT), BYTES, st, act->Mt, act->Mx, coupling, d_state, n_overrelax, \
                     n_sweeps, key, vs_table, (uint8_t *)d_work, chunk, schedule_only, out_sortkey, out_round)
  constexpr int BIG = ACT == RS_SIGMA ? 256 : 1024;  // workgroup size that keeps the update out of scratch
  if (!tune.random_sweep_global && lds <= kRsLdsMax) {
    if (n >= 2048) RS_GO(true, BIG, lds);
    else RS_GO(true, 256, lds);
  } else {
    RS_GO(false, BIG, 0);
  }
#undef RS_GO
  MLMCPI_LAUNCH_CHECK("random_sweep_kernel");
  return MLMCPI_OK;
}

int rs_dispatch(int a, const mlmcpi_lattice_action *act, uint32_t n, double *d_state, uint32_t B, uint32_t n_overrelax, uint32_t n_sweeps,
                RngKey key, void *d_work, bool schedule_only, uint64_t *out_sortkey, uint32_t *out_round, hipStream_t st) {
  if (int rc = rs_init_attrs()) return rc;
  const uint32_t *vs_table = nullptr;
  if (a == RS_SCHW && !schedule_only && n_sweeps > n_overrelax && 2. * act->beta <= kVsKappaMax)
    if (int rc = vs_table_device(2. * act->beta, &vs_table)) return rc;
  if (a == RS_SCHW) return rs_launch<RS_SCHW>(act, n, d_state, B, n_overrelax, n_sweeps, key, vs_table, d_work, schedule_only, out_sortkey, out_round, st);
  if (a == RS_GFF) return rs_launch<RS_GFF>(act, n, d_state, B, n_overrelax, n_sweeps, key, vs_table, d_work, schedule_only, out_sortkey, out_round, st);
  return rs_launch<RS_SIGMA>(act, n, d_state, B, n_overrelax, n_sweeps, key, vs_table, d_work, schedule_only, out_sortkey, out_round, st);
}

}  // namespace
}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_lattice_random_sweep_workspace_bytes(const mlmcpi_lattice_action *act, uint32_t B, size_t *bytes) {
  int a = 0;
  uint32_t n = 0;
  if (int rc = rs_check(act, &a, &n)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  *bytes = (size_t)B * rs_work_stride(n);
  return MLMCPI_OK;
}

int mlmcpi_lattice_random_sweep_draw(const mlmcpi_lattice_action *act, double *d_state, uint32_t B, uint32_t n_overrelax, uint32_t n_heatbath,
                                     uint64_t seed, uint32_t chain0, uint32_t sweep0, void *d_work, void *stream) {
  int a = 0;
  uint32_t n = 0;
  if (int rc = rs_check(act, &a, &n)) return rc;
  MLMCPI_REQUIRE(d_state && d_work && B > 0, "bad arguments");
  MLMCPI_REQUIRE((uint64_t)n_overrelax + n_heatbath <= 0xFFFFFFFFull - sweep0, "sweep0 + n_overrelax + n_heatbath must fit 32 bits");
  if (n_overrelax + n_heatbath == 0) return MLMCPI_OK;
  return rs_dispatch(a, act, n, d_state, B, n_overrelax, n_overrelax + n_heatbath, make_key(seed, chain0, sweep0), d_work, false, nullptr,
                     nullptr, as_stream(stream));
}

int mlmcpi_lattice_random_sweep_order(const mlmcpi_lattice_action *act, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t sweep,
                                      uint32_t *d_order, uint32_t *d_round, void *stream) {
  int a = 0;
  uint32_t n = 0;
  if (int rc = rs_check(act, &a, &n)) return rc;
  MLMCPI_REQUIRE(d_order && B > 0, "bad arguments");
  hipStream_t st = as_stream(stream);
  const size_t total = (size_t)B * n, work = (size_t)B * rs_work_stride(n);
  size_t cub = 0;
  MLMCPI_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, cub, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, 64, st));
  cub = (cub + 255) / 256 * 256;
  void *buf = nullptr;
  if (int rc = scratch(16 * total + work + cub, &buf, st)) return rc;
  uint64_t *sortkey = (uint64_t *)buf, *sorted = sortkey + total;
  uint8_t *d_work = (uint8_t *)(sorted + total), *d_cub = d_work + work;
  if (int rc = rs_dispatch(a, act, n, nullptr, B, 0, 1, make_key(seed, chain0, sweep), d_work, true, sortkey, d_round, st)) return rc;
  for (uint32_t b = 0; b < B; ++b)
    MLMCPI_HIP_TRY(hipcub::DeviceRadixSort::SortKeys(d_cub, cub, sortkey + (size_t)b * n, sorted + (size_t)b * n, (int)n, 0, 64, st));
  hipLaunchKernelGGL(rs_order_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, sorted, d_order, total);
  MLMCPI_LAUNCH_CHECK("rs_order_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
