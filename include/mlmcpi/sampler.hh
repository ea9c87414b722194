// sampler.hh -- MCMCStep (montecarlo/mcmcstep.hh:21-72), Sampler / SamplerFactory
// (sampler/sampler.hh:20-43), HMCSampler (sampler/hmcsampler.{hh,cc}) and
// OverrelaxedHeatBathSampler (sampler/overrelaxedheatbathsampler.{hh,cc}) driving device chains.
#ifndef MLMCPI_SAMPLER_HH
#define MLMCPI_SAMPLER_HH
#include <chrono>
#include <cmath>
#include <iomanip>
#include <iostream>
#include <algorithm>
#include <memory>
#include <random>
#include <typeinfo>
#include <vector>

#include "action.hh"
#include "correlator.hh"

namespace mlmcpi {

class MCMCStep {
public:
  MCMCStep() : accept(false), copy_if_rejected(false) { reset_stats(); }
  virtual ~MCMCStep() {}
  void reset_stats() { n_total_samples = 0; n_accepted_samples = 0; }
  /** acceptance probability; with a batch, averaged over its chains */
  double p_accept() { return n_accepted_samples / (1. * n_total_samples); }
  virtual void show_stats() {
    std::cout << std::setprecision(5) << std::fixed;
    std::cout << "  acceptance probability  p = " << p_accept() << std::endl;
    std::cout << "  rejection probability 1-p = " << 1. - p_accept() << std::endl;
  }
  bool accepted() const { return accept; }
  virtual void set_state(std::shared_ptr<SampleState> x_state) = 0;
  virtual double cost_per_sample() { fatal(std::string(" Cost per sample not defined for class ") + typeid(*this).name()); }

protected:
  mutable double n_accepted_samples;  // fractional for batches: mean over chains per draw
  mutable unsigned int n_total_samples;
  mutable bool accept;
  mutable bool copy_if_rejected;
};

class Sampler : public MCMCStep {
public:
  Sampler() : MCMCStep() {}
  virtual ~Sampler() {}
  /** sampler/sampler.hh:36 */
  virtual void draw(std::shared_ptr<SampleState> phi_state) = 0;
};

class SamplerFactory {
public:
  virtual ~SamplerFactory() {}
  virtual std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) = 0;
};

/** sampler/hmcsampler.hh:21-65 */
struct HMCParameters {
  unsigned int nt = 100;
  double dt = 0.1;
  unsigned int n_burnin = 100;
  unsigned int n_rep = 1;
  bool autotune = true;             // the reference always tunes (hmcsampler.hh:107)
  unsigned int batch = 1;           // independent chains advanced together
  unsigned int tune_iterations = 100, tune_samples = 1000;  // hmcsampler.cc:78,89
};

/** HMC on device chains.  One draw = n_rep fused trajectories (mlmcpi_path_hmc_draw for 1-D
 *  actions, mlmcpi_lattice_hmc_draw for 2-D ones).  Construction follows hmcsampler.hh:84-109:
 *  initialise_state, n_burnin draws, step-size auto-tuning, reset of the counters. */
class HMCSampler : public Sampler {
public:
  HMCSampler(const std::shared_ptr<Action> action_, const HMCParameters hmc_param_)
      : Sampler(), action(action_), nt_hmc(hmc_param_.nt), dt_hmc(hmc_param_.dt), n_rep(hmc_param_.n_rep),
        n_burnin(hmc_param_.n_burnin), B(hmc_param_.batch), accept_flags(hmc_param_.batch, sizeof(int32_t)),
        energies(4 * (size_t)hmc_param_.batch) {
    qm = dynamic_cast<QMAction *>(action.get());
    qft = dynamic_cast<QFTAction *>(action.get());
    if (!qm && !qft) fatal("HMCSampler: action has no device implementation");
    size_t bytes = 0;
    if (qm) check(mlmcpi_path_hmc_workspace_bytes(&qm->abi_action(), B, nt_hmc, &bytes), "hmc_workspace_bytes");
    else check(mlmcpi_lattice_hmc_workspace_bytes(&qft->abi_action(), B, &bytes), "hmc_workspace_bytes");
    check(mlmcpi_malloc(&work, bytes), "mlmcpi_malloc");
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < n_burnin; ++i) draw(tmp);
    if (hmc_param_.autotune) autotune_stepsize(0.8, hmc_param_.tune_iterations, hmc_param_.tune_samples);
    reset_stats();
  }
  virtual ~HMCSampler() { mlmcpi_free(work); }

  /** hmcsampler.cc:8-19.  With a batch, `accepted()` reports chain 0 and rejected chains keep their
   *  previous content in phi_state (copy_if_rejected == false), like the reference. */
  void draw(std::shared_ptr<SampleState> phi_state) override {
    const double mean_acc = step();
    n_total_samples++;
    n_accepted_samples += mean_acc;
    // hmcsampler.cc:16-18: copy out only if accepted.  For a batch the whole current state is copied:
    // a rejected chain's current state equals what the caller received at its last acceptance.
    if (copy_if_rejected || accept || B > 1) phi_state->data = phi_state_cur->data;
  }
  void set_state(std::shared_ptr<SampleState> phi_state) override { phi_state_cur->data = phi_state->data; }
  double get_dt() const { return dt_hmc; }
  /** the Philox trajectory counter: the `traj0` of the next launch (burn-in and tuning have advanced it) */
  uint32_t trajectories_used() const { return traj; }
  std::shared_ptr<SampleState> current_state() { return phi_state_cur; }

  /** hmcsampler.cc:77-113: bisection on [dt/2, 2dt], fixed iteration count, result kept only if some
   *  iterate came within 0.01 of the target.  Each iterate averages ~tune_samples trajectories. */
  void autotune_stepsize(const double p_accept_target, unsigned iterations = 100, unsigned n_autotune_samples = 1000) {
    const double tolerance = 1.E-2, dt_original = dt_hmc;
    double dt_min = 0.5 * dt_hmc, dt_max = 2. * dt_hmc;
    bool converged = false;
    std::cout << std::setprecision(4) << std::fixed;
    std::cout << " Auto-tuning HMC step size to achieve acceptance rate of " << p_accept_target << " ..." << std::endl;
    std::cout << "  Starting with dt_{HMC} = " << dt_hmc << std::endl;
    const unsigned draws = (n_autotune_samples + B - 1) / B;
    for (unsigned int k = 0; k < iterations; ++k) {
      reset_stats();
      dt_hmc = 0.5 * (dt_min + dt_max);
      for (unsigned int j = 0; j < draws; ++j) {
        n_accepted_samples += single_step();
        n_total_samples++;
      }
      if (p_accept() > p_accept_target) dt_min = dt_hmc; else dt_max = dt_hmc;
      if (std::fabs(p_accept() - p_accept_target) < tolerance) converged = true;
    }
    if (converged) {
      std::cout << "  Tuned         dt_{HMC} = " << dt_hmc << std::endl;
    } else {
      dt_hmc = dt_original;
      std::cout << "  FAILED to tune, reverting to " << dt_hmc << std::endl;
    }
    std::cout << std::endl;
    reset_stats();
  }

private:
  double launch(unsigned reps) {
    double *x = phi_state_cur->device_mutable();
    if (qm)
      check(mlmcpi_path_hmc_draw(&qm->abi_action(), x, B, nt_hmc, dt_hmc, reps, action->get_seed(), action->get_chain0(),
                                 traj, work, (int32_t *)accept_flags.ptr(), (double *)energies.ptr(), nullptr), "path_hmc_draw");
    else
      check(mlmcpi_lattice_hmc_draw(&qft->abi_action(), x, B, nt_hmc, dt_hmc, reps, action->get_seed(),
                                    action->get_chain0(), traj, work, (int32_t *)accept_flags.ptr(),
                                    (double *)energies.ptr(), nullptr), "lattice_hmc_draw");
    traj += reps;
    std::vector<int32_t> flags = accept_flags.download<int32_t>();
    double acc = 0;
    for (int32_t f : flags) acc += f;
    accept = flags[0] != 0;
    return acc / B;
  }
  double step() { return launch(n_rep); }      // one draw
  double single_step() { return launch(1); }   // hmcsampler.cc:22-69

protected:
  const std::shared_ptr<Action> action;
  const unsigned int nt_hmc;
  mutable double dt_hmc;
  const unsigned int n_rep, n_burnin, B;
  mutable std::shared_ptr<SampleState> phi_state_cur;
  QMAction *qm = nullptr;
  QFTAction *qft = nullptr;
  void *work = nullptr;
  DeviceVector accept_flags, energies;
  uint32_t traj = 0;
};

/** sampler/overrelaxedheatbathsampler.hh:22-71 */
struct OverrelaxedHeatBathParameters {
  unsigned int n_sweep_heatbath = 1;
  unsigned int n_sweep_overrelax = 10;
  unsigned int n_burnin = 100;
  // overrelaxedheatbathsampler.hh:60-63.  false (the default here; the reference's template says true): the fixed sweep
  // order -- on the device the multicolour order instead of the reference's lexicographic one (a different, equally
  // valid fixed order; said once on stderr).  true: the reference's own loop, every sweep over a freshly shuffled index
  // set, through the site-at-a-time updates (sequential within a chain, chains in parallel): exact semantics, slow.
  bool random_order = false;
  // with random_order = true: 0 = the host shuffle (std::mt19937_64) and the site-at-a-time loop, as above; 1 = the device
  // order (Philox purpose 18: every chain and sweep its own order) run in parallel rounds, one launch per draw, exactly the
  // sequential sweep in that order (mlmcpi_lattice_random_sweep_draw; 2-D actions)
  unsigned int random_order_mode = 0;
  unsigned int batch = 1;
};

/** overrelaxedheatbathsampler.cc:8-37: n_sweep_overrelax overrelaxation sweeps, then
 *  n_sweep_heatbath heat-bath sweeps, every sample accepted.
 *
 *  No copy per draw.  The reference ends draw() with `phi_state->data = phi_state_cur->data` (:30); here the caller's
 *  state becomes a second holder of the buffer the new sample was written to (SampleState::share), and the sampler
 *  rotates a small pool of buffers: a draw reads the current sample (which the caller may still hold: it is not written)
 *  and lets the launches alternate between two buffers nobody else holds.  In the loop of
 *  MonteCarloSingleLevel::evaluate that settles at three buffers and zero copies. */
class OverrelaxedHeatBathSampler : public Sampler {
public:
  OverrelaxedHeatBathSampler(const std::shared_ptr<Action> action_, const OverrelaxedHeatBathParameters p)
      : Sampler(), action(action_), n_sweep_heatbath(p.n_sweep_heatbath), n_sweep_overrelax(p.n_sweep_overrelax),
        n_burnin(p.n_burnin), random_order(p.random_order), random_order_mode(p.random_order_mode) {
    if (!action->has_local_updates()) fatal("heat bath update not implemented for this action ");
    if (random_order_mode > 1) fatal("random_order_mode must be 0 (host shuffle) or 1 (device order)");
    if (random_order && random_order_mode == 1) {
      // no index set on the host: the order is a function of (seed, chain, sweep)
    } else if (random_order) {  // overrelaxedheatbathsampler.hh:110-116: the action's index set, or every entry
      index_map = action->get_heatbath_indexset();
      if (index_map.empty()) {
        index_map.resize(action->sample_size());
        for (unsigned int l = 0; l < index_map.size(); ++l) index_map[l] = l;
      }
      d_index = std::make_shared<DeviceVector>((index_map.size() + 1) / 2);  // uint32 entries in 8-byte units
    } else {
      static bool said = false;
      if (!said) std::cerr << "NOTE: random_order = false: device sweeps run in multicolour order, not lexicographically" << std::endl;
      said = true;
    }
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), p.batch);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), p.batch);
    for (unsigned int i = 0; i < n_burnin; ++i) draw(tmp);
    reset_stats();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    advance();
    if (phi_state != phi_state_cur) phi_state->share(*phi_state_cur);
  }
  /** draw + QoI in one pass over the state: d_q[b] = the QoI (QoI::fused_kind()) of the new sample, summed inside the
   *  draw's last launch; d_acc != NULL: stats->record_sample(q) into the per-chain device moments d_acc[batch][5] as well
   *  (mlmcpi_stats_accumulate's layout), in the same call.  Returns false (and does nothing) when the action cannot fuse it. */
  bool draw_with_qoi(std::shared_ptr<SampleState> phi_state, int qoi_kind, double *d_q, double *d_acc = nullptr) {
    if (!advance(qoi_kind, d_q, d_acc)) return false;
    if (phi_state != phi_state_cur) phi_state->share(*phi_state_cur);
    return true;
  }
  /** the draw without handing the sample out (callers that read current_state()) */
  bool advance(int qoi_kind = 0, double *d_q = nullptr, double *d_acc = nullptr) {
    if (qoi_kind && (n_sweep_heatbath == 0 || random_order)) return false;
    if (random_order && random_order_mode == 1) {  // one launch per draw: no host shuffle, no copy to the device
      action->random_sweep_draw(phi_state_cur, n_sweep_overrelax, n_sweep_heatbath, sweep_counter);
    } else
    if (random_order) {  // overrelaxedheatbathsampler.cc:8-31 as written: shuffle, then one local update per index
      // (site_updates works in place; a sample handed out earlier keeps its values: SampleState::device_mutable detaches)
      for (unsigned int s = 0; s < n_sweep_overrelax + n_sweep_heatbath; ++s) {
        std::shuffle(index_map.begin(), index_map.end(), engine);
        check(mlmcpi_copy_h2d(d_index->ptr(), index_map.data(), index_map.size() * sizeof(uint32_t), nullptr), "copy_h2d");
        action->set_site_step(sweep_counter + s);
        action->site_updates(phi_state_cur, (const uint32_t *)d_index->ptr(), (unsigned int)index_map.size(), 0, s >= n_sweep_overrelax);
      }
    } else
    if (n_sweep_overrelax + n_sweep_heatbath > 0) {
      std::shared_ptr<DeviceBuffer> src = phi_state_cur->buffer();
      // `src` is held by phi_state_cur, by this local variable and by the pool if it came from there: one holder more
      // means somebody outside still reads the current sample
      long own = 2;
      for (auto &c : pool) own += (c == src) ? 1 : 0;
      const bool src_is_lent = src.use_count() > own;
      std::shared_ptr<DeviceBuffer> w0 = free_buffer(src, nullptr);
      std::shared_ptr<DeviceBuffer> w1 = src_is_lent ? free_buffer(src, w0) : src;
      const int where = qoi_kind ? action->sweep_from_qoi(src->p, w0->p, w1->p, phi_state_cur->batch(), n_sweep_overrelax,
                                                          n_sweep_heatbath, sweep_counter, qoi_kind, d_q, d_acc)
                                 : action->sweep_from(src->p, w0->p, w1->p, phi_state_cur->batch(), n_sweep_overrelax,
                                                      n_sweep_heatbath, sweep_counter);
      if (where < 0) return false;
      phi_state_cur->adopt(where == 0 ? w0 : w1);
    }
    sweep_counter += n_sweep_overrelax + n_sweep_heatbath;
    accept = true;
    n_total_samples++;
    n_accepted_samples++;
    return true;
  }
  void set_state(std::shared_ptr<SampleState> phi_state) override { phi_state_cur->data = phi_state->data; }
  std::shared_ptr<SampleState> current_state() { return phi_state_cur; }
  size_t pool_size() const { return pool.size(); }

protected:
  /** a pool buffer nobody else holds (other than `a`, `b`), allocated on first need */
  std::shared_ptr<DeviceBuffer> free_buffer(const std::shared_ptr<DeviceBuffer> &a, const std::shared_ptr<DeviceBuffer> &b) {
    for (auto &c : pool)
      if (c != a && c != b && c.use_count() == 1) return c;
    pool.push_back(std::make_shared<DeviceBuffer>(phi_state_cur->bytes()));
    return pool.back();
  }
  const std::shared_ptr<Action> action;
  const unsigned int n_sweep_heatbath, n_sweep_overrelax, n_burnin;
  bool random_order;
  unsigned int random_order_mode;
  std::vector<unsigned int> index_map;      // random_order: the index set, reshuffled per sweep
  std::shared_ptr<DeviceVector> d_index;    // ... and its device copy
  std::mt19937_64 engine{871417};           // overrelaxedheatbathsampler.hh:111
  mutable std::shared_ptr<SampleState> phi_state_cur;
  std::vector<std::shared_ptr<DeviceBuffer>> pool;  // buffers that have carried a sample (some may still be lent out)
  uint32_t sweep_counter = 0;
};

class HMCSamplerFactory : public SamplerFactory {
public:
  explicit HMCSamplerFactory(const HMCParameters p) : param(p) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override { return std::make_shared<HMCSampler>(action, param); }
private:
  const HMCParameters param;
};

class OverrelaxedHeatBathSamplerFactory : public SamplerFactory {
public:
  explicit OverrelaxedHeatBathSamplerFactory(const OverrelaxedHeatBathParameters p) : param(p) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override {
    return std::make_shared<OverrelaxedHeatBathSampler>(action, param);
  }
private:
  const OverrelaxedHeatBathParameters param;
};

/** The exact sampler of the harmonic oscillator.  In the reference HarmonicOscillatorAction is itself a Sampler
 *  (harmonicoscillatoraction.hh:83, draw at harmonicoscillatoraction.cc:59-66, Cholesky factor at :38-56) and the
 *  drivers select it with sampler = 'exact'.  Here the factor is built once on the host and every draw is one fp64
 *  matrix-core product for the whole batch of chains (mlmcpi_path_exact_draw). */
class HarmonicOscillatorExactSampler : public Sampler {
public:
  HarmonicOscillatorExactSampler(const std::shared_ptr<Action> action_, unsigned int batch = 1)
      : Sampler(), action(std::dynamic_pointer_cast<HarmonicOscillatorAction>(action_)), B(batch) {
    if (!action) fatal("exact sampler only for the harmonic oscillator action");
    const size_t M = action->sample_size();
    std::vector<double> LT(M * M);
    check(mlmcpi_ho_cholesky_factor(&action->abi_action(), LT.data()), "ho_cholesky_factor");
    factor = std::make_shared<DeviceVector>(M * M);
    check(mlmcpi_copy_h2d(factor->ptr(), LT.data(), M * M * sizeof(double), nullptr), "copy_h2d");
    state = std::make_shared<SampleState>(M, B);
  }
  void draw(std::shared_ptr<SampleState> x_path) override {
    check(mlmcpi_path_exact_draw(&action->abi_action(), (const double *)factor->ptr(), state->device_mutable(), B,
                                 action->get_seed() ^ 0x45584143ull, action->get_chain0(), step++, nullptr), "path_exact_draw");
    accept = true;
    n_total_samples++;
    n_accepted_samples++;
    x_path->data = state->data;
  }
  void set_state(std::shared_ptr<SampleState>) override {}  // independent draws: there is no chain state

private:
  const std::shared_ptr<HarmonicOscillatorAction> action;
  const unsigned int B;
  std::shared_ptr<DeviceVector> factor;
  std::shared_ptr<SampleState> state;
  uint32_t step = 0;
};

/** The exact sampler of the Gaussian free field (GFFAction is a Sampler in the reference, gffaction.hh:120,
 *  draw at gffaction.cc:200-213): spectral synthesis on the device, mlmcpi_lattice_exact_draw. */
class GFFExactSampler : public Sampler {
public:
  GFFExactSampler(const std::shared_ptr<Action> action_, unsigned int batch = 1)
      : Sampler(), action(std::dynamic_pointer_cast<GFFAction>(action_)), B(batch) {
    if (!action) fatal("exact sampler only for the GFF action");
    if (action->plain()) {
      size_t bytes = 0;
      check(mlmcpi_lattice_exact_workspace_bytes(&action->abi_action(), B, &bytes), "lattice_exact_workspace_bytes");
      check(mlmcpi_malloc(&work, bytes), "mlmcpi_malloc");
    }
    state = std::make_shared<SampleState>(action->sample_size(), B);
  }
  ~GFFExactSampler() { mlmcpi_free(work); }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    if (action->plain())  // the finest level: spectral synthesis at any size
      check(mlmcpi_lattice_exact_draw(&action->abi_action(), state->device_mutable(), B, action->get_seed() ^ 0x45584143ull,
                                      action->get_chain0(), step++, work, nullptr), "lattice_exact_draw");
    else  // a level of the hierarchy (rotated and / or Gibbs smoothed): GFFAction::draw, gffaction.cc:200-213
      action->draw_level(state, step++);
    accept = true;
    n_total_samples++;
    n_accepted_samples++;
    phi_state->data = state->data;
  }
  void set_state(std::shared_ptr<SampleState>) override {}

private:
  const std::shared_ptr<GFFAction> action;
  const unsigned int B;
  void *work = nullptr;
  std::shared_ptr<SampleState> state;
  uint32_t step = 0;
};

/** sampler = 'exact' (driver_qm.cc / driver_qft.cc): the harmonic oscillator and the GFF are their own samplers
 *  (driver_qft.cc:84-85: GFFSamplerFactory for every level of a GFF hierarchy) */
class ExactSamplerFactory : public SamplerFactory {
public:
  explicit ExactSamplerFactory(unsigned int batch_ = 1) : batch(batch_) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override {
    if (std::dynamic_pointer_cast<GFFAction>(action)) return std::make_shared<GFFExactSampler>(action, batch);
    return std::make_shared<HarmonicOscillatorExactSampler>(action, batch);
  }
private:
  const unsigned int batch;
};

/** sampler/clustersampler.hh:29 (section clusteralgorithm: of the parameter file) */
struct ClusterParameters {
  unsigned int n_burnin = 100;
  unsigned int n_updates = 10;
  unsigned int batch = 1;
  unsigned int n_meas = 20;  // draws timed for cost_per_sample (10 000 in the reference's constructor)
  bool improved = false;     // WolffClusterSampler: also the improved chi_m of the single cluster (SwendsenWangSampler always has its own)
  bool structure = false;    // both cluster samplers: also the cluster-improved structure factor and xi_2 (off: the plain entry point)
  bool correlator = false;   // both cluster samplers: also the cluster-improved time-slice correlator C(tau) (off: the plain entry point)
};

/** ClusterSampler on a 1-D lattice (sampler/clustersampler.{hh,cc}; single_cluster_update1d): the rotor.  One draw =
 *  n_updates reflection-cluster updates of every chain in one launch (mlmcpi_path_cluster_draw), then the copy out.
 *  Counters advance by n_updates per draw (clustersampler.cc:44-48); set_state is a no-op (clustersampler.hh:116). */
class ClusterSampler : public Sampler {
public:
  ClusterSampler(const std::shared_ptr<Action> action_, const ClusterParameters p)
      : Sampler(), action(std::dynamic_pointer_cast<RotorAction>(action_)), n_burnin(p.n_burnin), n_updates(p.n_updates),
        B(p.batch), sites(p.batch, sizeof(uint32_t)) {
    if (!action) fatal(" cluster not supported for chosen action.");
    fold_period = std::max<uint64_t>(1, std::min<uint64_t>(1024, (1ull << 31) / ((uint64_t)std::max(1u, n_updates) * action->sample_size())));
    x_path_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(x_path_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < n_burnin; ++i) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int k = 0; k < p.n_meas; ++k) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    cost_per_sample_ = 1.E6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (p.n_meas ? p.n_meas : 1);
    reset_stats();
    fold_sites();
    flipped_total = 0.0;
  }
  void draw(std::shared_ptr<SampleState> x_path) override {
    if (update_counter > 0xFFFFFFFFu - n_updates) fatal("ClusterSampler: the 32-bit update counter of the Philox contract is used up.");
    check(mlmcpi_path_cluster_draw(&action->abi_action(), x_path_cur->device_mutable(), B, n_updates, action->get_seed(),
                                   action->get_chain0(), update_counter, (uint32_t *)sites.ptr(), nullptr), "path_cluster_draw");
    update_counter += n_updates;
    if (++draws_unfolded >= fold_period) fold_sites();
    n_total_samples += n_updates;
    n_accepted_samples += n_updates;
    x_path->data = x_path_cur->data;
    accept = true;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }
  /** flipped sites per update, averaged over chains and over the updates since construction */
  double mean_cluster_size() {
    if (!n_total_samples) return 0.0;
    fold_sites();
    return flipped_total / B / n_total_samples;
  }
  void show_stats() override {
    std::cout << std::setprecision(3) << std::fixed << "  cluster updates per draw = " << n_updates << std::endl
              << "  mean cluster size        = " << mean_cluster_size() << " sites" << std::endl;
  }
  /** the host total of flipped sites (folds so far) and the device counters not yet folded into it; read only */
  double flipped_sites_folded() const { return flipped_total; }
  std::vector<uint32_t> flipped_sites_unfolded() const { return sites.download<uint32_t>(); }

private:
  /** the device counters are 32 bits per chain: add them to the host total and zero them before they can wrap */
  void fold_sites() {
    for (uint32_t v : sites.download<uint32_t>()) flipped_total += v;
    check(mlmcpi_memset(sites.ptr(), 0, B * sizeof(uint32_t), nullptr), "mlmcpi_memset");
    draws_unfolded = 0;
  }
  const std::shared_ptr<RotorAction> action;
  const unsigned int n_burnin, n_updates, B;
  std::shared_ptr<SampleState> x_path_cur;
  DeviceVector sites;  // uint32 per chain: flipped sites since the last fold, added up on the device
  double flipped_total = 0.0;
  // an update flips at most M sites: fold before 2^31 could have been added to a chain's counter, at least every 1024 draws
  uint64_t fold_period = 1;
  uint64_t draws_unfolded = 0;
  uint32_t update_counter = 0;
  double cost_per_sample_ = 0.0;
};

/** sampler/quenchedschwingerclustersampler.{hh,cc}: the sampler's state is the plaquette path psi (a rotor with
 *  m0 / a = beta on Mt Mx sites); a draw advances it by n_updates cluster updates and overwrites the link field. */
class QuenchedSchwingerClusterSampler : public Sampler {
public:
  QuenchedSchwingerClusterSampler(const std::shared_ptr<Action> action_, const ClusterParameters p)
      : Sampler(), action(std::dynamic_pointer_cast<QuenchedSchwingerAction>(action_)), n_updates(p.n_updates), B(p.batch) {
    if (!action) fatal(" cluster not supported for chosen action.");
    const mlmcpi_lattice_action &abi = action->abi_action();
    size_t bytes = 0;
    check(mlmcpi_schwinger_cluster_workspace_bytes(&abi, B, &bytes), "schwinger_cluster_workspace_bytes");
    work = std::make_shared<DeviceBuffer>(bytes);
    check(mlmcpi_memset(work->p, 0, bytes, nullptr), "mlmcpi_memset");
    psi = std::make_shared<DeviceBuffer>((size_t)B * abi.Mt * abi.Mx * sizeof(double));
    check(mlmcpi_schwinger_cluster_init(&abi, psi->p, B, action->get_seed(), action->get_chain0(), nullptr), "schwinger_cluster_init");
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < p.n_burnin; ++i) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int k = 0; k < p.n_meas; ++k) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    cost_per_sample_ = 1.E6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (p.n_meas ? p.n_meas : 1);
    reset_stats();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    if (phi_state->batch() != B || phi_state->size() != action->sample_size()) fatal("cluster draw into a state of wrong shape.");
    check(mlmcpi_schwinger_cluster_draw(&action->abi_action(), psi->p, phi_state->device_overwrite(), B, n_updates,
                                        action->get_seed(), action->get_chain0(), draw_counter++, work->p, nullptr),
          "schwinger_cluster_draw");
    accept = true;
    n_total_samples++;
    n_accepted_samples++;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }

private:
  const std::shared_ptr<QuenchedSchwingerAction> action;
  const unsigned int n_updates, B;
  std::shared_ptr<DeviceBuffer> psi, work;  // work: the library's 32-bit flipped-site counters; this class never reads them (they may wrap)
  uint32_t draw_counter = 0;
  double cost_per_sample_ = 0.0;
};

/** driver_qm.cc:62-70, driver_qft.cc:69-80: the cluster sampler of the action at hand */
class ClusterSamplerFactory : public SamplerFactory {
public:
  explicit ClusterSamplerFactory(const ClusterParameters p) : param(p) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override {
    if (std::dynamic_pointer_cast<QuenchedSchwingerAction>(action)) return std::make_shared<QuenchedSchwingerClusterSampler>(action, param);
    if (std::dynamic_pointer_cast<NonlinearSigmaAction>(action))
      fatal(" cluster not supported for chosen action: the generic 2-D cluster update of the sigma model is not built (DESIGN.md 8).");
    return std::make_shared<ClusterSampler>(action, param);  // fatal unless the action is the rotor
  }
private:
  const ClusterParameters param;
};

/** What the cluster samplers of the sigma model keep of their improved estimators (WolffClusterSampler, SwendsenWangSampler):
 *  since the last reset(), the mean over draws of the per-draw improved chi_m (the mean over the draw's updates and the chains)
 *  with its standard error over the draws and, PER CHAIN, the sums over the updates of the improved chi_m, F_t, F_x (structure)
 *  and of the improved C_t and C_x, every lag (correlator).  structure_factor(d) and correlator() are means over the chains with
 *  their spread as the error, as SigmaCorrelator::means_and_errors; xi(d) is xi_2 from the chain-averaged (chi, F) with a
 *  jackknife over the chains, the arithmetic of SigmaCorrelator::xi (NaN where chi / F < 1). */
class ClusterImprovedSums {
public:
  struct Estimate {
    double value, error;
    bool has_error;  // the spread and the jackknife over chains need batch >= 2
  };
  struct CorrelatorEstimate {
    std::vector<double> mean, error;  // [n_out], C_t first: the layout of SigmaCorrelator::Estimate
    bool chain_spread;                // true: error = spread of the per-chain means (batch >= 2); false: no error (one chain)
  };
  ClusterImprovedSums(const char *owner_, unsigned int B_, unsigned int n_updates_, bool structure, bool correlator, unsigned int n_out_)
      : owner(owner_), B(B_), n_updates(n_updates_), with_structure(structure), with_correlator(correlator), n_out(n_out_),
        chain_C(correlator ? (size_t)B_ * n_out_ : 0, 0.0), chain_chi(B_, 0.0),
        chain_F{std::vector<double>(B_, 0.0), std::vector<double>(B_, 0.0)} {}
  void reset() {
    improved_sum = improved_sum2 = 0.0;
    draws_counted = 0;
    std::fill(chain_chi.begin(), chain_chi.end(), 0.0);
    for (std::vector<double> &f : chain_F) std::fill(f.begin(), f.end(), 0.0);
    std::fill(chain_C.begin(), chain_C.end(), 0.0);
  }
  /** one draw: imp [B], the draw's improved chi_m per chain summed over its updates; F [B][2] (may be NULL) and C [B][n_out] (may
   *  be NULL) likewise.  With structure and no F, F_d of the draw is structure_factor() of the draw's improved C_d, chain by chain. */
  void record(const mlmcpi_sigma_level &lv, const std::vector<double> &imp, const std::vector<double> *F, const std::vector<double> *C) {
    double v = 0.0;
    for (double x : imp) v += x;
    if (with_correlator && C)
      for (size_t k = 0; k < C->size(); ++k) chain_C[k] += (*C)[k];
    if (with_structure && F) {
      for (unsigned int b = 0; b < B; ++b) {
        chain_chi[b] += imp[b];
        chain_F[0][b] += (*F)[2 * b];
        chain_F[1][b] += (*F)[2 * b + 1];
      }
    } else if (with_structure && C) {
      const unsigned int nt = lv.Mt / 2 + 1;
      for (unsigned int b = 0; b < B; ++b) {
        const std::vector<double>::const_iterator c = C->begin() + (size_t)b * n_out;
        chain_chi[b] += imp[b];
        chain_F[0][b] += mlmcpi::structure_factor(std::vector<double>(c, c + nt), lv.Mt);
        chain_F[1][b] += mlmcpi::structure_factor(std::vector<double>(c + nt, c + n_out), lv.Mx);
      }
    }
    v /= (double)B * n_updates;                          // this draw's value: the mean over its updates and the chains
    improved_sum += v;
    improved_sum2 += v * v;
    ++draws_counted;
  }
  uint64_t draws() const { return draws_counted; }
  CorrelatorEstimate correlator() const {
    if (!with_correlator) fatal(owner + "::improved_correlator: constructed without ClusterParameters::correlator.");
    if (!draws_counted) fatal(owner + "::improved_correlator: no draws since reset_improved().");
    CorrelatorEstimate e{std::vector<double>(n_out, 0.0), std::vector<double>(n_out, 0.0), B >= 2};
    const double n = (double)draws_counted * n_updates;
    for (unsigned int k = 0; k < n_out; ++k) {
      double m = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) m += chain_C[(size_t)b * n_out + k] / n / B;
      for (unsigned int b = 0; b < B; ++b) s2 += (chain_C[(size_t)b * n_out + k] / n - m) * (chain_C[(size_t)b * n_out + k] / n - m);
      e.mean[k] = m;
      e.error[k] = B >= 2 ? std::sqrt(s2 / ((double)B * (B - 1.0))) : 0.0;
    }
    return e;
  }
  Estimate structure_factor(int d) const {
    need_structure("improved_structure_factor");
    const double n = (double)draws_counted * n_updates;
    double m = 0.0, s2 = 0.0;
    for (unsigned int b = 0; b < B; ++b) m += chain_F[d][b] / n / B;
    for (unsigned int b = 0; b < B; ++b) s2 += (chain_F[d][b] / n - m) * (chain_F[d][b] / n - m);
    return Estimate{m, B >= 2 ? std::sqrt(s2 / ((double)B * (B - 1.0))) : 0.0, B >= 2};
  }
  Estimate xi(int d, const mlmcpi_sigma_level &lv) const {
    need_structure("improved_xi");
    const unsigned int M = d == 0 ? lv.Mt : lv.Mx;
    double chi = 0.0, F = 0.0;
    for (unsigned int b = 0; b < B; ++b) {
      chi += chain_chi[b];
      F += chain_F[d][b];
    }
    Estimate r{xi_from_chi_and_F(chi / B, F / B, M), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        x[b] = xi_from_chi_and_F((chi - chain_chi[b]) / (B - 1.0), (F - chain_F[d][b]) / (B - 1.0), M);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      r.error = std::sqrt((B - 1.0) / B * s2);
    }
    return r;
  }
  double mean() const { return draws_counted ? improved_sum / draws_counted : 0.0; }
  double error() const {
    if (draws_counted < 2) return 0.0;
    const double n = (double)draws_counted, m = improved_sum / n, var = std::max(0.0, (improved_sum2 - n * m * m) / (n - 1.0));
    return std::sqrt(var / n);
  }

private:
  void need_structure(const char *what) const {
    if (!with_structure) fatal(owner + "::" + what + ": constructed without ClusterParameters::structure.");
    if (!draws_counted) fatal(owner + "::" + what + ": no draws since reset_improved().");
  }
  const std::string owner;
  const unsigned int B, n_updates;
  const bool with_structure, with_correlator;
  const unsigned int n_out;
  std::vector<double> chain_C;                // per chain and lag: sums over the updates of the improved C
  std::vector<double> chain_chi, chain_F[2];  // per chain: sums over the updates of improved chi_m, F_t, F_x
  double improved_sum = 0.0, improved_sum2 = 0.0;
  uint64_t draws_counted = 0;
};

/** The Wolff single-cluster sampler of the O(3) nonlinear sigma model on either kind of lattice (mlmcpi_sigma_level_cluster_draw
 *  with the action's level: the unrotated lattice delegates to mlmcpi_sigma_cluster_draw, the same bits; the rotated level of
 *  the CoarsenRotate hierarchy runs sigma_cluster.hip, so the sampler can be the coarse sampler of a two-level or
 *  hierarchical run; everything is sized by the level's n = sample_size / 2 vertices).  It is NOT
 *  the reference's ClusterSampler for this action: single_cluster_update (clustersampler.cc:52-89) bonds all eight entries of
 *  Lattice2D::neighbour_vertices while the action couples four, which samples another model; this is the same
 *  walk over the four links per vertex the action has.  One draw = n_updates updates of every chain in one launch, then the
 *  copy out; counters advance by n_updates per draw; set_state is a no-op, as for ClusterSampler.
 *  With ClusterParameters::improved, ::structure or ::correlator it calls mlmcpi_sigma_level_cluster_improved_draw (the same state
 *  and count) and keeps the improved estimators of the single cluster in a ClusterImprovedSums, with the semantics and error
 *  rules of SwendsenWangSampler; with all three off it calls the plain entry point. */
class WolffClusterSampler : public Sampler {
public:
  using Estimate = ClusterImprovedSums::Estimate;
  using CorrelatorEstimate = ClusterImprovedSums::CorrelatorEstimate;
  WolffClusterSampler(const std::shared_ptr<Action> action_, const ClusterParameters p)
      : Sampler(), action(std::dynamic_pointer_cast<NonlinearSigmaAction>(action_)), n_updates(p.n_updates), B(p.batch),
        with_improved(p.improved || p.structure || p.correlator), with_structure(p.structure), with_correlator(p.correlator),
        sites(p.batch, sizeof(uint32_t)) {
    if (!action) fatal(" wolff sampler not supported for chosen action: it is built for the nonlinear sigma model only.");
    // the device adds the flipped vertices of one call to a uint32 per chain: n_updates updates of at most N vertices each
    if ((uint64_t)n_updates * (action->sample_size() / 2) > 0xFFFFFFFFull)
      fatal("WolffClusterSampler: n_updates x vertices must stay below 2^32 (the per-chain counter of one draw).");
    size_t bytes = 0;
    const mlmcpi_sigma_level lv = action->level();
    if (with_improved) {
      if (n_updates == 0) fatal("WolffClusterSampler: n_updates must be positive with the improved estimators.");
      uint32_t n = 0;
      check(mlmcpi_sigma_level_correlator_size(&lv, &n), "sigma_level_correlator_size");
      n_out = n;
      improved = std::make_unique<DeviceVector>((size_t)B);
      if (with_structure) structure = std::make_unique<DeviceVector>(2 * (size_t)B);
      if (with_correlator) corr = std::make_unique<DeviceVector>((size_t)B * n_out);
      sums = std::make_unique<ClusterImprovedSums>("WolffClusterSampler", B, n_updates, with_structure, with_correlator, n_out);
      check(mlmcpi_sigma_level_cluster_improved_workspace_bytes(&lv, B, &bytes), "sigma_level_cluster_improved_workspace_bytes");
    } else {
      check(mlmcpi_sigma_level_cluster_workspace_bytes(&lv, B, &bytes), "sigma_level_cluster_workspace_bytes");
    }
    work_bytes = bytes;
    work = std::make_shared<DeviceBuffer>(bytes);
    // an update flips at most N = sample_size / 2 vertices: fold before 2^31 could have been added to a chain's counter
    fold_period = std::max<uint64_t>(1, std::min<uint64_t>(1024, (1ull << 32) / ((uint64_t)std::max(1u, n_updates) * action->sample_size())));
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < p.n_burnin; ++i) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int k = 0; k < p.n_meas; ++k) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    cost_per_sample_ = 1.E6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (p.n_meas ? p.n_meas : 1);
    reset_stats();
    fold_sites();
    flipped_total = 0.0;
    updates_counted = 0;
    if (sums) sums->reset();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    if (update_counter > 0xFFFFFFFFu - n_updates) fatal("WolffClusterSampler: the 32-bit update counter of the Philox contract is used up.");
    const mlmcpi_sigma_level lv = action->level();
    if (with_improved) {
      check(mlmcpi_memset(improved->ptr(), 0, B * sizeof(double), nullptr), "mlmcpi_memset");
      if (with_structure) check(mlmcpi_memset(structure->ptr(), 0, 2 * (size_t)B * sizeof(double), nullptr), "mlmcpi_memset");
      if (with_correlator) check(mlmcpi_memset(corr->ptr(), 0, (size_t)B * n_out * sizeof(double), nullptr), "mlmcpi_memset");
      check(mlmcpi_sigma_level_cluster_improved_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                                   action->get_chain0(), update_counter, (uint32_t *)sites.ptr(), (double *)improved->ptr(),
                                                   with_structure ? (double *)structure->ptr() : nullptr,
                                                   with_correlator ? (double *)corr->ptr() : nullptr, work->p, work_bytes, nullptr),
            "sigma_level_cluster_improved_draw");
      const std::vector<double> imp = improved->download<double>();
      std::vector<double> F, C;
      if (with_structure) F = structure->download<double>();
      if (with_correlator) C = corr->download<double>();
      sums->record(lv, imp, with_structure ? &F : nullptr, with_correlator ? &C : nullptr);
    } else {
      check(mlmcpi_sigma_level_cluster_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                            action->get_chain0(), update_counter, (uint32_t *)sites.ptr(), work->p, nullptr),
            "sigma_level_cluster_draw");
    }
    update_counter += n_updates;
    updates_counted += n_updates;
    if (++draws_unfolded >= fold_period) fold_sites();
    n_total_samples += n_updates;
    n_accepted_samples += n_updates;
    phi_state->data = phi_state_cur->data;
    accept = true;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }
  /** flipped vertices per update, averaged over chains and over the updates since construction (burn-in and timing draws
   *  excluded); it keeps its own count of updates, so reset_stats() does not touch it */
  double mean_cluster_size() {
    if (!updates_counted) return 0.0;
    fold_sites();
    return flipped_total / B / (double)updates_counted;
  }
  void show_stats() override {
    std::cout << std::setprecision(3) << std::fixed << "  cluster updates per draw = " << n_updates << std::endl
              << "  mean cluster size        = " << mean_cluster_size() << " sites" << std::endl;
  }
  /** the improved estimators of the single cluster since the last reset_improved() (the constructor resets after burn-in and
   *  timing draws), with the semantics and error rules of SwendsenWangSampler's; fatal unless constructed with the option */
  bool has_improved() const { return with_improved; }
  bool has_structure() const { return with_structure; }
  bool has_correlator() const { return with_correlator; }
  void reset_improved() { need_improved("reset_improved").reset(); }
  double improved_mean() const { return need_improved("improved_mean").mean(); }
  double improved_error() const { return need_improved("improved_error").error(); }
  Estimate improved_structure_factor(int d) const { return need_improved("improved_structure_factor").structure_factor(d); }
  Estimate improved_xi(int d) const { return need_improved("improved_xi").xi(d, action->level()); }
  CorrelatorEstimate improved_correlator() const { return need_improved("improved_correlator").correlator(); }
  /** the host total of flipped sites (folds so far) and the device counters not yet folded into it; read only */
  double flipped_sites_folded() const { return flipped_total; }
  std::vector<uint32_t> flipped_sites_unfolded() const { return sites.download<uint32_t>(); }

private:
  ClusterImprovedSums &need_improved(const char *what) const {
    if (!sums) fatal(std::string("WolffClusterSampler::") + what + ": constructed without ClusterParameters::improved, ::structure or ::correlator.");
    return *sums;
  }
  void fold_sites() {
    for (uint32_t v : sites.download<uint32_t>()) flipped_total += v;
    check(mlmcpi_memset(sites.ptr(), 0, B * sizeof(uint32_t), nullptr), "mlmcpi_memset");
    draws_unfolded = 0;
  }
  const std::shared_ptr<NonlinearSigmaAction> action;
  const unsigned int n_updates, B;
  const bool with_improved, with_structure, with_correlator;
  unsigned int n_out = 0;
  std::unique_ptr<DeviceVector> improved, structure, corr;  // double [batch], [batch][2], [batch][n_out]: the draw at hand, summed over its updates
  std::unique_ptr<ClusterImprovedSums> sums;                // what is kept since reset_improved(); NULL with the three options off
  std::shared_ptr<SampleState> phi_state_cur;
  std::shared_ptr<DeviceBuffer> work;
  size_t work_bytes = 0;
  DeviceVector sites;  // uint32 per chain: flipped vertices since the last fold, added up on the device
  double flipped_total = 0.0;
  uint64_t fold_period = 1;
  uint64_t draws_unfolded = 0;
  uint64_t updates_counted = 0;  // the updates flipped_total belongs to
  uint32_t update_counter = 0;
  double cost_per_sample_ = 0.0;
};

class WolffClusterSamplerFactory : public SamplerFactory {
public:
  explicit WolffClusterSamplerFactory(const ClusterParameters p) : param(p) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override {
    return std::make_shared<WolffClusterSampler>(action, param);  // fatal unless the action is the nonlinear sigma model
  }
private:
  const ClusterParameters param;
};

/** The Swendsen-Wang multi-cluster sampler of the O(3) nonlinear sigma model on either kind of lattice
 *  (mlmcpi_sigma_level_sw_draw with the action's level: the unrotated lattice delegates to mlmcpi_sigma_sw_draw, the same bits;
 *  the rotated level of the CoarsenRotate hierarchy runs sigma_sw.hip, so the sampler can be the coarse sampler of a
 *  two-level or hierarchical run; everything is sized by the level's n = sample_size / 2 vertices): the
 *  multi-cluster form of WolffClusterSampler's embedding, the project's own sampler like that one.  One draw = n_updates
 *  updates of every chain, then the copy out; it runs its own update counter, which advances by n_updates per draw; set_state
 *  is a no-op.  Every draw also returns the clusters and the improved estimator of chi_m (3 sum_C A_C^2 / N of the field
 *  before each update): the sampler keeps, since the last reset_improved(), the mean over draws of the per-draw value (the
 *  mean over the draw's updates and over the chains) and its standard error over the draws.
 *  With ClusterParameters::structure it calls mlmcpi_sigma_level_sw_structure_draw (the same state and the same three outputs)
 *  and keeps PER CHAIN the sums of the improved chi_m, F_t and F_x since reset_improved(): improved_structure_factor(d) is the
 *  mean over the chains with their spread as the error, improved_xi(d) is xi_2 from the chain-averaged improved (chi, F) with a
 *  jackknife over the chains, the arithmetic of SigmaCorrelator::xi (NaN where chi / F < 1).
 *  With ClusterParameters::correlator it calls mlmcpi_sigma_level_sw_correlator_draw (again the same state and three outputs)
 *  and keeps PER CHAIN the sums of the improved C_t and C_x, every lag, since reset_improved(): improved_correlator() gives
 *  their means and errors as SigmaCorrelator::means_and_errors does.  With both options set it still makes that one call per
 *  draw: F_d of a draw is then structure_factor() of the draw's improved C_d (correlator.hh), chain by chain. */
class SwendsenWangSampler : public Sampler {
public:
  using Estimate = ClusterImprovedSums::Estimate;
  using CorrelatorEstimate = ClusterImprovedSums::CorrelatorEstimate;
  SwendsenWangSampler(const std::shared_ptr<Action> action_, const ClusterParameters p)
      : Sampler(), action(std::dynamic_pointer_cast<NonlinearSigmaAction>(action_)), n_updates(p.n_updates), B(p.batch),
        with_structure(p.structure), with_correlator(p.correlator), clusters(p.batch, sizeof(uint32_t)), improved(p.batch),
        structure(2 * (size_t)p.batch) {
    if (!action) fatal(" swendsenwang sampler not supported for chosen action: it is built for the nonlinear sigma model only.");
    if (n_updates == 0) fatal("SwendsenWangSampler: n_updates must be positive.");
    // the device adds the clusters of one call to a uint32 per chain: n_updates updates of at most N clusters each
    if ((uint64_t)n_updates * (action->sample_size() / 2) > 0xFFFFFFFFull)
      fatal("SwendsenWangSampler: n_updates x vertices must stay below 2^32 (the per-chain counter of one draw).");
    const mlmcpi_sigma_level lv = action->level();
    if (with_correlator) {
      uint32_t n = 0;
      check(mlmcpi_sigma_level_correlator_size(&lv, &n), "sigma_level_correlator_size");
      n_out = n;
      corr = std::make_unique<DeviceVector>((size_t)B * n_out);
      check(mlmcpi_sigma_level_sw_correlator_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_correlator_workspace_bytes");
    } else if (with_structure) check(mlmcpi_sigma_level_sw_structure_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_structure_workspace_bytes");
    else check(mlmcpi_sigma_level_sw_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_workspace_bytes");
    sums = std::make_unique<ClusterImprovedSums>("SwendsenWangSampler", B, n_updates, with_structure, with_correlator, n_out);
    work = std::make_shared<DeviceBuffer>(work_bytes);
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < p.n_burnin; ++i) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned int k = 0; k < p.n_meas; ++k) draw(tmp);
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    cost_per_sample_ = 1.E6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (p.n_meas ? p.n_meas : 1);
    reset_stats();
    reset_improved();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    if (update_counter > 0xFFFFFFFFu - n_updates) fatal("SwendsenWangSampler: the 32-bit update counter of the Philox contract is used up.");
    check(mlmcpi_memset(clusters.ptr(), 0, B * sizeof(uint32_t), nullptr), "mlmcpi_memset");
    check(mlmcpi_memset(improved.ptr(), 0, B * sizeof(double), nullptr), "mlmcpi_memset");
    const mlmcpi_sigma_level lv = action->level();
    if (with_correlator) {
      check(mlmcpi_memset(corr->ptr(), 0, (size_t)B * n_out * sizeof(double), nullptr), "mlmcpi_memset");
      check(mlmcpi_sigma_level_sw_correlator_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                                action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                                (double *)improved.ptr(), (double *)corr->ptr(), work->p, work_bytes, nullptr),
            "sigma_level_sw_correlator_draw");
    } else if (with_structure) {
      check(mlmcpi_memset(structure.ptr(), 0, 2 * (size_t)B * sizeof(double), nullptr), "mlmcpi_memset");
      check(mlmcpi_sigma_level_sw_structure_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                               action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                               (double *)improved.ptr(), (double *)structure.ptr(), work->p, work_bytes, nullptr),
            "sigma_level_sw_structure_draw");
    } else {
      check(mlmcpi_sigma_level_sw_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                       action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                       (double *)improved.ptr(), work->p, nullptr),
            "sigma_level_sw_draw");
    }
    update_counter += n_updates;
    double c = 0.0;
    for (uint32_t x : clusters.download<uint32_t>()) c += x;
    const std::vector<double> imp = improved.download<double>();
    if (with_correlator) {
      const std::vector<double> C = corr->download<double>();
      sums->record(lv, imp, nullptr, &C);
    } else if (with_structure) {
      const std::vector<double> F = structure.download<double>();
      sums->record(lv, imp, &F, nullptr);
    } else {
      sums->record(lv, imp, nullptr, nullptr);
    }
    clusters_total += c / B;
    n_total_samples += n_updates;
    n_accepted_samples += n_updates;
    phi_state->data = phi_state_cur->data;
    accept = true;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }
  /** forget the clusters and improved values recorded so far (the constructor does, after burn-in and timing draws) */
  void reset_improved() {
    clusters_total = 0.0;
    sums->reset();
  }
  bool has_structure() const { return with_structure; }
  bool has_correlator() const { return with_correlator; }
  /** the improved C_t (first Mt / 2 + 1 entries) and C_x: per lag the mean over the chains of their means over the updates since
   *  the last reset; batch >= 2: with the spread of the per-chain means over sqrt(batch), as SigmaCorrelator::means_and_errors */
  CorrelatorEstimate improved_correlator() const { return sums->correlator(); }
  /** improved structure factor of direction d (0: t, 1: x) at the lowest momentum: the mean over the chains of their means
   *  since the last reset; batch >= 2: with the spread of the per-chain means over sqrt(batch) */
  Estimate improved_structure_factor(int d) const { return sums->structure_factor(d); }
  /** xi_2 of direction d from the chain-averaged improved chi_m and F_d (xi_from_chi_and_F: NaN where chi / F < 1); batch >= 2:
   *  with the jackknife error over the chains, as SigmaCorrelator::xi forms it */
  Estimate improved_xi(int d) const { return sums->xi(d, action->level()); }
  /** clusters per update, averaged over the chains and the updates since the last reset */
  double mean_clusters_per_update() const { return sums->draws() ? clusters_total / ((double)sums->draws() * n_updates) : 0.0; }
  /** improved estimator of chi_m, averaged over the chains and the updates since the last reset */
  double improved_mean() const { return sums->mean(); }
  /** its standard error over the draws, each draw contributing the mean of its updates */
  double improved_error() const { return sums->error(); }
  void show_stats() override {
    std::cout << std::setprecision(3) << std::fixed << "  cluster updates per draw = " << n_updates << std::endl
              << std::setprecision(6) << "  improved chi_m = " << improved_mean() << " +/- " << improved_error() << std::endl
              << std::setprecision(3) << "  mean clusters per update = " << mean_clusters_per_update() << std::endl;
  }

private:
  const std::shared_ptr<NonlinearSigmaAction> action;
  const unsigned int n_updates, B;
  const bool with_structure, with_correlator;
  unsigned int n_out = 0;
  std::unique_ptr<DeviceVector> corr;  // double [batch][n_out]: the improved C of the draw at hand, summed over its updates
  std::unique_ptr<ClusterImprovedSums> sums;  // what is kept since reset_improved()
  std::shared_ptr<SampleState> phi_state_cur;
  std::shared_ptr<DeviceBuffer> work;
  size_t work_bytes = 0;
  DeviceVector clusters;   // uint32 per chain: the clusters of the draw at hand
  DeviceVector improved;   // double per chain: the improved values of the draw at hand, summed over its updates
  DeviceVector structure;  // double [batch][2]: the improved (F_t, F_x) of the draw at hand, summed over its updates
  double clusters_total = 0.0;
  uint32_t update_counter = 0;
  double cost_per_sample_ = 0.0;
};

class SwendsenWangSamplerFactory : public SamplerFactory {
public:
  explicit SwendsenWangSamplerFactory(const ClusterParameters p) : param(p) {}
  std::shared_ptr<Sampler> get(std::shared_ptr<Action> action) override {
    return std::make_shared<SwendsenWangSampler>(action, param);  // fatal unless the action is the nonlinear sigma model
  }
private:
  const ClusterParameters param;
};

}  // namespace mlmcpi
#endif
