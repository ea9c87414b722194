// cluster_sampler.hh -- the cluster samplers: ClusterSampler (sampler/clustersampler.{hh,cc}, the rotor),
// QuenchedSchwingerClusterSampler (sampler/quenchedschwingerclustersampler.{hh,cc}) and the project's own WolffClusterSampler and
// SwendsenWangSampler of the O(3) sigma model, with the parts they share: the flipped-site counter, the per-draw device outputs
// of the improved estimators and the two checks of the 32-bit counters.
#ifndef MLMCPI_CLUSTER_SAMPLER_HH
#define MLMCPI_CLUSTER_SAMPLER_HH
#include <algorithm>
#include <iomanip>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "cluster_improved.hh"
#include "sampler.hh"

namespace mlmcpi {

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

/** a draw advances the Philox update counter by n_updates: fatal where the next draw would pass 2^32 */
inline void check_update_counter(const char *owner, uint32_t update_counter, unsigned int n_updates) {
  if (update_counter > 0xFFFFFFFFu - n_updates) fatal(std::string(owner) + ": the 32-bit update counter of the Philox contract is used up.");
}

/** the device adds what one call flips or finds to a uint32 per chain: n_updates updates of at most `vertices` each */
inline void check_draw_fits_counter(const char *owner, unsigned int n_updates, uint64_t vertices) {
  if ((uint64_t)n_updates * vertices > 0xFFFFFFFFull)
    fatal(std::string(owner) + ": n_updates x vertices must stay below 2^32 (the per-chain counter of one draw).");
}

/** The flipped sites of ClusterSampler and WolffClusterSampler: a uint32 per chain that the draws add to on the device, and the
 *  host total they are folded into before they can wrap.  A draw adds at most `most_per_draw` (updates x sites) to a chain's
 *  counter: fold before 2^31 could have been added to it, at least every 1024 draws. */
class FlippedSiteCounter {
public:
  FlippedSiteCounter(unsigned int B_, uint64_t most_per_draw)
      : B(B_), sites(B_, sizeof(uint32_t)), fold_period(std::max<uint64_t>(1, std::min<uint64_t>(1024, (1ull << 31) / most_per_draw))) {}
  /** uint32 [B]: where a draw adds the sites it flipped */
  uint32_t *device() { return (uint32_t *)sites.ptr(); }
  /** add the device counters to the host total and zero them */
  void fold() {
    for (uint32_t v : sites.download<uint32_t>()) flipped_total += v;
    check(mlmcpi_memset(sites.ptr(), 0, B * sizeof(uint32_t), nullptr), "mlmcpi_memset");
    draws_unfolded = 0;
  }
  void after_draw() {
    if (++draws_unfolded >= fold_period) fold();
  }
  /** forget what was counted so far, on the device and here */
  void reset_total() {
    fold();
    flipped_total = 0.0;
  }
  /** the host total (folds so far) and the device counters not yet folded into it; read only */
  double total() const { return flipped_total; }
  std::vector<uint32_t> unfolded() const { return sites.download<uint32_t>(); }
  /** flipped sites per update, averaged over chains: folds */
  double mean_per_update(double updates) {
    fold();
    return flipped_total / B / updates;
  }

private:
  const unsigned int B;
  DeviceVector sites;
  double flipped_total = 0.0;
  const uint64_t fold_period;
  uint64_t draws_unfolded = 0;
};

/** show_stats() of ClusterSampler and WolffClusterSampler */
inline void show_cluster_stats(unsigned int n_updates, double mean_cluster_size) {
  std::cout << std::setprecision(3) << std::fixed << "  cluster updates per draw = " << n_updates << std::endl
            << "  mean cluster size        = " << mean_cluster_size << " sites" << std::endl;
}

/** ClusterSampler on a 1-D lattice (sampler/clustersampler.{hh,cc}; single_cluster_update1d): the rotor.  One draw =
 *  n_updates reflection-cluster updates of every chain in one launch (mlmcpi_path_cluster_draw), then the copy out.
 *  Counters advance by n_updates per draw (clustersampler.cc:44-48); set_state is a no-op (clustersampler.hh:116). */
class ClusterSampler : public Sampler {
public:
  ClusterSampler(const std::shared_ptr<Action> action_, const ClusterParameters p)
      : Sampler(), action(std::dynamic_pointer_cast<RotorAction>(action_)), n_burnin(p.n_burnin), n_updates(p.n_updates), B(p.batch) {
    if (!action) fatal(" cluster not supported for chosen action.");
    // an update flips at most M sites
    flipped = std::make_unique<FlippedSiteCounter>(B, (uint64_t)std::max(1u, n_updates) * action->sample_size());
    x_path_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(x_path_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < n_burnin; ++i) draw(tmp);
    cost_per_sample_ = timed_cost_per_sample(p.n_meas, [&]() { draw(tmp); });
    reset_stats();
    flipped->reset_total();
  }
  void draw(std::shared_ptr<SampleState> x_path) override {
    check_update_counter("ClusterSampler", update_counter, n_updates);
    check(mlmcpi_path_cluster_draw(&action->abi_action(), x_path_cur->device_mutable(), B, n_updates, action->get_seed(),
                                   action->get_chain0(), update_counter, flipped->device(), nullptr), "path_cluster_draw");
    update_counter += n_updates;
    flipped->after_draw();
    n_total_samples += n_updates;
    n_accepted_samples += n_updates;
    x_path->data = x_path_cur->data;
    accept = true;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }
  /** flipped sites per update, averaged over chains and over the updates since construction */
  double mean_cluster_size() { return n_total_samples ? flipped->mean_per_update(n_total_samples) : 0.0; }
  void show_stats() override { show_cluster_stats(n_updates, mean_cluster_size()); }
  /** the host total of flipped sites (folds so far) and the device counters not yet folded into it; read only */
  double flipped_sites_folded() const { return flipped->total(); }
  std::vector<uint32_t> flipped_sites_unfolded() const { return flipped->unfolded(); }

private:
  const std::shared_ptr<RotorAction> action;
  const unsigned int n_burnin, n_updates, B;
  std::shared_ptr<SampleState> x_path_cur;
  std::unique_ptr<FlippedSiteCounter> flipped;
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
    cost_per_sample_ = timed_cost_per_sample(p.n_meas, [&]() { draw(tmp); });
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

/** The device outputs of one draw of the improved estimators (WolffClusterSampler, SwendsenWangSampler), each summed over the
 *  draw's updates: improved double [B] and, where asked for, structure [B][2] (F_t, F_x) and corr [B][n_out].  The draw ADDS to
 *  them, so zero() comes before it; record_into() downloads them after it, in the order improved, structure, corr both times. */
class ImprovedDrawOutputs {
public:
  ImprovedDrawOutputs(unsigned int B_, bool with_structure, bool with_correlator, unsigned int n_out_)
      : B(B_), n_out(n_out_), improved_(B_), structure_(with_structure ? std::make_unique<DeviceVector>(2 * (size_t)B_) : nullptr),
        corr_(with_correlator ? std::make_unique<DeviceVector>((size_t)B_ * n_out_) : nullptr) {}
  void zero() {
    check(mlmcpi_memset(improved_.ptr(), 0, B * sizeof(double), nullptr), "mlmcpi_memset");
    if (structure_) check(mlmcpi_memset(structure_->ptr(), 0, 2 * B * sizeof(double), nullptr), "mlmcpi_memset");
    if (corr_) check(mlmcpi_memset(corr_->ptr(), 0, B * n_out * sizeof(double), nullptr), "mlmcpi_memset");
  }
  /** the device pointers; NULL where the option is off */
  double *improved() { return (double *)improved_.ptr(); }
  double *structure() { return structure_ ? (double *)structure_->ptr() : nullptr; }
  double *corr() { return corr_ ? (double *)corr_->ptr() : nullptr; }
  /** the finished draw on an Mt x Mx level, into what is kept since the last reset */
  void record_into(ClusterImprovedSums &sums, unsigned int Mt, unsigned int Mx) const {
    const std::vector<double> imp = improved_.download<double>();
    std::vector<double> F, C;
    if (structure_) F = structure_->download<double>();
    if (corr_) C = corr_->download<double>();
    sums.record(Mt, Mx, imp, structure_ ? &F : nullptr, corr_ ? &C : nullptr);
  }

private:
  const size_t B, n_out;
  DeviceVector improved_;
  const std::unique_ptr<DeviceVector> structure_, corr_;
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
        with_improved(p.improved || p.structure || p.correlator), with_structure(p.structure), with_correlator(p.correlator) {
    if (!action) fatal(" wolff sampler not supported for chosen action: it is built for the nonlinear sigma model only.");
    check_draw_fits_counter("WolffClusterSampler", n_updates, action->sample_size() / 2);
    const mlmcpi_sigma_level lv = action->level();
    if (with_improved) {
      if (n_updates == 0) fatal("WolffClusterSampler: n_updates must be positive with the improved estimators.");
      uint32_t n_out = 0;
      check(mlmcpi_sigma_level_correlator_size(&lv, &n_out), "sigma_level_correlator_size");
      outputs = std::make_unique<ImprovedDrawOutputs>(B, with_structure, with_correlator, n_out);
      sums = std::make_unique<ClusterImprovedSums>("WolffClusterSampler", B, n_updates, with_structure, with_correlator, n_out);
      check(mlmcpi_sigma_level_cluster_improved_workspace_bytes(&lv, B, &work_bytes), "sigma_level_cluster_improved_workspace_bytes");
    } else {
      check(mlmcpi_sigma_level_cluster_workspace_bytes(&lv, B, &work_bytes), "sigma_level_cluster_workspace_bytes");
    }
    work = std::make_shared<DeviceBuffer>(work_bytes);
    // an update flips at most N = sample_size / 2 vertices
    flipped = std::make_unique<FlippedSiteCounter>(B, (uint64_t)std::max(1u, n_updates) * (action->sample_size() / 2));
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < p.n_burnin; ++i) draw(tmp);
    cost_per_sample_ = timed_cost_per_sample(p.n_meas, [&]() { draw(tmp); });
    reset_stats();
    flipped->reset_total();
    updates_counted = 0;
    if (sums) sums->reset();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    check_update_counter("WolffClusterSampler", update_counter, n_updates);
    const mlmcpi_sigma_level lv = action->level();
    if (with_improved) {
      outputs->zero();
      check(mlmcpi_sigma_level_cluster_improved_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                                   action->get_chain0(), update_counter, flipped->device(), outputs->improved(),
                                                   outputs->structure(), outputs->corr(), work->p, work_bytes, nullptr),
            "sigma_level_cluster_improved_draw");
      outputs->record_into(*sums, lv.Mt, lv.Mx);
    } else {
      check(mlmcpi_sigma_level_cluster_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                            action->get_chain0(), update_counter, flipped->device(), work->p, nullptr),
            "sigma_level_cluster_draw");
    }
    update_counter += n_updates;
    updates_counted += n_updates;
    flipped->after_draw();
    n_total_samples += n_updates;
    n_accepted_samples += n_updates;
    phi_state->data = phi_state_cur->data;
    accept = true;
  }
  void set_state(std::shared_ptr<SampleState>) override {}
  double cost_per_sample() override { return cost_per_sample_; }
  /** flipped vertices per update, averaged over chains and over the updates since construction (burn-in and timing draws
   *  excluded); it keeps its own count of updates, so reset_stats() does not touch it */
  double mean_cluster_size() { return updates_counted ? flipped->mean_per_update((double)updates_counted) : 0.0; }
  void show_stats() override { show_cluster_stats(n_updates, mean_cluster_size()); }
  /** the improved estimators of the single cluster since the last reset_improved() (the constructor resets after burn-in and
   *  timing draws), with the semantics and error rules of SwendsenWangSampler's; fatal unless constructed with the option */
  bool has_improved() const { return with_improved; }
  bool has_structure() const { return with_structure; }
  bool has_correlator() const { return with_correlator; }
  void reset_improved() { need_improved("reset_improved").reset(); }
  double improved_mean() const { return need_improved("improved_mean").mean(); }
  double improved_error() const { return need_improved("improved_error").error(); }
  Estimate improved_structure_factor(int d) const { return need_improved("improved_structure_factor").structure_factor(d); }
  Estimate improved_xi(int d) const { return need_improved("improved_xi").xi(d, extent(d)); }
  CorrelatorEstimate improved_correlator() const { return need_improved("improved_correlator").correlator(); }
  /** the host total of flipped sites (folds so far) and the device counters not yet folded into it; read only */
  double flipped_sites_folded() const { return flipped->total(); }
  std::vector<uint32_t> flipped_sites_unfolded() const { return flipped->unfolded(); }

private:
  ClusterImprovedSums &need_improved(const char *what) const {
    if (!sums) fatal(std::string("WolffClusterSampler::") + what + ": constructed without ClusterParameters::improved, ::structure or ::correlator.");
    return *sums;
  }
  unsigned int extent(int d) const { return d == 0 ? action->level().Mt : action->level().Mx; }
  const std::shared_ptr<NonlinearSigmaAction> action;
  const unsigned int n_updates, B;
  const bool with_improved, with_structure, with_correlator;
  std::unique_ptr<ImprovedDrawOutputs> outputs;  // the draw at hand; NULL with the three options off
  std::unique_ptr<ClusterImprovedSums> sums;     // what is kept since reset_improved(); NULL with the three options off
  std::shared_ptr<SampleState> phi_state_cur;
  std::shared_ptr<DeviceBuffer> work;
  size_t work_bytes = 0;
  std::unique_ptr<FlippedSiteCounter> flipped;
  uint64_t updates_counted = 0;  // the updates the flipped total belongs to
  uint32_t update_counter = 0;
  double cost_per_sample_ = 0.0;
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
        with_structure(p.structure), with_correlator(p.correlator), clusters(p.batch, sizeof(uint32_t)) {
    if (!action) fatal(" swendsenwang sampler not supported for chosen action: it is built for the nonlinear sigma model only.");
    if (n_updates == 0) fatal("SwendsenWangSampler: n_updates must be positive.");
    check_draw_fits_counter("SwendsenWangSampler", n_updates, action->sample_size() / 2);
    const mlmcpi_sigma_level lv = action->level();
    uint32_t n_out = 0;
    if (with_correlator) {
      check(mlmcpi_sigma_level_correlator_size(&lv, &n_out), "sigma_level_correlator_size");
      check(mlmcpi_sigma_level_sw_correlator_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_correlator_workspace_bytes");
    } else if (with_structure) check(mlmcpi_sigma_level_sw_structure_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_structure_workspace_bytes");
    else check(mlmcpi_sigma_level_sw_workspace_bytes(&lv, B, &work_bytes), "sigma_level_sw_workspace_bytes");
    // with the correlator the device returns C alone: F, if asked for, is formed from it on the host
    outputs = std::make_unique<ImprovedDrawOutputs>(B, with_structure && !with_correlator, with_correlator, n_out);
    sums = std::make_unique<ClusterImprovedSums>("SwendsenWangSampler", B, n_updates, with_structure, with_correlator, n_out);
    work = std::make_shared<DeviceBuffer>(work_bytes);
    phi_state_cur = std::make_shared<SampleState>(action->sample_size(), B);
    action->initialise_state(phi_state_cur);
    std::shared_ptr<SampleState> tmp = std::make_shared<SampleState>(action->sample_size(), B);
    for (unsigned int i = 0; i < p.n_burnin; ++i) draw(tmp);
    cost_per_sample_ = timed_cost_per_sample(p.n_meas, [&]() { draw(tmp); });
    reset_stats();
    reset_improved();
  }
  void draw(std::shared_ptr<SampleState> phi_state) override {
    check_update_counter("SwendsenWangSampler", update_counter, n_updates);
    check(mlmcpi_memset(clusters.ptr(), 0, B * sizeof(uint32_t), nullptr), "mlmcpi_memset");
    outputs->zero();
    const mlmcpi_sigma_level lv = action->level();
    if (with_correlator) {
      check(mlmcpi_sigma_level_sw_correlator_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                                action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                                outputs->improved(), outputs->corr(), work->p, work_bytes, nullptr),
            "sigma_level_sw_correlator_draw");
    } else if (with_structure) {
      check(mlmcpi_sigma_level_sw_structure_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                               action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                               outputs->improved(), outputs->structure(), work->p, work_bytes, nullptr),
            "sigma_level_sw_structure_draw");
    } else {
      check(mlmcpi_sigma_level_sw_draw(&lv, phi_state_cur->device_mutable(), B, n_updates, action->get_seed(),
                                       action->get_chain0(), update_counter, nullptr, (uint32_t *)clusters.ptr(),
                                       outputs->improved(), work->p, nullptr),
            "sigma_level_sw_draw");
    }
    update_counter += n_updates;
    double c = 0.0;
    for (uint32_t x : clusters.download<uint32_t>()) c += x;
    outputs->record_into(*sums, lv.Mt, lv.Mx);
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
  Estimate improved_xi(int d) const { return sums->xi(d, d == 0 ? action->level().Mt : action->level().Mx); }
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
  std::unique_ptr<ImprovedDrawOutputs> outputs;  // the draw at hand
  std::unique_ptr<ClusterImprovedSums> sums;     // what is kept since reset_improved()
  std::shared_ptr<SampleState> phi_state_cur;
  std::shared_ptr<DeviceBuffer> work;
  size_t work_bytes = 0;
  DeviceVector clusters;  // uint32 per chain: the clusters of the draw at hand
  double clusters_total = 0.0;
  uint32_t update_counter = 0;
  double cost_per_sample_ = 0.0;
};

typedef ParameterSamplerFactory<WolffClusterSampler, ClusterParameters> WolffClusterSamplerFactory;  // fatal unless the action is the nonlinear sigma model
typedef ParameterSamplerFactory<SwendsenWangSampler, ClusterParameters> SwendsenWangSamplerFactory;  // likewise

}  // namespace mlmcpi
#endif
