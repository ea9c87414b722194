// qoi.hh -- QoI interface (qoi/quantityofinterest.hh:16-36) and the five observables of the sweep
// path as device reductions.  evaluate() returns chain 0; evaluate_batch() all chains of the state;
// evaluate_device() leaves the per-chain values on the device (asynchronous: no host round trip per sample, for
// loops that accumulate statistics on the device with mlmcpi_stats_accumulate).
// After the QoIs, the measurements beside the QoI (SigmaCorrelator, PathCorrelator, WilsonLoops, GffCorrelator): each is its ABI
// call and its one derived quantity on top of CorrelatorMeasurement, which keeps the per-chain sums on the device; the arithmetic
// on those sums is chain_estimate.hh, the derived quantities themselves correlator.hh.
#ifndef MLMCPI_QOI_HH
#define MLMCPI_QOI_HH
#include <algorithm>
#include <cmath>

#include "action.hh"
#include "chain_estimate.hh"
#include "correlator.hh"

namespace mlmcpi {

class QoI {
public:
  QoI() {}
  virtual ~QoI() {}
  const double virtual evaluate(const std::shared_ptr<SampleState> phi_state) { return evaluate_batch(phi_state)[0]; }
  virtual std::vector<double> evaluate_batch(const std::shared_ptr<SampleState> phi_state) {
    if (!out || out_n != phi_state->batch()) {
      out = std::make_unique<DeviceVector>(phi_state->batch());  // allocated once per batch size, not per sample
      out_n = phi_state->batch();
    }
    evaluate_device(phi_state, (double *)out->ptr());
    return out->download<double>();
  }
  /** d_out[b] = Q(chain b), enqueued on the default stream */
  virtual void evaluate_device(const std::shared_ptr<SampleState> phi_state, double *d_out) = 0;
  /** selector of mlmcpi_lattice_sweep_draw_qoi for QoIs a sweep sampler can sum inside its last launch (0: none) */
  virtual int fused_kind() const { return 0; }

private:
  std::unique_ptr<DeviceVector> out;
  unsigned int out_n = 0;
};

class QoIFactory {
public:
  virtual ~QoIFactory() {}
  virtual std::shared_ptr<QoI> get(std::shared_ptr<Action> action) = 0;
};

/** qoi/qm/qoixsquared.cc:7-20 (the size check and its message, verbatim quirk included) */
class QoIXsquared : public QoI {
public:
  explicit QoIXsquared(const std::shared_ptr<Lattice1D> lattice) : M_lat(lattice->getM_lat()) {}
  void evaluate_device(const std::shared_ptr<SampleState> x, double *d_out) override {
    if (x->size() != M_lat) fatal("Evaluating QoISusceptibility on path of wrong size.");
    check(mlmcpi_qoi_xsquared(x->device(), M_lat, x->batch(), d_out, nullptr), "qoi_xsquared");
  }
private:
  const unsigned int M_lat;
};

/** qoi/qm/qoisusceptibility.cc:8-23 */
class QoISusceptibility : public QoI {
public:
  explicit QoISusceptibility(const std::shared_ptr<Lattice1D> lattice) : M_lat(lattice->getM_lat()), T_final(lattice->getT_final()) {}
  void evaluate_device(const std::shared_ptr<SampleState> x, double *d_out) override {
    if (x->size() != M_lat) fatal("Evaluating QoISusceptibility on path of wrong size.");
    check(mlmcpi_qoi_susceptibility(x->device(), M_lat, T_final, x->batch(), d_out, nullptr), "qoi_susceptibility");
  }
  int fused_kind() const override { return 4; }  // mlmcpi_path_sweep_draw_qoi (rotor sweeps)
private:
  const unsigned int M_lat;
  const double T_final;
};

/** qoi/qft/qoi2dsusceptibility.cc:8-27 */
class QoI2DSusceptibility : public QoI {
public:
  explicit QoI2DSusceptibility(const std::shared_ptr<Lattice2D> lattice) : Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()) {}
  int fused_kind() const override { return 2; }
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * Mt_lat * Mx_lat) fatal("Evaluating QoI2DSusceptibility on state of wrong size.");
    check(mlmcpi_qoi_2d_susceptibility(phi->device(), Mt_lat, Mx_lat, phi->batch(), d_out, nullptr), "qoi_2d_susceptibility");
  }
private:
  const unsigned int Mt_lat, Mx_lat;
};

/** qoi/qft/qoiavgplaquette.cc:8-27 */
class QoIAvgPlaquette : public QoI {
public:
  explicit QoIAvgPlaquette(const std::shared_ptr<Lattice2D> lattice) : Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()) {}
  int fused_kind() const override { return 1; }
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * Mt_lat * Mx_lat) fatal("Evaluating QoIAvgPlaquette on state of wrong size.");
    check(mlmcpi_qoi_avg_plaquette(phi->device(), Mt_lat, Mx_lat, phi->batch(), d_out, nullptr), "qoi_avg_plaquette");
  }
private:
  const unsigned int Mt_lat, Mx_lat;
};

/** qoi/qft/qoi2dphisquared.cc:8-15 */
class QoI2DPhiSquared : public QoI {
public:
  explicit QoI2DPhiSquared(const std::shared_ptr<Lattice2D> lattice) : M_lat(lattice->getNvertices()) {}
  int fused_kind() const override { return 3; }
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    check(mlmcpi_qoi_phi_squared(phi->device(), M_lat, phi->batch(), d_out, nullptr), "qoi_phi_squared");
  }
private:
  const unsigned int M_lat;
};

/** qoi/qft/qoi2dmagneticsusceptibility.cc:7-21: |sum_n sigma_n|^2 / N of the O(3) sigma model, on any level of its hierarchy
 *  (N = the vertices of the level; rotated levels through mlmcpi_sigma_level_magnetic_susceptibility) */
class QoI2DMagneticSusceptibility : public QoI {
public:
  explicit QoI2DMagneticSusceptibility(const std::shared_ptr<Lattice2D> lattice)
      : Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()), n_vertices(lattice->getNvertices()), rotated(lattice->is_rotated()) {}
  int fused_kind() const override { return 4; }
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * n_vertices) fatal("Evaluating QoI2DMagneticSusceptibility on state of wrong size.");
    if (rotated) {
      const mlmcpi_sigma_level lv{Mt_lat, Mx_lat, 1, 0.0};
      check(mlmcpi_sigma_level_magnetic_susceptibility(&lv, phi->device(), phi->batch(), d_out, nullptr), "sigma_level_magnetic_susceptibility");
    } else
      check(mlmcpi_qoi_magnetic_susceptibility(phi->device(), Mt_lat, Mx_lat, phi->batch(), d_out, nullptr), "qoi_magnetic_susceptibility");
  }
private:
  const unsigned int Mt_lat, Mx_lat, n_vertices;
  const bool rotated;
};

/** The topological susceptibility chi_t = Q^2 / N of the O(3) sigma model, Q the geometric (Berg-Luescher) charge, on any level of
 *  its hierarchy (mlmcpi_sigma_level_topological_charge; definitions in mlmcpi_hip.h).  Not a QoI of the
 *  reference.  No sweep launch sums it (fused_kind 0): the samplers take the unfused path. */
class QoI2DSigmaTopologicalSusceptibility : public QoI {
public:
  explicit QoI2DSigmaTopologicalSusceptibility(const std::shared_ptr<Lattice2D> lattice)
      : level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0}, n_vertices(lattice->getNvertices()) {}
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * n_vertices) fatal("Evaluating QoI2DSigmaTopologicalSusceptibility on state of wrong size.");
    check(mlmcpi_sigma_level_topological_charge(&level, phi->device(), phi->batch(), nullptr, d_out, nullptr, nullptr),
          "sigma_level_topological_charge");
  }
private:
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices;
};

/** chi_t of the field after n_cool cooling sweeps (mlmcpi_sigma_level_cooled_charge at the one depth n_cool), on
 *  plain and rotated lattices.  The state is only read: cooling runs on a copy in this QoI's own workspace, sized for the batch at
 *  hand.  n_cool = 0 returns what QoI2DSigmaTopologicalSusceptibility returns, bit for bit.  fused_kind 0. */
class QoI2DSigmaCooledTopologicalSusceptibility : public QoI {
public:
  QoI2DSigmaCooledTopologicalSusceptibility(const std::shared_ptr<Lattice2D> lattice, unsigned int n_cool_)
      : level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0}, n_vertices(lattice->getNvertices()),
        n_cool(n_cool_) {}
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * n_vertices) fatal("Evaluating QoI2DSigmaCooledTopologicalSusceptibility on state of wrong size.");
    if (!work || work_B != phi->batch()) {
      check(mlmcpi_sigma_level_cooling_workspace_bytes(&level, phi->batch(), &work_bytes), "sigma_level_cooling_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    const uint32_t depth = n_cool;
    check(mlmcpi_sigma_level_cooled_charge(&level, phi->device(), phi->batch(), &depth, 1, nullptr, d_out, nullptr, nullptr, work->p,
                                           work_bytes, nullptr),
          "sigma_level_cooled_charge");
  }
private:
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices, n_cool;
  unsigned int work_B = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
};

/** chi_t of the field after n_steps gradient-flow steps of size eps, flow time t = n_steps eps
 *  (mlmcpi_sigma_level_flowed_charge at the one step count n_steps), on plain and rotated lattices.  The state is
 *  only read: the flow runs on a copy in this QoI's own workspace, sized for the batch at hand.  n_steps = 0 returns what
 *  QoI2DSigmaTopologicalSusceptibility returns, bit for bit.  fused_kind 0. */
class QoI2DSigmaFlowedTopologicalSusceptibility : public QoI {
public:
  QoI2DSigmaFlowedTopologicalSusceptibility(const std::shared_ptr<Lattice2D> lattice, double eps_, unsigned int n_steps_)
      : level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0}, n_vertices(lattice->getNvertices()),
        eps(eps_), n_steps(n_steps_) {}
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) override {
    if (phi->size() != 2 * n_vertices) fatal("Evaluating QoI2DSigmaFlowedTopologicalSusceptibility on state of wrong size.");
    if (!work || work_B != phi->batch()) {
      check(mlmcpi_sigma_level_flow_workspace_bytes(&level, phi->batch(), &work_bytes), "sigma_level_flow_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    const uint32_t steps = n_steps;
    check(mlmcpi_sigma_level_flowed_charge(&level, phi->device(), phi->batch(), eps, &steps, 1, nullptr, d_out, nullptr, nullptr, work->p,
                                           work_bytes, nullptr),
          "sigma_level_flowed_charge");
  }
private:
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices;
  const double eps;
  const unsigned int n_steps;
  unsigned int work_B = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
};

/** A measurement beside the QoI: not a QoI, its value is a vector of n_out() numbers per chain.  MonteCarloSingleLevel asks it for
 *  one more sample of the state at hand (accumulate) and how many it has taken (samples).  accumulate() adds the sample's values and
 *  their squares to per-chain sums on the device; the means and their errors are host arithmetic on those sums (chain_estimate.hh).
 *  A measurement supplies its name (the fatal messages carry it), the size of the state it takes, and its two ABI calls. */
class CorrelatorMeasurement {
public:
  using Estimate = ChainEstimate;
  virtual ~CorrelatorMeasurement() {}
  unsigned int n_out() const { return n_out_; }
  /** d_out[b][n_out()] = the values of chain b, enqueued on the default stream */
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) { launch(phi, d_out, nullptr); }
  /** one more sample: its values are added to the per-chain sums (the batch is fixed by the first call) */
  void accumulate(const std::shared_ptr<SampleState> phi) {
    if (!acc || B != phi->batch()) {
      if (n_calls) fatal(name + "::accumulate: the batch changed between samples.");
      B = phi->batch();
      acc = std::make_unique<DeviceVector>(2 * (size_t)B * n_out_);
      out = std::make_unique<DeviceVector>((size_t)B * n_out_);
    }
    launch(phi, (double *)out->ptr(), (double *)acc->ptr());
    ++n_calls;
  }
  unsigned int samples() const { return n_calls; }
  unsigned int batch() const { return B; }
  /** per-chain means over the accumulated samples, [batch][n_out()] */
  std::vector<std::vector<double>> chain_means() const { return chain_means_of(sums(), B, n_out_, n_calls); }
  /** mean and error per entry: the spread of the per-chain means for batch >= 2, the naive error of one chain (chain_estimate) */
  Estimate means_and_errors() const { return chain_estimate(sums(), B, n_out_, n_calls); }

protected:
  CorrelatorMeasurement(const char *name_, unsigned int n_out_) : name(name_), n_out_(n_out_) {}
  /** fatal, with the measurement's own message, unless n is the size of the states it takes */
  virtual void check_size(unsigned int n) const = 0;
  virtual void workspace_bytes(unsigned int batch, size_t *bytes) const = 0;
  virtual void run(const double *d_state, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const = 0;

private:
  std::vector<double> sums() const {
    if (!n_calls) fatal(name + ": no samples accumulated.");
    return acc->download<double>();
  }
  void launch(const std::shared_ptr<SampleState> phi, double *d_out, double *d_acc) {
    check_size(phi->size());
    if (!work || work_B != phi->batch()) {
      workspace_bytes(phi->batch(), &work_bytes);
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    run(phi->device(), phi->batch(), d_out, d_acc, work->p, work_bytes);
  }
  const std::string name;
  const unsigned int n_out_;
  unsigned int B = 0, work_B = 0, n_calls = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
  std::unique_ptr<DeviceVector> acc, out;
};

/** The time-slice correlators C_t(tau), C_x(tau) of the O(3) sigma model on a lattice, rotated or not
 *  (mlmcpi_sigma_level_correlator; definitions in mlmcpi_hip.h): n_out() = (Mt/2 + 1) + (Mx/2 + 1) numbers per chain, C_t first.
 *  xi_2 (correlator.hh) is host arithmetic on their means. */
class SigmaCorrelator : public CorrelatorMeasurement {
public:
  using Xi = ChainScalar;
  explicit SigmaCorrelator(const std::shared_ptr<Lattice2D> lattice)
      : CorrelatorMeasurement("SigmaCorrelator", size_of(level_of(lattice))), level(level_of(lattice)), n_vertices(lattice->getNvertices()) {}
  unsigned int Mt() const { return level.Mt; }
  unsigned int Mx() const { return level.Mx; }
  /** the part of a vector of n_out() entries that belongs to direction d (0: t, 1: x) */
  std::vector<double> direction(const std::vector<double> &v, int d) const {
    const unsigned int nt = level.Mt / 2 + 1;
    return d == 0 ? std::vector<double>(v.begin(), v.begin() + nt) : std::vector<double>(v.begin() + nt, v.end());
  }
  /** xi_2 of direction d from the mean correlator; batch >= 2: with the jackknife error over the chains */
  Xi xi(int d) const {
    const unsigned int M = d == 0 ? level.Mt : level.Mx;
    return chain_jackknife(chain_means(), [&](const std::vector<double> &C) { return xi_second_moment(direction(C, d), M); });
  }

protected:
  void check_size(unsigned int n) const override {
    if (n != 2 * n_vertices) fatal("Evaluating SigmaCorrelator on state of wrong size.");
  }
  void workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_sigma_level_correlator_workspace_bytes(&level, batch, bytes), "sigma_level_correlator_workspace_bytes");
  }
  void run(const double *d_state, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_sigma_level_correlator(&level, d_state, batch, d_out, d_acc, d_work, work_bytes, nullptr), "sigma_level_correlator");
  }

private:
  static mlmcpi_sigma_level level_of(const std::shared_ptr<Lattice2D> lattice) {
    return mlmcpi_sigma_level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0};
  }
  static unsigned int size_of(const mlmcpi_sigma_level &level) {
    uint32_t n = 0;
    check(mlmcpi_sigma_level_correlator_size(&level, &n), "sigma_level_correlator_size");
    return n;
  }
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices;
};

/** What the cooling and the flow profile share: per chain and sample chi_t = Q^2 / n at each of the ascending `points` (depths
 *  or step counts), then E / 4 pi at each of them, n_out() = 2 points.size() numbers.  The device calls have no accumulator
 *  argument, so a sample's 2 n_points numbers per chain make one round trip through the host, where E is divided by 4 pi and the
 *  value and its square are added to the per-chain sums.  A profile supplies its two ABI calls. */
class SigmaSmoothingProfile : public CorrelatorMeasurement {
public:
  /** entry k of the mean over chains; batch >= 2: with the jackknife error over the chains */
  ChainScalar entry(unsigned int k) const {
    return chain_jackknife(chain_means(), [](const std::vector<double> &v) { return v[0]; }, k, 1);
  }

protected:
  SigmaSmoothingProfile(const char *name_, const std::shared_ptr<Lattice2D> lattice, const std::vector<uint32_t> &points_)
      : CorrelatorMeasurement(name_, 2 * (unsigned int)points_.size()),
        level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0}, n_vertices(lattice->getNvertices()),
        points(points_), name(name_) {}
  /** bytes of the device call's own workspace */
  virtual void call_workspace_bytes(unsigned int batch, size_t *bytes) const = 0;
  /** d_chi, d_e [batch][points.size()] of the states d_state */
  virtual void measure(const double *d_state, unsigned int batch, double *d_chi, double *d_e, void *d_work, size_t work_bytes) const = 0;
  void check_size(unsigned int n) const override {
    if (n != 2 * n_vertices) fatal("Evaluating " + name + " on state of wrong size.");
  }
  void workspace_bytes(unsigned int batch, size_t *bytes) const override {
    call_workspace_bytes(batch, bytes);
    *bytes += raw_bytes(batch);
  }
  void run(const double *d_state, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const override {
    const size_t nd = points.size(), raw = raw_bytes(batch), count = (size_t)batch * nd;
    double *d_chi = (double *)((char *)d_work + (work_bytes - raw)), *d_e = d_chi + count;
    measure(d_state, batch, d_chi, d_e, d_work, work_bytes - raw);
    std::vector<double> h(2 * count), v(2 * count);
    check(mlmcpi_copy_d2h(h.data(), d_chi, 2 * count * sizeof(double), nullptr), "copy_d2h");
    const double four_pi = 4.0 * std::acos(-1.0);
    for (size_t b = 0; b < batch; ++b)
      for (size_t k = 0; k < nd; ++k) {
        v[b * 2 * nd + k] = h[b * nd + k];
        v[b * 2 * nd + nd + k] = h[count + b * nd + k] / four_pi;
      }
    check(mlmcpi_copy_h2d(d_out, v.data(), v.size() * sizeof(double), nullptr), "copy_h2d");
    if (d_acc) {
      std::vector<double> a(2 * v.size());
      check(mlmcpi_copy_d2h(a.data(), d_acc, a.size() * sizeof(double), nullptr), "copy_d2h");
      for (size_t i = 0; i < v.size(); ++i) {
        a[2 * i] += v[i];
        a[2 * i + 1] += v[i] * v[i];
      }
      check(mlmcpi_copy_h2d(d_acc, a.data(), a.size() * sizeof(double), nullptr), "copy_h2d");
    }
  }
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices;
  const std::vector<uint32_t> points;

private:
  size_t raw_bytes(unsigned int batch) const { return (2 * (size_t)batch * points.size() * sizeof(double) + 255) & ~(size_t)255; }
  const std::string name;
};

/** The cooling profile of the O(3) sigma model on a lattice, rotated or not (mlmcpi_sigma_level_cooled_charge): chi_t
 *  and E / 4 pi at each of the ascending `depths` (SigmaSmoothingProfile). */
class SigmaCoolingProfile : public SigmaSmoothingProfile {
public:
  SigmaCoolingProfile(const std::shared_ptr<Lattice2D> lattice, const std::vector<uint32_t> &depths_)
      : SigmaSmoothingProfile("SigmaCoolingProfile", lattice, depths_) {}
  const std::vector<uint32_t> &get_depths() const { return points; }

protected:
  void call_workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_sigma_level_cooling_workspace_bytes(&level, batch, bytes), "sigma_level_cooling_workspace_bytes");
  }
  void measure(const double *d_state, unsigned int batch, double *d_chi, double *d_e, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_sigma_level_cooled_charge(&level, d_state, batch, points.data(), (uint32_t)points.size(), nullptr, d_chi, d_e, nullptr,
                                           d_work, work_bytes, nullptr),
          "sigma_level_cooled_charge");
  }
};

/** The flow profile of the O(3) sigma model on a lattice, rotated or not (mlmcpi_sigma_level_flowed_charge): chi_t
 *  and E / 4 pi at each of the ascending step counts `steps` of size eps, flow time t = steps[k] eps (SigmaSmoothingProfile).  The
 *  dimensionless t <E> / n and the reference scale at which it reaches c (correlator.hh flow_scale) are host arithmetic on the
 *  per-chain means. */
class SigmaFlowProfile : public SigmaSmoothingProfile {
public:
  SigmaFlowProfile(const std::shared_ptr<Lattice2D> lattice, double eps_, const std::vector<uint32_t> &steps_)
      : SigmaSmoothingProfile("SigmaFlowProfile", lattice, steps_), eps(eps_) {}
  const std::vector<uint32_t> &get_steps() const { return points; }
  double time(unsigned int k) const { return points[k] * eps; }
  /** t <E> / n at step count k of the list; batch >= 2: with the jackknife error over the chains */
  ChainScalar t_energy(unsigned int k) const {
    const double f = time(k) * 4.0 * std::acos(-1.0) / n_vertices;  // the entries hold E / 4 pi
    return chain_jackknife(chain_means(), [f](const std::vector<double> &v) { return f * v[0]; }, points.size() + k, 1);
  }
  /** the flow time at which t <E> / n = c (flow_scale; NaN where the listed times do not bracket c), jackknife over the chains */
  ChainScalar scale(double c) const {
    const size_t nd = points.size();
    std::vector<double> times(nd);
    for (size_t k = 0; k < nd; ++k) times[k] = time((unsigned int)k);
    const double four_pi_n = 4.0 * std::acos(-1.0) / n_vertices;
    return chain_jackknife(chain_means(), [&](const std::vector<double> &v) {
      std::vector<double> tE(nd);
      for (size_t k = 0; k < nd; ++k) tE[k] = times[k] * four_pi_n * v[k];
      return flow_scale(times, tE, c);
    }, nd, nd);
  }

protected:
  void call_workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_sigma_level_flow_workspace_bytes(&level, batch, bytes), "sigma_level_flow_workspace_bytes");
  }
  void measure(const double *d_state, unsigned int batch, double *d_chi, double *d_e, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_sigma_level_flowed_charge(&level, d_state, batch, eps, points.data(), (uint32_t)points.size(), nullptr, d_chi, d_e, nullptr,
                                           d_work, work_bytes, nullptr),
          "sigma_level_flowed_charge");
  }

private:
  const double eps;
};

/** The time correlator C(tau), tau = 0 .. n_lag - 1, of a 1-D path action (mlmcpi_path_correlator; definitions in
 *  mlmcpi_hip.h): x_j x_{j+tau} averaged over the path for the oscillators, cos(x_j - x_{j+tau}) for the rotor; n_lag numbers per
 *  chain.  The effective mass (correlator.hh) is host arithmetic on their means. */
class PathCorrelator : public CorrelatorMeasurement {
public:
  using Mass = ChainScalar;
  PathCorrelator(const std::shared_ptr<Lattice1D> lattice, int kind, unsigned int n_lag_)
      : CorrelatorMeasurement("PathCorrelator", n_lag_), act{kind, lattice->getM_lat(), lattice->getT_final(), 1.0, 1.0, 0.0, 0.0} {}
  unsigned int n_lag() const { return n_out(); }
  unsigned int M() const { return act.M; }
  /** m_eff(tau), 1 <= tau <= n_lag() - 2, from the mean correlator; batch >= 2: with the jackknife error over the chains */
  Mass effective_mass(unsigned int tau) const {
    if (tau < 1 || tau + 1 >= n_lag()) fatal("PathCorrelator::effective_mass: lag outside 1 .. n_lag - 2.");
    return chain_jackknife(chain_means(), [&](const std::vector<double> &C) { return mlmcpi::effective_mass(C, tau); });
  }

protected:
  void check_size(unsigned int n) const override {
    if (n != act.M) fatal("Evaluating PathCorrelator on path of wrong size.");
  }
  void workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_path_correlator_workspace_bytes(&act, n_lag(), batch, bytes), "path_correlator_workspace_bytes");
  }
  void run(const double *d_x, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_path_correlator(&act, d_x, batch, n_lag(), d_out, d_acc, d_work, work_bytes, nullptr), "path_correlator");
  }

private:
  const mlmcpi_path_action act;  // kind and M are all the correlator reads
};

/** The Wilson loops W(r, s), 1 <= r <= R, 1 <= s <= S, of a quenched Schwinger state (mlmcpi_schwinger_wilson_loops; definitions in
 *  mlmcpi_hip.h): R S numbers per chain, entry (r - 1) S + (s - 1).  The Creutz ratios (correlator.hh) are host arithmetic on
 *  their means. */
class WilsonLoops : public CorrelatorMeasurement {
public:
  using Ratio = ChainScalar;
  WilsonLoops(const std::shared_ptr<Lattice2D> lattice, unsigned int R_, unsigned int S_)
      : CorrelatorMeasurement("WilsonLoops", R_ * S_), Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()), R_(R_), S_(S_) {}
  unsigned int R() const { return R_; }
  unsigned int S() const { return S_; }
  unsigned int Mt() const { return Mt_lat; }
  unsigned int Mx() const { return Mx_lat; }
  /** means_and_errors() on downloaded sums a [batch][n_out][2] (W, W^2) of n samples */
  static Estimate wilson_loops_estimate(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    return chain_estimate(a, B, n_out, n_calls);
  }
  /** the Creutz ratio chi(r, s), 1 <= r <= R(), 1 <= s <= S(), of the mean loops; batch >= 2: with the jackknife error over the chains */
  Ratio creutz(unsigned int r, unsigned int s) const {
    if (r < 1 || r > R_ || s < 1 || s > S_) fatal("WilsonLoops::creutz: loop outside 1 .. R x 1 .. S.");
    return creutz_jackknife(chain_means(), R_, S_, r, s);
  }
  /** the same arithmetic on per-chain means m [batch][R S] */
  static Ratio creutz_jackknife(const std::vector<std::vector<double>> &m, unsigned int R, unsigned int S, unsigned int r, unsigned int s) {
    return chain_jackknife(m, [&](const std::vector<double> &W) { return creutz_ratio(W, R, S, r, s); }, 0, (size_t)R * S);
  }

protected:
  void check_size(unsigned int n) const override {
    if (n != 2 * Mt_lat * Mx_lat) fatal("Evaluating WilsonLoops on state of wrong size.");
  }
  void workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_schwinger_wilson_loops_workspace_bytes(Mt_lat, Mx_lat, R_, S_, batch, bytes), "schwinger_wilson_loops_workspace_bytes");
  }
  void run(const double *d_theta, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_schwinger_wilson_loops(d_theta, Mt_lat, Mx_lat, batch, R_, S_, d_out, d_acc, d_work, work_bytes, nullptr), "schwinger_wilson_loops");
  }

private:
  const unsigned int Mt_lat, Mx_lat, R_, S_;
};

/** The momentum-projected slice correlators C_t(tau; q), C_x(tau; q), q < P, of a Gaussian free field state on a lattice, rotated
 *  or not (mlmcpi_gff_correlator; definitions in mlmcpi_hip.h): n_out() = P (Mt/2 + 1) + P (Mx/2 + 1) numbers per chain, C_t
 *  first, momentum-major, lag fastest.  The energies E_q (the effective mass of correlator.hh) are host arithmetic on their means. */
class GffCorrelator : public CorrelatorMeasurement {
public:
  using Energy = ChainScalar;
  GffCorrelator(const std::shared_ptr<Lattice2D> lattice, unsigned int P_)
      : CorrelatorMeasurement("GffCorrelator", P_ * (lattice->getMt_lat() / 2 + 1) + P_ * (lattice->getMx_lat() / 2 + 1)),
        Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()), rotated(lattice->is_rotated() ? 1 : 0),
        n_vertices(lattice->getNvertices()), P_(P_) {}
  unsigned int n_mom() const { return P_; }
  unsigned int Mt() const { return Mt_lat; }
  unsigned int Mx() const { return Mx_lat; }
  /** where C_d(tau; q) sits in a vector of n_out() entries (d = 0: t, 1: x) */
  static unsigned int index(unsigned int Mt, unsigned int Mx, unsigned int P, int d, unsigned int q, unsigned int tau) {
    const unsigned int nt = Mt / 2 + 1, nx = Mx / 2 + 1;
    return d == 0 ? q * nt + tau : P * nt + q * nx + tau;
  }
  unsigned int index(int d, unsigned int q, unsigned int tau) const { return index(Mt_lat, Mx_lat, P_, d, q, tau); }
  /** chain_means() and means_and_errors() on downloaded sums a [batch][n_out][2] (C, C^2) of n samples */
  static std::vector<std::vector<double>> chain_means_of(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    return mlmcpi::chain_means_of(a, B, n_out, n_calls);
  }
  static Estimate estimate(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    return chain_estimate(a, B, n_out, n_calls);
  }
  /** E_q of direction d (0: t, 1: x) from the effective mass of the mean correlator at lag tau, 1 <= tau <= M_d/2 - 1; batch >= 2:
   *  with the jackknife error over the chains */
  Energy energy(int d, unsigned int q, unsigned int tau) const {
    const unsigned int M = d == 0 ? Mt_lat : Mx_lat;
    if (q >= P_ || tau < 1 || tau + 1 > M / 2) fatal("GffCorrelator::energy: momentum or lag outside its range.");
    return energy_jackknife(chain_means(), Mt_lat, Mx_lat, P_, d, q, tau);
  }
  /** E_q along t, the direction the dispersion relation of correlator.hh speaks of */
  Energy energy(unsigned int q, unsigned int tau) const { return energy(0, q, tau); }
  /** the same arithmetic on per-chain means m [batch][n_out]: the jackknife sees the lags of (d, q) alone */
  static Energy energy_jackknife(const std::vector<std::vector<double>> &m, unsigned int Mt, unsigned int Mx, unsigned int P, int d,
                                 unsigned int q, unsigned int tau) {
    return chain_jackknife(m, [&](const std::vector<double> &C) { return effective_mass(C, tau); }, index(Mt, Mx, P, d, q, 0),
                           (d == 0 ? Mt : Mx) / 2 + 1);
  }

protected:
  void check_size(unsigned int n) const override {
    if (n != n_vertices) fatal("Evaluating GffCorrelator on state of wrong size.");
  }
  void workspace_bytes(unsigned int batch, size_t *bytes) const override {
    check(mlmcpi_gff_correlator_workspace_bytes(Mt_lat, Mx_lat, rotated, P_, batch, bytes), "gff_correlator_workspace_bytes");
  }
  void run(const double *d_phi, unsigned int batch, double *d_out, double *d_acc, void *d_work, size_t work_bytes) const override {
    check(mlmcpi_gff_correlator(Mt_lat, Mx_lat, rotated, P_, d_phi, batch, d_out, d_acc, d_work, work_bytes, nullptr), "gff_correlator");
  }

private:
  const unsigned int Mt_lat, Mx_lat;
  const int rotated;
  const unsigned int n_vertices, P_;
};

}  // namespace mlmcpi
#endif
