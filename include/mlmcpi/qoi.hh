// qoi.hh -- QoI interface (qoi/quantityofinterest.hh:16-36) and the five observables of the sweep
// path as device reductions.  evaluate() returns chain 0; evaluate_batch() all chains of the state;
// evaluate_device() leaves the per-chain values on the device (asynchronous: no host round trip per sample, for
// loops that accumulate statistics on the device with mlmcpi_stats_accumulate).
#ifndef MLMCPI_QOI_HH
#define MLMCPI_QOI_HH
#include <algorithm>
#include <cmath>

#include "action.hh"
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

/** What MonteCarloSingleLevel asks of a correlator it measures beside the QoI: one more sample of the state at hand, and how
 *  many it has taken (SigmaCorrelator, PathCorrelator). */
class CorrelatorMeasurement {
public:
  virtual ~CorrelatorMeasurement() {}
  virtual void accumulate(const std::shared_ptr<SampleState> phi) = 0;
  virtual unsigned int samples() const = 0;
};

/** The time-slice correlators C_t(tau), C_x(tau) of the O(3) sigma model on a lattice, rotated or not
 *  (mlmcpi_sigma_level_correlator; definitions in mlmcpi_hip.h).  Not a QoI: its value is a vector of n_out() =
 *  (Mt/2 + 1) + (Mx/2 + 1) numbers per chain, C_t first.  accumulate() adds the sample's C and C^2 to per-chain sums on the
 *  device; the means, their errors and xi_2 (correlator.hh) are host arithmetic on those sums. */
class SigmaCorrelator : public CorrelatorMeasurement {
public:
  struct Estimate {
    std::vector<double> mean, error;
    bool chain_spread;  // true: error = spread of the per-chain means (batch >= 2); false: the naive error of one chain
  };
  struct Xi {
    double value, error;
    bool has_error;  // the jackknife over chains needs batch >= 2
  };
  explicit SigmaCorrelator(const std::shared_ptr<Lattice2D> lattice)
      : level{lattice->getMt_lat(), lattice->getMx_lat(), lattice->is_rotated() ? 1 : 0, 0.0}, n_vertices(lattice->getNvertices()) {
    uint32_t n = 0;
    check(mlmcpi_sigma_level_correlator_size(&level, &n), "sigma_level_correlator_size");
    n_out_ = n;
  }
  unsigned int n_out() const { return n_out_; }
  unsigned int Mt() const { return level.Mt; }
  unsigned int Mx() const { return level.Mx; }
  /** d_out[b][n_out()] = the correlators of chain b, enqueued on the default stream */
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) { launch(phi, d_out, nullptr); }
  /** one more sample: its correlators are added to the per-chain sums (the batch is fixed by the first call) */
  void accumulate(const std::shared_ptr<SampleState> phi) override {
    if (!acc || B != phi->batch()) {
      if (n_calls) fatal("SigmaCorrelator::accumulate: the batch changed between samples.");
      B = phi->batch();
      acc = std::make_unique<DeviceVector>(2 * (size_t)B * n_out_);
      out = std::make_unique<DeviceVector>((size_t)B * n_out_);
    }
    launch(phi, (double *)out->ptr(), (double *)acc->ptr());
    ++n_calls;
  }
  unsigned int samples() const override { return n_calls; }
  unsigned int batch() const { return B; }
  /** per-chain means of C over the accumulated samples, [batch][n_out()] */
  std::vector<std::vector<double>> chain_means() const {
    if (!n_calls) fatal("SigmaCorrelator: no samples accumulated.");
    const std::vector<double> a = acc->download<double>();
    std::vector<std::vector<double>> m(B, std::vector<double>(n_out_));
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_out_; ++k) m[b][k] = a[2 * ((size_t)b * n_out_ + k)] / n_calls;
    return m;
  }
  /** mean and error per entry.  batch >= 2: the error is the spread of the per-chain means over sqrt(batch), so
   *  autocorrelation inside a chain cannot understate it; batch 1: the naive error of the samples (it ignores autocorrelation) */
  Estimate means_and_errors() const {
    if (!n_calls) fatal("SigmaCorrelator: no samples accumulated.");
    const std::vector<double> a = acc->download<double>();
    Estimate e{std::vector<double>(n_out_, 0.0), std::vector<double>(n_out_, 0.0), B >= 2};
    const double n = n_calls;
    for (unsigned int k = 0; k < n_out_; ++k) {
      if (B >= 2) {
        double s = 0.0, s2 = 0.0;
        for (unsigned int b = 0; b < B; ++b) s += a[2 * ((size_t)b * n_out_ + k)] / n;
        const double m = s / B;
        for (unsigned int b = 0; b < B; ++b) {
          const double d = a[2 * ((size_t)b * n_out_ + k)] / n - m;
          s2 += d * d;
        }
        e.mean[k] = m;
        e.error[k] = std::sqrt(s2 / ((double)B * (B - 1.0)));
      } else {
        const double m = a[2 * k] / n, var = n_calls > 1 ? std::max(0.0, (a[2 * k + 1] / n - m * m) * n / (n - 1.0)) : 0.0;
        e.mean[k] = m;
        e.error[k] = std::sqrt(var / n);
      }
    }
    return e;
  }
  /** the part of a vector of n_out() entries that belongs to direction d (0: t, 1: x) */
  std::vector<double> direction(const std::vector<double> &v, int d) const {
    const unsigned int nt = level.Mt / 2 + 1;
    return d == 0 ? std::vector<double>(v.begin(), v.begin() + nt) : std::vector<double>(v.begin() + nt, v.end());
  }
  /** xi_2 of direction d from the mean correlator; batch >= 2: with the jackknife error over the chains */
  Xi xi(int d) const {
    const unsigned int M = d == 0 ? level.Mt : level.Mx;
    const std::vector<std::vector<double>> m = chain_means();
    std::vector<double> all(n_out_, 0.0);
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_out_; ++k) all[k] += m[b][k];
    std::vector<double> mean(all);
    for (double &v : mean) v /= B;
    Xi r{xi_second_moment(direction(mean, d), M), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B), leave(n_out_);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        for (unsigned int k = 0; k < n_out_; ++k) leave[k] = (all[k] - m[b][k]) / (B - 1.0);
        x[b] = xi_second_moment(direction(leave, d), M);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      r.error = std::sqrt((B - 1.0) / B * s2);
    }
    return r;
  }

private:
  void launch(const std::shared_ptr<SampleState> phi, double *d_out, double *d_acc) {
    if (phi->size() != 2 * n_vertices) fatal("Evaluating SigmaCorrelator on state of wrong size.");
    if (!work || work_B != phi->batch()) {
      check(mlmcpi_sigma_level_correlator_workspace_bytes(&level, phi->batch(), &work_bytes), "sigma_level_correlator_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    check(mlmcpi_sigma_level_correlator(&level, phi->device(), phi->batch(), d_out, d_acc, work->p, work_bytes, nullptr),
          "sigma_level_correlator");
  }
  const mlmcpi_sigma_level level;
  const unsigned int n_vertices;
  unsigned int n_out_ = 0, B = 0, work_B = 0, n_calls = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
  std::unique_ptr<DeviceVector> acc, out;
};

/** The time correlator C(tau), tau = 0 .. n_lag - 1, of a 1-D path action (mlmcpi_path_correlator; definitions in
 *  mlmcpi_hip.h): x_j x_{j+tau} averaged over the path for the oscillators, cos(x_j - x_{j+tau}) for the rotor.  Not a QoI: n_lag
 *  numbers per chain.  accumulate() adds the sample's C and C^2 to per-chain sums on the device; the means, their errors and the
 *  effective mass (correlator.hh) are host arithmetic on those sums. */
class PathCorrelator : public CorrelatorMeasurement {
public:
  struct Estimate {
    std::vector<double> mean, error;
    bool chain_spread;  // true: error = spread of the per-chain means (batch >= 2); false: the naive error of one chain
  };
  struct Mass {
    double value, error;
    bool has_error;  // the jackknife over chains needs batch >= 2
  };
  PathCorrelator(const std::shared_ptr<Lattice1D> lattice, int kind, unsigned int n_lag_)
      : act{kind, lattice->getM_lat(), lattice->getT_final(), 1.0, 1.0, 0.0, 0.0}, n_lag_(n_lag_) {}
  unsigned int n_lag() const { return n_lag_; }
  unsigned int M() const { return act.M; }
  /** d_out[b][n_lag()] = the correlator of chain b, enqueued on the default stream */
  void evaluate_device(const std::shared_ptr<SampleState> x, double *d_out) { launch(x, d_out, nullptr); }
  /** one more sample: its correlator is added to the per-chain sums (the batch is fixed by the first call) */
  void accumulate(const std::shared_ptr<SampleState> x) override {
    if (!acc || B != x->batch()) {
      if (n_calls) fatal("PathCorrelator::accumulate: the batch changed between samples.");
      B = x->batch();
      acc = std::make_unique<DeviceVector>(2 * (size_t)B * n_lag_);
      out = std::make_unique<DeviceVector>((size_t)B * n_lag_);
    }
    launch(x, (double *)out->ptr(), (double *)acc->ptr());
    ++n_calls;
  }
  unsigned int samples() const override { return n_calls; }
  unsigned int batch() const { return B; }
  /** per-chain means of C over the accumulated samples, [batch][n_lag()] */
  std::vector<std::vector<double>> chain_means() const {
    if (!n_calls) fatal("PathCorrelator: no samples accumulated.");
    const std::vector<double> a = acc->download<double>();
    std::vector<std::vector<double>> m(B, std::vector<double>(n_lag_));
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_lag_; ++k) m[b][k] = a[2 * ((size_t)b * n_lag_ + k)] / n_calls;
    return m;
  }
  /** mean and error per lag.  batch >= 2: the error is the spread of the per-chain means over sqrt(batch), so autocorrelation
   *  inside a chain cannot understate it; batch 1: the naive error of the samples (it ignores autocorrelation) */
  Estimate means_and_errors() const {
    if (!n_calls) fatal("PathCorrelator: no samples accumulated.");
    const std::vector<double> a = acc->download<double>();
    Estimate e{std::vector<double>(n_lag_, 0.0), std::vector<double>(n_lag_, 0.0), B >= 2};
    const double n = n_calls;
    for (unsigned int k = 0; k < n_lag_; ++k) {
      if (B >= 2) {
        double s = 0.0, s2 = 0.0;
        for (unsigned int b = 0; b < B; ++b) s += a[2 * ((size_t)b * n_lag_ + k)] / n;
        const double m = s / B;
        for (unsigned int b = 0; b < B; ++b) {
          const double d = a[2 * ((size_t)b * n_lag_ + k)] / n - m;
          s2 += d * d;
        }
        e.mean[k] = m;
        e.error[k] = std::sqrt(s2 / ((double)B * (B - 1.0)));
      } else {
        const double m = a[2 * k] / n, var = n_calls > 1 ? std::max(0.0, (a[2 * k + 1] / n - m * m) * n / (n - 1.0)) : 0.0;
        e.mean[k] = m;
        e.error[k] = std::sqrt(var / n);
      }
    }
    return e;
  }
  /** m_eff(tau), 1 <= tau <= n_lag() - 2, from the mean correlator; batch >= 2: with the jackknife error over the chains */
  Mass effective_mass(unsigned int tau) const {
    if (tau < 1 || tau + 1 >= n_lag_) fatal("PathCorrelator::effective_mass: lag outside 1 .. n_lag - 2.");
    const std::vector<std::vector<double>> m = chain_means();
    std::vector<double> all(n_lag_, 0.0);
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_lag_; ++k) all[k] += m[b][k];
    std::vector<double> mean(all);
    for (double &v : mean) v /= B;
    Mass r{mlmcpi::effective_mass(mean, tau), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B), leave(n_lag_);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        for (unsigned int k = 0; k < n_lag_; ++k) leave[k] = (all[k] - m[b][k]) / (B - 1.0);
        x[b] = mlmcpi::effective_mass(leave, tau);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      r.error = std::sqrt((B - 1.0) / B * s2);
    }
    return r;
  }

private:
  void launch(const std::shared_ptr<SampleState> x, double *d_out, double *d_acc) {
    if (x->size() != act.M) fatal("Evaluating PathCorrelator on path of wrong size.");
    if (!work || work_B != x->batch()) {
      check(mlmcpi_path_correlator_workspace_bytes(&act, n_lag_, x->batch(), &work_bytes), "path_correlator_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = x->batch();
    }
    check(mlmcpi_path_correlator(&act, x->device(), x->batch(), n_lag_, d_out, d_acc, work->p, work_bytes, nullptr), "path_correlator");
  }
  const mlmcpi_path_action act;  // kind and M are all the correlator reads
  const unsigned int n_lag_;
  unsigned int B = 0, work_B = 0, n_calls = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
  std::unique_ptr<DeviceVector> acc, out;
};

/** The Wilson loops W(r, s), 1 <= r <= R, 1 <= s <= S, of a quenched Schwinger state (mlmcpi_schwinger_wilson_loops; definitions in
 *  mlmcpi_hip.h).  Not a QoI: R S numbers per chain, entry (r - 1) S + (s - 1).  accumulate() adds the sample's W and W^2 to
 *  per-chain sums on the device; the means, their errors and the Creutz ratios (correlator.hh) are host arithmetic on those sums. */
class WilsonLoops : public CorrelatorMeasurement {
public:
  struct Estimate {
    std::vector<double> mean, error;
    bool chain_spread;  // true: error = spread of the per-chain means (batch >= 2); false: the naive error of one chain
  };
  struct Ratio {
    double value, error;
    bool has_error;  // the jackknife over chains needs batch >= 2
  };
  WilsonLoops(const std::shared_ptr<Lattice2D> lattice, unsigned int R_, unsigned int S_)
      : Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()), R_(R_), S_(S_), n_out_(R_ * S_) {}
  unsigned int R() const { return R_; }
  unsigned int S() const { return S_; }
  unsigned int Mt() const { return Mt_lat; }
  unsigned int Mx() const { return Mx_lat; }
  /** d_out[b][R()][S()] = the loops of chain b, enqueued on the default stream */
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) { launch(phi, d_out, nullptr); }
  /** one more sample: its loops are added to the per-chain sums (the batch is fixed by the first call) */
  void accumulate(const std::shared_ptr<SampleState> phi) override {
    if (!acc || B != phi->batch()) {
      if (n_calls) fatal("WilsonLoops::accumulate: the batch changed between samples.");
      B = phi->batch();
      acc = std::make_unique<DeviceVector>(2 * (size_t)B * n_out_);
      out = std::make_unique<DeviceVector>((size_t)B * n_out_);
    }
    launch(phi, (double *)out->ptr(), (double *)acc->ptr());
    ++n_calls;
  }
  unsigned int samples() const override { return n_calls; }
  unsigned int batch() const { return B; }
  /** per-chain means of W over the accumulated samples, [batch][R() S()] */
  std::vector<std::vector<double>> chain_means() const {
    if (!n_calls) fatal("WilsonLoops: no samples accumulated.");
    const std::vector<double> a = acc->download<double>();
    std::vector<std::vector<double>> m(B, std::vector<double>(n_out_));
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_out_; ++k) m[b][k] = a[2 * ((size_t)b * n_out_ + k)] / n_calls;
    return m;
  }
  /** mean and error per loop.  batch >= 2: the error is the spread of the per-chain means over sqrt(batch), so autocorrelation
   *  inside a chain cannot understate it; batch 1: the naive error of the samples (it ignores autocorrelation) */
  Estimate means_and_errors() const {
    if (!n_calls) fatal("WilsonLoops: no samples accumulated.");
    return wilson_loops_estimate(acc->download<double>(), B, n_out_, n_calls);
  }
  /** the same arithmetic on downloaded sums a [batch][n_out][2] (W, W^2) of n samples */
  static Estimate wilson_loops_estimate(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    Estimate e{std::vector<double>(n_out, 0.0), std::vector<double>(n_out, 0.0), B >= 2};
    const double n = n_calls;
    for (unsigned int k = 0; k < n_out; ++k) {
      if (B >= 2) {
        double s = 0.0, s2 = 0.0;
        for (unsigned int b = 0; b < B; ++b) s += a[2 * ((size_t)b * n_out + k)] / n;
        const double m = s / B;
        for (unsigned int b = 0; b < B; ++b) {
          const double d = a[2 * ((size_t)b * n_out + k)] / n - m;
          s2 += d * d;
        }
        e.mean[k] = m;
        e.error[k] = std::sqrt(s2 / ((double)B * (B - 1.0)));
      } else {
        const double m = a[2 * k] / n, var = n_calls > 1 ? std::max(0.0, (a[2 * k + 1] / n - m * m) * n / (n - 1.0)) : 0.0;
        e.mean[k] = m;
        e.error[k] = std::sqrt(var / n);
      }
    }
    return e;
  }
  /** the Creutz ratio chi(r, s), 1 <= r <= R(), 1 <= s <= S(), of the mean loops; batch >= 2: with the jackknife error over the chains */
  Ratio creutz(unsigned int r, unsigned int s) const {
    if (r < 1 || r > R_ || s < 1 || s > S_) fatal("WilsonLoops::creutz: loop outside 1 .. R x 1 .. S.");
    return creutz_jackknife(chain_means(), R_, S_, r, s);
  }
  /** the same arithmetic on per-chain means m [batch][R S] */
  static Ratio creutz_jackknife(const std::vector<std::vector<double>> &m, unsigned int R, unsigned int S, unsigned int r, unsigned int s) {
    const unsigned int B = (unsigned int)m.size(), n_out = R * S;
    std::vector<double> all(n_out, 0.0);
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_out; ++k) all[k] += m[b][k];
    std::vector<double> mean(all);
    for (double &v : mean) v /= B;
    Ratio res{creutz_ratio(mean, R, S, r, s), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B), leave(n_out);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        for (unsigned int k = 0; k < n_out; ++k) leave[k] = (all[k] - m[b][k]) / (B - 1.0);
        x[b] = creutz_ratio(leave, R, S, r, s);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      res.error = std::sqrt((B - 1.0) / B * s2);
    }
    return res;
  }

private:
  void launch(const std::shared_ptr<SampleState> phi, double *d_out, double *d_acc) {
    if (phi->size() != 2 * Mt_lat * Mx_lat) fatal("Evaluating WilsonLoops on state of wrong size.");
    if (!work || work_B != phi->batch()) {
      check(mlmcpi_schwinger_wilson_loops_workspace_bytes(Mt_lat, Mx_lat, R_, S_, phi->batch(), &work_bytes), "schwinger_wilson_loops_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    check(mlmcpi_schwinger_wilson_loops(phi->device(), Mt_lat, Mx_lat, phi->batch(), R_, S_, d_out, d_acc, work->p, work_bytes, nullptr),
          "schwinger_wilson_loops");
  }
  const unsigned int Mt_lat, Mx_lat, R_, S_, n_out_;
  unsigned int B = 0, work_B = 0, n_calls = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
  std::unique_ptr<DeviceVector> acc, out;
};

/** The momentum-projected slice correlators C_t(tau; q), C_x(tau; q), q < P, of a Gaussian free field state on a lattice, rotated
 *  or not (mlmcpi_gff_correlator; definitions in mlmcpi_hip.h).  Not a QoI: n_out() = P (Mt/2 + 1) + P (Mx/2 + 1) numbers per
 *  chain, C_t first, momentum-major, lag fastest.  accumulate() adds the sample's C and C^2 to per-chain sums on the device; the
 *  means, their errors and the energies E_q (the effective mass of correlator.hh) are host arithmetic on those sums. */
class GffCorrelator : public CorrelatorMeasurement {
public:
  struct Estimate {
    std::vector<double> mean, error;
    bool chain_spread;  // true: error = spread of the per-chain means (batch >= 2); false: the naive error of one chain
  };
  struct Energy {
    double value, error;
    bool has_error;  // the jackknife over chains needs batch >= 2
  };
  GffCorrelator(const std::shared_ptr<Lattice2D> lattice, unsigned int P_)
      : Mt_lat(lattice->getMt_lat()), Mx_lat(lattice->getMx_lat()), rotated(lattice->is_rotated() ? 1 : 0),
        n_vertices(lattice->getNvertices()), P_(P_), n_out_(P_ * (Mt_lat / 2 + 1) + P_ * (Mx_lat / 2 + 1)) {}
  unsigned int n_mom() const { return P_; }
  unsigned int n_out() const { return n_out_; }
  unsigned int Mt() const { return Mt_lat; }
  unsigned int Mx() const { return Mx_lat; }
  /** where C_d(tau; q) sits in a vector of n_out() entries (d = 0: t, 1: x) */
  static unsigned int index(unsigned int Mt, unsigned int Mx, unsigned int P, int d, unsigned int q, unsigned int tau) {
    const unsigned int nt = Mt / 2 + 1, nx = Mx / 2 + 1;
    return d == 0 ? q * nt + tau : P * nt + q * nx + tau;
  }
  unsigned int index(int d, unsigned int q, unsigned int tau) const { return index(Mt_lat, Mx_lat, P_, d, q, tau); }
  /** d_out[b][n_out()] = the correlators of chain b, enqueued on the default stream */
  void evaluate_device(const std::shared_ptr<SampleState> phi, double *d_out) { launch(phi, d_out, nullptr); }
  /** one more sample: its correlators are added to the per-chain sums (the batch is fixed by the first call) */
  void accumulate(const std::shared_ptr<SampleState> phi) override {
    if (!acc || B != phi->batch()) {
      if (n_calls) fatal("GffCorrelator::accumulate: the batch changed between samples.");
      B = phi->batch();
      acc = std::make_unique<DeviceVector>(2 * (size_t)B * n_out_);
      out = std::make_unique<DeviceVector>((size_t)B * n_out_);
    }
    launch(phi, (double *)out->ptr(), (double *)acc->ptr());
    ++n_calls;
  }
  unsigned int samples() const override { return n_calls; }
  unsigned int batch() const { return B; }
  /** per-chain means of C over the accumulated samples, [batch][n_out()] */
  std::vector<std::vector<double>> chain_means() const {
    if (!n_calls) fatal("GffCorrelator: no samples accumulated.");
    return chain_means_of(acc->download<double>(), B, n_out_, n_calls);
  }
  /** the same arithmetic on downloaded sums a [batch][n_out][2] (C, C^2) of n samples */
  static std::vector<std::vector<double>> chain_means_of(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    std::vector<std::vector<double>> m(B, std::vector<double>(n_out));
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < n_out; ++k) m[b][k] = a[2 * ((size_t)b * n_out + k)] / n_calls;
    return m;
  }
  /** mean and error per entry.  batch >= 2: the error is the spread of the per-chain means over sqrt(batch), so autocorrelation
   *  inside a chain cannot understate it; batch 1: the naive error of the samples (it ignores autocorrelation) */
  Estimate means_and_errors() const {
    if (!n_calls) fatal("GffCorrelator: no samples accumulated.");
    return estimate(acc->download<double>(), B, n_out_, n_calls);
  }
  /** the same arithmetic on downloaded sums a [batch][n_out][2] (C, C^2) of n samples */
  static Estimate estimate(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
    Estimate e{std::vector<double>(n_out, 0.0), std::vector<double>(n_out, 0.0), B >= 2};
    const double n = n_calls;
    for (unsigned int k = 0; k < n_out; ++k) {
      if (B >= 2) {
        double s = 0.0, s2 = 0.0;
        for (unsigned int b = 0; b < B; ++b) s += a[2 * ((size_t)b * n_out + k)] / n;
        const double m = s / B;
        for (unsigned int b = 0; b < B; ++b) {
          const double d = a[2 * ((size_t)b * n_out + k)] / n - m;
          s2 += d * d;
        }
        e.mean[k] = m;
        e.error[k] = std::sqrt(s2 / ((double)B * (B - 1.0)));
      } else {
        const double m = a[2 * k] / n, var = n_calls > 1 ? std::max(0.0, (a[2 * k + 1] / n - m * m) * n / (n - 1.0)) : 0.0;
        e.mean[k] = m;
        e.error[k] = std::sqrt(var / n);
      }
    }
    return e;
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
  /** the same arithmetic on per-chain means m [batch][n_out] */
  static Energy energy_jackknife(const std::vector<std::vector<double>> &m, unsigned int Mt, unsigned int Mx, unsigned int P, int d,
                                 unsigned int q, unsigned int tau) {
    const unsigned int B = (unsigned int)m.size(), nl = (d == 0 ? Mt : Mx) / 2 + 1, o = index(Mt, Mx, P, d, q, 0);
    std::vector<double> all(nl, 0.0);
    for (unsigned int b = 0; b < B; ++b)
      for (unsigned int k = 0; k < nl; ++k) all[k] += m[b][o + k];
    std::vector<double> mean(all);
    for (double &v : mean) v /= B;
    Energy r{effective_mass(mean, tau), 0.0, B >= 2};
    if (B >= 2) {
      std::vector<double> x(B), leave(nl);
      double xm = 0.0, s2 = 0.0;
      for (unsigned int b = 0; b < B; ++b) {
        for (unsigned int k = 0; k < nl; ++k) leave[k] = (all[k] - m[b][o + k]) / (B - 1.0);
        x[b] = effective_mass(leave, tau);
        xm += x[b] / B;
      }
      for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
      r.error = std::sqrt((B - 1.0) / B * s2);
    }
    return r;
  }

private:
  void launch(const std::shared_ptr<SampleState> phi, double *d_out, double *d_acc) {
    if (phi->size() != n_vertices) fatal("Evaluating GffCorrelator on state of wrong size.");
    if (!work || work_B != phi->batch()) {
      check(mlmcpi_gff_correlator_workspace_bytes(Mt_lat, Mx_lat, rotated, P_, phi->batch(), &work_bytes), "gff_correlator_workspace_bytes");
      work = std::make_unique<DeviceBuffer>(work_bytes);
      work_B = phi->batch();
    }
    check(mlmcpi_gff_correlator(Mt_lat, Mx_lat, rotated, P_, phi->device(), phi->batch(), d_out, d_acc, work->p, work_bytes, nullptr),
          "gff_correlator");
  }
  const unsigned int Mt_lat, Mx_lat;
  const int rotated;
  const unsigned int n_vertices, P_, n_out_;
  unsigned int B = 0, work_B = 0, n_calls = 0;
  size_t work_bytes = 0;
  std::unique_ptr<DeviceBuffer> work;
  std::unique_ptr<DeviceVector> acc, out;
};

}  // namespace mlmcpi
#endif
