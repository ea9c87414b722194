// chain_estimate.hh -- host arithmetic on the per-chain sums a [batch][n_out][2] (the sample's value and its square, summed over
// n_calls samples) that the correlator measurements of qoi.hh accumulate on the device: per-chain means, the mean over chains with
// its error, and the leave-one-chain-out jackknife of any scalar function of the mean vector.  Plain functions on std::vector; no
// device code, no ABI header (host/test_chain_estimate.cc runs them alone).
#ifndef MLMCPI_CHAIN_ESTIMATE_HH
#define MLMCPI_CHAIN_ESTIMATE_HH
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace mlmcpi {

struct ChainEstimate {
  std::vector<double> mean, error;
  bool chain_spread;  // true: error = spread of the per-chain means (batch >= 2); false: the naive error of one chain
};

struct ChainScalar {
  double value, error;
  bool has_error;  // the jackknife over chains needs batch >= 2
};

/** per-chain means over the n_calls samples, [B][n_out] */
inline std::vector<std::vector<double>> chain_means_of(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
  std::vector<std::vector<double>> m(B, std::vector<double>(n_out));
  for (unsigned int b = 0; b < B; ++b)
    for (unsigned int k = 0; k < n_out; ++k) m[b][k] = a[2 * ((size_t)b * n_out + k)] / n_calls;
  return m;
}

/** mean and error per entry.  B >= 2: the error is the spread of the per-chain means over sqrt(B), so autocorrelation inside a
 *  chain cannot understate it; B = 1: the naive error of the samples (it ignores autocorrelation; 0 for a single sample) */
inline ChainEstimate chain_estimate(const std::vector<double> &a, unsigned int B, unsigned int n_out, unsigned int n_calls) {
  ChainEstimate e{std::vector<double>(n_out, 0.0), std::vector<double>(n_out, 0.0), B >= 2};
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

/** f of the mean over chains of the per-chain means m [B][..]; B >= 2: with the jackknife error over the chains (f of the mean
 *  with one chain left out, chain by chain).  f is any double(const std::vector<double> &); it sees the entries first .. first +
 *  count - 1 of a chain as a vector of count entries (count = -1: all from first on). */
template <class F>
ChainScalar chain_jackknife(const std::vector<std::vector<double>> &m, F f, size_t first = 0, size_t count = (size_t)-1) {
  const unsigned int B = (unsigned int)m.size();
  if (count == (size_t)-1) count = B ? m[0].size() - first : 0;
  std::vector<double> all(count, 0.0);
  for (unsigned int b = 0; b < B; ++b)
    for (size_t k = 0; k < count; ++k) all[k] += m[b][first + k];
  std::vector<double> mean(all);
  for (double &v : mean) v /= B;
  ChainScalar r{f(mean), 0.0, B >= 2};
  if (B >= 2) {
    std::vector<double> x(B), leave(count);
    double xm = 0.0, s2 = 0.0;
    for (unsigned int b = 0; b < B; ++b) {
      for (size_t k = 0; k < count; ++k) leave[k] = (all[k] - m[b][first + k]) / (B - 1.0);
      x[b] = f(leave);
      xm += x[b] / B;
    }
    for (unsigned int b = 0; b < B; ++b) s2 += (x[b] - xm) * (x[b] - xm);
    r.error = std::sqrt((B - 1.0) / B * s2);
  }
  return r;
}

}  // namespace mlmcpi
#endif
