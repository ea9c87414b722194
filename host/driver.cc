// driver.cc -- counterpart of the reference's drivers (driver_qm.cc:98-429, driver_qft.cc:100-459) on device
// chains: builds lattice, action, QoI factory and sampler factory, runs MonteCarloSingleLevel::evaluate
// (method singlelevel) or MonteCarloMultiLevel::evaluate (method multilevel) and prints the statistics and, where
// the reference has one, the analytic value.  Parameters come from the command line (the reference's
// parameter-file parser is plumbing outside the hot path).
//   driver --action harmonicoscillator --M_lat 128 --T_final 4 --sampler hmc --n_samples 100000
//   driver --action schwinger --Mt_lat 16 --beta 1 --sampler heatbath --n_samples 20000
//   driver --method multilevel --action quarticoscillator --M_lat 256 --T_final 8 --sampler hierarchical --n_level 3 --epsilon 0.02
//   driver --method twolevel --action quarticoscillator --M_lat 256 --T_final 8 --coarsesampler hmc --n_samples 5000
//   driver --method multilevel --action schwinger --Mt_lat 16 --beta 2 --coarsening both --coarsesampler heatbath
//          --sampler hierarchical --n_level 2 --epsilon 0.005
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1 --sampler heatbath --n_samples 20000
//          (O(3) sigma model: heat-bath sampler; twolevel and hierarchical with --coarsening rotate, never multilevel: DESIGN.md 4.4a, 8)
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1 --coarsening rotate --method twolevel --coarsesampler heatbath
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1 --coarsening rotate --sampler hierarchical --coarsesampler heatbath --n_level 3
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1.5 --sampler wolff --n_updates 10 --n_samples 20000
//          (Wolff single-cluster updates over the four links per vertex; prints chi_m and the mean cluster size)
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1.5 --coarsening rotate --sampler hierarchical --coarsesampler levelwolff
//          --n_level 2 --n_updates 40
//          (the Wolff sampler on the coarsest level of a hierarchical or --method twolevel run, n_updates cluster updates per coarse
//           draw: the rotated level with --n_level 2, the unrotated M/2 level with --n_level 3)
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1.5 --sampler swendsenwang --n_updates 1 --n_samples 20000
//          (Swendsen-Wang multi-cluster updates; prints chi_m, its cluster-improved estimator and the clusters per update)
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1.5 --coarsening rotate --sampler hierarchical --coarsesampler levelsw
//          --n_level 2 --n_updates 4
//          (the Swendsen-Wang sampler on the coarsest level of a hierarchical or --method twolevel run, n_updates updates per coarse
//           draw: the rotated level with --n_level 2, the unrotated M/2 level with --n_level 3)
//   driver --action nonlinearsigma --Mt_lat 16 --beta 1.5 --sampler swendsenwang --n_updates 1 --batch 64 --n_samples 500 --correlator 1
//          (--correlator 1, single-level heatbath / wolff / swendsenwang runs: all `batch` chains are sampled, Q is their mean per
//           sample, and after the statistics come the time-slice correlators C_t, C_x per lag, chi and F from them, and the
//           second-moment correlation length xi_2 with its jackknife error over the chains)
//          (with --sampler swendsenwang the cluster-improved F, xi_2 and, per lag, C_t and C_x follow: DESIGN.md 4.6b)
//   driver --action harmonicoscillator --M_lat 16 --T_final 4 --sampler exact --batch 256 --n_samples 200 --path_correlator 9
//          (--path_correlator N, single-level runs of the three 1-D actions: all `batch` chains are sampled and after the statistics
//           come C(tau) = <x(0) x(tau)> (rotor: <cos(x(0) - x(tau))>) for tau < N, the effective mass per interior lag with its
//           jackknife error and the gap m_eff / a; for the harmonic oscillator the exact lattice values beside them)
//   driver --action schwinger --Mt_lat 8 --beta 2 --sampler heatbath --batch 256 --n_samples 200 --wilson_loops 3
//          (--wilson_loops N, single-level runs of the quenched Schwinger action: all `batch` chains are sampled and after the
//           statistics come the Wilson loops W(r, s), r, s <= N, beside the exact values of the periodic lattice, and the Creutz
//           ratios chi(r, r) with their jackknife error beside the string tension -log(I_1 / I_0))
//   driver --action gff --Mt_lat 8 --mass 4 --sampler exact --batch 256 --n_samples 100 --gff_correlator 3
//          (--gff_correlator P, single-level runs of the Gaussian free field with the exact, heatbath or hmc sampler: all `batch`
//           chains are sampled and after the statistics come the slice correlators C_t(tau; q), q < P, beside the exact law, the
//           energies E_q from the effective mass at tau <= Mt_lat / 4 with their jackknife error beside the lattice dispersion
//           relation, and the same along x)
//   driver --action rotor --M_lat 256 --T_final 25.6 --m0 0.25 --sampler cluster --n_updates 10 --n_samples 20000
//          (cluster samplers: rotor and schwinger; also --coarsesampler cluster for twolevel / hierarchical rotor runs)
//   driver --action nonlinearsigma --Mt_lat 8 --beta 1.2 --sampler heatbath --batch 64 --n_samples 200 --qoi topological
//          (--qoi magnetic|topological, nonlinearsigma only: chi_m, the default, or the topological susceptibility chi_t = Q^2 / n
//           of the geometric charge, in single-level, --method twolevel and --sampler hierarchical runs)
//   driver --action nonlinearsigma --Mt_lat 8 --beta 1.2 --sampler heatbath --batch 64 --n_samples 200 --qoi topological --n_cool 3
//          (--n_cool k with --qoi topological: chi_t is read from the field after k cooling sweeps, each level cooling its own
//           field, wherever --qoi topological runs; the chain's state is not touched)
//   driver --action nonlinearsigma --Mt_lat 8 --beta 1.2 --sampler heatbath --batch 64 --n_samples 200 --qoi topological --cooling_profile 0,1,3
//          (--cooling_profile d0,d1,.. with --qoi topological, --method singlelevel: after the run, per depth chi_t and <E> / 4 pi
//           of the cooled field with their jackknife error over the chains)
//   driver --action nonlinearsigma --Mt_lat 8 --beta 1.2 --sampler heatbath --batch 64 --n_samples 200 --qoi topological --flow_time 0.5 --flow_eps 0.05
//          (--flow_time t [--flow_eps e, default 0.05] with --qoi topological: chi_t is read from the field after t / e gradient-flow
//           steps of size e, each level flowing its own field to the same t, wherever --n_cool runs)
//   driver --action nonlinearsigma --Mt_lat 8 --beta 1.2 --sampler heatbath --batch 64 --n_samples 200 --qoi topological --flow_profile 0,0.25,1 --flow_scale 0.03
//          (--flow_profile t0,t1,.. with --qoi topological, --method singlelevel: after the run, per flow time chi_t, <E> / 4 pi and
//           t <E> / n with their jackknife error over the chains; with --flow_scale c the time at which t <E> / n = c)
//   driver --method throughput --action schwinger --Mt_lat 1024 --sampler heatbath --batch 32 --n_samples 20
//          (the sampling loop of MonteCarloSingleLevel on a batch of chains, statistics accumulated on the device:
//           prints link-updates/s of the C++ path)
// Several ranks (one process per GPU): start N copies with RANK / WORLD_SIZE / LOCAL_RANK set (torchrun, mpirun, a
// shell loop); they meet through RCCL (mlmcpi::RcclExchange, rendezvous file $MLMCPI_ID_FILE or
// /dev/shm/mlmcpi_id_<launcher pid>_$MASTER_PORT) and verify the group (RcclExchange::verify) or exit non-zero; rank r
// samples chain(s) r * batch ...
#include <unistd.h>

#include <chrono>
#include <cstring>
#include <map>
#include <set>

#include "mlmcpi/cluster_sampler.hh"
#include "mlmcpi/multilevel.hh"

using namespace mlmcpi;

/** the value v of --name, a count (0: off); anything but a non-negative integer is refused, before any device call */
static unsigned count_option(const std::string &name, const std::string &v, const char *counted) {
  if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos)
    fatal("--" + name + " takes a non-negative integer (" + counted + ", 0: off), not " + v);
  return (unsigned)std::stoul(v);
}

/** the first lines of a measurement's block: its title, then samples, chains, `more` and what its errors are */
static void measurement_header(const char *title, const CorrelatorMeasurement &m, const ChainEstimate &e, const std::string &more = "") {
  std::cout << std::endl << "=== " << title << " ===" << std::endl
            << " samples = " << m.samples() << ", chains = " << m.batch() << more << ", errors: "
            << (e.chain_spread ? "spread of the per-chain means" : "naive (one chain: autocorrelation ignored)") << std::endl;
}

/** what follows the value of a quantity derived from the mean over chains */
static void jackknife_suffix(const ChainScalar &s) {
  if (s.has_error) std::cout << " +/- " << s.error << " (jackknife over chains)";
  else std::cout << " (one chain: no jackknife error)";
}

int main(int argc, char **argv) {
  std::map<std::string, std::string> o = {{"action", "harmonicoscillator"}, {"M_lat", "128"}, {"T_final", "4.0"},
      {"Mt_lat", "16"}, {"m0", "1.0"}, {"mu2", "1.0"}, {"lambda", "1.0"}, {"x0", "1.0"}, {"beta", "1.0"}, {"mass", "10.0"},
      {"sampler", "hmc"}, {"nt", "100"}, {"dt", "0.1"}, {"n_burnin", "100"}, {"n_samples", "20000"}, {"n_sweep_overrelax", "10"},
      {"n_sweep_heatbath", "1"}, {"autotune", "1"}, {"window", "20"}, {"method", "singlelevel"}, {"n_level", "3"},
      {"epsilon", "0.01"}, {"coarsening", "both"}, {"coarsesampler", "hmc"}, {"renormalisation", "none"}, {"n_meas", "200"},
      {"batch", "1"}, {"seed", "2481317"}, {"warmup", "5"}, {"random_order", "0"}, {"n_updates", "10"}, {"correlator", "0"},
      {"path_correlator", "0"}, {"wilson_loops", "0"}, {"gff_correlator", "0"}, {"qoi", "magnetic"}, {"n_cool", "0"}, {"cooling_profile", ""},
      {"flow_time", "0"}, {"flow_eps", "0.05"}, {"flow_profile", ""}, {"flow_scale", ""}};
  std::set<std::string> given;  // the options on the command line
  for (int i = 1; i + 1 < argc; i += 2) {
    if (std::strncmp(argv[i], "--", 2) || !o.count(argv[i] + 2)) fatal(std::string("unknown option ") + argv[i]);
    o[argv[i] + 2] = argv[i + 1];
    given.insert(argv[i] + 2);
  }
  auto num = [&](const char *k) { return std::stod(o[k]); };
  // ranks: one process per GPU, the launcher's environment names them
  auto env_int = [](const char *k, int d) { const char *v = std::getenv(k); return v ? std::atoi(v) : d; };
  const int rank = env_int("RANK", 0), world = env_int("WORLD_SIZE", 1), local_rank = env_int("LOCAL_RANK", rank);
  const unsigned batch = (unsigned)num("batch");
  // --path_correlator N: the time correlator C(tau), tau = 0 .. N - 1, of a 1-D path action beside the QoI, and the energy gap from
  // its decay (qoi.hh PathCorrelator); 0: off.  Refused here, before any device call.
  const unsigned path_lags = count_option("path_correlator", o["path_correlator"], "the number of lags");
  if (path_lags > 0) {
    const std::string &pa = o["action"];
    if (pa != "harmonicoscillator" && pa != "quarticoscillator" && pa != "rotor")
      fatal("--path_correlator " + o["path_correlator"] + " is not supported for chosen action: the path correlator is built for "
            "harmonicoscillator, quarticoscillator and rotor only, not " + pa + " (the sigma model has --correlator 1)");
    if (o["method"] != "singlelevel")
      fatal("--path_correlator runs --method singlelevel only, not " + o["method"] + " (the two-level and multilevel estimators have "
            "no difference estimator for C(tau); the throughput loop measures the QoI alone)");
    if (world > 1) fatal("--path_correlator runs on one rank (its sums are not exchanged)");
    const unsigned M_lat = (unsigned)num("M_lat");
    if (path_lags > M_lat / 2 + 1)
      fatal("--path_correlator " + o["path_correlator"] + " is more than M_lat / 2 + 1 = " + std::to_string(M_lat / 2 + 1) +
            " lags (C(M_lat - tau) = C(tau))");
  }
  // --wilson_loops N: the Wilson loops W(r, s), r, s <= N, of the quenched Schwinger action beside the QoI, and the Creutz ratios
  // from them (qoi.hh WilsonLoops); 0: off.  Refused here, before any device call.
  const unsigned wilson_n = count_option("wilson_loops", o["wilson_loops"], "the largest loop side");
  if (wilson_n > 0) {
    if (o["action"] != "schwinger")
      fatal("--wilson_loops " + o["wilson_loops"] + " is not supported for chosen action: Wilson loops are built for schwinger only, not " +
            o["action"] + " (the sigma model has --correlator 1, the 1-D actions --path_correlator N)");
    if (o["method"] != "singlelevel")
      fatal("--wilson_loops runs --method singlelevel only, not " + o["method"] + " (the two-level and multilevel estimators have "
            "no difference estimator for W(r, s); the throughput loop measures the QoI alone)");
    if (o["sampler"] == "hierarchical")
      fatal("--wilson_loops takes a single-level sampler (hmc, heatbath or cluster), not hierarchical (Wilson loops are not built "
            "on coarsened levels)");
    if (world > 1) fatal("--wilson_loops runs on one rank (its sums are not exchanged)");
    const unsigned Mt_lat = (unsigned)num("Mt_lat"), cap = std::min(Mt_lat, (unsigned)MLMCPI_WILSON_LOOPS_MAX);
    if (wilson_n > cap)
      fatal("--wilson_loops " + o["wilson_loops"] + " is more than min(Mt_lat, Mx_lat, " + std::to_string(MLMCPI_WILSON_LOOPS_MAX) + ") = " +
            std::to_string(cap) + " links a side");
  }
  // --gff_correlator P: the slice correlators C_t(tau; q), C_x(tau; q), q < P, of the Gaussian free field beside the QoI, and the
  // energies E_q from their decay (qoi.hh GffCorrelator); 0: off.  Refused here, before any device call.
  const unsigned gff_mom = count_option("gff_correlator", o["gff_correlator"], "the number of momenta");
  if (gff_mom > 0) {
    if (o["action"] != "gff")
      fatal("--gff_correlator " + o["gff_correlator"] + " is not supported for chosen action: the momentum-projected correlator is built "
            "for gff only, not " + o["action"] + " (the sigma model has --correlator 1, the 1-D actions --path_correlator N, schwinger "
            "--wilson_loops N)");
    if (o["method"] != "singlelevel")
      fatal("--gff_correlator runs --method singlelevel only, not " + o["method"] + " (the two-level and multilevel estimators have "
            "no difference estimator for C(tau; q); the throughput loop measures the QoI alone)");
    if (o["sampler"] != "exact" && o["sampler"] != "heatbath" && o["sampler"] != "hmc")
      fatal("--gff_correlator takes a single-level sampler (exact, heatbath or hmc), not " + o["sampler"] + " (the exact law is that of "
            "the plain lattice, not of coarsened levels)");
    if (world > 1) fatal("--gff_correlator runs on one rank (its sums are not exchanged)");
    const unsigned Mt_lat = (unsigned)num("Mt_lat");
    if (Mt_lat < 2 || Mt_lat % 2) fatal("--gff_correlator needs an even Mt_lat >= 2, not " + o["Mt_lat"]);
    const unsigned cap = std::min(Mt_lat / 2 + 1, (unsigned)MLMCPI_GFF_CORRELATOR_MAX_MOMENTA);
    if (gff_mom > cap)
      fatal("--gff_correlator " + o["gff_correlator"] + " is more than min(Mt_lat / 2 + 1, " +
            std::to_string(MLMCPI_GFF_CORRELATOR_MAX_MOMENTA) + ") = " + std::to_string(cap) + " momenta");
  }
  // --qoi magnetic|topological: the QoI of the O(3) sigma model, chi_m (the default) or the topological susceptibility chi_t = Q^2 / n
  // of the geometric charge (qoi.hh QoI2DSigmaTopologicalSusceptibility), on every level of a single-level,
  // twolevel or hierarchical run.  Refused here, before any device call.
  if (o["qoi"] != "magnetic" && o["qoi"] != "topological") fatal("--qoi takes magnetic or topological, not " + o["qoi"]);
  const bool topological = o["qoi"] == "topological";
  if (topological && o["action"] != "nonlinearsigma")
    fatal("--qoi topological is not supported for chosen action: the geometric topological charge is built for nonlinearsigma only, "
          "not " + o["action"] + " (the rotor and schwinger measure their own topological susceptibility by default)");
  // --n_cool k: chi_t of the field after k cooling sweeps (qoi.hh QoI2DSigmaCooledTopologicalSusceptibility),
  // wherever --qoi topological runs.  --cooling_profile d0,d1,..: per depth chi_t and <E> / 4 pi after a single-level run
  // (qoi.hh SigmaCoolingProfile).  Both refused here, before any device call.
  const bool cooled = given.count("n_cool") != 0, wants_profile = given.count("cooling_profile") != 0;
  const unsigned n_cool = cooled ? count_option("n_cool", o["n_cool"], "the number of cooling sweeps") : 0u;
  std::vector<uint32_t> profile_depths;
  for (const char *flag : {"n_cool", "cooling_profile"}) {
    if (!given.count(flag)) continue;
    const std::string f = std::string("--") + flag;
    if (o["action"] != "nonlinearsigma")
      fatal(f + " " + o[flag] + " is not supported for chosen action: cooling is built for nonlinearsigma only, not " + o["action"]);
    if (!topological) fatal(f + " needs --qoi topological (cooling serves the topological charge), not --qoi " + o["qoi"]);
  }
  if (n_cool > MLMCPI_SIGMA_COOLING_MAX_DEPTH)
    fatal("--n_cool " + o["n_cool"] + " is more than " + std::to_string(MLMCPI_SIGMA_COOLING_MAX_DEPTH) + " cooling sweeps");
  if (wants_profile) {
    if (o["method"] != "singlelevel")
      fatal("--cooling_profile runs --method singlelevel only, not " + o["method"] + " (the two-level estimator takes --n_cool k)");
    if (o["correlator"] == "1") fatal("--cooling_profile and --correlator 1 do not run together (one measurement beside the QoI per run)");
    if (world > 1) fatal("--cooling_profile runs on one rank (its sums are not exchanged)");
    const std::string &v = o["cooling_profile"];
    if (v.empty() || v.find_first_not_of("0123456789,") != std::string::npos || v.front() == ',' || v.back() == ',' ||
        v.find(",,") != std::string::npos)
      fatal("--cooling_profile takes a comma-separated list of depths d0,d1,.., not " + v);
    for (size_t at = 0; at < v.size();) {
      const size_t end = std::min(v.find(',', at), v.size());
      if (end - at > 9) fatal("--cooling_profile takes depths up to " + std::to_string(MLMCPI_SIGMA_COOLING_MAX_DEPTH) + ", not " + v.substr(at, end - at));
      profile_depths.push_back((uint32_t)std::stoul(v.substr(at, end - at)));
      at = end + 1;
    }
    for (size_t k = 0; k < profile_depths.size(); ++k) {
      if (k && profile_depths[k] <= profile_depths[k - 1]) fatal("--cooling_profile takes strictly ascending depths, not " + v);
      if (profile_depths[k] > MLMCPI_SIGMA_COOLING_MAX_DEPTH)
        fatal("--cooling_profile takes depths up to " + std::to_string(MLMCPI_SIGMA_COOLING_MAX_DEPTH) + ", not " + std::to_string(profile_depths[k]));
    }
    if (profile_depths.size() > MLMCPI_SIGMA_COOLING_MAX_DEPTHS)
      fatal("--cooling_profile takes at most " + std::to_string(MLMCPI_SIGMA_COOLING_MAX_DEPTHS) + " depths, not " + std::to_string(profile_depths.size()));
  }
  // --flow_time t [--flow_eps e]: chi_t of the field after t / e gradient-flow steps (qoi.hh QoI2DSigmaFlowedTopologicalSusceptibility,
  // DESIGN.md 4.1h), wherever --n_cool runs.  --flow_profile t0,t1,.. [--flow_scale c]: per flow time chi_t, <E> / 4 pi and t <E> / n
  // after a single-level run (qoi.hh SigmaFlowProfile).  All refused here, before any device call.
  const bool flowed = given.count("flow_time") != 0, wants_flow_profile = given.count("flow_profile") != 0;
  double flow_eps = 0.05;
  unsigned flow_steps = 0;
  std::vector<uint32_t> flow_profile_steps;
  std::vector<double> flow_profile_times;
  double flow_scale_c = NAN;
  for (const char *flag : {"flow_time", "flow_eps", "flow_profile", "flow_scale"}) {
    if (!given.count(flag)) continue;
    const std::string f = std::string("--") + flag;
    if (o["action"] != "nonlinearsigma")
      fatal(f + " " + o[flag] + " is not supported for chosen action: the gradient flow is built for nonlinearsigma only, not " + o["action"]);
    if (!topological) fatal(f + " needs --qoi topological (the flow serves the topological charge), not --qoi " + o["qoi"]);
  }
  if (given.count("flow_eps") && !flowed && !wants_flow_profile) fatal("--flow_eps needs --flow_time t or --flow_profile t0,t1,..");
  if (given.count("flow_scale") && !wants_flow_profile) fatal("--flow_scale needs --flow_profile t0,t1,..");
  if (flowed && cooled) fatal("--flow_time and --n_cool do not run together (one smoothing of the field per QoI)");
  if (flowed || wants_flow_profile) {
    auto real = [&](const char *flag, const std::string &v, double &out) {
      char *end = nullptr;
      out = v.empty() ? NAN : std::strtod(v.c_str(), &end);
      return !v.empty() && end && *end == 0 && std::isfinite(out);
    };
    if (!real("flow_eps", o["flow_eps"], flow_eps) || !(flow_eps > 0.0 && flow_eps <= 0.25))
      fatal("--flow_eps takes a step size 0 < eps <= 0.25, not " + o["flow_eps"]);
    // t / eps must be an integer to 1e-9
    auto steps_of = [&](const std::string &flag, const std::string &v) {
      double t = 0.0;
      if (!real(flag.c_str(), v, t) || t < 0.0) fatal("--" + flag + " takes flow times t >= 0, not " + v);
      const double s = t / flow_eps, r = std::floor(s + 0.5);
      if (std::fabs(s - r) > 1e-9) fatal("--" + flag + " " + v + " is not a whole number of steps of --flow_eps " + o["flow_eps"]);
      if (r > MLMCPI_SIGMA_FLOW_MAX_STEPS)
        fatal("--" + flag + " " + v + " is more than " + std::to_string(MLMCPI_SIGMA_FLOW_MAX_STEPS) + " steps of --flow_eps " + o["flow_eps"]);
      return (uint32_t)r;
    };
    if (flowed) flow_steps = steps_of("flow_time", o["flow_time"]);
    if (wants_flow_profile) {
      if (o["method"] != "singlelevel")
        fatal("--flow_profile runs --method singlelevel only, not " + o["method"] + " (the two-level estimator takes --flow_time t)");
      if (o["correlator"] == "1") fatal("--flow_profile and --correlator 1 do not run together (one measurement beside the QoI per run)");
      if (wants_profile) fatal("--flow_profile and --cooling_profile do not run together (one measurement beside the QoI per run)");
      if (world > 1) fatal("--flow_profile runs on one rank (its sums are not exchanged)");
      const std::string &v = o["flow_profile"];
      if (v.empty() || v.find_first_not_of("0123456789.,eE+-") != std::string::npos || v.front() == ',' || v.back() == ',' ||
          v.find(",,") != std::string::npos)
        fatal("--flow_profile takes a comma-separated list of flow times t0,t1,.., not " + v);
      for (size_t at = 0; at < v.size();) {
        const size_t end = std::min(v.find(',', at), v.size());
        flow_profile_steps.push_back(steps_of("flow_profile", v.substr(at, end - at)));
        flow_profile_times.push_back(flow_profile_steps.back() * flow_eps);
        at = end + 1;
      }
      for (size_t k = 1; k < flow_profile_steps.size(); ++k)
        if (flow_profile_steps[k] <= flow_profile_steps[k - 1]) fatal("--flow_profile takes strictly ascending flow times, not " + v);
      if (flow_profile_steps.size() > MLMCPI_SIGMA_FLOW_MAX_TIMES)
        fatal("--flow_profile takes at most " + std::to_string(MLMCPI_SIGMA_FLOW_MAX_TIMES) + " flow times, not " + std::to_string(flow_profile_steps.size()));
      if (given.count("flow_scale") && !real("flow_scale", o["flow_scale"], flow_scale_c))
        fatal("--flow_scale takes the value c of t <E> / n that sets the scale, not " + o["flow_scale"]);
    }
  }
  std::shared_ptr<Exchange> exchange;
  if (world > 1) {
    check(mlmcpi_set_device(local_rank), "mlmcpi_set_device");
    const char *idf = std::getenv("MLMCPI_ID_FILE");
    // unique per launch: the launcher's pid (the ranks are its children) and its port; a file a dead run left behind is
    // rejected by mlmcpi_comm_init_file in any case (it names its writer)
    const std::string id_file = idf ? idf : std::string("/dev/shm/mlmcpi_id_") + std::to_string((long)getppid()) + "_" +
                                                (std::getenv("MASTER_PORT") ? std::getenv("MASTER_PORT") : "0");
    auto rccl = std::make_shared<RcclExchange>(rank, world, id_file, local_rank);
    rccl->verify(world);  // the communicator's own rank count and a sum over ranks, or message + exit(EXIT_FAILURE)
    exchange = rccl;
    if (rank != 0) std::cout.setstate(std::ios_base::failbit);  // mpi_parallel::cout: the master prints
  }
  std::shared_ptr<Action> action;
  std::shared_ptr<QoI> qoi;
  std::shared_ptr<SigmaCorrelator> correlator;
  std::shared_ptr<SigmaCoolingProfile> cooling_profile;
  std::shared_ptr<SigmaFlowProfile> flow_profile;
  std::shared_ptr<PathCorrelator> path_correlator;
  std::shared_ptr<WilsonLoops> wilson_loops;
  std::shared_ptr<GffCorrelator> gff_correlator;
  std::shared_ptr<QoIFactory> qoi_factory;
  std::shared_ptr<ConditionedFineActionFactory> cfa_factory;
  double analytic = NAN;
  const std::string a = o["action"];
  const RenormalisationType renorm = o["renormalisation"] == "perturbative" ? RenormalisationPerturbative
                                     : o["renormalisation"] == "exact"      ? RenormalisationNonperturbative
                                                                            : RenormalisationNone;
  const std::map<std::string, CoarseningType> coarsenings = {{"both", CoarsenBoth}, {"temporal", CoarsenTemporal},
      {"spatial", CoarsenSpatial}, {"alternate", CoarsenAlternate}, {"rotate", CoarsenRotate}};
  if (!coarsenings.count(o["coarsening"])) fatal("unknown coarsening " + o["coarsening"]);
  // --correlator 1: the time-slice correlators of the sigma model and xi_2 beside the QoI (qoi.hh SigmaCorrelator)
  if (o["correlator"] != "0" && o["correlator"] != "1") fatal("--correlator takes 0 or 1, not " + o["correlator"]);
  const bool wants_correlator = o["correlator"] == "1";
  if (wants_correlator && a != "nonlinearsigma")
    fatal(" --correlator 1 is not supported for chosen action: the time-slice correlator is built for nonlinearsigma only, not " + a);
  if (wants_correlator && o["method"] != "singlelevel")
    fatal("nonlinearsigma: --correlator 1 runs --method singlelevel only, not " + o["method"] + " (the two-level estimator has no "
          "difference estimator for C(tau); the throughput loop measures the QoI alone)");
  if (wants_correlator && o["sampler"] != "heatbath" && o["sampler"] != "wolff" && o["sampler"] != "swendsenwang")
    fatal("nonlinearsigma: --correlator 1 takes --sampler heatbath, wolff or swendsenwang, not " + o["sampler"]);
  if (wants_correlator && world > 1) fatal("nonlinearsigma: --correlator 1 runs on one rank (its sums are not exchanged)");
  // driver_qm.cc:62-70, driver_qft.cc:69-80: the cluster sampler exists for the rotor and the quenched Schwinger action
  const bool wants_cluster = o["sampler"] == "cluster" ||
                             (o["coarsesampler"] == "cluster" && (o["sampler"] == "hierarchical" || o["method"] == "twolevel"));
  if (wants_cluster && a == "nonlinearsigma")
    fatal(" cluster not supported for chosen action: nonlinearsigma needs the generic 2-D cluster update (connected components "
          "on the lattice), which is not built (DESIGN.md 8)");
  if (wants_cluster && a != "rotor" && a != "schwinger") fatal(" cluster not supported for chosen action.");
  // --sampler wolff: the Wolff single-cluster sampler of the sigma model (cluster_sampler.hh WolffClusterSampler)
  if (o["sampler"] == "wolff" && a != "nonlinearsigma")
    fatal(" wolff sampler not supported for chosen action: it is built for nonlinearsigma only (the rotor and schwinger have "
          "--sampler cluster; the other actions have no reflection the bond form is symmetric under)");
  if (o["sampler"] == "wolff" && o["method"] != "singlelevel")
    fatal("nonlinearsigma: --sampler wolff runs --method singlelevel only, not " + o["method"] + " (the two-level step of this action "
          "takes the heat-bath sampler on its coarse level, DESIGN.md 4.4a; the throughput loop is the heat-bath sampler's)");
  if (o["coarsesampler"] == "wolff")
    fatal(" --coarsesampler wolff is not supported: the wolff sampler is a single-level sampler of the nonlinear sigma model, "
          "whose hierarchical and two-level runs sample the coarse level with --coarsesampler heatbath (DESIGN.md 4.4a)");
  // --coarsesampler levelwolff: the same sampler on the coarsest level of a two-level or hierarchical sigma-model run, whichever
  // orientation that level has (mlmcpi_sigma_level_cluster_draw)
  if (o["sampler"] == "levelwolff")
    fatal(" --sampler levelwolff is not supported: levelwolff names the Wolff sampler as a coarse sampler (--coarsesampler levelwolff "
          "with --method twolevel or --sampler hierarchical); the single-level sampler is --sampler wolff");
  if (o["coarsesampler"] == "levelwolff") {
    if (a != "nonlinearsigma")
      fatal(" --coarsesampler levelwolff is not supported for chosen action: the Wolff cluster update is built for nonlinearsigma only "
            "(the rotor has --coarsesampler cluster)");
    if (o["method"] == "throughput" || (o["method"] != "twolevel" && o["sampler"] != "hierarchical"))
      fatal("nonlinearsigma: --coarsesampler levelwolff needs --method twolevel or --sampler hierarchical (and not --method throughput): "
            "with --method " + o["method"] + " --sampler " + o["sampler"] + " no coarse level is sampled; the single-level sampler is --sampler wolff");
    if (o["coarsening"] != "rotate")
      fatal("nonlinearsigma: --coarsesampler levelwolff needs --coarsening rotate, not " + o["coarsening"] +
            ": this action coarsens by rotate only (nonlinearsigmaaction.hh:143-149)");
  }
  // --sampler swendsenwang: the multi-cluster sampler of the sigma model (cluster_sampler.hh SwendsenWangSampler)
  if (o["sampler"] == "swendsenwang" && a != "nonlinearsigma")
    fatal(" swendsenwang sampler not supported for chosen action: it is built for nonlinearsigma only (the rotor and schwinger have "
          "--sampler cluster; the other actions have no reflection the bond form is symmetric under)");
  if (o["sampler"] == "swendsenwang" && o["method"] != "singlelevel")
    fatal("nonlinearsigma: --sampler swendsenwang runs --method singlelevel only, not " + o["method"] + " (the two-level step of this "
          "action takes the heat-bath sampler on its coarse level, DESIGN.md 4.4a; the throughput loop is the heat-bath sampler's)");
  if (o["coarsesampler"] == "swendsenwang")
    fatal(" --coarsesampler swendsenwang is not supported: the swendsenwang sampler is a single-level sampler of the nonlinear sigma "
          "model, whose hierarchical and two-level runs sample the coarse level with --coarsesampler heatbath (DESIGN.md 4.4a)");
  // --coarsesampler levelsw: the same sampler on the coarsest level of a two-level or hierarchical sigma-model run, whichever
  // orientation that level has (mlmcpi_sigma_level_sw_draw)
  if (o["sampler"] == "levelsw")
    fatal(" --sampler levelsw is not supported: levelsw names the Swendsen-Wang sampler as a coarse sampler (--coarsesampler levelsw "
          "with --method twolevel or --sampler hierarchical); the single-level sampler is --sampler swendsenwang");
  if (o["coarsesampler"] == "levelsw") {
    if (a != "nonlinearsigma")
      fatal(" --coarsesampler levelsw is not supported for chosen action: the Swendsen-Wang update is built for nonlinearsigma only "
            "(the rotor has --coarsesampler cluster)");
    if (o["method"] == "throughput" || (o["method"] != "twolevel" && o["sampler"] != "hierarchical"))
      fatal("nonlinearsigma: --coarsesampler levelsw needs --method twolevel or --sampler hierarchical (and not --method throughput): "
            "with --method " + o["method"] + " --sampler " + o["sampler"] + " no coarse level is sampled; the single-level sampler is --sampler swendsenwang");
    if (o["coarsening"] != "rotate")
      fatal("nonlinearsigma: --coarsesampler levelsw needs --coarsening rotate, not " + o["coarsening"] +
            ": this action coarsens by rotate only (nonlinearsigmaaction.hh:143-149)");
  }
  if (a == "harmonicoscillator" || a == "quarticoscillator" || a == "rotor") {
    auto lat = std::make_shared<Lattice1D>((unsigned)num("M_lat"), num("T_final"));
    if (a == "harmonicoscillator") {
      auto act = std::make_shared<HarmonicOscillatorAction>(lat, renorm, num("m0"), num("mu2"));
      analytic = act->Xsquared_analytical();
      action = act;
      qoi = std::make_shared<QoIXsquared>(lat);
      qoi_factory = std::make_shared<QoIXsquaredFactory>();
      cfa_factory = std::make_shared<GaussianConditionedFineActionFactory>();
    } else if (a == "quarticoscillator") {
      action = std::make_shared<QuarticOscillatorAction>(lat, renorm, num("m0"), num("mu2"), num("lambda"), num("x0"));
      qoi = std::make_shared<QoIXsquared>(lat);
      qoi_factory = std::make_shared<QoIXsquaredFactory>();
      cfa_factory = std::make_shared<GaussianConditionedFineActionFactory>();
    } else {
      action = std::make_shared<RotorAction>(lat, renorm, num("m0"));
      // RotorAction::chit_exact (rotoraction.cc:92-95) = Phi_chit(m0 / a, M) / m0 = [(M / kappa) Phi_chit(kappa, M)] / T_final
      check(mlmcpi_schwinger_chit_analytical(num("m0") / lat->geta_lat(), lat->getM_lat(), &analytic), "chit_analytical");
      analytic /= lat->getT_final();
      qoi = std::make_shared<QoISusceptibility>(lat);
      qoi_factory = std::make_shared<QoISusceptibilityFactory>();
      cfa_factory = std::make_shared<RotorConditionedFineActionFactory>();
    }
    if (path_lags > 0)
      path_correlator = std::make_shared<PathCorrelator>(lat, a == "harmonicoscillator" ? MLMCPI_HARMONIC : a == "quarticoscillator" ? MLMCPI_QUARTIC : MLMCPI_ROTOR, path_lags);
  } else if (a == "nonlinearsigma") {  // driver_qft.cc:159-166, 241-246
    auto lat = std::make_shared<Lattice2D>((unsigned)num("Mt_lat"), (unsigned)num("Mt_lat"), coarsenings.at(o["coarsening"]));
    if (o["sampler"] != "heatbath" && o["sampler"] != "wolff" && o["sampler"] != "swendsenwang" && o["sampler"] != "hierarchical")
      fatal("nonlinearsigma: only --sampler heatbath, --sampler wolff, --sampler swendsenwang and --sampler hierarchical are supported (HMC: the reference's force omits the sin theta of the measure "
            "in (theta, phi) coordinates and would sample the wrong law; DESIGN.md 8)");
    // driver_qft.cc:406-410: the reference refuses multilevel for this action; its two-level method and hierarchical sampler run
    if (o["method"] == "multilevel")
      fatal("nonlinearsigma: --method multilevel is not supported (the reference's driver refuses multilevel for this action, "
            "driver_qft.cc:406-410); --method twolevel and --sampler hierarchical run with --coarsening rotate");
    const bool levels = o["method"] == "twolevel" || o["sampler"] == "hierarchical";
    if (o["method"] != "singlelevel" && o["method"] != "throughput" && o["method"] != "twolevel")
      fatal("nonlinearsigma: --method " + o["method"] + " is not supported, only singlelevel, throughput and twolevel");
    if (levels && o["coarsening"] != "rotate")
      fatal("nonlinearsigma: " + std::string(o["method"] == "twolevel" ? "--method twolevel" : "--sampler hierarchical") +
            " needs --coarsening rotate, not " + o["coarsening"] + ": this action coarsens by rotate only (nonlinearsigmaaction.hh:143-149)");
    if (levels && o["coarsesampler"] != "heatbath" && o["coarsesampler"] != "levelwolff" && o["coarsesampler"] != "levelsw")
      fatal("nonlinearsigma: the coarse level of a twolevel or hierarchical run is sampled by --coarsesampler heatbath only, not " +
            o["coarsesampler"] + " (or by --coarsesampler levelwolff: Wolff cluster updates on that level; --coarsesampler levelsw is "
            "also allowed: Swendsen-Wang updates on that level)");
    if (o["renormalisation"] == "exact" && levels)
      fatal("nonlinearsigma: non-perturbative renormalisation not implemented for non-linear sigma model.");
    action = std::make_shared<NonlinearSigmaAction>(lat, nullptr, renorm, num("beta"));
    if (topological && cooled) {  // --n_cool 0 is the uncooled chi_t through the cooling call: the same bits
      qoi = std::make_shared<QoI2DSigmaCooledTopologicalSusceptibility>(lat, n_cool);
      qoi_factory = std::make_shared<QoI2DSigmaCooledTopologicalSusceptibilityFactory>(n_cool);
    } else if (topological && flowed) {  // --flow_time 0 is the uncooled chi_t through the flow call: the same bits
      qoi = std::make_shared<QoI2DSigmaFlowedTopologicalSusceptibility>(lat, flow_eps, flow_steps);
      qoi_factory = std::make_shared<QoI2DSigmaFlowedTopologicalSusceptibilityFactory>(flow_eps, flow_steps);
    } else if (topological) {
      qoi = std::make_shared<QoI2DSigmaTopologicalSusceptibility>(lat);
      qoi_factory = std::make_shared<QoI2DSigmaTopologicalSusceptibilityFactory>();
    } else {
      qoi = std::make_shared<QoI2DMagneticSusceptibility>(lat);
      qoi_factory = std::make_shared<QoI2DMagneticSusceptibilityFactory>();
    }
    if (wants_correlator) correlator = std::make_shared<SigmaCorrelator>(lat);
    if (wants_profile) cooling_profile = std::make_shared<SigmaCoolingProfile>(lat, profile_depths);
    if (wants_flow_profile) flow_profile = std::make_shared<SigmaFlowProfile>(lat, flow_eps, flow_profile_steps);
    cfa_factory = std::make_shared<NonlinearSigmaConditionedFineActionFactory>();
  } else if (a == "schwinger" || a == "gff") {
    auto lat = std::make_shared<Lattice2D>((unsigned)num("Mt_lat"), (unsigned)num("Mt_lat"), coarsenings.at(o["coarsening"]));
    if (a == "schwinger") {
      action = std::make_shared<QuenchedSchwingerAction>(lat, nullptr, renorm, num("beta"));
      qoi = std::make_shared<QoIAvgPlaquette>(lat);
      qoi_factory = std::make_shared<QoIAvgPlaquetteFactory>();
      cfa_factory = std::make_shared<QuenchedSchwingerConditionedFineActionFactory>();
      if (wilson_n > 0) wilson_loops = std::make_shared<WilsonLoops>(lat, wilson_n, wilson_n);
    } else {
      action = std::make_shared<GFFAction>(lat, nullptr, num("mass"));
      qoi = std::make_shared<QoI2DPhiSquared>(lat);
      if (gff_mom > 0) gff_correlator = std::make_shared<GffCorrelator>(lat, gff_mom);
      qoi_factory = std::make_shared<QoI2DPhiSquaredFactory>();           // driver_qft.cc:247-252
      cfa_factory = std::make_shared<GFFConditionedFineActionFactory>();  // driver_qft.cc:331-333 (use --coarsening rotate)
    }
  } else {
    fatal("unknown action " + a);
  }
  action->set_seed((uint64_t)num("seed"), (uint32_t)rank * batch);  // chain index = Philox counter word: distinct per rank
  std::cout << "Action: " << action->info_string() << std::endl;
  if (topological)
    std::cout << "QoI: topological susceptibility chi_t = Q^2 / n of the geometric (Berg-Luescher) charge" << std::endl;
  if (n_cool > 0) std::cout << "Cooling: chi_t is read after " << n_cool << " cooling sweeps of a copy of the field" << std::endl;
  if (flow_steps > 0)
    std::cout << "Gradient flow: chi_t is read at flow time " << flow_steps * flow_eps << " (" << flow_steps << " steps of " << flow_eps
              << ") of a copy of the field" << std::endl;
  auto basic_factory = [&](const std::string &name) -> std::shared_ptr<SamplerFactory> {
    if (name == "hmc") {
      HMCParameters hp;
      hp.nt = (unsigned)num("nt"); hp.dt = num("dt"); hp.n_burnin = (unsigned)num("n_burnin"); hp.autotune = num("autotune") != 0;
      hp.batch = batch;
      return std::make_shared<HMCSamplerFactory>(hp);
    }
    if (name == "exact") return std::make_shared<ExactSamplerFactory>(path_lags > 0 || gff_mom > 0 ? batch : 1u);  // driver_qm.cc: sampler = 'exact' (harmonic oscillator, GFF)
    if (name == "cluster") {  // driver_qm.cc:62-70, driver_qft.cc:69-80
      ClusterParameters cp;
      cp.n_burnin = (unsigned)num("n_burnin"); cp.n_updates = (unsigned)num("n_updates"); cp.batch = batch;
      return std::make_shared<ClusterSamplerFactory>(cp);
    }
    if (name == "wolff" || name == "levelwolff") {  // levelwolff: on whatever level the hierarchy hands it (checked above)
      ClusterParameters cp;
      cp.n_burnin = (unsigned)num("n_burnin"); cp.n_updates = (unsigned)num("n_updates"); cp.batch = batch;
      cp.improved = cp.structure = cp.correlator = name == "wolff" && wants_correlator;  // the single cluster's estimators
      return std::make_shared<WolffClusterSamplerFactory>(cp);
    }
    if (name == "swendsenwang" || name == "levelsw") {  // levelsw: on whatever level the hierarchy hands it (checked above)
      ClusterParameters cp;
      cp.n_burnin = (unsigned)num("n_burnin"); cp.n_updates = (unsigned)num("n_updates"); cp.batch = batch;
      cp.structure = name == "swendsenwang" && wants_correlator;  // xi_2 from cluster sums beside the plain one
      cp.correlator = cp.structure;                                // and the improved C(tau) they come from: one call per draw
      return std::make_shared<SwendsenWangSamplerFactory>(cp);
    }
    if (name != "heatbath") fatal("unknown sampler " + name);
    OverrelaxedHeatBathParameters hb;
    hb.n_sweep_overrelax = (unsigned)num("n_sweep_overrelax"); hb.n_sweep_heatbath = (unsigned)num("n_sweep_heatbath");
    hb.n_burnin = (unsigned)num("n_burnin");
    hb.batch = batch;
    // heatbath.random_order of the reference's parameter file (template: true).  Default here: 0, the multicolour kernels.
    // 2: random order as well, drawn on the device and run in parallel rounds (2-D actions).
    hb.random_order = num("random_order") != 0;
    hb.random_order_mode = num("random_order") == 2 ? 1 : 0;
    if (hb.random_order_mode == 1) {
      if (a != "schwinger" && a != "gff" && a != "nonlinearsigma")
        fatal("--random_order 2: the parallel random order is built for the 2-D actions (schwinger, gff, nonlinearsigma), not " + a);
      std::cerr << "heatbath: random_order = true (device order per chain and sweep, parallel rounds, one launch per draw)" << std::endl;
    } else
    std::cerr << "heatbath: random_order = " << (hb.random_order ? "true (shuffled index set, site-at-a-time updates)"
                                                                 : "false (multicolour sweep kernels)") << std::endl;
    return std::make_shared<OverrelaxedHeatBathSamplerFactory>(hb);
  };
  std::shared_ptr<SamplerFactory> factory;
  if (o["sampler"] == "hierarchical") {  // driver_qm.cc:61-75: hierarchical sampler over `coarsesampler`
    if (!cfa_factory) fatal("no conditioned fine action for action " + a);
    HierarchicalParameters hier;
    hier.n_max_level = (unsigned)num("n_level"); hier.n_meas = (unsigned)num("n_meas");
    factory = std::make_shared<HierarchicalSamplerFactory>(basic_factory(o["coarsesampler"]), cfa_factory, hier);
  } else {
    factory = basic_factory(o["sampler"]);
  }
  if (o["method"] == "multilevel") {  // driver_qm.cc:340-398
    if (!cfa_factory || !qoi_factory) fatal("multilevel method is not available for action " + a);
    MultiLevelMCParameters mlp;
    mlp.n_level = (unsigned)num("n_level"); mlp.n_burnin = (unsigned)num("n_burnin"); mlp.epsilon = num("epsilon");
    mlp.n_autocorr_window = (unsigned)num("window"); mlp.n_meas = (unsigned)num("n_meas");
    if (world > 1) {  // level l on rank l % world (multilevel.hh), one all-reduce of the level table per pass
      mlp.level_rank = (unsigned)rank;
      mlp.level_ranks = (unsigned)world;
    }
    MonteCarloMultiLevel mlmc(action, qoi_factory, factory, cfa_factory, mlp);
    if (exchange) mlmc.set_exchange(std::make_shared<LevelExchangeOver>(exchange));
    mlmc.evaluate();
    std::cout << std::endl << "=== Multilevel MC ===" << std::endl;
    mlmc.show_statistics();
    if (!std::isnan(analytic))
      std::cout << std::setprecision(6) << " analytic result = " << analytic << std::endl
                << " |analytic - numerical| / error = " << std::fabs(analytic - mlmc.numerical_result()) / mlmc.statistical_error()
                << std::endl;
    return 0;
  }
  if (o["method"] == "twolevel") {  // driver_qm.cc:313-338
    if (!cfa_factory || !qoi_factory) fatal("twolevel method is not available for action " + a);
    TwoLevelMCParameters tp;
    tp.n_burnin = (unsigned)num("n_burnin"); tp.n_samples = (unsigned)num("n_samples"); tp.n_meas = (unsigned)num("n_meas");
    tp.n_autocorr_window = (unsigned)num("window");
    if (topological) tp.batch = batch;  // --qoi topological: every state holds the samplers' `batch` chains, Q is their mean
    MonteCarloTwoLevel two(action, qoi_factory, basic_factory(o["coarsesampler"]), cfa_factory, tp);
    two.evaluate_difference();
    std::cout << std::endl << "=== Two level MC ===" << std::endl;
    two.show_statistics();
    return 0;
  }
  if (o["method"] == "throughput") {
    // The loop of montecarlosinglelevel.cc:59-77 over `batch` chains with nothing on the host per sample: draw (no copy:
    // the sampler lends its buffer), QoI into device memory, per-chain moments accumulated on the device.
    std::shared_ptr<Sampler> sampler = factory->get(action);
    auto phi_state = std::make_shared<SampleState>(action->sample_size(), batch);
    DeviceVector q(batch), acc(5 * (size_t)batch);
    const unsigned n_samples = (unsigned)num("n_samples"), warmup = (unsigned)num("warmup");
    auto sweeper = std::dynamic_pointer_cast<OverrelaxedHeatBathSampler>(sampler);
    const int fused = sweeper ? qoi->fused_kind() : 0;
    auto one = [&]() {  // draw + QoI + record_sample as one call where the sampler can; else the three steps
      if (fused && sweeper->draw_with_qoi(phi_state, fused, (double *)q.ptr(), (double *)acc.ptr())) return;
      sampler->draw(phi_state);
      qoi->evaluate_device(phi_state, (double *)q.ptr());
      check(mlmcpi_stats_accumulate((double *)acc.ptr(), (const double *)q.ptr(), batch, nullptr), "stats_accumulate");
    };
    for (unsigned i = 0; i < warmup; ++i) one();
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned i = 0; i < n_samples; ++i) one();
    check(mlmcpi_stream_synchronize(nullptr), "sync");
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const std::vector<double> m = acc.download<double>();
    double n = 0, s1 = 0;
    for (unsigned b = 0; b < batch; ++b) { n += m[5 * b]; s1 += m[5 * b + 1]; }
    std::vector<double> tot = {n, s1, el};
    if (exchange) {  // sum of counts and of QoI sums; the slowest rank's time
      std::vector<double> times(world, 0.0);
      times[rank] = el;
      tot.insert(tot.end(), times.begin(), times.end());
      exchange->allreduce_sum(tot.data(), tot.size());
      tot[2] = 0;
      for (int r = 0; r < world; ++r) tot[2] = std::max(tot[2], tot[3 + r]);
    }
    const double sweeps = num("n_sweep_overrelax") + num("n_sweep_heatbath");
    const bool sweeping = o["sampler"] == "heatbath";
    // updated units per sweep: state entries (links, vertices); vertices for the sigma model (one update moves both angles)
    const double per_sweep = a == "nonlinearsigma" ? 0.5 * action->sample_size() : (double)action->sample_size();
    double units = sweeping ? per_sweep * sweeps : (double)action->sample_size() * (num("nt") + 1);
    std::string unit_name = sweeping ? "site updates per draw" : "force evaluations per draw";
    if (auto rotor_cluster = std::dynamic_pointer_cast<ClusterSampler>(sampler)) {  // what a draw moved: flipped sites
      units = rotor_cluster->mean_cluster_size() * num("n_updates");
      unit_name = "flipped sites per draw (measured mean)";
    } else if (o["sampler"] == "cluster") {  // Schwinger: every draw rewrites the whole link field
      units = (double)action->sample_size();
      unit_name = "state entries written per draw";
    }
    std::cout << std::setprecision(6) << "{\"driver\": \"host/driver (C++ Sampler::draw + QoI::evaluate_device + stats_accumulate)\", "
              << "\"units\": \"" << unit_name << "\", \"units_per_draw\": " << units << ", "
              << "\"ranks\": " << (exchange ? exchange->size() : 1) << ", \"batch\": " << batch << ", \"samples\": " << n_samples
              << ", \"ms_per_sample\": " << 1e3 * tot[2] / n_samples << ", \"updates_per_s\": " << std::scientific
              << units * batch * world * n_samples / tot[2] << std::fixed << ", \"qoi_mean\": " << tot[1] / tot[0] << "}" << std::endl;
    return 0;
  }
  if (o["method"] != "singlelevel") fatal("unknown method " + o["method"]);
  SingleLevelMCParameters mp;
  mp.n_burnin = (unsigned)num("n_burnin"); mp.n_samples = (unsigned)num("n_samples"); mp.n_autocorr_window = (unsigned)num("window");
  // with --correlator 1 the loop runs on all `batch` chains (Q = their mean per sample) and measures C(tau) on the same states
  // (--path_correlator N likewise)
  std::shared_ptr<CorrelatorMeasurement> measured = correlator;
  if (path_correlator) measured = path_correlator;
  if (wilson_loops) measured = wilson_loops;  // --wilson_loops N likewise
  if (gff_correlator) measured = gff_correlator;  // and --gff_correlator P
  if (cooling_profile) measured = cooling_profile;  // and --cooling_profile d0,d1,..
  if (flow_profile) measured = flow_profile;        // and --flow_profile t0,t1,..
  // (--qoi topological likewise: Q is the mean of chi_t over the chains)
  MonteCarloSingleLevel mc(action, qoi, factory, mp, exchange, measured || topological ? batch : 1u, measured);
  mc.evaluate();
  std::cout << std::endl << "=== Single level MC ===" << std::endl;
  mc.show_statistics();
  mc.get_sampler()->show_stats();
  if (cooling_profile) {
    const SigmaCoolingProfile::Estimate e = cooling_profile->means_and_errors();
    const std::vector<uint32_t> &depths = cooling_profile->get_depths();
    measurement_header("Cooling profile", *cooling_profile, e);
    std::cout << std::setprecision(8) << std::scientific;
    for (unsigned k = 0; k < depths.size(); ++k) {
      const ChainScalar chi = cooling_profile->entry(k), en = cooling_profile->entry((unsigned)depths.size() + k);
      std::cout << " depth " << depths[k] << ": chi_t = " << chi.value;
      jackknife_suffix(chi);
      std::cout << ", <E> / 4 pi = " << en.value;
      jackknife_suffix(en);
      std::cout << std::endl;
    }
  }
  if (flow_profile) {
    const SigmaFlowProfile::Estimate e = flow_profile->means_and_errors();
    const unsigned nt = (unsigned)flow_profile->get_steps().size();
    measurement_header("Flow profile", *flow_profile, e, ", eps = " + o["flow_eps"]);
    std::cout << std::setprecision(8) << std::scientific;
    for (unsigned k = 0; k < nt; ++k) {
      const ChainScalar chi = flow_profile->entry(k), en = flow_profile->entry(nt + k), te = flow_profile->t_energy(k);
      std::cout << " t " << flow_profile->time(k) << " (step " << flow_profile->get_steps()[k] << "): chi_t = " << chi.value;
      jackknife_suffix(chi);
      std::cout << ", <E> / 4 pi = " << en.value;
      jackknife_suffix(en);
      std::cout << ", t <E> / n = " << te.value;
      jackknife_suffix(te);
      std::cout << std::endl;
    }
    if (given.count("flow_scale")) {
      const ChainScalar sc = flow_profile->scale(flow_scale_c);
      std::cout << " flow scale: t <E> / n = " << flow_scale_c << " at t = " << sc.value;
      if (std::isnan(sc.value)) std::cout << " (the listed flow times do not bracket it)";
      else jackknife_suffix(sc);
      std::cout << std::endl;
    }
  }
  if (correlator) {
    const SigmaCorrelator::Estimate e = correlator->means_and_errors();
    const unsigned Mt = correlator->Mt(), Mx = correlator->Mx(), nt = Mt / 2 + 1, nx = Mx / 2 + 1, B = correlator->batch();
    const std::vector<double> Ct = correlator->direction(e.mean, 0), Cx = correlator->direction(e.mean, 1);
    const std::vector<double> Et = correlator->direction(e.error, 0), Ex = correlator->direction(e.error, 1);
    std::vector<double> avg_err(nt, 0.0);  // of (C_t + C_x) / 2 where Mt = Mx: chain spread again, else the mean of the two naive errors
    if (Mt == Mx) {
      const std::vector<std::vector<double>> m = correlator->chain_means();
      for (unsigned tau = 0; tau < nt; ++tau) {
        if (B < 2) { avg_err[tau] = 0.5 * (Et[tau] + Ex[tau]); continue; }
        double s2 = 0.0;
        for (unsigned b = 0; b < B; ++b) {
          const double d = 0.5 * (m[b][tau] + m[b][nt + tau]) - 0.5 * (Ct[tau] + Cx[tau]);
          s2 += d * d;
        }
        avg_err[tau] = std::sqrt(s2 / ((double)B * (B - 1.0)));
      }
    }
    measurement_header("Time-slice correlator", *correlator, e);
    std::cout << std::setprecision(6) << std::fixed;
    for (unsigned tau = 0; tau < std::max(nt, nx); ++tau) {
      std::cout << " C(tau = " << tau << "):";
      if (tau < nt) std::cout << " C_t = " << Ct[tau] << " +/- " << Et[tau];
      if (tau < nx) std::cout << " C_x = " << Cx[tau] << " +/- " << Ex[tau];
      if (Mt == Mx) std::cout << " avg = " << 0.5 * (Ct[tau] + Cx[tau]) << " +/- " << avg_err[tau];
      std::cout << std::endl;
    }
    std::cout << " chi from C_t = " << correlator_susceptibility(Ct, Mt) << ", from C_x = " << correlator_susceptibility(Cx, Mx) << std::endl
              << " F_t = " << structure_factor(Ct, Mt) << ", F_x = " << structure_factor(Cx, Mx) << std::endl;
    for (int d = 0; d < 2; ++d) {
      const SigmaCorrelator::Xi xi = correlator->xi(d);
      std::cout << " xi_2 (" << (d ? "x" : "t") << ") = " << xi.value;
      jackknife_suffix(xi);
      std::cout << ", xi_2 / M = " << xi.value / (d ? Mx : Mt) << std::endl;
    }
    // --sampler swendsenwang or wolff: the same two numbers from the cluster sums of the updates (the field BEFORE each update);
    // the Wolff sampler's improved chi_m first (the Swendsen-Wang sampler prints its own with its statistics)
    const auto sw = std::dynamic_pointer_cast<SwendsenWangSampler>(mc.get_sampler());
    const auto wolff = std::dynamic_pointer_cast<WolffClusterSampler>(mc.get_sampler());
    if (wolff && wolff->has_improved())
      std::cout << " improved chi_m = " << wolff->improved_mean() << " +/- " << wolff->improved_error() << std::endl;
    if ((sw && sw->has_structure()) || (wolff && wolff->has_structure())) {
      for (int d = 0; d < 2; ++d) {
        const ClusterImprovedSums::Estimate F = sw ? sw->improved_structure_factor(d) : wolff->improved_structure_factor(d);
        std::cout << " improved F (" << (d ? "x" : "t") << ") = " << F.value << " +/- " << F.error << std::endl;
      }
      for (int d = 0; d < 2; ++d) {
        const ClusterImprovedSums::Estimate xi = sw ? sw->improved_xi(d) : wolff->improved_xi(d);
        std::cout << " improved xi_2 (" << (d ? "x" : "t") << ") = " << xi.value << " +/- " << xi.error
                  << ", xi_2 / M = " << xi.value / (d ? Mx : Mt) << std::endl;
      }
    }
    // and the cluster-improved correlators themselves, per lag, in the format of the plain block
    if ((sw && sw->has_correlator()) || (wolff && wolff->has_correlator())) {
      const ClusterImprovedSums::CorrelatorEstimate ie = sw ? sw->improved_correlator() : wolff->improved_correlator();
      const std::vector<double> It = correlator->direction(ie.mean, 0), Ix = correlator->direction(ie.mean, 1);
      const std::vector<double> IEt = correlator->direction(ie.error, 0), IEx = correlator->direction(ie.error, 1);
      for (unsigned tau = 0; tau < std::max(nt, nx); ++tau) {
        std::cout << " improved C(tau = " << tau << "):";
        if (tau < nt) std::cout << " improved C_t = " << It[tau] << " +/- " << IEt[tau];
        if (tau < nx) std::cout << " improved C_x = " << Ix[tau] << " +/- " << IEx[tau];
        std::cout << std::endl;
      }
    }
  }
  if (!std::isnan(analytic)) {  // driver_qm.cc:411-425
    auto st = mc.get_statistics();
    std::cout << std::setprecision(6) << " analytic result = " << analytic << std::endl
              << " |analytic - numerical| / error = " << std::fabs(analytic - st->average()) / st->error() << std::endl;
  }
  if (path_correlator) {
    const PathCorrelator::Estimate e = path_correlator->means_and_errors();
    const unsigned M_lat = path_correlator->M();
    const double T_final = num("T_final"), a_lat = T_final / M_lat;
    const bool ho = a == "harmonicoscillator";
    measurement_header("Path correlator", *path_correlator, e);
    std::cout << std::setprecision(8) << std::fixed;
    for (unsigned tau = 0; tau < path_lags; ++tau) {
      std::cout << " C(tau = " << tau << ") = " << e.mean[tau] << " +/- " << e.error[tau];
      if (ho) std::cout << " exact = " << path_correlator_ho_exact(M_lat, T_final, num("m0"), num("mu2"), tau);
      std::cout << std::endl;
    }
    for (unsigned tau = 1; tau + 1 < path_lags; ++tau) {
      const PathCorrelator::Mass m = path_correlator->effective_mass(tau);
      std::cout << " m_eff(tau = " << tau << ") = " << m.value;
      jackknife_suffix(m);
      std::cout << ", Delta E = m_eff / a = " << m.value / a_lat << std::endl;
    }
    if (ho) {
      const double w = path_ho_lattice_omega(M_lat, T_final, num("mu2"));
      std::cout << " exact lattice gap: omega~ = " << w << ", omega~ / a = " << w / a_lat << std::endl;
    }
  }
  if (wilson_loops) {
    const WilsonLoops::Estimate e = wilson_loops->means_and_errors();
    const unsigned Mt = wilson_loops->Mt(), Mx = wilson_loops->Mx();
    const double beta = num("beta");
    measurement_header("Wilson loops", *wilson_loops, e);
    std::cout << std::setprecision(8) << std::fixed;
    for (unsigned r = 1; r <= wilson_n; ++r)
      for (unsigned s = 1; s <= wilson_n; ++s)
        std::cout << " W(r = " << r << ", s = " << s << ") = " << e.mean[(r - 1) * wilson_n + s - 1] << " +/- "
                  << e.error[(r - 1) * wilson_n + s - 1] << " exact = " << wilson_loop_exact(beta, Mt, Mx, r, s) << std::endl;
    for (unsigned r = 1; r <= wilson_n; ++r) {
      const WilsonLoops::Ratio c = wilson_loops->creutz(r, r);
      std::cout << " chi(r = " << r << ", s = " << r << ") = " << c.value;
      jackknife_suffix(c);
      std::cout << std::endl;
    }
    std::cout << " exact string tension: -log(I_1(beta) / I_0(beta)) = " << string_tension_exact(beta) << std::endl;
  }
  if (gff_correlator) {
    const GffCorrelator::Estimate e = gff_correlator->means_and_errors();
    const unsigned Mt = gff_correlator->Mt(), Mx = gff_correlator->Mx();
    const double mass = num("mass");
    measurement_header("GFF correlator", *gff_correlator, e, ", momenta = " + std::to_string(gff_mom));
    std::cout << std::setprecision(8) << std::fixed;
    // the exact law along x is that along t with the extents exchanged, mu^2 = (mass / Mt)^2 kept: the mass argument rescaled
    auto correlators = [&](int d) {
      const unsigned M = d ? Mx : Mt, Mo = d ? Mt : Mx;
      for (unsigned q = 0; q < gff_mom; ++q)
        for (unsigned tau = 0; tau <= M / 2; ++tau) {
          const unsigned k = gff_correlator->index(d, q, tau);
          std::cout << " C_" << (d ? "x" : "t") << "(tau = " << tau << "; q = " << q << ") = " << e.mean[k] << " +/- " << e.error[k]
                    << " exact = " << gff_correlator_exact(M, Mo, mass * M / Mt, q, tau) << std::endl;
        }
    };
    auto energies = [&](int d) {
      const unsigned M = d ? Mx : Mt, Mo = d ? Mt : Mx;
      for (unsigned q = 0; q < gff_mom; ++q)
        for (unsigned tau = 1; tau <= M / 4; ++tau) {
          const GffCorrelator::Energy en = gff_correlator->energy(d, q, tau);
          std::cout << " E_" << (d ? "x" : "t") << "(q = " << q << "; tau = " << tau << ") = " << en.value;
          jackknife_suffix(en);
          std::cout << " exact = " << gff_dispersion_exact(M, Mo, mass * M / Mt, q) << std::endl;
        }
    };
    correlators(0);
    std::cout << "=== GFF energies (effective mass of C_t) ===" << std::endl;
    energies(0);
    std::cout << "=== GFF correlator along x ===" << std::endl;
    correlators(1);
    energies(1);
  }
  return 0;
}
