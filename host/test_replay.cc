// test_replay.cc -- the C++ host samplers (include/mlmcpi/*.hh) pinned, draw by draw, to the raw ABI calls they stand for.
//   test_replay CASE     CASE = samplestate | heatbath_sweeps | heatbath_random | hmc | exact_and_cluster | twolevel |
//                               hierarchical | mlmc_table
// Every case has two sides.  The OBJECT side drives a host class through its public interface.  The REPLAY side issues the
// mlmcpi_* calls of mlmcpi_hip.h on its own mlmcpi_malloc buffers, with the seeds and counters of the contract written in the
// headers ("the host layer's counter contract"): no SampleState, no sampler, no action class, only the
// mlmcpi_*_action / mlmcpi_sigma_level structs.  Same call, same arguments, same bits: after every draw the two states are
// compared with memcmp.  The only tolerances in this file: FUSED_QOI_TOL, the one tests/test_gpu_parity.py uses for the same
// pair (a QoI summed inside a fused launch against the stand-alone QoI kernel), and the 1 ulp of the two doubles of mlmc_table.
// Exit code 0 and a last line "all checks passed" = every check of the case held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <limits>
#include <numeric>
#include <utility>

#include "mlmcpi/cluster_sampler.hh"
#include "mlmcpi/multilevel.hh"

using namespace mlmcpi;

static int failures = 0;
#define EXPECT(cond, ...)                                \
  do {                                                   \
    if (!(cond)) {                                       \
      ++failures;                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);   \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
    }                                                    \
  } while (0)

// tests/test_gpu_parity.py: test_fused_qoi_equals_separate_evaluation (kind 1) and
// test_draw_qoi_record_in_one_call_equals_the_three_steps: |fused - separate| <= 1e-12 max(1, max |separate|)
static const double FUSED_QOI_TOL = 1e-12;

static const uint64_t SEED = 90210771ull;  // not an action's default: a class that ignored set_seed would show
static const uint32_t CHAIN0 = 5;
static const uint64_t EXACT_XOR = 0x45584143ull;  // sampler.hh: the exact samplers' key

typedef std::vector<double> Vec;

/** a raw device buffer of the replay side, zeroed */
struct Dev {
  explicit Dev(size_t bytes_) : bytes(bytes_ ? bytes_ : 8) {
    check(mlmcpi_malloc(&p, bytes), "mlmcpi_malloc");
    check(mlmcpi_memset(p, 0, bytes, nullptr), "mlmcpi_memset");
  }
  ~Dev() { mlmcpi_free(p); }
  Dev(const Dev &) = delete;
  Dev &operator=(const Dev &) = delete;
  double *d() const { return (double *)p; }
  template <class T>
  std::vector<T> get() const {
    std::vector<T> h(bytes / sizeof(T));
    check(mlmcpi_copy_d2h(h.data(), p, h.size() * sizeof(T), nullptr), "copy_d2h");
    return h;
  }
  template <class T>
  void put(const std::vector<T> &h) {
    if (h.size() * sizeof(T) > bytes) fatal("Dev::put: too large");
    check(mlmcpi_copy_h2d(p, h.data(), h.size() * sizeof(T), nullptr), "copy_h2d");
  }
  void zero() { check(mlmcpi_memset(p, 0, bytes, nullptr), "mlmcpi_memset"); }
  void *p = nullptr;
  const size_t bytes;
};

/** what a state's device buffer holds now (pending host writes uploaded first, as any kernel would see it) */
static Vec dev_of(const std::shared_ptr<SampleState> &s) {
  Vec h((size_t)s->size() * s->batch());
  check(mlmcpi_copy_d2h(h.data(), s->device(), h.size() * sizeof(double), nullptr), "copy_d2h");
  return h;
}
/** what host code reads through data[j] */
static Vec host_of(const std::shared_ptr<SampleState> &s) {
  const SampleState::Data &d = s->data;
  return Vec(d.data(), d.data() + d.size());
}
/** equal doubles, where 0 / 0 on both sides (no draw counted yet) is equal too */
static bool eq(double a, double b) { return a == b || (std::isnan(a) && std::isnan(b)); }
static bool same(const Vec &a, const Vec &b) { return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(double)); }
static long first_diff(const Vec &a, const Vec &b) {
  if (a.size() != b.size()) return -2;
  for (size_t j = 0; j < a.size(); ++j)
    if (std::memcmp(&a[j], &b[j], sizeof(double))) return (long)j;
  return -1;
}
#define EXPECT_SAME(a, b, ...)                                                        \
  do {                                                                                \
    const Vec a__ = (a), b__ = (b);                                                   \
    if (!same(a__, b__)) {                                                            \
      ++failures;                                                                     \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);                                \
      std::printf(__VA_ARGS__);                                                       \
      const long j__ = first_diff(a__, b__);                                          \
      if (j__ >= 0) std::printf(": entry %ld: %.17g vs %.17g", j__, a__[j__], b__[j__]); \
      else std::printf(": sizes %zu vs %zu", a__.size(), b__.size());                 \
      std::printf("\n");                                                              \
    }                                                                                 \
  } while (0)

/** a known state: values in (0.1, 0.9), valid for every action here (angles, polar angles, fields) */
static Vec known_state(size_t n, double shift = 0.0) {
  Vec v(n);
  for (size_t l = 0; l < n; ++l) v[l] = 0.5 + 0.4 * std::sin(1.0 + l + shift);
  return v;
}
static void write_host(const std::shared_ptr<SampleState> &s, const Vec &v) {
  std::memcpy(s->data.data(), v.data(), v.size() * sizeof(double));
}
static bool within_fused_tol(const Vec &got, const Vec &want) {
  double scale = 1.0, err = 0.0;
  for (size_t j = 0; j < want.size(); ++j) {
    scale = std::fmax(scale, std::fabs(want[j]));
    err = std::fmax(err, std::fabs(got[j] - want[j]));
  }
  return got.size() == want.size() && err <= FUSED_QOI_TOL * scale;
}

// =====================================================================================================================
// 1. samplestate: value semantics against a std::vector<double> model
// =====================================================================================================================
static void case_samplestate() {
  const unsigned M = 6, B = 2, N = M * B;
  const Vec va = known_state(N, 0), vb = known_state(N, 100), vc = known_state(N, 200);
  auto fresh = [&](const Vec &v) {
    auto s = std::make_shared<SampleState>(M, B);
    write_host(s, v);
    return s;
  };
  {  // a host write through data[j] on a shared state does not reach the other holder
    auto a = fresh(va), b = std::make_shared<SampleState>(M, B);
    b->share(*a);
    EXPECT(a->device_shared() && b->device_shared(), "share: both holders must report a shared buffer");
    Vec mb = va;  // the model of b
    b->data[3] = 42.0;
    mb[3] = 42.0;
    EXPECT_SAME(dev_of(a), va, "host write on a shared state reached the other holder (device)");
    EXPECT_SAME(host_of(a), va, "host write on a shared state reached the other holder (host)");
    EXPECT_SAME(dev_of(b), mb, "host write on a shared state lost");
    EXPECT(!a->device_shared() && !b->device_shared(), "after the write was uploaded nobody shares a buffer");
    // ... and the same the other way round: the lender writes
    auto c = std::make_shared<SampleState>(M, B);
    c->share(*a);
    a->data[0] = -7.0;
    Vec ma = va;
    ma[0] = -7.0;
    EXPECT_SAME(dev_of(c), va, "host write of the lender reached the borrower");
    EXPECT_SAME(dev_of(a), ma, "host write of the lender lost");
  }
  {  // device_mutable() on a shared buffer detaches; the other holder keeps its values
    auto a = fresh(va), b = std::make_shared<SampleState>(M, B);
    b->share(*a);
    double *p = b->device_mutable();
    EXPECT(!a->device_shared() && !b->device_shared(), "device_mutable on a shared buffer must detach");
    EXPECT_SAME(dev_of(b), va, "device_mutable must keep the values");
    check(mlmcpi_memset(p, 0, N * sizeof(double), nullptr), "mlmcpi_memset");
    EXPECT_SAME(dev_of(a), va, "a kernel writing through device_mutable() reached the other holder");
    EXPECT_SAME(host_of(b), Vec(N, 0.0), "the write through device_mutable() is not visible in its own state");
  }
  {  // device_overwrite() on a shared buffer leaves the other holder intact
    auto a = fresh(va), b = std::make_shared<SampleState>(M, B);
    b->share(*a);
    double *p = b->device_overwrite();
    check(mlmcpi_copy_h2d(p, vb.data(), N * sizeof(double), nullptr), "copy_h2d");
    EXPECT_SAME(dev_of(a), va, "device_overwrite on a shared buffer reached the other holder");
    EXPECT_SAME(host_of(b), vb, "device_overwrite: the new content is not what the state reads");
    EXPECT(!a->device_shared() && !b->device_shared(), "device_overwrite on a shared buffer must drop it");
  }
  {  // share after a pending host write on `other`
    auto a = fresh(va), b = std::make_shared<SampleState>(M, B), c = std::make_shared<SampleState>(M, B);
    c->share(*a);     // a's buffer is lent out ...
    a->data[1] = 3.5;  // ... and a has a host write pending
    Vec ma = va;
    ma[1] = 3.5;
    b->share(*a);
    EXPECT_SAME(dev_of(b), ma, "share after a pending host write: the borrower misses the write");
    EXPECT_SAME(dev_of(c), va, "share after a pending host write: the earlier borrower changed");
    EXPECT_SAME(dev_of(a), ma, "share after a pending host write: the lender lost it");
  }
  {  // adopt
    auto a = fresh(va), b = fresh(vb);
    std::shared_ptr<DeviceBuffer> buf = a->buffer();
    b->adopt(buf);
    EXPECT_SAME(host_of(b), va, "adopt: the state does not read the adopted buffer");
    buf.reset();
    EXPECT(a->device_shared() && b->device_shared(), "adopt: two holders");
    b->data[2] = 9.0;
    Vec mb = va;
    mb[2] = 9.0;
    EXPECT_SAME(dev_of(a), va, "write after adopt reached the first holder");
    EXPECT_SAME(dev_of(b), mb, "write after adopt lost");
  }
  {  // swap_device when one side is shared with a third state
    auto a = fresh(va), b = fresh(vb), c = std::make_shared<SampleState>(M, B);
    c->share(*a);
    a->swap_device(*b);
    EXPECT_SAME(dev_of(a), vb, "swap_device: a");
    EXPECT_SAME(dev_of(b), va, "swap_device: b");
    EXPECT_SAME(dev_of(c), va, "swap_device: the third holder changed");
    check(mlmcpi_memset(b->device_mutable(), 0, N * sizeof(double), nullptr), "mlmcpi_memset");  // b now shares with c
    EXPECT_SAME(dev_of(c), va, "swap_device, then a kernel on the swapped side: the third holder changed");
    EXPECT_SAME(dev_of(b), Vec(N, 0.0), "swap_device, then a kernel on the swapped side: lost");
    EXPECT_SAME(host_of(a), vb, "swap_device: a read through the host");
  }
  {  // a->data = b->data, then a write to b, leaves a alone (device-valid and host-valid sources)
    auto a = fresh(va), b = fresh(vb);
    (void)b->device();
    a->data = b->data;  // device to device
    b->data[4] = 1.25;
    EXPECT_SAME(dev_of(a), vb, "assignment then a host write to the source changed the copy");
    check(mlmcpi_memset(b->device_mutable(), 0, N * sizeof(double), nullptr), "mlmcpi_memset");
    EXPECT_SAME(host_of(a), vb, "assignment then a kernel on the source changed the copy");
    auto c = fresh(vc), d = std::make_shared<SampleState>(M, B);
    d->data = c->data;  // host to host (c's write is still pending)
    c->data[0] = 77.0;
    EXPECT_SAME(dev_of(d), vc, "host assignment then a write to the source changed the copy");
    // assignment INTO a state whose buffer is lent out must not reach the borrower
    auto e = fresh(va), f = std::make_shared<SampleState>(M, B);
    f->share(*e);
    (void)c->device();
    e->data = c->data;
    Vec mc = vc;
    mc[0] = 77.0;
    EXPECT_SAME(dev_of(f), va, "assignment into a lent-out state reached the borrower");
    EXPECT_SAME(dev_of(e), mc, "assignment into a lent-out state lost");
  }
  {  // device_shared() is true exactly when two states hold the buffer
    auto a = fresh(va);
    EXPECT(!a->device_shared(), "a fresh state shares nothing");
    {
      auto b = std::make_shared<SampleState>(M, B);
      b->share(*a);
      EXPECT(a->device_shared() && b->device_shared(), "two holders");
    }
    EXPECT(!a->device_shared(), "the borrower is gone: one holder");
  }
}

// =====================================================================================================================
// 2. / 3. OverrelaxedHeatBathSampler
// =====================================================================================================================
typedef std::function<void(double *x, double *scratch, unsigned n_or, unsigned n_hb, uint32_t sweep0)> DrawFn;

struct SweepSetup {
  std::string name;
  unsigned M = 0, B = 3, n_or = 2, n_hb = 1;
  int qoi_kind = 0;
  bool random_order = false;
  unsigned random_order_mode = 0;
  std::function<std::shared_ptr<Action>()> make_action;  // object side
  std::function<void(double *)> init;                     // replay: *_initialise(SEED, CHAIN0)
  std::function<DrawFn()> make_draw;                      // replay: one draw = one ABI call (a fresh one per chain of draws)
  std::function<void(const double *, double *)> qoi;      // replay: the stand-alone QoI kernel
};
static const unsigned N_BURNIN = 2;

struct SweepReplay {
  explicit SweepReplay(const SweepSetup &c_) : c(c_), x((size_t)c_.M * c_.B * sizeof(double)), scratch(x.bytes), fn(c_.make_draw()) {
    c.init(x.d());
    for (unsigned i = 0; i < N_BURNIN; ++i) draw();  // the constructor's burn-in draws count
  }
  Vec draw() { return draw(c.n_or, c.n_hb); }
  Vec draw(unsigned n_or, unsigned n_hb) {
    fn(x.d(), scratch.d(), n_or, n_hb, sweep_counter);
    sweep_counter += n_or + n_hb;
    return x.get<double>();
  }
  const SweepSetup &c;
  Dev x, scratch;
  DrawFn fn;
  uint32_t sweep_counter = 0;
};

static std::shared_ptr<OverrelaxedHeatBathSampler> make_sweep_sampler(const SweepSetup &c) {
  std::shared_ptr<Action> act = c.make_action();
  act->set_seed(SEED, CHAIN0);
  OverrelaxedHeatBathParameters p;
  p.n_sweep_heatbath = c.n_hb;
  p.n_sweep_overrelax = c.n_or;
  p.n_burnin = N_BURNIN;
  p.random_order = c.random_order;
  p.random_order_mode = c.random_order_mode;
  p.batch = c.B;
  return std::make_shared<OverrelaxedHeatBathSampler>(act, p);
}

/** (a) the same SampleState passed to every draw */
static void pattern_a(const SweepSetup &c, bool check_pool) {
  auto sampler = make_sweep_sampler(c);
  SweepReplay replay(c);
  auto s = std::make_shared<SampleState>(c.M, c.B);
  for (int k = 0; k < 8; ++k) {
    sampler->draw(s);
    EXPECT_SAME(dev_of(s), replay.draw(), "%s (a) draw %d", c.name.c_str(), k);
    EXPECT(sampler->accepted(), "%s (a): every sample is accepted", c.name.c_str());
  }
  EXPECT(sampler->p_accept() == 1.0, "%s (a): p_accept = %g", c.name.c_str(), sampler->p_accept());
  if (check_pool) EXPECT(sampler->pool_size() <= 3, "%s (a): pool of %zu buffers after 8 draws, the class promises three", c.name.c_str(), sampler->pool_size());
}
/** (b) a fresh SampleState per draw, all kept: no later draw may change a sample handed out earlier */
static void pattern_b(const SweepSetup &c) {
  auto sampler = make_sweep_sampler(c);
  SweepReplay replay(c);
  std::vector<std::shared_ptr<SampleState>> kept;
  std::vector<Vec> want;
  for (int k = 0; k < 7; ++k) {
    kept.push_back(std::make_shared<SampleState>(c.M, c.B));
    sampler->draw(kept.back());
    want.push_back(replay.draw());
    EXPECT_SAME(dev_of(kept.back()), want.back(), "%s (b) draw %d", c.name.c_str(), k);
  }
  for (int k = 0; k < 7; ++k) EXPECT_SAME(dev_of(kept[k]), want[k], "%s (b): the sample of draw %d changed after it was handed out", c.name.c_str(), k);
}
/** (c) the caller writes into the state it received: the sampler's chain must not notice, the caller must keep its write */
static void pattern_c(const SweepSetup &c) {
  for (int how = 0; how < 2; ++how) {
    auto sampler = make_sweep_sampler(c);
    SweepReplay replay(c);
    auto s = std::make_shared<SampleState>(c.M, c.B);
    Vec mine;
    for (int k = 0; k < 6; ++k) {
      sampler->draw(s);
      const Vec want = replay.draw();
      EXPECT_SAME(dev_of(s), want, "%s (c%d) draw %d", c.name.c_str(), how, k);
      EXPECT_SAME(dev_of(sampler->current_state()), want, "%s (c%d) current state after draw %d", c.name.c_str(), how, k);
      if (k == 2) {
        mine = want;
        if (how == 0) {
          s->data[0] = 0.125;
          mine[0] = 0.125;
        } else {
          check(mlmcpi_memset(s->device_mutable(), 0, s->bytes(), nullptr), "mlmcpi_memset");
          mine.assign(mine.size(), 0.0);
        }
        EXPECT_SAME(host_of(s), mine, "%s (c%d): the caller's write is not visible in its own state", c.name.c_str(), how);
        EXPECT_SAME(dev_of(s), mine, "%s (c%d): the caller's write is not visible on the device", c.name.c_str(), how);
        EXPECT_SAME(dev_of(sampler->current_state()), want, "%s (c%d): the caller's write reached the sampler's state", c.name.c_str(), how);
      }
    }
  }
}
/** (d) set_state(x), then draws: the replay's sweeps from x at the current counter */
static void pattern_d(const SweepSetup &c) {
  auto sampler = make_sweep_sampler(c);
  SweepReplay replay(c);
  auto s = std::make_shared<SampleState>(c.M, c.B);
  sampler->draw(s);
  EXPECT_SAME(dev_of(s), replay.draw(), "%s (d) draw before set_state", c.name.c_str());
  const Vec x = known_state((size_t)c.M * c.B);
  auto xs = std::make_shared<SampleState>(c.M, c.B);
  write_host(xs, x);
  sampler->set_state(xs);
  replay.x.put(x);
  for (int k = 0; k < 3; ++k) {
    sampler->draw(s);
    EXPECT_SAME(dev_of(s), replay.draw(), "%s (d) draw %d after set_state", c.name.c_str(), k);
  }
  EXPECT_SAME(dev_of(xs), x, "%s (d): the state handed to set_state changed", c.name.c_str());
}
/** (e) draw_with_qoi */
static void pattern_e(const SweepSetup &c) {
  const unsigned B = c.B;
  {
    auto sampler = make_sweep_sampler(c);
    SweepReplay replay(c);
    auto s = std::make_shared<SampleState>(c.M, B);
    Dev d_q(B * sizeof(double)), d_acc(5 * B * sizeof(double)), r_q(B * sizeof(double)), r_acc(5 * B * sizeof(double)), r_sep(B * sizeof(double));
    for (int k = 0; k < 5; ++k) {
      const bool with_acc = k != 2;  // one draw without the moments
      const bool ok = sampler->draw_with_qoi(s, c.qoi_kind, d_q.d(), with_acc ? d_acc.d() : nullptr);
      EXPECT(ok, "%s (e) draw %d: draw_with_qoi refused", c.name.c_str(), k);
      if (!ok) return;
      const Vec want = replay.draw();
      EXPECT_SAME(dev_of(s), want, "%s (e) draw %d", c.name.c_str(), k);
      c.qoi(replay.x.d(), r_sep.d());
      const Vec q = d_q.get<double>(), q_sep = r_sep.get<double>();
      EXPECT(within_fused_tol(q, q_sep), "%s (e) draw %d: fused QoI %.17g vs separate %.17g (chain 0)", c.name.c_str(), k, q[0], q_sep[0]);
      if (with_acc) {
        r_q.put(q);
        check(mlmcpi_stats_accumulate(r_acc.d(), r_q.d(), B, nullptr), "stats_accumulate");
      }
      EXPECT_SAME(d_acc.get<double>(), r_acc.get<double>(), "%s (e) draw %d: moments", c.name.c_str(), k);
    }
    EXPECT(sampler->p_accept() == 1.0, "%s (e): p_accept", c.name.c_str());
  }
  // refused: no heat-bath sweep at the end, and random order; state, counters and statistics untouched
  for (int why = 0; why < 2; ++why) {
    SweepSetup r = c;
    if (why == 0) r.n_hb = 0;
    else {
      r.random_order = true;
      r.random_order_mode = 0;
    }
    auto sampler = make_sweep_sampler(r);
    auto s = std::make_shared<SampleState>(c.M, B);
    const Vec marker = known_state((size_t)c.M * B, 7);
    write_host(s, marker);
    Dev d_q(B * sizeof(double)), d_acc(5 * B * sizeof(double));
    const Vec sentinel(B, 7.0), acc0(5 * B, 3.0);
    d_q.put(sentinel);
    d_acc.put(acc0);
    const Vec before = dev_of(sampler->current_state());
    const bool ok = sampler->draw_with_qoi(s, c.qoi_kind, d_q.d(), d_acc.d());
    EXPECT(!ok, "%s (e) refusal %d: draw_with_qoi must return false", c.name.c_str(), why);
    EXPECT_SAME(dev_of(sampler->current_state()), before, "%s (e) refusal %d: the chain moved", c.name.c_str(), why);
    EXPECT_SAME(dev_of(s), marker, "%s (e) refusal %d: the caller's state changed", c.name.c_str(), why);
    EXPECT_SAME(d_q.get<double>(), sentinel, "%s (e) refusal %d: d_q written", c.name.c_str(), why);
    EXPECT_SAME(d_acc.get<double>(), acc0, "%s (e) refusal %d: d_acc written", c.name.c_str(), why);
    EXPECT(std::isnan(sampler->p_accept()), "%s (e) refusal %d: statistics counted a draw (p_accept = %g)", c.name.c_str(), why, sampler->p_accept());
    if (why == 0) {  // the counter did not move: the next plain draw is the replay's draw at the same counter
      SweepReplay replay(r);
      sampler->draw(s);
      EXPECT_SAME(dev_of(s), replay.draw(), "%s (e) refusal: the draw after it", c.name.c_str());
    }
  }
}

static mlmcpi_lattice_action lattice_abi(int kind, unsigned Mt, unsigned Mx, double beta, double mass) {
  mlmcpi_lattice_action a;
  a.kind = kind; a.Mt = Mt; a.Mx = Mx; a.beta = beta; a.mass = mass;
  return a;
}
static mlmcpi_path_action path_abi(int kind, unsigned M, double T, double m0, double mu2) {
  mlmcpi_path_action a;
  a.kind = kind; a.M = M; a.T_final = T; a.m0 = m0; a.mu2 = mu2; a.lambda = 0; a.x0 = 0;
  return a;
}

/** a 2-D action under OverrelaxedHeatBathSampler; order: 0 fixed, 1 random mode 1 (device order), 2 random mode 0 (host shuffle) */
static SweepSetup lattice_setup(const std::string &name, int kind, unsigned Mt, unsigned Mx, double beta, double mass, unsigned B,
                                unsigned n_or, unsigned n_hb, int order) {
  SweepSetup c;
  const mlmcpi_lattice_action act = lattice_abi(kind, Mt, Mx, beta, mass);
  c.name = name;
  c.M = (kind == MLMCPI_GFF ? 1 : 2) * Mt * Mx;
  c.B = B; c.n_or = n_or; c.n_hb = n_hb;
  c.random_order = order != 0;
  c.random_order_mode = order == 1 ? 1 : 0;
  c.qoi_kind = kind == MLMCPI_SCHWINGER ? 1 : kind == MLMCPI_GFF ? 3 : 4;
  c.make_action = [=]() -> std::shared_ptr<Action> {
    if (kind == MLMCPI_SCHWINGER) return std::make_shared<QuenchedSchwingerAction>(std::make_shared<Lattice2D>(Mt, Mx, CoarsenBoth), nullptr, RenormalisationNone, beta);
    if (kind == MLMCPI_GFF) return std::make_shared<GFFAction>(std::make_shared<Lattice2D>(Mt, Mx, CoarsenBoth), nullptr, mass);
    return std::make_shared<NonlinearSigmaAction>(std::make_shared<Lattice2D>(Mt, Mx, CoarsenRotate), nullptr, RenormalisationNone, beta);
  };
  c.init = [=](double *x) { check(mlmcpi_lattice_initialise(&act, x, B, SEED, CHAIN0, nullptr), "lattice_initialise"); };
  const unsigned M = c.M;
  if (order == 0)
    c.make_draw = [=]() -> DrawFn {
      return [=](double *x, double *scratch, unsigned nor, unsigned nhb, uint32_t sweep0) {
        check(mlmcpi_lattice_sweep_draw(&act, x, scratch, B, nor, nhb, SEED, CHAIN0, sweep0, 0, nullptr), "lattice_sweep_draw");
      };
    };
  else if (order == 1)
    c.make_draw = [=]() -> DrawFn {
      size_t bytes = 0;
      check(mlmcpi_lattice_random_sweep_workspace_bytes(&act, B, &bytes), "random_sweep_workspace_bytes");
      auto work = std::make_shared<Dev>(bytes);
      return [=](double *x, double *, unsigned nor, unsigned nhb, uint32_t sweep0) {
        check(mlmcpi_lattice_random_sweep_draw(&act, x, B, nor, nhb, SEED, CHAIN0, sweep0, work->p, nullptr), "lattice_random_sweep_draw");
      };
    };
  else
    c.make_draw = [=]() -> DrawFn {
      // overrelaxedheatbathsampler.hh:110-116 as the class does it: the index set (sigma model: the vertices; else every entry),
      // shuffled before every sweep by ONE engine that lives as long as the sampler
      const unsigned n = kind == MLMCPI_NONLINEAR_SIGMA ? M / 2 : M;
      auto index = std::make_shared<std::vector<unsigned int>>(n);
      std::iota(index->begin(), index->end(), 0u);
      auto engine = std::make_shared<std::mt19937_64>(871417);
      auto d_index = std::make_shared<Dev>(n * sizeof(uint32_t));
      return [=](double *x, double *, unsigned nor, unsigned nhb, uint32_t sweep0) {
        for (unsigned s = 0; s < nor + nhb; ++s) {
          std::shuffle(index->begin(), index->end(), *engine);
          d_index->put(*index);
          check(mlmcpi_lattice_site_updates(&act, x, B, (const uint32_t *)d_index->p, n, 0, s >= nor ? 1 : 0, SEED, CHAIN0, sweep0 + s, nullptr), "lattice_site_updates");
        }
      };
    };
  c.qoi = [=](const double *x, double *out) {
    if (kind == MLMCPI_SCHWINGER) check(mlmcpi_qoi_avg_plaquette(x, Mt, Mx, B, out, nullptr), "qoi_avg_plaquette");
    else if (kind == MLMCPI_GFF) check(mlmcpi_qoi_phi_squared(x, Mt * Mx, B, out, nullptr), "qoi_phi_squared");
    else check(mlmcpi_qoi_magnetic_susceptibility(x, Mt, Mx, B, out, nullptr), "qoi_magnetic_susceptibility");
  };
  return c;
}

static SweepSetup rotor_setup(const std::string &name, unsigned M, unsigned B, unsigned n_or, unsigned n_hb, bool shuffled) {
  SweepSetup c;
  const double T = 4.0, m0 = 0.25;
  const mlmcpi_path_action act = path_abi(MLMCPI_ROTOR, M, T, m0, 0.0);
  c.name = name;
  c.M = M; c.B = B; c.n_or = n_or; c.n_hb = n_hb;
  c.random_order = shuffled;
  c.random_order_mode = 0;
  c.qoi_kind = 4;
  c.make_action = [=]() -> std::shared_ptr<Action> { return std::make_shared<RotorAction>(std::make_shared<Lattice1D>(M, T), RenormalisationNone, m0); };
  c.init = [=](double *x) { check(mlmcpi_path_initialise(&act, x, B, SEED, CHAIN0, nullptr), "path_initialise"); };
  if (!shuffled)
    c.make_draw = [=]() -> DrawFn {
      return [=](double *x, double *scratch, unsigned nor, unsigned nhb, uint32_t sweep0) {
        check(mlmcpi_path_sweep_draw(&act, x, scratch, B, nor, nhb, SEED, CHAIN0, sweep0, nullptr), "path_sweep_draw");
      };
    };
  else
    c.make_draw = [=]() -> DrawFn {
      auto index = std::make_shared<std::vector<unsigned int>>(M);
      std::iota(index->begin(), index->end(), 0u);
      auto engine = std::make_shared<std::mt19937_64>(871417);
      auto d_index = std::make_shared<Dev>(M * sizeof(uint32_t));
      return [=](double *x, double *, unsigned nor, unsigned nhb, uint32_t sweep0) {
        for (unsigned s = 0; s < nor + nhb; ++s) {
          std::shuffle(index->begin(), index->end(), *engine);
          d_index->put(*index);
          check(mlmcpi_path_site_updates(&act, x, B, (const uint32_t *)d_index->p, M, 0, s >= nor ? 1 : 0, SEED, CHAIN0, sweep0 + s, nullptr), "path_site_updates");
        }
      };
    };
  c.qoi = [=](const double *x, double *out) { check(mlmcpi_qoi_susceptibility(x, M, T, B, out, nullptr), "qoi_susceptibility"); };
  return c;
}

static void case_heatbath_sweeps() {
  const std::vector<SweepSetup> setups = {
      lattice_setup("schwinger 16x16", MLMCPI_SCHWINGER, 16, 16, 1.0, 0.0, 3, 2, 1, 0),
      // the smallest lattice where the planner takes the last overrelaxation launch and the heat bath in one launch
      lattice_setup("schwinger 128x128", MLMCPI_SCHWINGER, 128, 128, 1.0, 0.0, 2, 3, 1, 0),
      lattice_setup("gff 16x16", MLMCPI_GFF, 16, 16, 0.0, 3.0, 3, 2, 1, 0),
      rotor_setup("rotor 32", 32, 3, 1, 1, false),
      lattice_setup("sigma 8x8", MLMCPI_NONLINEAR_SIGMA, 8, 8, 1.0, 0.0, 3, 2, 1, 0),
  };
  for (const SweepSetup &c : setups) {
    pattern_a(c, true);
    pattern_b(c);
    pattern_c(c);
    pattern_d(c);
    pattern_e(c);
    std::printf(" %s: patterns (a)-(e) done, %d failures so far\n", c.name.c_str(), failures);
  }
}

static void case_heatbath_random() {
  const std::vector<SweepSetup> setups = {
      lattice_setup("schwinger 6x8, device order", MLMCPI_SCHWINGER, 6, 8, 1.0, 0.0, 3, 2, 1, 1),
      lattice_setup("gff 12x12, device order", MLMCPI_GFF, 12, 12, 0.0, 3.0, 3, 2, 1, 1),
      lattice_setup("schwinger 6x8, host shuffle", MLMCPI_SCHWINGER, 6, 8, 1.0, 0.0, 3, 2, 1, 2),
      rotor_setup("rotor 16, host shuffle", 16, 3, 2, 1, true),
  };
  for (const SweepSetup &c : setups) {
    pattern_a(c, false);
    pattern_b(c);
    std::printf(" %s: patterns (a), (b) done, %d failures so far\n", c.name.c_str(), failures);
  }
}

// =====================================================================================================================
// 4. HMCSampler
// =====================================================================================================================
static void hmc_run(const std::string &name, std::shared_ptr<Action> action, const mlmcpi_path_action *qm, const mlmcpi_lattice_action *qft,
                    unsigned M, unsigned B, unsigned n_rep, bool autotune) {
  action->set_seed(SEED, CHAIN0);
  HMCParameters p;
  p.nt = 8;
  p.dt = 0.15;
  p.n_burnin = 2;
  p.n_rep = n_rep;
  p.autotune = autotune;
  p.batch = B;
  p.tune_iterations = 2;
  p.tune_samples = 2 * B;  // two launches of one trajectory per iterate
  HMCSampler sampler(action, p);
  // the constructor: n_burnin draws of n_rep trajectories, then tune_iterations x ceil(tune_samples / B) single trajectories
  const uint32_t expected = p.n_burnin * n_rep + (autotune ? p.tune_iterations * ((p.tune_samples + B - 1) / B) : 0);
  uint32_t traj = sampler.trajectories_used();
  EXPECT(traj == expected, "%s: the constructor used %u trajectories, the contract says %u", name.c_str(), traj, expected);
  const double dt = sampler.get_dt();
  if (!autotune) EXPECT(dt == p.dt, "%s: dt changed without tuning", name.c_str());
  EXPECT(std::isnan(sampler.p_accept()), "%s: statistics not reset by the constructor", name.c_str());

  size_t bytes = 0;
  if (qm) check(mlmcpi_path_hmc_workspace_bytes(qm, B, p.nt, &bytes), "hmc_workspace_bytes");
  else check(mlmcpi_lattice_hmc_workspace_bytes(qft, B, &bytes), "hmc_workspace_bytes");
  Dev x((size_t)M * B * sizeof(double)), work(bytes), flags(B * sizeof(int32_t));
  const Vec x0 = known_state((size_t)M * B);
  auto xs = std::make_shared<SampleState>(M, B);
  write_host(xs, x0);
  sampler.set_state(xs);
  x.put(x0);
  auto s = std::make_shared<SampleState>(M, B);
  Vec model((size_t)M * B, 0.0);  // the caller's state: what it held, overwritten under the class's copy rule
  double n_acc = 0.0;
  unsigned n_tot = 0, seen_acc = 0, seen_rej = 0;
  for (int k = 0; k < 5; ++k) {
    sampler.draw(s);
    if (qm) check(mlmcpi_path_hmc_draw(qm, x.d(), B, p.nt, dt, n_rep, SEED, CHAIN0, traj, work.p, (int32_t *)flags.p, nullptr, nullptr), "path_hmc_draw");
    else check(mlmcpi_lattice_hmc_draw(qft, x.d(), B, p.nt, dt, n_rep, SEED, CHAIN0, traj, work.p, (int32_t *)flags.p, nullptr, nullptr), "lattice_hmc_draw");
    traj += n_rep;
    const std::vector<int32_t> f = flags.get<int32_t>();
    double acc = 0;
    for (int32_t v : f) {
      acc += v;
      (v ? seen_acc : seen_rej)++;
    }
    n_acc += acc / B;
    n_tot++;
    // sampler.hh: accepted() reports chain 0; copy out if accepted, and always for a batch
    if (f[0] != 0 || B > 1) model = x.get<double>();
    EXPECT(sampler.accepted() == (f[0] != 0), "%s draw %d: accepted() = %d, flag 0 = %d", name.c_str(), k, (int)sampler.accepted(), f[0]);
    EXPECT_SAME(dev_of(s), model, "%s draw %d: the caller's state", name.c_str(), k);
    EXPECT_SAME(dev_of(sampler.current_state()), x.get<double>(), "%s draw %d: the current state", name.c_str(), k);
    EXPECT(sampler.p_accept() == n_acc / (1. * n_tot), "%s draw %d: p_accept %.17g vs %.17g", name.c_str(), k, sampler.p_accept(), n_acc / (1. * n_tot));
    EXPECT(sampler.trajectories_used() == traj, "%s draw %d: trajectory counter %u vs %u", name.c_str(), k, sampler.trajectories_used(), traj);
  }
  std::printf(" %s: 5 draws, chain-draws accepted %u, rejected %u, %d failures so far\n", name.c_str(), seen_acc, seen_rej, failures);
}

static void case_hmc() {
  const double T = 4.0, m0 = 1.0, mu2 = 1.0;
  const mlmcpi_path_action ho = path_abi(MLMCPI_HARMONIC, 32, T, m0, mu2);
  const mlmcpi_lattice_action sch = lattice_abi(MLMCPI_SCHWINGER, 16, 8, 1.0, 0.0);
  auto make_ho = [&]() { return std::make_shared<HarmonicOscillatorAction>(std::make_shared<Lattice1D>(32, T), RenormalisationNone, m0, mu2); };
  auto make_sch = [&]() { return std::make_shared<QuenchedSchwingerAction>(std::make_shared<Lattice2D>(16, 8, CoarsenBoth), nullptr, RenormalisationNone, 1.0); };
  for (unsigned n_rep : {1u, 3u}) {
    const std::string r = ", n_rep = " + std::to_string(n_rep);
    hmc_run("HO 32, batch 3" + r, make_ho(), &ho, nullptr, 32, 3, n_rep, false);
    hmc_run("HO 32, batch 1" + r, make_ho(), &ho, nullptr, 32, 1, n_rep, false);
    hmc_run("HO 32, batch 3, tuned" + r, make_ho(), &ho, nullptr, 32, 3, n_rep, true);
    hmc_run("schwinger 16x8, batch 3" + r, make_sch(), nullptr, &sch, 2 * 16 * 8, 3, n_rep, false);
    hmc_run("schwinger 16x8, batch 3, tuned" + r, make_sch(), nullptr, &sch, 2 * 16 * 8, 3, n_rep, true);
  }
}

// =====================================================================================================================
// 5. exact and cluster samplers
// =====================================================================================================================
/** pattern (b) on any Sampler: 6 draws into fresh states, each equal to the replay's, none changed at the end */
static void held_samples(const std::string &name, Sampler &sampler, unsigned M, unsigned B, const std::function<Vec()> &replay_draw) {
  std::vector<std::shared_ptr<SampleState>> kept;
  std::vector<Vec> want;
  for (int k = 0; k < 6; ++k) {
    kept.push_back(std::make_shared<SampleState>(M, B));
    sampler.draw(kept.back());
    want.push_back(replay_draw());
    EXPECT_SAME(dev_of(kept.back()), want.back(), "%s draw %d", name.c_str(), k);
    EXPECT(sampler.accepted(), "%s draw %d: accepted()", name.c_str(), k);
  }
  for (int k = 0; k < 6; ++k) EXPECT_SAME(dev_of(kept[k]), want[k], "%s: the sample of draw %d changed after it was handed out", name.c_str(), k);
  std::printf(" %s: 6 draws, %d failures so far\n", name.c_str(), failures);
}

/** what the replay side keeps of the improved outputs of the sigma model's cluster draws since its last reset: the sum over the
 *  draws of a draw's chi_m (the sum over the chains over B n_updates) and, per chain, the sums of F_d and of C; structure_factor(d)
 *  and correlator() reduce them in the order ClusterImprovedSums documents: every chain's sum over the updates counted, then over
 *  B, added chain by chain */
struct ImprovedReplay {
  ImprovedReplay(unsigned B_, unsigned n_updates_, unsigned n_out_, unsigned Mt_, unsigned Mx_)
      : B(B_), n_updates(n_updates_), n_out(n_out_), Mt(Mt_), Mx(Mx_), chain_F(2 * B_, 0.0), chain_C((size_t)B_ * n_out_, 0.0) {}
  /** one draw: imp [B], F [B][2] or NULL, C [B][n_out] or NULL; F_from_C: without F, F_d of the draw is structure_factor() of its C_d */
  void add(const Vec &imp, const Vec *F, const Vec *C, bool F_from_C = false) {
    double v = 0.0;
    for (double q : imp) v += q;
    v /= (double)B * n_updates;
    improved_sum += v;
    ++draws;
    for (size_t k = 0; C && k < chain_C.size(); ++k) chain_C[k] += (*C)[k];
    for (unsigned b = 0; b < B; ++b) {
      if (F) {
        chain_F[2 * b] += (*F)[2 * b];
        chain_F[2 * b + 1] += (*F)[2 * b + 1];
      } else if (F_from_C && C) {
        const Vec::const_iterator c = C->begin() + (size_t)b * n_out;
        chain_F[2 * b] += mlmcpi::structure_factor(Vec(c, c + Mt / 2 + 1), Mt);
        chain_F[2 * b + 1] += mlmcpi::structure_factor(Vec(c + Mt / 2 + 1, c + n_out), Mx);
      }
    }
  }
  double improved_mean() const { return improved_sum / draws; }
  double structure_factor(int d) const {
    const double n = (double)draws * n_updates;
    double m = 0.0;
    for (unsigned b = 0; b < B; ++b) m += chain_F[2 * b + d] / n / B;
    return m;
  }
  Vec correlator() const {
    const double n = (double)draws * n_updates;
    Vec m(n_out, 0.0);
    for (unsigned k = 0; k < n_out; ++k)
      for (unsigned b = 0; b < B; ++b) m[k] += chain_C[(size_t)b * n_out + k] / n / B;
    return m;
  }
  unsigned B, n_updates, n_out, Mt, Mx, draws = 0;
  double improved_sum = 0.0;
  Vec chain_F, chain_C;
};

static void case_exact_and_cluster() {
  const unsigned B = 3;
  {  // HarmonicOscillatorExactSampler, M = 32
    const unsigned M = 32;
    const mlmcpi_path_action ho = path_abi(MLMCPI_HARMONIC, M, 4.0, 1.0, 1.0);
    auto act = std::make_shared<HarmonicOscillatorAction>(std::make_shared<Lattice1D>(M, 4.0), RenormalisationNone, 1.0, 1.0);
    act->set_seed(SEED, CHAIN0);
    HarmonicOscillatorExactSampler sampler(act, B);
    Vec LT((size_t)M * M);
    check(mlmcpi_ho_cholesky_factor(&ho, LT.data()), "ho_cholesky_factor");
    Dev d_LT(LT.size() * sizeof(double)), x((size_t)M * B * sizeof(double));
    d_LT.put(LT);
    uint32_t step = 0;
    held_samples("HO exact 32", sampler, M, B, [&]() {
      check(mlmcpi_path_exact_draw(&ho, d_LT.d(), x.d(), B, SEED ^ EXACT_XOR, CHAIN0, step++, nullptr), "path_exact_draw");
      return x.get<double>();
    });
  }
  {  // GFFExactSampler on the plain 8 x 8 level
    const mlmcpi_lattice_action gff = lattice_abi(MLMCPI_GFF, 8, 8, 0.0, 3.0);
    auto act = std::make_shared<GFFAction>(std::make_shared<Lattice2D>(8, 8, CoarsenRotate), nullptr, 3.0);
    act->set_seed(SEED, CHAIN0);
    GFFExactSampler sampler(act, B);
    size_t bytes = 0;
    check(mlmcpi_lattice_exact_workspace_bytes(&gff, B, &bytes), "lattice_exact_workspace_bytes");
    Dev work(bytes), x(64 * B * sizeof(double));
    uint32_t step = 0;
    held_samples("GFF exact 8x8", sampler, 64, B, [&]() {
      check(mlmcpi_lattice_exact_draw(&gff, x.d(), B, SEED ^ EXACT_XOR, CHAIN0, step++, work.p, nullptr), "lattice_exact_draw");
      return x.get<double>();
    });
    // ... and on the rotated, smoothed level below it (GFFAction::draw_level)
    auto coarse = std::dynamic_pointer_cast<GFFAction>(act->coarse_action());
    coarse->set_seed(SEED + 1, CHAIN0 + 1);
    EXPECT(!coarse->plain() && coarse->sample_size() == 32, "the coarse GFF level is the rotated 8 x 8 lattice");
    GFFExactSampler level_sampler(coarse, B);
    mlmcpi_gff_level *level = nullptr;
    check(mlmcpi_gff_level_create(8, 8, (int32_t)CoarsenRotate, 1, 3.0, 2, 1.0, &level), "gff_level_create");
    Dev xl(32 * B * sizeof(double));
    uint32_t lstep = 0;
    held_samples("GFF exact rotated 8x8 level", level_sampler, 32, B, [&]() {
      check(mlmcpi_gff_level_draw(level, xl.d(), B, (SEED + 1) ^ EXACT_XOR, CHAIN0 + 1, lstep++, nullptr), "gff_level_draw");
      return xl.get<double>();
    });
    mlmcpi_gff_level_destroy(level);
  }
  ClusterParameters cp;
  cp.n_burnin = 2;
  cp.n_meas = 3;
  cp.batch = B;
  const unsigned n_ctor = cp.n_burnin + cp.n_meas;  // draws the constructors make: burn-in, then the timing draws
  {  // ClusterSampler: rotor M = 32, n_updates = 3
    const unsigned M = 32, n_updates = 3;
    cp.n_updates = n_updates;
    const mlmcpi_path_action rot = path_abi(MLMCPI_ROTOR, M, 4.0, 0.25, 0.0);
    auto act = std::make_shared<RotorAction>(std::make_shared<Lattice1D>(M, 4.0), RenormalisationNone, 0.25);
    act->set_seed(SEED, CHAIN0);
    ClusterSampler sampler(act, cp);
    Dev x((size_t)M * B * sizeof(double)), sites(B * sizeof(uint32_t));
    check(mlmcpi_path_initialise(&rot, x.d(), B, SEED, CHAIN0, nullptr), "path_initialise");
    uint32_t update = 0;
    auto draw = [&]() {
      check(mlmcpi_path_cluster_draw(&rot, x.d(), B, n_updates, SEED, CHAIN0, update, (uint32_t *)sites.p, nullptr), "path_cluster_draw");
      update += n_updates;
      return x.get<double>();
    };
    for (unsigned k = 0; k < n_ctor; ++k) draw();
    sites.zero();
    held_samples("rotor cluster 32", sampler, M, B, draw);
    double total = 0.0;
    for (uint32_t v : sites.get<uint32_t>()) total += v;
    double held = sampler.flipped_sites_folded();
    for (uint32_t v : sampler.flipped_sites_unfolded()) held += v;
    EXPECT(held == total, "rotor cluster: flipped sites %.17g, the replay's counters sum to %.17g", held, total);
    const double mean = sampler.mean_cluster_size();  // folds
    EXPECT(mean == total / B / (6 * n_updates), "rotor cluster: mean cluster size %.17g vs %.17g", mean, total / B / (6 * n_updates));
    EXPECT(sampler.flipped_sites_folded() == total, "rotor cluster: the total after the fold %.17g vs %.17g", sampler.flipped_sites_folded(), total);
    for (uint32_t v : sampler.flipped_sites_unfolded()) EXPECT(v == 0, "rotor cluster: a device counter is %u after the fold", v);
    EXPECT(sampler.mean_cluster_size() == mean && sampler.flipped_sites_folded() == total, "rotor cluster: a second fold changed the total");
    EXPECT(sampler.p_accept() == 1.0, "rotor cluster: p_accept");
  }
  {  // QuenchedSchwingerClusterSampler 8 x 8
    const unsigned n_updates = 3;
    cp.n_updates = n_updates;
    const mlmcpi_lattice_action sch = lattice_abi(MLMCPI_SCHWINGER, 8, 8, 1.0, 0.0);
    auto act = std::make_shared<QuenchedSchwingerAction>(std::make_shared<Lattice2D>(8, 8, CoarsenBoth), nullptr, RenormalisationNone, 1.0);
    act->set_seed(SEED, CHAIN0);
    QuenchedSchwingerClusterSampler sampler(act, cp);
    size_t bytes = 0;
    check(mlmcpi_schwinger_cluster_workspace_bytes(&sch, B, &bytes), "schwinger_cluster_workspace_bytes");
    Dev work(bytes), psi(64 * B * sizeof(double)), theta(128 * B * sizeof(double));
    check(mlmcpi_schwinger_cluster_init(&sch, psi.d(), B, SEED, CHAIN0, nullptr), "schwinger_cluster_init");
    uint32_t draw_counter = 0;
    auto draw = [&]() {
      check(mlmcpi_schwinger_cluster_draw(&sch, psi.d(), theta.d(), B, n_updates, SEED, CHAIN0, draw_counter++, work.d(), nullptr), "schwinger_cluster_draw");
      return theta.get<double>();
    };
    for (unsigned k = 0; k < n_ctor; ++k) draw();
    held_samples("schwinger cluster 8x8", sampler, 128, B, draw);
  }
  // WolffClusterSampler and SwendsenWangSampler: sigma 8 x 8 and the rotated 8 x 8 level below it
  for (int rotated = 0; rotated < 2; ++rotated) {
    const unsigned n_updates = 2, n = rotated ? 32 : 64, M = 2 * n;
    cp.n_updates = n_updates;
    const double beta = 1.0;
    const mlmcpi_sigma_level lv{8, 8, rotated, beta};
    const mlmcpi_lattice_action plain = lattice_abi(MLMCPI_NONLINEAR_SIGMA, 8, 8, beta, 0.0);
    const std::string where = rotated ? "sigma rotated 8x8 level" : "sigma 8x8";
    auto make = [&]() {
      auto fine = std::make_shared<NonlinearSigmaAction>(std::make_shared<Lattice2D>(8, 8, CoarsenRotate), nullptr, RenormalisationNone, beta);
      std::shared_ptr<NonlinearSigmaAction> act = rotated ? std::dynamic_pointer_cast<NonlinearSigmaAction>(fine->coarse_action()) : fine;
      act->set_seed(SEED, CHAIN0);
      return act;
    };
    auto init = [&](double *x) {
      if (rotated) check(mlmcpi_sigma_level_initialise(&lv, x, B, SEED, CHAIN0, nullptr), "sigma_level_initialise");
      else check(mlmcpi_lattice_initialise(&plain, x, B, SEED, CHAIN0, nullptr), "lattice_initialise");
    };
    {
      auto act = make();
      EXPECT(act->sample_size() == M && act->rotated() == (rotated != 0), "%s: the level", where.c_str());
      WolffClusterSampler sampler(act, cp);
      size_t bytes = 0;
      check(mlmcpi_sigma_level_cluster_workspace_bytes(&lv, B, &bytes), "sigma_level_cluster_workspace_bytes");
      Dev x((size_t)M * B * sizeof(double)), sites(B * sizeof(uint32_t)), work(bytes);
      init(x.d());
      uint32_t update = 0;
      auto draw = [&]() {
        check(mlmcpi_sigma_level_cluster_draw(&lv, x.d(), B, n_updates, SEED, CHAIN0, update, (uint32_t *)sites.p, work.p, nullptr), "sigma_level_cluster_draw");
        update += n_updates;
        return x.get<double>();
      };
      for (unsigned k = 0; k < n_ctor; ++k) draw();
      sites.zero();
      held_samples("wolff, " + where, sampler, M, B, draw);
      double total = 0.0;
      for (uint32_t v : sites.get<uint32_t>()) total += v;
      double held = sampler.flipped_sites_folded();
      for (uint32_t v : sampler.flipped_sites_unfolded()) held += v;
      EXPECT(held == total, "wolff, %s: flipped sites %.17g, the replay's counters sum to %.17g", where.c_str(), held, total);
      const double mean = sampler.mean_cluster_size();  // folds
      EXPECT(mean == total / B / (double)(6 * n_updates), "wolff, %s: mean cluster size %.17g vs %.17g", where.c_str(), mean, total / B / (double)(6 * n_updates));
      EXPECT(sampler.flipped_sites_folded() == total, "wolff, %s: the total after the fold", where.c_str());
      for (uint32_t v : sampler.flipped_sites_unfolded()) EXPECT(v == 0, "wolff, %s: a device counter is %u after the fold", where.c_str(), v);
      EXPECT(sampler.mean_cluster_size() == mean && sampler.flipped_sites_folded() == total, "wolff, %s: a second fold changed the total", where.c_str());
    }
    {
      SwendsenWangSampler sampler(make(), cp);
      size_t bytes = 0;
      check(mlmcpi_sigma_level_sw_workspace_bytes(&lv, B, &bytes), "sigma_level_sw_workspace_bytes");
      Dev x((size_t)M * B * sizeof(double)), clusters(B * sizeof(uint32_t)), improved(B * sizeof(double)), work(bytes);
      init(x.d());
      uint32_t update = 0;
      double clusters_total = 0.0, improved_sum = 0.0;
      auto draw = [&]() {
        clusters.zero();
        improved.zero();
        check(mlmcpi_sigma_level_sw_draw(&lv, x.d(), B, n_updates, SEED, CHAIN0, update, nullptr, (uint32_t *)clusters.p, improved.d(), work.p, nullptr), "sigma_level_sw_draw");
        update += n_updates;
        double c = 0.0, v = 0.0;
        for (uint32_t q : clusters.get<uint32_t>()) c += q;
        for (double q : improved.get<double>()) v += q;
        v /= (double)B * n_updates;
        clusters_total += c / B;
        improved_sum += v;
        return x.get<double>();
      };
      for (unsigned k = 0; k < n_ctor; ++k) draw();
      clusters_total = improved_sum = 0.0;  // reset_improved() at the end of the constructor
      held_samples("swendsen-wang, " + where, sampler, M, B, draw);
      EXPECT(sampler.mean_clusters_per_update() == clusters_total / (6.0 * n_updates), "swendsen-wang, %s: clusters per update %.17g vs %.17g", where.c_str(),
             sampler.mean_clusters_per_update(), clusters_total / (6.0 * n_updates));
      EXPECT(sampler.improved_mean() == improved_sum / 6, "swendsen-wang, %s: improved chi_m %.17g vs %.17g", where.c_str(), sampler.improved_mean(), improved_sum / 6);
    }
    // the option paths: the improved entry points, their outputs kept by the replay per chain
    uint32_t n_out = 0;
    check(mlmcpi_sigma_level_correlator_size(&lv, &n_out), "sigma_level_correlator_size");
    struct Options {
      const char *name;
      bool improved, structure, correlator;
    };
    auto with_options = [&](const Options &o) {
      ClusterParameters q = cp;
      q.improved = o.improved;
      q.structure = o.structure;
      q.correlator = o.correlator;
      return q;
    };
    for (const Options &o : {Options{"improved", true, false, false}, Options{"structure", false, true, false}, Options{"correlator", false, false, true},
                             Options{"structure + correlator", false, true, true}}) {
      const std::string name = std::string("wolff (") + o.name + "), " + where;
      WolffClusterSampler sampler(make(), with_options(o));
      size_t bytes = 0;
      check(mlmcpi_sigma_level_cluster_improved_workspace_bytes(&lv, B, &bytes), "sigma_level_cluster_improved_workspace_bytes");
      Dev x((size_t)M * B * sizeof(double)), sites(B * sizeof(uint32_t)), improved(B * sizeof(double)), structure(2 * B * sizeof(double)),
          corr((size_t)B * n_out * sizeof(double)), work(bytes);
      init(x.d());
      uint32_t update = 0;
      ImprovedReplay kept(B, n_updates, n_out, lv.Mt, lv.Mx);
      auto draw = [&]() {
        improved.zero();
        structure.zero();
        corr.zero();
        check(mlmcpi_sigma_level_cluster_improved_draw(&lv, x.d(), B, n_updates, SEED, CHAIN0, update, (uint32_t *)sites.p, improved.d(),
                                                       o.structure ? structure.d() : nullptr, o.correlator ? corr.d() : nullptr, work.p, bytes, nullptr),
              "sigma_level_cluster_improved_draw");
        update += n_updates;
        const Vec F = structure.get<double>(), C = corr.get<double>();
        kept.add(improved.get<double>(), o.structure ? &F : nullptr, o.correlator ? &C : nullptr);
        return x.get<double>();
      };
      for (unsigned k = 0; k < n_ctor; ++k) draw();
      sites.zero();
      kept = ImprovedReplay(B, n_updates, n_out, lv.Mt, lv.Mx);  // the constructor resets after its draws
      held_samples(name, sampler, M, B, draw);
      double total = 0.0, held = sampler.flipped_sites_folded();
      for (uint32_t v : sites.get<uint32_t>()) total += v;
      for (uint32_t v : sampler.flipped_sites_unfolded()) held += v;
      EXPECT(held == total, "%s: flipped sites %.17g, the replay's counters sum to %.17g", name.c_str(), held, total);
      EXPECT(sampler.improved_mean() == kept.improved_mean(), "%s: improved chi_m %.17g vs %.17g", name.c_str(), sampler.improved_mean(), kept.improved_mean());
      for (int d = 0; o.structure && d < 2; ++d)
        EXPECT(sampler.improved_structure_factor(d).value == kept.structure_factor(d), "%s: improved F_%d %.17g vs %.17g", name.c_str(), d,
               sampler.improved_structure_factor(d).value, kept.structure_factor(d));
      if (o.correlator) EXPECT_SAME(sampler.improved_correlator().mean, kept.correlator(), "%s: improved correlator", name.c_str());
    }
    for (const Options &o : {Options{"structure", false, true, false}, Options{"correlator", false, false, true}, Options{"structure + correlator", false, true, true}}) {
      const std::string name = std::string("swendsen-wang (") + o.name + "), " + where;
      SwendsenWangSampler sampler(make(), with_options(o));
      size_t bytes = 0;
      if (o.correlator) check(mlmcpi_sigma_level_sw_correlator_workspace_bytes(&lv, B, &bytes), "sigma_level_sw_correlator_workspace_bytes");
      else check(mlmcpi_sigma_level_sw_structure_workspace_bytes(&lv, B, &bytes), "sigma_level_sw_structure_workspace_bytes");
      Dev x((size_t)M * B * sizeof(double)), clusters(B * sizeof(uint32_t)), improved(B * sizeof(double)), structure(2 * B * sizeof(double)),
          corr((size_t)B * n_out * sizeof(double)), work(bytes);
      init(x.d());
      uint32_t update = 0;
      ImprovedReplay kept(B, n_updates, n_out, lv.Mt, lv.Mx);
      auto draw = [&]() {
        clusters.zero();
        improved.zero();
        structure.zero();
        corr.zero();
        // with the correlator the library returns C alone: F of the draw, where asked for, is structure_factor() of its C
        if (o.correlator)
          check(mlmcpi_sigma_level_sw_correlator_draw(&lv, x.d(), B, n_updates, SEED, CHAIN0, update, nullptr, (uint32_t *)clusters.p, improved.d(), corr.d(),
                                                      work.p, bytes, nullptr), "sigma_level_sw_correlator_draw");
        else
          check(mlmcpi_sigma_level_sw_structure_draw(&lv, x.d(), B, n_updates, SEED, CHAIN0, update, nullptr, (uint32_t *)clusters.p, improved.d(),
                                                     structure.d(), work.p, bytes, nullptr), "sigma_level_sw_structure_draw");
        update += n_updates;
        const Vec F = structure.get<double>(), C = corr.get<double>();
        kept.add(improved.get<double>(), o.correlator ? nullptr : &F, o.correlator ? &C : nullptr, o.structure);
        return x.get<double>();
      };
      for (unsigned k = 0; k < n_ctor; ++k) draw();
      kept = ImprovedReplay(B, n_updates, n_out, lv.Mt, lv.Mx);  // reset_improved() at the end of the constructor
      held_samples(name, sampler, M, B, draw);
      EXPECT(sampler.improved_mean() == kept.improved_mean(), "%s: improved chi_m %.17g vs %.17g", name.c_str(), sampler.improved_mean(), kept.improved_mean());
      for (int d = 0; o.structure && d < 2; ++d)
        EXPECT(sampler.improved_structure_factor(d).value == kept.structure_factor(d), "%s: improved F_%d %.17g vs %.17g", name.c_str(), d,
               sampler.improved_structure_factor(d).value, kept.structure_factor(d));
      if (o.correlator) EXPECT_SAME(sampler.improved_correlator().mean, kept.correlator(), "%s: improved correlator", name.c_str());
    }
  }
}

// =====================================================================================================================
// 6. TwoLevelMetropolisStep
// =====================================================================================================================
static uint64_t level_seed(uint64_t seed, int level) {  // multilevel.hh: TwoLevelMetropolisStep::level_seed()
  return (seed ^ 0x5517A4B3ull) + 0x9E3779B97F4A7C15ull * (uint64_t)(level + 1);
}
static const unsigned N_MEAS = 3;

struct TwoLevelFamily {
  std::string name;
  unsigned Mf = 0, Mc = 0;
  // object side: the step on (coarse, fine) with the fine action's seed set
  std::function<std::shared_ptr<TwoLevelMetropolisStep>(uint64_t seed, unsigned B)> make_step;
  // replay side
  std::function<void(double *d_xc, unsigned B, uint32_t k)> propose;  // coarse input of draw k, from the matching *_initialise
  std::function<size_t(unsigned B)> work_bytes;
  std::function<void(const double *xc, double *theta, unsigned B, uint64_t lseed, uint32_t step, void *work, int32_t *acc)> draw;
};

static void twolevel_run(const TwoLevelFamily &fam, unsigned B) {
  const int n_draws = 8;
  Dev xc((size_t)fam.Mc * B * sizeof(double)), theta((size_t)fam.Mf * B * sizeof(double)), work(fam.work_bytes(B)), flags(B * sizeof(int32_t));
  std::vector<Vec> proposals;
  for (int k = 0; k < n_draws; ++k) {
    fam.propose(xc.d(), B, k);
    proposals.push_back(xc.get<double>());
  }
  // the replay alone: find the first seed with which chain 0 both accepts and rejects in the 8 draws
  std::vector<Vec> states;
  std::vector<std::vector<int32_t>> accepts;
  uint64_t seed = 0;
  bool both = false;
  for (unsigned trial = 0; trial < 32 && !both; ++trial) {
    seed = SEED + trial;
    states.clear();
    accepts.clear();
    theta.zero();                // the step starts from a zero theta_fine ...
    uint32_t step = N_MEAS;      // ... and the constructor's timing draws have used the first n_meas steps
    unsigned n_acc = 0;
    for (int k = 0; k < n_draws; ++k) {
      xc.put(proposals[k]);
      fam.draw(xc.d(), theta.d(), B, level_seed(seed, 0), step++, work.p, (int32_t *)flags.p);
      states.push_back(theta.get<double>());
      accepts.push_back(flags.get<int32_t>());
      n_acc += accepts.back()[0] != 0;
    }
    both = n_acc > 0 && n_acc < (unsigned)n_draws;
  }
  EXPECT(both, "%s, batch %u: no seed of 32 shows both an accept and a reject of chain 0 in %d draws: the case would pass vacuously", fam.name.c_str(), B, n_draws);
  if (!both) return;

  auto step = fam.make_step(seed, B);
  EXPECT(step->steps_used() == N_MEAS, "%s: the constructor used %u steps, n_meas = %u", fam.name.c_str(), step->steps_used(), N_MEAS);
  auto coarse = std::make_shared<SampleState>(fam.Mc, B), s = std::make_shared<SampleState>(fam.Mf, B);
  const Vec marker = known_state((size_t)fam.Mf * B, 3);
  write_host(s, marker);
  Vec model = marker;
  double n_acc = 0.0;
  unsigned n_tot = 0, rejected = 0;
  for (int k = 0; k < n_draws; ++k) {
    write_host(coarse, proposals[k]);
    step->draw(coarse, s);
    double acc = 0;
    for (int32_t v : accepts[k]) acc += v;
    n_acc += acc / B;
    n_tot++;
    const bool a0 = accepts[k][0] != 0;
    rejected += !a0;
    if (a0 || B > 1) model = states[k];  // copy_if_rejected == false: a rejected draw of one chain leaves the caller's state alone
    EXPECT(step->accepted() == a0, "%s, batch %u, draw %d: accepted() = %d, flag 0 = %d", fam.name.c_str(), B, k, (int)step->accepted(), accepts[k][0]);
    EXPECT_SAME(dev_of(s), model, "%s, batch %u, draw %d%s", fam.name.c_str(), B, k, a0 ? "" : " (rejected)");
    EXPECT(step->p_accept() == n_acc / (1. * n_tot), "%s, batch %u, draw %d: p_accept %.17g vs %.17g", fam.name.c_str(), B, k, step->p_accept(), n_acc / (1. * n_tot));
    EXPECT_SAME(dev_of(coarse), proposals[k], "%s, batch %u, draw %d: the coarse input changed", fam.name.c_str(), B, k);
  }
  std::printf(" %s, batch %u: seed %llu, chain 0 rejected %u of %d, %d failures so far\n", fam.name.c_str(), B, (unsigned long long)seed, rejected, n_draws, failures);
}

static const uint64_t PROPOSAL_SEED = 424243ull;
static uint32_t proposal_chain0(uint32_t k) { return 100 + 16 * k; }

static TwoLevelFamily path_family(const std::string &name, int kind, double T, double m0, double mu2) {
  TwoLevelFamily f;
  const unsigned Mf = 32, Mc = 16;
  const mlmcpi_path_action fine = path_abi(kind, Mf, T, m0, mu2), coarse = path_abi(kind, Mc, T, m0, mu2);  // no renormalisation
  f.name = name;
  f.Mf = Mf;
  f.Mc = Mc;
  f.make_step = [=](uint64_t seed, unsigned B) {
    std::shared_ptr<Action> fa;
    std::shared_ptr<ConditionedFineAction> cfa;
    if (kind == MLMCPI_ROTOR) {
      auto r = std::make_shared<RotorAction>(std::make_shared<Lattice1D>(Mf, T), RenormalisationNone, m0);
      fa = r;
      cfa = std::make_shared<RotorConditionedFineAction>(r);
    } else {
      auto h = std::make_shared<HarmonicOscillatorAction>(std::make_shared<Lattice1D>(Mf, T), RenormalisationNone, m0, mu2);
      fa = h;
      cfa = std::make_shared<GaussianConditionedFineAction>(h);
    }
    fa->set_seed(seed, CHAIN0);
    return std::make_shared<TwoLevelMetropolisStep>(fa->coarse_action(), fa, cfa, B, N_MEAS);
  };
  if (kind == MLMCPI_ROTOR) {
    f.propose = [=](double *x, unsigned B, uint32_t k) { check(mlmcpi_path_initialise(&coarse, x, B, PROPOSAL_SEED, proposal_chain0(k), nullptr), "path_initialise"); };
  } else {
    // mlmcpi_path_initialise gives the oscillator zeros, and a zero proposal onto a zero state is accepted with dS = 0 for ever:
    // the coarse inputs come from the coarse action's exact draw instead, so that both outcomes occur
    Vec LT((size_t)Mc * Mc);
    check(mlmcpi_ho_cholesky_factor(&coarse, LT.data()), "ho_cholesky_factor");
    auto d_LT = std::make_shared<Dev>(LT.size() * sizeof(double));
    d_LT->put(LT);
    f.propose = [=](double *x, unsigned B, uint32_t k) {
      check(mlmcpi_path_exact_draw(&coarse, d_LT->d(), x, B, PROPOSAL_SEED, proposal_chain0(k), k, nullptr), "path_exact_draw");
    };
  }
  f.work_bytes = [=](unsigned B) {
    size_t bytes = 0;
    check(mlmcpi_path_twolevel_workspace_bytes(&fine, B, &bytes), "path_twolevel_workspace_bytes");
    return bytes;
  };
  f.draw = [=](const double *xc, double *theta, unsigned B, uint64_t lseed, uint32_t step, void *work, int32_t *acc) {
    check(mlmcpi_path_twolevel_draw(&fine, &coarse, xc, theta, B, lseed, CHAIN0, step, work, acc, nullptr, nullptr), "path_twolevel_draw");
  };
  return f;
}

static TwoLevelFamily schwinger_family(const std::string &name, unsigned Mt, unsigned Mx, CoarseningType type, int cfa_kind, double beta) {
  TwoLevelFamily f;
  const bool both = type == CoarsenBoth;
  const unsigned Mtc = Mt / 2, Mxc = both ? Mx / 2 : Mx;  // CoarsenAlternate halves the temporal direction on level 0
  const mlmcpi_lattice_action fine = lattice_abi(MLMCPI_SCHWINGER, Mt, Mx, beta, 0.0);
  const mlmcpi_lattice_action coarse = lattice_abi(MLMCPI_SCHWINGER, Mtc, Mxc, (both ? 0.25 : 0.5) * beta, 0.0);  // action.hh: beta_coarse, unrenormalised
  f.name = name;
  f.Mf = 2 * Mt * Mx;
  f.Mc = 2 * Mtc * Mxc;
  f.make_step = [=](uint64_t seed, unsigned B) {
    auto fa = std::make_shared<QuenchedSchwingerAction>(std::make_shared<Lattice2D>(Mt, Mx, type), nullptr, RenormalisationNone, beta);
    fa->set_seed(seed, CHAIN0);
    std::shared_ptr<ConditionedFineAction> cfa;
    if (cfa_kind == 1) cfa = QuenchedSchwingerGaussianConditionedFineActionFactory().get(fa);
    else cfa = QuenchedSchwingerConditionedFineActionFactory().get(fa);
    return std::make_shared<TwoLevelMetropolisStep>(fa->coarse_action(), fa, cfa, B, N_MEAS);
  };
  f.propose = [=](double *x, unsigned B, uint32_t k) { check(mlmcpi_lattice_initialise(&coarse, x, B, PROPOSAL_SEED, proposal_chain0(k), nullptr), "lattice_initialise"); };
  f.work_bytes = [=](unsigned B) {
    size_t bytes = 0;
    check(mlmcpi_lattice_twolevel_workspace_bytes(&fine, &coarse, B, &bytes), "lattice_twolevel_workspace_bytes");
    return bytes;
  };
  f.draw = [=](const double *xc, double *theta, unsigned B, uint64_t lseed, uint32_t step, void *work, int32_t *acc) {
    check(mlmcpi_lattice_twolevel_draw_cfa(&fine, &coarse, cfa_kind, xc, theta, B, lseed, CHAIN0, step, work, acc, nullptr, nullptr), "lattice_twolevel_draw_cfa");
  };
  return f;
}

static TwoLevelFamily gff_family(double mass) {
  TwoLevelFamily f;
  mlmcpi_gff_level *fine = nullptr, *coarse = nullptr;  // kept for the life of the process
  check(mlmcpi_gff_level_create(8, 8, (int32_t)CoarsenRotate, 0, mass, 0, 1.0, &fine), "gff_level_create");
  check(mlmcpi_gff_level_create(8, 8, (int32_t)CoarsenRotate, 1, mass, 2, 1.0, &coarse), "gff_level_create");  // gffaction.hh:201-208
  f.name = "gff 8x8, rotated coarse level";
  f.Mf = 64;
  f.Mc = 32;
  f.make_step = [=](uint64_t seed, unsigned B) {
    auto fa = std::make_shared<GFFAction>(std::make_shared<Lattice2D>(8, 8, CoarsenRotate), nullptr, mass);
    fa->set_seed(seed, CHAIN0);
    return std::make_shared<TwoLevelMetropolisStep>(fa->coarse_action(), fa, GFFConditionedFineActionFactory().get(fa), B, N_MEAS);
  };
  // GFFAction::initialise_state of a level that is not plain = draw_level(phi, 0xFFFFFF) with the exact samplers' key
  f.propose = [=](double *x, unsigned B, uint32_t k) {
    check(mlmcpi_gff_level_draw(coarse, x, B, PROPOSAL_SEED ^ EXACT_XOR, proposal_chain0(k), 0xFFFFFFu, nullptr), "gff_level_draw");
  };
  f.work_bytes = [=](unsigned B) {
    size_t bytes = 0;
    check(mlmcpi_gff_twolevel_workspace_bytes(fine, B, &bytes), "gff_twolevel_workspace_bytes");
    return bytes;
  };
  f.draw = [=](const double *xc, double *theta, unsigned B, uint64_t lseed, uint32_t step, void *work, int32_t *acc) {
    check(mlmcpi_gff_twolevel_draw(fine, coarse, xc, theta, B, lseed, CHAIN0, step, work, acc, nullptr, nullptr), "gff_twolevel_draw");
  };
  return f;
}

static TwoLevelFamily sigma_family(double beta) {
  TwoLevelFamily f;
  const mlmcpi_sigma_level fine{8, 8, 0, beta}, coarse{8, 8, 1, beta};  // action.hh: beta_coarse = beta without renormalisation
  f.name = "sigma 8x8, rotated coarse level";
  f.Mf = 128;
  f.Mc = 64;
  f.make_step = [=](uint64_t seed, unsigned B) {
    auto fa = std::make_shared<NonlinearSigmaAction>(std::make_shared<Lattice2D>(8, 8, CoarsenRotate), nullptr, RenormalisationNone, beta);
    fa->set_seed(seed, CHAIN0);
    return std::make_shared<TwoLevelMetropolisStep>(fa->coarse_action(), fa, NonlinearSigmaConditionedFineActionFactory().get(fa), B, N_MEAS);
  };
  f.propose = [=](double *x, unsigned B, uint32_t k) { check(mlmcpi_sigma_level_initialise(&coarse, x, B, PROPOSAL_SEED, proposal_chain0(k), nullptr), "sigma_level_initialise"); };
  f.work_bytes = [=](unsigned B) {
    size_t bytes = 0;
    check(mlmcpi_sigma_twolevel_workspace_bytes(&fine, B, &bytes), "sigma_twolevel_workspace_bytes");
    return bytes;
  };
  f.draw = [=](const double *xc, double *theta, unsigned B, uint64_t lseed, uint32_t step, void *work, int32_t *acc) {
    check(mlmcpi_sigma_twolevel_draw(&fine, &coarse, xc, theta, B, lseed, CHAIN0, step, work, acc, nullptr, nullptr), "sigma_twolevel_draw");
  };
  return f;
}

static void case_twolevel() {
  const std::vector<TwoLevelFamily> families = {
      path_family("HO 32 -> 16", MLMCPI_HARMONIC, 32.0, 1.0, 1.0),
      path_family("rotor 32 -> 16", MLMCPI_ROTOR, 4.0, 0.25, 0.0),
      schwinger_family("schwinger 16x8 CoarsenAlternate", 16, 8, CoarsenAlternate, 0, 2.0),
      schwinger_family("schwinger 8x8 CoarsenBoth, cfa 0", 8, 8, CoarsenBoth, 0, 2.0),
      schwinger_family("schwinger 8x8 CoarsenBoth, cfa 1", 8, 8, CoarsenBoth, 1, 2.0),
      gff_family(3.0),
      sigma_family(1.0),
  };
  for (const TwoLevelFamily &f : families)
    for (unsigned B : {1u, 3u}) twolevel_run(f, B);
}

// =====================================================================================================================
// 7. HierarchicalSampler and MultilevelSampler on HO M = 32, three levels
// =====================================================================================================================
static const unsigned HL = 3;                                  // levels
static const unsigned HM[HL] = {32, 16, 8};
static const double HT = 32.0, Hm0 = 1.0, Hmu2 = 1.0;          // a = 1: unrenormalised coarse actions differ enough to reject

/** what the hierarchy's classes share on the replay side: states, the two-level steps' theta / workspace / step, the exact draw */
struct HierarchyReplay {
  HierarchyReplay(unsigned B_, uint64_t seed0, uint64_t seed1, uint64_t seed2) : B(B_), seeds{seed0, seed1, seed2}, LT((size_t)HM[2] * HM[2] * sizeof(double)),
                                                                               exact((size_t)HM[2] * B_ * sizeof(double)), flags(B_ * sizeof(int32_t)), q(B_ * sizeof(double)) {
    for (unsigned l = 0; l < HL; ++l) {
      act[l] = path_abi(MLMCPI_HARMONIC, HM[l], HT, Hm0, Hmu2);  // RenormalisationNone: every level keeps (m0, mu2)
      st.push_back(std::make_shared<Dev>((size_t)HM[l] * B * sizeof(double)));
    }
    for (unsigned l = 0; l + 1 < HL; ++l) {
      size_t bytes = 0;
      check(mlmcpi_path_twolevel_workspace_bytes(&act[l], B, &bytes), "path_twolevel_workspace_bytes");
      work.push_back(std::make_shared<Dev>(bytes));
      theta.push_back(std::make_shared<Dev>((size_t)HM[l] * B * sizeof(double)));  // zero after the constructor
      step[l] = N_MEAS;                                                           // its timing draws
    }
    Vec h((size_t)HM[2] * HM[2]);
    check(mlmcpi_ho_cholesky_factor(&act[2], h.data()), "ho_cholesky_factor");
    LT.put(h);
  }
  /** HarmonicOscillatorExactSampler::draw into st[2] */
  void coarse_draw() {
    check(mlmcpi_path_exact_draw(&act[2], LT.d(), exact.d(), B, seeds[2] ^ EXACT_XOR, CHAIN0, exact_step++, nullptr), "path_exact_draw");
    check(mlmcpi_copy_d2d(st[2]->p, exact.p, exact.bytes, nullptr), "copy_d2d");
  }
  /** TwoLevelMetropolisStep::draw(st[l + 1], st[l]) of level l; returns the flags */
  std::vector<int32_t> twolevel_draw(unsigned l) {
    check(mlmcpi_path_twolevel_draw(&act[l], &act[l + 1], st[l + 1]->d(), theta[l]->d(), B, level_seed(seeds[l], (int)l), CHAIN0, step[l]++, work[l]->p,
                                    (int32_t *)flags.p, nullptr, nullptr), "path_twolevel_draw");
    const std::vector<int32_t> f = flags.get<int32_t>();
    double acc = 0;
    for (int32_t v : f) acc += v;
    lev_tot[l]++;
    lev_acc[l] += acc / B;
    if (f[0] != 0 || B > 1) check(mlmcpi_copy_d2d(st[l]->p, theta[l]->p, theta[l]->bytes, nullptr), "copy_d2d");
    return f;
  }
  const unsigned B;
  const uint64_t seeds[HL];
  mlmcpi_path_action act[HL];
  std::vector<std::shared_ptr<Dev>> st, theta, work;
  uint32_t step[HL] = {0, 0, 0}, exact_step = 0;
  double lev_acc[HL] = {0, 0, 0}, lev_tot[HL] = {0, 0, 0};
  Dev LT, exact, flags, q;
};

/** HierarchicalSampler::draw (hierarchicalsampler.cc:55-81) in ABI calls; returns accept */
static bool hierarchical_replay_draw(HierarchyReplay &r) {
  bool accept = true;
  for (unsigned l = 1; l < HL; ++l) check(mlmcpi_path_copy_from_fine(r.st[l - 1]->d(), r.st[l]->d(), HM[l], r.B, nullptr), "path_copy_from_fine");
  for (int l = (int)HL - 1; l >= 0; --l) {
    if (l == (int)HL - 1) {
      r.coarse_draw();  // set_state of an exact sampler does nothing; its draws are always accepted
      r.lev_tot[l]++;
      r.lev_acc[l]++;
    } else {
      check(mlmcpi_copy_d2d(r.theta[l]->p, r.st[l]->p, r.st[l]->bytes, nullptr), "copy_d2d");  // set_state(phi_sampler_state[l])
      accept = accept && r.twolevel_draw(l)[0] != 0;
    }
    if (!accept) break;
  }
  return accept;
}

static std::shared_ptr<HarmonicOscillatorAction> hierarchy_fine_action(uint64_t seed) {
  auto a = std::make_shared<HarmonicOscillatorAction>(std::make_shared<Lattice1D>(HM[0], HT), RenormalisationNone, Hm0, Hmu2);
  a->set_seed(seed, CHAIN0);
  return a;
}

/** the windowed statistics of common/statistics.cc:4-27 restated: n, the running average a1, S_k <- ((N_k - 1) S_k + Q Q_{-k}) / N_k with
 *  N_k = n - k over the k the window holds; tau_int = max(1, 1 + 2 sum_{k >= 1} (1 - k / n) (S_k - a1^2) / (S_0 - a1^2)) */
struct WindowStats {
  explicit WindowStats(unsigned W_) : W(W_), S(W_, 0.0) {}
  void record(double Q) {
    n += 1.0;
    ring.push_front(Q);
    if (ring.size() > W) ring.pop_back();
    a1 = ((n - 1.0) * a1 + Q) / (1.0 * n);
    for (unsigned k = 0; k < ring.size(); ++k) {
      const double N_k = n - k;
      S[k] = ((N_k - 1.0) * S[k] + ring[0] * ring[k]) / (1.0 * N_k);
    }
  }
  double tau_int() const {
    const double a2 = a1 * a1;
    double t = 0.0;
    for (unsigned k = 1; k < W; ++k) t += (1. - k / (1.0 * n)) * (S[k] - a2);
    return std::fmax(1.0, 1.0 + 2.0 * t / (S[0] - a2));
  }
  const unsigned W;
  double n = 0.0, a1 = 0.0;
  std::vector<double> S;
  std::deque<double> ring;
};

static void case_hierarchical() {
  const unsigned B = 3, n_draws = 12;
  HierarchicalParameters hp;
  hp.n_max_level = HL;
  hp.batch = B;
  hp.n_meas = N_MEAS;
  {
    // the replay alone: the first seed whose 12 draws show both outcomes
    uint64_t seed = 0;
    bool both = false;
    for (unsigned trial = 0; trial < 32 && !both; ++trial) {
      seed = SEED + trial;
      HierarchyReplay r(B, seed, seed, seed);
      for (unsigned k = 0; k < N_MEAS; ++k) hierarchical_replay_draw(r);
      unsigned n_acc = 0;
      for (unsigned k = 0; k < n_draws; ++k) n_acc += hierarchical_replay_draw(r);
      both = n_acc > 0 && n_acc < n_draws;
    }
    EXPECT(both, "hierarchical: no seed of 32 shows both an accepted and a rejected draw in %u: the case would pass vacuously", n_draws);
    if (both) {
      HierarchicalSampler sampler(hierarchy_fine_action(seed), std::make_shared<ExactSamplerFactory>(B), std::make_shared<GaussianConditionedFineActionFactory>(), hp);
      HierarchyReplay r(B, seed, seed, seed);  // HierarchicalSampler gives every level the fine action's seed
      double n_acc = 0.0;
      unsigned n_tot = 0, rejected = 0;
      for (unsigned k = 0; k < N_MEAS; ++k) {  // the constructor's timing draws: the sampler does not reset its counters after them
        n_acc += hierarchical_replay_draw(r) ? 1 : 0;
        n_tot++;
      }
      auto s = std::make_shared<SampleState>(HM[0], B);
      const Vec marker = known_state((size_t)HM[0] * B, 5);
      write_host(s, marker);
      Vec model = marker;
      for (unsigned k = 0; k < n_draws; ++k) {
        sampler.draw(s);
        const bool accept = hierarchical_replay_draw(r);
        n_acc += accept ? 1 : 0;
        n_tot++;
        rejected += !accept;
        if (accept) model = r.st[0]->get<double>();  // copy_if_rejected == false
        EXPECT(sampler.accepted() == accept, "hierarchical draw %u: accepted() = %d, the replay %d", k, (int)sampler.accepted(), (int)accept);
        EXPECT_SAME(dev_of(s), model, "hierarchical draw %u%s", k, accept ? "" : " (rejected)");
        EXPECT(sampler.p_accept() == n_acc / (1. * n_tot), "hierarchical draw %u: p_accept %.17g vs %.17g", k, sampler.p_accept(), n_acc / (1. * n_tot));
        for (unsigned l = 0; l < HL; ++l)
          EXPECT(eq(sampler.level_p_accept(l), r.lev_acc[l] / (1. * r.lev_tot[l])), "hierarchical draw %u: level %u p_accept %.17g vs %.17g (%g draws)", k, l,
                 sampler.level_p_accept(l), r.lev_acc[l] / (1. * r.lev_tot[l]), r.lev_tot[l]);
      }
      std::printf(" hierarchical: seed %llu, %u of %u draws rejected, %d failures so far\n", (unsigned long long)seed, rejected, n_draws, failures);
    }
  }
  {  // MultilevelSampler (one chain): the do ... while of draw(), with the windowed tau_int restated
    const unsigned window = 3, n_ml_draws = 10;
    hp.batch = 1;
    auto fine = hierarchy_fine_action(SEED);
    MultilevelSampler sampler(fine, std::make_shared<QoIXsquaredFactory>(), std::make_shared<ExactSamplerFactory>(1), std::make_shared<GaussianConditionedFineActionFactory>(), window, hp);
    HierarchyReplay r(1, SEED, SEED + 104729ull, SEED + 2 * 104729ull);  // multilevel.hh: seed + 104729 (ell + 1)
    std::vector<WindowStats> stats(HL, WindowStats(window));
    double t_indep[HL] = {0, 0, 0};
    unsigned n_indep[HL] = {0, 0, 0}, t_sampler[HL] = {0, 0, 0};
    unsigned long launches = 0;
    auto replay_draw = [&]() {
      int level = (int)HL - 1;
      do {
        if (level == (int)HL - 1) r.coarse_draw();
        else r.twolevel_draw(level);
        ++launches;
        check(mlmcpi_qoi_xsquared(r.st[level]->d(), HM[level], 1, r.q.d(), nullptr), "qoi_xsquared");
        stats[level].record(r.q.get<double>()[0]);
        t_sampler[level]++;
        double tau = std::ceil(stats[level].tau_int());
        if (!(tau <= 1. + 2. * window)) tau = 1. + 2. * window;
        if (t_sampler[level] >= tau) {
          t_indep[level] = (n_indep[level] * t_indep[level] + t_sampler[level]) / (1.0 + n_indep[level]);
          n_indep[level]++;
          t_sampler[level] = 0;
          level--;
        } else {
          level = (int)HL - 1;
        }
      } while (level >= 0);
    };
    for (unsigned k = 0; k < N_MEAS; ++k) replay_draw();  // the constructor's timing draws
    auto s = std::make_shared<SampleState>(HM[0], 1);
    for (unsigned k = 0; k < n_ml_draws; ++k) {
      sampler.draw(s);
      replay_draw();
      EXPECT_SAME(dev_of(s), r.st[0]->get<double>(), "multilevel sampler draw %u", k);
      for (unsigned l = 0; l < HL; ++l)
        EXPECT(sampler.independent_spacing(l) == t_indep[l], "multilevel sampler draw %u: t_indep[%u] = %.17g vs %.17g", k, l, sampler.independent_spacing(l), t_indep[l]);
    }
    std::printf(" multilevel sampler: %lu level draws for %u samples, t_indep = %g %g %g, %d failures so far\n", launches, N_MEAS + n_ml_draws, t_indep[0], t_indep[1],
                t_indep[2], failures);
  }
}

// =====================================================================================================================
// 8. the arithmetic of MonteCarloMultiLevel
// =====================================================================================================================
static const double UINT_TARGET_LIMIT = 4294967295.0;

/** montecarlomultilevel.cc:148-164 in long double, with the guard multilevel.hh documents: a target that is not finite or does not fit
 *  an unsigned int leaves the level's target where it was */
static bool update_restated(const Vec &table, double epsilon, std::vector<unsigned int> &n_target) {
  const unsigned L = (unsigned)n_target.size();
  const long double two_epsilon_inv2 = 2.0L / ((long double)epsilon * (long double)epsilon);
  long double sum = 0.0L;
  for (unsigned l = 0; l < L; ++l) sum += sqrtl((long double)table[5 * l + 2] * (long double)table[5 * l + 4]);
  bool sufficient = true;
  for (unsigned l = 0; l < L; ++l) {
    const long double V = table[5 * l + 2], C = table[5 * l + 4];
    const long double want = ceill(two_epsilon_inv2 * sum * sqrtl(V / C) * (long double)table[5 * l + 3]);
    if (std::isfinite(want) && want < (long double)UINT_TARGET_LIMIT) n_target[l] = (unsigned int)want;
    sufficient = sufficient && ((long double)table[5 * l] >= (long double)n_target[l]);
  }
  return sufficient;
}
static bool within_one_ulp(double got, long double want) {
  const double w = (double)want;
  return got == w || got == std::nextafter(w, -std::numeric_limits<double>::infinity()) || got == std::nextafter(w, std::numeric_limits<double>::infinity());
}

static void case_mlmc_table() {
  const unsigned L = 3, M = 32;
  const double epsilon = 0.05;
  auto make = [&](unsigned rank, unsigned ranks, uint64_t seed) {
    auto fine = std::make_shared<HarmonicOscillatorAction>(std::make_shared<Lattice1D>(M, 4.0), RenormalisationNone, 1.0, 1.0);
    fine->set_seed(seed, CHAIN0);
    MultiLevelMCParameters p;
    p.n_level = L;
    p.n_burnin = 2;
    p.epsilon = epsilon;
    p.n_autocorr_window = 3;
    p.n_min_samples_qoi = 4;
    p.n_meas = 1;
    p.level_rank = rank;
    p.level_ranks = ranks;
    HierarchicalParameters hp;  // the level samplers: hierarchical ones, which know their cost per sample
    hp.n_max_level = L;
    hp.batch = 1;
    hp.n_meas = 1;
    auto cfa = std::make_shared<GaussianConditionedFineActionFactory>();
    auto samplers = std::make_shared<HierarchicalSamplerFactory>(std::make_shared<ExactSamplerFactory>(1), cfa, hp);
    return std::make_shared<MonteCarloMultiLevel>(fine, std::make_shared<QoIXsquaredFactory>(), samplers, cfa, p);
  };
  auto mc = make(0, 1, SEED);
  std::vector<unsigned int> model(L, 4u);  // n_min_samples_qoi
  for (unsigned l = 0; l < L; ++l) EXPECT(mc->target_samples(l) == 4u, "initial target of level %u", l);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // rows: samples, mean, variance, tau_int, cost
  struct Table { const char *name; Vec t; bool finite[3]; };
  const std::vector<Table> tables = {
      {"(i) generic", {120, 0.4812, 0.0371, 1.37, 11.3, 64, 0.0219, 0.00412, 1.12, 23.9, 31, 0.00871, 0.00093, 1.05, 41.7}, {true, true, true}},
      {"(iii) a row with C = 0", {120, 0.4812, 0.0371, 1.37, 11.3, 64, 0.0219, 0.00412, 1.12, 0.0, 31, 0.00871, 0.00093, 1.05, 41.7}, {true, false, true}},
      {"(iv) a row with NaN tau_int", {120, 0.4812, 0.0371, 1.37, 11.3, 64, 0.0219, 0.00412, 1.12, 23.9, 31, 0.00871, 0.00093, nan, 41.7}, {true, true, false}},
      {"(v) a target beyond 2^32 - 1", {120, 0.4812, 3.1e9, 1.37, 11.3, 64, 0.0219, 0.00412, 1.12, 23.9, 31, 0.00871, 0.00093, 1.05, 41.7}, {false, true, true}},
      // last: the target of 0 it leaves must not be what a row without a usable target has to keep
      {"(ii) a row with V = 0", {120, 0.4812, 0.0371, 1.37, 11.3, 64, 0.0219, 0.0, 1.12, 23.9, 31, 0.00871, 0.00093, 1.05, 41.7}, {true, true, true}},
  };
  for (const Table &tb : tables) {
    const std::vector<unsigned int> before = model;
    const bool want = update_restated(tb.t, epsilon, model);
    const bool got = mc->update(tb.t);
    EXPECT(got == want, "%s: update returned %d, the restatement %d", tb.name, (int)got, (int)want);
    for (unsigned l = 0; l < L; ++l) {
      EXPECT(mc->target_samples(l) == model[l], "%s: target of level %u = %u, the restatement %u", tb.name, l, mc->target_samples(l), model[l]);
      if (!tb.finite[l]) EXPECT(mc->target_samples(l) == before[l] && before[l] != 0, "%s: level %u has no usable target and must keep %u, has %u", tb.name, l, before[l], mc->target_samples(l));
    }
    long double q = 0.0L, e2 = 0.0L;
    for (unsigned l = 0; l < L; ++l) {
      q += (long double)tb.t[5 * l + 1];
      e2 += (long double)tb.t[5 * l + 3] * (long double)tb.t[5 * l + 2] / (long double)tb.t[5 * l];
    }
    EXPECT(within_one_ulp(mc->numerical_result(), q), "%s: numerical_result %.17g vs %.21Lg", tb.name, mc->numerical_result(), q);
    if (std::isfinite((double)e2)) EXPECT(within_one_ulp(mc->statistical_error(), sqrtl(e2)), "%s: statistical_error %.17g vs %.21Lg", tb.name, mc->statistical_error(), sqrtl(e2));
    else EXPECT(std::isnan(mc->statistical_error()), "%s: statistical_error of a NaN row must be NaN", tb.name);
    std::printf(" %s: targets %u %u %u\n", tb.name, mc->target_samples(0), mc->target_samples(1), mc->target_samples(2));
  }
  {  // (vi) targets exactly met, and one sample short
    Vec t = tables[0].t;
    std::vector<unsigned int> target(L, 4u);
    update_restated(t, epsilon, target);  // the targets do not depend on the sample column
    for (unsigned l = 0; l < L; ++l) t[5 * l] = target[l];
    model = target;
    EXPECT(mc->update(t) == true, "(vi) targets exactly met: sufficient must be true");
    for (unsigned l = 0; l < L; ++l) {
      EXPECT(mc->target_samples(l) == target[l], "(vi) target of level %u = %u, the restatement %u", l, mc->target_samples(l), target[l]);
      Vec u = t;
      u[5 * l] -= 1.0;
      EXPECT(mc->update(u) == false, "(vi) level %u one sample short: sufficient must be false", l);
    }
  }
  // level sharding
  for (unsigned ranks : {2u, 3u}) {
    std::vector<std::shared_ptr<MonteCarloMultiLevel>> r;
    for (unsigned rank = 0; rank < ranks; ++rank) r.push_back(make(rank, ranks, SEED + 10 * rank));
    for (unsigned rank = 0; rank < ranks; ++rank)
      for (unsigned l = 0; l < L; ++l) EXPECT(r[rank]->owns(l) == (l % ranks == rank), "owns(%u) of rank %u of %u", l, rank, ranks);
    if (ranks != 2) continue;
    Vec sum(5 * L, 0.0);
    for (unsigned rank = 0; rank < ranks; ++rank) {
      r[rank]->begin();
      const Vec t = r[rank]->pass();
      for (unsigned l = 0; l < L; ++l)
        for (unsigned j = 0; j < 5; ++j) {
          if (!r[rank]->owns(l)) EXPECT(t[5 * l + j] == 0.0 && !std::signbit(t[5 * l + j]), "pass() of rank %u: entry %u of the unowned level %u is %g", rank, j, l, t[5 * l + j]);
          else if (j == 0) EXPECT(t[5 * l] == 4.0, "pass() of rank %u: level %u has %g samples, the target is 4", rank, l, t[5 * l]);
          sum[5 * l + j] += t[5 * l + j];
        }
    }
    const bool s0 = r[0]->update(sum), s1 = r[1]->update(sum);
    const double q0 = r[0]->numerical_result(), q1 = r[1]->numerical_result(), e0 = r[0]->statistical_error(), e1 = r[1]->statistical_error();
    EXPECT(s0 == s1, "two lock-stepped ranks disagree on `sufficient`");
    EXPECT(!std::memcmp(&q0, &q1, sizeof(double)), "two lock-stepped ranks: numerical_result %.17g vs %.17g", q0, q1);
    EXPECT(!std::memcmp(&e0, &e1, sizeof(double)), "two lock-stepped ranks: statistical_error %.17g vs %.17g", e0, e1);
    for (unsigned l = 0; l < L; ++l) EXPECT(r[0]->target_samples(l) == r[1]->target_samples(l), "two lock-stepped ranks: target of level %u", l);
    std::printf(" two ranks: Q = %.12g +/- %.3g\n", q0, e0);
  }
}

int main(int argc, char **argv) {
  const std::vector<std::pair<std::string, void (*)()>> cases = {
      {"samplestate", case_samplestate},   {"heatbath_sweeps", case_heatbath_sweeps}, {"heatbath_random", case_heatbath_random}, {"hmc", case_hmc},
      {"exact_and_cluster", case_exact_and_cluster}, {"twolevel", case_twolevel}, {"hierarchical", case_hierarchical}, {"mlmc_table", case_mlmc_table},
  };
  if (argc == 2)
    for (const auto &c : cases)
      if (c.first == argv[1]) {
        std::printf("case %s\n", argv[1]);
        c.second();
        if (failures) {
          std::printf("%d checks FAILED\n", failures);
          return 1;
        }
        std::printf("all checks passed\n");
        return 0;
      }
  std::fprintf(stderr, "usage: test_replay CASE, with CASE one of");
  for (const auto &c : cases) std::fprintf(stderr, " %s", c.first.c_str());
  std::fprintf(stderr, "\n");
  return 2;
}
