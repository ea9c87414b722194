// test_math.hip -- mlmcpi_test_math: the device math primitives, one function per call (tests/test_device_math_gpu.py).  The
// only unit in which the primitives of the two-level fill-ins (fillin.hpp) and of the sigma model (sigma_device.hpp, which
// switches fp contraction off for what follows it) meet; test_math_kernel only calls functions whose bodies were compiled
// where they are defined.
#include "internal.hpp"
#include "vonmises.hpp"
#include "fillin.hpp"
#include "sigma_device.hpp"

namespace mlmcpi {

// (out0[k], out1[k]) = fn(a[k], b[k]): mlmcpi_math_fn in include/mlmcpi_hip.h.  `b` is read by the functions of two operands only.
__global__ void __launch_bounds__(256)
    test_math_kernel(uint32_t fn, const double *a, const double *b, uint32_t n, double *out0, double *out1) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double x = a[k];
  const uint64_t bits = (uint64_t)__double_as_longlong(x);
  const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
  double r0 = 0.0, r1 = 0.0;
  switch (fn) {
    case MLMCPI_MATH_FAST_RCP: r0 = fast_rcp(x); break;
    case MLMCPI_MATH_FAST_DIV: r0 = fast_div(x, b[k]); break;
    case MLMCPI_MATH_FAST_SQRT: r0 = fast_sqrt(x); break;
    case MLMCPI_MATH_FAST_ACOS: r0 = fast_acos(x); break;
    case MLMCPI_MATH_SIN_REDUCED: r0 = sin_reduced(x); break;
    case MLMCPI_MATH_COSPI_UNIT: r0 = cospi_unit(x); break;
    case MLMCPI_MATH_COS_REDUCED: r0 = cos_reduced(x); break;
    case MLMCPI_MATH_COS_HALF: r0 = cos_half(x); break;
    case MLMCPI_MATH_LOG_UNIT: r0 = log_unit(x); break;
    case MLMCPI_MATH_SINCOS_2PI_UNIT: sincos_2pi_unit(x, r0, r1); break;
    case MLMCPI_MATH_BOX_MULLER: box_muller(x, b[k], r0, r1); break;
    case MLMCPI_MATH_MOD_2PI: r0 = mod_2pi(x); break;
    case MLMCPI_MATH_MOD_2PI_FAST: r0 = mod_2pi_fast(x); break;
    case MLMCPI_MATH_U01: r0 = u01(lo, hi); break;
    case MLMCPI_MATH_U01_52: r0 = u01_52(lo, hi); break;
    case MLMCPI_MATH_VM_ENVELOPE: r0 = vm_envelope(x); break;
    case MLMCPI_MATH_BESSEL_I0_SCALED: r0 = bessel_i0_scaled(x); break;
    case MLMCPI_MATH_TWO_PI_I0_SCALED: r0 = two_pi_i0_scaled(x); break;
    case MLMCPI_MATH_BESSEL_I0: r0 = bessel_i0(x); break;
    case MLMCPI_MATH_COMPACT_EXP_INVERSE: r0 = compact_exp_inverse(x, b[k]); break;
    case MLMCPI_MATH_VM_TRY: {
      const double kappa = b[k];
      double f;
      r1 = (double)vm_try(lo, hi, kappa, vm_envelope(kappa), f, r0);
      break;
    }
    case MLMCPI_MATH_VM_SCREEN: {
      float af, band;
      vm_screen(x, af, band);
      r0 = (double)af;
      r1 = (double)band;
      break;
    }
    case MLMCPI_MATH_VM_EXACT: {
      const double m = floor(b[k]);
      r0 = (double)vm_exact((uint32_t)m << 1, b[k] - m, x);
      break;
    }
    default: break;  // (the host refuses an unknown fn before the launch)
  }
  out0[k] = r0;
  out1[k] = r1;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_test_math(uint32_t fn, const double *d_a, const double *d_b, uint32_t n, double *d_out0, double *d_out1, void *stream) {
  MLMCPI_REQUIRE(fn < MLMCPI_MATH_COUNT, "unknown function %u", fn);
  const bool two_operands = fn == MLMCPI_MATH_FAST_DIV || fn == MLMCPI_MATH_BOX_MULLER || fn == MLMCPI_MATH_COMPACT_EXP_INVERSE ||
                            fn == MLMCPI_MATH_VM_TRY || fn == MLMCPI_MATH_VM_EXACT;
  MLMCPI_REQUIRE(d_a && d_out0 && d_out1 && n > 0 && (d_b || !two_operands), "bad arguments");
  hipLaunchKernelGGL(test_math_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), fn, d_a, d_b, n, d_out0, d_out1);
  MLMCPI_LAUNCH_CHECK("test_math_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
