// What every piece of the probe shares: the native vector types of the kernels, the error every
// host step throws and the check that turns a HIP status into it.
#pragma once

#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#define PROBE_CHECK(expr)                                                                 \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      throw ProbeError(std::string(#expr) + " -> " + hipGetErrorString(e_));             \
    }                                                                                     \
  } while (0)

namespace {

struct ProbeError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;  // native vector: 16-B global ops
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __attribute__((address_space(3))) void lds_void_t;  // global_load_lds destination

}  // namespace
