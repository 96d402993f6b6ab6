// The error mechanism of the C ABI, shared by libocc4d.so (csrc/common.hpp) and the g++ twin (csrc_cpu/occ4d_twin.cpp): no HIP
// in here.  Each library defines occ4d::set_error over its own thread-local buffer, so an argument contract written once with
// these macros (the host-only check_* functions of the *_math.hpp headers) fails with the same status and text in both.
#pragma once
#include <stdint.h>

#include "occ4d.h"

namespace occ4d {
void set_error(const char* fmt, ...);
}

#define OCC4D_REQUIRE(cond, ...)        \
  do {                                  \
    if (!(cond)) {                      \
      occ4d::set_error(__VA_ARGS__);    \
      return OCC4D_EINVAL;              \
    }                                   \
  } while (0)

#define OCC4D_TRY(expr)                 \
  do {                                  \
    const int rc_ = (expr);             \
    if (rc_ != OCC4D_OK) return rc_;    \
  } while (0)
