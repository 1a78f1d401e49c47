// hip_try.hpp -- the HIP-call check of the C-ABI translation units: a failed call becomes CERES_EHIP
// with the message "<the call as written>: <HIP's error string>".
#pragma once
#include <hip/hip_runtime_api.h>

#include "ceres_render.h"
#include "host_common.hpp"

// returns the status from the enclosing function
#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return ceres::set_error(CERES_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// for functions with one exit: sets their `rc` and jumps to their `done` label
#define HIP_TRY_DONE(expr)                                                                                               \
    do {                                                                                                                 \
        hipError_t e_ = (expr);                                                                                          \
        if (e_ != hipSuccess) { rc = ceres::set_error(CERES_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); goto done; } \
    } while (0)
