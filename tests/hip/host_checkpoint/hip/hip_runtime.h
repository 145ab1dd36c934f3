// TEST ONLY: the host stand-in for the HIP runtime (tests/hip/host_query) with what tests/hip/checkpoint_probe.hip and the PT_D functions
// of pt_checkpoint_kernels.h need on top of it.  tests/checkpoint_probe.py compiles the probe against this directory.
#pragma once
#include "../../host_query/hip/hip_runtime.h"
inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
