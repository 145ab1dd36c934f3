// TEST ONLY: the host stand-in for the HIP runtime (tests/hip/host) with what tests/hip/pose_probe.hip and the batched mesh assembler
// (pt_mesh_batch_kernels.h) need on top of it.  tests/pose_probe.py compiles the probe against this directory.
#pragma once
#include "../../host/hip/hip_runtime.h"
enum { hipErrorInvalidValue = 1, hipErrorUnknown = 999 };
#ifndef __restrict__
#define __restrict__ __restrict
#endif
