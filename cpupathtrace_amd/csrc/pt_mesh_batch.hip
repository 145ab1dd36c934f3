// pt_mesh_batch.hip -- the batched mesh assembler for the device (pt_mesh_batch.h): the kernels and their chain are
// pt_mesh_batch_kernels.h, this unit adds the two library steps, hipcub's exclusive sum and stable radix sort.
// Compiled with -ffp-contract=off and correctly rounded divide / sqrt like the rest: every operation is the IEEE operation of the host code.
#include "pt_mesh_batch_kernels.h"

#include <hipcub/hipcub.hpp>

hipError_t pt_mesh_batch_scan(void *temp, size_t *bytes, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(temp, *bytes, in, out, static_cast<int>(n), stream);
}

hipError_t pt_mesh_batch_sort(void *temp, size_t *bytes, const uint32_t *keys_in, uint32_t *keys_out, const uint32_t *values_in, uint32_t *values_out, uint32_t n, int end_bit,
                              hipStream_t stream) {
    return hipcub::DeviceRadixSort::SortPairs(temp, *bytes, keys_in, keys_out, values_in, values_out, static_cast<int>(n), 0, end_bit, stream);
}
