// What the multi-tensor optimizer kernels share (optim.hip: Adam, sgd.hip: SGD with momentum): the chunk a workgroup owns
// and the scan that finds its tensor in the table that travels in the kernel arguments.
#pragma once
#include "common.h"

namespace yolo {

constexpr int MT_CHUNK = 8192;  // elements per workgroup: 256 lanes x float4 x 8

__device__ __forceinline__ int find_tensor(const int *first, int count, int b)
{
    int i = 0;
    while (i + 1 < count && first[i + 1] <= b) ++i;  // wave-uniform scalar scan of <= 48 entries
    return i;
}

}  // namespace yolo
