// store_run.h -- a lane's run of kRun consecutive floats of one row into global memory, 16 bytes wide where the address
// allows. Shared by the kernels that write float input planes from uint8 pixels (image_fill.hip, augment.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bcnn_hip {

constexpr int kRun = 8;          // destination pixels of one row per lane

// Stores a full run v[0 .. kRun) to d: HEAD scalar stores up to the first 16-byte boundary, 16-byte stores, scalar tail.
// HEAD is a template argument so that every index into v is a compile-time constant (v stays in registers).
template <int HEAD>
__device__ __forceinline__ void store_full_run(float* __restrict__ d, const float (&v)[kRun]) {
    static_assert(kRun == 8, "one 16-byte store after a head, two without");
#pragma unroll
    for (int j = 0; j < HEAD; ++j) d[j] = v[j];
    *reinterpret_cast<float4*>(d + HEAD) = make_float4(v[HEAD], v[HEAD + 1], v[HEAD + 2], v[HEAD + 3]);
    if (HEAD == 0) {
        *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int j = HEAD + 4; j < kRun; ++j) d[j] = v[j];
    }
}
// Stores v[0 .. len) to d; a run cut short by the end of its row (len < kRun) goes out in scalar stores.
__device__ __forceinline__ void store_run(float* __restrict__ d, const float (&v)[kRun], int len) {
    if (len == kRun) {
        switch ((4 - (int)((reinterpret_cast<uintptr_t>(d) >> 2) & 3)) & 3) {  // floats up to the 16-byte boundary
            case 0: store_full_run<0>(d, v); break;
            case 1: store_full_run<1>(d, v); break;
            case 2: store_full_run<2>(d, v); break;
            default: store_full_run<3>(d, v); break;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRun - 1; ++j)
            if (j < len) d[j] = v[j];
    }
}

}  // namespace bcnn_hip
