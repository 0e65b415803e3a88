// The function attributes of the headers that compile for the device AND as plain C++17 for the host programs of tests/stubs/.
#pragma once

#if defined(__HIPCC__)
#define GVI_HD __host__ __device__
#define GVI_HD_INLINE __host__ __device__ __forceinline__
#define GVI_UNROLL _Pragma("unroll")     // short compile-time loops: their arrays stay in registers
#else
#define GVI_HD
#define GVI_HD_INLINE inline
#define GVI_UNROLL
#endif
