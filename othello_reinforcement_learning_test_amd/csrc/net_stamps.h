// net_stamps.h -- the in-kernel clocks of the diagnostic builds of the fp16-split trunks (-DOTH_STAMPS: s_memtime phase
// stamps, tools/build_variant.sh).  Never compiled into the shipped library.
#pragma once
#ifdef OTH_STAMPS
namespace oth {
__device__ __forceinline__ unsigned long long oth_clk() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
__device__ __forceinline__ unsigned long long oth_realclk() {   // 100 MHz constant clock
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
}  // namespace oth
#endif
