#pragma once
// Hand-overs between workgroups of a grid that are all still running (DESIGN.md 3.10 lists every one): the producer
// stores its data write-through (relaxed agent-scope stores: global_store ... sc1), waits until they have been
// acknowledged (drain_stores), then publishes one word with a relaxed agent-scope store or atomic; the consumer polls that
// word in a bounded loop with relaxed agent-scope loads (global_load ... sc1: served by the L2, never by its own L1) and
// reads the data the same way.  No cache write-back or invalidation is involved on either side.
#include "riab_device.h"

namespace riab {

typedef __attribute__((address_space(1))) uint32_t riab_g32;
typedef __attribute__((address_space(1))) unsigned long long riab_g64;

// ---- relaxed, agent-scope accesses
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) {
  __hip_atomic_store((riab_g32*)(uintptr_t)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load((riab_g32*)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int32_t* p, int32_t v) { st_agent(reinterpret_cast<uint32_t*>(p), (uint32_t)v); }
__device__ __forceinline__ int32_t ld_agent(const int32_t* p) { return (int32_t)ld_agent(reinterpret_cast<const uint32_t*>(p)); }
__device__ __forceinline__ void st_agent(uint64_t* p, uint64_t v) {
  __hip_atomic_store((riab_g64*)(uintptr_t)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
  return (uint64_t)__hip_atomic_load((riab_g64*)(uintptr_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double* p, double v) { st_agent(reinterpret_cast<uint64_t*>(p), (uint64_t)__double_as_longlong(v)); }
__device__ __forceinline__ double ld_agent(const double* p) {
  return __longlong_as_double((long long)ld_agent(reinterpret_cast<const uint64_t*>(p)));
}
__device__ __forceinline__ void st_agent(float* p, float v) { st_agent(reinterpret_cast<uint32_t*>(p), __float_as_uint(v)); }
__device__ __forceinline__ void st_agent(uint8_t* p, uint8_t v) {
  __hip_atomic_store((__attribute__((address_space(1))) uint8_t*)(uintptr_t)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t fetch_add_agent(uint32_t* p, uint32_t v) {
  return __hip_atomic_fetch_add((riab_g32*)(uintptr_t)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t fetch_add_agent(int32_t* p, int32_t v) {
  return (int32_t)fetch_add_agent(reinterpret_cast<uint32_t*>(p), (uint32_t)v);
}
__device__ __forceinline__ uint64_t fetch_max_agent(uint64_t* p, uint64_t v) {
  return (uint64_t)__hip_atomic_fetch_max((riab_g64*)(uintptr_t)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16 bytes write-through / past the L1: two 8-byte relaxed agent-scope accesses (global_store_dwordx2 / global_load_dwordx2 ... sc1)
__device__ __forceinline__ void st_agent_v4f(void* p, riab_v4f v) {
  riab_g64* const g = (riab_g64*)(uintptr_t)p;
  __hip_atomic_store(g, ((unsigned long long)__float_as_uint(v.y) << 32) | __float_as_uint(v.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(g + 1, ((unsigned long long)__float_as_uint(v.w) << 32) | __float_as_uint(v.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ riab_v4f ld_agent_v4f(const void* p) {
  riab_g64* const g = (riab_g64*)(uintptr_t)p;
  const unsigned long long lo = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long hi = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return riab_v4f{__uint_as_float((uint32_t)lo), __uint_as_float((uint32_t)(lo >> 32)), __uint_as_float((uint32_t)hi),
                  __uint_as_float((uint32_t)(hi >> 32))};
}

// ---- the wave's stores (and atomics) have been acknowledged: what it wrote through is in the L2 for every reader.  A
// workgroup barrier does not wait for them (the compiler puts `lgkmcnt(0)` in front of it, not `vmcnt(0)`).
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// The same wait without an asm statement, for a site where one costs an instantiation a stack frame.  The immediate is
// gfx9's s_waitcnt encoding: vmcnt 0 (bits 3:0 and 15:14), expcnt 7 (bits 6:4) and lgkmcnt 15 (bits 11:8), i.e. no wait
// on the other two counters.  The builtin alone is no compiler barrier (LLVM declares it IntrNoMem); the signal fences
// keep memory operations from being moved across it.
#define RIAB_WAITCNT_VMCNT0 0x0F70
__device__ __forceinline__ void drain_stores_nofence_asm() {
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(RIAB_WAITCNT_VMCNT0);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// ---- epoch-tagged mail: an 8-byte entry carries the launch's epoch with its value, so no entry has to be ordered
// against another: a reader takes an entry once it is fresh
__device__ __forceinline__ uint64_t mail_word(uint32_t epoch, uint32_t v) { return ((uint64_t)epoch << 32) | v; }
__device__ __forceinline__ bool mail_fresh(uint64_t e, uint32_t epoch) { return (uint32_t)(e >> 32) == epoch; }

}  // namespace riab
