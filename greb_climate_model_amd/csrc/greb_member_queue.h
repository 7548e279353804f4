// greb_member_queue.h -- the ready queue of a dealt launch of the fused member kernel: the item words and how a workgroup
// pops its next (member, chunk) item and pushes the member's next chunk (greb_member.hip, "The deal of member-year
// chunks", says what a chunk is and why it is dealt).
//
// The queue: `q_capacity` = members x chunks item words behind a head and a tail counter, re-made on the stream before
// every launch with chunk 0 of every member in the first `members` slots.  A workgroup takes the next INDEX (atomic add on
// head), leaves when that is beyond the capacity, else waits until the slot is filled; having run the chunk it pushes the
// member's next one (atomic add on tail, store of the item).  A slot below the capacity is always filled in the end: by
// the image, or by a workgroup that holds an item and is therefore running -- nothing depends on which workgroups are
// resident or in what order they start.  The wait is bounded all the same (kCircSpinTicks); a workgroup that gives up sets
// q_status, which ends every other wait, and the host reports it (greb_engine.cpp: finish_years).
// A member's next chunk usually runs on another XCD, whose L2 may hold lines of that member from an earlier chunk: the
// push is a release at agent scope behind a workgroup barrier, the pop an acquire at agent scope in front of the first
// load of the member's data.  Only scalars (m, s0, s1) depend on the item.
#pragma once

#include "greb_kernels.h"
#include "greb_member_lds.h"

namespace greb {

__device__ __forceinline__ int item_member(unsigned item) { return (int)((item - 1u) >> 4); }
__device__ __forceinline__ int item_chunk(unsigned item) { return (int)((item - 1u) & 15u); }
__device__ __forceinline__ __attribute__((address_space(3))) unsigned* item_words(lfloat* lds) {
  return (__attribute__((address_space(3))) unsigned*)(lds + kLdsItemWord);
}
// word i of the two, block-uniform, read anew wherever it is used
__device__ __forceinline__ unsigned item_word(lfloat* lds, int i) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)*(volatile __attribute__((address_space(3))) unsigned*)(item_words(lds) + i));
}
// the next item of this workgroup, in every thread (block-uniform); 0: none -- the queue is drained, or the wait was given up
__device__ __forceinline__ unsigned pop_item(const MemberArgs& a, lfloat* lds) {
  __attribute__((address_space(3))) unsigned* word = item_words(lds) + 2; // (a word of its own: see member_kernel on the other two)
  if (threadIdx.x == 0) {
    unsigned item = 0u;
    const unsigned idx = __hip_atomic_fetch_add(a.queue + kQHead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (idx < a.q_capacity) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        item = __hip_atomic_load(a.queue + kQItems + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (item != 0u) break;
        if (__hip_atomic_load(a.q_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break; // somebody gave up
        if (__builtin_amdgcn_s_memrealtime() - t0 > kCircSpinTicks) {
          __hip_atomic_store(a.q_status + 1, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(a.q_status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(64); // ~4 000 cycles between two polls
      }
    }
    *word = item;
  }
  __syncthreads(); // (the word is not written again before every thread has passed the barrier behind the prologue)
  const unsigned item = (unsigned)__builtin_amdgcn_readfirstlane((int)*word);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return item;
}

// after the last step of a chunk: hand the member on
__device__ __forceinline__ void push_next(const MemberArgs& a, unsigned item) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // every wave's stores of the chunk ...
  __syncthreads();
  if (threadIdx.x == 0 && item_chunk(item) + 1 < a.chunks.n) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); // ... in front of the item
    const unsigned slot = __hip_atomic_fetch_add(a.queue + kQTail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot < a.q_capacity) // (item + 1: the same member's next chunk)
      __hip_atomic_store(a.queue + kQItems + slot, item + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

} // namespace greb
