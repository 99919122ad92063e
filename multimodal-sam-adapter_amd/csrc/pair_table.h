// The open-addressing pair table, once: csrc/pairs.hip (label segment x prediction segment of one frame) and csrc/track.hip (current segment x previous
// segment of a stream) fill it with the same device code.
// The table.  keys int64 [capacity] (all-ones: empty), counts int32 [capacity], capacity a power of two.  A key is below 2^62 and never all-ones.
// A wave first reduces its lanes per distinct key in registers (the form of comp_wave_add, the key's halves through readlane), PAIR_WAVE_ROUNDS = 8 rounds
// at the most; what is pending after them goes lane by lane (pair_wave_reduce; the round counts that were timed: header of csrc/pairs.hip).  Every lane that
// then holds a (key, n) inserts it (pair_insert): slot = the top log2(capacity) bits of key * 2^64 / phi, then linear probing.  ONE atomicCAS(empty -> key)
// per slot, and its return value alone decides: empty or the same key -- atomicAdd(counts[slot], n), done; another key -- the next slot.  Keys are written
// once and never change, so no lane ever waits for a value another lane must write, and the loop is bounded by PAIR_MAX_PROBES = 128 slots (and by the
// capacity): a key that finds no slot adds its n to *overflow and is dropped -- the caller must look.
// Which key sits in which slot depends on the order of arrival; the SET of occupied slots of a linear-probing table does not (as long as nothing is
// dropped), and neither does the multiset of (key, count).
#pragma once
#include "common.h"

#ifndef PAIR_MAX_PROBES
#define PAIR_MAX_PROBES 128                   // slots a key looks at before it is dropped into *overflow
#endif
#ifndef PAIR_WAVE_ROUNDS
#define PAIR_WAVE_ROUNDS 8                    // rounds of the in-wave reduction (64: one inserting lane per distinct key, whatever the wave holds)
#endif
#define PAIR_EMPTY 0xffffffffffffffffull
#define PAIR_HASH_MUL 0x9e3779b97f4a7c15ull   // 2^64 / phi, odd
#define PAIR_MAX_LOG2 30                      // capacity <= 2^30 slots

struct PairTable {
  unsigned long long* keys;         // [capacity]
  int* counts;                      // [capacity]
  int* overflow;                    // [1]
  int log2cap;                      // 1 .. 30
};

__device__ __forceinline__ unsigned pair_slot(unsigned long long key, int log2cap) {      // < 2^log2cap
  return (unsigned)((key * PAIR_HASH_MUL) >> (64 - log2cap));
}

__device__ __forceinline__ void pair_insert(const PairTable& t, unsigned long long key, int n) {
  const unsigned mask = (1u << t.log2cap) - 1u;
  const int probes = (int)min((unsigned)PAIR_MAX_PROBES, mask + 1u);
  unsigned at = pair_slot(key, t.log2cap) & mask;
  for (int p = 0; p < probes; ++p) {
    const unsigned long long old = atomicCAS(&t.keys[at], PAIR_EMPTY, key);
    if (old == PAIR_EMPTY || old == key) {
      atomicAdd(&t.counts[at], n);
      return;
    }
    at = (at + 1u) & mask;
  }
  atomicAdd(t.overflow, n);
}

// Called by all 64 lanes of a wave together; `pending`: this lane holds `key`.  -> n > 0 in the lanes that insert (key, n): the first lane of every key
// that a round retired with the number of its lanes, and 1 in every lane that is still pending after the rounds; 0 elsewhere.
__device__ __forceinline__ int pair_wave_reduce(bool pending, unsigned long long key) {
  const unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
  int n = 0;
  unsigned long long live = __ballot(pending);
  for (int r = 0; r < PAIR_WAVE_ROUNDS && live != 0ull; ++r) {
    const int lead = __ffsll((long long)live) - 1;
    const unsigned llo = __builtin_amdgcn_readlane(lo, lead), lhi = __builtin_amdgcn_readlane(hi, lead);
    const bool same = pending && lo == llo && hi == lhi;
    const unsigned long long ms = __ballot(same);
    if ((int)(threadIdx.x & 63u) == lead) n = (int)__popcll(ms);
    pending = pending && !same;
    live &= ~ms;
  }
  if (pending) n = 1;                                                          // beyond the rounds: lane by lane
  return n;
}

static inline int pair_check_table(const char* name, const void* keys, const void* counts, long capacity, int* log2cap) {
  MMSA_CHECK_ARG(keys && counts, "%s: keys and counts are required", name);
  int lg = 0;
  while (lg < PAIR_MAX_LOG2 && (1l << lg) < capacity) ++lg;
  MMSA_CHECK_ARG(capacity >= 2 && (1l << lg) == capacity, "%s: capacity = %ld; a power of two, 2 .. 2^%d slots, is expected", name, capacity, PAIR_MAX_LOG2);
  *log2cap = lg;
  return MMSA_OK;
}
