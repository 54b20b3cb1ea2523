// Device helpers shared by the global-memory hash tables off the per-batch hot path (roll-up, positions) and by the
// kernels that dump a table's live slots: one probe loop (find, or find-or-claim by CAS) and one workgroup compaction.
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// open addressing over slots with a 64-bit key word, linear probing from `home` over mask + 1 slots
// =====================================================================================================
constexpr unsigned long long TAB_NONE = ~0ull;   // no slot: the probe bound ran out (or, reading only, a free slot ended the chain)
// the "matches" rules: is the key word `cur` of an occupied slot the one looked for?
struct TabNoMatch {   // claim only: the caller guarantees that the key is not in the table and that no other thread brings it
    __device__ bool operator()(unsigned long long) const { return false; }
};
struct TabKeyIs {     // equality, ignoring the flag bits `ignore`
    unsigned long long key, ignore;
    __device__ bool operator()(unsigned long long cur) const { return (cur & ~ignore) == key; }
};
// The slot of the chain from `home` whose key word matches, at most min(probes, mask + 1) slots on; key_at(i) = the
// address of slot i's key word, `empty` = the word of a free slot.
//  CLAIM   the first free slot met before a match is claimed by a CAS of `store` over `empty`.  The key word is read by
//          a relaxed agent-scope load first and the CAS only tried on `empty`: a stale read can only be `empty`, and
//          the CAS then returns the slot's owner, which is matched like any other occupant.  seen = the slot's key
//          word as found: `empty` iff this thread claimed it.  TAB_NONE: the bound ran out.
//  !CLAIM  read only (plain loads: the table holds what earlier launches wrote); a free slot ends the chain: TAB_NONE.
template <bool CLAIM, class KeyAt, class Match>
__device__ __forceinline__ unsigned long long tab_probe(KeyAt key_at, unsigned long long mask, unsigned long long home,
                                                        unsigned long long probes, unsigned long long empty,
                                                        unsigned long long store, Match match, unsigned long long &seen) {
    unsigned long long at = home;
    for (unsigned long long q = 0; q < probes && q <= mask; q++) {
        auto *kp = key_at(at);
        unsigned long long cur;
        if constexpr (CLAIM) {
            cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == empty) cur = atomicCAS(kp, empty, store);
        } else {
            cur = *kp;
            if (cur == empty) break;
        }
        if (cur == empty || match(cur)) {
            seen = cur;
            return at;
        }
        at = (at + 1) & mask;
    }
    return TAB_NONE;
}

// =====================================================================================================
// compaction of a table's live slots into a dense output, by a workgroup of 256 threads
// =====================================================================================================
// Each workgroup iteration reads DUMP_PER x 256 consecutive slots (coalesced: slot k * 256 + tid) and appends its live
// ones with ONE atomic on the shared counter: a wave-aggregated append still made one same-address atomic per wave --
// 1.5 M of them over three 2^25-slot windows serialised at the L2 (12.7 ms for a 1e7-key delta, profiles/r6/r6w2).
// The order within an iteration is wave-major, then k, then lane; the order of the iterations in the output is
// whatever the atomics make it (irrelevant to every caller: growth re-partitions, checkpoints and exports are key sets).
constexpr int DUMP_PER = 8;
// base: the iteration's first slot.  is_live(i): slot i is live (it also tests i against the table's size); emit(i, at)
// is then called for it with its index in the output, and reads the slot's body only then (nothing of it is kept across
// the barriers).  The callbacks capture by value: by reference, a record copied through them stays in memory.
// CAPPED: an index >= out_cap is counted in *counter but not emitted.  Every thread of the workgroup calls this once
// per iteration (barriers inside; the last one lets the next iteration reuse the LDS words).
template <bool CAPPED, class Live, class Emit>
__device__ __forceinline__ void block256_compact(int64_t base, Live is_live, unsigned long long *counter,
                                                 unsigned long long out_cap, Emit emit) {
    __shared__ unsigned wave_n[4];
    __shared__ unsigned long long blk_base;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned long long below = (UINT64_C(1) << lane) - 1;
    bool live[DUMP_PER];
    unsigned long long m[DUMP_PER];
    unsigned wtot = 0;
#pragma unroll
    for (int k = 0; k < DUMP_PER; k++) {
        live[k] = is_live(base + k * 256 + threadIdx.x);
        m[k] = __ballot(live[k]);
        wtot += __popcll(m[k]);
    }
    // the wave's k-th records go after its records of earlier k, in lane order
    if (lane == 0) wave_n[wave] = wtot;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        blk_base = tot ? atomicAdd(counter, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long pos = blk_base;
    for (int w = 0; w < wave; w++) pos += wave_n[w];
#pragma unroll
    for (int k = 0; k < DUMP_PER; k++) {
        const unsigned long long at = pos + __popcll(m[k] & below);
        if (live[k] && (!CAPPED || at < out_cap)) emit(base + k * 256 + threadIdx.x, at);
        pos += __popcll(m[k]);
    }
    __syncthreads();   // (wave_n / blk_base reused by the next iteration)
}
