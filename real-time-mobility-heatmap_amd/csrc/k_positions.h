// Latest position per (provider, vehicleId) across batches, on the device: the fold the reference leaves to MongoDB
// (heatmap_stream.py:217-228, UpdateOne with {ts: {$lt: ts}} and upsert).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// A batch's vkey is provider_code * n_vehicles + vehicle_code of that batch's own dictionaries, so the state is keyed by
// the strings themselves.  Three tables, all open addressing with linear probing, load <= 1/2, sized by the host before
// the launch for everything the batch can bring (no kernel can run out of slots or arena mid-flight).  Every claim and
// the pair table's lookups go through tab_probe (dev_table.h), bounded by POS_PROBES; the export's compaction is
// block256_compact (dev_table.h):
//  string dictionaries  one for provider, one for vehicleId.  A slot (PosStr, 24 B, cleared to all-ones bytes) holds the
//                    string's 63-bit hash, its span in an append-only byte arena and its persistent code (dense, in
//                    order of insertion; never reused).  code_off / code_len list the spans by code (the export).
//                    A batch maps each of its dictionary ENTRIES (not its rows) to a persistent code:
//                      k_pos_str_find    read only: hash, then bytes against the arena; equal hash and unequal bytes
//                                        probe on (never merged, never an error).  Entries not found are counted (with
//                                        their bytes): the host grows table and arena for exactly those.
//                      k_pos_str_insert  the entries not found claim the first free slot of their probe chain by a
//                                        64-bit CAS and append their bytes (one arena and one code reservation per
//                                        wave).  INVARIANT: a batch dictionary holds distinct strings, and none of the
//                                        inserted ones is in the table (k_pos_str_find ran on the same table contents),
//                                        so no two threads ever insert the same string and a slot taken during this
//                                        launch is by construction another string: the insert compares nothing and
//                                        never reads bytes that may still be in flight.
//  pair table        key = provider code << 32 | vehicle code (exact: no strings needed), PosSlot 32 B + one candidate
//                    word per slot.  Codes stay below 2^31 - 1, so bit 63 of a key word is free: it marks a slot
//                    claimed by the running fold (POS_FRESH), whose ts is not yet meaningful.
//                      k_pos_pair_pass1  every latest row finds or claims its slot; if the slot is fresh or the row's
//                                        ts is greater than the stored one (strictly), atomicMin of the row index into
//                                        the slot's candidate word.
//                      k_pos_pair_pass2  the row that equals its slot's candidate writes ts, lat, lon, clears
//                                        POS_FRESH and resets the candidate: one writer per slot.
//                    Two passes resolve a batch's tied maxima to the lowest row without packing (ts, row) into one
//                    word; the result does not depend on scheduling, and folding a batch twice changes nothing.
// Growth: k_pos_str_rehash / k_pos_pair_put move the old table's slots into a larger one (ahead of the update).
// =====================================================================================================
struct PosStr {
    unsigned long long key;   // string hash < 2^63; ~0 = free
    unsigned long long off;   // the string's bytes in the arena
    unsigned len;
    unsigned code;            // persistent code
};
static_assert(sizeof(PosStr) == 24, "PosStr is 24 B");
struct PosSlot {
    unsigned long long key;   // provider code << 32 | vehicle code (| POS_FRESH during a fold); ~0 = free
    long long ts;
    double lat, lon;
};
static_assert(sizeof(PosSlot) == 32, "PosSlot is 32 B");
constexpr unsigned long long POS_EMPTY = ~0ull;
constexpr unsigned long long POS_FRESH = 1ull << 63;
constexpr unsigned POS_NONE = ~0u;          // no candidate / entry not in the dictionary
constexpr unsigned POS_MAX_CODES = 0x7ffffffeu;   // (code 0x7fffffff with vehicle code ~0 | POS_FRESH would read as POS_EMPTY)
constexpr unsigned long long POS_PROBES = 4096;   // probe bound (a chain this long at load <= 1/2: the hashes collide)
constexpr uint64_t POS_SEED = UINT64_C(0x5bd1e9955bd1e995);

// str_hash (k_json.h) cut to its low `bits` bits (hm_positions_debug_hash_bits; 64 = all of them)
__device__ __forceinline__ unsigned long long pos_hash(const uint8_t *s, int n, int bits) {
    const unsigned long long h = str_hash(s, n, POS_SEED);
    return bits >= 64 ? h : bits <= 0 ? 0ull : h & ((1ull << bits) - 1);
}
__device__ __forceinline__ bool pos_bytes_equal(const uint8_t *a, const uint8_t *b, int n) {
    for (int k = 0; k < n; k++)
        if (a[k] != b[k]) return false;
    return true;
}
// the key words of a positions table (PosStr or PosSlot), as tab_probe (dev_table.h) reaches them
template <class Slot>
__device__ __forceinline__ auto pos_keys(Slot *tab) {
    return [tab](unsigned long long i) { return &tab[i].key; };
}
// claims the first free slot of `key`'s probe chain and compares nothing: the caller guarantees distinct keys, none of
// them in the table.  TAB_NONE: no free slot within the probe bound (the caller counts it in words[PW_OVERFLOW]).
template <class Slot>
__device__ __forceinline__ unsigned long long pos_claim(Slot *tab, unsigned long long mask, unsigned long long key) {
    unsigned long long seen;
    return tab_probe<true>(pos_keys(tab), mask, mix64(key) & mask, POS_PROBES, POS_EMPTY, key, TabNoMatch{}, seen);
}

// words of the control block (device; zeroed before every call that counts into them)
enum { PW_BAD = 0, PW_OVERFLOW, PW_NEW_P, PW_BYTES_P, PW_NEW_V, PW_BYTES_V, PW_NEW_PAIRS, PW_OUT, PW_WORDS };

// the latest rows' codes (vkey / n_vehicles < n_providers): what the passes index the batch's code lists with
__global__ __launch_bounds__(256) void k_pos_check(int64_t np_, int64_t nv, const int64_t *__restrict__ rows, int64_t n,
                                                   const uint64_t *__restrict__ vk, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride)
        bad += nv <= 0 || vk[rows[q]] / (uint64_t)nv >= (uint64_t)np_;
    bad = wave_sum(bad);
    if (bad && lane_id() == 0) atomicAdd(&words[PW_BAD], bad);
}

// entry k of a batch dictionary -> its persistent code, or POS_NONE (counted in words[w_new], its bytes in
// words[w_new + 1]).  Read only; the table holds what earlier launches wrote.  An entry whose offsets are not ascending
// from >= 0 inside `total` bytes, or longer than 2^20 bytes, is counted in words[PW_BAD] and its bytes are not read.
__global__ __launch_bounds__(256) void k_pos_str_find(const int64_t *__restrict__ off, const uint8_t *__restrict__ bytes,
                                                      int64_t n, int64_t total, const PosStr *__restrict__ tab, unsigned long long mask,
                                                      const uint8_t *__restrict__ arena, int bits,
                                                      unsigned *__restrict__ code_of, unsigned long long *words, int w_new) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long fresh = 0, fresh_bytes = 0, bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const int64_t a = off[k], b = off[k + 1];
        if (a < 0 || a > b || b > total || b - a > (1 << 20)) {
            bad++;
            code_of[k] = POS_NONE;
            continue;
        }
        const uint8_t *s = bytes + a;
        const int len = (int)(b - a);
        unsigned code = POS_NONE;
        if (tab) {
            const unsigned long long h = pos_hash(s, len, bits);
            unsigned long long at = mix64(h) & mask;
            for (unsigned long long q = 0; q <= mask; q++) {   // (load <= 1/2: a free slot ends the chain)
                const PosStr e = tab[at];
                if (e.key == POS_EMPTY) break;
                if (e.key == h && e.len == (unsigned)len && pos_bytes_equal(arena + e.off, s, len)) {
                    code = e.code;
                    break;
                }
                at = (at + 1) & mask;
            }
        }
        code_of[k] = code;
        if (code == POS_NONE) { fresh++; fresh_bytes += (unsigned long long)len; }
    }
    fresh = wave_sum(fresh);
    fresh_bytes = wave_sum(fresh_bytes);
    bad = wave_sum(bad);
    if (lane_id() == 0) {
        if (fresh) atomicAdd(&words[w_new], fresh);
        if (fresh_bytes) atomicAdd(&words[w_new + 1], fresh_bytes);
        if (bad) atomicAdd(&words[PW_BAD], bad);
    }
}

// the entries k_pos_str_find did not find (code_of[k] == POS_NONE) enter the dictionary: see the invariant above.
// used[0] = arena bytes in use, used[1] = codes in use (both advanced by one atomic per wave).
__global__ __launch_bounds__(256) void k_pos_str_insert(const int64_t *__restrict__ off, const uint8_t *__restrict__ bytes,
                                                        int64_t n, PosStr *tab, unsigned long long mask, uint8_t *arena,
                                                        int bits, unsigned *code_of, unsigned long long *used,
                                                        unsigned long long *__restrict__ code_off,
                                                        unsigned *__restrict__ code_len, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int ln = lane_id();
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {   // (uniform trip count: shuffles)
        const int64_t k = base + threadIdx.x;
        const bool mine = k < n && code_of[k] == POS_NONE;
        const uint8_t *s = mine ? bytes + off[k] : nullptr;
        const unsigned len = mine ? (unsigned)(off[k + 1] - off[k]) : 0u;
        // (claim only: a slot's owner of this launch is another string by the invariant, an older one was compared by
        // k_pos_str_find: probe on)
        const unsigned long long slot = mine ? pos_claim(tab, mask, pos_hash(s, (int)len, bits)) : TAB_NONE;
        const bool won = slot != TAB_NONE;
        // this wave's reservation: bytes and codes, one atomic each
        const unsigned long long m = __ballot(won);
        const unsigned long long pre = wave_inclusive_scan<unsigned long long>(won ? len : 0u);
        const unsigned long long tot = __shfl(pre, 63, 64);
        unsigned long long b0 = 0, c0 = 0;
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            if (ln == leader) {
                b0 = atomicAdd(&used[0], tot);
                c0 = atomicAdd(&used[1], (unsigned long long)__popcll(m));
            }
            b0 = __shfl(b0, leader, 64);
            c0 = __shfl(c0, leader, 64);
        }
        if (won) {
            const unsigned long long at = b0 + pre - len;
            const unsigned code = (unsigned)(c0 + __popcll(m & ((1ull << ln) - 1)));
            for (unsigned q = 0; q < len; q++) arena[at + q] = s[q];
            tab[slot].off = at;
            tab[slot].len = len;
            tab[slot].code = code;
            code_off[code] = at;
            code_len[code] = len;
            code_of[k] = code;
        }
        if (mine && !won) atomicAdd(&words[PW_OVERFLOW], 1ull);
    }
}

// import: string k of the imported dictionary keeps code k; its bytes are already in the arena at off[k]
__global__ __launch_bounds__(256) void k_pos_str_import(const int64_t *__restrict__ off, int64_t n, PosStr *tab,
                                                        unsigned long long mask, const uint8_t *__restrict__ arena, int bits,
                                                        unsigned long long *__restrict__ code_off,
                                                        unsigned *__restrict__ code_len, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const unsigned len = (unsigned)(off[k + 1] - off[k]);
        const unsigned long long slot = pos_claim(tab, mask, pos_hash(arena + off[k], (int)len, bits));
        if (slot == TAB_NONE) { atomicAdd(&words[PW_OVERFLOW], 1ull); continue; }
        tab[slot].off = (unsigned long long)off[k];
        tab[slot].len = len;
        tab[slot].code = (unsigned)k;
        code_off[k] = (unsigned long long)off[k];
        code_len[k] = len;
    }
}

// growth: the old table's strings into the new one (their hashes are in the slots; the arena is copied separately)
__global__ __launch_bounds__(256) void k_pos_str_rehash(const PosStr *__restrict__ old, int64_t old_cap, PosStr *tab,
                                                        unsigned long long mask, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < old_cap; i += stride) {
        const PosStr e = old[i];
        if (e.key == POS_EMPTY) continue;
        const unsigned long long slot = pos_claim(tab, mask, e.key);
        if (slot == TAB_NONE) { atomicAdd(&words[PW_OVERFLOW], 1ull); continue; }
        tab[slot].off = e.off;
        tab[slot].len = e.len;
        tab[slot].code = e.code;
    }
}

// the slot of pair key `key` (< 2^63), claimed with POS_FRESH if absent; TAB_NONE: the probe bound ran out.
// claimed: by this thread; fresh: the slot was claimed during this launch (by this thread or another).
__device__ __forceinline__ unsigned long long pos_pair_slot(PosSlot *tab, unsigned long long mask, unsigned long long key,
                                                            bool &fresh, bool &claimed) {
    // (an occupied slot's word is never POS_EMPTY with POS_FRESH ignored: a key's codes stay below POS_MAX_CODES)
    unsigned long long seen = 0;
    const unsigned long long at = tab_probe<true>(pos_keys(tab), mask, mix64(key) & mask, POS_PROBES, POS_EMPTY, key | POS_FRESH,
                                                  TabKeyIs{key, POS_FRESH}, seen);
    claimed = seen == POS_EMPTY;
    fresh = (seen & POS_FRESH) != 0;   // (POS_EMPTY has the bit too)
    return at;
}

// read only, ahead of a fold whose worst case (every row a new pair) would not fit the table: the latest rows whose pair
// is not in it (a row of a string without a code yet, or of a key the probe chain does not hold; tied rows of one new
// key count once each: an upper bound of the pairs the fold creates, exact but for those ties)
__global__ __launch_bounds__(256) void k_pos_pair_count(const int64_t *__restrict__ rows, int64_t n,
                                                        const uint64_t *__restrict__ vk, uint64_t n_vehicles,
                                                        const unsigned *__restrict__ p_code,
                                                        const unsigned *__restrict__ v_code, const PosSlot *__restrict__ tab,
                                                        unsigned long long mask, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long absent = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const uint64_t v = vk[rows[q]];
        const unsigned pc = p_code[v / n_vehicles], vc = v_code[v % n_vehicles];
        bool found = false;
        if (tab && pc != POS_NONE && vc != POS_NONE) {
            const unsigned long long key = ((unsigned long long)pc << 32) | vc;
            unsigned long long seen;   // (the table was written by earlier launches: no POS_FRESH, no race)
            found = tab_probe<false>(pos_keys(tab), mask, mix64(key) & mask, POS_PROBES, POS_EMPTY, 0ull, TabKeyIs{key, 0ull},
                                     seen) != TAB_NONE;
        }
        absent += !found;
    }
    absent = wave_sum(absent);
    if (absent && lane_id() == 0) atomicAdd(&words[PW_NEW_PAIRS], absent);
}

// pass 1 over the latest rows (rows[q] ascending): slot_of[q] = the row's slot; candidates by atomicMin of the row index
__global__ __launch_bounds__(256) void k_pos_pair_pass1(const int64_t *__restrict__ rows, int64_t n,
                                                        const uint64_t *__restrict__ vk, const int64_t *__restrict__ ts,
                                                        uint64_t n_vehicles, const unsigned *__restrict__ p_code,
                                                        const unsigned *__restrict__ v_code, PosSlot *tab,
                                                        unsigned long long mask, unsigned *cand,
                                                        unsigned *__restrict__ slot_of, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long created = 0, lost = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const int64_t r = rows[q];
        const uint64_t v = vk[r];
        const unsigned pc = p_code[v / n_vehicles], vc = v_code[v % n_vehicles];
        const unsigned long long key = ((unsigned long long)pc << 32) | vc;
        bool fresh = false, claimed = false;
        // (a string k_pos_str_insert found no slot for has no code: its rows are lost, and counted)
        const unsigned long long s = pc == POS_NONE || vc == POS_NONE ? TAB_NONE : pos_pair_slot(tab, mask, key, fresh, claimed);
        slot_of[q] = s == TAB_NONE ? POS_NONE : (unsigned)s;
        if (s == TAB_NONE) { lost++; continue; }
        created += claimed;
        // (a slot that is not fresh holds the ts an earlier fold wrote: nothing writes ts during this launch)
        if (fresh || ts[r] > tab[s].ts) atomicMin(&cand[s], (unsigned)r);
    }
    created = wave_sum(created);
    lost = wave_sum(lost);
    if (lane_id() == 0) {
        if (created) atomicAdd(&words[PW_NEW_PAIRS], created);
        if (lost) atomicAdd(&words[PW_OVERFLOW], lost);
    }
}
// pass 2: the candidate row of each slot writes it
__global__ __launch_bounds__(256) void k_pos_pair_pass2(const int64_t *__restrict__ rows, int64_t n,
                                                        const int64_t *__restrict__ ts, const double *__restrict__ lat,
                                                        const double *__restrict__ lon, PosSlot *__restrict__ tab,
                                                        unsigned *__restrict__ cand, const unsigned *__restrict__ slot_of) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const unsigned s = slot_of[q];
        if (s == POS_NONE) continue;
        const int64_t r = rows[q];
        if (cand[s] != (unsigned)r) continue;
        PosSlot e;
        e.key = tab[s].key & ~POS_FRESH;
        e.ts = ts[r];
        e.lat = lat[r];
        e.lon = lon[r];
        tab[s] = e;
        cand[s] = POS_NONE;
    }
}

// growth / import: records (key, ts, lat, lon) into the table (distinct keys: the caller's guarantee)
__global__ __launch_bounds__(256) void k_pos_pair_put(const PosSlot *__restrict__ src, int64_t n, PosSlot *tab,
                                                      unsigned long long mask, unsigned long long *words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const PosSlot e = src[i];
        if (e.key == POS_EMPTY) continue;
        const unsigned long long slot = pos_claim(tab, mask, e.key);
        if (slot == TAB_NONE) { atomicAdd(&words[PW_OVERFLOW], 1ull); continue; }
        tab[slot].ts = e.ts;
        tab[slot].lat = e.lat;
        tab[slot].lon = e.lon;
    }
}

// export: the occupied slots as hm_position_rec, compacted by block256_compact (dev_table.h); records past out_cap are
// counted, not written
__global__ __launch_bounds__(256) void k_pos_emit(const PosSlot *__restrict__ tab, int64_t nslots,
                                                  hm_position_rec *__restrict__ out, int64_t out_cap,
                                                  unsigned long long *n_out) {
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nslots; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < nslots && tab[i].key != POS_EMPTY; };
        block256_compact<true>(base, is_live, n_out, (unsigned long long)out_cap, [=](int64_t i, unsigned long long at) {
            const PosSlot e = tab[i];
            hm_position_rec r;
            r.provider = (uint32_t)(e.key >> 32);
            r.vehicle = (uint32_t)e.key;
            r.ts_us = e.ts;
            r.lat = e.lat;
            r.lon = e.lon;
            out[at] = r;
        });
    }
}
// export: a persistent dictionary's bytes in code order (offs: the exclusive scan of code_len)
__global__ __launch_bounds__(256) void k_pos_str_gather(const unsigned long long *__restrict__ code_off,
                                                        const unsigned *__restrict__ code_len, int64_t n,
                                                        const uint8_t *__restrict__ arena,
                                                        const unsigned long long *__restrict__ offs, uint8_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += stride) {
        const uint8_t *s = arena + code_off[c];
        uint8_t *d = out + offs[c];
        for (unsigned q = 0; q < code_len[c]; q++) d[q] = s[q];
    }
}
