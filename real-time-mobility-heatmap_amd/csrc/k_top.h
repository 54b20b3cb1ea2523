// Read side: the k records with the largest count, in rank order -- key extraction, an MSD radix select over the key
// bytes that vary, the compaction of the selected and their ordering by counting (k_top_keys, k_top_hist, k_top_pick,
// k_top_compact, k_top_rank, k_top_scatter).
// Part of the single translation unit mobheat.hip (included there in dependency order; not compiled alone).
#pragma once

// =====================================================================================================
// The order: a ranks before b iff a.count > b.count (int64), then a.cell < b.cell (uint64), then a's input index is the
// lower.  As one key of three words compared as unsigned numbers, "ranks first" = "smaller key":
//   word 0  kc    ~(count ^ 2^63): the sign flip makes int64 order unsigned order, the complement reverses it
//   word 1  cell
//   word 2  idx   the input index (u32: at most 2^31 candidates), never stored for the candidates
// The select never sorts the candidates.  k_top_keys writes kc[] and cell[] (16 of a record's 64 bytes) and reduces the
// OR and the AND of both words; a byte whose OR equals its AND is the same in every key and needs no pass.  The host
// then walks the varying bytes from the most significant (api_top.h): k_top_hist counts the digits of the candidates
// still tied with the prefix chosen so far (the examined bytes, `TopMasks`), k_top_pick -- one wave -- finds the digit
// where the running total crosses what is still needed, extends the prefix by it and lowers the need by the candidates
// of smaller digits, which are selected for good.  The walk ends when the tied group is exactly as large as the need
// (all of it is taken) -- with the index bytes at the end of the walk that always happens.  Selected is then: the key
// restricted to the examined bytes <= the prefix (top_selected); bytes that were skipped are constant, bytes never
// reached belong to a tied group taken whole.
// k_top_compact gathers the min(k, n) selected keys with their indices, k_top_rank gives each the number of selected
// keys that rank before it (all distinct: a permutation), k_top_scatter copies the records whole into rank order.
// =====================================================================================================
constexpr int64_t TOP_MAX = HM_TOP_MAX;
// words of the top's control block (device)
enum {
    TW_OR_C = 0, TW_NAND_C, TW_OR_CELL, TW_NAND_CELL,   // OR of the keys' words, OR of their complements (AND = ~that)
    TW_PC, TW_PCELL, TW_PIDX,                           // the prefix: the digits chosen so far, in place, 0 elsewhere
    TW_NEED, TW_TIED,                                   // still to select among the tied; the tied group's size
    TW_OUT,                                             // k_top_compact's counter
    TW_VIEW,                                            // hm_window_top's view filter: records kept
    TW_HIST = 16,                                       // 256 digit counts (k_top_pick clears them)
    TW_WORDS = TW_HIST + 256
};
struct TopMasks { unsigned long long c, cell; unsigned idx; };   // the examined bytes of the three words

HM_HD unsigned long long top_key_count(long long count) { return ~((unsigned long long)count ^ (1ull << 63)); }
HM_HD unsigned top_digit(unsigned long long word, int shift) { return (unsigned)(word >> shift) & 0xffu; }
// key a < key b (a ranks before b)
HM_HD bool top_before(unsigned long long ac, unsigned long long acell, unsigned ai, unsigned long long bc,
                      unsigned long long bcell, unsigned bi) {
    return (ac < bc) | ((ac == bc) & ((acell < bcell) | ((acell == bcell) & (ai < bi))));
}
HM_HD bool top_tied(unsigned long long c, unsigned long long cell, unsigned i, const TopMasks &M, unsigned long long pc,
                    unsigned long long pcell, unsigned pidx) {
    return ((c & M.c) == pc) & ((cell & M.cell) == pcell) & ((i & M.idx) == pidx);
}
HM_HD bool top_selected(unsigned long long c, unsigned long long cell, unsigned i, const TopMasks &M, unsigned long long pc,
                        unsigned long long pcell, unsigned pidx) {
    return top_tied(c, cell, i, M, pc, pcell, pidx) || top_before(c & M.c, cell & M.cell, i & M.idx, pc, pcell, pidx);
}

// kc[i], cell[i] of every record; words[TW_OR_C .. TW_NAND_CELL] gain one atomic each per workgroup
__global__ __launch_bounds__(256) void k_top_keys(const GrowRec *__restrict__ recs, int64_t n, unsigned long long *__restrict__ kc,
                                                  unsigned long long *__restrict__ cell, unsigned long long *words) {
    __shared__ unsigned long long part[4][4];
    unsigned long long r[4] = {0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned long long c = top_key_count((long long)recs[i].count), l = recs[i].cell;
        kc[i] = c;
        cell[i] = l;
        r[0] |= c;
        r[1] |= ~c;
        r[2] |= l;
        r[3] |= ~l;
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
        for (int o = 32; o > 0; o >>= 1) r[q] |= __shfl_xor(r[q], o, 64);
    if (lane_id() == 0)
        for (int q = 0; q < 4; q++) part[threadIdx.x >> 6][q] = r[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][threadIdx.x] | part[1][threadIdx.x] | part[2][threadIdx.x] | part[3][threadIdx.x];
        if (v) atomicOr(&words[TW_OR_C + threadIdx.x], v);
    }
}

// one pass: the digit (byte `shift` / 8 of word `word`: 0 kc, 1 cell, 2 idx) of every candidate tied with the prefix
// under the examined bytes M, counted in LDS, flushed with one atomic per non-empty bin and workgroup.  A count pass
// (no cell byte examined yet) does not read cell[].
__global__ __launch_bounds__(256) void k_top_hist(const unsigned long long *__restrict__ kc, const unsigned long long *__restrict__ cell,
                                                  int64_t n, TopMasks M, int word, int shift, unsigned long long *words) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    const unsigned long long pc = words[TW_PC], pcell = words[TW_PCELL];
    const unsigned pidx = (unsigned)words[TW_PIDX];
    const bool with_cell = M.cell != 0 || word != 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned long long c = kc[i], l = with_cell ? cell[i] : 0ull;
        if (top_tied(c, l, (unsigned)i, M, pc, pcell, pidx))
            atomicAdd(&h[top_digit(word == 0 ? c : word == 1 ? l : (unsigned long long)(unsigned)i, shift)], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&words[TW_HIST + threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// one wave: the digit d whose bin holds the need-th tied candidate (bins in ascending digit order) joins the prefix;
// need -= the candidates of smaller digits, tied = bin d.  Clears the bins for the next pass.  (The bins sum to the tied
// group's size >= need >= 1, so exactly one lane finds its range crossed.)
__global__ __launch_bounds__(64) void k_top_pick(unsigned long long *words, int word, int shift) {
    const int ln = threadIdx.x;
    unsigned long long b[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        b[q] = words[TW_HIST + 4 * ln + q];
        words[TW_HIST + 4 * ln + q] = 0;
        s += b[q];
    }
    const unsigned long long need = words[TW_NEED];
    unsigned long long below = wave_inclusive_scan(s) - s;
    if (below < need && need <= below + s) {
        int q = 0;   // the first of the lane's four bins that reaches the need
#pragma unroll
        for (int t = 0; t < 3; t++)
            if (q == t && below + b[t] < need) { below += b[t]; q = t + 1; }
        words[TW_PC + word] |= (unsigned long long)(4 * ln + q) << shift;
        words[TW_NEED] = need - below;
        words[TW_TIED] = q == 0 ? b[0] : q == 1 ? b[1] : q == 2 ? b[2] : b[3];
    }
}

// the selected candidates' keys and indices, compacted (at most cap written)
__global__ __launch_bounds__(256) void k_top_compact(const unsigned long long *__restrict__ kc, const unsigned long long *__restrict__ cell,
                                                     int64_t n, TopMasks M, unsigned long long *words,
                                                     unsigned long long *__restrict__ skc, unsigned long long *__restrict__ scell,
                                                     unsigned *__restrict__ sidx, unsigned long long cap) {
    const unsigned long long pc = words[TW_PC], pcell = words[TW_PCELL];
    const unsigned pidx = (unsigned)words[TW_PIDX];
    const int64_t tile = 256 * DUMP_PER;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n; base += (int64_t)gridDim.x * tile) {
        const auto is_live = [=](int64_t i) { return i < n && top_selected(kc[i], cell[i], (unsigned)i, M, pc, pcell, pidx); };
        block256_compact<true>(base, is_live, words + TW_OUT, cap, [=](int64_t i, unsigned long long at) {
            skc[at] = kc[i];
            scell[at] = cell[i];
            sidx[at] = (unsigned)i;
        });
    }
}

// rank[j] += the selected keys of this workgroup's tiles that rank before selected key j.  blockIdx.x: the 256 keys j,
// blockIdx.y: the tiles t = y, y + gridDim.y, ... of 256 keys, streamed through LDS (every lane reads the same key: a
// broadcast).  rank[] is zeroed before the launch; the sums are integers, so their order does not matter.  A tile's
// tail is padded with the largest key, which ranks before nothing.
__global__ __launch_bounds__(256) void k_top_rank(const unsigned long long *__restrict__ skc, const unsigned long long *__restrict__ scell,
                                                  const unsigned *__restrict__ sidx, int m, unsigned *rank) {
    __shared__ unsigned long long tc[256], tl[256];
    __shared__ unsigned ti[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    const bool has = j < m;
    const unsigned long long jc = has ? skc[j] : 0ull, jl = has ? scell[j] : 0ull;
    const unsigned ji = has ? sidx[j] : 0u;
    unsigned before = 0;
    const int tiles = (m + 255) / 256;
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int i = t * 256 + threadIdx.x;
        __syncthreads();   // (the previous tile has been read)
        tc[threadIdx.x] = i < m ? skc[i] : ~0ull;
        tl[threadIdx.x] = i < m ? scell[i] : ~0ull;
        ti[threadIdx.x] = i < m ? sidx[i] : ~0u;
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 256; q++) before += top_before(tc[q], tl[q], ti[q], jc, jl, ji) ? 1u : 0u;
    }
    if (has && before) atomicAdd(&rank[j], before);
}

// out[rank[j]] = recs[sidx[j]], whole: four lanes per record, 16 bytes each (a stale index or rank writes nothing)
__global__ __launch_bounds__(256) void k_top_scatter(const uint4 *__restrict__ recs, int64_t n, const unsigned *__restrict__ sidx,
                                                     const unsigned *__restrict__ rank, int m, uint4 *__restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)m * 4; t += (int64_t)gridDim.x * 256) {
        const unsigned src = sidx[t >> 2], r = rank[t >> 2];
        if ((int64_t)src < n && r < (unsigned)m) out[(int64_t)r * 4 + (t & 3)] = recs[(int64_t)src * 4 + (t & 3)];
    }
}
