// The embedding stage of a full fine-tune on gfx950: the fp32 forward (a sum of table rows per token) and its backward, a
// deterministic index-add of gradient rows into table rows.  No atomics on floating-point data anywhere: every output element
// has one writer and a summation order that depends only on (idx, src_row, n, R, C), so the same input gives the same bits on
// every run.  Everything runs on the caller's stream; nothing comes back to the host between the launches.
//
// vk_index_add_rows    dst[r, :C] = sum over the entries i (ascending) with idx[i] == r of src[src_row ? src_row[i] : i, :C]
//
//   keys       entry i sorts under key idx[i]; an entry that is skipped (idx outside [0, R), idx == padding_idx, a source row
//              outside [0, M)) sorts under the sentinel key R, behind every row, and is never read through.
//   sort       a stable LSD radix sort of (key, i), 8 bits per pass, ceil(bits(R) / 8) passes (bits(R): the bits of the value R,
//              which the sentinel needs: 1 pass up to R = 255, 2 up to 65 535, 3 up to 2^24 - 1, else 4).  A pass is three launches:
//                sort_count_kernel   a workgroup owns SORT_TILE = 1024 consecutive entries, each of its 4 waves 256 of them, walked
//                                    in 4 rounds of 64.  Per round a lane finds the lanes of its wave with the same digit (8
//                                    ballots); the lowest of them adds their number to the wave's own LDS counter row.  Integer
//                                    counters with one writer each; the workgroup's totals go to count[digit][workgroup].
//                sort_scan_kernel    one workgroup, an exclusive scan over count[digit][workgroup] in that order: 2048 values a
//                                    step (8 per thread, wave shuffles, 4 wave totals through LDS).
//                sort_place_kernel   the count again, then base[wave][digit] = the scanned offset + the counters of the waves
//                                    before it; an entry lands at base + its rank among the equal digits of its round (the
//                                    lanes below it), and the round's number is added to base.  Lanes in order, rounds in order,
//                                    waves in order, workgroups in order: the placement is stable.
//              The first pass reads idx / src_row and makes the keys; the sorted keys and the permutation ping-pong between two
//              buffers of the workspace.  A run is a maximal stretch of equal sorted keys; its head is where the key changes.
//   sum        the sorted entries are cut into chunks of IA_CHUNK = 32 entries (S; tests/test_gpu_index_add.py aims at S - 1, S,
//              S + 1).  segsum_kernel: a wave owns a chunk and a slab of 64 * VW columns, VW = 4 (one 16-byte load per lane and
//              entry) where row_norm.h's launch rule allows, else 1.  Lane j holds key and source row of entry j; the wave walks
//              them by readlane, four row loads in flight, with VW fp64 accumulators per lane, and flushes at a change of key: a run
//              that lies inside the chunk is rounded once and stored to dst; the part of a run that began in an earlier chunk
//              goes to part[chunk][0][C] (fp64), the part of a run that begins here and goes on in the next chunk to
//              part[chunk][1][C].
//   stitch     stitch_kernel: the wave of the chunk where a crossing run begins adds part[chunk][1], then part[c][0] of the
//              chunks c after it while the run goes on, in chunk order, and stores the row, rounded once.
//   fill       fill_kernel: a wave per row of dst looks its row up in the sorted keys (binary search) and writes zeros where it is
//              absent: the rows no entry names, padding_idx among them.  Rows with entries are written by sum or stitch, all
//              others here: one writer per element, no clear of dst that a later store would race with.
//
// Rounding: fp64 adds of the fp32 terms, in entry order within a chunk's part of a run, the parts in chunk order; ONE rounding to
// fp32 at the store.  Integer data whose sums stay below 2^24 is exact.
//
// vk_embed_sum_f32     out[out_row ? out_row[m] : m, :C] = (base ? base[m] : 0) + table_0[idx[0, m]] + .. in fp32, left to right
//                      (without base the first table's row starts the sum); an out_row outside out's rows is skipped.
//                      embed_sum_kernel: one wave per row, four rows per workgroup, row_norm.h's chunk loader; the tables ride
//                      in the kernel's argument struct.
#include "row_norm.h"

namespace vk {

constexpr int IA_CHUNK = 32;                 // S: sorted entries per chunk of the segmented sum
constexpr int SORT_ROUNDS = 4;               // rounds of 64 entries per wave
constexpr int SORT_WAVE = 64 * SORT_ROUNDS;  // entries a wave owns
constexpr int SORT_TILE = 4 * SORT_WAVE;     // entries a workgroup owns
constexpr int SCAN_PER = 8;                  // values per thread and step of the scan
constexpr unsigned NO_KEY = 0xffffffffu;     // "no neighbour" beside the first / last sorted entry (every key is <= R < 2^31)

struct IaArgs {
    const float *src;
    const int32_t *idx, *src_row;
    float *dst;
    double *part;
    long ld_src, ld_dst, M;
    int n, R, C, padding_idx;
};

// ---- the ordering pass ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned entry_key(const IaArgs &a, int i) {
    const int r = a.idx[i];
    if (r < 0 || r >= a.R || r == a.padding_idx) return (unsigned)a.R;
    if (a.src_row) {
        const long s = a.src_row[i];
        if (s < 0 || s >= a.M) return (unsigned)a.R;
    } else if (i >= a.M) {
        return (unsigned)a.R;
    }
    return (unsigned)r;
}

// the lanes of the wave that are `valid` and hold the same 8-bit digit as this one
__device__ __forceinline__ unsigned long long digit_peers(unsigned digit, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((digit >> b) & 1u);
        peers &= ((digit >> b) & 1u) ? m : ~m;
    }
    return peers;
}

struct SortArgs {
    IaArgs a;
    const unsigned *kin;        // null: the first pass, keys from idx / src_row and the identity permutation
    const int32_t *pin;
    unsigned *kout;
    int32_t *pout;
    unsigned *count;            // [256][nwg]
    int shift, nwg;
};

// wcnt[wave][digit] = the wave's entries per digit; -> this thread's 4 (key, entry) pairs are left in k[], p[] for the placement
__device__ __forceinline__ void sort_count(const SortArgs &s, unsigned (*wcnt)[256], unsigned (&k)[SORT_ROUNDS], int32_t (&p)[SORT_ROUNDS]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    const long e0 = (long)blockIdx.x * SORT_TILE + wave * SORT_WAVE + lane;
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const long e = e0 + 64 * r;
        const bool valid = e < s.a.n;
        k[r] = 0;
        p[r] = 0;
        if (valid) {
            k[r] = s.kin ? s.kin[e] : entry_key(s.a, (int)e);
            p[r] = s.kin ? s.pin[e] : (int32_t)e;
        }
        const unsigned d = (k[r] >> s.shift) & 255u;
        const unsigned long long peers = digit_peers(d, valid);
        if (valid && (peers & ((1ull << lane) - 1)) == 0) wcnt[wave][d] += (unsigned)__popcll(peers);      // the lowest peer: one writer
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void sort_count_kernel(SortArgs s) {
    __shared__ unsigned wcnt[4][256];
    unsigned k[SORT_ROUNDS];
    int32_t p[SORT_ROUNDS];
    sort_count(s, wcnt, k, p);
    const int d = threadIdx.x;
    s.count[(size_t)d * s.nwg + blockIdx.x] = wcnt[0][d] + wcnt[1][d] + wcnt[2][d] + wcnt[3][d];
}

// count[0 .. total) -> its exclusive prefix sums, in place; one workgroup
__global__ __launch_bounds__(256) void sort_scan_kernel(unsigned *count, size_t total) {
    __shared__ unsigned wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned carry = 0;
    for (size_t base = 0; base < total; base += 256 * SCAN_PER) {
        unsigned v[SCAN_PER], t = 0;
#pragma unroll
        for (int i = 0; i < SCAN_PER; ++i) {
            const size_t e = base + (size_t)tid * SCAN_PER + i;
            v[i] = e < total ? count[e] : 0u;
            t += v[i];
        }
        unsigned inc = t;                                 // the inclusive scan of the threads' totals within the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = carry + inc - t;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        const unsigned step_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
#pragma unroll
        for (int i = 0; i < SCAN_PER; ++i) {
            const size_t e = base + (size_t)tid * SCAN_PER + i;
            if (e < total) count[e] = before;
            before += v[i];
        }
        carry += step_total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void sort_place_kernel(SortArgs s) {
    __shared__ unsigned wcnt[4][256];
    unsigned k[SORT_ROUNDS];
    int32_t p[SORT_ROUNDS];
    sort_count(s, wcnt, k, p);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {   // thread d turns the counters of digit d into the waves' bases
        unsigned at = s.count[(size_t)tid * s.nwg + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned c = wcnt[w][tid];
            wcnt[w][tid] = at;
            at += c;
        }
    }
    __syncthreads();
    const long e0 = (long)blockIdx.x * SORT_TILE + wave * SORT_WAVE + lane;
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const bool valid = e0 + 64 * r < s.a.n;
        const unsigned d = (k[r] >> s.shift) & 255u;
        const unsigned long long peers = digit_peers(d, valid);
        const unsigned long long below = peers & ((1ull << lane) - 1);
        unsigned at = 0;
        if (valid) at = wcnt[wave][d] + (unsigned)__popcll(below);
        __syncthreads();
        if (valid && at < (unsigned)s.a.n) {
            s.kout[at] = k[r];
            s.pout[at] = p[r];
            if (below == 0) wcnt[wave][d] += (unsigned)__popcll(peers);
        }
        __syncthreads();
    }
}

// ---- the segmented sum ---------------------------------------------------------------------------------------------------------------
template <int VW>
__device__ __forceinline__ void ia_store_row(float *p, const double (&acc)[VW]) {
    float o[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) o[e] = (float)acc[e];
    st_chunk<float, VW>(p, o);
}

template <int VW>
__global__ __launch_bounds__(64) void segsum_kernel(IaArgs a, const unsigned *__restrict__ keys, const int32_t *__restrict__ perm) {
    const int lane = threadIdx.x;
    const long e0 = (long)blockIdx.x * IA_CHUNK;
    const int cnt = (int)min((long)IA_CHUNK, a.n - e0);
    const int col = ((int)blockIdx.y * 64 + lane) * VW;
    const bool active = col < a.C;
    unsigned my_key = (unsigned)a.R;                      // lanes past the chunk hold the sentinel: the walk ends there
    int my_row = 0;
    if (lane < cnt) {
        my_key = keys[e0 + lane];
        if (my_key < (unsigned)a.R) {
            const int p = perm[e0 + lane];
            if ((unsigned)p < (unsigned)a.n) my_row = a.src_row ? a.src_row[p] : p;
            if (my_row < 0 || my_row >= a.M) my_row = -1;     // cannot be: the key says the row is inside src.  Never read outside it.
        }
    }
    const unsigned prev_key = e0 > 0 ? keys[e0 - 1] : NO_KEY;
    const unsigned next_key = e0 + cnt < a.n ? keys[e0 + cnt] : NO_KEY;
    double *part = a.part + (size_t)blockIdx.x * 2 * a.C + col;

    double acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = 0.0;
    unsigned cur = (unsigned)__builtin_amdgcn_readlane((int)my_key, 0);
    bool head = cur == prev_key;                          // the first run began in an earlier chunk
    bool done = false;
    for (int j0 = 0; j0 < IA_CHUNK && !done; j0 += 4) {
        float v[4][VW];
        unsigned k4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                     // four row loads in flight
            k4[u] = (unsigned)__builtin_amdgcn_readlane((int)my_key, j0 + u);
            const long row = __builtin_amdgcn_readlane(my_row, j0 + u);
#pragma unroll
            for (int e = 0; e < VW; ++e) v[u][e] = 0.f;
            if (active && k4[u] < (unsigned)a.R && row >= 0) ld_chunk<float, VW>(a.src + row * a.ld_src + col, v[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (done) break;
            if (k4[u] != cur) {                           // a run ends inside the chunk (cur is a row: the sentinel comes last)
                if (active) {
                    if (head) {
#pragma unroll
                        for (int e = 0; e < VW; ++e) part[e] = acc[e];
                    } else {
                        ia_store_row<VW>(a.dst + (long)cur * a.ld_dst + col, acc);
                    }
                }
                head = false;
                cur = k4[u];
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = 0.0;
            }
            if (k4[u] >= (unsigned)a.R) {
                done = true;
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] += (double)v[u][e];
            }
        }
    }
    if (cur < (unsigned)a.R && active) {                  // the run the chunk ends in
        if (head) {
#pragma unroll
            for (int e = 0; e < VW; ++e) part[e] = acc[e];
        } else if (cur == next_key) {
#pragma unroll
            for (int e = 0; e < VW; ++e) part[a.C + e] = acc[e];
        } else {
            ia_store_row<VW>(a.dst + (long)cur * a.ld_dst + col, acc);
        }
    }
}

template <int VW>
__global__ __launch_bounds__(64) void stitch_kernel(IaArgs a, const unsigned *__restrict__ keys) {
    const long e1 = ((long)blockIdx.x + 1) * IA_CHUNK;    // the first entry of the next chunk
    if (e1 >= a.n) return;
    const unsigned key = keys[e1 - 1];
    if (key >= (unsigned)a.R || keys[e1] != key) return;  // nothing crosses into the next chunk
    if (blockIdx.x > 0 && keys[e1 - IA_CHUNK - 1] == key) return;      // the run began earlier: that chunk's wave adds it up
    const int col = ((int)blockIdx.y * 64 + (int)threadIdx.x) * VW;
    if (col >= a.C) return;
    const double *part = a.part + col;
    double acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = part[((size_t)blockIdx.x * 2 + 1) * a.C + e];
    for (long c = (long)blockIdx.x + 1;; ++c) {
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] += part[(size_t)c * 2 * a.C + e];
        const long nxt = (c + 1) * IA_CHUNK;
        if (nxt >= a.n || keys[nxt] != key) break;
    }
    ia_store_row<VW>(a.dst + (long)key * a.ld_dst + col, acc);
}

// a wave per row of dst: zeros where no sorted key names the row
template <int VW>
__global__ __launch_bounds__(256) void fill_kernel(IaArgs a, const unsigned *__restrict__ keys) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.R) return;
    long lo = 0, hi = a.n;                                // the first sorted entry whose key is >= row
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < (unsigned)row) lo = mid + 1; else hi = mid;
    }
    if (lo < a.n && keys[lo] == (unsigned)row) return;
    float zero[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) zero[e] = 0.f;
    for (int c = (threadIdx.x & 63) * VW; c < a.C; c += 64 * VW) st_chunk<float, VW>(a.dst + row * a.ld_dst + c, zero);
}

// ---- the forward: a sum of table rows ------------------------------------------------------------------------------------------------
struct EmbedSumArgs {
    vk_embed_tables t;
    const int32_t *idx, *out_row;
    const float *base;
    float *out;
    long M, ld_base, ld_out, out_rows;
    int C;
};

template <int VW>
__global__ __launch_bounds__(256) void embed_sum_kernel(EmbedSumArgs a) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;
    const int lane = threadIdx.x & 63;
    const float *rows[VK_EMBED_MAX_TABLES];
#pragma unroll
    for (int t = 0; t < VK_EMBED_MAX_TABLES; ++t)
        if (t < a.t.count) rows[t] = a.t.table[t] + clamp_row(a.idx[(long)t * a.M + m], a.t.rows[t]) * a.C;
    const long orow = a.out_row ? (long)a.out_row[m] : m;
    if (orow < 0 || orow >= a.out_rows) return;
    float *o = a.out + orow * a.ld_out;
    for (int c = lane * VW; c < a.C; c += 64 * VW) {
        float acc[VW], v[VW];
        if (a.base)
            ld_chunk<float, VW>(a.base + m * a.ld_base + c, acc);
        else
            ld_chunk<float, VW>(rows[0] + c, acc);
#pragma unroll
        for (int t = 0; t < VK_EMBED_MAX_TABLES; ++t)
            if (t < a.t.count && (t > 0 || a.base)) {
                ld_chunk<float, VW>(rows[t] + c, v);
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] += v[e];
            }
        st_chunk<float, VW>(o + c, acc);
    }
}

static int key_passes(long R) {                           // ceil(bits(R) / 8)
    int bits = 0;
    for (long v = R; v; v >>= 1) ++bits;
    return (bits + 7) / 8;
}
static size_t sort_tiles(long n) { return (size_t)((n + SORT_TILE - 1) / SORT_TILE); }
static size_t ia_chunks(long n) { return (size_t)((n + IA_CHUNK - 1) / IA_CHUNK); }
// the workspace: part [chunks][2][C] fp64 | keys [2][n] | perm [2][n] | count [256][tiles]
static size_t ia_part_bytes(long n, int C) { return ia_chunks(n) * 2 * (size_t)C * sizeof(double); }

}  // namespace vk

using namespace vk;

extern "C" {

size_t vk_index_add_rows_workspace_bytes(long n, long R, int C) {
    if (n < 1 || R < 1 || C < 1 || n >= (1l << 31) || R >= (1l << 31)) return 0;
    return ia_part_bytes(n, C) + (size_t)n * 16 + 256 * sort_tiles(n) * sizeof(unsigned);
}

int vk_index_add_rows_check(const float *src, long ld_src, long M, const int32_t *idx, const int32_t *src_row, long n, float *dst,
                            long ld_dst, long R, int C, int padding_idx, void *workspace, size_t workspace_bytes) {
    (void)src_row;
    VK_REQUIRE(src && idx && dst && workspace, VK_EINVAL, "index_add_rows: null argument (src, idx, dst and workspace are required)");
    VK_REQUIRE(n >= 1 && R >= 1 && C >= 1 && M >= 1, VK_EINVAL, "index_add_rows: sizes must be at least 1: n=%ld R=%ld C=%d M=%ld", n, R, C, M);
    VK_REQUIRE(n < (1l << 31) && R < (1l << 31), VK_EINVAL, "index_add_rows: n=%ld and R=%ld must lie below 2^31", n, R);
    VK_REQUIRE(ld_src >= C && ld_dst >= C, VK_EINVAL, "index_add_rows: leading dimensions ld_src=%ld ld_dst=%ld must be at least C=%d", ld_src,
               ld_dst, C);
    VK_REQUIRE(padding_idx == -1 || (padding_idx >= 0 && padding_idx < R), VK_EINVAL,
               "index_add_rows: padding_idx=%d must be -1 (none) or a row of [0, %ld)", padding_idx, R);
    VK_REQUIRE((((uintptr_t)src | (uintptr_t)idx | (uintptr_t)src_row | (uintptr_t)dst) & 3) == 0, VK_EINVAL,
               "index_add_rows: src, idx, src_row and dst must be 4-byte aligned");
    VK_REQUIRE(ia_chunks(n) <= 0x7fffffffu && ceil_div(C, 64) <= 65535, VK_EINVAL, "index_add_rows: n=%ld C=%d are beyond the grid", n, C);
    const size_t need = vk_index_add_rows_workspace_bytes(n, R, C);
    VK_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, VK_EINVAL,
               "index_add_rows: needs an 8-byte aligned workspace of %zu bytes, got %zu", need, workspace_bytes);
    return VK_OK;
}

int vk_index_add_rows(const float *src, long ld_src, long M, const int32_t *idx, const int32_t *src_row, long n, float *dst, long ld_dst,
                      long R, int C, int padding_idx, void *workspace, size_t workspace_bytes, void *stream) {
    VK_TRY(vk_index_add_rows_check(src, ld_src, M, idx, src_row, n, dst, ld_dst, R, C, padding_idx, workspace, workspace_bytes));
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)workspace;
    double *part = (double *)w;
    unsigned *keys[2];
    int32_t *perm[2];
    keys[0] = (unsigned *)(w + ia_part_bytes(n, C));
    keys[1] = keys[0] + n;
    perm[0] = (int32_t *)(keys[1] + n);
    perm[1] = perm[0] + n;
    unsigned *count = (unsigned *)(perm[1] + n);
    const IaArgs a = {src, idx, src_row, dst, part, ld_src, ld_dst, M, (int)n, (int)R, C, padding_idx};
    const int nwg = (int)sort_tiles(n), passes = key_passes(R);
    for (int p = 0; p < passes; ++p) {
        const SortArgs sa = {a, p ? keys[(p - 1) & 1] : nullptr, p ? perm[(p - 1) & 1] : nullptr, keys[p & 1], perm[p & 1], count, 8 * p, nwg};
        hipLaunchKernelGGL(sort_count_kernel, dim3(nwg), dim3(256), 0, s, sa);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(256), 0, s, count, (size_t)256 * nwg);
        hipLaunchKernelGGL(sort_place_kernel, dim3(nwg), dim3(256), 0, s, sa);
    }
    const unsigned *sk = keys[(passes - 1) & 1];
    const int32_t *sp = perm[(passes - 1) & 1];
    const bool chunked = row_chunked(4, (int)((C | ld_src | ld_dst) & 3), (uintptr_t)src | (uintptr_t)dst);
    const int vw = chunked ? 4 : 1;
    const dim3 grid((unsigned)ia_chunks(n), ceil_div(C, 64 * vw));
    const dim3 rows((unsigned)((R + 3) / 4));
    if (chunked) {
        hipLaunchKernelGGL(segsum_kernel<4>, grid, dim3(64), 0, s, a, sk, sp);
        hipLaunchKernelGGL(stitch_kernel<4>, grid, dim3(64), 0, s, a, sk);
        hipLaunchKernelGGL(fill_kernel<4>, rows, dim3(256), 0, s, a, sk);
    } else {
        hipLaunchKernelGGL(segsum_kernel<1>, grid, dim3(64), 0, s, a, sk, sp);
        hipLaunchKernelGGL(stitch_kernel<1>, grid, dim3(64), 0, s, a, sk);
        hipLaunchKernelGGL(fill_kernel<1>, rows, dim3(256), 0, s, a, sk);
    }
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_embed_sum_f32(const vk_embed_tables *tables, const int32_t *idx, long M, int C, const float *base, long ld_base, const int32_t *out_row,
                     float *out, long ld_out, long out_rows, void *stream) {
    VK_REQUIRE(tables && idx && out, VK_EINVAL, "embed_sum_f32: null argument");
    VK_REQUIRE(tables->count >= 1 && tables->count <= VK_EMBED_MAX_TABLES, VK_EINVAL, "embed_sum_f32: %d tables, 1..%d are taken", tables->count,
               VK_EMBED_MAX_TABLES);
    VK_REQUIRE(M >= 1 && M < (1l << 31) && C >= 1 && ld_out >= C && (!base || ld_base >= C) && out_rows >= (out_row ? 1 : M), VK_EINVAL,
               "embed_sum_f32: bad shape M=%ld C=%d ld_base=%ld ld_out=%ld out_rows=%ld", M, C, ld_base, ld_out, out_rows);
    uintptr_t bases = (uintptr_t)base | (uintptr_t)out;
    for (int t = 0; t < tables->count; ++t) {
        VK_REQUIRE(tables->table[t] && tables->rows[t] >= 1, VK_EINVAL, "embed_sum_f32: table %d is null or has no rows", t);
        bases |= (uintptr_t)tables->table[t];
    }
    EmbedSumArgs a = {*tables, idx, out_row, base, out, M, ld_base, ld_out, out_rows, C};
    const bool chunked = row_chunked(4, (int)((C | ld_out | (base ? ld_base : 0)) & 3), bases);
    return chunked ? row_launch(embed_sum_kernel<4>, M, (hipStream_t)stream, a) : row_launch(embed_sum_kernel<1>, M, (hipStream_t)stream, a);
}

}  // extern "C"
