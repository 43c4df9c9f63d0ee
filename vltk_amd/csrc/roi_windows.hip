// Distinct RoIPool windows of a Res5 chunk.
//
// RoIPool (pool.hip: roi_pool_kernel, torchvision semantics, oracle/tv_ops.c) turns a box into P x P bins, and a bin pools the
// clamped cell window [y0, y1) x [x0, x1) of its image's res4 map.  Boxes narrower than P cells give windows of one or two cells
// on a side, so neighbouring bins of a RoI and bins of overlapping RoIs pool the same window -- and everything Res5 block 0 computes
// from a pooled row alone (its conv1) is then the same row again.  This file finds the distinct windows on the device:
//   vk_roi_windows        idx[row] = id of the row's window, win[id] = (image, y0, y1, x0, x1), *u_dev = number of ids
//   vk_roi_pool_windows   pooled_u[id] = the row roi_pool_kernel writes for every bin with that window (bit-equal)
//   vk_gather_rows        dst[row] = src[idx[row]] in 16-byte lanes (conv1's rows back to the dense tensor; "pooled" on demand)
//   vk_roi_neighbourhoods nid[row] = id of the row's NINE-window neighbourhood (its own window and the eight a dilated 3x3 reads),
//                         rep[id] = the smallest row with it, idx_rep[id] = idx[rep[id]], *v_dev = number of ids
//   vk_roi_out_rows       out_row[row] = nid[row] where rep[nid[row]] == row, -1 elsewhere: where conv2 stores the row
// Ids are the RANK of the window's key (image, y0, y1, x0, x1) among the keys present, so they do not depend on the order in which
// the device happens to run anything: one bit per possible key, a marking pass, popcount sums over 8-word blocks, a two-level
// exclusive scan of the block sums, and id = scanned sum + popcount of the bits below the key's own.  No host read-back, no
// synchronisation: the consumers read *u_dev on the device.
#include "vk_common.h"

namespace vk {

constexpr int RW_BLK = 8;        // bitmap words per block sum
constexpr int RW_GRP = 1024;     // block sums per group of the scan

// The window of bin (ph, pw) of RoI r, exactly as roi_pool_kernel computes it (same rounding, float bin size, floor / ceil, clamp).
// An empty window (y1 <= y0 or x1 <= x0) is a key like any other: its row is all zeros.
__device__ __forceinline__ void roi_bin_window(const float *__restrict__ r, int ph, int pw, int N, int H, int W, int P, float scale,
                                               int &b, int &y0, int &y1, int &x0, int &x1) {
    b = min(max((int)r[0], 0), N - 1);
    const int rsw = (int)roundf(r[1] * scale), rsh = (int)roundf(r[2] * scale);
    const int rew = (int)roundf(r[3] * scale), reh = (int)roundf(r[4] * scale);
    const int roi_w = max(rew - rsw + 1, 1), roi_h = max(reh - rsh + 1, 1);
    const float bin_h = (float)roi_h / (float)P, bin_w = (float)roi_w / (float)P;
    int hs = (int)floorf((float)ph * bin_h), he = (int)ceilf((float)(ph + 1) * bin_h);
    y0 = min(max(hs + rsh, 0), H);
    y1 = min(max(he + rsh, 0), H);
    int ws = (int)floorf((float)pw * bin_w), we = (int)ceilf((float)(pw + 1) * bin_w);
    x0 = min(max(ws + rsw, 0), W);
    x1 = min(max(we + rsw, 0), W);
}

__device__ __forceinline__ unsigned long long window_key(int b, int y0, int y1, int x0, int x1, int H, int W) {
    return ((((unsigned long long)b * (H + 1) + y0) * (H + 1) + y1) * (W + 1) + x0) * (W + 1) + x1;
}

__global__ void rw_mark_kernel(const float *__restrict__ rois, long rows, int N, int H, int W, int P, float scale,
                               unsigned *__restrict__ bits) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int pw = (int)(row % P), ph = (int)((row / P) % P);
    int b, y0, y1, x0, x1;
    roi_bin_window(rois + 5 * (row / ((long)P * P)), ph, pw, N, H, W, P, scale, b, y0, y1, x0, x1);
    const unsigned long long key = window_key(b, y0, y1, x0, x1, H, W);
    atomicOr(bits + (key >> 5), 1u << (unsigned)(key & 31));
}

// bsum[i] = set bits of block i (RW_BLK words; the bitmap is padded to whole blocks, bsum to whole groups)
__global__ void rw_block_sums_kernel(const unsigned *__restrict__ bits, long n_blocks, long n_padded, unsigned *__restrict__ bsum) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_padded) return;
    unsigned c = 0;
    if (i < n_blocks) {
        const uint4 a = reinterpret_cast<const uint4 *>(bits)[2 * i], d = reinterpret_cast<const uint4 *>(bits)[2 * i + 1];
        c = __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(d.x) + __popc(d.y) + __popc(d.z) + __popc(d.w);
    }
    bsum[i] = c;
}

// exclusive scan of 256 per-thread values through LDS (Hillis-Steele); returns the thread's offset, *total the sum of all
__device__ __forceinline__ unsigned scan256(unsigned v, unsigned *sh, unsigned *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned incl = sh[t];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}

// one workgroup per group of RW_GRP block sums: exclusive scan in place, the group's total to gsum
__global__ __launch_bounds__(256) void rw_group_scan_kernel(unsigned *__restrict__ bsum, unsigned *__restrict__ gsum) {
    __shared__ unsigned sh[256];
    uint4 *p = reinterpret_cast<uint4 *>(bsum + (long)blockIdx.x * RW_GRP) + threadIdx.x;
    const uint4 v = *p;
    unsigned total;
    const unsigned off = scan256(v.x + v.y + v.z + v.w, sh, &total);
    *p = uint4{off, off + v.x, off + v.x + v.y, off + v.x + v.y + v.z};
    if (threadIdx.x == 0) gsum[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the group totals in place, 256 at a time with a carry; the grand total is the id count
__global__ __launch_bounds__(256) void rw_top_scan_kernel(unsigned *__restrict__ gsum, int n_groups, int32_t *__restrict__ u_dev) {
    __shared__ unsigned sh[256];
    unsigned carry = 0;
    for (int g0 = 0; g0 < n_groups; g0 += 256) {
        const int g = g0 + (int)threadIdx.x;
        const unsigned v = g < n_groups ? gsum[g] : 0u;
        unsigned total;
        const unsigned off = scan256(v, sh, &total);
        if (g < n_groups) gsum[g] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) *u_dev = (int32_t)carry;
}

// the rank of set bit `key`: set bits below it (scanned block sums + popcounts inside its block)
__device__ __forceinline__ unsigned rw_rank(const unsigned *__restrict__ bits, const unsigned *__restrict__ bsum, const unsigned *__restrict__ gsum,
                                            unsigned long long key) {
    const unsigned long long word = key >> 5, blk = word / RW_BLK;
    unsigned id = gsum[blk / RW_GRP] + bsum[blk];
    for (unsigned long long w = blk * RW_BLK; w < word; ++w) id += __popc(bits[w]);
    return id + __popc(bits[word] & ((1u << (unsigned)(key & 31)) - 1u));
}

// every bin of one window writes the same five values to win[id]
__global__ void rw_assign_kernel(const float *__restrict__ rois, long rows, int N, int H, int W, int P, float scale,
                                 const unsigned *__restrict__ bits, const unsigned *__restrict__ bsum, const unsigned *__restrict__ gsum,
                                 int32_t *__restrict__ idx, int32_t *__restrict__ win) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int pw = (int)(row % P), ph = (int)((row / P) % P);
    int b, y0, y1, x0, x1;
    roi_bin_window(rois + 5 * (row / ((long)P * P)), ph, pw, N, H, W, P, scale, b, y0, y1, x0, x1);
    const unsigned long long key = window_key(b, y0, y1, x0, x1, H, W);
    const unsigned id = rw_rank(bits, bsum, gsum, key);
    idx[row] = (int32_t)id;
    int32_t *o = win + 5 * (long)id;
    o[0] = b;
    o[1] = y0;
    o[2] = y1;
    o[3] = x0;
    o[4] = x1;
}

// RoIPool of the distinct windows: the f16 branch of roi_pool_kernel on a window from the list (packed maximum, -inf start,
// zeros for an empty window).  A workgroup takes 256 / (C / 8) windows per step and strides over the *u_dev ids.
__global__ __launch_bounds__(256) void roi_pool_windows_kernel(const _Float16 *__restrict__ feat, const int32_t *__restrict__ win,
                                                               const int32_t *__restrict__ u_dev, int max_u, _Float16 *__restrict__ out,
                                                               int H, int W, int C) {
    typedef _Float16 vec __attribute__((ext_vector_type(8)));
    const int U = min(*u_dev, max_u);
    const int cv = C / 8;
    const int wpb = cv >= 256 ? 1 : 256 / cv, cstep = cv >= 256 ? 256 : cv;
    const int wi = (int)threadIdx.x / cstep;
    if (wi >= wpb) return;
    for (long u = (long)blockIdx.x * wpb + wi; u < U; u += (long)gridDim.x * wpb) {
        const int32_t *wd = win + 5 * u;
        const int b = wd[0], hs = wd[1], he = wd[2], ws = wd[3], we = wd[4];
        const bool empty = (he <= hs) || (we <= ws);
        const _Float16 *fb = feat + (long)b * H * W * C;
        for (int c = (int)threadIdx.x % cstep; c < cv; c += cstep) {
            vec o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = empty ? (_Float16)0.f : (_Float16)(-__builtin_inff());
            for (int h = hs; h < he; ++h)
                for (int w = ws; w < we; ++w) o = __builtin_elementwise_max(o, reinterpret_cast<const vec *>(fb + ((long)h * W + w) * C)[c]);
            reinterpret_cast<vec *>(out + u * C)[c] = o;
        }
    }
}

// dst[row] = src[idx[row]], rows of `chunks` 16-byte lanes
// (rows_dev: the row count lives on the device, `rows` bounds it)
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4 *__restrict__ src, const int32_t *__restrict__ idx, long rows,
                                                          const int32_t *__restrict__ rows_dev, int chunks, uint4 *__restrict__ dst) {
    if (rows_dev) rows = min((long)*rows_dev, rows);
    const long total = rows * chunks;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / chunks;
        const int c = (int)(i - row * chunks);
        dst[i] = src[(long)idx[row] * chunks + c];
    }
}

// ---- distinct nine-window neighbourhoods ----
// Res5 block 0 is stride 1 with a 3x3 of dilation d, so its output row at bin (k, i, j) -- and with it block 0's shortcut operand and
// conv1 of block 1 -- is a function of the nine windows at (i + {-d, 0, d}, j + {-d, 0, d}), "outside the P x P map" being a value of
// its own.  Window ids are ranks of the full (image, y0, y1, x0, x1) key, so nine equal ids (-1 = outside) ARE nine equal keys.
// Two rows are merged only after all nine ids compared equal: the hash below picks where a probe starts and nothing else.
//   insert   open addressing over row numbers: a slot is claimed by the first row that finds it empty; a row whose nine ids equal those
//            of the slot's row lowers the slot to min(row) (the ids a slot stands for never change once it is claimed), any other row
//            moves on to the next slot.  After the kernel a slot holds the SMALLEST row of its neighbourhood, whatever ran first.
//   find     every row probes to its slot again and notes that smallest row (in nid[], for the moment); the smallest rows mark their
//            bit in a bitmap over the rows
//   rank     the window table's block sums and two-level scan over that bitmap; *v_dev = set bits
//   assign   nid[row] = rank of the row's smallest row; the smallest rows write rep[] and idx_rep[]
// So ids number the neighbourhoods in the order of their smallest rows: a function of the chunk's boxes alone, rep[] ascending.
constexpr int NB_OUT = -1;

__device__ __forceinline__ void nbr_ids(const int32_t *__restrict__ idx, long row, int P, int d, int (&k)[9]) {
    const int pw = (int)(row % P), ph = (int)((row / P) % P);
    const int32_t *roi = idx + (row - (long)ph * P - pw);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int i = ph + (a - 1) * d, j = pw + (b - 1) * d;
            k[a * 3 + b] = (i >= 0 && i < P && j >= 0 && j < P) ? roi[i * P + j] : NB_OUT;
        }
}

__device__ __forceinline__ bool nbr_same(const int32_t *__restrict__ idx, long other, int P, int d, const int (&k)[9]) {
    int o[9];
    nbr_ids(idx, other, P, d, o);
    bool same = true;
#pragma unroll
    for (int t = 0; t < 9; ++t) same = same && o[t] == k[t];
    return same;
}

__device__ __forceinline__ unsigned nbr_hash(const int (&k)[9]) {
    unsigned h = 2166136261u;
#pragma unroll
    for (int t = 0; t < 9; ++t) h = (h ^ (unsigned)k[t]) * 16777619u;
    return h ^ (h >> 15);
}

__global__ void nb_insert_kernel(const int32_t *__restrict__ idx, long rows, int P, int d, int *__restrict__ table, unsigned mask) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    int k[9];
    nbr_ids(idx, row, P, d, k);
    for (unsigned slot = nbr_hash(k) & mask;; slot = (slot + 1) & mask) {       // (the table has at least two slots per row: a probe ends)
        const int cur = atomicCAS(table + slot, -1, (int)row);
        if (cur < 0) return;                                                     // claimed
        if (nbr_same(idx, cur, P, d, k)) {
            atomicMin(table + slot, (int)row);
            return;
        }
    }
}

__global__ void nb_find_kernel(const int32_t *__restrict__ idx, long rows, int P, int d, const int *__restrict__ table, unsigned mask,
                               int32_t *__restrict__ first, unsigned *__restrict__ bits) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    int k[9];
    nbr_ids(idx, row, P, d, k);
    for (unsigned slot = nbr_hash(k) & mask;; slot = (slot + 1) & mask) {
        int cur = table[slot];                                                   // (never empty before the row's own slot: it was inserted)
        if (cur < 0) cur = (int)row;
        if (cur == (int)row || nbr_same(idx, cur, P, d, k)) {
            first[row] = cur;
            if (cur == (int)row) atomicOr(bits + (row >> 5), 1u << (unsigned)(row & 31));
            return;
        }
    }
}

__global__ void nb_assign_kernel(const int32_t *__restrict__ idx, long rows, const unsigned *__restrict__ bits, const unsigned *__restrict__ bsum,
                                 const unsigned *__restrict__ gsum, int32_t *__restrict__ nid, int32_t *__restrict__ rep,
                                 int32_t *__restrict__ idx_rep) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int32_t f = nid[row];                                                  // the smallest row of this row's neighbourhood (nb_find_kernel)
    const unsigned id = rw_rank(bits, bsum, gsum, (unsigned long long)f);
    nid[row] = (int32_t)id;
    if (f == (int32_t)row) {
        rep[id] = (int32_t)row;
        idx_rep[id] = idx[row];
    }
}

// out_row[row] = the row's neighbourhood id where the row is that neighbourhood's representative, -1 elsewhere: every
// id of [0, V) exactly once, ascending with the row since rep[] is.  The panel kernel stores its output rows through it.
__global__ void nb_out_rows_kernel(const int32_t *__restrict__ nid, const int32_t *__restrict__ rep, long rows, int32_t *__restrict__ out_row) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int32_t id = nid[row];
    out_row[row] = rep[id] == (int32_t)row ? id : -1;
}

struct RwLayout {
    size_t n_words, n_blocks, n_blocks_padded, n_groups;
    size_t off_bsum, off_gsum, total;
};

// the bitmap over `nbits` keys with its block sums and group sums, from byte `base` of a workspace on
static void rw_carve(size_t nbits, size_t base, RwLayout *L) {
    L->n_blocks = (nbits + 32 * RW_BLK - 1) / (32 * RW_BLK);
    L->n_words = L->n_blocks * RW_BLK;
    L->n_groups = (L->n_blocks + RW_GRP - 1) / RW_GRP;
    L->n_blocks_padded = L->n_groups * RW_GRP;
    L->off_bsum = base + align_up(L->n_words * 4, 256);
    L->off_gsum = L->off_bsum + align_up(L->n_blocks_padded * 4, 256);
    L->total = L->off_gsum + align_up(L->n_groups * 4, 256);
}

// the neighbourhood table's workspace: the slots (a power of two, two per row at least), then a bitmap over the rows
static bool nb_layout(long rows, size_t *slots, RwLayout *L) {
    if (rows <= 0 || rows >= (1L << 30)) return false;
    size_t t = 1024;
    while (t < 2 * (size_t)rows) t <<= 1;
    *slots = t;
    rw_carve((size_t)rows, t * sizeof(int), L);
    return true;
}

static bool rw_layout(int N, int H, int W, RwLayout *L) {
    if (N <= 0 || H <= 0 || W <= 0) return false;
    const double nbits_d = (double)N * (H + 1) * (H + 1) * (double)(W + 1) * (W + 1);
    if (nbits_d >= 34359738368.0) return false;                    // 2^35 bits = 4 GiB of bitmap: beyond any map this is meant for
    const size_t nbits = (size_t)N * (H + 1) * (H + 1) * (size_t)(W + 1) * (W + 1);
    rw_carve(nbits, 0, L);
    return true;
}

}  // namespace vk

using namespace vk;

extern "C" {

size_t vk_roi_windows_workspace_bytes(int N, int H, int W) {
    RwLayout L;
    return rw_layout(N, H, W, &L) ? L.total : 0;
}

int vk_roi_windows(const float *rois, int K, int N, int H, int W, int P, float spatial_scale, int32_t *idx, int32_t *win,
                   int32_t *u_dev, void *workspace, size_t workspace_bytes, void *stream) {
    VK_REQUIRE(rois && idx && win && u_dev && workspace && K > 0 && P > 0, VK_EINVAL, "roi_windows: bad arguments");
    RwLayout L;
    VK_REQUIRE(rw_layout(N, H, W, &L), VK_EINVAL, "roi_windows: %d maps of %d x %d need a bitmap beyond 4 GiB", N, H, W);
    VK_REQUIRE(workspace_bytes >= L.total, VK_EINVAL, "roi_windows: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    VK_REQUIRE(((uintptr_t)workspace & 15) == 0, VK_EINVAL, "roi_windows: workspace must be 16-byte aligned");
    const long rows = (long)K * P * P;
    VK_REQUIRE(rows < (1L << 31), VK_EINVAL, "roi_windows: %ld rows", rows);
    hipStream_t s = (hipStream_t)stream;
    unsigned *bits = (unsigned *)workspace;
    unsigned *bsum = (unsigned *)((char *)workspace + L.off_bsum), *gsum = (unsigned *)((char *)workspace + L.off_gsum);
    VK_CHECK_HIP(hipMemsetAsync(bits, 0, L.n_words * 4, s));
    const unsigned row_grid = (unsigned)((rows + 255) / 256);
    hipLaunchKernelGGL(rw_mark_kernel, dim3(row_grid), dim3(256), 0, s, rois, rows, N, H, W, P, spatial_scale, bits);
    hipLaunchKernelGGL(rw_block_sums_kernel, dim3((unsigned)(L.n_blocks_padded / 256)), dim3(256), 0, s, bits, (long)L.n_blocks,
                       (long)L.n_blocks_padded, bsum);
    hipLaunchKernelGGL(rw_group_scan_kernel, dim3((unsigned)L.n_groups), dim3(256), 0, s, bsum, gsum);
    hipLaunchKernelGGL(rw_top_scan_kernel, dim3(1), dim3(256), 0, s, gsum, (int)L.n_groups, u_dev);
    hipLaunchKernelGGL(rw_assign_kernel, dim3(row_grid), dim3(256), 0, s, rois, rows, N, H, W, P, spatial_scale, bits, bsum, gsum, idx, win);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

size_t vk_roi_neighbourhoods_workspace_bytes(long rows) {
    size_t slots;
    RwLayout L;
    return nb_layout(rows, &slots, &L) ? L.total : 0;
}

int vk_roi_neighbourhoods(const int32_t *idx, int K, int P, int dil, int32_t *nid, int32_t *rep, int32_t *idx_rep, int32_t *v_dev,
                          void *workspace, size_t workspace_bytes, void *stream) {
    VK_REQUIRE(idx && nid && rep && idx_rep && v_dev && workspace && K > 0 && P > 0 && dil >= 1, VK_EINVAL, "roi_neighbourhoods: bad arguments");
    const long rows = (long)K * P * P;
    size_t slots;
    RwLayout L;
    VK_REQUIRE(nb_layout(rows, &slots, &L), VK_EINVAL, "roi_neighbourhoods: %ld rows", rows);
    VK_REQUIRE(workspace_bytes >= L.total, VK_EINVAL, "roi_neighbourhoods: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    VK_REQUIRE(((uintptr_t)workspace & 15) == 0, VK_EINVAL, "roi_neighbourhoods: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int *table = (int *)workspace;
    unsigned *bits = (unsigned *)((char *)workspace + slots * sizeof(int));
    unsigned *bsum = (unsigned *)((char *)workspace + L.off_bsum), *gsum = (unsigned *)((char *)workspace + L.off_gsum);
    VK_CHECK_HIP(hipMemsetAsync(table, 0xff, slots * sizeof(int), s));          // every slot empty (-1)
    VK_CHECK_HIP(hipMemsetAsync(bits, 0, L.n_words * 4, s));
    const unsigned row_grid = (unsigned)((rows + 255) / 256);
    hipLaunchKernelGGL(nb_insert_kernel, dim3(row_grid), dim3(256), 0, s, idx, rows, P, dil, table, (unsigned)(slots - 1));
    hipLaunchKernelGGL(nb_find_kernel, dim3(row_grid), dim3(256), 0, s, idx, rows, P, dil, table, (unsigned)(slots - 1), nid, bits);
    hipLaunchKernelGGL(rw_block_sums_kernel, dim3((unsigned)(L.n_blocks_padded / 256)), dim3(256), 0, s, bits, (long)L.n_blocks,
                       (long)L.n_blocks_padded, bsum);
    hipLaunchKernelGGL(rw_group_scan_kernel, dim3((unsigned)L.n_groups), dim3(256), 0, s, bsum, gsum);
    hipLaunchKernelGGL(rw_top_scan_kernel, dim3(1), dim3(256), 0, s, gsum, (int)L.n_groups, v_dev);
    hipLaunchKernelGGL(nb_assign_kernel, dim3(row_grid), dim3(256), 0, s, idx, rows, bits, bsum, gsum, nid, rep, idx_rep);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_roi_out_rows(const int32_t *nid, const int32_t *rep, long rows, int32_t *out_row, void *stream) {
    VK_REQUIRE(nid && rep && out_row && rows > 0 && rows < (1L << 30), VK_EINVAL, "roi_out_rows: bad arguments (%ld rows)", rows);
    hipLaunchKernelGGL(nb_out_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nid, rep, rows, out_row);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_roi_pool_windows(const void *feat, int N, int H, int W, int C, const int32_t *win, const int32_t *u_dev, int max_u, void *out,
                        vk_dtype dt, void *stream) {
    (void)N;
    VK_REQUIRE(feat && win && u_dev && out && max_u > 0, VK_EINVAL, "roi_pool_windows: bad arguments");
    VK_REQUIRE(dt == VK_F16 && C % 8 == 0 && C >= 8, VK_EINVAL, "roi_pool_windows: f16 rows of whole 16-byte lanes only (C=%d)", C);
    DeviceState *ds = nullptr;
    VK_TRY(device_state(&ds));
    const int cv = C / 8, wpb = cv >= 256 ? 1 : 256 / cv;
    const long need = ((long)max_u + wpb - 1) / wpb, cap = (long)ds->n_cu * 16;
    hipLaunchKernelGGL(roi_pool_windows_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16 *)feat, win, u_dev, max_u, (_Float16 *)out, H, W, C);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

int vk_gather_rows(const void *src, const int32_t *idx, long rows, int row_bytes, void *dst, void *stream) {
    return vk_gather_rows_dev(src, idx, rows, nullptr, row_bytes, dst, stream);
}

int vk_gather_rows_dev(const void *src, const int32_t *idx, long rows, const int32_t *rows_dev, int row_bytes, void *dst, void *stream) {
    VK_REQUIRE(src && idx && dst && rows > 0, VK_EINVAL, "gather_rows: bad arguments");
    VK_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, VK_EINVAL, "gather_rows: rows of whole 16-byte lanes only (%d bytes)", row_bytes);
    DeviceState *ds = nullptr;
    VK_TRY(device_state(&ds));
    const int chunks = row_bytes / 16;
    const long need = (rows * chunks + 255) / 256, cap = (long)ds->n_cu * 16;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(256), 0, (hipStream_t)stream, (const uint4 *)src,
                       idx, rows, rows_dev, chunks, (uint4 *)dst);
    VK_CHECK_HIP(hipGetLastError());
    return VK_OK;
}

}  // extern "C"
