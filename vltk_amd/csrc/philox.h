// The dropout mask of the training kernels (dropout.hip, attention.hip, attention_grad16.hip): Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11) in plain C++, integer multiplies only, no state.  Host and
// device compile the same text.
//
// A decision is a pure function of (seed, stream, granule, byte), whatever the launch geometry, the tile order or the wave count:
//   key      (seed_lo, seed_hi)
//   counter  (granule_lo, granule_hi, stream_lo, stream_hi)
//   bytes    one call yields 16: byte i is bits 8 (i & 3) .. of output word i >> 2
//   rule     t = lrintf(p * 256); an element is kept iff byte >= t; the rate in effect is t / 256 and a survivor is scaled by
//            rs = 256.0f / (256 - t), one fp32 division
//   granule  elementwise, n contiguous floats: element i is byte i & 15 of granule i >> 4
//            attention, element (b, h, q, k): byte 4 (q & 3) + (k & 3) of granule
//            ((b heads + h) ceil(Lq / 4) + (q >> 2)) ceil(Lk / 4) + (k >> 2), a 64-bit number: a 4 x 4 block of the probability
//            matrix per call, word = q & 3, byte of the word = k & 3, which a transposition maps onto itself
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_PHILOX_FN __host__ __device__ __forceinline__
#else
#define VK_PHILOX_FN inline
#endif

namespace vk {

struct Philox4 {
    uint32_t w[4];
};

VK_PHILOX_FN Philox4 philox4x32_10(uint64_t seed, uint64_t stream, uint64_t granule) {
    uint32_t c0 = (uint32_t)granule, c1 = (uint32_t)(granule >> 32), c2 = (uint32_t)stream, c3 = (uint32_t)(stream >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

VK_PHILOX_FN uint32_t philox_byte(const Philox4 &r, int i) { return (r.w[i >> 2] >> (8 * (i & 3))) & 255u; }

// t of the rule for a rate p, or -1 where the entry points refuse p (p < 0, p >= 1, NaN, or a t above 255)
inline int dropout_threshold(float p) {
    if (!(p >= 0.0f && p < 1.0f)) return -1;
    const long t = lrintf(p * 256.0f);
    return t > 255 ? -1 : (int)t;
}
inline float dropout_scale(int t) { return 256.0f / (float)(256 - t); }

// The keep bits of one call as a word: bit 8 c + w is set iff byte c of word w is >= t (0 <= t <= 255).  Four bytes of a word are
// compared at once: the low seven bits by a subtraction that cannot borrow across bytes, then the top bits.
VK_PHILOX_FN uint32_t philox_keep16(const Philox4 &r, uint32_t t) {
    const uint32_t H = 0x80808080u, T = t * 0x01010101u;
    uint32_t m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t x = r.w[w];
        const uint32_t low = (x | H) - (T & ~H);                        // bit 7 of a byte: its low seven bits are >= t's
        const uint32_t ge = ((x & ~T) | (~(x ^ T) & low)) & H;
        m |= (ge >> 7) << w;
    }
    return m;
}

// the arguments the kernels take: the threshold, the survivors' scale and the two 64-bit numbers of the key and the counter
struct DropArgs {
    uint32_t t;
    float rs;
    uint64_t seed, stream;
};

#if defined(__HIPCC__)
// the DropArgs a DROP kernel takes as its one trailing argument; a plain kernel takes none
template <typename... A>
static __device__ __forceinline__ DropArgs drop_args_of(A... a) {
    if constexpr (sizeof...(A) == 1) return (a, ...);
    else return DropArgs{};
}

// The attention kernels' exchange.  A 16 x 64 tile of the probability matrix (16 queries x 64 keys in the forward and dQ kernels,
// 64 queries x 16 keys in the dK/dV kernel) is 64 blocks of the mask, one per lane: lane 16 g + jj makes the one Philox call of the
// block whose index along the tile's 16-wide side is g and along its 64-wide side jj, and folds it into 16 keep bits.  A lane of
// group g that holds the elements of column 16 n + j of the 64-wide side needs block (g, 4 n + (j >> 2)): bits[n] is that block's
// word, fetched from lane 16 g + 4 n + (j >> 2) (ds_bpermute_b32); bit 8 (k & 3) + (q & 3) of it decides element (q, k).
// Where a tile overhangs Lq or Lk its lanes take granules past the row's last block (the next row's, or past the matrix): harmless,
// those elements are padding that no result reads.
// `first` + query block is the row of blocks, `pitch` = ceil(Lk / 4) blocks per row; qb0, kb0: the tile's first query and key block.
static __device__ __forceinline__ void drop_tile_bits(uint32_t (&bits)[4], const DropArgs &da, uint64_t first, uint64_t pitch, int qb0, int kb0,
                                                      bool queries_are_g, int g, int j) {
    const uint64_t qb = (uint64_t)(qb0 + (queries_are_g ? g : j)), kb = (uint64_t)(kb0 + (queries_are_g ? j : g));
    const uint32_t mine = philox_keep16(philox4x32_10(da.seed, da.stream, (first + qb) * pitch + kb), da.t);
#pragma unroll
    for (int n = 0; n < 4; ++n) bits[n] = (uint32_t)__shfl((int)mine, 16 * g + 4 * n + (j >> 2), 64);
}
#endif

}  // namespace vk
