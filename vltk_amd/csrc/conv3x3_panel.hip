// 3x3 convolution (stride 1, pad == dilation) with an LDS-RESIDENT INPUT PANEL: the conv-native kernel
// for the layers where an im2col GEMM wastes the most bytes (Res5 conv2 with dilation 2, res4 conv2, RPN 3x3).
//
// Why: the 256x256 im2col ring kernel (conv_mfma256.hip) is bound by the supply of distinct cache lines
// through the CU's L1-miss path (~15 B/clk/CU) and an im2col GEMM fetches every input pixel
// NINE times (once per tap).  Here K is walked channel-stage-major / tap-minor: the 32-channel slab of the
// tile's pixels PLUS HALO (all pixels any tap can touch) is brought into LDS ONCE per channel stage and the
// nine taps read it at nine row shifts; only the weights stream per (tap, stage).  Bytes through the CU per
// 32-channel stage: 9 x 16 KiB weights + ~24-32 KiB panel  vs  9 x 32 KiB  (-40...-45 %).
//
//   * LDS: 2 panel buffers of PP*128 rows x 64 B (PP = 3 or 4: halo 64 / 128 rows >= dil*(W+1)) + a ring of
//     6 weight slots (256 channels x 64 B): 144 / 160 KiB.  Same 64-B-row XOR swizzle as the ring kernel,
//     applied on the DMA source address; the fragment address is recomputed per tap (the shift moves the key).
//   * a tap is a UNIFORM row shift ((kh-1)*W + (kw-1))*dil of the fragment reads; pixels whose tap falls outside
//     the image (or into the neighbouring image, or rows >= M) are zeroed in registers from a precomputed
//     72-bit per-lane validity mask (4 v_cndmask per fragment).
//   * per step (one tap of one stage) = 32 MFMAs per wave, one raw barrier, 2 weight DMA pieces per wave,
//     plus one panel piece of the NEXT channel stage on the first PP taps; hand-issued ds_read_b128 with
//     counted lgkmcnt, counted vmcnt (the count depends only on the tap index: compile-time).
//   * same per-wave geometry (2x4 waves, 128x64 per wave, 16x16x32 f16 MFMA) as conv_mfma256.hip and, in its first
//     form (DBG & 8), the same LDS-staged whole-row epilogue (StagedEpi, conv_prims.h).
//   * PHASE form (dilation 2, even H, even W <= 14): the kernel's INTERNAL row order is
//     [group of 16 images][phase = (y & 1, x & 1)][qy][qx][image % 16], so an aligned 16-row MFMA tile is one position of
//     the (H/2) x (W/2) grid of one phase in 16 images: a tap is a uniform shift of (dy * W/2 + dx) * 16 rows and is inside
//     the image for all 16 rows or for none.  Validity is a per-wave scalar, a (row tile, tap) outside the image issues no MFMAs.
//     x and y keep their natural [image][y][x] rows: only the DMA source row of a panel piece and the epilogue's row are permuted.
//     Its tile is 512 rows x 128 channels (4x2 waves, WR = 4): 2 panel buffers of 768 rows (48 KiB) + 6 weight slots
//     of 128 channels (8 KiB) = 144 KiB, 9 x 8 + 48 = 120 KiB through the CU per stage and 65 536 outputs instead of 176, one
//     weight DMA piece per wave and step.  VK_PANEL_TALL=0 selects the 256 x 256 tile (same bits).
//     On that tile the three taps of a tap row work from ONE window of ten fragment registers (REUSE): a tap shift is
//     whole 16-row tiles, so (row tile mi, tap dx) and (mi - 1, dx + 1) are the same LDS bytes at the same lane address.  30 A-fragment
//     ds_read_b128 per wave and stage instead of 72 (66 instead of 108 with the weights), the same MFMAs on the same operands in the
//     same order.  VK_PANEL_REUSE=0 selects the schedule in which every tap reads its eight fragments (same bits).
#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "vk_common.h"
#include "conv_prims.h"

namespace vk {

struct PanelK {
    const char *x;
    const char *w;
    const float *bias;
    const char *res;
    char *y;
    int H, W, HW, M;
    int cin_bytes, ldy;
    int dil;
    int cstages;              // Cin / 32 (even)
    int wrow_bytes;           // 9 * Cin * 2
    int relu;
    int m_tiles, n_tiles;
    unsigned long *stamps;    // DBG & 4 builds: 6 words per workgroup
    // Dynamic tail (round 3; two-panel launches of many rounds only).  The dispatcher gives every XCD the same number of workgroups
    // (blockIdx mod 8) and the XCDs of one chip differ by ~4.5 % in speed at the power limit (stamps: the last workgroup of the slowest
    // ends 300 us after the fastest's on a 7.1 ms launch, 2 % of the CU time idle).  Workgroups [0, static_tiles) take the tile of their
    // index as before; the grid carries `total - static_tiles` + spare further workgroups, each of which takes the next tail tile from an
    // atomic counter when it STARTS (so a fast XCD does more of them) and leaves at once when none is left.
    unsigned *tile_ctr;       // nullptr: every workgroup is its own tile
    int static_tiles;
    unsigned ctr_last;        // the launch's last fetch (one per tail workgroup): whoever draws it zeroes the word for its next user
    // PHASE form only
    int groups;               // M / (16 * HW)
    unsigned rcp_w2;          // 65536 / (W / 2) + 1: q / (W / 2) == (q * rcp_w2) >> 16 for q < 9362
    // IDX builds only: natural row m of the launch reads row x_idx[m] of x; [groups * 16 * HW] entries
    const int *x_idx;
    // OIDX builds only: natural row m of the launch is stored to row y_idx[m] of y, and not at all where that entry
    // is outside [0, y_rows); [groups * 16 * HW] entries
    const int *y_idx;
    unsigned y_rows;
};

// PHASE form: 16-row block `gb` of a group ([phase][qy][qx], HW blocks) -> its position in the phase's grid, and the natural row
// (y * W + x) of the block's pixel inside an image.  Uniform arithmetic, no division.
struct PhaseBlk {
    int qy, qx, row;
};
__device__ __forceinline__ PhaseBlk phase_blk(const PanelK &p, int gb) {
    const int W2 = p.W >> 1, Q = p.HW >> 2;
    const int ph = (gb >= Q ? 1 : 0) + (gb >= 2 * Q ? 1 : 0) + (gb >= 3 * Q ? 1 : 0);
    const int q = gb - ph * Q;
    const int qy = (int)(((unsigned)q * p.rcp_w2) >> 16), qx = q - qy * W2;
    return {qy, qx, (2 * qy + (ph >> 1)) * p.W + 2 * qx + (ph & 1)};
}

constexpr int P_NW = 6;                     // weight ring slots
constexpr int P_WSLOT = 256 * 64;           // 16 KiB: 256 output channels x 64 B (the tall phase form's slot is 128 channels, 8 KiB)

// The counted vmcnt of a step.  A step's POST issues, in this order, one panel piece of the next stage (taps < PP, not in the last
// stage) and NWP weight pieces (2 per wave with 256-column tiles, 1 with 128) for step t + P_NW.  The wait at the end of step t's
// PRE leaves outstanding exactly what was issued after the weights of step t + 1, i.e. by the POSTs of steps t-4 .. t-1 (the
// "window" of P_NW - 2 steps): NWP * (P_NW - 2) weight pieces plus the panel pieces of those steps.
// panel pieces issued in the window before tap J (taps of the previous stage when negative)
template <int J, int PP>
constexpr int panel_in_window() {
    int c = 0;
    for (int d = 1; d <= P_NW - 2; ++d) {
        int t = ((J - d) % 9 + 9) % 9;
        if (t < PP) ++c;
    }
    return c;
}
// Not the last stage.  FIRST: step 0 of the tile, whose window is the prologue's weight pieces alone (the prologue issues its
// panel pieces AHEAD of its weights; only tap 0 can see a panel piece of a previous stage in its window, and only with PP > 5:
// the window of tap J >= 1 reaches back to tap 5 + J).  Tap 8 hands over to the next stage's panel, so its wait must also cover
// the last panel piece (tap PP - 1): behind it come only the weight pieces of taps PP-1 .. 7, NWP * (9 - PP).  With PP <= 4 that
// is more than the window holds and changes nothing (PP = 4, NWP = 2: 10 against 8); with PP = 6, NWP = 1 it is 3 against 4 + 2.
template <int J, int PP, int NWP, bool FIRST>
constexpr int pieces_in_window() {
    static_assert(PP <= 6, "a panel piece of the previous stage in the window of a tap other than 0");
    if (FIRST) return NWP * (P_NW - 2);
    const int c = NWP * (P_NW - 2) + panel_in_window<J, PP>();
    const int after_panel = NWP * (9 - PP);
    return J == 8 && after_panel < c ? after_panel : c;
}
// The LAST channel stage: its taps >= 3 issue no weights and none of its taps a panel piece; the taps of the stage before it
// (negative t) issue their weights and, below PP, their panel piece (PP = 6: tap 5 is in the window of tap 0)
template <int J, int PP, int NWP>
constexpr int last_in_window() {
    int c = 0;
    for (int d = 1; d <= P_NW - 2; ++d) {
        int t = J - d;                     // < 0: previous stage, always issues
        if (t < 0 || t + P_NW < 9) c += NWP;
        if (t < 0 && 9 + t < PP) ++c;
    }
    return c;
}

template <int N>
__device__ __forceinline__ void vm_wait() {
    static_assert(N >= 0 && N <= 15, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// REUSE (the 512 x 128 phase form): the fragment window of one tap row dy.  In the phase form tap (dy, dx) of row tile mi
// reads panel tile b + mi + dy * W/2 + dx (b: the wave's first row tile in the panel; the shift is whole 16-row tiles, which the
// swizzle key (row >> 2) & 3 does not see), so (mi, dx) and (mi - 1, dx + 1) are the same tile at the same lane address.  The three
// taps of a dy share a window of 10 fragments: slot s holds tile b + dy * W/2 + s - 1.  Tap dx = -1 reads slots 0..7 as a step always
// did (0..2 in the POST of the step before), taps dx = 0 / +1 read the one slot they are first to use (8 / 9) and take the rest from
// registers: 10 ds_read_b128 per dy where there were 24.
constexpr int P_WIN = 10;
constexpr int reuse_slot(int dx, int mi) { return mi + dx + 1; }                      // the slot tap dx (-1, 0, 1) of row tile mi works from
constexpr int reuse_tile(int dy, int slot, int w2) { return dy * w2 + slot - 1; }     // the panel tile a slot holds, relative to b
constexpr int reuse_read_dx(int slot) { return slot < 8 ? -1 : slot - 8; }            // the tap that reads the slot from LDS
constexpr bool reuse_window_ok() {
    for (int w2 = 1; w2 <= 7; ++w2)                                                    // W / 2 of every phase launch (W even, <= 14)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
                for (int mi = 0; mi < 8; ++mi) {
                    const int s = reuse_slot(dx, mi);
                    if (s < 0 || s >= P_WIN) return false;
                    if (reuse_tile(dy, s, w2) != mi + dy * w2 + dx) return false;      // == the tile x_addr_of(tap) + mi * 1024 addresses
                    if (reuse_read_dx(s) > dx) return false;                           // read by this tap or an earlier one of the dy
                    if (reuse_tile(dy, s, w2) < -8 || reuse_tile(dy, s, w2) > 15) return false;   // the halo: 8 tiles either side
                }
    return true;
}
static_assert(reuse_window_ok(), "REUSE: (tap, row tile) -> window slot -> panel tile, W / 2 = 1 .. 7, inside tiles b - 8 .. b + 15");

// DBG: diagnostic builds: 1 = no tap-validity masking (VK_CONV256_DBG=1; timing only, WRONG results); 4 = stamps around the K loop
// and the whole workgroup (VK_PANEL_STAMPS=<file>, tools/panel_stamps.py)
// TAG 1: second symbol for launches of the two-stream backbone section (see conv_mfma_duo.hip)
// MI: 16-pixel row tiles per wave: 8 (256-pixel tiles) or 9 (288-pixel tiles, halo 48 / 112).  Rows are independent, so the tile
// height does not change a bit of the output; it changes how many rounds a grid takes (res4 at 32 x 800 x 1333: 525 tiles of 256
// = 2.05 rounds on 256 CUs, paid as 3; 467 tiles of 288 = 1.82 rounds, paid as 2 x 9/8), and a step carries 36 instead of 32
// MFMAs per wave over the same barrier, weight reads and DMA.  The launcher picks per launch.
// PHASE: 0 = rows in their natural order; 2 = the phase-interleaved internal row order with a scalar branch around the MFMAs of
// each (row tile, tap); 1 = the same order with the MFMAs of invalid taps still issued on zeroed fragments (tools build: the
// addressing alone)
// WR: the wave grid: WR row blocks of MI*16 rows x 8 / WR column blocks of 64 channels.  2 = 256 x 256 tiles (288 x 256 at MI = 9);
// 4 = 512 x 128 tiles (the phase form only): the same 128 x 64 per wave and the same step, but a weight slot of 128
// channels (8 KiB, one DMA piece per wave and step) serves 512 rows, and the panel is 6 pieces (768 rows, halo 128): 72 + 48 KiB
// through the CU per stage and 65 536 outputs instead of 144 + 32.  Rows are independent and every element sums the same products
// in the same order, so the tile shape does not change a bit.
// REUSE: 1 = the A-fragment window above (512 x 128 phase tiles only): 66 instead of 108 ds_read_b128 per wave and stage, the same
// MFMAs on the same operands in the same order.  0 (VK_PANEL_REUSE=0) = every tap reads its eight fragments.
// IDX: 1 = INDEXED INPUT ROWS (the 512 x 128 REUSE phase form only): output and internal row m reads row x_idx[m] of x,
// which is then [*, Cin] and not [M, Cin] (Res5 block 0: conv1's rows exist once per distinct RoIPool window).  y, res, the validity
// words and the epilogue go by m.  req_panel is the only place the input is addressed: a lane's six source offsets of a tile are
// x_idx[its natural row] * cin_bytes, six registers loaded once per tile, where the dense form adds a uniform block offset to ps_lane.
// The K loop, its vmcnt / lgkmcnt tables, the fragment window and the MFMAs are those of IDX = 0.
// OIDX: 1 = INDEXED OUTPUT ROWS (the same form only, with or without IDX): the epilogue stores natural row m to row
// y_idx[m] of y, which is then [y_rows, ldy], and drops the store where y_idx[m] is outside [0, y_rows) (Res5 block 0: conv2 writes
// the representative row of each nine-window neighbourhood and no other).  No residual.  A lane's eight indices, one per row tile,
// are requested behind the K loop's LAST counted wait (the vmcnt(0) of the final stage's tap 7: no later step issues or waits for
// anything), so they travel under the last 44 MFMAs of the wave and no table of the loop sees them.
template <int PP, int DBG, int TAG = 0, int MI = 8, int PHASE = 0, int WR = 2, int REUSE = 0, int IDX = 0, int OIDX = 0>
__global__ __launch_bounds__(512, 2) void conv3x3_panel_kernel(PanelK p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(MI == 8 || MI == 9, "8 or 9 row tiles per wave");
    static_assert(WR == 2 || WR == 4, "2 x 4 or 4 x 2 waves");
    static_assert(!PHASE || (PP == (WR == 4 ? 6 : 4) && MI == 8 && !(DBG & 9)), "the phase form: halo 128 = (W / 2 + 1) * 16 at W = 14, 256- or 512-row tiles");
    static_assert(WR == 2 || PHASE == 2, "512 x 128 tiles: the phase form only (a plain res4 launch would read its panel twice)");
    static_assert(MI == 8 || !(DBG & 8), "the LDS-staged epilogue is written for 128-row halves");
    static_assert(!REUSE || (PHASE == 2 && WR == 4 && MI == 8 && DBG == 0), "the fragment window: tap shifts of whole 16-row tiles, 512 x 128 tiles");
    static_assert(!IDX || (PHASE == 2 && WR == 4 && REUSE == 1 && DBG == 0 && PP == 6), "indexed input rows: the 512 x 128 REUSE phase form only");
    static_assert(!OIDX || (PHASE == 2 && WR == 4 && REUSE == 1 && DBG == 0 && PP == 6), "indexed output rows: the 512 x 128 REUSE phase form only");
    constexpr int WC = 8 / WR;                    // column blocks of 64 channels
    constexpr int CT = 64 * WC;                   // channels per tile: 256 or 128
    constexpr int NWP = CT / 128;                 // weight DMA pieces (16 rows) per wave and step: 2 or 1
    constexpr int WSLOT = CT * 64;                // a weight slot: 16 or 8 KiB
    constexpr int TILE = WR * MI * 16;            // pixels per tile
    constexpr int PROWS = PP * 128;               // panel rows
    constexpr int HALO = (PROWS - TILE) / 2;      // 64 or 128 (MI = 9: 48 or 112)
    constexpr int PBYTES = PROWS * 64;
    constexpr int WBASE = 2 * PBYTES;
    // a wave's first row tile is panel tile b = HALO / 16 + wr * MI: the window's tiles b - 8 .. b + 15 are panel tiles 0 .. PROWS / 16 - 1
    static_assert(!REUSE || (HALO / 16 == 8 && HALO / 16 + (WR - 1) * MI + 15 < PROWS / 16), "REUSE: the halo (8 tiles) covers tiles b - 8 .. b + 15");
    static_assert(HALO >= (PHASE ? 128 : 48) && WBASE + P_NW * WSLOT + (PP == 3 || WR == 4 ? 256 : 0) <= 160 * 1024, "halo / LDS");
    // PP = 3 leaves 16 KiB of the CU's LDS unused: 64 bytes of zeros behind the weight ring.  A fragment read of a pixel whose tap
    // falls outside the image is pointed there (two VALU instructions per read: a sign-extended bit-field and a bit-select
    // of the address) instead of zeroing the fragment afterwards (four v_cndmask per read and a compare): round 3, see DESIGN.md 6b.
    constexpr bool ZROW = PP == 3;
    constexpr int ZOFF = WBASE + P_NW * WSLOT;

    int bid = blockIdx.x;
    const int nwg = p.m_tiles * p.n_tiles;        // tiles (== gridDim.x unless the launch has a dynamic tail)
    unsigned long st_k0 = 0;
    if constexpr (DBG & 4) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_k0)::"memory");
    if constexpr (PP == 3 || PHASE) {
        if (p.tile_ctr && bid >= p.static_tiles) {               // (uniform) one atomic per workgroup, through the spare LDS behind the zero row
            // (PHASE with 256 x 256 tiles: PP = 4 has no spare LDS; the word is the panel's first, and a second barrier keeps the
            // prologue's DMA off it.  512 x 128 tiles leave 16 KiB: the word lies behind the weight ring, as with PP = 3)
            constexpr bool MAIL_IN_PANEL = PHASE && WR == 2;
            int *mail = reinterpret_cast<int *>(smem + (MAIL_IN_PANEL ? 0 : ZOFF + 128));
            if (threadIdx.x == 0) {
                const unsigned v = atomicAdd(p.tile_ctr, 1u);
                if (v == p.ctr_last) *p.tile_ctr = 0u;
                *mail = p.static_tiles + (int)v;
            }
            __syncthreads();
            bid = __builtin_amdgcn_readfirstlane(*mail);
            if constexpr (MAIL_IN_PANEL) __syncthreads();
            if (bid >= nwg) return;
        }
    }
    const int t_ = xcd_tile(bid, nwg);
    // (the n_tiles column tiles of one panel, 2 or 4, are consecutive t_: consecutive workgroups of one XCD, whose L2 holds the panel)
    const int n_tile = t_ % p.n_tiles, m_tile = t_ / p.n_tiles;
    const int m0 = m_tile * TILE, n0 = n_tile * CT;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave & (WC - 1);
    const int g = lane >> 4, j = lane & 15;

    unsigned vm0 = 0, vm1 = 0, vm2 = 0;           // per-lane tap validity, taps 0-2 | 3-5 | 6-8: filled behind the prologue's requests

    // ---- LDS-DMA source state ----
    const int lrow = lane >> 2;
    const int lchunk = (lane & 3) ^ ((-(lrow >> 2)) & 3);
    const int pm_first = m0 - HALO + wave * 16 + lrow;        // pixel of panel row (piece q): + q*128
    // 32-bit byte offsets from the (uniform) tensor bases: the launcher checks both tensors are < 4 GiB
    const unsigned wsrc0 = (unsigned)(n0 + wave * (16 * NWP) + lrow) * (unsigned)p.wrow_bytes + lchunk * 16;   // piece i: + i*16 rows
    const unsigned wstep = 16u * p.wrow_bytes;
    // PHASE: block m0 / 16 + off of the internal order -> its group (return value: the block inside the group), clamped into the tensor
    int g0 = 0, gb0 = 0;
    if constexpr (PHASE) {
        g0 = (m0 >> 4) / p.HW;
        gb0 = (m0 >> 4) - g0 * p.HW;
    }
    auto blk_of = [&](int off, int &G) -> int {
        int t = gb0 + off;
        G = g0;
        while (t < 0) {
            t += p.HW;
            --G;
        }
        while (t >= p.HW) {
            t -= p.HW;
            ++G;
        }
        if (G < 0) G = 0, t = 0;
        if (G >= p.groups) G = p.groups - 1, t = p.HW - 1;
        return t;
    };
    // PHASE: a wave's 16 rows of a panel piece are one block: image lrow of the group (per lane) at one pixel (uniform).  The PP
    // source offsets are found once per tile; rows outside the tensor are clamped to a real block as below.
    [[maybe_unused]] unsigned ps_lane = 0, ps_blk[PP] = {};
    // IDX: the index of the lane's row of each piece, requested HERE, ahead of everything else the tile asks of memory: one
    // global_load_dword per piece at natural row (G * 16 + lrow) * HW + the block's pixel.  blk_of clamps every halo block into
    // [0, groups * 16 * HW), so x_idx is never read out of range (a clamped halo row is only read by taps the validity words drop).
    // The prologue turns the six indices into byte offsets once they have landed.
    [[maybe_unused]] unsigned ps_idx[PP] = {};
    if constexpr (IDX) {
#pragma unroll
        for (int q2 = 0; q2 < PP; ++q2) {
            int G;
            const int t = blk_of(wave - HALO / 16 + q2 * 8, G);
            const int *ip = p.x_idx + ((long)(G * 16 + lrow) * p.HW + phase_blk(p, t).row);
            asm volatile("global_load_dword %0, %1, off" : "=v"(ps_idx[q2]) : "v"(ip));
        }
    } else if constexpr (PHASE) {
        ps_lane = (unsigned)(lrow * p.HW) * (unsigned)p.cin_bytes + lchunk * 16;
#pragma unroll
        for (int q2 = 0; q2 < PP; ++q2) {
            int G;
            const int t = blk_of(wave - HALO / 16 + q2 * 8, G);
            ps_blk[q2] = __builtin_amdgcn_readfirstlane((unsigned)(G * 16 * p.HW + phase_blk(p, t).row) * (unsigned)p.cin_bytes);
        }
    }
    auto req_panel = [&](int cs, int piece) {                 // rows (piece*8 + wave)*16 .. +15 of panel(cs)
        if constexpr (IDX) {
            unsigned pl = ps_idx[piece];
            asm volatile("" : "+v"(pl));                       // opaque (see x_addr_of)
            glds16(p.x + (pl + cs * 64), smem + (cs & 1) * PBYTES + (piece * 8 + wave) * 1024);
            return;
        }
        if constexpr (PHASE) {
            unsigned pl = ps_lane;
            asm volatile("" : "+v"(pl));                       // opaque (see x_addr_of)
            glds16(p.x + (pl + (ps_blk[piece] + cs * 64)), smem + (cs & 1) * PBYTES + (piece * 8 + wave) * 1024);
            return;
        }
        int pf = pm_first;
        asm volatile("" : "+v"(pf));                           // opaque (see x_addr_of)
        // rows outside [0, M) are only ever read by taps the validity mask zeroes: any finite-or-not data
        // will do there, so clamp to a real row instead of branching to a zero page
        const int m = min(max(pf + piece * 128, 0), p.M - 1);
        const unsigned off = (unsigned)m * (unsigned)p.cin_bytes + cs * 64 + lchunk * 16;
        glds16(p.x + off, smem + (cs & 1) * PBYTES + (piece * 8 + wave) * 1024);
    };
    auto req_w = [&](int slot, int cs, int tap, int i) {      // rows (wave*NWP+i)*16 .. +15 of weight slot `slot`
        const unsigned koff = (unsigned)(tap * p.cstages + cs) * 64;  // K layout = (tap, channel): tap*Cin*2 + cs*64 bytes
        unsigned wb_ = wsrc0;
        asm volatile("" : "+v"(wb_));                          // opaque (see x_addr_of)
        glds16(p.w + (wb_ + i * wstep + koff), smem + WBASE + slot * WSLOT + (wave * NWP + i) * 1024);
    };

    // ---- fragment addressing ----
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) char *)smem;
    [[maybe_unused]] const unsigned zrow = lds0 + ZOFF;
    if constexpr (ZROW) {                         // (complete before the prologue's barrier, ahead of the first fragment read)
        if (tid < 16) *reinterpret_cast<unsigned *>(smem + ZOFF + tid * 4) = 0u;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    unsigned w_a[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int wrow = wc * 64 + (j >> 2) * 8 + par * 4 + (j & 3);
        w_a[par] = lds0 + WBASE + wrow * 64 + ((g ^ ((-(wrow >> 2)) & 3)) << 4);
    }
    const int jbase = HALO + wr * (MI * 16) + j;              // panel row of fragment pixel mi = 0 at zero shift
    auto x_addr_of = [&](int parity, int tap) -> unsigned {   // byte address of fragment row mi = 0 (panel `parity`, tap)
        const int shift = PHASE ? ((tap / 3 - 1) * (p.W >> 1) + (tap % 3 - 1)) * 16 : ((tap / 3 - 1) * p.W + (tap % 3 - 1)) * p.dil;
        int jb = jbase;
        asm volatile("" : "+v"(jb));                           // opaque: the 18 (panel, tap) addresses must not be hoisted
        const int rb = jb + shift;                             // >= 0: HALO >= dil*(W+1)
        return lds0 + parity * PBYTES + (rb << 6) + ((g ^ ((-(rb >> 2)) & 3)) << 4);
    };

    floatx4 acc[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};
    half8 wa[4], wb[4], xw[REUSE ? P_WIN : (MI == 9 ? 5 : 4)];      // (MI = 9: row tile 8 has a fragment register of its own; REUSE: the window of a dy)
    const int CS = p.cstages;

#define VKP_DSR(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(dst) : "v"(addr))
    // fragment read of row tile MI_ of tap J_ (TW: the lane's validity word of taps 3*(J_/3)..+2, unshifted).  Written as asm: left to
    // hipcc the select becomes and + compare + s_nop + cndmask.
#define VKP_DSRX(dst, addr, OFF, TW, J_, MI_)                                                        \
    do {                                                                                             \
        if constexpr (ZROW && !(DBG & 1)) {                                                          \
            unsigned m_, ad_;                                                                        \
            const unsigned zc_ = zrow - (OFF);                                                       \
            asm volatile("v_bfe_i32 %0, %1, %2, 1" : "=v"(m_) : "v"(TW), "n"(((J_) % 3) * 9 + (MI_))); \
            asm volatile("v_bfi_b32 %0, %1, %2, %3" : "=v"(ad_) : "v"(m_), "v"(addr), "s"(zc_));    \
            VKP_DSR(dst, ad_, OFF);                                                                  \
        } else                                                                                       \
            VKP_DSR(dst, addr, OFF);                                                                 \
    } while (0)
#define VKP_WAIT3(reg) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(reg))
#define VKP_WAIT4(reg) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(reg))
#define VKP_SB() __builtin_amdgcn_sched_barrier(0)
    // zero a fragment whose pixel is outside the image for this tap (4 v_cndmask), then 4 MFMAs
#define VKP_MMA_ROW(MI, XR, WF, TM)                                                                  \
    do {                                                                                             \
        if constexpr (PHASE == 2) {                                                                  \
            if (((TM) >> (MI)) & 1u) { /* uniform: s_bitcmp1 + s_cbranch */                          \
                __builtin_amdgcn_s_setprio(1);                                                       \
                _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) acc[MI][ni] =                       \
                    __builtin_amdgcn_mfma_f32_16x16x32_f16(WF[ni], XR, acc[MI][ni], 0, 0, 0);        \
                __builtin_amdgcn_s_setprio(0);                                                       \
            }                                                                                        \
            break;                                                                                   \
        }                                                                                            \
        if constexpr (!(DBG & 1) && !ZROW) {                                                         \
            u32x4 u_ = __builtin_bit_cast(u32x4, XR);                                              \
            const bool v_ = ((TM) >> (MI)) & 1u;                                                     \
            u_[0] = v_ ? u_[0] : 0u;                                                                 \
            u_[1] = v_ ? u_[1] : 0u;                                                                 \
            u_[2] = v_ ? u_[2] : 0u;                                                                 \
            u_[3] = v_ ? u_[3] : 0u;                                                                 \
            XR = __builtin_bit_cast(half8, u_);                                                      \
        }                                                                                            \
        __builtin_amdgcn_s_setprio(1);                                                               \
        _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) acc[MI][ni] =                               \
            __builtin_amdgcn_mfma_f32_16x16x32_f16(WF[ni], XR, acc[MI][ni], 0, 0, 0);                \
        __builtin_amdgcn_s_setprio(0);                                                               \
    } while (0)
    // (the slot addresses are recomputed in the loop from opaque copies: hipcc would otherwise keep all
    //  2 x 6 slot addresses in registers)
#define VKP_READ_W(WF, so)                              \
    do {                                                \
        unsigned a0_ = w_a[0], a1_ = w_a[1];            \
        asm volatile("" : "+v"(a0_), "+v"(a1_));        \
        a0_ += so;                                      \
        a1_ += so;                                      \
        VKP_DSR(WF[0], a0_, 0);                         \
        VKP_DSR(WF[1], a1_, 0);                         \
        VKP_DSR(WF[2], a0_, 2048);                      \
        VKP_DSR(WF[3], a1_, 2048);                      \
    } while (0)

    // One step = tap J of channel stage cs (global step t = 9*cs + J).  LAST: cs is the final stage
    // (no panel prefetch, weight requests stop when t + 6 >= 9*CS, no step after tap 8).
    // ODD = parity of cs (stages run in pairs, so it is known at compile time): panel buffer = ODD, and the
    // weight slot of step t = 9*cs + J is (3*ODD + J) % 6.
    // A step is cut at its barrier into PRE (rows 0-4, then every LDS read of the step is complete) and POST (rows
    // 5-7 together with the first fragment reads of the next step); the loop iterates POST(t-1) + PRE(t), so NO
    // hand-issued ds_read is in flight at a loop boundary, where hipcc may copy fragment registers
    // (tools/check_asm_hazards.py; see conv_mfma256.hip).
    auto tap_mask = [&](auto j_c) -> unsigned {
        constexpr int J = decltype(j_c)::value;
        // opaque copy of the mask word BEFORE the shift: otherwise hipcc hoists either the 72 (tap, row-tile)
        // lane masks (SGPR pairs) or the 9 shifted words out of the loop and spills them
        unsigned tw = J < 3 ? vm0 : (J < 6 ? vm1 : vm2);
        if constexpr (PHASE)
            asm volatile("" : "+s"(tw));                       // (the phase form's words are per wave)
        else
            asm volatile("" : "+v"(tw));
        return tw >> ((J % 3) * 9);
    };
    auto tap_word = [&](auto j_c) -> unsigned {       // the unshifted word (VKP_DSRX extracts its bit itself)
        constexpr int J = decltype(j_c)::value;
        unsigned tw = J < 3 ? vm0 : (J < 6 ? vm1 : vm2);
        asm volatile("" : "+v"(tw));
        return tw;
    };
    auto pre = [&](auto last_c, auto odd_c, auto j_c, unsigned xa, unsigned &xa_next, const half8 (&wcur)[4], auto first_c) {
        constexpr bool LAST = decltype(last_c)::value, FIRST = decltype(first_c)::value;      // FIRST: step 0 of the tile
        constexpr int ODD = decltype(odd_c)::value;
        constexpr int J = decltype(j_c)::value;
        const unsigned tm = ZROW ? 0u : tap_mask(j_c);
        [[maybe_unused]] const unsigned tw = ZROW ? tap_word(j_c) : 0u;
        constexpr bool has_next = !(LAST && J == 8);
        if constexpr (REUSE) {
            // xa addresses slot 0 of the window (tap dx = -1 of this dy) for all three taps; slot s is at + s * 1024
            constexpr int D = J % 3;
            if constexpr (has_next && D == 2)
                xa_next = (J == 8) ? x_addr_of(1 - ODD, 0) : x_addr_of(ODD, J + 1);
            else
                xa_next = xa;
#define VKP_ROWX(MI_) VKP_SB(); VKP_MMA_ROW(MI_, xw[reuse_slot(D - 1, MI_)], wcur, tm); VKP_SB()
            if constexpr (D == 0) {        // in flight: 4 weight fragments, slots 0 1 2 (POST of the step before / prologue)
                static_assert(reuse_slot(-1, 4) == 4 && reuse_read_dx(7) == -1);
                VKP_DSR(xw[3], xa, 3072); VKP_WAIT3(xw[0]); VKP_ROWX(0);
                VKP_DSR(xw[4], xa, 4096); VKP_WAIT3(xw[1]); VKP_ROWX(1);
                VKP_DSR(xw[5], xa, 5120); VKP_WAIT3(xw[2]); VKP_ROWX(2);
                VKP_DSR(xw[6], xa, 6144); VKP_WAIT3(xw[3]); VKP_ROWX(3);
                VKP_DSR(xw[7], xa, 7168); VKP_WAIT3(xw[4]); VKP_ROWX(4);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xw[5]), "+v"(xw[6]), "+v"(xw[7])::"memory");
            } else {                       // in flight: the 4 weight fragments alone; the one new slot is first used by row tile 7 (POST)
                static_assert(reuse_read_dx(7 + D) == D - 1 && reuse_slot(D - 1, 7) == 7 + D);
                half8(&wm)[4] = (9 * ODD + J) % 2 == 0 ? wa : wb;           // == wcur, writable: the wait is tied to the fragments it covers
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wm[0]), "+v"(wm[1]), "+v"(wm[2]), "+v"(wm[3]));
                if constexpr (D == 1)
                    VKP_DSR(xw[8], xa, 8192);
                else
                    VKP_DSR(xw[9], xa, 9216);
                VKP_ROWX(0); VKP_ROWX(1); VKP_ROWX(2); VKP_ROWX(3); VKP_ROWX(4);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xw[7 + D])::"memory");
            }
#undef VKP_ROWX
        } else {                           // every tap reads its eight fragments through a window of four
            // address of the next step's fragments (next tap; next stage's panel after tap 8)
            if constexpr (has_next) xa_next = (J == 8) ? x_addr_of(1 - ODD, 0) : x_addr_of(ODD, J + 1);
            VKP_DSRX(xw[3], xa, 3072, tw, J, 3); VKP_WAIT3(xw[0]); VKP_SB(); VKP_MMA_ROW(0, xw[0], wcur, tm); VKP_SB();
            VKP_DSRX(xw[0], xa, 4096, tw, J, 4); VKP_WAIT3(xw[1]); VKP_SB(); VKP_MMA_ROW(1, xw[1], wcur, tm); VKP_SB();
            VKP_DSRX(xw[1], xa, 5120, tw, J, 5); VKP_WAIT3(xw[2]); VKP_SB(); VKP_MMA_ROW(2, xw[2], wcur, tm); VKP_SB();
            VKP_DSRX(xw[2], xa, 6144, tw, J, 6); VKP_WAIT3(xw[3]); VKP_SB(); VKP_MMA_ROW(3, xw[3], wcur, tm); VKP_SB();
            if constexpr (MI == 9) {
                VKP_DSRX(xw[3], xa, 7168, tw, J, 7); VKP_DSRX(xw[4], xa, 8192, tw, J, 8); VKP_WAIT4(xw[0]); VKP_SB(); VKP_MMA_ROW(4, xw[0], wcur, tm); VKP_SB();
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xw[1]), "+v"(xw[2]), "+v"(xw[3]), "+v"(xw[MI == 9 ? 4 : 3])::"memory");
            } else {
                VKP_DSRX(xw[3], xa, 7168, tw, J, 7); VKP_WAIT3(xw[0]); VKP_SB(); VKP_MMA_ROW(4, xw[0], wcur, tm); VKP_SB();
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xw[1]), "+v"(xw[2]), "+v"(xw[3])::"memory");
            }
        }
        VKP_SB();
        if constexpr (has_next) {
            // vmcnt: everything older than the pieces issued in the last P_NW-2 steps has landed = weights of step
            // t+1 (and, before tap 0, the next stage's panel); barrier: weight slot (t % 6) is free for step t+6,
            // the other panel buffer is free once the stage ends.  The counts (pieces_in_window / last_in_window above), taps 0..8:
            //   256 x 256, PP = 4, NWP = 2: 8 9 10 11 12 11 10 9 8, first step 8; last stage 8 8 8 8 6 4 2 0
            //   512 x 128, PP = 6, NWP = 1: 5 5 6 7 8 8 8 7 3 (tap 8: the panel piece of tap 5 must have landed), first step 4;
            //                               last stage 5 4 4 4 3 2 1 0
            constexpr int OUT = LAST ? last_in_window<J, PP, NWP>() : pieces_in_window<J, PP, NWP, FIRST>();
            vm_wait<OUT>();
            // (DBG 16 / 32, timing only, WRONG results: the barrier on every third tap only / never -- what the per-step barrier costs)
            if constexpr (!(DBG & 48) || ((DBG & 16) && J % 3 == 2)) asm volatile("s_barrier" ::: "memory");
        }
        VKP_SB();
    };
    auto post = [&](auto last_c, auto odd_c, auto j_c, int cs, unsigned xa_next, const half8 (&wcur)[4], half8 (&wnext)[4]) {
        constexpr bool LAST = decltype(last_c)::value;
        constexpr int ODD = decltype(odd_c)::value;
        constexpr int J = decltype(j_c)::value;
        static_assert(!(LAST && J == 8), "the final step has no POST");
        constexpr int SLOT = (3 * ODD + J) % P_NW;            // == t % 6; also the slot of step t + 6
        const unsigned tm = ZROW ? 0u : tap_mask(j_c);
        constexpr int JN = (J + 1) % 9;                   // the next step's tap (tap 0 of the next stage after tap 8)
        [[maybe_unused]] const unsigned twn = ZROW ? tap_word(std::integral_constant<int, JN>{}) : 0u;
        constexpr bool issue_w = !LAST || (J + P_NW < 9);
        constexpr bool issue_p = !LAST && (J < PP);
        constexpr unsigned so = (unsigned)((SLOT + 1) % P_NW) * WSLOT;
        // REUSE: row tiles 5 6 7 of tap dx work from slots 6 + dx .. 8 + dx; only the last tap of a dy reads ahead (slots 0 1 2 of the
        // next dy: their last users were row tile 0 of this dy's three taps, issued before this step's barrier)
        constexpr int D = J % 3;
        constexpr bool ahead = !REUSE || D == 2;
        constexpr int X5 = REUSE ? reuse_slot(D - 1, 5) : 1, X6 = REUSE ? reuse_slot(D - 1, 6) : 2, X7 = REUSE ? reuse_slot(D - 1, 7) : 3;
        VKP_READ_W(wnext, so);
        if constexpr (ahead) VKP_DSRX(xw[0], xa_next, 0, twn, JN, 0);
        VKP_SB();
        VKP_MMA_ROW(5, xw[X5], wcur, tm);
        VKP_SB();
        if constexpr (issue_p) req_panel(cs + 1, J);
        if constexpr (issue_w) req_w(SLOT, cs + (J + P_NW) / 9, (J + P_NW) % 9, 0);
        if constexpr (ahead) VKP_DSRX(xw[1], xa_next, 1024, twn, JN, 1);
        VKP_SB();
        VKP_MMA_ROW(6, xw[X6], wcur, tm);
        VKP_SB();
        if constexpr (issue_w && NWP == 2) req_w(SLOT, cs + (J + P_NW) / 9, (J + P_NW) % 9, 1);
        if constexpr (ahead) VKP_DSRX(xw[2], xa_next, 2048, twn, JN, 2);
        VKP_SB();
        VKP_MMA_ROW(7, xw[X7], wcur, tm);
        VKP_SB();
        if constexpr (MI == 9) {
            VKP_MMA_ROW(8, xw[MI == 9 ? 4 : 3], wcur, tm);
            VKP_SB();
        }
    };
    // u = 9*ODD + J numbers the 18 steps of a pair of stages; step u works from fragment set u % 2
    auto wset = [&](auto u_c) -> half8(&)[4] {
        if constexpr (decltype(u_c)::value % 2 == 0)
            return wa;
        else
            return wb;
    };
#define VKP_IC(V) std::integral_constant<int, (V)> {}
    // POST(u-1) + PRE(u) inside the pair that starts at stage cs; LP / LC: is step u-1 / u in the final stage
#define VKP_UNIT(LP, LC, U)                                                                                          \
    post(LP, VKP_IC(((U) - 1) / 9), VKP_IC(((U) - 1) % 9), cs + ((U) - 1) / 9, xan, wset(VKP_IC((U) - 1)), wset(VKP_IC(U)));  \
    xa = xan;                                                                                                        \
    pre(LC, VKP_IC((U) / 9), VKP_IC((U) % 9), xa, xan, wset(VKP_IC(U)), F_{});
    using T_ = std::integral_constant<bool, true>;
    using F_ = std::integral_constant<bool, false>;

    // ---- prologue: panel(0), weights of steps 0..5; panel(0) and weights(0) must have landed ----
    // (IDX: the panel pieces wait for their indices and go out behind the validity words, see below)
    if constexpr (!IDX) {
#pragma unroll
        for (int q2 = 0; q2 < PP; ++q2) req_panel(0, q2);
    }
#pragma unroll
    for (int st = 0; st < P_NW; ++st) {
        req_w(st, 0, st, 0);
        if constexpr (NWP == 2) req_w(st, 0, st, 1);
    }
    // ---- per-lane tap validity of its MI fragment pixels (rows wr*MI*16 + mi*16 + j): bit ((tap % 3) * 9 + mi) of word tap / 3 ----
    // Computed HERE, behind the prologue's requests, so that it runs under their HBM latency; and without per-pixel integer
    // division (round 3: the first form, two divisions and 81 tap tests per lane ahead of the requests, was ~1300 VALU
    // instructions per wave = 4.7 us of a 133 us workgroup on Res5 conv2).  The wave's first row is placed in its image by
    // two uniform divisions; a lane's row is at most MI*16 - 1 pixels further: column by a float reciprocal with an exact
    // +-1 correction (operands < 2^24), at most one image wrap when the image has >= MI*16 pixels.  Tap validity is separable:
    // three row tests, three column tests.  Images smaller than a wave's rows keep the division form.
    if constexpr (PHASE) {
        // one bit per (row tile, tap), the same for the wave's 64 lanes: row tile mi is grid position (qy, qx) of a phase in 16
        // images, tap (dy, dx) is inside the image iff 0 <= qy + dy < H / 2 and 0 <= qx + dx < W / 2
        unsigned u0 = 0, u1 = 0, u2 = 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            int G;
            const PhaseBlk b = phase_blk(p, blk_of(wr * MI + mi, G));
            const unsigned c0 = b.qx >= 1, c2 = b.qx + 1 < (p.W >> 1);
            const unsigned cw = m0 + (wr * MI + mi) * 16 < p.M ? (c0 << mi) | (1u << (9 + mi)) | (c2 << (18 + mi)) : 0u;
            u0 |= b.qy >= 1 ? cw : 0u;
            u1 |= cw;
            u2 |= b.qy + 1 < (p.H >> 1) ? cw : 0u;
        }
        vm0 = __builtin_amdgcn_readfirstlane(u0);
        vm1 = __builtin_amdgcn_readfirstlane(u1);
        vm2 = __builtin_amdgcn_readfirstlane(u2);
    } else if (p.HW >= MI * 16 + p.W) {
        const int mbase = m0 + wr * (MI * 16);
        const int rem0 = mbase % p.HW, ho0 = rem0 / p.W, wo0 = rem0 - ho0 * p.W;
        const float rcpw = 1.0f / (float)p.W;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int xcol = wo0 + mi * 16 + j;
            int q = (int)((float)xcol * rcpw), wo = xcol - q * p.W;
            if (wo >= p.W) {
                wo -= p.W;
                ++q;
            }
            if (wo < 0) {
                wo += p.W;
                --q;
            }
            int ho = ho0 + q;
            if (ho >= p.H) ho -= p.H;
            const unsigned c0 = (unsigned)(wo - p.dil) < (unsigned)p.W, c1 = 1u, c2 = (unsigned)(wo + p.dil) < (unsigned)p.W;
            const unsigned cw = mbase + mi * 16 + j < p.M ? (c0 << mi) | (c1 << (9 + mi)) | (c2 << (18 + mi)) : 0u;
            vm0 |= (unsigned)(ho - p.dil) < (unsigned)p.H ? cw : 0u;
            vm1 |= cw;
            vm2 |= (unsigned)(ho + p.dil) < (unsigned)p.H ? cw : 0u;
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int m = m0 + wr * (MI * 16) + mi * 16 + j;
            if (m < p.M) {
                const int n_img = m / p.HW;
                const int rem = m - n_img * p.HW;
                const int ho = rem / p.W, wo = rem - ho * p.W;
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int hi = ho + (tap / 3 - 1) * p.dil, wi = wo + (tap % 3 - 1) * p.dil;
                    const unsigned ok = ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W) ? 1u : 0u;
                    if (tap < 3)
                        vm0 |= ok << (tap * 9 + mi);
                    else if (tap < 6)
                        vm1 |= ok << ((tap - 3) * 9 + mi);
                    else
                        vm2 |= ok << ((tap - 6) * 9 + mi);
                }
            }
        }
    }

    if constexpr (IDX) {
        // The index loads count in vmcnt like every vector-memory instruction, and loads retire in order: behind them only the
        // P_NW * NWP weight pieces have been issued, so vmcnt(P_NW * NWP) says all six indices are in their registers (the wait names
        // them, so nothing that reads them moves above it).  Offsets: x_idx[m] * cin_bytes < 2^32, the launcher checks x's rows.
        // Then the panel pieces, and vmcnt(0): the pieces are now the NEWEST requests, so no count short of zero covers them.
        // That keeps every table of the K loop as it is: a step's wait says "at most N requests outstanding, all issued inside the
        // window"; step 0 (FIRST) allows the prologue's NWP * (P_NW - 2) newest weight pieces and finds none outstanding, which
        // satisfies it, and every later window reaches back to POSTs of the K loop alone, whose issue order has not changed.
        static_assert(PP == 6 && P_NW * NWP <= 15);
        asm volatile("s_waitcnt vmcnt(%6)"
                     : "+v"(ps_idx[0]), "+v"(ps_idx[1]), "+v"(ps_idx[2]), "+v"(ps_idx[3]), "+v"(ps_idx[4]), "+v"(ps_idx[5])
                     : "n"(P_NW * NWP)
                     : "memory");
#pragma unroll
        for (int q2 = 0; q2 < PP; ++q2) ps_idx[q2] = ps_idx[q2] * (unsigned)p.cin_bytes + lchunk * 16;
#pragma unroll
        for (int q2 = 0; q2 < PP; ++q2) req_panel(0, q2);
        vm_wait<0>();
    } else {
        vm_wait<NWP * (P_NW - 1)>();              // all but the weights of steps 1..5: panel(0) and the weights of step 0 are in LDS
    }
    asm volatile("s_barrier" ::: "memory");
    unsigned long st_c0 = 0, st_r0 = 0;
    if constexpr (DBG & 4) asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_c0), "=s"(st_r0)::"memory");
    unsigned xa = x_addr_of(0, 0), xan = 0;
    VKP_READ_W(wa, 0u);
    {
        [[maybe_unused]] const unsigned tw0 = tap_word(VKP_IC(0));
        VKP_DSRX(xw[0], xa, 0, tw0, 0, 0);
        VKP_DSRX(xw[1], xa, 1024, tw0, 0, 1);
        VKP_DSRX(xw[2], xa, 2048, tw0, 0, 2);
    }
    pre(F_{}, VKP_IC(0), VKP_IC(0), xa, xan, wa, T_{});
    // CS is even: stages go in pairs (18 steps, so the roles of the two fragment sets repeat per pair)
    int cs = 0;
    for (; cs + 2 < CS; cs += 2) {
        VKP_UNIT(F_{}, F_{}, 1) VKP_UNIT(F_{}, F_{}, 2) VKP_UNIT(F_{}, F_{}, 3) VKP_UNIT(F_{}, F_{}, 4) VKP_UNIT(F_{}, F_{}, 5)
        VKP_UNIT(F_{}, F_{}, 6) VKP_UNIT(F_{}, F_{}, 7) VKP_UNIT(F_{}, F_{}, 8) VKP_UNIT(F_{}, F_{}, 9) VKP_UNIT(F_{}, F_{}, 10)
        VKP_UNIT(F_{}, F_{}, 11) VKP_UNIT(F_{}, F_{}, 12) VKP_UNIT(F_{}, F_{}, 13) VKP_UNIT(F_{}, F_{}, 14) VKP_UNIT(F_{}, F_{}, 15)
        VKP_UNIT(F_{}, F_{}, 16) VKP_UNIT(F_{}, F_{}, 17)
        // last step of this pair, first step of the next one
        post(F_{}, VKP_IC(1), VKP_IC(8), cs + 1, xan, wb, wa);
        xa = xan;
        pre(F_{}, VKP_IC(0), VKP_IC(0), xa, xan, wa, F_{});
    }
    // final pair: its second stage is the LAST one
    VKP_UNIT(F_{}, F_{}, 1) VKP_UNIT(F_{}, F_{}, 2) VKP_UNIT(F_{}, F_{}, 3) VKP_UNIT(F_{}, F_{}, 4) VKP_UNIT(F_{}, F_{}, 5)
    VKP_UNIT(F_{}, F_{}, 6) VKP_UNIT(F_{}, F_{}, 7) VKP_UNIT(F_{}, F_{}, 8) VKP_UNIT(F_{}, T_{}, 9) VKP_UNIT(T_{}, T_{}, 10)
    VKP_UNIT(T_{}, T_{}, 11) VKP_UNIT(T_{}, T_{}, 12) VKP_UNIT(T_{}, T_{}, 13) VKP_UNIT(T_{}, T_{}, 14) VKP_UNIT(T_{}, T_{}, 15)
    VKP_UNIT(T_{}, T_{}, 16)
    // OIDX: the output rows of the lane's eight row tiles.  Step 16 (tap 7 of the last stage) has just waited for vmcnt(0) and neither
    // its POST nor step 17 issues or waits for a vector-memory request (last_in_window<7> == 0, no weights from tap 3 on, no wait
    // behind tap 8), so these loads are alone in the queue until the epilogue's own wait.  min(mo, M - 1) as for the residual: blk_of
    // clamps every block into the tensor, so y_idx is never read out of range.
    [[maybe_unused]] int yrow[MI] = {};
    if constexpr (OIDX) {
        static_assert(last_in_window<7, PP, NWP>() == 0, "the index loads go out behind the loop's last counted wait");
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            int G;
            const int t = blk_of(wr * MI + mi, G);
            const long mo = (long)(G * 16 + j) * p.HW + phase_blk(p, t).row;
            const int *ip = p.y_idx + min(mo, (long)p.M - 1);
            asm volatile("global_load_dword %0, %1, off" : "=v"(yrow[mi]) : "v"(ip));
        }
    }
    VKP_UNIT(T_{}, T_{}, 17)
    {
        const unsigned tm = ZROW ? 0u : tap_mask(VKP_IC(8));
        VKP_MMA_ROW(5, xw[REUSE ? reuse_slot(1, 5) : 1], wb, tm);
        VKP_MMA_ROW(6, xw[REUSE ? reuse_slot(1, 6) : 2], wb, tm);
        VKP_MMA_ROW(7, xw[REUSE ? reuse_slot(1, 7) : 3], wb, tm);
        if constexpr (MI == 9) VKP_MMA_ROW(8, xw[MI == 9 ? 4 : 3], wb, tm);
    }
    unsigned long st_c1 = 0, st_r1 = 0;
    if constexpr (DBG & 4) asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_c1), "=s"(st_r1)::"memory");
#undef VKP_UNIT
#undef VKP_IC
#undef VKP_DSR
#undef VKP_DSRX
#undef VKP_WAIT3
#undef VKP_WAIT4
#undef VKP_MMA_ROW
#undef VKP_READ_W
#undef VKP_SB

    // ---- epilogue: + bias (+ residual)(ReLU) -> f16 ----
    // DIRECT (the default since round 2): straight from the accumulator layout -- a lane owns 8 consecutive channels of a pixel
    // (16-byte stores, 64 B per pixel row and instruction), specialised on residual / ReLU / ragged tile like conv_ws.hip; same
    // arithmetic, same bits.  DBG & 8: the first form, through LDS in two 128-row halves so that HBM sees whole 512-B rows
    // (two barriers more, 64 ds_write_b128 + 32 ds_read_b128 per thread and tile).
    if constexpr (!(DBG & 8)) {
        // (PHASE: the epilogue places its row tiles afresh: held from the prologue, their 16 scalars would be spilled across the K loop)
        if constexpr (PHASE) asm volatile("" : "+s"(g0), "+s"(gb0));
        if constexpr (OIDX) {                                  // the eight indices have landed (the wait names them: no reader moves above it)
            static_assert(MI == 8);
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(yrow[0]), "+v"(yrow[1]), "+v"(yrow[2]), "+v"(yrow[3]), "+v"(yrow[4]), "+v"(yrow[5]), "+v"(yrow[6]), "+v"(yrow[7])
                         :
                         : "memory");
        }
        auto epilogue = [&](auto res_c, auto relu_c, auto full_c) {
            constexpr bool RES = decltype(res_c)::value, RELU = decltype(relu_c)::value, FULL = decltype(full_c)::value;
            // row tile outer, channel half inner: the two 64-byte halves of a pixel's 128-byte line (this wave's 64 channels) leave in
            // consecutive instructions (round 3; they used to be nine stores apart)
            const int ch0 = n0 + wc * 64 + g * 8;
            floatx4 bq[2][2];
#pragma unroll
            for (int qn = 0; qn < 2; ++qn) {
                bq[qn][0] = *reinterpret_cast<const floatx4 *>(p.bias + ch0 + qn * 32);
                bq[qn][1] = *reinterpret_cast<const floatx4 *>(p.bias + ch0 + qn * 32 + 4);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const long m = m0 + wr * (MI * 16) + mi * 16 + j;
                long mo = m;                                   // the row of y and of the residual
                if constexpr (PHASE) {                         // (clamped into the tensor: rows >= M are not stored)
                    int G;
                    const int t = blk_of(wr * MI + mi, G);
                    mo = (long)(G * 16 + j) * p.HW + phase_blk(p, t).row;
                }
                half8 rr[2];
                if constexpr (RES) {
                    const long mr = min(mo, (long)p.M - 1);
#pragma unroll
                    for (int qn = 0; qn < 2; ++qn) rr[qn] = *reinterpret_cast<const half8 *>(p.res + (mr * p.ldy + ch0 + qn * 32) * 2);
                }
#pragma unroll
                for (int qn = 0; qn < 2; ++qn) {
                    const half8 o = epi_unit<RES, RELU>(acc[mi][2 * qn], acc[mi][2 * qn + 1], bq[qn][0], bq[qn][1], rr[qn]);
                    if constexpr (OIDX) {                      // row y_idx[mo], or no store (one unsigned compare: not negative, below y_rows)
                        if ((FULL || m < p.M) && (unsigned)yrow[mi] < p.y_rows)
                            *reinterpret_cast<half8 *>(p.y + ((long)yrow[mi] * p.ldy + ch0 + qn * 32) * 2) = o;
                    } else if (FULL || m < p.M)
                        *reinterpret_cast<half8 *>(p.y + (mo * p.ldy + ch0 + qn * 32) * 2) = o;
                }
            }
        };
        // (epi_dispatch of conv_prims.h, written out: called through it, the 256 x 256 builds' K loops get other registers)
        const bool full = m0 + TILE <= p.M;
        auto by_full = [&](auto r_, auto l_) {
            if (full)
                epilogue(r_, l_, std::true_type{});
            else
                epilogue(r_, l_, std::false_type{});
        };
        auto by_relu = [&](auto r_) {
            if (p.relu)
                by_full(r_, std::true_type{});
            else
                by_full(r_, std::false_type{});
        };
        if (!OIDX && p.res)                                    // (OIDX: the launcher refuses a residual)
            by_relu(std::true_type{});
        else
            by_relu(std::false_type{});
    } else {
    asm volatile("s_barrier" ::: "memory");
    floatx4 *stg = reinterpret_cast<floatx4 *>(smem);
    half8 r0[8];
    const StagedEpi<512, _Float16, half8, PanelK> epi{p, tid, g, j, m0, n0, stg};     // (conv_prims.h; one residual set, loaded twice)
    epi.load_res(0, r0);
    if (wr == 0) epi.stage<0, 8>(wc * 64, acc);
    lds_barrier();
    epi.write(0, r0);
    epi.load_res(1, r0);
    lds_barrier();
    if (wr == 1) epi.stage<0, 8>(wc * 64, acc);
    lds_barrier();
    epi.write(1, r0);
    }
    if constexpr (DBG & 4) {
        unsigned long st_k1;
        asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_k1)::"memory");
        if (threadIdx.x == 0) {
            unsigned long *o = p.stamps + (long)blockIdx.x * 6;
            o[0] = st_c1 - st_c0;       // K loop, core cycles
            o[1] = st_r1 - st_r0;       // K loop, 10 ns ticks
            o[2] = st_k1 - st_k0;       // whole workgroup, 10 ns ticks
            o[3] = st_r0 - st_k0;       // start .. K loop start
            o[4] = st_k0;               // absolute start / end (10 ns ticks): which XCD finishes when
            o[5] = st_k1;
        }
    }
}

static int panel_pp(const ConvArgs &a, int mi = 8) {
    const int reach = a.dil * (a.W + 1);
    if (mi == 9) return reach <= 48 ? 3 : (reach <= 112 ? 4 : 0);
    return reach <= 64 ? 3 : (reach <= 128 ? 4 : 0);
}

// 8 or 9 row tiles per wave (256- or 288-pixel tiles): whichever takes fewer MFMA rows over the rounds of the grid on a device
// of n_cu CUs.  VK_PANEL_MI=8 / 9 forces one where it is legal.
static int panel_mi(const ConvArgs &a, long M, int n_cu) {
    if (panel_pp(a, 9) == 0) return 8;
    if (const char v = env_first("VK_PANEL_MI"); v == '8' || v == '9') return v - '0';
    // few rounds: count MFMA rows over the rounds (res4 of 32 images: 3 x 8 against 2 x 9).  Many rounds: the workgroups drift apart
    // and the rounds blur; 36 MFMAs per barrier instead of 32 then win by ~1 % (measured on the Res5 conv2 grids, 14 rounds)
    const long nt = a.Cout / 256;
    const long n8 = ((M + 255) / 256 * nt + n_cu - 1) / n_cu, n9 = ((M + 287) / 288 * nt + n_cu - 1) / n_cu;
    if (n8 > 4) return 9;
    return n9 * 9 < n8 * 8 ? 9 : 8;
}

bool conv3x3_panel_eligible(const ConvArgs &a) {
    if (env_off("VK_CONV3X3_PANEL")) return false;
    if (a.stem || a.dt != VK_F16 || a.out_dt != VK_F16 || a.relu > 1) return false;
    if (a.kh != 3 || a.kw != 3 || a.stride != 1 || a.pad != a.dil) return false;
    if (a.Cout % 256 != 0 || a.ldy != a.Cout || a.Cin % 64 != 0 || a.Cin < 128) return false;
    if (panel_pp(a) == 0) return false;
    if ((a.x_idx ? a.x_rows : (long)a.N * a.H * a.W) * a.Cin * 2 >= (1L << 32)) return false;   // 32-bit DMA offsets (of the indexed tensor, with x_idx)
    // no lower bound on M: the K walk (channel-stage major, tap minor) sums in a different order than the
    // im2col kernels, and a layer's bits must not depend on how many RoIs share a launch (head chunking)
    return true;
}

// The leading images of the launch that take the PHASE form (whole groups of 16), 0 = none.  f16 is implied by the panel kernel;
// dilation 2, even H, even W <= 14 (halo (W / 2 + 1) * 16 <= 128 rows); H <= 1024 keeps the reciprocal of W / 2 exact.
// VK_PANEL_PHASE=0 selects the plain form.
static bool panel_phase_off() { return env_off("VK_PANEL_PHASE"); }
#ifdef VK_ABLATION      // VK_PANEL_PHASE=A: the phase form's row order with every MFMA still issued, on zeroed fragments (what the order alone costs)
static bool panel_phase_ablation() { return env_first("VK_PANEL_PHASE") == 'A'; }
#endif

int conv3x3_panel_phase_images(const ConvArgs &a) {
    if (panel_phase_off()) return 0;
    if (a.dil != 2 || a.H % 2 != 0 || a.W % 2 != 0 || a.W > 14 || a.H > 1024 || a.N < 16) return 0;
    return a.N / 16 * 16;
}

// Rows of a tile of the launch's phase part: 512 (512 x 128 tiles), 256 under VK_PANEL_TALL=0 (the 256 x 256 phase
// instantiation), 0 where no image of the launch takes the phase form.
int conv3x3_panel_phase_tile_rows(const ConvArgs &a) {
    if (a.Cout % 256 != 0 || conv3x3_panel_phase_images(a) == 0) return 0;
    return env_off("VK_PANEL_TALL") ? 256 : 512;
}

// 1 where the launch's phase part runs the fragment-window schedule (REUSE): every 512 x 128 launch, unless
// VK_PANEL_REUSE=0 selects the schedule in which each tap reads its eight fragments.
int conv3x3_panel_phase_reuse(const ConvArgs &a) {
    if (conv3x3_panel_phase_tile_rows(a) != 512) return 0;
    return env_off("VK_PANEL_REUSE") ? 0 : 1;
}

// 1 where the WHOLE launch runs the 512 x 128 fragment-window phase form, the one form that reads its input through a row index
// (ConvArgs::x_idx): every image in a group of 16, none of VK_PANEL_PHASE / TALL / REUSE = 0.  VK_PANEL_INDEXED=0
// answers 0 everywhere: callers then gather the rows and launch the dense form (the A/B and bit-identity partner).
int conv3x3_panel_phase_indexed(const ConvArgs &a) {
    if (env_off("VK_PANEL_INDEXED")) return 0;
    return conv3x3_panel_phase_images(a) == a.N && conv3x3_panel_phase_reuse(a) == 1 ? 1 : 0;
}

// 1 where the launch can store its rows through an index (ConvArgs::y_idx): the form above, whatever
// VK_PANEL_INDEXED says (the output index does not need the input one).  VK_PANEL_OUT_INDEXED=0 answers 0 everywhere: Res5 block 0
// then writes the dense rows and gathers the representatives (the A/B and bit-identity partner).
int conv3x3_panel_out_indexed(const ConvArgs &a) {
    if (env_off("VK_PANEL_OUT_INDEXED")) return 0;
    return conv3x3_panel_phase_images(a) == a.N && conv3x3_panel_phase_reuse(a) == 1 ? 1 : 0;
}

static int launch_panel_one(const ConvArgs &a, hipStream_t stream, bool phase);

int launch_conv3x3_panel(const ConvArgs &a, hipStream_t stream) {
    const int np = conv3x3_panel_phase_images(a);
    // ... and so is an output index: any other form would store every row where it always did
    VK_REQUIRE(!a.y_idx || conv3x3_panel_out_indexed(a), VK_EINVAL,
               "conv3x3_panel: y_idx needs the whole launch in the 512 x 128 fragment-window phase form (N %% 16 == 0, dilation 2, even H, "
               "even W <= 14; VK_PANEL_PHASE / TALL / REUSE / OUT_INDEXED not 0): N=%d H=%d W=%d dil=%d", a.N, a.H, a.W, a.dil);
    VK_REQUIRE(!a.y_idx || !a.res, VK_EINVAL, "conv3x3_panel: y_idx takes no residual (its rows would be those of the dense output)");
    VK_REQUIRE(!a.y_idx || a.y_rows > 0, VK_EINVAL, "conv3x3_panel: y_idx needs y_rows > 0, the rows of y (got %ld)", a.y_rows);
    // a row index is read by one instantiation alone: any other form would run on the wrong rows
    VK_REQUIRE(!a.x_idx || conv3x3_panel_phase_indexed(a), VK_EINVAL,
               "conv3x3_panel: x_idx needs the whole launch in the 512 x 128 fragment-window phase form (N %% 16 == 0, dilation 2, even H, "
               "even W <= 14; VK_PANEL_PHASE / TALL / REUSE / INDEXED not 0): N=%d H=%d W=%d dil=%d", a.N, a.H, a.W, a.dil);
    if (np == 0) return launch_panel_one(a, stream, false);
    ConvArgs b = a;
    b.N = np;
    VK_TRY(launch_panel_one(b, stream, true));
    if (np == a.N) return VK_OK;
    // the remainder (fewer than 16 images) in the plain form: a row's bits do not depend on the form or on its launch
    const size_t rows = (size_t)np * a.H * a.W;
    b.N = a.N - np;
    b.x = (const char *)a.x + rows * a.Cin * 2;
    b.y = (char *)a.y + rows * a.ldy * 2;
    if (a.res) b.res = (const char *)a.res + rows * a.ldy * 2;
    return launch_panel_one(b, stream, false);
}

static int launch_panel_one(const ConvArgs &a, hipStream_t stream, bool phase) {
    DeviceState *ds = nullptr;
    VK_TRY(device_state(&ds));
    PanelK k;
    k.x = (const char *)a.x;
    k.w = (const char *)a.w;
    k.bias = a.bias;
    k.res = (const char *)a.res;
    k.y = (char *)a.y;
    k.H = a.H;
    k.W = a.W;
    k.HW = a.H * a.W;
    const long M = (long)a.N * a.H * a.W;
    VK_REQUIRE(M > 0 && M < (1L << 31) - 512, VK_EINVAL, "conv3x3_panel: M=%ld out of range", M);
    // (with x_idx the offsets are those of the indexed tensor: the caller states its rows)
    VK_REQUIRE(!a.x_idx || a.x_rows > 0, VK_EINVAL, "conv3x3_panel: x_idx needs x_rows > 0, the rows of x (got %ld)", a.x_rows);
    const long xr = a.x_idx ? a.x_rows : M;
    VK_REQUIRE(xr * a.Cin * 2 < (1L << 32) && (long)a.Cout * 9 * a.Cin * 2 < (1L << 32), VK_EINVAL,
               "conv3x3_panel: tensor beyond the 32-bit DMA offsets (rows of x=%ld Cin=%d Cout=%d)", xr, a.Cin, a.Cout);
    k.x_idx = a.x_idx;
    k.y_idx = a.y_idx;
    k.y_rows = (unsigned)std::min<long>(a.y_idx ? a.y_rows : 0, 1L << 31);      // (an index is below 2^31)
    k.M = (int)M;
    k.cin_bytes = a.Cin * 2;
    k.ldy = a.ldy;
    k.dil = a.dil;
    k.cstages = a.Cin / 32;
    k.wrow_bytes = 9 * a.Cin * 2;
    k.relu = a.relu;
    // phase launches take 512 x 128 tiles (4 x 2 waves, 6 panel pieces, 8 KiB weight slots); the plain form and VK_PANEL_TALL=0 keep 256 columns
    bool tall = phase && conv3x3_panel_phase_tile_rows(a) == 512;
#ifdef VK_ABLATION
    if (panel_phase_ablation()) tall = false;      // (the PHASE = 1 build has 256 x 256 tiles only)
#endif
    const int mi = phase ? 8 : panel_mi(a, M, ds->n_cu), pp = tall ? 6 : (phase ? 4 : panel_pp(a, mi));
    const int wslot = tall ? P_WSLOT / 2 : P_WSLOT;
    k.groups = phase ? a.N / 16 : 0;
    k.rcp_w2 = phase ? 65536u / (unsigned)(a.W / 2) + 1u : 0u;
    k.m_tiles = ceil_div(k.M, tall ? 512 : mi * 32);
    k.n_tiles = a.Cout / (tall ? 128 : 256);
    Timed t;
    VK_TRY(t.begin(stream));
    const int total_tiles = k.m_tiles * k.n_tiles;
    k.tile_ctr = nullptr;
    k.static_tiles = total_tiles;
    int n_wgs = total_tiles;
    // many rounds on every CU: the last sixteenth is handed out dynamically (VK_PANEL_DYNAMIC=0: every tile static)
    if (!env_off("VK_PANEL_DYNAMIC") && (pp == 3 || phase) && total_tiles >= 16 * 256) {
        VK_TRY(acquire_tile_counter(&k.tile_ctr));
        // (a multiple of 8: whole rounds of the XCD map, and whole panels: the 2 or 4 column tiles of a panel stay together, since the
        //  kernel takes n_tile = t_ % n_tiles of consecutive tile indices of one XCD)
        k.static_tiles = total_tiles * 15 / 16 / 8 * 8;
        n_wgs = total_tiles + (total_tiles / 32 + 63) / 64 * 64;    // spare workgroups: an XCD 3 % faster than the mean can take 3 % more tiles
        k.ctr_last = (unsigned)(n_wgs - k.static_tiles - 1);
    }
    const dim3 grid(n_wgs), block(512);
#ifdef VK_ABLATION
    const int dbg = env_int("VK_CONV256_DBG", 0);
#endif
    const int smem = 2 * pp * 128 * 64 + P_NW * wslot + (pp == 3 || tall ? 256 : 0);      // PP = 3: + the zero row; 512 x 128: + the tail's mailbox word
    k.stamps = nullptr;
    // (the limit of a PP-piece build is that of its 256-column form, whatever this launch's smem)
#define VKP_LAUNCH(PP_, DBG_, TAG_, MI_)                                                                   \
    VK_TRY(launch_lds(conv3x3_panel_kernel<PP_, DBG_, TAG_, MI_>, grid, block, smem,                       \
                      2 * PP_ * 128 * 64 + P_NW * P_WSLOT + (PP_ == 3 ? 256 : 0), stream, k))
#define VKP_LAUNCH_PHASE(...) VK_TRY(launch_lds(conv3x3_panel_kernel<__VA_ARGS__>, grid, block, smem, smem, stream, k))
#ifdef VK_ABLATION      // stamp / timing-only (dbg 1: WRONG results) / LDS-epilogue builds: tools/ builds only (make ABLATION=1)
    if (const char *sf = env_text("VK_PANEL_STAMPS"); sf && pp == 3) {   // diagnostic: one stamped launch (halo-64 / 48 build), 6 words per workgroup appended to the file
        Stamps st;
        VK_TRY(st.open((size_t)grid.x * 6, stream));              // (spare workgroups of a dynamic tail leave without a stamp)
        k.stamps = st.dev;
        if (mi == 9)
            VKP_LAUNCH(3, 4, 0, 9);
        else
            VKP_LAUNCH(3, 4, 0, 8);
        VK_TRY(st.finish(stream, sf, "# wg k_loop_cycles k_loop_ticks workgroup_ticks ticks_before_k_loop start_tick end_tick (tick = 10 ns)",
                         grid.x, 6, 6, 0));
    } else if (mi == 8 && pp == 3 && dbg == 8)
        VKP_LAUNCH(3, 8, 0, 8);
    else if (mi == 8 && pp == 3 && dbg == 1)
        VKP_LAUNCH(3, 1, 0, 8);
    else if (mi == 9 && pp == 3 && dbg == 1)
        VKP_LAUNCH(3, 1, 0, 9);
    else if (mi == 9 && pp == 3 && dbg == 16)
        VKP_LAUNCH(3, 16, 0, 9);
    else if (mi == 9 && pp == 3 && dbg == 32)
        VKP_LAUNCH(3, 32, 0, 9);
    else if (phase && panel_phase_ablation())
        VKP_LAUNCH_PHASE(4, 0, 0, 8, 1);
    else
#endif
    if (a.y_idx) {
        VK_REQUIRE(tall && conv3x3_panel_phase_reuse(a) && !a.res, VK_EINVAL, "conv3x3_panel: y_idx outside the fragment-window phase form");
        if (a.x_idx)
            VKP_LAUNCH_PHASE(6, 0, 0, 8, 2, 4, 1, 1, 1);
        else
            VKP_LAUNCH_PHASE(6, 0, 0, 8, 2, 4, 1, 0, 1);
    } else if (a.x_idx) {
        VK_REQUIRE(tall && conv3x3_panel_phase_reuse(a), VK_EINVAL, "conv3x3_panel: x_idx outside the fragment-window phase form");
        VKP_LAUNCH_PHASE(6, 0, 0, 8, 2, 4, 1, 1);
    } else if (tall && conv3x3_panel_phase_reuse(a))
        VKP_LAUNCH_PHASE(6, 0, 0, 8, 2, 4, 1);
    else if (tall)
        VKP_LAUNCH_PHASE(6, 0, 0, 8, 2, 4);
    else if (phase)        // (one symbol: the form is not launched beside another stream's kernels)
        VKP_LAUNCH_PHASE(4, 0, 0, 8, 2);
    else if (mi == 8 && pp == 3 && a.concurrent)
        VKP_LAUNCH(3, 0, 1, 8);
    else if (mi == 8 && pp == 3)
        VKP_LAUNCH(3, 0, 0, 8);
    else if (mi == 8 && a.concurrent)
        VKP_LAUNCH(4, 0, 1, 8);
    else if (mi == 8)
        VKP_LAUNCH(4, 0, 0, 8);
    else if (pp == 3 && a.concurrent)
        VKP_LAUNCH(3, 0, 1, 9);
    else if (pp == 3)
        VKP_LAUNCH(3, 0, 0, 9);
    else if (a.concurrent)
        VKP_LAUNCH(4, 0, 1, 9);
    else
        VKP_LAUNCH(4, 0, 0, 9);
#undef VKP_LAUNCH_PHASE
#undef VKP_LAUNCH
    return t.end(stream, a.concurrent ? 6 : 4, 2.0 * (double)k.M * a.Cout * 9 * a.Cin, k.M, a.Cout, a.Cin, 9, 1,
                 2.0 * ((double)k.M * a.Cin + (double)k.M * a.Cout * (a.res ? 2 : 1) + (double)a.Cout * 9 * a.Cin));
}

}  // namespace vk
