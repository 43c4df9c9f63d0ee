// Device-side primitives shared by the conv kernels (include after vk_common.h, inside .hip files only): the vector types,
// the LDS-DMA request, the workgroup -> tile map, the raw LDS barrier and the epilogue arithmetic.  "A layer's bits do not
// depend on which kernel the dispatcher picks" holds because every kernel's epilogue is the code below, not a restatement.
#pragma once
#include <cstdint>
#include <type_traits>

namespace vk {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One LDS-DMA request (global_load_lds_dwordx4): 16 B per lane from gptr straight into LDS, no VGPR staging.  The LDS image
// is lane-linear per wave-instruction (lptr is the wave's base), so any swizzle goes on the SOURCE address.
__device__ __forceinline__ void glds16(const void *gptr, void *lptr) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gptr, (__attribute__((address_space(3))) void *)lptr, 16, 0,
                                     0);
}

// XCD-aware (bijective) workgroup -> tile map: the 8 XCDs each get a contiguous range of tiles (workgroup bid runs on XCD
// bid & 7), and within it tiles that share the same pixel rows (different channel tiles: n_tile = t % n_tiles) are
// adjacent, so the pixel panel is fetched from HBM once per XCD L2.
__device__ __forceinline__ int xcd_tile(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// Raw workgroup barrier that waits for this wave's LDS traffic only: global loads / stores stay in flight across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- register-form epilogue: a lane's 8 consecutive channels of one pixel, straight from the accumulator layout ----
// (x + residual), v_cvt_pk_f16_f32, ReLU on the rounded halves (the same bits as max before rounding; NaN -> 0 either way).
// x0 / x1 already hold acc + bias: a kernel that waits for its residual between the two adds calls this half on its own.
template <bool RES, bool RELU>
__device__ __forceinline__ half8 epi_finish(floatx4 x0, floatx4 x1, const half8 &rr) {
    if constexpr (RES) {
        x0 += __builtin_convertvector(__builtin_shufflevector(rr, rr, 0, 1, 2, 3), floatx4);
        x1 += __builtin_convertvector(__builtin_shufflevector(rr, rr, 4, 5, 6, 7), floatx4);
    }
    half4 h0 = __builtin_convertvector(x0, half4), h1 = __builtin_convertvector(x1, half4);
    half8 o = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (RELU) o = __builtin_elementwise_max(o, half8{0, 0, 0, 0, 0, 0, 0, 0});
    return o;
}
// the whole unit: a0 / a1 the two accumulator tiles, b0 / b1 their bias, rr the residual (read only when RES)
template <bool RES, bool RELU>
__device__ __forceinline__ half8 epi_unit(floatx4 a0, floatx4 a1, floatx4 b0, floatx4 b1, const half8 &rr) {
    return epi_finish<RES, RELU>(a0 + b0, a1 + b1, rr);
}

// Runtime flags -> compile-time booleans: f(res_c, relu_c, full_c) with std::bool_constant arguments, one copy of the
// epilogue per combination (residual present, ReLU, whole tile inside M).  The flags come by reference (p.res, p.relu as they
// are) and are tested here, in this order: the caller's code is what the nested if / else ladders it replaces compiled to.
template <typename B, typename F>
__device__ __forceinline__ void by_flag(const B &b, F &&f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
template <typename R, typename L, typename F>
__device__ __forceinline__ void epi_dispatch(const R &res, const L &relu, const bool &full, F &&f) {
    by_flag(res, [&](auto r_) { by_flag(relu, [&](auto l_) { by_flag(full, [&](auto u_) { f(r_, l_, u_); }); }); });
}

// ---- LDS-staged tile epilogue: + bias (+ residual) (ReLU) -> 16-bit, through LDS so that HBM sees whole rows ----
// In the accumulator layout a wave-instruction touches 16 rows x 64 B (half cache lines).  The K loop's LDS is dead by
// now, so the f32 tile goes through it in two halves of NT / 4 rows x 256 channels (16-B chunks XOR-swizzled by row) and is
// read back row-contiguous: every residual load and every store of a wave covers 2 rows x 512 B = 8 whole 128-B lines.
// NT = threads of the workgroup (512: 128-row halves, 256: 64-row halves); thread tid owns eight 8-channel pieces of a half,
// piece i = 16-B chunk k8 of row `row` with tid + NT * i = row * 32 + k8.  ET / V8: the 16-bit element type and its vector.
// P is the kernel's argument struct (res, bias, y, M, ldy, relu).  The three bodies are shared; each kernel keeps its own
// sequence of calls, residual register sets and barriers.
// The members are REFERENCES to the kernel's own variables, as a [&] lambda's captures are: handed over by value the same
// bodies compile to a different kernel (other registers, the argument loads split up), measured on conv_mfma256.hip.
template <int NT, typename ET, typename V8, typename P>
struct StagedEpi {
    const P &p;
    const int &tid, &g, &j;      // thread, and its lane's place in the accumulator layout (lane >> 4, lane & 15)
    const int &m0, &n0;          // the tile's origin
    floatx4 *const &stg;         // the staging tile: [NT / 4 rows][64 chunks of 4 floats]

    // residual rows of half h -> registers (zeros without a residual); rows beyond M read row M - 1
    __device__ __forceinline__ void load_res(int h, V8 (&rr)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int it = tid + NT * i, row = it >> 5, k8 = it & 31;
            const int m = min(m0 + h * (NT / 4) + row, p.M - 1);
            if (p.res)
                rr[i] = *reinterpret_cast<const V8 *>(p.res + ((long)m * p.ldy + n0 + k8 * 8) * 2);
            else
                rr[i] = V8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    // this wave's accumulator row tiles [R0, R0 + NR) + bias -> staging rows 0 .. NR * 16 - 1; col0: the wave's first
    // tile-local channel of 64
    template <int R0, int NR, int NA>
    __device__ __forceinline__ void stage(int col0, const floatx4 (&acc)[NA][4]) const {
#pragma unroll
        for (int qn = 0; qn < 2; ++qn) {
            const int col = col0 + qn * 32 + g * 8;              // tile-local channel of this lane's 8 values
            const floatx4 b0 = reinterpret_cast<const floatx4 *>(p.bias + n0 + col)[0];
            const floatx4 b1 = reinterpret_cast<const floatx4 *>(p.bias + n0 + col)[1];
#pragma unroll
            for (int mq = 0; mq < NR; ++mq) {
                const int row = mq * 16 + j;
                const int c16 = col >> 2;
                stg[row * 64 + (c16 ^ (row & 7))] = acc[R0 + mq][2 * qn] + b0;
                stg[row * 64 + ((c16 + 1) ^ (row & 7))] = acc[R0 + mq][2 * qn + 1] + b1;
            }
        }
    }
    // half h out of the staging tile: (staged + residual) (ReLU), round to ET, rows below M to y
    // (conv_mfma_duo.hip keeps a write of its own, with its GELU branch and the fused mean in it: DESIGN.md 4a)
    __device__ __forceinline__ void write(int h, const V8 (&rr)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int it = tid + NT * i, row = it >> 5, k8 = it & 31;
            const int m = m0 + h * (NT / 4) + row;
            const floatx4 v0 = stg[row * 64 + ((2 * k8) ^ (row & 7))];
            const floatx4 v1 = stg[row * 64 + ((2 * k8 + 1) ^ (row & 7))];
            V8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = v0[e] + (float)rr[i][e], b = v1[e] + (float)rr[i][4 + e];
                if (p.relu) {
                    a = a > 0.f ? a : 0.f;
                    b = b > 0.f ? b : 0.f;
                }
                o[e] = (ET)a;
                o[4 + e] = (ET)b;
            }
            if (m < p.M) *reinterpret_cast<V8 *>(p.y + ((long)m * p.ldy + n0 + k8 * 8) * 2) = o;
        }
    }
};

}  // namespace vk
