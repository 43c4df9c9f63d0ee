// Host-only weight packing: the conv and stem weights as the kernels read them (BN folded, rows padded to whole output
// tiles, K ordered tap by tap), and the float -> storage type conversion.  Nothing here calls the HIP runtime.
#include <algorithm>
#include <cmath>

#include "vk_common.h"

using namespace vk;

namespace vk {

void to_dt(const float *src, size_t n, vk_dtype dt, void *dst) {
    if (dt == VK_F16) {
        _Float16 *d = (_Float16 *)dst;
        for (size_t i = 0; i < n; ++i) d[i] = (_Float16)src[i];
    } else if (dt == VK_BF16) {          // round to nearest even, like torch's float -> bfloat16
        uint16_t *d = (uint16_t *)dst;
        for (size_t i = 0; i < n; ++i) {
            uint32_t u;
            memcpy(&u, &src[i], 4);
            if ((u & 0x7fffffffu) > 0x7f800000u)
                d[i] = (uint16_t)((u >> 16) | 0x40);              // NaN stays NaN
            else
                d[i] = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        }
    } else {
        memcpy(dst, src, n * sizeof(float));
    }
}

}  // namespace vk

extern "C" {

int vk_packed_cout(int cout) { return (cout + CONV_COUT_ALIGN - 1) / CONV_COUT_ALIGN * CONV_COUT_ALIGN; }

int vk_conv_slice_channels(int cin, int groups) {
    if (groups <= 1) return cin;
    if (cin <= 0 || cin % groups != 0) return -1;
    const int cpg = cin / groups;
    if (cpg & (cpg - 1)) return -1;                     // power of two: slices and groups nest
    return std::min(std::max(cpg, 64), cin);
}

size_t vk_packed_weight_bytes(int cout, int cin, int kh, int kw, int groups, vk_dtype dt) {
    const int sw = vk_conv_slice_channels(cin, groups);
    return sw <= 0 ? 0 : (size_t)vk_packed_cout(cout) * kh * kw * sw * dtype_size(dt);
}

int vk_pack_conv_weight(const float *w, const float *bn, const float *bias, int cout, int cin, int kh, int kw, int groups,
                        vk_dtype dt, void *w_packed, float *bias_packed) {
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32 || dt == VK_BF16, VK_EINVAL, "pack: dtype must be f16, bf16 or f32");
    VK_REQUIRE(groups >= 1, VK_EINVAL, "pack: groups=%d", groups);
    const int sw = vk_conv_slice_channels(cin, groups);     // K channels per tap in the packed row (== cin when dense)
    VK_REQUIRE(sw > 0, VK_EINVAL, "pack: cin=%d / groups=%d must be a power of two", cin, groups);
    VK_REQUIRE(groups == 1 || cin == cout, VK_EINVAL, "pack: grouped convolution needs cin == cout (got %d, %d)", cin, cout);
    VK_REQUIRE((sw * (int)dtype_size(dt)) % CONV_KTILE_BYTES == 0, VK_EINVAL,
               "pack: %d channels per tap is not a whole number of 128-byte K-tiles for this dtype", sw);
    const int cp = vk_packed_cout(cout);
    const int cpg = cin / groups;                           // input channels of one group (= row length of w_oihw)
    const size_t K = (size_t)kh * kw * sw;
    std::vector<float> row(K);
    for (int co = 0; co < cp; ++co) {
        double s = 1.0;
        float b = 0.f;
        std::fill(row.begin(), row.end(), 0.f);
        if (co < cout) {
            if (bn) {   // eval BatchNorm folded into the conv: eps 1e-5 (nn.BatchNorm2d default)
                const double g = bn[co], be = bn[cout + co], mu = bn[2 * (size_t)cout + co], var = bn[3 * (size_t)cout + co];
                s = g / std::sqrt(var + 1e-5);
                b = (float)(be - mu * s);
            } else if (bias) {
                b = bias[co];
            }
            // the slice this channel's 64-wide output tile reads starts at slice0; its own group at g0
            const int slice0 = groups == 1 ? 0 : (co / 64 * 64) / sw * sw;
            const int g0 = groups == 1 ? 0 : co / cpg * cpg;
            for (int c = 0; c < cpg; ++c)
                for (int y = 0; y < kh; ++y)
                    for (int x = 0; x < kw; ++x)
                        row[((size_t)y * kw + x) * sw + (g0 + c - slice0)] =
                            (float)((double)w[(((size_t)co * cpg + c) * kh + y) * kw + x] * s);
        }
        bias_packed[co] = b;
        to_dt(row.data(), K, dt, (char *)w_packed + (size_t)co * K * dtype_size(dt));
    }
    return VK_OK;
}

size_t vk_packed_stem_bytes(int cout, vk_dtype dt) {
    const int ktiles = dt == VK_F16 ? 4 : 7;
    return (size_t)vk_packed_cout(cout) * ktiles * CONV_KTILE_BYTES;
}

int vk_pack_stem_weight(const float *w, const float *bn, int cout, vk_dtype dt, void *w_packed, float *bias_packed) {
    VK_REQUIRE(dt == VK_F16 || dt == VK_F32, VK_EINVAL, "pack_stem: dtype must be f16 or f32");
    const int cp = vk_packed_cout(cout);
    const int ktiles = dt == VK_F16 ? 4 : 7;
    const size_t K = (size_t)ktiles * CONV_KTILE_BYTES / dtype_size(dt);   // 256 (f16) / 224 (f32)
    std::vector<float> row(K);
    for (int co = 0; co < cp; ++co) {
        std::fill(row.begin(), row.end(), 0.f);
        float b = 0.f;
        if (co < cout) {
            double s = 1.0;
            if (bn) {
                const double g = bn[co], be = bn[cout + co], mu = bn[2 * (size_t)cout + co], var = bn[3 * (size_t)cout + co];
                s = g / std::sqrt(var + 1e-5);
                b = (float)(be - mu * s);
            }
            for (int c = 0; c < 3; ++c)
                for (int y = 0; y < 7; ++y)
                    for (int x = 0; x < 7; ++x)   // K index = kernel row * 32 + (kernel col * 4 + channel)
                        row[(size_t)y * 32 + x * 4 + c] = (float)((double)w[(((size_t)co * 3 + c) * 7 + y) * 7 + x] * s);
        }
        bias_packed[co] = b;
        to_dt(row.data(), K, dt, (char *)w_packed + (size_t)co * K * dtype_size(dt));
    }
    return VK_OK;
}

}  // extern "C"
