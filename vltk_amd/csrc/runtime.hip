// What every launcher of libvltk_hip.so links against and nothing of which knows what a model is: the per-launch event
// timer (KernelTimer, Timed), the launcher state per device (device_state, set_max_lds), the reader of the environment (env_*),
// the stamped launch of the ablation build (Stamps) and the thread's error text.
// The one translation unit that queries device properties, raises an LDS limit, keeps state between launches or calls
// getenv (tests/test_launcher_state.py).
#include <cstdlib>
#include <mutex>
#include <set>

#include "vk_common.h"

namespace vk {

thread_local KernelTimer *g_timer = nullptr;

hipEvent_t KernelTimer::get() {
    if (pool.empty()) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        all.push_back(e);
        return e;
    }
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
}
void KernelTimer::collect() {
    const char *logp = env_text("VK_CONV_LOG");   // debug: one line per conv launch (shape, ms, TFLOP/s)
    FILE *lf = logp ? fopen(logp, "a") : nullptr;
    std::vector<Rec> pending;       // launches of a forward that is still in flight (vk_forward_begin without its _end yet)
    for (auto &r : recs) {
        float t = 0.f;
        if (hipEventQuery(r.e1) != hipSuccess) {
            pending.push_back(r);
            continue;
        }
        if (hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) {
            if (lf) fprintf(lf, "%d %d %d %d %d %d %.5f %.1f\n", r.bucket, r.M, r.cout, r.cin, r.k, r.stride, t, r.flops / (t * 1e-3) / 1e12);
            launches[r.bucket] += 1;
            ms[r.bucket] += t;
            flops[r.bucket] += r.flops;
            bytes[r.bucket] += r.bytes;
        }
        pool.push_back(r.e0);
        pool.push_back(r.e1);
    }
    if (lf) fclose(lf);
    recs.swap(pending);
    (void)hipGetLastError();        // hipEventQuery's "not ready" must not show up in a later launch check
}
KernelTimer::~KernelTimer() {
    for (auto e : all) (void)hipEventDestroy(e);
}

int Timed::begin(hipStream_t stream) {
    if (!tm) return VK_OK;
    e0 = tm->get();
    e1 = tm->get();
    VK_CHECK_HIP(hipEventRecord(e0, stream));
    return VK_OK;
}
int Timed::end(hipStream_t stream, int bucket, double flops, int M, int cout, int cin, int k, int stride, double bytes) {
    if (!tm) return VK_OK;
    VK_CHECK_HIP(hipEventRecord(e1, stream));
    tm->recs.push_back({bucket, flops, e0, e1, M, cout, cin, k, stride, bytes});
    return VK_OK;
}

// Launcher state per device: published once fully built; the lock only serialises the first launch on each device.
static std::atomic<DeviceState *> g_devices[VK_MAX_DEVICES];
static std::mutex g_devices_mu;

int device_state(DeviceState **out) {
    int dev = 0;
    VK_CHECK_HIP(hipGetDevice(&dev));
    VK_REQUIRE(dev >= 0 && dev < VK_MAX_DEVICES, VK_EINVAL, "device %d beyond VK_MAX_DEVICES", dev);
    DeviceState *d = g_devices[dev].load(std::memory_order_acquire);
    if (!d) {
        std::lock_guard<std::mutex> lock(g_devices_mu);
        d = g_devices[dev].load(std::memory_order_relaxed);
        if (!d) {
            hipDeviceProp_t prop;
            VK_CHECK_HIP(hipGetDeviceProperties(&prop, dev));
            // one allocation: [zero page 256 B][tile ring 256 words][bneck scratch]; the first two start zeroed, and the
            // scratch comes last so that nothing it receives can land in them
            char *p = nullptr;
            VK_CHECK_HIP(hipMalloc((void **)&p, 256 + 256 * sizeof(unsigned) + BN_TRASH_BYTES));
            VK_CHECK_HIP(hipMemset(p, 0, 256 + 256 * sizeof(unsigned)));     // (synchronous: done before any launch can read it)
            d = new DeviceState;
            d->n_cu = prop.multiProcessorCount;
            d->zero_page = p;
            d->tile_ring = (unsigned *)(p + 256);
            d->bn_trash = p + 256 + 256 * sizeof(unsigned);
            d->tile_next = 0;
            g_devices[dev].store(d, std::memory_order_release);
        }
    }
    *out = d;
    return VK_OK;
}

static std::set<std::pair<int, const void *>> g_lds_set;     // (device, kernel) pairs whose LDS limit is raised
static std::mutex g_lds_mu;

int set_max_lds(const void *kernel, size_t bytes) {
    int dev = 0;
    VK_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_lds_mu);
    if (g_lds_set.count({dev, kernel})) return VK_OK;
    VK_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    g_lds_set.insert({dev, kernel});
    return VK_OK;
}

const char *env_text(const char *name) { return getenv(name); }
bool env_set(const char *name) { return getenv(name) != nullptr; }
char env_first(const char *name) {
    const char *v = getenv(name);
    return v ? v[0] : '\0';
}
bool env_off(const char *name) { return env_first(name) == '0'; }
int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

#ifdef VK_ABLATION
int Stamps::open(size_t n, hipStream_t stream) {
    words = n;
    VK_CHECK_HIP(hipMalloc((void **)&dev, words * sizeof(unsigned long)));
    VK_CHECK_HIP(hipMemsetAsync(dev, 0, words * sizeof(unsigned long), stream));     // (a workgroup may leave without a stamp)
    return VK_OK;
}
int Stamps::finish(hipStream_t stream, const char *path, const char *header, size_t rows, int stride, int cols, int per_wg) {
    VK_CHECK_HIP(hipStreamSynchronize(stream));
    std::vector<unsigned long> h(words);
    VK_CHECK_HIP(hipMemcpy(h.data(), dev, words * sizeof(unsigned long), hipMemcpyDeviceToHost));
    VK_CHECK_HIP(hipFree(dev));
    dev = nullptr;
    FILE *f = fopen(path, "a");
    if (!f) return VK_OK;
    fprintf(f, "%s\n", header);
    for (size_t r = 0; r < rows && (r + 1) * stride <= words; ++r) {
        if (per_wg)
            fprintf(f, "%zu %zu", r / per_wg, r % per_wg);
        else
            fprintf(f, "%zu", r);
        for (int i = 0; i < cols; ++i) fprintf(f, " %lu", h[r * stride + i]);
        fprintf(f, "\n");
    }
    fclose(f);
    return VK_OK;
}
#endif

static thread_local char g_err[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace vk

extern "C" {

const char *vk_last_error(void) { return vk::g_err; }
int vk_version(void) { return 1; }

}  // extern "C"
