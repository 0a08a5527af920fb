// side_host.hpp -- the host scaffold the side libraries share (devio, gate, consistency, health, lookahead, sequence, score, bank, imm, adapt, stateio: csrc/Makefile, SIDE).
// Host code only, every symbol internal: a library that includes it has an error string, a launch counter and a launch census of its
// own, and exports what its QLE_SIDE_* lines name.  A *_capi.hip file keeps its static_asserts, the refusals that are its own, its launches
// and its extern "C" entries; what every one of them needs around those is here.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/qle_ekf.h"
#include "device_mem.hpp"
#include "ekf_layout.hpp"

namespace qle {
namespace side {
namespace {

thread_local std::string g_err;
std::atomic<int64_t> g_launches{0};

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
// the two diagnostics entries of a library's header, over the library's own copies of the string and the counter
#define QLE_SIDE_LAST_ERROR(name) extern "C" const char* name(void) { return qle::side::g_err.c_str(); }
#define QLE_SIDE_LAUNCH_COUNT(name) extern "C" int64_t name(void) { return qle::side::g_launches.load(std::memory_order_relaxed); }

// after every launch: counts the launches the runtime took, not attempts
int launched()
{
    HIP_TRY(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);
    return QLE_OK;
}

// ---- launch census: the distinct kernels launch() has launched since <prefix>_launch_census_begin, process-wide and per library (the
// contract of qle_launch_census_begin / _end, include/qle_ekf.h).  A process may drive handles from several host threads, so the list
// is guarded by a mutex; while the census is off, launch() pays one relaxed atomic load.
std::atomic<bool> g_census_on{false};
std::mutex g_census_mu;
std::vector<const void*> g_census;

void census_record(const void* kernel)
{
    std::lock_guard<std::mutex> lock(g_census_mu);
    if (g_census_on.load(std::memory_order_relaxed) && std::find(g_census.begin(), g_census.end(), kernel) == g_census.end()) g_census.push_back(kernel);
}
int census_begin()
{
    std::lock_guard<std::mutex> lock(g_census_mu);
    g_census.clear();
    g_census_on.store(true, std::memory_order_relaxed);
    return QLE_OK;
}
// The host handle of a kernel is an exported symbol of the library whose name is the device kernel's mangled name; a handle the
// dynamic symbol table does not name is asked of the runtime.
const char* kernel_name(const void* kernel)
{
    Dl_info info;
    if (dladdr(kernel, &info) && info.dli_sname && info.dli_saddr == kernel) return info.dli_sname;
    return hipKernelNameRefByPtr(kernel, nullptr);
}
// stops the census; the list stays until the next begin, so it may be called again with a larger buffer
int census_end(char* names, int64_t cap, int64_t* needed)
{
    std::lock_guard<std::mutex> lock(g_census_mu);
    g_census_on.store(false, std::memory_order_relaxed);
    std::vector<std::string> list;
    for (const void* k : g_census) {
        const char* n = kernel_name(k);
        if (!n) return fail(QLE_ERR_INVALID, "launch census: no symbol name for the kernel at %p", k);
        list.emplace_back(n);
    }
    std::sort(list.begin(), list.end());
    std::string out;
    for (const std::string& n : list) out += n + "\n";
    if (needed) *needed = (int64_t)out.size() + 1;
    if (names) {
        if (cap < (int64_t)out.size() + 1) return fail(QLE_ERR_INVALID, "launch census: %lld bytes needed, %lld given", (long long)out.size() + 1, (long long)cap);
        std::memcpy(names, out.c_str(), out.size() + 1);
    }
    return QLE_OK;
}
// the two census entries of a library's header: <prefix>_launch_census_begin and <prefix>_launch_census_end
#define QLE_SIDE_LAUNCH_CENSUS(prefix)                                                                                        \
    extern "C" int prefix##_launch_census_begin(void) { return qle::side::census_begin(); }                                   \
    extern "C" int prefix##_launch_census_end(char* names, int64_t cap, int64_t* needed) { return qle::side::census_end(names, cap, needed); }

// Every kernel launch of a side library: the census sees the kernel's host handle, the runtime takes the launch, launched() counts it.
template <typename... P, typename... Args>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args)
{
    if (g_census_on.load(std::memory_order_relaxed)) census_record(reinterpret_cast<const void*>(kernel));
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return launched();
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// view->struct_size: the libraries differ, on purpose, and say which rule they keep where they call check_view
enum class ViewSize { exact, at_least };

// What every entry refuses about the view; no GPU call.  state_aligned: also refuse records that are not 16-byte aligned.
int check_view(const qle_device_view* v, ViewSize size, bool state_aligned)
{
    if (!v) return fail(QLE_ERR_INVALID, "view is null");
    if (size == ViewSize::exact ? v->struct_size != sizeof(qle_device_view) : v->struct_size < sizeof(qle_device_view))
        return fail(QLE_ERR_INVALID, "view: struct_size %u, this library was built for %zu", v->struct_size, sizeof(qle_device_view));
    if (v->dtype != QLE_F32 && v->dtype != QLE_F64) return fail(QLE_ERR_INVALID, "view: dtype %d", v->dtype);
    if (v->batch <= 0 || v->padded_batch != padded_filters(v->batch)) return fail(QLE_ERR_INVALID, "view: batch %lld / padded %lld", (long long)v->batch, (long long)v->padded_batch);
    if (!v->state || v->state_words != kSW) return fail(QLE_ERR_INVALID, "view: state records of %d words (this library: %d)", v->state_words, kSW);
    if (state_aligned && !aligned(v->state, 16)) return fail(QLE_ERR_INVALID, "view: state must be 16-byte aligned");
    if (v->num_states != 15 && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: num_states %d", v->num_states);
    if (v->compact && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: compact records with num_states %d", v->num_states);
    return QLE_OK;
}

// the first GPU call of an entry, behind its refusals
int use_device(const qle_device_view* v)
{
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(v->device));
    return QLE_OK;
}

inline dim3 tiles(const qle_device_view* v) { return dim3((unsigned)(v->padded_batch / kTile)); }
inline hipStream_t stream_of(const qle_device_view* v) { return (hipStream_t)v->stream; }

// a run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{}), and what it returns
template <typename F>
auto with(bool b, F&& f)
{
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// The [tiles][sums] partials of a batch summary: one buffer per (device, stream), grown on demand and kept -- two calls on one
// stream are ordered, two streams never share a buffer.  A cache for the life of the process, never destroyed: it keeps its own hipMalloc /
// hipFree instead of a DeviceMem (device_mem.hpp), which is what the device buffers of one *_host call are held by.
class Partials {
public:
    explicit Partials(int sums) : sums_(sums) {}
    int get(const qle_device_view* v, int64_t tiles, double** out)
    {
        std::lock_guard<std::mutex> lk(mu_);
        auto& slot = slots_[{v->device, v->stream}];
        if (slot.second < tiles) {
            if (slot.first) {
                HIP_TRY(hipStreamSynchronize(stream_of(v)));   // a launch that reads the old buffer may be in flight
                HIP_TRY(hipFree(slot.first));
                slot = {nullptr, 0};
            }
            double* buf = nullptr;
            HIP_TRY(hipMalloc(&buf, (size_t)tiles * sums_ * sizeof(double)));
            slot = {buf, tiles};
        }
        *out = slot.first;
        return QLE_OK;
    }

private:
    const int sums_;
    std::mutex mu_;
    std::map<std::pair<int, void*>, std::pair<double*, int64_t>> slots_;
};

}  // namespace
}  // namespace side
}  // namespace qle
