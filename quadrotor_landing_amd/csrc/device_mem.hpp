// device_mem.hpp -- what the host code of every library here shares (ekf_host.hpp for the tick library, side_host.hpp for the ones
// beside it): the two early-return macros and the one owner of device allocations.  Host code only, no symbol of its own: `fail` is
// whatever the including library defines (qle_fail, exported once for the tick library's translation units; an internal one per side
// library).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(QLE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define QLE_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != QLE_OK) return rc_; \
    } while (0)

#pragma GCC visibility push(hidden)   // no library exports these
namespace qle {

// One buffer of a group: the pointer field it is for, its size (0: no buffer, the field becomes null) and whether it starts zero-filled.
struct DevAlloc {
    void** field;
    size_t bytes;
    bool zero;
    template <typename T>
    DevAlloc(T*& f, size_t b, bool z = false) : field(reinterpret_cast<void**>(&f)), bytes(b), zero(z) {}
};

// Every hipMalloc result of one handle, sequence or call.  The fields the launchers read stay raw pointers; the owner sits beside them
// and is the only place that frees: a buffer cannot be allocated without being owned, so destroying the owner leaks nothing.
class DeviceMem {
public:
    DeviceMem() = default;
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { release_all(); }

    // A group, all or nothing: every buffer is allocated, the `zero` ones are cleared on `stream` (sync: and the stream is waited for),
    // and only then do the fields change -- a buffer a field pointed to before is freed, in the order of the list.  On an error nothing
    // is left behind and the fields, with what they point to, are as they were.
    hipError_t acquire(std::initializer_list<DevAlloc> group, hipStream_t stream = nullptr, bool sync = false)
    {
        const DevAlloc* g = group.begin();
        const int n = (int)group.size();
        long room = std::count(held_, held_ + kSlots, nullptr);   // the free slots and those of the buffers this group replaces
        for (int k = 0; k < n; ++k) room += *g[k].field && std::find(held_, held_ + kSlots, *g[k].field) != held_ + kSlots;
        if (n > room) return hipErrorOutOfMemory;   // kSlots is too small for what its user owns
        void* got[kSlots] = {};
        hipError_t e = hipSuccess;
        for (int k = 0; k < n && e == hipSuccess; ++k)
            if (g[k].bytes) e = hipMalloc(&got[k], g[k].bytes);
        for (int k = 0; k < n && e == hipSuccess; ++k)
            if (g[k].zero && got[k]) e = hipMemsetAsync(got[k], 0, g[k].bytes, stream);
        if (e == hipSuccess && sync) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            for (void* p : got) release(p, got);
            return e;
        }
        for (int k = 0; k < n; ++k) {
            release(*g[k].field, held_);
            *g[k].field = got[k];
            if (got[k]) *std::find(held_, held_ + kSlots, nullptr) = got[k];
        }
        return hipSuccess;
    }

    void release_all() { for (void* p : held_) release(p, held_); }

private:
    static constexpr int kSlots = 24;   // a handle with everything enabled holds 19 buffers
    // frees p if `list` holds it, and empties its slot
    static void release(void* p, void* (&list)[kSlots])
    {
        void** slot = std::find(list, list + kSlots, p);
        if (!p || slot == list + kSlots) return;
        (void)hipFree(p);
        *slot = nullptr;
    }
    void* held_[kSlots] = {};
};

}  // namespace qle
#pragma GCC visibility pop
