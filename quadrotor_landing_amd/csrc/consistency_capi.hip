// consistency_capi.hip -- C ABI of include/qle_consistency.h over ekf_consistency.hpp.  Host side: argument checks (every refusal
// before any GPU call), the partials buffer of the batch summary, and the two launches on the view's stream.  Works from the view struct
// of include/qle_ekf.h and the public parameters; links libqle_ekf.so for qle_params_derive and derives the launch's parameter block
// as the handle does (ekf_params.hpp).
#include "../../include/qle_consistency.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "ekf_consistency.hpp"
#include "ekf_params.hpp"

using namespace qle;

static_assert(sizeof(qcs_summary) == kNeesSums * sizeof(double), "k_nees_reduce writes the summary as eight doubles");

static thread_local std::string g_err;
static std::atomic<int64_t> g_launches{0};

static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(QLE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define QCS_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != QLE_OK) return rc_; \
    } while (0)

extern "C" const char* qcs_last_error(void) { return g_err.c_str(); }
extern "C" int64_t qcs_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Everything that can be refused, in the order include/qle_consistency.h lists it; no GPU call.  host: the pointers are host arrays
// (no alignment to ask for, no dtypes).
static int check_args(const qle_device_view* v, const qle_params* p, const void* x_true, int32_t true_dtype, uint32_t blocks, double chi2_hi,
                      const void* nees, const void* err, const void* summary, int32_t dst_dtype, bool host)
{
    if (!v) return fail(QLE_ERR_INVALID, "view is null");
    if (v->struct_size < sizeof(qle_device_view)) return fail(QLE_ERR_INVALID, "view: struct_size %u, this library was built for %zu", v->struct_size, sizeof(qle_device_view));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (!x_true) return fail(QLE_ERR_INVALID, "x_true is null");
    if (blocks == 0 || (blocks & ~kNeesAllBlocks)) return fail(QLE_ERR_INVALID, "blocks 0x%x: expected a non-empty selection of bits 0..4 (r, v, theta, ab, wb)", blocks);
    if (v->num_states != 15 && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: num_states %d", v->num_states);
    if (v->num_states == 9 && (blocks & ~7u)) return fail(QLE_ERR_INVALID, "blocks 0x%x selects a bias block, the handle has n = 9 states (est_bias = false)", blocks);
    if (!(chi2_hi > 0.0)) return fail(QLE_ERR_INVALID, "chi2_hi must be > 0 (got %g)", chi2_hi);
    if (true_dtype != QCS_F32 && true_dtype != QCS_F64) return fail(QLE_ERR_INVALID, "true_dtype must be QCS_F32 or QCS_F64 (got %d)", true_dtype);
    if (dst_dtype != QCS_F32 && dst_dtype != QCS_F64) return fail(QLE_ERR_INVALID, "dst_dtype must be QCS_F32 or QCS_F64 (got %d)", dst_dtype);
    if (v->dtype != QLE_F32 && v->dtype != QLE_F64) return fail(QLE_ERR_INVALID, "view: dtype %d", v->dtype);
    if (v->batch <= 0 || v->padded_batch != padded_filters(v->batch)) return fail(QLE_ERR_INVALID, "view: batch %lld / padded %lld", (long long)v->batch, (long long)v->padded_batch);
    if (!v->state || v->state_words != kSW) return fail(QLE_ERR_INVALID, "view: state records of %d words (this library: %d)", v->state_words, kSW);
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (v->compact && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: compact records with num_states %d", v->num_states);
    if (!host) {
        const uintptr_t w = dst_dtype == QCS_F64 ? 8 : 4;
        if (!aligned(x_true, 16)) return fail(QLE_ERR_INVALID, "x_true must be 16-byte aligned");
        if (!aligned(nees, w) || !aligned(err, w)) return fail(QLE_ERR_INVALID, "nees and err must be aligned to their element size");
        if (!aligned(summary, 8)) return fail(QLE_ERR_INVALID, "summary must be 8-byte aligned");
    }
    return QLE_OK;
}

// The [tiles][8] partials of a summary: one buffer per (device, stream), grown on demand and kept -- two calls on one stream are
// ordered, two streams never share a buffer.
static std::mutex g_mu;
static std::map<std::pair<int, void*>, std::pair<double*, int64_t>> g_partials;

static int partials_for(const qle_device_view* v, int64_t tiles, double** out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto& slot = g_partials[{v->device, v->stream}];
    if (slot.second < tiles) {
        if (slot.first) {
            HIP_TRY(hipStreamSynchronize((hipStream_t)v->stream));   // a launch that reads the old buffer may be in flight
            HIP_TRY(hipFree(slot.first));
            slot = {nullptr, 0};
        }
        double* buf = nullptr;
        HIP_TRY(hipMalloc(&buf, (size_t)tiles * kNeesSums * sizeof(double)));
        slot = {buf, tiles};
    }
    *out = slot.first;
    return QLE_OK;
}

struct Call { const void* x_true; int32_t true_f64; const uint8_t* mask; uint32_t blocks; double chi2_hi; void* nees; void* err; double* summary; int32_t dst_f64; };

template <typename T>
static int launch_t(const qle_device_view* v, const qle_params& pub, const qle_derived& der, const Call& c)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    const int64_t tiles = v->padded_batch / kTile;
    double* partials = nullptr;
    if (c.summary) QCS_TRY(partials_for(v, tiles, &partials));
    const dim3 grid((unsigned)tiles), block(kTile);
    hipStream_t s = (hipStream_t)v->stream;
    auto go = [&](auto pfp, auto compact) {
        hipLaunchKernelGGL((k_nees<T, decltype(pfp)::value, decltype(compact)::value>), grid, block, 0, s, (const T*)v->state, c.x_true, v->batch,
                           c.mask, (const T*)v->filter_params, c.nees, c.err, partials, c.blocks, v->num_states, c.true_f64, c.dst_f64, c.chi2_hi, dp);
    };
    auto with = [](bool b, auto&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); };
    with(v->filter_params != nullptr, [&](auto f) { with(v->compact != 0, [&](auto k) { go(f, k); }); });
    HIP_TRY(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);   // counts launches the runtime took, not attempts
    if (c.summary) {
        hipLaunchKernelGGL(k_nees_reduce, dim3(1), dim3(kBlock), 0, s, (const double*)partials, tiles, c.summary);
        HIP_TRY(hipGetLastError());
        g_launches.fetch_add(1, std::memory_order_relaxed);
    }
    return QLE_OK;
}

static int run(const qle_device_view* v, const qle_params* p, const Call& c)
{
    qle_derived der;
    if (qle_params_derive(p, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    if (!c.nees && !c.err && !c.summary) return QLE_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(v->device));
    return v->dtype == QLE_F32 ? launch_t<float>(v, *p, der, c) : launch_t<double>(v, *p, der, c);
}

extern "C" int qcs_nees(const qle_device_view* view, const qle_params* params, const void* x_true, int32_t true_dtype, const uint8_t* mask,
                        uint32_t blocks, double chi2_hi, void* nees, void* err, qcs_summary* summary, int32_t dst_dtype)
{
    QCS_TRY(check_args(view, params, x_true, true_dtype, blocks, chi2_hi, nees, err, summary, dst_dtype, false));
    return run(view, params, Call{x_true, true_dtype == QCS_F64, mask, blocks, chi2_hi, nees, err, reinterpret_cast<double*>(summary), dst_dtype == QCS_F64});
}

namespace {
// device buffers of one qcs_nees_host call, freed however the call ends
struct Staging {
    void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Staging() { for (void* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" int qcs_nees_host(const qle_device_view* view, const qle_params* params, const double* x_true, const uint8_t* mask, uint32_t blocks,
                             double chi2_hi, double* nees, double* err, qcs_summary* summary)
{
    QCS_TRY(check_args(view, params, x_true, QCS_F64, blocks, chi2_hi, nees, err, summary, QCS_F64, true));
    if (!nees && !err && !summary) return QLE_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(view->device));
    hipStream_t s = (hipStream_t)view->stream;
    const size_t B = (size_t)view->batch, n = (size_t)view->num_states;
    Staging d;
    HIP_TRY(hipMalloc(&d.p[0], B * 16 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d.p[0], x_true, B * 16 * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) {
        HIP_TRY(hipMalloc(&d.p[1], B));
        HIP_TRY(hipMemcpyAsync(d.p[1], mask, B, hipMemcpyHostToDevice, s));
    }
    if (nees) HIP_TRY(hipMalloc(&d.p[2], B * sizeof(double)));
    if (err) HIP_TRY(hipMalloc(&d.p[3], B * n * sizeof(double)));
    if (summary) HIP_TRY(hipMalloc(&d.p[4], sizeof(qcs_summary)));
    QCS_TRY(run(view, params, Call{d.p[0], 1, (const uint8_t*)d.p[1], blocks, chi2_hi, d.p[2], d.p[3], (double*)d.p[4], 1}));
    if (nees) HIP_TRY(hipMemcpyAsync(nees, d.p[2], B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (err) HIP_TRY(hipMemcpyAsync(err, d.p[3], B * n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (summary) HIP_TRY(hipMemcpyAsync(summary, d.p[4], sizeof(qcs_summary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
