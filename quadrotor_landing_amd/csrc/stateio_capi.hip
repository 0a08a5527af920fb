// stateio_capi.hip -- C ABI of include/qle_stateio.h over ekf_stateio.hpp.  Host side: argument checks (every refusal before any GPU
// call) and ONE launch per call on the destination view's stream.  Works from the view struct of include/qle_ekf.h alone; links the HIP
// runtime only.  Allocates nothing: a snapshot goes into the caller's workspace (the host entry stages its host arrays through buffers
// of its own).
#include "../../include/qle_stateio.h"

#include "ekf_stateio.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QSI_F32 == QLE_F32 && QSI_F64 == QLE_F64, "the dtypes of the header");
static_assert(qsi::quads_of(kXW + kPW, 4) == qsi::kCopyBatch && qsi::quads_of(kXW + kPW, 8) == 2 * qsi::kCopyBatch, "k_si_copy: one batch of loads per fp32 record");

QLE_SIDE_LAST_ERROR(qsi_last_error)
QLE_SIDE_LAUNCH_COUNT(qsi_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qsi)

static int wsz(const qle_device_view* v) { return v->dtype == QLE_F64 ? 8 : 4; }
static int64_t state_bytes(const qle_device_view* v) { return v->padded_batch * (int64_t)kSW * wsz(v); }

// what every entry refuses about a view; no GPU call.  A view of exactly this library's size (a snapshot is a copy of it), with 16-byte
// aligned records of the length the layout gives them.
static int check_view(const qle_device_view* v)
{
    QLE_TRY(check_view(v, ViewSize::exact, true));
    const int words = v->compact ? kXW + kPWc : kXW + kPW;
    if (v->record_words != words) return fail(QLE_ERR_INVALID, "view: record_words %d (this library: %d for %s records)", v->record_words, words, v->compact ? "compact" : "full");
    return QLE_OK;
}

static bool overlap(const void* a, const void* b, int64_t bytes_a, int64_t bytes_b)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)bytes_b && b0 < a0 + (uintptr_t)bytes_a;
}

extern "C" int64_t qsi_workspace_bytes(const qle_device_view* view)
{
    QLE_TRY(check_view(view));
    return state_bytes(view);
}

// ------------------------------------------------------------------ pack
template <typename T, typename S>
static int launch_pack(const qle_device_view* v, const void* x, const void* P, const uint8_t* mask)
{
    auto go = [&](auto n, auto compact) {
        return launch(qsi::k_si_pack<T, S, decltype(n)::value, decltype(compact)::value>, tiles(v), dim3(kTile), 0, stream_of(v), (const S*)x, (const S*)P,
                      mask, (T*)v->state, v->batch);
    };
    if (v->compact) return go(std::integral_constant<int, 9>{}, std::true_type{});
    if (v->num_states == 9) return go(std::integral_constant<int, 9>{}, std::false_type{});
    return go(std::integral_constant<int, 15>{}, std::false_type{});
}

extern "C" int qsi_pack_state(const qle_device_view* view, const void* x, const void* P, int32_t src_dtype, const uint8_t* mask)
{
    QLE_TRY(check_view(view));
    if (src_dtype != QSI_F32 && src_dtype != QSI_F64) return fail(QLE_ERR_INVALID, "src_dtype must be QSI_F32 or QSI_F64 (got %d)", src_dtype);
    if (!x && !P) return fail(QLE_ERR_INVALID, "x and P are both null: nothing to write");
    if (!aligned(x, 16)) return fail(QLE_ERR_INVALID, "x must be 16-byte aligned");
    if (!aligned(P, 16)) return fail(QLE_ERR_INVALID, "P must be 16-byte aligned");
    QLE_TRY(use_device(view));
    const bool s64 = src_dtype == QSI_F64;
    if (view->dtype == QLE_F32) return s64 ? launch_pack<float, double>(view, x, P, mask) : launch_pack<float, float>(view, x, P, mask);
    return s64 ? launch_pack<double, double>(view, x, P, mask) : launch_pack<double, float>(view, x, P, mask);
}

// ------------------------------------------------------------------ copy
// Everything include/qle_stateio.h lists as refused, the views first; no GPU call.  host: index, mask and written are host arrays (no
// alignment to ask for).
static int check_copy(const qle_device_view* s, const qle_device_view* d, const int32_t* index, int32_t with_params, bool host)
{
    QLE_TRY(check_view(s));
    QLE_TRY(check_view(d));
    if (s->dtype != d->dtype) return fail(QLE_ERR_INVALID, "src and dst differ in dtype (%d, %d)", s->dtype, d->dtype);
    if (s->num_states != d->num_states) return fail(QLE_ERR_INVALID, "src and dst differ in num_states (%d, %d)", s->num_states, d->num_states);
    if ((s->compact != 0) != (d->compact != 0)) return fail(QLE_ERR_INVALID, "src and dst differ in compact (%d, %d)", s->compact, d->compact);
    if (s->device != d->device) return fail(QLE_ERR_INVALID, "src and dst are on different devices (%d, %d)", s->device, d->device);
    if (!index && s->batch != d->batch) return fail(QLE_ERR_INVALID, "src and dst differ in batch (%lld, %lld) and no index is given", (long long)s->batch, (long long)d->batch);
    if (!host && !aligned(index, 4)) return fail(QLE_ERR_INVALID, "index must be 4-byte aligned");
    if (overlap(s->state, d->state, state_bytes(s), state_bytes(d)))
        return fail(QLE_ERR_INVALID, index ? "src->state and dst->state overlap: an in-place permutation races, copy into a snapshot first"
                                           : "src->state and dst->state overlap: a copy never writes the records it reads");
    if (with_params) {
        if (!s->filter_params || !d->filter_params) return fail(QLE_ERR_INVALID, "with_params: %s has no filter_params", s->filter_params ? "dst" : "src");
        if (!aligned(s->filter_params, 16) || !aligned(d->filter_params, 16)) return fail(QLE_ERR_INVALID, "filter_params must be 16-byte aligned");
        if (overlap(s->filter_params, d->filter_params, s->padded_batch * (int64_t)kFW * wsz(s), d->padded_batch * (int64_t)kFW * wsz(d)))
            return fail(QLE_ERR_INVALID, "with_params: the filter_params of src and dst overlap");
    }
    return QLE_OK;
}

// the launch; the arguments are checked
static int run_copy(const qle_device_view* s, const qle_device_view* d, const int32_t* index, const uint8_t* mask, int32_t with_params, uint8_t* written)
{
    auto go = [&](auto rows, auto recq, auto parq) {
        return launch(qsi::k_si_copy<decltype(rows)::value, decltype(recq)::value, decltype(parq)::value>, tiles(d), dim3(kTile), 0, stream_of(d),
                      (const qsi::qsi_u4*)s->state, (qsi::qsi_u4*)d->state, index, mask, s->batch, d->batch,
                      (const qsi::qsi_u4*)(with_params ? s->filter_params : nullptr), (qsi::qsi_u4*)(with_params ? d->filter_params : nullptr), written);
    };
    using std::integral_constant;
    auto by_dtype = [&](auto w) {
        constexpr int W = decltype(w)::value;
        constexpr integral_constant<int, qsi::quads_of(kSW, W)> recq{};
        constexpr integral_constant<int, qsi::quads_of(kFW, W)> parq{};
        if (d->compact) return go(integral_constant<int, qsi::quads_of(kXW + kPWc, W)>{}, recq, parq);
        return go(integral_constant<int, qsi::quads_of(kXW + kPW, W)>{}, recq, parq);
    };
    if (d->dtype == QLE_F32) return by_dtype(integral_constant<int, 4>{});
    return by_dtype(integral_constant<int, 8>{});
}

extern "C" int qsi_copy(const qle_device_view* src, const qle_device_view* dst, const int32_t* index, const uint8_t* mask, int32_t with_params,
                        uint8_t* written)
{
    QLE_TRY(check_copy(src, dst, index, with_params, false));
    QLE_TRY(use_device(dst));
    return run_copy(src, dst, index, mask, with_params, written);
}

extern "C" int qsi_copy_host(const qle_device_view* src, const qle_device_view* dst, const int32_t* index, const uint8_t* mask, int32_t with_params,
                             uint8_t* written)
{
    QLE_TRY(check_copy(src, dst, index, with_params, true));
    QLE_TRY(use_device(dst));
    hipStream_t s = stream_of(dst);
    const size_t B = (size_t)dst->batch;
    DeviceMem own;
    void* d[3] = {};
    HIP_TRY(own.acquire({{d[0], index ? B * sizeof(int32_t) : 0}, {d[1], mask ? B : 0}, {d[2], written ? B : 0}}));
    if (index) HIP_TRY(hipMemcpyAsync(d[0], index, B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[1], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(run_copy(src, dst, (const int32_t*)d[0], (const uint8_t*)d[1], with_params, (uint8_t*)d[2]));
    if (written) HIP_TRY(hipMemcpyAsync(written, d[2], B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
