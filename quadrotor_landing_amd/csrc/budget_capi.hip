// budget_capi.hip -- C ABI of include/qle_budget.h over ekf_budget.hpp.  Host side: argument checks (every refusal before any GPU
// call), the [tiles][256] partials buffer, and the two launches on the view's stream.  Works from the view struct of include/qle_ekf.h
// and the public parameters; links libqle_ekf.so for qle_params_derive and derives the launch's parameter block as the handle does
// (ekf_params.hpp), as consistency_capi.hip.
#include "../../include/qle_budget.h"

#include <cmath>

#include "ekf_budget.hpp"
#include "ekf_params.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QBG_WORDS == kBudgetWords, "the header's word count is the kernels'");

QLE_SIDE_LAST_ERROR(qbg_last_error)
QLE_SIDE_LAUNCH_COUNT(qbg_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qbg)

extern "C" int64_t qbg_groups(int64_t batch, int64_t group_tiles)
{
    if (batch <= 0) return fail(QLE_ERR_INVALID, "batch %lld", (long long)batch);
    if (group_tiles < 0) return fail(QLE_ERR_INVALID, "group_tiles must be >= 0 (got %lld)", (long long)group_tiles);
    const int64_t tiles = padded_filters(batch) / kTile;
    return group_tiles == 0 ? 1 : (tiles + group_tiles - 1) / group_tiles;
}

// Everything include/qle_budget.h lists as refused; no GPU call.  The view may be larger than this library's (a smaller one is
// refused).  host: the pointers are host arrays (no alignment to ask for, no dtypes).
static int check_args(const qle_device_view* v, const qle_params* p, const void* x_true, int32_t true_dtype, int64_t true_rows, int64_t group_tiles,
                      const void* sums, const void* err, int32_t dst_dtype, bool host)
{
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (!x_true) return fail(QLE_ERR_INVALID, "x_true is null");
    if (!sums) return fail(QLE_ERR_INVALID, "sums is null");
    if (true_rows != 1 && true_rows != v->batch) return fail(QLE_ERR_INVALID, "true_rows must be 1 or the batch %lld (got %lld)", (long long)v->batch, (long long)true_rows);
    if (group_tiles < 0) return fail(QLE_ERR_INVALID, "group_tiles must be >= 0 (got %lld)", (long long)group_tiles);
    if (true_dtype != QBG_F32 && true_dtype != QBG_F64) return fail(QLE_ERR_INVALID, "true_dtype must be QBG_F32 or QBG_F64 (got %d)", true_dtype);
    if (dst_dtype != QBG_F32 && dst_dtype != QBG_F64) return fail(QLE_ERR_INVALID, "dst_dtype must be QBG_F32 or QBG_F64 (got %d)", dst_dtype);
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (!host) {
        if (!aligned(x_true, 16)) return fail(QLE_ERR_INVALID, "x_true must be 16-byte aligned");
        if (!aligned(sums, 8)) return fail(QLE_ERR_INVALID, "sums must be 8-byte aligned");
        if (!aligned(err, dst_dtype == QBG_F64 ? 8 : 4)) return fail(QLE_ERR_INVALID, "err must be aligned to its element size");
    }
    return QLE_OK;
}

static Partials g_partials(kBudgetWords);   // the [tiles][256] partials of a call

struct Call { const void* x_true; int32_t true_f64; int32_t truth_stride; const uint8_t* mask; int64_t group_tiles; double* sums; void* err; int32_t dst_f64; uint8_t* status; };

template <typename T>
static int launch_t(const qle_device_view* v, const qle_params& pub, const qle_derived& der, const Call& c)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    const int64_t tiles = v->padded_batch / kTile;
    const int64_t group_tiles = c.group_tiles == 0 ? tiles : c.group_tiles;
    const int64_t groups = (tiles + group_tiles - 1) / group_tiles;
    double* partials = nullptr;
    QLE_TRY(g_partials.get(v, tiles, &partials));
    hipStream_t s = stream_of(v);
    auto go = [&](auto pfp, auto compact) {
        return launch(k_budget<T, decltype(pfp)::value, decltype(compact)::value>, dim3((unsigned)tiles), dim3(kTile), 0, s, (const T*)v->state, c.x_true,
                      v->batch, c.mask, (const T*)v->filter_params, partials, c.err, c.status, c.truth_stride, v->num_states, c.true_f64, c.dst_f64, dp);
    };
    QLE_TRY(with(v->filter_params != nullptr, [&](auto f) { return with(v->compact != 0, [&](auto k) { return go(f, k); }); }));
    return launch(k_budget_reduce, dim3((unsigned)groups), dim3(kBlock), 0, s, (const double*)partials, tiles, group_tiles, c.sums);
}

static int run(const qle_device_view* v, const qle_params* p, const Call& c)
{
    qle_derived der;
    if (qle_params_derive(p, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    QLE_TRY(use_device(v));
    return v->dtype == QLE_F32 ? launch_t<float>(v, *p, der, c) : launch_t<double>(v, *p, der, c);
}

extern "C" int qbg_budget(const qle_device_view* view, const qle_params* params, const void* x_true, int32_t true_dtype, int64_t true_rows,
                          const uint8_t* mask, int64_t group_tiles, double* sums, void* err, int32_t dst_dtype, uint8_t* status)
{
    QLE_TRY(check_args(view, params, x_true, true_dtype, true_rows, group_tiles, sums, err, dst_dtype, false));
    return run(view, params, Call{x_true, true_dtype == QBG_F64, true_rows == view->batch ? 16 : 0, mask, group_tiles, sums, err, dst_dtype == QBG_F64, status});
}

extern "C" int qbg_budget_host(const qle_device_view* view, const qle_params* params, const double* x_true, int64_t true_rows, const uint8_t* mask,
                               int64_t group_tiles, double* sums, double* err, uint8_t* status)
{
    QLE_TRY(check_args(view, params, x_true, QBG_F64, true_rows, group_tiles, sums, err, QBG_F64, true));
    QLE_TRY(use_device(view));
    hipStream_t s = stream_of(view);
    const size_t B = (size_t)view->batch, n = (size_t)view->num_states, rows = (size_t)true_rows;
    const size_t sum_bytes = (size_t)qbg_groups(view->batch, group_tiles) * kBudgetWords * sizeof(double);
    DeviceMem own;
    void* d[5] = {};
    HIP_TRY(own.acquire({{d[0], rows * 16 * sizeof(double)}, {d[1], mask ? B : 0}, {d[2], sum_bytes}, {d[3], err ? B * n * sizeof(double) : 0}, {d[4], status ? B : 0}}));
    HIP_TRY(hipMemcpyAsync(d[0], x_true, rows * 16 * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[1], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(run(view, params, Call{d[0], 1, true_rows == view->batch ? 16 : 0, (const uint8_t*)d[1], group_tiles, (double*)d[2], d[3], 1, (uint8_t*)d[4]}));
    HIP_TRY(hipMemcpyAsync(sums, d[2], sum_bytes, hipMemcpyDeviceToHost, s));
    if (err) HIP_TRY(hipMemcpyAsync(err, d[3], B * n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, d[4], B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
