// consistency_capi.hip -- C ABI of include/qle_consistency.h over ekf_consistency.hpp.  Host side: argument checks (every refusal
// before any GPU call), the partials buffer of the batch summary, and the two launches on the view's stream.  Works from the view struct
// of include/qle_ekf.h and the public parameters; links libqle_ekf.so for qle_params_derive and derives the launch's parameter block
// as the handle does (ekf_params.hpp).
#include "../../include/qle_consistency.h"

#include <cmath>

#include "ekf_consistency.hpp"
#include "ekf_params.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(sizeof(qcs_summary) == kNeesSums * sizeof(double), "k_nees_reduce writes the summary as eight doubles");

QLE_SIDE_LAST_ERROR(qcs_last_error)
QLE_SIDE_LAUNCH_COUNT(qcs_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qcs)

// Everything include/qle_consistency.h lists as refused; no GPU call.  The view may be larger than this library's (a smaller one is
// refused).  host: the pointers are host arrays (no alignment to ask for, no dtypes).
static int check_args(const qle_device_view* v, const qle_params* p, const void* x_true, int32_t true_dtype, uint32_t blocks, double chi2_hi,
                      const void* nees, const void* err, const void* summary, int32_t dst_dtype, bool host)
{
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (!x_true) return fail(QLE_ERR_INVALID, "x_true is null");
    if (blocks == 0 || (blocks & ~kNeesAllBlocks)) return fail(QLE_ERR_INVALID, "blocks 0x%x: expected a non-empty selection of bits 0..4 (r, v, theta, ab, wb)", blocks);
    if (v->num_states == 9 && (blocks & ~7u)) return fail(QLE_ERR_INVALID, "blocks 0x%x selects a bias block, the handle has n = 9 states (est_bias = false)", blocks);
    if (!(chi2_hi > 0.0)) return fail(QLE_ERR_INVALID, "chi2_hi must be > 0 (got %g)", chi2_hi);
    if (true_dtype != QCS_F32 && true_dtype != QCS_F64) return fail(QLE_ERR_INVALID, "true_dtype must be QCS_F32 or QCS_F64 (got %d)", true_dtype);
    if (dst_dtype != QCS_F32 && dst_dtype != QCS_F64) return fail(QLE_ERR_INVALID, "dst_dtype must be QCS_F32 or QCS_F64 (got %d)", dst_dtype);
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (!host) {
        const uintptr_t w = dst_dtype == QCS_F64 ? 8 : 4;
        if (!aligned(x_true, 16)) return fail(QLE_ERR_INVALID, "x_true must be 16-byte aligned");
        if (!aligned(nees, w) || !aligned(err, w)) return fail(QLE_ERR_INVALID, "nees and err must be aligned to their element size");
        if (!aligned(summary, 8)) return fail(QLE_ERR_INVALID, "summary must be 8-byte aligned");
    }
    return QLE_OK;
}

static Partials g_partials(kNeesSums);   // the [tiles][8] partials of a summary

struct Call { const void* x_true; int32_t true_f64; const uint8_t* mask; uint32_t blocks; double chi2_hi; void* nees; void* err; double* summary; int32_t dst_f64; };

template <typename T>
static int launch_t(const qle_device_view* v, const qle_params& pub, const qle_derived& der, const Call& c)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    const int64_t tiles = v->padded_batch / kTile;
    double* partials = nullptr;
    if (c.summary) QLE_TRY(g_partials.get(v, tiles, &partials));
    const dim3 grid((unsigned)tiles), block(kTile);
    hipStream_t s = (hipStream_t)v->stream;
    auto go = [&](auto pfp, auto compact) {
        return launch(k_nees<T, decltype(pfp)::value, decltype(compact)::value>, grid, block, 0, s, (const T*)v->state, c.x_true, v->batch,
                      c.mask, (const T*)v->filter_params, c.nees, c.err, partials, c.blocks, v->num_states, c.true_f64, c.dst_f64, c.chi2_hi, dp);
    };
    QLE_TRY(with(v->filter_params != nullptr, [&](auto f) { return with(v->compact != 0, [&](auto k) { return go(f, k); }); }));
    if (c.summary) QLE_TRY(launch(k_nees_reduce, dim3(1), dim3(kBlock), 0, s, (const double*)partials, tiles, c.summary));
    return QLE_OK;
}

static int run(const qle_device_view* v, const qle_params* p, const Call& c)
{
    qle_derived der;
    if (qle_params_derive(p, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    if (!c.nees && !c.err && !c.summary) return QLE_OK;
    QLE_TRY(use_device(v));
    return v->dtype == QLE_F32 ? launch_t<float>(v, *p, der, c) : launch_t<double>(v, *p, der, c);
}

extern "C" int qcs_nees(const qle_device_view* view, const qle_params* params, const void* x_true, int32_t true_dtype, const uint8_t* mask,
                        uint32_t blocks, double chi2_hi, void* nees, void* err, qcs_summary* summary, int32_t dst_dtype)
{
    QLE_TRY(check_args(view, params, x_true, true_dtype, blocks, chi2_hi, nees, err, summary, dst_dtype, false));
    return run(view, params, Call{x_true, true_dtype == QCS_F64, mask, blocks, chi2_hi, nees, err, reinterpret_cast<double*>(summary), dst_dtype == QCS_F64});
}

extern "C" int qcs_nees_host(const qle_device_view* view, const qle_params* params, const double* x_true, const uint8_t* mask, uint32_t blocks,
                             double chi2_hi, double* nees, double* err, qcs_summary* summary)
{
    QLE_TRY(check_args(view, params, x_true, QCS_F64, blocks, chi2_hi, nees, err, summary, QCS_F64, true));
    if (!nees && !err && !summary) return QLE_OK;
    QLE_TRY(use_device(view));
    hipStream_t s = (hipStream_t)view->stream;
    const size_t B = (size_t)view->batch, n = (size_t)view->num_states;
    DeviceMem own;
    void* d[5] = {};
    HIP_TRY(own.acquire({{d[0], B * 16 * sizeof(double)}, {d[1], mask ? B : 0}, {d[2], nees ? B * sizeof(double) : 0}, {d[3], err ? B * n * sizeof(double) : 0},
                         {d[4], summary ? sizeof(qcs_summary) : 0}}));
    HIP_TRY(hipMemcpyAsync(d[0], x_true, B * 16 * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[1], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(run(view, params, Call{d[0], 1, (const uint8_t*)d[1], blocks, chi2_hi, d[2], d[3], (double*)d[4], 1}));
    if (nees) HIP_TRY(hipMemcpyAsync(nees, d[2], B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (err) HIP_TRY(hipMemcpyAsync(err, d[3], B * n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (summary) HIP_TRY(hipMemcpyAsync(summary, d[4], sizeof(qcs_summary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
