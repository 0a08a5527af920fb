// stateio_harness.cpp -- host build of the index and packing arithmetic of quadrotor_landing_amd/csrc/ekf_stateio.hpp (TEST ONLY; the
// product has no CPU path).
//
// The header is compiled unmodified by a host compiler: the HIP headers define the device decorators away and the kernels themselves
// are behind the header's device guard.  The program walks every tile, pass, lane and piece of a ragged batch as k_si_pack and k_si_copy
// do, with the same calls (tile_valid, piece_word, piece_kind, pass_filters, cov_ab, pack_x_word, pack_cov_word, tile_word, copy_source,
// quad_at, quads_of), on heap arrays of exactly the sizes the kernels may touch -- B * W words on the AoS side, padded_batch records on
// the tile side -- so that a sanitizer build faults on any access outside them.  tests/test_stateio_cpu.py writes the input, and holds
// the WHOLE destination array (ragged tail and words >= record_words included) to a numpy restatement of off(w, i).
//
//   stateio_harness <in> <out>
// in  (doubles): B, mode, fp64, src_fp64, n, compact, src_B, use_index, use_x, use_P, then
//     mode 0 (pack): x [B][16], P [B][n][n], mask [B], the destination array before [padded B][144] in array order
//     mode 1 (copy): index [B], mask [B], the source array [padded src_B][144], the destination array before [padded B][144]
// out (doubles): the destination array after, in array order, then written [B] (pack: the lanes that were on)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct HarnessDim3 { unsigned x = 0, y = 0, z = 0; };
static HarnessDim3 blockIdx, gridDim, threadIdx, blockDim;
#define __builtin_amdgcn_readfirstlane(v) (v)

#include "../../quadrotor_landing_amd/csrc/ekf_stateio.hpp"
#include "harness_io.hpp"

using namespace qsi;

static const int kHdr = 10;
static int64_t padded(int64_t B) { return qle::padded_filters(B); }

// stage_span / stage_aos: the walk of a span of `span` words of which `valid` exist, in 16-byte pieces; lds_at(j) is where AoS word j lands
template <typename S, typename At>
static void stage(const S* src, int valid, int span, S* lds, At lds_at)
{
    const int V = 16 / (int)sizeof(S);
    for (int lane = 0; lane < kTile; ++lane)
        for (int k = 0; qdv::piece_word(0, k, V) < span; ++k) {
            const int j = qdv::piece_word(lane, k, V);
            if (j >= span) break;
            const int kind = qdv::piece_kind(j, V, valid);
            for (int e = 0; e < V; ++e)
                if (kind == 2 || (kind == 1 && j + e < valid)) lds[lds_at(j + e)] = src[j + e];
        }
}

template <typename T, typename S>
static void pack(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0], Bp = padded(B);
    const int n = (int)h[4], NN = n * n;
    const bool compact = h[5] != 0, use_x = h[8] != 0, use_P = h[9] != 0;
    const int V = 16 / (int)sizeof(T);
    // the AoS side: exactly B rows, on the heap
    S* x = (S*)std::malloc((size_t)B * kXW * sizeof(S));
    S* P = (S*)std::malloc((size_t)B * NN * sizeof(S));
    uint8_t* mask = (uint8_t*)std::malloc((size_t)B);
    T* st = (T*)std::malloc((size_t)Bp * kSW * sizeof(T));
    for (int64_t k = 0; k < B * kXW; ++k) x[k] = (S)d[k];
    d += B * kXW;
    for (int64_t k = 0; k < B * NN; ++k) P[k] = (S)d[k];
    d += B * NN;
    for (int64_t k = 0; k < B; ++k) mask[k] = d[k] != 0;
    d += B;
    for (int64_t k = 0; k < Bp * kSW; ++k) st[k] = (T)d[k];
    const int FPB = pass_filters<S>(n);
    const int lds_words = FPB * NN > kTile * kPitchX ? FPB * NN : kTile * kPitchX;
    S* lds = (S*)std::malloc((size_t)lds_words * sizeof(S));
    for (int64_t tile = 0; tile < Bp / kTile; ++tile) {
        const int nv = qdv::tile_valid(B, tile);
        T* tb = st + qdv::tile_base(tile, kSW);
        auto on = [&](int lane) { return lane < nv && mask[tile * kTile + lane] != 0; };
        for (int lane = 0; lane < nv; ++lane) out[Bp * kSW + tile * kTile + lane] = on(lane);
        if (use_x) {
            stage<S>(x + tile * (kTile * kXW), nv * kXW, kTile * kXW, lds, [](int j) { const int f = qdv::aos_filter(j, kXW); return qdv::lds_word(f, j - f * kXW, kPitchX); });
            for (int lane = 0; lane < kTile; ++lane)
                if (on(lane))
                    for (int k = 0; k < kXW / V; ++k)
                        for (int e = 0; e < V; ++e) tb[qdv::tile_word<T>(k * V, lane, kSW) + e] = pack_x_word<T, S>(lds[qdv::lds_word(lane, k * V + e, kPitchX)]);
        }
        if (!use_P) continue;
        for (int f0 = 0; f0 < nv; f0 += FPB) {
            const int nvp = nv - f0 < FPB ? nv - f0 : FPB;
            stage<S>(P + (tile * kTile + f0) * NN, nvp * NN, FPB * NN, lds, [](int j) { return j; });
            for (int lane = f0; lane < f0 + FPB; ++lane)
                if (on(lane))
                    for (int k = 0; k < cov_words(compact) / V; ++k)
                        for (int e = 0; e < V; ++e) {
                            const CovAB ab = cov_ab(k * V + e, compact);
                            tb[qdv::tile_word<T>((kXW / V + k) * V, lane, kSW) + e] = pack_cov_word<T, S>(lds + (lane - f0) * NN, ab.a, ab.b, n);
                        }
        }
    }
    for (int64_t k = 0; k < Bp * kSW; ++k) out[k] = (double)st[k];
    std::free(x); std::free(P); std::free(mask); std::free(st); std::free(lds);
}

template <typename T>
static void copy(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0], Bp = padded(B), sB = (int64_t)h[6], sBp = padded(sB);
    const bool compact = h[5] != 0, use_index = h[7] != 0;
    int32_t* index = (int32_t*)std::malloc((size_t)B * sizeof(int32_t));
    uint8_t* mask = (uint8_t*)std::malloc((size_t)B);
    T* src = (T*)std::malloc((size_t)sBp * kSW * sizeof(T));
    T* dst = (T*)std::malloc((size_t)Bp * kSW * sizeof(T));
    for (int64_t k = 0; k < B; ++k) index[k] = (int32_t)d[k];
    d += B;
    for (int64_t k = 0; k < B; ++k) mask[k] = d[k] != 0;
    d += B;
    for (int64_t k = 0; k < sBp * kSW; ++k) src[k] = (T)d[k];
    d += sBp * kSW;
    for (int64_t k = 0; k < Bp * kSW; ++k) dst[k] = (T)d[k];
    const int rows = quads_of(compact ? kXW + kPWc : kXW + kPW, (int)sizeof(T)), recq = quads_of(kSW, (int)sizeof(T));
    for (int64_t i = 0; i < Bp; ++i) {   // every lane of every tile, the ones beyond the batch included
        const int64_t j = copy_source(i, B, use_index ? index : nullptr, mask, sB);
        if (i < B) out[Bp * kSW + i] = j >= 0;
        if (j < 0) continue;
        for (int k = 0; k < rows; ++k)
            std::memcpy((char*)dst + (quad_at(i, 0, recq) + (int64_t)k * kTile) * kQuadBytes, (const char*)src + (quad_at(j, 0, recq) + (int64_t)k * kTile) * kQuadBytes, kQuadBytes);
    }
    for (int64_t k = 0; k < Bp * kSW; ++k) out[k] = (double)dst[k];
    std::free(index); std::free(mask); std::free(src); std::free(dst);
}

int main(int argc, char** argv)
{
    return harness_main(
        argc, argv, kHdr,
        [](const double* h) { return (h[0] < 1 || (h[4] != 15 && h[4] != 9) || (h[5] != 0 && h[4] != 9) || h[6] < 1) ? 7 : 0; },
        [](const double* h) {
            const int64_t B = (int64_t)h[0], n = (int64_t)h[4];
            return h[1] == 0 ? (size_t)(B * (kXW + n * n + 1) + padded(B) * kSW) : (size_t)(2 * B + (padded((int64_t)h[6]) + padded(B)) * kSW);
        },
        [](const double* h) { return (size_t)(padded((int64_t)h[0]) * kSW + (int64_t)h[0]); },
        [](const double* h, const double* d, double* out) {
            const bool pack_mode = h[1] == 0, sf64 = h[3] != 0;
            by_dtype(h[2] != 0, [&](auto t) {
                using T = decltype(t);
                if (!pack_mode) copy<T>(h, d, out);
                else if (sf64) pack<T, double>(h, d, out);
                else pack<T, float>(h, d, out);
            });
        });
}
