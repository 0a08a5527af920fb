// side_census_harness.cpp -- the launch census of quadrotor_landing_amd/csrc/side_host.hpp as a stand-alone host program (TEST ONLY).
//
// The header is compiled unmodified by a host compiler.  No kernel is launched and no GPU call is made: census_record is what launch()
// calls with a kernel's host handle, and here it is called with the addresses of exported functions of this program (linked with
// -rdynamic, so that dladdr names them as it names the host handles of a library's kernels).  Eight threads record three handles many
// times while the census is on; the list is then read by the two-call size protocol of <prefix>_launch_census_end.
//
//   side_census_harness        prints OK and returns 0, or says what is wrong and returns 1
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

// what ekf_layout.hpp (behind side_host.hpp) names of the device: stand-ins, as in stateio_harness.cpp; nothing here calls them
struct HarnessDim3 { unsigned x = 0, y = 0, z = 0; };
static HarnessDim3 blockIdx, gridDim, threadIdx, blockDim;
#define __builtin_amdgcn_readfirstlane(v) (v)

#include "../../quadrotor_landing_amd/csrc/side_host.hpp"

extern "C" void census_handle_b(void) {}
extern "C" void census_handle_a(void) {}
extern "C" void census_handle_c(void) {}

QLE_SIDE_LAST_ERROR(qxx_last_error)
QLE_SIDE_LAUNCH_CENSUS(qxx)

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::printf("line %d: %s (last error: %s)\n", __LINE__, #cond, qxx_last_error()); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main()
{
    using qle::side::census_record;
    const void* handles[3] = {(const void*)&census_handle_b, (const void*)&census_handle_a, (const void*)&census_handle_c};
    int64_t need = -1;
    // off: nothing is recorded, the list is empty ("" and its terminator)
    census_record(handles[0]);
    EXPECT(qxx_launch_census_end(nullptr, 0, &need) == QLE_OK && need == 1);
    // on, from eight threads
    EXPECT(qxx_launch_census_begin() == QLE_OK);
    std::vector<std::thread> pool;
    for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t] {
            for (int k = 0; k < 2000; ++k) census_record(handles[(k + t) % 3]);
        });
    for (std::thread& th : pool) th.join();
    EXPECT(qxx_launch_census_end(nullptr, 0, &need) == QLE_OK);
    const char want[] = "census_handle_a\ncensus_handle_b\ncensus_handle_c\n";
    EXPECT(need == (int64_t)sizeof(want));
    std::vector<char> exact((size_t)need), small((size_t)need - 1, 'x');
    EXPECT(qxx_launch_census_end(small.data(), need - 1, nullptr) == QLE_ERR_INVALID);   // one byte short: refused, nothing written
    EXPECT(small[0] == 'x' && std::strstr(qxx_last_error(), "bytes needed") != nullptr);
    EXPECT(qxx_launch_census_end(exact.data(), need, &need) == QLE_OK && std::memcmp(exact.data(), want, sizeof(want)) == 0);
    // the census is off behind end: a record is ignored and the list stays for another read
    census_record((const void*)&main);
    EXPECT(qxx_launch_census_end(exact.data(), need, &need) == QLE_OK && std::memcmp(exact.data(), want, sizeof(want)) == 0);
    // begin clears it
    EXPECT(qxx_launch_census_begin() == QLE_OK);
    census_record(handles[2]);
    EXPECT(qxx_launch_census_end(exact.data(), (int64_t)exact.size(), &need) == QLE_OK && std::strcmp(exact.data(), "census_handle_c\n") == 0);
    std::printf("OK\n");
    return 0;
}
