#!/bin/bash
# CPU-only ThreadSanitizer run of the Poisson host tail (mpb_poisson_finish_host): two threads reach
# factorial_table() for the first time concurrently, as two contexts on two threads can.  The HIP kernels are
# not involved (GPU sanitizers are not available on this pool): the function lives in the HIP-free unit of the C ABI
# layer (mpb_hostonly.cpp), which is all this builds -- no HIP header, no HIP library, no stub.
set -e
cd "$(dirname "$0")/.."
D=${TMPDIR:-/tmp}/mpb_tsan; mkdir -p $D
cat > $D/main.cpp <<'CPP'
#include "moira_pb.h"
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>
int main()
{
    const int n = 2000;
    std::vector<double> lam(n), ee1(n), ee2(n);
    std::vector<int32_t> ns(n, 0);
    std::vector<uint8_t> p1(n), p2(n);
    for (int i = 0; i < n; i++) lam[i] = 0.05 * i;
    mpb_filter_params prm = {0.005, 0.01, NAN, MPB_AMBIG_IGNORE, 0};
    int rc1 = -1, rc2 = -1;
    std::thread a([&] { rc1 = mpb_poisson_finish_host(lam.data(), ns.data(), nullptr, 300, n, &prm, ee1.data(), p1.data()); });
    std::thread b([&] { rc2 = mpb_poisson_finish_host(lam.data(), ns.data(), nullptr, 300, n, &prm, ee2.data(), p2.data()); });
    a.join(); b.join();
    int same = 1;
    for (int i = 0; i < n; i++) same &= (ee1[i] == ee2[i]) || (std::isnan(ee1[i]) && std::isnan(ee2[i]));
    std::printf("tsan_poisson: rc %d %d, results identical: %d, ee[100] = %.17g\n", rc1, rc2, same, ee1[100]);
    return (rc1 || rc2 || !same) ? 1 : 0;
}
CPP
g++ -std=c++17 -O1 -g -fsanitize=thread -ffp-contract=off -pthread -Iinclude moira_amd/csrc/mpb_hostonly.cpp $D/main.cpp -o $D/tsan_poisson
TSAN_OPTIONS="halt_on_error=1" $D/tsan_poisson
