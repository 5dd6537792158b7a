// per_pow_host.cpp -- csrc/per_pow.hpp compiled for the host, for tests/test_per_pow_host.py.
//
//   per_pow_host IN OUT      IN: (x, y) pairs as raw little-endian doubles;  OUT: per pair the double libm_pow wrote (0 when
//                            the pair is outside the covered range) and a 64-bit flag, 1 = covered
//
// Build as the Makefile's PER_FLAGS say: -ffp-contract=off, and hardware fused multiply-add for every fma() (-mfma on x86-64).
#define PER_POW_TABLE static
#define PER_POW_FN
#include "../../trajtrack_mpcndqn_rlboost_amd/csrc/per_pow.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    std::vector<double> xy;
    double pair[2];
    while (fread(pair, sizeof(double), 2, in) == 2) { xy.push_back(pair[0]); xy.push_back(pair[1]); }
    fclose(in);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    for (size_t i = 0; i + 1 < xy.size(); i += 2) {
        double v = 0.0;
        const uint64_t ok = pergpu::libm_pow(xy[i], xy[i + 1], &v) ? 1 : 0;
        if (!ok) v = 0.0;
        if (fwrite(&v, sizeof v, 1, out) != 1 || fwrite(&ok, sizeof ok, 1, out) != 1) { perror(argv[2]); return 2; }
    }
    return fclose(out) == 0 ? 0 : 2;
}
