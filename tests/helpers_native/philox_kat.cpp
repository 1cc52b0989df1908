// Host program for tests/test_hap_sample_rules.py: nanosnp_amd/csrc/nsnp_philox.hpp compiled by the host compiler under
// -fsanitize=address,undefined.  Arguments: groups of six hex words c0 c1 c2 c3 k0 k1; per group one line with the four output words of
// Philox4x32-10 and the multiply-shift index of word 0 into a list of 0x9e3779b1 entries.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nsnp_philox.hpp"

int main(int argc, char** argv)
{
    if (argc < 7 || (argc - 1) % 6 != 0) {
        std::fprintf(stderr, "usage: philox_kat (c0 c1 c2 c3 k0 k1)+   hex words\n");
        return 2;
    }
    std::vector<uint32_t> w;
    for (int i = 1; i < argc; ++i) w.push_back((uint32_t)std::strtoul(argv[i], nullptr, 16));
    for (size_t g = 0; g + 6 <= w.size(); g += 6) {
        const nsnp_philox4 o = nsnp_philox4x32_10(w[g], w[g + 1], w[g + 2], w[g + 3], w[g + 4], w[g + 5]);
        std::printf("%08x %08x %08x %08x %llu\n", o.v[0], o.v[1], o.v[2], o.v[3], (unsigned long long)nsnp_philox_index(o.v[0], 0x9e3779b1u));
    }
    return 0;
}
