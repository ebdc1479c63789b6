// Stand-alone host build of rt_reject.hpp (tests/test_reject_sampler_host.py): classifies the candidates of a file with the header's
// own functions.  usage: reject_host K in.bin out.bin — in: n * K raw 64-bit draws (K = 3 unit sphere, 2 unit disk); out: n bytes of
// f32 verdicts, n bytes of exact verdicts, n * K doubles (the coordinates).
#include "rt_reject.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int K = std::atoi(argv[1]);
    if (K != 2 && K != 3) return 2;
    FILE *in = std::fopen(argv[2], "rb");
    if (!in) return 3;
    std::vector<uint64_t> w;
    uint64_t buf[4096];
    for (size_t got; (got = std::fread(buf, sizeof buf[0], 4096, in)) > 0;) w.insert(w.end(), buf, buf + got);
    std::fclose(in);
    const size_t n = w.size() / (size_t)K;
    std::vector<unsigned char> verdict(n), exact(n);
    std::vector<double> coords(n * (size_t)K);
    for (size_t c = 0; c < n; ++c) {
        const uint64_t *d = &w[c * (size_t)K];
        verdict[c] = (unsigned char)(K == 3 ? rtm::reject_sphere_f32(d[0], d[1], d[2]) : rtm::reject_disk_f32(d[0], d[1]));
        exact[c] = (K == 3 ? rtm::reject_sphere_exact(d[0], d[1], d[2]) : rtm::reject_disk_exact(d[0], d[1])) ? 1 : 0;
        for (int k = 0; k < K; ++k) coords[c * (size_t)K + (size_t)k] = rtm::reject_coord(d[k]);
    }
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 3;
    const bool ok = std::fwrite(verdict.data(), 1, n, out) == n && std::fwrite(exact.data(), 1, n, out) == n &&
                    std::fwrite(coords.data(), sizeof(double), coords.size(), out) == coords.size();
    return std::fclose(out) == 0 && ok ? 0 : 4;
}
