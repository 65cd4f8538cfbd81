// CPU run of the prime kernels' lane code (heartbeat_amd/csrc/hb_prime.hpp),
// built with AddressSanitizer and UBSan by tests/test_prime_emul.py.
//
// Reads vectors from the file named on the command line, one per line, and
// prints one result per line:
//   T <NL> <n hex> <a hex> <base2 0|1> <maxbits>   -> hb_sprp_lane: 0 | 1
//   K <NL> <start hex> <q decimal>                 -> hb_sieve_first_k
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "hb_prime.hpp"

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

template <int NL>
static bool parse(const char *hex, u32 out[NL]) {
    for (int t = 0; t < NL; ++t) out[t] = 0;
    const size_t n = strlen(hex);
    if (n == 0 || n > 8u * NL) return false;
    for (size_t k = 0; k < n; ++k) {
        const int v = hexval(hex[n - 1 - k]);
        if (v < 0) return false;
        out[k / 8] |= (u32)v << (4 * (k % 8));
    }
    return true;
}

template <int NL>
static int run_test(const char *n_hex, const char *a_hex, int base2, unsigned maxbits) {
    u32 n[NL], a[NL];
    if (!parse<NL>(n_hex, n) || !parse<NL>(a_hex, a)) return -1;
    return hb_sprp_lane<NL>(n, a, base2 != 0, maxbits) ? 1 : 0;
}

template <int NL>
static long run_first_k(const char *s_hex, unsigned q) {
    u32 s[NL];
    if (!parse<NL>(s_hex, s)) return -1;
    return (long)hb_sieve_first_k<NL>(s, q);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    std::vector<char> line(4096), f1(1100), f2(1100);
    while (fgets(line.data(), (int)line.size(), fh)) {
        char kind = 0;
        int nl = 0;
        if (sscanf(line.data(), " %c %d", &kind, &nl) != 2) continue;
        long r = -1;
        if (kind == 'T') {
            int base2 = 0;
            unsigned maxbits = 0;
            if (sscanf(line.data(), " %*c %*d %1024s %1024s %d %u", f1.data(), f2.data(), &base2, &maxbits) != 4) return 3;
            switch (nl) {
            case 2: r = run_test<2>(f1.data(), f2.data(), base2, maxbits); break;
            case 8: r = run_test<8>(f1.data(), f2.data(), base2, maxbits); break;
            case 16: r = run_test<16>(f1.data(), f2.data(), base2, maxbits); break;
            case 32: r = run_test<32>(f1.data(), f2.data(), base2, maxbits); break;
            case 64: r = run_test<64>(f1.data(), f2.data(), base2, maxbits); break;
            default: return 3;
            }
        } else if (kind == 'K') {
            unsigned q = 0;
            if (sscanf(line.data(), " %*c %*d %1024s %u", f1.data(), &q) != 2) return 3;
            switch (nl) {
            case 2: r = run_first_k<2>(f1.data(), q); break;
            case 8: r = run_first_k<8>(f1.data(), q); break;
            case 16: r = run_first_k<16>(f1.data(), q); break;
            case 32: r = run_first_k<32>(f1.data(), q); break;
            case 64: r = run_first_k<64>(f1.data(), q); break;
            default: return 3;
            }
        } else {
            return 3;
        }
        if (r < 0) return 4;
        printf("%ld\n", r);
    }
    fclose(fh);
    return 0;
}
