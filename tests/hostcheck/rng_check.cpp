// rng_check - prints what rafft_rng.h computes on the host, for tests/test_sample_host.py to compare with its own restatement.
// stdin: lines "key k t" (decimal).  stdout, per line: the four words of the Philox block of counter (k, t, 0, 0) under `key`, in
// hex, and the 53 bits of the uniform as an integer (uniform * 2^53); a line "raw k0 k1 c0 c1 c2 c3" prints the block of any counter.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../rafft_amd/csrc/rafft_rng.h"

int main()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        uint32_t o[4];
        if (!strncmp(line, "raw ", 4)) {
            uint32_t v[6];
            if (sscanf(line + 4, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) return 2;
            philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5], o);
            printf("%08x %08x %08x %08x\n", o[0], o[1], o[2], o[3]);
            continue;
        }
        uint64_t key;
        uint32_t k, t;
        if (sscanf(line, "%" SCNu64 " %" SCNu32 " %" SCNu32, &key, &k, &t) != 3) return 2;
        philox4x32_10((uint32_t)key, (uint32_t)(key >> 32), k, t, 0u, 0u, o);
        const double u = rafft_uniform(key, k, t);
        if (!(u >= 0.0 && u < 1.0)) return 3;
        printf("%08x %08x %08x %08x %.0f\n", o[0], o[1], o[2], o[3], u * 9007199254740992.0);
    }
    return 0;
}
