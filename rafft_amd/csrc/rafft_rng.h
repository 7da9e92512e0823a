// rafft_rng.h - the random numbers of rafft_sample_batch: Philox4x32-10 (Salmon, Moraes, Dror, Shaw:
// "Parallel random numbers: as easy as 1, 2, 3", SC 2011), counter based and stateless - a block of four 32-bit words is a pure
// function of (key, counter), nothing is stored per sample and no draw depends on another.  Plain C++ for host and device:
// tests/hostcheck/rng_check.cpp prints what the kernel computes.
//   key      the sequence's 64-bit seed (low word, high word)
//   counter  (sample index k, draw number t within the sample, 0, 0)
//   uniform  the upper 53 bits of (word 0 << 32 | word 1), times 2^-53: in [0, 1)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAFFT_RNG_FN __host__ __device__ inline
#else
#define RAFFT_RNG_FN inline
#endif

#define PHILOX_M0 0xD2511F53u       // the two multipliers of a round
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u       // the key's increments between rounds (golden ratio, sqrt(3) - 1)
#define PHILOX_W1 0xBB67AE85u

// out[0..3] = Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1)
RAFFT_RNG_FN void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// draw t of sample k under `seed`: 53 bits of the block, in [0, 1)
RAFFT_RNG_FN double rafft_uniform(uint64_t seed, uint32_t k, uint32_t t)
{
    uint32_t o[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), k, t, 0u, 0u, o);
    return (double)(((uint64_t)o[0] << 32 | o[1]) >> 11) * 0x1.0p-53;
}
