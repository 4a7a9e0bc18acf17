// Host-only check of philox.h's two-block draw (draw2 with pair_invariants) against philox10:
// for every (key, quad id, t) below, draw2's FUEL and GATE blocks must equal
// draw(k, t, kSlotFuel) and draw(k, t, kSlotGate) word for word. philox10 itself is first
// checked against Random123's published known-answer vectors for philox4x32-10.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -o philox_pair_check tools/philox_pair_check.cpp
//   ./philox_pair_check        (prints the number of tuples; exit status 1 on a mismatch)
//
// tests/test_philox_pair_host.py builds and runs it (no GPU needed).
#include <cstdio>
#include <cstring>

#include "../shippingenv_amd/csrc/philox.h"

using namespace shipenv;

static bool same(const U4& a, const U4& b) { return std::memcmp(a.v, b.v, sizeof a.v) == 0; }

int main() {
    // Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
    const uint32_t kat[3][10] = {
        {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu,
         0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu,
         0x5001e420u, 0x24126ea1u},
    };
    for (const auto& k : kat) {
        const U4 got = philox10(k[0], k[1], k[2], k[3], k[4], k[5]);
        if (!same(got, U4{{k[6], k[7], k[8], k[9]}})) {
            std::printf("philox10 misses a known-answer vector: %08x %08x %08x %08x\n", got.v[0], got.v[1], got.v[2],
                        got.v[3]);
            return 1;
        }
    }

    // seeds with a zero and a non-zero high word, and all-ones words
    const uint64_t seeds[] = {0ull, 22ull, 0xffffffffull, 1ull << 32, 0x9e3779b97f4a7c15ull, ~0ull};
    // quad ids below and beyond 2^32 (env_id_base >= 2^34 gives e1 != 0)
    const uint64_t quads[] = {0ull, 1ull, 255ull, 0xffffffffull, 1ull << 32, (1ull << 32) + 7, 1ull << 40,
                              0x0123456789abcdefull, ~0ull >> 2};
    // counters at both ends and across the 2^32 wrap
    const uint32_t ts[] = {0u, 1u, 2u, 33u, 1000u, 0x7fffffffu, 0x80000000u, 0xfffffffdu, 0xfffffffeu, 0xffffffffu};
    long checked = 0;
    uint64_t x = 0x2545f4914f6cdd1dull;  // xorshift64*: more tuples of all four kinds
    auto next = [&x] {
        x ^= x >> 12;
        x ^= x << 25;
        x ^= x >> 27;
        return x * 0x2545f4914f6cdd1dull;
    };
    auto check = [&checked](uint64_t seed, uint64_t quad, uint32_t t) {
        Key k;
        k.k0 = (uint32_t)seed;
        k.k1 = (uint32_t)(seed >> 32);
        k.e0 = (uint32_t)quad;
        k.e1 = (uint32_t)(quad >> 32);
        const PairInv inv = pair_invariants(k);
        const U4x2 got = draw2(k, inv, t);
        ++checked;
        if (same(got.fuel, draw(k, t, kSlotFuel)) && same(got.gate, draw(k, t, kSlotGate))) return true;
        std::printf("draw2 differs: seed %016llx quad %016llx t %08x\n", (unsigned long long)seed,
                    (unsigned long long)quad, t);
        return false;
    };
    for (uint64_t s : seeds)
        for (uint64_t q : quads)
            for (uint32_t t : ts)
                if (!check(s, q, t)) return 1;
    // a run that wraps t with the invariants of one quad, as the step loop uses them
    for (uint32_t i = 0; i < 40; ++i)
        if (!check(22ull, (1ull << 32) + 5, 0xffffffecu + i)) return 1;
    for (int i = 0; i < 4000; ++i) {
        const uint64_t s = (i & 1) ? next() : (uint32_t)next(), q = (i & 2) ? next() : (uint32_t)next();
        if (!check(s, q, (uint32_t)next())) return 1;
    }
    std::printf("philox_pair_check: %ld tuples, draw2 == philox10\n", checked);
    return 0;
}
