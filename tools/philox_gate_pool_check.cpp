// Host-only check of philox.h's single-block draws from a quad's exchanged words, as the
// state-only step's GATE pool uses them (step_seq.h): for every (key, quad id, t, offset) below,
//   draw_gate_pooled(k0, k1, gate_seed(k, inv), t + offset) == draw(k, t + offset, kSlotGate)
//   draw_fuel(k, inv, t + offset)                           == draw(k, t + offset, kSlotFuel)
// word for word, with the counter's sum wrapping 2^32 as the kernel's does. The GateSeed is
// first copied through a plain array of four words, as it travels through LDS, and drawn under
// another quad's Key object: nothing but the four words and the seed may enter the block.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -o philox_gate_pool_check tools/philox_gate_pool_check.cpp
//   ./philox_gate_pool_check   (prints the number of tuples; exit status 1 on a mismatch)
//
// tests/test_philox_gate_pool_host.py builds and runs it (no GPU needed).
#include <cstdio>
#include <cstring>

#include "../shippingenv_amd/csrc/philox.h"

using namespace shipenv;

static bool same(const U4& a, const U4& b) { return std::memcmp(a.v, b.v, sizeof a.v) == 0; }

static Key key_of(uint64_t seed, uint64_t quad) {
    Key k;
    k.k0 = (uint32_t)seed;
    k.k1 = (uint32_t)(seed >> 32);
    k.e0 = (uint32_t)quad;
    k.e1 = (uint32_t)(quad >> 32);
    return k;
}

int main() {
    // seeds with a zero and a non-zero high word, and all-ones words
    const uint64_t seeds[] = {0ull, 22ull, 0xffffffffull, 1ull << 32, 0x9e3779b97f4a7c15ull, ~0ull};
    // quad ids below and beyond 2^32 (env_id_base >= 2^34 gives e1 != 0), both sides of an e1 step
    const uint64_t quads[] = {0ull, 1ull, 255ull, 0xffffffffull, 1ull << 32, (1ull << 32) + 7, (1ull << 32) - 32, 1ull << 40,
                              0x0123456789abcdefull, ~0ull >> 2};
    // window starts at both ends and such that start + offset wraps 2^32 inside a window of 8
    const uint32_t ts[] = {0u, 1u, 33u, 1000u, 0x7fffffffu, 0x80000000u, 0xfffffff8u, 0xfffffff9u, 0xfffffffdu, 0xffffffffu};
    long checked = 0, e1_nonzero = 0, wrapped = 0;
    uint64_t x = 0x2545f4914f6cdd1dull;  // xorshift64*
    auto next = [&x] {
        x ^= x >> 12;
        x ^= x << 25;
        x ^= x >> 27;
        return x * 0x2545f4914f6cdd1dull;
    };
    auto check = [&](uint64_t seed, uint64_t quad, uint32_t t, uint32_t off) {
        const Key k = key_of(seed, quad);
        const PairInv inv = pair_invariants(k);
        const GateSeed g = gate_seed(k, inv);
        uint32_t row[4] = {g.c3, g.hi, g.lo, g.e1};  // the LDS row
        const Key other = key_of(seed, quad ^ 0x5a5a5a5a00000001ull);  // the drawing lane's own quad
        const uint32_t tc = t + off;  // wraps as the kernel's counter does
        const U4 gate = draw_gate_pooled(other.k0, other.k1, GateSeed{row[0], row[1], row[2], row[3]}, tc);
        const U4 fuel = draw_fuel(k, inv, tc);
        ++checked;
        e1_nonzero += k.e1 != 0;
        wrapped += tc < t;
        if (same(gate, draw(k, tc, kSlotGate)) && same(fuel, draw(k, tc, kSlotFuel))) return true;
        std::printf("pooled draw differs: seed %016llx quad %016llx t %08x offset %u\n", (unsigned long long)seed,
                    (unsigned long long)quad, t, off);
        return false;
    };
    for (uint64_t s : seeds)
        for (uint64_t q : quads)
            for (uint32_t t : ts)
                for (uint32_t off = 0; off < 8; ++off)
                    if (!check(s, q, t, off)) return 1;
    // the window of the GPU suite: t = 2^32 - 3 .. 2^32 + 4, quads either side of e1 0 -> 1
    for (uint64_t q = (1ull << 32) - 32; q < (1ull << 32) + 32; ++q)
        for (uint32_t off = 0; off < 8; ++off)
            if (!check(22ull, q, 0xfffffffdu, off)) return 1;
    for (int i = 0; i < 4000; ++i) {
        const uint64_t s = (i & 1) ? next() : (uint32_t)next(), q = (i & 2) ? next() : (uint32_t)next();
        if (!check(s, q, (uint32_t)next(), (uint32_t)next() & 7u)) return 1;
    }
    if (e1_nonzero < 1000 || wrapped < 100) {
        std::printf("coverage: %ld tuples with e1 != 0, %ld with a wrapped counter\n", e1_nonzero, wrapped);
        return 1;
    }
    std::printf("philox_gate_pool_check: %ld tuples (%ld with e1 != 0, %ld with t + offset past 2^32), pooled == philox10\n",
                checked, e1_nonzero, wrapped);
    return 0;
}
