// Host-only check of the carried cell address of the regular state-only step (step_lean.h:
// ring_delta, ring_byte_deltas, ring_unindex_mul, ring_unindex; step_seq.h, step_group_ring<kAddr>)
// against the packed position it replaces (ring_bias, ring_index, a 16-bit packed add of the move).
//   The way back: for every W in 1 .. 256 and every index below 258 (W + 2), the most a bordered
//   table of that width holds (H <= 256), the multiply by ceil(2^32 / (W + 2)) and the product's
//   high word give index / (W + 2), and ring_unindex the biased position
//   index / (W + 2) | index % (W + 2) << 16.
//   The deltas: for every W, every cell (x, y) of a map 256 rows high and every one of the four
//   packed moves, ring_index of the packed add is ring_index of the cell plus ring_delta, and
//   ring_unindex takes the sum back to the packed target (on the border ring too). Up to W = 125,
//   where ring_byte_deltas says yes, the delta survives an int8; at W = 126 it says no, and the delta
//   of a move down the map, +128, does not survive.
//
//   hipcc -x hip --cuda-host-only -O2 -std=c++17 -ffp-contract=off -o step_addr_check tools/step_addr_check.cpp
//   ./step_addr_check   (prints the numbers of cases; exit status 1 on a mismatch)
// It may be built with -fsanitize=address,undefined as its own program.
//
// tests/test_step_addr_host.py builds and runs it (no GPU needed).
#include <cstdio>

#include "../shippingenv_amd/csrc/step_lean.h"

using namespace shipenv;

static uint32_t pk_add_u16(uint32_t a, uint32_t b) { return ((a + b) & 0xffffu) | ((((a >> 16) + (b >> 16)) & 0xffffu) << 16); }

int main() {
    // N, E, S, W as packed 16-bit (dx, dy), as the world image holds them
    const int mdx[4] = {0, -1, 0, 1}, mdy[4] = {-1, 0, 1, 0};
    uint32_t moves[4];
    for (int k = 0; k < 4; ++k) moves[k] = ((uint32_t)mdx[k] & 0xffffu) | (((uint32_t)mdy[k] & 0xffffu) << 16);
    long divisions = 0, targets = 0, byte_widths = 0;
    for (int W = 1; W <= 256; ++W) {
        const uint32_t S = (uint32_t)(W + 2), mul = ring_unindex_mul(W);
        for (uint32_t i = 0; i < 258u * S; ++i, ++divisions) {
            const uint32_t q = (uint32_t)(((uint64_t)i * mul) >> 32);
            if (q != i / S || ring_unindex(i, W, mul) != (i / S | (i % S) << 16)) {
                std::printf("ring_unindex: W %d index %u gives %u, %u / %u is %u\n", W, i, q, i, S, i / S);
                return 1;
            }
        }
        const bool bytes = ring_byte_deltas(W);
        if (bytes != (W <= 125)) {
            std::printf("ring_byte_deltas(%d) is %d\n", W, (int)bytes);
            return 1;
        }
        byte_widths += bytes;
        for (int k = 0; k < 4; ++k) {
            const int d = ring_delta(moves[k], W);
            if (d != mdx[k] * (W + 2) + mdy[k] || (bytes && (int)(int8_t)d != d) || (W == 126 && mdx[k] > 0 && (int)(int8_t)d == d)) {
                std::printf("ring_delta: W %d move %d gives %d\n", W, k, d);
                return 1;
            }
            for (uint32_t x = 0; x < 256; ++x)
                for (uint32_t y = 0; y < (uint32_t)W; ++y, ++targets) {
                    const uint32_t bp = ring_bias(x | (y << 16)), np = pk_add_u16(bp, moves[k]);
                    const uint32_t sum = ring_index(bp, W) + (uint32_t)(bytes ? (int)(int8_t)d : d);
                    if (sum != ring_index(np, W) || ring_unindex(sum, W, mul) != np || ring_unindex(ring_index(bp, W), W, mul) != bp) {
                        std::printf("delta: W %d cell (%u, %u) move %d: index %u, the packed add's %u\n", W, x, y, k, sum, ring_index(np, W));
                        return 1;
                    }
                }
        }
    }
    std::printf("step_addr_check: %ld divisions, %ld move targets, %ld widths with byte deltas, address == packed position\n", divisions, targets,
                byte_widths);
    return 0;
}
